"""ctypes binding of include/efe_engine.h.  There is NO fallback: if the HIP library is missing the
import fails loudly (the product path never routes through the CPU oracle)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EFE_LIB_PATH') or os.path.join(HERE, 'libefe_mi355x.so')    # override: A/B of kernel builds

EXPORTS = ['efe_create', 'efe_destroy', 'efe_last_error', 'efe_abi_version', 'efe_set_weight', 'efe_commit_weights',
           'efe_set_option', 'efe_transition', 'efe_decoder', 'efe_encoder', 'efe_habit', 'efe_calculate_g',
           'efe_rollout', 'efe_trajectory', 'efe_simulate', 'efe_action_posterior', 'efe_last_call_macs',
           'efe_prof_enable', 'efe_prof_classes', 'efe_prof_read', 'efe_env_reset', 'efe_env_step', 'efe_env_render',
           'efe_check_reward', 'efe_reparameterize', 'efe_mcts_select', 'efe_mcts_expand', 'efe_mcts_backprop', 'efe_mcts_stop',
           'efe_build_id', 'efe_reserve', 'efe_rollout_scratch_bytes', 'efe_arena_stats', 'efe_env_new_image', 'efe_create_cfg', 'efe_get_config', 'efe_get_device', 'efe_ctx_alive',
           'efe_calculate_g_rows', 'efe_simulate_rows', 'efe_mcts_step',
           'efe_free_energy', 'efe_loss_top', 'efe_loss_mid', 'efe_loss_down',
           'efe_param_count', 'efe_get_weights', 'efe_top_grad', 'efe_adam_step', 'efe_train_top',
           'efe_mid_grad', 'efe_train_mid', 'efe_dec_tail_grad', 'efe_dec_grad', 'efe_enc_grad', 'efe_down_grad',
           'efe_train_down', 'efe_down_adam_step', 'efe_down_get_weights', 'efe_train_step', 'efe_eval_stats',
           'efe_encoder_rows', 'efe_rollout_rows', 'efe_agent_need', 'efe_agent_choose', 'efe_agent_enqueue', 'efe_agent_act',
           'efe_agent_mcts_root', 'efe_agent_mcts_enqueue', 'efe_eval_mi',
           'efe_agent_trace_tick', 'efe_agent_trace_decision', 'efe_agent_plan_mask', 'efe_agent_view']
ABI_VERSION = 6


class EfeMctsTree(C.Structure):
    _fields_ = [('W', C.c_void_p), ('N', C.c_void_p), ('Qpi', C.c_void_p), ('child', C.c_void_p), ('S', C.c_void_p),
                ('E', C.c_int32), ('cap', C.c_int32), ('A', C.c_int32), ('s_dim', C.c_int32)]


class EfeAgent(C.Structure):
    _fields_ = [('queue', C.c_void_p), ('head', C.c_void_p), ('len', C.c_void_p), ('crossings', C.c_void_p), ('reward_sum', C.c_void_p),
                ('E', C.c_int32), ('cap', C.c_int32)]


EFE_AGENT_AI, EFE_AGENT_T1, EFE_AGENT_T12, EFE_AGENT_PROBS = 0, 1, 2, 3
EFE_AGENT_NONE = -1

# efe_agent_trace (include/efe_engine.h): the arrays of the record in struct order, then T, E, Lp
TRACE_FIELDS = ('state', 'last_r', 'action', 'queue_len', 'decided', 'choice', 'u', 'G', 'terms', 'probs', 'path', 'path_len')


class EfeAgentTrace(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in TRACE_FIELDS] + [('T', C.c_int32), ('E', C.c_int32), ('Lp', C.c_int32)]


class EfeNoise(C.Structure):
    _fields_ = [('seed', C.c_uint64), ('stage', C.c_uint32), ('pass_', C.c_uint32), ('sample', C.c_uint32),
                ('row_offset', C.c_uint32)]


EFE_OMEGA_ARRAY, EFE_OMEGA_SCALAR, EFE_OMEGA_DERIVED = 0, 1, 2


class EfeFeParams(C.Structure):
    _fields_ = [('gamma', C.c_float), ('beta_s', C.c_float), ('beta_o', C.c_float), ('omega_mode', C.c_int32),
                ('omega', C.c_void_p), ('omega_scalar', C.c_float), ('a', C.c_float), ('b', C.c_float), ('c', C.c_float),
                ('d', C.c_float)]


FE_OUT_FIELDS = ('F_top', 'kl_pi', 'kl_pi_anal', 'Qpi', 'omega', 'F_mid', 'kl_s_mid', 'kl_s_mid_anal', 'ps1', 'ps1_mean', 'ps1_logvar',
                 'F_down', 'nlogpo1', 'kl_s', 'kl_s_anal', 'kl_naive', 'kl_naive_anal', 'po1', 'qs1', 's0', 'qs1_mean', 'qs1_logvar')


class EfeAdamParams(C.Structure):
    _fields_ = [('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('step', C.c_int64)]


class EfeFeOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in FE_OUT_FIELDS]


# efe_train_step (include/efe_engine.h): its inputs, one part's optimiser state + hyper-parameters, its outputs
EFE_STEP_MEANS = 8
STEP_MEANS_FIELDS = ('kl_pi', 'omega', 'F_mid', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'omega_std')
STEP_OUT_FIELDS = ('kl_pi', 'omega', 'qs0', 'F_mid', 'ps1_mean', 'ps1_logvar', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'means')


# efe_eval_stats (include/efe_engine.h): the row of the epoch report, its input arrays in struct order, then Mr
EFE_EVAL_STATS, EFE_EVAL_MAX_ROWS = 98, 8192
EVAL_IN_FIELDS = ('F_top', 'F_mid', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'kl_pi', 'kl_s_anal', 'kl_naive_anal', 'kl_pi_anal', 'qs1', 's0',
                  'S_real', 'o1_r', 'po1_r')


class EfeEvalIn(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in EVAL_IN_FIELDS] + [('Mr', C.c_int32)]


# efe_eval_mi (include/efe_engine.h): the [60] table of mutual-information scores, latent-major
EFE_EVAL_MI, EFE_EVAL_MI_MAX_NEIGHBORS = 60, 4
EVAL_MI_IN_FIELDS = ('s0', 'S_real', 'noise', 'n_neighbors', 'seed', 'stage')


class EfeEvalMiIn(C.Structure):
    _fields_ = [('s0', C.c_void_p), ('S_real', C.c_void_p), ('noise', C.c_void_p), ('n_neighbors', C.c_int32), ('seed', C.c_uint64),
                ('stage', C.c_uint32)]


class EfeStepIn(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ('o0', 'o1', 'pi0', 'log_Ppi', 'eps')]


class EfeStepAdam(C.Structure):
    _fields_ = [('exp_avg', C.c_void_p), ('exp_avg_sq', C.c_void_p), ('hp', EfeAdamParams)]


class EfeStepOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in STEP_OUT_FIELDS]


_lib = None
_ops = None
OPS_PATH = os.path.join(HERE, 'libefe_torch_ops.so')


def load_ops():
    """torch.ops.efe -- the custom-op registration library (csrc/torch_ops.cpp) over the C ABI.  Loud if missing or stale."""
    global _ops
    if _ops is not None:
        return _ops
    load()                                    # the engine library first (same checks), so the ops library resolves against it
    import torch
    from . import build as _build
    if not os.path.exists(OPS_PATH):
        raise ImportError(f'{OPS_PATH} not built: run `python -c "import __graft_entry__ as g; g.build()"`')
    want, have = _build.ops_digest(), _build._stamp(OPS_PATH, 'EFE_OPS_BUILD_ID')
    if want != have:
        raise ImportError(f'{OPS_PATH} is stale: built from sources {have}, the sources here are {want}; re-run build()')
    torch.ops.load_library(OPS_PATH)
    try:        # one engine copy in the process: the ops library must have resolved to the library ctypes loaded (A/B runs with EFE_LIB_PATH)
        mapped = {line.split()[-1] for line in open('/proc/self/maps') if 'libefe_mi355x' in line or os.path.basename(LIB_PATH) in line}
        engines = {m for m in mapped if os.path.realpath(m) != os.path.realpath(OPS_PATH)}
    except OSError:
        engines = set()
    if len({os.path.realpath(m) for m in engines}) > 1:
        raise ImportError(f'two engine libraries are mapped ({sorted(engines)}): libefe_torch_ops.so did not resolve to {LIB_PATH}; '
                          'rebuild the override with build.py (it sets the SONAME libefe_mi355x.so)')
    _ops = torch.ops.efe
    return _ops


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} not built: run `python -c "import __graft_entry__ as g; g.build()"` '
                          '(hipcc --offload-arch=gfx950); there is no CPU fallback')
    # RTLD_GLOBAL + the library's SONAME (build.py): when libefe_torch_ops.so is loaded later, its DT_NEEDED libefe_mi355x.so resolves
    # to THIS copy even if EFE_LIB_PATH points somewhere else -- the context and every hot-path op then run the same build
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    lib.efe_abi_version.argtypes = []; lib.efe_abi_version.restype = C.c_int
    if lib.efe_abi_version() != ABI_VERSION:
        raise ImportError(f'{LIB_PATH}: ABI version {lib.efe_abi_version()} != {ABI_VERSION} (stale build: re-run build())')
    lib.efe_build_id.argtypes = []; lib.efe_build_id.restype = C.c_char_p
    if not os.environ.get('EFE_LIB_PATH'):
        # a shipped binary must come from the sources next to it: compare the digest compiled into it
        from . import build as _build
        want, have = _build.source_digest(), lib.efe_build_id().decode()
        if want != have:
            raise ImportError(f'{LIB_PATH} is stale: built from sources {have}, the sources here are {want}; '
                              're-run `python -c "import __graft_entry__ as g; g.build()"`')
    p, i, f32p = C.c_void_p, C.c_int, C.c_void_p
    nzp = C.POINTER(EfeNoise)
    lib.efe_create.argtypes = [C.POINTER(p), i]; lib.efe_create.restype = i
    lib.efe_get_config.argtypes = [p, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]; lib.efe_get_config.restype = i
    lib.efe_get_device.argtypes = [p, C.POINTER(i), C.c_char_p, i]; lib.efe_get_device.restype = i
    lib.efe_create_cfg.argtypes = [C.POINTER(p), i, i, i, i, i]; lib.efe_create_cfg.restype = i
    lib.efe_destroy.argtypes = [p]; lib.efe_destroy.restype = None
    lib.efe_last_error.argtypes = [p]; lib.efe_last_error.restype = C.c_char_p
    lib.efe_set_weight.argtypes = [p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), i]; lib.efe_set_weight.restype = i
    lib.efe_commit_weights.argtypes = [p]; lib.efe_commit_weights.restype = i
    lib.efe_set_option.argtypes = [p, C.c_char_p, C.c_int64]; lib.efe_set_option.restype = i
    lib.efe_transition.argtypes = [p, f32p, f32p, i, nzp, f32p, f32p, f32p, f32p, p]; lib.efe_transition.restype = i
    lib.efe_decoder.argtypes = [p, f32p, i, nzp, f32p, p]; lib.efe_decoder.restype = i
    lib.efe_encoder.argtypes = [p, f32p, i, nzp, f32p, f32p, f32p, f32p, p]; lib.efe_encoder.restype = i
    lib.efe_habit.argtypes = [p, f32p, i, f32p, f32p, f32p, p]; lib.efe_habit.restype = i
    lib.efe_calculate_g.argtypes = [p, f32p, f32p, i, i, i, nzp, f32p, f32p, f32p, f32p, f32p, f32p, f32p, p]
    lib.efe_calculate_g.restype = i
    lib.efe_rollout.argtypes = [p, f32p, f32p, i, i, i, i, i, nzp, f32p, f32p, f32p, f32p, p]; lib.efe_rollout.restype = i
    lib.efe_trajectory.argtypes = [p, f32p, f32p, f32p, f32p, f32p, i, nzp, f32p, f32p, p]; lib.efe_trajectory.restype = i
    lib.efe_simulate.argtypes = [p, f32p, i, i, i, nzp, f32p, f32p, f32p, f32p, f32p, p]; lib.efe_simulate.restype = i
    lib.efe_reserve.argtypes = [p, C.c_int64]; lib.efe_reserve.restype = i
    lib.efe_ctx_alive.argtypes = [p]; lib.efe_ctx_alive.restype = i
    lib.efe_rollout_scratch_bytes.argtypes = [p, i, i, i]; lib.efe_rollout_scratch_bytes.restype = C.c_int64
    lib.efe_arena_stats.argtypes = [p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]; lib.efe_arena_stats.restype = i
    lib.efe_env_new_image.argtypes = [p, f32p, i, nzp, p]; lib.efe_env_new_image.restype = i
    lib.efe_action_posterior.argtypes = [p, f32p, i, i, C.c_float, f32p, f32p, p]; lib.efe_action_posterior.restype = i
    lib.efe_last_call_macs.argtypes = [p]; lib.efe_last_call_macs.restype = C.c_int64
    lib.efe_prof_enable.argtypes = [p, i]; lib.efe_prof_enable.restype = i
    lib.efe_prof_classes.argtypes = []; lib.efe_prof_classes.restype = i
    lib.efe_prof_read.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]; lib.efe_prof_read.restype = i
    lib.efe_env_reset.argtypes = [p, f32p, f32p, i, nzp, p]; lib.efe_env_reset.restype = i
    lib.efe_env_step.argtypes = [p, f32p, f32p, C.c_void_p, i, i, nzp, C.c_void_p, p]; lib.efe_env_step.restype = i
    lib.efe_env_render.argtypes = [p, f32p, f32p, C.c_void_p, C.c_int64, f32p, C.c_void_p, i, p]; lib.efe_env_render.restype = i
    lib.efe_check_reward.argtypes = [p, f32p, i, f32p, p]; lib.efe_check_reward.restype = i
    lib.efe_reparameterize.argtypes = [p, f32p, f32p, i, i, nzp, f32p, f32p, p]; lib.efe_reparameterize.restype = i
    tp = C.POINTER(EfeMctsTree)
    lib.efe_mcts_select.argtypes = [p, tp, p, C.c_float, i, i, p, p, p, p, f32p, f32p, p]; lib.efe_mcts_select.restype = i
    lib.efe_mcts_expand.argtypes = [p, tp, p, p, p, f32p, f32p, p]; lib.efe_mcts_expand.restype = i
    lib.efe_mcts_backprop.argtypes = [p, tp, p, p, p, p, p, f32p, i, f32p, i, f32p, p, p]; lib.efe_mcts_backprop.restype = i
    lib.efe_mcts_stop.argtypes = [p, tp, p, p, i, C.c_float, p, p]; lib.efe_mcts_stop.restype = i
    lib.efe_mcts_step.argtypes = [p, tp, p, p, f32p, i, f32p, f32p, p, p, p, i, C.c_float, p, C.c_float, i, i, p, p, p, p, f32p, f32p, p, f32p, f32p, p]; lib.efe_mcts_step.restype = i
    fpp, fop = C.POINTER(EfeFeParams), C.POINTER(EfeFeOut)
    lib.efe_free_energy.argtypes = [p, f32p, f32p, f32p, f32p, i, fpp, nzp, f32p, fop, p]; lib.efe_free_energy.restype = i
    lib.efe_loss_top.argtypes = [p, f32p, f32p, i, fop, p]; lib.efe_loss_top.restype = i
    lib.efe_loss_mid.argtypes = [p, f32p, f32p, f32p, f32p, i, fpp, nzp, f32p, fop, p]; lib.efe_loss_mid.restype = i
    lib.efe_loss_down.argtypes = [p, f32p, f32p, f32p, i, fpp, nzp, f32p, fop, p]; lib.efe_loss_down.restype = i
    ap = C.POINTER(EfeAdamParams)
    lib.efe_param_count.argtypes = [p, C.c_char_p]; lib.efe_param_count.restype = C.c_int64
    lib.efe_get_weights.argtypes = [p, C.c_char_p, f32p, C.c_int64, p]; lib.efe_get_weights.restype = i
    lib.efe_top_grad.argtypes = [p, f32p, f32p, i, f32p, f32p, p]; lib.efe_top_grad.restype = i
    lib.efe_adam_step.argtypes = [p, C.c_char_p, f32p, f32p, f32p, ap, p]; lib.efe_adam_step.restype = i
    lib.efe_train_top.argtypes = [p, f32p, f32p, i, f32p, f32p, f32p, ap, p]; lib.efe_train_top.restype = i
    lib.efe_mid_grad.argtypes = [p, f32p, f32p, f32p, f32p, i, fpp, nzp, f32p, f32p, f32p, f32p, p]; lib.efe_mid_grad.restype = i
    lib.efe_train_mid.argtypes = [p, f32p, f32p, f32p, f32p, i, fpp, nzp, f32p, f32p, f32p, f32p, f32p, ap, p]; lib.efe_train_mid.restype = i
    lib.efe_dec_tail_grad.argtypes = [p, f32p, f32p, i, C.c_float, C.c_float, f32p, f32p, f32p, f32p, f32p, f32p, f32p, p]; lib.efe_dec_tail_grad.restype = i
    lib.efe_dec_grad.argtypes = [p, f32p, f32p, i, C.c_float, C.c_float, C.POINTER(EfeNoise)] + [f32p] * 11 + [p]; lib.efe_dec_grad.restype = i
    lib.efe_enc_grad.argtypes = [p, f32p, f32p, f32p, i, nzp] + [f32p] * 10 + [p]; lib.efe_enc_grad.restype = i
    lib.efe_down_grad.argtypes = [p, f32p, f32p, f32p, i, fpp, nzp, f32p, fop, f32p, f32p, f32p, p]; lib.efe_down_grad.restype = i
    lib.efe_train_down.argtypes = [p, f32p, f32p, f32p, i, fpp, nzp, f32p, fop, f32p, f32p, ap, p]; lib.efe_train_down.restype = i
    lib.efe_down_adam_step.argtypes = [p, f32p, f32p, f32p, ap, p]; lib.efe_down_adam_step.restype = i
    lib.efe_down_get_weights.argtypes = [p, f32p, C.c_int64, p]; lib.efe_down_get_weights.restype = i
    sap = C.POINTER(EfeStepAdam)
    lib.efe_train_step.argtypes = [p, C.POINTER(EfeStepIn), i, fpp, nzp, sap, sap, sap, C.POINTER(EfeStepOut), p]; lib.efe_train_step.restype = i
    lib.efe_eval_stats.argtypes = [p, C.POINTER(EfeEvalIn), i, f32p, p]; lib.efe_eval_stats.restype = i
    lib.efe_eval_mi.argtypes = [p, C.POINTER(EfeEvalMiIn), i, f32p, p, p]; lib.efe_eval_mi.restype = i
    lib.efe_encoder_rows.argtypes = [p, f32p, i, nzp, f32p, p, f32p, f32p, f32p, p]; lib.efe_encoder_rows.restype = i
    lib.efe_rollout_rows.argtypes = [p, f32p, f32p, i, i, i, i, i, nzp, f32p, p, f32p, f32p, f32p, p]; lib.efe_rollout_rows.restype = i
    agp = C.POINTER(EfeAgent)
    lib.efe_agent_need.argtypes = [p, agp, p, p, p]; lib.efe_agent_need.restype = i
    lib.efe_agent_choose.argtypes = [p, agp, p, i, i, f32p, f32p, f32p, i, C.c_float, i, nzp, f32p, p, f32p, p]; lib.efe_agent_choose.restype = i
    lib.efe_agent_enqueue.argtypes = [p, agp, p, i, p, p, i, i, p]; lib.efe_agent_enqueue.restype = i
    lib.efe_agent_act.argtypes = [p, agp, f32p, f32p, nzp, p, p]; lib.efe_agent_act.restype = i
    lib.efe_agent_mcts_root.argtypes = [p, agp, p, i, f32p, i, i, C.c_float, i, i, nzp, f32p, p, p, p, f32p, p]; lib.efe_agent_mcts_root.restype = i
    lib.efe_agent_mcts_enqueue.argtypes = [p, agp, C.POINTER(EfeMctsTree), p, i, p, i, i, p, p, p]; lib.efe_agent_mcts_enqueue.restype = i
    trp = C.POINTER(EfeAgentTrace)
    lib.efe_agent_trace_tick.argtypes = [p, agp, trp, i, f32p, f32p, p]; lib.efe_agent_trace_tick.restype = i
    lib.efe_agent_trace_decision.argtypes = [p, trp, i, p, i, i, p, f32p, f32p, f32p, f32p, i, C.c_float, p, p, i, p]; lib.efe_agent_trace_decision.restype = i
    lib.efe_agent_plan_mask.argtypes = [p, p, i, i, f32p, p, p, p, i, i, i, i, i, f32p, p]; lib.efe_agent_plan_mask.restype = i
    lib.efe_agent_view.argtypes = [p, f32p, f32p, p, i, i, p, p]; lib.efe_agent_view.restype = i
    _lib = lib
    return lib
