"""ctypes binding of include/efe_engine.h.  There is NO fallback: if the HIP library is missing the
import fails loudly (the product path never routes through the CPU oracle)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EFE_LIB_PATH') or os.path.join(HERE, 'libefe_mi355x.so')    # override: A/B of kernel builds

ABI_VERSION = 6


def ptr(t):
    """the address of a tensor's data as the C ABI takes it; None is NULL"""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class EfeRows(C.Structure):
    _fields_ = [('mask', C.c_void_p), ('ids', C.c_void_p), ('rows_per_entry', C.c_int32), ('n_total', C.c_int32)]


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


class EfeEvalMiIn(C.Structure):
    _fields_ = [('s0', C.c_void_p), ('S_real', C.c_void_p), ('noise', C.c_void_p), ('n_neighbors', C.c_int32), ('seed', C.c_uint64),
                ('stage', C.c_uint32)]


EVAL_MI_IN_FIELDS = tuple(f for f, _ in EfeEvalMiIn._fields_)


class EfeStepIn(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ('o0', 'o1', 'pi0', 'log_Ppi', 'eps')]


class EfeStepAdam(C.Structure):
    _fields_ = [('exp_avg', C.c_void_p), ('exp_avg_sq', C.c_void_p), ('hp', EfeAdamParams)]


class EfeStepOut(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in STEP_OUT_FIELDS]


# the struct of include/efe_engine.h each class above mirrors (tests/test_abi.py compiles the header and compares every size and offset)
STRUCTS = {'efe_rows': EfeRows, 'efe_noise': EfeNoise, 'efe_agent': EfeAgent, 'efe_mcts_tree': EfeMctsTree, 'efe_agent_trace': EfeAgentTrace,
           'efe_fe_params': EfeFeParams, 'efe_fe_out': EfeFeOut, 'efe_adam_params': EfeAdamParams, 'efe_step_in': EfeStepIn,
           'efe_step_adam': EfeStepAdam, 'efe_step_out': EfeStepOut, 'efe_eval_in': EfeEvalIn, 'efe_eval_mi_in': EfeEvalMiIn}

# Every prototype of include/efe_engine.h as name: (restype, argtypes), in the header's order; load() applies it and tests/test_abi.py holds
# it to the header argument by argument.  _p: the context, the stream and every device or host array; a struct pointer is POINTER(its mirror).
_p, _i, _f, _l, _s = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_char_p
_nz, _rows, _ag, _tp, _tr = C.POINTER(EfeNoise), C.POINTER(EfeRows), C.POINTER(EfeAgent), C.POINTER(EfeMctsTree), C.POINTER(EfeAgentTrace)
_fp, _fo, _ap, _sa = C.POINTER(EfeFeParams), C.POINTER(EfeFeOut), C.POINTER(EfeAdamParams), C.POINTER(EfeStepAdam)
_ip, _lp = C.POINTER(C.c_int), C.POINTER(C.c_int64)
SIGNATURES = {
    'efe_create': (_i, (C.POINTER(_p), _i)),
    'efe_create_cfg': (_i, (C.POINTER(_p), _i, _i, _i, _i, _i)),
    'efe_get_config': (_i, (_p, _ip, _ip, _ip, _ip)),
    'efe_get_device': (_i, (_p, _ip, _s, _i)),
    'efe_destroy': (None, (_p,)),
    'efe_last_error': (_s, (_p,)),
    'efe_ctx_alive': (_i, (_p,)),
    'efe_abi_version': (_i, ()),
    'efe_build_id': (_s, ()),
    'efe_set_weight': (_i, (_p, _s, _p, _lp, _i)),
    'efe_commit_weights': (_i, (_p,)),
    'efe_set_option': (_i, (_p, _s, _l)),
    'efe_reserve': (_i, (_p, _l)),
    'efe_rollout_scratch_bytes': (_l, (_p, _i, _i, _i)),
    'efe_arena_stats': (_i, (_p, _lp, _lp, _lp)),
    'efe_transition': (_i, (_p, _p, _p, _i, _nz, _p, _p, _p, _p, _p)),
    'efe_decoder': (_i, (_p, _p, _i, _nz, _p, _p)),
    'efe_encoder': (_i, (_p, _p, _i, _nz, _p, _p, _p, _p, _p)),
    'efe_encoder_rows': (_i, (_p, _p, _i, _nz, _p, _rows, _p, _p, _p, _p)),
    'efe_habit': (_i, (_p, _p, _i, _p, _p, _p, _p)),
    'efe_check_reward': (_i, (_p, _p, _i, _p, _p)),
    'efe_reparameterize': (_i, (_p, _p, _p, _i, _i, _nz, _p, _p, _p)),
    'efe_calculate_g': (_i, (_p, _p, _p, _i, _i, _i, _nz, _p, _p, _p, _p, _p, _p, _p, _p)),
    'efe_calculate_g_rows': (_i, (_p, _p, _p, _i, _i, _i, _nz, _p, _rows, _p, _p, _p, _p, _p, _p, _p)),
    'efe_rollout': (_i, (_p, _p, _p, _i, _i, _i, _i, _i, _nz, _p, _p, _p, _p, _p)),
    'efe_rollout_rows': (_i, (_p, _p, _p, _i, _i, _i, _i, _i, _nz, _p, _rows, _p, _p, _p, _p)),
    'efe_trajectory': (_i, (_p, _p, _p, _p, _p, _p, _i, _nz, _p, _p, _p)),
    'efe_simulate': (_i, (_p, _p, _i, _i, _i, _nz, _p, _p, _p, _p, _p, _p)),
    'efe_simulate_rows': (_i, (_p, _p, _i, _i, _i, _nz, _p, _p, _rows, _p, _p, _p, _p)),
    'efe_action_posterior': (_i, (_p, _p, _i, _i, _f, _p, _p, _p)),
    'efe_env_reset': (_i, (_p, _p, _p, _i, _nz, _p)),
    'efe_env_new_image': (_i, (_p, _p, _i, _nz, _p)),
    'efe_env_step': (_i, (_p, _p, _p, _p, _i, _i, _nz, _p, _p)),
    'efe_env_render': (_i, (_p, _p, _p, _p, _l, _p, _p, _i, _p)),
    'efe_agent_need': (_i, (_p, _ag, _p, _p, _p)),
    'efe_agent_choose': (_i, (_p, _ag, _p, _i, _i, _p, _p, _p, _i, _f, _i, _nz, _p, _p, _p, _p)),
    'efe_agent_enqueue': (_i, (_p, _ag, _p, _i, _p, _p, _i, _i, _p)),
    'efe_agent_act': (_i, (_p, _ag, _p, _p, _nz, _p, _p)),
    'efe_mcts_step': (_i, (_p, _tp, _p, _p, _p, _i, _p, _p, _p, _p, _p, _i, _f, _p, _f, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p)),
    'efe_mcts_select': (_i, (_p, _tp, _p, _f, _i, _i, _p, _p, _p, _p, _p, _p, _p)),
    'efe_mcts_expand': (_i, (_p, _tp, _p, _p, _p, _p, _p, _p)),
    'efe_mcts_backprop': (_i, (_p, _tp, _p, _p, _p, _p, _p, _p, _i, _p, _i, _p, _p, _p)),
    'efe_mcts_stop': (_i, (_p, _tp, _p, _p, _i, _f, _p, _p)),
    'efe_agent_mcts_root': (_i, (_p, _ag, _p, _i, _p, _i, _i, _f, _i, _i, _nz, _p, _p, _p, _p, _p, _p)),
    'efe_agent_mcts_enqueue': (_i, (_p, _ag, _tp, _p, _i, _p, _i, _i, _p, _p, _p)),
    'efe_agent_trace_tick': (_i, (_p, _ag, _tr, _i, _p, _p, _p)),
    'efe_agent_trace_decision': (_i, (_p, _tr, _i, _p, _i, _i, _p, _p, _p, _p, _p, _i, _f, _p, _p, _i, _p)),
    'efe_agent_plan_mask': (_i, (_p, _p, _i, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p)),
    'efe_agent_view': (_i, (_p, _p, _p, _p, _i, _i, _p, _p)),
    'efe_free_energy': (_i, (_p, _p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p)),
    'efe_loss_top': (_i, (_p, _p, _p, _i, _fo, _p)),
    'efe_loss_mid': (_i, (_p, _p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p)),
    'efe_loss_down': (_i, (_p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p)),
    'efe_param_count': (_l, (_p, _s)),
    'efe_get_weights': (_i, (_p, _s, _p, _l, _p)),
    'efe_top_grad': (_i, (_p, _p, _p, _i, _p, _p, _p)),
    'efe_adam_step': (_i, (_p, _s, _p, _p, _p, _ap, _p)),
    'efe_train_top': (_i, (_p, _p, _p, _i, _p, _p, _p, _ap, _p)),
    'efe_mid_grad': (_i, (_p, _p, _p, _p, _p, _i, _fp, _nz, _p, _p, _p, _p, _p)),
    'efe_train_mid': (_i, (_p, _p, _p, _p, _p, _i, _fp, _nz, _p, _p, _p, _p, _p, _ap, _p)),
    'efe_dec_tail_grad': (_i, (_p, _p, _p, _i, _f, _f) + (_p,) * 8),
    'efe_dec_tail_grad_g': (_i, (_p, _p, _p, _i, _f, _f) + (_p,) * 8),
    'efe_dec_grad': (_i, (_p, _p, _p, _i, _f, _f, _nz) + (_p,) * 12),
    'efe_dec_grad_g': (_i, (_p, _p, _p, _i, _f, _f, _nz) + (_p,) * 12),
    'efe_enc_grad': (_i, (_p, _p, _p, _p, _i, _nz) + (_p,) * 11),
    'efe_down_grad': (_i, (_p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p, _p, _p, _p)),
    'efe_enc_grad_g': (_i, (_p, _p, _p, _p, _i, _nz) + (_p,) * 11),
    'efe_down_grad_g': (_i, (_p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p, _p, _p, _p)),
    'efe_train_down': (_i, (_p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p, _p, _ap, _p)),
    'efe_down_adam_step': (_i, (_p, _p, _p, _p, _ap, _p)),
    'efe_down_get_weights': (_i, (_p, _p, _l, _p)),
    'efe_train_down_g': (_i, (_p, _p, _p, _p, _i, _fp, _nz, _p, _fo, _p, _p, _ap, _p)),
    'efe_down_adam_step_g': (_i, (_p, _p, _p, _p, _ap, _p)),
    'efe_down_get_weights_g': (_i, (_p, _p, _l, _p)),
    'efe_train_step': (_i, (_p, C.POINTER(EfeStepIn), _i, _fp, _nz, _sa, _sa, _sa, C.POINTER(EfeStepOut), _p)),
    'efe_eval_stats': (_i, (_p, C.POINTER(EfeEvalIn), _i, _p, _p)),
    'efe_eval_mi': (_i, (_p, C.POINTER(EfeEvalMiIn), _i, _p, _p, _p)),
    'efe_last_call_macs': (_l, (_p,)),
    'efe_prof_enable': (_i, (_p, _i)),
    'efe_prof_classes': (_i, ()),
    'efe_prof_read': (_i, (_p, C.POINTER(C.c_double), _lp)),
}
EXPORTS = list(SIGNATURES)


def _declare(lib, names):
    for n in names:
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = SIGNATURES[n]


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
    _declare(lib, ('efe_abi_version', 'efe_build_id'))        # what the two checks below call; the rest once the library is known to be this ABI
    if lib.efe_abi_version() != ABI_VERSION:
        raise ImportError(f'{LIB_PATH}: ABI version {lib.efe_abi_version()} != {ABI_VERSION} (stale build: re-run build())')
    if not os.environ.get('EFE_LIB_PATH'):
        # a shipped binary must come from the sources next to it: compare the digest compiled into it
        from . import build as _build
        want, have = _build.source_digest(), lib.efe_build_id().decode()
        if want != have:
            raise ImportError(f'{LIB_PATH} is stale: built from sources {have}, the sources here are {want}; '
                              're-run `python -c "import __graft_entry__ as g; g.build()"`')
    _declare(lib, SIGNATURES)
    _lib = lib
    return lib
