"""CPU tests of the drop-in boundary: the C-ABI library builds, loads and exports every symbol that
include/efe_engine.h declares; the Python mirror exposes the reference's method names."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(efe_[a-z_0-9]+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from daimc_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f'{n} declared in efe_engine.h but not exported'
    assert sorted(_lib.EXPORTS) == names


def test_create_fails_cleanly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from daimc_amd import _lib
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.efe_create(ctypes.byref(ctx), 0) != 0
    import daimc_amd
    with pytest.raises(RuntimeError):
        daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0)


def test_python_mirror_has_reference_api():
    import daimc_amd
    M = daimc_amd.ActiveInferenceModel
    for name in ('calculate_G', 'calculate_G_mean', 'calculate_G_repeated', 'calculate_G_4_repeated',
                 'calculate_G_given_trajectory', 'mcts_step_simulate', 'check_reward', 'habitual_net',
                 'imagine_future_from_o', 'save_weights', 'load_weights', 'save_all', 'load_all'):
        assert callable(getattr(M, name))
    for name in ('encoder', 'encoder_with_sample', 'decoder', 'reparameterize'):
        assert callable(getattr(daimc_amd.ModelDown, name))
    for name in ('transition', 'transition_with_sample', 'reparameterize'):
        assert callable(getattr(daimc_amd.ModelMid, name))
    assert callable(daimc_amd.ModelTop.encode_s)
    p = daimc_amd.MCTS_Params()
    assert (p.C, p.threshold, p.repeats, p.simulation_repeats, p.simulation_depth, p.use_habit, p.use_means) == \
        (1.0, 0.5, 300, 1, 3, False, True)


def test_host_softmax_matches_golden(golden):
    import numpy as np
    from daimc_amd import softmax_multi_with_log
    g = golden('rollout_m8d2s2')
    P, logP = softmax_multi_with_log(-g['sum_G'], 4)
    np.testing.assert_allclose(P, g['Ppi'], rtol=1e-6)
    np.testing.assert_allclose(logP, g['logPpi'], rtol=1e-6, atol=1e-6)


def test_torch_ops_library_registers_every_op():
    """torch.ops.efe.* (SURVEY 8b item 1): the registration library builds, loads without a GPU and carries the schemas;
    no CPU kernel exists, so a CPU call is a loud NotImplementedError (no fallback)."""
    import torch
    import __graft_entry__ as ge
    ge.build()
    from daimc_amd import _lib
    ops = _lib.load_ops()
    want = {'transition', 'decoder', 'encoder', 'habit', 'calculate_g', 'rollout', 'trajectory', 'simulate', 'action_posterior',
            'check_reward', 'reparameterize'}
    for n in want:
        schema = str(getattr(ops, n).default._schema)
        assert schema.startswith(f'efe::{n}(int ctx, Tensor'), schema
    assert 'Tensor? eps' in str(ops.calculate_g.default._schema) and 'int row_offset' in str(ops.rollout.default._schema)
    with pytest.raises(NotImplementedError):
        ops.habit(1, torch.zeros(2, 10))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'efe_engine.h')).read(), flags=re.S)


def _prototypes():
    """every prototype of the header -> [(name, return type, [(base type, stars)])], comments stripped, arguments split on commas"""
    out = []
    for ret, name, args in re.findall(r'((?:const\s+)?\w+\s*\*?)\s*\b(efe_\w+)\s*\(([^()]*)\)\s*;', _header()):
        parsed = []
        for a in (a.strip() for a in args.split(',')):
            if a == 'void':
                continue
            m = re.fullmatch(r'(\w+)\s*(\*{0,2})\s*\w*', re.sub(r'\bconst\b', '', a).strip())
            assert m, f'{name}: cannot parse argument {a!r}'
            parsed.append((m.group(1), m.group(2)))
        out.append((name, re.sub(r'\s+', '', ret.replace('const', '')), parsed))
    return out


_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'double': ctypes.c_double}
_RETURNS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'void': None, 'char*': ctypes.c_char_p}


def _kind(base, stars, structs):
    """the ctypes type an argument of the header must be bound as"""
    if stars == '**':
        return ctypes.POINTER(ctypes.c_void_p) if base == 'efe_ctx' else f'<no rule for {base}**>'
    if stars == '':
        return _SCALARS.get(base, f'<no rule for {base}>')
    if base.startswith('efe_') and base != 'efe_ctx':
        return ctypes.POINTER(structs[base]) if base in structs else f'<no mirror of {base}>'
    if base == 'char':
        return ctypes.c_char_p
    if base in ('int', 'int64_t', 'double'):                     # host words the call writes (or reads: efe_set_weight's shape)
        return ctypes.POINTER(_SCALARS[base])
    return ctypes.c_void_p                                       # efe_ctx*, void*, device arrays


def signature_mismatches(signatures, structs):
    """the prototypes of the header against a {name: (restype, argtypes)} table -> one line per disagreement"""
    protos, bad = _prototypes(), []
    assert len(protos) >= 74 and len({n for n, _, _ in protos}) == len(protos), len(protos)
    for name in sorted(set(signatures) - {n for n, _, _ in protos}):
        bad.append(f'{name}: in the table, not in the header')
    for name, ret, args in protos:
        if signatures.get(name) is None or signatures[name][1] is None:
            bad.append(f'{name}: no signature')
            continue
        restype, argtypes = signatures[name]
        if restype is not _RETURNS[ret]:
            bad.append(f'{name}: returns {ret}, bound as {restype}')
        if len(argtypes) != len(args):
            bad.append(f'{name}: {len(args)} arguments, bound with {len(argtypes)}')
            continue
        for k, ((base, stars), have) in enumerate(zip(args, argtypes)):
            want = _kind(base, stars, structs)
            if have is not want:
                bad.append(f'{name}: argument {k} is {base}{stars}, bound as {getattr(have, "__name__", have)}, wants {getattr(want, "__name__", want)}')
    return bad


def test_signature_table_matches_the_header():
    """SIGNATURES against every prototype of include/efe_engine.h: name, argument count, the kind of every argument (a struct pointer is
    POINTER of that very struct's mirror) and of the return value; load() leaves no export unbound"""
    from daimc_amd import _lib
    assert signature_mismatches(_lib.SIGNATURES, _lib.STRUCTS) == []
    lib = _lib.load()
    for name in _lib.EXPORTS:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(_lib.SIGNATURES[name][1]) and fn.restype is _lib.SIGNATURES[name][0], name
    rows = _lib.EfeRows(None, None, 4, 3)                        # NULL and a row set both pass where the header says const efe_rows*
    for conv in (lambda: None, lambda: ctypes.byref(rows)):
        ctypes.POINTER(_lib.EfeRows).from_param(conv())


def _struct_fields():
    """every typedef struct of the header but the opaque efe_ctx -> {name: [field names in order]}"""
    out = {}
    for name, body, alias in re.findall(r'typedef\s+struct\s+(efe_\w+)\s*\{(.*?)\}\s*(\w+)\s*;', _header(), flags=re.S):
        assert name == alias
        out[name] = [re.sub(r'^.*[\s*]', '', d.strip()) for decl in body.split(';') if decl.strip() for d in decl.split(',')]
    return out


def layout_mismatches(structs, constants, tmp_path):
    """sizeof / offsetof of every mirrored struct and the value of every mirrored enum constant, from the header as gcc compiles it"""
    import subprocess
    fields = _struct_fields()
    bad = [f'{n}: no mirror' for n in fields if n not in structs] + [f'{n}: mirrored, not in the header' for n in structs if n not in fields]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "efe_engine.h"', 'int main(void) {']
    for n in (n for n in fields if n in structs):
        lines.append(f'    printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'    printf("{n}.{f} %zu %zu\\n", offsetof({n}, {f}), sizeof((({n}*)0)->{f}));' for f in fields[n]]
    lines += [f'    printf("{c} %lld\\n", (long long){c});' for c in constants] + ['    return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = {k: [int(v) for v in rest] for k, *rest in (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    for n in (n for n in fields if n in structs):
        mirror = structs[n]
        if got[n] != [ctypes.sizeof(mirror)]:
            bad.append(f'{n}: sizeof {got[n][0]}, mirror {ctypes.sizeof(mirror)}')
        names = [f for f, _ in mirror._fields_]
        if [f.rstrip('_') for f in names] != fields[n]:
            bad.append(f'{n}: fields {fields[n]}, mirror {names}')
            continue
        for f, hf in zip(names, fields[n]):
            d = getattr(mirror, f)
            if got[f'{n}.{hf}'] != [d.offset, d.size]:
                bad.append(f'{n}.{hf}: offset, size {got[f"{n}.{hf}"]}, mirror {[d.offset, d.size]}')
    return bad, {c: got[c][0] for c in constants}


def test_struct_mirrors_and_constants_match_the_compiled_header(tmp_path):
    """a C file that includes the header prints sizeof and every offsetof of each struct and every enum constant the binding mirrors;
    every typedef struct of the header (but the opaque efe_ctx) has a mirror"""
    from daimc_amd import _lib
    constants = ['EFE_STEP_MEANS', 'EFE_EVAL_STATS', 'EFE_EVAL_MAX_ROWS', 'EFE_EVAL_MI', 'EFE_EVAL_MI_MAX_NEIGHBORS']
    constants += sorted(set(re.findall(r'\b(EFE_(?:AGENT|OMEGA)_[A-Z0-9_]+)\s*=', _header())))
    assert len(constants) == 13 and len(_struct_fields()) >= 13
    bad, values = layout_mismatches(_lib.STRUCTS, constants, tmp_path)
    assert bad == []
    assert values == {c: getattr(_lib, c) for c in constants}


SCHEMAS = [
    'transition(int ctx, Tensor pi, Tensor s0, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> (Tensor ps1, Tensor mean, Tensor logvar)',
    'decoder(int ctx, Tensor s, int seed, int stage, int pass_id, int sample, int row_offset) -> Tensor',
    'encoder(int ctx, Tensor o, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, bool want_s) -> (Tensor s, Tensor mean, Tensor logvar)',
    'encoder_rows(int ctx, Tensor o, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, bool want_s, Tensor? mask=None, Tensor? ids=None, int rows_per_entry=1, int n_total=0) -> (Tensor s, Tensor mean, Tensor logvar)',
    'rollout_rows(int ctx, Tensor o, Tensor pi, int steps, int samples, bool calc_mean, bool per_stage_mean, int seed, int stage, int row_offset, Tensor? eps, Tensor? mask=None, Tensor? ids=None, int rows_per_entry=1, int n_total=0) -> (Tensor sum_G, Tensor sum_terms, Tensor po1)',
    'habit(int ctx, Tensor s) -> (Tensor logits, Tensor q, Tensor logq)',
    'calculate_g(int ctx, Tensor s0, Tensor pi0, int samples, bool mean_mode, int seed, int stage, int row_offset, Tensor? eps, Tensor? mask=None, Tensor? ids=None, int rows_per_entry=1, int n_total=0) -> (Tensor G, Tensor terms, Tensor ps1, Tensor ps1_mean, Tensor po1, Tensor t2parts)',
    'rollout(int ctx, Tensor o, Tensor pi, int steps, int samples, bool calc_mean, bool per_stage_mean, int seed, int stage, int row_offset, Tensor? eps) -> (Tensor sum_G, Tensor sum_terms, Tensor po1)',
    'trajectory(int ctx, Tensor s0_traj, Tensor ps1_traj, Tensor ps1_mean_traj, Tensor ps1_logvar_traj, Tensor pi0_traj, int seed, int stage, int row_offset, Tensor? eps) -> Tensor',
    'simulate(int ctx, Tensor starting_s, int depth, bool use_means, int seed, int stage, int row_offset, Tensor? eps, Tensor? u, Tensor? mask=None, Tensor? ids=None, int n_total=0) -> (Tensor G, Tensor pi0, Tensor Qpi0)',
    'action_posterior(int ctx, Tensor sum_G, int n, float temperature) -> (Tensor P, Tensor logP)',
    'check_reward(int ctx, Tensor o) -> Tensor',
    'reparameterize(int ctx, Tensor mean, Tensor logvar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> Tensor',
    'free_energy(int ctx, Tensor o0, Tensor o1, Tensor pi0, Tensor log_Ppi, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, float a, float b, float c, float d, int seed, int stage, int row_offset, Tensor? eps) -> Tensor[]',
    'loss_top(int ctx, Tensor s, Tensor log_Ppi) -> (Tensor F_top, Tensor kl_pi, Tensor kl_pi_anal, Tensor Qpi)',
    'loss_mid(int ctx, Tensor s0, Tensor Ppi_sampled, Tensor qs1_mean, Tensor qs1_logvar, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> (Tensor F_mid, Tensor kl_s, Tensor kl_s_anal, Tensor ps1, Tensor ps1_mean, Tensor ps1_logvar)',
    'loss_down(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> (Tensor F_down, Tensor nlogpo1, Tensor kl_s, Tensor kl_s_anal, Tensor kl_naive, Tensor kl_naive_anal, Tensor po1, Tensor qs1)',
    'top_grad(int ctx, Tensor s, Tensor log_Ppi) -> (Tensor kl_pi, Tensor grad)',
    'adam_step(int ctx, str part, Tensor grad, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> ()',
    'train_top(int ctx, Tensor s, Tensor log_Ppi, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> Tensor',
    'mid_grad(int ctx, Tensor s0, Tensor Ppi_sampled, Tensor qs1_mean, Tensor qs1_logvar, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset) -> (Tensor F_mid, Tensor ps1_mean, Tensor ps1_logvar, Tensor grad)',
    'train_mid(int ctx, Tensor s0, Tensor Ppi_sampled, Tensor qs1_mean, Tensor qs1_logvar, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> (Tensor ps1_mean, Tensor ps1_logvar, Tensor F_mid)',
    'dec_tail_grad(int ctx, Tensor h4, Tensor o1, float scale, float beta_o, bool want_y) -> (Tensor nlogpo1, Tensor po1, Tensor d_h4, Tensor grad, Tensor y1, Tensor y2, Tensor y3)',
    'dec_grad(int ctx, Tensor s, Tensor o1, float scale, float beta_o, int seed, int stage, int pass_id, int sample, int row_offset, bool want_act) -> Tensor[]',
    'enc_grad(int ctx, Tensor o, Tensor d_mean, Tensor d_logvar, int seed, int stage, int pass_id, int sample, int row_offset, bool want_act) -> Tensor[]',
    'down_grad(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> Tensor[]',
    'train_down(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float adam_eps, int step) -> Tensor[]',
    'train_step(int ctx, Tensor o0, Tensor o1, Tensor pi0, Tensor log_Ppi, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, float a, float b, float c, float d, int seed, int stage, int row_offset, Tensor? eps, Tensor(a!) top_exp_avg, Tensor(b!) top_exp_avg_sq, Tensor(c!) mid_exp_avg, Tensor(d!) mid_exp_avg_sq, Tensor(e!) down_exp_avg, Tensor(f!) down_exp_avg_sq, float[] hyper, int[] steps, Tensor(g!) means) -> Tensor[]',
    'eval_stats(int ctx, Tensor? F_top, Tensor? F_mid, Tensor? F_down, Tensor? nlogpo1, Tensor? kl_s, Tensor? kl_naive, Tensor? kl_pi, Tensor? kl_s_anal, Tensor? kl_naive_anal, Tensor? kl_pi_anal, Tensor? qs1, Tensor? s0, Tensor? S_real, Tensor? o1_r, Tensor? po1_r, int M, int Mr, Tensor(a!) out) -> ()',
    'down_adam_step(int ctx, Tensor grad, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> ()',
    'eval_mi(int ctx, Tensor s0, Tensor S_real, Tensor? noise, int n_neighbors, int seed, int stage, Tensor(a!) out, Tensor(b!)? counts) -> ()',
]


def test_torch_ops_schemas_are_unchanged():
    """the 31 ops and their schema strings as csrc/torch_ops.cpp registered them before its bodies were folded: a caller sees no change"""
    import torch
    from daimc_amd import _lib
    ops = _lib.load_ops()
    assert len(SCHEMAS) == 31
    names = {s.name.split('::')[1] for s in torch._C._jit_get_all_schemas() if s.name.startswith('efe::')}
    assert names == {s.split('(')[0] for s in SCHEMAS}
    for s in SCHEMAS:
        assert str(getattr(ops, s.split('(')[0]).default._schema) == 'efe::' + s


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """a binary whose embedded source digest differs from the sources next to it must not load"""
    from daimc_amd import _lib, build
    assert build._stamp(_lib.LIB_PATH, 'EFE_BUILD_ID') == build.source_digest()
    monkeypatch.setattr(build, 'source_digest', lambda files=None: '0' * 16)
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(ImportError, match='stale'):
        _lib.load()


def test_build_lists_match_csrc():
    """build.py's lists and csrc/ name the same files: a listed file that does not exist is a typo (build() refuses it), and a .hip or
    .h file that no list names would be left out of the library, or out of the digest that marks a binary stale"""
    import glob
    from daimc_amd import build
    for f in build.SOURCES + build.HEADERS + build.OPS_SOURCES:
        assert os.path.isfile(os.path.join(build.HERE, f)), f'build.py lists {f}, which does not exist'
    in_csrc = lambda ext: sorted('csrc/' + os.path.basename(p) for p in glob.glob(os.path.join(build.HERE, 'csrc', '*' + ext)))
    assert in_csrc('.hip') == sorted(build.SOURCES)
    assert in_csrc('.h') == sorted(h for h in build.HEADERS if h.startswith('csrc/'))
    assert len(set(build.SOURCES)) == len(build.SOURCES) and len(set(build.HEADERS)) == len(build.HEADERS)


def test_bench_refuses_more_ranks_than_devices():
    """`python bench.py --gpus N` without a launcher environment starts its own N ranks -- one per GPU; with fewer visible HIP devices
    than ranks it stops with a message (exit code 2) instead of stacking ranks on one device (--share-device is the explicit
    launcher-test mode).  Runs on the CPU box: zero devices are visible here."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0'], capture_output=True, text=True, env=env, timeout=300)
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('two devices are visible: the launcher would start the ranks')
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])
    assert 'one rank per GPU' in r.stderr and r.stdout.strip() == ''
