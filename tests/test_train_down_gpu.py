"""GPU tests (-m gpu) of the gradient of F_down for all of ModelDown (loss.grad_down, efe_down_grad: csrc/train_enc.hip around
csrc/train_dec_head.hip + csrc/train_dec.hip) against tests/train_down_ref.py -- the reference's compute_loss_down restated for autograd
on the CPU in fp32 and fp64, itself pinned bit for bit to the reference by tests/test_train_down_cpu.py.

Engine seed 7, stage 3, the default pass (PASS_FE_DOWN), inputs train_down_ref.inputs(2000 + M, M), the model's gamma 0.5 and
beta_s = beta_o = 1 unless a test sets gamma.  grad_down returns no activations, so the fourteen gates of BOTH oracles come from
grad_encoder and grad_decoder called with the same keys on the returned upstream pair and qs1 -- whose outputs test_composition shows to
be grad_down's own, bit for bit; the gates themselves are held to the gate condition by tests/test_train_enc_gpu.py and
tests/test_train_dec_head_gpu.py.  All 32 parameter tensors, g_mean, g_logvar, qs1_mean, qs1_logvar, qs1 and po1 (image=True) meet the
project's fp64 rule (alpha 4, beta 8), F_down and nlogpo1 tests/test_free_energy_gpu.py's sumtol, kl_s / kl_naive the rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_down_ref as TDN
from test_free_energy_gpu import sumtol
from test_train_dec_gpu import apply_rule, c, family, model_for

pytestmark = pytest.mark.gpu

STAGE = 3
_ENG = {}


def engine(fam, o1, pm, pv, om, model=None, gamma=None, gates=False, **key):
    """-> dict of numpy arrays with train_down_ref.run's names (gates: also those of grad_encoder / grad_decoder on the same keys)"""
    import daimc_amd
    m = model or model_for(fam)
    stage = key.pop('stage', STAGE)
    g0 = m.gamma
    if gamma is not None:
        m.gamma = float(gamma)
    try:
        F, (nl, kls, kln), po1, qs1, qm, qv, g, (gm, gv) = daimc_amd.loss.grad_down(m.model_down, o1, pm, pv, om, stage=stage, return_upstream=True, **key)
    finally:
        m.gamma = g0
    assert list(g) == list(TDN.KEYS)
    flat = next(iter(g.values()))
    assert sum(v.numel() for v in g.values()) == TDN.P and flat.dtype == torch.float32
    out = dict(F_down=c(F), nlogpo1=c(nl), kl_s=c(kls), kl_naive=c(kln), po1=c(po1), qs1=c(qs1), mean=c(qm), logvar=c(qv), g_mean=c(gm), g_logvar=c(gv),
               grads={k: c(v) for k, v in g.items()})
    if gates:
        key.pop('eps', None)
        _, _, ge, act = daimc_amd.loss.grad_encoder(m.model_down, o1, gm, gv, stage=stage, return_activations=True, **key)
        _, _, _, gd, dact = daimc_amd.loss.grad_decoder(m.model_down, qs1, o1, stage=stage, return_activations=True, **key)
        out.update(gates=tuple(c(a) for a in act), dec_gates=tuple(c(a) for a in dact), enc_grads={k: c(v) for k, v in ge.items()},
                   dec_grads={k: c(v) for k, v in gd.items()})
    return out


def rule_rows(eng, o32, o64):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in TDN.KEYS]
    rows += [(k, eng[k], o32[k], o64[k], False) for k in ('g_mean', 'g_logvar', 'mean', 'logvar', 'qs1', 'kl_s', 'kl_naive')]
    rows.append(('po1', eng['po1'], o32['po1'], o64['po1'], True))
    return rows


def oracles(w, o1, pm, pv, om, eng, **kw):
    return tuple(TDN.run(w, o1, pm, pv, om, STAGE, dt, gates=eng['gates'], dec_gates=eng['dec_gates'], **kw) for dt in (torch.float32, torch.float64))


def check(tag, fam, o1, pm, pv, om, gamma=0.5, eng=None, w=None, **kw):
    eng = eng or engine(fam, o1, pm, pv, om, gamma=gamma, gates=True)
    o32, o64 = oracles(w or family(fam), o1, pm, pv, om, eng, gamma=gamma, **kw)
    for k in ('F_down', 'nlogpo1'):
        print(f'{tag} {k}: max err {np.abs(eng[k] - o32[k]).max():.3e} tol {sumtol(o32[k]):.3e}')
    apply_rule(tag, rule_rows(eng, o32, o64))
    for k in ('F_down', 'nlogpo1'):
        np.testing.assert_allclose(eng[k], o32[k], rtol=0, atol=sumtol(o32[k]), err_msg=f'{tag} {k}')
    assert all(np.isfinite(v).all() for v in eng['grads'].values())
    return eng


def cached_engine(fam, M):
    if (fam, M) not in _ENG:
        inp = TDN.inputs(2000 + M, M)
        _ENG[fam, M] = inp + (engine(fam, *inp, gates=True),)
    return _ENG[fam, M]


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', M) for M in (1, 2, 5, 17, 33, 65)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)]


@pytest.mark.parametrize('fam,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, M):
    o1, pm, pv, om, eng = cached_engine(fam, M)
    check(f'{fam} M={M}', fam, o1, pm, pv, om, eng=eng)


@pytest.mark.parametrize('gamma', [0.0, 0.5, 1.0])
def test_gamma_branches(gamma):
    o1, pm, pv, om = TDN.inputs(2005, 5)
    check(f'gamma={gamma}', 'g115', o1, pm, pv, om, gamma=gamma)


def test_scalar_omega_and_injected_normals():
    o1, pm, pv, _ = TDN.inputs(2005, 5)
    eng = check('scalar omega', 'g115', o1, pm, pv, 1.75)
    arr = engine('g115', o1, pm, pv, np.full(5, 1.75, np.float32))
    for k in TDN.KEYS:
        assert np.array_equal(eng['grads'][k], arr['grads'][k]), k
    eps = np.random.RandomState(11).randn(5, 10).astype(np.float32)
    e2 = engine('g115', o1, pm, pv, 1.75, gates=True, eps=eps)
    assert not np.array_equal(e2['qs1'], eng['qs1']) and np.array_equal(e2['mean'], eng['mean'])
    check('injected normals', 'g115', o1, pm, pv, 1.75, eng=e2, eps=eps)


# ---- 2. composition, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [5, 65])
def test_composition(M):
    """grad_down's po_net gradients, po1 and nlogpo1 are grad_decoder(qs1, o1, scale=None)'s, its qs_net gradients grad_encoder(o1, g_mean,
    g_logvar)'s, bit for bit; F_down and its terms agree with compute_loss_down under the same keys"""
    import daimc_amd
    o1, pm, pv, om, eng = cached_engine('g115', M)
    m = model_for('g115')
    nl, po1, _, gd = daimc_amd.loss.grad_decoder(m.model_down, eng['qs1'], o1, stage=STAGE)
    assert np.array_equal(c(nl), eng['nlogpo1']) and np.array_equal(c(po1), eng['po1'])
    for k, v in gd.items():
        assert np.array_equal(c(v), eng['grads'][k]) and np.array_equal(eng['dec_grads'][k], eng['grads'][k]), k
    mean, lv, ge = daimc_amd.loss.grad_encoder(m.model_down, o1, eng['g_mean'], eng['g_logvar'], stage=STAGE)
    assert np.array_equal(c(mean), eng['mean']) and np.array_equal(c(lv), eng['logvar'])
    for k, v in ge.items():
        assert np.array_equal(c(v), eng['grads'][k]), k
    assert list(gd) == list(TDN.TH.KEYS) and list(ge) == list(TDN.ENC_KEYS)
    F, (fnl, kls, _, kln, _), fpo1, fqs1 = daimc_amd.loss.compute_loss_down(m.model_down, o1, pm, pv, om, stage=STAGE)
    o32, o64 = oracles(family('g115'), o1, pm, pv, om, eng)
    apply_rule('compute_loss_down', [('kl_s', c(kls), o32['kl_s'], o64['kl_s'], False), ('kl_naive', c(kln), o32['kl_naive'], o64['kl_naive'], False),
                                     ('qs1', c(fqs1), o32['qs1'], o64['qs1'], False), ('po1', c(fpo1), o32['po1'], o64['po1'], True)])
    for name, got in (('F_down', c(F)), ('nlogpo1', c(fnl))):
        print(f'{name}: max |compute_loss_down - grad_down| {np.abs(got - eng[name]).max():.3e}')
        np.testing.assert_allclose(got, o32[name], rtol=0, atol=sumtol(o32[name]), err_msg=name)
    mean2, lv2 = m.model_down.encoder(o1, stage=STAGE, pass_=daimc_amd.model.PASS_FE_DOWN)
    apply_rule('forward encoder', [('mean', c(mean2), o32['mean'], o64['mean'], False), ('logvar', c(lv2), o32['logvar'], o64['logvar'], False)])


# ---- 3. reproducibility and row independence ---------------------------------------------------------------------------
PER_ROW = ('F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'po1', 'qs1', 'mean', 'logvar')


def test_rows_are_independent_and_calls_reproducible():
    M = 5
    o1, pm, pv, om = TDN.inputs(2005, M)
    a = engine('g115', o1, pm, pv, om)
    b = engine('g115', o1, pm, pv, om)
    for k in PER_ROW + ('g_mean', 'g_logvar'):
        assert np.array_equal(a[k], b[k]), k
    for k in TDN.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', o1[r:r + 1], pm[r:r + 1], pv[r:r + 1], om[r:r + 1], row_offset=r)
        for k in PER_ROW:
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
    for key in (dict(stage=STAGE + 1), dict(sample=1)):
        other = engine('g115', o1, pm, pv, om, **key)
        assert not np.array_equal(other['qs1'], a['qs1']) and not np.array_equal(other['mean'], a['mean']), key


# ---- 4. boundary -----------------------------------------------------------------------------------------------------
def raw_call(m, M, *, o1=True, pm=True, pv=True, params=True, nz=True, out=True, F=True, grad=True, mode=None):
    import daimc_amd
    L = daimc_amd._lib
    e = m._ready()
    n = max(M, 1)
    t = [torch.zeros(n * 4096, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'),
         torch.zeros(TDN.P, device='cuda:0'), torch.zeros(n, device='cuda:0'), torch.ones(n, device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) if use else None for x, use in zip(t, (o1, pm, pv, grad))]
    noise = L.EfeNoise(7, STAGE, TDN.PASS_FE_DOWN, 0, 0)
    fp = L.EfeFeParams(0.5, 1.0, 1.0, L.EFE_OMEGA_ARRAY if mode is None else mode, t[5].data_ptr(), 1.5, 1.0, 25.0, 5.0, 1.5)
    fo = L.EfeFeOut()
    if F:
        fo.F_down = t[4].data_ptr()
    rc = e.lib.efe_down_grad(e.ctx, p[0], p[1], p[2], M, C.byref(fp) if params else None, C.byref(noise) if nz else None, None,
                             C.byref(fo) if out else None, None, None, p[3], e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, o1=False), dict(M=1, pm=False), dict(M=1, pv=False), dict(M=1, params=False),
                                dict(M=1, nz=False), dict(M=1, out=False), dict(M=1, F=False), dict(M=1, grad=False), dict(M=1, mode=2),
                                dict(M=1, mode=7)])
def test_bad_arguments_fail_cleanly(kw):
    rc, msg = raw_call(model_for('g115'), **kw)
    assert rc == 1 and 'efe_down_grad' in msg, (rc, msg)
    rc, _ = raw_call(model_for('g115'), 1)          # and the context still works
    assert rc == 0
    assert raw_call(model_for('g115'), 1, mode=1)[0] == 0


def test_other_geometry_is_refused():
    import daimc_amd
    m = model_for('g115', (3, 3, 32))
    rc, msg = raw_call(m, 1)
    assert rc == 1 and 'efe_down_grad' in msg and '64' in msg, (rc, msg)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_down(m.model_down, np.zeros((1, 1, 64, 64), np.float32), np.zeros((1, 10), np.float32), np.zeros((1, 10), np.float32), 1.5)


def test_split_operand_options_are_refused():
    m = model_for('g115', fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_down_grad' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_gradient_call_has_no_side_effects_and_allocates_once():
    m = model_for('g115')
    e = m._ready()
    inp = TDN.inputs(2003, 3)
    before = tuple(c(t) for t in m.model_down.encoder_with_sample(inp[0], stage=2))
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    o1, pm, pv, om = TDN.inputs(2017, 17)
    a = engine('g115', o1, pm, pv, om)
    st0 = m.arena_stats()
    b = engine('g115', o1, pm, pv, om)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1['grow_count'] == st0['grow_count'] and st1['high_water_bytes'] == st0['high_water_bytes'] and st1['capacity_bytes'] == st0['capacity_bytes']
    assert all(np.array_equal(a['grads'][k], b['grads'][k]) for k in TDN.KEYS)
    after = tuple(c(t) for t in m.model_down.encoder_with_sample(inp[0], stage=2))
    assert all(np.array_equal(p, q) for p, q in zip(before, after))
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before
