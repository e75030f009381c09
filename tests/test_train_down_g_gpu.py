"""GPU tests (-m gpu) of the gradient of F_down for all of ModelDown at every admitted geometry (loss.grad_down_g, efe_down_grad_g:
csrc/train_enc_g.hip around csrc/train_dec_head_g.hip + csrc/train_dec_g.hip) against tests/train_enc_g_ref.py's composed form -- autograd on
the CPU in fp32 and fp64 over compute_loss_down restated at (C, R), which at (1, 64) is tests/train_down_ref.run bit for bit
(tests/test_train_enc_g_cpu.py).

Engine seed 7, stage 3, inputs train_enc_g_ref.inputs(2000 + M, M, C, R).  Both oracles take their fourteen gates from the engine
(grad_encoder_g / grad_decoder_g on the same keys, whose gradients the composed call must reproduce bit for bit).  All 32 parameter tensors,
g_mean, g_logvar, mean, logvar, qs1, kl_s, kl_naive and po1 (image=True) are held to the project's fp64 rule; F_down and nlogpo1 to
tests/test_generic_geometry.py's sumtol against the fp32 oracle, and to tests/test_free_energy_gpu.py's sumtol (what
tests/test_train_down_gpu.py uses) against compute_loss_down.

(4, 1, 44) M = 33: even extents on two layers, K = 64, three 16-row tiles (slab = the tile's index in the call), conv slab 0 walks a second
image.  (3, 3, 84) M = 2: the Animal-AI size, K = 1 024, 32-row groups.  (4, 1, 64): the cross-check against grad_down."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_down_ref as TDN
import train_enc_g_ref as TEG
from test_free_energy_gpu import sumtol as fe_sumtol
from test_generic_geometry import sumtol
from test_train_dec_g_gpu import apply_rule, c, family, model_for

pytestmark = pytest.mark.gpu

STAGE = 3
G32, G44, G64, G84 = (3, 3, 32), (4, 1, 44), (4, 1, 64), (3, 3, 84)
PER_ROW = ('F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'po1', 'qs1', 'mean', 'logvar')
_ENG = {}


def engine(fam, geo, o1, pm, pv, om, model=None, gamma=None, gates=False, **key):
    """-> dict of numpy arrays with train_enc_g_ref.run's names (gates: also those of grad_encoder_g / grad_decoder_g on the same keys)"""
    import daimc_amd
    m = model or model_for(fam, geo)
    stage = key.pop('stage', STAGE)
    g0 = m.gamma
    if gamma is not None:
        m.gamma = float(gamma)
    try:
        F, (nl, kls, kln), po1, qs1, qm, qv, g, (gm, gv) = daimc_amd.loss.grad_down_g(m.model_down, o1, pm, pv, om, stage=stage, return_upstream=True, **key)
    finally:
        m.gamma = g0
    M = o1.shape[0]
    assert list(g) == list(TEG.KEYS)
    assert sum(v.numel() for v in g.values()) == TEG.param_count(geo[1], geo[2]) and next(iter(g.values())).dtype == torch.float32
    assert tuple(po1.shape) == (M, geo[1], geo[2], geo[2]) and tuple(F.shape) == (M,) and tuple(gm.shape) == (M, 10)
    out = dict(F_down=c(F), nlogpo1=c(nl), kl_s=c(kls), kl_naive=c(kln), po1=c(po1), qs1=c(qs1), mean=c(qm), logvar=c(qv), g_mean=c(gm), g_logvar=c(gv),
               grads={k: c(v) for k, v in g.items()})
    if gates:
        key.pop('eps', None)
        _, _, ge, act = daimc_amd.loss.grad_encoder_g(m.model_down, o1, gm, gv, stage=stage, return_activations=True, **key)
        _, _, _, gd, dact = daimc_amd.loss.grad_decoder_g(m.model_down, qs1, o1, stage=stage, return_activations=True, **key)
        out.update(gates=tuple(c(a) for a in act), dec_gates=tuple(c(a) for a in dact), enc_grads={k: c(v) for k, v in ge.items()},
                   dec_grads={k: c(v) for k, v in gd.items()})
    return out


def rule_rows(eng, o32, o64, keys=TEG.KEYS):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in keys]
    rows += [(k, eng[k], o32[k], o64[k], False) for k in ('g_mean', 'g_logvar', 'mean', 'logvar', 'qs1', 'kl_s', 'kl_naive')]
    rows.append(('po1', eng['po1'], o32['po1'], o64['po1'], True))
    return rows


def oracles(w, geo, o1, pm, pv, om, eng, **kw):
    return tuple(TEG.run(w, o1, pm, pv, om, geo[1], geo[2], STAGE, dt, gates=eng['gates'], dec_gates=eng['dec_gates'], **kw)
                 for dt in (torch.float32, torch.float64))


def check(tag, fam, geo, o1, pm, pv, om, gamma=0.5, eng=None, **kw):
    eng = eng or engine(fam, geo, o1, pm, pv, om, gamma=gamma, gates=True)
    o32, o64 = oracles(family(fam, geo), geo, o1, pm, pv, om, eng, gamma=gamma, **kw)
    for k in ('F_down', 'nlogpo1'):
        print(f'{tag} {k}: max err {np.abs(eng[k] - o32[k]).max():.3e} tol {sumtol(o32[k]):.3e}')
    apply_rule(tag, rule_rows(eng, o32, o64))
    for k in ('F_down', 'nlogpo1'):
        np.testing.assert_allclose(eng[k], o32[k], rtol=0, atol=sumtol(o32[k]), err_msg=f'{tag} {k}')
    assert all(np.isfinite(v).all() for v in eng['grads'].values())
    return eng, o32, o64


CASES = [(G44, 33), (G84, 2)]


def cached_engine(geo, M):
    if (geo, M) not in _ENG:
        inp = TEG.inputs(2000 + M, M, geo[1], geo[2])
        _ENG[geo, M] = inp + (engine('g115', geo, *inp, gates=True),)
    return _ENG[geo, M]


# ---- 7. composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geo,M', CASES)
def test_composition(geo, M):
    """grad_down_g's po_net gradients, po1 and nlogpo1 are grad_decoder_g(qs1, o1)'s, its qs_net gradients grad_encoder_g(o1, g_mean,
    g_logvar)'s, bit for bit; F_down and its terms agree with compute_loss_down under the same keys"""
    import daimc_amd
    o1, pm, pv, om, eng = cached_engine(geo, M)
    m = model_for('g115', geo)
    nl, po1, _, gd = daimc_amd.loss.grad_decoder_g(m.model_down, eng['qs1'], o1, stage=STAGE)
    assert np.array_equal(c(nl), eng['nlogpo1']) and np.array_equal(c(po1), eng['po1'])
    for k, v in gd.items():
        assert np.array_equal(c(v), eng['grads'][k]) and np.array_equal(eng['dec_grads'][k], eng['grads'][k]), k
    mean, lv, ge = daimc_amd.loss.grad_encoder_g(m.model_down, o1, eng['g_mean'], eng['g_logvar'], stage=STAGE)
    assert np.array_equal(c(mean), eng['mean']) and np.array_equal(c(lv), eng['logvar'])
    for k, v in ge.items():
        assert np.array_equal(c(v), eng['grads'][k]) and np.array_equal(eng['enc_grads'][k], eng['grads'][k]), k
    assert list(gd) == list(TEG.THG.KEYS) and list(ge) == list(TEG.ENC_KEYS)
    F, (fnl, kls, _, kln, _), fpo1, fqs1 = daimc_amd.loss.compute_loss_down(m.model_down, o1, pm, pv, om, stage=STAGE)
    o32, o64 = oracles(family('g115', geo), geo, o1, pm, pv, om, eng)
    apply_rule('compute_loss_down', [('kl_s', c(kls), o32['kl_s'], o64['kl_s'], False), ('kl_naive', c(kln), o32['kl_naive'], o64['kl_naive'], False),
                                     ('qs1', c(fqs1), o32['qs1'], o64['qs1'], False), ('po1', c(fpo1), o32['po1'], o64['po1'], True)])
    for name, got in (('F_down', c(F)), ('nlogpo1', c(fnl))):
        print(f'{name}: max |compute_loss_down - grad_down_g| {np.abs(got - eng[name]).max():.3e}  |compute_loss_down - o32| '
              f'{np.abs(got - o32[name]).max():.3e}  |grad_down_g - o32| {np.abs(eng[name] - o32[name]).max():.3e}  tol {fe_sumtol(o32[name]):.3e}')
    for name, got in (('F_down', c(F)), ('nlogpo1', c(fnl))):
        np.testing.assert_allclose(got, o32[name], rtol=0, atol=fe_sumtol(o32[name]), err_msg=name)
        np.testing.assert_allclose(eng[name], o32[name], rtol=0, atol=fe_sumtol(o32[name]), err_msg=name + ' (grad_down_g)')


@pytest.mark.parametrize('geo,M', CASES)
def test_gradients_vs_fp64(geo, M):
    o1, pm, pv, om, eng = cached_engine(geo, M)
    check(f'g115 {geo} M={M}', 'g115', geo, o1, pm, pv, om, eng=eng)


@pytest.mark.parametrize('geo,M', CASES)
@pytest.mark.parametrize('gamma', [0.0, 1.0])
def test_gamma_branches(geo, M, gamma):
    o1, pm, pv, om = TEG.inputs(2000 + M, M, geo[1], geo[2])
    check(f'{geo} gamma={gamma}', 'g115', geo, o1, pm, pv, om, gamma=gamma)


@pytest.mark.parametrize('geo,M', CASES)
def test_scalar_omega_and_injected_normals(geo, M):
    o1, pm, pv, _ = TEG.inputs(2000 + M, M, geo[1], geo[2])
    eng, _, _ = check(f'{geo} scalar omega', 'g115', geo, o1, pm, pv, 1.75)
    arr = engine('g115', geo, o1, pm, pv, np.full(M, 1.75, np.float32))
    for k in TEG.KEYS:
        assert np.array_equal(eng['grads'][k], arr['grads'][k]), k
    eps = np.random.RandomState(11).randn(M, 10).astype(np.float32)
    e2 = engine('g115', geo, o1, pm, pv, 1.75, gates=True, eps=eps)
    assert not np.array_equal(e2['qs1'], eng['qs1']) and np.array_equal(e2['mean'], eng['mean'])
    check(f'{geo} injected normals', 'g115', geo, o1, pm, pv, 1.75, eng=e2, eps=eps)


# ---- 5. reproducibility and row independence ---------------------------------------------------------------------------
def test_rows_are_independent_and_calls_reproducible():
    geo, M = G44, 5
    o1, pm, pv, om = TEG.inputs(2000 + M, M, geo[1], geo[2])
    a = engine('g115', geo, o1, pm, pv, om)
    b = engine('g115', geo, o1, pm, pv, om)
    for k in PER_ROW + ('g_mean', 'g_logvar'):
        assert np.array_equal(a[k], b[k]), k
    for k in TEG.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', geo, o1[r:r + 1], pm[r:r + 1], pv[r:r + 1], om[r:r + 1], row_offset=r)
        for k in PER_ROW:
            assert np.array_equal(one[k][0], a[k][r]), (k, r)


# ---- 8. cross-check at 1 x 64 x 64 -------------------------------------------------------------------------------------
def test_cross_check_at_1x64x64():
    import daimc_amd
    geo, M = G64, 5
    w = family('g115', geo)
    o1, pm, pv, om = TEG.inputs(2000 + M, M, 1, 64)
    m = model_for('g115', geo)
    g = engine('g115', geo, o1, pm, pv, om, gates=True)
    F, (nl, kls, kln), po1, qs1, qm, qv, gr, (gm, gv) = daimc_amd.loss.grad_down(m.model_down, o1, pm, pv, om, stage=STAGE, return_upstream=True)
    sp = dict(F_down=c(F), nlogpo1=c(nl), kl_s=c(kls), kl_naive=c(kln), po1=c(po1), qs1=c(qs1), mean=c(qm), logvar=c(qv), g_mean=c(gm), g_logvar=c(gv),
              grads={k: c(v) for k, v in gr.items()})
    _, _, _, act = daimc_amd.loss.grad_encoder(m.model_down, o1, gm, gv, stage=STAGE, return_activations=True)
    _, _, _, _, dact = daimc_amd.loss.grad_decoder(m.model_down, qs1, o1, stage=STAGE, return_activations=True)
    sp.update(gates=tuple(c(a) for a in act), dec_gates=tuple(c(a) for a in dact))
    for tag, eng in (('1x64x64 run-time geometry', g), ('1x64x64 specialised', sp)):
        o32, o64 = (TDN.run(w, o1, pm, pv, om, STAGE, dt, gates=eng['gates'], dec_gates=eng['dec_gates']) for dt in (torch.float32, torch.float64))
        apply_rule(tag, rule_rows(eng, o32, o64, TDN.KEYS))
        for k in ('F_down', 'nlogpo1'):
            np.testing.assert_allclose(eng[k], o32[k], rtol=0, atol=fe_sumtol(o32[k]), err_msg=f'{tag} {k}')


# ---- 9. refusals -------------------------------------------------------------------------------------------------------
def raw_call(m, M, *, o1=True, pm=True, pv=True, params=True, nz=True, out=True, F=True, grad=True, mode=None):
    import daimc_amd
    L = daimc_amd._lib
    e = m._ready()
    Cc, R = int(m.colour_channels), int(m.resolution)
    n = max(M, 1)
    t = [torch.zeros(n * Cc * R * R, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'),
         torch.zeros(TEG.param_count(Cc, R), device='cuda:0'), torch.zeros(n, device='cuda:0'), torch.ones(n, device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) if use else None for x, use in zip(t, (o1, pm, pv, grad))]
    noise = L.EfeNoise(7, STAGE, TEG.PASS_FE_DOWN, 0, 0)
    fp = L.EfeFeParams(0.5, 1.0, 1.0, L.EFE_OMEGA_ARRAY if mode is None else mode, t[5].data_ptr(), 1.5, 1.0, 25.0, 5.0, 1.5)
    fo = L.EfeFeOut()
    if F:
        fo.F_down = t[4].data_ptr()
    rc = e.lib.efe_down_grad_g(e.ctx, p[0], p[1], p[2], M, C.byref(fp) if params else None, C.byref(noise) if nz else None, None,
                               C.byref(fo) if out else None, None, None, p[3], e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, o1=False), dict(M=1, pm=False), dict(M=1, pv=False), dict(M=1, params=False),
                                dict(M=1, nz=False), dict(M=1, out=False), dict(M=1, F=False), dict(M=1, grad=False), dict(M=1, mode=2),
                                dict(M=1, mode=7)])
def test_bad_arguments_fail_cleanly(kw):
    m = model_for('g115', G32)
    rc, msg = raw_call(m, **kw)
    assert rc == 1 and 'efe_down_grad_g' in msg, (rc, msg)
    rc, _ = raw_call(m, 1)          # and the context still works
    assert rc == 0
    assert raw_call(m, 1, mode=1)[0] == 0


def test_split_operand_options_are_refused():
    m = model_for('g115', G64, fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_down_grad_g' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_the_other_entry_points_still_refuse():
    import daimc_amd
    m = model_for('g115', G32)
    z = np.zeros((1, 10), np.float32)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_down(m.model_down, np.zeros((1, 1, 64, 64), np.float32), z, z, 1.5)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_encoder(m.model_down, np.zeros((1, 1, 64, 64), np.float32), z, z)
    assert raw_call(m, 1)[0] == 0


def test_second_call_allocates_nothing():
    geo, M = G44, 17
    m = model_for('g115', geo, fresh=True)
    e = m._ready()
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    inp = TEG.inputs(2000 + M, M, geo[1], geo[2])
    a = engine('g115', geo, *inp, model=m)
    st0 = m.arena_stats()
    b = engine('g115', geo, *inp, model=m)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1['grow_count'] == st0['grow_count'] and st1['high_water_bytes'] == st0['high_water_bytes'] and st1['capacity_bytes'] == st0['capacity_bytes']
    assert all(np.array_equal(a['grads'][k], b['grads'][k]) for k in TEG.KEYS)
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before
