"""GPU tests (-m gpu) of the decoder tail's backward at every admitted geometry (csrc/train_dec_g.hip, loss.grad_decoder_convs_g,
efe_dec_tail_grad_g) against tests/train_dec_g_ref.py -- conv_transpose2d autograd on the CPU in fp32 and fp64, which at (1, 64) is
tests/train_dec_ref.py bit for bit (tests/test_train_dec_g_cpu.py).

Inputs: train_dec_g_ref.inputs(1000 + M, M, C, R).  As in tests/test_train_dec_gpu.py the engine is called with return_activations=True and
BOTH oracles take their ReLU gates from the engine's y1..y3; test_gate_condition keeps that override from hiding a wrong gate.  Every
parameter tensor, d_h4, y1..y3 and po1 (image=True) are held to the project's fp64 rule (tests/test_fp64_parity.py fp64_rule, alpha 4,
beta 8), nlogpo1 to tests/test_generic_geometry.py's sumtol (8e-6 max|ref| + 2e-2) against the fp32 oracle.

Geometries are (pi_dim, C, R); B = R / 4 is the decoder's base grid (16 at R = 32, where the third layer has stride 1).  The kernels tile
64 flattened positions per wave and 32 per weight-gradient chunk: B = 9 (81 positions), 10, 21 leave ragged last tiles at every layer;
(4, 3, 64) has whole tiles; (4, 2, 128) the largest index ranges.  Rows per pass are 64 (B <= 16) or 32: M = 65 at (4, 1, 36) and M = 33
at (4, 1, 68) (B = 17) make a second row group add into the slabs; at M = 33 slab 0 also walks a second image."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_dec_g_ref as TG
import train_dec_ref as TD
from oracle import synth
from test_fp64_parity import fp64_rule
from test_generic_geometry import sumtol

pytestmark = pytest.mark.gpu

SEED = 7
_FAMILIES, _MODELS, _ENG = {}, {}, {}


def c(t):
    return t.detach().cpu().numpy()


def family(name, geo):
    key = (name, geo)
    if key not in _FAMILIES:
        if name == 'g115':
            w = synth.make_weights(1234, 1.15, *geo)
        elif name == 'g100':
            w = synth.make_weights(7, 1.0, *geo)
        else:
            w = synth.stress_weights(name, *geo)
        _FAMILIES[key] = w
    return _FAMILIES[key]


def model_for(name, geo, fresh=False):
    import daimc_amd
    key = (name, geo)
    if not fresh and key in _MODELS:
        return _MODELS[key]
    m = daimc_amd.ActiveInferenceModel(10, geo[0], 0.5, 1.0, 1.0, colour_channels=geo[1], resolution=geo[2], device='cuda:0', seed=SEED,
                                       init_weights=False)
    m.load_flat_weights(family(name, geo))
    if not fresh:
        _MODELS[key] = m
    return m


def as_dict(out):
    nl, po1, d_h4, g, ys = out
    return dict(nlogpo1=c(nl), po1=c(po1), d_h4=c(d_h4), grads={k: c(v) for k, v in g.items()}, y=tuple(c(y) for y in ys))


def engine(fam, geo, h4, o1, scale=None):
    """-> dict of numpy arrays with train_dec_g_ref.run's names"""
    import daimc_amd
    nl, po1, d_h4, g, ys = out = daimc_amd.loss.grad_decoder_convs_g(model_for(fam, geo).model_down, h4, o1, scale=scale, return_activations=True)
    _, Cc, R = geo
    B, M = TG.base_of(R), h4.shape[0]
    assert list(g) == list(TG.KEYS) and sum(v.numel() for v in g.values()) == TG.param_count(Cc)
    assert tuple(po1.shape) == (M, Cc, R, R) and tuple(d_h4.shape) == (M, 64 * B * B) and tuple(nl.shape) == (M,)
    assert [tuple(y.shape) for y in ys] == [(M, 64, B, B), (M, 64, 2 * B, 2 * B), (M, 32, R, R)]
    return as_dict(out)


def apply_rule(tag, rows):
    """fp64_rule on [(name, eng, o32, o64, image)]; every figure is printed before the assertion"""
    bad = []
    for name, eng, o32, o64, image in rows:
        for r in fp64_rule(name, eng, o32, o64, image):
            print(f'{tag} {r[0]}: e_eng {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}')
            if not r[-1]:
                bad.append(r)
    assert not bad, f'{tag}: ' + '; '.join(f'{n}: e_eng {e:.3e} > bound {b:.3e} (e_32 {e3:.3e})' for n, e, e3, b, _, _ in bad)


def rule_rows(eng, o32, o64):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in TG.KEYS]
    rows.append(('d_h4', eng['d_h4'], o32['d_h4'], o64['d_h4'], False))
    rows += [(f'y{i + 1}', eng['y'][i], o32['y'][i], o64['y'][i], False) for i in range(3)]
    rows.append(('po1', eng['po1'], o32['po1'], o64['po1'], True))
    return rows


def hold(tag, w, geo, h4, o1, eng):
    """`eng` against both oracles gated by its own activations"""
    o32 = TG.run(w, h4, o1, geo[1], geo[2], torch.float32, gates=eng['y'])
    o64 = TG.run(w, h4, o1, geo[1], geo[2], torch.float64, gates=eng['y'])
    print(f'{tag} nlogpo1: max err {np.abs(eng["nlogpo1"] - o32["nlogpo1"]).max():.3e} tol {sumtol(o32["nlogpo1"]):.3e}')
    apply_rule(tag, rule_rows(eng, o32, o64))
    np.testing.assert_allclose(eng['nlogpo1'], o32['nlogpo1'], rtol=0, atol=sumtol(o32['nlogpo1']), err_msg=tag + ' nlogpo1')
    return o32


def check(tag, fam, geo, h4, o1):
    eng = engine(fam, geo, h4, o1)
    hold(tag, family(fam, geo), geo, h4, o1, eng)
    return eng


def cached_engine(fam, geo, M):
    if (fam, geo, M) not in _ENG:
        h4, o1 = TG.inputs(1000 + M, M, geo[1], geo[2])
        _ENG[fam, geo, M] = (h4, o1, engine(fam, geo, h4, o1))
    return _ENG[fam, geo, M]


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
G36, G40, G84, G32, G64, G128, G68 = (4, 1, 36), (4, 1, 40), (3, 3, 84), (3, 3, 32), (4, 3, 64), (4, 2, 128), (4, 1, 68)
GRAD_CASES = [('g115', G36, M) for M in (1, 2, 5, 33, 65)] + [('g115', G40, 2), ('g115', G84, 1), ('g115', G84, 2), ('g115', G32, 1), ('g115', G32, 5),
                                                               ('g115', G64, 2), ('g115', G128, 1), ('g115', G68, 33)]
GRAD_CASES += [(f, geo, M) for f in ('g100', 'sparse') for geo in (G36, G84) for M in (1, 2)]


@pytest.mark.parametrize('fam,geo,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, geo, M):
    h4, o1 = TG.inputs(1000 + M, M, geo[1], geo[2])
    eng = check(f'{fam} {geo} M={M}', fam, geo, h4, o1)
    _ENG.setdefault((fam, geo, M), (h4, o1, eng))
    assert all(np.isfinite(v).all() for v in eng['grads'].values())


# ---- 2. every admitted resolution -------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', list(range(32, 129, 4)))
def test_sweep_of_all_resolutions(R):
    geo = (4, 1 + (R // 4) % 3, R)
    h4, o1 = TG.inputs(1001, 1, geo[1], R)
    check(f'sweep {geo}', 'g115', geo, h4, o1)
    _MODELS.pop(('g115', geo), None)                  # one context per resolution: hand its device memory back
    _FAMILIES.pop(('g115', geo), None)


# ---- 3. gate condition -----------------------------------------------------------------------------------------------
def gates_within_cap(tag, ya, yb_or_a64, a64):
    """two gate sets may differ only where |a_64| <= 1e-5, on at most 1e-4 of a layer"""
    for li in range(3):
        diff = (ya[li] > 0) != (yb_or_a64[li] > 0)
        worst = float(np.abs(a64[li][diff]).max()) if diff.any() else 0.0
        print(f'{tag} layer {li + 1}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}')
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))


@pytest.mark.parametrize('fam,geo,M', [('g115', G84, 2), ('g115', G36, 5), ('g115', G32, 2), ('g115', G128, 1), ('sparse', G36, 2), ('g100', G84, 1)])
def test_gate_condition(fam, geo, M):
    """the engine's gates against the fp64 oracle's OWN ReLUs"""
    h4, o1, eng = cached_engine(fam, geo, M)
    own = TG.run(family(fam, geo), h4, o1, geo[1], geo[2], torch.float64)
    gates_within_cap(f'{fam} {geo} M={M}', eng['y'], own['a'], own['a'])


# ---- 4. cross-check against the specialised kernels at 1 x 64 x 64 ----------------------------------------------------
@pytest.mark.parametrize('M', [2, 33])
def test_cross_check_at_1x64x64(M):
    import daimc_amd
    geo = (4, 1, 64)
    w = family('g115', geo)
    h4, o1 = TG.inputs(1000 + M, M, 1, 64)
    g = engine('g115', geo, h4, o1)
    s = as_dict(daimc_amd.loss.grad_decoder_convs(model_for('g115', geo).model_down, h4, o1, return_activations=True))
    hold(f'1x64x64 M={M} run-time geometry', w, geo, h4, o1, g)
    ref = hold(f'1x64x64 M={M} specialised', w, geo, h4, o1, s)
    np.testing.assert_allclose(g['nlogpo1'], s['nlogpo1'], rtol=0, atol=sumtol(ref['nlogpo1']))
    own = TD.run(w, h4, o1, torch.float64)
    gates_within_cap(f'1x64x64 M={M} both engines', g['y'], s['y'], own['a'])


# ---- 5. row independence and determinism -----------------------------------------------------------------------------
def test_rows_are_independent_and_calls_reproducible():
    M, scale, geo = 5, 0.25, G84
    h4, o1 = TG.inputs(2005, M, geo[1], geo[2])
    a = engine('g115', geo, h4, o1, scale=scale)
    b = engine('g115', geo, h4, o1, scale=scale)
    for k in ('nlogpo1', 'po1', 'd_h4'):
        assert np.array_equal(a[k], b[k]), k
    for i in range(3):
        assert np.array_equal(a['y'][i], b['y'][i]), i
    for k in TG.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', geo, h4[r:r + 1], o1[r:r + 1], scale=scale)
        for k in ('nlogpo1', 'po1', 'd_h4'):
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
        for i in range(3):
            assert np.array_equal(one['y'][i][0], a['y'][i][r]), (i, r)


# ---- 6. nlogpo1's order ------------------------------------------------------------------------------------------------
def test_nlogpo1_is_the_documented_block_sum():
    """a CPU replay of the 256-thread ordered sum over the C R R NCHW terms of the row (thread t adds terms t, t + 256, ... ascending, xor
    butterfly, ((w0 + w1) + w2) + w3) on the engine's po1; rtol 2e-6: logf on the device and numpy's log may differ in the last place"""
    geo = G36
    h4, o1, eng = cached_engine('g115', geo, 2)
    N = geo[1] * geo[2] * geo[2]
    p, x = eng['po1'].reshape(2, N), o1.reshape(2, N)
    f = np.float32
    steps = (N + 255) // 256
    for r in range(2):
        t = (x[r] * np.log(f(0.00001) + p[r]).astype(f) + (f(1) - x[r]) * np.log(f(1.00001) - p[r]).astype(f)).astype(f)
        t = np.concatenate([t, np.zeros(256 * steps - N, f)])                 # (a thread without a term at the last step adds nothing)
        lanes = np.zeros(256, f)
        for j in range(steps):
            lanes = (lanes + t[256 * j:256 * (j + 1)]).astype(f)
        waves = lanes.reshape(4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            waves = (waves + waves[:, np.arange(64) ^ off]).astype(f)
        s = f(f(f(waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0])
        np.testing.assert_allclose(eng['nlogpo1'][r], -s, rtol=2e-6)


# ---- 7. borders ------------------------------------------------------------------------------------------------------
def border_case(name, geo):
    _, Cc, R = geo
    B = TG.base_of(R)
    h4, o1 = TG.inputs(3002, 2, Cc, R)
    if name == 'h4_ring':
        x = h4.reshape(2, 64, B, B).copy()
        x[:, :, 1:-1, 1:-1] = 0
        ring = np.zeros((B, B), bool)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
        x[:, :, ring] = np.abs(x[:, :, ring]) + 0.5
        h4 = x.reshape(2, 64 * B * B)
    elif name == 'o1_ring':
        o1 = np.zeros_like(o1)
        o1[:, :, 0], o1[:, :, -1], o1[:, :, :, 0], o1[:, :, :, -1] = 1, 1, 1, 1
    elif name == 'h4_zero':
        h4 = np.zeros_like(h4)
    elif name == 'o1_zero':
        o1 = np.zeros_like(o1)
    elif name == 'o1_one':
        o1 = np.ones_like(o1)
    return h4, o1


@pytest.mark.parametrize('geo', [G36, G84])
@pytest.mark.parametrize('name', ['h4_ring', 'o1_ring', 'h4_zero', 'o1_zero', 'o1_one'])
def test_borders(name, geo):
    h4, o1 = border_case(name, geo)
    check(f'border {name} {geo}', 'g115', geo, h4, o1)


# ---- 8. non-finite values ----------------------------------------------------------------------------------------------
def test_nan_in_one_row_stays_in_its_row():
    """one NaN in row 1's h4: every element that is NaN in the fp32 autograd oracle (its own ReLUs) is NaN in the engine, and the per-row
    outputs of rows 0 and 2 are those of the clean call, bit for bit"""
    geo, M = G36, 3
    h4, o1 = TG.inputs(8003, M, geo[1], geo[2])
    clean = engine('g115', geo, h4, o1)
    bad = h4.copy()
    bad[1, 64 * 40 + 31] = np.nan
    eng = engine('g115', geo, bad, o1)
    orc = TG.run(family('g115', geo), bad, o1, geo[1], geo[2], torch.float32)
    pairs = [(k, eng[k], orc[k]) for k in ('nlogpo1', 'po1', 'd_h4')] + [(f'y{i + 1}', eng['y'][i], orc['y'][i]) for i in range(3)]
    pairs += [(k, eng['grads'][k], orc['grads'][k]) for k in TG.KEYS]
    for name, e, o in pairs:
        on = np.isnan(o.reshape(e.shape))
        print(f'{name}: {int(on.sum())} NaN in the oracle, {int(np.isnan(e).sum())} in the engine')
        assert np.isnan(e[on]).all(), name
    assert np.isnan(orc['nlogpo1'][1]) and np.isnan(orc['grads']['po_net.13.weight']).any()
    for r in (0, 2):
        for k in ('nlogpo1', 'po1', 'd_h4'):
            assert np.array_equal(eng[k][r], clean[k][r]), (k, r)
        for i in range(3):
            assert np.array_equal(eng['y'][i][r], clean['y'][i][r]), (i, r)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------
def raw_call(m, M, *, h4=True, o1=True, nl=True, grad=True, fn='efe_dec_tail_grad_g'):
    e = m._ready()
    Cc, R = int(m.colour_channels), int(m.resolution)
    n = max(M, 1)
    t = [torch.zeros(n * 64 * TG.base_of(R) ** 2, device='cuda:0'), torch.zeros(n * Cc * R * R, device='cuda:0'), torch.zeros(n, device='cuda:0'),
         torch.zeros(TG.param_count(Cc), device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) if use else None for x, use in zip(t, (h4, o1, nl, grad))]
    rc = getattr(e.lib, fn)(e.ctx, p[0], p[1], M, C.c_float(-1.0), C.c_float(1.0), p[2], None, None, p[3], None, None, None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, h4=False), dict(M=1, o1=False), dict(M=1, nl=False), dict(M=1, grad=False)])
def test_bad_arguments_fail_cleanly(kw):
    m = model_for('g115', G36)
    rc, msg = raw_call(m, **kw)
    assert rc == 1 and 'efe_dec_tail_grad_g' in msg, (rc, msg)
    rc, _ = raw_call(m, 1)          # and the context still works
    assert rc == 0


def test_split_operand_options_are_refused():
    m = model_for('g115', (4, 1, 64), fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_dec_tail_grad_g' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_the_specialised_entry_point_still_refuses_other_geometries():
    m = model_for('g115', G32)
    e = m._ready()
    t = [torch.zeros(16384, device='cuda:0'), torch.zeros(4096, device='cuda:0'), torch.zeros(1, device='cuda:0'), torch.zeros(TD.P, device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) for x in t]
    rc = e.lib.efe_dec_tail_grad(e.ctx, p[0], p[1], 1, C.c_float(-1.0), C.c_float(1.0), p[2], None, None, p[3], None, None, None, e.stream())
    torch.cuda.synchronize()
    msg = e.lib.efe_last_error(e.ctx).decode()
    assert rc == 1 and 'efe_dec_tail_grad' in msg and '64' in msg, (rc, msg)
    assert raw_call(m, 1)[0] == 0
    assert e.lib.efe_param_count(e.ctx, b'po_net_convt') == TG.param_count(3)


def test_bad_scale_raises_and_macs_follow_the_geometry():
    import daimc_amd
    geo = G84
    m = model_for('g115', geo)
    h4, o1 = TG.inputs(1001, 1, geo[1], geo[2])
    for s in (-0.5, float('nan')):
        with pytest.raises(ValueError):
            daimc_amd.loss.grad_decoder_convs_g(m.model_down, h4, o1, scale=s)
    daimc_amd.loss.grad_decoder_convs_g(m.model_down, h4, o1)
    e = m._ready()
    B, R = 21, 84
    assert e.lib.efe_last_call_macs(e.ctx) == 3 * (2 * 64 * 64 * 9 * B * B + 64 * 32 * 9 * 4 * B * B + 32 * 3 * 9 * R * R)


def test_weight_update_reaches_the_raw_copy():
    """efe_set_weight + efe_commit_weights on a generic context: the gradient call reads the new values"""
    geo = G36
    m = model_for('g115', geo, fresh=True)
    h4, o1 = TG.inputs(6001, 1, geo[1], geo[2])
    import daimc_amd
    w = {k: np.array(v) for k, v in family('g115', geo).items()}
    w['down.po_net.19.bias'] = w['down.po_net.19.bias'] + np.float32(0.5)
    w['down.po_net.15.weight'] = (w['down.po_net.15.weight'] * np.float32(0.75)).astype(np.float32)
    m.load_flat_weights(w)
    eng = as_dict(daimc_amd.loss.grad_decoder_convs_g(m.model_down, h4, o1, return_activations=True))
    hold('updated weights', w, geo, h4, o1, eng)
