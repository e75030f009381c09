"""GPU tests (-m gpu) of the encoder's training forward and backward at every admitted geometry (csrc/train_enc_g.hip, loss.grad_encoder_g,
efe_enc_grad_g) against tests/train_enc_g_ref.py -- F.conv2d / F.linear autograd on the CPU in fp32 and fp64 with the Philox dropout masks
as multiplications, which at (1, 64) is tests/train_down_ref.py and elsewhere encodes oracle.efe_oracle's encoder, bit for bit
(tests/test_train_enc_g_cpu.py).

Engine seed 7, stage 3, the default pass (PASS_FE_DOWN), images train_enc_g_ref.inputs(2000 + M, M, C, R), upstream pair N(0, 1) / M, weights
by oracle.synth as in tests/test_train_dec_g_gpu.py.  The engine is called with return_activations=True and BOTH oracles take their seven
gates from the engine's y1..y4 and h1..h3; test_masks_and_gates keeps that override from hiding a wrong gate or a wrongly keyed mask.  All
16 parameter tensors, mean, logvar, y1..y4 and h1..h3 are held to the project's fp64 rule (tests/test_fp64_parity.py fp64_rule, alpha 4,
beta 8).

Geometries are (pi_dim, C, R); conv extents H_l = (H_{l-1} - 3) // 2 + 1, K = 64 H4^2 inputs of qs_net.9:
  (3, 3, 32)   15, 7, 3, 1; K = 64; three channels          (4, 1, 44)   21, 10, 4, 1: even inputs on two layers; K = 64: 4 chunks < 8 accumulators
  (4, 2, 48)   K = 256 = one full segment; two channels      (4, 1, 68)   33, 16, 7, 3: K = 576 with an even extent
  (3, 3, 84)   41, 20, 9, 4: K = 1 024                        (4, 2, 128)  63, 31, 15, 7: K = 3 136, 32-row groups
M = 17: a ragged second tile; 33: conv slab 0 walks a second image (and at resolution 128 a second 32-row group); 65: a second 64-row group."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_down_ref as TDN
import train_enc_g_ref as TEG
from test_train_dec_g_gpu import _FAMILIES, _MODELS, apply_rule, c, family, model_for

pytestmark = pytest.mark.gpu

STAGE = 3
ACT = ('y1', 'y2', 'y3', 'y4', 'h1', 'h2', 'h3')
G32, G44, G48, G64, G68, G84, G128 = (3, 3, 32), (4, 1, 44), (4, 2, 48), (4, 1, 64), (4, 1, 68), (3, 3, 84), (4, 2, 128)
_ENG = {}


def as_dict(out):
    mean, lv, g, act = out
    act = tuple(c(a) for a in act)
    return dict(mean=c(mean), logvar=c(lv), grads={k: c(v) for k, v in g.items()}, y=act[:4], h=act[4:])


def engine(fam, geo, o, gm, gv, model=None, **key):
    """-> dict of numpy arrays with train_enc_g_ref.run_encoder's names"""
    import daimc_amd
    m = model or model_for(fam, geo)
    out = daimc_amd.loss.grad_encoder_g(m.model_down, o, gm, gv, stage=key.pop('stage', STAGE), return_activations=True, **key)
    mean, lv, g, act = out
    _, Cc, R = geo
    H, M = TEG.extents(R), o.shape[0]
    assert list(g) == list(TEG.ENC_KEYS) and len(act) == 7
    assert sum(v.numel() for v in g.values()) == TEG.enc_param_count(Cc, R) and next(iter(g.values())).dtype == torch.float32
    assert tuple(g['qs_net.0.weight'].shape) == (32, Cc, 3, 3) and tuple(g['qs_net.9.weight'].shape) == (256, TEG.n_in(R))
    assert tuple(mean.shape) == (M, 10) and tuple(lv.shape) == (M, 10)
    assert [tuple(a.shape) for a in act] == [(M, 32, H[0], H[0]), (M, 32, H[1], H[1]), (M, 64, H[2], H[2]), (M, 64, H[3], H[3])] + [(M, 256)] * 3
    return as_dict(out)


def rule_rows(eng, o32, o64):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in TEG.ENC_KEYS]
    rows += [(k, eng[k], o32[k], o64[k], False) for k in ('mean', 'logvar')]
    rows += [(f'y{i + 1}', eng['y'][i], o32['y'][i], o64['y'][i], False) for i in range(4)]
    rows += [(f'h{i + 1}', eng['h'][i], o32['h'][i], o64['h'][i], False) for i in range(3)]
    return rows


def oracles(w, geo, o, gm, gv, eng, **key):
    gates = eng['y'] + eng['h']
    return tuple(TEG.run_encoder(w, o, gm, gv, geo[1], geo[2], STAGE, dt, gates=gates, **key) for dt in (torch.float32, torch.float64))


def case(geo, M):
    return TEG.inputs(2000 + M, M, geo[1], geo[2])[0], *TEG.upstream(2000 + M, M)


def cached_engine(fam, geo, M):
    if (fam, geo, M) not in _ENG:
        o, gm, gv = case(geo, M)
        _ENG[fam, geo, M] = (o, gm, gv, engine(fam, geo, o, gm, gv))
    return _ENG[fam, geo, M]


def hold(tag, w, geo, o, gm, gv, eng, **key):
    o32, o64 = oracles(w, geo, o, gm, gv, eng, **key)
    apply_rule(tag, rule_rows(eng, o32, o64))
    return o32, o64


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', G44, M) for M in (1, 2, 5, 17, 33, 65)] + [('g115', G128, 1), ('g115', G128, 33), ('g115', G32, 2), ('g115', G48, 2),
                                                                  ('g115', G68, 1), ('g115', G84, 2)]
GRAD_CASES += [(f, geo, M) for f in ('g100', 'sparse') for geo in (G44, G84) for M in (1, 2)]


@pytest.mark.parametrize('fam,geo,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, geo, M):
    o, gm, gv, eng = cached_engine(fam, geo, M)
    hold(f'{fam} {geo} M={M}', family(fam, geo), geo, o, gm, gv, eng)
    assert all(np.isfinite(v).all() for v in eng['grads'].values())
    if M > 5:
        _ENG.pop((fam, geo, M))


# ---- 2. every admitted resolution -------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', list(range(32, 129, 4)))
def test_sweep_of_all_resolutions(R):
    geo = (4, 1 + (R // 4) % 3, R)
    o, gm, gv = case(geo, 1)
    eng = engine('g115', geo, o, gm, gv)
    hold(f'sweep {geo}', family('g115', geo), geo, o, gm, gv, eng)
    _MODELS.pop(('g115', geo), None)                  # one context per resolution: hand its device memory back
    _FAMILIES.pop(('g115', geo), None)


# ---- 3. masks and gates ----------------------------------------------------------------------------------------------
GATE_CASES = [('g115', G44, 5), ('g115', G84, 2), ('g115', G32, 2), ('g115', G128, 1), ('sparse', G44, 2), ('g100', G84, 1)]


@pytest.mark.parametrize('fam,geo,M', GATE_CASES)
def test_masks_and_gates(fam, geo, M):
    """head: h_l > 0 only where the oracle's Philox mask bit is set (exact), and against the fp64 oracle's OWN pre-activations the gate may
    differ from mask * [a_64 > 0] only where |a_64| <= 1e-5, on at most 1e-4 of a layer; convolutions: the same condition on [y > 0]"""
    o, gm, gv, eng = cached_engine(fam, geo, M)
    own = TEG.run_encoder(family(fam, geo), o, gm, gv, geo[1], geo[2], STAGE, torch.float64)
    for li in range(3):
        h, mask = eng['h'][li], own['enc_masks'][li]
        assert h.shape == mask.shape
        outside = int(((h > 0) & (mask == 0)).sum())
        print(f'{fam} {geo} M={M} head layer {li}: {int((h > 0).sum())} of {h.size} kept, {outside} outside the mask')
        assert outside == 0, li
    have = eng['y'] + eng['h']
    want = [a > 0 for a in own['a_conv']] + [(own['enc_masks'][li] > 0) & (own['a_dense'][li] > 0) for li in range(3)]
    a64 = own['a_conv'] + own['a_dense']
    for li in range(7):
        diff = (have[li] > 0) != want[li]
        worst = float(np.abs(a64[li][diff]).max()) if diff.any() else 0.0
        print(f'{fam} {geo} M={M} {ACT[li]}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}')
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))


# ---- 4. unread rows are zeros, whatever the arena held -----------------------------------------------------------------
@pytest.mark.parametrize('geo', [G44, G84])
def test_unread_rows_are_zeros_whatever_the_arena_held(geo):
    """a layer with an even input extent never reads the last row and column of its input; the gradient there must be STORED as zero: the
    same case on a fresh model and on a second model whose arena a larger call with other inputs has filled gives the same bits"""
    M = 2
    o, gm, gv = case(geo, M)
    a = engine('g115', geo, o, gm, gv, model=model_for('g115', geo, fresh=True))
    m2 = model_for('g115', geo, fresh=True)
    ob, gmb, gvb = case(geo, 65)
    engine('g115', geo, ob + np.float32(0.5), gmb * np.float32(1e3), gvb * np.float32(-1e3), model=m2)
    b = engine('g115', geo, o, gm, gv, model=m2)
    for k in ('mean', 'logvar'):
        assert np.array_equal(a[k], b[k]), k
    for i, (x, y) in enumerate(zip(a['y'] + a['h'], b['y'] + b['h'])):
        assert np.array_equal(x, y), ACT[i]
    for k in TEG.ENC_KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    hold(f'after a larger call {geo}', family('g115', geo), geo, o, gm, gv, b)


# ---- 5. determinism and row independence -------------------------------------------------------------------------------
@pytest.mark.parametrize('geo', [G44, G84])
def test_rows_are_independent_and_calls_reproducible(geo):
    M = 5
    o, gm, gv = case(geo, M)
    a = engine('g115', geo, o, gm, gv)
    b = engine('g115', geo, o, gm, gv)
    for k in ('mean', 'logvar'):
        assert np.array_equal(a[k], b[k]), k
    for i, (x, y) in enumerate(zip(a['y'] + a['h'], b['y'] + b['h'])):
        assert np.array_equal(x, y), ACT[i]
    for k in TEG.ENC_KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', geo, o[r:r + 1], gm[r:r + 1], gv[r:r + 1], row_offset=r)
        for k in ('mean', 'logvar'):
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
        for i, (x, y) in enumerate(zip(one['y'] + one['h'], a['y'] + a['h'])):
            assert np.array_equal(x[0], y[r]), (ACT[i], r)
    for key in (dict(stage=STAGE + 1), dict(sample=1)):
        other = engine('g115', geo, o, gm, gv, **key)
        for i in range(3):
            assert not np.array_equal(other['h'][i] > 0, a['h'][i] > 0), (key, i)


# ---- 6. padded last layer ----------------------------------------------------------------------------------------------
def test_padded_features_of_the_last_layer_feed_zeros():
    """qs_net.18.bias lies directly behind the 20 x 256 weight in the flat copy: with 1e30 there the 12 padded features of the last
    layer's tile must not leak into any output"""
    geo = G44
    m = model_for('g115', geo, fresh=True)
    w = {k: np.array(v) for k, v in family('g115', geo).items()}
    w['down.qs_net.18.bias'] = np.full_like(w['down.qs_net.18.bias'], 1e30)
    m.load_flat_weights(w)
    o, gm, gv = case(geo, 5)
    eng = engine('g115', geo, o, gm, gv, model=m)
    ref = cached_engine('g115', geo, 5)[3]
    for k in ('mean', 'logvar'):
        assert np.isfinite(eng[k]).all() and (eng[k] > 1e29).all(), k
    assert all(np.isfinite(a).all() for a in eng['y'] + eng['h'])
    for k in TEG.ENC_KEYS:          # the bias enters no gradient: they are those of the unchanged weights, bit for bit
        assert np.isfinite(eng['grads'][k]).all() and np.array_equal(eng['grads'][k], ref['grads'][k]), k


# ---- 8. cross-check against the specialised kernels at 1 x 64 x 64 -------------------------------------------------------
@pytest.mark.parametrize('M', [2, 33])
def test_cross_check_at_1x64x64(M):
    import daimc_amd
    geo = G64
    w = family('g115', geo)
    o, gm, gv = case(geo, M)
    assert np.array_equal(o, TDN.inputs(2000 + M, M)[0])
    m = model_for('g115', geo)
    g = engine('g115', geo, o, gm, gv)
    sp = as_dict(daimc_amd.loss.grad_encoder(m.model_down, o, gm, gv, stage=STAGE, return_activations=True))
    for tag, eng in ((f'1x64x64 M={M} run-time geometry', g), (f'1x64x64 M={M} specialised', sp)):
        o32, o64 = (TDN.run_encoder(w, o, gm, gv, STAGE, dt, gates=eng['y'] + eng['h']) for dt in (torch.float32, torch.float64))
        apply_rule(tag, rule_rows(eng, o32, o64))


def test_forward_encoder_agrees_with_mean_and_logvar():
    """model_down.encoder with the same keys encodes the same network (the same masks) at (3, 3, 84)"""
    import daimc_amd
    geo = G84
    o, gm, gv, eng = cached_engine('g115', geo, 2)
    o32, o64 = oracles(family('g115', geo), geo, o, gm, gv, eng)
    mean, lv = model_for('g115', geo).model_down.encoder(o, stage=STAGE, pass_=daimc_amd.model.PASS_FE_DOWN)
    print(f'max |encoder - grad_encoder_g| mean {np.abs(c(mean) - eng["mean"]).max():.3e} logvar {np.abs(c(lv) - eng["logvar"]).max():.3e}')
    apply_rule('forward encoder', [('mean', c(mean), o32['mean'], o64['mean'], False), ('logvar', c(lv), o32['logvar'], o64['logvar'], False)])


# ---- non-finite input ----------------------------------------------------------------------------------------------------
def test_nan_in_one_row_stays_in_its_row():
    """one NaN pixel in row 1's image: every element that is NaN in the fp32 autograd oracle (its own ReLUs and masks) is NaN in the engine
    (mean, logvar and gradients among them), and the per-row outputs of rows 0 and 2 are those of the clean call, bit for bit"""
    geo, M = G44, 3
    o, gm, gv = case(geo, M)
    clean = engine('g115', geo, o, gm, gv)
    bad = o.copy()
    bad[1, 0, 20, 22] = np.nan
    eng = engine('g115', geo, bad, gm, gv)
    with np.errstate(all='ignore'):
        orc = TEG.run_encoder(family('g115', geo), bad, gm, gv, geo[1], geo[2], STAGE, torch.float32)
    pairs = [(k, eng[k], orc[k]) for k in ('mean', 'logvar')] + [(ACT[i], x, y) for i, (x, y) in enumerate(zip(eng['y'] + eng['h'], orc['y'] + orc['h']))]
    pairs += [(k, eng['grads'][k], orc['grads'][k]) for k in TEG.ENC_KEYS]
    for name, e, r in pairs:
        on = np.isnan(r.reshape(e.shape))
        print(f'{name}: {int(on.sum())} NaN in the oracle, {int(np.isnan(e).sum())} in the engine')
        assert np.isnan(e[on]).all(), name
    assert np.isnan(orc['mean'][1]).all() and np.isnan(eng['mean'][1]).all() and np.isnan(orc['grads']['qs_net.0.weight']).any()
    for r in (0, 2):
        for k in ('mean', 'logvar'):
            assert np.array_equal(eng[k][r], clean[k][r]), (k, r)
        for i, (x, y) in enumerate(zip(eng['y'] + eng['h'], clean['y'] + clean['h'])):
            assert np.array_equal(x[r], y[r]), (ACT[i], r)


# ---- 9. raw calls: refusals, counts, scratch -------------------------------------------------------------------------------
def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def raw_call(m, M, *, o=True, gm=True, gv=True, nz=True, grad=True):
    import daimc_amd
    e = m._ready()
    Cc, R = int(m.colour_channels), int(m.resolution)
    n = max(M, 1)
    t = [torch.zeros(n * Cc * R * R, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'),
         torch.zeros(TEG.enc_param_count(Cc, R), device='cuda:0')]
    p = [ptr(x) if use else None for x, use in zip(t, (o, gm, gv, grad))]
    noise = daimc_amd._lib.EfeNoise(7, STAGE, TEG.PASS_FE_DOWN, 0, 0)
    rc = e.lib.efe_enc_grad_g(e.ctx, p[0], p[1], p[2], M, C.byref(noise) if nz else None, None, None, p[3], None, None, None, None, None, None, None,
                              e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, o=False), dict(M=1, gm=False), dict(M=1, gv=False), dict(M=1, nz=False),
                                dict(M=1, grad=False)])
def test_bad_arguments_fail_cleanly(kw):
    m = model_for('g115', G44)
    rc, msg = raw_call(m, **kw)
    assert rc == 1 and 'efe_enc_grad_g' in msg, (rc, msg)
    rc, _ = raw_call(m, 1)          # and the context still works
    assert rc == 0


def test_split_operand_options_are_refused():
    m = model_for('g115', G64, fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_enc_grad_g' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_param_counts_and_no_adam_for_these_parts():
    import daimc_amd
    m = model_for('g115', G32)
    e = m._ready()
    P, PD = TEG.enc_param_count(3, 32), TEG.param_count(3, 32)
    assert P == 201684 + 288 * 3 + 256 * 64
    assert e.lib.efe_param_count(e.ctx, b'qs_net_g') == P and e.lib.efe_param_count(e.ctx, b'down_g') == PD
    assert e.lib.efe_param_count(e.ctx, b'qs_net') == 0 and e.lib.efe_param_count(e.ctx, b'down') == 0
    g = torch.zeros(PD, device='cuda:0')
    hp = daimc_amd._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    for part, n in ((b'qs_net_g', P), (b'down_g', PD)):
        rc = e.lib.efe_adam_step(e.ctx, part, ptr(g), ptr(g), ptr(g), C.byref(hp), e.stream())
        assert rc == 1 and 'efe_adam_step' in e.lib.efe_last_error(e.ctx).decode(), part
        rc = e.lib.efe_get_weights(e.ctx, part, ptr(g), n, e.stream())
        assert rc == 1 and 'efe_get_weights' in e.lib.efe_last_error(e.ctx).decode(), part
    assert raw_call(m, 1)[0] == 0
    m64 = model_for('g115', G64)
    e64 = m64._ready()
    assert e64.lib.efe_param_count(e64.ctx, b'qs_net_g') == e64.lib.efe_param_count(e64.ctx, b'qs_net') == 349428
    assert e64.lib.efe_param_count(e64.ctx, b'down_g') == e64.lib.efe_param_count(e64.ctx, b'down') == 4787125


def test_weight_update_macs_and_second_call_allocates_nothing():
    geo, M = G44, 17
    m = model_for('g115', geo, fresh=True)
    e = m._ready()
    o, gm, gv = case(geo, M)
    old = engine('g115', geo, o, gm, gv, model=m)
    w = {k: np.array(v) for k, v in family('g115', geo).items()}
    w['down.qs_net.18.bias'] = w['down.qs_net.18.bias'] + np.float32(0.25)
    w['down.qs_net.2.weight'] = (w['down.qs_net.2.weight'] * np.float32(0.75)).astype(np.float32)
    m.load_flat_weights(w)
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    eng = engine('g115', geo, o, gm, gv, model=m)
    assert not np.array_equal(eng['y'][1], old['y'][1]) and not np.array_equal(eng['mean'], old['mean'])
    hold('updated weights', w, geo, o, gm, gv, eng)
    H = TEG.extents(44)
    assert e.lib.efe_last_call_macs(e.ctx) == 3 * M * (288 * H[0] ** 2 + 9216 * H[1] ** 2 + 18432 * H[2] ** 2 + 36864 * H[3] ** 2 + 256 * 64 + 136192)
    st0 = m.arena_stats()
    again = engine('g115', geo, o, gm, gv, model=m)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1['grow_count'] == st0['grow_count'] and st1['high_water_bytes'] == st0['high_water_bytes'] and st1['capacity_bytes'] == st0['capacity_bytes']
    assert all(np.array_equal(again['grads'][k], eng['grads'][k]) for k in TEG.ENC_KEYS)
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before
