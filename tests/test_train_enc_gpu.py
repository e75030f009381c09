"""GPU tests (-m gpu) of the encoder's training forward and backward (csrc/train_enc.hip, loss.grad_encoder, efe_enc_grad) against
tests/train_down_ref.py -- F.conv2d / F.linear autograd on the CPU in fp32 and fp64 with the Philox dropout masks as multiplications,
itself pinned bit for bit to the reference's own compute_loss_down by tests/test_train_down_cpu.py.

Engine seed 7, stage 3, the default pass (PASS_FE_DOWN), images train_down_ref.inputs(2000 + M, M), upstream pair N(0, 1) / M.  The
engine is called with return_activations=True and BOTH oracles take their seven gates from the engine's y1..y4 and h1..h3, so an fp32
ReLU decision on a pre-activation within rounding of zero is not counted as a kernel error; test_masks_and_gates keeps that override
from hiding a wrong gate or a wrongly keyed mask.  All 16 parameter tensors, mean, logvar, y1..y4 and h1..h3 are held to the project's
fp64 rule (tests/test_fp64_parity.py fp64_rule, alpha 4, beta 8, applied by test_train_dec_gpu.apply_rule).

Sizes: M = 17 is two 16-row tiles, the second ragged; M = 33 makes the convolutions' slab 0 walk a second image; M = 65 is a second
64-row group, where every slab accumulates across groups.  Every extent of the network is odd (31, 15, 7, 3): each case runs ragged
position tiles on every layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_down_ref as TDN
from test_train_dec_gpu import apply_rule, c, family, model_for

pytestmark = pytest.mark.gpu

STAGE = 3
ACT = ('y1', 'y2', 'y3', 'y4', 'h1', 'h2', 'h3')
_ENG = {}


def engine(fam, o, gm, gv, model=None, **key):
    """-> dict of numpy arrays with train_down_ref.run_encoder's names"""
    import daimc_amd
    m = model or model_for(fam)
    mean, lv, g, act = daimc_amd.loss.grad_encoder(m.model_down, o, gm, gv, stage=key.pop('stage', STAGE), return_activations=True, **key)
    assert list(g) == list(TDN.ENC_KEYS) and len(act) == 7
    flat = next(iter(g.values()))
    assert sum(v.numel() for v in g.values()) == TDN.P_ENC and flat.dtype == torch.float32
    act = tuple(c(a) for a in act)
    return dict(mean=c(mean), logvar=c(lv), grads={k: c(v) for k, v in g.items()}, y=act[:4], h=act[4:])


def rule_rows(eng, o32, o64):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in TDN.ENC_KEYS]
    rows += [(k, eng[k], o32[k], o64[k], False) for k in ('mean', 'logvar')]
    rows += [(f'y{i + 1}', eng['y'][i], o32['y'][i], o64['y'][i], False) for i in range(4)]
    rows += [(f'h{i + 1}', eng['h'][i], o32['h'][i], o64['h'][i], False) for i in range(3)]
    return rows


def oracles(w, o, gm, gv, eng, **key):
    gates = eng['y'] + eng['h']
    return tuple(TDN.run_encoder(w, o, gm, gv, STAGE, dt, gates=gates, **key) for dt in (torch.float32, torch.float64))


def case(M):
    return TDN.inputs(2000 + M, M)[0], *TDN.upstream(2000 + M, M)


def cached_engine(fam, M):
    if (fam, M) not in _ENG:
        o, gm, gv = case(M)
        _ENG[fam, M] = (o, gm, gv, engine(fam, o, gm, gv))
    return _ENG[fam, M]


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', M) for M in (1, 2, 5, 17, 33, 65)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)]


@pytest.mark.parametrize('fam,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, M):
    o, gm, gv, eng = cached_engine(fam, M)
    o32, o64 = oracles(family(fam), o, gm, gv, eng)
    apply_rule(f'{fam} M={M}', rule_rows(eng, o32, o64))
    assert all(np.isfinite(v).all() for v in eng['grads'].values())


# ---- 2. masks and gates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam,M', [('g115', M) for M in (1, 5, 17)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)])
def test_masks_and_gates(fam, M):
    """head: h_l > 0 only where the oracle's Philox mask bit is set (exact), and against the fp64 oracle's OWN pre-activations the gate may
    differ from mask * [a_64 > 0] only where |a_64| <= 1e-5, on at most 1e-4 of a layer; convolutions: the same condition on [y > 0]"""
    o, gm, gv, eng = cached_engine(fam, M)
    own = TDN.run_encoder(family(fam), o, gm, gv, STAGE, torch.float64)
    for li in range(3):
        h, mask, a64 = eng['h'][li], own['enc_masks'][li], own['a_dense'][li]
        assert h.shape == mask.shape
        outside = int(((h > 0) & (mask == 0)).sum())
        diff = (h > 0) != ((mask > 0) & (a64 > 0))
        worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
        print(f'{fam} M={M} head layer {li}: {int((h > 0).sum())} of {h.size} kept, {outside} outside the mask, {int(diff.sum())} gates differ, '
              f'worst |a_64| {worst:.3e}')
        assert outside == 0, li
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))
    for li in range(4):
        a64 = own['a_conv'][li]
        assert eng['y'][li].shape == a64.shape
        diff = (eng['y'][li] > 0) != (a64 > 0)
        worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
        print(f'{fam} M={M} conv layer {li + 1}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}')
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))


# ---- 3. ragged edges -------------------------------------------------------------------------------------------------
def test_last_row_and_column_of_the_image_are_never_read():
    """an image whose only non-zero pixels are row 63 and column 63 gives the y1 and the qs_net.0 gradients of the all-zero image (and every
    other output with them)"""
    M = 2
    zero = np.zeros((M, 1, 64, 64), np.float32)
    edge = zero.copy()
    edge[:, :, 63, :] = 1.0
    edge[:, :, :, 63] = 3.0
    gm, gv = TDN.upstream(2002, M)
    a, b = engine('g115', zero, gm, gv), engine('g115', edge, gm, gv)
    assert np.array_equal(a['y'][0], b['y'][0]) and np.abs(a['y'][0]).max() > 0
    for k in TDN.ENC_KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    assert not np.any(a['grads']['qs_net.0.weight']) and np.any(a['grads']['qs_net.0.bias'])


def probe_weights():
    """weights that isolate one gradient path: qs_net.0 / .2 pass the centre tap only (bias 0), so the one-hot image (4 Y + 3, 4 X + 3) makes
    y2 one-hot at (Y, X) in every channel; qs_net.4 / .6 have a large bias (every y3, y4 > 0: open gates); qs_net.9 reads y4 pixel (2, 2)
    only, so dL / da4 is one-hot in space at (2, 2).  Then qs_net.4.weight's gradient [co][ci][ky][kx] is dL / da3[co] at the pixel
    ((Y - ky) / 2, (X - kx) / 2) times y2[ci][Y][X]: it shows where the data gradient of layer 4 put dL / da3"""
    w = {k: np.array(v) for k, v in family('g115').items()}
    for key, n in (('down.qs_net.0', 1.0), ('down.qs_net.2', 1.0 / 32)):
        t = np.zeros_like(w[key + '.weight'])
        t[:, :, 1, 1] = n
        w[key + '.weight'] = t
        w[key + '.bias'] = np.zeros_like(w[key + '.bias'])
    w['down.qs_net.4.bias'] = np.full_like(w['down.qs_net.4.bias'], 5.0)
    w['down.qs_net.6.bias'] = np.full_like(w['down.qs_net.6.bias'], 5.0)
    w['down.qs_net.6.weight'] = (w['down.qs_net.6.weight'] * np.float32(0.05)).astype(np.float32)       # (576 terms of y3 ~ 5 stay below the bias)
    w9 = w['down.qs_net.9.weight'].reshape(256, 64, 9).copy()
    w9[:, :, :8] = 0.0
    w['down.qs_net.9.weight'] = w9.reshape(256, 576)
    return w


def test_gradient_of_y4_pixel_2_2_reaches_y3_pixels_4_to_6_only():
    """a gradient that is one-hot in space on y4 pixel (2, 2) reaches y3 pixels (4..6, 4..6) only (observed through qs_net.4.weight's
    gradient under the probe weights), and the whole gradient still meets the fp64 rule"""
    import daimc_amd
    m = model_for('g115', fresh=True)
    w = probe_weights()
    m.load_flat_weights(w)
    gm, gv = TDN.upstream(2001, 1)
    # probe pixel (Y, X) of y2 -> the taps (ky, kx) of qs_net.4.weight's gradient that may be non-zero: y3 pixel ((Y - ky) / 2, (X - kx) / 2) in 4..6
    for (Y, X), taps in (((9, 9), {(1, 1)}), ((14, 14), {(2, 2)}), ((10, 12), {(0, 0), (0, 2), (2, 0), (2, 2)}), ((7, 10), set()), ((9, 6), set()),
                         ((8, 8), {(0, 0)})):
        o = np.zeros((1, 1, 64, 64), np.float32)
        o[0, 0, 4 * Y + 3, 4 * X + 3] = 1.0
        eng = engine('g115', o, gm, gv, model=m)
        y2 = eng['y'][1][0]
        assert np.count_nonzero(y2[0]) == 1 and y2[0, Y, X] == 1.0 and (eng['y'][2] > 0).all() and (eng['y'][3] > 0).all(), (Y, X)
        g = eng['grads']['qs_net.4.weight']
        for ky in range(3):
            for kx in range(3):
                if (ky, kx) in taps:
                    assert np.abs(g[:, :, ky, kx]).max() > 0, (Y, X, ky, kx)
                else:
                    assert not np.any(g[:, :, ky, kx]), (Y, X, ky, kx)
        if (Y, X) == (10, 12):
            o32, o64 = oracles(w, o, gm, gv, eng)
            apply_rule('probe weights', rule_rows(eng, o32, o64))


def test_padded_features_of_the_last_layer_feed_zeros():
    """qs_net.18.bias lies directly behind the 20 x 256 weight in the flat copy: with 1e30 there the 12 padded features of the last
    layer's tile must not leak into any output"""
    m = model_for('g115', fresh=True)
    w = {k: np.array(v) for k, v in family('g115').items()}
    w['down.qs_net.18.bias'] = np.full_like(w['down.qs_net.18.bias'], 1e30)
    m.load_flat_weights(w)
    o, gm, gv = case(5)
    eng = engine('g115', o, gm, gv, model=m)
    ref = cached_engine('g115', 5)[3]
    for k in ('mean', 'logvar'):
        assert np.isfinite(eng[k]).all() and (eng[k] > 1e29).all(), k
    assert all(np.isfinite(a).all() for a in eng['y'] + eng['h'])
    for k in TDN.ENC_KEYS:          # the bias enters no gradient: they are those of the unchanged weights, bit for bit
        assert np.isfinite(eng['grads'][k]).all() and np.array_equal(eng['grads'][k], ref['grads'][k]), k


# ---- 4. the forward encoder ------------------------------------------------------------------------------------------
def test_forward_encoder_agrees_with_mean_and_logvar():
    """model_down.encoder with the same keys encodes the same network (the same masks): its outputs meet the fp64 rule against the
    oracle that the gradient call is held to"""
    import daimc_amd
    o, gm, gv, eng = cached_engine('g115', 5)
    o32, o64 = oracles(family('g115'), o, gm, gv, eng)
    mean, lv = model_for('g115').model_down.encoder(o, stage=STAGE, pass_=daimc_amd.model.PASS_FE_DOWN)
    print(f'max |encoder - grad_encoder| mean {np.abs(c(mean) - eng["mean"]).max():.3e} logvar {np.abs(c(lv) - eng["logvar"]).max():.3e}')
    apply_rule('forward encoder', [('mean', c(mean), o32['mean'], o64['mean'], False), ('logvar', c(lv), o32['logvar'], o64['logvar'], False)])


# ---- 5. reproducibility and row independence ---------------------------------------------------------------------------
def test_rows_are_independent_and_calls_reproducible():
    M = 5
    o, gm, gv = case(M)
    a = engine('g115', o, gm, gv)
    b = engine('g115', o, gm, gv)
    for k in ('mean', 'logvar'):
        assert np.array_equal(a[k], b[k]), k
    for i, (x, y) in enumerate(zip(a['y'] + a['h'], b['y'] + b['h'])):
        assert np.array_equal(x, y), ACT[i]
    for k in TDN.ENC_KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', o[r:r + 1], gm[r:r + 1], gv[r:r + 1], row_offset=r)
        for k in ('mean', 'logvar'):
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
        for i, (x, y) in enumerate(zip(one['y'] + one['h'], a['y'] + a['h'])):
            assert np.array_equal(x[0], y[r]), (ACT[i], r)
    for key in (dict(stage=STAGE + 1), dict(sample=1)):
        other = engine('g115', o, gm, gv, **key)
        for i in range(3):
            assert not np.array_equal(other['h'][i] > 0, a['h'][i] > 0), (key, i)


# ---- 6. boundary -----------------------------------------------------------------------------------------------------
def raw_call(m, M, *, o=True, gm=True, gv=True, nz=True, grad=True):
    import daimc_amd
    e = m._ready()
    n = max(M, 1)
    t = [torch.zeros(n * 4096, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'), torch.zeros(n * 10, device='cuda:0'),
         torch.zeros(TDN.P_ENC, device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) if use else None for x, use in zip(t, (o, gm, gv, grad))]
    noise = daimc_amd._lib.EfeNoise(7, STAGE, TDN.PASS_FE_DOWN, 0, 0)
    rc = e.lib.efe_enc_grad(e.ctx, p[0], p[1], p[2], M, C.byref(noise) if nz else None, None, None, p[3], None, None, None, None, None, None, None,
                            e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, o=False), dict(M=1, gm=False), dict(M=1, gv=False), dict(M=1, nz=False),
                                dict(M=1, grad=False)])
def test_bad_arguments_fail_cleanly(kw):
    rc, msg = raw_call(model_for('g115'), **kw)
    assert rc == 1 and 'efe_enc_grad' in msg, (rc, msg)
    rc, _ = raw_call(model_for('g115'), 1)          # and the context still works
    assert rc == 0


def test_other_geometry_is_refused():
    import daimc_amd
    m = model_for('g115', (3, 3, 32))
    rc, msg = raw_call(m, 1)
    assert rc == 1 and 'efe_enc_grad' in msg and '64' in msg, (rc, msg)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_encoder(m.model_down, np.zeros((1, 1, 64, 64), np.float32), np.zeros((1, 10), np.float32), np.zeros((1, 10), np.float32))
    e = m._ready()
    assert e.lib.efe_param_count(e.ctx, b'qs_net') == 0 and e.lib.efe_param_count(e.ctx, b'down') == 0


def test_split_operand_options_are_refused():
    m = model_for('g115', fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_enc_grad' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_param_counts_and_no_adam_for_these_parts():
    import daimc_amd
    m = model_for('g115')
    e = m._ready()
    assert e.lib.efe_param_count(e.ctx, b'qs_net') == TDN.P_ENC == 349428
    assert e.lib.efe_param_count(e.ctx, b'down') == TDN.P == 4787125
    assert e.lib.efe_param_count(e.ctx, b'po_net') == 4437697 and e.lib.efe_param_count(e.ctx, b'mid') == 0
    g = torch.zeros(TDN.P, device='cuda:0')
    hp = daimc_amd._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    for part, n in ((b'qs_net', TDN.P_ENC), (b'down', TDN.P)):
        rc = e.lib.efe_adam_step(e.ctx, part, C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), C.byref(hp), e.stream())
        assert rc == 1 and 'efe_adam_step' in e.lib.efe_last_error(e.ctx).decode(), part
        rc = e.lib.efe_get_weights(e.ctx, part, C.c_void_p(g.data_ptr()), n, e.stream())
        assert rc == 1 and 'efe_get_weights' in e.lib.efe_last_error(e.ctx).decode(), part


def test_gradient_call_has_no_side_effects_and_allocates_once():
    m = model_for('g115')
    e = m._ready()
    x = TDN.inputs(2003, 3)[0]
    before = tuple(c(t) for t in m.model_down.encoder(x, stage=2))
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    o, gm, gv = case(17)
    a = engine('g115', o, gm, gv)
    st0 = m.arena_stats()
    b = engine('g115', o, gm, gv)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1['grow_count'] == st0['grow_count'] and st1['high_water_bytes'] == st0['high_water_bytes'] and st1['capacity_bytes'] == st0['capacity_bytes']
    assert all(np.array_equal(a['grads'][k], b['grads'][k]) for k in TDN.ENC_KEYS)
    after = tuple(c(t) for t in m.model_down.encoder(x, stage=2))
    assert all(np.array_equal(p, q) for p, q in zip(before, after))
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before


def test_weight_update_reaches_the_raw_copy():
    """load_flat_weights with a changed qs_net.2.weight and qs_net.18.bias: the gradient call reads the new values"""
    m = model_for('g115', fresh=True)
    o, gm, gv = case(2)
    old = engine('g115', o, gm, gv, model=m)
    w = {k: np.array(v) for k, v in family('g115').items()}
    w['down.qs_net.18.bias'] = w['down.qs_net.18.bias'] + np.float32(0.25)
    w['down.qs_net.2.weight'] = (w['down.qs_net.2.weight'] * np.float32(0.75)).astype(np.float32)
    m.load_flat_weights(w)
    eng = engine('g115', o, gm, gv, model=m)
    assert not np.array_equal(eng['y'][1], old['y'][1]) and not np.array_equal(eng['mean'], old['mean'])
    o32, o64 = oracles(w, o, gm, gv, eng)
    apply_rule('updated weights', rule_rows(eng, o32, o64))
