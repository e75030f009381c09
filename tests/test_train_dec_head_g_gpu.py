"""GPU tests (-m gpu) of the backward of the reconstruction loss through the whole decoder at every admitted geometry
(csrc/train_dec_head_g.hip + csrc/train_dec_g.hip, loss.grad_decoder_g, efe_dec_grad_g) against tests/train_dec_head_g_ref.py -- F.linear /
conv_transpose2d autograd on the CPU in fp32 and fp64 with the Philox dropout masks as multiplications, which at (1, 64) is
tests/train_dec_head_ref.py and elsewhere decodes oracle.efe_oracle's image, bit for bit (tests/test_train_dec_head_g_cpu.py).

Engine seed 7, stage 3, the default pass (PASS_FE_DOWN), inputs train_dec_head_g_ref.inputs(1000 + M, M, C, R), weights by oracle.synth as
in tests/test_train_dec_g_gpu.py.  The engine is called with return_activations=True and BOTH oracles take their seven gates from the
engine's h1..h4 and y1..y3; test_masks_and_gates keeps that override from hiding a wrong gate or a wrongly keyed mask.  Every parameter
tensor, d_s, h1..h4, y1..y3 and po1 (image=True) are held to the project's fp64 rule (tests/test_fp64_parity.py fp64_rule, alpha 4, beta 8),
nlogpo1 to tests/test_generic_geometry.py's sumtol against the fp32 oracle.

Geometries are (pi_dim, C, R); B = R / 4 (16 at R = 32), F = 64 B^2 features of po_net.9, S = ceil(F / 256) segments of d_h3.  B = 9: a
wave's 16 features straddle channel boundaries with odd B^2 (81), the last segment is ragged, S = 21 = 8 + 8 + 5.  B = 10: straddling
with even B^2, S = 25.  B = 16 / 32: whole tiles, the largest index ranges, S = 256.  Rows per pass are 64 (B <= 16) or 32: M = 65 at B = 9
and M = 33 at B = 17 make a second row group add into dW_3 and the slabs; M = 33 and 65 tell the tile's index in the call from its index
in the group (slab = global tile index mod 4)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import train_dec_head_g_ref as THG
import train_dec_head_ref as TH
from test_generic_geometry import sumtol
from test_train_dec_g_gpu import _FAMILIES, _MODELS, apply_rule, c, family, model_for

pytestmark = pytest.mark.gpu

STAGE = 3
ACT = ('h1', 'h2', 'h3', 'h4', 'y1', 'y2', 'y3')
PER_ROW = ('nlogpo1', 'po1', 'd_s')
G36, G40, G84, G32, G64, G128, G68 = (4, 1, 36), (4, 1, 40), (3, 3, 84), (3, 3, 32), (4, 3, 64), (4, 2, 128), (4, 1, 68)
_ENG = {}


def as_dict(out):
    nl, po1, d_s, g, act = out
    act = tuple(c(a) for a in act)
    return dict(nlogpo1=c(nl), po1=c(po1), d_s=c(d_s), grads={k: c(v) for k, v in g.items()}, h=act[:4], y=act[4:])


def engine(fam, geo, s, o1, scale=None, model=None, **key):
    """-> dict of numpy arrays with train_dec_head_g_ref.run's names"""
    import daimc_amd
    m = model or model_for(fam, geo)
    out = daimc_amd.loss.grad_decoder_g(m.model_down, s, o1, scale=scale, stage=key.pop('stage', STAGE), return_activations=True, **key)
    nl, po1, d_s, g, act = out
    _, Cc, R = geo
    B, M = THG.base_of(R), s.shape[0]
    assert list(g) == list(THG.KEYS) and len(act) == 7
    assert sum(v.numel() for v in g.values()) == THG.param_count(Cc, R) and next(iter(g.values())).dtype == torch.float32
    assert tuple(po1.shape) == (M, Cc, R, R) and tuple(d_s.shape) == (M, 10) and tuple(nl.shape) == (M,)
    assert [tuple(a.shape) for a in act] == [(M, 256)] * 3 + [(M, 64 * B * B), (M, 64, B, B), (M, 64, 2 * B, 2 * B), (M, 32, R, R)]
    return as_dict(out)


def rule_rows(eng, o32, o64, keys=THG.KEYS):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in keys]
    rows.append(('d_s', eng['d_s'], o32['d_s'], o64['d_s'], False))
    rows += [(f'h{i + 1}', eng['h'][i], o32['h'][i], o64['h'][i], False) for i in range(4)]
    rows += [(f'y{i + 1}', eng['y'][i], o32['y'][i], o64['y'][i], False) for i in range(3)]
    rows.append(('po1', eng['po1'], o32['po1'], o64['po1'], True))
    return rows


def oracles(w, geo, s, o1, eng, **key):
    gates = eng['h'] + eng['y']
    return tuple(THG.run(w, s, o1, geo[1], geo[2], STAGE, dt, gates=gates, **key) for dt in (torch.float32, torch.float64))


def hold(tag, w, geo, s, o1, eng, **key):
    """`eng` against both oracles gated by its own activations -> (o32, o64)"""
    o32, o64 = oracles(w, geo, s, o1, eng, **key)
    print(f'{tag} nlogpo1: max err {np.abs(eng["nlogpo1"] - o32["nlogpo1"]).max():.3e} tol {sumtol(o32["nlogpo1"]):.3e}')
    apply_rule(tag, rule_rows(eng, o32, o64))
    np.testing.assert_allclose(eng['nlogpo1'], o32['nlogpo1'], rtol=0, atol=sumtol(o32['nlogpo1']), err_msg=tag + ' nlogpo1')
    return o32, o64


def check(tag, fam, geo, s, o1):
    eng = engine(fam, geo, s, o1)
    hold(tag, family(fam, geo), geo, s, o1, eng)
    return eng


def cached_engine(fam, geo, M):
    if (fam, geo, M) not in _ENG:
        s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
        _ENG[fam, geo, M] = (s, o1, engine(fam, geo, s, o1))
    return _ENG[fam, geo, M]


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', G36, M) for M in (1, 2, 5, 33, 65)] + [('g115', G40, 2), ('g115', G84, 1), ('g115', G84, 2), ('g115', G32, 1), ('g115', G32, 5),
                                                               ('g115', G64, 2), ('g115', G128, 1), ('g115', G68, 33)]
GRAD_CASES += [(f, geo, M) for f in ('g100', 'sparse') for geo in (G36, G84) for M in (1, 2)]


@pytest.mark.parametrize('fam,geo,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, geo, M):
    s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
    eng = check(f'{fam} {geo} M={M}', fam, geo, s, o1)
    _ENG.setdefault((fam, geo, M), (s, o1, eng))
    assert all(np.isfinite(v).all() for v in eng['grads'].values())


# ---- 2. every admitted resolution -------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', list(range(32, 129, 4)))
def test_sweep_of_all_resolutions(R):
    geo = (4, 1 + (R // 4) % 3, R)
    s, o1 = THG.inputs(1001, 1, geo[1], R)
    check(f'sweep {geo}', 'g115', geo, s, o1)
    _MODELS.pop(('g115', geo), None)                  # one context per resolution: hand its device memory back
    _FAMILIES.pop(('g115', geo), None)
    _ENG.pop(('g115', geo, 1), None)


# ---- 3. masks and gates ----------------------------------------------------------------------------------------------
def gates_within_cap(tag, ga, gb, a64):
    """two gate sets may differ only where |a_64| <= 1e-5, on at most 1e-4 of a layer"""
    for li, (x, y, a) in enumerate(zip(ga, gb, a64)):
        diff = (x > 0) != (y.reshape(x.shape) > 0)
        worst = float(np.abs(a.reshape(x.shape)[diff]).max()) if diff.any() else 0.0
        print(f'{tag} {ACT[li]}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}')
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))


@pytest.mark.parametrize('fam,geo,M', [('g115', G36, 5), ('g115', G84, 2), ('g115', G32, 2), ('g115', G128, 1), ('sparse', G36, 2), ('g100', G84, 1)])
def test_masks_and_gates(fam, geo, M):
    """head: h_l > 0 only where the oracle's Philox mask bit is set (exact; layer 3 in the NHWC transposition), and against the fp64
    oracle's OWN pre-activations the gate may differ from mask * [a_64 > 0] only where |a_64| <= 1e-5, on at most 1e-4 of a layer;
    tail: the same condition on [y > 0] against [a_64 > 0]"""
    s, o1, eng = cached_engine(fam, geo, M)
    own = THG.run(family(fam, geo), s, o1, geo[1], geo[2], STAGE, torch.float64)
    for li in range(4):
        h, mask = eng['h'][li], own['masks'][li]
        assert h.shape == mask.shape
        outside = int(((h > 0) & (mask == 0)).sum())
        print(f'{fam} {geo} M={M} head layer {li}: {int((h > 0).sum())} of {h.size} kept, {outside} outside the mask')
        assert outside == 0, li
    want = [own['masks'][li] * (own['a_head'][li] > 0) for li in range(4)] + [own['a'][li] for li in range(3)]
    gates_within_cap(f'{fam} {geo} M={M}', eng['h'] + eng['y'], want, own['a_head'] + own['a'][:3])


# ---- 4. composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geo,M,scale', [(G36, 65, None), (G84, 5, 0.25)])
def test_tail_is_grad_decoder_convs_g_on_the_returned_h4(geo, M, scale):
    import daimc_amd
    s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
    eng = engine('g115', geo, s, o1, scale=scale)
    nl, po1, _, g, ys = daimc_amd.loss.grad_decoder_convs_g(model_for('g115', geo).model_down, eng['h'][3], o1, scale=scale, return_activations=True)
    assert np.array_equal(c(nl), eng['nlogpo1']) and np.array_equal(c(po1), eng['po1'])
    for i in range(3):
        assert np.array_equal(c(ys[i]), eng['y'][i]), i
    for k, v in g.items():
        assert np.array_equal(c(v), eng['grads'][k]), k


@pytest.mark.parametrize('geo', [G84, G36])
def test_forward_decoder_agrees_with_po1(geo):
    """model_down.decoder with the same keys decodes the same network (the same masks): its image meets the fp64 rule against the oracle
    that the gradient call is held to"""
    import daimc_amd
    s, o1, eng = cached_engine('g115', geo, 5)
    o32, o64 = oracles(family('g115', geo), geo, s, o1, eng)
    po = c(model_for('g115', geo).model_down.decoder(s, stage=STAGE, pass_=daimc_amd.model.PASS_FE_DOWN)).reshape(eng['po1'].shape)
    print(f'max |decoder - grad_decoder_g po1| {np.abs(po - eng["po1"]).max():.3e}')
    apply_rule(f'forward decoder {geo}', [('po1', po, o32['po1'], o64['po1'], True)])


# ---- 5. cross-check against the specialised kernels at 1 x 64 x 64 ----------------------------------------------------
@pytest.mark.parametrize('M', [2, 33])
def test_cross_check_at_1x64x64(M):
    import daimc_amd
    geo = (4, 1, 64)
    w = family('g115', geo)
    s, o1 = THG.inputs(1000 + M, M, 1, 64)
    m = model_for('g115', geo)
    g = engine('g115', geo, s, o1)
    sp = as_dict(daimc_amd.loss.grad_decoder(m.model_down, s, o1, stage=STAGE, return_activations=True))
    ref = None
    for tag, eng in ((f'1x64x64 M={M} run-time geometry', g), (f'1x64x64 M={M} specialised', sp)):
        o32, o64 = (TH.run(w, s, o1, STAGE, dt, gates=eng['h'] + eng['y']) for dt in (torch.float32, torch.float64))
        print(f'{tag} nlogpo1: max err {np.abs(eng["nlogpo1"] - o32["nlogpo1"]).max():.3e} tol {sumtol(o32["nlogpo1"]):.3e}')
        apply_rule(tag, rule_rows(eng, o32, o64, TH.KEYS))
        np.testing.assert_allclose(eng['nlogpo1'], o32['nlogpo1'], rtol=0, atol=sumtol(o32['nlogpo1']), err_msg=tag)
        ref = o32
    np.testing.assert_allclose(g['nlogpo1'], sp['nlogpo1'], rtol=0, atol=sumtol(ref['nlogpo1']))
    own = TH.run(w, s, o1, STAGE, torch.float64)
    gates_within_cap(f'1x64x64 M={M} both engines', g['h'] + g['y'], sp['h'] + sp['y'], own['a_head'] + own['a'][:3])


# ---- 6. row independence and determinism -----------------------------------------------------------------------------
def test_rows_are_independent_and_calls_reproducible():
    M, scale, geo, ro = 5, 0.25, G84, 7
    s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
    a = engine('g115', geo, s, o1, scale=scale, row_offset=ro)
    b = engine('g115', geo, s, o1, scale=scale, row_offset=ro)
    for k in PER_ROW:
        assert np.array_equal(a[k], b[k]), k
    for i, (x, y) in enumerate(zip(a['h'] + a['y'], b['h'] + b['y'])):
        assert np.array_equal(x, y), ACT[i]
    for k in THG.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', geo, s[r:r + 1], o1[r:r + 1], scale=scale, row_offset=ro + r)
        for k in PER_ROW:
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
        for i, (x, y) in enumerate(zip(one['h'] + one['y'], a['h'] + a['y'])):
            assert np.array_equal(x[0], y[r]), (ACT[i], r)
    other = engine('g115', geo, s, o1, scale=scale)          # another row offset draws other masks
    assert not np.array_equal(other['h'][3] > 0, a['h'][3] > 0)


# ---- 7. raw calls: padding rows and refusals -------------------------------------------------------------------------
def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def raw_call(m, M, *, s=True, o1=True, nz=True, nl=True, grad=True, scale=-1.0, beta_o=1.0, fn='efe_dec_grad_g'):
    import daimc_amd
    e = m._ready()
    Cc, R = int(m.colour_channels), int(m.resolution)
    n = max(M, 1)
    t = [torch.zeros(n * 10, device='cuda:0'), torch.zeros(n * Cc * R * R, device='cuda:0'), torch.zeros(n, device='cuda:0'),
         torch.zeros(THG.param_count(Cc, R), device='cuda:0')]
    p = [ptr(x) if use else None for x, use in zip(t, (s, o1, nl, grad))]
    noise = daimc_amd._lib.EfeNoise(7, STAGE, THG.PASS_FE_DOWN, 0, 0)
    rc = getattr(e.lib, fn)(e.ctx, p[0], p[1], M, C.c_float(scale), C.c_float(beta_o), C.byref(noise) if nz else None, p[2], None, None, p[3],
                            None, None, None, None, None, None, None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


def test_padding_rows_feed_zeros_not_memory():
    """caller-owned h1..h4 one tile longer than M, NaN beyond row M - 1: the same gradient bits as the clean call, and nothing stored there"""
    import daimc_amd
    geo, M = G36, 17
    m = model_for('g115', geo)
    e = m._ready()
    s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
    clean = engine('g115', geo, s, o1)
    F = THG.n_feat(geo[2])
    dev = dict(device='cuda:0')
    hb = [torch.full((M + 16, w), float('nan'), **dev) for w in (256, 256, 256, F)]
    ts, to = torch.tensor(s, **dev), torch.tensor(o1, **dev)
    nl, ds, grad = torch.zeros(M, **dev), torch.zeros(M, 10, **dev), torch.zeros(THG.param_count(geo[1], geo[2]), **dev)
    noise = daimc_amd._lib.EfeNoise(7, STAGE, THG.PASS_FE_DOWN, 0, 0)
    rc = e.lib.efe_dec_grad_g(e.ctx, ptr(ts), ptr(to), M, C.c_float(-1.0), C.c_float(1.0), C.byref(noise), ptr(nl), None, ptr(ds), ptr(grad),
                              ptr(hb[0]), ptr(hb[1]), ptr(hb[2]), ptr(hb[3]), None, None, None, e.stream())
    torch.cuda.synchronize()
    assert rc == 0, e.lib.efe_last_error(e.ctx).decode()
    flat, off = c(grad), 0
    for k in THG.KEYS:
        n = clean['grads'][k].size
        assert np.array_equal(flat[off:off + n], clean['grads'][k].ravel()), k
        off += n
    assert off == flat.size and np.array_equal(c(ds), clean['d_s']) and np.array_equal(c(nl), clean['nlogpo1'])
    for i in range(4):
        h = c(hb[i])
        assert np.array_equal(h[:M], clean['h'][i]) and np.isnan(h[M:]).all(), ACT[i]


def test_nan_in_one_row_stays_in_its_row():
    """one NaN in row 1's s: every element that is NaN in the fp32 autograd oracle (its own ReLUs and masks) is NaN in the engine, and the
    per-row outputs of rows 0 and 2 are those of the clean call, bit for bit"""
    geo, M = G36, 3
    s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
    clean = engine('g115', geo, s, o1)
    bad = s.copy()
    bad[1, 4] = np.nan
    eng = engine('g115', geo, bad, o1)
    orc = THG.run(family('g115', geo), bad, o1, geo[1], geo[2], STAGE, torch.float32)
    pairs = [(k, eng[k], orc[k]) for k in PER_ROW] + [(ACT[i], x, y) for i, (x, y) in enumerate(zip(eng['h'] + eng['y'], orc['h'] + orc['y']))]
    pairs += [(k, eng['grads'][k], orc['grads'][k]) for k in THG.KEYS]
    for name, e, o in pairs:
        on = np.isnan(o.reshape(e.shape))
        print(f'{name}: {int(on.sum())} NaN in the oracle, {int(np.isnan(e).sum())} in the engine')
        assert np.isnan(e[on]).all(), name
    assert np.isnan(orc['nlogpo1'][1]) and np.isnan(orc['grads']['po_net.9.weight']).any()
    for r in (0, 2):
        for k in PER_ROW:
            assert np.array_equal(eng[k][r], clean[k][r]), (k, r)
        for i, (x, y) in enumerate(zip(eng['h'] + eng['y'], clean['h'] + clean['y'])):
            assert np.array_equal(x[r], y[r]), (ACT[i], r)


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, s=False), dict(M=1, o1=False), dict(M=1, nz=False), dict(M=1, nl=False),
                                dict(M=1, grad=False), dict(M=1, scale=float('nan')), dict(M=1, scale=-1.0, beta_o=float('inf')),
                                dict(M=1, scale=-1.0, beta_o=float('nan'))])
def test_bad_arguments_fail_cleanly(kw):
    m = model_for('g115', G36)
    rc, msg = raw_call(m, **kw)
    assert rc == 1 and 'efe_dec_grad_g' in msg, (rc, msg)
    rc, _ = raw_call(m, 1)          # and the context still works
    assert rc == 0


def test_split_operand_options_are_refused():
    m = model_for('g115', (4, 1, 64), fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_dec_grad_g' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_bad_scale_raises_before_the_engine():
    import daimc_amd
    s, o1 = THG.inputs(1001, 1, G36[1], G36[2])
    for scale in (-0.5, float('nan')):
        with pytest.raises(ValueError):
            daimc_amd.loss.grad_decoder_g(model_for('g115', G36).model_down, s, o1, scale=scale)


def test_the_other_entry_points_still_refuse():
    import daimc_amd
    m = model_for('g115', G32)
    e = m._ready()
    rc, msg = raw_call(m, 1, fn='efe_dec_grad')
    assert rc == 1 and 'efe_dec_grad' in msg and 'efe_dec_grad_g' not in msg and '64' in msg, (rc, msg)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_decoder(m.model_down, np.zeros((1, 10), np.float32), np.zeros((1, 3, 32, 32), np.float32))
    P = THG.param_count(3, 32)
    assert e.lib.efe_param_count(e.ctx, b'po_net') == P
    g = torch.zeros(P, device='cuda:0')
    hp = daimc_amd._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    rc = e.lib.efe_adam_step(e.ctx, b'po_net', ptr(g), ptr(g), ptr(g), C.byref(hp), e.stream())
    assert rc == 1 and 'efe_adam_step' in e.lib.efe_last_error(e.ctx).decode()
    rc = e.lib.efe_get_weights(e.ctx, b'po_net', ptr(g), P, e.stream())
    assert rc == 1 and 'efe_get_weights' in e.lib.efe_last_error(e.ctx).decode()
    assert raw_call(m, 1)[0] == 0


# ---- 8. weights, MACs, scratch ---------------------------------------------------------------------------------------
def test_weight_update_macs_and_second_call_allocates_nothing():
    geo, M = G36, 2
    m = model_for('g115', geo, fresh=True)
    e = m._ready()
    s, o1 = THG.inputs(1000 + M, M, geo[1], geo[2])
    old = engine('g115', geo, s, o1, model=m)
    w = {k: np.array(v) for k, v in family('g115', geo).items()}
    w['down.po_net.9.bias'] = w['down.po_net.9.bias'] + np.float32(0.5)
    w['down.po_net.3.weight'] = (w['down.po_net.3.weight'] * np.float32(0.75)).astype(np.float32)
    m.load_flat_weights(w)
    eng = engine('g115', geo, s, o1, model=m)
    assert not np.array_equal(eng['h'][1], old['h'][1]) and not np.array_equal(eng['po1'], old['po1'])
    hold('updated weights', w, geo, s, o1, eng)
    B, R, Cc = 9, 36, 1
    tail = 3 * M * (2 * 64 * 64 * 9 * B * B + 64 * 32 * 9 * 4 * B * B + 32 * Cc * 9 * R * R)
    assert e.lib.efe_last_call_macs(e.ctx) == 3 * M * (2560 + 131072 + 256 * 64 * B * B) + tail
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    del old

    def settled():
        """device bytes held by torch once every tensor that is only garbage (of this test or an earlier one, cycles included) is freed"""
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()
    mem0, st0 = settled(), m.arena_stats()
    again = engine('g115', geo, s, o1, model=m)
    mem1, st1 = settled(), m.arena_stats()
    print('arena', st0, st1, 'torch', mem0, mem1)
    assert mem1 == mem0
    assert st1['grow_count'] == st0['grow_count'] and st1['high_water_bytes'] == st0['high_water_bytes'] and st1['capacity_bytes'] == st0['capacity_bytes']
    assert all(np.array_equal(again['grads'][k], eng['grads'][k]) for k in THG.KEYS)
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before
