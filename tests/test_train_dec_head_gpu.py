"""GPU tests (-m gpu) of the backward of the reconstruction loss through the whole decoder (csrc/train_dec_head.hip + csrc/train_dec.hip,
loss.grad_decoder, efe_dec_grad) against tests/train_dec_head_ref.py -- F.linear / conv_transpose2d autograd on the CPU in fp32 and fp64
with the Philox dropout masks as multiplications, itself pinned bit for bit to the reference's own po_net by
tests/test_train_dec_head_cpu.py.

Engine seed 7, stage 3, the default pass (PASS_FE_DOWN), inputs train_dec_head_ref.inputs(2000 + M, M).  The engine is called with
return_activations=True and BOTH oracles take their seven gates from the engine's h1..h4 and y1..y3, so an fp32 ReLU decision on a
pre-activation within rounding of zero is not counted as a kernel error; test_masks_and_gates keeps that override from hiding a wrong
gate or a wrongly keyed mask.  All 16 parameter tensors, d_s, h1..h4, y1..y3 and po1 (image=True) are held to the project's fp64 rule
(tests/test_fp64_parity.py fp64_rule, alpha 4, beta 8, applied by test_train_dec_gpu.apply_rule), nlogpo1 to tests/test_free_energy_gpu.py's sumtol.

Sizes: M = 17 is two 16-row tiles, the second ragged; M = 33 makes the tail's slab 0 walk a second image; M = 65 is a second 64-row
group, where the head's weight gradient of po_net.9 and its slabs accumulate across groups."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_dec_head_ref as TH
from test_free_energy_gpu import sumtol
from test_train_dec_gpu import apply_rule, c, family, model_for

pytestmark = pytest.mark.gpu

STAGE = 3
ACT = ('h1', 'h2', 'h3', 'h4', 'y1', 'y2', 'y3')
_ENG = {}


def engine(fam, s, o1, scale=None, model=None, **key):
    """-> dict of numpy arrays with train_dec_head_ref.run's names"""
    import daimc_amd
    m = model or model_for(fam)
    nl, po1, d_s, g, act = daimc_amd.loss.grad_decoder(m.model_down, s, o1, scale=scale, stage=key.pop('stage', STAGE), return_activations=True, **key)
    assert list(g) == list(TH.KEYS) and len(act) == 7
    flat = next(iter(g.values()))
    assert sum(v.numel() for v in g.values()) == TH.P and flat.dtype == torch.float32
    act = tuple(c(a) for a in act)
    return dict(nlogpo1=c(nl), po1=c(po1), d_s=c(d_s), grads={k: c(v) for k, v in g.items()}, h=act[:4], y=act[4:])


def rule_rows(eng, o32, o64):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in TH.KEYS]
    rows.append(('d_s', eng['d_s'], o32['d_s'], o64['d_s'], False))
    rows += [(f'h{i + 1}', eng['h'][i], o32['h'][i], o64['h'][i], False) for i in range(4)]
    rows += [(f'y{i + 1}', eng['y'][i], o32['y'][i], o64['y'][i], False) for i in range(3)]
    rows.append(('po1', eng['po1'], o32['po1'], o64['po1'], True))
    return rows


def oracles(w, s, o1, eng, **key):
    gates = eng['h'] + eng['y']
    return tuple(TH.run(w, s, o1, STAGE, dt, gates=gates, **key) for dt in (torch.float32, torch.float64))


def check(tag, fam, s, o1, enforce=True):
    """the engine against both oracles gated by the engine's activations -> (engine outputs, o32, o64)"""
    eng = engine(fam, s, o1)
    o32, o64 = oracles(family(fam), s, o1, eng)
    print(f'{tag} nlogpo1: max err {np.abs(eng["nlogpo1"] - o32["nlogpo1"]).max():.3e} tol {sumtol(o32["nlogpo1"]):.3e}')
    apply_rule(tag, rule_rows(eng, o32, o64), enforce)
    if enforce:
        np.testing.assert_allclose(eng['nlogpo1'], o32['nlogpo1'], rtol=0, atol=sumtol(o32['nlogpo1']), err_msg=tag + ' nlogpo1')
    return eng, o32, o64


def cached_engine(fam, M):
    if (fam, M) not in _ENG:
        s, o1 = TH.inputs(2000 + M, M)
        _ENG[fam, M] = (s, o1, engine(fam, s, o1))
    return _ENG[fam, M]


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', M) for M in (1, 2, 5, 17, 33, 65)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)]


@pytest.mark.parametrize('fam,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, M):
    s, o1 = TH.inputs(2000 + M, M)
    eng, _, _ = check(f'{fam} M={M}', fam, s, o1)
    _ENG.setdefault((fam, M), (s, o1, eng))
    assert all(np.isfinite(v).all() for v in eng['grads'].values())


def test_saturated_outputs_are_finite():
    """family `saturated`: fp32 p rounds to 1, where the reference's own error is unbounded -- the rule's rows are printed, not asserted"""
    s, o1 = TH.inputs(2002, 2)
    eng, _, _ = check('saturated M=2', 'saturated', s, o1, enforce=False)
    for k in ('nlogpo1', 'po1', 'd_s'):
        assert np.isfinite(eng[k]).all(), k
    assert all(np.isfinite(v).all() for v in eng['grads'].values()) and all(np.isfinite(a).all() for a in eng['h'] + eng['y'])


# ---- 2. masks and gates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam,M', [('g115', M) for M in (1, 5, 17)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)])
def test_masks_and_gates(fam, M):
    """head: h_l > 0 only where the oracle's Philox mask bit is set (exact; layer 3 in the NHWC transposition), and against the fp64
    oracle's OWN pre-activations the gate may differ from mask * [a_64 > 0] only where |a_64| <= 1e-5, on at most 1e-4 of a layer;
    tail: the same condition on [y > 0] against [a_64 > 0]"""
    s, o1, eng = cached_engine(fam, M)
    own = TH.run(family(fam), s, o1, STAGE, torch.float64)
    for li in range(4):
        h, mask, a64 = eng['h'][li], own['masks'][li], own['a_head'][li]
        assert h.shape == mask.shape
        outside = int(((h > 0) & (mask == 0)).sum())
        diff = (h > 0) != ((mask > 0) & (a64 > 0))
        worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
        print(f'{fam} M={M} head layer {li}: {int((h > 0).sum())} of {h.size} kept, {outside} outside the mask, {int(diff.sum())} gates differ, '
              f'worst |a_64| {worst:.3e}')
        assert outside == 0, li
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))
    for li in range(3):
        a64 = own['a'][li]
        diff = (eng['y'][li] > 0) != (a64 > 0)
        worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
        print(f'{fam} M={M} tail layer {li + 1}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}')
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))


# ---- 3. composition --------------------------------------------------------------------------------------------------
def test_tail_is_grad_decoder_convs_on_the_returned_h4():
    import daimc_amd
    for M, scale in ((5, 0.25), (65, None)):
        s, o1 = TH.inputs(2000 + M, M)
        eng = engine('g115', s, o1, scale=scale)
        nl, po1, _, g = daimc_amd.loss.grad_decoder_convs(model_for('g115').model_down, eng['h'][3], o1, scale=scale)
        assert np.array_equal(c(nl), eng['nlogpo1']) and np.array_equal(c(po1), eng['po1']), M
        for k, v in g.items():
            assert np.array_equal(c(v), eng['grads'][k]), (M, k)


def test_forward_decoder_agrees_with_po1():
    """model_down.decoder with the same keys decodes the same network (the same masks): its image meets the fp64 rule against the oracle
    that the gradient call is held to"""
    import daimc_amd
    s, o1, eng = cached_engine('g115', 5)
    o32, o64 = oracles(family('g115'), s, o1, eng)
    po = c(model_for('g115').model_down.decoder(s, stage=STAGE, pass_=daimc_amd.model.PASS_FE_DOWN)).reshape(eng['po1'].shape)
    print(f'max |decoder - grad_decoder po1| {np.abs(po - eng["po1"]).max():.3e}')
    apply_rule('forward decoder', [('po1', po, o32['po1'], o64['po1'], True)])


# ---- 4. reproducibility and row independence ---------------------------------------------------------------------------
def test_rows_are_independent_and_calls_reproducible():
    M, scale = 5, 0.25
    s, o1 = TH.inputs(2005, M)
    a = engine('g115', s, o1, scale=scale)
    b = engine('g115', s, o1, scale=scale)
    for k in ('nlogpo1', 'po1', 'd_s'):
        assert np.array_equal(a[k], b[k]), k
    for i, (x, y) in enumerate(zip(a['h'] + a['y'], b['h'] + b['y'])):
        assert np.array_equal(x, y), ACT[i]
    for k in TH.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', s[r:r + 1], o1[r:r + 1], scale=scale, row_offset=r)
        for k in ('nlogpo1', 'po1', 'd_s'):
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
        for i, (x, y) in enumerate(zip(one['h'] + one['y'], a['h'] + a['y'])):
            assert np.array_equal(x[0], y[r]), (ACT[i], r)
    for key in (dict(stage=STAGE + 1), dict(sample=1)):
        other = engine('g115', s, o1, scale=scale, **key)
        for i in range(4):
            assert not np.array_equal(other['h'][i] > 0, a['h'][i] > 0), (key, i)


# ---- 5. boundary -----------------------------------------------------------------------------------------------------
def raw_call(m, M, *, s=True, o1=True, nz=True, nl=True, grad=True):
    import daimc_amd
    e = m._ready()
    n = max(M, 1)
    t = [torch.zeros(n * 10, device='cuda:0'), torch.zeros(n * 4096, device='cuda:0'), torch.zeros(n, device='cuda:0'),
         torch.zeros(TH.P, device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) if use else None for x, use in zip(t, (s, o1, nl, grad))]
    noise = daimc_amd._lib.EfeNoise(7, STAGE, TH.PASS_FE_DOWN, 0, 0)
    rc = e.lib.efe_dec_grad(e.ctx, p[0], p[1], M, C.c_float(-1.0), C.c_float(1.0), C.byref(noise) if nz else None, p[2], None, None, p[3],
                            None, None, None, None, None, None, None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, s=False), dict(M=1, o1=False), dict(M=1, nz=False), dict(M=1, nl=False),
                                dict(M=1, grad=False)])
def test_bad_arguments_fail_cleanly(kw):
    rc, msg = raw_call(model_for('g115'), **kw)
    assert rc == 1 and 'efe_dec_grad' in msg, (rc, msg)
    rc, _ = raw_call(model_for('g115'), 1)          # and the context still works
    assert rc == 0


def test_other_geometry_is_refused():
    import daimc_amd
    m = model_for('g115', (3, 3, 32))
    rc, msg = raw_call(m, 1)
    assert rc == 1 and 'efe_dec_grad' in msg and '64' in msg, (rc, msg)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_decoder(m.model_down, np.zeros((1, 10), np.float32), np.zeros((1, 1, 64, 64), np.float32))


def test_bad_scale_is_refused():
    import daimc_amd
    s, o1 = TH.inputs(2001, 1)
    for scale in (-0.5, float('nan')):
        with pytest.raises(ValueError):
            daimc_amd.loss.grad_decoder(model_for('g115').model_down, s, o1, scale=scale)


def test_split_operand_options_are_refused():
    m = model_for('g115', fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_dec_grad' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_param_counts_and_no_adam_for_this_part():
    import daimc_amd
    m = model_for('g115')
    e = m._ready()
    assert e.lib.efe_param_count(e.ctx, b'po_net') == TH.P == 4437697
    assert e.lib.efe_param_count(e.ctx, b'po_net_convt') == 92609
    g = torch.zeros(TH.P, device='cuda:0')
    hp = daimc_amd._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    rc = e.lib.efe_adam_step(e.ctx, b'po_net', C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), C.byref(hp), e.stream())
    assert rc == 1 and 'efe_adam_step' in e.lib.efe_last_error(e.ctx).decode()
    rc = e.lib.efe_get_weights(e.ctx, b'po_net', C.c_void_p(g.data_ptr()), TH.P, e.stream())
    assert rc == 1 and 'efe_get_weights' in e.lib.efe_last_error(e.ctx).decode()


def test_gradient_call_has_no_side_effects_and_allocates_once():
    m = model_for('g115')
    e = m._ready()
    x = np.random.RandomState(5).randn(3, 10).astype(np.float32)
    before = c(m.model_down.decoder(x, stage=2))
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    s, o1 = TH.inputs(2017, 17)
    a = engine('g115', s, o1)
    st0 = m.arena_stats()
    b = engine('g115', s, o1)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1['grow_count'] == st0['grow_count'] and st1['high_water_bytes'] == st0['high_water_bytes'] and st1['capacity_bytes'] == st0['capacity_bytes']
    assert all(np.array_equal(a['grads'][k], b['grads'][k]) for k in TH.KEYS)
    assert np.array_equal(c(m.model_down.decoder(x, stage=2)), before)
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before


def test_weight_update_reaches_the_raw_copy():
    """load_flat_weights with a changed po_net.9.bias and po_net.3.weight: the gradient call reads the new values"""
    m = model_for('g115', fresh=True)
    s, o1 = TH.inputs(2002, 2)
    old = engine('g115', s, o1, model=m)
    w = {k: np.array(v) for k, v in family('g115').items()}
    w['down.po_net.9.bias'] = w['down.po_net.9.bias'] + np.float32(0.25)
    w['down.po_net.3.weight'] = (w['down.po_net.3.weight'] * np.float32(0.75)).astype(np.float32)
    m.load_flat_weights(w)
    eng = engine('g115', s, o1, model=m)
    assert not np.array_equal(eng['h'][1], old['h'][1]) and not np.array_equal(eng['po1'], old['po1'])
    o32, o64 = oracles(w, s, o1, eng)
    apply_rule('updated weights', rule_rows(eng, o32, o64))
