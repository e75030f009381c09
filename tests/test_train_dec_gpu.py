"""GPU tests (-m gpu) of the backward of the reconstruction loss through the decoder's ConvTranspose2d tail (csrc/train_dec.hip,
loss.grad_decoder_convs, efe_dec_tail_grad) against tests/train_dec_ref.py -- conv_transpose2d autograd on the CPU in fp32 and fp64,
itself pinned bit for bit to the reference's own po_net[12:] by tests/test_train_dec_cpu.py.

Inputs: train_dec_ref.inputs(seed, M): h4 = 2 relu(N(0, 1)) Bernoulli(0.5), o1 = Bernoulli(0.1).  The engine is called with
return_activations=True and BOTH oracles take their ReLU gates from the engine's y1..y3, so an fp32 ReLU decision on a pre-activation
within rounding of zero is not counted as a kernel error; test_gate_condition keeps that override from hiding a wrong gate.  Every
parameter tensor, d_h4, y1..y3 and po1 (image=True) are held to the project's fp64 rule (tests/test_fp64_parity.py fp64_rule, alpha 4,
beta 8), nlogpo1 to tests/test_free_energy_gpu.py's sumtol.

WALK_M = 33: the weight-gradient kernels run G = min(M, 32) slabs (csrc/kernels.h DEC_TAIL_SLABS) and row m belongs to slab m mod G, so at
M = 33 the workgroups of slab 0 walk a second image (rows 0 and 32)."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_dec_ref as TD
from oracle import synth
from test_fp64_parity import fp64_rule
from test_free_energy_gpu import sumtol

pytestmark = pytest.mark.gpu

SEED = 7
WALK_M = 32 + 1
GEO = (4, 1, 64)


def c(t):
    return t.detach().cpu().numpy()


_FAMILIES, _MODELS, _ENG, _ORC = {}, {}, {}, {}


def family(name, geo=GEO):
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


def model_for(name, geo=GEO, fresh=False):
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


def engine(fam, h4, o1, scale=None):
    """-> dict of numpy arrays with train_dec_ref.run's names"""
    import daimc_amd
    nl, po1, d_h4, g, ys = daimc_amd.loss.grad_decoder_convs(model_for(fam).model_down, h4, o1, scale=scale, return_activations=True)
    assert list(g) == list(TD.KEYS)
    flat = next(iter(g.values()))
    assert sum(v.numel() for v in g.values()) == TD.P and flat.dtype == torch.float32
    return dict(nlogpo1=c(nl), po1=c(po1), d_h4=c(d_h4), grads={k: c(v) for k, v in g.items()}, y=tuple(c(y) for y in ys))


def apply_rule(tag, rows, enforce=True):
    """fp64_rule on [(name, eng, o32, o64, image)]; every figure is printed before the assertion"""
    bad = []
    for name, eng, o32, o64, image in rows:
        for r in fp64_rule(name, eng, o32, o64, image):
            print(f'{tag} {r[0]}: e_eng {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}')
            if not r[-1]:
                bad.append(r)
    if enforce:
        assert not bad, f'{tag}: ' + '; '.join(f'{n}: e_eng {e:.3e} > bound {b:.3e} (e_32 {e3:.3e})' for n, e, e3, b, _, _ in bad)


def rule_rows(eng, o32, o64):
    rows = [(k, eng['grads'][k], o32['grads'][k], o64['grads'][k], False) for k in TD.KEYS]
    rows.append(('d_h4', eng['d_h4'], o32['d_h4'], o64['d_h4'], False))
    rows += [(f'y{i + 1}', eng['y'][i], o32['y'][i], o64['y'][i], False) for i in range(3)]
    rows.append(('po1', eng['po1'], o32['po1'], o64['po1'], True))
    return rows


def check(tag, fam, h4, o1, enforce=True):
    """the engine against both oracles gated by the engine's activations -> the engine's outputs"""
    eng = engine(fam, h4, o1)
    w = family(fam)
    o32 = TD.run(w, h4, o1, torch.float32, gates=eng['y'])
    o64 = TD.run(w, h4, o1, torch.float64, gates=eng['y'])
    print(f'{tag} nlogpo1: max err {np.abs(eng["nlogpo1"] - o32["nlogpo1"]).max():.3e} tol {sumtol(o32["nlogpo1"]):.3e}')
    apply_rule(tag, rule_rows(eng, o32, o64), enforce)
    if enforce:
        np.testing.assert_allclose(eng['nlogpo1'], o32['nlogpo1'], rtol=0, atol=sumtol(o32['nlogpo1']), err_msg=tag + ' nlogpo1')
    return eng


def cached_engine(fam, M):
    if (fam, M) not in _ENG:
        h4, o1 = TD.inputs(1000 + M, M)
        _ENG[fam, M] = (h4, o1, engine(fam, h4, o1))
    return _ENG[fam, M]


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', M) for M in (1, 2, 5, WALK_M)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 2, 5)]


@pytest.mark.parametrize('fam,M', GRAD_CASES)
def test_gradients_vs_fp64(fam, M):
    h4, o1 = TD.inputs(1000 + M, M)
    eng = check(f'{fam} M={M}', fam, h4, o1)
    _ENG.setdefault((fam, M), (h4, o1, eng))
    assert all(np.isfinite(v).all() for v in eng['grads'].values())


# ---- 2. gate condition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fam,M', [(f, M) for f in ('g115', 'g100', 'sparse') for M in (1, 5)])
def test_gate_condition(fam, M):
    """the engine's gates against the fp64 oracle's OWN ReLUs: they may differ only where |a_64| <= 1e-5, on at most 1e-4 of a layer"""
    h4, o1, eng = cached_engine(fam, M)
    own = TD.run(family(fam), h4, o1, torch.float64)
    for li in range(3):
        a64 = own['a'][li]
        diff = (eng['y'][li] > 0) != (a64 > 0)
        worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
        print(f'{fam} M={M} layer {li + 1}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}')
        assert worst <= 1e-5, (li, worst)
        assert diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()))


# ---- 3. row independence and determinism -----------------------------------------------------------------------------
def test_rows_are_independent_and_calls_reproducible():
    M, scale = 5, 0.25
    h4, o1 = TD.inputs(2005, M)
    a = engine('g115', h4, o1, scale=scale)
    b = engine('g115', h4, o1, scale=scale)
    for k in ('nlogpo1', 'po1', 'd_h4'):
        assert np.array_equal(a[k], b[k]), k
    for i in range(3):
        assert np.array_equal(a['y'][i], b['y'][i]), i
    for k in TD.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for r in range(M):
        one = engine('g115', h4[r:r + 1], o1[r:r + 1], scale=scale)
        for k in ('nlogpo1', 'po1', 'd_h4'):
            assert np.array_equal(one[k][0], a[k][r]), (k, r)
        for i in range(3):
            assert np.array_equal(one['y'][i][0], a['y'][i][r]), (i, r)


def test_nlogpo1_is_the_free_energy_kernels_sum():
    """k_fe_down's expression and reduction order: efe_loss_down on the same image gives the same bits.  (compute_loss_down decodes its
    own sample, so the comparison goes through the documented order instead: a CPU replay of the 256-thread sum on the engine's po1)"""
    h4, o1, eng = cached_engine('g115', 2)
    p, x = eng['po1'].reshape(2, 4096), o1.reshape(2, 4096)
    f = np.float32
    for r in range(2):
        t = (x[r] * np.log(f(0.00001) + p[r]).astype(f) + (f(1) - x[r]) * np.log(f(1.00001) - p[r]).astype(f)).astype(f)
        lanes = np.zeros(256, f)
        for j in range(16):
            lanes = (lanes + t[256 * j:256 * (j + 1)]).astype(f)
        waves = lanes.reshape(4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            waves = (waves + waves[:, np.arange(64) ^ off]).astype(f)
        s = f(f(f(waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0])
        # (logf on the device and numpy's log may differ in the last place: the sum of 4096 terms moves by a few ulp of the largest)
        np.testing.assert_allclose(eng['nlogpo1'][r], -s, rtol=2e-6)


# ---- 4. borders ------------------------------------------------------------------------------------------------------
def border_case(name):
    h4, o1 = TD.inputs(3002, 2)
    if name == 'h4_ring':
        x = h4.reshape(2, 64, 16, 16).copy()
        x[:, :, 1:-1, 1:-1] = 0
        ring = np.zeros((16, 16), bool)
        ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
        x[:, :, ring] = np.abs(x[:, :, ring]) + 0.5
        h4 = x.reshape(2, 16384)
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


@pytest.mark.parametrize('name', ['h4_ring', 'o1_ring', 'h4_zero', 'o1_zero', 'o1_one'])
def test_borders(name):
    h4, o1 = border_case(name)
    check(f'border {name}', 'g115', h4, o1)


# ---- 5. saturation ---------------------------------------------------------------------------------------------------
def test_saturated_outputs_are_finite():
    """family `saturated`: fp32 p rounds to 1, where the reference's own error is unbounded -- the rule's rows are printed, not asserted"""
    h4, o1 = TD.inputs(4002, 2)
    eng = check('saturated M=2', 'saturated', h4, o1, enforce=False)
    for k in ('nlogpo1', 'po1', 'd_h4'):
        assert np.isfinite(eng[k]).all(), k
    assert all(np.isfinite(v).all() for v in eng['grads'].values()) and all(np.isfinite(y).all() for y in eng['y'])


# ---- 6. bad arguments ------------------------------------------------------------------------------------------------
def raw_call(m, M, *, h4=True, o1=True, nl=True, grad=True):
    e = m._ready()
    n = max(M, 1)
    t = [torch.zeros(n * 16384, device='cuda:0'), torch.zeros(n * 4096, device='cuda:0'), torch.zeros(n, device='cuda:0'),
         torch.zeros(TD.P, device='cuda:0')]
    p = [C.c_void_p(x.data_ptr()) if use else None for x, use in zip(t, (h4, o1, nl, grad))]
    rc = e.lib.efe_dec_tail_grad(e.ctx, p[0], p[1], M, C.c_float(-1.0), C.c_float(1.0), p[2], None, None, p[3], None, None, None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


@pytest.mark.parametrize('kw', [dict(M=0), dict(M=-3), dict(M=1, h4=False), dict(M=1, o1=False), dict(M=1, nl=False), dict(M=1, grad=False)])
def test_bad_arguments_fail_cleanly(kw):
    rc, msg = raw_call(model_for('g115'), **kw)
    assert rc == 1 and 'efe_dec_tail_grad' in msg, (rc, msg)
    rc, _ = raw_call(model_for('g115'), 1)          # and the context still works
    assert rc == 0


def test_other_geometry_is_refused():
    import daimc_amd
    geo = (3, 3, 32)
    m = model_for('g115', geo)
    rc, msg = raw_call(m, 1)
    assert rc == 1 and 'efe_dec_tail_grad' in msg and '64' in msg, (rc, msg)
    with pytest.raises(ValueError):
        daimc_amd.loss.grad_decoder_convs(m.model_down, np.zeros((1, 16384), np.float32), np.zeros((1, 1, 64, 64), np.float32))
    e = m._ready()
    assert e.lib.efe_param_count(e.ctx, b'mid') == 0


def test_split_operand_options_are_refused():
    m = model_for('g115', fresh=True)
    e = m._ready()
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_call(m, 1)
        assert rc == 1 and 'efe_dec_tail_grad' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    assert raw_call(m, 1)[0] == 0


def test_param_count_and_no_adam_for_this_part():
    m = model_for('g115')
    e = m._ready()
    assert e.lib.efe_param_count(e.ctx, b'po_net_convt') == TD.P == 36928 + 36928 + 18464 + 289
    g = torch.zeros(TD.P, device='cuda:0')
    hp = __import__('daimc_amd')._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    rc = e.lib.efe_adam_step(e.ctx, b'po_net_convt', C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), C.byref(hp), e.stream())
    assert rc == 1 and 'efe_adam_step' in e.lib.efe_last_error(e.ctx).decode()


# ---- 7. no side effects ----------------------------------------------------------------------------------------------
def test_gradient_call_has_no_side_effects():
    m = model_for('g115')
    e = m._ready()
    s = np.random.RandomState(5).randn(3, 10).astype(np.float32)
    before = c(m.model_down.decoder(s, stage=2))
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    h4, o1 = TD.inputs(5003, 3)
    engine('g115', h4, o1)
    assert np.array_equal(c(m.model_down.decoder(s, stage=2)), before)
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before


def test_weight_update_reaches_the_raw_copy():
    """efe_set_weight + efe_commit_weights of a po_net.1[3579] tensor: the gradient call reads the new values"""
    m = model_for('g115', fresh=True)
    h4, o1 = TD.inputs(6001, 1)
    import daimc_amd
    w = {k: np.array(v) for k, v in family('g115').items()}
    w['down.po_net.19.bias'] = w['down.po_net.19.bias'] + np.float32(0.5)
    w['down.po_net.15.weight'] = (w['down.po_net.15.weight'] * np.float32(0.75)).astype(np.float32)
    m.load_flat_weights(w)
    nl, po1, d_h4, g, ys = daimc_amd.loss.grad_decoder_convs(m.model_down, h4, o1, return_activations=True)
    eng = dict(nlogpo1=c(nl), po1=c(po1), d_h4=c(d_h4), grads={k: c(v) for k, v in g.items()}, y=tuple(c(y) for y in ys))
    o32 = TD.run(w, h4, o1, torch.float32, gates=eng['y'])
    o64 = TD.run(w, h4, o1, torch.float64, gates=eng['y'])
    apply_rule('updated weights', rule_rows(eng, o32, o64))
