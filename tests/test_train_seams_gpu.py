"""GPU tests (-m gpu) of the training calls at every row-group, head-tile and slab seam of the batch: loss.grad_down (csrc/train_enc.hip
around csrc/train_dec_head.hip + csrc/train_dec.hip), loss.grad_down_g (their _g forms), the parts they are composed of, and the optimiser
steps train_model_down / train_model_down_g, whose group loops are csrc/engine_train.hip's (DecGrad, DecGradG, EncGrad, EncGradG,
down_grad_run, down_grad_g_run).

A batch of M rows is cut into row groups of 64 rows (the 1 x 64 x 64 family and every geometry with base B = R / 4 <= 16) or 32 rows
(B > 16: R >= 68).  Row m adds to conv slab m mod G, G = min(M, 32); the 16-row tile t of the call adds to head slab t mod 4; the first
group writes a slab element and later groups add to it (tests/train_seams.py holds the table, tests/test_train_seams_cpu.py ties it to
csrc/kernels.h and shows that the fp64 rule rejects a gradient that lost one seam row).

    M           reaches
    31, 32      G = M against G = 32, no slab with a second image (33 is covered by the neighbouring files)
    64          exactly one full 64-row group / exactly two full 32-row groups
    96, 97      a second 64-row group of 32 / 33 rows: every slab once more / slab 0 twice
    128         two full groups and no third
    129, 130    a third group of 1 / 2 rows: `first` is false a second time, most slabs untouched in it
    257         train_step's largest tested batch: a fifth group of one row

    (4, 1, 64)  all of the above, by the specialised family (grad_down) and by the _g family; 257 once, by grad_down (what train_step runs)
    (4, 1, 68)  the smallest resolution with B > 16: 32-row groups, K = 576; M = 32, 64, 65 (a third group, head tile 4 wraps onto slab
                0), 97 (four groups, head tile 6)
    (4, 1, 44)  64-row groups in the _g family with even extents; M = 64, 129

Engine seed 7, stage 3, weights 'g115', inputs train_enc_g_ref.inputs(2000 + M, M, C, R) (at (1, 64) train_down_ref.inputs(2000 + M, M)),
as the neighbouring files.  The references are tests/train_enc_g_ref.py, train_dec_head_g_ref.py and train_dec_g_ref.py, which at (1, 64)
are the specialised family's references bit for bit (tests/test_train_enc_g_cpu.py and its neighbours).  Both oracles take the engine's
own fourteen gates, exactly as tests/test_train_down_gpu.check and tests/test_train_down_g_gpu.check do; all 32 tensors, g_mean,
g_logvar, mean, logvar, qs1, kl_s and kl_naive are held to the project's fp64 rule (alpha 4, beta 8), po1 with image=True, F_down and
nlogpo1 to sumtol: tests/test_free_energy_gpu.py's (stated for 4 096-term sums) up to resolution 64, tests/test_generic_geometry.py's at
(4, 1, 68), each as the family's own check uses it."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_train_down_g_gpu as GG
import test_train_down_gpu as SP
import test_train_down_step_g_gpu as STG
import test_train_down_step_gpu as ST
import train_dec_g_ref as TG
import train_dec_head_g_ref as THG
import train_enc_g_ref as TEG
import train_seams as TS
from test_fp64_parity import fp64_rule
from test_free_energy_gpu import sumtol as fe_sumtol
from test_generic_geometry import sumtol as g_sumtol
from test_train_dec_g_gpu import apply_rule, c, family, model_for
from test_train_dec_g_gpu import rule_rows as tail_rule_rows

pytestmark = pytest.mark.gpu

STAGE = TS.STAGE
G44, G64, G68 = TS.G44, TS.G64, TS.G68
PER_ROW = GG.PER_ROW
KEYS = TEG.KEYS
# (family, geometry, M): 'sp' the specialised 1 x 64 x 64 calls, 'g' the run-time-geometry calls
GRAD_CASES = [('sp', geo, M) for geo, M in TS.CASES if geo == G64] + [('g', geo, M) for geo, M in TS.CASES if M != TS.M_MAX]
PART_CASES = [('sp',) + TS.THREE_GROUPS[0], ('g',) + TS.THREE_GROUPS[0], ('g',) + TS.THREE_GROUPS[1]]
ROW_CASES = [('sp',) + TS.ROW_CASES[0], ('g',) + TS.ROW_CASES[1]]
KEPT = set(PART_CASES + ROW_CASES)           # the engine's outputs and the slim references of these cases are shared by the tests below
_ENG, _REF = {}, {}


def sumtol_of(geo):
    return fe_sumtol if geo[2] <= 64 else g_sumtol


def engine(kind, geo, inp, model=None, **kw):
    m = model or model_for('g115', geo)
    if kind == 'sp':
        return SP.engine('g115', *inp, model=m, **kw)
    return GG.engine('g115', geo, *inp, model=m, **kw)


def case(kind, geo, M):
    """-> (inputs, the engine's outputs with the gates of its parts); computed once for the cases several tests share"""
    key = (kind, geo, M)
    if key in _ENG:
        return _ENG[key]
    inp = TS.inputs(geo, M)
    out = (inp, engine(kind, geo, inp, gates=True))
    if key in KEPT:
        _ENG[key] = out
    return out


def hold(tag, kind, geo, inp, eng):
    """the composed call against both oracles on its own gates -> (o32, o64) without their activations"""
    oracles = SP.oracles(family('g115', geo), *inp, eng) if kind == 'sp' else GG.oracles(family('g115', geo), geo, *inp, eng)
    o32, o64 = ({k: v for k, v in o.items() if not isinstance(v, tuple)} for o in oracles)
    tol = sumtol_of(geo)
    for k in ('F_down', 'nlogpo1'):
        print(f'{tag} {k}: max err {np.abs(eng[k] - o32[k]).max():.3e} tol {tol(o32[k]):.3e}')
    rows = GG.rule_rows(eng, o32, o64)
    worst = max((r[4], r[0]) for name, e, a, b, image in rows for r in fp64_rule(name, e, a, b, image))
    print(f'SEAM {tag}: worst fp64-rule ratio {worst[0]:.2f} ({worst[1]})')
    apply_rule(tag, rows)
    for k in ('F_down', 'nlogpo1'):
        np.testing.assert_allclose(eng[k], o32[k], rtol=0, atol=tol(o32[k]), err_msg=f'{tag} {k}')
    assert all(np.isfinite(v).all() for v in eng['grads'].values())
    return o32, o64


def refs(kind, geo, M):
    key = (kind, geo, M)
    if key in _REF:
        return _REF[key]
    inp, eng = case(kind, geo, M)
    out = hold(f'{kind} {geo} M={M}', kind, geo, inp, eng)
    if key in KEPT:
        _REF[key] = out
    return out


def same_outputs(tag, a, b, keys=PER_ROW + ('g_mean', 'g_logvar')):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), f'{tag}: {k} differs'
    for k in KEYS:
        assert a['grads'][k].tobytes() == b['grads'][k].tobytes(), f'{tag}: gradient {k} differs'


# ---- 1. the composed gradient vs fp64 at every table entry -------------------------------------------------------------
@pytest.mark.parametrize('kind,geo,M', GRAD_CASES, ids=TS.ids(GRAD_CASES))
def test_gradients_vs_fp64(kind, geo, M):
    assert list(KEYS) == list(SP.TDN.KEYS) and len(KEYS) == 32
    refs(kind, geo, M)


# ---- 2. the parts at a three-group batch -------------------------------------------------------------------------------
def part_calls(kind):
    import daimc_amd
    L = daimc_amd.loss
    return (L.grad_decoder_convs, L.grad_decoder, L.grad_encoder) if kind == 'sp' else (L.grad_decoder_convs_g, L.grad_decoder_g, L.grad_encoder_g)


@pytest.mark.parametrize('kind,geo,M', PART_CASES, ids=TS.ids(PART_CASES))
def test_parts_are_the_composed_call(kind, geo, M):
    """grad_decoder(qs1, o1), grad_encoder(o1, g_mean, g_logvar) and grad_decoder_convs on the returned h4 give the composed call's
    gradients, po1 and nlogpo1 bit for bit, with and without returned activations (the caller's arrays / one group's scratch); d_s meets
    the fp64 rule against the composed oracles' gradient at qs1"""
    (o1, pm, pv, om), eng = case(kind, geo, M)
    o32, o64 = refs(kind, geo, M)
    tail, dec, enc = part_calls(kind)
    md = model_for('g115', geo).model_down
    tag = f'{kind} {geo} M={M}'
    nl, po1, d_s, gd = dec(md, eng['qs1'], o1, stage=STAGE)
    nl2, po2, d_s2, gd2, act = dec(md, eng['qs1'], o1, stage=STAGE, return_activations=True)
    for x, y in ((nl, nl2), (po1, po2), (d_s, d_s2)):
        assert np.array_equal(c(x), c(y))
    assert np.array_equal(c(nl), eng['nlogpo1']) and np.array_equal(c(po1), eng['po1'])
    assert list(gd) == list(THG.KEYS) == list(KEYS[16:])
    for k in gd:
        assert np.array_equal(c(gd[k]), eng['grads'][k]) and np.array_equal(c(gd2[k]), eng['grads'][k]) and np.array_equal(eng['dec_grads'][k], eng['grads'][k]), k
    for i, a in enumerate(act):
        assert np.array_equal(c(a), eng['dec_gates'][i]), i
    apply_rule(tag + ' grad_decoder', [('d_s', c(d_s), o32['d_s'], o64['d_s'], False)])
    mean, lv, ge = enc(md, o1, eng['g_mean'], eng['g_logvar'], stage=STAGE)
    assert np.array_equal(c(mean), eng['mean']) and np.array_equal(c(lv), eng['logvar'])
    assert list(ge) == list(TEG.ENC_KEYS) == list(KEYS[:16])
    for k in ge:
        assert np.array_equal(c(ge[k]), eng['grads'][k]) and np.array_equal(eng['enc_grads'][k], eng['grads'][k]), k
    # the tail alone on the caller's h4
    h4 = eng['dec_gates'][3]
    tnl, tpo, d_h4, gt = tail(md, h4, o1)
    tnl2, tpo2, d_h42, gt2, ys = tail(md, h4, o1, return_activations=True)
    for x, y in ((tnl, tnl2), (tpo, tpo2), (d_h4, d_h42)):
        assert np.array_equal(c(x), c(y))
    assert np.array_equal(c(tnl), eng['nlogpo1']) and np.array_equal(c(tpo), eng['po1'])
    assert list(gt) == list(TG.KEYS)
    for k in gt:
        assert np.array_equal(c(gt[k]), eng['grads'][k]) and np.array_equal(c(gt2[k]), eng['grads'][k]), k
    for i in range(3):
        assert np.array_equal(c(ys[i]), eng['dec_gates'][4 + i]), i
    te = dict(nlogpo1=c(tnl), po1=c(tpo), d_h4=c(d_h4), grads={k: c(v) for k, v in gt.items()}, y=tuple(c(y) for y in ys))
    w = family('g115', geo)
    t32, t64 = (TG.run(w, h4, o1, geo[1], geo[2], dt, gates=te['y']) for dt in (torch.float32, torch.float64))
    tol = sumtol_of(geo)(t32['nlogpo1'])
    print(f'{tag} grad_decoder_convs nlogpo1: max err {np.abs(te["nlogpo1"] - t32["nlogpo1"]).max():.3e} tol {tol:.3e}')
    apply_rule(tag + ' grad_decoder_convs', tail_rule_rows(te, t32, t64))
    np.testing.assert_allclose(te['nlogpo1'], t32['nlogpo1'], rtol=0, atol=tol)


@pytest.mark.parametrize('kind,geo,M', PART_CASES, ids=TS.ids(PART_CASES))
def test_gates_of_the_later_groups(kind, geo, M):
    """the activations that grad_encoder / grad_decoder return for the rows of the second and third group against the fp64 references' OWN
    ReLUs and masks on those rows (row_offset = the second group's first row): the existing gate condition"""
    (o1, pm, pv, om), eng = case(kind, geo, M)
    r0 = TS.rows_per_group(geo)
    assert M > 2 * r0
    w = family('g115', geo)
    tag = f'{kind} {geo} M={M} rows {r0}..{M - 1}'
    own = TEG.run_encoder(w, o1[r0:], eng['g_mean'][r0:], eng['g_logvar'][r0:], geo[1], geo[2], STAGE, torch.float64, row_offset=r0)
    for i in range(4):
        TS.gate_diff(f'{tag} y{i + 1}', eng['gates'][i][r0:], own['a_conv'][i] > 0, own['a_conv'][i])
    for i in range(3):
        mask = own['enc_masks'][i]
        TS.gate_diff(f'{tag} h{i + 1}', eng['gates'][4 + i][r0:], (mask > 0) & (own['a_dense'][i] > 0), own['a_dense'][i], mask=mask)
    own = THG.run(w, eng['qs1'][r0:], o1[r0:], geo[1], geo[2], STAGE, torch.float64, row_offset=r0)
    for i in range(4):
        mask = own['masks'][i]
        TS.gate_diff(f'{tag} dec h{i + 1}', eng['dec_gates'][i][r0:], (mask > 0) & (own['a_head'][i] > 0), own['a_head'][i], mask=mask)
    for i in range(3):
        TS.gate_diff(f'{tag} dec y{i + 1}', eng['dec_gates'][4 + i][r0:], own['a'][i] > 0, own['a'][i])


# ---- 3. rows do not see the seams --------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,geo,M', ROW_CASES, ids=TS.ids(ROW_CASES))
def test_rows_do_not_see_the_seams(kind, geo, M):
    """the per-row outputs of one call are those of one call per row group (rows m0 .. m0 + rows, row_offset = m0) and of single-row calls
    on each side of every seam, bit for bit (g_mean / g_logvar carry 1 / M and are left out); two calls at the same M agree in every
    output, a call on another stage does not"""
    inp, a = case(kind, geo, M)
    same_outputs(f'{kind} {geo} M={M} second call', a, engine(kind, geo, inp))
    rows = TS.rows_per_group(geo)
    seams = list(range(rows, M, rows))
    assert len(seams) >= 2
    for m0 in [0] + seams:
        n = min(rows, M - m0)
        one = engine(kind, geo, tuple(x[m0:m0 + n] for x in inp), row_offset=m0)
        for k in PER_ROW:
            assert one[k].tobytes() == a[k][m0:m0 + n].tobytes(), (k, m0)
    for r in sorted({s + d for s in seams for d in (-1, 0)}):
        one = engine(kind, geo, tuple(x[r:r + 1] for x in inp), row_offset=r)
        for k in PER_ROW:
            assert one[k][0].tobytes() == a[k][r].tobytes(), (k, r)
    other = engine(kind, geo, inp, stage=STAGE + 1)
    assert not np.array_equal(other['qs1'], a['qs1']) and not np.array_equal(other['mean'], a['mean'])
    assert not np.array_equal(other['grads'][KEYS[0]], a['grads'][KEYS[0]])


# ---- 4. the optimiser step across the seam -----------------------------------------------------------------------------
def master(m, kind, geo):
    """the master copy through the C ABI"""
    e = m._ready()
    P = TEG.param_count(geo[1], geo[2])
    buf = torch.empty(P, device='cuda:0')
    get = e.lib.efe_down_get_weights if kind == 'sp' else e.lib.efe_down_get_weights_g
    assert get(e.ctx, C.c_void_p(buf.data_ptr()), P, e.stream()) == 0, e.lib.efe_last_error(e.ctx).decode()
    return c(buf)


STEP_CASES = [('sp',) + TS.THREE_GROUPS[0], ('g',) + TS.THREE_GROUPS[1]]


@pytest.mark.parametrize('kind,geo,M', STEP_CASES, ids=TS.ids(STEP_CASES))
def test_training_call_is_grad_then_adam_at_a_third_group(kind, geo, M):
    """train_model_down / train_model_down_g equal grad_down / grad_down_g followed by Adam.step over two steps, bit for bit: weights,
    master copy, exp_avg, exp_avg_sq and the step count.  With test 1 and tests/test_train_step_gpu.py's `step == the sequence of calls`
    at M = 257 this ties train_step to the fp64 reference at the batch it is tested at."""
    import daimc_amd
    b = TS.inputs(geo, M)
    ma, mb = model_for('g115', geo, fresh=True), model_for('g115', geo, fresh=True)
    if kind == 'sp':
        oa, ob = daimc_amd.Adam(ma.model_down, lr=1e-3), daimc_amd.Adam(mb.model_down.parameters(), lr=1e-3)
        train, grad = ST.train, ST.grad
    else:
        oa, ob = STG.adam(ma, lr=1e-3), daimc_amd.Adam(mb.model_down.parameters(), lr=1e-3, any_geometry=True)
        train, grad = STG.train, STG.grad
    for _ in range(2):
        Fa, ta = train(ma, oa, b)
        out = grad(mb, b)
        ob.step(out[6])
        assert np.array_equal(c(Fa), c(out[0]))
        STG.same_bits('terms', ta, out[1])
    assert np.array_equal(master(ma, kind, geo), master(mb, kind, geo))
    sa, sb = STG.down_weights(ma), STG.down_weights(mb)
    for k in KEYS:
        assert np.array_equal(sa[k], sb[k]), k
        assert not np.array_equal(sa[k], family('g115', geo)['down.' + k]), k
    assert np.array_equal(master(ma, kind, geo), STG.flat_weights(sa))
    for x, y in zip(STG.opt_state(oa), STG.opt_state(ob)):
        assert np.array_equal(x, y)
    assert oa._step == ob._step == 2


# ---- 5. scratch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,geo,M', ROW_CASES, ids=TS.ids(ROW_CASES))
def test_scratch_is_sized_once_and_written_before_it_is_read(kind, geo, M):
    """a fresh model: the second call grows the arena by nothing; with the development option `poison` (every call starts on scratch
    filled with that byte: 0xff a NaN, 0x7f 3.4e38) the outputs keep every bit, so no slab element or group scratch is read before this
    call wrote it; and they are the outputs of the shared model, whose arena other calls have used"""
    inp, ref = case(kind, geo, M)
    m = model_for('g115', geo, fresh=True)
    tag = f'{kind} {geo} M={M}'
    a = engine(kind, geo, inp, model=m)
    st0 = m.arena_stats()
    b = engine(kind, geo, inp, model=m)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1['grow_count'] == st0['grow_count'] and st1['capacity_bytes'] == st0['capacity_bytes'] and st1['high_water_bytes'] == st0['high_water_bytes']
    same_outputs(tag + ' second call', a, b)
    same_outputs(tag + ' fresh model', a, ref)
    try:
        for byte in (0xff, 0x7f):
            m.set_option('poison', byte)
            same_outputs(f'{tag} poison {byte:#x}', a, engine(kind, geo, inp, model=m))
    finally:
        m.set_option('poison', -1)
    assert m.arena_stats()['grow_count'] == st0['grow_count']
