"""GPU tests (-m gpu) of non-finite propagation ("Non-finite values"): a NaN or an infinity in a state row, an observation
pixel, a prior entry or a weight comes out of every entry point where the reference puts it out -- relu(NaN) is NaN, a dropout mask
multiplies (NaN * 0 is NaN) and a NaN gate lets the upstream gradient through -- on the default fp32 path, at both geometries.

  C1  every output element that is NaN in the oracle is NaN in the engine, every element that is +-inf in the oracle is not finite in the
      engine.  The engine's non-finite set may be larger (the Winograd / F(2,2) input transforms mix a 4 x 4 tile), so no set equality.
  C2  a row whose oracle outputs are all finite is bit-identical to the same row of the same call on the clean batch (the poisoned element
      replaced by its healthy value; same stage, same row offsets).  Not applied to batch reductions (gradients, step means).
  Guard (every case): the oracle is not finite in each poisoned row and fully finite in every other row.

"Oracle" is the fp32 OracleModel (whose NaN positions are the reference's own: tests/test_oracle_golden.py
test_nonfinite_masks_vs_reference) for forward calls and the torch-autograd restatements train_ref / train_mid_ref / train_down_ref /
free_energy_ref for gradients and the training step.  No numeric tolerance anywhere: every assertion is an isnan / isfinite pattern or
equality of bits.  Engine seed 7, weights 'g115', explicit stage; the poisons are the four bit patterns of oracle/nonfinite.py (+NaN,
-NaN, +inf, -inf: a ReLU written as an integer maximum tells the two NaNs apart, arithmetic does not).  Sizes are the smallest that reach
each kernel family; each spec_* function builds the inputs and the oracle side of one test on the CPU, verify() adds the engine."""
import numpy as np
import pytest
import torch

import free_energy_ref as FR
import train_down_ref as TDN
import train_mid_ref as TM
import train_ref as TR
from oracle import efe_oracle as EO
from oracle import nonfinite as NF
from oracle import philox as PX
from oracle import synth
from train_common import SEED, c, family, model_for

pytestmark = pytest.mark.gpu

POISONS = list(NF.POISONS)
STAGE = 40
GEO32 = (4, 1, 32)
poisoned = NF.poisoned


def L():
    import daimc_amd
    return daimc_amd.loss


_ORC = {}


def oracle(geo=(4, 1, 64), weights=None):
    if weights is not None:
        return EO.OracleModel(weights, EO.PhiloxNoise(SEED), pi_dim=geo[0], channels=geo[1], resolution=geo[2])
    if geo not in _ORC:
        _ORC[geo] = EO.OracleModel(family('g115', geo), EO.PhiloxNoise(SEED), pi_dim=geo[0], channels=geo[1], resolution=geo[2])
    return _ORC[geo]


def engine_with(weights, geo=(4, 1, 64)):
    """a fresh engine model over the given (poisoned) weights, configured as train_common.model_for configures its own"""
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, geo[0], 0.5, 1.0, 1.0, colour_channels=geo[1], resolution=geo[2], device='cuda:0', seed=SEED,
                                       init_weights=False)
    m.load_flat_weights(weights)
    return m


def states(M):
    return PX.uniform_fill(3, (M, 10), 50 + M, -1.5, 1.5)


def actions(M):
    return np.eye(4, dtype=np.float32)[np.arange(M) % 4]


def poison_rows(a, rows, tail, poison):
    for r in rows:
        a = poisoned(a, (r,) + tuple(tail), poison)
    return a


def arrays(outs):
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    flat = []
    for o in outs:
        if isinstance(o, (tuple, list)):
            flat += list(o)
        else:
            flat.append(o)
    return [o.detach().cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o) for o in flat]


def rows2d(outs, M):
    return np.concatenate([np.asarray(a, dtype=np.float32).reshape(M, -1) for a in arrays(outs)], axis=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def guard(tag, orc, bad, M):
    """the vacuity guard on the oracle's row-wise outputs [M, n] -> mask of its non-finite rows"""
    o = rows2d(orc, M)
    nf = ~np.isfinite(o).all(axis=1)
    assert np.flatnonzero(nf).tolist() == sorted(bad), f'{tag}: the oracle is not finite in rows {np.flatnonzero(nf).tolist()}, poisoned rows {sorted(bad)}'
    return o, nf


def c1(tag, o, e):
    miss_nan = np.isnan(o) & ~np.isnan(e)
    miss_inf = np.isinf(o) & np.isfinite(e)
    print(f'{tag}: oracle NaN {int(np.isnan(o).sum())} inf {int(np.isinf(o).sum())} of {o.size}; engine NaN {int(np.isnan(e).sum())} '
          f'inf {int(np.isinf(e).sum())}; oracle-NaN not NaN in the engine {int(miss_nan.sum())}, oracle-inf finite in the engine {int(miss_inf.sum())}')
    assert o.shape == e.shape, tag
    assert not miss_nan.any(), f'{tag}: {int(miss_nan.sum())} elements are NaN in the oracle and not in the engine (first: {np.argwhere(miss_nan)[:4].tolist()})'
    assert not miss_inf.any(), f'{tag}: {int(miss_inf.sum())} elements are +-inf in the oracle and finite in the engine (first: {np.argwhere(miss_inf)[:4].tolist()})'


def c2(tag, nf, e, k):
    same = (bits(e) == bits(k)).all(axis=1)
    print(f'{tag}: healthy rows {int((~nf).sum())}, of them bit-identical to the clean batch {int((same & ~nf).sum())}')
    assert np.isfinite(k[~nf]).all(), f'{tag}: the clean batch is not finite in a healthy row'
    assert same[~nf].all(), f'{tag}: healthy rows {np.flatnonzero(~same & ~nf).tolist()} differ from the clean batch'


def verify(spec):
    """spec: dict(tag, M, bad, orc, eng, clean): orc the oracle's outputs on the poisoned batch, eng / clean callables -> the engine's outputs
    on the poisoned / on the clean batch"""
    tag, M = spec['tag'], spec['M']
    o, nf = guard(tag, spec['orc'], spec['bad'], M)
    e = rows2d(spec['eng'](), M)
    c1(tag, o, e)
    c2(tag, nf, e, rows2d(spec['clean'](), M))


def grads_c1(tag, ref, eng):
    """C1 on a gradient (or parameter) dictionary: {key: array} of the autograd restatement against the engine's"""
    n_ref = 0
    for k, g in ref.items():
        g = np.asarray(g, dtype=np.float32)
        n_ref += int((~np.isfinite(g)).sum())
        c1(f'{tag} {k}', g.reshape(1, -1), c(eng[k]).reshape(1, -1))
    assert n_ref > 0, f'{tag}: the restatement has no non-finite gradient element'


# ---- forward, 1 x 64 x 64 ------------------------------------------------------------------------------------------------
SMALL = [(5, (2,)), (65, (0, 63, 64))]           # M = 65: the two sides of a 16-row and of a 64-row tile edge


def spec_habit(M, bad, poison):
    s = states(M)
    sb = poison_rows(s, bad, (3,), poison)
    with torch.no_grad():
        orc = oracle().encode_s(torch.from_numpy(sb))
    return dict(tag=f'encode_s M={M} {poison}', M=M, bad=bad, orc=orc, eng=lambda: model_for('g115').model_top.encode_s(sb),
                clean=lambda: model_for('g115').model_top.encode_s(s))


def spec_transition(M, bad, poison):
    s, pi = states(M), actions(M)
    sb = poison_rows(s, bad, (3,), poison)
    with torch.no_grad():
        orc = oracle().transition_with_sample(torch.from_numpy(pi), torch.from_numpy(sb), PX.PASS_T1, 0, STAGE)
    run = lambda x: model_for('g115').model_mid.transition_with_sample(pi, x, stage=STAGE, pass_=PX.PASS_T1)          # noqa: E731
    return dict(tag=f'transition M={M} {poison}', M=M, bad=bad, orc=orc, eng=lambda: run(sb), clean=lambda: run(s))


def spec_decoder(N, bad, poison, geo=(4, 1, 64)):
    s = states(N)
    sb = poison_rows(s, bad, (3,), poison)
    with torch.no_grad():
        orc = oracle(geo).decoder(torch.from_numpy(sb), PX.PASS_D1, 0, STAGE)
    run = lambda x: model_for('g115', geo).model_down.decoder(x, stage=STAGE, pass_=PX.PASS_D1)          # noqa: E731
    return dict(tag=f'decoder {geo} N={N} {poison}', M=N, bad=bad, orc=orc, eng=lambda: run(sb), clean=lambda: run(s))


def frames_for(M, geo=(4, 1, 64)):
    return synth.make_frames(11, M) if geo == (4, 1, 64) else synth.make_frames_rgb(11, M, channels=geo[1], resolution=geo[2])


def spec_encoder(pixel, read, poison, geo=(4, 1, 64)):
    M, row = 5, 2
    o = frames_for(M, geo)
    ob = poisoned(o, (row, 0) + tuple(pixel), poison)
    with torch.no_grad():
        orc = oracle(geo).encoder_with_sample(torch.from_numpy(ob), PX.PASS_E1, 0, STAGE)
    run = lambda x: model_for('g115', geo).model_down.encoder_with_sample(x, stage=STAGE, pass_=PX.PASS_E1)          # noqa: E731
    return dict(tag=f'encoder {geo} pixel {pixel} {poison}', M=M, bad=(row,) if read else (), orc=orc, eng=lambda: run(ob), clean=lambda: run(o))


def spec_calculate_G(M, bad, poison):
    s, pi = states(M), actions(M)
    sb = poison_rows(s, bad, (3,), poison)
    with torch.no_grad():
        orc = oracle().calculate_G(torch.from_numpy(sb), torch.from_numpy(pi), 1, STAGE)
    run = lambda x: model_for('g115').calculate_G(x, pi, samples=1, stage=STAGE)          # noqa: E731
    return dict(tag=f'calculate_G M={M} {poison}', M=M, bad=bad, orc=orc, eng=lambda: run(sb), clean=lambda: run(s))


def spec_rollout(poison):
    M, row = 4, 1
    o, pi = frames_for(M), actions(M)
    ob = poisoned(o, (row, 0, 31, 31), poison)
    with torch.no_grad():
        orc = oracle().calculate_G_repeated(torch.from_numpy(ob), torch.from_numpy(pi), 2, False, 1, STAGE)
    run = lambda x: model_for('g115').calculate_G_repeated(x, pi, steps=2, samples=1, stage=STAGE)          # noqa: E731
    return dict(tag=f'calculate_G_repeated {poison}', M=M, bad=(row,), orc=orc, eng=lambda: run(ob), clean=lambda: run(o))


def spec_action_posterior(poison):
    G = PX.uniform_fill(5, (3, 4), 77, -30.0, 30.0)
    Gb = poisoned(G, (1, 2), poison)
    with np.errstate(all='ignore'):
        orc = EO.softmax_multi_with_log(-Gb, 4)
    run = lambda x: model_for('g115').action_posterior(x)          # noqa: E731
    return dict(tag=f'action_posterior {poison}', M=3, bad=(1,), orc=orc, eng=lambda: run(Gb), clean=lambda: run(G))


def fe_batch(M=5):
    r = np.random.RandomState(4100 + M)
    pi0 = np.eye(4, dtype=np.float32)[r.randint(0, 4, M)]
    lp = torch.log_softmax(torch.from_numpy(r.randn(M, 4).astype(np.float32)), 1).numpy()
    return synth.make_frames(300 + M, M), synth.make_frames(700 + M, M), pi0, lp


FE_WHERE = {'o0': (0, (2, 0, 31, 31)), 'o1': (1, (2, 0, 31, 31)), 'log_Ppi': (3, (2, 1))}


def spec_free_energy(where, poison):
    M = 5
    b = fe_batch(M)
    i, index = FE_WHERE[where]
    bb = b[:i] + (poisoned(b[i], index, poison),) + b[i + 1:]
    with torch.no_grad():
        r = FR.free_energy(oracle(), *bb, gamma=0.5, stage=STAGE)
    run = lambda x: [getattr(L().free_energy(model_for('g115'), *x, stage=STAGE), f) for f in FR.FIELDS]          # noqa: E731
    return dict(tag=f'free_energy {where} {poison}', M=M, bad=(2,), orc=[r[f] for f in FR.FIELDS], eng=lambda: run(bb), clean=lambda: run(b))


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('M,bad', SMALL)
def test_habit(M, bad, poison):
    verify(spec_habit(M, bad, poison))


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('M,bad', SMALL)
def test_transition(M, bad, poison):
    verify(spec_transition(M, bad, poison))


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('N,bad', [(5, (0, 4)), (130, (0, 64, 129))])         # k_dec_a_s / k_dec_b4<4>, then the persistent k_dec_a / k_dec_b4<1>
def test_decoder(N, bad, poison):
    verify(spec_decoder(N, bad, poison))


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('pixel,read', [((0, 0), True), ((31, 31), True), ((62, 62), True), ((63, 63), False)])
def test_encoder(pixel, read, poison):
    """(62, 62) is the last pixel the stride-2 convolutions read; (63, 63) is never read, the oracle stays finite and the row falls under C2"""
    verify(spec_encoder(pixel, read, poison))


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('M,bad', [(5, (2,)), (44, (0, 43))])                 # M = 44: 132 decoder images in one launch
def test_calculate_G(M, bad, poison):
    verify(spec_calculate_G(M, bad, poison))


@pytest.mark.parametrize('poison', POISONS)
def test_calculate_G_repeated(poison):
    verify(spec_rollout(poison))


@pytest.mark.parametrize('poison', POISONS)
def test_action_posterior(poison):
    verify(spec_action_posterior(poison))


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('where', list(FE_WHERE))
def test_free_energy(where, poison):
    verify(spec_free_energy(where, poison))


def spec_simulate(poison):
    E, T, ep = 3, 3, 1
    starts = PX.uniform_fill(4, (E, 10), 81, -1.0, 1.0)
    sb = poisoned(starts, (ep, 3), poison)
    orc = oracle()
    with torch.no_grad():
        per = [orc.mcts_step_simulate(torch.from_numpy(sb[e]), T, False, STAGE, episode=e) for e in range(E)]
    G = np.array([p[0] for p in per], dtype=np.float32)
    pi0 = np.stack([p[1].numpy() for p in per], 0)
    q = np.stack([p[2].numpy() for p in per], 0)
    return dict(tag=f'simulate_batch {poison}', E=E, T=T, ep=ep, starts=starts, sb=sb, G=G, pi0=pi0, q=q)


def guard_simulate(sp):
    ep, T = sp['ep'], sp['T']
    assert np.isnan(sp['G'][ep]) and np.isfinite(np.delete(sp['G'], ep)).all(), sp['G']
    assert np.array_equal(sp['pi0'][ep], np.eye(4, dtype=np.float32)[[0] * T]) and np.array_equal(sp['q'][ep], [1, 0, 0, 0])     # the fallback


@pytest.mark.parametrize('poison', POISONS)
def test_simulate_batch(poison):
    """a bad start row in episode 1 of 3: its G is NaN, its actions and Qpi are the reference's fallback (action 0 on every step, Qpi the
    one-hot: torchmodel.py's bare except), the neighbouring episodes are bit-identical to the clean batch"""
    sp = spec_simulate(poison)
    guard_simulate(sp)
    m, ep, T = model_for('g115'), sp['ep'], sp['T']
    G, pi0, q = (c(t) for t in m.simulate_batch(sp['sb'], T, use_means=False, stage=STAGE, row_offset=0))
    Gk, pk, qk = (c(t) for t in m.simulate_batch(sp['starts'], T, use_means=False, stage=STAGE, row_offset=0))
    print(f"{sp['tag']}: G {G.tolist()} oracle {sp['G'].tolist()} clean {Gk.tolist()}; pi0[{ep}] {pi0[ep].argmax(1).tolist()} Qpi[{ep}] {q[ep].tolist()}")
    assert np.isnan(G[ep])
    assert np.array_equal(pi0[ep], sp['pi0'][ep]) and np.array_equal(q[ep], sp['q'][ep])
    keep = [e for e in range(sp['E']) if e != ep]
    assert np.isfinite(Gk).all()
    for a, k in ((G, Gk), (pi0, pk), (q, qk)):
        assert np.array_equal(bits(a[keep]), bits(k[keep]))


# ---- forward, generic geometry (the kernels of generic*.hip) ---------------------------------------------------------------------
@pytest.mark.parametrize('poison', POISONS)
def test_generic_decoder(poison):
    verify(spec_decoder(5, (0, 4), poison, GEO32))


@pytest.mark.parametrize('poison', POISONS)
def test_generic_encoder(poison):
    verify(spec_encoder((15, 15), True, poison, GEO32))


# ---- weights: one NaN element per case, C1 only ------------------------------------------------------------------------------------
# (key, element, network, (dropout tag, features, pass) of the mask the poisoned unit sits behind or None)
WEIGHTS = [('top.qpi_net.0.weight', (3, 0), 'habit', None),
           ('mid.ps_net.0.weight', (5, 0), 'transition', (PX.TAG_MID, 512, PX.PASS_T1)),
           ('down.po_net.0.weight', (7, 0), 'decoder', (PX.TAG_DEC, 256, PX.PASS_D1)),
           ('down.po_net.9.weight', (100, 0), 'decoder', None),            # a pixel-local NaN that the Winograd layers spread
           ('down.qs_net.0.weight', (0, 0, 0, 0), 'encoder', None),
           ('down.qs_net.9.weight', (11, 0), 'encoder', (PX.TAG_ENC, 256, PX.PASS_E1))]
WEIGHT_STAGE = 40


def spec_weight(key, index, net, mask):
    M = 5
    w = NF.poisoned_weights(family('g115'), key, index)
    s, pi, o = states(M), actions(M), frames_for(M)
    dropped = []
    if mask is not None:         # the stage must drop the poisoned unit in some row: there a select-style mask would hide the NaN, a product keeps it
        tag, nf, pas = mask
        dropped = np.flatnonzero(PX.dropout_mask(SEED, tag, M, nf, pas, 0, WEIGHT_STAGE)[:, index[0]] == 0).tolist()
        assert dropped, f'{key}: stage {WEIGHT_STAGE} keeps unit {index[0]} in all {M} rows'
    orc = oracle(weights=w)
    t = torch.from_numpy
    with torch.no_grad():
        out = {'habit': lambda: orc.encode_s(t(s)), 'transition': lambda: orc.transition_with_sample(t(pi), t(s), PX.PASS_T1, 0, WEIGHT_STAGE),
               'decoder': lambda: orc.decoder(t(s), PX.PASS_D1, 0, WEIGHT_STAGE), 'encoder': lambda: orc.encoder_with_sample(t(o), PX.PASS_E1, 0, WEIGHT_STAGE)}[net]()
    eng = {'habit': lambda m: m.model_top.encode_s(s), 'transition': lambda m: m.model_mid.transition_with_sample(pi, s, stage=WEIGHT_STAGE, pass_=PX.PASS_T1),
           'decoder': lambda m: m.model_down.decoder(s, stage=WEIGHT_STAGE, pass_=PX.PASS_D1),
           'encoder': lambda m: m.model_down.encoder_with_sample(o, stage=WEIGHT_STAGE, pass_=PX.PASS_E1)}[net]
    return dict(tag=f'{key}{list(index)} = NaN', M=M, orc=out, dropped=dropped, eng=lambda: eng(engine_with(w)))


def guard_weight(sp):
    o = rows2d(sp['orc'], sp['M'])
    nf = ~np.isfinite(o).all(axis=1)
    assert nf.any(), f"{sp['tag']}: the oracle is finite everywhere"
    assert nf[sp['dropped']].all(), f"{sp['tag']}: the oracle is finite in a row whose mask drops the poisoned unit"
    return o


@pytest.mark.parametrize('key,index,net,mask', WEIGHTS, ids=[w[0] for w in WEIGHTS])
def test_weight(key, index, net, mask):
    sp = spec_weight(key, index, net, mask)
    o = guard_weight(sp)
    c1(sp['tag'], o, rows2d(sp['eng'](), sp['M']))


# ---- gradients: M = 5, one bad input row ------------------------------------------------------------------------------------------
def spec_grad_top(poison):
    M = 5
    s, lp = TR.batch(21, M)
    sb = poisoned(s, (2, 3), poison)
    kl, g = TR.grads(family('g115'), sb, lp)
    run = lambda x: L().grad_top(model_for('g115').model_top, x, lp)          # noqa: E731
    return dict(tag=f'grad_top {poison}', M=M, bad=(2,), orc=[kl], grads=g, run=run, xb=sb, x=s, rows=lambda r: [r[0]], g=lambda r: r[1])


def spec_grad_mid(poison):
    M = 5
    b = TM.batch_mid(22, M)
    s0b = poisoned(b[0], (2, 3), poison)
    F, mean, lv, g = TM.grads(family('g115'), (s0b,) + b[1:], STAGE)
    run = lambda x: L().grad_mid(model_for('g115').model_mid, x, b[2], b[3], b[1], b[4], stage=STAGE)          # noqa: E731
    return dict(tag=f'grad_mid {poison}', M=M, bad=(2,), orc=[F, mean, lv], grads=g, run=run, xb=s0b, x=b[0], rows=lambda r: list(r[:3]), g=lambda r: r[3])


def down_rows(r):
    F, (nl, kls, kln), po1, qs1, qm, qv = r[:6]
    return [F, nl, kls, kln, po1, qs1, qm, qv]


def spec_grad_down(poison):
    M = 5
    o1, pm, pv, om = TDN.inputs(23, M)
    o1 = np.asarray(o1, dtype=np.float32).reshape(M, 1, 64, 64)
    ob = poisoned(o1, (2, 0, 31, 31), poison)
    with np.errstate(all='ignore'):
        r = TDN.run(family('g115'), ob, pm, pv, om, STAGE, gamma=0.5)
    orc = [r[k] for k in ('F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'po1', 'qs1', 'mean', 'logvar')]
    run = lambda x: L().grad_down(model_for('g115').model_down, x, pm, pv, om, stage=STAGE)          # noqa: E731
    return dict(tag=f'grad_down {poison}', M=M, bad=(2,), orc=orc, grads=r['grads'], run=run, xb=ob, x=o1, rows=down_rows, g=lambda r: r[6])


def verify_grad(sp):
    o, nf = guard(sp['tag'], sp['orc'], sp['bad'], sp['M'])
    assert any(np.isnan(np.asarray(g)).any() for g in sp['grads'].values()), f"{sp['tag']}: the restatement has no NaN gradient"
    r = sp['run'](sp['xb'])
    e = rows2d(sp['rows'](r), sp['M'])
    c1(sp['tag'], o, e)
    c2(sp['tag'], nf, e, rows2d(sp['rows'](sp['run'](sp['x'])), sp['M']))
    grads_c1(sp['tag'], sp['grads'], sp['g'](r))


@pytest.mark.parametrize('poison', POISONS)
def test_grad_top(poison):
    verify_grad(spec_grad_top(poison))


@pytest.mark.parametrize('poison', POISONS)
def test_grad_mid(poison):
    verify_grad(spec_grad_mid(poison))


@pytest.mark.parametrize('poison', POISONS)
def test_grad_down(poison):
    verify_grad(spec_grad_down(poison))


# ---- one training step --------------------------------------------------------------------------------------------------------
STEP_ROWS = ('kl_pi', 'omega', 'qs0', 'F_mid', 'ps1_mean', 'ps1_logvar', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive')       # TrainStep's per-row fields
STEP_REF = dict(qs0='s0')                                                                                              # ... under free_energy_ref's names
LR = {'top': 1e-4, 'mid': 1e-4, 'down': 1e-3}


def spec_train_step(poison):
    """the oracle side of one loss.train_step with a bad pixel in o1: the per-row outputs (free_energy_ref, derived omega) and the gradients
    of the three parts at those values (train_ref, train_mid_ref, train_down_ref), all of the weights before the step"""
    M = 5
    b = fe_batch(M)
    bb = (b[0], poisoned(b[1], (2, 0, 31, 31), poison)) + b[2:]
    w = family('g115')
    with torch.no_grad():
        r = {k: v.numpy() for k, v in FR.free_energy(oracle(), *bb, gamma=0.5, stage=STAGE).items()}
    with np.errstate(all='ignore'):
        g_top = TR.grads(w, r['s0'], bb[3])[1]
        g_mid = TM.grads(w, (r['s0'], bb[2], r['qs1_mean'], r['qs1_logvar'], r['omega']), STAGE)[3]
        g_down = TDN.run(w, bb[1], r['ps1_mean'], r['ps1_logvar'], r['omega'], STAGE, gamma=0.5)['grads']
    return dict(tag=f'train_step {poison}', M=M, bad=(2,), b=b, bb=bb, ref=r, orc=[r[STEP_REF.get(f, f)] for f in STEP_ROWS],
                grads={'top': g_top, 'mid': g_mid, 'down': g_down})


def guard_train_step(sp):
    o, nf = guard(sp['tag'], sp['orc'], sp['bad'], sp['M'])
    assert np.isfinite(sp['ref']['kl_pi']).all() and np.isfinite(sp['ref']['omega']).all()        # o0 is clean: the habit net's step is healthy
    assert all(np.isfinite(g).all() for g in sp['grads']['top'].values())
    for part in ('mid', 'down'):
        assert any(np.isnan(g).any() for g in sp['grads'][part].values()), part
    return o, nf


_CLEAN_STEP = {}


def run_step(b):
    import daimc_amd
    m = model_for('g115', fresh=True)
    opts = {k: daimc_amd.Adam(getattr(m, 'model_' + k), lr=LR[k]) for k in LR}
    return m, opts, L().train_step(m, *b, opts, stage=STAGE)


@pytest.mark.parametrize('poison', POISONS)
def test_train_step(poison):
    sp = spec_train_step(poison)
    o, nf = guard_train_step(sp)
    m, opts, A = run_step(sp['bb'])
    if 'rows' not in _CLEAN_STEP:
        _CLEAN_STEP['rows'] = rows2d([getattr(run_step(sp['b'])[2], f) for f in STEP_ROWS], sp['M'])
    e = rows2d([getattr(A, f) for f in STEP_ROWS], sp['M'])
    c1(sp['tag'], o, e)
    c2(sp['tag'], nf, e, _CLEAN_STEP['rows'])
    means = c(A.means)
    print(f"{sp['tag']}: means {dict(zip(L().STEP_MEANS_FIELDS, means.tolist()))}")
    for i, f in enumerate(L().STEP_MEANS_FIELDS):
        rows = sp['ref']['omega' if f == 'omega_std' else f]
        if np.isnan(rows).any():
            assert np.isnan(means[i]), f'means[{f}] = {means[i]} with a NaN row'
    for part in ('top', 'mid', 'down'):
        sd = getattr(m, 'model_' + part).state_dict()
        for k, g in sp['grads'][part].items():
            nan = np.isnan(np.asarray(g))
            got = np.isnan(c(sd[k]))
            print(f"{sp['tag']}: {part}.{k}: NaN gradient elements {int(nan.sum())}, NaN parameter elements after the step {int(got.sum())}")
            assert got[nan].all(), f'{part}.{k}: {int((nan & ~got).sum())} elements with a NaN gradient are not NaN after the step'
    assert [opts[k]._step for k in ('top', 'mid', 'down')] == [1, 1, 1]
