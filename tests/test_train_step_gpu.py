"""GPU tests (-m gpu) of the whole training step (efe_train_step; csrc/loss.hip k_step_omega + k_step_means; loss.train_step).

Engine seed 7, weights 'g115' (and 'sat_top', whose kl_pi is large, for the omega expression), gamma 0.5 so that both KL branches enter,
the reference learning rates 1e-4 / 1e-4 / 1e-3.  Inputs: synthetic frames (oracle/synth.py), one-hot actions and a log-softmax prior.
The batch sizes are those at which the step's own code can go wrong: M = 1 (one padded tile; the standard deviation's NaN branch), 50 (the
reference batch), 65 (crosses a 64-row group and a 16-row tile) and 257 (the second trip of the 256-stride loops).

The contract under test is equality of bits with the public calls issued one after another (encoder_with_sample under PASS_FE_Q0,
train_model_top, encoder under PASS_FE_Q1, train_model_mid, train_model_down) at the same stage with the step's per-row omega."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import synth
from train_common import SEED, c, model_for

pytestmark = pytest.mark.gpu

LR = {'top': 1e-4, 'mid': 1e-4, 'down': 1e-3}
MS = [1, 50, 65, 257]
U = 2.0 ** -24
OUT = ('kl_pi', 'qs0', 'ps1_mean', 'ps1_logvar', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive')


def L():
    import daimc_amd
    return daimc_amd.loss


_BATCH = {}


def batch(M, seed=0):
    """(o0, o1 [M,1,64,64], pi0 one-hot [M,4], log_Ppi [M,4]) as numpy; computed once per size and left unchanged"""
    if (M, seed) not in _BATCH:
        r = np.random.RandomState(4000 + 10 * M + seed)
        pi0 = np.eye(4, dtype=np.float32)[r.randint(0, 4, M)]
        lp = torch.log_softmax(torch.from_numpy(r.randn(M, 4).astype(np.float32)), 1).numpy()
        _BATCH[(M, seed)] = (synth.make_frames(300 + M + seed, M), synth.make_frames(700 + M + seed, M), pi0, lp)
    return _BATCH[(M, seed)]


def twin(name='g115'):
    import daimc_amd
    m = model_for(name, fresh=True)
    return m, {k: daimc_amd.Adam(getattr(m, 'model_' + k), lr=LR[k]) for k in LR}


def sequence(m, opts, b, t, omega, eps=None):
    """the public calls one after another, all at stage t (t None: ONE stage of the model's counter)"""
    from daimc_amd.model import PASS_FE_Q0, PASS_FE_Q1
    o0, o1, pi0, lp = b
    t = m._take_stage(t)
    qs0, _, _ = m.model_down.encoder_with_sample(o0, stage=t, pass_=PASS_FE_Q0, eps=None if eps is None else eps[0])
    kl = L().train_model_top(m.model_top, qs0, lp, opts['top'])
    qm, qv = m.model_down.encoder(o1, stage=t, pass_=PASS_FE_Q1)
    pm, pv = L().train_model_mid(m.model_mid, qs0, qm, qv, pi0, omega, opts['mid'], stage=t)
    F, (nl, kls, kln) = L().train_model_down(m.model_down, o1, pm, pv, omega, opts['down'], stage=t, eps=None if eps is None else eps[2])
    return dict(kl_pi=kl, qs0=qs0, ps1_mean=pm, ps1_logvar=pv, F_down=F, nlogpo1=nl, kl_s=kls, kl_naive=kln)


def snapshot(m, opts):
    """every weight, every optimiser vector and the three step counts, as numpy"""
    s = {}
    for part in ('top', 'mid', 'down'):
        for k, v in getattr(m, 'model_' + part).state_dict().items():
            s[f'{part}.{k}'] = c(v)
        o = opts[part]
        ea, es = o._buffers()
        s[f'{part}.exp_avg'], s[f'{part}.exp_avg_sq'], s[f'{part}.step'] = c(ea), c(es), np.array(o._step)
    return s


def assert_same(tag, a, b):
    assert a.keys() == b.keys(), tag
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f'{tag}: {k}')


def outputs(r, fields=OUT):
    d = r._asdict() if hasattr(r, '_asdict') else r
    return {k: c(d[k]) for k in fields}


# ---- 1. equals the sequence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', MS)
def test_step_equals_the_sequence(M):
    b, t = batch(M), 5
    (ma, oa), (mb, ob), (mc, _) = twin(), twin(), twin()
    A = L().train_step(ma, *b, oa, stage=t)
    B = sequence(mb, ob, b, t, A.omega)
    assert_same(f'outputs M={M}', outputs(A), outputs(B))
    assert_same(f'state M={M}', snapshot(ma, oa), snapshot(mb, ob))
    assert all(o._step == 1 for o in oa.values())
    from daimc_amd.model import PASS_FE_Q1
    qm, qv = mc.model_down.encoder(b[1], stage=t, pass_=PASS_FE_Q1)
    F_mid = L().grad_mid(mc.model_mid, A.qs0, qm, qv, b[2], A.omega, stage=t)[0]
    np.testing.assert_array_equal(c(A.F_mid), c(F_mid))
    assert not np.array_equal(snapshot(ma, oa)['down.qs_net.0.weight'], snapshot(mc, _)['down.qs_net.0.weight'])     # it did train


# ---- 2. derived omega ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,params', [('g115', None), ('g115', (2.0, 0.5, 0.25, 0.75)), ('sat_top', None)])
def test_derived_omega(name, params):
    M, t = 50, 9
    b = batch(M)
    if name == 'sat_top':       # a sharp prior against the family's saturated habit posterior: kl_pi reaches past the sigmoid's midpoint b = 25
        b = b[:3] + (torch.log_softmax(16.0 * torch.from_numpy(b[3]), 1).numpy(),)
    kw = {} if params is None else {'omega_params': params}
    (ma, oa), (mc, oc) = twin(name), twin(name)
    A = L().train_step(ma, *b, oa, stage=t, **kw)
    Cc = L().train_step(mc, *b, oc, stage=t, omega=A.omega)
    assert_same('given its own omega', outputs(A, OUT + ('omega', 'F_mid', 'means')), outputs(Cc, OUT + ('omega', 'F_mid', 'means')))
    assert_same('state', snapshot(ma, oa), snapshot(mc, oc))
    want = c(L().compute_omega(A.kl_pi, *(params or L().OMEGA_PARAMS)))
    print(f'{name} {params}: kl_pi in [{c(A.kl_pi).min():.3g}, {c(A.kl_pi).max():.3g}], omega in [{c(A.omega).min():.6g}, {c(A.omega).max():.6g}], '
          f'max rel err {np.abs(c(A.omega) / want - 1).max():.3e}')
    np.testing.assert_allclose(c(A.omega), want, rtol=2e-6, atol=0)
    if name == 'sat_top':
        assert c(A.kl_pi).max() > 25.0 and c(A.omega).min() < 2.0


def test_scalar_omega():
    M, t = 50, 9
    b = batch(M)
    (ma, oa), (mb, ob) = twin(), twin()
    A = L().train_step(ma, *b, oa, stage=t, omega=2.0)
    B = sequence(mb, ob, b, t, 2.0)
    np.testing.assert_array_equal(c(A.omega), np.full(M, 2.0, np.float32))
    assert_same('outputs', outputs(A), outputs(B))
    assert_same('state', snapshot(ma, oa), snapshot(mb, ob))


# ---- 3. state carries over ---------------------------------------------------------------------------------------------
def test_five_steps_carry_state():
    M = 50
    (ma, oa), (mb, ob) = twin(), twin()
    for i in range(5):
        b = batch(M, seed=i)
        A = L().train_step(ma, *b, oa)
        B = sequence(mb, ob, b, None, A.omega)
        assert_same(f'outputs of step {i}', outputs(A), outputs(B))
        assert_same(f'state after step {i}', snapshot(ma, oa), snapshot(mb, ob))
    assert ma._stage == mb._stage == 5
    assert [o._step for o in oa.values()] == [5, 5, 5]


# ---- 4. forward paths see the step -----------------------------------------------------------------------------------
def test_forward_paths_see_the_step():
    import daimc_amd
    M = 50
    ma, oa = twin()
    for i in range(2):
        L().train_step(ma, *batch(M, seed=i), oa)
    w = {f'{part}.{k}': c(v) for part in ('top', 'mid', 'down') for k, v in getattr(ma, 'model_' + part).state_dict().items()}
    fresh = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=SEED, init_weights=False)
    fresh.load_flat_weights(w)
    o0, o1, pi0, lp = batch(M, seed=7)
    s0 = np.random.RandomState(3).randn(M, 10).astype(np.float32)

    def calls(m):
        fe = daimc_amd.free_energy(m, o0, o1, pi0, lp, stage=11)
        G, terms, ps1, ps1_mean, po1 = m.calculate_G(s0, pi0, samples=2, stage=12)
        return [c(x) for x in fe] + [c(G), c(ps1), c(ps1_mean), c(po1)] + [c(x) for x in terms] + [c(x) for x in m.model_top.encode_s(s0)]

    for i, (p, q) in enumerate(zip(calls(ma), calls(fresh))):
        np.testing.assert_array_equal(p, q, err_msg=f'forward output {i}')


# ---- 5. means ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', MS)
def test_means(M):
    """Each mean against the float64 mean of the returned rows within (ceil(M / 256) + 12) u mean|x|, u = 2^-24: a term passes through at
    most ceil(M / 256) strided adds, 6 butterfly steps and 3 wave adds (the forward bound (ceil(M / 256) + 10) u sum|x| of that
    summation, second-order terms dropped), and the slack of 2 u covers the division.  The standard deviation: the same bound on the sum
    of the squared deviations d_r (all positive: a relative bound k u on the variance), carried through the square root, whose derivative
    halves a relative error: |std - numpy's| <= (k u / 2 + u) std, the last u for the square root's own rounding."""
    b = batch(M)
    (ma, oa), (mb, ob) = twin(), twin()
    mine = torch.full((8,), 7.0, device='cuda:0')
    A = L().train_step(ma, *b, oa, stage=5, means=mine)
    B = L().train_step(mb, *b, ob, stage=5)
    assert A.means is mine and c(mine).tobytes() == c(B.means).tobytes()            # written in place; twice the same bits
    k = math.ceil(M / 256) + 12
    got = c(A.means).astype(np.float64)
    bad = []
    for i, name in enumerate(L().STEP_MEANS_FIELDS[:7]):
        x = c(getattr(A, name)).astype(np.float64)
        err, bound = abs(got[i] - x.mean()), k * U * np.abs(x).mean()
        print(f'M={M} mean {name}: engine {got[i]:.9g} fp64 {x.mean():.9g} err {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append((name, err, bound))
    om = c(A.omega).astype(np.float64)
    if M == 1:
        assert np.isnan(got[7])
    else:
        std = om.std(ddof=1)
        err, bound = abs(got[7] - std), (k * U / 2 + U) * std
        print(f'M={M} omega_std: engine {got[7]:.9g} numpy {std:.9g} err {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append(('omega_std', err, bound))
    assert not bad, bad


# ---- 6. injected normals -----------------------------------------------------------------------------------------------
def test_injected_normals():
    M, t = 50, 4
    b = batch(M)
    eps = np.random.RandomState(8).randn(3, M, 10).astype(np.float32)
    (ma, oa), (mb, ob), (mc, oc) = twin(), twin(), twin()
    A = L().train_step(ma, *b, oa, stage=t, eps=eps)
    B = sequence(mb, ob, b, t, A.omega, eps=eps)
    assert_same('outputs', outputs(A), outputs(B))
    assert_same('state', snapshot(ma, oa), snapshot(mb, ob))
    eps2 = eps.copy()
    eps2[1] = 100.0
    Cc = L().train_step(mc, *b, oc, stage=t, eps=eps2)
    assert_same('plane 1 is not read', outputs(A, OUT + ('omega', 'F_mid', 'means')), outputs(Cc, OUT + ('omega', 'F_mid', 'means')))
    assert_same('state', snapshot(ma, oa), snapshot(mc, oc))


# ---- 7. refusals change nothing ------------------------------------------------------------------------------------------
def raw_step(m, opts, b, M, *, o1=True, kl=True, mode=2, omega=None):
    """efe_train_step through ctypes -> (return code, message)"""
    from daimc_amd import _lib as LB
    e = m._ready()
    t = [e.tensor(x) for x in b]
    outs = {f: e.empty(max(M, 1) * (10 if f in ('qs0', 'ps1_mean', 'ps1_logvar') else 1)) for f in LB.STEP_OUT_FIELDS[:-1]}
    p = lambda x: C.c_void_p(x.data_ptr())
    si = LB.EfeStepIn(p(t[0]), p(t[1]) if o1 else None, p(t[2]), p(t[3]), None)
    so = LB.EfeStepOut(*[p(outs[f]) if (f != 'kl_pi' or kl) else None for f in LB.STEP_OUT_FIELDS[:-1]], None)
    fp = LB.EfeFeParams(0.5, 1.0, 1.0, mode, omega, 1.0, 1.0, 25.0, 5.0, 1.5)
    ad = []
    for k in ('top', 'mid', 'down'):
        ea, es = opts[k]._buffers()
        ad.append(LB.EfeStepAdam(p(ea), p(es), LB.EfeAdamParams(*opts[k]._hyper(), opts[k]._step + 1)))
    nz = LB.EfeNoise(SEED, 5, 0, 0, 0)
    rc = e.lib.efe_train_step(e.ctx, C.byref(si), M, C.byref(fp), C.byref(nz), C.byref(ad[0]), C.byref(ad[1]), C.byref(ad[2]), C.byref(so), e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


def test_refusals_change_nothing():
    import daimc_amd
    M = 3
    b = batch(M)
    m, opts = twin()
    L().train_step(m, *b, opts, stage=1)              # state exists: a refused step must not touch it
    before = snapshot(m, opts)
    other, other_opts = twin()
    with pytest.raises(ValueError, match="optimizers\\['down'\\]"):
        L().train_step(m, *b, dict(opts, down=other_opts['down']), stage=2)
    with pytest.raises(ValueError, match="no entry 'mid'"):
        L().train_step(m, *b, {k: v for k, v in opts.items() if k != 'mid'}, stage=2)
    for rc, msg in (raw_step(m, opts, b, 0), raw_step(m, opts, b, M, o1=False), raw_step(m, opts, b, M, kl=False), raw_step(m, opts, b, M, mode=0),
                    raw_step(m, opts, b, M, mode=5)):
        print(rc, msg)
        assert rc == 1 and 'efe_train_step' in msg
    for opt_name in ('mfma_bf16x3', 'mfma_f16x2'):
        m.set_option(opt_name, 1)
        with pytest.raises(RuntimeError, match='efe_train_step.*split-operand'):
            L().train_step(m, *b, opts, stage=2)
        m.set_option(opt_name, 0)
    assert_same('after the refusals', before, snapshot(m, opts))
    L().train_step(m, *b, opts, stage=2)              # and the model still trains
    assert opts['top']._step == opts['mid']._step == opts['down']._step == 2


@pytest.mark.parametrize('geo', [(4, 3, 64), (4, 1, 32)])
def test_other_geometries_are_refused(geo):
    import daimc_amd
    m = model_for('g115', geo=geo, fresh=True)
    top, mid = daimc_amd.Adam(m.model_top), daimc_amd.Adam(m.model_mid)
    w0 = {k: c(v) for k, v in m.model_top.state_dict().items()}
    o = np.zeros((2, geo[1], geo[2], geo[2]), np.float32)
    pi0 = np.eye(4, dtype=np.float32)[:2]
    with pytest.raises(ValueError, match='Adam: ModelDown is trainable on the engine at 1 x 64 x 64 only'):
        daimc_amd.Adam(m.model_down)
    with pytest.raises(ValueError, match='train_step: built for 1 x 64 x 64 models'):
        L().train_step(m, o, o, pi0, np.log(np.full((2, 4), 0.25, np.float32)), {'top': top, 'mid': mid, 'down': None})
    assert top._step == mid._step == 0 and top.exp_avg is None
    assert_same('weights', w0, {k: c(v) for k, v in m.model_top.state_dict().items()})


# ---- 8. allocates once -------------------------------------------------------------------------------------------------
def test_second_call_allocates_nothing():
    M = 65
    b = batch(M)
    m, opts = twin()
    L().train_step(m, *b, opts)
    grown = m.arena_stats()['grow_count']
    L().train_step(m, *b, opts)
    torch.cuda.synchronize()
    assert m.arena_stats()['grow_count'] == grown
