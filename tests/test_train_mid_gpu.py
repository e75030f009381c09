"""GPU tests (-m gpu) of the transition network's training step on the engine (csrc/train.hip: k_mid_grad, k_slab_sum, k_adam;
loss.train_model_mid, loss.grad_mid, daimc_amd.Adam over model_mid) against tests/train_mid_ref.py -- autograd and torch.optim.Adam over
the CPU oracle's transition with the Philox dropout masks, in fp32 and fp64, itself pinned bit for bit to the reference's train_model_mid
by tests/test_train_mid_cpu.py.

Gradients and optimiser results are held to the project's fp64 rule (tests/test_fp64_parity.py fp64_rule):
    max|x_engine - x_64| <= 4 max|x_32 - x_64| + 8 ulp32(max|x_64|)   per parameter tensor,
F_mid to the KL tolerance of tests/test_free_energy_gpu.py (rtol 1e-5 / atol 1e-4), ps1_mean / ps1_logvar and the network outputs after
training to its network tolerance (rtol 1e-5 / atol 2e-6).

Inputs: train_mid_ref.batch_mid(seed, M).  Engine seed 7, pass PASS_FE_T, sample 0, an explicit stage (3 unless stated).  Every gradient
case first asserts that no hidden pre-activation of the fp64 oracle lies within 1e-5 of zero (an fp32 ReLU decision that differs from
fp64's is not a kernel error); the seeds below were chosen so that this holds.  M = 129 = 16 * 8 + 1: k_mid_grad runs at most 8 workgroups
(csrc/kernels.h TRAIN_MID_SLABS), so workgroup 0 walks a second tile."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_mid_ref as TM
import train_ref as TR
from conftest import load_golden
from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise
from train_common import apply_rule, c, family, model_for, synth_grads, torch_adam_run

pytestmark = pytest.mark.gpu

SEED = TM.SEED
STAGE = 3
WALK_M = 16 * 8 + 1
KL = dict(rtol=1e-5, atol=1e-4)
NET = dict(rtol=1e-5, atol=2e-6)
P4, P3 = 543252, 542740         # parameters of ps_net at pi_dim 4 / 3


def engine_grads(m, b, stage=STAGE, **key):
    """loss.grad_mid with train_mid_ref's argument order (batch_mid: s0, pi, qs1_mean, qs1_logvar, omega)"""
    import daimc_amd
    s0, pi, qm, qv, om = b
    return daimc_amd.loss.grad_mid(m.model_mid, s0, qm, qv, pi, om, stage=stage, **key)


def engine_train(m, b, opt, stage=STAGE):
    import daimc_amd
    s0, pi, qm, qv, om = b
    return daimc_amd.loss.train_model_mid(m.model_mid, s0, qm, qv, pi, om, opt, stage=stage)


_ORACLE = {}


def oracle_grads(fam, geo, b_key, b, stage, key):
    """the fp32 and fp64 oracle of one case, computed once and shared"""
    k = (fam, geo, b_key, stage, tuple(sorted(key.items())))
    if k not in _ORACLE:
        w = family(fam, geo)
        _ORACLE[k] = (TM.grads(w, b, stage, torch.float32, geo[0], **key), TM.grads(w, b, stage, torch.float64, geo[0], **key))
    return _ORACLE[k]


def check_grads(tag, fam, M, seed, geo=(4, 1, 64), stage=STAGE, omega=None, **key):
    b = TM.batch_mid(seed, M, geo[0])
    if omega is not None:
        b = b[:4] + (omega,)
    w = family(fam, geo)
    assert TM.preact_margin(w, b, stage, geo[0], **key) >= 1e-5, 'precondition: a hidden pre-activation within 1e-5 of zero (pick another seed)'
    F, mean, lv, g = engine_grads(model_for(fam, geo), b, stage, **key)
    (F32, m32, l32, g32), (_, _, _, g64) = oracle_grads(fam, geo, (seed, M, omega), b, stage, key)
    assert list(g) == list(TM.KEYS)
    np.testing.assert_allclose(c(F), F32, err_msg=tag + ' F_mid', **KL)
    np.testing.assert_allclose(c(mean), m32, err_msg=tag + ' ps1_mean', **NET)
    np.testing.assert_allclose(c(lv), l32, err_msg=tag + ' ps1_logvar', **NET)
    apply_rule(tag, [(k, c(g[k]), g32[k], g64[k]) for k in TM.KEYS])
    g = {k: c(v) for k, v in g.items()}
    assert all(np.isfinite(v).all() for v in g.values())
    return g


# ---- 1. gradients vs fp64 --------------------------------------------------------------------------------------------
GRAD_CASES = [('g115', M, s) for M, s in ((1, 101), (3, 103), (16, 116), (17, 117), (50, 150), (WALK_M, 229))] + \
             [('g100', 17, 117), ('g100', 50, 151), ('sparse', 17, 117), ('sparse', 50, 150)]


@pytest.mark.parametrize('fam,M,seed', GRAD_CASES)
def test_gradients_vs_fp64(fam, M, seed):
    check_grads(f'{fam} M={M}', fam, M, seed)


def test_gradients_with_other_noise_keys():
    """row_offset 5, stage 9, sample 2 against the oracle keyed the same way: a backward gate keyed differently from the forward mask
    would show here"""
    check_grads('keyed M=17', 'g115', 17, 118, stage=9, sample=2, row_offset=5)


def test_gradients_generic_geometry():
    """pi_dim 3 on a 3 x 32 x 32 context: the first layer contracts K = 13 inputs"""
    geo = (3, 3, 32)
    g = check_grads('generic M=17', 'g115', 17, 117, geo=geo)
    assert g['ps_net.0.weight'].shape == (512, 13)


def test_gradients_scalar_omega():
    check_grads('scalar omega M=17', 'g115', 17, 117, omega=2.0)


# ---- 2. reference fixture --------------------------------------------------------------------------------------------
def test_gradients_of_reference_fixture():
    fx = load_golden('train_mid_g115')
    import json
    meta = json.loads(str(fx['meta']))
    b = tuple(fx[k] for k in ('s0', 'pi', 'qs1_mean', 'qs1_logvar', 'omega'))
    _, mean, lv, g = engine_grads(model_for('g115'), b, meta['stage'])
    np.testing.assert_allclose(c(mean), fx['ps1_mean_1'], **NET)
    np.testing.assert_allclose(c(lv), fx['ps1_logvar_1'], **NET)
    g64 = TM.grads(family('g115'), b, meta['stage'], torch.float64)[3]
    trip = []
    for k in TM.KEYS:
        if k in meta['big']:
            for part, ix in (('rows', np.ix_(meta['slice'], meta['idx'])), ('cols', np.ix_(meta['idx'], meta['slice']))):
                trip.append((f'{k}.{part}', c(g[k])[ix], fx[f'grad1.{k}.{part}'], g64[k][ix]))
        else:
            trip.append((k, c(g[k]), fx['grad1.' + k], g64[k]))
    apply_rule('fixture', trip)


# ---- 3. dead and dropped units ---------------------------------------------------------------------------------------
def test_dead_and_dropped_units_have_exactly_zero_gradient():
    """a hidden unit that is inactive or dropped for every row of the batch: its weight row, bias and outgoing column get exactly 0;
    every other unit's do not"""
    w = family('g115')
    b = TM.batch_mid(117, 17)
    assert TM.preact_margin(w, b, STAGE) >= 1e-5
    hid = TM.hidden(w, b, STAGE)
    _, _, _, g = engine_grads(model_for('g115'), b)
    g = {k: c(v) for k, v in g.items()}
    idx = (0, 3, 6, 9)
    for li, (a, mask) in enumerate(hid):
        dead = ((a <= 0) | (mask == 0)).all(0)
        assert dead.sum() > 0, f'precondition: the batch leaves units of hidden layer {li} inactive or dropped for every row'
        gw, gb, gn = g[f'ps_net.{idx[li]}.weight'], g[f'ps_net.{idx[li]}.bias'], g[f'ps_net.{idx[li + 1]}.weight']
        assert not gw[dead].any() and not gb[dead].any() and not gn[:, dead].any(), li
        live = ~dead
        assert (np.abs(gw[live]).max(1) > 0).all() and (gb[live] != 0).all() and (np.abs(gn[:, live]).max(0) > 0).all(), li


# ---- 4. reproducible -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,seed', [(3, 103), (50, 150), (WALK_M, 229)])
def test_reproducible(M, seed):
    b = TM.batch_mid(seed, M)
    m = model_for('g115')
    F1, m1, l1, g1 = engine_grads(m, b)
    F2, m2, l2, g2 = engine_grads(m, b)
    assert np.array_equal(c(F1), c(F2)) and np.array_equal(c(m1), c(m2)) and np.array_equal(c(l1), c(l2))
    for k in TM.KEYS:
        assert np.array_equal(c(g1[k]), c(g2[k])), k


# ---- 5. composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,seed', [(3, 103), (50, 150)])
def test_train_model_mid_is_grad_then_adam(M, seed):
    import daimc_amd
    b = TM.batch_mid(seed, M)
    ma, mb = model_for('g115', fresh=True), model_for('g115', fresh=True)
    oa, ob = daimc_amd.Adam(ma.model_mid, lr=1e-3), daimc_amd.Adam(mb.model_mid.parameters(), lr=1e-3)
    for _ in range(2):
        mean_a, lv_a = engine_train(ma, b, oa)
        _, mean_b, lv_b, g = engine_grads(mb, b)
        ob.step(g)
        assert np.array_equal(c(mean_a), c(mean_b)) and np.array_equal(c(lv_a), c(lv_b))
    sa, sb = ma.model_mid.state_dict(), mb.model_mid.state_dict()
    for k in TM.KEYS:
        assert np.array_equal(c(sa[k]), c(sb[k])), k
        assert not np.array_equal(c(sa[k]), family('g115')['mid.' + k]), k
    osa, osb = oa.state_dict()['state'], ob.state_dict()['state']
    for i in range(8):
        for f in ('exp_avg', 'exp_avg_sq', 'step'):
            assert np.array_equal(c(osa[i][f]), c(osb[i][f])), (i, f)


# ---- 6. Adam on the big part -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['fresh', 'loaded_step_1000'])
def test_adam_three_steps_vs_fp64(case):
    import daimc_amd
    m = model_for('g115', fresh=True)
    w0 = {k: np.array(family('g115')['mid.' + k], dtype=np.float32) for k in TM.KEYS}
    shapes = [w0[k].shape for k in TM.KEYS]
    steps = [synth_grads(900 + i, shapes) for i in range(3)]
    lr = 1e-3
    opt = daimc_amd.Adam(m.model_mid, lr=lr)
    state = None
    if case == 'loaded_step_1000':
        r = np.random.RandomState(5)
        state = {'step': 1000, 'm': [(r.randn(*s) * 1e-2).astype(np.float32) for s in shapes],
                 'v': [(r.uniform(0, 1e-3, s)).astype(np.float32) for s in shapes]}
        sd = opt.state_dict()
        sd['state'] = {i: {'step': torch.tensor(1000.0), 'exp_avg': torch.from_numpy(state['m'][i].copy()), 'exp_avg_sq': torch.from_numpy(state['v'][i].copy())}
                       for i in range(8)}
        opt.load_state_dict(sd)
    for gs in steps:
        opt.step(torch.from_numpy(np.concatenate([g.reshape(-1) for g in gs])))
    sd, osd = m.model_mid.state_dict(), opt.state_dict()
    assert int(osd['state'][0]['step']) == (1003 if state else 3)
    w32, m32, v32 = torch_adam_run(TM.KEYS, w0, steps, torch.float32, lr, state)
    w64, m64, v64 = torch_adam_run(TM.KEYS, w0, steps, torch.float64, lr, state)
    trip = []
    for i, k in enumerate(TM.KEYS):
        trip += [('exp_avg.' + k, c(osd['state'][i]['exp_avg']), m32[i], m64[i]), ('exp_avg_sq.' + k, c(osd['state'][i]['exp_avg_sq']), v32[i], v64[i]),
                 ('w.' + k, c(sd[k]), w32[i], w64[i])]
        assert not np.array_equal(c(sd[k]), w0[k]), k
    apply_rule('adam ' + case, trip)


# ---- 7. every forward path sees the step -----------------------------------------------------------------------------
def test_forward_paths_see_the_step():
    import daimc_amd
    w = family('g115')
    m = model_for('g115', fresh=True)
    m.eps_source, m.u_source = PX.normals, PX.uniforms
    b = TM.batch_mid(117, 17)
    s0, pi, qm, qv, om = b
    starts = s0[:2]
    before = c(m.model_mid.transition_with_sample(pi, s0, stage=5, pass_=TM.PASS_FE_T)[1])
    replica_before = m.cached_replica()
    top0 = {k: c(v) for k, v in m.model_top.state_dict().items()}
    opt = daimc_amd.Adam(m.model_mid, lr=1e-3)
    for _ in range(2):
        engine_train(m, b, opt)
    sd = m.model_mid.state_dict()
    w2 = dict(w)
    for k in TM.KEYS:
        w2['mid.' + k] = c(sd[k])
        assert not np.array_equal(w2['mid.' + k], w['mid.' + k]), k
    orc = OracleModel(w2, PhiloxNoise(SEED))
    with torch.no_grad():
        ops1, omean, olv = (t.numpy() for t in orc.transition_with_sample(torch.from_numpy(pi), torch.from_numpy(s0), TM.PASS_FE_T, 0, 5))
        oF = TM.f_mid(orc, b, 6)[0].numpy()
        osim = [orc.mcts_step_simulate(torch.from_numpy(starts[e]), 2, False, 11, episode=e) for e in range(len(starts))]
    assert np.abs(omean - before).max() > 1e-2, 'the two steps must move the transition visibly'

    def check_transition(mod, tag):
        ps1, mean, lv = (c(t) for t in mod.model_mid.transition_with_sample(pi, s0, stage=5, pass_=TM.PASS_FE_T))
        np.testing.assert_allclose(mean, omean, err_msg=tag + ' ps1_mean', **NET)
        np.testing.assert_allclose(lv, olv, err_msg=tag + ' ps1_logvar', **NET)
        np.testing.assert_allclose(ps1, ops1, err_msg=tag + ' ps1', **NET)

    def check_paths(mod, tag):
        check_transition(mod, tag)                                                                 # k_trans_fused, the 16x16x4 packing
        F = c(daimc_amd.loss.compute_loss_mid(mod.model_mid, s0, pi, qm, qv, om, stage=6)[0])
        np.testing.assert_allclose(F, oF, err_msg=tag + ' F_mid', **KL)
        G, pi0, _ = mod.simulate_batch(starts, 2, use_means=False, stage=11)                       # k_sim_chain, the same packing
        for e, (oG, opi0, _) in enumerate(osim):
            assert np.array_equal(c(pi0[e]), opi0.numpy()), tag
            assert abs(float(G[e]) - oG) < 1e-6 * 2800.0 + 5e-4, (tag, e, float(G[e]), oG)          # test_gpu_parity's gtol for a simulation's G
        mod.set_option('mid_unfused', 1)                                                           # k_dense, the 32x32x2 packing
        try:
            check_transition(mod, tag + ' mid_unfused')
        finally:
            mod.set_option('mid_unfused', 0)

    check_paths(m, 'model')
    r = m.cached_replica()
    assert r is not replica_before, 'a step bumps the weight version: the cached replica is rebuilt'
    check_paths(r, 'replica')
    m.model_top.load_state_dict(m.model_top.state_dict())           # a re-commit must not revert the transition net
    check_paths(m, 're-commit')
    for k in TM.KEYS:
        assert np.array_equal(c(m.model_mid.state_dict()[k]), w2['mid.' + k]), k
    # training the habit net afterwards leaves the transition net's bits alone, and the other way round
    s, log_Ppi = TR.batch(117, 17)
    otop = daimc_amd.Adam(m.model_top, lr=1e-3)
    daimc_amd.loss.train_model_top(m.model_top, s, log_Ppi, otop)
    top1 = {k: c(v) for k, v in m.model_top.state_dict().items()}
    assert all(not np.array_equal(top1[k], top0[k]) for k in TR.KEYS)
    for k in TM.KEYS:
        assert np.array_equal(c(m.model_mid.state_dict()[k]), w2['mid.' + k]), k
    check_transition(m, 'after a habit step')
    engine_train(m, b, opt)
    for k in TR.KEYS:
        assert np.array_equal(c(m.model_top.state_dict()[k]), top1[k]), k
    assert all(not np.array_equal(c(m.model_mid.state_dict()[k]), w2['mid.' + k]) for k in TM.KEYS)
    # loading the transition net must not revert the trained habit net
    m.model_mid.load_state_dict(m.model_mid.state_dict())
    m._ready()
    for k in TR.KEYS:
        assert np.array_equal(c(m.model_top.state_dict()[k]), top1[k]), k


# ---- 8. descent ------------------------------------------------------------------------------------------------------
def test_descent():
    """20 steps at lr 1e-4 on batch_mid(117, 17) at one fixed stage: mean F_mid falls strictly every step and ends at <= 0.5 of its start
    (the fp32 CPU oracle goes 98.67 -> 20.27, ratio 0.21, monotone)"""
    import daimc_amd
    b = TM.batch_mid(117, 17)
    s0, pi, qm, qv, om = b
    m = model_for('g115', fresh=True)
    opt = daimc_amd.Adam(m.model_mid, lr=1e-4)
    Fs = []
    for _ in range(20):
        Fs.append(float(c(daimc_amd.loss.compute_loss_mid(m.model_mid, s0, pi, qm, qv, om, stage=STAGE)[0]).mean()))
        engine_train(m, b, opt)
    Fs.append(float(c(daimc_amd.loss.compute_loss_mid(m.model_mid, s0, pi, qm, qv, om, stage=STAGE)[0]).mean()))
    print('mean F_mid per step:', ' '.join(f'{v:.4f}' for v in Fs))
    assert all(y < x for x, y in zip(Fs, Fs[1:])), Fs
    assert Fs[-1] <= 0.5 * Fs[0], (Fs[0], Fs[-1])


# ---- 9. optimiser state interchange and checkpoints ------------------------------------------------------------------
def test_state_dict_moves_to_torch_and_back():
    import daimc_amd
    b = TM.batch_mid(117, 17)
    m = model_for('g115', fresh=True)
    opt = daimc_amd.Adam(m.model_mid, lr=2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert opt.param_groups[0]['lr'] == 2e-4 and opt.param_groups[0]['params'] == list(range(8))
    assert opt.state_dict()['state'] == {}
    for _ in range(2):
        engine_train(m, b, opt)
    sd = opt.state_dict()
    params = [torch.nn.Parameter(t.clone()) for t in m.model_mid.parameters()]
    assert [tuple(p.shape) for p in params] == [tuple(family('g115')['mid.' + k].shape) for k in TM.KEYS]
    topt = torch.optim.Adam(params, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['lr'] == 2e-4 and tuple(topt.param_groups[0]['betas']) == (0.8, 0.99) and topt.param_groups[0]['eps'] == 1e-7
    for i, p in enumerate(params):
        assert float(topt.state[p]['step']) == 2.0
        assert np.array_equal(topt.state[p]['exp_avg'].numpy(), c(sd['state'][i]['exp_avg']))
    back = daimc_amd.Adam(m.model_mid.parameters())
    back.load_state_dict(topt.state_dict())
    bsd = back.state_dict()
    assert bsd['param_groups'][0]['lr'] == 2e-4
    for i in range(8):
        for f in ('step', 'exp_avg', 'exp_avg_sq'):
            assert np.array_equal(c(bsd['state'][i][f]), c(sd['state'][i][f])), (i, f)
    assert len(m.parameters()) == 6 + 8 + 32          # ActiveInferenceModel.parameters() keeps working


def test_save_all_load_all_continues_bit_identically(tmp_path):
    import daimc_amd
    b = TM.batch_mid(117, 17)
    s, log_Ppi = TR.batch(117, 17)
    stats = {'var_beta_s': [], 'var_gamma': [], 'var_beta_o': []}
    ma = model_for('g115', fresh=True)
    oa = {'top': daimc_amd.Adam(ma.model_top, lr=1e-3), 'mid': daimc_amd.Adam(ma.model_mid, lr=2e-3)}

    def steps(m, o):
        out = []
        for _ in range(2):
            out.append(c(daimc_amd.loss.train_model_top(m.model_top, s, log_Ppi, o['top'])))
            out += [c(t) for t in engine_train(m, b, o['mid'])]
        return out

    steps(ma, oa)
    ma.save_all(str(tmp_path), stats, optimizers=oa)
    mb = model_for('g100', fresh=True)
    _, ob = mb.load_all(str(tmp_path))
    assert sorted(ob) == ['mid', 'top'] and all(isinstance(o, daimc_amd.Adam) for o in ob.values())
    assert ob['top']._module is mb.model_top and ob['mid']._module is mb.model_mid
    assert ob['top'].param_groups[0]['lr'] == 1e-3 and ob['mid'].param_groups[0]['lr'] == 2e-3
    for x, y in zip(steps(ma, oa), steps(mb, ob)):
        assert np.array_equal(x, y)
    for mod_a, mod_b, keys in ((ma.model_top, mb.model_top, TR.KEYS), (ma.model_mid, mb.model_mid, TM.KEYS)):
        for k in keys:
            assert np.array_equal(c(mod_a.state_dict()[k]), c(mod_b.state_dict()[k])), k
    for name, n in (('top', 6), ('mid', 8)):
        sa, sb = oa[name].state_dict()['state'], ob[name].state_dict()['state']
        for i in range(n):
            for f in ('step', 'exp_avg', 'exp_avg_sq'):
                assert np.array_equal(c(sa[i][f]), c(sb[i][f])), (name, i, f)


# ---- 10. bad arguments -----------------------------------------------------------------------------------------------
def test_bad_arguments_fail_cleanly():
    import daimc_amd
    from daimc_amd import _lib
    m = model_for('g115')
    e = m._ready()
    lib = e.lib
    P = int(lib.efe_param_count(e.ctx, b'ps_net'))
    assert P == 14 * 512 + 512 + 2 * (512 * 512 + 512) + 20 * 512 + 20 == P4
    e3 = model_for('g115', (3, 3, 32))._ready()
    assert int(e3.lib.efe_param_count(e3.ctx, b'ps_net')) == P3
    M = 2
    s0, pi = e.tensor(np.zeros((M, 10), np.float32)), e.tensor(np.eye(4, dtype=np.float32)[:M])
    qm, qv, om = e.tensor(np.zeros((M, 10), np.float32)), e.tensor(np.zeros((M, 10), np.float32)), e.tensor(np.full(M, 2.0, np.float32))
    pm, pv, F = e.empty(M, 10), e.empty(M, 10), e.empty(M)
    g, ea, es = e.empty(P), torch.zeros(P, device=e.device), torch.zeros(P, device=e.device)
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    null, st = C.c_void_p(0), e.stream()
    hp = _lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    nz = _lib.EfeNoise(SEED, STAGE, TM.PASS_FE_T, 0, 0)
    fp = _lib.EfeFeParams(0.0, 0.0, 0.0, _lib.EFE_OMEGA_ARRAY, om.data_ptr(), 0.0, 0.0, 0.0, 0.0, 0.0)
    fp_der = _lib.EfeFeParams(0.0, 0.0, 0.0, _lib.EFE_OMEGA_DERIVED, om.data_ptr(), 0.0, 1.0, 25.0, 5.0, 1.5)
    fp_null = _lib.EfeFeParams(0.0, 0.0, 0.0, _lib.EFE_OMEGA_ARRAY, None, 0.0, 0.0, 0.0, 0.0, 0.0)
    B = C.byref

    def grad(ctx=e.ctx, s0=p(s0), pi=p(pi), qm=p(qm), qv=p(qv), M=M, fp=B(fp), nz=B(nz), pm=p(pm), pv=p(pv), F=p(F), g=p(g)):
        return lib.efe_mid_grad(ctx, s0, pi, qm, qv, M, fp, nz, pm, pv, F, g, st)

    def train(ctx=e.ctx, s0=p(s0), pi=p(pi), qm=p(qm), qv=p(qv), M=M, fp=B(fp), nz=B(nz), pm=p(pm), pv=p(pv), F=p(F), ea=p(ea), es=p(es), hp=B(hp)):
        return lib.efe_train_mid(ctx, s0, pi, qm, qv, M, fp, nz, pm, pv, F, ea, es, hp, st)

    assert grad(M=0) == 1 and b'efe_mid_grad' in lib.efe_last_error(e.ctx)
    for kw in (dict(s0=null), dict(pi=null), dict(qm=null), dict(qv=null), dict(fp=None), dict(nz=None), dict(g=null), dict(M=-1),
               dict(fp=B(fp_der)), dict(fp=B(fp_null))):
        assert grad(**kw) == 1, kw
    assert grad(pm=null, pv=null, F=null) == 0          # the three outputs are optional
    assert train(M=0) == 1 and b'efe_train_mid' in lib.efe_last_error(e.ctx)
    hp0 = _lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 0)
    for kw in (dict(s0=null), dict(pi=null), dict(qm=null), dict(qv=null), dict(fp=None), dict(nz=None), dict(ea=null), dict(es=null), dict(hp=None),
               dict(hp=B(hp0)), dict(fp=B(fp_der))):
        assert train(**kw) == 1, kw
    assert lib.efe_adam_step(e.ctx, b'ps_net', null, p(ea), p(es), B(hp), st) == 1
    assert lib.efe_adam_step(e.ctx, b'ps_net', p(g), p(ea), p(es), None, st) == 1
    assert lib.efe_adam_step(e.ctx, b'nope', p(g), p(ea), p(es), B(hp), st) == 1
    assert b'"top"' in lib.efe_last_error(e.ctx) and b'"ps_net"' in lib.efe_last_error(e.ctx)
    assert lib.efe_get_weights(e.ctx, b'ps_net', p(g), P - 1, st) == 1
    assert lib.efe_get_weights(e.ctx, b'ps_net', null, P, st) == 1
    torch.cuda.synchronize()
    # a CPU tensor through the ops: only the HIP dispatch key is registered
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        e.ops.mid_grad(e.h, z(2, 10), z(2, 4), z(2, 10), z(2, 10), 1, None, 2.0, SEED, STAGE, TM.PASS_FE_T, 0, 0)
    with pytest.raises(NotImplementedError):
        e.ops.train_mid(e.h, z(2, 10), z(2, 4), z(2, 10), z(2, 10), 1, None, 2.0, SEED, STAGE, TM.PASS_FE_T, 0, 0, z(P), z(P), 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):           # wrong-length state
        e.ops.adam_step(e.h, 'ps_net', g, ea[:-1], es, 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):
        e.ops.train_mid(e.h, s0, pi, qm, qv, 1, None, 2.0, SEED, STAGE, TM.PASS_FE_T, 0, 0, ea, es[:-1], 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):           # a gradient of the habit net's length
        e.ops.adam_step(e.h, 'ps_net', g[:18436], ea, es, 1e-3, 0.9, 0.999, 1e-8, 1)
    b = TM.batch_mid(103, 3)
    with pytest.raises(ValueError):             # a foreign optimizer: another model's, and this model's habit-net optimizer
        engine_train(m, b, daimc_amd.Adam(model_for('g100').model_mid))
    with pytest.raises(ValueError):
        engine_train(m, b, daimc_amd.Adam(m.model_top))
    with pytest.raises(TypeError):
        daimc_amd.Adam([torch.zeros(3)])
    # a stale handle: return code 1 from the C ABI, RuntimeError from the ops, nothing dereferenced
    ctx = C.c_void_p()
    assert lib.efe_create(C.byref(ctx), 0) == 0
    h = int(ctx.value)
    lib.efe_destroy(ctx)
    assert grad(ctx=ctx) == 1 and train(ctx=ctx) == 1
    assert lib.efe_adam_step(ctx, b'ps_net', p(g), p(ea), p(es), B(hp), st) == 1
    assert lib.efe_get_weights(ctx, b'ps_net', p(g), P, st) == 1
    assert lib.efe_param_count(ctx, b'ps_net') == 0
    with pytest.raises(RuntimeError):
        e.ops.mid_grad(h, s0, pi, qm, qv, 1, None, 2.0, SEED, STAGE, TM.PASS_FE_T, 0, 0)
    # the context is still good, and none of the refused calls changed the weights
    for k in TM.KEYS:
        assert np.array_equal(c(m.model_mid.state_dict()[k]), family('g115')['mid.' + k]), k
