"""GPU tests (-m gpu) of the habit network's training step on the engine (csrc/train.hip: k_top_grad, k_slab_sum, k_adam; loss.train_model_top,
loss.grad_top, daimc_amd.Adam) against tests/train_ref.py -- autograd and torch.optim.Adam over the CPU oracle in fp32 and fp64, itself
pinned bit for bit to the reference's train_model_top by tests/test_train_top_cpu.py.

Gradients and optimiser results are held to the project's fp64 rule (tests/test_fp64_parity.py fp64_rule):
    max|x_engine - x_64| <= 4 max|x_32 - x_64| + 8 ulp32(max|x_64|)   per parameter tensor,
the returned kl_pi to the KL tolerance of tests/test_free_energy_gpu.py (rtol 1e-5 / atol 1e-4), network outputs after training to its
network tolerance (rtol 1e-5 / atol 2e-6).

Inputs: train_ref.batch(seed, M).  Every gradient case first asserts that no hidden pre-activation of the fp64 oracle lies within 1e-5 of
zero (an fp32 ReLU decision that differs from fp64's is not a kernel error); the seeds below were chosen so that this holds -- 100 + M for
the small batches, 2002 for M = 1025 (2000 and 2001 violate it).  Weight families: make_weights(1234, 1.15), make_weights(7, 1.0),
stress_weights('sparse'), stress_weights('saturated') (whose habit net is the 1.15 family's: it saturates the decoder), and 'sat_top', the
same with qpi_net.4.weight x 40 in the manner of that family, which drives some Qpi to exactly 0 in fp32 and exercises the 1e-20 term."""
import ctypes as C

import numpy as np
import pytest
import torch

import free_energy_ref as FR
import train_ref as TR
from conftest import load_golden
from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise
from train_common import SEED, apply_rule, c, family, model_for, synth_grads, torch_adam_run

pytestmark = pytest.mark.gpu

WALK_M = 64 * 16 + 1            # k_top_grad runs at most 64 workgroups (csrc/kernels.h TRAIN_MAX_SLABS): workgroup 0 walks a second tile


def check_grads(tag, m, weights, s, log_Ppi, pi_dim=4):
    import daimc_amd
    assert TR.preact_margin(weights, s, pi_dim) >= 1e-5, 'precondition: a hidden pre-activation within 1e-5 of zero (pick another seed)'
    kl, g = daimc_amd.loss.grad_top(m.model_top, s, log_Ppi)
    kl32, g32 = TR.grads(weights, s, log_Ppi, torch.float32, pi_dim)
    _, g64 = TR.grads(weights, s, log_Ppi, torch.float64, pi_dim)
    assert list(g) == list(TR.KEYS)
    np.testing.assert_allclose(c(kl), kl32, rtol=1e-5, atol=1e-4, err_msg=tag + ' kl_pi')
    apply_rule(tag, [(k, c(g[k]), g32[k], g64[k]) for k in TR.KEYS])
    return {k: c(v) for k, v in g.items()}


GRAD_CASES = [('g115', M, 100 + M) for M in (1, 3, 16, 17, 50)] + [('g115', WALK_M, 2002)] + \
             [(f, M, 100 + M) for f in ('g100', 'sparse', 'saturated', 'sat_top') for M in (17, 50)]


@pytest.mark.parametrize('fam,M,seed', GRAD_CASES)
def test_gradients_vs_fp64(fam, M, seed):
    s, log_Ppi = TR.batch(seed, M)
    w = family(fam)
    if fam == 'sat_top':
        orc, _ = TR.oracle(w)
        with torch.no_grad():
            assert int((orc.encode_s(torch.as_tensor(s))[1] == 0).sum()) > 0, 'precondition: some Qpi exactly 0 in fp32'
    g = check_grads(f'{fam} M={M}', model_for(fam), w, s, log_Ppi)
    assert all(np.isfinite(v).all() for v in g.values())


def test_gradients_generic_geometry():
    """pi_dim 3 on a 3 x 32 x 32 context: three logits, the same kernels"""
    geo = (3, 3, 32)
    s, log_Ppi = TR.batch(117, 17, 3)
    check_grads('generic M=17', model_for('g115', geo), family('g115', geo), s, log_Ppi, pi_dim=3)


def test_gradients_of_reference_fixture():
    import daimc_amd
    g = load_golden('train_top_g115')
    w = family('g115')
    kl, ge = daimc_amd.loss.grad_top(model_for('g115').model_top, g['s'], g['log_Ppi'])
    _, g64 = TR.grads(w, g['s'], g['log_Ppi'], torch.float64)
    np.testing.assert_allclose(c(kl), g['kl_pi_1'], rtol=1e-5, atol=1e-4)
    apply_rule('fixture', [(k, c(ge[k]), g['grad1.' + k], g64[k]) for k in TR.KEYS])


def test_dead_units_have_exactly_zero_gradient():
    """a hidden unit that is inactive for every row of the batch: its weight row, bias and outgoing column get exactly 0"""
    import daimc_amd
    w = family('g115')
    s, log_Ppi = TR.batch(103, 3)
    orc, _ = TR.oracle(w, torch.float64)
    with torch.no_grad():
        x = torch.as_tensor(s).double()
        a1 = torch.nn.functional.linear(x, orc.w['top.qpi_net.0.weight'], orc.w['top.qpi_net.0.bias'])
        a2 = torch.nn.functional.linear(torch.relu(a1), orc.w['top.qpi_net.2.weight'], orc.w['top.qpi_net.2.bias'])
        assert TR.preact_margin(w, s) >= 1e-5
        dead1 = np.nonzero((a1 <= 0).all(0).numpy())[0]
        dead2 = np.nonzero((a2 <= 0).all(0).numpy())[0]
    assert len(dead1) > 0 and len(dead2) > 0, 'precondition: the batch leaves units of both hidden layers inactive'
    _, g = daimc_amd.loss.grad_top(model_for('g115').model_top, s, log_Ppi)
    g = {k: c(v) for k, v in g.items()}
    assert not g['qpi_net.0.weight'][dead1].any() and not g['qpi_net.0.bias'][dead1].any() and not g['qpi_net.2.weight'][:, dead1].any()
    assert not g['qpi_net.2.weight'][dead2].any() and not g['qpi_net.2.bias'][dead2].any() and not g['qpi_net.4.weight'][:, dead2].any()
    assert g['qpi_net.2.weight'].any() and g['qpi_net.4.weight'].any()


@pytest.mark.parametrize('M,seed', [(3, 103), (50, 150), (WALK_M, 2002)])
def test_reproducible(M, seed):
    import daimc_amd
    s, log_Ppi = TR.batch(seed, M)
    m = model_for('g115')
    kl1, g1 = daimc_amd.loss.grad_top(m.model_top, s, log_Ppi)
    kl2, g2 = daimc_amd.loss.grad_top(m.model_top, s, log_Ppi)
    assert np.array_equal(c(kl1), c(kl2))
    for k in TR.KEYS:
        assert np.array_equal(c(g1[k]), c(g2[k])), k


# ---- Adam alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['fresh', 'loaded_step_1000', 'zero_weights'])
def test_adam_three_steps_vs_fp64(case):
    import daimc_amd
    m = model_for('g115', fresh=True)
    w0 = {k: np.array(family('g115')['top.' + k], dtype=np.float32) for k in TR.KEYS}
    if case == 'zero_weights':          # the update itself is resolved, not hidden under ulp(w)
        w0 = {k: np.zeros_like(v) for k, v in w0.items()}
        m.model_top.load_state_dict({k: torch.from_numpy(v) for k, v in w0.items()})
    shapes = [w0[k].shape for k in TR.KEYS]
    steps = [synth_grads(900 + i, shapes) for i in range(3)]
    lr = 1e-3
    opt = daimc_amd.Adam(m.model_top, lr=lr)
    state = None
    if case == 'loaded_step_1000':
        r = np.random.RandomState(5)
        state = {'step': 1000, 'm': [(r.randn(*s) * 1e-2).astype(np.float32) for s in shapes],
                 'v': [(r.uniform(0, 1e-3, s)).astype(np.float32) for s in shapes]}
        sd = opt.state_dict()
        sd['state'] = {i: {'step': torch.tensor(1000.0), 'exp_avg': torch.from_numpy(state['m'][i].copy()), 'exp_avg_sq': torch.from_numpy(state['v'][i].copy())}
                       for i in range(6)}
        opt.load_state_dict(sd)
    for gs in steps:
        opt.step(torch.from_numpy(np.concatenate([g.reshape(-1) for g in gs])))
    sd, osd = m.model_top.state_dict(), opt.state_dict()
    assert int(osd['state'][0]['step']) == (1003 if state else 3)
    w32, m32, v32 = torch_adam_run(TR.KEYS, w0, steps, torch.float32, lr, state)
    w64, m64, v64 = torch_adam_run(TR.KEYS, w0, steps, torch.float64, lr, state)
    trip = []
    for i, k in enumerate(TR.KEYS):
        trip += [('exp_avg.' + k, c(osd['state'][i]['exp_avg']), m32[i], m64[i]), ('exp_avg_sq.' + k, c(osd['state'][i]['exp_avg_sq']), v32[i], v64[i]),
                 ('w.' + k, c(sd[k]), w32[i], w64[i])]
        assert not np.array_equal(c(sd[k]), w0[k]), k
    apply_rule('adam ' + case, trip)


# ---- composition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,seed', [(3, 103), (50, 150)])
def test_train_model_top_is_grad_then_adam(M, seed):
    import daimc_amd
    s, log_Ppi = TR.batch(seed, M)
    ma, mb = model_for('g115', fresh=True), model_for('g115', fresh=True)
    oa, ob = daimc_amd.Adam(ma.model_top, lr=1e-3), daimc_amd.Adam(mb.model_top.parameters(), lr=1e-3)
    for _ in range(2):
        kla = daimc_amd.loss.train_model_top(ma.model_top, s, log_Ppi, oa)
        klb, g = daimc_amd.loss.grad_top(mb.model_top, s, log_Ppi)
        ob.step(g)
        assert np.array_equal(c(kla), c(klb))
    sa, sb = ma.model_top.state_dict(), mb.model_top.state_dict()
    for k in TR.KEYS:
        assert np.array_equal(c(sa[k]), c(sb[k])), k
        assert not np.array_equal(c(sa[k]), family('g115')['top.' + k]), k
    for i in range(6):
        for f in ('exp_avg', 'exp_avg_sq', 'step'):
            assert np.array_equal(c(oa.state_dict()['state'][i][f]), c(ob.state_dict()['state'][i][f])), (i, f)


# ---- every forward path sees the step --------------------------------------------------------------------------------
def test_forward_paths_see_the_step():
    import daimc_amd
    NET = dict(rtol=1e-5, atol=2e-6)
    w = family('g115')
    m = model_for('g115', fresh=True)
    m.eps_source, m.u_source = PX.normals, PX.uniforms
    s, log_Ppi = TR.batch(117, 17)
    starts = s[:4]
    frames = synth.make_frames(21, 4)
    pi0 = np.eye(4, dtype=np.float32)
    before = c(m.model_top.encode_s(s)[1])
    replica_before = m.cached_replica()
    opt = daimc_amd.Adam(m.model_top, lr=1e-3)
    for _ in range(2):
        daimc_amd.loss.train_model_top(m.model_top, s, log_Ppi, opt)
    sd = m.model_top.state_dict()
    w2 = dict(w)
    for k in TR.KEYS:
        w2['top.' + k] = c(sd[k])
        assert not np.array_equal(w2['top.' + k], w['top.' + k]), k
    orc = OracleModel(w2, PhiloxNoise(SEED))
    with torch.no_grad():
        ol, oq, olq = (t.numpy() for t in orc.encode_s(torch.from_numpy(s)))
        oq_starts = orc.encode_s(torch.from_numpy(starts))[1].numpy()
        fe_ref = FR.free_energy(orc, frames, frames, pi0, log_Ppi[:4], 0.5, stage=3)
    assert np.abs(oq - before).max() > 1e-4, 'the two steps must move the habit posterior visibly'

    def check_paths(mod, tag):
        lg, q, lq = (c(t) for t in mod.model_top.encode_s(s))                                    # layer-wise 32x32x2 packing
        np.testing.assert_allclose(lg, ol, err_msg=tag + ' logits', **NET)
        np.testing.assert_allclose(q, oq, err_msg=tag + ' Qpi', **NET)
        np.testing.assert_allclose(lq, olq, err_msg=tag + ' log_Qpi', **NET)
        q0 = c(mod.simulate_batch(starts, 2, use_means=False, stage=11)[2])                       # fused 16x16x4 packing (k_sim_chain)
        np.testing.assert_allclose(q0, oq_starts, err_msg=tag + ' simulate Qpi0', **NET)
        fe = daimc_amd.free_energy(mod, frames, frames, pi0, log_Ppi[:4], stage=3)
        np.testing.assert_allclose(c(fe.Qpi), fe_ref['Qpi'].numpy(), err_msg=tag + ' free_energy Qpi', **NET)

    check_paths(m, 'model')
    r = m.cached_replica()
    assert r is not replica_before, 'a step bumps the weight version: the cached replica is rebuilt'
    check_paths(r, 'replica')
    m.model_mid.load_state_dict(m.model_mid.state_dict())           # a re-commit must not revert the habit net
    check_paths(m, 're-commit')
    for k in TR.KEYS:
        assert np.array_equal(c(m.model_top.state_dict()[k]), w2['top.' + k]), k


# ---- descent ---------------------------------------------------------------------------------------------------------
def test_descent():
    """20 steps at lr 1e-4 on batch(117, 17): mean kl_pi falls strictly every step and ends at <= 0.85 of its start (the fp32 CPU oracle
    goes 1.24005 -> 0.95232, ratio 0.77, monotone)"""
    import daimc_amd
    s, log_Ppi = TR.batch(117, 17)
    m = model_for('g115', fresh=True)
    opt = daimc_amd.Adam(m.model_top, lr=1e-4)
    kls = [float(c(daimc_amd.loss.train_model_top(m.model_top, s, log_Ppi, opt)).mean()) for _ in range(20)]
    kls.append(float(c(daimc_amd.loss.compute_loss_top(m.model_top, s, log_Ppi)[1]).mean()))
    print('mean kl_pi per step:', ' '.join(f'{v:.5f}' for v in kls))
    assert all(b < a for a, b in zip(kls, kls[1:])), kls
    assert kls[-1] <= 0.85 * kls[0], (kls[0], kls[-1])


# ---- optimiser state interchange -------------------------------------------------------------------------------------
def test_state_dict_moves_to_torch_and_back():
    import daimc_amd
    s, log_Ppi = TR.batch(117, 17)
    m = model_for('g115', fresh=True)
    opt = daimc_amd.Adam(m.model_top, lr=2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert opt.param_groups[0]['lr'] == 2e-4
    assert opt.state_dict()['state'] == {}
    for _ in range(2):
        daimc_amd.loss.train_model_top(m.model_top, s, log_Ppi, opt)
    sd = opt.state_dict()
    params = [torch.nn.Parameter(t.clone()) for t in m.model_top.parameters()]
    topt = torch.optim.Adam(params, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['lr'] == 2e-4 and tuple(topt.param_groups[0]['betas']) == (0.8, 0.99) and topt.param_groups[0]['eps'] == 1e-7
    for i, p in enumerate(params):
        assert float(topt.state[p]['step']) == 2.0
        assert np.array_equal(topt.state[p]['exp_avg'].numpy(), c(sd['state'][i]['exp_avg']))
    back = daimc_amd.Adam(m.model_top.parameters())
    back.load_state_dict(topt.state_dict())
    bsd = back.state_dict()
    assert bsd['param_groups'][0]['lr'] == 2e-4
    for i in range(6):
        for f in ('step', 'exp_avg', 'exp_avg_sq'):
            assert np.array_equal(c(bsd['state'][i][f]), c(sd['state'][i][f])), (i, f)


def test_save_all_load_all_continues_bit_identically(tmp_path):
    import daimc_amd
    s, log_Ppi = TR.batch(117, 17)
    stats = {'var_beta_s': [], 'var_gamma': [], 'var_beta_o': []}
    ma = model_for('g115', fresh=True)
    oa = daimc_amd.Adam(ma.model_top, lr=1e-3)
    for _ in range(2):
        daimc_amd.loss.train_model_top(ma.model_top, s, log_Ppi, oa)
    ma.save_all(str(tmp_path), stats, optimizers={'top': oa})
    mb = model_for('g100', fresh=True)
    _, opts = mb.load_all(str(tmp_path))
    assert list(opts) == ['top'] and isinstance(opts['top'], daimc_amd.Adam) and opts['top'].param_groups[0]['lr'] == 1e-3
    for _ in range(2):
        kla = daimc_amd.loss.train_model_top(ma.model_top, s, log_Ppi, oa)
        klb = daimc_amd.loss.train_model_top(mb.model_top, s, log_Ppi, opts['top'])
        assert np.array_equal(c(kla), c(klb))
    for k in TR.KEYS:
        assert np.array_equal(c(ma.model_top.state_dict()[k]), c(mb.model_top.state_dict()[k])), k
    sa, sb = oa.state_dict()['state'], opts['top'].state_dict()['state']
    for i in range(6):
        for f in ('step', 'exp_avg', 'exp_avg_sq'):
            assert np.array_equal(c(sa[i][f]), c(sb[i][f])), (i, f)


# ---- bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_fail_cleanly():
    import daimc_amd
    from daimc_amd import _lib
    m = model_for('g115')
    e = m._ready()
    lib = e.lib
    P = int(lib.efe_param_count(e.ctx, b'top'))
    assert P == 10 * 128 + 128 + 128 * 128 + 128 + 4 * 128 + 4 == 18436
    assert lib.efe_param_count(e.ctx, b'mid') == 0
    s, lp = e.tensor(np.zeros((2, 10), np.float32)), e.tensor(np.full((2, 4), -1.386, np.float32))
    kl, g, ea, es = e.empty(2), e.empty(P), torch.zeros(P, device=e.device), torch.zeros(P, device=e.device)
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    null, st = C.c_void_p(0), e.stream()
    hp = _lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    assert lib.efe_top_grad(e.ctx, p(s), p(lp), 0, p(kl), p(g), st) == 1 and b'efe_top_grad' in lib.efe_last_error(e.ctx)
    assert lib.efe_top_grad(e.ctx, null, p(lp), 2, p(kl), p(g), st) == 1
    assert lib.efe_top_grad(e.ctx, p(s), null, 2, p(kl), p(g), st) == 1
    assert lib.efe_top_grad(e.ctx, p(s), p(lp), 2, p(kl), null, st) == 1
    assert lib.efe_top_grad(e.ctx, p(s), p(lp), 2, null, p(g), st) == 0          # kl_pi is optional
    assert lib.efe_adam_step(e.ctx, b'top', null, p(ea), p(es), C.byref(hp), st) == 1
    assert lib.efe_adam_step(e.ctx, b'top', p(g), p(ea), p(es), None, st) == 1
    assert lib.efe_adam_step(e.ctx, b'mid', p(g), p(ea), p(es), C.byref(hp), st) == 1
    hp0 = _lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 0)
    assert lib.efe_adam_step(e.ctx, b'top', p(g), p(ea), p(es), C.byref(hp0), st) == 1
    assert lib.efe_train_top(e.ctx, p(s), p(lp), -1, p(kl), p(ea), p(es), C.byref(hp), st) == 1
    assert lib.efe_train_top(e.ctx, p(s), p(lp), 2, p(kl), null, p(es), C.byref(hp), st) == 1
    assert lib.efe_get_weights(e.ctx, b'top', p(g), P - 1, st) == 1
    assert lib.efe_get_weights(e.ctx, b'top', null, P, st) == 1
    torch.cuda.synchronize()
    # a CPU tensor through the ops: only the HIP dispatch key is registered
    with pytest.raises(NotImplementedError):
        e.ops.top_grad(e.h, torch.zeros(2, 10), torch.zeros(2, 4))
    with pytest.raises(NotImplementedError):
        e.ops.train_top(e.h, torch.zeros(2, 10), torch.zeros(2, 4), torch.zeros(P), torch.zeros(P), 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):
        e.ops.adam_step(e.h, 'top', g, ea[:-1], es, 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(ValueError):
        daimc_amd.loss.train_model_top(m.model_top, s, lp, daimc_amd.Adam(model_for('g100').model_top))
    with pytest.raises(TypeError):
        daimc_amd.Adam([torch.zeros(3)])
    # a stale handle: return code 1 from the C ABI, RuntimeError from the ops, nothing dereferenced
    ctx = C.c_void_p()
    assert lib.efe_create(C.byref(ctx), 0) == 0
    h = int(ctx.value)
    lib.efe_destroy(ctx)
    assert lib.efe_top_grad(ctx, p(s), p(lp), 2, p(kl), p(g), st) == 1
    assert lib.efe_train_top(ctx, p(s), p(lp), 2, p(kl), p(ea), p(es), C.byref(hp), st) == 1
    assert lib.efe_adam_step(ctx, b'top', p(g), p(ea), p(es), C.byref(hp), st) == 1
    assert lib.efe_get_weights(ctx, b'top', p(g), P, st) == 1
    assert lib.efe_param_count(ctx, b'top') == 0
    with pytest.raises(RuntimeError):
        e.ops.top_grad(h, s, lp)
    # the context is still good, and none of the refused calls changed the weights
    for k in TR.KEYS:
        assert np.array_equal(c(m.model_top.state_dict()[k]), family('g115')['top.' + k]), k
