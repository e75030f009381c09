"""GPU tests (-m gpu) of ModelDown's optimiser step (csrc/train_down.hip: k_adam_down + k_repack_down; efe_train_down, efe_down_adam_step,
efe_down_get_weights; loss.train_model_down, daimc_amd.Adam over model_down).

Engine seed 7, weights 'g115', inputs train_down_ref.inputs(2000 + M, M); every training call passes the fixed stage 3, so the dropout
masks and the objective are the same at each step.  The batch sizes are the smallest at which the code can go wrong: M = 1 (one row, the
gradient is the slab), 3 (one row group), 65 (two row groups, one ragged), and the reference's 50 in the composition test.

The repack test compares the trained model with a FRESH model built by the host packers from the downloaded weights, bit for bit, on every
reader of the packed forms that engine_forward.hip's launch code has at 1 x 64 x 64 (DESIGN.md section 7g lists the forms against these calls):
    encoder / encoder_with_sample        k_enc_trunk (enc_w1, enc_b1, conv2 / conv3 taps, conv4 16x16x4), k_head (enc16) or, head_unfused,
                                         k_dense (enc_fc 32x32x2, the first layer's columns NHWC)
    decoder                              k_head (dec16) or k_dense (dec_fc), k_fc4 (po_net.9, rows NHWC), k_dec_a_s / k_dec_a (Winograd of
                                         po_net.13, F(2,2) of po_net.15; dec_split 0 selects the persistent k_dec_a), k_dec_b4 (F(2,2) of
                                         po_net.17, the final taps, po_net.19.bias by value)
    calculate_G, simulate_batch          the same through the rollout's launch groups
    free_energy, compute_loss_down       the same through loss.hip's callers
    grad_down                            the raw copy (train_enc.hip, train_dec_head.hip, train_dec.hip)
and against the CPU oracle on the downloaded weights, so that "fresh" cannot be wrong in the same way."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_down_ref as TDN
from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise
from train_common import SEED, apply_rule, c, family, model_for, synth_grads, torch_adam_run

pytestmark = pytest.mark.gpu

STAGE = 3
KEYS = TDN.KEYS
NK = len(KEYS)          # 32


def batch(M):
    return TDN.inputs(2000 + M, M)


def train(m, opt, b, **kw):
    import daimc_amd
    o1, pm, pv, om = b
    return daimc_amd.loss.train_model_down(m.model_down, o1, pm, pv, om, opt, stage=STAGE, **kw)


def grad(m, b):
    import daimc_amd
    o1, pm, pv, om = b
    return daimc_amd.loss.grad_down(m.model_down, o1, pm, pv, om, stage=STAGE)


def down_weights(m):
    return {k: c(v) for k, v in m.model_down.state_dict().items()}


def model_from(w):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=SEED, init_weights=False)
    m.load_flat_weights(w)
    return m


def with_down(w, down):
    w2 = dict(w)
    for k in KEYS:
        w2['down.' + k] = down[k]
    return w2


def opt_state(opt):
    sd = opt.state_dict()['state']
    return [c(sd[i][f]) for i in range(NK) for f in ('step', 'exp_avg', 'exp_avg_sq')]


def flat_of(x):
    """every tensor of a call's result, in order, as numpy arrays"""
    if isinstance(x, torch.Tensor):
        return [c(x)]
    if isinstance(x, dict):
        return [a for v in x.values() for a in flat_of(v)]
    if isinstance(x, (tuple, list)):
        return [a for v in x for a in flat_of(v)]
    return []


def same_bits(tag, a, b):
    fa, fb = flat_of(a), flat_of(b)
    assert len(fa) == len(fb) and len(fa) > 0, tag
    for i, (p, q) in enumerate(zip(fa, fb)):
        assert p.shape == q.shape and p.tobytes() == q.tobytes(), f'{tag}: output {i} differs (max |d| {np.abs(p.astype(np.float64) - q).max():.3e})'


# ---- 1. Adam alone against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['fresh', 'loaded_step_1000', 'zero_weights'])
def test_adam_three_steps_vs_fp64(case):
    import daimc_amd
    m = model_for('g115', fresh=True)
    w0 = {k: np.array(family('g115')['down.' + k], dtype=np.float32) for k in KEYS}
    if case == 'zero_weights':          # the update itself is resolved, not hidden under ulp(w)
        w0 = {k: np.zeros_like(v) for k, v in w0.items()}
        m.model_down.load_state_dict({k: torch.from_numpy(v) for k, v in w0.items()})
    shapes = [w0[k].shape for k in KEYS]
    steps = [synth_grads(900 + i, shapes) for i in range(3)]
    lr = 1e-3
    opt = daimc_amd.Adam(m.model_down, lr=lr)
    state = None
    if case == 'loaded_step_1000':
        r = np.random.RandomState(5)
        state = {'step': 1000, 'm': [(r.randn(*s) * 1e-2).astype(np.float32) for s in shapes],
                 'v': [(r.uniform(0, 1e-3, s)).astype(np.float32) for s in shapes]}
        sd = opt.state_dict()
        sd['state'] = {i: {'step': torch.tensor(1000.0), 'exp_avg': torch.from_numpy(state['m'][i].copy()), 'exp_avg_sq': torch.from_numpy(state['v'][i].copy())}
                       for i in range(NK)}
        opt.load_state_dict(sd)
    for gs in steps:
        opt.step(torch.from_numpy(np.concatenate([g.reshape(-1) for g in gs])))
    sd, osd = m.model_down.state_dict(), opt.state_dict()
    assert int(osd['state'][0]['step']) == (1003 if state else 3)
    w32, m32, v32 = torch_adam_run(KEYS, w0, steps, torch.float32, lr, state)
    w64, m64, v64 = torch_adam_run(KEYS, w0, steps, torch.float64, lr, state)
    trip, differ, total = [], 0, 0
    for i, k in enumerate(KEYS):
        trip += [('exp_avg.' + k, c(osd['state'][i]['exp_avg']), m32[i], m64[i]), ('exp_avg_sq.' + k, c(osd['state'][i]['exp_avg_sq']), v32[i], v64[i]),
                 ('w.' + k, c(sd[k]), w32[i], w64[i])]
        assert not np.array_equal(c(sd[k]), w0[k]), k
        differ += int((c(sd[k]) != w32[i]).sum()); total += w32[i].size
    print(f'adam {case}: {differ} of {total} weights differ from the fp32 torch.optim.Adam run')
    apply_rule('adam_down ' + case, trip)


# ---- 2. composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [3, 65, 50])
def test_train_model_down_is_grad_then_adam(M):
    import daimc_amd
    b = batch(M)
    ma, mb = model_for('g115', fresh=True), model_for('g115', fresh=True)
    oa, ob = daimc_amd.Adam(ma.model_down, lr=1e-3), daimc_amd.Adam(mb.model_down.parameters(), lr=1e-3)
    for _ in range(2):
        Fa, ta = train(ma, oa, b)
        out = grad(mb, b)
        ob.step(out[6])
        assert np.array_equal(c(Fa), c(out[0]))
        same_bits('terms', ta, out[1])
    sa, sb = down_weights(ma), down_weights(mb)
    for k in KEYS:
        assert np.array_equal(sa[k], sb[k]), k
        assert not np.array_equal(sa[k], family('g115')['down.' + k]), k
    for x, y in zip(opt_state(oa), opt_state(ob)):
        assert np.array_equal(x, y)
    assert oa._step == ob._step == 2


# ---- 3. every forward path sees the step -----------------------------------------------------------------------------
def forward_calls(mod, cfg_only=False):
    """the readers of the packed forms (the file's head); cfg_only: those an engine option can route differently"""
    import daimc_amd
    out = {}
    for M in (1, 65):
        o1, pm, pv, om = batch(M)
        s = pm                                                      # any [M, 10] latent
        out[f'encoder M={M}'] = mod.model_down.encoder(o1, stage=5)
        out[f'encoder_with_sample M={M}'] = mod.model_down.encoder_with_sample(o1, stage=5)
        out[f'decoder M={M}'] = mod.model_down.decoder(s, stage=6)
    o1, pm, pv, om = batch(3)
    pi0 = np.eye(4, dtype=np.float32)[[0, 1, 3]]
    out['calculate_G'] = mod.calculate_G(pm, pi0, samples=2, stage=7)
    if cfg_only:
        return out
    out['simulate_batch'] = mod.simulate_batch(pm, 2, use_means=False, stage=11)
    frames = synth.make_frames(21, 3)
    out['free_energy'] = tuple(daimc_amd.free_energy(mod, frames, frames, pi0, np.log(np.full((3, 4), 0.25, np.float32)), stage=3))
    out['compute_loss_down'] = daimc_amd.loss.compute_loss_down(mod.model_down, o1, pm, pv, om, stage=STAGE)
    out['grad_down'] = grad(mod, (o1, pm, pv, om))
    return out


OPTION_READERS = [('ct_fuse12', 0, 1), ('enc_tiled', 0, 2), ('enc_tiled', 1, 2), ('head_unfused', 1, 0), ('dec_split', 0, 1)]


def test_forward_paths_see_the_step():
    import daimc_amd
    NET = dict(rtol=1e-5, atol=2e-6)
    w = family('g115')
    m = model_for('g115', fresh=True)
    m.eps_source, m.u_source = PX.normals, PX.uniforms
    b = batch(65)
    o_probe, s_probe = batch(3)[0], batch(3)[1]
    before_po = c(m.model_down.decoder(s_probe, stage=6))
    before_qm = c(m.model_down.encoder(o_probe, stage=5)[0])
    replica_before = m.cached_replica()
    opt = daimc_amd.Adam(m.model_down, lr=1e-3)
    for _ in range(2):
        train(m, opt, b)
    down = down_weights(m)
    for k in KEYS:
        assert not np.array_equal(down[k], w['down.' + k]), k
    w2 = with_down(w, down)
    fresh = model_from(w2)
    fresh.eps_source, fresh.u_source = PX.normals, PX.uniforms

    # the oracle on the downloaded weights: "fresh" cannot be wrong in the same way
    orc = OracleModel(w2, PhiloxNoise(SEED))
    with torch.no_grad():
        o_po = orc.decoder(torch.from_numpy(s_probe), daimc_amd.model.PASS_D1, 0, 6).numpy()
        o_qm = orc.encoder(torch.from_numpy(o_probe), daimc_amd.model.PASS_ROOT, 0, 5)[0].numpy()
    po, qm = c(m.model_down.decoder(s_probe, stage=6)), c(m.model_down.encoder(o_probe, stage=5)[0])
    print(f'oracle: po1 max |d| {np.abs(po - o_po).max():.3e}, qs_mean max |d| {np.abs(qm - o_qm).max():.3e}; '
          f'moved by the steps: po1 {np.abs(po - before_po).max():.3e}, qs_mean {np.abs(qm - before_qm).max():.3e}')
    np.testing.assert_allclose(po, o_po.reshape(po.shape), err_msg='decoder vs oracle', **NET)
    np.testing.assert_allclose(qm, o_qm, err_msg='encoder vs oracle', **NET)
    assert np.abs(po - before_po).max() > 1e-4 and np.abs(qm - before_qm).max() > 1e-4, 'the two steps must move po1 and qs_mean visibly'

    def check_paths(mod, tag, cfg_only=False):
        got, want = forward_calls(mod, cfg_only), forward_calls(fresh, cfg_only)
        for name in want:
            same_bits(f'{tag}: {name}', got[name], want[name])

    check_paths(m, 'model')
    for name, value, default in OPTION_READERS:
        m.set_option(name, value); fresh.set_option(name, value)
        try:
            check_paths(m, f'{name}={value}', cfg_only=True)
        finally:
            m.set_option(name, default); fresh.set_option(name, default)
    r = m.cached_replica()
    assert r is not replica_before, 'a step bumps the weight version: the cached replica is rebuilt'
    check_paths(r, 'replica', cfg_only=True)
    m.model_top.load_state_dict(m.model_top.state_dict())           # a re-commit must not revert ModelDown
    check_paths(m, 're-commit', cfg_only=True)
    for k in KEYS:
        assert np.array_equal(down_weights(m)[k], down[k]), k


def test_recommit_and_partial_set_weight_keep_the_trained_tensors():
    """at the C ABI, without the Python side's own download: efe_commit_weights alone, then efe_set_weight of ONE down tensor + commit"""
    import daimc_amd
    w = family('g115')
    m = model_for('g115', fresh=True)
    e = m._ready()
    opt = daimc_amd.Adam(m.model_down, lr=1e-3)
    train(m, opt, batch(3))
    down = down_weights(m)
    P = TDN.P

    def master():
        buf = torch.empty(P, device='cuda:0')
        assert e.lib.efe_down_get_weights(e.ctx, C.c_void_p(buf.data_ptr()), P, e.stream()) == 0
        return c(buf)
    flat = np.concatenate([down[k].reshape(-1) for k in KEYS])
    assert np.array_equal(master(), flat)
    assert e.lib.efe_commit_weights(e.ctx) == 0                     # the host tensors still hold the weights before the step
    assert np.array_equal(master(), flat)
    new = np.full((20,), 0.125, np.float32)
    shape = (C.c_int64 * 1)(20)
    assert e.lib.efe_set_weight(e.ctx, b'down.qs_net.18.bias', C.c_void_p(new.ctypes.data), shape, 1) == 0
    assert e.lib.efe_commit_weights(e.ctx) == 0
    want = dict(down); want['qs_net.18.bias'] = new
    assert np.array_equal(master(), np.concatenate([want[k].reshape(-1) for k in KEYS]))
    fresh = model_from(with_down(w, want))
    m.model_down._sd = {k: torch.from_numpy(v.copy()) for k, v in want.items()}      # (the Python copy follows; no re-upload: _weights_dirty stays False)
    for name, a in forward_calls(m, cfg_only=True).items():
        same_bits('partial set_weight: ' + name, a, forward_calls(fresh, cfg_only=True)[name])
    # and through load_state_dict: one replaced tensor, 31 trained ones
    m2 = model_for('g115', fresh=True)
    o2 = daimc_amd.Adam(m2.model_down, lr=1e-3)
    train(m2, o2, batch(3))
    sd = m2.model_down.state_dict()
    sd['po_net.19.bias'] = torch.tensor([0.5])
    m2.model_down.load_state_dict(sd)
    got = down_weights(m2)
    for k in KEYS:
        assert np.array_equal(got[k], c(sd[k])), k
        if k != 'po_net.19.bias':
            assert np.array_equal(got[k], down[k]), k
    same_bits('load_state_dict', m2.model_down.decoder(batch(3)[1], stage=6), model_from(with_down(w, got)).model_down.decoder(batch(3)[1], stage=6))


@pytest.mark.parametrize('opt', ['mfma_bf16x3', 'mfma_f16x2'])
@pytest.mark.parametrize('way', ['first_on_after_the_step', 'on_off_step_on'])
def test_split_operand_planes_follow_the_step(opt, way):
    """The 16-bit planes of po_net.9 / .13 / .15 / .17 (bf16x3.hip) are packed on the host from the host tensors when the option goes on.  A
    step is refused while it is on; turned on AFTER a step -- for the first time, or again with planes of the old weights still packed --
    it must pack the trained weights: the decoder equals, bit for bit, a fresh model of the downloaded weights under the same option.
    130 images run the large-launch kernels (k_fc4_b3, k_dec_a_b3, k_dec_b_b3); calculate_G runs them under dec_split = 0."""
    import daimc_amd
    w = family('g115')
    m = model_for('g115', fresh=True)
    m._ready()
    s130 = TDN.inputs(2130, 130)[1]
    o1, pm, pv, om = batch(3)
    pi0 = np.eye(4, dtype=np.float32)[[0, 1, 3]]
    if way == 'on_off_step_on':
        m.set_option(opt, 1)
        old = c(m.model_down.decoder(s130, stage=6))
        m.set_option(opt, 0)
    else:
        old = None
    o = daimc_amd.Adam(m.model_down, lr=1e-3)
    for _ in range(2):
        train(m, o, (o1, pm, pv, om))
    m.set_option(opt, 1)
    fresh = model_from(with_down(w, down_weights(m)))
    fresh.set_option(opt, 1)
    got = m.model_down.decoder(s130, stage=6)
    same_bits(f'{opt} {way}: decoder', got, fresh.model_down.decoder(s130, stage=6))
    if old is not None:
        assert not np.array_equal(c(got), old)
    m.set_option('dec_split', 0); fresh.set_option('dec_split', 0)
    same_bits(f'{opt} {way}: calculate_G', m.calculate_G(pm, pi0, samples=2, stage=7), fresh.calculate_G(pm, pi0, samples=2, stage=7))
    with pytest.raises(RuntimeError):           # and while the option is on a step is refused, by name
        train(m, o, (o1, pm, pv, om))
    assert o._step == 2


# ---- 4. the last bias alone ------------------------------------------------------------------------------------------
def test_last_bias_alone_reaches_the_decoder():
    import daimc_amd
    w = family('g115')
    m = model_for('g115', fresh=True)
    s = batch(3)[1]
    before = c(m.model_down.decoder(s, stage=6))
    g = torch.zeros(TDN.P)
    g[-1] = 1.0
    daimc_amd.Adam(m.model_down, lr=1e-2).step(g)
    after = c(m.model_down.decoder(s, stage=6))
    down = down_weights(m)
    for k in KEYS:
        assert np.array_equal(down[k], w['down.' + k]) == (k != 'po_net.19.bias'), k
    assert not np.array_equal(after, before)
    assert np.array_equal(after, c(model_from(with_down(w, down)).model_down.decoder(s, stage=6)))


# ---- 5. reproducibility ----------------------------------------------------------------------------------------------
def test_reproducible():
    import daimc_amd
    res = []
    for _ in range(2):
        m = model_for('g115', fresh=True)
        opt = daimc_amd.Adam(m.model_down, lr=1e-3)
        Fs = [c(train(m, opt, batch(65))[0]) for _ in range(3)]
        res.append((Fs, down_weights(m), opt_state(opt)))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    for k in KEYS:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
    for x, y in zip(res[0][2], res[1][2]):
        assert np.array_equal(x, y)


# ---- 6. descent ------------------------------------------------------------------------------------------------------
def test_descent():
    """20 steps at lr 1e-4 on train_down_ref.inputs(117, 17), stage 3.  The CPU fp32 restatement (train_down_ref.run + torch.optim.Adam) goes
    2978.099 2915.314 2850.356 2780.038 2703.060 2619.691 2530.510 2435.844 2336.572 2234.014 2130.886 2030.023 1934.938 1849.476 1777.600
    1721.889 1681.899 1653.160 1629.237 1605.177 1578.645: monotone, relative drop 0.4699.  So the engine's mean F_down must fall at every
    step and end at or below (1 - 0.4699 / 2) = 0.765 of its start."""
    import daimc_amd
    b = TDN.inputs(117, 17)
    m = model_for('g115', fresh=True)
    opt = daimc_amd.Adam(m.model_down, lr=1e-4)
    Fs = [float(c(train(m, opt, b)[0]).mean()) for _ in range(20)]
    Fs.append(float(c(grad(m, b)[0]).mean()))
    print('mean F_down per step:', ' '.join(f'{v:.3f}' for v in Fs))
    assert all(y < x for x, y in zip(Fs, Fs[1:])), Fs
    assert Fs[-1] <= Fs[0] * (1.0 - 0.5 * (1.0 - 1578.645 / 2978.099)), (Fs[0], Fs[-1])


# ---- 7. state interchange and checkpoints ----------------------------------------------------------------------------
def test_state_dict_moves_to_torch_and_back():
    import daimc_amd
    m = model_for('g115', fresh=True)
    opt = daimc_amd.Adam(m.model_down, lr=2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert opt.state_dict()['state'] == {}
    for _ in range(2):
        train(m, opt, batch(3))
    sd = opt.state_dict()
    params = [torch.nn.Parameter(t.clone()) for t in m.model_down.parameters()]
    assert len(params) == NK
    topt = torch.optim.Adam(params, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['lr'] == 2e-4 and tuple(topt.param_groups[0]['betas']) == (0.8, 0.99) and topt.param_groups[0]['eps'] == 1e-7
    for i, p in enumerate(params):
        assert float(topt.state[p]['step']) == 2.0
        assert np.array_equal(topt.state[p]['exp_avg'].numpy(), c(sd['state'][i]['exp_avg']))
    back = daimc_amd.Adam(m.model_down.parameters())
    back.load_state_dict(topt.state_dict())
    assert back.state_dict()['param_groups'][0]['lr'] == 2e-4
    for x, y in zip(opt_state(back), opt_state(opt)):
        assert np.array_equal(x, y)


def test_save_all_load_all_continues_bit_identically(tmp_path):
    import daimc_amd
    import train_mid_ref as TM
    import train_ref as TR
    stats = {'var_beta_s': [], 'var_gamma': [], 'var_beta_o': []}
    b = batch(3)
    s, log_Ppi = TR.batch(117, 5)
    ma = model_for('g115', fresh=True)
    oa = {'top': daimc_amd.Adam(ma.model_top, lr=1e-3), 'mid': daimc_amd.Adam(ma.model_mid, lr=1e-3), 'down': daimc_amd.Adam(ma.model_down, lr=1e-3)}
    for _ in range(2):
        train(ma, oa['down'], b)
    daimc_amd.loss.train_model_top(ma.model_top, s, log_Ppi, oa['top'])
    ma.save_all(str(tmp_path), stats, optimizers=oa)
    mb = model_for('g100', fresh=True)
    _, ob = mb.load_all(str(tmp_path))
    assert sorted(ob) == ['down', 'mid', 'top'] and all(isinstance(v, daimc_amd.Adam) for v in ob.values())
    assert ob['down']._module is mb.model_down and ob['top']._module is mb.model_top and ob['mid']._module is mb.model_mid
    for _ in range(2):
        Fa, Fb = train(ma, oa['down'], b)[0], train(mb, ob['down'], b)[0]
        assert np.array_equal(c(Fa), c(Fb))
    sa, sb = down_weights(ma), down_weights(mb)
    for k in KEYS:
        assert np.array_equal(sa[k], sb[k]), k
    for x, y in zip(opt_state(oa['down']), opt_state(ob['down'])):
        assert np.array_equal(x, y)


# ---- 8. refusals and hygiene -----------------------------------------------------------------------------------------
def raw_train(m, M, *, ctx=None, o1=True, pm=True, pv=True, params=True, nz=True, out=True, ea=True, es=True, hp=(1e-3, 0.9, 0.999, 1e-8, 1),
              omega_mode=None, state=None):
    import daimc_amd
    L = daimc_amd._lib
    e = m._ready()
    n = max(M, 1)
    dev = 'cuda:0'
    t = [torch.zeros(n * 4096, device=dev), torch.zeros(n * 10, device=dev), torch.zeros(n * 10, device=dev)]
    ea_t, es_t = state if state is not None else (torch.zeros(TDN.P, device=dev), torch.zeros(TDN.P, device=dev))
    F = torch.zeros(n, device=dev)
    p = lambda x, use=True: C.c_void_p(x.data_ptr()) if use else None
    fp = L.EfeFeParams(0.5, 1.0, 1.0, L.EFE_OMEGA_SCALAR if omega_mode is None else omega_mode, None, 2.0, 1.0, 25.0, 5.0, 1.5)
    fo = L.EfeFeOut()
    fo.F_down = F.data_ptr()
    noise = L.EfeNoise(7, STAGE, TDN.PASS_FE_DOWN, 0, 0)
    rc = e.lib.efe_train_down(ctx or e.ctx, p(t[0], o1), p(t[1], pm), p(t[2], pv), M, C.byref(fp) if params else None, C.byref(noise) if nz else None, None,
                              C.byref(fo) if out else None, p(ea_t, ea), p(es_t, es), C.byref(L.EfeAdamParams(*hp)) if hp else None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(ctx or e.ctx).decode()


def raw_step(m, *, ctx=None, g=True, ea=True, es=True, hp=(1e-3, 0.9, 0.999, 1e-8, 1), state=None):
    import daimc_amd
    e = m._ready()
    gt = torch.ones(TDN.P, device='cuda:0')
    ea_t, es_t = state if state is not None else (torch.zeros(TDN.P, device='cuda:0'), torch.zeros(TDN.P, device='cuda:0'))
    p = lambda x, use=True: C.c_void_p(x.data_ptr()) if use else None
    rc = e.lib.efe_down_adam_step(ctx or e.ctx, p(gt, g), p(ea_t, ea), p(es_t, es), C.byref(daimc_amd._lib.EfeAdamParams(*hp)) if hp else None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(ctx or e.ctx).decode()


TRAIN_REFUSALS = [dict(M=0), dict(M=-3), dict(M=1, o1=False), dict(M=1, pm=False), dict(M=1, pv=False), dict(M=1, params=False), dict(M=1, nz=False),
                  dict(M=1, out=False), dict(M=1, ea=False), dict(M=1, es=False), dict(M=1, hp=None), dict(M=1, hp=(1e-3, 0.9, 0.999, 1e-8, 0)),
                  dict(M=1, omega_mode=2)]
STEP_REFUSALS = [dict(g=False), dict(ea=False), dict(es=False), dict(hp=None), dict(hp=(1e-3, 0.9, 0.999, 1e-8, 0))]


def test_refusals_change_nothing():
    import daimc_amd
    m = model_for('g115', fresh=True)
    e = m._ready()
    w = family('g115')
    state = (torch.full((TDN.P,), 0.25, device='cuda:0'), torch.full((TDN.P,), 0.5, device='cuda:0'))
    for kw in TRAIN_REFUSALS:
        rc, msg = raw_train(m, state=state, **kw)
        assert rc == 1 and 'efe_train_down' in msg, (kw, rc, msg)
    for kw in STEP_REFUSALS:
        rc, msg = raw_step(m, state=state, **kw)
        assert rc == 1 and 'efe_down_adam_step' in msg, (kw, rc, msg)
    buf = torch.zeros(TDN.P, device='cuda:0')
    assert e.lib.efe_down_get_weights(e.ctx, C.c_void_p(buf.data_ptr()), TDN.P - 1, e.stream()) == 1
    assert 'efe_down_get_weights' in e.lib.efe_last_error(e.ctx).decode()
    assert e.lib.efe_down_get_weights(e.ctx, None, TDN.P, e.stream()) == 1
    assert 'efe_down_get_weights' in e.lib.efe_last_error(e.ctx).decode()
    # the split-operand options
    for opt in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, opt, 1) == 0
        rc, msg = raw_train(m, 1, state=state)
        assert rc == 1 and 'efe_train_down' in msg and 'split' in msg, (opt, rc, msg)
        rc, msg = raw_step(m, state=state)
        assert rc == 1 and 'efe_down_adam_step' in msg and 'split' in msg, (opt, rc, msg)
        assert e.lib.efe_set_option(e.ctx, opt, 0) == 0
    # a stale handle
    ctx = C.c_void_p()
    assert e.lib.efe_create(C.byref(ctx), 0) == 0
    h = int(ctx.value)
    e.lib.efe_destroy(ctx)
    rc, msg = raw_train(m, 1, ctx=ctx, state=state)
    assert rc == 1 and 'efe_train_down' in msg and 'stale' in msg, (rc, msg)
    rc, msg = raw_step(m, ctx=ctx, state=state)
    assert rc == 1 and 'efe_down_adam_step' in msg and 'stale' in msg, (rc, msg)
    assert e.lib.efe_down_get_weights(ctx, C.c_void_p(buf.data_ptr()), TDN.P, e.stream()) == 1
    msg = e.lib.efe_last_error(ctx).decode()
    assert 'efe_down_get_weights' in msg and 'stale' in msg, msg
    assert e.lib.efe_param_count(ctx, b'down') == 0 and e.lib.efe_last_error(ctx).decode() == 'stale or invalid context handle'
    with pytest.raises(RuntimeError):
        e.ops.down_adam_step(h, buf, state[0], state[1], 1e-3, 0.9, 0.999, 1e-8, 1)
    # Python
    z = torch.zeros
    with pytest.raises(NotImplementedError):          # CPU tensors: only the HIP dispatch key is registered
        e.ops.down_adam_step(e.h, z(TDN.P), z(TDN.P), z(TDN.P), 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(NotImplementedError):
        e.ops.train_down(e.h, z(1, 4096), z(1, 10), z(1, 10), 0.5, 1.0, 1.0, 1, None, 2.0, SEED, STAGE, TDN.PASS_FE_DOWN, 0, 0, None, z(TDN.P), z(TDN.P),
                         1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):                 # wrong-length state
        e.ops.down_adam_step(e.h, buf, state[0][:-1], state[1], 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):                 # a gradient of the encoder's length
        e.ops.down_adam_step(e.h, buf[:TDN.P_ENC], state[0], state[1], 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(ValueError):                   # a foreign optimiser: another model's, and this model's habit-net optimiser
        train(m, daimc_amd.Adam(model_for('g100').model_down), batch(1))
    with pytest.raises(ValueError):
        train(m, daimc_amd.Adam(m.model_top), batch(1))
    # nothing moved: the optimiser state, the master copy, the forward paths; and the context still works
    assert bool((state[0] == 0.25).all()) and bool((state[1] == 0.5).all())
    assert e.lib.efe_down_get_weights(e.ctx, C.c_void_p(buf.data_ptr()), TDN.P, e.stream()) == 0
    assert np.array_equal(c(buf), np.concatenate([np.asarray(w['down.' + k], np.float32).reshape(-1) for k in KEYS]))
    down = down_weights(m)
    for k in KEYS:
        assert np.array_equal(down[k], w['down.' + k]), k
    same_bits('decoder after refusals', m.model_down.decoder(batch(3)[1], stage=6), model_for('g115').model_down.decoder(batch(3)[1], stage=6))
    assert raw_train(m, 1)[0] == 0


def test_other_geometry_is_refused():
    import daimc_amd
    m = model_for('g115', (3, 3, 32))
    e = m._ready()
    g = torch.zeros(TDN.P, device='cuda:0')
    hp = daimc_amd._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    p = C.c_void_p(g.data_ptr())
    assert e.lib.efe_down_adam_step(e.ctx, p, p, p, C.byref(hp), e.stream()) == 1
    msg = e.lib.efe_last_error(e.ctx).decode()
    assert 'efe_down_adam_step' in msg and '64' in msg, msg
    rc, msg = raw_train(m, 1)
    assert rc == 1 and 'efe_train_down' in msg and '64' in msg, (rc, msg)
    assert e.lib.efe_down_get_weights(e.ctx, p, TDN.P, e.stream()) == 1
    assert 'efe_down_get_weights' in e.lib.efe_last_error(e.ctx).decode()
    with pytest.raises(ValueError):
        daimc_amd.Adam(m.model_down)
    with pytest.raises(ValueError):
        daimc_amd.Adam(m.model_down.parameters())
    daimc_amd.Adam(m.model_top)                       # the small nets stay trainable there


def test_training_call_allocates_once():
    import daimc_amd
    m = model_for('g115', fresh=True)
    e = m._ready()
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    opt = daimc_amd.Adam(m.model_down, lr=1e-3)
    b = batch(65)
    train(m, opt, b)
    st0 = m.arena_stats()
    train(m, opt, b)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1 == st0
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before
