"""GPU tests (-m gpu) of ModelDown's optimiser step at every admitted geometry (csrc/train_down_g.hip: k_repack_down_g behind k_adam_down;
efe_train_down_g, efe_down_adam_step_g, efe_down_get_weights_g; loss.train_model_down_g, daimc_amd.Adam(model_down, any_geometry=True)).

Engine seed 7, weights 'g115' at the geometry, inputs train_enc_g_ref.inputs(2000 + M, M, C, R); every training call passes the fixed stage
3.  Geometries (pi_dim, C, R), the smallest that reach each branch:
    (3, 3, 32)   last_s1, B = 16, C = 3
    (4, 2, 36)   C = 2: the zero padding of g_enc1p, g_wf and g_enc[0]
    (4, 1, 44)   even extents, K = 64, B = 11: 64 B^2 = 7 744 rows of po_net.9, no multiple of 256
    (3, 3, 84)   K = 1 024
    (4, 1, 64)   the cross-check against the 1 x 64 x 64 step (csrc/train_down.hip), which shares the master copy there

The repack tests compare the trained model with a FRESH model built by the host packers from the downloaded weights, bit for bit, on every
reader of the generic path's packed forms (DESIGN.md section 7g-g lists the forms against these calls):
    encoder / encoder_with_sample    k_conv_e12 (g_enc1p, g_enc[1]), k_conv_e (enc_tiled 1), k_conv_g (g_enc[0..3]; enc_tiled 0), k_head (enc16)
                                     or, head_unfused, k_dense (enc_fc, the first layer's columns NHWC)
    decoder                          k_head (dec16) or k_dense (dec_fc), k_dense on g_fc4 (rows NHWC), k_convt_12 or (ct_fuse12 0) k_conv_g
                                     (g_ct[0..1]), k_dec_bg or (fuse_final_g 0) k_conv_g + k_final_g (g_ct[2], g_wf, g_bf by value)
    calculate_G, free_energy         the same through the rollout's and loss.hip's callers
    grad_down_g                      the master copy itself (train_enc_g.hip, train_dec_head_g.hip, train_dec_g.hip)"""
import ctypes as C

import numpy as np
import pytest
import torch

import train_down_step_g_ref as TSG
import train_enc_g_ref as TEG
from test_train_dec_g_gpu import c, family, model_for
from test_train_down_g_gpu import engine
from train_common import apply_rule

pytestmark = pytest.mark.gpu

STAGE = 3
SEED = 7
G32, G36, G44, G64, G84 = (3, 3, 32), (4, 2, 36), (4, 1, 44), (4, 1, 64), (3, 3, 84)
KEYS = TEG.KEYS
NK = len(KEYS)          # 32


def count(geo):
    return TEG.param_count(geo[1], geo[2])


def batch(geo, M):
    return TEG.inputs(2000 + M, M, geo[1], geo[2])


def adam(m, **kw):
    import daimc_amd
    return daimc_amd.Adam(m.model_down, any_geometry=True, **kw)


def train(m, opt, b, **kw):
    import daimc_amd
    o1, pm, pv, om = b
    return daimc_amd.loss.train_model_down_g(m.model_down, o1, pm, pv, om, opt, stage=STAGE, **kw)


def grad(m, b):
    import daimc_amd
    o1, pm, pv, om = b
    return daimc_amd.loss.grad_down_g(m.model_down, o1, pm, pv, om, stage=STAGE)


def down_weights(m):
    return {k: c(v) for k, v in m.model_down.state_dict().items()}


def model_from(w, geo):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, geo[0], 0.5, 1.0, 1.0, colour_channels=geo[1], resolution=geo[2], device='cuda:0', seed=SEED,
                                       init_weights=False)
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


def master(m, geo):
    """the master copy through the C ABI, without the Python side's own download"""
    e = m._ready()
    P = count(geo)
    buf = torch.empty(P, device='cuda:0')
    assert e.lib.efe_down_get_weights_g(e.ctx, C.c_void_p(buf.data_ptr()), P, e.stream()) == 0, e.lib.efe_last_error(e.ctx).decode()
    return c(buf)


def flat_weights(down):
    return np.concatenate([np.asarray(down[k], np.float32).reshape(-1) for k in KEYS])


# ---- 1. Adam against fp64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geo,M', [(G44, 33), (G32, 3)])
def test_three_steps_vs_fp64(geo, M):
    """three steps of train_model_down_g against torch.optim.Adam on train_enc_g_ref's composed loss in fp32 and fp64; each reference step
    takes the engine's gates of the weights before that step.  All 32 tensors, exp_avg and exp_avg_sq under the project's fp64 rule."""
    lr = 1e-3
    b = batch(geo, M)
    w0 = family('g115', geo)
    m = model_for('g115', geo, fresh=True)
    opt = adam(m, lr=lr)
    r32, r64 = (TSG.AdamRun(w0, geo[1], geo[2], dt, lr, STAGE) for dt in (torch.float32, torch.float64))
    for _ in range(3):
        eng = engine('g115', geo, *b, model=m, gates=True)
        F, _ = train(m, opt, b)
        assert np.array_equal(c(F), eng['F_down'])
        for r in (r32, r64):
            r.step(*b, gates=eng['gates'], dec_gates=eng['dec_gates'])
    sd, osd = m.model_down.state_dict(), opt.state_dict()
    assert int(osd['state'][0]['step']) == 3
    (w32, m32, v32), (w64, m64, v64) = r32.state(), r64.state()
    trip = []
    for i, k in enumerate(KEYS):
        trip += [('exp_avg.' + k, c(osd['state'][i]['exp_avg']), m32[i], m64[i]), ('exp_avg_sq.' + k, c(osd['state'][i]['exp_avg_sq']), v32[i], v64[i]),
                 ('w.' + k, c(sd[k]), w32[i], w64[i])]
        assert not np.array_equal(c(sd[k]), w0['down.' + k]), k
    from test_fp64_parity import fp64_rule
    worst = max((r[4], r[0]) for name, e_, a, b_ in trip for r in fp64_rule(name, e_, a, b_))
    print(f'adam_down_g {geo} M={M}: worst ratio {worst[0]:.2f} ({worst[1]}); mean F_down of the fp32 run per step: ' + ' '.join(f'{v:.3f}' for v in r32.F))
    apply_rule(f'adam_down_g {geo} M={M}', trip)


# ---- 2. composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geo,M', [(G44, 1), (G44, 33), (G44, 65), (G84, 2)])
def test_train_model_down_g_is_grad_then_adam(geo, M):
    b = batch(geo, M)
    ma, mb = model_for('g115', geo, fresh=True), model_for('g115', geo, fresh=True)
    import daimc_amd
    oa, ob = adam(ma, lr=1e-3), daimc_amd.Adam(mb.model_down.parameters(), lr=1e-3, any_geometry=True)
    for _ in range(2):
        Fa, ta = train(ma, oa, b)
        out = grad(mb, b)
        ob.step(out[6])
        assert np.array_equal(c(Fa), c(out[0]))
        same_bits('terms', ta, out[1])
    assert np.array_equal(master(ma, geo), master(mb, geo))
    sa, sb = down_weights(ma), down_weights(mb)
    for k in KEYS:
        assert np.array_equal(sa[k], sb[k]), k
        assert not np.array_equal(sa[k], family('g115', geo)['down.' + k]), k
    assert np.array_equal(master(ma, geo), flat_weights(sa))
    for x, y in zip(opt_state(oa), opt_state(ob)):
        assert np.array_equal(x, y)
    assert oa._step == ob._step == 2


# ---- 3. every packed form follows the step ---------------------------------------------------------------------------
def forward_calls(mod, geo, Ms, cfg_only=False):
    """the readers of the packed forms (the file's head); cfg_only: those an engine option can route differently"""
    import daimc_amd
    out = {}
    for M in Ms:
        o1, pm, pv, om = batch(geo, M)
        out[f'encoder M={M}'] = mod.model_down.encoder(o1, stage=5)
        out[f'encoder_with_sample M={M}'] = mod.model_down.encoder_with_sample(o1, stage=5)
        out[f'decoder M={M}'] = mod.model_down.decoder(pm, stage=6)
    M = Ms[-1] if Ms[-1] <= 4 else 3
    o1, pm, pv, om = batch(geo, M)
    pi0 = np.eye(geo[0], dtype=np.float32)[np.arange(M) % geo[0]]
    out['calculate_G'] = mod.calculate_G(pm, pi0, samples=2, stage=7)
    if cfg_only:
        return out
    out['free_energy'] = tuple(daimc_amd.free_energy(mod, o1, o1, pi0, np.log(np.full((M, geo[0]), 1.0 / geo[0], np.float32)), stage=3))
    out['grad_down_g'] = grad(mod, (o1, pm, pv, om))
    return out


OPTION_READERS = [('head_unfused', 1, 0), ('ct_fuse12', 0, 1), ('enc_tiled', 0, 2), ('enc_tiled', 1, 2), ('enc_tiled', 2, 2), ('fuse_final_g', 0, 1)]


def packed_forms_follow(geo, Ms, train_M):
    w = family('g115', geo)
    m = model_for('g115', geo, fresh=True)
    probe = batch(geo, 2)
    before_po = c(m.model_down.decoder(probe[1], stage=6))
    before_qm = c(m.model_down.encoder(probe[0], stage=5)[0])
    opt = adam(m, lr=1e-3)
    b = batch(geo, train_M)
    for _ in range(2):
        train(m, opt, b)
    down = down_weights(m)
    for k in KEYS:
        assert not np.array_equal(down[k], w['down.' + k]), k
    fresh = model_from(with_down(w, down), geo)
    po, qm = c(m.model_down.decoder(probe[1], stage=6)), c(m.model_down.encoder(probe[0], stage=5)[0])
    assert not np.array_equal(po, before_po) and not np.array_equal(qm, before_qm), 'the two steps must move po1 and qs_mean'

    def check_paths(tag, cfg_only=False):
        got, want = forward_calls(m, geo, Ms, cfg_only), forward_calls(fresh, geo, Ms, cfg_only)
        for name in want:
            same_bits(f'{geo} {tag}: {name}', got[name], want[name])

    check_paths('defaults')
    for name, value, default in OPTION_READERS:
        m.set_option(name, value); fresh.set_option(name, value)
        try:
            check_paths(f'{name}={value}', cfg_only=True)
        finally:
            m.set_option(name, default); fresh.set_option(name, default)


RES = list(range(32, 129, 4))
assert len(RES) == 25


@pytest.mark.parametrize('R', [r for r in RES if r <= 84])
def test_packed_forms_follow_the_step(R):
    packed_forms_follow((4, 1 + RES.index(R) % 3, R), (1, 33), 33)          # (resolution 64 comes with C = 3: the generic path)


@pytest.mark.parametrize('R', [r for r in RES if r > 84])
def test_packed_forms_follow_the_step_large(R):
    packed_forms_follow((4, 1 + RES.index(R) % 3, R), (2,), 2)


@pytest.mark.parametrize('geo', [G32, G84])       # C = 3 at both ends: last_s1, and the Animal-AI size
def test_packed_forms_follow_the_step_named_geometries(geo):
    packed_forms_follow(geo, (1, 33) if geo != G84 else (2,), 33 if geo != G84 else 2)


# ---- 4. the last bias alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fuse_final', [1, 0])
def test_last_bias_alone_reaches_the_decoder(fuse_final):
    geo = G32
    w = family('g115', geo)
    m = model_for('g115', geo, fresh=True)
    m.set_option('fuse_final_g', fuse_final)
    s = batch(geo, 3)[1]
    before = c(m.model_down.decoder(s, stage=6))
    g = torch.zeros(count(geo))
    g[-3:] = torch.tensor([1.0, -1.0, 0.5])
    adam(m, lr=1e-2).step(g)
    after = c(m.model_down.decoder(s, stage=6))
    down = down_weights(m)
    for k in KEYS:
        assert np.array_equal(down[k], w['down.' + k]) == (k != 'po_net.19.bias'), k
    assert np.all(down['po_net.19.bias'] != w['down.po_net.19.bias'])
    assert not np.array_equal(after, before)
    for ch in range(3):
        assert not np.array_equal(after[:, ch], before[:, ch]), ch
    fresh = model_from(with_down(w, down), geo)
    fresh.set_option('fuse_final_g', fuse_final)
    assert np.array_equal(after, c(fresh.model_down.decoder(s, stage=6)))


# ---- 5. re-commit and partial set_weight -----------------------------------------------------------------------------
def test_recommit_and_partial_set_weight_keep_the_trained_tensors():
    """at the C ABI, without the Python side's own download: efe_commit_weights alone, then efe_set_weight of ONE down tensor + commit"""
    geo = G36
    w = family('g115', geo)
    m = model_for('g115', geo, fresh=True)
    e = m._ready()
    opt = adam(m, lr=1e-3)
    train(m, opt, batch(geo, 3))
    down = down_weights(m)
    flat = flat_weights(down)
    assert np.array_equal(master(m, geo), flat) and not np.array_equal(flat, flat_weights({k: w['down.' + k] for k in KEYS}))
    assert e.lib.efe_commit_weights(e.ctx) == 0                     # the host tensors still hold the weights before the step
    assert np.array_equal(master(m, geo), flat)
    new = np.full((20,), 0.125, np.float32)
    shape = (C.c_int64 * 1)(20)
    assert e.lib.efe_set_weight(e.ctx, b'down.qs_net.18.bias', C.c_void_p(new.ctypes.data), shape, 1) == 0
    assert e.lib.efe_commit_weights(e.ctx) == 0
    want = dict(down); want['qs_net.18.bias'] = new
    assert np.array_equal(master(m, geo), flat_weights(want))
    fresh = model_from(with_down(w, want), geo)
    m.model_down._sd = {k: torch.from_numpy(v.copy()) for k, v in want.items()}      # (the Python copy follows; no re-upload: _weights_dirty stays False)
    got, ref = forward_calls(m, geo, (3,), cfg_only=True), forward_calls(fresh, geo, (3,), cfg_only=True)
    for name in ref:
        same_bits('partial set_weight: ' + name, got[name], ref[name])
    # a further step continues from the re-committed master copy, bit for bit with the fresh model's
    of = adam(fresh, lr=1e-3)
    of.load_state_dict(opt.state_dict())
    same_bits('step after re-commit', train(m, opt, batch(geo, 3)), train(fresh, of, batch(geo, 3)))
    assert np.array_equal(master(m, geo), master(fresh, geo))
    # and through load_state_dict: one replaced tensor, 31 trained ones; po_net.19.bias is the tensor handed over by value
    m2 = model_for('g115', geo, fresh=True)
    o2 = adam(m2, lr=1e-3)
    train(m2, o2, batch(geo, 3))
    sd = m2.model_down.state_dict()
    sd['po_net.19.bias'] = torch.tensor([0.5, -0.25])
    m2.model_down.load_state_dict(sd)
    got = down_weights(m2)
    for k in KEYS:
        assert np.array_equal(got[k], c(sd[k])), k
        if k != 'po_net.19.bias':
            assert np.array_equal(got[k], down[k]), k
    s = batch(geo, 3)[1]
    same_bits('load_state_dict', m2.model_down.decoder(s, stage=6), model_from(with_down(w, got), geo).model_down.decoder(s, stage=6))


# ---- 6. the cross-check at 1 x 64 x 64 -------------------------------------------------------------------------------
def test_cross_check_at_1x64x64():
    import daimc_amd
    geo = G64
    P = count(geo)
    assert P == 4787125
    ma, mb = model_for('g115', geo, fresh=True), model_for('g115', geo, fresh=True)
    oa, ob = daimc_amd.Adam(ma.model_down, lr=1e-3), adam(mb, lr=1e-3)
    r = np.random.RandomState(11)
    for _ in range(2):
        g = torch.from_numpy((r.randn(P) * 10.0 ** r.uniform(-8, 0, P)).astype(np.float32))
        oa.step(g); ob.step(g)
    assert np.array_equal(master(ma, geo), master(mb, geo))
    sa, sb = down_weights(ma), down_weights(mb)
    for k in KEYS:
        assert np.array_equal(sa[k], sb[k]) and not np.array_equal(sa[k], family('g115', geo)['down.' + k]), k
    for x, y in zip(opt_state(oa), opt_state(ob)):
        assert np.array_equal(x, y)
    fa, fb = forward_calls(ma, geo, (1, 3)), forward_calls(mb, geo, (1, 3))
    for name in fa:
        same_bits('1x64x64: ' + name, fa[name], fb[name])


def test_the_two_families_share_one_master_copy_at_1x64x64():
    """train_model_down_g then train_model_down on one model, the other order on its twin: each continues from the other's master copy and
    state.  Both end within the fp64 rule of two reference steps (gates of the first model before each of its steps)."""
    import daimc_amd
    geo, M, lr = G64, 3, 1e-3
    b = batch(geo, M)
    w0 = family('g115', geo)
    ma, mb = model_for('g115', geo, fresh=True), model_for('g115', geo, fresh=True)
    oa, ob = adam(ma, lr=lr), adam(mb, lr=lr)
    plain = lambda m, o: daimc_amd.loss.train_model_down(m.model_down, *b, o, stage=STAGE)
    r32, r64 = (TSG.AdamRun(w0, 1, 64, dt, lr, STAGE) for dt in (torch.float32, torch.float64))
    for step in range(2):
        eng = engine('g115', geo, *b, model=ma, gates=True)
        for r in (r32, r64):
            r.step(*b, gates=eng['gates'], dec_gates=eng['dec_gates'])
        if step == 0:
            train(ma, oa, b); plain(mb, ob)
        else:
            plain(ma, oa); train(mb, ob, b)
    assert oa._step == ob._step == 2
    (w32, m32, v32), (w64, m64, v64) = r32.state(), r64.state()
    for tag, m, o in (('g then plain', ma, oa), ('plain then g', mb, ob)):
        sd, osd = m.model_down.state_dict(), o.state_dict()
        trip = []
        for i, k in enumerate(KEYS):
            trip += [('exp_avg.' + k, c(osd['state'][i]['exp_avg']), m32[i], m64[i]), ('exp_avg_sq.' + k, c(osd['state'][i]['exp_avg_sq']), v32[i], v64[i]),
                     ('w.' + k, c(sd[k]), w32[i], w64[i])]
        apply_rule('1x64x64 ' + tag, trip)
        assert np.array_equal(master(m, geo), flat_weights({k: c(v) for k, v in sd.items()}))


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def raw_train(m, geo, M, *, ctx=None, o1=True, pm=True, pv=True, params=True, nz=True, out=True, ea=True, es=True, hp=(1e-3, 0.9, 0.999, 1e-8, 1),
              omega_mode=None, state=None):
    import daimc_amd
    L = daimc_amd._lib
    e = m._ready()
    n, P, dev = max(M, 1), count(geo), 'cuda:0'
    t = [torch.zeros(n * geo[1] * geo[2] * geo[2], device=dev), torch.zeros(n * 10, device=dev), torch.zeros(n * 10, device=dev)]
    ea_t, es_t = state if state is not None else (torch.zeros(P, device=dev), torch.zeros(P, device=dev))
    F = torch.zeros(n, device=dev)
    p = lambda x, use=True: C.c_void_p(x.data_ptr()) if use else None
    fp = L.EfeFeParams(0.5, 1.0, 1.0, L.EFE_OMEGA_SCALAR if omega_mode is None else omega_mode, None, 2.0, 1.0, 25.0, 5.0, 1.5)
    fo = L.EfeFeOut()
    fo.F_down = F.data_ptr()
    noise = L.EfeNoise(7, STAGE, TEG.PASS_FE_DOWN, 0, 0)
    rc = e.lib.efe_train_down_g(ctx or e.ctx, p(t[0], o1), p(t[1], pm), p(t[2], pv), M, C.byref(fp) if params else None, C.byref(noise) if nz else None,
                                None, C.byref(fo) if out else None, p(ea_t, ea), p(es_t, es), C.byref(L.EfeAdamParams(*hp)) if hp else None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(ctx or e.ctx).decode()


def raw_step(m, geo, *, ctx=None, g=True, ea=True, es=True, hp=(1e-3, 0.9, 0.999, 1e-8, 1), state=None):
    import daimc_amd
    e = m._ready()
    P = count(geo)
    gt = torch.ones(P, device='cuda:0')
    ea_t, es_t = state if state is not None else (torch.zeros(P, device='cuda:0'), torch.zeros(P, device='cuda:0'))
    p = lambda x, use=True: C.c_void_p(x.data_ptr()) if use else None
    rc = e.lib.efe_down_adam_step_g(ctx or e.ctx, p(gt, g), p(ea_t, ea), p(es_t, es), C.byref(daimc_amd._lib.EfeAdamParams(*hp)) if hp else None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(ctx or e.ctx).decode()


BAD_HP = [None, (1e-3, 0.9, 0.999, 1e-8, 0), (-1.0, 0.9, 0.999, 1e-8, 1), (1e-3, 1.0, 0.999, 1e-8, 1), (1e-3, 0.9, -0.1, 1e-8, 1), (1e-3, 0.9, 0.999, -1.0, 1),
          (float('nan'), 0.9, 0.999, 1e-8, 1)]
TRAIN_REFUSALS = [dict(M=0), dict(M=-3), dict(M=1, o1=False), dict(M=1, pm=False), dict(M=1, pv=False), dict(M=1, params=False), dict(M=1, nz=False),
                  dict(M=1, out=False), dict(M=1, ea=False), dict(M=1, es=False), dict(M=1, omega_mode=2)] + [dict(M=1, hp=h) for h in BAD_HP]
STEP_REFUSALS = [dict(g=False), dict(ea=False), dict(es=False)] + [dict(hp=h) for h in BAD_HP]


def test_refusals_change_nothing():
    """every refusal is a host-side check before the first launch"""
    import daimc_amd
    geo = G32
    P = count(geo)
    m = model_for('g115', geo, fresh=True)
    e = m._ready()
    w = family('g115', geo)
    s = batch(geo, 3)[1]
    po_before = c(m.model_down.decoder(s, stage=6))
    state = (torch.full((P,), 0.25, device='cuda:0'), torch.full((P,), 0.5, device='cuda:0'))
    for kw in TRAIN_REFUSALS:
        rc, msg = raw_train(m, geo, state=state, **kw)
        assert rc == 1 and 'efe_train_down_g' in msg, (kw, rc, msg)
    for kw in STEP_REFUSALS:
        rc, msg = raw_step(m, geo, state=state, **kw)
        assert rc == 1 and 'efe_down_adam_step_g' in msg, (kw, rc, msg)
    buf = torch.zeros(P, device='cuda:0')
    for dst, n in ((C.c_void_p(buf.data_ptr()), P - 1), (None, P)):
        assert e.lib.efe_down_get_weights_g(e.ctx, dst, n, e.stream()) == 1
        assert 'efe_down_get_weights_g' in e.lib.efe_last_error(e.ctx).decode()
    # the split-operand options: refused outright on a generic context, so no _g call can meet one there ...
    for o in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e.lib.efe_set_option(e.ctx, o, 1) == 1
    # ... and at 1 x 64 x 64, where they can be on, the _g calls refuse while one is
    m64 = model_for('g115', G64, fresh=True)
    e64 = m64._ready()
    for o in (b'mfma_bf16x3', b'mfma_f16x2'):
        assert e64.lib.efe_set_option(e64.ctx, o, 1) == 0
        rc, msg = raw_train(m64, G64, 1)
        assert rc == 1 and 'efe_train_down_g' in msg and 'split' in msg, (o, rc, msg)
        rc, msg = raw_step(m64, G64)
        assert rc == 1 and 'efe_down_adam_step_g' in msg and 'split' in msg, (o, rc, msg)
        assert e64.lib.efe_set_option(e64.ctx, o, 0) == 0
    assert np.array_equal(master(m64, G64), flat_weights({k: family('g115', G64)['down.' + k] for k in KEYS}))
    # an uncommitted context of the same geometry, and a stale handle
    ctx = C.c_void_p()
    assert e.lib.efe_create_cfg(C.byref(ctx), 0, 10, *geo) == 0
    rc, msg = raw_train(m, geo, 1, ctx=ctx, state=state)
    assert rc == 1 and 'efe_train_down_g' in msg and 'not committed' in msg, (rc, msg)
    rc, msg = raw_step(m, geo, ctx=ctx, state=state)
    assert rc == 1 and 'efe_down_adam_step_g' in msg and 'not committed' in msg, (rc, msg)
    assert e.lib.efe_down_get_weights_g(ctx, C.c_void_p(buf.data_ptr()), P, e.stream()) == 1
    assert 'efe_down_get_weights_g' in e.lib.efe_last_error(ctx).decode()
    h = int(ctx.value)
    e.lib.efe_destroy(ctx)
    rc, msg = raw_train(m, geo, 1, ctx=ctx, state=state)
    assert rc == 1 and 'efe_train_down_g' in msg and 'stale' in msg, (rc, msg)
    rc, msg = raw_step(m, geo, ctx=ctx, state=state)
    assert rc == 1 and 'efe_down_adam_step_g' in msg and 'stale' in msg, (rc, msg)
    with pytest.raises(RuntimeError):
        torch.ops.efe_g.down_adam_step(h, buf, state[0], state[1], 1e-3, 0.9, 0.999, 1e-8, 1)
    # the 1 x 64 x 64 family still refuses this geometry
    hp = daimc_amd._lib.EfeAdamParams(1e-3, 0.9, 0.999, 1e-8, 1)
    big = torch.zeros(4787125, device='cuda:0')
    pb = C.c_void_p(big.data_ptr())
    assert e.lib.efe_down_adam_step(e.ctx, pb, pb, pb, C.byref(hp), e.stream()) == 1
    assert 'efe_down_adam_step' in e.lib.efe_last_error(e.ctx).decode() and '64' in e.lib.efe_last_error(e.ctx).decode()
    fp = daimc_amd._lib.EfeFeParams(0.5, 1.0, 1.0, daimc_amd._lib.EFE_OMEGA_SCALAR, None, 2.0, 1.0, 25.0, 5.0, 1.5)
    fo = daimc_amd._lib.EfeFeOut()
    fo.F_down = big.data_ptr()
    nzs = daimc_amd._lib.EfeNoise(7, STAGE, TEG.PASS_FE_DOWN, 0, 0)
    assert e.lib.efe_train_down(e.ctx, pb, pb, pb, 1, C.byref(fp), C.byref(nzs), None, C.byref(fo), pb, pb, C.byref(hp), e.stream()) == 1
    assert 'efe_train_down' in e.lib.efe_last_error(e.ctx).decode() and '64' in e.lib.efe_last_error(e.ctx).decode()
    assert e.lib.efe_down_get_weights(e.ctx, pb, 4787125, e.stream()) == 1
    assert 'efe_down_get_weights' in e.lib.efe_last_error(e.ctx).decode()
    with pytest.raises(ValueError):
        daimc_amd.Adam(m.model_down)
    with pytest.raises(ValueError):
        daimc_amd.Adam(m.model_down.parameters())
    # Python
    with pytest.raises(RuntimeError):                 # wrong-length state, a gradient of the encoder's length
        torch.ops.efe_g.down_adam_step(e.h, buf, state[0][:-1], state[1], 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(RuntimeError):
        torch.ops.efe_g.down_adam_step(e.h, buf[:TEG.enc_param_count(geo[1], geo[2])], state[0], state[1], 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(ValueError):                   # a foreign optimiser: another model's, one without the keyword's step, the habit net's
        train(m, adam(model_for('g115', geo)), batch(geo, 1))
    with pytest.raises(ValueError):
        train(m64, daimc_amd.Adam(m64.model_down), batch(G64, 1))
    with pytest.raises(ValueError):
        train(m, daimc_amd.Adam(m.model_top), batch(geo, 1))
    with pytest.raises(ValueError):
        daimc_amd.Adam(m.model_top, any_geometry=True)
    # nothing moved: the optimiser state, the master copy, the packed forms; and the context still works
    assert bool((state[0] == 0.25).all()) and bool((state[1] == 0.5).all())
    assert np.array_equal(master(m, geo), flat_weights({k: w['down.' + k] for k in KEYS}))
    down = down_weights(m)
    for k in KEYS:
        assert np.array_equal(down[k], w['down.' + k]), k
    assert np.array_equal(c(m.model_down.decoder(s, stage=6)), po_before)
    assert raw_train(m, geo, 1)[0] == 0


# ---- 8. reproducibility ----------------------------------------------------------------------------------------------
def test_reproducible():
    geo = G44
    res = []
    for _ in range(2):
        m = model_for('g115', geo, fresh=True)
        opt = adam(m, lr=1e-3)
        Fs = [c(train(m, opt, batch(geo, 65))[0]) for _ in range(3)]
        res.append((Fs, master(m, geo), opt_state(opt)))
    for x, y in zip(res[0][0], res[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(res[0][1], res[1][1])
    for x, y in zip(res[0][2], res[1][2]):
        assert np.array_equal(x, y)


# ---- 9. hygiene ------------------------------------------------------------------------------------------------------
def test_training_call_allocates_once():
    geo = G44
    m = model_for('g115', geo, fresh=True)
    e = m._ready()
    bytes_before = e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3)
    opt = adam(m, lr=1e-3)
    b = batch(geo, 65)
    train(m, opt, b)
    st0 = m.arena_stats()
    train(m, opt, b)
    st1 = m.arena_stats()
    print('arena', st0, st1)
    assert st1 == st0
    assert e.lib.efe_rollout_scratch_bytes(e.ctx, 8, 2, 3) == bytes_before


# ---- 10. state interchange -------------------------------------------------------------------------------------------
def test_state_dict_moves_to_torch_and_back():
    import daimc_amd
    geo = G44
    m = model_for('g115', geo, fresh=True)
    opt = adam(m, lr=2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert opt.state_dict()['state'] == {}
    for _ in range(2):
        train(m, opt, batch(geo, 3))
    sd = opt.state_dict()
    params = [torch.nn.Parameter(t.clone()) for t in m.model_down.parameters()]
    assert len(params) == NK and sum(p.numel() for p in params) == count(geo)
    topt = torch.optim.Adam(params, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['lr'] == 2e-4 and tuple(topt.param_groups[0]['betas']) == (0.8, 0.99) and topt.param_groups[0]['eps'] == 1e-7
    for i, p in enumerate(params):
        assert float(topt.state[p]['step']) == 2.0
        assert np.array_equal(topt.state[p]['exp_avg'].numpy(), c(sd['state'][i]['exp_avg']))
        assert np.array_equal(topt.state[p]['exp_avg_sq'].numpy(), c(sd['state'][i]['exp_avg_sq']))
    back = daimc_amd.Adam(m.model_down.parameters(), any_geometry=True)
    back.load_state_dict(topt.state_dict())
    assert back.state_dict()['param_groups'][0]['lr'] == 2e-4
    for x, y in zip(opt_state(back), opt_state(opt)):
        assert np.array_equal(x, y)


# ---- 11. descent -----------------------------------------------------------------------------------------------------
def test_descent():
    """20 steps at lr 1e-4 on train_enc_g_ref.inputs(2008, 8, 3, 32), stage 3: the mean F_down of the last step is below the first's.  The CPU
    fp32 restatement (train_down_step_g_ref.AdamRun, its own gates) is printed beside it and is no gate."""
    geo, M, lr = G32, 8, 1e-4
    b = batch(geo, M)
    m = model_for('g115', geo, fresh=True)
    opt = adam(m, lr=lr)
    Fs = [float(c(train(m, opt, b)[0]).mean()) for _ in range(20)]
    ref = TSG.AdamRun(family('g115', geo), geo[1], geo[2], torch.float32, lr, STAGE)
    for _ in range(20):
        ref.step(*b)
    print('mean F_down per step, engine:', ' '.join(f'{v:.3f}' for v in Fs))
    print('mean F_down per step, CPU fp32:', ' '.join(f'{v:.3f}' for v in ref.F))
    assert Fs[-1] < Fs[0], (Fs[0], Fs[-1])
