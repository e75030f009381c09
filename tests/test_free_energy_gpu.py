"""GPU tests (-m gpu) of the training-side free energy (efe_free_energy / efe_loss_*, csrc/loss.hip; daimc_amd.loss):
  * the engine against the reference fixtures (tests/golden/free_energy_*.npz) in injected-noise mode, every returned quantity;
  * against the fp64 restatement on the stress weight families (the fp64 rule of tests/test_fp64_parity.py, restated here);
  * the gamma branches at the fp32 boundaries and the three omega modes;
  * bit equality of every output over chunked calls (row_offset) and over the per-function calls composed in Python;
  * end to end from the device batch producer, the generic geometries, the mfma_f16x2 decoder, bad arguments and stale handles.
Tolerances are those of tests/test_gpu_parity.py: network outputs rtol 1e-5 / atol 2e-6, sigmoid images atol 4e-6, and the 4096-pixel
log-likelihood sums (nlogpo1, F_down) in the form of the term2 sums there, atol = 1e-6 * max(|sum|, 1) + 1e-3."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import free_energy_ref as FR
from conftest import load_golden
from oracle import philox as PX
from oracle import synth
from oracle import efe_oracle as EO

pytestmark = pytest.mark.gpu
FIXTURES = ['free_energy_g100', 'free_energy_g135', 'free_energy_sparse']
NETS = ('Qpi', 'ps1', 'ps1_mean', 'ps1_logvar', 'qs1', 's0', 'qs1_mean', 'qs1_logvar')
SUMS = ('F_down', 'nlogpo1')


def c(t):
    return t.detach().cpu().numpy()


def sumtol(ref):
    return 1e-6 * max(float(np.max(np.abs(ref))), 1.0) + 1e-3


def check_close(name, got, want, sum_tol=sumtol):
    got, want = np.asarray(got).reshape(np.shape(want)), np.asarray(want)
    if name in SUMS:
        np.testing.assert_allclose(got, want, rtol=0, atol=sum_tol(want), err_msg=name)
    elif name == 'po1':
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=4e-6, err_msg=name)
    elif name in NETS:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6, err_msg=name)
    else:           # KL terms, omega, F_top / F_mid: sums of a few exp / log terms of the network outputs
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4, err_msg=name)


def model_for(weights, seed, geo=(4, 1, 64), gamma=0.5):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, geo[0], gamma, 1.0, 1.0, colour_channels=geo[1], resolution=geo[2], device='cuda:0',
                                       seed=seed, init_weights=False)
    m.load_flat_weights(weights)
    return m


def weights_of(meta):
    return synth.stress_weights(meta['family']) if meta['family'] else synth.make_weights(int(meta['wseed']), float(meta['gain']))


def set_gamma(m, gamma):
    m.gamma = torch.tensor(float(np.float32(gamma)), device=m.device)


@pytest.mark.parametrize('name', FIXTURES)
def test_engine_vs_reference_fixture(name):
    import daimc_amd
    g = load_golden(name)
    meta = json.loads(str(g['meta']))
    m = model_for(weights_of(meta), meta['nseed'], gamma=meta['gamma'])
    m.eps_source = PX.normals
    kw = dict(stage=meta['stage'], row_offset=meta['row_offset'])
    fe = daimc_amd.free_energy(m, g['o0'], g['o1'], g['pi0'], g['log_Ppi'], **kw)
    for k in FR.FIELDS:
        check_close(k, c(getattr(fe, k)), g[k])
    for i, gam in enumerate(meta['gammas']):
        set_gamma(m, gam)
        check_close('F_down', c(daimc_amd.free_energy(m, g['o0'], g['o1'], g['pi0'], g['log_Ppi'], **kw).F_down), g['F_down_g'][i])
    set_gamma(m, meta['gamma'])
    sc = daimc_amd.free_energy(m, g['o0'], g['o1'], g['pi0'], g['log_Ppi'], omega=meta['omega_scalar'], **kw)
    check_close('F_mid', c(sc.F_mid), g['F_mid_sc'])
    check_close('F_down', c(sc.F_down), g['F_down_sc'])
    assert np.all(c(sc.omega) == np.float32(meta['omega_scalar']))


# ---- fp64 rule (tests/test_fp64_parity.py, restated): e_eng <= ALPHA e_32 + BETA ulp32(max|Q_64|), relative form for images ----
ALPHA, BETA = 4.0, 8.0


def ulp32(x):
    return float(np.spacing(np.float32(min(abs(float(x)), 3.0e38))))


def fp64_bad(eng, o32, o64, image=False):
    o64 = np.asarray(c(o64), dtype=np.float64)
    eng, o32 = (np.asarray(c(x), dtype=np.float64).reshape(o64.shape) for x in (eng, o32))
    bad = []
    e_eng, e_32 = np.max(np.abs(eng - o64)), np.max(np.abs(o32 - o64))
    if not (e_eng <= ALPHA * e_32 + BETA * ulp32(np.max(np.abs(o64)))):
        bad.append(('abs', e_eng, e_32))
    if image:
        sel = (o64 > 1e-30) & (o64 < 1 - 1e-3)
        if sel.any():
            r_eng, r_32 = np.max(np.abs(eng[sel] - o64[sel]) / o64[sel]), np.max(np.abs(o32[sel] - o64[sel]) / o64[sel])
            if not (r_eng <= ALPHA * r_32 + BETA * 2.0 ** -24):
                bad.append(('rel', r_eng, r_32))
    return bad


@pytest.mark.parametrize('family', ['control'] + list(synth.STRESS_FAMILIES))
def test_engine_vs_fp64_restatement(family):
    import daimc_amd
    w = synth.make_weights(1234, 1.15) if family == 'control' else synth.stress_weights(family)
    M, st, seed = 6, 3, 7
    o0, o1 = synth.make_frames(40, M), synth.make_frames(41, M)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]
    log_Ppi = np.log(np.full((M, 4), 0.25, dtype=np.float32))
    m = model_for(w, seed)
    m.eps_source = PX.normals
    fe = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st)
    with torch.no_grad():
        r32 = FR.free_energy(EO.OracleModel(w, EO.PhiloxNoise(seed)), o0, o1, pi0, log_Ppi, 0.5, stage=st)
        r64 = FR.free_energy(EO.OracleModel(w, EO.PhiloxNoise(seed), dtype=torch.float64), o0, o1, pi0, log_Ppi, 0.5, stage=st)
    bad = {}
    for k in ('F_top', 'omega', 'F_mid', 'kl_s_mid_anal', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'kl_s_anal', 'po1', 'qs1'):
        b = fp64_bad(getattr(fe, k), r32[k], r64[k], image=(k == 'po1'))
        if b:
            bad[k] = b
    assert not bad, (family, bad)


@pytest.mark.parametrize('gamma', [0.0, float(np.float32(0.05)), 0.5, float(np.float32(0.95)), 1.0])
def test_gamma_branches(gamma):
    import daimc_amd
    w = synth.make_weights(1234, 1.0)
    M, st = 5, 2
    o0, o1 = synth.make_frames(50, M), synth.make_frames(51, M)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]
    log_Ppi = np.log(np.full((M, 4), 0.25, dtype=np.float32))
    m = model_for(w, 11, gamma=gamma)
    m.eps_source = PX.normals
    fe = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st)
    with torch.no_grad():
        r = FR.free_energy(EO.OracleModel(w, EO.PhiloxNoise(11)), o0, o1, pi0, log_Ppi, gamma, stage=st)
    check_close('F_down', c(fe.F_down), r['F_down'].numpy())
    # the branch itself: F_down is the restatement's formula for this gamma applied to the engine's OWN terms
    own = FR.loss_down_F(-fe.nlogpo1.cpu(), fe.kl_s.cpu(), fe.kl_naive.cpu(), gamma, 1.0, 1.0, torch.float32)
    np.testing.assert_allclose(c(fe.F_down), own.numpy(), rtol=1e-6, atol=1e-4)


def test_omega_modes():
    import daimc_amd
    w = synth.make_weights(1234, 1.35)
    M, st = 7, 4
    o0, o1 = synth.make_frames(60, M), synth.make_frames(61, M)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]
    log_Ppi = np.log(np.full((M, 4), 0.25, dtype=np.float32))
    m = model_for(w, 5)
    m.eps_source = PX.normals
    derived = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st)
    np.testing.assert_allclose(c(derived.omega), c(daimc_amd.loss.compute_omega(derived.kl_pi, *FR.OMEGA_PARAMS)), rtol=2e-6, atol=0)
    p2 = (2.0, 10.0, 3.0, 0.5)
    d2 = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st, omega_params=p2)
    np.testing.assert_allclose(c(d2.omega), c(daimc_amd.loss.compute_omega(d2.kl_pi, *p2)), rtol=2e-6, atol=0)
    scalar = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st, omega=2.0)
    assert np.all(c(scalar.omega) == 2.0)
    arr = np.linspace(0.5, 3.0, M).astype(np.float32)
    per_row = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st, omega=arr)
    np.testing.assert_array_equal(c(per_row.omega), arr)
    with torch.no_grad():
        orc = EO.OracleModel(w, EO.PhiloxNoise(5))
        for fe, om in ((derived, None), (scalar, 2.0), (per_row, arr)):
            r = FR.free_energy(orc, o0, o1, pi0, log_Ppi, 0.5, omega=om, stage=st)
            for k in ('omega', 'F_top', 'F_mid', 'kl_s_mid_anal', 'F_down', 'kl_s', 'kl_naive'):
                check_close(k, c(getattr(fe, k)), r[k].numpy())
    # the derived values handed back per row give the same bits
    same = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st, omega=derived.omega)
    for k in FR.FIELDS:
        assert torch.equal(getattr(same, k), getattr(derived, k)), k


def test_chunked_and_composed_calls_are_bit_identical():
    import daimc_amd
    from daimc_amd.model import PASS_FE_Q0, PASS_FE_Q1
    N, st = 1000, 9
    m = model_for(synth.make_weights(1234, 1.15), 21, gamma=0.3)
    dev = m.device
    o0 = torch.from_numpy(synth.make_frames(70, N)).to(dev)
    o1 = torch.from_numpy(synth.make_frames(71, N)).to(dev)
    pi0 = torch.eye(4, device=dev)[torch.arange(N, device=dev) % 4]
    log_Ppi = torch.log_softmax(torch.linspace(-1, 1, N * 4, device=dev).reshape(N, 4), dim=1)
    full = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st)
    for f in ('F_top', 'F_mid', 'F_down'):
        assert torch.isfinite(getattr(full, f)).all(), f
    for chunk in (1, 7, 128, 333):
        parts = [daimc_amd.free_energy(m, o0[a:a + chunk], o1[a:a + chunk], pi0[a:a + chunk], log_Ppi[a:a + chunk], stage=st, row_offset=a)
                 for a in range(0, N, chunk)]
        for k in FR.FIELDS:
            got = torch.cat([getattr(p, k) for p in parts], 0)
            assert torch.equal(got, getattr(full, k)), (chunk, k)
    # the reference's functions one by one (same stage, each on its own pass id), omega given per row
    L = daimc_amd.loss
    s0, _, _ = m.model_down.encoder_with_sample(o0, stage=st, pass_=PASS_FE_Q0)
    qm, qv = m.model_down.encoder(o1, stage=st, pass_=PASS_FE_Q1)
    F_top, kl_pi, kl_pi_anal, Qpi = L.compute_loss_top(m.model_top, s0, log_Ppi)
    F_mid, (kl_s_mid, kl_s_mid_anal), ps1, ps1_mean, ps1_logvar = L.compute_loss_mid(m.model_mid, s0, pi0, qm, qv, full.omega, stage=st)
    F_down, (nl, kls, klsa, kln, klna), po1, qs1 = L.compute_loss_down(m.model_down, o1, ps1_mean, ps1_logvar, full.omega, stage=st)
    composed = dict(s0=s0, qs1_mean=qm, qs1_logvar=qv, F_top=F_top, kl_pi=kl_pi, kl_pi_anal=kl_pi_anal, Qpi=Qpi, F_mid=F_mid, kl_s_mid=kl_s_mid,
                    kl_s_mid_anal=kl_s_mid_anal, ps1=ps1, ps1_mean=ps1_mean, ps1_logvar=ps1_logvar, F_down=F_down, nlogpo1=nl, kl_s=kls,
                    kl_s_anal=klsa, kl_naive=kln, kl_naive_anal=klna, po1=po1, qs1=qs1)
    for k, v in composed.items():
        assert torch.equal(v, getattr(full, k)), k
    assert torch.equal(L.compute_kl_div_pi(m, o0, log_Ppi, stage=st), full.kl_pi)


def test_end_to_end_from_device_batches():
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=3)
    games = daimc_amd.Game(16, model=m, seed=4)
    games.randomize_environment_all()
    o0, o1, pi0, log_Ppi = daimc_amd.make_batch_dsprites_active_inference(games, m, deepness=1, samples=1, calc_mean=True, repeats=5)
    assert all(t.is_cuda for t in (o0, o1, pi0, log_Ppi))
    fe = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi)
    for k in FR.FIELDS:
        t = getattr(fe, k)
        assert t.is_cuda and t.shape[0] == 16 and torch.isfinite(t).all(), k
    assert np.isfinite((fe.F_top + fe.F_mid + fe.F_down).mean().item())        # train.py:149's stats["F"]


@pytest.mark.parametrize('geo', [(3, 3, 84), (4, 1, 32)])
def test_generic_geometry_vs_restatement(geo):
    import daimc_amd
    A, Ch, R = geo
    w = synth.make_weights(4321, 1.15, A, Ch, R)
    M, st = 4, 6
    fr0, fr1 = synth.make_frames_rgb(80, M, Ch, R), synth.make_frames_rgb(81, M, Ch, R)
    pi0 = np.eye(A, dtype=np.float32)[np.arange(M) % A]
    log_Ppi = np.log(np.full((M, A), 1.0 / A, dtype=np.float32))
    m = model_for(w, 9, geo)
    m.eps_source = PX.normals
    fe = daimc_amd.free_energy(m, fr0, fr1, pi0, log_Ppi, stage=st)
    with torch.no_grad():
        r = FR.free_energy(EO.OracleModel(w, EO.PhiloxNoise(9), pi_dim=A, channels=Ch, resolution=R), fr0, fr1, pi0, log_Ppi, 0.5, stage=st)
    gsum = lambda ref: 8e-6 * max(float(np.max(np.abs(ref))), 1.0) + 2e-2       # noqa: E731  (tests/test_generic_geometry.py sumtol)
    for k in FR.FIELDS:
        if k == 'po1':
            np.testing.assert_allclose(c(fe.po1), r['po1'].numpy(), rtol=1e-5, atol=1e-5)
        else:
            check_close(k, c(getattr(fe, k)), r[k].numpy(), sum_tol=gsum)


def test_f16x2_decoder_image_feeds_f_down():
    import daimc_amd
    w = synth.make_weights(1234, 1.15)
    M, st = 200, 1
    o0, o1 = synth.make_frames(90, M), synth.make_frames(91, M)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]
    log_Ppi = np.log(np.full((M, 4), 0.25, dtype=np.float32))
    m = model_for(w, 13)
    m.set_option('mfma_f16x2', 1)
    fe = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=st)
    nl = FR.nlogpo1_of(torch.from_numpy(o1), fe.po1.cpu())
    check_close('nlogpo1', c(fe.nlogpo1), nl.numpy())
    F = FR.loss_down_F(-nl, fe.kl_s.cpu(), fe.kl_naive.cpu(), 0.5, 1.0, 1.0, torch.float32)
    check_close('F_down', c(fe.F_down), F.numpy())


def test_bad_arguments_and_stale_handle():
    from daimc_amd import _lib
    m = model_for(synth.make_weights(1234, 1.0), 1)
    e = m._ready()
    lib = e.lib
    M = 3
    dev = m.device
    o = torch.zeros(M, 1, 64, 64, device=dev)
    pi0 = torch.eye(4, device=dev)[:M].contiguous()
    lp = torch.full((M, 4), -1.3862944, device=dev)
    s = torch.zeros(M, 10, device=dev)
    bufs = {f: torch.zeros(M * 4096, device=dev) for f in _lib.FE_OUT_FIELDS}
    out = _lib.EfeFeOut(**{f: b.data_ptr() for f, b in bufs.items()})
    prm = _lib.EfeFeParams(0.5, 1.0, 1.0, _lib.EFE_OMEGA_DERIVED, None, 1.0, 1.0, 25.0, 5.0, 1.5)
    nz = _lib.EfeNoise(1, 0, 0, 0, 0)
    P = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    st = e.stream()

    def call(ctx=e.ctx, **kw):
        a = dict(o0=P(o), M=M, prm=C.byref(prm), out=C.byref(out))
        a.update(kw)
        rc = lib.efe_free_energy(ctx, a['o0'], P(o), P(pi0), P(lp), a['M'], a['prm'], C.byref(nz), None, a['out'], st)
        return rc, lib.efe_last_error(ctx).decode()

    def err(rc, want):
        got = lib.efe_last_error(e.ctx).decode()
        assert rc != 0 and got == want, (rc, got)

    assert call()[0] == 0
    torch.cuda.synchronize()
    rc, msg = call(o0=None)
    assert rc != 0 and msg.startswith('efe_free_energy: bad arguments'), msg
    rc, msg = call(M=0)
    assert rc != 0 and msg.startswith('efe_free_energy: bad arguments'), msg
    err(call(prm=None)[0], 'efe_free_energy: params is NULL')
    missing = _lib.EfeFeOut(**{f: b.data_ptr() for f, b in bufs.items() if f != 'F_mid'})
    err(call(out=C.byref(missing))[0], 'efe_free_energy: out->F_top, out->F_mid and out->F_down are required')
    arr = _lib.EfeFeParams(0.5, 1.0, 1.0, _lib.EFE_OMEGA_ARRAY, None, 1.0, 1.0, 25.0, 5.0, 1.5)
    err(call(prm=C.byref(arr))[0], 'efe_free_energy: omega_mode EFE_OMEGA_ARRAY needs params->omega')
    bad = _lib.EfeFeParams(0.5, 1.0, 1.0, 7, None, 1.0, 1.0, 25.0, 5.0, 1.5)
    err(call(prm=C.byref(bad))[0], 'efe_free_energy: unknown omega_mode 7')
    err(lib.efe_loss_mid(e.ctx, P(s), P(pi0), P(s), P(s), M, C.byref(prm), C.byref(nz), None, C.byref(out), st),
        'efe_loss_mid: omega_mode EFE_OMEGA_DERIVED needs kl_pi (efe_free_energy only)')
    err(lib.efe_loss_down(e.ctx, P(o), P(s), P(s), M, C.byref(prm), C.byref(nz), None, C.byref(out), st),
        'efe_loss_down: omega_mode EFE_OMEGA_DERIVED needs kl_pi (efe_free_energy only)')
    err(lib.efe_loss_top(e.ctx, P(s), P(lp), M, C.byref(_lib.EfeFeOut()), st), 'efe_loss_top: out->F_top is required')
    import daimc_amd
    with pytest.raises(ValueError, match='omega has 2 elements'):
        daimc_amd.free_energy(m, o, o, pi0, lp, omega=np.ones(2, np.float32))
    torch.cuda.synchronize()
    # a stale handle: refused with return code 1 (no use of freed memory), and the torch op raises
    ctx = C.c_void_p()
    assert lib.efe_create(C.byref(ctx), 0) == 0
    lib.efe_destroy(ctx)
    assert call(ctx)[0] == 1
    assert lib.efe_loss_top(ctx, P(s), P(lp), M, C.byref(out), st) == 1
    assert lib.efe_loss_mid(ctx, P(s), P(pi0), P(s), P(s), M, C.byref(prm), C.byref(nz), None, C.byref(out), st) == 1
    assert lib.efe_loss_down(ctx, P(o), P(s), P(s), M, C.byref(prm), C.byref(nz), None, C.byref(out), st) == 1
    assert lib.efe_last_error(ctx).decode() == 'stale or invalid context handle'
    with pytest.raises(RuntimeError, match='stale or invalid engine context handle'):
        e.ops.loss_top(int(ctx.value), s, lp)
