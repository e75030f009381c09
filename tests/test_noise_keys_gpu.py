"""GPU tests (-m gpu): every noise draw site of the engine at the corners of the Philox key space.

A result is a pure function of (seed, stage, pass, sample, global row, element) -- csrc/philox.h -- but each of the hand-written
sites that builds (k0, k1, tag, blk, row, stream, stage) was reached from one corner only: 32-bit seeds (k1 == 0), small stages, rows
and samples.  KEYS lists the other corners: a seed with a high word, with a ZERO low word, above 2^63 (the signed torch-op schema),
negative; a stage with the sign bit, `stage0 + t` that wraps inside a multi-stage call; a launch whose rows straddle 2^31 and 2^32;
everything at once.  The wraps are defined by the engine's uint32 arithmetic (kernels.h global_row / group_key, fused.hip
k_sim_chain's `erow * T + t`), which oracle/philox.py mirrors (tests/test_noise_keys_cpu.py).

EVERY test below runs at EVERY key of KEYS (the whole product fits in seconds), except where a docstring names its own corners: the
free energy (k1, stagewrap, rowwrap, all), the environment (k1, top), the generic geometry (all), the compacted call (rowwrap), the
0x33333332 simulation and the Python stage counter.

Sites -> tests:
  k_trans_fused epilogue (fused.hip:97/176/515)  test_transition_masks[default], test_calculate_G*, test_simulate*
  k_dense (kernels.hip:145)                      test_transition_masks[mid_unfused], test_decoder_masks / test_encoder_masks[head_unfused]
  k_head (fused.hip epilogue helpers)            test_decoder_masks[default], test_encoder_masks[default]
  k_fc4 (decoder.hip:930)                        test_decoder_masks, test_calculate_G*
  k_fc4_b3 (bf16x3.hip:264)                      test_decoder_masks_split_modes
  k_trans_post (kernels.hip:214)                 test_calculate_G* (injected), test_site_normals_rollout_root (device)
  k_root_post (kernels.hip:359)                  test_site_normals_rollout_root
  k_reparam (kernels.hip:469)                    test_device_normals_vs_mirror
  k_sim_chain (fused.hip:355/380/398)            test_simulate*, test_device_uniforms_bit_equal, test_site_normals_simulate
  pass_noise (engine_forward.hip)                test_free_energy
  k_env_* (kernels.hip:486/545/546)              test_environment
  generic launchers (GemmArgs filled separately) test_generic_geometry

Tolerances are the existing ones of tests/test_gpu_parity.py (network outputs rtol 1e-5 / atol 2e-6, images atol 4e-6, terms atol
1e-4, G and term2 `gtol`): a wrong mask bit or normal moves the outputs by O(0.1).  The device's normals differ from the mirror's
only by libm; they are held to the fp64 rule of tests/test_fp64_parity.py (ALPHA 4, BETA 8) against the same Box-Muller evaluated in
float64 from the same Philox words.  Where a test needs a bound on |device normal - mirror normal| (test_site_normals_networks) it is
the rule's own consequence, (ALPHA + 1) e_32 + BETA ulp32(max|n_64|), computed from the mirror alone.

Set EFE_NOISE_KEYS_RECORD=<file> to write the measured device-vs-mirror ratios and the per-site maxima."""
import os

import numpy as np
import pytest
import torch

import free_energy_ref as FR
from conftest import eps_calcG, eps_rollout
from oracle import efe_oracle as EO
from oracle import env_oracle as EV
from oracle import philox as PX
from oracle import synth
from test_fp64_parity import ALPHA, BETA, fp64_rule, ulp32

pytestmark = pytest.mark.gpu

TOP = 0xFEDCBA9876543210
KEYS = {                       # name: (seed, stage, row_offset)
    'base': (7, 5, 0),
    'k1': (7 + (0x9E3779B9 << 32), 5, 0),
    'k0zero': (0xDEADBEEF << 32, 5, 0),
    'top': (TOP, 5, 0),
    'neg': (-1, 5, 0),
    'stage31': (7, 0x80000003, 0),
    'stagewrap': (7, 0xFFFFFFFE, 0),
    'row31': (7, 5, 0x7FFFFFFD),
    'rowwrap': (7, 5, 0xFFFFFFFD),
    'all': (TOP, 0xFFFFFFFE, 0xFFFFFFFD),
}
ALL_KEYS = list(KEYS)
PASS_FE_T = 11                 # csrc/philox.h
RECORD = []                    # (test, key, quantity, value ...) lines of the profile
G2800 = np.array([2800.0])     # |term2_1| of this weight family (tests/test_gpu_parity.py)


def c(t):
    return t.detach().cpu().numpy()


def gtol(t21):
    return 1e-6 * max(float(np.max(np.abs(t21))), 1.0) + 5e-4


def net_close(got, want, msg=''):
    np.testing.assert_allclose(c(got) if torch.is_tensor(got) else got, want.numpy() if torch.is_tensor(want) else want,
                               rtol=1e-5, atol=2e-6, err_msg=msg)


def img_close(got, want, msg=''):
    np.testing.assert_allclose(c(got) if torch.is_tensor(got) else got, want.numpy() if torch.is_tensor(want) else want,
                               rtol=1e-5, atol=4e-6, err_msg=msg)


@pytest.fixture(scope='module', autouse=True)
def record_file():
    yield
    path = os.environ.get('EFE_NOISE_KEYS_RECORD')
    if path and RECORD:
        with open(path, 'w') as f:
            f.write(f'# noise key corners (tests/test_noise_keys_gpu.py).  normals rows: the fp64 rule, ALPHA {ALPHA}, BETA {BETA}; ratio = '
                    'e_eng / (e_32 + BETA / ALPHA * ulp32(max|n_64|)), eng = device normal_elem, 32 = oracle/philox.py normals, 64 = the same '
                    'Box-Muller in float64\n# site rows: max |device-noise result - injected-mirror-noise result| and the bound it was held to\n')
            for line in RECORD:
                f.write(line + '\n')


@pytest.fixture(scope='module')
def weights():
    return synth.make_weights(1234, 1.15)


@pytest.fixture(scope='module')
def model(weights):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=7, init_weights=False)
    m.load_flat_weights(weights)
    return m


_ORC = {}


@pytest.fixture(scope='module')
def setup(model, weights):
    """-> (engine model keyed at the corner, oracle keyed the same way, seed, stage, row_offset)"""
    def at(key):
        seed, stage, ro = KEYS[key]
        model.seed, model.row_offset = seed, ro
        model.eps_source, model.u_source = None, None
        if key not in _ORC:
            _ORC[key] = EO.OracleModel(weights, EO.PhiloxNoise(seed, row_offset=ro))
        return model, _ORC[key], seed, stage, ro
    return at


def option(m, name, value):
    """context manager: an engine option for the length of a block"""
    class _Opt:
        def __enter__(self):
            m.set_option(name, value)

        def __exit__(self, *a):
            m.set_option(name, {'sim_split': 1}.get(name, 0))
    return _Opt()


def key_is_used(key, out, base_fn, model):
    """for the corners that differ from `base` in the seed's high word only: the output must differ from the base output"""
    if key in ('k1', 'k0zero'):
        seed, stage, ro = KEYS['base']
        model.seed, model.row_offset = seed, ro
        base = base_fn(model, seed, stage, ro)
        assert not np.allclose(c(out), c(base), atol=1e-3), f'{key}: the output equals the base seed\'s'


S6 = PX.uniform_fill(31, (6, 10), 400, -1.0, 1.0)
PI6 = np.eye(4, dtype=np.float32)[np.arange(6) % 4]


# ------------------------------------------------------------------------------------------------------------------------------
# masks: exact bits, seen through the network outputs (normals injected from the mirror)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['default', 'mid_unfused'])
@pytest.mark.parametrize('key', ALL_KEYS)
def test_transition_masks(setup, key, variant):
    """k_trans_fused / k_dense, M = 6, at sample 0 and at the last 16-bit sample 0xFFFF"""
    m, orc, seed, stage, ro = setup(key)

    def run(m, seed, stage, ro, sample=0):
        eps = PX.normals(seed, 6, 10, PX.PASS_T1, sample, stage, ro)
        return m.model_mid.transition_with_sample(PI6, S6, stage=stage, pass_=PX.PASS_T1, sample=sample, eps=eps)
    with option(m, 'mid_unfused', int(variant == 'mid_unfused')):
        for sample in (0, 0xFFFF):
            ps1, mean, lv = run(m, seed, stage, ro, sample)
            with torch.no_grad():
                ops1, omean, olv = orc.transition_with_sample(torch.from_numpy(PI6), torch.from_numpy(S6), PX.PASS_T1, sample, stage)
            net_close(mean, omean, f'mean s{sample}'); net_close(lv, olv, f'lv s{sample}'); net_close(ps1, ops1, f'ps1 s{sample}')
        key_is_used(key, run(m, seed, stage, ro)[1], lambda *a: run(*a)[1], m)


@pytest.mark.parametrize('variant', ['default', 'head_unfused'])
@pytest.mark.parametrize('key', ALL_KEYS)
def test_decoder_masks(setup, key, variant):
    """k_head / k_dense + k_fc4 (small launch), M = 6"""
    m, orc, seed, stage, ro = setup(key)

    def run(m, seed, stage, ro):
        return m.model_down.decoder(S6, stage=stage, pass_=PX.PASS_D1, sample=3)
    with option(m, 'head_unfused', int(variant == 'head_unfused')):
        po = run(m, seed, stage, ro)
        with torch.no_grad():
            opo = orc.decoder(torch.from_numpy(S6), PX.PASS_D1, 3, stage)
        img_close(po, opo)
        key_is_used(key, po, run, m)


@pytest.mark.parametrize('mode', ['mfma_bf16x3', 'mfma_f16x2'])
@pytest.mark.parametrize('key', ALL_KEYS)
def test_decoder_masks_split_modes(setup, key, mode):
    """k_fc4_b3 in a launch of more than 128 images (M = 130); the oracle evaluates rows [0:3] and [127:130] through its row offset"""
    m, orc, seed, stage, ro = setup(key)
    s = PX.uniform_fill(32, (130, 10), 401, -1.0, 1.0)
    with option(m, mode, 1):
        po = m.model_down.decoder(s, stage=stage, pass_=PX.PASS_D2A, sample=1).cpu()
    for a, b in ((0, 3), (127, 130)):
        with torch.no_grad():
            opo = orc.decoder(torch.from_numpy(s[a:b]), PX.PASS_D2A, 1, stage, ro + a)
        img_close(po[a:b], opo, f'rows {a}:{b}')


@pytest.mark.parametrize('variant', ['default', 'head_unfused'])
@pytest.mark.parametrize('key', ALL_KEYS)
def test_encoder_masks(setup, key, variant):
    """encoder dense head (k_head / k_dense), M = 6"""
    m, orc, seed, stage, ro = setup(key)
    fr = synth.make_frames(33, 6)

    def run(m, seed, stage, ro):
        eps = PX.normals(seed, 6, 10, PX.PASS_E1, 2, stage, ro)
        return m.model_down.encoder_with_sample(fr, stage=stage, pass_=PX.PASS_E1, sample=2, eps=eps)
    with option(m, 'head_unfused', int(variant == 'head_unfused')):
        s, mean, lv = run(m, seed, stage, ro)
        with torch.no_grad():
            os_, omean, olv = orc.encoder_with_sample(torch.from_numpy(fr), PX.PASS_E1, 2, stage)
        net_close(mean, omean, 'mean'); net_close(lv, olv, 'lv'); net_close(s, os_, 's')
        key_is_used(key, mean, lambda *a: run(*a)[1], m)


# ------------------------------------------------------------------------------------------------------------------------------
# EFE entry points: group_key / global_row
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ALL_KEYS)
def test_calculate_G(setup, key):
    m, orc, seed, stage, ro = setup(key)
    M, S = 5, 2
    s0 = PX.uniform_fill(8, (M, 10), 305, -1.0, 1.0)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]

    def run(m, seed, stage, ro):
        return m.calculate_G(s0, pi0, samples=S, stage=stage, eps=eps_calcG(seed, M, S, stage, ro))
    G, terms, ps1, ps1m, po1 = run(m, seed, stage, ro)
    with torch.no_grad():
        oG, oT, ops1, ops1m, opo1 = orc.calculate_G(torch.from_numpy(s0), torch.from_numpy(pi0), S, stage)
    net_close(ps1, ops1, 'ps1'); net_close(ps1m, ops1m, 'ps1_mean')
    np.testing.assert_allclose(c(po1), opo1.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(c(terms[0]), oT[0].numpy(), atol=1e-4)
    np.testing.assert_allclose(c(terms[1]), oT[1].numpy(), atol=1e-4)
    np.testing.assert_allclose(c(G), oG.numpy(), atol=gtol(orc.last_term2_parts[0].numpy()))
    key_is_used(key, G, lambda *a: run(*a)[0], m)


@pytest.mark.parametrize('key', ALL_KEYS)
def test_calculate_G_mean(setup, key):
    m, orc, seed, stage, ro = setup(key)
    s0 = PX.uniform_fill(8, (4, 10), 306, -1.0, 1.0)
    G, terms, ps1m, po1 = m.calculate_G_mean(s0, m.pi_one_hot, stage=stage, eps=eps_calcG(seed, 4, 1, stage, ro))
    with torch.no_grad():
        oG, oT, ops1m, opo1 = orc.calculate_G_mean(torch.from_numpy(s0), torch.eye(4), stage)
    net_close(ps1m, ops1m, 'ps1_mean')
    np.testing.assert_allclose(c(terms[0]), oT[0].numpy(), atol=1e-4)
    np.testing.assert_allclose(c(terms[1]), oT[1].numpy(), atol=1e-4)
    np.testing.assert_allclose(c(G), oG.numpy(), atol=gtol(orc.last_term2_parts[0].numpy()))


@pytest.mark.parametrize('key', ALL_KEYS)
def test_calculate_G_given_trajectory(setup, key):
    m, orc, seed, stage, ro = setup(key)
    T = 3
    s0, ps1, mean = (PX.uniform_fill(8, (T, 10), 307 + i, -1.0, 1.0) for i in range(3))
    lv = PX.uniform_fill(8, (T, 10), 310, -3.0, -1.0)
    pi0 = np.eye(4, dtype=np.float32)[[2, 0, 3]]
    G = m.calculate_G_given_trajectory(s0, ps1, mean, lv, pi0, stage=stage, eps=eps_calcG(seed, T, 1, stage, ro))
    with torch.no_grad():
        oG = orc.calculate_G_given_trajectory(*(torch.from_numpy(x) for x in (s0, ps1, mean, lv, pi0)), stage)
    np.testing.assert_allclose(c(G), oG.numpy(), atol=gtol(G2800))


@pytest.mark.parametrize('key', ALL_KEYS)
def test_calculate_G_repeated(setup, key):
    """M = 4, steps = 3, S = 2: at stagewrap / all the three stages are 0xFFFFFFFE, 0xFFFFFFFF, 0"""
    m, orc, seed, stage, ro = setup(key)
    M, D, S = 4, 3, 2
    o = synth.make_frames(34, M)
    pi = np.eye(4, dtype=np.float32)
    sum_G, terms, po1 = m.calculate_G_repeated(o, pi, steps=D, samples=S, stage=stage, eps=eps_rollout(seed, M, D, S, stage, ro))
    with torch.no_grad():
        oG, oT, opo1 = orc.calculate_G_repeated(torch.from_numpy(o), torch.from_numpy(pi), D, False, S, stage)
    np.testing.assert_allclose(c(terms[0]), oT[0].numpy(), atol=1e-4)
    np.testing.assert_allclose(c(terms[1]), oT[1].numpy(), atol=1e-4)
    np.testing.assert_allclose(c(sum_G), oG.numpy(), atol=gtol(orc.last_term2_parts[0].numpy()))


def test_compacted_call_across_the_row_wrap(setup):
    """Rows(ids=[0, 2], rows_per_entry=4) at rowwrap: entry 0 holds rows 0xFFFFFFFD .. 0, entry 2 rows 5 .. 8 -- bit-equal to the rows of
    the full call (device noise)"""
    from daimc_amd.model import Rows
    m, orc, seed, stage, ro = setup('rowwrap')
    s0 = torch.from_numpy(PX.uniform_fill(2, (12, 10), 77, -1, 1)).to(m.device)
    pi0 = m.pi_one_hot.repeat(3, 1)
    ref = m.calculate_G(s0, pi0, samples=2, stage=stage)
    kr = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11], device=m.device)
    rc = Rows(ids=torch.tensor([0, 2], dtype=torch.int32, device=m.device), rows_per_entry=4, ids_host=[0, 2])
    cmp_ = m.calculate_G(s0[kr], pi0[kr], samples=2, stage=stage, rows=rc)
    assert torch.equal(cmp_[0], ref[0][kr]) and torch.equal(cmp_[2], ref[2][kr]) and torch.equal(cmp_[4], ref[4][kr])
    for k in range(3):
        assert torch.equal(cmp_[1][k], ref[1][k][kr])


# ------------------------------------------------------------------------------------------------------------------------------
# efe_simulate (k_sim_chain)
# ------------------------------------------------------------------------------------------------------------------------------
def _simulate_vs_oracle(m, orc, starts, T, stage, ro, episodes):
    m.eps_source, m.u_source = PX.normals, PX.uniforms
    G, pi0, q0 = m.simulate_batch(starts, T, use_means=False, stage=stage)
    m.eps_source, m.u_source = None, None
    for e in episodes:
        with torch.no_grad():
            oG, opi0, oq = orc.mcts_step_simulate(torch.from_numpy(starts[e]), T, False, stage, episode=ro + e)
        assert np.array_equal(c(pi0[e]), opi0.numpy()), f'episode {e}: actions'
        np.testing.assert_allclose(c(q0[e]), oq.numpy(), rtol=1e-5, atol=1e-6)
        assert abs(float(G[e]) - oG) < gtol(G2800), f'episode {e}: G'
    return G


@pytest.mark.parametrize('split', [1, 0])
@pytest.mark.parametrize('key', ALL_KEYS)
def test_simulate_small(setup, key, split):
    """E = 3, depth = 5: the split chain (sim_split 1) and the one-workgroup chain (0), every episode against the oracle"""
    m, orc, seed, stage, ro = setup(key)
    starts = PX.uniform_fill(8, (3, 10), 910, -1, 1)
    with option(m, 'sim_split', split):
        _simulate_vs_oracle(m, orc, starts, 5, stage, ro, range(3))


@pytest.mark.parametrize('key', ALL_KEYS)
def test_simulate_unsplit_17(setup, key):
    """E = 17 (more than 16 episodes: the un-split path, three blocks of 8): one episode of each block against the oracle"""
    m, orc, seed, stage, ro = setup(key)
    starts = PX.uniform_fill(8, (17, 10), 911, -1, 1)
    _simulate_vs_oracle(m, orc, starts, 5, stage, ro, (0, 8, 16))


@pytest.mark.parametrize('key', ['base', 'all'])
def test_simulate_trajectory_rows_cross_2_32(setup, key):
    """row_offset 0x33333332, depth 5: the trajectory rows (row_offset + e) * 5 + t are 0xFFFFFFFA .. 0xFFFFFFFE, 0xFFFFFFFF .. 3, 4 .. 8"""
    m, orc, seed, stage, _ = setup(key)
    ro = 0x33333332
    m.row_offset = ro
    starts = PX.uniform_fill(8, (3, 10), 912, -1, 1)
    _simulate_vs_oracle(m, orc, starts, 5, stage, ro, range(3))


# ------------------------------------------------------------------------------------------------------------------------------
# device-generated draws against the mirror: nothing injected
# ------------------------------------------------------------------------------------------------------------------------------
def normals64(seed, rows, n, pas, sample, stage, ro):
    """PX.normals with the Box-Muller evaluated in float64 from the same Philox words (and the same fp32 uniforms)"""
    k0, k1 = PX._key(seed)
    nblk = (n + 3) // 4
    blk = np.arange(nblk, dtype=np.uint64)[None, :]
    row = ((np.arange(rows, dtype=np.uint64) + np.uint64(ro & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))[:, None]
    x = PX.philox4x32_10(blk | (np.uint64(PX.TAG_EPS) << np.uint64(16)), row, np.uint64(PX.stream_id(pas, sample)),
                         np.uint64(stage & 0xFFFFFFFF), k0, k1)
    out = np.empty((rows, nblk, 4), dtype=np.float64)
    for lane, (a, b) in enumerate(((x[0], x[1]), (x[2], x[3]))):
        u1, u2 = PX._u01(a).astype(np.float64), PX._u01(b).astype(np.float64)
        r, th = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        out[..., 2 * lane], out[..., 2 * lane + 1] = r * np.cos(th), r * np.sin(th)
    return out.reshape(rows, nblk * 4)[:, :n]


def normal_margin(seed, rows, n, pas, sample, stage, ro):
    """bound on |device normal - mirror normal| that the fp64 rule implies: e_eng + e_32 <= (ALPHA + 1) e_32 + BETA ulp32(max|n_64|)"""
    n32, n64 = PX.normals(seed, rows, n, pas, sample, stage, ro), normals64(seed, rows, n, pas, sample, stage, ro)
    return (ALPHA + 1) * float(np.max(np.abs(n32 - n64))) + BETA * ulp32(np.max(np.abs(n64)))


@pytest.mark.parametrize('key', ALL_KEYS)
def test_device_normals_vs_mirror(setup, key):
    """k_reparam with mean = logvar = 0 returns normal_elem itself: M = 8, n = 10 and 13 (a partial last Box-Muller block), three passes,
    samples 0 and 9"""
    m, orc, seed, stage, ro = setup(key)
    bad = []
    for n in (10, 13):
        z = np.zeros((8, n), dtype=np.float32)
        for pas in (PX.PASS_ROOT, PX.PASS_SIM, PASS_FE_T):
            for sample in (0, 9):
                dev = c(m._reparameterize(z, z, pass_=pas, sample=sample, stage=stage, row_offset=ro))
                n32 = PX.normals(seed, 8, n, pas, sample, stage, ro)
                n64 = normals64(seed, 8, n, pas, sample, stage, ro)
                for name, e, e3, b, q, ok in fp64_rule(f'n{n}/p{pas}/s{sample}', dev, n32, n64):
                    RECORD.append(f'normals  {key:<10} {name:<12} e_eng {e:10.3e} e_32 {e3:10.3e} bound {b:10.3e} ratio {q:7.3f}{"" if ok else "  FAIL"}')
                    if not ok:
                        bad.append((name, e, e3, b))
    assert not bad, bad


@pytest.mark.parametrize('key', ALL_KEYS)
def test_device_uniforms_bit_equal(setup, key):
    """u01 has no libm: simulate_batch with the normals injected and the uniforms LEFT TO THE DEVICE == the same call with
    PX.uniforms injected, bit for bit"""
    m, orc, seed, stage, ro = setup(key)
    starts = PX.uniform_fill(8, (3, 10), 913, -1, 1)
    m.eps_source = PX.normals
    dev = m.simulate_batch(starts, 4, use_means=False, stage=stage)
    m.u_source = PX.uniforms
    inj = m.simulate_batch(starts, 4, use_means=False, stage=stage)
    m.eps_source, m.u_source = None, None
    for a, b, name in zip(dev, inj, ('G', 'pi0', 'Qpi0')):
        assert torch.equal(a, b), name


@pytest.mark.parametrize('key', ALL_KEYS)
def test_site_normals_networks(setup, key):
    """transition_with_sample / encoder_with_sample with device normals: the sample is mean + eps exp(lv / 2) of the RETURNED mean and
    logvar with the mirror's eps, within the normals' margin times exp(lv / 2) (plus the network tolerance for the fp32 evaluation)"""
    m, orc, seed, stage, ro = setup(key)
    fr = synth.make_frames(33, 6)
    for site, pas, call in (('transition', PX.PASS_T2, lambda: m.model_mid.transition_with_sample(PI6, S6, stage=stage, pass_=PX.PASS_T2, sample=4)),
                            ('encoder', PX.PASS_E1, lambda: m.model_down.encoder_with_sample(fr, stage=stage, pass_=PX.PASS_E1, sample=4))):
        s, mean, lv = (c(t).astype(np.float64) for t in call())
        want = mean + PX.normals(seed, 6, 10, pas, 4, stage, ro).astype(np.float64) * np.exp(lv * 0.5)
        bound = normal_margin(seed, 6, 10, pas, 4, stage, ro) * np.exp(lv * 0.5) + 1e-5 * np.abs(want) + 2e-6
        err = np.abs(s - want)
        RECORD.append(f'site     {key:<10} {site:<12} max|s - (mean + eps_mirror exp(lv/2))| {err.max():10.3e}  smallest bound {bound.min():10.3e}  '
                      f'max err/bound {np.max(err / bound):6.3f}')
        assert (err <= bound).all(), (site, float(err.max()), float(np.max(err / bound)))


@pytest.mark.parametrize('key', ALL_KEYS)
def test_site_normals_rollout_root(setup, key):
    """calculate_G_repeated with device noise (k_root_post's PASS_ROOT draw, k_trans_post's T1 / T2 / D2B draws) against the same call
    with the mirror's normals: the bound test_device_noise_mode_vs_oracle uses for G"""
    m, orc, seed, stage, ro = setup(key)
    o = synth.make_frames(35, 4)
    pi = np.eye(4, dtype=np.float32)
    for steps in (1, 2):          # the root draw alone, then with a second stage (k_trans_post's `stage0 + t`); the bound is per stage
        dev = m.calculate_G_repeated(o, pi, steps=steps, samples=2, stage=stage)
        m.eps_source = PX.normals
        try:
            inj = m.calculate_G_repeated(o, pi, steps=steps, samples=2, stage=stage)
        finally:
            m.eps_source = None
        err, bound = float(np.max(np.abs(c(dev[0]) - c(inj[0])))), steps * (gtol(G2800) + 4e-3)
        RECORD.append(f'site     {key:<10} {"rollout_d" + str(steps):<12} max|sum_G device - sum_G mirror| {err:10.3e}  bound {bound:10.3e}')
        assert err <= bound, (steps, err)


@pytest.mark.parametrize('key', ALL_KEYS)
def test_site_normals_simulate(setup, key):
    """simulate_batch with device noise (k_sim_chain's PASS_SIM normals and TAG_ACT uniforms) against the same call with the mirror's"""
    m, orc, seed, stage, ro = setup(key)
    starts = PX.uniform_fill(8, (3, 10), 914, -1, 1)
    dev = m.simulate_batch(starts, 4, use_means=False, stage=stage)
    m.eps_source, m.u_source = PX.normals, PX.uniforms
    inj = m.simulate_batch(starts, 4, use_means=False, stage=stage)
    m.eps_source, m.u_source = None, None
    assert torch.equal(dev[1], inj[1])                     # the same actions
    np.testing.assert_allclose(c(dev[2]), c(inj[2]), rtol=1e-5, atol=1e-6)
    err = float(np.max(np.abs(c(dev[0]) - c(inj[0]))))
    RECORD.append(f'site     {key:<10} {"simulate":<12} max|G device - G mirror| {err:10.3e}  bound {gtol(G2800) + 4e-3:10.3e}')
    assert err <= gtol(G2800) + 4e-3


# ------------------------------------------------------------------------------------------------------------------------------
# free energy, environment, generic geometry, Python bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['k1', 'stagewrap', 'rowwrap', 'all'])
def test_free_energy(setup, weights, key):
    """daimc_amd.free_energy (pass_noise: four passes), M = 3, against tests/free_energy_ref.py on the oracle keyed the same way, under
    the fp64 rule that tests/test_free_energy_gpu.py applies to its stress rows"""
    import daimc_amd
    m, orc, seed, stage, ro = setup(key)
    M = 3
    o0, o1 = synth.make_frames(40, M), synth.make_frames(41, M)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]
    log_Ppi = np.log(np.full((M, 4), 0.25, dtype=np.float32))
    gamma0 = m.gamma
    m.gamma = torch.tensor(0.5, device=m.device)
    m.eps_source = PX.normals
    try:
        fe = daimc_amd.free_energy(m, o0, o1, pi0, log_Ppi, stage=stage)
    finally:
        m.gamma, m.eps_source = gamma0, None
    orc64 = EO.OracleModel(weights, EO.PhiloxNoise(seed, row_offset=ro), dtype=torch.float64)
    with torch.no_grad():
        r32 = FR.free_energy(orc, o0, o1, pi0, log_Ppi, 0.5, stage=stage, ro=ro)
        r64 = FR.free_energy(orc64, o0, o1, pi0, log_Ppi, 0.5, stage=stage, ro=ro)
    bad = []
    for k in ('F_top', 'omega', 'F_mid', 'kl_s_mid_anal', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'kl_s_anal', 'po1', 'qs1'):
        got = c(getattr(fe, k)).reshape(tuple(r64[k].shape))
        bad += [r for r in fp64_rule(k, got, r32[k], r64[k], image=(k == 'po1')) if not r[-1]]
    assert not bad, bad


@pytest.mark.parametrize('seedname', ['k1', 'top'])
def test_environment(seedname):
    """k_env_* (TAG_ENV): 4 games at game_offset 0xFFFFFFFE (games 0xFFFFFFFE, 0xFFFFFFFF, 0, 1), reset at a stage with the sign bit,
    one step at stage 0xFFFFFFFF in which games 0 and 2 finish a round and draw new latents -- equal states, exact"""
    import daimc_amd
    seed, go = KEYS[seedname][0], 0xFFFFFFFE
    games = daimc_amd.Game(4, device='cuda:0', seed=seed, game_offset=go, init_stage=0x80000002)
    s = EV.new_image_all(seed, np.zeros((4, 7), np.float32), 0x80000002, go)
    assert np.array_equal(c(games.current_s), s)
    games.randomize_environment_all(stage=0x80000003)
    s, r = EV.reset(seed, 4, 0x80000003, go)
    assert np.array_equal(c(games.current_s), s) and np.array_equal(c(games.last_r), r)
    assert not np.array_equal(s[:2], EV.reset(seed, 2, 0x80000003, 0)[0]) and np.array_equal(s[2:], EV.reset(seed, 2, 0x80000003, 0)[0])
    s[[0, 2], 5] = 31.0
    games.current_s.copy_(torch.from_numpy(s))
    actions = [0, 1, 0, 2]
    changed = games.pi_to_action_all(actions, repeats=2, stage=0xFFFFFFFF)
    och = EV.step(seed, s, r, actions, 2, 0xFFFFFFFF, go)
    assert np.array_equal(c(changed), och) and list(och) == [True, False, True, False]
    assert np.array_equal(c(games.current_s), s) and np.array_equal(c(games.last_r), r)


def test_generic_geometry():
    """the smallest generic geometry (pi 3, 1 x 32 x 32) at `all`: decoder, encoder and calculate_G (M = 3, S = 2) -- the generic launchers
    fill GemmArgs / HeadArgs on their own.  Tolerances of tests/test_generic_geometry.py"""
    import daimc_amd
    A, C, R = 3, 1, 32
    seed, stage, ro = KEYS['all']
    w = synth.make_weights(1234, 1.15, A, C, R)
    m = daimc_amd.ActiveInferenceModel(10, A, 0.0, 1.0, 1.0, colour_channels=C, resolution=R, device='cuda:0', seed=seed, row_offset=ro,
                                       init_weights=False)
    m.load_flat_weights(w)
    orc = EO.OracleModel(w, EO.PhiloxNoise(seed, row_offset=ro), pi_dim=A, channels=C, resolution=R)
    M, S = 3, 2
    s0 = PX.uniform_fill(4, (M, 10), 63, -1.0, 1.0)
    pi0 = np.eye(A, dtype=np.float32)
    fr = synth.make_frames_rgb(11, M, C, R)
    with torch.no_grad():
        opo = orc.decoder(torch.from_numpy(s0), PX.PASS_D1, 1, stage)
        oes, oem, oelv = orc.encoder_with_sample(torch.from_numpy(fr), PX.PASS_E1, 1, stage)
        oG, oT, ops1, _, opo1 = orc.calculate_G(torch.from_numpy(s0), torch.from_numpy(pi0), S, stage)
    np.testing.assert_allclose(c(m.model_down.decoder(s0, stage=stage, pass_=PX.PASS_D1, sample=1)), opo.numpy(), rtol=1e-5, atol=1e-5)
    es, em, elv = m.model_down.encoder_with_sample(fr, stage=stage, pass_=PX.PASS_E1, sample=1, eps=PX.normals(seed, M, 10, PX.PASS_E1, 1, stage, ro))
    np.testing.assert_allclose(c(em), oem.numpy(), rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(c(elv), oelv.numpy(), rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(c(es), oes.numpy(), rtol=1e-5, atol=5e-6)
    G, T, ps1, _, po1 = m.calculate_G(s0, pi0, samples=S, stage=stage, eps=eps_calcG(seed, M, S, stage, ro))
    sumtol = 8e-6 * max(float(np.max(np.abs(oT[0].numpy()))), 1.0) + 2e-2
    np.testing.assert_allclose(c(ps1), ops1.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(c(po1), opo1.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(c(T[0]), oT[0].numpy(), atol=sumtol)
    np.testing.assert_allclose(c(T[1]), oT[1].numpy(), atol=1e-3)
    np.testing.assert_allclose(c(G), oG.numpy(), atol=3 * sumtol)


def test_python_stage_counter_wraps(setup):
    """model._stage counts calls without bound: at 0xFFFFFFFF two calculate_G(stage=None) calls are stage 0xFFFFFFFF and stage 0"""
    m, orc, seed, stage, ro = setup('k1')
    s0 = PX.uniform_fill(8, (4, 10), 306, -1.0, 1.0)
    m._stage = 0xFFFFFFFF
    a = m.calculate_G(s0, m.pi_one_hot, samples=2)
    b = m.calculate_G(s0, m.pi_one_hot, samples=2)
    assert m._stage == 0xFFFFFFFF + 2
    ea = m.calculate_G(s0, m.pi_one_hot, samples=2, stage=0xFFFFFFFF)
    eb = m.calculate_G(s0, m.pi_one_hot, samples=2, stage=0)
    for x, y in ((a, ea), (b, eb)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2]) and torch.equal(x[4], y[4])
    assert not torch.equal(a[0], b[0])
