"""GPU tests (-m gpu): the generic-geometry kernels (generic.hip, generic_dec.hip, generic_enc.hip) at EVERY resolution efe_create_cfg
admits -- 32 .. 128 in steps of 4, 25 of them -- where tests/test_generic_geometry.py and tests/test_fp64_parity.py run six.  The resolution
decides the strip shapes of k_convt_12 (Win = R / 4, TH = 64 / Win rows per strip, the short last strip), of k_dec_bg (Win = R / 2,
TH = 128 / Win, tiles that span two rows, the ring sizes) and of k_conv_e12 (TY, the strip count, the last strip), the multiply-high
divisors, the encoder head's contraction length and the scratch plans.

  1. decoder and encoder against the fp64 oracle, every resolution x 1..3 channels              (test_networks_vs_fp64)
  2. calculate_G against the fp64 oracle, every resolution, pi_dim 2..6                          (test_calculate_G_vs_fp64)
  3. ... and in the same call the launch counts per kernel class: the fused kernels ran, not the per-layer forms (EXPECTED_PATH)
  4. fused kernels against separate launches and against small launch groups, every resolution   (test_fused_equals_separate)
  5. the scratch plan is exact at every resolution                                               (test_reserve_no_growth)

1 and 2 use the comparison rule of tests/test_fp64_parity.py unchanged (fp64_rule / check, ALPHA = 4, BETA = 8: the engine's error
against fp64 is bounded by the fp32 oracle's own error on the same inputs plus a floor in ulps).  With EFE_FP64_RECORD=<file> set their
rows are written in that module's format (profiles/generic_sweep_fp64.txt is the first MI355X run).  Every case creates its own model
and drops it when it ends: at base 32 the decoder's Linear(256, 64 base^2) alone is 64 MB."""
import gc
import os

import numpy as np
import pytest
import torch

from conftest import eps_calcG
from oracle import philox as PX
from oracle import synth
from oracle import efe_oracle as EO
import test_fp64_parity as FP
from test_fp64_parity import check, _calcG_quantities, _orc_G
from test_generic_geometry import sumtol, c

pytestmark = pytest.mark.gpu

RESOLUTIONS = list(range(32, 129, 4))
SEED = 7          # noise seed
WSEED = 2468      # weight seed (+ resolution)


def channels_of(R):
    return 1 + (R // 4) % 3


def pi_dim_of(R):
    return 2 + (R // 4) % 5


@pytest.fixture(scope='module', autouse=True)
def record_file():
    """the rows this module added to test_fp64_parity's record, in its format (appended when that module wrote the file in this session)"""
    n0 = len(FP.RECORD)
    yield
    path = os.environ.get('EFE_FP64_RECORD')
    rows = FP.RECORD[n0:]
    if path and rows:
        with open(path, 'a' if n0 else 'w') as f:
            f.write(f'# fp64 parity record, generic-geometry sweep: ALPHA {FP.ALPHA}, BETA {FP.BETA}; ratio = e_eng / (e_32 + BETA / ALPHA * floor),'
                    ' floor = ulp32(max|Q_64|) (absolute rows) or 2^-24 (.rel rows)\n')
            f.write(f'# {"resolution, channels, pi_dim / call":<44} {"quantity":<12} {"e_eng":>10} {"e_32":>10} {"bound":>10} {"ratio":>7}\n')
            for tag, name, e, e3, b, q, ok in rows:
                f.write(f'{tag:<46} {name:<12} {e:10.3e} {e3:10.3e} {b:10.3e} {q:7.3f}{"" if ok else "  FAIL"}\n')


def make_model(A, C, R, weights=None, seed=SEED):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, A, 0.0, 1.0, 1.0, colour_channels=C, resolution=R, device='cuda:0', seed=seed,
                                       init_weights=weights is None)
    if weights is not None:
        m.load_flat_weights(weights)
    return m


def release():
    """the model and its modules refer to each other: the engine context (arena, packed weights) goes with the collection"""
    gc.collect()
    torch.cuda.empty_cache()


def oracle_pair(w, A, C, R):
    kw = dict(pi_dim=A, channels=C, resolution=R)
    return EO.OracleModel(w, EO.PhiloxNoise(SEED), **kw), EO.OracleModel(w, EO.PhiloxNoise(SEED), dtype=torch.float64, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. decoder (image form of the rule) and encoder (mean, logvar) against the fp64 oracle: 25 resolutions x 3 channel counts
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('R', RESOLUTIONS)
def test_networks_vs_fp64(R, C):
    A, M, st = 3, 3, 5
    w = synth.make_weights(WSEED + R, 1.15, A, C, R)
    s = PX.uniform_fill(3, (M, 10), 740 + R, -1.5, 1.5)
    fr = synth.make_frames_rgb(11 + R, M, C, R)
    m = make_model(A, C, R, w)
    try:
        po = m.model_down.decoder(s, stage=st, pass_=PX.PASS_D1).cpu()
        _, emean, elv = m.model_down.encoder_with_sample(fr, stage=st, pass_=PX.PASS_E1, eps=PX.normals(SEED, M, 10, PX.PASS_E1, 0, st))
        emean, elv = emean.cpu(), elv.cpu()
    finally:
        del m
        release()
    assert po.shape == (M, C, R, R)
    r32, r64 = [], []
    with torch.no_grad():
        for o, out in zip(oracle_pair(w, A, C, R), (r32, r64)):
            out += [o.decoder(torch.from_numpy(s), PX.PASS_D1, 0, st), *o.encoder(torch.from_numpy(fr), PX.PASS_E1, 0, st)]
    check(f'R{R}c{C}a{A}/nets_m{M}', [('po', po, r32[0], r64[0], True), ('e_mean', emean, r32[1], r64[1], False),
                                      ('e_lv', elv, r32[2], r64[2], False)])


# ------------------------------------------------------------------------------------------------------------------------------
# 2 + 3. calculate_G against the fp64 oracle (G, the three terms, the partial entropy sums, the stored images) and the launch counts of
# the call.  One decoder pass over 3 S M images and one encoder pass over S M images, each ONE launch group at the default options
# (run_core; dec_chunk_g = 16384, enc_chunk = 32768), so a class's count is its launches per group in run_decoder_g / run_encoder_g:
#   convT1_generic            : k_conv_g / k_convt_p<1> of the per-layer form -- 0 when k_convt_12 took layers 1 + 2
#   dec_a_convT1_convT2       : 1 either way (k_convt_12, or layer 2 alone)
#   dec_b_convT3_final_reduce : 1 (k_dec_bg, or layer 3 alone)
#   final_layer_generic       : 0 when k_dec_bg took the last two layers; 1 = k_final_g (resolution 32 by design: stride-1 third layer)
#   encoder                   : 4 = k_conv_e12 + k_conv_g (layer 3) + k_conv_g (layer 4) + the dense head; the per-layer form has 5
# A geometry that a launch predicate declines shows as (1, 1, 1, 1, 5) in its column.
# ------------------------------------------------------------------------------------------------------------------------------
PATH_CLASSES = ('convT1_generic', 'dec_a_convT1_convT2', 'dec_b_convT3_final_reduce', 'final_layer_generic', 'encoder')
EXPECTED_PATH = {
    32: (0, 1, 1, 1, 4),        # k_convt_12, k_convt_p + k_final_g, k_conv_e12
    36: (0, 1, 1, 0, 4),        # k_convt_12, k_dec_bg, k_conv_e12: this one and every one below
    40: (0, 1, 1, 0, 4),
    44: (0, 1, 1, 0, 4),
    48: (0, 1, 1, 0, 4),
    52: (0, 1, 1, 0, 4),
    56: (0, 1, 1, 0, 4),
    60: (0, 1, 1, 0, 4),
    64: (0, 1, 1, 0, 4),
    68: (0, 1, 1, 0, 4),
    72: (0, 1, 1, 0, 4),
    76: (0, 1, 1, 0, 4),
    80: (0, 1, 1, 0, 4),
    84: (0, 1, 1, 0, 4),
    88: (0, 1, 1, 0, 4),
    92: (0, 1, 1, 0, 4),
    96: (0, 1, 1, 0, 4),
    100: (0, 1, 1, 0, 4),
    104: (0, 1, 1, 0, 4),
    108: (0, 1, 1, 0, 4),
    112: (0, 1, 1, 0, 4),
    116: (0, 1, 1, 0, 4),
    120: (0, 1, 1, 0, 4),
    124: (0, 1, 1, 0, 4),
    128: (0, 1, 1, 0, 4),
}
DEC_GROUPS = ENC_GROUPS = 1


@pytest.mark.parametrize('R', RESOLUTIONS)
def test_calculate_G_vs_fp64(R):
    C, A = channels_of(R), pi_dim_of(R)
    M, S, st = A + 1, 2, 6
    w = synth.make_weights(WSEED + R, 1.15, A, C, R)
    s0 = PX.uniform_fill(4, (M, 10), 741 + R, -1.0, 1.0)
    pi0 = np.eye(A, dtype=np.float32)[np.arange(M) % A]
    m = make_model(A, C, R, w)
    try:
        parts = []
        m.prof_enable(True)
        try:
            r = m.calculate_G(s0, pi0, samples=S, stage=st, eps=eps_calcG(SEED, M, S, st), _parts=parts)
            prof = m.prof_read()
        finally:
            m.prof_enable(False)
        r = (r[0].cpu(), [t.cpu() for t in r[1]], r[2].cpu(), r[3].cpu(), r[4].cpu())
        parts = [[p.cpu() for p in parts[0]]]
    finally:
        del m
        release()
    counts = tuple(int(prof[k][1]) for k in PATH_CLASSES)
    groups = (DEC_GROUPS, DEC_GROUPS, DEC_GROUPS, DEC_GROUPS, ENC_GROUPS)
    want = tuple(n * g for n, g in zip(EXPECTED_PATH[R], groups))
    print(f'R{R}c{C}a{A}: launches', dict(zip(PATH_CLASSES, counts)))
    assert counts == want, f'resolution {R}: launches per class {dict(zip(PATH_CLASSES, counts))}, expected {dict(zip(PATH_CLASSES, want))}'
    with torch.no_grad():
        o32, o64 = (_orc_G(s0, pi0, S, st)(o) for o in oracle_pair(w, A, C, R))
    check(f'R{R}c{C}a{A}/calcG_m{M}s{S}', _calcG_quantities(r, parts, o32, o64))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. A/B on the GPU alone: the fused kernels against the separate launches they replace, and small launch groups against one
# ------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = {'ct_fuse12': 1, 'enc_tiled': 2, 'fuse_final_g': 1, 'dec_chunk_g': 16384, 'enc_chunk': 32768}


@pytest.mark.parametrize('R', RESOLUTIONS)
def test_fused_equals_separate(R):
    """k_convt_12 against k_convt_p<1> + k_convt_p<2> (option ct_fuse12 1 / 0) and k_conv_e12 against k_conv_e per layer against k_conv_g
    (enc_tiled 2 / 1 / 0): the same operations per element in the same order, bit-identical.  k_dec_bg against k_convt_p + k_final_g
    (fuse_final_g 1 / 0; not at resolution 32, which has no fused form): images up to the summation order of the 3 x 3 taps, sums within
    the fp32 bound -- the tolerances of tests/test_generic_geometry.py.  Launch groups of two images (dec_chunk_g = enc_chunk = 2: 2, 2 and
    1 images of the encoder call) against one group: bit-identical.  Five rows, with and without the row mask [1, 1, 0, 1, 0]."""
    from daimc_amd.model import Rows
    C, A = channels_of(R), pi_dim_of(R)
    M, S, st = 5, 2, 4
    w = synth.make_weights(WSEED + 1 + R, 1.15, A, C, R)
    s0 = PX.uniform_fill(4, (M, 10), 61 + R, -1.2, 1.2)
    pi0 = np.eye(A, dtype=np.float32)[np.arange(M) % A]
    fr = synth.make_frames_rgb(16 + R, M, C, R)
    m = make_model(A, C, R, w, seed=6)
    m.eps_source, m.u_source = PX.normals, PX.uniforms
    mask = torch.tensor([1, 1, 0, 1, 0], dtype=torch.uint8, device=m.device)
    live = mask.bool()

    def run():
        parts = []
        full = m.calculate_G(s0, pi0, samples=S, stage=st, _parts=parts)
        part = m.calculate_G(s0, pi0, samples=S, stage=st, rows=Rows(mask=mask))
        enc = m.model_down.encoder_with_sample(fr, stage=3, pass_=PX.PASS_E1)
        return {'full': [full[0], *full[1], full[2], full[4], parts[0][0], parts[0][1]], 'live': [part[0][live], part[4][live]], 'enc': list(enc)}

    def same_bits(x, y, what):
        for key in x:
            for i, (a, b) in enumerate(zip(x[key], y[key])):
                assert torch.equal(a, b), f'resolution {R}, {what}: output {key}[{i}] differs, max|d| = {float((a - b).abs().max()):.3e}'

    try:
        ref = run()
        assert all(torch.isfinite(t).all() for v in ref.values() for t in v)
        for i, t in enumerate(ref['live']):
            assert torch.equal(t, (ref['full'][0], ref['full'][5])[i][live]), f'resolution {R}: live rows of the masked call differ from the full call'
        m.set_option('ct_fuse12', 0)
        same_bits(ref, run(), 'ct_fuse12 0')
        m.set_option('ct_fuse12', 1)
        for mode in (1, 0):
            m.set_option('enc_tiled', mode)
            same_bits(ref, run(), f'enc_tiled {mode}')
        m.set_option('enc_tiled', 2)
        m.set_option('dec_chunk_g', 2)
        m.set_option('enc_chunk', 2)
        same_bits(ref, run(), 'dec_chunk_g 2, enc_chunk 2')
        m.set_option('dec_chunk_g', DEFAULTS['dec_chunk_g'])
        m.set_option('enc_chunk', DEFAULTS['enc_chunk'])
        if R != 32:
            m.set_option('fuse_final_g', 0)
            sep = run()
            G, t0, t1, t2, ps1, po, p21, p22 = ref['full']
            Gu, t0u, t1u, t2u, ps1u, pou, p21u, p22u = sep['full']
            np.testing.assert_allclose(c(po), c(pou), rtol=0, atol=4e-6)
            tol = sumtol(c(t0u))
            np.testing.assert_allclose(c(t0), c(t0u), atol=tol)
            np.testing.assert_allclose(c(p21), c(p21u), atol=tol)
            np.testing.assert_allclose(c(p22), c(p22u), atol=tol)
            np.testing.assert_allclose(c(G), c(Gu), atol=3 * tol)
            np.testing.assert_allclose(c(t1), c(t1u), atol=1e-4)      # term1 reads the encoder's view of the stored images (a few ulp apart)
            np.testing.assert_allclose(c(ref['live'][1]), c(sep['live'][1]), rtol=0, atol=4e-6)
            np.testing.assert_allclose(c(ref['live'][0]), c(sep['live'][0]), atol=3 * tol)
    finally:
        for name, value in DEFAULTS.items():
            m.set_option(name, value)
        del m
        release()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the scratch plan: what tests/test_generic_geometry.py::test_reserve_no_growth_generic asserts at 84, at every resolution
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RESOLUTIONS)
def test_reserve_no_growth(R):
    """after efe_reserve for (rows, steps, samples) a rollout at that size never grows the arena, and efe_rollout_scratch_bytes is exact:
    the arena use of efe_rollout plus 1 MiB of head-room.  (As in the test at 84 the high-water mark is that of the call the plan counts,
    efe_rollout without a sum_terms output, which takes 3 M floats more than calculate_G_repeated's.)"""
    from test_gpu_parity import rollout_without_terms
    C, A = channels_of(R), pi_dim_of(R)
    rows, steps, samples = 4, 2, 2
    m = make_model(A, C, R, seed=2)
    try:
        need = m.reserve(rows, steps, samples)
        st0 = m.arena_stats()
        assert st0['capacity_bytes'] >= need
        o = synth.make_frames_rgb(35, rows, C, R)
        pi = np.eye(A, dtype=np.float32)[np.arange(rows) % A]
        G = m.calculate_G_repeated(o, pi, steps=steps, samples=samples, stage=0)[0]
        assert torch.isfinite(G).all()
        rollout_without_terms(m, o, pi, steps, samples, 10)
        st1 = m.arena_stats()
    finally:
        del m
        release()
    assert st1['grow_count'] == st0['grow_count'] and st1['capacity_bytes'] == st0['capacity_bytes']
    print('resolution', R, 'need', need, 'high water', st1['high_water_bytes'], 'difference', need - st1['high_water_bytes'])
    assert need - st1['high_water_bytes'] == 1 << 20
