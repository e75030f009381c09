#!/usr/bin/env python
"""Writes tests/golden/generic_bits.npz: the outputs of the geometry-generic kernels (generic_dec.hip, generic_enc.hip), stored bit for
bit, so that a change that claims to leave every output element's operations and their order alone can be held to it
(tests/test_generic_bits_frozen_gpu.py).

Run it ONCE, on the GPU, on the build of the commit BEFORE the kernel change (the fixture tests new code against its parent, never
against itself):

    python tools/make_generic_bits.py [out.npz]

The six geometries (A, C, R) are those of tests/test_generic_geometry.py, the smallest set that hits every strip shape (decoder base 21,
12, 16, 32, 9, 8: strips of 3, 5, 4, 2, 7, 8 rows; short last strips, a Win that does not divide the tile, 1..3 channels, the stride-1
last layer of resolution 32).  Weights synth.make_weights(300 + R, 1.15, A, C, R), seed 13, M = 3 rows, one sample.  Per geometry
(run_cases() is shared with the test):
  default     calculate_G under the default options: k_convt_12, k_dec_bg
  ct_fuse12   the same with ct_fuse12 = 0: k_convt_p<1>, k_convt_p<2, 4> per layer
  fuse_final  the same with fuse_final_g = 0: k_convt_p<2, 8> as layer 3 (k_convt_p<1, 8> at resolution 32) + k_final_g
  mask        the default call with the row mask [1, 0, 1]; the live rows are kept
  enc2, enc1  model_down.encoder_with_sample on make_frames_rgb frames under enc_tiled = 2 (k_conv_e12) and 1 (k_conv_e per layer)
G, the three terms and the encoder's s / mean / logvar are stored in full, the stored images as the SHA-256 of their float32 bytes."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'generic_bits.npz')
GEOMETRIES = ((3, 3, 84), (4, 1, 48), (3, 3, 64), (5, 2, 128), (2, 3, 36), (3, 3, 32))
G_CASES = ('default', 'ct_fuse12', 'fuse_final', 'mask')
E_CASES = ('enc2', 'enc1')
CASES = G_CASES + E_CASES
G_NAMES = ('G', 'term0', 'term1', 'term2', 'po1_sha256')
E_NAMES = ('s', 'mean', 'logvar')
M = 3
MASK = (1, 0, 1)
LIVE = [i for i, a in enumerate(MASK) if a]


def digest(x):
    """SHA-256 of the float32 bytes of x, as uint8[32]"""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    assert x.dtype == np.float32
    return np.frombuffer(hashlib.sha256(x.tobytes()).digest(), dtype=np.uint8).copy()


def _g_arrays(r, rows=None):
    sel = (lambda x: x) if rows is None else (lambda x: x[rows])
    out = {n: sel(x.detach().cpu().numpy()).copy() for n, x in zip(G_NAMES, (r[0], r[1][0], r[1][1], r[1][2]))}
    out['po1_sha256'] = digest(sel(r[4].detach().cpu().numpy()))
    return out


def run_cases(geometry, device='cuda:0'):
    """-> {case: {name: array}} for one geometry (A, C, R); case 'mask' holds the rows LIVE only"""
    import daimc_amd
    from daimc_amd.model import Rows
    from oracle import philox as PX
    from oracle import synth
    A, C, R = geometry
    m = daimc_amd.ActiveInferenceModel(10, A, 0.0, 1.0, 1.0, colour_channels=C, resolution=R, device=device, seed=13, init_weights=False)
    m.load_flat_weights(synth.make_weights(300 + R, 1.15, A, C, R))
    s0 = PX.uniform_fill(4, (M, 10), 70 + R, -1.2, 1.2)
    pi0 = np.eye(A, dtype=np.float32)[np.arange(M) % A]
    fr = synth.make_frames_rgb(17, M, C, R)
    alive = torch.tensor(MASK, dtype=torch.uint8, device=m.device)
    out = {}
    try:
        out['default'] = _g_arrays(m.calculate_G(s0, pi0, samples=1, stage=5))
        out['mask'] = _g_arrays(m.calculate_G(s0, pi0, samples=1, stage=5, rows=Rows(mask=alive)), LIVE)
        m.set_option('ct_fuse12', 0)
        out['ct_fuse12'] = _g_arrays(m.calculate_G(s0, pi0, samples=1, stage=5))
        m.set_option('ct_fuse12', 1)
        m.set_option('fuse_final_g', 0)
        out['fuse_final'] = _g_arrays(m.calculate_G(s0, pi0, samples=1, stage=5))
        m.set_option('fuse_final_g', 1)
        for case, mode in (('enc2', 2), ('enc1', 1)):
            m.set_option('enc_tiled', mode)
            r = m.model_down.encoder_with_sample(fr, stage=3, pass_=PX.PASS_E1)
            out[case] = {n: x.detach().cpu().numpy().copy() for n, x in zip(E_NAMES, r)}
    finally:
        m.set_option('ct_fuse12', 1)
        m.set_option('fuse_final_g', 1)
        m.set_option('enc_tiled', 2)
    torch.cuda.synchronize()
    return out


def key(geometry, case, name):
    return 'a%dc%dr%d_%s_%s' % (*geometry, case, name)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


def main(path):
    arrs = {}
    for g in GEOMETRIES:
        c = run_cases(g)
        for case in CASES:
            for n, x in c[case].items():
                assert x.dtype == np.uint8 or np.isfinite(x).all(), (g, case, n)
                arrs[key(g, case, n)] = x
        # the engine's own contracts on this build: the fused and per-layer forms agree bit for bit, a masked call leaves live rows alone
        for n in G_NAMES[:-1]:
            assert bits_equal(c['default'][n], c['ct_fuse12'][n]), (g, n, 'ct_fuse12 = 0 and 1 disagree on this build')
            assert bits_equal(c['default'][n][LIVE], c['mask'][n]), (g, n, 'the masked call changed a live row on this build')
        assert bits_equal(c['default']['po1_sha256'], c['ct_fuse12']['po1_sha256']), g
        for n in E_NAMES:
            assert bits_equal(c['enc2'][n], c['enc1'][n]), (g, n, 'enc_tiled = 2 and 1 disagree on this build')
            assert float(c['enc2'][n].std()) > 1e-4, (g, n)
        print(g, 'ok', flush=True)
    np.savez_compressed(path, **arrs)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT)
