#!/usr/bin/env python
"""Writes tests/golden/decoder_ab_bits_r13.npz: the outputs of the fused decoder tail k_dec_ab (and of the small-launch pair k_dec_a_s,
k_dec_b4<4>), stored bit for bit, so that a change of k_dec_a's two layers that claims to leave every output element's operations in
the same order is held to the build BEFORE it (tests/test_decoder_overlap_gpu.py).  tests/test_decoder_fused_ab_gpu.py compares two
forms of one tree with each other; both forms share wino_l1 and f22_l2, so it cannot see a change of those.

Run it ONCE, on the GPU, on the build of the parent commit (the fixture tests new code against its parent, never against itself):

    python tools/make_decoder_ab_bits.py [out.npz]

Two weight sets: 'control' = synth.make_weights(1234, 1.15) and 'gain2' = synth.stress_weights('gain2') (the high-gain family of the fp64
tests).  Cases per weight set (run_case() is shared with the test), dec_fuse_ab = 1 throughout:
  roll   calculate_G_repeated, 2 rows x depth 1 x 22 samples = 132 decoder images, the smallest launch k_dec_ab takes (> 128); the three
         pass kinds, so the entropy and the reward mode, and the root step's stored images.  dec_ab_grid 0 (one workgroup per image) and
         3 (44 images per workgroup: what one image leaves pending is retired across an image boundary)
  mask   calculate_G, 15 rows x 3 samples = 135 images, row mask [1,1,0,1,0] x 3: dead images between live ones.  The live rows' G, terms
         and per-image sums (`parts`), and the stored images of a seeded sample of the live rows; dec_ab_grid 0 and 3
  small  calculate_G, 4 rows x 1 sample = 12 images with dec_split = 1: k_dec_a_s (the NR = 1 form of wino_l1) and k_dec_b4<4>
The grid is a schedule, not a computation: this tool refuses to write the file if the parent build's two grids disagree, and the file
holds one copy of each case."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'decoder_ab_bits_r13.npz')
WEIGHTS = ('control', 'gain2')
CASES = ('roll', 'mask', 'small')
GRIDS = (0, 3)
MASK_ROWS, MASK_S = 15, 3
ALIVE = np.array([1, 1, 0, 1, 0] * (MASK_ROWS // 5), dtype=np.uint8)
LIVE = np.flatnonzero(ALIVE)
IMG_ROWS = np.sort(np.random.RandomState(14).choice(LIVE, 4, replace=False))      # the live rows whose stored images the file keeps


def make_model(wname, device='cuda:0'):
    import daimc_amd
    from oracle import synth
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=device, seed=11, init_weights=False)
    m.load_flat_weights(synth.make_weights(1234, 1.15) if wname == 'control' else synth.stress_weights(wname))
    return m


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).view(np.uint32).copy()


def run_case(m, case, grid=0):
    """-> {name: uint32 array}, the bit patterns of the case's outputs (the model's options are put back)"""
    from daimc_amd.model import Rows
    from oracle import philox as PX
    from oracle import synth
    try:
        m.set_option('dec_fuse_ab', 1)
        m.set_option('dec_ab_grid', grid)
        if case == 'roll':
            r = m.calculate_G_repeated(synth.make_frames(23, 2), np.eye(4, dtype=np.float32)[[1, 2]], steps=1, samples=22, stage=8)
            out = {'G': _bits(r[0]), 'term0': _bits(r[1][0]), 'term1': _bits(r[1][1]), 'term2': _bits(r[1][2]), 'po1': _bits(r[2])}
        elif case == 'mask':
            s0 = torch.from_numpy(PX.uniform_fill(3, (MASK_ROWS, 10), 61, -1.5, 1.5).astype(np.float32)).to(m.device)
            pi = torch.from_numpy(np.eye(4, dtype=np.float32)[np.arange(MASK_ROWS) % 4]).to(m.device)
            parts = []
            r = m.calculate_G(s0, pi, samples=MASK_S, stage=5, rows=Rows(mask=torch.from_numpy(ALIVE).to(m.device)), _parts=parts)
            out = {'G': _bits(r[0])[LIVE], 'term0': _bits(r[1][0])[LIVE], 'term1': _bits(r[1][1])[LIVE], 'term2': _bits(r[1][2])[LIVE],
                   'po1': _bits(r[4])[IMG_ROWS], 'parts': _bits(parts[0])[:, LIVE]}
        elif case == 'small':
            m.set_option('dec_split', 1)
            s0 = torch.from_numpy(PX.uniform_fill(3, (4, 10), 61, -1.5, 1.5).astype(np.float32)).to(m.device)
            parts = []
            r = m.calculate_G(s0, m.pi_one_hot, samples=1, stage=5, _parts=parts)
            out = {'G': _bits(r[0]), 'term0': _bits(r[1][0]), 'term1': _bits(r[1][1]), 'term2': _bits(r[1][2]), 'po1': _bits(r[4]),
                   'parts': _bits(parts[0])}
        else:
            raise ValueError(case)
        torch.cuda.synchronize()
        return out
    finally:
        m.set_option('dec_ab_grid', 0)


def main(path):
    arrs = {}
    for wname in WEIGHTS:
        m = make_model(wname)
        for case in CASES:
            got = run_case(m, case, 0)
            if case != 'small':
                other = run_case(m, case, GRIDS[1])
                for n in got:
                    assert np.array_equal(got[n], other[n]), f'{wname} {case} {n}: dec_ab_grid 0 and {GRIDS[1]} disagree on this build'
            po = got['po1'].view(np.float32)
            assert float(po[np.isfinite(po)].std()) > 1e-3, (wname, case)          # (the images are not flat)
            if wname == 'control':
                assert all(np.isfinite(v.view(np.float32)).all() for v in got.values()), (wname, case)
            print(wname, case, {n: (v.shape, int((~np.isfinite(v.view(np.float32))).sum())) for n, v in got.items()})
            arrs.update({f'{wname}_{case}_{n}': v for n, v in got.items()})
    np.savez_compressed(path, **arrs)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT)
