#!/usr/bin/env python
"""Writes tests/golden/decoder_bits_r11.npz: the outputs of four small decoder-heavy engine calls, stored bit for bit, so that a kernel
change that claims to leave every output element's operations in the same order can be held to it (tests/test_decoder_bits_frozen_gpu.py).

Run it ONCE, on the GPU, on the build of the commit BEFORE the kernel change (the fixture tests new code against its parent, never
against itself):

    python tools/make_decoder_bits.py [out.npz]

Weights synth.make_weights(1234, 1.15), seed 11.  The cases (run_cases() is shared with the test):
  i    calculate_G, 4 rows x S = 1 (12 decoder images), option dec_split = 0: the large-launch k_fc4<2>, k_dec_a, k_dec_b4<1>
  ii   the same with dec_split = 1: k_dec_a_s and k_dec_b4<4>
  iii  case i with a row mask that kills rows 1 and 2 (the dead-row schedule); the live rows 0 and 3 are compared
  iv   calculate_G_repeated, 8 rows x depth 2 x S = 2; the rollout stores the root step's images (po1)
Cases i - iii are the same computation by the engine's own contracts (launch forms agree bit for bit; a masked call leaves live rows
untouched), so the file holds ONE copy of their arrays (g_*): this tool refuses to write the file if the parent build breaks that."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'decoder_bits_r11.npz')
NAMES = ('G', 'term0', 'term1', 'term2', 'po1')
LIVE = (0, 3)                  # rows of case iii that stay alive


def _arrays(G, terms, po1):
    return {n: x.detach().cpu().numpy().copy() for n, x in zip(NAMES, (G, terms[0], terms[1], terms[2], po1))}


def run_cases(device='cuda:0'):
    """-> {'i' | 'ii' | 'iii' | 'iv': {name: float32 array}} (case iii: rows LIVE only)"""
    import daimc_amd
    from daimc_amd.model import Rows
    from oracle import philox as PX
    from oracle import synth
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=device, seed=11, init_weights=False)
    m.load_flat_weights(synth.make_weights(1234, 1.15))
    s0 = torch.from_numpy(PX.uniform_fill(3, (4, 10), 61, -1.5, 1.5).astype(np.float32)).to(m.device)
    alive = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=m.device)
    out = {}
    try:
        m.set_option('dec_split', 0)
        r = m.calculate_G(s0, m.pi_one_hot, samples=1, stage=5)
        out['i'] = _arrays(r[0], r[1], r[4])
        r = m.calculate_G(s0, m.pi_one_hot, samples=1, stage=5, rows=Rows(mask=alive))
        out['iii'] = {k: v[list(LIVE)] for k, v in _arrays(r[0], r[1], r[4]).items()}
        m.set_option('dec_split', 1)
        r = m.calculate_G(s0, m.pi_one_hot, samples=1, stage=5)
        out['ii'] = _arrays(r[0], r[1], r[4])
    finally:
        m.set_option('dec_split', 1)
    o = np.repeat(synth.make_frames(23, 2), 4, axis=0)
    pi = np.tile(np.eye(4, dtype=np.float32), (2, 1))
    r = m.calculate_G_repeated(o, pi, steps=2, samples=2, stage=8)
    out['iv'] = _arrays(r[0], r[1], r[2])
    torch.cuda.synchronize()
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def main(path):
    c = run_cases()
    for n in NAMES:
        assert np.isfinite(c['i'][n]).all() and np.isfinite(c['iv'][n]).all(), n
        assert bits_equal(c['i'][n], c['ii'][n]), f'{n}: dec_split = 0 and 1 disagree on this build'
        assert bits_equal(c['i'][n][list(LIVE)], c['iii'][n]), f'{n}: the masked call changed a live row on this build'
    assert c['i']['po1'].shape == (4, 1, 64, 64) and c['iv']['po1'].shape == (8, 1, 64, 64)
    assert float(c['i']['po1'].std()) > 1e-3 and float(c['iv']['po1'].std()) > 1e-3          # (the images are not flat)
    arrs = {f'g_{n}': c['i'][n] for n in NAMES}
    arrs.update({f'r_{n}': c['iv'][n] for n in NAMES})
    np.savez_compressed(path, **arrs)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT)
