"""CPU emulation of the fp32 summation orders of csrc/train_dec_head.hip, to check the fp64 rule of tests/test_fp64_parity.py on the gradient
cases of tests/test_train_dec_head_gpu.py before a GPU run.  Every contraction of the head is emulated:
  * over a layer's width (forward of the four layers, d_h3 per 256-feature segment, the data gradients of layers 2, 1, 0, d_s): the chain
    of csrc/train_mlp.h's order contract with NACC = 8, joined by its tree<8> (tree8 below);
  * d_h3's join of the 64 segments: tree8 of eight sequential sums of eight consecutive segments;
  * dW_3 / db_3: per 64-row group the 16-row tiles ascending, one 16-term chain (db: sequential sum) per tile, group = chunks added in
    ascending order, gradient = groups added in ascending order;
  * dW / db of layers 0..2: one 16-term chain per tile into slab t mod 4, gradient = ((slab_0 + slab_1) + slab_2) + slab_3.
The ConvTranspose2d tail between the emulated forward and backward is torch's fp32 on the CPU (its kernels are csrc/train_dec.hip's, with
tests of their own): it maps the emulated h4 to d_h4.  Both oracles take their gates from the emulated h1..h4 and that tail's y1..y3, as
the GPU tests take them from the engine.  An fp32 fma is formed in float64 and rounded once more (a double rounding that moves a result by
at most one ulp in rare ties).  Prints every figure and the worst ratio e_emu / (e_32 + 2 ulp) (the rule allows 4).

Usage:  python tools/emulate_dec_head.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import synth                              # noqa: E402
import train_dec_ref as TD                            # noqa: E402
import train_dec_head_ref as TH                       # noqa: E402
from test_fp64_parity import fp64_rule                # noqa: E402

f32 = np.float32
STAGE = 3


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def tree8(a):
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def contract8(A, B):
    """C[r][f] = sum_k A[r][k] B[f][k] in the kernels' order; K is padded to whole 16-feature chunks with zeros"""
    K = A.shape[1]
    Kp = (K + 15) // 16 * 16
    A = np.pad(A, ((0, 0), (0, Kp - K)))
    B = np.pad(B, ((0, 0), (0, Kp - K)))
    acc = [np.zeros((A.shape[0], B.shape[0]), f32) for _ in range(8)]
    for c in range(Kp // 16):
        j = c & 7
        for s in range(4):
            for q in range(4):
                k = 16 * c + 4 * q + s
                acc[j] = fma(A[:, k:k + 1], B[None, :, k], acc[j])
    return tree8(acc)


def rows_chain(g, x):
    """one tile: sum_r g[r][:, None] x[r][None, :] as a 16-term chain over the tile's rows in ascending order (absent rows: exact zeros)"""
    acc = np.zeros((g.shape[1], x.shape[1]), f32)
    for r in range(g.shape[0]):
        acc = fma(g[r][:, None], x[r][None, :], acc)
    return acc


def rows_sum(g):
    s = g[0].copy()
    for r in range(1, g.shape[0]):
        s = s + g[r]
    return s


def forward(w, s, mk):
    W = [np.asarray(w[f'down.po_net.{i}.weight'], f32) for i in TH.HEAD]
    B = [np.asarray(w[f'down.po_net.{i}.bias'], f32) for i in TH.HEAD]
    x, hs = s.astype(f32), []
    for l in range(4):
        x = (np.maximum(contract8(x, W[l]) + B[l][None, :], f32(0)) * mk[l]).astype(f32)
        hs.append(x)
    return hs


def backward(w, s, hs, d_h4):
    W = [np.asarray(w[f'down.po_net.{i}.weight'], f32) for i in TH.HEAD]
    M = s.shape[0]
    gate = lambda h: np.where(h > 0, f32(2), f32(0))          # noqa: E731
    g3 = (d_h4.astype(f32) * gate(hs[3])).astype(f32)
    grads = {}
    # layer 3: groups of 64 rows, tiles of 16
    gw = gb = None
    for m0 in range(0, M, 64):
        aw = np.zeros((16384, 256), f32)
        ab = np.zeros(16384, f32)
        for r0 in range(m0, min(m0 + 64, M), 16):
            r1 = min(r0 + 16, M)
            aw = aw + rows_chain(g3[r0:r1], hs[2][r0:r1])
            ab = ab + (np.zeros(16384, f32) + rows_sum(g3[r0:r1]))
        gw, gb = (aw, ab) if gw is None else (gw + aw, gb + ab)
    grads['po_net.9.weight'], grads['po_net.9.bias'] = gw, gb
    # d_h3: 64 segments of 256 features, joined as tree8 of eight sequential sums
    W3T = np.ascontiguousarray(W[3].T)
    seg = [contract8(g3[:, 256 * i:256 * (i + 1)], W3T[:, 256 * i:256 * (i + 1)]) for i in range(64)]
    j8 = []
    for j in range(8):
        sm = seg[8 * j]
        for i in range(1, 8):
            sm = sm + seg[8 * j + i]
        j8.append(sm)
    g = (tree8(j8) * gate(hs[2])).astype(f32)
    xs = [s.astype(f32), hs[0], hs[1]]
    for l in (2, 1, 0):
        slabs_w, slabs_b = [None] * 4, [None] * 4
        for t in range((M + 15) // 16):
            r0, r1 = 16 * t, min(16 * t + 16, M)
            cw, cb = rows_chain(g[r0:r1], xs[l][r0:r1]), rows_sum(g[r0:r1])
            p = t % 4
            slabs_w[p] = cw if slabs_w[p] is None else slabs_w[p] + cw
            slabs_b[p] = cb if slabs_b[p] is None else slabs_b[p] + cb
        sw, sb = slabs_w[0], slabs_b[0]
        for p in range(1, 4):
            if slabs_w[p] is not None:
                sw, sb = sw + slabs_w[p], sb + slabs_b[p]
        idx = TH.HEAD[l]
        grads[f'po_net.{idx}.weight'], grads[f'po_net.{idx}.bias'] = sw, sb
        nxt = contract8(g, np.ascontiguousarray(W[l].T))
        g = (nxt * gate(xs[l])).astype(f32) if l > 0 else nxt
    return grads, g


def tail32(w, h4, o1, scale):
    """torch fp32 over the tail from a given h4 -> (d_h4, y1..y3)"""
    r = TD.run(w, h4, o1, torch.float32, scale=scale)
    return r['d_h4'], r['y']


CASES = [('g115', M) for M in (1, 2, 5, 17, 33, 65)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)]


def main():
    fams = {'g115': synth.make_weights(1234, 1.15), 'g100': synth.make_weights(7, 1.0), 'sparse': synth.stress_weights('sparse')}
    worst = 0.0
    for fam, M in CASES:
        w = fams[fam]
        s, o1 = TH.inputs(2000 + M, M)
        mk = TH.masks(M, STAGE)
        hs = forward(w, s, [m.numpy() for m in mk])
        d_h4, ys = tail32(w, hs[3], o1, 1.0 / M)
        grads, d_s = backward(w, s, hs, d_h4)
        gates = tuple(hs) + tuple(ys)
        o32 = TH.run(w, s, o1, STAGE, torch.float32, gates=gates)
        o64 = TH.run(w, s, o1, STAGE, torch.float64, gates=gates)
        rows = [(k, grads[k], o32['grads'][k], o64['grads'][k]) for k in TH.HEAD_KEYS]
        rows.append(('d_s', d_s, o32['d_s'], o64['d_s']))
        rows += [(f'h{i + 1}', hs[i], o32['h'][i], o64['h'][i]) for i in range(4)]
        for name, e, a32, a64 in rows:
            for r in fp64_rule(name, e, a32, a64):
                worst = max(worst, r[4])
                print(f'{fam} M={M} {r[0]}: e_emu {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}{"" if r[5] else "  FAILS"}', flush=True)
    print(f'worst ratio {worst:.2f} (allowed 4)')


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
