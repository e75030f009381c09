"""CPU emulation of k_mid_grad's fp32 summation order (csrc/train.hip), to check the fp64 rule of tests/test_fp64_parity.py on the gradient
cases of tests/test_train_mid_gpu.py before a GPU run: sixteen interleaved accumulators per contraction over a layer's width (16-channel
chunk c -> accumulator c & 15, within a chunk MFMA step s contracts channels 16 c + 4 q + s, q = 0..3 in turn), the fixed tree of
tree<16> of csrc/train_mlp.h (tree16 below), one 16-row chain per tile for dW, per-workgroup slabs (tiles p, p + G, ..., G = min(T, 8)) summed in ascending order.
An fp32 fma is formed in float64 and rounded once more (a double rounding that moves a result by at most one ulp in rare ties); expf /
logf are numpy's.  Prints every figure and the worst ratio e_eng / (e_32 + 2 ulp) (the rule allows 4).

Usage:  python tools/emulate_mid_grad.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import philox as PX                       # noqa: E402
from oracle import synth                              # noqa: E402
import train_mid_ref as TM                            # noqa: E402
from test_fp64_parity import fp64_rule                # noqa: E402

f32 = np.float32
SLABS = 8


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def tree16(a):
    b = [(a[4 * i] + a[4 * i + 1]) + (a[4 * i + 2] + a[4 * i + 3]) for i in range(4)]
    return (b[0] + b[1]) + (b[2] + b[3])


def contract(A, B):
    """C[r][f] = sum_k A[r][k] B[f][k] in the kernel's order; K is padded to whole 16-channel chunks with zeros"""
    K = A.shape[1]
    Kp = (K + 15) // 16 * 16
    A = np.pad(A, ((0, 0), (0, Kp - K)))
    B = np.pad(B, ((0, 0), (0, Kp - K)))
    acc = [np.zeros((A.shape[0], B.shape[0]), f32) for _ in range(16)]
    for c in range(Kp // 16):
        j = c & 15
        for s in range(4):
            for q in range(4):
                k = 16 * c + 4 * q + s
                acc[j] = fma(A[:, k:k + 1], B[None, :, k], acc[j])
    return tree16(acc)


def emulate(weights, b, stage, pi_dim=4, seed=TM.SEED, pass_=TM.PASS_FE_T, sample=0, row_offset=0):
    s0, pi, qm, qv, om = b
    M = s0.shape[0]
    W = [np.asarray(weights[f'mid.ps_net.{i}.weight'], f32) for i in (0, 3, 6, 9)]
    Bs = [np.asarray(weights[f'mid.ps_net.{i}.bias'], f32) for i in (0, 3, 6, 9)]
    om = np.broadcast_to(np.asarray(om, f32).reshape(-1), (M,))
    T = (M + 15) // 16
    Mp = 16 * T
    x = np.zeros((Mp, pi_dim + 10), f32)
    x[:M] = np.concatenate([pi, s0], 1)
    acts = [x]
    for l in range(4):
        y = contract(acts[l], W[l]) + Bs[l][None, :]
        if l < 3:
            mask = PX.dropout_mask(seed, PX.TAG_MID + l, Mp, 512, pass_, sample, stage, row_offset).astype(f32)
            y = np.maximum(y, f32(0)) * mask
        acts.append(y.astype(f32))
    z = acts[4]
    mu2, lv2 = z[:M, :10], z[:M, 10:]
    w = om[:, None]
    inv_M = f32(1.0) / f32(M)
    d = qm - mu2
    num = np.exp(qv) + d * d
    den = (f32(2) * np.exp(lv2)) / w
    ratio = num / den
    dz = np.zeros((Mp, 20), f32)
    dz[:M, :10] = inv_M * (-((f32(2) * d) / den))
    dz[:M, 10:] = inv_M * (f32(0.5) - ratio)
    G = min(T, SLABS)
    grads = {}
    dl = dz
    for l in (3, 2, 1, 0):
        xl = acts[l]
        slabs_w = [None] * G
        slabs_b = [None] * G
        for t in range(T):
            rows = slice(16 * t, 16 * t + 16)
            acc = np.zeros((dl.shape[1], xl.shape[1]), f32)
            for r in range(16 * t, 16 * t + 16):
                acc = fma(dl[r][:, None], xl[r][None, :], acc)
            sb = dl[16 * t].copy()
            for r in range(16 * t + 1, 16 * t + 16):
                sb = sb + dl[r]
            p = t % G
            slabs_w[p] = acc if slabs_w[p] is None else slabs_w[p] + acc
            slabs_b[p] = sb if slabs_b[p] is None else slabs_b[p] + sb
            del rows
        gw, gb = slabs_w[0], slabs_b[0]
        for p in range(1, G):
            gw, gb = gw + slabs_w[p], gb + slabs_b[p]
        idx = (0, 3, 6, 9)[l]
        grads[f'ps_net.{idx}.weight'], grads[f'ps_net.{idx}.bias'] = gw, gb
        if l > 0:
            dl = (contract(dl, W[l].T.copy()) * np.where(xl > 0, f32(2), f32(0))).astype(f32)
    return grads


CASES = [('g115', M, s) for M, s in ((1, 101), (3, 103), (16, 116), (17, 117), (50, 150), (129, 229))] + \
        [('g100', 17, 117), ('g100', 50, 151), ('sparse', 17, 117), ('sparse', 50, 150)]


def main():
    fams = {'g115': synth.make_weights(1234, 1.15), 'g100': synth.make_weights(7, 1.0), 'sparse': synth.stress_weights('sparse')}
    worst = 0.0
    for fam, M, seed in CASES:
        w, b = fams[fam], TM.batch_mid(seed, M)
        margin = TM.preact_margin(w, b, 3)
        g = emulate(w, b, 3)
        g32 = TM.grads(w, b, 3, torch.float32)[3]
        g64 = TM.grads(w, b, 3, torch.float64)[3]
        for k in TM.KEYS:
            for r in fp64_rule(k, g[k], g32[k], g64[k]):
                worst = max(worst, r[4])
                print(f'{fam} M={M} seed={seed} margin {margin:.2e} {r[0]}: e_emu {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}'
                      f'{"" if r[5] else "  FAILS"}', flush=True)
    print(f'worst ratio {worst:.2f} (allowed 4)')


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
