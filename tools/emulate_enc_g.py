"""CPU emulation of the fp32 summation orders of csrc/train_enc_g.hip, to check the fp64 rule of tests/test_fp64_parity.py on gradient cases
of tests/test_train_enc_g_gpu.py before a GPU run.  tools/emulate_dec_head.py's chain (contract8 = contract<8, 16> + tree<8>), tile chain
and row sum are used as they are.  What depends on the geometry is restated here:
  * qs_net.9 forward: S = ceil(K / 256) segments of 256 consecutive inputs (K = 64 H4^2), each one contract8; the last one ragged (64 inputs
    at K = 576, 1 600, 3 136, and the ONLY one at K = 64: chunks 4 .. 15 are exact zeros in both operands, accumulators 4 .. 7 stay + 0 and
    tree<8> adds them, which contract8's zero padding restates); joined as sequential sums of runs of eight consecutive segments, ascending,
    the last run shorter, the runs then added in ascending order; then + bias;
  * dW9 / db9: row groups of P = 64 rows (resolution <= 64) or 32; per group the 16-row tiles ascending, one 16-term chain (db: sequential
    sum) per tile, group = chunks added in ascending order from + 0, gradient = groups added in ascending order;
  * g4 = (g_0 W9) [y4 > 0]: one contract8 over the 256 features;
  * dW / db of qs_net.12 / .15 / .18: tile t OF THE CALL goes to slab t mod 4, tiles ascending, gradient = ((slab_0 + slab_1) + slab_2) + slab_3;
  * the convolutions: row m goes to slab m mod min(M, 32); per slab the images of a row group ascending (from + 0), the groups ascending;
    gradient = ((slab_0 + slab_1) + ...).  An image's own contribution (the chunk order inside it, train_conv.h) and the convolutions'
    forward and data gradient are torch's fp32 on the CPU, gated by the emulated activations.
Both oracles (tests/train_enc_g_ref.py) take their gates from the emulated y1..y4 and h1..h3.  Prints every figure and the worst ratio
e_emu / (e_32 + 2 ulp) (the rule allows 4).

Usage:  python tools/emulate_enc_g.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle import synth                              # noqa: E402
import emulate_dec_head as E                          # noqa: E402
from emulate_dec_head_g import join_segments, rows_per_pass      # noqa: E402
import train_enc_g_ref as TEG                         # noqa: E402
from test_fp64_parity import fp64_rule                # noqa: E402

f32 = np.float32
STAGE = 3
CONV_KEYS = TEG.ENC_KEYS[:8]


def convs(w, o, gate_from=None):
    """torch fp32 forward of the four convolutions -> (leaf parameters, [y1..y4] with a graph)"""
    p = {k: torch.tensor(np.array(w['down.' + k])).requires_grad_(True) for k in CONV_KEYS}
    x, ys = torch.tensor(o), []
    for idx in TEG.CONVS:
        x = torch.relu(F.conv2d(x, p[f'qs_net.{idx}.weight'], p[f'qs_net.{idx}.bias'], stride=2))
        ys.append(x)
    return p, ys


def head_forward(w, y4, mk):
    W = [np.asarray(w[f'down.qs_net.{i}.weight'], f32) for i in TEG.DENSE]
    B = [np.asarray(w[f'down.qs_net.{i}.bias'], f32) for i in TEG.DENSE]
    K = y4.shape[1]
    seg = [E.contract8(y4[:, k0:k0 + 256], W[0][:, k0:k0 + 256]) for k0 in range(0, K, 256)]
    x = (np.maximum(join_segments(seg) + B[0][None, :], f32(0)) * mk[0]).astype(f32)
    hs = [x]
    for l in (1, 2):
        x = (np.maximum(E.contract8(x, W[l]) + B[l][None, :], f32(0)) * mk[l]).astype(f32)
        hs.append(x)
    return hs, (E.contract8(x, W[3]) + B[3][None, :]).astype(f32)


def head_backward(w, y4, hs, g_out, R):
    """-> (grads of the eight dense tensors, g4 [M, K])"""
    W = [np.asarray(w[f'down.qs_net.{i}.weight'], f32) for i in TEG.DENSE]
    M, P = y4.shape[0], rows_per_pass(R)
    gate = lambda h: np.where(h > 0, f32(2), f32(0))          # noqa: E731
    grads, g = {}, g_out.astype(f32)
    xs = [y4, hs[0], hs[1], hs[2]]
    for l in (3, 2, 1):
        slabs_w, slabs_b = [None] * 4, [None] * 4
        for t in range((M + 15) // 16):                      # the tile's index in the call, whatever the row group
            r0, r1 = 16 * t, min(16 * t + 16, M)
            cw, cb = E.rows_chain(g[r0:r1], xs[l][r0:r1]), E.rows_sum(g[r0:r1])
            p = t % 4
            slabs_w[p] = cw if slabs_w[p] is None else slabs_w[p] + cw
            slabs_b[p] = cb if slabs_b[p] is None else slabs_b[p] + cb
        sw, sb = slabs_w[0], slabs_b[0]
        for p in range(1, 4):
            if slabs_w[p] is not None:
                sw, sb = sw + slabs_w[p], sb + slabs_b[p]
        idx = TEG.DENSE[l]
        grads[f'qs_net.{idx}.weight'], grads[f'qs_net.{idx}.bias'] = sw, sb
        g = (E.contract8(g, np.ascontiguousarray(W[l].T)) * gate(xs[l])).astype(f32)
    gw = gb = None                                           # qs_net.9 from g = g_0
    for m0 in range(0, M, P):
        aw = np.zeros((256, y4.shape[1]), f32)
        ab = np.zeros(256, f32)
        for r0 in range(m0, min(m0 + P, M), 16):
            r1 = min(r0 + 16, M)
            aw = aw + E.rows_chain(g[r0:r1], y4[r0:r1])
            ab = ab + (np.zeros(256, f32) + E.rows_sum(g[r0:r1]))
        gw, gb = (aw, ab) if gw is None else (gw + aw, gb + ab)
    grads['qs_net.9.weight'], grads['qs_net.9.bias'] = gw, gb
    g4 = (E.contract8(g, np.ascontiguousarray(W[0].T)) * np.where(y4 > 0, f32(1), f32(0))).astype(f32)
    return grads, g4


def conv_backward(p, ys, g4, R):
    """per-image gradients by torch's fp32, joined by the slab and group rules"""
    M, P = g4.shape[0], rows_per_pass(R)
    G = min(M, 32)
    per = []
    for r in range(M):
        sel = torch.zeros_like(ys[3])
        sel[r] = torch.tensor(g4[r]).reshape(ys[3].shape[1:])
        gr = torch.autograd.grad((ys[3] * sel).sum(), [p[k] for k in CONV_KEYS], retain_graph=True)
        per.append([t.numpy().copy() for t in gr])
    out = {}
    for i, k in enumerate(CONV_KEYS):
        slabs = []
        for s in range(G):
            slab = None
            for m0 in range(0, M, P):
                acc = np.zeros_like(per[0][i])
                rows = [r for r in range(m0, min(m0 + P, M)) if (r - m0) % G == s]
                if not rows:
                    continue
                for r in rows:
                    acc = acc + per[r][i]
                slab = acc if slab is None else slab + acc
            slabs.append(slab)
        total = slabs[0]
        for s in slabs[1:]:
            total = total + s
        out[k] = total
    return out


CASES = [((4, 1, 44), M) for M in (1, 2, 5, 17, 33)] + [((3, 3, 32), 2), ((4, 2, 48), 2), ((4, 1, 68), 1), ((3, 3, 84), 2), ((4, 2, 128), 1)]


def main():
    worst, where = 0.0, None
    for geo, M in CASES:
        _, C, R = geo
        w = synth.make_weights(1234, 1.15, *geo)
        o = TEG.inputs(2000 + M, M, C, R)[0]
        gm, gv = TEG.upstream(2000 + M, M)
        mk = [m.numpy() for m in TEG.enc_masks(M, STAGE)]
        p, ys = convs(w, o)
        y4 = ys[3].detach().numpy().reshape(M, -1).copy()
        hs, out = head_forward(w, y4, mk)
        grads, g4 = head_backward(w, y4, hs, np.concatenate([gm, gv], axis=1), R)
        grads.update(conv_backward(p, ys, g4, R))
        gates = tuple(y.detach().numpy() for y in ys) + tuple(hs)
        o32 = TEG.run_encoder(w, o, gm, gv, C, R, STAGE, torch.float32, gates=gates)
        o64 = TEG.run_encoder(w, o, gm, gv, C, R, STAGE, torch.float64, gates=gates)
        rows = [(k, grads[k], o32['grads'][k], o64['grads'][k]) for k in TEG.ENC_KEYS]
        rows += [('mean', out[:, :10], o32['mean'], o64['mean']), ('logvar', out[:, 10:], o32['logvar'], o64['logvar'])]
        rows += [(f'h{i + 1}', hs[i], o32['h'][i], o64['h'][i]) for i in range(3)]
        for name, e, a32, a64 in rows:
            for r in fp64_rule(name, e, a32, a64):
                if r[4] > worst:
                    worst, where = r[4], f'{geo} M={M} {r[0]}'
                print(f'{geo} M={M} {r[0]}: e_emu {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}{"" if r[5] else "  FAILS"}', flush=True)
    print(f'worst ratio {worst:.2f} at {where} (allowed 4)')
    return worst


if __name__ == '__main__':
    torch.set_num_threads(8)
    sys.exit(0 if main() <= 4.0 else 1)
