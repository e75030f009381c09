"""CPU emulation of the fp32 summation orders of csrc/train_dec_head_g.hip, to check the fp64 rule of tests/test_fp64_parity.py on gradient
cases of tests/test_train_dec_head_g_gpu.py before a GPU run.  tools/emulate_dec_head.py with the width of po_net.9 taken from the geometry,
F = 64 B^2; its chain (contract8 = contract<8, 16> + tree<8>), tile chain and row sum are used as they are.  What depends on the geometry is
restated here:
  * d_h3: S = ceil(F / 256) segments of 256 consecutive reference features, the last one ragged (64 features at odd B: its chunks 4 .. 15
    are exact zeros in both operands, which contract8's zero padding restates); joined as sequential sums of runs of eight consecutive
    segments, ascending, the last run shorter, the runs then added in ascending order;
  * dW_3 / db_3: row groups of P = 64 rows (B <= 16) or 32; per group the 16-row tiles ascending, one 16-term chain (db: sequential sum)
    per tile, group = chunks added in ascending order, gradient = groups added in ascending order;
  * dW / db of layers 0..2: tile t OF THE CALL goes to slab t mod 4, tiles ascending, gradient = ((slab_0 + slab_1) + slab_2) + slab_3.
The ConvTranspose2d tail between the emulated forward and backward is torch's fp32 on the CPU (tests/train_dec_g_ref.py).  Both oracles
(tests/train_dec_head_g_ref.py) take their gates from the emulated h1..h4 and that tail's y1..y3.  Prints every figure and the worst ratio
e_emu / (e_32 + 2 ulp) (the rule allows 4).

Usage:  python tools/emulate_dec_head_g.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from oracle import synth                              # noqa: E402
import emulate_dec_head as E                          # noqa: E402
import train_dec_g_ref as TG                          # noqa: E402
import train_dec_head_g_ref as THG                    # noqa: E402
from test_fp64_parity import fp64_rule                # noqa: E402

f32 = np.float32
STAGE = 3


def rows_per_pass(R):
    return 64 if THG.base_of(R) <= 16 else 32


def join_segments(seg):
    """sequential sums of runs of eight consecutive segments, then the runs in ascending order"""
    total = None
    for j0 in range(0, len(seg), 8):
        sm = seg[j0]
        for s in seg[j0 + 1:j0 + 8]:
            sm = sm + s
        total = sm if total is None else total + sm
    return total


def backward(w, s, hs, d_h4, R):
    W = [np.asarray(w[f'down.po_net.{i}.weight'], f32) for i in THG.HEAD]
    M, F, P = s.shape[0], THG.n_feat(R), rows_per_pass(R)
    gate = lambda h: np.where(h > 0, f32(2), f32(0))          # noqa: E731
    g3 = (d_h4.astype(f32) * gate(hs[3])).astype(f32)
    grads = {}
    gw = gb = None
    for m0 in range(0, M, P):
        aw = np.zeros((F, 256), f32)
        ab = np.zeros(F, f32)
        for r0 in range(m0, min(m0 + P, M), 16):
            r1 = min(r0 + 16, M)
            aw = aw + E.rows_chain(g3[r0:r1], hs[2][r0:r1])
            ab = ab + (np.zeros(F, f32) + E.rows_sum(g3[r0:r1]))
        gw, gb = (aw, ab) if gw is None else (gw + aw, gb + ab)
    grads['po_net.9.weight'], grads['po_net.9.bias'] = gw, gb
    W3T = np.ascontiguousarray(W[3].T)
    S = (F + 255) // 256
    seg = [E.contract8(g3[:, 256 * i:256 * (i + 1)], W3T[:, 256 * i:256 * (i + 1)]) for i in range(S)]
    g = (join_segments(seg) * gate(hs[2])).astype(f32)
    xs = [s.astype(f32), hs[0], hs[1]]
    for l in (2, 1, 0):
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
        idx = THG.HEAD[l]
        grads[f'po_net.{idx}.weight'], grads[f'po_net.{idx}.bias'] = sw, sb
        nxt = E.contract8(g, np.ascontiguousarray(W[l].T))
        g = (nxt * gate(xs[l])).astype(f32) if l > 0 else nxt
    return grads, g


CASES = [((4, 1, 36), M) for M in (1, 2, 5, 33)] + [((3, 3, 32), 2)]


def main():
    worst = 0.0
    for geo, M in CASES:
        _, C, R = geo
        w = synth.make_weights(1234, 1.15, *geo)
        s, o1 = THG.inputs(1000 + M, M, C, R)
        mk = THG.masks(M, R, STAGE)
        hs = E.forward(w, s, [m.numpy() for m in mk])
        t = TG.run(w, hs[3], o1, C, R, torch.float32, scale=1.0 / M)
        grads, d_s = backward(w, s, hs, t['d_h4'], R)
        gates = tuple(hs) + tuple(t['y'])
        o32 = THG.run(w, s, o1, C, R, STAGE, torch.float32, gates=gates)
        o64 = THG.run(w, s, o1, C, R, STAGE, torch.float64, gates=gates)
        rows = [(k, grads[k], o32['grads'][k], o64['grads'][k]) for k in THG.HEAD_KEYS]
        rows.append(('d_s', d_s, o32['d_s'], o64['d_s']))
        rows += [(f'h{i + 1}', hs[i], o32['h'][i], o64['h'][i]) for i in range(4)]
        for name, e, a32, a64 in rows:
            for r in fp64_rule(name, e, a32, a64):
                worst = max(worst, r[4])
                print(f'{geo} M={M} {r[0]}: e_emu {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}{"" if r[5] else "  FAILS"}', flush=True)
    print(f'worst ratio {worst:.2f} (allowed 4)')


if __name__ == '__main__':
    torch.set_num_threads(8)
    main()
