"""The per-parity F(2, 2) form of a ConvTranspose2d(Cin, Cout, 3, s2, p1, op1) (decoder.hip f22_contract, kernels.h f22_*), restated
in torch on the CPU in the kernels' association: 16 weight matrices formed in fp64 and rounded once, 9 input views per 2 x 2 input block
(x_2 = 0 beyond the last row / column), 25 products added into the block's 4 x 4 outputs -- the bias first; group by group, direct
products chained into their output, the others added into theirs in chain order (torch contracts the channels of a product in its own
order).  Shared by tests/test_f22_convt2.py (ConvT2, 8 x 8 blocks) and tests/test_winograd_convt3.py (ConvT3, 16 x 16 blocks)."""
import torch
import torch.nn.functional as F

# 1D products P1..P5: view (d0 = x0 - x1, d1 = x1, d2 = x2 - x1), weight (g1, g2, g0 + g2, g0), outputs of the block
VIEW = [0, 1, 0, 1, 2]
WT = [0, 0, 1, 2, 3]
OUTS = [(0,), (0, 2), (1,), (1, 3), (3,)]
CW = [[0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 0, 0]]            # tap coefficients of each weight
# the schedule of f22_contract: groups of (row product, column product)
GROUPS = [[(0, 0), (0, 2), (2, 0), (2, 2)], [(0, 1), (0, 3), (2, 1), (2, 3)], [(1, 0), (1, 2), (3, 0), (3, 2)],
          [(1, 1), (1, 3), (3, 1), (3, 3)], [(1, 4), (3, 4), (4, 1), (4, 3), (4, 4)], [(0, 4), (2, 4), (4, 0), (4, 2)]]


def f22_weights(W):
    """W [Cin, Cout, 3, 3] -> U [4, 4, Cin, Cout] in fp64 (rounded by the caller): U[wr][wc] = sum cw[wr][kh] cw[wc][kw] W[..., kh, kw]"""
    C = torch.tensor(CW, dtype=torch.float64)
    return torch.einsum('ah,bw,iohw->abio', C, C, W.double())


def f22_convt(x, W, b, dtype):
    """x [N, Cin, H, H] (H even), W [Cin, Cout, 3, 3], b [Cout] -> [N, Cout, 2H, 2H] in `dtype`, in f22_contract's order of operations"""
    H = x.shape[-1]
    U = f22_weights(W).to(dtype)
    xp = F.pad(x.to(dtype), (0, 1, 0, 1))                                    # x[H] = 0 (row and column)
    nb = xp.unfold(2, 3, 2).unfold(3, 3, 2)                                   # [N, Cin, H/2, H/2, 3, 3]: block (u, v), x[i][jj]

    def cview(i, vb):
        return (nb[..., i, 0] - nb[..., i, 1]) if vb == 0 else (nb[..., i, 1] if vb == 1 else nb[..., i, 2] - nb[..., i, 1])

    def view(va, vb):
        return (cview(0, vb) - cview(1, vb)) if va == 0 else (cview(1, vb) if va == 1 else cview(2, vb) - cview(1, vb))

    out = [[None] * 4 for _ in range(4)]
    bias = b.to(dtype).view(1, -1, 1, 1)

    def add(r, c, m):
        out[r][c] = (bias + m) if out[r][c] is None else out[r][c] + m

    for grp in GROUPS:
        temps = []
        for pr, pc in grp:
            M = torch.einsum('io,nihw->nohw', U[WT[pr], WT[pc]], view(VIEW[pr], VIEW[pc]))
            if len(OUTS[pr]) == 1 and len(OUTS[pc]) == 1:                     # direct: chained into its output during the group
                add(OUTS[pr][0], OUTS[pc][0], M)
            else:
                temps.append((pr, pc, M))
        for pr, pc, M in temps:                                               # then the temporaries, in chain order
            for r in OUTS[pr]:
                for c in OUTS[pc]:
                    add(r, c, M)
    y = torch.stack([torch.stack(row, -1) for row in out], -2)                # [N, Cout, H/2, H/2, 4 (r), 4 (c)]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(x.shape[0], -1, 2 * H, 2 * H)
