"""The premise of k_dec_a's layer 1 (decoder.hip wino_l1): ConvTranspose2d(64, 64, 3, s1, p1) computed as Winograd F(2x2, 3x3) in fp32 --
weights transformed in fp64 and rounded once, input transform, 16 xi-GEMMs and output transform in fp32 -- is as accurate as the direct
form.  Restated here in torch on the CPU: exact in fp64, and within the fp64 parity rule's ALPHA of the direct fp32 error on every weight
family (tests/test_fp64_parity.py: e <= ALPHA * e_32 + BETA ulp)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth

ALPHA, BETA = 4.0, 8.0
BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def wino_convt1(x, W, b, dtype):
    """x [N, 64, 16, 16], W [Cin, Cout, 3, 3] (ConvTranspose2d layout), b [Cout] -> [N, Cout, 16, 16] in `dtype`, in the kernel's order:
    out = bias, then + AT[r][a] AT[c][b] M_xi for xi = 4a + b ascending"""
    g = torch.flip(W.double(), dims=(2, 3)).permute(1, 0, 2, 3)           # correlation kernel [Cout, Cin, u, v]
    Gd = torch.tensor(G, dtype=torch.float64)
    U = torch.einsum('au,oiuv,bv->abio', Gd, g, Gd).to(dtype)                # [a, b, Cin, Cout], rounded once
    xp = F.pad(x.to(dtype), (1, 1, 1, 1))                                     # 18 x 18
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                    # [N, Cin, 8, 8, 4, 4]: tile (ty, tx), d[i][jj]
    # B^T d B with the kernel's association: row a of B^T d = d[i0] + s d[i1], then the same over the columns
    idx = [(0, 2, -1.0), (1, 2, 1.0), (2, 1, -1.0), (1, 3, -1.0)]
    rows = torch.stack([d[..., i0, :] + s * d[..., i1, :] for i0, i1, s in idx], dim=-2)           # [..., a, jj]
    V = torch.stack([rows[..., j0] + s * rows[..., j1] for j0, j1, s in idx], dim=-1)              # [..., a, b]
    out = b.to(dtype).view(1, -1, 1, 1, 1, 1).expand(x.shape[0], -1, 8, 8, 2, 2).clone()
    for a in range(4):
        for bb in range(4):
            M = torch.einsum('io,nihw->nohw', U[a, bb], V[..., a, bb])
            for r in range(2):
                for c in range(2):
                    cf = AT[r][a] * AT[c][bb]
                    if cf:
                        out[..., r, c] = out[..., r, c] + cf * M
    return out.permute(0, 1, 2, 4, 3, 5).reshape(x.shape[0], -1, 16, 16)


def layer_input(weights, n, seed):
    """ConvT1 inputs of the family's regime: the fc head's post-ReLU activations for random latents (dropout-free, so scaled by 2 on half)"""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(n, 14, generator=gen, dtype=torch.float64)
    for idx in (0, 3, 6, 9):
        w = torch.as_tensor(np.asarray(weights[f'down.po_net.{idx}.weight']), dtype=torch.float64)
        bias = torch.as_tensor(np.asarray(weights[f'down.po_net.{idx}.bias']), dtype=torch.float64)
        h = F.relu(F.linear(h[:, :w.shape[1]], w, bias))
        h = h * (torch.rand(h.shape, generator=gen, dtype=torch.float64) < 0.5) * 2.0
    return h.reshape(n, 64, 16, 16).float()


FAMILIES = ['control'] + list(synth.STRESS_FAMILIES)


def family_weights(name):
    return synth.make_weights(1234, 1.15) if name == 'control' else synth.stress_weights(name)


def test_winograd_restatement_is_exact_in_fp64():
    w = family_weights('control')
    W = torch.as_tensor(np.asarray(w['down.po_net.13.weight']), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(w['down.po_net.13.bias']), dtype=torch.float64)
    x = layer_input(w, 4, 11).double()
    x[:, :, 0, :] += 1.0; x[:, :, -1, :] += 1.0; x[:, :, :, 0] += 1.0; x[:, :, :, -1] += 1.0     # active borders: the padding edges matter
    ref = F.conv_transpose2d(x, W, b, stride=1, padding=1)
    got = wino_convt1(x, W, b, torch.float64)
    assert torch.allclose(got, ref, rtol=0, atol=1e-12 * float(ref.abs().max()))


@pytest.mark.parametrize('family', FAMILIES)
def test_winograd_fp32_error_is_within_the_fp64_rule(family):
    w = family_weights(family)
    W = torch.as_tensor(np.asarray(w['down.po_net.13.weight']), dtype=torch.float32)
    b = torch.as_tensor(np.asarray(w['down.po_net.13.bias']), dtype=torch.float32)
    x = layer_input(w, 16, 5)
    ref = F.conv_transpose2d(x.double(), W.double(), b.double(), stride=1, padding=1)
    direct = F.conv_transpose2d(x, W, b, stride=1, padding=1).double()
    wino = wino_convt1(x, W, b, torch.float32).double()
    e32 = float((direct - ref).abs().max())
    ew = float((wino - ref).abs().max())
    ulp = float(np.spacing(np.float32(float(ref.abs().max()))))
    assert ew <= ALPHA * e32 + BETA * ulp, (family, ew, e32, ulp)
    # and after the layer's ReLU, the quantity the next layer reads
    assert float((F.relu(wino) - F.relu(ref)).abs().max()) <= ALPHA * float((F.relu(direct) - F.relu(ref)).abs().max()) + BETA * ulp
