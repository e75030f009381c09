"""The premise of layer 2 of k_dec_a / k_dec_a_s (decoder.hip f22_l2, kernels.h f22_*): ConvTranspose2d(64, 64, 3, s2, p1, op1) on the
16 x 16 layer-1 image computed by per-parity minimal filtering F(2, 2) in fp32 -- 16 weight matrices formed in fp64 and rounded once,
9 input views per 2 x 2 input block (x_2 = 0 beyond the last row / column), 25 products added into the block's 4 x 4 outputs -- is as
accurate as the direct form.  Restated in torch on the CPU (tests/f22_ref.py) in the kernel's association (the bias first; group by group, direct
products chained into their output, the others added into theirs in chain order; torch contracts the 64 channels of a product in its
own order): exact in fp64, and within the fp64 parity rule of the direct fp32 error on every weight family, before and after the ReLU
(tests/test_fp64_parity.py: e <= ALPHA * e_32 + BETA ulp).  The maths is that of ConvT3 (tests/test_winograd_convt3.py) on 8 x 8 blocks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f22_ref import GROUPS, OUTS, VIEW, WT, f22_convt
from oracle import synth

ALPHA, BETA = 4.0, 8.0

def layer_input(weights, n, seed):
    """ConvT2 inputs of the family's regime: the decoder's post-ReLU ConvT1 activations for random latents (dropout-free, so scaled by 2 on half)"""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(n, 14, generator=gen, dtype=torch.float64)
    for idx in (0, 3, 6, 9):
        w = torch.as_tensor(np.asarray(weights[f'down.po_net.{idx}.weight']), dtype=torch.float64)
        bias = torch.as_tensor(np.asarray(weights[f'down.po_net.{idx}.bias']), dtype=torch.float64)
        h = F.relu(F.linear(h[:, :w.shape[1]], w, bias))
        h = h * (torch.rand(h.shape, generator=gen, dtype=torch.float64) < 0.5) * 2.0
    h = h.reshape(n, 64, 16, 16)
    w = torch.as_tensor(np.asarray(weights['down.po_net.13.weight']), dtype=torch.float64)
    bias = torch.as_tensor(np.asarray(weights['down.po_net.13.bias']), dtype=torch.float64)
    return F.relu(F.conv_transpose2d(h, w, bias, stride=1, padding=1)).float()


FAMILIES = ['control'] + list(synth.STRESS_FAMILIES)


def family_weights(name):
    return synth.make_weights(1234, 1.15) if name == 'control' else synth.stress_weights(name)


def ct2(w, dtype):
    W = torch.as_tensor(np.asarray(w['down.po_net.15.weight']), dtype=dtype)
    b = torch.as_tensor(np.asarray(w['down.po_net.15.bias']), dtype=dtype)
    return W, b


def test_schedule_covers_every_product_once():
    prods = [p for g in GROUPS for p in g]
    assert sorted(prods) == [(r, c) for r in range(5) for c in range(5)]
    # every one of the 16 weight matrices is used, and the 1D identity holds for all four outputs
    assert sorted({(WT[r], WT[c]) for r, c in prods}) == [(a, b) for a in range(4) for b in range(4)]
    x0, x1, x2 = 0.3, -1.7, 2.9
    g = [0.11, -0.53, 1.9]
    d = [x0 - x1, x1, x2 - x1]
    wv = [g[1], g[2], g[0] + g[2], g[0]]
    o = [0.0] * 4
    for p in range(5):
        for k in OUTS[p]:
            o[k] += d[VIEW[p]] * wv[WT[p]]
    assert np.allclose(o, [x0 * g[1], x0 * g[2] + x1 * g[0], x1 * g[1], x1 * g[2] + x2 * g[0]], rtol=0, atol=1e-14)


def test_f22_restatement_is_exact_in_fp64():
    w = family_weights('control')
    W, b = ct2(w, torch.float64)
    x = layer_input(w, 4, 11).double()
    assert x.shape[1:] == (64, 16, 16) and W.shape == (64, 64, 3, 3)
    x[:, :, -1, :] += 1.0; x[:, :, :, -1] += 1.0; x[:, :, 0, :] += 1.0; x[:, :, :, 0] += 1.0     # active last row / column: x2 = 0 matters
    ref = F.conv_transpose2d(x, W, b, stride=2, padding=1, output_padding=1)
    got = f22_convt(x, W, b, torch.float64)
    assert got.shape == ref.shape == (4, 64, 32, 32)
    assert torch.allclose(got, ref, rtol=0, atol=1e-12 * float(ref.abs().max()))


@pytest.mark.parametrize('family', FAMILIES)
def test_f22_fp32_error_is_within_the_fp64_rule(family):
    w = family_weights(family)
    W, b = ct2(w, torch.float32)
    x = layer_input(w, 8, 5)
    ref = F.conv_transpose2d(x.double(), W.double(), b.double(), stride=2, padding=1, output_padding=1)
    direct = F.conv_transpose2d(x, W, b, stride=2, padding=1, output_padding=1).double()
    f22 = f22_convt(x, W, b, torch.float32).double()
    e32 = float((direct - ref).abs().max())
    ef = float((f22 - ref).abs().max())
    ulp = float(np.spacing(np.float32(float(ref.abs().max()))))
    print(f'{family}: y2 max|err| F(2,2) {ef:.3e}, direct {e32:.3e} (ratio {ef / e32:.2f}), ulp {ulp:.3e}')
    assert ef <= ALPHA * e32 + BETA * ulp, (family, ef, e32, ulp)
    # and after the layer's ReLU, the quantity ConvT3 reads
    er = float((F.relu(f22) - F.relu(ref)).abs().max())
    er32 = float((F.relu(direct) - F.relu(ref)).abs().max())
    assert er <= ALPHA * er32 + BETA * ulp, (family, er, er32, ulp)
