"""Reference of the decoder tail's backward (csrc/train_dec.hip, loss.grad_decoder_convs): autograd over torch's conv_transpose2d on the
CPU, in a given dtype, for po_net[12:] of the reference's ModelDown (torchmodel.py:119-127) and the binary cross entropy of
compute_loss_down (torchloss.py:45-46), L = scale * sum_r nlogpo1_r.

The ReLUs can take their gates from GIVEN activations: relu(a) is then replaced by a * gate with gate = [y_given > 0] held constant, so
that a pre-activation within rounding of zero, which fp32 and fp64 may see on different sides, does not count as an error of the code
under test (the gate condition itself is checked separately by the GPU tests).  With gates=None the ReLUs are the model's own; in fp32
that reproduces the reference's own po_net[12:] bit for bit (tests/test_train_dec_cpu.py against tests/golden/train_dec_g115.npz)."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ((13, 1), (15, 2), (17, 2), (19, 1))            # (index in po_net, stride)
KEYS = tuple(f'po_net.{i}.{s}' for i, _ in LAYERS for s in ('weight', 'bias'))
P = 92609


def inputs(seed, M):
    """h4 = 2 relu(N(0, 1)) Bernoulli(0.5) [M, 16384], o1 = Bernoulli(0.1) [M, 1, 64, 64], from a seeded generator"""
    g = torch.Generator().manual_seed(seed)
    h4 = 2.0 * torch.relu(torch.randn(M, 16384, generator=g)) * (torch.rand(M, 16384, generator=g) < 0.5).float()
    o1 = (torch.rand(M, 1, 64, 64, generator=g) < 0.1).float()
    return h4.numpy().copy(), o1.numpy().copy()


def run(weights, h4, o1, dtype=torch.float32, scale=None, beta_o=1.0, gates=None):
    """weights: {'down.po_net.13.weight': ...}.  -> dict(nlogpo1 [M], po1, d_h4 [M, 16384], grads {key: array}, y (y1, y2, y3), a (a1..a4)),
    numpy arrays in `dtype`.  scale None = beta_o / M."""
    M = h4.shape[0]
    scale = float(beta_o) / M if scale is None else float(scale)
    params = {k: torch.tensor(np.array(weights['down.' + k])).to(dtype).requires_grad_(True) for k in KEYS}
    x0 = torch.tensor(np.array(h4)).to(dtype).requires_grad_(True)
    o = torch.tensor(np.array(o1)).to(dtype).reshape(M, 1, 64, 64)
    x = x0.reshape(M, 64, 16, 16)
    ys, pre = [], []
    for li, (idx, s) in enumerate(LAYERS):
        a = F.conv_transpose2d(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'], stride=s, padding=1, output_padding=s - 1)
        pre.append(a)
        if li == 3:
            break
        if gates is None:
            x = torch.relu(a)
        else:
            x = a * (torch.as_tensor(np.asarray(gates[li])) > 0).to(dtype).reshape(a.shape)
        ys.append(x)
    p = torch.sigmoid(pre[3])
    bce = o * torch.log(1e-5 + p) + (1 - o) * torch.log(1e-5 + 1 - p)
    nl = -torch.sum(bce, dim=[1, 2, 3])
    (scale * nl.sum()).backward()
    n = lambda t: t.detach().numpy().copy()          # noqa: E731
    return dict(nlogpo1=n(nl), po1=n(p), d_h4=n(x0.grad), grads={k: n(v.grad) for k, v in params.items()}, y=tuple(n(y) for y in ys),
                a=tuple(n(a) for a in pre))
