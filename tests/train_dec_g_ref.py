"""tests/train_dec_ref.py generalised to (channels, resolution): the reference of the decoder tail's backward at every admitted geometry
(csrc/train_dec_g.hip, loss.grad_decoder_convs_g) -- autograd over torch's conv_transpose2d on the CPU in a given dtype, for po_net[12:] of
the reference's ModelDown (torchmodel.py:119-127) and the binary cross entropy of compute_loss_down (torchloss.py:45-46),
L = scale * sum_r nlogpo1_r.  The third layer's stride / output_padding follow the reference's last_strides (torchmodel.py:77-80): 1 / 0
at resolution 32, where the decoder's base grid is res / 2, else 2 / 1 and res / 4.  Same `gates=` override as train_dec_ref.run: relu(a)
becomes a * [y_given > 0].  At (1, 64) the function is train_dec_ref.run, bit for bit (tests/test_train_dec_g_cpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F

KEYS = tuple(f'po_net.{i}.{s}' for i in (13, 15, 17, 19) for s in ('weight', 'bias'))


def base_of(R):
    return R // 2 if R == 32 else R // 4


def layers(R):
    """(index in po_net, stride)"""
    return ((13, 1), (15, 2), (17, 1 if R == 32 else 2), (19, 1))


def param_count(C):
    return 92320 + 289 * C


def inputs(seed, M, C, R):
    """h4 = 2 relu(N(0, 1)) Bernoulli(0.5) [M, 64 B B], o1 = Bernoulli(0.1) [M, C, R, R], from a seeded generator"""
    n = 64 * base_of(R) ** 2
    g = torch.Generator().manual_seed(seed)
    h4 = 2.0 * torch.relu(torch.randn(M, n, generator=g)) * (torch.rand(M, n, generator=g) < 0.5).float()
    o1 = (torch.rand(M, C, R, R, generator=g) < 0.1).float()
    return h4.numpy().copy(), o1.numpy().copy()


def run(weights, h4, o1, C, R, dtype=torch.float32, scale=None, beta_o=1.0, gates=None):
    """weights: {'down.po_net.13.weight': ...}.  -> dict(nlogpo1 [M], po1 [M,C,R,R], d_h4 [M, 64 B B], grads {key: array}, y (y1, y2, y3),
    a (a1..a4)), numpy arrays in `dtype`.  scale None = beta_o / M."""
    M, B = h4.shape[0], base_of(R)
    scale = float(beta_o) / M if scale is None else float(scale)
    params = {k: torch.tensor(np.array(weights['down.' + k])).to(dtype).requires_grad_(True) for k in KEYS}
    x0 = torch.tensor(np.array(h4)).to(dtype).requires_grad_(True)
    o = torch.tensor(np.array(o1)).to(dtype).reshape(M, C, R, R)
    x = x0.reshape(M, 64, B, B)
    ys, pre = [], []
    for li, (idx, s) in enumerate(layers(R)):
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
