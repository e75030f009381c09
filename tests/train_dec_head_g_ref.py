"""tests/train_dec_head_ref.py generalised to (channels, resolution): the reference of the whole decoder's backward at every admitted geometry
(csrc/train_dec_head_g.hip + csrc/train_dec_g.hip, loss.grad_decoder_g) -- autograd on the CPU, in a given dtype, over the dense head
po_net.0 / .3 / .6 / .9 of the reference's ModelDown (torchmodel.py:107-118) as F.linear with the Philox dropout masks of
oracle.efe_oracle.PhiloxNoise applied as multiplications (tag TAG_DEC + layer; the last mask, over the 64 B^2 features of po_net.9, in the
engine's NHWC keying, fc4_perm), followed by the ConvTranspose2d tail and the binary cross entropy exactly as tests/train_dec_g_ref.py
states them, L = scale * sum_r nlogpo1_r.  B = R / 4, or R / 2 = 16 at R = 32.

Same `gates=` override over the seven gated layers as train_dec_head_ref.run: relu(a) * mask becomes a * 2 [h_given > 0] in the head and
relu(a) becomes a * [y_given > 0] in the tail.  At (1, 64) the function is train_dec_head_ref.run, bit for bit
(tests/test_train_dec_head_g_cpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F

import train_dec_g_ref as TG
from oracle import philox as PX
from oracle.efe_oracle import PhiloxNoise

HEAD = (0, 3, 6, 9)                                      # indices in po_net
HEAD_KEYS = tuple(f'po_net.{i}.{s}' for i in HEAD for s in ('weight', 'bias'))
KEYS = HEAD_KEYS + TG.KEYS                               # parameters() order
PASS_FE_DOWN = 12
SEED = 7                                                 # the engine seed of the GPU tests
base_of = TG.base_of


def n_feat(R):
    return 64 * base_of(R) ** 2


def param_count(C, R):
    return 134400 + 257 * n_feat(R) + TG.param_count(C)


def inputs(seed, M, C, R):
    """s = N(0, 1) [M, 10], o1 = Bernoulli(0.1) [M, C, R, R], from a seeded generator"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(M, 10, generator=g)
    o1 = (torch.rand(M, C, R, R, generator=g) < 0.1).float()
    return s.numpy().copy(), o1.numpy().copy()


def masks(M, R, stage, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """the four keep masks (x 2) of the head, float32 [M, 256] x 3 and [M, 64 B^2] in the reference's feature order"""
    nz = PhiloxNoise(seed)
    return tuple(nz.mask(PX.TAG_DEC + li, M, n_feat(R) if li == 3 else 256, pass_, sample, stage, row_offset, fc4_perm=(li == 3))
                 for li in range(4))


def run(weights, s, o1, C, R, stage, dtype=torch.float32, scale=None, beta_o=1.0, gates=None, seed=SEED, pass_=PASS_FE_DOWN, sample=0,
        row_offset=0):
    """weights: {'down.po_net.0.weight': ...}; gates: None or (h1, h2, h3, h4, y1, y2, y3).  -> dict(nlogpo1 [M], po1 [M,C,R,R], d_s [M, 10],
    d_h4 [M, 64 B^2], grads {key: array}, h (h1..h4), y (y1..y3), a_head (the head's four pre-activations), a (the tail's a1..a4),
    masks (the four keep masks x 2)), numpy arrays in `dtype`.  scale None = beta_o / M."""
    M, B = s.shape[0], base_of(R)
    scale = float(beta_o) / M if scale is None else float(scale)
    params = {k: torch.tensor(np.array(weights['down.' + k])).to(dtype).requires_grad_(True) for k in KEYS}
    x0 = torch.tensor(np.array(s)).to(dtype).requires_grad_(True)
    o = torch.tensor(np.array(o1)).to(dtype).reshape(M, C, R, R)
    mk = masks(M, R, stage, seed, pass_, sample, row_offset)
    x, hs, pre_h = x0, [], []
    for li, idx in enumerate(HEAD):
        a = F.linear(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'])
        pre_h.append(a)
        if gates is None:
            x = torch.relu(a) * mk[li].to(dtype)
        else:
            x = a * (2.0 * (torch.as_tensor(np.asarray(gates[li])) > 0).to(dtype).reshape(a.shape))
        if li == 3:
            x.retain_grad()
        hs.append(x)
    h4 = x
    x = h4.reshape(M, 64, B, B)
    ys, pre = [], []
    for li, (idx, st) in enumerate(TG.layers(R)):
        a = F.conv_transpose2d(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'], stride=st, padding=1, output_padding=st - 1)
        pre.append(a)
        if li == 3:
            break
        if gates is None:
            x = torch.relu(a)
        else:
            x = a * (torch.as_tensor(np.asarray(gates[4 + li])) > 0).to(dtype).reshape(a.shape)
        ys.append(x)
    p = torch.sigmoid(pre[3])
    bce = o * torch.log(1e-5 + p) + (1 - o) * torch.log(1e-5 + 1 - p)
    nl = -torch.sum(bce, dim=[1, 2, 3])
    (scale * nl.sum()).backward()
    n = lambda t: t.detach().numpy().copy()          # noqa: E731
    return dict(nlogpo1=n(nl), po1=n(p), d_s=n(x0.grad), d_h4=n(h4.grad), grads={k: n(v.grad) for k, v in params.items()},
                h=tuple(n(h) for h in hs), y=tuple(n(y) for y in ys), a_head=tuple(n(a) for a in pre_h), a=tuple(n(a) for a in pre),
                masks=tuple(m.numpy() for m in mk))
