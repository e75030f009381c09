"""Reference of the gradient of F_down for all of ModelDown (csrc/train_enc.hip + csrc/train_dec_head.hip + csrc/train_dec.hip,
loss.grad_encoder / loss.grad_down): autograd on the CPU, in a given dtype, over the reference's compute_loss_down (torchloss.py:39-63)
restated with F.conv2d / F.linear for qs_net (torchmodel.py:84-104, qs_net.9.weight [256][576]), the Philox dropout masks of
oracle.efe_oracle.PhiloxNoise applied as multiplications (tag TAG_ENC + layer for the encoder, TAG_DEC + layer for the decoder), the
injected or Philox normal of the sample, and the decoder exactly as tests/train_dec_head_ref.py states it (its keys, masks and layer
tables are imported).  The loss is F_down.mean(); ps1_mean, ps1_logvar and omega are constants.

The fourteen gated layers can take their gates from GIVEN activations (gates = (y1..y4, h1..h3) of the encoder, then (h1..h4, y1..y3) of
the decoder; either half may be None): relu(a) becomes a * [y_given > 0] and relu(a) * mask becomes a * 2 [h_given > 0], held constant,
so that a pre-activation within rounding of zero, which fp32 and fp64 may see on different sides, does not count as an error of the code
under test (the gate condition itself is checked separately by the GPU tests).  With gates=None the ReLUs and masks are the model's own;
in fp32 that reproduces the reference's own compute_loss_down + F.mean().backward() bit for bit (tests/test_train_down_cpu.py against
tests/golden/train_down_g115.npz)."""
import numpy as np
import torch
import torch.nn.functional as F

import train_dec_head_ref as TH
import train_dec_ref as TD
from oracle import philox as PX
from oracle.efe_oracle import PhiloxNoise

CONVS = (0, 2, 4, 6)                                     # indices in qs_net
DENSE = (9, 12, 15, 18)
ENC_KEYS = tuple(f'qs_net.{i}.{s}' for i in CONVS + DENSE for s in ('weight', 'bias'))
KEYS = ENC_KEYS + TH.KEYS                                # parameters() order of ModelDown
P_ENC = 349428
P = P_ENC + TH.P                                         # 4 787 125
PASS_FE_DOWN = TH.PASS_FE_DOWN
SEED = TH.SEED


def inputs(seed, M):
    """o1 of train_dec_head_ref.inputs(seed, M); ps1_mean, ps1_logvar = 0.5 N(0, 1) [M, 10]; omega per row in [1.5, 2.5]"""
    _, o1 = TH.inputs(seed, M)
    g = torch.Generator().manual_seed(seed + 50000)
    pm = 0.5 * torch.randn(M, 10, generator=g)
    pv = 0.5 * torch.randn(M, 10, generator=g)
    om = 1.5 + torch.rand(M, generator=g)
    return o1, pm.numpy().copy(), pv.numpy().copy(), om.numpy().copy()


def upstream(seed, M):
    """an upstream pair for grad_encoder: N(0, 1) / M, [M, 10] each"""
    g = torch.Generator().manual_seed(seed + 70000)
    return (torch.randn(M, 10, generator=g) / M).numpy().copy(), (torch.randn(M, 10, generator=g) / M).numpy().copy()


def enc_masks(M, stage, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """the three keep masks (x 2) of the encoder's head, float32 [M, 256] each"""
    nz = PhiloxNoise(seed)
    return tuple(nz.mask(PX.TAG_ENC + li, M, 256, pass_, sample, stage, row_offset) for li in range(3))


def normals(M, stage, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """the normals of the sample, float32 [M, 10]"""
    return PhiloxNoise(seed).eps(M, 10, pass_, sample, stage, row_offset)


def _params(weights, keys, dtype):
    return {k: torch.tensor(np.array(weights['down.' + k])).to(dtype).requires_grad_(True) for k in keys}


def _gate(a, given, dtype, keep):
    return a * (keep * (torch.as_tensor(np.asarray(given)) > 0).to(dtype).reshape(a.shape))


def encode(params, o, mk, dtype, gates=None):
    """-> (out [M, 20], ys (y1..y4), hs (h1..h3), pre-activations of the four convolutions, of the three gated dense layers)"""
    x, ys, hs, pre_c, pre_d = o, [], [], [], []
    for li, idx in enumerate(CONVS):
        a = F.conv2d(x, params[f'qs_net.{idx}.weight'], params[f'qs_net.{idx}.bias'], stride=2)
        pre_c.append(a)
        x = torch.relu(a) if gates is None else _gate(a, gates[li], dtype, 1.0)
        ys.append(x)
    x = x.flatten(1)
    for li, idx in enumerate(DENSE):
        a = F.linear(x, params[f'qs_net.{idx}.weight'], params[f'qs_net.{idx}.bias'])
        if li == 3:
            return a, ys, hs, pre_c, pre_d
        pre_d.append(a)
        x = torch.relu(a) * mk[li].to(dtype) if gates is None else _gate(a, gates[4 + li], dtype, 2.0)
        hs.append(x)


def decode(params, s, o, mk, dtype, gates=None):
    """train_dec_head_ref.run's forward on a tensor s that carries a graph -> (p, nlogpo1 [M], hs (h1..h4), ys (y1..y3), head pre-activations,
    tail pre-activations)"""
    M = s.shape[0]
    x, hs, pre_h = s, [], []
    for li, idx in enumerate(TH.HEAD):
        a = F.linear(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'])
        pre_h.append(a)
        x = torch.relu(a) * mk[li].to(dtype) if gates is None else _gate(a, gates[li], dtype, 2.0)
        hs.append(x)
    x = x.reshape(M, 64, 16, 16)
    ys, pre = [], []
    for li, (idx, st) in enumerate(TD.LAYERS):
        a = F.conv_transpose2d(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'], stride=st, padding=1, output_padding=st - 1)
        pre.append(a)
        if li == 3:
            break
        x = torch.relu(a) if gates is None else _gate(a, gates[4 + li], dtype, 1.0)
        ys.append(x)
    p = torch.sigmoid(pre[3])
    bce = o * torch.log(1e-5 + p) + (1 - o) * torch.log(1e-5 + 1 - p)
    return p, torch.sum(bce, dim=[1, 2, 3]), hs, ys, pre_h, pre


def _n(t):
    return t.detach().numpy().copy()


def _enc_out(out, ys, hs, pre_c, pre_d, mk):
    return dict(y=tuple(_n(y) for y in ys), h=tuple(_n(h) for h in hs), a_conv=tuple(_n(a) for a in pre_c), a_dense=tuple(_n(a) for a in pre_d),
                enc_masks=tuple(m.numpy() for m in mk))


def run_encoder(weights, o, d_mean, d_logvar, stage, dtype=torch.float32, gates=None, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """the encoder's vector-Jacobian product for the upstream pair -> dict(mean, logvar [M, 10], grads {key: array}, y, h, a_conv, a_dense,
    enc_masks), numpy arrays in `dtype`"""
    M = o.shape[0]
    params = _params(weights, ENC_KEYS, dtype)
    x0 = torch.tensor(np.array(o)).to(dtype).reshape(M, 1, 64, 64)
    mk = enc_masks(M, stage, seed, pass_, sample, row_offset)
    out, ys, hs, pre_c, pre_d = encode(params, x0, mk, dtype, gates)
    mean, logvar = torch.split(out, 10, dim=1)
    gm, gv = (torch.tensor(np.array(g)).to(dtype).reshape(M, 10) for g in (d_mean, d_logvar))
    ((mean * gm).sum() + (logvar * gv).sum()).backward()
    return dict(mean=_n(mean), logvar=_n(logvar), grads={k: _n(v.grad) for k, v in params.items()}, **_enc_out(out, ys, hs, pre_c, pre_d, mk))


def run(weights, o1, ps1_mean, ps1_logvar, omega, stage, dtype=torch.float32, gamma=0.5, beta_s=1.0, beta_o=1.0, gates=None, dec_gates=None,
        eps=None, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """compute_loss_down and F.mean().backward().  omega: [M] or a number; eps: None (the Philox normals) or [M, 10].  -> dict(F_down,
    nlogpo1, kl_s, kl_naive [M], po1, qs1, mean, logvar, g_mean, g_logvar, d_s (the gradient at qs1) [M, 10], grads {32 keys}, the encoder's y / h / a_conv / a_dense /
    enc_masks, and the decoder's dec_h, dec_y, dec_a_head, dec_a, dec_masks), numpy arrays in `dtype`"""
    M = o1.shape[0]
    params = _params(weights, KEYS, dtype)
    o = torch.tensor(np.array(o1)).to(dtype).reshape(M, 1, 64, 64)
    mk = enc_masks(M, stage, seed, pass_, sample, row_offset)
    dmk = TH.masks(M, stage, seed, pass_, sample, row_offset)
    out, ys, hs, pre_c, pre_d = encode(params, o, mk, dtype, gates)
    mean, logvar = torch.split(out, 10, dim=1)
    mean.retain_grad()
    logvar.retain_grad()
    e = torch.as_tensor(np.asarray(eps, dtype=np.float32)) if eps is not None else normals(M, stage, seed, pass_, sample, row_offset)
    qs1 = e.to(dtype).reshape(M, 10) * torch.exp(logvar * 0.5) + mean
    qs1.retain_grad()
    p, logpo1, dhs, dys, dpre_h, dpre = decode(params, qs1, o, dmk, dtype, dec_gates)
    w = torch.as_tensor(np.asarray(omega, dtype=np.float32)).to(dtype).reshape(-1, 1)
    if w.numel() == 1:
        w = w.expand(M, 1)
    pm, pv = (torch.tensor(np.array(t)).to(dtype).reshape(M, 10) for t in (ps1_mean, ps1_logvar))
    zero = torch.tensor(0.0, dtype=dtype)

    def kl(mu1, lv1, mu2, lv2):          # torchutils.py:7-8
        return 0.5 * (lv2 - torch.log(w) - lv1) + (torch.exp(lv1) + torch.square(mu1 - mu2)) / (2.0 * torch.exp(lv2) / w) - 0.5
    kl_naive = torch.sum(kl(mean, logvar, zero, zero), dim=1)
    kl_s = torch.sum(kl(mean, logvar, pm, pv), dim=1)
    g32 = torch.tensor(gamma, dtype=torch.float32)           # the branches compare in fp32, whatever the dtype of the run
    ga, bs, bo = (torch.tensor(float(np.float32(v)), dtype=dtype) for v in (gamma, beta_s, beta_o))
    if g32 <= 0.05:
        Fd = -bo * logpo1 + bs * kl_naive
    elif g32 >= 0.95:
        Fd = -bo * logpo1 + bs * kl_s
    else:
        Fd = -bo * logpo1 + bs * (ga * kl_s + (1.0 - ga) * kl_naive)
    Fd.mean().backward()
    return dict(F_down=_n(Fd), nlogpo1=_n(-logpo1), kl_s=_n(kl_s), kl_naive=_n(kl_naive), po1=_n(p), qs1=_n(qs1), mean=_n(mean), logvar=_n(logvar),
                g_mean=_n(mean.grad), g_logvar=_n(logvar.grad), d_s=_n(qs1.grad), grads={k: _n(v.grad) for k, v in params.items()},
                dec_h=tuple(_n(h) for h in dhs), dec_y=tuple(_n(y) for y in dys), dec_a_head=tuple(_n(a) for a in dpre_h),
                dec_a=tuple(_n(a) for a in dpre), dec_masks=tuple(m.numpy() for m in dmk), **_enc_out(out, ys, hs, pre_c, pre_d, mk))
