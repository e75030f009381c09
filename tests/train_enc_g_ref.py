"""tests/train_down_ref.py generalised to (channels, resolution): the reference of the encoder's training forward and backward and of the
gradient of F_down for all of ModelDown at every admitted geometry (csrc/train_enc_g.hip around csrc/train_dec_head_g.hip +
csrc/train_dec_g.hip, loss.grad_encoder_g / loss.grad_down_g) -- autograd on the CPU, in a given dtype, over qs_net (torchmodel.py:84-104)
restated with F.conv2d / F.linear, the Philox dropout masks of oracle.efe_oracle.PhiloxNoise applied as multiplications (tag TAG_ENC +
layer), the injected or Philox normal of the sample, the decoder exactly as tests/train_dec_head_g_ref.py states it, and
compute_loss_down's KL terms (torchloss.py:39-63).  The loss of the composed form is F_down.mean(); ps1_mean, ps1_logvar and omega are
constants.

Conv extents H_l = (H_{l-1} - 3) // 2 + 1 from H_0 = R; K = 64 H4^2 inputs of qs_net.9 in the Flatten's order c H4^2 + p.

Same `gates=` override as train_down_ref: gates = (y1..y4, h1..h3) of the encoder, dec_gates = (h1..h4, y1..y3) of the decoder.  At (1, 64)
run_encoder is train_down_ref.run_encoder and run is train_down_ref.run, bit for bit; at other geometries the forward is
oracle.efe_oracle's encoder bit for bit (tests/test_train_enc_g_cpu.py)."""
import numpy as np
import torch
import torch.nn.functional as F

import train_dec_g_ref as TG
import train_dec_head_g_ref as THG
import train_down_ref as TDN

CONVS, DENSE, ENC_KEYS = TDN.CONVS, TDN.DENSE, TDN.ENC_KEYS
KEYS = ENC_KEYS + THG.KEYS                               # parameters() order of ModelDown
PASS_FE_DOWN = THG.PASS_FE_DOWN
SEED = THG.SEED
enc_masks, normals, upstream = TDN.enc_masks, TDN.normals, TDN.upstream


def extents(R):
    """(H1, H2, H3, H4)"""
    hs = []
    for _ in range(4):
        R = (R - 3) // 2 + 1
        hs.append(R)
    return tuple(hs)


def n_in(R):
    """K: inputs of qs_net.9"""
    return 64 * extents(R)[3] ** 2


def enc_param_count(C, R):
    return 201684 + 288 * C + 256 * n_in(R)


def param_count(C, R):
    return enc_param_count(C, R) + THG.param_count(C, R)


def inputs(seed, M, C, R):
    """o1 of train_dec_head_g_ref.inputs(seed, M, C, R); ps1_mean, ps1_logvar, omega of train_down_ref.inputs(seed, M)"""
    _, o1 = THG.inputs(seed, M, C, R)
    g = torch.Generator().manual_seed(seed + 50000)
    pm = 0.5 * torch.randn(M, 10, generator=g)
    pv = 0.5 * torch.randn(M, 10, generator=g)
    om = 1.5 + torch.rand(M, generator=g)
    return o1, pm.numpy().copy(), pv.numpy().copy(), om.numpy().copy()


encode = TDN.encode          # geometry-free as written: the shapes follow the weights


def decode(params, s, o, mk, C, R, dtype, gates=None):
    """train_dec_head_g_ref.run's forward on a tensor s that carries a graph -> (p, logpo1 [M], hs, ys, head pre-activations, tail's)"""
    M, B = s.shape[0], THG.base_of(R)
    x, hs, pre_h = s, [], []
    for li, idx in enumerate(THG.HEAD):
        a = F.linear(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'])
        pre_h.append(a)
        x = torch.relu(a) * mk[li].to(dtype) if gates is None else TDN._gate(a, gates[li], dtype, 2.0)
        hs.append(x)
    x = x.reshape(M, 64, B, B)
    ys, pre = [], []
    for li, (idx, st) in enumerate(TG.layers(R)):
        a = F.conv_transpose2d(x, params[f'po_net.{idx}.weight'], params[f'po_net.{idx}.bias'], stride=st, padding=1, output_padding=st - 1)
        pre.append(a)
        if li == 3:
            break
        x = torch.relu(a) if gates is None else TDN._gate(a, gates[4 + li], dtype, 1.0)
        ys.append(x)
    p = torch.sigmoid(pre[3])
    bce = o * torch.log(1e-5 + p) + (1 - o) * torch.log(1e-5 + 1 - p)
    return p, torch.sum(bce, dim=[1, 2, 3]), hs, ys, pre_h, pre


_n = TDN._n


def run_encoder(weights, o, d_mean, d_logvar, C, R, stage, dtype=torch.float32, gates=None, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """the encoder's vector-Jacobian product for the upstream pair -> dict(mean, logvar [M, 10], grads {key: array}, y, h, a_conv, a_dense,
    enc_masks), numpy arrays in `dtype`"""
    M = o.shape[0]
    params = TDN._params(weights, ENC_KEYS, dtype)
    x0 = torch.tensor(np.array(o)).to(dtype).reshape(M, C, R, R)
    mk = enc_masks(M, stage, seed, pass_, sample, row_offset)
    out, ys, hs, pre_c, pre_d = encode(params, x0, mk, dtype, gates)
    mean, logvar = torch.split(out, 10, dim=1)
    gm, gv = (torch.tensor(np.array(g)).to(dtype).reshape(M, 10) for g in (d_mean, d_logvar))
    ((mean * gm).sum() + (logvar * gv).sum()).backward()
    return dict(mean=_n(mean), logvar=_n(logvar), grads={k: _n(v.grad) for k, v in params.items()}, **TDN._enc_out(out, ys, hs, pre_c, pre_d, mk))


def run(weights, o1, ps1_mean, ps1_logvar, omega, C, R, stage, dtype=torch.float32, gamma=0.5, beta_s=1.0, beta_o=1.0, gates=None, dec_gates=None,
        eps=None, seed=SEED, pass_=PASS_FE_DOWN, sample=0, row_offset=0):
    """compute_loss_down and F.mean().backward() at (C, R); arguments and result as train_down_ref.run"""
    M = o1.shape[0]
    params = TDN._params(weights, KEYS, dtype)
    o = torch.tensor(np.array(o1)).to(dtype).reshape(M, C, R, R)
    mk = enc_masks(M, stage, seed, pass_, sample, row_offset)
    dmk = THG.masks(M, R, stage, seed, pass_, sample, row_offset)
    out, ys, hs, pre_c, pre_d = encode(params, o, mk, dtype, gates)
    mean, logvar = torch.split(out, 10, dim=1)
    mean.retain_grad()
    logvar.retain_grad()
    e = torch.as_tensor(np.asarray(eps, dtype=np.float32)) if eps is not None else normals(M, stage, seed, pass_, sample, row_offset)
    qs1 = e.to(dtype).reshape(M, 10) * torch.exp(logvar * 0.5) + mean
    qs1.retain_grad()
    p, logpo1, dhs, dys, dpre_h, dpre = decode(params, qs1, o, dmk, C, R, dtype, dec_gates)
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
                dec_a=tuple(_n(a) for a in dpre), dec_masks=tuple(m.numpy() for m in dmk), **TDN._enc_out(out, ys, hs, pre_c, pre_d, mk))
