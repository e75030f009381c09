"""Forward free energy of one training step on the engine: mirror of /root/reference/src/torchloss.py (compute_omega, compute_kl_div_pi,
compute_loss_top, compute_loss_mid, compute_loss_down) with the reference's names, arguments and return tuples, plus `free_energy`, the
composition train.py:104-123 evaluates before its optimizer steps, in one engine call (efe_free_energy, csrc/loss.hip).

No autograd graph is built.  The habit network and the transition network are trainable: `train_model_top` (torchloss.py:65-74) and
`train_model_mid` (torchloss.py:76-88) are each one Adam step on the device (csrc/train.hip: backward + update in two launches, with a
daimc_amd.Adam holding the state), and `grad_top` / `grad_mid` return the gradients.  `train_model_down` (torchloss.py:90-98, the encoder /
decoder, 1 x 64 x 64 models) is one engine call too: the gradient, Adam over the 4 787 125 parameters, and every packed forward form of
po_net and the encoder rebuilt on the device (csrc/train_down.hip).  `grad_down` returns F_down and d mean(F_down) / d every parameter of ModelDown (qs_net, then
po_net: the order an Adam over model_down.parameters() sees) in one engine call -- per 64-row group the encoder evaluated for training
with the forward encoder's three dropout masks (csrc/train_enc.hip), the sample, the decoder's forward and backward, the gradient of the
reconstruction and KL terms at the latent, and the encoder's backward.  Its pieces run on their own: `grad_encoder` is the encoder's
vector-Jacobian product for a given upstream pair, `grad_decoder` the gradient of the reconstruction term with respect to every
parameter of po_net and to s -- the dense head po_net.0 / .3 / .6 / .9 evaluated for training with the forward decoder's four dropout
masks (csrc/train_dec_head.hip), then the four ConvTranspose2d layers (po_net.13 / .15 / .17 / .19, csrc/train_dec.hip), which
`grad_decoder_convs` also runs from a given Unflatten input.  `train_step` is the loop body of train.py:111-126 as ONE engine call
(efe_train_step): the o0 encoder + sample, the habit net's step, compute_omega of its kl_pi on the device, the o1 encoder, the transition
net's step and ModelDown's step, bit-identical to those public calls issued one after another, plus the batch means a loop logs
(`TrainStep.means`) without a synchronisation; daimc_amd.train.Trainer drives it.  `eval_stats` reduces what an epoch's evaluation logs
(train.py:136-187: means, order statistics, TC, the reward-transition error of `compare_reward`, Spearman correlations of the latents
with the true factors) into one device row (efe_eval_stats, csrc/eval.hip).  Every
call dispatches through torch.ops.efe.* on the model's device; there is no CPU fallback.

Noise: each loss draws its masks / normals under its own pass id (model.PASS_FE_*: FE_Q0 for the o0 encoder + sample, FE_Q1 for the o1
encoder, FE_T for the transition + sample, FE_DOWN for compute_loss_down's encoder + sample + decoder), one stage per call, rows keyed
by global row (`row_offset`).  So encoder_with_sample(o0, pass_=PASS_FE_Q0), encoder(o1, pass_=PASS_FE_Q1), compute_loss_top,
compute_loss_mid and compute_loss_down at one stage reproduce `free_energy` bit for bit.  `model.eps_source` (injected normals) is honoured.
train_model_mid / grad_mid draw the transition's three dropout masks under the same keys as compute_loss_mid (default pass PASS_FE_T) and
no normals: the reference's randn_like sample does not enter the loss.

Deviations from the reference, each a defect of the shipped code ("training-side free energy"):
  * compute_loss_down reads gamma / beta_s / beta_o from the owning ActiveInferenceModel: the reference reads them from ModelDown,
    which has none (train.py:101), and passes 0.0 to torch.exp, which raises TypeError (exp(0) = 1 is used).
  * compute_kl_div_pi encodes with encoder_with_sample: the reference calls a nonexistent encode_o_and_sample_s.
  * compute_omega accepts a tensor, a numpy array or a number (train.py:118 passes numpy, which torch.exp rejects) and computes in fp32.
  * omega may be a Python float (the evaluation block, train.py:142-143, whose torch.log rejects it): it is broadcast to every row.
"""
import collections

import numpy as np
import torch

from . import _lib
from .model import PASS_FE_Q0, PASS_FE_Q1, PASS_FE_T, PASS_FE_DOWN

FreeEnergy = collections.namedtuple('FreeEnergy', _lib.FE_OUT_FIELDS)
TrainStep = collections.namedtuple('TrainStep', _lib.STEP_OUT_FIELDS)
STEP_MEANS_FIELDS = _lib.STEP_MEANS_FIELDS      # what TrainStep.means [8] holds, in order
OMEGA_PARAMS = (1.0, 25.0, 5.0, 1.5)        # train.py:29-32 (var_a, var_b, var_c, var_d)


def _f32(x):
    return float(np.float32(float(x)))


def compute_omega(kl_pi, a, b, c, d):
    """torchloss.py:8-9 in fp32 -> tensor (on kl_pi's device when kl_pi is a tensor)"""
    t = kl_pi if isinstance(kl_pi, torch.Tensor) else torch.as_tensor(np.asarray(kl_pi))
    t = t.to(torch.float32)
    return a * (1.0 - 1.0 / (1.0 + torch.exp(-(t - b) / c))) + d


def _omega(e, omega, M):
    """-> (omega_mode, per-row tensor or None, scalar): a number (or one-element value) is broadcast to every row, otherwise M values"""
    if isinstance(omega, (int, float, np.floating, np.integer)):
        return _lib.EFE_OMEGA_SCALAR, None, _f32(omega)
    t = e.tensor(omega).reshape(-1)
    if t.numel() == 1 and M != 1:
        return _lib.EFE_OMEGA_SCALAR, None, _f32(t.item())
    if t.numel() != M:
        raise ValueError(f'omega has {t.numel()} elements, expected a scalar or one per row ({M})')
    return _lib.EFE_OMEGA_ARRAY, t, 1.0


def _eps(m, e, eps, M, pass_, sample, stage, row_offset):
    if eps is None and m.eps_source is not None:
        eps = m._src_eps(M, m.s_dim, pass_, sample, stage, row_offset)
    return e.tensor(eps, (M, m.s_dim)) if eps is not None else None


def compute_loss_top(model_top, s, log_Ppi):
    """torchloss.py:19-26 -> (F_top, kl_div_pi, kl_div_pi_anal, Qpi)"""
    m = model_top._owner
    e = m._ready()
    s = e.tensor(s, (-1, m.s_dim))
    return tuple(e.ops.loss_top(e.h, s, e.tensor(log_Ppi, (s.shape[0], m.pi_dim))))


def compute_kl_div_pi(model, o0, log_Ppi, *, stage=None, row_offset=None):
    """torchloss.py:11-17 -> kl_div_pi [M]; the posterior sample comes from encoder_with_sample (pass PASS_FE_Q0)"""
    qs0, _, _ = model.model_down.encoder_with_sample(o0, stage=stage, pass_=PASS_FE_Q0, row_offset=row_offset)
    return compute_loss_top(model.model_top, qs0, log_Ppi)[1]


def compute_loss_mid(model_mid, s0, Ppi_sampled, qs1_mean, qs1_logvar, omega, *, stage=None, pass_=PASS_FE_T, sample=0, eps=None,
                     row_offset=None):
    """torchloss.py:28-36 -> (F_mid, (kl_div_s, kl_div_s_anal), ps1, ps1_mean, ps1_logvar)"""
    m = model_mid._owner
    e = m._ready()
    s0 = e.tensor(s0, (-1, m.s_dim))
    M = s0.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    F, kl, anal, ps1, mean, lv = e.ops.loss_mid(e.h, s0, e.tensor(Ppi_sampled, (M, m.pi_dim)), e.tensor(qs1_mean, (M, m.s_dim)),
                                                e.tensor(qs1_logvar, (M, m.s_dim)), mode, om, sc, m._seed64(), nz.stage, pass_, sample,
                                                nz.row_offset, _eps(m, e, eps, M, pass_, sample, nz.stage, row_offset))
    return F, (kl, anal), ps1, mean, lv


def compute_loss_down(model_down, o1, ps1_mean, ps1_logvar, omega, displacement=1e-5, *, stage=None, pass_=PASS_FE_DOWN, sample=0, eps=None,
                      row_offset=None):
    """torchloss.py:53-74 -> (F_down, (-logpo1_s1, kl_div_s, kl_div_s_anal, kl_div_s_naive, kl_div_s_naive_anal), po1, qs1);
    gamma / beta_s / beta_o are the owning ActiveInferenceModel's"""
    if float(displacement) != 1e-5:
        raise ValueError('compute_loss_down: the engine evaluates the reference displacement 1e-5 only')
    m = model_down._owner
    e = m._ready()
    o1 = e.tensor(o1, (-1, m.colour_channels, m.resolution, m.resolution))
    M = o1.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    F, nl, kls, klsa, kln, klna, po1, qs1 = e.ops.loss_down(
        e.h, o1, e.tensor(ps1_mean, (M, m.s_dim)), e.tensor(ps1_logvar, (M, m.s_dim)), _f32(m.gamma), _f32(m.beta_s), _f32(m.beta_o),
        mode, om, sc, m._seed64(), nz.stage, pass_, sample, nz.row_offset, _eps(m, e, eps, M, pass_, sample, nz.stage, row_offset))
    return F, (nl, kls, klsa, kln, klna), po1, qs1


def free_energy(model, o0, o1, pi0, log_Ppi, *, omega=None, omega_params=OMEGA_PARAMS, stage=None, row_offset=None, eps=None):
    """The forward free energy of one training step (train.py:104-123) -> FreeEnergy (fields: _lib.FE_OUT_FIELDS, include/efe_engine.h
    efe_fe_out).  omega: None = compute_omega(kl_pi, *omega_params) of this call (train.py's current_omega), a number = that value for
    every row (the evaluation block), or M values.  eps: optional injected normals [3, M, s_dim] (FE_Q0, FE_T, FE_DOWN)."""
    e = model._ready()
    shp = (-1, model.colour_channels, model.resolution, model.resolution)
    o0 = e.tensor(o0, shp)
    M = o0.shape[0]
    o1 = e.tensor(o1, (M,) + shp[1:])
    if omega is None:
        mode, om, sc = _lib.EFE_OMEGA_DERIVED, None, 1.0
    else:
        mode, om, sc = _omega(e, omega, M)
    a, b, c, d = (_f32(v) for v in omega_params)
    nz = model._noise(stage, 0, 0, row_offset)
    if eps is None and model.eps_source is not None:
        eps = np.stack([model._src_eps(M, model.s_dim, p, 0, nz.stage, row_offset) for p in (PASS_FE_Q0, PASS_FE_T, PASS_FE_DOWN)], 0)
    eps_t = e.tensor(eps, (3, M, model.s_dim)) if eps is not None else None
    outs = e.ops.free_energy(e.h, o0, o1, e.tensor(pi0, (M, model.pi_dim)), e.tensor(log_Ppi, (M, model.pi_dim)), _f32(model.gamma),
                             _f32(model.beta_s), _f32(model.beta_o), mode, om, sc, a, b, c, d, model._seed64(), nz.stage, nz.row_offset, eps_t)
    return FreeEnergy(*outs)


def _views(flat, tensors, keys=None):
    """views of the flat gradient `flat` per state_dict key: {key: flat[its span].reshape(its shape)}, keys in parameters() order"""
    grads, off = {}, 0
    for key in (tensors if keys is None else keys):
        t = tensors[key]
        grads[key] = flat[off:off + t.numel()].reshape(t.shape)
        off += t.numel()
    return grads


def grad_top(model_top, s, log_Ppi):
    """-> (kl_div_pi [M], {state_dict key: d mean(F_top) / d tensor}): what torchloss.py:69-72 leaves in .grad (views of one flat tensor)"""
    m = model_top._owner
    e = m._ready()
    s = e.tensor(s, (-1, m.s_dim))
    kl, flat = e.ops.top_grad(e.h, s, e.tensor(log_Ppi, (s.shape[0], m.pi_dim)))
    return kl, _views(flat, model_top._sd_host)


def train_model_top(model_top, s, log_Ppi, optimizer):
    """torchloss.py:65-74: one optimiser step of the habit net on F_top.mean() -> kl_div_pi [M] of the weights before the step.
    optimizer: a daimc_amd.Adam over this model_top.  Bit-identical to grad_top followed by optimizer.step(grads)."""
    if getattr(optimizer, '_module', None) is not model_top:
        raise ValueError('train_model_top: optimizer must be a daimc_amd.Adam over this model_top')
    m = model_top._owner
    e = m._ready()
    s = e.tensor(s, (-1, m.s_dim))
    lp = e.tensor(log_Ppi, (s.shape[0], m.pi_dim))
    ea, es = optimizer._buffers()
    hyper = optimizer._hyper()
    optimizer._step += 1
    kl = e.ops.train_top(e.h, s, lp, ea, es, *hyper, optimizer._step)
    model_top._stepped()
    return kl


def _mid_inputs(model_mid, s0, qs1_mean, qs1_logvar, Ppi_sampled, omega, stage, pass_, sample, row_offset):
    m = model_mid._owner
    e = m._ready()
    s0 = e.tensor(s0, (-1, m.s_dim))
    M = s0.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    return m, e, (e.h, s0, e.tensor(Ppi_sampled, (M, m.pi_dim)), e.tensor(qs1_mean, (M, m.s_dim)), e.tensor(qs1_logvar, (M, m.s_dim)),
                  mode, om, sc, m._seed64(), nz.stage, pass_, sample, nz.row_offset)


def grad_mid(model_mid, s0, qs1_mean, qs1_logvar, Ppi_sampled, omega, *, stage=None, pass_=PASS_FE_T, sample=0, row_offset=None):
    """-> (F_mid [M], ps1_mean, ps1_logvar [M, s_dim], {state_dict key: d mean(F_mid) / d tensor}): what torchloss.py:83-85 leaves in
    .grad (views of one flat tensor), with the dropout masks of (stage, pass_, sample, row_offset)"""
    _, _, args = _mid_inputs(model_mid, s0, qs1_mean, qs1_logvar, Ppi_sampled, omega, stage, pass_, sample, row_offset)
    F, mean, lv, flat = model_mid._owner._engine.ops.mid_grad(*args)
    return F, mean, lv, _views(flat, model_mid._sd_host)


def train_model_mid(model_mid, s0, qs1_mean, qs1_logvar, Ppi_sampled, omega, optimizer, *, stage=None, pass_=PASS_FE_T, sample=0,
                    row_offset=None):
    """torchloss.py:76-88: one optimiser step of the transition net on F_mid.mean() -> (ps1_mean, ps1_logvar) of the weights before the
    step.  optimizer: a daimc_amd.Adam over this model_mid.  Bit-identical to grad_mid followed by optimizer.step(grads)."""
    if getattr(optimizer, '_module', None) is not model_mid:
        raise ValueError('train_model_mid: optimizer must be a daimc_amd.Adam over this model_mid')
    _, e, args = _mid_inputs(model_mid, s0, qs1_mean, qs1_logvar, Ppi_sampled, omega, stage, pass_, sample, row_offset)
    ea, es = optimizer._buffers()
    hyper = optimizer._hyper()
    optimizer._step += 1
    mean, lv, _ = e.ops.train_mid(*args, ea, es, *hyper, optimizer._step)
    model_mid._stepped()
    return mean, lv


DEC_CONVT_KEYS = tuple(f'po_net.{i}.{sfx}' for i in (13, 15, 17, 19) for sfx in ('weight', 'bias'))


def grad_decoder_convs(model_down, h4, o1, *, scale=None, return_activations=False):
    """Backward of L = scale * sum_r -log p(o1_r) through po_net[12:] (Unflatten, four ConvTranspose2d, ReLUs, sigmoid; torchmodel.py:119-127,
    torchloss.py:62) -> (nlogpo1 [M], po1 [M,1,64,64], d_h4 [M,16384], {state_dict key: dL / d tensor}) and, with return_activations,
    (y1, y2, y3), the stored post-ReLU activations (NCHW) whose sign is the backward gate.  h4 [M,16384] is what po_net[0:12] hands to the
    Unflatten (reference order); scale None = beta_o / M, the decoder's share of F_down.mean().  The gradients are views of one flat tensor
    in parameters() order.  1 x 64 x 64 models only."""
    m = model_down._owner
    if (m.colour_channels, m.resolution) != (1, 64):
        raise ValueError(f'grad_decoder_convs: built for 1 x 64 x 64 models, this one is {m.colour_channels} x {m.resolution} x {m.resolution}')
    e = m._ready()
    h4 = e.tensor(h4, (-1, 16384))
    M = h4.shape[0]
    o1 = e.tensor(o1, (M, 1, 64, 64))
    if scale is not None and not float(scale) >= 0.0:
        raise ValueError('grad_decoder_convs: scale must be >= 0 (None = beta_o / M)')
    nl, po1, d_h4, flat, y1, y2, y3 = e.ops.dec_tail_grad(e.h, h4, o1, -1.0 if scale is None else _f32(scale), _f32(m.beta_o),
                                                          bool(return_activations))
    out = (nl, po1, d_h4, _views(flat, model_down._sd_host, DEC_CONVT_KEYS))
    return out + ((y1, y2, y3),) if return_activations else out


def grad_decoder_convs_g(model_down, h4, o1, *, scale=None, return_activations=False):
    """grad_decoder_convs at every admitted geometry (csrc/train_dec_g.hip, efe_dec_tail_grad_g): the sizes come from the model.  With
    C colour channels, resolution R and B = R / 4 (16 at R = 32, where po_net.17 has stride 1): h4 [M, 64 B B], o1 [M,C,R,R] ->
    (nlogpo1 [M], po1 [M,C,R,R], d_h4 [M, 64 B B], {state_dict key: dL / d tensor}) and, with return_activations, (y1 [M,64,B,B],
    y2 [M,64,2B,2B], y3 [M,32,R,R]).  scale None = beta_o / M.  The gradients are views of one flat tensor over DEC_CONVT_KEYS in
    parameters() order.  1 x 64 x 64 models run the same run-time-geometry kernels (grad_decoder_convs is then a cross-check)."""
    m = model_down._owner
    if scale is not None and not float(scale) >= 0.0:
        raise ValueError('grad_decoder_convs_g: scale must be >= 0 (None = beta_o / M)')
    e = m._ready()
    C_, R = int(m.colour_channels), int(m.resolution)
    B = 16 if R == 32 else R // 4
    h4 = e.tensor(h4, (-1, 64 * B * B))
    M = h4.shape[0]
    o1 = e.tensor(o1, (M, C_, R, R))
    nl, po1, d_h4, flat, y1, y2, y3 = torch.ops.efe_g.dec_tail_grad(e.h, h4, o1, -1.0 if scale is None else _f32(scale), _f32(m.beta_o),
                                                                    bool(return_activations))
    out = (nl, po1, d_h4, _views(flat, model_down._sd_host, DEC_CONVT_KEYS))
    return out + ((y1, y2, y3),) if return_activations else out


DEC_HEAD_KEYS = tuple(f'po_net.{i}.{sfx}' for i in (0, 3, 6, 9) for sfx in ('weight', 'bias'))


def grad_decoder(model_down, s, o1, *, scale=None, stage=None, pass_=PASS_FE_DOWN, sample=0, row_offset=None, return_activations=False):
    """Backward of L = scale * sum_r -log p(o1_r) through the whole decoder po_net (torchmodel.py:106-128, torchloss.py:62) -> (nlogpo1 [M],
    po1 [M,1,64,64], d_s [M,10], {state_dict key: dL / d tensor}) and, with return_activations, (h1, h2, h3, h4, y1, y2, y3): the stored
    activations after ReLU and dropout mask (h1..h3 [M,256], h4 [M,16384] in the Unflatten's order; y1..y3 NCHW), whose sign is the
    backward gate.  The four dropout masks are those `model_down.decoder(s, stage=, pass_=, sample=, row_offset=)` draws, so po1 agrees
    with it to rounding.  scale None = beta_o / M, the decoder's share of F_down.mean().  The gradients are views of one flat tensor over
    the 16 po_net.* keys in parameters() order.  1 x 64 x 64 models only."""
    m = model_down._owner
    if (m.colour_channels, m.resolution) != (1, 64):
        raise ValueError(f'grad_decoder: built for 1 x 64 x 64 models, this one is {m.colour_channels} x {m.resolution} x {m.resolution}')
    if scale is not None and not float(scale) >= 0.0:
        raise ValueError('grad_decoder: scale must be >= 0 (None = beta_o / M)')
    e = m._ready()
    s = e.tensor(s, (-1, m.s_dim))
    M = s.shape[0]
    o1 = e.tensor(o1, (M, 1, 64, 64))
    nz = m._noise(stage, pass_, sample, row_offset)
    out = e.ops.dec_grad(e.h, s, o1, -1.0 if scale is None else _f32(scale), _f32(m.beta_o), m._seed64(), nz.stage, pass_, sample,
                         nz.row_offset, bool(return_activations))
    nl, po1, d_s, flat = out[:4]
    res = (nl, po1, d_s, _views(flat, model_down._sd_host, DEC_HEAD_KEYS + DEC_CONVT_KEYS))
    return res + (tuple(out[4:]),) if return_activations else res


def grad_decoder_g(model_down, s, o1, *, scale=None, stage=None, pass_=PASS_FE_DOWN, sample=0, row_offset=None, return_activations=False):
    """grad_decoder at every admitted geometry (csrc/train_dec_head_g.hip + csrc/train_dec_g.hip, efe_dec_grad_g): the sizes come from the
    model.  With C colour channels, resolution R, B = R / 4 (16 at R = 32) and F = 64 B B: s [M,10], o1 [M,C,R,R] -> (nlogpo1 [M],
    po1 [M,C,R,R], d_s [M,10], {state_dict key: dL / d tensor}) and, with return_activations, (h1, h2, h3 [M,256], h4 [M,F] in the
    Unflatten's order, y1 [M,64,B,B], y2 [M,64,2B,2B], y3 [M,32,R,R]).  The four dropout masks are those `model_down.decoder(s, stage=,
    pass_=, sample=, row_offset=)` draws at that geometry.  scale None = beta_o / M.  The gradients are views of one flat tensor over
    DEC_HEAD_KEYS + DEC_CONVT_KEYS in parameters() order; the tail's are grad_decoder_convs_g's on the returned h4, bit for bit.
    1 x 64 x 64 models run the same run-time-geometry kernels (grad_decoder is then a cross-check)."""
    m = model_down._owner
    if scale is not None and not float(scale) >= 0.0:
        raise ValueError('grad_decoder_g: scale must be >= 0 (None = beta_o / M)')
    e = m._ready()
    C_, R = int(m.colour_channels), int(m.resolution)
    s = e.tensor(s, (-1, m.s_dim))
    M = s.shape[0]
    o1 = e.tensor(o1, (M, C_, R, R))
    nz = m._noise(stage, pass_, sample, row_offset)
    out = torch.ops.efe_g.dec_grad(e.h, s, o1, -1.0 if scale is None else _f32(scale), _f32(m.beta_o), m._seed64(), nz.stage, pass_, sample,
                                   nz.row_offset, bool(return_activations))
    nl, po1, d_s, flat = out[:4]
    res = (nl, po1, d_s, _views(flat, model_down._sd_host, DEC_HEAD_KEYS + DEC_CONVT_KEYS))
    return res + (tuple(out[4:]),) if return_activations else res


ENC_KEYS =tuple(f'qs_net.{i}.{sfx}' for i in (0, 2, 4, 6, 9, 12, 15, 18) for sfx in ('weight', 'bias'))


def _down_model(model_down, who):
    m = model_down._owner
    if (m.colour_channels, m.resolution) != (1, 64):
        raise ValueError(f'{who}: built for 1 x 64 x 64 models, this one is {m.colour_channels} x {m.resolution} x {m.resolution}')
    return m, m._ready()


def grad_encoder(model_down, o, d_mean, d_logvar, *, stage=None, pass_=PASS_FE_DOWN, sample=0, row_offset=None, return_activations=False):
    """The encoder qs_net (torchmodel.py:84-104) evaluated for training and its vector-Jacobian product for the upstream pair d_mean,
    d_logvar [M,10] -> (qs_mean [M,10], qs_logvar [M,10], {state_dict key: sum_r d_mean_r . d qs_mean_r / d tensor + d_logvar_r . d qs_logvar_r
    / d tensor}) and, with return_activations, (y1, y2, y3, y4, h1, h2, h3): the stored activations (y1..y4 NCHW after the ReLU, h1..h3
    [M,256] after ReLU and dropout mask), whose sign is the backward gate.  The three dropout masks are those `model_down.encoder(o, stage=,
    pass_=, sample=, row_offset=)` draws, so qs_mean / qs_logvar agree with it to rounding.  The gradients are views of one flat tensor
    over the 16 qs_net.* keys in parameters() order.  1 x 64 x 64 models only."""
    m, e = _down_model(model_down, 'grad_encoder')
    o = e.tensor(o, (-1, 1, 64, 64))
    M = o.shape[0]
    nz = m._noise(stage, pass_, sample, row_offset)
    out = e.ops.enc_grad(e.h, o, e.tensor(d_mean, (M, m.s_dim)), e.tensor(d_logvar, (M, m.s_dim)), m._seed64(), nz.stage, pass_, sample,
                         nz.row_offset, bool(return_activations))
    res = (out[0], out[1], _views(out[2], model_down._sd_host, ENC_KEYS))
    return res + (tuple(out[3:]),) if return_activations else res


def grad_down(model_down, o1, ps1_mean, ps1_logvar, omega, *, stage=None, pass_=PASS_FE_DOWN, sample=0, eps=None, row_offset=None,
              return_upstream=False):
    """train_model_down (torchloss.py:90-98) up to the gradient -> (F_down [M], (nlogpo1, kl_div_s, kl_div_s_naive) [M] each, po1 [M,1,64,64],
    qs1, qs1_mean, qs1_logvar [M,10], {state_dict key: d mean(F_down) / d tensor}) and, with return_upstream, (g_mean, g_logvar) [M,10]: the
    gradient at the encoder's outputs.  The gradients are views of one flat tensor over all 32 keys of model_down in parameters() order
    (qs_net, then po_net).  ps1_mean, ps1_logvar and omega are constants, as the reference detaches them; gamma / beta_s / beta_o are the
    owning ActiveInferenceModel's, as in compute_loss_down, whose keys (stage, pass_, sample, row_offset, eps) this call shares: F_down and
    its terms agree with it to rounding.  1 x 64 x 64 models only."""
    m, e = _down_model(model_down, 'grad_down')
    o1 = e.tensor(o1, (-1, 1, 64, 64))
    M = o1.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    F, nl, kls, kln, po1, qs1, qm, qv, gm, gv, flat = e.ops.down_grad(
        e.h, o1, e.tensor(ps1_mean, (M, m.s_dim)), e.tensor(ps1_logvar, (M, m.s_dim)), _f32(m.gamma), _f32(m.beta_s), _f32(m.beta_o),
        mode, om, sc, m._seed64(), nz.stage, pass_, sample, nz.row_offset, _eps(m, e, eps, M, pass_, sample, nz.stage, row_offset))
    res = (F, (nl, kls, kln), po1, qs1, qm, qv, _views(flat, model_down._sd_host, ENC_KEYS + DEC_HEAD_KEYS + DEC_CONVT_KEYS))
    return res + ((gm, gv),) if return_upstream else res


def grad_encoder_g(model_down, o, d_mean, d_logvar, *, stage=None, pass_=PASS_FE_DOWN, sample=0, row_offset=None, return_activations=False):
    """grad_encoder at every admitted geometry (csrc/train_enc_g.hip, efe_enc_grad_g): the sizes come from the model.  With C colour
    channels, resolution R, H_l = (H_{l-1} - 3) // 2 + 1 from H_0 = R and K = 64 H4^2: o [M,C,R,R], d_mean, d_logvar [M,10] -> (qs_mean [M,10],
    qs_logvar [M,10], {state_dict key: gradient}) and, with return_activations, (y1 [M,32,H1,H1], y2 [M,32,H2,H2], y3 [M,64,H3,H3],
    y4 [M,64,H4,H4], h1, h2, h3 [M,256]).  The three dropout masks are those `model_down.encoder(o, stage=, pass_=, sample=, row_offset=)`
    draws at that geometry.  The gradients are views of one flat tensor over ENC_KEYS in parameters() order (qs_net.9.weight is [256, K]).
    1 x 64 x 64 models run the same run-time-geometry kernels (grad_encoder is then a cross-check)."""
    m = model_down._owner
    e = m._ready()
    C_, R = int(m.colour_channels), int(m.resolution)
    o = e.tensor(o, (-1, C_, R, R))
    M = o.shape[0]
    nz = m._noise(stage, pass_, sample, row_offset)
    out = torch.ops.efe_g.enc_grad(e.h, o, e.tensor(d_mean, (M, m.s_dim)), e.tensor(d_logvar, (M, m.s_dim)), m._seed64(), nz.stage, pass_, sample,
                                   nz.row_offset, bool(return_activations))
    res = (out[0], out[1], _views(out[2], model_down._sd_host, ENC_KEYS))
    return res + (tuple(out[3:]),) if return_activations else res


def grad_down_g(model_down, o1, ps1_mean, ps1_logvar, omega, *, stage=None, pass_=PASS_FE_DOWN, sample=0, eps=None, row_offset=None,
                return_upstream=False):
    """grad_down at every admitted geometry (csrc/train_enc_g.hip around csrc/train_dec_head_g.hip + csrc/train_dec_g.hip, efe_down_grad_g):
    o1 [M,C,R,R] of the model's geometry -> (F_down [M], (nlogpo1, kl_div_s, kl_div_s_naive) [M] each, po1 [M,C,R,R], qs1, qs1_mean,
    qs1_logvar [M,10], {state_dict key: d mean(F_down) / d tensor}) and, with return_upstream, (g_mean, g_logvar) [M,10].  The gradients are
    views of one flat tensor over all 32 keys of model_down in parameters() order (qs_net, then po_net): the po_net half, po1 and nlogpo1
    are grad_decoder_g(qs1, o1)'s, the qs_net half grad_encoder_g's on the returned upstream pair, bit for bit.  Keys, constants and
    hyper-parameters as grad_down.  1 x 64 x 64 models run the same run-time-geometry kernels (grad_down is then a cross-check)."""
    m = model_down._owner
    e = m._ready()
    C_, R = int(m.colour_channels), int(m.resolution)
    o1 = e.tensor(o1, (-1, C_, R, R))
    M = o1.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    F, nl, kls, kln, po1, qs1, qm, qv, gm, gv, flat = torch.ops.efe_g.down_grad(
        e.h, o1, e.tensor(ps1_mean, (M, m.s_dim)), e.tensor(ps1_logvar, (M, m.s_dim)), _f32(m.gamma), _f32(m.beta_s), _f32(m.beta_o),
        mode, om, sc, m._seed64(), nz.stage, pass_, sample, nz.row_offset, _eps(m, e, eps, M, pass_, sample, nz.stage, row_offset))
    res = (F, (nl, kls, kln), po1, qs1, qm, qv, _views(flat, model_down._sd_host, ENC_KEYS + DEC_HEAD_KEYS + DEC_CONVT_KEYS))
    return res + ((gm, gv),) if return_upstream else res


def train_model_down(model_down, o1, ps1_mean, ps1_logvar, omega, optimizer, *, stage=None, pass_=PASS_FE_DOWN, sample=0, eps=None,
                     row_offset=None):
    """torchloss.py:90-98: one optimiser step of the encoder and decoder on F_down.mean() -> (F_down [M], (nlogpo1, kl_div_s, kl_div_s_naive)
    [M] each) of the weights before the step.  One engine call (efe_train_down): grad_down's row groups, Adam over all 32 tensors, and
    every packed forward form rebuilt on the device, with no host synchronisation.  optimizer: a daimc_amd.Adam over this model_down.
    Bit-identical to grad_down followed by optimizer.step(grads).  1 x 64 x 64 models only."""
    if getattr(optimizer, '_module', None) is not model_down:
        raise ValueError('train_model_down: optimizer must be a daimc_amd.Adam over this model_down')
    m, e = _down_model(model_down, 'train_model_down')
    o1 = e.tensor(o1, (-1, 1, 64, 64))
    M = o1.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    ea, es = optimizer._buffers()
    hyper = optimizer._hyper()
    F, nl, kls, kln = e.ops.train_down(
        e.h, o1, e.tensor(ps1_mean, (M, m.s_dim)), e.tensor(ps1_logvar, (M, m.s_dim)), _f32(m.gamma), _f32(m.beta_s), _f32(m.beta_o),
        mode, om, sc, m._seed64(), nz.stage, pass_, sample, nz.row_offset, _eps(m, e, eps, M, pass_, sample, nz.stage, row_offset),
        ea, es, *hyper, optimizer._step + 1)
    optimizer._step += 1
    model_down._stepped()
    return F, (nl, kls, kln)


def train_model_down_g(model_down, o1, ps1_mean, ps1_logvar, omega, optimizer, *, stage=None, pass_=PASS_FE_DOWN, sample=0, eps=None,
                       row_offset=None):
    """train_model_down at every admitted geometry (efe_train_down_g): o1 [M,C,R,R] of the model's geometry -> (F_down [M], (nlogpo1,
    kl_div_s, kl_div_s_naive) [M] each) of the weights before the step.  One engine call: grad_down_g's row groups, Adam over all 32
    tensors, and every packed forward form of the model's path rebuilt on the device (csrc/train_down_g.hip), with no host
    synchronisation.  optimizer: daimc_amd.Adam(model_down, any_geometry=True).  Bit-identical to grad_down_g followed by
    optimizer.step(grads).  At 1 x 64 x 64 the step is train_model_down's on the same master copy (the gradient is grad_down_g's)."""
    if getattr(optimizer, '_module', None) is not model_down or not getattr(optimizer, '_any_geometry', False):
        raise ValueError('train_model_down_g: optimizer must be a daimc_amd.Adam(model_down, any_geometry=True) over this model_down')
    m = model_down._owner
    e = m._ready()
    C_, R = int(m.colour_channels), int(m.resolution)
    o1 = e.tensor(o1, (-1, C_, R, R))
    M = o1.shape[0]
    mode, om, sc = _omega(e, omega, M)
    nz = m._noise(stage, pass_, sample, row_offset)
    ea, es = optimizer._buffers()
    hyper = optimizer._hyper()
    F, nl, kls, kln = torch.ops.efe_g.train_down(
        e.h, o1, e.tensor(ps1_mean, (M, m.s_dim)), e.tensor(ps1_logvar, (M, m.s_dim)), _f32(m.gamma), _f32(m.beta_s), _f32(m.beta_o),
        mode, om, sc, m._seed64(), nz.stage, pass_, sample, nz.row_offset, _eps(m, e, eps, M, pass_, sample, nz.stage, row_offset),
        ea, es, *hyper, optimizer._step + 1)
    optimizer._step += 1
    model_down._stepped()
    return F, (nl, kls, kln)


def _step_optimizers(model, optimizers):
    """the reference's optimizers dict -> (top, mid, down) daimc_amd.Adam, each over this model's part"""
    out = []
    for name, mod in (('top', model.model_top), ('mid', model.model_mid), ('down', model.model_down)):
        if not hasattr(optimizers, 'get') or optimizers.get(name) is None:
            raise ValueError(f"train_step: optimizers has no entry '{name}' (expected {{'top': Adam(model.model_top), 'mid': "
                             "Adam(model.model_mid), 'down': Adam(model.model_down)}})")
        if getattr(optimizers[name], '_module', None) is not mod:
            raise ValueError(f"train_step: optimizers['{name}'] must be a daimc_amd.Adam over this model's model_{name}")
        out.append(optimizers[name])
    return out


def train_step(model, o0, o1, pi0, log_Ppi, optimizers, *, omega=None, omega_params=OMEGA_PARAMS, stage=None, row_offset=None, eps=None,
               means=None):
    """The loop body of train.py:111-126 as one engine call (efe_train_step) -> TrainStep (fields: _lib.STEP_OUT_FIELDS): qs0 =
    encoder_with_sample(o0), train_model_top, omega, encoder(o1), train_model_mid, train_model_down, all at ONE stage under the passes
    PASS_FE_Q0 / _Q1 / _T / _DOWN, with no host synchronisation.  Bit-identical to those public calls issued one after another at that
    stage with this call's per-row omega.  Every output is of the weights before the step.
    optimizers: {'top': Adam(model.model_top), 'mid': Adam(model.model_mid), 'down': Adam(model.model_down)} (daimc_amd.Adam).
    omega: None = compute_omega(kl_pi, *omega_params) of this call on the device (train.py:118), a number, or M values.
    eps: optional injected normals [3, M, s_dim] as free_energy lays them out (plane 0: the FE_Q0 sample, plane 2: the FE_DOWN sample,
    plane 1 is not read).  means: optional [8] device tensor written in place (STEP_MEANS_FIELDS: the batch means of kl_pi, omega, F_mid,
    F_down, nlogpo1, kl_s, kl_naive and the unbiased standard deviation of omega); one is allocated otherwise.  1 x 64 x 64 models only."""
    if (model.colour_channels, model.resolution) != (1, 64):        # (first: no Adam over model_down exists at another geometry)
        raise ValueError(f'train_step: built for 1 x 64 x 64 models, this one is {model.colour_channels} x {model.resolution} x {model.resolution}')
    opts = _step_optimizers(model, optimizers)
    e = model._ready()
    o0 = e.tensor(o0, (-1, 1, 64, 64))
    M = o0.shape[0]
    o1 = e.tensor(o1, (M, 1, 64, 64))
    if omega is None:
        mode, om, sc = _lib.EFE_OMEGA_DERIVED, None, 1.0
    else:
        mode, om, sc = _omega(e, omega, M)
    a, b, c, d = (_f32(v) for v in omega_params)
    if means is None:
        means = e.empty(_lib.EFE_STEP_MEANS)
    elif not (isinstance(means, torch.Tensor) and means.device == e.device and means.dtype == torch.float32 and means.is_contiguous()
              and means.numel() == _lib.EFE_STEP_MEANS):
        raise ValueError(f'train_step: means must be a contiguous float32 tensor of {_lib.EFE_STEP_MEANS} elements on the model device')
    hyper = [v for o in opts for v in o._hyper()]
    state = [t for o in opts for t in o._buffers()]
    pi0, log_Ppi = e.tensor(pi0, (M, model.pi_dim)), e.tensor(log_Ppi, (M, model.pi_dim))
    nz = model._noise(stage, 0, 0, row_offset)
    if eps is None and model.eps_source is not None:
        eps = np.stack([model._src_eps(M, model.s_dim, p, 0, nz.stage, row_offset) for p in (PASS_FE_Q0, PASS_FE_T, PASS_FE_DOWN)], 0)
    eps_t = e.tensor(eps, (3, M, model.s_dim)) if eps is not None else None
    outs = e.ops.train_step(e.h, o0, o1, pi0, log_Ppi, _f32(model.gamma), _f32(model.beta_s), _f32(model.beta_o), mode, om, sc, a, b, c, d,
                            model._seed64(), nz.stage, nz.row_offset, eps_t, *state, hyper, [o._step + 1 for o in opts], means)
    for o in opts:
        o._step += 1
        o._module._stepped()
    return TrainStep(*outs, means)


# ---- the epoch report (efe_eval_stats, csrc/eval.hip): the statistics train.py:136-187 appends to `stats`, one device row ---------------
EVAL_FE_ARRAYS = ('F_top', 'F_mid', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'kl_pi', 'kl_s_anal', 'kl_naive_anal', 'kl_pi_anal')
# name -> slice of the [98] row (include/efe_engine.h efe_eval_stats); spearman is [10][6] row-major
EVAL_STATS_FIELDS = {
    'F': slice(0, 1), 'F_top': slice(1, 2), 'F_mid': slice(2, 3), 'F_down': slice(3, 4), 'mse_o': slice(4, 5), 'kl_div_s': slice(5, 6),
    'kl_div_s_naive': slice(6, 7), 'kl_div_pi': slice(7, 8), 'kl_div_pi_min': slice(8, 9), 'kl_div_pi_max': slice(9, 10),
    'kl_div_pi_med': slice(10, 11), 'kl_div_pi_std': slice(11, 12), 'TC': slice(12, 13), 'mse_r': slice(13, 14),
    'kl_div_s_anal': slice(14, 24), 'kl_div_s_naive_anal': slice(24, 34), 'kl_div_pi_anal': slice(34, 38), 'spearman': slice(38, 98),
}
EVAL_FACTORS = ('shape', 'scale', 'orientation', 'posX', 'posY', 'reward')      # the columns of S_real, and of spearman's rows
_stats_engines = {}


def _stats_engine(device):
    """an engine context of `device` for calls that read no weights (one per device, made on first use)"""
    from .model import _Engine
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _stats_engines:
        _stats_engines[idx] = _Engine(idx)
    return _stats_engines[idx]


def eval_stats(fe=None, S_real=None, reward=None, out=None, *, engine=None):
    """The batch statistics of an evaluation batch, reduced on the device in one engine call (efe_eval_stats) with no synchronisation ->
    the [98] float32 device row EVAL_STATS_FIELDS names.  Inputs come in four groups, each whole or absent; an absent group's fields
    are NaN:
      fe      : a FreeEnergy (or any object / mapping with some of its fields): its ten loss arrays (EVAL_FE_ARRAYS) give the means, the
                order statistics of kl_pi and the column means; its qs1 gives TC; its s0 goes with S_real
      S_real  : [M, 6] true factors of the rows of fe.s0 (util.make_batch_dsprites_random) -> spearman
      reward  : (o1, po1), [Mr, 1, 64, 64] each -> mse_r (compare_reward)
    out: an optional contiguous float32 [98] device tensor (or view) written in place.  engine: the engine context to run on (a model's
    `_ready()`); by default one per device that holds no weights.  At most 8192 rows per group."""
    get = (lambda k: fe.get(k)) if hasattr(fe, 'get') else (lambda k: getattr(fe, k, None))
    vals = [get(k) for k in EVAL_FE_ARRAYS] + [get('qs1'), get('s0') if S_real is not None else None, S_real]      # (s0 is read with S_real only)
    vals += list(reward) if reward is not None else [None, None]
    if all(v is None for v in vals):
        raise RuntimeError('efe_eval_stats: no input group (FE, TC, RHO or R) given')
    e = engine
    if e is None:           # the device of the first device tensor among the arguments, else the current one
        e = _stats_engine(next((t.device for t in [out] + vals if isinstance(t, torch.Tensor) and t.is_cuda), 'cuda'))
    arrs = [None if v is None else e.tensor(v) for v in vals]
    Mr = next((t.shape[0] if t.dim() else 1 for t in arrs[13:] if t is not None), 0)
    M = next((t.shape[0] if t.dim() else 1 for t in arrs[:13] if t is not None), Mr)      # (the R group alone: M is not read, and must be >= 1)
    if out is None:
        out = e.empty(_lib.EFE_EVAL_STATS)
    e.ops.eval_stats(e.h, *arrs, M, Mr, out)
    return out


def eval_mutual_info(s0, S_real, *, n_neighbors=3, noise=None, seed=0, stage=0, out=None, counts=None, engine=None):
    """The mutual information of every latent column of s0 [M, 10] with every true factor of S_real [M, 6] (EVAL_FACTORS), the scores
    sklearn.feature_selection.mutual_info_regression gives generate_traversals.py:36-46, in one engine call (efe_eval_mi,
    csrc/eval_mi.hip) with no synchronisation -> a float32 [60] device tensor, latent-major like `spearman`.  The estimator is the one
    scikit-learn defines for float64 columns (the reference hands it a float32 factor column, whose value is an
    accident of that dtype and is not reproduced).
      noise  : float64 [60, 2, M], pair-major, the latent's vector first: the standard normals of the tie-breaking jitter.  None: drawn on
               the device from (seed, stage), and the result is a function of (s0, S_real, n_neighbors, seed, stage) alone.
      out    : an optional contiguous float32 [60] device tensor (or view) written in place.
      counts : an optional contiguous int32 [60, 2, M] device tensor: the marginal neighbour counts nx, ny of every point of every pair.
    n_neighbors in 1 .. 4, n_neighbors < M <= 8192.  engine: as eval_stats."""
    e = engine
    if e is None:
        e = _stats_engine(next((t.device for t in (s0, S_real, out) if isinstance(t, torch.Tensor) and t.is_cuda), 'cuda'))
    s0, S_real = e.tensor(s0), e.tensor(S_real)
    if noise is not None:
        noise = torch.as_tensor(noise, dtype=torch.float64).to(s0.device).contiguous()
    if out is None:
        out = e.empty(_lib.EFE_EVAL_MI)
    e.ops.eval_mi(e.h, s0, S_real, noise, int(n_neighbors), int(seed), int(stage), out, counts)
    return out


def compare_reward(o1, po1, *, engine=None):
    """src/util.py:82-85 on the device: the mean squared error of the prediction po1 against o1 over the reward bar (image rows 0..2),
    both [M, 1, 64, 64] (NCHW; the reference slices its NHWC arrays as [:, 0:3, 0:64, :]) -> a 0-d device tensor"""
    return eval_stats(reward=(o1, po1), engine=engine)[EVAL_STATS_FIELDS['mse_r']].reshape(())
