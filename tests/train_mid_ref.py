"""Test-side restatement of train_model_mid (the reference's src/torchloss.py:76-88) on the CPU oracle: OracleModel.transition
(oracle/efe_oracle.py) is torch functional ops on `orc.w` with the Philox dropout masks applied as multiplications, so requires_grad_ on the
eight mid.* tensors gives the reference's gradients by autograd and lets torch.optim.Adam run on them, in fp32 (the restatement) or fp64
(the reference the kernel's error is measured against).  The transition's randn_like sample does not enter the loss and is not drawn.
Shared by tests/test_train_mid_cpu.py (bit-exact against the reference fixture) and tests/test_train_mid_gpu.py (the engine against it)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import philox as PX
from oracle.efe_oracle import OracleModel, PhiloxNoise

KEYS = ('ps_net.0.weight', 'ps_net.0.bias', 'ps_net.3.weight', 'ps_net.3.bias', 'ps_net.6.weight', 'ps_net.6.bias',
        'ps_net.9.weight', 'ps_net.9.bias')      # parameters() order
PASS_FE_T = 11
SEED = 7                # the engine seed of the GPU tests


def batch_mid(seed, M, A=4):
    """s0 [M,10], pi one-hot [M,A], qs1_mean [M,10], qs1_logvar [M,10], omega [M], float32, drawn in this order"""
    r = np.random.RandomState(seed)
    s0 = r.randn(M, 10).astype(np.float32)
    pi = np.eye(A, dtype=np.float32)[r.randint(0, A, M)]
    qs1_mean = r.randn(M, 10).astype(np.float32)
    qs1_logvar = (0.5 * r.randn(M, 10) - 1.0).astype(np.float32)
    omega = r.uniform(1.5, 2.5, M).astype(np.float32)
    return s0, pi, qs1_mean, qs1_logvar, omega


def mid_only(weights):
    """the transition net's tensors, copied: OracleModel wraps fp32 arrays without a copy and torch.optim.Adam updates in place"""
    return {k: np.array(v, dtype=np.float32) for k, v in weights.items() if k.startswith('mid.')}


def oracle(weights, dtype=torch.float32, pi_dim=4, seed=SEED):
    """OracleModel over the transition net's weights alone, its eight tensors as autograd leaves -> (orc, [leaf tensors in KEYS order])"""
    orc = OracleModel(mid_only(weights), PhiloxNoise(seed), pi_dim=pi_dim, dtype=dtype)
    params = [orc.w['mid.' + k].requires_grad_(True) for k in KEYS]
    return orc, params


def kl(mu1, lv1, mu2, lv2, omega):
    """torchutils.py:7-8, operation for operation"""
    return 0.5 * (lv2 - torch.log(omega) - lv1) + (torch.exp(lv1) + torch.square(mu1 - mu2)) / (2.0 * torch.exp(lv2) / omega) - 0.5


def f_mid(orc, b, stage, pass_=PASS_FE_T, sample=0, row_offset=0):
    """compute_loss_mid (torchloss.py:28-37) -> (F_mid [M], ps1_mean, ps1_logvar); omega: [M] values or a number"""
    s0, pi, qm, qv = (torch.as_tensor(x).to(orc.dtype) for x in b[:4])
    om = torch.as_tensor(np.asarray(b[4], dtype=np.float32)).to(orc.dtype).reshape(-1, 1)
    mean, lv = orc.transition(pi, s0, pass_, sample, stage, row_offset)
    return kl(qm, qv, mean, lv, om).sum(1), mean, lv


def grads(weights, b, stage, dtype=torch.float32, pi_dim=4, **key):
    """-> (F_mid [M], ps1_mean, ps1_logvar, {key: d mean(F_mid) / d tensor}) as numpy arrays of `dtype`"""
    orc, params = oracle(weights, dtype, pi_dim)
    Fm, mean, lv = f_mid(orc, b, stage, **key)
    Fm.mean().backward()
    return Fm.detach().numpy(), mean.detach().numpy(), lv.detach().numpy(), {k: p.grad.detach().numpy().copy() for k, p in zip(KEYS, params)}


def train(weights, b, stage, steps, lr, dtype=torch.float32, pi_dim=4, betas=(0.9, 0.999), eps=1e-8):
    """`steps` calls of train_model_mid with torch.optim.Adam at one stage -> (ps1_mean per step [steps, M, 10], ps1_logvar per step,
    F_mid per step [steps, M], {key: weight}, {key: exp_avg}, {key: exp_avg_sq})"""
    orc, params = oracle(weights, dtype, pi_dim)
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
    means, lvs, Fs = [], [], []
    for _ in range(steps):
        opt.zero_grad()
        Fm, mean, lv = f_mid(orc, b, stage)
        Fm.mean().backward()
        opt.step()
        means.append(mean.detach().numpy().copy()); lvs.append(lv.detach().numpy().copy()); Fs.append(Fm.detach().numpy().copy())
    out = lambda f: {k: f(p).detach().numpy().copy() for k, p in zip(KEYS, params)}      # noqa: E731
    return (np.stack(means, 0), np.stack(lvs, 0), np.stack(Fs, 0), out(lambda p: p), out(lambda p: opt.state[p]['exp_avg']),
            out(lambda p: opt.state[p]['exp_avg_sq']))


def hidden(weights, b, stage, pi_dim=4, pass_=PASS_FE_T, sample=0, row_offset=0):
    """the fp64 oracle's three hidden pre-activations and keep masks (x 2), the masks applied where a layer feeds the next
    -> [(a [M,512], mask [M,512])] * 3"""
    orc = OracleModel(mid_only(weights), PhiloxNoise(SEED), pi_dim=pi_dim, dtype=torch.float64)
    M = b[0].shape[0]
    h = torch.cat([torch.as_tensor(b[1]).double(), torch.as_tensor(b[0]).double()], 1)
    out = []
    with torch.no_grad():
        for li, idx in enumerate((0, 3, 6)):
            a = F.linear(h, orc.w[f'mid.ps_net.{idx}.weight'], orc.w[f'mid.ps_net.{idx}.bias'])
            mask = orc._mask(PX.TAG_MID + li, M, 512, pass_, sample, stage, row_offset)
            out.append((a.numpy(), mask.numpy()))
            h = F.relu(a) * mask
    return out


def preact_margin(weights, b, stage, pi_dim=4, **key):
    """min |hidden pre-activation| of the fp64 oracle over the batch: an fp32 evaluation whose ReLU decisions could differ from fp64's
    (margin below ~1e-5) would make a gradient comparison measure the flip, not the kernel"""
    return float(min(np.abs(a).min() for a, _ in hidden(weights, b, stage, pi_dim, **key)))


def flat(d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in KEYS])
