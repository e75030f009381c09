"""Test-side restatement of train_model_top (/root/reference/src/torchloss.py:65-74) on the CPU oracle: OracleModel.encode_s
(oracle/efe_oracle.py) is torch functional ops on `orc.w`, so requires_grad_ on the six top.* tensors gives the reference's gradients by
autograd and lets torch.optim.Adam run on them, in fp32 (the restatement) or fp64 (the reference the kernels' error is measured against).
Shared by tests/test_train_top_cpu.py (bit-exact against the reference fixture) and tests/test_train_top_gpu.py (the engine against it)."""
import numpy as np
import torch

from oracle.efe_oracle import OracleModel

KEYS = ('qpi_net.0.weight', 'qpi_net.0.bias', 'qpi_net.2.weight', 'qpi_net.2.bias', 'qpi_net.4.weight', 'qpi_net.4.bias')      # parameters() order


def batch(seed, M, A=4):
    """s [M,10], log_Ppi [M,A] (the log of a softmax of a fixed draw, as a planner's action posterior), float32"""
    r = np.random.RandomState(seed)
    s = r.randn(M, 10).astype(np.float32)
    z = torch.from_numpy((2.0 * r.randn(M, A)).astype(np.float32))
    log_Ppi = torch.log(torch.softmax(z, dim=1) + 1e-15).numpy().astype(np.float32)
    return s, log_Ppi


def top_only(weights):
    """the habit net's tensors, copied: OracleModel wraps fp32 arrays without a copy and torch.optim.Adam updates in place"""
    return {k: np.array(v, dtype=np.float32) for k, v in weights.items() if k.startswith('top.')}


def oracle(weights, dtype=torch.float32, pi_dim=4):
    """OracleModel over the habit net's weights alone, its six tensors as autograd leaves -> (orc, [leaf tensors in KEYS order])"""
    orc = OracleModel(top_only(weights), None, pi_dim=pi_dim, dtype=dtype)
    params = [orc.w['top.' + k].requires_grad_(True) for k in KEYS]
    return orc, params


def kl_pi(orc, s, log_Ppi):
    """compute_loss_top's kl_div_pi (torchloss.py:19-26)"""
    _, Qpi, log_Qpi = orc.encode_s(torch.as_tensor(s))
    return torch.sum(Qpi * (log_Qpi - torch.as_tensor(log_Ppi).to(orc.dtype)), dim=1)


def grads(weights, s, log_Ppi, dtype=torch.float32, pi_dim=4):
    """-> (kl_pi [M], {key: d mean(kl_pi) / d tensor}) as numpy arrays of `dtype`"""
    orc, params = oracle(weights, dtype, pi_dim)
    kl = kl_pi(orc, s, log_Ppi)
    kl.mean().backward()
    return kl.detach().numpy(), {k: p.grad.detach().numpy().copy() for k, p in zip(KEYS, params)}


def train(weights, s, log_Ppi, steps, lr, dtype=torch.float32, pi_dim=4, betas=(0.9, 0.999), eps=1e-8):
    """`steps` calls of train_model_top with torch.optim.Adam -> (kl_pi per step [steps, M], {key: weight}, {key: exp_avg}, {key: exp_avg_sq})"""
    orc, params = oracle(weights, dtype, pi_dim)
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
    kls = []
    for _ in range(steps):
        opt.zero_grad()
        kl = kl_pi(orc, s, log_Ppi)
        kl.mean().backward()
        opt.step()
        kls.append(kl.detach().numpy().copy())
    out = lambda f: {k: f(p).detach().numpy().copy() for k, p in zip(KEYS, params)}      # noqa: E731
    return np.stack(kls, 0), out(lambda p: p), out(lambda p: opt.state[p]['exp_avg']), out(lambda p: opt.state[p]['exp_avg_sq'])


def preact_margin(weights, s, pi_dim=4):
    """min |hidden pre-activation| of the fp64 oracle over the batch: an fp32 evaluation whose ReLU decisions could differ from fp64's
    (margin below ~1e-5) would make a gradient comparison measure the flip, not the kernel"""
    w = {k: torch.as_tensor(np.asarray(v, dtype=np.float32)).double() for k, v in top_only(weights).items()}
    x = torch.as_tensor(s).double()
    a1 = torch.nn.functional.linear(x, w['top.qpi_net.0.weight'], w['top.qpi_net.0.bias'])
    a2 = torch.nn.functional.linear(torch.relu(a1), w['top.qpi_net.2.weight'], w['top.qpi_net.2.bias'])
    return float(min(a1.abs().min(), a2.abs().min()))


def flat(d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in KEYS])
