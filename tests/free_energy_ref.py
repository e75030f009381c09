"""Test-side restatement of the training-side free energy (/root/reference/src/torchloss.py, train.py:104-123) on the CPU oracle
(oracle/efe_oracle.py OracleModel, fp32 or fp64), in the reference's torch operation order.  Shared by tests/test_free_energy_cpu.py
(bit-exact against the reference fixtures) and tests/test_free_energy_gpu.py (the engine against it).  Pass ids 9-12 are
csrc/philox.h's PASS_FE_Q0, _Q1, _T and _DOWN."""
import numpy as np
import torch

from oracle import efe_oracle as EO

PASS_FE_Q0, PASS_FE_Q1, PASS_FE_T, PASS_FE_DOWN = 9, 10, 11, 12
OMEGA_PARAMS = (1.0, 25.0, 5.0, 1.5)
FIELDS = ('F_top', 'kl_pi', 'kl_pi_anal', 'Qpi', 'omega', 'F_mid', 'kl_s_mid', 'kl_s_mid_anal', 'ps1', 'ps1_mean', 'ps1_logvar',
          'F_down', 'nlogpo1', 'kl_s', 'kl_s_anal', 'kl_naive', 'kl_naive_anal', 'po1', 'qs1', 's0', 'qs1_mean', 'qs1_logvar')


def kl(mu1, lv1, mu2, lv2, omega):
    """torchutils.py:7-8 (mu2 = lv2 = 0.0 for the naive prior: exp(0) = 1)"""
    e2 = torch.exp(lv2) if torch.is_tensor(lv2) else torch.ones((), dtype=mu1.dtype)
    return 0.5 * (lv2 - torch.log(omega) - lv1) + (torch.exp(lv1) + torch.square(mu1 - mu2)) / (2.0 * e2 / omega) - 0.5


def compute_omega(kl_pi, a, b, c, d):
    """torchloss.py:8-9"""
    return a * (1.0 - 1.0 / (1.0 + torch.exp(-(kl_pi - b) / c))) + d


def gamma_branch(gamma):
    """which formula compute_loss_down (torchloss.py:67-72) takes: torch compares its fp32 gamma tensor with the Python floats in fp32"""
    g = torch.tensor(gamma, dtype=torch.float32)
    return 'naive' if bool(g <= 0.05) else 'prior' if bool(g >= 0.95) else 'mixture'


def loss_down_F(logpo1, kl_s, kl_naive, gamma, beta_s, beta_o, dtype):
    g = torch.tensor(np.float32(gamma), dtype=torch.float32).to(dtype)
    bs, bo = torch.tensor(np.float32(beta_s)).to(dtype), torch.tensor(np.float32(beta_o)).to(dtype)
    br = gamma_branch(gamma)
    if br == 'naive':
        return -bo * logpo1 + bs * kl_naive
    if br == 'prior':
        return -bo * logpo1 + bs * kl_s
    return -bo * logpo1 + bs * (g * kl_s + (1.0 - g) * kl_naive)


def nlogpo1_of(o1, po1):
    """-sum over (C, H, W) of torchloss.py:62 (the displacements as fp32 sees them, EO._displacements)"""
    d, d1 = EO._displacements(1e-5)
    return -torch.sum(o1 * torch.log(d + po1) + (1 - o1) * torch.log(d1 - po1), dim=[1, 2, 3])


def free_energy(orc, o0, o1, pi0, log_Ppi, gamma, beta_s=1.0, beta_o=1.0, omega=None, omega_params=OMEGA_PARAMS, stage=0, ro=0):
    """-> dict FIELDS -> tensor in orc.dtype.  omega: None = derived, a float = every row, else [M] values"""
    dt = orc.dtype
    o0, o1, pi0, log_Ppi = (torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dt) for x in (o0, o1, pi0, log_Ppi))
    M = o0.shape[0]
    r = {}
    s0, _, _ = orc.encoder_with_sample(o0, PASS_FE_Q0, 0, stage, ro)
    _, Qpi, log_Qpi = orc.encode_s(s0)
    kl_pi_anal = Qpi * (log_Qpi - log_Ppi)
    kl_pi = torch.sum(kl_pi_anal, dim=1)
    if omega is None:
        w = compute_omega(kl_pi, *omega_params).reshape(-1, 1)
    elif np.ndim(omega) == 0:
        w = torch.full((M, 1), float(np.float32(omega)), dtype=dt)
    else:
        w = torch.as_tensor(np.asarray(omega, dtype=np.float32)).to(dt).reshape(-1, 1)
    qs1_mean, qs1_logvar = orc.encoder(o1, PASS_FE_Q1, 0, stage, ro)
    ps1, ps1_mean, ps1_logvar = orc.transition_with_sample(pi0, s0, PASS_FE_T, 0, stage, ro)
    kl_s_mid_anal = kl(qs1_mean, qs1_logvar, ps1_mean, ps1_logvar, w)
    kl_s_mid = torch.sum(kl_s_mid_anal, dim=1)
    qm, qv = orc.encoder(o1, PASS_FE_DOWN, 0, stage, ro)
    qs1 = orc.reparameterize(qm, qv, PASS_FE_DOWN, 0, stage, ro)
    po1 = orc.decoder(qs1, PASS_FE_DOWN, 0, stage, ro)
    nl = nlogpo1_of(o1, po1)
    kl_naive_anal = kl(qm, qv, 0.0, 0.0, w)
    kl_naive = torch.sum(kl_naive_anal, dim=1)
    kl_s_anal = kl(qm, qv, ps1_mean, ps1_logvar, w)
    kl_s = torch.sum(kl_s_anal, dim=1)
    r.update(F_top=kl_pi, kl_pi=kl_pi, kl_pi_anal=kl_pi_anal, Qpi=Qpi, omega=w.reshape(-1), F_mid=kl_s_mid, kl_s_mid=kl_s_mid,
             kl_s_mid_anal=kl_s_mid_anal, ps1=ps1, ps1_mean=ps1_mean, ps1_logvar=ps1_logvar,
             F_down=loss_down_F(-nl, kl_s, kl_naive, gamma, beta_s, beta_o, dt), nlogpo1=nl, kl_s=kl_s, kl_s_anal=kl_s_anal,
             kl_naive=kl_naive, kl_naive_anal=kl_naive_anal, po1=po1, qs1=qs1, s0=s0, qs1_mean=qs1_mean, qs1_logvar=qs1_logvar)
    return r
