"""Reference-captured fixtures of the training-side free energy: tests/golden/free_energy_<tag>.npz.

Runs only where the reference checkout exists (/root/reference).  Reuses oracle/make_golden.py's load_reference (its three-line shim)
and Injector (Philox noise consumed by the patched F.dropout / torch.randn_like in the reference's own draw order) by import; oracle/
itself is unchanged.  The reference's src/torchloss.py then evaluates one training step (train.py:104-123) on M = 8 rows of Game frames
(oracle/env_oracle.py over its synthetic sprite bank), under three extra shims that its shipped code needs to run at all:
  * model.model_down.gamma / beta_s / beta_o are set as fp32 0-d tensors (ModelDown has none: train.py:101 would raise AttributeError);
  * during the capture torch.exp / torch.log accept a Python float as an fp32 0-d tensor (compute_loss_down passes 0.0, 0.0 to
    kl_div_loss_analytically_from_logvar_and_precision and torch.exp(0.0) raises TypeError; exp(0) = 1 exactly);
  * omega is passed as a tensor: compute_omega on the fp32 kl_div_pi tensor (train.py:118 hands it a numpy array), reshaped to [M, 1];
    the scalar case (the evaluation block's var_a / 2 + var_d) as an fp32 [M, 1] tensor of that value.
Noise: pass ids 9-12 (csrc/philox.h PASS_FE_Q0, _Q1, _T, _DOWN), sample 0, one stage.  compute_loss_down is re-run once per gamma
(0, f32(0.05), 0.5, f32(0.95), 1) with the same draws, so every branch of its gamma test is pinned.

Files: WSEED 1234 at gains 1.0 and 1.35 (oracle.synth.make_weights) and the 'sparse' stress family (oracle.synth.stress_weights).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_free_energy.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import philox as PX            # noqa: E402
from oracle import synth                   # noqa: E402
from oracle import env_oracle as ENV       # noqa: E402
from oracle.make_golden import GOLD, REF, load_reference, npy   # noqa: E402

PASS_FE_Q0, PASS_FE_Q1, PASS_FE_T, PASS_FE_DOWN = 9, 10, 11, 12
M, NSEED, STAGE, RO = 8, 2024, 7, 0
GAMMAS = [0.0, float(np.float32(0.05)), 0.5, float(np.float32(0.95)), 1.0]
GAMMA_MAIN, BETA_S, BETA_O = 0.5, 1.0, 1.0
OMEGA_PARAMS = (1.0, 25.0, 5.0, 1.5)
OMEGA_SCALAR = OMEGA_PARAMS[0] / 2.0 + OMEGA_PARAMS[3]


def batch(seed):
    """o0, o1 [M,1,64,64] (frames before / after one action of pi0), pi0 one-hot [M,4], log_Ppi [M,4] (a log-softmax of a fixed draw)"""
    imgs = ENV.sprite_bank()
    s, last_r = ENV.reset(seed, M, 0)
    o0 = ENV.render(s, last_r, imgs).transpose(0, 3, 1, 2).copy()
    acts = (PX.uniform_fill(seed, (M,), 61, 0.0, 1.0) * 4).astype(np.int64).clip(0, 3)
    ENV.step(seed, s, last_r, acts, 5, 1)
    o1 = ENV.render(s, last_r, imgs).transpose(0, 3, 1, 2).copy()
    pi0 = np.eye(4, dtype=np.float32)[acts]
    logits = torch.from_numpy(PX.uniform_fill(seed, (M, 4), 62, -2.0, 2.0))
    log_Ppi = torch.log(torch.softmax(logits, dim=1) + 1e-15)
    return o0, o1, pi0, log_Ppi.numpy()


def capture(weights, tag, meta):
    model, inj, _, _ = load_reference(weights, NSEED)
    sys.path.insert(0, REF)
    import src.torchloss as loss
    md = model.model_down
    md.beta_s = torch.tensor(BETA_S, dtype=torch.float32)
    md.beta_o = torch.tensor(BETA_O, dtype=torch.float32)
    o0, o1, pi0, log_Ppi = batch(NSEED)
    o0t, o1t, pi0t, lpt = (torch.from_numpy(x) for x in (o0, o1, pi0, log_Ppi))

    exp0, log0 = torch.exp, torch.log
    as_t = lambda x: torch.tensor(x, dtype=torch.float32) if isinstance(x, float) else x     # noqa: E731
    torch.exp = lambda x, *a, **k: exp0(as_t(x), *a, **k)
    torch.log = lambda x, *a, **k: log0(as_t(x), *a, **k)
    try:
        out = {}
        inj.p_enc(PASS_FE_Q0, 0, STAGE, RO)
        s0, _, _ = md.encoder_with_sample(o0t)
        F_top, kl_pi, kl_pi_anal, Qpi = loss.compute_loss_top(model.model_top, s0, lpt)
        omega = loss.compute_omega(kl_pi, *OMEGA_PARAMS).reshape(-1, 1)
        inj.p_enc(PASS_FE_Q1, 0, STAGE, RO, with_eps=False)
        qs1_mean, qs1_logvar = md.encoder(o1t)

        def mid(w):
            inj.p_trans(PASS_FE_T, 0, STAGE, RO)
            return loss.compute_loss_mid(model.model_mid, s0, pi0t, qs1_mean, qs1_logvar, w)

        def down(w, gamma):
            md.gamma = torch.tensor(gamma, dtype=torch.float32)
            inj.p_enc(PASS_FE_DOWN, 0, STAGE, RO)
            inj.p_dec(PASS_FE_DOWN, 0, STAGE, RO)
            return loss.compute_loss_down(md, o1t, ps1_mean, ps1_logvar, w)

        F_mid, (kl_s_mid, kl_s_mid_anal), ps1, ps1_mean, ps1_logvar = mid(omega)
        F_down, (nlogpo1, kl_s, kl_s_anal, kl_naive, kl_naive_anal), po1, qs1 = down(omega, GAMMA_MAIN)
        F_down_g = torch.stack([down(omega, g)[0] for g in GAMMAS], 0)
        w_sc = torch.full((M, 1), OMEGA_SCALAR, dtype=torch.float32)
        F_mid_sc = mid(w_sc)[0]
        F_down_sc = down(w_sc, GAMMA_MAIN)[0]
        assert not inj.q, inj.q
    finally:
        torch.exp, torch.log = exp0, log0
    out.update(s0=s0, F_top=F_top, kl_pi=kl_pi, kl_pi_anal=kl_pi_anal, Qpi=Qpi, omega=omega.reshape(-1), qs1_mean=qs1_mean,
               qs1_logvar=qs1_logvar, F_mid=F_mid, kl_s_mid=kl_s_mid, kl_s_mid_anal=kl_s_mid_anal, ps1=ps1, ps1_mean=ps1_mean,
               ps1_logvar=ps1_logvar, F_down=F_down, nlogpo1=nlogpo1, kl_s=kl_s, kl_s_anal=kl_s_anal, kl_naive=kl_naive,
               kl_naive_anal=kl_naive_anal, po1=po1, qs1=qs1, F_down_g=F_down_g, F_mid_sc=F_mid_sc, F_down_sc=F_down_sc)
    meta = dict(meta, nseed=NSEED, stage=STAGE, row_offset=RO, M=M, gamma=GAMMA_MAIN, gammas=GAMMAS, beta_s=BETA_S, beta_o=BETA_O,
                omega_params=OMEGA_PARAMS, omega_scalar=OMEGA_SCALAR, passes=[PASS_FE_Q0, PASS_FE_Q1, PASS_FE_T, PASS_FE_DOWN],
                torch=torch.__version__,
                shim=['cv2 stub', 'qs_net[9]=Linear(576,256)', 'precision=float32', 'model_down.gamma/beta_s/beta_o = fp32 0-d tensors',
                      'torch.exp/torch.log take a Python float as an fp32 0-d tensor (capture only)', 'omega passed as a tensor [M,1]'])
    arrs = {k: npy(v).astype(np.float32) for k, v in out.items()}
    path = os.path.join(GOLD, f'free_energy_{tag}.npz')
    np.savez_compressed(path, o0=o0.astype(np.float32), o1=o1.astype(np.float32), pi0=pi0, log_Ppi=log_Ppi, meta=json.dumps(meta), **arrs)
    print(path, os.path.getsize(path), 'bytes', 'F_down', arrs['F_down'][:3], 'omega', arrs['omega'][:3])


def main():
    torch.set_grad_enabled(False)
    for tag, gain in (('g100', 1.0), ('g135', 1.35)):
        capture(synth.make_weights(1234, gain), tag, dict(wseed=1234, gain=gain, family=''))
    capture(synth.stress_weights('sparse'), 'sparse', dict(wseed=0, gain=0.0, family='sparse'))


if __name__ == '__main__':
    main()
