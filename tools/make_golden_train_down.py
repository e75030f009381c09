"""Reference-captured fixture of the gradient of F_down for all of ModelDown: tests/golden/train_down_g115.npz.

Runs only where the reference checkout exists.  The reference's own compute_loss_down (src/torchloss.py:39-63) and F.mean().backward()
(train_model_down, :90-98, without the optimiser) run on ModelDown in train mode, loaded with oracle.synth.make_weights(1234, 1.15), on
tests/train_down_ref.inputs(315, 2), under the shims of oracle/make_golden.py's load_reference (imported; oracle/ itself is unchanged)
and tools/make_golden_free_energy.py:
  * qs_net[9] = Linear(576, 256) (the shipped Linear(256, 256) does not take the 576 features its trunk emits),
  * F.dropout and torch.randn_like are fed by the Injector: the Philox masks of p_enc / p_dec(PASS_FE_DOWN, 0, STAGE, 0) and the Philox
    normals of the sample, consumed in the reference's own draw order, engine seed 7,
  * model_down.gamma / beta_s / beta_o are fp32 0-d tensors set on the module (the reference reads them from ModelDown, which has none),
  * during the capture torch.exp / torch.log accept a Python float as an fp32 0-d tensor (compute_loss_down passes 0.0 for the naive prior),
  * omega is passed as a tensor [M, 1].
One capture per gamma in GAMMAS (the three branches of compute_loss_down).

Recorded per gamma: F_down, nlogpo1, kl_s, kl_naive, qs1 whole, po1 and every one of the 32 gradients as the elements flat[::stride] of the
flattened tensor (stride 1 up to 1024 elements, 61 up to 62 464, else 1021: primes, so every row, channel and tap is reached), and for
every gradient the float64 sum and the float64 sum of absolute values of the whole tensor.  Only data goes into the file.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_down.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import synth                                        # noqa: E402
from oracle.make_golden import GOLD, REF, load_reference       # noqa: E402
import train_down_ref as TDN                                    # noqa: E402

WSEED, GAIN, BSEED, M, NSEED, STAGE = 1234, 1.15, 315, 2, TDN.SEED, 3
GAMMAS = (0.0, 0.5, 1.0)
BETA_S, BETA_O = 0.75, 1.25


def stride(n):
    return 1 if n <= 1024 else 61 if n <= 62464 else 1021


def main():
    weights = synth.make_weights(WSEED, GAIN)
    model, inj, _, _ = load_reference(weights, NSEED)
    sys.path.insert(0, REF)
    import src.torchloss as loss
    md = model.model_down
    md.train()
    assert [n for n, _ in md.named_parameters()] == list(TDN.KEYS)
    md.beta_s = torch.tensor(BETA_S, dtype=torch.float32)
    md.beta_o = torch.tensor(BETA_O, dtype=torch.float32)
    o1, pm, pv, om = TDN.inputs(BSEED, M)
    o1t, pmt, pvt = (torch.from_numpy(x.copy()) for x in (o1, pm, pv))
    w = torch.from_numpy(om.copy()).reshape(M, 1)
    exp0, log0 = torch.exp, torch.log
    as_t = lambda x: torch.tensor(x, dtype=torch.float32) if isinstance(x, float) else x     # noqa: E731
    torch.exp = lambda x, *a, **k: exp0(as_t(x), *a, **k)
    torch.log = lambda x, *a, **k: log0(as_t(x), *a, **k)
    out = {}
    try:
        for gi, gamma in enumerate(GAMMAS):
            md.gamma = torch.tensor(gamma, dtype=torch.float32)
            md.zero_grad()
            inj.p_enc(TDN.PASS_FE_DOWN, 0, STAGE, 0)
            inj.p_dec(TDN.PASS_FE_DOWN, 0, STAGE, 0)
            Fd, (nl, kl_s, _, kl_naive, _), po1, qs1 = loss.compute_loss_down(md, o1t, pmt.detach(), pvt.detach(), w.detach())
            assert not inj.q, inj.q
            Fd.mean().backward()
            n = lambda t: t.detach().numpy().astype(np.float32).copy()          # noqa: E731
            out.update({f'g{gi}.F_down': n(Fd), f'g{gi}.nlogpo1': n(nl), f'g{gi}.kl_s': n(kl_s), f'g{gi}.kl_naive': n(kl_naive), f'g{gi}.qs1': n(qs1),
                        f'g{gi}.po1': n(po1).reshape(-1)[::stride(po1.numel())].copy()})
            for k, (_, p) in zip(TDN.KEYS, md.named_parameters()):
                g = n(p.grad).reshape(-1)
                g64 = g.astype(np.float64)
                out[f'g{gi}.sums.{k}'] = np.array([g64.sum(), np.abs(g64).sum()], dtype=np.float64)
                out[f'g{gi}.grad.{k}'] = g[::stride(g.size)].copy()
    finally:
        torch.exp, torch.log = exp0, log0
    meta = dict(wseed=WSEED, gain=GAIN, batch_seed=BSEED, M=M, gammas=list(GAMMAS), beta_s=BETA_S, beta_o=BETA_O, nseed=NSEED, stage=STAGE,
                pass_id=TDN.PASS_FE_DOWN, sample=0, row_offset=0, strides='1 (n <= 1024), 61 (n <= 62464), 1021', torch=torch.__version__,
                shim=['cv2 stub', 'qs_net[9]=Linear(576,256)', 'F.dropout / torch.randn_like patched by oracle.make_golden.Injector',
                      'model_down.gamma/beta_s/beta_o = fp32 0-d tensors', 'torch.exp/torch.log take a Python float as an fp32 0-d tensor (capture only)',
                      'omega passed as a tensor [M,1]'])
    path = os.path.join(GOLD, 'train_down_g115.npz')
    np.savez_compressed(path, o1=o1, ps1_mean=pm, ps1_logvar=pv, omega=om, meta=json.dumps(meta), **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
