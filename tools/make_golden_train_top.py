"""Reference-captured fixture of the habit-network training step: tests/golden/train_top_g115.npz.

Runs only where the reference checkout exists.  The reference's own ModelTop (src/torchmodel.py:10-31), loaded with
oracle.synth.make_weights(1234, 1.15), is driven through src/torchloss.py's train_model_top with torch.optim.Adam(lr=1e-4) for three
steps on M = 17 rows of tests/train_ref.batch(117, 17).  Recorded: the inputs, kl_pi of every step, the gradients of step 1 (read from
.grad after the first call), and the weights, exp_avg and exp_avg_sq after step 3.  No noise is involved (the habit net has no dropout)
and no shim is needed beyond the cv2 stub that importing src.torchmodel takes.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_top.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import synth                              # noqa: E402
from oracle.make_golden import GOLD, REF              # noqa: E402
import train_ref as TR                                # noqa: E402

WSEED, GAIN, BSEED, M, STEPS, LR = 1234, 1.15, 117, 17, 3, 1e-4


def main():
    sys.path.insert(0, REF)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    from src.torchmodel import ModelTop
    import src.torchloss as loss

    weights = synth.make_weights(WSEED, GAIN)
    top = ModelTop(10, 4)
    top.load_state_dict({k: torch.from_numpy(np.array(weights['top.' + k], dtype=np.float32)) for k in TR.KEYS})
    assert [n for n, _ in top.named_parameters()] == list(TR.KEYS)
    opt = torch.optim.Adam(top.parameters(), lr=LR)
    s, log_Ppi = TR.batch(BSEED, M)
    st, lt = torch.from_numpy(s), torch.from_numpy(log_Ppi)
    out = {}
    for step in range(STEPS):
        kl = loss.train_model_top(model_top=top, s=st, log_Ppi=lt, optimizer=opt)
        out[f'kl_pi_{step + 1}'] = kl.detach().numpy().copy()
        if step == 0:
            for k, p in top.named_parameters():
                out['grad1.' + k] = p.grad.detach().numpy().copy()
    for k, p in top.named_parameters():
        out['w3.' + k] = p.detach().numpy().copy()
        out['exp_avg3.' + k] = opt.state[p]['exp_avg'].numpy().copy()
        out['exp_avg_sq3.' + k] = opt.state[p]['exp_avg_sq'].numpy().copy()
    meta = dict(wseed=WSEED, gain=GAIN, batch_seed=BSEED, M=M, steps=STEPS, lr=LR, betas=[0.9, 0.999], eps=1e-8, torch=torch.__version__,
                shim=['cv2 stub'])
    path = os.path.join(GOLD, 'train_top_g115.npz')
    np.savez_compressed(path, s=s, log_Ppi=log_Ppi, meta=json.dumps(meta), **{k: v.astype(np.float32) for k, v in out.items()})
    print(path, os.path.getsize(path), 'bytes; mean kl_pi per step', [float(out[f'kl_pi_{i + 1}'].mean()) for i in range(STEPS)])


if __name__ == '__main__':
    main()
