"""Reference-captured fixture of the transition-network training step: tests/golden/train_mid_g115.npz.

Runs only where the reference checkout exists.  The reference's own ModelMid (src/torchmodel.py:34-66) in train mode, loaded with
oracle.synth.make_weights(1234, 1.15), is driven through src/torchloss.py's train_model_mid with torch.optim.Adam(lr=1e-4) for three
steps on M = 17 rows of tests/train_mid_ref.batch_mid(117, 17), omega as an fp32 [M, 1] tensor.  Its nn.Dropout layers and the
randn_like of transition_with_sample are fed by oracle/make_golden.py's Injector (Philox noise consumed by the patched F.dropout /
torch.randn_like in the reference's own draw order; imported, oracle/ itself is unchanged): p_trans(PASS_FE_T, 0, STAGE, 0) before every
step, one fixed stage for all three, engine seed 7.

Recorded: the inputs, ps1_mean / ps1_logvar of every step, the gradients of step 1 (read from .grad after the first call), and the
weights, exp_avg and exp_avg_sq after step 3.  The small tensors (ps_net.0.weight, every bias, ps_net.9.weight) are stored whole; of the
two 512 x 512 tensors the rows SLICE x columns IDX and rows IDX x columns SLICE, SLICE = the first and the last 16-wide tile, IDX = SLICE
plus every 64th index, and the float64 sum and sum of squares of the full tensor.  Only data goes into the file.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_mid.py
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
from oracle import synth                                        # noqa: E402
from oracle.make_golden import GOLD, REF, Injector              # noqa: E402
import train_mid_ref as TM                                      # noqa: E402

WSEED, GAIN, BSEED, M, STEPS, LR, NSEED, STAGE = 1234, 1.15, 117, 17, 3, 1e-4, TM.SEED, 3
SLICE = list(range(16)) + list(range(496, 512))
IDX = sorted(set(SLICE) | set(range(0, 512, 64)))
BIG = ('ps_net.3.weight', 'ps_net.6.weight')


def record(out, name, key, arr):
    """a tensor of the fixture: whole, or (512 x 512) its two slices and its float64 sum / sum of squares"""
    arr = np.asarray(arr, dtype=np.float32)
    if key in BIG:
        out[f'{name}.{key}.rows'] = arr[np.ix_(SLICE, IDX)].copy()
        out[f'{name}.{key}.cols'] = arr[np.ix_(IDX, SLICE)].copy()
        out[f'{name}.{key}.sums'] = np.array([arr.astype(np.float64).sum(), np.square(arr.astype(np.float64)).sum()], dtype=np.float64)
    else:
        out[f'{name}.{key}'] = arr.copy()


def main():
    sys.path.insert(0, REF)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    import torch.nn.functional as F
    from src.torchmodel import ModelMid
    import src.torchloss as loss

    weights = synth.make_weights(WSEED, GAIN)
    mid = ModelMid(10, 4)
    mid.load_state_dict({k: torch.from_numpy(np.array(weights['mid.' + k], dtype=np.float32)) for k in TM.KEYS})
    mid.train()
    assert [n for n, _ in mid.named_parameters()] == list(TM.KEYS)
    opt = torch.optim.Adam(mid.parameters(), lr=LR)
    s0, pi, qm, qv, om = TM.batch_mid(BSEED, M)
    t = lambda x: torch.from_numpy(x)                           # noqa: E731
    inj = Injector(NSEED)
    drop0, randn0 = F.dropout, torch.randn_like
    F.dropout, torch.randn_like = inj.dropout, inj.randn_like
    out = {}
    try:
        for step in range(STEPS):
            inj.p_trans(TM.PASS_FE_T, 0, STAGE, 0)
            mean, lv = loss.train_model_mid(model_mid=mid, s0=t(s0), qs1_mean=t(qm), qs1_logvar=t(qv), Ppi_sampled=t(pi),
                                            omega=t(om).reshape(-1, 1), optimizer=opt)
            assert not inj.q, inj.q
            out[f'ps1_mean_{step + 1}'] = mean.detach().numpy().astype(np.float32).copy()
            out[f'ps1_logvar_{step + 1}'] = lv.detach().numpy().astype(np.float32).copy()
            if step == 0:
                for k, p in mid.named_parameters():
                    record(out, 'grad1', k, p.grad.detach().numpy())
    finally:
        F.dropout, torch.randn_like = drop0, randn0
    for k, p in mid.named_parameters():
        record(out, 'w3', k, p.detach().numpy())
        record(out, 'exp_avg3', k, opt.state[p]['exp_avg'].numpy())
        record(out, 'exp_avg_sq3', k, opt.state[p]['exp_avg_sq'].numpy())
    meta = dict(wseed=WSEED, gain=GAIN, batch_seed=BSEED, M=M, steps=STEPS, lr=LR, betas=[0.9, 0.999], eps=1e-8, nseed=NSEED, stage=STAGE,
                pass_id=TM.PASS_FE_T, sample=0, row_offset=0, slice=SLICE, idx=IDX, big=list(BIG), torch=torch.__version__,
                shim=['cv2 stub', 'F.dropout / torch.randn_like patched by oracle.make_golden.Injector', 'omega passed as a tensor [M,1]'])
    path = os.path.join(GOLD, 'train_mid_g115.npz')
    np.savez_compressed(path, s0=s0, pi=pi, qs1_mean=qm, qs1_logvar=qv, omega=om, meta=json.dumps(meta), **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
