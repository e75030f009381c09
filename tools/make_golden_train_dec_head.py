"""Reference-captured fixture of the whole decoder's backward: tests/golden/train_dec_head_g115.npz.

Runs only where the reference checkout exists.  The reference's own ModelDown.po_net (src/torchmodel.py:106-128) in train mode, loaded
with oracle.synth.make_weights(1234, 1.15), runs on tests/train_dec_head_ref.inputs(215, 2) with autograd; its four nn.Dropout layers
are fed by oracle/make_golden.py's Injector (Philox masks consumed by the patched F.dropout in the reference's own draw order; imported,
oracle/ itself is unchanged): p_dec(PASS_FE_DOWN, 0, STAGE, 0), engine seed 7.  The loss is the reconstruction term of compute_loss_down
(src/torchloss.py:45-46) times beta_o = 1, and F.mean().backward() leaves the gradients.

Recorded whole: the inputs, nlogpo1, d_s, the gradients of po_net.0.weight, of the five biases of po_net.0 / .3 / .6 / .9 / .19 and of
po_net.13 / .15 / .17.bias.  Recorded subsampled: of po_net.3.weight and po_net.6.weight the rows 0::4, of po_net.9.weight the rows 0::61
(a stride coprime to 64 and 256 reaches every channel and pixel).  For every one of the 16 tensors the float64 sum and the float64 sum of
absolute values of the whole gradient.  Only data goes into the file.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_dec_head.py
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
import train_dec_head_ref as TH                                 # noqa: E402

WSEED, GAIN, BSEED, M, NSEED, STAGE = 1234, 1.15, 215, 2, TH.SEED, 3
ROWS = {'po_net.3.weight': 4, 'po_net.6.weight': 4, 'po_net.9.weight': 61}          # row strides of the subsampled tensors
WHOLE = ('po_net.0.weight', 'po_net.0.bias', 'po_net.3.bias', 'po_net.6.bias', 'po_net.9.bias', 'po_net.19.bias',
         'po_net.13.bias', 'po_net.15.bias', 'po_net.17.bias')


def main():
    sys.path.insert(0, REF)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    import torch.nn.functional as F
    from src.torchmodel import ModelDown

    weights = synth.make_weights(WSEED, GAIN)
    down = ModelDown(10, 4, 1, 64)
    # (the decoder alone: the shipped encoder's first Linear does not take the 576 features its trunk emits, torchmodel.py:94)
    down.po_net.load_state_dict({k: torch.from_numpy(np.array(weights['down.po_net.' + k], dtype=np.float32)) for k in down.po_net.state_dict()})
    down.train()
    assert ['po_net.' + n for n, _ in down.po_net.named_parameters()] == list(TH.KEYS)
    s, o1 = TH.inputs(BSEED, M)
    x = torch.from_numpy(s.copy()).requires_grad_(True)
    o = torch.from_numpy(o1.copy())
    inj = Injector(NSEED)
    drop0 = F.dropout
    F.dropout = inj.dropout
    try:
        inj.p_dec(TH.PASS_FE_DOWN, 0, STAGE, 0)
        po1 = down.po_net(x)
        assert not inj.q, inj.q
    finally:
        F.dropout = drop0
    displacement = 1e-5
    bin_cross_entr = o * torch.log(displacement + po1) + (1 - o) * torch.log(displacement + 1 - po1)
    logpo1 = torch.sum(bin_cross_entr, dim=[1, 2, 3])
    Fd = -1.0 * logpo1
    Fd.mean().backward()
    out = {}
    for k, (_, p) in zip(TH.KEYS, down.po_net.named_parameters()):
        g = p.grad.detach().numpy().astype(np.float32)
        g64 = g.astype(np.float64)
        out['sums.' + k] = np.array([g64.sum(), np.abs(g64).sum()], dtype=np.float64)
        if k in ROWS:
            out['grad.' + k] = g[0::ROWS[k]].copy()
        elif k in WHOLE:
            out['grad.' + k] = g.copy()
    meta = dict(wseed=WSEED, gain=GAIN, batch_seed=BSEED, M=M, beta_o=1.0, nseed=NSEED, stage=STAGE, pass_id=TH.PASS_FE_DOWN, sample=0,
                row_offset=0, row_stride=ROWS, whole=list(WHOLE), torch=torch.__version__,
                shim=['cv2 stub', 'F.dropout patched by oracle.make_golden.Injector'])
    path = os.path.join(GOLD, 'train_dec_head_g115.npz')
    np.savez_compressed(path, s=s, o1=o1, nlogpo1=(-logpo1).detach().numpy().copy(), d_s=x.grad.detach().numpy().copy(),
                        meta=json.dumps(meta), **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
