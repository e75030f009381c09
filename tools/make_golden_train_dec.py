"""Reference-captured fixture of the decoder tail's backward: tests/golden/train_dec_g115.npz.

Runs only where the reference checkout exists.  The reference's own ModelDown (src/torchmodel.py:69-128), loaded with
oracle.synth.make_weights(1234, 1.15), is cut at the Unflatten: po_net[12:] (Unflatten, four ConvTranspose2d, ReLUs, Sigmoid; no Dropout
lies behind the cut, so nothing is injected) runs on tests/train_dec_ref.inputs(115, 1) with autograd, the loss is the reconstruction
term of compute_loss_down (src/torchloss.py:45-46) times beta_o / M = 1, and .backward() leaves the gradients.

Recorded: the inputs, nlogpo1, po1, d_h4 (the gradient of the Unflatten's input) and the gradients of the eight tensors, whole.  Only data
goes into the file.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_train_dec.py
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
from oracle.make_golden import GOLD, REF                        # noqa: E402
import train_dec_ref as TD                                      # noqa: E402

WSEED, GAIN, BSEED, M = 1234, 1.15, 115, 1


def main():
    sys.path.insert(0, REF)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    from src.torchmodel import ModelDown

    weights = synth.make_weights(WSEED, GAIN)
    down = ModelDown(10, 4, 1, 64)
    # (the decoder alone: the shipped encoder's first Linear does not take the 576 features its trunk emits, torchmodel.py:94)
    down.po_net.load_state_dict({k: torch.from_numpy(np.array(weights['down.po_net.' + k], dtype=np.float32)) for k in down.po_net.state_dict()})
    down.train()
    tail = down.po_net[12:]
    assert [n for n, _ in tail.named_parameters()] == [k[len('po_net.'):] for k in TD.KEYS]      # (a slice of a Sequential keeps the indices)
    h4, o1 = TD.inputs(BSEED, M)
    x = torch.from_numpy(h4.copy()).requires_grad_(True)
    o = torch.from_numpy(o1.copy())
    po1 = tail(x)
    displacement = 1e-5
    bin_cross_entr = o * torch.log(displacement + po1) + (1 - o) * torch.log(displacement + 1 - po1)
    logpo1 = torch.sum(bin_cross_entr, dim=[1, 2, 3])
    F = -1.0 * logpo1
    F.mean().backward()
    out = {'grad.' + k: p.grad.detach().numpy().astype(np.float32).copy() for k, (_, p) in zip(TD.KEYS, tail.named_parameters())}
    meta = dict(wseed=WSEED, gain=GAIN, batch_seed=BSEED, M=M, beta_o=1.0, torch=torch.__version__, shim=['cv2 stub'])
    path = os.path.join(GOLD, 'train_dec_g115.npz')
    np.savez_compressed(path, h4=h4, o1=o1, nlogpo1=(-logpo1).detach().numpy().copy(), po1=po1.detach().numpy().copy(),
                        d_h4=x.grad.detach().numpy().copy(), meta=json.dumps(meta), **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
