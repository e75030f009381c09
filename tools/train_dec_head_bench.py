"""Timing of the backward of the reconstruction loss through the whole decoder (daimc_amd.loss.grad_decoder -> efe_dec_grad,
csrc/train_dec_head.hip + csrc/train_dec.hip) -> one JSON line on stdout, and the same record in profiles/train_dec_head_bench.json with
--write (or at --out).

Legs per batch size M (default 50, the reference's batch, and 1024), each a window of --steps consecutive calls between two HIP events
after --warmup calls, reported as milliseconds per call (median / min / max of --repeats windows):
  engine    : torch.ops.efe.dec_grad (forward with the four dropout masks and stored activations, loss, data and weight gradients of
              the eight layers, slab sums)
  autograd  : the reference's own path on the same GPU -- po_net as a plain torch.nn.Sequential (four Linear + ReLU + Dropout(0.5) in
              train mode, Unflatten, four ConvTranspose2d with ReLU / Sigmoid) on cuda:0, the binary cross entropy of torchloss.py:45-46,
              (beta_o / M * nlogpo1.sum()).backward()
No speed ratio is a gate.

Usage:  python tools/train_dec_head_bench.py [--sizes 50,1024] [--steps 20] [--warmup 3] [--write] [--out path.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_dec_head_bench.json')


def inputs(seed, M):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(M, 10, generator=g)
    o1 = (torch.rand(M, 1, 64, 64, generator=g) < 0.1).float()
    return s, o1


def window_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='50,1024')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-autograd', action='store_true')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_dec_head_bench needs a HIP device')
    import daimc_amd
    from oracle import synth
    w = synth.make_weights(1234, 1.15)
    res = {'metric': 'dec_grad_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'legs': {}}
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=1, init_weights=False)
    m.load_flat_weights(w)
    e = m._ready()
    for M in (int(v) for v in args.sizes.split(',')):
        s, o1 = (t.to('cuda:0') for t in inputs(100 + M, M))
        legs = {'engine': lambda: e.ops.dec_grad(e.h, s, o1, -1.0, 1.0, 1, 3, 12, 0, 0, False)}
        if not args.no_autograd:
            nn = torch.nn
            CT, R, L, D = nn.ConvTranspose2d, nn.ReLU, nn.Linear, nn.Dropout
            net = nn.Sequential(L(10, 256), R(), D(0.5), L(256, 256), R(), D(0.5), L(256, 256), R(), D(0.5), L(256, 16384), R(), D(0.5),
                                nn.Unflatten(1, (64, 16, 16)), CT(64, 64, 3, 1, 1), R(), CT(64, 64, 3, 2, 1, 1), R(), CT(64, 32, 3, 2, 1, 1), R(),
                                CT(32, 1, 3, 1, 1), nn.Sigmoid()).to('cuda:0')
            net.load_state_dict({k: torch.from_numpy(np.array(w['down.po_net.' + k])) for k in net.state_dict()})
            net.train()
            x = s.clone().requires_grad_(True)

            def autograd_call():
                net.zero_grad()
                x.grad = None
                p = net(x)
                bce = o1 * torch.log(1e-5 + p) + (1 - o1) * torch.log(1e-5 + 1 - p)
                nl = -torch.sum(bce, dim=[1, 2, 3])
                (nl.sum() * (1.0 / M)).backward()
                return nl
            legs['autograd'] = autograd_call
        for name, fn in legs.items():
            t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
            res['legs'][f'{name}_M{M}'] = {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1]}
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
