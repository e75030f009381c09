"""Timing of one transition-network training step (daimc_amd.loss.train_model_mid -> efe_train_mid: k_mid_grad + k_adam) -> one JSON line
on stdout, and the same record in profiles/train_mid_bench.json with --write (or at --out).

Legs per batch size M (default 50, the reference's batch, and 1024), each a window of --steps consecutive steps (>= 200) between two HIP
events after --warmup steps, reported as milliseconds per step:
  engine    : daimc_amd.loss.train_model_mid with a daimc_amd.Adam (two launches per step), one fixed stage
  autograd  : the reference's own path on the same GPU -- its ps_net as a plain torch.nn.Sequential with nn.Dropout(0.5) in train mode on
              cuda:0, torch.optim.Adam, train_model_mid of torchloss.py:76-88 (zero_grad, compute_loss_mid with its randn_like sample,
              F.mean().backward(), step)
  mid_grad, adam_step : the two engine calls alone, back to back on the stream
No speed ratio is a gate.  At M = 50 the call is latency-bound: four workgroups.

Usage:  python tools/train_mid_bench.py [--sizes 50,1024] [--steps 200] [--warmup 20] [--write] [--out path.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_mid_bench.json')


def batch_mid(seed, M, A=4):
    r = np.random.RandomState(seed)
    s0 = r.randn(M, 10).astype(np.float32)
    pi = np.eye(A, dtype=np.float32)[r.randint(0, A, M)]
    qm = r.randn(M, 10).astype(np.float32)
    qv = (0.5 * r.randn(M, 10) - 1.0).astype(np.float32)
    om = r.uniform(1.5, 2.5, M).astype(np.float32)
    return tuple(torch.from_numpy(x) for x in (s0, pi, qm, qv, om))


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
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-autograd', action='store_true')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_mid_bench needs a HIP device')
    import daimc_amd
    from oracle import synth
    w = synth.make_weights(1234, 1.15)
    res = {'metric': 'train_model_mid_ms_per_step', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'lr': 1e-4,
           'device': torch.cuda.get_device_name(0), 'legs': {}}
    for M in (int(v) for v in args.sizes.split(',')):
        s0, pi, qm, qv, om = (t.to('cuda:0') for t in batch_mid(100 + M, M))
        m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=1, init_weights=False)
        m.load_flat_weights(w)
        opt = daimc_amd.Adam(m.model_mid, lr=1e-4)
        e = m._ready()
        legs = {'engine': lambda: daimc_amd.loss.train_model_mid(m.model_mid, s0, qm, qv, pi, om, opt, stage=3)}
        g = daimc_amd.loss.grad_mid(m.model_mid, s0, qm, qv, pi, om, stage=3)[3]
        flat = torch.cat([v.reshape(-1) for v in g.values()]).contiguous()
        ea, es = torch.zeros_like(flat), torch.zeros_like(flat)
        legs['mid_grad'] = lambda: e.ops.mid_grad(e.h, s0, pi, qm, qv, 0, om, 1.0, 1, 3, 11, 0, 0)
        legs['adam_step'] = lambda: e.ops.adam_step(e.h, 'ps_net', flat, ea, es, 1e-4, 0.9, 0.999, 1e-8, 1)
        if not args.no_autograd:
            L, R, D = torch.nn.Linear, torch.nn.ReLU, torch.nn.Dropout
            net = torch.nn.Sequential(L(14, 512), R(), D(0.5), L(512, 512), R(), D(0.5), L(512, 512), R(), D(0.5), L(512, 20)).to('cuda:0')
            net.load_state_dict({k[len('mid.ps_net.'):]: torch.from_numpy(np.array(v)) for k, v in w.items() if k.startswith('mid.')})
            net.train()
            topt = torch.optim.Adam(net.parameters(), lr=1e-4)
            omc = om.reshape(-1, 1)

            def autograd_step():
                topt.zero_grad()
                mean, lv = torch.split(net(torch.cat([pi, s0], dim=1)), 10, dim=1)
                ps1 = torch.randn_like(mean) * torch.exp(lv * 0.5) + mean        # transition_with_sample draws it; the loss does not use it
                kl = 0.5 * (lv - torch.log(omc) - qv) + (torch.exp(qv) + torch.square(qm - mean)) / (2.0 * torch.exp(lv) / omc) - 0.5
                F = torch.sum(kl, dim=1)
                F.mean().backward()
                topt.step()
                return ps1
            legs['autograd'] = autograd_step
        for name, fn in legs.items():
            t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
            res['legs'][f'{name}_M{M}'] = {'ms_per_step_median': t[len(t) // 2], 'ms_per_step_min': t[0], 'ms_per_step_max': t[-1]}
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
