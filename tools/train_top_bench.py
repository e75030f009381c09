"""Timing of one habit-network training step (daimc_amd.loss.train_model_top -> efe_train_top: k_top_grad + k_adam) -> one JSON line on
stdout, and the same record in profiles/train_top_bench.json with --write.

Legs per batch size M (default 50, 64 and 4096), each a window of --steps consecutive steps (>= 200) between two HIP events after
--warmup steps, reported as milliseconds per step:
  engine    : daimc_amd.loss.train_model_top with a daimc_amd.Adam (two launches per step)
  autograd  : the reference's own path on the same GPU -- its qpi_net as a plain torch.nn.Sequential on cuda:0, torch.optim.Adam,
              train_model_top of torchloss.py:65-74 (zero_grad, compute_loss_top, F.mean().backward(), step)
  top_grad, adam_step : the two engine calls alone, back to back on the stream (launch-bound at these sizes)
Kernel times proper come from a `rocprofv3 --kernel-trace` run of this tool at ONE size (`--sizes M --no-autograd`): --kernel-trace
<csv> of a later invocation merges the median duration of k_top_grad / k_adam / k_slab_sum from that trace under "kernels_M<M>".

Usage:  python tools/train_top_bench.py [--sizes 50,64,4096] [--steps 200] [--warmup 20] [--write] [--merge-only --kernel-trace M=path.csv ...]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_top_bench.json')


def batch(seed, M, A=4):
    r = np.random.RandomState(seed)
    s = r.randn(M, 10).astype(np.float32)
    z = torch.from_numpy((2.0 * r.randn(M, A)).astype(np.float32))
    return torch.from_numpy(s), torch.log(torch.softmax(z, dim=1) + 1e-15)


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


def kernel_medians(path):
    """{kernel: {'median_us', 'min_us', 'calls'}} of the training kernels in a rocprofv3 kernel trace csv"""
    calls = {}
    for r in csv.DictReader(open(path)):
        name = r['Kernel_Name'].replace('void efe::', '').replace('efe::', '').split('(')[0]
        if name in ('k_top_grad', 'k_adam', 'k_slab_sum'):
            calls.setdefault(name, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    return {k: {'median_us': float(np.median(v)), 'min_us': float(min(v)), 'calls': len(v)} for k, v in calls.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='50,64,4096')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-autograd', action='store_true')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--merge-only', action='store_true', help='no timing: merge --kernel-trace tables into the existing record')
    ap.add_argument('--kernel-trace', action='append', default=[], metavar='M=CSV')
    args = ap.parse_args()
    if args.merge_only:
        res = json.load(open(OUT))
        for spec in args.kernel_trace:
            M, path = spec.split('=', 1)
            res[f'kernels_M{M}'] = kernel_medians(path)
        with open(OUT, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
        print(json.dumps(res))
        return
    if not torch.cuda.is_available():
        raise SystemExit('train_top_bench needs a HIP device')
    import daimc_amd
    from oracle import synth
    w = synth.make_weights(1234, 1.15)
    res = {'metric': 'train_model_top_ms_per_step', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'lr': 1e-4,
           'device': torch.cuda.get_device_name(0), 'legs': {}}
    for M in (int(v) for v in args.sizes.split(',')):
        s, lp = (t.to('cuda:0') for t in batch(100 + M, M))
        m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=1, init_weights=False)
        m.load_flat_weights(w)
        opt = daimc_amd.Adam(m.model_top, lr=1e-4)
        e = m._ready()
        legs = {'engine': lambda: daimc_amd.loss.train_model_top(m.model_top, s, lp, opt)}
        g = daimc_amd.loss.grad_top(m.model_top, s, lp)[1]
        flat = torch.cat([v.reshape(-1) for v in g.values()]).contiguous()
        ea, es = torch.zeros_like(flat), torch.zeros_like(flat)
        legs['top_grad'] = lambda: e.ops.top_grad(e.h, s, lp)
        legs['adam_step'] = lambda: e.ops.adam_step(e.h, 'top', flat, ea, es, 1e-4, 0.9, 0.999, 1e-8, 1)
        if not args.no_autograd:
            net = torch.nn.Sequential(torch.nn.Linear(10, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(),
                                      torch.nn.Linear(128, 4)).to('cuda:0')
            net.load_state_dict({k[len('top.qpi_net.'):]: torch.from_numpy(np.array(v)) for k, v in w.items() if k.startswith('top.')})
            topt = torch.optim.Adam(net.parameters(), lr=1e-4)

            def autograd_step():
                topt.zero_grad()
                q = torch.nn.functional.softmax(net(s), dim=-1)
                F = torch.sum(q * (torch.log(q + 1e-20) - lp), dim=1)
                F.mean().backward()
                topt.step()
                return F
            legs['autograd'] = autograd_step
        for name, fn in legs.items():
            t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
            res['legs'][f'{name}_M{M}'] = {'ms_per_step_median': t[len(t) // 2], 'ms_per_step_min': t[0], 'ms_per_step_max': t[-1]}
    if args.write and os.path.exists(OUT):          # keep kernel tables merged by earlier invocations
        res.update({k: v for k, v in json.load(open(OUT)).items() if k.startswith('kernels_M')})
    for spec in args.kernel_trace:
        M, path = spec.split('=', 1)
        res[f'kernels_M{M}'] = kernel_medians(path)
    line = json.dumps(res)
    if args.write:
        with open(OUT, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
