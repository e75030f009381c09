"""Timing of one whole training step (daimc_amd.loss.train_step -> efe_train_step) beside the five public calls it replaces -> one JSON
line on stdout, and the same record in profiles/train_step_bench.json with --write (or at --out).

Legs per batch size M (default 50, the reference's batch, and 1024), each a window of --steps consecutive calls between two HIP events
after --warmup calls, reported as milliseconds per call (median / min / max of --repeats windows; DESIGN.md section 7f's protocol):
  step       : loss.train_step (one engine call; derived omega, the statistics written into a caller's tensor)
  sequence   : encoder_with_sample(o0), train_model_top, compute_omega in torch on the device, encoder(o1), train_model_mid,
               train_model_down -- the loop body of train.py:111-126 as five engine calls, in the same process on the same build
  train_down : loss.train_model_down alone (the largest part of either), also timed on a build without the step: --tag parent
Both step legs run at the Python level, because that is where the five calls' marshalling lives; the learning rates are 1e-6 so that the
weights stay where they are while the windows run.  No speed ratio is a gate.

Usage:  python tools/train_step_bench.py [--sizes 50,1024] [--steps 20] [--warmup 3] [--tag name] [--write] [--out path.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_step_bench.json')


def inputs(seed, M):
    g = torch.Generator().manual_seed(seed)
    o0, o1 = ((torch.rand(M, 1, 64, 64, generator=g) < 0.1).float() for _ in range(2))
    pi0 = torch.eye(4)[torch.randint(0, 4, (M,), generator=g)]
    return o0, o1, pi0, torch.log_softmax(torch.randn(M, 4, generator=g), 1)


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
    ap.add_argument('--tag', default='', help='a name for this build in the record (e.g. parent)')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_step_bench needs a HIP device')
    import daimc_amd
    from daimc_amd import loss
    from daimc_amd.model import PASS_FE_Q0, PASS_FE_Q1
    from oracle import synth
    res = {'metric': 'train_step_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'tag': args.tag, 'legs': {}}
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=1, init_weights=False)
    m.load_flat_weights(synth.make_weights(1234, 1.15))
    m.gamma, m.beta_s, m.beta_o = 0.5, 1.0, 1.0          # Python floats, as the Trainer keeps them: no leg fetches a device scalar
    opts = {'top': daimc_amd.Adam(m.model_top, lr=1e-6), 'mid': daimc_amd.Adam(m.model_mid, lr=1e-6), 'down': daimc_amd.Adam(m.model_down, lr=1e-6)}
    for M in (int(v) for v in args.sizes.split(',')):
        o0, o1, pi0, lp = (t.to('cuda:0') for t in inputs(100 + M, M))
        means = torch.zeros(8, device='cuda:0')
        pm, pv = 0.5 * torch.randn(M, 10, device='cuda:0'), 0.5 * torch.randn(M, 10, device='cuda:0')
        om = 1.5 + torch.rand(M, device='cuda:0')

        def sequence():
            qs0, _, _ = m.model_down.encoder_with_sample(o0, pass_=PASS_FE_Q0)
            kl = loss.train_model_top(m.model_top, qs0, lp, opts['top'])
            omega = loss.compute_omega(kl, *loss.OMEGA_PARAMS)
            qm, qv = m.model_down.encoder(o1, pass_=PASS_FE_Q1)
            mean, lv = loss.train_model_mid(m.model_mid, qs0, qm, qv, pi0, omega, opts['mid'])
            return loss.train_model_down(m.model_down, o1, mean, lv, omega, opts['down'])
        legs = {'train_down': lambda: loss.train_model_down(m.model_down, o1, pm, pv, om, opts['down'])}
        if hasattr(loss, 'train_step'):
            legs['step'] = lambda: loss.train_step(m, o0, o1, pi0, lp, opts, means=means)
            legs['sequence'] = sequence
        for name, fn in legs.items():
            t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
            res['legs'][f'{name}_M{M}'] = {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1]}
        if 'step' in legs:
            a, b = res['legs'][f'step_M{M}']['ms_per_call_median'], res['legs'][f'sequence_M{M}']['ms_per_call_median']
            res['legs'][f'step_over_sequence_M{M}'] = a / b
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
