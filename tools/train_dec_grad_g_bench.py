"""Timing of the whole decoder's backward at run-time geometry (daimc_amd.loss.grad_decoder_g -> efe_dec_grad_g, csrc/train_dec_head_g.hip +
csrc/train_dec_g.hip) -> one JSON line on stdout, and the same record in profiles/train_dec_grad_g_bench.json with --write (or at --out).

Steps, each a window of --steps consecutive calls between two HIP events after --warmup calls, reported as milliseconds per call
(median / min / max of --repeats windows), per batch size M (default 50, the reference's batch, and 1024), at 3 x 84 x 84 (the Animal-AI
size) and at 1 x 64 x 64:
    engine_g    : torch.ops.efe_g.dec_grad (training forward of head and tail with stored activations, loss, data and weight gradients, slab sums)
    autograd    : the reference's own path on the same GPU -- po_net as a plain torch.nn.Sequential (Linear / ReLU / Dropout(0.5) x 4, Unflatten,
                  four ConvTranspose2d with ReLU / Sigmoid) in train mode on cuda:0, the binary cross entropy of torchloss.py:45-46,
                  (beta_o / M * nlogpo1.sum()).backward()
    tail_g      : torch.ops.efe_g.dec_tail_grad alone on an h4 of the same size, so that the head's own share is visible
    engine      : (1 x 64 x 64 only) torch.ops.efe.dec_grad, the kernels specialised to that geometry (csrc/train_dec_head.hip, csrc/train_dec.hip)
Every step runs in a process of its own under its own time limit (--step-timeout seconds); a step that fails or runs out of time is
recorded as such and ends the run: nothing more is started on the device behind it.  No speed ratio is a gate.

Usage:  python tools/train_dec_grad_g_bench.py [--sizes 50,1024] [--steps 20] [--warmup 3] [--write] [--out path.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_dec_grad_g_bench.json')
STEPS = [((3, 3, 84), 'engine_g'), ((3, 3, 84), 'autograd'), ((3, 3, 84), 'tail_g'), ((4, 1, 64), 'engine_g'), ((4, 1, 64), 'autograd'),
         ((4, 1, 64), 'engine'), ((4, 1, 64), 'tail_g')]


def window_ms(fn, steps, warmup):
    import torch
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


def run_step(geo, leg, M, args):
    """one step, in this process -> {'ms_per_call_median': ..., 'ms_per_call_min': ..., 'ms_per_call_max': ...}"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('train_dec_grad_g_bench needs a HIP device')
    from oracle import synth
    _, C, R = geo
    B, S3 = (16, 1) if R == 32 else (R // 4, 2)
    w = synth.make_weights(1234, 1.15, *geo)
    g = torch.Generator().manual_seed(100 + M)
    s = torch.randn(M, 10, generator=g).to('cuda:0')
    h4 = (2.0 * torch.relu(torch.randn(M, 64 * B * B, generator=g)) * (torch.rand(M, 64 * B * B, generator=g) < 0.5).float()).to('cuda:0')
    o1 = (torch.rand(M, C, R, R, generator=g) < 0.1).float().to('cuda:0')
    if leg == 'autograd':
        nn = torch.nn
        dense = [l for i, o in ((10, 256), (256, 256), (256, 256), (256, 64 * B * B)) for l in (nn.Linear(i, o), nn.ReLU(), nn.Dropout(0.5))]
        CT = nn.ConvTranspose2d
        net = nn.Sequential(*dense, nn.Unflatten(1, (64, B, B)), CT(64, 64, 3, 1, 1), nn.ReLU(), CT(64, 64, 3, 2, 1, 1), nn.ReLU(),
                            CT(64, 32, 3, S3, 1, S3 - 1), nn.ReLU(), CT(32, C, 3, 1, 1), nn.Sigmoid()).to('cuda:0')
        net.load_state_dict({k[len('down.po_net.'):]: torch.from_numpy(np.array(v)) for k, v in w.items() if k.startswith('down.po_net.')})
        net.train()
        x = s.clone().requires_grad_(True)

        def fn():
            net.zero_grad()
            x.grad = None
            p = net(x)
            bce = o1 * torch.log(1e-5 + p) + (1 - o1) * torch.log(1e-5 + 1 - p)
            nl = -torch.sum(bce, dim=[1, 2, 3])
            (nl.sum() * (1.0 / M)).backward()
            return nl
    else:
        import daimc_amd
        m = daimc_amd.ActiveInferenceModel(10, geo[0], 0.5, 1.0, 1.0, colour_channels=C, resolution=R, device='cuda:0', seed=1, init_weights=False)
        m.load_flat_weights(w)
        e = m._ready()
        if leg == 'tail_g':
            def fn():
                return torch.ops.efe_g.dec_tail_grad(e.h, h4, o1, -1.0, 1.0, False)
        else:
            op = torch.ops.efe_g.dec_grad if leg == 'engine_g' else e.ops.dec_grad

            def fn():
                return op(e.h, s, o1, -1.0, 1.0, 1, 3, 12, 0, 0, False)
    t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
    return {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1], 'device': torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='50,1024')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--step-timeout', type=float, default=240.0)
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--one', default=None, help='internal: run the one step "pi,C,R,leg,M" in this process and print its record')
    args = ap.parse_args()
    if args.one:
        a, c, r, leg, M = args.one.split(',')
        print(json.dumps(run_step((int(a), int(c), int(r)), leg, int(M), args)))
        return 0
    res = {'metric': 'dec_grad_g_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'legs': {}}
    rc = 0
    for geo, leg in STEPS:
        for M in (int(v) for v in args.sizes.split(',')):
            name = f'{leg}_{geo[1]}x{geo[2]}x{geo[2]}_M{M}'
            cmd = [sys.executable, os.path.abspath(__file__), '--one', f'{geo[0]},{geo[1]},{geo[2]},{leg},{M}', '--steps', str(args.steps),
                   '--warmup', str(args.warmup), '--repeats', str(args.repeats)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
                if p.returncode == 0:
                    res['legs'][name] = json.loads(p.stdout.strip().splitlines()[-1])
                    res['device'] = res['legs'][name].pop('device')
                    continue
                res['legs'][name] = {'error': f'exit status {p.returncode}', 'stderr': p.stderr[-400:]}
            except subprocess.TimeoutExpired:
                res['legs'][name] = {'error': f'no result within {args.step_timeout:g} s'}
            rc = 1
            break
        if rc:
            break
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)
    return rc


if __name__ == '__main__':
    sys.exit(main())
