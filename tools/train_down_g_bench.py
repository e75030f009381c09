"""Timing of the gradient of F_down for all of ModelDown at run-time geometry (daimc_amd.loss.grad_down_g -> efe_down_grad_g, and
loss.grad_encoder_g -> efe_enc_grad_g: csrc/train_enc_g.hip around csrc/train_dec_head_g.hip + csrc/train_dec_g.hip) -> one JSON line on
stdout, and the same record in profiles/train_down_g_bench.json with --write (or at --out).

Steps, each a window of --steps consecutive calls between two HIP events after --warmup calls, reported as milliseconds per call
(median / min / max of --repeats windows), per batch size M (default 50, the reference's batch, and 1024), at 3 x 84 x 84 (the Animal-AI
size) and at 1 x 64 x 64:
    down_g        : torch.ops.efe_g.down_grad (per row group the encoder's training forward, the sample, the decoder's forward and backward,
                    F_down's terms, the gradient at the latent, the encoder's backward; then the slab sums)
    enc_g         : torch.ops.efe_g.enc_grad alone (training forward and backward of qs_net for a given upstream pair)
    dec_g         : torch.ops.efe_g.dec_grad alone, so that the encoder's own share of down_g is visible
    autograd_down : the reference's own path on the same GPU -- qs_net and po_net as plain torch.nn.Sequential in train mode on cuda:0,
                    compute_loss_down's expressions (torchloss.py:39-63), F_down.mean().backward()
    autograd_enc  : qs_net alone, ((mean * d_mean).sum() + (logvar * d_logvar).sum()).backward()
    down, enc     : (1 x 64 x 64 only) torch.ops.efe.down_grad / enc_grad, the kernels specialised to that geometry: the price of run-time geometry
Every step runs in a process of its own under its own time limit (--step-timeout seconds); a step that fails or runs out of time is
recorded as such and ends the run: nothing more is started on the device behind it.  No speed ratio is a gate.

Usage:  python tools/train_down_g_bench.py [--sizes 50,1024] [--steps 20] [--warmup 3] [--write] [--out path.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_down_g_bench.json')
G84, G64 = (3, 3, 84), (4, 1, 64)
STEPS = [(G84, leg) for leg in ('down_g', 'enc_g', 'dec_g', 'autograd_down', 'autograd_enc')]
STEPS += [(G64, leg) for leg in ('down_g', 'down', 'enc_g', 'enc', 'dec_g', 'autograd_down', 'autograd_enc')]


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


def torch_nets(w, C, R):
    """qs_net and po_net of the reference's ModelDown (torchmodel.py:84-128) as plain torch modules with the weights `w`"""
    import numpy as np
    import torch
    nn = torch.nn
    B, S3 = (16, 1) if R == 32 else (R // 4, 2)
    H = R
    for _ in range(4):
        H = (H - 3) // 2 + 1
    enc = nn.Sequential(nn.Conv2d(C, 32, 3, 2), nn.ReLU(), nn.Conv2d(32, 32, 3, 2), nn.ReLU(), nn.Conv2d(32, 64, 3, 2), nn.ReLU(), nn.Conv2d(64, 64, 3, 2),
                        nn.ReLU(), nn.Flatten(), nn.Linear(64 * H * H, 256), nn.ReLU(), nn.Dropout(0.5), nn.Linear(256, 256), nn.ReLU(), nn.Dropout(0.5),
                        nn.Linear(256, 256), nn.ReLU(), nn.Dropout(0.5), nn.Linear(256, 20))
    dense = [l for i, o in ((10, 256), (256, 256), (256, 256), (256, 64 * B * B)) for l in (nn.Linear(i, o), nn.ReLU(), nn.Dropout(0.5))]
    CT = nn.ConvTranspose2d
    dec = nn.Sequential(*dense, nn.Unflatten(1, (64, B, B)), CT(64, 64, 3, 1, 1), nn.ReLU(), CT(64, 64, 3, 2, 1, 1), nn.ReLU(),
                        CT(64, 32, 3, S3, 1, S3 - 1), nn.ReLU(), CT(32, C, 3, 1, 1), nn.Sigmoid())
    for net, pre in ((enc, 'down.qs_net.'), (dec, 'down.po_net.')):
        net.load_state_dict({k[len(pre):]: torch.from_numpy(np.array(v)) for k, v in w.items() if k.startswith(pre)})
        net.to('cuda:0').train()
    return enc, dec


def run_step(geo, leg, M, args):
    """one step, in this process -> {'ms_per_call_median': ..., 'ms_per_call_min': ..., 'ms_per_call_max': ...}"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('train_down_g_bench needs a HIP device')
    from oracle import synth
    _, C, R = geo
    w = synth.make_weights(1234, 1.15, *geo)
    g = torch.Generator().manual_seed(100 + M)
    dev = 'cuda:0'
    o1 = (torch.rand(M, C, R, R, generator=g) < 0.1).float().to(dev)
    pm, pv = (0.5 * torch.randn(M, 10, generator=g)).to(dev), (0.5 * torch.randn(M, 10, generator=g)).to(dev)
    om = (1.5 + torch.rand(M, generator=g)).to(dev)
    gm, gv = (torch.randn(M, 10, generator=g) / M).to(dev), (torch.randn(M, 10, generator=g) / M).to(dev)
    s = torch.randn(M, 10, generator=g).to(dev)
    gamma, beta_s, beta_o = 0.5, 1.0, 1.0
    if leg.startswith('autograd'):
        enc, dec = torch_nets(w, C, R)
        wcol = om.reshape(M, 1)

        def kl(mu1, lv1, mu2, lv2):
            return 0.5 * (lv2 - torch.log(wcol) - lv1) + (torch.exp(lv1) + torch.square(mu1 - mu2)) / (2.0 * torch.exp(lv2) / wcol) - 0.5
        if leg == 'autograd_enc':
            def fn():
                enc.zero_grad()
                mean, lv = torch.split(enc(o1), 10, dim=1)
                ((mean * gm).sum() + (lv * gv).sum()).backward()
        else:
            def fn():
                enc.zero_grad()
                dec.zero_grad()
                mean, lv = torch.split(enc(o1), 10, dim=1)
                qs1 = torch.randn_like(mean) * torch.exp(0.5 * lv) + mean
                p = dec(qs1)
                logpo1 = torch.sum(o1 * torch.log(1e-5 + p) + (1 - o1) * torch.log(1e-5 + 1 - p), dim=[1, 2, 3])
                kl_n = torch.sum(kl(mean, lv, 0.0 * mean, 0.0 * lv), dim=1)
                kl_s = torch.sum(kl(mean, lv, pm, pv), dim=1)
                (-beta_o * logpo1 + beta_s * (gamma * kl_s + (1.0 - gamma) * kl_n)).mean().backward()
    else:
        import daimc_amd
        m = daimc_amd.ActiveInferenceModel(10, geo[0], gamma, beta_s, beta_o, colour_channels=C, resolution=R, device=dev, seed=1, init_weights=False)
        m.load_flat_weights(w)
        e = m._ready()
        G = torch.ops.efe_g
        legs = {'down_g': lambda: G.down_grad(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None),
                'enc_g': lambda: G.enc_grad(e.h, o1, gm, gv, 1, 3, 12, 0, 0, False),
                'dec_g': lambda: G.dec_grad(e.h, s, o1, -1.0, beta_o, 1, 3, 12, 0, 0, False),
                'down': lambda: e.ops.down_grad(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None),
                'enc': lambda: e.ops.enc_grad(e.h, o1, gm, gv, 1, 3, 12, 0, 0, False)}
        fn = legs[leg]
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
    res = {'metric': 'down_grad_g_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'legs': {}}
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
                    print(f"{name}: {res['legs'][name]['ms_per_call_median']:.3f} ms", file=sys.stderr, flush=True)
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
