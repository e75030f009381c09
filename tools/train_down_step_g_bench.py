"""Timing of ModelDown's training step at every admitted geometry (daimc_amd.loss.train_model_down_g -> efe_train_down_g: efe_down_grad_g's
row groups, k_adam_down, k_repack_down_g of csrc/train_down_g.hip) -> one JSON line on stdout, and the same record in
profiles/train_down_step_g_bench.json with --write (or at --out).

Geometries 3 x 84 x 84 (pi 3) and 1 x 64 x 64 (pi 4); batch sizes M (default 50, the reference's batch, and 1024).  Legs, each a window of
--steps consecutive calls between two HIP events after --warmup calls, reported as milliseconds per call (median / min / max of --repeats
windows; tools/train_down_bench.py's protocol):
  grad_g      : torch.ops.efe_g.down_grad -- the gradient alone
  train_g     : torch.ops.efe_g.train_down -- the gradient, Adam over all parameters, the repack; lr 1e-5 with the step count running
  adam_step_g : torch.ops.efe_g.down_adam_step alone on a fixed gradient: k_adam_down + the repack kernel of the geometry.  Its cost does
                not depend on M; the record carries the bytes the two kernels move at the least (step_bytes) and the rate against them
  train       : 1 x 64 x 64 only, torch.ops.efe.train_down from the same build: the fixed-geometry gradient in front of the same step
No speed ratio is a gate.

Usage:  python tools/train_down_step_g_bench.py [--sizes 50,1024] [--steps 20] [--warmup 3] [--write] [--out path.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_down_step_g_bench.json')
GEOS = [(3, 3, 84), (4, 1, 64)]


def extent4(R):
    for _ in range(4):
        R = (R - 3) // 2 + 1
    return R


def step_bytes(C, R):
    """bytes the optimiser step moves at the least on the generic path: k_adam_down reads gradient, both moments and the weight and writes the
    last three (7 x 4 P); k_repack_down_g reads the master copy once (the Linears packed in two forms, and qs_net.0, twice) and writes
    every packed buffer.  (1 x 64 x 64 runs k_repack_down: tools/train_down_bench.py step_bytes.)"""
    B, K = (16 if R == 32 else R // 4), 64 * extent4(R) ** 2
    F = 64 * B * B
    P = 201684 + 288 * C + 256 * K + 134400 + 257 * F + 92320 + 289 * C
    dense = [(256, 16), (256, 256), (256, 256), (256, 256), (256, 256), (32, 256), (256, K)]      # rows x padded K of the layers packed in both dense forms
    twice = sum(r * k + r for r, k in dense)
    packed = 2 * twice
    packed += 9 * (32 * 8 + 32 * 32 + 64 * 32 + 64 * 64) + 32 + 32 + 64 + 64 + 1152               # g_enc[0..3], g_enc1p
    packed += F * 256 + F + 9 * (64 * 64 + 64 * 64 + 32 * 64) + 64 + 64 + 32 + 1152                # g_fc4, g_ct[0..2], g_wf
    return {'P': P, 'adam': 7 * 4 * P, 'repack_read': 4 * (P + twice + 288 * C), 'repack_write': 4 * packed,
            'total': 4 * (8 * P + twice + 288 * C + packed)}


def inputs(seed, M, C, R):
    g = torch.Generator().manual_seed(seed)
    o1 = (torch.rand(M, C, R, R, generator=g) < 0.1).float()
    pm, pv = 0.5 * torch.randn(M, 10, generator=g), 0.5 * torch.randn(M, 10, generator=g)
    om = 1.5 + torch.rand(M, generator=g)
    return o1, pm, pv, om


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
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_down_step_g_bench needs a HIP device')
    import daimc_amd
    from oracle import synth
    gamma, beta_s, beta_o = 0.5, 1.0, 1.0
    res = {'metric': 'train_down_g_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'geometries': {}}
    for A, C, R in GEOS:
        m = daimc_amd.ActiveInferenceModel(10, A, gamma, beta_s, beta_o, colour_channels=C, resolution=R, device='cuda:0', seed=1, init_weights=False)
        m.load_flat_weights(synth.make_weights(1234, 1.15, A, C, R))
        e = m._ready()
        sb = step_bytes(C, R)
        NP = int(e.lib.efe_param_count(e.ctx, b'down_g'))
        assert NP == sb['P'], (NP, sb['P'])
        rec = {'step_bytes': sb if (C, R) != (1, 64) else {'P': NP, 'adam': 7 * 4 * NP}, 'legs': {}}
        ea, es, g = torch.zeros(NP, device='cuda:0'), torch.zeros(NP, device='cuda:0'), 1e-3 * torch.randn(NP, device='cuda:0')
        step = [0]
        G = torch.ops.efe_g
        for M in (int(v) for v in args.sizes.split(',')):
            o1, pm, pv, om = (t.to('cuda:0') for t in inputs(100 + M, M, C, R))

            def train_g():
                step[0] += 1
                return G.train_down(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None, ea, es, 1e-5, 0.9, 0.999, 1e-8, step[0])

            def step_g():
                step[0] += 1
                G.down_adam_step(e.h, g, ea, es, 1e-5, 0.9, 0.999, 1e-8, step[0])

            def train_64():
                step[0] += 1
                return e.ops.train_down(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None, ea, es, 1e-5, 0.9, 0.999, 1e-8, step[0])
            legs = {'grad_g': lambda: G.down_grad(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None), 'train_g': train_g,
                    'adam_step_g': step_g}
            if (C, R) == (1, 64):
                legs['train'] = train_64
            for name, fn in legs.items():
                t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
                leg = {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1]}
                if name == 'adam_step_g' and 'total' in rec['step_bytes']:
                    leg['achieved_TB_per_s'] = sb['total'] / (t[len(t) // 2] * 1e-3) / 1e12
                rec['legs'][f'{name}_M{M}'] = leg
        res['geometries'][f'{C}x{R}x{R}'] = rec
        del m
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
