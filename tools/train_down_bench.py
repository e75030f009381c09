"""Timing of the gradient of F_down for all of ModelDown (daimc_amd.loss.grad_down -> efe_down_grad, csrc/train_enc.hip around
csrc/train_dec_head.hip + csrc/train_dec.hip) -> one JSON line on stdout, and the same record in profiles/train_down_bench.json with
--write (or at --out).

Legs per batch size M (default 50, the reference's batch, and 1024), each a window of --steps consecutive calls between two HIP events
after --warmup calls, reported as milliseconds per call (median / min / max of --repeats windows):
  down      : torch.ops.efe.down_grad (per 64-row group the encoder's training forward, the sample, the decoder's forward and backward,
              the gradient at the latent and the encoder's backward; slab sums)
  decoder   : torch.ops.efe.dec_grad alone on the same rows in the same run: the share of `down` the decoder takes
  encoder   : torch.ops.efe.enc_grad alone (training forward and backward of qs_net for a given upstream pair)
  autograd  : the reference's own path on the same GPU -- qs_net and po_net built HERE from torch.nn layers (qs_net.9 = Linear(576, 256),
              Dropout(0.5) in train mode), compute_loss_down's expressions (torchloss.py:39-63) and F.mean().backward()
  train     : torch.ops.efe.train_down -- `down`, then Adam over the 4 787 125 parameters and the repack of every packed forward form
              (csrc/train_down.hip), at lr 1e-5 with the step count running
  adam_step : torch.ops.efe.down_adam_step alone on a fixed gradient: k_adam_down + k_repack_down.  Its cost does not depend on M; the
              record carries the byte count of the two kernels (STEP_BYTES below) and the rate achieved against it
The two step legs are skipped (and `down` still timed) on a build without the ops: the parent commit, timed in the same session with
--tag parent --no-autograd.
No speed ratio is a gate.

Usage:  python tools/train_down_bench.py [--sizes 50,1024] [--steps 20] [--warmup 3] [--tag name] [--write] [--out path.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'train_down_bench.json')


def step_bytes():
    """bytes the optimiser step moves at the least: k_adam_down reads gradient, both moments and the weight and writes the last three
    (7 x 4 P); k_repack_down reads the raw copy once (the small Linears, packed in two forms, twice) and writes every packed buffer"""
    P = 4787125
    dense = [(256, 16), (256, 256), (256, 256), (256, 256), (256, 256), (32, 256), (256, 576)]      # rows x padded K of the layers packed in both dense forms
    packed = 2 * sum(r * k + r for r, k in dense)
    packed += 288 + 32 + 9 * (32 * 32 + 64 * 32 + 64 * 64) + 32 + 64 + 64                         # the encoder's convolutions
    packed += 16384 * 256 + 16384 + 16 * (64 * 64 + 64 * 64 + 32 * 64) + 64 + 64 + 32 + 288         # po_net.9, the Winograd / F(2,2) matrices, the final taps
    twice = sum(r * k + r for r, k in dense)
    return {'adam': 7 * 4 * P, 'repack_read': 4 * (P + twice), 'repack_write': 4 * packed, 'total': 4 * (8 * P + twice + packed)}


def inputs(seed, M):
    g = torch.Generator().manual_seed(seed)
    o1 = (torch.rand(M, 1, 64, 64, generator=g) < 0.1).float()
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


def autograd_nets(w):
    nn = torch.nn
    CV, CT, R, L, D = nn.Conv2d, nn.ConvTranspose2d, nn.ReLU, nn.Linear, nn.Dropout
    qs = nn.Sequential(CV(1, 32, 3, 2), R(), CV(32, 32, 3, 2), R(), CV(32, 64, 3, 2), R(), CV(64, 64, 3, 2), R(), nn.Flatten(), L(576, 256), R(), D(0.5),
                       L(256, 256), R(), D(0.5), L(256, 256), R(), D(0.5), L(256, 20))
    po = nn.Sequential(L(10, 256), R(), D(0.5), L(256, 256), R(), D(0.5), L(256, 256), R(), D(0.5), L(256, 16384), R(), D(0.5),
                       nn.Unflatten(1, (64, 16, 16)), CT(64, 64, 3, 1, 1), R(), CT(64, 64, 3, 2, 1, 1), R(), CT(64, 32, 3, 2, 1, 1), R(),
                       CT(32, 1, 3, 1, 1), nn.Sigmoid())
    for net, name in ((qs, 'qs_net'), (po, 'po_net')):
        net.load_state_dict({k: torch.from_numpy(np.array(w[f'down.{name}.{k}'])) for k in net.state_dict()})
        net.to('cuda:0').train()
    return qs, po


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='50,1024')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-autograd', action='store_true')
    ap.add_argument('--tag', default='', help='a name for this build in the record (e.g. parent)')
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_down_bench needs a HIP device')
    import daimc_amd
    from oracle import synth
    w = synth.make_weights(1234, 1.15)
    gamma, beta_s, beta_o = 0.5, 1.0, 1.0
    res = {'metric': 'down_grad_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'tag': args.tag, 'step_bytes': step_bytes(), 'legs': {}}
    m = daimc_amd.ActiveInferenceModel(10, 4, gamma, beta_s, beta_o, device='cuda:0', seed=1, init_weights=False)
    m.load_flat_weights(w)
    e = m._ready()
    for M in (int(v) for v in args.sizes.split(',')):
        o1, pm, pv, om = (t.to('cuda:0') for t in inputs(100 + M, M))
        s = torch.randn(M, 10, device='cuda:0')
        gm, gv = torch.randn(M, 10, device='cuda:0') / M, torch.randn(M, 10, device='cuda:0') / M
        legs = {'down': lambda: e.ops.down_grad(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None),
                'decoder': lambda: e.ops.dec_grad(e.h, s, o1, -1.0, beta_o, 1, 3, 12, 0, 0, False),
                'encoder': lambda: e.ops.enc_grad(e.h, o1, gm, gv, 1, 3, 12, 0, 0, False)}
        if not args.no_autograd:
            qs, po = autograd_nets(w)
            wcol = om.reshape(M, 1)

            def kl(mu1, lv1, mu2, lv2):
                return 0.5 * (lv2 - torch.log(wcol) - lv1) + (torch.exp(lv1) + torch.square(mu1 - mu2)) / (2.0 * torch.exp(lv2) / wcol) - 0.5
            zero = torch.zeros((), device='cuda:0')

            def autograd_call():
                qs.zero_grad()
                po.zero_grad()
                mean, lv = torch.split(qs(o1), 10, dim=1)
                p = po(torch.randn_like(mean) * torch.exp(lv * 0.5) + mean)
                logpo1 = torch.sum(o1 * torch.log(1e-5 + p) + (1 - o1) * torch.log(1e-5 + 1 - p), dim=[1, 2, 3])
                F = -beta_o * logpo1 + beta_s * (gamma * torch.sum(kl(mean, lv, pm, pv), dim=1) + (1.0 - gamma) * torch.sum(kl(mean, lv, zero, zero), dim=1))
                F.mean().backward()
                return F
            legs['autograd'] = autograd_call
        if hasattr(e.lib, 'efe_train_down'):
            NP = 4787125
            ea, es, g = torch.zeros(NP, device='cuda:0'), torch.zeros(NP, device='cuda:0'), 1e-3 * torch.randn(NP, device='cuda:0')
            step = [0]

            def train_call():
                step[0] += 1
                return e.ops.train_down(e.h, o1, pm, pv, gamma, beta_s, beta_o, 0, om, 1.0, 1, 3, 12, 0, 0, None, ea, es, 1e-5, 0.9, 0.999, 1e-8, step[0])

            def step_call():
                step[0] += 1
                e.ops.down_adam_step(e.h, g, ea, es, 1e-5, 0.9, 0.999, 1e-8, step[0])
            legs['train'] = train_call
            legs['adam_step'] = step_call
        for name, fn in legs.items():
            t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
            res['legs'][f'{name}_M{M}'] = {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1]}
            if name == 'adam_step':
                res['legs'][f'{name}_M{M}']['achieved_TB_per_s'] = res['step_bytes']['total'] / (t[len(t) // 2] * 1e-3) / 1e12
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
