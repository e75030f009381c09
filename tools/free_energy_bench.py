"""Timing of the training-side free energy (daimc_amd.free_energy -> efe_free_energy) -> one JSON line on stdout.

Legs, each timed with HIP events after warm-up (the CPU leg with a wall clock):
  engine   : one free_energy call per size (default M = 1000 = train.py's TEST_SIZE, and 19 200)
  stitched : the same values from the existing network calls (encoder_with_sample, encode_s, encoder, transition_with_sample,
             encoder + reparameterize + decoder) plus torch arithmetic on the GPU -- what a user could do without the feature
  cpu      : the torch-CPU restatement (tests/free_energy_ref.py on oracle/efe_oracle.py) at --threads threads, on --cpu-rows rows

Usage:  python tools/free_energy_bench.py [--sizes 1000,19200] [--reps 5] [--cpu-rows 200] [--threads 16] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import daimc_amd                                   # noqa: E402
from daimc_amd.model import PASS_FE_Q0, PASS_FE_Q1, PASS_FE_T, PASS_FE_DOWN   # noqa: E402
from oracle import synth                           # noqa: E402


def inputs(M, dev, A=4):
    fr = torch.from_numpy(synth.make_frames(5, 64))
    idx = torch.arange(M) % 64
    o0 = fr[idx].to(dev)
    o1 = fr[(idx + 1) % 64].to(dev)
    pi0 = torch.eye(A, device=dev)[torch.arange(M, device=dev) % A]
    log_Ppi = torch.log_softmax(torch.linspace(-1, 1, M * A, device=dev).reshape(M, A), dim=1)
    return o0, o1, pi0, log_Ppi


def stitched(m, o0, o1, pi0, log_Ppi, stage, params=(1.0, 25.0, 5.0, 1.5)):
    """the free energy from the network-level calls and torch ops on the device (torchloss.py expressions)"""
    md = m.model_down
    s0, _, _ = md.encoder_with_sample(o0, stage=stage, pass_=PASS_FE_Q0)
    _, Qpi, logQ = m.model_top.encode_s(s0)
    kl_pi = torch.sum(Qpi * (logQ - log_Ppi), dim=1)
    a, b, c, d = params
    w = (a * (1.0 - 1.0 / (1.0 + torch.exp(-(kl_pi - b) / c))) + d).reshape(-1, 1)
    qm, qv = md.encoder(o1, stage=stage, pass_=PASS_FE_Q1)
    _, pm, pv = m.model_mid.transition_with_sample(pi0, s0, stage=stage, pass_=PASS_FE_T)

    def kl(m1, l1, m2, l2):
        return 0.5 * (l2 - torch.log(w) - l1) + (torch.exp(l1) + torch.square(m1 - m2)) / (2.0 * torch.exp(l2) / w) - 0.5
    F_mid = torch.sum(kl(qm, qv, pm, pv), dim=1)
    qm2, qv2 = md.encoder(o1, stage=stage, pass_=PASS_FE_DOWN)
    qs1 = md.reparameterize(qm2, qv2, stage=stage, pass_=PASS_FE_DOWN)
    po1 = md.decoder(qs1, stage=stage, pass_=PASS_FE_DOWN)
    logpo1 = torch.sum(o1 * torch.log(1e-5 + po1) + (1 - o1) * torch.log(1e-5 + 1 - po1), dim=[1, 2, 3])
    z = torch.zeros_like(qm2)
    kln, kls = torch.sum(kl(qm2, qv2, z, z), dim=1), torch.sum(kl(qm2, qv2, pm, pv), dim=1)
    g = m.gamma
    F_down = -m.beta_o * logpo1 + m.beta_s * (g * kls + (1.0 - g) * kln)
    return kl_pi, F_mid, F_down


def gpu_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000,19200')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-rows', type=int, default=200)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device='cuda:0', seed=1, init_weights=False)
    m.load_flat_weights(synth.make_weights(1234, 1.15))
    res = {'metric': 'free_energy', 'legs': {}}
    for M in (int(s) for s in args.sizes.split(',')):
        o0, o1, pi0, lp = inputs(M, m.device)
        eng = gpu_ms(lambda: daimc_amd.free_energy(m, o0, o1, pi0, lp, stage=3), args.reps)
        sti = gpu_ms(lambda: stitched(m, o0, o1, pi0, lp, 3), args.reps)
        res['legs'][f'engine_M{M}'] = {'ms_median': eng[0], 'ms_min': eng[1], 'rows_per_s': M / (eng[0] / 1e3)}
        res['legs'][f'stitched_M{M}'] = {'ms_median': sti[0], 'ms_min': sti[1], 'rows_per_s': M / (sti[0] / 1e3)}
        del o0, o1, pi0, lp
    if not args.no_cpu:
        import free_energy_ref as FR
        from oracle import efe_oracle as EO
        torch.set_num_threads(args.threads)
        n = args.cpu_rows
        o0, o1, pi0, lp = (t.cpu().numpy() for t in inputs(n, 'cpu'))
        orc = EO.OracleModel(synth.make_weights(1234, 1.15), EO.PhiloxNoise(1))
        with torch.no_grad():
            FR.free_energy(orc, o0[:2], o1[:2], pi0[:2], lp[:2], 0.5)
            t = time.perf_counter()
            FR.free_energy(orc, o0, o1, pi0, lp, 0.5)
            dt = time.perf_counter() - t
        res['legs'][f'cpu_torch_{args.threads}t_M{n}'] = {'ms': dt * 1e3, 'rows_per_s': n / dt}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
