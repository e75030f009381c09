"""Timing of the epoch report -> one JSON line on stdout, and the same record in profiles/eval_report_bench.json with --write (or at --out).

Legs (milliseconds per call: device events around a window of `steps` calls after `warmup` calls, the median of `repeats` windows):
  eval_stats_M{M}   : loss.eval_stats over all four groups on synthetic arrays of M rows (the reward batch has M images): the four kernels
                      of csrc/eval.hip, no download
  free_energy_M{M}  : loss.free_energy on M rows on the same build (what the O(M^2) rank sweep is held against)
  report_G{G}       : Trainer.report on G test games: both batch producers, free_energy, imagine_future_from_o, eval_stats, ONE download
  evaluate_G{G}     : train.make_batch_random + Trainer.evaluate on G test games: the same block with a reduction and a download per number
                      and numpy's TC (no reward-transition test, no Spearman table)
The last two end in a download, so their windows include the host's wait.

Usage:  python tools/eval_report_bench.py [--sizes 1000,8192] [--games 1000] [--steps 20] [--warmup 3] [--repeats 3] [--write] [--out path.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'eval_report_bench.json')


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


def synthetic(M, dev):
    g = torch.Generator(device=dev).manual_seed(100 + M)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    fe = {k: rnd(M) for k in ('F_top', 'F_mid', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'kl_pi')}
    fe.update(kl_s_anal=rnd(M, 10), kl_naive_anal=rnd(M, 10), kl_pi_anal=rnd(M, 4), qs1=torch.randn(M, 10, device=dev, generator=g),
              s0=torch.randn(M, 10, device=dev, generator=g))
    S = torch.stack([torch.randint(0, k, (M,), device=dev, generator=g).float() for k in (3, 6, 40, 32, 32)] + [rnd(M) * 2 - 1], 1).contiguous()
    return fe, S, (rnd(M, 1, 64, 64), rnd(M, 1, 64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000,8192')
    ap.add_argument('--games', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_report_bench needs a HIP device')
    import daimc_amd
    from daimc_amd import loss
    from daimc_amd.train import make_batch_random
    from oracle import synth
    dev = 'cuda:0'
    res = {'metric': 'eval_report_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats,
           'device': torch.cuda.get_device_name(0), 'legs': {}}
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device=dev, seed=1, init_weights=False)
    m.load_flat_weights(synth.make_weights(1234, 1.15))
    e = m._ready()

    def leg(name, fn):
        t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
        res['legs'][name] = {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1]}

    for M in (int(v) for v in args.sizes.split(',')):
        fe, S, rw = synthetic(M, dev)
        out = torch.empty(98, device=dev)
        leg(f'eval_stats_M{M}', lambda: loss.eval_stats(fe, S, rw, out=out, engine=e))
        pi0 = torch.eye(4, device=dev)[torch.arange(M, device=dev) % 4].contiguous()
        lp = torch.log(pi0 + 1e-15)
        leg(f'free_energy_M{M}', lambda: loss.free_energy(m, rw[0], rw[1], pi0, lp, omega=2.0))
    G = args.games
    games, test = daimc_amd.Game(8, model=m, seed=3), daimc_amd.Game(G, model=m, seed=4)
    gen = torch.Generator(device=dev).manual_seed(11)
    tr = daimc_amd.Trainer(m, games, generator=gen)
    leg(f'report_G{G}', lambda: tr.report(test))
    leg(f'evaluate_G{G}', lambda: tr.evaluate(*make_batch_random(test, tr.repeats, gen)))
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
