"""Timing of the mutual-information table -> one JSON line on stdout, and the same record in profiles/eval_mi_bench.json with --write (or at
--out).

Legs (milliseconds per call: device events around a window of `steps` calls after `warmup` calls, the median of `repeats` windows):
  eval_mutual_info_M{M}          : loss.eval_mutual_info (efe_eval_mi, csrc/eval_mi.hip) on synthetic latents and factor columns of M rows,
                                   n_neighbors = 3, device noise, no download
  eval_mutual_info_injected_M{M} : the same with injected noise [60, 2, M]
  eval_stats_M{M}                : loss.eval_stats over all four groups on the same rows in the same run (tools/eval_report_bench.py's leg)
  sklearn_host_M{M}              : wall time of the 60 mutual_info_regression calls on downloaded float64 columns, the download included
                                   (one pass; absent where scikit-learn is not importable)

Usage:  python tools/eval_mi_bench.py [--sizes 1000,8192] [--steps 20] [--warmup 3] [--repeats 3] [--write] [--out path.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.eval_report_bench import synthetic, window_ms  # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'eval_mi_bench.json')


def sklearn_ms(s0, S):
    """the host route: download both arrays, 60 calls -> milliseconds, or None without scikit-learn"""
    try:
        from sklearn.feature_selection import mutual_info_regression
    except ImportError:
        return None
    import numpy as np
    t = time.perf_counter()
    a, b = s0.cpu().numpy().astype(np.float64), S.cpu().numpy().astype(np.float64)
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            mutual_info_regression(a[:, i].reshape(-1, 1), b[:, j], random_state=np.random.RandomState(0))
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000,8192')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--write', action='store_true')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_mi_bench needs a HIP device')
    from daimc_amd import loss
    dev = 'cuda:0'
    res = {'metric': 'eval_mi_ms_per_call', 'steps': args.steps, 'warmup': args.warmup, 'repeats': args.repeats, 'n_neighbors': 3,
           'device': torch.cuda.get_device_name(0), 'legs': {}}

    def leg(name, fn):
        t = sorted(window_ms(fn, args.steps, args.warmup) for _ in range(args.repeats))
        res['legs'][name] = {'ms_per_call_median': t[len(t) // 2], 'ms_per_call_min': t[0], 'ms_per_call_max': t[-1]}

    for M in (int(v) for v in args.sizes.split(',')):
        fe, S, rw = synthetic(M, dev)
        out, row = torch.empty(60, device=dev), torch.empty(98, device=dev)
        noise = torch.randn(60, 2, M, dtype=torch.float64, device=dev)
        leg(f'eval_mutual_info_M{M}', lambda: loss.eval_mutual_info(fe['s0'], S, seed=5, stage=1, out=out))
        leg(f'eval_mutual_info_injected_M{M}', lambda: loss.eval_mutual_info(fe['s0'], S, noise=noise, out=out))
        leg(f'eval_stats_M{M}', lambda: loss.eval_stats(fe, S, rw, out=row))
        ms = sklearn_ms(fe['s0'], S)
        if ms is not None:
            res['legs'][f'sklearn_host_M{M}'] = {'ms_wall_one_pass': ms}
    line = json.dumps(res)
    if args.write:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
