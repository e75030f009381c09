"""Throughput of the agent loop (daimc_amd.agent.AgentRunner), recorded in profiles/agent_bench.json -- a measurement, not a gate.

    python tools/agent_bench.py [--ticks 120] [--games 1 64 1024] [--method habit ai mcts] [--mcts-ticks 20]
                                [--parent PATH_TO_A_BUILT_PARENT_CHECKOUT] [--out profiles/agent_bench.json]

Per method (habit, ai at steps 7, samples 10) and number of games: game-ticks per second of an unsynchronised run (wall time over
`--ticks` ticks after a warm-up run of the same length on the same model), and the share of wall time spent in decisions, taken from a
second run whose decisions are bracketed by device synchronisations (so that run is slower and only its ratio is used).  Freshly
initialised weights and the synthetic sprite bank: the figures are about the loop, not about an agent's skill.
--method mcts measures the planner in BOTH of its modes -- the slot planner (the default of AgentRunner) and the id-keyed one
(keyed_planner = True) -- at the reference's demo settings (`MCTS_Params()` untouched, jumps 5) over `--mcts-ticks` ticks: per number of
games one warm-up run per mode, then three unsynchronised runs per mode, ALTERNATING between the modes; per mode the median game-ticks/s and
decisions/s, the spread of the three, and the decision share from one synchronised run.  An existing --out file keeps the rows of the
(method, games) pairs this call does not measure.
With --parent, `bench.py --gpus 1 --steps 20 --warmup 5` is run three times each from this checkout and from the parent's, alternating,
and both sets of result lines are recorded: no existing kernel changes, so the two should sit inside each other's spread.

    python tools/agent_bench.py --trace [--trace-frames 4] [--method ai mcts] [--games 1 64 1024] [--out profiles/agent_trace_bench.json]

measures what recording a run costs (AgentRunner(trace=...)): per method (ai; mcts = the keyed planner) and number of games one warm-up run,
then three unsynchronised runs each of the untraced loop, the loop with the log, and the loop with the log and the frames of the first
--trace-frames games, ALTERNATING between the three; per variant the median game-ticks/s and the spread.  ai runs --ticks ticks, mcts
--mcts-ticks.  The default --out is then profiles/agent_trace_bench.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed_runner():
    """AgentRunner whose decisions are bracketed by device synchronisations; .spent = seconds inside decisions"""
    import torch
    import daimc_amd

    class TimedRunner(daimc_amd.AgentRunner):
        spent = 0.0

        def _decide(self, ids, t):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            super()._decide(ids, t)
            torch.cuda.synchronize()
            self.spent += time.perf_counter() - t0
    return TimedRunner


def one(model, method, E, ticks, timed_decisions, keyed=False, trace=None):
    """-> (wall seconds of `ticks` ticks, seconds inside decisions (0 unless timed), run()'s result)"""
    import torch
    import daimc_amd
    games = daimc_amd.Game(E, model=model, seed=1)
    cls = timed_runner() if timed_decisions else daimc_amd.AgentRunner
    kw = {} if trace is None else {'trace': trace}
    runner = cls(model, games, method, steps=7, jumps=5, samples=10, keyed_planner=keyed, **kw)    # mcts: MCTS_Params() as they come
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = runner.run(ticks)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall, getattr(runner, 'spent', 0.0), res


def mcts_rows(model, E, ticks, runs=3):
    """the slot and the keyed planner at E games, `runs` alternating unsynchronised runs each -> one row per mode"""
    modes = (('slot', False), ('keyed', True))
    for _, keyed in modes:
        one(model, 'mcts', E, ticks, False, keyed)                                        # warm-up: planner buffers, replica context, arena
    walls, results = {m: [] for m, _ in modes}, {}
    for _ in range(runs):
        for mode, keyed in modes:
            wall, _, res = one(model, 'mcts', E, ticks, False, keyed)
            walls[mode].append(wall)
            results[mode] = res
    rows = []
    for mode, keyed in modes:
        wall_s, spent, _ = one(model, 'mcts', E, ticks, True, keyed)
        w, res = sorted(walls[mode]), results[mode]
        med = w[len(w) // 2]
        rows.append({'method': 'mcts', 'planner': mode, 'games': E, 'ticks': ticks, 'jumps': 5, 'params': 'MCTS_Params() defaults',
                     'wall_s': walls[mode], 'wall_median_s': med, 'game_ticks_per_s': E * ticks / med,
                     'game_ticks_per_s_min_max': [E * ticks / w[-1], E * ticks / w[0]], 'decisions': res['decisions'],
                     'decisions_per_s': res['decisions'] / med, 'failed_ticks': res['failed_ticks'],
                     'decision_share_of_wall': spent / wall_s, 'synchronised_wall_s': wall_s})
    return rows


def trace_row(model, method, E, ticks, n_frames, runs=3):
    """the untraced loop, the loop with the log, and with log + frames at E games: `runs` alternating unsynchronised runs each -> one row"""
    import daimc_amd
    keyed = method == 'mcts'
    variants = {'untraced': lambda: None, 'log': lambda: daimc_amd.AgentTrace(),
                'log_frames': lambda: daimc_amd.AgentTrace(frames=range(min(n_frames, E)))}
    one(model, method, E, ticks, False, keyed, variants['log_frames']())                  # warm-up: arena, planner buffers, the record's allocation
    walls = {v: [] for v in variants}
    for _ in range(runs):
        for v, make in variants.items():
            walls[v].append(one(model, method, E, ticks, False, keyed, make())[0])
    row = {'method': method, 'planner': 'keyed' if keyed else None, 'games': E, 'ticks': ticks, 'frames_of_games': min(n_frames, E)}
    for v, w in walls.items():
        w = sorted(w)
        row[v] = {'wall_s': walls[v], 'game_ticks_per_s': E * ticks / w[len(w) // 2], 'game_ticks_per_s_min_max': [E * ticks / w[-1], E * ticks / w[0]]}
    for v in ('log', 'log_frames'):
        row[v]['relative_to_untraced'] = row[v]['game_ticks_per_s'] / row['untraced']['game_ticks_per_s']
    return row


def bench_line(path):
    r = subprocess.run([sys.executable, os.path.join(path, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'], capture_output=True,
                       text=True, cwd=path, timeout=900)
    if r.returncode != 0:
        return {'error': r.stderr[-400:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--ticks', type=int, default=120)
    ap.add_argument('--games', type=int, nargs='+', default=[1, 64, 1024])
    ap.add_argument('--method', nargs='+', default=['habit', 'ai', 'mcts'], choices=['habit', 'ai', 'mcts'])
    ap.add_argument('--mcts-ticks', type=int, default=20)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--trace', action='store_true', help='measure the cost of recording a run instead (AgentRunner(trace=...))')
    ap.add_argument('--trace-frames', type=int, default=4, help='--trace: the first N games are filmed in the log + frames variant')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'agent_trace_bench.json' if args.trace else 'agent_bench.json')
    import daimc_amd
    model = daimc_amd.ActiveInferenceModel(10, 4, 1.0, 1.0, 1.0, device='cuda:0', seed=0)
    if args.trace:
        rows = []
        for method in [m for m in ('ai', 'mcts') if m in args.method]:
            for E in args.games:
                row = trace_row(model, method, E, args.mcts_ticks if method == 'mcts' else args.ticks, args.trace_frames)
                print(json.dumps(row), flush=True)
                rows.append(row)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'what': 'AgentRunner throughput untraced, with the log, and with log + frames; freshly initialised weights, '
                               'synthetic sprite bank', 'trace': rows}, fh, indent=1)
        print('wrote', args.out)
        return
    rows = []
    for E in args.games if 'mcts' in args.method else ():
        for row in mcts_rows(model, E, args.mcts_ticks):
            print(json.dumps(row), flush=True)
            rows.append(row)
    for method in [m for m in ('habit', 'ai') if m in args.method]:
        for E in args.games:
            one(model, method, E, args.ticks, False)                                      # warm-up: arena growth, planner buffers
            wall, _, res = one(model, method, E, args.ticks, False)
            wall_s, spent, _ = one(model, method, E, args.ticks, True)
            row = {'method': method, 'games': E, 'ticks': args.ticks, 'steps': 7, 'jumps': 5, 'samples': 10, 'wall_s': wall,
                   'game_ticks_per_s': E * args.ticks / wall, 'decisions': res['decisions'], 'failed_ticks': res['failed_ticks'],
                   'decision_share_of_wall': spent / wall_s, 'synchronised_wall_s': wall_s}
            print(json.dumps(row), flush=True)
            rows.append(row)
    out = {'what': 'AgentRunner throughput, freshly initialised weights, synthetic sprite bank', 'loop': rows}
    if os.path.isfile(args.out):                                                          # keep what this call did not measure
        with open(args.out) as fh:
            old = json.load(fh)
        out['loop'] += [r for r in old.get('loop', []) if r.get('method') not in args.method or r.get('games') not in args.games]
        if 'bench' in old and not args.parent:
            out['bench'] = old['bench']
    if args.parent:
        out['bench'] = {'this': [], 'parent': []}
        for _ in range(3):
            out['bench']['this'].append(bench_line(ROOT))
            out['bench']['parent'].append(bench_line(os.path.abspath(args.parent)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
