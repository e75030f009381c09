"""The reference's test_demo.py without the window and the keyboard: an agent (or many, --games) in Dynamic-dSprites on the device, a
command line over daimc_amd.agent.AgentRunner.

    python tools/run_agent.py --network runs/a/checkpoints --method ai --duration 5001 [--games 64] [--sprites dsprites.npz]

Every 1000 ticks it prints test_demo.py's line (`<t> ROUND SCORE: <score> t: <seconds>`, one per game); at the end it writes a JSON summary
(round scores, reward crossings, the sum of the rewards received, decisions made).  --network takes the folder model.save_all wrote, or
`random` for freshly initialised weights.  --sprites takes the dSprites archive (an .npz with `imgs`, or an .npy of [N,64,64] uint8);
without it the games run on the synthetic sprite bank, because the archive does not ship.
--trace OUT.npz records the run (daimc_amd.AgentTrace: per tick and game the state, the executed action, G and its terms, the softmax the
action was drawn from, the planned path) and writes the record's arrays; --trace-frames N adds the frames of the first N games (`view`,
uint8, every --frame-every ticks) with the planner's heat mask laid over them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parser():
    ap = argparse.ArgumentParser(description='Run the agent on the device (test_demo.py of the reference).')
    ap.add_argument('-n', '--network', required=True, help='checkpoint folder to load (model.save_all), or "random"')
    ap.add_argument('-m', '--mean', action='store_true', help='expected free energy from the mean instead of sampling')
    ap.add_argument('-d', '--duration', type=int, default=50001, help='ticks (test_demo.py: 50001)')
    ap.add_argument('-method', '--method', default='mcts', choices=['t1', 't12', 'ai', 'mcts', 'habit'])
    ap.add_argument('-steps', '--steps', type=int, default=7, help='how many steps ahead the agent imagines (-1: 10, or 1 for mcts)')
    ap.add_argument('-temp', '--temperature', type=float, default=1.0)
    ap.add_argument('-jumps', '--jumps', type=int, default=5, help='ticks per imagined step')
    ap.add_argument('-C', '--C', type=float, default=1.0, help='MCTS: exploration weight')
    ap.add_argument('-repeats', '--repeats', type=int, default=300, help='MCTS: planning iterations')
    ap.add_argument('-threshold', '--threshold', type=float, default=0.5, help='MCTS: threshold to decide early')
    ap.add_argument('-depth', '--depth', type=int, default=3, help='MCTS: simulation depth')
    ap.add_argument('-no_habit', '--no_habit', action='store_true', help='MCTS: as test_demo.py, the flag is handed to params.use_habit')
    ap.add_argument('--keyed-planner', action='store_true',
                    help='MCTS: one id-keyed planner for all games (a game plays the same trajectory alone and in any batch; no host draw)')
    ap.add_argument('--games', type=int, default=1, help='games run at once (test_demo.py: 1)')
    ap.add_argument('--sprites', default=None, metavar='PATH', help='dSprites images; default: the synthetic sprite bank')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default='agent_run.json', help='the JSON summary')
    ap.add_argument('--trace', default=None, metavar='OUT.npz', help='record the run and write the record here')
    ap.add_argument('--trace-frames', type=int, default=0, metavar='N', help='with --trace: also the frames of the first N games')
    ap.add_argument('--frame-every', type=int, default=1, metavar='K', help='with --trace-frames: one frame every K ticks')
    return ap


def sprites(path):
    if path is None:
        return None
    import numpy as np
    z = np.load(path, allow_pickle=False)
    return z['imgs'] if hasattr(z, 'files') else z


def main(argv=None):
    args = parser().parse_args(argv)
    import daimc_amd
    if args.steps == -1:                                                                   # test_demo.py:70-77
        args.steps = 1 if args.method == 'mcts' else 10
    model = daimc_amd.ActiveInferenceModel(10, 4, 1.0, 1.0, 1.0, device=args.device, seed=args.seed)   # test_demo.py:48
    if args.network != 'random':
        model.load_all(args.network.rstrip('/\\'))
    params = daimc_amd.MCTS_Params()                                                       # test_demo.py:35-40
    params.C, params.repeats, params.threshold, params.simulation_depth = args.C, args.repeats, args.threshold, args.depth
    params.use_habit = args.no_habit
    games = daimc_amd.Game(args.games, model=model, imgs=sprites(args.sprites), seed=args.seed)
    trace = None
    if args.trace:
        trace = daimc_amd.AgentTrace(frames=range(min(args.trace_frames, args.games)) if args.trace_frames > 0 else None, frame_every=args.frame_every)
    runner = daimc_amd.AgentRunner(model, games, args.method, steps=args.steps, jumps=args.jumps, temperature=args.temperature,
                                   calc_mean=args.mean, mcts_params=params, keyed_planner=args.keyed_planner, trace=trace)
    if trace is not None:
        trace.reserve(args.duration)                                                       # (the chunks below would otherwise grow it one by one)
    start = time.time()
    res, printed, done = None, 0, 0
    while done < args.duration:
        # a score is recorded at the START of tick 1000 k: the first chunk runs ticks 0 .. 1000, every later one the next 1000
        n = min(args.duration - done, runner.report_ticks + (1 if done == 0 else 0))
        res = runner.run(n, fetch_trace=done + n >= args.duration)                        # the record is downloaded once, at the end
        done += n
        for row in res['round_scores'][printed:]:
            printed += 1
            for score in row:
                print(printed * runner.report_ticks, 'ROUND SCORE:', float(score), 't:', time.time() - start, flush=True)
            start = time.time()
    if res is None:
        res = runner.run(0)
    summary = {'method': args.method, 'keyed_planner': runner.keyed_planner, 'games': args.games, 'ticks': res['ticks'], 'steps': args.steps, 'jumps': args.jumps,
               'temperature': args.temperature, 'mean': args.mean, 'samples': runner.samples, 'decisions': res['decisions'],
               'failed_ticks': res['failed_ticks'], 'round_scores': res['round_scores'].tolist(), 'crossings': res['crossings'].tolist(),
               'reward_sum': res['reward_sum'].tolist()}
    with open(args.out, 'w') as fh:
        json.dump(summary, fh)
    if args.trace:
        import numpy as np
        np.savez_compressed(args.trace, **res['trace'])
        print('wrote', args.trace, '-', res['ticks'], 'rows')
    print('wrote', args.out, '- ticks', res['ticks'], 'decisions', res['decisions'], 'crossings', int(res['crossings'].sum()),
          'reward sum', float(res['reward_sum'].sum()))


if __name__ == '__main__':
    main()
