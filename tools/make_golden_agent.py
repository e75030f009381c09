"""Reference-captured fixture of the agent loop: tests/golden/agent_loop.npz.

Runs only where the reference checkout exists.  The reference's own `Game` (src/game_environment.py, through the patches of
oracle.make_golden_env.reference_game: synthetic sprite bank, Philox-addressed latents) is driven through `Game.pi_to_action(repeats=1)`
by a loop that follows the schedule of the reference's test_demo.py:118-204 (stated here in this project's own words) for 24 games at once:

  A : 240 ticks, round_ticks 20, report_ticks 60, steps 2, jumps 3, temperature 1; the method of a tick's decisions is
      ('ai', 't1', 't12')[tick % 3]
  B : 120 ticks at the defaults (round_ticks 100, report_ticks 1000, steps 7, jumps 5), method 'ai'

The decision values are synthetic: per (tick, game) tables of sum_G [4] and sum_terms [3, 4] from a fixed numpy seed, scaled so that
some decisions overflow exp at temperature 1 (inf / inf), some underflow in all four actions (0 / 0) and some give an action p = 0.  The
probabilities are the script's quantities (:82-84, 152-159) formed on float32 arrays and the action is drawn by the real
np.random.choice; the uniform it consumed is recorded by saving the generator state, drawing, and drawing random_sample() from the
saved state.  A decision that np.random.choice refuses is test_demo.py's `except: "Not executing anything"` (choice -1).  Only the
table rows of decisions that happened are stored (every one of them), with the tick and game they belong to.

Before anything is written, tests/agent_ref.py must reproduce every array, and every recorded decision must keep at least 1e-4 between
its uniform and every edge of the cumulative distribution (the float32 restatement and a device then draw what numpy's float64 drew):
the seed is advanced until this holds for every decision of both trajectories.

Recorded tensors only: latents as uint8, floats as their bits.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_agent.py
"""
import contextlib
import io
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import make_golden_env as MGE             # noqa: E402
import agent_ref as AR                                # noqa: E402

E = 24
MARGIN = 1e-4
TRAJ = {'A': dict(ticks=240, round_ticks=20, report_ticks=60, steps=2, jumps=3, temperature=1.0, modes=('ai', 't1', 't12')),
        'B': dict(ticks=120, round_ticks=100, report_ticks=1000, steps=7, jumps=5, temperature=1.0, modes=('ai',))}
BASE_SEED = 20250611


def action_probabilities(method, sum_G, sum_terms, steps, temperature):
    """float32 [4]: the distribution the reference's script hands to np.random.choice for `method` -- the Boltzmann weights of the
    per-step values at `temperature`, normalised by their plain sum (no shift by the maximum, so exp may overflow or underflow).
    numpy float32 arrays against Python floats, as in the script: every operation rounds to float32."""
    n = float(steps)
    if method == 'ai':
        value = -(sum_G / n)                            # minus the expected free energy per step
    elif method == 't1':
        value = sum_terms[0] / n                        # the reward term alone
    else:
        value = sum_terms[0] / n - sum_terms[1] / n     # reward term minus the second term
    with np.errstate(all='ignore'):
        weight = np.exp(value / temperature)
        return weight / weight.sum()


def recorded_choice(p):
    """np.random.choice(4, p=p) with the uniform it consumed -> (choice, u, distance of u from the nearest cdf edge); a distribution
    numpy refuses -> (-1, nan, inf), and the generator state is then untouched"""
    before = np.random.get_state()
    same = lambda s1, s2: all(np.array_equal(a, b) for a, b in zip(s1, s2))
    try:
        choice = int(np.random.choice(4, p=p))
    except ValueError:
        assert same(np.random.get_state(), before), 'a refused draw consumed randomness'
        return -1, np.nan, np.inf
    after = np.random.get_state()
    np.random.set_state(before)
    u = np.random.random_sample()
    assert same(np.random.get_state(), after), 'choice consumed more than one uniform'
    cdf = np.cumsum(p.astype(np.float64))
    cdf /= cdf[-1]
    assert int(cdf.searchsorted(u, side='right')) == choice
    return choice, u, float(np.abs(cdf - u).min())


def tables(rng, steps):
    """one decision's sum_G [4], sum_terms [3, 4] (float32)"""
    x = rng.normal(0.0, 2.0, 4)
    kind = rng.choice(8)
    if kind == 0:
        x = x + 250.0                                   # every exp overflows: inf / inf
    elif kind == 1:
        x[rng.integers(4)] += 300.0                     # one overflows: that entry is inf / inf, the others 0
    elif kind == 2:
        x = x - 300.0                                   # every exp underflows: 0 / 0
    elif kind == 3:
        x[rng.integers(4)] -= 300.0                     # one action with p = 0
    st = np.zeros((3, 4), dtype=np.float32)
    st[0] = (x * steps).astype(np.float32)
    st[1] = (rng.normal(0.0, 0.5, 4) * steps).astype(np.float32)
    st[2] = (rng.normal(0.0, 0.5, 4) * steps).astype(np.float32)
    return (-x * steps).astype(np.float32), st


def run_reference(Game, ctx, cfg, seed):
    """the loop on the reference's Game: a game with nothing queued decides (a failed draw queues nothing, so it neither moves nor ticks),
    a game with something queued takes its action for one tick of Game.pi_to_action, and a finished round drops the rest of its queue"""
    rng = np.random.default_rng(seed)
    np.random.seed(seed & 0x7FFFFFFF)
    steps, jumps = cfg['steps'], cfg['jumps']
    with contextlib.redirect_stdout(io.StringIO()):
        game = Game(E)
    ctx.update(stage=0, k=0, rand_blk=6)
    game.randomize_environment_all()
    game.current_s[:, 6] = 0.0
    queued = np.zeros(E, np.int64)                      # ticks the current action is still to be taken for
    action = np.full(E, 255, np.uint8)
    crossings, reward_sum = np.zeros(E, np.int32), np.zeros(E, np.float32)
    rec = {k: [] for k in ('lat', 'acc', 'r', 'qlen', 'qact', 'cross', 'rsum')}
    dec = {k: [] for k in ('tick', 'game', 'sum_G', 'sum_terms', 'u', 'choice')}
    scores, min_margin = [], np.inf
    for t in range(cfg['ticks']):
        if t > 0 and t % cfg['report_ticks'] == 0:      # the score is reported and starts again
            scores.append(game.current_s[:, 6].numpy().copy())
            game.current_s[:, 6] = 0.0
        if t % cfg['round_ticks'] == 0:                 # a new round: fresh games, the score carried over, nothing queued
            kept = game.current_s[:, 6].clone()
            ctx.update(stage=1 + 2 * t, k=0, rand_blk=6)
            game.randomize_environment_all()
            game.current_s[:, 6] = kept
            queued[:] = 0
        method = cfg['modes'][t % len(cfg['modes'])]
        for g in range(E):
            if queued[g] == 0:
                sum_G, sum_terms = tables(rng, steps)
                p = action_probabilities(method, sum_G, sum_terms, steps, cfg['temperature'])
                assert p.dtype == np.float32
                choice, u, margin = recorded_choice(p)
                min_margin = min(min_margin, margin)
                if choice >= 0:
                    queued[g], action[g] = steps * jumps, choice
                for k, v in zip(('tick', 'game', 'sum_G', 'sum_terms', 'u', 'choice'), (t, g, sum_G, sum_terms, u, choice)):
                    dec[k].append(v)
            if queued[g] > 0:
                ctx.update(stage=2 + 2 * t, game=g, k=0)
                if game.pi_to_action(int(action[g]), g, repeats=1):
                    queued[g] = 0
                    crossings[g] += 1
                    reward_sum[g] = np.float32(reward_sum[g] + game.last_r[g].numpy())
                else:
                    queued[g] -= 1
        lat, acc = MGE._pack(game.current_s.numpy().astype(np.float32))
        rec['lat'].append(lat); rec['acc'].append(MGE._bits(acc)); rec['r'].append(MGE._bits(game.last_r.numpy()))
        rec['qlen'].append(queued.astype(np.uint8))
        rec['qact'].append(np.where(queued > 0, action, 255).astype(np.uint8))
        rec['cross'].append(crossings.astype(np.uint16).copy()); rec['rsum'].append(MGE._bits(reward_sum))
    out = {k: np.stack(v) for k, v in rec.items()}
    out['scores'] = MGE._bits(np.stack(scores)) if scores else np.zeros((0, E), np.uint32)
    out['dec_tick'] = np.array(dec['tick'], np.uint16); out['dec_game'] = np.array(dec['game'], np.uint8)
    out['dec_sum_G'] = MGE._bits(np.stack(dec['sum_G'])); out['dec_sum_terms'] = MGE._bits(np.stack(dec['sum_terms']))
    out['dec_u'] = np.array(dec['u'], np.float64).view(np.uint64); out['dec_choice'] = np.array(dec['choice'], np.int8)
    return out, min_margin


def check_against_agent_ref(name, cfg, out):
    """tests/agent_ref.py fed the recorded tables and uniforms reproduces every recorded array"""
    ref = AR.AgentRef(MGE.SEED, E, steps=cfg['steps'], jumps=cfg['jumps'], temperature=cfg['temperature'], round_ticks=cfg['round_ticks'],
                      report_ticks=cfg['report_ticks'])
    index = {(int(t), int(g)): i for i, (t, g) in enumerate(zip(out['dec_tick'], out['dec_game']))}
    u = out['dec_u'].view(np.float64)
    sG, sT = out['dec_sum_G'].view(np.float32), out['dec_sum_terms'].view(np.float32)
    used = 0
    for t in range(cfg['ticks']):
        mode = cfg['modes'][t % len(cfg['modes'])]

        def decide(t, g):
            i = index[(t, g)]
            return mode, dict(sum_G=sG[i], sum_terms=sT[i]), (0.5 if np.isnan(u[i]) else u[i])
        chosen = ref.tick(t, decide)
        for g, c in chosen.items():
            assert c == out['dec_choice'][index[(t, g)]], (name, t, g, c)
        used += len(chosen)
        lat, acc = MGE._pack(ref.s)
        assert np.array_equal(lat, out['lat'][t]) and np.array_equal(MGE._bits(acc), out['acc'][t]), (name, t, 'state')
        assert np.array_equal(MGE._bits(ref.last_r), out['r'][t]), (name, t, 'last_r')
        assert np.array_equal(ref.queue_len(), out['qlen'][t]) and np.array_equal(ref.queue_action(), out['qact'][t]), (name, t, 'queues')
        assert np.array_equal(ref.crossings, out['cross'][t]) and np.array_equal(MGE._bits(ref.reward_sum), out['rsum'][t]), (name, t, 'score')
    assert used == len(out['dec_tick']), 'a recorded decision was not taken'
    got = MGE._bits(np.stack(ref.scores)) if ref.scores else np.zeros((0, E), np.uint32)
    assert np.array_equal(got, out['scores']), (name, 'round scores')


def main():
    ctx = {'stage': 1000, 'game': 0, 'k': 0, 'rand_blk': 6}
    Game, restore = MGE.reference_game(ctx)
    arrays, meta = {}, {'env_seed': MGE.SEED, 'games': E, 'margin': MARGIN, 'trajectories': {}}
    seed = BASE_SEED
    for name, cfg in TRAJ.items():
        while True:
            out, margin = run_reference(Game, ctx, cfg, seed)
            if margin >= MARGIN:                        # a condition, not a measurement: every decision, no exception
                break
            seed += 1
        check_against_agent_ref(name, cfg, out)
        ch = out['dec_choice']
        assert (ch < 0).sum() >= 10 and all((ch == a).any() for a in range(4)) and out['cross'][-1].sum() >= 10, name
        arrays.update({f'{name}_{k}': v for k, v in out.items()})
        meta['trajectories'][name] = dict(cfg, modes=list(cfg['modes']), seed=seed, decisions=int(len(ch)), failed=int((ch < 0).sum()),
                                          crossings=int(out['cross'][-1].sum()))
        seed += 1
    restore()
    arrays['meta'] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(ROOT, 'tests', 'golden', 'agent_loop.npz')
    MGE.write_npz(path, arrays)
    limit = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'env_sweep.npz'))
    assert os.path.getsize(path) < limit, (os.path.getsize(path), limit)
    print(path, os.path.getsize(path), 'bytes', json.dumps(meta['trajectories']))


if __name__ == '__main__':
    main()
