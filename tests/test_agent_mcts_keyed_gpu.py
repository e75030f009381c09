"""The id-keyed mcts planner of the agent loop (daimc_amd.mcts.BatchedMCTS(keyed=True), AgentRunner(keyed_planner=True)) and the two
kernels at the ends of its decision (csrc/agent_mcts.hip): a game plans and plays the same alone and in any batch, the keyed planner at
identity ids returns the slot planner's paths (on the reference's own captures), a subset decides what the whole batch decides for it,
both kernels against their numpy restatement (tests/agent_mcts_ref.py), AgentRunner against a loop of the public calls, and the refusals.
Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import agent_mcts_ref as MR
from agent_ref import bits
from oracle import philox as PX
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -9
STEPS, JUMPS, ROUND, REPORT, TICKS = 2, 2, 10, 20, 45


def tbits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def model():
    import daimc_amd
    return daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=DEV, seed=23)


def mcts_params(use_habit=False, threshold=None):
    import daimc_amd
    p = daimc_amd.MCTS_Params()
    p.repeats, p.simulation_depth, p.use_habit = 4, 2, use_habit
    if threshold is not None:
        p.threshold = threshold
    return p


def split_threshold(model, frames=None):
    """a threshold between the habit criteria max(Qpi) - mean(Qpi) of `frames` (default: the first frames of the 5-game run below), so that
    the shortcut decides some games and the planner the others (the criterion is a property of the model and the frames, not of the code
    under test)"""
    import daimc_amd
    if frames is None:
        g = daimc_amd.Game(5, model=model, seed=7)
        g.randomize_environment_all(stage=0)
        g.current_s[:, 6] = 0.0
        g.randomize_environment_all(stage=1)
        frames = g.current_frame_nchw()
    q = model.habitual_net(frames).cpu().numpy()
    thr = np.sort([float(MR.threshold_value(r)) for r in q])
    assert thr[-1] > thr[0], thr
    k = len(thr) // 2
    return float((thr[k - 1] + thr[k]) / 2) if thr[k] > thr[k - 1] else float((thr[0] + thr[-1]) / 2)


def decision(model, planner, st, frames, ids, game_offset, stage0, tick, jumps, u=None):
    """one keyed decision with the public calls -> (choice, path [n, max_depth], path_len [n])"""
    p = planner.p
    Qpi = planner.begin_keyed(frames, ids, game_offset, stage0, o_shape=(1, 64, 64))
    choice = st.mcts_root(ids, Qpi, planner.active, planner.decided, use_habit=p.use_habit, threshold=p.threshold, max_depth=planner.max_depth,
                          jumps=jumps, seed=model.seed, stage=tick, game_offset=game_offset, u=u)
    planner.plan_keyed()
    path, plen = st.mcts_enqueue(ids, planner.tree_of(int(ids.numel())), planner.decided, planner.max_depth, jumps, want_path=True)
    return choice, path, plen


# ---- the invariance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_habit', [False, True])
def test_a_game_plans_the_same_alone_and_in_any_batch(model, use_habit):
    """game 2 of a 5-game keyed mcts run equals, tick by tick and bit for bit, the 1-game run with game_offset = 2 and game 2 of a 65-game
    run (more than a wave, a workgroup tail).  The slot planner cannot do this: its noise rows are the slots among the deciding games."""
    import daimc_amd
    params = mcts_params(use_habit, split_threshold(model) if use_habit else None)
    kw = dict(steps=STEPS, jumps=JUMPS, mcts_params=params, round_ticks=ROUND, report_ticks=REPORT, keyed_planner=True)
    runs = []
    for E, off in ((5, 0), (1, 2), (65, 0)):
        games = daimc_amd.Game(E, model=model, seed=7, game_offset=off)
        runs.append((games, daimc_amd.AgentRunner(model, games, 'mcts', **kw), 2 - off, []))
    model._stage = stage_before = 4242
    decided_flags = []
    for t in range(TICKS):
        for games, r, k, rec in runs:
            before = r.decisions
            r.tick()
            st = r.state
            rec.append(torch.cat([tbits(games.current_s[k]), tbits(games.last_r[k:k + 1]), st.queue[k], st.head[k:k + 1], st.len[k:k + 1],
                                  st.crossings[k:k + 1], tbits(st.reward_sum[k:k + 1])]))
            if r.decisions > before and games.games_no == 5:
                decided_flags.append(r.planner.decided[:r.planner.n].clone())
    a, b, c = (torch.stack(rec) for _, _, _, rec in runs)
    assert torch.equal(a, b), 'game 2 of 5 against the game alone'
    assert torch.equal(a, c), 'game 2 of 5 against game 2 of 65'
    g5, r5 = runs[0][0], runs[0][1]
    assert not torch.equal(tbits(g5.current_s[1]), tbits(g5.current_s[2]))                         # (another game goes another way)
    assert runs[1][1].decisions >= TICKS // ROUND and r5.run(0)['failed_ticks'] == 0
    assert model._stage == stage_before                                                            # the model's counter is neither read nor advanced
    flags = torch.cat(decided_flags).cpu().numpy()
    if use_habit:
        assert (flags == 1).any() and (flags == 0).any(), 'the shortcut and the planner must both have decided games'
    else:
        assert (flags == 0).all()


# ---- keyed equals slot at identity -----------------------------------------------------------------------------------------------------
def fixture_model(g):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=DEV, seed=int(g['nseed']), init_weights=False)
    m.load_flat_weights(synth.make_weights(int(g['wseed']), float(g['gain'])))
    m.eps_source, m.u_source = PX.normals, PX.uniforms              # both planners consume the numpy Philox mirror's noise
    return m


def fixture_params(g, name):
    import daimc_amd
    p = daimc_amd.MCTS_Params()
    if name == 'mcts_defaults':
        assert (int(g['repeats']), int(g['simulation_depth']), float(g['threshold'])) == (p.repeats, p.simulation_depth, p.threshold)
        return p                                                      # the reference's MCTS_Params() untouched
    p.repeats, p.simulation_depth, p.use_means, p.threshold = int(g['repeats']), int(g['simulation_depth']), False, float(g['threshold'])
    p.samples = int(g['samples'])
    p.using_prior_for_exploration, p.use_habit = bool(g['using_prior_for_exploration']), bool(g['use_habit'])
    return p


def paths_of(path, plen):
    path, plen = path.cpu().numpy(), plen.cpu().numpy()
    return [path[i, :plen[i]].tolist() for i in range(len(plen))]


@pytest.mark.parametrize('name', ['mcts_defaults', 'mcts_deep_s10_thr'])
def test_keyed_planner_at_identity_returns_the_slot_planners_paths(golden, name):
    """identity ids, game_offset = episode_offset, model._stage = stage0: efe_agent_mcts_enqueue's path_out is active_inference_mcts_batch's
    final path for every episode, on the reference's own captures (mcts_defaults: MCTS_Params() untouched, five early stops between
    iterations 21 and 217 and one episode that never stops; mcts_deep_s10_thr: 10-sample expansions, depth-5 simulations) -- and the
    fixtures' final paths, which are the reference planner's."""
    import daimc_amd
    from daimc_amd.mcts import BatchedMCTS
    g = golden(name)
    m = fixture_model(g)
    p = fixture_params(g, name)
    stage0 = int(g['stage'])
    frames = torch.from_numpy(g['frames'])
    n = frames.shape[0]
    if name == 'mcts_defaults':
        gids, E, off = [int(i) for i in g['episode_ids']], int(g['n_frames']), 3      # fixture episode k is global episode gids[k] of n_frames
    else:
        gids, E, off = list(range(n)), n, 0
    want = [[int(a) for a in g['final_path'][k] if a >= 0] for k in range(n)]
    # the slot planner on these frames at a global episode offset, and the keyed planner at identity
    m._stage = stage0
    out, _ = daimc_amd.active_inference_mcts_batch(m, frames, p, o_shape=(1, 64, 64), episode_offset=off)
    assert m._stage == stage0 + BatchedMCTS.stages_per_decision(p)
    planner = BatchedMCTS(m, E, p, keyed=True)
    st = daimc_amd.AgentState(m._ready(), E, planner.max_depth)
    m._stage = 77
    _, path, plen = decision(m, planner, st, frames.to(DEV), torch.arange(n, dtype=torch.int32, device=DEV), off, stage0, 0, 1)
    got = paths_of(path, plen)
    assert got == [[int(a) for a in o[0]] for o in out]
    assert m._stage == 77
    if off == 0:
        assert got == want
    else:
        # the keyed planner with the fixture's global episode ids (6 of 40, ascending as efe_agent_need lists them) plans the fixture's episodes
        order = np.argsort(gids)
        ids = torch.tensor([gids[k] for k in order], dtype=torch.int32, device=DEV)
        st.clear()
        _, path, plen = decision(m, planner, st, frames[order].to(DEV), ids, 0, stage0, 0, 1)
        assert paths_of(path, plen) == [want[k] for k in order]
        assert st.len[ids.long()].cpu().tolist() == [len(want[k]) for k in order]


# ---- subsets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_habit', [False, True])
def test_a_subset_decides_what_the_whole_batch_decides_for_it(model, use_habit):
    import daimc_amd
    from daimc_amd.mcts import BatchedMCTS
    E, off, tick = 6, 11, 9
    games = daimc_amd.Game(E, model=model, seed=7, game_offset=off)
    games.randomize_environment_all(stage=3)
    frames = games.current_frame_nchw()
    params = mcts_params(use_habit, split_threshold(model, frames) if use_habit else None)
    planner = BatchedMCTS(model, E, params, keyed=True)
    stage0 = tick * BatchedMCTS.stages_per_decision(params)
    full, sub = (daimc_amd.AgentState(model._ready(), E, planner.max_depth * JUMPS) for _ in range(2))
    for st in (full, sub):
        st.queue.fill_(SENTINEL)
    all_ids = torch.arange(E, dtype=torch.int32, device=DEV)
    ch_full, _, _ = decision(model, planner, full, frames, all_ids, off, stage0, tick, JUMPS)
    ids = torch.tensor([4, 1, 5], dtype=torch.int32, device=DEV)
    ch_sub, _, _ = decision(model, planner, sub, frames[ids.long()], ids, off, stage0, tick, JUMPS)
    k = ids.long()
    assert torch.equal(ch_sub, ch_full[k])
    assert torch.equal(sub.queue[k], full.queue[k]) and torch.equal(sub.len[k], full.len[k]) and (sub.head == 0).all()
    rest = torch.tensor([0, 2, 3], device=DEV)
    assert (sub.queue[rest] == SENTINEL).all() and (sub.len[rest] == 0).all()
    assert int(full.len.max()) > 0
    if use_habit:
        assert (ch_full >= 0).any() and (ch_full == -2).any()


# ---- efe_agent_mcts_enqueue against numpy ----------------------------------------------------------------------------------------------
MAX_DEPTH, EJ = 12, 3


def synthetic_trees(n, A, rng):
    cap = 1 + A * MAX_DEPTH
    long_plain = ([0, 2] * MAX_DEPTH)[:MAX_DEPTH - 1] if A == 4 else ([0, 1] * MAX_DEPTH)[:MAX_DEPTH - 1]
    pair = [0, 1] if A == 4 else [1, 2]
    kinds = [lambda: MR.random_tree(rng, cap, A, int(rng.integers(0, MAX_DEPTH - 1))),
             lambda: MR.random_tree(rng, cap, A, int(rng.integers(0, MAX_DEPTH - 1)), ties=True),
             lambda: (rng.integers(0, 3, size=(cap, A)).astype(np.float32), np.full((cap, A), -1, np.int32)),      # a root-only tree
             lambda: MR.chain_tree(long_plain, cap, A),                                                           # max_depth nodes, nothing cancels
             lambda: MR.chain_tree((pair * MAX_DEPTH)[:MAX_DEPTH - 2], cap, A),                                   # cancelling pairs only
             lambda: MR.chain_tree((pair[::-1] * MAX_DEPTH)[:MAX_DEPTH - 1], cap, A),                             # pairs, then a last action that is dropped
             lambda: MR.chain_tree([int(rng.integers(0, A))], cap, A),                                            # one action: trims to nothing
             lambda: MR.chain_tree(rng.integers(0, A, size=MAX_DEPTH - 1).tolist(), cap, A, rng)]
    trees = [kinds[i % len(kinds)]() for i in range(n)]
    return np.stack([t[0] for t in trees]), np.stack([t[1] for t in trees])


@pytest.mark.parametrize('A', [4, 3])
@pytest.mark.parametrize('n', [1, 63, 65, 129])
def test_enqueue_against_numpy(n, A):
    import daimc_amd
    from daimc_amd import _lib
    rng = np.random.default_rng(100 * A + n)
    E = n + 4
    games = daimc_amd.Game(E, device=DEV, seed=1)
    st = daimc_amd.AgentState(games._engine, E, MAX_DEPTH * EJ)                                  # a cap of exactly max_depth * jumps
    N, child = synthetic_trees(n, A, rng)
    ids = np.sort(rng.choice(E, size=n, replace=False)).astype(np.int32)
    decided = (np.arange(n) % 5 == 3).astype(np.uint8)
    st.queue.fill_(SENTINEL); st.head.fill_(3); st.len.fill_(2)
    q0, h0, l0 = (t.cpu().numpy() for t in (st.queue, st.head, st.len))
    Nd, cd = torch.from_numpy(N).to(DEV), torch.from_numpy(child).to(DEV)
    dummy = torch.zeros(1, device=DEV)
    tree = _lib.EfeMctsTree(dummy.data_ptr(), Nd.data_ptr(), dummy.data_ptr(), cd.data_ptr(), dummy.data_ptr(), n, N.shape[1], A, 10)
    path, plen = st.mcts_enqueue(torch.from_numpy(ids).to(DEV), tree, torch.from_numpy(decided).to(DEV), MAX_DEPTH, EJ, want_path=True)
    wq, wh, wl, paths = MR.enqueue(N, child, ids, decided, q0, h0, l0, EJ)
    assert np.array_equal(st.queue.cpu().numpy(), wq) and np.array_equal(st.head.cpu().numpy(), wh) and np.array_equal(st.len.cpu().numpy(), wl)
    want_path = np.full((n, MAX_DEPTH), -1, np.int32)
    for i, p in enumerate(paths):
        if p is not None:
            want_path[i, :len(p)] = p
    assert np.array_equal(path.cpu().numpy(), want_path)
    assert plen.cpu().tolist() == [-1 if p is None else len(p) for p in paths]
    lens = [len(p) for p in paths if p is not None]
    if n >= 63:
        assert 0 in lens and max(lens) == MAX_DEPTH - 2                                          # nothing left, and the longest a tree can give


# ---- efe_agent_mcts_root against numpy -------------------------------------------------------------------------------------------------
def root_cases(A, rng):
    """Qpi rows and uniforms: random distributions, peaked and flat ones, p = 0 entries, every edge from both sides, u = 1, non-distributions"""
    rows, us = [], []
    base = [rng.dirichlet(np.ones(A)).astype(np.float32) for _ in range(12)]
    base += [np.eye(A, dtype=np.float32)[k] for k in range(A)]
    base += [np.full(A, 1.0 / A, np.float32), np.array([0.9, 0.0, 0.1, 0.0][:A], np.float32), np.array([0.0, 0.0, 1.0, 0.0][:A], np.float32),
             np.array([0.0, 0.7, 0.3, 0.0][:A], np.float32)]
    for q in base:
        cdf = np.cumsum(q, dtype=np.float32) / np.cumsum(q, dtype=np.float32)[-1]
        for u in [0.0, 0.5, 1.0, float(rng.random())] + [float(e) + d for e in cdf[:-1] for d in (-1e-4, 1e-4) if 0.0 <= float(e) + d < 1.0]:
            rows.append(q); us.append(u)
    for bad in (np.nan, np.inf, -0.25):
        for k in (0, A - 1):
            q = np.full(A, 1.0 / A, np.float32)
            q[k] = bad
            rows.append(q); us.append(0.5)
    return np.stack(rows), np.array(us, dtype=np.float32)


@pytest.mark.parametrize('A', [4, 3])
def test_root_against_numpy(A):
    import daimc_amd
    rng = np.random.default_rng(3 + A)
    Qpi, u = root_cases(A, rng)
    n = Qpi.shape[0]
    assert n > 128                                                                               # more than one workgroup
    E = n + 3
    games = daimc_amd.Game(E, device=DEV, seed=1)
    ids = np.sort(rng.choice(E, size=n, replace=False)).astype(np.int32)
    ids_t = torch.from_numpy(ids).to(DEV)
    crit = float(MR.threshold_value(Qpi[0]))
    seen = set()
    for use_habit in (True, False):
        for threshold in (0.05, 0.5, crit - 1e-4, crit + 1e-4, 0.74, 0.75):                      # 0.75 = 1 - 1/4: out of reach for A = 4
            st = daimc_amd.AgentState(games._engine, E, 2 * EJ)
            st.queue.fill_(SENTINEL); st.head.fill_(3); st.len.fill_(2)
            active = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
            decided = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
            choice, u_out = st.mcts_root(ids_t, Qpi, active, decided, use_habit=use_habit, threshold=threshold, max_depth=2, jumps=EJ, u=u,
                                         want_u=True)
            wc, wd, wa, wq = MR.root(Qpi, u, use_habit, threshold, EJ)
            assert np.array_equal(choice.cpu().numpy(), wc), (use_habit, threshold)
            assert np.array_equal(decided.cpu().numpy(), wd) and np.array_equal(active.cpu().numpy(), wa)
            assert np.array_equal(bits(u_out.cpu().numpy()), bits(u))
            queue, head, length = np.full((E, 2 * EJ), SENTINEL, np.int32), np.full(E, 3, np.int32), np.full(E, 2, np.int32)
            for i, q in enumerate(wq):
                if q is not None:
                    queue[ids[i], :len(q)] = q
                    head[ids[i]], length[ids[i]] = 0, len(q)
            assert np.array_equal(st.queue.cpu().numpy(), queue) and np.array_equal(st.head.cpu().numpy(), head)
            assert np.array_equal(st.len.cpu().numpy(), length)
            seen |= set(wc.tolist())
            if use_habit and threshold == 0.05:
                assert (wc[-6:] == -1).all() and (wc[:-6] >= -2).all()
    assert seen == set(range(-2, A))
    # thresholds on both sides of the first row's criterion decide it differently
    assert MR.root(Qpi[:1], u[:1], True, crit - 1e-4, 1)[1][0] == 1 and MR.root(Qpi[:1], u[:1], True, crit + 1e-4, 1)[1][0] == 0


def test_root_uniform_is_the_philox_word():
    """not injected: word 0 of the counter (tag 0x70, global game, stream 0, the tick) -- oracle.philox's, and efe_agent_choose's key"""
    import daimc_amd
    import agent_ref as AR
    E = 70
    games = daimc_amd.Game(E, device=DEV, seed=1)
    st = daimc_amd.AgentState(games._engine, E, 4)
    ids = torch.tensor([0, 3, 64, 69, 17], dtype=torch.int32, device=DEV)
    Qpi = torch.tensor([[0.7, 0.1, 0.1, 0.1]] * 5, device=DEV)
    active, decided = torch.zeros(5, dtype=torch.uint8, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV)
    for seed in (0, 0x1234_5678_9ABC_DEF0):
        for off in (0, 1000, 0xFFFFFFF0):
            for stage in (0, 7, 0xFFFFFFFF):
                kw = dict(use_habit=True, threshold=0.3, max_depth=2, jumps=2, seed=seed, stage=stage, game_offset=off)
                ch, u = st.mcts_root(ids, Qpi, active, decided, want_u=True, **kw)
                want = PX.uniforms(seed, E, 0, 0, stage, row_offset=off, tag=AR.TAG_AGENT)[ids.cpu().numpy()]
                assert np.array_equal(bits(u.cpu().numpy()), bits(want)), (seed, off, stage)
                assert ch.cpu().tolist() == [MR.draw(Qpi[0].cpu().numpy(), w) for w in want]
                ch2, u2 = st.choose(ids, 'probs', probs=Qpi, repeat=2, seed=seed, stage=stage, game_offset=off, want_u=True)
                assert torch.equal(tbits(u), tbits(u2)) and torch.equal(ch, ch2)


# ---- AgentRunner against a loop of the public calls ------------------------------------------------------------------------------------
def public_loop(model, games, params, ticks):
    """AgentRunner's tick in keyed mcts mode, written out with the public calls"""
    import daimc_amd
    from daimc_amd.mcts import BatchedMCTS
    E, go = games.games_no, games.game_offset
    planner = BatchedMCTS(model, E, params, keyed=True)
    P = 2 + params.repeats * (1 + params.simulation_repeats)
    st = daimc_amd.AgentState(model._ready(), E, max(STEPS * JUMPS, (params.repeats + 2) * JUMPS))
    scores, decisions, failed = [], 0, 0
    games.randomize_environment_all(stage=0)
    games.current_s[:, 6] = 0.0
    for t in range(ticks):
        if t % REPORT == 0 and t > 0:
            scores.append(games.current_s[:, 6].clone())
            games.current_s[:, 6] = 0.0
        if t % ROUND == 0:
            score = games.current_s[:, 6].clone()
            games.randomize_environment_all(stage=1 + 2 * t)
            games.current_s[:, 6] = score
            st.clear()
        ids, count = st.need()
        n = int(count.item())
        if n:
            decisions += n
            ids = ids[:n]
            frames = games.current_frame_nchw()[ids.long()]
            Qpi = planner.begin_keyed(frames, ids, go, t * P, o_shape=(1, 64, 64))
            choice = st.mcts_root(ids, Qpi, planner.active, planner.decided, use_habit=params.use_habit, threshold=params.threshold,
                                  max_depth=params.repeats + 2, jumps=JUMPS, seed=model.seed, stage=t, game_offset=go)
            planner.plan_keyed()
            st.mcts_enqueue(ids, planner.tree_of(n), planner.decided, params.repeats + 2, JUMPS)
            failed += int((choice == -1).any())
        st.act(games, stage=2 + 2 * t)
    return st, scores, decisions, failed


@pytest.mark.parametrize('E', [3, 65])
def test_runner_equals_a_loop_of_the_public_calls(model, E):
    import daimc_amd
    params = mcts_params(True, split_threshold(model))
    ga = daimc_amd.Game(E, model=model, seed=7, game_offset=2)
    gb = daimc_amd.Game(E, model=model, seed=7, game_offset=2)
    runner = daimc_amd.AgentRunner(model, ga, 'mcts', steps=STEPS, jumps=JUMPS, mcts_params=params, round_ticks=ROUND, report_ticks=REPORT,
                                   keyed_planner=True)
    res = runner.run(TICKS)
    st, scores, decisions, failed = public_loop(model, gb, params, TICKS)
    assert torch.equal(tbits(ga.current_s), tbits(gb.current_s)) and torch.equal(tbits(ga.last_r), tbits(gb.last_r))
    for nm in ('queue', 'head', 'len', 'crossings'):
        assert torch.equal(getattr(runner.state, nm), getattr(st, nm)), nm
    assert torch.equal(tbits(runner.state.reward_sum), tbits(st.reward_sum))
    assert np.array_equal(bits(res['round_scores']), bits(torch.stack(scores).cpu().numpy())) and res['round_scores'].shape == (2, E)
    assert res['decisions'] == decisions >= E * (TICKS // ROUND + 1) and res['ticks'] == TICKS and res['failed_ticks'] == failed == 0
    assert (ga.current_s[:, :6] != 0).any() and torch.isfinite(ga.last_r).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import daimc_amd
    from daimc_amd import _lib
    games = daimc_amd.Game(4, device=DEV, seed=1)
    st = daimc_amd.AgentState(games._engine, 4, 6)
    e = games._engine
    st.queue.fill_(SENTINEL); st.len.fill_(2)
    before = (st.len.clone(), st.queue.clone(), st.head.clone())
    n, A, depth, jumps = 4, 4, 3, 2
    ids = torch.arange(4, dtype=torch.int32, device=DEV)
    Qpi = torch.tensor([[0.97, 0.01, 0.01, 0.01]] * 4, device=DEV)                               # the shortcut would decide and write every queue
    active, decided = torch.full((4,), 7, dtype=torch.uint8, device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV)
    choice = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    N, child = MR.chain_tree([0, 2], 1 + 4 * depth, 4)
    Nd = torch.from_numpy(np.stack([N] * 4)).to(DEV)
    cd = torch.from_numpy(np.stack([child] * 4)).to(DEV)
    nz = _lib.EfeNoise(1, 0, 0, 0, 0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def tree_of(E=4, cap=1 + 4 * depth, A=4, N=Nd, child=cd):
        return _lib.EfeMctsTree(p(Nd), p(N), p(Nd), p(child), p(Nd), E, cap, A, 10)

    def root(ag=None, ids=ids, n=n, Qpi=Qpi, A=A, depth=depth, jumps=jumps, nz=nz, u=None, active=active, decided=decided, choice=choice):
        return e.lib.efe_agent_mcts_root(e.ctx, C.byref(ag) if ag is not None else None, p(ids), n, p(Qpi), A, 1, C.c_float(0.5), depth, jumps,
                                         C.byref(nz) if nz is not None else None, p(u), p(active), p(decided), p(choice), None, e.stream())

    def enq(ag=None, tree=None, ids=ids, n=n, decided=decided, depth=depth, jumps=jumps):
        return e.lib.efe_agent_mcts_enqueue(e.ctx, C.byref(ag) if ag is not None else None, C.byref(tree) if tree is not None else None, p(ids),
                                            n, p(decided), depth, jumps, None, None, e.stream())

    def msg(rc):
        assert rc == 1
        return e.lib.efe_last_error(e.ctx).decode()
    s = st._struct
    for name, call in (('efe_agent_mcts_root', root), ('efe_agent_mcts_enqueue', lambda **kw: enq(tree=kw.pop('tree', tree_of()), **kw))):
        for E_bad in (0, -3):
            assert f'{name}: E < 1' in msg(call(ag=_lib.EfeAgent(s.queue, s.head, s.len, s.crossings, s.reward_sum, E_bad, s.cap)))
        assert f'{name}: n < 0 or n > E' in msg(call(ag=s, n=-1))
        assert f'{name}: n < 0 or n > E' in msg(call(ag=s, n=5))
        assert f'{name}: jumps < 1' in msg(call(ag=s, jumps=0))
        assert f'{name}: the queue capacity 6 is smaller than max_depth * jumps = 8' in msg(call(ag=s, depth=4))
        assert f'{name}: the queue capacity 6 is smaller than max_depth * jumps = 9' in msg(call(ag=s, jumps=3))
        assert f'{name}: agent is NULL' in msg(call(ag=None))
        assert f'{name}: a NULL array' in msg(call(ag=_lib.EfeAgent(s.queue, None, s.len, s.crossings, s.reward_sum, s.E, s.cap)))
        assert f'{name}: ids' in msg(call(ag=s, ids=None))
    for A_bad in (2, 5, 8):
        assert f'efe_agent_mcts_root: A = {A_bad}' in msg(root(ag=s, A=A_bad))
        assert f'efe_agent_mcts_enqueue: A = {A_bad}' in msg(enq(ag=s, tree=tree_of(A=A_bad)))
    for kw in (dict(Qpi=None), dict(active=None), dict(decided=None), dict(choice=None)):
        assert 'efe_agent_mcts_root: ids, Qpi, active, decided or choice is NULL' in msg(root(ag=s, **kw))
    assert 'efe_agent_mcts_root: neither efe_noise nor injected uniforms' in msg(root(ag=s, nz=None))
    assert 'efe_agent_mcts_enqueue: tree is NULL' in msg(enq(ag=s, tree=None))
    assert 'efe_agent_mcts_enqueue: N or child' in msg(enq(ag=s, tree=tree_of(N=None)))
    assert 'efe_agent_mcts_enqueue: N or child' in msg(enq(ag=s, tree=tree_of(child=None)))
    assert 'efe_agent_mcts_enqueue: the tree has cap < 1 or fewer than n slots' in msg(enq(ag=s, tree=tree_of(E=3)))
    assert 'efe_agent_mcts_enqueue: ids or decided is NULL' in msg(enq(ag=s, tree=tree_of(), decided=None))
    torch.cuda.synchronize()
    assert torch.equal(st.len, before[0]) and torch.equal(st.queue, before[1]) and torch.equal(st.head, before[2])     # a refused call launches nothing
    assert (active == 7).all() and (choice == 7).all()
    # the same arguments, accepted: n = 0 launches nothing and is no error; n = 4 writes every queue
    assert root(ag=s, n=0) == 0 and enq(ag=s, tree=tree_of(), n=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(st.queue, before[1]) and (active == 7).all()
    assert enq(ag=s, tree=tree_of()) == 0 and st.len.cpu().tolist() == [2] * 4 and (st.queue[:, :2] == 0).all()         # [0, 2] trims to [0]
    assert root(ag=s) == 0 and (decided == 1).all() and (active == 0).all() and (choice >= 0).all()
    with pytest.raises(ValueError):
        st.mcts_root(ids, Qpi[:3], active, decided, use_habit=True, threshold=0.5, max_depth=3, jumps=2)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_run_agent_keyed_planner_flag(tmp_path):
    """tools/run_agent.py --keyed-planner in-process: the summary names the planner, and a second run of the same command plays the same
    games (with the slot planner it would not: its habit draw comes from the host's global generator, its stages from the model's counter)"""
    import importlib.util
    import json
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('run_agent', os.path.join(ROOT, 'tools', 'run_agent.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = []
    for k in range(2):
        out = tmp_path / f'run{k}.json'
        mod.main(['--network', 'random', '--method', 'mcts', '--keyed-planner', '--no_habit', '--threshold', '0.05', '--repeats', '4',
                  '--depth', '2', '--jumps', '2', '--duration', '35', '--games', '3', '--out', str(out)])
        got.append(json.loads(out.read_text()))
    assert got[0]['keyed_planner'] is True and got[0]['method'] == 'mcts' and got[0]['ticks'] == 35 and got[0]['decisions'] >= 3
    assert got[0] == got[1]
