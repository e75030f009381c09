"""The agent loop on the device (csrc/agent.hip, daimc_amd.agent): the kernels against the trajectory captured from the reference's Game
driven by test_demo.py's loop (tests/golden/agent_loop.npz), efe_agent_act against efe_env_step, the order of efe_agent_need, the action
uniform against oracle.philox, AgentRunner against a loop of the public calls, and the batch-invariance of a game's trajectory.
Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from agent_ref import Trajectory, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7777


def tbits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def model():
    import daimc_amd
    return daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=DEV, seed=23)


def new_state(games, cap):
    import daimc_amd
    return daimc_amd.AgentState(games._engine, games.games_no, cap)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'B'])
def test_kernels_reproduce_the_reference_trajectory(name):
    import daimc_amd
    tr = Trajectory(load_golden('agent_loop'), name)
    c, a, E = tr.cfg, tr.a, tr.E
    games = daimc_amd.Game(E, device=DEV, seed=tr.env_seed)
    st = new_state(games, c['steps'] * c['jumps'])
    games.randomize_environment_all(stage=0)
    games.current_s[:, 6] = 0.0
    by_tick = {}
    for i, t in enumerate(a['dec_tick']):
        by_tick.setdefault(int(t), []).append(i)
    rec = {k: [] for k in ('s', 'r', 'len', 'head', 'queue', 'cross', 'rsum')}
    scores, choices = [], []
    for t in range(c['ticks']):
        if t % c['report_ticks'] == 0 and t > 0:
            scores.append(games.current_s[:, 6].clone())
            games.current_s[:, 6] = 0.0
        if t % c['round_ticks'] == 0:
            score = games.current_s[:, 6].clone()
            games.randomize_environment_all(stage=1 + 2 * t)
            games.current_s[:, 6] = score
            st.clear()
        ids, count = st.need()
        n = int(count.item())
        idx = by_tick.get(t, [])
        assert n == len(idx), t
        if n:
            assert ids[:n].cpu().tolist() == [int(a['dec_game'][i]) for i in idx], t           # ascending, as the reference loops over the games
            sum_terms = np.transpose(tr.sum_terms[idx], (1, 0, 2)).reshape(3, 4 * n)
            u = np.array([tr.uniform(i) for i in idx], dtype=np.float32)
            choices.append((idx, st.choose(ids[:n], tr.mode(t), sum_G=tr.sum_G[idx].reshape(-1), sum_terms=sum_terms, steps=c['steps'],
                                           temperature=c['temperature'], repeat=c['steps'] * c['jumps'], u=u)))
        st.act(games, stage=2 + 2 * t)
        for k, v in zip(('s', 'r', 'len', 'head', 'queue', 'cross', 'rsum'),
                        (games.current_s, games.last_r, st.len, st.head, st.queue, st.crossings, st.reward_sum)):
            rec[k].append(v.clone())
    got = {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}
    for idx, ch in choices:
        assert np.array_equal(ch.cpu().numpy(), a['dec_choice'][idx].astype(np.int32)), idx[0]
    assert np.array_equal(got['s'][:, :, :6], a['lat'].astype(np.float32)) and np.array_equal(bits(got['s'][:, :, 6]), a['acc'])
    assert np.array_equal(bits(got['r']), a['r'])
    assert np.array_equal(got['len'], a['qlen'].astype(np.int32))
    assert (got['head'][got['len'] == 0] == 0).all()
    T, cap = c['ticks'], got['queue'].shape[2]
    slot = np.arange(cap)[None, None, :]
    inside = (slot >= got['head'][:, :, None]) & (slot < (got['head'] + got['len'])[:, :, None])
    want = np.broadcast_to(a['qact'].astype(np.int32)[:, :, None], (T, E, cap))
    assert np.array_equal(got['queue'][inside], want[inside])                                    # every queued action is the recorded one
    assert np.array_equal(got['cross'], a['cross'].astype(np.int32)) and np.array_equal(bits(got['rsum']), a['rsum'])
    sc = bits(torch.stack(scores).cpu().numpy()) if scores else np.zeros((0, E), np.uint32)
    assert np.array_equal(sc, a['scores'])


# ---- act against step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 127, 129])
def test_act_with_full_queues_equals_env_step(E):
    import daimc_amd
    pad = 3
    ga = daimc_amd.Game(E, device=DEV, seed=41, game_offset=5)
    gb = daimc_amd.Game(E, device=DEV, seed=41, game_offset=5)
    for g in (ga, gb):
        g.randomize_environment_all(stage=2)
    ga.current_s[:, 5].clamp_(max=20.0)                           # ... and no other game is
    ga.current_s[::3, 5] = 31.0                                   # every third game is about to cross when it moves up
    ga.current_s[1::4, 4] = 31.0
    gb.current_s.copy_(ga.current_s)
    # the agent's game tensors and its own arrays live inside sentinel-filled buffers
    big_s = torch.full((E + 2 * pad, 7), float(SENTINEL), device=DEV); big_r = torch.full((E + 2 * pad,), float(SENTINEL), device=DEV)
    big_s[pad:pad + E] = ga.current_s; big_r[pad:pad + E] = ga.last_r
    ga.current_s, ga.last_r = big_s[pad:pad + E], big_r[pad:pad + E]
    st = new_state(ga, 4)
    bufs = {}
    for nm in ('queue', 'head', 'len', 'crossings', 'reward_sum'):
        t = getattr(st, nm)
        big = torch.full((E + 2 * pad,) + tuple(t.shape[1:]), SENTINEL, dtype=t.dtype, device=DEV)
        big[pad:pad + E] = t
        bufs[nm] = big
        setattr(st, nm, big[pad:pad + E])
    st._bind()
    actions = (torch.arange(E, device=DEV) % 4).to(torch.int32)
    actions[::3] = 0
    ids = torch.arange(E, dtype=torch.int32, device=DEV)
    st.enqueue(ids, actions[:, None], torch.ones(E, dtype=torch.int32), jumps=2)
    assert (st.len == 2).all() and torch.equal(st.queue[:, :2], actions[:, None].expand(E, 2))
    ch_a = st.act(ga, stage=9, want_changed=True)
    ch_b = gb.pi_to_action_all(actions, repeats=1, stage=9)
    assert torch.equal(ch_a, ch_b) and int(ch_a.sum()) == len(range(0, E, 3))
    assert torch.equal(tbits(ga.current_s), tbits(gb.current_s)) and torch.equal(tbits(ga.last_r), tbits(gb.last_r))
    assert torch.equal(st.len, torch.where(ch_a, 0, 1).to(torch.int32)) and torch.equal(st.head, torch.where(ch_a, 0, 1).to(torch.int32))
    assert torch.equal(st.crossings, ch_a.to(torch.int32))
    assert torch.equal(tbits(st.reward_sum), tbits(torch.where(ch_a, ga.last_r, torch.zeros_like(ga.last_r))))
    # a second tick: the games that crossed have an empty queue and are left untouched, the others equal another step
    before_s, before_r = ga.current_s.clone(), ga.last_r.clone()
    st.act(ga, stage=10)
    gb.pi_to_action_all(actions, repeats=1, stage=10)
    assert torch.equal(tbits(ga.current_s[ch_a]), tbits(before_s[ch_a])) and torch.equal(tbits(ga.last_r[ch_a]), tbits(before_r[ch_a]))
    assert torch.equal(tbits(ga.current_s[~ch_a]), tbits(gb.current_s[~ch_a])) and torch.equal(tbits(ga.last_r[~ch_a]), tbits(gb.last_r[~ch_a]))
    assert (st.len == 0).all() and (st.head == 0).all()
    for big in (big_s, big_r, *bufs.values()):
        assert (big[:pad] == SENTINEL).all() and (big[pad + E:] == SENTINEL).all()


# ---- the order of need -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 65, 257, 2049])
def test_need_is_ascending_and_exact(E):
    """2049 games: three chunks of the kernel's one 1024-thread workgroup"""
    import daimc_amd
    games = daimc_amd.Game(E, device=DEV, seed=1)
    st = new_state(games, 2)
    pad = 2
    big = torch.full((E + 2 * pad,), SENTINEL, dtype=torch.int32, device=DEV)
    st.ids = big[pad:pad + E]
    ar = torch.arange(E, device=DEV)
    for pattern, lens in (('every', torch.zeros(E)), ('none', torch.ones(E)), ('alternate', ar % 2), ('thirds', (ar % 3 != 1).float()),
                          ('last', (ar != E - 1).float())):
        big.fill_(SENTINEL)
        st.len.copy_(lens.to(torch.int32))
        ids, count = st.need()
        want = torch.nonzero(st.len == 0).flatten().to(torch.int32)
        n = int(count.item())
        assert n == want.numel(), pattern
        assert torch.equal(ids[:n], want), pattern
        assert (big[:pad] == SENTINEL).all() and (big[pad + n:] == SENTINEL).all(), pattern        # nothing beyond the count is written


# ---- the action uniform ----------------------------------------------------------------------------------------------------------------
def test_action_uniform_is_the_philox_word():
    import daimc_amd
    from oracle import philox as PX
    import agent_ref as AR
    E = 70
    games = daimc_amd.Game(E, device=DEV, seed=1)
    st = new_state(games, 3)
    ids = torch.tensor([0, 3, 64, 69, 17], dtype=torch.int32, device=DEV)
    probs = torch.full((5, 4), 0.25, device=DEV)
    for seed in (0, 0x1234_5678_9ABC_DEF0):
        for off in (0, 1000, 0xFFFFFFF0):
            for stage in (0, 7, 0xFFFFFFFF):
                ch, u = st.choose(ids, 'probs', probs=probs, repeat=3, seed=seed, stage=stage, game_offset=off, want_u=True)
                full = PX.uniforms(seed, E, 0, 0, stage, row_offset=off, tag=AR.TAG_AGENT)
                want = full[ids.cpu().numpy()]
                assert np.array_equal(bits(u.cpu().numpy()), bits(want)), (seed, off, stage)
                assert np.array_equal(ch.cpu().numpy(), np.minimum((want / np.float32(0.25)).astype(np.int64), 3)), (seed, off, stage)


def test_draw_at_u_one_and_failed_draws():
    import daimc_amd
    games = daimc_amd.Game(6, device=DEV, seed=1)
    st = new_state(games, 4)
    ids = torch.arange(6, dtype=torch.int32, device=DEV)
    probs = torch.tensor([[0.25, 0.25, 0.25, 0.25], [0.3, 0.7, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.5, -0.1, 0.6, 0.0],
                          [0.5, float('nan'), 0.5, 0.0]], device=DEV)
    st.len.fill_(2)
    ch = st.choose(ids, 'probs', probs=probs, repeat=4, u=torch.ones(6))
    assert ch.cpu().tolist() == [3, 1, 0, -1, -1, -1]                     # u == 1.0: the last action with p > 0
    assert st.len.cpu().tolist() == [4, 4, 4, 0, 0, 0] and (st.head == 0).all()
    assert torch.equal(st.queue[:3], torch.tensor([3, 1, 0], dtype=torch.int32, device=DEV)[:, None].expand(3, 4))
    # softmax without max-subtraction: x = 100 overflows exp at temperature 1 (inf / inf), not at temperature 10
    sum_G = torch.tensor([-100.0, 0.0, 0.0, 0.0] * 6, device=DEV)
    assert (st.choose(ids, 'ai', sum_G=sum_G, steps=1, temperature=1.0, repeat=4, u=torch.full((6,), 0.5)) == -1).all()
    assert (st.choose(ids, 'ai', sum_G=sum_G, steps=1, temperature=10.0, repeat=4, u=torch.full((6,), 0.5)) == 0).all()
    assert (st.choose(ids, 'ai', sum_G=sum_G, steps=10, temperature=1.0, repeat=4, u=torch.full((6,), 0.5)) == 0).all()
    assert (st.choose(ids, 'ai', sum_G=-sum_G, steps=1, temperature=1.0, repeat=4, u=torch.full((6,), 0.5)) == 2).all()   # p = (0, 1/3, 1/3, 1/3)
    assert (st.choose(ids, 'ai', sum_G=torch.full((24,), 500.0), steps=1, temperature=1.0, repeat=4, u=torch.full((6,), 0.5)) == -1).all()   # 0 / 0


def test_refusals():
    import daimc_amd
    from daimc_amd import _lib
    games = daimc_amd.Game(4, device=DEV, seed=1)
    st = new_state(games, 6)
    e = games._engine
    ids = torch.arange(4, dtype=torch.int32, device=DEV)
    probs = torch.full((4, 4), 0.25, device=DEV)
    before = (st.len.clone(), st.queue.clone())

    def refused(match, fn):
        with pytest.raises(RuntimeError, match=match):
            fn()
    refused('efe_agent_choose.*capacity', lambda: st.choose(ids, 'probs', probs=probs, repeat=7))
    refused('efe_agent_choose.*steps', lambda: st.choose(ids, 'ai', sum_G=torch.zeros(16), steps=0, repeat=2))
    for T in (0.0, -1.0, float('inf'), float('nan')):
        refused('efe_agent_choose.*temperature', lambda: st.choose(ids, 'ai', sum_G=torch.zeros(16), temperature=T, repeat=2))
    refused('efe_agent_choose.*sum_G', lambda: st.choose(ids, 'ai', probs=probs, repeat=2))
    refused('efe_agent_choose.*sum_terms', lambda: st.choose(ids, 't12', sum_G=torch.zeros(16), repeat=2))
    refused('efe_agent_choose.*probs', lambda: st.choose(ids, 'probs', sum_G=torch.zeros(16), repeat=2))
    refused('efe_agent_enqueue.*capacity', lambda: st.enqueue(ids, torch.zeros(4, 4), torch.ones(4), jumps=2))
    refused('efe_agent_enqueue.*jumps', lambda: st.enqueue(ids, torch.zeros(4, 2), torch.ones(4), jumps=0))
    with pytest.raises(ValueError):
        st.choose(ids, 'softmax', probs=probs)
    st.enqueue(ids[:0], torch.zeros(0, 2), torch.zeros(0), jumps=2)                             # no game: nothing happens, nothing is refused
    assert st.choose(ids[:0], 'probs', probs=probs[:0], repeat=2).numel() == 0
    nz = _lib.EfeNoise(1, 0, 0, 0, 0)
    ch = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda ag, n=4, mode=3: (e.ctx, C.byref(ag), p(ids), n, mode, None, None, p(probs), 1, C.c_float(1.0), 2, C.byref(nz), None, p(ch), None, e.stream())

    def msg(rc):
        assert rc == 1
        return e.lib.efe_last_error(e.ctx).decode()
    assert 'efe_agent_choose: unknown mode' in msg(e.lib.efe_agent_choose(*args(st._struct, mode=4)))
    assert 'efe_agent_choose: n < 0' in msg(e.lib.efe_agent_choose(*args(st._struct, n=-1)))
    s = st._struct
    for E_bad in (0, -3):
        bad = _lib.EfeAgent(s.queue, s.head, s.len, s.crossings, s.reward_sum, E_bad, s.cap)
        assert 'efe_agent_choose: E < 1' in msg(e.lib.efe_agent_choose(*args(bad)))
        assert 'efe_agent_need: E < 1' in msg(e.lib.efe_agent_need(e.ctx, C.byref(bad), p(st.ids), p(st.count), e.stream()))
        assert 'efe_agent_act: E < 1' in msg(e.lib.efe_agent_act(e.ctx, C.byref(bad), p(games.current_s), p(games.last_r), C.byref(nz), None, e.stream()))
        assert 'efe_agent_enqueue: E < 1' in msg(e.lib.efe_agent_enqueue(e.ctx, C.byref(bad), p(ids), 4, p(ids), p(ids), 1, 1, e.stream()))
    null = _lib.EfeAgent(s.queue, None, s.len, s.crossings, s.reward_sum, s.E, s.cap)
    assert 'efe_agent_act: a NULL array' in msg(e.lib.efe_agent_act(e.ctx, C.byref(null), p(games.current_s), p(games.last_r), C.byref(nz), None, e.stream()))
    assert 'efe_agent_need: ids or count is NULL' in msg(e.lib.efe_agent_need(e.ctx, C.byref(s), None, p(st.count), e.stream()))
    assert 'efe_agent_act: state' in msg(e.lib.efe_agent_act(e.ctx, C.byref(s), None, p(games.last_r), C.byref(nz), None, e.stream()))
    assert 'efe_agent_need: agent is NULL' in msg(e.lib.efe_agent_need(e.ctx, None, p(st.ids), p(st.count), e.stream()))
    torch.cuda.synchronize()
    assert torch.equal(st.len, before[0]) and torch.equal(st.queue, before[1])                  # a refused call launches nothing


# ---- composition -----------------------------------------------------------------------------------------------------------------------
STEPS, JUMPS, SAMPLES, ROUND, REPORT, TICKS = 2, 2, 2, 10, 20, 45


def mcts_params():
    import daimc_amd
    p = daimc_amd.MCTS_Params()
    p.repeats, p.simulation_depth, p.use_habit = 4, 2, False
    return p


def public_loop(model, games, method, ticks):
    """AgentRunner's tick written out with the public calls"""
    import daimc_amd
    from daimc_amd.model import Rows
    E, go = games.games_no, games.game_offset
    params = mcts_params()
    st = daimc_amd.AgentState(model._ready(), E, max(STEPS * JUMPS, (params.repeats + 2) * JUMPS) if method == 'mcts' else STEPS * JUMPS)
    scores, decisions = [], 0
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
            key = dict(seed=model.seed, stage=t, game_offset=go)
            if method == 'habit':
                mean, _ = model.model_down.encoder(frames, stage=t * STEPS, row_offset=go, rows=Rows(ids=ids, rows_per_entry=1, n_total=E))
                st.choose(ids, 'probs', probs=model.model_top.encode_s(mean)[1], repeat=STEPS, **key)
            elif method == 'mcts':
                out, _ = daimc_amd.active_inference_mcts_batch(model, frames, params, o_shape=(1, 64, 64), episode_offset=go)
                paths = [list(o[0]) for o in out]
                L = max(1, max(map(len, paths)))
                st.enqueue(ids, [p + [0] * (L - len(p)) for p in paths], [len(p) for p in paths], JUMPS)
            else:
                sG, sT, _ = model.calculate_G_4_repeated(frames.repeat_interleave(4, dim=0), steps=STEPS, samples=SAMPLES, stage=t * STEPS,
                                                         row_offset=4 * go, rows=Rows(ids=ids, rows_per_entry=4, n_total=E))
                st.choose(ids, method, sum_G=sG, sum_terms=torch.stack(sT), steps=STEPS, temperature=1.0, repeat=STEPS * JUMPS, **key)
        st.act(games, stage=2 + 2 * t)
    return st, scores, decisions


@pytest.mark.parametrize('E', [3, 65])
@pytest.mark.parametrize('method', ['habit', 'ai', 't1', 't12', 'mcts'])
def test_runner_equals_a_loop_of_the_public_calls(model, method, E):
    import daimc_amd
    ga = daimc_amd.Game(E, model=model, seed=7, game_offset=2)
    gb = daimc_amd.Game(E, model=model, seed=7, game_offset=2)
    model._stage = 0                                                 # (mcts: the planner takes its stages from the model's counter)
    model.__dict__.pop('_planners', None)
    runner = daimc_amd.AgentRunner(model, ga, method, steps=STEPS, jumps=JUMPS, samples=SAMPLES, mcts_params=mcts_params(), round_ticks=ROUND,
                                   report_ticks=REPORT)
    res = runner.run(TICKS)
    model._stage = 0
    model.__dict__.pop('_planners', None)
    st, scores, decisions = public_loop(model, gb, method, TICKS)
    assert torch.equal(tbits(ga.current_s), tbits(gb.current_s)) and torch.equal(tbits(ga.last_r), tbits(gb.last_r))
    for nm in ('queue', 'head', 'len', 'crossings'):
        assert torch.equal(getattr(runner.state, nm), getattr(st, nm)), nm
    assert torch.equal(tbits(runner.state.reward_sum), tbits(st.reward_sum))
    assert np.array_equal(bits(res['round_scores']), bits(torch.stack(scores).cpu().numpy())) and res['round_scores'].shape == (2, E)
    assert res['decisions'] == decisions >= E * (TICKS // ROUND + 1) and res['ticks'] == TICKS
    assert np.array_equal(res['crossings'], st.crossings.cpu().numpy()) and np.array_equal(bits(res['state']), bits(gb.current_s.cpu().numpy()))
    assert (ga.current_s[:, :6] != 0).any() and torch.isfinite(ga.last_r).all()


# ---- invariance ------------------------------------------------------------------------------------------------------------------------
def test_a_game_runs_the_same_alone_and_in_a_batch(model):
    """game 2 of a 5-game `ai` run equals the 1-game run with game_offset = 2, tick by tick"""
    import daimc_amd
    kw = dict(steps=STEPS, jumps=JUMPS, samples=SAMPLES, round_ticks=ROUND, report_ticks=REPORT)
    g5 = daimc_amd.Game(5, model=model, seed=7)
    g1 = daimc_amd.Game(1, model=model, seed=7, game_offset=2)
    r5, r1 = daimc_amd.AgentRunner(model, g5, 'ai', **kw), daimc_amd.AgentRunner(model, g1, 'ai', **kw)
    rec5, rec1 = [], []
    for t in range(TICKS):
        r5.tick(); r1.tick()
        rec5.append(torch.cat([g5.current_s[2], g5.last_r[2:3], r5.state.len[2:3].float(), r5.state.crossings[2:3].float(), r5.state.reward_sum[2:3]]))
        rec1.append(torch.cat([g1.current_s[0], g1.last_r[0:1], r1.state.len[0:1].float(), r1.state.crossings[0:1].float(), r1.state.reward_sum[0:1]]))
    a, b = torch.stack(rec5), torch.stack(rec1)
    assert torch.equal(tbits(a), tbits(b))
    assert not torch.equal(tbits(g5.current_s[1]), tbits(g5.current_s[2]))                         # (another game goes another way)
    assert r1.decisions >= TICKS // (STEPS * JUMPS)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_run_agent_prints_round_scores_and_writes_the_summary(tmp_path, capsys):
    """tools/run_agent.py in-process: 2101 ticks of the habit method for two games -> ROUND SCORE lines at ticks 1000 and 2000"""
    import importlib.util
    import json
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('run_agent', os.path.join(ROOT, 'tools', 'run_agent.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / 'run.json'
    mod.main(['--network', 'random', '--method', 'habit', '--duration', '2101', '--games', '2', '--steps', '3', '--out', str(out)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if 'ROUND SCORE:' in ln]
    assert [ln.split()[0] for ln in lines] == ['1000', '1000', '2000', '2000']
    summary = json.loads(out.read_text())
    assert summary['ticks'] == 2101 and summary['method'] == 'habit' and summary['samples'] == 10
    assert np.asarray(summary['round_scores']).shape == (2, 2) and len(summary['crossings']) == 2
    assert summary['decisions'] >= 2 * 2101 // 3 and summary['failed_ticks'] == 0
    assert [float(ln.split()[3]) for ln in lines] == [s for row in summary['round_scores'] for s in row]
