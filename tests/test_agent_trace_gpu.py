"""The record of an agent run (daimc_amd.AgentTrace, csrc/agent_trace.hip): the mask and view kernels against their numpy restatements
(tests/agent_trace_ref.py), the mask through the real slot planner, every field of the record against an untraced twin runner driven tick
by tick, the recorded draw against the edge rule, G and its terms against a separate rollout, growth of the record, non-finite weights,
the refusals and the command line.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import agent_trace_ref as TR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -7.0
STEPS, JUMPS, SAMPLES, ROUND, REPORT, TICKS = 2, 2, 2, 10, 20, 25
STAGE0 = 4242                                                        # where the slot planner's stage counter stands when a run starts
FILL = {'choice': -1, 'u': np.nan, 'G': np.nan, 'terms': np.nan, 'probs': np.nan, 'path': 0, 'path_len': 0}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


@pytest.fixture(scope='module')
def model():
    import daimc_amd
    return daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device=DEV, seed=23)


def mcts_params():
    import daimc_amd
    p = daimc_amd.MCTS_Params()
    p.repeats, p.simulation_depth, p.threshold, p.use_habit = 6, 2, 0.5, False
    return p


# ---- 1. the mask kernel on synthetic histories ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_iter', [1, 7, 257])
@pytest.mark.parametrize('jumps', [1, 5])
@pytest.mark.parametrize('slots', [1, 3])
def test_mask_kernel_equals_the_restatement(model, slots, jumps, n_iter):
    from daimc_amd.agent import plan_mask
    E, D = 6, 9
    rng = np.random.default_rng(100 * slots + 10 * jumps + n_iter)
    rows = n_iter + 2                                                # two rows beyond n_iter: live, long, and not to be counted
    H_act = rng.integers(0, 4, size=(rows, slots, D)).astype(np.int32)
    H_len = rng.integers(0, D + 1, size=(rows, slots)).astype(np.int32)
    H_active = (rng.random((rows, slots)) < 0.7).astype(np.uint8)
    H_len[0, 0] = 0                                                  # a live row without a path
    H_active[n_iter:] = 1
    H_len[n_iter:] = D
    if n_iter > 1:
        H_active[1, 0], H_len[1, 0] = 0, D                           # a long path in a row that is not live
        H_active[2 % n_iter, 0], H_len[2 % n_iter, 0] = 1, D
    if slots == 3:
        H_active[:n_iter, 1] = 0                                     # slot 1 has no live row: zeros
    state = np.zeros((E, 7), dtype=np.float32)
    state[:, 4], state[:, 5] = rng.integers(0, 32, E), rng.integers(0, 32, E)
    ids = [0, 2, 5] if slots == 3 else [3]
    for g, (tx, ty) in zip(ids, [(0, 0), (31, 31), (0, 31)][:slots] if slots == 3 else [((0, 0), (31, 31), (0, 31))[(jumps + n_iter) % 3]]):
        state[g, 5], state[g, 4] = tx, ty
    mask = torch.full((E, 32, 32), SENTINEL, device=DEV)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    plan_mask(model._ready(), i32(ids), dev(state), dev(H_act), dev(H_len), dev(H_active), n_iter, jumps, mask)
    got = mask.cpu().numpy()
    for i, g in enumerate(ids):
        want = TR.plan_mask(TR.history_paths(H_act, H_len, H_active, n_iter, i), state[g], jumps)
        assert same(got[g], want), (g, np.abs(got[g] - want).max())
    if slots == 3:
        assert not got[2].any()
    assert got[ids[0]].max() == 1.0 or not got[ids[0]].any()
    others = [g for g in range(E) if g not in ids]
    assert (got[others] == SENTINEL).all()                           # the masks of games that do not decide are not touched


def test_mask_of_a_start_outside_the_grid_is_clamped(model):
    from daimc_amd.agent import plan_mask
    state = torch.tensor([[0, 0, 0, 0, -4.0, 77.5, 0], [0, 0, 0, 0, float('nan'), 31.9, 0]], device=DEV)
    H_act = i32([[[1, 2, 0], [3, 2, 1]]])
    mask = torch.full((2, 32, 32), SENTINEL, device=DEV)
    plan_mask(model._ready(), i32([0, 1]), state, H_act, i32([[3, 3]]), torch.ones(1, 2, dtype=torch.uint8, device=DEV), 1, 2, mask)
    for g in range(2):
        assert same(mask[g].cpu().numpy(), TR.plan_mask([H_act[0, g].cpu().tolist()], state[g].cpu().numpy(), 2))


# ---- 2. the mask through the real slot planner ---------------------------------------------------------------------------------------------
def test_mask_of_the_slot_planner_equals_the_restatement_on_all_paths(model):
    import daimc_amd
    E, go = 3, 2
    games = daimc_amd.Game(E, model=model, seed=7, game_offset=go)
    twin = daimc_amd.Game(E, model=model, seed=7, game_offset=go)
    model._stage = STAGE0
    model.__dict__.pop('_planners', None)
    runner = daimc_amd.AgentRunner(model, games, 'mcts', steps=STEPS, jumps=JUMPS, mcts_params=mcts_params(), round_ticks=ROUND,
                                   report_ticks=REPORT, trace=True)
    assert not runner.plan_mask.any() and tuple(runner.plan_mask.shape) == (E, 32, 32)       # zeros before the first decision
    res = runner.run(1)                                              # tick 0: every game decides
    tr = res['trace']
    assert tr['decided'][0].all()
    # the same decision with the public call, from the stage the runner's decision started from and without its cached planner
    twin.randomize_environment_all(stage=0)
    twin.current_s[:, 6] = 0.0
    twin.randomize_environment_all(stage=1)
    twin.current_s[:, 6] = 0.0
    assert same(tr['state'][0], twin.current_s.cpu().numpy())
    model._stage = STAGE0
    model.__dict__.pop('_planners', None)
    out, _ = daimc_amd.active_inference_mcts_batch(model, twin.current_frame_nchw(), mcts_params(), o_shape=(1, 64, 64), episode_offset=go)
    got, state = runner.plan_mask.cpu().numpy(), twin.current_s.cpu().numpy()
    explored = 0
    for e in range(E):
        path, _, _, all_paths, _ = out[e]
        explored += len(all_paths)
        assert same(got[e], TR.plan_mask(all_paths, state[e], JUMPS)), e
        assert tr['path_len'][0, e] == len(path) and tr['path'][0, e, :len(path)].tolist() == list(path)
        assert tr['choice'][0, e] == -1 and np.isnan(tr['u'][0, e])
    assert explored > 0 and got.any()
    model.__dict__.pop('_planners', None)


# ---- 3. the view kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('with_mask', [False, True])
def test_view_kernel_equals_the_restatement(model, n, with_mask):
    from daimc_amd.agent import agent_view
    E = 5
    rng = np.random.default_rng(7 + n)
    frames = rng.random((n, 1, 64, 64)).astype(np.float32)
    frames[:, 0, 20:24, 20:24] = 1.0                                 # a sprite under the mask
    frames[:, 0, 60, 31] = 0.25                                      # under the marker
    frames[0, 0, 2, 2] = np.nan
    masks = rng.random((E, 32, 32)).astype(np.float32)
    masks[:, 4, 4] = 1.0                                             # pixel (20, 20): 1.0 + 1.0
    masks[:, 8:, :] *= (rng.random((E, 24, 32)) < 0.5)
    ids = [1, 3, 4][:n] if n == 3 else [2]
    view = agent_view(model._ready(), torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV) if with_mask else None,
                      i32(ids) if with_mask else None)
    got = view.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (n, 64, 64)
    for i, g in enumerate(ids):
        assert same(got[i], TR.view(frames[i, 0], masks[g] if with_mask else None)), i
        assert (got[i, 59:63, 31] == 255).all() and got[i, 20, 20] == 255
    assert got[0, 2, 2] == 0
    if with_mask:
        assert ((frames[:, 0, 16:48, 16:48] + masks[ids]) > 1.0).any() and (got[:, 16:48, 16:48] == 255).any()


# ---- 4. the record against a live twin -----------------------------------------------------------------------------------------------------
CASES = {'habit': ('habit', False), 'ai': ('ai', False), 't1': ('t1', False), 't12': ('t12', False), 'mcts_slot': ('mcts', False),
         'mcts_keyed': ('mcts', True)}
_PAIRS = {}


def new_runner(model, case, E, trace):
    import daimc_amd
    method, keyed = CASES[case]
    games = daimc_amd.Game(E, model=model, seed=7, game_offset=2)
    model._stage = STAGE0                                            # no run starts from another's stage counter or planner cache
    model.__dict__.pop('_planners', None)
    return daimc_amd.AgentRunner(model, games, method, steps=STEPS, jumps=JUMPS, samples=SAMPLES, mcts_params=mcts_params(), round_ticks=ROUND,
                                 report_ticks=REPORT, keyed_planner=keyed, trace=trace)


def drive(runner, ticks):
    """`ticks` bare ticks of an untraced runner -> per tick the deciding games, and the environment and the queues just before act"""
    st, g = runner.state, runner.games
    need0, act0, cur, rec = st.need, st.act, {}, []

    def need():
        ids, count = need0()
        cur['ids'] = ids[:int(count.item())].cpu().numpy().copy()
        return ids, count

    def act(games, stage):
        cur.update(state=g.current_s.cpu().numpy(), last_r=g.last_r.cpu().numpy(), len=st.len.cpu().numpy(), head=st.head.cpu().numpy(),
                   queue=st.queue.cpu().numpy())
        cur['changed'] = act0(games, stage, want_changed=True).cpu().numpy()
    st.need, st.act = need, act
    for _ in range(ticks):
        runner.tick()
        rec.append(dict(cur))
    st.need, st.act = need0, act0
    return rec


def pair(model, case, E):
    """the traced run and its untraced twin, once per (case, E) for all the tests below"""
    if (case, E) not in _PAIRS:
        traced = new_runner(model, case, E, True)
        res = traced.run(TICKS)
        twin = new_runner(model, case, E, None)
        rec = drive(twin, TICKS)
        model.__dict__.pop('_planners', None)
        _PAIRS[case, E] = (traced, res, twin, rec)
    return _PAIRS[case, E]


@pytest.mark.parametrize('case,E', [('habit', 3), ('habit', 65), ('ai', 3), ('ai', 65), ('t12', 3), ('t12', 65), ('mcts_slot', 3), ('mcts_keyed', 3)])
def test_record_equals_the_live_twin(model, case, E):
    traced, res, twin, rec = pair(model, case, E)
    tr = res['trace']
    method, keyed = CASES[case]
    assert all(tr[k].shape[:2] == (TICKS, E) for k in traced.trace.FIELDS) and tr['path'].shape == (TICKS, E, 16)
    decisions = 0
    for t, r in enumerate(rec):
        assert same(tr['state'][t], r['state']) and same(tr['last_r'][t], r['last_r']), t
        head = r['queue'][np.arange(E), r['head']]
        assert same(tr['action'][t], np.where(r['len'] > 0, head, -1).astype(np.int32)), t
        assert same(tr['queue_len'][t], r['len']) and same(tr['changed'][t], r['changed'].astype(np.int32)), t
        dec = np.zeros(E, dtype=np.uint8)
        dec[r['ids']] = 1
        assert same(tr['decided'][t], dec), t
        decisions += int(dec.sum())
        idle = dec == 0
        for k, fill in FILL.items():
            assert same(tr[k][t][idle], np.full_like(tr[k][t][idle], fill)), (t, k)
        d = ~idle
        if method == 'mcts':
            plen, path = tr['path_len'][t][d], tr['path'][t][d]
            assert (plen >= 0).all() and (plen * JUMPS == r['len'][d]).all()
            assert (path[plen > 0, 0] == tr['action'][t][d][plen > 0]).all()
            assert np.isnan(tr['G'][t][d]).all() and np.isnan(tr['terms'][t][d]).all()
            if keyed:
                assert (tr['choice'][t][d] == -2).all() and np.isfinite(tr['probs'][t][d]).all() and np.isfinite(tr['u'][t][d]).all()
            else:
                assert (tr['choice'][t][d] == -1).all() and np.isnan(tr['probs'][t][d]).all() and np.isnan(tr['u'][t][d]).all()
        else:
            assert same(tr['choice'][t][d], tr['action'][t][d]) and (tr['choice'][t][d] >= 0).all()
            assert ((tr['u'][t][d] >= 0) & (tr['u'][t][d] <= 1)).all() and np.isfinite(tr['probs'][t][d]).all()
            assert (r['len'][d] == (STEPS if method == 'habit' else STEPS * JUMPS)).all()
            assert np.isnan(tr['G'][t][d]).all() if method == 'habit' else np.isfinite(tr['G'][t][d]).all() and np.isfinite(tr['terms'][t][d]).all()
    assert decisions == res['decisions'] >= E * (TICKS // ROUND + 1)
    assert tr['changed'].sum() == res['crossings'].sum()


# ---- 5. the draw, G and the terms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,E', [('habit', 3), ('habit', 65), ('ai', 3), ('ai', 65)])
def test_recorded_choice_is_the_edge_rule_on_the_recorded_probs(model, case, E):
    tr = pair(model, case, E)[1]['trace']
    rows = np.argwhere(tr['decided'] == 1)
    assert len(rows) >= E
    for t, e in rows:
        assert tr['choice'][t, e] == TR.choice(tr['probs'][t, e], tr['u'][t, e]), (t, e)
    assert len(set(tr['choice'][tr['decided'] == 1].tolist())) > 1


def test_recorded_G_and_terms_are_the_divisions_of_a_separate_rollout(model):
    import daimc_amd
    from daimc_amd.model import Rows
    E = 3
    traced, res, _, _ = pair(model, 'ai', E)
    tr, go = res['trace'], traced.games.game_offset
    g = daimc_amd.Game(E, model=model, seed=7, game_offset=go)
    fs, seen = np.float32(STEPS), 0
    for t in range(TICKS):
        ids = np.flatnonzero(tr['decided'][t])
        if not len(ids):
            continue
        g.current_s.copy_(torch.from_numpy(tr['state'][t]))
        g.last_r.copy_(torch.from_numpy(tr['last_r'][t]))
        ids_d = i32(ids.tolist())
        frames = g.current_frame_nchw()[ids_d.long()]
        sG, sT, _ = model.calculate_G_4_repeated(frames.repeat_interleave(4, dim=0), steps=STEPS, samples=SAMPLES, stage=t * STEPS,
                                                 row_offset=4 * go, rows=Rows(ids=ids_d, rows_per_entry=4, n_total=E))
        sG, sT = sG.cpu().numpy().reshape(-1, 4), [x.cpu().numpy().reshape(-1, 4) for x in sT]
        assert same(tr['G'][t][ids], sG / fs), t
        assert same(tr['terms'][t][ids], np.stack([-sT[0] / fs, sT[1] / fs, sT[2] / fs], axis=1)), t
        ex = np.exp(-(sG / fs) / np.float32(1.0))
        np.testing.assert_allclose(tr['probs'][t][ids], ex / ex.sum(axis=1, keepdims=True), rtol=1e-5)
        seen += len(ids)
    assert seen == res['decisions']


# ---- 6. tracing changes nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_traced_and_untraced_runs_end_bit_identical(model, case):
    traced, res, twin, _ = pair(model, case, 3)
    plain = twin.run(0)
    assert 'trace' not in plain and 'trace' in res and sorted(set(res) - {'trace'}) == sorted(plain)
    assert twin.trace is None and twin.plan_mask is None
    a, b = traced.state, twin.state
    assert same(traced.games.current_s.cpu().numpy(), twin.games.current_s.cpu().numpy())
    assert same(traced.games.last_r.cpu().numpy(), twin.games.last_r.cpu().numpy())
    for nm in ('queue', 'head', 'len', 'crossings', 'reward_sum'):
        assert same(getattr(a, nm).cpu().numpy(), getattr(b, nm).cpu().numpy()), nm
    assert same(res['round_scores'], plain['round_scores']) and res['round_scores'].shape == (1, 3)
    assert res['decisions'] == plain['decisions'] and res['failed_ticks'] == plain['failed_ticks'] == 0


# ---- 7. growth -----------------------------------------------------------------------------------------------------------------------------
def test_record_grows_over_runs_and_bare_ticks(model):
    whole = new_runner(model, 'habit', 3, True).run(20)['trace']
    r = new_runner(model, 'habit', 3, True)
    assert r.run(10)['trace']['state'].shape[0] == 10
    assert r.run(7)['trace']['state'].shape[0] == 17
    for _ in range(3):
        r.tick()
    parts = r.run(0)['trace']
    assert r.trace.T >= 20
    for k in r.trace.FIELDS:
        assert parts[k].shape[0] == 20 and same(parts[k], whole[k]), k


def test_frames_are_the_view_of_the_state_after_act(model):
    import daimc_amd
    from daimc_amd.agent import agent_view
    k, film = 2, [2, 0]
    r = new_runner(model, 'mcts_keyed', 3, daimc_amd.AgentTrace(frames=film, frame_every=k))
    want = []
    for t in range(7):
        r.tick()
        if (t + 1) % k == 0:
            frames = r.games.current_frame_nchw()[torch.tensor(film, device=DEV)].contiguous()
            want.append(agent_view(model._ready(), frames, r.plan_mask, i32(film)).cpu().numpy())
    tr = r.run(0)['trace']
    assert tr['view'].shape == (3, 2, 64, 64) and tr['view'].dtype == np.uint8 and tr['view_games'].tolist() == film
    assert same(tr['view'], np.stack(want))
    assert r.plan_mask.any() and (tr['view'][:, :, 59:63, 31] == 255).all()


# ---- 8. non-finite weights -----------------------------------------------------------------------------------------------------------------
def test_a_habit_head_of_nan_weights_records_failed_draws(model):
    import daimc_amd
    from oracle import nonfinite as NF
    from train_common import SEED, family
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.5, 1.0, 1.0, device=DEV, seed=SEED, init_weights=False)
    m.load_flat_weights(NF.poisoned_weights(family('g115'), 'top.qpi_net.0.weight', (3, 0)))
    E, ticks = 3, 12
    games = daimc_amd.Game(E, model=m, seed=7)
    res = daimc_amd.AgentRunner(m, games, 'habit', steps=STEPS, jumps=JUMPS, round_ticks=ROUND, report_ticks=REPORT, trace=True).run(ticks)
    tr = res['trace']
    assert tr['decided'].all() and (tr['choice'] == -1).all() and (tr['action'] == -1).all() and (tr['queue_len'] == 0).all()
    assert np.isnan(tr['probs']).all() and np.isfinite(tr['u']).all() and (tr['changed'] == 0).all()
    assert res['failed_ticks'] == ticks
    for t in range(ticks - 1):
        if (t + 1) % ROUND:                                          # no round reset between the two ticks: nothing moved
            assert same(tr['state'][t], tr['state'][t + 1]) and same(tr['last_r'][t], tr['last_r'][t + 1]), t
    assert same(tr['state'][-1], res['state']) and same(tr['last_r'][-1], res['last_r'])


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(model):
    import daimc_amd
    from daimc_amd import _lib
    E, T = 4, 3
    games = daimc_amd.Game(E, model=model, seed=1)
    st = daimc_amd.AgentState(model._ready(), E, 4)
    tr = daimc_amd.AgentTrace()
    tr.bind(model._ready(), E)
    tr.reserve(T)
    e = model._ready()
    before = {k: getattr(tr, k).clone() for k in tr.FIELDS}
    p = lambda t: C.c_void_p(t.data_ptr())
    ids, s = i32([0, 1, 2, 3]), tr._struct
    ptrs = [getattr(s, f) for f in _lib.TRACE_FIELDS]

    def struct(T_=T, E_=E, Lp=16, null=None):
        return _lib.EfeAgentTrace(*[None if f == null else v for f, v in zip(_lib.TRACE_FIELDS, ptrs)], T_, E_, Lp)

    def msg(rc):
        assert rc == 1
        return e.lib.efe_last_error(e.ctx).decode()
    tick = lambda trs=s, row=0, ag=st._struct, state=games.current_s: e.lib.efe_agent_trace_tick(
        e.ctx, C.byref(ag), C.byref(trs) if trs is not None else None, row, p(state) if state is not None else None, p(games.last_r), e.stream())
    a = st._struct
    assert 'efe_agent_trace_tick: E < 1' in msg(tick(ag=_lib.EfeAgent(a.queue, a.head, a.len, a.crossings, a.reward_sum, 0, a.cap)))
    assert 'efe_agent_trace_tick: E < 1' in msg(tick(trs=struct(E_=0)))
    for row in (-1, T):
        assert 'efe_agent_trace_tick: row' in msg(tick(row=row))
    assert 'efe_agent_trace_tick: a NULL array in efe_agent_trace' in msg(tick(trs=struct(null='action')))
    assert 'efe_agent_trace_tick: trace is NULL' in msg(tick(trs=None))
    assert 'efe_agent_trace_tick: state or last_r is NULL' in msg(tick(state=None))
    assert 'efe_agent_trace_tick: the record holds' in msg(tick(trs=struct(E_=E + 1)))

    probs = torch.full((E, 4), 0.25, device=DEV)
    dec = lambda trs=s, row=0, n=E, mode=_lib.EFE_AGENT_PROBS, ids_=ids, probs_=probs: e.lib.efe_agent_trace_decision(
        e.ctx, C.byref(trs), row, p(ids_) if ids_ is not None else None, n, mode, None, None, None, None, p(probs_) if probs_ is not None else None,
        1, C.c_float(1.0), None, None, 0, e.stream())
    assert 'efe_agent_trace_decision: E < 1' in msg(dec(trs=struct(E_=-2)))
    for n in (-1, E + 1):
        assert 'efe_agent_trace_decision: n < 0 or n > E' in msg(dec(n=n))
    for row in (-1, T):
        assert 'efe_agent_trace_decision: row' in msg(dec(row=row))
    assert 'efe_agent_trace_decision: unknown mode' in msg(dec(mode=7))
    assert 'efe_agent_trace_decision: ids is NULL' in msg(dec(ids_=None))
    assert 'efe_agent_trace_decision: mode probs needs probs' in msg(dec(probs_=None))
    assert 'efe_agent_trace_decision: modes ai' in msg(dec(mode=_lib.EFE_AGENT_AI))
    assert 'efe_agent_trace_decision: a NULL array' in msg(dec(trs=struct(null='probs')))

    D = 5
    H_act, H_len = torch.zeros(2, E, D, dtype=torch.int32, device=DEV), torch.full((2, E), D, dtype=torch.int32, device=DEV)
    H_active, mask = torch.ones(2, E, dtype=torch.uint8, device=DEV), torch.full((E, 32, 32), SENTINEL, device=DEV)
    pm = lambda n=E, E_=E, jumps=1, A=4, slots=E, ha=H_act, mk=mask: e.lib.efe_agent_plan_mask(
        e.ctx, p(ids), n, E_, p(games.current_s), p(ha) if ha is not None else None, p(H_len), p(H_active), 2, slots, D, jumps, A,
        p(mk) if mk is not None else None, e.stream())
    assert 'efe_agent_plan_mask: E < 1' in msg(pm(E_=0, n=0))
    for n in (-1, E + 1):
        assert 'efe_agent_plan_mask: n < 0 or n > E' in msg(pm(n=n))
    assert 'efe_agent_plan_mask: jumps < 1' in msg(pm(jumps=0))
    for A in (3, 5):
        assert 'efe_agent_plan_mask: A = ' in msg(pm(A=A))
    assert 'efe_agent_plan_mask: the history has fewer' in msg(pm(slots=E - 1))
    assert 'efe_agent_plan_mask: ids, state' in msg(pm(ha=None)) and 'efe_agent_plan_mask: ids, state' in msg(pm(mk=None))

    frames, view = torch.zeros(E, 64, 64, device=DEV), torch.full((E, 64, 64), 9, dtype=torch.uint8, device=DEV)
    vw = lambda n=E, E_=E, fr=frames, mk=None, ids_=None, out=view: e.lib.efe_agent_view(
        e.ctx, p(fr) if fr is not None else None, p(mk) if mk is not None else None, p(ids_) if ids_ is not None else None, n, E_,
        p(out) if out is not None else None, e.stream())
    assert 'efe_agent_view: E < 1' in msg(vw(E_=0, n=0))
    for n in (-1, E + 1):
        assert 'efe_agent_view: n < 0 or n > E' in msg(vw(n=n))
    assert 'efe_agent_view: frames or view is NULL' in msg(vw(fr=None)) and 'efe_agent_view: frames or view is NULL' in msg(vw(out=None))
    assert 'efe_agent_view: a mask needs ids' in msg(vw(mk=mask))
    with pytest.raises(ValueError):
        daimc_amd.AgentTrace(max_path=0)
    with pytest.raises(ValueError):
        daimc_amd.AgentRunner(model, games, 'habit', trace=daimc_amd.AgentTrace(frames=[E]))
    with pytest.raises(TypeError):
        daimc_amd.AgentRunner(model, games, 'habit', trace='yes')
    torch.cuda.synchronize()
    for k, v in before.items():                                      # a refused call launches nothing
        assert same(getattr(tr, k).cpu().numpy(), v.cpu().numpy()), k
    assert (mask == SENTINEL).all() and (view == 9).all()


# ---- 10. the command line ------------------------------------------------------------------------------------------------------------------
def test_run_agent_writes_the_record(tmp_path, capsys):
    import importlib.util
    import json
    import os
    from conftest import ROOT
    import daimc_amd
    spec = importlib.util.spec_from_file_location('run_agent', os.path.join(ROOT, 'tools', 'run_agent.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, npz = tmp_path / 'run.json', tmp_path / 'trace.npz'
    base = ['--network', 'random', '--method', 'habit', '--duration', '30', '--games', '2', '--steps', '3', '--out', str(out)]
    mod.main(base + ['--trace', str(npz), '--trace-frames', '2', '--frame-every', '3'])
    z = np.load(npz)
    shapes = {'state': (7,), 'last_r': (), 'action': (), 'queue_len': (), 'changed': (), 'decided': (), 'choice': (), 'u': (), 'G': (4,),
              'terms': (3, 4), 'probs': (4,), 'path': (16,), 'path_len': ()}
    assert set(shapes) == set(daimc_amd.AgentTrace.FIELDS) and set(z.files) == set(shapes) | {'view', 'view_games'}
    for k, tail in shapes.items():
        assert z[k].shape == (30, 2) + tail and z[k].dtype == {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}[
            daimc_amd.AgentTrace.FIELDS[k][1]], k
    assert z['view'].shape == (10, 2, 64, 64) and z['view'].dtype == np.uint8
    assert z['decided'].sum() == json.loads(out.read_text())['decisions'] >= 2 * 30 // 3
    traced_out = capsys.readouterr().out
    mod.main(base)                                                   # without --trace the tool prints what it printed
    plain_out = capsys.readouterr().out
    assert [ln for ln in traced_out.splitlines() if 'trace.npz' not in ln][-1].split('decisions')[1] == plain_out.splitlines()[-1].split('decisions')[1]
    assert '.npz' not in plain_out
