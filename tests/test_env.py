"""Dynamic-dSprites environment: CPU oracle vs the fixtures captured from the reference `Game`, and
(-m gpu) the HIP kernels vs the same fixtures, bit-exact (integer / exactly-representable state arithmetic)."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import load_golden, ROOT
from oracle import env_oracle as EV


def test_env_oracle_vs_reference_fixture():
    g = load_golden('env')
    seed = int(g['seed'])
    assert np.array_equal(EV.new_image_all(seed, np.zeros((6, 7), np.float32), int(g['init_stage'])), g['s_init'])   # constructor state
    assert not g['r_init'].any() and not g['s_init'][:, 6].any()
    s, r = EV.reset(seed, 6, 0)
    assert np.array_equal(s, g['s_reset']) and np.array_equal(r, g['r_reset'])
    bank = EV.sprite_bank()
    s, r = g['s_in'].copy(), g['r_in'].copy()
    assert np.array_equal(EV.render(s, r, bank)[..., 0], g['frames_in'])
    for t in range(len(g['actions'])):
        ch = EV.step(seed, s, r, g['actions'][t], int(g['repeats']), 1 + t)
        assert np.array_equal(ch, g['changed'][t])
        assert np.array_equal(s, g['states'][t]) and np.array_equal(r, g['last_r'][t])
        assert np.array_equal(EV.render(s, r, bank)[..., 0], g['frames'][t])
    assert g['changed'].sum() >= 4          # the fixture exercises finished rounds (latent resampling + reward restart)


def test_env_render_rejects_out_of_range_reward():
    s, r = EV.reset(1, 2, 0)
    r[1] = 1.5
    with pytest.raises(ValueError):
        EV.render(s, r, EV.sprite_bank())


@pytest.mark.gpu
def test_env_kernels_vs_reference_fixture():
    import daimc_amd
    g = load_golden('env')
    games = daimc_amd.Game(6, device='cuda:0', seed=int(g['seed']), init_stage=int(g['init_stage']))
    # the constructor is new_image_all (game_environment.py:21): fresh latents, reward 0, last_r 0
    assert np.array_equal(games.current_s.cpu().numpy(), g['s_init']) and np.array_equal(games.last_r.cpu().numpy(), g['r_init'])
    games.randomize_environment_all(stage=0)
    assert np.array_equal(games.current_s.cpu().numpy(), g['s_reset']) and np.array_equal(games.last_r.cpu().numpy(), g['r_reset'])
    games.current_s.copy_(torch.from_numpy(g['s_in'])); games.last_r.copy_(torch.from_numpy(g['r_in']))
    f = games.current_frame_all()
    assert f.shape == (6, 64, 64, 1)
    assert np.array_equal(f.cpu().numpy()[..., 0], g['frames_in'])
    for t in range(len(g['actions'])):
        ch = games.pi_to_action_all(g['actions'][t], repeats=int(g['repeats']), stage=1 + t)
        assert np.array_equal(ch.cpu().numpy(), g['changed'][t])
        assert np.array_equal(games.current_s.cpu().numpy(), g['states'][t])
        assert np.array_equal(games.last_r.cpu().numpy(), g['last_r'][t])
        assert np.array_equal(games.current_frame_all().cpu().numpy()[..., 0], g['frames'][t])
    games.last_r[2] = -1.5
    with pytest.raises(ValueError):
        games.current_frame_all()
    with pytest.raises(ValueError):
        games.pi_to_action_all([0, 1, 2, 3, 4, 0])


@pytest.mark.gpu
def test_closed_loop_batch_producer():
    """make_batch_dsprites_active_inference (util.py:55-80) end to end on the device: observe -> EFE rollouts -> act -> observe"""
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=5)
    games = daimc_amd.Game(16, model=m, seed=9)
    s_before = games.current_s.clone()
    o0, o1, pi0, logP = daimc_amd.make_batch_dsprites_active_inference(games, m, deepness=2, samples=2, repeats=3)
    assert o0.shape == (16, 64, 64, 1) and o1.shape == (16, 64, 64, 1) and pi0.shape == (16, 4) and logP.shape == (16, 4)
    assert torch.all(pi0.sum(1) == 1) and torch.isfinite(logP).all()
    # every game either moved, was already at a wall for its action, or finished a round; reward bar decays by 0.95^3 otherwise
    moved = (games.current_s != s_before).any(dim=1)
    a = pi0.argmax(1)
    wall = ((a == 1) & (s_before[:, 5] == 0)) | ((a == 2) & (s_before[:, 4] == 31)) | ((a == 3) & (s_before[:, 4] == 0))
    assert bool((moved | wall).all())
    # sharded games reproduce the unsharded ones (global game keys)
    g_all = daimc_amd.Game(8, model=m, seed=3); g_all.randomize_environment_all(stage=4)
    g_hi = daimc_amd.Game(4, model=m, seed=3, game_offset=4); g_hi.randomize_environment_all(stage=4)
    assert torch.equal(g_all.current_s[4:], g_hi.current_s) and torch.equal(g_all.last_r[4:], g_hi.last_r)


# ---------------------------------------------------------------------------------------------------------------------
# The exhaustive sweep (tests/golden/env_sweep.npz, oracle/make_golden_env.py --sweep): one step of the reference Game from every
# (shape, x, y, action) at repeats 1, 2 and 5, every frame's checksum, a 40-step trajectory, find_move and the clamped draw.
# Everything below is compared bit for bit: the state arithmetic is integral or exactly representable and the tick is a single
# fp32 multiply, so no tolerance enters.
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = -777.25
CHUNK = 2048                       # frames per render call of the sweep: 32 MiB


@pytest.fixture(scope='module')
def sweep():
    g = load_golden('env_sweep')
    g['meta'] = json.loads(str(g['meta']))
    return g


@pytest.fixture(scope='module')
def bank():
    return EV.sprite_bank()


def _state(lat, acc):
    s = np.zeros((len(lat), 7), dtype=np.float32)
    s[:, :6], s[:, 6] = lat, acc
    return s


def _f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).copy()


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _crcs(frames):
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    return np.array([zlib.crc32(f.tobytes()) for f in frames], dtype=np.uint32)


def _grid_in(g):
    return _state(g['s_in'], g['acc_in']), _f32(g['r_in_bits']), g['actions'].astype(np.int64)


def _tuples(g, wrong):
    """the first five grid tuples (shape, x, y, action) at which `wrong` is set"""
    return [(int(g['s_in'][i, 1]), int(g['s_in'][i, 4]), int(g['s_in'][i, 5]), int(g['actions'][i])) for i in np.flatnonzero(wrong)[:5]]


def _check_step(g, rep, s, r, ch):
    """state [G,7], last_r [G] and flags [G] after one step of the grid against the recorded reference, bit for bit"""
    want = _state(g[f's_r{rep}'], g[f'acc_r{rep}'])
    wrong = (_bits(s) != _bits(want)).any(axis=1) | (_bits(r) != g[f'r_bits_r{rep}']) | (np.asarray(ch, dtype=bool) != g[f'changed_r{rep}'])
    assert not wrong.any(), f'repeats={rep}: {int(wrong.sum())} games differ; first (shape, x, y, action): {_tuples(g, wrong)}'


def _check_frame_crcs(g, key, crcs):
    wrong = crcs != g[key]
    assert not wrong.any(), f'{key}: {int(wrong.sum())} frames differ; first (shape, x, y, action): {_tuples(g, wrong)}'


def _stored_frame_states(g):
    """states and last_r of the 64 games whose whole frames are stored (before or after the repeats = 5 step)"""
    s_in, r_in, _ = _grid_in(g)
    s5, r5 = _state(g['s_r5'], g['acc_r5']), _f32(g['r_bits_r5'])
    fg, after = g['frame_games'], g['frame_after'].astype(bool)
    return np.where(after[:, None], s5[fg], s_in[fg]), np.where(after, r5[fg], r_in[fg])


def test_sweep_fixture_is_small_and_is_the_documented_grid(sweep):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'env_sweep.npz')) < 512 * 1024
    m = sweep['meta']
    s, r, a = EV.sweep_grid()
    gs, gr, ga = _grid_in(sweep)
    assert len(s) == 12288 and np.array_equal(_bits(s), _bits(gs)) and np.array_equal(_bits(r), _bits(gr)) and np.array_equal(a, ga)
    # every (shape, x, y, action) once; each action, x and shape meets every starting last_r
    assert len({(int(p[1]), int(p[4]), int(p[5]), int(q)) for p, q in zip(s, a)}) == 3 * 32 * 32 * 4
    for col in (a, s[:, 4], s[:, 1]):
        assert len(set(zip(col.tolist(), _bits(r).tolist()))) == len(set(col.tolist())) * 7
    assert (m['seed'], m['stage'], m['repeats']) == (77, 5, [1, 2, 5])
    # a finished round needs `up` from y >= 32 - repeats: 3 shapes x 32 x positions x repeats rows
    assert m['finished'] == [96, 192, 480] == [int(sweep[f'changed_r{k}'].sum()) for k in (1, 2, 5)]
    assert m['traj_finished'] == int(sweep['traj_changed'].sum()) >= 30
    assert sweep['frames'].shape == (64, 64, 64) and 3 * int((sweep['changed_r5'][sweep['frame_games']] & (sweep['frame_after'] == 1)).sum()) >= 64
    assert m['clamp']['reached'] and m['clamp']['word'] == 2 ** 24 - 1 and m['clamp']['latent'] in (3, 4, 5)


@pytest.mark.parametrize('repeats', [1, 2, 5])
def test_env_oracle_step_sweep(sweep, repeats):
    s, r, a = _grid_in(sweep)
    ch = EV.step(sweep['meta']['seed'], s, r, a, repeats, sweep['meta']['stage'])
    _check_step(sweep, repeats, s, r, ch)


def test_env_oracle_render_sweep(sweep, bank):
    s_in, r_in, _ = _grid_in(sweep)
    s5, r5 = _state(sweep['s_r5'], sweep['acc_r5']), _f32(sweep['r_bits_r5'])
    for key, s, r in (('crc_in', s_in, r_in), ('crc_r5', s5, r5)):
        crcs = np.concatenate([_crcs(EV.render(s[i:i + CHUNK], r[i:i + CHUNK], bank)) for i in range(0, len(s), CHUNK)])
        _check_frame_crcs(sweep, key, crcs)
    fs, fr = _stored_frame_states(sweep)
    assert np.array_equal(_bits(EV.render(fs, fr, bank)[..., 0]), _bits(sweep['frames']))


def test_env_oracle_trajectory(sweep, bank):
    m = sweep['meta']
    s, r = EV.reset(m['seed'], sweep['traj_s0'].shape[0], m['traj_reset_stage'])
    assert np.array_equal(_bits(s), _bits(_state(sweep['traj_s0'], sweep['traj_acc0']))) and np.array_equal(_bits(r), sweep['traj_r0_bits'])
    for t, a in enumerate(sweep['traj_actions']):
        ch = EV.step(m['seed'], s, r, a, m['traj_repeats'], m['traj_first_stage'] + t)
        assert np.array_equal(_bits(s), _bits(_state(sweep['traj_s'][t], sweep['traj_acc'][t]))), t
        assert np.array_equal(_bits(r), sweep['traj_r_bits'][t]) and np.array_equal(ch, sweep['traj_changed'][t]), t
    # the chain of 0.95 ticks is long: some game went at least 20 steps (100 ticks) without a finished round
    run = np.zeros(s.shape[0], dtype=int); longest = 0
    for ch in sweep['traj_changed']:
        run = np.where(ch, 0, run + 1); longest = max(longest, int(run.max()))
    assert longest >= 20


def test_env_randint_clamp_at_the_largest_draw(sweep):
    c = sweep['meta']['clamp']
    size = EV.SIZES[c['latent']]
    u = EV.env_u(sweep['meta']['seed'], c['game'], c['stage'], c['latent'])
    assert u == np.float32(1.0) and np.float32(u) * np.float32(size) == size          # word 2^24 - 1 rounds to 1.0: int(u * size) = size
    assert EV.env_randint(sweep['meta']['seed'], c['game'], c['stage'], c['latent']) == c['expected'] == size - 1
    games = np.array([c['game'] - 1, c['game'], c['game'] + 1])
    assert EV.env_randint(sweep['meta']['seed'], games, c['stage'], c['latent'])[1] == size - 1           # the array form clamps too


def test_find_move_all_formula(sweep):
    import daimc_amd
    games = object.__new__(daimc_amd.Game)              # find_move_all reads the state only: no engine, no device
    games.device = torch.device('cpu')
    games.current_s = torch.zeros(3, 7)
    games.current_s[:, 1] = torch.tensor([0.0, 1.0, 2.0])
    for i, rnd in enumerate(sweep['meta']['find_move_randomness']):
        got = games.find_move_all(rnd)
        assert got.dtype == torch.float32 and np.array_equal(_bits(got), _bits(sweep['find_move'][i])), rnd


def test_game_refuses_a_short_sprite_bank():
    import daimc_amd
    with pytest.raises(ValueError, match='3581'):
        daimc_amd.Game(2, imgs=np.zeros((3580, 64, 64), np.uint8))


def _game(n, bank, **kw):
    import daimc_amd
    return daimc_amd.Game(n, imgs=bank, **kw)


def _load(games, s, r):
    games.current_s.copy_(torch.from_numpy(np.ascontiguousarray(s)))
    games.last_r.copy_(torch.from_numpy(np.ascontiguousarray(r)))


def _same(games, s, r):
    return np.array_equal(_bits(games.current_s), _bits(s)) and np.array_equal(_bits(games.last_r), _bits(r))


@pytest.mark.gpu
def test_game_accepts_exactly_the_bank_the_index_rule_needs():
    with pytest.raises(ValueError, match='3581'):
        _game(2, np.zeros((3580, 64, 64), np.uint8))
    games = _game(1, EV.sprite_bank(3581))
    games.current_s[0, :6] = torch.tensor([0.0, 2.0, 5.0, 39.0, 31.0, 31.0], device=games.device)      # index 3580, the last image
    s, r = games.current_s.cpu().numpy(), games.last_r.cpu().numpy()
    assert np.array_equal(_bits(games.current_frame_all()), _bits(EV.render(s, r, EV.sprite_bank(3581))))


@pytest.mark.gpu
@pytest.mark.parametrize('repeats', [1, 2, 5])
def test_env_step_sweep_gpu(sweep, bank, repeats):
    s, r, a = _grid_in(sweep)
    games = _game(len(s), bank, seed=sweep['meta']['seed'])
    _load(games, s, r)
    ch = games.pi_to_action_all(a, repeats=repeats, stage=sweep['meta']['stage'])
    _check_step(sweep, repeats, games.current_s.cpu().numpy(), games.last_r.cpu().numpy(), ch.cpu().numpy())


@pytest.mark.gpu
def test_env_render_sweep_gpu(sweep, bank, monkeypatch):
    s_in, r_in, _ = _grid_in(sweep)
    s5, r5 = _state(sweep['s_r5'], sweep['acc_r5']), _f32(sweep['r_bits_r5'])
    games = _game(CHUNK, bank)
    for key, s, r in (('crc_in', s_in, r_in), ('crc_r5', s5, r5)):
        crcs = []
        for i in range(0, len(s), CHUNK):
            _load(games, s[i:i + CHUNK], r[i:i + CHUNK])
            f = games.current_frame_nchw()
            assert f.shape == (CHUNK, 1, 64, 64) and f.dtype == torch.float32 and f.is_contiguous()
            crcs.append(_crcs(f.cpu().numpy()))
        _check_frame_crcs(sweep, key, np.concatenate(crcs))
    few = _game(64, bank)
    _load(few, *_stored_frame_states(sweep))
    made = []
    nchw = few.current_frame_nchw
    monkeypatch.setattr(few, 'current_frame_nchw', lambda: made.append(nchw()) or made[-1])
    f = few.current_frame_all()
    assert np.array_equal(_bits(f)[..., 0], _bits(sweep['frames']))
    # current_frame_all is the NCHW frame's own memory, seen as [G,64,64,1]
    assert len(made) == 1 and f.shape == (64, 64, 64, 1) and f.is_contiguous() and f.data_ptr() == made[0].data_ptr()


@pytest.mark.gpu
def test_env_trajectory_gpu(sweep, bank):
    m = sweep['meta']
    games = _game(sweep['traj_s0'].shape[0], bank, seed=m['seed'])
    games.randomize_environment_all(stage=m['traj_reset_stage'])
    assert _same(games, _state(sweep['traj_s0'], sweep['traj_acc0']), _f32(sweep['traj_r0_bits']))
    for t, a in enumerate(sweep['traj_actions']):
        ch = games.pi_to_action_all(a.astype(np.int64), repeats=m['traj_repeats'], stage=m['traj_first_stage'] + t)
        s, r = _state(sweep['traj_s'][t], sweep['traj_acc'][t]), _f32(sweep['traj_r_bits'][t])
        assert _same(games, s, r) and np.array_equal(ch.cpu().numpy(), sweep['traj_changed'][t]), t
        assert np.array_equal(_bits(games.current_frame_all()), _bits(EV.render(s, r, bank))), t


@pytest.mark.gpu
@pytest.mark.parametrize('E', [1, 127, 129])
def test_env_ragged_launch_leaves_other_rows_alone(bank, E):
    """a game count that is no multiple of the 128-thread block: the first E rows equal the oracle, every row behind them keeps its sentinel"""
    rows, seed = 384, 77
    games = _game(E, bank, seed=seed)
    big_s = torch.full((rows, 7), SENTINEL, device=games.device)
    big_r = torch.full((rows,), SENTINEL, device=games.device)
    games.current_s, games.last_r = big_s[:E], big_r[:E]

    def untouched():
        return bool((big_s[E:] == SENTINEL).all()) and bool((big_r[E:] == SENTINEL).all())

    games.randomize_environment_all(stage=2)
    s, r = EV.reset(seed, E, 2)
    assert _same(games, s, r) and untouched()
    games.new_image_all(stage=3)
    EV.new_image_all(seed, s, 3)
    assert _same(games, s, r) and untouched()
    games.current_s[:, 5] = 31.0                          # every game one `up` away from finishing
    s[:, 5] = 31.0
    ch = games.pi_to_action_all(np.zeros(E, np.int64), repeats=5, stage=4)
    och = EV.step(seed, s, r, np.zeros(E, np.int64), 5, 4)
    assert och.all() and np.array_equal(ch.cpu().numpy(), och)
    assert _same(games, s, r) and untouched()
    assert np.array_equal(_bits(games.current_frame_all()), _bits(EV.render(s, r, bank)))


@pytest.mark.gpu
def test_env_draws_gpu(bank):
    E, seed = 4097, 77
    games = _game(E, bank, seed=seed)
    games.randomize_environment_all(stage=11)
    s, r = EV.reset(seed, E, 11)
    for k, size in enumerate(EV.SIZES):                  # every value of every latent occurs in the oracle's draw
        assert set(s[:, k].tolist()) == set(range(size)), k
    assert -10.0 <= s[:, 6].min() < -9.9 and 9.9 < s[:, 6].max() <= 10.0 and -1.0 <= r.min() < -0.99 and 0.99 < r.max() <= 1.0
    wrong = (_bits(games.current_s) != _bits(s)).any(axis=1) | (_bits(games.last_r) != _bits(r))       # s[6], last_r: multiply, round, then add
    assert not wrong.any(), f'reset: games {np.flatnonzero(wrong)[:5]} differ'
    games.new_image_all(stage=12)
    EV.new_image_all(seed, s, 12)
    assert _same(games, s, r)


@pytest.mark.gpu
def test_env_largest_draw_is_clamped_gpu(sweep, bank):
    c = sweep['meta']['clamp']
    games = _game(1, bank, seed=sweep['meta']['seed'], game_offset=c['game'])
    games.new_image_all(stage=c['stage'])
    s = EV.new_image_all(sweep['meta']['seed'], np.zeros((1, 7), np.float32), c['stage'], game_offset=c['game'])
    assert s[0, c['latent']] == c['expected'] == EV.SIZES[c['latent']] - 1
    assert _same(games, s, np.zeros(1, np.float32))
    assert np.array_equal(_bits(games.current_frame_all()), _bits(EV.render(s, np.zeros(1, np.float32), bank)))


@pytest.mark.gpu
def test_finished_round_in_a_shard_gpu(bank):
    """a round that finishes in the upper shard of a sharded Game draws the same fresh latents as in the whole Game (global game keys)"""
    seed = 77
    g_all, g_hi = _game(8, bank, seed=seed), _game(4, bank, seed=seed, game_offset=4)
    s, r = EV.reset(seed, 8, 2)
    s[:, 5] = 31.0
    _load(g_all, s, r); _load(g_hi, s[4:], r[4:])
    up = np.zeros(8, np.int64)
    ch_all, ch_hi = g_all.pi_to_action_all(up, repeats=1, stage=6), g_hi.pi_to_action_all(up[4:], repeats=1, stage=6)
    och = EV.step(seed, s, r, up, 1, 6)
    assert och.all() and bool(ch_all.all()) and bool(ch_hi.all())
    assert _same(g_all, s, r) and _same(g_hi, s[4:], r[4:])
    assert len({tuple(row) for row in s[:, :6].tolist()}) == 8          # the eight games drew different latents: an offset of 0 would show


@pytest.mark.gpu
def test_reward_bar_edges_gpu(bank):
    ok = np.array([1.0, -1.0, -0.0, 2.0 ** -149], dtype=np.float32)
    games = _game(4, bank, seed=3)
    games.last_r.copy_(torch.from_numpy(ok))
    s = games.current_s.cpu().numpy()
    want = EV.render(s, ok, bank)
    assert _bits(want[2, 0, 0])[0] == 0x80000000 and _bits(want[3, 0, 0])[0] == 1          # the zero keeps its sign, the subnormal its bit
    assert np.array_equal(_bits(games.current_frame_all()), _bits(want))
    one = np.float32(1.0)
    for bad in (np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), np.float32(np.nan), np.float32(np.inf)):
        r = ok.copy(); r[1] = bad
        games.last_r.copy_(torch.from_numpy(r))
        with pytest.raises(ValueError):
            games.current_frame_all()
        with pytest.raises(ValueError):
            EV.render(s, r, bank)
        assert _same(games, s, r), bad                  # a refused frame changes nothing


@pytest.mark.gpu
def test_subnormal_tick_gpu(bank):
    """five `down` steps from last_r = +-1e-40: the tick's fp32 product stays subnormal and is not flushed (the library is built with no
    denormal-flushing flag), so it equals numpy's fp32 product bit for bit"""
    games = _game(2, bank, seed=3)
    s = games.current_s.cpu().numpy()
    r = np.array([1e-40, -1e-40], dtype=np.float32)
    assert 0 < abs(r[0]) < np.finfo(np.float32).tiny
    _load(games, s, r)
    down = np.ones(2, np.int64)
    for t in range(5):
        games.pi_to_action_all(down, repeats=1, stage=20 + t)
        EV.step(3, s, r, down, 1, 20 + t)
        assert r[0] != 0 and _same(games, s, r), (t, _bits(games.last_r), _bits(r))


@pytest.mark.gpu
def test_batch_producers_equal_their_parts_gpu(bank):
    """make_batch_dsprites_active_inference at the training configuration and train.make_batch_random are their parts and nothing else:
    render, plan (a twin model at the same stage, a twin generator), step with the game's own stage, render"""
    import daimc_amd
    n, seed = 8, 9
    m, twin = (daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=5) for _ in range(2))
    gen, gen_plan, gen_draw = (torch.Generator(device='cuda:0').manual_seed(4242) for _ in range(3))
    games = _game(n, bank, model=m, seed=seed)
    games.randomize_environment_all()
    s, r = games.current_s.cpu().numpy(), games.last_r.cpu().numpy()
    stage_model, stage_game = m._stage, games._stage
    o0, o1, pi0, log_Ppi = daimc_amd.make_batch_dsprites_active_inference(games, m, deepness=1, samples=1, calc_mean=True, repeats=5, generator=gen)
    want_o0 = EV.render(s, r, bank)
    assert np.array_equal(_bits(o0), _bits(want_o0))
    _, t_log, t_Ppi, _ = daimc_amd.plan_actions_batch(twin, torch.from_numpy(want_o0).to(twin.device), deepness=1, samples=1, calc_mean=True,
                                                      generator=gen_plan, stage=stage_model)
    assert torch.equal(log_Ppi, t_log)
    choice = torch.multinomial(t_Ppi, 1, generator=gen_draw).squeeze(1)
    assert torch.equal(pi0, torch.nn.functional.one_hot(choice, 4).to(pi0.dtype))
    ch = EV.step(seed, s, r, choice.cpu().numpy(), 5, stage_game)
    assert _same(games, s, r) and np.array_equal(_bits(o1), _bits(EV.render(s, r, bank)))
    assert games._stage == stage_game + 1 and ch.shape == (n,)

    stage_game = games._stage
    o0, o1, pi0 = daimc_amd.train.make_batch_random(games, repeats=5, generator=gen)
    s, r = EV.reset(seed, n, stage_game)
    assert o0.shape == (n, 1, 64, 64) and np.array_equal(_bits(o0).reshape(n, 64, 64, 1), _bits(EV.render(s, r, bank)))
    assert bool((pi0.sum(1) == 1).all()) and bool(((pi0 == 0) | (pi0 == 1)).all())
    EV.step(seed, s, r, pi0.argmax(1).cpu().numpy(), 5, stage_game + 1)
    assert _same(games, s, r) and np.array_equal(_bits(o1).reshape(n, 64, 64, 1), _bits(EV.render(s, r, bank)))
