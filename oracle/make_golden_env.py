"""ORACLE tooling (build container only): captures fixtures of the reference's Dynamic-dSprites `Game`
(/root/reference/src/game_environment.py) for SURVEY row 8f-3.  The dSprites archive is absent, so `numpy.load` is patched
to hand the Game the synthetic sprite bank of oracle/env_oracle.py (the shapes the Game reads: imgs uint8 [N,64,64],
metadata['latents_sizes'] = [1,3,6,40,32,32]); `torch.randint` / `torch.rand` are patched to consume the addressable
Philox stream (tag 0x60) in the reference's own call order.  Only tensors are written to tests/golden/env.npz.

`--sweep` writes tests/golden/env_sweep.npz instead: one step of the reference from EVERY (shape, x, y, action) at repeats
1, 2 and 5, the checksums of every rendered frame, a 40-step trajectory in which many rounds finish, find_move, and the
draw key at which the `size - 1` clamp of the latent draw acts.  Recorded tensors and plain settings only.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_env [--sweep]
"""
import os
import sys
import io
import json
import zlib
import zipfile
import contextlib
import numpy as np

sys.dont_write_bytecode = True
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import env_oracle as EV
from oracle import philox as PX

REF = '/root/reference'
SEED = 77


def reference_game(ctx):
    """the reference's Game class with np.load, torch.randint and torch.rand patched; ctx = {'stage', 'game', 'k', 'rand_blk'} addresses the draws.
    -> (Game, restore)"""
    sys.path.insert(0, REF)
    bank = EV.sprite_bank()
    meta = np.empty((), dtype=object)
    meta[()] = {'latents_sizes': np.array([1, 3, 6, 40, 32, 32])}
    fake = {'imgs': bank, 'latents_values': np.zeros((1, 6)), 'latents_classes': np.zeros((1, 6), dtype=np.int64), 'metadata': meta}
    np_load = np.load
    np.load = lambda *a, **k: fake

    def randint(*args, **kw):
        if len(args) == 2:
            high, size = args
        else:
            _, high, size = args
        high = int(high)
        k = ctx['k']; ctx['k'] = (k + 1) % 6
        assert high == EV.SIZES[k], (high, k)
        if tuple(size) == (1,):
            return torch.tensor([EV.env_randint(SEED, ctx['game'], ctx['stage'], k)])
        return torch.from_numpy(EV.env_randint(SEED, np.arange(size[0]), ctx['stage'], k))

    def rand(*size, **kw):
        n = size[0]
        blk = ctx['rand_blk']; ctx['rand_blk'] = 7 if blk == 6 else 6
        return torch.from_numpy(EV.env_u(SEED, np.arange(n), ctx['stage'], blk).astype(np.float32))

    torch.randint = randint
    torch.rand = rand
    from src.game_environment import Game

    def restore():
        np.load = np_load
    return Game, restore


def main():
    bank = EV.sprite_bank()
    ctx = {'stage': 1000, 'game': 0, 'k': 0, 'rand_blk': 6}
    Game, restore = reference_game(ctx)

    G, T, REPEATS = 6, 6, 2
    with contextlib.redirect_stdout(io.StringIO()):
        games = Game(G)                                   # __init__ draws (new_image_all) use stage 1000
        s_init, r_init = games.current_s.numpy().copy(), games.last_r.numpy().copy()
        assert np.array_equal(s_init, EV.new_image_all(SEED, np.zeros((G, 7), np.float32), 1000)) and not r_init.any(), 'constructor mismatch'
        ctx.update(stage=0, k=0, rand_blk=6)
        games.randomize_environment_all()
    restore()
    s_reset, r_reset = games.current_s.numpy().copy(), games.last_r.numpy().copy()
    o_s, o_r = EV.reset(SEED, G, 0)
    assert np.array_equal(s_reset, o_s) and np.array_equal(r_reset, o_r), 'reset mismatch'

    games.current_s[:, 5] = torch.tensor([31.0, 30.0, 5.0, 31.0, 0.0, 29.0])      # some games about to finish a round
    games.current_s[:, 4] = torch.tensor([3.0, 20.0, 31.0, 16.0, 0.0, 15.0])
    games.current_s[:, 1] = torch.tensor([0.0, 1.0, 2.0, 0.0, 1.0, 2.0])
    s_in, r_in = games.current_s.numpy().copy(), games.last_r.numpy().copy()
    frames_in = games.current_frame_all().numpy().copy()
    os_, or_ = s_in.copy(), r_in.copy()
    assert np.array_equal(EV.render(os_, or_, bank), frames_in), 'render mismatch'

    actions = np.array([[0, 0, 2, 0, 1, 0], [0, 0, 2, 3, 1, 0], [1, 0, 3, 0, 3, 0], [0, 2, 0, 0, 2, 3], [3, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0]])
    states, rs, frames, changed = [], [], [], []
    for t in range(T):
        ch = np.zeros(G, dtype=bool)
        for e in range(G):
            ctx.update(stage=1 + t, game=e, k=0)
            ch[e] = games.pi_to_action(int(actions[t, e]), e, repeats=REPEATS)
        och = EV.step(SEED, os_, or_, actions[t], REPEATS, 1 + t)
        if not (np.array_equal(games.current_s.numpy(), os_) and np.array_equal(games.last_r.numpy(), or_)):
            print('ref', games.current_s.numpy(), games.last_r.numpy()); print('orc', os_, or_)
            raise AssertionError(f'step {t} mismatch')
        assert np.array_equal(ch, och)
        f = games.current_frame_all().numpy().copy()
        assert np.array_equal(EV.render(os_, or_, bank), f)
        states.append(os_.copy()); rs.append(or_.copy()); frames.append(f[..., 0]); changed.append(ch)
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'env.npz'), seed=SEED, s_init=s_init, r_init=r_init, init_stage=1000, s_reset=s_reset, r_reset=r_reset, s_in=s_in,
                        r_in=r_in, frames_in=frames_in[..., 0], actions=actions, repeats=REPEATS, states=np.stack(states),
                        last_r=np.stack(rs), frames=np.stack(frames), changed=np.stack(changed))
    print('env golden written; rounds finished per step:', [int(c.sum()) for c in changed])


# ---------------------------------------------------------------------------------------------------------------------
# --sweep
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_STAGE, SWEEP_REPEATS = 5, (1, 2, 5)
TRAJ_GAMES, TRAJ_STEPS, TRAJ_REPEATS, TRAJ_ACTION_SEED = 32, 40, 5, 20240607
CLAMP_STAGE, CLAMP_CHUNK, CLAMP_MAX_DRAWS = 3, 1 << 20, 1 << 27


def _bits(r):
    return np.ascontiguousarray(r, dtype=np.float32).view(np.uint32).copy()


def _pack(s):
    """state [n,7] float32 -> (latents uint8 [n,6], accumulated reward float32 [n]); the latents are small whole numbers"""
    lat = s[:, :6].astype(np.uint8)
    assert np.array_equal(lat.astype(np.float32), s[:, :6])
    return lat, s[:, 6].astype(np.float32).copy()


def _crc(frame):
    return zlib.crc32(np.ascontiguousarray(frame, dtype=np.float32).tobytes())


def _ref_step_all(games, ctx, actions, repeats, stage):
    ch = np.zeros(len(actions), dtype=bool)
    for e in range(len(actions)):
        ctx.update(stage=stage, game=e, k=0)
        ch[e] = games.pi_to_action(int(actions[e]), e, repeats=repeats)
    return ch


def _ref_frames(games, idx=None):
    """reference frames one game at a time ([64,64] float32), so that 12288 of them never sit in memory at once"""
    for e in (range(games.games_no) if idx is None else idx):
        yield games.current_frame(int(e)).numpy()[..., 0]


def find_largest_draw():
    """first (game, latent in 3..5) at CLAMP_STAGE whose 24-bit word is 2^24 - 1: u01 rounds to 1.0 there, u * size to size, and the clamp acts"""
    k0, k1 = PX._key(SEED)
    best = (-1, 0, 3)
    for lo in range(0, CLAMP_MAX_DRAWS // 3, CLAMP_CHUNK):
        g = np.arange(lo, lo + CLAMP_CHUNK, dtype=np.uint64)
        for k in (3, 4, 5):
            x0 = PX.philox4x32_10(np.uint64(k) | (np.uint64(EV.TAG_ENV) << np.uint64(16)), g, np.uint64(PX.stream_id(EV.PASS_ENV, 0)),
                                  np.uint64(CLAMP_STAGE), k0, k1)[0] >> np.uint32(8)
            i = int(x0.argmax())
            if int(x0[i]) > best[0]:
                best = (int(x0[i]), lo + i, k)
        if best[0] == (1 << 24) - 1:
            break
    return best


def sweep():
    bank = EV.sprite_bank()
    ctx = {'stage': 1000, 'game': 0, 'k': 0, 'rand_blk': 6}
    Game, restore = reference_game(ctx)
    s_in, r_in, actions = EV.sweep_grid()
    G = len(s_in)
    out = {}
    out['s_in'], out['acc_in'] = _pack(s_in)
    out['r_in_bits'], out['actions'] = _bits(r_in), actions.astype(np.uint8)

    with contextlib.redirect_stdout(io.StringIO()):
        games = Game(G)
    crc_in = None
    finished = {}
    for rep in SWEEP_REPEATS:
        games.current_s = torch.from_numpy(s_in.copy()); games.last_r = torch.from_numpy(r_in.copy())
        if crc_in is None:
            crc_in = np.array([_crc(f) for f in _ref_frames(games)], dtype=np.uint32)
        ch = _ref_step_all(games, ctx, actions, rep, SWEEP_STAGE)
        s_ref, r_ref = games.current_s.numpy().copy(), games.last_r.numpy().copy()
        o_s, o_r = s_in.copy(), r_in.copy()
        o_ch = EV.step(SEED, o_s, o_r, actions, rep, SWEEP_STAGE)
        assert np.array_equal(o_s, s_ref) and np.array_equal(_bits(o_r), _bits(r_ref)) and np.array_equal(o_ch, ch), f'sweep repeats={rep}: oracle mismatch'
        out[f's_r{rep}'], out[f'acc_r{rep}'] = _pack(s_ref)
        out[f'r_bits_r{rep}'], out[f'changed_r{rep}'] = _bits(r_ref), ch
        finished[rep] = int(ch.sum())
    # games now holds the repeats = 5 result
    crc_out = np.array([_crc(f) for f in _ref_frames(games)], dtype=np.uint32)
    # 64 whole frames: 24 finished rounds and 20 other games after the step, 20 games before it
    fin = np.flatnonzero(ch)
    fg = np.concatenate([fin[np.linspace(0, len(fin) - 1, 24).astype(int)], (np.arange(20) * 613 + 101) % G, (np.arange(20) * 587 + 7) % G])
    fw = np.concatenate([np.ones(44, np.uint8), np.zeros(20, np.uint8)])          # 1: after the repeats = 5 step, 0: input state
    frames = np.zeros((64, 64, 64), np.float32)
    frames[:44] = np.stack(list(_ref_frames(games, fg[:44])))
    games.current_s = torch.from_numpy(s_in.copy()); games.last_r = torch.from_numpy(r_in.copy())
    frames[44:] = np.stack(list(_ref_frames(games, fg[44:])))
    assert ch[fg[:24]].all() and len(set(zip(fg.tolist(), fw.tolist()))) == 64
    o_in, o_out = EV.render(s_in, r_in, bank)[..., 0], EV.render(o_s, o_r, bank)[..., 0]
    assert np.array_equal(np.array([_crc(f) for f in o_in], np.uint32), crc_in), 'input frames: oracle mismatch'
    assert np.array_equal(np.array([_crc(f) for f in o_out], np.uint32), crc_out), 'repeats=5 frames: oracle mismatch'
    assert np.array_equal(o_out[fg[:44]].view(np.uint32), frames[:44].view(np.uint32)) and np.array_equal(o_in[fg[44:]].view(np.uint32), frames[44:].view(np.uint32))
    out.update(crc_in=crc_in, crc_r5=crc_out, frame_games=fg.astype(np.int32), frame_after=fw, frames=frames)

    # trajectory: reset at stage 0, then 40 steps of 5 repeats with `up` favoured so that many rounds finish
    T, N = TRAJ_STEPS, TRAJ_GAMES
    with contextlib.redirect_stdout(io.StringIO()):
        games = Game(N)
        ctx.update(stage=0, k=0, rand_blk=6)
        games.randomize_environment_all()
    t_s, t_r = games.current_s.numpy().copy(), games.last_r.numpy().copy()
    o_s, o_r = EV.reset(SEED, N, 0)
    assert np.array_equal(t_s, o_s) and np.array_equal(_bits(t_r), _bits(o_r)), 'trajectory reset mismatch'
    t_act = np.random.RandomState(TRAJ_ACTION_SEED).choice(4, size=(T, N), p=[0.55, 0.15, 0.15, 0.15]).astype(np.uint8)
    lat0, acc0 = _pack(t_s)
    lats, accs, rbits, chs = [], [], [], []
    for t in range(T):
        ch = _ref_step_all(games, ctx, t_act[t], TRAJ_REPEATS, 1 + t)
        o_ch = EV.step(SEED, o_s, o_r, t_act[t], TRAJ_REPEATS, 1 + t)
        s_ref, r_ref = games.current_s.numpy().copy(), games.last_r.numpy().copy()
        assert np.array_equal(o_s, s_ref) and np.array_equal(_bits(o_r), _bits(r_ref)) and np.array_equal(o_ch, ch), f'trajectory step {t}: oracle mismatch'
        assert np.array_equal(EV.render(o_s, o_r, bank), games.current_frame_all().numpy()), f'trajectory frame {t}: oracle mismatch'
        lat, acc = _pack(s_ref)
        lats.append(lat); accs.append(acc); rbits.append(_bits(r_ref)); chs.append(ch)
    traj_finished = int(np.sum(chs))
    assert traj_finished >= 30, traj_finished
    out.update(traj_s0=lat0, traj_acc0=acc0, traj_r0_bits=_bits(t_r), traj_actions=t_act, traj_s=np.stack(lats), traj_acc=np.stack(accs),
               traj_r_bits=np.stack(rbits), traj_changed=np.stack(chs))

    # find_move for the three shapes
    with contextlib.redirect_stdout(io.StringIO()):
        games = Game(3)
    games.current_s[:, 1] = torch.tensor([0.0, 1.0, 2.0])
    rnd = [0.0, 0.4, 1.0]
    out['find_move'] = np.stack([games.find_move_all(x).numpy() for x in rnd]).astype(np.float32)       # [randomness, shape, 4]
    restore()

    word, cg, ck = find_largest_draw()
    reached = word == (1 << 24) - 1
    clamp_expected = EV.env_randint(SEED, cg, CLAMP_STAGE, ck)
    unclamped = int(np.float32(EV.env_u(SEED, cg, CLAMP_STAGE, ck)) * np.float32(EV.SIZES[ck]))
    assert unclamped == EV.SIZES[ck] and clamp_expected == EV.SIZES[ck] - 1 if reached else clamp_expected == unclamped
    meta = {'seed': SEED, 'stage': SWEEP_STAGE, 'repeats': list(SWEEP_REPEATS), 'finished': [finished[r] for r in SWEEP_REPEATS],
            'traj_repeats': TRAJ_REPEATS, 'traj_reset_stage': 0, 'traj_first_stage': 1, 'traj_action_seed': TRAJ_ACTION_SEED, 'traj_finished': traj_finished,
            'find_move_randomness': rnd,
            'clamp': {'stage': CLAMP_STAGE, 'game': cg, 'latent': ck, 'word': word, 'expected': int(clamp_expected), 'reached': bool(reached),
                      'note': 'word 2^24 - 1: u01 = 1.0, u * size = size, clamped to size - 1' if reached else 'the clamp was NOT reached within the search; largest word found'}}
    out['meta'] = np.array(json.dumps(meta, sort_keys=True))
    path = os.path.join(ROOT, 'tests', 'golden', 'env_sweep.npz')
    write_npz(path, out)
    print('env sweep written:', os.path.getsize(path), 'bytes; rounds finished', meta['finished'], 'trajectory', traj_finished, 'clamp', meta['clamp'])


def write_npz(path, arrays):
    """np.savez_compressed with a fixed member time stamp: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


if __name__ == '__main__':
    sweep() if '--sweep' in sys.argv[1:] else main()
