"""The agent of the reference's test_demo.py on the device, batched over games: observe a frame, choose an action sequence by one of the
paper's methods, execute it tick by tick in Dynamic-dSprites, drop the rest of the sequence when a reward is collected, start a new round
every `round_ticks` ticks and report the score every `report_ticks` ticks (test_demo.py:118-204).

The per-game control state (the action queue `executing_steps`, the reward crossings and the sum of the rewards received) lives in device
arrays behind `efe_agent` of the C ABI; `AgentState` binds its four kernels (csrc/agent.hip) and the two ends of an mcts decision
(csrc/agent_mcts.hip: the habit shortcut's draw, and the walk, trim and queueing of the planned path), and `AgentRunner` is the loop.  Only the games
whose queue is empty decide on a tick, as a compacted call whose noise follows the game (Rows: efe_encoder_rows / efe_rollout_rows).
`AgentTrace` is the record of a run (csrc/agent_trace.hip): what test_demo.py shows on every tick, kept in device arrays."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .model import Rows

MODES = {'ai': _lib.EFE_AGENT_AI, 't1': _lib.EFE_AGENT_T1, 't12': _lib.EFE_AGENT_T12, 'probs': _lib.EFE_AGENT_PROBS}
METHODS = ('habit', 'ai', 't1', 't12', 'mcts')
TAG_AGENT = 0x70


class AgentState:
    """Device arrays of `efe_agent` for E games: queue [E, cap] int32 with head [E] and len [E], crossings [E] int32, reward_sum [E] float32.
    The queue of game g is queue[g, head[g] : head[g] + len[g]]; head is 0 whenever len is 0."""

    def __init__(self, engine, games_no, cap):
        self._engine = engine
        self.E, self.cap = int(games_no), int(cap)
        dev = engine.device
        self.queue = torch.zeros(max(self.E, 0), max(self.cap, 0), dtype=torch.int32, device=dev)
        self.head = torch.zeros(max(self.E, 0), dtype=torch.int32, device=dev)
        self.len = torch.zeros(max(self.E, 0), dtype=torch.int32, device=dev)
        self.crossings = torch.zeros(max(self.E, 0), dtype=torch.int32, device=dev)
        self.reward_sum = torch.zeros(max(self.E, 0), dtype=torch.float32, device=dev)
        self.ids = torch.zeros(max(self.E, 1), dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._bind()

    def _bind(self):
        """(re)builds the efe_agent struct from the tensors this object holds"""
        self._struct = _lib.EfeAgent(self.queue.data_ptr(), self.head.data_ptr(), self.len.data_ptr(), self.crossings.data_ptr(),
                                     self.reward_sum.data_ptr(), self.E, self.cap)

    def _call(self, fn, *args):
        e = self._engine
        e.check(fn(e.ctx, C.byref(self._struct), *args, e.stream()))

    def clear(self):
        """empties every queue (test_demo.py:129); crossings and reward sums are kept"""
        self.len.zero_()
        self.head.zero_()

    def need(self):
        """-> (ids [E] int32, count [1] int32), both on the device: ids[:count] are the games whose queue is empty, ascending"""
        self._call(self._engine.lib.efe_agent_need, ptr(self.ids), ptr(self.count))
        return self.ids, self.count

    def choose(self, ids, mode, *, sum_G=None, sum_terms=None, probs=None, steps=1, temperature=1.0, repeat=1, seed=0, stage=0,
               game_offset=0, u=None, want_u=False):
        """efe_agent_choose for the deciding games `ids` (int32 device tensor [n]) -> choice [n] int32 (-1: the decision failed and the queue
        stays empty), or (choice, u) with want_u.  mode: 'ai' (sum_G [4n]), 't1' / 't12' (sum_terms [3, 4n]), 'probs' (probs [n, 4])."""
        if mode not in MODES:
            raise ValueError(f'unknown mode {mode!r}: one of {sorted(MODES)}')
        e = self._engine
        n = int(ids.numel())
        sum_G, sum_terms, probs = self._f32(sum_G, 4 * n, 'sum_G'), self._f32(sum_terms, 12 * n, 'sum_terms'), self._f32(probs, 4 * n, 'probs')
        u_t = self._f32(u, n, 'u')
        choice = torch.empty(n, dtype=torch.int32, device=e.device)
        u_out = torch.empty(n, dtype=torch.float32, device=e.device) if want_u else None
        if n == 0:                                                   # no game decides (empty tensors have no address to hand over)
            return (choice, u_out) if want_u else choice
        nz = _lib.EfeNoise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stage) & 0xFFFFFFFF, 0, 0, int(game_offset) & 0xFFFFFFFF)
        self._call(e.lib.efe_agent_choose, ptr(ids), n, MODES[mode], ptr(sum_G), ptr(sum_terms), ptr(probs), int(steps),
                   C.c_float(float(temperature)), int(repeat), C.byref(nz), ptr(u_t), ptr(choice), ptr(u_out))
        return (choice, u_out) if want_u else choice

    def _f32(self, t, numel, name):
        """an optional input as a contiguous float32 device tensor of `numel` elements"""
        if t is None:
            return None
        t = self._engine.tensor(t)
        if t.numel() != numel:
            raise ValueError(f'{name} has {t.numel()} elements, expected {numel}')
        return t

    def enqueue(self, ids, actions, lengths, jumps=1):
        """efe_agent_enqueue: the queue of game ids[i] becomes actions[i, :lengths[i]], each action `jumps` times"""
        e = self._engine
        n = int(ids.numel())
        if n == 0:                                                   # nothing to queue (the engine accepts n = 0 and launches nothing)
            return
        a = torch.as_tensor(actions).to(device=e.device, dtype=torch.int32).reshape(n, -1).contiguous()
        ln = torch.as_tensor(lengths).to(device=e.device, dtype=torch.int32).reshape(n).contiguous()
        self._call(e.lib.efe_agent_enqueue, ptr(ids), n, ptr(a), ptr(ln), int(a.shape[1]), int(jumps))

    def mcts_root(self, ids, Qpi, active, decided, *, use_habit, threshold, max_depth, jumps=1, seed=0, stage=0, game_offset=0, u=None,
                  want_u=False):
        """efe_agent_mcts_root: the beginning of an mcts decision for the deciding games `ids` (int32 device tensor [n]; slot i plans for game
        ids[i]).  Qpi [n, A] is the habit posterior of the root states; `active` and `decided` (uint8 device tensors, [>= n]) are written:
        the planner's liveness mask and what mcts_enqueue skips.  -> choice [n] int32: the habit shortcut's action (its queue is written,
        `jumps` times), -1 for a Qpi that is no distribution (empty queue, decided), -2 where the planner goes on; or (choice, u) with want_u.
        stage is the tick: the uniform has the key of choose()'s."""
        e = self._engine
        n = int(ids.numel())
        choice = torch.empty(n, dtype=torch.int32, device=e.device)
        u_out = torch.empty(n, dtype=torch.float32, device=e.device) if want_u else None
        if n == 0:
            return (choice, u_out) if want_u else choice
        Qpi = e.tensor(Qpi)
        if Qpi.dim() != 2 or Qpi.shape[0] != n:
            raise ValueError(f'Qpi has shape {tuple(Qpi.shape)}, expected ({n}, pi_dim)')
        for t, nm in ((active, 'active'), (decided, 'decided')):
            if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f'{nm}: a contiguous uint8 device tensor of at least {n} entries is required')
        u_t = self._f32(u, n, 'u')
        nz = _lib.EfeNoise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stage) & 0xFFFFFFFF, 0, 0, int(game_offset) & 0xFFFFFFFF)
        self._call(e.lib.efe_agent_mcts_root, ptr(ids), n, ptr(Qpi), int(Qpi.shape[1]), 1 if use_habit else 0, C.c_float(float(threshold)),
                   int(max_depth), int(jumps), C.byref(nz), ptr(u_t), ptr(active), ptr(decided), ptr(choice), ptr(u_out))
        return (choice, u_out) if want_u else choice

    def mcts_enqueue(self, ids, tree, decided, max_depth, jumps=1, want_path=False):
        """efe_agent_mcts_enqueue: for every slot i with decided[i] == 0 the queue of game ids[i] becomes the trimmed most-visited path of tree
        slot i (`tree`: an _lib.EfeMctsTree, e.g. BatchedMCTS.tree_of(n)), each action `jumps` times.  want_path -> (path [n, max_depth] int32,
        path_len [n] int32) on the device, pre-filled with -1 (decided slots and entries beyond the length are not written)."""
        e = self._engine
        n = int(ids.numel())
        path = torch.full((n, max(int(max_depth), 1)), -1, dtype=torch.int32, device=e.device) if want_path else None
        plen = torch.full((n,), -1, dtype=torch.int32, device=e.device) if want_path else None
        if n:
            self._call(e.lib.efe_agent_mcts_enqueue, C.byref(tree), ptr(ids), n, ptr(decided), int(max_depth), int(jumps), ptr(path), ptr(plen))
        return (path, plen) if want_path else None

    def act(self, games, stage, want_changed=False, changed_out=None):
        """efe_agent_act on `games` (a daimc_amd.Game of the same size): one tick for every game with a non-empty queue.  changed_out: a
        contiguous int32 device tensor [E] that receives round_changed (a row of AgentTrace.changed)"""
        e = self._engine
        if games.games_no != self.E:
            raise ValueError(f'the agent state holds {self.E} games, the environment {games.games_no}')
        changed = changed_out if changed_out is not None else torch.empty(self.E, dtype=torch.int32, device=e.device) if want_changed else None
        nz = _lib.EfeNoise(games.seed, int(stage) & 0xFFFFFFFF, 9, 0, games.game_offset)
        self._call(e.lib.efe_agent_act, ptr(games.current_s), ptr(games.last_r), C.byref(nz), ptr(changed))
        return changed.bool() if want_changed else None


class AgentTrace:
    """The record of an AgentRunner run in device arrays, T rows (ticks) x E games (efe_agent_trace of the C ABI, csrc/agent_trace.hip).
    Row t belongs to tick t of the runner.  FIELDS: name -> (shape behind [T, E], dtype, fill); the arrays are allocated pre-filled with
    "nothing happened" (NaN, -1 for action and choice, 0 for the rest), a kernel writes only what happened, and rows of games that did not
    decide on a tick keep the fill in the decision fields (decided .. path_len).

      state, last_r     the environment as the tick's decision sees it: after the round reset, before act
      action, queue_len the head of the queue just before act (-1: empty, the game does not move) and its length
      changed           efe_agent_act's round_changed of the tick
      decided           1 where the game decided on this tick
      choice, u         what efe_agent_choose / efe_agent_mcts_root returned (-1 a failed draw, -2 the planner goes on) and the uniform it
                        used; the slot planner's decisions leave both at the fill (no root draw on the device)
      G, terms          ai / t1 / t12: sum_G / steps and (-sum_terms[0], sum_terms[1], sum_terms[2]) / steps (test_demo.py:152-155)
      probs             the distribution the action was drawn from (habit and the keyed planner's root: Qpi), the bits the draw used
      path, path_len    mcts: the trimmed path the decision queued, before the jumps-fold repetition; path_len is the true length, also
                        above max_path.  A game the habit shortcut decided queued no planned path and keeps the fill

    frames = ids (the games to film), frame_every = k: `view` [T // k, len(ids), 64, 64] uint8, entry j the frame after the act of tick
    (j + 1) k - 1 with the demo's marker and, for mcts, the game's plan mask laid over it (efe_agent_view).  4 KB per game and frame: off by
    default."""
    FIELDS = {'state': ((7,), torch.float32, float('nan')), 'last_r': ((), torch.float32, float('nan')), 'action': ((), torch.int32, -1),
              'queue_len': ((), torch.int32, 0), 'changed': ((), torch.int32, 0), 'decided': ((), torch.uint8, 0), 'choice': ((), torch.int32, -1),
              'u': ((), torch.float32, float('nan')), 'G': ((4,), torch.float32, float('nan')), 'terms': ((3, 4), torch.float32, float('nan')),
              'probs': ((4,), torch.float32, float('nan')), 'path': (None, torch.int32, 0), 'path_len': ((), torch.int32, 0)}

    def __init__(self, max_path=16, frames=None, frame_every=1):
        self.max_path, self.frame_every = int(max_path), int(frame_every)
        if self.max_path < 1 or self.frame_every < 1:
            raise ValueError('max_path and frame_every must be >= 1')
        self.frame_games = None if frames is None else [int(i) for i in frames]
        if self.frame_games is not None and not self.frame_games:
            self.frame_games = None
        self.T, self.E, self._engine, self.view = 0, None, None, None

    _f32 = AgentState._f32

    def _shape(self, name, T):
        tail = self.FIELDS[name][0]
        return (T, self.E) + ((self.max_path,) if tail is None else tail)

    def bind(self, engine, games_no):
        """called by the runner: the record belongs to `games_no` games on the engine's device"""
        if self.E is not None and (self.E != int(games_no) or self._engine is not engine):
            raise ValueError('this AgentTrace already records another runner')
        self.E, self._engine = int(games_no), engine
        if self.frame_games is not None:
            if min(self.frame_games) < 0 or max(self.frame_games) >= self.E:
                raise ValueError(f'frames: game indices must lie in [0, {self.E})')
            self.frame_ids = torch.tensor(self.frame_games, dtype=torch.int32, device=engine.device)
        for name in self.FIELDS:
            setattr(self, name, torch.empty(self._shape(name, 0), dtype=self.FIELDS[name][1], device=engine.device))
        if self.frame_games is not None:
            self.view = torch.zeros(0, len(self.frame_games), 64, 64, dtype=torch.uint8, device=engine.device)

    def reserve(self, T):
        """room for at least T rows; the record grows on the device (the rows written so far are kept, the new ones hold the fill)"""
        T = int(T)
        if T <= self.T:
            return
        dev = self._engine.device
        for name, (_, dtype, fill) in self.FIELDS.items():
            more = torch.full(self._shape(name, T - self.T), fill, dtype=dtype, device=dev)
            setattr(self, name, torch.cat([getattr(self, name), more], 0))
        if self.view is not None:
            rows = T // self.frame_every - self.view.shape[0]
            self.view = torch.cat([self.view, torch.zeros(rows, len(self.frame_games), 64, 64, dtype=torch.uint8, device=dev)], 0)
        self.T = T
        self._struct = _lib.EfeAgentTrace(*[getattr(self, f).data_ptr() for f in _lib.TRACE_FIELDS], self.T, self.E, self.max_path)

    def record_tick(self, state, games, row):
        """efe_agent_trace_tick: state, last_r, action and queue_len of row `row` (after the decision, before act)"""
        e = self._engine
        e.check(e.lib.efe_agent_trace_tick(e.ctx, C.byref(state._struct), C.byref(self._struct), int(row), ptr(games.current_s),
                                           ptr(games.last_r), e.stream()))

    def record_decision(self, row, ids, mode=None, *, choice=None, u=None, sum_G=None, sum_terms=None, probs=None, steps=1, temperature=1.0,
                        path=None, path_len=None):
        """efe_agent_trace_decision for the deciding games `ids` (int32 device tensor [n]); mode: None (no distribution), 'ai', 't1', 't12'
        (sum_G [4n] and sum_terms [3, 4n]) or 'probs' (probs [n, 4]); path [n, L] with path_len [n] (int32 device tensors)"""
        e = self._engine
        n = int(ids.numel())
        if n == 0:
            return
        if mode is not None and mode not in MODES:
            raise ValueError(f'unknown mode {mode!r}: one of {sorted(MODES)}')
        f32 = self._f32
        sum_G, sum_terms, probs, u = f32(sum_G, 4 * n, 'sum_G'), f32(sum_terms, 12 * n, 'sum_terms'), f32(probs, 4 * n, 'probs'), f32(u, n, 'u')
        for t, nm in ((choice, 'choice'), (path, 'path'), (path_len, 'path_len')):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous()):
                raise ValueError(f'{nm}: a contiguous int32 device tensor is required')
        stride = int(path.shape[1]) if path is not None else 0
        e.check(e.lib.efe_agent_trace_decision(e.ctx, C.byref(self._struct), int(row), ptr(ids), n, _lib.EFE_AGENT_NONE if mode is None else MODES[mode],
                                               ptr(choice), ptr(u), ptr(sum_G), ptr(sum_terms), ptr(probs), int(steps),
                                               C.c_float(float(temperature)), ptr(path), ptr(path_len), stride, e.stream()))

    def numpy(self, ticks):
        """the first `ticks` rows as numpy arrays (one download per field)"""
        out = {name: getattr(self, name)[:ticks].cpu().numpy() for name in self.FIELDS}
        if self.view is not None:
            out['view'] = self.view[:ticks // self.frame_every].cpu().numpy()
            out['view_games'] = np.asarray(self.frame_games, dtype=np.int32)
        return out


def plan_mask(engine, ids, state, H_act, H_len, H_active, n_iter, jumps, mask, pi_dim=4):
    """efe_agent_plan_mask: make_mask of test_demo.py:87-113 for the deciding slots `ids` (int32 device tensor [n]) into mask [E, 32, 32] at
    the games' rows.  state [E, 7]; H_act [rows, slots, max_depth] int32, H_len [rows, slots] int32, H_active [rows, slots] uint8: the
    planner's history, of which the rows below n_iter count."""
    n = int(ids.numel())
    if n == 0:
        return
    for t, dt, nm in ((H_act, torch.int32, 'H_act'), (H_len, torch.int32, 'H_len'), (H_active, torch.uint8, 'H_active')):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f'{nm}: a contiguous {dt} device tensor is required')
    if H_act.dim() != 3 or H_len.shape != H_act.shape[:2] or H_active.shape != H_act.shape[:2] or int(n_iter) > H_act.shape[0]:
        raise ValueError('H_act [rows, slots, max_depth], H_len and H_active [rows, slots] with rows >= n_iter are required')
    if mask.dtype != torch.float32 or not mask.is_contiguous() or mask.dim() != 3 or tuple(mask.shape[1:]) != (32, 32):
        raise ValueError('mask: a contiguous float32 tensor [E, 32, 32] is required')
    if state.dtype != torch.float32 or not state.is_contiguous() or tuple(state.shape) != (mask.shape[0], 7):
        raise ValueError(f'state: a contiguous float32 tensor [{mask.shape[0]}, 7] is required')
    if ids.dtype != torch.int32 or not ids.is_contiguous() or n > H_act.shape[1]:
        raise ValueError('ids: a contiguous int32 tensor of at most as many entries as the history has slots is required')
    engine.check(engine.lib.efe_agent_plan_mask(engine.ctx, ptr(ids), n, int(mask.shape[0]), ptr(state), ptr(H_act), ptr(H_len), ptr(H_active),
                                                int(n_iter), int(H_act.shape[1]), int(H_act.shape[2]), int(jumps), int(pi_dim), ptr(mask),
                                                engine.stream()))


def agent_view(engine, frames, mask=None, ids=None):
    """efe_agent_view: frames [n, 1, 64, 64] float32 (efe_env_render) -> [n, 64, 64] uint8 with the demo's marker and, with mask [E, 32, 32]
    and ids (int32 device tensor [n]: the game of each frame), the games' plan masks laid over rows and columns 16..47; saturating"""
    n = int(frames.shape[0])
    view = torch.empty(n, 64, 64, dtype=torch.uint8, device=frames.device)
    view_into(engine, frames, mask, ids, view)
    return view


def view_into(engine, frames, mask, ids, view):
    """agent_view into `view`, a contiguous uint8 device tensor [n, 64, 64]"""
    n = int(frames.shape[0])
    if n == 0:
        return
    if frames.dtype != torch.float32 or not frames.is_contiguous() or frames.numel() != n * 4096:
        raise ValueError('frames: a contiguous float32 tensor [n, 1, 64, 64] is required')
    if view.dtype != torch.uint8 or not view.is_contiguous() or view.numel() != n * 4096:
        raise ValueError('view: a contiguous uint8 tensor [n, 64, 64] is required')
    if mask is not None:
        if mask.dtype != torch.float32 or not mask.is_contiguous() or mask.dim() != 3 or tuple(mask.shape[1:]) != (32, 32):
            raise ValueError('mask: a contiguous float32 tensor [E, 32, 32] is required')
        if ids is None or ids.dtype != torch.int32 or not ids.is_contiguous() or ids.numel() != n:
            raise ValueError('ids: with a mask, a contiguous int32 tensor of one game per frame is required')
    E = int(mask.shape[0]) if mask is not None else n
    engine.check(engine.lib.efe_agent_view(engine.ctx, ptr(frames), ptr(mask), ptr(ids), n, E, ptr(view), engine.stream()))


def default_samples(method):
    """test_demo.py:70-77"""
    return 10 if method in ('t1', 't12', 'ai', 'habit') else 1


class AgentRunner:
    """test_demo.py's loop for every game of `games` at once.

    Start (test_demo.py:51-52): randomize_environment_all, then the score column is set to 0.  Tick t, in the order of :118-204:
      1. t % report_ticks == 0 and t > 0: every game's s[6] is recorded as a round score and set to 0
      2. t % round_ticks == 0: randomize_environment_all with the score column put back, all queues cleared
      3. efe_agent_need; the decision for the deciding games only; efe_agent_act
    Decisions (the deciding games' frames are rendered from their gathered state rows):
      habit          : encoder(rows=ids) -> encode_s -> choose('probs'), the action `steps` times
      ai / t1 / t12  : batched calculate_G_4_repeated(rows=ids, steps, samples, calc_mean) -> choose, the action steps * jumps times
      mcts           : active_inference_mcts_batch on the deciding frames -> enqueue(path, jumps); with keyed_planner = True one id-keyed
                       planner for all the games (BatchedMCTS(keyed=True)): root encoder(rows=ids) -> encode_s -> mcts_root (the habit
                       shortcut's draw, on the device) -> the planner's iterations -> mcts_enqueue (walk, trim and queue, on the device)

    Noise: every draw's stage is a function of the tick alone and its row a function of the game's global index g = games.game_offset + e:
      environment    : seed games.seed; start = stage 0, the reset of tick t = stage 1 + 2 t, its act = stage 2 + 2 t; row g
      model          : seed model.seed; the decision of tick t starts at stage t * steps (a rollout takes `steps` stages); rows 4 g .. 4 g + 3
                       for the rollouts, row g for the habit encoder
      action uniform : seed model.seed, tag 0x70, stage t, row g
      keyed planner  : seed model.seed; the decision of tick t starts at stage t * P, P = 2 + repeats * (1 + simulation_repeats): root encoder
                       t P, root expansion t P + 1, expansion of iteration r  t P + 2 + r (1 + simulation_repeats), its simulation k that
                       + 1 + k; row g for the encoder and the simulations, rows A g .. A g + A - 1 for the expansions; the habit shortcut's
                       action uniform is the one above (tag 0x70, stage t, row g)
    (all modulo 2^32).  The trajectory of a game is therefore the same whether it runs alone (game_offset = g) or inside any batch -- for
    habit, ai, t1 and t12, and for mcts with keyed_planner = True.  NOT for mcts with the default slot planner (keyed_planner = False, kept
    as the default for now; the keyed planner is meant to replace it): that planner keys an episode by its slot among the deciding games and
    takes its stages from the model's own counter, so the trajectory depends on which other games decide on the same tick, and its habit
    shortcut draws from the host's global generator.

    Host traffic per tick: one 4-byte read-back (the number of deciding games), plus the render validity flag on ticks where a game decides
    (mcts: plus the planner's own read-backs -- keyed: only its lagged stop snapshot, one pinned copy per iteration that the host reads two
    iterations later).  run() fetches everything else once at its end.

    trace = True (or an AgentTrace): the run is recorded on the device -- per tick and game the state, the executed action, and per
    decision the choice, its uniform, G and its terms, the distribution it was drawn from and the planned path; for mcts `plan_mask`
    [E, 32, 32] holds the heat mask of every path each game's most recent planning decision explored (zeros before the first).  Recording
    adds launches, no host traffic per tick, and leaves every trajectory as it is; run() then adds 'trace' to its result."""

    def __init__(self, model, games, method, *, steps=7, jumps=5, temperature=1.0, samples=None, calc_mean=False, mcts_params=None,
                 round_ticks=100, report_ticks=1000, keyed_planner=False, trace=None):
        if method not in METHODS:
            raise ValueError(f'unknown method {method!r}: one of {METHODS}')
        self.model, self.games, self.method = model, games, method
        self.steps, self.jumps, self.temperature = int(steps), int(jumps), float(temperature)
        self.samples = default_samples(method) if samples is None else int(samples)
        self.calc_mean, self.round_ticks, self.report_ticks = bool(calc_mean), int(round_ticks), int(report_ticks)
        if self.steps < 1 or self.jumps < 1 or self.round_ticks < 1 or self.report_ticks < 1:
            raise ValueError('steps, jumps, round_ticks and report_ticks must be >= 1')
        if games.device != model.device:
            raise ValueError('the games and the model must live on the same device')
        cap = self.steps * self.jumps
        if method == 'mcts':
            from .mcts import MCTS_Params
            self.mcts_params = mcts_params if mcts_params is not None else MCTS_Params()
            cap = max(cap, (self.mcts_params.repeats + 2) * self.jumps)
        self.keyed_planner = bool(keyed_planner) and method == 'mcts'      # (the other methods key every draw by the game as they are)
        self.state = AgentState(model._ready(), games.games_no, cap)
        # the record of the run (AgentTrace): off by default, and then a tick launches what it always launched
        self.trace = AgentTrace() if trace is True else trace if trace else None
        self.plan_mask = None
        if self.trace is not None:
            if not isinstance(self.trace, AgentTrace):
                raise TypeError('trace: True or an AgentTrace')
            self.trace.bind(model._ready(), games.games_no)
            if method == 'mcts':
                if model.pi_dim != 4:
                    raise ValueError('the plan mask of a traced mcts run is defined for pi_dim 4 only')
                self.plan_mask = torch.zeros(games.games_no, 32, 32, dtype=torch.float32, device=model.device)
        if self.keyed_planner:
            from .mcts import BatchedMCTS
            # ONE planner for all the games, reused by every decision; the decision of tick t starts at stage t * P.  A traced run keeps
            # the whole history of a decision (the plan mask is taken from it), an untraced one the two-row ring
            self.planner = BatchedMCTS(model, games.games_no, self.mcts_params, keyed=True, history=self.trace is not None)
            self.stages_per_decision = BatchedMCTS.stages_per_decision(self.mcts_params)
        self.t = 0
        self.decisions = 0
        self.scores = []
        self._failed = torch.zeros(1, dtype=torch.int32, device=model.device)

    # ---- one tick ----------------------------------------------------------------------------------------------------------------------
    def _frames(self, ids):
        """[n,1,64,64] frames of the games `ids` (s_to_o on their gathered state rows)"""
        g, e = self.games, self.model._ready()
        n = int(ids.numel())
        s = g.current_s.index_select(0, ids).contiguous()
        r = g.last_r.index_select(0, ids).contiguous()
        frames = torch.empty(n, 1, 64, 64, device=g.device)
        err = torch.empty(n, dtype=torch.int32, device=g.device)
        e.check(e.lib.efe_env_render(e.ctx, ptr(s), ptr(r), ptr(g.imgs), g.imgs.shape[0], ptr(frames), ptr(err), n, e.stream()))
        if bool(err.any()):
            raise ValueError(f'Error: Reward: {r[err.bool()][0].item()}')              # game_environment.py:53
        return frames

    def _decide(self, ids, t):
        m, g, st, tr = self.model, self.games, self.state, self.trace
        n, E = int(ids.numel()), g.games_no
        frames = self._frames(ids)
        stage = (t * self.steps) & 0xFFFFFFFF
        key = dict(seed=m.seed, stage=t, game_offset=g.game_offset)
        u = None                                                     # (a traced decision also asks for the uniform: one more output, the same draw)
        if self.method == 'habit':
            mean, _ = m.model_down.encoder(frames, stage=stage, row_offset=g.game_offset & 0xFFFFFFFF, rows=Rows(ids=ids, rows_per_entry=1, n_total=E))
            _, Qpi, _ = m.model_top.encode_s(mean)
            choice = st.choose(ids, 'probs', probs=Qpi, steps=self.steps, temperature=self.temperature, repeat=self.steps, want_u=tr is not None, **key)
            if tr is not None:
                choice, u = choice
                tr.record_decision(t, ids, 'probs', choice=choice, u=u, probs=Qpi)
        elif self.keyed_planner:
            pl, p = self.planner, self.planner.p
            Qpi = pl.begin_keyed(frames, ids, g.game_offset, (t * self.stages_per_decision) & 0xFFFFFFFF, o_shape=(1, 64, 64))
            choice = st.mcts_root(ids, Qpi, pl.active, pl.decided, use_habit=p.use_habit, threshold=p.threshold, max_depth=pl.max_depth,
                                  jumps=self.jumps, want_u=tr is not None, **key)
            n_iter = pl.plan_keyed()
            if tr is not None:
                choice, u = choice
                path, plen = st.mcts_enqueue(ids, pl.tree_of(n), pl.decided, pl.max_depth, self.jumps, want_path=True)
                plan_mask(m._ready(), ids, g.current_s, pl.H_act, pl.H_len, pl.H_active, n_iter, self.jumps, self.plan_mask)
                tr.record_decision(t, ids, 'probs', choice=choice, u=u, probs=Qpi, path=path, path_len=plen)
            else:
                st.mcts_enqueue(ids, pl.tree_of(n), pl.decided, pl.max_depth, self.jumps)
            self._failed += (choice == -1).any().to(torch.int32)
            return
        elif self.method == 'mcts':
            from .mcts import active_inference_mcts_batch
            hook = None
            if tr is not None:                                       # the mask from the planner's device history, before it is read back
                hook = lambda pl, n_iter: plan_mask(m._ready(), ids, g.current_s, pl.H_act, pl.H_len, pl.H_active, n_iter, self.jumps, self.plan_mask)
            out, _ = active_inference_mcts_batch(m, frames, self.mcts_params, o_shape=(1, 64, 64), episode_offset=g.game_offset, history_hook=hook)
            paths = [list(o[0]) for o in out]
            L = max(1, max(len(p) for p in paths))
            acts = np.zeros((n, L), dtype=np.int32)
            for i, p in enumerate(paths):
                acts[i, :len(p)] = p
            lens = np.array([len(p) for p in paths], dtype=np.int32)
            if tr is not None:
                acts, lens = torch.from_numpy(acts).to(g.device), torch.from_numpy(lens).to(g.device)
                tr.record_decision(t, ids, None, path=acts, path_len=lens)
            st.enqueue(ids, acts, lens, self.jumps)
            return
        else:
            sum_G, sum_terms, _ = m.calculate_G_4_repeated(frames.repeat_interleave(4, dim=0), steps=self.steps, calc_mean=self.calc_mean,
                                                           samples=self.samples, stage=stage, row_offset=(4 * g.game_offset) & 0xFFFFFFFF,
                                                           rows=Rows(ids=ids, rows_per_entry=4, n_total=E))
            sum_terms = torch.stack(sum_terms)
            choice = st.choose(ids, self.method, sum_G=sum_G, sum_terms=sum_terms, steps=self.steps,
                               temperature=self.temperature, repeat=self.steps * self.jumps, want_u=tr is not None, **key)
            if tr is not None:
                choice, u = choice
                tr.record_decision(t, ids, self.method, choice=choice, u=u, sum_G=sum_G, sum_terms=sum_terms, steps=self.steps,
                                   temperature=self.temperature)
        self._failed += (choice < 0).any().to(torch.int32)

    def tick(self):
        g, st, t, tr = self.games, self.state, self.t, self.trace
        if tr is not None and t >= tr.T:                             # a bare tick beyond the rows run() sized: the record doubles on the device
            tr.reserve(max(t + 1, 2 * tr.T))
        if t == 0:                                                   # test_demo.py:51-52
            g.randomize_environment_all(stage=0)
            g.current_s[:, 6] = 0.0
        if t % self.report_ticks == 0 and t > 0:                     # :121-124
            self.scores.append(g.current_s[:, 6].clone())
            g.current_s[:, 6] = 0.0
        if t % self.round_ticks == 0:                                # :125-129
            score = g.current_s[:, 6].clone()
            g.randomize_environment_all(stage=(1 + 2 * t) & 0xFFFFFFFF)
            g.current_s[:, 6] = score
            st.clear()
        ids, count = st.need()
        n = int(count.item())                                        # the tick's one read-back
        if n:
            self.decisions += n
            self._decide(ids[:n], t)
        if tr is None:
            st.act(g, stage=(2 + 2 * t) & 0xFFFFFFFF)
        else:
            tr.record_tick(st, g, t)
            st.act(g, stage=(2 + 2 * t) & 0xFFFFFFFF, changed_out=tr.changed[t])
            if tr.view is not None and (t + 1) % tr.frame_every == 0:
                self._film((t + 1) // tr.frame_every - 1)
        self.t = t + 1

    def _film(self, j):
        """entry j of the record's `view`: the filmed games' frames as they stand (after act), marker and plan mask laid over them"""
        g, e, tr = self.games, self.model._ready(), self.trace
        ids = tr.frame_ids
        n = int(ids.numel())
        s = g.current_s.index_select(0, ids).contiguous()
        r = g.last_r.index_select(0, ids).contiguous()
        frames = torch.empty(n, 1, 64, 64, device=g.device)
        # (no validity flag: reading it would be a host round trip per frame; the tick's decision checks the rewards it renders)
        e.check(e.lib.efe_env_render(e.ctx, ptr(s), ptr(r), ptr(g.imgs), g.imgs.shape[0], ptr(frames), None, n, e.stream()))
        view_into(e, frames, self.plan_mask, ids if self.plan_mask is not None else None, tr.view[j])

    def run(self, ticks, fetch_trace=True):
        """`ticks` more ticks -> dict: round_scores [reports so far, E], crossings [E], reward_sum [E], state [E, 7], last_r [E] (numpy,
        fetched once here), ticks, decisions (game decisions made) and failed_ticks (ticks in which a decision failed); a traced runner adds
        'trace': the record's fields as numpy arrays cut to the ticks run so far (AgentTrace.numpy; fetch_trace = False leaves it on the device)"""
        if self.trace is not None:
            self.trace.reserve(self.t + int(ticks))                  # the rows of the ticks about to run
        for _ in range(int(ticks)):
            self.tick()
        g, st = self.games, self.state
        scores = torch.stack(self.scores).cpu().numpy() if self.scores else np.zeros((0, g.games_no), dtype=np.float32)
        res = {'round_scores': scores, 'crossings': st.crossings.cpu().numpy(), 'reward_sum': st.reward_sum.cpu().numpy(),
               'state': g.current_s.cpu().numpy(), 'last_r': g.last_r.cpu().numpy(), 'ticks': self.t, 'decisions': self.decisions,
               'failed_ticks': int(self._failed.item())}
        if self.trace is not None and fetch_trace:
            res['trace'] = self.trace.numpy(self.t)
        return res


def run_agent(model, games, method, ticks, **kw):
    """AgentRunner(model, games, method, **kw).run(ticks)"""
    return AgentRunner(model, games, method, **kw).run(ticks)
