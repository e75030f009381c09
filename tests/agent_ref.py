"""CPU restatement (numpy fp32, per-game loops) of the agent loop of the reference's test_demo.py:118-204 over oracle.env_oracle, batched
over games -- the authority for the arithmetic of csrc/agent.hip.  Test infrastructure only.

  probabilities(mode, ...) : test_demo.py:152-159 in float32 -- x / steps, exp(x / T) / sum, no max-subtraction
  draw(p, u)               : np.random.choice(4, p=p) given the uniform it consumed -- cdf = cumsum(p) / cumsum(p)[-1], the first edge above u;
                             -1 where numpy refuses p (a NaN or a negative entry; an infinite entry always comes with a NaN)
  AgentRef                 : start, the tick (report, round reset, decide, act) and the bookkeeping of efe_agent

Stages (one per tick, as daimc_amd.agent.AgentRunner): start = 0, the reset of tick t = 1 + 2 t, its act = 2 + 2 t."""
import json

import numpy as np

from oracle import env_oracle as EV
from oracle import philox as PX

TAG_AGENT = 0x70
MODES = ('ai', 't1', 't12', 'probs')
F = np.float32


def action_uniform(seed, game, stage):
    """the uniform of efe_agent_choose: word 0 of the counter (tag 0x70, global game, stream 0, stage); `game` may be an array"""
    k0, k1 = PX._key(seed)
    g = np.asarray(game, dtype=np.uint64) & PX.MASK32
    x0 = PX.philox4x32_10(np.uint64(TAG_AGENT) << np.uint64(16), g, np.uint64(0), np.uint64(PX.u32(stage)), k0, k1)[0]
    return PX._u01(np.asarray(x0, dtype=np.uint32))


def probabilities(mode, sum_G=None, sum_terms=None, steps=1, temperature=1.0, probs=None):
    """float32 [4]; test_demo.py:152-159 (82-84: softmax without max-subtraction)"""
    if mode == 'probs':
        return np.asarray(probs, dtype=F)
    fs, T = F(steps), F(temperature)
    with np.errstate(all='ignore'):
        if mode == 'ai':
            x = -(np.asarray(sum_G, dtype=F) / fs)
        elif mode == 't1':
            x = np.asarray(sum_terms, dtype=F)[0] / fs
        elif mode == 't12':
            st = np.asarray(sum_terms, dtype=F)
            x = st[0] / fs - st[1] / fs
        else:
            raise ValueError(mode)
        e = np.exp(x / T).astype(F)
        tot = F(0)
        for k in range(4):
            tot = e[k] if k == 0 else F(tot + e[k])
        return (e / tot).astype(F)


def draw(p, u):
    """np.random.choice's rule in float32; u == 1.0 (which the engine's 24-bit uniform can round to): the last action with p > 0"""
    p = np.asarray(p, dtype=F)
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        return -1
    cdf = np.zeros(4, dtype=F)
    acc = F(0)
    for k in range(4):
        acc = p[k] if k == 0 else F(acc + p[k])
        cdf[k] = acc
    with np.errstate(all='ignore'):
        cdf = (cdf / cdf[3]).astype(F)
    for k in range(4):
        if cdf[k] > F(u):
            return k
    pos = np.flatnonzero(p > 0)
    return int(pos[-1]) if len(pos) else -1


class AgentRef:
    def __init__(self, seed, games_no, *, steps=7, jumps=5, temperature=1.0, round_ticks=100, report_ticks=1000, game_offset=0):
        self.seed, self.E, self.go = int(seed), int(games_no), int(game_offset)
        self.steps, self.jumps, self.temperature = int(steps), int(jumps), float(temperature)
        self.round_ticks, self.report_ticks = int(round_ticks), int(report_ticks)
        self.queues = [[] for _ in range(self.E)]
        self.crossings = np.zeros(self.E, dtype=np.int32)
        self.reward_sum = np.zeros(self.E, dtype=F)
        self.scores = []
        self.s, self.last_r = EV.reset(self.seed, self.E, 0, self.go)      # test_demo.py:51-52
        self.s[:, 6] = 0.0

    def tick(self, t, decide):
        """decide(t, g) -> (mode, kwargs of probabilities(), u) for a game whose queue is empty, or a list of actions (a planner's path).
        -> {game: choice} of this tick's decisions (paths: None)"""
        if t % self.report_ticks == 0 and t > 0:
            self.scores.append(self.s[:, 6].copy())
            self.s[:, 6] = 0.0
        if t % self.round_ticks == 0:
            score = self.s[:, 6].copy()
            self.s, self.last_r = EV.reset(self.seed, self.E, 1 + 2 * t, self.go)
            self.s[:, 6] = score
            self.queues = [[] for _ in range(self.E)]
        chosen = {}
        for g in range(self.E):
            q = self.queues[g]
            if len(q) == 0:
                d = decide(t, g)
                if isinstance(d, (list, np.ndarray)):
                    q = [int(a) for a in d for _ in range(self.jumps)]
                    chosen[g] = None
                else:
                    mode, kw, u = d
                    c = draw(probabilities(mode, steps=self.steps, temperature=self.temperature, **kw), u)
                    chosen[g] = c
                    q = [] if c < 0 else [c] * (self.steps if mode == 'probs' else self.steps * self.jumps)
            if len(q) > 0:
                changed = EV.step(self.seed, self.s[g:g + 1], self.last_r[g:g + 1], [q[0]], 1, 2 + 2 * t, self.go + g)[0]
                if changed:
                    self.crossings[g] += 1
                    self.reward_sum[g] = F(self.reward_sum[g] + self.last_r[g])
                    q = []
                else:
                    q = q[1:]
            self.queues[g] = q
        return chosen

    def queue_len(self):
        return np.array([len(q) for q in self.queues], dtype=np.int32)

    def queue_action(self):
        """the action a queue repeats (every queue of the draw methods holds one action), 255 for an empty one"""
        return np.array([q[0] if q else 255 for q in self.queues], dtype=np.uint8)


# ---- the fixture tests/golden/agent_loop.npz (tools/make_golden_agent.py) ----
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Trajectory:
    """one trajectory of the fixture: its settings, the recorded arrays and the decision tables by (tick, game)"""

    def __init__(self, g, name):
        meta = json.loads(str(g['meta']))
        self.env_seed, self.E = int(meta['env_seed']), int(meta['games'])
        self.cfg = meta['trajectories'][name]
        self.a = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + '_')}
        self.index = {(int(t), int(gm)): i for i, (t, gm) in enumerate(zip(self.a['dec_tick'], self.a['dec_game']))}
        self.u = self.a['dec_u'].view(np.float64)
        self.sum_G = self.a['dec_sum_G'].view(np.float32)
        self.sum_terms = self.a['dec_sum_terms'].view(np.float32)

    def mode(self, t):
        return self.cfg['modes'][t % len(self.cfg['modes'])]

    def uniform(self, i):
        return 0.5 if np.isnan(self.u[i]) else float(self.u[i])       # a refused draw consumed no uniform: any value does

    def ref(self):
        c = self.cfg
        return AgentRef(self.env_seed, self.E, steps=c['steps'], jumps=c['jumps'], temperature=c['temperature'],
                           round_ticks=c['round_ticks'], report_ticks=c['report_ticks'])

    def decide(self, t, g):
        i = self.index[(t, g)]
        return self.mode(t), dict(sum_G=self.sum_G[i], sum_terms=self.sum_terms[i]), self.uniform(i)
