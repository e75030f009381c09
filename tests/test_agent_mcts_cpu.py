"""CPU side of the keyed mcts decision: the numpy restatement that csrc/agent_mcts.hip is tested against (tests/agent_mcts_ref.py) reproduces
`Node.action_selection` of daimc_amd.mcts.Node on random trees, trimming included, and the stage layout of a keyed decision --
P = 2 + repeats * (1 + simulation_repeats) stages from stage0 -- is what the slot planner takes from the model's counter, counted with a
stub model."""
import types

import numpy as np
import pytest
import torch

import agent_mcts_ref as MR


def node_tree(N, child, A):
    """daimc_amd.mcts.Node objects for a [cap][A] array tree"""
    from daimc_amd.mcts import Node
    nodes = {}

    def build(i):
        nd = nodes[i] = Node(torch.zeros(10), None, 1.0, A)
        nd.N = torch.from_numpy(N[i].copy())
        if child[i, 0] >= 0:
            nd.children_nodes = [build(int(c)) for c in child[i]]
        return nd
    return build(0)


@pytest.mark.parametrize('A', [4, 3])
def test_restatement_reproduces_node_action_selection(A):
    from daimc_amd.mcts import _trim_path
    rng = np.random.default_rng(5 + A)
    seen = set()
    for case in range(300):
        cap = 1 + A * 42
        if case % 3 == 0:        # a chain: long paths, many cancelling pairs
            N, child = MR.chain_tree(rng.integers(0, A, size=int(rng.integers(1, 40))).tolist(), cap, A, rng)
        else:
            N, child = MR.random_tree(rng, cap, A, int(rng.integers(0, 40)), ties=case % 3 == 1)
        want = node_tree(N, child, A).action_selection(deterministic=True)
        visited = MR.walk(N[None], child[None], 0)
        assert _trim_path(visited, A) == want, case
        q, h, ln, paths = MR.enqueue(N[None], child[None], [0], [0], np.full((1, 3 * 42), -5, np.int32), np.ones(1, np.int32), np.ones(1, np.int32), 3)
        assert paths[0] == want and h[0] == 0 and ln[0] == 3 * len(want), case
        assert q[0, :ln[0]].tolist() == [a for a in want for _ in range(3)] and (q[0, ln[0]:] == -5).all(), case
        seen.add((len(visited) > 1, len(want) == 0, len(want) < len(visited) - 1))
    # the cases cover: one-action walks, paths that trim to nothing, paths that lose a pair in the middle, and plain ones
    assert {(False, True, False), (True, True, True), (True, False, True), (True, False, False)} <= seen, seen


class StubModel:
    """counts the stages a planner takes from the model's counter; every network call returns zeros"""
    pi_dim, s_dim, colour_channels, resolution = 4, 10, 1, 64
    device = 'cpu'

    def __init__(self, stage0, habit_q):
        self._stage, self.log, self.habit_q = stage0, [], habit_q
        self.pi_one_hot = torch.eye(4)
        self.model_down = types.SimpleNamespace(encoder=self._encoder)
        self.model_top = types.SimpleNamespace(encode_s=self._encode_s)
        self._engine = types.SimpleNamespace(lib=None)

    def _take_stage(self, stage, n=1):
        assert stage is None
        stage, self._stage = self._stage, self._stage + n
        return stage

    def _encoder(self, o, **kw):
        self.log.append(('encoder', self._take_stage(kw.get('stage'))))
        return torch.zeros(o.shape[0], 10), None

    def _encode_s(self, s):
        return None, self.habit_q.repeat(s.shape[0], 1), None

    def calculate_G_mean(self, s, pi, **kw):
        self.log.append(('expand', self._take_stage(kw.get('stage'))))
        return torch.arange(4, dtype=torch.float32), None, torch.zeros(4, 10), None

    def mcts_step_simulate(self, s, depth, use_means=False, **kw):
        self.log.append(('simulate', self._take_stage(kw.get('stage'))))
        return 0.0, None, torch.full((4,), 0.25)


@pytest.mark.parametrize('repeats,sim_repeats', [(4, 1), (7, 3)])
def test_stage_layout_is_what_the_slot_planner_takes_from_the_counter(repeats, sim_repeats):
    import daimc_amd
    from daimc_amd.mcts import BatchedMCTS, _mcts_one
    p = daimc_amd.MCTS_Params()
    p.repeats, p.simulation_repeats, p.threshold = repeats, sim_repeats, 2.0      # (the early stop out of reach: every iteration runs)
    P = BatchedMCTS.stages_per_decision(p)
    assert P == 2 + repeats * (1 + sim_repeats)
    stage0 = 1000
    # the order of the draws, from the host tree (which takes a stage where it draws)
    m = StubModel(stage0, torch.full((4,), 0.25))
    _mcts_one(m, torch.zeros(1, 64, 64), p, (1, 64, 64))
    want = [('encoder', stage0), ('expand', stage0 + 1)]
    for r in range(repeats):
        e = stage0 + 2 + r * (1 + sim_repeats)
        want += [('expand', e)] + [('simulate', e + 1 + k) for k in range(sim_repeats)]
    assert m.log == want and m._stage == stage0 + P
    # the lock-step slot planner reserves the same P stages in the same order: the encoder's, the root expansion's, then repeats * (1 +
    # simulation_repeats) for the loop -- also when the habit shortcut decides every episode and nothing is planned
    p.use_habit, p.threshold = True, 0.5
    m = StubModel(stage0, torch.tensor([1.0, 0.0, 0.0, 0.0]))
    taken = []
    take = m._take_stage
    m._take_stage = lambda stage, n=1: (taken.append((m._stage, n)), take(stage, n))[1]
    stub = types.SimpleNamespace(model=m, E=3, p=p, pi_dim=4, _p=None, ep0=0, S=torch.zeros(3, 5, 10), Qpi=torch.zeros(3, 5, 4))
    res = BatchedMCTS._run(stub, torch.zeros(3, 1, 64, 64), (1, 64, 64))
    assert taken == [(stage0, 1), (stage0 + 1, 1), (stage0 + 2, repeats * (1 + sim_repeats))] and m._stage == stage0 + P
    assert all(r[0] == [0] and r[1] == 0 for r in res)
