"""The agent loop's CPU restatement (tests/agent_ref.py) against the fixture captured from the reference's Game driven by test_demo.py's
loop body (tests/golden/agent_loop.npz, tools/make_golden_agent.py), and the rules of the loop that the device kernels must keep: a
crossing empties the queue, a failed decision leaves the game un-ticked, a round reset keeps the score."""
import numpy as np
import pytest

from conftest import load_golden
import agent_ref as AR
from agent_ref import Trajectory, bits


@pytest.fixture(scope='module')
def fixture():
    return load_golden('agent_loop')


@pytest.mark.parametrize('name', ['A', 'B'])
def test_agent_ref_equals_the_reference_trajectory(fixture, name):
    tr = Trajectory(fixture, name)
    ref, a = tr.ref(), tr.a
    used = 0
    for t in range(tr.cfg['ticks']):
        chosen = ref.tick(t, tr.decide)
        for g, c in chosen.items():
            assert c == a['dec_choice'][tr.index[(t, g)]], (t, g)
        used += len(chosen)
        assert np.array_equal(ref.s[:, :6], a['lat'][t].astype(np.float32)) and np.array_equal(bits(ref.s[:, 6]), a['acc'][t]), t
        assert np.array_equal(bits(ref.last_r), a['r'][t]), t
        assert np.array_equal(ref.queue_len(), a['qlen'][t]) and np.array_equal(ref.queue_action(), a['qact'][t]), t
        assert np.array_equal(ref.crossings, a['cross'][t]) and np.array_equal(bits(ref.reward_sum), a['rsum'][t]), t
    assert used == len(a['dec_tick']) == tr.cfg['decisions']
    scores = bits(np.stack(ref.scores)) if ref.scores else np.zeros((0, tr.E), np.uint32)
    assert np.array_equal(scores, a['scores'])
    assert len(a['scores']) == (tr.cfg['ticks'] - 1) // tr.cfg['report_ticks']


def test_fixture_covers_the_cases(fixture):
    """failed decisions (overflow and 0 / 0), every action, crossings, and the 1e-4 margin of every recorded draw"""
    for name in ('A', 'B'):
        tr = Trajectory(fixture, name)
        ch = tr.a['dec_choice']
        assert (ch < 0).sum() >= 10 and all((ch == k).any() for k in range(4)) and tr.a['cross'][-1].sum() >= 10
        kinds = set()
        for i, c in enumerate(ch):
            p = AR.probabilities(tr.mode(int(tr.a['dec_tick'][i])), sum_G=tr.sum_G[i], sum_terms=tr.sum_terms[i], steps=tr.cfg['steps'],
                                 temperature=tr.cfg['temperature'])
            if c < 0:
                assert np.isnan(p).any() and np.isnan(tr.u[i])
                kinds.add('all-nan' if np.isnan(p).all() else 'some-nan')
            else:
                cdf = np.cumsum(p.astype(np.float64)); cdf /= cdf[-1]
                assert np.abs(cdf - tr.u[i]).min() >= 1e-4, (name, i)
                if (p == 0).any():
                    kinds.add('p=0')
        assert kinds == {'all-nan', 'some-nan', 'p=0'}, kinds


def test_queue_is_empty_after_a_crossing(fixture):
    tr = Trajectory(fixture, 'A')
    a = tr.a
    crossed = np.diff(a['cross'].astype(np.int64), axis=0) > 0                  # [T-1, E]: a crossing in tick t + 1
    assert crossed.sum() >= 10
    assert (a['qlen'][1:][crossed] == 0).all() and (a['qact'][1:][crossed] == 255).all()
    assert (a['acc'][1:][crossed] == 0).all()                                     # new_image restarts the score column (the port's quirk)
    # ... and the reward went to the sum: the difference of the sums is the reward bar right after the crossing
    rs, r = a['rsum'].view(np.float32), a['r'].view(np.float32)
    t, g = np.nonzero(crossed)
    assert np.array_equal(bits(rs[t, g] + r[t + 1, g]), bits(rs[t + 1, g]))


def test_failed_decision_leaves_last_r_unticked():
    ref = AR.AgentRef(5, 3, steps=2, jumps=2, round_ticks=1000)
    ref.tick(0, lambda t, g: ('ai', dict(sum_G=np.zeros(4, np.float32)), 0.9))  # uniform p, u = 0.9 -> action 3 for four ticks
    s0, r0 = ref.s.copy(), ref.last_r.copy()
    ref.queues[1] = []
    overflow = np.full(4, -1e4, np.float32)                                      # exp(5000) = inf for every action: inf / inf

    def decide(t, g):
        assert g == 1
        return 'ai', dict(sum_G=overflow), 0.5
    chosen = ref.tick(1, decide)
    assert chosen == {1: -1} and ref.queues[1] == []
    assert np.array_equal(ref.s[1], s0[1]) and ref.last_r[1] == r0[1]            # no move, no tick
    assert np.array_equal(bits(ref.last_r[[0, 2]]), bits(r0[[0, 2]] * np.float32(0.95)))
    assert AR.draw(AR.probabilities('ai', sum_G=np.full(4, 1e4, np.float32)), 0.5) == -1      # 0 / 0


def test_round_reset_keeps_the_score_and_clears_the_queues():
    ref = AR.AgentRef(9, 4, steps=3, jumps=2, round_ticks=5, report_ticks=7)
    up = lambda t, g: ('probs', dict(probs=np.array([1, 0, 0, 0], np.float32)), 0.25)
    for t in range(5):
        ref.tick(t, up)
    ref.s[:, 6] = np.array([1.5, -2.25, 0.0, 3.0], np.float32)
    before, crossed_before = ref.s.copy(), ref.crossings.copy()
    ref.queues = [[0, 0], [0], [0, 0, 0], []]
    decided = ref.tick(5, up)
    assert sorted(decided) == [0, 1, 2, 3]                                       # every queue was cleared, so every game decided
    assert not np.array_equal(ref.s[:, :6], before[:, :6])                       # fresh latents
    stayed = ref.crossings == crossed_before                                     # a crossing in this very tick restarts that game's score at 0
    assert np.array_equal(ref.s[stayed, 6], before[stayed, 6]) and (ref.s[~stayed, 6] == 0).all() and stayed.sum() >= 2
    assert ref.scores == []
    ref.tick(6, up)
    ref.tick(7, up)                                                              # t = 7: report
    assert len(ref.scores) == 1


def test_draw_rule_edges():
    p = np.array([0.25, 0.0, 0.75, 0.0], np.float32)
    assert AR.draw(p, 0.0) == 0 and AR.draw(p, 0.2499) == 0 and AR.draw(p, 0.25) == 2 and AR.draw(p, 0.999) == 2
    assert AR.draw(p, 1.0) == 2                                                  # u == 1.0: the last action with p > 0
    assert AR.draw(np.array([0.5, -0.1, 0.6, 0.0], np.float32), 0.3) == -1
    assert AR.draw(np.array([0.5, np.inf, 0.0, 0.0], np.float32), 0.3) == -1
    assert AR.draw(np.zeros(4, np.float32), 0.3) == -1
    # the uniform: word 0 of the counter (tag 0x70, game, 0, stage), as oracle.philox.uniforms with that tag, pass 0 and sample 0
    from oracle import philox as PX
    assert np.array_equal(AR.action_uniform(11, 7 + np.arange(5), 3), PX.uniforms(11, 5, 0, 0, 3, row_offset=7, tag=AR.TAG_AGENT))
