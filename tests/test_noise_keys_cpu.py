"""CPU tests of the numpy Philox mirror (oracle/philox.py) at the edges of the key space, where the engine wraps: the counter words
row, stage and stream are uint32_t in csrc/philox.h, so a row range that straddles 2^32, a stage past 0xFFFFFFFF and
`episode * depth + t` past 2^32 wrap, `sample` is 16 bits of the stream word, and the 64-bit seed is two 32-bit key words.  The mirror
states the same -- otherwise the oracle cannot say what the engine must compute there (tests/test_noise_keys_gpu.py).  The seed
identities held before the mirror reduced its counter words and are pinned so that they stay."""
import numpy as np
import pytest
import torch

from oracle import efe_oracle as EO
from oracle import env_oracle as EV
from oracle import mcts_oracle as MO
from oracle import philox as PX

P, S, ST = PX.PASS_T2, 3, 5          # a pass / sample / stage with every field non-zero


def _mask(seed=7, rows=2, sample=S, stage=ST, row_offset=0):
    return PX.dropout_mask(seed, PX.TAG_MID + 1, rows, 200, P, sample, stage, row_offset)


def _normals(seed=7, rows=2, sample=S, stage=ST, row_offset=0):
    return PX.normals(seed, rows, 10, P, sample, stage, row_offset)


def _uniforms(seed=7, rows=2, sample=S, stage=ST, row_offset=0):
    return PX.uniforms(seed, rows, P, sample, stage, row_offset)


DRAWS = [_mask, _normals, _uniforms]


@pytest.mark.parametrize('draw', DRAWS)
def test_rows_wrap_at_2_32(draw):
    """a launch of 4 rows at row_offset 2^32 - 2 holds global rows 2^32 - 2, 2^32 - 1, 0, 1"""
    wrapped = draw(rows=4, row_offset=2 ** 32 - 2)
    assert np.array_equal(wrapped[2:], draw(rows=2, row_offset=0))
    assert np.array_equal(wrapped[:2], draw(rows=2, row_offset=2 ** 32 - 2))
    assert not np.array_equal(wrapped[:2], wrapped[2:])
    assert np.array_equal(draw(rows=2, row_offset=2 ** 32 + 9), draw(rows=2, row_offset=9))
    # the sign bit of the row word is an ordinary bit
    assert np.array_equal(draw(rows=4, row_offset=2 ** 31 - 2)[2:], draw(rows=2, row_offset=2 ** 31))


@pytest.mark.parametrize('draw', DRAWS)
def test_stage_is_modulo_2_32(draw):
    assert np.array_equal(draw(stage=2 ** 32 + 3), draw(stage=3))
    assert np.array_equal(draw(stage=0xFFFFFFFE + 2), draw(stage=0))
    assert not np.array_equal(draw(stage=0x80000003), draw(stage=3))


@pytest.mark.parametrize('draw', DRAWS)
def test_sample_is_16_bits(draw):
    assert np.array_equal(draw(sample=0x10000), draw(sample=0))
    assert np.array_equal(draw(sample=0x10000 + S), draw(sample=S))
    assert not np.array_equal(draw(sample=0xFFFF), draw(sample=0))
    assert PX.stream_id(0x10008, 0x10003) == (8 << 16) | 3


@pytest.mark.parametrize('draw', DRAWS)
def test_seed_is_64_bits(draw):
    assert np.array_equal(draw(seed=-1), draw(seed=2 ** 64 - 1))
    assert np.array_equal(draw(seed=2 ** 64 + 7), draw(seed=7))
    assert not np.array_equal(draw(seed=0xDEADBEEF << 32), draw(seed=0))               # k0 == 0: the high word alone keys the draw
    assert not np.array_equal(draw(seed=7 + (0x9E3779B9 << 32)), draw(seed=7))        # the high word is used beside the low one
    assert not np.array_equal(draw(seed=0xDEADBEEF << 32), draw(seed=0xDEADBEEF))     # and the words are not interchangeable


def test_in_range_keys_did_not_move():
    """known words of the generator under the draw layout (the reduction changes nothing below 2^32): row 1000, stage 110"""
    k0, k1 = PX._key(2026)
    w = PX.philox4x32_10(np.uint64(PX.TAG_ACT << 16), np.uint64(1000), np.uint64(PX.stream_id(P, S)), np.uint64(110), k0, k1)
    assert PX.uniforms(2026, 1, P, S, 110, 1000)[0] == PX._u01(w[0])


def test_env_mirror_wraps_like_the_draws():
    """the environment's draws (oracle/env_oracle.py, TAG_ENV): game = game_offset + e and stage are the same uint32 counter words"""
    seed = 7 + (0x9E3779B9 << 32)
    s4, r4 = EV.reset(seed, 4, 0x80000003, game_offset=0xFFFFFFFE)
    s2, r2 = EV.reset(seed, 2, 0x80000003)
    assert np.array_equal(s4[2:], s2) and np.array_equal(r4[2:], r2) and not np.array_equal(s4[:2], s2)
    assert np.array_equal(EV.reset(seed, 2, 2 ** 32 + 3)[0], EV.reset(seed, 2, 3)[0])
    assert not np.array_equal(EV.reset(seed, 2, 3)[0], EV.reset(7, 2, 3)[0])


class _Recorder(EO.PhiloxNoise):
    """PhiloxNoise that notes the (stage, row_offset) of every draw"""

    def __init__(self, seed):
        super().__init__(seed)
        self.seen = set()

    def mask(self, tag, rows, n_feat, pas, sample, stage, row_offset=None, fc4_perm=False):
        self.seen.add((stage, row_offset))
        return torch.ones(rows, n_feat)

    def eps(self, rows, n, pas, sample, stage, row_offset=None):
        self.seen.add((stage, row_offset))
        return torch.zeros(rows, n)

    def uniform(self, rows, pas, sample, stage, row_offset=None):
        self.seen.add((stage, row_offset))
        return np.full(rows, 0.5, dtype=np.float32)


class _Stub(EO.OracleModel):
    """OracleModel with the networks cut out: only the stage / row bookkeeping of the callers runs"""

    def __init__(self, noise):
        self.noise, self.s_dim, self.pi_dim, self.dtype = noise, 10, 4, torch.float32
        self.pi_one_hot = torch.eye(4)
        self.calls = []

    def encode_s(self, s0):
        return None, torch.full((s0.shape[0], 4), 0.25), None

    def transition_with_sample(self, pi, s0, pas, sample, stage, ro=None):
        self.calls.append(('trans', stage, ro))
        z = torch.zeros(s0.shape[0], 10)
        return z, z, z

    def encoder(self, o, pas, sample, stage, ro=None):
        self.calls.append(('enc', stage, ro))
        return torch.zeros(o.shape[0], 10), torch.zeros(o.shape[0], 10)

    def calculate_G(self, s0, pi0, samples, stage, ro=None):
        self.calls.append(('G', stage, ro))
        z = torch.zeros(s0.shape[0])
        return z, [z, z, z], torch.zeros(s0.shape[0], 10), torch.zeros(s0.shape[0], 10), None

    def calculate_G_mean(self, s0, pi0, stage, ro=None):
        self.calls.append(('Gmean', stage, ro))
        z = torch.zeros(s0.shape[0])
        return z, [z, z, z], torch.zeros(s0.shape[0], 10), None

    def calculate_G_given_trajectory(self, s0, ps1, mean, lv, pi0, stage, ro=None):
        self.calls.append(('traj', stage, ro))
        return torch.zeros(s0.shape[0])


def test_oracle_stage_and_row_arithmetic_is_uint32():
    """`stage0 + t` of the rollouts and `episode * depth + t` of the simulation are uint32 expressions in the engine (kernels.h
    group_key, fused.hip k_sim_chain): the oracle hands the reduced values on"""
    orc = _Stub(_Recorder(7))
    orc.calculate_G_repeated(torch.zeros(2, 1, 64, 64), torch.zeros(2, 4), 3, False, 1, 0xFFFFFFFE)
    assert [c[1] for c in orc.calls if c[0] == 'G'] == [0xFFFFFFFE, 0xFFFFFFFF, 0]
    orc.calls.clear()
    orc.calculate_G_4_repeated(torch.zeros(4, 1, 64, 64), 3, True, 1, 0xFFFFFFFF)
    assert [c[1] for c in orc.calls if c[0] == 'Gmean'] == [0xFFFFFFFF, 0, 1]
    orc.calls.clear()
    # episode 0x33333334, depth 5: 0x33333334 * 5 = 2^32 + 4
    orc.mcts_step_simulate(torch.zeros(10), 5, False, 9, episode=0x33333334)
    assert [c for c in orc.calls if c[0] == 'traj'] == [('traj', 9, 4)]
    assert all(c[2] == 0x33333334 for c in orc.calls if c[0] == 'trans')


def test_planner_stage_counter_and_expansion_rows_wrap():
    """mcts_oracle.plan: one stage per engine-level call, counted modulo 2^32; expansion rows 4 e + a modulo 2^32"""
    orc = _Stub(_Recorder(7))
    orc.channels, orc.resolution = 1, 64
    p = MO.Params(repeats=2, simulation_depth=2, use_means=True, threshold=2.0)
    MO.plan(orc, np.zeros((1, 64, 64), np.float32), p, 0xFFFFFFFE, episode=0x40000001)
    stages = [c[1] for c in orc.calls if c[0] in ('enc', 'Gmean', 'traj')]
    assert stages == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1, 2, 3]          # root encode, root expansion, (expansion, simulation) x 2
    assert all(c[2] == 4 for c in orc.calls if c[0] == 'Gmean')    # 4 * 0x40000001 = 2^32 + 4
    assert all(c[2] == 0x80000002 for c in orc.calls if c[0] == 'traj')     # 0x40000001 * 2: the sign bit is an ordinary bit
