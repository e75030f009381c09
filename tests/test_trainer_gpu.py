"""GPU tests (-m gpu) of daimc_amd.train.Trainer: the loop of the reference's train.py:100-173 over loss.train_step.

Eight games on the synthetic sprite bank, engine seed 7, weights 'g115', a seeded torch.Generator on the device for the action draws.
Twins share every seed, so two loops that issue the same calls stay bit-identical."""
import numpy as np
import pytest
import torch

from test_train_step_gpu import assert_same, snapshot
from train_common import SEED, c, model_for

pytestmark = pytest.mark.gpu

GAMES = 8


def setup(**kw):
    import daimc_amd
    m = model_for('g115', fresh=True)
    games = daimc_amd.Game(GAMES, model=m, seed=3)
    gen = torch.Generator(device='cuda:0').manual_seed(11)
    return m, games, gen, daimc_amd.Trainer(m, games, generator=gen, **kw)


def hand_round(m, games, gen, opts, means_row):
    """train.py:107-126 written out with the public calls"""
    import daimc_amd
    games.randomize_environment_all()
    o0, o1, pi0, log_Ppi = daimc_amd.make_batch_dsprites_active_inference(games=games, model=m, deepness=1, samples=1, calc_mean=True, repeats=5,
                                                                          generator=gen)
    return daimc_amd.loss.train_step(m, o0, o1, pi0, log_Ppi, opts, means=means_row)


def test_two_rounds_equal_the_hand_written_loop():
    import daimc_amd
    ma, _, _, tr = setup()
    mb = model_for('g115', fresh=True)
    gb, genb = daimc_amd.Game(GAMES, model=mb, seed=3), torch.Generator(device='cuda:0').manual_seed(11)
    ob = {'top': daimc_amd.Adam(mb.model_top, lr=1e-4), 'mid': daimc_amd.Adam(mb.model_mid, lr=1e-4), 'down': daimc_amd.Adam(mb.model_down, lr=1e-3)}
    means_b = torch.zeros(2, 8, device='cuda:0')
    for i in range(2):
        A = tr.round()
        B = hand_round(mb, gb, genb, ob, means_b[i])
        np.testing.assert_array_equal(c(A.F_down), c(B.F_down))
    assert tr.rounds_done == 2 and tuple(tr.means.shape) == (2, 8)
    assert c(tr.means).tobytes() == c(means_b).tobytes() and np.isfinite(c(tr.means)).all()
    assert_same('trainer against the loop', snapshot(ma, tr.optimizers), snapshot(mb, ob))
    assert ma._stage == mb._stage and [o._step for o in tr.optimizers.values()] == [2, 2, 2]
    assert isinstance(ma.gamma, float) and ma.gamma == 0.5


def test_gamma_schedule():
    """train.py:101-102 run literally on a float32 tensor, against begin_epoch at every epoch up to 200"""
    m, _, _, tr = setup()
    m.gamma = 0.0
    g = torch.tensor(0.0)
    seen = {}
    for epoch in range(1, 201):
        if epoch > 30 and g < 0.8:
            g += 0.01
        seen[epoch] = (tr.begin_epoch(epoch), g.item())
        assert m.gamma == seen[epoch][0]
    print({e: seen[e] for e in (30, 31, 200)})
    assert all(a == b for a, b in seen.values())
    assert seen[30][0] == 0.0 and seen[31][0] == float(np.float32(0.01)) and 0.79 < seen[200][0] < 0.82


def test_epoch_and_evaluate():
    import daimc_amd
    from daimc_amd.train import EPOCH_KEYS, EVAL_KEYS, make_batch_random
    m, games, gen, tr = setup()
    out = tr.epoch(2)
    assert tuple(out) == EPOCH_KEYS and all(isinstance(v, float) and np.isfinite(v) for v in out.values()), out
    last = c(tr.means)[-1]
    assert out['omega_last'] == float(last[1]) and out['omega_std_last'] == float(last[7])
    o0, o1, pi0 = make_batch_random(games, 5, gen)
    stage = m._stage
    st = tr.evaluate(o0, o1, pi0)
    assert tuple(st) == EVAL_KEYS
    fe = daimc_amd.free_energy(m, o0, o1, pi0, torch.log(pi0 + 1e-15), omega=1.0 / 2.0 + 1.5, stage=stage)
    assert st['F'] == (fe.F_down + fe.F_mid + fe.F_top).mean().item()
    assert st['F_top'] == fe.F_top.mean().item() and st['mse_o'] == fe.nlogpo1.mean().item() and st['kl_div_pi_med'] == fe.kl_pi.median().item()
    assert st['omega'] == out['omega_last'] and st['var_gamma'] == 0.5 and np.isfinite(st['TC']) and st['kl_div_s_anal'].shape == (10,)


def test_checkpoint_round_trip_continues_bit_identically(tmp_path):
    import daimc_amd
    ma, _, _, ta = setup()
    md, gd, gend, td = setup()
    ta.round(); ta.round()
    td.round()
    md.save_all(str(tmp_path), {}, optimizers=td.optimizers)
    me = model_for('g100', fresh=True)                # other weights: everything it continues with comes from the checkpoint
    _, opts = me.load_all(str(tmp_path))
    assert sorted(opts) == ['down', 'mid', 'top']
    me._stage = md._stage                             # (the noise stage counter is the caller's, not the checkpoint's)
    te = daimc_amd.Trainer(me, gd, opts, generator=gend)
    te.round()
    assert c(te.means)[0].tobytes() == c(ta.means)[1].tobytes()
    assert_same('resumed against uninterrupted', snapshot(ma, ta.optimizers), snapshot(me, te.optimizers))
