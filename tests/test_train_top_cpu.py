"""CPU test of the training restatement: tests/train_ref.py (autograd + torch.optim.Adam over OracleModel.encode_s) reproduces the fixture
captured from the reference's own ModelTop + torchloss.train_model_top + optim.Adam (tools/make_golden_train_top.py) bit for bit --
kl_pi of every step, the gradients of step 1, and the weights and Adam state after step 3.  The GPU tests then hold the engine against
this restatement (tests/test_train_top_gpu.py)."""
import json

import numpy as np
import pytest

import train_ref as TR
from oracle import synth


@pytest.fixture(scope='module')
def fix(golden):
    g = golden('train_top_g115')
    g['meta'] = json.loads(str(g['meta']))
    return g


def test_fixture_inputs_are_the_documented_batch(fix):
    m = fix['meta']
    s, log_Ppi = TR.batch(m['batch_seed'], m['M'])
    assert np.array_equal(s, fix['s']) and np.array_equal(log_Ppi, fix['log_Ppi'])


def test_restatement_reproduces_reference_gradients(fix):
    m = fix['meta']
    kl, g = TR.grads(synth.make_weights(m['wseed'], m['gain']), fix['s'], fix['log_Ppi'])
    assert np.array_equal(kl, fix['kl_pi_1'])
    for k in TR.KEYS:
        assert np.array_equal(g[k], fix['grad1.' + k]), k


def test_restatement_reproduces_reference_training(fix):
    m = fix['meta']
    kls, w, ea, es = TR.train(synth.make_weights(m['wseed'], m['gain']), fix['s'], fix['log_Ppi'], m['steps'], m['lr'])
    for i in range(m['steps']):
        assert np.array_equal(kls[i], fix[f'kl_pi_{i + 1}']), i
    for k in TR.KEYS:
        assert np.array_equal(w[k], fix['w3.' + k]), k
        assert np.array_equal(ea[k], fix['exp_avg3.' + k]), k
        assert np.array_equal(es[k], fix['exp_avg_sq3.' + k]), k
    assert any(not np.array_equal(w[k], synth.make_weights(m['wseed'], m['gain'])['top.' + k]) for k in TR.KEYS)
