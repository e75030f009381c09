"""CPU test of the transition net's training restatement: tests/train_mid_ref.py (autograd + torch.optim.Adam over OracleModel.transition
with the Philox dropout masks) reproduces the fixture captured from the reference's own ModelMid (train mode) + torchloss.train_model_mid
+ optim.Adam (tools/make_golden_train_mid.py) bit for bit on everything recorded -- ps1_mean / ps1_logvar of every step, the gradients
of step 1, and the weights and Adam state after step 3 (the 512 x 512 tensors by their recorded slices and float64 sums).  The GPU
tests then hold the engine against this restatement (tests/test_train_mid_gpu.py)."""
import json

import numpy as np
import pytest

import train_mid_ref as TM
from oracle import synth


@pytest.fixture(scope='module')
def fix(golden):
    g = golden('train_mid_g115')
    g['meta'] = json.loads(str(g['meta']))
    return g


@pytest.fixture(scope='module')
def weights(fix):
    return synth.make_weights(fix['meta']['wseed'], fix['meta']['gain'])


def inputs(fix):
    return tuple(fix[k] for k in ('s0', 'pi', 'qs1_mean', 'qs1_logvar', 'omega'))


def assert_recorded(fix, name, key, arr):
    """`arr` equals what the fixture holds of tensor `key` under `name`, bit for bit"""
    m = fix['meta']
    if key in m['big']:
        assert np.array_equal(arr[np.ix_(m['slice'], m['idx'])], fix[f'{name}.{key}.rows']), (name, key, 'rows')
        assert np.array_equal(arr[np.ix_(m['idx'], m['slice'])], fix[f'{name}.{key}.cols']), (name, key, 'cols')
        sums = np.array([arr.astype(np.float64).sum(), np.square(arr.astype(np.float64)).sum()])
        assert np.array_equal(sums, fix[f'{name}.{key}.sums']), (name, key, 'sums')
    else:
        assert np.array_equal(arr, fix[f'{name}.{key}']), (name, key)


def test_fixture_inputs_are_the_documented_batch(fix):
    m = fix['meta']
    for a, b in zip(TM.batch_mid(m['batch_seed'], m['M']), inputs(fix)):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert m['nseed'] == TM.SEED and m['pass_id'] == TM.PASS_FE_T


def test_restatement_reproduces_reference_gradients(fix, weights):
    m = fix['meta']
    _, mean, lv, g = TM.grads(weights, inputs(fix), m['stage'])
    assert np.array_equal(mean, fix['ps1_mean_1']) and np.array_equal(lv, fix['ps1_logvar_1'])
    for k in TM.KEYS:
        assert_recorded(fix, 'grad1', k, g[k])


def test_restatement_reproduces_reference_training(fix, weights):
    m = fix['meta']
    means, lvs, _, w, ea, es = TM.train(weights, inputs(fix), m['stage'], m['steps'], m['lr'])
    for i in range(m['steps']):
        assert np.array_equal(means[i], fix[f'ps1_mean_{i + 1}']), i
        assert np.array_equal(lvs[i], fix[f'ps1_logvar_{i + 1}']), i
    for k in TM.KEYS:
        assert_recorded(fix, 'w3', k, w[k])
        assert_recorded(fix, 'exp_avg3', k, ea[k])
        assert_recorded(fix, 'exp_avg_sq3', k, es[k])
    assert all(not np.array_equal(w[k], weights['mid.' + k]) for k in TM.KEYS)
