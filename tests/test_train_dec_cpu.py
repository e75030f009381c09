"""CPU tests of the decoder tail's backward: tests/train_dec_ref.py (autograd over conv_transpose2d with its own ReLUs, fp32) reproduces
the fixture captured from the reference's own ModelDown.po_net[12:] (tools/make_golden_train_dec.py) bit for bit; the GPU tests then hold
the engine against this restatement (tests/test_train_dec_gpu.py).  And the torch op of the feature is registered with the documented
schema."""
import json

import numpy as np
import pytest
import torch

import train_dec_ref as TD
from oracle import synth


@pytest.fixture(scope='module')
def fix(golden):
    g = golden('train_dec_g115')
    g['meta'] = json.loads(str(g['meta']))
    return g


def test_fixture_inputs_are_the_documented_batch(fix):
    m = fix['meta']
    h4, o1 = TD.inputs(m['batch_seed'], m['M'])
    assert h4.dtype == np.float32 and np.array_equal(h4, fix['h4']) and np.array_equal(o1, fix['o1'])
    assert 0.15 < (h4 > 0).mean() < 0.35 and 0.05 < o1.mean() < 0.15


def test_restatement_reproduces_reference_backward(fix):
    m = fix['meta']
    r = TD.run(synth.make_weights(m['wseed'], m['gain']), fix['h4'], fix['o1'], torch.float32, beta_o=m['beta_o'])
    assert np.array_equal(r['nlogpo1'], fix['nlogpo1']) and np.array_equal(r['po1'], fix['po1'])
    assert np.array_equal(r['d_h4'], fix['d_h4'])
    assert sum(v.size for v in r['grads'].values()) == TD.P
    for k in TD.KEYS:
        assert np.array_equal(r['grads'][k], fix['grad.' + k]), k
        assert np.abs(r['grads'][k]).max() > 0, k


def test_given_gates_equal_own_gates_when_taken_from_the_same_run(fix):
    """the gate override is the same function when the gates are the run's own activations"""
    m = fix['meta']
    w = synth.make_weights(m['wseed'], m['gain'])
    own = TD.run(w, fix['h4'], fix['o1'], torch.float64)
    giv = TD.run(w, fix['h4'], fix['o1'], torch.float64, gates=own['y'])
    assert np.array_equal(own['d_h4'], giv['d_h4'])
    for k in TD.KEYS:
        assert np.array_equal(own['grads'][k], giv['grads'][k]), k


def test_dec_tail_grad_op_schema():
    import daimc_amd
    ops = daimc_amd._lib.load_ops()
    schema = str(ops.dec_tail_grad.default._schema)
    assert schema.startswith('efe::dec_tail_grad(int ctx, Tensor'), schema
    assert 'efe_dec_tail_grad' in daimc_amd._lib.EXPORTS
    assert callable(daimc_amd.loss.grad_decoder_convs)
