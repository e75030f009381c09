"""CPU tests of the whole decoder's backward: tests/train_dec_head_ref.py (autograd over F.linear / conv_transpose2d with the Philox masks
as multiplications and its own ReLUs, fp32) reproduces the fixture captured from the reference's own ModelDown.po_net in train mode
(tools/make_golden_train_dec_head.py) bit for bit on the recorded tensors and rows; the GPU tests then hold the engine against this
restatement (tests/test_train_dec_head_gpu.py).  And the torch op and the C entry point of the feature are registered."""
import json
import os

import numpy as np
import pytest
import torch

import train_dec_head_ref as TH
from oracle import philox as PX
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fix(golden):
    g = golden('train_dec_head_g115')
    g['meta'] = json.loads(str(g['meta']))
    return g


@pytest.fixture(scope='module')
def own32(fix):
    m = fix['meta']
    return TH.run(synth.make_weights(m['wseed'], m['gain']), fix['s'], fix['o1'], m['stage'], torch.float32, beta_o=m['beta_o'], seed=m['nseed'],
                  pass_=m['pass_id'], sample=m['sample'], row_offset=m['row_offset'])


def test_fixture_is_small_and_inputs_are_the_documented_batch(fix):
    m = fix['meta']
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'train_dec_head_g115.npz')) < 512 * 1024
    s, o1 = TH.inputs(m['batch_seed'], m['M'])
    assert s.dtype == np.float32 and np.array_equal(s, fix['s']) and np.array_equal(o1, fix['o1'])
    assert s.shape == (2, 10) and 0.05 < o1.mean() < 0.15


def test_restatement_reproduces_reference_backward(fix, own32):
    m = fix['meta']
    r = own32
    assert np.array_equal(r['nlogpo1'], fix['nlogpo1']) and np.array_equal(r['d_s'], fix['d_s'])
    assert list(r['grads']) == list(TH.KEYS) and sum(v.size for v in r['grads'].values()) == TH.P
    seen = 0
    for k in TH.KEYS:
        g = r['grads'][k]
        assert np.abs(g).max() > 0, k
        if 'grad.' + k in fix:
            want = fix['grad.' + k]
            got = g[0::m['row_stride'][k]] if k in m['row_stride'] else g
            assert k in m['row_stride'] or k in m['whole'], k
            assert np.array_equal(got, want), k
            seen += 1
        g64 = g.astype(np.float64)
        np.testing.assert_allclose([g64.sum(), np.abs(g64).sum()], fix['sums.' + k], rtol=1e-12, atol=0, err_msg=k)
    assert seen == len(m['row_stride']) + len(m['whole']) == 12


def test_given_gates_equal_own_gates_when_taken_from_the_same_run(fix):
    """the gate override is the same function when the gates are the run's own activations"""
    m = fix['meta']
    w = synth.make_weights(m['wseed'], m['gain'])
    own = TH.run(w, fix['s'], fix['o1'], m['stage'], torch.float64)
    giv = TH.run(w, fix['s'], fix['o1'], m['stage'], torch.float64, gates=own['h'] + own['y'])
    for k in ('nlogpo1', 'po1', 'd_s', 'd_h4'):
        assert np.array_equal(own[k], giv[k]), k
    for k in TH.KEYS:
        assert np.array_equal(own['grads'][k], giv['grads'][k]), k


def test_fc4_mask_is_the_nhwc_keyed_mask_transposed(fix, own32):
    """the reference feature c * 256 + p of po_net.9 takes the mask bit of the engine's NHWC feature p * 64 + c"""
    m = fix['meta']
    M = m['M']
    raw = PX.dropout_mask(m['nseed'], PX.TAG_DEC + 3, M, 16384, m['pass_id'], m['sample'], m['stage'], m['row_offset'])      # indexed by f' = p * 64 + c
    mk = own32['masks'][3]
    assert mk.shape == (M, 16384) and set(np.unique(mk)) == {0.0, 2.0}
    assert np.array_equal(mk.reshape(M, 64, 256), raw.reshape(M, 256, 64).transpose(0, 2, 1))
    assert not np.array_equal(mk, raw)
    c, p = 37, 201
    assert np.array_equal(mk[:, c * 256 + p], raw[:, p * 64 + c])
    # the stored activation is zero wherever the mask drops the feature, and the first three masks are untransposed
    assert not (own32['h'][3][mk == 0] != 0).any()
    for li in range(3):
        assert np.array_equal(own32['masks'][li], PX.dropout_mask(m['nseed'], PX.TAG_DEC + li, M, 256, m['pass_id'], m['sample'], m['stage'], m['row_offset']))


def test_dec_grad_op_schema_and_export():
    import daimc_amd
    ops = daimc_amd._lib.load_ops()
    schema = str(ops.dec_grad.default._schema)
    assert schema.startswith('efe::dec_grad(int ctx, Tensor s, Tensor o1, float scale, float beta_o, int seed, int stage'), schema
    assert 'efe_dec_grad' in daimc_amd._lib.EXPORTS
    assert daimc_amd._lib.load().efe_dec_grad.argtypes is not None
    assert callable(daimc_amd.loss.grad_decoder)
    assert daimc_amd.loss.DEC_HEAD_KEYS + daimc_amd.loss.DEC_CONVT_KEYS == TH.KEYS
