"""CPU tests of the decoder tail's backward at every admitted geometry: tests/train_dec_g_ref.py is tests/train_dec_ref.py at (1, 64), bit
for bit in fp32 (so the reference's own po_net[12:], through tests/test_train_dec_cpu.py's fixture), its shapes follow the reference's
geometry rule elsewhere, and the entry point is declared, bound and registered."""
import os
import re

import numpy as np
import pytest
import torch

import train_dec_g_ref as TG
import train_dec_ref as TD
from conftest import ROOT
from oracle import synth


def test_reference_equals_the_1x64x64_reference_bit_for_bit():
    w = synth.make_weights(1234, 1.15)
    h4, o1 = TD.inputs(1003, 3)
    g4, g1 = TG.inputs(1003, 3, 1, 64)
    assert np.array_equal(h4, g4) and np.array_equal(o1, g1)
    a = TD.run(w, h4, o1, torch.float32)
    b = TG.run(w, h4, o1, 1, 64, torch.float32)
    for k in ('nlogpo1', 'po1', 'd_h4'):
        assert np.array_equal(a[k], b[k]), k
    for k in TD.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for i in range(3):
        assert np.array_equal(a['y'][i], b['y'][i]), i
    giv = TG.run(w, h4, o1, 1, 64, torch.float32, gates=a['y'])
    ref = TD.run(w, h4, o1, torch.float32, gates=a['y'])
    assert np.array_equal(giv['d_h4'], ref['d_h4'])
    assert TG.param_count(1) == TD.P and TG.KEYS == TD.KEYS


@pytest.mark.parametrize('C,R', [(1, 36), (3, 32), (3, 84)])
def test_reference_shapes_follow_the_geometry(C, R):
    w = synth.make_weights(1234, 1.15, 4, C, R)
    B = TG.base_of(R)
    h4, o1 = TG.inputs(1001, 1, C, R)
    assert h4.shape == (1, 64 * B * B) and o1.shape == (1, C, R, R)
    r = TG.run(w, h4, o1, C, R, torch.float32)
    assert r['po1'].shape == (1, C, R, R) and r['d_h4'].shape == h4.shape
    assert [y.shape for y in r['y']] == [(1, 64, B, B), (1, 64, 2 * B, 2 * B), (1, 32, R, R)]
    assert sum(v.size for v in r['grads'].values()) == TG.param_count(C)
    assert r['grads']['po_net.19.weight'].shape == (32, C, 3, 3)


def test_entry_point_is_declared_bound_and_registered():
    import daimc_amd
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'efe_engine.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+efe_dec_tail_grad_g\s*\(', txt)
    assert 'efe_dec_tail_grad_g' in daimc_amd._lib.SIGNATURES
    assert daimc_amd._lib.SIGNATURES['efe_dec_tail_grad_g'] == daimc_amd._lib.SIGNATURES['efe_dec_tail_grad']
    assert callable(daimc_amd.loss.grad_decoder_convs_g)
    daimc_amd._lib.load_ops()
    schema = str(torch.ops.efe_g.dec_tail_grad.default._schema)
    assert schema.startswith('efe_g::dec_tail_grad(int ctx, Tensor h4, Tensor o1, float scale, float beta_o, bool want_y)'), schema
