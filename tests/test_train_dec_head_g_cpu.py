"""CPU tests of the whole decoder's backward at every admitted geometry: tests/train_dec_head_g_ref.py is tests/train_dec_head_ref.py at
(1, 64) bit for bit (which tests/test_train_dec_head_cpu.py pins to the reference's own po_net), and at other geometries its forward is
oracle.efe_oracle's decoder on the same weights and keys bit for bit, which pins the transposed keying of po_net.9's mask at a feature count
other than 16384.  And the C entry point and the torch op of the feature are declared, listed and exported."""
import os
import re

import numpy as np
import pytest
import torch

import train_dec_head_g_ref as THG
import train_dec_head_ref as TH
from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 3


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('gated', [False, True])
def test_at_1x64x64_it_is_the_specialised_reference(dtype, gated):
    w = synth.make_weights(1234, 1.15)
    s, o1 = THG.inputs(1002, 2, 1, 64)
    s0, o0 = TH.inputs(1002, 2)
    assert np.array_equal(s, s0) and np.array_equal(o1, o0)
    gates = None
    if gated:
        own = TH.run(w, s, o1, STAGE, torch.float32)
        gates = own['h'] + own['y']
    a = THG.run(w, s, o1, 1, 64, STAGE, dtype, gates=gates)
    b = TH.run(w, s, o1, STAGE, dtype, gates=gates)
    assert THG.KEYS == TH.KEYS and THG.param_count(1, 64) == TH.P
    for k in ('nlogpo1', 'po1', 'd_s', 'd_h4'):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    for k in TH.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    for name in ('h', 'y', 'a_head', 'a', 'masks'):
        assert len(a[name]) == len(b[name]) and all(np.array_equal(x, y) for x, y in zip(a[name], b[name])), name


@pytest.mark.parametrize('geo', [(3, 3, 32), (4, 1, 36)])
def test_forward_is_the_oracle_decoder(geo):
    """fp32, own gates: po1 is oracle.efe_oracle's decoder on the same weights and keys, bit for bit"""
    pi, C, R = geo
    w = synth.make_weights(1234, 1.15, *geo)
    s, o1 = THG.inputs(1002, 2, C, R)
    r = THG.run(w, s, o1, C, R, STAGE, torch.float32)
    orc = OracleModel(w, PhiloxNoise(THG.SEED), pi_dim=pi, channels=C, resolution=R)
    po = orc.decoder(torch.tensor(s), THG.PASS_FE_DOWN, 0, STAGE, 0).detach().numpy().reshape(2, C, R, R)
    assert np.array_equal(r['po1'], po)
    # the last mask is the NHWC-keyed mask transposed at this feature count; the first three are untransposed
    B, n = THG.base_of(R), THG.n_feat(R)
    raw = PX.dropout_mask(THG.SEED, PX.TAG_DEC + 3, 2, n, THG.PASS_FE_DOWN, 0, STAGE, 0)
    mk = r['masks'][3]
    assert mk.shape == (2, n) and np.array_equal(mk.reshape(2, 64, B * B), raw.reshape(2, B * B, 64).transpose(0, 2, 1))
    c, p = 37, B * B - 3
    assert np.array_equal(mk[:, c * B * B + p], raw[:, p * 64 + c])
    assert not (r['h'][3][mk == 0] != 0).any()
    assert sum(v.size for v in r['grads'].values()) == THG.param_count(C, R)


def test_entry_point_is_declared_listed_and_exported():
    import daimc_amd
    header = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    assert re.search(r'^int efe_dec_grad_g\(efe_ctx\*, const float\* s, const float\* o1, int M, float scale, float beta_o, const efe_noise\* nz,', header, re.M)
    assert 'efe_dec_grad_g' in daimc_amd._lib.SIGNATURES and 'efe_dec_grad_g' in daimc_amd._lib.EXPORTS
    assert daimc_amd._lib.SIGNATURES['efe_dec_grad_g'] == daimc_amd._lib.SIGNATURES['efe_dec_grad']
    assert daimc_amd._lib.load().efe_dec_grad_g.argtypes is not None
    daimc_amd._lib.load_ops()
    schema = str(torch.ops.efe_g.dec_grad.default._schema)
    assert schema.startswith('efe_g::dec_grad(int ctx, Tensor s, Tensor o1, float scale, float beta_o, int seed, int stage'), schema
    assert callable(daimc_amd.loss.grad_decoder_g)
    assert daimc_amd.loss.DEC_HEAD_KEYS + daimc_amd.loss.DEC_CONVT_KEYS == THG.KEYS
