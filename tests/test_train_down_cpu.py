"""CPU tests of the gradient of F_down for all of ModelDown: tests/train_down_ref.py (autograd over F.conv2d / F.linear / conv_transpose2d
with the Philox masks as multiplications, the Philox normals and its own ReLUs, fp32) reproduces the fixture captured from the
reference's own compute_loss_down + F.mean().backward() (tools/make_golden_train_down.py) bit for bit on the recorded elements, for the
three gamma branches; the GPU tests then hold the engine against this restatement (tests/test_train_enc_gpu.py,
tests/test_train_down_gpu.py).  The gate override is the same function on a run's own gates, the fp32 restatement's own gates meet the
GPU tests' gate condition against the fp64 one on every input those tests use, and the torch ops, the C entry points and the key lists
of the feature are registered."""
import json
import os

import numpy as np
import pytest
import torch

import train_dec_head_ref as TH
import train_down_ref as TDN
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stride(n):
    return 1 if n <= 1024 else 61 if n <= 62464 else 1021


@pytest.fixture(scope='module')
def fix(golden):
    g = golden('train_down_g115')
    g['meta'] = json.loads(str(g['meta']))
    return g


def own(fix, gamma, dtype=torch.float32, **kw):
    m = fix['meta']
    return TDN.run(synth.make_weights(m['wseed'], m['gain']), fix['o1'], fix['ps1_mean'], fix['ps1_logvar'], fix['omega'], m['stage'], dtype,
                   gamma=gamma, beta_s=m['beta_s'], beta_o=m['beta_o'], seed=m['nseed'], pass_=m['pass_id'], sample=m['sample'],
                   row_offset=m['row_offset'], **kw)


def test_fixture_is_small_and_inputs_are_the_documented_batch(fix):
    m = fix['meta']
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'train_down_g115.npz')) < 512 * 1024
    o1, pm, pv, om = TDN.inputs(m['batch_seed'], m['M'])
    for a, k in ((o1, 'o1'), (pm, 'ps1_mean'), (pv, 'ps1_logvar'), (om, 'omega')):
        assert a.dtype == np.float32 and np.array_equal(a, fix[k]), k
    assert np.array_equal(o1, TH.inputs(m['batch_seed'], m['M'])[1])
    assert om.min() >= 1.5 and om.max() <= 2.5 and m['gammas'] == [0.0, 0.5, 1.0]


@pytest.mark.parametrize('gi', [0, 1, 2])
def test_restatement_reproduces_reference_backward(fix, gi):
    r = own(fix, fix['meta']['gammas'][gi])
    for k in ('F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'qs1'):
        assert np.array_equal(r[k], fix[f'g{gi}.{k}']), k
    assert np.array_equal(r['po1'].reshape(-1)[::stride(r['po1'].size)], fix[f'g{gi}.po1'])
    assert list(r['grads']) == list(TDN.KEYS) and len(TDN.KEYS) == 32 and sum(v.size for v in r['grads'].values()) == TDN.P == 4787125
    assert sum(r['grads'][k].size for k in TDN.ENC_KEYS) == TDN.P_ENC
    for k in TDN.KEYS:
        g = r['grads'][k].reshape(-1)
        assert np.abs(g).max() > 0, k
        assert np.array_equal(g[::stride(g.size)], fix[f'g{gi}.grad.{k}']), k
        g64 = g.astype(np.float64)
        np.testing.assert_allclose([g64.sum(), np.abs(g64).sum()], fix[f'g{gi}.sums.{k}'], rtol=1e-12, atol=0, err_msg=k)


def test_gamma_branches_differ(fix):
    F = [fix[f'g{gi}.F_down'] for gi in range(3)]
    assert not np.array_equal(F[0], F[1]) and not np.array_equal(F[1], F[2]) and not np.array_equal(F[0], F[2])


def test_given_gates_equal_own_gates_when_taken_from_the_same_run(fix):
    """the gate override is the same function when the gates are the run's own activations, in the composed run and in the encoder's"""
    a = own(fix, 0.5, torch.float64)
    b = own(fix, 0.5, torch.float64, gates=a['y'] + a['h'], dec_gates=a['dec_h'] + a['dec_y'])
    for k in ('F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'po1', 'qs1', 'mean', 'logvar', 'g_mean', 'g_logvar'):
        assert np.array_equal(a[k], b[k]), k
    for k in TDN.KEYS:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k
    m = fix['meta']
    w = synth.make_weights(m['wseed'], m['gain'])
    gm, gv = TDN.upstream(m['batch_seed'], m['M'])
    c = TDN.run_encoder(w, fix['o1'], gm, gv, m['stage'], torch.float64)
    d = TDN.run_encoder(w, fix['o1'], gm, gv, m['stage'], torch.float64, gates=c['y'] + c['h'])
    assert np.array_equal(c['mean'], d['mean']) and np.array_equal(c['logvar'], d['logvar'])
    for k in TDN.ENC_KEYS:
        assert np.array_equal(c['grads'][k], d['grads'][k]), k


def test_encoder_vjp_of_the_composed_upstream_is_the_composed_gradient(fix):
    """chain rule: run_encoder on run's g_mean / g_logvar gives run's qs_net gradients (fp64, to rounding)"""
    m = fix['meta']
    a = own(fix, 0.5, torch.float64)
    c = TDN.run_encoder(synth.make_weights(m['wseed'], m['gain']), fix['o1'], a['g_mean'], a['g_logvar'], m['stage'], torch.float64)
    for k in TDN.ENC_KEYS:
        np.testing.assert_allclose(c['grads'][k], a['grads'][k], rtol=1e-9, atol=1e-14, err_msg=k)


GATE_CASES = [('g115', M) for M in (1, 2, 5, 17, 33, 65)] + [(f, M) for f in ('g100', 'sparse') for M in (1, 5)] + [('saturated', 2)]


@pytest.mark.parametrize('fam,M', GATE_CASES)
def test_fp32_gates_meet_the_gate_condition_against_fp64(fam, M):
    """the encoder's seven gated layers on the inputs of the GPU tests: the fp32 restatement's gate may differ from the fp64 one's only
    where |a_64| <= 1e-5, on at most 1e-4 of a layer (the condition the GPU tests hold the engine to)"""
    w = synth.make_weights(1234, 1.15) if fam == 'g115' else synth.make_weights(7, 1.0) if fam == 'g100' else synth.stress_weights(fam)
    o1 = TDN.inputs(2000 + M, M)[0]
    mk = TDN.enc_masks(M, 3)
    acts = {}
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            p = {k: torch.tensor(np.array(w['down.' + k])).to(dt) for k in TDN.ENC_KEYS}
            _, ys, hs, pre_c, pre_d = TDN.encode(p, torch.tensor(o1).to(dt), mk, dt)
            acts[dt] = ([t.numpy() for t in ys + hs], [t.numpy() for t in pre_c + pre_d])
    for li in range(7):
        a64 = acts[torch.float64][1][li]
        diff = (acts[torch.float32][0][li] > 0) != (acts[torch.float64][0][li] > 0)
        worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
        assert worst <= 1e-5 and diff.sum() <= 1e-4 * diff.size, (li, int(diff.sum()), worst)


def test_ops_exports_and_key_lists_are_registered():
    import daimc_amd
    ops = daimc_amd._lib.load_ops()
    schema = str(ops.enc_grad.default._schema)
    assert schema.startswith('efe::enc_grad(int ctx, Tensor o, Tensor d_mean, Tensor d_logvar, int seed, int stage'), schema
    schema = str(ops.down_grad.default._schema)
    assert schema.startswith('efe::down_grad(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o'), schema
    lib = daimc_amd._lib.load()
    for name in ('efe_enc_grad', 'efe_down_grad'):
        assert name in daimc_amd._lib.EXPORTS and getattr(lib, name).argtypes is not None, name
    assert callable(daimc_amd.loss.grad_encoder) and callable(daimc_amd.loss.grad_down)
    assert daimc_amd.loss.ENC_KEYS == TDN.ENC_KEYS
    assert daimc_amd.loss.ENC_KEYS + daimc_amd.loss.DEC_HEAD_KEYS + daimc_amd.loss.DEC_CONVT_KEYS == TDN.KEYS
