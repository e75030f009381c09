"""CPU tests of the training-side free energy: the test-side restatement (tests/free_energy_ref.py on oracle/efe_oracle.py) reproduces
the fixtures captured from the shimmed reference (tools/make_golden_free_energy.py -> tests/golden/free_energy_*.npz) bit for bit in
fp32, its gamma branches agree with torch's at the fp32 boundaries, and the library's export list matches the header."""
import json
import os
import re

import numpy as np
import pytest
import torch

import free_energy_ref as FR
from conftest import ROOT, load_golden
from oracle import synth
from oracle import efe_oracle as EO

FIXTURES = ['free_energy_g100', 'free_energy_g135', 'free_energy_sparse']


def weights_of(meta):
    return synth.stress_weights(meta['family']) if meta['family'] else synth.make_weights(int(meta['wseed']), float(meta['gain']))


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_reproduces_reference_fixture_bit_for_bit(name):
    g = load_golden(name)
    meta = json.loads(str(g['meta']))
    orc = EO.OracleModel(weights_of(meta), EO.PhiloxNoise(int(meta['nseed'])))
    kw = dict(beta_s=meta['beta_s'], beta_o=meta['beta_o'], stage=meta['stage'], ro=meta['row_offset'])
    with torch.no_grad():
        r = FR.free_energy(orc, g['o0'], g['o1'], g['pi0'], g['log_Ppi'], meta['gamma'], **kw)
        for k in FR.FIELDS:
            np.testing.assert_array_equal(r[k].numpy().reshape(g[k].shape), g[k], err_msg=k)
        for i, gam in enumerate(meta['gammas']):
            F = FR.loss_down_F(-r['nlogpo1'], r['kl_s'], r['kl_naive'], gam, meta['beta_s'], meta['beta_o'], torch.float32)
            np.testing.assert_array_equal(F.numpy(), g['F_down_g'][i], err_msg=f'gamma {gam}')
        sc = FR.free_energy(orc, g['o0'], g['o1'], g['pi0'], g['log_Ppi'], meta['gamma'], omega=meta['omega_scalar'], **kw)
        np.testing.assert_array_equal(sc['F_mid'].numpy(), g['F_mid_sc'])
        np.testing.assert_array_equal(sc['F_down'].numpy(), g['F_down_sc'])
    # the fixture pins all three branches of the gamma test
    assert {FR.gamma_branch(x) for x in meta['gammas']} == {'naive', 'prior', 'mixture'}


def test_fixtures_are_small():
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', name + '.npz')) < 512 * 1024


@pytest.mark.parametrize('gamma', [np.float32(0.05), np.float32(0.95), np.nextafter(np.float32(0.05), np.float32(1)),
                                   np.nextafter(np.float32(0.95), np.float32(0)), 0.0, 0.5, 1.0])
def test_gamma_branch_matches_torch_fp32(gamma):
    """torch compares an fp32 0-d tensor with a Python float in fp32: float32(0.05) <= 0.05 holds there, although it does not in double"""
    g = torch.tensor(float(gamma), dtype=torch.float32)
    want = 'naive' if bool(g <= 0.05) else 'prior' if bool(g >= 0.95) else 'mixture'
    assert FR.gamma_branch(float(gamma)) == want
    if gamma == np.float32(0.05):
        assert want == 'naive' and not (float(gamma) <= 0.05)
    if gamma == np.float32(0.95):
        assert want == 'prior'


def test_free_energy_exports_match_header():
    from daimc_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = sorted(set(re.findall(r'\b(efe_[a-z_0-9]+)\s*\(', txt)))
    assert sorted(_lib.EXPORTS) == declared
    for n in ('efe_free_energy', 'efe_loss_top', 'efe_loss_mid', 'efe_loss_down'):
        assert n in _lib.EXPORTS
    # the efe_fe_out field order is the one the ctypes mirror and the torch op return
    body = re.search(r'typedef struct efe_fe_out \{(.*?)\} efe_fe_out;', txt, flags=re.S).group(1)
    assert tuple(re.findall(r'float\*\s*(\w+)', body)) == _lib.FE_OUT_FIELDS == FR.FIELDS


def test_loss_module_keeps_reference_names():
    import daimc_amd
    for n in ('compute_omega', 'compute_kl_div_pi', 'compute_loss_top', 'compute_loss_mid', 'compute_loss_down', 'free_energy'):
        assert callable(getattr(daimc_amd.loss, n))
    assert daimc_amd.free_energy is daimc_amd.loss.free_energy
    assert daimc_amd.FreeEnergy._fields == FR.FIELDS
    # compute_omega accepts what train.py hands it (a numpy array) and computes in fp32
    kl = np.array([0.5, 25.0, 80.0], dtype=np.float32)
    w = daimc_amd.loss.compute_omega(kl, *FR.OMEGA_PARAMS)
    assert w.dtype == torch.float32
    np.testing.assert_array_equal(w.numpy(), FR.compute_omega(torch.from_numpy(kl), *FR.OMEGA_PARAMS).numpy())
