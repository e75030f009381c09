"""CPU tests of the training loop's host side: the command line of tools/train_loop.py (its defaults are the reference train.py's), the
gamma schedule helper of daimc_amd.train (train.py:101-102 in the reference's fp32 arithmetic), total_correlation, and the binding of
efe_train_step."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT


def tool():
    spec = importlib.util.spec_from_file_location('train_loop', os.path.join(ROOT, 'tools', 'train_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_loop.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-400:]
    for flag in ('--batch', '--epochs', '--rounds', '--resume', '--folder', '--sprites'):
        assert flag in r.stdout, flag


def test_defaults_are_the_reference_train_py():
    """train.py:20, 29-49: batch 50, ROUNDS 1000, epochs 1000, TEST_SIZE 1000, the three learning rates, the gamma schedule, the planner"""
    a = tool().parser().parse_args([])
    assert (a.batch, a.rounds, a.epochs, a.test_size, a.resume, a.sprites) == (50, 1000, 1000, 1000, False, None)
    a = tool().parser().parse_args(['-r', '-b', '8', '--rounds', '3', '--folder', 'x', '--sprites', 'd.npz'])
    assert (a.batch, a.rounds, a.resume, a.folder, a.sprites) == (8, 3, True, 'x', 'd.npz')
    from daimc_amd.train import DEFAULTS as D
    import daimc_amd
    assert (D['lr_top'], D['lr_mid'], D['lr_down']) == (1e-4, 1e-4, 1e-3)
    assert (D['gamma_rate'], D['gamma_max'], D['gamma_delay'], D['deepness'], D['samples'], D['repeats']) == (0.01, 0.8, 30, 1, 1, 5)
    assert daimc_amd.loss.OMEGA_PARAMS == (1.0, 25.0, 5.0, 1.5)
    import inspect
    sig = inspect.signature(daimc_amd.Trainer.__init__).parameters
    for k in ('lr_top', 'lr_mid', 'lr_down', 'deepness', 'samples', 'repeats', 'gamma_rate', 'gamma_max', 'gamma_delay'):
        assert sig[k].default == D[k], k
    assert sig['calc_mean'].default is True


def test_epoch_line_is_the_reference_format():
    st = {'F': 1234.567, 'mse_o': 0.12345, 'kl_div_s': 3.14159, 'omega': 2.4933, 'omega_std': 0.001, 'kl_div_pi': 0.5, 'TC': 1.005}
    assert tool().epoch_line(7, st, 12.345) == '7, F: 1234.57, MSEo: 0.123, KLs: 3.14, omega: 2.49+-0.00, KLpi: 0.50, TC: 1.00, dur. 12.35s'


def test_gamma_schedule_is_the_reference_fp32_loop():
    from daimc_amd.train import gamma_at, next_gamma
    g = torch.tensor(0.0)
    mine = 0.0
    for epoch in range(1, 201):
        if epoch > 30 and g < 0.8:                    # train.py:101-102 on a float32 tensor
            g += 0.01
        mine = next_gamma(mine, epoch)
        assert mine == g.item(), epoch
        if epoch in (30, 31, 200):
            assert gamma_at(epoch) == mine
    assert gamma_at(30) == 0.0 and gamma_at(31) == float(np.float32(0.01)) and gamma_at(200) == gamma_at(150)
    assert next_gamma(0.3, 50, gamma_rate=0.1, gamma_max=0.35, gamma_delay=50) == float(np.float32(0.3))      # not past the delay (the value is the fp32 tensor's)


def test_total_correlation():
    from daimc_amd.train import total_correlation
    r = np.random.RandomState(0)
    x = r.randn(4000, 3)
    assert abs(total_correlation(x)) < 5e-3                         # independent columns
    x[:, 1] = x[:, 0] + 0.1 * x[:, 1]
    rho2 = 1.0 / 1.01
    assert abs(total_correlation(x) - (-0.5 * np.log(1.0 - rho2))) < 0.05


def test_step_structs_match_the_header():
    from daimc_amd import _lib
    assert C.sizeof(_lib.EfeStepIn) == 40 and C.sizeof(_lib.EfeStepOut) == 88 and C.sizeof(_lib.EfeStepAdam) == 16 + C.sizeof(_lib.EfeAdamParams) == 56
    assert _lib.EFE_STEP_MEANS == len(_lib.STEP_MEANS_FIELDS) == 8
    txt = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    assert 'enum { EFE_STEP_MEANS = 8 };' in txt
    fields = txt[txt.index('typedef struct efe_step_out {'):txt.index('} efe_step_out;')]
    import re
    assert tuple(re.findall(r'float\* (\w+)', fields)) == _lib.STEP_OUT_FIELDS
    import daimc_amd
    assert daimc_amd.TrainStep._fields == _lib.STEP_OUT_FIELDS and callable(daimc_amd.train_step)
    schema = str(_lib.load_ops().train_step.default._schema)
    assert schema.startswith('efe::train_step(int ctx, Tensor o0, Tensor o1') and 'Tensor(g!) means' in schema
