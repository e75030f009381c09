"""CPU tests of the epoch report's host side (efe_eval_stats; loss.eval_stats): the fp64 restatements of tests/eval_ref.py against their
sources (scipy.stats.spearmanr, daimc_amd.train.total_correlation, the reference's compare_reward expression), and the registration of
the entry point: header, ctypes binding, torch op and Python layout agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_ref
from conftest import ROOT


def factor_columns(r, n):
    """columns drawn like the game's true factors: 3, 6, 40, 32 and 32 values, and a uniform reward"""
    return [r.randint(0, k, n).astype(np.float32) for k in (3, 6, 40, 32, 32)] + [r.uniform(-1, 1, n).astype(np.float32)]


@pytest.mark.parametrize('n', [2, 3, 12, 257, 1000, 8192])
def test_spearman_is_scipys(n):
    stats = pytest.importorskip('scipy.stats')
    r = np.random.RandomState(n)
    cols = factor_columns(r, n)
    lat = r.randn(n).astype(np.float32)
    worst = 0.0
    for j, y in enumerate(cols + [lat[::-1].copy()]):
        for x in (lat, cols[(j + 1) % 6]):
            mine = eval_ref.spearman(x, y)
            with np.errstate(all='ignore'):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    ref = stats.spearmanr(x, y)[0]
            if np.isnan(ref):
                assert np.isnan(mine), (n, j)
                continue
            worst = max(worst, abs(mine - ref))
            assert abs(mine - ref) <= 1e-7, (n, j, mine, ref)
    print(f'n {n}: largest |rho - scipy| {worst:.3e}')


def test_spearman_edges():
    up = np.arange(7, dtype=np.float32)
    assert eval_ref.spearman(up, up * 2 + 1) == 1.0 and eval_ref.spearman(up, -up) == -1.0
    assert np.isnan(eval_ref.spearman(up, np.ones(7, np.float32)))                      # a constant column: 0 / 0
    assert np.isnan(eval_ref.spearman(up, np.where(up == 3, np.nan, up)))
    assert list(eval_ref.doubled_ranks([5.0, 1.0, 5.0, 2.0])) == [7, 2, 7, 4]             # ranks 3.5, 1, 3.5, 2


def test_total_correlation_is_the_trainers():
    from daimc_amd.train import total_correlation
    r = np.random.RandomState(3)
    for n in (12, 63, 1000):
        x = (r.randn(n, 10) @ r.randn(10, 10)).astype(np.float32)
        assert eval_ref.total_correlation(x) == total_correlation(x)
    x = np.random.RandomState(0).randn(12, 10).astype(np.float32)
    print('condition number of a seeded normal [12, 10] covariance:', eval_ref.covariance_condition(x))
    assert eval_ref.covariance_condition(x) < 1e6


def test_median_and_std():
    import torch
    r = np.random.RandomState(5)
    for n in (1, 2, 3, 8, 9):
        x = r.randint(0, 4, n).astype(np.float32)                                       # duplicates
        assert eval_ref.lower_median(x) == torch.tensor(x).median().item()
        t = torch.tensor(x).double().std().item()
        assert (np.isnan(t) and np.isnan(eval_ref.std(x))) or abs(t - eval_ref.std(x)) < 1e-12
    assert np.isnan(eval_ref.lower_median(np.array([1.0, np.nan, 0.0], np.float32)))


def test_compare_reward_nchw_is_the_reference_expression_on_nhwc():
    r = np.random.RandomState(1)
    o1, po1 = r.rand(5, 1, 64, 64).astype(np.float32), r.rand(5, 1, 64, 64).astype(np.float32)
    a, b = (np.transpose(t, (0, 2, 3, 1)).astype(np.float64) for t in (o1, po1))       # NHWC, as the reference holds its frames
    ref = np.square(a[:, 0:3, 0:64, :] - b[:, 0:3, 0:64, :]).mean(axis=(0, 1, 2, 3))     # src/util.py:84
    assert eval_ref.compare_reward(o1, po1) == ref


def test_registration():
    import daimc_amd
    from daimc_amd import _lib, loss
    txt = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    n = int(re.search(r'EFE_EVAL_STATS = (\d+)', txt).group(1))
    cap = int(re.search(r'EFE_EVAL_MAX_ROWS = (\d+)', txt).group(1))
    covered = sorted(i for s in loss.EVAL_STATS_FIELDS.values() for i in range(s.start, s.stop))
    assert covered == list(range(n)) and n == _lib.EFE_EVAL_STATS == eval_ref.STATS == 98 and cap == _lib.EFE_EVAL_MAX_ROWS == 8192
    fields = txt[txt.index('typedef struct efe_eval_in {'):txt.index('} efe_eval_in;')]
    assert tuple(re.findall(r'const float\* (\w+);', fields)) == _lib.EVAL_IN_FIELDS
    assert _lib.EVAL_IN_FIELDS[:10] == loss.EVAL_FE_ARRAYS == eval_ref.FE_ARRAYS and set(loss.EVAL_FE_ARRAYS) <= set(daimc_amd.FreeEnergy._fields)
    assert C.sizeof(_lib.EfeEvalIn) == 15 * 8 + 8
    assert 'efe_eval_stats' in _lib.EXPORTS and 'efe_abi_version' in _lib.EXPORTS and _lib.ABI_VERSION == 6
    schema = str(_lib.load_ops().eval_stats.default._schema)
    assert schema.startswith('efe::eval_stats(int ctx') and 'Tensor(a!) out' in schema
    from daimc_amd.train import EVAL_KEYS, REPORT_KEYS
    assert REPORT_KEYS == EVAL_KEYS + ('mse_r', 'spearman') and callable(daimc_amd.Trainer.report)
    for f in ('eval_stats', 'compare_reward', 'make_batch_dsprites_random', 'make_batch_dsprites_random_reward_transitions'):
        assert callable(getattr(daimc_amd, f)), f
    from daimc_amd import build as _build
    assert len(loss.EVAL_FACTORS) == 6 and 'csrc/eval.hip' in _build.SOURCES


def test_train_loop_has_the_report_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_loop', os.path.join(ROOT, 'tools', 'train_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parser().parse_args([]).report is False and mod.parser().parse_args(['--report']).report is True
