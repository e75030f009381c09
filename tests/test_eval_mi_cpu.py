"""CPU tests of the mutual-information table's host side (efe_eval_mi; loss.eval_mutual_info): the numpy restatement of
tests/eval_mi_ref.py against its source, scikit-learn's mutual_info_regression on float64 columns and its _compute_mi_cc on exactly tied
columns, in both orders of the sums; the engine's digamma table against scipy; and the registration of the entry point: header,
ctypes binding, torch op and the Python layers agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_mi_ref as R
from conftest import ROOT


def columns(M):
    """(name, latent column, factor column) of every pair compared at M rows: a normal latent and one that follows a factor against every
    factor column, a constant factor (the reward is usually all zero) and a constant (dead) latent"""
    r = np.random.RandomState(100 + M)
    fac = R.factor_columns(r, M)
    lat = r.randn(M).astype(np.float32)
    follow = (fac[2] + 0.01 * r.randn(M)).astype(np.float32)
    out = [(f'normal x f{j}', lat, f) for j, f in enumerate(fac)] + [(f'follow x f{j}', follow, f) for j, f in enumerate(fac)]
    out.append(('normal x constant factor', lat, np.zeros(M, np.float32)))
    out.append(('constant latent x f3', np.full(M, 0.25, np.float32), fac[3]))
    return out


@pytest.mark.parametrize('order', ['numpy', 'device'])
@pytest.mark.parametrize('M', [4, 5, 257, 1000])
def test_restatement_is_mutual_info_regression(M, order):
    fs = pytest.importorskip('sklearn.feature_selection')
    worst = 0.0
    for k in (1, 3):
        for seed, (name, x, y) in enumerate(columns(M)):
            g = np.random.RandomState(seed)
            nx, ny = g.standard_normal((M, 1))[:, 0], g.standard_normal(M)
            mine = R.pair(x, y, nx, ny, (k,), order)[k][0]
            ref = fs.mutual_info_regression(x.astype(np.float64).reshape(-1, 1), y.astype(np.float64), n_neighbors=k,
                                            random_state=np.random.RandomState(seed))[0]
            worst = max(worst, abs(mine - ref))
            assert abs(mine - ref) <= 1e-12, (M, k, name, mine, ref)
    print(f'M {M} order {order}: largest |MI - sklearn| {worst:.3e}')


@pytest.mark.parametrize('M', [4, 5, 7, 64, 65, 257, 1025])
def test_exact_ties_are_compute_mi_cc(M):
    mi = pytest.importorskip('sklearn.feature_selection._mutual_info')
    r = np.random.RandomState(M)
    worst = 0.0
    for name, x, y in (('integers', r.randint(0, 3, M), r.randint(0, 6, M)), ('constant y', r.randint(0, 40, M), np.zeros(M)),
                       ('identical', r.randint(0, 5, M), None), ('all constant', np.ones(M), np.ones(M))):
        x = x.astype(np.float64)
        y = x.copy() if y is None else y.astype(np.float64)
        ks = tuple(k for k in (1, 2, 3, 4) if k < M)
        cnt = R.neighbour_counts(x, y, ks)
        for k in ks:
            mine = R.mi_from_counts(cnt[k][0], cnt[k][1], M, k)
            ref = mi._compute_mi_cc(x, y, k)
            worst = max(worst, abs(mine - ref))
            assert abs(mine - ref) <= 1e-12, (M, k, name, mine, ref)
    print(f'M {M}: largest |MI - _compute_mi_cc| on tied columns {worst:.3e}')


def test_psi_is_scipys_digamma():
    sp = pytest.importorskip('scipy.special')
    n = np.arange(1, 8194)
    err = np.abs(R.psi(n) - sp.digamma(n.astype(np.float64)))
    print(f'largest |psi - digamma| on 1 .. 8193: {err.max():.3e} at n = {n[err.argmax()]}')
    assert err.max() <= 1e-13


def test_device_order_sum():
    """the replay is the contract: thread t adds t, t + 256, ...; butterfly; ((w0 + w1) + w2) + w3"""
    r = np.random.RandomState(0)
    for n in (1, 63, 256, 257, 1000):
        v = r.randn(n) * 10.0 ** r.uniform(-3, 3, n)
        acc = [0.0] * 256
        for i, e in enumerate(v):
            acc[i % 256] = acc[i % 256] + float(e)
        for off in (32, 16, 8, 4, 2, 1):
            acc = [acc[t] + acc[t ^ off] for t in range(256)]
        assert R.device_sum(v) == ((acc[0] + acc[64]) + acc[128]) + acc[192]
        assert abs(R.device_sum(v) - R.numpy_sum(v)) <= 1e-12 * np.abs(v).sum()


def test_registration():
    import daimc_amd
    from daimc_amd import _lib, loss
    from daimc_amd import build as _build
    txt = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    assert int(re.search(r'EFE_EVAL_MI = (\d+)', txt).group(1)) == _lib.EFE_EVAL_MI == R.PAIRS == 60
    assert int(re.search(r'EFE_EVAL_MI_MAX_NEIGHBORS = (\d+)', txt).group(1)) == _lib.EFE_EVAL_MI_MAX_NEIGHBORS == 4
    fields = txt[txt.index('typedef struct efe_eval_mi_in {'):txt.index('} efe_eval_mi_in;')]
    assert tuple(re.findall(r'(?:const float\*|const double\*|int|uint64_t|uint32_t) (\w+);', fields)) == _lib.EVAL_MI_IN_FIELDS
    assert tuple(f for f, _ in _lib.EfeEvalMiIn._fields_) == _lib.EVAL_MI_IN_FIELDS
    assert C.sizeof(_lib.EfeEvalMiIn) == 3 * 8 + 8 + 8 + 8          # three pointers, int + padding, uint64, uint32 + padding
    assert _lib.EfeEvalMiIn.seed.offset == 32 and _lib.EfeEvalMiIn.stage.offset == 40
    assert 'efe_eval_mi' in _lib.EXPORTS and _lib.ABI_VERSION == 6 and _lib.load().efe_abi_version() == 6
    assert hasattr(_lib.load(), 'efe_eval_mi')
    schema = str(_lib.load_ops().eval_mi.default._schema)
    assert schema.startswith('efe::eval_mi(int ctx, Tensor s0, Tensor S_real, Tensor? noise, int n_neighbors, int seed, int stage')
    assert 'Tensor(a!) out' in schema and 'Tensor(b!)? counts' in schema
    assert callable(daimc_amd.eval_mutual_info) and daimc_amd.eval_mutual_info is loss.eval_mutual_info
    from daimc_amd.train import EVAL_KEYS, REPORT_KEYS
    assert 'mutual_info' not in REPORT_KEYS and REPORT_KEYS == EVAL_KEYS + ('mse_r', 'spearman')
    import inspect
    assert inspect.signature(daimc_amd.Trainer.report).parameters['mutual_info'].default is False
    sig = inspect.signature(loss.eval_mutual_info).parameters
    assert [sig[k].default for k in ('n_neighbors', 'noise', 'seed', 'stage', 'out', 'counts', 'engine')] == [3, None, 0, 0, None, None, None]
    assert 'csrc/eval_mi.hip' in _build.SOURCES
    philox = open(os.path.join(ROOT, 'deep-active-inference-mc_amd', 'csrc', 'philox.h')).read()
    assert re.search(r'TAG_MI = 0x80', philox)


def test_train_loop_has_the_report_mi_flag():
    import importlib.util
    spec = importlib.util.spec_from_file_location('train_loop', os.path.join(ROOT, 'tools', 'train_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.parser()
    assert p.parse_args([]).report_mi is False and p.parse_args(['--report-mi']).report_mi is True
    assert p.parse_args(['--report']).report_mi is False and p.parse_args(['--report']).report is True
