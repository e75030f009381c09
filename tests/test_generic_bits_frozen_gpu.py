"""The geometry-generic kernels' outputs, frozen bit for bit.  tests/golden/generic_bits.npz was written by tools/make_generic_bits.py on the
build of the commit BEFORE k_convt_p / k_convt_12 and k_conv_e / k_conv_e12 were made to share one strip pass: that change leaves every
output element's operations and their order alone, so not one bit of G, its three terms, the stored images (compared by SHA-256) or the
encoder's s / mean / logvar may move -- under the default options, with ct_fuse12 = 0, with fuse_final_g = 0 (the only way k_convt_p<2, 8>
and, at resolution 32, k_convt_p<1, 8> run), with a row mask, and with enc_tiled = 2 and 1 -- on the six geometries of
tests/test_generic_geometry.py, the smallest set that hits every strip shape."""
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location('make_generic_bits', os.path.join(ROOT, 'tools', 'make_generic_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _cases(geometry):
    """one model and one pass over the option settings per geometry, shared by that geometry's cases (they run back to back)"""
    return _tool().run_cases(geometry)


@pytest.fixture(scope='module')
def frozen(golden):
    return golden('generic_bits')


@pytest.mark.gpu
@pytest.mark.parametrize('case', _tool().CASES)
@pytest.mark.parametrize('geometry', _tool().GEOMETRIES, ids=lambda g: 'a%dc%dr%d' % g)
def test_generic_outputs_keep_every_bit(frozen, geometry, case):
    tool = _tool()
    got_all = _cases(geometry)[case]
    names = tool.G_NAMES if case in tool.G_CASES else tool.E_NAMES
    assert sorted(got_all) == sorted(names)
    for n in names:
        want, got = frozen[tool.key(geometry, case, n)], got_all[n]
        assert got.dtype == want.dtype and got.shape == want.shape, (geometry, case, n, got.shape, want.shape)
        if n.endswith('sha256'):
            assert got.dtype == np.uint8 and got.shape == (32,) and np.array_equal(got, want), (geometry, case, n)
        else:
            assert got.dtype == np.float32
            gu, wu = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
            assert np.array_equal(gu, wu), (geometry, case, n, int((gu != wu).sum()), float(np.abs(got - want).max()))
