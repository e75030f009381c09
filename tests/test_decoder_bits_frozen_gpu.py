"""The decoder kernels' outputs, frozen bit for bit.  tests/golden/decoder_bits_r11.npz was written by tools/make_decoder_bits.py on the
build of the commit BEFORE k_dec_b4's strip staging and its single-lane adds changed: those changes leave every
output element's operations and their order alone, so not one bit of G, its three terms or the stored images may move -- in the
large-launch kernels (k_fc4<2>, k_dec_a, k_dec_b4<1>), the small-launch forms (k_dec_a_s, k_dec_b4<4>), the dead-row schedule and a rollout.
The shapes are the smallest that still hit the first and last strip, the halo row below the image, the zero column and both launch forms."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('make_decoder_bits', os.path.join(ROOT, 'tools', 'make_decoder_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def cases():
    return _tool().run_cases()


@pytest.fixture(scope='module')
def frozen(golden):
    return golden('decoder_bits_r11')


# case -> (prefix of its arrays in the fixture, rows of them the case holds)
CASES = {'i': ('g', None), 'ii': ('g', None), 'iii': ('g', [0, 3]), 'iv': ('r', None)}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_decoder_outputs_keep_every_bit(cases, frozen, case):
    tool = _tool()
    prefix, rows = CASES[case]
    assert rows is None or tuple(rows) == tuple(tool.LIVE)
    for n in tool.NAMES:
        want = frozen[f'{prefix}_{n}']
        want = want if rows is None else want[rows]
        got = cases[case][n]
        assert got.dtype == np.float32 and got.shape == want.shape, (case, n, got.shape, want.shape)
        assert np.array_equal(got, want), (case, n, int((got != want).sum()), float(np.abs(got - want).max()))
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (case, n)
