"""k_dec_ab's outputs (and those of the small-launch pair k_dec_a_s, k_dec_b4<4>) held to every bit of the build BEFORE layer 1's output
transform moved under the next xi's MFMAs (two accumulators in wino_l1) and the fused kernel's layer-2 temporaries moved a step later:
both changes leave every output element's operations and their order alone.  tests/golden/decoder_ab_bits_r13.npz was written by
tools/make_decoder_ab_bits.py on that parent build (e1a555a); tests/test_decoder_fused_ab_gpu.py cannot see such a change, as it compares two
forms of one tree that share wino_l1 and f22_l2.

Cases (the tool's docstring has the shapes): 132 images, the smallest launch k_dec_ab takes, with one workgroup per image and with
dec_ab_grid = 3 (44 images per workgroup, so a deferred transform or temporary could leak across an image boundary); the entropy and the
reward mode (a rollout has both); a row mask [1,1,0,1,0] x 3 (a dead image between live ones must neither retire nor drop what a live
one left pending); a 4-row call on the small-launch kernels (the NR = 1 form of wino_l1); the fixture weights and the high-gain family.
The comparison is == on the bit patterns, so NaN positions count too."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('make_decoder_ab_bits', os.path.join(ROOT, 'tools', 'make_decoder_ab_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
RUNS = [(c, g) for c in ('roll', 'mask') for g in TOOL.GRIDS] + [('small', 0)]


@pytest.fixture(scope='module')
def models():
    cache = {}

    def get(wname):
        if wname not in cache:
            cache[wname] = TOOL.make_model(wname)
        return cache[wname]
    return get


@pytest.fixture(scope='module')
def frozen(golden):
    return golden('decoder_ab_bits_r13')


@pytest.mark.gpu
@pytest.mark.parametrize('case,grid', RUNS, ids=[f'{c}_grid{g}' for c, g in RUNS])
@pytest.mark.parametrize('wname', TOOL.WEIGHTS)
def test_outputs_keep_every_bit_of_the_parent_build(models, frozen, wname, case, grid):
    got = TOOL.run_case(models(wname), case, grid)
    want = {n[len(f'{wname}_{case}_'):]: frozen[n] for n in frozen if n.startswith(f'{wname}_{case}_')}
    assert sorted(got) == sorted(want) and len(want) >= 5, (sorted(got), sorted(want))
    for n in sorted(want):
        assert want[n].dtype == np.uint32 and got[n].dtype == np.uint32 and got[n].shape == want[n].shape, (n, got[n].shape, want[n].shape)
        assert np.array_equal(got[n], want[n]), (wname, case, grid, n, int((got[n] != want[n]).sum()), 'of', got[n].size, 'words differ')
