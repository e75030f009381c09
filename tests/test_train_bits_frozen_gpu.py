"""The training kernels' outputs, frozen bit for bit.  tests/golden/train_bits.npz was written by tools/make_train_bits.py on the build of
the commit BEFORE csrc/train_mlp.h existed: the k_dech_* kernels were rebuilt of its passes, k_top_grad and k_mid_grad took its mfma4, and the
two decoder-gradient entry points were merged on the host.  That change leaves every sum's operands and order alone, so not one bit of a loss,
a stored activation, a gradient, an updated weight or an Adam moment may move.  The shapes are the smallest that still reach a partial
tile, a second workgroup, a second tile of one workgroup (the add path of the slabs), the padded pi_dim 3 geometry, a second 64-row group
of the decoder and the decoder tail without its head (tools/make_train_bits.py lists them).  Arrays above 16 384 elements are held by the
SHA-256 of their bytes and by every 4 099th element; the decoder's gradient is held per state_dict key.
The enc_*, down_m17 and step_m257 cases were written on the build of the commit BEFORE csrc/block_sum.h and csrc/train_conv.h existed
(every older entry came out of that run array-equal): they hold the encoder's gradient and stored activations at one slab, at 32 slabs
with a second image in slab 0 and at a second row group, grad_down's composition (k_fe_down beside k_dect_loss, both gradients in one
array), and one whole training step with k_step_means' eight statistics and every trained weight and Adam moment."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('make_train_bits', os.path.join(ROOT, 'tools', 'make_train_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope='module')
def cases():
    return TOOL.run_cases()


@pytest.fixture(scope='module')
def frozen(golden):
    return golden('train_bits')


def test_fixture_stays_small_and_complete(frozen):
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'train_bits.npz')) <= TOOL.MAX_BYTES
    assert {k.split('.')[0] for k in frozen} == set(TOOL.CASES)
    assert all(v.size <= TOOL.WHOLE or k.endswith('.every4099') for k, v in frozen.items())


@pytest.mark.gpu
@pytest.mark.parametrize('case', TOOL.CASES)
def test_training_outputs_keep_every_bit(cases, frozen, case):
    got = TOOL.pack({case: cases[case]})
    want = {k: v for k, v in frozen.items() if k.startswith(case + '.')}
    assert want and sorted(got) == sorted(want), (case, sorted(set(got) ^ set(want)))
    for k in sorted(want, key=lambda k: (k.endswith('.sha256'), k)):          # (samples before digests: they say where and by how much)
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (k, int((g.view(np.uint32) != w.view(np.uint32)).sum()),
                                                                          float(np.abs(g - w).max()))
        else:
            assert np.array_equal(g, w), (k, 'the digest of the whole array differs')
