"""Compiler budget of the decoder tail's backward kernels (csrc/train_dec.hip), read from the BUILT library's AMDGPU code-object metadata
(tools/isa_report.py; no GPU, no recompilation): every kernel is present, has no private segment (no scratch memory) and spills neither
vector nor scalar registers."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAP = ['k_dect_tap<1, 64, 64, 16, false>', 'k_dect_tap<2, 64, 64, 16, false>', 'k_dect_tap<2, 64, 32, 32, false>',
       'k_dect_tap<1, 64, 64, 16, true>', 'k_dect_tap<2, 64, 64, 16, true>', 'k_dect_tap<2, 64, 32, 32, true>']
WGRAD = ['k_dect_wgrad<1, 64, 64, 16>', 'k_dect_wgrad<2, 64, 64, 16>', 'k_dect_wgrad<2, 64, 32, 32>']
VALU = ['k_dect_out', 'k_dect_loss', 'k_dect_dx4', 'k_dect_w4', 'k_conv_bias']


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    return mod.kernels()


@pytest.mark.parametrize('name', TAP + WGRAD + VALU)
def test_kernel_has_no_scratch_and_no_spills(kernels, name):
    assert name in kernels, sorted(k for k in kernels if 'dect' in k)
    k = kernels[name]
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256, k
    assert k['.vgpr_count'] <= 512, k                     # (the unified count, accumulation registers included)
    assert k['.group_segment_fixed_size'] <= 16, k        # at most the four wave sums of a block reduction
