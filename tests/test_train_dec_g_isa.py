"""Compiler budget of the run-time-geometry decoder tail kernels (csrc/train_dec_g.hip), read from the BUILT library's AMDGPU code-object
metadata (tools/isa_report.py; no GPU, no recompilation): every kernel is present, has no private segment (no scratch memory), spills
neither vector nor scalar registers, and is built for workgroups of 256."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = ['1, 64, 64', '2, 64, 64', '2, 64, 32', '1, 64, 32']           # (stride, Cin, Cout): layers 1, 2, 3 and layer 3 at resolution 32
TAP = [f'k_dectg_tap<{p}, {b}>' for p in PAIRS for b in ('false', 'true')]
WGRAD = [f'k_dectg_wgrad<{p}>' for p in PAIRS]
VALU = ['k_dectg_out', 'k_dectg_loss', 'k_dectg_dx4<1>', 'k_dectg_dx4<2>', 'k_dectg_dx4<3>', 'k_dectg_w4']


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
    assert name in kernels, sorted(k for k in kernels if 'dectg' in k)
    k = kernels[name]
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256, k
    assert k['.vgpr_count'] <= 512, k                     # (the unified count, accumulation registers included)
    assert k['.group_segment_fixed_size'] <= 16, k        # at most the four wave sums of a block reduction


def test_no_other_kernel_of_the_file_is_unlisted(kernels):
    assert sorted(k for k in kernels if 'dectg' in k) == sorted(TAP + WGRAD + VALU)
