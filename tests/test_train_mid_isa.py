"""Compiler budget of k_mid_grad (csrc/train.hip), read from the BUILT library's AMDGPU code-object metadata (tools/isa_report.py; no GPU,
no recompilation): the kernel is present, has no private segment (no scratch memory), spills neither vector nor scalar registers, and
its registers leave room for the one 4-wave workgroup per CU that its 100 KiB of dynamic LDS allows."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    return mod.kernels()


def test_k_mid_grad_has_no_scratch_and_no_spills(kernels):
    assert 'k_mid_grad' in kernels, sorted(kernels)
    k = kernels['k_mid_grad']
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256, k
    assert k['.vgpr_count'] + k['.agpr_count'] <= 512, k          # one wave per SIMD: the whole register file of a lane
    assert k['.group_segment_fixed_size'] == 0, k                 # its LDS is dynamic (102 656 bytes, set at launch)
