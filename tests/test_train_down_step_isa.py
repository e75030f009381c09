"""Compiler budget of ModelDown's optimiser-step kernels (csrc/train_down.hip), read from the BUILT library's AMDGPU code-object metadata
(tools/isa_report.py; no GPU, no recompilation): both kernels are present, have no private segment (no scratch memory), spill neither
vector nor scalar registers and use no LDS, as the file states."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS = {'k_adam_down': 0, 'k_repack_down': 0}


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    return mod.kernels()


@pytest.mark.parametrize('name', sorted(LDS))
def test_kernel_has_no_scratch_and_no_spills(kernels, name):
    assert name in kernels, sorted(k for k in kernels if 'down' in k)
    k = kernels[name]
    print(name, {f: k[f] for f in ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')})
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256, k
    assert k['.vgpr_count'] <= 128, k                     # a gather and an element-wise update: a quarter of the register file at most
    assert k['.group_segment_fixed_size'] == LDS[name] <= 64 * 1024, k
