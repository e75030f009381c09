"""Compiler budget of the training step's two kernels (csrc/loss.hip: k_step_omega, k_step_means), read from the BUILT library's AMDGPU
code-object metadata (tools/isa_report.py; no GPU, no recompilation): both are present, have no private segment (no scratch memory) and
spill neither vector nor scalar registers; k_step_means keeps its four wave sums in 16 bytes of LDS."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (LDS bytes, workgroup size)
KERNELS = {'k_step_omega': (0, 128), 'k_step_means': (16, 256)}


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import __graft_entry__ as ge
    ge.build()
    return mod.kernels()


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_kernel_has_no_scratch_and_no_spills(kernels, name):
    assert name in kernels, sorted(k for k in kernels if 'step' in k)
    k = kernels[name]
    print(name, {f: k[f] for f in ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')})
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    lds, wg = KERNELS[name]
    assert k['.max_flat_workgroup_size'] == wg and k['.group_segment_fixed_size'] == lds, k
    assert k['.vgpr_count'] <= 64, k                      # a per-row expression and a strided sum: an eighth of the register file at most
