"""Compiler budget of the kernels that record an agent run (csrc/agent_trace.hip), read from the BUILT library's AMDGPU code-object
metadata (tools/isa_report.py; no GPU, no recompilation): all four are present, have no private segment (no scratch memory) and spill
neither vector nor scalar registers; k_agent_plan_mask keeps its 1024 int32 counters (4096 B) and the one word of its max-reduction in
LDS.  The workgroup sizes are the launch bounds the launchers use; the register ceilings are the compiled counts (14, 25, 19, 12 VGPRs
and 30, 43, 52, 25 SGPRs) rounded up to the next allocation granule of 8 and 16."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (LDS bytes, workgroup size, VGPR ceiling, SGPR ceiling)
KERNELS = {'k_agent_trace_tick': (0, 128, 16, 32), 'k_agent_trace_decision': (0, 128, 32, 48), 'k_agent_plan_mask': (4096 + 4, 256, 24, 64),
           'k_agent_view': (0, 256, 16, 32)}


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
    assert name in kernels, sorted(k for k in kernels if 'agent' in k)
    k = kernels[name]
    print(name, {f: k[f] for f in ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')})
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    lds, wg, vgprs, sgprs = KERNELS[name]
    assert k['.max_flat_workgroup_size'] == wg and k['.group_segment_fixed_size'] == lds, k
    assert k['.vgpr_count'] <= vgprs and k['.sgpr_count'] <= sgprs, k
