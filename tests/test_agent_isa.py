"""Compiler budget of the agent loop's kernels (csrc/agent.hip) and of the id-aware root post-processing (csrc/kernels.hip:
k_root_post_rows), read from the BUILT library's AMDGPU code-object metadata (tools/isa_report.py; no GPU, no recompilation): all are
present, have no private segment (no scratch memory) and spill neither vector nor scalar registers; k_agent_need keeps its sixteen wave
totals in 64 bytes of LDS.  The workgroup sizes are the launch bounds the launchers use."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (LDS bytes, workgroup size, VGPR ceiling)
KERNELS = {'k_agent_need': (64, 1024, 64), 'k_agent_choose': (0, 128, 64), 'k_agent_enqueue': (0, 128, 64), 'k_agent_act': (0, 128, 64),
           'k_root_post_rows': (0, 256, 64)}


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
    lds, wg, vgprs = KERNELS[name]
    assert k['.max_flat_workgroup_size'] == wg and k['.group_segment_fixed_size'] == lds, k
    # one thread per game and a handful of scalars each; k_agent_need's 1024-thread workgroup may use at most 64 VGPRs per thread at all
    assert k['.vgpr_count'] <= vgprs, k
