"""Compiler budget of the two kernels at the ends of an mcts decision (csrc/agent_mcts.hip), read from the BUILT library's AMDGPU
code-object metadata (tools/isa_report.py; no GPU, no recompilation): both are present, have no private segment (no scratch memory -- the
walk trims while it walks and keeps no per-thread path array) and spill neither vector nor scalar registers; no LDS.  The workgroup size is
the launch bound the launchers use."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (LDS bytes, workgroup size, VGPR ceiling)
KERNELS = {'k_agent_mcts_root': (0, 128, 64), 'k_agent_mcts_enqueue': (0, 128, 64)}


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
    # one thread per deciding slot and a handful of scalars each (as the kernels of csrc/agent.hip: tests/test_agent_isa.py)
    assert k['.vgpr_count'] <= vgprs, k
