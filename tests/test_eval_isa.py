"""Compiler budget of the epoch report's kernels (csrc/eval.hip), read from the BUILT library's AMDGPU code-object metadata
(tools/isa_report.py; no GPU, no recompilation): every kernel is present, has no private segment (no scratch memory), spills neither
vector nor scalar registers and keeps its LDS within 64 KiB: one staged column of 8192 floats plus the wave partials in the two counting
kernels."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> workgroup size
KERNELS = {'k_eval_means': 256, 'k_eval_median': 1024, 'k_eval_tc': 256, 'k_eval_rho': 1024}


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import __graft_entry__ as ge
    ge.build()
    return mod.kernels()


def test_every_kernel_of_the_file_is_listed():
    src = open(os.path.join(ROOT, 'deep-active-inference-mc_amd', 'csrc', 'eval.hip')).read()
    import re
    assert sorted(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(k_\w+)', src)) == sorted(KERNELS)


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_kernel_has_no_scratch_no_spills_and_fits_lds(kernels, name):
    assert name in kernels, sorted(k for k in kernels if 'eval' in k)
    k = kernels[name]
    print(name, {f: k[f] for f in ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')})
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == KERNELS[name] and k['.group_segment_fixed_size'] <= 65536, k
