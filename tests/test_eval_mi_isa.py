"""Compiler budget of the mutual-information kernels (csrc/eval_mi.hip), read from the BUILT library's AMDGPU code-object metadata
(tools/isa_report.py; no GPU, no recompilation): every kernel of the file is present, in every instantiation the launcher uses, has no
private segment (no scratch memory) and spills neither vector nor scalar registers; the sweep keeps one tile of 256 prepared points
(4 KiB) and its wave partials in LDS."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (workgroup size, LDS ceiling in bytes)
KERNELS = {'k_mi_cols': (256, 64), 'k_mi_finish': (64, 0),
           'k_mi_sweep<1>': (256, 8192), 'k_mi_sweep<2>': (256, 8192), 'k_mi_sweep<3>': (256, 8192), 'k_mi_sweep<4>': (256, 8192)}


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import __graft_entry__ as ge
    ge.build()
    return mod.kernels()


def test_every_kernel_of_the_file_is_listed():
    src = open(os.path.join(ROOT, 'deep-active-inference-mc_amd', 'csrc', 'eval_mi.hip')).read()
    names = re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(k_\w+)', src)
    assert sorted(names) == sorted({k.split('<')[0] for k in KERNELS})
    launched = re.findall(r'hipLaunchKernelGGL\((k_\w+(?:<\d>)?)', src)
    assert sorted(set(launched)) == sorted(KERNELS)


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_kernel_has_no_scratch_and_no_spills(kernels, name):
    assert name in kernels, sorted(k for k in kernels if 'k_mi' in k)
    k = kernels[name]
    print(name, {f: k[f] for f in ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')})
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    wg, lds = KERNELS[name]
    assert k['.max_flat_workgroup_size'] == wg and k['.group_segment_fixed_size'] <= lds, k
