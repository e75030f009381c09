"""Compiler budget of the encoder's run-time-geometry training kernels (csrc/train_enc_g.hip), read from the BUILT library's AMDGPU
code-object metadata (tools/isa_report.py; no GPU, no recompilation): every kernel is present, has no private segment (no scratch memory),
spills neither vector nor scalar registers, runs workgroups of 256 and keeps its LDS static and below 64 KiB; and the list is complete."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONVS = ('<32, 32>', '<32, 64>', '<64, 64>')
LDS = {'k_encg_conv1': 0, 'k_encg_w1': 16, 'k_enchg_fc0': 0, 'k_enchg_join': 0, 'k_enchg_fwd': 49920, 'k_enchg_small': 35584, 'k_enchg_w9grad': 0,
       'k_enchg_dy4': 0}
LDS.update({f'{k}{t}': 0 for k in ('k_encg_conv', 'k_encg_wgrad', 'k_encg_dx') for t in CONVS})


@pytest.fixture(scope='module')
def kernels():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.exists(mod.DEFAULT_LIB), 'engine library not built'
    return mod.kernels()


@pytest.mark.parametrize('name', sorted(LDS))
def test_kernel_has_no_scratch_and_no_spills(kernels, name):
    assert name in kernels, sorted(k for k in kernels if 'encg' in k or 'enchg' in k)
    k = kernels[name]
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256, k
    assert k['.vgpr_count'] <= 512, k                     # (the unified count, accumulation registers included)
    assert k['.group_segment_fixed_size'] == LDS[name] <= 64 * 1024, k


def test_the_list_is_complete(kernels):
    assert sorted(k for k in kernels if 'encg' in k or 'enchg' in k) == sorted(LDS)
