"""Compiler budget of the generic-geometry repack kernel (csrc/train_down_g.hip k_repack_down_g), read from the BUILT library's AMDGPU
code-object metadata (tools/isa_report.py; no GPU, no recompilation): the kernel is present, has no private segment (no scratch memory),
spills neither vector nor scalar registers, uses no LDS, and its vector-register count allows at least the occupancy k_repack_down has
(csrc/train_down.hip, which carries the fp64 Winograd / F(2,2) transforms the generic forms do not need)."""
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


def waves_per_simd(k):
    """gfx950: 512 unified vector registers per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    regs = (k['.vgpr_count'] + k.get('.agpr_count', 0) + 7) // 8 * 8
    return min(8, 512 // max(regs, 8))


def test_repack_down_g_exists_without_scratch_or_spills(kernels):
    assert 'k_repack_down_g' in kernels, sorted(k for k in kernels if 'down' in k)
    k = kernels['k_repack_down_g']
    print('k_repack_down_g', {f: k[f] for f in ('.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')})
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256 and k['.group_segment_fixed_size'] == 0, k


def test_repack_down_g_occupancy_is_at_least_repack_down_s(kernels):
    g, d = kernels['k_repack_down_g'], kernels['k_repack_down']
    print(f'k_repack_down_g: {g[".vgpr_count"]} VGPRs, {waves_per_simd(g)} waves per SIMD; k_repack_down: {d[".vgpr_count"]} VGPRs, '
          f'{waves_per_simd(d)} waves per SIMD')
    assert g['.vgpr_count'] <= d['.vgpr_count'] and waves_per_simd(g) >= waves_per_simd(d), (g, d)


def test_the_kernels_of_the_1x64x64_step_are_still_there(kernels):
    assert 'k_adam_down' in kernels and 'k_repack_down' in kernels
