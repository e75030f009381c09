"""Compiler budget of the encoder's training kernels (csrc/train_enc.hip), read from the BUILT library's AMDGPU code-object metadata
(tools/isa_report.py; no GPU, no recompilation): every kernel is present, has no private segment (no scratch memory), spills neither
vector nor scalar registers and keeps the static LDS its file states, below 64 KiB."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ('32, 32, 31', '32, 64, 15', '64, 64, 7')          # <CI, CO, HIN> of layers 2, 3, 4
LDS = {'k_enc_conv1': 0, 'k_ench_fwd': 3 * 16 * 260 * 4, 'k_ench_bwd': (16 * 36 + 16 * 260 + 16 * 580) * 4, 'k_enc_w1': 16, 'k_conv_bias': 16,
       'k_down_latent': 0}
LDS.update({f'{k}<{s}>': 0 for k in ('k_enc_conv', 'k_enc_wgrad', 'k_enc_dx') for s in SHAPES})


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
    assert name in kernels, sorted(k for k in kernels if 'k_enc' in k or 'k_down' in k)
    k = kernels[name]
    assert k['.private_segment_fixed_size'] == 0 and k['.vgpr_spill_count'] == 0 and k['.sgpr_spill_count'] == 0, k
    assert k['.max_flat_workgroup_size'] == 256, k
    assert k['.vgpr_count'] <= 512, k                     # (the unified count, accumulation registers included)
    assert k['.group_segment_fixed_size'] == LDS[name] <= 64 * 1024, k
