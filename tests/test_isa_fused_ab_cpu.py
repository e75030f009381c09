"""Resource budget of k_dec_ab, the decoder tail as one persistent launch (option dec_fuse_ab), read from the code-object metadata and the
disassembly of the BUILT library (tools/isa_report.py, as tests/test_isa_strip_overhead_cpu.py does; no GPU, no recompilation).

Two workgroups of 256 threads share a CU, so a wave has 256 VGPRs and the workgroup 80 KiB of LDS; scratch or spilled registers inside
the image loop would put memory traffic (and, for spill reloads, s_waitcnt vmcnt(0) behind every outstanding y2 store) into both bodies.
The kernel's LDS is all static (the launch passes none): the metadata's figure is held against the constant DAB_LDS_BYTES of csrc/decoder.hip,
evaluated here from the source's own constant expressions.  The code of the two bodies together must stay inside the 64 KiB instruction cache two CUs share.

                     VGPRs   scratch   spilled VGPRs   spilled SGPRs   LDS bytes   code bytes
  k_dec_a             244       0            0               0           74 784      30 344
  k_dec_b4<1>         176       0            0               0           76 768      13 568
  k_dec_ab            252       0            0               0           79 024      43 620      (the build that added it)

Each body uses about a hundred SGPRs on its own (k_dec_a 98, k_dec_b4<1> 106), so a scalar of the one kept through the other is a spilled
SGPR: the first form of the kernel spilled 86.  What brought it to none: the kernel arguments are read again per image (karg_reload: 31),
the LDS is static so that every region's address is a constant of the instruction, and the uniform values that live through an image with
a few uses -- the image schedule, the slot's address, the kernel-argument address, body b's mode, store pointers and reward switch -- are
parked in vector registers and read back as scalars where they are used (vpark / vscalar).
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'deep-active-inference-mc_amd', 'csrc', 'decoder.hip')
KERNEL = 'k_dec_ab'


@pytest.fixture(scope='module')
def report():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    k = mod.kernels()
    assert len(k) > 40 and KERNEL in k, sorted(k)
    return mod, k


def launch_lds_bytes():
    """DAB_LDS_BYTES, from the constant expressions of csrc/decoder.hip"""
    text = open(SRC).read()
    env = {}
    for name in ('DA_PS', 'DA_BIAS', 'DAB_SB3', 'DAB_SQ', 'DAB_SQQ', 'DAB_LDS_BYTES'):
        m = re.search(r'^constexpr [^\n]*\b' + name + r' = ([^;,]+)[;,]', text, re.M)
        assert m, name
        env[name] = int(eval(m.group(1).replace('sizeof(float4)', '16'), {'__builtins__': {}}, env))
    return env['DAB_LDS_BYTES']


def code_bytes(mod, name):
    """size of the kernel's text: the address after its last instruction minus its first one"""
    import subprocess, tempfile
    for img in mod.code_objects(mod.DEFAULT_LIB):
        with tempfile.NamedTemporaryFile(suffix='.elf') as f:
            f.write(img); f.flush()
            txt = subprocess.run([os.path.join(mod.LLVM, 'llvm-readelf'), '-sW', '--demangle', f.name], capture_output=True, text=True).stdout
        for line in txt.splitlines():
            p = line.split(None, 7)
            if len(p) == 8 and p[3] == 'FUNC' and re.sub(r'\(.*$', '', p[7]).replace('efe::', '').replace('void ', '') == name:
                return int(p[2])
    raise AssertionError(f'{name}: no FUNC symbol')


def test_k_dec_ab_register_budget(report):
    mod, k = report
    v = k[KERNEL]
    print(f'{KERNEL}: VGPRs {v[".vgpr_count"]} + AGPRs {v[".agpr_count"]}, scratch {v[".private_segment_fixed_size"]} bytes, '
          f'spilled VGPRs {v[".vgpr_spill_count"]}, spilled SGPRs {v[".sgpr_spill_count"]}')
    assert v['.vgpr_count'] + v['.agpr_count'] <= 256, v
    assert v['.private_segment_fixed_size'] == 0 and v['.vgpr_spill_count'] == 0, v
    assert v['.sgpr_spill_count'] == 0, v
    assert v['.max_flat_workgroup_size'] == 256, v


def test_k_dec_ab_lds_lets_two_workgroups_share_a_cu(report):
    mod, k = report
    static, declared = k[KERNEL]['.group_segment_fixed_size'], launch_lds_bytes()
    print(f'{KERNEL}: LDS {static} bytes, all static (the launch passes no dynamic LDS); DAB_LDS_BYTES {declared}')
    assert static == declared, (static, declared)            # (the premise: the metadata is the whole of it)
    assert static <= 81920, static
    assert static >= 74784 + 4240 - 16, static               # (k_dec_a's region and k_dec_b4's static arrays both fit)


def test_k_dec_ab_code_fits_the_instruction_cache(report):
    mod, _ = report
    sizes = {n: code_bytes(mod, n) for n in ('k_dec_a', 'k_dec_b4<1>', KERNEL)}
    print('code bytes:', sizes)
    assert sizes[KERNEL] <= sizes['k_dec_a'] + sizes['k_dec_b4<1>'] + 2048, sizes       # the two bodies once each, not a copy more
    assert sizes[KERNEL] <= 48 * 1024, sizes                                           # well inside 64 KiB
