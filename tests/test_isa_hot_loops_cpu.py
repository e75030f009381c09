"""Instructions that must stay out of the decoder kernels' hot loops, read from the disassembly of the BUILT library (tools/isa_report.py,
as tests/test_isa_budget.py reads its metadata; no GPU, no recompilation).  They cost issue slots beside the MFMA stream without failing
any numerical test when they come back:
  * v_mad_u64_u32 in k_dec_b4: hipcc formed every LDS address of the strip staging (and of the H-plane stores) with this quarter-rate
    64-bit multiply-add, ten per strip, in front of the strip barrier; the addresses are one register plus immediates now;
  * v_pk_add_f32 / v_pk_mul_f32 in k_dec_b4: hipcc lowers f32x4 + f32x4 to packed adds and SLP-packs neighbouring scalar ones (with v_mov
    shuffles to pair the registers); the kernel uses the single-lane forms of mfma_pipe.h (add1, sub1, add4, sub4).  (k_dec_a and
    k_dec_a_s keep their packed adds: the single-lane forms measured no gain there)"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def listing():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    d = mod.disassembly()
    assert len(d) > 40, sorted(d)
    return d


def count(text, word):
    return len(re.findall(r'\b' + re.escape(word) + r'\b', text))


@pytest.mark.parametrize('name', ['k_dec_b4<1>', 'k_dec_b4<4>', 'k_dec_a', 'k_dec_a_s'])
def test_the_listing_is_the_kernel(listing, name):
    """the premise of the two tests below: the text is the whole kernel (its MFMA count is the contraction's)"""
    assert name in listing, sorted(listing)
    want = {'k_dec_b4<1>': 464, 'k_dec_b4<4>': 464}.get(name)
    n = count(listing[name], 'v_mfma_f32_16x16x4_f32') + count(listing[name], 'v_mfma_f32_32x32x2_f32')
    assert n == want if want else n >= 400, (name, n)


@pytest.mark.parametrize('name', ['k_dec_b4<1>', 'k_dec_b4<4>'])
def test_strip_staging_forms_no_64_bit_addresses(listing, name):
    assert count(listing[name], 'v_mad_u64_u32') == 0, name


@pytest.mark.parametrize('name', ['k_dec_b4<1>', 'k_dec_b4<4>'])
def test_no_packed_fp32_adds_beside_the_mfma_stream(listing, name):
    for word in ('v_pk_add_f32', 'v_pk_mul_f32'):
        assert count(listing[name], word) == 0, (name, word, count(listing[name], word))
