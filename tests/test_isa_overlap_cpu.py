"""Static figures of body a's non-matrix work in k_dec_ab after layer 1 moved to the row form (wino_l1_rows) and the fused kernel's layer-2
temporaries moved a step later, read from the BUILT library through tools/isa_report.py (no GPU, no recompilation), against the parent build
e1a555a measured with the same tool:

  * hazard wait states (the sum over s_nop N of N + 1) of k_dec_ab are not above the parent's.  The figure is taken over the kernel's own
    text: behind it the listing holds the s_nop 0 padding that fills the code object up to its alignment (263 of
    them in the parent, another number whenever the code length changes), which no wave executes.  Parent: 284 (with the padding: 547);
    this build: 274 (543).  Both forms of the figure are held.
  * its v_mfma count is the parent's 1248: the change moves and removes non-matrix instructions only.
  * k_dec_a, which keeps wino_l1 and the early temporaries because it has no registers for either change, has no scratch.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = 'e1a555a'
PARENT_WAIT_STATES = 284          # k_dec_ab of PARENT, the kernel's text without the padding behind it
PARENT_WAIT_STATES_LISTING = 547  # the same over the tool's whole listing of the kernel, padding included
PARENT_MFMA = 1248


@pytest.fixture(scope='module')
def report():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    return mod, mod.kernels(), mod.disassembly()


def kernel_text(mod, text):
    """the kernel's instructions without the padding behind its code (blocks laid out behind s_endpgm are code and stay)"""
    lines = mod.listing(text)
    while lines and lines[-1] in ('s_nop 0', 's_code_end', '...'):
        lines.pop()
    assert 's_endpgm' in lines
    return lines


def test_k_dec_ab_wait_states_and_mfma_count(report):
    mod, _, d = report
    lines = kernel_text(mod, d['k_dec_ab'])
    wait_states = sum(int(line.split()[1]) + 1 for line in lines if line.split()[0] == 's_nop')
    mfma = sum(1 for line in lines if line.split()[0].startswith('v_mfma'))
    print(f'k_dec_ab: {len(lines)} instructions, hazard wait states {wait_states} (parent {PARENT}: {PARENT_WAIT_STATES}), MFMAs {mfma}')
    assert mfma == PARENT_MFMA, mfma
    assert wait_states <= PARENT_WAIT_STATES, wait_states
    whole = sum(int(line.split()[1]) + 1 for line in mod.listing(d['k_dec_ab']) if line.split()[0] == 's_nop')
    print(f'k_dec_ab: the whole listing, padding included: {whole} (parent: {PARENT_WAIT_STATES_LISTING})')
    assert whole <= PARENT_WAIT_STATES_LISTING, whole


def test_k_dec_a_has_no_scratch(report):
    _, k, _ = report
    v = k['k_dec_a']
    assert v['.private_segment_fixed_size'] == 0 and v['.vgpr_spill_count'] == 0 and v['.sgpr_spill_count'] == 0, v
    assert v['.vgpr_count'] + v['.agpr_count'] <= 256, v
