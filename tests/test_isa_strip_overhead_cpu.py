"""Per-strip bookkeeping that was taken OUT of k_dec_b4 and must not come back, read from the disassembly of the BUILT library
(tools/isa_report.py, as tests/test_isa_hot_loops_cpu.py does; no GPU, no recompilation).  None of it fails a numerical test when it
returns; it costs issue slots and wait states beside the MFMA stream:
  * scalar ALU instructions: the H-ring slots of the six gather rows and four write rows were add / compare / select / multiply chains
    per strip; the ring's schedule is fixed, and the slots are wrapped additions (add, subtract, unsigned minimum) from one carried offset;
  * branches: the gather's "row inside the image" conditions were uniform branches inside the contraction; they are masks now;
  * hazard wait states (the sum over s_nop N of N + 1): the temporaries' adds, the ReLUs and the presums of the 32 -> 1 conv stood right
    behind the MFMAs whose results they read (or right in front of the MFMA that reads theirs).

Counts are of the whole kernel.  Budgets: the listing of the build that made the change, plus a slack of about 4 % for compiler drift.
                      scalar ALU   branches   wait states
  k_dec_b4<1>  before     591         49         444         (the parent commit, regenerated with this file's own counting)
               now        444         25         136
  k_dec_b4<4>  before     642         48         444
               now        499         29         147
"""
import collections
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scalar instructions that are not ALU work: waits, barriers, the program end, priority, loads of kernel arguments, and the branches
# (counted on their own)
NOT_ALU = re.compile(r's_(nop|waitcnt|barrier|endpgm|setprio|sleep|code_end|load_|buffer_load_|branch|cbranch_)')
BRANCH = re.compile(r's_(branch|cbranch_)')

BUDGET = {     # kernel: (scalar ALU, branches, wait states)
    'k_dec_b4<1>': (462, 26, 142),
    'k_dec_b4<4>': (519, 30, 153),
}


@pytest.fixture(scope='module')
def report():
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'tools', 'isa_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.DEFAULT_LIB):
        pytest.skip('engine library not built')
    d = mod.disassembly()
    assert len(d) > 40, sorted(d)
    return mod, d


def figures(mod, text):
    lines = mod.listing(text)
    ops = collections.Counter(line.split()[0] for line in lines)
    salu = sum(n for op, n in ops.items() if op.startswith('s_') and not NOT_ALU.match(op))
    branches = sum(n for op, n in ops.items() if BRANCH.match(op))
    wait_states = sum(int(line.split()[1]) + 1 for line in lines if line.split()[0] == 's_nop')
    mfma = sum(n for op, n in ops.items() if op.startswith('v_mfma'))
    return salu, branches, wait_states, mfma


@pytest.mark.parametrize('name', sorted(BUDGET))
def test_strip_bookkeeping_stays_out(report, name):
    mod, d = report
    assert name in d, sorted(d)
    salu, branches, wait_states, mfma = figures(mod, d[name])
    print(f'{name}: scalar ALU {salu}, branches {branches}, wait states {wait_states}, MFMAs {mfma}')
    assert mfma == 464, (name, mfma)              # the premise: the text is the whole kernel
    b_salu, b_br, b_ws = BUDGET[name]
    assert salu <= b_salu, (name, 'scalar ALU', salu, b_salu)
    assert branches <= b_br, (name, 'branches', branches, b_br)
    assert wait_states <= b_ws, (name, 'wait states', wait_states, b_ws)
