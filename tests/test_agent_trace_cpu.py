"""The rules behind the record of an agent run, on the CPU: the numpy restatements (tests/agent_trace_ref.py) on hand-made cases, and the
agreement of header, library and Python binding on the four new calls."""
import ctypes
import os
import re

import numpy as np

import agent_trace_ref as TR
from conftest import ROOT

NEW_CALLS = ('efe_agent_trace_tick', 'efe_agent_trace_decision', 'efe_agent_plan_mask', 'efe_agent_view')


def state_at(tx, ty):
    s = np.zeros(7, dtype=np.float32)
    s[5], s[4] = tx, ty
    return s


# ---- the mask --------------------------------------------------------------------------------------------------------------------------
def test_a_walker_pinned_at_a_border_counts_nothing():
    for action, (tx, ty) in ((0, (31, 5)), (1, (0, 5)), (2, (5, 31)), (3, (5, 0))):
        assert not TR.plan_mask([[action, action]], state_at(tx, ty), 3).any(), action


def test_a_walker_leaves_the_border_the_other_way():
    m = TR.plan_mask([[1]], state_at(31, 5), 2)                      # tx 31 -> 30 -> 29
    want = np.zeros((32, 32), dtype=np.float32)
    want[30, 5] = want[29, 5] = 1.0
    assert np.array_equal(m, want)
    m = TR.plan_mask([[0, 2]], state_at(30, 30), 3)                  # one move up, two blocked; one move left, two blocked
    want[:] = 0
    want[31, 30] = want[31, 31] = 1.0
    assert np.array_equal(m, want)


def test_no_path_gives_zeros():
    for paths in ([], [[]], [[], []]):
        m = TR.plan_mask(paths, state_at(3, 4), 5)
        assert m.dtype == np.float32 and m.shape == (32, 32) and not m.any()


def test_two_paths_sharing_cells():
    m = TR.plan_mask([[0, 2], [0, 0], [0]], state_at(10, 10), 1)
    want = np.zeros((32, 32), dtype=np.float32)
    want[11, 10] = 1.0                                               # all three paths
    want[11, 11] = want[12, 10] = np.float32(1) / np.float32(3)
    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))


def test_a_start_outside_the_grid_is_clamped():
    assert TR.start(-3.0) == 0 and TR.start(40.0) == 31 and TR.start(float('nan')) == 0 and TR.start(7.9) == 7
    m = TR.plan_mask([[1]], state_at(99, -2), 1)
    assert m[30, 0] == 1.0 and m.sum() == 1.0


# ---- the view --------------------------------------------------------------------------------------------------------------------------
def test_view_marker_mask_and_saturation():
    frame = np.zeros((64, 64), dtype=np.float32)
    frame[20, 20], frame[21, 21], frame[5, 5], frame[6, 6] = 1.0, 0.5, 0.999, float('nan')
    mask = np.zeros((32, 32), dtype=np.float32)
    mask[4, 4], mask[5, 5], mask[6, 6] = 1.0, 0.75, 0.25             # over pixels (20, 20), (21, 21), (22, 22)
    v = TR.view(frame, mask)
    assert v.dtype == np.uint8 and v.shape == (64, 64)
    assert v[20, 20] == 255                                          # 1.0 + 1.0: saturates where a wrapping cast gives 254
    assert v[21, 21] == 255 and v[22, 22] == 63                      # 1.25 saturates; trunc(0.25 * 255) = 63
    assert v[5, 5] == 254 and v[6, 6] == 0                           # trunc(254.745); NaN -> 0
    assert (v[59:63, 31] == 255).all() and v[58, 31] == 0 and v[63, 31] == 0 and v[60, 30] == 0
    plain = TR.view(frame)
    assert plain[20, 20] == 255 and plain[21, 21] == 127 and plain[22, 22] == 0 and (plain[59:63, 31] == 255).all()


# ---- the draw --------------------------------------------------------------------------------------------------------------------------
def test_the_edge_rule():
    assert [TR.choice([0.25] * 4, u) for u in (0.0, 0.25, 0.49, 0.75, 1.0)] == [0, 1, 1, 3, 3]
    assert TR.choice([0.3, 0.7, 0.0, 0.0], 1.0) == 1 and TR.choice([1.0, 0.0, 0.0, 0.0], 1.0) == 0
    assert TR.choice([0.0] * 4, 0.5) == -1
    assert TR.choice([0.5, -0.1, 0.6, 0.0], 0.5) == -1 and TR.choice([0.5, float('nan'), 0.5, 0.0], 0.5) == -1
    assert TR.choice([float('inf'), 0.0, 0.0, 0.0], 0.5) == -1


# ---- header, library, binding ------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_new_calls():
    import __graft_entry__ as ge
    ge.build()
    from daimc_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    loaded = _lib.load()
    for name in NEW_CALLS:
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', txt)
        assert decl, f'{name} is not declared in efe_engine.h'
        assert hasattr(lib, name) and name in _lib.EXPORTS
        n_args = len([a for a in decl.group(1).split(',') if a.strip()])
        assert len(getattr(loaded, name).argtypes) == n_args, name
    fields = re.search(r'typedef struct efe_agent_trace \{(.*?)\} efe_agent_trace;', txt, flags=re.S).group(1)
    names = re.findall(r'\*\s*([a-z_A-Z]+)\s*;', fields)
    assert tuple(names) == _lib.TRACE_FIELDS
    assert [f for f, _ in _lib.EfeAgentTrace._fields_] == names + ['T', 'E', 'Lp']


def test_the_record_lists_every_field_of_the_struct():
    import daimc_amd
    from daimc_amd import _lib
    assert set(_lib.TRACE_FIELDS) | {'changed'} == set(daimc_amd.AgentTrace.FIELDS)
