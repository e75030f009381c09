"""CPU tests behind tests/test_train_seams_gpu.py (the seam table: tests/train_seams.py).

1. The gate cap of the GPU gate tests (two gate sets may differ only where |a_64| <= 1e-5, on at most 1e-4 of a layer) holds between the fp32
   and the fp64 run of tests/train_enc_g_ref.run on their own gates, in all fourteen gated layers, for every (geometry, M) of the table: an
   input seed that did not hold it here would fail on the GPU for no fault of the kernels.
2. The fp64 rule sees a lost row.  The fp32 reference gradient minus the contribution of the one row that starts the last row group
   (run(row alone, row_offset = r).grads / M) fails the rule in every one of the 32 tensors -- the counterpart of
   tests/test_fp64_oracle.py::test_rule_rejects_simulated_kernel_errors at these shapes: a kernel or host loop that drops one row at a seam
   cannot pass the GPU cases.  The single row's forward differs from the batched run's row by the CPU's summation order only; that is
   checked with a tolerance (below), not by bits.
3. The table's group sizes and slab counts are csrc/kernels.h's, read from the header by text: a later change of a group size fails here
   and does not quietly move the seams away from the cases."""
import os
import re

import numpy as np
import pytest
import torch

import train_enc_g_ref as TEG
import train_seams as TS
from oracle import synth
from test_fp64_parity import ALPHA, fp64_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = TS.STAGE
_W = {}


def weights(geo):
    if geo not in _W:
        _W[geo] = synth.make_weights(1234, 1.15, *geo)          # 'g115'
    return _W[geo]


def run(geo, inp, dtype, **kw):
    return TEG.run(weights(geo), *inp, geo[1], geo[2], STAGE, dtype, **kw)


# ---- 1. the gate cap on the reference alone --------------------------------------------------------------------------
@pytest.mark.parametrize('geo,M', TS.CASES, ids=TS.ids(TS.CASES))
def test_gate_cap_holds_on_the_reference_alone(geo, M):
    inp = TS.inputs(geo, M)
    r32, r64 = run(geo, inp, torch.float32), run(geo, inp, torch.float64)
    layers = [(f'y{i + 1}', r32['y'][i], r64['y'][i], r64['a_conv'][i]) for i in range(4)]
    layers += [(f'h{i + 1}', r32['h'][i], r64['h'][i], r64['a_dense'][i]) for i in range(3)]
    layers += [(f'dec h{i + 1}', r32['dec_h'][i], r64['dec_h'][i], r64['dec_a_head'][i]) for i in range(4)]
    layers += [(f'dec y{i + 1}', r32['dec_y'][i], r64['dec_y'][i], r64['dec_a'][i]) for i in range(3)]
    assert len(layers) == 14
    worst = [TS.gate_diff(f'{geo} M={M} {name}', a, b > 0, a64) for name, a, b, a64 in layers]
    print(f'{geo} M={M}: worst |a_64| at a differing gate {max(w for w, _ in worst):.3e}, largest differing share {max(s for _, s in worst):.3e}')


# ---- 2. the rule sees a lost row -------------------------------------------------------------------------------------
LOST = [(TS.G64, 130, 128), (TS.G64, 130, 129), (TS.G68, 65, 64), (TS.G64, TS.M_MAX, 256)]


@pytest.mark.parametrize('geo,M,r', LOST, ids=TS.ids(LOST))
def test_rule_rejects_a_lost_seam_row(geo, M, r):
    inp = TS.inputs(geo, M)
    o32 = run(geo, inp, torch.float32)
    o64 = run(geo, inp, torch.float64, gates=o32['y'] + o32['h'], dec_gates=o32['dec_h'] + o32['dec_y'])
    one = run(geo, tuple(x[r:r + 1] for x in inp), torch.float32, row_offset=r)
    # the row alone is the batched run's row up to the order of the CPU's fp32 sums: dot products of at most 576 (encoder) and 256 (decoder
    # head) terms of O(1) values, sqrt(576) * 2^-24 * a few = 1e-5 at the worst
    for k in ('qs1', 'mean', 'logvar'):
        d = float(np.abs(one[k][0] - o32[k][r]).max())
        print(f'{geo} M={M} row {r}: max |alone - batched| {k} {d:.3e}')
        np.testing.assert_allclose(one[k][0], o32[k][r], rtol=1e-5, atol=2e-5, err_msg=k)
    np.testing.assert_allclose(one['F_down'][0], o32['F_down'][r], rtol=1e-5)
    ratios = {}
    for k in TEG.KEYS:
        lost = o32['grads'][k] - one['grads'][k] / np.float32(M)
        rows = fp64_rule(k, lost, o32['grads'][k], o64['grads'][k])
        ratios[k] = min(row[4] for row in rows)
        assert not any(row[-1] for row in rows), f'{geo} M={M}: the gradient without row {r} passes the rule in {k} (ratio {ratios[k]:.2f})'
    k = min(ratios, key=ratios.get)
    print(f'{geo} M={M}: without row {r} the smallest ratio over the 32 tensors is {ratios[k]:.0f} ({k}); the rule allows {ALPHA:.0f}')


# ---- 3. the table against the code's constants -------------------------------------------------------------------------
def test_seam_table_follows_the_constants_of_kernels_h():
    h = open(os.path.join(ROOT, 'deep-active-inference-mc_amd', 'csrc', 'kernels.h')).read()

    def const(name):
        m = re.search(r'^constexpr int ' + name + r' = (\d+);', h, re.M)
        assert m, name
        return int(m.group(1))

    assert const('DEC_TAIL_SLABS') == const('ENC_CONV_SLABS') == TS.CONV_SLABS
    assert const('DEC_HEAD_SLABS') == const('ENC_HEAD_SLABS') == TS.HEAD_SLABS
    assert const('DEC_TAIL_ROWS') == TS.ROWS_SMALL
    m = re.search(r'int rows_per_pass\(\) const \{ return B <= (\d+) \? (\d+) : (\d+); \}', h)
    assert m and tuple(int(x) for x in m.groups()) == (TS.BASE_SPLIT, TS.ROWS_SMALL, TS.ROWS_LARGE)
    # the slab of a row and of a tile, as the table's text states them
    assert re.search(r'dec_tail_slabs\(int M\) \{ return M < DEC_TAIL_SLABS \? M : DEC_TAIL_SLABS; \}', h)
    assert re.search(r'enc_conv_slabs\(int M\) \{ return M < ENC_CONV_SLABS \? M : ENC_CONV_SLABS; \}', h)
    assert re.search(r'dec_head_slabs\(int M\) \{ const int t = \(M \+ 15\) / 16; return t < DEC_HEAD_SLABS \? t : DEC_HEAD_SLABS; \}', h)
    assert re.search(r'enc_head_slabs\(int M\) \{ const int t = \(M \+ 15\) / 16; return t < ENC_HEAD_SLABS \? t : ENC_HEAD_SLABS; \}', h)
    # a group holds whole slabs' worth of rows and whole tiles; a 64-row group holds exactly HEAD_SLABS tiles (the 1 x 64 x 64 heads' first = m0 == 0)
    assert TS.ROWS_SMALL % TS.CONV_SLABS == 0 and TS.ROWS_LARGE % TS.CONV_SLABS == 0 and TS.ROWS_LARGE % TS.TILE == 0
    assert TS.ROWS_SMALL == TS.HEAD_SLABS * TS.TILE
    assert [TS.rows_per_group(g) for g in (TS.G44, TS.G64, TS.G68)] == [64, 64, 32] and TS.base_of(68) == 17 and TEG.n_in(68) == 576
    for geo, M, groups, last in TS.TABLE:
        rows = TS.rows_per_group(geo)
        assert (-(-M // rows), M - (-(-M // rows) - 1) * rows) == (groups, last), (geo, M)
    # what each entry is there for
    assert set(M for g, M in TS.CASES if g == TS.G64) == {31, 32, 64, 96, 97, 128, 129, 130, 257}
    assert set(M for g, M in TS.CASES if g == TS.G68) == {32, 64, 65, 97} and set(M for g, M in TS.CASES if g == TS.G44) == {64, 129}
    assert min(31, TS.CONV_SLABS) == 31 and min(32, TS.CONV_SLABS) == 32                  # G = M against G = 32, no slab with a second image
    assert (96 - 64, 97 - 64) == (TS.CONV_SLABS, TS.CONV_SLABS + 1)                       # every slab once more / slab 0 twice
    assert (64 // TS.TILE) % TS.HEAD_SLABS == 0 and (96 // TS.TILE) % TS.HEAD_SLABS == 2  # (4, 1, 68): tile 4 wraps onto slab 0, tile 6 onto slab 2
    assert all(g in TS.CASES for g in TS.THREE_GROUPS + TS.ROW_CASES)
