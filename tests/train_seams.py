"""The seam table of tests/test_train_seams_gpu.py and tests/test_train_seams_cpu.py: the batch sizes at which the training calls
(csrc/engine_train.hip's group loops around train_dec*.hip, train_dec_head*.hip, train_enc*.hip) cut a batch into row groups, 16-row head
tiles and partial-gradient slabs.  A plain module, like train_common.py: the table, what it assumes of csrc/kernels.h (which the CPU test
reads back from the header), the inputs of a case and the gate condition both files apply.

Geometries are (pi_dim, C, R); B = R / 4 is the decoder's base grid.  A row group is 64 rows at B <= 16 and 32 rows above; row m adds to
conv slab m mod min(M, 32); the 16-row tile t of the call adds to head slab t mod 4; the first group writes a slab, later groups add."""
import numpy as np

import train_enc_g_ref as TEG

STAGE = 3
G44, G64, G68 = (4, 1, 44), (4, 1, 64), (4, 1, 68)

# what the table assumes of csrc/kernels.h
CONV_SLABS = 32                  # DEC_TAIL_SLABS, ENC_CONV_SLABS
HEAD_SLABS = 4                   # DEC_HEAD_SLABS, ENC_HEAD_SLABS
TILE = 16                        # rows of a head tile
ROWS_SMALL, ROWS_LARGE, BASE_SPLIT = 64, 32, 16          # DecTailGeo::rows_per_pass(): B <= 16 ? 64 : 32; DEC_TAIL_ROWS = 64

M_MAX = 257                      # train_step's largest tested batch: run once, by the specialised family
# (geometry, M, number of row groups, rows of the last group)
TABLE = [(G64, 31, 1, 31), (G64, 32, 1, 32), (G64, 64, 1, 64), (G64, 96, 2, 32), (G64, 97, 2, 33), (G64, 128, 2, 64), (G64, 129, 3, 1),
         (G64, 130, 3, 2), (G64, M_MAX, 5, 1),
         (G68, 32, 1, 32), (G68, 64, 2, 32), (G68, 65, 3, 1), (G68, 97, 4, 1),
         (G44, 64, 1, 64), (G44, 129, 3, 1)]
CASES = [(geo, M) for geo, M, _, _ in TABLE]
# the cases at which the parts, the rows, the optimiser step and the scratch are examined
THREE_GROUPS = [(G64, 130), (G68, 65)]
ROW_CASES = [(G64, 130), (G68, 97)]


def ids(cases):
    """pytest ids of (..., geometry, M, ...) cases: sp-1x64-130, 1x68-65-64"""
    return ['-'.join(f'{x[1]}x{x[2]}' if isinstance(x, tuple) else str(x) for x in case) for case in cases]


def base_of(R):
    return R // 2 if R == 32 else R // 4


def rows_per_group(geo):
    return ROWS_SMALL if base_of(geo[2]) <= BASE_SPLIT else ROWS_LARGE


def inputs(geo, M):
    """(o1, ps1_mean, ps1_logvar, omega) of a case; at (1, 64) these are train_down_ref.inputs(2000 + M, M)"""
    return TEG.inputs(2000 + M, M, geo[1], geo[2])


def gate_diff(tag, have, want, a64, mask=None):
    """the gate condition of the GPU gate tests on one layer: the gates `have` > 0 and `want` (bool) may differ only where |a_64| <= 1e-5, on
    at most 1e-4 of the layer; mask (a head layer's keep mask): no gate is open outside it.  -> (worst |a_64|, share) after printing them"""
    have = np.asarray(have) > 0
    want, a64 = np.asarray(want).reshape(have.shape), np.asarray(a64).reshape(have.shape)
    if mask is not None:
        outside = int((have & (np.asarray(mask).reshape(have.shape) == 0)).sum())
        assert outside == 0, f'{tag}: {outside} open gates outside the dropout mask'
    diff = have != want
    worst = float(np.abs(a64[diff]).max()) if diff.any() else 0.0
    share = float(diff.sum()) / diff.size
    print(f'{tag}: {int(diff.sum())} of {diff.size} gates differ, worst |a_64| {worst:.3e}, share {share:.3e}')
    assert worst <= 1e-5, (tag, worst)
    assert diff.sum() <= 1e-4 * diff.size, (tag, int(diff.sum()))
    return worst, share
