"""k_dec_ab (engine option dec_fuse_ab = 1): k_dec_a and k_dec_b4<1> as one persistent launch, y2 in a 256 KiB slot per workgroup.
The fused launch calls the two kernels' own bodies, so every output must keep every bit of the two-launch form (dec_fuse_ab = 0):
G, its three terms, the stored images and -- where the call hands them out (calculate_G's parts) -- the per-sample pieces of the
per-image sums `val`; a rollout only returns sums of `val`, which its terms are.

Shapes: 132 decoder images (2 rows x depth 1 x 22 samples x 3 passes), the smallest launch above DEC_SPLIT_MAX = 128, so the large-launch
kernels run; the rollout has the three pass kinds, the reward mode (pass 0) and the image store.  With dec_ab_grid = 3 every workgroup
carries 44 images: the static pair, the tickets, the reuse of a slot and the per-image reload of the zero row, the zero column and the tap
operand.  The masked call (33 rows x 4 samples = 396 images, rows 1, 3, .. dead) has dead images on both sides of every live one.
dec_chunk = 70 makes two fused launches (70 + 62 images) share the slots.  The model is this file's own; dec_fuse_ab is set explicitly by
every run (the tests do not depend on the engine's default), the other options are put back on exit."""
import numpy as np
import pytest
import torch

IMAGES = 2 * 1 * 22 * 3
KIB256 = 256 * 1024
CLS_A, CLS_B = 'dec_a_convT1_convT2', 'dec_b_convT3_final_reduce'
DEFAULTS = {'dec_ab_grid': 0, 'dec_chunk': 32768}


@pytest.fixture(scope='module')
def model():
    import daimc_amd
    from oracle import synth
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=11, init_weights=False)
    m.load_flat_weights(synth.make_weights(1234, 1.15))
    return m


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).view(np.uint32).copy()


def _rollout(m):
    from oracle import synth
    o = synth.make_frames(23, 2)
    pi = np.eye(4, dtype=np.float32)[[1, 2]]
    r = m.calculate_G_repeated(o, pi, steps=1, samples=22, stage=8)
    torch.cuda.synchronize()
    return {'G': _bits(r[0]), 'term0': _bits(r[1][0]), 'term1': _bits(r[1][1]), 'term2': _bits(r[1][2]), 'po1': _bits(r[2])}


def _masked(m):
    from daimc_amd.model import Rows
    from oracle import philox as PX
    s0 = torch.from_numpy(PX.uniform_fill(3, (33, 10), 61, -1.5, 1.5).astype(np.float32)).to(m.device)
    pi = torch.from_numpy(np.eye(4, dtype=np.float32)[np.arange(33) % 4]).to(m.device)
    alive = torch.tensor([1 - (i & 1) for i in range(33)], dtype=torch.uint8, device=m.device)
    parts = []
    r = m.calculate_G(s0, pi, samples=4, stage=5, rows=Rows(mask=alive), _parts=parts)
    torch.cuda.synchronize()
    live = np.arange(0, 33, 2)
    out = {'G': _bits(r[0])[live], 'term0': _bits(r[1][0])[live], 'term1': _bits(r[1][1])[live], 'term2': _bits(r[1][2])[live],
           'po1': _bits(r[4])[live]}
    out['parts'] = _bits(parts[0])[:, live]          # [2][rows]
    return out


def _with(m, fuse, fn, **opts):
    try:
        m.set_option('dec_fuse_ab', fuse)
        for k, v in opts.items():
            m.set_option(k, v)
        return fn(m)
    finally:
        for k in opts:
            m.set_option(k, DEFAULTS[k])


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for n in want:
        assert got[n].shape == want[n].shape, (what, n, got[n].shape, want[n].shape)
        assert np.array_equal(got[n], want[n]), (what, n, int((got[n] != want[n]).sum()), 'of', got[n].size, 'words differ')


@pytest.fixture(scope='module')
def unfused_rollout(model):
    ref = _with(model, 0, _rollout)
    assert np.isfinite(ref['G'].view(np.float32)).all() and float(ref['po1'].view(np.float32).std()) > 1e-3      # (finite, and the images are not flat)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize('opts', [{}, {'dec_ab_grid': 3}, {'dec_chunk': 70}, {'dec_chunk': 70, 'dec_ab_grid': 3}],
                         ids=['grid_132', 'grid_3', 'two_launches', 'two_launches_grid_3'])
def test_fused_rollout_keeps_every_bit(model, unfused_rollout, opts):
    _same(_with(model, 1, _rollout, **opts), unfused_rollout, opts)


@pytest.mark.gpu
@pytest.mark.parametrize('grid', [0, 3])
def test_fused_masked_call_keeps_every_bit_of_the_live_rows(model, grid):
    ref = _with(model, 0, _masked)
    assert np.isfinite(ref['G'].view(np.float32)).all()
    _same(_with(model, 1, _masked, dec_ab_grid=grid), ref, ('mask', grid))


@pytest.mark.gpu
def test_fused_scratch_is_one_slot_per_workgroup(model):
    """reserve(2, 1, 22): the fused plan with a grid of 3 needs (132 - 3) x 256 KiB less than the two-launch plan, and a call after the
    reservation never grows the arena"""
    need0 = _with(model, 0, lambda m: m.reserve(2, 1, 22))
    def fused(m):
        need = m.reserve(2, 1, 22)
        before = m.arena_stats()['grow_count']
        _rollout(m)
        return need, before, m.arena_stats()['grow_count']
    need1, before, after = _with(model, 1, fused, dec_ab_grid=3)
    print(f'scratch: two launches {need0} bytes, fused with 3 slots {need1} bytes')
    assert need0 - need1 == (IMAGES - 3) * KIB256, (need0, need1)
    assert after == before, (before, after)


@pytest.mark.gpu
@pytest.mark.parametrize('classes', [(CLS_A,), (CLS_B,), (CLS_A, CLS_B)], ids=['class_a', 'class_b', 'both'])
def test_profiling_a_tail_class_runs_the_two_launches(model, unfused_rollout, classes):
    """one launch has no boundary between the two classes: while either is timed the call runs k_dec_a and k_dec_b4, every timed class
    reports its launch, and the results are those of the fused run"""
    def timed(m):
        try:
            m.prof_enable(True, classes=list(classes))
            out = _rollout(m)
            return out, m.prof_read()
        finally:
            m.prof_enable(False)
    out, prof = _with(model, 1, timed)
    for c in classes:
        assert prof[c][1] == 1 and prof[c][0] > 0.0, (c, prof[c])
    _same(out, _with(model, 1, _rollout), classes)
    _same(out, unfused_rollout, classes)
