"""Row sets for the root of a decision (efe_encoder_rows, efe_rollout_rows): a call over a compacted subset of the entries of a batch draws
the noise of the entries it holds, so it returns the bits the full call returns for those rows -- 6 games x 4 rows, steps 2, samples 2, both
calc_mean values, device noise and injected noise.  rows = None is today's efe_rollout / efe_encoder bit for bit; a mask with dead
entries leaves the live entries alone; the refusals hold."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES, STEPS, SAMPLES, IDS = 6, 2, 2, [4, 1, 5]
ROWS4 = [4 * i + k for i in IDS for k in range(4)]          # 16..19, 4..7, 20..23
STAGE, OFFSET = 11, 40


@pytest.fixture(scope='module')
def model():
    import daimc_amd
    return daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=17)


@pytest.fixture(scope='module')
def frames(model):
    import daimc_amd
    games = daimc_amd.Game(GAMES, model=model, seed=3)
    games.randomize_environment_all(stage=1)
    return games.current_frame_nchw()                        # [6,1,64,64]


@pytest.fixture(params=['device', 'injected'])
def noise(request, model):
    from oracle import philox as PX
    model.eps_source = PX.normals if request.param == 'injected' else None
    yield request.param
    model.eps_source = None


def rows_of(model, ids, per, mask=None):
    import daimc_amd.model as M
    t = torch.tensor(ids, dtype=torch.int32, device=model.device)
    return M.Rows(mask=mask, ids=t, rows_per_entry=per, ids_host=list(ids), n_total=GAMES)


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('calc_mean', [False, True])
@pytest.mark.parametrize('per_stage_mean', [False, True])
def test_rollout_rows_equal_the_rows_of_the_full_call(model, frames, noise, calc_mean, per_stage_mean):
    o4 = frames.repeat_interleave(4, dim=0)
    pi = model.pi_one_hot.repeat(GAMES, 1)
    kw = dict(steps=STEPS, calc_mean=calc_mean, samples=SAMPLES, stage=STAGE, row_offset=OFFSET)
    if per_stage_mean:
        call = lambda o, p, rows: model.calculate_G_4_repeated(o, rows=rows, **kw)
        import daimc_amd.model as M
        full = call(o4, pi, M.Rows(rows_per_entry=4, n_total=GAMES))      # the batched form, identity rows
    else:
        call = lambda o, p, rows: model.calculate_G_repeated(o, p, rows=rows, **kw)
        full = call(o4, pi, None)
    sub = call(o4[ROWS4], pi[ROWS4], rows_of(model, IDS, 4))
    assert same(sub[0], full[0][ROWS4])
    for k in range(3):
        assert same(sub[1][k], full[1][k][ROWS4]), k
    assert same(sub[2], full[2][ROWS4])
    assert torch.isfinite(full[0]).all() and len(torch.unique(full[0])) == 4 * GAMES      # the rows differ: the comparison is not vacuous


def test_batched_4_repeated_equals_one_game_at_a_time(model, frames, noise):
    """the batched calculate_G_4_repeated is the reference's 4-row call per game with row_offset 4 g"""
    import daimc_amd.model as M
    o4 = frames.repeat_interleave(4, dim=0)
    full = model.calculate_G_4_repeated(o4, steps=STEPS, samples=SAMPLES, stage=STAGE, row_offset=OFFSET, rows=M.Rows(rows_per_entry=4, n_total=GAMES))
    for g in (0, 3, 5):
        one = model.calculate_G_4_repeated(o4[4 * g:4 * g + 4], steps=STEPS, samples=SAMPLES, stage=STAGE, row_offset=OFFSET + 4 * g)
        assert same(one[0], full[0][4 * g:4 * g + 4]), g
        assert all(same(one[1][k], full[1][k][4 * g:4 * g + 4]) for k in range(3)), g


def test_encoder_rows_equal_the_rows_of_the_full_call(model, frames, noise):
    kw = dict(stage=STAGE, row_offset=OFFSET)
    s_f, m_f, l_f = model.model_down.encoder_with_sample(frames, **kw)
    s_s, m_s, l_s = model.model_down.encoder_with_sample(frames[IDS], rows=rows_of(model, IDS, 1), **kw)
    assert same(s_s, s_f[IDS]) and same(m_s, m_f[IDS]) and same(l_s, l_f[IDS])
    mf, lf = model.model_down.encoder(frames, **kw)
    ms, ls = model.model_down.encoder(frames[IDS], rows=rows_of(model, IDS, 1), **kw)
    assert same(ms, mf[IDS]) and same(ls, lf[IDS])
    assert not same(s_f[IDS], s_f[:3])                       # another game draws other noise
    # rows_per_entry = 4 on the encoder: the layout of the decision's repeated frames
    o4 = frames.repeat_interleave(4, dim=0)
    s4f, m4f, _ = model.model_down.encoder_with_sample(o4, **kw)
    s4s, m4s, _ = model.model_down.encoder_with_sample(o4[ROWS4], rows=rows_of(model, IDS, 4), **kw)
    assert same(s4s, s4f[ROWS4]) and same(m4s, m4f[ROWS4])


def test_dead_entries_leave_live_entries_alone(model, frames):
    import daimc_amd.model as M
    o4 = frames.repeat_interleave(4, dim=0)
    pi = model.pi_one_hot.repeat(GAMES, 1)
    kw = dict(steps=STEPS, samples=SAMPLES, stage=STAGE, row_offset=OFFSET)
    full = model.calculate_G_repeated(o4, pi, **kw)
    mask = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8, device=model.device)
    live = [4 * g + k for g in (0, 2, 3, 5) for k in range(4)]
    masked = model.calculate_G_repeated(o4, pi, rows=M.Rows(mask=mask, rows_per_entry=4, n_total=GAMES), **kw)
    assert same(masked[0][live], full[0][live]) and all(same(masked[1][k][live], full[1][k][live]) for k in range(3))
    # ... also through ids: entries [4, 1, 5], entry 1 dead
    mask = torch.tensor([1, 0, 1, 1, 1, 1], dtype=torch.uint8, device=model.device)          # (the mask is indexed by entry id)
    sub = model.calculate_G_repeated(o4[ROWS4], pi[ROWS4], rows=rows_of(model, IDS, 4, mask=mask), **kw)
    keep = [0, 1, 2, 3, 8, 9, 10, 11]
    assert same(sub[0][keep], full[0][[ROWS4[i] for i in keep]])
    mf, _ = model.model_down.encoder(frames, stage=STAGE, row_offset=OFFSET)
    mm, _ = model.model_down.encoder(frames, stage=STAGE, row_offset=OFFSET, rows=M.Rows(mask=mask, rows_per_entry=1, n_total=GAMES))
    assert same(mm[[0, 2, 3, 5]], mf[[0, 2, 3, 5]])


def test_rows_none_is_the_existing_entry_point(model, frames):
    """efe_rollout / efe_encoder are the rows = NULL call of the _rows forms: both names, and the Python path without `rows`, give the
    same bits.  The two names are one function now, so this cannot show a change of bits against earlier builds: that guarantee is
    carried by the existing fixture tests of efe_rollout and efe_encoder (tests/test_gpu_parity.py, tests/test_noise_keys_gpu.py), which
    go through the rows = NULL path."""
    e = model._ready()
    from daimc_amd import _lib
    from daimc_amd.model import _ptr
    o4 = frames.repeat_interleave(4, dim=0).contiguous()
    pi = model.pi_one_hot.repeat(GAMES, 1).contiguous()
    M_ = o4.shape[0]
    nz = _lib.EfeNoise(model.seed, STAGE, 0, 0, OFFSET)
    out = []
    for rows_form in (False, True):
        G, T = torch.empty(M_, device=model.device), torch.empty(3, M_, device=model.device)
        if rows_form:
            e.check(e.lib.efe_rollout_rows(e.ctx, _ptr(o4), _ptr(pi), M_, STEPS, SAMPLES, 0, 0, C.byref(nz), None, None, _ptr(G), _ptr(T), None, e.stream()))
        else:
            e.check(e.lib.efe_rollout(e.ctx, _ptr(o4), _ptr(pi), M_, STEPS, SAMPLES, 0, 0, C.byref(nz), None, _ptr(G), _ptr(T), None, e.stream()))
        out.append((G, T))
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    ref = model.calculate_G_repeated(o4, pi, steps=STEPS, samples=SAMPLES, stage=STAGE, row_offset=OFFSET)
    assert same(ref[0], out[0][0])
    nz = _lib.EfeNoise(model.seed, STAGE, 6, 0, OFFSET)
    enc = []
    for rows_form in (False, True):
        s, mean, lv = (torch.empty(GAMES, 10, device=model.device) for _ in range(3))
        if rows_form:
            e.check(e.lib.efe_encoder_rows(e.ctx, _ptr(frames), GAMES, C.byref(nz), None, None, _ptr(s), _ptr(mean), _ptr(lv), e.stream()))
        else:
            e.check(e.lib.efe_encoder(e.ctx, _ptr(frames), GAMES, C.byref(nz), None, _ptr(s), _ptr(mean), _ptr(lv), e.stream()))
        enc.append((s, mean, lv))
    assert all(same(a, b) for a, b in zip(*enc))
    s_py, m_py, _ = model.model_down.encoder_with_sample(frames, stage=STAGE, pass_=6, row_offset=OFFSET)
    assert same(s_py, enc[0][0]) and same(m_py, enc[0][1])


def test_ctypes_row_sets_equal_the_custom_ops(model):
    """efe_calculate_g_rows and efe_simulate_rows through ctypes with an EfeRows (the binding's mirror of efe_rows) against ops.calculate_g
    and ops.simulate given the same tensors: 3 entries compacted to ids [2, 0], n_total 3 -- the same C call twice, so the same bits"""
    from daimc_amd import _lib
    e, dev, p = model._ready(), model.device, _lib.ptr
    gen = torch.Generator().manual_seed(5)
    ids = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    mask = torch.ones(3, dtype=torch.uint8, device=dev)
    nz = _lib.EfeNoise(model.seed, STAGE, 0, 0, OFFSET)
    # calculate_G: 2 entries x pi_dim 4 rows, one sample
    s0 = torch.randn(8, 10, generator=gen).to(dev)
    pi0 = model.pi_one_hot.repeat(2, 1).contiguous()
    want = e.ops.calculate_g(e.h, s0, pi0, 1, False, model._seed64(), STAGE, OFFSET, None, mask, ids, 4, 3)
    rows = _lib.EfeRows(mask.data_ptr(), ids.data_ptr(), 4, 3)
    got = [torch.empty_like(t) for t in want]                   # G, terms, ps1, ps1_mean, po1, t2parts
    e.check(e.lib.efe_calculate_g_rows(e.ctx, p(s0), p(pi0), 8, 1, 0, C.byref(nz), None, C.byref(rows), *[p(t) for t in got], e.stream()))
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert torch.isfinite(want[0]).all()
    plain = [torch.empty_like(t) for t in want]                 # NULL: entries 0 and 1 of the batch, other noise
    e.check(e.lib.efe_calculate_g_rows(e.ctx, p(s0), p(pi0), 8, 1, 0, C.byref(nz), None, None, *[p(t) for t in plain], e.stream()))
    assert not same(plain[0], want[0])
    # simulate: 2 of 3 episodes, depth 2
    s = torch.randn(2, 10, generator=gen).to(dev)
    want = e.ops.simulate(e.h, s, 2, False, model._seed64(), STAGE, OFFSET, None, None, None, ids, 3)
    rows = _lib.EfeRows(None, ids.data_ptr(), 1, 3)
    got = [torch.empty_like(t) for t in want]                   # G, pi0, Qpi0
    e.check(e.lib.efe_simulate_rows(e.ctx, p(s), 2, 2, 0, C.byref(nz), None, None, C.byref(rows), *[p(t) for t in got], e.stream()))
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert torch.isfinite(want[0]).all() and want[1].sum() == 4       # one-hot actions: 2 episodes x depth 2


def test_refusals(model, frames):
    import daimc_amd
    import daimc_amd.model as M
    o4 = frames.repeat_interleave(4, dim=0)
    with pytest.raises(ValueError, match='4 rows'):
        model.calculate_G_4_repeated(o4, steps=1, samples=1)                                  # the 4-row refusal stays without rows
    with pytest.raises(ValueError, match='rows_per_entry=4'):
        model.calculate_G_4_repeated(o4, steps=1, samples=1, rows=M.Rows(rows_per_entry=1))
    with pytest.raises(ValueError, match='rows_per_entry=4'):
        model.calculate_G_4_repeated(o4[:6], steps=1, samples=1, rows=M.Rows(rows_per_entry=4))
    ids = torch.tensor(IDS, dtype=torch.int32, device=model.device)
    with pytest.raises(RuntimeError, match='ids'):                                             # 3 ids for 6 entries
        model.calculate_G_repeated(o4, model.pi_one_hot.repeat(GAMES, 1), rows=M.Rows(ids=ids, rows_per_entry=4))
    with pytest.raises(RuntimeError, match='divide'):
        model.model_down.encoder(frames[:5], rows=M.Rows(ids=ids[:1], rows_per_entry=4))
    with pytest.raises(RuntimeError, match='n_total'):                                         # more entries than the un-compacted batch has
        model.model_down.encoder(frames, rows=M.Rows(ids=torch.arange(GAMES, dtype=torch.int32, device=model.device), rows_per_entry=1, n_total=3))
    model.set_option('check_rows', 1)
    try:
        with pytest.raises(RuntimeError, match='efe_rollout_rows.*outside'):
            model.calculate_G_repeated(o4[ROWS4], model.pi_one_hot.repeat(3, 1), rows=M.Rows(ids=ids, rows_per_entry=4, n_total=5))
        with pytest.raises(RuntimeError, match='efe_encoder_rows.*outside'):
            model.model_down.encoder(frames[IDS], rows=M.Rows(ids=ids, rows_per_entry=1, n_total=5))
    finally:
        model.set_option('check_rows', 0)
    # a refusal names the entry point the caller used
    from daimc_amd import _lib
    from daimc_amd.model import _ptr
    e, nz = model._ready(), _lib.EfeNoise(model.seed, STAGE, 6, 0, 0)
    G = torch.empty(4, device=model.device)
    last = lambda: e.lib.efe_last_error(e.ctx).decode()
    assert e.lib.efe_rollout_rows(e.ctx, _ptr(o4), _ptr(model.pi_one_hot), 0, 1, 1, 0, 0, C.byref(nz), None, None, _ptr(G), None, None, e.stream()) == 1
    assert last() == 'efe_rollout_rows: bad arguments'
    assert e.lib.efe_rollout(e.ctx, _ptr(o4), _ptr(model.pi_one_hot), 0, 1, 1, 0, 0, C.byref(nz), None, _ptr(G), None, None, e.stream()) == 1
    assert last() == 'efe_rollout: bad arguments'
    assert e.lib.efe_encoder_rows(e.ctx, None, 4, C.byref(nz), None, None, None, _ptr(G), None, e.stream()) == 1
    assert last() == 'efe_encoder_rows: bad arguments'
    assert e.lib.efe_encoder(e.ctx, None, 4, C.byref(nz), None, None, _ptr(G), None, e.stream()) == 1
    assert last() == 'efe_encoder: bad arguments'
    g = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, colour_channels=1, resolution=32, device='cuda:0', seed=1)
    o = torch.rand(4, 1, 32, 32, device=g.device)
    i2 = torch.tensor([1, 0, 3, 2], dtype=torch.int32, device=g.device)
    with pytest.raises(RuntimeError, match='efe_encoder_rows.*geometry'):
        g.model_down.encoder(o, rows=M.Rows(ids=i2, rows_per_entry=1, n_total=4))
    with pytest.raises(RuntimeError, match='efe_rollout_rows.*geometry'):
        g.calculate_G_repeated(o, g.pi_one_hot, rows=M.Rows(ids=i2, rows_per_entry=1, n_total=4))
    g.model_down.encoder(o)                                                                    # without rows the generic path still runs
