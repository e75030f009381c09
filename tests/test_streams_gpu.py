"""GPU tests (-m gpu) of the stream contract of include/efe_engine.h ("threading / streams"), INTEGRATION.md and csrc/engine.h (`Call`):
every entry point is stream-ordered on the stream it is given; a call on another stream than the previous call first waits for that call's
last kernel (done_ev), so the arena reset at the start of a call never races with work in flight; two contexts share nothing; host threads
may share a context.  Every comparison is of bits: the same kernels on the same inputs, on another stream.

The delay.  `_delay` blocks a stream for about DELAY_MS with torch.cuda._sleep, sized once from a probe timed with events.  The 50 ms are no
tolerance: they have to outlast the host-side issue of one warmed-up call (well under a millisecond), and every test asserts that premise --
the event recorded behind the delay has not completed when the engine call returns, so the whole call was enqueued while its stream was
still blocked.  Before a blocked call the same call runs once on the same stream with OTHER inputs: arena growth, torch's allocator, the
dec_bf refresh behind an optimiser step would synchronise, and the scratch then holds valid data of another call.  The module's models run
with option poison = 255 (every call starts on scratch of 0xff bytes: an early read is a NaN, not a plausible number), so a launch, memset
or copy put on stream 0 by mistake runs a whole delay ahead of its producers and shows.  gamma / beta_s / beta_o of a model that
evaluates the free energy are Python floats, as daimc_amd.train.Trainer keeps them: loss.py would fetch a 0-d device tensor on the current
stream, i.e. wait for the delay.

1. a call on a side stream is the call on the default stream -- per entry-point family at the smallest shape that reaches its launch path:
   decoder 24 images (k_dec_a_s, k_dec_b4<4>), 132 images with dec_ab_grid = 3 (k_dec_ab: ticket memset, slot reuse) and with
   dec_fuse_ab = 0 (k_dec_a + k_dec_b4<1>); encoder 200 rows; calculate_G M = 6, S = 3 with its parts; calculate_G_repeated 2 rows x 1 step
   x 22 samples with the stored images; simulate_batch depth 4 at E = 3, 16 (split chain) and 20 (one workgroup); resolution 32,
   calculate_G M = 5; free_energy and train_step at M = 1 on fresh twins; efe_eval_stats at M = 1 and 12, efe_eval_mi at M = 4 (k = 1) and
   5 (k = 3); the lock-step planner at E = 8, 8 repeats, overlap on, with a side stream as the current stream.  The model's methods go
   through torch.ops.efe.* (csrc/torch_ops.cpp takes torch's current stream itself); calculate_g, rollout and simulate also run through
   ctypes with the stream as an argument, against the bits of the custom op.
2. a stream switch orders the arena: A behind the delay on s1, B at once on s2; when B's event has completed, A's has.
3. a model and its replica() on two streams, released together, equal the calls run alone.
4. two host threads on one context, each with its own stream."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DELAY_MS = 50.0
OPTION_DEFAULTS = {'dec_fuse_ab': 1, 'dec_ab_grid': 0}


def L():
    import daimc_amd
    return daimc_amd.loss


# ---- models ------------------------------------------------------------------------------------------------------------------------------
def _new_model(weights, resolution=64, gamma=0.0, seed=11):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, gamma, 1.0, 1.0, colour_channels=1, resolution=resolution, device=DEV, seed=seed, init_weights=False)
    m.load_flat_weights(weights)
    m.gamma, m.beta_s, m.beta_o = float(gamma), 1.0, 1.0        # Python floats (see the module docstring)
    m.set_option('poison', 255)
    return m


@pytest.fixture(scope='module')
def model(weights_cache):
    m = _new_model(weights_cache(1234, 1.15))
    yield m
    torch.cuda.synchronize()
    m.set_option('poison', -1)


@pytest.fixture(scope='module')
def model32():
    from oracle import synth
    m = _new_model(synth.make_weights(1234, 1.15, 4, 1, 32), resolution=32)
    yield m
    torch.cuda.synchronize()
    m.set_option('poison', -1)


def _trainable(weights):
    """a fresh model with its three optimisers (the learning rates of tests/test_train_step_gpu.py)"""
    import daimc_amd
    m = _new_model(weights, gamma=0.5, seed=7)
    return m, {'top': daimc_amd.Adam(m.model_top, lr=1e-4), 'mid': daimc_amd.Adam(m.model_mid, lr=1e-4), 'down': daimc_amd.Adam(m.model_down, lr=1e-3)}


class _options:
    """engine options for the length of a block, the defaults back on exit"""

    def __init__(self, m, **opts):
        self.m, self.opts = m, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.m.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.m.set_option(k, OPTION_DEFAULTS[k])


# ---- the delay ---------------------------------------------------------------------------------------------------------------------------
_CYCLES = []


def _delay_cycles():
    """the argument of torch.cuda._sleep that lasts DELAY_MS, from a probe of at least 2 ms timed with events (once per process)"""
    if not _CYCLES:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        n, ms = 1 << 20, 0.0
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 2.0 or n >= 1 << 34:
                break
            n *= 4
        assert ms >= 2.0, f'torch.cuda._sleep({n}) lasted {ms} ms: no delay can be sized from it'
        _CYCLES.append(int(n * DELAY_MS / ms) + 1)
        print(f'delay: torch.cuda._sleep({n}) lasted {ms:.3f} ms; {DELAY_MS} ms = {_CYCLES[0]} cycles')
    return _CYCLES[0]


def _delay(stream):
    """blocks `stream` (the current one) for DELAY_MS -> the event behind the delay: while query() is False the stream is still blocked"""
    torch.cuda._sleep(_delay_cycles())
    gate = torch.cuda.Event()
    gate.record(stream)
    return gate


def _streams(n):
    """n fresh streams that wait for what the default stream has queued (the inputs)"""
    _delay_cycles()
    out = [torch.cuda.Stream(device=DEV) for _ in range(n)]
    for s in out:
        s.wait_stream(torch.cuda.current_stream(DEV))
    return out


PREMISE = 'premise: the delay had run out before the call was enqueued (a synchronisation inside the call, or a stalled host)'


# ---- bits --------------------------------------------------------------------------------------------------------------------------------
def _snap(x):
    """every tensor of a nested result on the host, in order (synchronises)"""
    if isinstance(x, torch.Tensor):
        return [np.ascontiguousarray(x.detach().cpu().numpy())]
    if isinstance(x, dict):
        return [a for k in x for a in _snap(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for v in x for a in _snap(v)]
    return [x]


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if not isinstance(w, np.ndarray):
            assert g == w or (g is None and w is None), (what, i, g, w)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)) if g.size else []
            raise AssertionError(f'{what}: output {i} of shape {g.shape}: {len(bad)} of {g.nbytes} bytes differ, the first at byte {bad[0] if len(bad) else -1}')


def _finite(snap, what):
    for i, a in enumerate(snap):
        if isinstance(a, np.ndarray) and a.dtype.kind == 'f':
            assert np.isfinite(a).all(), (what, i, 'the reference itself is not finite')


# ---- inputs (made on the default stream, before any side stream waits for it) ----------------------------------------------------------------
def _states(seed, n):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1.5, 1.5, (n, 10)).astype(np.float32)).to(DEV)


def _actions(seed, n):
    return torch.from_numpy(np.eye(4, dtype=np.float32)[np.random.RandomState(seed).randint(0, 4, n)]).to(DEV)


def _frames(seed, n):
    from oracle import synth
    return torch.from_numpy(synth.make_frames(seed, n)).to(DEV)


def _fe_batch(seed, M):
    r = np.random.RandomState(seed)
    lp = torch.log_softmax(torch.from_numpy(r.randn(M, 4).astype(np.float32)), 1).to(DEV)
    return {'o0': _frames(seed, M), 'o1': _frames(seed + 1, M), 'pi0': _actions(seed + 2, M), 'lp': lp}


def _stats_batch(seed, M):
    """the four input groups of efe_eval_stats: (fe mapping with qs1 and s0, S_real, (o1_r, po1_r))"""
    r = np.random.RandomState(seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    fe = {k: t(r.gamma(2.0, 1.0, M)) for k in L().EVAL_FE_ARRAYS[:7]}
    fe.update(kl_s_anal=t(r.gamma(2.0, 0.3, (M, 10))), kl_naive_anal=t(r.randn(M, 10)), kl_pi_anal=t(r.randn(M, 4)), qs1=t(r.randn(M, 10)),
              s0=t(r.randn(M, 10)))
    S = t(np.stack([r.randint(0, k, M) for k in (3, 6, 40, 32, 32)] + [r.uniform(-1, 1, M)], 1))
    return {'fe': fe, 'S': S, 'rw': (t(r.rand(M, 1, 64, 64) < 0.5), t(r.rand(M, 1, 64, 64)))}


def _mi_batch(seed, M, k):
    r = np.random.RandomState(seed)
    S = np.stack([r.randint(0, n, M) for n in (3, 6, 40, 32, 32)] + [r.uniform(-1, 1, M)], 1).astype(np.float32)
    return {'s0': torch.from_numpy(r.randn(M, 10).astype(np.float32)).to(DEV), 'S': torch.from_numpy(S).to(DEV), 'k': k, 't': 40 + seed}


# ---- the calls: run(x) -> device tensors; make(i) -> the inputs of variant i (0: the compared call, 1: the other data) --------------------------
def _decoder(m, n):
    return (lambda x: m.model_down.decoder(x['s'], stage=x['t'])), (lambda i: {'s': _states(100 + n + i, n), 't': 3 + i})


def _encoder(m, n):
    return (lambda x: m.model_down.encoder_with_sample(x['o'], stage=x['t'])), (lambda i: {'o': _frames(200 + i, n), 't': 5 + i})


def _calculate_g(m, M, S):
    def run(x):
        parts = []
        r = m.calculate_G(x['s0'], x['pi'], samples=S, stage=x['t'], _parts=parts)
        return list(r) + parts
    return run, (lambda i: {'s0': _states(300 + M + i, M), 'pi': _actions(310 + i, M), 't': 7 + i})


def _rollout(m, M, steps, S):
    return ((lambda x: m.calculate_G_repeated(x['o'], x['pi'], steps=steps, samples=S, stage=x['t'])),
            (lambda i: {'o': _frames(23 + i, M), 'pi': _actions(320 + i, M), 't': 8 + 2 * i}))


def _simulate(m, E, depth=4):
    return (lambda x: m.simulate_batch(x['s'], depth, stage=x['t'])), (lambda i: {'s': _states(400 + E + i, E), 't': 11 + i})


def _eval_mi(engine, M, k):
    return ((lambda x: L().eval_mutual_info(x['s0'], x['S'], n_neighbors=x['k'], seed=77, stage=x['t'], engine=engine)),
            (lambda i: _mi_batch(500 + i, M, k)))


def _side(run, make, premise=True):
    """run(make(0)) on a fresh side stream behind the delay, after run(make(1)) on that stream -> (host bits, whether the call returned while
    its stream was still blocked); drains the device on every exit"""
    x, other = make(0), make(1)
    (s,) = _streams(1)
    try:
        with torch.cuda.stream(s):
            run(other)
            gate = _delay(s)
            out = run(x)
            blocked = not gate.query()
        s.synchronize()
        got = _snap(out)
    finally:
        torch.cuda.synchronize()
    assert blocked or not premise, PREMISE
    return got


def _default(run, make, what, nan_ok=False):
    ref = _snap(run(make(0)))
    if not nan_ok:
        _finite(ref, what)
    assert not all(np.array_equal(a, b) for a, b in zip(ref, _snap(run(make(1)))) if isinstance(a, np.ndarray)), (what, 'the other inputs give the same bits')
    return ref


# ---- 1. a call on a side stream is the call on the default stream --------------------------------------------------------------------------
FAMILIES = {
    'decoder_24': (lambda m: _decoder(m, 24), {}),
    'decoder_132_fused_grid_3': (lambda m: _decoder(m, 132), {'dec_fuse_ab': 1, 'dec_ab_grid': 3}),
    'decoder_132_two_launches': (lambda m: _decoder(m, 132), {'dec_fuse_ab': 0}),
    'encoder_200': (lambda m: _encoder(m, 200), {}),
    'calculate_G_6x3': (lambda m: _calculate_g(m, 6, 3), {}),
    'rollout_2x1x22': (lambda m: _rollout(m, 2, 1, 22), {}),
    'simulate_E3': (lambda m: _simulate(m, 3), {}),
    'simulate_E16': (lambda m: _simulate(m, 16), {}),
    'simulate_E20': (lambda m: _simulate(m, 20), {}),
}


@pytest.mark.parametrize('family', list(FAMILIES))
def test_side_stream_equals_default_stream(model, family):
    build, opts = FAMILIES[family]
    run, make = build(model)
    with _options(model, **opts):
        ref = _default(run, make, family)
        _same(_side(run, make), ref, family)


def test_side_stream_generic_geometry(model32):
    run, make = _calculate_g(model32, 5, 2)
    ref = _default(run, make, 'resolution 32')
    _same(_side(run, make), ref, 'resolution 32')


def _c_calls(m):
    """calculate_g, rollout and simulate as (custom op, the same C call through ctypes with the stream as an argument, inputs)"""
    from daimc_amd import _lib
    e, p = m._ready(), _lib.ptr
    nz = lambda x: C.byref(_lib.EfeNoise(m.seed, x['t'], 0, 0, m.row_offset))
    like = lambda ts: [torch.full_like(t, float('nan')) for t in ts]

    def g_op(x):
        return e.ops.calculate_g(e.h, x['s0'], x['pi'], 3, False, m._seed64(), x['t'], m.row_offset, None, None, None, 1, 0)

    def g_c(x):
        out = like(x['like'])
        e.check(e.lib.efe_calculate_g(e.ctx, p(x['s0']), p(x['pi']), x['s0'].shape[0], 3, 0, nz(x), None, *[p(t) for t in out], e.stream()))
        return out

    def r_op(x):
        return e.ops.rollout(e.h, x['o'], x['pi'], 1, 22, False, False, m._seed64(), x['t'], m.row_offset, None)

    def r_c(x):
        out = like(x['like'])
        e.check(e.lib.efe_rollout(e.ctx, p(x['o']), p(x['pi']), x['o'].shape[0], 1, 22, 0, 0, nz(x), None, *[p(t) for t in out], e.stream()))
        return out

    def s_op(x):
        return e.ops.simulate(e.h, x['s'], 4, False, m._seed64(), x['t'], m.row_offset, None, None, None, None, 0)

    def s_c(x):
        out = like(x['like'])
        e.check(e.lib.efe_simulate(e.ctx, p(x['s']), x['s'].shape[0], 4, 0, nz(x), None, None, *[p(t) for t in out], e.stream()))
        return out

    return {'calculate_g': (g_op, g_c, _calculate_g(m, 6, 3)[1]), 'rollout': (r_op, r_c, _rollout(m, 2, 1, 22)[1]),
            'simulate_E16': (s_op, s_c, _simulate(m, 16)[1])}


@pytest.mark.parametrize('name', ['calculate_g', 'rollout', 'simulate_E16'])
def test_side_stream_through_ctypes_equals_the_custom_op(model, name):
    """the ctypes binding hands the engine e.stream(), the custom op asks torch for the current stream itself: both on a side stream, against
    the custom op on the default stream"""
    op, c_call, make = _c_calls(model)[name]
    ref_dev = op(make(0))
    ref = _default(op, make, name)
    with_like = lambda i: dict(make(i), like=ref_dev)
    _same(_side(c_call, with_like), ref, name + ' through ctypes')
    _same(_side(op, make), ref, name + ' through torch.ops.efe')


def test_side_stream_free_energy(weights_cache):
    import daimc_amd
    m = _new_model(weights_cache(1234, 1.15), gamma=0.5, seed=7)
    run = lambda x: daimc_amd.free_energy(m, x['o0'], x['o1'], x['pi0'], x['lp'], stage=x['t'])
    make = lambda i: dict(_fe_batch(600 + 10 * i, 1), t=5 + i)
    ref = _default(run, make, 'free_energy')
    _same(_side(run, make), ref, 'free_energy M = 1')


def test_side_stream_train_step(weights_cache):
    """two fresh models with the same weights, one per stream: a warming step on the other batch, then the compared step; the returned terms
    and every weight read back"""
    w = weights_cache(1234, 1.15)
    (ma, oa), (mb, ob) = _trainable(w), _trainable(w)
    make = lambda i: dict(_fe_batch(700 + 10 * i, 1), t=5 + i)
    step = lambda m, o: (lambda x: L().train_step(m, x['o0'], x['o1'], x['pi0'], x['lp'], o, stage=x['t']))
    step(ma, oa)(make(1))
    ref = _snap(step(ma, oa)(make(0)))
    _finite(ref[:-1], 'train_step')
    assert np.isfinite(ref[-1][:7]).all() and np.isnan(ref[-1][7])        # (means: the standard deviation of omega over one row is NaN)
    got = _side(step(mb, ob), make)
    _same(got, ref, 'train_step M = 1')
    for part in ('top', 'mid', 'down'):
        sa, sb = getattr(ma, 'model_' + part).state_dict(), getattr(mb, 'model_' + part).state_dict()
        _same(_snap(sb), _snap(sa), 'weights of ' + part)
    assert [o._step for o in ob.values()] == [2, 2, 2]


@pytest.mark.parametrize('M', [1, 12])
def test_side_stream_eval_stats(M):
    run = lambda x: L().eval_stats(x['fe'], x['S'], x['rw'])
    make = lambda i: _stats_batch(800 + M + 100 * i, M)
    ref = _default(run, make, 'eval_stats', nan_ok=True)        # (one row: numpy's NaN fields)
    if M > 10:
        _finite(ref, 'eval_stats')
    _same(_side(run, make), ref, f'eval_stats M = {M}')


@pytest.mark.parametrize('M,k', [(4, 1), (5, 3)])
def test_side_stream_eval_mi(M, k):
    run, make = _eval_mi(None, M, k)
    ref = _default(run, make, 'eval_mi')
    _same(_side(run, make), ref, f'eval_mi M = {M} k = {k}')


def test_planner_with_a_side_stream_as_the_current_stream(model):
    """active_inference_mcts_batch reads the history back as it goes, so no premise can hold over the whole decision: the delay only puts
    whatever the planner would launch on stream 0 ahead of the rest.  E = 8, 8 repeats, the simulations on the planner's own second stream
    through the replica context"""
    import daimc_amd
    p = daimc_amd.MCTS_Params()
    p.repeats, p.simulation_depth, p.use_means, p.threshold, p.samples = 8, 3, False, 2.0, 2
    frames = _frames(31, 8)

    def run(_=None):
        model._stage = 100
        out, visits = daimc_amd.active_inference_mcts_batch(model, frames, p, o_shape=(1, 64, 64))
        planner = next(pl for pl in model._planners.values() if pl.E == 8)
        assert planner.overlap and planner.sim_model is not model
        return [list(o) for o in out], visits

    ref = run()
    assert all(len(o[3]) == p.repeats and np.isfinite(o[4]).all() for o in ref[0])
    got = _side(run, lambda i: None, premise=False)
    assert got[:-1] == _snap(ref)[:-1], 'paths, repeats, G history'
    _same(got[-1:], _snap(ref)[-1:], 'root visits')


# ---- 2. a stream switch orders the arena -----------------------------------------------------------------------------------------------------
def _serial(jobs):
    """the warming calls and then the compared calls of `jobs` (run, make) one after another on the default stream -> host bits per job"""
    for run, make in jobs:
        run(make(1))
    return [_snap(run(make(0))) for run, make in jobs]


def _switched(jobs, between=None):
    """jobs[0] behind the delay on its own stream, then the others at once, each on a stream of its own (`between`: a call made on one more
    stream after jobs[0]) -> (bits per job, per job whether it returned while the first stream was blocked, whether the first job's event
    had completed when the last job's event had)"""
    xs, others = [make(0) for _, make in jobs], [make(1) for _, make in jobs]
    streams = _streams(len(jobs) + 1)
    try:
        for s, (run, _), other in zip(streams, jobs, others):
            with torch.cuda.stream(s):
                run(other)
            s.synchronize()                 # (the warming calls never overlap, whatever the engine orders)
        del others
        torch.cuda.synchronize()
        outs, blocked, events = [], [], []
        for i, (s, (run, _)) in enumerate(zip(streams, jobs)):
            with torch.cuda.stream(s):
                if i == 0:
                    gate = _delay(s)
                outs.append(run(xs[i]))
                ev = torch.cuda.Event()
                ev.record(s)
                events.append(ev)
                blocked.append(not gate.query())
            if i == 0 and between is not None:
                with torch.cuda.stream(streams[-1]):
                    between()
        events[-1].synchronize()
        first_done = events[0].query()
        torch.cuda.synchronize()
        return [_snap(o) for o in outs], blocked, first_done
    finally:
        torch.cuda.synchronize()


ORDER = 'the later call on another stream finished before the earlier call: no wait for done_ev'


def test_switch_fused_decoder_then_calculate_g(model):
    jobs = [_decoder(model, 132), _calculate_g(model, 6, 3)]
    with _options(model, dec_fuse_ab=1, dec_ab_grid=3):
        ref = _serial(jobs)
        got, blocked, first_done = _switched(jobs)
    assert all(blocked), PREMISE
    assert first_done, ORDER
    _same(got[0], ref[0], 'A: decoder 132')
    _same(got[1], ref[1], 'B: calculate_G')


def test_switch_calculate_g_then_eval_mi(model):
    """efe_eval_mi opens its scope in the `ordered` mode: no weights, no arena, the same ordering"""
    jobs = [_calculate_g(model, 6, 3), _eval_mi(model._ready(), 5, 3)]
    ref = _serial(jobs)
    got, blocked, first_done = _switched(jobs)
    assert all(blocked), PREMISE
    assert first_done, ORDER
    _same(got[0], ref[0], 'A: calculate_G')
    _same(got[1], ref[1], 'B: eval_mi')


def test_switch_simulate_then_simulate(model):
    """the split chain's exchange buffer and arrival counters (sim_xch, sim_sync) belong to the context, outside the arena: two split
    launches of one context on two streams must not be in flight together"""
    jobs = [_simulate(model, 16), _simulate(model, 3)]
    ref = _serial(jobs)
    got, blocked, first_done = _switched(jobs)
    assert all(blocked), PREMISE
    assert first_done, ORDER
    _same(got[0], ref[0], 'A: simulate E = 16')
    _same(got[1], ref[1], 'B: simulate E = 3')


def test_switch_train_step_then_decoder(weights_cache):
    """B reads the weights A writes: it must be the decoder after the step of a serial run.  (The first decoder pass behind a step fetches
    po_net.19.bias on its stream and waits for it, so B itself returns after A: only A's return is held to the premise.)"""
    w = weights_cache(1234, 1.15)
    make = lambda i: dict(_fe_batch(900 + 10 * i, 1), t=5 + i)
    jobs = []
    for m, o in (_trainable(w), _trainable(w)):
        step = (lambda m, o: (lambda x: L().train_step(m, x['o0'], x['o1'], x['pi0'], x['lp'], o, stage=x['t'])))(m, o)
        jobs.append([(step, make), _decoder(m, 24)])
    ref = _serial(jobs[0])
    got, blocked, first_done = _switched(jobs[1])
    assert blocked[0], PREMISE
    assert first_done, ORDER
    _same(got[0], ref[0], 'A: train_step')
    _same(got[1], ref[1], 'B: the decoder after the step')


def test_switch_across_a_refused_call(model):
    """A on s1 behind the delay, a call with bad arguments on s2 (it returns 1 behind its scope's start), C on s3: C still completes behind A"""
    from daimc_amd import _lib
    e, p = model._ready(), _lib.ptr
    jobs = [_decoder(model, 132), _calculate_g(model, 6, 3)]
    rcs, G, o, pi = [], torch.empty(4, device=DEV), _frames(1, 1), _actions(1, 1)

    def refused():
        nz = _lib.EfeNoise(model.seed, 1, 0, 0, 0)
        rcs.append(e.lib.efe_rollout(e.ctx, p(o), p(pi), 0, 1, 1, 0, 0, C.byref(nz), None, p(G), None, None, e.stream()))
        rcs.append(e.lib.efe_last_error(e.ctx).decode())

    with _options(model, dec_fuse_ab=1, dec_ab_grid=3):
        ref = _serial(jobs)
        got, blocked, first_done = _switched(jobs, between=refused)
    assert rcs == [1, 'efe_rollout: bad arguments'], rcs
    assert all(blocked), PREMISE
    assert first_done, ORDER
    _same(got[0], ref[0], 'A: decoder 132')
    _same(got[1], ref[1], 'C: calculate_G')


def test_same_stream_adds_no_wait(model):
    """two consecutive calls on one stream: the event behind the second completes with no other stream touched, and both are exact"""
    jobs = [_decoder(model, 24), _calculate_g(model, 6, 3)]
    ref = _serial(jobs)
    xs = [make(0) for _, make in jobs]
    (s,) = _streams(1)
    try:
        with torch.cuda.stream(s):
            outs = [run(x) for (run, _), x in zip(jobs, xs)]
            ev = torch.cuda.Event()
            ev.record(s)
        ev.synchronize()
        assert ev.query()
        got = [_snap(o) for o in outs]
    finally:
        torch.cuda.synchronize()
    _same(got[0], ref[0], 'decoder 24')
    _same(got[1], ref[1], 'calculate_G')


# ---- 3. two contexts share nothing ---------------------------------------------------------------------------------------------------------
def test_model_and_replica_on_two_streams(model):
    """396 decoder images (33 rows x 4 samples x 3 passes) on one context beside the split simulation chain (E = 3, E = 16: workgroups that
    spin on their peers under a bounded timeout which poisons the outputs) on the other, both behind one gate; then the roles swapped"""
    replica = model.replica()
    try:
        for big, small in ((model, replica), (replica, model)):
            jobs = [_calculate_g(big, 33, 4), _simulate(small, 3), _simulate(small, 16)]
            alone = [_snap(run(make(0))) for run, make in jobs]
            for a in alone:
                _finite(a, 'alone')
            xs = [make(0) for _, make in jobs]
            others = [make(1) for _, make in jobs]
            s0, s1, s2 = _streams(3)
            try:
                with torch.cuda.stream(s1):
                    jobs[0][0](others[0])
                with torch.cuda.stream(s2):
                    jobs[1][0](others[1])
                    jobs[2][0](others[2])
                torch.cuda.synchronize()
                with torch.cuda.stream(s0):
                    gate = _delay(s0)
                s1.wait_event(gate)
                s2.wait_event(gate)
                with torch.cuda.stream(s1):
                    g = jobs[0][0](xs[0])
                with torch.cuda.stream(s2):
                    sim3 = jobs[1][0](xs[1])
                    sim16 = jobs[2][0](xs[2])
                blocked = not gate.query()
                torch.cuda.synchronize()
                got = [_snap(g), _snap(sim3), _snap(sim16)]
            finally:
                torch.cuda.synchronize()
            assert blocked, PREMISE
            who = 'model' if big is model else 'replica'
            for name, a, b in zip(('calculate_G 33 x 4 on the ' + who, 'simulate E = 3 beside it', 'simulate E = 16 beside it'), got, alone):
                _finite(a, name)
                _same(a, b, name)
    finally:
        torch.cuda.synchronize()
        replica.set_option('poison', -1)


# ---- 4. host threads share a context -----------------------------------------------------------------------------------------------------------
def test_two_host_threads_share_a_context(model):
    """two threads, each with its own stream and 8 calls through ctypes: efe_calculate_g (M = 6, S = 3) and the 24-image efe_decoder"""
    from daimc_amd import _lib
    from daimc_amd.model import PASS_D1
    e, p, N = model._ready(), _lib.ptr, 8
    gx = [{'s0': _states(1000 + i, 6), 'pi': _actions(1100 + i, 6), 't': 20 + i} for i in range(N)]
    dx = [{'s': _states(1200 + i, 24), 't': 40 + i} for i in range(N)]
    g_shapes = [(6,), (3, 6), (6, 10), (6, 10), (6, 1, 64, 64), (2, 6)]
    new = lambda *shape: torch.full(shape, float('nan'), device=DEV)

    def calc(x, out, stream):
        nz = _lib.EfeNoise(model.seed, x['t'], 0, 0, model.row_offset)
        return e.lib.efe_calculate_g(e.ctx, p(x['s0']), p(x['pi']), 6, 3, 0, C.byref(nz), None, *[p(t) for t in out], stream)

    def dec(x, out, stream):
        nz = _lib.EfeNoise(model.seed, x['t'], PASS_D1, 0, model.row_offset)
        return e.lib.efe_decoder(e.ctx, p(x['s']), 24, C.byref(nz), p(out[0]), stream)

    try:
        model.reserve(6, 1, 3)
        serial = []
        for fn, xs, shapes in ((calc, gx, g_shapes), (dec, dx, [(24, 1, 64, 64)])):
            outs = [[new(*s) for s in shapes] for _ in range(N)]
            for x, o in zip(xs, outs):
                e.check(fn(x, o, e.stream()))
            serial.append([_snap(o) for o in outs])
            for o in serial[-1]:
                _finite(o, 'serial')
        grown = model.arena_stats()['grow_count']
        streams = _streams(2)
        outs = [[[new(*s) for s in g_shapes] for _ in range(N)], [[new(24, 1, 64, 64)] for _ in range(N)]]
        torch.cuda.synchronize()
        failures, start = [], threading.Barrier(2)

        def worker(fn, xs, out, stream):
            try:
                handle = C.c_void_p(stream.cuda_stream)
                start.wait()
                for x, o in zip(xs, out):
                    rc = fn(x, o, handle)
                    if rc:
                        failures.append((fn.__name__, rc, e.lib.efe_last_error(e.ctx).decode()))
            except BaseException as ex:                 # (reported by the test's thread)
                failures.append((fn.__name__, repr(ex)))

        threads = [threading.Thread(target=worker, args=a) for a in ((calc, gx, outs[0], streams[0]), (dec, dx, outs[1], streams[1]))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not failures, failures
        for k, name in enumerate(('calculate_g', 'decoder')):
            for i in range(N):
                _same(_snap(outs[k][i]), serial[k][i], f'{name} call {i} of its thread')
        assert model.arena_stats()['grow_count'] == grown
    finally:
        torch.cuda.synchronize()
