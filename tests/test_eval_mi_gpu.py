"""GPU tests (-m gpu) of the mutual-information table: efe_eval_mi (csrc/eval_mi.hip) through loss.eval_mutual_info against the numpy
restatement of tests/eval_mi_ref.py, and Trainer.report(mutual_info=True) against a twin.

What is compared.  The restatement replays the kernels' order of the three column sums, so the prepared columns are the bits the kernels
form and the neighbour counts nx, ny are compared EXACTLY.  The score: `out` is within 1 fp32 ulp of float32(restatement).  For a score of
ordinary size the fp64 error of the psi sums (at most M 2^-53 max psi ~ 1e-11) is far below the spacing of fp32 whatever their order, and
one ulp covers a rounding boundary; where the true score is exactly 0 (M = 4 at k = 3, constant columns) step 5 cancels to rounding noise,
which only the same order reproduces, so the restatement replays the kernels' order of step 5 as well (its psi is the engine's table).
Sizes: the sweep gives a workgroup 256 points and stages 256 points j at a time (kernels.h EVAL_MI_POINTS), so 255, 256, 257
stand next to the issue's 4, 5, 63, 1023, 1024, 1025; 8192 is the cap.  Noise is injected unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_mi_ref as R
from train_common import c, model_for

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MS = (4, 5, 63, 255, 256, 257, 1023, 1024, 1025)
KS = (1, 3, 4)


def L():
    import daimc_amd
    return daimc_amd.loss


_DATA, _REF = {}, {}


def data(M):
    """one synthetic batch per size (host arrays, never changed): latents of which some follow a factor, the game's factor columns,
    injected normals [60, 2, M]"""
    if M not in _DATA:
        r = np.random.RandomState(2000 + M)
        S = np.stack(R.factor_columns(r, M), 1)
        s0 = r.randn(M, 10)
        s0[:, 3] += 0.2 * S[:, 3]
        s0[:, 7] = S[:, 2] + 0.01 * r.randn(M)
        _DATA[M] = (np.ascontiguousarray(s0, dtype=np.float32), np.ascontiguousarray(S, dtype=np.float32), r.standard_normal((R.PAIRS, 2, M)))
    return _DATA[M]


def ref(M):
    """the restatement of data(M) in the kernels' sum order, every admissible k of KS in one sweep, computed once"""
    if M not in _REF:
        s0, S, noise = data(M)
        _REF[M] = R.table(s0, S, noise, tuple(k for k in KS if k < M), 'device')
    return _REF[M]


def run(s0, S, noise=None, k=3, want_counts=True, **kw):
    """-> (out fp32 [60], counts int32 [60, 2, M] or None) as numpy"""
    M = len(s0)
    cnt = torch.full((R.PAIRS, 2, M), -7, dtype=torch.int32, device=DEV) if want_counts else None
    out = L().eval_mutual_info(torch.as_tensor(s0).to(DEV), torch.as_tensor(S).to(DEV), n_neighbors=k, noise=noise, counts=cnt, **kw)
    assert tuple(out.shape) == (R.PAIRS,) and out.dtype == torch.float32 and out.is_cuda
    return c(out), (c(cnt) if want_counts else None)


def check(tag, out, counts, ref_mi, ref_counts, pairs=None):
    pairs = list(range(R.PAIRS)) if pairs is None else list(pairs)
    if counts is not None:
        wrong = [p for p in pairs if not np.array_equal(counts[p], ref_counts[p])]
        assert not wrong, (tag, 'counts differ in pairs', wrong[:8])
    ulps = R.ulp_distance(out[pairs], ref_mi[pairs].astype(np.float32))
    print(f'{tag}: largest |out - float32(restatement)| {int(ulps.max())} ulp; MI in [{np.nanmin(out[pairs]):.4f}, {np.nanmax(out[pairs]):.4f}]')
    assert ulps.max() <= 1, (tag, [(p, out[p], ref_mi[p]) for p in pairs if R.ulp_distance(out[p], np.float32(ref_mi[p])) > 1][:8])


# ---- 1. counts and scores over the shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,k', [(M, k) for M in MS for k in KS if k < M])
def test_counts_and_scores(M, k):
    s0, S, noise = data(M)
    out, counts = run(s0, S, noise, k)
    ref_mi, ref_counts = ref(M)[k]
    check(f'M {M} k {k}', out, counts, ref_mi, ref_counts)
    assert np.isfinite(out).all() and (out >= 0).all()
    if M >= 255:                                        # latent 7 follows factor 2 closely, latent 0 follows nothing
        assert out[7 * 6 + 2] > 1.0 > out[0 * 6 + 2]


def test_cap():
    M, k, pairs = 8192, 3, (3, 20, 44, 59)
    s0, S, noise = data(M)
    out, counts = run(s0, S, noise, k)
    got = R.table(s0, S, noise, (k,), 'device', pairs=pairs)[k]
    check(f'M {M} k {k} pairs {pairs}', out, counts, got[0], got[1], pairs)
    assert np.isfinite(out).all() and (out >= 0).all()
    assert (counts >= 0).all() and (counts < M).all()


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', (5, 257))
def test_exact_ties(M):
    """all-zero noise on integer columns: ties everywhere and radius 0 where a point has k exact twins; a constant factor (the reward is
    usually all zero), a constant latent, and a latent identical to a factor"""
    r = np.random.RandomState(M)
    S = np.stack([r.randint(0, n, M) for n in (3, 6, 40, 32, 32)] + [np.zeros(M)], 1).astype(np.float32)
    s0 = r.randint(0, 4, (M, 10)).astype(np.float32)
    s0[:, 9] = 0.25                                     # a dead latent
    s0[:, 8] = S[:, 3]                                  # two identical columns: pair (8, 3)
    noise = np.zeros((R.PAIRS, 2, M))
    for k in (k for k in KS if k < M):
        out, counts = run(s0, S, noise, k)
        ref_mi, ref_counts = R.table(s0, S, noise, (k,), 'device')[k]
        check(f'ties M {M} k {k}', out, counts, ref_mi, ref_counts)
        assert np.isfinite(out).all()
        assert (counts[9 * 6 + 5] == M - 1).all()       # both columns constant: every other point is within radius 0
        assert np.array_equal(counts[8 * 6 + 3, 0], counts[8 * 6 + 3, 1])


# ---- 3. row order ----------------------------------------------------------------------------------------------------------------------
def test_row_order():
    """M = 512 rows of values on a 2^-6 grid: the mean and the sum of squared deviations are exact in any order, so a permutation of the
    rows changes no sigma; the counts follow the permutation and the scores stay within 1 ulp (their sums of psi change order)"""
    M, k = 512, 3
    r = np.random.RandomState(9)
    S = np.stack(R.factor_columns(r, M), 1)
    S[:, 5] = np.round(S[:, 5] * 64) / 64
    s0 = np.clip(np.round(r.randn(M, 10) * 64) / 64, -4, 4)
    s0[:, 7] = S[:, 2] + np.round(r.randn(M) * 4) / 64
    s0, S = s0.astype(np.float32), S.astype(np.float32)
    noise = r.standard_normal((R.PAIRS, 2, M))
    perm = r.permutation(M)
    out, counts = run(s0, S, noise, k)
    out_p, counts_p = run(s0[perm], S[perm], np.ascontiguousarray(noise[:, :, perm]), k)
    ref_mi, ref_counts = R.table(s0[perm], S[perm], noise[:, :, perm], (k,), 'device')[k]
    check('permuted rows', out_p, counts_p, ref_mi, ref_counts)
    assert np.array_equal(counts_p, counts[:, :, perm])
    ulps = R.ulp_distance(out, out_p)
    print('row order: largest change of a score', int(ulps.max()), 'ulp')
    assert ulps.max() <= 1


# ---- 4. non-finite input ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['nan', 'inf'])
def test_nonfinite(what):
    M, k = 65, 3
    v = np.float32('nan') if what == 'nan' else np.float32('inf')
    s0, S, noise = data(M)
    clean, _ = run(s0, S, noise, k, want_counts=False)
    assert np.isfinite(clean).all()
    bad_lat, bad_fac, bad_noise = s0.copy(), S.copy(), noise.copy()
    bad_lat[40, 3], bad_fac[64, 4], bad_noise[17, 1, 5] = v, -v, v
    for tag, args, hit in (('latent 3', (bad_lat, S, noise), [3 * 6 + f for f in range(6)]),
                           ('factor 4', (s0, bad_fac, noise), [l * 6 + 4 for l in range(10)]),
                           ('noise of pair 17', (s0, S, bad_noise), [17])):
        got, _ = run(*args, k, want_counts=False)
        rest = [p for p in range(R.PAIRS) if p not in hit]
        print(what, tag, '->', got[hit])
        assert np.isnan(got[hit]).all(), (what, tag)
        assert got[rest].tobytes() == clean[rest].tobytes(), (what, tag)


# ---- 5. device noise -------------------------------------------------------------------------------------------------------------------
def test_device_noise():
    from oracle import philox as PX
    M, k, seed, stage = 257, 3, 0x1234567890abcdef, 41
    s0, S, _ = data(M)
    a, ca = run(s0, S, None, k, seed=seed, stage=stage)
    b, cb = run(s0, S, None, k, seed=seed, stage=stage)
    assert a.tobytes() == b.tobytes() and np.array_equal(ca, cb)                          # a function of its arguments alone
    other, _ = run(s0, S, None, k, seed=seed + 1, stage=stage)
    assert other.tobytes() != a.tobytes()
    # The mirror's normals differ from the device's in the last bits of an fp32 (another libm), which moves a prepared value by one fp64
    # step now and then; on the tied factor columns, where the jitter alone orders the points, such a step can flip a count.  The chance
    # grows with M^2, so this comparison takes the smallest batch of the shapes that still has ties in every factor column.
    Ms = 63
    s0s, Ss, _ = data(Ms)
    dev_out, _ = run(s0s, Ss, None, k, seed=seed, stage=stage)
    mirror = np.stack([np.stack([PX.normals(seed, Ms, 1, p, w, stage, tag=0x80)[:, 0] for w in (0, 1)]) for p in range(R.PAIRS)]).astype(np.float64)
    inj, _ = run(s0s, Ss, mirror, k)
    ulps = R.ulp_distance(dev_out, inj)
    print('device noise against the injected Philox mirror:', int(ulps.max()), 'ulp')
    assert ulps.max() <= 1
    # zero-variance inputs: the prepared columns are a constant plus the jitter, so the counts depend on the drawn normals alone
    flat0, flatS = np.full((M, 10), 0.5, np.float32), np.full((M, 6), 2.0, np.float32)
    _, c1 = run(flat0, flatS, None, k, seed=seed, stage=stage)
    _, c2 = run(flat0, flatS, None, k, seed=seed, stage=stage + 1)
    assert not np.array_equal(c1, c2) and (c1 >= k - 1).all() and (c1 < M).all()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def raw(e, s0, S, M, out, k=3, null_in=False):
    """efe_eval_mi through ctypes -> (return code, message)"""
    from daimc_amd import _lib as LB
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    mi = LB.EfeEvalMiIn(p(s0), p(S), None, k, 0, 0)
    rc = e.lib.efe_eval_mi(e.ctx, None if null_in else C.byref(mi), M, p(out), None, e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


def test_refusals_write_nothing():
    M = 12
    s0h, Sh, _ = data(63)
    s0, S = torch.as_tensor(s0h[:M]).to(DEV), torch.as_tensor(Sh[:M]).to(DEV)
    out = torch.full((R.PAIRS,), 777.0, device=DEV)
    big0, bigS = torch.zeros(8193, 10, device=DEV), torch.zeros(8193, 6, device=DEV)
    cases = {'k = 0': lambda: L().eval_mutual_info(s0, S, n_neighbors=0, out=out), 'k = 5': lambda: L().eval_mutual_info(s0, S, n_neighbors=5, out=out),
             'M = k': lambda: L().eval_mutual_info(s0[:3], S[:3], n_neighbors=3, out=out),
             'M = 8193': lambda: L().eval_mutual_info(big0, bigS, out=out)}
    for tag, call in cases.items():
        with pytest.raises(RuntimeError, match='efe_eval_mi') as ei:
            call()
        print(tag, '->', str(ei.value).splitlines()[0])
        assert (c(out) == 777.0).all(), tag
    e = L()._stats_engine(DEV)
    for tag, (a0, aS, m, o, k, null_in, word) in {
            'NULL in': (s0, S, M, out, 3, True, 'in and out'), 'NULL out': (s0, S, M, None, 3, False, 'in and out'),
            'NULL s0': (None, S, M, out, 3, False, 's0'), 'NULL S_real': (s0, None, M, out, 3, False, 'S_real'),
            'k = 0': (s0, S, M, out, 0, False, 'n_neighbors'), 'k = 5': (s0, S, M, out, 5, False, 'n_neighbors'),
            'M = k': (s0, S, 3, out, 3, False, 'n_neighbors + 1'), 'M = 0': (s0, S, 0, out, 1, False, 'n_neighbors + 1'),
            'M = 8193': (big0, bigS, 8193, out, 3, False, 'above the cap')}.items():
        rc, msg = raw(e, a0, aS, m, o, k, null_in)
        print(tag, '->', rc, msg)
        assert rc == 1 and 'efe_eval_mi' in msg and word in msg, (tag, msg)
        assert (c(out) == 777.0).all(), tag
    rc, msg = raw(e, s0, S, M, out)                     # and the same arguments, whole, are accepted: the context still works
    assert rc == 0 and np.isfinite(c(out)).all() and not (c(out) == 777.0).any()
    buf = torch.full((R.PAIRS + 64,), 777.0, device=DEV)
    view = L().eval_mutual_info(s0, S, seed=3, out=buf[32:92])
    h = c(buf)
    assert view.data_ptr() == buf[32:92].data_ptr() and (h[:32] == 777.0).all() and (h[92:] == 777.0).all() and np.isfinite(h[32:92]).all()


# ---- 7. Trainer.report -----------------------------------------------------------------------------------------------------------------
def trainer():
    import daimc_amd
    m = model_for('g115', fresh=True)
    games = daimc_amd.Game(8, model=m, seed=3)
    test = daimc_amd.Game(64, model=m, seed=4)
    gen = torch.Generator(device=DEV).manual_seed(11)
    return m, test, gen, daimc_amd.Trainer(m, games, generator=gen)


def test_trainer_report():
    import daimc_amd
    from daimc_amd.train import REPORT_KEYS
    ma, test_a, _, ta = trainer()
    mb, test_b, gen_b, tb = trainer()
    ta.epoch(1)
    tb.epoch(1)
    rep = ta.report(test_a, mutual_info=True)
    assert tuple(rep) == REPORT_KEYS + ('mutual_info',)
    mi = rep['mutual_info']
    assert mi.shape == (10, 6) and mi.dtype == np.float32 and np.isfinite(mi).all() and (mi >= 0).all()
    # the twin takes the same steps by hand: the evaluation batch with its true factors, free_energy at the report's omega
    a, _, _, d = tb.omega_params
    o0, o1, pi0, S0_real, _ = daimc_amd.make_batch_dsprites_random(test_b, tb.repeats, gen_b)
    pi0 = mb._ready().tensor(pi0, (-1, mb.pi_dim))
    fe = daimc_amd.free_energy(mb, o0, o1, pi0, torch.log(pi0 + 1e-15), omega=a / 2.0 + d, omega_params=tb.omega_params)
    assert tb.rounds_done == 1
    want = c(daimc_amd.eval_mutual_info(fe.s0, S0_real, seed=mb.seed, stage=tb.rounds_done))
    print('mutual_info of the report, largest entry', mi.max(), 'at', np.unravel_index(mi.argmax(), mi.shape))
    assert mi.reshape(-1).tobytes() == want.tobytes()
    assert np.array_equal(rep['spearman'].shape, (10, 6))
    rep2 = ta.report(test_a)                            # the default call is unchanged
    assert tuple(rep2) == REPORT_KEYS and 'mutual_info' not in rep2
