"""numpy fp64 restatement of the mutual-information table of the epoch report (csrc/eval_mi.hip, efe_eval_mi): the
Kraskov-Stoegbauer-Grassberger k-nearest-neighbour estimator as scikit-learn's mutual_info_regression defines it for float64 columns,
steps 1-5 of the definition in that file's header, by brute force.  A plain module, like eval_ref.py.

The order of the sums is a parameter: 'numpy' (np.mean's pairwise sums) or 'device' (a replay of csrc/block_sum.h's contract: 256 strided fp64
accumulators, an xor butterfly over each wave of 64, ((w0 + w1) + w2) + w3; for step 5 one such sum per slice of 256 points, the slices in
ascending order).  With 'device' the prepared columns are the bits the kernels form, so the neighbour counts can be compared exactly, and
so is the score, also where it cancels to rounding noise (a true score of 0).  psi is the engine's table in both.  The sweep is chunked
over the points, so 8192 rows fit in memory."""
import numpy as np

PAIRS, FACTORS, LATENTS = 60, 6, 10
TINY = 10.0 * 2.0 ** -52


def factor_columns(r, n):
    """columns drawn like the game's true factors: 3, 6, 40, 32 and 32 values, and a uniform reward (tests/test_eval_report_cpu.py)"""
    return [r.randint(0, k, n).astype(np.float32) for k in (3, 6, 40, 32, 32)] + [r.uniform(-1, 1, n).astype(np.float32)]


def device_sum(v):
    """the sum of v in the kernels' order (csrc/block_sum.h's block_sum_of in fp64): a function of len(v) alone"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    rows = -(-v.size // 256)
    pad = np.zeros(rows * 256)
    pad[:v.size] = v
    acc = np.zeros(256)
    for row in pad.reshape(rows, 256):                # thread t adds t, t + 256, ... in ascending order (x + 0.0 leaves x as it is)
        acc = acc + row
    lanes = np.arange(256)
    for off in (32, 16, 8, 4, 2, 1):                  # xor butterfly inside each wave of 64
        acc = acc + acc[lanes ^ off]
    return ((acc[0] + acc[64]) + acc[128]) + acc[192]


def numpy_sum(v):
    return np.asarray(v, dtype=np.float64).sum()


SUMS = {'numpy': numpy_sum, 'device': device_sum}


def column_stats(col, order='numpy'):
    """step 1 and the amplitude of step 2 -> (sigma, 1e-10 * max(1, mean|v / sigma|))"""
    tot = SUMS[order]
    v = np.asarray(col).astype(np.float64)
    M = np.float64(v.size)
    with np.errstate(all='ignore'):
        mean = tot(v) / M
        d = v - mean
        sigma = np.sqrt(tot(d * d) / M)
        if sigma < TINY:
            sigma = np.float64(1.0)
        mabs = tot(np.abs(v / sigma)) / M
        return sigma, np.float64(1e-10) * (np.float64(1.0) if mabs < 1.0 else mabs)


def prepare(col, noise, order='numpy'):
    """steps 1 and 2: the scaled column with its jitter"""
    sigma, amp = column_stats(col, order)
    with np.errstate(all='ignore'):
        return np.asarray(col).astype(np.float64) / sigma + amp * np.asarray(noise, dtype=np.float64)


def neighbour_counts(x, y, ks, chunk=256):
    """steps 3 and 4 on prepared columns, for every k of `ks` in one sweep -> {k: (nx, ny)} (int64 [M] each)"""
    M = x.size
    out = {k: (np.empty(M, np.int64), np.empty(M, np.int64)) for k in ks}
    for c0 in range(0, M, chunk):
        c1 = min(M, c0 + chunk)
        dx = np.abs(x[c0:c1, None] - x[None, :])
        dy = np.abs(y[c0:c1, None] - y[None, :])
        d = np.maximum(dx, dy)
        d[np.arange(c1 - c0), np.arange(c0, c1)] = np.inf          # j != i
        kth = np.partition(d, [k - 1 for k in ks], axis=1)
        for k in ks:
            r = np.nextafter(kth[:, k - 1], 0.0)[:, None]          # one step toward zero; zero stays zero
            out[k][0][c0:c1] = (dx <= r).sum(1) - 1                # (the point itself is within any radius)
            out[k][1][c0:c1] = (dy <= r).sum(1) - 1
    return out


def psi_table(n=8194):
    """digamma at the integers 0 .. n - 1 as the engine builds it (eval_mi_psi_table): psi(m) = H(m - 1) - gamma, the harmonic numbers by
    compensated summation in ascending order, IEEE operations only (Python floats): the same bits.  Entry 0 is NaN."""
    gamma = 0.5772156649015329
    H, comp, t = 0.0, 0.0, [float('nan'), -gamma]
    for m in range(1, n - 1):
        y = 1.0 / m - comp
        s = H + y
        comp = (s - H) - y
        H = s
        t.append(H - gamma)
    return np.array(t)


PSI = psi_table()


def psi(n):
    """digamma at positive integers <= 8193: the engine's table"""
    return PSI[np.asarray(n, dtype=np.int64)]


def mi_from_counts(nx, ny, M, k, order='numpy'):
    """step 5 in fp64 (before the rounding to fp32).  'numpy': np.mean, scikit-learn's expression.  'device': the kernels' order -- each
    slice of 256 points through device_sum, the slices added in ascending order from 0, ((psi(M) + psi(k)) - sx / M) - sy / M."""
    if order == 'numpy':
        mi = psi(M) + psi(k) - psi(nx + 1).mean() - psi(ny + 1).mean()
    else:
        sx = sy = np.float64(0.0)
        for c0 in range(0, M, 256):
            sx = sx + device_sum(psi(nx[c0:c0 + 256] + 1))
            sy = sy + device_sum(psi(ny[c0:c0 + 256] + 1))
        mi = ((psi(M) + psi(k)) - sx / np.float64(M)) - sy / np.float64(M)
    return max(0.0, float(mi))


def pair(x_col, y_col, noise_x, noise_y, ks=(3,), order='numpy', chunk=256):
    """one (latent, factor) pair -> {k: (MI fp64, nx, ny)}; NaN (and no counts) where a column or the noise is not finite"""
    x, y = prepare(x_col, noise_x, order), prepare(y_col, noise_y, order)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return {k: (np.float64('nan'), None, None) for k in ks}
    cnt = neighbour_counts(x, y, ks, chunk)
    return {k: (mi_from_counts(cnt[k][0], cnt[k][1], x.size, k, order), cnt[k][0], cnt[k][1]) for k in ks}


def table(s0, S_real, noise, ks=(3,), order='device', pairs=None, chunk=256):
    """the pairs `pairs` (default: all 60, latent-major) of s0 [M, 10] x S_real [M, 6] with noise [60, 2, M]
    -> {k: (MI fp64 [60], counts int64 [60, 2, M])}; entries of pairs that were not asked for are NaN / -1"""
    s0, S_real, noise = np.asarray(s0), np.asarray(S_real), np.asarray(noise, dtype=np.float64)
    M = s0.shape[0]
    res = {k: (np.full(PAIRS, np.nan), np.full((PAIRS, 2, M), -1, np.int64)) for k in ks}
    for p in (range(PAIRS) if pairs is None else pairs):
        li, fj = divmod(p, FACTORS)
        got = pair(s0[:, li], S_real[:, fj], noise[p, 0], noise[p, 1], ks, order, chunk)
        for k in ks:
            res[k][0][p] = got[k][0]
            if got[k][1] is not None:
                res[k][1][p, 0], res[k][1][p, 1] = got[k][1], got[k][2]
    return res


def ulp_distance(a, b):
    """the distance of two float32 arrays in units in the last place (both finite, or both NaN -> 0)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.where(both_nan, 0, np.abs(ia - ib))
