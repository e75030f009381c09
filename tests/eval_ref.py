"""numpy fp64 restatements of what the epoch report reduces on the device (csrc/eval.hip, efe_eval_stats): means, the unbiased standard
deviation, torch.median's lower median, total_correlation as the reference's src/torchutils.py:40-42 computes it, Spearman's rho with ties
at their average rank, and compare_reward (src/util.py:82-85).  A plain module, like free_energy_ref.py; `row` assembles the whole [98]
row in the layout of include/efe_engine.h."""
import warnings

import numpy as np

FE_ARRAYS = ('F_top', 'F_mid', 'F_down', 'nlogpo1', 'kl_s', 'kl_naive', 'kl_pi', 'kl_s_anal', 'kl_naive_anal', 'kl_pi_anal')
STATS = 98


def mean(x, axis=None):
    return np.asarray(x, dtype=np.float64).mean(axis=axis)


def std(x):
    """unbiased (ddof 1); NaN for one element, as torch.std"""
    x = np.asarray(x, dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return x.std(ddof=1) if x.size > 1 else np.float64('nan')


def lower_median(x):
    """torch.median: the element of sorted rank (n - 1) // 2, NaN if any element is NaN -> an element of x (its dtype)"""
    x = np.asarray(x).reshape(-1)
    if np.isnan(x).any():
        return x.dtype.type('nan')
    return np.sort(x)[(x.size - 1) // 2]


def total_correlation(data):
    """torchutils.py:40-42: (sum_k log cov_kk - log det cov) / 2 of the covariance (divisor n - 1) of the rows of data"""
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        cov = np.atleast_2d(np.cov(np.asarray(data, dtype=np.float64), rowvar=False))
        return 0.5 * (np.log(np.diag(cov)).sum() - np.linalg.slogdet(cov)[1])


def covariance_condition(data):
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        cov = np.atleast_2d(np.cov(np.asarray(data, dtype=np.float64), rowvar=False))
        return np.linalg.cond(cov) if np.isfinite(cov).all() else np.inf


def doubled_ranks(x):
    """2 * (average rank) of every element, an exact integer: 2 #less + #equal + 1"""
    x = np.asarray(x).reshape(-1)
    s = np.sort(x)
    return (np.searchsorted(s, x, 'left') + np.searchsorted(s, x, 'right') + 1).astype(np.int64)


def spearman(x, y):
    """Spearman's rho, ties at their average rank (scipy.stats.spearmanr's convention): Pearson's r of the ranks, from exact integer
    moments of the doubled ranks and one fp64 quotient.  NaN for a constant column (0 / 0) or a NaN in either column."""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    if np.isnan(x).any() or np.isnan(y).any():
        return np.float64('nan')
    n = x.size
    RX, RY = [int(v) for v in doubled_ranks(x)], [int(v) for v in doubled_ranks(y)]      # Python integers: no overflow at any n
    sx, sy = sum(RX), sum(RY)
    sxx, syy, sxy = sum(v * v for v in RX), sum(v * v for v in RY), sum(u * v for u, v in zip(RX, RY))
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    with np.errstate(all='ignore'):
        return np.float64(num) / np.sqrt(np.float64(dx) * np.float64(dy))


def spearman_table(s0, S_real):
    s0, S_real = np.asarray(s0), np.asarray(S_real)
    return np.array([[spearman(s0[:, i], S_real[:, j]) for j in range(S_real.shape[1])] for i in range(s0.shape[1])])


def compare_reward(o1, po1):
    """util.py:82-85 on NCHW [M, C, 64, 64]: the reference slices NHWC [:, 0:3, 0:64, :]"""
    o1, po1 = np.asarray(o1, dtype=np.float64), np.asarray(po1, dtype=np.float64)
    return np.square(o1[:, :, 0:3, 0:64] - po1[:, :, 0:3, 0:64]).mean()


def row(fe=None, qs1=None, s0=None, S_real=None, o1_r=None, po1_r=None):
    """the [98] row in fp64 (NaN where a group is absent); min / max / med are exact input elements"""
    out = np.full(STATS, np.nan)
    if fe is not None:
        f = {k: np.asarray(fe[k]) for k in FE_ARRAYS}
        per_row = ((f['F_down'] + f['F_mid']).astype(np.float32) + f['F_top']).astype(np.float32)       # the fp32 per-row sum, train.py:149
        out[0] = mean(per_row)
        for i, k in enumerate(FE_ARRAYS[:7]):
            out[1 + i] = mean(f[k])
        kl = f['kl_pi']
        bad = np.isnan(kl).any()
        out[8], out[9] = (np.nan, np.nan) if bad else (kl.min(), kl.max())
        out[10], out[11] = lower_median(kl), std(kl)
        out[14:24], out[24:34], out[34:38] = mean(f['kl_s_anal'], 0), mean(f['kl_naive_anal'], 0), mean(f['kl_pi_anal'], 0)
    if qs1 is not None:
        out[12] = total_correlation(qs1)
    if o1_r is not None:
        out[13] = compare_reward(o1_r, po1_r)
    if s0 is not None:
        out[38:98] = spearman_table(s0, S_real).reshape(-1)
    return out
