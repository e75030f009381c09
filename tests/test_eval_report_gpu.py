"""GPU tests (-m gpu) of the epoch report: efe_eval_stats (csrc/eval.hip) through loss.eval_stats against the fp64 restatements of
tests/eval_ref.py, the two evaluation batch producers of daimc_amd.util against oracle/env_oracle.py, and Trainer.report against
Trainer.evaluate on a twin.

Bounds (u = 2^-24).  A mean of N elements: (ceil(N / 256) + 13) u mean|x| against the fp64 mean -- a term passes through at most
ceil(N / 256) strided adds, 6 butterfly steps and 3 wave adds, the division adds one rounding and the slack of 2 u of the training
step's bound stays (ceil(N / 256) + 12), plus one rounding where the element itself is computed (the per-row sum of
F, the square of mse_r).  The standard deviation: the same relative bound k u on the sum of squared deviations (all positive), carried
through the square root, whose derivative halves it: (k u / 2 + u) std; the arrays here have a spread comparable to their mean, so the
error of the mean enters in second order only.  min / max / med are input elements: bit-equal.  TC: fp64 arithmetic and one fp32
rounding, 1.2e-7 |TC| + 1e-9, where the reference covariance has a condition number below 1e6.  rho: one fp32 rounding of a number in
[-1, 1], 1e-7.  Every figure is printed before it is asserted; the largest fraction of each bound is printed per size."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import eval_ref
from train_common import c, model_for

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MS = (1, 2, 12, 63, 64, 65, 255, 256, 257, 1000, 8192)
DEV = 'cuda:0'


def L():
    import daimc_amd
    return daimc_amd.loss


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


_DATA = {}


def data(M):
    """one synthetic evaluation batch per size (host arrays, never changed): loss-like positive rows with a spread comparable to their
    mean, correlated latents, latents that follow some true factors, and a reward batch of M images whose rows 0..2 differ"""
    if M not in _DATA:
        r = np.random.RandomState(1000 + M)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        fe = {'F_top': f32(r.gamma(2.0, 0.3, M)), 'F_mid': f32(r.gamma(3.0, 2.0, M)), 'F_down': f32(120.0 + 30.0 * r.randn(M)),
              'nlogpo1': f32(r.gamma(4.0, 20.0, M)), 'kl_s': f32(r.gamma(2.0, 3.0, M)), 'kl_naive': f32(r.gamma(2.0, 5.0, M)),
              'kl_pi': f32(r.gamma(2.0, 0.3, M)), 'kl_s_anal': f32(r.gamma(2.0, 0.3, (M, 10))), 'kl_naive_anal': f32(r.randn(M, 10)),
              'kl_pi_anal': f32(r.randn(M, 4) * 0.2)}
        qs1 = f32(r.randn(M, 10) @ (np.eye(10) + 0.3 * r.randn(10, 10)))
        S = np.stack([r.randint(0, k, M) for k in (3, 6, 40, 32, 32)] + [r.uniform(-1, 1, M)], 1)
        s0 = r.randn(M, 10)
        s0[:, 3] += 0.2 * S[:, 3]
        s0[:, 4] -= 0.1 * S[:, 4]
        s0[:, 7] = S[:, 2] + 0.01 * r.randn(M)
        bar_o, bar_p = f32(r.rand(M, 1, 3, 64) < 0.5), f32(r.rand(M, 1, 3, 64))
        _DATA[M] = dict(fe=fe, qs1=qs1, s0=f32(s0), S_real=f32(S), bar_o=bar_o, bar_p=bar_p)
    return _DATA[M]


def images(bar, fill):
    """[M, 1, 64, 64] on the device: rows 0..2 from `bar`, every other pixel `fill` (the report must not read them)"""
    t = torch.full((bar.shape[0], 1, 64, 64), fill, dtype=torch.float32, device=DEV)
    t[:, :, 0:3, :] = torch.as_tensor(bar).to(DEV)
    return t


def dev(d, **poison):
    """the device inputs of loss.eval_stats for data `d`: (fe mapping with qs1 and s0, S_real, (o1_r, po1_r)); poison = {array: (index, value)}"""
    host = dict(d['fe'], qs1=d['qs1'], s0=d['s0'], S_real=d['S_real'], bar_o=d['bar_o'], bar_p=d['bar_p'])
    for k, (idx, v) in poison.items():
        host[k] = host[k].copy()
        host[k][idx] = v
    fe = {k: torch.as_tensor(host[k]).to(DEV) for k in eval_ref.FE_ARRAYS + ('qs1', 's0')}
    return host, fe, torch.as_tensor(host['S_real']).to(DEV), (images(host['bar_o'], 3.0), images(host['bar_p'], -5.0))


def ref_row(host):
    o1 = np.zeros((len(host['bar_o']), 1, 64, 64), np.float32)
    po1 = np.zeros_like(o1)
    o1[:, :, 0:3, :], po1[:, :, 0:3, :] = host['bar_o'], host['bar_p']
    return eval_ref.row({k: host[k] for k in eval_ref.FE_ARRAYS}, host['qs1'], host['s0'], host['S_real'], o1, po1)


_RUNS = {}


def run(M):
    """(host arrays, device row as fp32 numpy, fp64 reference row) of the clean batch of M rows, computed once"""
    if M not in _RUNS:
        host, fe, S, rw = dev(data(M))
        _RUNS[M] = (host, c(L().eval_stats(fe, S, rw)), ref_row(host))
    return _RUNS[M]


def mean_bounds(host, M):
    """{row index: bound} of every mean of the row and of mse_r"""
    f = host
    k = (math.ceil(M / 256) + 13) * U
    per_row = ((f['F_down'] + f['F_mid']).astype(np.float32) + f['F_top']).astype(np.float32)
    b = {0: k * np.abs(per_row.astype(np.float64)).mean()}
    for i, name in enumerate(eval_ref.FE_ARRAYS[:7]):
        b[1 + i] = k * np.abs(f[name].astype(np.float64)).mean()
    for base, name in ((14, 'kl_s_anal'), (24, 'kl_naive_anal'), (34, 'kl_pi_anal')):
        for j in range(f[name].shape[1]):
            b[base + j] = k * np.abs(f[name][:, j].astype(np.float64)).mean()
    sq = np.square(f['bar_o'].astype(np.float64) - f['bar_p'].astype(np.float64))
    b[13] = (math.ceil(sq.size / 256) + 13) * U * sq.mean()
    return b


def check_row(tag, host, got, ref, M):
    """the assertions of item 1 on one row; -> the largest observed fraction of each bound"""
    bad, frac = [], {'mean': 0.0, 'mse_r': 0.0, 'std': 0.0, 'TC': 0.0, 'rho': 0.0}
    g = got.astype(np.float64)
    for i, bound in sorted(mean_bounds(host, M).items()):
        if np.isnan(ref[i]):
            assert np.isnan(g[i]), (tag, i)
            continue
        err = abs(g[i] - ref[i])
        key = 'mse_r' if i == 13 else 'mean'
        frac[key] = max(frac[key], err / bound)
        print(f'{tag} [{i}] engine {g[i]:.9g} fp64 {ref[i]:.9g} err {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append((i, err, bound))
    kl = host['kl_pi']
    for i in (8, 9, 10):                                # min, max, med: input elements
        if np.isnan(ref[i]):
            assert np.isnan(got[i]), (tag, i)
        else:
            assert bits(got[i]) == bits(ref[i]), (tag, i, got[i], ref[i])
    assert bits(got[10]) == bits(torch.as_tensor(kl).median().item()) or np.isnan(got[10])
    if np.isnan(ref[11]):
        assert np.isnan(got[11]), tag
    else:
        k = (math.ceil(M / 256) + 13) * U
        err, bound = abs(g[11] - ref[11]), (k / 2 + U) * ref[11]
        frac['std'] = err / bound if bound else 0.0
        print(f'{tag} std engine {g[11]:.9g} numpy {ref[11]:.9g} err {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append(('std', err, bound))
    cond = eval_ref.covariance_condition(host['qs1'])
    if np.isnan(ref[12]):
        assert np.isnan(got[12]), tag
    elif cond < 1e6:
        err, bound = abs(g[12] - ref[12]), 1.2e-7 * abs(ref[12]) + 1e-9
        frac['TC'] = err / bound
        print(f'{tag} TC engine {g[12]:.9g} numpy {ref[12]:.9g} err {err:.3e} bound {bound:.3e} (condition {cond:.3g})')
        if not err <= bound:
            bad.append(('TC', err, bound))
    else:
        print(f'{tag} TC engine {g[12]} numpy {ref[12]} (condition {cond:.3g}: not asserted)')
    rho, rr = g[38:], ref[38:]
    assert (np.isnan(rho) == np.isnan(rr)).all(), (tag, np.isnan(rho).reshape(10, 6), np.isnan(rr).reshape(10, 6))
    if (~np.isnan(rr)).any():
        err = np.nanmax(np.abs(rho - rr))
        frac['rho'] = err / 1e-7
        print(f'{tag} rho largest err {err:.3e} bound 1e-7; largest |rho| {np.nanmax(np.abs(rr)):.3f}')
        if not err <= 1e-7:
            bad.append(('rho', err, 1e-7))
    print(f'{tag} largest fraction of each bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in frac.items()))
    assert not bad, (tag, bad)
    return frac


# ---- 1. synthetic arrays against eval_ref ---------------------------------------------------------------------------------
@pytest.mark.parametrize('M', MS)
def test_synthetic_against_fp64(M):
    host, got, ref = run(M)
    check_row(f'M={M}', host, got, ref, M)
    if M == 1:                                          # what numpy makes NaN at one row: the std, TC, every rho
        assert np.isnan(got[11]) and np.isnan(got[12]) and np.isnan(got[38:]).all()
        assert not np.isnan(got[:11]).any() and not np.isnan(got[13:38]).any()
    if M > 10:
        assert np.isfinite(got).all()


# ---- 2. ties and order statistics -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', (6, 64, 257, 8192))
def test_ties_and_order_statistics(M):
    r = np.random.RandomState(M)
    d = data(M)
    host = dict(d['fe'], qs1=d['qs1'])
    kl = r.randint(0, 4, M).astype(np.float32)           # even M, many duplicates: the lower median is an element, not a midpoint
    if M == 6:
        kl = np.array([3, 1, 2, 2, 5, 1], np.float32)
    up = np.cumsum(r.rand(M) + 0.01)
    s0 = r.randn(M, 10)
    s0[:, 0], s0[:, 1], s0[:, 2] = up, 2.5, r.randint(0, 3, M)
    S = r.randn(M, 6)
    S[:, 0], S[:, 1], S[:, 2] = np.exp(up / up.max()), -up, s0[:, 2] * 2.0      # increasing, decreasing, the same ties
    fe = {k: torch.as_tensor(v).to(DEV) for k, v in host.items()}
    fe['kl_pi'] = torch.as_tensor(kl).to(DEV)
    fe['kl_s'] = torch.full((M,), 2.5, device=DEV)        # all equal; every multiple of 2.5 up to 8192 x 2.5 is exact in fp32, so the mean is 2.5
    fe['s0'] = torch.as_tensor(s0.astype(np.float32)).to(DEV)
    got = c(L().eval_stats(fe, torch.as_tensor(S.astype(np.float32)).to(DEV)))
    rho = got[38:].reshape(10, 6)
    assert got[10] == np.sort(kl)[(M - 1) // 2] == torch.as_tensor(kl).median().item() and got[8] == kl.min() and got[9] == kl.max()
    fe2 = dict(fe, kl_pi=fe['kl_s'])
    got2 = c(L().eval_stats(fe2))
    assert bits(got2[11]) == bits(0.0) and bits(got2[7]) == bits(got2[8]) == bits(got2[9]) == bits(got2[10]) == bits(2.5)      # std exactly 0
    assert bits(rho[0, 0]) == bits(1.0) and bits(rho[0, 1]) == bits(-1.0), rho[0]
    ref = eval_ref.spearman_table(s0.astype(np.float32), S.astype(np.float32))
    assert np.isnan(rho[1]).all() and (np.isnan(rho) == np.isnan(ref)).all()                    # a constant column: 0 / 0
    assert bits(rho[2, 2]) == bits(1.0) or np.isnan(ref[2, 2])                                  # the same tie pattern on both sides
    assert np.nanmax(np.abs(rho - ref)) <= 1e-7


# ---- 3. non-finite values -----------------------------------------------------------------------------------------------------
READS = {'kl_pi': range(7, 12), 'qs1': (12,), 'po1_r': (13,), 's0': range(38 + 4 * 6, 38 + 5 * 6)}


@pytest.mark.parametrize('case', ['kl_pi nan', 'kl_pi inf', 'qs1 nan', 's0 nan', 'po1_r nan'])
def test_nonfinite(case):
    M = 65
    name, what = case.split()
    v = np.float32('nan') if what == 'nan' else np.float32('inf')
    key, idx = {'kl_pi': ('kl_pi', 40), 'qs1': ('qs1', (40, 3)), 's0': ('s0', (64, 4)), 'po1_r': ('bar_p', (7, 0, 2, 63))}[name]
    _, clean, _ = run(M)
    host, fe, S, rw = dev(data(M), **{key: (idx, v)})
    got, ref = c(L().eval_stats(fe, S, rw)), ref_row(host)
    reads = set(READS[name])
    print(case, {i: (got[i], ref[i]) for i in sorted(reads)})
    assert (np.isnan(got) == np.isnan(ref)).all(), (case, np.flatnonzero(np.isnan(got) != np.isnan(ref)))
    assert np.isnan(got[sorted(reads)]).any()
    if what == 'inf':                                   # mean inf, min / med finite input elements, max inf, std NaN
        assert got[7] == np.inf and got[9] == np.inf and np.isnan(got[11]) and bits(got[8]) == bits(ref[8]) and bits(got[10]) == bits(ref[10])
    else:
        assert np.isnan(got[sorted(reads)]).all()
    others = [i for i in range(98) if i not in reads]
    assert bits(got[others]).tobytes() == bits(clean[others]).tobytes(), case


# ---- 4. groups and memory -----------------------------------------------------------------------------------------------------
GROUPS = {'FE': list(range(0, 12)) + list(range(14, 38)), 'TC': [12], 'R': [13], 'RHO': list(range(38, 98))}


def test_groups_and_memory():
    M = 257
    _, full, _ = run(M)
    _, fe, S, rw = dev(data(M))
    calls = {'FE': lambda **kw: L().eval_stats({k: fe[k] for k in eval_ref.FE_ARRAYS}, **kw),
             'TC': lambda **kw: L().eval_stats({'qs1': fe['qs1']}, **kw),
             'RHO': lambda **kw: L().eval_stats({'s0': fe['s0']}, S, **kw),
             'R': lambda **kw: L().eval_stats(reward=rw, **kw)}
    for g, call in calls.items():
        got = c(call())
        mine = GROUPS[g]
        rest = [i for i in range(98) if i not in mine]
        assert bits(got[mine]).tobytes() == bits(full[mine]).tobytes(), g
        assert np.isnan(got[rest]).all(), (g, [i for i in rest if not np.isnan(got[i])])
    assert bits(c(L().compare_reward(*rw))) == bits(full[13]) and L().compare_reward(*rw).dim() == 0
    buf = torch.full((98 + 64,), 777.0, device=DEV)
    out = L().eval_stats(fe, S, rw, out=buf[32:130])
    assert out.data_ptr() == buf[32:130].data_ptr()
    h = c(buf)
    assert (h[:32] == 777.0).all() and (h[130:] == 777.0).all() and bits(h[32:130]).tobytes() == bits(full).tobytes()      # guards; twice the same bytes


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def raw(e, ptrs, M, out, Mr=0):
    """efe_eval_stats through ctypes -> (return code, message)"""
    from daimc_amd import _lib as LB
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ei = LB.EfeEvalIn(*[p(ptrs.get(f)) for f in LB.EVAL_IN_FIELDS], Mr)
    rc = e.lib.efe_eval_stats(e.ctx, C.byref(ei) if ptrs is not None else None, M, p(out), e.stream())
    torch.cuda.synchronize()
    return rc, e.lib.efe_last_error(e.ctx).decode()


def test_refusals_write_nothing():
    M = 12
    _, fe, S, rw = dev(data(M))
    out = torch.full((98,), 777.0, device=DEV)
    empty = {k: v[:0] for k, v in fe.items()}
    big = {k: torch.zeros((8193,) + tuple(v.shape[1:]), device=DEV) for k, v in fe.items()}
    cases = {'M = 0': lambda: L().eval_stats(empty, out=out),
             'M = 8193': lambda: L().eval_stats(big, out=out),
             'no group': lambda: L().eval_stats(out=out),
             'FE group with one array missing': lambda: L().eval_stats({k: v for k, v in fe.items() if k != 'kl_s'}, out=out)}
    for tag, call in cases.items():
        with pytest.raises(RuntimeError, match='efe_eval_stats') as ei:
            call()
        print(tag, '->', str(ei.value).splitlines()[0])
        assert (c(out) == 777.0).all(), tag
    e = L()._stats_engine(DEV)
    full = dict(fe, S_real=S, o1_r=rw[0], po1_r=rw[1])
    for tag, (ptrs, m, o, mr, word) in {
            'M = 0': (full, 0, out, M, 'M must be >= 1'), 'M = 8193': (full, 8193, out, M, 'above the cap'), 'Mr = 8193': (full, M, out, 8193, 'Mr'),
            'no group': ({}, M, out, 0, 'no input group'), 'partial FE': ({k: v for k, v in full.items() if k != 'F_mid'}, M, out, M, 'partial FE'),
            'partial RHO': ({'s0': fe['s0']}, M, out, 0, 'partial RHO'), 'partial R': ({'o1_r': rw[0]}, M, out, M, 'partial R'),
            'NULL out': (full, M, None, M, 'out')}.items():
        rc, msg = raw(e, ptrs, m, o, mr)
        print(tag, '->', rc, msg)
        assert rc == 1 and 'efe_eval_stats' in msg and word in msg, (tag, msg)
        assert (c(out) == 777.0).all(), tag
    rc, msg = raw(e, full, M, out, M)                   # and the same arguments, whole, are accepted
    assert rc == 0 and not (c(out) == 777.0).any()


# ---- 6. batch producers -------------------------------------------------------------------------------------------------------------
ENV_SEED = 5


def s_real(s, last_r):
    S = s[:, 1:7].copy()
    S[:, 5] = last_r
    return S


@pytest.mark.parametrize('games', (1, 127, 129))
def test_reward_transition_batch(games):
    import daimc_amd
    from oracle import env_oracle as EO
    m = model_for('g115')
    imgs = EO.sprite_bank()
    for repeats in (1, 5):
        for deepness in (1, 2):
            g = daimc_amd.Game(games, model=m, seed=ENV_SEED)
            st = g._stage
            o0, o1, pi = daimc_amd.make_batch_dsprites_random_reward_transitions(g, deepness=deepness, repeats=repeats)
            s, last_r = EO.reset(ENV_SEED, games, st)
            s[:, 5] = 31.0
            f0 = EO.render(s, last_r, imgs)
            for t in range(deepness):
                changed = EO.step(ENV_SEED, s, last_r, np.zeros(games, np.int64), repeats, st + 1 + t)
                assert t > 0 or changed.all()           # right below the edge: the first `up` ends every game's round
            f1 = EO.render(s, last_r, imgs)
            assert tuple(o0.shape) == tuple(o1.shape) == (games, 1, 64, 64) and o0.device.type == 'cuda'
            assert c(o0).reshape(games, 64, 64, 1).tobytes() == f0.tobytes() and c(o1).reshape(games, 64, 64, 1).tobytes() == f1.tobytes()
            assert np.array_equal(c(pi), np.tile(np.array([1, 0, 0, 0], np.float32), (games, 1)))
            assert np.array_equal(c(g.current_s), s) and np.array_equal(c(g.last_r), last_r) and g._stage == st + 1 + deepness
    twin = daimc_amd.Game(games, model=m, seed=ENV_SEED)
    twin.randomize_environment_all()
    twin.current_s[:, 5] = 31.0
    assert bool(twin.pi_to_action_all(torch.zeros(games, dtype=torch.int32), repeats=5).all())


@pytest.mark.parametrize('games', (1, 127, 129))
def test_random_batch_with_latents(games):
    import daimc_amd
    from daimc_amd.train import make_batch_random
    from oracle import env_oracle as EO
    m = model_for('g115')
    ga, gb = (daimc_amd.Game(games, model=m, seed=ENV_SEED) for _ in range(2))
    gen_a, gen_b = (torch.Generator(device=DEV).manual_seed(21) for _ in range(2))
    st = ga._stage
    o0, o1, pi0, S0, S1 = daimc_amd.make_batch_dsprites_random(ga, 5, gen_a)
    p0, p1, ppi = make_batch_random(gb, 5, gen_b)
    assert c(o0).tobytes() == c(p0).tobytes() and c(o1).tobytes() == c(p1).tobytes() and c(pi0).tobytes() == c(ppi).tobytes()
    assert np.array_equal(c(ga.current_s), c(gb.current_s)) and ga._stage == gb._stage
    assert torch.equal(torch.rand(3, device=DEV, generator=gen_a), torch.rand(3, device=DEV, generator=gen_b))      # the same draws were taken
    s, last_r = EO.reset(ENV_SEED, games, st)
    assert tuple(S0.shape) == tuple(S1.shape) == (games, 6)
    assert np.array_equal(c(S0), s_real(s, last_r))                                     # the state before the action
    EO.step(ENV_SEED, s, last_r, c(pi0).argmax(1), 5, st + 1)
    assert np.array_equal(c(S1), s_real(s, last_r)) and np.array_equal(c(S1)[:, :5], c(ga.current_s)[:, 1:6])      # and after it


# ---- 7. Trainer.report -----------------------------------------------------------------------------------------------------------------
GAMES = 8


def trainer():
    import daimc_amd
    m = model_for('g115', fresh=True)
    games = daimc_amd.Game(GAMES, model=m, seed=3)
    test = daimc_amd.Game(GAMES, model=m, seed=4)
    gen = torch.Generator(device=DEV).manual_seed(11)
    return m, test, gen, daimc_amd.Trainer(m, games, generator=gen)


def test_trainer_report():
    import daimc_amd
    from daimc_amd.train import REPORT_KEYS, make_batch_random
    ma, test_a, _, ta = trainer()
    mb, test_b, gen_b, tb = trainer()
    ta.epoch(1)
    tb.epoch(1)
    rep = ta.report(test_a)
    o0, o1, pi0 = make_batch_random(test_b, tb.repeats, gen_b)
    stage = mb._stage
    st = tb.evaluate(o0, o1, pi0)
    fe = daimc_amd.free_energy(mb, o0, o1, pi0, torch.log(pi0 + 1e-15), omega=1.0 / 2.0 + 1.5, stage=stage)
    r0, r1, rpi = daimc_amd.make_batch_dsprites_random_reward_transitions(test_b, deepness=1, repeats=tb.repeats)
    po1 = mb.imagine_future_from_o(r0, rpi)
    assert tuple(rep) == REPORT_KEYS
    for k in ('kl_div_pi_min', 'kl_div_pi_max', 'kl_div_pi_med', 'var_beta_s', 'var_gamma', 'var_beta_o', 'var_a', 'var_b', 'var_c', 'var_d',
              'omega', 'omega_std'):
        assert rep[k] == st[k] and isinstance(rep[k], float), (k, rep[k], st[k])
    assert np.isfinite(rep['omega']) and ma._stage == mb._stage and test_a._stage == test_b._stage
    host = {k: c(getattr(fe, k)) for k in eval_ref.FE_ARRAYS}
    host['bar_o'], host['bar_p'] = c(r1)[:, :, 0:3, :], c(po1)[:, :, 0:3, :]
    ref = eval_ref.row({k: host[k] for k in eval_ref.FE_ARRAYS}, o1_r=c(r1), po1_r=c(po1))
    row = np.full(98, np.nan)
    for k, sl in L().EVAL_STATS_FIELDS.items():
        row[sl] = np.asarray(rep[k], dtype=np.float64).reshape(-1)
    bad = []
    for i, bound in sorted(mean_bounds(host, GAMES).items()):
        err = abs(row[i] - ref[i])
        print(f'report [{i}] {row[i]:.9g} fp64 {ref[i]:.9g} err {err:.3e} bound {bound:.3e}')
        if not err <= bound:
            bad.append((i, err, bound))
    assert not bad, bad
    k = (math.ceil(GAMES / 256) + 13) * U
    assert abs(rep['kl_div_pi_std'] - ref[11]) <= (k / 2 + U) * ref[11]
    assert rep['spearman'].shape == (10, 6) and rep['kl_div_s_anal'].shape == (10,) and rep['kl_div_pi_anal'].shape == (4,)
    ref_rho = eval_ref.spearman_table(c(fe.s0), c(daimc_amd.make_batch_dsprites_random(daimc_amd.Game(GAMES, model=mb, seed=4), 5,
                                                                                      torch.Generator(device=DEV).manual_seed(99))[3]))
    assert (np.isnan(rep['spearman']) == np.isnan(ref_rho)).all() and np.nanmax(np.abs(rep['spearman'] - ref_rho)) <= 1e-7
    assert np.isnan(rep['TC'])                         # 8 rows: a covariance of rank < 10 (the documented deviation from numpy's inf)
    assert isinstance(rep['mse_r'], float) and rep['mse_r'] > 0.0
