"""CPU tests of the fp64 parity machinery (tests/test_fp64_parity.py): the oracle's float64 mode really computes in float64, every
stress weight family of oracle/synth.py still reaches the regime it targets, the fp32 oracle reproduces the reference-captured stress
fixtures (oracle/make_golden_stress.py) bit for bit, and the comparison rule rejects simulated subtle kernel errors that the fixed
fp32 tolerances of tests/test_gpu_parity.py let through."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import philox as PX
from oracle import synth
from oracle import efe_oracle as EO
from test_fp64_parity import fp64_rule

SEED = 7
GEN = (3, 3, 84)


def _pair(w, geo=(4, 1, 64)):
    kw = dict(pi_dim=geo[0], channels=geo[1], resolution=geo[2])
    return EO.OracleModel(w, EO.PhiloxNoise(SEED), **kw), EO.OracleModel(w, EO.PhiloxNoise(SEED), dtype=torch.float64, **kw)


def _G_inputs(M, A=4):
    s0 = torch.from_numpy(PX.uniform_fill(4, (M, 10), 59, -1.0, 1.0))
    return s0, torch.eye(A)[torch.arange(M) % A]


def test_fp64_mode_computes_in_fp64():
    w = synth.make_weights(1234, 1.15)
    o32, o64 = _pair(w)
    assert all(t.dtype == torch.float64 for t in o64.w.values()) and o64.pi_one_hot.dtype == torch.float64
    s0, pi0 = _G_inputs(6)
    with torch.no_grad():
        G, T, ps1, ps1m, po1 = o64.calculate_G(s0, pi0, 2, 3)
        parts = o64.last_term2_parts
        assert all(t.dtype == torch.float64 for t in [G, ps1, ps1m, po1, *T, *parts])
        # a batch split (rows keyed globally) changes nothing beyond fp64 rounding
        Ga = o64.calculate_G(s0[:2], pi0[:2], 2, 3, 0)[0]
        Gb = o64.calculate_G(s0[2:], pi0[2:], 2, 3, 2)[0]
        np.testing.assert_allclose(torch.cat([Ga, Gb]).numpy(), G.numpy(), rtol=1e-12, atol=0)
        # an input change far below fp32's resolution moves G (an fp32 intermediate anywhere on the path would round it away)
        G2 = o64.calculate_G(s0.double() + 1e-11, pi0, 2, 3)[0]
        d = (G2 - G).abs().numpy()
        assert (d > 0).all() and d.max() < 1e-6
        assert np.array_equal(o32.calculate_G(s0.double() + 1e-11, pi0, 2, 3)[0].numpy(), o32.calculate_G(s0, pi0, 2, 3)[0].numpy())
        # the reward targets follow the images' dtype; the fp32 path is the restatement itself
        assert EO.check_reward(po1).dtype == torch.float64 and EO.check_reward_generic(po1).dtype == torch.float64
        assert EO.check_reward_upstream_intent(po1).dtype == torch.float64
        # and it agrees with the fp32 oracle to fp32 accuracy
        G32 = o32.calculate_G(s0, pi0, 2, 3)[0]
    np.testing.assert_allclose(G32.numpy(), G.numpy(), rtol=1e-5, atol=1e-3)
    assert not np.array_equal(G32.double().numpy(), G.numpy())


# ----------------------------------------------------------------------------------------------------------------------
# every family reaches its regime (fp64 oracle images of calculate_G at M = 8, S = 2)
# ----------------------------------------------------------------------------------------------------------------------
def _images(w, geo=(4, 1, 64)):
    o32, o64 = _pair(w, geo)
    s0, pi0 = _G_inputs(8, geo[0])
    with torch.no_grad():
        r64 = o64.calculate_G(s0, pi0, 2, 3)
        r32 = o32.calculate_G(s0, pi0, 2, 3)
        s = s0.double()
        for d in range(5):                        # five chained transition means (the planner's depth)
            s = o64.transition(pi0, s, PX.PASS_T1, 0, 3 + d)[0]
    return r64[4].numpy(), r32[4].numpy(), float(s.abs().max()), o64


@pytest.mark.parametrize('family,geo', [(f, (4, 1, 64)) for f in synth.STRESS_FAMILIES] + [('sparse', GEN), ('gain2', GEN)])
def test_stress_family_reaches_its_regime(family, geo):
    w = synth.stress_weights(family, *geo)
    assert set(w) == set(synth.make_weights(1234, 1.0, *geo))
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in w.values())
    p64, p32, s5, _ = _images(w, geo)
    assert s5 < 10.0                                          # imagined states stay bounded over depth 5
    dark = float((p64 < 1e-3).mean())
    if family == 'seed2':                                     # another draw of the fixture family: the p ~ 0.5 plateau
        assert 0.2 < np.median(p64) < 0.8 and dark == 0.0
        assert not np.array_equal(w['down.po_net.9.weight'], synth.make_weights(1234, 1.15)['down.po_net.9.weight'])
    elif family == 'gain2':                                   # about half the pixels below 1e-3, saturated logits on both sides
        assert dark > 0.3 and (p32 == 1.0).sum() > 0
    elif family == 'sparse':                                  # trained-like: dark images, nothing saturated
        assert np.median(p64) < 5e-3 and dark > 0.1 and (p64 > 0.5).mean() < 0.01 and (p32 == 1.0).sum() == 0
        assert w['mid.ps_net.0.weight'].max() > np.sqrt(3.0 / 14)              # transition net above gain 1 ...
    elif family == 'saturated':                               # p = 1 in fp32 (x > 17) and x < -89 (hw_sigmoid's exp2 overflows)
        assert (p32 == 1.0).sum() > 0 and float(np.log(p64[p64 > 0]).min()) < -89.0 and (p64 > 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 oracle reproduces the reference-captured stress fixtures bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', synth.STRESS_FAMILIES)
def test_stress_fixture_vs_reference(family):
    g = load_golden(f'stress_{family}')
    assert str(g['family']) == family
    m = EO.OracleModel(synth.stress_weights(family), EO.PhiloxNoise(int(g['nseed'])))
    st = int(g['net_stage'])
    t = lambda k: torch.from_numpy(g[k])
    with torch.no_grad():
        got = dict(zip(('t_ps1', 't_mean', 't_lv'), m.transition_with_sample(t('net_pi'), t('net_s'), PX.PASS_T1, 0, st)))
        got['d_po'] = m.decoder(t('net_s'), PX.PASS_D1, 0, st)
        got.update(zip(('e_s', 'e_mean', 'e_lv'), m.encoder_with_sample(t('net_frames'), PX.PASS_E1, 0, st)))
        got.update(zip(('ed_s', 'ed_mean', 'ed_lv'), m.encoder_with_sample(t('d_po'), PX.PASS_E1, 1, st)))
        G, T, ps1, ps1m, po1 = m.calculate_G(t('g_s0'), t('g_pi0'), int(g['g_samples']), int(g['g_stage']))
        got.update(G=G, t0=T[0], t1=T[1], t2=T[2], ps1=ps1, ps1_mean=ps1m, po1=po1)
        sG, sT, rpo1 = m.calculate_G_repeated(t('r_o'), t('r_pi'), int(g['r_steps']), False, int(g['r_samples']), int(g['r_stage']))
        got.update(r_sum_G=sG, r_t0=sT[0], r_t1=sT[1], r_t2=sT[2], r_po1=rpo1)
    for k, v in got.items():
        assert np.isfinite(g[k]).all(), k
        assert np.array_equal(v.numpy(), g[k]), (k, float(np.abs(v.numpy() - g[k]).max()))


# ----------------------------------------------------------------------------------------------------------------------
# the rule rejects subtle kernel errors (simulated by hooking the fp32 oracle) that it must catch
# ----------------------------------------------------------------------------------------------------------------------
class _Bf16Images(EO.OracleModel):
    """simulated kernel error 2: pixel p rounded to bf16 before the entropy and reward sums"""

    def decoder(self, *a, **k):
        return super().decoder(*a, **k).to(torch.bfloat16).to(self.dtype)


def _calcG_rows(o, s0, pi0):
    G, T, ps1, _, po1 = o.calculate_G(s0, pi0, 2, 3)
    p = o.last_term2_parts
    return [('G', G), ('t0', T[0]), ('t1', T[1]), ('t2', T[2]), ('t2_1', p[0]), ('t2_2', p[1]), ('ps1', ps1), ('po1', po1)]


def _verdict(eng, r32, r64):
    rows = []
    for (n, e), (_, a), (_, b) in zip(eng, r32, r64):
        rows += fp64_rule(n, e, a, b, image=(n == 'po1'))
    return all(r[-1] for r in rows), rows


@pytest.mark.parametrize('family', ['control'] + list(synth.STRESS_FAMILIES))
def test_rule_rejects_simulated_kernel_errors(family, monkeypatch):
    w = synth.make_weights(1234, 1.15) if family == 'control' else synth.stress_weights(family)
    o32, o64 = _pair(w)
    s0, pi0 = _G_inputs(4)
    with torch.no_grad():
        r32, r64 = _calcG_rows(o32, s0, pi0), _calcG_rows(o64, s0, pi0)
        ok, rows = _verdict(r32, r32, r64)
        assert ok, rows                                               # the fp32 oracle itself passes (ratio <= 1)
        bf = _calcG_rows(_Bf16Images(w, EO.PhiloxNoise(SEED)), s0, pi0)
        ok, rows = _verdict(bf, r32, r64)
        assert not ok, rows
        orig = EO.entropy_bernoulli
        monkeypatch.setattr(EO, 'entropy_bernoulli', lambda p, displacement=0.00001: orig(p, 0.0))     # simulated error 1
        nod = _calcG_rows(o32, s0, pi0)
        ok, rows = _verdict(nod, r32, r64)
        assert not ok, rows
