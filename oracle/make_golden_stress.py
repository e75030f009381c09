"""ORACLE tooling -- runs ONLY in the build container (needs /root/reference).

Reference-captured fixtures for the stress weight families of oracle/synth.py (`stress_weights`: seed2, gain2, sparse, saturated), in
the dSprites geometry: one small file per family, tests/golden/stress_<family>.npz, with
  * the networks at M = 6 (transition_with_sample, decoder, encoder_with_sample on synthetic frames and on the decoder's own images),
  * calculate_G at M = 6, S = 3,
  * calculate_G_repeated at M = 4, D = 2, S = 2,
captured from the shimmed reference with injected Philox noise exactly as oracle/make_golden.py does (its load_reference / Injector
are imported, not changed, so the existing fixtures regenerate bit-identically).  tests/test_fp64_oracle.py checks that the fp32
oracle reproduces them bit for bit: the restatement is still the reference in the dark and saturated regimes, which is what lets the
fp64 oracle stand in for the reference there.

Usage:  PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_stress
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise
from oracle.make_golden import GOLD, load_reference, maxdiff, npy

NSEED = 7
NET_M, NET_STAGE = 6, 40
G_M, G_S, G_STAGE = 6, 3, 10
R_M, R_D, R_S, R_STAGE = 4, 2, 2, 30


def main():
    torch.set_grad_enabled(False)
    mpath = os.path.join(GOLD, 'MANIFEST.json')
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    manifest.setdefault('cases', {})
    report = {}
    for fam in synth.STRESS_FAMILIES:
        weights = synth.stress_weights(fam)
        model, inj, _, _ = load_reference(weights, NSEED)
        orc = OracleModel(weights, PhiloxNoise(NSEED))
        out = dict(family=np.array(fam), nseed=NSEED)

        # ---- networks ----
        M, st = NET_M, NET_STAGE
        frames = torch.from_numpy(synth.make_frames(12, M))
        s = torch.from_numpy(PX.uniform_fill(3, (M, 10), 150, -1.5, 1.5))
        pi = torch.eye(4)[torch.arange(M) % 4]
        inj.p_trans(PX.PASS_T1, 0, st, 0)
        t_ps1, t_mean, t_lv = model.model_mid.transition_with_sample(pi, s)
        inj.p_dec(PX.PASS_D1, 0, st, 0)
        d_po = model.model_down.decoder(s)
        inj.p_enc(PX.PASS_E1, 0, st, 0)
        e_s, e_mean, e_lv = model.model_down.encoder_with_sample(frames)
        inj.p_enc(PX.PASS_E1, 1, st, 0)
        ed_s, ed_mean, ed_lv = model.model_down.encoder_with_sample(d_po)       # the decoder's own (dark / saturated) images
        assert not inj.q
        out.update(net_frames=frames, net_s=s, net_pi=pi, net_stage=st, t_ps1=t_ps1, t_mean=t_mean, t_lv=t_lv, d_po=d_po,
                   e_s=e_s, e_mean=e_mean, e_lv=e_lv, ed_s=ed_s, ed_mean=ed_mean, ed_lv=ed_lv)
        report[f'{fam}_nets'] = dict(dec=maxdiff(d_po, orc.decoder(s, PX.PASS_D1, 0, st)),
                                     enc=maxdiff(e_mean, orc.encoder(frames, PX.PASS_E1, 0, st)[0]))

        # ---- calculate_G ----
        M, S, st = G_M, G_S, G_STAGE
        s0 = torch.from_numpy(PX.uniform_fill(4, (M, 10), 151, -1.0, 1.0))
        pi0 = torch.eye(4)[torch.arange(M) % 4]
        inj.stage = st
        G, terms, ps1, ps1_mean, po1 = model.calculate_G(s0, pi0, samples=S)
        assert not inj.q
        out.update(g_s0=s0, g_pi0=pi0, g_samples=S, g_stage=st, G=G, t0=terms[0], t1=terms[1], t2=terms[2], ps1=ps1, ps1_mean=ps1_mean,
                   po1=po1)
        report[f'{fam}_G'] = dict(G=maxdiff(G, orc.calculate_G(s0, pi0, S, st)[0]))

        # ---- calculate_G_repeated ----
        M, D, S, st = R_M, R_D, R_S, R_STAGE
        o = torch.from_numpy(np.repeat(synth.make_frames(26, 1), M, axis=0))
        pi = torch.eye(4)
        inj.stage = st
        sum_G, sum_terms, rpo1 = model.calculate_G_repeated(o, pi, steps=D, calc_mean=False, samples=S)
        assert not inj.q
        out.update(r_o=o, r_pi=pi, r_steps=D, r_samples=S, r_stage=st, r_sum_G=sum_G, r_t0=sum_terms[0], r_t1=sum_terms[1],
                   r_t2=sum_terms[2], r_po1=rpo1)
        report[f'{fam}_rollout'] = dict(G=maxdiff(sum_G, orc.calculate_G_repeated(o, pi, D, False, S, st)[0]))

        name = f'stress_{fam}'
        np.savez_compressed(os.path.join(GOLD, name + '.npz'), **{k: npy(v) for k, v in out.items()})
        manifest['cases'][name] = sorted(out.keys())

    with open(mpath, 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1))


if __name__ == '__main__':
    main()
