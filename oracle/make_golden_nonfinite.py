"""ORACLE tooling -- runs ONLY in the build container (needs /root/reference).

Where the reference itself puts NaN and inf when one input element or one weight element is not finite: habit, transition, decoder and
encoder at M = 5 (the clean batch of the nets_* fixtures, weights seed 1234 gain 1.15, stage 40), one poisoned element per case --
+NaN, -NaN, +inf, -inf in state row 2 / in pixel (31, 31) of frame 2, and a NaN in down.po_net.9.weight[100, 0] and in
mid.ps_net.0.weight[5, 0] (oracle/nonfinite.py lists the cases).  The fixture holds, per case, the bit-packed isnan and isinf masks of the
network's outputs concatenated row-wise ([5, n], np.packbits of the flattened mask) and n.  The fp32 oracle must reproduce them exactly
(tests/test_oracle_golden.py): that is what makes it a NaN reference for the engine (tests/test_nonfinite_gpu.py).

Shim and noise injection are those of oracle/make_golden.py (imported, not repeated).  Fixtures hold tensors only.
Usage:  PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_nonfinite
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
from oracle import nonfinite as NF
from oracle import philox as PX
from oracle.efe_oracle import OracleModel, PhiloxNoise
from oracle.make_golden import load_reference, GOLD

NAME = 'nonfinite_ref'


def main():
    torch.set_grad_enabled(False)
    man_path = os.path.join(GOLD, 'MANIFEST.json')
    manifest = json.load(open(man_path))
    arrs = dict(wseed=NF.WSEED, gain=NF.GAIN, nseed=NF.NSEED, stage=NF.STAGE, rows=NF.M)
    for case, (net, weights, frames, s, pi) in NF.cases().items():
        model, inj, _, _ = load_reference(weights, NF.NSEED)
        plan = {'habit': lambda: None, 'transition': lambda: inj.p_trans(PX.PASS_T1, 0, NF.STAGE, 0),
                'decoder': lambda: inj.p_dec(PX.PASS_D1, 0, NF.STAGE, 0), 'encoder': lambda: inj.p_enc(PX.PASS_E1, 0, NF.STAGE, 0)}
        plan[net]()
        ref = NF.run_net({'habit': model.model_top.encode_s, 'transition': model.model_mid.transition_with_sample,
                          'decoder': model.model_down.decoder, 'encoder': model.model_down.encoder_with_sample}, net, frames, s, pi)
        assert not inj.q
        orc = NF.run_net(NF.oracle_calls(OracleModel(weights, PhiloxNoise(NF.NSEED))), net, frames, s, pi)
        assert np.array_equal(np.isnan(ref), np.isnan(orc)) and np.array_equal(np.isinf(ref), np.isinf(orc)), case
        assert not np.isfinite(ref).all(), case
        arrs[case + '__nan'] = np.packbits(np.isnan(ref).reshape(-1))
        arrs[case + '__inf'] = np.packbits(np.isinf(ref).reshape(-1))
        arrs[case + '__n'] = ref.shape[1]
        print(case, 'nan', int(np.isnan(ref).sum()), 'inf', int(np.isinf(ref).sum()), 'of', ref.size,
              'rows', np.flatnonzero(~np.isfinite(ref).all(axis=1)).tolist())
    np.savez_compressed(os.path.join(GOLD, NAME + '.npz'), **arrs)
    manifest['cases'][NAME] = sorted(arrs.keys())
    json.dump(manifest, open(man_path, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
