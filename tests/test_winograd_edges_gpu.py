"""k_dec_a / k_dec_a_s compute ConvT1 by Winograd F(2x2, 3x3) over 2 x 2 output tiles of the zero-padded 18 x 18 image: the tiles at
the image edges read the padding.  The decoder's images are checked against the fp32 CPU oracle at the image border bands (the pixels
that depend on layer-1 edge tiles) and inside, on weights and latents whose layer-1 inputs are active at the borders, for the persistent
launch (one image per workgroup) and the small one (an image over eight workgroups), by the fp64 parity rule of
tests/test_fp64_parity.py: max|engine - fp64| <= ALPHA max|fp32 oracle - fp64| + BETA ulp, on each band separately."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise

ALPHA, BETA = 4.0, 8.0


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['control', 'gain2'])
def test_decoder_images_at_the_padding_edges(family):
    import daimc_amd
    seed, stage = 3, 12
    weights = synth.make_weights(1234, 1.15) if family == 'control' else synth.stress_weights(family)
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=seed, init_weights=False)
    m.load_flat_weights(weights)
    orc = OracleModel(weights, PhiloxNoise(seed))
    o64 = OracleModel(weights, PhiloxNoise(seed), dtype=torch.float64)
    for M in (24, 160):          # <= 128 images: k_dec_a_s; above: k_dec_a
        s = PX.uniform_fill(4, (M, 10), 31 + M, -2, 2).astype(np.float32)
        po = m.model_down.decoder(s, stage=stage, pass_=PX.PASS_D1)
        torch.cuda.synchronize()
        with torch.no_grad():
            ref = orc.decoder(torch.from_numpy(s), PX.PASS_D1, 0, stage)
            ref64 = o64.decoder(torch.from_numpy(s).double(), PX.PASS_D1, 0, stage)
            # the premise: layer 1's input is active at its border rows and columns for these latents
            w = orc.w
            h = orc._in(torch.from_numpy(s))
            for li, idx in enumerate((0, 3, 6, 9)):
                h = F.relu(F.linear(h, w[f'down.po_net.{idx}.weight'], w[f'down.po_net.{idx}.bias']))
                h = h * orc._mask(PX.TAG_DEC + li, M, h.shape[1], PX.PASS_D1, 0, stage, None, fc4_perm=(li == 3))
            x4 = h.reshape(M, 64, 16, 16)
        border = torch.cat([x4[:, :, 0], x4[:, :, -1], x4[:, :, :, 0], x4[:, :, :, -1]], -1)
        assert float((border > 0).float().mean()) > 0.05, (family, M)
        got = po.detach().cpu().double().numpy()[:, 0]
        want = ref.double().numpy()[:, 0]
        exact = ref64.numpy()[:, 0]
        assert got.shape == want.shape == exact.shape == (M, 64, 64)
        band = np.zeros((64, 64), bool)
        band[:8], band[-8:], band[:, :8], band[:, -8:] = True, True, True, True
        for name, sel in (('border', band), ('inside', ~band)):
            e_eng = float(np.abs(got[:, sel] - exact[:, sel]).max())
            e_32 = float(np.abs(want[:, sel] - exact[:, sel]).max())
            ulp = float(np.spacing(np.float32(np.abs(exact[:, sel]).max())))
            assert np.isfinite(got).all() and e_eng <= ALPHA * e_32 + BETA * ulp, (family, M, name, e_eng, e_32, ulp)
