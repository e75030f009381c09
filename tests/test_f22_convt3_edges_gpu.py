"""k_dec_b4 computes ConvT3 by F(2, 2) over 2 x 2 input blocks: the last block column and row read the zero pixel x[32], a wave owns one
block row of a 4-row strip, and k_dec_b4<4> splits an image into quarters of two strips (plus a halo strip).  The decoder's images are
checked against the fp32 CPU oracle on each of these bands separately -- the last output rows / columns, the rows around strip and quarter
boundaries, and the rest -- by the fp64 parity rule of tests/test_fp64_parity.py (max|engine - fp64| <= ALPHA max|fp32 oracle - fp64|
+ BETA ulp), for the small launch (k_dec_b4<4>) and the persistent one (k_dec_b4<1>); the images both launches share must agree bit for bit."""
import numpy as np
import pytest
import torch

from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise

ALPHA, BETA = 4.0, 8.0


def bands():
    last = np.zeros((64, 64), bool)
    last[-4:], last[:, -4:] = True, True
    rows = np.arange(64)
    strip = np.zeros((64, 64), bool)
    strip[(rows % 8 == 7) | (rows % 8 == 0)] = True                # y3 rows 8k - 1, 8k: the ConvT4 taps straddle two strips
    strip &= ~last
    return (('last', last), ('strip', strip), ('inside', ~(last | strip)))


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['control', 'gain2'])
def test_decoder_images_at_the_block_and_strip_edges(family):
    import daimc_amd
    seed, stage = 5, 17
    weights = synth.make_weights(1234, 1.15) if family == 'control' else synth.stress_weights(family)
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=seed, init_weights=False)
    m.load_flat_weights(weights)
    orc = OracleModel(weights, PhiloxNoise(seed))
    o64 = OracleModel(weights, PhiloxNoise(seed), dtype=torch.float64)
    s = PX.uniform_fill(4, (160, 10), 77, -2.5, 2.5).astype(np.float32)
    got = {}
    for M in (24, 160):          # <= 128 images: k_dec_b4<4>; above: k_dec_b4<1>
        po = m.model_down.decoder(s[:M], stage=stage, pass_=PX.PASS_D1)
        torch.cuda.synchronize()
        got[M] = po.detach().cpu().numpy()[:, 0]
        with torch.no_grad():
            want = orc.decoder(torch.from_numpy(s[:M]), PX.PASS_D1, 0, stage).double().numpy()[:, 0]
            exact = o64.decoder(torch.from_numpy(s[:M]).double(), PX.PASS_D1, 0, stage).numpy()[:, 0]
        g = got[M].astype(np.float64)
        assert g.shape == want.shape == exact.shape == (M, 64, 64) and np.isfinite(g).all()
        # the premise: the images vary at the last rows and columns (a dead edge would not test x[32] = 0)
        assert float(exact[:, -1, :].std()) > 1e-4 and float(exact[:, :, -1].std()) > 1e-4, (family, M)
        for name, sel in bands():
            e_eng = float(np.abs(g[:, sel] - exact[:, sel]).max())
            e_32 = float(np.abs(want[:, sel] - exact[:, sel]).max())
            ulp = float(np.spacing(np.float32(np.abs(exact[:, sel]).max())))
            assert e_eng <= ALPHA * e_32 + BETA * ulp, (family, M, name, e_eng, e_32, ulp)
    # the images of rows 0..23 are the same computation in both launches: k_dec_b4<4> and k_dec_b4<1> agree bit for bit
    assert np.array_equal(got[24].view(np.uint32), got[160][:24].view(np.uint32)), family
