"""k_dec_a / k_dec_a_s compute ConvT2 by F(2, 2) over 8 x 8 blocks of 2 x 2 layer-1 pixels (decoder.hip f22_l2): the last block row and
column read x_2 = 0 behind the image, a wave of k_dec_a owns two block rows, a workgroup of k_dec_a_s one.  A ConvT2 edge block covers
4 y2 pixels, i.e. 8 pixels of the decoder's image.  The images are checked against the fp32 CPU oracle on these border bands and inside,
separately, by the fp64 parity rule of tests/test_fp64_parity.py (max|engine - fp64| <= ALPHA max|fp32 oracle - fp64| + BETA ulp), for the
small launch (k_dec_a_s) and the persistent one (k_dec_a); the images both launches share must agree bit for bit; and a call with a row
mask (dead images keep k_dec_a's schedule and skip its work) leaves the live rows' results unchanged."""
import numpy as np
import pytest
import torch

from oracle import philox as PX
from oracle import synth
from oracle.efe_oracle import OracleModel, PhiloxNoise

ALPHA, BETA = 4.0, 8.0


def bands():
    first = np.zeros((64, 64), bool)
    first[:8], first[:, :8] = True, True
    last = np.zeros((64, 64), bool)
    last[-8:], last[:, -8:] = True, True                      # the blocks whose x_2 is the zero row / column
    first &= ~last
    return (('last', last), ('first', first), ('inside', ~(last | first)))


def model(weights, seed):
    import daimc_amd
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=seed, init_weights=False)
    m.load_flat_weights(weights)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['control', 'gain2'])
def test_decoder_images_at_the_block_edges(family):
    seed, stage = 7, 21
    weights = synth.make_weights(1234, 1.15) if family == 'control' else synth.stress_weights(family)
    m = model(weights, seed)
    orc = OracleModel(weights, PhiloxNoise(seed))
    o64 = OracleModel(weights, PhiloxNoise(seed), dtype=torch.float64)
    s = PX.uniform_fill(4, (160, 10), 91, -2.5, 2.5).astype(np.float32)
    got = {}
    for M in (24, 160):          # <= 128 images: k_dec_a_s; above: k_dec_a
        po = m.model_down.decoder(s[:M], stage=stage, pass_=PX.PASS_D1)
        torch.cuda.synchronize()
        got[M] = po.detach().cpu().numpy()[:, 0]
        with torch.no_grad():
            want = orc.decoder(torch.from_numpy(s[:M]), PX.PASS_D1, 0, stage).double().numpy()[:, 0]
            exact = o64.decoder(torch.from_numpy(s[:M]).double(), PX.PASS_D1, 0, stage).numpy()[:, 0]
        g = got[M].astype(np.float64)
        assert g.shape == want.shape == exact.shape == (M, 64, 64) and np.isfinite(g).all()
        # the premise: the images vary at the last rows and columns (a dead edge would not test x_2 = 0)
        assert float(exact[:, -1, :].std()) > 1e-4 and float(exact[:, :, -1].std()) > 1e-4, (family, M)
        for name, sel in bands():
            e_eng = float(np.abs(g[:, sel] - exact[:, sel]).max())
            e_32 = float(np.abs(want[:, sel] - exact[:, sel]).max())
            ulp = float(np.spacing(np.float32(np.abs(exact[:, sel]).max())))
            print(f'{family} M={M} {name}: e_eng {e_eng:.3e} e_32 {e_32:.3e} ulp {ulp:.3e}')
            assert e_eng <= ALPHA * e_32 + BETA * ulp, (family, M, name, e_eng, e_32, ulp)
    # the images of rows 0..23 are the same computation in both launches: k_dec_a_s and k_dec_a agree bit for bit
    assert np.array_equal(got[24].view(np.uint32), got[160][:24].view(np.uint32)), family


@pytest.mark.gpu
def test_row_mask_keeps_the_live_rows_of_the_persistent_launch():
    from daimc_amd.model import Rows
    m = model(synth.make_weights(1234, 1.15), 33)
    A, Eps, S = 4, 16, 3                                        # 64 rows x 3 samples = 192 decoder images per step: k_dec_a
    M = A * Eps
    s0 = PX.uniform_fill(2, (M, 10), 77, -1, 1)
    pi0 = np.eye(4, dtype=np.float32)[np.arange(M) % 4]
    ref = m.calculate_G(s0, pi0, samples=S, stage=4)
    alive = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 1], dtype=torch.uint8, device=m.device)
    out = m.calculate_G(s0, pi0, samples=S, stage=4, rows=Rows(mask=alive, rows_per_entry=A))
    rows = alive.bool().repeat_interleave(A)
    assert torch.equal(out[0][rows], ref[0][rows])                       # G
    for k in range(3):
        assert torch.equal(out[1][k][rows], ref[1][k][rows])             # terms
    assert torch.equal(out[4][rows], ref[4][rows])                       # po1
    again = m.calculate_G(s0, pi0, samples=S, stage=4)                   # the mask belonged to that call only
    assert torch.equal(again[0], ref[0]) and torch.equal(again[4], ref[4])
