"""ORACLE / test infrastructure: deterministic synthetic weights and frames.

No trained checkpoint or dSprites file ships with the reference
(`/root/reference/.MISSING_LARGE_BLOBS`), so tests and the bench synthesise
weights of the reference architecture (`/root/reference/src/torchmodel.py:10-128`,
state_dict key names of SURVEY.md section 8b) from the Philox stream.
Bounds are He-uniform-like with a gain chosen so the decoder leaves the
p = 0.5 plateau and G depends visibly on (s, pi).
"""
import numpy as np
from . import philox as PX

# (key, shape, fan_in)
SPECS = [
    ('top.qpi_net.0', (128, 10)), ('top.qpi_net.2', (128, 128)), ('top.qpi_net.4', (4, 128)),
    ('mid.ps_net.0', (512, 14)), ('mid.ps_net.3', (512, 512)), ('mid.ps_net.6', (512, 512)), ('mid.ps_net.9', (20, 512)),
    ('down.qs_net.0', (32, 1, 3, 3)), ('down.qs_net.2', (32, 32, 3, 3)), ('down.qs_net.4', (64, 32, 3, 3)),
    ('down.qs_net.6', (64, 64, 3, 3)), ('down.qs_net.9', (256, 576)), ('down.qs_net.12', (256, 256)),
    ('down.qs_net.15', (256, 256)), ('down.qs_net.18', (20, 256)),
    ('down.po_net.0', (256, 10)), ('down.po_net.3', (256, 256)), ('down.po_net.6', (256, 256)),
    ('down.po_net.9', (16384, 256)),
    # ConvTranspose2d weights are [Cin, Cout, kh, kw]
    ('down.po_net.13', (64, 64, 3, 3)), ('down.po_net.15', (64, 64, 3, 3)),
    ('down.po_net.17', (64, 32, 3, 3)), ('down.po_net.19', (32, 1, 3, 3)),
]
CONVT = {'down.po_net.13': 1, 'down.po_net.15': 2, 'down.po_net.17': 2, 'down.po_net.19': 1}  # stride


def _fan_in(name, shape):
    if len(shape) == 2:
        return shape[1]
    if name in CONVT:      # transposed conv: each output sees ~ Cin*9/stride^2 inputs
        return shape[0] * 9 / (CONVT[name] ** 2)
    return shape[1] * 9


def specs_for(pi_dim=4, channels=1, resolution=64):
    """(key, shape) list for a geometry: SPECS for the reference's dSprites model; build-defined sizes otherwise"""
    if (pi_dim, channels, resolution) == (4, 1, 64):
        return SPECS
    h = resolution
    for _ in range(4):
        h = (h - 3) // 2 + 1
    base = resolution // 2 if resolution == 32 else resolution // 4
    repl = {'top.qpi_net.4': (pi_dim, 128), 'mid.ps_net.0': (512, pi_dim + 10), 'down.qs_net.0': (32, channels, 3, 3),
            'down.qs_net.9': (256, 64 * h * h), 'down.po_net.9': (64 * base * base, 256), 'down.po_net.19': (32, channels, 3, 3)}
    return [(k, repl.get(k, shp)) for k, shp in SPECS]


def make_weights(seed=1234, gain=1.0, pi_dim=4, channels=1, resolution=64):
    """dict key -> float32 array; keys are '<top|mid|down>.<state_dict key>'."""
    w = {}
    for i, (name, shape) in enumerate(specs_for(pi_dim, channels, resolution)):
        fan = _fan_in(name, shape)
        # dropout(0.5) doubles the second moment of kept activations, so use sqrt(3/fan) for the
        # layers that follow a dropout and sqrt(6/fan) elsewhere; overall scale via `gain`.
        g = 1.0 if name.startswith('mid.') else gain      # transition net: keep the depth recursion contractive
        bound = g * np.sqrt(3.0 / fan)
        w[name + '.weight'] = PX.uniform_fill(seed, shape, 2 * i, -bound, bound)
        bshape = (shape[1],) if name in CONVT else (shape[0],)
        w[name + '.bias'] = PX.uniform_fill(seed, bshape, 2 * i + 1, -0.1, 0.1)
    w['mid.ps_net.9.weight'] *= 0.3   # bounded imagined states over >= 7 chained stages
    # final logvar halves: keep them moderate so exp(0.5*logvar) stays O(0.3)
    for k in ('mid.ps_net.9', 'down.qs_net.18'):
        w[k + '.bias'][10:] -= 2.0
    return w


def make_frames_rgb(seed, n, channels=3, resolution=84):
    """[n, C, R, R] float32 synthetic colour frames (a filled box per channel on a dim background), values in [0, 1]"""
    u = PX.uniform_fill(seed, (n, channels, 5), 2000, 0.0, 1.0)
    frames = np.zeros((n, channels, resolution, resolution), dtype=np.float32)
    for i in range(n):
        for c in range(channels):
            side = 8 + int(u[i, c, 0] * (resolution // 3))
            y = int(u[i, c, 1] * (resolution - side)); x = int(u[i, c, 2] * (resolution - side))
            frames[i, c] = 0.1 * u[i, c, 3]
            frames[i, c, y:y + side, x:x + side] = 0.5 + 0.5 * u[i, c, 4]
    return frames


def make_frames(seed, n):
    """[n, 1, 64, 64] float32 dSprites-like frames: one filled square plus the reward bar of
    `/root/reference/src/game_environment.py:44-54,70-71` (rows 0..2, left half = +r, right half = -r)."""
    u = PX.uniform_fill(seed, (n, 4), 1000, 0.0, 1.0)
    frames = np.zeros((n, 1, 64, 64), dtype=np.float32)
    for i in range(n):
        side = 6 + int(u[i, 0] * 18)
        y = 3 + int(u[i, 1] * (61 - side))
        x = int(u[i, 2] * (64 - side))
        frames[i, 0, y:y + side, x:x + side] = 1.0
        r = 2.0 * u[i, 3] - 1.0
        if r > 0:
            frames[i, 0, 0:3, 0:32] = r
        else:
            frames[i, 0, 0:3, 32:64] = -r
    return frames


# --------------------------------------------------------------------------
# stress families: weights that drive the kernels into the regimes the fixture family (make_weights at gains 1.00 / 1.15 / 1.35,
# images around p = 0.5) never reaches.  Each one names the hazard it targets; tests/test_fp64_oracle.py checks that it still
# reaches its regime.  make_weights itself is untouched: every fixture depends on it bit for bit.
# --------------------------------------------------------------------------
STRESS_FAMILIES = ('seed2', 'gain2', 'sparse', 'saturated')


def stress_weights(family, pi_dim=4, channels=1, resolution=64):
    """dict key -> float32 array for one stress family (any geometry):
      * 'seed2'     -- gain 1.15 from another weight seed: a second draw of the fixture family (control).
      * 'gain2'     -- gain 2.0: large pre-activations, cancellation in term2_1 - term2_2, about half the pixels below 1e-3 (the
                       encoder's output layer scaled back, see below, so that rollouts stay finite).
      * 'sparse'    -- trained-like: per-layer weight scales spread over a decade (fixed Philox draw), biases uniform in +-1 (the
                       logvar halves kept at make_weights' -2 offset), a transition net above gain 1 that is still contractive over
                       depth 5, and po_net.19 (weights x 6, bias -6) such that most pixels are dark, as in dSprites: p ln p on tiny p.
      * 'saturated' -- po_net.19 weights x 40: some pre-sigmoids above +17 (p rounds to 1 in fp32, 1 - p = 0) and some below -89
                       (hw_sigmoid's exp2 overflows to p = 0 where torch gives a denormal; csrc/mfma_pipe.h hw_sigmoid)."""
    geo = (pi_dim, channels, resolution)
    if family == 'seed2':
        return make_weights(4321, 1.15, *geo)
    if family == 'gain2':
        w = make_weights(1234, 2.0, *geo)
        # the encoder's output layer x 2^-6: gain 2 over its eight layers would put the posterior logvar near 110, exp(logvar / 2) near
        # 1e24, and every rollout from a frame would be NaN in the reference itself; its hidden layers keep their large pre-activations
        w['down.qs_net.18.weight'] = w['down.qs_net.18.weight'] * np.float32(2.0 ** -6)
        return w
    if family == 'saturated':
        w = make_weights(1234, 1.15, *geo)
        w['down.po_net.19.weight'] = w['down.po_net.19.weight'] * np.float32(40.0)
        return w
    if family == 'sparse':
        specs = specs_for(*geo)
        scale = 10.0 ** PX.uniform_fill(77, (len(specs),), 3000, -0.5, 0.5)      # per-layer factor in [0.32, 3.2]
        w = {}
        for i, (name, shape) in enumerate(specs):
            fan = _fan_in(name, shape)
            g = 1.3 if name.startswith('mid.') else float(scale[i])
            bound = g * np.sqrt(3.0 / fan)
            w[name + '.weight'] = PX.uniform_fill(77, shape, 3001 + 2 * i, -bound, bound)
            bshape = (shape[1],) if name in CONVT else (shape[0],)
            w[name + '.bias'] = PX.uniform_fill(77, bshape, 3002 + 2 * i, -1.0, 1.0)
        w['mid.ps_net.9.weight'] *= 0.3
        for k in ('mid.ps_net.9', 'down.qs_net.18'):
            w[k + '.bias'][10:] = w[k + '.bias'][10:] * np.float32(0.1) - np.float32(2.0)
        w['down.po_net.19.weight'] *= 6.0         # logits spread over ~ -9 .. -4 around the bias: a quarter of the pixels below 1e-3
        w['down.po_net.19.bias'][:] = -6.0
        return w
    raise ValueError(f'unknown stress family {family!r}')
