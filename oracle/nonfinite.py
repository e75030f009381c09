"""ORACLE -- test infrastructure only.  The poison values and the M = 5 network cases of the non-finite propagation contract (DESIGN.md,
"Non-finite values"): shared by oracle/make_golden_nonfinite.py (the reference's own isnan / isinf masks -> tests/golden/nonfinite_ref.npz),
tests/test_oracle_golden.py (the fp32 oracle reproduces those masks) and tests/test_nonfinite_gpu.py (the engine against the oracle).

A poison is a float32 BIT PATTERN: the two quiet NaNs differ in the sign bit only, which arithmetic keeps or flips but never tests --
a ReLU written as an integer maximum does."""
import numpy as np
import torch

from . import philox as PX
from . import synth

POISONS = {'pnan': 0x7FC00000, 'nnan': 0xFFC00000, 'pinf': 0x7F800000, 'ninf': 0xFF800000}
WSEED, GAIN, NSEED, M, STAGE, BAD_ROW = 1234, 1.15, 7, 5, 40, 2
STATE_ELEM = (BAD_ROW, 3)                    # the poisoned state element
PIXEL = (BAD_ROW, 0, 31, 31)                 # the poisoned observation pixel
NETS = ('habit', 'transition', 'decoder', 'encoder')
# (net, weight key, element): the two weight cases of the fixture -- a pixel-local NaN in the decoder's last dense layer, and a hidden unit of
# the transition network's first layer, which sits behind a dropout mask
WEIGHT_CASES = {'w_dec9': ('decoder', 'down.po_net.9.weight', (100, 0)), 'w_mid0': ('transition', 'mid.ps_net.0.weight', (5, 0))}


def value(name):
    return np.array([POISONS[name]], dtype=np.uint32).view(np.float32)[0]


def poisoned(a, index, name):
    """a copy of the float32 array `a` with the element `index` set to the poison's bit pattern"""
    out = np.array(a, dtype=np.float32, copy=True)
    out.view(np.uint32)[tuple(index)] = np.uint32(POISONS[name])
    return out


def poisoned_weights(weights, key, index, name='pnan'):
    w = dict(weights)
    w[key] = poisoned(weights[key], index, name)
    return w


def base_inputs():
    """the clean M = 5 batch of the nets_* fixtures (oracle/make_golden.py): frames, states, one-hot actions"""
    frames = synth.make_frames(11, M)
    s = PX.uniform_fill(3, (M, 10), 50, -1.5, 1.5)
    pi = np.eye(4, dtype=np.float32)[[0, 1, 2, 3, 1]]
    return frames, s, pi


def cases():
    """{case: (net, weights, frames, s, pi)}: every poison in the input of every network, then the two weight cases"""
    weights = synth.make_weights(WSEED, GAIN)
    frames, s, pi = base_inputs()
    out = {}
    for p in POISONS:
        for net in NETS:
            if net == 'encoder':
                out[f'{net}_{p}'] = (net, weights, poisoned(frames, PIXEL, p), s, pi)
            else:
                out[f'{net}_{p}'] = (net, weights, frames, poisoned(s, STATE_ELEM, p), pi)
    for name, (net, key, index) in WEIGHT_CASES.items():
        out[name] = (net, poisoned_weights(weights, key, index), frames, s, pi)
    return out


def run_net(call, net, frames, s, pi):
    """the outputs of one network, concatenated row-wise into [M, n].  call: {net: function of the tensors} -> tuple of tensors"""
    t = torch.from_numpy
    outs = call[net](t(frames)) if net == 'encoder' else call[net](t(pi), t(s)) if net == 'transition' else call[net](t(s))
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    return np.concatenate([o.detach().numpy().reshape(M, -1) for o in outs], axis=1)


def oracle_calls(orc):
    return {'habit': orc.encode_s, 'transition': lambda pi, s: orc.transition_with_sample(pi, s, PX.PASS_T1, 0, STAGE),
            'decoder': lambda s: orc.decoder(s, PX.PASS_D1, 0, STAGE), 'encoder': lambda o: orc.encoder_with_sample(o, PX.PASS_E1, 0, STAGE)}
