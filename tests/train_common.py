"""Helpers shared by the GPU tests of the two trainable parts (tests/test_train_top_gpu.py, tests/test_train_mid_gpu.py): weight families, engine
models, the fp64 rule's printing wrapper, synthetic gradients and a torch.optim.Adam run on given gradients.  A plain module, like
train_ref.py; the engine seed of both files is SEED."""
import numpy as np
import torch

from oracle import synth
from test_fp64_parity import fp64_rule

SEED = 7


def c(t):
    return t.detach().cpu().numpy()


_FAMILIES = {}


def family(name, geo=(4, 1, 64)):
    """'g115', 'g100', a stress family of oracle/synth.py, or 'sat_top': 'saturated' with qpi_net.4.weight x 40"""
    key = (name, geo)
    if key not in _FAMILIES:
        if name == 'g115':
            w = synth.make_weights(1234, 1.15, *geo)
        elif name == 'g100':
            w = synth.make_weights(7, 1.0, *geo)
        elif name == 'sat_top':
            w = dict(synth.stress_weights('saturated', *geo))
            w['top.qpi_net.4.weight'] = w['top.qpi_net.4.weight'] * np.float32(40.0)
        else:
            w = synth.stress_weights(name, *geo)
        _FAMILIES[key] = w
    return _FAMILIES[key]


_MODELS = {}


def model_for(name, geo=(4, 1, 64), fresh=False):
    """an engine model with the family's weights; cached ones are for tests that do not train"""
    import daimc_amd
    key = (name, geo)
    if not fresh and key in _MODELS:
        return _MODELS[key]
    m = daimc_amd.ActiveInferenceModel(10, geo[0], 0.5, 1.0, 1.0, colour_channels=geo[1], resolution=geo[2], device='cuda:0', seed=SEED,
                                       init_weights=False)
    m.load_flat_weights(family(name, geo))
    if not fresh:
        _MODELS[key] = m
    return m


def apply_rule(tag, triples):
    """fp64_rule on [(name, eng, o32, o64)]; every figure is printed before the assertion"""
    bad = []
    for name, eng, o32, o64 in triples:
        for r in fp64_rule(name, eng, o32, o64):
            print(f'{tag} {r[0]}: e_eng {r[1]:.3e} e_32 {r[2]:.3e} bound {r[3]:.3e} ratio {r[4]:.2f}')
            if not r[-1]:
                bad.append(r)
    assert not bad, f'{tag}: ' + '; '.join(f'{n}: e_eng {e:.3e} > bound {b:.3e} (e_32 {e3:.3e})' for n, e, e3, b, _, _ in bad)


def synth_grads(seed, shapes):
    """magnitudes 10^U(-12, 2), random signs, 5 % exact zeros"""
    r = np.random.RandomState(seed)
    out = []
    for shp in shapes:
        g = (10.0 ** r.uniform(-12, 2, shp)) * r.choice([-1.0, 1.0], shp)
        g[r.uniform(size=shp) < 0.05] = 0.0
        out.append(g.astype(np.float32))
    return out


def torch_adam_run(keys, w0, grads_per_step, dtype, lr, state=None):
    """torch.optim.Adam over the tensors w0[k], k in keys (parameters() order), fed the given gradients -> (weights, exp_avg, exp_avg_sq)"""
    # (every array is copied: torch wraps fp32 numpy memory without a copy and Adam updates in place)
    params = [torch.nn.Parameter(torch.tensor(np.array(w0[k])).to(dtype)) for k in keys]
    opt = torch.optim.Adam(params, lr=lr)
    if state is not None:
        opt.load_state_dict({'state': {i: {'step': torch.tensor(float(state['step'])), 'exp_avg': torch.tensor(np.array(state['m'][i])).to(dtype),
                                           'exp_avg_sq': torch.tensor(np.array(state['v'][i])).to(dtype)} for i in range(len(keys))},
                             'param_groups': opt.state_dict()['param_groups']})
    for gs in grads_per_step:
        for p, g in zip(params, gs):
            p.grad = torch.as_tensor(g).to(dtype)
        opt.step()
    return ([p.detach().numpy() for p in params], [opt.state[p]['exp_avg'].numpy() for p in params],
            [opt.state[p]['exp_avg_sq'].numpy() for p in params])
