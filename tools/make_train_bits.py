#!/usr/bin/env python
"""Writes tests/golden/train_bits.npz: the outputs of the training calls under csrc/train_mlp.h's order contract (habit net, transition
net, the decoder's dense head), of the decoder-gradient host path and of the calls under csrc/train_conv.h's and csrc/block_sum.h's (the
encoder's gradient, grad_down, one whole training step), stored bit for bit, so that a change that claims to leave
every sum's order alone can be held to it (tests/test_train_bits_frozen_gpu.py).

Run it ONCE, on the GPU, on the build of the commit BEFORE the kernel change (the fixture tests new code against its parent, never
against itself):

    python tools/make_train_bits.py [out.npz]

Weights synth.make_weights(1234, 1.15), model seed 11.  The cases (run_cases() is shared with the test) are the smallest shapes at which
these kernels can still go wrong:
  top_m3 / top_m17 / top_m1025   loss.grad_top: one partial tile (rows >= M contribute exact zeros); two workgroups, the second with one
                                 live row; 64 workgroups, workgroup 0 walking a second tile (the add path of `first`)
  top_pi3_m17                    the same at pi_dim 3 (3 x 32 x 32 context): a padded output tile
  top_step_m17                   loss.train_model_top, one step: master weights, exp_avg, exp_avg_sq
  mid_m3 / mid_m17 / mid_m129    loss.grad_mid under a non-default key (stage 5, row_offset 3); 129 = 16 * 8 + 1: a second tile
  mid_pi3_m17                    the same at pi_dim 3: the first layer's K = 13 is padded
  mid_step_m17                   loss.train_model_mid, one step
  dec_m1 / dec_m17 / dec_m65     loss.grad_decoder(return_activations=True), stage 5, row_offset 3: two tiles and two slabs; a second
                                 64-row group (first = 0 in k_dech_w4grad and in the slabs)
  dectail_m5                     loss.grad_decoder_convs on the first 5 rows of dec_m17's h4: the host path without the head
  enc_m1 / enc_m33 / enc_m65     loss.grad_encoder(return_activations=True), stage 5, row_offset 3.  G = 1: the one slab is the gradient (the
                                 `first` store alone) and the head has one ragged tile; 32 slabs, slab 0 walking a second image (the add
                                 of the row loop) and a third, ragged 16-row head tile; a second 64-row group (first = 0: the
                                 read-add-write path of the slabs in all three parameter-gradient passes)
  down_m17                       loss.grad_down on device normals: k_dect_loss and k_fe_down on the same images, k_down_latent, the
                                 encoder's and the decoder's gradient in one array
  step_m257                      loss.train_step, one step, omega derived: k_step_means with a second strided add in thread 0 alone, and
                                 every trained weight and Adam moment behind it

Storage: an array of up to 16 384 elements is stored whole under '<case>.<name>'; a larger one as '<case>.<name>.sha256' (the digest of
its little-endian float32 bytes) and '<case>.<name>.every4099' (elements 0, 4099, 8198, ... of the flattened array).  The decoder's
gradient (4.4 M floats; 92 609 for the tail alone) is stored in that form per state_dict key, '<case>.grad.<key>.*', whatever the key's size,
so that a failure names the layer.  (16 384, not 65 536: with the larger bound the seven habit-net vectors of 18 436 floats and dec_m1's
y2 are stored whole and the file is 888 KB; with this one it was 182 KB, and is 364 KB with the enc_*, down_* and step_* cases, below
MAX_BYTES, the 512 KiB the other training fixtures keep to.)"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, 'tests', 'golden', 'train_bits.npz')
CASES = ('top_m3', 'top_m17', 'top_m1025', 'top_pi3_m17', 'top_step_m17', 'mid_m3', 'mid_m17', 'mid_m129', 'mid_pi3_m17', 'mid_step_m17',
         'dec_m1', 'dec_m17', 'dec_m65', 'dectail_m5', 'enc_m1', 'enc_m33', 'enc_m65', 'down_m17', 'step_m257')
WHOLE, STRIDE = 16384, 4099
MAX_BYTES = 512 * 1024
KEY = dict(stage=5, row_offset=3)
GENERIC = (3, 3, 32)            # pi_dim, colour channels, resolution of the *_pi3_* cases


def _c(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _flat(d):
    return np.concatenate([_c(v).reshape(-1) for v in d.values()])


def _top_batch(seed, M, A=4):
    r = np.random.RandomState(seed)
    s = r.randn(M, 10).astype(np.float32)
    z = (2.0 * r.randn(M, A)).astype(np.float64)
    z -= z.max(1, keepdims=True)
    return s, (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def _mid_batch(seed, M, A=4):
    r = np.random.RandomState(seed)
    s0 = r.randn(M, 10).astype(np.float32)
    pi = np.eye(A, dtype=np.float32)[r.randint(0, A, M)]
    qm = r.randn(M, 10).astype(np.float32)
    qv = (0.5 * r.randn(M, 10) - 1.0).astype(np.float32)
    return s0, qm, qv, pi, r.uniform(1.5, 2.5, M).astype(np.float32)


def _dec_batch(seed, M):
    r = np.random.RandomState(seed)
    return r.randn(M, 10).astype(np.float32), (r.uniform(size=(M, 1, 64, 64)) < 0.1).astype(np.float32)


def _enc_batch(seed, M):
    r = np.random.RandomState(seed)
    o = (r.uniform(size=(M, 1, 64, 64)) < 0.1).astype(np.float32)
    return o, r.randn(M, 10).astype(np.float32), r.randn(M, 10).astype(np.float32)


def _down_batch(seed, M):
    r = np.random.RandomState(seed)
    o1 = (r.uniform(size=(M, 1, 64, 64)) < 0.1).astype(np.float32)
    return o1, r.randn(M, 10).astype(np.float32), (0.5 * r.randn(M, 10) - 1.0).astype(np.float32), r.uniform(1.5, 2.5, M).astype(np.float32)


def _step_batch(seed, M, A=4):
    r = np.random.RandomState(seed)
    o0, o1 = ((r.uniform(size=(M, 1, 64, 64)) < 0.1).astype(np.float32) for _ in range(2))
    z = (2.0 * r.randn(M, A)).astype(np.float64)
    z -= z.max(1, keepdims=True)
    return o0, o1, np.eye(A, dtype=np.float32)[r.randint(0, A, M)], (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def _step(module, opt):
    sd = module.state_dict()
    return {'w': _flat(sd), 'exp_avg': _c(opt.exp_avg), 'exp_avg_sq': _c(opt.exp_avg_sq)}


def run_cases(device='cuda:0'):
    """-> {case: {name: float32 array}}, every array whole"""
    import daimc_amd
    from daimc_amd import loss
    from oracle import synth

    def model(geo=(4, 1, 64)):
        m = daimc_amd.ActiveInferenceModel(10, geo[0], 0.0, 1.0, 1.0, colour_channels=geo[1], resolution=geo[2], device=device, seed=11,
                                           init_weights=False)
        m.load_flat_weights(synth.make_weights(1234, 1.15, *geo))
        return m
    m, mg = model(), model(GENERIC)
    out = {}
    for name, mod, M, A in (('top_m3', m, 3, 4), ('top_m17', m, 17, 4), ('top_m1025', m, 1025, 4), ('top_pi3_m17', mg, 17, 3)):
        kl, g = loss.grad_top(mod.model_top, *_top_batch(300 + M, M, A))
        out[name] = {'kl': _c(kl), 'grad': _flat(g)}
    for name, mod, M, A in (('mid_m3', m, 3, 4), ('mid_m17', m, 17, 4), ('mid_m129', m, 129, 4), ('mid_pi3_m17', mg, 17, 3)):
        F, mean, lv, g = loss.grad_mid(mod.model_mid, *_mid_batch(400 + M, M, A), **KEY)
        out[name] = {'F_mid': _c(F), 'ps1_mean': _c(mean), 'ps1_logvar': _c(lv), 'grad': _flat(g)}
    mt = model()                   # (the steps change the weights: each gets a model of its own)
    opt = daimc_amd.Adam(mt.model_top, lr=1e-3)
    kl = loss.train_model_top(mt.model_top, *_top_batch(317, 17), opt)
    out['top_step_m17'] = {'kl': _c(kl), **_step(mt.model_top, opt)}
    mm = model()
    opt = daimc_amd.Adam(mm.model_mid, lr=1e-3)
    mean, lv = loss.train_model_mid(mm.model_mid, *_mid_batch(417, 17), opt, **KEY)
    out['mid_step_m17'] = {'ps1_mean': _c(mean), 'ps1_logvar': _c(lv), **_step(mm.model_mid, opt)}
    for M in (1, 17, 65):
        s, o1 = _dec_batch(500 + M, M)
        nl, po1, d_s, g, act = loss.grad_decoder(m.model_down, s, o1, return_activations=True, **KEY)
        d = {'nlogpo1': _c(nl), 'po1': _c(po1), 'd_s': _c(d_s)}
        d.update({n: _c(a) for n, a in zip(('h1', 'h2', 'h3', 'h4', 'y1', 'y2', 'y3'), act)})
        d.update({'grad.' + k: _c(v) for k, v in g.items()})
        out[f'dec_m{M}'] = d
        if M == 17:
            nl, po1, d_h4, g = loss.grad_decoder_convs(m.model_down, d['h4'][:5], o1[:5])
            out['dectail_m5'] = {'nlogpo1': _c(nl), 'po1': _c(po1), 'd_h4': _c(d_h4), **{'grad.' + k: _c(v) for k, v in g.items()}}
    for M in (1, 33, 65):
        mean, lv, g, act = loss.grad_encoder(m.model_down, *_enc_batch(600 + M, M), return_activations=True, **KEY)
        d = {'qs_mean': _c(mean), 'qs_logvar': _c(lv)}
        d.update({n: _c(a) for n, a in zip(('y1', 'y2', 'y3', 'y4', 'h1', 'h2', 'h3'), act)})
        d.update({'grad.' + k: _c(v) for k, v in g.items()})
        out[f'enc_m{M}'] = d
    F, (nl, kls, kln), po1, qs1, qm, qv, g, (gm, gv) = loss.grad_down(m.model_down, *_down_batch(717, 17), return_upstream=True, **KEY)
    out['down_m17'] = {'F_down': _c(F), 'nlogpo1': _c(nl), 'kl_s': _c(kls), 'kl_naive': _c(kln), 'po1': _c(po1), 'qs1': _c(qs1),
                       'qs1_mean': _c(qm), 'qs1_logvar': _c(qv), 'g_mean': _c(gm), 'g_logvar': _c(gv),
                       **{'grad.' + k: _c(v) for k, v in g.items()}}
    ms = model()
    opts = {k: daimc_amd.Adam(getattr(ms, 'model_' + k), lr=1e-3) for k in ('top', 'mid', 'down')}
    res = loss.train_step(ms, *_step_batch(1057, 257), opts, **KEY)
    d = {k: _c(v) for k, v in res._asdict().items()}
    for part, opt in opts.items():
        d.update({f'{part}.{k}': v for k, v in _step(getattr(ms, 'model_' + part), opt).items()})
    out['step_m257'] = d
    torch.cuda.synchronize()
    assert tuple(sorted(out)) == tuple(sorted(CASES))
    return out


def pack(cases):
    """the stored form of run_cases()' result -> {'<case>.<name>[.sha256 | .every4099]': array}"""
    arrs = {}
    for case, d in cases.items():
        for name, a in d.items():
            a = np.ascontiguousarray(a)
            assert a.dtype == np.float32, (case, name, a.dtype)
            if a.size <= WHOLE and not name.startswith('grad.'):
                arrs[f'{case}.{name}'] = a
            else:
                arrs[f'{case}.{name}.sha256'] = np.frombuffer(hashlib.sha256(a.astype('<f4').tobytes()).digest(), dtype=np.uint8)
                arrs[f'{case}.{name}.every4099'] = a.reshape(-1)[::STRIDE].copy()
    return arrs


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


def main(path):
    first, second = run_cases(), run_cases()
    for case in CASES:
        assert list(first[case]) == list(second[case]), case
        for name, a in first[case].items():
            assert np.isfinite(a).all(), f'{case}.{name}: not finite on this build'
            assert bits_equal(a, second[case][name]), f'{case}.{name}: two identical calls disagree on this build'
    assert float(np.abs(first['top_m1025']['grad']).max()) > 0 and float(first['dec_m65']['po1'].std()) > 1e-3      # (not flat)
    arrs = pack(first)
    np.savez_compressed(path, **arrs)
    print(path, os.path.getsize(path), 'bytes,', len(arrs), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT)
