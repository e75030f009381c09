"""The reference of ModelDown's training step at every admitted geometry (loss.train_model_down_g): tests/train_enc_g_ref.py's composed
loss F_down.mean() differentiated by autograd on the CPU in a given dtype, and torch.optim.Adam over the 32 tensors in parameters() order.
One step takes the fourteen ReLU / dropout gates the engine had BEFORE that step (so a pre-activation within rounding of zero cannot send
the two runs down different branches); the weights, exp_avg and exp_avg_sq of each dtype evolve on their own."""
import numpy as np
import torch

import train_enc_g_ref as TEG

KEYS = TEG.KEYS


class AdamRun:
    """weights `w0` ({'down.<key>': array}) trained in `dtype`"""

    def __init__(self, w0, C, R, dtype, lr, stage):
        self.C, self.R, self.dtype, self.stage = C, R, dtype, stage
        self.params = [torch.nn.Parameter(torch.tensor(np.array(w0['down.' + k])).to(dtype)) for k in KEYS]
        self.opt = torch.optim.Adam(self.params, lr=lr)
        self.F = []

    def weights(self):
        return {'down.' + k: p.detach().numpy() for k, p in zip(KEYS, self.params)}

    def step(self, o1, pm, pv, om, gates=None, dec_gates=None):
        out = TEG.run(self.weights(), o1, pm, pv, om, self.C, self.R, self.stage, self.dtype, gates=gates, dec_gates=dec_gates)
        self.F.append(float(np.mean(out['F_down'])))
        for k, p in zip(KEYS, self.params):
            p.grad = torch.as_tensor(np.array(out['grads'][k])).to(self.dtype)
        self.opt.step()
        return out

    def state(self):
        """-> (weights, exp_avg, exp_avg_sq), lists of arrays in parameters() order"""
        return ([p.detach().numpy() for p in self.params], [self.opt.state[p]['exp_avg'].numpy() for p in self.params],
                [self.opt.state[p]['exp_avg_sq'].numpy() for p in self.params])
