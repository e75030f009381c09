"""daimc_amd.Adam: torch.optim.Adam (default flags: no amsgrad, no weight decay) for the parts of the model the engine trains on the
device: the habit network ModelTop.qpi_net (six parameters, C ABI part "top"), the transition network ModelMid.ps_net (eight
parameters, part "ps_net") and, at 1 x 64 x 64, the encoder / decoder ModelDown (32 parameters, 4 787 125 elements).  One optimiser
holds one part.  The update runs on the engine's master copy of the weights: csrc/train.hip (k_adam, which also refreshes the two packed
copies of the small nets) or, for ModelDown, csrc/train_down.hip (k_adam_down, then k_repack_down rebuilds every packed forward form;
efe_down_adam_step).  This class holds the part's name, the optimiser state (exp_avg, exp_avg_sq: flat device tensors in parameters()
order) and the step count, and speaks torch.optim.Adam's state_dict format for the part's parameters, so state moves both ways between
the two.

`Adam(model.model_down, any_geometry=True)` is the optimiser over ModelDown at the model's OWN geometry (C ABI count "down_g"; every
admitted one, 1 x 64 x 64 included): the same state layout and state_dict format, the step through efe_down_adam_step_g
(csrc/train_down_g.hip rebuilds the generic path's packed forms; at 1 x 64 x 64 it is the step above on the same master copy)."""
import torch

from .model import _TrainableModule


def _torch_group():
    """torch.optim.Adam's param-group keys and defaults of the installed torch (load_state_dict of either side sees what it expects)"""
    return dict(torch.optim.Adam([torch.zeros(1)]).state_dict()['param_groups'][0])


class Adam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, any_geometry=False):
        mod = params if isinstance(params, _TrainableModule) else getattr(params, 'module', None)
        if not isinstance(mod, _TrainableModule):
            raise TypeError('daimc_amd.Adam takes model.model_top, model.model_mid, model.model_down or the parameters() of one of them '
                            '(the trainable parts)')
        own = mod._owner
        if any_geometry and mod._train_part != 'down':
            raise ValueError('daimc_amd.Adam: any_geometry selects the run-time-geometry step of ModelDown; the habit and transition '
                             'networks have one geometry')
        if mod._train_part == 'down' and not any_geometry and (own.colour_channels, own.resolution) != (1, 64):
            raise ValueError(f'daimc_amd.Adam: ModelDown is trainable on the engine at 1 x 64 x 64 only, this model is '
                             f'{own.colour_channels} x {own.resolution} x {own.resolution}')
        self._module = mod
        self._any_geometry = bool(any_geometry)     # ModelDown through efe_g.down_adam_step / efe_g.train_down
        self._part = mod._train_part                # the part's name in the C ABI: "top" / "ps_net"; "down": the step's own entry point
        self._shapes = [tuple(t.shape) for t in mod._sd_host.values()]
        self._numel = [int(torch.Size(s).numel()) for s in self._shapes]
        group = _torch_group()
        group.update(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), params=list(range(len(self._shapes))))
        self.param_groups = [group]
        self._step = 0
        self.exp_avg = self.exp_avg_sq = None

    # ---- state ------------------------------------------------------------------------------------------------------
    def _buffers(self):
        if self.exp_avg is None:
            dev = self._module._owner.device
            self.exp_avg = torch.zeros(sum(self._numel), dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        return self.exp_avg, self.exp_avg_sq

    def _hyper(self):
        g = self.param_groups[0]
        if g.get('weight_decay', 0) or g.get('amsgrad', False) or g.get('maximize', False):
            raise ValueError('daimc_amd.Adam: weight_decay, amsgrad and maximize are not implemented (the reference uses none)')
        return float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps'])

    def zero_grad(self, set_to_none=True):
        """no-op: the engine never accumulates gradients"""

    def step(self, grad):
        """one update with the caller's gradient: the dict loss.grad_top / grad_mid / grad_down / grad_down_g returns, or the flat [P]
        tensor (parameters() order)"""
        m = self._module._owner
        e = m._ready()
        if isinstance(grad, dict):
            grad = torch.cat([e.tensor(grad[k]).reshape(-1) for k in self._module._sd_host])
        grad = e.tensor(grad).reshape(-1)
        ea, es = self._buffers()
        hyper = self._hyper()
        if self._any_geometry:
            torch.ops.efe_g.down_adam_step(e.h, grad, ea, es, *hyper, self._step + 1)
        elif self._part == 'down':
            e.ops.down_adam_step(e.h, grad, ea, es, *hyper, self._step + 1)
        else:
            e.ops.adam_step(e.h, self._part, grad, ea, es, *hyper, self._step + 1)
        self._step += 1
        self._module._stepped()

    def state_dict(self):
        state = {}
        if self._step > 0:
            ea, es = (t.cpu() for t in self._buffers())
            off = 0
            for i, (shape, n) in enumerate(zip(self._shapes, self._numel)):
                state[i] = {'step': torch.tensor(float(self._step)), 'exp_avg': ea[off:off + n].reshape(shape).clone(),
                            'exp_avg_sq': es[off:off + n].reshape(shape).clone()}
                off += n
        group = dict(self.param_groups[0])
        group['params'] = list(range(len(self._shapes)))
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self._shapes):
            raise ValueError(f'daimc_amd.Adam: expected one param group of {len(self._shapes)} parameters')
        group = dict(self.param_groups[0], **{k: v for k, v in groups[0].items() if k != 'params'})
        state = sd['state']
        if not state:
            self.param_groups, self._step, self.exp_avg, self.exp_avg_sq = [group], 0, None, None
            return
        ids = list(groups[0]['params'])
        steps, ea, es = set(), [], []
        for pid, shape in zip(ids, self._shapes):
            st = state[pid]
            if tuple(st['exp_avg'].shape) != shape or tuple(st['exp_avg_sq'].shape) != shape:
                raise ValueError(f'daimc_amd.Adam: state of parameter {pid} has shape {tuple(st["exp_avg"].shape)}, expected {shape}')
            steps.add(int(float(st['step'])))
            ea.append(torch.as_tensor(st['exp_avg']).detach().to('cpu', torch.float32).reshape(-1))
            es.append(torch.as_tensor(st['exp_avg_sq']).detach().to('cpu', torch.float32).reshape(-1))
        if len(steps) != 1:
            raise ValueError(f'daimc_amd.Adam: the parameters carry different step counts {sorted(steps)}')
        dev = self._module._owner.device
        self.param_groups, self._step = [group], steps.pop()
        self.exp_avg, self.exp_avg_sq = torch.cat(ea).to(dev).contiguous(), torch.cat(es).to(dev).contiguous()
