"""CPU tests of ModelDown's optimiser step at every admitted geometry: the C ABI exports and their ctypes signatures, the torch ops'
schemas, daimc_amd.Adam's any_geometry keyword without a device, and tools/emulate_repack_g.py -- the generic host packers and
k_repack_down_g's destination -> source maps restated in numpy, held to each other element for element at all 75 geometries."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_are_declared_listed_and_exported():
    import daimc_amd
    L = daimc_amd._lib
    lib = L.load()
    header = open(os.path.join(ROOT, 'include', 'efe_engine.h')).read()
    for g, s in (('efe_train_down_g', 'efe_train_down'), ('efe_down_adam_step_g', 'efe_down_adam_step'), ('efe_down_get_weights_g', 'efe_down_get_weights')):
        assert f'int {g}(' in header and hasattr(lib, g), g
        assert g in L.SIGNATURES and g in L.EXPORTS and L.SIGNATURES[g] == L.SIGNATURES[s], g
        fn = getattr(lib, g)
        assert tuple(fn.argtypes) == tuple(L.SIGNATURES[g][1]) and fn.restype is L.SIGNATURES[g][0], g
    assert L.ABI_VERSION == 6 and lib.efe_abi_version() == 6
    L.load_ops()
    schema = str(torch.ops.efe_g.train_down.default._schema)
    assert schema.startswith('efe_g::train_down(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o'), schema
    assert 'Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq' in schema and schema.endswith('-> Tensor[]'), schema
    assert str(torch.ops.efe_g.train_down.default._schema).split('(', 1)[1] == str(torch.ops.efe.train_down.default._schema).split('(', 1)[1]
    schema = str(torch.ops.efe_g.down_adam_step.default._schema)
    assert schema.startswith('efe_g::down_adam_step(int ctx, Tensor grad, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq'), schema
    assert schema.split('(', 1)[1] == str(torch.ops.efe.down_adam_step.default._schema).split('(', 1)[1]


def test_stale_handles_are_refused_by_name_without_a_device():
    import ctypes as C
    import daimc_amd
    lib = daimc_amd._lib.load()
    bad = C.c_void_p(0x1234)
    assert lib.efe_down_get_weights_g(bad, None, 0, None) == 1
    assert lib.efe_last_error(bad).decode() == 'efe_down_get_weights_g: stale or invalid context handle'
    assert lib.efe_down_adam_step_g(bad, None, None, None, None, None) == 1
    assert lib.efe_last_error(bad).decode() == 'efe_down_adam_step_g: stale or invalid context handle'
    assert lib.efe_train_down_g(bad, None, None, None, 1, None, None, None, None, None, None, None, None) == 1
    assert lib.efe_last_error(bad).decode() == 'efe_train_down_g: stale or invalid context handle'


class _Owner:
    def __init__(self, C_, R):
        self.colour_channels, self.resolution, self.device = C_, R, 'cpu'


def _module(part, C_=1, R=64):
    """a trainable module as daimc_amd.Adam sees it, without an engine"""
    import daimc_amd
    cls = {'top': daimc_amd.model.ModelTop, 'down': daimc_amd.model.ModelDown}[part]
    mod = cls.__new__(cls)
    mod._owner, mod._part = _Owner(C_, R), part
    mod._sd_host = {'a.weight': torch.zeros(3, 2), 'a.bias': torch.zeros(3)}
    mod.colour_channels, mod.resolution = C_, R
    return mod


def test_adam_keyword_without_a_device():
    import daimc_amd
    down84, down64, top = _module('down', 3, 84), _module('down'), _module('top')
    with pytest.raises(ValueError, match='1 x 64 x 64 only'):        # without the keyword: exactly as before
        daimc_amd.Adam(down84)
    with pytest.raises(ValueError, match='1 x 64 x 64 only'):
        daimc_amd.Adam(down84.parameters())
    with pytest.raises(TypeError):
        daimc_amd.Adam([torch.zeros(1)], any_geometry=True)
    with pytest.raises(ValueError, match='any_geometry'):
        daimc_amd.Adam(top, any_geometry=True)
    with pytest.raises(TypeError):                                   # keyword-only
        daimc_amd.Adam(down84, 1e-3, (0.9, 0.999), 1e-8, True)
    for mod in (down84, down64):
        for params in (mod, mod.parameters()):
            o = daimc_amd.Adam(params, lr=2e-4, any_geometry=True)
            assert o._module is mod and o._any_geometry and o._part == 'down' and o._numel == [6, 3]
            sd = o.state_dict()
            assert sd['state'] == {} and sd['param_groups'][0]['lr'] == 2e-4 and sd['param_groups'][0]['params'] == [0, 1]
            # the state_dict format is torch.optim.Adam's: a state written by it loads, and comes back unchanged
            ps = [torch.nn.Parameter(t.clone()) for t in mod._sd_host.values()]
            t = torch.optim.Adam(ps, lr=1e-3)
            for p in ps:
                p.grad = torch.ones_like(p)
            t.step()
            o.load_state_dict(t.state_dict())
            back = o.state_dict()
            assert o._step == 1 and torch.equal(back['state'][0]['exp_avg'], t.state_dict()['state'][0]['exp_avg'])
            assert torch.equal(back['state'][1]['exp_avg_sq'], t.state_dict()['state'][1]['exp_avg_sq'])
    assert not daimc_amd.Adam(down64)._any_geometry and not daimc_amd.Adam(top)._any_geometry
    assert down84._count_part() == 'down_g' and down64._count_part() == 'down' and top._count_part() == 'top'


def test_train_model_down_g_wants_the_keyword_optimiser():
    import daimc_amd
    down = _module('down', 3, 84)
    with pytest.raises(ValueError, match='any_geometry'):
        daimc_amd.loss.train_model_down_g(down, None, None, None, 1.0, daimc_amd.Adam(_module('down'), any_geometry=True))
    with pytest.raises(ValueError, match='any_geometry'):
        daimc_amd.loss.train_model_down_g(down, None, None, None, 1.0, object())


@pytest.mark.parametrize('C_', [1, 2, 3])
def test_the_maps_invert_the_host_packers_at_every_geometry(C_):
    E = load_tool('emulate_repack_g')
    assert len(E.RES) == 25
    for R in E.RES:
        P, n, blocks = E.check(C_, R)
        g = E.Geo(C_, R)
        assert P == 201684 + 288 * C_ + 256 * g.K + 134400 + 257 * g.F + 92320 + 289 * C_ and n == 46
    assert E.Geo(1, 64).P == 4787125 and E.Geo(3, 84).F * 256 == 7225344 and E.Geo(3, 128).F * 256 == 16777216


def test_the_emulation_catches_a_wrong_map():
    """the comparison is not vacuous: a transposed-conv entry read as a Conv2d, and a missing zero of the padding, both fail"""
    E = load_tool('emulate_repack_g')
    real = E.entry_map

    def conv_for_convt(d):
        return real(dict(d, kind=E.CONV32)) if d['kind'] == E.CONVT32 and d['out'] != d['cin'] else real(d)

    def no_padding(d):
        dst, src = real(d)
        return (dst, abs(src)) if d['name'] == 'g_wf' else (dst, src)
    for wrong in (conv_for_convt, no_padding):
        E.entry_map = wrong
        with pytest.raises(AssertionError):
            E.check(2, 36)
    E.entry_map = real
    E.check(2, 36)
