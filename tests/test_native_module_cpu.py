"""The shared autograd node, module mixin and engine base of the native networks (core/native.py), driven on the CPU by
a tiny fake engine: ``y = w * x + b`` written in torch.  Nothing here loads the HIP library."""
import pytest
import torch
import torch.nn as nn

from climsr_amd.core.native import NativeEngine, NativeModule


class _FakeEngine(NativeEngine):
    def __init__(self, owner):
        super().__init__(owner)
        self.packs = 0
        self.runs = []  # (keep, need_w, saved is not None)
        self.backs = []  # (need_w, need_x, accumulate)
        self.gw = self.gb = None

    def pack(self):
        self.packs += 1

    def bind_grads(self):
        self.gw, self.gb = self.owner.w.grad, self.owner.b.grad

    def run(self, x, keep, need_w):
        self.ensure_packed()
        o = self.owner
        saved = dict(x=x.detach().clone()) if keep else None
        self.runs.append((keep, need_w, saved is not None))
        return o.w.detach() * x.detach() + o.b.detach(), saved

    def backward(self, gout, saved, need_w, need_x, accumulate):
        self.backs.append((need_w, need_x, accumulate))
        if need_w:
            gw, gb = (gout * saved["x"]).sum(0), gout.sum(0)
            if accumulate:
                self.gw.add_(gw)
                self.gb.add_(gb)
            else:
                self.gw.copy_(gw)
                self.gb.copy_(gb)
            self.grads_final()
        return gout * self.owner.w.detach() if need_x else None


class _Lin(NativeModule, nn.Module):
    _engine_cls = _FakeEngine
    _label = "lin"
    _device_type = "cpu"

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor([1.0, -2.0, 0.5]))
        self.b = nn.Parameter(torch.tensor([0.25, 0.0, -1.0]))
        self._flatten()

    def forward(self, x):
        return self._native_forward(x)


class _LinDx(_Lin):
    _input_grad = True


X = torch.tensor([[1.0, 2.0, 3.0], [-1.0, 0.5, 4.0]])
GW, GB = X.sum(0), torch.full((3,), 2.0)  # d sum(y) / dw, d sum(y) / db


def _views_ok(net):
    base = net._flat_grad.data_ptr()
    return all(p.grad is not None and p.grad.data_ptr() == base + 4 * off for p, off, _n in net._flat_index)


def test_in_place_route_overwrites_accumulates_and_relinks():
    net = _Lin()
    net._flat_grad.fill_(7.0)  # stale content: the first backward must overwrite it
    net.zero_grad(set_to_none=True)
    net(X).sum().backward()
    assert _views_ok(net)
    assert torch.equal(net._flat_grad, torch.cat([GW, GB]))
    assert net.engine().backs[-1] == (True, False, False)
    net(X).sum().backward()  # no zeroing in between: accumulates
    assert torch.equal(net._flat_grad, 2 * torch.cat([GW, GB])) and torch.equal(net.w.grad, 2 * GW)
    assert net.engine().backs[-1] == (True, False, True)
    net.b.grad = torch.full((3,), 99.0)  # one foreign grad tensor: all are relinked, and the backward overwrites
    net(X).sum().backward()
    assert _views_ok(net) and torch.equal(net._flat_grad, torch.cat([GW, GB]))
    assert net.engine().backs[-1] == (True, False, False)


def test_autograd_route_goes_through_accumulate_grad():
    ref = _Lin()
    ref(X).sum().backward()
    net = _Lin()
    net.grads_through_autograd = True
    seen = []
    net.w.register_hook(lambda g: seen.append(g.clone()))
    net._flat_grad.fill_(7.0)
    prev_w = torch.ones(3)
    net.w.grad = prev_w  # a previous gradient: restored before autograd adds to it; b has none: autograd installs one
    net(X).sum().backward()
    assert len(seen) == 1 and torch.equal(seen[0], GW)  # the tensor hook fired: the gradient came through autograd
    assert torch.equal(net._flat_grad, torch.full((6,), 7.0))  # untouched
    assert net.w.grad is prev_w and torch.equal(prev_w, 1.0 + GW)
    assert torch.equal(net.b.grad, GB) and not _views_ok(net)
    assert net.engine().backs[-1] == (True, False, False)
    assert torch.equal(net.w.grad - 1.0, ref.w.grad) and torch.equal(net.b.grad, ref.b.grad)  # = the in-place route's
    net.set_grad_ready_hook(lambda lo: None)  # the flat-buffer reducer's hook and this route exclude each other
    y = net(X).sum()
    with pytest.raises(RuntimeError, match="grad-ready hook"):
        y.backward()


def test_frozen_parameters_with_an_input_that_requires_grad():
    net = _LinDx()
    net.requires_grad_(False)
    x = X.clone().requires_grad_(True)
    net(x).sum().backward()
    assert torch.equal(x.grad, net.w.detach().expand(2, 3))
    assert net.w.grad is None and net.b.grad is None and torch.equal(net._flat_grad, torch.zeros(6))
    assert net.engine().runs[-1] == (True, False, True)
    assert net.engine().backs[-1] == (False, True, True)  # need_w False: accumulate is passed as True
    # both at once: dx and the parameter gradients
    net.requires_grad_(True)
    x = X.clone().requires_grad_(True)
    net(x).sum().backward()
    assert torch.equal(x.grad, net.w.detach().expand(2, 3)) and torch.equal(net.w.grad, GW)
    # a module that gives no input gradient says so, before anything else
    gen = _Lin()
    gen.requires_grad_(False)
    x = X.clone().requires_grad_(True)
    y = gen(x).sum()
    assert gen.engine().runs[-1] == (False, False, False)
    with pytest.raises(NotImplementedError, match=r"gradient w\.r\.t\. the lin input is not implemented"):
        y.backward()


def test_no_grad_saves_nothing():
    net = _LinDx()
    with torch.no_grad():
        y = net(X.clone().requires_grad_(True))
    assert not y.requires_grad and net.engine().runs[-1] == (False, False, False)
    assert torch.equal(y, net.w.detach() * X + net.b.detach())


def test_one_bucket_hook_and_gpu_only_check():
    net = _Lin()
    ready = []
    net.set_grad_ready_hook(ready.append)
    net(X).sum().backward()
    assert ready == [0]
    net.set_grad_ready_hook(None)
    net(X).sum().backward()
    assert ready == [0]
    net._device_type = "cuda"
    with pytest.raises(RuntimeError, match="GPU only"):
        net(X)


def test_repack_rule():
    net = _Lin()
    eng = net.engine()
    assert eng.packs == 0
    net(X)
    v0 = eng._params_version()
    net(X)
    assert eng.packs == 1 and eng._params_version() == v0  # nothing in between: no re-pack
    other = _Lin()
    with torch.no_grad():
        other.w.add_(1.0)
    net.load_state_dict(other.state_dict())
    v1 = eng._params_version()
    assert v1 != v0
    assert torch.equal(net(X).detach(), other.w.detach() * X + other.b.detach()) and eng.packs == 2
    with torch.no_grad():
        net.b.mul_(2.0)
    v2 = eng._params_version()
    assert v2 != v1
    net(X)
    assert eng.packs == 3
    net._flat.mul_(0.5)  # the flat buffer itself, in place
    v3 = eng._params_version()
    assert v3 != v2
    net(X)
    net(X)
    assert eng.packs == 4 and eng._params_version() == v3
    net.repack_weights()  # what an optimizer calls after writing the buffer behind torch's back
    assert eng.packs == 5 and eng.version == v3


def test_engine_identity():
    net = _Lin()
    eng = net.engine()
    net(X).sum().backward()
    net(X)
    assert net.engine() is eng
    net.w.data = net.w.data.clone()  # something replaced a parameter's storage: the flat buffer is re-homed
    assert not net._flat_intact()
    eng2 = net.engine()
    assert eng2 is not eng and eng2.owner is net and net._flat_intact()
    assert net.engine() is eng2
    net.double()  # an _apply that changes dtype: parameters leave the flat buffer and are brought back
    assert net.engine() is not eng2 and net._flat.dtype == torch.float32


def test_engine_rebuilt_after_apply_only_where_declared():
    class _LinBuffers(_Lin):
        _engine_dies_on_apply = True

    a, b = _Lin(), _LinBuffers()
    ea, eb = a.engine(), b.engine()
    a.float()
    b.float()  # nothing moves, but an engine that also holds buffers is rebuilt after any _apply
    assert a.engine() is ea and b.engine() is not eb
