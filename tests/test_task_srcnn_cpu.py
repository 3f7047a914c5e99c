"""Task dispatch of ``generator_type`` (reference task.py:141,235-239), on the CPU with a stub generator: "srcnn" picks
the MSE loss and calls the generator with the batch's ``lr`` alone; every other type keeps L1 and the three-argument
call.  The stand-alone SRCNN's constructor contract and the parents' inert ``srcnn`` child are checked here as well."""
import pytest
import torch
import torch.nn as nn


class Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(1))
        self.calls = []

    def forward(self, *args):
        self.calls.append(args)
        return args[0][:, :1] * self.w


def _batch():
    g = torch.Generator().manual_seed(1)
    return {"lr": torch.rand((2, 3, 8, 8), generator=g), "hr": torch.rand((2, 1, 8, 8), generator=g),
            "elevation": torch.rand((2, 1, 8, 8), generator=g), "mask": torch.ones((2, 1, 8, 8))}


def test_srcnn_task_uses_mse_and_one_argument():
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    stub = Stub()
    m = SuperResolutionLightningModule(generator=stub, generator_type="srcnn")
    assert type(m.loss).__name__ == "MSELoss"
    bt = _batch()
    hr, sr = m.common_step(bt)
    assert len(stub.calls) == 1 and len(stub.calls[0]) == 1 and stub.calls[0][0] is bt["lr"]
    assert hr is bt["hr"] and sr.shape == hr.shape


def test_other_generator_types_keep_l1_and_three_arguments():
    from climsr_amd.task.pl_generator_pre_training import SuperResolutionLightningModule

    for kw in ({"generator_type": "esrgan"}, {}):
        stub = Stub()
        m = SuperResolutionLightningModule(generator=stub, **kw)
        assert type(m.loss).__name__ == "L1Loss"
        bt = _batch()
        m.common_step(bt)
        assert len(stub.calls) == 1 and len(stub.calls[0]) == 3
        assert stub.calls[0][0] is bt["lr"] and stub.calls[0][1] is bt["elevation"] and stub.calls[0][2] is bt["mask"]


def test_standalone_srcnn_constructor_contract():
    from climsr_amd.models.srcnn import SRCNN

    with pytest.raises(NotImplementedError, match="out_channels"):
        SRCNN(in_channels=3, out_channels=3)
    net = SRCNN(in_channels=2, scale_factor=4)  # extra kwargs are swallowed as in the reference (srcnn.py:7)
    assert list(net.state_dict()) == [f"conv{k}.{t}" for k in (1, 2, 3) for t in ("weight", "bias")]
    assert net.conv1.weight.shape == (64, 2, 9, 9) and net.conv3.weight.shape == (1, 32, 5, 5)
    assert net._flat.numel() == sum(p.numel() for p in net.parameters()) and net._flat_intact()
    assert hasattr(net, "repack_weights")  # what the instantiator keys the fused AdamW on
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 2, 8, 8))


def test_parents_srcnn_child_is_inert():
    """ESRGANGenerator / RCAN keep ``srcnn.conv{1,2,3}`` as a plain container: it has no flat buffer of its own, and the
    ESRGAN parent's flat index still ends with its six tensors in the reference's order."""
    from climsr_amd.models.esrgan import ESRGANGenerator
    from climsr_amd.models.rcan import RCAN

    g = ESRGANGenerator(3, 1, nf=64, nb=1, gc=16)
    r = RCAN(n_resgroups=1, n_resblocks=1)
    for parent in (g, r):
        assert not hasattr(parent.srcnn, "_flat") and not hasattr(parent.srcnn, "_flat_index")
        assert [k for k in parent.state_dict() if k.startswith("srcnn.")] == \
            [f"srcnn.conv{k}.{t}" for k in (1, 2, 3) for t in ("weight", "bias")]
    tail = [p for p, _o, _n in g._flat_index][-6:]
    want = [g.srcnn.conv1.weight, g.srcnn.conv1.bias, g.srcnn.conv2.weight, g.srcnn.conv2.bias, g.srcnn.conv3.weight,
            g.srcnn.conv3.bias]
    assert all(a is b for a, b in zip(tail, want)) and g._flat_intact()
