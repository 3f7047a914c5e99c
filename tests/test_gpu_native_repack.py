"""The one re-pack rule of core/native.py on the GPU: after a forward has packed the bf16 MFMA weights, a
``load_state_dict`` or an in-place write through a parameter must re-pack them, for every natively trained network.
The parameters are views of the flat buffer with version counters of their own, so the flat buffer's counter alone
misses both.  Eval mode under ``no_grad``; the outputs must be bit-identical to those of a network that packed the new
weights first."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _esrgan():
    from climsr_amd.models.esrgan import ESRGANGenerator
    return ESRGANGenerator(3, 1, 64, 1, 16, 4)


def _srcnn():
    from climsr_amd.models.srcnn import SRCNN
    return SRCNN(3, 1)


def _rcan():
    from climsr_amd.models.rcan import TrainableRCAN
    return TrainableRCAN(n_resgroups=1, n_resblocks=1)


def _rfb_d():
    from climsr_amd.models.rfb_esrgan import RFBESRGANDiscriminator
    return RFBESRGANDiscriminator(1)


def _plain_d():
    from climsr_amd.models.discriminator import Discriminator
    return Discriminator(1)


def _inputs(kind):
    g = torch.Generator().manual_seed(5)
    if kind == "d":
        return (torch.rand((2, 1, 128, 128), generator=g).to(DEV),)
    x = torch.rand((1, 3, 16, 16), generator=g)
    if kind == "x":
        return (x.to(DEV),)
    return x.to(DEV), torch.rand((1, 1, 64, 64), generator=g).to(DEV), torch.ones(1, 1, 64, 64, device=DEV)


def _make(factory, seed):
    torch.manual_seed(seed)
    return factory().to(DEV).eval()


CASES = [("esrgan", _esrgan, "g"), ("srcnn", _srcnn, "x"), ("rcan", _rcan, "g"), ("rfb_d", _rfb_d, "d"), ("plain_d", _plain_d, "d")]


@pytest.mark.parametrize("name,factory,kind", CASES, ids=[c[0] for c in CASES])
def test_load_state_dict_after_a_forward_repacks(name, factory, kind):
    a, b = _make(factory, 1), _make(factory, 2)
    inp = _inputs(kind)
    with torch.no_grad():
        want = b(*inp)
        first = a(*inp)
        assert not torch.equal(first, want), "the two seeds must give different networks"
        eng = a.engine()
        a.load_state_dict(b.state_dict())
        got = a(*inp)
    assert a.engine() is eng  # re-packed, not rebuilt
    assert torch.equal(got, want)


def test_in_place_parameter_write_after_a_forward_repacks():
    a, b = _make(_esrgan, 1), _make(_esrgan, 2)
    b.load_state_dict(a.state_dict())
    inp = _inputs("g")
    with torch.no_grad():
        b.conv_first.weight.mul_(2)  # before b's first forward: packed from the doubled weights
        want = b(*inp)
        first = a(*inp)
        assert not torch.equal(first, want)
        a.conv_first.weight.mul_(2)
        got = a(*inp)
    assert torch.equal(got, want)
