"""GPU: the one autograd node of the three discriminators (genvox_amd/_device_module.py, ``_DiscriminatorNode``) owns the blob and the
tape of its forward.  On the TINY configurations of each discriminator's own tests, 2 ragged rows of at most 90 samples, in eval mode
(so that the scale discriminator's spectral buffers stand still and only the test changes a weight):

  - a module that packs again between a forward and its backward - another tensor under one parameter, with other values and no
    version change, then a second forward - differentiates the first forward on the weights it ran on: ``wav.grad`` and every
    parameter's gradient are the bits of an identical module that ran forward and backward with nothing in between (the same launches
    with the same arguments), and afterwards the module's current blob is bound again: a plain forward has the second forward's bits;
  - a module moved off the device between forward and backward is refused before anything is launched."""
import pytest
import torch

from tests.test_hifigan_disc_autograd_gpu import _module as _period_module
from tests.test_hifigan_msd_autograd_gpu import _module as _scale_module
from tests.test_melgan_disc_gpu import DEV, _module as _melgan_module

pytestmark = pytest.mark.gpu

MAKE = {"melgan": lambda: _melgan_module("TINY")[2], "period": lambda: _period_module("TINY")[2],
        "scale": lambda: _scale_module("TINY", spectral=(0,))[2]}
LENS = (90, 61)


def _wav(model):
    assert model.min_samples <= min(LENS)
    return torch.randn(len(LENS), max(LENS), generator=torch.Generator().manual_seed(5)).to(DEV)


def _loss(maps):
    return sum((m * m).sum() for sub in maps for m in sub)


def _same(a, b):
    return all(torch.equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


@pytest.mark.parametrize("kind", sorted(MAKE))
def test_a_node_differentiates_the_weights_it_ran_on(kind):
    model, twin = MAKE[kind]().eval(), MAKE[kind]().eval()
    twin.load_state_dict(model.state_dict())   # the spectral buffers start at random: the twin takes the model's
    x, y = _wav(model).requires_grad_(True), _wav(twin).requires_grad_(True)
    first = model(x, LENS)
    kept = [[m.detach().clone() for m in sub] for sub in first]
    p = [q for k, q in model.named_parameters() if k.endswith(".weight")][-1]
    p.data = p.data.clone() * 2.0              # another tensor under the parameter, other weights: no version changes
    with torch.no_grad():
        second = model(x.detach(), LENS)       # packs again, into a new blob
    assert not _same(second, kept), "the second forward did not see the changed weight"
    _loss(first).backward()
    want = twin(y, LENS)
    assert _same(want, kept)
    _loss(want).backward()
    assert torch.equal(x.grad, y.grad)
    for (k, a), b in zip(model.named_parameters(), twin.parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), k
    with torch.no_grad():
        assert _same(model(x.detach(), LENS), second), "the module's current blob was not bound back after the backward"


@pytest.mark.parametrize("kind", sorted(MAKE))
def test_a_moved_module_is_refused(kind):
    model = MAKE[kind]().eval()
    out = model(_wav(model).requires_grad_(True), LENS)
    model.to("cpu")
    with pytest.raises(RuntimeError, match="moved"):
        _loss(out).backward()
    assert model._train_workspace is None   # the backward got as far as no scratch, let alone a launch
