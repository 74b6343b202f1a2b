"""GPU: HiFiGANPeriodDiscriminator's autograd node against the C-ABI calls it wraps (tests/test_hifigan_disc_gpu.py holds those to
float64): the same bits under no_grad and with grad, .grad of the parameters and of wav, the parameters-off path, torch's version error
for in-place edits of a map or a parameter between forward and backward, and re-packing after an optimizer step."""
import pytest
import torch

from genvox_amd.configs import HiFiGANPeriodDiscriminatorConfig
from genvox_amd.hifigan_disc import HiFiGANPeriodDiscriminator
from tests import hifigan_disc_ref64 as DR
from tests.test_hifigan_disc_gpu import DEV, _net, _poisoned

pytestmark = pytest.mark.gpu


def _module(name):
    cfg, sd, net = _net(name)
    model = HiFiGANPeriodDiscriminator(HiFiGANPeriodDiscriminatorConfig(periods=cfg["periods"], channels=cfg["channels"], kernel_size=cfg["kernel_size"],
                                                                         stride=cfg["stride"], leaky_slope=cfg["slope"]))
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    return cfg, net, model.to(DEV)


def test_module_gradients_are_the_c_abi_calls_bits():
    cfg, net, model = _module("MIXED")
    lens = (261, 5, 135)
    n_maps = len(cfg["channels"]) + 1
    wav = _poisoned(DR.random_wav(3, 261, 3), lens)
    G = DR.random_cotangents(cfg, 3, 261, 8)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav, lens_d)
    want = net.backward(wav, lens_d, feats, net.cotangent_buffer(G, 3, 261, lens))
    x = wav.clone().requires_grad_(True)
    out = model(x, lens)
    assert len(out) == len(cfg["periods"]) and all(len(o) == n_maps for o in out)
    assert model.map_lengths(lens) == [[[DR.map_heights(cfg, nb)[j][i] for nb in lens] for i in range(n_maps)] for j in range(len(cfg["periods"]))]
    loss = 0.0
    for j, period in enumerate(out):
        for i, m in enumerate(period):
            assert m.shape == (3, DR.layer_shapes(cfg)[i][1], DR.map_heights(cfg, 261)[j][i], cfg["periods"][j])
            assert torch.equal(m, maps[j][i]), f"the module's map ({j}, {i}) is not the C-ABI call's"
            g = torch.zeros(m.shape, device=DEV)
            for b, nb in enumerate(lens):
                H = DR.map_heights(cfg, nb)[j][i]
                g[b, :, :H] = G[j][i][b, :, :H].to(DEV, torch.float32)
            loss = loss + (m * g).sum()
    loss.backward()
    assert torch.equal(x.grad, want["wav"])
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, want[k]), k
    # under no_grad, and when nothing asks for a gradient: the plain forward's bits
    with torch.no_grad():
        plain = model(wav, lens)
    for p in model.parameters():
        p.requires_grad_(False)
        p.grad = None
    frozen = model(wav, lens)
    for j in range(len(cfg["periods"])):
        for i in range(n_maps):
            assert torch.equal(plain[j][i], maps[j][i]) and not plain[j][i].requires_grad and torch.equal(frozen[j][i], maps[j][i])
    # the generator's step: wav alone asks for a gradient; cotangents that never arrive count as zero (scores only)
    x2 = wav.clone().requires_grad_(True)
    scores_only = sum(period[-1][b, :, :DR.map_heights(cfg, nb)[j][-1]].sum() for j, period in enumerate(model(x2, lens)) for b, nb in enumerate(lens))
    scores_only.backward()
    ones = [[None if i < n_maps - 1 else torch.ones_like(g) for i, g in enumerate(gs)] for gs in G]
    want2 = net.backward(wav, lens_d, feats, net.cotangent_buffer(ones, 3, 261, lens), want_params=False)
    assert torch.equal(x2.grad, want2["wav"])
    assert all(p.grad is None and not p.requires_grad for p in model.parameters()), "the parameters-off path computed a parameter gradient"


def test_module_refuses_short_rows_and_in_place_changes_and_packs_again():
    cfg, net, model = _module("TINY")
    wav = DR.random_wav(2, 40, 1).to(DEV, torch.float32)
    with pytest.raises(ValueError, match="row 1"):
        model(wav, [40, 2])
    with pytest.raises(ValueError):
        model(wav[:, :2])
    out = model(wav)
    with torch.no_grad():
        model.discriminators[0].convs[1].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[0][-1].sum().backward()
    # a parameter that changed is packed again: the next forward sees it
    after = model(wav)
    assert not torch.equal(after[0][-1], out[0][-1]) and torch.equal(after[1][0], out[1][0])
    # the returned maps are the backward's tape: one changed in place raises too, whichever map the loss hangs on
    again = model(wav)
    with pytest.raises(RuntimeError, match="inplace"):   # torch refuses at the operation or, at the latest, at the backward
        again[1][-1].clamp_(min=0.0)
        again[0][0].sum().backward()
    # an optimizer step changes every parameter in place: the blob is rebuilt, and the maps are those of a fresh module on the new weights
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    model(wav)[0][-1].sum().backward()
    opt.step()
    stepped = model(wav)
    fresh = HiFiGANPeriodDiscriminator(model.model_config)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(DEV)
    with torch.no_grad():
        want = fresh(wav)
    assert not torch.equal(stepped[0][-1], after[0][-1])
    for j in range(len(cfg["periods"])):
        for a, b in zip(stepped[j], want[j]):
            assert torch.equal(a, b)
