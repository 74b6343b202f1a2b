"""GPU: HiFiGANScaleDiscriminator's autograd node against the C-ABI calls it wraps (tests/test_hifigan_msd_gpu.py holds those to
float64): the same bits under no_grad and with grad, .grad of the parameters and of wav, the parameters-off path; with a spectral scale
in training mode the weight_orig gradients (through sigma) and the updated u and v against float64 autograd of the restatement; eval
mode leaves u and v alone; two forwards before one backward (the GAN step's pattern) each keep the weights they ran on; torch's version
error for in-place edits of a map or a parameter between forward and backward; re-packing after .to(), a reload and an optimizer step.

Tolerance of the spectral test: the project's rule - per tensor, e is the largest |float32 restatement - float64|, and the device may
differ from float64 by at most 8 x max(e, 2^-23 x the tensor's largest value)."""
import pytest
import torch

from genvox_amd.configs import HiFiGANScaleDiscriminatorConfig
from genvox_amd.hifigan_msd import HiFiGANScaleDiscriminator
from tests import hifigan_msd_ref64 as SR
from tests.test_hifigan_msd_gpu import DEV, DiscNet, _net, _poisoned

pytestmark = pytest.mark.gpu


def _config(cfg, spectral):
    return HiFiGANScaleDiscriminatorConfig(n_scales=cfg["n_scales"], channels=cfg["channels"], kernel_sizes=cfg["kernel_sizes"], strides=cfg["strides"],
                                           groups=cfg["groups"], spectral_norm_scales=spectral, leaky_slope=cfg["slope"])


def _module(name, spectral=()):
    cfg, sd, net = _net(name)
    model = HiFiGANScaleDiscriminator(_config(cfg, spectral))
    model.load_state_dict({k: v.float() for k, v in sd.items()})   # a plain weight becomes a spectral scale's weight_orig
    return cfg, net, model.to(DEV)


def _cotangents_on(cfg, G, lens, n, dtype, device):
    """G cut to every row's own lengths, zeros behind."""
    out = []
    for s, gs in enumerate(G):
        row = []
        for i, g in enumerate(gs):
            z = torch.zeros(g.shape, dtype=dtype, device=device)
            for b, nb in enumerate(lens):
                L = SR.map_lengths(cfg, nb)[s][i]
                z[b, :, :L] = g[b, :, :L].to(device, dtype)
            row.append(z)
        out.append(row)
    return out


def test_module_gradients_are_the_c_abi_calls_bits():
    cfg, net, model = _module("MIXED")
    lens = (261, 1, 135)
    n_maps = len(cfg["channels"]) + 1
    wav = _poisoned(SR.random_wav(3, 261, 3), lens)
    G = SR.random_cotangents(cfg, 3, 261, 8)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav, lens_d)
    want = net.backward(wav, lens_d, feats, net.cotangent_buffer(G, 3, 261, lens))
    x = wav.clone().requires_grad_(True)
    out = model(x, lens)
    assert len(out) == cfg["n_scales"] and all(len(o) == n_maps for o in out)
    assert model.map_lengths(lens) == [[[SR.map_lengths(cfg, nb)[s][i] for nb in lens] for i in range(n_maps)] for s in range(cfg["n_scales"])]
    Gd = _cotangents_on(cfg, G, lens, 261, torch.float32, DEV)
    loss = 0.0
    for s, scale in enumerate(out):
        for i, m in enumerate(scale):
            assert m.shape == (3, SR.layer_shapes(cfg)[i][1], SR.map_lengths(cfg, 261)[s][i])
            assert torch.equal(m, maps[s][i]), f"the module's map ({s}, {i}) is not the C-ABI call's"
            loss = loss + (m * Gd[s][i]).sum()
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
    for s in range(cfg["n_scales"]):
        for i in range(n_maps):
            assert torch.equal(plain[s][i], maps[s][i]) and not plain[s][i].requires_grad and torch.equal(frozen[s][i], maps[s][i])
    # the generator's step: wav alone asks for a gradient; cotangents that never arrive count as zero (scores only)
    x2 = wav.clone().requires_grad_(True)
    scores_only = sum(scale[-1][b, :, :SR.map_lengths(cfg, nb)[s][-1]].sum() for s, scale in enumerate(model(x2, lens)) for b, nb in enumerate(lens))
    scores_only.backward()
    ones = [[None if i < n_maps - 1 else torch.ones_like(g) for i, g in enumerate(gs)] for gs in G]
    want2 = net.backward(wav, lens_d, feats, net.cotangent_buffer(ones, 3, 261, lens), want_params=False)
    assert torch.equal(x2.grad, want2["wav"])
    assert all(p.grad is None and not p.requires_grad for p in model.parameters()), "the parameters-off path computed a parameter gradient"


def _restated_step(cfg, state, wav, lens, G, masks, dtype):
    """The training-mode forward and backward of a module whose scale 0 is spectral, restated on the CPU in ``dtype``: one power iteration
    outside the graph, sigma inside it, every row alone.  -> ({key: gradient}, {key: updated u or v})."""
    leaves = {k: v.to(dtype).clone().requires_grad_(k.endswith(("weight_orig", "weight", "bias"))) for k, v in state.items()}
    sd, buffers = {}, {}
    for k, v in leaves.items():
        if k.endswith("weight_orig"):
            prefix = k[:-len(".weight_orig")]
            w, u, vv = SR.spectral_weight(v, leaves[prefix + ".weight_u"], leaves[prefix + ".weight_v"], training=True)
            sd[prefix + ".weight"], buffers[prefix + ".weight_u"], buffers[prefix + ".weight_v"] = w, u, vv
        elif k.endswith((".weight", ".bias")):
            sd[k] = v
    x = wav.to(dtype).clone().requires_grad_(True)
    loss = 0.0
    for b, nb in enumerate(lens):
        own = SR.map_lengths(cfg, nb)
        mk = [[m[b:b + 1, :, :own[s][i]].to(dtype) for i, m in enumerate(ms)] for s, ms in enumerate(masks)]
        for s, ms in enumerate(SR.discriminator(sd, x[b:b + 1, :nb], cfg, mk)):
            for i, m in enumerate(ms):
                loss = loss + (m * G[s][i][b:b + 1, :, :m.shape[2]].to(dtype)).sum()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items() if v.requires_grad}
    grads["wav"] = x.grad
    return grads, buffers


def test_spectral_scale_in_training_mode_against_float64():
    cfg, _, model = _module("TINY", spectral=(0,))
    assert "discriminators.0.convs.1.weight_orig" in dict(model.named_parameters()) and "discriminators.1.convs.1.weight" in dict(model.named_parameters())
    lens = (150, 1, 77)
    wav64 = SR.random_wav(3, 150, 4)
    for b, nb in enumerate(lens):
        wav64[b, nb:] = 0.0
    G = SR.random_cotangents(cfg, 3, 150, 6)
    state = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items()}
    model.train()
    x = _poisoned(wav64, lens).requires_grad_(True)
    out = model(x, lens)
    # the maps are the C-ABI call's on the effective weights of the updated u and v
    model.eval()
    with torch.no_grad():
        eff = {k: v.detach().clone() for k, v in zip(model.weight_names(), model.effective_weights())}
    model.train()
    net = DiscNet(cfg, eff)
    _, maps = net.forward(x.detach(), torch.tensor(lens, dtype=torch.int32, device=DEV))
    Gd = _cotangents_on(cfg, G, lens, 150, torch.float32, DEV)
    loss = 0.0
    for s, scale in enumerate(out):
        for i, m in enumerate(scale):
            assert torch.equal(m, maps[s][i]), f"map ({s}, {i}) is not the C-ABI call's on weight_orig / sigma"
            loss = loss + (m * Gd[s][i]).sum()
    loss.backward()
    masks = SR.masks_from_maps(maps, cfg["slope"])
    g64, b64 = _restated_step(cfg, state, wav64, lens, G, masks, torch.float64)
    g32, b32 = _restated_step(cfg, state, wav64, lens, G, masks, torch.float32)
    got = {k: p.grad for k, p in model.named_parameters()}
    got["wav"] = x.grad
    assert set(got) == set(g64)
    worst = 0.0
    for k, want in list(g64.items()) + list(b64.items()):
        have = (got[k] if k in got else dict(model.named_buffers())[k]).double().cpu()
        e, tol = SR.tol_of((g32[k] if k in g32 else b32[k]), want)
        d = (have - want).abs().max().item()
        print(f"  {k}: {d:.3e} of {tol:.3e}")
        assert not torch.isnan(have).any() and d <= tol, f"{k}: {d:.3e} from float64, above the bound {tol:.3e} (float32 restatement {e:.3e})"
        worst = max(worst, d / tol)
    print(f"spectral scale, training mode: largest error {worst:.3f} of its bound")
    for b, nb in enumerate(lens):
        assert not x.grad[b, nb:].any()
    # u and v did move, and eval mode leaves them alone
    assert not torch.equal(model.discriminators[0].convs[1].weight_u.cpu().double(), state["discriminators.0.convs.1.weight_u"])
    model.eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    with torch.no_grad():
        first = model(x.detach(), lens)
    second = model(x.detach().requires_grad_(True), lens)
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    assert all(torch.equal(a, b) for sa, sb in zip(first, second) for a, b in zip(sa, sb))


def test_two_forwards_before_one_backward_keep_their_own_weights():
    """The discriminators' step runs D(real) and D(fake) and then one backward: in training mode the second forward's power iteration
    changes the effective weights, and the first node must still differentiate the weights it ran on."""
    cfg, _, model = _module("TINY", spectral=(0,))
    start = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    a, b = SR.random_wav(2, 90, 1).to(DEV, torch.float32), SR.random_wav(2, 90, 2).to(DEV, torch.float32)
    model.train()
    xa, xb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    oa = model(xa)
    ob = model(xb)
    (sum(m.sum() for s in oa for m in s) + sum((m * m).sum() for s in ob for m in s)).backward()
    other = HiFiGANScaleDiscriminator(model.model_config)
    other.load_state_dict(start)
    other = other.to(DEV).train()
    ya, yb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    sum(m.sum() for s in other(ya) for m in s).backward()
    sum((m * m).sum() for s in other(yb) for m in s).backward()
    assert torch.equal(xa.grad, ya.grad) and torch.equal(xb.grad, yb.grad)
    for (k, p), q in zip(model.named_parameters(), other.parameters()):   # the same terms, added in autograd's order: not bit for bit
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-5, atol=1e-5 * q.grad.abs().max().item(), msg=k)
    for (k, p), q in zip(model.named_buffers(), other.buffers()):
        assert torch.equal(p, q), k


def test_module_refuses_bad_rows_and_in_place_changes_and_packs_again():
    cfg, net, model = _module("TINY", spectral=(0,))
    model.eval()
    wav = SR.random_wav(2, 40, 1).to(DEV, torch.float32)
    with pytest.raises(ValueError, match="row 1"):
        model(wav, [40, 0])
    with pytest.raises(ValueError, match="row 0"):
        model(wav, [41, 3])
    with pytest.raises(ValueError):
        model(wav[:, :0])
    out = model(wav)
    with torch.no_grad():
        model.discriminators[1].convs[1].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[1][-1].sum().backward()
    # a parameter that changed is packed again: the next forward sees it
    after = model(wav)
    assert not torch.equal(after[1][-1], out[1][-1]) and torch.equal(after[0][-1], out[0][-1]) and torch.equal(after[1][0], out[1][0])
    with torch.no_grad():
        model.discriminators[0].convs[1].weight_orig.mul_(2.0)   # behind sigma: the effective weight is its function
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        after[0][-1].sum().backward()
    # the returned maps are the backward's tape: one changed in place raises too, whichever map the loss hangs on
    again = model(wav)
    with pytest.raises(RuntimeError, match="inplace"):   # torch refuses at the operation or, at the latest, at the backward
        again[1][-1].clamp_(min=0.0)
        again[0][0].sum().backward()
    # .to() moves every tensor: packed again, the same bits
    with torch.no_grad():
        here = model(wav)
        model.to("cpu")
        with pytest.raises(RuntimeError, match="MI355X"):
            model(wav)
        model.to(DEV)
        moved = model(wav)
    assert all(torch.equal(x, y) for sx, sy in zip(here, moved) for x, y in zip(sx, sy))
    # an optimizer step changes every parameter in place, a reload replaces them: the blob is rebuilt each time
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    sum(s[-1].sum() for s in model(wav)).backward()
    opt.step()
    stepped = model(wav)
    fresh = HiFiGANScaleDiscriminator(model.model_config)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        want = fresh(wav)
    assert not torch.equal(stepped[0][-1], moved[0][-1]) and not torch.equal(stepped[1][-1], moved[1][-1])
    assert all(torch.equal(x, y) for sx, sy in zip(stepped, want) for x, y in zip(sx, sy))
    _, sd, _ = _net("TINY")
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    with torch.no_grad():
        reloaded = model(wav)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = fresh(wav)
    assert all(torch.equal(x, y) for sx, sy in zip(reloaded, want) for x, y in zip(sx, sy))
