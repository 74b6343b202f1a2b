"""CPU: the host side of the MelGAN discriminator - symbols, config refusals, the layout's arithmetic against lengths worked by hand,
parameter counts, the restatement against an independently built nn.Sequential stack (through the published key names and weight
normalisation), the two GAN losses against values worked by hand, and the C ABI's refusals before any pointer is looked at.  No GPU call."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

from genvox_amd import _lib, build
from genvox_amd.configs import MelGANDiscriminatorConfig
from genvox_amd.losses import MelGANDiscriminatorLoss, MelGANGeneratorLoss
from genvox_amd.melgan_disc import MelGANDiscriminator, dims_from_config, map_published_keys
from tests import melgan_disc_ref64 as DR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gvx_melgan_disc_blob_floats", "gvx_melgan_disc_pack_weights_device", "gvx_melgan_disc_create", "gvx_melgan_disc_destroy",
       "gvx_melgan_disc_bind", "gvx_melgan_disc_layout", "gvx_melgan_disc_features_bytes", "gvx_melgan_disc_workspace_bytes",
       "gvx_melgan_disc_forward", "gvx_melgan_disc_backward")


def _config(cfg) -> MelGANDiscriminatorConfig:
    return MelGANDiscriminatorConfig(n_scales=cfg["n_scales"], base_channels=cfg["base_channels"], n_layers=cfg["n_layers"],
                                     downsampling_factor=cfg["s"], max_channels=cfg["max_channels"], leaky_slope=cfg["slope"])


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    declared = set(re.findall(r"\b(gvx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "melgan_disc.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "melgan_disc.hip"))
    import genvox_amd
    assert genvox_amd.MelGANDiscriminator is MelGANDiscriminator and genvox_amd.MelGANDiscriminatorConfig is MelGANDiscriminatorConfig
    assert genvox_amd.MelGANTrainer.__name__ == "MelGANTrainer" and genvox_amd.MelGANGeneratorLoss is MelGANGeneratorLoss


@pytest.mark.parametrize("bad", [dict(n_scales=0), dict(n_scales=5), dict(base_channels=6), dict(base_channels=0), dict(n_layers=0), dict(n_layers=7),
                                 dict(downsampling_factor=0), dict(downsampling_factor=9), dict(leaky_slope=1.5), dict(base_channels=16.0),
                                 dict(base_channels=32, downsampling_factor=2, max_channels=36),    # 36 channels in 8 groups
                                 dict(base_channels=8, downsampling_factor=4, max_channels=30, n_layers=2)])   # layer 2's input 30 is no multiple of 4
def test_config_refusals(bad):
    with pytest.raises(ValueError):
        MelGANDiscriminatorConfig(**bad)
    d = dims_from_config(MelGANDiscriminatorConfig())
    for k, v in bad.items():
        setattr(d, {"leaky_slope": "slope"}.get(k, k), v if k == "leaky_slope" else int(v))
    if bad != dict(base_channels=16.0):   # the C side sees an integer there
        h = C.c_void_p()
        assert _lib.load().gvx_melgan_disc_create(C.byref(d), C.byref(h)) == -1
        assert _lib.load().gvx_melgan_disc_blob_floats(C.byref(d)) == 0


def test_default_parameter_counts():
    """By hand, one scale of the default shape (weights + biases):
    layer 0  1 -> 16, k 15:                   16 * 1 * 15 + 16        =       256
    layer 1  16 -> 64, k 41, 4 groups:        64 * 4 * 41 + 64        =    10,560
    layer 2  64 -> 256, 16 groups:            256 * 4 * 41 + 256      =    42,240
    layer 3  256 -> 1024, 64 groups:          1024 * 4 * 41 + 1024    =   168,960
    layer 4  1024 -> 1024 (capped), 256 gr.:  1024 * 4 * 41 + 1024    =   168,960
    layer 5  1024 -> 1024, k 5, dense:        1024 * 1024 * 5 + 1024  = 5,243,904
    score    1024 -> 1, k 3:                  1024 * 3 + 1            =     3,073"""
    per_scale = 256 + 10560 + 42240 + 168960 + 168960 + 5243904 + 3073
    assert per_scale == 5637953
    cfg = MelGANDiscriminatorConfig()
    assert cfg.parameter_count() == 3 * per_scale == 16913859
    model = MelGANDiscriminator(cfg)
    assert sum(p.numel() for p in model.parameters()) == 16913859
    assert sum(p.numel() for p in model.scales[1].parameters()) == per_scale
    assert [tuple(l.weight.shape) for l in model.scales[0].layers] == [(16, 1, 15), (64, 4, 41), (256, 4, 41), (1024, 4, 41), (1024, 4, 41), (1024, 1024, 5), (1, 1024, 3)]
    blob = _lib.load().gvx_melgan_disc_blob_floats(C.byref(model.dims()))
    assert blob >= 16913859 and blob % 64 == 0 and blob < 16913859 + 3 * 14 * 64   # every tensor rounded up to 64 floats


# Default shape, s = 4: a scale sees n >> k samples; layer 0 keeps the length, layers 1 .. 4 each take L -> (L - 1) // 4 + 1, the k = 5
# layer and the score keep it.  Worked by hand:
HAND = {
    32: [[32, 8, 2, 1, 1, 1, 1], [16, 4, 1, 1, 1, 1, 1], [8, 2, 1, 1, 1, 1, 1]],
    33: [[33, 9, 3, 1, 1, 1, 1], [16, 4, 1, 1, 1, 1, 1], [8, 2, 1, 1, 1, 1, 1]],     # pooled: 33 // 2 = 16, 16 // 2 = 8
    35: [[35, 9, 3, 1, 1, 1, 1], [17, 5, 2, 1, 1, 1, 1], [8, 2, 1, 1, 1, 1, 1]],     # 35 // 2 = 17, 17 // 2 = 8
    36: [[36, 9, 3, 1, 1, 1, 1], [18, 5, 2, 1, 1, 1, 1], [9, 3, 1, 1, 1, 1, 1]],     # 36 // 2 = 18, 18 // 2 = 9
}
CHANNELS = [16, 64, 256, 1024, 1024, 1024, 1]


@pytest.mark.parametrize("n", sorted(HAND))
def test_layout_and_feature_lengths_by_hand(n):
    model = MelGANDiscriminator()
    assert model.feature_lengths(n) == HAND[n] == DR.map_lengths(DR.DEFAULT, n)
    for B in (1, 3):
        lay = model.layout(B, n)
        assert [[(c, L) for _, c, L in scale] for scale in lay] == [list(zip(CHANNELS, lens)) for lens in HAND[n]]
        at = 0
        for scale in lay:
            for off, c, L in scale:
                assert off == at and off % 256 == 0
                at += (4 * B * c * L + 255) // 256 * 256
        d = model.dims()
        lib = _lib.load()
        assert lib.gvx_melgan_disc_features_bytes(C.byref(d), B, n) == at
        fw, bw = lib.gvx_melgan_disc_workspace_bytes(C.byref(d), B, n, 0), lib.gvx_melgan_disc_workspace_bytes(C.byref(d), B, n, 1)
        assert fw == sum((4 * B * (n >> k) + 255) // 256 * 256 for k in (1, 2)) and bw > fw and bw % 256 == 0
        assert lib.gvx_melgan_disc_layout(C.byref(d), B, n, None, 0) == 21
    assert model.map_lengths([n, 32])[1][1] == [HAND[n][1][1], 4]


def test_size_calls_return_zero_for_refused_shapes():
    lib, d = _lib.load(), dims_from_config(MelGANDiscriminatorConfig())
    for B, n in ((1, 31), (0, 64), (65536, 64), (1, (1 << 24) + 1)):
        assert lib.gvx_melgan_disc_features_bytes(C.byref(d), B, n) == 0
        assert lib.gvx_melgan_disc_workspace_bytes(C.byref(d), B, n, 1) == 0
        assert lib.gvx_melgan_disc_layout(C.byref(d), B, n, None, 0) == 0
    assert lib.gvx_melgan_disc_features_bytes(C.byref(d), 1, 32) > 0
    with pytest.raises(ValueError):
        MelGANDiscriminator().layout(1, 31)


class _Published(nn.Module):
    """The published implementation's module tree, built independently of the restatement: NLayerDiscriminator's ``model`` dict of
    ``layer_<i>`` Sequentials under ``model.discriminator_<k>``, weight-normalised convolutions, AvgPool1d between the scales."""

    def __init__(self, cfg):
        super().__init__()
        wn = nn.utils.weight_norm
        self.model = nn.ModuleDict()
        s, c = cfg["s"], cfg["base_channels"]
        for k in range(cfg["n_scales"]):
            layers = nn.ModuleDict()
            layers["layer_0"] = nn.Sequential(nn.ReflectionPad1d(7), wn(nn.Conv1d(1, c, kernel_size=15)), nn.LeakyReLU(cfg["slope"]))
            nf = c
            for i in range(1, cfg["n_layers"] + 1):
                prev, nf = nf, min(nf * s, cfg["max_channels"])
                layers[f"layer_{i}"] = nn.Sequential(wn(nn.Conv1d(prev, nf, kernel_size=10 * s + 1, stride=s, padding=5 * s, groups=prev // 4)),
                                                     nn.LeakyReLU(cfg["slope"]))
            nf2 = min(nf * 2, cfg["max_channels"])
            layers[f"layer_{cfg['n_layers'] + 1}"] = nn.Sequential(wn(nn.Conv1d(nf, nf2, kernel_size=5, padding=2)), nn.LeakyReLU(cfg["slope"]))
            layers[f"layer_{cfg['n_layers'] + 2}"] = nn.Sequential(wn(nn.Conv1d(nf2, 1, kernel_size=3, padding=1)))
            holder = nn.Module()
            holder.model = layers
            self.model[f"discriminator_{k}"] = holder
        self.pool = nn.AvgPool1d(4, stride=2, padding=1, count_include_pad=False)
        self.n_scales, self.n_maps = cfg["n_scales"], cfg["n_layers"] + 3

    def forward(self, x):
        out = []
        for k in range(self.n_scales):
            maps, h = [], x
            for i in range(self.n_maps):
                h = self.model[f"discriminator_{k}"].model[f"layer_{i}"](h)
                maps.append(h)
            out.append(maps)
            x = self.pool(x)
        return out


@pytest.mark.parametrize("cfg", [DR.TINY, DR.MIXED], ids=["TINY", "MIXED"])
def test_restatement_equals_an_independent_sequential_stack(cfg):
    """Through the published key names and the weight-norm fold: the module's load_state_dict reads the stack's state dict, and the
    restatement on the folded weights gives the stack's maps to float64 rounding, at an odd and an even length."""
    torch.manual_seed(5)
    stack = _Published(cfg).double()
    for p in stack.parameters():
        p.data.normal_(0.0, 0.3)
    sd = stack.state_dict()
    assert any(k.startswith("model.discriminator_0.model.layer_0.1.") for k in sd) and any(k.startswith("model.discriminator_1.model.layer_1.0.") for k in sd)
    model = MelGANDiscriminator(_config(cfg)).double()
    model.load_state_dict(sd)
    folded = {k: v.detach() for k, v in model.state_dict().items()}
    assert set(folded) == set(DR.param_names(cfg))
    for n in (DR.min_samples(cfg), 67, 70):
        wav = DR.random_wav(2, n, 3)
        with torch.no_grad():
            want = stack(wav[:, None, :])
        got = DR.discriminator(folded, wav, cfg)
        assert [[m.shape[2] for m in ms] for ms in got] == DR.map_lengths(cfg, n)
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                torch.testing.assert_close(x, y, rtol=1e-12, atol=1e-13)
    with pytest.raises(KeyError):
        map_published_keys({"model.discriminator_0.model.layer_0.0.bias": torch.zeros(1)})


def test_pinned_restatement_and_ragged_rows():
    """Pinning to its own decisions changes nothing beyond float64 rounding; ragged rows are the rows alone, summed; nothing behind a
    row's length matters (NaN there)."""
    cfg = DR.TINY
    sd = DR.random_state(cfg, 7)
    wav = DR.random_wav(2, 37, 2)
    G = DR.random_cotangents(cfg, 2, 37, 9)
    free = DR.reference(sd, wav, None, cfg, G)
    pinned = DR.reference(sd, wav, None, cfg, G, DR.masks_from_maps(free["maps"], cfg["slope"]))
    for k in free["grads"]:
        torch.testing.assert_close(pinned["grads"][k], free["grads"][k], rtol=1e-12, atol=1e-14)
    lens = (37, 21)
    poisoned = wav.clone()
    poisoned[1, 21:] = float("nan")
    rag = DR.reference(sd, poisoned, lens, cfg, G)
    alone = [DR.reference(sd, wav[b:b + 1, :n], None, cfg, [[g[b:b + 1] for g in gs] for gs in G]) for b, n in enumerate(lens)]
    for k in sd:
        torch.testing.assert_close(rag["grads"][k], alone[0]["grads"][k] + alone[1]["grads"][k], rtol=1e-12, atol=1e-14)
    assert not rag["grads"]["wav"][1, 21:].any() and torch.equal(rag["grads"]["wav"][1, :21], alone[1]["grads"]["wav"][0])
    own = DR.map_lengths(cfg, 21)
    for k, ms in enumerate(rag["maps"]):
        for i, m in enumerate(ms):
            assert not m[1, :, own[k][i]:].any() and not torch.isnan(m).any()


def test_losses_by_hand():
    """One scale of three maps (two features and the score), B = 2.
    Scores, uniform (3 positions):  real [[.5, 2, -1], [0, 3, 1]], fake [[-2, 0, 1], [-.5, 1, -3]].
      hinge: relu(1 - real) = [.5, 0, 2], [1, 0, 0]: row means 2.5 / 3 and 1 / 3, their mean 3.5 / 6;
             relu(1 + fake) = [0, 1, 2], [.5, 2, 0]: row means 1 and 2.5 / 3, their mean 5.5 / 6;        d = 9 / 6 = 1.5
      adversarial: -mean(fake): rows -1 / 3 and -2.5 / 3 -> +(1 / 3 + 2.5 / 3) / 2 = 3.5 / 6
    Ragged, lengths of the score (3, 2): row 1 counts its first two positions only.
      hinge: real row 1 [1, 0] -> .5, fake row 1 [.5, 2] -> 1.25:  (2.5 / 3 + .5) / 2 + (1 + 1.25) / 2 = 2 / 3 + 1.125
      adversarial: fake row 1 mean .25: -(-1 / 3 + .25) / 2 = 1 / 24
    Features: map 0 [2, 1, 2]: |fake - real| = [[1, 3]], [[2, 4]];  map 1 [2, 2, 1]: [[1], [3]], [[5], [7]].  n_layers + 1 = 1 and one scale:
      weight 4.  Uniform: map 0 rows 2 and 3 -> 2.5, map 1 rows 2 and 6 -> 4:  feat_match * 4 * 6.5 = 260 at feat_match = 10.
      Ragged, map 0 lengths (2, 1): rows 2 and 2 -> 2; map 1 lengths (1, 1): 4:  10 * 4 * 6 = 240."""
    nan = float("nan")
    real_s = torch.tensor([[[.5, 2., -1.]], [[0., 3., 1.]]])
    fake_s = torch.tensor([[[-2., 0., 1.]], [[-.5, 1., -3.]]])
    r0, r1 = torch.zeros(2, 1, 2), torch.ones(2, 2, 1)
    f0 = torch.tensor([[[1., -3.]], [[2., 4.]]])
    f1 = torch.tensor([[[2.], [4.]], [[-4.], [8.]]])
    real, fake = [[r0, r1, real_s]], [[f0, f1, fake_s]]
    d_loss, g_loss = MelGANDiscriminatorLoss(), MelGANGeneratorLoss(10.0)
    torch.testing.assert_close(d_loss(real, fake), torch.tensor(1.5))
    torch.testing.assert_close(g_loss(real, fake), torch.tensor(3.5 / 6 + 260.0))
    torch.testing.assert_close(g_loss.last_terms[0], torch.tensor(3.5 / 6))
    torch.testing.assert_close(g_loss.last_terms[1], torch.tensor(260.0))
    # ragged: whatever lies behind a row's length - NaN here - never enters
    lengths = [[[2, 1], [1, 1], [3, 2]]]
    real_s[1, 0, 2] = fake_s[1, 0, 2] = nan
    f0[1, 0, 1] = nan
    assert torch.isnan(d_loss(real, fake)) and torch.isnan(g_loss(real, fake))   # without the lengths the NaN is part of the rows
    torch.testing.assert_close(d_loss(real, fake, lengths), torch.tensor(2.0 / 3 + 1.125))
    torch.testing.assert_close(g_loss(real, fake, lengths), torch.tensor(1.0 / 24 + 240.0))
    # the real features are detached: only the fake side gets a gradient
    r0.requires_grad_(True)
    f0g = f0.clone().requires_grad_(True)
    g_loss([[r0, r1, real_s]], [[f0g, f1, fake_s]], lengths).backward()
    assert r0.grad is None and f0g.grad is not None and f0g.grad[1, 0, 1] == 0


def test_calls_refuse_on_the_host():
    """Bad B and n_max, NULL arguments, no blob, short or misaligned buffers, missing gradient names: all refused before the (bogus)
    pointers are looked at.  A call that got past its checks would launch on made-up addresses."""
    lib, d = _lib.load(), dims_from_config(_config(DR.TINY))
    h = C.c_void_p()
    assert lib.gvx_melgan_disc_create(C.byref(d), C.byref(h)) == 0
    P = 1 << 20
    fb, fw, bw = (lib.gvx_melgan_disc_features_bytes(C.byref(d), 2, 40), lib.gvx_melgan_disc_workspace_bytes(C.byref(d), 2, 40, 0),
                  lib.gvx_melgan_disc_workspace_bytes(C.byref(d), 2, 40, 1))
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 40, P, fb, P, fw, None) == -7          # no blob bound
    assert lib.gvx_melgan_disc_bind(h, 4) == -1 and lib.gvx_melgan_disc_bind(h, None) == -1
    assert lib.gvx_melgan_disc_bind(h, 256) == 0
    assert lib.gvx_melgan_disc_forward(None, P, None, 2, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_melgan_disc_forward(h, None, None, 2, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 40, None, fb, P, fw, None) == -1
    assert lib.gvx_melgan_disc_forward(h, P, None, 0, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_melgan_disc_forward(h, P, None, 65536, 40, P, 1 << 40, P, 1 << 40, None) == -1
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 15, P, fb, P, fw, None) == -1          # TINY has 2 scales: 16 samples at least
    assert b"reflection" in lib.gvx_last_error()
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, (1 << 24) + 1, P, 1 << 40, P, 1 << 40, None) == -2
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 40, P, fb - 1, P, fw, None) == -5
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 40, P + 4, fb, P, fw, None) == -5
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 40, P, fb, None, fw, None) == -5
    assert lib.gvx_melgan_disc_forward(h, P, None, 2, 40, P, fb, P, fw - 1, None) == -5
    names = DR.param_names(DR.TINY)
    shapes = {k: v.numel() for k, v in DR.random_state(DR.TINY, 1).items()}
    table = (_lib.gvx_weight_desc * len(names))(*[_lib.gvx_weight_desc(k.encode(), P, shapes[k]) for k in names])
    back = lambda *a: lib.gvx_melgan_disc_backward(h, P, None, *a)
    assert back(2, 15, P, P, table, len(names), P, P, bw, None) == -1
    assert back(2, 40, None, P, table, len(names), P, P, bw, None) == -1
    assert back(2, 40, P, None, table, len(names), P, P, bw, None) == -1
    assert back(2, 40, P, P, None, 0, None, P, bw, None) == -1                                  # nothing is asked for
    assert back(2, 40, P, P, None, 3, P, P, bw, None) == -1
    assert back(2, 40, P, P, table, len(names), P, P, bw - 1, None) == -5
    assert back(2, 40, P, P, table, len(names), P, None, bw, None) == -5
    assert back(2, 40, P, P, table, len(names) - 1, P, P, bw, None) == -3                       # the last bias has no destination
    assert names[-1].encode() in lib.gvx_last_error()
    table[2].numel += 1
    assert back(2, 40, P, P, table, len(names), P, P, bw, None) == -4
    assert lib.gvx_melgan_disc_pack_weights_device(C.byref(d), table, len(names), P, None) == -4
    assert lib.gvx_melgan_disc_pack_weights_device(C.byref(d), table, 2, P, None) == -3
    lib.gvx_melgan_disc_destroy(h)


def test_module_refuses_on_the_host():
    model = MelGANDiscriminator(_config(DR.TINY))
    assert model.min_samples == 16
    with pytest.raises(RuntimeError, match="MI355X"):
        model(torch.zeros(1, 64))
