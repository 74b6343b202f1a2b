"""CPU: the host side of the HiFi-GAN period discriminators - symbols, config refusals, the parameter count, the heights and the layout's
arithmetic against values worked by hand, the restatement against torch.nn.Conv2d composed as in the published DiscriminatorP (through
weight normalisation and the three checkpoint forms), the least-squares losses against the published formulas, and the C ABI's refusals
before any pointer is looked at.  No GPU call."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from genvox_amd import _lib, build
from genvox_amd.configs import HiFiGANPeriodDiscriminatorConfig, HiFiGANTrainingConfig
from genvox_amd.hifigan_disc import HiFiGANPeriodDiscriminator, dims_from_config
from genvox_amd.losses import HiFiGANDiscriminatorLoss, HiFiGANGeneratorLoss
from tests import hifigan_disc_ref64 as DR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gvx_hifigan_mpd_blob_floats", "gvx_hifigan_mpd_pack_weights_device", "gvx_hifigan_mpd_create", "gvx_hifigan_mpd_destroy",
       "gvx_hifigan_mpd_bind", "gvx_hifigan_mpd_layout", "gvx_hifigan_mpd_features_bytes", "gvx_hifigan_mpd_workspace_bytes",
       "gvx_hifigan_mpd_forward", "gvx_hifigan_mpd_backward")


def _config(cfg) -> HiFiGANPeriodDiscriminatorConfig:
    return HiFiGANPeriodDiscriminatorConfig(periods=cfg["periods"], channels=cfg["channels"], kernel_size=cfg["kernel_size"], stride=cfg["stride"],
                                            leaky_slope=cfg["slope"])


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    declared = set(re.findall(r"\b(gvx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "hifigan_disc.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "hifigan_disc.hip"))
    import genvox_amd
    assert genvox_amd.HiFiGANPeriodDiscriminator is HiFiGANPeriodDiscriminator
    assert genvox_amd.HiFiGANPeriodDiscriminatorConfig is HiFiGANPeriodDiscriminatorConfig and genvox_amd.HiFiGANTrainingConfig is HiFiGANTrainingConfig
    assert genvox_amd.HiFiGANTrainer.__name__ == "HiFiGANTrainer" and genvox_amd.HiFiGANGeneratorLoss is HiFiGANGeneratorLoss
    assert genvox_amd.HiFiGANDiscriminatorLoss is HiFiGANDiscriminatorLoss


def test_the_matrix_instruction_is_in_the_source():
    src = open(os.path.join(build.CSRC, "hifigan_disc.hip")).read()
    assert src.count("__builtin_amdgcn_mfma_f32_32x32x2f32") >= 5   # four in the convolution kernel's k-step, one in the weight gradient's


@pytest.mark.parametrize("bad,field", [(dict(kernel_size=4), "kernel_size"), (dict(kernel_size=17), "kernel_size"), (dict(periods=(2, 65)), "periods"),
                                       (dict(periods=(0,)), "periods"), (dict(periods=tuple(range(2, 11))), "periods"), (dict(periods=()), "periods"),
                                       (dict(channels=(8,)), "channels"), (dict(channels=(8,) * 9), "channels"), (dict(channels=(8, 100)), "channels"),
                                       (dict(channels=(8, 0)), "channels"), (dict(stride=0), "stride"), (dict(stride=9), "stride"),
                                       (dict(leaky_slope=1.5), "leaky_slope"), (dict(kernel_size=5.0), "kernel_size")])
def test_config_refusals(bad, field):
    with pytest.raises(ValueError, match=field):
        HiFiGANPeriodDiscriminatorConfig(**bad)
    if field in ("periods", "channels") and len(bad[field]) > 8 or bad == dict(kernel_size=5.0):
        return   # no C struct holds those
    d = dims_from_config(HiFiGANPeriodDiscriminatorConfig())
    if field == "periods":
        d.n_periods = len(bad[field])
        for i, p in enumerate(bad[field]):
            d.periods[i] = p
    elif field == "channels":
        d.n_layers = len(bad[field])
        for i, c in enumerate(bad[field]):
            d.channels[i] = c
    else:
        setattr(d, {"leaky_slope": "slope"}.get(field, field), bad[field])
    h = C.c_void_p()
    assert _lib.load().gvx_hifigan_mpd_create(C.byref(d), C.byref(h)) == -1
    assert _lib.load().gvx_hifigan_mpd_blob_floats(C.byref(d)) == 0


def test_default_parameter_count_and_training_config():
    """By hand, one period of the default shape (weights + biases):
    1 -> 32:       32 * 1 * 5 + 32         =       192
    32 -> 128:     128 * 32 * 5 + 128      =    20,608
    128 -> 512:    512 * 128 * 5 + 512     =   328,192
    512 -> 1024:   1024 * 512 * 5 + 1024   = 2,622,464
    1024 -> 1024:  1024 * 1024 * 5 + 1024  = 5,243,904
    score:         1024 * 3 + 1            =     3,073"""
    per = 192 + 20608 + 328192 + 2622464 + 5243904 + 3073
    assert per == 8218433
    cfg = HiFiGANPeriodDiscriminatorConfig()
    assert cfg.parameter_count() == 5 * per == 41092165 and cfg.min_samples == 11
    assert cfg.layer_shapes() == [(1, 32, 5, 3, 2), (32, 128, 5, 3, 2), (128, 512, 5, 3, 2), (512, 1024, 5, 3, 2), (1024, 1024, 5, 1, 2), (1024, 1, 3, 1, 1)]
    blob = _lib.load().gvx_hifigan_mpd_blob_floats(C.byref(dims_from_config(cfg)))
    assert blob % 64 == 0 and 2 * 41092165 - 5 * 4609 <= blob < 2 * 41092165 + 5 * 18 * 64   # every weight twice, rounded up to 64 floats
    tc = HiFiGANTrainingConfig()
    assert (tc.learning_rate, tc.adam_b1, tc.adam_b2, tc.lr_decay, tc.feat_match, tc.aux_weight) == (2e-4, 0.8, 0.99, 0.999, 2.0, 45.0)
    assert not tc.grad_clip_thresh > 0
    assert HiFiGANTrainingConfig.from_published({"learning_rate": 1e-4, "adam_b1": 0.5, "segment_size": 8192}).adam_b1 == 0.5


# Default shape: H_0 = ceil(n / p); the four strided layers each take H -> (H - 1) // 3 + 1; the last layer and the score keep it.
HAND = {
    11: [[2, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],       # H_0 = 6, 4, 3, 2, 1
    12: [[2, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]],       # H_0 = 6, 4, 3, 2, 2
    8192: [[1366, 456, 152, 51, 51, 51], [911, 304, 102, 34, 34, 34], [547, 183, 61, 21, 21, 21], [391, 131, 44, 15, 15, 15],
           [249, 83, 28, 10, 10, 10]],     # H_0 = 4096, 2731, 1639, 1171, 745
}
CHANNELS = [32, 128, 512, 1024, 1024, 1]


@pytest.mark.parametrize("n", sorted(HAND))
def test_heights_and_layout_by_hand(n):
    model = HiFiGANPeriodDiscriminator()
    assert model.feature_heights(n) == HAND[n] == DR.map_heights(DR.DEFAULT, n)
    lib, d = _lib.load(), model.dims()
    for B in (1, 3):
        lay = model.layout(B, n)
        at = 0
        for j, (period, p) in enumerate(zip(lay, (2, 3, 5, 7, 11))):
            for i, (off, c, h, pp, strides) in enumerate(period):
                assert (off, c, h, pp) == (at, CHANNELS[i], HAND[n][j][i], p) and off % 256 == 0
                assert strides == (h * p * c, 1, p * c, c)   # channels-last storage behind the [B, C, H, p] view
                at += (4 * B * c * h * p + 255) // 256 * 256
        assert lib.gvx_hifigan_mpd_features_bytes(C.byref(d), B, n) == at
        fw, bw = lib.gvx_hifigan_mpd_workspace_bytes(C.byref(d), B, n, 0), lib.gvx_hifigan_mpd_workspace_bytes(C.byref(d), B, n, 1)
        assert fw == 256 and bw > fw and bw % 256 == 0
        assert lib.gvx_hifigan_mpd_layout(C.byref(d), B, n, None, 0) == 30
    assert model.map_lengths([n, 11])[4][0] == [HAND[n][4][0], 1]


def test_reflection_by_hand():
    """n = 11 with p = 11: nothing is reflected, H = 1 everywhere.  n = 12 with p = 11: H_0 = 2, the 10 samples 12 .. 21 of the grid are
    the reflection x[10], x[9], .. x[1] (no repeated edge sample)."""
    x = torch.arange(12.0)[None, :]
    assert torch.equal(DR.to_grid(x[:, :11], 11), x[:, :11].reshape(1, 1, 1, 11))
    grid = DR.to_grid(x, 11)
    assert grid.shape == (1, 1, 2, 11)
    assert grid[0, 0, 1].tolist() == [11.0] + [float(v) for v in range(10, 0, -1)]
    assert DR.to_grid(x, 2).shape == (1, 1, 6, 2) and torch.equal(DR.to_grid(x, 2).reshape(1, 12), x)
    assert DR.to_grid(torch.arange(7.0)[None, :], 3)[0, 0].tolist() == [[0, 1, 2], [3, 4, 5], [6, 5, 4]]   # n % p = 1: p - 1 = 2 reflected


def test_size_calls_return_zero_for_refused_shapes():
    lib, d = _lib.load(), dims_from_config(HiFiGANPeriodDiscriminatorConfig())
    for B, n in ((1, 10), (0, 64), (65536, 64), (1, (1 << 24) + 1)):
        assert lib.gvx_hifigan_mpd_features_bytes(C.byref(d), B, n) == 0
        assert lib.gvx_hifigan_mpd_workspace_bytes(C.byref(d), B, n, 1) == 0
        assert lib.gvx_hifigan_mpd_layout(C.byref(d), B, n, None, 0) == 0
    assert lib.gvx_hifigan_mpd_features_bytes(C.byref(d), 1, 11) > 0
    with pytest.raises(ValueError):
        HiFiGANPeriodDiscriminator().layout(1, 10)


class _PublishedP(nn.Module):
    """The published DiscriminatorP, built independently of the restatement."""

    def __init__(self, period, cfg):
        super().__init__()
        wn, k, s = nn.utils.weight_norm, cfg["kernel_size"], cfg["stride"]
        chans = (1,) + tuple(cfg["channels"])
        self.period, self.slope = period, cfg["slope"]
        self.convs = nn.ModuleList([wn(nn.Conv2d(chans[i], chans[i + 1], (k, 1), (s if i < len(chans) - 2 else 1, 1), padding=(k // 2, 0)))
                                    for i in range(len(chans) - 1)])
        self.conv_post = wn(nn.Conv2d(chans[-1], 1, (3, 1), 1, padding=(1, 0)))

    def forward(self, x):
        fmap = []
        b, c, t = x.shape
        if t % self.period != 0:
            n_pad = self.period - (t % self.period)
            x = F.pad(x, (0, n_pad), "reflect")
            t = t + n_pad
        x = x.view(b, c, t // self.period, self.period)
        for l in self.convs:
            x = F.leaky_relu(l(x), self.slope)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return fmap


class _PublishedMPD(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.discriminators = nn.ModuleList([_PublishedP(p, cfg) for p in cfg["periods"]])

    def forward(self, x):
        return [d(x) for d in self.discriminators]


@pytest.mark.parametrize("cfg", [DR.TINY, DR.MIXED], ids=["TINY", "MIXED"])
def test_restatement_equals_the_published_composition_and_checkpoint_forms(cfg):
    torch.manual_seed(5)
    stack = _PublishedMPD(cfg).double()
    for p in stack.parameters():
        p.data.normal_(0.0, 0.3)
    sd = stack.state_dict()
    assert any("weight_g" in k or "parametrizations" in k for k in sd)
    model = HiFiGANPeriodDiscriminator(_config(cfg)).double()
    model.load_state_dict(sd)                                   # weight-normalised keys
    folded = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert set(folded) == set(DR.random_state(cfg, 1)) and all(folded[k].shape == v.shape for k, v in DR.random_state(cfg, 1).items())
    for n in (DR.min_samples(cfg), 67, 70, 71):
        wav = DR.random_wav(2, n, 3)
        with torch.no_grad():
            want = stack(wav[:, None, :])
        got = DR.discriminator(folded, wav, cfg)
        assert [[m.shape[2] for m in ms] for ms in got] == DR.map_heights(cfg, n) == model.feature_heights(n)
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                torch.testing.assert_close(x, y, rtol=1e-12, atol=1e-13)
    other = HiFiGANPeriodDiscriminator(_config(cfg)).double()
    other.load_state_dict({"mpd": sd, "msd": {"ignored": torch.zeros(1)}})        # the published checkpoint file
    third = HiFiGANPeriodDiscriminator(_config(cfg)).double()
    third.load_checkpoint_statedicts(model.get_checkpoint_statedicts())           # this project's own form
    fourth = HiFiGANPeriodDiscriminator(_config(cfg)).double()
    fourth.load_state_dict(model.get_checkpoint_statedicts())
    for m in (other, third, fourth):
        for k, v in m.state_dict().items():
            assert torch.equal(v, folded[k]), k


def test_pinned_restatement_and_ragged_rows():
    cfg = DR.TINY
    sd = DR.random_state(cfg, 7)
    wav = DR.random_wav(2, 37, 2)
    G = DR.random_cotangents(cfg, 2, 37, 9)
    free = DR.reference(sd, wav, None, cfg, G)
    pinned = DR.reference(sd, wav, None, cfg, G, DR.masks_from_maps(free["maps"], cfg["slope"]))
    for k in free["grads"]:
        torch.testing.assert_close(pinned["grads"][k], free["grads"][k], rtol=1e-12, atol=1e-14)
    lens = (37, 20)
    poisoned = wav.clone()
    poisoned[1, 20:] = float("nan")
    rag = DR.reference(sd, poisoned, lens, cfg, G)
    alone = [DR.reference(sd, wav[b:b + 1, :n], None, cfg, [[g[b:b + 1] for g in gs] for gs in G]) for b, n in enumerate(lens)]
    for k in sd:
        torch.testing.assert_close(rag["grads"][k], alone[0]["grads"][k] + alone[1]["grads"][k], rtol=1e-12, atol=1e-14)
    assert not rag["grads"]["wav"][1, 20:].any() and torch.equal(rag["grads"]["wav"][1, :20], alone[1]["grads"]["wav"][0])


def test_losses_are_the_published_formulas():
    """Equal-length rows: the published discriminator_loss, generator_loss and feature_loss (times 2), written out here, over a 4-D
    output (two periods) and a 3-D output (one scale) together; then the ragged rule on a map with NaN behind a row's height."""
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g)
    real_p = [[mk(2, 4, 5, 2), mk(2, 1, 3, 2)], [mk(2, 4, 4, 3), mk(2, 1, 2, 3)]]
    fake_p = [[mk(2, 4, 5, 2), mk(2, 1, 3, 2)], [mk(2, 4, 4, 3), mk(2, 1, 2, 3)]]
    real_s = [[mk(2, 3, 7), mk(2, 1, 7)]]
    fake_s = [[mk(2, 3, 7), mk(2, 1, 7)]]
    subs_r, subs_f = real_p + real_s, fake_p + fake_s
    d_want = sum(torch.mean((1 - r[-1]) ** 2) + torch.mean(f[-1] ** 2) for r, f in zip(subs_r, subs_f))
    adv_want = sum(torch.mean((1 - f[-1]) ** 2) for f in subs_f)
    fm_want = 2 * sum(torch.mean(torch.abs(rl - gl)) for r, f in zip(subs_r, subs_f) for rl, gl in zip(r, f))
    d_loss, g_loss = HiFiGANDiscriminatorLoss(), HiFiGANGeneratorLoss(2.0)
    torch.testing.assert_close(d_loss([real_p, real_s], [fake_p, fake_s]), d_want)
    torch.testing.assert_close(g_loss([real_p, real_s], [fake_p, fake_s]), adv_want + fm_want)
    torch.testing.assert_close(g_loss.last_terms[0], adv_want)
    torch.testing.assert_close(g_loss.last_terms[1], fm_want)
    # one discriminator's output passes as it is
    torch.testing.assert_close(d_loss(real_s, fake_s), torch.mean((1 - real_s[0][-1]) ** 2) + torch.mean(fake_s[0][-1] ** 2))
    # ragged, by hand: score [2, 1, 2, 2], row 1 has height 1; real = 0 -> (1 - 0)^2 = 1 everywhere; fake row 0 = 2 -> 4, row 1 = 3 -> 9
    real = [[torch.zeros(2, 1, 2, 2)]]
    fake = [[torch.tensor([[[[2.0, 2.0], [2.0, 2.0]]], [[[3.0, 3.0], [float("nan"), float("nan")]]]])]]
    assert torch.isnan(d_loss(real, fake))
    torch.testing.assert_close(d_loss(real, fake, [[[2, 1]]]), torch.tensor(1.0 + (4.0 + 9.0) / 2))
    torch.testing.assert_close(g_loss(real, fake, [[[2, 1]]]), torch.tensor((1.0 + 4.0) / 2 + 2.0 * (2.0 + 3.0) / 2))
    # the real maps are detached
    r = real_p[0][0].clone().requires_grad_(True)
    f = fake_p[0][0].clone().requires_grad_(True)
    g_loss([[r, real_p[0][1]]], [[f, fake_p[0][1]]]).backward()
    assert r.grad is None and f.grad is not None
    with pytest.raises(ValueError):
        d_loss([[torch.zeros(2, 3)]], [[torch.zeros(2, 3)]], [[[1, 1]]])


def test_calls_refuse_on_the_host():
    """Bad B and n_max, NULL arguments, no blob, short or misaligned buffers, missing gradient names: all refused before the (bogus)
    pointers are looked at."""
    lib, d = _lib.load(), dims_from_config(_config(DR.TINY))
    h = C.c_void_p()
    assert lib.gvx_hifigan_mpd_create(C.byref(d), C.byref(h)) == 0
    P = 1 << 20
    fb, fw, bw = (lib.gvx_hifigan_mpd_features_bytes(C.byref(d), 2, 40), lib.gvx_hifigan_mpd_workspace_bytes(C.byref(d), 2, 40, 0),
                  lib.gvx_hifigan_mpd_workspace_bytes(C.byref(d), 2, 40, 1))
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 40, P, fb, P, fw, None) == -7          # no blob bound
    assert lib.gvx_hifigan_mpd_bind(h, 4) == -1 and lib.gvx_hifigan_mpd_bind(h, None) == -1
    assert lib.gvx_hifigan_mpd_bind(h, 256) == 0
    assert lib.gvx_hifigan_mpd_forward(None, P, None, 2, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_mpd_forward(h, None, None, 2, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 40, None, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 0, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 65536, 40, P, 1 << 40, P, 1 << 40, None) == -1
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 2, P, fb, P, fw, None) == -1           # TINY's largest period is 3
    assert b"reflection" in lib.gvx_last_error()
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, (1 << 24) + 1, P, 1 << 40, P, 1 << 40, None) == -2
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 40, P, fb - 1, P, fw, None) == -5
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 40, P + 4, fb, P, fw, None) == -5
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 40, P, fb, None, fw, None) == -5
    assert lib.gvx_hifigan_mpd_forward(h, P, None, 2, 40, P, fb, P, fw - 1, None) == -5
    shapes = {k: v.numel() for k, v in DR.random_state(DR.TINY, 1).items()}
    names = list(shapes)
    table = (_lib.gvx_weight_desc * len(names))(*[_lib.gvx_weight_desc(k.encode(), P, shapes[k]) for k in names])
    back = lambda *a: lib.gvx_hifigan_mpd_backward(h, P, None, *a)
    assert back(2, 2, P, P, table, len(names), P, P, bw, None) == -1
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
    assert lib.gvx_hifigan_mpd_pack_weights_device(C.byref(d), table, len(names), P, None) == -4
    assert lib.gvx_hifigan_mpd_pack_weights_device(C.byref(d), table, 2, P, None) == -3
    lib.gvx_hifigan_mpd_destroy(h)


def test_module_refuses_on_the_host():
    model = HiFiGANPeriodDiscriminator(_config(DR.TINY))
    assert model.min_samples == 3
    with pytest.raises(RuntimeError, match="MI355X"):
        model(torch.zeros(1, 64))
