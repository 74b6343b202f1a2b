"""CPU: the host side of the HiFi-GAN scale discriminators - symbols, config refusals, the parameter count, the lengths and the layout's
arithmetic against values worked by hand, the restatement against torch.nn.Conv1d and AvgPool1d composed as in the published
DiscriminatorS / MultiScaleDiscriminator (through spectral and weight normalisation and the three checkpoint forms), the spectral-norm
parametrisation against torch.nn.utils.spectral_norm in training mode, and the C ABI's refusals before any pointer is looked at.
No GPU call."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from genvox_amd import _lib, build
from genvox_amd.configs import HiFiGANScaleDiscriminatorConfig
from genvox_amd.hifigan_msd import HiFiGANScaleDiscriminator, _SpectralLayer, dims_from_config
from tests import hifigan_msd_ref64 as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gvx_hifigan_msd_blob_floats", "gvx_hifigan_msd_pack_weights_device", "gvx_hifigan_msd_create", "gvx_hifigan_msd_destroy",
       "gvx_hifigan_msd_bind", "gvx_hifigan_msd_layout", "gvx_hifigan_msd_features_bytes", "gvx_hifigan_msd_workspace_bytes",
       "gvx_hifigan_msd_forward", "gvx_hifigan_msd_backward", "gvx_hifigan_msd_timing_enable", "gvx_hifigan_msd_layer_times_ms")
ULP32 = 2.0 ** -23


def _config(cfg, spectral=(0,)) -> HiFiGANScaleDiscriminatorConfig:
    return HiFiGANScaleDiscriminatorConfig(n_scales=cfg["n_scales"], channels=cfg["channels"], kernel_sizes=cfg["kernel_sizes"], strides=cfg["strides"],
                                           groups=cfg["groups"], spectral_norm_scales=spectral, leaky_slope=cfg["slope"])


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    declared = set(re.findall(r"\b(gvx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "hifigan_msd.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "hifigan_msd.hip"))
    import genvox_amd
    assert genvox_amd.HiFiGANScaleDiscriminator is HiFiGANScaleDiscriminator
    assert genvox_amd.HiFiGANScaleDiscriminatorConfig is HiFiGANScaleDiscriminatorConfig


def test_both_matrix_instructions_are_in_the_source():
    src = open(os.path.join(build.CSRC, "hifigan_msd.hip")).read()
    assert src.count("__builtin_amdgcn_mfma_f32_32x32x2f32") >= 2 and src.count("__builtin_amdgcn_mfma_f32_16x16x4f32") >= 2   # convolution, weight gradient
    assert "atomic" not in src.replace("No atomics", "")


def test_which_layers_run_on_the_matrix_instruction():
    """The rule of the header: per-group input channels a multiple of 8, output channels a multiple of 16 - layers 1 to 6 of the
    published shape; both counts multiples of 32 for the 32x32x2 form."""
    kind = lambda cin, cout, g: 0 if (cin // g) % 8 or (cout // g) % 16 else (32 if (cin // g) % 32 == 0 and (cout // g) % 32 == 0 else 16)
    assert [kind(ci, co, g) for ci, co, _k, _s, _p, g in SR.layer_shapes(SR.DEFAULT)] == [0, 32, 16, 16, 32, 32, 32, 0]
    assert [kind(ci, co, g) for ci, co, _k, _s, _p, g in SR.layer_shapes(SR.MIXED)] == [0, 32, 16, 16, 32, 32, 32, 0]
    assert [kind(ci, co, g) for ci, co, _k, _s, _p, g in SR.layer_shapes(SR.TINY)] == [0, 0, 0, 0, 0]
    internal = open(os.path.join(build.CSRC, "hifigan_msd_internal.h")).read()
    assert "SD_MFMA_IN = 8;" in internal and "SD_MFMA_OUT = 16;" in internal


@pytest.mark.parametrize("bad,field", [(dict(kernel_sizes=(15, 40)), "kernel_sizes"), (dict(kernel_sizes=(15, 43)), "kernel_sizes"),
                                       (dict(n_scales=0), "n_scales"), (dict(n_scales=5), "n_scales"), (dict(n_scales=2.0), "n_scales"),
                                       (dict(channels=(8,), kernel_sizes=(5,), strides=(1,), groups=(1,)), "channels"),
                                       (dict(channels=(8,) * 9, kernel_sizes=(5,) * 9, strides=(1,) * 9, groups=(1,) * 9), "channels"),
                                       (dict(channels=(8, 0)), "channels"), (dict(channels=(8, 5000)), "channels"),
                                       (dict(strides=(1, 0)), "strides"), (dict(strides=(1, 9)), "strides"),
                                       (dict(groups=(1, 3)), "groups"), (dict(groups=(2, 1)), "groups"), (dict(groups=(1, 0)), "groups"),
                                       (dict(groups=(1,)), "groups"), (dict(spectral_norm_scales=(3,)), "spectral_norm_scales"),
                                       (dict(spectral_norm_scales=(0, 0)), "spectral_norm_scales"), (dict(leaky_slope=1.5), "leaky_slope")])
def test_config_refusals(bad, field):
    base = dict(n_scales=2, channels=(8, 16), kernel_sizes=(15, 41), strides=(1, 2), groups=(1, 4))
    with pytest.raises(ValueError, match=field):
        HiFiGANScaleDiscriminatorConfig(**{**base, **bad})
    if field == "spectral_norm_scales" or bad in (dict(n_scales=2.0), dict(groups=(1,))) or len(bad.get("channels", ())) > 8:
        return   # no C struct holds those
    d = dims_from_config(HiFiGANScaleDiscriminatorConfig(**base))
    for k, v in bad.items():
        if k in ("channels", "kernel_sizes", "strides", "groups"):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
            if k == "channels":
                d.n_layers = len(v)
        else:
            setattr(d, {"leaky_slope": "slope"}.get(k, k), v)
    h = C.c_void_p()
    assert _lib.load().gvx_hifigan_msd_create(C.byref(d), C.byref(h)) == -1
    assert _lib.load().gvx_hifigan_msd_blob_floats(C.byref(d)) == 0
    assert _lib.load().gvx_hifigan_msd_features_bytes(C.byref(d), 1, 64) == 0


def test_default_parameter_count():
    """By hand, one scale of the published shape (weights + biases; a grouped weight is [c_out][c_in / groups][k]):
    1 -> 128       k 15:        128 * 1 * 15 + 128       =     2,048
    128 -> 128     k 41, g 4:   128 * 32 * 41 + 128      =   168,064
    128 -> 256     k 41, g 16:  256 * 8 * 41 + 256       =    84,224
    256 -> 512     k 41, g 16:  512 * 16 * 41 + 512      =   336,384
    512 -> 1024    k 41, g 16:  1024 * 32 * 41 + 1024    = 1,344,512
    1024 -> 1024   k 41, g 16:  1024 * 64 * 41 + 1024    = 2,688,000
    1024 -> 1024   k 5:         1024 * 1024 * 5 + 1024   = 5,243,904
    score          k 3:         1024 * 3 + 1             =     3,073
    which is 9,870,209 per scale, 29,610,627 for the three, and with the period discriminators' 41,092,165 the published 70,702,792."""
    per = 2048 + 168064 + 84224 + 336384 + 1344512 + 2688000 + 5243904 + 3073
    assert per == 9870209
    cfg = HiFiGANScaleDiscriminatorConfig()
    assert cfg.parameter_count() == 3 * per == 29610627 and 29610627 + 41092165 == 70702792 and cfg.min_samples == 1
    assert cfg.spectral_norm_scales == [0]
    assert cfg.layer_shapes() == [(1, 128, 15, 1, 7, 1), (128, 128, 41, 2, 20, 4), (128, 256, 41, 2, 20, 16), (256, 512, 41, 4, 20, 16),
                                  (512, 1024, 41, 4, 20, 16), (1024, 1024, 41, 1, 20, 16), (1024, 1024, 5, 1, 2, 1), (1024, 1, 3, 1, 1, 1)]
    assert cfg.layer_shapes() == SR.layer_shapes(SR.DEFAULT)
    model = HiFiGANScaleDiscriminator(cfg)
    assert sum(p.numel() for p in model.parameters()) == 29610627
    blob = _lib.load().gvx_hifigan_msd_blob_floats(C.byref(dims_from_config(cfg)))
    assert blob % 64 == 0 and 2 * 29610627 - 3 * 4865 <= blob < 2 * 29610627 + 3 * 24 * 64   # every weight twice, rounded up to 64 floats
    sd = model.state_dict()
    assert sd["discriminators.0.convs.2.weight_orig"].shape == (256, 8, 41) and sd["discriminators.0.convs.2.weight_u"].shape == (256,)
    assert sd["discriminators.0.convs.2.weight_v"].shape == (8 * 41,) and sd["discriminators.1.convs.2.weight"].shape == (256, 8, 41)
    assert "discriminators.1.convs.2.weight_u" not in sd and "discriminators.0.convs.2.weight" not in sd


# The published shape: n' = n / 2 + 1 per scale; strides 1, 2, 2, 4, 4, 1, 1 and the score take L -> (L - 1) // stride + 1.
HAND = {
    1: [[1] * 8, [1] * 8, [1] * 8],                                                     # n_s = 1, 1, 1
    2: [[2, 1, 1, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1, 1, 1]],  # n_s = 2, 2, 2
    3: [[3, 2, 1, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1, 1, 1], [2, 1, 1, 1, 1, 1, 1, 1]],  # n_s = 3, 2, 2
    7: [[7, 4, 2, 1, 1, 1, 1, 1], [4, 2, 1, 1, 1, 1, 1, 1], [3, 2, 1, 1, 1, 1, 1, 1]],  # n_s = 7, 4, 3
    8192: [[8192, 4096, 2048, 512, 128, 128, 128, 128], [4097, 2049, 1025, 257, 65, 65, 65, 65], [2049, 1025, 513, 129, 33, 33, 33, 33]],
}
CHANNELS = [128, 128, 256, 512, 1024, 1024, 1024, 1]
POOLED = {1: [1, 1], 2: [2, 2], 3: [2, 2], 7: [4, 3], 8192: [4097, 2049]}


@pytest.mark.parametrize("n", sorted(HAND))
def test_lengths_and_layout_by_hand(n):
    model = HiFiGANScaleDiscriminator()
    assert model.feature_lengths(n) == HAND[n] == SR.map_lengths(SR.DEFAULT, n) and SR.scale_samples(SR.DEFAULT, n)[1:] == POOLED[n]
    lib, d = _lib.load(), model.dims()
    for B in (1, 3):
        lay = model.layout(B, n)
        at = 0
        for s, scale in enumerate(lay):
            for i, (off, c, length, strides) in enumerate(scale):
                assert (off, c, length) == (at, CHANNELS[i], HAND[n][s][i]) and off % 256 == 0
                assert strides == (length * c, 1, c)   # channels-last storage behind the [B, C, L] view
                at += (4 * B * c * length + 255) // 256 * 256
        assert lib.gvx_hifigan_msd_features_bytes(C.byref(d), B, n) == at
        fw, bw = lib.gvx_hifigan_msd_workspace_bytes(C.byref(d), B, n, 0), lib.gvx_hifigan_msd_workspace_bytes(C.byref(d), B, n, 1)
        assert fw == sum((4 * B * m + 255) // 256 * 256 for m in POOLED[n]) and bw > fw and bw % 256 == 0   # the pooled waveforms
        assert lib.gvx_hifigan_msd_layout(C.byref(d), B, n, None, 0) == 24
    assert model.map_lengths([n, 7])[2][1] == [HAND[n][2][1], 2]


def test_pooling_by_hand():
    """AvgPool1d(4, 2, 2) with count_include_pad: y[j] = (the sum of x[2j - 2 .. 2j + 1] inside the row) / 4, j = 0 .. n / 2."""
    x = torch.arange(1.0, 8.0, dtype=torch.float64)[None, None, :]   # 1 .. 7
    assert F.avg_pool1d(x, 4, 2, 2)[0, 0].tolist() == [(1 + 2) / 4, (1 + 2 + 3 + 4) / 4, (3 + 4 + 5 + 6) / 4, (5 + 6 + 7) / 4]
    assert F.avg_pool1d(x[:, :, :1], 4, 2, 2)[0, 0].tolist() == [1 / 4]
    assert F.avg_pool1d(x[:, :, :2], 4, 2, 2)[0, 0].tolist() == [3 / 4, 3 / 4]


def test_size_calls_return_zero_for_refused_shapes():
    lib, d = _lib.load(), dims_from_config(HiFiGANScaleDiscriminatorConfig())
    for B, n in ((1, 0), (0, 64), (65536, 64), (1, (1 << 24) + 1)):
        assert lib.gvx_hifigan_msd_features_bytes(C.byref(d), B, n) == 0
        assert lib.gvx_hifigan_msd_workspace_bytes(C.byref(d), B, n, 1) == 0
        assert lib.gvx_hifigan_msd_layout(C.byref(d), B, n, None, 0) == 0
    assert lib.gvx_hifigan_msd_features_bytes(C.byref(d), 1, 1) > 0
    with pytest.raises(ValueError):
        HiFiGANScaleDiscriminator().layout(1, 0)


class _PublishedS(nn.Module):
    """The published DiscriminatorS, built independently of the restatement."""

    def __init__(self, cfg, use_spectral_norm):
        super().__init__()
        norm_f = nn.utils.spectral_norm if use_spectral_norm else nn.utils.weight_norm
        chans = (1,) + tuple(cfg["channels"])
        self.slope = cfg["slope"]
        self.convs = nn.ModuleList([norm_f(nn.Conv1d(chans[i], chans[i + 1], k, s, groups=g, padding=k // 2))
                                    for i, (k, s, g) in enumerate(zip(cfg["kernel_sizes"], cfg["strides"], cfg["groups"]))])
        self.conv_post = norm_f(nn.Conv1d(chans[-1], 1, 3, 1, padding=1))

    def forward(self, x):
        fmap = []
        for l in self.convs:
            x = F.leaky_relu(l(x), self.slope)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return fmap


class _PublishedMSD(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.discriminators = nn.ModuleList([_PublishedS(cfg, use_spectral_norm=s == 0) for s in range(cfg["n_scales"])])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2) for _ in range(cfg["n_scales"] - 1)])

    def forward(self, x):
        out = []
        for i, d in enumerate(self.discriminators):
            if i != 0:
                x = self.meanpools[i - 1](x)
            out.append(d(x))
        return out


def _effective(model):
    return {k: v.detach() for k, v in zip(model.weight_names(), model.effective_weights())}


@pytest.mark.parametrize("cfg", [SR.TINY, SR.MIXED], ids=["TINY", "MIXED"])
def test_restatement_equals_the_published_composition_and_checkpoint_forms(cfg):
    torch.manual_seed(5)
    stack = _PublishedMSD(cfg).double()
    for p in stack.parameters():
        p.data.normal_(0.0, 0.3)
    stack.eval()
    sd = stack.state_dict()
    assert any(k.endswith("weight_orig") for k in sd) and any("weight_g" in k or "parametrizations" in k for k in sd)
    model = HiFiGANScaleDiscriminator(_config(cfg)).double().eval()
    model.load_state_dict(sd)                                   # spectral triples as they are, weight-norm pairs folded
    own = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert torch.equal(own["discriminators.0.convs.1.weight_orig"], sd["discriminators.0.convs.1.weight_orig"])
    assert torch.equal(own["discriminators.0.convs.1.weight_u"], sd["discriminators.0.convs.1.weight_u"])
    assert torch.equal(own["discriminators.0.conv_post.weight_v"], sd["discriminators.0.conv_post.weight_v"])
    eff = _effective(model)
    assert set(eff) == set(SR.random_state(cfg, 1)) and all(eff[k].shape == v.shape for k, v in SR.random_state(cfg, 1).items())
    folded = HiFiGANScaleDiscriminator(_config(cfg, spectral=())).double().eval()
    folded.load_state_dict(sd)                                  # a scale configured without spectral norm: weight_orig / sigma
    for k, v in folded.state_dict().items():
        torch.testing.assert_close(v, eff[k], rtol=1e-13, atol=0.0)
    for n in (1, 2, 7, 67, 130, 131):
        wav = SR.random_wav(2, n, 3)
        with torch.no_grad():
            want = stack(wav[:, None, :])
        got = SR.discriminator(eff, wav, cfg)
        assert [[m.shape[2] for m in ms] for ms in got] == SR.map_lengths(cfg, n) == model.feature_lengths(n)
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                torch.testing.assert_close(x, y, rtol=1e-12, atol=1e-13)
    other = HiFiGANScaleDiscriminator(_config(cfg)).double()
    other.load_state_dict({"mpd": {"ignored": torch.zeros(1)}, "msd": sd})        # the published checkpoint file
    third = HiFiGANScaleDiscriminator(_config(cfg)).double()
    third.load_checkpoint_statedicts(model.get_checkpoint_statedicts())           # this project's own form
    fourth = HiFiGANScaleDiscriminator(_config(cfg)).double()
    fourth.load_state_dict(model.get_checkpoint_statedicts())
    for m in (other, third, fourth):
        for k, v in m.state_dict().items():
            assert torch.equal(v, own[k]), k
    # a plain weight given to a spectral scale becomes its weight_orig; the scale keeps its u and v
    fifth = HiFiGANScaleDiscriminator(_config(cfg)).double()
    before = {k: v.clone() for k, v in fifth.state_dict().items()}
    fifth.load_state_dict(folded.state_dict())
    for k, v in fifth.state_dict().items():
        if k.endswith("weight_orig"):
            assert torch.equal(v, folded.state_dict()[k.replace("weight_orig", "weight")]), k
        elif k.endswith(("weight_u", "weight_v")) and k.startswith("discriminators.0."):
            assert torch.equal(v, before[k]), k
    with pytest.raises(KeyError):
        fifth.load_state_dict({k: v for k, v in sd.items() if k != "discriminators.0.convs.0.weight_u"})


def test_spectral_norm_is_torchs_in_training_mode():
    """Three successive training-mode forwards of torch.nn.utils.spectral_norm(Conv1d) beside three effective_weight() calls from the
    same start: u, v and the effective weight to within 4 float32 ulps of their largest value, and so the gradient on weight_orig from a
    random cotangent on the effective weight (sigma is in the graph, u and v are constants).  Then eval mode: no iteration."""
    torch.manual_seed(2)
    conv = nn.utils.spectral_norm(nn.Conv1d(16, 32, 41, 2, groups=2, padding=20))
    layer = _SpectralLayer((32, 8, 41), 32, 8 * 41)
    with torch.no_grad():
        layer.weight_orig.copy_(conv.weight_orig)
        layer.weight_u.copy_(conv.weight_u)
        layer.weight_v.copy_(conv.weight_v)
    assert layer.weight_u.shape == conv.weight_u.shape == (32,) and layer.weight_v.shape == conv.weight_v.shape == (8 * 41,)
    x = torch.randn(2, 16, 50)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=0.0, atol=4 * ULP32 * b.abs().max().item())
    conv.train(), layer.train()
    for step in range(3):
        conv(x)
        theirs, mine = conv.weight, layer.effective_weight()
        close(layer.weight_u, conv.weight_u)
        close(layer.weight_v, conv.weight_v)
        close(mine, theirs)
        G = torch.randn(32, 8, 41)
        conv.weight_orig.grad = layer.weight_orig.grad = None
        (theirs * G).sum().backward()
        (mine * G).sum().backward()
        close(layer.weight_orig.grad, conv.weight_orig.grad)
        ref, u, v = SR.spectral_weight(conv.weight_orig.detach().double(), conv.weight_u.double(), conv.weight_v.double(), training=False)
        close(mine.detach(), ref.float())
    conv.eval(), layer.eval()
    u0, v0 = layer.weight_u.clone(), layer.weight_v.clone()
    conv(x)
    close(layer.effective_weight(), conv.weight)
    assert torch.equal(layer.weight_u, u0) and torch.equal(layer.weight_v, v0)


def test_pinned_restatement_and_ragged_rows():
    cfg = SR.TINY
    sd = SR.random_state(cfg, 7)
    wav = SR.random_wav(2, 37, 2)
    G = SR.random_cotangents(cfg, 2, 37, 9)
    free = SR.reference(sd, wav, None, cfg, G)
    pinned = SR.reference(sd, wav, None, cfg, G, SR.masks_from_maps(free["maps"], cfg["slope"]))
    for k in free["grads"]:
        torch.testing.assert_close(pinned["grads"][k], free["grads"][k], rtol=1e-12, atol=1e-14)
    lens = (37, 1)
    poisoned = wav.clone()
    poisoned[1, 1:] = float("nan")
    rag = SR.reference(sd, poisoned, lens, cfg, G)
    alone = [SR.reference(sd, wav[b:b + 1, :n], None, cfg, [[g[b:b + 1] for g in gs] for gs in G]) for b, n in enumerate(lens)]
    for k in sd:
        torch.testing.assert_close(rag["grads"][k], alone[0]["grads"][k] + alone[1]["grads"][k], rtol=1e-12, atol=1e-14)
    assert not rag["grads"]["wav"][1, 1:].any() and torch.equal(rag["grads"]["wav"][1, :1], alone[1]["grads"]["wav"][0])


def test_calls_refuse_on_the_host():
    """Bad B and n_max, NULL arguments, no blob, short or misaligned buffers, missing gradient names: all refused before the (bogus)
    pointers are looked at."""
    lib, d = _lib.load(), dims_from_config(_config(SR.TINY))
    h = C.c_void_p()
    assert lib.gvx_hifigan_msd_create(C.byref(d), C.byref(h)) == 0
    assert lib.gvx_hifigan_msd_create(None, C.byref(h.__class__())) == -1
    P = 1 << 20
    fb, fw, bw = (lib.gvx_hifigan_msd_features_bytes(C.byref(d), 2, 40), lib.gvx_hifigan_msd_workspace_bytes(C.byref(d), 2, 40, 0),
                  lib.gvx_hifigan_msd_workspace_bytes(C.byref(d), 2, 40, 1))
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 40, P, fb, P, fw, None) == -7          # no blob bound
    assert lib.gvx_hifigan_msd_bind(h, 4) == -1 and lib.gvx_hifigan_msd_bind(h, None) == -1
    assert lib.gvx_hifigan_msd_bind(h, 256) == 0
    assert lib.gvx_hifigan_msd_forward(None, P, None, 2, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_msd_forward(h, None, None, 2, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 40, None, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_msd_forward(h, P, None, 0, 40, P, fb, P, fw, None) == -1
    assert lib.gvx_hifigan_msd_forward(h, P, None, 65536, 40, P, 1 << 40, P, 1 << 40, None) == -1
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 0, P, fb, P, fw, None) == -1
    assert b"at least 1 sample" in lib.gvx_last_error()
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, (1 << 24) + 1, P, 1 << 40, P, 1 << 40, None) == -2
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 40, P, fb - 1, P, fw, None) == -5
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 40, P + 4, fb, P, fw, None) == -5
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 40, P, fb, None, fw, None) == -5
    assert lib.gvx_hifigan_msd_forward(h, P, None, 2, 40, P, fb, P, fw - 1, None) == -5
    shapes = {k: v.numel() for k, v in SR.random_state(SR.TINY, 1).items()}
    names = list(shapes)
    table = (_lib.gvx_weight_desc * len(names))(*[_lib.gvx_weight_desc(k.encode(), P, shapes[k]) for k in names])
    back = lambda *a: lib.gvx_hifigan_msd_backward(h, P, None, *a)
    assert back(2, 0, P, P, table, len(names), P, P, bw, None) == -1
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
    assert lib.gvx_hifigan_msd_pack_weights_device(C.byref(d), table, len(names), P, None) == -4
    assert lib.gvx_hifigan_msd_pack_weights_device(C.byref(d), table, 2, P, None) == -3
    assert lib.gvx_hifigan_msd_timing_enable(None, 1) == -1
    lib.gvx_hifigan_msd_destroy(h)


def test_module_refuses_on_the_host():
    model = HiFiGANScaleDiscriminator(_config(SR.TINY))
    assert model.min_samples == 1
    with pytest.raises(RuntimeError, match="MI355X"):
        model(torch.zeros(1, 64))
