"""CPU: the host side of the multi-resolution spectrogram discriminator - symbols, config and dims refusals, the parameter count, the
widths and the layout's arithmetic against values worked by hand and against the restatement's own shapes, the restatement against the
published composition (torch.stft + norm + weight-normalised Conv2d) through the checkpoint forms, and the C ABI's refusals before any
pointer is looked at.  No GPU call."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from genvox_amd import _lib, build
from genvox_amd.configs import MultiResolutionDiscriminatorConfig
from genvox_amd.mrd import MultiResolutionDiscriminator, dims_from_config, map_widths
from tests import mrd_cases as MC
from tests import mrd_ref64 as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gvx_mrd_blob_floats", "gvx_mrd_pack_weights_device", "gvx_mrd_create", "gvx_mrd_destroy", "gvx_mrd_bind", "gvx_mrd_layout",
       "gvx_mrd_features_bytes", "gvx_mrd_workspace_bytes", "gvx_mrd_forward", "gvx_mrd_backward", "gvx_mrd_timing_enable",
       "gvx_mrd_layer_times_ms")


def _config(cfg) -> MultiResolutionDiscriminatorConfig:
    return MultiResolutionDiscriminatorConfig(resolutions=cfg["resolutions"], channels=cfg["channels"], leaky_slope=cfg["slope"], window=cfg["window"])


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    declared = set(re.findall(r"\b(gvx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "mrd.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mrd.hip"))
    import genvox_amd
    assert genvox_amd.MultiResolutionDiscriminator is MultiResolutionDiscriminator
    assert genvox_amd.MultiResolutionDiscriminatorConfig is MultiResolutionDiscriminatorConfig


def test_the_matrix_instruction_is_in_the_source_and_the_constants_are_the_tests():
    src = open(os.path.join(build.CSRC, "mrd.hip")).read()
    assert src.count("__builtin_amdgcn_mfma_f32_32x32x2f32") >= 5   # four in the convolution kernel's k-step, one in the weight gradient's
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    assert f"GVX_MRD_TILE = {MC.TILE}," in header and f"GVX_MRD_TILE_NARROW = {MC.TILE_NARROW}," in header
    assert f"GVX_MRD_PIECE_FRAMES = {MC.PIECE_FRAMES}," in header
    internal = open(os.path.join(build.CSRC, "mrd_internal.h")).read()
    assert f"MR_TILE = {MC.TILE};" in internal and f"MR_TILE_NARROW = {MC.TILE_NARROW};" in internal and f"MR_PIECE_FRAMES = {MC.PIECE_FRAMES};" in internal


@pytest.mark.parametrize("bad,field", [(dict(resolutions=()), "resolutions"), (dict(resolutions=((512, 50, 240),) * 9), "resolutions"),
                                       (dict(resolutions=((256, 50, 240),)), "n_fft"), (dict(resolutions=((1000, 50, 240),)), "n_fft"),
                                       (dict(resolutions=((512, 0, 240),)), "hop"), (dict(resolutions=((512, 241, 240),)), "hop"),
                                       (dict(resolutions=((512, 50, 513),)), "win"), (dict(resolutions=((512, 50),)), "triple"),
                                       (dict(channels=16), "channels"), (dict(channels=48), "channels"), (dict(channels=160), "channels"),
                                       (dict(channels=32.0), "channels"), (dict(leaky_slope=1.5), "leaky_slope"), (dict(leaky_slope=-0.1), "leaky_slope"),
                                       (dict(window="hamming"), "window")])
def test_config_and_dims_refusals(bad, field):
    with pytest.raises(ValueError, match=field):
        MultiResolutionDiscriminatorConfig(**bad)
    d = dims_from_config(MultiResolutionDiscriminatorConfig())
    if "resolutions" in bad:
        if len(bad["resolutions"]) > 8 or any(len(r) != 3 for r in bad["resolutions"]):
            return   # no C struct holds those
        d.n_resolutions = len(bad["resolutions"])
        for i, (n_fft, hop, win) in enumerate(bad["resolutions"]):
            d.n_fft[i], d.hop[i], d.win[i] = n_fft, hop, win
    elif field == "channels":
        if not isinstance(bad["channels"], int):
            return
        d.channels = bad["channels"]
    elif field == "leaky_slope":
        d.slope = bad["leaky_slope"]
    else:
        d.window = 2
    lib, h = _lib.load(), C.c_void_p()
    assert lib.gvx_mrd_create(C.byref(d), C.byref(h)) == -1
    assert lib.gvx_mrd_blob_floats(C.byref(d)) == 0
    assert lib.gvx_mrd_features_bytes(C.byref(d), 1, 4000) == 0 and lib.gvx_mrd_workspace_bytes(C.byref(d), 1, 4000, 1) == 0
    assert lib.gvx_mrd_layout(C.byref(d), 1, 4000, None, 0) == 0
    assert lib.gvx_mrd_pack_weights_device(C.byref(d), None, 0, None, None) == -1


def test_default_parameter_count():
    """By hand, one resolution of the default shape (weights + biases):
    1 -> 32, (3, 9):       32 * 27 + 32            =    896
    32 -> 32, (3, 9) x 3:  3 * (32 * 32 * 27 + 32) = 83,040
    32 -> 32, (3, 3):      32 * 32 * 9 + 32        =  9,248
    score, (3, 3):         32 * 9 + 1              =    289"""
    per = 896 + 83040 + 9248 + 289
    cfg = MultiResolutionDiscriminatorConfig()
    assert cfg.parameter_count() == 3 * per == 280419 == MR.parameter_count(MR.DEFAULT) and cfg.min_samples == 905 == MR.min_samples(MR.DEFAULT)
    assert cfg.layer_shapes() == MR.layer_shapes(MR.DEFAULT)
    model = MultiResolutionDiscriminator()
    assert sum(p.numel() for p in model.parameters()) == 280419
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in MR.random_state(MR.DEFAULT, 1).items()}
    blob = _lib.load().gvx_mrd_blob_floats(C.byref(dims_from_config(cfg)))
    tables = sum(3 * n_fft + 2 for n_fft, _h, _w in cfg.resolutions)   # the window, the two twiddle tables
    assert blob % 64 == 0 and 2 * 280419 - 3 * 289 + tables <= blob < 2 * 280419 + tables + (3 * 18 + 9) * 64   # every weight twice, rounded up to 64 floats
    hann = _config(MR.HANN)
    assert hann.parameter_count() == MR.parameter_count(MR.HANN) and hann.min_samples == 225


# Default shape, p = (n_fft - hop) // 2 = 452, 904, 231: W_0 = 1 + (n + 2p - n_fft) // hop; the three strided layers each take
# W -> (W - 1) // 2 + 1; the last layer and the score keep it.
HAND = {
    905: [[7, 4, 2, 1, 1, 1], [3, 2, 1, 1, 1, 1], [18, 9, 5, 3, 3, 3]],          # 1 + 785 // 120, 1 + 665 // 240, 1 + 855 // 50
    3250: [[27, 14, 7, 4, 4, 4], [13, 7, 4, 2, 2, 2], [65, 33, 17, 9, 9, 9]],    # 1 + 3130 // 120, 1 + 3010 // 240, 1 + 3200 // 50
    8192: [[68, 34, 17, 9, 9, 9], [34, 17, 9, 5, 5, 5], [163, 82, 41, 21, 21, 21]],
}
CHANNELS = [32, 32, 32, 32, 32, 1]
BINS = (513, 1025, 257)


@pytest.mark.parametrize("n", sorted(HAND))
def test_widths_and_layout_by_hand(n):
    model = MultiResolutionDiscriminator()
    assert model.map_widths(n) == HAND[n] == MR.map_widths(MR.DEFAULT, n) == map_widths(model.model_config, n)
    lib, d = _lib.load(), model.dims()
    for B in (1, 3):
        lay = model.layout(B, n)
        at = 0
        for j, (sub, f) in enumerate(zip(lay, BINS)):
            for i, (off, c, w, ff, strides) in enumerate(sub):
                assert (off, c, w, ff) == (at, CHANNELS[i], HAND[n][j][i], f) and off % 256 == 0
                assert strides == (w * f * c, 1, f * c, c)   # channels-last storage [B][W][F][C] behind the [B, C, W, F] view
                at += (4 * B * c * w * f + 255) // 256 * 256
        assert lib.gvx_mrd_features_bytes(C.byref(d), B, n) == at
        fw, bw = lib.gvx_mrd_workspace_bytes(C.byref(d), B, n, 0), lib.gvx_mrd_workspace_bytes(C.byref(d), B, n, 1)
        mag = max((4 * B * HAND[n][j][0] * f + 255) // 256 * 256 for j, f in enumerate(BINS))   # the forward's: one spectrogram
        assert fw == mag and bw > fw and bw % 256 == 0
        assert lib.gvx_mrd_layout(C.byref(d), B, n, None, 0) == 18
    assert model.map_lengths([n, 905])[2][0] == [HAND[n][2][0], 18]


@pytest.mark.parametrize("name", sorted(MC.CFGS))
def test_widths_are_the_restatements_shapes_at_every_test_length(name):
    cfg = MC.CFGS[name]
    sd = MR.random_state(cfg, 1)
    for n in MC.LENGTHS[name]:
        with torch.no_grad():
            maps, mags = MR.discriminator(sd, MR.random_wav(1, n, 1), cfg)
        want = map_widths(_config(cfg), n)
        assert [[m.shape[2] for m in ms] for ms in maps] == want == MR.map_widths(cfg, n)
        assert [[m.shape[3] for m in ms] for ms in maps] == [[MR.bins(res)] * 6 for res in cfg["resolutions"]]
        assert [m.shape[1] for m in mags] == [w[0] for w in want]


def test_the_lengths_hold_what_the_docstring_says():
    for name, cfg in MC.CFGS.items():
        L, q = MC.LENGTHS[name], MR.min_samples(cfg)
        assert q in L and 905 in L and min(L) == q and max(L) < 4200
        widths = {n: MR.map_widths(cfg, n) for n in L}
        for j, res in enumerate(cfg["resolutions"]):
            for i in (0, 1, 2):   # the inputs of the strided layers
                assert {widths[n][j][i] % 2 for n in L} == {0, 1}, (name, j, i)
        widest = max(range(len(cfg["resolutions"])), key=lambda j: widths[max(L)][j][0])
        n = MC.CROSS[name]
        assert n in L and (widths[n][widest][0] * MR.bins(cfg["resolutions"][widest])) % MC.TILE == 1
        assert (widths[n][widest][0] * MR.bins(cfg["resolutions"][widest])) % MC.TILE_NARROW in (1, MC.TILE + 1)
        a, b, c, d = MC.PIECES[name]
        assert {a, b, c, d} <= set(L)
        assert MC.PIECE_FRAMES in [w[0] for w in widths[a]] and MC.PIECE_FRAMES + 1 in [w[0] for w in widths[b]]
        assert MC.PIECE_FRAMES in [w[1] for w in widths[c]] and MC.PIECE_FRAMES + 1 in [w[1] for w in widths[d]]
    assert MR.map_widths(MR.DEFAULT, 905)[0][3:] == [1, 1, 1] and MR.map_widths(MR.DEFAULT, 905)[1][2:] == [1, 1, 1, 1]


def test_padding_and_framing_by_hand():
    """(512, 64, 256): p = 224.  A row of 225 samples is padded to 673: frames at 0, 64, 128 (the next would end at 704).  Padded sample
    -1 - i is sample 1 + i, padded sample n + i is sample n - 2 - i; the window covers samples 128 .. 383 of a frame."""
    x = torch.arange(225.0, dtype=torch.float64)[None, :]
    padded = F.pad(x[:, None, :], (224, 224), mode="reflect")[0, 0]
    assert padded.shape == (673,) and padded[223] == 1.0 and padded[0] == 224.0 and padded[224 + 225] == 223.0 and padded[672] == 0.0
    assert MR.frames(225, (512, 64, 256)) == 3 and MR.frames(255, (512, 64, 256)) == 3 and MR.frames(256, (512, 64, 256)) == 4
    one = dict(MR.HANN, window="rectangular")
    impulse = torch.zeros(1, 400, dtype=torch.float64)
    impulse[0, 0] = 1.0   # padded position 224: inside frame 0's window [128, 384) and frame 1's [192, 448), outside frame 2's [256, 512)
    mag = MR.spectrogram(impulse, one, (512, 64, 256))
    assert mag.shape == (1, 257, 6)
    torch.testing.assert_close(mag[0, :, 0], torch.ones(257, dtype=torch.float64))
    torch.testing.assert_close(mag[0, :, 1], torch.ones(257, dtype=torch.float64))
    assert not mag[0, :, 2:].any()
    w = MR.window_of(MR.HANN, (512, 64, 256), torch.float64)
    assert w[0] == 0.0 and abs(w[128].item() - 1.0) < 1e-15 and abs(w[1].item() - w[255].item()) < 1e-15   # periodic
    z = torch.zeros(1, 400, dtype=torch.float64, requires_grad=True)
    MR.spectrogram(z, one, (512, 64, 256)).sum().backward()
    assert not z.grad.any()   # mag == 0: the gradient is exactly 0, as torch's norm backward gives


def test_size_calls_return_zero_for_refused_shapes():
    lib, d = _lib.load(), dims_from_config(MultiResolutionDiscriminatorConfig())
    for B, n in ((1, 904), (0, 4000), (65536, 4000), (1, (1 << 24) + 1)):
        assert lib.gvx_mrd_features_bytes(C.byref(d), B, n) == 0
        assert lib.gvx_mrd_workspace_bytes(C.byref(d), B, n, 1) == 0
        assert lib.gvx_mrd_layout(C.byref(d), B, n, None, 0) == 0
    assert lib.gvx_mrd_features_bytes(C.byref(d), 1, 905) > 0
    with pytest.raises(ValueError):
        MultiResolutionDiscriminator().layout(1, 904)


class _PublishedR(nn.Module):
    """The published DiscriminatorR, built independently of the restatement."""

    def __init__(self, resolution, cfg):
        super().__init__()
        wn, ch = nn.utils.weight_norm, cfg["channels"]
        self.resolution, self.slope = resolution, cfg["slope"]
        self.convs = nn.ModuleList([
            wn(nn.Conv2d(1, ch, (3, 9), padding=(1, 4))),
            wn(nn.Conv2d(ch, ch, (3, 9), stride=(1, 2), padding=(1, 4))),
            wn(nn.Conv2d(ch, ch, (3, 9), stride=(1, 2), padding=(1, 4))),
            wn(nn.Conv2d(ch, ch, (3, 9), stride=(1, 2), padding=(1, 4))),
            wn(nn.Conv2d(ch, ch, (3, 3), padding=(1, 1))),
        ])
        self.conv_post = wn(nn.Conv2d(ch, 1, (3, 3), padding=(1, 1)))

    def spectrogram(self, x):
        n_fft, hop_length, win_length = self.resolution
        x = F.pad(x, (int((n_fft - hop_length) / 2), int((n_fft - hop_length) / 2)), mode="reflect")
        x = x.squeeze(1)
        x = torch.view_as_real(torch.stft(x, n_fft=n_fft, hop_length=hop_length, win_length=win_length, center=False, return_complex=True))
        return torch.norm(x, p=2, dim=-1)

    def forward(self, x):
        fmap = []
        x = self.spectrogram(x).unsqueeze(1)
        for l in self.convs:
            x = F.leaky_relu(l(x), self.slope)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return fmap


class _PublishedMRD(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.discriminators = nn.ModuleList([_PublishedR(r, cfg) for r in cfg["resolutions"]])

    def forward(self, x):
        return [d(x) for d in self.discriminators]


def test_restatement_equals_the_published_composition_and_checkpoint_forms():
    """torch.stft without a window is the rectangular one, so the published module is the DEFAULT config; its maps are [B, C, F, W], the
    restatement's and the device's [B, C, W, F]."""
    cfg = MR.DEFAULT
    torch.manual_seed(5)
    stack = _PublishedMRD(cfg).double()
    for p in stack.parameters():
        p.data.normal_(0.0, 0.3)
    sd = stack.state_dict()
    assert any("weight_g" in k or "parametrizations" in k for k in sd)
    model = MultiResolutionDiscriminator(_config(cfg)).double()
    model.load_state_dict(sd)                                   # weight-normalised keys
    folded = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert set(folded) == set(MR.random_state(cfg, 1)) and all(folded[k].shape == v.shape for k, v in MR.random_state(cfg, 1).items())
    for n in (905, 1650):
        wav = MR.random_wav(2, n, 3)
        with torch.no_grad():
            want = stack(wav[:, None, :])
            got, _ = MR.discriminator(folded, wav, cfg)
        assert [[m.shape[2] for m in ms] for ms in got] == MR.map_widths(cfg, n) == model.map_widths(n)
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                torch.testing.assert_close(x, y.transpose(2, 3), rtol=1e-12, atol=1e-12)
    plain = MultiResolutionDiscriminator(_config(cfg)).double()
    plain.load_state_dict(folded)                                                 # a plain dict
    other = MultiResolutionDiscriminator(_config(cfg)).double()
    other.load_state_dict({"mpd": {"ignored": torch.zeros(1)}, "mrd": sd})        # the published checkpoint file
    third = MultiResolutionDiscriminator(_config(cfg)).double()
    third.load_checkpoint_statedicts(model.get_checkpoint_statedicts())           # this project's own form
    fourth = MultiResolutionDiscriminator(_config(cfg)).double()
    fourth.load_state_dict(model.get_checkpoint_statedicts())
    for m in (plain, other, third, fourth):
        for k, v in m.state_dict().items():
            assert torch.equal(v, folded[k]), k


@pytest.mark.parametrize("suffix", ["weight_orig", "weight_u"])
def test_spectral_norm_checkpoints_are_refused_by_name(suffix):
    model = MultiResolutionDiscriminator()
    sd = dict(model.state_dict())
    key = f"discriminators.1.convs.2.{suffix}"
    sd[key] = torch.zeros(3)
    with pytest.raises(ValueError, match=re.escape(key)):
        model.load_state_dict(sd)
    with pytest.raises(ValueError, match=re.escape(key)):
        model.load_state_dict({"mrd": sd})


def test_pinned_restatement_ragged_rows_and_the_silent_row():
    cfg = MR.HANN
    sd = MR.random_state(cfg, 7)
    wav = MR.random_wav(2, 700, 2)
    G = MR.random_cotangents(cfg, 2, 700, 9)
    free = MR.reference(sd, wav, None, cfg, G)
    assert MR.well_conditioned(free, cfg, 2, 700, None)
    pinned = MR.reference(sd, wav, None, cfg, G, MR.masks_from_maps(free["maps"], cfg["slope"]))
    for k in free["grads"]:
        torch.testing.assert_close(pinned["grads"][k], free["grads"][k], rtol=1e-12, atol=1e-14)
    lens = (700, 300)
    poisoned = wav.clone()
    poisoned[1, 300:] = float("nan")
    rag = MR.reference(sd, poisoned, lens, cfg, G)
    alone = [MR.reference(sd, wav[b:b + 1, :n], None, cfg, [[g[b:b + 1, :, :MR.map_widths(cfg, n)[0][i]] for i, g in enumerate(gs)] for gs in G])
             for b, n in enumerate(lens)]
    for k in sd:
        torch.testing.assert_close(rag["grads"][k], alone[0]["grads"][k] + alone[1]["grads"][k], rtol=1e-12, atol=1e-14)
    assert not rag["grads"]["wav"][1, 300:].any() and torch.equal(rag["grads"]["wav"][1, :300], alone[1]["grads"]["wav"][0])
    quiet = MR.reference(sd, MR.random_wav(2, 700, 2, silent=(1,)), None, cfg, G)
    assert not quiet["mags"][0][1].any() and not quiet["grads"]["wav"][1].any() and quiet["grads"]["wav"][0].any()
    assert not MR.well_conditioned(quiet, cfg, 2, 700, None) and MR.well_conditioned(quiet, cfg, 2, 700, None, silent=(1,))
    inner = quiet["maps"][0][0][1, :, 4:-4, 1:-1]   # away from the zero padding a silent row's first map is the bias's image
    want = F.leaky_relu(sd["discriminators.0.convs.0.bias"], cfg["slope"])
    assert inner.numel() and torch.equal(inner, want[:, None, None].expand_as(inner))


def test_calls_refuse_on_the_host():
    """Bad B and n_max, NULL arguments, no blob, short or misaligned buffers, missing gradient names: all refused before the (bogus)
    pointers are looked at."""
    lib, d = _lib.load(), dims_from_config(_config(MR.HANN))
    h = C.c_void_p()
    assert lib.gvx_mrd_create(C.byref(d), C.byref(h)) == 0
    P = 1 << 20
    fb, fw, bw = (lib.gvx_mrd_features_bytes(C.byref(d), 2, 400), lib.gvx_mrd_workspace_bytes(C.byref(d), 2, 400, 0),
                  lib.gvx_mrd_workspace_bytes(C.byref(d), 2, 400, 1))
    assert fb > 0 and fw > 0 and bw > fw
    assert lib.gvx_mrd_forward(h, P, None, 2, 400, P, fb, P, fw, None) == -7          # no blob bound
    assert lib.gvx_mrd_bind(h, 4) == -1 and lib.gvx_mrd_bind(h, None) == -1
    assert lib.gvx_mrd_bind(h, 256) == 0
    assert lib.gvx_mrd_forward(None, P, None, 2, 400, P, fb, P, fw, None) == -1
    assert lib.gvx_mrd_forward(h, None, None, 2, 400, P, fb, P, fw, None) == -1
    assert lib.gvx_mrd_forward(h, P, None, 2, 400, None, fb, P, fw, None) == -1
    assert lib.gvx_mrd_forward(h, P, None, 0, 400, P, fb, P, fw, None) == -1
    assert lib.gvx_mrd_forward(h, P, None, 65536, 400, P, 1 << 40, P, 1 << 40, None) == -1
    assert lib.gvx_mrd_forward(h, P, None, 2, 224, P, fb, P, fw, None) == -1           # HANN's reflection is 224 samples
    assert b"reflection" in lib.gvx_last_error()
    assert lib.gvx_mrd_forward(h, P, None, 2, (1 << 24) + 1, P, 1 << 40, P, 1 << 40, None) == -2
    assert lib.gvx_mrd_forward(h, P, None, 2, 400, P, fb - 1, P, fw, None) == -5
    assert lib.gvx_mrd_forward(h, P, None, 2, 400, P + 4, fb, P, fw, None) == -5
    assert lib.gvx_mrd_forward(h, P, None, 2, 400, P, fb, None, fw, None) == -5
    assert lib.gvx_mrd_forward(h, P, None, 2, 400, P, fb, P, fw - 1, None) == -5
    shapes = {k: v.numel() for k, v in MR.random_state(MR.HANN, 1).items()}
    names = list(shapes)
    table = (_lib.gvx_weight_desc * len(names))(*[_lib.gvx_weight_desc(k.encode(), P, shapes[k]) for k in names])
    back = lambda *a: lib.gvx_mrd_backward(h, P, None, *a)
    assert back(2, 224, P, P, table, len(names), P, P, bw, None) == -1
    assert back(2, 400, None, P, table, len(names), P, P, bw, None) == -1
    assert back(2, 400, P, None, table, len(names), P, P, bw, None) == -1
    assert back(2, 400, P, P, None, 0, None, P, bw, None) == -1                                  # nothing is asked for
    assert back(2, 400, P, P, None, 3, P, P, bw, None) == -1
    assert back(2, 400, P, P, table, len(names), P, P, bw - 1, None) == -5
    assert back(2, 400, P, P, table, len(names), P, None, bw, None) == -5
    assert back(2, 400, P, P, table, len(names) - 1, P, P, bw, None) == -3                       # the last bias has no destination
    assert names[-1].encode() in lib.gvx_last_error()
    table[2].numel += 1
    assert back(2, 400, P, P, table, len(names), P, P, bw, None) == -4
    assert lib.gvx_mrd_pack_weights_device(C.byref(d), table, len(names), P, None) == -4
    assert lib.gvx_mrd_pack_weights_device(C.byref(d), table, 2, P, None) == -3
    lib.gvx_mrd_destroy(h)


def test_module_refuses_on_the_host():
    model = MultiResolutionDiscriminator(_config(MR.HANN))
    assert model.min_samples == 225
    with pytest.raises(RuntimeError, match="MI355X"):
        model(torch.zeros(1, 400))
