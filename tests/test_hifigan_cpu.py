"""CPU: the HiFi-GAN restatement against the published module structure, the config, the checkpoint forms and the host arithmetic of the
C ABI (no GPU call)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from genvox_amd import _lib, build
from genvox_amd.configs import AudioConfig, BaseConfig, HiFiGANConfig
from genvox_amd.hifigan import HiFiGANGenerator, dims_from_config
from tests import hifigan_ref64 as R

V3_FIELDS = dict(upsample_initial_channel=256, upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8), resblock="2",
                 resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=((1, 2), (2, 6), (3, 12)))
SMALL1 = dict(upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4))
SMALL2 = dict(SMALL1, resblock="2", resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)))


def _audio8(n_mels=12):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = 8, n_mels   # below the reference's ranges for a preprocessing config; a vocoder of hop 8 is a test's size
    return ac


def _cfg_of(mc: HiFiGANConfig, ac: AudioConfig):
    """The restatement's description of a config."""
    return dict(n_mels=ac.n_mels, c0=mc.upsample_initial_channel, rates=tuple(mc.upsample_rates), resblock=mc.resblock,
                kernels=tuple(mc.resblock_kernel_sizes), dilations=tuple(tuple(d) for d in mc.resblock_dilation_sizes),
                slope=mc.leaky_slope, post_slope=mc.post_leaky_slope)


# ---- the published implementation's module structure, written from the definition in include/genvox_amd.h with torch.nn modules
class _PubResBlock1(nn.Module):
    def __init__(self, wrap, c, k, dilations):
        super().__init__()
        self.convs1 = nn.ModuleList([wrap(nn.Conv1d(c, c, k, dilation=d, padding=(k - 1) * d // 2)) for d in dilations])
        self.convs2 = nn.ModuleList([wrap(nn.Conv1d(c, c, k, dilation=1, padding=(k - 1) // 2)) for _ in dilations])

    def forward(self, x):
        for c1, c2 in zip(self.convs1, self.convs2):
            x = x + c2(F.leaky_relu(c1(F.leaky_relu(x, 0.1)), 0.1))
        return x


class _PubResBlock2(nn.Module):
    def __init__(self, wrap, c, k, dilations):
        super().__init__()
        self.convs = nn.ModuleList([wrap(nn.Conv1d(c, c, k, dilation=d, padding=(k - 1) * d // 2)) for d in dilations])

    def forward(self, x):
        for c in self.convs:
            x = x + c(F.leaky_relu(x, 0.1))
        return x


class _PubGenerator(nn.Module):
    def __init__(self, wrap, mc: HiFiGANConfig, n_mels: int):
        super().__init__()
        self.n_k = len(mc.resblock_kernel_sizes)
        c = mc.upsample_initial_channel
        self.conv_pre = wrap(nn.Conv1d(n_mels, c, 7, padding=3))
        block = _PubResBlock1 if mc.resblock == "1" else _PubResBlock2
        self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
        for r, k in zip(mc.upsample_rates, mc.upsample_kernel_sizes):
            self.ups.append(wrap(nn.ConvTranspose1d(c, c // 2, k, stride=r, padding=(k - r) // 2)))
            c //= 2
            for kr, ds in zip(mc.resblock_kernel_sizes, mc.resblock_dilation_sizes):
                self.resblocks.append(block(wrap, c, kr, ds))
        self.conv_post = wrap(nn.Conv1d(c, 1, 7, padding=3))

    def forward(self, x):
        x = self.conv_pre(x)
        for i, up in enumerate(self.ups):
            x = up(F.leaky_relu(x, 0.1))
            xs = None
            for j in range(self.n_k):
                y = self.resblocks[i * self.n_k + j](x)
                xs = y if xs is None else xs + y
            x = xs / self.n_k
        return torch.tanh(self.conv_post(F.leaky_relu(x)))   # F.leaky_relu's default slope: 0.01


@pytest.mark.parametrize("fields", [SMALL1, SMALL2], ids=["resblock1", "resblock2"])
@pytest.mark.parametrize("style", ["weight_g", "parametrizations"])
def test_published_module_loads_and_the_restatement_is_its_forward(style, fields):
    """Names, padding, slopes and the average: a weight-normalised module of the published structure with g and v perturbed; its
    state dict loads through HiFiGANGenerator.load_state_dict, the folded weights are remove_weight_norm's, and the restatement on
    those weights is the module's own float64 forward."""
    torch.manual_seed(0)
    wrap = torch.nn.utils.weight_norm if style == "weight_g" else torch.nn.utils.parametrizations.weight_norm
    mc, ac = HiFiGANConfig(**fields), _audio8()
    pub = _PubGenerator(wrap, mc, ac.n_mels).double()
    with torch.no_grad():
        for p in pub.parameters():
            p.add_(0.3 * torch.randn_like(p))   # g no longer equals ||v||
    sd = {k: v.clone() for k, v in pub.state_dict().items()}
    assert any(("weight_g" in k) if style == "weight_g" else ("parametrizations" in k) for k in sd)
    mel = R.random_mel(_cfg_of(mc, ac), 2, 9, 5)
    with torch.no_grad():
        want_wav = pub(mel)[:, 0]
    model = HiFiGANGenerator(mc, ac).double()
    model.load_state_dict(sd)
    for m in pub.modules():
        if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
            if style == "weight_g":
                torch.nn.utils.remove_weight_norm(m)
            else:
                torch.nn.utils.parametrize.remove_parametrizations(m, "weight")
    plain = pub.state_dict()
    got = model.state_dict()
    assert set(got) == set(plain)
    for k, v in plain.items():
        assert got[k].shape == v.shape
        torch.testing.assert_close(got[k], v, rtol=1e-6, atol=1e-9)
    wav, _ = R.generator({k: v.double() for k, v in got.items()}, mel, _cfg_of(mc, ac))
    assert wav.shape == want_wav.shape == (2, 72)
    assert (wav - want_wav).abs().max().item() <= 1e-12


def test_parameter_counts_of_the_published_generators():
    ac = AudioConfig()
    count = lambda **kw: sum(p.numel() for p in HiFiGANGenerator(HiFiGANConfig(**kw), ac).parameters())
    assert count() == 13926017
    assert count(upsample_initial_channel=128) == 925985
    assert count(**V3_FIELDS) == 1462273
    for cfg, n in ((R.V1, 13926017), (R.V2, 925985), (R.V3, 1462273)):
        assert sum(v.numel() for v in R.random_state(cfg, 0).values()) == n


@pytest.mark.parametrize("name,T", [("NARROW", 1), ("NARROW", 5), ("TWO", 37)])
def test_restatement_length_is_frames_times_hop(name, T):
    cfg = getattr(R, name)
    wav, stages = R.generator(R.random_state(cfg, 0), R.random_mel(cfg, 2, T, 1), cfg)
    assert wav.shape == (2, T * R.hop(cfg))
    mul, c = 1, cfg["c0"]
    for r, s in zip(cfg["rates"], stages):
        mul, c = mul * r, c // 2
        assert s.shape == (2, c, T * mul)
    assert wav.abs().max() < 1


def test_ragged_restatement_equals_rows_alone():
    cfg, lens = R.NARROW, (9, 1, 7)
    sd, mel = R.random_state(cfg, 3), R.random_mel(cfg, 3, 9, 4)
    for b, t in enumerate(lens):
        mel[b, :, t:] = float("nan")
    wav, stages = R.generator_ragged(sd, mel, lens, cfg)
    for b, t in enumerate(lens):
        w, st = R.generator(sd, mel[b:b + 1, :, :t], cfg)
        assert torch.equal(wav[b, :t * 8], w[0]) and not wav[b, t * 8:].any()
        assert torch.equal(stages[0][b, :, :t * 4], st[0][0]) and not stages[0][b, :, t * 4:].any()
    assert not torch.isnan(wav).any()


def test_config_roundtrip_and_from_published(tmp_path):
    mc = HiFiGANConfig()
    assert (mc.upsample_initial_channel, mc.upsample_rates, mc.upsample_kernel_sizes, mc.resblock, mc.resblock_kernel_sizes,
            mc.resblock_dilation_sizes, mc.leaky_slope, mc.post_leaky_slope) == (512, [8, 8, 2, 2], [16, 16, 4, 4], "1", [3, 7, 11],
                                                                                 [[1, 3, 5]] * 3, 0.1, 0.01)
    assert mc.hop == 256
    path = str(tmp_path / "config.yaml")
    BaseConfig.write_configs_to_file(path, {"model_config": HiFiGANConfig(**V3_FIELDS), "audio_config": AudioConfig()})
    model = HiFiGANGenerator.load_from_config(path)
    assert model.model_name == "hifigan" and model.hop == 256
    assert model.model_config.to_dict() == HiFiGANConfig(**V3_FIELDS).to_dict()
    assert model.state_dict()["ups.2.weight"].shape == (64, 32, 8) and "resblocks.8.convs.1.weight" in model.state_dict()
    # a published config.json: the generator's keys among the training and audio keys, which are ignored
    published = {"resblock": "2", "num_gpus": 0, "batch_size": 16, "learning_rate": 0.0002, "adam_b1": 0.8, "adam_b2": 0.99, "lr_decay": 0.999,
                 "seed": 1234, "upsample_rates": [8, 8, 4], "upsample_kernel_sizes": [16, 16, 8], "upsample_initial_channel": 256,
                 "resblock_kernel_sizes": [3, 5, 7], "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]], "segment_size": 8192, "num_mels": 80,
                 "num_freq": 1025, "n_fft": 1024, "hop_size": 256, "win_size": 1024, "sampling_rate": 22050, "fmin": 0, "fmax": 8000,
                 "fmax_for_loss": None, "num_workers": 4, "dist_config": {"dist_backend": "nccl", "dist_url": "tcp://localhost:54321", "world_size": 1}}
    assert HiFiGANConfig.from_published(published).to_dict() == HiFiGANConfig(**V3_FIELDS).to_dict()
    assert HiFiGANConfig.from_published({"upsample_initial_channel": 128}).to_dict() == HiFiGANConfig(upsample_initial_channel=128).to_dict()
    with pytest.raises(TypeError):
        HiFiGANConfig(num_mels=80)


def _set(d, **kw):
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            arr = getattr(d, k)
            for i, e in enumerate(v):
                if isinstance(e, (list, tuple)):
                    for m, f in enumerate(e):
                        arr[i][m] = f
                else:
                    arr[i] = e
        else:
            setattr(d, k, v)
    return d


REFUSALS = [   # (what, config fields that HiFiGANConfig refuses, the message, the same change made to V1's C dims)
    ("kernel size != 2 r", dict(upsample_kernel_sizes=(16, 16, 4, 6)), "2 \\* upsample_rates", dict(upsample_kernel_sizes=[16, 16, 4, 6])),
    ("odd rate", dict(upsample_rates=(8, 8, 3, 2), upsample_kernel_sizes=(16, 16, 6, 4)), "even", dict(upsample_rates=[8, 8, 3, 2], upsample_kernel_sizes=[16, 16, 6, 4])),
    ("channels not a multiple of 4", dict(upsample_initial_channel=96), "multiple of 4", dict(upsample_initial_channel=96)),
    ("channels not divisible", dict(upsample_initial_channel=520), "multiple of 4", dict(upsample_initial_channel=520)),
    ("even resblock kernel", dict(resblock_kernel_sizes=(3, 6, 11)), "odd", dict(resblock_kernel_sizes=[3, 6, 11])),
    ("resblock kernel above 11", dict(resblock_kernel_sizes=(3, 7, 13)), "odd", dict(resblock_kernel_sizes=[3, 7, 13])),
    ("window above the cap", dict(resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 8))), "window cap", dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 8]])),
    ("resblock kind", dict(resblock="3"), "resblock", dict(resblock=3)),
    ("five resblocks", dict(resblock_kernel_sizes=(3,) * 5, resblock_dilation_sizes=((1, 3, 5),) * 5), "1 to 4", dict(n_resblocks=5)),
]


@pytest.mark.parametrize("what,fields,message,dims_change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_in_the_config_and_in_the_c_abi(what, fields, message, dims_change):
    with pytest.raises(ValueError, match=message):
        HiFiGANConfig(**fields)
    lib = _lib.load()
    good = dims_from_config(HiFiGANConfig(), AudioConfig())
    h = C.c_void_p()
    assert lib.gvx_hifigan_create(C.byref(good), C.byref(h)) == 0 and lib.gvx_hifigan_blob_floats(C.byref(good)) > 0
    lib.gvx_hifigan_destroy(h)
    bad = _set(dims_from_config(HiFiGANConfig(), AudioConfig()), **dims_change)
    h = C.c_void_p()
    assert lib.gvx_hifigan_create(C.byref(bad), C.byref(h)) == -1, what
    assert lib.gvx_last_error(), what
    assert lib.gvx_hifigan_blob_floats(C.byref(bad)) == 0 and lib.gvx_hifigan_workspace_bytes(C.byref(bad), 1, 8) == 0


def test_window_cap_admits_v3_and_hop_mismatch_is_refused():
    assert HiFiGANConfig.MAX_WINDOW == 72 == (7 - 1) * 12
    HiFiGANConfig(**V3_FIELDS)
    with pytest.raises(ValueError, match="hop_length"):
        HiFiGANGenerator(HiFiGANConfig(upsample_rates=(8, 8, 2), upsample_kernel_sizes=(16, 16, 4)), AudioConfig())
    lib = _lib.load()
    # V2 reaches 16 and 8 channels: a real configuration
    d = dims_from_config(HiFiGANConfig(upsample_initial_channel=128), AudioConfig())
    assert lib.gvx_hifigan_blob_floats(C.byref(d)) > 925985


def _widest(mc):
    widest, mul, c = mc.upsample_initial_channel, 1, mc.upsample_initial_channel
    for r in mc.upsample_rates:
        mul, c = mul * r, c // 2
        widest = max(widest, mul * c)
    return widest


def test_workspace_bytes_is_host_arithmetic():
    """Monotone in T, linear in B, the header's formula; no device is touched (this test runs without one)."""
    lib = _lib.load()
    for mc, ac in ((HiFiGANConfig(), AudioConfig()), (HiFiGANConfig(upsample_initial_channel=128), AudioConfig()), (HiFiGANConfig(**V3_FIELDS), AudioConfig()),
                   (HiFiGANConfig(**SMALL2), _audio8(10))):
        d = dims_from_config(mc, ac)
        f = lambda B, T: lib.gvx_hifigan_workspace_bytes(C.byref(d), B, T)
        r256 = lambda n: (n + 255) // 256 * 256
        for T in (1, 5, 37, 800):
            one = f(1, T)
            assert one == r256(4 * T * ((ac.n_mels + 3) // 4 * 4)) + 4 * r256(4 * T * _widest(mc)) and one % 256 == 0
            assert f(1, T + 1) > one
            for B in (2, 3, 32):
                assert f(B, T) == B * one
        assert f(1, 0) == 0 and f(0, 8) == 0 and f(1, 32769) == 0   # shapes the call refuses
    assert [_widest(HiFiGANConfig()), _widest(HiFiGANConfig(upsample_initial_channel=128)), _widest(HiFiGANConfig(**V3_FIELDS))] == [8192, 2048, 8192]
    assert 131392 * 100 == lib.gvx_hifigan_workspace_bytes(C.byref(dims_from_config(HiFiGANConfig(), AudioConfig())), 1, 100)   # V1's bytes per frame


def test_blob_floats_is_parameters_plus_stated_padding():
    lib = _lib.load()
    for mc, ac in ((HiFiGANConfig(), AudioConfig()), (HiFiGANConfig(**V3_FIELDS), AudioConfig()), (HiFiGANConfig(**SMALL1), _audio8()),
                   (HiFiGANConfig(**SMALL2), _audio8(10))):
        model = HiFiGANGenerator(mc, ac)
        r64 = lambda n: (n + 63) // 64 * 64
        total = 0
        for k, v in model.state_dict().items():
            n = v.numel()
            if k == "conv_pre.weight":
                n = n // ac.n_mels * ((ac.n_mels + 3) // 4 * 4)
            total += r64(n)
        assert model.blob_numel() == total == lib.gvx_hifigan_blob_floats(C.byref(model.dims()))
        assert total >= sum(p.numel() for p in model.parameters())


def test_bad_shapes_are_refused_on_the_host_before_any_pointer_is_read():
    model = HiFiGANGenerator(HiFiGANConfig(**SMALL1), _audio8())
    with pytest.raises(RuntimeError, match="MI355X"):
        model.vocode(torch.zeros(1, 12, 8))   # a CPU model: no fallback
    lib = _lib.load()
    d = model.dims()
    h = C.c_void_p()
    assert lib.gvx_hifigan_create(C.byref(d), C.byref(h)) == 0
    one = C.c_float()
    assert lib.gvx_hifigan_forward(h, C.addressof(one), None, 1, 4, C.addressof(one), None, 256, 1 << 30, None) == -7   # no blob bound
    assert lib.gvx_hifigan_bind(h, 256) == 0
    # T = 0 is refused on the host, before the (bogus) pointers are looked at; so are a short and a misaligned workspace
    assert lib.gvx_hifigan_forward(h, C.addressof(one), None, 1, 0, C.addressof(one), None, 256, 1 << 30, None) == -1
    assert b"frame" in lib.gvx_last_error()
    assert lib.gvx_hifigan_forward(h, C.addressof(one), None, 0, 4, C.addressof(one), None, 256, 1 << 30, None) == -1
    assert lib.gvx_hifigan_forward(h, C.addressof(one), None, 1, 32769, C.addressof(one), None, 256, 1 << 30, None) == -2
    need = lib.gvx_hifigan_workspace_bytes(C.byref(d), 1, 4)
    assert lib.gvx_hifigan_forward(h, C.addressof(one), None, 1, 4, C.addressof(one), None, 256, need - 1, None) == -5
    assert lib.gvx_hifigan_forward(h, C.addressof(one), None, 1, 4, C.addressof(one), None, 260, need, None) == -5
    lib.gvx_hifigan_destroy(h)


def test_row_lengths_outside_1_to_T_raise_before_any_launch(monkeypatch):
    model = HiFiGANGenerator(HiFiGANConfig(**SMALL1), _audio8())
    dev = torch.device("cpu")
    monkeypatch.setattr(model, "_require_gpu", lambda: dev)   # past the device check: the next thing that runs is the length check
    monkeypatch.setattr(model, "_ensure_packed", lambda: pytest.fail("a launch was prepared"))
    mel = torch.zeros(3, 12, 8)
    for lens in ((8, 0, 3), (8, 9, 3), (8, -1, 3)):
        with pytest.raises(ValueError, match="frames are outside"):
            model.vocode(mel, lens)
    with pytest.raises(ValueError, match="lengths for"):
        model.vocode(mel, (8, 3))
    with pytest.raises(ValueError, match="at least 1"):
        model.vocode(torch.zeros(1, 12, 0))


def test_checkpoint_forms(tmp_path):
    """Our {"model_statedict": ...} and the published file's {"generator": weight-normalised dict} load to the same weights."""
    torch.manual_seed(1)
    mc, ac = HiFiGANConfig(**SMALL1), _audio8()
    pub = _PubGenerator(torch.nn.utils.weight_norm, mc, ac.n_mels)
    a, b = HiFiGANGenerator(mc, ac), HiFiGANGenerator(mc, ac)
    a.load_checkpoint_statedicts({"generator": pub.state_dict()})
    b.load_checkpoint_statedicts(a.get_checkpoint_statedicts())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    torch.testing.assert_close(a.state_dict()["ups.0.weight"], pub.ups[0].weight.detach(), rtol=1e-6, atol=1e-7)
    with pytest.raises(KeyError):
        a.load_checkpoint_statedicts({"weights": {}})
    a._packed_key = "packed"
    a.load_state_dict(b.state_dict())
    assert a._packed_key is None   # a load invalidates the packed blob


def test_symbols_and_source_are_bound():
    assert "hifigan.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "hifigan.hip"))
    assert os.path.exists(os.path.join(build.CSRC, "hifigan_internal.h"))
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "genvox_amd.h")).read()
    lib = _lib.load()
    for name in ("gvx_hifigan_blob_floats", "gvx_hifigan_workspace_bytes", "gvx_hifigan_pack_weights_device", "gvx_hifigan_create",
                 "gvx_hifigan_destroy", "gvx_hifigan_bind", "gvx_hifigan_forward", "gvx_hifigan_timing_enable", "gvx_hifigan_stage_times_ms"):
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(lib, name)
    assert "gvx_hifigan_dims" in header and C.sizeof(_lib.gvx_hifigan_dims) == 4 * (3 + 8 + 8 + 3 + 4 + 12 + 2)
    import genvox_amd

    assert genvox_amd.HiFiGANGenerator is HiFiGANGenerator and genvox_amd.HiFiGANConfig is HiFiGANConfig
