"""CPU: the MelGAN restatement's own properties, the config, weight-norm folding, and the host arithmetic of the C ABI (no GPU call)."""
import ctypes as C
import os

import pytest
import torch
import yaml

from genvox_amd import _lib, build
from genvox_amd.configs import AudioConfig, BaseConfig, MelGANConfig
from genvox_amd.melgan import MelGANGenerator, dims_from_config, fold_weight_norm
from tests import melgan_ref64 as R

SMALL = dict(base_channels=32, upsample_ratios=(4, 2))


def _small_model():
    return MelGANGenerator(MelGANConfig(**SMALL), _audio8())


def _audio8():
    ac = AudioConfig(n_mels=12)
    ac.hop_length = 8   # below the reference's range for a preprocessing config; a vocoder of hop 8 is a test's size
    return ac


@pytest.mark.parametrize("T", [4, 5, 37])
def test_restatement_length_is_frames_times_hop(T):
    cfg = R.NARROW
    wav, stages = R.generator(R.random_state(cfg, 0), R.random_mel(cfg, 2, T, 1), cfg)
    assert wav.shape == (2, T * 8) and [s.shape for s in stages] == [(2, 16, T * 4), (2, 8, T * 8)]
    assert wav.abs().max() < 1


def test_restatement_default_sizes_and_saturation():
    cfg = R.DEFAULT
    wav, stages = R.generator(R.random_state(cfg, 0), R.random_mel(cfg, 1, 4, 1), cfg)
    assert wav.shape == (1, 1024) and stages[-1].shape == (1, 32, 1024)
    assert wav.abs().max() < 0.99 and 0.2 < wav.pow(2).mean().sqrt() < 0.5


def test_ragged_restatement_equals_rows_alone():
    cfg, lens = R.NARROW, (9, 4, 7)
    sd, mel = R.random_state(cfg, 3), R.random_mel(cfg, 3, 9, 4)
    for b, t in enumerate(lens):
        mel[b, :, t:] = float("nan")
    wav, stages = R.generator_ragged(sd, mel, lens, cfg)
    for b, t in enumerate(lens):
        w, st = R.generator(sd, mel[b:b + 1, :, :t], cfg)
        assert torch.equal(wav[b, :t * 8], w[0]) and not wav[b, t * 8:].any()
        assert torch.equal(stages[0][b, :, :t * 4], st[0][0]) and not stages[0][b, :, t * 4:].any()
    assert not torch.isnan(wav).any()


@pytest.mark.parametrize("style", ["weight_g", "parametrizations"])
def test_weight_norm_folding(style):
    """A weight-normalised layer's state dict, folded by load_state_dict, gives that layer's effective weight: Conv1d and
    ConvTranspose1d (norm over all axes but the first, which is `in` there), both spellings of the keys."""
    torch.manual_seed(0)
    model = _small_model()
    wrap = torch.nn.utils.weight_norm if style == "weight_g" else torch.nn.utils.parametrizations.weight_norm
    layers = {"pre": torch.nn.Conv1d(12, 32, 7), "ups.0": torch.nn.ConvTranspose1d(32, 16, 8, stride=4, padding=2),
              "res.1.2.mix": torch.nn.Conv1d(8, 8, 1)}
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    want = {}
    for name, layer in layers.items():
        layer = wrap(layer)
        with torch.no_grad():
            for p in layer.parameters():
                p.add_(0.3 * torch.randn_like(p))   # g no longer equals ||v||
        del sd[name + ".weight"]
        for k, v in layer.state_dict().items():
            sd[f"{name}.{k}"] = v.clone()
        if style == "weight_g":
            torch.nn.utils.remove_weight_norm(layer)
        else:
            torch.nn.utils.parametrize.remove_parametrizations(layer, "weight")
        want[name] = layer.weight.detach().clone()
    assert any(("weight_g" in k) == (style == "weight_g") and ("parametrizations" in k) == (style != "weight_g") for k in sd if "pre." in k and "bias" not in k)
    model.load_state_dict(sd)
    for name, w in want.items():
        got = model.state_dict()[name + ".weight"]
        assert got.shape == w.shape
        torch.testing.assert_close(got, w, rtol=1e-6, atol=1e-7)
    with pytest.raises(KeyError):
        fold_weight_norm({"pre.weight_g": torch.ones(3, 1, 1)})


def test_config_roundtrip_and_refusals(tmp_path):
    mc = MelGANConfig()
    assert (mc.train_repeat_discriminator, mc.max_frames, mc.feat_match, mc.learning_rate, mc.weight_decay, mc.grad_clip_thresh, mc.beta1,
            mc.beta2) == (1, 200, 10.0, 1e-4, 0, 1.0, 0.5, 0.9)   # the reference's eight fields and defaults
    assert (mc.base_channels, mc.upsample_ratios, mc.n_residual_layers, mc.dilation_base, mc.leaky_slope) == (512, [8, 8, 2, 2], 3, 3, 0.2)
    assert list(mc.to_dict())[:8] == ["train_repeat_discriminator", "max_frames", "feat_match", "learning_rate", "weight_decay",
                                      "grad_clip_thresh", "beta1", "beta2"]
    with pytest.raises(AssertionError):
        MelGANConfig(max_frames=50)
    with pytest.raises(AssertionError):
        MelGANConfig(beta1=1.5)
    path = str(tmp_path / "config.yaml")
    BaseConfig.write_configs_to_file(path, {"model_config": MelGANConfig(base_channels=64, upsample_ratios=(4, 4, 4, 4)), "audio_config": AudioConfig()})
    model = MelGANGenerator.load_from_config(path)
    assert model.model_config.upsample_ratios == [4, 4, 4, 4] and model.model_config.base_channels == 64 and model.hop == 256
    assert model.model_name == "melgan" and model.state_dict()["ups.0.weight"].shape == (64, 32, 8)
    # a yaml written from the reference's MelGANConfig: its eight fields only
    ref = {"model_config": dict(train_repeat_discriminator=2, max_frames=300, feat_match=10.0, learning_rate=1e-4, weight_decay=0,
                                grad_clip_thresh=1.0, beta1=0.5, beta2=0.9), "audio_config": AudioConfig().to_dict()}
    with open(path, "w") as f:
        yaml.dump(ref, f, sort_keys=False)
    model = MelGANGenerator.load_from_config(path)
    assert model.model_config.max_frames == 300 and model.model_config.upsample_ratios == [8, 8, 2, 2] and model.model_config.base_channels == 512
    assert sum(p.numel() for p in model.parameters()) == 4260257   # worked by hand from the definition
    with pytest.raises(ValueError, match="even"):
        MelGANConfig(upsample_ratios=(8, 8, 4, 1))
    with pytest.raises(ValueError, match="even"):
        MelGANConfig(upsample_ratios=(8, 8, 3, 2))
    with pytest.raises(ValueError, match="divisible"):
        MelGANConfig(base_channels=72)
    with pytest.raises(ValueError, match="hop_length"):
        MelGANGenerator(MelGANConfig(upsample_ratios=(8, 8, 2)), AudioConfig())
    lib, bad = _lib.load(), dims_from_config(MelGANConfig(), AudioConfig())
    bad.ratios[2] = 3
    h = C.c_void_p()
    assert lib.gvx_melgan_create(C.byref(bad), C.byref(h)) == -1 and lib.gvx_melgan_blob_floats(C.byref(bad)) == 0
    assert lib.gvx_melgan_workspace_bytes(C.byref(bad), 1, 8) == 0


def test_workspace_bytes_is_host_arithmetic():
    """Monotone in B and T, linear in B, the header's formula; no device is touched (this test runs without one)."""
    lib = _lib.load()
    for mc, ac in ((MelGANConfig(), AudioConfig()), (MelGANConfig(**SMALL), _audio8())):
        d = dims_from_config(mc, ac)
        f = lambda B, T: lib.gvx_melgan_workspace_bytes(C.byref(d), B, T)
        widest, mul, c = mc.base_channels, 1, mc.base_channels
        for r in mc.upsample_ratios:
            mul, c = mul * r, c // 2
            widest = max(widest, mul * c)
        r256 = lambda n: (n + 255) // 256 * 256
        for T in (4, 5, 37, 800):
            one = f(1, T)
            assert one == r256(4 * T * ((ac.n_mels + 3) // 4 * 4)) + 3 * r256(4 * T * widest)
            assert f(1, T + 1) > one
            for B in (2, 3, 32):
                assert f(B, T) == B * one
        assert f(1, 3) == 0 and f(0, 8) == 0 and f(1, 32769) == 0   # shapes the call refuses
    assert lib.gvx_melgan_workspace_bytes(C.byref(dims_from_config(MelGANConfig(), AudioConfig())), 1, 1) == 0
    assert 98624 * 100 == lib.gvx_melgan_workspace_bytes(C.byref(dims_from_config(MelGANConfig(), AudioConfig())), 1, 100)   # the header's bytes per frame


def test_blob_floats_is_parameters_plus_stated_padding():
    lib = _lib.load()
    for mc, ac in ((MelGANConfig(), AudioConfig()), (MelGANConfig(**SMALL), _audio8()), (MelGANConfig(base_channels=32, upsample_ratios=(4, 2)), _audio10())):
        model = MelGANGenerator(mc, ac)
        sd = model.state_dict()
        r64 = lambda n: (n + 63) // 64 * 64
        total = 0
        for k, v in sd.items():
            if k.endswith("mix.weight"):
                continue   # side by side with the shortcut: one tensor
            n = v.numel()
            if k == "pre.weight":
                n = n // ac.n_mels * ((ac.n_mels + 3) // 4 * 4)
            if k.endswith("shortcut.weight"):
                n *= 2
            total += r64(n)
        assert model.blob_numel() == total == lib.gvx_melgan_blob_floats(C.byref(model.dims()))
        assert total >= sum(p.numel() for p in model.parameters())


def _audio10():
    ac = _audio8()
    ac.n_mels = 10
    return ac


def test_short_rows_raise_before_any_launch():
    """3 frames cannot be reflected by 3: ValueError from the Python surface; it is raised before the device is looked at."""
    model = _small_model()
    with pytest.raises(RuntimeError, match="MI355X"):
        model.vocode(torch.zeros(1, 12, 8))   # a CPU model: no fallback
    lib = _lib.load()
    d = model.dims()
    h = C.c_void_p()
    assert lib.gvx_melgan_create(C.byref(d), C.byref(h)) == 0
    one = C.c_float()
    # T = 3 is refused by the C ABI on the host as well, before the (bogus) pointers are looked at
    assert lib.gvx_melgan_bind(h, 256) == 0
    assert lib.gvx_melgan_forward(h, C.addressof(one), None, 1, 3, C.addressof(one), None, 256, 1 << 30, None) == -1
    assert b"reflection" in lib.gvx_last_error()
    lib.gvx_melgan_destroy(h)


def test_symbols_and_source_are_bound():
    assert "melgan.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "melgan.hip"))
    for name in ("gvx_melgan_blob_floats", "gvx_melgan_workspace_bytes", "gvx_melgan_pack_weights_device", "gvx_melgan_create",
                 "gvx_melgan_destroy", "gvx_melgan_bind", "gvx_melgan_forward"):
        assert name in _lib.SIGNATURES
    import genvox_amd

    assert genvox_amd.MelGANGenerator is MelGANGenerator and genvox_amd.MelGANConfig is MelGANConfig
