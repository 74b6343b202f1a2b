"""CPU: the BigVGAN generator's definition (include/genvox_amd.h, "BigVGAN generator"): the anti-aliasing filter, the index form of the
activation against the padded-convolution form of tests/bigvgan_ref64.py, the config, the checkpoint forms and the C ABI's host
arithmetic.  Nothing here touches a GPU."""
import ctypes as C
import math

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.bigvgan import BigVGANGenerator, dims_from_config, kaiser_sinc_filter
from genvox_amd.configs import AudioConfig, BaseConfig, BigVGANConfig, HiFiGANConfig
from tests import bigvgan_ref64 as R

LARGE_FIELDS = dict(upsample_initial_channel=1536, upsample_rates=(4, 4, 2, 2, 2, 2), upsample_kernel_sizes=(8, 8, 4, 4, 4, 4))
SMALL1 = dict(upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4))
SMALL2 = dict(SMALL1, resblock="2", resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)), activation="snake", snake_logscale=False)


def _audio(hop=8, n_mels=12):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = hop, n_mels   # below the ranges of a preprocessing config; a vocoder of hop 8 is a test's size
    return ac


def activation_index_form(x, f, a, g):
    """The definition's index form, written out: x [C, n], f [12], a / g [C], float64 -> y [C, n]."""
    C_, n = x.shape
    u = torch.zeros(C_, 2 * n, dtype=x.dtype)
    for m in range(2 * n):
        for i in range(n + 8):
            j = m + 13 - 2 * i
            if 0 <= j <= 11:
                u[:, m] += x[:, min(max(i - 4, 0), n - 1)] * f[j]
    u = 2 * u
    z = u + g[:, None] * torch.sin(a[:, None] * u) ** 2
    y = torch.zeros(C_, n, dtype=x.dtype)
    for t in range(n):
        for j in range(12):
            y[:, t] += f[j] * z[:, min(max(2 * t + j - 5, 0), 2 * n - 1)]
    return y


def test_filter_sums_to_one_and_is_symmetric():
    f = kaiser_sinc_filter()
    assert f.dtype == torch.float64 and f.shape == (12,)
    assert abs(f.sum().item() - 1.0) < 1e-15
    assert torch.allclose(f, f.flip(0), rtol=0, atol=1e-16)
    assert torch.allclose(f, R.kaiser_sinc_filter(), rtol=0, atol=1e-14)   # torch.special.i0 here, torch.kaiser_window there


@pytest.mark.parametrize("n", [1, 2, 5, 6, 11, 40])
def test_index_form_is_the_padded_convolution_form(n):
    g_ = torch.Generator().manual_seed(n)
    x = torch.randn(3, n, generator=g_, dtype=torch.float64)
    alpha, beta = R.random_snake(3, g_, True), R.random_snake(3, g_, True)
    want = R.activation(x[None], alpha, beta)[0]
    got = activation_index_form(x, R.kaiser_sinc_filter(), alpha.exp(), 1.0 / (beta.exp() + 1e-9))
    assert got.shape == want.shape == (3, n)
    assert (got - want).abs().max().item() < 1e-13


def test_without_snake_a_constant_row_comes_back_and_a_slow_sinusoid_within_the_filter_ripple():
    f = R.kaiser_sinc_filter()
    zero, one = torch.zeros(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    for n in (1, 7, 40):
        c = torch.full((1, n), 3.25, dtype=torch.float64)
        assert (activation_index_form(c, f, one, zero) - c).abs().max().item() < 1e-14
    # up then down is linear and, away from the ends, shift invariant: with f centred (tap j at j - 5.5, F real) its response at nu
    # cycles per sample is F(pi nu)^2 + F(pi nu + pi)^2 - the baseband and the image that the decimation folds back
    nu, n = 0.05, 80
    F_ = lambda w: (f * torch.cos(w * (torch.arange(12, dtype=torch.float64) - 5.5))).sum().item()
    gain = F_(math.pi * nu) ** 2 + F_(math.pi * nu + math.pi) ** 2
    ripple = abs(gain - 1.0)
    assert 0 < ripple < 1e-2   # a low-pass at half the band passes 0.05 almost untouched
    x = torch.sin(2 * math.pi * nu * torch.arange(n, dtype=torch.float64))[None]
    y = activation_index_form(x, f, one, zero)
    assert (y - x)[:, 5:n - 5].abs().max().item() <= ripple + 1e-13
    assert (y - gain * x)[:, 5:n - 5].abs().max().item() < 1e-13
    assert (R.activation(x[None], zero, zero + 40.0)[0] - y).abs().max().item() < 1e-12   # g = exp(-40): the restatement agrees


def test_config_validation_and_from_published(tmp_path):
    base = BigVGANConfig()
    assert (base.upsample_initial_channel, tuple(base.upsample_rates), tuple(base.upsample_kernel_sizes)) == (512, (8, 8, 2, 2), (16, 16, 4, 4))
    assert (base.resblock, base.activation, base.snake_logscale, base.use_tanh_at_final, base.use_bias_at_final) == ("1", "snakebeta", True, True, True)
    assert base.hop == 256 and not hasattr(base, "leaky_slope")
    published = dict(resblock="1", num_gpus=0, batch_size=32, learning_rate=1e-4, upsample_rates=[4, 4, 2, 2, 2, 2],
                     upsample_kernel_sizes=[8, 8, 4, 4, 4, 4], upsample_initial_channel=1536, resblock_kernel_sizes=[3, 7, 11],
                     resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation="snakebeta", snake_logscale=True, num_mels=80,
                     sampling_rate=22050)
    large = BigVGANConfig.from_published(published)
    assert large.hop == 256 and large.upsample_initial_channel == 1536 and len(large.upsample_rates) == 6
    lib = _lib.load()
    assert lib.gvx_bigvgan_blob_floats(C.byref(dims_from_config(large, AudioConfig()))) > 112_000_000   # six stages are admitted
    base2 = BigVGANConfig.from_published(dict(published, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512))
    assert base2.to_dict() == base.to_dict()
    path = str(tmp_path / "c.yaml")
    BaseConfig.write_configs_to_file(path, {"model_config": large, "audio_config": AudioConfig()})
    assert BaseConfig.load_configs_from_file(path, {"model_config": BigVGANConfig})["model_config"].to_dict() == large.to_dict()
    for fields, message in [(dict(activation="relu"), "activation"), (dict(snake_logscale=1), "snake_logscale"), (dict(use_tanh_at_final="yes"), "use_tanh"),
                            (dict(upsample_rates=(8, 3), upsample_kernel_sizes=(16, 6)), "even"), (dict(resblock="3"), "resblock"),
                            (dict(resblock_kernel_sizes=(3, 7, 13)), "odd and in"), (dict(upsample_initial_channel=24), "multiple of 4")]:
        with pytest.raises(ValueError, match=message):
            BigVGANConfig(**fields)
        if "activation" not in fields and "snake_logscale" not in fields and "use_tanh_at_final" not in fields:
            with pytest.raises(ValueError, match=message):   # the structural checks are HiFiGANConfig's own
                HiFiGANConfig(**fields)
    with pytest.raises(TypeError):
        BigVGANConfig(leaky_slope=0.1)
    with pytest.raises(ValueError, match="hop_length"):
        BigVGANGenerator(BigVGANConfig(**SMALL1), _audio(hop=16))


def _published_state(model: BigVGANGenerator, seed: int, filters: bool = True):
    """A state dict as the published implementation saves it: weight-normalised layers (g, v), alpha / beta, and the filter buffers."""
    g_ = torch.Generator().manual_seed(seed)
    f = kaiser_sinc_filter().float().view(1, 1, 12)
    sd, plain = {}, {}
    for k, v in model.state_dict().items():
        v = torch.randn(v.shape, generator=g_) * 0.3
        if k.endswith(".weight"):
            norm = torch.linalg.vector_norm(v.reshape(v.shape[0], -1), dim=1).reshape(-1, *([1] * (v.dim() - 1)))
            gain = torch.rand(v.shape[0], *([1] * (v.dim() - 1)), generator=g_) + 0.5
            sd[k + "_g"], sd[k + "_v"] = gain, v
            plain[k] = v * (gain / norm)
        else:
            sd[k] = plain[k] = v
        if filters and k.endswith(".act.alpha"):
            name = k[:-len(".act.alpha")]
            sd[name + ".upsample.filter"], sd[name + ".downsample.lowpass.filter"] = f.clone(), f.clone()
    return sd, plain


@pytest.mark.parametrize("fields", [SMALL1, SMALL2, dict(SMALL1, use_bias_at_final=False)], ids=["amp1-snakebeta", "amp2-snake", "no-final-bias"])
def test_state_dict_round_trip(fields):
    mc = BigVGANConfig(**fields)
    model = BigVGANGenerator(mc, _audio())
    keys = set(model.state_dict())
    assert "ups.0.0.weight" in keys and "activation_post.act.alpha" in keys and "resblocks.3.activations.0.act.alpha" in keys
    assert ("activation_post.act.beta" in keys) == (mc.activation == "snakebeta")
    assert ("conv_post.bias" in keys) == mc.use_bias_at_final
    assert not any("filter" in k for k in keys)
    start = 0.0 if mc.snake_logscale else 1.0
    assert all((v == start).all() for k, v in model.state_dict().items() if ".act." in k)
    sd, plain = _published_state(model, seed=3)
    model.load_state_dict(sd)
    got = model.state_dict()
    assert set(got) == keys
    for k in keys:
        assert torch.allclose(got[k], plain[k], rtol=1e-6, atol=1e-7), k
    model.load_checkpoint_statedicts({"generator": sd})                       # the published file's form
    model.load_checkpoint_statedicts(model.get_checkpoint_statedicts())      # and our own
    with pytest.raises(KeyError):
        model.load_checkpoint_statedicts({"weights": sd})
    bad_key = "resblocks.1.activations.0.downsample.lowpass.filter"
    bad = dict(sd)
    bad[bad_key] = sd[bad_key].clone()
    bad[bad_key][0, 0, 4] += 1e-5
    with pytest.raises(ValueError, match=bad_key.replace(".", r"\.")):
        model.load_state_dict(bad)
    ok = dict(sd)
    ok[bad_key] = sd[bad_key].clone()
    ok[bad_key][0, 0, 4] += 5e-7   # within 1e-6
    model.load_state_dict(ok)


def test_pack_items_name_what_the_packer_reads():
    model = BigVGANGenerator(BigVGANConfig(**dict(SMALL1, use_bias_at_final=False, snake_logscale=False)), _audio())
    with torch.no_grad():
        model.activation_post.act.alpha.fill_(2.0)
        model.activation_post.act.beta.fill_(4.0)
    items = dict(model._pack_items())
    assert "ups.1.weight" in items and "ups.1.0.weight" not in items
    assert items["conv_post.bias"].shape == (1,) and not items["conv_post.bias"].any()
    assert torch.equal(items["filter"], kaiser_sinc_filter())
    assert (items["activation_post.a"] == 2.0).all() and torch.allclose(items["activation_post.g"], torch.full((8,), 0.25))
    assert items["activation_post.a"].dtype == torch.float32 and "resblocks.5.activations.5.g" in items
    assert not any(".act." in k for k in items)


def test_blob_floats_and_workspace_bytes_are_host_arithmetic():
    lib = _lib.load()
    r64 = lambda v: (v + 63) // 64 * 64
    r256 = lambda v: (v + 255) // 256 * 256
    for fields, ac in [(SMALL1, _audio()), (SMALL2, _audio()), ({}, AudioConfig()), (LARGE_FIELDS, AudioConfig())]:
        mc = BigVGANConfig(**fields)
        d = dims_from_config(mc, ac)
        hifi = HiFiGANConfig(**{k: getattr(mc, k) for k in BigVGANConfig._STRUCTURE})
        from genvox_amd.hifigan import dims_from_config as hifi_dims
        convs = lib.gvx_hifigan_blob_floats(C.byref(hifi_dims(hifi, ac)))
        acts, c = 0, mc.upsample_initial_channel
        per_block = len(mc.resblock_dilation_sizes[0]) * (2 if mc.resblock == "1" else 1)
        for _ in mc.upsample_rates:
            c //= 2
            acts += len(mc.resblock_kernel_sizes) * per_block * 2 * r64(c)
        acts += 2 * r64(c)
        assert lib.gvx_bigvgan_blob_floats(C.byref(d)) == convs + r64(12) + acts
        widest, mul, c = mc.upsample_initial_channel, 1, mc.upsample_initial_channel
        for r in mc.upsample_rates:
            mul, c = mul * r, c // 2
            widest = max(widest, mul * c)
        for B, T in [(1, 1), (3, 7), (32, 800)]:
            want = B * (r256(4 * T * ((ac.n_mels + 3) // 4 * 4)) + 5 * r256(4 * T * widest))
            assert lib.gvx_bigvgan_workspace_bytes(C.byref(d), B, T) == want
        assert lib.gvx_bigvgan_workspace_bytes(C.byref(d), 0, 4) == 0 and lib.gvx_bigvgan_workspace_bytes(C.byref(d), 1, 32769) == 0
    assert 164160 * 100 == lib.gvx_bigvgan_workspace_bytes(C.byref(dims_from_config(BigVGANConfig(), AudioConfig())), 1, 100)   # the base model's bytes per frame
    bad = dims_from_config(BigVGANConfig(), AudioConfig())
    bad.tanh_at_final = 2
    h = C.c_void_p()
    assert lib.gvx_bigvgan_blob_floats(C.byref(bad)) == 0 and lib.gvx_bigvgan_create(C.byref(bad), C.byref(h)) == -1   # GVX_ERR_INVALID_ARG
    bad = dims_from_config(BigVGANConfig(), AudioConfig())
    bad.net.upsample_rates[0] = 3
    assert lib.gvx_bigvgan_blob_floats(C.byref(bad)) == 0 and lib.gvx_bigvgan_workspace_bytes(C.byref(bad), 1, 8) == 0


def test_vocode_with_grad_says_the_backward_is_not_built():
    model = BigVGANGenerator(BigVGANConfig(**SMALL1), _audio())
    mel = torch.zeros(1, 12, 4)
    with pytest.raises(NotImplementedError, match="backward"):
        model.vocode_with_grad(mel)
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="backward"):
        model.vocode_with_grad(mel.clone().requires_grad_(True))
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):   # no gradient asked for: it is vocode, which needs the device
        model.vocode_with_grad(mel)


def test_parameter_count_is_the_restatement_modules():
    for fields, cfg in [(SMALL1, dict(R.NARROW, c0=32)), (SMALL2, dict(R.NARROW, c0=32, resblock="2", kernels=(3, 5), dilations=((1, 2), (2, 6)), activation="snake"))]:
        model = BigVGANGenerator(BigVGANConfig(**fields), _audio())
        want = R.Generator(cfg, seed=0)
        assert sum(p.numel() for p in model.parameters()) == sum(p.numel() for p in want.parameters())
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in want.state_dict().items()}
