"""CPU: the UnivNet generator's definition (include/genvox_amd.h, "UnivNet generator"): symbols, the C ABI's host arithmetic, the config
and dims refusals, the parameter counts, the checkpoint forms, the packed layouts, and the two statements of the location-variable
convolution in tests/univnet_ref64.py against each other.  Nothing here touches a GPU."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import genvox_amd
from genvox_amd import _lib, build
from genvox_amd.configs import AudioConfig, BaseConfig, UnivNetConfig
from genvox_amd.univnet import UnivNetGenerator, device_order, dims_from_config, tconv_phase_taps
from tests import univnet_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gvx_univnet_blob_floats", "gvx_univnet_workspace_bytes", "gvx_univnet_pack_weights_device", "gvx_univnet_create",
           "gvx_univnet_destroy", "gvx_univnet_bind", "gvx_univnet_forward", "gvx_univnet_timing_enable", "gvx_univnet_stage_times_ms",
           "gvx_lvc_gated"]


def _audio(cfg):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = R.hop_of(cfg), cfg["n_mels"]   # a vocoder of hop 4 or 32 is a test's size
    return ac


def _model(cfg):
    return UnivNetGenerator(UnivNetConfig(**R.model_kwargs(cfg)), _audio(cfg))


def _dims(cfg=R.DEFAULT, **over):
    d = dims_from_config(UnivNetConfig(**R.model_kwargs(cfg)), _audio(cfg))
    for k, v in over.items():
        if isinstance(v, tuple):
            for i, e in enumerate(v):
                getattr(d, k)[i] = e
        else:
            setattr(d, k, v)
    return d


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "genvox_amd.h")).read()
    assert "UnivNet generator" in header
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert getattr(lib, name).argtypes is not None, name
    assert [f for f, _ in _lib.gvx_univnet_dims._fields_] == ["n_mels", "noise_dim", "channel_size", "n_dilations", "dilations", "n_blocks", "strides",
                                                              "kpnet_hidden_channels", "kpnet_conv_size", "slope"]
    assert "univnet.hip" in build.SOURCES
    assert genvox_amd.UnivNetGenerator is UnivNetGenerator and genvox_amd.UnivNetConfig is UnivNetConfig
    assert UnivNetGenerator._abi == "gvx_univnet" and UnivNetGenerator.model_name == "univnet"


def test_blob_and_workspace_arithmetic_by_hand():
    lib = _lib.load()
    r = lambda n: (n + 63) // 64 * 64
    r256 = lambda n: (n + 255) // 256 * 256
    for cfg in (R.NARROW, R.MID, R.ODD, R.C16, R.DEFAULT):
        d = _dims(cfg)
        c, h, m, nd, D = cfg["channel_size"], cfg["kpnet_hidden_channels"], cfg["n_mels"], cfg["noise_dim"], len(cfg["dilations"])
        mp, np_ = (m + 3) // 4 * 4, (nd + 3) // 4 * 4
        ld = D * (6 * c * c + 2 * c)
        want = r(c * 7 * np_) + r(c) + r(7 * c) + r(1)
        for s in cfg["strides"]:
            want += r(s * c * 2 * c) + r(c) + r(h * 5 * mp) + r(h) + 6 * (r(h * 3 * h) + r(h)) + r(ld * 3 * h) + r(ld) + D * (r(c * 3 * c) + r(c))
        assert lib.gvx_univnet_blob_floats(C.byref(d)) == want, cfg
        hop = R.hop_of(cfg)
        for B, T in ((1, 4), (3, 33), (2, 70)):
            ws = B * (r256(4 * T * mp) + r256(4 * (T + 6) * np_) + 3 * r256(4 * T * h) + r256(4 * (T + 2) * h) + r256(4 * T * ld)
                      + 3 * r256(4 * T * hop * c))
            assert lib.gvx_univnet_workspace_bytes(C.byref(d), B, T) == ws, (cfg, B, T)
        assert lib.gvx_univnet_workspace_bytes(C.byref(d), 0, 5) == 0 and lib.gvx_univnet_workspace_bytes(C.byref(d), 1, 0) == 0
    # c32 with 100 mels: 199,312 bytes per frame and row - 99,328 of them the predicted kernels - and the halos' 6 x 256 + 2 x 256
    d = _dims()
    assert 4 * 4 * (6 * 32 * 32 + 64) == 99328
    assert lib.gvx_univnet_workspace_bytes(C.byref(d), 1, 64) == 64 * 199312 + 6 * 256 + 2 * 256
    assert lib.gvx_univnet_workspace_bytes(C.byref(d), 1, 1 << 16) > 0 and lib.gvx_univnet_workspace_bytes(C.byref(d), 1, (1 << 16) + 1) == 0


@pytest.mark.parametrize("over", [dict(n_mels=0), dict(noise_dim=0), dict(noise_dim=1025), dict(channel_size=0), dict(channel_size=18),
                                  dict(channel_size=36), dict(channel_size=64), dict(n_dilations=0), dict(n_dilations=9), dict(dilations=(1, 0)),
                                  dict(dilations=(37,)), dict(n_blocks=0), dict(n_blocks=5), dict(strides=(8, 7)), dict(strides=(0,)),
                                  dict(strides=(66,)), dict(strides=(64, 64, 2)), dict(kpnet_hidden_channels=48), dict(kpnet_hidden_channels=0),
                                  dict(kpnet_hidden_channels=288), dict(kpnet_conv_size=5), dict(slope=-0.1), dict(slope=1.5)])
def test_every_dims_field_is_checked(over):
    lib = _lib.load()
    good = _dims()
    assert lib.gvx_univnet_blob_floats(C.byref(good)) > 0
    bad = _dims(**over)
    assert lib.gvx_univnet_blob_floats(C.byref(bad)) == 0
    assert lib.gvx_univnet_workspace_bytes(C.byref(bad), 1, 8) == 0
    h = C.c_void_p()
    assert lib.gvx_univnet_create(C.byref(bad), C.byref(h)) == -1 and not h.value   # GVX_ERR_INVALID_ARG
    assert lib.gvx_univnet_create(C.byref(good), C.byref(h)) == 0 and h.value
    lib.gvx_univnet_destroy(h)


def test_config_defaults_refusals_and_file_round_trip(tmp_path):
    base = UnivNetConfig()
    assert (base.noise_dim, base.channel_size, base.dilations, base.strides, base.lReLU_slope, base.kpnet_conv_size, base.kpnet_hidden_channels,
            base.tail_pad_frames, base.tail_pad_value) == (64, 32, [1, 3, 9, 27], [8, 8, 4], 0.2, 3, 64, 10, -11.5129)
    assert base.hop == 256 and UnivNetConfig(channel_size=16).channel_size == 16
    for fields, message in [(dict(noise_dim=0), "noise_dim"), (dict(channel_size=18), "channel_size"), (dict(channel_size=64), "channel_size"),
                            (dict(dilations=()), "dilations"), (dict(dilations=(1, 37)), "dilation"), (dict(strides=()), "strides"),
                            (dict(strides=(8, 8, 8, 8, 2)), "strides"), (dict(strides=(8, 5)), "odd stride's output_padding"),
                            (dict(strides=(66,)), "stride"), (dict(strides=(64, 64, 2)), "4096"), (dict(kpnet_hidden_channels=48), "kpnet_hidden_channels"),
                            (dict(kpnet_conv_size=5), "kpnet_conv_size"), (dict(lReLU_slope=1.5), "lReLU_slope"), (dict(tail_pad_frames=-1), "tail_pad_frames"),
                            (dict(dilations="a"), "sequences")]:
        with pytest.raises(ValueError, match=message):
            UnivNetConfig(**fields)
    with pytest.raises(TypeError):
        UnivNetConfig(n_mel_channels=100)
    with pytest.raises(ValueError, match="hop_length"):
        UnivNetGenerator(UnivNetConfig(), _audio(dict(strides=(8, 8, 8), n_mels=100)))
    path = str(tmp_path / "c.yaml")
    mid = UnivNetConfig(**R.model_kwargs(R.MID))
    BaseConfig.write_configs_to_file(path, {"model_config": mid, "audio_config": AudioConfig()})
    assert BaseConfig.load_configs_from_file(path, {"model_config": UnivNetConfig})["model_config"].to_dict() == mid.to_dict()
    BaseConfig.write_configs_to_file(path, {"model_config": UnivNetConfig(channel_size=16), "audio_config": AudioConfig()})
    loaded = UnivNetGenerator.load_from_config(path)
    assert isinstance(loaded, UnivNetGenerator) and loaded.model_config.channel_size == 16


def test_parameter_and_multiply_add_counts():
    for cfg in (R.NARROW, R.MID, R.ODD, R.C16, R.DEFAULT):
        ref, model = R.Generator(cfg), _model(cfg)
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    count = lambda cfg: sum(p.numel() for p in _model(cfg).parameters())
    by_hand = 0
    c, h, m, nd, D = 32, 64, 100, 64, 4
    by_hand += c * nd * 7 + c + c * 7 + 1
    for s in (8, 8, 4):
        by_hand += c * c * 2 * s + c + D * (c * c * 3 + c) + (h * m * 5 + h) + 6 * (h * h * 3 + h) + (h * 3 + 1) * (6 * c * c * D + 2 * c * D)
    assert count(R.DEFAULT) == by_hand == 14_789_153
    assert count(R.C16) == 3_977_009
    # multiply-adds per mel frame, c32: the three kernel_conv products, the LVCs, the dilated and the transposed convolutions
    cums = (8, 64, 256)
    assert 3 * (3 * h) * (6 * c * c * D) == 14_155_776                             # "about 14.6 M" with bias_conv and the residual pairs
    assert 3 * ((3 * h) * (6 * c * c * D + 2 * c * D) + 6 * 3 * h * h + 5 * m * h) == 14_620_416
    assert sum(cum * D * (3 * c) * (2 * c) for cum in cums) == 8_060_928          # the LVCs: 8.1 M
    assert sum(cum * D * 3 * c * c for cum in cums) == 4_030_464                   # the dilated convolutions: 4.0 M
    assert sum(cum * 2 * c * c for cum in cums) == 671_744                         # the transposed convolutions: two taps per output, 0.7 M


def test_lvc_forms_agree_with_each_other_to_1e_12():
    """The unfold + einsum form against the loop over the definition: several frames (a frame boundary inside the row), one frame (both
    row ends in one window), one position per frame, and kernels that are zero everywhere but in ONE frame - the result may change at
    that frame's positions only, by that frame's weights."""
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    for B, C_, T, cum in ((2, 4, 3, 5), (1, 3, 1, 7), (1, 2, 4, 1), (1, 4, 2, 8)):
        y, k, b = rnd(B, C_, T * cum), rnd(B, C_, 2 * C_, 3, T), rnd(B, 2 * C_, T)
        a, l = R.lvc_einsum(y, k, b), R.lvc_loops(y, k, b)
        assert a.shape == l.shape == (B, 2 * C_, T * cum)
        assert (a - l).abs().max().item() < 1e-12
    y, k, b = rnd(1, 4, 15), torch.zeros(1, 4, 8, 3, 3, dtype=torch.float64), torch.zeros(1, 8, 3, dtype=torch.float64)
    k[..., 1] = rnd(1, 4, 8, 3)
    for form in (R.lvc_einsum, R.lvc_loops):
        o = form(y, k, b)
        assert not o[:, :, :5].any() and not o[:, :, 10:].any() and o[:, :, 5:10].abs().min().item() > 0
        # frame 1's first position reads y[4], a position of frame 0, under frame 1's weights; its last reads y[10]
        want = sum(k[0, :, :, t, 1].t() @ y[0, :, 5 + t - 1] for t in range(3))
        assert (o[0, :, 5] - want).abs().max().item() < 1e-12
        want = sum(k[0, :, :, t, 1].t() @ y[0, :, 9 + t - 1] for t in range(3))
        assert (o[0, :, 9] - want).abs().max().item() < 1e-12
    # the row's two ends: a zero outside [0, L)
    y, k, b = rnd(1, 2, 6), rnd(1, 2, 4, 3, 2), rnd(1, 4, 2)
    o = R.lvc_loops(y, k, b)
    assert (o[0, :, 0] - (b[0, :, 0] + k[0, :, :, 1, 0].t() @ y[0, :, 0] + k[0, :, :, 2, 0].t() @ y[0, :, 1])).abs().max().item() < 1e-12
    assert (o[0, :, 5] - (b[0, :, 1] + k[0, :, :, 0, 1].t() @ y[0, :, 4] + k[0, :, :, 1, 1].t() @ y[0, :, 5])).abs().max().item() < 1e-12
    assert (R.lvc_einsum(y, k, b) - o).abs().max().item() < 1e-12


def test_state_dict_forms_weight_norm_and_the_refusals():
    cfg = R.MID
    ref = R.Generator(cfg, seed=3)
    model = _model(cfg)
    plain = {k: v.float() for k, v in ref.state_dict().items()}
    published = {}
    g = torch.Generator().manual_seed(1)
    for k, v in plain.items():   # every layer weight-normalised, as the published checkpoint holds it
        if k.endswith(".weight"):
            scale = 0.5 + torch.rand(v.shape[0], *([1] * (v.dim() - 1)), generator=g)
            published[k[:-len("weight")] + "weight_g"] = torch.linalg.vector_norm(v.reshape(v.shape[0], -1), dim=1).reshape(scale.shape) * scale
            published[k[:-len("weight")] + "weight_v"] = v * 1.7
        else:
            published[k] = v
    model.load_checkpoint_statedicts({"model_g": published, "model_d": {}, "step": 3})
    for k, v in model.state_dict().items():
        if k.endswith(".weight"):
            want = torch._weight_norm(published[k[:-len("weight")] + "weight_v"], published[k[:-len("weight")] + "weight_g"], 0)
            assert torch.allclose(v, want, rtol=1e-6, atol=0), k
        else:
            assert torch.equal(v, plain[k]), k
    other = _model(cfg)
    other.load_checkpoint_statedicts(model.get_checkpoint_statedicts())    # our own form
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in model.state_dict().items())
    other = _model(cfg)
    other.load_checkpoint_statedicts(plain)                                 # the plain state dict
    assert all(torch.equal(v, plain[k]) for k, v in other.state_dict().items())
    with pytest.raises(KeyError, match="model_g"):
        other.load_checkpoint_statedicts({"generator": {}})
    with pytest.raises(KeyError, match=r"res_stack\.0\.kernel_predictor\.extra\.weight"):
        model.load_state_dict({**plain, "res_stack.0.kernel_predictor.extra.weight": torch.zeros(3)})
    with pytest.raises(KeyError, match="both its g and its v"):
        model.load_state_dict({**plain, "conv_pre.weight_g": torch.zeros(32, 1, 1)})
    with pytest.raises(RuntimeError, match="conv_post"):   # a missing tensor: torch's own strict refusal
        model.load_state_dict({k: v for k, v in plain.items() if not k.startswith("conv_post")})


def test_packed_layouts_round_trip_against_the_published_views():
    """device_order against the published view of kernel_conv's output; every packed convolution against torch's own convolution on
    the tensor the kernels multiply; the transposed convolution's two-tap phases against F.conv_transpose1d."""
    for c, D in ((16, 4), (32, 2), (4, 1)):
        order = device_order(c, D)
        assert sorted(order.tolist()) == list(range(6 * c * c * D))
        pub = torch.arange(6 * c * c * D).view(D, c, 2 * c, 3)         # [layer][in][out][tap]: the published view of one frame
        dev = pub.reshape(-1)[order].view(D, 2 * c, 3, c)               # [layer][out][tap][in]
        assert torch.equal(dev.permute(0, 3, 1, 2), pub)
    cfg = R.MID
    model = _model(cfg)
    items = dict(model._pack_items())
    state = model.state_dict()
    c, h, D = cfg["channel_size"], cfg["kpnet_hidden_channels"], len(cfg["dilations"])
    ld = D * (6 * c * c + 2 * c)
    assert tuple(items["conv_pre.weight"].shape) == (c, 7, 16) and tuple(items["res_stack.0.kernel_predictor.input_conv.weight"].shape) == (h, 5, 20)
    assert tuple(items["res_stack.1.kernel_predictor.kb.weight"].shape) == (ld, 3, h) and tuple(items["res_stack.1.kernel_predictor.kb.bias"].shape) == (ld,)
    assert tuple(items["conv_post.weight"].shape) == (7, c) and tuple(items["res_stack.0.conv_blocks.3.weight"].shape) == (c, 3, c)
    g = torch.Generator().manual_seed(2)
    hidden = torch.randn(1, h, 5, generator=g)
    kp = "res_stack.1.kernel_predictor."
    pub_k = F.conv1d(hidden, state[kp + "kernel_conv.weight"], state[kp + "kernel_conv.bias"], padding=1).view(1, D, c, 2 * c, 3, 5)
    pub_b = F.conv1d(hidden, state[kp + "bias_conv.weight"], state[kp + "bias_conv.bias"], padding=1).view(1, D, 2 * c, 5)
    rows = F.pad(hidden, (1, 1)).unfold(2, 3, 1)[0].permute(1, 2, 0).reshape(5, 3 * h)            # [T][tap * H + h]: the GEMM's A rows
    got = rows @ items[kp + "kb.weight"].reshape(ld, 3 * h).t() + items[kp + "kb.bias"]           # [T][ld], the device order
    dev_k = got[:, :D * 6 * c * c].view(5, D, 2 * c, 3, c)
    assert torch.allclose(dev_k.permute(1, 4, 2, 3, 0), pub_k[0], atol=1e-5)
    assert torch.allclose(got[:, D * 6 * c * c:].view(5, D, 2 * c).permute(1, 2, 0), pub_b[0], atol=1e-5)
    # the transposed convolution, s = 8 and s = 4
    for i, s in enumerate(cfg["strides"]):
        w, b = state[f"res_stack.{i}.convt_pre.1.weight"], state[f"res_stack.{i}.convt_pre.1.bias"]
        packed = items[f"res_stack.{i}.convt_pre.weight"]
        assert tuple(packed.shape) == (s, c, 2, c) and tconv_phase_taps(s).shape == (s, 2)
        x = torch.randn(1, c, 6, generator=g)
        want = F.conv_transpose1d(x, w, b, stride=s, padding=s // 2)
        xp = F.pad(x, (1, 1))
        got = torch.zeros_like(want)
        for ph in range(s):
            other = xp[0, :, 0:6] if ph < s // 2 else xp[0, :, 2:8]   # input q - 1 or q + 1
            got[0, :, ph::s] = packed[ph, :, 0] @ x[0] + packed[ph, :, 1] @ other + b[:, None]
        assert torch.allclose(got, want, atol=1e-5)


def test_min_frames_stage_shapes_noise_checks_and_vocode_with_grad_without_a_gradient():
    model = _model(R.MID)
    assert model._min_frames == 4 and model.hop == 32
    assert model.sample_counts([5, 4]) == [160, 128]
    assert model._stage_tensor_shapes(9) == [(9, 32), (72, 32), (288, 32), (288, 1)]
    mel = torch.zeros(1, 20, 4)
    with pytest.raises(RuntimeError, match="MI355X"):   # nothing asks for a gradient: it is vocode, which has no CPU path
        with torch.no_grad():
            model.vocode_with_grad(mel)
