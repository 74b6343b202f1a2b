"""CPU: the Vocos generator's definition (include/genvox_amd.h, "Vocos generator"): symbols, the C ABI's host arithmetic, the config
and dims refusals, the checkpoint forms, and the restatement of tests/vocos_ref64.py against torch.istft.  Nothing here touches a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import genvox_amd
from genvox_amd import _lib, build
from genvox_amd.configs import AudioConfig, BaseConfig, VocosConfig
from genvox_amd.vocos import VocosGenerator, dims_from_config, hann_window
from tests import vocos_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gvx_vocos_blob_floats", "gvx_vocos_workspace_bytes", "gvx_vocos_pack_weights_device", "gvx_vocos_create", "gvx_vocos_destroy",
           "gvx_vocos_bind", "gvx_vocos_forward", "gvx_vocos_timing_enable", "gvx_vocos_stage_times_ms", "gvx_dwconv_layernorm", "gvx_istft_head",
           "gvx_istft_head_workspace_bytes"]


def _audio(cfg):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = cfg["hop_length"], cfg["n_mels"]   # a vocoder of hop 128 or 130 is a test's size
    return ac


def _model(cfg):
    return VocosGenerator(VocosConfig(**R.model_kwargs(cfg)), _audio(cfg))


def _dims(**over):
    fields = dict(n_mels=100, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256, center=1)
    fields.update(over)
    d = _lib.gvx_vocos_dims()
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "genvox_amd.h")).read()
    assert "Vocos generator" in header
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert getattr(lib, name).argtypes is not None, name
    assert "gvx_vocos_dims" in header and [f for f, _ in _lib.gvx_vocos_dims._fields_] == ["n_mels", "dim", "intermediate_dim", "num_layers", "n_fft",
                                                                                           "hop_length", "center"]
    assert "vocos.hip" in build.SOURCES and not any(s.startswith("gvx_") and "vocos" in s for s in build.SOURCES)
    assert genvox_amd.VocosGenerator is VocosGenerator and genvox_amd.VocosConfig is VocosConfig
    assert VocosGenerator._abi == "gvx_vocos" and VocosGenerator.model_name == "vocos"


def test_blob_and_workspace_arithmetic_by_hand():
    lib = _lib.load()
    r = lambda n: (n + 63) // 64 * 64
    r256 = lambda n: (n + 255) // 256 * 256
    for cfg in (R.NARROW, R.MID, R.ODD, R.DEFAULT):
        d = dims_from_config(VocosConfig(**R.model_kwargs(cfg)), _audio(cfg))
        C_, I, L, N, M = cfg["dim"], cfg["intermediate_dim"], cfg["num_layers"], cfg["n_fft"], cfg["n_mels"]
        Cp, H = (M + 3) // 4 * 4, N // 2
        want = (r(7 * C_ * Cp) + 3 * r(C_) + L * (r(7 * C_) + 4 * r(C_) + 2 * r(I * C_) + r(I)) + 2 * r(C_) + r((N + 2) * C_) + r(N + 2)
                + r(N) + r(2 * H) + r(2 * (H + 1)))
        assert lib.gvx_vocos_blob_floats(C.byref(d)) == want, cfg
        for B, T in ((1, 1), (3, 33), (2, 130)):
            ws = B * (r256(4 * (T + 6) * Cp) + 2 * r256(4 * T * C_) + r256(4 * T * I) + r256(4 * T * (N + 2)) + r256(4 * T * N))
            assert lib.gvx_vocos_workspace_bytes(C.byref(d), B, T) == ws, (cfg, B, T)
        assert lib.gvx_vocos_workspace_bytes(C.byref(d), 0, 5) == 0 and lib.gvx_vocos_workspace_bytes(C.byref(d), 1, 0) == 0
    # the default model: 18,840 bytes per frame and row, and the halo's 6 x 400
    d = _dims()
    assert lib.gvx_vocos_workspace_bytes(C.byref(d), 1, 64) == 64 * 18840 + 2400 + (256 - (70 * 400) % 256) % 256
    assert lib.gvx_istft_head_workspace_bytes(2, 5, 1024) == r256(4 * 2 * 5 * 1024) + r256(8 * 1025)
    assert lib.gvx_istft_head_workspace_bytes(2, 5, 1000) == 0


@pytest.mark.parametrize("over", [dict(n_mels=0), dict(dim=48), dict(dim=0), dict(dim=544), dict(intermediate_dim=100), dict(intermediate_dim=0),
                                  dict(num_layers=0), dict(num_layers=65), dict(n_fft=256), dict(n_fft=1000), dict(n_fft=4096), dict(hop_length=127),
                                  dict(hop_length=513), dict(hop_length=255), dict(center=2), dict(center=-1)])
def test_every_dims_field_is_checked(over):
    lib = _lib.load()
    good = _dims()
    assert lib.gvx_vocos_blob_floats(C.byref(good)) > 0
    bad = _dims(**over)
    assert lib.gvx_vocos_blob_floats(C.byref(bad)) == 0
    assert lib.gvx_vocos_workspace_bytes(C.byref(bad), 1, 8) == 0
    h = C.c_void_p()
    assert lib.gvx_vocos_create(C.byref(bad), C.byref(h)) == -1 and not h.value   # GVX_ERR_INVALID_ARG
    assert lib.gvx_vocos_create(C.byref(good), C.byref(h)) == 0 and h.value
    lib.gvx_vocos_destroy(h)


def test_config_defaults_refusals_and_file_round_trip(tmp_path):
    base = VocosConfig()
    assert (base.dim, base.intermediate_dim, base.num_layers, base.n_fft, base.hop_length, base.padding, base.layer_scale_init_value) == \
        (512, 1536, 8, 1024, 256, "center", None)
    assert base.hop == 256 and base.layer_scale == 1 / 8 and VocosConfig(layer_scale_init_value=0.5).layer_scale == 0.5
    for fields, message in [(dict(n_fft=256), "n_fft"), (dict(n_fft=1000), "n_fft"), (dict(hop_length=127), "hop_length"),
                            (dict(hop_length=600), "hop_length"), (dict(hop_length=255), "hop_length"), (dict(n_fft=512, hop_length=63), "hop_length"),
                            (dict(dim=100), "dim"), (dict(intermediate_dim=1000), "intermediate_dim"), (dict(padding="reflect"), "padding"),
                            (dict(num_layers=0), "num_layers")]:
        with pytest.raises(ValueError, match=message):
            VocosConfig(**fields)
    with pytest.raises(TypeError):
        VocosConfig(input_channels=100)
    with pytest.raises(ValueError, match="hop_length"):
        VocosGenerator(VocosConfig(), _audio(dict(hop_length=300, n_mels=100)))
    path = str(tmp_path / "c.yaml")
    odd = VocosConfig(**R.model_kwargs(R.ODD))
    BaseConfig.write_configs_to_file(path, {"model_config": odd, "audio_config": AudioConfig()})
    assert BaseConfig.load_configs_from_file(path, {"model_config": VocosConfig})["model_config"].to_dict() == odd.to_dict()


def test_parameter_count_equals_the_restatements():
    for cfg in (R.NARROW, R.ODD, R.DEFAULT):
        ref = R.Generator(cfg)
        model = _model(cfg)
        want = sum(p.numel() for p in ref.parameters())
        assert sum(p.numel() for p in model.parameters()) == want
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    C_, I, N, M = 512, 1536, 1024, 100
    by_hand = (C_ * M * 7 + C_) + 2 * C_ + 8 * ((7 * C_ + C_) + 2 * C_ + (I * C_ + I) + (C_ * I + C_) + C_) + 2 * C_ + ((N + 2) * C_ + N + 2)
    assert want == by_hand == 13_531_650
    model = _model(R.DEFAULT)
    assert model.backbone.convnext[0].gamma.detach().unique().tolist() == [1 / 8]


def test_published_keys_load_and_the_refusals():
    cfg = R.MID
    ref = R.Generator(cfg, seed=3)
    model = _model(cfg)
    published = {k: v.float() for k, v in ref.state_dict().items()}
    published["head.istft.window"] = torch.hann_window(cfg["n_fft"])
    published["feature_extractor.mel_spec.spectrogram.window"] = torch.hann_window(1024)
    published["feature_extractor.mel_spec.mel_scale.fb"] = torch.zeros(513, 100)
    model.load_checkpoint_statedicts(published)                             # the plain published state dict
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k].float()), k
    other = _model(cfg)
    other.load_checkpoint_statedicts(model.get_checkpoint_statedicts())    # our own form
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in model.state_dict().items())
    with pytest.raises(KeyError, match="model_statedict"):
        other.load_checkpoint_statedicts({"generator": {}})
    bad = dict(published)
    bad["head.istft.window"] = torch.hann_window(cfg["n_fft"], periodic=False)
    with pytest.raises(ValueError, match=r"head\.istft\.window"):
        model.load_state_dict(bad)
    bad["head.istft.window"] = torch.hann_window(cfg["n_fft"] * 2)
    with pytest.raises(ValueError, match=r"head\.istft\.window"):
        model.load_state_dict(bad)
    ada = {k: v for k, v in published.items() if not k.startswith("backbone.norm.")}
    ada["backbone.norm.scale.weight"] = torch.ones(4, cfg["dim"])
    ada["backbone.norm.shift.weight"] = torch.zeros(4, cfg["dim"])
    with pytest.raises(ValueError, match=r"backbone\.norm\.(scale|shift)\.weight"):
        model.load_state_dict(ada)
    assert torch.equal(hann_window(512), torch.hann_window(512, dtype=torch.float64))


@pytest.mark.parametrize("n_fft,hop,T", [(512, 128, 9), (1024, 256, 5), (1024, 130, 12), (2048, 1024, 2), (512, 64, 17)])
def test_center_restatement_is_torch_istft(n_fft, hop, T):
    g = torch.Generator().manual_seed(n_fft + hop + T)
    c = torch.randn(2, T, n_fft + 2, generator=g, dtype=torch.float64)
    c[..., :n_fft // 2 + 1] = 2.3 + 3.0 * c[..., :n_fft // 2 + 1]
    got = R.istft(c, n_fft, hop, "center")
    H = n_fft // 2
    mag = torch.clip(torch.exp(c[..., :H + 1]), max=100.0)
    S = torch.polar(mag, c[..., H + 1:]).transpose(1, 2)
    want = torch.istft(S, n_fft, hop, n_fft, torch.hann_window(n_fft, dtype=torch.float64), center=True)
    assert got.shape == want.shape == (2, (T - 1) * hop)
    assert (got - want).abs().max().item() < 1e-11 * max(1.0, want.abs().max().item())
    same = R.istft(c, n_fft, hop, "same")
    assert same.shape == (2, T * hop)
    shift = n_fft // 2 - (n_fft - hop) // 2   # the two paddings trim the same overlap-add differently
    assert torch.equal(same[:, shift:shift + (T - 1) * hop], got)


def test_the_envelope_is_positive_at_every_delivered_sample_for_every_allowed_corner():
    for n_fft in VocosConfig.N_FFTS:
        hops = {n_fft // 8, n_fft // 8 + 2, n_fft // 4, n_fft // 2 - 2, n_fft // 2}
        for hop in sorted(hops):
            VocosConfig(n_fft=n_fft, hop_length=hop)   # allowed
            for padding, frames in (("same", 1), ("same", 2), ("same", 9), ("center", 2), ("center", 3), ("center", 9)):
                env = R.envelope(n_fft, hop, frames, padding)
                assert env.numel() == R.sample_count(dict(hop_length=hop, padding=padding), frames)
                assert env.min().item() > 1e-3, (n_fft, hop, padding, frames, env.min().item())


def test_sample_counts_min_frames_and_the_refused_backward():
    same, center = _model(R.NARROW), _model(R.MID)
    assert (same._min_frames, center._min_frames) == (1, 2)
    assert same.sample_counts([5, 1]) == [5 * 128, 128] and center.sample_counts([5, 2]) == [4 * 256, 256]
    assert same.sample_counts(7) == 7 * 128 and center.sample_counts(7) == 6 * 256
    assert center.sample_counts(torch.tensor([5, 2], dtype=torch.int32)).tolist() == [1024, 256]
    assert same._stage_tensor_shapes(9) == [(9, 32)] * 3 + [(9, 514)]
    mel = torch.zeros(1, 80, 4, requires_grad=True)
    with pytest.raises(NotImplementedError, match="backward"):
        center.vocode_with_grad(mel)
    with pytest.raises(RuntimeError, match="MI355X"):   # nothing asks for a gradient: it is vocode, which has no CPU path
        with torch.no_grad():
            center.vocode_with_grad(mel)
