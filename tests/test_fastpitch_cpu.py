"""CPU: the float64 restatement of FastPitch (tests/fastpitch_ref64.py) against torch's own attention and against itself row by row,
the regulator's integer plan against a numpy restatement worked by hand, the state-dict conversion and the config ranges of
``genvox_amd.fastpitch``, the C ABI's host arithmetic for refused dims, the blob's size for unequal stacks (ASYM: no energy branch, three
predictor layers; WIDE: one) against the sum over the restatement's state dict, and the tie condition of tests/test_fastpitch_gpu.py: no
token of any of the nine cases it runs has a duration inside the margin of a rounding decision."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from genvox_amd import _lib
from genvox_amd.configs import AudioConfig, FastPitchConfig, TextConfig
from genvox_amd.fastpitch import FastPitch, dims_from_config
from tests import fastpitch_ref64 as R


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.Model(getattr(R, name), seed=R.MODEL_SEED)


def _module(cfg):
    ac = AudioConfig()
    ac.n_mels = cfg["n_mels"]   # WIDE's 7 bins: below what AudioConfig's constructor takes (a mel front end's range), inside the model's [1, 4096]
    return FastPitch(FastPitchConfig(**R.model_kwargs(cfg)), ac, TextConfig(n_tokens=cfg["n_tokens"]))


@pytest.mark.parametrize("H,D,T,lens", [(1, 64, 9, None), (2, 64, 70, (70, 1, 33)), (4, 32, 17, (5, 17))])
def test_attention_equals_torch_sdpa_with_a_key_padding_mask(H, D, T, lens):
    g = torch.Generator().manual_seed(T)
    B = 1 if lens is None else len(lens)
    qkv = torch.randn(B, T, 3 * H * D, generator=g, dtype=torch.float64)
    got = R.attention_rows(qkv, lens, H, D)
    q, k, v = (t.reshape(B, T, H, D).transpose(1, 2) for t in qkv.chunk(3, dim=2))
    n = torch.tensor([T] * B if lens is None else lens)
    mask = (torch.arange(T)[None, :] < n[:, None])[:, None, None, :]   # [B, 1, 1, T]: True = the key takes part
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, T, H * D)
    for b in range(B):
        assert torch.allclose(got[b, :n[b]], want[b, :n[b]], rtol=0, atol=1e-13)
        assert not got[b, n[b]:].any()


def test_a_ragged_batch_equals_its_rows_alone():
    ref = _ref("NARROW")
    tokens = R.random_tokens(R.NARROW, 3, 9, seed=5)
    lens = (9, 1, 4)
    with torch.no_grad():
        batch = R._ragged(ref, tokens, lens, 1.0, None, None, None)
        for b, n in enumerate(lens):
            alone = R._ragged(ref, tokens[b:b + 1, :n], None, 1.0, None, None, None)
            t = alone["frames"][0]
            assert batch["frames"][b] == t
            for s, a in zip(batch["stages"][:-1], alone["stages"][:-1]):
                assert torch.equal(s[b, :a.shape[1]], a[0]) and not s[b, a.shape[1]:].any()
            assert torch.equal(batch["mel"][b, :, :t], alone["mel"][0]) and not batch["mel"][b, :, t:].any()
            assert torch.equal(batch["alignments"][b, :t, :n], alone["alignments"][0])


def _np_plan(dur, pace, least, cap):
    """The plan by hand: numpy scalars, one token after the other."""
    reps, starts, cum = [], [], 0
    for d in dur:
        r = max(int(np.floor(np.float64(d) / pace + 0.5)), least)
        end = min(cum + r, cap)
        starts.append(cum)
        reps.append(end - cum)
        cum = end
    if cum == 0:
        reps[-1] = 1
    return reps, starts


@pytest.mark.parametrize("dur,pace,least,cap,reps,starts", [
    ([0.4, 1.5, 2.49, 0.0], 1.0, 0, 2000, [0, 2, 2, 0], [0, 0, 2, 4]),          # tokens of 0 frames, a half rounds up
    ([0.4, 1.5, 2.49, 0.0], 1.0, 1, 2000, [1, 2, 2, 1], [0, 1, 3, 5]),          # min_token_frames = 1
    ([0.4, 1.5, 2.49, 0.0, 3.0], 1.0, 0, 3, [0, 2, 1, 0, 0], [0, 0, 2, 3, 3]),  # the cut at max_decoder_steps
    ([0.0, 0.2, 0.1], 1.0, 0, 2000, [0, 0, 1], [0, 0, 0]),                      # the all-zero row: one frame of its last token
    ([1.2, 0.3, 2.0], 0.5, 0, 2000, [2, 1, 4], [0, 2, 3]),                      # pace 0.5: twice as slow
    ([1.2, 0.3, 2.0, 5.0], 2.0, 0, 2000, [1, 0, 1, 3], [0, 1, 1, 2]),           # pace 2
])
def test_the_regulators_plan_equals_the_plan_by_hand(dur, pace, least, cap, reps, starts):
    assert _np_plan(dur, pace, least, cap) == (reps, starts)
    got_reps, got_starts = R.plan(torch.tensor(dur, dtype=torch.float64), pace, least, cap)
    assert got_reps.tolist() == reps and got_starts.tolist() == starts
    # ... and the regulated sequence and the alignment built from it
    align = torch.repeat_interleave(torch.eye(len(dur)), got_reps, dim=0)
    assert align.shape[0] == sum(reps) and align.sum(0).tolist() == reps


def test_state_dict_conversion_prefix_dropped_and_refused_keys():
    ref = _ref("NARROW")
    model = _module(R.NARROW)
    sd = {k: v.float() for k, v in ref.state_dict().items()}
    assert set(sd) == set(model.state_dict())
    published = {"module." + k: v for k, v in sd.items()}
    published["module.encoder.pos_emb.inv_freq"] = torch.zeros(16)
    published["module.decoder.pos_emb.inv_freq"] = torch.zeros(16)
    published["module.attention.key_proj.0.conv.weight"] = torch.zeros(4, 4, 3)
    published["module.pitch_mean"] = torch.tensor([214.7])
    published["module.pitch_std"] = torch.tensor([65.7])
    for form in ({"state_dict": published}, {"model_statedict": published}, published):
        model = _module(R.NARROW)
        model.load_checkpoint_statedicts(form)
        assert model.pitch_mean.item() == pytest.approx(214.7) and model.pitch_std.item() == pytest.approx(65.7)
        for k, v in sd.items():
            if not k.startswith("pitch_"):
                assert torch.equal(model.state_dict()[k], v), k
    assert set(model.get_checkpoint_statedicts()) == {"model_statedict"}
    with pytest.raises(ValueError, match="speaker_emb.weight"):
        _module(R.NARROW).load_state_dict({**sd, "speaker_emb.weight": torch.zeros(2, 32)})
    with pytest.raises(KeyError):
        _module(R.NARROW).load_checkpoint_statedicts({"weights": sd})
    # the packer's items: the convolutions tap-major, no buffer among them
    items = dict(model._pack_items())
    assert "pitch_mean" not in items and items["encoder.layers.0.pos_ff.CoreNet.0.weight"].shape == (64, 3, 32)
    assert model.model_name == "FastPitch" and model.text_config.n_tokens == 24 and model.audio_config.n_mels == 20


def test_load_from_config_round_trip(tmp_path):
    from genvox_amd.configs import BaseConfig

    mc = FastPitchConfig(**R.model_kwargs(R.NARROW), min_token_frames=1)
    path = str(tmp_path / "config.yaml")
    BaseConfig.write_configs_to_file(path, {"model_config": mc, "audio_config": AudioConfig(n_mels=20), "text_config": TextConfig(n_tokens=24)})
    model = FastPitch.load_from_config(path)
    assert model.model_config.to_dict() == mc.to_dict() and model.model_config.max_decoder_steps == 2000


@pytest.mark.parametrize("kwargs,word", [
    (dict(pre_lnorm=True), "pre_lnorm"), (dict(n_speakers=2), "n_speakers"), (dict(enc_d_head=48), "enc_d_head"), (dict(dec_d_head=128), "dec_d_head"),
    (dict(d_model=544), "d_model"), (dict(d_model=100), "d_model"), (dict(enc_d_inner=100), "enc_d_inner"), (dict(predictor_filter_size=1024), "predictor_filter_size"),
    (dict(enc_kernel_size=5), "enc_kernel_size"), (dict(dec_kernel_size=2), "dec_kernel_size"), (dict(dec_n_layers=0), "dec_n_layers"),
    (dict(max_decoder_steps=0), "max_decoder_steps"), (dict(min_token_frames=-1), "min_token_frames"), (dict(max_tokens=5000), "max_tokens"),
    (dict(d_model=384.0), "d_model")])
def test_config_ranges(kwargs, word):
    with pytest.raises(ValueError, match=word):
        FastPitchConfig(**kwargs)


def test_config_defaults_are_the_published_model():
    mc = FastPitchConfig()
    assert (mc.d_model, mc.enc_n_layers, mc.enc_n_head, mc.enc_d_head, mc.enc_d_inner, mc.enc_kernel_size) == (384, 6, 1, 64, 1536, 3)
    assert (mc.dec_n_layers, mc.dec_n_head, mc.dec_d_head, mc.dec_d_inner, mc.dec_kernel_size) == (6, 1, 64, 1536, 3)
    assert (mc.predictor_filter_size, mc.predictor_n_layers, mc.energy_conditioning, mc.min_token_frames, mc.max_decoder_steps) == (256, 2, True, 0, 2000)
    FastPitchConfig(enc_kernel_size=1, dec_d_head=32, energy_conditioning=False)


def _dims(**changes):
    d = dims_from_config(FastPitchConfig(), AudioConfig(), 148)
    for k, v in changes.items():
        node = d
        *path, leaf = k.split(".")
        for p in path:
            node = getattr(node, p)
        setattr(node, leaf, v)
    return d


@pytest.mark.parametrize("change,reason", [
    ({"enc.d_head": 48}, "d_head must be 32 or 64"), ({"dec.d_head": 16}, "d_head must be 32 or 64"), ({"d_model": 544}, "d_model"), ({"d_model": 48}, "d_model"),
    ({"enc.d_inner": 100}, "d_inner"), ({"pred_filter": 40}, "pred_filter"), ({"pred_filter": 1024}, "pred_filter"), ({"dec.kernel_size": 5}, "kernel_size must be 1 or 3"),
    ({"enc.kernel_size": 2}, "kernel_size must be 1 or 3"), ({"enc.n_layers": 0}, "n_layers"), ({"dec.n_head": 0}, "n_head"), ({"n_mels": 0}, "n_mels"),
    ({"n_tokens": 0}, "n_tokens"), ({"energy": 2}, "energy"), ({"max_tokens": 0}, "max_tokens"), ({"max_decoder_steps": 0}, "max_decoder_steps"),
    ({"max_duration": 0}, "max_duration"), ({"min_token_frames": -1}, "min_token_frames"), ({"pred_layers": 9}, "pred_layers")])
def test_refused_dims_give_zero_sizes_and_a_reason(change, reason):
    lib = _lib.load()
    d = _dims(**change)
    assert lib.gvx_fastpitch_blob_floats(C.byref(d)) == 0
    assert lib.gvx_fastpitch_workspace_bytes(C.byref(d), 2, 16) == 0
    h = C.c_void_p()
    assert lib.gvx_fastpitch_create(C.byref(d), C.byref(h)) == -1   # GVX_ERR_INVALID_ARG
    assert reason in lib.gvx_last_error().decode()


def test_accepted_dims_sizes_and_refused_shapes():
    lib = _lib.load()
    d = _dims()
    Cm = 384
    r = lambda n: (n + 63) // 64 * 64
    layer = r(3 * 64 * Cm) + r(3 * 64) + r(Cm * 64) + 4 * r(Cm) + r(1536 * 3 * Cm) + r(1536) + r(Cm * 3 * 1536) + r(Cm)
    pred = r(256 * 3 * Cm) + r(256 * 3 * 256) + 6 * r(256) + r(256) + r(1)
    want = r(148 * Cm) + 12 * layer + 3 * pred + 2 * (r(3 * Cm) + r(Cm)) + r(80 * Cm) + r(80) + r(2000 * Cm)
    assert lib.gvx_fastpitch_blob_floats(C.byref(d)) == want
    assert lib.gvx_fastpitch_workspace_bytes(C.byref(d), 0, 16) == 0 and lib.gvx_fastpitch_workspace_bytes(C.byref(d), 2, 0) == 0
    r256 = lambda n: (4 * n + 255) // 256 * 256
    N = 50
    per_row = 2 * r256((N + 2) * Cm) + r256(N * 192) + r256(N * 64) + r256(N * Cm) + r256((N + 2) * 1536) + 2 * r256((N + 2) * 256) + r256(N * 256) + r256(N * 80)
    assert lib.gvx_fastpitch_workspace_bytes(C.byref(d), 3, N) == 3 * per_row
    h = C.c_void_p()
    assert lib.gvx_fastpitch_create(C.byref(d), C.byref(h)) == 0
    lib.gvx_fastpitch_destroy(h)


@pytest.mark.parametrize("name", ["ASYM", "WIDE"])
def test_blob_floats_of_unequal_stacks_equal_the_sum_over_the_state_dict(name):
    """Unequal stacks, kernel sizes 1 and 3, one and three predictor layers, with and without the energy branch: the blob is every tensor of
    the restatement's state dict (each stack's layers at that stack's own sizes; no ``energy_*`` tensor without energy conditioning) and
    the position table, each rounded up to 64 floats."""
    cfg = R.full(getattr(R, name))
    sd = {k: v for k, v in _ref(name).state_dict().items() if k not in ("pitch_mean", "pitch_std")}
    r = lambda n: (n + 63) // 64 * 64
    want = sum(r(v.numel()) for v in sd.values()) + r(max(cfg["max_tokens"], cfg["max_decoder_steps"]) * cfg["d_model"])
    model = _module(getattr(R, name))
    assert _lib.load().gvx_fastpitch_blob_floats(C.byref(model.dims())) == want
    assert set(model.state_dict()) == set(_ref(name).state_dict())
    assert dict(model._pack_items()).keys() == sd.keys()
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in model.state_dict().items() if k in sd)
    has_energy = any(k.startswith("energy_") for k in model.state_dict())
    assert has_energy == cfg["energy_conditioning"] and has_energy == (name == "WIDE")
    # by hand for the tensors whose sizes differ between the stacks
    k_enc, k_dec = cfg["enc_kernel_size"], cfg["dec_kernel_size"]
    assert sd["encoder.layers.0.pos_ff.CoreNet.0.weight"].shape == (cfg["enc_d_inner"], cfg["d_model"], k_enc)
    assert sd["decoder.layers.0.pos_ff.CoreNet.2.weight"].shape == (cfg["d_model"], cfg["dec_d_inner"], k_dec)
    assert sd["decoder.layers.0.dec_attn.qkv_net.weight"].shape == (3 * cfg["dec_n_head"] * cfg["dec_d_head"], cfg["d_model"])
    assert len([k for k in sd if k.startswith("duration_predictor.layers.") and k.endswith("conv.weight")]) == cfg["predictor_n_layers"]


def test_the_one_token_case_is_decided_by_the_ulp_at_scale_not_by_the_hosts_rounding():
    """"narrow 1 x 1": each predictor's output is one number, so the float32 restatement's error on it is one draw of the host library's
    rounding.  For the token the case draws, 8 ulp at each number's scale - the term of the rule that no host changes - is at least twice
    the 90th percentile of what the encoder output's float32 error moves the number, in float64."""
    cfg_name, B, L, _ = R.CASES["narrow 1 x 1"]
    assert (B, L) == (1, 1)
    values, moved = R.one_token_movement(_ref(cfg_name), R.case_tokens("narrow 1 x 1")[0, 0])
    floor = R.FACTOR * R.ULP * values.abs()
    print(f"values {values.tolist()}, 90th percentile of the movement over 8 ulp at scale {(moved / floor).tolist()}")
    assert (2.0 * moved <= floor).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_no_token_of_a_gpu_case_lies_inside_the_margin_of_a_rounding_decision(name):
    """The tie condition: for the restatement, with the weights and seeds tests/test_fastpitch_gpu.py uses, the float64
    ``dur / pace + 0.5`` of every token is farther from an integer than 8 x max(float32 restatement's error on dur, one ulp at its
    scale) - so the GPU test's exclusion of undecided tokens is empty unless the device is wrong."""
    cfg_name, B, L, lens = R.CASES[name]
    want, _, err_dur = R.reference_pair(_ref(cfg_name), R.case_tokens(name), lens)
    near = R.undecided(want, err_dur, lens)
    print(f"{name}: float32 error on dur {err_dur:.3e}, durations {want['durations'].tolist()}")
    assert not near.any(), f"{name}: tokens {near.nonzero().tolist()} lie inside the margin: choose another seed"
    assert min(want["frames"]) >= 1
