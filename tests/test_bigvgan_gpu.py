"""GPU: the BigVGAN generator (gvx_bigvgan_forward, csrc/bigvgan.hip, through ``BigVGANGenerator``) against the float64 restatement of
tests/bigvgan_ref64.py: the waveform and x after every stage's average, element by element.

Tolerance: as tests/test_hifigan_gpu.py.  Every case evaluates the SAME restatement in float32 on the CPU and takes, tensor by tensor
(waveform, every stage), its largest distance from float64 - a number that depends on the reference alone.  The device may differ from
float64 by at most 8 times the larger of that number and one float32 ulp at the tensor's scale (2^-23 x its largest magnitude).
With random weights and a_c up to 5 the network amplifies rounding about tenfold per stage, so that number grows from 1e-5 at stage 0
to 1e-2 and more at the last stage of the published shapes: the early stages and tests/test_bigvgan_activation_gpu.py are the tight
checks, and the device stays within 0.9 - 2.2 times the restatement's own error at every stage.

Largest ratios of device error to that bound's base seen on an MI355X: see README.md, "BigVGAN"."""
import functools

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.bigvgan import BigVGANGenerator
from genvox_amd.configs import AudioConfig, BigVGANConfig
from tests import bigvgan_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23


def _build(cfg):
    if cfg["n_mels"] >= 12:
        ac = AudioConfig(n_mels=cfg["n_mels"])
    else:   # ONE_CLAMP's 5 mels are below the range of a preprocessing config, which the C ABI does not share: set on the object
        ac = AudioConfig()
        ac.n_mels = cfg["n_mels"]
    ac.hop_length = R.hop(cfg)   # below the range of a preprocessing config; a vocoder of hop 8 is a test's size
    mc = BigVGANConfig(upsample_initial_channel=cfg["c0"], upsample_rates=cfg["rates"], upsample_kernel_sizes=[2 * r for r in cfg["rates"]],
                       resblock=cfg["resblock"], resblock_kernel_sizes=cfg["kernels"], resblock_dilation_sizes=cfg["dilations"],
                       activation=cfg["activation"], snake_logscale=cfg["logscale"], use_tanh_at_final=cfg["tanh"], use_bias_at_final=cfg["bias"])
    return BigVGANGenerator(mc, ac)


@functools.lru_cache(maxsize=None)
def _net(name):
    """(the restatement's module with random weights and random alpha / beta, the device module with the same ones)."""
    cfg = getattr(R, name)
    ref = R.Generator(cfg, seed=11)
    model = _build(cfg)
    assert sum(p.numel() for p in model.parameters()) == sum(p.numel() for p in ref.parameters())
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return cfg, ref, model.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, B, T, lens):
    """(mel float64 with NaN behind every row's length, reference outputs, per-tensor float32 error of the reference): computed once."""
    cfg, ref, _ = _net(name)
    mel = R.random_mel(cfg, B, T, seed=100 * B + T)
    if lens is not None:
        for b, t in enumerate(lens):
            mel[b, :, t:] = float("nan")
    want, errs = R.reference_pair(ref, mel, lens)
    return mel, want, errs


def _run(model, mel, lens=None, ws=None):
    """-> (wav, stages [B, C, len] like the restatement's); a workspace of this call's own starts as NaN."""
    if ws is None:
        ws = torch.full((model.workspace_bytes(*mel.shape[::2]) // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    wav, stages = model.vocode(mel, lens, stage_outputs=True, workspace=ws)
    torch.cuda.synchronize()
    return wav, [s.transpose(1, 2) for s in stages]


def _compare(got, want, errs, what):
    names = ["wav"] + [f"stage {i}" for i in range(len(want[1]))]
    for name, g, w, e in zip(names, [got[0]] + list(got[1]), [want[0]] + list(want[1]), errs):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        d = (g.double().cpu() - w).abs().max().item()
        base = max(e, ULP * w.abs().max().item())
        print(f"{what}: {name}: device error {d:.3e}, float32 restatement error {e:.3e}, one ulp at scale {ULP * w.abs().max().item():.3e}, ratio {d / base:.2f}")
        assert d <= FACTOR * base, f"{what}: {name} differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"


def _check(name, B, T, lens=None):
    _, _, model = _net(name)
    mel, want, errs = _case(name, B, T, lens)
    got = _run(model, mel.to(DEV, torch.float32), lens)
    _compare(got, want, errs, f"{name} {B} x {T}" + (f" lengths {lens}" if lens else ""))
    return got


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (2, 6), (2, 7), (1, 32), (2, 33), (1, 65)])
def test_mid_sizes(B, T):
    """tests/test_hifigan_gpu.py's sizes: every convolution on the matrix kernel, the activation at 128 and 64 channels; stage 0 has
    4 T positions, so T = 1 and 2 are rows shorter than the activation's reach and T = 33 leaves a 4-position tile behind four full ones."""
    wav, _ = _check("MID", B, T)
    assert wav.abs().max().item() <= 1.0   # tanh; float32 rounds a large x to 1 exactly


@pytest.mark.parametrize("T", [1, 7, 33])
def test_narrow_sizes(T):
    """Channels 24 and 12: the activation's 32- and 16-channel blocks with idle lanes."""
    _check("NARROW", 3, T)


@pytest.mark.parametrize("T", [1, 9, 33])
def test_resblock_two_and_the_widest_window(T):
    """AMPBlock2 at 32 and 16 channels: one activation per convolution."""
    _check("TWO", 2, T)


@pytest.mark.parametrize("name,B,T", [("BASE", 1, 1), ("BASE", 2, 5), ("LARGE", 1, 2)])
def test_published_configurations(name, B, T):
    """bigvgan_base_22khz_80band and, with six stages from 1536 channels, bigvgan_22khz_80band."""
    wav, _ = _check(name, B, T)
    assert wav.abs().max().item() <= 1.0   # tanh; float32 rounds a large x to 1 exactly
    if name == "LARGE":   # its weights are not kept
        _net.cache_clear()
        _case.cache_clear()


@pytest.mark.parametrize("name", ["MID_CLAMP", "NARROW_NOBIAS", "TWO_SNAKE"])
def test_final_clamp_no_final_bias_and_plain_snake(name):
    """use_tanh_at_final = False, use_bias_at_final = False, and activation "snake" with alpha on the linear scale."""
    cfg, _, model = _net(name)
    wav, _ = _check(name, 2, 7, (7, 4))
    assert ("conv_post.bias" in model.state_dict()) == cfg["bias"]
    if not cfg["tanh"]:
        assert wav.abs().max().item() <= 1.0
        assert not wav[1, 4 * R.hop(cfg):].any()


@pytest.mark.parametrize("B,T", [(1, 1), (2, 11), (1, 22)])
@pytest.mark.parametrize("name", R.NEVER_RUN)
def test_configurations_no_published_shape_reaches(name, B, T):
    """The BigVGAN forms of tests/hifigan_ref64.py's ODD, FOUR and ONE: the activation at 72 and 36 channels, under four blocks per stage
    (the last index of the blob's activation table), and a net of 5 mels without tanh or final bias."""
    wav, _ = _check(name, B, T)
    assert wav.abs().max().item() <= 1.0


@pytest.mark.parametrize("name,lens", [("MID", (33, 1, 32, 17)), ("NARROW", (33, 1, 32, 7)), ("ODD_BETA", (22, 1, 11)), ("FOUR_SNAKE", (22, 1, 11)),
                                       ("ONE_CLAMP", (22, 1, 11))])
def test_ragged_rows_equal_the_rows_alone(name, lens):
    """Every row against the restatement of that row alone; the mel behind a row's frames is NaN, so a read past the row's end shows;
    samples and stage rows behind a row's own length are exact zeros."""
    cfg, _, model = _net(name)
    T = max(lens)
    wav, stages = _check(name, len(lens), T, lens)
    for b, t in enumerate(lens):
        assert not wav[b, t * R.hop(cfg):].any()
        mul = 1
        for r, st in zip(cfg["rates"], stages):
            mul *= r
            assert not st[b, :, t * mul:].any()
    mel = _case(name, len(lens), T, lens)[0].to(DEV, torch.float32)
    for b in (1, len(lens) - 1):   # a row of a ragged batch has the bits of that row run alone
        alone, _ = _run(model, mel[b:b + 1, :, :lens[b]].contiguous())
        assert torch.equal(alone[0], wav[b, :lens[b] * R.hop(cfg)])


@pytest.mark.parametrize("name,B,T,lens", [("MID", 2, 9, (5, 9)), ("NARROW", 3, 7, None), ("ODD_BETA", 2, 11, (5, 11)), ("FOUR_SNAKE", 2, 11, (11, 3)),
                                           ("ONE_CLAMP", 1, 22, None)])
def test_workspace_contract(name, B, T, lens):
    """Exactly the stated size, all NaN before, a NaN guard behind it that stays NaN; one byte short is refused before anything is
    written; a reused (dirty) workspace gives the same bits; stage_out changes no bit of the waveform."""
    _, _, model = _net(name)
    mel, want, errs = _case(name, B, T, lens)
    mel = mel.to(DEV, torch.float32)
    need = model.workspace_bytes(B, T)
    assert need % 256 == 0 and need > 0
    guard = 4096
    buf = torch.full(((need + guard) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    ws = buf.view(torch.uint8)[:need]
    got = _run(model, mel, lens, ws=ws)
    _compare(got, want, errs, f"{name} exact workspace")
    assert torch.isnan(buf[need // 4:]).all(), "the call wrote behind the workspace"
    again = _run(model, mel, lens, ws=ws)   # the leftovers of the first call
    assert torch.equal(again[0], got[0]) and all(torch.equal(a, b) for a, b in zip(again[1], got[1]))
    plain = model.vocode(mel, lens, workspace=ws)
    assert torch.equal(plain, got[0])
    wav = torch.full_like(got[0], 7.0)
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    before = buf.clone()
    stream = torch.cuda.current_stream().cuda_stream
    rc = lambda ws_ptr, n: _lib.load().gvx_bigvgan_forward(model._handle, mel.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, T,
                                                            wav.data_ptr(), None, ws_ptr, n, stream)
    got_rc = rc(ws.data_ptr(), need - 1)
    torch.cuda.synchronize()
    assert got_rc == -5, got_rc   # GVX_ERR_WORKSPACE
    assert (wav == 7.0).all() and torch.equal(before.view(torch.int32), buf.view(torch.int32))
    assert rc(ws.data_ptr() + 1, need) == -5   # misaligned


def test_two_calls_give_the_same_bits():
    _, _, model = _net("MID")
    mel = _case("MID", 2, 33, None)[0].to(DEV, torch.float32)
    a, b = _run(model, mel), _run(model, mel)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_python_call_split_by_rows_is_bit_equal():
    """BigVGANGenerator.vocode splits a batch by rows when the workspace would pass its cap: forced low, 4 rows run one by one."""
    cfg, _, shared = _net("MID")
    model = _build(cfg)
    model.load_state_dict(shared.state_dict())
    model.to(DEV)
    lens = (33, 1, 32, 17)
    mel = _case("MID", 4, 33, lens)[0].to(DEV, torch.float32)
    whole = model.vocode(mel, lens)
    assert model.workspace_bytes(4, 33) <= model.WORKSPACE_CAP_BYTES
    model.WORKSPACE_CAP_BYTES = model.workspace_bytes(1, 33)
    model._workspace = None
    split = model.vocode(mel, torch.tensor(lens))
    torch.cuda.synchronize()
    assert model._workspace.numel() == model.workspace_bytes(1, 33)
    assert torch.equal(whole, split)
    assert torch.equal(whole, _run(shared, mel, lens)[0])
    with torch.no_grad():
        assert torch.equal(model.vocode_with_grad(mel, lens), whole)   # nothing asks for a gradient: it is vocode
    with pytest.raises(NotImplementedError, match="backward"):
        model.vocode_with_grad(mel, lens)
    out = model.inference({"mel": mel, "mel_lengths": torch.tensor(lens)})
    assert out["lengths"].tolist() == [t * R.hop(cfg) for t in lens] and out["lengths"].dtype == torch.int32
    assert torch.equal(model({"mel": mel, "mel_lengths": lens})["waveform"], whole)
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (33, 0, 32, 17))
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (34, 1, 32, 17))


def test_stage_timing_gives_one_duration_per_part():
    _, _, model = _net("MID")
    mel = _case("MID", 2, 33, None)[0].to(DEV, torch.float32)
    model.enable_stage_timing(True)
    model.vocode(mel)
    times = model.stage_times_ms()
    model.enable_stage_timing(False)
    assert len(times) == 4 and all(t >= 0 for t in times)   # conv_pre, two stages, activation_post with conv_post
