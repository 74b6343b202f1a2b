"""GPU: the UnivNet generator (gvx_univnet_forward, csrc/univnet.hip, through ``UnivNetGenerator``) against the float64 restatement of
tests/univnet_ref64.py: the waveform and every stage output - x after conv_pre, after every block, and the output layer before its tanh -
element by element.  Mel and noise are NaN behind every row's length.

Tolerance: as tests/test_vocos_gpu.py.  Every case evaluates the SAME restatement in float32 on the CPU and takes, tensor by tensor, its
largest distance from float64 - a number that depends on the reference alone.  The device may differ from float64 by at most 8 times
the larger of that number and one float32 ulp at the tensor's scale (2^-23 x its largest magnitude).  The ratio is printed.

Largest ratios seen on an MI355X: see README.md, "UnivNet"."""
import functools

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.configs import AudioConfig, UnivNetConfig
from genvox_amd.univnet import UnivNetGenerator
from tests import univnet_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23


def _build(cfg):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = R.hop_of(cfg), cfg["n_mels"]   # a vocoder of hop 4 or 32 is a test's size
    return UnivNetGenerator(UnivNetConfig(**R.model_kwargs(cfg)), ac)


@functools.lru_cache(maxsize=None)
def _net(name):
    """(the restatement's module with random weights, the device module with the same ones)."""
    cfg = getattr(R, name)
    ref = R.Generator(cfg, seed=11)
    model = _build(cfg)
    assert sum(p.numel() for p in model.parameters()) == sum(p.numel() for p in ref.parameters())
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    # the restatement holds exactly what the device holds: float32 weights
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    return cfg, ref, model.to(DEV)


def _inputs(cfg, B, T, lens, seed):
    """(mel, noise) as float32 values in float64, NaN behind every row's length."""
    mel, noise = R.random_mel(cfg, B, T, seed).float().double(), R.random_noise(cfg, B, T, seed).float().double()
    if lens is not None:
        for b, t in enumerate(lens):
            mel[b, :, t:] = float("nan")
            noise[b, :, t:] = float("nan")
    return mel, noise


@functools.lru_cache(maxsize=None)
def _case(name, B, T, lens):
    """(mel, noise, reference outputs, per-tensor float32 error of the reference): computed once."""
    cfg, ref, _ = _net(name)
    mel, noise = _inputs(cfg, B, T, lens, seed=100 * B + T)
    want, errs = R.reference_pair(ref, mel, noise, lens)
    return mel, noise, want, errs


def _run(model, mel, noise, lens=None, ws=None):
    """-> (wav, stages); a workspace of this call's own starts as NaN."""
    if ws is None:
        ws = torch.full((model.workspace_bytes(*mel.shape[::2]) // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    wav, stages = model.vocode(mel, lens, stage_outputs=True, workspace=ws, noise=noise)
    torch.cuda.synchronize()
    return wav, stages


def _compare(got, want, errs, what):
    names = ["wav"] + [f"stage {i}" for i in range(len(want[1]))]
    assert len(got[1]) == len(want[1])
    for name, g, w, e in zip(names, [got[0]] + list(got[1]), [want[0]] + list(want[1]), errs):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        d = (g.double().cpu() - w).abs().max().item()
        base = max(e, ULP * w.abs().max().item())
        print(f"{what}: {name}: device error {d:.3e}, float32 restatement error {e:.3e}, one ulp at scale {ULP * w.abs().max().item():.3e}, ratio {d / base:.2f}")
        assert d <= FACTOR * base, f"{what}: {name} differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"


def _check(name, B, T, lens=None):
    cfg, _, model = _net(name)
    mel, noise, want, errs = _case(name, B, T, lens)
    got = _run(model, mel.to(DEV, torch.float32), noise.to(DEV, torch.float32), lens)
    _compare(got, want, errs, f"{name} {B} x {T}" + (f" lengths {lens}" if lens else ""))
    hop = R.hop_of(cfg)
    for b, t in enumerate(lens if lens is not None else [T] * B):   # exact zeros behind every row, in every tensor
        assert not got[0][b, t * hop:].any()
        for st in got[1]:
            assert not st[b, t * (st.shape[1] // T):].any()
    return got


@pytest.mark.parametrize("name,B,T,lens", [("NARROW", 2, 5, None), ("MID", 3, 33, (33, 4, 17)), ("ODD", 2, 7, (7, 4)), ("C16", 1, 6, None),
                                           ("DEFAULT", 1, 12, None), ("DEFAULT", 2, 70, None)])
def test_every_stage_and_the_waveform(name, B, T, lens):
    """NARROW: frames of 2 and 4 positions, the fmaf LVC at C = 32; MID ragged: the fmaf LVC at 8 positions per frame, then the
    matrix-pipe one at 32, a row of the least 4 frames; ODD: 12 channels, 10 mels, 6 noise channels, strides 6 and 2 - the least the config
    allows that is no power of two anywhere; C16: the fmaf path throughout; DEFAULT: the published c32, the matrix pipe at 64
    and 256 positions per frame, and at 2 x 70 B * T crosses a 128-row GEMM tile."""
    wav, stages = _check(name, B, T, lens)
    cfg = getattr(R, name)
    assert wav.shape == (B, T * R.hop_of(cfg)) and len(stages) == len(cfg["strides"]) + 2
    if (name, B, T) == ("DEFAULT", 2, 70):   # the large models' weights and cases are not kept
        _net.cache_clear()
        _case.cache_clear()


def test_ragged_rows_equal_the_rows_alone():
    """A row of a ragged batch has the bits of that row run alone; mel and noise behind a row's frames are NaN, so a read past the row's
    end shows."""
    cfg, _, model = _net("MID")
    lens = (33, 4, 17, 32)
    mel, noise = (t.to(DEV, torch.float32) for t in _inputs(cfg, 4, 33, lens, seed=5))
    wav, stages = _run(model, mel, noise, lens)
    assert not torch.isnan(wav).any()
    hop = R.hop_of(cfg)
    for b, t in enumerate(lens):
        alone, st = _run(model, mel[b:b + 1, :, :t].contiguous(), noise[b:b + 1, :, :t].contiguous())
        assert torch.equal(alone[0], wav[b, :t * hop]) and not wav[b, t * hop:].any()
        for one, many in zip(st, stages):
            n = one.shape[1]
            assert torch.equal(one[0], many[b, :n]) and not many[b, n:].any()


def test_python_call_split_by_rows_inference_lengths_and_the_refusals():
    cfg, _, shared = _net("MID")
    model = _build(cfg)
    model.load_state_dict(shared.state_dict())
    model.to(DEV)
    lens = (33, 4, 32, 17)
    mel, noise = (t.to(DEV, torch.float32) for t in _inputs(cfg, 4, 33, lens, seed=8))
    whole = model.vocode(mel, lens, noise=noise)
    assert model.workspace_bytes(4, 33) <= model.WORKSPACE_CAP_BYTES
    model.WORKSPACE_CAP_BYTES = model.workspace_bytes(1, 33)
    model._workspace = None
    split = model.vocode(mel, torch.tensor(lens), noise=noise)   # the noise is sliced with the rows
    torch.cuda.synchronize()
    assert model._workspace.numel() == model.workspace_bytes(1, 33)
    assert torch.equal(whole, split)
    assert torch.equal(whole, _run(shared, mel, noise, lens)[0])   # stage_out changes no bit of the waveform
    with torch.no_grad():
        assert torch.equal(model.vocode_with_grad(mel, lens, noise=noise), whole)   # nothing asks for a gradient: it is vocode
    out = model.inference({"mel": mel, "mel_lengths": torch.tensor(lens)})
    assert out["lengths"].tolist() == [t * 32 for t in lens] and out["lengths"].dtype == torch.int32
    assert out["waveform"].shape == (4, 33 * 32)
    with pytest.raises(ValueError, match="4 frames"):
        model.vocode(mel, (33, 3, 32, 17), noise=noise)   # the reflection by 3 needs 4 frames
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (34, 4, 32, 17), noise=noise)
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel[:, :, :3].contiguous())
    with pytest.raises(ValueError, match="noise"):
        model.vocode(mel, lens, noise=noise[:, :, :32])
    with pytest.raises(ValueError, match="noise"):
        model.vocode(mel, lens, noise=noise.double())
    with pytest.raises(ValueError, match="noise"):
        model.vocode(mel, lens, noise=noise.cpu())


def test_drawn_noise_repeats_under_manual_seed_and_differs_without_it():
    cfg, _, model = _net("MID")
    mel = R.random_mel(cfg, 2, 9, seed=4).float().to(DEV)
    model.manual_seed(123)
    a = model.vocode(mel)
    b = model.vocode(mel)
    model.manual_seed(123)
    c = model.vocode(mel)
    assert torch.equal(a, c) and not torch.equal(a, b)
    model.manual_seed(123)
    noise = model.draw_noise(2, 9)
    assert noise.shape == (2, cfg["noise_dim"], 9) and torch.equal(model.vocode(mel, noise=noise), a)
    model.manual_seed(124)
    assert not torch.equal(model.vocode(mel), a)


@pytest.mark.parametrize("name,B,T,lens", [("MID", 2, 9, (5, 9)), ("NARROW", 3, 7, None)])
def test_workspace_contract(name, B, T, lens):
    """Exactly the stated size, all NaN before, a NaN guard behind it that stays NaN; one byte short is refused before anything is
    written; the same workspace reused (dirty) for this shape and for another one gives the same bits."""
    _, _, model = _net(name)
    mel, noise, want, errs = _case(name, B, T, lens)
    mel, noise = mel.to(DEV, torch.float32), noise.to(DEV, torch.float32)
    need = model.workspace_bytes(B, T)
    assert need % 256 == 0 and need > 0
    guard = 4096
    buf = torch.full(((need + guard) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    ws = buf.view(torch.uint8)[:need]
    got = _run(model, mel, noise, lens, ws=ws)
    _compare(got, want, errs, f"{name} exact workspace")
    assert torch.isnan(buf[need // 4:]).all(), "the call wrote behind the workspace"
    again = _run(model, mel, noise, lens, ws=ws)   # the leftovers of the first call
    assert torch.equal(again[0], got[0]) and all(torch.equal(a, b) for a, b in zip(again[1], got[1]))
    small, small_noise = mel[B - 1:, :, :T - 2].contiguous(), noise[B - 1:, :, :T - 2].contiguous()   # another shape in the same, now dirty, workspace
    assert torch.equal(model.vocode(small, workspace=ws, noise=small_noise), _run(model, small, small_noise)[0])
    plain = model.vocode(mel, lens, workspace=ws, noise=noise)
    assert torch.equal(plain, got[0])
    wav = torch.full_like(got[0], 7.0)
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    before = buf.clone()
    stream = torch.cuda.current_stream().cuda_stream
    rc = lambda ws_ptr, n: _lib.load().gvx_univnet_forward(model._handle, mel.data_ptr(), noise.data_ptr(),
                                                            lens_dev.data_ptr() if lens_dev is not None else None, B, T, wav.data_ptr(), None, ws_ptr, n, stream)
    got_rc = rc(ws.data_ptr(), need - 1)
    torch.cuda.synchronize()
    assert got_rc == -5, got_rc   # GVX_ERR_WORKSPACE
    assert (wav == 7.0).all() and torch.equal(before.view(torch.int32), buf.view(torch.int32))
    assert rc(ws.data_ptr() + 1, need) == -5   # misaligned
    assert _lib.load().gvx_univnet_forward(model._handle, mel.data_ptr(), noise.data_ptr(), None, B, 3, wav.data_ptr(), None, ws.data_ptr(), need,
                                           stream) == -1   # 3 frames: GVX_ERR_INVALID_ARG, before anything is launched
    assert (wav == 7.0).all()


def test_two_calls_give_the_same_bits_and_a_changed_weight_repacks():
    cfg, _, shared = _net("MID")
    model = _build(cfg)
    model.load_state_dict(shared.state_dict())
    model.to(DEV)
    mel, noise = (t.to(DEV, torch.float32) for t in _inputs(cfg, 2, 33, None, seed=3))
    a, b = _run(model, mel, noise), _run(model, mel, noise)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    blob = model._blob
    with torch.no_grad():
        model.res_stack[1].kernel_predictor.bias_conv.bias.mul_(0.5)   # part of the permuted kernel_conv + bias_conv layer of block 1
    c = _run(model, mel, noise)
    assert model._blob is not blob
    assert torch.equal(c[1][1], a[1][1]) and not torch.equal(c[1][2], a[1][2]) and not torch.equal(c[0], a[0])
    with torch.no_grad():
        model.res_stack[1].kernel_predictor.bias_conv.bias.mul_(2.0)   # exact: back to the first weights
    assert torch.equal(_run(model, mel, noise)[0], a[0])


def test_stage_timing_gives_its_count_of_durations():
    cfg, _, model = _net("MID")
    mel = R.random_mel(cfg, 2, 33, seed=3).float().to(DEV)
    model.enable_stage_timing(True)
    model.vocode(mel)
    times = model.stage_times_ms()
    model.enable_stage_timing(False)
    assert len(times) == 2 * len(cfg["strides"]) + 2 and all(t >= 0 for t in times)   # conv_pre, per block predictor and layers, conv_post


def test_a_row_of_three_frames_is_refused():
    cfg, _, model = _net("NARROW")
    mel, noise = (t.to(DEV, torch.float32) for t in _inputs(cfg, 2, 5, None, seed=1))
    with pytest.raises(ValueError, match="4 frames"):
        model.vocode(mel, [5, 3], noise=noise)
    with pytest.raises(ValueError, match="4 of the frames"):
        model.vocode(mel[:, :, :3].contiguous(), noise=noise[:, :, :3].contiguous())
