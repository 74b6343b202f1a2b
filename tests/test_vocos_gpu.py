"""GPU: the Vocos generator (gvx_vocos_forward, csrc/vocos.hip, through ``VocosGenerator``) against the float64 restatement of
tests/vocos_ref64.py: the waveform and every stage output - x after embed + norm, after every block, after the final norm, and the head
product - element by element.

Tolerance: as tests/test_bigvgan_gpu.py.  Every case evaluates the SAME restatement in float32 on the CPU and takes, tensor by tensor,
its largest distance from float64 - a number that depends on the reference alone.  The device may differ from float64 by at most 8
times the larger of that number and one float32 ulp at the tensor's scale (2^-23 x its largest magnitude).  The ratio is printed.

Largest ratios seen on an MI355X: see README.md, "Vocos"."""
import functools

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.configs import AudioConfig, VocosConfig
from genvox_amd.vocos import VocosGenerator
from tests import vocos_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23


def _build(cfg):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = cfg["hop_length"], cfg["n_mels"]   # a vocoder of hop 128 or 130 is a test's size
    return VocosGenerator(VocosConfig(**R.model_kwargs(cfg)), ac)


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


@functools.lru_cache(maxsize=None)
def _case(name, B, T, lens):
    """(mel float64 with NaN behind every row's length, reference outputs, per-tensor float32 error of the reference): computed once."""
    cfg, ref, _ = _net(name)
    mel = R.random_mel(cfg, B, T, seed=100 * B + T).float().double()
    if lens is not None:
        for b, t in enumerate(lens):
            mel[b, :, t:] = float("nan")
    want, errs = R.reference_pair(ref, mel, lens)
    return mel, want, errs


def _run(model, mel, lens=None, ws=None):
    """-> (wav, stages); a workspace of this call's own starts as NaN."""
    if ws is None:
        ws = torch.full((model.workspace_bytes(*mel.shape[::2]) // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    wav, stages = model.vocode(mel, lens, stage_outputs=True, workspace=ws)
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
    mel, want, errs = _case(name, B, T, lens)
    got = _run(model, mel.to(DEV, torch.float32), lens)
    _compare(got, want, errs, f"{name} {B} x {T}" + (f" lengths {lens}" if lens else ""))
    for b, t in enumerate(lens if lens is not None else [T] * B):   # exact zeros behind every row, in every tensor
        assert not got[0][b, R.sample_count(cfg, t):].any()
        for st in got[1]:
            assert not st[b, t:].any()
    return got


@pytest.mark.parametrize("name,B,T,lens", [("NARROW", 2, 5, None), ("MID", 3, 33, (33, 2, 17)), ("ODD", 2, 130, None), ("DEFAULT", 1, 12, None),
                                           ("DEFAULT", 2, 70, None)])
def test_every_stage_and_the_waveform(name, B, T, lens):
    """NARROW: the 128 x 32 GEMM tile and half-idle waves in the LayerNorm; MID ragged; ODD at 2 x 130: B * T crosses a 128-row tile, a
    hop that divides nothing; DEFAULT: the published configuration."""
    wav, stages = _check(name, B, T, lens)
    cfg = getattr(R, name)
    assert wav.shape == (B, T * cfg["hop_length"]) and len(stages) == cfg["num_layers"] + 3
    if name == "DEFAULT":   # its weights are not kept
        if (B, T) == (2, 70):
            _net.cache_clear()
            _case.cache_clear()


@pytest.mark.parametrize("name,lens", [("MID", (33, 2, 17, 32)), ("ODD", (130, 1, 129, 64))])
def test_ragged_rows_equal_the_rows_alone(name, lens):
    """A row of a ragged batch has the bits of that row run alone - the products' sums do not depend on M or on the tile shape; the mel
    behind a row's frames is NaN, so a read past the row's end shows."""
    cfg, _, model = _net(name)
    T = max(lens)
    mel = R.random_mel(cfg, len(lens), T, seed=5).float()
    for b, t in enumerate(lens):
        mel[b, :, t:] = float("nan")
    mel = mel.to(DEV)
    wav, stages = _run(model, mel, lens)
    assert not torch.isnan(wav).any()
    for b, t in enumerate(lens):
        alone, st = _run(model, mel[b:b + 1, :, :t].contiguous())
        n = R.sample_count(cfg, t)
        assert torch.equal(alone[0, :n], wav[b, :n]) and not wav[b, n:].any()
        for one, many in zip(st, stages):
            assert torch.equal(one[0], many[b, :t]) and not many[b, t:].any()


def test_rows_do_not_depend_on_the_gemm_tile_shape():
    """4 x 8250 frames of MID: 33,000 rows, which plan_gemm covers with 128 x 128 tiles for the first 32,768 and 64 x 64 tiles for the
    rest (N = 192: 516 tiles of 128 x 128, a remainder of 4 over two rounds of 256), while a row alone (8,250 or 40 rows) runs on 64 x 64
    tiles throughout.  Every shape adds the k-steps in the same order, so the last row - which lies across the cut - and a short row
    have the bits of their runs alone."""
    cfg, _, model = _net("MID")
    lens = (8250, 40, 8100, 8250)
    mel = R.random_mel(cfg, 4, 8250, seed=21).float().to(DEV)
    wav = model.vocode(mel, lens)
    for b in (1, 3):
        t = lens[b]
        alone = model.vocode(mel[b:b + 1, :, :t].contiguous())
        n = R.sample_count(cfg, t)
        assert torch.equal(alone[0, :n], wav[b, :n]) and not wav[b, n:].any()
    model._workspace = None   # 190 MB of scratch: not kept


def test_python_call_split_by_rows_inference_lengths_and_the_refused_backward():
    cfg, _, shared = _net("MID")
    model = _build(cfg)
    model.load_state_dict(shared.state_dict())
    model.to(DEV)
    lens = (33, 2, 32, 17)
    mel = R.random_mel(cfg, 4, 33, seed=8).float().to(DEV)
    whole = model.vocode(mel, lens)
    assert model.workspace_bytes(4, 33) <= model.WORKSPACE_CAP_BYTES
    model.WORKSPACE_CAP_BYTES = model.workspace_bytes(1, 33)
    model._workspace = None
    split = model.vocode(mel, torch.tensor(lens))
    torch.cuda.synchronize()
    assert model._workspace.numel() == model.workspace_bytes(1, 33)
    assert torch.equal(whole, split)
    assert torch.equal(whole, _run(shared, mel, lens)[0])   # stage_out changes no bit of the waveform
    with torch.no_grad():
        assert torch.equal(model.vocode_with_grad(mel, lens), whole)   # nothing asks for a gradient: it is vocode
    with pytest.raises(NotImplementedError, match="backward"):
        model.vocode_with_grad(mel, lens)
    out = model.inference({"mel": mel, "mel_lengths": torch.tensor(lens)})
    assert out["lengths"].tolist() == [(t - 1) * 256 for t in lens] and out["lengths"].dtype == torch.int32   # "center"
    assert model.inference({"mel": mel})["lengths"].tolist() == [32 * 256] * 4
    assert torch.equal(model({"mel": mel, "mel_lengths": lens})["waveform"], whole)
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (33, 1, 32, 17))   # "center" needs 2 frames
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (34, 2, 32, 17))
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel[:, :, :1].contiguous())
    _, _, same = _net("NARROW")
    mel = R.random_mel(R.NARROW, 2, 5, seed=1).float().to(DEV)
    out = same.inference({"mel": mel, "mel_lengths": [5, 1]})
    assert out["lengths"].tolist() == [5 * 128, 128] and out["waveform"].shape == (2, 5 * 128)   # "same"
    assert same.inference({"mel": mel})["lengths"].tolist() == [5 * 128] * 2


@pytest.mark.parametrize("name,B,T,lens", [("MID", 2, 9, (5, 9)), ("NARROW", 3, 7, None)])
def test_workspace_contract(name, B, T, lens):
    """Exactly the stated size, all NaN before, a NaN guard behind it that stays NaN; one byte short is refused before anything is
    written; the same workspace reused (dirty) for this shape and for another one gives the same bits."""
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
    small = mel[B - 1:, :, :T - 2].contiguous()   # another shape (of a row without NaN frames) in the same, now dirty, workspace
    assert torch.equal(model.vocode(small, workspace=ws), _run(model, small)[0])
    plain = model.vocode(mel, lens, workspace=ws)
    assert torch.equal(plain, got[0])
    wav = torch.full_like(got[0], 7.0)
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    before = buf.clone()
    stream = torch.cuda.current_stream().cuda_stream
    rc = lambda ws_ptr, n: _lib.load().gvx_vocos_forward(model._handle, mel.data_ptr(), lens_dev.data_ptr() if lens_dev is not None else None, B, T,
                                                          wav.data_ptr(), None, ws_ptr, n, stream)
    got_rc = rc(ws.data_ptr(), need - 1)
    torch.cuda.synchronize()
    assert got_rc == -5, got_rc   # GVX_ERR_WORKSPACE
    assert (wav == 7.0).all() and torch.equal(before.view(torch.int32), buf.view(torch.int32))
    assert rc(ws.data_ptr() + 1, need) == -5   # misaligned


def test_two_calls_give_the_same_bits_and_a_changed_weight_repacks():
    cfg, _, shared = _net("MID")
    model = _build(cfg)
    model.load_state_dict(shared.state_dict())
    model.to(DEV)
    mel = R.random_mel(cfg, 2, 33, seed=3).float().to(DEV)
    a, b = _run(model, mel), _run(model, mel)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    blob = model._blob
    with torch.no_grad():
        model.backbone.convnext[1].gamma.mul_(0.5)   # folded into pwconv2 when the blob is packed
    c = _run(model, mel)
    assert model._blob is not blob
    assert torch.equal(c[1][1], a[1][1]) and not torch.equal(c[1][2], a[1][2]) and not torch.equal(c[0], a[0])
    with torch.no_grad():
        model.backbone.convnext[1].gamma.mul_(2.0)   # exact: back to the first weights
    assert torch.equal(_run(model, mel)[0], a[0])


def test_stage_timing_gives_four_durations():
    _, _, model = _net("MID")
    mel = R.random_mel(R.MID, 2, 33, seed=3).float().to(DEV)
    model.enable_stage_timing(True)
    model.vocode(mel)
    times = model.stage_times_ms()
    model.enable_stage_timing(False)
    assert len(times) == 4 and all(t >= 0 for t in times)   # embed + norm, the blocks, final norm + head product, the ISTFT
