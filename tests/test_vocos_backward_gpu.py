"""GPU: gvx_vocos_forward_train and gvx_vocos_backward (csrc/vocos_train.hip) through the C ABI against float64 autograd of the
restatement (tests/vocos_grad_ref64.py): every tape tensor, every parameter gradient and d_mel, tensor by tensor.  The tape, the
workspaces and every output start as NaN; tape and workspace have exactly their stated sizes; NaN sits behind every row's frames in the
mel and behind its delivered samples in d_wav; forward_train's waveform is compared bit for bit with gvx_vocos_forward's in every case.

Tolerance: the project's rule (tests/vocos_train_helpers.py, bound_check).  Per tensor, e is the largest |float32 restatement - float64|;
the device may differ from float64 by at most 8 x max(e, 2^-23 max|g64|).  Every ratio is printed.

The clamp.  Tie-free cases assert on the CPU that no float64 log-magnitude inside a row lies within 8 x max(e, ulp) of the head product
from ln 100 (the first mel seed of 1..8 for which that holds; none: the case fails) and compare with plain autograd; 20 - 24 % of the
magnitudes are clamped, so both branches of the clip run.  NARROW at 513 and 515 frames has no tie-free seed: those cases are pinned to
the device's own decisions, read off its tape, after asserting that every decision that differs from float64's is such a near-tie.
They are the piece edges of the whole call: one piece of GVX_VOCOS_GRAD_PIECE = 128 frames per 128 frames of a row, so 513 frames are
four pieces and one frame, and (515, 1, 257) has rows whose last pieces lie wholly or partly behind them; B * T crosses the 512-row
threshold of the split-K choice and the 128-row GEMM tile.

Largest ratios seen on an MI355X: DESIGN.md, "Vocos generator: tape forward and backward"."""
import functools

import pytest
import torch

from tests import vocos_grad_ref64 as GR
from tests import vocos_ref64 as R
from tests.vocos_train_helpers import DEV, NAN, TrainNet, compare_grads, compare_mel_slot, compare_tape, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    _net.cache_clear()
    _tie_free.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _net(name):
    cfg = getattr(R, name)
    ref = R.Generator(cfg, seed=11)
    ref.load_state_dict({k: v.float().double() for k, v in ref.state_dict().items()})   # what the device holds: float32 weights
    return cfg, ref, TrainNet(cfg, ref)


@functools.lru_cache(maxsize=None)
def _tie_free(name, B, T, lens):
    cfg, ref, _ = _net(name)
    seed, mel, G, want = GR.tie_free_case(ref, cfg, B, T, lens, G_seed=1000 * B + T)
    print(f"{name} {B} x {T} {lens}: mel seed {seed} is tie-free, {100 * GR.clamped_share(want, lens, cfg):.1f} % of the magnitudes clamped")
    return mel, G, want


def _device_run(name, mel, G, lens, want_mel=True):
    cfg, _, net = _net(name)
    B, _, T = mel.shape
    mel_d, G_d = poisoned(cfg, mel, G, lens)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    wav, tape = net.forward_train(mel_d, lens_d)
    plain = net.forward(mel_d, lens_d)
    assert torch.equal(wav, plain), "forward_train's waveform is not gvx_vocos_forward's, bit for bit"
    grads = net.backward(G_d, lens_d, B, T, tape, want_mel)
    return wav, tape, grads


def _check_rows_alone(name, mel, G, lens, grads):
    cfg, _, net = _net(name)
    hop = cfg["hop_length"]
    for b, t in enumerate(lens):
        assert not grads["mel"][b, :, t:].any(), f"row {b}: d_mel is not 0 behind its {t} frames"
        mel_d, G_d = poisoned(cfg, mel[b:b + 1, :, :t].contiguous(), G[b:b + 1, :t * hop].contiguous(), None)
        wav_b, tape_b = net.forward_train(mel_d)
        assert torch.equal(wav_b, net.forward(mel_d)), "forward_train's waveform is not gvx_vocos_forward's, bit for bit"
        alone = net.backward(G_d, None, 1, t, tape_b)
        assert torch.equal(alone["mel"][0], grads["mel"][b, :, :t]), f"row {b}: d_mel differs from that row run alone"


def _check_tie_free(name, B, T, lens=None):
    cfg, _, net = _net(name)
    mel, G, want = _tie_free(name, B, T, lens)
    wav, tape, grads = _device_run(name, mel, G, lens)
    what = f"{name} {B} x {T}" + (f" lengths {lens}" if lens else "")
    compare_mel_slot(net, tape, mel, lens, what)
    compare_tape(net.tape_views(tape, B, T), want, lens, what)
    compare_grads(grads, want, what)
    if lens is not None:
        _check_rows_alone(name, mel, G, lens, grads)
    return mel, G, want, tape, grads


def _check_pinned(name, B, T, lens=None, mel_seed=1):
    cfg, ref, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, mel_seed).float().double(), GR.cotangent(cfg, B, T, 1000 * B + T)
    wav, tape, grads = _device_run(name, mel, G, lens)
    views = [v.cpu() for v in net.tape_views(tape, B, T)]
    free = GR.reference(ref, mel, lens, G)
    H = cfg["n_fft"] // 2
    m64 = free["tape"][-1][..., :H + 1]
    masks = GR.masks_from_coeffs(views[-1], cfg)
    differ = masks != (m64 <= R.LOG_CLAMP)
    if lens is not None:
        for b, t in enumerate(lens):
            differ[b, t:] = False
    assert ((m64[differ] - R.LOG_CLAMP).abs() <= GR.clamp_margin(free)).all(), "a clamp decision differs from float64's away from ln 100"
    want = GR.reference(ref, mel, lens, G, masks)
    what = f"{name} {B} x {T}" + (f" lengths {lens}" if lens else "") + f" pinned ({GR.near_ties(free, lens, cfg)} near-ties, {int(differ.sum())} decided the other way)"
    compare_mel_slot(net, tape, mel, lens, what)
    compare_tape(views, want, lens, what)
    compare_grads(grads, want, what)
    if lens is not None:
        _check_rows_alone(name, mel, G, lens, grads)


@pytest.mark.parametrize("name,B,T,lens", [
    ("NARROW", 1, 1, None), ("NARROW", 2, 17, None), ("NARROW", 3, 19, (19, 1, 16)),
    ("MID", 1, 2, None), ("MID", 2, 17, None), ("MID", 3, 33, (33, 2, 17)),
    ("ODD", 2, 9, None), ("ODD", 3, 17, (17, 1, 6)),
    ("DEFAULT", 1, 18, None), ("DEFAULT", 3, 17, (17, 2, 9))])
def test_gradients_tie_free(name, B, T, lens):
    """NARROW: 32 channels (half-idle waves), the 128 x 32 tile, K = 140 in the embedding; MID: "center", T = 2 the least; ODD: 37 mels in
    40 padded channels, 96 channels (NC = 2 with an idle half chunk), n_fft 1024 at a hop that divides nothing; DEFAULT: the published
    sizes, NC = 8.  The ragged cases also assert d_mel's zeros and row-alone bits."""
    _check_tie_free(name, B, T, lens)
    if name == "DEFAULT" and lens is not None:
        _net.cache_clear()
        _tie_free.cache_clear()


@pytest.mark.parametrize("B,T,lens", [(1, 513, None), (3, 515, (515, 1, 257))])
def test_piece_edges_pinned(B, T, lens):
    _check_pinned("NARROW", B, T, lens)


def test_a_gamma_of_zero():
    """gamma[0] = 0 in the block: d gamma[0], and row 0 of d pwconv2.weight and of d pwconv2.bias (exact zeros), come from the unfold's
    products, never from a division."""
    cfg = R.NARROW
    ref = R.Generator(cfg, seed=11)
    sd = {k: v.float().double() for k, v in ref.state_dict().items()}
    sd["backbone.convnext.0.gamma"][0] = 0.0
    ref.load_state_dict(sd)
    net = TrainNet(cfg, ref)
    B, T = 2, 17
    seed, mel, G, want = GR.tie_free_case(ref, cfg, B, T, None, G_seed=7)
    mel_d, G_d = poisoned(cfg, mel, G, None)
    wav, tape = net.forward_train(mel_d)
    assert torch.equal(wav, net.forward(mel_d))
    grads = net.backward(G_d, None, B, T, tape)
    compare_mel_slot(net, tape, mel, None, "NARROW with gamma[0] = 0")
    compare_tape(net.tape_views(tape, B, T), want, None, "NARROW with gamma[0] = 0")
    compare_grads(grads, want, "NARROW with gamma[0] = 0")
    assert want["grads"]["backbone.convnext.0.gamma"][0].abs().item() > 0.0
    assert not grads["backbone.convnext.0.pwconv2.weight"][0].any() and grads["backbone.convnext.0.pwconv2.bias"][0].item() == 0.0


def test_determinism_null_d_mel_and_dirty_workspace():
    """Two backward calls on one tape give the same bits; d_mel_out = NULL changes no bit of a parameter gradient; the workspace is
    exactly gvx_vocos_backward_workspace_bytes with a NaN guard behind it that stays NaN, and a reused (dirty) one gives the same bits."""
    name, B, T, lens = "MID", 3, 33, (33, 2, 17)
    cfg, _, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, 1).float().double(), GR.cotangent(cfg, B, T, 5)
    mel_d, G_d = poisoned(cfg, mel, G, lens)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    wav, tape = net.forward_train(mel_d, lens_d)
    assert torch.equal(wav, net.forward(mel_d, lens_d)), "forward_train's waveform is not gvx_vocos_forward's, bit for bit"
    first = net.backward(G_d, lens_d, B, T, tape)
    again = net.backward(G_d, lens_d, B, T, tape)
    without = net.backward(G_d, lens_d, B, T, tape, want_mel=False)
    for k in first:
        assert not torch.isnan(first[k]).any(), k
        assert torch.equal(first[k], again[k]), k
        assert k == "mel" or torch.equal(first[k], without[k]), k
    need = net.ws_bytes(B, T)
    assert need % 256 == 0 and net.tape_bytes(B, T) == tape.numel() * 4
    buf = torch.full(((need + 4096) // 4,), NAN, dtype=torch.float32, device=DEV)
    for _ in range(2):   # the second call finds the first one's leftovers
        grads = net.new_grads(True, B, T)
        assert net.backward_rc(G_d, lens_d, B, T, tape, tape.numel() * 4, grads, buf, need) == 0
        torch.cuda.synchronize()
        assert torch.isnan(buf[need // 4:]).all(), "the call wrote behind the workspace"
        assert all(torch.equal(first[k], grads[k]) for k in first)


def test_refusals_happen_before_any_launch():
    """A short or misaligned tape, a short workspace, a missing name, a wrong element count, a NULL destination, a missing raw parameter,
    B and T as the forward refuses them, T below 1 + center: each returns its code and leaves every output NaN."""
    name, B, T = "MID", 2, 5
    cfg, _, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, 1).float().double(), GR.cotangent(cfg, B, T, 3)
    mel_d, G_d = poisoned(cfg, mel, G, None)
    wav, tape = net.forward_train(mel_d)
    assert torch.equal(wav, net.forward(mel_d)), "forward_train's waveform is not gvx_vocos_forward's, bit for bit"
    tb, wb = tape.numel() * 4, net.ws_bytes(B, T)
    ws = torch.full((wb // 4,), NAN, dtype=torch.float32, device=DEV)
    wav = torch.full((B, T * cfg["hop_length"]), NAN, dtype=torch.float32, device=DEV)
    scratch = torch.full_like(tape, NAN)
    assert net.forward_train_rc(mel_d, None, wav, scratch, tb - 1) == -5                      # GVX_ERR_WORKSPACE
    assert net.forward_train_rc(mel_d, None, wav, scratch, tb, ws, 16) == -5
    torch.cuda.synchronize()
    assert torch.isnan(wav).all() and torch.isnan(scratch).all()
    cases = ((-5, {}, B, T, tb - 1, wb), (-5, {}, B, T, tb, wb - 1), (-3, dict(skip=("backbone.convnext.1.gamma",)), B, T, tb, wb),
             (-3, dict(skip_raw=("backbone.convnext.0.pwconv2.bias",)), B, T, tb, wb),
             (-4, dict(numel={"head.out.weight": 7}), B, T, tb, wb), (-4, dict(null=("backbone.embed.bias",)), B, T, tb, wb),
             (-1, {}, 0, T, tb, wb), (-1, {}, B, 0, tb, wb), (-1, {}, B, 1, tb, wb))       # -1 INVALID_ARG, -3 MISSING_WEIGHT, -4 SHAPE
    for want, kw, b_, t_, tbytes, wbytes in cases:
        grads = net.new_grads(True, B, T)
        assert net.backward_rc(G_d, None, b_, t_, tape, tbytes, grads, ws, wbytes, **kw) == want, (want, kw, b_, t_)
        torch.cuda.synchronize()
        assert all(torch.isnan(g).all() for g in grads.values()) and torch.isnan(ws).all()
    grads = net.new_grads(True, B, T)
    assert net.backward_rc(G_d, None, B, T, tape.view(torch.uint8)[1:], tb - 1, grads, ws, wb) == -5   # misaligned
    assert net.backward_rc(G_d, None, B, T, tape, tb, grads, ws.view(torch.uint8)[1:], wb - 1) == -5
    torch.cuda.synchronize()
    assert all(torch.isnan(g).all() for g in grads.values()) and torch.isnan(ws).all()
