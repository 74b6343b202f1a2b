"""GPU: gvx_melgan_forward_train and gvx_melgan_backward (csrc/melgan_train.hip) through the C ABI against float64 autograd of the
restatement in tests/melgan_grad_ref64.py: every tape tensor, every parameter gradient and d_mel, tensor by tensor.  The tape, the
workspace and every output start as NaN; tape and workspace have exactly their stated sizes.

Tolerance.  Per gradient tensor, e is the largest |float32 restatement - float64| (a number of the reference alone; e / max|g64| lies
between 1e-7 and 2e-6 on the CPU for these cases); the device may differ from float64 by at most 8 x max(e, 2^-23 max|g64|), the
second term being one ulp of the tensor's scale - a floor for one-element tensors such as post.bias.  Tape tensors follow the forward
tests' 8 x rule.

LeakyReLU ties.  Tie-free cases assert on the CPU that no float64 pre-activation lies within 8 x its tensor's float32 error of 0 (the
mel seed is the first of 1..8 for which that holds; none: the case fails) and compare with plain autograd.  Pinned cases (the default
sizes, and the long rows of the split-piece cases) read the LeakyReLU decisions from the device's own tape, assert that every decision
that differs from float64's is a true near-tie, and compare with the restatement pinned to those decisions.

Pieces.  The weight and bias gradients reduce over the positions of all rows laid end to end, B * T * mul of them for a layer at
`mul` positions per frame, in pieces of MGB_PIECE = 512 positions.  test_split_pieces picks B * T = 512, 513 and 1030 for the layers
at mul = 1 - exactly one piece, one piece plus one position, two pieces plus a tail of 6 - which are, per weight-gradient kernel:
mgb_wgrad_valu_kernel NARROW's ups.0 (16 output channels), mgb_wgrad_mfma_kernel<1> NARROW's pre (32), mgb_wgrad_mfma_kernel<2>
SHALLOW's pre and ups.0 (128 and 64), mgb_colsum_kernel every bias of those; the layers at mul = 4 and 8 run 4 to 17 pieces with and
without a tail in the same calls.  There B = 1: no piece meets a row boundary.  test_pieces_across_rows runs the same kernels with
several rows and several pieces in one call (shapes in tests/backward_piece_cases.py, all pinned):
    NARROW, SHALLOW 3 x 350                    rows begin at 350 and 700 of the line at mul = 1, inside pieces 0 and 1 and inside a
                                               32-position k-tile of the matrix kernel, whose threads each decide their own row;
    NARROW, SHALLOW 3 x 1030, (300, 4, 301)    7 pieces at mul = 1: piece 1 lies wholly behind row 0's length and must come out as
                                               zeros, not as what the workspace held; rows 1 and 2 begin inside pieces 2 and 4 and
                                               inside k-tiles that begin behind the previous row's length; the last piece has 18
                                               positions, all dead; 25 and 49 pieces at mul = 4 and 8, several wholly dead;
    DEFAULT 4 x 32                             the training benchmark's shape class: one piece holding four rows at mul = 1, pieces
                                               of exactly two rows at mul = 8, four pieces per row at mul = 64;
    DEFAULT 4 x 33, (33, 5, 32, 17)            Lmax = 33 and 264 at the 512- and 256-channel layers: k-tiles with live positions of
                                               two rows; row 1 leaves whole pieces dead from mul = 64 on;
and test_pieces_across_rows_without_kinks DEFAULT 4 x 32 at slope 1 against plain autograd.  tests/test_backward_piece_layouts_cpu.py
asserts from the lengths alone that each shape contains these situations."""
import functools

import pytest
import torch

from tests import backward_piece_cases as PC
from tests import melgan_grad_ref64 as GR
from tests import melgan_ref64 as R
from tests.melgan_train_helpers import DEV, NAN, TrainNet, compare_grads, compare_tape, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """The NaN-filled tapes and workspaces of this module go back to the driver, not into the allocator's cache for later modules."""
    yield
    torch.cuda.empty_cache()

CFGS = dict(NARROW=R.NARROW, SHALLOW=R.SHALLOW, TWO_DEEP=R.TWO_DEEP, DEFAULT=R.DEFAULT,
            WIDE=dict(R.SHALLOW, base_channels=512),      # channels 256 and 128: the 128-wide tile of the data gradients
            DEFAULT_LINEAR=dict(R.DEFAULT, slope=1.0),    # no kinks: the same kernels against plain autograd at the default sizes
            ODD=R.ODD, DEEP=R.DEEP)


@functools.lru_cache(maxsize=None)
def _net(name):
    cfg = CFGS[name]
    sd = R.random_state(cfg, seed=11)
    return cfg, sd, TrainNet(cfg, sd)


def _cotangent(cfg, B, T):
    g = torch.Generator().manual_seed(1000 * B + T)
    return torch.randn(B, T * R.hop(cfg), generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _tie_free(name, B, T, lens):
    """(mel, G, reference) of a case without near-ties: computed once, shared by the tests, never changed."""
    cfg, sd, _ = _net(name)
    seed, mel, G, ref = GR.tie_free_case(sd, cfg, B, T, lens, G_seed=1000 * B + T)
    assert GR.near_ties(ref, lens) == 0
    print(f"{name} {B} x {T} {lens}: mel seed {seed} is tie-free")
    return mel, G, ref


def _device_run(name, mel, G, lens, want_mel=True):
    cfg, _, net = _net(name)
    B, _, T = mel.shape
    mel_d, G_d = poisoned(mel, G, lens, R.hop(cfg))
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    wav, tape = net.forward_train(mel_d, lens_d)
    plain = net.forward(mel_d, lens_d)
    grads = net.backward(G_d, lens_d, B, T, tape, want_mel)
    assert torch.equal(wav, plain), "forward_train's waveform is not gvx_melgan_forward's, bit for bit"
    return wav, tape, grads


def _check_tie_free(name, B, T, lens=None):
    _, _, net = _net(name)
    mel, G, ref = _tie_free(name, B, T, lens)
    wav, tape, grads = _device_run(name, mel, G, lens)
    what = f"{name} {B} x {T}" + (f" lengths {lens}" if lens else "")
    compare_tape(net.tape_views(tape, B, T), ref, lens, what)
    compare_grads(grads, ref, what)
    return mel, G, ref, tape, grads


def _check_pinned(name, B, T, lens=None, mel_seed=1):
    """The reference is pinned to the device's own LeakyReLU decisions, after asserting that each one that differs from float64's
    is a true near-tie.  With lengths the signs are compared inside each row (behind it the device's tape holds NaN and the reference
    0, and the restatement takes no decision from there), and the case asserts what test_ragged_rows asserts."""
    cfg, sd, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, mel_seed), _cotangent(cfg, B, T)
    wav, tape, grads = _device_run(name, mel, G, lens)
    views = [v.cpu() for v in net.tape_views(tape, B, T)]
    free = GR.reference(sd, mel, lens, cfg, G)   # float64's own decisions
    flips = 0
    for i, mul in enumerate(GR.tape_muls_of(free)):
        if i == 0:
            continue
        differ = (views[i] > 0) != (free["tape"][i] > 0)
        if lens is not None:
            for b, t in enumerate(lens):
                differ[b, :, t * mul:] = False
        flips += int(differ.sum())
        assert (free["tape"][i][differ].abs() <= GR.FACTOR * free["tape_err"][i]).all(), f"tape tensor {i}: a sign differs from float64 away from 0"
    ref = GR.reference(sd, mel, lens, cfg, G, GR.masks_from_tape(views, cfg["slope"]))
    what = f"{name} {B} x {T}" + (f" lengths {lens}" if lens else "") + f" pinned ({GR.near_ties(free, lens)} near-ties, {flips} decided the other way)"
    compare_tape(views, ref, lens, what)
    print(f"{what}: largest gradient error / bound {compare_grads(grads, ref, what):.3f}")
    if lens is not None:
        _check_rows_alone(name, mel, G, lens, grads)


def _check_rows_alone(name, mel, G, lens, grads):
    """d_mel of every row is exactly 0 behind its length and bit-equal to that row run alone."""
    cfg, _, net = _net(name)
    hop = R.hop(cfg)
    for b, t in enumerate(lens):
        assert not grads["mel"][b, :, t:].any(), f"row {b}: d_mel is not 0 behind its {t} frames"
        mel_d, G_d = poisoned(mel[b:b + 1, :, :t].contiguous(), G[b:b + 1, :t * hop].contiguous(), None, hop)
        _, tape_b = net.forward_train(mel_d)
        alone = net.backward(G_d, None, 1, t, tape_b)
        assert torch.equal(alone["mel"][0], grads["mel"][b, :, :t]), f"row {b}: d_mel differs from that row run alone"


@pytest.mark.parametrize("name,B,T", [("NARROW", 2, 4), ("NARROW", 2, 7), ("SHALLOW", 2, 5), ("TWO_DEEP", 1, 4), ("TWO_DEEP", 2, 17), ("WIDE", 2, 4)])
def test_gradients_tie_free(name, B, T):
    """NARROW: fmaf layers, K = 70 in the first convolution; at T = 4 both reflections of the dilation-9 layer fold onto the same
    positions of a 16-position row.  TWO_DEEP 2 x 17: lengths 68 and 136 cross a 128-position tile.  WIDE: the 128-wide tile."""
    _check_tie_free(name, B, T)


@pytest.mark.parametrize("name,B,T,lens,tie_free", [
    ("ODD", 2, 5, None, False), ("ODD", 1, 11, None, False), ("ODD", 3, 11, (11, 4, 6), False),
    ("DEEP", 2, 5, None, True), ("DEEP", 1, 11, None, True), ("DEEP", 3, 11, (11, 4, 6), True)])
def test_configurations_no_other_case_reaches(name, B, T, lens, tie_free):
    """ODD and DEEP of tests/melgan_ref64.py.  ODD: 37 mels in 40 padded channels, 136 and 68 channels on the matrix kernels, and 34
    channels - tensors whose rows are no multiple of 16 bytes - through mgb_wide's three conditions: every gradient of stage 1 and the
    data gradient into stage 0 run on the dot-product kernels.  DEEP: eight residual layers at dilation 1 under slope 1.  DEEP is small
    enough for a tie-free mel; ODD is pinned (most mel seeds leave a near-tie or two among its 10^5 tape elements)."""
    if tie_free:
        mel, G, _, _, grads = _check_tie_free(name, B, T, lens)
        if lens is not None:
            _check_rows_alone(name, mel, G, lens, grads)
    else:
        _check_pinned(name, B, T, lens, mel_seed=R.BACKWARD_MEL_SEEDS.get((name, B, T), 1))   # tests/melgan_ref64.py says why 1 x 11 has its own


@pytest.mark.parametrize("T", [4, 5])
def test_gradients_default_sizes_pinned(T):
    _check_pinned("DEFAULT", 1, T)


def test_gradients_default_sizes_without_kinks():
    """slope = 1: LeakyReLU is the identity, so plain float64 autograd is the reference at the default sizes, with no tape reading."""
    name, B, T = "DEFAULT_LINEAR", 1, 4
    cfg, sd, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, 1), _cotangent(cfg, B, T)
    ref = GR.reference(sd, mel, None, cfg, G)
    wav, tape, grads = _device_run(name, mel, G, None)
    compare_tape(net.tape_views(tape, B, T), ref, None, name)
    compare_grads(grads, ref, name)


@pytest.mark.parametrize("name,T", [("NARROW", 512), ("NARROW", 513), ("NARROW", 1030), ("SHALLOW", 512), ("SHALLOW", 513), ("SHALLOW", 1030)])
def test_split_pieces(name, T):
    """Reduction lengths of one piece, one piece plus one position, two pieces plus a tail, for every weight-gradient kernel (the
    module docstring names the layers)."""
    _check_pinned(name, 1, T)


@pytest.mark.parametrize("name,B,T,lens", PC.MELGAN_CASES)
def test_pieces_across_rows(name, B, T, lens):
    """Several rows and several pieces in one call, padded and ragged (the module docstring says what each shape reaches;
    tests/test_backward_piece_layouts_cpu.py asserts that it does).  The ragged cases also assert what test_ragged_rows asserts."""
    _check_pinned(name, B, T, lens)


def test_pieces_across_rows_without_kinks():
    """slope = 1 at the default sizes, 4 x 32 frames: plain float64 autograd, no tape reading."""
    name, B, T, lens = PC.MELGAN_LINEAR_CASE
    cfg, sd, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, 1), _cotangent(cfg, B, T)
    ref = GR.reference(sd, mel, lens, cfg, G)
    wav, tape, grads = _device_run(name, mel, G, lens)
    what = f"{name} {B} x {T}"
    compare_tape(net.tape_views(tape, B, T), ref, lens, what)
    print(f"{what}: largest gradient error / bound {compare_grads(grads, ref, what):.3f}")


@pytest.mark.parametrize("name,T,lens", [("NARROW", 9, (4, 9, 5)), ("TWO_DEEP", 17, (4, 17, 8))])
def test_ragged_rows(name, T, lens):
    """NaN in mel at and behind each length and in d_wav at and behind T_b * hop.  Parameter gradients equal the float64 sum of the
    rows run alone (that is what the reference computes); d_mel of every row is bit-equal to that row run alone and exactly 0 behind
    its length.  TWO_DEEP: the 4-frame row has 32 positions at the last stage and leaves the second 128-position tile empty."""
    cfg, _, net = _net(name)
    mel, G, ref, tape, grads = _check_tie_free(name, len(lens), T, lens)
    hop = R.hop(cfg)
    for b, t in enumerate(lens):
        assert not grads["mel"][b, :, t:].any(), f"row {b}: d_mel is not 0 behind its {t} frames"
        mel_d, G_d = poisoned(mel[b:b + 1, :, :t].contiguous(), G[b:b + 1, :t * hop].contiguous(), None, hop)
        _, tape_b = net.forward_train(mel_d)
        alone = net.backward(G_d, None, 1, t, tape_b)
        assert torch.equal(alone["mel"][0], grads["mel"][b, :, :t]), f"row {b}: d_mel differs from that row run alone"


def test_determinism_null_d_mel_and_dirty_workspace():
    """Two backward calls give the same bits; d_mel_out = NULL changes no bit of a parameter gradient; the workspace is exactly
    gvx_melgan_backward_workspace_bytes with a NaN guard behind it that stays NaN, and a reused (dirty) one gives the same bits."""
    name, B, T, lens = "TWO_DEEP", 3, 17, (4, 17, 8)
    cfg, _, net = _net(name)
    mel, G, _ = _tie_free(name, B, T, lens)
    mel_d, G_d = poisoned(mel, G, lens, R.hop(cfg))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _, tape = net.forward_train(mel_d, lens_d)
    first = net.backward(G_d, lens_d, B, T, tape)
    again = net.backward(G_d, lens_d, B, T, tape)
    without = net.backward(G_d, lens_d, B, T, tape, want_mel=False)
    for k in first:
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
    """A short tape, a short workspace, a missing name, a wrong element count: each returns its code and leaves every output NaN."""
    name, B, T = "NARROW", 2, 7
    cfg, _, net = _net(name)
    mel, G, _ = _tie_free(name, B, T, None)
    mel_d, G_d = poisoned(mel, G, None, R.hop(cfg))
    _, tape = net.forward_train(mel_d)
    tb, wb = tape.numel() * 4, net.ws_bytes(B, T)
    ws = torch.full((wb // 4,), NAN, dtype=torch.float32, device=DEV)
    wav = torch.full((B, T * R.hop(cfg)), NAN, dtype=torch.float32, device=DEV)
    scratch = torch.full_like(tape, NAN)
    assert net.forward_train_rc(mel_d, None, wav, scratch, tb - 1) == -5                      # GVX_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(wav).all() and torch.isnan(scratch).all()
    for want, kw, tbytes, wbytes in ((-5, {}, tb - 1, wb), (-5, {}, tb, wb - 1), (-3, dict(skip=("res.1.2.mix.bias",)), tb, wb),
                                     (-4, dict(numel={"ups.0.weight": 7}), tb, wb)):          # -3 GVX_ERR_MISSING_WEIGHT, -4 GVX_ERR_SHAPE
        grads = net.new_grads(True, B, T)
        assert net.backward_rc(G_d, None, B, T, tape, tbytes, grads, ws, wbytes, **kw) == want, (want, kw)
        torch.cuda.synchronize()
        assert all(torch.isnan(g).all() for g in grads.values()) and torch.isnan(ws).all()
    assert net.backward_rc(G_d, None, B, T, tape.view(torch.uint8)[1:], tb - 1, net.new_grads(True, B, T), ws, wb) == -5   # misaligned
