"""GPU: gvx_hifigan_forward_train and gvx_hifigan_backward (csrc/hifigan_train.hip) through the C ABI against float64 autograd of the
restatement in tests/hifigan_grad_ref64.py: every tape tensor, every parameter gradient and d_mel, tensor by tensor.  The tape, the
workspace and every output start as NaN; tape and workspace have exactly their stated sizes; forward_train's waveform is compared bit
for bit with gvx_hifigan_forward's in every case.

Tolerance.  Per gradient tensor, e is the largest |float32 restatement - float64| (a number of the reference alone); the device may
differ from float64 by at most 8 x max(e, 2^-23 max|g64|), the second term being one ulp of the tensor's scale - a floor for
one-element tensors such as conv_post.bias.  Tape tensors follow the forward tests' 8 x rule.  The project's vocoder tests all use
this rule.

LeakyReLU ties.  Tie-free cases assert on the CPU that no float64 pre-activation lies within 8 x its tensor's float32 error of 0 (the
mel seed is the first of 1..8 for which that holds; none: the case fails) and compare with plain autograd.  Above roughly 10^5 tape
elements no seed is tie-free, so every larger case is pinned: it reads the LeakyReLU decisions from the device's own tape, asserts that
every decision that differs from float64's is a true near-tie, and compares with the restatement pinned to those decisions.

Pieces.  The weight and bias gradients reduce every row in pieces of HGB_PIECE = 512 positions: a layer at `mul` positions per frame
has T * mul positions per row.  test_split_pieces runs B = 1 at
    T = 512, 513, 1030   the layers at mul = 1 see exactly one piece, one piece plus one position, two pieces plus a tail of 6:
                         hgb_wgrad_mfma_kernel<2> on conv_pre (NARROW 48, TWO 64 output channels; its bias sums come from the same
                         launch) and on ups.0 in its 3-tap form (96 and 128), hgb_colsum_kernel on ups.0's bias at mul = 4; the layers at mul = 4 then have 2048, 2052 and 4120 positions (four
                         pieces, four plus 4 positions, eight plus 24): hgb_wgrad_valu_kernel on NARROW's 24-channel convolutions and on
                         its ups.1 (24 columns), hgb_wgrad_mfma_kernel<1> on TWO's 32-channel convolutions, <2> on TWO's ups.1 (64); the
                         layers at mul = 8 / 16 (12 and 16 channels, and conv_post) run hgb_wgrad_valu_kernel over 8 to 33 pieces;
    T = 128, 129 (TWO)   512 and 516 positions at mul = 4: exactly one piece and one piece plus a tail for hgb_wgrad_mfma_kernel<1> and
                         the bias sums it makes, and for hgb_colsum_kernel on ups.0's bias.
With B = 1, and in every other case of one piece per row, the piece index is the position's and the row index: piece p belongs to
row p / ppr and starts at (p % ppr) * 512 only matters where B > 1 and ppr > 1.  test_pieces_across_rows runs those (shapes in
tests/backward_piece_cases.py, all pinned):
    NARROW, TWO 2 x 513                      ppr = 2 at mul = 1 with both rows full: pieces 1 and 3 hold one position;
    NARROW, TWO 3 x 1030, (513, 1, 1030)     ppr = 3 at mul = 1: row 0 is a full piece / one position / a piece behind the row, row 1
                                             one position / dead / dead, row 2 full / full / a tail of 6; ppr = 9 at mul = 4; a piece
                                             behind its row (n_st <= 0, count <= 0) must write zeros over what the workspace held:
                                             hgb_wgrad_mfma_kernel<2> on conv_pre and ups.0 with its part_b, <1> on TWO's 32-channel
                                             layers, hgb_wgrad_valu_kernel, hgb_colsum_kernel;
    MID 3 x 300, (300, 1, 129)               the matrix kernel everywhere; ppr = 3 at mul = 4, where row 2's 516 positions are a full
                                             piece, a 4-position piece and a dead one; ppr = 5 at mul = 8;
    V1 3 x 17, (17, 1, 16)                   the published widths; ppr = 3, 5, 9 at mul = 64, 128, 256; row 2 fills exactly two pieces
                                             at mul = 64 and its third is dead.
tests/test_backward_piece_layouts_cpu.py asserts from the lengths alone that each shape contains these situations.
The sizes around the 128-position tile of the data gradients and the 64-position tile of the weight gradients are the pinned cases
MID 2 x 16 / 2 x 17 (64 / 128 and 68 / 136 positions) and TWO 1 x 8 / 1 x 9 (128 and 144 positions at stage 1, under the 72-row window).

Largest error / bound ratios observed on an MI355X are recorded in DESIGN.md ("HiFi-GAN generator: tape forward and backward")."""
import functools

import pytest
import torch

from tests import backward_piece_cases as PC
from tests import hifigan_grad_ref64 as GR
from tests import hifigan_ref64 as R
from tests.hifigan_train_helpers import DEV, NAN, TrainNet, compare_grads, compare_tape, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """The NaN-filled tapes and workspaces of this module go back to the driver, not into the allocator's cache for later modules."""
    yield
    torch.cuda.empty_cache()


CFGS = dict(NARROW=R.NARROW, TWO=R.TWO, MID=R.MID, V1=R.V1,
            V1_LINEAR=dict(R.V1, slope=1.0, post_slope=1.0),   # no kinks: the same kernels against plain autograd at V1's sizes
            ODD=R.ODD, ONE=R.ONE, FOUR=R.FOUR)


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
    assert torch.equal(wav, plain), "forward_train's waveform is not gvx_hifigan_forward's, bit for bit"
    return wav, tape, grads


def _check_tie_free(name, B, T, lens=None):
    _, _, net = _net(name)
    mel, G, ref = _tie_free(name, B, T, lens)
    wav, tape, grads = _device_run(name, mel, G, lens)
    what = f"{name} {B} x {T}" + (f" lengths {lens}" if lens else "")
    print(f"{what}: largest tape error / bound {compare_tape(net.tape_views(tape, B, T), ref, lens, what):.3f}")
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
    ref = GR.reference(sd, mel, lens, cfg, G, GR.masks_from_tape(views, cfg))
    what = f"{name} {B} x {T}" + (f" lengths {lens}" if lens else "") + f" pinned ({GR.near_ties(free, lens)} near-ties, {flips} decided the other way)"
    print(f"{what}: largest tape error / bound {compare_tape(views, ref, lens, what):.3f}")
    compare_grads(grads, ref, what)
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


@pytest.mark.parametrize("name,B,T", [("NARROW", 2, 5), ("NARROW", 1, 1), ("TWO", 2, 5), ("TWO", 1, 33), ("MID", 1, 3), ("MID", 1, 1)])
def test_gradients_tie_free(name, B, T):
    """NARROW: fmaf layers throughout, K = 84 in conv_pre.  TWO: resblock 2, the 32-channel matrix tiles, 16-channel dot products.
    MID: the matrix kernels everywhere.  T = 1 puts every dilated window almost wholly outside the row."""
    _check_tie_free(name, B, T)


@pytest.mark.parametrize("name,B,T", [("MID", 2, 16), ("MID", 2, 17), ("TWO", 1, 8), ("TWO", 1, 9), ("V1", 1, 4)])
def test_gradients_pinned(name, B, T):
    """MID: 64 / 128 and 68 / 136 positions, both sides of the 128-position tile.  TWO: 128 and 144 positions at stage 1 with the
    72-row window.  V1: 512 to 32 channels, every matrix tile."""
    _check_pinned(name, B, T)


@pytest.mark.parametrize("name,B,T,lens,tie_free", [
    ("ODD", 2, 5, None, False), ("ODD", 1, 11, None, False), ("ODD", 3, 11, (11, 1, 5), False),
    ("ONE", 2, 5, None, True), ("ONE", 1, 11, None, True), ("ONE", 3, 11, (11, 1, 5), True),
    ("FOUR", 2, 5, None, True), ("FOUR", 1, 11, None, True), ("FOUR", 3, 11, (11, 1, 5), True)])
def test_configurations_no_published_shape_reaches(name, B, T, lens, tie_free):
    """ODD, ONE and FOUR of tests/hifigan_ref64.py: 37 mels in 40 padded channels through conv_pre's weight gradient and d_mel, 72 and
    36 channels (K tails of 8 and 4 in the data gradients, ups in its 3-tap form at 432 and 72 columns), 6 and 10 phases, two, one
    and four blocks per stage, slopes 0 and 1.  ONE and FOUR are small enough for a tie-free mel (with slope 0 a float64 pre-activation
    within its tensor's bound of 0 is a tie like any other); ODD's 10^5 tape elements are pinned."""
    if tie_free:
        mel, G, _, _, grads = _check_tie_free(name, B, T, lens)
        if lens is not None:
            _check_rows_alone(name, mel, G, lens, grads)
    else:
        _check_pinned(name, B, T, lens)


def test_gradients_v1_sizes_without_kinks():
    """slope = post_slope = 1: LeakyReLU is the identity, so plain float64 autograd is the reference at V1's sizes, with no tape
    reading."""
    name, B, T = "V1_LINEAR", 1, 4
    cfg, sd, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, 1), _cotangent(cfg, B, T)
    ref = GR.reference(sd, mel, None, cfg, G)
    wav, tape, grads = _device_run(name, mel, G, None)
    compare_tape(net.tape_views(tape, B, T), ref, None, name)
    compare_grads(grads, ref, name)


@pytest.mark.parametrize("name,T", [("NARROW", 512), ("NARROW", 513), ("NARROW", 1030), ("TWO", 512), ("TWO", 513), ("TWO", 1030), ("TWO", 128),
                                    ("TWO", 129)])
def test_split_pieces(name, T):
    """Reduction lengths of one piece, one piece plus one position, two pieces plus a tail, for every weight-gradient kernel and the
    bias sums (the module docstring names the layers)."""
    _check_pinned(name, 1, T)


@pytest.mark.parametrize("name,B,T,lens", PC.HIFIGAN_CASES)
def test_pieces_across_rows(name, B, T, lens):
    """Several rows with several pieces each in one call, padded and ragged (the module docstring says what each shape reaches;
    tests/test_backward_piece_layouts_cpu.py asserts that it does).  The ragged cases also assert what test_ragged_rows asserts."""
    _check_pinned(name, B, T, lens)


@pytest.mark.parametrize("name,T,lens", [("NARROW", 9, (4, 9, 5)), ("MID", 17, (4, 17, 8))])
def test_ragged_rows(name, T, lens):
    """NaN in mel at and behind each length and in d_wav at and behind T_b * hop.  Parameter gradients equal the float64 sum of the
    rows run alone (that is what the reference computes); d_mel of every row is bit-equal to that row run alone and exactly 0 behind
    its length.  MID: the 4-frame row has 32 positions at the last stage and leaves the second 128-position tile empty.  The rows'
    LeakyReLU decisions are pinned to the device's where no mel seed is tie-free (MID)."""
    cfg, sd, net = _net(name)
    B, hop = len(lens), R.hop(cfg)
    if name == "NARROW":
        mel, G, ref, tape, grads = _check_tie_free(name, B, T, lens)
    else:
        mel, G = R.random_mel(cfg, B, T, 1), _cotangent(cfg, B, T)
        wav, tape, grads = _device_run(name, mel, G, lens)
        views = [v.cpu().clone() for v in net.tape_views(tape, B, T)]
        free = GR.reference(sd, mel, lens, cfg, G)
        for i, mul in enumerate(GR.tape_muls_of(free)):
            for b, t in enumerate(lens):
                views[i][b, :, t * mul:] = 0.0   # behind a row the tape holds what it held
            if i:
                differ = (views[i] > 0) != (free["tape"][i] > 0)
                assert (free["tape"][i][differ].abs() <= GR.FACTOR * free["tape_err"][i]).all(), f"tape tensor {i}: a sign differs from float64 away from 0"
        ref = GR.reference(sd, mel, lens, cfg, G, GR.masks_from_tape(views, cfg))
        what = f"{name} {B} x {T} lengths {lens} pinned"
        compare_tape(views, ref, lens, what)
        compare_grads(grads, ref, what)
    for b, t in enumerate(lens):
        assert not grads["mel"][b, :, t:].any(), f"row {b}: d_mel is not 0 behind its {t} frames"
        mel_d, G_d = poisoned(mel[b:b + 1, :, :t].contiguous(), G[b:b + 1, :t * hop].contiguous(), None, hop)
        _, tape_b = net.forward_train(mel_d)
        alone = net.backward(G_d, None, 1, t, tape_b)
        assert torch.equal(alone["mel"][0], grads["mel"][b, :, :t]), f"row {b}: d_mel differs from that row run alone"


def test_determinism_null_d_mel_and_dirty_workspace():
    """Two backward calls give the same bits; d_mel_out = NULL changes no bit of a parameter gradient; the workspace is exactly
    gvx_hifigan_backward_workspace_bytes with a NaN guard behind it that stays NaN, and a reused (dirty) one gives the same bits."""
    name, B, T, lens = "MID", 3, 17, (4, 17, 8)
    cfg, _, net = _net(name)
    mel, G = R.random_mel(cfg, B, T, 1), _cotangent(cfg, B, T)
    mel_d, G_d = poisoned(mel, G, lens, R.hop(cfg))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _, tape = net.forward_train(mel_d, lens_d)
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
    """A short or misaligned tape, a short workspace, a missing name, a wrong element count, a NULL destination, B and T as the forward
    refuses them: each returns its code and leaves every output NaN."""
    name, B, T = "NARROW", 2, 5
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
    cases = ((-5, {}, B, T, tb - 1, wb), (-5, {}, B, T, tb, wb - 1), (-3, dict(skip=("resblocks.4.convs2.1.bias",)), B, T, tb, wb),
             (-4, dict(numel={"ups.0.weight": 7}), B, T, tb, wb), (-4, dict(null=("conv_post.bias",)), B, T, tb, wb),
             (-1, {}, 0, T, tb, wb), (-1, {}, B, 0, tb, wb), (-2, {}, 1, 32769, tb, wb))       # -1 INVALID_ARG, -2 UNSUPPORTED, -3 MISSING_WEIGHT, -4 SHAPE
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
