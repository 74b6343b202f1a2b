"""GPU: gvx_stft_loss (csrc/stft_loss.hip) through the C ABI against the float64 restatement in tests/stft_loss_ref64.py: the loss, its
parts, every resolution's magnitudes of both signals (read through the call's debug pointers) and d_pred.  The workspace, d_pred, the
outputs and everything behind n_b in both inputs start as NaN; the workspace has exactly its stated size.

Tolerance (the rule of test_melgan_backward_gpu.py).  Per tensor, e is the largest |float32 twin - float64| on the CPU, a number of
the reference alone, printed per case; the device may differ from float64 by at most 8 x max(e, 2^-23 max|ref64|).

Sign ties.  d|log M_t - log M_p| takes a sign per bin, and unit-variance noise always holds bins where float32 and float64 may decide
it differently.  So the gradient is pinned: the device's magnitudes are read back, its signs sign(M_t - M_p) are taken, every sign
that differs from float64's is asserted to be a true near-tie (|dlog64| <= 8 (E_f(pred) / M_p + E_f(target) / M_t), E_f the twin's
largest complex error in that frame), and d_pred is compared with float64 autograd of the restatement pinned to those signs.  Each
shape also runs once with w_mag = 0, the smooth term alone, against plain autograd.  Each case asserts that no float64 power lies
within [eps / 2, 2 eps] (unit-variance noise, the first seed of 1..8 for which that holds).

Shapes.  G = 4 frames per workgroup, S = 256 samples per gather workgroup.  S - 1, S, S + 1 are below the shortest legal row of the
smallest n_fft (257 samples), so the gather's edge is taken at 2 S and 3 S.  Nothing is longer than 8192 samples."""
import functools

import pytest
import torch

from tests import stft_loss_ref64 as R
from tests.stft_loss_helpers import DEV, G, NAN, S, Plan, device_signs, poisoned, ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


# name: (resolutions, lengths of the 3 rows or None, n_max)
CASES = {
    # n_fft 512, win_length == n_fft, hop 128: the shortest legal row (both reflections cover the whole row and overlap each other's
    # frames); k hop - 1 and k hop at k = 3 (3 frames, then G = 4)
    "r512_shortest_khop": (((512, 128, 512),), (257, 383, 384), 400),
    # k hop + 1; G + 1 = 5 frames (512 = 4 hop); 2 G = 8 frames (896 = 7 hop); 2 S = 512
    "r512_frames_g": (((512, 128, 512),), (385, 512, 896), 900),
    # win_length < n_fft; 2 S - 1, 2 S, 2 S + 1
    "r512_gather_2s": (((512, 50, 240),), (2 * S - 1, 2 * S, 2 * S + 1), 520),
    "r512_odd_win": (((512, 100, 301),), (257, 400, 601), 640),
    # hop == n_fft: no overlap, one frame covers a sample (plus the reflections)
    "r512_hop_is_nfft": (((512, 512, 512),), (257, 1024, 1025), 1030),
    "r1024_short_win": (((1024, 120, 600),), (513, 1025, 1200), 1210),
    "r1024_odd_win_3s": (((1024, 256, 1023),), (3 * S - 1, 3 * S, 3 * S + 1), 770),
    "r1024_full_win": (((1024, 256, 1024),), (513, 1024, 1279), 1300),
    "r1024_hop_is_nfft": (((1024, 1024, 1024),), (513, 2047, 2048), 2048),
    "r2048_full_win": (((2048, 512, 2048),), (1025, 2048, 2049), 2100),
    "r2048_odd_win": (((2048, 240, 1199),), (1025, 2047, 3000), 3000),
    "r2048_hop_is_nfft": (((2048, 2048, 2048),), (1025, 4096, 4097), 4100),
    # R = 3, the default resolutions: the shortest row, rows crossing frame and workgroup edges of all three, n_max beyond the longest
    "default_ragged": (R.DEFAULT_RESOLUTIONS, (1025, 2400, 4097), 4200),
    "default_one_row": (R.DEFAULT_RESOLUTIONS, None, 1025),
    "default_long": (R.DEFAULT_RESOLUTIONS, (8192, 5000), 8192),
}
WORST = {}


def _shape(name):
    res, lengths, n_max = CASES[name]
    return res, (None if lengths is None else list(lengths)), n_max, (1 if lengths is None else len(lengths))


@functools.lru_cache(maxsize=None)
def _free(name):
    """(seed, pred, target, free float64 reference) of a case: computed once, shared by the tests, never changed."""
    res, lengths, n_max, B = _shape(name)
    seed, pred, target, ref = R.noise_case(B, n_max, lengths, res)
    assert R.eps_clear(ref)
    return seed, pred, target, ref


def _note(what, tensor, r):
    WORST[tensor] = max(WORST.get(tensor, 0.0), r)
    print(f"  {what}: {tensor} at {r:.3f} of its bound (largest so far {WORST[tensor]:.3f})")
    return r


def _check(dev, ref, err, what, tensor):
    r = _note(what, tensor, ratio(dev, ref, err))
    assert r <= 1.0, f"{what}: {tensor} differs from float64 by {r:.3f} of 8 x max(e = {err:.3e}, one ulp of {float(ref.abs().max()):.3e})"


def _check_grad_tail(out, lengths, n_max):
    if lengths is not None:
        for b, n in enumerate(lengths):
            assert bool((out["d_pred"][b, n:] == 0).all()), f"row {b}: d_pred behind n_b is not exact zeros"
    assert bool(torch.isfinite(out["d_pred"]).all())


@pytest.mark.parametrize("name", list(CASES))
def test_value_magnitudes_and_pinned_gradient(name):
    res, lengths, n_max, B = _shape(name)
    seed, pred, target, free = _free(name)
    e = free["err"]
    print(f"{name}: seed {seed}; float32 twin errors: loss {e['loss']:.3e} parts {e['parts']:.3e} Mp {max(e['Mp']):.3e} Mt {max(e['Mt']):.3e}")
    out = Plan(res).run(pred, target, lengths, want_dbg=True)
    _check(out["loss"], free["loss"], e["loss"], name, "loss")
    _check(out["parts"], free["parts"], e["parts"], name, "parts")
    lens = [n_max] * B if lengths is None else lengths
    for r, (n_fft, hop, _) in enumerate(res):
        for k in ("Mp", "Mt"):
            dev = torch.cat([out[k][r][b, :R.frames(lens[b], hop)].reshape(-1) for b in range(B)])
            want = torch.cat([free[k][b][r].reshape(-1) for b in range(B)])
            _check(dev, want, e[k][r], name, f"{k}[{r}]")
    signs = device_signs(out, lengths, res, n_max)
    flips, ties = R.sign_flips_are_near_ties(free, signs)
    pinned = R.reference(pred, target, lengths, res, signs=signs)
    print(f"  {ties} near-ties, {flips} decided the other way; pinned d_pred twin error {pinned['err']['d_pred']:.3e} "
          f"of scale {float(pinned['d_pred'].abs().max()):.3e}")
    _check(out["d_pred"], pinned["d_pred"], pinned["err"]["d_pred"], name + " pinned", "d_pred")
    _check_grad_tail(out, lengths, n_max)


@pytest.mark.parametrize("name", list(CASES))
def test_smooth_term_alone_against_plain_autograd(name):
    """w_mag = 0: spectral convergence has no sign decisions, so float64 autograd of the restatement is the reference as it stands."""
    res, lengths, n_max, B = _shape(name)
    seed, pred, target, _ = _free(name)
    ref = R.reference(pred, target, lengths, res, w_mag=0.0)
    print(f"{name} w_mag = 0: d_pred twin error {ref['err']['d_pred']:.3e} of scale {float(ref['d_pred'].abs().max()):.3e}")
    out = Plan(res, w_mag=0.0).run(pred, target, lengths)
    _check(out["loss"], ref["loss"], ref["err"]["loss"], name + " smooth", "loss")
    _check(out["d_pred"], ref["d_pred"], ref["err"]["d_pred"], name + " smooth", "d_pred (w_mag = 0)")
    _check_grad_tail(out, lengths, n_max)


# ---- exact properties

@pytest.mark.parametrize("name", ["r512_frames_g", "r1024_odd_win_3s", "default_ragged"])
def test_ragged_row_is_the_row_run_alone(name):
    """parts of a row are the bits of the row run alone (B = 1, n_max = n_b).  d_pred carries the loss's 1 / (B R): a row's gradient is
    the bits of that row in ANY batch of the same size - other companions, another slot, another n_max - and, the factor being a
    power of two there, exactly half of the row run alone when it sits in a batch of two."""
    res, lengths, n_max, B = _shape(name)
    _, pred, target, _ = _free(name)
    plan = Plan(res)
    out = plan.run(pred, target, lengths)
    g = torch.Generator().manual_seed(77)
    for b, n in enumerate(lengths):
        alone = plan.run(pred[b:b + 1, :n], target[b:b + 1, :n], None)
        assert torch.equal(alone["parts"][0], out["parts"][b]), f"row {b}: parts differ from the row run alone"
        # another batch of three: the row in slot (b + 1) % 3, new companions of other lengths, a longer n_max
        slot, n2 = (b + 1) % B, n_max + 37
        p2, t2 = torch.randn(B, n2, generator=g), torch.randn(B, n2, generator=g)
        p2[slot, :n], t2[slot, :n] = pred[b, :n], target[b, :n]
        l2 = [max(res_[0] for res_ in res) // 2 + 1 + 11 * i for i in range(B)]
        l2[slot] = n
        other = plan.run(p2, t2, l2)
        assert torch.equal(other["parts"][slot], out["parts"][b])
        assert torch.equal(other["d_pred"][slot, :n], out["d_pred"][b, :n]), f"row {b}: d_pred depends on the rows beside it"
        pair = plan.run(torch.stack([p2[0, :n], pred[b, :n]]), torch.stack([t2[0, :n], target[b, :n]]), [l2[0] if l2[0] <= n else n, n])
        assert torch.equal(pair["d_pred"][1] * 2, alone["d_pred"][0]), f"row {b}: d_pred in a batch of two is not half the row run alone"


def test_two_calls_give_equal_bits_on_a_reused_workspace():
    res, lengths, n_max, B = _shape("default_ragged")
    _, pred, target, _ = _free("default_ragged")
    plan = Plan(res)
    lens_d = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    p, t = poisoned(pred, lengths), poisoned(target, lengths)
    ws = torch.full((plan.ws_bytes(B, n_max) // 4,), NAN, dtype=torch.float32, device=DEV)
    a = plan.raw(p, t, lens_d, ws=ws)
    other = Plan(((512, 128, 512),))   # another plan dirties the same buffer in between
    assert other.raw(p, t, lens_d, ws=ws[: other.ws_bytes(B, n_max) // 4])[0] == 0
    b = plan.raw(p, t, lens_d, ws=ws)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    # d_pred = NULL: the same loss and parts bits; parts = NULL as well
    c = plan.raw(p, t, lens_d, want_grad=False)
    d = plan.raw(p, t, lens_d, want_grad=False, want_parts=False)
    assert c[0] == 0 and d[0] == 0 and torch.equal(c[1], a[1]) and torch.equal(c[2], a[2]) and torch.equal(d[1], a[1])


@pytest.mark.parametrize("name", ["r512_shortest_khop", "default_ragged"])
def test_equal_signals_and_silence(name):
    res, lengths, n_max, B = _shape(name)
    _, pred, target, _ = _free(name)
    plan = Plan(res)
    same = plan.run(target, target, lengths)
    assert float(same["loss"]) == 0.0 and bool((same["parts"] == 0).all()) and bool((same["d_pred"] == 0).all())
    silent = plan.run(torch.zeros_like(pred), target, lengths)   # every power of pred is below eps: the clamp passes no gradient
    assert bool(torch.isfinite(silent["loss"])) and float(silent["loss"]) > 0 and bool((silent["d_pred"] == 0).all())


def test_refusals():
    """Each refusal gives its status; what is refused on the host launches nothing (every output keeps its NaN), and a row refused by
    its device-side length leaves only defined values: NaN loss, NaN parts of that row, an all-zero gradient."""
    res = R.DEFAULT_RESOLUTIONS
    plan = Plan(res)
    B, n_max = 3, 1500
    g = torch.Generator().manual_seed(5)
    p, t = torch.randn(B, n_max, generator=g).to(DEV), torch.randn(B, n_max, generator=g).to(DEV)
    for lengths, row in (([1500, 1024, 1300], 1), ([1025, 1200, 1501], 2), ([0, 1200, 1500], 0), ([1500, 1500, -3], 2)):
        rc, loss, parts, d_pred, _, _ = plan.raw(p, t, torch.tensor(lengths, dtype=torch.int32, device=DEV))
        assert rc == -4 and f"row {row} ".encode() in plan.lib.gvx_last_error(), (lengths, plan.lib.gvx_last_error())
        assert bool(torch.isnan(loss).all()) and bool((d_pred == 0).all()) and bool(torch.isnan(parts[row]).all())
        assert bool(torch.isfinite(parts[[b for b in range(B) if b != row]]).all())
    untouched = lambda out: all(bool(torch.isnan(x).all()) for x in out[1:4])
    short = plan.raw(p[:, :1024].contiguous(), t[:, :1024].contiguous(), None)           # n_max below n_fft_max / 2 + 1
    assert short[0] == -4 and untouched(short)
    need = plan.ws_bytes(B, n_max)
    ws = torch.full((need // 4 + 64,), NAN, dtype=torch.float32, device=DEV)
    small = plan.raw(p, t, None, ws=ws, ws_bytes=need - 1)
    assert small[0] == -5 and b"too small" in plan.lib.gvx_last_error() and untouched(small)
    skew = plan.raw(p, t, None, ws=ws[1:])
    assert skew[0] == -5 and b"256-byte aligned" in plan.lib.gvx_last_error() and untouched(skew)
    lib = plan.lib
    one = torch.zeros(1, device=DEV)
    assert lib.gvx_stft_loss(plan.h, None, t.data_ptr(), None, B, n_max, one.data_ptr(), None, None, None, ws.data_ptr(), need, None) == -1
    assert lib.gvx_stft_loss(plan.h, p.data_ptr(), t.data_ptr(), None, 0, n_max, one.data_ptr(), None, None, None, ws.data_ptr(), need, None) == -1
    assert lib.gvx_stft_loss(None, p.data_ptr(), t.data_ptr(), None, B, n_max, one.data_ptr(), None, None, None, ws.data_ptr(), need, None) == -1
    ok = plan.raw(p, t, None, ws=ws)   # the same buffers serve a good call afterwards
    assert ok[0] == 0 and bool(torch.isfinite(ok[1]).all()) and bool(torch.isfinite(ok[3]).all())


def test_case_table_reaches_what_it_promises():
    """Every supported n_fft as a single-resolution plan with win_length == n_fft, < n_fft and odd, and with hop == n_fft; frame counts
    G, G + 1 and 2 G; lengths k hop - 1, k hop, k hop + 1; the gather's workgroup edge; R = 1 and R = 3; nothing beyond 8192 samples."""
    single = [(c[0][0], c[1]) for c in CASES.values() if len(c[0]) == 1]
    for n_fft in (512, 1024, 2048):
        mine = [r for r, _ in single if r[0] == n_fft]
        assert any(w == n_fft for _, _, w in mine) and any(w < n_fft for _, _, w in mine) and any(w % 2 for _, _, w in mine)
        assert any(h == n_fft for _, h, _ in mine)
        assert any(n_fft // 2 + 1 in lens for r, lens in single if r[0] == n_fft)
    counts = {R.frames(n, r[1]) for r, lens in single for n in lens}
    assert {G, G + 1, 2 * G} <= counts
    assert any({k * r[1] - 1, k * r[1], k * r[1] + 1} <= {n for r2, lens in single if r2 == r for n in lens} for r, _ in single for k in (2, 3, 4))
    assert any({m * S - 1, m * S, m * S + 1} <= set(lens) for _, lens in single for m in (2, 3))
    assert {len(c[0]) for c in CASES.values()} == {1, 3}
    assert all(c[2] <= 8192 for c in CASES.values()) and any(c[1] is not None and c[2] > max(c[1]) for c in CASES.values())
