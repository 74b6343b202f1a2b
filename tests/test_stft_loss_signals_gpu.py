"""GPU: gvx_stft_loss through the C ABI on signals that are not noise - the cases of tests/stft_loss_ref64.SIGNAL_CASES, held to their
promises on the CPU by tests/test_stft_loss_signals_cpu.py - against the float64 restatement: digital silence beside noise (whole
frames under the clamp next to live ones, silent edges under the reflection, a target that is silent throughout), the same stretches
hushed to 2^-20 instead (powers far below eps that are not 0: only there does the clamp's derivative multiply a spectrum that is
not 0), tones 70 dB above their noise floor, noise at 2^15 and 2^-6 of unit scale, and a row equal to its target beside rows that are not.

Everything is as in tests/test_stft_loss_gpu.py: the plan of tests/stft_loss_helpers.py (workspace NaN-filled at its exact size, NaN
behind every n_b), the bound 8 x max(float32 twin error, 2^-23 x scale) per tensor, a number of the reference alone, and the gradient
pinned to the device's own signs after every differing sign is shown to be a near-tie.  Each case also runs with w_mag = 0 against
plain autograd.  The largest error / bound ratio per tensor is printed as the tests go."""
import functools

import pytest
import torch

from tests import stft_loss_ref64 as R
from tests.stft_loss_helpers import Plan, device_signs, ratio

pytestmark = pytest.mark.gpu

GATED = [n for n, c in R.SIGNAL_CASES.items() if c[1] is R.gated_case]
SQRT_EPS = torch.tensor(R.EPS, dtype=torch.float32).sqrt()   # sqrtf(eps) of the float32 eps the plan holds
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    print("signal cases, largest error / bound per tensor: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(WORST.items())))
    torch.cuda.empty_cache()


def _note(what, tensor, r):
    WORST[tensor] = max(WORST.get(tensor, 0.0), r)
    print(f"  {what}: {tensor} at {r:.3f} of its bound (largest so far {WORST[tensor]:.3f})")
    return r


def _check(dev, ref, err, what, tensor):
    r = _note(what, tensor, ratio(dev, ref, err))
    assert r <= 1.0, f"{what}: {tensor} differs from float64 by {r:.3f} of 8 x max(e = {err:.3e}, one ulp of {float(ref.abs().max()):.3e})"


def _check_grad_tail(out, lengths):
    for b, n in enumerate(lengths):
        assert bool((out["d_pred"][b, n:] == 0).all()), f"row {b}: d_pred behind n_b is not exact zeros"
    assert bool(torch.isfinite(out["d_pred"]).all())


@functools.lru_cache(maxsize=None)
def _device(name):
    """One call with the debug pointers per case, shared by the tests that read it."""
    case = R.signal_case(name)
    return Plan(case["res"]).run(case["pred"], case["target"], case["lengths"], want_dbg=True)


@pytest.mark.parametrize("name", list(R.SIGNAL_CASES))
def test_value_magnitudes_and_pinned_gradient(name):
    case = R.signal_case(name)
    res, lengths, free = case["res"], case["lengths"], case["ref"]
    e, B = free["err"], len(lengths)
    print(f"{name}: seed {case['seed']}; float32 twin errors: loss {e['loss']:.3e} parts {e['parts']:.3e} Mp {max(e['Mp']):.3e} Mt {max(e['Mt']):.3e}")
    out = _device(name)
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["parts"]).all())
    _check(out["loss"], free["loss"], e["loss"], name, "loss")
    for b in range(B):   # row by row: a silent target's row is 1e4 times the row beside it
        if bool(free["parts"][b].any()):   # the equal row of the mixed case: exact zeros, asserted as such
            _check(out["parts"][b], free["parts"][b], e["parts_rows"][b], f"{name} row {b}", "parts")
        else:
            assert bool((out["parts"][b] == 0).all())
    for r, (n_fft, hop, _) in enumerate(res):
        for k in ("Mp", "Mt"):
            dev = torch.cat([out[k][r][b, :R.frames(lengths[b], hop)].reshape(-1) for b in range(B)])
            want = torch.cat([free[k][b][r].reshape(-1) for b in range(B)])
            _check(dev, want, e[k][r], name, f"{k}[{r}]")
    signs = device_signs(out, lengths, res, case["n_max"])
    flips, ties = R.sign_flips_are_near_ties(free, signs)
    pinned = R.reference(case["pred"], case["target"], lengths, res, signs=signs)
    print(f"  {ties} near-ties, {flips} decided the other way; pinned d_pred twin error {pinned['err']['d_pred']:.3e} "
          f"of scale {float(pinned['d_pred'].abs().max()):.3e}")
    for b in range(B):
        if bool(pinned["d_pred"][b].any()):   # the equal row of the mixed case: exact zeros, asserted as such below
            _check(out["d_pred"][b], pinned["d_pred"][b], pinned["err"]["d_pred_rows"][b], f"{name} row {b} pinned", "d_pred")
        else:
            assert bool((out["d_pred"][b] == 0).all())
    _check_grad_tail(out, lengths)


@pytest.mark.parametrize("name", list(R.SIGNAL_CASES))
def test_smooth_term_alone_against_plain_autograd(name):
    """w_mag = 0: spectral convergence has no sign decisions, so float64 autograd of the restatement is the reference as it stands."""
    case = R.signal_case(name)
    ref = R.reference(case["pred"], case["target"], case["lengths"], case["res"], w_mag=0.0)
    print(f"{name} w_mag = 0: d_pred twin error {ref['err']['d_pred']:.3e} of scale {float(ref['d_pred'].abs().max()):.3e}")
    out = Plan(case["res"], w_mag=0.0).run(case["pred"], case["target"], case["lengths"])
    _check(out["loss"], ref["loss"], ref["err"]["loss"], name + " smooth", "loss")
    for b in range(len(case["lengths"])):
        if bool(ref["d_pred"][b].any()):
            _check(out["d_pred"][b], ref["d_pred"][b], ref["err"]["d_pred_rows"][b], f"{name} row {b} smooth", "d_pred (w_mag = 0)")
        else:
            assert bool((out["d_pred"][b] == 0).all())
    _check_grad_tail(out, case["lengths"])


# ---- exact properties

@pytest.mark.parametrize("name", GATED)
def test_silent_frames_sit_on_the_clamp_and_pass_no_gradient(name):
    """Every bin of a silent frame - or a hushed one, whose powers are far below eps without being 0 - has the magnitude sqrtf(eps) bit
    for bit, in both signals, and no live frame lies there; both-silent bins carry the sign 0; d_pred is exactly 0 on every sample
    that only clamped frames of pred read."""
    case = R.signal_case(name)
    res, lengths, free = case["res"], case["lengths"], case["ref"]
    out = _device(name)
    signs = device_signs(out, lengths, res, case["n_max"])
    for key, dev in (("Xp", out["Mp"]), ("Xt", out["Mt"])):
        sil = R.clamped_frames(free, key)
        for b in range(len(lengths)):
            for r in range(len(res)):
                M = dev[r][b, :len(sil[b][r])]
                assert bool((M[sil[b][r]] == SQRT_EPS).all()), f"{name}: {key} row {b} resolution {r}: a silent frame is off sqrtf(eps)"
                assert bool((M[~sil[b][r]] > SQRT_EPS).any(dim=1).all()), f"{name}: {key} row {b} resolution {r}: a live frame sits at the clamp"
    sp, st = R.clamped_frames(free, "Xp"), R.clamped_frames(free, "Xt")
    for b in range(len(lengths)):
        for r in range(len(res)):
            both = sp[b][r] & st[b][r]
            assert bool((signs[b][r][both] == 0).all()) and bool((signs[b][r][sp[b][r] & ~st[b][r]] == 1).all())
            assert bool((signs[b][r][~sp[b][r] & st[b][r]] == -1).all())
    live = R.live_support(free, lengths, res, case["n_max"])
    assert bool((out["d_pred"][~live] == 0).all()), f"{name}: a gradient came through the clamp"
    assert bool((out["d_pred"][live] != 0).any())
    smooth = Plan(res, w_mag=0.0).run(case["pred"], case["target"], lengths)
    assert bool((smooth["d_pred"][~live] == 0).all())


def test_a_silent_target_row_is_large_finite_and_within_its_own_bound():
    """gated_r512, row 1: the target is silent throughout, so the spectral-convergence denominator is sqrt(eps x count) and the term
    about 1e4.  Held on its own, not under the batch's largest value: the row run alone, loss and parts against float64."""
    case = R.signal_case("gated_r512")
    n = case["lengths"][1]
    pred, target = case["pred"][1:2, :n], case["target"][1:2, :n]
    assert not bool(target.any()) and bool(pred.any())
    ref = R.reference(pred, target, None, case["res"])
    assert 1e4 < float(ref["parts"][0, 0, 0]) < 1e5
    out = Plan(case["res"]).run(pred, target, None)
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["parts"]).all()) and bool(torch.isfinite(out["d_pred"]).all())
    _check(out["loss"], ref["loss"], ref["err"]["loss"], "silent target row", "loss")
    _check(out["parts"], ref["parts"], ref["err"]["parts"], "silent target row", "parts")
    both = _device("gated_r512")
    assert torch.equal(both["parts"][1], out["parts"][0])   # and in the batch the row's parts are these bits


def test_an_equal_row_beside_unequal_rows():
    """mixed_equal_r512: row 0 equals its target bit for bit - its parts and its gradient are exact zeros (the ||D|| = 0 side of the
    reduce kernel's coefficient) while rows 1 and 2 of the same call take the other side (held to their own rows' bounds by the two
    tests above); row 1 is equal on its first half, where every sign is 0.  Row 0's bits do not change when the rows beside it do."""
    case = R.signal_case("mixed_equal_r512")
    res, lengths = case["res"], case["lengths"]
    out = _device("mixed_equal_r512")
    assert bool((out["parts"][0] == 0).all()) and bool((out["d_pred"][0] == 0).all())
    assert bool((out["Mp"][0][0, :R.frames(lengths[0], res[0][1])] == out["Mt"][0][0, :R.frames(lengths[0], res[0][1])]).all())
    signs = device_signs(out, lengths, res, case["n_max"])
    assert bool((signs[0][0] == 0).all()) and bool((signs[1][0] == 0).all(dim=1).any()) and bool((signs[2][0] != 0).any())
    g = torch.Generator().manual_seed(91)
    pred, target = case["pred"].clone(), case["target"].clone()
    pred[1:], target[1:] = torch.randn(2, case["n_max"], generator=g), torch.randn(2, case["n_max"], generator=g)
    other = Plan(res).run(pred, target, lengths, want_dbg=True)
    assert torch.equal(other["parts"][0], out["parts"][0]) and torch.equal(other["d_pred"][0], out["d_pred"][0])
    F0 = R.frames(lengths[0], res[0][1])
    assert torch.equal(other["Mp"][0][0, :F0], out["Mp"][0][0, :F0]) and torch.equal(other["Mt"][0][0, :F0], out["Mt"][0][0, :F0])
    assert not torch.equal(other["parts"][1:], out["parts"][1:])


@pytest.mark.parametrize("name", ["loud_r2048", "quiet_r2048"])
def test_parts_do_not_depend_on_the_scale(name):
    """Both signals times 2^15 or 2^-6.  The loss is invariant to a common scale except through eps, and these cases clamp nothing
    (at 1e-3 of unit scale some bins do fall below eps): the device's parts of the scaled signals are held to float64's parts of the
    UNSCALED ones, within the scaled case's own bound.  The gradient scales by the inverse; the first test holds it to float64."""
    case, unit = R.signal_case(name), R.signal_case("unit_r2048")
    out = _device(name)
    _check(out["parts"], unit["ref"]["parts"], case["ref"]["err"]["parts"], name + " against unit scale", "parts")
    _check(out["loss"], unit["ref"]["loss"], case["ref"]["err"]["loss"], name + " against unit scale", "loss")
