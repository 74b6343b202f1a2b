"""CPU: the signal cases of tests/stft_loss_ref64.py (SIGNAL_CASES: gated silence, tones, scaled noise, rows equal to their target) held
to what they promise, on the float64 restatement alone.  tests/test_stft_loss_signals_gpu.py runs the same cases on the device."""
import pytest
import torch

from tests import stft_loss_ref64 as R

GATED = [n for n, c in R.SIGNAL_CASES.items() if c[1] is R.gated_case]
UNCLAMPED = [n for n, c in R.SIGNAL_CASES.items() if c[1] in (R.tone_case, R.scaled_case, R.mixed_equal_case)]
KINDS = ("both live", "only pred silent", "only target silent", "both silent")


def _counts(case, key):
    """(clamped bins, all bins) of one signal over rows and resolutions."""
    cl = R.clamped(case["ref"], key)
    return sum(int(m.sum()) for rows in cl for m in rows), sum(m.numel() for rows in cl for m in rows)


def _kinds(case, r):
    """How many frames of resolution r are of each of the four kinds, over the rows."""
    sp, st = R.clamped_frames(case["ref"], "Xp"), R.clamped_frames(case["ref"], "Xt")
    n = [0, 0, 0, 0]
    for b in range(len(sp)):
        for kind in (sp[b][r].long() + 2 * st[b][r].long()).tolist():
            n[kind] += 1
    return n


@pytest.mark.parametrize("name", list(R.SIGNAL_CASES))
def test_every_case_is_clear_of_the_clamp_finite_and_small(name):
    case = R.signal_case(name)   # fails if no seed of 1..8 qualifies
    ref = case["ref"]
    assert 1 <= case["seed"] <= 8 and R.eps_clear(ref) and R.clamp_takes_whole_frames(ref)
    assert case["pred"].dtype == case["target"].dtype == torch.float32 and case["pred"].shape == case["target"].shape
    assert case["n_max"] <= 8192 and len(case["lengths"]) <= 3 and all(max(r[0] for r in case["res"]) // 2 < n <= case["n_max"] for n in case["lengths"])
    assert bool(torch.isfinite(ref["loss"])) and bool(torch.isfinite(ref["parts"]).all()) and bool(torch.isfinite(ref["d_pred"]).all())
    for b, n in enumerate(case["lengths"]):
        assert bool((ref["d_pred"][b, n:] == 0).all())
    print(f"{name}: seed {case['seed']}, loss {float(ref['loss']):.6g}, clamped bins pred {_counts(case, 'Xp')} target {_counts(case, 'Xt')}")


@pytest.mark.parametrize("name", GATED)
def test_gated_cases_hold_silent_and_live_frames_side_by_side(name):
    case = R.signal_case(name)
    ref, res = case["ref"], case["res"]
    cp, ct = _counts(case, "Xp"), _counts(case, "Xt")
    assert 0 < cp[0] < cp[1] and 0 < ct[0] < ct[1]
    # the clamp takes whole frames, no live frame holds a clamped bin; every clamped power is exactly 0 - or, in the hushed case, none is
    hush = len(R.SIGNAL_CASES[name][2]) > 4
    for key in ("Xp", "Xt"):
        cl, fr, sil = R.clamped(ref, key), R.clamped_frames(ref, key), R.silent_frames(ref, key)
        for b in range(len(cl)):
            for r in range(len(res)):
                assert torch.equal(cl[b][r], fr[b][r][:, None].expand_as(cl[b][r])), f"{name}: row {b} resolution {r} clamps a bin of a live frame"
                assert not bool(sil[b][r].any()) if hush else torch.equal(sil[b][r], fr[b][r])
                if hush:
                    P = ref[key][b][r].real ** 2 + ref[key][b][r].imag ** 2
                    assert bool((P[fr[b][r]] > 0).all()) and bool((P[fr[b][r]] < R.EPS / 10).all())
    kinds = [_kinds(case, r) for r in range(len(res))]
    print(f"{name}: frames per kind {dict(zip(KINDS, map(list, zip(*kinds))))}")
    assert all(sum(k[i] for k in kinds) > 0 for i in range(4)), f"{name}: a frame kind is missing: {kinds}"
    # more than one workgroup of G = 4 frames holds silent and live frames of pred together
    sp = R.clamped_frames(ref, "Xp")
    assert any(0 < int(s[r][g:g + 4].sum()) < len(s[r][g:g + 4]) for s in sp for r in range(len(res)) for g in range(0, len(s[r]), 4))
    # the float64 gradient is exactly zero wherever only clamped frames reach
    live = R.live_support(ref, case["lengths"], res, case["n_max"])
    assert bool((~live).any()) and bool(live.any()) and bool((ref["d_pred"][~live] == 0).all())
    assert bool((ref["d_pred"][live] != 0).any())


def test_every_transform_size_sees_all_four_frame_kinds():
    """Per resolution over the gated cases: each of (512, 1024, 2048) has at least one frame of every kind, and so has every single-
    resolution gated case on its own."""
    seen = {}
    for name in GATED:
        case = R.signal_case(name)
        for r, res in enumerate(case["res"]):
            k = _kinds(case, r)
            seen[res[0]] = [a + b for a, b in zip(seen.get(res[0], [0] * 4), k)]
            if len(case["res"]) == 1:
                assert all(v > 0 for v in k), f"{name}: {dict(zip(KINDS, k))}"
    assert set(seen) == {512, 1024, 2048} and all(v > 0 for k in seen.values() for v in k), seen
    singles = sorted(c[0][0][0] for c in R.SIGNAL_CASES.values() if len(c[0]) == 1)
    assert set(singles) == {512, 1024, 2048} and any(c[0] == R.DEFAULT_RESOLUTIONS for c in R.SIGNAL_CASES.values())


def test_the_two_gated_shapes_counted_by_hand():
    """gated_r512: frames of 512 samples at hop 128, 11 + 10 of them.  Row 0: pred silent in frames 5 .. 7, target in 7 .. 10 (through the
    right reflection); row 1: pred silent in frames 0 .. 2 (through the left reflection), target in all 10.  257 bins each.
    gated_default: non-zero taps within +-299 / +-599 / +-119 samples of a frame's position; pred silent in 15 + 5 + 43 frames."""
    a = R.signal_case("gated_r512")
    assert _counts(a, "Xp") == (6 * 257, 5397) and _counts(a, "Xt") == (14 * 257, 5397)
    sp, st = R.silent_frames(a["ref"], "Xp"), R.silent_frames(a["ref"], "Xt")
    assert torch.nonzero(sp[0][0]).flatten().tolist() == [5, 6, 7] and torch.nonzero(st[0][0]).flatten().tolist() == [7, 8, 9, 10]
    assert torch.nonzero(sp[1][0]).flatten().tolist() == [0, 1, 2] and bool(st[1][0].all()) and len(st[1][0]) == 10
    assert 1e4 < float(a["ref"]["parts"][1, 0, 0]) < 1e5 and 1e4 < float(a["ref"]["loss"]) < 2e4   # the silent target: sqrt(eps count) below
    d = R.signal_case("gated_default")
    assert _counts(d, "Xp") == (15 * 513 + 5 * 1025 + 43 * 257, 67487) == (23871, 67487) and _counts(d, "Xt") == (29256, 67487)


@pytest.mark.parametrize("name", UNCLAMPED)
def test_tone_scaled_and_mixed_cases_clamp_nothing(name):
    case = R.signal_case(name)
    assert _counts(case, "Xp")[0] == 0 and _counts(case, "Xt")[0] == 0


@pytest.mark.parametrize("name", [n for n, c in R.SIGNAL_CASES.items() if c[1] is R.tone_case])
def test_tone_frames_span_fifty_decibels(name):
    """The tone's peak bin against the frame's weakest: a ratio of powers of at least 1e5 in every frame (about 60 dB in most)."""
    case = R.signal_case(name)
    worst = min(float((M.amax(dim=1) / M.amin(dim=1)).min()) for k in ("Mp", "Mt") for rows in case["ref"][k] for M in rows)
    print(f"{name}: smallest per-frame ratio of magnitudes {worst:.1f} ({20 * torch.log10(torch.tensor(worst)):.1f} dB)")
    assert worst ** 2 >= 1e5


def test_scaled_cases_are_exact_scalings_with_the_parts_of_the_unit_case():
    """The loss is invariant to a common scale of both signals except through eps: with no bin clamped the float64 parts agree to
    rounding."""
    unit, loud, quiet = (R.signal_case(n) for n in ("unit_r2048", "loud_r2048", "quiet_r2048"))
    assert unit["seed"] == loud["seed"] == quiet["seed"]
    assert torch.equal(loud["pred"], unit["pred"] * 2.0 ** 15) and torch.equal(quiet["target"] * 2.0 ** 6, unit["target"])
    for other in (loud, quiet):
        assert float((other["ref"]["parts"] - unit["ref"]["parts"]).abs().max()) <= 1e-12 * float(unit["ref"]["parts"].abs().max())


def test_mixed_equal_case_has_an_equal_row_beside_unequal_ones():
    case = R.signal_case("mixed_equal_r512")
    ref, (n0, n1, n2) = case["ref"], case["lengths"]
    assert torch.equal(case["pred"][0], case["target"][0]) and torch.equal(case["pred"][1, :n1 // 2], case["target"][1, :n1 // 2])
    assert not bool((case["pred"][1, n1 // 2:n1] == case["target"][1, n1 // 2:n1]).any()) and not bool((case["pred"][2] == case["target"][2]).any())
    assert bool((ref["parts"][0] == 0).all()) and bool((ref["d_pred"][0] == 0).all())
    assert bool((ref["parts"][1:] > 0).all()) and bool((ref["d_pred"][1, n1 // 2:n1] != 0).all()) and bool((ref["d_pred"][2, :n2] != 0).all())
    u = torch.log(ref["Mt"][1][0]) - torch.log(ref["Mp"][1][0])
    assert bool((u == 0).all(dim=1).any()) and bool((u != 0).all(dim=1).any())   # row 1: frames with sign 0 throughout beside frames without
