"""CPU: the cases of tests/pitch_edge_cases.py on the references alone.  Every YIN case respects the cap on marginal frames that
tests.test_pitch_gpu.hold applies on the device (5 % of the case's frames), and every case reaches the path it is named for - from
the parameters and from the references, before a GPU is involved."""
import numpy as np
import pytest

from genvox_amd import _lib
from tests import pitch_edge_cases as C
from tests import psola_ref as R

YIN_NAMES = [c.name for c in C.YIN_CASES]
PSOLA_NAMES = [c.name for c in C.PSOLA_CASES]


@pytest.mark.parametrize("name", YIN_NAMES)
def test_yin_marginal_cap(name):
    case = C.YIN_BY_NAME[name]
    _, ref = C.yin_reference(case)
    marginal, total = C.marginal_frames(ref, case.p)
    print(f"{name}: {marginal} marginal of {total} frames")
    assert total == sum(-(-n // case.p["hop"]) for n in case.lengths) and total > 0
    assert marginal <= 0.05 * total, (name, marginal, total)


def test_yin_cases_reach_their_paths():
    lib = _lib.load()
    for case in C.YIN_CASES:
        p = case.p
        if "tail" in case.claims:
            assert p["window"] % 64 != 0, case.name
        if "mod3" in case.claims:
            assert (p["lag_max"] + 1) % 3 == 1, case.name
    assert {c.p["window"] for c in C.WINDOW_CASES if "tail" in c.claims} == {32, 33, 63, 65, 100, 127, 1000, 2047}
    assert {c.p["lag_max"] for c in C.LAG_CASES if "mod3" in c.claims} == {42, 192}
    assert [c.p["lag_max"] + 1 for c in C.LAG_CASES[6:9]] == [192, 193, 194]          # a pass of the kernel is 3 * 64 lags
    assert [-(-c.p["lag_max"] // 64) for c in C.LAG_CASES[2:6]] == [1, 2, 2, 3]       # lags of a lane in the running sum
    for case in C.TILE_CASES:
        hop = case.p["hop"]
        tile, F = C.TILE_FRAMES[hop]
        q = _lib.gvx_pitch_params(case.p["sampling_rate"], hop, case.p["window"], case.p["lag_min"], case.p["lag_max"], case.p["threshold"], 0)
        assert lib.gvx_pitch_tile_frames(q) == tile, case.name
        frames = [-(-n // hop) for n in case.lengths]
        assert frames[0] == F and F > tile and (F % tile != 0 or tile == 1) and frames[1] == F - 1 and 0 < frames[2] <= tile, case.name
    assert [C.TILE_FRAMES[h][0] for h in (700, 1024, 4096, 9300)] == [14, 9, 3, 1]
    # the threshold no frame reaches: every frame of the case is unvoiced in the reference
    case = C.YIN_BY_NAME["threshold1e-06"]
    _, ref = C.yin_reference(case)
    assert (ref["lag"] == -1).all()
    for name in ("threshold0.5", "threshold0.9", "lag4_42", "lag4_192", "W33", "W127"):
        _, ref = C.yin_reference(C.YIN_BY_NAME[name])
        unvoiced = sum(int((ref["lag"][b, :Fb] == -1).sum()) for b, Fb in enumerate(ref["frames"]))
        assert (ref["lag"] >= 0).sum() >= 10 and unvoiced > 0, name   # voiced and unvoiced frames inside rows


@pytest.mark.parametrize("name", PSOLA_NAMES)
def test_psola_cases_reach_their_paths(name):
    case = C.PSOLA_BY_NAME[name]
    cfg = case.cfg
    wav, lengths, lag, ratio = C.psola_input(case)
    ref = C.psola_reference(case)   # the reference's own K / J assertions run in here
    P = max(cfg["lag_max"], cfg["unvoiced_period"])
    p_min = min(cfg["lag_min"], cfg["unvoiced_period"])
    for b, n in enumerate(case.lengths):
        assert ref["n_marks"][b] <= R.max_marks(n, p_min) and ref["n_grains"][b] <= R.max_grains(n, p_min)
        assert np.isnan(wav[b, n:]).all() and not np.isnan(wav[b, :n]).any()
    if case.kind != "ratios":
        assert [int(s) for s in ref["status"]] == [R.OK if n else R.EMPTY for n in case.lengths]
    windows = [(b, lo, hi) for b in range(len(case.lengths)) for lo, hi in C.search_windows(case, b)]
    assert windows
    if "wide" in case.claims:
        assert any(hi - lo + 1 > 64 for _, lo, hi in windows)
    if "chunks" in case.claims:
        assert max(case.lengths) > C.PS_STAGE + P
    if "ties" in case.claims:
        assert np.abs(wav[0, :case.lengths[0]]).max() == C.CLIP and (wav[1, :case.lengths[1]] == np.float32(0.1)).all()
        spread = [C.lanes_holding_maximum(wav[b], lo, hi) for b, lo, hi in windows]
        assert any(run >= 2 and len(lanes) >= 2 for run, lanes in spread)
        assert any(run >= 2 and len(lanes) >= 2 for (run, lanes), (b, _, _) in zip(spread, windows) if b != 1)   # in a clipped row too
    if "lag_kinds" in case.claims:
        for b in (0, 1):
            kinds = C.lag_kinds(case)[b]
            voiced = lag[b, :len(kinds)] >= 1
            beside = [{bool(voiced[g]) for f in np.flatnonzero(kinds == k) for g in (f - 1, f + 1) if 0 <= g < len(kinds)} for k in range(5)]
            assert b or all(s == {True, False} for s in beside), beside   # the row of 36 frames: every kind beside both
            assert (lag[b, :len(kinds)][kinds == 3] == 5000).all() and (lag[b, :len(kinds)][kinds == 1] == -5).all()
        periods = {abs(p) for row in ref["periods"] for p in row}
        assert {cfg["lag_min"], cfg["lag_max"], cfg["unvoiced_period"]} <= periods    # lag 1 clamps up, 5000 down, 0 and -5 are unvoiced
    if case.kind == "ratios":
        assert [int(s) for s in ref["status"]] == [R.BAD_RATIO] * 4 + [R.OK]
        assert [float(q) for q in C.BAD_RATIOS[:2]] == [0.5 - 2.0 ** -25, 2.0 + 2.0 ** -22]
        assert set(ratio[4, :R.frames_of(case.lengths[4], cfg["hop"])].tolist()) == {0.5, 2.0} and ref["n_grains"][4] > 0
    if name == "p_min1":
        lib = _lib.load()
        N = max(case.lengths)
        assert lib.gvx_psola_max_marks(N, 1) == lib.gvx_psola_max_grains(N, 1) == N + 1
        assert min(abs(p) for row in ref["periods"] for p in row) == 1
    if name == "hop1":
        assert R.frames_of(max(case.lengths), 1) > C.PS_STAGE
    if case.first_centre:
        assert abs(case.first_centre) > 3 * cfg["hop"]


def test_psola_reference_float32_stays_inside_the_bound():
    """The bound the device is held to covers the restatement's own float32 run of every case."""
    worst = 0.0
    for case in C.PSOLA_CASES:
        if case.name in ("default_fc-3000", "default_fc3000"):
            continue
        wav, lengths, lag, ratio = C.psola_input(case)
        r64 = C.psola_reference(case)
        r32 = R.psola(wav, lengths, lag, ratio, first_centre=case.first_centre, dtype=np.float32, **case.cfg)
        for b, n in enumerate(case.lengths):
            bound = R.y_bound(r64["rows"][b], wav[b], n)
            err = np.abs(r32["y"][b].astype(np.float64) - r64["y"][b])
            assert (err <= bound).all(), (case.name, b)
            if n:
                worst = max(worst, float((err[:n] / np.maximum(bound[:n], 1e-300)).max()))
    print(f"float32 restatement: largest error / bound = {worst:.3f}")
