"""GPU: gvx_psola_plan and gvx_psola_synth against the numpy restatement of tests/psola_ref.py.  Everything integral - marks, periods,
synthesis positions and sources, counts, statuses - is compared exactly; every output sample is held to the rounding bound derived
in psola_ref.y_bound, evaluated on the float64 restatement (no measured multiple).  The lag contours are made up, not tracked: the
plan is defined for any table, and a made-up one switches between voiced and unvoiced and between far-apart lags more often than a
voice does."""
import functools

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from tests import psola_ref as R
from tests.psola_ref import tiled_period

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(hop=16, lag_min=4, lag_max=40, unvoiced_period=20)   # sampling_rate 2000: fmax 500, fmin 50, U = 2000 // 100
TILE = 256
SENTINEL = -777


def made_up_lags(rng, frames: int, lag_min: int, lag_max: int) -> np.ndarray:
    """Runs of 1 .. 6 frames, voiced at a lag that wanders or jumps, or unvoiced."""
    out, f = np.empty(frames, np.int32), 0
    lag = int(rng.integers(lag_min, lag_max + 1))
    while f < frames:
        run = int(rng.integers(1, 7))
        kind = rng.random()
        if kind < 0.3:
            out[f:f + run] = -1
        else:
            lag = int(rng.integers(lag_min, lag_max + 1)) if kind < 0.5 else int(np.clip(lag + rng.integers(-3, 4), lag_min, lag_max))
            out[f:f + run] = lag
        f += run
    return out


def make_batch(lengths, N, seed, first_centre, cfg=SMALL):
    """Rows at their own lengths with poison at and behind them in every input: NaN in wav and ratio, a huge lag.  Row i takes the
    ratio kind i mod 4: all 0.5, all 1, all 2, a ramp from 0.5 to 2 with noise."""
    rng = np.random.default_rng(seed)
    B, F = len(lengths), R.frames_of(N, cfg["hop"])
    wav = np.full((B, N), np.nan, np.float32)
    lag = np.full((B, F), 2 ** 30, np.int32)
    ratio = np.full((B, F), np.nan, np.float32)
    for b, n in enumerate(lengths):
        Fb = R.frames_of(n, cfg["hop"])
        period = int(rng.integers(cfg["lag_min"] + 2, cfg["lag_max"]))
        wav[b, :n] = tiled_period(period, n) + 0.05 * rng.standard_normal(n).astype(np.float32)
        lag[b, :Fb] = made_up_lags(rng, Fb, cfg["lag_min"], cfg["lag_max"])
        kind = b % 4
        ratio[b, :Fb] = (0.5, 1.0, 2.0)[kind] if kind < 3 else np.clip(np.linspace(0.5, 2.0, Fb) + 0.1 * rng.standard_normal(Fb), 0.5, 2.0)
    return wav, np.asarray(lengths, np.int32), lag, ratio


def params_of(first_centre, cfg=SMALL):
    return _lib.gvx_psola_params(cfg["hop"], first_centre, cfg["lag_min"], cfg["lag_max"], cfg["unvoiced_period"])


def run_device(wav, lengths, lag, ratio, params):
    """Both calls through the C ABI on sentinel-filled outputs.  Returns host arrays and the two return codes."""
    lib = _lib.load()
    B, N = wav.shape
    p_min = min(params.lag_min, params.unvoiced_period)
    K, J = lib.gvx_psola_max_marks(N, p_min), lib.gvx_psola_max_grains(N, p_min)
    t = lambda a: torch.from_numpy(a).to(DEV)
    x, n, lg, rt = t(wav), t(lengths), t(lag), t(ratio)
    ints = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)
    out = {"marks": ints(B, K), "periods": ints(B, K), "syn_pos": ints(B, J), "syn_src": ints(B, J), "counts": ints(B, 2), "status": ints(B),
           "y": torch.full((B, N), float(SENTINEL), dtype=torch.float32, device=DEV)}
    stream = torch.cuda.current_stream().cuda_stream
    rc_plan = lib.gvx_psola_plan(x.data_ptr(), n.data_ptr(), lg.data_ptr(), rt.data_ptr(), B, N, params, out["marks"].data_ptr(),
                                 out["periods"].data_ptr(), out["syn_pos"].data_ptr(), out["syn_src"].data_ptr(), out["counts"].data_ptr(),
                                 out["status"].data_ptr(), stream)
    rc_synth = lib.gvx_psola_synth(x.data_ptr(), n.data_ptr(), out["marks"].data_ptr(), out["periods"].data_ptr(), out["syn_pos"].data_ptr(),
                                   out["syn_src"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr(), B, N, params, out["y"].data_ptr(),
                                   stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, rc_plan, rc_synth


def compare(got, ref, wav, lengths, label):
    """Integers exactly, sentinels untouched, zeros behind the rows, every sample inside the derived bound.  Returns the largest
    error over its bound."""
    B, N = wav.shape
    assert np.array_equal(got["status"], ref["status"]), label
    assert np.array_equal(got["counts"][:, 0], ref["n_marks"]) and np.array_equal(got["counts"][:, 1], ref["n_grains"]), label
    worst = 0.0
    for b in range(B):
        n, K, J = int(lengths[b]), int(ref["n_marks"][b]), int(ref["n_grains"][b])
        assert got["marks"][b, :K].tolist() == ref["marks"][b] and got["periods"][b, :K].tolist() == ref["periods"][b], (label, b)
        assert got["syn_pos"][b, :J].tolist() == ref["syn_pos"][b] and got["syn_src"][b, :J].tolist() == ref["syn_src"][b], (label, b)
        for key, count in (("marks", K), ("periods", K), ("syn_pos", J), ("syn_src", J)):
            assert (got[key][b, count:] == SENTINEL).all(), (label, b, key)
        assert (got["y"][b, n:] == 0).all(), (label, b)
        bound = R.y_bound(ref["rows"][b], wav[b], n)
        err = np.abs(got["y"][b].astype(np.float64) - ref["y"][b])
        assert np.isfinite(got["y"][b]).all() and (err <= bound).all(), (label, b, float((err - bound).max()))
        if n:
            worst = max(worst, float((err[:n] / np.maximum(bound[:n], 1e-300)).max()))
    return worst


LENGTHS = [0, 1, 3, 40, 41, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 300, 200, 333]
NAN_ROW, UNVOICED_ROW = 10, 11


@functools.lru_cache(maxsize=None)
def small_case(first_centre):
    wav, lengths, lag, ratio = make_batch(LENGTHS, 2 * TILE + 1, 40 + first_centre, first_centre)
    ratio[NAN_ROW, 5] = np.nan
    lag[UNVOICED_ROW, :R.frames_of(LENGTHS[UNVOICED_ROW], 16)] = -1
    ref = R.psola(wav, lengths, lag, ratio, first_centre=first_centre, **SMALL)
    return wav, lengths, lag, ratio, ref


@pytest.mark.parametrize("first_centre", [0, -7, 5])
def test_rows_at_every_edge(first_centre):
    wav, lengths, lag, ratio, ref = small_case(first_centre)
    assert ref["status"].tolist() == [R.EMPTY] + [R.OK] * 9 + [R.BAD_RATIO, R.OK]
    assert sum(len(set(np.sign(p))) == 2 for p in ref["periods"][5:10]) >= 4   # these rows switch between voiced and unvoiced
    got, rc_plan, rc_synth = run_device(wav, lengths, lag, ratio, params_of(first_centre))
    assert rc_plan == 0 and rc_synth == 0
    worst = compare(got, ref, wav, lengths, first_centre)
    print(f"first_centre {first_centre}: largest error / bound = {worst:.3f}")
    assert np.array_equal(got["y"][NAN_ROW, :200], wav[NAN_ROW, :200])                  # a bad ratio: the row goes through unchanged
    assert np.abs(ref["y"][UNVOICED_ROW] - np.nan_to_num(wav[UNVOICED_ROW].astype(np.float64))).max() < 1e-15   # unvoiced: grains at U tile the row
    again, _, _ = run_device(wav, lengths, lag, ratio, params_of(first_centre))
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_rows_longer_than_a_staged_chunk():
    """9001 samples: the plan's wave moves its 4096 staged samples twice; the row at lag 4 and ratio 2 has more marks than the second
    walk holds at a time (2050), and the grains of a tile reach the synthesis' capacity order."""
    N = 9001
    wav, lengths, lag, ratio = make_batch([N, N - 700, N], N, 9, 0)
    lag[2], ratio[2] = 4, 2.0
    wav[2] = 0.3 * np.sin(np.arange(N) * 0.9).astype(np.float32)
    ref = R.psola(wav, lengths, lag, ratio, **SMALL)
    assert ref["n_marks"][2] > 2100 and ref["n_grains"][2] > 4200 and (ref["status"] == R.OK).all()
    got, rc_plan, rc_synth = run_device(wav, lengths, lag, ratio, params_of(0))
    assert rc_plan == 0 and rc_synth == 0
    print(f"long rows: largest error / bound = {compare(got, ref, wav, lengths, 'long'):.3f}")


def test_refused_calls_write_nothing():
    wav, lengths, lag, ratio = make_batch([100, 64], 100, 1, 0)
    for bad in (dict(hop=0), dict(lag_min=0), dict(unvoiced_period=0), dict(lag_max=3), dict(lag_max=1025), dict(unvoiced_period=2000)):
        cfg = {**SMALL, **bad}
        p = _lib.gvx_psola_params(cfg["hop"], 0, cfg["lag_min"], cfg["lag_max"], cfg["unvoiced_period"])
        lib = _lib.load()
        t = lambda a: torch.from_numpy(a).to(DEV)
        x, n, lg, rt = t(wav), t(lengths), t(lag), t(ratio)
        outs = [torch.full((2, 128), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(6)]
        y = torch.full((2, 100), float(SENTINEL), device=DEV)
        rc = lib.gvx_psola_plan(x.data_ptr(), n.data_ptr(), lg.data_ptr(), rt.data_ptr(), 2, 100, p, *[o.data_ptr() for o in outs], None)
        rc2 = lib.gvx_psola_synth(x.data_ptr(), n.data_ptr(), *[o.data_ptr() for o in outs], 2, 100, p, y.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc in (-1, -2) and rc2 == rc, bad
        assert all((o == SENTINEL).all().item() for o in outs) and (y == SENTINEL).all().item(), bad


def test_python_calls_are_the_c_calls():
    wav, lengths, lag, ratio, ref = small_case(-7)
    t = lambda a: torch.from_numpy(a).to(DEV)
    kw = dict(sampling_rate=2000, hop_length=16, first_centre=-7, fmin=50.0, fmax=500.0)
    got, _, _ = run_device(wav, lengths, lag, ratio, params_of(-7))
    plan = metrics.psola_plan(t(wav), t(lengths), t(lag), t(ratio), **kw)
    out = metrics.pitch_shift(t(wav), t(lengths), t(lag), t(ratio), **kw)
    assert set(out) == {"wav", "status", "n_marks", "n_grains"}
    assert out["wav"].cpu().numpy().tobytes() == got["y"].tobytes()
    assert np.array_equal(out["status"].cpu().numpy(), ref["status"]) and np.array_equal(out["n_marks"].cpu().numpy(), ref["n_marks"])
    assert np.array_equal(out["n_grains"].cpu().numpy(), ref["n_grains"]) and np.array_equal(plan["n_grains"].cpu().numpy(), ref["n_grains"])
    for b, K in enumerate(ref["n_marks"]):
        assert plan["marks"][b, :K].tolist() == ref["marks"][b]
    assert [metrics.PSOLA_STATUS_NAMES[s] for s in out["status"].tolist()[:2] + [out["status"].tolist()[NAN_ROW]]] == ["empty", "ok", "bad_ratio"]
    with pytest.raises(ValueError):
        metrics.pitch_shift(t(wav), t(lengths), t(lag)[:, :-1], t(ratio), **kw)


def test_track_shift_track_at_the_default_configuration():
    """22050 Hz, hop 256, lags 44 .. 368: a tiled period of 100 samples, 20 frames, tracked, raised by 1.25, tracked again: the lag of
    every interior frame is round(100 / 1.25) = 80."""
    P, rho, n = 100, 1.25, 20 * 256
    x = torch.from_numpy(tiled_period(P, n))[None].to(DEV)
    grid = dict(sampling_rate=22050, hop_length=256)
    before = metrics.pitch_track(x, **grid)
    interior = [f for f in range(20) if f * 256 - 696 >= 400 and f * 256 + 696 <= n - 400]
    assert (before["lag"][0, interior] == P).all()
    shifted = metrics.pitch_shift(x, None, before["lag"], torch.full((1, 20), rho, device=DEV), **grid)
    assert shifted["status"].tolist() == [0] and shifted["n_grains"].item() > shifted["n_marks"].item() > 40
    after = metrics.pitch_track(shifted["wav"], **grid)
    assert (after["lag"][0, interior] == 80).all(), after["lag"][0].tolist()
    y = shifted["wav"][0].cpu().numpy()
    assert np.abs(y[800:n - 880] - y[880:n - 800]).max() < 1e-5 and np.abs(y).max() > 0.3
