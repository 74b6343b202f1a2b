"""CPU: the restatement of the pitch tracker and of the contour comparison (tests/pitch_ref64.py) on cases with known answers, the
host function that groups a contour by token, the frame count and the argument checks that need no device."""
import math

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from genvox_amd.synthesizer import token_pitch
from tests import pitch_ref64 as R

DEFAULTS = dict(sampling_rate=22050, hop=256, window=1024, lag_min=44, lag_max=368, threshold=0.15)


def _inside(n, first_centre=0, **p):
    """Frames whose W + lag_max samples lie inside a row of n samples."""
    half = (p["window"] + p["lag_max"]) // 2
    return [f for f in range(R.frames_of(n, p["hop"]))
            if first_centre + f * p["hop"] - half >= 0 and first_centre + f * p["hop"] - half + p["window"] + p["lag_max"] <= n]


def test_sine_of_an_integer_period_gives_that_lag():
    period, n = 100, 8192
    x = (0.5 * np.sin(2 * np.pi * np.arange(n) / period))[None]
    for dtype in (np.float64, np.float32):
        got = R.yin(x.astype(np.float32), None, dtype=dtype, **DEFAULTS)
        inside = _inside(n, **DEFAULTS)
        assert len(inside) >= 20
        assert (got["lag"][0, inside] == period).all()
        assert np.abs(got["f0"][0, inside] - 22050 / period).max() < 0.05   # the normalisation by tau / sum tilts the parabola a little
        assert (got["aperiodicity"][0, inside] < 1e-4).all()
    assert got["frames"].tolist() == [32] and got["f0"].shape == (1, 32)


def test_silence_and_noise_are_unvoiced():
    n = 4096
    silent = R.yin(np.zeros((1, n), np.float32), None, **DEFAULTS)
    assert (silent["lag"] == -1).all() and (silent["f0"] == 0).all()
    assert (silent["cmnd"] == 1).all() and (silent["aperiodicity"] == 1).all() and (silent["d"] == 0).all()
    noise = np.random.default_rng(5).standard_normal((1, 8192)).astype(np.float32)
    got = R.yin(noise, None, **DEFAULTS)
    inside = _inside(8192, **DEFAULTS)
    assert (got["lag"][0, inside] == -1).all() and (got["f0"][0, inside] == 0).all()
    assert got["aperiodicity"][0, inside].min() > 0.5
    assert np.array_equal(got["aperiodicity"][0], got["cmnd"][0, :, 44:368].min(axis=1))


def test_hand_sized_case():
    """W = 4, lags 1 .. 4, a period of 3 samples, frame 0 at s = first_centre - (4 + 4) / 2 = 0:
        x        = 1 0 -1 1 0 -1 1 0 -1 1 0 -1
        d(1)     = (1-0)^2 + (0+1)^2 + (-1-1)^2 + (1-0)^2 = 7        d(2) = (1+1)^2 + (0-1)^2 + (-1-0)^2 + (1+1)^2 = 10
        d(3)     = 0                                                 d(4) = d(1) = 7
        c        = 1, 7/7, 10*2/17, 0, 7*4/24
        scan     tau = 1: 1 >= 0.5; tau = 2: 20/17 >= 0.5; tau = 3: 0 < 0.5 -> lag 3; tau + 1 = 4 > lag_max - 1: no walk
        den      = 20/17 - 0 + 7/6 = 239/102      shift = (20/17 - 7/6) / (2 * 239/102) = (1/102) / (478/102) = 1/478
        f0       = 300 / (3 + 1/478)
    Frame 1 (s = 4) sees the same period one sample on: x = 0 -1 1 0 | -1 1 0 -1, d(1) = 1 + 4 + 1 + 1 = 7, d(2) = 1 + 1 + 4 + 1 = 7, d(3) = 0.  Frame 2
    (s = 8) runs off the row: x = -1 1 0 -1 and then zeros."""
    x = np.array([[1, 0, -1] * 4], np.float32)
    p = dict(sampling_rate=300, hop=4, window=4, lag_min=1, lag_max=4, threshold=0.5, first_centre=4)
    got = R.yin(x, None, **p)
    assert got["frames"].tolist() == [3]
    assert got["d"][0, 0].tolist() == [0, 7, 10, 0, 7]
    assert np.allclose(got["cmnd"][0, 0], [1, 1, 20 / 17, 0, 7 / 6], rtol=1e-15)
    assert got["lag"][0].tolist()[:2] == [3, 3]
    assert math.isclose(got["shift"][0, 0], 1 / 478, rel_tol=1e-12) and math.isclose(got["den"][0, 0], 239 / 102, rel_tol=1e-12)
    assert math.isclose(got["f0"][0, 0], 300 / (3 + 1 / 478), rel_tol=1e-12)
    assert got["d"][0, 1].tolist() == [0, 7, 7, 0, 7] and got["aperiodicity"][0, 0] == 0
    # frame 2: the row's last four samples and zeros behind them
    w = np.array([-1, 1, 0, -1, 0, 0, 0, 0], np.float64)
    assert got["d"][0, 2].tolist() == [float(((w[:4] - w[t:t + 4]) ** 2).sum()) for t in range(5)]
    # what lies behind the row's length is not read: NaN there changes nothing
    y = np.concatenate([x, np.full((1, 5), np.nan, np.float32)], axis=1)
    again = R.yin(y, [12], **p)
    assert np.array_equal(again["cmnd"][0, :3], got["cmnd"][0]) and again["frames"].tolist() == [3] and again["lag"][0, 3] == -1
    # the margin: frame 0's scan compared c(1) = 1, c(2) = 20/17 and c(3) = 0 (infinitely far, relatively) with 0.5, and did not walk
    assert math.isclose(got["margin"][0, 0], min(abs(1 - 0.5) / 1, abs(20 / 17 - 0.5) / (20 / 17)), rel_tol=1e-12)


def test_walk_and_margin():
    c = np.array([1, 1, 0.4, 0.3, 0.2, 0.25, 0.1, 1.0])
    assert R.decide(c, 1, 7, 0.5)[0] == 4              # first under the threshold at 2, down to the local minimum at 4, not on to 6
    assert R.decide(c, 1, 7, 0.15)[0] == 6 and R.decide(c, 1, 6, 0.15)[0] == -1 and R.decide(c, 5, 7, 0.5)[0] == 6
    assert R.decide(c, 1, 4, 0.5)[0] == 3              # the walk stops at lag_max - 1
    lag, margin = R.decide(c, 1, 7, 0.4000001)
    assert lag == 4 and margin < 1e-6                   # c(2) = 0.4 against a threshold a hair above: marginal
    assert R.table_bound(1024, 368) == 2424 * 2.0 ** -24 and abs(R.table_bound(1024, 368) - 1.45e-4) < 1e-6


def test_f0_compare_by_hand():
    fa = np.array([[100, 100, 0, 0, 200, 150, 0],
                   [0, 0, 0, 0, 0, 0, 0],
                   [100, 200, 300, 0, 0, 0, 0],
                   [100, 0, 100, 0, 7, 7, 7],
                   [100, 110, 0, 0, 0, 0, 0]], np.float32)
    fb = np.array([[100, 121, 0, 50, 100, 0, 9],
                   [0, 0, 0, 0, 0, 0, 0],
                   [200, 100, 100, 0, 0, 0, 0],
                   [0, 100, 0, 100, 7, 7, 7],
                   [100, 100, 0, 0, 0, 0, 0]], np.float32)
    counts, vde, gpe, rmse = R.f0_compare(fa, fb, [6, 7, 3, 4, 0], [7, 7, 7, 7, 7])
    # row 0 over 6 frames: both voiced at 0, 1, 4; one voiced at 3, 5; gross at 4 (ratio 2) - 100/121 = 0.826 is inside 20 %
    assert counts[0].tolist() == [6, 3, 2, 1] and vde[0] == 2 / 6 and gpe[0] == 1 / 3
    assert math.isclose(rmse[0], math.sqrt((0 + (1200 * math.log2(100 / 121)) ** 2) / 2), rel_tol=1e-12)
    # row 1: frames but nothing voiced: vde 0, gpe and rmse NaN
    assert counts[1].tolist() == [7, 0, 0, 0] and vde[1] == 0 and math.isnan(gpe[1]) and math.isnan(rmse[1])
    # row 2: only gross errors: gpe 1, rmse NaN
    assert counts[2].tolist() == [3, 3, 0, 3] and vde[2] == 0 and gpe[2] == 1 and math.isnan(rmse[2])
    # row 3 over 4 frames: voiced in exactly one everywhere
    assert counts[3].tolist() == [4, 0, 4, 0] and vde[3] == 1 and math.isnan(gpe[3]) and math.isnan(rmse[3])
    # row 4: no frames: every ratio NaN
    assert counts[4].tolist() == [0, 0, 0, 0] and math.isnan(vde[4]) and math.isnan(gpe[4]) and math.isnan(rmse[4])
    # the edge of "gross": 1.2 in float32 is a hair above 1.2 -> gross; 0.8 in float32 is a hair above 0.8 -> not
    edge = R.f0_compare(np.array([[1.2, 0.8]], np.float32), np.array([[1.0, 1.0]], np.float32))
    assert edge[0][0].tolist() == [2, 2, 0, 1]
    c32 = R.f0_compare(fa, fb, [6, 7, 3, 4, 0], [7, 7, 7, 7, 7], dtype=np.float32)
    assert np.array_equal(c32[0], counts) and c32[3].dtype == np.float32 and abs(c32[3][0] - rmse[0]) < 1e-3


def test_token_pitch():
    f0 = [0, 100, 110, 0, 0, 200, 0, 300]
    got = token_pitch([0, 3, 5, 6], 8, f0)
    assert got == [(105.0, 2 / 3), (None, 0.0), (200.0, 1.0), (300.0, 0.5)]   # boundaries, an all-unvoiced token, a token of one frame
    assert token_pitch([0, 3, 5, 6], 7, f0)[-1] == (None, 0.0)                 # the last token ends at n_frames, not at the contour's end
    assert token_pitch([0, 3, 3, 6], 8, f0)[1] == (None, 0.0)                  # a token without frames
    assert token_pitch([0, 3, 5, 6], 20, f0)[-1] == (300.0, 0.5)               # n_frames beyond the contour: the contour's end
    assert token_pitch([], 8, f0) == [] and token_pitch([0], 0, []) == [(None, 0.0)]
    assert token_pitch([0, 4], 8, np.asarray(f0, np.float32)) == [(105.0, 0.5), (250.0, 0.5)]
    with pytest.raises(ValueError):
        token_pitch([0], 8, [[1.0]])
    with pytest.raises(ValueError):
        token_pitch([0], -1, f0)


def test_pitch_frames_and_tile():
    lib = _lib.load()
    assert [lib.gvx_pitch_frames(n, 256) for n in (0, 1, 255, 256, 257, 204800, -5)] == [0, 1, 1, 1, 2, 800, 0]
    assert lib.gvx_pitch_frames(10, 0) == 0 and metrics.pitch_frames(2840, 256) == 12
    assert [R.frames_of(n, 256) for n in (0, 1, 255, 256, 257, 204800, -5)] == [0, 1, 1, 1, 2, 800, 0]
    tile = lambda **k: lib.gvx_pitch_tile_frames(metrics.pitch_params(22050, **k))
    assert tile(hop_length=256) == 16 and tile(hop_length=4096) == 4 and tile(hop_length=100000) == 1
    p = _lib.gvx_pitch_params(22050, 16, 2048, 1, 1024, 0.15, 0)
    assert lib.gvx_pitch_tile_frames(p) == 16
    p.hop = 2048                          # 16384 floats of LDS: 4 * 1025 of tables, 3072 of one frame, 9212 / 2048 = 4 more frames
    assert lib.gvx_pitch_tile_frames(p) == 5
    p.window = 2049
    assert lib.gvx_pitch_tile_frames(p) == -1 and lib.gvx_pitch_tile_frames(None) == -1


def test_argument_checks_without_a_device():
    p = metrics.pitch_params(22050, 256)
    assert (p.sampling_rate, p.hop, p.window, p.lag_min, p.lag_max, p.first_centre) == (22050, 256, 1024, 44, 368, 0)
    assert abs(p.threshold - 0.15) < 1e-7
    assert metrics.pitch_params(16000, 200, fmin=50, fmax=400, first_centre=-500).lag_max == 320
    for bad in (dict(hop_length=0), dict(sampling_rate=0), dict(fmin=500.0, fmax=60.0), dict(fmin=0.0), dict(fmin=float("nan")),
                dict(fmin=10.0), dict(fmax=30000.0), dict(window=31), dict(window=2049), dict(threshold=0.0), dict(threshold=1.5),
                dict(threshold=float("nan")), dict(hop_length=2.5), dict(first_centre=2 ** 31), dict(window=True)):
        kw = dict(sampling_rate=22050, hop_length=256)
        kw.update(bad)
        with pytest.raises(ValueError):
            metrics.pitch_params(**kw)
        with pytest.raises(ValueError):
            metrics.pitch_track(torch.zeros(1, 4096), **kw)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        metrics.pitch_track(torch.zeros(1, 4096), sampling_rate=22050, hop_length=256)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        metrics.f0_compare(torch.zeros(1, 8), torch.zeros(1, 8))
    with pytest.raises(TypeError):
        metrics.pitch_track(torch.zeros(1, 4096))   # the rate and the hop have no defaults
    # the C ABI's own checks run before anything is launched: made-up addresses are never touched
    lib, P = _lib.load(), 1 << 20
    ok = lambda **k: _lib.gvx_pitch_params(**{**dict(sampling_rate=22050, hop=256, window=1024, lag_min=44, lag_max=368, threshold=0.15, first_centre=0), **k})
    call = lambda p, B=1, N=4096, wav=P, f0=P, lag=P, ap=P: lib.gvx_pitch_yin(wav, None, B, N, p, f0, lag, ap, None, None)
    for p in (ok(hop=0), ok(window=0), ok(lag_min=0), ok(lag_min=368), ok(lag_min=400), ok(threshold=0.0), ok(threshold=1.0001),
              ok(threshold=float("nan")), ok(sampling_rate=0)):
        assert call(p) == -1
    assert call(ok(), B=0) == -1 and call(ok(), N=0) == -1 and call(None) == -1
    assert call(ok(), wav=None) == -1 and call(ok(), f0=None) == -1 and call(ok(), lag=None) == -1 and call(ok(), ap=None) == -1
    for p in (ok(window=31), ok(window=2049), ok(lag_max=1025)):
        assert call(p) == -2 and b"limits" in lib.gvx_last_error()
    assert call(ok(), B=65536) == -2 and call(ok(hop=1), N=32769) == -2 and b"frames" in lib.gvx_last_error()
    cmp = lambda B=1, F=8, a=P, b=P, c=P, v=P, g=P, r=P: lib.gvx_f0_compare(a, b, None, None, B, F, c, v, g, r, None)
    assert cmp(B=0) == -1 and cmp(F=0) == -1 and cmp(a=None) == -1 and cmp(b=None) == -1 and cmp(c=None) == -1 and cmp(v=None) == -1
    assert cmp(g=None) == -1 and cmp(r=None) == -1 and cmp(F=32769) == -2
