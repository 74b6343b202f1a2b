"""CPU: the restatement of the pitch control (tests/psola_ref.py) on cases with known answers, the host helpers of the synthesizer,
the capacities and the argument checks that need no device."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from genvox_amd.synthesizer import Synthesizer, frame_ratios, semitones_to_ratio, token_semitones
from tests import pitch_ref64 as Y
from tests import psola_ref as R
from tests.psola_ref import tiled_period

SMALL = dict(hop=16, lag_min=4, lag_max=40, unvoiced_period=20)
DEFAULTS = dict(sampling_rate=22050, hop=256, window=1024, lag_min=44, lag_max=368, threshold=0.15)


def test_pulse_train_by_hand():
    """Unit pulses every 20 samples, every frame voiced at lag 20.  The marks are the pulses (the window 20 k +- 5 holds one sample
    that is not 0).  A grain is two periods of the input around a pulse: a single 1 at its centre, so the output has a pulse at every
    synthesis mark and nothing else between the first and the last.  Ratio 1.25: step = floor(20 / 1.25 + 0.5) = 16; the grains
    overlap, D at a mark is 1 + 2 S(1 - 16/20) = 1 + 2 * 0.04 * 2.6 = 1.208.  Ratio 0.5: step 40, the grains just touch: D = 1 at a
    mark.  Ratio 1: the input."""
    n = 400
    x = np.zeros((1, n), np.float32)
    x[0, ::20] = 1
    lag = np.full((1, R.frames_of(n, 16)), 20, np.int32)
    for ratio, step, height in ((1.0, 20, 1.0), (1.25, 16, 1 / 1.208), (0.5, 40, 1.0)):
        got = R.psola(x, None, lag, np.full(lag.shape, ratio, np.float32), **SMALL)
        assert got["marks"][0] == list(range(0, n, 20)) and got["periods"][0] == [20] * 20 and got["status"][0] == R.OK
        assert got["syn_pos"][0] == list(range(0, n, step))
        assert got["syn_src"][0] == [min(range(20), key=lambda k: (abs(20 * k - s), k)) for s in got["syn_pos"][0]]
        last = got["syn_pos"][0][-1]
        y = got["y"][0, :last + 1]
        assert np.flatnonzero(y).tolist() == got["syn_pos"][0]
        assert np.allclose(y[::step][1:-1], height, rtol=1e-12)                    # the first and the last mark have one neighbour only:
        assert np.allclose(y[[0, last]], 1.0 if step >= 20 else 1 / 1.104, rtol=1e-12)    # D = 1 + S(0.2) there
    same = R.psola(x, None, lag, np.ones(lag.shape, np.float32), **SMALL)
    assert np.array_equal(same["y"], x.astype(np.float64))   # ratio 1 at a constant period: the grains sum to one, the input comes back


def test_tiled_period_shifts_to_the_rounded_period():
    """P = 100 at rho = 1.25: the marks lock to the period's peak, every grain is the same two periods, the synthesis marks are 80
    apart - the interior of the output is exactly periodic with round(P / rho) = 80, and the tracker's restatement finds that lag."""
    P, rho, n = 100, 1.25, 20 * 256
    x = tiled_period(P, n)[None]
    before = Y.yin(x, None, **DEFAULTS)
    frames = R.frames_of(n, 256)
    interior = [f for f in range(frames) if f * 256 - 696 >= 400 and f * 256 + 696 <= n - 400]
    assert len(interior) >= 10 and (before["lag"][0, interior] == P).all() and (before["lag"][0] >= 1).all()
    got = R.psola(x, None, before["lag"], np.full((1, frames), rho, np.float32), hop=256, lag_min=44, lag_max=368, unvoiced_period=220)
    marks, pos = np.array(got["marks"][0]), np.array(got["syn_pos"][0])
    inner_marks = marks[(marks >= 400) & (marks < n - 400)]
    assert (inner_marks % P == 0).all() and (np.diff(inner_marks) == P).all()
    inner_pos = pos[(pos >= 400) & (pos < n - 400)]
    assert (np.diff(inner_pos) == 80).all()
    y = got["y"][0]
    assert np.abs(y[800:n - 880] - y[880:n - 800]).max() < 1e-12 and np.abs(y[800:n - 800]).max() > 0.3
    after = Y.yin(y[None], None, **DEFAULTS)
    assert (after["lag"][0, interior] == 80).all()


def test_unvoiced_rows_heads_and_tails():
    rng = np.random.default_rng(3)
    n = 333
    x = rng.standard_normal((1, n)).astype(np.float32)
    F = R.frames_of(n, 16)
    lag = np.full((1, F), -1, np.int32)
    got = R.psola(x, None, lag, np.full((1, F), 2.0, np.float32), **SMALL)   # a ratio never repitches unvoiced sound
    assert got["marks"][0] == list(range(0, n, 20)) and got["periods"][0] == [-20] * 17
    assert got["syn_pos"][0] == got["marks"][0] and got["syn_src"][0] == list(range(17))
    row = got["rows"][0]
    last = got["syn_pos"][0][-1]
    assert np.abs(row["D"][:last + 1] - 1).max() < 1e-15          # grains at the period U tile the row
    assert np.abs(got["y"][0] - x[0]).max() < 1e-15              # and behind the last mark the rest of the input is kept
    assert (row["grains"][:last + 1] <= 2).all() and (row["grains"][:last + 1] >= 1).all()
    # a voiced row whose first mark is not sample 0: the head before it and the tail behind the last mark are the input's
    v = tiled_period(20, 200)
    v = np.roll(v, 7)[None]
    lag = np.full((1, R.frames_of(200, 16)), 20, np.int32)
    got = R.psola(v, None, lag, np.full(lag.shape, 1.6, np.float32), **SMALL)
    first, last = got["syn_pos"][0][0], got["syn_pos"][0][-1]
    assert first == 5 and got["marks"][0][1] == 27            # the window of c = 0 is [0, 5]: the peak at 7 is out of reach; c = 25 finds 27
    row = got["rows"][0]
    assert not row["inside"][:first].any() and not row["inside"][last + 1:200].any() and row["inside"][first:last + 1].all()
    outside = list(range(first)) + list(range(last + 1, 200))
    for t in outside:
        D, Num = row["D"][t], row["Num"][t]
        assert row["y"][t] == (Num / D if D >= 1 else Num + (1 - D) * np.float64(v[0, t]))
    assert any(row["D"][t] < 1 for t in outside) and any(row["D"][t] >= 1 for t in outside)   # both forms occur
    # what lies behind a row's length is not read, and comes out 0
    padded = np.concatenate([v, np.full((1, 9), np.nan, np.float32)], axis=1)
    lag9 = np.concatenate([lag, np.full((1, R.frames_of(209, 16) - lag.shape[1]), 7, np.int32)], axis=1)
    again = R.psola(padded, [200], lag9, np.full(lag9.shape, 1.6, np.float32), **SMALL)
    assert again["marks"][0] == got["marks"][0] and np.array_equal(again["y"][0, :200], got["y"][0]) and (again["y"][0, 200:] == 0).all()


def test_statuses_and_capacities():
    x = tiled_period(20, 100)[None]
    F = R.frames_of(100, 16)
    lag = np.full((1, F), 20, np.int32)
    for bad in (np.nan, 0.49, 2.01, np.inf, -1.0):
        ratio = np.ones((1, F), np.float32)
        ratio[0, F - 1] = bad
        got = R.psola(x, None, lag, ratio, **SMALL)
        assert got["status"][0] == R.BAD_RATIO and got["n_grains"][0] == 0 and got["n_marks"][0] > 0
        assert np.array_equal(got["y"][0], x[0].astype(np.float64))
        # the same value behind the row's frames is not looked at
        short = R.psola(x, [100 - 16], lag, ratio, **SMALL)
        assert short["status"][0] == R.OK
    empty = R.psola(x, [0], lag, np.ones((1, F), np.float32), **SMALL)
    assert empty["status"][0] == R.EMPTY and empty["n_marks"][0] == 0 and (empty["y"] == 0).all()
    lib = _lib.load()
    for N, p in ((1, 1), (100, 4), (513, 4), (513, 20), (204800, 44), (204800, 220), (7, 1024), (2 ** 25, 1)):
        assert lib.gvx_psola_max_marks(N, p) == R.max_marks(N, p) == N // math.ceil(3 * p / 4) + 1
        assert lib.gvx_psola_max_grains(N, p) == R.max_grains(N, p) == N // max(1, (p + 1) // 2) + 1
    assert lib.gvx_psola_max_marks(204800, 44) == 6207 and lib.gvx_psola_max_grains(204800, 44) == 9310
    assert lib.gvx_psola_max_marks(0, 4) == 0 and lib.gvx_psola_max_marks(10, 0) == 0 and lib.gvx_psola_max_grains(-1, 4) == 0
    # the densest rows reach the capacities' order: every lag at lag_min, every ratio 2
    n = 512
    dense = R.psola(np.ones((1, n), np.float32), None, np.full((1, 32), 4, np.int32), np.full((1, 32), 2.0, np.float32), **SMALL)
    assert dense["n_marks"][0] <= R.max_marks(n, 4) and dense["n_grains"][0] <= R.max_grains(n, 4)
    assert dense["n_marks"][0] == 171 and dense["n_grains"][0] == 256    # marks every 3 (the lowest index of equal samples), grains every 2


def test_bound_is_the_float32_scale():
    """The derived bound holds for the restatement's own float32 run, and is not orders of magnitude above it."""
    rng = np.random.default_rng(11)
    n = 700
    x = (tiled_period(23, n) + 0.05 * rng.standard_normal(n).astype(np.float32))[None]
    F = R.frames_of(n, 16)
    lag = np.full((1, F), 23, np.int32)
    lag[0, 10:20] = -1
    ratio = np.linspace(0.5, 2.0, F).astype(np.float32)[None]
    r64 = R.psola(x, None, lag, ratio, **SMALL)
    r32 = R.psola(x, None, lag, ratio, dtype=np.float32, **SMALL)
    bound = R.y_bound(r64["rows"][0], x[0], n)
    err = np.abs(r32["y"][0].astype(np.float64) - r64["y"][0])
    assert (err <= bound).all() and err.max() > 0
    assert bound.max() < 1e-4 * np.abs(r64["y"][0]).max()


def test_host_helpers():
    assert semitones_to_ratio(12) == 2.0 and semitones_to_ratio(-12) == 0.5 and semitones_to_ratio(0) == 1.0
    assert math.isclose(semitones_to_ratio(7), 2 ** (7 / 12), rel_tol=1e-15)
    for bad in (float("nan"), float("inf"), "3", None, True):
        with pytest.raises(ValueError):
            semitones_to_ratio(bad)
    toks = list(" hi  there, you. ")
    words = [-1, 0, 0, -1, -1, 1, 1, 1, 1, 1, 1, -1, 2, 2, 2, 2, -1]
    assert token_semitones(toks, None) == [0.0] * len(toks)
    assert token_semitones(toks, [1, -2.5, 0]) == [0.0 if w < 0 else (1.0, -2.5, 0.0)[w] for w in words]
    assert token_semitones(toks, {1: 4}) == [4.0 if w == 1 else 0.0 for w in words]
    assert token_semitones([], None) == [] and token_semitones(list("  "), []) == [0.0, 0.0]
    for bad in ([1, 2], [1, 2, 3, 4], {3: 1.0}, {-1: 1.0}, {1.0: 1.0}, {True: 1.0}, {0: float("nan")}, [1, float("inf"), 0], {0: "2"}, {0: True}):
        with pytest.raises(ValueError):
            token_semitones(toks, bad)
    got = frame_ratios([0, 3, 5], 8, [0.0, 12.0, -12.0], 0.0)
    assert got.dtype == np.float32 and got.tolist() == [1, 1, 1, 2, 2, 0.5, 0.5, 0.5]
    assert frame_ratios([2, 4], 6, [1.0, 0.0], 3.0).tolist() == [np.float32(2 ** (3 / 12))] * 2 + [np.float32(2 ** (4 / 12))] * 2 + [np.float32(2 ** (3 / 12))] * 2
    assert frame_ratios([0, 9], 4, [1.0, 5.0], 0.0).tolist() == [np.float32(2 ** (1 / 12))] * 4     # a start behind the frames: clamped
    assert frame_ratios([], 3, [], 2.0).tolist() == [np.float32(2 ** (2 / 12))] * 3 and frame_ratios([0], 0, [1.0]).shape == (0,)
    with pytest.raises(ValueError):
        frame_ratios([0, 1], 4, [0.0])
    with pytest.raises(ValueError):
        frame_ratios([0], -1, [0.0])
    # the checks of tts / tts_batch that run before anything touches the device
    assert Synthesizer._check_pitch_control(3, 1) == (3.0, 1.0) and Synthesizer._check_pitch_control(-12.0, 0.0) == (-12.0, 0.0)
    for shift, rng in ((12.5, 1.0), (float("nan"), 1.0), (0.0, -0.1), (0.0, float("inf")), ("1", 1.0), (0.0, None)):
        with pytest.raises(ValueError):
            Synthesizer._check_pitch_control(shift, rng)
    assert Synthesizer._sentence_semitones(toks, {0: 2.0}, 10.0, "s")[1] == 2.0
    with pytest.raises(ValueError, match="sentence 4"):
        Synthesizer._sentence_semitones(toks, {0: 2.5}, 10.0, "sentence 4")
    with pytest.raises(ValueError):
        Synthesizer._sentence_semitones(toks, {2: -3.0}, -9.5, "s")
    # pitch_range 0 brings every voiced frame to the row's mean log-F0 (here log2 200), 2 doubles its distance; unvoiced frames get 1.
    # The mean is kept in units of 2^-20 octave: off by at most 2^-21 octave, 3.3e-7 relative, on top of float32's own roundings
    f0 = torch.tensor([[100.0, 0.0, 200.0, 400.0], [0.0, 0.0, 0.0, 0.0]])
    assert np.allclose(Synthesizer._range_ratios(f0, 0.0).numpy(), [[2, 1, 1, 0.5], [1, 1, 1, 1]], rtol=1e-6, atol=0)
    assert np.allclose(Synthesizer._range_ratios(f0, 2.0).numpy(), [[0.5, 1, 1, 2], [1, 1, 1, 1]], rtol=1e-6, atol=0)
    assert (Synthesizer._range_ratios(f0, 1.0) == 1).all()
    alone, padded = Synthesizer._range_ratios(f0[:1], 0.3), Synthesizer._range_ratios(torch.nn.functional.pad(f0, (0, 5)), 0.3)
    assert alone.numpy().tobytes() == padded[:1, :4].contiguous().numpy().tobytes()   # a row's ratios do not depend on the batch it is in
    for fn in (Synthesizer.tts, Synthesizer.tts_batch):
        sig = inspect.signature(fn).parameters
        assert (sig["pitch_shift"].default, sig["word_pitch"].default, sig["pitch_range"].default) == (0.0, None, 1.0)
    assert metrics.PSOLA_STATUS_NAMES == ("ok", "empty", "bad_ratio")


def test_symbols_and_argument_checks_without_a_device():
    lib = _lib.load()
    for name in ("gvx_psola_max_marks", "gvx_psola_max_grains", "gvx_psola_plan", "gvx_psola_synth"):
        restype, argtypes = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert ctypes.sizeof(_lib.gvx_psola_params) == 20
    p = metrics.psola_params(22050, 256)
    assert (p.hop, p.first_centre, p.lag_min, p.lag_max, p.unvoiced_period) == (256, 0, 44, 368, 220)
    q = metrics.psola_params(2000, 16, first_centre=-7, unvoiced_period=20, fmin=50.0, fmax=500.0)
    assert (q.hop, q.first_centre, q.lag_min, q.lag_max, q.unvoiced_period) == (16, -7, 4, 40, 20)
    for bad in (dict(unvoiced_period=0), dict(unvoiced_period=1025), dict(unvoiced_period=2.5), dict(hop_length=0), dict(fmin=10.0)):
        kw = dict(sampling_rate=22050, hop_length=256)
        kw.update(bad)
        with pytest.raises(ValueError):
            metrics.psola_params(**kw)
    z, zi = torch.zeros(1, 4096), torch.zeros(1, 16, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        metrics.pitch_shift(z, None, zi, torch.ones(1, 16), sampling_rate=22050, hop_length=256)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        metrics.psola_plan(z, None, zi, torch.ones(1, 16), sampling_rate=22050, hop_length=256)
    with pytest.raises(TypeError):
        metrics.pitch_shift(z, None, zi, torch.ones(1, 16))   # the rate and the hop have no defaults
    # the C ABI's own checks run before anything is launched: made-up addresses are never touched
    A = 1 << 20
    ok = lambda **k: _lib.gvx_psola_params(**{**dict(hop=256, first_centre=0, lag_min=44, lag_max=368, unvoiced_period=220), **k})
    names = ("wav", "lag", "ratio", "marks", "periods", "pos", "src", "counts", "status")

    def plan(p, B=1, N=4096, **null):
        a = {k: (None if k in null else A) for k in names}
        return lib.gvx_psola_plan(a["wav"], None, a["lag"], a["ratio"], B, N, p, a["marks"], a["periods"], a["pos"], a["src"], a["counts"], a["status"], None)

    def synth(p, B=1, N=4096, **null):
        a = {k: (None if k in null else A) for k in names + ("out",)}
        return lib.gvx_psola_synth(a["wav"], None, a["marks"], a["periods"], a["pos"], a["src"], a["counts"], a["status"], B, N, p, a["out"], None)

    for call in (plan, synth):
        for p in (ok(hop=0), ok(lag_min=0), ok(lag_min=369), ok(unvoiced_period=0), ok(lag_max=0), None):
            assert call(p) == -1
        assert call(ok(), B=0) == -1 and call(ok(), N=0) == -1
        for p in (ok(lag_max=1025), ok(unvoiced_period=1025)):
            assert call(p) == -2 and b"limit" in lib.gvx_last_error()
        assert call(ok(), B=65536) == -2 and call(ok(hop=1), N=32769) == -2 and b"frames" in lib.gvx_last_error()
        assert call(ok(hop=2 ** 20), N=2 ** 25 + 1) == -2
    for k in names:
        assert plan(ok(), **{k: True}) == -1, k
    for k in ("wav", "marks", "periods", "pos", "src", "counts", "status", "out"):
        assert synth(ok(), **{k: True}) == -1, k
