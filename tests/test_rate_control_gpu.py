"""GPU: speaking rate control - the plan (gvx_duration_scale), the warp (gvx_mel_time_warp) and the Synthesizer path built on them.

Plan.  Every output equals tests/warp_ref.duration_scale exactly: both sides do the same IEEE double operations in the same order
(one multiply, one divide and one add per token, to nearest-even), so there is no tolerance.

Warp.  src_frame_out and the bits of src_frac_out equal the restatement (exact integers; the double quotient and its conversion to
fp32 round the same way on both sides).  mel_out against the float64 value x0 + frac (x1 - x0) formed from the device's own frac,
under the derived bound of warp_ref.interp_bound: half an fp32 ulp of |x1 - x0| for the subtraction plus half an ulp of the result
for the fused multiply-add - the two roundings the formula contains (the library is built with -ffp-contract=off and the fmaf is
explicit) - and exactly 0 where frac == 0.  Largest error observed on the MI355X over every case of this file: see EXPERIMENTS.md,
"Speaking rate control" (the tests print it, in ulps of the larger of |x1 - x0| and |result| - under cancellation an ulp of the
result alone says nothing about a rounding of the difference - and as a fraction of the bound).
"""
import os

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from genvox_amd.synthesizer import token_rates, token_times
from tests import warp_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 1024
SENT = 0x5A
NAN_BITS = 0x7FC00000     # as an int32: a poison duration; as an fp32: NaN


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A tensor of `shape` in the middle of one allocation, 0x5A bytes all over it and in GUARD bytes on both sides."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape)) * 4
        self.buf = torch.full((2 * GUARD + self.n,), SENT, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


# ---- the plan -------------------------------------------------------------------------------------------------------------------

def call_plan(d, tl=None, rates=None, speed=1.0, want_starts=True, expect=0):
    lib = _lib.load()
    B, L = np.asarray(d).shape
    dd, tt, rr = _dev(d, torch.int32), _dev(tl, torch.int32), _dev(rates, torch.float32)
    o = {"durations": Guarded((B, L), torch.int32), "starts": Guarded((B, L), torch.int32), "out_lengths": Guarded((B,), torch.int32),
         "status": Guarded((B,), torch.int32)}
    rc = lib.gvx_duration_scale(dd.data_ptr(), _p(tt), _p(rr), B, L, speed, o["durations"].ptr(), o["starts"].ptr() if want_starts else None,
                                o["out_lengths"].ptr(), o["status"].ptr(), _stream())
    assert rc == expect, (rc, lib.gvx_last_error())
    torch.cuda.synchronize()
    assert all(g.intact() for g in o.values()), "a guard byte of an output was written"
    if not want_starts:
        assert o["starts"].untouched()
    return {k: g.t.cpu().numpy() for k, g in o.items()}


def check_plan(d, tl=None, rates=None, speed=1.0, what=""):
    got = call_plan(d, tl, rates, speed)
    want = ref.duration_scale(d, tl, speed, rates)
    for k in ("status", "out_lengths", "durations", "starts"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} places"
    return want


SPEEDS = (0.125, 0.3, 0.5, 0.8, 1.0, 1.25, 2.0, 3.7, 8.0)
PLAN_SHAPES = ((1, 1), (2, 2), (3, 63), (64, 64), (5, 65), (7, 1000), (4, 4096))


def _durations(rng, B, L, hi=9, zeros=0.1):
    d = rng.integers(1, hi, (B, L))
    d[rng.random((B, L)) < zeros] = 0
    d[:, 0] = np.maximum(d[:, 0], 1)
    return d.astype(np.int32)


@pytest.mark.parametrize("B,L", PLAN_SHAPES)
def test_plan_equals_the_restatement_at_global_speeds(B, L):
    rng = np.random.default_rng(100 * B + L)
    d = _durations(rng, B, L, hi=7 if L == 4096 else 9)
    for speed in SPEEDS:
        want = check_plan(d, speed=speed, what=f"{B}x{L} speed {speed}")
        ok = want["status"] == ref.OK
        assert ok.all() or (L >= 1000 and speed < 0.5)                   # thousands of tokens slowed down pass 32768 frames: BAD
        if speed == 1.0:
            assert np.array_equal(want["durations"], d)
    got = call_plan(d, speed=1.25, want_starts=False)                     # starts_out may be NULL
    assert np.array_equal(got["durations"], ref.duration_scale(d, None, 1.25)["durations"])


@pytest.mark.parametrize("B,L", PLAN_SHAPES)
def test_plan_with_random_per_token_rates(B, L):
    rng = np.random.default_rng(7 * B + L)
    d = _durations(rng, B, L, hi=5 if L == 4096 else 9)
    for speed in (0.5, 1.0, 1.6, 4.0):
        rates = rng.uniform(max(0.125 / speed, 0.4), min(8.0 / speed, 2.5), (B, L)).astype(np.float32)
        want = check_plan(d, rates=rates, speed=speed, what=f"{B}x{L} rates at speed {speed}")
        assert (want["status"] == ref.OK).all() or L == 4096
        assert ((want["durations"] > 0) == (d > 0)).all() or L == 4096


def test_plan_rounds_exact_ties_to_even():
    rng = np.random.default_rng(3)
    B, L = 6, 300
    d = (2 * rng.integers(0, 6, (B, L)) + 1).astype(np.int32)             # odd counts at e = 2: every second E ends in .5
    want = check_plan(d, speed=2.0, what="odd counts at speed 2")
    E = np.cumsum(d / 2.0, axis=1)
    assert (E % 1 == 0.5).sum() > B * L // 3                              # the ties are there
    ones = np.ones((2, 64), np.int32)
    rates = np.full((2, 64), 2.0, np.float32)
    rates[1] = 4.0                                                        # E = 0.25 l: .5 at every second pair
    want = check_plan(ones, rates=rates, speed=1.0, what="single frames at rate 2 and 4")
    assert want["durations"].tolist() == ones.tolist()                    # the one-frame minimum binds all along
    d = np.array([[5, 2, 4, 1, 6, 3]], np.int32)                          # E = 2.5 3.5 5.5 6 9 10.5 -> 2 4 6 6 9 10
    want = check_plan(d, speed=2.0, what="by hand")
    assert want["starts"].tolist() == [[0, 2, 4, 6, 7, 9]] and want["out_lengths"].tolist() == [10]


def test_plan_empty_bad_and_ragged_rows_with_poison_behind_the_lengths():
    rng = np.random.default_rng(11)
    B, L = 12, 130
    d = _durations(rng, B, L)
    rates = rng.uniform(0.5, 2.0, (B, L)).astype(np.float32)
    tl = rng.integers(1, L + 1, B).tolist()
    tl[0], tl[1], tl[2], tl[3] = 0, -4, L + 50, L                         # EMPTY, clamped to 0: EMPTY, clamped to L
    d[4, :tl[4]] = 0                                                      # a duration sum of 0: EMPTY
    tl[5] = max(tl[5], 3); d[5, 1] = -1                                   # BAD: a negative duration
    tl[6] = max(tl[6], 3); rates[6, 2] = np.nan                           # BAD: a rate that is not finite
    tl[7] = max(tl[7], 3); rates[7, 0] = np.inf
    tl[8] = max(tl[8], 3); rates[8, 1] = 0.0                              # BAD: a rate that is not positive
    tl[9] = max(tl[9], 3); rates[9, 1] = -1.0
    tl[10] = max(tl[10], 3); rates[10, 2] = 8.0                           # BAD: e = 1.5 * 8 above GVX_RATE_MAX
    tl[11] = max(tl[11], 3); rates[11, 2] = 0.05                          # BAD: e = 0.075 below GVX_RATE_MIN
    want = check_plan(d, tl, rates, 1.5, "ragged")
    assert want["status"].tolist() == [ref.EMPTY, ref.EMPTY, ref.OK, ref.OK, ref.EMPTY] + [ref.BAD] * 7
    for b in range(B):
        if want["status"][b] != ref.OK:
            assert (want["durations"][b] == 0).all() and (want["starts"][b] == -1).all() and want["out_lengths"][b] == 0
    # poison behind every row's tokens changes no output
    pd, pr = d.copy(), rates.copy()
    for b in range(B):
        Lb = max(0, min(tl[b], L))
        pd[b, Lb:] = NAN_BITS if b % 2 else -7
        pr[b, Lb:] = np.nan if b % 2 else -np.inf
    got = call_plan(pd, tl, pr, 1.5)
    for k in ("status", "out_lengths", "durations", "starts"):
        assert np.array_equal(got[k], want[k]), f"poison behind the lengths changed {k}"
    # a row whose new length passes GVX_MAS_MAX_FRAMES is BAD; at the limit itself it is OK
    big = np.full((2, 4096), 8, np.int32)
    big[1, 0] = 9
    want = check_plan(big, speed=1.0, what="32768 and 32769 frames")
    assert want["status"].tolist() == [ref.OK, ref.BAD] and want["out_lengths"].tolist() == [32768, 0]
    again = call_plan(big, speed=1.0)
    assert np.array_equal(again["durations"], want["durations"])


# ---- the warp -------------------------------------------------------------------------------------------------------------------

_WORST = {"ulp": 0.0, "of_bound": 0.0}


def call_warp(mel, d, dp, tl, T_out, want_map=True, expect=0):
    """One gvx_mel_time_warp on host arrays; every output in its own guarded allocation."""
    lib = _lib.load()
    B, M, T = mel.shape
    L = np.asarray(d).shape[1]
    x, dd, pp, tt = torch.from_numpy(mel).cuda(), _dev(d, torch.int32), _dev(dp, torch.int32), _dev(tl, torch.int32)
    o = {"mel": Guarded((B, M, T_out), torch.float32), "src_frame": Guarded((B, T_out), torch.int32),
         "src_frac": Guarded((B, T_out), torch.float32), "status": Guarded((B,), torch.int32)}
    rc = lib.gvx_mel_time_warp(x.data_ptr(), dd.data_ptr(), pp.data_ptr(), _p(tt), B, M, T, L, T_out, o["mel"].ptr(),
                               o["src_frame"].ptr() if want_map else None, o["src_frac"].ptr() if want_map else None, o["status"].ptr(), _stream())
    assert rc == expect, (rc, lib.gvx_last_error())
    torch.cuda.synchronize()
    assert all(g.intact() for g in o.values()), "a guard byte of an output was written"
    if not want_map:
        assert o["src_frame"].untouched() and o["src_frac"].untouched()
    return {k: g.t.cpu().numpy() for k, g in o.items()}


def check_warp(mel, d, dp, tl, T_out, what):
    """The device against the restatement: map exact, frac bit for bit, mel under the derived bound from the device's own frac."""
    got = call_warp(mel, d, dp, tl, T_out)
    want = ref.mel_time_warp(mel, d, dp, tl, T_out)
    assert np.array_equal(got["status"], want["status"]), f"{what}: status {got['status'].tolist()} != {want['status'].tolist()}"
    assert np.array_equal(got["src_frame"], want["src_frame"]), f"{what}: src_frame differs"
    assert np.array_equal(got["src_frac"].view(np.int32), want["src_frac"].view(np.int32)), f"{what}: the bits of src_frac differ"
    B, M, T = mel.shape
    for b in range(B):
        n = int((got["src_frame"][b] >= 0).sum())
        assert (got["src_frame"][b, :n] >= 0).all() and (got["mel"][b, :, n:].view(np.int32) == 0).all(), f"{what}: row {b}: not exact zeros behind T'"
        if n == 0:
            continue
        i0, frac = got["src_frame"][b, :n], got["src_frac"][b, :n]
        x0 = mel[b][:, i0].astype(np.float64)
        x1 = mel[b][:, np.where(frac == 0, i0, np.minimum(i0 + 1, T - 1))].astype(np.float64)     # where frac == 0 the neighbour is not looked at
        x1 = np.where(frac[None, :] == 0, x0, x1)
        want64 = x0 + frac.astype(np.float64)[None, :] * (x1 - x0)
        bound = ref.interp_bound(x0, x1, np.broadcast_to(frac[None, :], x0.shape))
        g = got["mel"][b, :, :n].astype(np.float64)
        assert np.isfinite(g).all(), f"{what}: row {b}: poison reached the output"
        err = np.abs(g - want64)
        assert (err <= bound).all(), f"{what}: row {b}: {int((err > bound).sum())} values beyond the derived bound, worst {np.max(err - bound):.3e} over"
        exact = np.broadcast_to(frac[None, :] == 0, x0.shape)
        assert np.array_equal(got["mel"][b, :, :n][exact].view(np.int32), mel[b][:, i0][exact].view(np.int32)), f"{what}: frac == 0 must return x0's bits"
        scale = np.maximum(np.abs(want64), np.abs(x1 - x0))          # what the two roundings act on: the difference and the result
        ulps = err / np.spacing(np.where(exact, 1.0, scale).astype(np.float32)).astype(np.float64)
        _WORST["ulp"] = max(_WORST["ulp"], float(ulps.max()))
        _WORST["of_bound"] = max(_WORST["of_bound"], float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0)
    print(f"[warp] {what}: largest interpolation error so far {_WORST['ulp']:.3f} ulp of max(|x1 - x0|, |result|) (at most 1 by the bound), "
          f"{_WORST['of_bound']:.3f} of the derived bound")
    return got, want


def _case(seed, B, M, L, speed, ragged=True, hi=9):
    """Durations, a plan for them from the restatement, ragged token lengths and a mel that is NaN at and behind every row's T_b;
    the padded token columns of both tables hold poison."""
    rng = np.random.default_rng(seed)
    d = _durations(rng, B, L, hi=hi)
    tl = rng.integers(max(1, L // 2), L + 1, B).tolist() if ragged else [L] * B
    rates = rng.uniform(max(0.125 / speed, 0.5), min(8.0 / speed, 2.0), (B, L)).astype(np.float32)
    plan = ref.duration_scale(d, tl, speed, rates)
    assert (plan["status"] == ref.OK).all()
    dp = plan["durations"].copy()
    Tb = [int(d[b, :tl[b]].sum()) for b in range(B)]
    T = max(Tb) + 3
    mel = (4.0 * rng.standard_normal((B, M, T)) - 5.0).astype(np.float32)
    for b in range(B):
        mel[b, :, Tb[b]:] = np.nan
        d[b, tl[b]:] = NAN_BITS
        dp[b, tl[b]:] = NAN_BITS if b % 2 else -9
    return mel, d, dp, tl, plan["out_lengths"].tolist()


@pytest.mark.parametrize("M", [8, 80, 81])
@pytest.mark.parametrize("speed", [0.5, 0.8, 1.25, 2.0])
def test_warp_equals_the_restatement(M, speed):
    mel, d, dp, tl, Tp = _case(int(100 * speed) + M, 5, M, 40, speed)
    got, want = check_warp(mel, d, dp, tl, max(Tp), f"M {M} speed {speed}")
    assert want["status"].tolist() == [ref.OK] * 5
    # without the map outputs: the same mel bits; a second call: the same bits
    bare = call_warp(mel, d, dp, tl, max(Tp), want_map=False)
    assert np.array_equal(bare["mel"].view(np.int32), got["mel"].view(np.int32)) and np.array_equal(bare["status"], got["status"])
    again = call_warp(mel, d, dp, tl, max(Tp))
    for k in got:
        assert np.array_equal(again[k].view(np.int32), got[k].view(np.int32)), k


def test_warp_T_out_around_the_tile_and_around_the_row():
    assert ref.TILE == 64
    mel, d, dp, tl, Tp = _case(5, 3, 8, 30, 0.8)
    assert min(Tp) > ref.TILE + 1
    for T_out in sorted({ref.TILE - 1, ref.TILE, ref.TILE + 1, 2 * ref.TILE - 1, 2 * ref.TILE, 2 * ref.TILE + 1, 1}
                        | {t + k for t in Tp for k in (-1, 0, 1)}):
        got, want = check_warp(mel, d, dp, tl, T_out, f"T_out {T_out}")
        assert got["status"].tolist() == [ref.CUT if t > T_out else ref.OK for t in Tp]
    # a single token stretched over exactly one, and one more than one, tile
    one = (np.arange(8 * 5, dtype=np.float32).reshape(1, 8, 5) - 7.0)
    for n in (ref.TILE - 1, ref.TILE, ref.TILE + 1):
        check_warp(one, np.array([[5]], np.int32), np.array([[n]], np.int32), None, n, f"5 -> {n} frames")


def test_warp_equal_tables_return_the_input_bits():
    mel, d, _, tl, _ = _case(9, 4, 80, 100, 1.0)
    dp = d.copy()
    Tb = [int(d[b, :tl[b]].sum()) for b in range(4)]
    got = call_warp(mel, d, dp, tl, max(Tb))
    for b in range(4):
        assert np.array_equal(got["mel"][b, :, :Tb[b]].view(np.int32), mel[b, :, :Tb[b]].view(np.int32))
        assert (got["mel"][b, :, Tb[b]:].view(np.int32) == 0).all()
        assert got["src_frame"][b, :Tb[b]].tolist() == list(range(Tb[b])) and (got["src_frac"][b] == 0).all()
    weird = mel.copy()                                                        # inf, NaN and -0.0 inside the row come through as they are
    weird[0, 0, 0], weird[0, 1, 1], weird[0, 2, 2] = np.inf, np.nan, -0.0
    got = call_warp(weird, d, dp, tl, max(Tb))
    assert np.array_equal(got["mel"][0, :, :Tb[0]].view(np.int32), weird[0, :, :Tb[0]].view(np.int32))


@pytest.mark.parametrize("B,L,hi", [(1, 1, 9), (64, 64, 9), (2, 4096, 4), (3, 1000, 6)])
def test_warp_batch_and_token_extremes(B, L, hi):
    mel, d, dp, tl, Tp = _case(B + L, B, 8, L, 1.25, ragged=L > 1, hi=hi)
    check_warp(mel, d, dp, tl, max(Tp), f"{B} rows of {L} tokens")


def test_warp_bad_and_empty_rows_come_out_zero():
    mel, d, dp, tl, Tp = _case(21, 7, 8, 20, 0.8)
    tl[0] = 0                                              # EMPTY
    d[1, 3] = -2                                           # BAD: a negative entry
    dp[2, 0] = -1
    k = int(np.argmax(d[3, :tl[3]] > 0)); dp[3, k] = 0     # BAD: d > 0 with d' == 0
    z = int(np.argmax(d[4, :tl[4]] == 0)); assert d[4, z] == 0; dp[4, z] = 2      # BAD: the converse
    d[5, 0] += mel.shape[2]                                # BAD: T_b > T
    got, want = check_warp(mel, d, dp, tl, max(Tp), "bad rows")
    assert got["status"].tolist() == [ref.EMPTY] + [ref.BAD] * 5 + [ref.OK]
    for b in range(6):
        assert (got["mel"][b].view(np.int32) == 0).all() and (got["src_frame"][b] == -1).all() and (got["src_frac"][b].view(np.int32) == 0).all()
    huge = np.array([[3, 2]], np.int32), np.array([[2 ** 31 - 1, 2 ** 31 - 1]], np.int32)      # sums beyond 32 bits: CUT, the first frames computed
    one = np.arange(40, dtype=np.float32).reshape(1, 8, 5)
    got, _ = check_warp(one, huge[0], huge[1], None, 70, "target counts of 2^31 - 1")
    assert got["status"].tolist() == [ref.CUT] and (got["src_frame"][0] == 0).all()


def test_the_python_wrappers_return_the_same():
    mel, d, dp, tl, Tp = _case(33, 4, 80, 50, 1.25)
    want = ref.duration_scale(np.where(d == NAN_BITS, 0, d), tl, 1.25)
    plan = metrics.scale_durations(torch.from_numpy(d).cuda(), torch.tensor(tl).cuda(), speed=1.25)
    assert set(plan) == {"durations", "starts", "out_lengths", "status"}
    for k, v in want.items():
        assert np.array_equal(plan[k].cpu().numpy(), v), k
    out = metrics.time_warp(torch.from_numpy(mel).cuda(), torch.from_numpy(d).cuda(), plan["durations"], torch.tensor(tl).cuda())
    assert set(out) == {"mel", "src_frame", "src_frac", "status"}
    assert out["mel"].shape == (4, 80, int(want["out_lengths"].max()))                     # T_out = None: the longest row
    raw = call_warp(mel, d, want["durations"], tl, int(want["out_lengths"].max()))
    for k, v in raw.items():
        assert np.array_equal(out[k].cpu().numpy().view(np.int32), v.view(np.int32)), k
    with pytest.raises(RuntimeError):
        metrics.scale_durations(torch.from_numpy(d))
    with pytest.raises(_lib.GvxError):
        metrics.scale_durations(torch.from_numpy(d).cuda(), speed=9.0)
    with pytest.raises(ValueError):
        metrics.time_warp(torch.from_numpy(mel).cuda(), torch.from_numpy(d).cuda(), plan["durations"][:2])


# ---- the Synthesizer ----------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OLD_KEYS = {"mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments", "waveform", "sampling_rate"}
SENTENCES = ["a cat.", "hi, you two.", "this sentence has many more tokens than frames."]


@pytest.fixture(scope="module")
def syn():
    from genvox_amd.synthesizer import Synthesizer
    from genvox_amd.tacotron2 import Tacotron2

    exp = os.path.join(GOLDEN, "ref_exp")
    return Synthesizer(tts_model_class=Tacotron2, tts_config_path=os.path.join(exp, "config.yaml"),
                       tts_checkpoint_path=os.path.join(exp, "checkpoint_3.pt"), use_cuda=True)


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a == b


def _own_plan(res, n_tokens, speed, rates=None):
    """The restatement's plan on the durations of the result's own alignment (one token of all frames where the search is infeasible)."""
    a = torch.from_numpy(res["alignments"])[None].cuda()
    al = metrics.monotonic_align(a)
    T = res["alignments"].shape[0]
    if int(al["status"][0]) != 0:
        assert T < n_tokens
        return [T], ref.plan_row([T], speed)
    d = al["durations"][0].cpu().tolist()
    return d, ref.plan_row(d, speed, rates)


def _check_paced(syn, text, res, speed, rates=None):
    toks = syn.text_processor.tokenize(text)
    ap = syn.audio_processor
    d, (st, dp, starts, Tp) = _own_plan(res, len(toks), speed, rates)
    assert st == ref.OK
    assert res["speed"] == speed and res["mel_outputs_warped"].shape == (res["mel_outputs_postnet"].shape[0], Tp)     # T' is the plan's
    assert res["waveform"].shape == (ap.row_samples([Tp])[0],)
    x = torch.from_numpy(res["mel_outputs_postnet"])[None].cuda()
    own = metrics.time_warp(x, torch.tensor([d], dtype=torch.int32).cuda(), torch.tensor([dp], dtype=torch.int32).cuda(), T_out=Tp)
    assert _same(own["mel"][0].cpu().numpy(), res["mel_outputs_warped"])
    alone = ap.convert_mel2wav_batch(torch.from_numpy(res["mel_outputs_warped"])[None].cuda())[0].cpu().numpy()
    assert np.array_equal(res["waveform"], alone)                       # the waveform is the vocoder on the warped mel
    if "timings_status" in res:
        if len(d) != len(toks):
            assert res["timings_status"] == "infeasible" and res["token_timings"] == []
        else:
            assert res["timings_status"] == "ok"
            tt = res["token_timings"]
            s, e = [v for _, v, _ in tt], [v for _, _, v in tt]
            assert [t for t, _, _ in tt] == toks and e[:-1] == s[1:] and all(a <= b for a, b in zip(s, s[1:]))
            assert e[-1] == len(res["waveform"]) / res["sampling_rate"] and e[-1] >= s[-1]
            ws, we = token_times(starts, ap.config.hop_length, ap.TRIM, ap.row_samples([Tp])[0], ap.config.sampling_rate, e[-1])
            assert s == ws and e == we                                  # the timings are token_times of the plan's own starts
    return d, dp, starts, Tp


def test_speed_one_is_todays_tts(syn):
    for text in SENTENCES[:2]:
        torch.manual_seed(3)
        plain = syn.tts(text, timings=True)
        after_plain = torch.rand(1)
        torch.manual_seed(3)
        same = syn.tts(text, timings=True, speed=1.0, word_speed=None, token_speed=None)
        after_same = torch.rand(1)
        assert set(plain) == set(same) == OLD_KEYS | {"token_timings", "word_timings", "timings_status"}
        for k in plain:
            assert _same(plain[k], same[k]), k
        assert torch.equal(after_plain, after_same)
        torch.manual_seed(3)
        assert set(syn.tts(text, speed=1.0)) == OLD_KEYS


@pytest.mark.parametrize("speed", [0.5, 0.8, 1.25, 2.0])
def test_tts_at_a_global_speed(syn, speed):
    seen = set()
    for text in SENTENCES:
        torch.manual_seed(3)
        plain = syn.tts(text)
        torch.manual_seed(3)
        res = syn.tts(text, speed=speed, timings=True)
        assert set(res) == OLD_KEYS | {"mel_outputs_warped", "speed", "token_timings", "word_timings", "timings_status"}
        for k in OLD_KEYS - {"waveform"}:
            assert _same(plain[k], res[k]), k                           # the decode is what it was
        d, dp, _, Tp = _check_paced(syn, text, res, speed)
        seen.add(res["timings_status"])
        if res["timings_status"] == "ok" and speed == 0.5:
            assert dp == [2 * v for v in d] and Tp == 2 * sum(d)
    assert seen == {"ok", "infeasible"}
    torch.manual_seed(3)
    low = syn.tts(SENTENCES[0], speed=speed, timings=True, sampling_rate=16000)
    torch.manual_seed(3)
    own = syn.tts(SENTENCES[0], speed=speed, timings=True)
    assert [x[:2] for x in low["token_timings"]] == [x[:2] for x in own["token_timings"]] and low["sampling_rate"] == 16000


def test_word_speed_slows_one_word_and_leaves_the_words_ahead_alone(syn):
    text = SENTENCES[1]
    toks = syn.text_processor.tokenize(text)
    rates = token_rates(toks, {1: 0.5})
    named = [l for l, r in enumerate(rates) if r == 0.5]
    assert "".join(toks[l] for l in named) == "you"
    torch.manual_seed(3)
    res = syn.tts(text, word_speed={1: 0.5}, timings=True)
    assert res["timings_status"] == "ok"
    d, dp, starts, Tp = _check_paced(syn, text, res, 1.0, rates)
    want = ref.plan_row(d, 1.0, rates)[1]
    assert [dp[l] for l in named] == [want[l] for l in named] == [2 * d[l] for l in named]          # that word's tokens, per the plan
    assert [dp[l] for l in range(len(toks)) if l not in named] == [d[l] for l in range(len(toks)) if l not in named]
    ahead = sum(d[:named[0]])                                                                       # frames of "hi, " - untouched, bit for bit
    assert ahead > 0 and starts[named[0]] == ahead
    assert _same(res["mel_outputs_warped"][:, :ahead], res["mel_outputs_postnet"][:, :ahead])
    assert Tp == sum(d) + sum(d[l] for l in named)
    torch.manual_seed(3)
    per_token = syn.tts(text, token_speed=rates, timings=True)                                      # the same rates, given per token
    for k in res:
        assert _same(res[k], per_token[k]), k
    with pytest.raises(ValueError, match="sentence 0"):
        syn.tts(text, speed=8.0, word_speed={1: 2.0})                                               # e = 16: the plan is BAD
    for bad in (dict(speed=0.0), dict(speed=9.0), dict(speed=float("nan")), dict(word_speed=[1.0]), dict(token_speed=[1.0]), dict(word_speed={7: 1.0})):
        with pytest.raises(ValueError):
            syn.tts(text, **bad)


def test_tts_batch_with_mixed_lengths_and_rates_per_sentence(syn):
    toks = [syn.text_processor.tokenize(t) for t in SENTENCES]
    word_speed = [{0: 0.5}, None, None]
    token_speed = [None, [1.0 + 0.1 * (l % 3) for l in range(len(toks[1]))], None]
    rates = [syn._sentence_rates(toks[i], word_speed[i], token_speed[i]) for i in range(3)]
    torch.manual_seed(5)
    plain = syn.tts_batch(SENTENCES)
    torch.manual_seed(5)
    got = syn.tts_batch(SENTENCES, speed=1.25, word_speed=word_speed, token_speed=token_speed, timings=True)
    seen = set()
    for i, (text, p, r) in enumerate(zip(SENTENCES, plain, got)):
        assert set(r) == OLD_KEYS | {"mel_outputs_warped", "speed", "token_timings", "word_timings", "timings_status"}
        for k in OLD_KEYS - {"waveform"}:
            assert _same(p[k], r[k]), (i, k)                            # the decode is the batch's decode as it was
        d = _own_plan(r, len(toks[i]), 1.25)[0]
        _check_paced(syn, text, r, 1.25, rates[i] if len(d) == len(toks[i]) else None)   # an infeasible row: one token at the global speed
        seen.add(r["timings_status"])
    assert seen == {"ok", "infeasible"}
    for i in (0, 1):                                                    # a batch of one sentence is exactly the tts path
        torch.manual_seed(11)
        one = syn.tts(SENTENCES[i], speed=0.8, word_speed=word_speed[i], token_speed=token_speed[i], timings=True)
        torch.manual_seed(11)
        row = syn.tts_batch([SENTENCES[i]], speed=0.8, word_speed=[word_speed[i]], token_speed=[token_speed[i]], timings=True)
        assert len(row) == 1 and set(row[0]) == set(one)
        for k in one:
            assert _same(one[k], row[0][k]), (i, k)
    torch.manual_seed(5)
    assert all(set(r) == OLD_KEYS for r in syn.tts_batch(SENTENCES, speed=1.0))
    with pytest.raises(ValueError, match="sentence 1"):
        syn.tts_batch(SENTENCES, speed=8.0, token_speed=[None, [2.0] * len(toks[1]), None])
    with pytest.raises(ValueError):
        syn.tts_batch(SENTENCES, word_speed=[None])
