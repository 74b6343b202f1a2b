"""Speaking rate control without a GPU: rates per word -> rates per token, the properties of the numpy restatement of the plan
(tests/warp_ref.py) and of its frame map, the two C-ABI entries as the header declares them, and their argument checks (nothing
is launched)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from genvox_amd import _lib
from genvox_amd.synthesizer import group_words, token_rates
from tests import warp_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- rates per word -> rates per token ----------------------------------------------------------------------------------------------

def test_token_rates_plain_sentence_both_forms():
    toks = list("hello, world.")
    #            h    e    l    l    o    ,    ' '  w    o    r    l    d    .
    assert token_rates(toks, [0.5, 2.0]) == [0.5] * 6 + [1.0] + [2.0] * 6           # punctuation stays on the word it touches
    assert token_rates(toks, {1: 2.0}) == [1.0] * 7 + [2.0] * 6                     # an unnamed word and the space get 1.0
    assert token_rates(toks, {}) == [1.0] * 13 and token_rates(toks, None) == [1.0] * 13
    assert token_rates(toks, (1, 3)) == [1.0] * 7 + [3.0] * 6                       # whole numbers are rates too
    assert token_rates(toks, np.array([0.5, 2.0], np.float32)) == [0.5] * 6 + [1.0] + [2.0] * 6


def test_token_rates_leading_trailing_and_double_spaces():
    toks = list("  a  bc ")
    assert [w for w, _, _ in group_words(toks, [0.0] * 8, [0.0] * 8)] == ["a", "bc"]     # the segmentation the rates are counted in
    assert token_rates(toks, [4.0, 0.25]) == [1.0, 1.0, 4.0, 1.0, 1.0, 0.25, 0.25, 1.0]
    assert token_rates(toks, {0: 4.0}) == [1.0, 1.0, 4.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert token_rates(list("   "), []) == [1.0, 1.0, 1.0] and token_rates([], []) == [] and token_rates([], {}) == []
    toks = list(" one two,  three! ")
    got = token_rates(toks, {2: 0.5, 0: 2.0})
    assert got == [1.0] + [2.0] * 3 + [1.0] + [1.0] * 4 + [1.0, 1.0] + [0.5] * 6 + [1.0]
    assert len(got) == len(toks)


def test_token_rates_refusals():
    toks = list("ab cd ef")
    for bad in ([1.0, 2.0], [1.0] * 4, []):                                          # a wrong count
        with pytest.raises(ValueError, match="3 words"):
            token_rates(toks, bad)
    for bad in ({3: 1.0}, {-1: 1.0}, {"0": 1.0}, {1.0: 1.0}, {True: 1.0}):            # not the number of a word
        with pytest.raises(ValueError, match="word index"):
            token_rates(toks, bad)
    for rate in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="finite number above 0"):
            token_rates(toks, [1.0, rate, 1.0])
        with pytest.raises(ValueError, match="finite number above 0"):
            token_rates(toks, {1: rate})


# ---- the plan's restatement -------------------------------------------------------------------------------------------------------

def _random_durations(rng, L, zeros=True):
    d = rng.integers(1, 12, L)
    if zeros:
        d[rng.random(L) < 0.15] = 0
    return d.tolist()


def test_plan_by_hand():
    # speed 2: E = 1.5, 3, 3.5, 6 -> c = 2, 3, 4 (3.5 is a tie: to the even 4), 6
    assert ref.plan_row([3, 3, 1, 5], 2.0) == (ref.OK, [2, 1, 1, 2], [0, 2, 3, 4], 6)
    # speed 0.5: every count doubles
    assert ref.plan_row([3, 0, 2], 0.5) == (ref.OK, [6, 0, 4], [0, 6, 6], 10)
    # speed 8 on single frames: E = 0.125 l; every spoken token keeps its frame although c lags behind
    assert ref.plan_row([1] * 5, 8.0) == (ref.OK, [1] * 5, [0, 1, 2, 3, 4], 5)
    # ties: E = 0.5 -> 0 (even), then the minimum binds; E = 2.5 -> 2, E = 3.5 -> 4
    assert ref.plan_row([1], 2.0) == (ref.OK, [1], [0], 1)
    assert ref.plan_row([5, 2], 2.0) == (ref.OK, [2, 2], [0, 2], 4)
    # per-token rates: token 1 at half speed, the others untouched
    assert ref.plan_row([4, 3, 4], 1.0, [1.0, 0.5, 1.0]) == (ref.OK, [4, 6, 4], [0, 4, 10], 14)
    assert ref.plan_row([], 1.0)[0] == ref.EMPTY and ref.plan_row([0, 0], 1.0) == (ref.EMPTY, [0, 0], [-1, -1], 0)
    assert ref.plan_row([2, -1], 1.0)[0] == ref.BAD
    for rate in (0.0, -1.0, float("nan"), float("inf"), 0.01, 100.0):
        assert ref.plan_row([2, 2], 1.0, [1.0, rate])[0] == ref.BAD
    assert ref.plan_row([2, 2], 4.0, [1.0, 4.0])[0] == ref.BAD and ref.plan_row([2, 2], 4.0, [1.0, 2.0])[0] == ref.OK   # e = 16, e = 8
    assert ref.plan_row([8192] * 4, 1.0)[0] == ref.OK and ref.plan_row([8192] * 4 + [1], 1.0)[0] == ref.BAD             # 32768 frames, 32769


@pytest.mark.parametrize("seed", range(6))
def test_plan_properties_on_random_durations(seed):
    rng = np.random.default_rng(seed)
    for trial in range(40):
        L = int(rng.integers(1, 200))
        d = _random_durations(rng, L)
        if sum(d) == 0:
            d[0] = 3
        st, dp, starts, Tp = ref.plan_row(d, 1.0)
        assert (st, dp, Tp) == (ref.OK, d, sum(d))                                   # speed 1 is the identity
        assert starts == np.concatenate([[0], np.cumsum(d)[:-1]]).tolist()
        speed = float(np.float32(rng.uniform(0.125, 8.0)))
        rates = None if trial % 2 else rng.uniform(0.5, 2.0, L).astype(np.float32)
        e = [speed * (1.0 if rates is None else float(rates[l])) for l in range(L)]
        if not all(0.125 <= v <= 8.0 for v in e):
            assert ref.plan_row(d, speed, rates)[0] == ref.BAD
            continue
        st, dp, starts, Tp = ref.plan_row(d, speed, rates)
        assert st == ref.OK
        assert sum(dp) == Tp and starts[0] == 0                                      # sum d' == T'
        assert all(a <= b for a, b in zip(starts, starts[1:])) and starts[-1] + dp[-1] == Tp     # starts are non-decreasing
        assert all((a > 0) == (b > 0) for a, b in zip(d, dp))                        # a spoken token has >= 1 frame, a silent one none
        E, binds, S = 0.0, False, 0
        for l in range(L):
            E += d[l] / e[l]
            binds = binds or (S + (d[l] > 0) > round(E))
            S = max(S + (d[l] > 0), round(E))
        if not binds:
            assert Tp == round(E)                                                    # T' == round(sum d / e) where no minimum binds
        assert abs(Tp - E) <= 0.5 or binds
    # slow enough, nothing binds: T' is the rounded sum for every row
    d = _random_durations(rng, 50, zeros=False)
    st, dp, _, Tp = ref.plan_row(d, 0.5)
    assert st == ref.OK and Tp == 2 * sum(d) and dp == [2 * v for v in d]


def test_batched_restatement_pads_and_clamps():
    d = np.array([[3, 3, 1, 5], [2, 2, 9, 9], [1, 1, 1, 1]])
    got = ref.duration_scale(d, token_lengths=[4, 2, 0], speed=2.0)
    assert got["durations"].tolist() == [[2, 1, 1, 2], [1, 1, 0, 0], [0, 0, 0, 0]]
    assert got["starts"].tolist() == [[0, 2, 3, 4], [0, 1, -1, -1], [-1] * 4]
    assert got["out_lengths"].tolist() == [6, 2, 0] and got["status"].tolist() == [ref.OK, ref.OK, ref.EMPTY]
    assert ref.duration_scale(d, token_lengths=[9, -3, 1], speed=1.0)["out_lengths"].tolist() == [12, 0, 1]


# ---- the map's restatement --------------------------------------------------------------------------------------------------------

def test_frame_map_by_hand():
    # 2 -> 4 frames: centres 0.25, 0.75, 1.25, 1.75 of the source token minus half a frame: -0.25, 0.25, 0.75, 1.25
    got = [ref.frame_map([2], [4], u) for u in range(4)]
    assert got == [(0, 0.0), (0, 0.25), (0, 0.75), (1, 0.0)]                         # clamped at both ends, frac 0 there
    # 4 -> 2 frames: centres 1.0 and 3.0, minus half a frame: 0.5 and 2.5
    assert [ref.frame_map([4], [2], u) for u in range(2)] == [(0, 0.5), (2, 0.5)]
    # the second token starts at source frame 3; stretched, its first frame leans back over the boundary
    assert ref.frame_map([3, 2], [3, 4], 3) == (2, 0.75) and ref.frame_map([3, 2], [3, 4], 4) == (3, 0.25)
    # identity
    d = [3, 0, 2, 1]
    assert [ref.frame_map(d, d, u) for u in range(6)] == [(u, 0.0) for u in range(6)]
    with pytest.raises(ValueError):
        ref.frame_map([2], [4], 4)


def test_warp_restatement_identity_poison_and_status():
    rng = np.random.default_rng(0)
    mel = rng.standard_normal((2, 5, 12)).astype(np.float32)
    mel[:, :, 9:] = np.nan
    d = np.array([[4, 0, 5, 7], [2, 3, 4, 7]])
    got = ref.mel_time_warp(mel, d, d, token_lengths=[3, 3], T_out=10)
    assert got["status"].tolist() == [ref.OK, ref.OK]
    assert np.array_equal(got["mel"][:, :, :9], mel[:, :, :9].astype(np.float64)) and (got["mel"][:, :, 9:] == 0).all()
    assert got["src_frame"][0].tolist() == list(range(9)) + [-1]
    dp = np.array([[8, 0, 3, 7], [1, 6, 9, 7]])
    got = ref.mel_time_warp(mel, d, dp, token_lengths=[3, 3], T_out=12)
    assert got["status"].tolist() == [ref.OK, ref.CUT] and np.isfinite(got["mel"]).all()          # nothing at or behind T_b = 9 is used
    assert (got["src_frame"][0, :11] >= 0).all() and got["src_frame"][0, 11] == -1 and (got["src_frame"][1] >= 0).all()
    assert ref.warp_status([1, 0], [1, 1], 9, 9) == (ref.BAD, 0) and ref.warp_status([1, 1], [1, 0], 9, 9) == (ref.BAD, 0)
    assert ref.warp_status([5, 5], [1, 1], 9, 9) == (ref.BAD, 0) and ref.warp_status([-1, 5], [1, 1], 9, 9) == (ref.BAD, 0)
    assert ref.warp_status([], [], 9, 9) == (ref.EMPTY, 0) and ref.warp_status([0, 0], [0, 0], 9, 9) == (ref.EMPTY, 0)
    b = ref.interp_bound(np.float32(1.0), np.float32(3.0), np.float32(0.5))
    assert b == 0.5 * 2.0 ** -22 + 0.5 * 2.0 ** -22 and ref.interp_bound(1.0, 3.0, 0.0) == 0.0     # ulp(2) = 2^-22


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

CTYPE_OF = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}


def _declared(name):
    """(restype, argtypes) of `name` as include/genvox_amd.h declares it: every pointer is a c_void_p, as _lib.py binds them."""
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header, re.M)
    assert m, f"{name} is not declared"
    args = []
    for arg in m.group(2).split(","):
        arg = " ".join(arg.split())
        args.append(C.c_void_p if "*" in arg else CTYPE_OF[arg.replace("const ", "").split(" ")[0]])
    return CTYPE_OF[m.group(1)], args


@pytest.mark.parametrize("name,n_args", [("gvx_duration_scale", 11), ("gvx_mel_time_warp", 14)])
def test_symbols_are_exported_and_bound_as_declared(name, n_args):
    lib = _lib.load()
    assert hasattr(lib, name)
    res, args = _declared(name)
    assert len(args) == n_args
    assert _lib.SIGNATURES[name] == (res, args)
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    assert header.index("gvx_monotonic_align(") < header.index(name + "(") < header.index("gvx_kernel_timing_enable(")
    assert re.search(r"GVX_WARP_OK = 0, GVX_WARP_EMPTY = 1, GVX_WARP_BAD = 2, GVX_WARP_CUT = 3", header)
    assert f"GVX_WARP_TILE_FRAMES = {ref.TILE}" in header
    from genvox_amd import build, metrics
    assert "time_warp.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "time_warp.hip"))
    assert metrics.WARP_STATUS_NAMES == ("ok", "empty", "bad", "cut")
    assert [metrics.WARP_STATUS_NAMES[i] for i in (ref.OK, ref.EMPTY, ref.BAD, ref.CUT)] == ["ok", "empty", "bad", "cut"]


OK, INVALID, UNSUPPORTED = 0, -1, -2
X = 256   # a non-null address that is never dereferenced: every call below fails before its launch


def test_duration_scale_checks_its_arguments_before_any_launch():
    lib = _lib.load()

    def err():
        return lib.gvx_last_error().decode()

    def call(d=X, tl=None, rates=None, B=2, L=8, speed=1.0, td=X, ts=X, out_len=X, status=X):
        return lib.gvx_duration_scale(d, tl, rates, B, L, speed, td, ts, out_len, status, None)

    for kw in (dict(d=None), dict(td=None), dict(out_len=None), dict(status=None)):
        assert call(**kw) == INVALID and "null" in err()
    for B, L in ((0, 8), (2, 0), (-1, 8), (2, -5)):
        assert call(B=B, L=L) == INVALID
    assert call(L=4097) == UNSUPPORTED and "4097" in err()
    assert call(L=4097, d=None) == UNSUPPORTED                      # the shape is looked at first, as gvx_monotonic_align does
    for speed in (0.0, -1.0, 0.1249, 8.001, float("nan"), float("inf"), -float("inf")):
        assert call(speed=speed) == INVALID and "speed" in err()


def test_mel_time_warp_checks_its_arguments_before_any_launch():
    lib = _lib.load()

    def err():
        return lib.gvx_last_error().decode()

    def call(mel=X, d=X, dp=X, tl=None, B=2, M=80, T=100, L=8, T_out=120, out=X, fr=None, fc=None, status=X):
        return lib.gvx_mel_time_warp(mel, d, dp, tl, B, M, T, L, T_out, out, fr, fc, status, None)

    for kw in (dict(mel=None), dict(d=None), dict(dp=None), dict(out=None), dict(status=None)):
        assert call(**kw) == INVALID and "null" in err()
    for kw in (dict(B=0), dict(M=0), dict(T=0), dict(L=0), dict(T_out=0), dict(B=-2), dict(T_out=-1)):
        assert call(**kw) == INVALID
    assert call(L=4097) == UNSUPPORTED and "4097" in err()
    assert call(T=32769) == UNSUPPORTED and "32769" in err()
    assert call(T_out=32769) == UNSUPPORTED and "32769" in err()
    assert call(T_out=32769, mel=None) == UNSUPPORTED
    assert math.isfinite(ref.RATE_MIN) and (ref.MAX_FRAMES, ref.MAX_TOKENS) == (32768, 4096)
