"""Token and word timings without a GPU: the numpy restatements of the monotonic alignment search (tests/mas_ref.py) against a
brute force over every monotone path and against cases done by hand, the grouping of tokens into words, the sample arithmetic of
the timings, and the argument checks of the three C-ABI entries (nothing is launched)."""
import math

import numpy as np
import pytest

from genvox_amd import _lib
from genvox_amd.audio import AudioProcessor
from genvox_amd.resample import resample_ratio, resampled_length
from genvox_amd.synthesizer import group_words, token_times
from tests import mas_ref as ref


# ---- the recurrence -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,L", [(T, L) for T in range(1, 8) for L in range(1, T + 1)])
def test_recurrence_equals_brute_force_over_all_monotone_paths(T, L):
    rng = np.random.default_rng(100 * T + L)
    for trial in range(4):
        s = np.log(rng.uniform(1e-4, 1.0, (T, L))).astype(np.float32)
        if trial == 3:
            s = np.round(s)   # small integers: ties between paths, every sum exact
        got = ref.align_f32(s[None])
        best, paths = ref.brute_force(s)
        assert got["status"][0] == ref.OK
        assert got["score"][0].tobytes() == np.float32(best).tobytes()        # rounding is monotone: max of sums == sum of maxes
        assert any(np.array_equal(got["path"][0], p) for p in paths)
        p = got["path"][0]
        assert p[0] == 0 and p[-1] == L - 1 and set(np.diff(p).tolist()) <= {0, 1}
        assert got["durations"][0].sum() == T and got["durations"][0].min() >= 1
        assert np.array_equal(got["starts"][0], np.concatenate([[0], np.cumsum(got["durations"][0])[:-1]]))
        g64 = ref.align_f64(np.exp(s.astype(np.float64))[None].astype(np.float32), 1e-8)
        assert g64["status"][0] == ref.OK and abs(g64["score"][0] - float(best)) <= 1e-4 * T


def test_four_by_three_by_hand_with_a_tie_resolved_by_stay():
    s = np.array([[-1.0, -9.0, -9.0],
                  [-1.0, -1.0, -9.0],
                  [-2.0, -1.0, -3.0],
                  [-9.0, -5.0, -1.0]], np.float32)
    # Q[0] = [ -1, -inf, -inf]
    # Q[1] = [ -2,   -2, -inf]    (1,1): only the advance from (0,0) exists: -1 + -1
    # Q[2] = [ -4,   -3,   -5]    (2,1): stay -2 == advance -2, a TIE: stays.  (2,2): advance from (1,1): -3 + -2
    # Q[3] = [-13,   -8,   -4]    (3,2): advance -3 beats stay -5: -1 + -3
    # back from (3,2): advanced at 3 -> (2,1) stayed -> (1,1) advanced at 1 -> (0,0)
    got = ref.align_f32(s[None])
    assert got["score"][0] == -4.0
    assert got["path"][0].tolist() == [0, 1, 1, 2]            # "advance wins" at (2,1) would give [0, 0, 1, 2], also -4
    assert got["durations"][0].tolist() == [1, 2, 1] and got["starts"][0].tolist() == [0, 1, 3]
    best, paths = ref.brute_force(s)
    assert best == -4.0 and sorted(p.tolist() for p in paths) == [[0, 0, 1, 2], [0, 1, 1, 2]]
    # a tie: both ways into (2, 1) cost the same; "stay" must win, so token 1 starts at frame 1, not 2
    tie = np.array([[-1.0, -9.0],
                    [-1.0, -1.0],     # Q[1] = [-2, -2]
                    [-9.0, -1.0]], np.float32)   # (2,1): stay -2 == advance -2
    got = ref.align_f32(tie[None])
    assert got["score"][0] == -3.0 and got["path"][0].tolist() == [0, 1, 1] and got["starts"][0].tolist() == [0, 1]
    best, paths = ref.brute_force(tie)
    assert best == -3.0 and len(paths) == 2       # the other best path, [0, 0, 1], is the one "advance wins" would give
    # uniform rows: every cell a tie.  Read back from the end, the path stays on the last token while it can, so every advance
    # happens at the first frame that allows it
    got = ref.align_f32(np.zeros((1, 5, 3), np.float32))
    assert got["path"][0].tolist() == [0, 1, 2, 2, 2] and got["durations"][0].tolist() == [1, 1, 3]


def test_infeasible_and_empty_rows_by_hand():
    s = np.zeros((4, 3, 4), np.float32)
    got = ref.align_f32(s, mel_lengths=[3, 3, 0, 2], token_lengths=[4, 3, 2, 0])
    assert got["status"].tolist() == [ref.INFEASIBLE, ref.OK, ref.EMPTY, ref.EMPTY]
    for b in (0, 2, 3):
        assert got["path"][b].tolist() == [-1] * 3 and got["durations"][b].tolist() == [0] * 4
        assert got["starts"][b].tolist() == [-1] * 4 and math.isnan(got["score"][b])
    assert got["path"][1].tolist() == [0, 1, 2] and got["durations"][1].tolist() == [1, 1, 1, 0] and got["starts"][1].tolist() == [0, 1, 2, -1]
    got = ref.align_f64(np.full((2, 3, 4), 0.25, np.float32), 1e-8, mel_lengths=[9, -1], token_lengths=[2, 2])   # lengths are clamped
    assert got["status"].tolist() == [ref.OK, ref.EMPTY] and got["path"][0].tolist() == [0, 1, 1]   # uniform: a tie stays
    assert got["score"][0] == 3 * math.log(0.25)


def test_scores_floor_zeros_and_nan():
    a = np.array([[[0.0, 0.5], [np.nan, 1e-12]]], np.float32)
    s = ref.scores_f64(a[0], np.float64(np.float32(1e-8)))
    lo = math.log(float(np.float32(1e-8)))
    assert s[0, 0] == lo and s[1, 0] == lo and s[1, 1] == lo and s[0, 1] == math.log(0.5)
    assert np.isfinite(ref.align_f64(a, 1e-8)["score"][0])


# ---- words ----------------------------------------------------------------------------------------------------------------------

def _tokens(text):
    toks = list(text)
    starts = [float(i) for i in range(len(toks))]
    return toks, starts, [v + 1.0 for v in starts]


def test_group_words_plain_sentence_and_punctuation():
    toks, st, en = _tokens("hello, world.")
    assert group_words(toks, st, en) == [("hello,", 0.0, 6.0), ("world.", 7.0, 13.0)]
    assert " ".join(w for w, _, _ in group_words(toks, st, en)) == "hello, world."


def test_group_words_leading_trailing_and_double_spaces():
    toks, st, en = _tokens("  a  bc ")
    assert group_words(toks, st, en) == [("a", 2.0, 3.0), ("bc", 5.0, 7.0)]
    assert group_words(*_tokens("   ")) == [] and group_words([], [], []) == []
    assert group_words(*_tokens("x")) == [("x", 0.0, 1.0)]
    words = group_words(*_tokens(" one two,  three! "))
    assert [w for w, _, _ in words] == ["one", "two,", "three!"]
    assert " ".join(w for w, _, _ in words) == " ".join(" one two,  three! ".split())
    with pytest.raises(ValueError):
        group_words(["a", "b"], [0.0], [1.0, 2.0])


# ---- sample arithmetic ----------------------------------------------------------------------------------------------------------

HOP, NFFT, RATE, TRIM = 256, 1024, 22050, AudioProcessor.TRIM


def test_token_times_trim_clamp_and_last_end():
    T = 10
    n = NFFT + (T - 1) * HOP - 2 * TRIM          # the delivered model-rate waveform: 2328 samples
    starts, ends = token_times([0, 1, 2, 7, 9], HOP, TRIM, n, RATE, n / RATE)
    assert TRIM == 500
    assert starts[0] == 0.0 and starts[1] == 0.0                 # frames 0 and 1 begin inside the 500 trimmed samples: clamped to 0
    assert starts[2] == (2 * HOP - TRIM) / RATE == 12 / RATE
    assert starts[3] == (7 * HOP - TRIM) / RATE
    assert starts[4] == (9 * HOP - TRIM) / RATE and 9 * HOP - TRIM < n
    assert ends == starts[1:] + [n / RATE]                          # a token ends where the next starts, the last at the end
    late, _ = token_times([0, 12], HOP, TRIM, n, RATE, n / RATE)    # a frame that begins behind the trimmed end: clamped to n
    assert late[1] == n / RATE
    assert all(a <= b for a, b in zip(starts, ends))


def test_token_times_hold_at_a_foreign_sampling_rate():
    T = 40
    n = NFFT + (T - 1) * HOP - 2 * TRIM
    up, down = resample_ratio(RATE, 16000)
    n16 = resampled_length(n, up, down)
    frames = [0, 3, 11, 30]
    own, own_ends = token_times(frames, HOP, TRIM, n, RATE, n / RATE)
    other, other_ends = token_times(frames, HOP, TRIM, n, RATE, n16 / 16000)
    assert own == other                                             # seconds do not depend on the rate delivered
    assert other_ends[:-1] == own_ends[:-1] and other_ends[-1] == n16 / 16000
    assert 0 <= other_ends[-1] - own_ends[-1] < 1 / 16000           # the resampled row is rounded up to a whole sample
    assert other_ends[-1] >= other[-1]


# ---- argument checks of the C ABI (nothing is launched) -------------------------------------------------------------------------

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -5
X = 256   # a non-null, 256-byte aligned address that is never dereferenced: every call below fails before its launch


def test_mas_plan_queries():
    lib = _lib.load()
    assert lib.gvx_monotonic_align_uses_lds(2000, 256) == 1 and lib.gvx_monotonic_align_workspace_bytes(32, 2000, 256) == 0
    assert lib.gvx_monotonic_align_uses_lds(800, 128) == 1 and lib.gvx_monotonic_align_uses_lds(1, 1) == 1
    assert 8 * 256 + 8 * 2000 * 4 <= 160 * 1024
    # 8 L + 8 T ceil(L / 64) bytes against 160 KiB = 163840
    assert lib.gvx_monotonic_align_uses_lds(2000, 1000) == 0
    assert lib.gvx_monotonic_align_workspace_bytes(32, 2000, 1000) == 32 * 2000 * 16 * 8
    assert lib.gvx_monotonic_align_workspace_bytes(1, 2001, 1000) == (2001 * 16 * 8 + 255) // 256 * 256
    assert lib.gvx_monotonic_align_uses_lds(20416, 64) == 1 and lib.gvx_monotonic_align_uses_lds(20417, 64) == 0   # 512 + 8 T <= 163840
    assert lib.gvx_monotonic_align_uses_lds(32768, 4096) == 0
    assert lib.gvx_monotonic_align_workspace_bytes(2, 32768, 4096) == 2 * 32768 * 64 * 8
    for bad in ((0, 5), (5, 0), (32769, 5), (5, 4097), (-1, 5)):
        assert lib.gvx_monotonic_align_uses_lds(*bad) == -1 and lib.gvx_monotonic_align_workspace_bytes(1, *bad) == 0
    assert lib.gvx_monotonic_align_workspace_bytes(0, 2000, 1000) == 0


def test_monotonic_align_checks_its_arguments_before_any_launch():
    lib = _lib.load()

    def err():
        return lib.gvx_last_error().decode()

    def call(a=X, B=1, T=8, L=4, floor=1e-8, path=X, dur=X, starts=X, score=X, status=X, scores=None, ws=None, ws_bytes=0):
        return lib.gvx_monotonic_align(a, None, None, B, T, L, floor, path, dur, starts, score, status, scores, ws, ws_bytes, None)

    assert call(a=None) == INVALID and "null" in err()
    assert call(dur=None) == INVALID and call(status=None) == INVALID
    for B, T, L in ((0, 8, 4), (1, 0, 4), (1, 8, 0)):
        assert call(B=B, T=T, L=L) == INVALID
    assert call(T=40000) == UNSUPPORTED and "40000" in err()
    assert call(L=4097) == UNSUPPORTED and "4097" in err()
    assert call(T=40000, a=None) == UNSUPPORTED           # the shape is looked at first, as gvx_dtw_distance does
    for floor in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        assert call(floor=floor) == INVALID and "floor" in err()
    need = lib.gvx_monotonic_align_workspace_bytes(2, 2000, 1000)
    assert need > 0
    big = dict(B=2, T=2000, L=1000)
    assert call(**big) == WORKSPACE                                                  # missing
    assert call(**big, ws=X + 64, ws_bytes=need) == WORKSPACE                        # misaligned
    assert call(**big, ws=X, ws_bytes=need - 1) == WORKSPACE and "too small" in err()   # one byte short
