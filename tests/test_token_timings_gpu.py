"""GPU: the monotonic alignment search (gvx_monotonic_align) and the timings built on it.

Exact half.  With scores_out requested, path, durations, starts, status and the BITS of score equal tests/mas_ref.align_f32 run on the
device's own score table: fp32 addition is correctly rounded on both sides, max is exact, the library is built with
-ffp-contract=off, so there is no tolerance.

Score half.  scores_out against log(max(a, floor)) in float64.  Documented accuracy of logf: 1 ulp (HIP math API reference, table of
single-precision functions; OCML computes it by the same routine).  Tolerance: 2 ulp of the score - the documented figure times
two for the rounding of the comparison itself (the float64 reference rounded to the fp32 grid).  Largest error observed on the
MI355X over every case of this file: 1.877 ulp (EXPERIMENTS.md, "Monotonic alignment search"; the test prints it).  score against
align_f64's score: a path of T_b frames carries T_b scores (each within SCORE_ULPS ulp of at most |log floor|) and T_b - 1 adds
(each within half an ulp of a partial sum of at most T_b |log floor|); rounding is monotone, so the maximum over paths moves by
no more than one path does.
"""
import math
import os

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from tests import mas_ref as ref

pytestmark = pytest.mark.gpu

FLOOR = 1e-8
LOGF_ULPS = 1.0            # documented
SCORE_ULPS = 2 * LOGF_ULPS
LDS_BYTES = 160 * 1024
ERR_WORKSPACE = -5
GUARD = 4096
SENT = 0x5A


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _uses_lds(T, L):
    return 8 * L + 8 * T * ((L + 63) // 64) <= LDS_BYTES


# ---- alignments ---------------------------------------------------------------------------------------------------------------

def _monotone_centres(rng, T, L):
    """A random monotone path of T frames over L tokens (T >= L): 0 at frame 0, L - 1 at the end, steps of 0 or 1."""
    ups = np.sort(rng.choice(np.arange(1, T), size=L - 1, replace=False)) if L > 1 else np.array([], int)
    c = np.zeros(T, int)
    for t in ups:
        c[t:] += 1
    return c


def make_alignment(kind, rng, T, L):
    """fp32 [T, L].  softmax: rows of a softmax around a random monotone path plus noise; windowed: the same, exact zeros outside
    a window of (1 back, 3 ahead) tokens around the path and renormalised; uniform: every cell 1 / L (every comparison a tie)."""
    if kind == "uniform":
        return np.full((T, L), np.float32(1.0 / L), np.float32)
    c = _monotone_centres(rng, max(T, L), L)[:T] if T >= L else np.minimum(np.arange(T), L - 1)
    l = np.arange(L)[None, :]
    logits = -0.5 * ((l - c[:, None]) / 1.5) ** 2 + 0.8 * rng.standard_normal((T, L))
    a = np.exp(logits - logits.max(axis=1, keepdims=True))
    if kind == "windowed":
        a = np.where((l >= c[:, None] - 1) & (l <= c[:, None] + 3), a, 0.0)
    a = a / a.sum(axis=1, keepdims=True)
    return a.astype(np.float32)


KINDS = ("softmax", "windowed", "uniform")


def make_batch(seed, B, T, L):
    rng = np.random.default_rng(seed)
    return np.stack([make_alignment(KINDS[b % 3], rng, T, L) for b in range(B)])


# ---- the call -----------------------------------------------------------------------------------------------------------------

class Outs:
    """Every output of one call, each in its own sentinel-filled allocation."""

    def __init__(self, B, T, L, want_scores):
        dev = "cuda"
        self.path = torch.full((B, T), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        self.durations = torch.full((B, L), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        self.starts = torch.full((B, L), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        self.score = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32)
        self.status = torch.full((B,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        self.scores = torch.full((B, T, L), 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32) if want_scores else None

    def named(self):
        d = {"path": self.path, "durations": self.durations, "starts": self.starts, "score": self.score, "status": self.status}
        if self.scores is not None:
            d["scores"] = self.scores
        return d

    def untouched(self):
        return all(bool((t.view(torch.int32) == 0x5A5A5A5A).all()) for t in self.named().values())


def call(a, ml=None, tl=None, floor=FLOOR, want_scores=True, ws=None, ws_bytes=None, expect=0):
    """One gvx_monotonic_align on the device tensor a [B, T, L]; ws: a uint8 tensor to use as the workspace (default: a fresh one of
    the size the query gives)."""
    lib = _lib.load()
    B, T, L = a.shape
    o = Outs(B, T, L, want_scores)
    need = lib.gvx_monotonic_align_workspace_bytes(B, T, L)
    assert (need == 0) == _uses_lds(T, L) and lib.gvx_monotonic_align_uses_lds(T, L) == int(_uses_lds(T, L))
    if ws is None and need:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.gvx_monotonic_align(a.data_ptr(), ml.data_ptr() if ml is not None else None, tl.data_ptr() if tl is not None else None, B, T, L,
                                 floor, o.path.data_ptr(), o.durations.data_ptr(), o.starts.data_ptr(), o.score.data_ptr(), o.status.data_ptr(),
                                 o.scores.data_ptr() if want_scores else None, ws.data_ptr() if ws is not None else None,
                                 (ws.numel() if ws is not None else 0) if ws_bytes is None else ws_bytes, _stream())
    assert rc == expect, (rc, lib.gvx_last_error())
    torch.cuda.synchronize()
    return o


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(x, y, what, keys=("path", "durations", "starts", "score", "status")):
    for k in keys:
        assert torch.equal(_bits(x.named()[k]), _bits(y.named()[k])), f"{what}: {k} differs"


def lengths_dev(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device="cuda")


def check_exact(o, ml, tl, what):
    """The device's outputs against align_f32 on the device's own score table: no tolerance."""
    want = ref.align_f32(o.scores.cpu().numpy(), ml, tl)
    for k in ("path", "durations", "starts", "status"):
        got = o.named()[k].cpu().numpy()
        assert np.array_equal(got, want[k]), f"{what}: {k} differs in {int((got != want[k]).sum())} places"
    got = o.score.cpu().numpy()
    assert got.view(np.int32).tolist() == want["score"].view(np.int32).tolist() or all(
        (math.isnan(g) and math.isnan(w)) or g.tobytes() == w.tobytes() for g, w in zip(got, want["score"])), f"{what}: score bits"
    return want


_WORST = {"ulp": 0.0}


def check_scores(o, a_host, ml, tl, floor, what):
    """scores_out against float64 inside every row's lengths, untouched (sentinel) outside; score against align_f64."""
    B, T, L = a_host.shape
    got = o.scores.cpu().numpy()
    raw = got.view(np.int32)
    f32_floor = np.float64(np.float32(floor))
    smax = abs(math.log(f32_floor))
    want64 = ref.align_f64(a_host, floor, ml, tl)
    for b in range(B):
        Tb = T if ml is None else max(0, min(ml[b], T))
        Lb = L if tl is None else max(0, min(tl[b], L))
        if Tb < Lb or Tb == 0 or Lb == 0:
            assert (raw[b] == 0x5A5A5A5A).all(), f"{what}: scores_out of a row without a path was written"
            continue
        assert (raw[b, Tb:] == 0x5A5A5A5A).all() and (raw[b, :, Lb:] == 0x5A5A5A5A).all(), f"{what}: scores_out written behind row {b}'s lengths"
        w = ref.scores_f64(a_host[b, :Tb, :Lb], f32_floor)
        g = got[b, :Tb, :Lb].astype(np.float64)
        ulp = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
        err = np.abs(g - w) / ulp
        _WORST["ulp"] = max(_WORST["ulp"], float(err.max()))
        assert err.max() <= SCORE_ULPS, f"{what}: row {b}: a score is {err.max():.3f} ulp from float64 (bound {SCORE_ULPS})"
        bound = Tb * SCORE_ULPS * 2.0 ** -23 * smax + (Tb - 1) * 2.0 ** -24 * Tb * smax
        d = abs(float(o.score[b].item()) - want64["score"][b])
        assert d <= bound, f"{what}: row {b}: score {d:.3e} from the float64 optimum (bound {bound:.3e})"
    print(f"[mas] {what}: largest score error so far {_WORST['ulp']:.3f} ulp (documented {LOGF_ULPS}, bound {SCORE_ULPS})")


# ---- exact half: every shape --------------------------------------------------------------------------------------------------

LS = (1, 2, 63, 64, 65, 127, 128, 129, 256, 1000)
SHAPES = sorted({(T, L) for L in LS for T in (L, L + 1, 800, 2000) if T >= L} | {(T, L) for T in (1, 2) for L in (1, 2)})


def test_the_shapes_cover_both_plans():
    assert any(_uses_lds(T, L) for T, L in SHAPES) and any(not _uses_lds(T, L) for T, L in SHAPES)
    assert _uses_lds(2000, 256) and _uses_lds(1000, 1000) and not _uses_lds(2000, 1000)


@pytest.mark.parametrize("T,L", SHAPES)
def test_exact_against_the_f32_restatement(T, L):
    a_host = make_batch(1000 * T + L, 3, T, L)           # one row of each kind
    a = torch.from_numpy(a_host).cuda()
    o = call(a)
    lib = _lib.load()
    assert lib.gvx_monotonic_align_uses_lds(T, L) == int(_uses_lds(T, L))
    what = f"{T}x{L} ({'LDS' if _uses_lds(T, L) else 'workspace'} plan)"
    want = check_exact(o, None, None, what)
    if T >= L:
        assert want["status"].tolist() == [ref.OK] * 3
        p = o.path.cpu().numpy()
        assert (p[:, 0] == 0).all() and (p[:, -1] == L - 1).all() and set(np.unique(np.diff(p, axis=1)).tolist()) <= {0, 1}
        d = o.durations.cpu().numpy()
        assert (d >= 1).all() and (d.sum(axis=1) == T).all()
        if T == L:
            assert (p == np.arange(T)[None]).all()        # every step advances
    else:
        assert want["status"].tolist() == [ref.INFEASIBLE] * 3
    check_scores(o, a_host, None, None, FLOOR, what)
    same_bits(o, call(a, want_scores=False), what + ": without scores_out")
    same_bits(o, call(a), what + ": second call", keys=("path", "durations", "starts", "score", "status", "scores"))


def test_uniform_rows_pin_the_tie_rule():
    """Every cell a tie: the path, read back from the end, stays on the last token while it can - token l starts at frame l."""
    T, L = 50, 7
    a = torch.full((1, T, L), 1.0 / L, device="cuda")
    o = call(a)
    assert o.starts[0].tolist() == list(range(L)) and o.durations[0].tolist() == [1] * (L - 1) + [T - L + 1]
    check_exact(o, None, None, "uniform")


# ---- ragged batches -----------------------------------------------------------------------------------------------------------

def _ragged_lengths(seed, B, T, L):
    rng = np.random.default_rng(seed)
    ml = rng.integers(L // 2, T + 1, B).tolist()
    tl = rng.integers(1, L + 1, B).tolist()
    ml[1], tl[2] = 0, 0                      # EMPTY both ways
    ml[3], tl[3] = L // 2, L                 # INFEASIBLE
    ml[4], tl[4] = T + 9, L + 9              # clamped to the full row
    ml[5], tl[5] = -3, 4                     # clamped to 0: EMPTY
    ml[6], tl[6] = 5, 5                      # every step advances
    ml[7], tl[7] = T, 1                      # one token takes every frame
    return ml, tl


@pytest.mark.parametrize("T,L", [(300, 100), (2000, 700)])
def test_ragged_batch_of_32_with_empty_and_infeasible_rows(T, L):
    B = 32
    a_host = make_batch(7 * T + L, B, T, L)
    ml, tl = _ragged_lengths(T + L, B, T, L)
    a = torch.from_numpy(a_host).cuda()
    o = call(a, lengths_dev(ml), lengths_dev(tl))
    what = f"ragged {T}x{L}"
    want = check_exact(o, ml, tl, what)
    st = want["status"].tolist()
    assert st[1] == st[2] == st[5] == ref.EMPTY and st[3] == ref.INFEASIBLE and st[4] == st[6] == st[7] == ref.OK
    assert ref.OK in st and st.count(ref.INFEASIBLE) >= 1
    for b in range(B):
        Tb, Lb = max(0, min(ml[b], T)), max(0, min(tl[b], L))
        if st[b] != ref.OK:
            assert (o.path[b] == -1).all() and (o.durations[b] == 0).all() and (o.starts[b] == -1).all() and math.isnan(o.score[b].item())
        else:
            assert (o.path[b, Tb:] == -1).all() and (o.durations[b, Lb:] == 0).all() and (o.starts[b, Lb:] == -1).all()
            assert int(o.durations[b].sum()) == Tb and int(o.durations[b, :Lb].min()) >= 1
    check_scores(o, a_host, ml, tl, FLOOR, what)
    # poison behind every row's lengths (and all over the rows without a path) changes no output bit
    poisoned = a_host.copy()
    for b in range(B):
        Tb, Lb = max(0, min(ml[b], T)), max(0, min(tl[b], L))
        if st[b] != ref.OK:
            poisoned[b] = np.nan
        else:
            poisoned[b, Tb:] = np.nan
            poisoned[b, :, Lb:] = np.inf if b % 2 else np.nan
    o2 = call(torch.from_numpy(poisoned).cuda(), lengths_dev(ml), lengths_dev(tl))
    same_bits(o, o2, what + ": poison behind the lengths", keys=("path", "durations", "starts", "score", "status", "scores"))
    # NULL outputs: the mandatory ones have the same bits
    lib = _lib.load()
    dur = torch.empty(B, L, dtype=torch.int32, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    need = lib.gvx_monotonic_align_workspace_bytes(B, T, L)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    ml_dev, tl_dev = lengths_dev(ml), lengths_dev(tl)
    _lib.check(lib.gvx_monotonic_align(a.data_ptr(), ml_dev.data_ptr(), tl_dev.data_ptr(), B, T, L, FLOOR, None, dur.data_ptr(),
                                       None, None, status.data_ptr(), None, ws.data_ptr() if need else None, need, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(dur, o.durations) and torch.equal(status, o.status)


def test_a_nan_inside_a_row_scores_log_floor_and_other_floors():
    T, L = 40, 9
    a_host = make_batch(5, 2, T, L)
    a_host[0, 7, 3] = np.nan
    a_host[0, 8, 4] = 0.0
    a_host[1, 3, 2] = np.inf
    for floor in (1e-8, 1e-4, 1.0):
        o = call(torch.from_numpy(a_host).cuda(), floor=floor)
        s = o.scores.cpu().numpy()
        assert s[0, 7, 3].tobytes() == s[0, 8, 4].tobytes() and np.isfinite(s[0, 7, 3])       # NaN scores what an exact zero scores
        assert abs(float(s[0, 7, 3]) - math.log(float(np.float32(floor)))) <= SCORE_ULPS * float(np.spacing(np.float32(abs(math.log(float(np.float32(floor)))))))
        assert np.isfinite(s[0]).all() and s[1, 3, 2] == np.inf
        check_exact(o, None, None, f"floor {floor}")
        if floor == 1.0:
            assert (s[0] == 0.0).all()                       # every weight <= 1 is lifted to 1: every cell a tie
            assert o.starts[0].tolist() == list(range(L))


def test_the_python_wrapper_returns_the_same_and_keeps_its_workspace():
    T, L = 2000, 700
    a = torch.from_numpy(make_batch(11, 2, T, L)).cuda()
    o = call(a)
    got = metrics.monotonic_align(a, want_scores=True)
    assert set(got) == {"path", "durations", "starts", "score", "status", "scores"}
    for k, v in o.named().items():
        assert torch.equal(_bits(v), _bits(got[k])), k
    ws = metrics._mas_ws[str(a.device)]
    again = metrics.monotonic_align(a[:1].contiguous())
    assert metrics._mas_ws[str(a.device)] is ws and "scores" not in again            # a smaller call reuses the buffer
    assert torch.equal(again["durations"], o.durations[:1])
    with pytest.raises(RuntimeError):
        metrics.monotonic_align(a.cpu())
    with pytest.raises(_lib.GvxError):
        metrics.monotonic_align(a, floor=0.0)


# ---- the workspace contract -------------------------------------------------------------------------------------------------------

class Arena:
    """[guard | n bytes | guard] in one allocation, the middle 256-byte aligned and exactly n bytes."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), SENT, dtype=torch.uint8, device="cuda")
        assert (self.buf.data_ptr() + GUARD) % 256 == 0

    def view(self):
        return self.buf[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())


@pytest.mark.parametrize("T,L,B", [(2000, 1000, 3), (2001, 1333, 5), (4100, 4096, 1)])
def test_workspace_dirty_exact_and_one_byte_short(T, L, B):
    lib = _lib.load()
    need = lib.gvx_monotonic_align_workspace_bytes(B, T, L)
    assert need > 0 and not _uses_lds(T, L)
    a_host = make_batch(3 * T + L, B, T, L)
    ml, tl = [T, T - 7, T // 2][:B] + [T] * (B - 3), [L, L - 1, L // 3][:B] + [L] * (B - 3)
    a = torch.from_numpy(a_host).cuda()
    clean = Arena(need)
    clean.view().zero_()
    o = call(a, lengths_dev(ml), lengths_dev(tl), ws=clean.view())
    assert clean.intact(), "the call wrote outside its workspace"
    check_exact(o, ml, tl, f"workspace {T}x{L}")
    dirty = Arena(need)
    dirty.view()[:need // 4 * 4].view(torch.int32).fill_(0x7FF8BEEF)                  # NaN words
    dirty.view()[need // 4 * 4:] = 0x7F
    o2 = call(a, lengths_dev(ml), lengths_dev(tl), ws=dirty.view())
    assert dirty.intact(), "the call wrote outside its dirty workspace"
    same_bits(o, o2, "NaN-filled workspace", keys=("path", "durations", "starts", "score", "status", "scores"))
    before = dirty.view().clone()
    o3 = call(a, lengths_dev(ml), lengths_dev(tl), ws=dirty.view(), ws_bytes=need - 1, expect=ERR_WORKSPACE)
    assert o3.untouched() and dirty.intact() and torch.equal(dirty.view(), before), "a refused call wrote something"
    assert b"too small" in lib.gvx_last_error()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OLD_KEYS = {"mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments", "waveform", "sampling_rate"}


@pytest.fixture(scope="module")
def syn():
    from genvox_amd.synthesizer import Synthesizer
    from genvox_amd.tacotron2 import Tacotron2

    exp = os.path.join(GOLDEN, "ref_exp")
    return Synthesizer(tts_model_class=Tacotron2, tts_config_path=os.path.join(exp, "config.yaml"),
                       tts_checkpoint_path=os.path.join(exp, "checkpoint_3.pt"), use_cuda=True)


def _check_timings(syn, text, res):
    """The timing keys of one sentence's result, whichever branch its frame and token counts dictate."""
    toks = syn.text_processor.tokenize(text)
    T = res["mel_outputs_postnet"].shape[1]
    assert {"token_timings", "word_timings", "timings_status"} <= set(res)
    if T < len(toks):
        assert res["timings_status"] == "infeasible" and res["token_timings"] == [] and res["word_timings"] == []
        return "infeasible"
    assert res["timings_status"] == "ok"
    tt = res["token_timings"]
    assert [t for t, _, _ in tt] == toks                                         # one entry per token, in order
    starts, ends = [s for _, s, _ in tt], [e for _, _, e in tt]
    assert starts[0] == 0.0 and all(a <= b for a, b in zip(starts, starts[1:]))
    assert ends[:-1] == starts[1:]
    assert ends[-1] == len(res["waveform"]) / res["sampling_rate"] and ends[-1] >= starts[-1]
    words = res["word_timings"]
    assert " ".join(w for w, _, _ in words) == "".join(toks).strip()
    assert all(s <= e for _, s, e in words) and all(a[2] <= b[1] for a, b in zip(words, words[1:]))
    return "ok"


SENTENCES = ["a cat.", "hi, you two.", "this sentence has many more tokens than frames."]


def test_tts_with_timings_changes_nothing_else(syn):
    seen = set()
    for text in SENTENCES:
        torch.manual_seed(3)
        plain = syn.tts(text)
        torch.manual_seed(3)
        timed = syn.tts(text, timings=True)
        assert set(plain) == OLD_KEYS and set(timed) == OLD_KEYS | {"token_timings", "word_timings", "timings_status"}
        for k in OLD_KEYS:
            assert np.array_equal(np.asarray(plain[k]).view(np.uint8) if isinstance(plain[k], np.ndarray) else plain[k],
                                  np.asarray(timed[k]).view(np.uint8) if isinstance(timed[k], np.ndarray) else timed[k]), k
        seen.add(_check_timings(syn, text, timed))
    assert seen == {"ok", "infeasible"}          # max_decoder_steps of this checkpoint is 12: both branches are met
    torch.manual_seed(3)
    both = syn.tts(SENTENCES[0], timings=True, diagnostics=True, attention_window=(1, 3))
    assert {"alignment_stats", "stopped", "attention_window", "attention_centres", "token_timings"} <= set(both)
    _check_timings(syn, SENTENCES[0], both)


@pytest.mark.parametrize("rate", [None, 16000])
def test_tts_batch_with_timings(syn, rate):
    torch.manual_seed(5)
    plain = syn.tts_batch(SENTENCES, sampling_rate=rate)
    torch.manual_seed(5)
    timed = syn.tts_batch(SENTENCES, sampling_rate=rate, timings=True)
    seen = set()
    for text, p, t in zip(SENTENCES, plain, timed):
        assert set(p) == OLD_KEYS and set(t) == OLD_KEYS | {"token_timings", "word_timings", "timings_status"}
        for k in OLD_KEYS - {"sampling_rate"}:
            assert p[k].shape == t[k].shape and np.array_equal(p[k].view(np.uint8), t[k].view(np.uint8)), k
        assert t["sampling_rate"] == (rate or 22050) == p["sampling_rate"]
        seen.add(_check_timings(syn, text, t))
    assert seen == {"ok", "infeasible"}
    if rate is not None:   # seconds do not depend on the rate delivered, except the last end (the waveform's own length)
        torch.manual_seed(5)
        own = syn.tts_batch(SENTENCES, timings=True)
        for a, b in zip(own, timed):
            assert [x[:2] for x in a["token_timings"]] == [x[:2] for x in b["token_timings"]]


def test_token_durations_are_the_search_on_forwards_own_alignments():
    from genvox_amd import weights as gw
    from genvox_amd.collate import TextMelCollateFn
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
    from genvox_amd.tacotron2 import Tacotron2

    mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024, log_func="np.log"), TextConfig(n_tokens=30)
    m = Tacotron2(mc, ac, tc).to("cuda:0")
    m.eval()
    g = torch.Generator().manual_seed(0)
    items = [{"tokens": torch.randint(0, 30, (n,), generator=g, dtype=torch.int32), "features": torch.randn(80, t, generator=g)}
             for n, t in ((9, 14), (21, 30), (15, 22), (12, 8))]
    batch = m.prepare_batch(TextMelCollateFn()(items), "cuda:0")
    B, T = batch["mel_padded"].shape[0], batch["mel_padded"].shape[2]
    masks = torch.from_numpy(gw.prenet_keep_masks((T + 1) * B, mc.prenet_dim)).reshape(2, T + 1, B, mc.prenet_dim)
    got = m.token_durations(batch, prenet_keep_masks=masks)
    assert set(got) == {"durations", "status"}
    out = m.forward({**batch, "prenet_keep_masks": masks})
    want = metrics.monotonic_align(out["alignments"], batch["mel_lengths"], batch["token_lengths"])
    assert torch.equal(got["durations"], want["durations"]) and torch.equal(got["status"], want["status"])
    ml, tl = batch["mel_lengths"].tolist(), batch["token_lengths"].tolist()
    for b in range(B):
        if ml[b] >= tl[b]:
            assert got["status"][b].item() == 0 and int(got["durations"][b].sum()) == ml[b]
            assert int(got["durations"][b, :tl[b]].min()) >= 1 and int(got["durations"][b, tl[b]:].sum()) == 0
        else:
            assert got["status"][b].item() == 2 and int(got["durations"][b].sum()) == 0
    assert sorted(zip(tl, ml)) == sorted([(9, 14), (21, 30), (15, 22), (12, 8)])      # one row has fewer frames than tokens
    free = m.token_durations(batch)                                                       # masks drawn from torch's RNG: still a valid answer
    assert free["durations"].shape == got["durations"].shape
