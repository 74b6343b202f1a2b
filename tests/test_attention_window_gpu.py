"""GPU: the autoregressive decode with a monotonic attention window - gvx_decoder_autoregressive_windowed through ctypes with buffers
of its own (sentinel borders, junk-filled outputs, as run_ar of tests/test_forward_loops_gpu.py), against the float64 decode of
tests/forward_window_ref64.py on every loop kind a windowed call can take; "off means off"; what the window guarantees through
Tacotron2.inference / Synthesizer; the chunked paths; repeatability on a dirty workspace.

Bounds: the ar_* bounds of tests/test_forward_loops_gpu.py (imported through its _check_ar, not restated) for mel, gate and alignment
per step slice, its row-sum bound and padding values.  Centres and frame counts are compared EXACTLY: tests/test_attention_window_cpu.py
holds every (case, weight set) used here to a top-two gap of 100 times the GPU's measured alignment error (CENTRE_MARGIN there).

Which kinds there are: the resident pair applies the window in its one-workgroup-per-row attention kernel (L <= 128, kind 2);
every other shape - rows of 129-256 tokens, which the un-windowed call gives to two workgroups per row, and handles with
GVX_AR_RESIDENT=1 - takes the launches per step (kind 0, with and without split_h), and GVX_ATTN_SPLIT=1 the two-kernel attention
step.  tests/attention_window_cases.py has a case for each.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics, weights as gw
from genvox_amd.tacotron2 import STREAM_ROWS, Tacotron2, dims_from_configs
from tests import forward_window_ref64 as fw
from tests.attention_window_cases import BY_NAME, WINDOW_CASES, WSET, reference
from tests.helpers import AR_CASES_FWD, create_handle, fwd_configs, graph_replays
from tests.test_bptt_gpu import GUARD, SENTINEL, _Out
from tests.test_forward_loops_gpu import (TOL, _ar_reference, _check_ar, _handle, _slack_intact, _status_clean, _stream, _weights, _workspace,
                                          run_ar)
from tests.test_attention_window_cpu import windowed_plan
from tests.test_tts_batch_gpu import TEXTS, syn  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ar_unwindowed_sha256.json")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    """The handles, blobs and references this module put into the caches of tests/test_forward_loops_gpu.py go when it is done."""
    yield
    from tests import test_forward_loops_gpu as T
    lib = _lib.load()
    torch.cuda.synchronize()
    for h in T._HANDLES.values():
        lib.gvx_model_destroy(h)
    T._HANDLES.clear(); T._WEIGHTS.clear(); T._REF.clear()


def run_ar_windowed(lib, h, cfgs, case, dev, thr, window, ws=None):
    """run_ar of tests/test_forward_loops_gpu.py for the windowed export: one more output with a border, junk-filled."""
    mc, ac, _ = cfgs
    B, L, S, M = case.B, case.L, case.T, ac.n_mels
    outs = {"mel": _Out((B, M, S), junk=True), "gate": _Out((B, S), junk=True), "align": _Out((B, S, L), junk=True)}
    nf = torch.full((B + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    cen = torch.full((B * S + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    cen[GUARD:GUARD + B * S] = 77777                                          # junk no centre can be
    nbytes = lib.gvx_workspace_bytes_autoregressive(h, B, L, S)
    assert nbytes > 0
    ws = _workspace(nbytes) if ws is None else ws
    steps = C.c_int(-1)
    rc = lib.gvx_decoder_autoregressive_windowed(
        h, dev["memory"].data_ptr(), dev["lengths"].data_ptr(), B, L, S, thr, dev["keep"].data_ptr(), outs["mel"].t.data_ptr(),
        outs["gate"].t.data_ptr(), outs["align"].t.data_ptr(), nf[GUARD:].data_ptr(), C.byref(steps), ws.data_ptr(), nbytes, _stream(),
        window[0], window[1], cen[GUARD:].data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (case.name, rc, lib.gvx_last_error())
    for k, o in outs.items():
        assert o.border_intact(), f"{case.name}: the call wrote outside {k}"
    assert bool((nf[:GUARD] == SENTINEL).all()) and bool((nf[GUARD + B:] == SENTINEL).all()), f"{case.name}: the call wrote outside n_frames_out"
    assert bool((cen[:GUARD] == SENTINEL).all()) and bool((cen[GUARD + B * S:] == SENTINEL).all()), f"{case.name}: the call wrote outside centres_out"
    assert _slack_intact(ws, nbytes), f"{case.name}: the call wrote behind its workspace"
    assert _status_clean(lib, h, ws, nbytes), f"{case.name}: a status word of the workspace is set"
    return outs, nf[GUARD:GUARD + B].cpu(), steps.value, ws, cen[GUARD:GUARD + B * S].view(B, S).cpu()


def _check_windowed(case, wname, outs, nf, steps, cen, want, lengths, kind, window):
    name = f"{case.name}/{wname}"
    _check_ar(case, outs, nf, steps, want, lengths, wname, kind)              # frame counts, steps, padding, ar_* bounds, row sums
    assert torch.equal(cen.long(), want["centres"]), (name, cen.tolist(), want["centres"].tolist())
    # weights outside every live step's window are exactly 0 (the window of step t sits at the centre step t - 1 gave)
    align = outs["align"].t.cpu()
    prev = torch.cat((torch.zeros(case.B, 1, dtype=torch.long), want["centres"][:, :-1]), 1)
    for b in range(case.B):
        for t in range(int(want["n_frames"][b])):
            out = fw.outside_window([int(prev[b, t])], window[0], window[1], case.L)[0]
            assert bool((align[b, t][out] == 0).all()), f"{name}: weight outside the window of row {b}, step {t}"
            assert int(cen[b, t]) == int(align[b, t].argmax()), name              # ... and the centre is the row's own argmax
    st = metrics.alignment_stats(outs["align"].t, nf.cuda(), torch.tensor(lengths, dtype=torch.int32).cuda())
    assert torch.equal(st["positions"].cpu(), cen), f"{name}: centres are not the positions of gvx_alignment_stats"


@pytest.mark.parametrize("case", WINDOW_CASES, ids=lambda c: c.name)
def test_windowed_decode_against_float64(lib, case):
    cfgs = fwd_configs(case.dims)
    for wname in case.wsets:
        h = _handle(lib, case.dims, cfgs, WSET[wname], case.env)
        rc, plan = windowed_plan(lib, h, case.B, case.L)
        assert rc == 0 and plan == case.plan, (case.name, plan)
        inp, want, thr = reference(case, wname)
        dev = {k: v.cuda() for k, v in inp.items()}
        outs, nf, steps, _, cen = run_ar_windowed(lib, h, cfgs, case, dev, thr, case.window)
        _check_windowed(case, wname, outs, nf, steps, cen, want, inp["lengths"].tolist(), plan[0], case.window)


def test_windowed_graph_replay(lib):
    """The launches per step bake the caller's centre buffer into their graphs: three calls on one handle and workspace with the SAME
    centre buffer - eager, capture + replay, replay - then a fourth with ANOTHER buffer, which must not replay the graphs of the first."""
    case, wname = BY_NAME["w0_loop0_5x77"], "peaky"
    cfgs = fwd_configs(case.dims)
    h = create_handle(lib, dims_from_configs(*cfgs), case.env)
    try:
        assert lib.gvx_model_bind_blob(h, _weights(case.dims, cfgs, WSET[wname])[1].data_ptr()) == 0
        inp, want, thr = reference(case, wname)
        dev = {k: v.cuda() for k, v in inp.items()}
        mc, ac, _ = cfgs
        B, L, S, M = case.B, case.L, case.T, ac.n_mels
        nbytes = lib.gvx_workspace_bytes_autoregressive(h, B, L, S)
        ws = _workspace(nbytes)
        cen = [torch.full((B, S), 77777, dtype=torch.int32, device="cuda") for _ in range(2)]
        runs, counts = [], [graph_replays(lib, h)]
        for i in range(4):
            outs = {"mel": _Out((B, M, S), junk=True), "gate": _Out((B, S), junk=True), "align": _Out((B, S, L), junk=True)}
            nf = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
            c = cen[0 if i < 3 else 1]
            c.fill_(77777)
            steps = C.c_int(-1)
            assert lib.gvx_decoder_autoregressive_windowed(
                h, dev["memory"].data_ptr(), dev["lengths"].data_ptr(), B, L, S, thr, dev["keep"].data_ptr(), outs["mel"].t.data_ptr(),
                outs["gate"].t.data_ptr(), outs["align"].t.data_ptr(), nf.data_ptr(), C.byref(steps), ws.data_ptr(), nbytes, _stream(),
                case.window[0], case.window[1], c.data_ptr()) == 0, lib.gvx_last_error()
            torch.cuda.synchronize()
            _check_windowed(case, wname, outs, nf.cpu(), steps.value, c.cpu(), want, inp["lengths"].tolist(), 0, case.window)
            runs.append(outs)
            counts.append(graph_replays(lib, h))
        assert counts[0] == 0 and counts[1] == 0 and counts[1] < counts[2] < counts[3], counts
        assert counts[4] == counts[3], counts                                     # a new centre buffer is a new key: eager again
        for k in runs[0]:
            for r in runs[1:]:
                assert torch.equal(runs[0][k].t, r[k].t), f"{k} differs between the eager run and a replay"
    finally:
        torch.cuda.synchronize()
        lib.gvx_model_destroy(h)


# ---------------------------------------------------------------------------------------------------- off means off
def _sha(outs, nf):
    return hashlib.sha256(b"".join(outs[k].t.cpu().numpy().tobytes() for k in ("mel", "gate", "align")) + nf.numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("case", AR_CASES_FWD, ids=lambda c: c.name)
def test_unwindowed_call_is_what_it_was_bit_for_bit(lib, case):
    """gvx_decoder_autoregressive on the AR_CASES_FWD shapes: SHA-256 over (mel, gate, align, n_frames) equals the one recorded on the
    commit before the window existed (tests/golden/ar_unwindowed_sha256.json, both weight sets)."""
    golden = json.load(open(GOLDEN))
    cfgs = fwd_configs(case.dims)
    from tests.test_forward_loops_gpu import WEIGHT_SETS
    for wset in WEIGHT_SETS:
        h = _handle(lib, case.dims, cfgs, wset, case.env, case.setter)
        inp, _, thr = _ar_reference(case, cfgs, wset)
        outs, nf, _, _ = run_ar(lib, h, cfgs, case, {k: v.cuda() for k, v in inp.items()}, thr)
        assert _sha(outs, nf) == golden[f"{case.name}/{wset[0]}"], f"{case.name}/{wset[0]}: the un-windowed decode changed"


@pytest.mark.parametrize("name", ["ar2_1x1", "ar2_5x77", "ar2_32x128", "ar0_17x129", "ar0_2x257", "ar0_loop0_5x77", "ar0_nosplit_5x77",
                                  "ar0_att16_3x40", "ar0_att256_3x40", "ar0_36x30", "ar0_small_5x13"])
def test_a_window_over_the_whole_row_is_the_unwindowed_call_bit_for_bit(lib, name):
    """Where the windowed and the un-windowed call take the same loop kind and split: mel, gate, alignments and frame counts are
    equal to the bit for a window of (L, L), and the centres are the alignments' argmax."""
    case = {c.name: c for c in AR_CASES_FWD}[name]
    cfgs = fwd_configs(case.dims)
    from tests.test_forward_loops_gpu import WEIGHT_SETS
    for wset in WEIGHT_SETS:
        h = _handle(lib, case.dims, cfgs, wset, case.env, case.setter)
        assert windowed_plan(lib, h, case.B, case.L)[1] == tuple(case.plan), name     # same kind, split_h, fold, graph
        inp, _, thr = _ar_reference(case, cfgs, wset)
        dev = {k: v.cuda() for k, v in inp.items()}
        a, nfa, sa, _ = run_ar(lib, h, cfgs, case, dev, thr)
        b, nfb, sb, _, cen = run_ar_windowed(lib, h, cfgs, case, dev, thr, (case.L, case.L))
        assert nfa.tolist() == nfb.tolist() and sa == sb
        for k in a:
            assert torch.equal(a[k].t, b[k].t), f"{name}/{wset[0]}: {k} differs under a window that covers the row"
        live = torch.arange(case.T)[None, :] < nfa[:, None]
        am = a["align"].t.cpu().argmax(-1)
        assert torch.equal(cen[live].long(), am[live]) and bool((cen[~live] == -1).all())


# ---------------------------------------------------------------------------------------------------- through the public surface
STEPS = 40


@pytest.fixture(scope="module")
def model():
    """Default layer sizes, a PLAIN weight set (seed 2): attention is near uniform and the free decode wanders - its most attended
    token jumps by up to 58 positions between two frames on the rows of test_what_the_window_guarantees."""
    mc, ac, tc = fwd_configs("def")
    mc.max_decoder_steps, mc.gate_threshold = STEPS, 1.0                           # (sigmoid never passes 1: every row runs STEPS frames)
    m = Tacotron2(mc, ac, tc)
    m.load_state_dict(gw.generate_state_dict(mc, ac, tc, seed=2, peaky_attention=False))
    return m.to("cuda:0")


def _tokens(B, L, lengths, seed=3):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, 40, (B, L), generator=g)
    for b, n in enumerate(lengths):
        tok[b, n:] = 0
    return tok


def _masks(B, P, seed=4, steps=STEPS):
    return (torch.rand(2, steps, B, P, generator=torch.Generator().manual_seed(seed)) < 0.5).to(torch.uint8)


def test_what_the_window_guarantees(model):
    B, L = 4, 60
    lengths = [60, 47, 33, 21]
    inputs = {"tokens": _tokens(B, L, lengths), "token_lengths": torch.tensor(lengths, dtype=torch.int32),
              "prenet_keep_masks": _masks(B, model.model_config.prenet_dim)}
    assert model.ar_windowed_loop_kind(B, L) == 2
    tl = inputs["token_lengths"].cuda()
    free = model.inference(inputs)
    assert "attention_centres" not in free
    free_jump = metrics.alignment_stats(free["alignments"], free["mel_lengths"], tl)["max_jump"].cpu()
    for back, ahead in ((1, 3), (0, 1), (3, 10), (0, 2)):
        out = model.inference({**inputs, "attention_window": (back, ahead)})
        st = metrics.alignment_stats(out["alignments"], out["mel_lengths"], tl)
        assert out["attention_centres"].dtype == torch.int32 and out["attention_centres"].shape == out["alignments"].shape[:2]
        assert torch.equal(st["positions"], out["attention_centres"])
        assert bool((st["max_jump"] <= max(back, ahead)).all()), (back, ahead, st["max_jump"].tolist())
        if back == 0:
            assert bool((st["monotonic_fraction"] == 1).all()), st["monotonic_fraction"].tolist()
        assert set(out) == set(free) | {"attention_centres"}
        # the test can fail: the same input without a window breaks this bound
        assert bool((free_jump > max(back, ahead)).any()), (back, ahead, free_jump.tolist())
    assert int((free_jump > 10).sum()) >= 2, free_jump.tolist()
    # eval_synthesis passes the window on
    batch = {"token_padded": inputs["tokens"], "token_lengths": inputs["token_lengths"], "mel_lengths": torch.full((B,), STEPS, dtype=torch.int32),
             "mel_padded": torch.zeros(B, model.audio_config.n_mels, STEPS)}
    ev = model.eval_synthesis(batch, prenet_keep_masks=inputs["prenet_keep_masks"], attention_window=(0, 2))
    assert bool((ev["alignment_stats"]["max_jump"] <= 2).all()) and torch.equal(ev["attention_centres"], out["attention_centres"])
    model.check_status()


def _rows_match(big, one, b, name):
    """Row b of a batched run against its batch-1 run as test_rows_do_not_depend_on_the_batch states it: per step, twice the float64
    bound relative to the step's largest entry."""
    n = one["mel_outputs"].shape[2]
    pairs = {"ar_mel": (big["mel_outputs"][b, :, :n].t(), one["mel_outputs"][0].t()), "ar_align": (big["alignments"][b, :n], one["alignments"][0])}
    for k, (x, y) in pairs.items():
        x, y = x.double().cpu(), y.double().cpu()
        assert bool((x[:, y.shape[1]:] == 0).all()), f"{name}: row {b} has weight past its length"
        for t in range(n):
            assert float((x[t, :y.shape[1]] - y[t]).abs().max()) <= 2 * TOL[k] * float(y[t].abs().max()), f"{name}: {k}[{t}] of row {b} moves with the batch"


@pytest.mark.parametrize("B,L,kind", [(STREAM_ROWS + 2, 40, 2), (STREAM_ROWS + 2, 130, 0)], ids=["sequential_chunks", "two_lanes"])
def test_chunked_inference_passes_the_window_on(model, monkeypatch, B, L, kind):
    """More than STREAM_ROWS rows: chunks one after the other (every chunk the resident pair) and on two lanes (rows of 130 tokens: kind 0).
    Every row obeys the window, and the rows looked at equal their batch-1 windowed runs (on the same padded tokens: the encoder's
    convolutions see a row's padding, with or without a window)."""
    monkeypatch.setattr(model.model_config, "max_decoder_steps", 12)
    window, S, P = (1, 3), 12, model.model_config.prenet_dim
    lengths = [max(5, L - 3 * b) for b in range(B)]
    tokens, masks = _tokens(B, L, lengths, seed=8), _masks(B, P, seed=9, steps=S)
    assert model.ar_windowed_loop_kind(B // 2, L) == kind
    big = model.inference({"tokens": tokens, "token_lengths": torch.tensor(lengths, dtype=torch.int32), "prenet_keep_masks": masks,
                           "attention_window": window})
    st = metrics.alignment_stats(big["alignments"], big["mel_lengths"], torch.tensor(lengths, dtype=torch.int32).cuda())
    assert torch.equal(st["positions"], big["attention_centres"]) and bool((st["max_jump"] <= 3).all())
    assert big["mel_lengths"].tolist() == [S] * B
    for b in (0, B // 2 - 1, B // 2, B - 1):                                       # first and last row of both chunks
        one = model.inference({"tokens": tokens[b:b + 1], "token_lengths": torch.tensor(lengths[b:b + 1], dtype=torch.int32),
                               "prenet_keep_masks": masks[:, :, b:b + 1], "attention_window": window})
        _rows_match(big, one, b, f"{B}x{L}")
    model.check_status()


def test_tts_batch_with_a_window(syn):  # noqa: F811
    """Synthesizer.tts_batch(attention_window=...): more sentences than STREAM_ROWS in one decoder call (chunks), every sentence with
    its own centres, bounded jumps, and the diagnostics record the window; tts gives the same keys for one sentence."""
    syn.tts_model.model_config.gate_threshold = 1.0
    texts = [TEXTS[i % len(TEXTS)] + " " + "ab" * (i % 4) for i in range(STREAM_ROWS + 3)]
    torch.manual_seed(5)
    plain = syn.tts_batch(texts[:3], diagnostics=True)
    torch.manual_seed(5)
    res = syn.tts_batch(texts, batch_size=64, diagnostics=True, attention_window=(0, 2))
    assert len(res) == len(texts)
    for r in res:
        assert set(r) == set(plain[0]) | {"attention_centres", "attention_window"} and r["attention_window"] == (0, 2)
        c = r["attention_centres"]
        assert c.dtype == np.int32 and c.shape == r["alignments"].shape[:1] and np.array_equal(c, r["alignments"].argmax(-1))
        d = np.diff(np.concatenate(([0], c)))
        assert d.min() >= 0 and d.max() <= 2 and r["alignment_stats"]["max_jump"] <= 2 and r["alignment_stats"]["monotonic_fraction"] == 1.0
    one = syn.tts(texts[0], diagnostics=True, attention_window=(0, 2))
    assert set(one) == set(res[0]) and one["attention_window"] == (0, 2) and one["attention_centres"].shape == one["alignments"].shape[:1]
    assert "attention_window" not in plain[0] and "attention_centres" not in plain[0]


# ---------------------------------------------------------------------------------------------------- twice, on a dirty workspace
@pytest.mark.parametrize("name", ["w2_5x77", "w2_32x128", "w0_17x129", "w0_nosplit_5x77", "w0_pair_5x77"])
def test_two_identical_windowed_calls_are_bit_equal(lib, name):
    """Two calls with the same inputs agree to the bit, the second on the workspace the first left behind (and behind an un-windowed
    call on it, whose leftovers are not the window's state: centres_out is)."""
    case, wname = BY_NAME[name], "peaky"
    cfgs = fwd_configs(case.dims)
    h = _handle(lib, case.dims, cfgs, WSET[wname], case.env)
    inp, want, thr = reference(case, wname)
    dev = {k: v.cuda() for k, v in inp.items()}
    a, nfa, sa, ws, ca = run_ar_windowed(lib, h, cfgs, case, dev, thr, case.window)
    run_ar(lib, h, cfgs, case, dev, thr, ws)
    b, nfb, sb, _, cb = run_ar_windowed(lib, h, cfgs, case, dev, thr, case.window, ws)
    assert nfa.tolist() == nfb.tolist() and sa == sb and torch.equal(ca, cb) and torch.equal(ca.long(), want["centres"])
    for k in a:
        assert torch.equal(a[k].t, b[k].t), f"{name}: {k} differs between two identical windowed calls"
