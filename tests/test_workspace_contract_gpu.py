"""GPU: the workspace contract of include/genvox_amd.h ("Workspaces and scratch"), held against every entry point that takes scratch.

The contract.  The caller clears the first GVX_WORKSPACE_CLEAR_BYTES (12804) bytes of a model workspace once, before first use; every
other byte of a workspace, a `saved` buffer or a scratch may hold any bit pattern - NaN, the leftovers of a call of another shape -
and no call writes outside [buffer, buffer + declared bytes).  One byte short is GVX_ERR_WORKSPACE and nothing is launched.

The reference of every comparison is THE SAME CALL on a zero-filled, freshly allocated scratch, and the criterion is bit equality
of every output (compared as bytes: NaN cannot compare equal by accident, -0.0 is not 0.0).  No tolerance anywhere in this file; what
the numbers are is the business of the float64 tests of each kernel family.

The arena: one device allocation [4 KiB of sentinel | scratch | sentinel], the scratch 256-byte aligned and exactly as many bytes as
the size query gave (the sentinel begins at the next byte); outputs stay in the sentinel-bordered, junk-filled _Out buffers of
tests/test_bptt_gpu.py.

Dirt, applied behind the contract's own clear:
  nan       every 32-bit word 0x7FF8BEEF: a quiet NaN as a float, a quiet NaN as the half of a double, positive as an integer (a
            counter or flag read from it is large, not negative), recognisable in a dump;
  leftover  what a call of the same handle at another B, L and T (another B T for the vocoder) left there, itself run on nan dirt;
  replay    on shapes whose loop replays a hipGraph: A, A until the replay counter moves, a call of shape B on the same workspace,
            nan dirt, A again - that last call is a replay (the counter says so) and bit-equal to the clean run.
Checked per case: return code 0 and both status words 0 (the run helpers assert it), every output bit-equal to the clean run and
finite, both guards intact, and with declared - 1 bytes GVX_ERR_WORKSPACE with outputs and guards untouched.

Cases come from the tables of tests/helpers.py, one per distinct plan (the plan tuple, layer sizes, settings and mode are the key).
No test here sets a debug knob or a spin limit: a wrong hand-off word shows as NaN outputs and status word [1].

The clean run of a case is computed once and shared by its dirt kinds (_CLEAN).
"""
import ctypes as C

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.tacotron2 import dims_from_configs
from tests import test_bptt_gpu as tb
from tests import test_conv_train_gpu as tcv
from tests import test_forward_loops_gpu as tf
from tests.helpers import (AR_CASES_FWD, BPTT_CASES, CONV_TRAIN_BY_NAME, ENC_BPTT_CASES, ENC_FWD_CASES, ENC_WHOLE_CASES, GEMM_SPLITK_CASES, TF_CASES_FWD,
                           TF_TRAIN_CASES_FWD, bptt_lengths, create_handle, decoder_plan, enc_fwd_configs, fwd_configs, gemm_scratch_bytes, graph_replays)
from tests.test_bptt_gpu import _Out

pytestmark = pytest.mark.gpu

NAN_WORD = 0x7FF8BEEF
CLEAR = 12804              # GVX_WORKSPACE_CLEAR_BYTES: the status words (bytes 0 .. 11) up to and including the hand-off time-out word
GUARD_BYTES = 4096
ERR_WORKSPACE = -5
WSET = tf.WEIGHT_SETS[1]   # peaky attention: the location features and the mask decide the result
DIRTS = ["leftover", "nan"]
_CLEAN = {}                # case label -> outputs of the call on a clean scratch (one clean run per case, shared by its dirt kinds)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _handles():
    yield
    torch.cuda.synchronize()
    lib = _lib.load()
    for h in tf._HANDLES.values():
        lib.gvx_model_destroy(h)
    tf._HANDLES.clear(); tf._WEIGHTS.clear(); tf._REF.clear(); _CLEAN.clear()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Arena:
    """[guard | cap bytes | guard] in one allocation.  view(n): the first n bytes of the scratch, as the tensor a call is given;
    seal(n): sentinel from byte n on; intact(n): both guards and everything from byte n on still hold the sentinel."""

    def __init__(self, cap, clear=0):
        self.cap = cap
        self.buf = torch.full((2 * GUARD_BYTES + (cap + 3) // 4 * 4,), 0x5A, dtype=torch.uint8, device="cuda")
        assert (self.buf.data_ptr() + GUARD_BYTES) % 256 == 0 and tb.SENTINEL == 0x5A5A5A5A
        self.buf[GUARD_BYTES:GUARD_BYTES + cap] = 0                          # clean: zero-filled (the contract's clear with it)
        self.clear = clear

    def view(self, n):
        assert 0 <= n <= self.cap
        return self.buf[GUARD_BYTES:GUARD_BYTES + n]

    def seal(self, n):
        self.buf[GUARD_BYTES + n:] = 0x5A

    def dirty(self, n):
        """NaN words in [clear, n), sentinel behind.  The cleared front is left as the calls before left it."""
        assert self.clear % 4 == 0 and n >= self.clear
        words = self.buf[GUARD_BYTES + self.clear:GUARD_BYTES + self.clear + (n - self.clear) // 4 * 4].view(torch.int32)
        words.fill_(NAN_WORD)
        self.buf[GUARD_BYTES + self.clear + words.numel() * 4:GUARD_BYTES + n] = 0x7F
        self.seal(n)

    def intact(self, n):
        return bool((self.buf[:GUARD_BYTES] == 0x5A).all()) and bool((self.buf[GUARD_BYTES + n:] == 0x5A).all())


def _payload(o):
    return o.t if isinstance(o, (_Out, tcv._Out)) else o


def _bytes(x):
    return _payload(x).contiguous().view(-1).view(torch.uint8)


def _same(ref, got, what):
    assert ref.keys() == got.keys(), what
    for k in ref:
        a, b = _payload(ref[k]), _payload(got[k])
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()), f"{what}: {k} of the clean run is not finite"
            assert bool(torch.isfinite(b).all()), f"{what}: {k} is not finite"
        assert torch.equal(_bytes(a), _bytes(b)), f"{what}: {k} differs from the run on a clean scratch in {int((_bytes(a) != _bytes(b)).sum())} bytes"


def _pristine(outs, what):
    """A refused call wrote nothing: sentinel-filled outputs still all sentinel, junk-filled ones still their junk."""
    for k, o in outs.items():
        if not isinstance(o, _Out):
            continue
        assert o.border_intact(), f"{what}: {k}"
        assert o.untouched() or torch.equal(o.t, _Out(tuple(o.t.shape), junk=True).t), f"{what}: the refused call wrote to {k}"


def hold(dirt, what, run, n, other=None, clear=0):
    """run(ws, **kw) -> {name: output}: one call on the byte tensor ws (exactly n bytes; kw: expect, ws_bytes for the refused call).
    other = (run of the leftover shape, its bytes).  dirt: "nan", "leftover" or "short".  `what` names the case: its clean run is
    made once and kept for the other dirt kinds."""
    assert n > 0
    if what not in _CLEAN:
        clean = Arena(n, clear)
        outs = run(clean.view(n))
        assert clean.intact(n), f"{what}: the call on a clean scratch wrote outside its {n} bytes"
        _CLEAN[what] = {k: _payload(v).clone() for k, v in outs.items()}
    ref = _CLEAN[what]
    if dirt == "short":
        a = Arena(n, clear)
        a.dirty(n)
        before = a.view(n).clone()
        outs = run(a.view(n), expect=ERR_WORKSPACE, ws_bytes=n - 1)
        _pristine(outs, what)
        assert a.intact(n) and torch.equal(a.view(n), before), f"{what}: a refused call wrote to its workspace"
        return ref
    n_other = other[1] if (dirt == "leftover" and other) else 0
    a = Arena(max(n, n_other), clear)
    if dirt == "leftover":
        assert other is not None and n_other > 0
        a.dirty(n_other)
        other[0](a.view(n_other))
        assert a.intact(n_other), f"{what}: the call of the other shape wrote outside its {n_other} bytes"
        if n > n_other:
            fresh = Arena(n, clear)                                          # (the bytes the other shape did not own: NaN)
            fresh.dirty(n)
            a.view(n)[n_other:] = fresh.view(n)[n_other:]
        a.seal(n)
    else:
        a.dirty(n)
    got = run(a.view(n))
    assert a.intact(n), f"{what}: the call wrote outside its {n} bytes under {dirt} dirt"
    _same(ref, got, f"{what} [{dirt}]")
    return ref


# ------------------------------------------------------------------------------------------------------------ decoder loops
def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.dims, tuple(sorted(c.env.items())), c.setter, c.mode, c.drop, tuple(c.plan))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _other_shape(case):
    """Another B, L and T on the same handle: every region of make_ws_plan behind the encoder's first buffer moves."""
    B = case.B + 1 if case.B < 32 else case.B - 1
    L = case.L + 3 if case.L < 250 else case.L - 5
    return case._replace(name=case.name + "/other", B=B, L=L, T=case.T + 1, lengths="ragged")


def _tf_run(lib, h, cfgs, case):
    dev = {k: v.cuda() for k, v in tf._tf_inputs(case, cfgs, WSET[0]).items()}
    return lambda ws, **kw: tf.run_tf(lib, h, cfgs, case, dev, ws=ws, **kw)[0]


def _ar_inputs(case, cfgs):
    mc = cfgs[0]
    B, L, S = case.B, case.L, case.T
    g = tf._gen(case.name, 1)
    lengths = bptt_lengths(case.lengths, B, L)
    return {"lengths": torch.tensor(lengths, dtype=torch.int32), "memory": tf._memory(g, B, L, mc.encoder_embedding_dim, lengths),
            "keep": (torch.rand(2, S, B, mc.prenet_dim, generator=g) < 0.5).to(torch.uint8)}


_AR_THR = {}   # case name -> the threshold of its free run (one free run per case)


def _ar_run(lib, h, cfgs, case, thr=None):
    """The autoregressive call; thr None: a threshold from this call's own free run (the median of its gate probabilities, so that
    rows stop at different steps) - bit equality needs no margin around it, both runs see the same bits or the test fails."""
    dev = {k: v.cuda() for k, v in _ar_inputs(case, cfgs).items()}
    if thr is None and case.name not in _AR_THR:
        n = lib.gvx_workspace_bytes_autoregressive(h, case.B, case.L, case.T)
        free = tf.run_ar(lib, h, cfgs, case, dev, 2.0, ws=Arena(n, CLEAR).view(n))[0]
        _AR_THR[case.name] = float(torch.sigmoid(free["gate"].t).median())
    thr = _AR_THR[case.name] if thr is None else thr

    def run(ws, **kw):
        outs, nf, steps, _ = tf.run_ar(lib, h, cfgs, case, dev, thr, ws=ws, **kw)
        return dict(outs, n_frames=nf, steps=torch.tensor([steps]))
    return run


TF_DISTINCT = _distinct(TF_CASES_FWD + TF_TRAIN_CASES_FWD)
AR_DISTINCT = _distinct(AR_CASES_FWD) + [c for c in AR_CASES_FWD if c.name in ("ar0_36x30",)]   # (36 rows: more than one 32-row tile)
AR_DISTINCT = list({c.name: c for c in AR_DISTINCT}.values())


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("case", TF_DISTINCT, ids=lambda c: c.name)
def test_teacher_forced(lib, case, dirt):
    """gvx_decoder_teacher_forced and _train (every tape buffer is an output)."""
    cfgs = fwd_configs(case.dims)
    h = tf._handle(lib, case.dims, cfgs, WSET, case.env, case.setter)
    rc, plan, _ = decoder_plan(lib, h, case.mode, case.B, case.L)
    assert rc == 0 and plan == tuple(case.plan), (case.name, plan)
    other = _other_shape(case)
    if case.mode and other.B > 32:
        other = other._replace(B=case.B - 1)
    hold(dirt, "tf_" + case.name, _tf_run(lib, h, cfgs, case), lib.gvx_workspace_bytes(h, case.B, case.L, case.T),
         (_tf_run(lib, h, cfgs, other), lib.gvx_workspace_bytes(h, other.B, other.L, other.T)), clear=CLEAR)


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("case", AR_DISTINCT, ids=lambda c: c.name)
def test_autoregressive(lib, case, dirt):
    cfgs = fwd_configs(case.dims)
    h = tf._handle(lib, case.dims, cfgs, WSET, case.env, case.setter)
    rc, _, plan = decoder_plan(lib, h, 0, case.B, case.L)
    assert rc == 0 and plan == tuple(case.plan), (case.name, plan)
    other = _other_shape(case)
    ref = hold(dirt, "ar_" + case.name, _ar_run(lib, h, cfgs, case), lib.gvx_workspace_bytes_autoregressive(h, case.B, case.L, case.T),
               (_ar_run(lib, h, cfgs, other, thr=0.5), lib.gvx_workspace_bytes_autoregressive(h, other.B, other.L, other.T)), clear=CLEAR)
    assert int(ref["n_frames"].min()) >= 1


# ------------------------------------------------------------------------------------------------------------ encoder
def _enc_inputs(case):
    E = enc_fwd_configs(case.H)[0].encoder_embedding_dim
    g = tf._gen(case.name, 1)
    return {"conv": torch.randn(case.B, E, case.L, generator=g).clamp_min_(0.0), "lengths": torch.tensor(bptt_lengths(case.lengths, case.B, case.L), dtype=torch.int32)}


def _enc_run(lib, h, case, tapes):
    dev = {k: v.cuda() for k, v in _enc_inputs(case).items()}
    return lambda ws, **kw: tf.run_encoder_lstm(lib, h, case, dev, tapes, ws=ws, **kw)[0]


def _enc_distinct():
    seen, out = set(), []
    for c in ENC_FWD_CASES:
        key = (c.H, tuple(sorted(c.env.items())), c.plan, c.B > 32)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("tapes", [True, False], ids=["tapes", "bare"])
@pytest.mark.parametrize("case", _enc_distinct(), ids=lambda c: c.name)
def test_encoder_lstm_forward(lib, case, tapes, dirt):
    """gvx_encoder_lstm_forward: the resident launch and the launch per position, with and without the tapes."""
    cfgs = enc_fwd_configs(case.H)
    h = tf._handle(lib, ("enc", case.H), cfgs, WSET, case.env)
    assert tf.encoder_resident(lib, h, case.B) == case.plan
    other = case._replace(name=case.name + "/other", B=case.B + 1 if case.B < 32 else case.B - 1, L=case.L + 3, lengths="ragged")
    size = lambda c: lib.gvx_workspace_bytes_autoregressive(h, c.B, c.L, 1)
    hold(dirt, f"enc_{case.name}_{tapes}", _enc_run(lib, h, case, tapes), size(case), (_enc_run(lib, h, other, tapes), size(other)), clear=CLEAR)


def _whole_enc_run(lib, h, cfgs, B, L, bad_token=False):
    g = tf._gen("whole_%dx%d" % (B, L), 1)
    tok = torch.randint(0, cfgs[2].n_tokens, (B, L), generator=g).cuda()
    ln = torch.tensor(bptt_lengths("ragged", B, L), dtype=torch.int32).cuda()
    n = lib.gvx_workspace_bytes_autoregressive(h, B, L, 1)

    def run(ws, expect=0, ws_bytes=None):
        out = _Out((B, L, cfgs[0].encoder_embedding_dim), junk=True)
        rc = lib.gvx_encoder_forward(h, tok.data_ptr(), ln.data_ptr(), B, L, out.t.data_ptr(), ws.data_ptr(), n if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        assert rc == expect and out.border_intact(), (rc, lib.gvx_last_error())
        if not expect:
            assert tf._status_clean(lib, h, ws, n), "a status word of the workspace is set"
        return {"memory": out}
    return run, n


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("B,L", ENC_WHOLE_CASES)
def test_whole_encoder(lib, B, L, dirt):
    """gvx_encoder_forward (embedding, convolutions with their halo rows, recurrence); the token-error word must stay 0."""
    cfgs = fwd_configs("def")
    h = tf._handle(lib, "def", cfgs, WSET, {})
    run, n = _whole_enc_run(lib, h, cfgs, B, L)
    hold(dirt, f"whole_{B}x{L}", run, n, _whole_enc_run(lib, h, cfgs, B + 1, L + 3), clear=CLEAR)


# ------------------------------------------------------------------------------------------------------------ whole forward, Postnet
WHOLE = [("small", B, 13, 6) for B in (1, 5, 32, 33)] + [("def", B, 24, 5) for B in (1, 5, 32, 33)]


def _forward_run(lib, h, cfgs, B, L, T, tag):
    """gvx_tacotron2_forward with mel_lengths, then the four gvx_train_export copies out of the same workspace."""
    mc, ac, tc = cfgs
    M, P, a = ac.n_mels, mc.prenet_dim, mc.attention_dim
    g = tf._gen(f"{tag}_{B}x{L}x{T}", 0)
    tok = torch.randint(0, tc.n_tokens, (B, L), generator=g).cuda()
    tl = torch.tensor(bptt_lengths("ragged", B, L), dtype=torch.int32).cuda()
    ml = torch.tensor(sorted((1 + (i * 3) % T for i in range(B)), reverse=True), dtype=torch.int32).cuda()
    mel_in = torch.randn(B, M, T, generator=g).cuda()
    keep = (torch.rand(2, (T + 1) * B, P, generator=g) < 0.5).to(torch.uint8).cuda()
    n = lib.gvx_workspace_bytes(h, B, L, T)

    def run(ws, expect=0, ws_bytes=None):
        told = n if ws_bytes is None else ws_bytes
        o = {"mel": _Out((B, M, T), junk=True), "post": _Out((B, M, T), junk=True), "gate": _Out((B, T), junk=True), "align": _Out((B, T, L), junk=True)}
        rc = lib.gvx_tacotron2_forward(h, tok.data_ptr(), tl.data_ptr(), B, L, mel_in.data_ptr(), ml.data_ptr(), T, keep.data_ptr(), o["mel"].t.data_ptr(),
                                       o["post"].t.data_ptr(), o["gate"].t.data_ptr(), o["align"].t.data_ptr(), ws.data_ptr(), told, _stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, lib.gvx_last_error())
        exports = {"frames": ((T + 1) * B, M), "pre1": ((T + 1) * B, P), "prenet": ((T + 1) * B, P), "pm": (B, L, a)}
        for what, (k, shape) in enumerate(exports.items()):
            o[k] = _Out(shape, junk=True)
            rc = lib.gvx_train_export(h, ws.data_ptr(), told, B, L, T, what, o[k].t.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert rc == expect, (k, rc, lib.gvx_last_error())
        for k, x in o.items():
            assert x.border_intact(), k
        if not expect:
            assert tf._status_clean(lib, h, ws, n), "a status word of the workspace is set"
        return o
    return run, n


def _postnet_run(lib, h, cfgs, B, T, with_lengths):
    M = cfgs[1].n_mels
    g = tf._gen(f"postnet_{B}x{T}", 0)
    mel = torch.randn(B, M, T, generator=g).cuda()
    ml = torch.tensor([1 + (i * 3) % T for i in range(B)], dtype=torch.int32).cuda() if with_lengths else None
    n = lib.gvx_postnet_workspace_bytes(h, B, T)

    def run(ws, expect=0, ws_bytes=None):
        o = {"post": _Out((B, M, T), junk=True)}
        rc = lib.gvx_postnet_forward(h, mel.data_ptr(), ml.data_ptr() if with_lengths else None, B, T, o["post"].t.data_ptr(), ws.data_ptr(),
                                     n if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        assert rc == expect and o["post"].border_intact(), (rc, lib.gvx_last_error())
        if not expect:
            assert tf._status_clean(lib, h, ws, n), "a status word of the workspace is set"
        return o
    return run, n


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("dims,B,L,T", WHOLE)
def test_whole_forward_and_exports(lib, dims, B, L, T, dirt):
    cfgs = fwd_configs(dims)
    h = tf._handle(lib, dims, cfgs, WSET, {})
    run, n = _forward_run(lib, h, cfgs, B, L, T, "fwd")
    hold(dirt, f"forward_{dims}_{B}x{L}x{T}", run, n, _forward_run(lib, h, cfgs, B + 1 if B < 33 else B - 2, L + 3, T + 1, "fwd_other"), clear=CLEAR)


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("with_lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("dims,B,T", [("small", 1, 1), ("small", 5, 2), ("small", 33, 6), ("def", 1, 1), ("def", 5, 7), ("def", 32, 5), ("def", 33, 3)])
def test_postnet_on_its_own_workspace(lib, dims, B, T, with_lengths, dirt):
    """gvx_postnet_forward on gvx_postnet_workspace_bytes bytes, not on the big one: T below the halo (the separate halo clear) and above."""
    cfgs = fwd_configs(dims)
    h = tf._handle(lib, dims, cfgs, WSET, {})
    run, n = _postnet_run(lib, h, cfgs, B, T, with_lengths)
    hold(dirt, f"postnet_{dims}_{B}x{T}_{with_lengths}", run, n, _postnet_run(lib, h, cfgs, B + 2, T + 3, with_lengths), clear=CLEAR)


# ------------------------------------------------------------------------------------------------------------ graph replay
@pytest.mark.parametrize("name", tf.GRAPH_TF + tf.GRAPH_AR)
def test_replay_over_dirt_decoder_loops(lib, name):
    case = tf._BY_NAME[name]
    cfgs = fwd_configs(case.dims)
    h = create_handle(lib, dims_from_configs(*cfgs), case.env, case.setter)   # (a handle of its own: counter and sightings start at zero)
    try:
        assert lib.gvx_model_bind_blob(h, tf._weights(case.dims, cfgs, WSET)[1].data_ptr()) == 0
        ar = name in tf.GRAPH_AR
        other = _other_shape(case)
        if ar:
            size = lambda c: lib.gvx_workspace_bytes_autoregressive(h, c.B, c.L, c.T)
            run, run_other = _ar_run(lib, h, cfgs, case), _ar_run(lib, h, cfgs, other, thr=0.5)
        else:
            size = lambda c: lib.gvx_workspace_bytes(h, c.B, c.L, c.T)
            run, run_other = _tf_run(lib, h, cfgs, case), _tf_run(lib, h, cfgs, other)
        _replay(lib, h, name, run, size(case), run_other, size(other))
    finally:
        torch.cuda.synchronize()
        lib.gvx_model_destroy(h)


@pytest.mark.parametrize("name", ["H24_3x21", "H256_33x21", "H256_3x21_per_position"])
def test_replay_over_dirt_encoder_loop(lib, name):
    case = {c.name: c for c in ENC_FWD_CASES}[name]
    cfgs = enc_fwd_configs(case.H)
    h = create_handle(lib, dims_from_configs(*cfgs), case.env)
    try:
        assert lib.gvx_model_bind_blob(h, tf._weights(("enc", case.H), cfgs, WSET)[1].data_ptr()) == 0
        other = case._replace(name=name + "/other", B=case.B + 1, L=case.L + 3)
        size = lambda c: lib.gvx_workspace_bytes_autoregressive(h, c.B, c.L, 1)
        _replay(lib, h, name, _enc_run(lib, h, case, False), size(case), _enc_run(lib, h, other, False), size(other))
    finally:
        torch.cuda.synchronize()
        lib.gvx_model_destroy(h)


def _replay(lib, h, name, run, n, run_other, n_other):
    clean = Arena(n, CLEAR)
    ref = run(clean.view(n))
    a = Arena(max(n, n_other), CLEAR)
    a.seal(n)
    c0 = graph_replays(lib, h)
    for i in range(4):                                                       # eager, capture + replay, replay
        _same(ref, run(a.view(n)), f"{name} [call {i}]")
        if graph_replays(lib, h) > c0:
            break
    assert graph_replays(lib, h) > c0, f"{name}: the loop never replayed a graph"
    a.dirty(n_other)
    run_other(a.view(n_other))
    assert a.intact(n_other), name
    a.dirty(n)
    before = graph_replays(lib, h)
    got = run(a.view(n))
    assert graph_replays(lib, h) > before, f"{name}: the call after the dirt was not a replay"
    assert a.intact(n), f"{name}: the replay wrote outside its {n} bytes"
    _same(ref, got, f"{name} [replay over nan dirt]")


# ------------------------------------------------------------------------------------------------------------ BPTT
def _bptt_distinct():
    seen, out = set(), []
    for c in BPTT_CASES:
        key = (c.sizes, tuple(c.plan))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _bptt_size(lib, c):
    from tests.helpers import bptt_args_for_plan
    return lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(bptt_args_for_plan(c.B, c.L, c.T, c.sizes)))


def _bptt_inputs(c):
    """Inputs of the right shapes and ranges without the float64 forward: bit equality needs no consistent tape.  w_all is a real
    softmax row, exactly 0 at and past a row's length (the call's only masking)."""
    B, L, T = c.B, c.L, c.T
    A, D, E, P, a, Fn, kl = c.sizes
    g = torch.Generator().manual_seed(9000 + sum(map(ord, c.name)))
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    lengths = torch.tensor(bptt_lengths(c.lengths, B, L))
    mask = torch.arange(L)[None, :] >= lengths[:, None]
    w = torch.softmax(r(T, B, L).masked_fill(mask[None], float("-inf")), -1)
    inp = {"dhc_all": r(T, B, D + E), "pre_a": r(T, B, A, 4), "pre_d": r(T, B, D, 4), "c_a_all": r(T + 1, B, A), "c_d_all": r(T + 1, B, D), "q_all": r(T, B, a),
           "ctx_all": r(T, B, E), "w_all": w, "memory": r(B, L, E), "pm": r(B, L, a), "w_ih_a": r(4 * A, P + E, scale=(P + E) ** -0.5),
           "w_hh_a": r(4 * A, A, scale=A ** -0.5), "w_ih_d": r(4 * D, A + E, scale=(A + E) ** -0.5), "w_hh_d": r(4 * D, D, scale=D ** -0.5),
           "wq": r(a, A, scale=A ** -0.5), "v": r(a, scale=a ** -0.5), "loc_conv": r(Fn, 2, kl, scale=kl ** -0.5), "loc_dense": r(a, Fn, scale=Fn ** -0.5)}
    inp = {k: x.float().contiguous() for k, x in inp.items()}
    inp["att_keep"], inp["dec_keep"] = (torch.rand(T, B, A, generator=g) < 0.8).to(torch.uint8), (torch.rand(T, B, D, generator=g) < 0.8).to(torch.uint8)
    return inp, r(T, B, L).masked_fill(mask[None], 0.0).float().contiguous()


def _bptt_run(lib, c, ext):
    inp, dw = _bptt_inputs(c)

    def run(ws, expect=0, ws_bytes=None):
        mutate = None if ws_bytes is None else (lambda p, n: (p, ws_bytes))
        return tb.run_decoder(lib, c.B, c.L, c.T, c.sizes, inp, expect=expect, ws_mutate=mutate, ws=ws, dw_ext=dw if ext else None)[1]
    return run


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("case", _bptt_distinct(), ids=lambda c: c.name)
def test_decoder_bptt(lib, case, ext, dirt):
    """gvx_train_decoder_bptt and _ext.  The header: "the workspace needs no clearing" - so the clear is 0 bytes here."""
    other = case._replace(name=case.name + "/other", B=case.B + 1 if case.B < 32 else case.B - 1, L=case.L + 3 if case.L + 3 <= 664 else case.L - 5, T=case.T + 1,
                          lengths="ragged")
    hold(dirt, f"bptt_{case.name}_{ext}", _bptt_run(lib, case, ext), _bptt_size(lib, case), (_bptt_run(lib, other, ext), _bptt_size(lib, other)))


def _enc_bptt_distinct():
    seen, out = set(), []
    for c in ENC_BPTT_CASES:
        key = (c.H, tuple(c.plan))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _enc_bptt_run(lib, c, resident):
    B, L, H = c.B, c.L, c.H
    g = torch.Generator().manual_seed(9500 + sum(map(ord, c.name)))
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).float().contiguous()
    inp = {"xg": r(2, B, L, 4 * H), "memory": r(B, L, 2 * H).tanh(), "cell_states": r(B, L, 2 * H), "dmemory": r(B, L, 2 * H), "w_hh": r(2, 4 * H, H, scale=H ** -0.5),
           "lengths": torch.tensor(bptt_lengths(c.lengths, B, L), dtype=torch.int32)}
    return lambda ws, expect=0, ws_bytes=None: tb.run_encoder(lib, c, inp, resident, expect=expect, ws=ws, short_ws=0 if ws_bytes is None else 1)


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "per_step"])
@pytest.mark.parametrize("case", _enc_bptt_distinct(), ids=lambda c: c.name)
def test_encoder_bptt(lib, case, resident, dirt):
    """gvx_train_encoder_lstm_bptt(_resident): flag lines and the status word live in the workspace; nothing is cleared by the caller."""
    other = case._replace(name=case.name + "/other", B=case.B + 1, L=case.L + 2, lengths="ragged")
    size = lambda c: lib.gvx_train_encoder_lstm_bptt_workspace_bytes(c.B, c.H)
    hold(dirt, f"enc_bptt_{case.name}_{resident}", _enc_bptt_run(lib, case, resident), size(case), (_enc_bptt_run(lib, other, resident), size(other)))


# ------------------------------------------------------------------------------------------------------------ split-K GEMM
@pytest.mark.parametrize("dirt", ["nan", "leftover"])
@pytest.mark.parametrize("c", [c for c in GEMM_SPLITK_CASES if c.scratch is not None], ids=lambda c: "%s_%dx%dx%d_%s" % ("tn" if c.kmajor else "nt", c.M, c.N, c.K, c.scratch))
def test_splitk_gemm(lib, c, dirt):
    """gvx_train_gemm_nt / _tn with a scratch of exactly gemm_scratch_bytes(case).  (A short scratch is no error here: the header lets
    the call take fewer K pieces, and tests/test_gemm_gpu.py pins the piece counts.)"""
    from tests.test_gemm_gpu import make_operands
    a, w, bias = make_operands(c, "rounded", 77)
    n = gemm_scratch_bytes(c)

    def runner(c2, a2, w2, b2, n2):
        def run(ws):
            M, N, K = c2.M, c2.N, c2.K
            out = _Out((M, N), junk=True)
            if c2.kmajor:
                rc = lib.gvx_train_gemm_tn(a2.data_ptr(), M, w2.data_ptr(), N, out.t.data_ptr(), N, M, N, K, ws.data_ptr(), n2, _stream())
            else:
                rc = lib.gvx_train_gemm_nt(a2.data_ptr(), K, w2.data_ptr(), K, out.t.data_ptr(), N, M, N, K, b2.data_ptr(), ws.data_ptr(), n2, _stream())
            torch.cuda.synchronize()
            assert rc == 0 and out.border_intact(), (rc, lib.gvx_last_error())
            return {"C": out}
        return run
    c2 = c._replace(M=c.M + 4, N=c.N + 4, K=c.K + 64)
    a2, w2, b2 = make_operands(c2, "rounded", 78)
    n2 = (8 if c.scratch == "full" else c.scratch) * c2.M * c2.N * 4
    hold(dirt, str(c), runner(c, a, w, bias, n), n, (runner(c2, a2, w2, b2, n2), n2))


# ------------------------------------------------------------------------------------------------------------ conv + BatchNorm layer
CONV_NAMES = ["r_1x1_8to8_k3", "t_1x1_24to40_k7", "t_50x2_40to8_k5", "t_5x33_40to8_k7", "sk_103x5_8to40_k5", "sk_12x64_512to512_k5", "sk_23x89_24to24_k5",
              "r_1x257_8to136_k3", "m_1x568_512to80_k5", "big_2x37_512to1536_k9", "norun_7x80_8to24_k3"]


class _DirtyScratch:
    """Stands in for tests/test_conv_train_gpu.py's _Scratch inside run_layer: `saved` and the workspace in arenas, filled by `mode`."""
    mode, left, made = "clean", [], 0

    def __init__(self, nbytes):
        self.nbytes, self.arena = nbytes, Arena(nbytes)
        self.ptr = self.arena.view(nbytes).data_ptr()
        self.slot = _DirtyScratch.made % 2                                   # run_layer makes `saved` first, the workspace second
        _DirtyScratch.made += 1

    def fill_nan(self):
        cls = _DirtyScratch
        if cls.mode == "clean":
            self.arena.view(self.nbytes).zero_()
            return
        self.arena.dirty(self.nbytes)
        if cls.mode == "leftover":
            src = cls.left[self.slot]
            k = min(self.nbytes, src.numel())
            self.arena.view(self.nbytes)[:k] = src[:k]

    def border_intact(self):
        if _DirtyScratch.mode == "record":
            _DirtyScratch.left.append(self.arena.view(self.nbytes).clone())
        return self.arena.intact(self.nbytes)


@pytest.mark.parametrize("dirt", DIRTS)
@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_train_layer(lib, monkeypatch, name, dirt):
    """gvx_conv_bn_act_train_forward / _backward through run_layer of tests/test_conv_train_gpu.py, `saved` and the workspace both in
    arenas of exactly the queried bytes (B T == 1, T below the halo, split-K weight gradients, the two-level map among them).
    Refused short buffers (saved and workspace one byte short): tests/test_host_cpu.py."""
    case = CONV_TRAIN_BY_NAME[name]
    monkeypatch.setattr(tcv, "_Scratch", _DirtyScratch)
    inp = tcv.make_inputs(case)

    def layer(c, inputs, mode):
        _DirtyScratch.mode, _DirtyScratch.made = mode, 0
        got = tcv.run_layer(lib, c, inputs, inputs["dy"])
        assert _DirtyScratch.made == 2, "run_layer no longer makes exactly `saved`, then the workspace: re-aim _DirtyScratch.slot"
        return {k: v for k, v in got.items() if v is not None}
    ref = layer(case, inp, "clean")
    if dirt == "leftover":
        other = case._replace(name=name + "/other", B=case.B + 1, T=case.T + 3)
        _DirtyScratch.left = []
        layer(other, tcv.make_inputs(other), "record")
        assert len(_DirtyScratch.left) == 2 and [x.numel() for x in _DirtyScratch.left] == [
            lib.gvx_conv_train_saved_bytes(other.B, other.Cin, other.Cout, other.T, other.k), lib.gvx_conv_train_workspace_bytes(other.B, other.Cin, other.Cout, other.T, other.k)]
    _same(ref, layer(case, inp, dirt), f"{name} [{dirt}]")


# ------------------------------------------------------------------------------------------------------------ losses, norms
def _loss_run(lib, B, M, T):
    g = torch.Generator().manual_seed(B * T + M)
    dev = [(torch.randn(B, M, T, generator=g) * 3).cuda() for _ in range(2)] + [(torch.randn(B, T, generator=g) * 4).cuda(),
                                                                               (torch.randn(B, M, T, generator=g) * 3).cuda(), (torch.rand(B, T, generator=g) < 0.3).float().cuda()]

    def run(ws, expect=0, ws_bytes=None):
        out = _Out((3,))
        rc = lib.gvx_tacotron2_loss(*(x.data_ptr() for x in dev), B, M, T, out.t.data_ptr(), ws.data_ptr(), 6144 if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        assert rc == expect and out.border_intact(), (rc, lib.gvx_last_error())
        return {"loss": out}
    return run, 6144


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("B,M,T", [(1, 8, 1), (3, 80, 7), (32, 80, 800)])
def test_tacotron2_loss(lib, B, M, T, dirt):
    """gvx_tacotron2_loss on the 6144 bytes the header documents."""
    hold(dirt, f"loss_{B}x{M}x{T}", _loss_run(lib, B, M, T)[0], 6144, _loss_run(lib, B + 1, M, T + 5))


def _guided_run(lib, B, T, L):
    g = torch.Generator().manual_seed(B + 10 * T + 100 * L)
    A = torch.softmax(torch.randn(B, T, L, generator=g), -1).cuda()
    tl = torch.tensor([1 + (i * 5 + L - 1) % L for i in range(B)], dtype=torch.int32).cuda()
    ml = torch.tensor([1 + (i * 3 + T - 1) % T for i in range(B)], dtype=torch.int32).cuda()
    n = lib.gvx_guided_attention_loss_scratch_bytes(B, T, L)

    def run(ws, expect=0, ws_bytes=None):
        o = {"loss": _Out((1,)), "dalign": _Out((B, T, L))}
        rc = lib.gvx_guided_attention_loss(A.data_ptr(), tl.data_ptr(), ml.data_ptr(), B, T, L, 0.4, 2.5, o["loss"].t.data_ptr(), o["dalign"].t.data_ptr(),
                                           ws.data_ptr(), n if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        assert rc == expect and o["loss"].border_intact() and o["dalign"].border_intact(), (rc, lib.gvx_last_error())
        return o
    return run, n


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("B,T,L", [(1, 1, 1), (3, 5, 7), (32, 200, 128), (64, 33, 257)])
def test_guided_attention_loss(lib, B, T, L, dirt):
    run, n = _guided_run(lib, B, T, L)
    hold(dirt, f"guided_{B}x{T}x{L}", run, n, _guided_run(lib, B + 1, T + 2, L + 3))


def _sqnorm_run(lib, n_tensors, seed):
    from tests.test_train_primitives_gpu import SQN_SIZES, _refs
    g = torch.Generator().manual_seed(seed)
    tensors = [torch.randn(SQN_SIZES[(i + n_tensors) % len(SQN_SIZES)], generator=g).cuda() for i in range(n_tensors)]
    refs = _refs([(t.data_ptr(), t.numel()) for t in tensors])
    n = lib.gvx_train_sqnorm_scratch_bytes(n_tensors)

    def run(ws):
        out = torch.full((1 + 2 * 8,), -1.0, dtype=torch.float64, device="cuda")
        rc = lib.gvx_train_sqnorm_many(refs.data_ptr(), n_tensors, ws.data_ptr(), out[8:].data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0 and bool((out[:8] == -1).all()) and bool((out[9:] == -1).all()), (rc, lib.gvx_last_error(), tensors[0].shape)
        return {"sumsq": out[8:9].clone()}
    return run, n


@pytest.mark.parametrize("dirt", DIRTS)
@pytest.mark.parametrize("n_tensors", [1, 10, 48])
def test_sqnorm_many(lib, n_tensors, dirt):
    """gvx_train_sqnorm_many takes no size: the scratch is gvx_train_sqnorm_scratch_bytes(n) bytes and the guards say where it stops."""
    run, n = _sqnorm_run(lib, n_tensors, 5)
    hold(dirt, f"sqnorm_{n_tensors}", run, n, _sqnorm_run(lib, n_tensors + 3, 6))


# ------------------------------------------------------------------------------------------------------------ DTW
def _dtw_run(lib, B, Tp, Tg, K):
    g = torch.Generator().manual_seed(B + Tp + Tg + K)
    cp, cg = torch.randn(B, Tp, K, generator=g).cuda(), torch.randn(B, Tg, K, generator=g).cuda()
    pl = torch.tensor([Tp - (i * 7) % max(1, Tp // 2) for i in range(B)], dtype=torch.int32).cuda()
    tl = torch.tensor([Tg - (i * 5) % max(1, Tg // 2) for i in range(B)], dtype=torch.int32).cuda()
    n = lib.gvx_dtw_workspace_bytes(B, Tp, Tg, K)

    def run(ws, expect=0, ws_bytes=None):
        o = {"dist": _Out((B,)), "acc": _Out((B, Tp, Tg))}
        rc = lib.gvx_dtw_distance(cp.data_ptr(), cg.data_ptr(), pl.data_ptr(), tl.data_ptr(), B, Tp, Tg, K, o["dist"].t.data_ptr(), o["acc"].t.data_ptr(),
                                  ws.data_ptr() if ws is not None else None, (n if ws_bytes is None else ws_bytes) if ws is not None else 0, _stream())
        torch.cuda.synchronize()
        assert rc == expect and o["dist"].border_intact() and o["acc"].border_intact(), (rc, lib.gvx_last_error())
        if not expect:                                                       # acc is written inside each row's rectangle only
            o["acc"] = torch.where(o["acc"].t.view(torch.int32) == tb.SENTINEL, torch.zeros((), device="cuda"), o["acc"].t)
        return o
    return run, n


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
def test_dtw_distance_with_a_workspace(lib, dirt):
    assert lib.gvx_dtw_uses_lds_tables(700, 650, 80) == 0
    run, n = _dtw_run(lib, 3, 700, 650, 80)
    hold(dirt, "dtw_3x700x650x80", run, n, _dtw_run(lib, 4, 500, 800, 80))


def test_dtw_distance_without_a_workspace(lib):
    """The LDS-table form: workspace NULL, size 0; there is no scratch to dirty, two calls give the same bits."""
    assert lib.gvx_dtw_uses_lds_tables(60, 70, 13) == 1 and lib.gvx_dtw_workspace_bytes(3, 60, 70, 13) == 0
    run, _ = _dtw_run(lib, 3, 60, 70, 13)
    ref = run(None)
    _same(ref, run(None), "dtw with its tables in the LDS, second call")


# ------------------------------------------------------------------------------------------------------------ vocoder

def _voc_stages(ap, B, T, seed):
    """Every workspace-taking call of the vocoder on B rows of T frames, straight through the C ABI on one AudioProcessor's plan and
    constants: stage -> (bytes of its size query, run(ws, expect=0, ws_bytes=None) -> outputs in sentinel-bordered buffers)."""
    lib = ap._ensure()
    c = ap.config
    F, hop, M = c.filter_length, c.hop_length, c.n_mels
    bins, n = F // 2 + 1, F + (T - 1) * hop
    g = torch.Generator().manual_seed(seed)
    sig = (torch.randn(B, n, generator=g) * 0.1).cuda()
    spec = torch.randn(B, bins, T, 2, generator=g).cuda()
    mel = (torch.randn(B, M, T, generator=g) - 4.0).cuda()
    mag = torch.rand(B, bins, T, generator=g).cuda()
    lens = torch.tensor([1 + (i * 3 + T - 1) % T for i in range(B)], dtype=torch.int32).cuda()
    bounds = torch.tensor([[0, F + (int(t) - 1) * hop] for t in lens.tolist()], dtype=torch.int32).cuda()
    win, inv, basis, plan, kind, ref = ap._window_dev, ap._inv_basis_dev, ap._mel_basis_dev, ap._plan, ap._log_kind, float(c.ref_level_db)
    # (the header: n_mels = 0 sizes the calls that take no mel; with n_mels the two that do)
    uniform, no_mel, ragged = lib.gvx_gl_workspace_bytes(plan, B, T, M), lib.gvx_gl_workspace_bytes(plan, B, T, 0), lib.gvx_gl_workspace_bytes_ragged(plan, B, T, 0)
    assert 0 < no_mel < uniform
    w2m_ragged = lib.gvx_wav_to_mel_ragged_workspace_bytes(plan, B, n, M)
    assert uniform > 0 and ragged > 0 and w2m_ragged > 0, lib.gvx_last_error()

    def stage(nbytes, shapes, call):
        def run(ws, expect=0, ws_bytes=None):
            o = {k: (_Out(sh) if dt is None else torch.full(sh, -77, dtype=dt, device="cuda")) for k, (sh, dt) in shapes.items()}
            ptr = lambda k: _payload(o[k]).data_ptr()
            rc = call(ptr, ws.data_ptr(), nbytes if ws_bytes is None else ws_bytes)
            torch.cuda.synchronize()
            assert rc == expect, (rc, lib.gvx_last_error())
            for k, x in o.items():
                if isinstance(x, _Out):
                    assert x.border_intact(), k
                elif expect:
                    assert bool((x == -77).all()), f"the refused call wrote to {k}"
            return o
        return nbytes, run
    f = lambda *sh: (sh, None)
    st = _stream()
    return {
        "stft": stage(no_mel, {"spec": f(B, bins, T, 2)}, lambda p, w, nb: lib.gvx_stft(plan, sig.data_ptr(), win.data_ptr(), B, n, p("spec"), w, nb, st)),
        "istft": stage(no_mel, {"wav": f(B, n)}, lambda p, w, nb: lib.gvx_istft(plan, spec.data_ptr(), win.data_ptr(), B, T, p("wav"), w, nb, st)),
        "mel_to_magnitude": stage(uniform, {"mag": f(B, bins, T)},
                                  lambda p, w, nb: lib.gvx_mel_to_magnitude(plan, mel.data_ptr(), inv.data_ptr(), B, M, T, kind, ref, p("mag"), w, nb, st)),
        "wav_to_mel": stage(uniform, {"mel": f(B, M, T)},
                            lambda p, w, nb: lib.gvx_wav_to_mel(plan, sig.data_ptr(), win.data_ptr(), basis.data_ptr(), B, n, M, kind, ref, p("mel"), w, nb, st)),
        "griffin_lim": stage(no_mel, {"phase": f(B, bins, T), "wav": f(B, n)},
                             lambda p, w, nb: lib.gvx_griffin_lim(plan, mag.data_ptr(), win.data_ptr(), B, T, 3, 0.99, p("phase"), p("wav"), w, nb, st)),
        "griffin_lim_ragged": stage(ragged, {"phase": f(B, bins, T), "wav": f(B, n)},
                                    lambda p, w, nb: lib.gvx_griffin_lim_ragged(plan, mag.data_ptr(), win.data_ptr(), B, T, lens.data_ptr(), 3, 0.99, p("phase"),
                                                                                p("wav"), w, nb, st)),
        "wav_to_mel_ragged": stage(w2m_ragged, {"mel": f(B, M, T), "gate": f(B, T), "frames": ((B,), torch.int32), "status": ((B,), torch.int32)},
                                   lambda p, w, nb: lib.gvx_wav_to_mel_ragged(plan, sig.data_ptr(), 1, win.data_ptr(), basis.data_ptr(), B, n, bounds.data_ptr(), 1, M,
                                                                              kind, ref, T, p("mel"), p("gate"), p("frames"), p("status"), w, nb, st)),
    }


VOC_STAGES = ["stft", "istft", "mel_to_magnitude", "wav_to_mel", "griffin_lim", "griffin_lim_ragged", "wav_to_mel_ragged"]
_AP = {}


def _processor(n_fft, hop):
    from tests.test_vocoder_kernels_gpu import processor
    if (n_fft, hop) not in _AP:
        _AP[(n_fft, hop)] = processor(n_fft=n_fft, hop=hop)
        _AP[(n_fft, hop)]._ensure()
    return _AP[(n_fft, hop)]


@pytest.mark.parametrize("dirt", DIRTS + ["short"])
@pytest.mark.parametrize("stage", VOC_STAGES)
@pytest.mark.parametrize("T", [1, 4, 13, 24, 59])
@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (512, 128), (256, 128)])
def test_vocoder_stages(n_fft, hop, T, stage, dirt):
    """gvx_stft, gvx_istft, gvx_mel_to_magnitude, gvx_wav_to_mel, gvx_griffin_lim(_ragged) and gvx_wav_to_mel_ragged (sized by its own
    query) at n_fft 1024 / 256 and 512, T around the workgroup edges of tests/test_vocoder_kernels_gpu.py; leftover: another B and T
    (another B and n_max for gvx_wav_to_mel_ragged) on the same plan; short: one byte less than the stage's own size query."""
    ap = _processor(n_fft, hop)
    B = 3
    n, run = _voc_stages(ap, B, T, 40 + T)[stage]
    ref = hold(dirt, f"voc_{stage}_{n_fft}_{T}", run, n, tuple(reversed(_voc_stages(ap, B + 1, T + 2, 90 + T)[stage])))
    if stage == "wav_to_mel_ragged":
        assert ref["status"].tolist() == [0] * B and ref["frames"].tolist() == [1 + (i * 3 + T - 1) % T for i in range(B)]


def _finalize_run(ap, B, T, ragged, seed):
    lib = ap._ensure()
    c = ap.config
    n = c.filter_length + (T - 1) * c.hop_length
    wav = (torch.randn(B, n, generator=torch.Generator().manual_seed(seed)) * 0.3).cuda()
    lens = torch.tensor([T - (i * 2) % max(1, T - 4) for i in range(B)], dtype=torch.int32).cuda()
    nb = len(ap._b)
    b, a_ = (C.c_double * nb)(*[float(v) for v in ap._b]), (C.c_double * nb)(*[float(v) for v in ap._a])

    def run(ws):
        out = torch.full((B, n - 2 * ap.TRIM), -7.0, dtype=torch.float64, device="cuda")
        rows = (lens.data_ptr(), c.filter_length, c.hop_length) if ragged else ()
        fn = lib.gvx_wav_finalize_ragged if ragged else lib.gvx_wav_finalize
        rc = fn(wav.data_ptr(), B, n, *rows, ap.TRIM, b, a_, nb - 1, out.data_ptr(), ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.gvx_last_error())
        return {"out": out}
    return run, 4 * B


@pytest.mark.parametrize("dirt", DIRTS)
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_wav_finalize_scratch(ragged, dirt):
    """gvx_wav_finalize(_ragged): scratch_B is B uint32 words (no size argument: the guards say where the call stops); leftover: what
    a call on another B left in the words."""
    ap = _processor(1024, 256)
    run, n = _finalize_run(ap, 5, 9, ragged, 3)
    hold(dirt, f"finalize_{ragged}", run, n, _finalize_run(ap, 7, 12, ragged, 4))


# ------------------------------------------------------------------------------------------------------------ the host mirror
class _DirtyEmpty:
    """torch.empty for the length of a scenario: every CUDA tensor it hands out is full of NaN words ("nan") or zeros ("zero"), so
    every workspace, `saved` buffer, scratch and output the mirror allocates starts dirty - the mirror's own clear of a new
    workspace's front runs behind it, as the contract has it."""

    def __init__(self, monkeypatch):
        self.mode, self.real = "zero", torch.empty
        monkeypatch.setattr(torch, "empty", self)

    def __call__(self, *args, **kw):
        t = self.real(*args, **kw)
        if t.is_cuda and t.numel() and t.is_contiguous():
            b = t.view(-1).view(torch.uint8)
            if self.mode == "zero":
                b.zero_()
            else:
                k = b.numel() // 4 * 4
                b[:k].view(torch.int32).fill_(NAN_WORD)
                b[k:] = 0x7F
        return t


def _state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_host_mirror_reuses_dirty_workspaces(monkeypatch):
    """One Tacotron2 instance under NaN-filled allocations - its workspaces (kept and reused across shapes), and every `saved`
    buffer, scratch and output of genvox_amd/training.py - running forward, inference and train_step at three shapes in the order
    A, B, C, B, A.  Every result is bit-equal to a fresh model under zero-filled allocations that starts the call from the same
    weights: the four forward outputs, the inference outputs, and of the training step the loss items, the gradient norm, every
    gradient and every parameter and buffer behind the optimizer step (a new Adam per call on both sides: first-step moments)."""
    from genvox_amd import weights as gw
    from genvox_amd.tacotron2 import Tacotron2
    from tests import train_ref64 as R
    cfgs = fwd_configs("def")
    mc, ac, tc = cfgs
    mc.max_decoder_steps, mc.gate_threshold = 6, 0.5
    sd = gw.generate_state_dict(mc, ac, tc, seed=1, peaky_attention=True)
    alloc = _DirtyEmpty(monkeypatch)

    def model(state):
        m = Tacotron2(mc, ac, tc)
        m.load_state_dict(state)
        return m.to("cuda:0")

    def calls(m, B, L, T):
        inp = gw.synthetic_inputs(B, L, T, tc.n_tokens, ac.n_mels, seed=B + L + T)
        batch = {k: torch.from_numpy(v) for k, v in inp.items()}
        masks = R.draw_masks(mc, ac.n_mels, B, L, T, 300 + B)
        m.eval()
        out = {"fwd_" + k: v.clone() for k, v in m.forward({**batch, "prenet_keep_masks": torch.from_numpy(gw.prenet_keep_masks((T + 1) * B, mc.prenet_dim))}).items() if isinstance(v, torch.Tensor)}
        ar_masks = torch.from_numpy(gw.prenet_keep_masks(6, mc.prenet_dim, seed=2)).reshape(2, 6, 1, mc.prenet_dim)
        ar = m.inference({"tokens": batch["token_padded"][:1], "prenet_keep_masks": ar_masks})
        out.update({"ar_" + k: v.clone() for k, v in ar.items() if isinstance(v, torch.Tensor)})
        m.train_step(R.gpu_batch(batch, masks), m.get_criterion(), m.get_optimizer())
        m.check_status()
        out.update({"loss_" + k: torch.tensor([v], dtype=torch.float64) for k, v in m.loss_items.items()})
        out["grad_norm"] = torch.tensor([m.grad_norm_val], dtype=torch.float64)
        out.update({"grad_" + k: v.detach().cpu().clone() for k, v in m.last_grads.items()})
        out.update({"after_" + k: v for k, v in _state(m).items()})
        return out
    shapes = {"A": (3, 12, 5), "B": (33, 40, 7), "C": (5, 150, 4)}
    alloc.mode = "nan"
    dirty, got = model(sd), []
    for s in "ABCBA":
        before = _state(dirty)
        got.append((s, before, calls(dirty, *shapes[s])))
    alloc.mode = "zero"
    for i, (s, before, g) in enumerate(got):
        _same(calls(model(before), *shapes[s]), g, f"host mirror, call {i} at shape {s}")


def test_audio_processor_reuses_a_dirty_workspace(monkeypatch):
    """One AudioProcessor under NaN-filled allocations (its one workspace, grown as shapes ask and reused between them; scratch_B;
    outputs): mel2wav and wav2mel, padded and ragged forms, at three shapes in the order A, B, C, B, A, each bit-equal to a fresh
    processor under zero-filled allocations."""
    from tests.test_vocoder_kernels_gpu import processor
    alloc = _DirtyEmpty(monkeypatch)

    def calls(ap, B, T):
        c = ap.config
        g = torch.Generator().manual_seed(B * 100 + T)
        mels = (torch.randn(B, c.n_mels, T, generator=g) - 4.0).cuda()
        lens = [T - (i * 3) % max(1, T - 5) for i in range(B)]
        n = c.filter_length + (T - 1) * c.hop_length
        sig = (torch.randn(B, n, generator=g) * 0.1).cuda()
        n_b = [c.filter_length + (t - 1) * c.hop_length for t in lens]
        out = {"mel2wav": ap.convert_mel2wav_batch(mels, n_iter=3)}
        wav_r, samples = ap.convert_mel2wav_batch(mels, n_iter=3, mel_lengths=lens)
        out.update(mel2wav_ragged=wav_r, samples=torch.tensor(samples), wav2mel=ap.wav_to_mel(sig))
        mel_r, frames, gate = ap.wav_to_mel_ragged(sig, sample_lengths=n_b, trim=False, normalize=True)
        out.update(wav2mel_ragged=mel_r, frames=frames, gate=gate)
        torch.cuda.synchronize()
        assert frames.tolist() == lens
        return {k: v.clone() for k, v in out.items()}
    shapes = {"A": (2, 9), "B": (5, 30), "C": (3, 14)}
    alloc.mode = "nan"
    dirty = processor()
    got = [(s, calls(dirty, *shapes[s])) for s in "ABCBA"]
    assert dirty._ws is not None
    alloc.mode = "zero"
    for i, (s, g) in enumerate(got):
        _same(calls(processor(), *shapes[s]), g, f"AudioProcessor, call {i} at shape {s}")
