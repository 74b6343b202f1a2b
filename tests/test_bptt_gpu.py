"""GPU: the two recurrences of the training step's backward as the operations they are - gvx_train_decoder_bptt and
gvx_train_encoder_lstm_bptt(_resident) (genvox_amd/csrc/train_bptt_decoder.hip, train_bptt_encoder.hip) through ctypes, every
direct output against float64 autograd.

The reference here is NOT oracle/train_ref.py: the FORWARD of the operation is written plainly in torch float64 (the decoder loop of
DESIGN.md section 1: attention LSTM cell, location-sensitive attention, decoder LSTM cell; the BiLSTM with packed-sequence
semantics) and autograd differentiates it, so it shares no derivation with the kernels (no `w . (dw_next + G) + dctx . ctx`, no
per-chunk partials, no parity buffers).  Every leaf is an fp32 number; the tape the kernel reads is that float64 forward rounded
once to fp32.

The bound.  With u = 2^-24, a time-major output's step slice (a whole tensor otherwise) must satisfy
max|got - ref| <= TOL[name] * max|ref slice|.  What enters: (1) the rounded tape - the kernel differentiates at pre-activations,
cell states, queries, contexts and alignments that are each up to u off in relative terms, and a gate gradient moves by about that
much times the sensitivity of sigmoid' / tanh' (order 1): a few u per step, growing linearly over the T <= 6 steps of recurrence;
(2) fp32 dot products: length 4A / 4D = 4096 on the MFMA path split over eight waves and two K halves, L and a inside the attention
kernel, E = 512 per position - each about sqrt(K) u of the operands' product in the typical case, against a result that is the
slice's largest entry only for some elements (the bound is relative to the slice's maximum, not per element); (3) fast_tanh =
1 - 2 rcp(__expf(2x) + 1): __expf and rcp are ~1 ulp each, so tanh carries an ABSOLUTE error of about 2 u, which (1 - th^2) and the
products v (1 - th^2) pass on as a relative error of a few u of the largest du.  Together: tens of u.  TOL is 1e-5 (168 u) for
every output but two; the largest error / bound per output that a run met is collected in RATIOS and written as JSON when
GVX_BPTT_REPORT names a file (measured: 0.02 .. 0.65).  The sums over rows and positions (dv, dloc_dense, dloc_conv) add T x B x L
products in fp32, through B x G per-chunk accumulators.  dloc_dense and dloc_conv take 3e-5: their terms (du x locf, dlocf x
weights) have both signs, and at L = 600 their largest entries are 3.5e-2 and 6.4e-2 where the summed magnitudes are far above
that, so the error measured against the result's largest entry reached 1.35e-5 and 1.67e-5 (def_2x600x2); every other case and
output stays below 1e-5.
Where float64 gives a slice of exact zeros the bound above is empty.  That happens at L = 1: a softmax over one position has no
gradient, and every output behind the energies (dq_all, dpm, dv, dloc_dense, dloc_conv) is zero.  The kernel forms the energy
gradient as w (dctx . memory_l + dw_l - s) with s = dctx . ctx + w . dw: two fp32 sums of the same E products in different orders
(a wave's shuffle tree, the workgroup's LDS tree), which cancel up to their rounding.  There the outputs are held to
8 u x max_b sum_e |dctx_e memory_e| x max|v| instead (the forward error of such a sum times the factor v (1 - th^2) <= |v|).

Row independence: every launch of the call is a grid over (something, batch row) - bptt_attention_kernel (chunk, row),
bptt_cells_kernel (units, row), memory_context_grad_kernel (positions, row) - and the products run on skinny_body<1, SK_DEPTH1>
in mode 2, where a batch row is one column of the 32-wide MFMA tile (rows past B read row 0 and are not stored), K is cut evenly
over the waves by the job's k-group count alone and the waves' partial tiles are added in wave order: no summation order depends
on B, so rows 0 .. 4 of a 32-row call are bit-equal to a 5-row call."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from genvox_amd import _lib
from tests.forward_ref import decoder_step, lstm_cell as _lstm_cell   # (the forward both this file and test_forward_loops_gpu.py state once)
from tests.helpers import (BPTT_BY_NAME, BPTT_CASES, BPTT_DEFAULT, BPTT_L_LIMIT, BPTT_ROW_CASES, BPTT_STRIDE_CASES, ENC_BPTT_CASES,
                           bptt_lengths)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 64            # words of sentinel in front of and behind every output (64 floats: the payload stays 256-byte aligned)
TOL = {k: 1e-5 for k in ("dga_all", "dgd_all", "dq_all", "dctx_all", "dpm", "dmemory", "dv", "dloc_dense", "dloc_conv", "dg_pos", "hprev_pos")}
TOL["dloc_dense"] = TOL["dloc_conv"] = 3e-5   # (module docstring: sums of T x B x L products of both signs, against the result's largest entry)
U = 2.0 ** -24
TIME_MAJOR = ("dga_all", "dgd_all", "dq_all", "dctx_all")
DEC_OUTPUTS = ("dga_all", "dgd_all", "dq_all", "dctx_all", "dpm", "dmemory", "dv", "dloc_dense", "dloc_conv")
ROW_OUTPUTS = ("dga_all", "dgd_all", "dq_all", "dctx_all", "dpm", "dmemory")
RATIOS = {}           # output name -> (largest error / bound, case)
ATT_SCALE, DEC_SCALE = 1.25, 2.0


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GVX_BPTT_REPORT")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({k: {"ratio": v[0], "case": v[1]} for k, v in sorted(RATIOS.items())}, f, indent=1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Out:
    """A device buffer with a sentinel border on both sides; `t` is the payload, pre-filled with the sentinel or with finite junk."""

    def __init__(self, shape, junk=False):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        if junk:
            self.t.copy_(torch.linspace(-7.0, 9.0, self.n, device="cuda").view(*shape))

    def border_intact(self):
        w = self.buf.view(torch.int32)
        return bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENTINEL).all())


def _f32(gen, *shape, scale=1.0):
    """A float64 leaf whose values are fp32 numbers."""
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * scale).double()


def _track(x):
    """x with its gradient kept after backward (a leaf when nothing before it asks for gradients)."""
    if not x.requires_grad:
        return x.requires_grad_()
    x.retain_grad()
    return x


# ------------------------------------------------------------------------------------------------------------ decoder loop
_DEC_REF = {}


def decoder_reference(case):
    """float64 forward of the decoder loop + autograd; returns (inputs as fp32 host tensors, expected outputs as float64)."""
    if case.name in _DEC_REF:
        return _DEC_REF[case.name]
    B, L, T = case.B, case.L, case.T
    A, D, E, P, a, Fn, kl = case.sizes
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, case.name)))
    lengths = torch.tensor(bptt_lengths(case.lengths, B, L))
    mask = torch.arange(L)[None, :] >= lengths[:, None]                      # True at and past a row's length
    leaf = lambda *s, scale: _f32(gen, *s, scale=scale).requires_grad_()
    w_ih_a, w_hh_a, b_a = _f32(gen, 4 * A, P + E, scale=1.5 / math.sqrt(P + E)), _f32(gen, 4 * A, A, scale=1.5 / math.sqrt(A)), _f32(gen, 4 * A, scale=0.3)
    w_ih_d, w_hh_d, b_d = _f32(gen, 4 * D, A + E, scale=1.5 / math.sqrt(A + E)), _f32(gen, 4 * D, D, scale=1.5 / math.sqrt(D)), _f32(gen, 4 * D, scale=0.3)
    wq = _f32(gen, a, A, scale=2.0 / math.sqrt(A))
    v = leaf(a, scale=3.0 / math.sqrt(a))
    loc_conv, loc_dense = leaf(Fn, 2, kl, scale=1.0 / math.sqrt(kl)), leaf(a, Fn, scale=1.0 / math.sqrt(Fn))
    pm, memory = leaf(B, L, a, scale=1.0), leaf(B, L, E, scale=1.0)
    x_p = _f32(gen, T, B, P, scale=1.0).clamp_min(0.0)
    dhc = _f32(gen, T, B, D + E, scale=1.0)
    att_keep = (torch.rand(T, B, A, generator=gen) < 0.8)
    dec_keep = (torch.rand(T, B, D, generator=gen) < 0.8)
    att_keep[T // 2, 0] = False                                              # a whole row dropped at one step
    dec_keep[0, B - 1] = False
    W = {"w_ih_a": w_ih_a, "w_hh_a": w_hh_a, "b_a": b_a, "w_ih_d": w_ih_d, "w_hh_d": w_hh_d, "b_d": b_d, "wq": wq, "v": v, "loc_conv": loc_conv,
         "loc_dense": loc_dense}
    z = lambda n: torch.zeros(B, n).double()
    st = {"h_a": z(A), "c_a": z(A), "h_d": z(D), "c_d": z(D), "ctx": z(E), "w": z(L), "wcum": z(L)}
    ga_l, gd_l, q_l, ctx_l, w_l, ca_l, cd_l = [], [], [], [], [], [st["c_a"]], [st["c_d"]]
    loss = 0.0
    for t in range(T):
        r = decoder_step(W, st, x_p[t], memory, pm, mask, att_keep[t].double() * ATT_SCALE, dec_keep[t].double() * DEC_SCALE, track=_track)
        loss = loss + (dhc[t] * torch.cat((r["h_d"], r["ctx"]), 1)).sum()
        ga_l.append(r["ga"]); gd_l.append(r["gd"]); q_l.append(r["q"]); ctx_l.append(r["ctx"]); w_l.append(r["w"]); ca_l.append(r["c_a"]); cd_l.append(r["c_d"])
    loss.backward()
    st = lambda xs: torch.stack([x.detach() for x in xs])
    unit_major = lambda g, H: g.detach().reshape(B, 4, H).permute(0, 2, 1)                    # [B][H][4]: unit-major, gate-minor
    w_all = st(w_l)
    assert bool((w_all[:, mask] == 0).all())
    inputs = {
        "dhc_all": dhc, "pre_a": torch.stack([unit_major(g, A) for g in ga_l]), "pre_d": torch.stack([unit_major(g, D) for g in gd_l]),
        "c_a_all": st(ca_l), "c_d_all": st(cd_l), "q_all": st(q_l), "ctx_all": st(ctx_l), "w_all": w_all,
        "memory": memory.detach(), "pm": pm.detach(), "w_ih_a": w_ih_a, "w_hh_a": w_hh_a, "w_ih_d": w_ih_d, "w_hh_d": w_hh_d, "wq": wq,
        "v": v.detach(), "loc_conv": loc_conv.detach(), "loc_dense": loc_dense.detach()}
    inputs = {k: x.float().contiguous() for k, x in inputs.items()}
    inputs["att_keep"], inputs["dec_keep"] = att_keep.to(torch.uint8).contiguous(), dec_keep.to(torch.uint8).contiguous()
    want = {"dga_all": st([g.grad for g in ga_l]), "dgd_all": st([g.grad for g in gd_l]), "dq_all": st([g.grad for g in q_l]),
            "dctx_all": st([g.grad for g in ctx_l]), "dpm": pm.grad, "dmemory": memory.grad, "dv": v.grad, "dloc_dense": loc_dense.grad,
            "dloc_conv": loc_conv.grad}
    _DEC_REF[case.name] = (inputs, want, lengths, mask)
    return _DEC_REF[case.name]


def _dec_shapes(B, L, T, sizes):
    A, D, E, P, a, Fn, kl = sizes
    return {"dga_all": (T, B, 4 * A), "dgd_all": (T, B, 4 * D), "dq_all": (T, B, a), "dctx_all": (T, B, E), "dpm": (B, L, a), "dmemory": (B, L, E),
            "dv": (a,), "dloc_dense": (a, Fn), "dloc_conv": (Fn, 2, kl)}


def _junk_workspace(nbytes, slack):
    """nbytes of finite junk with `slack` words of sentinel behind them (_slack_intact)."""
    ws = torch.linspace(-3.0, 5.0, nbytes // 4 + slack, device="cuda")
    ws.view(torch.int32)[nbytes // 4:] = SENTINEL
    return ws


def _slack_intact(ws, nbytes):
    return bool((ws.view(torch.int32).flatten()[nbytes // 4:] == SENTINEL).all())


def run_decoder(lib, B, L, T, sizes, inputs, dense_ctx=True, expect=0, ws_mutate=None, args_mutate=None, ws=None, dw_ext=None):
    """One gvx_train_decoder_bptt call.  ctx_all goes in as a dense [T][B][E] array (dense_ctx) or as the columns D .. D + E of a
    [T][B][D + E] array, the layout of the training forward's tape.  dpm and the workspace are handed over full of finite junk.
    ws: a workspace of the caller's (a byte tensor of at least the queried size) in place of the junk-filled one.  dw_ext [T][B][L]:
    the call goes through gvx_train_decoder_bptt_ext with that gradient on the alignments.
    Returns (status, outputs as {name: _Out}, workspace bytes the size query gave)."""
    A, D, E, P, a, Fn, kl = sizes
    dev = {k: x.cuda() for k, x in inputs.items()}
    outs = {k: _Out(s, junk=(k == "dpm")) for k, s in _dec_shapes(B, L, T, sizes).items()}
    args = _lib.gvx_bptt_decoder_args()
    args.B, args.L, args.T, args.A, args.D, args.E, args.P, args.a, args.F, args.kl = B, L, T, A, D, E, P, a, Fn, kl
    args.att_scale, args.dec_scale = ATT_SCALE, DEC_SCALE
    for k in ("dhc_all", "pre_a", "pre_d", "c_a_all", "c_d_all", "att_keep", "dec_keep", "q_all", "w_all", "memory", "pm", "w_ih_a", "w_hh_a",
              "w_ih_d", "w_hh_d", "wq", "v", "loc_conv", "loc_dense"):
        setattr(args, k, dev[k].data_ptr())
    if dense_ctx:
        args.ctx_all, args.ctx_ts, args.ctx_bs = dev["ctx_all"].data_ptr(), B * E, E
    else:
        hc = torch.full((T, B, D + E), float("nan"), device="cuda")        # (the h_d columns are not the call's to read)
        hc[:, :, D:] = dev["ctx_all"]
        dev["hc"] = hc
        args.ctx_all, args.ctx_ts, args.ctx_bs = hc.data_ptr() + 4 * D, B * (D + E), D + E
    for k, o in outs.items():
        setattr(args, k, o.t.data_ptr())
    ap = C.byref(args)
    if args_mutate is not None and args_mutate(args) is False:
        ap = None                                                            # (a NULL argument block)
    wsb = lib.gvx_train_decoder_bptt_workspace_bytes(ap)
    ws_n = max(wsb, 256)
    if ws is None:
        ws = _junk_workspace(ws_n, 128)                                      # finite junk: the call clears what it accumulates into
    ws_ptr, ws_bytes = ws.data_ptr(), wsb
    if ws_mutate:
        ws_ptr, ws_bytes = ws_mutate(ws_ptr, wsb)
    if dw_ext is None:
        rc = lib.gvx_train_decoder_bptt(ap, ws_ptr, ws_bytes, _stream())
    else:
        dw_dev = dw_ext.cuda()
        rc = lib.gvx_train_decoder_bptt_ext(ap, dw_dev.data_ptr(), B * L, L, ws_ptr, ws_bytes, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.gvx_last_error())
    assert _slack_intact(ws, ws_n), "the call wrote behind its workspace"
    return rc, outs, wsb


def _compare(name, got, want, case_name, slices, zero_floor=0.0):
    """max|got - ref| of every slice against TOL[name] x the slice's largest |ref|; the largest ratio goes into RATIOS.  A slice
    of exact zeros in float64 must be within zero_floor (module docstring)."""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    parts = [(got[t], want[t], f"{name}[{t}]") for t in range(got.shape[0])] if slices else [(got, want, name)]
    for g, w, label in parts:
        scale = float(w.abs().max())
        err = float((g - w).abs().max())
        bound = TOL[name] * scale
        if scale == 0.0:
            assert err <= zero_floor, (case_name, label, err, zero_floor)
            continue
        ratio = err / bound
        if ratio > RATIOS.get(name, (0.0, ""))[0]:
            RATIOS[name] = (ratio, case_name)
        if ratio > 1.0:
            idx = np.unravel_index(int((g - w).abs().argmax()), tuple(g.shape))
            raise AssertionError(f"{case_name}: {label} differs from float64 by {err:.3e} at {idx} (got {float(g[idx]):.6e}, want {float(w[idx]):.6e}), "
                                 f"bound {bound:.3e} = {TOL[name]} x {scale:.3e}")


@pytest.mark.parametrize("case", BPTT_CASES, ids=lambda c: c.name)
def test_decoder_bptt_against_float64_autograd(lib, case):
    """Every output of the call against autograd of the float64 forward (module docstring: the bound), with: sentinel borders round
    every output, dpm and the workspace full of junk on entry, exact zeros of dpm / dmemory past a row's length, a second call
    bit-equal to the first ("deterministic, no atomics"), and junk in memory / pm past the length changing no bit."""
    inputs, want, lengths, mask = decoder_reference(case)
    _, outs, wsb = run_decoder(lib, case.B, case.L, case.T, case.sizes, inputs)
    assert wsb > 0
    got = {k: o.t.clone() for k, o in outs.items()}
    for k, o in outs.items():
        assert o.border_intact(), f"{case.name}: the call wrote outside {k}"
        assert bool(torch.isfinite(o.t).all()), f"{case.name}: {k} is not finite"
    floor = 0.0
    if case.L == 1:   # (softmax over one position: module docstring)
        floor = 8 * U * float((want["dctx_all"].abs() * inputs["memory"][:, 0].double().abs()[None]).sum(-1).max()) * float(inputs["v"].abs().max())
    for k in DEC_OUTPUTS:
        _compare(k, got[k], want[k], case.name, k in TIME_MAJOR, zero_floor=floor if k in ("dq_all", "dpm", "dv", "dloc_dense", "dloc_conv") else 0.0)
    m = mask.cuda()
    assert bool((got["dpm"][m] == 0).all()) and bool((got["dmemory"][m] == 0).all()), f"{case.name}: gradient past a row's length"
    # (float64 agrees: a padded position has zero weight at every step)
    assert bool((want["dpm"][mask] == 0).all()) and bool((want["dmemory"][mask] == 0).all())
    _, again, _ = run_decoder(lib, case.B, case.L, case.T, case.sizes, inputs)
    for k in DEC_OUTPUTS:
        assert torch.equal(again[k].t, got[k]), f"{case.name}: {k} differs between two identical calls"
    if bool(mask.any()):
        junk = dict(inputs)
        for k in ("memory", "pm"):
            x = inputs[k].clone()
            x[mask] = torch.linspace(-50.0, 60.0, int(mask.sum()) * x.shape[2]).view(-1, x.shape[2])
            junk[k] = x
        _, jo, _ = run_decoder(lib, case.B, case.L, case.T, case.sizes, junk)
        for k in DEC_OUTPUTS:
            assert torch.equal(jo[k].t, got[k]), f"{case.name}: {k} depends on memory / pm past a row's length"


@pytest.mark.parametrize("name", BPTT_STRIDE_CASES)
def test_decoder_bptt_context_strides(lib, name):
    """ctx_all is read through ctx_ts / ctx_bs: the columns D .. D + E of a [T][B][D + E] array (the tape's layout; NaN in the other
    columns) give the bits of the dense [T][B][E] copy."""
    case = BPTT_BY_NAME[name]
    inputs = decoder_reference(case)[0]
    _, dense, _ = run_decoder(lib, case.B, case.L, case.T, case.sizes, inputs, dense_ctx=True)
    _, strided, _ = run_decoder(lib, case.B, case.L, case.T, case.sizes, inputs, dense_ctx=False)
    for k in DEC_OUTPUTS:
        assert strided[k].border_intact() and torch.equal(dense[k].t, strided[k].t), (name, k)


@pytest.mark.parametrize("name", BPTT_ROW_CASES)
def test_decoder_bptt_rows_do_not_depend_on_the_batch(lib, name):
    """Rows 0 .. 4 of a 32-row call, recomputed as a 5-row call on those rows' tape: the per-row outputs are bit-equal (module
    docstring: no summation order of the call depends on B).  dv / dloc_dense / dloc_conv are sums over rows: float64 only."""
    case = BPTT_BY_NAME[name]
    assert case.B == 32
    inputs, want, _, _ = decoder_reference(case)
    _, big, _ = run_decoder(lib, case.B, case.L, case.T, case.sizes, inputs)
    R = 5
    sub = {}
    for k, x in inputs.items():
        if k in ("dhc_all", "pre_a", "pre_d", "c_a_all", "c_d_all", "q_all", "ctx_all", "w_all", "att_keep", "dec_keep"):
            sub[k] = x[:, :R].contiguous()
        elif k in ("memory", "pm"):
            sub[k] = x[:R].contiguous()
        else:
            sub[k] = x
    _, small, _ = run_decoder(lib, R, case.L, case.T, case.sizes, sub)
    for k in ROW_OUTPUTS:
        b = big[k].t[:, :R] if k in TIME_MAJOR else big[k].t[:R]
        assert torch.equal(b, small[k].t), f"{name}: {k} of rows 0..{R - 1} depends on the batch ({float((b - small[k].t).abs().max()):.3e})"


_SMALL = BPTT_BY_NAME["odd_L9"]


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


@pytest.mark.parametrize("what,mutate,code", [
    ("B = 0", _set(B=0), -2), ("B = 33", _set(B=33), -2), ("T = 0", _set(T=0), -2), ("L = 0", _set(L=0), -2),
    ("A % 8", _set(A=44), -2), ("D % 8", _set(D=60), -2), ("a = 257", _set(a=257), -2), ("F = 33", _set(F=33), -2), ("even kl", _set(kl=4), -2),
    ("L past the LDS limit", _set(L=BPTT_L_LIMIT + 1, A=1024, D=1024, E=512, P=256, a=128, F=32, kl=31), -2),
] + [("NULL " + n, _set(**{n: None}), -1) for n, t in _lib.gvx_bptt_decoder_args._fields_ if t is C.c_void_p])
def test_decoder_bptt_refusals_leave_every_output_untouched(lib, what, mutate, code):
    """A refused argument block: the status, a message in gvx_last_error, 0 from the size query, and not one word of any output
    written (the sizes in the block are never trusted before they are checked: the buffers are those of the small valid case)."""
    inputs = decoder_reference(_SMALL)[0]
    rc, outs, wsb = run_decoder(lib, _SMALL.B, _SMALL.L, _SMALL.T, _SMALL.sizes, inputs, expect=code, args_mutate=mutate)
    assert wsb == 0 and lib.gvx_last_error(), what
    for k, o in outs.items():
        if k != "dpm":
            assert o.untouched(), f"{what}: {k} was written"
    assert outs["dpm"].border_intact() and torch.equal(outs["dpm"].t, _Out(outs["dpm"].t.shape, junk=True).t), what


def test_decoder_bptt_refuses_bad_workspaces_and_a_null_block(lib):
    inputs = decoder_reference(_SMALL)[0]
    for what, mut in (("one byte short", lambda p, n: (p, n - 1)), ("not 256-byte aligned", lambda p, n: (p + 4, n)), ("NULL", lambda p, n: (None, n))):
        rc, outs, wsb = run_decoder(lib, _SMALL.B, _SMALL.L, _SMALL.T, _SMALL.sizes, inputs, expect=-5, ws_mutate=mut)
        assert wsb > 0 and b"workspace" in lib.gvx_last_error(), what
        assert all(o.untouched() for k, o in outs.items() if k != "dpm") and outs["dpm"].border_intact(), what
    rc, outs, wsb = run_decoder(lib, _SMALL.B, _SMALL.L, _SMALL.T, _SMALL.sizes, inputs, expect=-1, args_mutate=lambda a: False)
    assert wsb == 0 and b"null argument block" in lib.gvx_last_error()
    assert all(o.untouched() for k, o in outs.items() if k != "dpm")


# ------------------------------------------------------------------------------------------------------------ encoder walk
_ENC_REF = {}


def encoder_reference(case):
    """float64 BiLSTM with packed-sequence semantics + autograd of sum(dmemory * memory)."""
    if case.name in _ENC_REF:
        return _ENC_REF[case.name]
    B, L, H = case.B, case.L, case.H
    gen = torch.Generator().manual_seed(2000 + sum(map(ord, case.name)))
    lengths = torch.tensor(bptt_lengths(case.lengths, B, L))
    xg = _f32(gen, 2, B, L, 4 * H, scale=1.0)
    w_hh = _f32(gen, 2, 4 * H, H, scale=1.5 / math.sqrt(H))
    dmem = _f32(gen, B, L, 2 * H, scale=1.0)
    rows = torch.arange(B)
    mem, cst = [], []
    gates_l = [[], []]                                                      # per direction: (gates, position per row, active rows)
    hprev = torch.zeros(2, B, L, H).double()
    for d in range(2):
        h, c = torch.zeros(B, H).double(), torch.zeros(B, H).double()
        m_d, c_d = torch.zeros(B, L, H).double(), torch.zeros(B, L, H).double()
        for s in range(L):
            active = s < lengths
            pos = torch.full((B,), s) if d == 0 else (lengths - 1 - s).clamp_min(0)
            g = _track(xg[d][rows, pos] + h @ w_hh[d].t())
            hn, cn = _lstm_cell(g, c)
            ar, ap = rows[active], pos[active]
            hprev[d].index_put_((ar, ap), h.detach()[active])
            h = torch.where(active[:, None], hn, h)
            c = torch.where(active[:, None], cn, c)
            m_d = m_d.index_put((ar, ap), hn[active])
            c_d = c_d.index_put((ar, ap), cn.detach()[active])
            gates_l[d].append((g, ar, ap))
        mem.append(m_d); cst.append(c_d)
    memory = torch.cat(mem, 2)
    (dmem * memory).sum().backward()
    dg = torch.zeros(2, B, L, 4 * H).double()
    for d in range(2):
        for g, ar, ap in gates_l[d]:
            if len(ar):
                dg[d].index_put_((ar, ap), g.grad[ar])
    inputs = {"xg": xg.float().contiguous(), "memory": memory.detach().float().contiguous(), "cell_states": torch.cat(cst, 2).float().contiguous(),
              "dmemory": dmem.float().contiguous(), "w_hh": w_hh.float().contiguous(), "lengths": lengths.to(torch.int32)}
    _ENC_REF[case.name] = (inputs, {"dg_pos": dg, "hprev_pos": hprev}, lengths)
    return _ENC_REF[case.name]


def run_encoder(lib, case, inputs, resident, expect=0, B=None, L=None, H=None, short_ws=0, ws=None):
    B0, L0, H0 = case.B, case.L, case.H
    dev = {k: x.cuda() for k, x in inputs.items()}
    outs = {"dg_pos": _Out((2, B0, L0, 4 * H0)), "hprev_pos": _Out((2, B0, L0, H0))}
    wsb = lib.gvx_train_encoder_lstm_bptt_workspace_bytes(B0, H0)
    assert wsb > 0
    if ws is None:
        ws = _junk_workspace(wsb, 64)
    fn = lib.gvx_train_encoder_lstm_bptt_resident if resident else lib.gvx_train_encoder_lstm_bptt
    rc = fn(dev["xg"].data_ptr(), dev["memory"].data_ptr(), dev["cell_states"].data_ptr(), dev["dmemory"].data_ptr(), dev["w_hh"].data_ptr(),
            dev["lengths"].data_ptr(), B0 if B is None else B, L0 if L is None else L, H0 if H is None else H, outs["dg_pos"].t.data_ptr(),
            outs["hprev_pos"].t.data_ptr(), ws.data_ptr(), wsb - short_ws, _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.gvx_last_error())
    assert _slack_intact(ws, wsb), "the call wrote behind its workspace"
    if rc == 0:
        code = C.c_int(-1)
        assert lib.gvx_train_encoder_lstm_bptt_status(ws.data_ptr(), wsb, B0, H0, C.byref(code), _stream()) == 0 and code.value == 0, code.value
    return outs


@pytest.mark.parametrize("case", ENC_BPTT_CASES, ids=lambda c: c.name)
def test_encoder_bptt_against_float64_autograd(lib, case):
    """Both entry points against autograd of the float64 BiLSTM: dg_pos per tensor and direction, hprev_pos (a copy of the tape: it
    must equal the fp32 memory of the previous position exactly); exact zeros past a row's length and, for hprev_pos, at each
    direction's first step; sentinel borders; the workspace full of junk; a status word of 0; two identical calls and the two
    entry points bit-equal (the resident walk does the launch-per-step walk's arithmetic in its order); junk in every input past
    a row's length changes no bit."""
    inputs, want, lengths = encoder_reference(case)
    B, L, H = case.B, case.L, case.H
    pad = (torch.arange(L)[None, :] >= lengths[:, None])
    got = {}
    for resident in (True, False):
        outs = run_encoder(lib, case, inputs, resident)
        for k, o in outs.items():
            assert o.border_intact() and bool(torch.isfinite(o.t).all()), (case.name, resident, k)
        got[resident] = {k: o.t.clone() for k, o in outs.items()}
        again = run_encoder(lib, case, inputs, resident)
        for k in outs:
            assert torch.equal(again[k].t, got[resident][k]), f"{case.name}: {k} differs between two identical calls (resident={resident})"
    for k in ("dg_pos", "hprev_pos"):
        assert torch.equal(got[True][k], got[False][k]), f"{case.name}: {k} differs between the resident walk and the launch per step"
    g = got[True]
    _compare("dg_pos", g["dg_pos"], want["dg_pos"], case.name + "/enc", True)
    # hprev_pos is the fp32 tape itself, moved by one position
    mem = inputs["memory"]
    exp_h = torch.zeros(2, B, L, H)
    exp_h[0, :, 1:] = mem[:, :-1, :H]
    exp_h[1, :, :-1] = mem[:, 1:, H:]
    exp_h[:, pad] = 0
    exp_h[1, torch.arange(B), lengths - 1] = 0                               # the reverse direction starts at each row's last token
    assert torch.equal(g["hprev_pos"].cpu(), exp_h), case.name
    _compare("hprev_pos", g["hprev_pos"], want["hprev_pos"], case.name + "/enc", True)
    padc = pad.cuda()
    assert bool((g["dg_pos"][:, padc] == 0).all()) and bool((g["hprev_pos"][:, padc] == 0).all()), case.name
    assert bool((g["hprev_pos"][0, :, 0] == 0).all()), case.name
    if bool(pad.any()):
        junk = dict(inputs)
        for k in ("memory", "cell_states", "dmemory"):
            x = inputs[k].clone(); x[pad] = 37.5; junk[k] = x
        x = inputs["xg"].clone(); x[:, pad] = -11.25; junk["xg"] = x
        jo = run_encoder(lib, case, junk, True)
        for k in jo:
            assert torch.equal(jo[k].t, g[k]), f"{case.name}: {k} depends on inputs past a row's length"


@pytest.mark.parametrize("resident", [True, False])
def test_encoder_bptt_refusals_leave_the_outputs_untouched(lib, resident):
    case = ENC_BPTT_CASES[3]
    inputs = encoder_reference(case)[0]
    for what, kw, code in (("H = 12", dict(H=12), -2), ("H = 0", dict(H=0), -2), ("L = 0", dict(L=0), -2), ("B = 0", dict(B=0), -2),
                           ("workspace one byte short", dict(short_ws=1), -5)):
        outs = run_encoder(lib, case, inputs, resident, expect=code, **kw)
        assert lib.gvx_last_error() and all(o.untouched() for o in outs.values()), what


def test_training_mode_is_refused_on_the_64_row_loop(lib, monkeypatch):
    """A handle created under GVX_TF_ROWS64=1 runs 33 .. 64 rows on the 64-row loop, which wires neither the hidden-state dropout
    nor the tape: gvx_decoder_teacher_forced_train must refuse such a call (GVX_ERR_UNSUPPORTED, outputs and tape untouched)
    instead of returning an inference-mode result.  32 rows on the same handle still run."""
    from genvox_amd import weights as gw
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
    from genvox_amd.tacotron2 import Tacotron2

    mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024, log_func="np.log"), TextConfig(n_tokens=40)
    sd = gw.generate_state_dict(mc, ac, tc, seed=1)
    A, D, E, P, M = mc.attention_rnn_dim, mc.decoder_rnn_dim, mc.encoder_embedding_dim, mc.prenet_dim, ac.n_mels
    L, T = 12, 3

    def call(model, B):
        ws = model._get_workspace(B, L, T)
        g = torch.Generator().manual_seed(B)
        memory = torch.randn(B, L, E, generator=g).cuda()
        lengths = torch.full((B,), L, dtype=torch.int32).cuda()
        mel_in = torch.randn(B, M, T, generator=g).cuda()
        masks = (torch.rand(2, T + 1, B, P, generator=g) < 0.5).to(torch.uint8).cuda()
        ak, dk = (torch.rand(T, B, A, generator=g) < 0.9).to(torch.uint8).cuda(), (torch.rand(T, B, D, generator=g) < 0.9).to(torch.uint8).cuda()
        outs = [_Out(s) for s in ((B, M, T), (B, T), (B, T, L), ((T + 1) * B * A,), (T + 1, B, A), (T + 1, B, D), ((T + 1) * B * (D + E),),
                                  (T, B, A, 4), (T, B, D, 4))]
        rc = lib.gvx_decoder_teacher_forced_train(model._handle, memory.data_ptr(), lengths.data_ptr(), B, L, mel_in.data_ptr(), T, masks.data_ptr(),
                                                  ak.data_ptr(), dk.data_ptr(), 0.1, 0.1, *[o.t.data_ptr() for o in outs], ws.data_ptr(), ws.numel(),
                                                  _stream())
        torch.cuda.synchronize()
        return rc, outs

    monkeypatch.setenv("GVX_TF_ROWS64", "1")
    m64 = Tacotron2(mc, ac, tc)
    m64.load_state_dict(sd)
    m64 = m64.to("cuda:0")
    m64._ensure_packed()                                                     # (the handle reads its settings when it is created)
    monkeypatch.delenv("GVX_TF_ROWS64")
    if lib.gvx_teacher_forced_rows_per_call(m64._handle, L) != 64:
        pytest.fail("the GVX_TF_ROWS64 handle does not plan 64 rows per call: the refusal below would not be reached")
    rc, outs = call(m64, 40)
    assert rc == -2 and b"64-row loop" in lib.gvx_last_error(), (rc, lib.gvx_last_error())
    assert all(o.untouched() for o in outs), "a refused training call wrote into its outputs"
    rc, outs = call(m64, 32)
    assert rc == 0 and all(o.border_intact() and bool(torch.isfinite(o.t).all()) for o in outs), lib.gvx_last_error()
