"""CPU: the monotonic attention window of the autoregressive decode - its float64 reference worked by hand, the condition under
which the GPU test may demand exact centres, the plan a windowed call takes, and the argument checks that need no GPU.

CENTRE_MARGIN.  tests/test_attention_window_gpu.py asserts centres_out EXACTLY, no step left out.  A centre is an argmax, so
that is safe only where the float64 reference's largest weight inside the window beats the second largest by much more than the
GPU's alignment error.  That error was measured as the largest |align_gpu - align_float64| over the un-windowed AR_CASES_FWD
cases (tests/helpers.py) on the commit before the window existed, per weight set:

    plain   1.952e-07        peaky   9.105e-06

CENTRE_MARGIN is 100 times that - two orders of magnitude, because inside a window the error re-normalises over fewer positions:

    plain   1.952e-05        peaky   9.105e-04

Every (case, weight set) of tests/attention_window_cases.py must have centre_margin >= CENTRE_MARGIN of its weight set
(test_centre_margins_allow_exact_centres); a case that does not is replaced, never skipped.  (EXPERIMENTS.md, "Attention window",
holds both tables and the cases' margins.)
"""
import ctypes as C
import math

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.tacotron2 import Tacotron2, dims_from_configs
from tests import forward_ref as fr
from tests import forward_window_ref64 as fw
from tests.attention_window_cases import WINDOW_CASES, inputs, reference, state_dict
from tests.helpers import AR_CASES_FWD, create_handle, decoder_plan, fwd_configs

ALIGN_ERROR = {"plain": 1.952e-7, "peaky": 9.105e-6}
CENTRE_MARGIN = {k: 100.0 * v for k, v in ALIGN_ERROR.items()}
NEG = float("-inf")


def _e(*rows):
    return torch.tensor(rows, dtype=torch.float64)


def _pad(lengths, L=6):
    return fr.pad_mask(lengths, L)


# ---------------------------------------------------------------------------------------------------- the reference, by hand
def test_window_by_hand_energy_sequence():
    """L = 6, one row of 5 tokens, window (1, 2), a hand-made energy sequence.  Step 0: centre 0 -> positions 0..2 (the left edge
    cuts the window at 0).  exp(0), exp(ln 3), exp(0) -> weights 1/5, 3/5, 1/5, next centre 1."""
    e0 = _e([0.0, math.log(3.0), 0.0, 50.0, 50.0, 50.0])     # the 50s are outside the window / past the length
    w, c, gap = fw.softmax_window_step(e0, _pad([5]), [0], 1, 2)
    assert torch.allclose(w, _e([0.2, 0.6, 0.2, 0.0, 0.0, 0.0]), rtol=0, atol=1e-15) and c.tolist() == [1]
    assert bool((w[0, 3:] == 0).all())
    assert abs(float(gap) - 0.4) < 1e-15
    # step 1: centre 1 -> positions 0..3; equal energies -> 1/4 each, the tie goes to the LOWEST index: centre 0 (it moved back by 1)
    w, c, gap = fw.softmax_window_step(_e([2.0, 2.0, 2.0, 2.0, 9.0, 9.0]), _pad([5]), [1], 1, 2)
    assert w.tolist() == [[0.25, 0.25, 0.25, 0.25, 0.0, 0.0]] and c.tolist() == [0] and float(gap) == 0.0
    # step 2: centre 3 -> positions 2..5, but the row has 5 tokens: 2..4.  The largest energy inside is at 4 = len - 1
    w, c, _ = fw.softmax_window_step(_e([9.0, 9.0, 0.0, 0.0, 1.0, 9.0]), _pad([5]), [3], 1, 2)
    z = 2.0 + math.e
    assert torch.allclose(w, _e([0.0, 0.0, 1 / z, 1 / z, math.e / z, 0.0]), rtol=0, atol=1e-15)
    assert c.tolist() == [4] and float(w[0, 5]) == 0.0 and float(w[0, :2].sum()) == 0.0
    # step 3: centre 4 = len - 1, ahead reaches past the length: positions 3..4 only
    w, c, _ = fw.softmax_window_step(_e([0.0, 0.0, 0.0, 1.0, 1.0, 7.0]), _pad([5]), [4], 1, 2)
    assert w.tolist() == [[0.0, 0.0, 0.0, 0.5, 0.5, 0.0]] and c.tolist() == [3]


def test_window_by_hand_back_zero_never_moves_back():
    """back = 0: nothing before the centre takes part, whatever its energy; (0, 0) keeps the centre where it is with weight 1."""
    e = _e([100.0, 100.0, 0.0, 1.0, -1.0, 100.0])
    w, c, _ = fw.softmax_window_step(e, _pad([6]), [2], 0, 1)
    assert bool((w[0, :2] == 0).all()) and bool((w[0, 4:] == 0).all()) and c.tolist() == [3]
    w, c, gap = fw.softmax_window_step(e, _pad([6]), [2], 0, 0)
    assert w.tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0, 0.0]] and c.tolist() == [2] and float(gap) == float("inf")


def test_window_by_hand_rows_are_independent_and_never_empty():
    """Two rows with centres of their own; a row of one token has a window of one position at every centre it can have."""
    e = _e([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [7.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    w, c, _ = fw.softmax_window_step(e, _pad([6, 1]), [5, 0], 3, 10)
    assert c.tolist() == [5, 0] and w[1].tolist() == [1.0, 0, 0, 0, 0, 0] and bool((w[0, :2] == 0).all())
    assert torch.allclose(w.sum(1), torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-15)
    assert fw.outside_window([0, 5], 1, 2, 6).tolist() == [[False, False, False, True, True, True], [True, True, True, True, False, False]]
    assert fw.first_argmax(_e([0.1, 0.4, 0.4, 0.1], [0.25, 0.25, 0.25, 0.25])).tolist() == [1, 0]


def test_a_window_over_the_whole_row_is_the_plain_decode():
    """back, ahead >= L: the mask is the length mask, and the windowed reference equals forward_ref.autoregressive exactly."""
    case = next(c for c in WINDOW_CASES if c.name == "w0_small_5x13")
    for wname in ("plain", "peaky"):
        inp = inputs(case, wname)
        W = fr.decoder_weights(state_dict(case.dims, wname))
        lengths = inp["lengths"].tolist()
        plain = fr.autoregressive(W, inp["memory"].double(), lengths, case.T, 0.6, inp["keep"])
        wide = fw.autoregressive_windowed(W, inp["memory"].double(), lengths, case.T, 0.6, inp["keep"], case.L, case.L)
        for k in ("mel_out", "gate_out", "align_out", "n_frames", "w", "ctx", "mel", "gate"):
            assert torch.equal(plain[k], wide[k]), k
        assert plain["margin"] == wide["margin"]
        live = torch.arange(case.T)[None, :] < wide["n_frames"][:, None]
        assert torch.equal(wide["centres"][live], plain["align_out"].argmax(-1)[live]) and bool((wide["centres"][~live] == -1).all())


def test_reference_centres_obey_the_window():
    """The definition's consequences on a real decode: the centre moves by at most max(back, ahead) per step, never back with
    back = 0, stays below the row's length, and the weights outside every step's window are exactly 0."""
    for case in WINDOW_CASES:
        if case.dims != "small" and case.B * case.L > 700:
            continue
        back, ahead = case.window
        inp, want, _ = reference(case, "plain")
        lengths = inp["lengths"]
        c = want["centres"]
        for b in range(case.B):
            n = int(want["n_frames"][b])
            seq = [0] + c[b, :n].tolist()
            assert all(0 <= v < int(lengths[b]) for v in seq), case.name
            assert all(-back <= y - x <= ahead for x, y in zip(seq, seq[1:])), (case.name, b, seq)
            for t in range(n):
                w = want["align_out"][b, t]
                lo, hi = seq[t] - back, seq[t] + ahead
                assert float(w[:max(lo, 0)].sum()) == 0.0 and float(w[hi + 1:].sum()) == 0.0


# ---------------------------------------------------------------------------------------------------- the GPU test's condition
@pytest.mark.parametrize("case", WINDOW_CASES, ids=lambda c: c.name)
def test_centre_margins_allow_exact_centres(case):
    for wname in case.wsets:
        _, want, _ = reference(case, wname)
        assert want["centre_margin"] >= CENTRE_MARGIN[wname], (case.name, wname, want["centre_margin"])
        assert want["margin"] > 1e-3, (case.name, wname, want["margin"])     # (stop steps: as tests/test_forward_loops_gpu.py)


def test_window_cases_cover_what_the_issue_lists():
    assert {(0, 1), (1, 3), (3, 10)} <= {c.window for c in WINDOW_CASES}
    assert all("peaky" in c.wsets for c in WINDOW_CASES)
    assert {c.plan[:2] for c in WINDOW_CASES} == {(2, 0), (0, 1), (0, 0)}                 # every kind a windowed call can take
    assert any(c.plan[3] == 1 and c.T > 16 for c in WINDOW_CASES)                          # a decode that replays graphs
    spread = capped = False
    for c in WINDOW_CASES:
        if c.B * c.L > 700:
            continue
        n = reference(c, "plain")[1]["n_frames"].tolist()
        spread |= len(set(n)) > 1
        capped |= max(n) == c.T and min(n) < c.T
    assert spread and capped                                                               # rows that stop at different steps


# ---------------------------------------------------------------------------------------------------- plan routing
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def windowed_plan(lib, handle, B, L):
    fn = lib.gvx_debug_decoder_plan_windowed
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 4)(-1, -1, -1, -1)
    return fn(handle, B, L, out), tuple(out)


# every autoregressive case shape of tests/helpers.py: the (kind, split_h, fold, graph) a WINDOWED call takes there.  The pair keeps
# rows of <= 128 tokens; rows of 129-256 tokens (two attention workgroups per row) and GVX_AR_RESIDENT=1 handles go to kind 0.
WINDOWED_PLANS = {
    "ar2_1x1": (2, 0, 1, 0), "ar2_5x77": (2, 0, 1, 0), "ar2_32x128": (2, 0, 1, 0),
    "ar2_1x129": (0, 1, 1, 1), "ar2_16x256": (0, 1, 1, 1),
    "ar0_17x129": (0, 1, 1, 1), "ar0_2x257": (0, 1, 1, 1), "ar1_5x77": (0, 1, 1, 1), "ar0_loop0_5x77": (0, 1, 1, 1),
    "ar0_nosplit_5x77": (0, 0, 1, 1), "ar0_att16_3x40": (0, 0, 1, 1), "ar0_att256_3x40": (0, 0, 1, 1), "ar0_36x30": (0, 0, 0, 1),
    "ar0_dec512_3x40": (0, 1, 0, 1), "ar0_p128_4x50": (0, 1, 1, 1), "ar0_mels88_4x50": (0, 1, 1, 1), "ar0_small_5x13": (0, 0, 1, 1),
}


def test_windowed_plan_of_every_autoregressive_case_shape(lib):
    assert set(WINDOWED_PLANS) == {c.name for c in AR_CASES_FWD}
    for case in AR_CASES_FWD:
        h = create_handle(lib, dims_from_configs(*fwd_configs(case.dims)), case.env, case.setter)
        try:
            rc, plan = windowed_plan(lib, h, case.B, case.L)
            assert rc == 0 and plan == WINDOWED_PLANS[case.name], (case.name, plan)
            assert lib.gvx_autoregressive_windowed_loop_kind(h, case.B, case.L) == plan[0] != 1
            # ... and the un-windowed plan of the same shape is what the table of tests/helpers.py says: the window changed no plan
            assert decoder_plan(lib, h, 0, case.B, case.L)[2] == tuple(case.plan), case.name
            if plan[0] != decoder_plan(lib, h, 0, case.B, case.L)[2][0]:
                assert plan[0] == 0, case.name                                             # a windowed call only ever leaves for kind 0
        finally:
            lib.gvx_model_destroy(h)


def test_windowed_plan_of_the_window_cases(lib):
    for case in WINDOW_CASES:
        h = create_handle(lib, dims_from_configs(*fwd_configs(case.dims)), case.env)
        try:
            assert windowed_plan(lib, h, case.B, case.L) == (0, case.plan), case.name
        finally:
            lib.gvx_model_destroy(h)


def test_windowed_plan_query_checks_its_arguments(lib):
    h = create_handle(lib, dims_from_configs(*fwd_configs("def")))
    try:
        out = (C.c_int * 4)()
        fn = lib.gvx_debug_decoder_plan_windowed
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
        assert fn(None, 1, 1, out) == -1 and fn(h, 0, 1, out) == -1 and fn(h, 1, 0, out) == -1 and fn(h, 1, 1, None) == -1
        assert lib.gvx_autoregressive_windowed_loop_kind(None, 1, 1) == 0 and lib.gvx_autoregressive_windowed_loop_kind(h, 0, 5) == 0
    finally:
        lib.gvx_model_destroy(h)


# ---------------------------------------------------------------------------------------------------- argument checks
def test_windowed_export_refuses_bad_windows_before_anything_else(lib):
    """Negative widths and a NULL centres_out are GVX_ERR_INVALID_ARG (-1) with a message of their own, checked first: the other
    arguments here are not even plausible (no GPU is touched)."""
    h = create_handle(lib, dims_from_configs(*fwd_configs("def")))
    try:
        steps = C.c_int(-7)
        base = (h, 256, None, 2, 5, 4, 0.5, 256, 256, 256, 256, 256, C.byref(steps), 256, 1 << 30, None)
        for back, ahead, centres, word in ((-1, 3, 256, b"window_back"), (1, -3, 256, b"window_back"), (-2, -2, 256, b"window_back"),
                                           (1, 3, None, b"centres_out")):
            assert lib.gvx_decoder_autoregressive_windowed(*base, back, ahead, centres) == -1
            assert word in lib.gvx_last_error(), lib.gvx_last_error()
        assert steps.value == -7
        # a null handle is refused as by gvx_decoder_autoregressive
        assert lib.gvx_decoder_autoregressive_windowed(None, *base[1:], 1, 3, 256) == lib.gvx_decoder_autoregressive(None, *base[1:]) < 0
    finally:
        lib.gvx_model_destroy(h)


@pytest.mark.parametrize("bad", [(1,), (1, 2, 3), (-1, 2), (1, -2), (1.5, 2), "ab", 3, (None, 1)])
def test_python_surface_refuses_bad_windows(bad):
    with pytest.raises(ValueError, match="attention_window"):
        Tacotron2._check_window(bad)


def test_python_surface_accepts_windows():
    assert Tacotron2._check_window(None) is None
    assert Tacotron2._check_window((0, 1)) == (0, 1) and Tacotron2._check_window([3, 10]) == (3, 10)
    assert Tacotron2._check_window(torch.tensor([1, 3]).tolist()) == (1, 3)
