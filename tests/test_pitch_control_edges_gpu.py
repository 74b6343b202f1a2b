"""GPU: gvx_psola_plan and gvx_psola_synth at the parameter sets of tests/pitch_edge_cases.py - the 22050 Hz grid and the limits
(runs of several samples per lane in the peak search, the staged chunk moving, P = 1024), U above lag_max, hops of 1 and of more
than a chunk, a period of 1, equal maxima, lags outside the range, ratios at and just outside the limits, NULL lengths.  Every case
goes through tests.test_pitch_control_gpu.run_device and compare: everything integral exactly, sentinels untouched, zeros behind
the rows, every sample inside psola_ref.y_bound; and twice, for the same bits."""
import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from tests import pitch_edge_cases as C
from tests import psola_ref as R
from tests.test_pitch_control_gpu import DEV, SENTINEL, compare, make_batch, params_of, run_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in C.PSOLA_CASES])
def test_case(name):
    case = C.PSOLA_BY_NAME[name]
    wav, lengths, lag, ratio = C.psola_input(case)
    ref = C.psola_reference(case)
    params = params_of(case.first_centre, case.cfg)
    got, rc_plan, rc_synth = run_device(wav, lengths, lag, ratio, params)
    assert rc_plan == 0 and rc_synth == 0, _lib.load().gvx_last_error()
    worst = compare(got, ref, wav, lengths, name)
    print(f"{name}: largest error / bound = {worst:.3f}")
    again, _, _ = run_device(wav, lengths, lag, ratio, params)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    if case.kind == "ratios":
        assert got["status"].tolist() == [R.BAD_RATIO] * 4 + [R.OK]
        for b in range(4):   # a bad ratio: the row goes through unchanged
            n = case.lengths[b]
            assert got["y"][b, :n].tobytes() == wav[b, :n].tobytes() and got["counts"][b, 1] == 0, b
        assert got["counts"][4, 1] > 0


def run_null_lengths(wav, lag, ratio, params):
    """run_device with NULL for sample_lengths at both calls."""
    lib = _lib.load()
    B, N = wav.shape
    p_min = min(params.lag_min, params.unvoiced_period)
    K, J = lib.gvx_psola_max_marks(N, p_min), lib.gvx_psola_max_grains(N, p_min)
    x, lg, rt = (torch.from_numpy(a).to(DEV) for a in (wav, lag, ratio))
    ints = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)
    out = {"marks": ints(B, K), "periods": ints(B, K), "syn_pos": ints(B, J), "syn_src": ints(B, J), "counts": ints(B, 2), "status": ints(B),
           "y": torch.full((B, N), float(SENTINEL), dtype=torch.float32, device=DEV)}
    stream = torch.cuda.current_stream().cuda_stream
    rc_plan = lib.gvx_psola_plan(x.data_ptr(), None, lg.data_ptr(), rt.data_ptr(), B, N, params, out["marks"].data_ptr(), out["periods"].data_ptr(),
                                 out["syn_pos"].data_ptr(), out["syn_src"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr(), stream)
    rc_synth = lib.gvx_psola_synth(x.data_ptr(), None, out["marks"].data_ptr(), out["periods"].data_ptr(), out["syn_pos"].data_ptr(),
                                   out["syn_src"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr(), B, N, params, out["y"].data_ptr(), stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, rc_plan, rc_synth


@pytest.mark.parametrize("grid", ["small", "default"])
def test_null_lengths_are_full_rows(grid):
    cfg, N = (C.PS_SMALL, 529) if grid == "small" else (C.PS_DEFAULT, 4500)
    wav, lengths, lag, ratio = make_batch([N] * 4, N, 61, 0, cfg)
    listed, rc_plan, rc_synth = run_device(wav, lengths, lag, ratio, params_of(0, cfg))
    assert rc_plan == 0 and rc_synth == 0
    ref = R.psola(wav, lengths, lag, ratio, **cfg)
    print(f"full rows, {grid}: largest error / bound = {compare(listed, ref, wav, lengths, grid):.3f}")
    null, rc_plan, rc_synth = run_null_lengths(wav, lag, ratio, params_of(0, cfg))
    assert rc_plan == 0 and rc_synth == 0
    for k in listed:
        assert listed[k].tobytes() == null[k].tobytes(), k


def test_python_calls_on_the_default_grid():
    """metrics.psola_plan and metrics.pitch_shift with their default fmin, fmax and unvoiced period at 22050 Hz are the C calls of
    the default-grid case: the same bits wherever the calls write."""
    case = C.PSOLA_BY_NAME["default_fc-3000"]
    wav, lengths, lag, ratio = C.psola_input(case)
    got, _, _ = run_device(wav, lengths, lag, ratio, params_of(case.first_centre, case.cfg))
    t = lambda a: torch.from_numpy(a).to(DEV)
    kw = dict(sampling_rate=22050, hop_length=256, first_centre=case.first_centre)
    plan = {k: v.cpu().numpy() for k, v in metrics.psola_plan(t(wav), t(lengths), t(lag), t(ratio), **kw).items()}
    out = {k: v.cpu().numpy() for k, v in metrics.pitch_shift(t(wav), t(lengths), t(lag), t(ratio), **kw).items()}
    assert out["wav"].tobytes() == got["y"].tobytes()
    for res in (plan, out):
        assert np.array_equal(res["status"], got["status"]) and np.array_equal(res["n_marks"], got["counts"][:, 0])
        assert np.array_equal(res["n_grains"], got["counts"][:, 1])
    assert plan["marks"].shape == got["marks"].shape and plan["syn_pos"].shape == got["syn_pos"].shape
    for b, (K, J) in enumerate(got["counts"]):
        for key, count in (("marks", K), ("periods", K), ("syn_pos", J), ("syn_src", J)):
            assert plan[key][b, :count].tobytes() == got[key][b, :count].tobytes(), (b, key)
