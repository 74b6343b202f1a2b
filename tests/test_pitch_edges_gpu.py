"""GPU: gvx_pitch_yin at the parameter sets of tests/pitch_edge_cases.py - windows that are no multiple of 64, workgroups of fewer
than 16 frames, lag tables at the edges of a lane's three lags, of a pass and of the running sum's ownership, other thresholds, and
the grid's limit in rows.  Every case is held by tests.test_pitch_gpu.hold to the float64 restatement with the bounds derived in
tests/pitch_ref64.py: every table element, lag, f0 and aperiodicity, NaN behind every row, the outputs behind a row's frames."""
import numpy as np
import pytest
import torch

from genvox_amd import _lib
from tests import pitch_edge_cases as C
from tests.test_pitch_gpu import DEV, SENTINEL, device_yin, hold, same

pytestmark = pytest.mark.gpu


def held(case):
    return hold(case.name, C.yin_input(case), case.lengths, case.p, case.first_centre)


@pytest.mark.parametrize("name", [c.name for c in C.WINDOW_CASES])
def test_window_tail(name):
    """W = 64 q + n: q unrolled blocks and py_block<false> over the n terms left (W < 64: that block alone)."""
    case = C.YIN_BY_NAME[name]
    got = held(case)
    assert (got["lag"] >= 0).any() and (got["lag"][-2:] == -1).any()


@pytest.mark.parametrize("name", [c.name for c in C.TILE_CASES])
def test_tile_below_sixteen(name):
    """W 2048 with lag_max 1024 leaves 9212 floats of LDS beside the first frame: hops of 700, 1024, 4096 and 9300 samples make
    workgroups of 14, 9, 3 and 1 frames - rounds in which some of the four waves have no frame, a tile below the number of waves."""
    case = C.YIN_BY_NAME[name]
    p = case.p
    tile, F = C.TILE_FRAMES[p["hop"]]
    params = _lib.gvx_pitch_params(p["sampling_rate"], p["hop"], p["window"], p["lag_min"], p["lag_max"], p["threshold"], 0)
    assert _lib.load().gvx_pitch_tile_frames(params) == tile
    x = C.yin_input(case)
    got = held(case)
    assert got["lag"].shape == (3, F)
    for b, n in enumerate(case.lengths):   # every row alone gives the bits it has in the batch
        rc, alone = device_yin(x[b:b + 1], [n], p)
        assert rc == 0
        same(got, alone, slice(b, b + 1))


@pytest.mark.parametrize("name", [c.name for c in C.LAG_CASES])
def test_lag_table_edges(name):
    case = C.YIN_BY_NAME[name]
    got = held(case)
    if case.p["lag_max"] == 2:
        assert (got["lag"] == -1).all()   # c(1) = d(1) / d(1): the one lag scanned is never under the threshold
    else:
        assert (got["lag"] >= 0).any()


@pytest.mark.parametrize("name", [c.name for c in C.THRESHOLD_CASES])
def test_thresholds(name):
    case = C.YIN_BY_NAME[name]
    p = case.p
    got = held(case)
    if p["threshold"] < 0.1:   # no frame is voiced: aperiodicity is the minimum of the device's own table over [lag_min, lag_max)
        frames = [-(-n // p["hop"]) for n in case.lengths]
        assert (got["lag"] == -1).all() and (got["f0"] == 0).all()
        for b, Fb in enumerate(frames):
            want = got["cmnd"][b, :Fb, p["lag_min"]:p["lag_max"]].min(axis=1)
            assert got["aperiodicity"][b, :Fb].tobytes() == want.tobytes(), b
    else:
        assert (got["lag"] >= 0).any()


def test_grid_limit_in_rows():
    """B = 65535, the most rows a launch's grid takes: rows and lengths repeat with period 8, and every row has the bits of the same
    row in a batch of 8, which is itself held to float64.  No table (it would be 43 MB); the outputs are allocated once."""
    case = C.GRID_CASE
    p, B, N = case.p, C.GRID_ROWS, C.GRID_N
    x8 = C.yin_input(case)
    small = held(case)
    lib = _lib.load()
    F = lib.gvx_pitch_frames(N, p["hop"])
    reps = -(-B // C.GRID_PERIOD)
    wav = torch.from_numpy(x8).to(DEV).repeat(reps, 1)[:B].contiguous()
    lens = torch.tensor(case.lengths, dtype=torch.int32, device=DEV).repeat(reps)[:B].contiguous()
    f0 = torch.full((B, F), float("nan"), device=DEV)
    ap = torch.full((B, F), float("nan"), device=DEV)
    lag = torch.full((B, F), SENTINEL, dtype=torch.int32, device=DEV)
    params = _lib.gvx_pitch_params(p["sampling_rate"], p["hop"], p["window"], p["lag_min"], p["lag_max"], p["threshold"], 0)
    rc = lib.gvx_pitch_yin(wav.data_ptr(), lens.data_ptr(), B, N, params, f0.data_ptr(), lag.data_ptr(), ap.data_ptr(), None,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.gvx_last_error()
    for key, out in (("f0", f0), ("lag", lag), ("aperiodicity", ap)):
        want = np.tile(small[key], (reps, 1))[:B]
        assert out.cpu().numpy().tobytes() == want.tobytes(), key
    assert lib.gvx_pitch_yin(wav.data_ptr(), lens.data_ptr(), B + 1, N, params, f0.data_ptr(), lag.data_ptr(), ap.data_ptr(), None, None) == -2
