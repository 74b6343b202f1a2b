"""Evaluation metrics without a GPU: the float64 restatement (tests/metrics_ref64.py) against cases small enough to do by hand, the
DCT rows, the optimizer's state dict against torch.optim.Adam, and the argument checks of the new C-ABI calls."""
import math

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from genvox_amd.training import Adam
from tests import metrics_ref64 as ref


# ---- the warp ----------------------------------------------------------------------------------------------------------------

def _scalars(*vals):
    return np.asarray(vals, np.float64)[:, None]   # frames of one feature: d(i, j) = |x_i - y_j|


def test_dtw_one_by_one():
    A = ref.dtw_accumulated(_scalars(3.0), _scalars(5.0))
    assert A.shape == (1, 1) and A[0, 0] == 4.0                      # 2 d(0, 0)
    assert ref.dtw_distance_row(_scalars(3.0), _scalars(5.0)) == 2.0  # 4 / (1 + 1)


def test_dtw_one_by_n_and_n_by_one():
    x, y = _scalars(1.0), _scalars(1.0, 2.0, 4.0)
    A = ref.dtw_accumulated(x, y)
    assert A.tolist() == [[0.0, 1.0, 4.0]]            # 2*0, + |1-2|, + |1-4|
    assert ref.dtw_accumulated(y, x).tolist() == [[0.0], [1.0], [4.0]]
    assert ref.dtw_distance_row(x, y) == 1.0 == ref.dtw_distance_row(y, x)


def test_dtw_three_by_four_written_out():
    x, y = _scalars(0.0, 2.0, 3.0), _scalars(0.0, 1.0, 3.0, 3.0)
    # d = [[0 1 3 3], [2 1 1 1], [3 2 0 0]]
    want = [[0.0, 1.0, 4.0, 7.0],
            [2.0, 2.0, 3.0, 4.0],    # (1,1): min(1+1, 2+1, 0+2) = 2; (1,2): min(4+1, 2+1, 1+2) = 3; (1,3): min(7+1, 3+1, 4+2) = 4
            [5.0, 4.0, 2.0, 2.0]]    # (2,1): min(2+2, 5+2, 2+4) = 4; (2,2): min(3+0, 4+0, 2+0) = 2; (2,3): min(4+0, 2+0, 3+0) = 2
    assert ref.dtw_accumulated(x, y).tolist() == want
    assert ref.dtw_distance_row(x, y) == 2.0 / 7.0


def test_dtw_identity_symmetry_and_frame_doubling():
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((9, 5)), rng.standard_normal((6, 5))
    assert ref.dtw_distance_row(x, x) == 0.0
    assert ref.dtw_distance_row(x, y) == ref.dtw_distance_row(y, x)
    assert np.array_equal(ref.dtw_accumulated(x, y), ref.dtw_accumulated(y, x).T)
    assert ref.dtw_distance_row(x, np.repeat(x, 2, axis=0)) == 0.0   # a sequence against its own frame-doubled copy
    assert ref.dtw_distance_row(x, y) > 0.0


def test_dtw_empty_rows_and_ragged_batch():
    rng = np.random.default_rng(1)
    cp, cg = rng.standard_normal((3, 5, 2)), rng.standard_normal((3, 4, 2))
    d = ref.dtw_distance(cp, cg, [5, 0, 9], [4, 2, -1])
    assert d[0] == ref.dtw_distance_row(cp[0], cg[0]) and math.isnan(d[1]) and math.isnan(d[2])


def test_dct_rows_are_orthonormal_and_leave_out_the_energy_term():
    for M, K in ((80, 13), (80, 79), (12, 1), (128, 40)):
        P = metrics.dct_rows(M, K)
        assert P.dtype == np.float64 and P.shape == (K, M)
        assert np.abs(P @ P.T - np.eye(K)).max() < 1e-13
        assert np.abs(P.sum(axis=1)).max() < 1e-13          # orthogonal to the constant row 0: a gain on every mel changes nothing
        assert np.array_equal(P, ref.dct_rows(M, K)) or np.abs(P - ref.dct_rows(M, K)).max() < 1e-15
    with pytest.raises(ValueError):
        metrics.dct_rows(80, 80)
    with pytest.raises(ValueError):
        metrics.dct_rows(80, 0)


def test_mcd_db_scale_follows_the_log_of_the_mels():
    class Cfg:
        log_func = "np.log10"
    d = torch.tensor([0.0, 1.0, 2.5])
    got10 = metrics.mcd_db(d, Cfg)
    Cfg.log_func = "np.log"
    got_e = metrics.mcd_db(d, Cfg)
    assert np.allclose(got10.numpy(), ref.mcd_db(d.numpy(), True), rtol=1e-6)
    assert np.allclose(got_e.numpy(), ref.mcd_db(d.numpy(), False), rtol=1e-6)
    assert np.allclose(got10[1].item(), 10.0 * math.sqrt(2.0), rtol=1e-6)


# ---- alignment statistics -------------------------------------------------------------------------------------------------------

def test_alignment_ties_go_to_the_lowest_index():
    a = np.zeros((1, 3, 4))
    a[0, 0] = [0.2, 0.4, 0.4, 0.0]
    a[0, 1] = [0.25, 0.25, 0.25, 0.25]
    a[0, 2] = [0.0, 0.1, 0.3, 0.3]
    s = ref.alignment_stats(a)
    assert s["positions"].tolist() == [[1, 0, 2]]
    assert s["durations"].tolist() == [[1, 1, 1, 0]]
    assert s["monotonic"][0] == 1 and s["max_jump"][0] == 2 and s["covered"][0] == 3
    assert s["focus"][0] == (0.4 + 0.25 + 0.3) / 3


def test_alignment_perfect_reversed_and_constant():
    n = 6
    eye = np.eye(n)[None]
    s = ref.alignment_stats(eye)
    assert s["positions"].tolist() == [list(range(n))] and s["durations"].tolist() == [[1] * n]
    assert (s["focus"][0], s["monotonic"][0], s["max_jump"][0], s["covered"][0]) == (1.0, n - 1, 1, n)
    assert (s["first_pos"][0], s["last_pos"][0], s["monotonic_fraction"][0], s["coverage"][0]) == (0, n - 1, 1.0, 1.0)
    s = ref.alignment_stats(eye[:, ::-1])
    assert (s["monotonic"][0], s["max_jump"][0], s["covered"][0], s["first_pos"][0], s["last_pos"][0]) == (0, 1, n, n - 1, 0)
    assert s["monotonic_fraction"][0] == 0.0
    s = ref.alignment_stats(np.full((1, 5, 4), 0.25))
    assert s["positions"].tolist() == [[0] * 5] and s["durations"].tolist() == [[5, 0, 0, 0]]
    assert (s["focus"][0], s["monotonic"][0], s["max_jump"][0], s["covered"][0], s["coverage"][0]) == (0.25, 4, 0, 1, 0.25)


def test_alignment_lengths_nan_frames_and_empty_rows():
    a = np.full((3, 4, 5), np.nan)
    a[0, :2, :3] = [[0.1, 0.7, 0.2], [0.0, 0.2, 0.8]]
    a[2, 0, :2] = [0.5, 0.5]              # row 2: frame 1 is all NaN inside its lengths
    s = ref.alignment_stats(a, mel_lengths=[2, 0, 2], token_lengths=[3, 5, 2])
    assert s["positions"].tolist() == [[1, 2, -1, -1], [-1] * 4, [0, 0, -1, -1]]
    assert s["durations"].tolist() == [[0, 1, 1, 0, 0], [0] * 5, [2, 0, 0, 0, 0]]
    assert s["focus"][0] == 0.75 and math.isnan(s["focus"][1]) and math.isnan(s["focus"][2])
    assert s["monotonic"].tolist() == [1, 0, 1] and s["covered"].tolist() == [2, 0, 1]
    assert math.isnan(s["peaks"][2, 1]) and s["peaks"][2, 0] == 0.5


# ---- the optimizer's state dict ------------------------------------------------------------------------------------------------

def _tiny():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2))


def test_adam_state_dict_has_torch_layout_and_round_trips_both_ways():
    model = _tiny()
    ours = Adam(model, lr=2e-3, weight_decay=1e-6, betas=(0.8, 0.99), eps=1e-7)
    theirs = torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=1e-6, betas=(0.8, 0.99), eps=1e-7)
    fresh, want = ours.state_dict(), theirs.state_dict()
    assert fresh["state"] == {} and set(fresh) == set(want)
    assert fresh["param_groups"] == want["param_groups"]       # same keys, same values, params [0 .. n-1]
    for _ in range(3):
        theirs.zero_grad()
        model(torch.ones(5, 3)).square().sum().backward()
        theirs.step()
    want = theirs.state_dict()
    ours.load_state_dict(want)                                    # what torch wrote
    got = ours.state_dict()
    names = [n for n, _ in model.named_parameters()]
    assert ours.step_count == 3 and list(got["state"]) == list(range(len(names))) == list(want["state"])
    for i, name in enumerate(names):
        assert set(got["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} == set(want["state"][i])
        assert float(got["state"][i]["step"]) == 3.0
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got["state"][i][key], want["state"][i][key])
            assert got["state"][i][key].data_ptr() != want["state"][i][key].data_ptr()     # copies: the two do not share moments
        assert ours.state[name][0] is got["state"][i]["exp_avg"]                           # index i is parameter i
    other = torch.optim.Adam(model.parameters(), lr=1.0)
    other.load_state_dict(got)                                    # what we wrote
    back = other.state_dict()
    assert back["param_groups"][0]["lr"] == 2e-3 and back["param_groups"][0]["betas"] == (0.8, 0.99)
    for i in range(len(names)):
        assert torch.equal(back["state"][i]["exp_avg_sq"], want["state"][i]["exp_avg_sq"]) and float(back["state"][i]["step"]) == 3.0
    other.step()                                                  # torch can go on from it
    ours.load_state_dict({"state": {i: {**st, "step": 7} for i, st in got["state"].items()}, "param_groups": got["param_groups"]})
    assert ours.step_count == 7                                   # a plain number as step


def test_adam_load_state_dict_refuses_what_it_cannot_honour():
    model = _tiny()
    ours = Adam(model, lr=1e-3)
    sd = ours.state_dict()
    with pytest.raises(ValueError):
        ours.load_state_dict({"state": {}, "param_groups": [{**sd["param_groups"][0], "amsgrad": True}]})
    with pytest.raises(ValueError):
        ours.load_state_dict({"state": {}, "param_groups": [{**sd["param_groups"][0], "params": [0, 1]}]})
    p = [q for _, q in model.named_parameters()]
    st = {i: {"step": torch.tensor(float(1 + (i == 2))), "exp_avg": torch.zeros_like(q), "exp_avg_sq": torch.zeros_like(q)} for i, q in enumerate(p)}
    with pytest.raises(ValueError):
        ours.load_state_dict({"state": st, "param_groups": sd["param_groups"]})
    st = {0: {"step": 1, "exp_avg": torch.zeros(2), "exp_avg_sq": torch.zeros(2)}}
    with pytest.raises(ValueError):
        ours.load_state_dict({"state": st, "param_groups": sd["param_groups"]})


# ---- argument checks of the C ABI (nothing is launched) -------------------------------------------------------------------------

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -5
X = 256   # a non-null, 256-byte aligned address that is never dereferenced: every call below fails before its launch


def test_dtw_plan_queries():
    lib = _lib.load()
    assert lib.gvx_dtw_uses_lds_tables(1000, 1000, 13) == 1 and lib.gvx_dtw_workspace_bytes(32, 1000, 1000, 13) == 0
    assert lib.gvx_dtw_uses_lds_tables(1000, 1000, 80) == 0
    assert lib.gvx_dtw_workspace_bytes(32, 1000, 1000, 80) == 32 * 3 * 1000 * 4
    assert lib.gvx_dtw_uses_lds_tables(10000, 800, 13) == 0 and lib.gvx_dtw_workspace_bytes(1, 10000, 800, 13) == (3 * 10000 * 4 + 255) // 256 * 256
    assert lib.gvx_dtw_workspace_bytes(1, 10000, 800, 13) % 256 == 0
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (32769, 5, 1), (5, 5, 257)):
        assert lib.gvx_dtw_uses_lds_tables(*bad) == -1 and lib.gvx_dtw_workspace_bytes(1, *bad) == 0
    assert lib.gvx_dtw_workspace_bytes(0, 5, 5, 1) == 0


def test_new_calls_check_their_arguments_before_any_launch():
    lib = _lib.load()

    def err():
        return lib.gvx_last_error().decode()

    assert lib.gvx_alignment_stats(None, None, None, 1, 4, 4, X, X, X, X, X, None) == INVALID and "null" in err()
    assert lib.gvx_alignment_stats(X, None, None, 1, 4, 4, X, X, None, X, X, None) == INVALID
    for B, T, L in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.gvx_alignment_stats(X, None, None, B, T, L, X, X, X, X, X, None) == INVALID
    assert lib.gvx_alignment_stats(X, None, None, 65536, 4, 4, X, X, X, X, X, None) == UNSUPPORTED
    assert lib.gvx_mel_project(None, 1, 80, 10, X, 13, X, None) == INVALID
    assert lib.gvx_mel_project(X, 1, 80, 10, X, 0, X, None) == INVALID
    assert lib.gvx_mel_project(X, 1, 80, 10, X, 81, X, None) == INVALID and "K = 81" in err()
    assert lib.gvx_mel_project(X, 1, 256, 10, X, 256, X, None) == UNSUPPORTED
    assert lib.gvx_dtw_distance(None, X, None, None, 1, 5, 5, 2, X, None, None, 0, None) == INVALID
    assert lib.gvx_dtw_distance(X, X, None, None, 1, 5, 5, 2, None, None, None, 0, None) == INVALID
    assert lib.gvx_dtw_distance(X, X, None, None, 1, 5, 0, 2, X, None, None, 0, None) == INVALID
    assert lib.gvx_dtw_distance(X, X, None, None, 1, 40000, 5, 2, X, None, None, 0, None) == UNSUPPORTED and "40000" in err()
    need = lib.gvx_dtw_workspace_bytes(2, 1000, 1000, 80)
    assert need > 0
    assert lib.gvx_dtw_distance(X, X, None, None, 2, 1000, 1000, 80, X, None, None, 0, None) == WORKSPACE
    assert lib.gvx_dtw_distance(X, X, None, None, 2, 1000, 1000, 80, X, None, X + 64, need, None) == WORKSPACE
    assert lib.gvx_dtw_distance(X, X, None, None, 2, 1000, 1000, 80, X, None, X, need - 1, None) == WORKSPACE and "too small" in err()
