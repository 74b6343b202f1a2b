"""GPU: gvx_pitch_yin and gvx_f0_compare against their float64 restatement (tests/pitch_ref64.py).

Every case runs with NaN in all samples at and behind each row's length and in every output beforehand (lags: a sentinel).  The
calls have no workspace.

The table.  d is a sum of W non-negative terms and the running sum a sum of non-negative terms, so in any summation order
|c32 - c64| <= (2 W + lag_max + 8) 2^-24 c64 (derived term by term in pitch_ref64.table_bound; 1.45e-4 at the defaults); every element
of every frame inside a row is held to it, and the largest observed ratio to the bound is printed.

The decisions.  A frame is marginal if a comparison its float64 scan actually performed - c(tau) < threshold up to and including
the first crossing, c(tau+1) < c(tau) along the walk - lies closer to a tie than that bound (relative to the numbers compared).
Marginal frames are not held on lag and f0; every other frame's lag is exact.  A voiced frame's f0 is held to the table's bound
carried through the parabola's quotient (pitch_ref64.f0_tolerance), unless the parabola's denominator is below 16 times the
table's absolute bound: then on lag only.  Both kinds count towards a cap of 5 % of a case's frames, which is a condition of the
test, not a measurement.  aperiodicity is a table element and held to the table's bound."""
import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics
from tests import pitch_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7777
DEFAULT = dict(sampling_rate=22050, hop=256, window=1024, lag_min=44, lag_max=368, threshold=0.15)
SMALL = dict(sampling_rate=2000, hop=16, window=64, lag_min=4, lag_max=40, threshold=0.15)
WIDE = dict(sampling_rate=22050, hop=256, window=2048, lag_min=44, lag_max=1024, threshold=0.15)


def master(rate: int) -> np.ndarray:
    """Two seconds of a five-harmonic glide from 110 Hz up 1.5 octaves with 2 % vibrato at 5 Hz, amplitude 0.3 (harmonics kept below
    0.45 of the rate).  Over a row of a quarter of a second the whole glide would be no periodic signal at all - 8 octaves a second -
    so the rows cut their voiced stretch out of this one at different places and cover the 1.5 octaves between them."""
    n = 2 * rate
    t = np.arange(n) / rate
    f = 110.0 * 2.0 ** (1.5 * np.arange(n) / n) * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))
    phase = 2 * np.pi * np.cumsum(f) / rate
    return 0.3 * sum(np.where(h * f < 0.45 * rate, np.sin(h * phase) / h, 0.0) for h in range(1, 6)) / 1.5


_masters = {}


def signal(n: int, rate: int, seed: int) -> np.ndarray:
    """float32 [n]: 60 % voiced (a stretch of master(rate) from a place the seed picks, Gaussian noise of 0.01 on top), 20 % noise
    alone (0.1), 20 % exact zeros."""
    rng = np.random.default_rng(seed)
    m = _masters.setdefault(rate, master(rate))
    n1, n2 = int(0.6 * n), int(0.8 * n)
    at = int(rng.uniform(0, 1) * (len(m) - n1))
    x = np.zeros(n)
    x[:n1] = m[at:at + n1] + 0.01 * rng.standard_normal(n1)
    x[n1:n2] = 0.1 * rng.standard_normal(n2 - n1)
    return x.astype(np.float32)


def batch(lengths, N, rate, seed):
    """[B, N] float32: row b is signal(lengths[b]) and NaN at and behind its length."""
    x = np.full((len(lengths), N), np.nan, np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = signal(n, rate, seed + b)
    return x


def device_yin(x: np.ndarray, lengths, p: dict, first_centre: int = 0, table: bool = True):
    """The C call on NaN-filled outputs -> (rc, {f0, lag, aperiodicity, cmnd} as numpy)."""
    lib = _lib.load()
    params = _lib.gvx_pitch_params(p["sampling_rate"], p["hop"], p["window"], p["lag_min"], p["lag_max"], p["threshold"], first_centre)
    wav = torch.from_numpy(x).to(DEV)
    B, N = x.shape
    F = max(lib.gvx_pitch_frames(N, max(p["hop"], 1)), 1)
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    f0 = torch.full((B, F), float("nan"), device=DEV)
    ap = torch.full((B, F), float("nan"), device=DEV)
    lag = torch.full((B, F), SENTINEL, dtype=torch.int32, device=DEV)
    cm = torch.full((B, F, p["lag_max"] + 1), float("nan"), device=DEV) if table else None
    rc = lib.gvx_pitch_yin(wav.data_ptr(), None if lens is None else lens.data_ptr(), B, N, params, f0.data_ptr(), lag.data_ptr(), ap.data_ptr(),
                           None if cm is None else cm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {"f0": f0.cpu().numpy(), "lag": lag.cpu().numpy(), "aperiodicity": ap.cpu().numpy(), "cmnd": None if cm is None else cm.cpu().numpy()}


def hold(name: str, x: np.ndarray, lengths, p: dict, first_centre: int = 0):
    """One case against float64.  Returns the device's outputs."""
    rc, got = device_yin(x, lengths, p, first_centre)
    assert rc == 0, _lib.load().gvx_last_error()
    ref = R.yin(x, lengths, first_centre=first_centre, **p)
    bound = R.table_bound(p["window"], p["lag_max"])
    B, F = ref["lag"].shape
    assert got["lag"].shape == (B, F)
    worst, marginal, total = 0.0, 0, 0
    for b in range(B):
        Fb = int(ref["frames"][b])
        assert (got["f0"][b, Fb:] == 0).all() and (got["lag"][b, Fb:] == -1).all() and (got["aperiodicity"][b, Fb:] == 1).all(), (name, b)
        assert np.isnan(got["cmnd"][b, Fb:]).all(), (name, b)          # not touched behind the row's frames
        for f in range(Fb):
            total += 1
            c64, c32 = ref["cmnd"][b, f], got["cmnd"][b, f].astype(np.float64)
            err = np.abs(c32 - c64)
            assert (err <= bound * c64).all(), (name, b, f, int(np.argmax(err - bound * c64)), float((err / np.maximum(c64, 1e-300)).max()), bound)
            worst = max(worst, float((err[c64 > 0] / (bound * c64[c64 > 0])).max(initial=0.0)))
            lag = int(ref["lag"][b, f])
            if ref["margin"][b, f] <= bound:
                marginal += 1
                continue
            assert got["lag"][b, f] == lag, (name, b, f, int(got["lag"][b, f]), lag)
            a64 = ref["aperiodicity"][b, f]
            assert abs(float(got["aperiodicity"][b, f]) - a64) <= bound * a64, (name, b, f)
            if lag < 0:
                assert got["f0"][b, f] == 0, (name, b, f)
                continue
            tol, _ = R.f0_tolerance(c64, lag, p["sampling_rate"], bound)
            if tol is None:
                marginal += 1
                continue
            assert abs(float(got["f0"][b, f]) - ref["f0"][b, f]) <= tol, (name, b, f, float(got["f0"][b, f]), float(ref["f0"][b, f]), tol)
    voiced = int((ref["lag"] >= 0).sum())
    print(f"{name}: {total} frames, {voiced} voiced, {marginal} marginal, largest table error {worst:.3f} of the bound {bound:.3e}")
    assert marginal <= 0.05 * total, (name, marginal, total)
    return got


def same(a: dict, b: dict, rows_a=slice(None), rows_b=slice(None), frames=None):
    for k in ("f0", "lag", "aperiodicity", "cmnd"):
        if a[k] is None or b[k] is None:
            continue
        u, v = a[k][rows_a], b[k][rows_b]
        if frames is not None:
            u, v = u[:, :frames], v[:, :frames]
        assert u.tobytes() == v.tobytes(), k


@pytest.mark.parametrize("first_centre", [0, -500, 300])
def test_default_parameters(first_centre):
    """22050 Hz, hop 256, W 1024, lags 44 - 368: a ragged batch of rows of about 24 frames (k hop - 1, k hop, k hop + 1 samples, a row
    shorter than W + lag_max, a row of nothing) on three frame grids; the glide makes voiced frames, the noise and the zeros unvoiced."""
    lengths = [24 * 256, 24 * 256 - 1, 23 * 256 + 1, 1300, 0]
    x = batch(lengths, 24 * 256, 22050, seed=11)
    got = hold(f"default, first_centre {first_centre}", x, lengths, DEFAULT, first_centre)
    assert (got["lag"][0] >= 0).sum() >= 8 and (got["lag"][0] == -1).sum() >= 6
    # two calls give the same bits; the table changes no bit of the other outputs
    _, again = device_yin(x, lengths, DEFAULT, first_centre)
    same(got, again)
    _, bare = device_yin(x, lengths, DEFAULT, first_centre, table=False)
    same(got, bare)


def test_row_edges_small_configuration():
    """hop 16, W 64, lags 4 - 40: a workgroup takes 16 frames.  Rows of 0 samples, less than a hop, less than W + lag_max, k hop - 1 /
    k hop / k hop + 1, and 15, 16, 17 and 33 frames; every row alone gives the bits it has in the batch."""
    lib = _lib.load()
    tile = lib.gvx_pitch_tile_frames(_lib.gvx_pitch_params(2000, 16, 64, 4, 40, 0.15, 0))
    assert tile == 16
    lengths = [0, 5, 90, 47, 48, 49, (tile - 1) * 16, tile * 16, tile * 16 + 1, 2 * tile * 16 + 3, 400]
    N = 528
    x = batch(lengths, N, 2000, seed=23)
    got = hold("small, ragged", x, lengths, SMALL)
    assert (got["lag"] >= 0).any()
    for b, n in enumerate(lengths):
        rc, alone = device_yin(x[b:b + 1], [n], SMALL)
        assert rc == 0
        same(got, alone, slice(b, b + 1))
    # NULL lengths: every row is N samples (no NaN may be left inside then)
    full = batch([N] * 3, N, 2000, seed=31)
    whole = hold("small, NULL lengths", full, None, SMALL)
    rc, listed = device_yin(full, [N] * 3, SMALL)
    same(whole, listed)
    # a narrower buffer: the row of 400 samples in a batch of stride 400 has the bits of its first frames in the stride of 528
    rc, narrow = device_yin(x[10:11, :400].copy(), [400], SMALL, table=False)
    same(got, narrow, slice(10, 11), frames=25)
    # B = 1 without lengths, positive and negative grids
    for fc in (-37, 21):
        hold(f"small, one row, first_centre {fc}", full[:1], None, SMALL, fc)


def test_lds_limit():
    """lag_max = 1024 with W = 2048: the largest tables and the longest window, one short row."""
    x = batch([3000], 3000, 22050, seed=5)
    got = hold("W 2048, lag_max 1024", x, [3000], WIDE)
    assert got["lag"].shape == (1, 12)


def test_refused_arguments_write_nothing():
    x = batch([600], 600, 2000, seed=3)
    for bad, want in ((dict(hop=0), -1), (dict(lag_min=0), -1), (dict(lag_min=40), -1), (dict(threshold=0.0), -1), (dict(threshold=1.5), -1),
                      (dict(window=31), -2), (dict(window=2049), -2), (dict(lag_max=1025), -2), (dict(sampling_rate=0), -1)):
        p = dict(SMALL)
        p.update(bad)
        rc, got = device_yin(x, [600], p)
        assert rc == want, (bad, rc)
        assert np.isnan(got["f0"]).all() and (got["lag"] == SENTINEL).all() and np.isnan(got["aperiodicity"]).all() and np.isnan(got["cmnd"]).all(), bad


def test_pitch_track_api():
    """metrics.pitch_track is the call: float32 and float64 input, the frame counts, the table on request."""
    lengths = [700, 333]
    x = batch(lengths, 700, 2000, seed=41)
    _, want = device_yin(x, lengths, SMALL, first_centre=-8)
    kw = dict(sampling_rate=2000, hop_length=16, fmin=50.0, fmax=500.0, window=64, first_centre=-8)
    for dtype in (torch.float32, torch.float64):
        got = metrics.pitch_track(torch.from_numpy(x).to(DEV, dtype), torch.tensor(lengths), want_table=True, **kw)
        assert set(got) == {"f0", "lag", "aperiodicity", "frames", "cmnd"} and got["frames"].tolist() == [44, 21] and got["frames"].dtype == torch.int32
        same(want, {k: got[k].cpu().numpy() for k in ("f0", "lag", "aperiodicity", "cmnd")})
    assert set(metrics.pitch_track(torch.from_numpy(x[:, :333].copy()).to(DEV), **kw)) == {"f0", "lag", "aperiodicity", "frames"}
    with pytest.raises(ValueError):
        metrics.pitch_track(torch.zeros(4, dtype=torch.float32, device=DEV), **kw)
    with pytest.raises(ValueError):
        metrics.pitch_track(torch.zeros(1, 64, dtype=torch.int16, device=DEV), **kw)


def test_f0_compare():
    """Counts, vde and gpe exact (the float32 quotient of the exact counts); rmse_cents against float64 within 8 times the float32
    restatement's own error - the largest relative one among the rows, since a row of a few frames can round to nothing by luck."""
    rng = np.random.default_rng(9)
    B, F = 7, 700
    fa = (200.0 * 2.0 ** rng.uniform(-1, 1, (B, F))).astype(np.float32)
    fb = (fa * 2.0 ** rng.normal(0, 0.03, (B, F))).astype(np.float32)
    fa[rng.random((B, F)) < 0.2] = 0
    fb[rng.random((B, F)) < 0.2] = 0
    octave = rng.random((B, F)) < 0.05
    fb[octave] *= 2
    fa[1], fb[1] = 0, 0                       # nothing voiced
    fb[2] = np.where(fa[2] > 0, 3 * fa[2], 0)  # only gross errors
    fb[4, 10] = np.nan                         # NaN is unvoiced
    na, nb = [700, 700, 650, 0, 300, 1, 257], [700, 600, 700, 700, 256, 700, 700]
    counts, vde, gpe, rmse = R.f0_compare(fa, fb, na, nb)
    r32 = R.f0_compare(fa, fb, na, nb, dtype=np.float32)[3]
    dead_a, dead_b = fa.copy(), fb.copy()
    for b in range(B):
        dead_a[b, min(na[b], nb[b]):] = np.nan   # what lies behind a row's frames is not read: NaN there is not counted as a frame
        dead_b[b, min(na[b], nb[b]):] = np.nan
    got = metrics.f0_compare(torch.from_numpy(dead_a).to(DEV), torch.from_numpy(dead_b).to(DEV), torch.tensor(na), torch.tensor(nb))
    ints = np.stack([got[k].cpu().numpy() for k in metrics.F0_ROW_INT_NAMES], axis=1)
    assert np.array_equal(ints, counts)
    assert counts[1].tolist() == [600, 0, 0, 0] and counts[2, 1] == counts[2, 3] > 0 and counts[3, 0] == 0
    with np.errstate(all="ignore"):
        want_vde = counts[:, 2].astype(np.float32) / counts[:, 0].astype(np.float32)
        want_gpe = counts[:, 3].astype(np.float32) / counts[:, 1].astype(np.float32)
    assert np.array_equal(got["vde"].cpu().numpy(), want_vde, equal_nan=True) and np.array_equal(got["gpe"].cpu().numpy(), want_gpe, equal_nan=True)
    assert np.isnan(want_vde[3]) and np.isnan(want_gpe[1]) and want_gpe[2] == 1
    dev = got["rmse_cents"].cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(dev), np.isnan(rmse)) and np.isnan(rmse[[1, 2, 3]]).all()
    ok = ~np.isnan(rmse)
    scale = float((np.abs(r32.astype(np.float64) - rmse)[ok] / rmse[ok]).max())
    mine = float((np.abs(dev - rmse)[ok] / rmse[ok]).max())
    print(f"f0_compare: device error {mine:.3e} relative, float32 restatement {scale:.3e}, ratio {mine / scale:.3f}")
    assert scale > 0 and mine <= 8 * scale
    full = metrics.f0_compare(torch.from_numpy(fa).to(DEV), torch.from_numpy(np.nan_to_num(fb)).to(DEV))
    assert full["frames"].tolist() == [F] * B
    again = metrics.f0_compare(torch.from_numpy(dead_a).to(DEV), torch.from_numpy(dead_b).to(DEV), torch.tensor(na), torch.tensor(nb))
    assert all(got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes() for k in got)
