"""CPU: the host side of the GPU resampler - rate ratios, the filter's measured response for every supported pair, the polyphase
table's layout, the float64 restatement against scipy's polyphase resampler, the grouping of a mixed batch."""
import ctypes

import numpy as np
import pytest
import scipy.signal

from genvox_amd import _lib
from genvox_amd import resample as rs
from tests import resample_ref64 as ref

MODEL_RATES = [r for r in rs.RATES if 16000 <= r <= 44100]          # what AudioConfig accepts out of the list
PAIRS = sorted({(s, d) for s in rs.RATES for d in MODEL_RATES if s != d} | {(d, s) for s in rs.RATES for d in MODEL_RATES if s != d})


def test_ratio_length_and_limits():
    assert rs.resample_ratio(48000, 22050) == (147, 320) and rs.resample_ratio(22050, 48000) == (320, 147)
    assert rs.resample_ratio(44100, 22050) == (1, 2) and rs.resample_ratio(16000, 22050) == (441, 320)
    assert rs.resample_ratio(11025, 32000) == (1280, 441) and rs.resample_ratio(22050, 22050) == (1, 1)
    assert max(rs.resample_ratio(s, d)[0] for s, d in PAIRS) == 1280
    assert rs.resampled_length(0, 147, 320) == 0 and rs.resampled_length(1, 147, 320) == 1 and rs.resampled_length(320, 147, 320) == 147
    assert rs.resampled_length(321, 147, 320) == 148 and rs.resampled_length(7, 2, 1) == 14
    for n in (1, 2, 99, 1000, 48001):
        assert rs.resampled_length(n, 147, 320) == ref.resampled_length(n, 147, 320) == int(np.ceil(n * 147 / 320))
    for s, d in PAIRS:
        up, down = rs.resample_ratio(s, d)
        K = rs.taps_per_phase(len(rs.resample_filter(up, down)), up)
        assert K % 4 == 0 and 4 <= K <= rs.MAX_TAPS, (s, d, K)
    with pytest.raises(ValueError, match="up = 22051"):
        rs.check_ratio(*rs.resample_ratio(22050, 22051))
    with pytest.raises(ValueError):
        rs.resample_filter(rs.MAX_UP + 1, 1)
    with pytest.raises(ValueError):
        rs.resample_ratio(0, 22050)


def test_library_says_which_pairs_stage_the_table_and_which_it_refuses():
    lib = _lib.load()   # the in-tree library: a host-side query, no GPU
    q = lib.gvx_resample_uses_lds_table
    assert q(rs.MAX_UP + 1, 68, 1) == -1 and q(0, 68, 1) == -1 and q(147, 70, 1) == -1 and q(147, 0, 1) == -1
    assert q(147, rs.MAX_TAPS + 4, 1) == -1 and q(147, 148, 3) == -1 and q(147, 148, -1) == -1
    assert q(147, 148, 0) == 1 and q(147, 148, 1) == 1 and q(441, 68, 1) == 1 and q(1, 408, 1) == 1    # the everyday pairs
    assert q(640, 68, 1) == 0 and q(1280, 68, 1) == 0 and q(rs.MAX_UP, 68, 0) == 0                      # the 11025 -> 16000 / 32000 class
    assert q(147, 148, 2) == 0 and q(320, 68, 2) == 0 and q(160, 68, 2) == 1                            # float64 rows are twice as wide
    assert lib.gvx_wav_resample_ragged(None, 1, 1, 10, None, 1, 2, None, 68, None, 5, None, None) == -1
    assert b"null" in lib.gvx_last_error()
    assert lib.gvx_wav_mixdown(None, 1, 1, 10, 2, None, None) == -1


def block_shape(lib, up, down, K):
    """(rc, S, R) of gvx_resample_block_shape; S and R stay -7 where the query writes nothing."""
    S, R = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.gvx_resample_block_shape(up, down, K, ctypes.addressof(S), ctypes.addressof(R))
    return rc, S.value, R.value


def test_library_says_which_block_shape_a_ratio_takes():
    lib = _lib.load()   # a host-side query as well
    assert block_shape(lib, 1, 2, 4) == (0, 256, 4)             # 44100 -> 22050 with the shortest table: 256 phases' worth of one phase
    assert block_shape(lib, 147, 320, 148) == (0, 294, 4)       # 48000 -> 22050: two sweeps of the 147 phases
    assert block_shape(lib, 1, 2048, 4) == (0, 1, 2)            # 4 * 2048 + 4 inputs pass the 6144-sample tile: R = 2, and c = 1
    assert block_shape(lib, 1280, 441, 68) == (0, 1280, 4) and block_shape(lib, 2048, 2047, 1024) == (0, 2048, 2)
    for up, down, K in [(0, 2, 4), (rs.MAX_UP + 1, 2, 4), (1, 0, 4), (1, rs.MAX_DOWN + 1, 4), (1, 2, 0), (1, 2, 6), (1, 2, rs.MAX_TAPS + 4), (-1, -1, -4)]:
        assert block_shape(lib, up, down, K) == (-1, -7, -7), (up, down, K)
    one = ctypes.c_int(-7)
    assert lib.gvx_resample_block_shape(1, 2, 4, None, ctypes.addressof(one)) == -1 and lib.gvx_resample_block_shape(1, 2, 4, ctypes.addressof(one), None) == -1
    assert one.value == -7
    # R = 1 cannot be asked for: it needs 2 * down + K > 6144 (span(2 * up) = floor((2 * up - 1) * down / up) + 1 + K <= 2 * down + K),
    # and the limits stop at 2 * 2048 + 1024 = 5120
    assert 2 * rs.MAX_DOWN + rs.MAX_TAPS <= 6144
    for up in (1, 2, 3, 2047, 2048):
        for down in (2047, 2048):
            assert block_shape(lib, up, down, rs.MAX_TAPS)[2] == 2, (up, down)


@pytest.mark.parametrize("up,down,K", [(3, 2, 8), (1, 2048, 4), (7, 5, 12), (147, 320, 148), (2048, 1, 4), (5, 5, 4)])
def test_vectorised_restatement_is_the_loop_form(up, down, K):
    """``resample_vec`` against ``resample`` on rows of 1, K - 1, K and about 500 samples.  The two sum the same terms (the vectorised
    form adds the exact zeros outside the row and the prototype) in different orders, so the bits may differ: both stay within
    1e-15 * (sum of magnitudes) of each other, the magnitudes themselves within the same, and the lengths are equal."""
    rng = np.random.default_rng(up * 4096 + down)
    if (up, down, K) == (147, 320, 148):
        h = rs.resample_filter(up, down)                 # the designer's prototype: its half is no multiple of up
        assert rs.taps_per_phase(len(h), up) == K
    else:
        h = ref.prototype(rng.uniform(-1.0, 1.0, size=(up, K)))
    for n in (1, K - 1, K, 503 if up < 2048 else 9):     # up = 2048, down = 1: 2048 outputs per sample
        x = rng.uniform(-1.0, 1.0, size=n)
        want, want_mag = ref.resample(x, h, up, down)
        got, got_mag = ref.resample_vec(x, h, up, down)
        assert got.shape == want.shape == got_mag.shape == (ref.resampled_length(n, up, down),)
        assert (np.abs(got - want) <= 1e-15 * want_mag).all(), (n, np.abs(got - want).max())
        assert (np.abs(got_mag - want_mag) <= 1e-15 * want_mag).all(), n
        wide, wide_mag = ref.resample_vec(x, h, up, down, wide=True)      # the same sums carried in long double, rounded once
        assert wide.dtype == wide_mag.dtype == np.float64 and (np.abs(wide - want) <= 1e-15 * want_mag).all() and (np.abs(wide_mag - want_mag) <= 1e-15 * want_mag).all()
    assert ref.resample_vec(np.zeros(0), h, up, down)[0].shape == (0,)


@pytest.mark.parametrize("up,K", [(1, 4), (3, 8), (7, 12), (160, 68), (2048, 4), (2, 1020)])
def test_full_table_and_prototype_round_trip(up, K):
    """``prototype`` is the inverse of the designer's ``polyphase_table`` for a table with every tap in use.  The prototype has
    K * up + 1 taps (the last a zero), for which the designer lays out K + 4 columns: the table between two columns of zeros."""
    table = np.random.default_rng(up + K).uniform(-1.0, 1.0, size=(up, K))
    h = ref.prototype(table)
    assert h.shape == (K * up + 1,) and h[-1] == 0.0 and np.count_nonzero(h) == up * K
    back = rs.polyphase_table(h, up, np.float64)
    assert back.shape == (up, K + 4) and np.array_equal(back[:, 2:-2], table) and not back[:, :2].any() and not back[:, -2:].any()
    # the header's own statement of the layout: table[p][k] = h[p + (K / 2 - 1 - k) * up], h centred
    half = (K // 2) * up
    for p, k in [(0, 0), (up - 1, K - 1), (up // 2, K // 2), (0, K - 1), (up - 1, 0)]:
        assert table[p, k] == h[half + p + (K // 2 - 1 - k) * up]
    # the designer's own inverse wraps around at the one tap the table does not hold
    assert rs.prototype_from_table(table, len(h))[-1] == table[0, -1] != 0.0


@pytest.mark.parametrize("src,dst", PAIRS)
def test_filter_meets_its_two_bars(src, dst):
    """On a zero-padded FFT of the prototype: pass band (0 .. 0.85 x the lower Nyquist) within 0.01 dB of unit gain, everything from
    1.05 x the lower Nyquist up at least 96 dB down (below a 16-bit LSB)."""
    up, down = rs.resample_ratio(src, dst)
    h = rs.resample_filter(up, down)
    assert len(h) % 2 == 1 and np.array_equal(h, h[::-1])
    n = 1 << int(np.ceil(np.log2(len(h) * 8)))
    gain = np.abs(np.fft.rfft(h, n)) / up
    f = np.arange(len(gain)) / n * 2 * max(up, down)          # frequency in units of the lower Nyquist
    assert np.abs(20 * np.log10(gain[f <= 0.85])).max() <= 0.01
    assert -20 * np.log10(gain[f >= 1.05].max()) >= 96.0


@pytest.mark.parametrize("src,dst", PAIRS)
def test_table_is_the_prototype_and_every_phase_has_unit_gain(src, dst):
    up, down = rs.resample_ratio(src, dst)
    h = rs.resample_filter(up, down)
    t64 = rs.polyphase_table(h, up, np.float64)
    K = rs.taps_per_phase(len(h), up)
    assert t64.shape == (up, K) and t64.flags.c_contiguous
    assert np.array_equal(rs.prototype_from_table(t64, len(h)), h)
    assert np.count_nonzero(t64) == np.count_nonzero(h)                     # the rest of every row is padding
    assert np.array_equal(rs.polyphase_table(h, up), t64.astype(np.float32))
    assert np.abs(t64.sum(axis=1) - 1.0).max() <= 1e-3                      # per-phase gain ripple: what would be heard as a tone
    # the order the kernel reads: tap k of row p = (m * down) % up multiplies input q - (K / 2 - 1) + k, q = (m * down) // up
    x = np.random.default_rng(src + dst).standard_normal(3 * K)
    m = len(x) * up // (2 * down)
    q, p = divmod(m * down, up)
    j = q - (K // 2 - 1) + np.arange(K)
    ok = (j >= 0) & (j < len(x))
    want, _ = ref.resample(x, h, up, down)
    assert abs((t64[p][ok] * x[j[ok]]).sum() - want[m]) <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("src,dst", [(22050, 44100), (44100, 22050), (48000, 22050), (16000, 22050)])
def test_restatement_agrees_with_scipy_resample_poly(src, dst):
    """An independent float64 second opinion, given the same prototype as ``window`` (scipy multiplies the window by ``up``; ours
    already carries that gain)."""
    up, down = rs.resample_ratio(src, dst)
    h = rs.resample_filter(up, down)
    x = np.random.default_rng(7).standard_normal(1501)
    got, mag = ref.resample(x, h, up, down)
    want = scipy.signal.resample_poly(x, up, down, window=h / up)
    assert got.shape == want.shape == (rs.resampled_length(len(x), up, down),)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max()
    assert (mag >= np.abs(got) - 1e-12).all()


def test_groups_map_a_mixed_batch_and_back():
    keys = [(48000, 1, "i"), (22050, 1, "i"), (44100, 2, "f"), (48000, 1, "i"), (22050, 1, "f"), (44100, 2, "f"), (48000, 2, "i")]
    groups = rs.plan_groups(keys)
    assert [k for k, _ in groups] == [(48000, 1, "i"), (22050, 1, "i"), (44100, 2, "f"), (22050, 1, "f"), (48000, 2, "i")]
    assert [idx for _, idx in groups] == [[0, 3], [1], [2, 5], [4], [6]]
    assert sorted(i for _, idx in groups for i in idx) == list(range(len(keys)))
    back = rs.scatter_groups(groups, [[f"r{i}" for i in idx] for _, idx in groups])
    assert back == [f"r{i}" for i in range(len(keys))]
    with pytest.raises(ValueError):
        rs.scatter_groups(groups, [[0]] * len(groups))
    assert rs.plan_groups([]) == []


def test_mixdown_restatement():
    frames = np.array([[1, 2], [32767, 32767], [-32768, 32767], [3, -4]], dtype=np.int16)
    assert ref.mixdown(frames).tolist() == [1.5, 32767.0, -0.5, -0.5]
