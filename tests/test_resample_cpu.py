"""CPU: the host side of the GPU resampler - rate ratios, the filter's measured response for every supported pair, the polyphase
table's layout, the float64 restatement against scipy's polyphase resampler, the grouping of a mixed batch."""
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
