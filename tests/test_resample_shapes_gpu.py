"""The resampler's block shapes, table sizes and grids, and the mix-down's channel counts, that tests/test_resample_gpu.py never
runs: caller-made tables through the C ABI, every output sample against the float64 restatement (tests/resample_ref64.py).

The tables are full: all K taps of every one of the `up` rows are random, uniform in [-1, 1], rounded to the table's type and kept
in float64 for the restatement - no padded zero taps that could hide an off-by-one at a row's end, no two phases alike.  Around
every row's bounds lies poison (+-32767 for int16, NaN otherwise), the output buffer is NaN beforehand with a stride a few samples
past what is needed, out_lengths is -1.  The bound per output is the one of tests/test_resample_gpu.py, unchanged:
|got - want| <= (K + 2) * u * sum |h * x|, u = 2^-24 for int16 and float32 and 2^-53 for float64; behind a row's length exact zeros.
Every case asserts the block shape (gvx_resample_block_shape) and the table path it was chosen for, and prints its largest
error / bound ratio (pytest -s shows it).

Measured on the MI355X (256 CUs), largest error / bound ratio over all cases of this file: int16 0.48, float32 0.48, float64 0.61
(against the restatement carried in long double), all three at (up, down, K) = (1, 2, 4) over 2304 blocks; K = 1024 stays below 0.01.
"""
import ctypes

import numpy as np
import pytest
import torch

from genvox_amd import _lib
from genvox_amd import resample as rs
from tests import resample_ref64 as ref
from tests.test_resample_gpu import KINDS, check_row, processor, signal

pytestmark = pytest.mark.gpu

TILE_SAMPLES, LDS_BYTES, MAX_PER_CU = 6144, 160 * 1024, 4      # of the kernel's plan (csrc/resample.hip), restated for the grid


@pytest.fixture(scope="module")
def ap():
    return processor()


def block_shape(up, down, K):
    S, R = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.load().gvx_resample_block_shape(up, down, K, ctypes.addressof(S), ctypes.addressof(R)) == 0
    return S.value, R.value


def random_table(rng, up, K, kind):
    """(table in its own type, the float64 prototype of exactly those values)"""
    table = rng.uniform(-1.0, 1.0, size=(up, K)).astype(np.float64 if kind == "float64" else np.float32)
    return table, ref.prototype(table)


def poison(rng, shape, kind):
    if kind == "int16":
        return np.where(rng.random(shape) < 0.5, 32767, -32767).astype(np.int16)
    return np.full(shape, np.nan, KINDS[kind][0])


class Call:
    """One gvx_wav_resample_ragged call over `rows` laid into a poisoned [B][n_max] batch at `lefts`; `bounds` overrides the
    bounds that the rows' places imply (the rows then only say where signal is laid)."""

    def __init__(self, ap, rng, kind, rows, lefts, up, down, K, table_dev, n_max=None, bounds=None):
        self.ap, self.kind, self.B = ap, kind, len(rows)
        self.n_max = max(l + len(x) for l, x in zip(lefts, rows)) + 3 if n_max is None else n_max
        pcm = poison(rng, (self.B, self.n_max), kind)
        for b, x in enumerate(rows):
            pcm[b, lefts[b]: lefts[b] + len(x)] = x
        self.x = torch.from_numpy(pcm).to(ap.device)
        own = [[l, l + len(x)] for l, x in zip(lefts, rows)]
        self.bounds = torch.tensor(own if bounds is None else bounds, dtype=torch.int32, device=ap.device)
        self.stride = rs.resampled_length(self.n_max, up, down) + 5
        self.args = (up, down, table_dev, K)

    def run(self):
        up, down, table_dev, K = self.args
        out = torch.full((self.B, self.stride), float("nan"), dtype=torch.float64 if self.kind == "float64" else torch.float32, device=self.ap.device)
        lengths = torch.full((self.B,), -1, dtype=torch.int32, device=self.ap.device)
        _lib.check(_lib.load().gvx_wav_resample_ragged(self.x.data_ptr(), KINDS[self.kind][1], self.B, self.n_max, self.bounds.data_ptr(), up, down,
                                                       table_dev.data_ptr(), K, out.data_ptr(), self.stride, lengths.data_ptr(), self.ap._stream()))
        return out, lengths


def check_rows(out, lengths, rows, h, up, down, K, kind, what):
    """Every sample of every row against ``resample_vec`` under the bound of ``check_row``; prints and returns the largest
    error / bound ratio, printed before anything is asserted."""
    host, lens, u = out.cpu().numpy().astype(np.float64), lengths.tolist(), KINDS[kind][2]
    ratios, wants = [], []
    for b, x in enumerate(rows):
        want, mag = ref.resample_vec(x, h, up, down, wide=kind == "float64")
        wants.append(want)
        ratios.append(float((np.abs(host[b, : len(want)] - want) / ((K + 2) * u * mag + 1e-300)).max()) if len(want) == lens[b] and len(want) else 0.0)
    worst = max(ratios) if np.isfinite(ratios).all() else float("nan")
    print(f"{what}: largest error / bound = {worst:.3f}")
    for b, x in enumerate(rows):
        n_out = rs.resampled_length(len(x), up, down)
        assert lens[b] == n_out == len(wants[b]), (what, b, lens[b], n_out)
        assert np.isfinite(host[b]).all(), (what, b)
        assert ratios[b] <= 1.0, (what, b, len(x), ratios[b])
        assert not host[b, n_out:].any(), (what, b)
    return worst


def edge_sizes(up, down, K, block):
    """Row lengths of a shape case: 1, K - 1, K samples, then rows whose output ends one sample before, on, one sample behind a
    block's end and one behind two blocks.  With up > down the lengths ceil(n * up / down) skip values: the nearest length on the
    side asked for is taken (the last row that ends before the block's end, the first that ends behind it)."""
    at_most = lambda t: (t * down) // up                # noqa: E731  the largest n with ceil(n * up / down) <= t
    at_least = lambda t: ((t - 1) * down) // up + 1     # noqa: E731  the smallest n with ceil(n * up / down) >= t
    around = [at_most(block - 1), at_most(block), at_least(block + 1), at_least(2 * block + 1)]
    n_outs = [rs.resampled_length(n, up, down) for n in around]
    if up <= down:
        assert n_outs == [block - 1, block, block + 1, 2 * block + 1], n_outs
    else:
        assert n_outs[0] < block <= n_outs[0] + -(-up // down) and n_outs[1] <= block < n_outs[2] <= block + -(-up // down) and n_outs[3] > 2 * block
    sizes = []
    for n in [1, K - 1, K] + around:
        if n >= 1 and n not in sizes:
            sizes.append(n)
    return sizes


R2_TRIPLES = [(1, 2048, 4, 1), (1, 2048, 1024, 1), (3, 2048, 64, 3), (64, 1500, 200, 64), (128, 2047, 4, 128), (255, 1400, 1024, 255),
              (2047, 2048, 8, 2047), (2048, 2047, 1024, 2048)]
# (up, down, K, S, R, table in LDS for float32 outputs, for float64 outputs)
SHAPES = [(u, d, K, S, 2, int((u, K) not in [(255, 1024), (2048, 1024)]), int((u, K) not in [(255, 1024), (2048, 1024), (2047, 8)])) for u, d, K, S in R2_TRIPLES] + [
    (1, 1, 4, 256, 4, 1, 1),            # nothing to convert: 256 outputs of the one phase per sweep
    (2048, 1, 4, 2048, 4, 1, 1),        # the most phases: eight passes of a workgroup's 256 threads over S, 2048 outputs per input sample
    (2, 3, 1024, 256, 4, 1, 1),         # the longest rows, c = 128 sweeps per S
    (7, 1300, 1024, 7, 4, 1, 1),        # c shrinks from 37 to 1: S = 7, less than a wave
    (300, 7, 12, 300, 4, 1, 1),
    (64, 1491, 200, 64, 4, 1, 1),       # the last down with R = 4 at up = 64, K = 200 ...
    (64, 1492, 200, 64, 2, 1, 1),       # ... and the first with R = 2
]


def test_the_shape_cases_cover_what_they_are_there_for():
    """R = 2 with S of 1, 3, 64, 128, 255, 2047 and 2048, S below a wave at R = 4, both table paths per output type, and the step from
    R = 4 to R = 2 between two neighbouring `down`: asked of the library, so that a change to the plan cannot quietly empty a case."""
    lib = _lib.load()
    for up, down, K, S, R, lds32, lds64 in SHAPES:
        assert block_shape(up, down, K) == (S, R), (up, down, K)
        assert [lib.gvx_resample_uses_lds_table(up, K, k) for k in (0, 1, 2)] == [lds32, lds32, lds64], (up, down, K)
    assert {S for _, _, _, S, R, _, _ in SHAPES if R == 2} == {1, 3, 64, 128, 255, 2047, 2048}
    assert {c[5] for c in SHAPES} == {0, 1} and {c[6] for c in SHAPES} == {0, 1}
    assert {c[5] for c in SHAPES if c[4] == 2} == {0, 1}      # R = 2 blocks on both table paths as well
    assert max(c[0] for c in SHAPES) == rs.MAX_UP and max(c[1] for c in SHAPES) == rs.MAX_DOWN
    assert {c[2] for c in SHAPES} >= {4, rs.MAX_TAPS}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "-".join(map(str, c[:3])))
def test_block_shapes_against_the_restatement(ap, kind, shape):
    """One call per shape: rows of 1, K - 1 and K samples, rows that end around one block's end and behind two blocks, a row with
    left > 0; the call repeated gives the same bits.  No row had to be dropped for size: the largest case, (2048, 1, 4), writes about
    150 000 outputs."""
    up, down, K, S, R, lds32, lds64 = shape
    assert block_shape(up, down, K) == (S, R)
    assert _lib.load().gvx_resample_uses_lds_table(up, K, KINDS[kind][1]) == (lds64 if kind == "float64" else lds32)
    rng = np.random.default_rng(up * 7919 + down * 31 + K)
    table, h = random_table(rng, up, K, kind)
    table_dev = torch.from_numpy(table).to(ap.device)
    block = R * S
    sizes = edge_sizes(up, down, K, block)
    lefts = [0, 3, 0, 1, 0, 17, 2][: len(sizes)]
    sizes.append(max(2, sizes[-1] // 3))
    lefts.append(5)                                     # and one more row that does not start at its buffer's start
    rows = [signal(rng, n, kind) for n in sizes]
    call = Call(ap, rng, kind, rows, lefts, up, down, K, table_dev)
    assert call.B * call.stride <= 300_000
    out, lengths = call.run()
    check_rows(out, lengths, rows, h, up, down, K, kind, f"shape {(up, down, K)} S={S} R={R} {kind}")
    again, l2 = call.run()
    assert torch.equal(out, again) and torch.equal(lengths, l2)


def launch_grid(up, K, kind, total, cus):
    """The grid the launcher gives `total` output blocks: as many workgroups per CU as their LDS lets a CU hold, 4 at the most."""
    size = 8 if kind == "float64" else 4
    per = 16 // size
    slots = K // per + (1 - (K // per) % 2)              # the LDS image's row stride: an odd number of 16-byte slots
    staged = _lib.load().gvx_resample_uses_lds_table(up, K, KINDS[kind][1])
    lds = ((up * slots * per if staged else 0) + TILE_SAMPLES) * size
    per_cu = min(MAX_PER_CU, LDS_BYTES // lds)
    return min(total, per_cu * cus), per_cu, staged


@pytest.mark.parametrize("up,down,K,kind,per_cu,staged", [(441, 160, 68, "float32", 1, 1), (1, 2, 4, "int16", 4, 1), (1, 2, 4, "float32", 4, 1), (1, 2, 4, "float64", 3, 1),
                                                         (640, 441, 68, "float32", 4, 0)])
def test_workgroups_that_take_a_second_and_a_third_block(ap, up, down, K, kind, per_cu, staged):
    """More than two blocks per workgroup of the grid: 8 rows of equal length with total blocks >= 2 * grid + grid / 4, so some
    workgroups walk three blocks and some two, and blocks of different rows pass through one workgroup over one staged table.
    Every sample against the restatement; every row bit-equal to the same row in a call of its own (where no workgroup takes a
    second block); the call repeated gives the same bits."""
    cus = torch.cuda.get_device_properties(ap.device).multi_processor_count
    S, R = block_shape(up, down, K)
    block, B = R * S, 8
    full, got_per_cu, got_staged = launch_grid(up, K, kind, 1 << 40, cus)
    assert (got_per_cu, got_staged) == (per_cu, staged)
    per_row = -(-(2 * full + full // 4) // B)
    n = ((per_row * block - block // 3) * down) // up               # the rows end inside their last block
    rng = np.random.default_rng(up + down)
    table, h = random_table(rng, up, K, kind)
    table_dev = torch.from_numpy(table).to(ap.device)
    rows = [signal(rng, n, kind) for _ in range(B)]
    call = Call(ap, rng, kind, rows, [0] * B, up, down, K, table_dev)
    total = B * -(-call.stride // block)
    grid = launch_grid(up, K, kind, total, cus)[0]
    assert grid == full and total >= 2 * grid + grid // 4 and total > grid, (total, grid)
    assert -(-call.stride // block) % grid != 0                     # a workgroup's blocks do not all sit at one place of their rows
    out, lengths = call.run()
    check_rows(out, lengths, rows, h, up, down, K, kind, f"{total} blocks on {grid} workgroups {(up, down, K)} {kind}")
    again, l2 = call.run()
    assert torch.equal(out, again) and torch.equal(lengths, l2)
    for b, x in enumerate(rows):
        alone = Call(ap, rng, kind, [x], [0], up, down, K, table_dev)
        assert -(-alone.stride // block) <= grid
        o1, l1 = alone.run()
        assert l1.tolist() == [lengths[b].item()] and torch.equal(o1[0], out[b, : alone.stride]), (kind, b)


@pytest.mark.parametrize("kind", ["int16", "float64"])
@pytest.mark.parametrize("src,dst,up,down,S,R,lds32", [(22050, 8000, 160, 441, 320, 4, 1), (22050, 96000, 640, 147, 640, 4, 0), (44100, 8000, 80, 441, 240, 4, 1),
                                                        (96000, 11025, 147, 1280, 147, 4, 0), (22050, 48000, 320, 147, 320, 4, 1)])
def test_designer_pairs_that_end_at_other_rates(ap, kind, src, dst, up, down, S, R, lds32):
    """Pairs that ``resample`` and ``tts(..., sampling_rate)`` reach and no test ran: 22050 -> 96000 reads a float32 table from global
    memory, 44100 -> 8000 shrinks c from 4 to 3, 96000 -> 11025 (down 1280, K 588) from 2 to 1."""
    assert rs.resample_ratio(src, dst) == (up, down)
    K = rs.taps_per_phase(len(rs.resample_filter(up, down)), up)
    assert block_shape(up, down, K) == (S, R) and _lib.load().gvx_resample_uses_lds_table(up, K, 0) == lds32
    rng = np.random.default_rng(src + dst)
    rows = [signal(rng, n, kind) for n in (1500, 1, 377)]
    out, lengths = ap.resample(rows, src, dst)
    assert out.dtype == (torch.float64 if kind == "float64" else torch.float32) and out.shape == (3, rs.resampled_length(1500, up, down))
    host, lens = out.cpu().numpy(), lengths.tolist()
    for b, x in enumerate(rows):
        check_row(host[b], lens[b], x, src, dst, kind, (src, dst, kind, b))


@pytest.mark.parametrize("kind", list(KINDS))
def test_bounds_are_clamped_on_the_device(ap, kind):
    """left == right, left > right, a negative left, a right behind the buffer, left at the buffer's end: the lengths and signals are
    those of the bounds clamped to [0, n_max], an empty row is length 0 and all zeros."""
    up, down, K = 7, 5, 12
    assert block_shape(up, down, K) == (259, 4)
    rng = np.random.default_rng(75)
    table, h = random_table(rng, up, K, kind)
    table_dev = torch.from_numpy(table).to(ap.device)
    n_max = 1600
    #          signal laid at        bounds given                clamped
    spec = [((40, 0), (40, 40)),                               # left == right: empty
            ((0, 0), (900, 300)),                              # left > right: empty
            ((0, 300), (-5, 300)),                             # [0, 300)
            ((10, n_max - 10), (10, n_max + 100)),             # [10, n_max)
            ((0, 0), (n_max, n_max + 100)),                    # [n_max, n_max): empty
            ((0, n_max), (-(2 ** 31), 2 ** 31 - 1)),           # the whole buffer
            ((700, 1), (700, 701))]                            # and one everyday row beside them
    rows = [signal(rng, n, kind) for (_, n), _ in spec]
    call = Call(ap, rng, kind, rows, [l for (l, _), _ in spec], up, down, K, table_dev, n_max=n_max, bounds=[list(b) for _, b in spec])
    out, lengths = call.run()
    assert lengths.tolist() == [0, 0, 420, 2226, 0, 2240, 2]
    check_rows(out, lengths, rows, h, up, down, K, kind, f"clamped bounds {kind}")
    assert not out[[0, 1, 4]].any()


# ---- mix-down ------------------------------------------------------------------------------------------------------------------------
def mixdown_call(ap, x, kind, B, n_max, channels):
    mono = torch.full((B, n_max), float("nan"), dtype=torch.float32, device=ap.device)
    _lib.check(_lib.load().gvx_wav_mixdown(x.data_ptr(), KINDS[kind][1], B, n_max, channels, mono.data_ptr(), ap._stream()))
    return mono


def frames_of(rng, n, channels, kind):
    frames = np.stack([signal(rng, n, kind) for _ in range(channels)], axis=1)
    if kind == "int16":
        frames[:4] = [[32767] * channels, [-32768] * channels, [32767, -32768] + [1] * (channels - 2), [1, 2] + [0] * (channels - 2)]
    return frames


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("channels", [2, 3, 4, 6, 7, 8])
def test_mixdown_of_every_channel_count_aligned_or_not(ap, kind, channels):
    """The float64 mean rounded once, exactly; for 2 and 4 channels (one vector load per frame where the batch is aligned to a
    frame) also from a buffer that starts one sample past an aligned address, which must give the aligned call's bits."""
    n = 3001
    frames = frames_of(np.random.default_rng(100 + channels), n, channels, kind)
    want = ref.mixdown(frames)
    x = torch.from_numpy(frames).to(ap.device)
    size = x.element_size()
    mono = mixdown_call(ap, x, kind, 1, n, channels)
    assert np.array_equal(mono[0].cpu().numpy(), want)
    if channels in (2, 4):
        assert x.data_ptr() % (size * channels) == 0                # that was the vector form
        big = torch.zeros(n * channels + 8, dtype=x.dtype, device=ap.device)
        view = big[1: 1 + n * channels]
        view.copy_(x.reshape(-1))
        assert view.data_ptr() % (size * channels) == size
        assert torch.equal(mixdown_call(ap, view, kind, 1, n, channels), mono)


def test_mixdown_of_more_frames_than_one_sweep_of_the_grid(ap):
    """3 x 350 000 stereo int16 frames: the grid stops at 4096 blocks of 256 threads = 1 048 576 frames, the rest is the loop's
    second round."""
    B, n = 3, 350_000
    assert B * n > 4096 * 256
    frames = frames_of(np.random.default_rng(9), B * n, 2, "int16")
    mono = mixdown_call(ap, torch.from_numpy(frames).to(ap.device), "int16", B, n, 2)
    assert np.array_equal(mono.cpu().numpy().reshape(-1), ref.mixdown(frames))
