"""Case tables of the pitch edge tests: parameter sets of gvx_pitch_yin and of gvx_psola_plan / gvx_psola_synth that reach the code
paths the kernels' first tests never ran (tests/test_pitch_edges_cpu.py proves on the references alone that every case reaches the
path it is named for and respects the GPU tests' conditions; tests/test_pitch_edges_gpu.py and tests/test_pitch_control_edges_gpu.py
run the cases).  Inputs are drawn as tests/test_pitch_gpu.py and tests/test_pitch_control_gpu.py draw theirs (batch and make_batch,
imported); the references are tests/pitch_ref64.py and tests/psola_ref.py, unchanged, and so are their bounds."""
import collections

import numpy as np

from tests import pitch_ref64 as Y
from tests import psola_ref as R
from tests.test_pitch_control_gpu import SMALL as PS_SMALL
from tests.test_pitch_control_gpu import make_batch
from tests.test_pitch_gpu import DEFAULT, SMALL, WIDE, batch

# ---- YIN -------------------------------------------------------------------------------------------------------------------------

# name, parameters, row lengths, N, seed of the generator, first_centre, what the case claims (checked on the CPU), what it is there for
YinCase = collections.namedtuple("YinCase", "name p lengths N seed first_centre claims why")

RAGGED = [0, 5, 90, 47, 48, 49, 240, 256, 257, 515, 400]   # the rows of test_row_edges_small_configuration
RAGGED_N = 528
DEFAULT_RAGGED = [24 * 256, 24 * 256 - 1, 23 * 256 + 1, 1300, 0]   # the rows of test_default_parameters, seed 11
SEED = 7


def _small(name, why, claims=(), first_centre=0, **change):
    return YinCase(name, {**SMALL, **change}, RAGGED, RAGGED_N, SEED, first_centre, tuple(claims), why)


WINDOW_CASES = [_small(f"W{W}", "py_block<false> " + ("alone" if W < 64 else "behind full blocks"), ("tail",), window=W)
                for W in (32, 33, 63, 65, 100, 127)] + [
    YinCase("W1000_default", {**DEFAULT, "window": 1000}, DEFAULT_RAGGED, 24 * 256, 11, 0, ("tail",), "15 full blocks and 40 terms"),
    YinCase("W2047_lag1023", {**WIDE, "window": 2047, "lag_max": 1023}, [6000, 3000], 6000, SEED, 0, ("tail",), "31 full blocks and 63 terms"),
    _small("W64_negative_centre", "the default set on a grid that starts before the row", first_centre=-21),
]

TILE_FRAMES = {700: (14, 35), 1024: (9, 19), 4096: (3, 7), 9300: (1, 3)}   # hop -> (frames of a workgroup, F of the longest row)
TILE_CASES = [YinCase(f"tile{tile}_hop{hop}", {**WIDE, "hop": hop}, [hop * F, hop * F - hop - 1, 3000], hop * F, SEED, 0, (),
                      f"{tile} frames per workgroup: a full tile, a partial last tile, a short row")
              for hop, (tile, F) in TILE_FRAMES.items()]

LAG_CASES = [_small(f"lag4_{m}", why, claims, lag_max=m) for m, claims, why in (
    (41, (), "n_lags 42: a multiple of 3"), (42, ("mod3",), "n_lags 43: the last lane is clamped by 2"),
    (64, (), "chunk 1, every lane owns a lag"), (65, (), "chunk 2: lanes 33 .. 63 own none"),
    (128, (), "chunk 2, every lane owns two"), (129, (), "chunk 3: 43 lanes own lags"),
    (191, (), "n_lags 192: one pass, full"), (192, ("mod3",), "n_lags 193: a second pass of one lane, clamped by 2"),
    (193, (), "n_lags 194: a second pass of one lane, clamped by 1"))] + [
    _small("lag1_2", "the smallest table: tau0 = 0 for every lane, one lag scanned", lag_min=1, lag_max=2),
    _small("lag9_10", "one lag scanned", lag_min=9, lag_max=10),
]

THRESHOLD_CASES = [_small(f"threshold{t:g}", "the unvoiced minimum alone" if t < 0.1 else "a threshold other than 0.15", threshold=t)
                   for t in (1e-6, 0.5, 0.9)]

# the grid's limit in rows: 65535 rows of 64 samples that repeat with period 8 - rows and lengths
GRID_ROWS, GRID_N, GRID_PERIOD = 65535, 64, 8
GRID_CASE = YinCase("grid8", dict(SMALL), [64, 63, 49, 48, 17, 5, 0, 33], GRID_N, SEED, 0, (), "the batch of 8 the 65535 rows repeat")

YIN_CASES = WINDOW_CASES + TILE_CASES + LAG_CASES + THRESHOLD_CASES + [GRID_CASE]
YIN_BY_NAME = {c.name: c for c in YIN_CASES}
assert len(YIN_BY_NAME) == len(YIN_CASES)

_YIN_REF = {}


def yin_input(case) -> np.ndarray:
    return batch(case.lengths, case.N, case.p["sampling_rate"], case.seed)


def yin_reference(case):
    """(wav, float64 restatement), computed once per process."""
    if case.name not in _YIN_REF:
        x = yin_input(case)
        _YIN_REF[case.name] = (x, Y.yin(x, case.lengths, first_centre=case.first_centre, **case.p))
    return _YIN_REF[case.name]


def marginal_frames(ref, p):
    """(marginal, total) as tests.test_pitch_gpu.hold counts them: a frame whose decision margin is not above the table's bound, or
    whose parabola is not determined to a useful width (f0_tolerance gives None)."""
    bound = Y.table_bound(p["window"], p["lag_max"])
    marginal = total = 0
    for b, Fb in enumerate(ref["frames"]):
        for f in range(int(Fb)):
            total += 1
            lag = int(ref["lag"][b, f])
            if ref["margin"][b, f] <= bound or (lag >= 0 and Y.f0_tolerance(ref["cmnd"][b, f], lag, p["sampling_rate"], bound)[0] is None):
                marginal += 1
    return marginal, total


# ---- PSOLA -----------------------------------------------------------------------------------------------------------------------

PS_DEFAULT = dict(hop=256, lag_min=44, lag_max=368, unvoiced_period=220)
PS_STAGE = 4096   # samples the plan's wave holds at a time (csrc/psola.hip)

# name, grid, row lengths, first_centre, seed, kind of input (plain | ties | lags | ratios), claims, what it is there for
PsolaCase = collections.namedtuple("PsolaCase", "name cfg lengths first_centre seed kind claims why")

_DEFAULT_ROWS = [13001, 9000, 4097, 300, 0]
PSOLA_CASES = [PsolaCase(f"default_fc{fc}", PS_DEFAULT, _DEFAULT_ROWS, fc, 50, "plain", ("wide", "chunks"),
                         "the 22050 Hz grid: runs of up to 3 samples per lane, the staged chunk moves three times" +
                         ("" if fc == 0 else "; frames clamp to 0 and F_b - 1 hops off the row's ends"))
               for fc in (0, -3000, 3000)] + [
    PsolaCase("limits", dict(hop=256, lag_min=32, lag_max=1024, unvoiced_period=1024), [20000, 12345, 2049, 1], 0, 51, "plain",
              ("wide", "chunks"), "P = 1024: the restaging rule moves half a chunk at a time, the synthesis' LDS at its largest"),
    PsolaCase("U_above_lag_max", dict(hop=16, lag_min=4, lag_max=40, unvoiced_period=100), [1000, 513, 40], 0, 52, "plain", (), "P = U = 100"),
    PsolaCase("hop1", dict(hop=1, lag_min=4, lag_max=40, unvoiced_period=20), [5000, 4100, 63], 0, 53, "plain", ("chunks",),
              "a frame per sample: PS_STAGE + 4 staged frames"),
    PsolaCase("hop5000", dict(hop=5000, lag_min=4, lag_max=40, unvoiced_period=20), [12000, 5001, 4999], 0, 54, "plain", ("chunks",),
              "a staged chunk inside one frame"),
    PsolaCase("p_min1", dict(hop=16, lag_min=1, lag_max=8, unvoiced_period=1), [700, 257], 0, 55, "plain", (),
              "a mark and a grain at every sample, K = J = N + 1"),
    PsolaCase("ties", PS_DEFAULT, [9000, 5000, 3000], 0, 56, "ties", ("wide", "chunks", "ties"),
              "clipped and constant rows: the maximum occurs more than once, in more than one lane's run"),
    PsolaCase("lags_out_of_range", PS_DEFAULT, [9000, 4097, 300], 0, 57, "lags", ("chunks", "lag_kinds"), "lags 0, -5, 1 and 5000 among lags in range"),
    PsolaCase("ratios", PS_SMALL, [300, 257, 200, 333, 400], 0, 58, "ratios", (), "ratios one float32 outside [0.5, 2], infinities, and the limits themselves"),
]
PSOLA_BY_NAME = {c.name: c for c in PSOLA_CASES}
assert len(PSOLA_BY_NAME) == len(PSOLA_CASES)

CLIP = 0.25
LAG_KINDS = ("zero", "minus5", "one", "5000", "in_range")
BAD_RATIOS = (np.float32(0.49999997), np.float32(2.0000002), np.float32(np.inf), np.float32(-np.inf))   # 0.5 - 2^-25, 2 + 2^-22
RATIO_FRAME = 7

_PS_IN, _PS_REF = {}, {}


def lag_kinds(case):
    """Per row the kind (index into LAG_KINDS) of every frame of the "lags" input: a fifth of the frames each, shuffled."""
    rng = np.random.default_rng(case.seed + 1000)
    return [rng.permutation(np.arange(R.frames_of(n, case.cfg["hop"])) % 5) for n in case.lengths]


def psola_input(case):
    """(wav, lengths, lag, ratio) with make_batch's poison behind every row; computed once per process, not to be written to."""
    if case.name in _PS_IN:
        return _PS_IN[case.name]
    cfg = case.cfg
    wav, lengths, lag, ratio = make_batch(case.lengths, max(case.lengths), case.seed, case.first_centre, cfg)
    if case.kind == "ties":
        wav = np.clip(wav, -CLIP, CLIP)   # after the noise; NaN stays NaN
        wav[1, :case.lengths[1]] = 0.1
    elif case.kind == "lags":
        rng = np.random.default_rng(case.seed + 2000)
        for b, kinds in enumerate(lag_kinds(case)):
            inside = rng.integers(cfg["lag_min"], cfg["lag_max"] + 1, len(kinds))
            lag[b, :len(kinds)] = np.choose(kinds, [0, -5, 1, 5000, inside])
    elif case.kind == "ratios":
        for b, q in enumerate(BAD_RATIOS):
            ratio[b, :R.frames_of(case.lengths[b], cfg["hop"])] = 1.0
            ratio[b, RATIO_FRAME] = q
        Fb = R.frames_of(case.lengths[4], cfg["hop"])
        ratio[4, :Fb] = np.where(np.arange(Fb) % 2 == 0, 0.5, 2.0)
    _PS_IN[case.name] = (wav, lengths, lag, ratio)
    return _PS_IN[case.name]


def psola_reference(case):
    """The float64 restatement of the case (its K / J assertions run inside), computed once per process."""
    if case.name not in _PS_REF:
        wav, lengths, lag, ratio = psola_input(case)
        _PS_REF[case.name] = R.psola(wav, lengths, lag, ratio, first_centre=case.first_centre, **case.cfg)
    return _PS_REF[case.name]


def search_windows(case, b):
    """The peak searches of row b, from the reference's marks: (lo, hi) of every voiced candidate, as the definition states them."""
    wav, lengths, lag, _ = psola_input(case)
    ref, cfg, n = psola_reference(case), case.cfg, int(lengths[b])
    g = R.Grid(n, lag[b], cfg["hop"], case.first_centre, cfg["lag_min"], cfg["lag_max"], cfg["unvoiced_period"])
    marks, periods = ref["marks"][b], [abs(p) for p in ref["periods"][b]]
    out = []
    for k in range(len(marks)):
        prev = marks[k - 1] if k else -1
        c = prev + periods[k - 1] if k else 0
        if g.voiced_at(c):
            r = (min(g.period_at(c), periods[k - 1]) if k else g.period_at(0)) // 4
            out.append((max(c - r, prev + 1), min(c + r, n - 1)))
    return out


def lanes_holding_maximum(x, lo, hi):
    """(samples a lane searches, the lanes whose run holds the window's maximum): lane l owns the l-th run of ceil(length / 64)."""
    run = -(-(hi - lo + 1) // 64)
    w = np.asarray(x[lo:hi + 1])
    return run, sorted({int(i) // run for i in np.flatnonzero(w == w.max())})
