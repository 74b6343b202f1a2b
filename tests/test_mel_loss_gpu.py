"""GPU: gvx_mel_loss (csrc/mel_loss.hip) through the C ABI against the float64 restatement in tests/mel_loss_ref64.py: the loss, the
rows' parts, the log-mels of both signals (read through the call's debug pointers) and d_pred.  The workspace, d_pred, the outputs and
everything behind n_b in both inputs start as NaN; the workspace has exactly its stated size.

Tolerance (the rule of test_melgan_backward_gpu.py and test_stft_loss_gpu.py).  Per tensor, e is the largest |float32 twin - float64|
on the CPU, a number of the reference alone, printed per case; the device may differ from float64 by at most
8 x max(e, 2^-23 max|ref64|).

Decisions.  A cell takes two: the sign of l_t - l_p and the clamp.  Each case takes the first seed of 1..8 whose float64 reference
keeps |l_t - l_p| >= 1e-4 (cells clamped on both sides aside) and |m / clamp - 1| >= 1e-4, and asserts on the CPU that 8 e(l) is
below 1e-4: a device inside its bound on l cannot decide differently, so plain float64 autograd is the reference of d_pred.

Shapes.  G frames per workgroup and S samples per gather workgroup come from the header's enum.  Nothing is longer than 8192 samples."""
import functools

import pytest
import torch

from tests import mel_loss_ref64 as R
from tests.mel_loss_helpers import DEV, G, NAN, S, Plan, poisoned, ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


def _hand_made_basis():
    """1024-point: an all-zero row, a row of two separated runs, single entries at bin 0 and at bin n_fft / 2 (the real-only bins of
    the adjoint), and two ordinary triangles."""
    b = torch.zeros(6, 513)
    b[1, 20:30] = 0.05
    b[1, 300:340] = 0.02
    b[2, 0] = 0.1
    b[3, 512] = 0.1
    b[4] = R.slaney(22050, 1024, 80)[10]
    b[5] = R.slaney(22050, 1024, 80)[70]
    return b


@functools.lru_cache(maxsize=None)
def _config(name):
    return {
        "published": lambda: R.Config(1024, 256, 1024, R.slaney(22050, 1024, 80)),            # pad 384
        "fmax8k": lambda: R.Config(512, 128, 512, R.slaney(22050, 512, 40, 0.0, 8000.0)),      # pad 192; the columns above 8 kHz are zero
        "no_pad": lambda: R.Config(512, 512, 301, R.slaney(22050, 512, 5)),                    # pad 0, bands wider than a wave, odd short window
        "widest": lambda: R.Config(2048, 512, 2048, R.slaney(16000, 2048, 128)),               # pad 768, the upper limit of n_mels
        "short_win": lambda: R.Config(1024, 120, 600, R.slaney(22050, 1024, 80)),              # pad 452, a hop that divides nothing
        "hand_made": lambda: R.Config(1024, 256, 1024, _hand_made_basis()),
    }[name]()


# name: (configuration, lengths of the rows or None, n_max)
CASES = {
    # the shortest legal row (one frame, both reflections cover the whole row); G hop - 1 and G hop
    "published_shortest": ("published", (385, G * 256 - 1, G * 256), G * 256 + 76),
    # G hop + 1; (G + 1) hop; 1279, no multiple of hop
    "published_g_edge": ("published", (G * 256 + 1, (G + 1) * 256, 1279), 1300),
    "published_row_of_n_max": ("published", (1500, 600, 900), 1500),
    "published_no_lengths": ("published", None, 1279),
    "fmax8k_shortest": ("fmax8k", (193, 511, 512), 520),
    "fmax8k_gather_2s": ("fmax8k", (2 * S - 1, 2 * S, 2 * S + 1), 2 * S + 1),
    "fmax8k_no_lengths": ("fmax8k", None, 640),
    # a tail that no frame reads: d_pred is exact zeros behind F hop
    "no_pad_tails": ("no_pad", (512, 1025, 1535), 1535),
    "no_pad_no_lengths": ("no_pad", None, 1030),
    "widest_ragged": ("widest", (769, 2048, 4097), 4100),
    "widest_no_lengths": ("widest", None, 2100),
    "short_win_ragged": ("short_win", (453, 1200, 3 * S + 1), 1200),
    "short_win_no_lengths": ("short_win", None, 1000),
    "hand_made_ragged": ("hand_made", (385, 1024, 1279), 1300),
    "hand_made_no_lengths": ("hand_made", None, 700),
}
WORST = {}


def _shape(name):
    cfg, lengths, n_max = CASES[name]
    return _config(cfg), (None if lengths is None else list(lengths)), n_max, (2 if lengths is None else len(lengths))


@functools.lru_cache(maxsize=None)
def _noise_case(name, scale=0.3):
    """(seed, pred, target, float64 reference) of a case: computed once, shared by the tests, never changed."""
    cfg, lengths, n_max, B = _shape(name)
    return R.seeded_case(lambda seed: R.noise(seed, B, n_max, scale), lengths, cfg)


def _note(what, tensor, r):
    WORST[tensor] = max(WORST.get(tensor, 0.0), r)
    print(f"  {what}: {tensor} at {r:.3f} of its bound (largest so far {WORST[tensor]:.3f})")
    return r


def _check(dev, ref, err, what, tensor):
    r = _note(what, tensor, ratio(dev, ref, err))
    assert r <= 1.0, f"{what}: {tensor} differs from float64 by {r:.3f} of 8 x max(e = {err:.3e}, one ulp of {float(ref.abs().max()):.3e})"


def _check_all(what, cfg, pred, target, lengths, ref):
    """One call with every output; loss, parts, both log-mels and d_pred against the reference; the exact zeros of d_pred."""
    B, n_max = pred.shape
    e = ref["err"]
    d_min, c_min, clamped = R.margins(ref, cfg)
    print(f"{what}: float32 twin errors: loss {e['loss']:.3e} parts {e['parts']:.3e} l_p {e['lp']:.3e} l_t {e['lt']:.3e} d_pred {e['d_pred']:.3e}; "
          f"smallest |l_t - l_p| {d_min:.3e}, smallest |m / clamp - 1| {c_min:.3e}, {100 * clamped:.1f} % of the cells clamped")
    assert R.decided(ref, cfg)
    out = Plan(cfg).run(pred, target, lengths, want_dbg=True)
    _check(out["loss"], ref["loss"], e["loss"], what, "loss")
    _check(out["parts"], ref["parts"], e["parts"], what, "parts")
    lens = [n_max] * B if lengths is None else lengths
    for k in ("lp", "lt"):
        for b in range(B):
            F = R.frames(lens[b], cfg.hop)
            assert bool(torch.isfinite(out[k][b, :F]).all()) and bool(torch.isnan(out[k][b, F:]).all()), f"row {b}: {k} is not NaN exactly behind its frames"
        dev = torch.cat([out[k][b, :R.frames(lens[b], cfg.hop)].reshape(-1) for b in range(B)])
        _check(dev, torch.cat([x.reshape(-1) for x in ref[k]]), e[k], what, k)
    _check(out["d_pred"], ref["d_pred"], e["d_pred"], what, "d_pred")
    pad = R.pad_of(cfg)
    for b, n in enumerate(lens):
        reach = min(n, R.frames(n, cfg.hop) * cfg.hop + pad)   # behind it no frame reads the row
        assert bool((out["d_pred"][b, reach:] == 0).all()), f"row {b}: d_pred behind min(n_b, F hop + pad) is not exact zeros"
    assert bool(torch.isfinite(out["d_pred"]).all())
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_value_log_mels_and_gradient(name):
    cfg, lengths, n_max, B = _shape(name)
    seed, pred, target, ref = _noise_case(name)
    print(f"{name}: seed {seed}")
    out = _check_all(name, cfg, pred, target, lengths, ref)
    if CASES[name][0] == "hand_made":   # the all-zero row: log(clamp) on both sides
        assert bool((out["lp"][0, 0, 0] == out["lt"][0, 0, 0])) and abs(float(out["lp"][0, 0, 0]) - float(torch.log(torch.tensor(cfg.clamp)))) < 1e-6


def test_zero_columns_have_no_band():
    """fmax 8000: no mel reaches a bin above 8 kHz, so the transposed product has nothing to add there and dS is exact 0."""
    import numpy as np
    from genvox_amd import _lib
    basis = _config("fmax8k").basis.numpy()
    n_mels, bins = basis.shape
    arrays = [np.zeros(n, dtype=np.int32) for n in (n_mels, n_mels, bins, bins)]
    assert _lib.load().gvx_mel_loss_bands(basis.ctypes.data, n_mels, bins, *[a.ctypes.data for a in arrays]) == 0
    above = int(8000.0 / (22050 / 2) * (bins - 1)) + 2
    assert (arrays[3][above:] == -1).all() and (arrays[3][1:above - 3] >= 0).all()


# ---- signals, at 1024 / 256 / 80

SIGNAL_LENGTHS, SIGNAL_N_MAX = [1279, 1025, 1536], 1536


def _quiet(seed):
    return R.noise(seed, 3, SIGNAL_N_MAX, 2.0 ** -16)


def _silent_target(seed):
    pred, target = R.noise(seed, 3, SIGNAL_N_MAX)
    return pred, torch.zeros_like(target)


def _zero_pred(seed):
    pred, target = R.noise(seed, 3, SIGNAL_N_MAX)
    return torch.zeros_like(pred), target


def _gated(seed):
    """Row 0: exact zeros in its first and last 400 samples, so that silence lies under both reflections; rows 1 and 2 unit noise."""
    pred, target = R.noise(seed, 3, SIGNAL_N_MAX, 1.0)
    n = SIGNAL_LENGTHS[0]
    for x in (pred, target):
        x[0, :400] = 0.0
        x[0, n - 400:] = 0.0
    return pred, target


SIGNALS = {"quiet_2e-16": _quiet, "silent_target": _silent_target, "zero_pred": _zero_pred, "gated_beside_unit_noise": _gated}


@functools.lru_cache(maxsize=None)
def _signal_case(name):
    return R.seeded_case(SIGNALS[name], SIGNAL_LENGTHS, _config("published"))


@pytest.mark.parametrize("name", list(SIGNALS))
def test_signals(name):
    cfg = _config("published")
    seed, pred, target, ref = _signal_case(name)
    print(f"{name}: seed {seed}")
    out = _check_all(name, cfg, pred, target, SIGNAL_LENGTHS, ref)
    _, _, clamped = R.margins(ref, cfg)
    if name == "quiet_2e-16":   # clamped and live cells side by side
        assert 0.05 < clamped < 0.95
        assert any(bool(((m < cfg.clamp).any(dim=1) & (m >= cfg.clamp).any(dim=1)).any()) for m in ref["mp"])
    if name == "zero_pred":
        assert bool(torch.isfinite(out["loss"])) and float(out["loss"]) > 0 and bool((out["d_pred"] == 0).all())
        assert bool((out["lp"][~torch.isnan(out["lp"])] == out["lp"][0, 0, 0]).all())   # every mel under the clamp
    if name == "silent_target":
        assert bool((out["lt"][~torch.isnan(out["lt"])] == out["lt"][0, 0, 0]).all())


def test_equal_signals():
    cfg = _config("published")
    _, pred, target, _ = _noise_case("published_g_edge")
    lengths = _shape("published_g_edge")[1]
    same = Plan(cfg).run(target, target, lengths)
    assert float(same["loss"]) == 0.0 and bool((same["parts"] == 0).all()) and bool((same["d_pred"] == 0).all())


# ---- contract

def test_two_calls_give_equal_bits_and_the_value_alone_the_same_loss():
    cfg, lengths, n_max, B = _shape("published_g_edge")
    _, pred, target, _ = _noise_case("published_g_edge")
    plan = Plan(cfg)
    lens_d = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    p, t = poisoned(pred, lengths), poisoned(target, lengths)
    ws = torch.full((plan.ws_bytes(B, n_max) // 4,), NAN, dtype=torch.float32, device=DEV)
    a = plan.raw(p, t, lens_d, ws=ws)
    other = Plan(_config("fmax8k"))   # another plan dirties the same buffer in between
    assert other.raw(p, t, lens_d, ws=ws[: other.ws_bytes(B, n_max) // 4])[0] == 0
    b = plan.raw(p, t, lens_d, ws=ws)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:4], b[1:4]):
        assert torch.equal(x, y)
    c = plan.raw(p, t, lens_d, want_grad=False)
    d = plan.raw(p, t, lens_d, want_grad=False, want_parts=False)
    e = plan.raw(p, t, lens_d, want_dbg=True)
    assert c[0] == 0 and d[0] == 0 and e[0] == 0
    assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2]) and torch.equal(d[1], a[1]) and torch.equal(e[1], a[1]) and torch.equal(e[3], a[3])


@pytest.mark.parametrize("name", ["published_g_edge", "short_win_ragged", "no_pad_tails"])
def test_ragged_row_is_the_row_run_alone(name):
    """A row's part is the bits of the row run alone (B = 1, n_max = n_b); its part and its d_pred are the bits of that row in any batch
    of the same B - other companions, another slot, another n_max."""
    cfg, lengths, n_max, B = _shape(name)
    _, pred, target, _ = _noise_case(name)
    plan = Plan(cfg)
    out = plan.run(pred, target, lengths)
    g = torch.Generator().manual_seed(77)
    for b, n in enumerate(lengths):
        alone = plan.run(pred[b:b + 1, :n], target[b:b + 1, :n], None)
        assert torch.equal(alone["parts"][0], out["parts"][b]), f"row {b}: the part differs from the row run alone"
        slot, n2 = (b + 1) % B, n_max + 37
        p2, t2 = 0.3 * torch.randn(B, n2, generator=g), 0.3 * torch.randn(B, n2, generator=g)
        p2[slot, :n], t2[slot, :n] = pred[b, :n], target[b, :n]
        l2 = [R.n_min(cfg) + 11 * i for i in range(B)]
        l2[slot] = n
        other = plan.run(p2, t2, l2)
        assert torch.equal(other["parts"][slot], out["parts"][b])
        assert torch.equal(other["d_pred"][slot, :n], out["d_pred"][b, :n]), f"row {b}: d_pred depends on the rows beside it"
        assert bool((other["d_pred"][slot, n:] == 0).all())


def test_refusals():
    """Each refusal gives its status; what is refused on the host launches nothing (every output keeps its NaN), and a row refused by
    its device-side length leaves only defined values: NaN loss, NaN part of that row, an all-zero gradient."""
    cfg = _config("published")
    plan = Plan(cfg)
    B, n_max = 3, 1500
    g = torch.Generator().manual_seed(5)
    p, t = torch.randn(B, n_max, generator=g).to(DEV), torch.randn(B, n_max, generator=g).to(DEV)
    for lengths, row in (([1500, 384, 1300], 1), ([385, 1200, 1501], 2), ([0, 1200, 1500], 0), ([1500, 1500, -3], 2)):
        rc, loss, parts, d_pred, _, _ = plan.raw(p, t, torch.tensor(lengths, dtype=torch.int32, device=DEV))
        assert rc == -4 and f"row {row} ".encode() in plan.lib.gvx_last_error(), (lengths, plan.lib.gvx_last_error())
        assert bool(torch.isnan(loss).all()) and bool((d_pred == 0).all()) and bool(torch.isnan(parts[row]))
        assert bool(torch.isfinite(parts[[b for b in range(B) if b != row]]).all())
    hop_rules = Plan(_config("no_pad"))   # pad 0: the shortest row is one hop
    rc, loss, parts, d_pred, _, _ = hop_rules.raw(p, t, torch.tensor([511, 512, 1500], dtype=torch.int32, device=DEV))
    assert rc == -4 and b"row 0 " in plan.lib.gvx_last_error() and bool((d_pred == 0).all()) and bool(torch.isfinite(parts[1:]).all())
    untouched = lambda out: all(bool(torch.isnan(x).all()) for x in out[1:4])
    short = plan.raw(p[:, :384].contiguous(), t[:, :384].contiguous(), None)   # n_max below max(hop, pad + 1)
    assert short[0] == -4 and untouched(short)
    need = plan.ws_bytes(B, n_max)
    ws = torch.full((need // 4 + 64,), NAN, dtype=torch.float32, device=DEV)
    small = plan.raw(p, t, None, ws=ws, ws_bytes=need - 1)
    assert small[0] == -5 and b"too small" in plan.lib.gvx_last_error() and untouched(small)
    skew = plan.raw(p, t, None, ws=ws[1:])
    assert skew[0] == -5 and b"256-byte aligned" in plan.lib.gvx_last_error() and untouched(skew)
    lib = plan.lib
    one = torch.zeros(1, device=DEV)
    assert lib.gvx_mel_loss(plan.h, None, t.data_ptr(), None, B, n_max, one.data_ptr(), None, None, None, ws.data_ptr(), need, None) == -1
    assert lib.gvx_mel_loss(plan.h, p.data_ptr(), t.data_ptr(), None, 0, n_max, one.data_ptr(), None, None, None, ws.data_ptr(), need, None) == -1
    assert lib.gvx_mel_loss(None, p.data_ptr(), t.data_ptr(), None, B, n_max, one.data_ptr(), None, None, None, ws.data_ptr(), need, None) == -1
    ok = plan.raw(p, t, None, ws=ws)   # the same buffers serve a good call afterwards
    assert ok[0] == 0 and bool(torch.isfinite(ok[1]).all()) and bool(torch.isfinite(ok[3]).all())


def test_case_table_reaches_what_it_promises():
    lens = lambda c: {n for name, (cfg, ls, _) in CASES.items() if cfg == c and ls for n in ls}
    assert {385, G * 256 - 1, G * 256, G * 256 + 1, (G + 1) * 256, 1279} <= lens("published")
    assert {193, 511, 512, 2 * S - 1, 2 * S, 2 * S + 1} <= lens("fmax8k") and {512, 1025, 1535} <= lens("no_pad")
    assert {769, 2048, 4097} <= lens("widest") and {453, 1200, 3 * S + 1} <= lens("short_win")
    assert any(ls and max(ls) == n_max for _, ls, n_max in CASES.values()) and any(ls and max(ls) < n_max for _, ls, n_max in CASES.values())
    assert all(any(c == cfg and ls is None for c, ls, _ in CASES.values()) for cfg in {c for c, _, _ in CASES.values()})
    assert all(n_max <= 8192 for _, _, n_max in CASES.values())
    for name in {c for c, _, _ in CASES.values()}:
        cfg = _config(name)
        assert all(n >= R.n_min(cfg) for n in lens(name)) and min(lens(name)) == R.n_min(cfg)
