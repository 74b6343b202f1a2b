"""GPU: gvx_denoise through the C ABI alone against the float64 restatement (tests/denoise_ref64.py), sample by sample and cell by
cell, at every length where a workgroup is added or a boundary sits, on noise, tones under a clamping bias, three scales and silence;
the special strengths and output modes; bit equality between calls, between a ragged row and its own one-row run, and over a dirty
workspace; the refusal that is only known on the device.  Workspace exactly sized and NaN-filled, outputs NaN before the call, the
input NaN at and behind every row's length (tests/denoise_helpers.py).

Largest |device - float64| as a fraction of the bound FACTOR x max(float32 twin's error, ulp of the row's scale), every case of this
file, on an MI355X: out 0.47 (the tone at 1024 / 512), mag 0.20 (noise at 512 / 60)."""
import pytest
import torch

from tests import denoise_ref64 as R
from tests.denoise_helpers import DEV, G, NAN, S, Plan, poisoned, zeros_behind

pytestmark = pytest.mark.gpu
SHAPE = -4
PLANS = [(n_fft, hop) for n_fft in (512, 1024, 2048) for hop in (n_fft // 4, n_fft // 2, 15 * n_fft // 128)]   # 60, 120, 240: no divisor of n_fft


def up(n, m):
    return (n + m - 1) // m * m


def edge_lengths(n_fft, hop):
    """Nine lengths in [pad + 1, 3 n_fft] as three ragged batches: the minimum; a multiple of hop whose frame count is 0 mod the
    frames per workgroup, and that multiple minus 1; a frame count of 1 mod it; one below, on and one above a multiple of the gather's
    samples per workgroup; 3 n_fft - 1 and a length in between."""
    pad = n_fft // 2
    m = up(pad + 1, hop) // hop
    while (1 + m) % G:
        m += 1
    whole = m * hop                      # F = 1 + m = 0 mod G
    j = up(pad + 1, G * hop) // (G * hop)
    one_more = j * G * hop + hop // 2    # F = 1 + j G = 1 mod G
    k = up(pad + 2, S)
    lengths = [pad + 1, whole, whole - 1, one_more, k - 1, k, k + 1, 3 * n_fft - 1, 2 * n_fft + 37]
    assert all(pad + 1 <= n <= 3 * n_fft for n in lengths), lengths
    assert R.frames(whole, hop) % G == 0 and R.frames(one_more, hop) % G == 1 and whole - 1 >= pad + 1
    return [lengths[0:3], lengths[3:6], lengths[6:9]]


def random_bias(seed, n_fft, level):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n_fft // 2 + 1, generator=g, dtype=torch.float64) * 2.0 * level).float()


def hold(plan, wav, lengths, bias, strength, ref, what):
    out, mag = plan.run(wav, lengths, bias, strength)
    zeros_behind(out, mag, lengths, plan.hop)
    r_out, r_mag = R.ratios(out, mag, ref)
    print(f"{what}: out at {r_out:.3f} of its bound, mag at {r_mag:.3f}")
    assert r_out <= 1.0 and r_mag <= 1.0, (what, r_out, r_mag)
    return out, mag


@pytest.mark.parametrize("n_fft,hop", PLANS)
def test_unit_noise_at_every_edge(n_fft, hop):
    plan = Plan(n_fft, hop)
    for i, lengths in enumerate(edge_lengths(n_fft, hop)):
        n_max = min(3 * n_fft, max(lengths) + 7 * i)   # the first batch ends on its longest row, the others behind it
        wav = R.noise(10 + i, 3, n_max)
        level = float(R.run(wav, lengths, n_fft, hop)["mag"].median())
        bias = random_bias(20 + i, n_fft, level)
        ref = R.reference(wav, lengths, n_fft, hop, bias, 1.0)
        assert 0.05 < R.clamped_fraction(ref) < 0.95
        hold(plan, wav, lengths, bias, 1.0, ref, f"noise {n_fft}/{hop} {lengths}")


_tones = {}


def tone(n_fft, hop):
    """(lengths, n_max, wav, bias, reference) at scale 1, computed once: the seed is picked on the CPU."""
    if (n_fft, hop) not in _tones:
        lengths = edge_lengths(n_fft, hop)[0]
        n_max = max(lengths) + 5
        _, wav, bias, ref = R.tone_case(n_fft, hop, lengths, n_max)
        _tones[(n_fft, hop)] = (lengths, n_max, wav, bias, ref)
    return _tones[(n_fft, hop)]


@pytest.mark.parametrize("exponent", [0, 20, -20])
@pytest.mark.parametrize("n_fft,hop", PLANS)
def test_tone_under_a_clamping_bias_at_three_scales(n_fft, hop, exponent):
    lengths, n_max, wav, bias, ref = tone(n_fft, hop)
    if exponent:   # exact scalings of the inputs, the bias scaled along; the reference is made anew, on the scaled signal
        wav, bias = wav * 2.0 ** exponent, bias * 2.0 ** exponent
        ref = R.reference(wav, lengths, n_fft, hop, bias, 1.0)
    assert 0.25 <= R.clamped_fraction(ref) <= 0.75   # on the float64 reference, not the device
    hold(Plan(n_fft, hop), wav, lengths, bias, 1.0, ref, f"tone {n_fft}/{hop} x 2^{exponent}")


@pytest.mark.parametrize("n_fft,hop", PLANS)
def test_a_silent_row_gives_exact_zeros(n_fft, hop):
    lengths = edge_lengths(n_fft, hop)[1]
    n_max = max(lengths)
    wav = R.noise(5, 3, n_max)
    wav[1] = 0.0
    bias = random_bias(6, n_fft, 10.0)
    plan = Plan(n_fft, hop)
    for b, s in ((bias, 1.0), (None, 0.0)):
        ref = R.reference(wav, lengths, n_fft, hop, b, s)
        out, mag = hold(plan, wav, lengths, b, s, ref, f"silent row {n_fft}/{hop} strength {s}")
        assert bool((out[1] == 0).all()) and bool((mag[1] == 0).all())


@pytest.mark.parametrize("n_fft,hop", PLANS)
def test_special_strengths_and_modes(n_fft, hop):
    lengths = edge_lengths(n_fft, hop)[2]
    n_max = 3 * n_fft
    wav = R.noise(7, 3, n_max)
    plan = Plan(n_fft, hop)
    # strength 0 without a bias: the input comes back, within the bound
    ref = R.reference(wav, lengths, n_fft, hop)
    out0, mag0 = hold(plan, wav, lengths, None, 0.0, ref, f"strength 0 {n_fft}/{hop}")
    for b, n in enumerate(lengths):
        assert float((out0[b, :n].double() - wav[b, :n].double()).abs().max()) <= R.tol(ref["err"]["out"][b], wav[b, :n])
    # a bias above every magnitude the device itself sees: exact zeros, the magnitudes as they were
    high = torch.full((n_fft // 2 + 1,), 2.0 * float(mag0.max()))
    out, mag = plan.run(wav, lengths, high, 1.0)
    assert bool((out == 0).all()) and torch.equal(mag, mag0)
    out, _ = plan.run(wav, lengths, high * 0.25, 4.0)
    assert bool((out == 0).all())
    # either output alone, and in place: the same bits
    bias = random_bias(8, n_fft, float(mag0.median()))
    both_out, both_mag = plan.run(wav, lengths, bias, 0.75)
    assert not torch.equal(both_out, out0)
    only_mag = plan.run(wav, lengths, bias, 0.75, want_out=False)
    only_out = plan.run(wav, lengths, bias, 0.75, want_mag=False)
    assert only_mag[0] is None and torch.equal(only_mag[1], both_mag) and only_out[1] is None and torch.equal(only_out[0], both_out)
    in_place, mag_ip = plan.run(wav, lengths, bias, 0.75, in_place=True)
    assert torch.equal(in_place, both_out) and torch.equal(mag_ip, both_mag)
    # strength 0 with a bias is strength 0 without one
    again, _ = plan.run(wav, lengths, bias, 0.0)
    assert torch.equal(again, out0)


@pytest.mark.parametrize("n_fft,hop", PLANS)
def test_bit_equality(n_fft, hop):
    lengths = edge_lengths(n_fft, hop)[0]
    n_max = max(lengths) + 3
    wav = R.noise(9, 3, n_max)
    plan = Plan(n_fft, hop)
    bias = random_bias(11, n_fft, float(R.run(wav, lengths, n_fft, hop)["mag"].median()))
    out, mag = plan.run(wav, lengths, bias, 1.0)
    twice = plan.run(wav, lengths, bias, 1.0)
    assert torch.equal(twice[0], out) and torch.equal(twice[1], mag)
    for b, n in enumerate(lengths):   # a ragged row is its own one-row run
        alone_out, alone_mag = plan.run(wav[b:b + 1, :n], None, bias, 1.0)
        assert torch.equal(alone_out[0], out[b, :n]) and torch.equal(alone_mag[0], mag[b, :R.frames(n, hop)]), (b, n)
    # a workspace that another call of another signal left behind
    ws = torch.full((plan.ws_bytes(3, n_max) // 4,), NAN, dtype=torch.float32, device=DEV)
    plan.run(R.noise(12, 3, n_max) * 100.0, None, bias, 0.5, ws=ws)
    assert bool(torch.isfinite(ws[:1024]).all())
    dirty = plan.run(wav, lengths, bias, 1.0, ws=ws)
    assert torch.equal(dirty[0], out) and torch.equal(dirty[1], mag)


@pytest.mark.parametrize("n_fft,hop", [(512, 128), (1024, 120), (2048, 1024)])
def test_a_row_outside_its_range_is_refused_behind_the_launches(n_fft, hop):
    pad, n_max = n_fft // 2, 2 * n_fft + 11
    plan = Plan(n_fft, hop)
    wav = R.noise(13, 3, n_max)
    bias = random_bias(14, n_fft, 10.0)
    good_out, good_mag = plan.run(wav[1:2], [n_max - 5], bias, 1.0)
    for lengths, first in (([pad, n_max - 5, n_max + 1], 0), ([n_max, n_max - 5, 0], 2), ([n_max, n_max - 5, -3], 2), ([n_max + 1, n_max - 5, n_max], 0)):
        wav_d = poisoned(wav, [n if pad + 1 <= n <= n_max else 0 for n in lengths])   # nothing of a refused row is read
        lens_d = torch.tensor(lengths, dtype=torch.int32, device=DEV)
        rc, out, mag = plan.raw(wav_d, lens_d, bias.to(DEV), 1.0)
        assert rc == SHAPE and f"row {first} has {lengths[first]} samples".encode() in plan.lib.gvx_last_error(), (lengths, plan.lib.gvx_last_error())
        out, mag = out.cpu(), mag.cpu()
        for b, n in enumerate(lengths):
            if not pad + 1 <= n <= n_max:
                assert bool((out[b] == 0).all()) and bool((mag[b] == 0).all()), (lengths, b)
        assert torch.equal(out[1], good_out[0]) and torch.equal(mag[1], good_mag[0])
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(mag).all())
