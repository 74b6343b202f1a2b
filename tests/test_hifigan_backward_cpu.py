"""No GPU: the float64 restatement behind the HiFi-GAN backward tests (tests/hifigan_grad_ref64.py) against the forward restatement and
against itself, and the host arithmetic of the tape and workspace queries (csrc/hifigan_train.hip)."""
import ctypes as C

import pytest
import torch

from genvox_amd import _lib
from tests import hifigan_grad_ref64 as GR
from tests import hifigan_ref64 as R
from tests.hifigan_train_helpers import dims_of, layout_of

CFGS = ("V1", "V2", "V3", "NARROW", "TWO", "MID", "ODD", "ONE", "FOUR")   # the last three: 37 and 5 mels, padded to 40 and 8 on the tape


def _cotangent(cfg, B, T):
    return torch.randn(B, T * R.hop(cfg), generator=torch.Generator().manual_seed(1000 * B + T), dtype=torch.float64)


@pytest.mark.parametrize("name,B,T", [("NARROW", 2, 5), ("TWO", 2, 5), ("MID", 1, 3)])
def test_restatement_has_the_forward_restatements_waveform(name, B, T):
    cfg = getattr(R, name)
    sd, mel = R.random_state(cfg, 11), R.random_mel(cfg, B, T, 1)
    wav, tape = GR.generator_tape(sd, mel, cfg)
    want, stages = R.generator(sd, mel, cfg)
    assert torch.equal(wav, want)
    entries = GR.tape_entries(cfg)
    assert [(t.shape[2] // T, t.shape[1]) for t in tape[1:]] == [(e[0], e[1]) for e in entries[1:]]
    avgs = [i for i in range(2, len(entries)) if i + 1 == len(entries) or entries[i + 1][0] != entries[i][0]]
    assert all(torch.equal(tape[i], s) for i, s in zip(avgs, stages))   # the last tensor of each stage is its average


@pytest.mark.parametrize("name,B,T,lens", [("NARROW", 2, 5, None), ("TWO", 3, 6, (2, 6, 3)), ("MID", 1, 3, None)])
def test_pinned_to_its_own_decisions_is_plain_autograd(name, B, T, lens):
    cfg = getattr(R, name)
    sd, mel, G = R.random_state(cfg, 11), R.random_mel(cfg, B, T, 1), _cotangent(cfg, B, T)
    wav, tape, grads = GR.run(sd, mel, lens, cfg, G)
    wav_p, tape_p, grads_p = GR.run(sd, mel, lens, cfg, G, GR.masks_from_tape(tape, cfg))
    assert torch.equal(wav, wav_p) and all(torch.equal(a, b) for a, b in zip(tape, tape_p))
    assert set(grads) == set(GR.param_names(cfg)) | {"mel"}
    for k in grads:
        assert torch.equal(grads[k], grads_p[k]), k


def _formula(cfg):
    """Floats per frame and row, and the (positions per frame, channels) list, from the header's statement of the tape."""
    n_k, n_dil, per_dil = len(cfg["kernels"]), len(cfg["dilations"][0]), 2 if cfg["resblock"] == "1" else 1
    entries, mul, c = [(1, (cfg["n_mels"] + 3) // 4 * 4), (1, cfg["c0"])], 1, cfg["c0"]
    for r in cfg["rates"]:
        mul, c = mul * r, c // 2
        entries += [(mul, c)] * (2 + n_k * (n_dil * per_dil - 1))
    return sum(m * ch for m, ch in entries), entries


def test_v1_tape_is_1812800_bytes_per_frame_and_row():
    floats, entries = _formula(R.V1)
    assert floats == 80 + 512 + 17 * (2048 + 3 * 8192) == 453200 and len(entries) == 2 + 4 * 17
    assert _lib.load().gvx_hifigan_tape_bytes(C.byref(dims_of(R.V1)), 1, 1) == 1812800
    assert len(_formula(dict(R.V1, rates=(8, 8)))[1]) == 36 and len(_formula(R.TWO)[1]) == 2 + 2 * 5


@pytest.mark.parametrize("name", CFGS)
def test_tape_bytes_and_layout_follow_the_formula(name):
    cfg = getattr(R, name)
    lib, d = _lib.load(), dims_of(cfg)
    floats, entries = _formula(cfg)
    assert [(e[0], e[1]) for e in GR.tape_entries(cfg)] == entries
    for B, T in ((1, 1), (2, 5), (3, 33)):
        assert lib.gvx_hifigan_tape_bytes(C.byref(d), B, T) == 4 * B * T * floats
        got, at = layout_of(lib, d, B, T), 0
        assert len(got) == len(entries) and lib.gvx_hifigan_tape_layout(C.byref(d), B, T, None, 0) == len(entries)
        for (off, mul, ch), (want_mul, want_ch) in zip(got, entries):
            assert (off, mul, ch) == (at, want_mul, want_ch) and off % 16 == 0
            at += 4 * B * T * mul * ch
        assert at == lib.gvx_hifigan_tape_bytes(C.byref(d), B, T)
    one = lib.gvx_hifigan_tape_bytes(C.byref(d), 1, 1)
    assert lib.gvx_hifigan_tape_bytes(C.byref(d), 7, 1) == 7 * one and lib.gvx_hifigan_tape_bytes(C.byref(d), 1, 9) == 9 * one


@pytest.mark.parametrize("name", CFGS)
def test_workspace_bytes_are_nonzero_and_aligned(name):
    lib, d = _lib.load(), dims_of(getattr(R, name))
    sizes = [lib.gvx_hifigan_backward_workspace_bytes(C.byref(d), B, T) for B, T in ((1, 1), (2, 5), (2, 64), (2, 65))]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)


def test_queries_return_zero_for_refused_shapes():
    lib, d = _lib.load(), dims_of(R.NARROW)
    queries = (lib.gvx_hifigan_tape_bytes, lib.gvx_hifigan_backward_workspace_bytes, lambda *a: lib.gvx_hifigan_tape_layout(*a, None, 0))
    for q in queries:
        assert q(C.byref(d), 1, 1) > 0
        for B, T in ((0, 4), (65536, 4), (1, 0), (1, 32769)):   # GVX_HIFIGAN_MAX_FRAMES = 32768
            assert q(C.byref(d), B, T) == 0, (B, T)
        bad = dims_of(dict(R.NARROW, rates=(3, 2)))   # an odd rate
        assert q(C.byref(bad), 1, 4) == 0
        bad = dims_of(dict(R.NARROW, kernels=(3, 7, 13)))
        assert q(C.byref(bad), 1, 4) == 0
