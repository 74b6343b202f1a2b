"""CPU: the host side of the MelGAN training calls - symbols, the tape's arithmetic against the header's statement, refusals that
happen before the device is looked at - and the restatement's own gradient properties.  No GPU call."""
import ctypes as C
import os
import re

import pytest
import torch

from genvox_amd import _lib, build
from genvox_amd.configs import AudioConfig, MelGANConfig
from genvox_amd.melgan import MelGANGenerator, dims_from_config
from tests import melgan_grad_ref64 as GR
from tests import melgan_ref64 as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gvx_melgan_tape_bytes", "gvx_melgan_tape_layout", "gvx_melgan_backward_workspace_bytes", "gvx_melgan_forward_train", "gvx_melgan_backward")


def _dims(cfg) -> _lib.gvx_melgan_dims:
    return _lib.gvx_melgan_dims(cfg["n_mels"], cfg["base_channels"], len(cfg["ratios"]), (C.c_int32 * 8)(*cfg["ratios"]), cfg["n_res"],
                                cfg["dil_base"], cfg["slope"])


def _layout(lib, d, B, T):
    e = (_lib.gvx_melgan_tape_entry * 256)()
    n = lib.gvx_melgan_tape_layout(C.byref(d), B, T, e, 256)
    return [(e[i].byte_offset, e[i].positions_per_frame, e[i].channels) for i in range(n)]


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    declared = set(re.findall(r"\b(gvx_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "melgan_train.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "melgan_train.hip"))


@pytest.mark.parametrize("cfg", [R.DEFAULT, R.NARROW, R.TWO_DEEP], ids=["DEFAULT", "NARROW", "TWO_DEEP"])
def test_tape_arithmetic_is_the_headers(cfg):
    """gvx_melgan_tape_bytes and gvx_melgan_tape_layout agree with each other and with the header's formula: tensors in forward
    order, each starting where the one before ends, 4 * B * T * F bytes in all; linear in B, monotone (linear) in T."""
    lib, d = _lib.load(), _dims(cfg)
    want, mul, c = [(1, (cfg["n_mels"] + 3) // 4 * 4), (1, cfg["base_channels"])], 1, cfg["base_channels"]
    for r in cfg["ratios"]:
        mul, c = mul * r, c // 2
        want += [(mul, c)] * (1 + 2 * cfg["n_res"])
    F = sum(m * ch for m, ch in want)
    for B, T in ((1, 4), (2, 5), (3, 37), (16, 32)):
        lay = _layout(lib, d, B, T)
        assert [(m, ch) for _, m, ch in lay] == want
        at = 0
        for (off, m, ch) in lay:
            assert off == at
            at += 4 * B * T * m * ch
        assert at == lib.gvx_melgan_tape_bytes(C.byref(d), B, T) == 4 * B * T * F
        assert lib.gvx_melgan_tape_layout(C.byref(d), B, T, None, 0) == len(want) == 2 + len(cfg["ratios"]) * (1 + 2 * cfg["n_res"])
        assert lib.gvx_melgan_tape_bytes(C.byref(d), B, T + 1) > at and lib.gvx_melgan_tape_bytes(C.byref(d), 2 * B, T) == 2 * at
        ws = lib.gvx_melgan_backward_workspace_bytes(C.byref(d), B, T)
        assert ws > 0 and ws % 256 == 0 and lib.gvx_melgan_backward_workspace_bytes(C.byref(d), B, T + 1) >= ws
    if cfg is R.DEFAULT:
        assert F == 186960 == 80 + 512 + 7 * (2048 + 3 * 8192)   # the header's floats per frame and row: 747,840 bytes
        assert lib.gvx_melgan_tape_bytes(C.byref(d), 1, 100) == 747840 * 100


def test_size_calls_return_zero_for_refused_shapes():
    lib = _lib.load()
    good, bad = _dims(R.DEFAULT), _dims(R.DEFAULT)
    bad.ratios[2] = 3
    e = (_lib.gvx_melgan_tape_entry * 64)()
    for d, B, T in ((bad, 1, 8), (good, 1, 3), (good, 0, 8), (good, 1, 32769)):
        assert lib.gvx_melgan_tape_bytes(C.byref(d), B, T) == 0
        assert lib.gvx_melgan_tape_layout(C.byref(d), B, T, e, 64) == 0
        assert lib.gvx_melgan_backward_workspace_bytes(C.byref(d), B, T) == 0
    assert lib.gvx_melgan_tape_bytes(C.byref(good), 1, 4) > 0


def test_training_calls_refuse_on_the_host():
    """T = 3, a NULL tape and a tape one byte short are refused before the (bogus) pointers are looked at; so is a missing gradient
    name.  A call that got past its checks would launch on made-up addresses and, without a device, fail with GVX_ERR_HIP."""
    lib, d = _lib.load(), _dims(R.NARROW)
    h = C.c_void_p()
    assert lib.gvx_melgan_create(C.byref(d), C.byref(h)) == 0
    P, one = 1 << 20, C.c_float()
    table = (_lib.gvx_weight_desc * 1)(_lib.gvx_weight_desc(b"pre.weight", P, 32 * 10 * 7))
    assert lib.gvx_melgan_forward_train(h, P, None, 1, 8, P, P, 1 << 30, None, 0, None) == -7          # no blob bound
    assert lib.gvx_melgan_bind(h, 256) == 0
    need, ws = lib.gvx_melgan_tape_bytes(C.byref(d), 1, 8), lib.gvx_melgan_backward_workspace_bytes(C.byref(d), 1, 8)
    assert lib.gvx_melgan_forward_train(h, C.addressof(one), None, 1, 3, C.addressof(one), P, 1 << 30, None, 0, None) == -1
    assert b"reflection" in lib.gvx_last_error()
    assert lib.gvx_melgan_backward(h, P, None, 1, 3, P, 1 << 30, table, 1, None, P, 1 << 30, None) == -1
    assert lib.gvx_melgan_forward_train(h, P, None, 1, 8, P, None, need, None, 0, None) == -5
    assert lib.gvx_melgan_forward_train(h, P, None, 1, 8, P, P, need - 1, None, 0, None) == -5
    assert lib.gvx_melgan_forward_train(h, P, None, 1, 8, P, P + 4, need, None, 0, None) == -5           # misaligned
    assert lib.gvx_melgan_backward(h, P, None, 1, 8, None, need, table, 1, None, P, ws, None) == -5
    assert lib.gvx_melgan_backward(h, P, None, 1, 8, P, need - 1, table, 1, None, P, ws, None) == -5
    assert lib.gvx_melgan_backward(h, P, None, 1, 8, P, need, table, 1, None, P, ws - 1, None) == -5
    assert lib.gvx_melgan_backward(h, P, None, 1, 8, P, need, table, 1, None, None, ws, None) == -5
    assert lib.gvx_melgan_backward(h, P, None, 1, 8, P, need, table, 1, None, P, ws, None) == -3           # pre.bias has no destination
    assert b"pre.bias" in lib.gvx_last_error()
    table[0].numel = 5
    assert lib.gvx_melgan_backward(h, P, None, 1, 8, P, need, table, 1, None, P, ws, None) == -4
    lib.gvx_melgan_destroy(h)


def test_vocode_with_grad_has_no_cpu_path():
    ac = AudioConfig(n_mels=12)
    ac.hop_length = 8
    model = MelGANGenerator(MelGANConfig(base_channels=32, upsample_ratios=(4, 2)), ac)
    with pytest.raises(RuntimeError, match="MI355X"):
        model.vocode_with_grad(torch.zeros(1, 12, 8))
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        model.vocode_with_grad(torch.zeros(1, 12, 8))
    assert dims_from_config(model.model_config, ac).n_mels == 12


def test_gradient_restatement_against_the_forward_restatement_and_finite_differences():
    """The restatement the device is held to: its waveform is melgan_ref64's, its tape ends in that module's stage tensors, pinning
    to its own decisions changes nothing beyond float64 rounding, and its float64 gradient matches a central difference along a random direction."""
    cfg = R.NARROW
    sd, mel = R.random_state(cfg, 11), R.random_mel(cfg, 2, 7, 1)
    G = torch.randn(2, 7 * R.hop(cfg), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref = GR.reference(sd, mel, None, cfg, G)
    wav, stages = R.generator(sd, mel, cfg)
    assert torch.equal(ref["wav"], wav) and torch.equal(ref["tape"][-1], stages[-1]) and torch.equal(ref["tape"][2 + 2 * cfg["n_res"]], stages[0])
    assert set(ref["grads"]) == set(GR.param_names(cfg)) | {"mel"} and len(ref["tape"]) == len(GR.tape_muls(cfg))
    pinned = GR.reference(sd, mel, None, cfg, G, GR.masks_from_tape(ref["tape"], cfg["slope"]))
    for k in ref["grads"]:   # x * m for lrelu(x): the same function, float64 rounding apart
        torch.testing.assert_close(pinned["grads"][k], ref["grads"][k], rtol=1e-12, atol=1e-14)
    gen = torch.Generator().manual_seed(4)
    step = {k: torch.randn(v.shape, generator=gen, dtype=torch.float64) for k, v in sd.items()}
    eps = 1e-6
    up = (R.generator({k: v + eps * step[k] for k, v in sd.items()}, mel, cfg)[0] * G).sum()
    down = (R.generator({k: v - eps * step[k] for k, v in sd.items()}, mel, cfg)[0] * G).sum()
    slope = sum((ref["grads"][k] * step[k]).sum() for k in sd)
    assert abs((up - down) / (2 * eps) - slope) <= 1e-6 * abs(slope)
    # ragged: the rows alone, summed
    lens = (4, 7)
    rag = GR.reference(sd, mel, lens, cfg, G)
    alone = [GR.reference(sd, mel[b:b + 1, :, :t], None, cfg, G[b:b + 1, :t * 8]) for b, t in enumerate(lens)]
    for k in sd:
        torch.testing.assert_close(rag["grads"][k], alone[0]["grads"][k] + alone[1]["grads"][k], rtol=1e-12, atol=1e-14)
    assert not rag["grads"]["mel"][0, :, 4:].any() and torch.equal(rag["grads"]["mel"][0, :, :4], alone[0]["grads"]["mel"][0])
