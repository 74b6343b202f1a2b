"""CPU: the layouts of the four discriminators, of the two generator backwards and of the two plans that need no device, pinned.

The layouts are host arithmetic on shared helpers (csrc/rounding.h, disc_handle.h, gen_backward.h, stft_plan.h), and a blob, a features
buffer or a tape written by one build is read by the next: a change of a size or of an entry is a change of the ABI.  Every number in
tests/golden/disc_and_loss_layouts.json was returned by the library built from commit 07c16dc ("Generator backwards: several rows times
several pieces against float64"), the last one in which the MelGAN discriminator, the three plans and the two backwards each carried
their own copy of that arithmetic; `python -m tests.test_disc_and_loss_layouts_cpu` prints what the loaded library returns, in the
file's form.  Nothing here touches a GPU."""
import ctypes as C
import json
import os

import pytest

from genvox_amd import _lib, hifigan, hifigan_disc, hifigan_msd, melgan, melgan_disc, mrd
from genvox_amd.configs import (AudioConfig, HiFiGANConfig, HiFiGANPeriodDiscriminatorConfig, HiFiGANScaleDiscriminatorConfig, MelGANConfig,
                                MelGANDiscriminatorConfig, MultiResolutionDiscriminatorConfig)
from tests import hifigan_disc_ref64, hifigan_msd_ref64, hifigan_ref64, melgan_disc_ref64, melgan_ref64, mrd_ref64
from tests.hifigan_train_helpers import dims_of as hifigan_dims_of
from tests.melgan_train_helpers import dims_of as melgan_dims_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disc_and_loss_layouts.json")
DISCS = {"melgan_disc": _lib.gvx_melgan_disc_entry, "hifigan_mpd": _lib.gvx_hifigan_mpd_entry, "hifigan_msd": _lib.gvx_hifigan_msd_entry,
         "mrd": _lib.gvx_mrd_entry}
MAX_SAMPLES = 1 << 24                                    # GVX_<MODEL>_MAX_SAMPLES of all four discriminators
FRAMES = {"melgan": (4, 32768), "hifigan": (1, 32768)}   # the least and the largest T of a backward
N_FFTS = (512, 1024, 2048)
PLAN_SHAPES = ((1, 1025), (3, 4096), (2, 22050))
PLAN_MAX = (65535, 1 << 30)                              # rows and samples, both plans
N_MELS = 80


def _disc_dims(model, which):
    """The dims of a discriminator at its default config, or at the small config ("small") that tests/test_<model>_gpu.py runs."""
    small = which == "small"
    if model == "melgan_disc":
        cfg = melgan_disc_ref64.TINY
        if not small:
            return melgan_disc.dims_from_config(MelGANDiscriminatorConfig())
        return _lib.gvx_melgan_disc_dims(cfg["n_scales"], cfg["base_channels"], cfg["n_layers"], cfg["s"], cfg["max_channels"], cfg["slope"])
    if model == "hifigan_mpd":
        cfg = hifigan_disc_ref64.TINY
        if not small:
            return hifigan_disc.dims_from_config(HiFiGANPeriodDiscriminatorConfig())
        periods, channels = (C.c_int32 * 8)(*cfg["periods"]), (C.c_int32 * 8)(*cfg["channels"])
        return _lib.gvx_hifigan_mpd_dims(len(cfg["periods"]), periods, len(cfg["channels"]), channels, cfg["kernel_size"], cfg["stride"], cfg["slope"])
    if model == "hifigan_msd":
        cfg = hifigan_msd_ref64.TINY
        if not small:
            return hifigan_msd.dims_from_config(HiFiGANScaleDiscriminatorConfig())
        arrays = [(C.c_int32 * 8)(*cfg[k]) for k in ("channels", "kernel_sizes", "strides", "groups")]
        return _lib.gvx_hifigan_msd_dims(cfg["n_scales"], len(cfg["channels"]), *arrays, cfg["slope"])
    assert model == "mrd"
    if not small:
        return mrd.dims_from_config(MultiResolutionDiscriminatorConfig())
    res = mrd_ref64.HANN["resolutions"]
    n_fft, hop, win = ((C.c_int32 * 8)(*[r[k] for r in res]) for k in range(3))
    return _lib.gvx_mrd_dims(len(res), n_fft, hop, win, mrd_ref64.HANN["channels"], 1, mrd_ref64.HANN["slope"])


def _least_n_max(lib, model, d):
    features = getattr(lib, f"gvx_{model}_features_bytes")
    return next(n for n in range(1, 1 << 16) if features(C.byref(d), 1, n))


def _disc(lib, model, which):
    d = _disc_dims(model, which)
    blob, layout, features, ws = (getattr(lib, f"gvx_{model}_{f}") for f in ("blob_floats", "layout", "features_bytes", "workspace_bytes"))
    out = {"blob_floats": blob(C.byref(d)), "least_n_max": _least_n_max(lib, model, d), "shapes": []}
    for B, n in ((1, out["least_n_max"]), (3, 4000), (2, 8192)):
        count = layout(C.byref(d), B, n, None, 0)
        entries = (DISCS[model] * count)()
        assert layout(C.byref(d), B, n, entries, count) == count
        out["shapes"].append({"B": B, "n_max": n, "features_bytes": features(C.byref(d), B, n), "workspace_bytes": [ws(C.byref(d), B, n, 0), ws(C.byref(d), B, n, 1)],
                              "layout": [[getattr(e, f) for f, _ in e._fields_] for e in entries]})
    return out


def _gen_dims(model, which):
    if model == "melgan":
        return melgan_dims_of(melgan_ref64.NARROW) if which == "small" else melgan.dims_from_config(MelGANConfig(), AudioConfig())
    return hifigan_dims_of(hifigan_ref64.NARROW) if which == "small" else hifigan.dims_from_config(HiFiGANConfig(), AudioConfig())


def _backward(lib, model, which):
    d = _gen_dims(model, which)
    tape, layout, ws = (getattr(lib, f"gvx_{model}_{f}") for f in ("tape_bytes", "tape_layout", "backward_workspace_bytes"))
    out = []
    for B, T in ((1, FRAMES[model][0]), (3, 37), (2, 200)):
        count = layout(C.byref(d), B, T, None, 0)
        entries = (_lib.gvx_melgan_tape_entry * count)()
        assert layout(C.byref(d), B, T, entries, count) == count
        out.append({"B": B, "T": T, "tape_bytes": tape(C.byref(d), B, T), "backward_workspace_bytes": ws(C.byref(d), B, T),
                    "tape_layout": [[e.byte_offset, e.positions_per_frame, e.channels] for e in entries]})
    return out


def _plan(lib, kind, n_fft):
    """A mel-loss plan (hop n_fft / 4, a full window, N_MELS mels of an all-zero basis) or a denoiser's (hop n_fft / 4): neither needs a device."""
    p = C.c_void_p()
    if kind == "mel_loss":
        basis = (C.c_float * (N_MELS * (n_fft // 2 + 1)))()
        _lib.check(lib.gvx_mel_loss_create(n_fft, n_fft // 4, n_fft, N_MELS, basis, 1e-5, 1e-9, C.byref(p)))
    else:
        _lib.check(lib.gvx_denoise_create(n_fft, n_fft // 4, C.byref(p)))
    return p


def _plan_sizes(lib, kind, n_fft):
    p = _plan(lib, kind, n_fft)
    try:
        return [getattr(lib, f"gvx_{kind}_workspace_bytes")(p, B, n) for B, n in PLAN_SHAPES]
    finally:
        getattr(lib, f"gvx_{kind}_destroy")(p)


def measure(lib):
    return {"discriminators": {f"{m}/{w}": _disc(lib, m, w) for m in DISCS for w in ("default", "small")},
            "backwards": {f"{m}/{w}": _backward(lib, m, w) for m in FRAMES for w in ("default", "small")},
            "plans": {f"{k}/{n}": _plan_sizes(lib, k, n) for k in ("mel_loss", "denoise") for n in N_FFTS}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("which", ("default", "small"))
@pytest.mark.parametrize("model", sorted(DISCS))
def test_discriminator_layouts_are_those_of_the_recorded_build(golden, model, which):
    got, want = _disc(_lib.load(), model, which), golden["discriminators"][f"{model}/{which}"]
    assert got == want
    assert got["blob_floats"] > 0 and [s["n_max"] for s in got["shapes"]] == [got["least_n_max"], 4000, 8192]
    assert all(s["features_bytes"] > 0 and min(s["workspace_bytes"]) > 0 and s["layout"] for s in got["shapes"])


@pytest.mark.parametrize("which", ("default", "small"))
@pytest.mark.parametrize("model", sorted(FRAMES))
def test_backward_tapes_and_workspaces_are_those_of_the_recorded_build(golden, model, which):
    got = _backward(_lib.load(), model, which)
    assert got == golden["backwards"][f"{model}/{which}"]
    assert all(s["tape_bytes"] > 0 and s["backward_workspace_bytes"] > 0 and s["tape_layout"] for s in got)


@pytest.mark.parametrize("n_fft", N_FFTS)
@pytest.mark.parametrize("kind", ("mel_loss", "denoise"))
def test_plan_workspaces_are_those_of_the_recorded_build(golden, kind, n_fft):
    got = _plan_sizes(_lib.load(), kind, n_fft)
    assert got == golden["plans"][f"{kind}/{n_fft}"] and all(v > 0 for v in got)


def test_everything_is_recorded(golden):
    assert sorted(golden) == ["backwards", "discriminators", "plans"]
    assert sorted(golden["discriminators"]) == sorted(f"{m}/{w}" for m in DISCS for w in ("default", "small"))
    assert sorted(golden["backwards"]) == sorted(f"{m}/{w}" for m in FRAMES for w in ("default", "small"))
    assert sorted(golden["plans"]) == sorted(f"{k}/{n}" for k in ("mel_loss", "denoise") for n in N_FFTS)


@pytest.mark.parametrize("model", sorted(DISCS))
def test_discriminator_size_functions_return_zero_for_what_the_forward_refuses(model):
    lib, d = _lib.load(), _disc_dims(model, "default")
    blob, layout, features, ws = (getattr(lib, f"gvx_{model}_{f}") for f in ("blob_floats", "layout", "features_bytes", "workspace_bytes"))
    least = _least_n_max(lib, model, d)
    sizes = lambda dims, B, n: (layout(dims, B, n, None, 0), features(dims, B, n), ws(dims, B, n, 0), ws(dims, B, n, 1))
    assert all(v > 0 for v in sizes(C.byref(d), 1, least)) and all(v > 0 for v in sizes(C.byref(d), 1, MAX_SAMPLES))
    assert blob(None) == 0 and sizes(None, 1, 4000) == (0, 0, 0, 0)    # null dims
    assert sizes(C.byref(d), 0, 4000) == (0, 0, 0, 0)                   # B = 0
    assert sizes(C.byref(d), 65536, 4000) == (0, 0, 0, 0)               # one row past the limit
    assert sizes(C.byref(d), 1, least - 1) == (0, 0, 0, 0)              # one sample below the least
    assert sizes(C.byref(d), 1, MAX_SAMPLES + 1) == (0, 0, 0, 0)        # one past the limit


@pytest.mark.parametrize("model", sorted(FRAMES))
def test_backward_size_functions_return_zero_for_what_the_backward_refuses(model):
    lib, d = _lib.load(), _gen_dims(model, "default")
    tape, layout, ws = (getattr(lib, f"gvx_{model}_{f}") for f in ("tape_bytes", "tape_layout", "backward_workspace_bytes"))
    sizes = lambda dims, B, T: (tape(dims, B, T), layout(dims, B, T, None, 0), ws(dims, B, T))
    least, most = FRAMES[model]
    assert all(v > 0 for v in sizes(C.byref(d), 1, least)) and all(v > 0 for v in sizes(C.byref(d), 1, most))
    assert sizes(None, 1, 37) == (0, 0, 0)                  # null dims
    assert sizes(C.byref(d), 0, 37) == (0, 0, 0)            # B = 0
    assert sizes(C.byref(d), 1, least - 1) == (0, 0, 0)     # one frame below the least
    assert sizes(C.byref(d), 1, most + 1) == (0, 0, 0)      # one past the limit


@pytest.mark.parametrize("kind", ("mel_loss", "denoise"))
def test_plan_size_functions_return_zero_for_what_the_call_refuses(kind):
    lib = _lib.load()
    ws, p = getattr(lib, f"gvx_{kind}_workspace_bytes"), _plan(lib, kind, 1024)
    try:
        assert ws(p, 1, 4096) > 0 and ws(p, PLAN_MAX[0], 1) > 0 and ws(p, 1, PLAN_MAX[1]) > 0
        assert ws(None, 1, 4096) == 0                                            # null plan
        assert ws(p, 0, 4096) == 0 and ws(p, PLAN_MAX[0] + 1, 4096) == 0         # B = 0, one row past the limit
        assert ws(p, 1, 0) == 0 and ws(p, 1, PLAN_MAX[1] + 1) == 0               # no samples, one past the limit
    finally:
        getattr(lib, f"gvx_{kind}_destroy")(p)


if __name__ == "__main__":
    print(json.dumps(measure(_lib.load()), separators=(",", ":")))
