"""CPU: the blob and workspace sizes of the six generators' C ABIs (MelGAN, HiFi-GAN, BigVGAN, Vocos, UnivNet, FastPitch), pinned.

The layouts are host arithmetic that the generators share (csrc/gen_host.h: the roundings, the row-wise workspace planner), and a blob
packed by one build is read by the next: a change of a size is a change of the ABI.  Every number below was returned by the library
built from commit a08adea ("FastPitch acoustic model: inference on the device, wired into tts"), the last one in which every generator
carried its own copy of that arithmetic.  Nothing here touches a GPU."""
import ctypes as C

import pytest

from genvox_amd import _lib, bigvgan, fastpitch, hifigan, melgan, univnet, vocos
from genvox_amd.configs import AudioConfig, BigVGANConfig, FastPitchConfig, HiFiGANConfig, MelGANConfig, UnivNetConfig, VocosConfig
from tests import bigvgan_ref64, fastpitch_ref64, hifigan_ref64, melgan_ref64, univnet_ref64, vocos_ref64


def _audio(n_mels, hop):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = hop, n_mels   # below the ranges of a preprocessing config; a vocoder of hop 8 is a test's size
    return ac


def _hifigan_fields(cfg):
    return dict(upsample_initial_channel=cfg["c0"], upsample_rates=cfg["rates"], upsample_kernel_sizes=[2 * r for r in cfg["rates"]],
                resblock=cfg["resblock"], resblock_kernel_sizes=cfg["kernels"], resblock_dilation_sizes=cfg["dilations"])


def _dims(model, which):
    """The dims of `model` at its default config, or at the small config ("small") that tests/test_<model>_gpu.py runs."""
    small = which == "small"
    if model == "melgan":
        cfg = melgan_ref64.NARROW
        if not small:
            return melgan.dims_from_config(MelGANConfig(), AudioConfig())
        return _lib.gvx_melgan_dims(cfg["n_mels"], cfg["base_channels"], len(cfg["ratios"]), (C.c_int32 * 8)(*cfg["ratios"]), cfg["n_res"],
                                    cfg["dil_base"], cfg["slope"])
    if model == "hifigan":
        cfg = hifigan_ref64.NARROW
        if not small:
            return hifigan.dims_from_config(HiFiGANConfig(), AudioConfig())
        return hifigan.dims_from_config(HiFiGANConfig(**_hifigan_fields(cfg)), _audio(cfg["n_mels"], hifigan_ref64.hop(cfg)))
    if model == "bigvgan":
        cfg = bigvgan_ref64.NARROW
        if not small:
            return bigvgan.dims_from_config(BigVGANConfig(), AudioConfig())
        mc = BigVGANConfig(**_hifigan_fields(cfg), activation=cfg["activation"], snake_logscale=cfg["logscale"], use_tanh_at_final=cfg["tanh"],
                           use_bias_at_final=cfg["bias"])
        return bigvgan.dims_from_config(mc, _audio(cfg["n_mels"], bigvgan_ref64.hop(cfg)))
    if model == "vocos":
        cfg = vocos_ref64.NARROW
        if not small:
            return vocos.dims_from_config(VocosConfig(), AudioConfig())
        return vocos.dims_from_config(VocosConfig(**vocos_ref64.model_kwargs(cfg)), _audio(cfg["n_mels"], cfg["hop_length"]))
    if model == "univnet":
        cfg = univnet_ref64.NARROW
        if not small:
            return univnet.dims_from_config(UnivNetConfig(), AudioConfig())
        return univnet.dims_from_config(UnivNetConfig(**univnet_ref64.model_kwargs(cfg)), _audio(cfg["n_mels"], univnet_ref64.hop_of(cfg)))
    assert model == "fastpitch"
    cfg = fastpitch_ref64.NARROW if small else fastpitch_ref64.DEFAULT
    return fastpitch.dims_from_config(FastPitchConfig(**fastpitch_ref64.model_kwargs(cfg)), AudioConfig(n_mels=cfg["n_mels"]), cfg["n_tokens"])


# model: (the smallest T it takes - Vocos: without centring -, the largest); FastPitch's T is the positions of either phase
FRAMES = {"melgan": (4, 32768), "hifigan": (1, 32768), "bigvgan": (1, 32768), "vocos": (1, 1 << 20), "univnet": (4, 1 << 16), "fastpitch": (1, 1 << 16)}

# (model, config): (blob floats, workspace bytes at (1, smallest T), at (3, 37), at (2, 200)), from the library of commit a08adea
EXPECTED = {
    ("melgan", "default"): (4260672, 394496, 10947840, 39449600),
    ("melgan", "small"): (13568, 3328, 90624, 326656),
    ("hifigan", "default"): (13926720, 131584, 14585088, 52556800),
    ("hifigan", "small"): (108096, 2304, 177408, 633856),
    ("bigvgan", "default"): (13945344, 164352, 18222336, 65664000),
    ("bigvgan", "small"): (112896, 2816, 220416, 787456),
    ("vocos", "default"): (13459072, 20992, 2088960, 7508480),
    ("vocos", "small"): (28096, 5888, 524544, 1880064),
    ("univnet", "default"): (14770560, 798976, 22121472, 79696896),
    ("univnet", "small"): (2471168, 207616, 5748480, 20704768),
    ("fastpitch", "default"): (46029632, 37888, 1751808, 6112256),
    ("fastpitch", "small"): (153408, 4352, 187392, 649728),
}


def _sizes(lib, model, d):
    blob, ws = getattr(lib, f"gvx_{model}_blob_floats"), getattr(lib, f"gvx_{model}_workspace_bytes")
    return blob, ws, (blob(C.byref(d)),) + tuple(ws(C.byref(d), B, T) for B, T in [(1, FRAMES[model][0]), (3, 37), (2, 200)])


@pytest.mark.parametrize("model,which", sorted(EXPECTED))
def test_blob_and_workspace_sizes_are_those_of_the_recorded_build(model, which):
    _, _, got = _sizes(_lib.load(), model, _dims(model, which))
    assert got == EXPECTED[model, which]


@pytest.mark.parametrize("model", sorted(FRAMES))
def test_size_functions_return_zero_for_what_the_forward_refuses(model):
    d = _dims(model, "default")
    blob, ws, sizes = _sizes(_lib.load(), model, d)
    assert all(v > 0 for v in sizes)
    assert blob(None) == 0 and ws(None, 1, 37) == 0   # null dims
    assert ws(C.byref(d), 0, 37) == 0                 # B = 0
    assert ws(C.byref(d), 1, FRAMES[model][1]) > 0 and ws(C.byref(d), 1, FRAMES[model][1] + 1) == 0   # T at its limit, and one past it


def test_every_generator_and_both_configs_are_recorded():
    assert sorted(EXPECTED) == sorted((m, w) for m in FRAMES for w in ("default", "small"))
