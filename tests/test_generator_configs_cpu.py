"""CPU: what the table of tests/hifigan_layer_cases.py holds, kernel by kernel, and the path every layer of the configurations ODD, ONE,
FOUR (tests/hifigan_ref64.py, their BigVGAN forms in tests/bigvgan_ref64.py) and ODD, DEEP (tests/melgan_ref64.py) takes - the dispatch
rule of hg_launch / mg_launch restated in a few lines, so that a later edit of a table row or of a config cannot silently move it off
the kernel, the tile or the tail it was chosen for.  Also: the C ABI's dims checks and the Python config classes accept every one of
those configurations (no GPU call)."""
import ctypes as C

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.bigvgan import BigVGANGenerator
from genvox_amd.configs import AudioConfig, BigVGANConfig, HiFiGANConfig, MelGANConfig
from genvox_amd.hifigan import HiFiGANGenerator
from genvox_amd.melgan import MelGANGenerator
from tests import bigvgan_ref64 as BR
from tests import hifigan_layer_cases as K
from tests import hifigan_ref64 as HR
from tests import melgan_ref64 as MR

TILE = {"tile128": 128, "tile64": 64, "tile32": 32}


def cpad(n_mels: int) -> int:
    return (n_mels + 3) & ~3


def path(cin: int, cout: int) -> str:
    """hg_launch / mg_launch / hgb_dgrad: Cout >= 32 and Cin a multiple of 4 go to the tile chosen by Cout, everything else to the
    dot-product kernel (eight lanes per element where Cout == 1)."""
    if cout >= 32 and cin % 4 == 0:
        return "tile128" if cout >= 128 else ("tile64" if cout > 32 else "tile32")
    return "valu8" if cout == 1 else "valu"


def hifigan_layers(cfg):
    """(name, Cin, Cout, taps, dilation, phases) of every launch of the forward, in order."""
    c = cfg["c0"]
    out = [("conv_pre", cpad(cfg["n_mels"]), c, 7, 1, 1)]
    for i, r in enumerate(cfg["rates"]):
        out.append((f"ups.{i}", c, c // 2, 2, 0, r))
        c //= 2
        for j, (k, ds) in enumerate(zip(cfg["kernels"], cfg["dilations"])):
            for m, d in enumerate(ds):
                out.append((f"stage {i} block {j} convs1.{m}", c, c, k, d, 1))
                if cfg["resblock"] == "1":
                    out.append((f"stage {i} block {j} convs2.{m}", c, c, k, 1, 1))
    return out + [("conv_post", c, 1, 7, 1, 1)]


def melgan_layers(cfg):
    c = cfg["base_channels"]
    out = [("pre", cpad(cfg["n_mels"]), c, 7, 1, 1)]
    for i, r in enumerate(cfg["ratios"]):
        out.append((f"ups.{i}", c, c // 2, 2, 0, r))
        c //= 2
        for j in range(cfg["n_res"]):
            out += [(f"res.{i}.{j}.conv", c, c, 3, cfg["dil_base"] ** j, 1), (f"res.{i}.{j}.tail", c, c, 2, 0, 1)]
    return out + [("post", c, 1, 7, 1, 1)]


def _paths(layers):
    return {name: path(cin, cout) for name, cin, cout, *_ in layers}


def _of(layers, name):
    return next(l for l in layers if l[0] == name)


# ---- the table of the layer test
def test_the_dispatch_restated_here_is_the_tables():
    for cin in range(1, 150):
        for cout in (1, 2, 31, 32, 33, 127, 128, 129, 260):
            assert path(cin, cout) == K.kernel_of(cin, cout)


@pytest.mark.parametrize("kernel", K.FORWARD_KERNELS)
def test_the_table_holds_every_item_for_every_forward_kernel(kernel):
    rows = [c for c in K.CASES if not c.grad and K.kernel_of(c.cin, c.cout) == kernel]
    assert {(c.taps, c.dil) for c in rows if c.phases == 1} >= set(K.WINDOWS)
    assert {c.phases for c in rows} >= set(K.PHASES)
    if kernel in TILE:   # every phase count at an odd number of column tiles: tile + n_tiles * phase with n_tiles = 1 or 3
        for r in K.PHASES:
            assert any(c.phases == r and ((c.cout + TILE[kernel] - 1) // TILE[kernel]) % 2 == 1 for c in rows), r
    plain = [c for c in rows if c.in_mul == 1 and c.phases == 1]
    positions = {n for c in plain for n in c.rows}
    assert positions >= {1, 2, 127, 128, 129, 257}
    assert any(K.left_of(c) >= 2 and K.left_of(c) in c.rows and K.left_of(c) + 1 in c.rows for c in plain), "rows of left and left + 1 positions"
    assert any(len(c.rows) == 3 and c.rows[1:] == (1, (c.rows[0] + 1) // 2) and c.rows[0] > 128 for c in rows), "a ragged batch (L, 1, (L + 1) // 2)"
    assert any(c.in_mul == 6 and max(c.rows) == 22 and len(set(c.rows)) > 1 for c in rows), "lens in units of in_mul"
    assert {c.epi for c in rows} >= set(K.EPILOGUES)
    assert {c.act for c in rows} == {True, False}
    assert {c.slope for c in rows if c.act} >= set(K.SLOPES)
    assert {c.zero_tail for c in rows} == {True, False}


def test_the_table_holds_the_channels_the_output_kernel_and_every_gradient_kernel():
    assert {(c.cin, c.cout) for c in K.CASES} >= set(K.CHANNELS)
    out = [c for c in K.CASES if K.kernel_of(c.cin, c.cout, c.grad) == "valu8"]
    assert out and all(c.tanh and c.cout == 1 for c in out)
    assert not any(c.tanh for c in K.CASES if K.kernel_of(c.cin, c.cout, c.grad) != "valu8")
    grads = [c for c in K.CASES if c.grad]
    assert {(c.cin, c.cout) for c in grads} >= set(K.CHANNELS)
    assert {(c.taps, c.dil) for c in grads} >= set(K.WINDOWS)
    for kernel in K.FORWARD_KERNELS:
        assert {c.epi for c in grads if K.kernel_of(c.cin, c.cout, True) == kernel} >= set(K.GRAD_EPILOGUES), kernel
    assert {c.slope for c in grads if "mask" in c.epi} >= set(K.SLOPES)
    # K tails inside a 32-channel block other than a padded mel's, a K block that is mostly padding, column tails of a few columns
    assert {c.cin % 32 for c in K.CASES if K.kernel_of(c.cin, c.cout) in TILE} >= {0, 4, 8, 16}
    assert {c.cout % TILE[k] for c in K.CASES for k in [K.kernel_of(c.cin, c.cout)] if k in TILE} >= {4, 8, 32, 36}
    assert (34, 34) in {(c.cin, c.cout) for c in K.CASES if K.kernel_of(c.cin, c.cout) == "valu"}
    assert all((c.taps - 1) * c.dil <= 72 for c in K.CASES) and 60 <= len(K.CASES) <= 70


def test_every_mask_value_is_away_from_zero_and_every_input_is_a_float32_value():
    for i, case in enumerate(K.CASES):
        t = K.inputs(case, seed=100 + i)
        for v in t.values():
            assert torch.equal(v, v.float().double())
        if "mask" in case.epi:
            assert t["mask"].abs().min().item() > K.MASK_MARGIN
            assert (t["mask"] > 0).any() and (t["mask"] < 0).any()


# ---- the configurations: accepted by the C ABI and by the config classes
def _audio(n_mels, hop):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = hop, n_mels   # 5 mels and a hop of 4 are below a preprocessing config's ranges: a test's sizes
    return ac


def _hifigan_config(cfg, cls=HiFiGANConfig, **more):
    return cls(upsample_initial_channel=cfg["c0"], upsample_rates=cfg["rates"], upsample_kernel_sizes=[2 * r for r in cfg["rates"]],
               resblock=cfg["resblock"], resblock_kernel_sizes=cfg["kernels"], resblock_dilation_sizes=cfg["dilations"], **more)


@pytest.mark.parametrize("name", HR.NEVER_RUN)
def test_hifigan_configurations_are_accepted(name):
    cfg, lib = getattr(HR, name), _lib.load()
    mc = _hifigan_config(cfg, leaky_slope=cfg["slope"], post_leaky_slope=cfg["post_slope"])
    d = HiFiGANGenerator(mc, _audio(cfg["n_mels"], HR.hop(cfg))).dims()
    assert lib.gvx_hifigan_blob_floats(C.byref(d)) > 0 and lib.gvx_hifigan_workspace_bytes(C.byref(d), 2, 11) > 0
    assert lib.gvx_hifigan_tape_bytes(C.byref(d), 2, 5) > 0 and lib.gvx_hifigan_backward_workspace_bytes(C.byref(d), 2, 5) > 0
    assert (d.n_mels, d.n_resblocks, d.n_stages) == (cfg["n_mels"], len(cfg["kernels"]), len(cfg["rates"]))
    assert (d.slope, d.post_slope) == (C.c_float(cfg["slope"]).value, C.c_float(cfg["post_slope"]).value)


@pytest.mark.parametrize("name", BR.NEVER_RUN)
def test_bigvgan_configurations_are_accepted(name):
    cfg, lib = getattr(BR, name), _lib.load()
    mc = _hifigan_config(cfg, BigVGANConfig, activation=cfg["activation"], snake_logscale=cfg["logscale"], use_tanh_at_final=cfg["tanh"],
                         use_bias_at_final=cfg["bias"])
    d = BigVGANGenerator(mc, _audio(cfg["n_mels"], BR.hop(cfg))).dims()
    assert lib.gvx_bigvgan_blob_floats(C.byref(d)) > 0 and lib.gvx_bigvgan_workspace_bytes(C.byref(d), 2, 11) > 0


@pytest.mark.parametrize("name", MR.NEVER_RUN)
def test_melgan_configurations_are_accepted(name):
    cfg, lib = getattr(MR, name), _lib.load()
    mc = MelGANConfig(base_channels=cfg["base_channels"], upsample_ratios=cfg["ratios"], n_residual_layers=cfg["n_res"], dilation_base=cfg["dil_base"],
                      leaky_slope=cfg["slope"])
    d = MelGANGenerator(mc, _audio(cfg["n_mels"], MR.hop(cfg))).dims()
    assert lib.gvx_melgan_blob_floats(C.byref(d)) > 0 and lib.gvx_melgan_workspace_bytes(C.byref(d), 2, 11) > 0
    assert lib.gvx_melgan_tape_bytes(C.byref(d), 2, 5) > 0 and lib.gvx_melgan_backward_workspace_bytes(C.byref(d), 2, 5) > 0
    assert (d.n_mels, d.n_residual_layers, d.dilation_base) == (cfg["n_mels"], cfg["n_res"], cfg["dil_base"])


# ---- the configurations: the path of every layer
def test_hifigan_odd_takes_the_paths_it_was_chosen_for():
    cfg, layers = HR.ODD, hifigan_layers(HR.ODD)
    p = _paths(layers)
    assert cpad(cfg["n_mels"]) == 40 != cfg["n_mels"]
    assert _of(layers, "conv_pre")[1:3] == (40, 144) and p["conv_pre"] == "tile128" and 144 % 128 == 16
    assert _of(layers, "ups.0")[1:3] == (144, 72) and _of(layers, "ups.0")[5] == 6 and p["ups.0"] == "tile64"
    assert _of(layers, "ups.1")[1:3] == (72, 36) and _of(layers, "ups.1")[5] == 2 and p["ups.1"] == "tile64"
    convs = [l for l in layers if "convs" in l[0]]
    assert {l[1:3] for l in convs} == {(72, 72), (36, 36)} and {p[l[0]] for l in convs} == {"tile64"}
    assert {l[1] % 32 for l in layers} >= {8, 4, 16} and {l[2] % 64 for l in layers if p[l[0]] == "tile64"} == {8, 36}
    assert len(cfg["kernels"]) == 2 and p["conv_post"] == "valu8"
    assert max((l[3] - 1) * l[4] for l in convs) == 72 == (9 - 1) * 9
    assert any(l[4] % 2 == 0 for l in convs)   # an even dilation in resblock "1"
    # 66 / 132 and 132 / 264 positions at 11 and 22 frames: either side of a 128-position tile at both stages
    assert [11 * 6, 22 * 6] == [66, 132] and [11 * 12, 22 * 12] == [132, 264]


def test_hifigan_one_takes_the_paths_it_was_chosen_for():
    cfg, layers = HR.ONE, hifigan_layers(HR.ONE)
    p = _paths(layers)
    assert cpad(cfg["n_mels"]) == 8 and len(cfg["rates"]) == 1 and len(cfg["kernels"]) == 1
    assert _of(layers, "conv_pre")[1:3] == (8, 64) and p["conv_pre"] == "tile64"
    assert _of(layers, "ups.0")[1:3] == (64, 32) and _of(layers, "ups.0")[5] == 10 and p["ups.0"] == "tile32"
    convs = [l for l in layers if "convs" in l[0]]
    assert len(convs) == 2 and {p[l[0]] for l in convs} == {"tile32"}
    assert max((l[3] - 1) * l[4] // 2 for l in convs) == 36   # left = 36: wider than the 10 positions of a 1-frame row
    assert (cfg["slope"], cfg["post_slope"]) == (0.0, 1.0) and p["conv_post"] == "valu8"


def test_hifigan_four_takes_the_paths_it_was_chosen_for():
    cfg, layers = HR.FOUR, hifigan_layers(HR.FOUR)
    p = _paths(layers)
    assert len(cfg["kernels"]) == 4   # GVX_HIFIGAN_MAX_RESBLOCKS
    assert p["conv_pre"] == "tile32" and p["conv_post"] == "valu8"
    assert {v for k, v in p.items() if k not in ("conv_pre", "conv_post")} == {"valu"}
    assert {l[1:3] for l in layers if "convs" in l[0]} == {(16, 16), (8, 8)} and {l[3] for l in layers if "convs" in l[0]} == {3, 5, 7, 9}


def test_the_bigvgan_forms_share_those_structures():
    for name, base in (("ODD_BETA", HR.ODD), ("FOUR_SNAKE", HR.FOUR), ("ONE_CLAMP", HR.ONE)):
        cfg = getattr(BR, name)
        assert all(cfg[k] == base[k] for k in ("n_mels", "c0", "rates", "resblock", "kernels", "dilations"))
    assert (BR.FOUR_SNAKE["activation"], BR.FOUR_SNAKE["logscale"]) == ("snake", False)
    assert (BR.ONE_CLAMP["tanh"], BR.ONE_CLAMP["bias"]) == (False, False) and BR.ODD_BETA["activation"] == "snakebeta"


def test_melgan_odd_takes_the_paths_it_was_chosen_for():
    cfg, layers = MR.ODD, melgan_layers(MR.ODD)
    p = _paths(layers)
    assert cpad(cfg["n_mels"]) == 40 and _of(layers, "pre")[1:3] == (40, 136) and p["pre"] == "tile128"
    assert _of(layers, "ups.0")[1:3] == (136, 68) and _of(layers, "ups.0")[5] == 6 and p["ups.0"] == "tile64"
    assert {p[l[0]] for l in layers if l[0].startswith("res.0.")} == {"tile64"} and 68 % 64 == 4
    assert _of(layers, "ups.1")[1:3] == (68, 34) and p["ups.1"] == "tile64"
    stage1 = [l for l in layers if l[0].startswith("res.1.")]
    assert {l[1:3] for l in stage1} == {(34, 34)} and {p[l[0]] for l in stage1} == {"valu"}   # Cout >= 32, Cin % 4 != 0
    assert p["post"] == "valu8" and [l[4] for l in layers if l[0].endswith(".conv")] == [1, 5, 1, 5]


def test_melgan_deep_takes_the_paths_it_was_chosen_for():
    cfg, layers = MR.DEEP, melgan_layers(MR.DEEP)
    p = _paths(layers)
    assert cpad(cfg["n_mels"]) == 8 and p["pre"] == "tile64" and _of(layers, "ups.0")[1:3] == (64, 32) and p["ups.0"] == "tile32"
    convs = [l for l in layers if l[0].endswith(".conv")]
    assert len(convs) == 8 and {l[4] for l in convs} == {1} and {p[l[0]] for l in layers if l[0].startswith("res.")} == {"tile32"}
    assert cfg["slope"] == 1.0 and p["post"] == "valu8"


def test_the_one_number_gradient_of_melgan_odd_1_x_11_is_decided_by_the_ulp_at_scale():
    """d post.bias is one number (tests/melgan_ref64.py, ``BACKWARD_MEL_SEEDS``): for the mel the case draws, 8 ulp at its scale - the
    term of the rule that no host changes - is above the 90th percentile of how far float32 arithmetic moves it."""
    from tests import melgan_grad_ref64 as GR

    (name, B, T), seed = next(iter(MR.BACKWARD_MEL_SEEDS.items()))
    cfg = getattr(MR, name)
    sd, mel = MR.random_state(cfg, seed=11), MR.random_mel(cfg, B, T, seed)
    G = torch.randn(B, T * MR.hop(cfg), generator=torch.Generator().manual_seed(1000 * B + T), dtype=torch.float64)
    value, moved = GR.one_number_movement(sd, cfg, mel, G)
    floor = GR.FACTOR * GR.ULP * abs(value)
    print(f"d post.bias {value:.4f}: 8 ulp at scale {floor:.3e}, 90th percentile of the movement {moved:.3e}")
    assert moved <= floor
