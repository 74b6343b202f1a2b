"""Case table and float64 references of the attention-window tests (tests/test_attention_window_cpu.py pins the plans and the
centre margins on the CPU, tests/test_attention_window_gpu.py runs the cases).  Inputs are drawn as tests/test_forward_loops_gpu.py
draws them (its _memory, _gen and _choose_threshold, imported); the float64 decode is tests/forward_window_ref64.py."""
import collections

import torch

from genvox_amd import weights as gw
from tests import forward_ref as fr
from tests import forward_window_ref64 as fw
from tests.helpers import bptt_lengths, fwd_configs
from tests.test_forward_loops_gpu import WEIGHT_SETS, _choose_threshold, _gen, _memory

# name, layer sizes, handle environment, B, L, max_steps, lengths kind, (back, ahead), weight sets, expected windowed plan
# (kind, split_h, fold, graph), what the case is there for
WinCase = collections.namedtuple("WinCase", "name dims env B L T lengths window wsets plan why")
_BOTH, _PEAKY = ("plain", "peaky"), ("peaky",)
_LOOP0 = {"GVX_AR_RESIDENT_LOOP": "0"}

WINDOW_CASES = [
    # ---- the resident pair, one attention workgroup per row (attn_persistent_kernel<3, false, true, true>)
    WinCase("w2_1x1", "def", {}, 1, 1, 8, "full", (0, 1), _BOTH, (2, 0, 1, 0), "L = 1: the window is the row"),
    WinCase("w2_5x77", "def", {}, 5, 77, 12, "ragged", (1, 3), _BOTH, (2, 0, 1, 0), "ragged rows, one of a single token"),
    WinCase("w2_32x128", "def", {}, 32, 128, 10, "ragged", (3, 10), _BOTH, (2, 0, 1, 0), "every row and position the layout holds"),
    WinCase("w2_3x128_back0", "def", {}, 3, 128, 14, "short", (0, 1), _BOTH, (2, 0, 1, 0), "back = 0, the narrowest window"),
    # ---- rows of 129-256 tokens leave the pair (two workgroups per row have no window): launches per step
    WinCase("w0_16x256", "def", {}, 16, 256, 8, "ragged", (3, 10), _BOTH, (0, 1, 1, 1), "un-windowed kind 2, layout 2 -> kind 0, split_h"),
    WinCase("w0_17x129", "def", {}, 17, 129, 8, "ragged", (0, 1), _BOTH, (0, 1, 1, 1), "split_h: the step beside tiles (ar_attn_tiles_win_kernel)"),
    WinCase("w0_2x257", "def", {}, 2, 257, 8, "ragged", (1, 3), _BOTH, (0, 1, 1, 1), "three energy passes per row"),
    WinCase("w0_loop0_5x77", "def", _LOOP0, 5, 77, 20, "ragged", (1, 3), _BOTH, (0, 1, 1, 1), "two chunks of 16 steps: the graph-replayed case"),
    WinCase("w0_ar1_5x77", "def", {"GVX_AR_RESIDENT": "1", "GVX_AR_RESIDENT_LOOP": "0"}, 5, 77, 20, "ragged", (3, 10), _BOTH, (0, 1, 1, 1),
            "un-windowed kind 1 -> kind 0"),
    WinCase("w0_nosplit_5x77", "def", {"GVX_AR_RESIDENT_LOOP": "0", "GVX_AR_SPLIT_H": "0"}, 5, 77, 8, "ragged", (3, 10), _BOTH, (0, 0, 1, 1),
            "the step as a launch of its own (attn_step_win_kernel<4>)"),
    WinCase("w0_att16_3x40", "att16", {}, 3, 40, 8, "ragged", (1, 3), _BOTH, (0, 0, 1, 1), "attn_step_win_kernel<1>"),
    WinCase("w0_att256_3x40", "att256", {}, 3, 40, 8, "ragged", (0, 1), _BOTH, (0, 0, 1, 1), "attn_step_win_kernel<8>"),
    WinCase("w0_36x30", "def", {}, 36, 30, 6, "ragged", (1, 3), _BOTH, (0, 0, 0, 1), "more than 32 rows, no fold"),
    WinCase("w0_small_5x13", "small", {}, 5, 13, 20, "ragged", (3, 10), _BOTH, (0, 0, 1, 1), "a window wider than the row"),
    # ---- the two-kernel fallback (GVX_ATTN_SPLIT=1: attn_energy_kernel<DPL, true> + attn_context_kernel<true>)
    WinCase("w0_pair_5x77", "def", {"GVX_ATTN_SPLIT": "1"}, 5, 77, 8, "ragged", (1, 3), _BOTH, (0, 0, 1, 1), "energy + context kernels"),
    WinCase("w0_pair_att256_3x40", "att256", {"GVX_ATTN_SPLIT": "1"}, 3, 40, 8, "ragged", (3, 10), _BOTH, (0, 0, 1, 1), "... DPL = 4"),
]
BY_NAME = {c.name: c for c in WINDOW_CASES}
WSET = {w[0]: w for w in WEIGHT_SETS}

_SD, _REF = {}, {}


def state_dict(dims, wname):
    key = (dims, wname)
    if key not in _SD:
        _SD[key] = gw.generate_state_dict(*fwd_configs(dims), seed=WSET[wname][1], peaky_attention=WSET[wname][2])
    return _SD[key]


def inputs(case, wname):
    mc = fwd_configs(case.dims)[0]
    g = _gen(case.name, 1 if wname == "peaky" else 0)
    lengths = bptt_lengths(case.lengths, case.B, case.L)
    return {"lengths": torch.tensor(lengths, dtype=torch.int32), "memory": _memory(g, case.B, case.L, mc.encoder_embedding_dim, lengths),
            "keep": (torch.rand(2, case.T, case.B, mc.prenet_dim, generator=g) < 0.5).to(torch.uint8)}


def reference(case, wname, window=None):
    """(inputs, float64 windowed decode, gate threshold).  The threshold is chosen from the windowed free run's gates as
    test_forward_loops_gpu chooses it: rows stop at different steps and no stop step hangs on rounding."""
    window = case.window if window is None else window
    key = (case.name, wname, window)
    if key not in _REF:
        inp = inputs(case, wname)
        W = fr.decoder_weights(state_dict(case.dims, wname))
        lengths = inp["lengths"].tolist()
        free = fw.autoregressive_windowed(W, inp["memory"].double(), lengths, case.T, 2.0, inp["keep"], *window)
        thr = _choose_threshold(torch.sigmoid(free["gate"]))
        want = fw.autoregressive_windowed(W, inp["memory"].double(), lengths, case.T, thr, inp["keep"], *window)
        _REF[key] = (inp, want, thr)
    return _REF[key]
