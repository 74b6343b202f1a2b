"""GPU: the Postnet's square 5-tap convolutions as Winograd F(4,5) (genvox_amd/csrc/winograd_conv.hip, winograd_f45.h), through
postnet_residual / gvx_postnet_forward, and on the CPU the transform identity itself.

What gates is the project's own budget: error / bound <= 1 under tests/test_gemm_gpu.py::_postnet_ref's five-layer bound and
|delta| <= 1e-3 against float64.  On top of it the tighter WINOGRAD_RATIO_LIMIT: four times the worst Winograd error / bound the
first run on an MI355X measured over every shape of this file.  Measured: 9.085e-06 of the bound (64 channels, B = 1, T = 5; the
bound carries every layer's error through the absolute weights of the layers behind it, which is why both forms sit five orders
below it), against 4.295e-06 for the direct form over the same shapes; at 512 channels, 2 x 41 frames, 2.376e-09 against 7.661e-10
and max |Winograd - direct| 1.9e-05.  Shape by shape the Winograd figure is 2 to 4.5 times the direct one.  The factor 4 leaves
room for other seeds.

Every row must equal, bit for bit, its batch-1 run at its own length: the path is chosen by (cin, cout, k) alone and tiles of
four frames start at frame 0 of each sequence, so neither the batch, nor T, nor a group boundary may change a bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from genvox_amd import _lib

MEASURED_WORST_RATIO = 9.085e-06    # Winograd error / bound, the worst of the first GPU run (module docstring)
MEASURED_WORST_DIRECT = 4.295e-06   # the direct form's, same shapes (not asserted: what the Winograd figure is read against)
WINOGRAD_RATIO_LIMIT = 4.0 * MEASURED_WORST_RATIO

EDGE_T = [1, 2, 3, 4, 5, 6, 7, 8, 9, 127, 128, 129, 130, 131]


# ---- CPU: the constants ---------------------------------------------------------------------------------------------------
def test_transform_identity_float64():
    """A^T [(G g) .* (B^T d)] is the 4-frame correlation of 5 taps with 8 frames, to 1e-12, for random g and d; the constants are
    read from the library (host only: no device is touched)."""
    lib = _lib.load()
    at, g, bt = np.zeros((4, 8)), np.zeros((8, 5)), np.zeros((8, 8))
    fn = lib.gvx_debug_winograd_constants
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * 3
    assert fn(at.ctypes.data, g.ctypes.data, bt.ctypes.data) == 0
    rng = np.random.default_rng(5)
    for _ in range(50):
        taps, d = rng.standard_normal(5), rng.standard_normal(8)
        got = at @ ((g @ taps) * (bt @ d))
        want = np.array([sum(taps[k] * d[i + k] for k in range(5)) for i in range(4)])
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # B^T and A^T are exact in fp32 (the kernels hold them as floats)
    assert np.array_equal(bt, bt.astype(np.float32)) and np.array_equal(at, at.astype(np.float32))


def test_the_choice_is_by_shape_alone():
    """gvx_debug_conv_plan under the three modes: host arithmetic, no device."""
    from genvox_amd.tacotron2 import dims_from_configs
    from tests.helpers import create_handle, fwd_configs

    lib = _lib.load()
    h = create_handle(lib, dims_from_configs(*fwd_configs("def")))
    try:
        plan = lambda *shape: lib.gvx_debug_conv_plan(h, *shape)
        assert plan(512, 512, 5) == 1 and plan(256, 256, 5) == 1          # mode 1 (default): wide square layers
        assert plan(64, 64, 5) == 0 and plan(80, 512, 5) == 0 and plan(512, 80, 5) == 0 and plan(512, 512, 3) == 0 and plan(520, 520, 5) == 0
        assert lib.gvx_model_set_winograd(h, 2) == 0
        assert plan(64, 64, 5) == 1 and plan(32, 32, 5) == 1 and plan(48, 48, 5) == 0 and plan(80, 512, 5) == 0 and plan(512, 512, 7) == 0
        assert lib.gvx_model_set_winograd(h, 0) == 0
        assert plan(512, 512, 5) == 0 and plan(64, 64, 5) == 0
        assert lib.gvx_model_set_winograd(h, 3) != 0 and lib.gvx_model_set_winograd(h, -1) != 0
        assert lib.gvx_debug_conv_plan(None, 512, 512, 5) == -1 and plan(0, 512, 5) == -1
    finally:
        lib.gvx_model_destroy(h)


def test_batched_plan_counts_the_tiles_of_all_slices():
    """plan_gemm over a batch of slices: the eight products of a Winograd layer at 32 x 800 frames are 1600 tiles of 128 x 128 (six
    rounds of 256 and 64: the last 256 rows go to the 64 x 64 launch), a group of 3200 tiles 800; one slice of the same shape would
    be 200 tiles and take the 64 x 128 shape.  With one slice the plan is gvx_debug_gemm_plan's, shape by shape."""
    from tests.helpers import GEMM_BRANCH_CASES, gemm_plan

    lib = _lib.load()
    fn = lib.gvx_debug_gemm_plan_batched
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)] * 2

    def batched(M, N, K, slices):
        tile, rows_big = C.c_int(), C.c_int()
        assert fn(M, N, K, slices, C.byref(tile), C.byref(rows_big)) == 0
        return tile.value, rows_big.value

    assert batched(6400, 512, 512, 8) == (4212, 6144)
    assert batched(3200, 512, 512, 8) == (4212, 3072)
    assert batched(6400, 512, 512, 1) == (2212, 0)
    assert batched(142, 512, 512, 8) == (2211, 0)        # one utterance of 568 frames: 2 x 4 x 8 = 64 tiles
    for c in GEMM_BRANCH_CASES:
        if not c.kmajor:
            assert batched(c.M, c.N, c.K, 1) == tuple(gemm_plan(lib, c.M, c.N, c.K)[1:3]), c


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _gemm_helpers():
    from tests import test_gemm_gpu as G
    return G


@pytest.fixture(scope="module")
def small_postnet():
    return _gemm_helpers()._postnet_model(False)   # postnet_embedding_dim = 64


@pytest.fixture(scope="module")
def full_postnet():
    return _gemm_helpers()._postnet_model(True)


def _set_group(model, seqs):
    fn = _lib.load().gvx_debug_set_winograd_group
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(model._handle, seqs) == 0


def _ragged_runs(B, T):
    """Length vectors of B rows that together hold 1, T and one length of each residue class mod 4 (where T has one)."""
    want = {1, T}
    for r in range(4):
        want.add(max((n for n in range(1, T + 1) if n % 4 == r), default=T))
    want = sorted(want, reverse=True)
    return [(want[i:i + B] + [T] * B)[:B] for i in range(0, len(want), B)]


def _check(model, sd64, mel, lengths, alone_cache, refs):
    """Rows of one call: bit-equal to the batch-1 run at their own length, zeros behind it, float64 within the budget.  Returns
    the worst error / bound."""
    G = _gemm_helpers()
    B, _, T = mel.shape
    out = model.postnet_residual(mel, None if lengths is None else torch.tensor(lengths, dtype=torch.int32))
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(B):
        n = T if lengths is None else lengths[b]
        if (b, n) not in alone_cache:
            alone_cache[b, n] = model.postnet_residual(mel[b:b + 1, :, :n].contiguous())
        assert torch.equal(out[b, :, :n], alone_cache[b, n][0]), (B, T, b, n)
        assert bool((out[b, :, n:] == 0).all()), (B, T, b, n)
        if (b, n) not in refs:
            refs[b, n] = G._postnet_ref(sd64, mel[b], n)
        want, bound = refs[b, n]
        diff = (out[b].double().cpu() - want).abs()
        ratio = float((diff / bound.clamp_min(1e-300))[:, :n].max())
        assert ratio <= 1.0 and float(diff.max()) <= 1e-3, (B, T, b, n, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", EDGE_T)
def test_winograd_edges_small_model(small_postnet, B, T):
    """64 channels, mode 2: T below one tile, at and around tile edges, a last tile that sticks out into the next sequence's rows;
    uniform and ragged lengths.  Mode 0 runs the same shapes for the comparison of the two error / bound figures."""
    model, sd64 = small_postnet
    lib = _lib.load()
    G = _gemm_helpers()
    mel = G._mel(B, 80, T, 20 * T + B)
    refs, worst = {}, {}
    try:
        for mode in (0, 2):
            model.set_winograd(mode)
            assert model.conv_plan(64, 64, 5) == (1 if mode else 0) and lib.gvx_debug_conv_plan(model._handle, 80, 64, 5) == 0
            alone, w = {}, 0.0
            for lengths in [None] + _ragged_runs(B, T):
                w = max(w, _check(model, sd64, mel, lengths, alone, refs))
            worst[mode] = w
    finally:
        model.set_winograd(1)
    print(f"winograd postnet B={B} T={T}: error / bound direct {worst[0]:.3e} winograd {worst[2]:.3e}")
    assert worst[2] <= WINOGRAD_RATIO_LIMIT, (B, T, worst)


@pytest.mark.gpu
def test_winograd_model_width_and_group_boundary(full_postnet):
    """512 channels in the default mode: B = 2, T = 41, lengths [41, 18]; and groups of one sequence give the bits of one group."""
    model, sd64 = full_postnet
    G = _gemm_helpers()
    assert model.conv_plan(512, 512, 5) == 1 and model.conv_plan(80, 512, 5) == 0 and model.conv_plan(512, 80, 5) == 0
    mel = G._mel(2, 80, 41, 411)
    lens = [41, 18]
    refs, alone = {}, {}
    worst = max(_check(model, sd64, mel, None, alone, refs), _check(model, sd64, mel, lens, alone, refs))
    one_group = model.postnet_residual(mel, torch.tensor(lens, dtype=torch.int32))
    try:
        for tiles in (11, 5, 1):   # T = 41 is 11 tiles: a group per sequence, groups that end inside a sequence, a group per tile
            _set_group(model, tiles)
            assert torch.equal(one_group, model.postnet_residual(mel, torch.tensor(lens, dtype=torch.int32))), tiles
    finally:
        _set_group(model, 0)
    model.set_winograd(0)
    try:
        direct = model.postnet_residual(mel, torch.tensor(lens, dtype=torch.int32))
        worst_direct = max(_check(model, sd64, mel, lens, {}, refs), 0.0)
    finally:
        model.set_winograd(1)
    print(f"winograd postnet 512 channels 2 x 41: error / bound direct {worst_direct:.3e} winograd {worst:.3e}, "
          f"max |winograd - direct| {float((one_group - direct).abs().max()):.3e}")
    assert not torch.equal(one_group, direct), "the two forms round differently: equal outputs mean the Winograd path did not run"
    assert worst <= WINOGRAD_RATIO_LIMIT, worst


@pytest.mark.gpu
def test_all_nan_mel_gives_all_nan(small_postnet, full_postnet):
    """A timed-out call poisons mel_out before the Postnet: NaN must come out of it everywhere, on both paths."""
    for model, mode in ((small_postnet[0], 2), (full_postnet[0], 1)):
        try:
            model.set_winograd(mode)
            for B, T in ((1, 1), (2, 7), (3, 8)):
                out = model.postnet_residual(torch.full((B, 80, T), float("nan"), device="cuda"))
                assert bool(torch.isnan(out).all()), (mode, B, T)
        finally:
            model.set_winograd(1)


@pytest.mark.gpu
def test_exact_workspace_dirty_or_zeroed(full_postnet):
    """gvx_postnet_forward on exactly gvx_postnet_workspace_bytes bytes: a workspace full of 0xFF gives the bits of a zeroed one
    (nothing is read before it is written); one byte less is refused."""
    model, _ = full_postnet
    lib = _lib.load()
    G = _gemm_helpers()
    model._ensure_packed()
    h, st = model._handle, torch.cuda.current_stream().cuda_stream
    for B, T, lens in ((2, 41, [41, 18]), (3, 6, None)):
        mel = G._mel(B, 80, T, 500 + T)
        ml = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
        n = lib.gvx_postnet_workspace_bytes(h, B, T)
        outs = []
        for fill in (0x00, 0xFF):
            ws = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
            ws[:1024] = 0   # the status words of a model workspace are cleared once by the caller
            out = torch.empty_like(mel)
            rc = lib.gvx_postnet_forward(h, mel.data_ptr(), None if ml is None else ml.data_ptr(), B, T, out.data_ptr(), ws.data_ptr(), n, st)
            torch.cuda.synchronize()
            assert rc == 0, lib.gvx_last_error()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[1]).all()), (B, T)
        assert lib.gvx_postnet_forward(h, mel.data_ptr(), None, B, T, out.data_ptr(), ws.data_ptr(), n - 1, st) == -5


def _tiny_configs():
    """Everything small, the Postnet 64 channels wide with three layers: the middle one is a Winograd layer in mode 2."""
    from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
    from tests.helpers import FWD_DIMS

    d = dict(FWD_DIMS["small"]["model"], postnet_embedding_dim=64)
    return Tacotron2Config(**d), AudioConfig(filter_length=1024, hop_length=256, n_mels=FWD_DIMS["small"]["n_mels"], log_func="np.log"), TextConfig(n_tokens=40)


def _tiny_model(sd):
    from genvox_amd.tacotron2 import Tacotron2

    m = Tacotron2(*_tiny_configs())
    m.load_state_dict(sd)
    m = m.to("cuda:0")
    m.set_winograd(2)
    assert m.conv_plan(64, 64, 5) == 1
    return m


@pytest.mark.gpu
def test_transformed_weights_follow_a_new_state_dict():
    """Seed-A weights, a run, seed-B weights into the same model, a run: the bits of a fresh model with seed B."""
    from genvox_amd import weights as gw

    cfgs = _tiny_configs()
    sd_a, sd_b = gw.generate_state_dict(*cfgs, seed=21), gw.generate_state_dict(*cfgs, seed=22)
    mel = torch.randn(2, cfgs[1].n_mels, 11, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    lens = torch.tensor([11, 6], dtype=torch.int32)
    m = _tiny_model(sd_a)
    out_a = m.postnet_residual(mel, lens)
    m.load_state_dict(sd_b)
    out_b = m.postnet_residual(mel, lens)
    fresh = _tiny_model(sd_b).postnet_residual(mel, lens)
    assert torch.equal(out_b, fresh) and not torch.equal(out_a, out_b)


@pytest.mark.gpu
def test_transformed_weights_follow_a_train_step():
    """One tiny train_step re-packs the blob on the device: the Postnet in eval mode afterwards gives the bits of a fresh model
    loaded from the stepped state_dict (whose blob the host packs)."""
    from genvox_amd import weights as gw
    from tests import train_ref64 as R
    from tests.helpers import bptt_lengths, train_step_mel_lengths

    cfgs = _tiny_configs()
    mc, ac, tc = cfgs
    B, L, T = 3, 6, 7
    m = _tiny_model(gw.generate_state_dict(mc, ac, tc, seed=23))
    mel = torch.randn(2, ac.n_mels, 11, generator=torch.Generator(device="cuda").manual_seed(4), device="cuda")
    lens = torch.tensor([11, 6], dtype=torch.int32)
    before = m.postnet_residual(mel, lens)
    inp = gw.synthetic_inputs(B, L, T, tc.n_tokens, ac.n_mels, seed=301, token_lengths=bptt_lengths("ragged", B, L), mel_lengths=train_step_mel_lengths(B, T))
    batch = {k: torch.from_numpy(v) for k, v in inp.items()}
    m.train_step(R.gpu_batch(batch, R.draw_masks(mc, ac.n_mels, B, L, T, 401)), m.get_criterion(), m.get_optimizer())
    m.check_status()
    m.eval()
    after = m.postnet_residual(mel, lens)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fresh = _tiny_model(sd).postnet_residual(mel, lens)
    assert torch.equal(after, fresh) and not torch.equal(after, before)
