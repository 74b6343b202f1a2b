"""GPU: gvx_hifigan_msd_forward and gvx_hifigan_msd_backward (csrc/hifigan_msd.hip) through the C ABI alone against the float64
restatement in tests/hifigan_msd_ref64.py - every map of every scale, every parameter gradient and d_wav, tensor by tensor.
Features, workspace, gradients and padded inputs all start as NaN; buffers have exactly their stated sizes, with a sentinel behind them
that must survive.

Tolerance.  Per tensor, e is the largest |float32 restatement - float64| (a number of the reference alone); the device may differ from
float64 by at most 8 x max(e, 2^-23 x the tensor's largest value).

LeakyReLU ties.  The backward reads its masks off the device's own maps.  Every decision that differs from float64's is asserted to be a
near-tie (the float64 value within its map's bound of 0), and the float64 gradient is taken with the restatement pinned to the device's
decisions.

Tiles.  Every convolution kernel works in tiles of GVX_HIFIGAN_MSD_TILE = 64 positions of one row: the forward kernels over the
positions L_i of their output map; the data-gradient kernels over the positions of ONE stride phase of their input map,
ceil(L_{i-1} / stride) = L_i.  So ``edge_lengths(cfg, s, i)`` - the two largest n at which map (s, i) still has at most 64 positions and
the two smallest at which it has more - puts the first tile edge of the forward kernel that writes map i AND of the data gradient that
leaves layer i under test.  LENGTHS takes that edge for every map of scale 0 and for map 0 of every scale (whose four lengths are an
odd and an even n on either side of a change of the pooled length n / 2 + 1), besides
  - n = 1, 2, 3 and 7: the shortest rows, every map of every scale 1 to 7 positions long;
  - n = 1, 5 and 9 (MIXED: 1, 2 and 3 positions into its first stride-4 layer, behind strides 1, 2, 2) and n = 1, 3 and 5 (TINY: the
    same behind strides 1, 2);
  - n = 257, 512 and 513: the weight gradient is summed in pieces of GVX_HIFIGAN_MSD_WG_RUN = 256 positions of a row, and these end the
    last piece of layer 0 (257) and of layer 1 (513: 257 positions) at 1 position and at a full run (512: 512 and 256 positions); the
    last map's edge lengths do the same for the deeper layers of MIXED (4097: 1025 and 257 positions into layers 3 and 4).
The ragged batches put a 1-sample row beside a row that has a second tile in every map of every scale, so the short rows' second tiles
lie wholly behind them."""
import ctypes as C
import functools

import pytest
import torch

from genvox_amd import _lib
from genvox_amd import hifigan_msd as _module_under_test  # noqa: F401  (the feature itself: absent before it)
from tests import hifigan_msd_ref64 as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
TILE = 64
WG_RUN = 256
SENTINEL = 64   # floats behind every exactly-sized buffer
CFGS = dict(TINY=SR.TINY, MIXED=SR.MIXED, DEFAULT=SR.DEFAULT)


def edge_lengths(cfg, s, i):
    n = 1
    while SR.map_lengths(cfg, n)[s][i] <= TILE:
        n += 1
    return (n - 2, n - 1, n, n + 1)


def lengths_of(cfg):
    out = set()
    for i in range(len(cfg["channels"]) + 1):
        out.update(edge_lengths(cfg, 0, i))
    for s in range(cfg["n_scales"]):
        out.update(edge_lengths(cfg, s, 0))
    out.update((1, 2, 3, 5, 7, 9, 257, 512, 513))
    return tuple(sorted(n for n in out if n >= 1))


LENGTHS = {name: lengths_of(CFGS[name]) for name in ("TINY", "MIXED")}
# the shortest row with a second tile in every map of every scale
LONGEST = {name: edge_lengths(CFGS[name], CFGS[name]["n_scales"] - 1, len(CFGS[name]["channels"]))[2] for name in ("TINY", "MIXED")}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


def test_the_tile_sizes_are_the_ones_the_lengths_were_chosen_for():
    header = open(__file__.replace("tests/test_hifigan_msd_gpu.py", "include/genvox_amd.h")).read()
    assert f"GVX_HIFIGAN_MSD_TILE = {TILE}" in header and f"GVX_HIFIGAN_MSD_WG_RUN = {WG_RUN}" in header
    assert "GVX_HIFIGAN_MSD_MFMA_IN_MULT = 8" in header and "GVX_HIFIGAN_MSD_MFMA_OUT_MULT = 16" in header
    internal = open(__file__.replace("tests/test_hifigan_msd_gpu.py", "genvox_amd/csrc/hifigan_msd_internal.h")).read()
    assert f"SD_TILE = {TILE};" in internal and f"SD_WG_RUN = {WG_RUN};" in internal


def test_the_lengths_hold_what_the_docstring_says():
    for name, cfg in (("TINY", SR.TINY), ("MIXED", SR.MIXED)):
        have = set(LENGTHS[name])
        for s, i in [(0, i) for i in range(len(cfg["channels"]) + 1)] + [(s, 0) for s in range(cfg["n_scales"])]:
            a, b, c, d = edge_lengths(cfg, s, i)
            pos = [SR.map_lengths(cfg, n)[s][i] for n in (a, b, c, d)]
            assert pos[0] <= TILE and pos[1] <= TILE and pos[2] > TILE and pos[3] > TILE and {a, b, c, d} <= have
        for s in range(1, cfg["n_scales"]):   # an odd and an even n on either side of a pooled length's change
            a, b, c, d = edge_lengths(cfg, s, 0)
            assert {a % 2, b % 2} == {0, 1} == {c % 2, d % 2} and SR.scale_samples(cfg, b)[1] != SR.scale_samples(cfg, c)[1]
        assert {1, 2, 3, 7} <= have
        first4 = cfg["strides"].index(4)   # positions into the first stride-4 layer
        assert {SR.map_lengths(cfg, n)[0][first4 - 1] for n in have} >= {1, 2, 3}
        for i in range(2):   # the last piece of a weight gradient: 1 position, and a full run
            tails = {SR.map_lengths(cfg, n)[0][i] % WG_RUN for n in have if SR.map_lengths(cfg, n)[0][i] >= WG_RUN}
            assert 1 in tails and 0 in tails
        assert all(SR.map_lengths(cfg, LONGEST[name])[s][-1] > TILE for s in range(cfg["n_scales"]))
    deep = SR.map_lengths(SR.MIXED, 4097)[0]
    assert 4097 in LENGTHS["MIXED"] and deep[2] == 1025 and deep[3] == 257


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _guarded(n_bytes):
    """A NaN-filled float32 buffer of n_bytes plus a sentinel run behind it."""
    assert n_bytes % 4 == 0
    return torch.full((n_bytes // 4 + SENTINEL,), NAN, dtype=torch.float32, device=DEV)


def _sentinel_intact(buf):
    return bool(torch.isnan(buf[-SENTINEL:]).all())


def dims_of(cfg):
    arrays = [(C.c_int32 * 8)(*cfg[k]) for k in ("channels", "kernel_sizes", "strides", "groups")]
    return _lib.gvx_hifigan_msd_dims(cfg["n_scales"], len(cfg["channels"]), *arrays, cfg["slope"])


class DiscNet:
    """A handle driven through the C ABI alone."""

    def __init__(self, cfg, sd):
        self.cfg, self.lib = cfg, _lib.load()
        self.dims = dims_of(cfg)
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.weights = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
        table = (_lib.gvx_weight_desc * len(self.weights))()
        for i, (k, v) in enumerate(self.weights.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        self.blob = torch.full((self.lib.gvx_hifigan_msd_blob_floats(C.byref(self.dims)),), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.lib.gvx_hifigan_msd_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream()))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_hifigan_msd_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_hifigan_msd_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_hifigan_msd_destroy(self.h)

    def views(self, buf, B, n):
        """[scale][map] views [B, C, L] of a features-shaped float32 buffer."""
        e = (_lib.gvx_hifigan_msd_entry * 40)()
        count = self.lib.gvx_hifigan_msd_layout(C.byref(self.dims), B, n, e, 40)
        per = len(self.cfg["channels"]) + 1
        assert count == per * self.cfg["n_scales"]
        flat = []
        for i in range(count):
            x = e[i]
            assert x.byte_offset % 256 == 0 and x.length == SR.map_lengths(self.cfg, n)[i // per][i % per]
            flat.append(buf[x.byte_offset // 4: x.byte_offset // 4 + B * x.channels * x.length].as_strided(
                (B, x.channels, x.length), (x.stride_b, x.stride_c, x.stride_l)))
        return [flat[s * per:(s + 1) * per] for s in range(self.cfg["n_scales"])]

    def forward(self, wav, lens=None):
        """-> (the features buffer, its maps as [scale][map] views)."""
        B, n = wav.shape
        fb, wb = self.lib.gvx_hifigan_msd_features_bytes(C.byref(self.dims), B, n), self.lib.gvx_hifigan_msd_workspace_bytes(C.byref(self.dims), B, n, 0)
        feats, ws = _guarded(fb), _guarded(wb)
        _lib.check(self.lib.gvx_hifigan_msd_forward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(), fb,
                                                    ws.data_ptr(), wb, stream()))
        torch.cuda.synchronize()
        assert _sentinel_intact(feats) and _sentinel_intact(ws), "the forward wrote behind its features buffer or its workspace"
        return feats, self.views(feats, B, n)

    def cotangent_buffer(self, G, B, n, lens):
        """d_features: NaN everywhere, G (or 0 where a map has no cotangent) inside every row's own lengths."""
        buf = _guarded(self.lib.gvx_hifigan_msd_features_bytes(C.byref(self.dims), B, n))
        for s, scale in enumerate(self.views(buf, B, n)):
            for i, view in enumerate(scale):
                for b in range(B):
                    L = SR.map_lengths(self.cfg, n if lens is None else lens[b])[s][i]
                    view[b, :, :L] = 0.0 if G[s][i] is None else G[s][i][b, :, :L].to(DEV, torch.float32)
        return buf

    def backward(self, wav, lens, feats, d_feats, want_params=True, want_wav=True):
        B, n = wav.shape
        grads = {k: torch.full(s, NAN, dtype=torch.float32, device=DEV) for k, s in self.shapes.items()} if want_params else {}
        table = (_lib.gvx_weight_desc * max(len(grads), 1))()
        for i, (k, g) in enumerate(grads.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        d_wav = torch.full((B, n), NAN, dtype=torch.float32, device=DEV) if want_wav else None
        wb = self.lib.gvx_hifigan_msd_workspace_bytes(C.byref(self.dims), B, n, 1)
        ws = _guarded(wb)
        _lib.check(self.lib.gvx_hifigan_msd_backward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(),
                                                     d_feats.data_ptr(), table if grads else None, len(grads), d_wav.data_ptr() if want_wav else None,
                                                     ws.data_ptr(), wb, stream()))
        torch.cuda.synchronize()
        assert _sentinel_intact(ws), "the backward wrote behind its workspace"
        if want_wav:
            grads["wav"] = d_wav
        return grads


@functools.lru_cache(maxsize=None)
def _net(name):
    cfg = CFGS[name]
    sd = SR.random_state(cfg, seed=11)
    return cfg, sd, DiscNet(cfg, sd)


def _poisoned(wav, lens):
    wav = wav.clone()
    if lens is not None:
        for b, nb in enumerate(lens):
            wav[b, nb:] = NAN
    return wav.to(DEV, torch.float32)


@functools.lru_cache(maxsize=None)
def _forward_case(name, B, n, lens):
    """(wav, float64 reference of the forward): computed once, shared, never changed."""
    cfg, sd, _ = _net(name)
    wav = SR.random_wav(B, n, seed=100 * B + n)
    return wav, SR.reference(sd, wav, lens, cfg)


def _check_forward(name, B, n, lens=None):
    cfg, sd, net = _net(name)
    wav, ref = _forward_case(name, B, n, lens)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(_poisoned(wav, lens), lens_d)
    worst = 0.0
    for s, scale in enumerate(maps):
        for i, got in enumerate(scale):
            got = got.double().cpu()
            assert got.shape == ref["maps"][s][i].shape
            for b in range(B):
                L = SR.map_lengths(cfg, n if lens is None else lens[b])[s][i]
                assert not got[b, :, L:].any() and not torch.isnan(got[b]).any(), f"{name} {B} x {n}: map ({s}, {i}) row {b} is not exact zeros behind {L}"
                d, tol = (got[b, :, :L] - ref["maps"][s][i][b, :, :L]).abs().max().item(), ref["map_tol"][s][i]
                worst = max(worst, d / tol)
                assert d <= tol, f"{name} {B} x {n} {lens}: map ({s}, {i}) row {b}: {d:.3e} from float64, above the bound {tol:.3e} (float32 restatement {ref['map_err'][s][i]:.3e})"
    print(f"{name} {B} x {n} {lens}: largest forward error {worst:.3f} of its bound")
    return wav, ref, feats, maps


def _check_backward(name, B, n, lens=None, only=None, seed=5):
    """Gradients against float64 pinned to the device's LeakyReLU decisions -> (wav, lens, feats, d_feats, grads, largest share of a bound)."""
    cfg, sd, net = _net(name)
    wav, free, feats, maps = _check_forward(name, B, n, lens)
    flips = 0
    for s, scale in enumerate(maps):
        for i, got in enumerate(scale[:-1]):
            want = free["maps"][s][i]
            differ = (got.cpu() > 0) != (want > 0)
            flips += int(differ.sum())
            assert (want[differ].abs() <= free["map_tol"][s][i]).all(), f"map ({s}, {i}): a sign differs from float64 away from 0"
    G = SR.random_cotangents(cfg, B, n, seed, only)
    ref = SR.reference(sd, wav, lens, cfg, G, SR.masks_from_maps(maps, cfg["slope"]))
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    wav_d = _poisoned(wav, lens)
    d_feats = net.cotangent_buffer(G, B, n, lens)
    grads = net.backward(wav_d, lens_d, feats, d_feats)
    what, worst = f"{name} {B} x {n} {lens or ''} cotangents {sorted(only) if only else 'on all maps'} ({flips} LeakyReLU decisions differ)", 0.0
    for key, want in ref["grads"].items():
        g = grads[key].double().cpu()
        assert g.shape == want.shape and not torch.isnan(g).any(), f"{what}: {key} holds NaN or has the wrong shape"
        d, tol = (g - want).abs().max().item(), ref["grad_tol"][key]
        print(f"  d {key}: {d:.3e} of {tol:.3e}")
        assert d <= tol, f"{what}: d {key} differs from float64 by {d:.3e}, above the bound {tol:.3e} (float32 restatement: {ref['grad_err'][key]:.3e})"
        worst = max(worst, d / tol if tol > 0.0 else 0.0)   # a bound of 0: a gradient no cotangent reaches, exact zeros on both sides
    for b in range(B):
        nb = n if lens is None else lens[b]
        assert not grads["wav"][b, nb:].any(), f"{what}: d_wav row {b} is not exact zeros behind {nb}"
    print(f"{what}: largest gradient error {worst:.3f} of its bound")
    return wav_d, lens_d, feats, d_feats, grads, worst


@pytest.mark.parametrize("name,n", [(name, n) for name in ("TINY", "MIXED") for n in LENGTHS[name]])
def test_forward_and_backward_one_row(name, n):
    """B = 1: every map, then every gradient with cotangents on all maps."""
    _check_backward(name, 1, n)


@pytest.mark.parametrize("name", ["TINY", "MIXED"])
def test_ragged_rows_partial_calls_and_repeats(name):
    """A ragged B = 3, a 1-sample row beside the longest: rows are their one-row runs bit for bit, forward and d_wav; the d_wav-only and
    the parameters-only call give the full call's bits; so does a second call."""
    cfg, sd, net = _net(name)
    lens = (LONGEST[name], 1, LONGEST[name] // 2 + 1)
    wav_d, lens_d, feats, d_feats, full, _ = _check_backward(name, 3, lens[0], lens)
    maps = net.views(feats, 3, lens[0])
    feats2, maps2 = net.forward(wav_d, lens_d)
    assert torch.equal(feats2[:-SENTINEL].view(torch.int32), feats[:-SENTINEL].view(torch.int32)), f"{name}: two forward calls differ"
    again = net.backward(wav_d, lens_d, feats, d_feats)
    dx_only = net.backward(wav_d, lens_d, feats, d_feats, want_params=False)
    dw_only = net.backward(wav_d, lens_d, feats, d_feats, want_wav=False)
    assert set(dx_only) == {"wav"} and set(dw_only) == set(sd)
    for k, v in full.items():
        assert torch.equal(again[k], v), f"{name}: d {k} differs between two calls"
        other = dx_only if k == "wav" else dw_only
        assert torch.equal(other[k], v), f"{name}: d {k} of a partial call differs from the full call"
    G_views = net.views(d_feats, 3, lens[0])
    for b, nb in enumerate(lens):
        one = wav_d[b:b + 1, :nb].contiguous()
        f1, m1 = net.forward(one)
        for s in range(cfg["n_scales"]):
            for i, m in enumerate(m1[s]):
                assert torch.equal(maps[s][i][b, :, :m.shape[2]], m[0]), f"{name}: row {b} of {nb} samples, map ({s}, {i}) differs from its one-row run"
        d1 = net.cotangent_buffer([[g[b:b + 1, :, :m.shape[2]].cpu() for g, m in zip(gs, ms)] for gs, ms in zip(G_views, m1)], 1, nb, None)
        alone = net.backward(one, None, f1, d1, want_params=False)
        assert torch.equal(alone["wav"][0], full["wav"][b, :nb]), f"{name}: d_wav of row {b} differs from its one-row run"


@pytest.mark.parametrize("name,only", [("MIXED", "scores"), ("MIXED", "middle"), ("TINY", "scores"), ("TINY", "middle")])
def test_backward_single_cotangents(name, only):
    """A cotangent on the scores alone, and one on a single middle map of the pooled scale: the other maps have none."""
    cfg = CFGS[name]
    last = len(cfg["channels"])
    which = {(s, last) for s in range(cfg["n_scales"])} if only == "scores" else {(1, 2)}
    _check_backward(name, 2, 200, only=frozenset(which))


def test_default_shape():
    """The published shape once, B = 2 and ragged at 300 and 130 samples: three scales, every grouped layer and the dense one."""
    _, _, _, _, _, worst = _check_backward("DEFAULT", 2, 300, (300, 130))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["TINY", "MIXED"])
def test_a_row_of_no_samples_is_silent(name):
    """The host cannot see device lengths: a row of 0 samples that reaches the kernels comes out as all-zero maps and an all-zero d_wav
    row, its neighbour as its one-row run, and nothing is written behind a buffer."""
    cfg, sd, net = _net(name)
    lens = (70, 0)
    wav = _poisoned(SR.random_wav(2, 70, 7), lens)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav, lens_d)
    _, alone = net.forward(wav[:1].contiguous())
    for s, scale in enumerate(maps):
        for i, m in enumerate(scale):
            assert not m[1].any() and not torch.isnan(m).any(), f"{name}: map ({s}, {i}) of the empty row is not exact zeros"
            assert torch.equal(m[0], alone[s][i][0])
    d_feats = _guarded(feats.numel() * 4 - SENTINEL * 4)
    for scale in net.views(d_feats, 2, 70):
        for v in scale:
            v[0] = 1.0
    grads = net.backward(wav, lens_d, feats, d_feats)
    assert not grads["wav"][1].any() and not any(torch.isnan(g).any() for g in grads.values())


def test_bad_arguments_are_refused_before_a_launch():
    cfg, sd, net = _net("TINY")
    lib, wav = net.lib, torch.zeros(1, 64, device=DEV)
    fb = lib.gvx_hifigan_msd_features_bytes(C.byref(net.dims), 1, 64)
    wb = lib.gvx_hifigan_msd_workspace_bytes(C.byref(net.dims), 1, 64, 0)
    feats, ws = _guarded(fb), _guarded(wb)
    assert lib.gvx_hifigan_msd_forward(net.h, wav.data_ptr(), None, 0, 64, feats.data_ptr(), fb, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_hifigan_msd_forward(net.h, wav.data_ptr(), None, 1, 0, feats.data_ptr(), fb, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_hifigan_msd_forward(net.h, wav.data_ptr(), None, 1, (1 << 24) + 1, feats.data_ptr(), fb, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_hifigan_msd_forward(net.h, wav.data_ptr(), None, 1, 64, feats.data_ptr(), fb - 256, ws.data_ptr(), wb, stream()) != 0
    assert lib.gvx_hifigan_msd_forward(net.h, wav.data_ptr(), None, 1, 64, feats.data_ptr(), fb, None, 0, stream()) != 0
    assert lib.gvx_hifigan_msd_backward(net.h, wav.data_ptr(), None, 1, 64, feats.data_ptr(), feats.data_ptr(), None, 0, None, ws.data_ptr(), wb, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(feats).all()), "a refused call wrote to the features buffer"
