"""GPU: gvx_melgan_disc_forward and gvx_melgan_disc_backward (csrc/melgan_disc.hip) through the C ABI against the float64 restatement in
tests/melgan_disc_ref64.py - every map of every scale, every parameter gradient and d_wav, tensor by tensor - and the module's autograd
node against the C-ABI call.  Features, workspace, gradients and padded inputs all start as NaN; buffers have exactly their stated
sizes, with a sentinel behind them that must survive.

Tolerance.  Per tensor, e is the largest |float32 restatement - float64| (a number of the reference alone); the device may differ from
float64 by at most 8 x max(e, 2^-23 x the tensor's largest value).

LeakyReLU ties.  The backward reads its masks off the device's own maps.  Every decision that differs from float64's is asserted to be a
near-tie (the float64 value within 8 x its map's float32 error of 0), and the float64 gradient is taken with the restatement pinned to
the device's decisions.

Tiles.  Every convolution kernel - md_fwd_kernel and md_fwd_one_kernel over output positions, md_dx_kernel over input positions -
works in tiles of GVX_MELGAN_DISC_TILE = 64 positions of one row, and a map of scale k, layer i has L_i(n >> k) positions.
EDGE_LENGTHS puts an odd and an even length on each side of the 64 | 65 edge of: layer 0 of scale 0 (n = 63, 64 | 65, 66), layer 0 of
scale 1 (n = 128, 129 | 130, 131), layer 0 of scale 2 and with it layer 1 of scale 0 at s = 4 (n = 255, 256 | 257, 260), layer 1 of
scale 0 at s = 2 (n = 127, 128 | 129, 130), besides the minimum and 33, 35, 36.
md_pool_kernel (over the pooled positions n >> k) and md_dx0_kernel (over a scale's samples n >> k) work in blocks of BLOCK = 256
positions.  BLOCK_LENGTHS puts an odd and an even length on each side of their 256 | 257 edge: md_dx0_kernel at scale 0 (n = 255, 256
| 257, 258, with EDGE_LENGTHS), the pooling into scale 1 and md_dx0_kernel there (n = 512, 513 | 514, 515), the pooling into scale 2
and md_dx0_kernel there (n = 1026, 1027 | 1028, 1029).  The same lengths put layer 1's maps at s = 2 and s = 4 on further 64-position
edges (n = 512 | 513: 256 | 257 positions at s = 2, 128 | 129 at s = 4).
Forward AND backward run every one of these lengths in both small configs.  The weight gradients' pieces are runs of about 32
positions (md_pieces), so the same lengths end their last run everywhere from 1 position to a full run; md_db_kernel strides a row in
steps of 256 positions, which the lengths above 256 cross.
The dense kernels md_fwd_kernel<8> and md_dx_kernel<8> (layers of 32 channels or more without groups) see maps of a few positions at
those lengths; test_dense_kernels_across_a_tile_edge runs them at 66 positions per row beside a short row, which takes their second
tile and the early exit of a tile that lies wholly behind a row."""
import ctypes as C
import functools

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.configs import MelGANDiscriminatorConfig
from genvox_amd.melgan_disc import MelGANDiscriminator
from tests import melgan_disc_ref64 as DR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
TILE = 64
SENTINEL = 64   # floats behind every exactly-sized buffer
CFGS = dict(TINY=DR.TINY, MIXED=DR.MIXED, DEFAULT=DR.DEFAULT)
BLOCK = 256   # positions per workgroup of md_pool_kernel and md_dx0_kernel
EDGE_LENGTHS = (33, 35, 36, 63, 64, 65, 66, 127, 128, 129, 130, 131, 255, 256, 257, 260)
BLOCK_LENGTHS = (258, 512, 513, 514, 515, 1026, 1027, 1028, 1029)
TINY_LENGTHS = (16, 32) + EDGE_LENGTHS + BLOCK_LENGTHS     # 16: the minimum of two scales
MIXED_LENGTHS = (32,) + EDGE_LENGTHS + BLOCK_LENGTHS       # 32: the minimum of three scales


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    torch.cuda.empty_cache()


def test_the_tile_size_is_the_one_the_lengths_were_chosen_for():
    header = open(__file__.replace("tests/test_melgan_disc_gpu.py", "include/genvox_amd.h")).read()
    assert f"GVX_MELGAN_DISC_TILE = {TILE}" in header


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _guarded(n_bytes):
    """A NaN-filled float32 buffer of n_bytes plus a sentinel run behind it."""
    assert n_bytes % 4 == 0
    return torch.full((n_bytes // 4 + SENTINEL,), NAN, dtype=torch.float32, device=DEV)


def _sentinel_intact(buf):
    return bool(torch.isnan(buf[-SENTINEL:]).all())


class DiscNet:
    """A handle driven through the C ABI alone."""

    def __init__(self, cfg, sd):
        self.cfg, self.lib = cfg, _lib.load()
        self.dims = _lib.gvx_melgan_disc_dims(cfg["n_scales"], cfg["base_channels"], cfg["n_layers"], cfg["s"], cfg["max_channels"], cfg["slope"])
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.weights = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
        table = (_lib.gvx_weight_desc * len(self.weights))()
        for i, (k, v) in enumerate(self.weights.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        self.blob = torch.full((self.lib.gvx_melgan_disc_blob_floats(C.byref(self.dims)),), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.lib.gvx_melgan_disc_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream()))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_melgan_disc_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_melgan_disc_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_melgan_disc_destroy(self.h)

    def layout(self, B, n):
        e = (_lib.gvx_melgan_disc_entry * 64)()
        count = self.lib.gvx_melgan_disc_layout(C.byref(self.dims), B, n, e, 64)
        per = self.cfg["n_layers"] + 3
        flat = [(e[i].byte_offset, e[i].channels, e[i].positions) for i in range(count)]
        return [flat[k * per:(k + 1) * per] for k in range(self.cfg["n_scales"])]

    def views(self, buf, B, n):
        return [[buf[off // 4: off // 4 + B * c * L].view(B, c, L) for off, c, L in scale] for scale in self.layout(B, n)]

    def forward(self, wav, lens=None):
        """-> (the features buffer, its maps as [scale][map] views)."""
        B, n = wav.shape
        fb, wb = self.lib.gvx_melgan_disc_features_bytes(C.byref(self.dims), B, n), self.lib.gvx_melgan_disc_workspace_bytes(C.byref(self.dims), B, n, 0)
        feats, ws = _guarded(fb), _guarded(wb)
        _lib.check(self.lib.gvx_melgan_disc_forward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(), fb,
                                                    ws.data_ptr(), wb, stream()))
        torch.cuda.synchronize()
        assert _sentinel_intact(feats) and _sentinel_intact(ws), "the forward wrote behind its features buffer or its workspace"
        return feats, self.views(feats, B, n)

    def cotangent_buffer(self, G, B, n, lens):
        """d_features: NaN everywhere, G (or 0 where a map has no cotangent) inside every row's own lengths."""
        fb = self.lib.gvx_melgan_disc_features_bytes(C.byref(self.dims), B, n)
        buf = _guarded(fb)
        for k, scale in enumerate(self.views(buf, B, n)):
            for i, view in enumerate(scale):
                for b in range(B):
                    L = DR.map_lengths(self.cfg, n if lens is None else lens[b])[k][i]
                    view[b, :, :L] = 0.0 if G[k][i] is None else G[k][i][b, :, :L].to(DEV, torch.float32)
        return buf

    def backward(self, wav, lens, feats, d_feats, want_params=True, want_wav=True):
        B, n = wav.shape
        grads = {k: torch.full(s, NAN, dtype=torch.float32, device=DEV) for k, s in self.shapes.items()} if want_params else {}
        table = (_lib.gvx_weight_desc * max(len(grads), 1))()
        for i, (k, g) in enumerate(grads.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), g.data_ptr(), g.numel())
        d_wav = torch.full((B, n), NAN, dtype=torch.float32, device=DEV) if want_wav else None
        wb = self.lib.gvx_melgan_disc_workspace_bytes(C.byref(self.dims), B, n, 1)
        ws = _guarded(wb)
        _lib.check(self.lib.gvx_melgan_disc_backward(self.h, wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, n, feats.data_ptr(),
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
    sd = DR.random_state(cfg, seed=11)
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
    wav = DR.random_wav(B, n, seed=100 * B + n)
    return wav, DR.reference(sd, wav, lens, cfg)


def _check_forward(name, B, n, lens=None):
    cfg, sd, net = _net(name)
    wav, ref = _forward_case(name, B, n, lens)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(_poisoned(wav, lens), lens_d)
    worst = 0.0
    for k, scale in enumerate(maps):
        for i, got in enumerate(scale):
            got = got.double().cpu()
            assert got.shape == ref["maps"][k][i].shape
            for b in range(B):
                L = DR.map_lengths(cfg, n if lens is None else lens[b])[k][i]
                assert not got[b, :, L:].any() and not torch.isnan(got[b]).any(), f"{name} {B} x {n}: map ({k}, {i}) row {b} is not exact zeros behind {L}"
                d, tol = (got[b, :, :L] - ref["maps"][k][i][b, :, :L]).abs().max().item(), ref["map_tol"][k][i]
                worst = max(worst, d / tol)
                assert d <= tol, f"{name} {B} x {n} {lens}: map ({k}, {i}) row {b}: {d:.3e} from float64, above the bound {tol:.3e} (float32 restatement {ref['map_err'][k][i]:.3e})"
    print(f"{name} {B} x {n} {lens}: largest forward error {worst:.3f} of its bound")
    return wav, ref, feats, maps


@pytest.mark.parametrize("n", TINY_LENGTHS)
def test_forward_tiny(n):
    _check_forward("TINY", 2, n)


@pytest.mark.parametrize("n", MIXED_LENGTHS)
def test_forward_mixed(n):
    _check_forward("MIXED", 2, n)


@pytest.mark.parametrize("name,lens", [("TINY", (131, 16, 77)), ("MIXED", (261, 32, 135))])
def test_forward_ragged_rows_are_their_one_row_runs(name, lens):
    cfg, _, net = _net(name)
    wav, _, _, maps = _check_forward(name, 3, lens[0], lens)
    for b, nb in enumerate(lens):
        _, alone = net.forward(wav[b:b + 1, :nb].to(DEV, torch.float32).contiguous())
        for k in range(cfg["n_scales"]):
            for i, one in enumerate(alone[k]):
                assert torch.equal(maps[k][i][b, :, :one.shape[2]], one[0]), f"{name}: row {b} of {nb} samples, map ({k}, {i}) differs from its one-row run"


def _check_backward(name, B, n, lens=None, only=None, seed=5):
    """Gradients against float64 pinned to the device's LeakyReLU decisions -> (wav, feats, d_feats, grads, largest share of a bound)."""
    cfg, sd, net = _net(name)
    wav, free, feats, maps = _check_forward(name, B, n, lens)
    flips = 0
    for k, scale in enumerate(maps):
        for i, got in enumerate(scale[:-1]):
            want = free["maps"][k][i]
            differ = (got.cpu() > 0) != (want > 0)
            flips += int(differ.sum())
            assert (want[differ].abs() <= DR.FACTOR * free["map_err"][k][i]).all(), f"map ({k}, {i}): a sign differs from float64 away from 0"
    G = DR.random_cotangents(cfg, B, n, seed, only)
    ref = DR.reference(sd, wav, lens, cfg, G, DR.masks_from_maps(maps, cfg["slope"]))
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    wav_d = _poisoned(wav, lens)
    d_feats = net.cotangent_buffer(G, B, n, lens)
    grads = net.backward(wav_d, lens_d, feats, d_feats)
    what, worst = f"{name} {B} x {n} {lens or ''} cotangents {sorted(only) if only else 'on all maps'} ({flips} LeakyReLU decisions differ)", 0.0
    for key, want in ref["grads"].items():
        g = grads[key].double().cpu()
        assert g.shape == want.shape and not torch.isnan(g).any(), f"{what}: {key} holds NaN or has the wrong shape"
        d, tol = (g - want).abs().max().item(), ref["grad_tol"][key]
        assert d <= tol, f"{what}: d {key} differs from float64 by {d:.3e}, above the bound {tol:.3e} (float32 restatement: {ref['grad_err'][key]:.3e})"
        worst = max(worst, d / tol if tol > 0.0 else 0.0)   # a bound of 0: a gradient no cotangent reaches, exact zeros on both sides
    for b in range(B):
        nb = n if lens is None else lens[b]
        assert not grads["wav"][b, nb:].any(), f"{what}: d_wav row {b} is not exact zeros behind {nb}"
    print(f"{what}: largest gradient error {worst:.3f} of its bound")
    return wav_d, lens_d, feats, d_feats, grads, worst


@pytest.mark.parametrize("name,n", [("TINY", n) for n in TINY_LENGTHS] + [("MIXED", n) for n in MIXED_LENGTHS])
def test_backward_all_cotangents(name, n):
    _check_backward(name, 2, n)


def test_dense_kernels_across_a_tile_edge():
    """MIXED at 4200 samples: 1050, 263 and 66 positions behind the three strided layers, so the dense 64 -> 64 k = 5 layer
    (md_fwd_kernel<8>, md_dx_kernel<8>) and the score (md_fwd_one_kernel) run two tiles per row at scale 0; the second row, 300
    samples, has 5 positions there, so its second tile lies wholly behind it."""
    _check_backward("MIXED", 2, 4200, (4200, 300))


@pytest.mark.parametrize("name,lens", [("TINY", (131, 16, 77)), ("MIXED", (261, 32, 135))])
def test_backward_ragged_partial_calls_and_repeats(name, lens):
    """The ragged batch; d_wav rows are their one-row runs; the dX-only and the dW-only call give the full call's bits; so does a second call."""
    cfg, sd, net = _net(name)
    wav_d, lens_d, feats, d_feats, full, _ = _check_backward(name, 3, lens[0], lens)
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
        d1 = net.cotangent_buffer([[g[b:b + 1, :, :m.shape[2]].cpu() for g, m in zip(gs, ms)] for gs, ms in zip(G_views, m1)], 1, nb, None)
        alone = net.backward(one, None, f1, d1, want_params=False)
        assert torch.equal(alone["wav"][0], full["wav"][b, :nb]), f"{name}: d_wav of row {b} differs from its one-row run"


@pytest.mark.parametrize("name,only", [("MIXED", "scores"), ("MIXED", "middle"), ("TINY", "scores"), ("TINY", "middle")])
def test_backward_single_cotangents(name, only):
    """A cotangent on the scores alone, and one on a single middle map: a dropped branch of the backward shows here."""
    cfg = CFGS[name]
    last = cfg["n_layers"] + 2
    which = {(k, last) for k in range(cfg["n_scales"])} if only == "scores" else {(1, 2)}
    _check_backward(name, 2, 130, only=frozenset(which))


def test_default_shape():
    """The default shape once, B = 2 and ragged: the dense 1024 -> 1024 layer, groups of 16 and (capped) 4 output columns."""
    _, _, _, _, _, worst = _check_backward("DEFAULT", 2, 150, (150, 97))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the module
def _module(name):
    cfg, sd, net = _net(name)
    model = MelGANDiscriminator(MelGANDiscriminatorConfig(n_scales=cfg["n_scales"], base_channels=cfg["base_channels"], n_layers=cfg["n_layers"],
                                                          downsampling_factor=cfg["s"], max_channels=cfg["max_channels"], leaky_slope=cfg["slope"]))
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    return cfg, net, model.to(DEV)


def test_module_gradients_are_the_c_abi_calls_bits():
    cfg, net, model = _module("MIXED")
    lens = (261, 32, 135)
    wav = _poisoned(DR.random_wav(3, 261, 3), lens)
    G = DR.random_cotangents(cfg, 3, 261, 8)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feats, maps = net.forward(wav, lens_d)
    want = net.backward(wav, lens_d, feats, net.cotangent_buffer(G, 3, 261, lens))
    x = wav.clone().requires_grad_(True)
    out = model(x, lens)
    assert len(out) == cfg["n_scales"] and all(len(o) == cfg["n_layers"] + 3 for o in out)
    loss = 0.0
    for k, scale in enumerate(out):
        for i, m in enumerate(scale):
            assert torch.equal(m, maps[k][i]), f"the module's map ({k}, {i}) is not the C-ABI call's"
            g = torch.zeros_like(m)
            for b, nb in enumerate(lens):
                L = DR.map_lengths(cfg, nb)[k][i]
                g[b, :, :L] = G[k][i][b, :, :L].to(DEV, torch.float32)
            loss = loss + (m * g).sum()
    loss.backward()
    assert torch.equal(x.grad, want["wav"])
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, want[k]), k
    # under no_grad, and when nothing asks for a gradient: the plain forward's bits
    with torch.no_grad():
        plain = model(wav, lens)
    for p in model.parameters():
        p.requires_grad_(False)
    frozen = model(wav, lens)
    for k in range(cfg["n_scales"]):
        for i in range(cfg["n_layers"] + 3):
            assert torch.equal(plain[k][i], maps[k][i]) and not plain[k][i].requires_grad and torch.equal(frozen[k][i], maps[k][i])
    # the generator's step: wav alone asks for a gradient; cotangents that never arrive count as zero (scores only)
    x2 = wav.clone().requires_grad_(True)
    scores_only = sum(scale[-1][b, :, :DR.map_lengths(cfg, nb)[k][-1]].sum() for k, scale in enumerate(model(x2, lens)) for b, nb in enumerate(lens))
    scores_only.backward()
    ones = [[None if i < cfg["n_layers"] + 2 else torch.ones_like(g) for i, g in enumerate(gs)] for gs in G]
    want2 = net.backward(wav, lens_d, feats, net.cotangent_buffer(ones, 3, 261, lens), want_params=False)
    assert torch.equal(x2.grad, want2["wav"]) and all(p.grad is not None and not p.requires_grad for p in model.parameters())


def test_module_refuses_short_rows_and_in_place_changes():
    cfg, net, model = _module("TINY")
    wav = DR.random_wav(2, 40, 1).to(DEV, torch.float32)
    with pytest.raises(ValueError, match="row 1"):
        model(wav, [40, 15])
    with pytest.raises(ValueError):
        model(wav[:, :15])
    out = model(wav)
    with torch.no_grad():
        model.scales[0].layers[1].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[0][-1].sum().backward()
    # a parameter that changed is packed again: the next forward sees it
    after = model(wav)
    assert not torch.equal(after[0][-1], out[0][-1]) and torch.equal(after[1][0], out[1][0])
    # the returned maps are the backward's tape: one changed in place raises too, whichever map the loss hangs on
    again = model(wav)
    with pytest.raises(RuntimeError, match="inplace"):   # torch refuses at the operation or, at the latest, at the backward
        again[1][-1].clamp_(min=0.0)
        again[0][0].sum().backward()
