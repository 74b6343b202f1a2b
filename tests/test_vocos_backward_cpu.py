"""No GPU: the host arithmetic of the Vocos training calls (include/genvox_amd.h, "Vocos generator: training") and the reference the
GPU tests lean on (tests/vocos_grad_ref64.py): the tape's formula and layout, the refusals of the size calls, the tie-free seeds, the
restatement's ISTFT gradient against a finite difference, and the unfold of gamma."""
import ctypes as C
import functools

import pytest
import torch

from genvox_amd import _lib
from genvox_amd.configs import AudioConfig, VocosConfig
from genvox_amd.vocos import VocosGenerator, dims_from_config
from tests import vocos_grad_ref64 as GR
from tests import vocos_ref64 as R

CFGS = ("NARROW", "MID", "ODD", "DEFAULT")
NEW_SYMBOLS = ("gvx_dwconv_layernorm_backward", "gvx_dwconv_layernorm_backward_workspace_bytes", "gvx_istft_head_backward",
               "gvx_istft_head_backward_workspace_bytes", "gvx_vocos_tape_bytes", "gvx_vocos_tape_layout", "gvx_vocos_backward_workspace_bytes",
               "gvx_vocos_forward_train", "gvx_vocos_backward", "gvx_vocos_backward_stage_times_ms")


def _dims(cfg):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = cfg["hop_length"], cfg["n_mels"]
    return dims_from_config(VocosConfig(**R.model_kwargs(cfg)), ac)


def test_the_new_symbols_exist():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", CFGS)
def test_tape_bytes_is_the_headers_formula_and_the_layout_agrees(name):
    cfg, lib = getattr(R, name), _lib.load()
    d = _dims(cfg)
    Cp = (cfg["n_mels"] + 3) // 4 * 4
    dim, I, L, N = cfg["dim"], cfg["intermediate_dim"], cfg["num_layers"], cfg["n_fft"]
    least = 2 if cfg["padding"] == "center" else 1
    for B, T in ((1, least), (2, 17), (3, 515), (32, 800)):
        want = 4 * B * ((T + 6) * Cp + T * ((L + 2) * dim + L * I + N + 2))
        assert lib.gvx_vocos_tape_bytes(C.byref(d), B, T) == want
        n = lib.gvx_vocos_tape_layout(C.byref(d), B, T, None, 0)
        assert n == 3 + 2 * L + 1
        entries = (_lib.gvx_vocos_tape_entry * n)()
        assert lib.gvx_vocos_tape_layout(C.byref(d), B, T, entries, n) == n
        shapes = [(T + 6, Cp), (T, dim), (T, dim)] + [(T, I), (T, dim)] * L + [(T, N + 2)]
        at = 0
        for e, (rows, ch) in zip(entries, shapes):
            assert (e.byte_offset, e.rows, e.channels) == (at, rows, ch)
            assert at % 16 == 0
            at += 4 * B * rows * ch
        assert at == want
        ws = lib.gvx_vocos_backward_workspace_bytes(C.byref(d), B, T)
        assert ws > 0 and ws % 256 == 0
    if name == "DEFAULT":   # the header's per-frame figure
        per_frame = (lib.gvx_vocos_tape_bytes(C.byref(d), 1, 101) - lib.gvx_vocos_tape_bytes(C.byref(d), 1, 100))
        assert per_frame == 74136


def test_size_calls_return_zero_for_refused_shapes():
    lib = _lib.load()
    d = _dims(R.MID)
    for fn in (lib.gvx_vocos_tape_bytes, lib.gvx_vocos_backward_workspace_bytes):
        assert fn(C.byref(d), 0, 5) == 0 and fn(C.byref(d), 1, 0) == 0 and fn(C.byref(d), 65536, 5) == 0 and fn(C.byref(d), 1, (1 << 20) + 1) == 0
        assert fn(C.byref(d), 1, 1) == 0 and fn(C.byref(d), 1, 2) > 0          # "center": a row needs 2 frames
        bad = _dims(R.MID)
        bad.dim = 48
        assert fn(C.byref(bad), 1, 5) == 0
        assert fn(None, 1, 5) == 0
    assert lib.gvx_vocos_tape_layout(C.byref(d), 0, 5, None, 0) == 0 and lib.gvx_vocos_tape_layout(C.byref(d), 1, 1, None, 0) == 0
    same = _dims(R.NARROW)
    assert lib.gvx_vocos_tape_bytes(C.byref(same), 1, 1) > 0                    # "same": 1 frame is a row
    f = lib.gvx_dwconv_layernorm_backward_workspace_bytes
    assert f(0, 5, 32, 7) == 0 and f(1, 0, 32, 7) == 0 and f(1, 5, 30, 7) == 0 and f(1, 5, 516, 7) == 0 and f(1, 5, 32, 5) == 0
    assert f(2, 129, 32, 7) == 2 * 2 * 10 * 32 * 4 + 2 * 129 * 32 * 4 and f(2, 129, 32, 0) == 2 * 2 * 10 * 32 * 4
    g = lib.gvx_istft_head_backward_workspace_bytes
    assert g(0, 5, 512, 128) == 0 and g(1, 0, 512, 128) == 0 and g(1, 5, 500, 128) == 0 and g(1, 5, 512, 32) == 0 and g(1, 5, 512, 129) == 0
    assert g(2, 5, 512, 128) == 2 * 5 * 128 * 4 + (8 * 513 + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def _ref(name):
    cfg = getattr(R, name)
    ref = R.Generator(cfg, seed=11)
    ref.load_state_dict({k: v.float().double() for k, v in ref.state_dict().items()})
    return cfg, ref


@pytest.mark.parametrize("name,B,T,lens", [
    ("NARROW", 1, 1, None), ("NARROW", 2, 17, None), ("NARROW", 3, 19, (19, 1, 16)),
    ("MID", 1, 2, None), ("MID", 2, 17, None), ("MID", 3, 33, (33, 2, 17)),
    ("ODD", 2, 9, None), ("ODD", 3, 17, (17, 1, 6)),
    ("DEFAULT", 1, 18, None), ("DEFAULT", 3, 17, (17, 2, 9))])
def test_the_gpu_cases_have_a_tie_free_seed(name, B, T, lens):
    """The cases of tests/test_vocos_backward_gpu.py::test_gradients_tie_free: a mel seed in 1..8 puts no log-magnitude within the margin
    of ln 100, and both branches of the clip are exercised."""
    cfg, ref = _ref(name)
    seed, mel, G, want = GR.tie_free_case(ref, cfg, B, T, lens, G_seed=1000 * B + T)
    share = GR.clamped_share(want, lens, cfg)
    print(f"{name} {B} x {T} {lens}: seed {seed}, {100 * share:.1f} % clamped, margin {GR.clamp_margin(want):.2e}")
    assert 1 <= seed <= 8 and GR.near_ties(want, lens, cfg) == 0
    assert 0.05 < share < 0.5


def test_the_piece_edge_case_has_no_tie_free_seed_and_is_pinned():
    """NARROW 3 x 515: 2 x 10^5 magnitudes - every seed in 1..8 has a near-tie, which is why the GPU test pins the clamp."""
    cfg, ref = _ref("NARROW")
    with pytest.raises(AssertionError, match="tie-free"):
        GR.tie_free_case(ref, cfg, 3, 515, (515, 1, 257), G_seed=1)


def test_the_restatements_istft_gradient_against_a_finite_difference():
    """2 frames of n_fft 512, hop 128, "same": central differences in float64, on the smooth side and on the clamped side of ln 100."""
    n_fft, hop, H = 512, 128, 256
    g = torch.Generator().manual_seed(3)
    c = torch.randn(1, 2, n_fft + 2, generator=g, dtype=torch.float64)
    c[..., :H + 1] = 2.3 + 3.0 * c[..., :H + 1]
    m = c[..., :H + 1]
    near = (m - R.LOG_CLAMP).abs() < 1e-3
    m[near] = R.LOG_CLAMP - 0.01
    G = torch.randn(1, 2 * hop, generator=g, dtype=torch.float64)
    for padding in ("same", "center"):   # the reference's forward IS the project's definition: the trim and the division commute
        assert torch.equal(GR.istft(c, n_fft, hop, padding), R.istft(c, n_fft, hop, padding))
        assert torch.equal(GR.istft(c.float(), n_fft, hop, padding), R.istft(c.float(), n_fft, hop, padding))
    f = lambda v: (GR.istft(v, n_fft, hop, "same") * G).sum()
    leaf = c.clone().requires_grad_(True)
    f(leaf).backward()
    keep = (m <= R.LOG_CLAMP)
    leaf2 = c.clone().requires_grad_(True)
    (GR.istft(leaf2, n_fft, hop, "same", keep) * G).sum().backward()
    assert torch.equal(leaf.grad, leaf2.grad)          # the pinned form with float64's own decisions is the plain one
    assert not leaf.grad[..., :H + 1][~keep].any()     # clamped bins: no gradient to m
    h = 1e-6
    idx = torch.randperm(c.numel(), generator=g)[:60]
    for i in idx.tolist():
        d = torch.zeros_like(c).view(-1)
        d[i] = h
        fd = (f(c + d.view_as(c)) - f(c - d.view_as(c))).item() / (2 * h)
        assert abs(fd - leaf.grad.view(-1)[i].item()) <= 1e-5 * max(1.0, abs(fd)), i   # rounding of f over 2 h


def test_the_unfold_of_gamma_equals_autograd_with_a_zero_gamma():
    g = torch.Generator().manual_seed(5)
    Cn, I, rows = 12, 20, 9
    gamma = torch.randn(Cn, generator=g, dtype=torch.float64)
    gamma[3] = 0.0
    w2 = torch.randn(Cn, I, generator=g, dtype=torch.float64)
    b2 = torch.randn(Cn, generator=g, dtype=torch.float64)
    h = torch.randn(rows, I, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, Cn, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (gamma, w2, b2)]
    ((leaves[0] * torch.nn.functional.linear(h, leaves[1], leaves[2])) * dy).sum().backward()
    dw2f, db2f = dy.t() @ h, dy.sum(0)                  # what the kernels produce: gradients w.r.t. the folded tensors
    dw2, db2, dgamma = GR.unfold_gamma(dw2f, db2f, gamma, w2, b2)
    for got, leaf in zip((dgamma, dw2, db2), leaves):
        assert torch.allclose(got, leaf.grad, rtol=1e-12, atol=1e-12)
    assert leaves[0].grad[3].abs().item() > 0.0 and not dw2[3].any()


def test_trainable_is_opt_in_and_off_by_default():
    cfg = R.NARROW
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = cfg["hop_length"], cfg["n_mels"]
    model = VocosGenerator(VocosConfig(**R.model_kwargs(cfg)), ac)
    assert model.trainable is False
    mel = torch.zeros(1, cfg["n_mels"], 4)
    with pytest.raises(NotImplementedError, match="backward.*trainable=True"):
        model.vocode_with_grad(mel)
    assert VocosGenerator(VocosConfig(**R.model_kwargs(cfg)), ac, trainable=True).trainable is True
