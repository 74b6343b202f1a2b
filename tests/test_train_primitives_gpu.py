"""GPU: the small training kernels of genvox_amd/csrc/train_ops.hip (and the criterion / mask kernels of misc.hip) that
genvox_amd/training.py strings together, each against its plain definition in float64 (or exactly, where the kernel moves or
selects values), at the sizes where their loops change shape: chunk and pass boundaries of the embedding gradient, the
two-stride loop of the squared norm, grid-stride tails.  Regions a kernel must not read hold NaN, regions it must not write a
sentinel bit pattern that has to survive.  The library is built with -ffp-contract=off: a * b + c in a kernel is two roundings."""
import math

import numpy as np
import pytest
import torch

from genvox_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 0x5A5A5A5A
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _guarded(n, guard=64, dtype=torch.float32):
    """A device buffer of n elements followed by `guard` more, all holding the sentinel (as 32-bit words; bytes for uint8)."""
    if dtype == torch.uint8:
        return torch.full((n + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    words = (n + guard) * (2 if dtype == torch.float64 else 1)
    return torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda").view(dtype)


def _untouched(buf, n):
    tail = buf[n:]
    return bool((tail == 0x5A).all()) if buf.dtype == torch.uint8 else bool((tail.view(torch.int32) == SENTINEL).all())


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 1000])
@pytest.mark.parametrize("cols", [1, 8, 33, 80, 513])
def test_transpose(lib, rows, cols):
    src = torch.randn(rows, cols, generator=_gen(rows + cols)).cuda()
    for rows_p in sorted({rows, rows + 1, (rows + 31) // 32 * 32, (rows + 63) // 64 * 64}):
        dst = _guarded(cols * rows_p)
        assert lib.gvx_train_transpose(src.data_ptr(), cols, dst.data_ptr(), rows, cols, rows_p, _stream()) == 0
        got = dst[:cols * rows_p].view(cols, rows_p)
        assert torch.equal(got[:, :rows], src.t()) and bool((got[:, rows:] == 0).all()), (rows, cols, rows_p)
        assert not bool(torch.signbit(got[:, rows:]).any()) and _untouched(dst, cols * rows_p), (rows, cols, rows_p)
    dst = _guarded(cols * rows)
    assert lib.gvx_train_transpose(src.data_ptr(), cols + 1, dst.data_ptr(), rows, cols, rows, _stream()) != 0   # dense sources only
    assert lib.gvx_train_transpose(src.data_ptr(), cols, dst.data_ptr(), rows, cols, rows - 1, _stream()) != 0
    torch.cuda.synchronize()
    assert _untouched(dst, 0)


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 127, 128, 129, 6400])
@pytest.mark.parametrize("Cc", [1, 31, 32, 33, 4096])
def test_colsum(lib, rows, Cc):
    """Sums in double: within one fp32 ulp of the float64 column sum (plus 1e-12 of sum |x| for the order of the double adds),
    on plain data and on columns that cancel to ~1e-7 of their terms."""
    g = _gen(rows * 3 + Cc)
    plain = torch.randn(rows, Cc, generator=g) * 10.0 ** (3 * torch.rand(rows, Cc, generator=g))
    cancel = plain.clone()
    if rows > 1:
        cancel[rows // 2:rows // 2 * 2] = -cancel[:rows // 2] * (1 + 2.0 ** -20)
    worst = 0.0
    for x in (plain, cancel):
        out = _guarded(Cc)
        assert lib.gvx_train_colsum(x.cuda().data_ptr(), rows, Cc, out.data_ptr(), _stream()) == 0
        want, mag = x.double().sum(0), x.double().abs().sum(0)
        err = (out[:Cc].cpu().double() - want).abs()
        tol = 2.0 ** -23 * want.abs() + 1e-12 * mag + 1e-45
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all()) and _untouched(out, Cc), (rows, Cc, worst)


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 33), (200, 512), (5000, 257)])
def test_axpby(lib, rows, cols):
    """y = fl(fl(alpha a) + fl(beta b)) exactly (no contraction to fma in this build), three different leading dimensions, padding
    of a and b NaN, padding of y untouched; b = NULL; y aliasing a."""
    g = _gen(rows + cols)
    lda, ldb, ldy = cols + 3, cols + 1, cols + 2
    alpha, beta = torch.tensor(0.3), torch.tensor(-1.7)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g) * 100
    ab, bb = torch.full((rows, lda), NAN), torch.full((rows, ldb), NAN)
    ab[:, :cols], bb[:, :cols] = a, b
    ab, bb = ab.cuda(), bb.cuda()
    for with_b in (True, False):
        y = _guarded(rows * ldy)
        assert lib.gvx_train_axpby(ab.data_ptr(), lda, alpha.item(), bb.data_ptr() if with_b else None, ldb, beta.item(), y.data_ptr(), ldy,
                                   rows, cols, _stream()) == 0
        want = alpha * a + beta * b if with_b else alpha * a     # float32 tensor arithmetic: one rounding per operation
        got = y[:rows * ldy].view(rows, ldy)
        assert torch.equal(got[:, :cols].cpu(), want), (rows, cols, with_b)
        assert bool((got[:, cols:].view(torch.int32) == SENTINEL).all()) and _untouched(y, rows * ldy)
    y = ab.clone()   # in place: y is a
    assert lib.gvx_train_axpby(y.data_ptr(), lda, alpha.item(), bb.data_ptr(), ldb, beta.item(), y.data_ptr(), lda, rows, cols, _stream()) == 0
    assert torch.equal(y[:, :cols].cpu(), alpha * a + beta * b) and bool(torch.isnan(y[:, cols:]).all())


@pytest.mark.parametrize("n", [1, 255, 257, 3_000_001])
def test_relu_dropout_backward(lib, n):
    """dz = dy * scale where the unit was kept and its output positive, else exactly +0.0 - whatever dy holds there (NaN);
    +0.0, -0.0 and negative outputs are all inactive.  The last size runs the grid-stride loop (4096 workgroups of 256)."""
    g = _gen(n)
    dy = torch.randn(n, generator=g)
    act = torch.randn(n, generator=g)
    sel = torch.randint(0, 5, (n,), generator=g)
    act[sel == 0], act[sel == 1] = 0.0, -0.0
    keep = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
    live = (keep != 0) & (act > 0)
    dy[~live] = NAN
    scale = torch.tensor(2.0 / 3.0)
    dz = _guarded(n)
    assert lib.gvx_train_relu_dropout_backward(dy.cuda().data_ptr(), act.cuda().data_ptr(), keep.cuda().data_ptr(), scale.item(), n,
                                               dz.data_ptr(), _stream()) == 0
    want = torch.where(live, dy * scale, torch.zeros(()))
    got = dz[:n].cpu()
    assert torch.equal(got, want) and not bool(torch.signbit(got[~live]).any()) and _untouched(dz, n)


@pytest.mark.parametrize("B", [1, 5, 32])
@pytest.mark.parametrize("K", [8, 80, 1536])
@pytest.mark.parametrize("n_slots", [1, 3, 201])
def test_unblock(lib, B, K, n_slots):
    """[slot][K / 8][B][8] -> [slot][B][K]: an exact permutation."""
    n = n_slots * B * K
    src = torch.arange(n, dtype=torch.float32).cuda() + 0.5
    dst = _guarded(n)
    assert lib.gvx_train_unblock(src.data_ptr(), dst.data_ptr(), n_slots, B, K, _stream()) == 0
    want = src.view(n_slots, K // 8, B, 8).permute(0, 2, 1, 3).reshape(n_slots, B, K)
    assert torch.equal(dst[:n].view(n_slots, B, K), want) and _untouched(dst, n)
    assert lib.gvx_train_unblock(src.data_ptr(), dst.data_ptr(), n_slots, B, K + 4, _stream()) != 0
    assert lib.gvx_train_unblock(src.data_ptr(), dst.data_ptr(), n_slots, B, 4, _stream()) != 0


@pytest.mark.parametrize("n_tok", [1, 255, 256, 257, 8191, 8192, 8193, 20000])
@pytest.mark.parametrize("E", [1, 8, 512, 1024, 1025, 1300])
def test_embedding_backward(lib, n_tok, E):
    """d embedding[row] = sum of dx over the positions that hold the row's token, "added in position order": bit-equal to a
    float32 sum taken in that order on the host, and within count * 2^-24 * sum |dx| of float64.  Positions cross the chunks of
    8192, channels the passes of 1024; rows 2 and 6 are used by no token and come back as zeros from a NaN-filled table; a second
    run puts the same token at every position (the compacted list fills a whole chunk)."""
    n_rows = 7
    g = _gen(n_tok * 7 + E)
    dx = torch.randn(n_tok, E, generator=g) * 10.0 ** (2 * torch.rand(n_tok, 1, generator=g))
    used = torch.tensor([0, 1, 3, 4, 5])
    for tokens in (used[torch.randint(0, 5, (n_tok,), generator=g)], torch.full((n_tok,), 4)):
        demb = torch.full((n_rows * E + 64,), NAN).cuda()
        demb[n_rows * E:] = 12345.0
        assert lib.gvx_train_embedding_backward(tokens.cuda().data_ptr(), dx.cuda().data_ptr(), n_tok, E, n_rows, demb.data_ptr(), _stream()) == 0
        got = demb[:n_rows * E].view(n_rows, E).cpu()
        assert bool((demb[n_rows * E:] == 12345.0).all())
        want32 = np.zeros((n_rows, E), dtype=np.float32)
        dxn, tk = dx.numpy(), tokens.numpy()
        for i in range(n_tok):
            want32[tk[i]] += dxn[i]
        assert np.array_equal(got.numpy(), want32), (n_tok, E, int((got.numpy() != want32).sum()))
        want64 = torch.zeros(n_rows, E, dtype=torch.float64).index_add_(0, tokens, dx.double())
        mag = torch.zeros(n_rows, E, dtype=torch.float64).index_add_(0, tokens, dx.double().abs())
        count = torch.bincount(tokens, minlength=n_rows).double()[:, None]
        assert bool(((got.double() - want64).abs() <= count * U * mag).all())
        assert bool((got[2] == 0).all()) and bool((got[6] == 0).all())


def _refs(entries):
    """A device array of structs of 64-bit fields (gvx_tensor_ref / gvx_adam_ref) from rows of integers."""
    return torch.from_numpy(np.array(entries, dtype=np.int64).reshape(-1)).cuda()


SQN_SIZES = [1, 255, 256, 257, 16383, 16384, 16385, 32768, 32769]


@pytest.mark.parametrize("n_tensors", [1, 10, 48, 300])
def test_sqnorm_many(lib, n_tensors):
    """The sum of squares of many tensors in one call (sizes around the 16 384-element stride of the two-stride loop and its
    tail; 10 tensors: all the sizes and one of 1 000 003), magnitudes from 1e-20 to 1e15: 1e-12 of float64, two calls the same
    bits, nothing written behind gvx_train_sqnorm_scratch_bytes."""
    g = _gen(n_tensors)
    sizes = [SQN_SIZES[(i + n_tensors) % len(SQN_SIZES)] for i in range(n_tensors)]
    if n_tensors == 10:
        sizes = SQN_SIZES + [1_000_003]
    tensors = [(torch.randn(n, generator=g) * 10.0 ** (35 * torch.rand(n, generator=g) - 20)).cuda() for n in sizes]
    refs = _refs([(t.data_ptr(), t.numel()) for t in tensors])
    nbytes = lib.gvx_train_sqnorm_scratch_bytes(n_tensors)
    assert nbytes == 64 * 8 * n_tensors
    scratch, out = _guarded(nbytes // 8, dtype=torch.float64), _guarded(1, dtype=torch.float64)
    assert lib.gvx_train_sqnorm_many(refs.data_ptr(), n_tensors, scratch.data_ptr(), out.data_ptr(), _stream()) == 0
    first = out[:1].clone()
    want = math.fsum(float((t.double() ** 2).sum()) for t in tensors)
    rel = abs(float(first) - want) / want
    assert rel <= 1e-12, (n_tensors, rel)
    assert _untouched(scratch, nbytes // 8) and _untouched(out, 1)
    out[:1] = 0
    assert lib.gvx_train_sqnorm_many(refs.data_ptr(), n_tensors, scratch.data_ptr(), out.data_ptr(), _stream()) == 0
    assert torch.equal(out[:1], first)
    print(f"sqnorm {n_tensors} tensors: relative error {rel:.2e}")


@pytest.mark.parametrize("weight_decay,grad_scale", [(0.0, 1.0), (1e-6, 0.37)])
def test_adam_step_many(lib, weight_decay, grad_scale):
    """Against torch.optim.Adam in float64 on the CPU at steps 1, 2, 3 and 1000 (the bias corrections), several tensors per
    launch with sizes around the 32 768 elements one grid pass covers, one tensor with zero gradients (0 / (0 + eps)).

    Every step is checked on its own: the reference starts from the kernel's fp32 state and is given the fp32 values of the
    hyper-parameters (the kernel forms 1 - beta in fp32 from them), so only the rounding of one update is left.  With u = 2^-24,
    G = |g s| + |wd p| and the kernel's operation order:
      g' = fl(fl(g s) + fl(wd p))                                   |dg'| <= 3u G
      m' = fl(fl(b1 m) + fl((1 - b1) g'))                            |dm'| <= 8u (b1 |m| + (1 - b1) G)
      v' = fl(fl(b2 v) + fl(fl((1 - b2) g') g'))                     |dv'| <= 12u (b2 v + (1 - b2) G^2)
      p' = fl(p - fl(fl(fl(lr / bc1) m') / fl(fl(sqrt(v') / bc2) + eps)))
    The update q = c m' / D, D = sqrt(v') / bc2 + eps, moves by |c| (|dm'| / D + |m'| dD / D^2) with dD <= |dv'| / (2 sqrt(v') bc2)
    + 4u D, plus 8u |q| for its own five roundings and the fp32 bias corrections, and p' adds one rounding of its own (2u |p| allowed)."""
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    lr, eps, wd, gs = float(np.float32(1e-3)), float(np.float32(1e-8)), float(np.float32(weight_decay)), float(np.float32(grad_scale))
    g = _gen(int(grad_scale * 100))
    sizes = [1, 32767, 32768, 32769, 100003, 4097]
    guard = 64
    P = [torch.cat([torch.randn(n, generator=g), torch.full((guard,), 7.0)]).cuda() for n in sizes]
    M_ = [torch.cat([torch.zeros(n), torch.full((guard,), 7.0)]).cuda() for n in sizes]
    V_ = [torch.cat([torch.zeros(n), torch.full((guard,), 7.0)]).cuda() for n in sizes]
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 3, 1000):
        grads = [torch.randn(n, generator=g) * 10.0 ** (4 * torch.rand(n, generator=g) - 3) for n in sizes]
        grads[-1].zero_()
        G_ = [torch.cat([gr, torch.full((guard,), NAN)]).cuda() for gr in grads]
        params = [torch.nn.Parameter(p[:n].cpu().double()) for p, n in zip(P, sizes)]
        opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        old = [(p[:n].cpu().double(), m[:n].cpu().double(), v[:n].cpu().double()) for p, m, v, n in zip(P, M_, V_, sizes)]
        for p, gr, (_, m0, v0) in zip(params, grads, old):
            p.grad = gr.double() * gs
            opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        opt.step()
        refs = _refs([(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n) for p, gr, m, v, n in zip(P, G_, M_, V_, sizes)])
        assert lib.gvx_train_adam_step_many(refs.data_ptr(), len(sizes), gs, lr, wd, b1, b2, eps, step, _stream()) == 0
        bc1, bc2 = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
        for i, (p, n) in enumerate(zip(params, sizes)):
            p0, m0, v0 = old[i]
            st = opt.state[p]
            Gm = (grads[i].double() * gs).abs() + wd * p0.abs()
            tol_m = 8 * U * (b1 * m0.abs() + (1 - b1) * Gm)
            tol_v = 12 * U * (b2 * v0 + (1 - b2) * Gm * Gm)
            root = st["exp_avg_sq"].sqrt()
            D = root / bc2 + eps
            dD = torch.where(root > 0, tol_v / (2 * root.clamp_min(1e-300) * bc2), torch.zeros_like(root)) + 4 * U * D
            q = (lr / bc1) * st["exp_avg"] / D
            tol_p = (lr / bc1) * (tol_m / D + st["exp_avg"].abs() * dD / (D * D)) + 8 * U * q.abs() + 2 * U * p.data.abs()
            for j, (got, want, tol) in enumerate(((P[i], p.data, tol_p), (M_[i], st["exp_avg"], tol_m), (V_[i], st["exp_avg_sq"], tol_v))):
                err = (got[:n].cpu().double() - want).abs()
                ratio = float((err / tol.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
                worst[j] = max(worst[j], ratio)
                assert ratio <= 1.0, (step, sizes[i], "p m v"[2 * j], ratio)
                assert bool((got[n:] == 7.0).all()), (step, sizes[i], "elements behind numel written")
        if wd == 0.0:
            assert torch.equal(P[-1][:sizes[-1]].cpu().double(), old[-1][0])   # zero gradients, no decay: 0 / (0 + eps) leaves p alone
    print(f"adam wd={weight_decay} scale={grad_scale}: error / bound p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


@pytest.mark.parametrize("B,n_mels,T", [(1, 1, 1), (3, 80, 7), (5, 8, 1000), (32, 80, 800)])
def test_tacotron2_loss_and_backward(lib, B, n_mels, T):
    """MSE + MSE + BCE-with-logits and its gradient against float64, gate logits of +-1e3 (what gvx_mask_padding writes) with
    targets 0 and 1 among them: finite, and the stable form's value."""
    g = _gen(B * T + n_mels)
    mel, post, mel_t = (torch.randn(B, n_mels, T, generator=g) * 3 for _ in range(3))
    gate = torch.randn(B, T, generator=g) * 4
    gate_t = (torch.rand(B, T, generator=g) < 0.3).float()
    flat = gate.view(-1)
    flat[::3] = torch.tensor([1e3, -1e3, 1e3, -1e3])[torch.arange(flat[::3].numel()) % 4]
    gate_t.view(-1)[::6] = 1.0
    dev = [x.cuda() for x in (mel, post, gate, mel_t, gate_t)]
    out = _guarded(3)
    scratch = torch.empty(6144, dtype=torch.uint8, device="cuda")
    assert lib.gvx_tacotron2_loss(*(x.data_ptr() for x in dev), B, n_mels, T, out.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()) == 0
    x, y = gate.double(), gate_t.double()
    bce = x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))
    mel_loss = ((mel.double() - mel_t.double()) ** 2).mean() + ((post.double() - mel_t.double()) ** 2).mean()
    gate_loss = bce.mean()
    got = out[:3].cpu().double()
    assert bool(torch.isfinite(got).all()) and _untouched(out, 3)
    # (a - t)^2 in fp32 is three roundings per term, the sums are double, the means round once more
    tol_gate = 8 * U * float((x.abs() + (x * y).abs() + 1).mean())
    assert abs(float(got[1] - mel_loss)) <= 8 * U * float(mel_loss), (float(got[1]), float(mel_loss))
    assert abs(float(got[2] - gate_loss)) <= tol_gate, (float(got[2]), float(gate_loss))
    assert abs(float(got[0] - (mel_loss + gate_loss))) <= 8 * U * float(mel_loss) + tol_gate + U * float(mel_loss + gate_loss)
    n_mel, n_gate = B * n_mels * T, B * T
    d = [_guarded(n_mel), _guarded(n_mel), _guarded(n_gate)]
    assert lib.gvx_tacotron2_loss_backward(*(x.data_ptr() for x in dev), B, n_mels, T, *(t.data_ptr() for t in d), _stream()) == 0
    for got_d, src in ((d[0], mel), (d[1], post)):
        want = 2.0 / n_mel * (src.double() - mel_t.double()).view(-1)
        assert bool(((got_d[:n_mel].cpu().double() - want).abs() <= 4 * U * want.abs()).all()) and _untouched(got_d, n_mel)
    want = (torch.sigmoid(x) - y).view(-1) / n_gate
    gd = d[2][:n_gate].cpu().double()
    assert bool(torch.isfinite(gd).all()) and bool(((gd - want).abs() <= 8 * U / n_gate).all()) and _untouched(d[2], n_gate)
    sat = flat.abs() == 1e3      # saturated logits: the sigmoid is exactly 0 or 1, the gradient exactly 0 or +-fl(1 / n_gate)
    assert torch.equal(gd[sat], (torch.sigmoid(x) - y).view(-1)[sat] * float(np.float32(1.0) / np.float32(n_gate)))


@pytest.mark.parametrize("B,n_mels,T", [(1, 1, 1), (4, 80, 37), (3, 8, 1000)])
def test_mask_padding(lib, B, n_mels, T):
    """Frames at or past a row's length: mel and mel_post exactly 0, gate exactly 1e3; live frames bit-unchanged; lengths 0,
    T - 1, T and beyond; each of the three tensors may be NULL (include/genvox_amd.h says so) and is then skipped."""
    g = _gen(B + T)
    lens = [0, T - 1, T, T + 5][:B] if B > 1 else [0]
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    src = [torch.randn(B, n_mels, T, generator=g), torch.randn(B, n_mels, T, generator=g), torch.randn(B, T, generator=g)]
    t_idx = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]          # [B, T] True where masked
    want = [torch.where(t_idx[:, None, :], torch.zeros(()), src[0]), torch.where(t_idx[:, None, :], torch.zeros(()), src[1]),
            torch.where(t_idx, torch.tensor(1e3), src[2])]
    for skip in (None, 0, 1, 2):
        bufs = [_guarded(s.numel()) for s in src]
        for b_, s in zip(bufs, src):
            b_[:s.numel()] = s.view(-1).cuda()
        ptrs = [None if i == skip else b_.data_ptr() for i, b_ in enumerate(bufs)]
        assert lib.gvx_mask_padding(*ptrs, lens_d.data_ptr(), B, n_mels, T, _stream()) == 0
        for i, (b_, s, w) in enumerate(zip(bufs, src, want)):
            expect = s if i == skip else w
            assert torch.equal(b_[:s.numel()].cpu().view(torch.int32), expect.reshape(-1).view(torch.int32)), (skip, i)
            assert _untouched(b_, s.numel())
    assert lib.gvx_mask_padding(None, None, None, None, B, n_mels, T, _stream()) != 0


def test_prenet_masks_generate(lib):
    """Bytes are 0 or 1, a seed fixes them, another seed gives others, the mean over 2^22 bytes is within five standard errors
    of one half, a length that is no multiple of 8 (or of a workgroup's 2048 bytes) leaves the bytes behind it alone."""
    n = 1 << 22
    a, b, c = _guarded(n, dtype=torch.uint8), _guarded(n, dtype=torch.uint8), _guarded(n, dtype=torch.uint8)
    assert lib.gvx_prenet_masks_generate(a.data_ptr(), n, 11, _stream()) == 0
    assert lib.gvx_prenet_masks_generate(b.data_ptr(), n, 11, _stream()) == 0
    assert lib.gvx_prenet_masks_generate(c.data_ptr(), n, 12, _stream()) == 0
    assert int(a[:n].max()) == 1 and int(a[:n].min()) == 0 and torch.equal(a, b) and _untouched(a, n)
    assert abs(float(a[:n].float().mean()) - 0.5) <= 5 * 0.5 / math.sqrt(n)
    assert abs(float((a[:n] == c[:n]).float().mean()) - 0.5) <= 0.01     # another seed: other bytes, half of them equal by chance
    for m in (1, 7, 8, 9, 2047, 100003):
        d = _guarded(m, dtype=torch.uint8)
        assert lib.gvx_prenet_masks_generate(d.data_ptr(), m, 11, _stream()) == 0
        assert torch.equal(d[:m], a[:m]) and _untouched(d, m), m            # a prefix of the same stream
    assert lib.gvx_prenet_masks_generate(None, 8, 1, _stream()) != 0


def test_conv_bn_train_forward_large_offset_small_spread(lib):
    """Batch statistics where the mean dwarfs the spread: inputs 1024 + k / 64 and small integer weights make every convolution
    output exact in fp32 (values near 1e3, standard deviation ~0.05), so what is left is BatchNorm itself - the two-pass variance
    in double.  Output against float64 batch normalisation, within the rounding of the fp32 mean and inverse deviation the
    kernel stores; running_mean / running_var against torch's update in float64."""
    B, Cin, Cout, T, k = 4, 8, 16, 50, 3
    g = _gen(5)
    x = 1024.0 + torch.randint(-2, 3, (B, Cin, T), generator=g).float() / 64.0
    w = torch.randint(-1, 2, (Cout, Cin, k), generator=g).float()
    w[:, 0, :] += torch.tensor([0.0, 1.0, 0.0]) - w.sum(1)   # the middle tap sums to 1 over the channels, the outer taps to 0: outputs
                                                             # near 1024 at the sequence edges too; partial sums stay below 2^16
    bias = torch.randint(-3, 4, (Cout,), generator=g).float()
    gamma, beta = 1.0 + 0.2 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    rm, rv = torch.randn(Cout, generator=g), 1.0 + torch.rand(Cout, generator=g)
    z = torch.nn.functional.conv1d(x.double(), w.double(), bias.double(), padding=1)
    assert torch.equal(z.float().double(), z)        # exact in fp32, as claimed
    rm64, rv64 = rm.double(), rv.double()
    want = torch.nn.functional.batch_norm(z, rm64, rv64, gamma.double(), beta.double(), training=True, momentum=0.1, eps=1e-5)
    mean = z.mean((0, 2))
    invstd = 1.0 / torch.sqrt(z.var((0, 2), unbiased=False) + 1e-5)
    saved = torch.empty(lib.gvx_conv_train_saved_bytes(B, Cin, Cout, T, k), dtype=torch.uint8, device="cuda")
    ws = torch.empty(lib.gvx_conv_train_workspace_bytes(B, Cin, Cout, T, k), dtype=torch.uint8, device="cuda")
    y = _guarded(B * Cout * T)
    dev = [t.cuda() for t in (x, w, bias, gamma, beta, rm, rv)]
    assert lib.gvx_conv_bn_act_train_forward(*(t.data_ptr() for t in dev), B, Cin, Cout, T, k, 0, None, 0.0, y.data_ptr(), saved.data_ptr(),
                                             saved.numel(), ws.data_ptr(), ws.numel(), _stream()) == 0
    got = y[:B * Cout * T].view(B, Cout, T).cpu().double()
    # xhat = fl(fl(z - fl(mean)) * fl(invstd)): the fp32 mean is off by u |mean|, the rest is a few relative roundings
    sc = (gamma.double().abs() * invstd)[None, :, None]
    tol = 2 * sc * U * mean.abs()[None, :, None] + 8 * U * (want.abs() + beta.double().abs()[None, :, None] + sc * (z - mean[None, :, None]).abs())
    ratio = float(((got - want).abs() / tol).max())
    assert ratio <= 1.0 and _untouched(y, B * Cout * T), ratio
    assert bool(((dev[5].cpu().double() - rm64).abs() <= 4 * U * (rm64.abs() + 0.1 * mean.abs())).all())
    assert bool(((dev[6].cpu().double() - rv64).abs() <= 4 * U * rv64.abs() + 1e-6 * 0.1 * z.var((0, 2))).all())
    print(f"conv + batch norm, offset 1e3: error / bound {ratio:.3f}")
