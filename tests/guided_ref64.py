"""The diagonal guided attention loss as plain float64 torch, and the training step with it, differentiated by autograd: what
tests/test_guided_attention_cpu.py works by hand and tests/test_guided_attention_gpu.py holds gvx_guided_attention_loss,
gvx_train_decoder_bptt_ext and ``Tacotron2.train_step`` under ``Tacotron2GuidedLoss`` to.

Written from the formula (Tachibana et al. 2017, section 4.1; the masked mean of ESPnet's Tacotron2 recipe), not from the kernel:

    G[b, t, l] = 1 - exp(-(l / L_b - t / T_b)^2 / (2 sigma^2))      for t < T_b and l < L_b, 0 elsewhere
    N          = sum_b T_b L_b
    guided_attention_loss = sum_{b, t, l} G A / N,   cells outside a row's T_b x L_b skipped (A may hold anything there)
    loss       = mel_loss + gate_loss + alpha * guided_attention_loss

The two quotients are formed as they stand (no integer numerator, no expm1 identity beyond torch.expm1 on the float64 argument):
in float64 l / L_b and t / T_b are the same rounded number whenever they are the same fraction, so the diagonal is exactly 0 here
too, and off it the difference is good to 1e-16 / |l / L_b - t / T_b| <= 1e-16 L T in relative terms, far below fp32 rounding.
"""
import torch

from tests import train_ref64 as R


def guide(token_lengths, mel_lengths, T, L, sigma):
    """G [B, T, L] (float64) and the mask of the cells that count (bool)."""
    tl = torch.as_tensor(token_lengths).long().clamp(0, L)
    ml = torch.as_tensor(mel_lengths).long().clamp(0, T)
    l = torch.arange(L, dtype=torch.float64)[None, None, :]
    t = torch.arange(T, dtype=torch.float64)[None, :, None]
    live = (torch.arange(T)[None, :, None] < ml[:, None, None]) & (torch.arange(L)[None, None, :] < tl[:, None, None])
    Lb, Tb = tl.double().clamp_min(1.0)[:, None, None], ml.double().clamp_min(1.0)[:, None, None]
    d = l / Lb - t / Tb
    G = -torch.expm1(-(d * d) / (2.0 * float(sigma) ** 2))
    return torch.where(live, G, torch.zeros_like(G)), live


def n_cells(token_lengths, mel_lengths, T, L):
    tl = torch.as_tensor(token_lengths).long().clamp(0, L)
    ml = torch.as_tensor(mel_lengths).long().clamp(0, T)
    return int((tl * ml).sum())


def guided_attention_loss(A, token_lengths, mel_lengths, sigma):
    """sum G A / N over the live cells as a float64 tensor (differentiable in A); 0 when N = 0."""
    B, T, L = A.shape
    G, live = guide(token_lengths, mel_lengths, T, L, sigma)
    N = n_cells(token_lengths, mel_lengths, T, L)
    if N == 0:
        return A.double().new_zeros(())
    # skipped, not multiplied by zero: a NaN outside a row's cells must not reach the sum
    return (G * torch.where(live, A.double(), torch.zeros_like(G))).sum() / N


def alignment_grad(token_lengths, mel_lengths, T, L, sigma, alpha):
    """d (alpha x guided_attention_loss) / d A [B, T, L]: alpha G / N, zeros outside the live cells (and everywhere when N = 0)."""
    G, _ = guide(token_lengths, mel_lengths, T, L, sigma)
    N = n_cells(token_lengths, mel_lengths, T, L)
    return G * (float(alpha) / N) if N else torch.zeros_like(G)


def train_step(sd, batch, masks, mc, alpha, sigma=0.4):
    """tests/train_ref64.py::train_step with loss = mel_loss + gate_loss + alpha x guided_attention_loss(alignments): the same float64
    forward, the term added to the scalar, autograd over the 48 leaves, clip_grad_norm_, float64 Adam from zero moments.  Also returns
    ``grads_unguided`` (the gradients of mel_loss + gate_loss alone, from the same graph) so that a caller can see how far the term moves
    them."""
    P, bufs = R._split(sd)
    for v in P.values():
        v.requires_grad_(True)
    outputs, loss, _ = R.forward(P, bufs, batch, masks, mc)
    ga = guided_attention_loss(outputs["alignments"], batch["token_lengths"], batch["mel_lengths"], sigma)
    total = loss["loss"] + float(alpha) * ga
    names = list(P)
    leaves = [P[k] for k in names]
    plain = dict(zip(names, torch.autograd.grad(loss["loss"], leaves, retain_graph=True)))
    grads = dict(zip(names, torch.autograd.grad(total, leaves)))
    items = {"loss": float(total.detach()), "mel_loss": float(loss["mel_loss"].detach()), "gate_loss": float(loss["gate_loss"].detach()),
             "guided_attention_loss": float(ga.detach())}
    res = {"outputs": {k: v.detach() for k, v in outputs.items()}, "loss_items": items, "grads": grads, "grads_unguided": plain, "state": bufs}
    norm = float(torch.sqrt(sum((g * g).sum() for g in grads.values())))
    coef = mc.grad_clip_thresh / (norm + 1e-6)
    res["grad_norm"], res["scale"] = norm, min(coef, 1.0)
    opt = torch.optim.Adam(leaves, lr=mc.learning_rate, weight_decay=mc.weight_decay)
    for k, p in zip(names, leaves):
        p.grad = grads[k] * res["scale"]
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    opt.step()
    res["after"] = {k: p.detach() for k, p in zip(names, leaves)}
    res["m"] = {k: opt.state[p]["exp_avg"] for k, p in zip(names, leaves)}
    res["v"] = {k: opt.state[p]["exp_avg_sq"] for k, p in zip(names, leaves)}
    return res
