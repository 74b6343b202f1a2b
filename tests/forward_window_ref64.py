"""Plain float64 restatement of the autoregressive decode with a monotonic attention window (gvx_decoder_autoregressive_windowed).

The step is tests.forward_ref.decoder_step, unchanged: its `pad` argument is per call, so the window is
`pad | outside_window(centre, back, ahead)` at every step.  Row b has a centre c_b(t), c_b(0) = 0; position l takes part in the
softmax of step t iff l < len_b and c_b(t) - back <= l <= c_b(t) + ahead; c_b(t + 1) is the lowest index at which the step's weights
are largest.  Stop rule, margin and padded outputs are those of forward_ref.autoregressive.
"""
import torch

from tests import forward_ref as fr


def outside_window(centre, back, ahead, L):
    """[B, L] bool: True where position l is not in [centre_b - back, centre_b + ahead]."""
    l = torch.arange(L)[None, :]
    c = torch.as_tensor(centre).long()[:, None]
    return (l < c - back) | (l > c + ahead)


def first_argmax(w):
    """Lowest index of the largest entry of every row of w [B, L] (comparisons only, as `positions` of gvx_alignment_stats)."""
    top = w.max(dim=1, keepdim=True).values
    return (w == top).double().argmax(dim=1)     # argmax of a 0 / 1 row returns the first 1


def softmax_window_step(e, pad, centre, back, ahead):
    """One softmax of the definition on given energies e [B, L] (the hand-worked tests): (weights, next centres, smallest top-two gap
    inside the window)."""
    mask = pad | outside_window(centre, back, ahead, e.shape[1])
    w = torch.softmax(e.masked_fill(mask, float("-inf")), dim=1)
    return w, first_argmax(w), top_two_gap(w, mask)


def top_two_gap(w, mask):
    """Per row: largest minus second largest weight among the positions that take part (inf for a window of one position)."""
    v = w.masked_fill(mask, float("-inf"))
    top2 = v.topk(min(2, v.shape[1]), dim=1).values
    if top2.shape[1] < 2:
        return torch.full((w.shape[0],), float("inf"), dtype=torch.float64)
    gap = top2[:, 0] - top2[:, 1]
    return torch.where(torch.isfinite(top2[:, 1]), gap, torch.full_like(gap, float("inf")))


@torch.no_grad()
def autoregressive_windowed(W, memory, lengths, max_steps, threshold, keep_masks, back, ahead):
    """forward_ref.autoregressive with the window.  Two more outputs: "centres" int64 [B, max_steps] (c_b(t + 1) at step t for
    t < n_frames[b], -1 behind) and "centre_margin": over all live steps and rows, the smallest gap between the largest and the
    second largest weight inside the window (inf if no window ever held two positions)."""
    assert back >= 0 and ahead >= 0
    B, L, E = memory.shape
    A, D, M = W["w_hh_a"].shape[1], W["w_hh_d"].shape[1], W["proj_w"].shape[0]
    pm, pad = memory @ W["wmem"].t(), fr.pad_mask(lengths, L)
    st = fr.initial_state(B, L, A, D, E)
    frame = torch.zeros(B, M, dtype=torch.float64)
    n_frames = torch.full((B,), max_steps, dtype=torch.long)
    alive = torch.ones(B, dtype=torch.bool)
    centre = torch.zeros(B, dtype=torch.long)
    centres = torch.full((B, max_steps), -1, dtype=torch.long)
    margin, centre_margin, recs = float("inf"), float("inf"), []
    for t in range(max_steps):
        mask = pad | outside_window(centre, back, ahead, L)
        r = fr.decoder_step(W, st, fr.prenet(W, frame, keep_masks[0, t], keep_masks[1, t]), memory, pm, mask)
        recs.append(r)
        assert bool((r["w"][mask] == 0).all())
        centre_margin = min(centre_margin, float(top_two_gap(r["w"], mask)[alive].min()))
        centre = first_argmax(r["w"])
        centres[alive, t] = centre[alive]
        s = torch.sigmoid(r["gate"])
        margin = min(margin, float((s - threshold).abs()[alive].min()))
        fired = alive & (s > threshold)
        n_frames[fired] = t + 1
        alive = alive & ~fired
        if not bool(alive.any()):
            break
        frame = r["mel"]
    out = fr._stack(recs)
    S = len(recs)
    live = torch.arange(max_steps)[None, :] < n_frames[:, None]
    mel = torch.zeros(B, M, max_steps, dtype=torch.float64)
    gate = torch.full((B, max_steps), 1e3, dtype=torch.float64)
    align = torch.zeros(B, max_steps, L, dtype=torch.float64)
    mel[:, :, :S], gate[:, :S], align[:, :S] = out["mel"].permute(1, 2, 0), out["gate"].t(), out["w"].permute(1, 0, 2)
    out.update(n_frames=n_frames, margin=margin, mel_out=mel * live[:, None, :], gate_out=torch.where(live, gate, torch.full_like(gate, 1e3)),
               align_out=align * live[:, :, None], centres=centres, centre_margin=centre_margin)
    return out
