"""Plain float64 restatement of the three forward recurrences, step by step, with every intermediate kept: what
tests/test_forward_loops_gpu.py holds the HIP loops to and what tests/test_bptt_gpu.py differentiates.

Written from DESIGN.md section 1 and the C ABI's header (which names the reference lines each call replaces), not from the
kernels: matrix products as `x @ W.t()`, torch's conv1d / softmax / sigmoid / tanh, one python loop over the steps.  Every input
is an fp32 number converted to float64 once; nothing is rounded on the way.  tests/test_oracle_golden.py pins the three entry
points to the committed fixtures of the reference (CPU).

  decoder_step        one step of the decoder loop (attention LSTM cell, location-sensitive attention, decoder LSTM cell, optional
                      mel / gate projection); `track` lets a caller mark tensors for autograd (the BPTT tests)
  teacher_forced      Prenet over all frames + T steps, optional hidden-state dropout masks and scales (the training call)
  autoregressive      a batch of rows, each stopping on its own; padding values as include/genvox_amd.h states them
  encoder_bilstm      BiLSTM with packed-sequence semantics on the convolution stack's output: memory, cell states, input
                      pre-activations
oracle/tacotron2_ref.py takes its dtype from its inputs, so its `encoder` (embedding + convolutions + BiLSTM) runs in float64 on a
float64 state dict: whole_encoder uses it for the convolution stack and this file's recurrence behind it.
"""
import torch
import torch.nn.functional as F

_ATT = "decoder.attention_layer."


def lstm_cell(gates, c):
    """torch's gate order i, f, g, o along the last dimension."""
    i, f, g, o = gates.chunk(4, dim=-1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c_new), c_new


def to_f64(sd):
    """A state dict's floating tensors as float64 (counters are left out)."""
    return {k: v.double() for k, v in sd.items() if v.is_floating_point()}


def decoder_weights(sd):
    """The decoder loop's parameters under short names, float64; the two biases of each cell as their sum."""
    sd = to_f64(sd)
    return {
        "w_ih_a": sd["decoder.attention_rnn.weight_ih"], "w_hh_a": sd["decoder.attention_rnn.weight_hh"],
        "b_a": sd["decoder.attention_rnn.bias_ih"] + sd["decoder.attention_rnn.bias_hh"],
        "w_ih_d": sd["decoder.decoder_rnn.weight_ih"], "w_hh_d": sd["decoder.decoder_rnn.weight_hh"],
        "b_d": sd["decoder.decoder_rnn.bias_ih"] + sd["decoder.decoder_rnn.bias_hh"],
        "wq": sd[_ATT + "query_layer.linear_layer.weight"], "v": sd[_ATT + "v.linear_layer.weight"][0],
        "wmem": sd[_ATT + "memory_layer.linear_layer.weight"],
        "loc_conv": sd[_ATT + "location_layer.location_conv.conv.weight"],
        "loc_dense": sd[_ATT + "location_layer.location_dense.linear_layer.weight"],
        "pre_w0": sd["decoder.prenet.layers.0.linear_layer.weight"], "pre_w1": sd["decoder.prenet.layers.1.linear_layer.weight"],
        "proj_w": sd["decoder.linear_projection.linear_layer.weight"], "proj_b": sd["decoder.linear_projection.linear_layer.bias"],
        "gate_w": sd["decoder.gate_layer.linear_layer.weight"][0], "gate_b": sd["decoder.gate_layer.linear_layer.bias"][0],
    }


def initial_state(B, L, A, D, E):
    z = lambda n: torch.zeros(B, n, dtype=torch.float64)
    return {"h_a": z(A), "c_a": z(A), "h_d": z(D), "c_d": z(D), "ctx": z(E), "w": z(L), "wcum": z(L)}


def decoder_step(W, st, x_p, memory, pm, pad, att_keep=None, dec_keep=None, track=lambda x: x):
    """One decoder step.  st: the state dict of initial_state (replaced in place by the step's); x_p [B, P] the Prenet output;
    pad [B, L] True at and past a row's length; att_keep / dec_keep [B, H]: keep mask times 1 / (1 - p) of the dropout on each
    cell's hidden output (None: none).  Returns every intermediate of the step."""
    kl = W["loc_conv"].shape[2]
    ga = track(torch.cat((x_p, st["ctx"]), 1) @ W["w_ih_a"].t() + st["h_a"] @ W["w_hh_a"].t() + W["b_a"])
    h, c_a = lstm_cell(ga, st["c_a"])
    h_a = h if att_keep is None else h * att_keep
    q = track(h_a @ W["wq"].t())
    locf = F.conv1d(torch.stack((st["w"], st["wcum"]), 1), W["loc_conv"], padding=(kl - 1) // 2)      # [B, F, L]
    loc = locf.transpose(1, 2) @ W["loc_dense"].t()                                                       # [B, L, a]
    e = torch.tanh(q[:, None, :] + loc + pm) @ W["v"]
    w = torch.softmax(e.masked_fill(pad, float("-inf")), dim=1)
    ctx = track((w[:, None, :] @ memory)[:, 0])
    wcum = st["wcum"] + w
    gd = track(torch.cat((h_a, ctx), 1) @ W["w_ih_d"].t() + st["h_d"] @ W["w_hh_d"].t() + W["b_d"])
    h, c_d = lstm_cell(gd, st["c_d"])
    h_d = h if dec_keep is None else h * dec_keep
    rec = {"prenet": x_p, "ga": ga, "c_a": c_a, "h_a": h_a, "q": q, "e": e, "w": w, "wcum": wcum, "ctx": ctx, "gd": gd, "c_d": c_d, "h_d": h_d}
    if "proj_w" in W:
        hc = torch.cat((h_d, ctx), 1)
        rec["mel"] = hc @ W["proj_w"].t() + W["proj_b"]
        rec["gate"] = hc @ W["gate_w"] + W["gate_b"]
    st.update(h_a=h_a, c_a=c_a, h_d=h_d, c_d=c_d, ctx=ctx, w=w, wcum=wcum)
    return rec


def prenet(W, frames, keep0, keep1):
    """relu(linear) and the always-on dropout of p = 0.5 (kept units times 2), twice."""
    h = torch.relu(frames @ W["pre_w0"].t()) * (keep0.double() * 2.0)
    return torch.relu(h @ W["pre_w1"].t()) * (keep1.double() * 2.0)


def pad_mask(lengths, L):
    return torch.arange(L)[None, :] >= torch.as_tensor(lengths).long()[:, None]


def _stack(recs):
    return {k: torch.stack([r[k] for r in recs]) for k in recs[0]}


@torch.no_grad()
def teacher_forced(W, memory, lengths, mel_in, keep_masks, att_keep=None, dec_keep=None, att_scale=1.0, dec_scale=1.0, keys=None):
    """memory [B, L, E], mel_in [B, M, T] (float64), keep_masks uint8 [2, (T+1) B, P] (row t B + b), att_keep / dec_keep uint8
    [T, B, H] or None.  Returns the stacked per-step records ([T, B, ...]) plus "pm"; keys: keep only these (long runs)."""
    B, L, E = memory.shape
    T = mel_in.shape[2]
    A, D, P = W["w_hh_a"].shape[1], W["w_hh_d"].shape[1], W["pre_w0"].shape[0]
    frames = torch.cat((torch.zeros(1, B, mel_in.shape[1], dtype=torch.float64), mel_in.permute(2, 0, 1)), 0)   # [T+1, B, M]
    km = keep_masks.reshape(2, T + 1, B, P)
    pre = prenet(W, frames, km[0], km[1])
    pm, pad = memory @ W["wmem"].t(), pad_mask(lengths, L)
    st = initial_state(B, L, A, D, E)
    recs = []
    for t in range(T):
        r = decoder_step(W, st, pre[t], memory, pm, pad, None if att_keep is None else att_keep[t].double() * att_scale,
                         None if dec_keep is None else dec_keep[t].double() * dec_scale)
        recs.append(r if keys is None else {k: r[k] for k in keys})
    out = _stack(recs)
    out["pm"] = pm
    return out


@torch.no_grad()
def autoregressive(W, memory, lengths, max_steps, threshold, keep_masks, forced_frames=None):
    """memory [B, L, E]; keep_masks uint8 [2, max_steps, B, P].  Every row stops on its own: n_frames[b] = index of the first step
    whose sigmoid(gate) > threshold, plus one (or max_steps).  Returns the per-step records over the steps that ran
    (max n_frames), "n_frames", "margin" (the smallest |sigmoid(gate) - threshold| over the steps a row was alive) and the
    padded outputs as the C ABI lays them out: "mel_out" [B, M, max_steps] (0 past n_frames), "gate_out" [B, max_steps] (1e3),
    "align_out" [B, max_steps, L] (0).
    forced_frames [steps, B, M] (float64): feed these instead of the reference's own frames (step t > 0 reads forced_frames[t - 1])
    - one step's arithmetic on somebody else's trajectory; the stop rule then also reads the given run (no early stop)."""
    B, L, E = memory.shape
    A, D, M = W["w_hh_a"].shape[1], W["w_hh_d"].shape[1], W["proj_w"].shape[0]
    pm, pad = memory @ W["wmem"].t(), pad_mask(lengths, L)
    st = initial_state(B, L, A, D, E)
    frame = torch.zeros(B, M, dtype=torch.float64)
    n_frames = torch.full((B,), max_steps, dtype=torch.long)
    alive = torch.ones(B, dtype=torch.bool)
    margin, recs = float("inf"), []
    steps = max_steps if forced_frames is None else min(max_steps, forced_frames.shape[0])
    for t in range(steps):
        r = decoder_step(W, st, prenet(W, frame, keep_masks[0, t], keep_masks[1, t]), memory, pm, pad)
        recs.append(r)
        s = torch.sigmoid(r["gate"])
        if forced_frames is None:
            margin = min(margin, float((s - threshold).abs()[alive].min()))
            fired = alive & (s > threshold)
            n_frames[fired] = t + 1
            alive = alive & ~fired
            if not bool(alive.any()):
                break
            frame = r["mel"]
        else:
            frame = forced_frames[t]
    out = _stack(recs)
    S = len(recs)
    live = torch.arange(max_steps)[None, :] < n_frames[:, None]                                   # [B, max_steps]
    mel = torch.zeros(B, M, max_steps, dtype=torch.float64)
    gate = torch.full((B, max_steps), 1e3, dtype=torch.float64)
    align = torch.zeros(B, max_steps, L, dtype=torch.float64)
    mel[:, :, :S], gate[:, :S], align[:, :S] = out["mel"].permute(1, 2, 0), out["gate"].t(), out["w"].permute(1, 0, 2)
    out.update(n_frames=n_frames, margin=margin, mel_out=mel * live[:, None, :], gate_out=torch.where(live, gate, torch.full_like(gate, 1e3)),
               align_out=align * live[:, :, None])
    return out


@torch.no_grad()
def encoder_bilstm(sd64, conv_out, lengths):
    """conv_out [B, E, L] float64 (the convolution stack's output, reference layout); lengths or None (= all L).  Packed-sequence
    semantics: the reverse direction starts at each row's own last token, nothing past a row's length is written.
    Returns memory [B, L, 2H], cells [B, L, 2H] (forward direction in the first H channels), xg [B, L, 2, 4H] = W_ih x + b_ih +
    b_hh in torch's gate-major row order."""
    x = conv_out.transpose(1, 2)
    B, L, _ = x.shape
    H = sd64["encoder.lstm.weight_hh_l0"].shape[1]
    lens = torch.full((B,), L, dtype=torch.long) if lengths is None else torch.as_tensor(lengths).long()
    memory, cells = torch.zeros(B, L, 2 * H, dtype=torch.float64), torch.zeros(B, L, 2 * H, dtype=torch.float64)
    xgs, rows = [], torch.arange(B)
    for d, sfx in enumerate(("", "_reverse")):
        w_hh = sd64["encoder.lstm.weight_hh_l0" + sfx]
        xg = x @ sd64["encoder.lstm.weight_ih_l0" + sfx].t() + (sd64["encoder.lstm.bias_ih_l0" + sfx] + sd64["encoder.lstm.bias_hh_l0" + sfx])
        xgs.append(xg)
        h, c = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        for s in range(L):
            active = s < lens
            pos = torch.full((B,), s) if d == 0 else (lens - 1 - s).clamp_min(0)
            hn, cn = lstm_cell(xg[rows, pos] + h @ w_hh.t(), c)
            h, c = torch.where(active[:, None], hn, h), torch.where(active[:, None], cn, c)
            memory[rows[active], pos[active], d * H:(d + 1) * H] = hn[active]
            cells[rows[active], pos[active], d * H:(d + 1) * H] = cn[active]
    return {"memory": memory, "cells": cells, "xg": torch.stack(xgs, 2)}


@torch.no_grad()
def whole_encoder(sd64, tokens, lengths):
    """Embedding + (convolution, eval-mode BatchNorm, relu) stack + BiLSTM.  The stack is oracle/tacotron2_ref.py's, which computes
    in the dtype of the state dict it is given; the recurrence is encoder_bilstm."""
    from oracle import tacotron2_ref as R

    x = sd64["embedding.weight"][tokens.long()].transpose(1, 2)
    i = 0
    while f"encoder.convolutions.{i}.0.conv.weight" in sd64:
        x = torch.relu(R._conv_bn(x, sd64, f"encoder.convolutions.{i}"))
        i += 1
    assert x.dtype == torch.float64
    return encoder_bilstm(sd64, x, lengths)
