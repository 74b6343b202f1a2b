"""Gradients of the HiFi-GAN generator of include/genvox_amd.h by torch autograd through a restatement with torch's own convolutions,
for the tests of the device's backward.  It imports nothing from genvox_amd.  ``loss = sum(wav * G)`` for a cotangent G supplied from
outside; everything is computed in the dtype of the state dict it is given.

The restatement here is tests/hifigan_ref64.py's ``generator`` with two additions: it returns every tensor of the backward's tape (raw
pre-activations, in the order the header states), and every ``lrelu(x)`` can be *pinned*: replaced by ``x * m`` with ``m`` in
{1, slope} supplied from outside, one mask per tape tensor.  A pre-activation within rounding of 0 flips a LeakyReLU and changes a
gradient by a finite amount; pinned to the device's own decisions, float64 and the device differentiate the same piecewise-linear
function."""
import torch
import torch.nn.functional as F

from tests import hifigan_ref64 as R

FACTOR = 8.0
ULP = 2.0 ** -23


def param_names(cfg):
    names, n_k = ["conv_pre"], len(cfg["kernels"])
    for i in range(len(cfg["rates"])):
        names.append(f"ups.{i}")
        for j in range(n_k):
            for m in range(len(cfg["dilations"][j])):
                names += R.conv_names(cfg, i * n_k + j, m)
    names.append("conv_post")
    return [n + s for n in names for s in (".weight", ".bias")]


def generator_tape(sd, mel, cfg, masks=None):
    """mel [B, n_mels, T] -> (wav [B, T * hop], tape): tape[0] is the mel itself, tape[1] conv_pre's output, then per stage ups' output,
    per residual block and dilation m the inner tensor (convs1's output, resblock "1" only) and the block's running value after m (every
    m but the last), and the stage's average; each [B, C, len].  ``masks``: None, or a list aligned with the tape (entry 0 unused) whose
    entry i replaces lrelu(tape[i]) by tape[i] * masks[i]."""
    tape = [mel]

    def keep(x):
        tape.append(x)
        return x

    def act(x, slope):
        if masks is None:
            return F.leaky_relu(x, slope)
        i = next(k for k in range(len(tape) - 1, 0, -1) if tape[k] is x)   # a kept tensor: found by identity
        return x * masks[i]

    s, n_k = cfg["slope"], len(cfg["kernels"])
    x = keep(F.conv1d(mel, sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3))
    for i, r in enumerate(cfg["rates"]):
        x = keep(F.conv_transpose1d(act(x, s), sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=r, padding=r // 2))
        xs = None
        for j, (k, ds) in enumerate(zip(cfg["kernels"], cfg["dilations"])):
            y = x
            for m, d in enumerate(ds):
                names = R.conv_names(cfg, i * n_k + j, m)
                t = F.conv1d(act(y, s), sd[names[0] + ".weight"], sd[names[0] + ".bias"], dilation=d, padding=(k - 1) * d // 2)
                if len(names) == 2:
                    t = F.conv1d(act(keep(t), s), sd[names[1] + ".weight"], sd[names[1] + ".bias"], padding=(k - 1) // 2)
                y = y + t
                if m < len(ds) - 1:
                    keep(y)
            xs = y if xs is None else xs + y
        x = keep(xs / n_k)
    wav = torch.tanh(F.conv1d(act(x, cfg["post_slope"]), sd["conv_post.weight"], sd["conv_post.bias"], padding=3))
    return wav[:, 0], tape


def tape_entries(cfg):
    """(positions per frame, channels, the slope of the LeakyReLU it passes through) of every tape tensor, in order: the header's
    formula, restated."""
    per_dil = 2 if cfg["resblock"] == "1" else 1
    out, mul, c = [(1, (cfg["n_mels"] + 3) // 4 * 4, None), (1, cfg["c0"], cfg["slope"])], 1, cfg["c0"]
    for i, r in enumerate(cfg["rates"]):
        mul, c = mul * r, c // 2
        count = 2 + sum(len(ds) * per_dil - 1 for ds in cfg["dilations"])
        out += [(mul, c, cfg["slope"])] * (count - 1)
        out.append((mul, c, cfg["post_slope"] if i == len(cfg["rates"]) - 1 else cfg["slope"]))
    return out


def tape_muls(cfg):
    return [e[0] for e in tape_entries(cfg)]


def run(sd, mel, lengths, cfg, G, masks=None, dtype=torch.float64):
    """Forward and backward in ``dtype``, every row alone at its own length (``lengths`` None: the whole batch at once).
    -> (wav, tape zero-filled behind the lengths, {name: gradient} with "mel" among the names; parameter gradients are the sum
    over the rows)."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    B, M, T = mel.shape
    rows = [(slice(0, B), T)] if lengths is None else [(slice(b, b + 1), t) for b, t in enumerate(lengths)]
    muls = tape_muls(cfg)
    wav_all, tape_all, d_mel = None, None, torch.zeros(B, M, T, dtype=dtype)
    for rs, t in rows:
        m = mel[rs, :, :t].to(dtype).clone().requires_grad_(True)
        mk = None if masks is None else [None if k is None else k[rs, :, :t * mu].to(dtype) for k, mu in zip(masks, muls)]
        wav, tape = generator_tape(sd, m, cfg, mk)
        (wav * G[rs, :wav.shape[1]].to(dtype)).sum().backward()
        if wav_all is None:
            wav_all = torch.zeros(B, T * R.hop(cfg), dtype=dtype)
            tape_all = [torch.zeros(B, x.shape[1], T * mu, dtype=dtype) for x, mu in zip(tape, muls)]
        wav_all[rs, :wav.shape[1]] = wav.detach()
        for full, one in zip(tape_all, tape):
            full[rs, :, :one.shape[2]] = one.detach()
        d_mel[rs, :, :t] = m.grad
    grads = {k: v.grad for k, v in sd.items()}
    grads["mel"] = d_mel
    return wav_all, tape_all, grads


def reference(sd, mel, lengths, cfg, G, masks=None):
    """-> dict(wav, tape, grads: float64;  tape_err, grad_err: per tensor the largest |float32 restatement - float64|;  grad_tol: what
    the device may differ from float64 by, FACTOR * max(grad_err, one ulp of the tensor's largest gradient))."""
    w64, t64, g64 = run(sd, mel, lengths, cfg, G, masks, torch.float64)
    w32, t32, g32 = run(sd, mel, lengths, cfg, G, masks, torch.float32)
    tape_err = [(a.double() - b).abs().max().item() for a, b in zip(t32, t64)]
    grad_err = {k: (g32[k].double() - g64[k]).abs().max().item() for k in g64}
    grad_tol = {k: FACTOR * max(grad_err[k], ULP * g64[k].abs().max().item()) for k in g64}
    return dict(wav=w64, tape=t64, grads=g64, tape_err=tape_err, grad_err=grad_err, grad_tol=grad_tol, wav_err=(w32.double() - w64).abs().max().item())


def tape_muls_of(ref):
    T = ref["tape"][0].shape[2]
    return [t.shape[2] // T for t in ref["tape"]]


def near_ties(ref, lengths=None):
    """How many pre-activations of the float64 tape (inside the rows) lie within FACTOR x that tensor's float32 error of 0: where float32
    arithmetic in another order may take the other side of a LeakyReLU."""
    count = 0
    muls = tape_muls_of(ref)
    for i, (t, e) in enumerate(zip(ref["tape"], ref["tape_err"])):
        if i == 0:
            continue
        close = t.abs() <= FACTOR * e
        if lengths is not None:
            for b, n in enumerate(lengths):
                close[b, :, n * muls[i]:] = False
        count += int(close.sum())
    return count


def masks_from_tape(tape, cfg):
    """tape tensors [B, C, len] (any dtype) -> the masks that pin every LeakyReLU to the side `x > 0` decides."""
    one = torch.tensor(1.0, dtype=torch.float64)
    return [None] + [torch.where(t > 0, one, torch.tensor(e[2], dtype=torch.float64)) for t, e in zip(tape[1:], tape_entries(cfg)[1:])]


def tie_free_case(sd, cfg, B, T, lengths, G_seed, seeds=range(1, 9)):
    """The first ``random_mel`` seed among ``seeds`` whose float64 forward has no near-tie -> (seed, mel, G, reference); an
    AssertionError if there is none."""
    g = torch.Generator().manual_seed(G_seed)
    G = torch.randn(B, T * R.hop(cfg), generator=g, dtype=torch.float64)
    for seed in seeds:
        mel = R.random_mel(cfg, B, T, seed)
        ref = reference(sd, mel, lengths, cfg, G)
        if near_ties(ref, lengths) == 0:
            return seed, mel, G, ref
    raise AssertionError(f"no tie-free mel among seeds {list(seeds)} for {B} x {T}")
