"""Gradients of the MelGAN generator of include/genvox_amd.h by torch autograd through a restatement with torch's own convolutions, for
the tests of the device's backward.  It imports nothing from genvox_amd.  ``loss = sum(wav * G)`` for a cotangent G supplied from
outside; everything is computed in the dtype of the state dict it is given.

The restatement here is tests/melgan_ref64.py's ``generator`` with two additions: it returns every tensor of the backward's tape (raw
pre-activations, in forward order), and every ``lrelu(x)`` can be *pinned*: replaced by ``x * m`` with ``m`` in {1, slope} supplied from
outside, one mask per tape tensor.  A pre-activation within rounding of 0 flips a LeakyReLU and changes a gradient by a finite amount;
pinned to the device's own decisions, float64 and the device differentiate the same piecewise-linear function."""
import torch
import torch.nn.functional as F

from tests import melgan_ref64 as R

FACTOR = 8.0
ULP = 2.0 ** -23


def param_names(cfg):
    names = ["pre"]
    for i in range(len(cfg["ratios"])):
        names.append(f"ups.{i}")
        for j in range(cfg["n_res"]):
            names += [f"res.{i}.{j}.conv", f"res.{i}.{j}.shortcut", f"res.{i}.{j}.mix"]
    names.append("post")
    return [n + s for n in names for s in (".weight", ".bias")]


def generator_tape(sd, mel, cfg, masks=None):
    """mel [B, n_mels, T] -> (wav [B, T * hop], tape): tape[0] is the mel itself, tape[1:] the raw x after the first convolution, then per
    stage the transposed convolution's output and per residual layer h and the new x, each [B, C, len].  ``masks``: None, or a list
    aligned with the tape (entry 0 unused) whose entry i replaces lrelu(tape[i]) by tape[i] * masks[i]."""
    s = cfg["slope"]
    tape = [mel]

    def keep(x):
        tape.append(x)
        return x

    def act(x):   # x is always the tensor kept last or the one before it: find it by identity
        i = next(k for k in range(len(tape) - 1, 0, -1) if tape[k] is x)
        return F.leaky_relu(x, s) if masks is None else x * masks[i]

    x = keep(F.conv1d(F.pad(mel, (3, 3), mode="reflect"), sd["pre.weight"], sd["pre.bias"]))
    for i, r in enumerate(cfg["ratios"]):
        x = keep(F.conv_transpose1d(act(x), sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=r, padding=r // 2))
        for j in range(cfg["n_res"]):
            d = cfg["dil_base"] ** j
            p = f"res.{i}.{j}."
            h = keep(F.conv1d(F.pad(act(x), (d, d), mode="reflect"), sd[p + "conv.weight"], sd[p + "conv.bias"], dilation=d))
            x = keep(F.conv1d(x, sd[p + "shortcut.weight"], sd[p + "shortcut.bias"]) + F.conv1d(act(h), sd[p + "mix.weight"], sd[p + "mix.bias"]))
    wav = torch.tanh(F.conv1d(F.pad(act(x), (3, 3), mode="reflect"), sd["post.weight"], sd["post.bias"]))
    return wav[:, 0], tape


def tape_muls(cfg):
    """Positions per frame of every tape tensor."""
    muls, mul = [1, 1], 1
    for r in cfg["ratios"]:
        mul *= r
        muls += [mul] * (1 + 2 * cfg["n_res"])
    return muls


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


def tape_muls_of(ref):
    T = ref["tape"][0].shape[2]
    return [t.shape[2] // T for t in ref["tape"]]


def masks_from_tape(tape, slope):
    """tape tensors [B, C, len] (any dtype) -> the masks that pin every LeakyReLU to the side `x > 0` decides."""
    one, low = torch.tensor(1.0, dtype=torch.float64), torch.tensor(slope, dtype=torch.float64)
    return [None] + [torch.where(t > 0, one, low) for t in tape[1:]]


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


def one_number_movement(sd, cfg, mel, G, name="post.bias", draws=24, seed=0):
    """For a gradient that is ONE number: (its float64 value, the 90th percentile of |float32 restatement - float64| over ``draws``
    evaluations whose mel is moved by up to one float32 ulp, element by element).  The float32 restatement's error on one number is a
    single draw of the host library's rounding; the percentile says how far float32 arithmetic moves the number whatever the host."""
    _, _, g64 = run(sd, mel, None, cfg, G, None, torch.float64)
    gen, ds = torch.Generator().manual_seed(seed), []
    for i in range(draws):
        m = mel.float()
        if i:
            m = m * (1 + (torch.randint(0, 3, m.shape, generator=gen) - 1).float() * ULP)
        _, _, g32 = run(sd, m.double(), None, cfg, G, None, torch.float32)
        ds.append((g32[name].double() - g64[name]).abs().item())
    return g64[name].item(), torch.tensor(ds).quantile(0.9).item()
