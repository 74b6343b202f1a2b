"""GPU: one MelGANTrainer.train_step of a tiny generator against a tiny discriminator (B = 2, ragged) against a restatement of the same
step: tests/melgan_ref64.py for G, tests/melgan_disc_ref64.py for D, the two losses written out, torch's Adam and clip_grad_norm_ on
float64 leaves.  The bound of every post-step parameter tensor and of every loss term is 8 x max(|float32 restatement of the step -
float64|, one ulp of the value), as everywhere in these tests.

Conditioning.  Adam's first step moves a parameter by lr * g / (|g| + eps), g being the clipped gradient plus weight_decay * p, and
d/dg of that is lr * eps / (|g| + eps)^2: up to lr / eps where g is within eps = 1e-8 of 0.  A gradient there that differs from float64
by well under its own bound still moves the parameter by more than the parameter's bound.  Seen at lr = 1e-3 and weight_decay = 1e-2:
in one element of ups.0.weight the gradient and the weight decay nearly cancelled, g = 1.2e-7; the device's gradient was 1e-9 from
float64, an eighth of its bound, and the parameter 5.6e-7 away against a bound of 5.0e-7.  That is a property of the step, not of
the kernels, and the float32 restatement shows it only by luck.  So the hyper-parameters keep the amplification low - the smallest
learning rate the config takes, a weight decay far below the gradients - and the inputs are chosen on the reference alone, as the
tie-free cases of the backward tests are: the first seed for which, at every element of the generator's step in float64, the
gradient's own bound times that derivative stays below half the parameter's bound (``well_conditioned``).  The device's gradients are
asserted against their bounds before the parameters are.
The discriminator cannot be chosen that way: the hinge loss's real and fake halves cancel exactly in some bias gradients (all
positions active on both sides), so those elements are 0 in exact arithmetic and rounding noise in any other, in every case; there the
weight decay term, 1e-6 |p|, far above that noise, is what Adam normalises.  Its steps are held to the float32 restatement's error
alone, as the issue states the bound.
"""
import functools

import pytest
import torch

from genvox_amd.configs import AudioConfig, MelGANConfig, MelGANDiscriminatorConfig
from genvox_amd.melgan import MelGANGenerator
from genvox_amd.melgan_disc import MelGANDiscriminator
from genvox_amd.melgan_training import MelGANTrainer
from tests import melgan_disc_ref64 as DR
from tests import melgan_ref64 as R
from tests import stft_loss_ref64 as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
G_CFG, D_CFG = R.NARROW, DR.TINY
HP = dict(train_repeat_discriminator=2, feat_match=10.0, learning_rate=1e-5, weight_decay=1e-6, grad_clip_thresh=1.0, beta1=0.5, beta2=0.9)
ADAM_EPS = 1e-8   # torch.optim.Adam's default, which MelGANTrainer keeps
MEL_LENGTHS = (9, 6)   # 72 and 48 samples at hop 8


def _row_mean(rows):
    """rows: one tensor [1, C, L_b] per row -> the mean over rows of every row's own mean."""
    return sum(r.mean() for r in rows) / len(rows)


def restated_step(sd_g, sd_d, mel, wav, dtype, mel_lengths=MEL_LENGTHS, stft=None):
    """The step of MelGANTrainer.train_step in ``dtype`` -> (post-step parameters of G and of D after every discriminator step, terms, G's clipped gradients).
    ``stft`` = (resolutions, stft_weight) adds the spectral-convergence term of tests/stft_loss_ref64.py (w_mag = 0) to the generator's
    loss: the mean over rows and resolutions, every row at its own length."""
    pg = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_g.items()}
    pd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_d.items()}
    adam = dict(lr=HP["learning_rate"], betas=(HP["beta1"], HP["beta2"]), weight_decay=HP["weight_decay"])
    opt_g, opt_d = torch.optim.Adam(list(pg.values()), **adam), torch.optim.Adam(list(pd.values()), **adam)
    hop = R.hop(G_CFG)
    fake = [R.generator(pg, mel[b:b + 1, :, :t].to(dtype), G_CFG)[0] for b, t in enumerate(mel_lengths)]
    real = [wav[b:b + 1, :t * hop].to(dtype) for b, t in enumerate(mel_lengths)]
    n_scales, n_maps = D_CFG["n_scales"], D_CFG["n_layers"] + 3
    d_states = []
    for _ in range(HP["train_repeat_discriminator"]):
        opt_d.zero_grad()
        d_real = [DR.discriminator(pd, r, D_CFG) for r in real]
        d_fake = [DR.discriminator(pd, f.detach(), D_CFG) for f in fake]
        d_loss = sum(_row_mean([torch.relu(1 - m[k][-1]) for m in d_real]) + _row_mean([torch.relu(1 + m[k][-1]) for m in d_fake]) for k in range(n_scales))
        d_loss.backward()
        assert all(p.grad is None for p in pg.values())
        torch.nn.utils.clip_grad_norm_(list(pd.values()), HP["grad_clip_thresh"])
        opt_d.step()
        d_states.append({k: v.detach().clone() for k, v in pd.items()})
    opt_g.zero_grad()
    with torch.no_grad():
        d_real = [DR.discriminator(pd, r, D_CFG) for r in real]
    d_fake = [DR.discriminator(pd, f, D_CFG) for f in fake]
    adv = sum(-_row_mean([m[k][-1] for m in d_fake]) for k in range(n_scales))
    weight = 4.0 / (D_CFG["n_layers"] + 1) / n_scales
    fm = HP["feat_match"] * sum(weight * _row_mean([(f[k][i] - r[k][i]).abs() for f, r in zip(d_fake, d_real)]) for k in range(n_scales) for i in range(n_maps - 1))
    g_loss = adv + fm
    terms = dict(d_loss=d_loss.item(), g_adv=adv.item(), g_feat_match=fm.item())
    if stft is not None:
        res, weight = stft
        g_stft = sum(SR.row_terms(f[0], r[0], rs)[0] for f, r in zip(fake, real) for rs in res) / (len(fake) * len(res))
        g_loss = g_loss + weight * g_stft
        terms["g_stft"] = g_stft.item()
    g_loss.backward()
    torch.nn.utils.clip_grad_norm_(list(pg.values()), HP["grad_clip_thresh"])
    g_grads = {k: v.grad.detach().clone() for k, v in pg.items()}   # as the optimizer sees them: clipped
    opt_g.step()
    terms["g_loss"] = g_loss.item()
    return {k: v.detach() for k, v in pg.items()}, d_states, terms, g_grads


def _bound(a32, a64):
    err = (a32.double() - a64).abs().max().item()
    return DR.FACTOR * max(err, DR.ULP * a64.abs().max().item())


def well_conditioned(sd_g, sd_d, r64, r32):
    """On the two restatements alone: at every element of G's step, (the gradient's bound) x lr eps / (|g| + eps)^2 is at most half the
    post-step parameter's bound."""
    lr, wd = HP["learning_rate"], HP["weight_decay"]
    firsts = [(k, r64[3][k], r32[3][k], sd_g[k], r64[0][k], r32[0][k]) for k in sd_g]
    for k, g64, g32, p_before, p64, p32 in firsts:
        total = g64 + wd * p_before
        worst = (lr * ADAM_EPS / (total.abs() + ADAM_EPS) ** 2).max().item()
        if worst * _bound(g32, g64) > 0.5 * _bound(p32, p64):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _case():
    """(weights, inputs, float64 and float32 restatement) of the first well-conditioned seed: computed once, never changed."""
    sd_g, sd_d = R.random_state(G_CFG, 21), DR.random_state(D_CFG, 22)
    for seed in range(1, 33):
        mel = R.random_mel(G_CFG, 2, max(MEL_LENGTHS), seed)
        wav = DR.random_wav(2, max(MEL_LENGTHS) * R.hop(G_CFG), 100 + seed)
        r64, r32 = restated_step(sd_g, sd_d, mel, wav, torch.float64), restated_step(sd_g, sd_d, mel, wav, torch.float32)
        if well_conditioned(sd_g, sd_d, r64, r32):
            print(f"input seed {seed} gives a well-conditioned step")
            return sd_g, sd_d, mel, wav, r64, r32
    raise AssertionError("no well-conditioned step among seeds 1 .. 32")


def _models(sd_g=None, sd_d=None):
    if sd_g is None:
        sd_g, sd_d = _case()[:2]
    ac = AudioConfig(n_mels=12)
    ac.n_mels, ac.hop_length = G_CFG["n_mels"], R.hop(G_CFG)   # below a preprocessing config's ranges: a test's size
    gen = MelGANGenerator(MelGANConfig(base_channels=G_CFG["base_channels"], upsample_ratios=G_CFG["ratios"], n_residual_layers=G_CFG["n_res"],
                                       dilation_base=G_CFG["dil_base"], leaky_slope=G_CFG["slope"], **HP), ac)
    disc = MelGANDiscriminator(MelGANDiscriminatorConfig(n_scales=D_CFG["n_scales"], base_channels=D_CFG["base_channels"], n_layers=D_CFG["n_layers"],
                                                         downsampling_factor=D_CFG["s"], max_channels=D_CFG["max_channels"], leaky_slope=D_CFG["slope"]))
    gen.load_state_dict({k: v.float() for k, v in sd_g.items()})
    disc.load_state_dict({k: v.float() for k, v in sd_d.items()})
    return gen.to(DEV), disc.to(DEV)


def _within(got, a64, a32, what):
    a64, a32 = torch.as_tensor(a64, dtype=torch.float64), torch.as_tensor(a32, dtype=torch.float64)
    err = (a32 - a64).abs().max().item()
    tol = DR.FACTOR * max(err, DR.ULP * a64.abs().max().item())
    d = (torch.as_tensor(got, dtype=torch.float64).cpu() - a64).abs().max().item()
    print(f"{what}: device error {d:.3e}, float32 restatement error {err:.3e}, bound {tol:.3e}")
    assert d <= tol, f"{what}: {d:.3e} from float64, above the bound {tol:.3e}"


def test_one_train_step_against_float64():
    sd_g, sd_d, mel, wav, (g64, d64, t64, gg64), (g32, d32, t32, gg32) = _case()
    gen, disc = _models()
    trainer = MelGANTrainer(gen, disc)
    assert trainer.optimizer_g.defaults["lr"] == 1e-5 and trainer.optimizer_d.defaults["betas"] == (0.5, 0.9) and trainer.optimizer_d.defaults["weight_decay"] == 1e-6
    assert trainer.optimizer_g.defaults["eps"] == ADAM_EPS == trainer.optimizer_d.defaults["eps"]
    mel_d, wav_d = mel.clone(), wav.clone()
    for b, t in enumerate(MEL_LENGTHS):   # whatever lies behind a row's length is never read
        mel_d[b, :, t:] = NAN
        wav_d[b, t * R.hop(G_CFG):] = NAN
    g_before = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    seen = dict(d_steps=[], g_grads_at_d_step=[], d_at_g_step=None)
    d_step, g_step = trainer.optimizer_d.step, trainer.optimizer_g.step

    def d_wrapped(*a, **kw):
        seen["g_grads_at_d_step"].append([p.grad for p in gen.parameters()])
        out = d_step(*a, **kw)
        seen["d_steps"].append({k: v.detach().clone() for k, v in disc.state_dict().items()})
        return out

    def g_wrapped(*a, **kw):
        seen["d_at_g_step"] = {k: v.detach().clone() for k, v in disc.state_dict().items()}
        seen["d_requires_grad"] = [p.requires_grad for p in disc.parameters()]
        seen["g_grads"] = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
        return g_step(*a, **kw)

    trainer.optimizer_d.step, trainer.optimizer_g.step = d_wrapped, g_wrapped
    terms = trainer.train_step(mel_d.to(DEV, torch.float32), wav_d.to(DEV, torch.float32), list(MEL_LENGTHS))

    # the discriminator took train_repeat_discriminator = 2 Adam steps, each within its bound
    assert len(seen["d_steps"]) == 2 == trainer.discriminator_steps
    assert all(int(s["step"]) == 2 for s in trainer.optimizer_d.state.values()) and all(int(s["step"]) == 1 for s in trainer.optimizer_g.state.values())
    for step in range(2):
        for k in sd_d:
            _within(seen["d_steps"][step][k], d64[step][k], d32[step][k], f"D after discriminator step {step + 1}: {k}")
    # its loss never reached the generator: the fake was detached
    assert all(g is None for grads in seen["g_grads_at_d_step"] for g in grads)
    # the generator's step leaves the discriminator's parameters bit-identical, and never asked for their gradients
    assert not any(seen["d_requires_grad"]) and all(p.requires_grad for p in disc.parameters())
    for k, v in disc.state_dict().items():
        assert torch.equal(v, seen["d_at_g_step"][k]) and torch.equal(v, seen["d_steps"][1][k]), k
    for k in sd_g:
        _within(seen["g_grads"][k], gg64[k], gg32[k], f"G's clipped gradient at its step: {k}")
    for k in sd_g:
        _within(gen.state_dict()[k], g64[k], g32[k], f"G after its step: {k}")
        assert not torch.equal(gen.state_dict()[k], g_before[k]), f"{k} did not move"
    assert set(terms) == set(t64) and all(isinstance(v, float) for v in terms.values())
    for k in t64:
        _within(terms[k], t64[k], t32[k], f"loss term {k}")


def test_train_step_with_the_stft_loss_runs_on_uniform_rows():
    """The spectral term rides along: rows long enough for the STFT's reflection, no lengths."""
    from genvox_amd.losses import MultiResolutionSTFTLoss
    gen, disc = _models()
    trainer = MelGANTrainer(gen, disc, stft_loss=MultiResolutionSTFTLoss(resolutions=((512, 50, 240),)), stft_weight=2.5)
    mel = R.random_mel(G_CFG, 2, 40, 9).to(DEV, torch.float32)
    wav = DR.random_wav(2, 320, 10).to(DEV, torch.float32)
    before = [p.detach().clone() for p in gen.parameters()]
    terms = trainer.train_step(mel, wav)
    assert set(terms) == {"d_loss", "g_adv", "g_feat_match", "g_stft", "g_loss"}
    assert abs(terms["g_loss"] - (terms["g_adv"] + terms["g_feat_match"] + 2.5 * terms["g_stft"])) <= 1e-5 * abs(terms["g_loss"])
    assert all(torch.isfinite(p).all() and not torch.equal(p, b) for p, b in zip(gen.parameters(), before))
