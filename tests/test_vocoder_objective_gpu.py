"""GPU: the generator's whole objective, composed - vocode_with_grad of a generator (MelGAN or HiFi-GAN), MelGANDiscriminator on its
waveform, MelGANGeneratorLoss plus stft_weight x MultiResolutionSTFTLoss, backward() - against float64 autograd of the restatements
composed on the CPU (tests/melgan_ref64.py or tests/hifigan_ref64.py, tests/melgan_disc_ref64.py, tests/stft_loss_ref64.row_terms, the
two losses written out as tests/test_melgan_gan_gpu.restated_step has them), and MelGANTrainer.train_step with the spectral term.

Ragged rows of 40 and 33 frames at hop 8: 320 and 264 samples, the second just above the 257 that the 512-point transform's
reflection needs; mel_lengths, sample_lengths and map_lengths must agree across the three calls.  Everything behind a row's length,
in the mel and in the recording, is NaN.  The bound of every tensor is 8 x max(|float32 restatement - float64|, one ulp of its
largest value), a number of the restatements alone.

Ties.  The gradient tests run with w_mag = 0 (the log term takes a sign per bin) and on the first input seed of 1..8 for which, in
float64, no LeakyReLU pre-activation of the generator or feature of the discriminator lies within 8 x its float32 error of 0 (the
near_ties rule of the backward tests, with the composed chain's own float32 error), no |fake feature - real feature| of the feature
matching lies within 8 x the two features' errors of 0, and no STFT power lies within [eps / 2, 2 eps]."""
import functools

import pytest
import torch

from genvox_amd.configs import AudioConfig, HiFiGANConfig, MelGANConfig, MelGANDiscriminatorConfig
from genvox_amd.hifigan import HiFiGANGenerator
from genvox_amd.losses import MelGANGeneratorLoss, MultiResolutionSTFTLoss
from genvox_amd.melgan import MelGANGenerator
from genvox_amd.melgan_disc import MelGANDiscriminator
from genvox_amd.melgan_training import MelGANTrainer
from tests import hifigan_grad_ref64 as HG
from tests import hifigan_ref64 as HR
from tests import melgan_disc_ref64 as DR
from tests import melgan_grad_ref64 as MG
from tests import melgan_ref64 as MR
from tests import stft_loss_ref64 as SR
from tests import test_melgan_gan_gpu as GAN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
D_CFG = DR.TINY
RES = ((512, 50, 240),)
STFT_WEIGHT = 2.5
FEAT_MATCH = 10.0
MEL_LENGTHS = (40, 33)
KINDS = {"melgan": (MR, MG, MR.NARROW), "hifigan": (HR, HG, HR.NARROW)}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    yield
    print("composed objective, largest error / bound: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(WORST.items())))
    torch.cuda.empty_cache()


def _row_mean(rows):
    return sum(r.mean() for r in rows) / len(rows)


def objective(kind, sd_g, sd_d, mel, wav, dtype, w_mag):
    """The generator's loss in ``dtype``, every row alone at its own length -> dict(loss, g_stft, parts [B, R, 2], grads {name: d loss}
    with "mel" among the names, and what the tie rules read: the generator's tape, the discriminator's maps of fake and real, the
    spectra)."""
    ref, grad_ref, cfg = KINDS[kind]
    hop = ref.hop(cfg)
    pg = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_g.items()}
    pd = {k: v.to(dtype) for k, v in sd_d.items()}
    mels = [mel[b:b + 1, :, :t].to(dtype).clone().requires_grad_(True) for b, t in enumerate(MEL_LENGTHS)]
    taped = [grad_ref.generator_tape(pg, m, cfg) for m in mels]
    fake, tapes = [w for w, _ in taped], [t for _, t in taped]
    real = [wav[b:b + 1, :t * hop].to(dtype) for b, t in enumerate(MEL_LENGTHS)]
    d_real = [DR.discriminator(pd, r, D_CFG) for r in real]
    d_fake = [DR.discriminator(pd, f, D_CFG) for f in fake]
    n_scales, n_maps = D_CFG["n_scales"], D_CFG["n_layers"] + 3
    adv = sum(-_row_mean([m[k][-1] for m in d_fake]) for k in range(n_scales))
    weight = 4.0 / (D_CFG["n_layers"] + 1) / n_scales
    fm = FEAT_MATCH * sum(weight * _row_mean([(f[k][i] - r[k][i]).abs() for f, r in zip(d_fake, d_real)]) for k in range(n_scales) for i in range(n_maps - 1))
    B, R = len(fake), len(RES)
    parts, g_stft, spectra = torch.zeros(B, R, 2, dtype=dtype), 0.0, []
    for b, (f, r) in enumerate(zip(fake, real)):
        for j, res in enumerate(RES):
            sc, mag, _, _, Xp, Xt = SR.row_terms(f[0], r[0], res)
            g_stft = g_stft + (sc + w_mag * mag) / (B * R)
            parts[b, j, 0], parts[b, j, 1] = sc.detach(), mag.detach()
            spectra.append((Xp.detach(), Xt.detach()))
    loss = adv + fm + STFT_WEIGHT * g_stft
    loss.backward()
    grads = {k: v.grad for k, v in pg.items()}
    grads["mel"] = torch.zeros(mel.shape, dtype=dtype)
    for b, (m, t) in enumerate(zip(mels, MEL_LENGTHS)):
        grads["mel"][b, :, :t] = m.grad[0]
    detach = lambda rows: [[[x.detach() for x in ms] for ms in row] for row in rows]
    return dict(loss=loss.detach(), g_stft=g_stft.detach(), parts=parts, grads=grads, tapes=[[x.detach() for x in t] for t in tapes],
                d_fake=detach(d_fake), d_real=detach(d_real), spectra=spectra)


def ties(r64, r32):
    """How many decisions of the float64 objective the float32 one could take the other way (the module docstring's rules)."""
    err = lambda a, b: float((a.double() - b).abs().max())
    count = 0
    n_tape = len(r64["tapes"][0])
    for i in range(1, n_tape):   # entry 0 is the mel
        e = max(err(t32[i], t64[i]) for t32, t64 in zip(r32["tapes"], r64["tapes"]))
        count += sum(int((t64[i].abs() <= SR.FACTOR * e).sum()) for t64 in r64["tapes"])
    for k in range(D_CFG["n_scales"]):
        for i in range(D_CFG["n_layers"] + 2):   # every map but the score passes a LeakyReLU and enters the feature matching
            ef = max(err(a[k][i], b[k][i]) for a, b in zip(r32["d_fake"], r64["d_fake"]))
            er = max(err(a[k][i], b[k][i]) for a, b in zip(r32["d_real"], r64["d_real"]))
            for f, r in zip(r64["d_fake"], r64["d_real"]):
                count += int((f[k][i].abs() <= SR.FACTOR * ef).sum()) + int(((f[k][i] - r[k][i]).abs() <= SR.FACTOR * (ef + er)).sum())
    for Xp, Xt in r64["spectra"]:
        for X in (Xp, Xt):
            P = X.real * X.real + X.imag * X.imag
            count += int(((P >= SR.EPS / 2) & (P <= 2 * SR.EPS)).sum())
    return count


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(weights, mel, wav, float64 and float32 objective at w_mag = 0) of the first tie-free seed of 1..8: computed once, never changed."""
    ref, _, cfg = KINDS[kind]
    sd_g, sd_d = ref.random_state(cfg, 21), DR.random_state(D_CFG, 22)
    T = max(MEL_LENGTHS)
    for seed in range(1, 9):
        mel, wav = ref.random_mel(cfg, 2, T, seed), DR.random_wav(2, T * ref.hop(cfg), 100 + seed)
        r64, r32 = objective(kind, sd_g, sd_d, mel, wav, torch.float64, 0.0), objective(kind, sd_g, sd_d, mel, wav, torch.float32, 0.0)
        if ties(r64, r32) == 0:
            print(f"{kind}: input seed {seed} is tie-free")
            return sd_g, sd_d, mel, wav, r64, r32
    raise AssertionError(f"{kind}: no tie-free inputs among seeds 1 .. 8")


def _generator(kind, sd_g):
    ref, _, cfg = KINDS[kind]
    ac = AudioConfig(n_mels=12)
    ac.n_mels, ac.hop_length = cfg["n_mels"], ref.hop(cfg)   # below a preprocessing config's ranges: a test's size
    if kind == "melgan":
        model = MelGANGenerator(MelGANConfig(base_channels=cfg["base_channels"], upsample_ratios=cfg["ratios"], n_residual_layers=cfg["n_res"],
                                             dilation_base=cfg["dil_base"], leaky_slope=cfg["slope"]), ac)
    else:
        model = HiFiGANGenerator(HiFiGANConfig(upsample_initial_channel=cfg["c0"], upsample_rates=list(cfg["rates"]),
                                               upsample_kernel_sizes=[2 * r for r in cfg["rates"]], resblock=cfg["resblock"],
                                               resblock_kernel_sizes=list(cfg["kernels"]), resblock_dilation_sizes=[list(d) for d in cfg["dilations"]],
                                               leaky_slope=cfg["slope"], post_leaky_slope=cfg["post_slope"]), ac)
    model.load_state_dict({k: v.float() for k, v in sd_g.items()})
    return model.to(DEV)


def _discriminator(sd_d):
    disc = MelGANDiscriminator(MelGANDiscriminatorConfig(n_scales=D_CFG["n_scales"], base_channels=D_CFG["base_channels"], n_layers=D_CFG["n_layers"],
                                                         downsampling_factor=D_CFG["s"], max_channels=D_CFG["max_channels"], leaky_slope=D_CFG["slope"]))
    disc.load_state_dict({k: v.float() for k, v in sd_d.items()})
    return disc.to(DEV)


def _poisoned(mel, wav, hop):
    """float32 device copies with NaN at and behind every row's length."""
    mel, wav = mel.clone(), wav.clone()
    for b, t in enumerate(MEL_LENGTHS):
        mel[b, :, t:] = NAN
        wav[b, t * hop:] = NAN
    return mel.to(DEV, torch.float32), wav.to(DEV, torch.float32)


def _within(got, a64, a32, what, tensor):
    a64, a32 = torch.as_tensor(a64, dtype=torch.float64), torch.as_tensor(a32, dtype=torch.float64)
    err = (a32 - a64).abs().max().item()
    tol = SR.FACTOR * max(err, SR.ULP * a64.abs().max().item())
    d = (torch.as_tensor(got).detach().double().cpu() - a64).abs().max().item()
    WORST[tensor] = max(WORST.get(tensor, 0.0), d / tol)
    print(f"{what}: device error {d:.3e}, float32 restatement error {err:.3e}, bound {tol:.3e}, scale {a64.abs().max().item():.3e}: {d / tol:.3f} of the bound")
    assert d <= tol, f"{what}: {d:.3e} from float64, above the bound {tol:.3e}"


def _device_objective(kind, w_mag):
    """The chain on the device -> (generator, mel with its .grad, loss, the STFT criterion)."""
    ref, _, cfg = KINDS[kind]
    sd_g, sd_d, mel, wav = _case(kind)[:4]
    gen, disc = _generator(kind, sd_g), _discriminator(sd_d)
    mel_d, wav_d = _poisoned(mel, wav, ref.hop(cfg))
    mel_d.requires_grad_(True)
    lens = list(MEL_LENGTHS)
    sample_lengths = [t * gen.hop for t in lens]
    assert sample_lengths == [320, 264] and min(sample_lengths) >= RES[0][0] // 2 + 1
    fake = gen.vocode_with_grad(mel_d, lens)
    with torch.no_grad():
        real_maps = disc(wav_d, sample_lengths)
    g_crit, stft = MelGANGeneratorLoss(FEAT_MATCH), MultiResolutionSTFTLoss(RES, w_mag=w_mag)
    g_stft = stft(fake, wav_d, sample_lengths)
    loss = g_crit(real_maps, disc(fake, sample_lengths), disc.map_lengths(sample_lengths)) + STFT_WEIGHT * g_stft
    return gen, mel_d, loss, g_stft, stft


@pytest.mark.parametrize("kind", list(KINDS))
def test_gradients_of_the_composed_objective_against_float64(kind):
    """d_wav is the sum of the discriminators' input gradient and 2.5 x the STFT loss's: every generator parameter's .grad and
    mel.grad against float64 autograd of the composed restatement, the value too; mel.grad exactly 0 behind each row's frames."""
    r64, r32 = _case(kind)[4:]
    gen, mel_d, loss, g_stft, _ = _device_objective(kind, 0.0)
    loss.backward()
    torch.cuda.synchronize()
    _within(loss, r64["loss"], r32["loss"], f"{kind}: generator loss", f"{kind} loss")
    _within(g_stft, r64["g_stft"], r32["g_stft"], f"{kind}: g_stft (w_mag = 0)", f"{kind} g_stft")
    params = dict(gen.named_parameters())
    assert set(params) == set(r64["grads"]) - {"mel"}
    for k, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        _within(p.grad, r64["grads"][k], r32["grads"][k], f"{kind}: d {k}", f"{kind} parameter gradients")
    _within(mel_d.grad, r64["grads"]["mel"], r32["grads"]["mel"], f"{kind}: d mel", f"{kind} d_mel")
    for b, t in enumerate(MEL_LENGTHS):
        assert bool((mel_d.grad[b, :, t:] == 0).all()), f"row {b}: mel.grad behind the row's frames is not exact zeros"
        assert bool((mel_d.grad[b, :, :t] != 0).any())


@pytest.mark.parametrize("kind", list(KINDS))
def test_value_with_the_log_term_against_float64(kind):
    """The same forward with w_mag = 1: g_stft and last_parts.  A value has no tie problem."""
    sd_g, sd_d, mel, wav = _case(kind)[:4]
    r64, r32 = (objective(kind, sd_g, sd_d, mel, wav, dt, 1.0) for dt in (torch.float64, torch.float32))
    _, _, loss, g_stft, stft = _device_objective(kind, 1.0)
    assert stft.last_parts.shape == (2, len(RES), 2)
    _within(g_stft, r64["g_stft"], r32["g_stft"], f"{kind}: g_stft (w_mag = 1)", f"{kind} g_stft")
    _within(stft.last_parts, r64["parts"], r32["parts"], f"{kind}: last_parts", f"{kind} parts")
    _within(loss, r64["loss"], r32["loss"], f"{kind}: generator loss (w_mag = 1)", f"{kind} loss")


# ---- MelGANTrainer.train_step with the spectral term, on the ragged rows

@functools.lru_cache(maxsize=None)
def _step_case():
    """As tests/test_melgan_gan_gpu._case: the first seed whose generator step is well conditioned, here with the spectral term."""
    sd_g, sd_d = MR.random_state(GAN.G_CFG, 21), DR.random_state(D_CFG, 22)
    T = max(MEL_LENGTHS)
    for seed in range(1, 33):
        mel, wav = MR.random_mel(GAN.G_CFG, 2, T, seed), DR.random_wav(2, T * MR.hop(GAN.G_CFG), 100 + seed)
        r64, r32 = (GAN.restated_step(sd_g, sd_d, mel, wav, dt, MEL_LENGTHS, (RES, STFT_WEIGHT)) for dt in (torch.float64, torch.float32))
        if GAN.well_conditioned(sd_g, sd_d, r64, r32):
            print(f"input seed {seed} gives a well-conditioned step")
            return sd_g, sd_d, mel, wav, r64, r32
    raise AssertionError("no well-conditioned step among seeds 1 .. 32")


def test_train_step_with_the_stft_loss_on_ragged_rows_against_float64():
    """MelGANTrainer(stft_loss = one resolution with w_mag = 0, stft_weight = 2.5).train_step(mel, wav, [40, 33]): the discriminator's two
    steps, the generator's clipped gradients at its step, its post-step parameters and the five loss terms against the restated step."""
    assert GAN.D_CFG is D_CFG and GAN.G_CFG is MR.NARROW
    sd_g, sd_d, mel, wav, (g64, d64, t64, gg64), (g32, d32, t32, gg32) = _step_case()
    gen, disc = GAN._models(sd_g, sd_d)
    trainer = MelGANTrainer(gen, disc, stft_loss=MultiResolutionSTFTLoss(RES, w_mag=0.0), stft_weight=STFT_WEIGHT)
    mel_d, wav_d = _poisoned(mel, wav, MR.hop(GAN.G_CFG))
    seen = dict(d_steps=[])
    d_step, g_step = trainer.optimizer_d.step, trainer.optimizer_g.step

    def d_wrapped(*a, **kw):
        out = d_step(*a, **kw)
        seen["d_steps"].append({k: v.detach().clone() for k, v in disc.state_dict().items()})
        return out

    def g_wrapped(*a, **kw):
        seen["g_grads"] = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
        return g_step(*a, **kw)

    trainer.optimizer_d.step, trainer.optimizer_g.step = d_wrapped, g_wrapped
    g_before = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    terms = trainer.train_step(mel_d, wav_d, list(MEL_LENGTHS))
    assert len(seen["d_steps"]) == 2 == trainer.discriminator_steps
    for step in range(2):
        for k in sd_d:
            _within(seen["d_steps"][step][k], d64[step][k], d32[step][k], f"D after discriminator step {step + 1}: {k}", "step: D parameters")
    for k in sd_g:
        _within(seen["g_grads"][k], gg64[k], gg32[k], f"G's clipped gradient at its step: {k}", "step: G clipped gradients")
    for k in sd_g:
        _within(gen.state_dict()[k], g64[k], g32[k], f"G after its step: {k}", "step: G parameters")
        assert not torch.equal(gen.state_dict()[k], g_before[k]), f"{k} did not move"
    assert set(terms) == set(t64) == {"d_loss", "g_adv", "g_feat_match", "g_stft", "g_loss"} and all(isinstance(v, float) for v in terms.values())
    for k in t64:
        _within(terms[k], t64[k], t32[k], f"loss term {k}", "step: loss terms")
