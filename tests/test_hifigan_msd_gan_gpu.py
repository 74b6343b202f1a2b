"""GPU: one HiFiGANTrainer.train_step of a tiny HiFi-GAN generator (tests/hifigan_ref64.py's NARROW) against [TINY period
discriminators, TINY scale discriminators whose scale 0 is under spectral norm], B = 2 and ragged, with MelSpectrogramLoss as the
spectral term - the published step at a test's size - against a restatement of the same step: tests/hifigan_ref64.py for G,
tests/hifigan_disc_ref64.py and tests/hifigan_msd_ref64.py for the discriminators, tests/mel_loss_ref64.py for the spectral term, the
least-squares losses written out, torch's AdamW on float64 leaves.  The scale discriminators are in training mode, so each of their
four forwards of the step (real and fake for D's step, real and fake for G's) does one power iteration first, and sigma is in the graph
of D's step.  The bound of every post-step parameter tensor, of every gradient, of u and v after the step and of every loss term is
8 x max(|float32 restatement of the step - float64|, one ulp of the value), as everywhere in these tests.

Conditioning, hyper-parameters and the choice of the input seed on the reference alone are those of tests/test_hifigan_gan_gpu.py, which
has the account; its helpers are imported.

The second test writes the published checkpoint layout {"mpd": ..., "msd": ...} from random weights - weight-normalised pairs for the
period discriminators and the pooled scales, spectral triples for scale 0 - and loads the file into the pair."""
import functools

import pytest
import torch

from genvox_amd.configs import HiFiGANPeriodDiscriminatorConfig, HiFiGANScaleDiscriminatorConfig, HiFiGANTrainingConfig
from genvox_amd.hifigan_disc import HiFiGANPeriodDiscriminator
from genvox_amd.hifigan_msd import HiFiGANScaleDiscriminator
from genvox_amd.hifigan_training import HiFiGANTrainer
from genvox_amd.losses import MelSpectrogramLoss
from tests import hifigan_disc_ref64 as DR
from tests import hifigan_msd_ref64 as SC
from tests import hifigan_ref64 as R
from tests import mel_loss_ref64 as ML
from tests.test_hifigan_gan_gpu import (ADAM_EPS, D_GAIN, DEV, G_CFG, HP, MEL_LENGTHS, NAN, P_CFG, _d_state, _models, _row_mean, _within,
                                        well_conditioned)

pytestmark = pytest.mark.gpu

S_CFG = SC.TINY
MEL = dict(sampling_rate=8000, n_fft=512, hop_length=64, win_length=512, n_mels=12)   # rows of 320 and 272 samples: 5 and 4 frames


def _mel_cfg():
    return ML.Config(MEL["n_fft"], MEL["hop_length"], MEL["win_length"], ML.slaney(MEL["sampling_rate"], MEL["n_fft"], MEL["n_mels"]))


def _msd_config():
    return HiFiGANScaleDiscriminatorConfig(n_scales=S_CFG["n_scales"], channels=S_CFG["channels"], kernel_sizes=S_CFG["kernel_sizes"],
                                           strides=S_CFG["strides"], groups=S_CFG["groups"], spectral_norm_scales=(0,), leaky_slope=S_CFG["slope"])


def restated_step(sd_g, sd_d, buffers, mel, wav, dtype):
    """HiFiGANTrainer.train_step in ``dtype`` -> (post-step G, post-step D, terms, G's gradients, D's gradients, u and v after the step)."""
    pg = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_g.items()}
    pd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd_d.items()}
    uv = {k: v.to(dtype).clone() for k, v in buffers.items()}
    adam = dict(lr=HP["learning_rate"], betas=(HP["adam_b1"], HP["adam_b2"]), weight_decay=HP["weight_decay"])
    opt_g, opt_d = torch.optim.AdamW(list(pg.values()), **adam), torch.optim.AdamW(list(pd.values()), **adam)
    hop, mel_cfg = R.hop(G_CFG), _mel_cfg()

    def discriminate(x):
        """One forward of both discriminators on the rows x -> [row][sub-discriminator][map]; the spectral layers iterate once."""
        msd = {}
        for k, v in pd.items():
            if not k.startswith("1."):
                continue
            if k.endswith(".weight_orig"):
                prefix = k[:-len(".weight_orig")]
                w, uv[prefix + ".weight_u"], uv[prefix + ".weight_v"] = SC.spectral_weight(v, uv[prefix + ".weight_u"], uv[prefix + ".weight_v"], training=True)
                msd[prefix[2:] + ".weight"] = w
            else:
                msd[k[2:]] = v
        mpd = {k[2:]: v for k, v in pd.items() if k.startswith("0.")}
        return [DR.discriminator(mpd, row, P_CFG) + SC.discriminator(msd, row, S_CFG) for row in x]

    fake = [R.generator(pg, mel[b:b + 1, :, :t].to(dtype), G_CFG)[0] for b, t in enumerate(MEL_LENGTHS)]
    real = [wav[b:b + 1, :t * hop].to(dtype) for b, t in enumerate(MEL_LENGTHS)]
    opt_d.zero_grad()
    d_real, d_fake = discriminate(real), discriminate([f.detach() for f in fake])
    n_sub = len(d_real[0])
    d_loss = sum(_row_mean([(1 - m[k][-1]) ** 2 for m in d_real]) + _row_mean([m[k][-1] ** 2 for m in d_fake]) for k in range(n_sub))
    d_loss.backward()
    assert all(p.grad is None for p in pg.values())
    d_grads = {k: v.grad.detach().clone() for k, v in pd.items()}
    opt_d.step()
    d_after = {k: v.detach().clone() for k, v in pd.items()}
    opt_g.zero_grad()
    with torch.no_grad():
        d_real = discriminate(real)
    d_fake = discriminate(fake)
    adv = sum(_row_mean([(1 - m[k][-1]) ** 2 for m in d_fake]) for k in range(n_sub))
    fm = HP["feat_match"] * sum(_row_mean([(f[k][i] - r[k][i]).abs() for f, r in zip(d_fake, d_real)]) for k in range(n_sub) for i in range(len(d_fake[0][k])))
    g_aux = sum((ML.mel(r[0], mel_cfg)[1] - ML.mel(f[0], mel_cfg)[1]).abs().mean() for f, r in zip(fake, real)) / len(fake)
    g_loss = adv + fm + HP["aux_weight"] * g_aux
    terms = dict(d_loss=d_loss.item(), g_adv=adv.item(), g_feat_match=fm.item(), g_aux=g_aux.item())
    for p in pd.values():
        p.grad = None
    g_loss.backward(inputs=list(pg.values()))
    g_grads = {k: v.grad.detach().clone() for k, v in pg.items()}
    opt_g.step()
    terms["g_loss"] = g_loss.item()
    return {k: v.detach() for k, v in pg.items()}, d_after, terms, g_grads, d_grads, uv


def _start_state():
    """Random weights of both sides; the scale discriminators' keys are the module's own (weight_orig, weight_u, weight_v on scale 0)."""
    sd_g = R.random_state(G_CFG, 21)
    sd_d = {"0." + k: v for k, v in DR.random_state(P_CFG, 22, D_GAIN).items()}
    buffers = {}
    g = torch.Generator().manual_seed(24)
    for k, v in SC.random_state(S_CFG, 23, D_GAIN).items():
        if k.startswith("discriminators.0.") and k.endswith(".weight"):
            sd_d["1." + k + "_orig"] = v
            buffers["1." + k + "_u"] = torch.nn.functional.normalize(torch.randn(v.shape[0], generator=g, dtype=torch.float64), dim=0)
            buffers["1." + k + "_v"] = torch.nn.functional.normalize(torch.randn(v.shape[1] * v.shape[2], generator=g, dtype=torch.float64), dim=0)
        else:
            sd_d["1." + k] = v
    return sd_g, sd_d, buffers


@functools.lru_cache(maxsize=None)
def _case():
    """(weights, inputs, float64 and float32 restatement) of the first well-conditioned seed: computed once, never changed."""
    sd_g, sd_d, buffers = _start_state()
    for seed in range(1, 33):
        mel = R.random_mel(G_CFG, 2, max(MEL_LENGTHS), seed)
        wav = DR.random_wav(2, max(MEL_LENGTHS) * R.hop(G_CFG), 100 + seed)
        r64 = restated_step(sd_g, sd_d, buffers, mel, wav, torch.float64)
        r32 = restated_step(sd_g, sd_d, buffers, mel, wav, torch.float32)
        if well_conditioned(r64, r32):
            print(f"input seed {seed} gives a well-conditioned step")
            return sd_g, sd_d, buffers, mel, wav, r64, r32
    raise AssertionError("no well-conditioned step among seeds 1 .. 32")


def _pair(sd_g, sd_d, buffers):
    gen, discs = _models(sd_g, sd_d, False)   # the generator and the period discriminators
    msd = HiFiGANScaleDiscriminator(_msd_config())
    msd.load_state_dict({k[2:]: v.float() for k, v in list(sd_d.items()) + list(buffers.items()) if k.startswith("1.")})
    return gen, discs + [msd.to(DEV)]


def test_one_published_train_step_against_float64():
    sd_g, sd_d, buffers, mel, wav, r64, r32 = _case()
    (g64, d64, t64, gg64, dg64, uv64), (g32, d32, t32, gg32, dg32, uv32) = r64, r32
    gen, discs = _pair(sd_g, sd_d, buffers)
    assert discs[1].training and isinstance(discs[0], HiFiGANPeriodDiscriminator)
    trainer = HiFiGANTrainer(gen, discs, HiFiGANTrainingConfig(**HP), aux_loss=MelSpectrogramLoss(**MEL))
    assert trainer.optimizer_d.defaults["eps"] == ADAM_EPS
    mel_d, wav_d = mel.clone(), wav.clone()
    for b, t in enumerate(MEL_LENGTHS):   # whatever lies behind a row's length is never read
        mel_d[b, :, t:] = NAN
        wav_d[b, t * R.hop(G_CFG):] = NAN
    g_before = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    seen = {}
    d_step, g_step = trainer.optimizer_d.step, trainer.optimizer_g.step

    def d_wrapped(*a, **kw):
        seen["g_grads_at_d_step"] = [p.grad for p in gen.parameters()]
        seen["d_grads"] = {f"{i}.{k}": p.grad.detach().clone() for i, D in enumerate(discs) for k, p in D.named_parameters()}
        out = d_step(*a, **kw)
        seen["d_after"] = {f"{i}.{k}": p.detach().clone() for i, D in enumerate(discs) for k, p in D.named_parameters()}
        return out

    def g_wrapped(*a, **kw):
        seen["d_requires_grad"] = [p.requires_grad for D in discs for p in D.parameters()]
        seen["g_grads"] = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
        return g_step(*a, **kw)

    trainer.optimizer_d.step, trainer.optimizer_g.step = d_wrapped, g_wrapped
    terms = trainer.train_step(mel_d.to(DEV, torch.float32), wav_d.to(DEV, torch.float32), list(MEL_LENGTHS))
    worst = []
    assert set(seen["d_grads"]) == set(sd_d)
    for k in sd_d:
        _within(seen["d_grads"][k], dg64[k], dg32[k], f"D's gradient at its step: {k}", worst)
        dead = (dg64[k] == 0) & (dg32[k] == 0)
        assert not seen["d_grads"][k].cpu()[dead].any(), f"{k}: a gradient that no data reaches is not exactly 0"
    for k in sd_d:
        _within(seen["d_after"][k], d64[k], d32[k], f"D after its step: {k}", worst)
    assert all(g is None for g in seen["g_grads_at_d_step"]), "the discriminators' loss reached the generator"
    # the generator's step leaves the discriminators' parameters bit-identical, and never asked for their gradients
    assert not any(seen["d_requires_grad"]) and all(p.requires_grad for D in discs for p in D.parameters())
    now = _d_state(discs)
    for k, v in seen["d_after"].items():
        assert torch.equal(v, now[k]), k
    for k in buffers:   # four power iterations
        _within(now[k], uv64[k], uv32[k], f"after the step: {k}", worst)
    for k in sd_g:
        _within(seen["g_grads"][k], gg64[k], gg32[k], f"G's gradient at its step: {k}", worst)
    for k in sd_g:
        _within(gen.state_dict()[k], g64[k], g32[k], f"G after its step: {k}", worst)
        assert not torch.equal(gen.state_dict()[k], g_before[k]), f"{k} did not move"
    assert set(terms) == set(t64) and all(isinstance(v, float) for v in terms.values())
    for k in t64:
        _within(terms[k], t64[k], t32[k], f"loss term {k}", worst)
    print(f"the published step: largest error {max(worst):.3f} of its bound")


def test_the_published_checkpoint_file_loads_into_the_pair(tmp_path):
    g = torch.Generator().manual_seed(9)
    mpd_sd, msd_sd, want = {}, {}, {}
    for k, v in DR.random_state(P_CFG, 31).items():
        if k.endswith(".weight"):
            v = v.float()
            gain = torch.rand(v.shape[0], 1, 1, 1, generator=g) + 0.5
            mpd_sd[k + "_g"], mpd_sd[k + "_v"] = gain, v
            want["mpd." + k] = v * (gain / torch.linalg.vector_norm(v.reshape(v.shape[0], -1), dim=1).reshape(-1, 1, 1, 1))
        else:
            mpd_sd[k] = want["mpd." + k] = v.float()
    for k, v in SC.random_state(S_CFG, 32).items():
        v = v.float()
        if k.endswith(".weight") and k.startswith("discriminators.0."):
            msd_sd[k + "_orig"] = want["msd." + k + "_orig"] = v
            msd_sd[k + "_u"] = want["msd." + k + "_u"] = torch.nn.functional.normalize(torch.randn(v.shape[0], generator=g), dim=0)
            msd_sd[k + "_v"] = want["msd." + k + "_v"] = torch.nn.functional.normalize(torch.randn(v.shape[1] * v.shape[2], generator=g), dim=0)
        elif k.endswith(".weight"):
            gain = torch.rand(v.shape[0], 1, 1, generator=g) + 0.5
            msd_sd[k + "_g"], msd_sd[k + "_v"] = gain, v
            want["msd." + k] = v * (gain / torch.linalg.vector_norm(v.reshape(v.shape[0], -1), dim=1).reshape(-1, 1, 1))
        else:
            msd_sd[k] = want["msd." + k] = v
    path = tmp_path / "do_00000001"
    torch.save({"mpd": mpd_sd, "msd": msd_sd, "optim_g": {}, "optim_d": {}, "steps": 1, "epoch": 0}, path)
    loaded = torch.load(path)
    mpd = HiFiGANPeriodDiscriminator(HiFiGANPeriodDiscriminatorConfig(periods=P_CFG["periods"], channels=P_CFG["channels"], kernel_size=P_CFG["kernel_size"],
                                                                       stride=P_CFG["stride"], leaky_slope=P_CFG["slope"]))
    msd = HiFiGANScaleDiscriminator(_msd_config())
    mpd.load_state_dict(loaded)
    msd.load_state_dict(loaded)
    got = {"mpd." + k: v for k, v in mpd.state_dict().items()}
    got.update({"msd." + k: v for k, v in msd.state_dict().items()})
    assert set(got) == set(want)
    for k, v in want.items():
        torch.testing.assert_close(got[k], v, rtol=1e-6, atol=0.0, msg=k)
    wav = DR.random_wav(2, 100, 1).to(DEV, torch.float32)
    with torch.no_grad():
        maps = mpd.to(DEV)(wav) + msd.to(DEV).eval()(wav)
    assert len(maps) == len(P_CFG["periods"]) + S_CFG["n_scales"] and all(torch.isfinite(m).all() for sub in maps for m in sub)
