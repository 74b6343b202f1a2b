"""GPU: the multi-resolution spectrogram discriminator in the GAN step.  One HiFiGANTrainer.train_step of a tiny HiFi-GAN generator
(tests/hifigan_ref64.py's NARROW) against [HiFiGANPeriodDiscriminator(), MultiResolutionDiscriminator()] - the pair the published
BigVGAN recipe trains with, both at their published sizes - with MelSpectrogramLoss() as the spectral term, B = 2 and ragged: every
loss term is finite and every parameter of the generator and of both discriminators changes.  The autograd node's rules - torch's
version error for an in-place change of a parameter or of a returned map between forward and backward, a new blob after every change of
the parameters - as tests/test_hifigan_msd_autograd_gpu.py has them for the scale discriminators.  And the least-squares losses over the
device's maps with ``map_lengths`` against the per-row means of the float64 restatement, written out: the bound of a term is
8 x max(|float32 restatement - float64|, one ulp of the value), as everywhere in these tests."""
import pytest
import torch

from genvox_amd.configs import AudioConfig, HiFiGANConfig, MultiResolutionDiscriminatorConfig
from genvox_amd.hifigan import HiFiGANGenerator
from genvox_amd.hifigan_disc import HiFiGANPeriodDiscriminator
from genvox_amd.hifigan_training import HiFiGANTrainer
from genvox_amd.losses import HiFiGANDiscriminatorLoss, HiFiGANGeneratorLoss, MelSpectrogramLoss
from genvox_amd.mrd import MultiResolutionDiscriminator
from tests import hifigan_ref64 as R
from tests import mrd_ref64 as MR
from tests.test_mrd_gpu import DEV, NAN, _net, _poisoned

pytestmark = pytest.mark.gpu

G_CFG = R.NARROW
MEL_LENGTHS = (160, 120)   # 1280 and 960 samples at hop 8: the widest reflection of the default resolutions needs 905


def _generator():
    ac = AudioConfig()
    ac.n_mels, ac.hop_length = G_CFG["n_mels"], R.hop(G_CFG)   # below a preprocessing config's ranges: a test's size
    gen = HiFiGANGenerator(HiFiGANConfig(upsample_initial_channel=G_CFG["c0"], upsample_rates=list(G_CFG["rates"]),
                                         upsample_kernel_sizes=[2 * r for r in G_CFG["rates"]], resblock=G_CFG["resblock"],
                                         resblock_kernel_sizes=list(G_CFG["kernels"]), resblock_dilation_sizes=[list(d) for d in G_CFG["dilations"]],
                                         leaky_slope=G_CFG["slope"], post_leaky_slope=G_CFG["post_slope"]), ac)
    gen.load_state_dict({k: v.float() for k, v in R.random_state(G_CFG, 21).items()})
    return gen.to(DEV)


def _module(name):
    cfg, sd, net = _net(name)
    model = MultiResolutionDiscriminator(MultiResolutionDiscriminatorConfig(resolutions=cfg["resolutions"], channels=cfg["channels"],
                                                                           leaky_slope=cfg["slope"], window=cfg["window"]))
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    return cfg, sd, model.to(DEV)


def test_one_train_step_with_the_published_pair():
    torch.manual_seed(3)
    gen = _generator()
    discs = [HiFiGANPeriodDiscriminator().to(DEV), MultiResolutionDiscriminator().to(DEV)]
    trainer = HiFiGANTrainer(gen, discs, aux_loss=MelSpectrogramLoss())
    hop, T = R.hop(G_CFG), max(MEL_LENGTHS)
    mel, wav = R.random_mel(G_CFG, 2, T, 1), MR.random_wav(2, T * hop, 2)
    for b, t in enumerate(MEL_LENGTHS):   # whatever lies behind a row's length is never read
        mel[b, :, t:] = NAN
        wav[b, t * hop:] = NAN
    before = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in [gen] + discs]
    terms = trainer.train_step(mel.to(DEV, torch.float32), wav.to(DEV, torch.float32), list(MEL_LENGTHS))
    assert set(terms) == {"d_loss", "g_adv", "g_feat_match", "g_aux", "g_loss"}
    for k, v in terms.items():
        assert isinstance(v, float) and v == v and abs(v) < float("inf"), f"loss term {k} = {v}"
    print(terms)
    for m, old in zip([gen] + discs, before):
        for k, v in m.state_dict().items():
            assert torch.isfinite(v).all(), f"{type(m).__name__}: {k} is not finite after the step"
            assert not torch.equal(v, old[k]), f"{type(m).__name__}: {k} did not move"
    assert all(p.requires_grad for D in discs for p in D.parameters())


def test_module_refuses_in_place_changes_and_packs_again():
    cfg, sd, model = _module("HANN")
    wav = MR.random_wav(2, 905, 1).to(DEV, torch.float32)
    with pytest.raises(ValueError, match="row 1"):
        model(wav, [905, 224])
    with pytest.raises(ValueError, match="row 0"):
        model(wav, [906, 300])
    out = model(wav)
    with torch.no_grad():
        model.discriminators[0].conv_post.weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out[0][-1].sum().backward()
    # a parameter that changed is packed again: the next forward sees it
    after = model(wav)
    assert not torch.equal(after[0][-1], out[0][-1]) and torch.equal(after[0][0], out[0][0])
    # the returned maps are the backward's tape: one changed in place raises too, whichever map the loss hangs on
    with pytest.raises(RuntimeError, match="inplace"):   # torch refuses at the operation or, at the latest, at the backward
        after[0][-1].clamp_(min=0.0)
        after[0][0].sum().backward()
    # two forwards before one backward (the discriminators' step): each node keeps the weights and the tape it ran on
    xa, xb = wav.clone().requires_grad_(True), (0.5 * wav).requires_grad_(True)
    oa, ob = model(xa), model(xb)
    (sum(m.sum() for m in oa[0]) + sum((m * m).sum() for m in ob[0])).backward()
    ya, yb = wav.clone().requires_grad_(True), (0.5 * wav).requires_grad_(True)
    sum(m.sum() for m in model(ya)[0]).backward()
    sum((m * m).sum() for m in model(yb)[0]).backward()
    assert torch.equal(xa.grad, ya.grad) and torch.equal(xb.grad, yb.grad)
    # .to() moves every tensor: packed again, the same bits
    with torch.no_grad():
        here = model(wav)
        model.to("cpu")
        with pytest.raises(RuntimeError, match="MI355X"):
            model(wav)
        model.to(DEV)
        moved = model(wav)
    assert all(torch.equal(x, y) for x, y in zip(here[0], moved[0]))
    # an optimizer step changes every parameter in place, a reload replaces them: the blob is rebuilt each time
    model.zero_grad()
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    model(wav)[0][-1].sum().backward()
    opt.step()
    stepped = model(wav)
    fresh = MultiResolutionDiscriminator(model.model_config)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(DEV)
    with torch.no_grad():
        want = fresh(wav)
    assert not torch.equal(stepped[0][-1], moved[0][-1])
    assert all(torch.equal(x, y) for x, y in zip(stepped[0], want[0]))
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    with torch.no_grad():
        reloaded = model(wav)
    assert all(torch.equal(x, y) for x, y in zip(reloaded[0], out[0])) and not torch.equal(reloaded[0][-1], stepped[0][-1])


def _restated_losses(sd, cfg, real, fake, lens, feat_match, dtype):
    """The least-squares losses over the restatement's maps in ``dtype``: every mean a mean per row over the row's own C x W_b x F
    elements, then over rows."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    r, _, _ = MR.run(sd, real.to(dtype), lens, cfg, dtype=dtype)
    f, _, _ = MR.run(sd, fake.to(dtype), lens, cfg, dtype=dtype)

    def row_mean(fn, j, i):
        return sum(fn(r[j][i][b, :, :MR.map_widths(cfg, nb)[j][i]], f[j][i][b, :, :MR.map_widths(cfg, nb)[j][i]]).mean() for b, nb in enumerate(lens)) / len(lens)

    subs = range(len(cfg["resolutions"]))
    d_loss = sum(row_mean(lambda a, b: (1 - a) ** 2, j, -1) + row_mean(lambda a, b: b ** 2, j, -1) for j in subs)
    adv = sum(row_mean(lambda a, b: (1 - b) ** 2, j, -1) for j in subs)
    fm = feat_match * sum(row_mean(lambda a, b: (b - a).abs(), j, i) for j in subs for i in range(MR.MAPS))
    return dict(d_loss=d_loss.item(), g_adv=adv.item(), g_feat_match=fm.item())


@pytest.mark.parametrize("name", ["DEFAULT", "HANN"])
def test_the_losses_with_map_lengths_are_the_restatements_row_means(name):
    cfg, sd, model = _module(name)
    lens = (1650, MR.min_samples(cfg))
    real, fake = MR.random_wav(2, lens[0], 5), MR.random_wav(2, lens[0], 6)
    t64 = _restated_losses(sd, cfg, real, fake, lens, 2.0, torch.float64)
    t32 = _restated_losses(sd, cfg, real, fake, lens, 2.0, torch.float32)
    with torch.no_grad():
        r, f = model(_poisoned(real, lens), list(lens)), model(_poisoned(fake, lens), list(lens))
        ml = model.map_lengths(lens)
        g_crit = HiFiGANGeneratorLoss(2.0)
        got = dict(d_loss=HiFiGANDiscriminatorLoss()(r, f, ml).item())
        g_crit(r, f, ml)
        got["g_adv"], got["g_feat_match"] = g_crit.last_terms[0].item(), g_crit.last_terms[1].item()
    for k in t64:
        tol = MR.FACTOR * max(abs(t32[k] - t64[k]), MR.ULP * abs(t64[k]))
        print(f"{name} {k}: {got[k]:.9g} against {t64[k]:.9g}, bound {tol:.3e}")
        assert abs(got[k] - t64[k]) <= tol, f"{name}: {k} is {abs(got[k] - t64[k]):.3e} from float64, above the bound {tol:.3e}"
