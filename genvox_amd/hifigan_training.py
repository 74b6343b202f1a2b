"""One GAN step of HiFi-GAN: the generator against the multi-period and the multi-scale discriminator - or any other list of
discriminators - all on the device's own kernels.  The published step:

    trainer = HiFiGANTrainer(generator, [HiFiGANPeriodDiscriminator(), HiFiGANScaleDiscriminator()], aux_loss=MelSpectrogramLoss())
    terms = trainer.train_step(mel, wav, mel_lengths)     # {"d_loss": ..., "g_adv": ..., "g_feat_match": ..., "g_aux": ..., "g_loss": ...}
    trainer.end_epoch()                                   # both learning rates times lr_decay

It is a step, not a loop: data loading, checkpoint rotation and logging belong to the caller.  A discriminator is any module that
offers ``forward(wav, sample_lengths)`` -> [sub-discriminator][map] and ``map_lengths(sample_lengths)``.  The spectral term is
``aux_loss(fake, wav, sample_lengths)``, weighted ``aux_weight``: with ``losses.MelSpectrogramLoss()`` - HiFi-GAN's mel-spectrogram L1
term - the default ``aux_weight`` of 45 carries its published meaning (``MultiResolutionSTFTLoss`` fits the same slot, on another scale).
``HiFiGANScaleDiscriminator`` in training mode does one power iteration of its spectral scale per forward, four per step, as the
published recipe does; ``MelGANDiscriminator`` fits the same list, and so does ``MultiResolutionDiscriminator`` (UnivNet's spectrogram
discriminator, which the published BigVGAN recipe trains with in place of the multi-scale one): its maps are [B, C, W, F] with the
frames, the ragged axis, on dim 2, where the period discriminators have their heights."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .configs import HiFiGANTrainingConfig
from .losses import HiFiGANDiscriminatorLoss, HiFiGANGeneratorLoss


class HiFiGANTrainer:
    def __init__(self, generator: torch.nn.Module, discriminators: Sequence[torch.nn.Module], training_config: Optional[HiFiGANTrainingConfig] = None,
                 aux_loss: Optional[torch.nn.Module] = None) -> None:
        if isinstance(discriminators, torch.nn.Module):
            discriminators = [discriminators]
        if not len(discriminators):
            raise ValueError("HiFiGANTrainer needs at least one discriminator")
        for D in discriminators:
            if not hasattr(D, "map_lengths"):
                raise ValueError(f"{type(D).__name__} offers no map_lengths(sample_lengths)")
        tc = training_config if training_config is not None else HiFiGANTrainingConfig()
        self.generator, self.discriminators, self.training_config, self.aux_loss = generator, list(discriminators), tc, aux_loss
        adam = dict(lr=tc.learning_rate, betas=(tc.adam_b1, tc.adam_b2), weight_decay=tc.weight_decay)
        self.optimizer_g = torch.optim.AdamW(generator.parameters(), **adam)
        self.optimizer_d = torch.optim.AdamW([p for D in self.discriminators for p in D.parameters()], **adam)
        self.d_criterion = HiFiGANDiscriminatorLoss()
        self.g_criterion = HiFiGANGeneratorLoss(tc.feat_match)
        self.steps = 0
        self.epochs = 0

    def _d_parameters(self):
        return [p for D in self.discriminators for p in D.parameters()]

    def end_epoch(self) -> None:
        """The published ExponentialLR: both learning rates times ``lr_decay``."""
        for opt in (self.optimizer_g, self.optimizer_d):
            for group in opt.param_groups:
                group["lr"] = group["lr"] * self.training_config.lr_decay
        self.epochs += 1

    def _clip(self, params) -> None:
        if self.training_config.grad_clip_thresh and self.training_config.grad_clip_thresh > 0.0:
            torch.nn.utils.clip_grad_norm_(params, self.training_config.grad_clip_thresh)

    def train_step(self, mel: torch.Tensor, wav: torch.Tensor, mel_lengths=None) -> Dict[str, float]:
        """mel float32 [B, n_mels, T] and the recordings wav float32 [B, T * hop] on the device; ``mel_lengths`` ([B], host) for ragged
        rows, row b then counting the samples the generator delivers for ``mel_lengths[b]`` frames (``G.sample_counts``; ``* hop`` where
        the generator has none).  A generator whose full rows deliver fewer than ``T * hop`` samples (Vocos with "center" padding) gets
        those counts without ``mel_lengths`` too: the discriminators and the spectral term would otherwise set a hop of recording against
        a hop of zeros.  The discriminators take one optimizer step together, then the generator takes one; the loss terms come back as
        floats."""
        G, tc = self.generator, self.training_config
        counts = getattr(G, "sample_counts", None) or (lambda frames: [int(t) * G.hop for t in frames])
        sample_lengths = map_lengths = None
        T = int(mel.shape[2])
        if mel_lengths is not None:
            host = [int(v) for v in (mel_lengths.tolist() if isinstance(mel_lengths, torch.Tensor) else mel_lengths)]
            sample_lengths = [int(n) for n in counts(host)]
        elif int(counts([T])[0]) != T * G.hop:
            sample_lengths = [int(counts([T])[0])] * int(mel.shape[0])
        if sample_lengths is not None:
            map_lengths = [D.map_lengths(sample_lengths) for D in self.discriminators]
        fake = G.vocode_with_grad(mel, mel_lengths)

        # the discriminators' step: the fake is detached, so nothing of it reaches the generator
        fake_d = fake.detach()
        self.optimizer_d.zero_grad(set_to_none=True)
        d_loss = self.d_criterion([D(wav, sample_lengths) for D in self.discriminators], [D(fake_d, sample_lengths) for D in self.discriminators], map_lengths)
        d_loss.backward()
        self._clip(self._d_parameters())
        self.optimizer_d.step()

        # the generator's step: through the discriminators' input gradients only - their parameters ask for none
        d_params = self._d_parameters()
        flags = [p.requires_grad for p in d_params]
        for p in d_params:
            p.requires_grad_(False)
        try:
            self.optimizer_g.zero_grad(set_to_none=True)
            with torch.no_grad():
                real_maps = [D(wav, sample_lengths) for D in self.discriminators]
            g_loss = self.g_criterion(real_maps, [D(fake, sample_lengths) for D in self.discriminators], map_lengths)
            g_adv, g_fm = self.g_criterion.last_terms
            terms = {"d_loss": d_loss.detach().item(), "g_adv": g_adv.detach().item(), "g_feat_match": g_fm.detach().item()}
            if self.aux_loss is not None:
                g_aux = self.aux_loss(fake, wav, sample_lengths)
                g_loss = g_loss + tc.aux_weight * g_aux
                terms["g_aux"] = g_aux.detach().item()
            g_loss.backward()
            self._clip(G.parameters())
            self.optimizer_g.step()
        finally:
            for p, flag in zip(d_params, flags):
                p.requires_grad_(flag)
        terms["g_loss"] = g_loss.detach().item()
        self.steps += 1
        return terms
