"""One GAN step of the neural vocoder: MelGAN generator against its multi-scale discriminator, both on the device's own kernels.

    trainer = MelGANTrainer(generator, discriminator, stft_loss=MultiResolutionSTFTLoss(), stft_weight=1.0)
    terms = trainer.train_step(mel, wav, mel_lengths)     # {"d_loss": ..., "g_adv": ..., "g_feat_match": ..., "g_stft": ..., "g_loss": ...}

It is a step, not a loop: data loading, checkpoint rotation and logging belong to the caller.  The generator config's training fields
are read here: ``learning_rate``, ``beta1``, ``beta2`` and ``weight_decay`` make the two Adam optimizers, ``grad_clip_thresh`` clips
both, ``train_repeat_discriminator`` repeats the discriminator's step and ``feat_match`` weighs the feature-matching term."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .losses import MelGANDiscriminatorLoss, MelGANGeneratorLoss
from .melgan import MelGANGenerator
from .melgan_disc import MelGANDiscriminator


class MelGANTrainer:
    def __init__(self, generator: MelGANGenerator, discriminator: MelGANDiscriminator, stft_loss: Optional[torch.nn.Module] = None,
                 stft_weight: float = 0.0) -> None:
        mc = generator.model_config
        self.generator, self.discriminator = generator, discriminator
        self.stft_loss, self.stft_weight = stft_loss, float(stft_weight)
        adam = dict(lr=mc.learning_rate, betas=(mc.beta1, mc.beta2), weight_decay=mc.weight_decay)
        self.optimizer_g = torch.optim.Adam(generator.parameters(), **adam)
        self.optimizer_d = torch.optim.Adam(discriminator.parameters(), **adam)
        self.d_criterion = MelGANDiscriminatorLoss()
        self.g_criterion = MelGANGeneratorLoss(mc.feat_match)
        self.discriminator_steps = 0

    def train_step(self, mel: torch.Tensor, wav: torch.Tensor, mel_lengths=None) -> Dict[str, float]:
        """mel float32 [B, n_mels, T] and the recordings wav float32 [B, T * hop] on the device; ``mel_lengths`` ([B], host) for ragged
        rows, row b then counting ``mel_lengths[b] * hop`` samples.  Both models take one optimizer step (the discriminator
        ``train_repeat_discriminator`` of them); the loss terms come back as floats."""
        G, D, mc = self.generator, self.discriminator, self.generator.model_config
        sample_lengths = map_lengths = None
        if mel_lengths is not None:
            host = [int(v) for v in (mel_lengths.tolist() if isinstance(mel_lengths, torch.Tensor) else mel_lengths)]
            sample_lengths = [t * G.hop for t in host]
            map_lengths = D.map_lengths(sample_lengths)
        fake = G.vocode_with_grad(mel, mel_lengths)

        # the discriminator's step: the fake is detached, so nothing of it reaches the generator
        fake_d = fake.detach()
        for _ in range(mc.train_repeat_discriminator):
            self.optimizer_d.zero_grad(set_to_none=True)
            d_loss = self.d_criterion(D(wav, sample_lengths), D(fake_d, sample_lengths), map_lengths)
            d_loss.backward()
            torch.nn.utils.clip_grad_norm_(D.parameters(), mc.grad_clip_thresh)
            self.optimizer_d.step()
            self.discriminator_steps += 1

        # the generator's step: through D's input gradient only - D's parameters ask for none, so their gradients are never computed
        flags = [p.requires_grad for p in D.parameters()]
        for p in D.parameters():
            p.requires_grad_(False)
        try:
            self.optimizer_g.zero_grad(set_to_none=True)
            with torch.no_grad():
                real_maps = D(wav, sample_lengths)
            g_loss = self.g_criterion(real_maps, D(fake, sample_lengths), map_lengths)
            g_adv, g_fm = self.g_criterion.last_terms
            terms = {"d_loss": d_loss.detach().item(), "g_adv": g_adv.detach().item(), "g_feat_match": g_fm.detach().item()}
            if self.stft_loss is not None:
                g_stft = self.stft_loss(fake, wav, sample_lengths)
                g_loss = g_loss + self.stft_weight * g_stft
                terms["g_stft"] = g_stft.detach().item()
            g_loss.backward()
            torch.nn.utils.clip_grad_norm_(G.parameters(), mc.grad_clip_thresh)
            self.optimizer_g.step()
        finally:
            for p, flag in zip(D.parameters(), flags):
                p.requires_grad_(flag)
        terms["g_loss"] = g_loss.detach().item()
        return terms
