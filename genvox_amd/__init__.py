"""genvox_amd: MI355X-native Tacotron2 text->mel forward path and Griffin-Lim vocoder behind GenVox's Python surface.

    from genvox_amd import Tacotron2, Synthesizer, AudioProcessor, Tacotron2Config, AudioConfig, TextConfig
    from genvox_amd import MelGANGenerator, MelGANConfig   # neural vocoder: Synthesizer(..., vocoder_model_class=MelGANGenerator, ...)
    from genvox_amd import HiFiGANGenerator, HiFiGANConfig   # HiFi-GAN V1 / V2 / V3 generators, the same place in Synthesizer
    from genvox_amd import BigVGANGenerator, BigVGANConfig   # BigVGAN (anti-aliased Snake activations), inference, the same place
    from genvox_amd import VocosGenerator, VocosConfig   # Vocos (ConvNeXt backbone at the frame rate + inverse STFT), inference, the same place
    from genvox_amd import UnivNetGenerator, UnivNetConfig   # UnivNet (noise through location-variable convolutions), inference, the same place
    from genvox_amd import FastPitch, FastPitchConfig   # non-autoregressive text->mel: Synthesizer(tts_model_class=FastPitch, ...)
    from genvox_amd import Tacotron2GuidedLoss    # training criterion: Tacotron2Loss + alpha x guided attention loss
    from genvox_amd import MelGANDiscriminator, MelGANDiscriminatorConfig, MelGANTrainer   # the other side of the vocoder's GAN step
    from genvox_amd import HiFiGANPeriodDiscriminator, HiFiGANPeriodDiscriminatorConfig, HiFiGANTrainer, HiFiGANTrainingConfig   # HiFi-GAN's GAN step
    from genvox_amd import HiFiGANScaleDiscriminator, HiFiGANScaleDiscriminatorConfig   # ... and its multi-scale discriminator
    from genvox_amd import MultiResolutionDiscriminator, MultiResolutionDiscriminatorConfig   # UnivNet's / BigVGAN's spectrogram discriminator
    from genvox_amd import MultiResolutionSTFTLoss, stft_distance   # vocoder training loss / waveform distance on the device
    from genvox_amd import MelSpectrogramLoss, mel_distance         # HiFi-GAN's mel-spectrogram L1 term / log-mel distance
    from genvox_amd import Denoiser   # vocoder denoiser: Denoiser.from_vocoder(vocoder)(wav), or Synthesizer.tts(text, denoise=0.01)
"""
from .configs import HiFiGANPeriodDiscriminatorConfig, HiFiGANScaleDiscriminatorConfig, HiFiGANTrainingConfig  # noqa: F401
from .configs import FastPitchConfig, MultiResolutionDiscriminatorConfig, UnivNetConfig, VocosConfig  # noqa: F401
from .configs import AudioConfig, BaseConfig, BigVGANConfig, HiFiGANConfig, MelGANConfig, MelGANDiscriminatorConfig, Tacotron2Config, TextConfig  # noqa: F401


def __getattr__(name):  # torch-dependent classes are imported lazily
    if name == "Tacotron2":
        from .tacotron2 import Tacotron2
        return Tacotron2
    if name == "Tacotron2GuidedLoss":
        from .tacotron2 import Tacotron2GuidedLoss
        return Tacotron2GuidedLoss
    if name == "FastPitch":
        from .fastpitch import FastPitch
        return FastPitch
    if name == "MelGANGenerator":
        from .melgan import MelGANGenerator
        return MelGANGenerator
    if name == "HiFiGANGenerator":
        from .hifigan import HiFiGANGenerator
        return HiFiGANGenerator
    if name == "BigVGANGenerator":
        from .bigvgan import BigVGANGenerator
        return BigVGANGenerator
    if name == "VocosGenerator":
        from .vocos import VocosGenerator
        return VocosGenerator
    if name == "UnivNetGenerator":
        from .univnet import UnivNetGenerator
        return UnivNetGenerator
    if name == "MelGANDiscriminator":
        from .melgan_disc import MelGANDiscriminator
        return MelGANDiscriminator
    if name == "MelGANTrainer":
        from .melgan_training import MelGANTrainer
        return MelGANTrainer
    if name == "HiFiGANPeriodDiscriminator":
        from .hifigan_disc import HiFiGANPeriodDiscriminator
        return HiFiGANPeriodDiscriminator
    if name == "HiFiGANScaleDiscriminator":
        from .hifigan_msd import HiFiGANScaleDiscriminator
        return HiFiGANScaleDiscriminator
    if name == "MultiResolutionDiscriminator":
        from .mrd import MultiResolutionDiscriminator
        return MultiResolutionDiscriminator
    if name == "HiFiGANTrainer":
        from .hifigan_training import HiFiGANTrainer
        return HiFiGANTrainer
    if name in ("MelGANDiscriminatorLoss", "MelGANGeneratorLoss", "HiFiGANDiscriminatorLoss", "HiFiGANGeneratorLoss"):
        from . import losses
        return getattr(losses, name)
    if name == "MultiResolutionSTFTLoss":
        from .losses import MultiResolutionSTFTLoss
        return MultiResolutionSTFTLoss
    if name == "MelSpectrogramLoss":
        from .losses import MelSpectrogramLoss
        return MelSpectrogramLoss
    if name == "Denoiser":
        from .denoiser import Denoiser
        return Denoiser
    if name == "mel_distance":
        from .metrics import mel_distance
        return mel_distance
    if name == "stft_distance":
        from .metrics import stft_distance
        return stft_distance
    if name == "Synthesizer":
        from .synthesizer import Synthesizer
        return Synthesizer
    if name == "AudioProcessor":
        from .audio import AudioProcessor
        return AudioProcessor
    if name == "TextProcessor":
        from .text import TextProcessor
        return TextProcessor
    raise AttributeError(name)
