"""GPU: ``VocosGenerator(trainable=True).vocode_with_grad`` as an autograd node (gvx_vocos_forward_train / gvx_vocos_backward behind
``_VocodeWithGrad``), and one ``HiFiGANTrainer`` step on it.  MID of tests/vocos_ref64.py ("center" padding: a row of t frames delivers
(t - 1) x hop samples), lengths (9, 5), the loss 0.5 (wav - target)^2 meaned per row over the row's own samples.

Tolerance: the project's rule, per tensor: 8 x max(|float32 restatement - float64|, 2^-23 max|g64|) (tests/vocos_train_helpers.py)."""
import pytest
import torch

from genvox_amd.hifigan_training import HiFiGANTrainer
from genvox_amd.losses import MelSpectrogramLoss
from genvox_amd.mrd import MultiResolutionDiscriminator
from tests import vocos_grad_ref64 as GR
from tests import vocos_ref64 as R
from tests.vocos_train_helpers import DEV, NAN, TrainNet, bound_check, build, poisoned

pytestmark = pytest.mark.gpu
CFG = R.MID
LENS = (9, 5)
T = max(LENS)


def _ref():
    ref = R.Generator(CFG, seed=11)
    ref.load_state_dict({k: v.float().double() for k, v in ref.state_dict().items()})
    return ref


def _model(ref, trainable=True):
    model = build(CFG, trainable=trainable)
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return model.to(DEV)


def _target(seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(len(LENS), T * CFG["hop_length"], generator=g, dtype=torch.float64)


def _loss(wav, target, lens):
    return sum(0.5 * ((wav[b, :n] - target[b, :n]) ** 2).mean() for b, n in enumerate(R.sample_count(CFG, t) for t in lens))


def _tie_free_mel(ref):
    """The first mel seed whose clamp has no near-tie; the cotangent of the loss is (wav - target) / n_b, which the restatement forms
    itself, so the reference is autograd of the same expression."""
    target = _target()
    for seed in range(1, 9):
        mel = R.random_mel(CFG, len(LENS), T, seed).float().double()
        probe = GR.reference(ref, mel, LENS, torch.zeros_like(target))
        if GR.near_ties(probe, LENS, CFG) == 0:
            return mel, target
    raise AssertionError("no tie-free mel seed in 1..8")


def _reference_grads(ref, mel, target, dtype):
    gen = ref if dtype == torch.float64 else None
    if gen is None:
        import copy
        gen = copy.deepcopy(ref).float()
        gen.cfg = ref.cfg
    gen.zero_grad(set_to_none=True)
    d_mel = torch.zeros_like(mel, dtype=dtype)
    total = 0.0
    for b, t in enumerate(LENS):
        row = mel[b:b + 1, :, :t].to(dtype).clone().requires_grad_(True)
        wav, _ = GR.forward(gen, row)
        n = wav.shape[1]
        loss = 0.5 * ((wav[0] - target[b, :n].to(dtype)) ** 2).mean()
        loss.backward()
        d_mel[b, :, :t] = row.grad[0]
        total += loss.item()
    return {k: p.grad.detach().clone() for k, p in gen.named_parameters()}, d_mel, total


def test_grad_of_every_parameter_and_of_the_mel():
    ref = _ref()
    mel, target = _tie_free_mel(ref)
    want, want_mel, _ = _reference_grads(ref, mel, target, torch.float64)
    g32, mel32, _ = _reference_grads(ref, mel, target, torch.float32)
    model = _model(ref)
    mel_d, _ = poisoned(CFG, mel, target, LENS)
    mel_d.requires_grad_(True)
    target_d = target.float().to(DEV)
    wav = model.vocode_with_grad(mel_d, list(LENS))
    with torch.no_grad():
        plain = model.vocode(mel_d.detach(), list(LENS))
        assert torch.equal(model.vocode_with_grad(mel_d.detach(), list(LENS)), plain)   # under no_grad it IS vocode
    assert torch.equal(wav.detach(), plain), "the waveform is not vocode's"
    _loss(wav, target_d, LENS).backward()
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        bound_check(p.grad, want[k], (g32[k].double() - want[k]).abs().max().item(), f"autograd: d {k}")
    bound_check(mel_d.grad, want_mel, (mel32.double() - want_mel).abs().max().item(), "autograd: d mel")
    for b, t in enumerate(LENS):
        assert not mel_d.grad[b, :, t:].any()

    # the same bits as the C-ABI call with the cotangent autograd handed the node
    net = TrainNet(CFG, ref)
    lens_d = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    w2, tape = net.forward_train(mel_d.detach(), lens_d)
    assert torch.equal(w2, plain)
    G = torch.full_like(plain, NAN)
    for b, t in enumerate(LENS):
        n = R.sample_count(CFG, t)
        G[b, :n] = (plain[b, :n] - target_d[b, :n]) / n
    grads = net.backward(G, lens_d, len(LENS), T, tape)
    for k, p in model.named_parameters():
        assert torch.equal(p.grad, grads[k]), k
    assert torch.equal(mel_d.grad, grads["mel"])


def test_version_error_repack_and_the_refusal():
    ref = _ref()
    model = _model(ref)
    mel = R.random_mel(CFG, 2, T, 1).float().to(DEV)
    wav = model.vocode_with_grad(mel, list(LENS))
    with torch.no_grad():
        model.head.out.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        wav.sum().backward()
    wav = model.vocode_with_grad(mel, list(LENS))
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})   # (in place too: the version error comes first)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        wav.sum().backward()
    wav = model.vocode_with_grad(mel, list(LENS))
    model.head.out.bias.data = model.head.out.bias.data.clone()   # another tensor under the parameter: no version changes
    model.vocode(mel, list(LENS))   # packs again
    with pytest.raises(RuntimeError, match="packed again"):
        wav.sum().backward()
    model.trainable = False
    with pytest.raises(NotImplementedError, match="backward"):
        model.vocode_with_grad(mel, list(LENS))
    with torch.no_grad():
        assert torch.equal(model.vocode_with_grad(mel, list(LENS)), model.vocode(mel, list(LENS)))
    model.trainable = True
    model.vocode_with_grad(mel, list(LENS)).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


class _Recorder:
    def __init__(self):
        self.seen = []


@pytest.mark.parametrize("lengths", [LENS, None])
def test_one_trainer_step(lengths):
    """MultiResolutionDiscriminator and MelSpectrogramLoss; with lengths (9, 5) and without: the sample counts handed on are
    sample_counts' - 2048 and 1024 (or 2048 twice), not 2304 and 1280."""
    torch.manual_seed(3)
    model = _model(_ref())
    disc = MultiResolutionDiscriminator().to(DEV)
    aux = MelSpectrogramLoss()
    rec = _Recorder()
    inner_map, inner_aux = disc.map_lengths, aux.forward
    disc.map_lengths = lambda n: (rec.seen.append(("map", list(n))), inner_map(n))[1]
    aux.forward = lambda fake, wav, n=None: (rec.seen.append(("aux", None if n is None else list(n))), inner_aux(fake, wav, n))[1]
    trainer = HiFiGANTrainer(model, [disc], aux_loss=aux)
    hop = CFG["hop_length"]
    lens = LENS if lengths is not None else (T, T)
    mel = R.random_mel(CFG, 2, T, 1).float()
    g = torch.Generator().manual_seed(2)
    wav = 0.1 * torch.randn(2, T * hop, generator=g)
    for b, t in enumerate(lens):
        mel[b, :, t:] = NAN
        wav[b, R.sample_count(CFG, t):] = NAN
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    terms = trainer.train_step(mel.to(DEV), wav.to(DEV), None if lengths is None else list(lengths))
    for k, v in terms.items():
        assert isinstance(v, float) and v == v and abs(v) < float("inf"), f"loss term {k} = {v}"
    for k, v in model.state_dict().items():
        assert torch.isfinite(v).all() and not torch.equal(v, before[k]), f"{k} did not move"
    want = [R.sample_count(CFG, t) for t in lens]
    assert want == ([2048, 1024] if lengths is not None else [2048, 2048])
    assert rec.seen and all(n == want for _, n in rec.seen), rec.seen
    assert {kind for kind, _ in rec.seen} == {"map", "aux"}
