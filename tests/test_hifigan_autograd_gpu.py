"""GPU: HiFiGANGenerator.vocode_with_grad - the C ABI's training calls behind a torch.autograd.Function - against the C-ABI calls
themselves (bit for bit) and, over ten optimizer steps, against the float64 restatement trained on the CPU."""
import functools

import pytest
import torch

from genvox_amd.configs import AudioConfig, HiFiGANConfig
from genvox_amd.hifigan import HiFiGANGenerator
from tests import hifigan_grad_ref64 as GR
from tests import hifigan_ref64 as R
from tests.hifigan_train_helpers import DEV, TrainNet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """The NaN-filled tapes and workspaces of this module go back to the driver, not into the allocator's cache for later modules."""
    yield
    torch.cuda.empty_cache()


CFG = R.NARROW
LENS = (7, 4)


def _model(sd) -> HiFiGANGenerator:
    ac = AudioConfig()
    ac.n_mels, ac.hop_length = CFG["n_mels"], R.hop(CFG)   # below a preprocessing config's ranges: a test's size
    mc = HiFiGANConfig(upsample_initial_channel=CFG["c0"], upsample_rates=list(CFG["rates"]), upsample_kernel_sizes=[2 * r for r in CFG["rates"]],
                       resblock=CFG["resblock"], resblock_kernel_sizes=list(CFG["kernels"]),
                       resblock_dilation_sizes=[list(d) for d in CFG["dilations"]], leaky_slope=CFG["slope"], post_leaky_slope=CFG["post_slope"])
    model = HiFiGANGenerator(mc, ac)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs():
    mel = R.random_mel(CFG, 2, 7, 1)
    G = torch.randn(2, 7 * R.hop(CFG), generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    return mel.to(DEV, torch.float32), G.to(DEV, torch.float32)


@pytest.mark.parametrize("lens", [None, LENS])
def test_grads_are_the_c_abi_calls_bits(lens):
    """.grad of every parameter and of mel after backward() is bit-equal to gvx_hifigan_backward's outputs on the same inputs; the
    waveform is vocode's; mel.requires_grad is honoured both ways."""
    sd = R.random_state(CFG, 11)
    model, net = _model(sd), TrainNet(CFG, sd)
    mel, G = _inputs()
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    _, tape = net.forward_train(mel, lens_d)
    want = net.backward(G, lens_d, 2, 7, tape)
    assert set(want) == {k for k, _ in model.named_parameters()} | {"mel"}
    for with_mel in (True, False):
        model.zero_grad(set_to_none=True)
        m = mel.clone().requires_grad_(with_mel)
        wav = model.vocode_with_grad(m, lens)
        assert wav.requires_grad and wav.dtype == torch.float32 and wav.shape == (2, 7 * R.hop(CFG))
        assert torch.equal(wav.detach(), model.vocode(mel, lens))
        (wav * G).sum().backward()
        for k, p in model.named_parameters():
            assert torch.equal(p.grad, want[k]), k
        assert (m.grad is not None) == with_mel and (not with_mel or torch.equal(m.grad, want["mel"]))


def test_no_grad_is_vocode_and_frozen_parameters_need_no_tape():
    model = _model(R.random_state(CFG, 11))
    mel, _ = _inputs()
    with torch.no_grad():
        wav = model.vocode_with_grad(mel, LENS)
    assert not wav.requires_grad and torch.equal(wav, model.vocode(mel, LENS))
    for p in model.parameters():
        p.requires_grad_(False)
    assert not model.vocode_with_grad(mel).requires_grad
    m = mel.clone().requires_grad_(True)   # only the mel: a gradient for whoever produced it
    model.vocode_with_grad(m).sum().backward()
    assert m.grad is not None and all(p.grad is None for p in model.parameters())


def test_in_place_change_between_forward_and_backward_raises():
    model = _model(R.random_state(CFG, 11))
    mel, G = _inputs()
    wav = model.vocode_with_grad(mel)
    with torch.no_grad():
        model.conv_post.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (wav * G).sum().backward()


def test_packing_again_between_forward_and_backward_raises():
    model = _model(R.random_state(CFG, 11))
    mel, G = _inputs()
    wav = model.vocode_with_grad(mel)
    model.conv_post.bias.data = model.conv_post.bias.data.clone()   # another tensor under the parameter: no version changes
    model.vocode(mel)                                                # packs again
    with pytest.raises(RuntimeError, match="packed again"):
        (wav * G).sum().backward()


def _restatement_losses(dtype, mel, target, lr, steps):
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in R.random_state(CFG, 11).items()}
    losses = []
    for _ in range(steps):
        loss = ((R.generator(sd, mel.to(dtype), CFG)[0] - target.to(dtype)) ** 2).mean()
        losses.append(loss.item())
        grads = torch.autograd.grad(loss, list(sd.values()))
        with torch.no_grad():
            for p, g in zip(sd.values(), grads):
                p -= lr * g
    return losses


def test_ten_sgd_steps_follow_the_float64_restatement():
    """NARROW 2 x 7, MSE against a teacher generator's waveform of the same mel, plain SGD at lr 0.02.  The inputs are chosen on the
    reference alone: the float64 losses must fall at every step and end below a quarter of the first.  The device's loss at every
    step is held to the float64 restatement trained from the same start on the CPU, within 8 x the float32 CPU restatement's own
    largest relative deviation from those float64 losses (measured in the test, printed with the device's)."""
    lr, steps = 0.02, 10
    mel64 = R.random_mel(CFG, 2, 7, 1)
    target = R.generator(R.random_state(CFG, 12), mel64, CFG)[0]
    want = _restatement_losses(torch.float64, mel64, target, lr, steps)
    assert all(b < a for a, b in zip(want, want[1:])) and want[-1] < 0.25 * want[0], want
    own = _restatement_losses(torch.float32, mel64, target, lr, steps)
    margin = GR.FACTOR * max(abs(a - b) / a for a, b in zip(want, own))
    model = _model(R.random_state(CFG, 11))
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    mel, tgt = mel64.to(DEV, torch.float32), target.to(DEV, torch.float32)
    got = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = ((model.vocode_with_grad(mel) - tgt) ** 2).mean()
        loss.backward()
        opt.step()
        got.append(loss.item())
    worst = max(abs(a - b) / a for a, b in zip(want, got))
    print(f"ten SGD steps: float64 losses {want[0]:.5f} -> {want[-1]:.5f}; device deviation {worst:.3e}, margin {margin:.3e}")
    for i, (a, b) in enumerate(zip(want, got)):
        assert abs(a - b) <= margin * a, f"step {i}: device loss {b:.9f}, float64 {a:.9f}, relative margin {margin:.3e}"
