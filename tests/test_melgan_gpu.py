"""GPU: the MelGAN generator's kernels (gvx_melgan_forward, csrc/melgan.hip) against the float64 restatement of tests/melgan_ref64.py,
through the C ABI: the waveform and x after every stage, element by element.

Tolerance.  Every case evaluates the SAME restatement in float32 on the CPU and takes, tensor by tensor (waveform, every stage), its
largest distance from float64 - a number that depends on the reference alone (about 3e-6 for the waveform and 5e-6 for the stage
tensors, whose values reach 5, at the default sizes; 5e-7 to 1e-6 at the narrow ones).  The device may differ from float64 by at
most 8 times that number on the same tensor: the factor covers another summation order (a k-ordered fmaf chain per output, the phase
split, the fused K = 2 C product) and the device's tanh."""
import ctypes as C
import functools

import pytest
import torch

from genvox_amd import _lib
from tests import melgan_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0


def _dims(cfg) -> _lib.gvx_melgan_dims:
    return _lib.gvx_melgan_dims(cfg["n_mels"], cfg["base_channels"], len(cfg["ratios"]), (C.c_int32 * 8)(*cfg["ratios"]), cfg["n_res"],
                                cfg["dil_base"], cfg["slope"])


class Net:
    """A handle with the packed weights of a state dict, driven through the C ABI alone."""

    def __init__(self, cfg, sd):
        self.cfg, self.lib, self.dims = cfg, _lib.load(), _dims(cfg)
        self.weights = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
        table = (_lib.gvx_weight_desc * len(self.weights))()
        for i, (k, v) in enumerate(self.weights.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        self.blob = torch.empty(self.lib.gvx_melgan_blob_floats(C.byref(self.dims)), dtype=torch.float32, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.gvx_melgan_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_melgan_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_melgan_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_melgan_destroy(self.h)

    def ws_bytes(self, B, T):
        return self.lib.gvx_melgan_workspace_bytes(C.byref(self.dims), B, T)

    def rc(self, mel, lens, wav, stages, ws, ws_bytes):
        ptrs = (C.c_void_p * len(stages))(*[s.data_ptr() for s in stages]) if stages is not None else None
        return self.lib.gvx_melgan_forward(self.h, mel.data_ptr(), lens.data_ptr() if lens is not None else None, mel.shape[0], mel.shape[2],
                                           wav.data_ptr(), ptrs, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)

    def run(self, mel, lens=None, ws=None, want_stages=True, poison=True):
        """mel float32 [B, M, T] on the device -> (wav, stages [B, C, len] like the restatement's).  Outputs and a workspace of this
        call's own start as NaN."""
        B, _, T = mel.shape
        fill = float("nan") if poison else 0.0
        wav = torch.full((B, T * R.hop(self.cfg)), fill, dtype=torch.float32, device=DEV)
        stages, mul, c = [], 1, self.cfg["base_channels"]
        for r in self.cfg["ratios"]:
            mul, c = mul * r, c // 2
            stages.append(torch.full((B, T * mul, c), fill, dtype=torch.float32, device=DEV))
        if ws is None:
            ws = torch.full((self.ws_bytes(B, T) // 4,), float("nan"), dtype=torch.float32, device=DEV)
        lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        _lib.check(self.rc(mel, lens_dev, wav, stages if want_stages else None, ws, ws.numel() * ws.element_size()))
        torch.cuda.synchronize()
        return wav, [s.transpose(1, 2) for s in stages]


@functools.lru_cache(maxsize=None)
def _net(name):
    cfg = getattr(R, name)
    sd = R.random_state(cfg, seed=11)
    return cfg, sd, Net(cfg, sd)


@functools.lru_cache(maxsize=None)
def _case(name, B, T, lens):
    """(mel float64 with NaN behind every row's length, reference outputs, per-tensor float32 error of the reference): computed once."""
    cfg, sd, _ = _net(name)
    mel = R.random_mel(cfg, B, T, seed=100 * B + T)
    if lens is not None:
        for b, t in enumerate(lens):
            mel[b, :, t:] = float("nan")
    want, errs = R.reference_pair(sd, mel, lens, cfg)
    return mel, want, errs


def _compare(got, want, errs, what):
    names = ["wav"] + [f"stage {i}" for i in range(len(want[1]))]
    for name, g, w, e in zip(names, [got[0]] + list(got[1]), [want[0]] + list(want[1]), errs):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        d = (g.double().cpu() - w).abs().max().item()
        print(f"{what}: {name}: device error {d:.3e}, float32 restatement error {e:.3e}, ratio {d / e:.2f}")
        assert d <= FACTOR * e, f"{what}: {name} differs from float64 by {d:.3e}, above {FACTOR} x {e:.3e}"


def _check(name, B, T, lens=None):
    _, _, net = _net(name)
    mel, want, errs = _case(name, B, T, lens)
    got = net.run(mel.to(DEV, torch.float32), lens)
    _compare(got, want, errs, f"{name} {B} x {T}" + (f" lengths {lens}" if lens else ""))
    return got


@pytest.mark.parametrize("B,T", [(1, 4), (2, 5), (3, 9), (2, 33), (1, 40)])
def test_default_sizes(B, T):
    """T = 4: the first stage is one 32-row tile and the dilation-9 reflections fold inside it; 5 and 9 leave row tails; 33 crosses a
    tile at every stage."""
    wav, _ = _check("DEFAULT", B, T)
    assert wav.abs().max().item() < 1.0


@pytest.mark.parametrize("T", [4, 7, 64])
def test_narrow_sizes(T):
    """Channels 16 and 8 (the dot-product kernel for every layer but the first), K = 70 in the first convolution: N and K tails."""
    _check("NARROW", 3, T)


@pytest.mark.parametrize("name", ["SHALLOW", "TWO_DEEP"])
def test_layer_count_and_dilation_come_from_the_dims(name):
    _check(name, 2, 9)


@pytest.mark.parametrize("B,T", [(1, 4), (2, 11), (1, 22)])
@pytest.mark.parametrize("name", R.NEVER_RUN)
def test_configurations_no_other_case_reaches(name, B, T):
    """ODD and DEEP (tests/melgan_ref64.py says what each reaches; tests/test_generator_configs_cpu.py asserts the path of every layer).
    11 and 22 frames put 66 / 132 and 132 / 264 positions into ODD's two stages, either side of a 128-position tile."""
    wav, _ = _check(name, B, T)
    assert wav.abs().max().item() <= 1.0   # tanh; DEEP's eight layers at slope 1 reach values that float32 rounds to 1 exactly


@pytest.mark.parametrize("name,T,lens", [("DEFAULT", 33, (33, 4, 32, 17)), ("DEFAULT", 9, (5, 9)), ("NARROW", 64, (64, 4, 63, 32)),
                                         ("ODD", 22, (22, 4, 11)), ("DEEP", 22, (22, 4, 11))])
def test_ragged_rows_equal_the_rows_alone(name, T, lens):
    """Every row against the restatement of that row alone; the mel behind a row's frames is NaN, so a read past the row's end shows;
    samples and stage rows behind a row's own length are exact zeros."""
    cfg = getattr(R, name)
    wav, stages = _check(name, len(lens), T, lens)
    for b, t in enumerate(lens):
        assert not wav[b, t * R.hop(cfg):].any()
        mul = 1
        for r, st in zip(cfg["ratios"], stages):
            mul *= r
            assert not st[b, :, t * mul:].any()
    # a row of a ragged batch has the bits of that row run alone
    _, _, net = _net(name)
    mel = _case(name, len(lens), T, lens)[0].to(DEV, torch.float32)
    b = 1
    alone, _ = net.run(mel[b:b + 1, :, :lens[b]].contiguous())
    assert torch.equal(alone[0], wav[b, :lens[b] * R.hop(cfg)])


@pytest.mark.parametrize("name,B,T,lens", [("DEFAULT", 2, 9, (5, 9)), ("NARROW", 3, 7, None), ("ODD", 2, 11, (5, 11)), ("DEEP", 1, 22, None)])
def test_workspace_contract(name, B, T, lens):
    """Exactly the stated size, all NaN before, a NaN guard behind it that stays NaN; one byte short is refused before anything is
    written; a reused (dirty) workspace gives the same bits; stage_out changes no bit of the waveform."""
    _, _, net = _net(name)
    mel, want, errs = _case(name, B, T, lens)
    mel = mel.to(DEV, torch.float32)
    need = net.ws_bytes(B, T)
    assert need % 256 == 0 and need > 0
    guard = 4096
    buf = torch.full(((need + guard) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    ws = buf[:need // 4]
    got = net.run(mel, lens, ws=ws)
    _compare(got, want, errs, f"{name} exact workspace")
    assert torch.isnan(buf[need // 4:]).all(), "the call wrote behind the workspace"
    again = net.run(mel, lens, ws=ws)   # the leftovers of the first call
    assert torch.equal(again[0], got[0]) and all(torch.equal(a, b) for a, b in zip(again[1], got[1]))
    plain = net.run(mel, lens, ws=ws, want_stages=False)
    assert torch.equal(plain[0], got[0])
    wav = torch.full_like(got[0], 7.0)
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    before = buf.clone()
    rc = net.rc(mel, lens_dev, wav, None, ws, need - 1)
    torch.cuda.synchronize()
    assert rc == -5, rc   # GVX_ERR_WORKSPACE
    assert (wav == 7.0).all() and torch.equal(before.view(torch.int32), buf.view(torch.int32))
    assert net.rc(mel, lens_dev, wav, None, buf.view(torch.uint8)[1:], need) == -5   # misaligned


def test_two_calls_give_the_same_bits():
    _, _, net = _net("DEFAULT")
    mel = _case("DEFAULT", 2, 33, None)[0].to(DEV, torch.float32)
    a, b = net.run(mel), net.run(mel)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_python_call_split_by_rows_is_bit_equal():
    """MelGANGenerator.vocode splits a batch by rows when the workspace would pass its cap: forced low, 4 rows run one by one."""
    from genvox_amd.configs import AudioConfig
    from genvox_amd.melgan import MelGANConfig, MelGANGenerator

    cfg, sd, net = _net("DEFAULT")
    model = MelGANGenerator(MelGANConfig(), AudioConfig())
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    model.to(DEV)
    lens = (33, 4, 32, 17)
    mel = _case("DEFAULT", 4, 33, lens)[0].to(DEV, torch.float32)
    whole = model.vocode(mel, lens)
    assert model.workspace_bytes(4, 33) <= model.WORKSPACE_CAP_BYTES
    model.WORKSPACE_CAP_BYTES = model.workspace_bytes(1, 33)
    model._workspace = None
    split = model.vocode(mel, torch.tensor(lens))
    torch.cuda.synchronize()
    assert model._workspace.numel() == model.workspace_bytes(1, 33)
    assert torch.equal(whole, split)
    assert torch.equal(whole, net.run(mel, lens)[0])   # and the Python surface is the C ABI's result
    out = model.inference({"mel": mel, "mel_lengths": torch.tensor(lens)})
    assert out["lengths"].tolist() == [t * 256 for t in lens] and out["lengths"].dtype == torch.int32
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (33, 3, 32, 17))
