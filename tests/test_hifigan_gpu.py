"""GPU: the HiFi-GAN generator's kernels (gvx_hifigan_forward, csrc/hifigan.hip) against the float64 restatement of
tests/hifigan_ref64.py, through the C ABI: the waveform and x after every stage's average, element by element.

Tolerance.  Every case evaluates the SAME restatement in float32 on the CPU and takes, tensor by tensor (waveform, every stage), its
largest distance from float64 - a number that depends on the reference alone (1e-7 to 8e-7 on the waveform, 2e-7 to 3e-6 on the stage
tensors, whose values stay below 4).  The device may differ from float64 by at most 8 times the larger of that number and one float32
ulp at the tensor's scale (2^-23 x its largest magnitude).  The factor is the project's, the one the MelGAN tests use for another
summation order (a k-ordered fmaf chain per output, channel blocks outside and taps inside, the phase split) and the device's tanh;
the floor is there because at T = 1 the restatement's error on a tensor of a few dozen elements can come out luckily small.

Largest ratios of device error to that bound's base seen on an MI355X: see DESIGN.md, "HiFi-GAN generator"."""
import ctypes as C
import functools

import pytest
import torch

from genvox_amd import _lib
from tests import hifigan_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0
ULP = 2.0 ** -23


def _dims(cfg) -> _lib.gvx_hifigan_dims:
    d = _lib.gvx_hifigan_dims()
    d.n_mels, d.upsample_initial_channel, d.n_stages = cfg["n_mels"], cfg["c0"], len(cfg["rates"])
    for i, r in enumerate(cfg["rates"]):
        d.upsample_rates[i], d.upsample_kernel_sizes[i] = r, 2 * r
    d.resblock, d.n_resblocks, d.n_dilations = int(cfg["resblock"]), len(cfg["kernels"]), len(cfg["dilations"][0])
    for j, (k, ds) in enumerate(zip(cfg["kernels"], cfg["dilations"])):
        d.resblock_kernel_sizes[j] = k
        for m, dil in enumerate(ds):
            d.resblock_dilation_sizes[j][m] = dil
    d.slope, d.post_slope = cfg["slope"], cfg["post_slope"]
    return d


class Net:
    """A handle with the packed weights of a state dict, driven through the C ABI alone."""

    def __init__(self, cfg, sd):
        self.cfg, self.lib, self.dims = cfg, _lib.load(), _dims(cfg)
        self.weights = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
        table = (_lib.gvx_weight_desc * len(self.weights))()
        for i, (k, v) in enumerate(self.weights.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        self.blob = torch.empty(self.lib.gvx_hifigan_blob_floats(C.byref(self.dims)), dtype=torch.float32, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.gvx_hifigan_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_hifigan_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_hifigan_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_hifigan_destroy(self.h)

    def ws_bytes(self, B, T):
        return self.lib.gvx_hifigan_workspace_bytes(C.byref(self.dims), B, T)

    def rc(self, mel, lens, wav, stages, ws, ws_bytes):
        ptrs = (C.c_void_p * len(stages))(*[s.data_ptr() for s in stages]) if stages is not None else None
        return self.lib.gvx_hifigan_forward(self.h, mel.data_ptr(), lens.data_ptr() if lens is not None else None, mel.shape[0], mel.shape[2],
                                            wav.data_ptr(), ptrs, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)

    def run(self, mel, lens=None, ws=None, want_stages=True):
        """mel float32 [B, M, T] on the device -> (wav, stages [B, C, len] like the restatement's).  Outputs and a workspace of this
        call's own start as NaN."""
        B, _, T = mel.shape
        wav = torch.full((B, T * R.hop(self.cfg)), float("nan"), dtype=torch.float32, device=DEV)
        stages, mul, c = [], 1, self.cfg["c0"]
        for r in self.cfg["rates"]:
            mul, c = mul * r, c // 2
            stages.append(torch.full((B, T * mul, c), float("nan"), dtype=torch.float32, device=DEV))
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
        base = max(e, ULP * w.abs().max().item())
        print(f"{what}: {name}: device error {d:.3e}, float32 restatement error {e:.3e}, one ulp at scale {ULP * w.abs().max().item():.3e}, ratio {d / base:.2f}")
        assert d <= FACTOR * base, f"{what}: {name} differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"


def _check(name, B, T, lens=None):
    _, _, net = _net(name)
    mel, want, errs = _case(name, B, T, lens)
    got = net.run(mel.to(DEV, torch.float32), lens)
    _compare(got, want, errs, f"{name} {B} x {T}" + (f" lengths {lens}" if lens else ""))
    return got


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (2, 6), (2, 7), (1, 32), (2, 33), (1, 65)])
def test_mid_sizes(B, T):
    """Every layer on the matrix kernel; stage 0 has 4 T positions.  T = 1: the row is shorter than every halo.  6 / 7 straddle the
    25-position reach of k = 11, d = 5: taps fall outside on both sides at once.  32 is exactly one 128-position tile, 33 leaves a
    4-row tile whose window reaches back into the previous one, 65 crosses tiles at both stages."""
    wav, _ = _check("MID", B, T)
    assert wav.abs().max().item() < 1.0


@pytest.mark.parametrize("T", [1, 7, 33])
def test_narrow_sizes(T):
    """Channels 24 and 12: the N tail of conv_pre's 48 columns, its K tail (7 x 12 channels in blocks of 32), and the dot-product
    kernel with its three epilogues for every residual block."""
    _check("NARROW", 3, T)


@pytest.mark.parametrize("T", [1, 9, 33])
def test_resblock_two_and_the_widest_window(T):
    """resblock "2" at 32 and 16 channels: one stage per kernel, and the 72-row halo of k = 7, d = 12."""
    _check("TWO", 2, T)


@pytest.mark.parametrize("name,B,T", [("V1", 1, 1), ("V1", 2, 5), ("V2", 1, 9), ("V3", 1, 5)])
def test_published_configurations(name, B, T):
    """The published shapes; V1's first stage sums 5632 terms per output."""
    wav, _ = _check(name, B, T)
    assert wav.abs().max().item() < 1.0


@pytest.mark.parametrize("B,T", [(1, 1), (2, 11), (1, 22)])
@pytest.mark.parametrize("name", R.NEVER_RUN)
def test_configurations_no_published_shape_reaches(name, B, T):
    """ODD, ONE and FOUR (tests/hifigan_ref64.py says what each reaches; tests/test_generator_configs_cpu.py asserts the path of every
    layer).  11 and 22 frames put 66 / 132 and 132 / 264 positions into ODD's two stages, either side of a 128-position tile; at 1 frame
    ONE's row of 10 positions is shorter than the 36 positions of its window's left half."""
    wav, _ = _check(name, B, T)
    assert wav.abs().max().item() < 1.0


@pytest.mark.parametrize("name,lens", [("MID", (33, 1, 32, 17)), ("NARROW", (33, 1, 32, 7)), ("ODD", (22, 1, 11)), ("ONE", (22, 1, 11)),
                                       ("FOUR", (22, 1, 11))])
def test_ragged_rows_equal_the_rows_alone(name, lens):
    """Every row against the restatement of that row alone; the mel behind a row's frames is NaN, so a read past the row's end shows;
    samples and stage rows behind a row's own length are exact zeros."""
    cfg, T = getattr(R, name), max(lens)
    wav, stages = _check(name, len(lens), T, lens)
    for b, t in enumerate(lens):
        assert not wav[b, t * R.hop(cfg):].any()
        mul = 1
        for r, st in zip(cfg["rates"], stages):
            mul *= r
            assert not st[b, :, t * mul:].any()
    # a row of a ragged batch has the bits of that row run alone
    _, _, net = _net(name)
    mel = _case(name, len(lens), T, lens)[0].to(DEV, torch.float32)
    b = len(lens) - 1
    alone, _ = net.run(mel[b:b + 1, :, :lens[b]].contiguous())
    assert torch.equal(alone[0], wav[b, :lens[b] * R.hop(cfg)])


@pytest.mark.parametrize("name,B,T,lens", [("MID", 2, 9, (5, 9)), ("NARROW", 3, 7, None), ("ODD", 2, 11, (5, 11)), ("ONE", 1, 22, None),
                                           ("FOUR", 2, 11, (11, 3))])
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
    _, _, net = _net("MID")
    mel = _case("MID", 2, 33, None)[0].to(DEV, torch.float32)
    a, b = net.run(mel), net.run(mel)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_python_call_split_by_rows_is_bit_equal():
    """HiFiGANGenerator.vocode splits a batch by rows when the workspace would pass its cap: forced low, 4 rows run one by one."""
    from genvox_amd.configs import AudioConfig, HiFiGANConfig
    from genvox_amd.hifigan import HiFiGANGenerator

    cfg, sd, net = _net("MID")
    ac = AudioConfig(n_mels=cfg["n_mels"])
    ac.hop_length = R.hop(cfg)   # below the range of a preprocessing config; a vocoder of hop 8 is a test's size
    model = HiFiGANGenerator(HiFiGANConfig(upsample_initial_channel=cfg["c0"], upsample_rates=cfg["rates"],
                                           upsample_kernel_sizes=[2 * r for r in cfg["rates"]]), ac)
    model.load_state_dict({k: v.float() for k, v in sd.items()})
    model.to(DEV)
    lens = (33, 1, 32, 17)
    mel = _case("MID", 4, 33, lens)[0].to(DEV, torch.float32)
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
    assert out["lengths"].tolist() == [t * R.hop(cfg) for t in lens] and out["lengths"].dtype == torch.int32
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (33, 0, 32, 17))
    with pytest.raises(ValueError, match="frames"):
        model.vocode(mel, (34, 1, 32, 17))
