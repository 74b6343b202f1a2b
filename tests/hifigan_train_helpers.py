"""What the GPU tests of the HiFi-GAN backward share: a handle driven through the C ABI alone (gvx_hifigan_forward_train,
gvx_hifigan_backward), with the tape, the workspace and every output starting as NaN and sized exactly."""
import ctypes as C

import torch

from genvox_amd import _lib
from tests import hifigan_grad_ref64 as GR
from tests import hifigan_ref64 as R

DEV = "cuda:0"
NAN = float("nan")


def dims_of(cfg) -> _lib.gvx_hifigan_dims:
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


def layout_of(lib, dims, B, T):
    e = (_lib.gvx_hifigan_tape_entry * 512)()
    n = lib.gvx_hifigan_tape_layout(C.byref(dims), B, T, e, 512)
    return [(e[i].byte_offset, e[i].positions_per_frame, e[i].channels) for i in range(n)]


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class TrainNet:
    def __init__(self, cfg, sd):
        self.cfg, self.lib, self.dims = cfg, _lib.load(), dims_of(cfg)
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.weights = {k: v.to(DEV, torch.float32).contiguous() for k, v in sd.items()}
        table = (_lib.gvx_weight_desc * len(self.weights))()
        for i, (k, v) in enumerate(self.weights.items()):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        self.blob = torch.empty(self.lib.gvx_hifigan_blob_floats(C.byref(self.dims)), dtype=torch.float32, device=DEV)
        _lib.check(self.lib.gvx_hifigan_pack_weights_device(C.byref(self.dims), table, len(self.weights), self.blob.data_ptr(), stream()))
        h = C.c_void_p()
        _lib.check(self.lib.gvx_hifigan_create(C.byref(self.dims), C.byref(h)))
        self.h = h.value
        _lib.check(self.lib.gvx_hifigan_bind(self.h, self.blob.data_ptr()))

    def __del__(self):
        self.lib.gvx_hifigan_destroy(self.h)

    def tape_bytes(self, B, T):
        return self.lib.gvx_hifigan_tape_bytes(C.byref(self.dims), B, T)

    def ws_bytes(self, B, T):
        return self.lib.gvx_hifigan_backward_workspace_bytes(C.byref(self.dims), B, T)

    def layout(self, B, T):
        return layout_of(self.lib, self.dims, B, T)

    def forward(self, mel, lens=None):
        """gvx_hifigan_forward: the inference call."""
        B, _, T = mel.shape
        wav = torch.full((B, T * R.hop(self.cfg)), NAN, dtype=torch.float32, device=DEV)
        ws = torch.full((self.lib.gvx_hifigan_workspace_bytes(C.byref(self.dims), B, T) // 4,), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.lib.gvx_hifigan_forward(self.h, mel.data_ptr(), lens.data_ptr() if lens is not None else None, B, T, wav.data_ptr(), None,
                                                ws.data_ptr(), ws.numel() * 4, stream()))
        return wav

    def forward_train_rc(self, mel, lens, wav, tape, tape_bytes):
        B, _, T = mel.shape
        return self.lib.gvx_hifigan_forward_train(self.h, mel.data_ptr(), lens.data_ptr() if lens is not None else None, B, T, wav.data_ptr(),
                                                  tape.data_ptr(), tape_bytes, None, 0, stream())

    def forward_train(self, mel, lens=None):
        """-> (wav, the tape as a flat float32 tensor of exactly gvx_hifigan_tape_bytes, NaN wherever the call did not write)."""
        B, _, T = mel.shape
        wav = torch.full((B, T * R.hop(self.cfg)), NAN, dtype=torch.float32, device=DEV)
        tape = torch.full((self.tape_bytes(B, T) // 4,), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.forward_train_rc(mel, lens, wav, tape, tape.numel() * 4))
        return wav, tape

    def tape_views(self, tape, B, T):
        """The tape's tensors as the restatement has them: [B, C, len] (entry 0 with the mel's padded channels)."""
        return [tape[off // 4: off // 4 + B * T * mul * c].view(B, T * mul, c).transpose(1, 2) for off, mul, c in self.layout(B, T)]

    def new_grads(self, want_mel, B, T):
        out = {k: torch.full(s, NAN, dtype=torch.float32, device=DEV) for k, s in self.shapes.items()}
        if want_mel:
            out["mel"] = torch.full((B, self.cfg["n_mels"], T), NAN, dtype=torch.float32, device=DEV)
        return out

    def backward_rc(self, d_wav, lens, B, T, tape, tape_bytes, grads, ws, ws_bytes, numel=None, skip=(), null=()):
        names = [k for k in grads if k != "mel" and k not in skip]
        table = (_lib.gvx_weight_desc * len(names))()
        for i, k in enumerate(names):
            table[i] = _lib.gvx_weight_desc(k.encode(), None if k in null else grads[k].data_ptr(), (numel or {}).get(k, grads[k].numel()))
        return self.lib.gvx_hifigan_backward(self.h, d_wav.data_ptr(), lens.data_ptr() if lens is not None else None, B, T, tape.data_ptr(), tape_bytes,
                                             table, len(names), grads["mel"].data_ptr() if "mel" in grads else None, ws.data_ptr(), ws_bytes, stream())

    def backward(self, d_wav, lens, B, T, tape, want_mel=True):
        grads = self.new_grads(want_mel, B, T)
        ws = torch.full((self.ws_bytes(B, T) // 4,), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.backward_rc(d_wav, lens, B, T, tape, tape.numel() * 4, grads, ws, ws.numel() * 4))
        torch.cuda.synchronize()
        return grads


def poisoned(mel, G, lens, hop):
    """float32 device copies of a case's mel and cotangent with NaN at and behind every row's length."""
    mel, G = mel.clone(), G.clone()
    if lens is not None:
        for b, t in enumerate(lens):
            mel[b, :, t:] = NAN
            G[b, t * hop:] = NAN
    return mel.to(DEV, torch.float32), G.to(DEV, torch.float32)


def compare_tape(views, ref, lens, what):
    """-> the largest error / bound ratio over the tape's tensors."""
    muls, worst = GR.tape_muls_of(ref), 0.0
    for i, (got, want, e, mul) in enumerate(zip(views, ref["tape"], ref["tape_err"], muls)):
        got = got.double().cpu()[:, :want.shape[1]]   # entry 0: without the padded channels
        B, _, L = want.shape
        for b in range(B):
            n = L if lens is None else lens[b] * mul
            d = (got[b, :, :n] - want[b, :, :n]).abs().max().item()
            assert not torch.isnan(got[b, :, :n]).any(), f"{what}: tape tensor {i}, row {b} holds NaN"
            assert d <= GR.FACTOR * e or (i == 0 and d == 0.0), f"{what}: tape tensor {i}, row {b}: {d:.3e} from float64, above {GR.FACTOR} x {e:.3e}"
            if e > 0:
                worst = max(worst, d / (GR.FACTOR * e))
    return worst


def compare_grads(got, ref, what):
    worst = 0.0
    for k, want in ref["grads"].items():
        if k not in got:
            continue
        g = got[k].double().cpu()
        assert g.shape == want.shape, (what, k, g.shape, want.shape)
        assert not torch.isnan(g).any(), f"{what}: {k} holds NaN"
        d, tol = (g - want).abs().max().item(), ref["grad_tol"][k]
        worst = max(worst, d / tol)
        print(f"{what}: {k}: device error {d:.3e}, float32 restatement error {ref['grad_err'][k]:.3e}, bound {tol:.3e}, scale {want.abs().max().item():.3e}")
        assert d <= tol, f"{what}: d {k} differs from float64 by {d:.3e}, above the bound {tol:.3e} (float32 restatement: {ref['grad_err'][k]:.3e})"
    print(f"{what}: largest gradient error / bound {worst:.3f}")
    return worst
