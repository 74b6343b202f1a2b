"""What the tests of the vocoder denoiser share: a plan driven through the C ABI alone (gvx_denoise), with the workspace and every
output starting as NaN, the input NaN at and behind every row's length, and the workspace sized exactly."""
import ctypes as C

import torch

from genvox_amd import _lib
from tests import denoise_ref64 as R

DEV = "cuda:0"
NAN = float("nan")
G = 4      # GVX_DENOISE_FRAMES_PER_WORKGROUP
S = 256    # GVX_DENOISE_GATHER_SAMPLES


def create(n_fft, hop):
    h = C.c_void_p()
    rc = _lib.load().gvx_denoise_create(n_fft, hop, C.byref(h))
    return rc, h.value


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def poisoned(x, lengths):
    """x on the device as float32, NaN at and behind every row's length."""
    d = x.to(DEV, torch.float32).clone()
    if lengths is not None:
        for b, n in enumerate(lengths):
            d[b, max(n, 0):] = NAN
    return d


class Plan:
    def __init__(self, n_fft, hop):
        self.lib, self.n_fft, self.hop = _lib.load(), n_fft, hop
        rc, self.h = create(n_fft, hop)
        assert rc == 0, self.lib.gvx_last_error()

    def __del__(self):
        if getattr(self, "h", None) is not None:
            self.lib.gvx_denoise_destroy(self.h)

    def ws_bytes(self, B, n_max):
        return self.lib.gvx_denoise_workspace_bytes(self.h, B, n_max)

    def raw(self, wav_d, lens_d, bias_d, strength, want_out=True, want_mag=True, ws=None, in_place=False):
        """One call on device tensors; returns (rc, out, mag), every output NaN before the call (in place: out is wav_d itself)."""
        B, n_max = wav_d.shape
        need = self.ws_bytes(B, n_max)
        assert need > 0 and need % 256 == 0
        if ws is None:
            ws = torch.full((need // 4,), NAN, dtype=torch.float32, device=DEV)   # exactly the stated size
        out = (wav_d if in_place else torch.full((B, n_max), NAN, dtype=torch.float32, device=DEV)) if want_out else None
        mag = torch.full((B, R.frames(n_max, self.hop), self.n_fft // 2 + 1), NAN, dtype=torch.float32, device=DEV) if want_mag else None
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.gvx_denoise(self.h, wav_d.data_ptr(), ptr(lens_d), B, n_max, ptr(bias_d), strength, ptr(out), ptr(mag), ws.data_ptr(), need, stream())
        torch.cuda.synchronize()
        return rc, out, mag

    def run(self, wav, lengths=None, bias=None, strength=0.0, **kw):
        """CPU tensors in, poisoned behind the lengths; asserts GVX_OK; CPU tensors (out, mag) back."""
        lens_d = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
        bias_d = None if bias is None else bias.to(DEV, torch.float32).contiguous()
        rc, out, mag = self.raw(poisoned(wav, lengths), lens_d, bias_d, strength, **kw)
        assert rc == 0, self.lib.gvx_last_error()
        return None if out is None else out.cpu(), None if mag is None else mag.cpu()


def zeros_behind(out, mag, lengths, hop):
    """out is exact zeros at and behind every row's length, mag behind its frames; nothing is NaN."""
    for b, n in enumerate(lengths):
        if out is not None:
            assert bool((out[b, n:] == 0).all()) and bool(torch.isfinite(out[b]).all()), b
        if mag is not None:
            assert bool((mag[b, R.frames(n, hop):] == 0).all()) and bool(torch.isfinite(mag[b]).all()), b
