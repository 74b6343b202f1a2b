"""What the GPU tests of the mel-spectrogram L1 loss share: a plan driven through the C ABI alone (gvx_mel_loss), with the workspace,
every output and everything behind a row's length in both inputs starting as NaN, and the workspace sized exactly."""
import ctypes as C
import os
import re

import numpy as np
import torch

from genvox_amd import _lib
from tests import mel_loss_ref64 as R

DEV = "cuda:0"
NAN = float("nan")
_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "genvox_amd.h")).read()


def enum(name):
    """A constant of the header's GVX_MEL_LOSS_* enum."""
    value, shift = re.search(name + r" = (\d+)(?: << (\d+))?", _HEADER).groups()
    return int(value) << int(shift or 0)


G = enum("GVX_MEL_LOSS_FRAMES_PER_WORKGROUP")
S = enum("GVX_MEL_LOSS_GATHER_SAMPLES")
MAX_MELS = enum("GVX_MEL_LOSS_MAX_MELS")


def create(cfg, n_mels=None, basis=None):
    """(status, handle) of gvx_mel_loss_create for a mel_loss_ref64.Config."""
    lib = _lib.load()
    b = np.ascontiguousarray((cfg.basis if basis is None else basis).numpy(), dtype=np.float32)
    h = C.c_void_p()
    rc = lib.gvx_mel_loss_create(cfg.n_fft, cfg.hop, cfg.win_length, b.shape[0] if n_mels is None else n_mels, b.ctypes.data, cfg.clamp, cfg.mag_eps,
                                 C.byref(h))
    return rc, h.value


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def poisoned(x, lengths):
    """x on the device as float32, NaN at and behind every row's length."""
    d = x.to(DEV, torch.float32).clone()
    if lengths is not None:
        for b, n in enumerate(lengths):
            d[b, n:] = NAN
    return d


class Plan:
    def __init__(self, cfg):
        self.lib, self.cfg = _lib.load(), cfg
        rc, self.h = create(cfg)
        _lib.check(rc)

    def __del__(self):
        if getattr(self, "h", None) is not None:
            self.lib.gvx_mel_loss_destroy(self.h)

    def ws_bytes(self, B, n_max):
        return self.lib.gvx_mel_loss_workspace_bytes(self.h, B, n_max)

    def raw(self, pred_d, target_d, lens_d, want_grad=True, want_parts=True, want_dbg=False, ws=None, ws_bytes=None):
        """One call on device tensors; returns (rc, loss, parts, d_pred, l_p, l_t), every output NaN (the debug tensors 7) before it."""
        B, n_max = pred_d.shape
        need = self.ws_bytes(B, n_max)
        assert need > 0 and need % 256 == 0
        if ws is None:
            ws = torch.full((need // 4,), NAN, dtype=torch.float32, device=DEV)   # exactly the stated size
        loss = torch.full((1,), NAN, dtype=torch.float32, device=DEV)
        parts = torch.full((B,), NAN, dtype=torch.float32, device=DEV) if want_parts else None
        d_pred = torch.full((B, n_max), NAN, dtype=torch.float32, device=DEV) if want_grad else None
        lp = lt = dbg = None
        if want_dbg:
            lp = torch.full((B, n_max // self.cfg.hop, self.cfg.basis.shape[0]), 7.0, dtype=torch.float32, device=DEV)
            lt = torch.full_like(lp, 7.0)
            dbg = _lib.gvx_mel_loss_debug(lp.data_ptr(), lt.data_ptr())
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.gvx_mel_loss(self.h, pred_d.data_ptr(), target_d.data_ptr(), ptr(lens_d), B, n_max, loss.data_ptr(), ptr(parts), ptr(d_pred),
                                   None if dbg is None else C.byref(dbg), ws.data_ptr(), need if ws_bytes is None else ws_bytes, stream())
        torch.cuda.synchronize()
        return rc, loss, parts, d_pred, lp, lt

    def run(self, pred, target, lengths=None, **kw):
        """CPU tensors in, poisoned behind the lengths; asserts GVX_OK; CPU tensors out."""
        lens_d = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
        rc, loss, parts, d_pred, lp, lt = self.raw(poisoned(pred, lengths), poisoned(target, lengths), lens_d, **kw)
        assert rc == 0, self.lib.gvx_last_error()
        cpu = lambda t: None if t is None else t.cpu()
        return dict(loss=loss.cpu()[0], parts=cpu(parts), d_pred=cpu(d_pred), lp=cpu(lp), lt=cpu(lt))


def ratio(dev, ref, err):
    """Largest |device - float64| as a fraction of its bound; where the bound is 0 (an all-zero reference that float32 gives exactly)
    only an exact result is inside it."""
    diff, bound = float((dev.double() - ref).abs().max()), R.tol(err, ref)
    if bound == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / bound
