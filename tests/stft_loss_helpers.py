"""What the GPU tests of the multi-resolution STFT loss share: a plan driven through the C ABI alone (gvx_stft_loss), with the
workspace, every output and everything behind a row's length in both inputs starting as NaN, and the workspace sized exactly."""
import ctypes as C

import torch

from genvox_amd import _lib
from tests import stft_loss_ref64 as R

DEV = "cuda:0"
NAN = float("nan")
G = 4      # GVX_STFT_LOSS_FRAMES_PER_WORKGROUP
S = 256    # GVX_STFT_LOSS_GATHER_SAMPLES


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
    def __init__(self, resolutions, w_sc=1.0, w_mag=1.0, eps=R.EPS):
        self.lib, self.res = _lib.load(), tuple(resolutions)
        table = (_lib.gvx_stft_resolution * len(self.res))(*[_lib.gvx_stft_resolution(*r) for r in self.res])
        h = C.c_void_p()
        _lib.check(self.lib.gvx_stft_loss_create(table, len(self.res), w_sc, w_mag, eps, C.byref(h)))
        self.h = h.value

    def __del__(self):
        if getattr(self, "h", None) is not None:
            self.lib.gvx_stft_loss_destroy(self.h)

    def ws_bytes(self, B, n_max):
        return self.lib.gvx_stft_loss_workspace_bytes(self.h, B, n_max)

    def raw(self, pred_d, target_d, lens_d, want_grad=True, want_parts=True, want_dbg=False, ws=None, ws_bytes=None):
        """One call on device tensors; returns (rc, loss, parts, d_pred, Mp list, Mt list), every output NaN before the call."""
        B, n_max = pred_d.shape
        need = self.ws_bytes(B, n_max)
        assert need > 0 and need % 256 == 0
        if ws is None:
            ws = torch.full((need // 4,), NAN, dtype=torch.float32, device=DEV)   # exactly the stated size
        loss = torch.full((1,), NAN, dtype=torch.float32, device=DEV)
        parts = torch.full((B, len(self.res), 2), NAN, dtype=torch.float32, device=DEV) if want_parts else None
        d_pred = torch.full((B, n_max), NAN, dtype=torch.float32, device=DEV) if want_grad else None
        Mp = Mt = None
        dbg = None
        if want_dbg:
            Mp = [torch.full((B, R.frames(n_max, hop), n_fft // 2 + 1), 7.0, dtype=torch.float32, device=DEV) for n_fft, hop, _ in self.res]
            Mt = [torch.full_like(m, 7.0) for m in Mp]
            dbg = _lib.gvx_stft_loss_debug()
            for r in range(len(self.res)):
                dbg.mag_pred[r], dbg.mag_target[r] = Mp[r].data_ptr(), Mt[r].data_ptr()
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.gvx_stft_loss(self.h, pred_d.data_ptr(), target_d.data_ptr(), ptr(lens_d), B, n_max, loss.data_ptr(), ptr(parts), ptr(d_pred),
                                    None if dbg is None else C.byref(dbg), ws.data_ptr(), need if ws_bytes is None else ws_bytes, stream())
        torch.cuda.synchronize()
        return rc, loss, parts, d_pred, Mp, Mt

    def run(self, pred, target, lengths=None, **kw):
        """CPU tensors in, poisoned behind the lengths; asserts GVX_OK; CPU tensors out."""
        lens_d = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
        rc, loss, parts, d_pred, Mp, Mt = self.raw(poisoned(pred, lengths), poisoned(target, lengths), lens_d, **kw)
        assert rc == 0, self.lib.gvx_last_error()
        cpu = lambda t: None if t is None else t.cpu()
        return dict(loss=loss.cpu()[0], parts=cpu(parts), d_pred=cpu(d_pred), Mp=None if Mp is None else [m.cpu() for m in Mp],
                    Mt=None if Mt is None else [m.cpu() for m in Mt])


def device_signs(out, lengths, resolutions, n_max):
    """sign(M_t - M_p) of the device's own magnitudes per row and resolution, [F_b, bins] each - the decision the gradient kernel takes
    (the logarithm is monotone) - after asserting that the debug tensors are NaN exactly behind every row's frames."""
    B = out["Mp"][0].shape[0]
    lengths = [n_max] * B if lengths is None else lengths
    signs = []
    for b in range(B):
        rows = []
        for r, (n_fft, hop, _) in enumerate(resolutions):
            F = R.frames(lengths[b], hop)
            for M in (out["Mp"][r], out["Mt"][r]):
                assert bool(torch.isfinite(M[b, :F]).all()) and bool(torch.isnan(M[b, F:]).all())
            rows.append(torch.sign(out["Mt"][r][b, :F].double() - out["Mp"][r][b, :F].double()))
        signs.append(rows)
    return signs


def ratio(dev, ref, err):
    """Largest |device - float64| as a fraction of its bound."""
    return float((dev.double() - ref).abs().max()) / R.tol(err, ref)
