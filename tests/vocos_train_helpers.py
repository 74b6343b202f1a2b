"""What the GPU tests of the Vocos backward share: a device model with the restatement's weights driven through the C ABI
(gvx_vocos_forward_train / gvx_vocos_backward), with NaN-filled tapes, workspaces and outputs of exactly their stated sizes, and the
project's bound: the device may differ from float64 by at most 8 x max(e, 2^-23 max|want|), e the float32 restatement's own error."""
import ctypes as C

import torch

from genvox_amd import _lib
from genvox_amd._device_module import _weight_table
from genvox_amd.configs import AudioConfig, VocosConfig
from genvox_amd.vocos import VocosGenerator
from tests import vocos_ref64 as R

DEV = "cuda:0"
NAN = float("nan")
FACTOR = 8.0
ULP = 2.0 ** -23
RAW = ("gamma", "pwconv2.weight", "pwconv2.bias")


def bound_check(got, want, err32, what):
    """-> error / bound; asserts the rule and prints the ratio."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got).any(), f"{what}: NaN"
    d = (got.double().cpu() - want).abs().max().item() if want.numel() else 0.0
    scale = ULP * want.abs().max().item() if want.numel() else 0.0
    base = max(err32, scale)
    ratio = d / base if base else 0.0
    print(f"{what}: device error {d:.3e}, float32 restatement error {err32:.3e}, one ulp at scale {scale:.3e}, ratio {ratio:.2f}")
    assert d <= FACTOR * base, f"{what}: differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"
    return ratio


def build(cfg, trainable=False):
    ac = AudioConfig()
    ac.hop_length, ac.n_mels = cfg["hop_length"], cfg["n_mels"]
    return VocosGenerator(VocosConfig(**R.model_kwargs(cfg)), ac, trainable=trainable)


def poisoned(cfg, mel, G, lens):
    """float32 device copies with NaN behind every row's frames (mel) and behind its delivered samples (d_wav)."""
    mel, G = mel.clone(), G.clone()
    B, _, T = mel.shape
    for b, t in enumerate(lens if lens is not None else [T] * B):
        mel[b, :, t:] = NAN
        G[b, R.sample_count(cfg, t):] = NAN
    return mel.float().to(DEV).contiguous(), G.float().to(DEV).contiguous()


class TrainNet:
    """The restatement ``ref`` (float64, float32-representable weights) and the device model holding the same weights."""

    def __init__(self, cfg, ref):
        self.cfg, self.ref = cfg, ref
        self.model = build(cfg)
        self.model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        self.model.to(DEV)
        self.lib = _lib.load()
        self.dims = self.model.dims()

    # ---- host arithmetic
    def tape_bytes(self, B, T):
        return self.lib.gvx_vocos_tape_bytes(C.byref(self.dims), B, T)

    def ws_bytes(self, B, T):
        return self.lib.gvx_vocos_backward_workspace_bytes(C.byref(self.dims), B, T)

    def tape_entries(self, B, T):
        n = self.lib.gvx_vocos_tape_layout(C.byref(self.dims), B, T, None, 0)
        entries = (_lib.gvx_vocos_tape_entry * n)()
        assert self.lib.gvx_vocos_tape_layout(C.byref(self.dims), B, T, entries, n) == n
        return [(e.byte_offset, e.rows, e.channels) for e in entries]

    def tape_views(self, tape, B, T):
        """The tape's tensors behind the mel, as float32 [B, T, C] views in the device's order."""
        out = []
        for off, rows, ch in self.tape_entries(B, T)[1:]:
            out.append(tape[off // 4:off // 4 + B * rows * ch].view(B, rows, ch))
        return out

    def mel_view(self, tape, B, T):
        off, rows, ch = self.tape_entries(B, T)[0]
        return tape[off // 4:off // 4 + B * rows * ch].view(B, rows, ch)

    # ---- calls
    def _stream(self):
        return torch.cuda.current_stream(torch.device(DEV)).cuda_stream

    def forward(self, mel_d, lens_d=None):
        B, _, T = mel_d.shape
        ws = torch.full((self.model.workspace_bytes(B, T) // 4,), NAN, dtype=torch.float32, device=DEV).view(torch.uint8)
        return self.model.vocode(mel_d, lens_d, workspace=ws)

    def forward_train_rc(self, mel_d, lens_d, wav, tape, tape_bytes, ws=None, ws_bytes=None):
        B, _, T = mel_d.shape
        h = self.model._ensure_packed()
        if ws is None:
            ws = torch.full((self.model.workspace_bytes(B, T) // 4,), NAN, dtype=torch.float32, device=DEV)
            ws_bytes = ws.numel() * 4
        return self.lib.gvx_vocos_forward_train(h, mel_d.data_ptr(), lens_d.data_ptr() if lens_d is not None else None, B, T, wav.data_ptr(),
                                                tape.data_ptr(), tape_bytes, ws.data_ptr(), ws_bytes, self._stream())

    def forward_train(self, mel_d, lens_d=None):
        B, _, T = mel_d.shape
        need = self.tape_bytes(B, T)
        assert need % 4 == 0 and need > 0
        tape = torch.full((need // 4,), NAN, dtype=torch.float32, device=DEV)
        wav = torch.full((B, T * self.cfg["hop_length"]), NAN, dtype=torch.float32, device=DEV)
        _lib.check(self.forward_train_rc(mel_d, lens_d, wav, tape, need))
        torch.cuda.synchronize()
        return wav, tape

    def new_grads(self, want_mel, B, T):
        grads = {k: torch.full(p.shape, NAN, dtype=torch.float32, device=DEV) for k, p in self.model.named_parameters()}
        if want_mel:
            grads["mel"] = torch.full((B, self.cfg["n_mels"], T), NAN, dtype=torch.float32, device=DEV)
        return grads

    def backward_rc(self, G_d, lens_d, B, T, tape, tape_bytes, grads, ws, ws_bytes, skip=(), numel=None, null=(), skip_raw=()):
        named = dict(self.model.named_parameters())
        raw = [(k, p.detach()) for k, p in named.items() if ".convnext." in k and k.split(".", 3)[3] in RAW and k not in skip_raw]
        raw_table, n_raw = _weight_table(raw)
        keys = [k for k in grads if k != "mel" and k not in skip]
        table = (_lib.gvx_weight_desc * len(keys))()
        for i, k in enumerate(keys):
            table[i] = _lib.gvx_weight_desc(k.encode(), None if k in null else grads[k].data_ptr(), (numel or {}).get(k, grads[k].numel()))
        d_mel = grads.get("mel")
        return self.lib.gvx_vocos_backward(self.model._handle, G_d.data_ptr(), lens_d.data_ptr() if lens_d is not None else None, B, T, tape.data_ptr(),
                                           tape_bytes, raw_table, n_raw, table, len(keys), d_mel.data_ptr() if d_mel is not None else None,
                                           ws.data_ptr(), ws_bytes, self._stream())

    def backward(self, G_d, lens_d, B, T, tape, want_mel=True):
        need = self.ws_bytes(B, T)
        assert need % 256 == 0 and need > 0
        ws = torch.full((need // 4,), NAN, dtype=torch.float32, device=DEV)
        grads = self.new_grads(want_mel, B, T)
        self.model._ensure_packed()
        _lib.check(self.backward_rc(G_d, lens_d, B, T, tape, tape.numel() * 4, grads, ws, need))
        torch.cuda.synchronize()
        return grads


def compare_mel_slot(net, tape, mel, lens, what):
    """The tape's first tensor, exactly: the mel transposed at rows 3 .. T + 2 of [B][T + 6][Cp], and exact zeros in the 3-frame halos, in
    the channel padding and at and behind every row's length - what the embedding's weight gradient reads through its row map."""
    B, M, T = mel.shape
    got = net.mel_view(tape, B, T).cpu()
    want = torch.zeros_like(got)
    for b, t in enumerate(lens if lens is not None else [T] * B):
        want[b, 3:3 + t, :M] = mel[b, :, :t].t().float()
    assert got.shape == (B, T + 6, (M + 3) // 4 * 4)
    assert torch.equal(got, want), f"{what}: the tape's haloed transposed mel is not the mel with zeros around it"


def compare_tape(views, ref, lens, what):
    """Every tape tensor behind the mel against float64; exact zeros behind every row."""
    worst = 0.0
    assert len(views) == len(ref["tape"])
    for i, (v, want, e) in enumerate(zip(views, ref["tape"], ref["tape_err"])):
        if lens is not None:
            for b, t in enumerate(lens):
                assert not v[b, t:].any(), f"{what}: tape tensor {i}: row {b} is not zero behind its {t} frames"
        worst = max(worst, bound_check(v, want, e, f"{what}: tape {i}"))
    return worst


def compare_grads(grads, ref, what):
    worst = 0.0
    for k, want in ref["grads"].items():
        worst = max(worst, bound_check(grads[k], want, ref["grad_err"][k], f"{what}: d {k}"))
    if "mel" in grads:
        worst = max(worst, bound_check(grads["mel"], ref["mel"], ref["mel_err"], f"{what}: d mel"))
    print(f"{what}: largest gradient error / bound {worst / FACTOR:.3f}")
    return worst
