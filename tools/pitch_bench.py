"""Time gvx_pitch_yin at the default parameters against the same sums written in torch on the device.

    python tools/pitch_bench.py [--rows 32] [--frames 800] [--runs 20] [--warmup 3]

The workload: `rows` waveforms of `frames` * 256 samples at 22050 Hz, hop 256, W 1024, lags 44 - 368.  Both sides are timed with device
events, alternating, after a warm-up; the median and the spread (min .. max) of the runs are printed with the kernel's rates:

    flops  3 per term (subtract, multiply, add): 3 * W * (lag_max + 1) per frame
    LDS    per wave and 64 terms of three lags: one 256-byte read of x[s + j] and 64 reads of 256 bytes of x[s + j + tau]
    bytes  the samples once in, three floats per frame out

The torch baseline is what a user would otherwise run: `unfold` of the padded rows into frames of W + lag_max samples, one batched
difference per lag, `cumsum`, and the scan as tensor operations (first lag under the threshold, then the walk to the local minimum
by a running comparison).  One JSON line at the end."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from genvox_amd import metrics  # noqa: E402

RATE, HOP, W, LAG_MIN, LAG_MAX, THRESHOLD = 22050, 256, 1024, 44, 368, 0.15


def torch_yin(x: torch.Tensor, chunk: int = 800) -> torch.Tensor:
    """f0 [B, F] by the definition of include/genvox_amd.h in tensor operations (fp32; frames in chunks to bound the memory)."""
    B, N = x.shape
    F = (N + HOP - 1) // HOP
    half = (W + LAG_MAX) // 2
    padded = torch.nn.functional.pad(x, (half, W + LAG_MAX + F * HOP - N))
    frames = padded.unfold(1, W + LAG_MAX, HOP)[:, :F].reshape(B * F, W + LAG_MAX)
    out = torch.empty(B * F, device=x.device)
    lags = torch.arange(LAG_MAX + 1, device=x.device, dtype=torch.float32)
    for lo in range(0, B * F, chunk):
        fr = frames[lo:lo + chunk]
        head = fr[:, :W]
        d = torch.stack([((head - fr[:, t:t + W]) ** 2).sum(dim=1) for t in range(LAG_MAX + 1)], dim=1)
        run = torch.cumsum(d[:, 1:], dim=1)
        c = torch.ones_like(d)
        c[:, 1:] = torch.where(run > 0, d[:, 1:] * lags[1:] / run, torch.ones_like(run))
        search = c[:, LAG_MIN:LAG_MAX]
        under = search < THRESHOLD
        voiced = under.any(dim=1)
        first = torch.where(voiced, under.to(torch.int32).argmax(dim=1), torch.zeros_like(voiced, dtype=torch.int64))
        # the walk: from `first` on, the run of strictly falling values
        falling = torch.ones_like(search, dtype=torch.bool)
        falling[:, 1:] = search[:, 1:] < search[:, :-1]
        idx = torch.arange(search.shape[1], device=x.device)[None, :]
        stop = (~falling) & (idx > first[:, None])
        end = torch.where(stop.any(dim=1), stop.to(torch.int32).argmax(dim=1), torch.full_like(first, search.shape[1])) - 1
        lag = end + LAG_MIN
        cm, c0, cp = (c.gather(1, (lag + k)[:, None])[:, 0] for k in (-1, 0, 1))
        den = cm - 2 * c0 + cp
        shift = torch.where(den > 0, ((cm - cp) / (2 * den)).clamp(-1, 1), torch.zeros_like(den))
        out[lo:lo + chunk] = torch.where(voiced, RATE / (lag + shift), torch.zeros_like(den))
    return out.reshape(B, F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pitch_bench needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    n = a.frames * HOP
    g = torch.Generator(device=dev).manual_seed(0)
    f = 110.0 * 2.0 ** (1.5 * torch.arange(n, device=dev) / n)
    phase = 2 * torch.pi * torch.cumsum(f, 0) / RATE
    x = 0.3 * sum(torch.sin(h * phase) / h for h in range(1, 6)) / 1.5
    x = x[None].repeat(a.rows, 1) + 0.01 * torch.randn(a.rows, n, device=dev, generator=g)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    kernel = lambda: metrics.pitch_track(x, sampling_rate=RATE, hop_length=HOP)["f0"]
    baseline = lambda: torch_yin(x)
    for _ in range(a.warmup):
        kernel()
    baseline()
    torch.cuda.synchronize()
    tk, tb = [], []
    for i in range(a.runs):
        ms, f0 = timed(kernel)
        tk.append(ms)
        if i < a.torch_runs:
            ms, ref = timed(baseline)
            tb.append(ms)
    agree = float(((f0 > 0) == (ref > 0)).float().mean())
    both = (f0 > 0) & (ref > 0)
    worst = float(((f0 - ref).abs() / ref.clamp(min=1))[both].max()) if both.any() else 0.0
    frames = a.rows * a.frames
    med = statistics.median(tk)
    flops = 3.0 * W * (LAG_MAX + 1) * frames
    passes = -(-(LAG_MAX + 1) // 192)
    lds_bytes = frames * passes * (W / 64) * 65 * 256.0
    hbm = x.numel() * 4 + frames * 12
    res = {"rows": a.rows, "frames": a.frames, "kernel_ms_median": med, "kernel_ms_min": min(tk), "kernel_ms_max": max(tk), "runs": a.runs,
           "torch_ms_median": statistics.median(tb), "torch_ms_min": min(tb), "torch_ms_max": max(tb), "torch_runs": len(tb),
           "speedup": statistics.median(tb) / med, "flops": flops, "tflops": flops / med / 1e9, "lds_bytes": lds_bytes,
           "lds_tb_per_s": lds_bytes / med / 1e9, "hbm_bytes": hbm, "hbm_gb_per_s": hbm / med / 1e6, "voicing_agreement": agree,
           "worst_relative_f0_difference": worst}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
