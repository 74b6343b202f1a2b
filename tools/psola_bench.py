"""Time gvx_psola_plan and gvx_psola_synth apart, next to what vocoding the same batch costs.

    python tools/psola_bench.py [--rows 32] [--frames 800] [--runs 20] [--warmup 3] [--no-vocoders]

The workload: `rows` waveforms of `frames` * 256 samples at 22050 Hz, hop 256, lags 44 - 368 - a glide of five harmonics from 110 Hz
up an octave and a half with a little noise, unvoiced (noise alone) in every fifth stretch of 40 frames - tracked once by
gvx_pitch_yin, then planned and synthesised at a ratio that ramps from 0.8 to 1.25.  The two calls are timed with device events on
outputs allocated before, alternating, after a warm-up; the median and the spread (min .. max) are printed with

    marks, grains   the largest count of a row: the length of the plan's two sequential walks
    us per mark     plan time over marks + grains of the longest row: what one step of a walk costs
    synth GB/s      samples once in, once out, plus the gather of two periods per grain, over the synthesis time

and, unless --no-vocoders, the time to vocode a random mel of the same rows and frames with Griffin-Lim (32 iterations) and with the
MelGAN generator (default configuration, random weights): pitch control runs once per vocoded batch, so their ratio is the figure
of merit.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genvox_amd import _lib, metrics  # noqa: E402

RATE, HOP = 22050, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-vocoders", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("psola_bench needs the GPU: there is nothing to time without one")
    dev = "cuda:0"
    B, F, n = a.rows, a.frames, a.frames * HOP
    g = torch.Generator(device=dev).manual_seed(0)
    f = 110.0 * 2.0 ** (1.5 * torch.arange(n, device=dev) / n)
    phase = 2 * torch.pi * torch.cumsum(f, 0) / RATE
    voiced = ((torch.arange(n, device=dev) // (40 * HOP)) % 5 != 4).float()
    x = voiced * 0.3 * sum(torch.sin(h * phase) / h for h in range(1, 6)) / 1.5
    x = (x[None].repeat(B, 1) + 0.01 * torch.randn(B, n, device=dev, generator=g)).contiguous()
    lag = metrics.pitch_track(x, sampling_rate=RATE, hop_length=HOP)["lag"]
    ratio = torch.linspace(0.8, 1.25, F, device=dev)[None].repeat(B, 1).contiguous()

    lib, params = _lib.load(), metrics.psola_params(RATE, HOP)
    p_min = min(params.lag_min, params.unvoiced_period)
    K, J = lib.gvx_psola_max_marks(n, p_min), lib.gvx_psola_max_grains(n, p_min)
    ints = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    marks, periods, pos, src, counts, status, y = ints(B, K), ints(B, K), ints(B, J), ints(B, J), ints(B, 2), ints(B), torch.empty_like(x)
    stream = torch.cuda.current_stream().cuda_stream
    plan = lambda: _lib.check(lib.gvx_psola_plan(x.data_ptr(), None, lag.data_ptr(), ratio.data_ptr(), B, n, params, marks.data_ptr(), periods.data_ptr(),
                                                 pos.data_ptr(), src.data_ptr(), counts.data_ptr(), status.data_ptr(), stream))
    synth = lambda: _lib.check(lib.gvx_psola_synth(x.data_ptr(), None, marks.data_ptr(), periods.data_ptr(), pos.data_ptr(), src.data_ptr(),
                                                   counts.data_ptr(), status.data_ptr(), B, n, params, y.data_ptr(), stream))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def runs(fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t = [timed(fn) for _ in range(reps)]
        return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "runs": reps}

    for _ in range(a.warmup):
        plan()
        synth()
    torch.cuda.synchronize()
    tp, ts = [], []
    for _ in range(a.runs):
        tp.append(timed(plan))
        ts.append(timed(synth))
    host = counts.cpu()
    n_marks, n_grains = int(host[:, 0].max()), int(host[:, 1].max())
    voiced_share = float((lag >= 1).float().mean())
    grain_samples = float((2 * periods.abs().gather(1, src.clamp(0, K - 1).long()) * (torch.arange(J, device=dev)[None] < counts[:, 1:2])).sum())
    synth_bytes = 4.0 * (2 * B * n + grain_samples)
    res = {"rows": B, "frames": F, "samples": n, "runs": a.runs, "statuses": sorted(set(status.tolist())), "voiced_share": voiced_share,
           "marks_max": n_marks, "grains_max": n_grains, "capacity_marks": K, "capacity_grains": J,
           "plan_ms_median": statistics.median(tp), "plan_ms_min": min(tp), "plan_ms_max": max(tp),
           "synth_ms_median": statistics.median(ts), "synth_ms_min": min(ts), "synth_ms_max": max(ts),
           "plan_us_per_walk_step": 1e3 * statistics.median(tp) / max(1, n_marks + n_grains),
           "synth_bytes": synth_bytes, "synth_gb_per_s": synth_bytes / statistics.median(ts) / 1e6}
    print(json.dumps(res), flush=True)
    if not a.no_vocoders:
        from genvox_amd.audio import AudioProcessor
        from genvox_amd.configs import AudioConfig, MelGANConfig
        from genvox_amd.melgan import MelGANGenerator

        ac = AudioConfig(filter_length=1024, log_func="np.log")
        mel = (0.5 * torch.randn(B, ac.n_mels, F, device=dev, generator=g) - 0.5).contiguous()
        gl = AudioProcessor(ac, device=dev)
        res["griffin_lim"] = runs(lambda: gl.convert_mel2wav_batch(mel), 1, 5)
        print(json.dumps({"griffin_lim": res["griffin_lim"]}), flush=True)
        voc = MelGANGenerator(MelGANConfig(), ac).to(dev)
        res["melgan"] = runs(lambda: voc.vocode(mel), 2, 5)
        both = res["plan_ms_median"] + res["synth_ms_median"]
        res["pitch_control_over_griffin_lim"] = both / res["griffin_lim"]["median_ms"]
        res["pitch_control_over_melgan"] = both / res["melgan"]["median_ms"]
        res["plan_over_melgan"] = res["plan_ms_median"] / res["melgan"]["median_ms"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
