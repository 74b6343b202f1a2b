#!/usr/bin/env python3
"""Secondary measurements for DESIGN.md (BASELINE.json configs 2-4 beyond the headline line of bench.py):
teacher-forced at B=64, autoregressive RTF (B=64, 1000 steps), Postnet-only MFMA rate, Griffin-Lim throughput;
`glr` (on request): the ragged Griffin-Lim call against the same rows padded through the uniform call;
`w2mr` (on request): 64 recordings of 2-10 s through one ragged wav -> mel call against 64 single-row `wav_to_mel` calls;
`w2m48` (on request): 32 recordings of 10 s at 48 kHz through `convert_wav2mel_batch` (resampled on the device) against the same
batch delivered at the model's rate;
`dtw` / `align` (on request): the evaluation metrics' C-ABI calls alone between device events - gvx_dtw_distance on 32 rows of
1000 x 1000 and 800 x 800 frames of 13 cepstra (and 1000 x 1000 of 80 features, the form without LDS tables), gvx_alignment_stats
on 32 x 1000 x 128 - and the Python entry points around them by the host clock;
`melgan` (on request): the MelGAN generator at 1 x 568 and 32 x 800 frames between device events, with the time per stage, against the
same float32 network through torch's own ROCm convolutions and against Griffin-Lim (32 iterations) on the same mels;
`melgan_train` (on request): `vocode_with_grad` + `backward()` (gvx_melgan_forward_train + gvx_melgan_backward) at 16 x 32 and 8 x 128
frames between device events, against autograd through torch's own convolutions on the same parameters, with the tape's size;
`mrstft` (on request): the multi-resolution STFT loss, value + gradient (MultiResolutionSTFTLoss + `backward()`: one gvx_stft_loss call),
at 16 x 8192 and 8 x 32768 samples with the default resolutions between device events, median of 7, against the same loss written
with torch.stft + autograd on the same device, with the workspace's size;
`melloss` (on request): the mel-spectrogram L1 loss, value + gradient (MelSpectrogramLoss + `backward()`: one gvx_mel_loss call), with the
published parameters (1024 / 256 / 1024, 80 mels to Nyquist) at the `mrstft` shapes between device events, median of 7, against the same
per-row loss written with torch.stft, a matmul and autograd on the same device, with the workspace's size;
`denoise` (on request): the vocoder denoiser (Denoiser.forward: one gvx_denoise call, two launches) at 1024 / 256 at the `mrstft` shapes,
200 calls per window between device events, the windows of the two sides alternating, median and range of 7, against the same
definition through torch.stft / torch.istft on the same device, with the largest difference between the two and the workspace's size;
`melgan_disc` (on request): the MelGAN discriminator at 16 x 8192 and 8 x 32768 samples (the `mrstft` shapes) between device events,
median of 7 with the spread: forward, forward + full backward (cotangents on every map), and the whole `MelGANTrainer.train_step` with
the default generator, against the same discriminator built from torch.nn modules that hold the same (seeded) parameters, through
torch's own convolutions and autograd; with the count of LeakyReLU decisions on which the two forwards differ and the gradient
difference again with torch differentiating through the device's own decisions;
`hifigan` (on request): the HiFi-GAN generator - V1 at 1 x 568 and 32 x 800 frames, V2 at 32 x 800 - between device events, median of 7
with the spread and the time per stage, against the same float32 network built from torch.nn modules that hold the same (seeded)
parameters, through torch's own ROCm convolutions, and against `MelGANGenerator` and Griffin-Lim (32 iterations) on the same mels;
`hifigan_train` (on request): HiFi-GAN V1 `vocode_with_grad` + `backward()` (gvx_hifigan_forward_train + gvx_hifigan_backward) at 16 x 32
and 8 x 128 frames between device events, median of 7 with the spread, against autograd through the same torch.nn network, with the
forward's and the backward's time per stage from the same run and the tape's and the workspace's size;
`hifigan_mpd` (on request): HiFi-GAN's multi-period discriminator, default shape, at 16 x 8192 and 8 x 32768 samples between device events,
median of 7 with the spread: forward, forward + full backward (cotangents on every map), against torch's own Conv2d + autograd on the
same parameters; per layer the counted multiply-adds, the time (events around every layer, summed over the periods) and the share of
the fp32 matrix rate; and one `HiFiGANTrainer.train_step` of the V1 generator against the period discriminators;
`hifigan_msd` (on request): HiFi-GAN's multi-scale discriminator, published shape, the same measurement at the same two sizes against
torch's own grouped Conv1d + avg_pool1d + autograd on the same effective weights (eval mode: no power iteration), the per-layer times
summed over the scales; and one `HiFiGANTrainer.train_step` of the V1 generator against the period and the scale discriminators with
`MelSpectrogramLoss` - the published step;
`mrd` (on request): the multi-resolution spectrogram discriminator, published shape, at 16 x 8192 and 32 x 8192 samples between device
events, median of 7 with the spread: forward, forward + full backward (cotangents on every map), against torch's own stft + Conv2d +
autograd on the same device and parameters; the per-layer times summed over the resolutions (the spectrogram and its adjoint count
towards layer 0) and the backward's workspace;
`bigvgan` (on request): the BigVGAN generator - the base model at 32 x 800 and 1 x 568 frames, the large one at 8 x 200 - between device
events, median of 7 with the spread and the time per stage, against the float32 restatement of tests/bigvgan_ref64.py (torch's own ROCm
convolutions, the activation as replicate padding + grouped conv_transpose1d / conv1d) on the same device and the same parameters; and
the anti-aliased activation's launches on their own: gvx_snake_antialiased timed at every stage's shape, times the launches of that
stage, summed, as a share of one call;
`vocos` (on request): the Vocos generator, default configuration with 100 mels, at 32 x 800, 1 x 568 and 8 x 200 frames between device
events, median of 7 with the spread: ours, the float32 restatement of tests/vocos_ref64.py on the same device and parameters ("torch"),
the four stage times (embed + norm, the blocks, final norm + head product, ISTFT), and the share of the fp32 matrix rate (157.3 TFLOP/s)
that the blocks' time amounts to for their MLP products;
`vocos_train` (on request): the Vocos generator's `vocode_with_grad` + `backward()` (gvx_vocos_forward_train + gvx_vocos_backward), default
configuration with 100 mels, at 16 x 32, 8 x 128 and 32 x 800 frames between device events, median and range of 7, against torch autograd
of the float32 restatement on the same device, with the backward's four part times, the blocks' product rate against 157.3 TFLOP/s and
the tape's and the workspace's size;
`fastpitch` (on request): the FastPitch acoustic model, published sizes, on given durations - 32 x 128 tokens -> 800 frames, 1 x 100 tokens
-> 568 frames, 8 x 40 tokens -> 200 frames - between device events, median of 7 with the spread: ours (both phases and the read-back of
the frame counts), the float32 restatement of tests/fastpitch_ref64.py run as a batch on the same device with the same weights ("torch":
F.scaled_dot_product_attention, Conv1d, LayerNorm), the four stage times (embedding + encoder, predictors + plan + regulator, decoder,
projection), the decoder's share of the fp32 matrix rate, and gvx_self_attention on its own at 32 x 800 and 1 x 568 against torch's;
`univnet` (on request): the UnivNet generator - c32 with 100 mels at 32 x 800, 1 x 568 and 8 x 200 frames, c16 at 32 x 800 - between device
events, median of 7 with the spread: ours as delivered (the row split under the workspace cap included), the float32 restatement of
tests/univnet_ref64.py on the same device with the same weights and noise ("torch", 8 rows at a time), the stage times of one call
(conv_pre, per block the predictor and the layers, conv_post), the fp32 matrix rate of kernel_conv + bias_conv timed on its own (the same product through gvx_train_gemm_nt) and
against each predictor's whole time, and gvx_lvc_gated timed on its own at every block's shape: its rate against 157.3 TFLOP/s and the rate at which it reads weights."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from genvox_amd import weights as gw
from genvox_amd.audio import AudioProcessor
from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
from genvox_amd.tacotron2 import Tacotron2


def timed(fn, warm=1, reps=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    which = set(sys.argv[1:]) or {"tf64", "ar", "postnet", "gl"}
    mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024, hop_length=256, log_func="np.log"), TextConfig(n_tokens=40)
    res = {}
    if which & {"tf64", "ar", "ar1", "postnet"}:
        model = Tacotron2(mc, ac, tc)
        model.load_state_dict(gw.generate_state_dict(mc, ac, tc, seed=0))
        model = model.to("cuda:0")
    if "tf64" in which:
        B, L, T = 64, 128, 800
        batch = {k: torch.from_numpy(v).cuda() for k, v in gw.synthetic_inputs(B, L, T, 40, 80, seed=3).items()}
        dt = timed(lambda: model.forward(batch), warm=2, reps=5)
        res["teacher_forced_b64"] = {"ms": round(dt * 1e3, 2), "mel_frames_per_s": round(B * T / dt)}
    if "ar" in which:
        B, L = 64, 128
        mc.gate_threshold = 1.0  # never fires: exactly max_decoder_steps = 1000 frames (BASELINE config 3)
        tok = torch.from_numpy(gw.synthetic_inputs(B, L, 8, 40, 80, seed=3)["token_padded"]).cuda()
        dt = timed(lambda: model.inference({"tokens": tok}), warm=1, reps=2)
        audio_s = mc.max_decoder_steps * ac.hop_length / ac.sampling_rate
        res["autoregressive_b64_1000steps"] = {"ms": round(dt * 1e3, 1), "us_per_step": round(dt / mc.max_decoder_steps * 1e6, 1),
                                               "rtf_per_utterance_stream": round(dt / audio_s, 5),
                                               "rtf_aggregate": round(dt / (audio_s * B), 6),
                                               "mel_frames_per_s": round(B * mc.max_decoder_steps / dt)}
        mc.gate_threshold = 0.5
    if "ar1" in which:   # the reference's own autoregressive shape: one utterance
        mc.gate_threshold = 1.0
        tok = torch.from_numpy(gw.synthetic_inputs(1, 128, 8, 40, 80, seed=3)["token_padded"]).cuda()
        dt = timed(lambda: model.inference({"tokens": tok}), warm=1, reps=2)
        audio_s = mc.max_decoder_steps * ac.hop_length / ac.sampling_rate
        res["autoregressive_b1_1000steps"] = {"ms": round(dt * 1e3, 1), "us_per_step": round(dt / mc.max_decoder_steps * 1e6, 1),
                                              "rtf": round(dt / audio_s, 5)}
    if "postnet" in which:
        B, T = 256, 800
        mel = torch.randn(64, 80, T, device="cuda")
        dt = timed(lambda: model.postnet_residual(mel), warm=1, reps=3) * (B / 64)
        flops = 8.68e6 * B * T
        res["postnet_b256x800"] = {"ms": round(dt * 1e3, 2), "tflops": round(flops / dt / 1e12, 1), "frac_of_157TF_fp32_mfma": round(flops / dt / 157.3e12, 3),
                                   "note": "4 calls of 64 rows (C-ABI batch limit)"}
    if "gl" in which:
        ap = AudioProcessor(ac)
        B, T, it = 256, 800, 60
        mel = torch.randn(B, 80, T, device="cuda") * 1.5 - 4.0
        mag = ap.mel_to_magnitude(mel)
        dt = timed(lambda: ap.griffin_lim(mag, n_iter=it, want_phase=False), warm=1, reps=2)
        res["griffin_lim_b256x800_60it"] = {"ms": round(dt * 1e3, 1), "frames_per_s": round(B * T / dt),
                                            "GBs_vs_min_fused_traffic": round(20516 * B * T * it / dt / 1e9),
                                            "utterances_per_s": round(B / dt, 1)}
        dt2 = timed(lambda: ap.convert_mel2wav_batch(mel, n_iter=32), warm=1, reps=2)
        res["convert_mel2wav_b256x800_32it"] = {"ms": round(dt2 * 1e3, 1), "utterances_per_s": round(B / dt2, 1)}
        sig = torch.rand(B, 1024 + (T - 1) * 256, device="cuda") * 2 - 1
        dt3 = timed(lambda: ap.wav_to_mel(sig), warm=1, reps=3)
        os.environ["GVX_GL_ROCFFT"] = "1"
        dt4 = timed(lambda: ap.wav_to_mel(sig), warm=1, reps=3)
        del os.environ["GVX_GL_ROCFFT"]
        res["wav_to_mel_b256x800"] = {"ms": round(dt3 * 1e3, 2), "frames_per_s": round(B * T / dt3), "ms_rocfft_pipeline": round(dt4 * 1e3, 2)}
    if "glr" in which:
        # ragged Griffin-Lim: 64 rows with frame counts spread evenly over 200-800, in one ragged call, against the same rows
        # padded to 800 through the uniform call (the padding's workgroups return at once: time should follow the sum of frames)
        ap = AudioProcessor(ac)
        B, T, it = 64, 800, 60
        lens = [200 + (600 * i) // (B - 1) for i in range(B)]
        lens = [lens[(i * 29) % B] for i in range(B)]            # not sorted: neighbours in the grid differ in length
        mag = ap.mel_to_magnitude(torch.randn(B, 80, T, device="cuda") * 1.5 - 4.0)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")

        def runs(fn, warm=2, reps=7):   # every run timed on its own: the spread goes next to the mean
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return {"mean_ms": round(sum(out) / len(out), 2), "min_ms": round(min(out), 2), "max_ms": round(max(out), 2), "runs": reps}

        padded = runs(lambda: ap.griffin_lim(mag, n_iter=it, want_phase=False))
        ragged = runs(lambda: ap.griffin_lim(mag, n_iter=it, want_phase=False, frame_lengths=lens_dev))
        full = runs(lambda: ap.griffin_lim(mag, n_iter=it, want_phase=False, frame_lengths=[T] * B))
        res["griffin_lim_ragged_b64_200to800_60it"] = {
            "padded_uniform": padded, "ragged": ragged, "ragged_all_rows_full_length": full,
            "frames_share": round(sum(lens) / (B * T), 3), "time_share": round(ragged["mean_ms"] / padded["mean_ms"], 3)}
    if "w2mr" in which:
        # ragged wav -> mel: 64 int16 recordings with lengths spread evenly over 2-10 s at 22 050 Hz, (a) through one
        # wav_to_mel_ragged call (trimming and normalisation on the device, one synchronisation), (b) the per-file route: peak
        # normalisation in NumPy on the host, one wav_to_mel call per recording, each result copied back like convert_wav2mel does.
        # Both sides produce every mel on the host-visible side of one synchronisation per batch / per file; 7 runs each.
        import statistics

        import numpy as np

        ap = AudioProcessor(AudioConfig(sampling_rate=22050, filter_length=1024, hop_length=256, log_func="np.log"))
        B, fs = 64, 22050
        rng = np.random.default_rng(0)
        secs = [2.0 + 8.0 * i / (B - 1) for i in range(B)]
        secs = [secs[(i * 29) % B] for i in range(B)]            # not sorted
        rows = [rng.integers(-12000, 12001, size=int(s * fs)).astype(np.int16) for s in secs]
        n_max = max(r.shape[0] for r in rows)
        pcm = np.zeros((B, n_max), np.int16)
        for b, r in enumerate(rows):
            pcm[b, : r.shape[0]] = r
        lengths = [r.shape[0] for r in rows]
        pcm_dev = torch.from_numpy(pcm).cuda()

        def runs(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return {"median_ms": round(statistics.median(out), 2), "min_ms": round(min(out), 2), "max_ms": round(max(out), 2), "runs": reps}

        def per_file():
            for r in rows:
                sig = (r / max(np.abs(np.min(r)), np.abs(np.max(r)))).astype(np.float32)
                ap.wav_to_mel(torch.from_numpy(sig)[None])[0].cpu()

        ragged_host = runs(lambda: ap.wav_to_mel_ragged(pcm, lengths))          # padded batch starts on the host (upload included)
        ragged_dev = runs(lambda: ap.wav_to_mel_ragged(pcm_dev, lengths))       # padded batch already on the device
        single = runs(per_file)
        frames = sum((n - 1024) // 256 + 1 for n in lengths)
        res["wav_to_mel_ragged_b64_2to10s"] = {
            "ragged_from_host_int16": ragged_host, "ragged_from_device_int16": ragged_dev, "single_row_calls_x64": single,
            "frames": frames, "padded_frames": B * ((n_max - 1024) // 256 + 1), "seconds_of_audio": round(sum(lengths) / fs, 1)}
    if "w2m48" in which:
        # resample + wav -> mel: 32 int16 recordings of 10 s, (a) at 48 kHz through convert_wav2mel_batch (resampled to 22 050 Hz on the
        # device, then one ragged wav -> mel call), (b) the same durations delivered at 22 050 Hz (today's path), (c) the resampler alone
        # on a batch that is already on the device.  Host arrays in, host mels out, as a preprocessing job calls it; 7 runs each.
        import statistics

        import numpy as np

        ap = AudioProcessor(AudioConfig(sampling_rate=22050, filter_length=1024, hop_length=256, log_func="np.log"))
        B, seconds = 32, 10
        rng = np.random.default_rng(0)
        at48 = [rng.integers(-12000, 12001, size=seconds * 48000).astype(np.int16) for _ in range(B)]
        at22 = [rng.integers(-12000, 12001, size=seconds * 22050).astype(np.int16) for _ in range(B)]
        dev48 = torch.from_numpy(np.stack(at48)).cuda()

        def runs(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return {"median_ms": round(statistics.median(out), 2), "min_ms": round(min(out), 2), "max_ms": round(max(out), 2), "runs": reps}

        foreign = runs(lambda: ap.convert_wav2mel_batch(at48, sample_rates=48000))
        native = runs(lambda: ap.convert_wav2mel_batch(at22))
        alone = runs(lambda: ap.resample(dev48, 48000, sample_lengths=[seconds * 48000] * B))
        outputs, taps = B * seconds * 22050, ap._resample_table(48000, 22050, False)[2]
        res["convert_wav2mel_batch_b32_10s"] = {
            "at_48k_resampled_on_device": foreign, "at_model_rate": native, "resample_kernel_alone_device_batch": alone,
            "cost_ratio": round(foreign["median_ms"] / native["median_ms"], 2), "outputs": outputs, "taps_per_phase": taps,
            "resample_gflop": round(2e-9 * outputs * taps, 2)}
    if which & {"dtw", "align"}:
        import statistics

        from genvox_amd import _lib, metrics

        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream

        def event_runs(fn, warm=3, reps=20):   # one C-ABI call per run, between device events: its launches and nothing else
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        def host_runs(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        gen = torch.Generator(device="cuda").manual_seed(0)
    if "dtw" in which:
        B = 32
        for Tp, Tg, K in ((1000, 1000, 13), (800, 800, 13), (1000, 1000, 80)):
            # random walks: neighbouring frames are close, as cepstra of speech are
            cp = torch.randn(B, Tp, K, device="cuda", generator=gen).mul_(0.3).cumsum(dim=1).contiguous()
            cg = torch.randn(B, Tg, K, device="cuda", generator=gen).mul_(0.3).cumsum(dim=1).contiguous()
            dist = torch.empty(B, device="cuda")
            ws = torch.empty(lib.gvx_dtw_workspace_bytes(B, Tp, Tg, K), dtype=torch.uint8, device="cuda")
            call = lambda: _lib.check(lib.gvx_dtw_distance(cp.data_ptr(), cg.data_ptr(), None, None, B, Tp, Tg, K, dist.data_ptr(), None,
                                                           ws.data_ptr() if ws.numel() else None, ws.numel(), stream))
            r = event_runs(call)
            r.update(lds_tables=lib.gvx_dtw_uses_lds_tables(Tp, Tg, K), cells=B * Tp * Tg, finite=bool(torch.isfinite(dist).all()))
            res[f"gvx_dtw_distance_b32_{Tp}x{Tg}_k{K}"] = r
        mel_p = torch.randn(B, 80, 1000, device="cuda", generator=gen).mul_(0.2).cumsum(dim=2)
        mel_g = torch.randn(B, 80, 1000, device="cuda", generator=gen).mul_(0.2).cumsum(dim=2)
        res["dtw_mel_distance_b32_1000x1000_with_projection"] = host_runs(lambda: metrics.dtw_mel_distance(mel_p, mel_g))
    if "align" in which:
        B, T, L = 32, 1000, 128
        a = torch.softmax(torch.randn(B, T, L, device="cuda", generator=gen) * 4.0, dim=-1).contiguous()
        pos, dur = torch.empty(B, T, dtype=torch.int32, device="cuda"), torch.empty(B, L, dtype=torch.int32, device="cuda")
        peaks, ints, focus = torch.empty(B, T, device="cuda"), torch.empty(B, 5, dtype=torch.int32, device="cuda"), torch.empty(B, device="cuda")
        call = lambda: _lib.check(lib.gvx_alignment_stats(a.data_ptr(), None, None, B, T, L, pos.data_ptr(), dur.data_ptr(), peaks.data_ptr(),
                                                          ints.data_ptr(), focus.data_ptr(), stream))
        r = event_runs(call)
        r.update(input_mb=round(a.numel() * 4 / 1e6, 1), gb_per_s=None)
        r["gb_per_s"] = round(a.numel() * 4 / 1e9 / (r["median_ms"] * 1e-3), 1)
        res[f"gvx_alignment_stats_b{B}_{T}x{L}"] = r
        res[f"alignment_stats_python_b{B}_{T}x{L}"] = host_runs(lambda: metrics.alignment_stats(a))
    if which & {"melgan", "melgan_train"}:
        import statistics

        import torch.nn.functional as F

        import ctypes as C

        from genvox_amd import _lib
        from genvox_amd.configs import MelGANConfig
        from genvox_amd.melgan import MelGANGenerator

        def ev_runs(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        gmc = MelGANConfig()
        voc = MelGANGenerator(gmc, ac).to("cuda:0")
        with torch.no_grad():
            for name, p in voc.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.1 * torch.randn_like(p))
        sd = {k: v.detach() for k, v in voc.state_dict().items()}

        def torch_net(mel):   # the same float32 network through torch's own convolutions
            x = F.conv1d(F.pad(mel, (3, 3), mode="reflect"), sd["pre.weight"], sd["pre.bias"])
            for i, r in enumerate(gmc.upsample_ratios):
                x = F.conv_transpose1d(F.leaky_relu(x, 0.2), sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=r, padding=r // 2)
                for j in range(gmc.n_residual_layers):
                    d, p = gmc.dilation_base ** j, f"res.{i}.{j}."
                    h = F.conv1d(F.pad(F.leaky_relu(x, 0.2), (d, d), mode="reflect"), sd[p + "conv.weight"], sd[p + "conv.bias"], dilation=d)
                    x = F.conv1d(x, sd[p + "shortcut.weight"], sd[p + "shortcut.bias"]) + F.conv1d(F.leaky_relu(h, 0.2), sd[p + "mix.weight"], sd[p + "mix.bias"])
            return torch.tanh(F.conv1d(F.pad(F.leaky_relu(x, 0.2), (3, 3), mode="reflect"), sd["post.weight"], sd["post.bias"]))[:, 0]

        ap = AudioProcessor(ac, device="cuda:0")
        gen = torch.Generator(device="cuda").manual_seed(0)
        for B, T in ((1, 568), (32, 800)) if "melgan" in which else ():
            key = f"melgan_{B}x{T}"
            mel = (0.5 * torch.randn(B, 80, T, device="cuda", generator=gen) - 0.5).contiguous()
            res[key] = {"as_delivered": ev_runs(lambda: voc.vocode(mel)), "rows_per_call_as_delivered": None}
            rows = B
            while rows > 1 and voc.workspace_bytes(rows, T) > voc.WORKSPACE_CAP_BYTES:
                rows = (rows + 1) // 2
            res[key]["rows_per_call_as_delivered"] = rows
            cap, voc.WORKSPACE_CAP_BYTES = voc.WORKSPACE_CAP_BYTES, 1 << 40   # one call for all rows: the stage times are of one call
            res[key]["one_call"] = ev_runs(lambda: voc.vocode(mel))
            voc.enable_stage_timing(True)
            per = []
            for _ in range(5):
                wav = voc.vocode(mel)
                per.append(voc.stage_times_ms())
            voc.enable_stage_timing(False)
            res[key]["stage_ms_median"] = [round(statistics.median(col), 3) for col in zip(*per)]   # first conv, stages 0 .. 3, output layer
            voc.WORKSPACE_CAP_BYTES, voc._workspace = cap, None
            print(json.dumps({key: res[key]}), flush=True)
            res[key]["griffin_lim_32it"] = ev_runs(lambda: ap.convert_mel2wav_batch(mel), warm=1, reps=5)
            print(json.dumps({key: res[key]["griffin_lim_32it"]}), flush=True)
            with torch.no_grad():
                res[key]["torch_convolutions"] = ev_runs(lambda: torch_net(mel), warm=2, reps=5)
                res[key]["max_abs_difference_from_torch"] = float((torch_net(mel) - wav).abs().max())
            print(json.dumps({key: res[key]["torch_convolutions"]}), flush=True)
        for B, T in ((16, 32), (8, 128)) if "melgan_train" in which else ():   # a training segment; a longer one
            key = f"melgan_train_{B}x{T}"
            mel = (0.5 * torch.randn(B, 80, T, device="cuda", generator=gen) - 0.5).contiguous()
            cot = torch.randn(B, T * voc.hop, device="cuda", generator=gen)
            params = list(voc.parameters())

            def ours():
                for p in params:
                    p.grad = None
                (voc.vocode_with_grad(mel) * cot).sum().backward()

            def torchs():   # autograd through torch's own convolutions, the same parameters
                for p in params:
                    p.grad = None
                (torch_net(mel) * cot).sum().backward()

            res[key] = {"forward_train_plus_backward": ev_runs(ours, warm=2, reps=7),
                        "tape_mb": round(_lib.load().gvx_melgan_tape_bytes(C.byref(voc.dims()), B, T) / 1e6, 1),
                        "backward_workspace_mb": round(_lib.load().gvx_melgan_backward_workspace_bytes(C.byref(voc.dims()), B, T) / 1e6, 1)}
            got = {k: p.grad.clone() for k, p in voc.named_parameters()}
            sd = dict(voc.named_parameters())   # torch_net reads sd: now the parameters themselves, so autograd reaches them
            res[key]["torch_autograd"] = ev_runs(torchs, warm=2, reps=5)
            res[key]["max_relative_gradient_difference_from_torch"] = max(
                float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in voc.named_parameters())
            sd = {k: v.detach() for k, v in voc.state_dict().items()}
            print(json.dumps({key: res[key]}), flush=True)
    if "mrstft" in which:
        import statistics

        from genvox_amd.losses import DEFAULT_RESOLUTIONS, MultiResolutionSTFTLoss

        def ev_median(fn, warm=3, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        windows = [torch.hann_window(w, periodic=True, device="cuda") for _, _, w in DEFAULT_RESOLUTIONS]

        def torch_loss(p, t):   # the header's definition on rows of full length: norms and means per row
            total = 0.0
            for (n_fft, hop, wl), w in zip(DEFAULT_RESOLUTIONS, windows):
                m = []
                for x in (p, t):
                    X = torch.stft(x, n_fft, hop, wl, w, center=True, pad_mode="reflect", return_complex=True)
                    m.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=1e-7)))
                sc = torch.linalg.norm(m[1] - m[0], dim=(1, 2)) / torch.linalg.norm(m[1], dim=(1, 2))
                total = total + (sc + (m[1].log() - m[0].log()).abs().mean(dim=(1, 2))).mean()
            return total / len(DEFAULT_RESOLUTIONS)

        crit = MultiResolutionSTFTLoss()
        gen = torch.Generator(device="cuda").manual_seed(0)
        for B, n in ((16, 8192), (8, 32768)):
            key = f"mrstft_{B}x{n}"
            pred = (0.3 * torch.randn(B, n, device="cuda", generator=gen)).requires_grad_(True)
            target = 0.3 * torch.randn(B, n, device="cuda", generator=gen)

            def ours():
                pred.grad = None
                crit(pred, target).backward()

            def torchs():
                pred.grad = None
                torch_loss(pred, target).backward()

            res[key] = {"value_plus_gradient": ev_median(ours)}
            got, got_loss = pred.grad.clone(), float(crit(pred, target))
            with torch.no_grad():
                res[key]["value_alone"] = ev_median(lambda: crit(pred, target))
            res[key]["torch_stft_autograd"] = ev_median(torchs)
            res[key]["relative_loss_difference_from_torch"] = abs(got_loss - float(torch_loss(pred, target))) / got_loss
            res[key]["max_relative_gradient_difference_from_torch"] = float((got - pred.grad).abs().max() / pred.grad.abs().max())
            res[key]["workspace_mb"] = round(crit._workspace.numel() / 1e6, 1)
            print(json.dumps({key: res[key]}), flush=True)
    if "melloss" in which:
        import statistics

        from genvox_amd.losses import MelSpectrogramLoss

        def ev_median(fn, warm=3, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        crit = MelSpectrogramLoss()
        basis = torch.from_numpy(crit.mel_basis).to("cuda")
        window = torch.hann_window(crit.win_length, periodic=True, device="cuda")

        def torch_loss(p, t):   # the header's definition on rows of full length: the published mel_spectrogram, the mean per row
            logs = []
            for x in (p, t):
                x = torch.nn.functional.pad(x.unsqueeze(1), (crit.pad, crit.pad), mode="reflect").squeeze(1)
                X = torch.stft(x, crit.n_fft, crit.hop_length, crit.win_length, window, center=False, return_complex=True)
                S = torch.sqrt(X.real ** 2 + X.imag ** 2 + crit.mag_eps)
                logs.append(torch.log(torch.clamp(torch.matmul(basis, S), min=crit.clamp)))
            return (logs[1] - logs[0]).abs().mean(dim=(1, 2)).mean()

        gen = torch.Generator(device="cuda").manual_seed(0)
        for B, n in ((16, 8192), (8, 32768)):
            key = f"melloss_{B}x{n}"
            pred = (0.3 * torch.randn(B, n, device="cuda", generator=gen)).requires_grad_(True)
            target = 0.3 * torch.randn(B, n, device="cuda", generator=gen)

            def ours():
                pred.grad = None
                crit(pred, target).backward()

            def torchs():
                pred.grad = None
                torch_loss(pred, target).backward()

            res[key] = {"value_plus_gradient": ev_median(ours)}
            got, got_loss = pred.grad.clone(), float(crit(pred, target))
            with torch.no_grad():
                res[key]["value_alone"] = ev_median(lambda: crit(pred, target))
            res[key]["torch_stft_matmul_autograd"] = ev_median(torchs)
            res[key]["relative_loss_difference_from_torch"] = abs(got_loss - float(torch_loss(pred, target))) / got_loss
            res[key]["max_relative_gradient_difference_from_torch"] = float((got - pred.grad).abs().max() / pred.grad.abs().max())
            res[key]["workspace_mb"] = round(crit._workspace.numel() / 1e6, 1)
            print(json.dumps({key: res[key]}), flush=True)
    if "denoise" in which:
        import statistics

        from genvox_amd.denoiser import Denoiser

        n_fft, hop, strength, inner = 1024, 256, 0.5, 200
        gen = torch.Generator(device="cuda").manual_seed(0)
        bias = torch.rand(n_fft // 2 + 1, device="cuda", generator=gen) * 20.0   # around the magnitudes of 0.3-sigma noise: part of the bins clamp
        dn = Denoiser(bias, n_fft, hop, strength).to("cuda")
        window = torch.hann_window(n_fft, periodic=True, device="cuda")

        def torch_denoise(x):   # the header's definition on rows of full length
            X = torch.stft(x, n_fft, hop, n_fft, window, center=True, pad_mode="reflect", return_complex=True)
            M = torch.sqrt(X.real ** 2 + X.imag ** 2)
            live = M > 0
            g = torch.where(live, torch.clamp(M - strength * bias[None, :, None], min=0.0) / torch.where(live, M, torch.ones_like(M)), torch.zeros_like(M))
            return torch.istft(X * g, n_fft, hop, n_fft, window, center=True, length=x.shape[1])

        def window_ms(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / inner

        def stats(out):
            return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "runs": len(out),
                    "calls_per_run": inner}

        for B, n in ((16, 8192), (8, 32768)):
            key = f"denoise_{B}x{n}"
            wav = 0.3 * torch.randn(B, n, device="cuda", generator=gen)
            with torch.no_grad():
                for _ in range(3):   # warm both sides at this shape
                    got, want = dn(wav), torch_denoise(wav)
                ours, theirs = [], []
                for _ in range(7):   # the two sides alternate, so that what else runs on the machine meets both
                    ours.append(window_ms(lambda: dn(wav)))
                    theirs.append(window_ms(lambda: torch_denoise(wav)))
                clamped = float(((torch.stft(wav, n_fft, hop, n_fft, window, return_complex=True).abs() <= strength * bias[None, :, None])).float().mean())
            res[key] = {"gvx_denoise": stats(ours), "torch_stft_istft": stats(theirs),
                        "max_abs_difference_from_torch": float((got - want).abs().max()), "max_abs_output": float(want.abs().max()),
                        "clamped_fraction": round(clamped, 3), "workspace_mb": round(dn._workspace.numel() / 1e6, 1)}
            print(json.dumps({key: res[key]}), flush=True)
    if "melgan_disc" in which:
        import statistics


        from genvox_amd.configs import MelGANConfig, MelGANDiscriminatorConfig
        from genvox_amd.melgan import MelGANGenerator
        from genvox_amd.melgan_disc import MelGANDiscriminator
        from genvox_amd.melgan_training import MelGANTrainer

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        torch.manual_seed(0)   # the same weights every run: the differences from torch below are comparable between runs
        dc = MelGANDiscriminatorConfig()
        disc = MelGANDiscriminator(dc).to("cuda:0")
        with torch.no_grad():
            for name, p in disc.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.1 * torch.randn_like(p))
        dparams = dict(disc.named_parameters())
        shapes = dc.layer_shapes()

        class TorchDisc(torch.nn.Module):
            """The same float32 network from torch.nn modules; its convolutions hold the discriminator's own parameters.  ``pin``:
            [scale][map] masks in {1, slope} that replace every LeakyReLU by a product (the device's own decisions)."""

            def __init__(self):
                super().__init__()
                self.pad, self.act = torch.nn.ReflectionPad1d(7), torch.nn.LeakyReLU(dc.leaky_slope)
                self.pool = torch.nn.AvgPool1d(4, stride=2, padding=1, count_include_pad=False)
                self.scales = torch.nn.ModuleList()
                for k in range(dc.n_scales):
                    convs = torch.nn.ModuleList()
                    for i, (ci, co, kk, stride, pad, groups) in enumerate(shapes):
                        conv = torch.nn.Conv1d(ci, co, kk, stride=stride, padding=0 if i == 0 else pad, groups=groups)
                        conv.weight, conv.bias = dparams[f"scales.{k}.layers.{i}.weight"], dparams[f"scales.{k}.layers.{i}.bias"]
                        convs.append(conv)
                    self.scales.append(convs)

            def forward(self, wav, pin=None):
                out, x = [], wav[:, None, :]
                for k, convs in enumerate(self.scales):
                    maps, h = [], x
                    for i, conv in enumerate(convs):
                        h = conv(self.pad(h) if i == 0 else h)
                        if i < len(convs) - 1:
                            h = self.act(h) if pin is None else h * pin[k][i]
                        maps.append(h)
                    out.append(maps)
                    x = self.pool(x)
                return out

        torch_disc = TorchDisc().to("cuda:0")

        voc = MelGANGenerator(MelGANConfig(), ac).to("cuda:0")
        gen = torch.Generator(device="cuda").manual_seed(0)
        for B, n in ((16, 8192), (8, 32768)):
            key = f"melgan_disc_{B}x{n}"
            wav = (0.3 * torch.randn(B, n, device="cuda", generator=gen)).requires_grad_(True)
            with torch.no_grad():
                ours_maps, torch_maps = disc(wav), torch_disc(wav)
                res[key] = {"forward": ev_spread(lambda: disc(wav)), "torch_forward": ev_spread(lambda: torch_disc(wav))}
            res[key]["max_relative_map_difference_from_torch"] = max(float((a - b).abs().max() / b.abs().max()) for x, y in zip(ours_maps, torch_maps) for a, b in zip(x, y))
            cots = [[torch.randn(m.shape, device="cuda", generator=gen) / m.numel() for m in ms] for ms in ours_maps]

            def step(net):
                wav.grad = None
                for p in dparams.values():
                    p.grad = None
                sum((m * c).sum() for ms, cs in zip(net(wav), cots) for m, c in zip(ms, cs)).backward()

            res[key]["forward_plus_backward"] = ev_spread(lambda: step(disc))
            got = {k: p.grad.clone() for k, p in dparams.items()}
            got["wav"] = wav.grad.clone()
            res[key]["torch_forward_plus_backward"] = ev_spread(lambda: step(torch_disc))

            def grad_difference():
                return max([float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in dparams.items()]
                           + [float((got["wav"] - wav.grad).abs().max() / wav.grad.abs().max())])

            res[key]["max_relative_gradient_difference_from_torch"] = grad_difference()
            # where the two forwards put a LeakyReLU on different sides (pre-activations within rounding of 0), and the same comparison
            # with torch differentiating through the device's own decisions
            res[key]["leaky_relu_decisions_that_differ"] = sum(int(((a > 0) != (b > 0)).sum()) for x, y in zip(ours_maps, torch_maps) for a, b in zip(x[:-1], y[:-1]))
            one, low = torch.ones((), device="cuda"), torch.full((), dc.leaky_slope, device="cuda")
            pin = [[torch.where(m > 0, one, low) for m in ms] for ms in ours_maps]
            step(lambda w: torch_disc(w, pin))
            res[key]["max_relative_gradient_difference_from_torch_pinned"] = grad_difference()
            res[key]["backward_workspace_mb"] = round(disc._train_workspace.numel() / 1e6, 1)
            print(json.dumps({key: res[key]}), flush=True)
            trainer = MelGANTrainer(voc, disc)
            mel = (0.5 * torch.randn(B, 80, n // voc.hop, device="cuda", generator=gen) - 0.5).contiguous()
            real = wav.detach()
            res[key]["train_step"] = ev_spread(lambda: trainer.train_step(mel, real), warm=2, reps=5)
            print(json.dumps({key: {"train_step": res[key]["train_step"]}}), flush=True)
    if "hifigan_mpd" in which:
        import ctypes as C
        import statistics

        import torch.nn.functional as F

        from genvox_amd import _lib
        from genvox_amd.configs import HiFiGANConfig, HiFiGANPeriodDiscriminatorConfig
        from genvox_amd.hifigan import HiFiGANGenerator
        from genvox_amd.hifigan_disc import HiFiGANPeriodDiscriminator
        from genvox_amd.hifigan_training import HiFiGANTrainer

        FP32_MATRIX_TFLOPS = 157.3   # the MI355X's fp32 matrix (= vector) peak

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        torch.manual_seed(0)
        pc = HiFiGANPeriodDiscriminatorConfig()
        mpd = HiFiGANPeriodDiscriminator(pc).to("cuda:0")
        with torch.no_grad():
            for name, p in mpd.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.1 * torch.randn_like(p))
        pparams = dict(mpd.named_parameters())
        pshapes = pc.layer_shapes()

        def torch_mpd(wav):
            """The published composition on the module's own parameters, through torch's Conv2d kernels."""
            out = []
            for j, p in enumerate(pc.periods):
                x, n = wav[:, None, :], wav.shape[1]
                if n % p:
                    x = F.pad(x, (0, p - n % p), "reflect")
                h, maps = x.view(wav.shape[0], 1, -1, p), []
                for i, (_ci, _co, _k, stride, pad) in enumerate(pshapes):
                    name = f"discriminators.{j}.conv_post" if i == len(pshapes) - 1 else f"discriminators.{j}.convs.{i}"
                    h = F.conv2d(h, pparams[name + ".weight"], pparams[name + ".bias"], stride=(stride, 1), padding=(pad, 0))
                    if i < len(pshapes) - 1:
                        h = F.leaky_relu(h, pc.leaky_slope)
                    maps.append(h)
                out.append(maps)
            return out

        def layer_macs(n):
            """Multiply-adds of one row of n samples per layer, summed over the periods (every tap counted, padding included)."""
            heights = mpd.feature_heights(n)
            return [sum(heights[j][i] * p * co * ci * k for j, p in enumerate(pc.periods)) for i, (ci, co, k, _s, _p) in enumerate(pshapes)]

        gen = torch.Generator(device="cuda").manual_seed(0)
        hvoc = HiFiGANGenerator(HiFiGANConfig(), ac).to("cuda:0")
        for B, n in ((16, 8192), (8, 32768)):
            key = f"hifigan_mpd_{B}x{n}"
            wav = (0.3 * torch.randn(B, n, device="cuda", generator=gen)).requires_grad_(True)
            with torch.no_grad():
                ours_maps, torch_maps = mpd(wav), torch_mpd(wav)
                res[key] = {"forward": ev_spread(lambda: mpd(wav)), "torch_forward": ev_spread(lambda: torch_mpd(wav))}
            res[key]["max_relative_map_difference_from_torch"] = max(float((a - b).abs().max() / b.abs().max()) for x, y in zip(ours_maps, torch_maps) for a, b in zip(x, y))
            cots = [[torch.randn(m.shape, device="cuda", generator=gen) / m.numel() for m in ms] for ms in ours_maps]

            def step(net):
                wav.grad = None
                for p in pparams.values():
                    p.grad = None
                sum((m * c).sum() for ms, cs in zip(net(wav), cots) for m, c in zip(ms, cs)).backward()

            res[key]["forward_plus_backward"] = ev_spread(lambda: step(mpd))
            got = {k: p.grad.clone() for k, p in pparams.items()}
            got["wav"] = wav.grad.clone()
            res[key]["torch_forward_plus_backward"] = ev_spread(lambda: step(torch_mpd))
            res[key]["max_relative_gradient_difference_from_torch"] = max(
                [float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in pparams.items()]
                + [float((got["wav"] - wav.grad).abs().max() / wav.grad.abs().max())])
            res[key]["backward_workspace_mb"] = round(mpd._train_workspace.numel() / 1e6, 1)
            # per layer: counted multiply-adds and the share of the fp32 matrix rate, from events around every layer of one more call
            lib = _lib.load()
            _lib.check(lib.gvx_hifigan_mpd_timing_enable(mpd._handle, 1))
            step(mpd)
            fwd_ms, bwd_ms, n_l = (C.c_float * 9)(), (C.c_float * 9)(), C.c_int()
            _lib.check(lib.gvx_hifigan_mpd_layer_times_ms(mpd._handle, fwd_ms, bwd_ms, C.byref(n_l)))
            _lib.check(lib.gvx_hifigan_mpd_timing_enable(mpd._handle, 0))
            macs = [B * m for m in layer_macs(n)]
            res[key]["multiply_adds_per_row_forward"] = sum(layer_macs(n))
            res[key]["layers"] = [
                {"layer": f"{ci}->{co}", "forward_gmacs": round(m / 1e9, 3), "forward_ms": round(fwd_ms[i], 3),
                 "forward_share_of_fp32_matrix_rate": round(2 * m / (fwd_ms[i] * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4) if fwd_ms[i] > 0 else None,
                 "backward_ms": round(bwd_ms[i], 3),
                 "backward_share_of_fp32_matrix_rate": round(2 * (2 if i else 1) * m / (bwd_ms[i] * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4) if bwd_ms[i] > 0 else None}
                for i, ((ci, co, _k, _s, _p), m) in enumerate(zip(pshapes, macs))]
            print(json.dumps({key: res[key]}), flush=True)
            trainer = HiFiGANTrainer(hvoc, [mpd])
            mel = (0.5 * torch.randn(B, 80, n // hvoc.hop, device="cuda", generator=gen) - 0.5).contiguous()
            real = wav.detach()
            res[key]["train_step_v1"] = ev_spread(lambda: trainer.train_step(mel, real), warm=2, reps=5)
            print(json.dumps({key: {"train_step_v1": res[key]["train_step_v1"]}}), flush=True)
            del trainer
    if "hifigan_msd" in which:
        import ctypes as C
        import statistics

        import torch.nn.functional as F

        from genvox_amd import _lib
        from genvox_amd.configs import HiFiGANConfig, HiFiGANScaleDiscriminatorConfig
        from genvox_amd.hifigan import HiFiGANGenerator
        from genvox_amd.hifigan_disc import HiFiGANPeriodDiscriminator
        from genvox_amd.hifigan_msd import HiFiGANScaleDiscriminator
        from genvox_amd.hifigan_training import HiFiGANTrainer
        from genvox_amd.losses import MelSpectrogramLoss

        FP32_MATRIX_TFLOPS = 157.3   # the MI355X's fp32 matrix (= vector) peak

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        torch.manual_seed(0)
        sc = HiFiGANScaleDiscriminatorConfig()
        msd = HiFiGANScaleDiscriminator(sc).to("cuda:0").eval()   # eval: the weights of both sides stay the same from call to call
        with torch.no_grad():
            for name, p in msd.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.1 * torch.randn_like(p))
        sparams = dict(msd.named_parameters())
        sshapes = sc.layer_shapes()

        def torch_msd(wav):
            """The published composition on the module's own parameters (spectral norm through the same sigma), through torch's grouped
            Conv1d and avg_pool1d kernels."""
            out, x = [], wav[:, None, :]
            eff = dict(zip(msd.weight_names(), msd.effective_weights()))
            for s in range(sc.n_scales):
                h, maps = x, []
                for i, (_ci, _co, _k, stride, pad, groups) in enumerate(sshapes):
                    name = f"discriminators.{s}.conv_post" if i == len(sshapes) - 1 else f"discriminators.{s}.convs.{i}"
                    h = F.conv1d(h, eff[name + ".weight"], eff[name + ".bias"], stride=stride, padding=pad, groups=groups)
                    if i < len(sshapes) - 1:
                        h = F.leaky_relu(h, sc.leaky_slope)
                    maps.append(h)
                out.append(maps)
                x = F.avg_pool1d(x, 4, 2, 2)
            return out

        def layer_macs(n):
            """Multiply-adds of one row of n samples per layer, summed over the scales (every tap counted, padding included)."""
            lengths = msd.feature_lengths(n)
            return [sum(lengths[s][i] * co * (ci // g) * k for s in range(sc.n_scales)) for i, (ci, co, k, _s, _p, g) in enumerate(sshapes)]

        gen = torch.Generator(device="cuda").manual_seed(0)
        hvoc = HiFiGANGenerator(HiFiGANConfig(), ac).to("cuda:0")
        for B, n in ((16, 8192), (8, 32768)):
            key = f"hifigan_msd_{B}x{n}"
            wav = (0.3 * torch.randn(B, n, device="cuda", generator=gen)).requires_grad_(True)
            with torch.no_grad():
                ours_maps, torch_maps = msd(wav), torch_msd(wav)
                res[key] = {"forward": ev_spread(lambda: msd(wav)), "torch_forward": ev_spread(lambda: torch_msd(wav))}
            res[key]["max_relative_map_difference_from_torch"] = max(float((a - b).abs().max() / b.abs().max()) for x, y in zip(ours_maps, torch_maps) for a, b in zip(x, y))
            cots = [[torch.randn(m.shape, device="cuda", generator=gen) / m.numel() for m in ms] for ms in ours_maps]

            def step(net):
                wav.grad = None
                for p in sparams.values():
                    p.grad = None
                sum((m * c).sum() for ms, cs in zip(net(wav), cots) for m, c in zip(ms, cs)).backward()

            res[key]["forward_plus_backward"] = ev_spread(lambda: step(msd))
            got = {k: p.grad.clone() for k, p in sparams.items()}
            got["wav"] = wav.grad.clone()
            res[key]["torch_forward_plus_backward"] = ev_spread(lambda: step(torch_msd))
            res[key]["max_relative_gradient_difference_from_torch"] = max(
                [float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in sparams.items()]
                + [float((got["wav"] - wav.grad).abs().max() / wav.grad.abs().max())])
            res[key]["backward_workspace_mb"] = round(msd._train_workspace.numel() / 1e6, 1)
            # per layer: counted multiply-adds and the share of the fp32 matrix rate, from events around every layer of one more call
            lib = _lib.load()
            _lib.check(lib.gvx_hifigan_msd_timing_enable(msd._handle, 1))
            step(msd)
            fwd_ms, bwd_ms, n_l = (C.c_float * 9)(), (C.c_float * 9)(), C.c_int()
            _lib.check(lib.gvx_hifigan_msd_layer_times_ms(msd._handle, fwd_ms, bwd_ms, C.byref(n_l)))
            _lib.check(lib.gvx_hifigan_msd_timing_enable(msd._handle, 0))
            macs = [B * m for m in layer_macs(n)]
            res[key]["multiply_adds_per_row_forward"] = sum(layer_macs(n))
            res[key]["layers"] = [
                {"layer": f"{ci}->{co} k{k} g{g}", "forward_gmacs": round(m / 1e9, 3), "forward_ms": round(fwd_ms[i], 3),
                 "forward_share_of_fp32_matrix_rate": round(2 * m / (fwd_ms[i] * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4) if fwd_ms[i] > 0 else None,
                 "backward_ms": round(bwd_ms[i], 3),
                 "backward_share_of_fp32_matrix_rate": round(2 * (2 if i else 1) * m / (bwd_ms[i] * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4) if bwd_ms[i] > 0 else None}
                for i, ((ci, co, k, _s, _p, g), m) in enumerate(zip(sshapes, macs))]
            print(json.dumps({key: res[key]}), flush=True)
            msd.train()
            trainer = HiFiGANTrainer(hvoc, [HiFiGANPeriodDiscriminator().to("cuda:0"), msd], aux_loss=MelSpectrogramLoss())
            mel = (0.5 * torch.randn(B, 80, n // hvoc.hop, device="cuda", generator=gen) - 0.5).contiguous()
            real = wav.detach()
            res[key]["train_step_v1_mpd_msd_mel"] = ev_spread(lambda: trainer.train_step(mel, real), warm=2, reps=5)
            print(json.dumps({key: {"train_step_v1_mpd_msd_mel": res[key]["train_step_v1_mpd_msd_mel"]}}), flush=True)
            del trainer
            msd.eval()
    if "mrd" in which:
        import ctypes as C
        import statistics

        import torch.nn.functional as F

        from genvox_amd import _lib
        from genvox_amd.configs import MultiResolutionDiscriminatorConfig
        from genvox_amd.mrd import MultiResolutionDiscriminator

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        torch.manual_seed(0)
        rc = MultiResolutionDiscriminatorConfig()
        mrd = MultiResolutionDiscriminator(rc).to("cuda:0")
        with torch.no_grad():
            for name, p in mrd.named_parameters():
                if name.endswith("bias"):
                    p.copy_(0.1 * torch.randn_like(p))
        rparams = dict(mrd.named_parameters())
        rshapes = rc.layer_shapes()

        def torch_mrd(wav):
            """The published composition on the module's own parameters, through torch's stft and Conv2d kernels; the maps transposed to
            the module's [B, C, W, F]."""
            out = []
            for j, (n_fft, hop, win) in enumerate(rc.resolutions):
                pad = (n_fft - hop) // 2
                x = F.pad(wav[:, None, :], (pad, pad), mode="reflect")[:, 0, :]
                spec = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.ones(win, device=wav.device), center=False, return_complex=True)
                h, maps = torch.linalg.vector_norm(torch.view_as_real(spec), dim=-1)[:, None], []
                for i, (_ci, _co, (kf, kt), stride) in enumerate(rshapes):
                    name = f"discriminators.{j}.conv_post" if i == len(rshapes) - 1 else f"discriminators.{j}.convs.{i}"
                    h = F.conv2d(h, rparams[name + ".weight"], rparams[name + ".bias"], stride=(1, stride), padding=(kf // 2, kt // 2))
                    if i < len(rshapes) - 1:
                        h = F.leaky_relu(h, rc.leaky_slope)
                    maps.append(h.transpose(2, 3))
                out.append(maps)
            return out

        gen = torch.Generator(device="cuda").manual_seed(0)
        for B, n in ((16, 8192), (32, 8192)):
            key = f"mrd_{B}x{n}"
            wav = (0.3 * torch.randn(B, n, device="cuda", generator=gen)).requires_grad_(True)
            with torch.no_grad():
                ours_maps, torch_maps = mrd(wav), torch_mrd(wav)
                res[key] = {"forward": ev_spread(lambda: mrd(wav)), "torch_forward": ev_spread(lambda: torch_mrd(wav))}
            res[key]["max_relative_map_difference_from_torch"] = max(float((a - b).abs().max() / b.abs().max()) for x, y in zip(ours_maps, torch_maps) for a, b in zip(x, y))
            cots = [[torch.randn(m.shape, device="cuda", generator=gen) / m.numel() for m in ms] for ms in ours_maps]

            def step(net):
                wav.grad = None
                for p in rparams.values():
                    p.grad = None
                sum((m * c).sum() for ms, cs in zip(net(wav), cots) for m, c in zip(ms, cs)).backward()

            res[key]["forward_plus_backward"] = ev_spread(lambda: step(mrd))
            got = {k: p.grad.clone() for k, p in rparams.items()}
            got["wav"] = wav.grad.clone()
            res[key]["torch_forward_plus_backward"] = ev_spread(lambda: step(torch_mrd))
            res[key]["max_relative_gradient_difference_from_torch"] = max(
                [float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in rparams.items()]
                + [float((got["wav"] - wav.grad).abs().max() / wav.grad.abs().max())])
            res[key]["leaky_relu_decisions_that_differ"] = sum(int(((a > 0) != (b > 0)).sum()) for x, y in zip(ours_maps, torch_maps) for a, b in zip(x[:-1], y[:-1]))
            res[key]["forward_workspace_mb"] = round(mrd._workspace.numel() / 1e6, 1)
            res[key]["backward_workspace_mb"] = round(mrd._train_workspace.numel() / 1e6, 1)
            res[key]["features_mb"] = round(_lib.load().gvx_mrd_features_bytes(C.byref(mrd.dims()), B, n) / 1e6, 1)
            lib = _lib.load()
            _lib.check(lib.gvx_mrd_timing_enable(mrd._handle, 1))
            step(mrd)
            fwd_ms, bwd_ms, n_l = (C.c_float * 9)(), (C.c_float * 9)(), C.c_int()
            _lib.check(lib.gvx_mrd_layer_times_ms(mrd._handle, fwd_ms, bwd_ms, C.byref(n_l)))
            _lib.check(lib.gvx_mrd_timing_enable(mrd._handle, 0))
            widths = mrd.map_widths(n)
            macs = [B * sum(widths[j][i] * (nf // 2 + 1) * co * ci * kf * kt for j, (nf, _h, _w) in enumerate(rc.resolutions))
                    for i, (ci, co, (kf, kt), _s) in enumerate(rshapes)]
            res[key]["layers"] = [{"layer": f"{ci}->{co} {kf}x{kt}", "forward_gmacs": round(m / 1e9, 3), "forward_ms": round(fwd_ms[i], 3), "backward_ms": round(bwd_ms[i], 3)}
                                  for i, ((ci, co, (kf, kt), _s), m) in enumerate(zip(rshapes, macs))]
            print(json.dumps({key: res[key]}), flush=True)
    if which & {"hifigan", "hifigan_train"}:
        import ctypes as C
        import statistics

        from torch import nn

        from genvox_amd.configs import HiFiGANConfig, MelGANConfig
        from genvox_amd import _lib
        from genvox_amd.hifigan import HiFiGANGenerator
        from genvox_amd.melgan import MelGANGenerator

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        class TorchHiFiGAN(nn.Module):   # the network of include/genvox_amd.h from torch.nn modules, plain weights
            def __init__(self, hc, n_mels):
                super().__init__()
                self.hc, c = hc, hc.upsample_initial_channel
                self.conv_pre = nn.Conv1d(n_mels, c, 7, padding=3)
                self.ups, self.resblocks = nn.ModuleList(), nn.ModuleList()
                for r in hc.upsample_rates:
                    self.ups.append(nn.ConvTranspose1d(c, c // 2, 2 * r, stride=r, padding=r // 2))
                    c //= 2
                    for k, ds in zip(hc.resblock_kernel_sizes, hc.resblock_dilation_sizes):
                        blk = nn.Module()
                        first = nn.ModuleList([nn.Conv1d(c, c, k, dilation=d, padding=(k - 1) * d // 2) for d in ds])
                        if hc.resblock == "1":
                            blk.convs1, blk.convs2 = first, nn.ModuleList([nn.Conv1d(c, c, k, padding=(k - 1) // 2) for _ in ds])
                        else:
                            blk.convs = first
                        self.resblocks.append(blk)
                self.conv_post = nn.Conv1d(c, 1, 7, padding=3)

            def forward(self, x):
                s, n_k = self.hc.leaky_slope, len(self.hc.resblock_kernel_sizes)
                x = self.conv_pre(x)
                for i, up in enumerate(self.ups):
                    x = up(F.leaky_relu(x, s))
                    xs = None
                    for blk in self.resblocks[i * n_k:(i + 1) * n_k]:
                        y = x
                        if self.hc.resblock == "1":
                            for c1, c2 in zip(blk.convs1, blk.convs2):
                                y = y + c2(F.leaky_relu(c1(F.leaky_relu(y, s)), s))
                        else:
                            for c1 in blk.convs:
                                y = y + c1(F.leaky_relu(y, s))
                        xs = y if xs is None else xs + y
                    x = xs / n_k
                return torch.tanh(self.conv_post(F.leaky_relu(x, self.hc.post_leaky_slope)))[:, 0]

        import torch.nn.functional as F

        ap = AudioProcessor(ac, device="cuda:0")
        gen = torch.Generator(device="cuda").manual_seed(0)
        melgan = MelGANGenerator(MelGANConfig(), ac).to("cuda:0")
        configs = (("v1", HiFiGANConfig(), ((1, 568), (32, 800))), ("v2", HiFiGANConfig(upsample_initial_channel=128), ((32, 800),)))
        for name, hc, shapes in configs if "hifigan" in which else ():
            torch.manual_seed(0)
            voc = HiFiGANGenerator(hc, ac).to("cuda:0")
            with torch.no_grad():
                for pname, p in voc.named_parameters():
                    if pname.endswith("bias"):
                        p.copy_(0.1 * torch.randn_like(p))
            ref = TorchHiFiGAN(hc, ac.n_mels).to("cuda:0")
            ref.load_state_dict(voc.state_dict())
            for B, T in shapes:
                key = f"hifigan_{name}_{B}x{T}"
                mel = (0.5 * torch.randn(B, 80, T, device="cuda", generator=gen) - 0.5).contiguous()
                rows = B
                while rows > 1 and voc.workspace_bytes(rows, T) > voc.WORKSPACE_CAP_BYTES:
                    rows = (rows + 1) // 2
                res[key] = {"as_delivered": ev_spread(lambda: voc.vocode(mel)), "rows_per_call_as_delivered": rows}
                voc.enable_stage_timing(True)   # the stage times are of one call: the rows of one group
                per = []
                for _ in range(5):
                    voc.vocode(mel[:rows])
                    per.append(voc.stage_times_ms())
                voc.enable_stage_timing(False)
                res[key]["stage_ms_median_of_one_call"] = [round(statistics.median(col), 3) for col in zip(*per)]   # conv_pre, every stage, conv_post
                wav = voc.vocode(mel)
                print(json.dumps({key: res[key]}), flush=True)
                with torch.no_grad():
                    res[key]["torch_convolutions"] = ev_spread(lambda: ref(mel), warm=2, reps=7)
                    res[key]["max_abs_difference_from_torch"] = float((ref(mel) - wav).abs().max())
                res[key]["melgan"] = ev_spread(lambda: melgan.vocode(mel))
                res[key]["griffin_lim_32it"] = ev_spread(lambda: ap.convert_mel2wav_batch(mel), warm=1, reps=5)
                print(json.dumps({key: res[key]}), flush=True)
            del voc, ref
        if "hifigan_train" in which:
            hc = HiFiGANConfig()
            torch.manual_seed(0)
            voc = HiFiGANGenerator(hc, ac).to("cuda:0")
            with torch.no_grad():
                for pname, p in voc.named_parameters():
                    if pname.endswith("bias"):
                        p.copy_(0.1 * torch.randn_like(p))
            ref = TorchHiFiGAN(hc, ac.n_mels).to("cuda:0")
            ref.load_state_dict(voc.state_dict())
            params, ref_params = list(voc.parameters()), dict(ref.named_parameters())
            for B, T in ((16, 32), (8, 128)):   # a training segment; a longer one
                key = f"hifigan_train_v1_{B}x{T}"
                mel = (0.5 * torch.randn(B, 80, T, device="cuda", generator=gen) - 0.5).contiguous()
                cot = torch.randn(B, T * voc.hop, device="cuda", generator=gen)

                def ours():
                    for p in params:
                        p.grad = None
                    (voc.vocode_with_grad(mel) * cot).sum().backward()

                def torchs():   # autograd through torch's own convolutions, the same parameter values
                    for p in ref_params.values():
                        p.grad = None
                    (ref(mel) * cot).sum().backward()

                lib, dims = _lib.load(), voc.dims()
                res[key] = {"forward_train_plus_backward": ev_spread(ours, warm=2, reps=7),
                            "inference_forward": ev_spread(lambda: voc.vocode(mel), warm=2, reps=7),
                            "tape_mb": round(lib.gvx_hifigan_tape_bytes(C.byref(dims), B, T) / 1e6, 1),
                            "backward_workspace_mb": round(lib.gvx_hifigan_backward_workspace_bytes(C.byref(dims), B, T) / 1e6, 1)}
                voc.enable_stage_timing(True)
                fwd, bwd = [], []
                for _ in range(5):
                    voc.vocode(mel)
                    fwd.append(voc.stage_times_ms())
                    ours()
                    bwd.append(voc.backward_stage_times_ms())
                voc.enable_stage_timing(False)
                fwd = [statistics.median(col) for col in zip(*fwd)]                 # conv_pre, every stage, conv_post
                bwd = [statistics.median(col) for col in zip(*bwd)]                 # transposes, conv_post, stages from the last, conv_pre
                bwd_fwd_order = [bwd[-1]] + bwd[2:-1][::-1] + [bwd[1]]
                res[key]["forward_stage_ms"] = [round(v, 3) for v in fwd]
                res[key]["backward_stage_ms"] = [round(v, 3) for v in bwd_fwd_order]
                res[key]["backward_over_forward_per_stage"] = [round(b / f, 2) for b, f in zip(bwd_fwd_order, fwd)]
                res[key]["backward_weight_transposes_ms"] = round(bwd[0], 3)
                ours()
                got = {k: p.grad.clone() for k, p in voc.named_parameters()}
                res[key]["torch_autograd"] = ev_spread(torchs, warm=2, reps=7)
                res[key]["max_relative_gradient_difference_from_torch"] = max(
                    float((got[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in ref_params.items())
                print(json.dumps({key: res[key]}), flush=True)
            del voc, ref
    if "bigvgan" in which:
        import ctypes as C
        import statistics

        from genvox_amd import _lib
        from genvox_amd.bigvgan import BigVGANGenerator, kaiser_sinc_filter, snake_constants
        from genvox_amd.configs import BigVGANConfig
        from tests import bigvgan_ref64 as R

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        lib = _lib.load()
        gen = torch.Generator(device="cuda").manual_seed(0)
        large = dict(upsample_initial_channel=1536, upsample_rates=(4, 4, 2, 2, 2, 2), upsample_kernel_sizes=(8, 8, 4, 4, 4, 4))
        for name, bc, cfg, shapes in (("base", BigVGANConfig(), R.BASE, ((32, 800), (1, 568))), ("large", BigVGANConfig(**large), R.LARGE, ((8, 200),))):
            ref = R.Generator(cfg, seed=0).float().to("cuda:0")   # random weights, a_c and b_c spread over 0.3 .. 5
            voc = BigVGANGenerator(bc, ac)
            voc.load_state_dict(ref.state_dict())
            voc.to("cuda:0")
            f_dev = kaiser_sinc_filter().to("cuda:0", torch.float32)
            for B, T in shapes:
                key = f"bigvgan_{name}_{B}x{T}"
                mel = (0.5 * torch.randn(B, 80, T, device="cuda", generator=gen) - 0.5).contiguous()
                rows = B
                while rows > 1 and voc.workspace_bytes(rows, T) > voc.WORKSPACE_CAP_BYTES:
                    rows = (rows + 1) // 2
                res[key] = {"as_delivered": ev_spread(lambda: voc.vocode(mel)), "rows_per_call_as_delivered": rows}
                voc.enable_stage_timing(True)   # the stage times are of one call: the rows of one group
                per = []
                for _ in range(5):
                    voc.vocode(mel[:rows])
                    per.append(voc.stage_times_ms())
                voc.enable_stage_timing(False)
                res[key]["stage_ms_median_of_one_call"] = [round(statistics.median(col), 3) for col in zip(*per)]   # conv_pre, every stage, activation_post + conv_post
                # the activation's launches alone, at every stage's shape of one call
                n_act = len(bc.resblock_kernel_sizes) * len(bc.resblock_dilation_sizes[0]) * (2 if bc.resblock == "1" else 1)
                c, mul, act_ms = bc.upsample_initial_channel, 1, []
                stream = torch.cuda.current_stream().cuda_stream
                for i, r in enumerate(bc.upsample_rates):
                    c, mul = c // 2, mul * r
                    x = torch.randn(rows, T * mul, c, device="cuda", generator=gen)
                    out = torch.empty_like(x)
                    a, g = snake_constants(R.random_snake(c, None, True).cuda(), R.random_snake(c, None, True).cuda(), "snakebeta", True)
                    one = lambda: _lib.check(lib.gvx_snake_antialiased(x.data_ptr(), None, rows, T * mul, c, f_dev.data_ptr(), a.data_ptr(), g.data_ptr(),
                                                                       out.data_ptr(), stream))
                    launches = n_act + (1 if i == len(bc.upsample_rates) - 1 else 0)   # activation_post runs at the last stage's shape
                    t = ev_spread(one, warm=2, reps=7)["median_ms"]
                    act_ms.append({"channels": c, "positions": T * mul, "one_launch_ms": t, "launches": launches, "ms": round(t * launches, 3),
                                   "GBs_read_plus_write": round(8.0 * x.numel() / t / 1e6, 1)})
                    del x, out
                res[key]["activation_launches_of_one_call"] = act_ms
                res[key]["activation_ms_of_one_call"] = round(sum(e["ms"] for e in act_ms), 3)
                res[key]["activation_share_of_one_call"] = round(sum(e["ms"] for e in act_ms) / sum(res[key]["stage_ms_median_of_one_call"]), 3)
                wav = voc.vocode(mel)
                print(json.dumps({key: res[key]}), flush=True)
                with torch.no_grad():
                    res[key]["torch_float32_restatement"] = ev_spread(lambda: ref(mel), warm=1, reps=5)
                    res[key]["max_abs_difference_from_torch"] = float((ref(mel)[0] - wav).abs().max())
                print(json.dumps({key: res[key]}), flush=True)
            del voc, ref
    if "vocos" in which:
        import statistics

        from genvox_amd.configs import VocosConfig
        from genvox_amd.vocos import VocosGenerator
        from tests import vocos_ref64 as R

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        cfg = R.DEFAULT
        vac = AudioConfig(filter_length=1024, hop_length=256, log_func="np.log")
        vac.n_mels = cfg["n_mels"]
        ref = R.Generator(cfg, seed=0).float().to("cuda:0")
        voc = VocosGenerator(VocosConfig(), vac)
        voc.load_state_dict(ref.state_dict())
        voc.to("cuda:0")
        gen = torch.Generator(device="cuda").manual_seed(0)
        mlp_flops_per_frame = 2.0 * cfg["num_layers"] * 2 * cfg["dim"] * cfg["intermediate_dim"]
        for B, T in ((32, 800), (1, 568), (8, 200)):
            key = f"vocos_{B}x{T}"
            mel = (1.5 * torch.randn(B, cfg["n_mels"], T, device="cuda", generator=gen) - 3.0).contiguous()
            res[key] = {"ours": ev_spread(lambda: voc.vocode(mel)), "workspace_bytes": voc.workspace_bytes(B, T)}
            voc.enable_stage_timing(True)
            per = []
            for _ in range(7):
                voc.vocode(mel)
                per.append(voc.stage_times_ms())
            voc.enable_stage_timing(False)
            stage = [statistics.median(col) for col in zip(*per)]
            res[key]["stage_ms_median"] = [round(v, 3) for v in stage]   # embed + norm, the blocks, final norm + head product, ISTFT
            res[key]["stage_ms_range"] = [[round(min(col), 3), round(max(col), 3)] for col in zip(*per)]
            tflops = mlp_flops_per_frame * B * T / (stage[1] * 1e-3) / 1e12
            res[key]["blocks_mlp_tflops"] = round(tflops, 1)   # the filter + LayerNorm launches count towards the time
            res[key]["blocks_mlp_fraction_of_157TF_fp32_mfma"] = round(tflops / 157.3, 3)
            wav = voc.vocode(mel)
            with torch.no_grad():
                res[key]["torch_float32_restatement"] = ev_spread(lambda: ref(mel), warm=1, reps=7)
                want = ref(mel)[0]
            res[key]["max_abs_difference_from_torch"] = float((want - wav[:, :want.shape[1]]).abs().max())
            res[key]["verdict"] = "faster" if res[key]["ours"]["median_ms"] < res[key]["torch_float32_restatement"]["median_ms"] else "SLOWER"
            print(json.dumps({key: res[key]}), flush=True)
        del voc, ref
    if "vocos_train" in which:
        import statistics

        from genvox_amd.configs import VocosConfig
        from genvox_amd.vocos import VocosGenerator
        from tests import vocos_grad_ref64 as GR
        from tests import vocos_ref64 as R

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        cfg = R.DEFAULT
        vac = AudioConfig(filter_length=1024, hop_length=256, log_func="np.log")
        vac.n_mels = cfg["n_mels"]
        ref = R.Generator(cfg, seed=0).float().to("cuda:0")
        voc = VocosGenerator(VocosConfig(), vac, trainable=True)
        voc.load_state_dict(ref.state_dict())
        voc.to("cuda:0")
        gen = torch.Generator(device="cuda").manual_seed(0)
        # the blocks' products: pwconv1 and pwconv2 forward (2), and per block two data and two weight gradients backward (4)
        block_flops_per_frame = 2.0 * cfg["num_layers"] * cfg["dim"] * cfg["intermediate_dim"]
        for B, T in ((16, 32), (8, 128), (32, 800)):
            key = f"vocos_train_{B}x{T}"
            mel = (1.5 * torch.randn(B, cfg["n_mels"], T, device="cuda", generator=gen) - 3.0).contiguous()
            G = torch.randn(B, T * cfg["hop_length"], device="cuda", generator=gen)

            def ours():
                voc.zero_grad(set_to_none=True)
                voc.vocode_with_grad(mel).backward(G)

            def torchs():
                ref.zero_grad(set_to_none=True)
                wav, _ = GR.forward(ref, mel)
                wav.backward(G[:, :wav.shape[1]])

            d = voc.dims()
            res[key] = {"ours_forward_train_plus_backward": ev_spread(ours), "torch_autograd_float32_restatement": ev_spread(torchs, warm=1),
                        "tape_bytes": voc._c("tape_bytes")(__import__("ctypes").byref(d), B, T),
                        "backward_workspace_bytes": voc._c("backward_workspace_bytes")(__import__("ctypes").byref(d), B, T)}
            voc.enable_stage_timing(True)
            per = []
            for _ in range(7):
                ours()
                per.append(voc._times_ms("backward_stage_times_ms", 4))
            voc.enable_stage_timing(False)
            stage = [statistics.median(col) for col in zip(*per)]
            res[key]["backward_stage_ms_median"] = [round(v, 3) for v in stage]   # transposes + ISTFT + head, the blocks, embed + norm, sums + unfold
            res[key]["backward_stage_ms_range"] = [[round(min(col), 3), round(max(col), 3)] for col in zip(*per)]
            tflops = 4 * block_flops_per_frame * B * T / (stage[1] * 1e-3) / 1e12
            res[key]["backward_blocks_products_tflops"] = round(tflops, 1)   # the elementwise and LayerNorm launches count towards the time
            res[key]["backward_blocks_fraction_of_157TF_fp32_mfma"] = round(tflops / 157.3, 3)
            res[key]["verdict"] = ("faster" if res[key]["ours_forward_train_plus_backward"]["median_ms"] < res[key]["torch_autograd_float32_restatement"]["median_ms"]
                                   else "SLOWER")
            print(json.dumps({key: res[key]}), flush=True)
        del voc, ref
    if "fastpitch" in which:
        import statistics

        import torch.nn.functional as F

        from genvox_amd.configs import FastPitchConfig
        from genvox_amd.fastpitch import FastPitch, self_attention
        from tests import fastpitch_ref64 as R

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        cfg = R.full(R.DEFAULT)
        ref = R.Model(R.DEFAULT, seed=0).float().to("cuda:0")
        fp = FastPitch(FastPitchConfig(), AudioConfig(filter_length=1024, hop_length=256, log_func="np.log"), TextConfig(n_tokens=cfg["n_tokens"]))
        fp.load_state_dict(ref.state_dict())
        fp.to("cuda:0")
        pos = R.position_table(2000, cfg["d_model"], torch.float32).to("cuda:0")

        def stack(st, x):   # the restatement's layers on a batch of full-length rows: [B, N, C]
            for layer in st.layers:
                a = layer.dec_attn
                B_, N_, _ = x.shape
                q, k, v = (t.reshape(B_, N_, a.n_head, a.d_head).transpose(1, 2) for t in a.qkv_net(x).chunk(3, dim=2))
                o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B_, N_, -1)
                x = a.layer_norm(x + a.o_net(o))
                x = layer.pos_ff.layer_norm(x + layer.pos_ff.CoreNet(x.transpose(1, 2)).transpose(1, 2))
            return x

        def pred(p, x):
            for layer in p.layers:
                x = layer.norm(F.relu(layer.conv(x.transpose(1, 2)).transpose(1, 2)))
            return p.fc(x)[..., 0]

        def torch_forward(tokens, reps):   # every row has the same durations: the regulated batch is rectangular
            x = stack(ref.encoder, ref.encoder.word_emb(tokens) + pos[:tokens.shape[1]])
            log_dur = pred(ref.duration_predictor, x)
            x = x + ref.pitch_emb(pred(ref.pitch_predictor, x)[:, None]).transpose(1, 2)
            x = x + ref.energy_emb(pred(ref.energy_predictor, x)[:, None]).transpose(1, 2)
            y = torch.repeat_interleave(x, reps, dim=1)
            y = stack(ref.decoder, y + pos[:y.shape[1]])
            return ref.proj(y).transpose(1, 2), log_dur

        gen = torch.Generator(device="cuda").manual_seed(0)
        C_, I_ = cfg["d_model"], cfg["enc_d_inner"]
        # multiply-adds of a position of one FFT layer: qkv, o_net, the two k = 3 convolutions (the attention's own products come on top: 2 N D)
        layer_macs = C_ * 3 * 64 + 64 * C_ + 2 * 3 * C_ * I_
        for B, L, T in ((32, 128, 800), (1, 100, 568), (8, 40, 200)):
            key = f"fastpitch_{B}x{L}tokens_{T}frames"
            tokens = torch.randint(0, cfg["n_tokens"], (B, L), device="cuda", generator=gen)
            row = torch.full((L,), T // L, dtype=torch.int64, device="cuda")
            row[:T - L * (T // L)] += 1
            durations = row[None].repeat(B, 1)
            inputs = {"tokens": tokens, "durations": durations}
            res[key] = {"ours": ev_spread(lambda: fp.inference(inputs)), "workspace_bytes": max(fp.workspace_bytes(B, L), fp.workspace_bytes(B, T))}
            fp.enable_stage_timing(True)
            per = []
            for _ in range(7):
                fp.inference(inputs)
                per.append(fp.stage_times_ms())
            fp.enable_stage_timing(False)
            stage = [statistics.median(col) for col in zip(*per)]
            res[key]["stage_ms_median"] = [round(v, 3) for v in stage]   # embedding + encoder, predictors + plan + regulator, decoder, projection
            res[key]["stage_ms_range"] = [[round(min(col), 3), round(max(col), 3)] for col in zip(*per)]
            dec_flops = 2.0 * cfg["dec_n_layers"] * B * T * (layer_macs + 2 * T * 64)
            res[key]["decoder_tflops"] = round(dec_flops / (stage[2] * 1e-3) / 1e12, 1)   # LayerNorm and attention launches count towards the time
            res[key]["decoder_fraction_of_157TF_fp32_mfma"] = round(dec_flops / (stage[2] * 1e-3) / 157.3e12, 3)
            out = fp.inference(inputs)
            with torch.no_grad():
                res[key]["torch_float32_restatement"] = ev_spread(lambda: torch_forward(tokens, row), warm=1, reps=7)
                want, _ = torch_forward(tokens, row)
            res[key]["max_abs_difference_from_torch"] = float((want - out["mel_outputs"]).abs().max())
            res[key]["verdict"] = "faster" if res[key]["ours"]["median_ms"] < res[key]["torch_float32_restatement"]["median_ms"] else "SLOWER"
            print(json.dumps({key: res[key]}), flush=True)
        for B, T in ((32, 800), (1, 568)):   # the attention launch on its own
            key = f"self_attention_{B}x{T}"
            qkv = torch.randn(B, T, 192, device="cuda", generator=gen)
            q, k, v = (t.reshape(B, T, 1, 64).transpose(1, 2) for t in qkv.chunk(3, dim=2))
            res[key] = {"ours": ev_spread(lambda: self_attention(qkv, None, 1, 64)), "torch_sdpa_float32": ev_spread(lambda: F.scaled_dot_product_attention(q, k, v))}
            flops = 4.0 * B * T * T * 64
            res[key]["tflops"] = round(flops / (res[key]["ours"]["median_ms"] * 1e-3) / 1e12, 1)
            res[key]["fraction_of_157TF_fp32_mfma"] = round(flops / (res[key]["ours"]["median_ms"] * 1e-3) / 157.3e12, 3)
            res[key]["max_abs_difference_from_torch"] = float((F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, 64) - self_attention(qkv, None, 1, 64)).abs().max())
            res[key]["verdict"] = "faster" if res[key]["ours"]["median_ms"] < res[key]["torch_sdpa_float32"]["median_ms"] else "SLOWER"
            print(json.dumps({key: res[key]}), flush=True)
        del fp, ref
    if "univnet" in which:
        import statistics

        from genvox_amd import _lib
        from genvox_amd.configs import UnivNetConfig
        from genvox_amd.univnet import UnivNetGenerator
        from tests import univnet_ref64 as R

        def ev_spread(fn, warm=2, reps=7):
            for _ in range(warm):
                fn()
            out = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return {"median_ms": round(statistics.median(out), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "runs": reps}

        lib = _lib.load()
        gen = torch.Generator(device="cuda").manual_seed(0)
        for name, cfg, shapes in (("c32", R.DEFAULT, ((32, 800), (1, 568), (8, 200))), ("c16", R.C16, ((32, 800),))):
            vac = AudioConfig(filter_length=1024, hop_length=256, log_func="np.log")
            vac.n_mels = cfg["n_mels"]
            ref = R.Generator(cfg, seed=0).float().to("cuda:0")
            voc = UnivNetGenerator(UnivNetConfig(**R.model_kwargs(cfg)), vac)
            voc.load_state_dict(ref.state_dict())
            voc.to("cuda:0")
            c, h, D = cfg["channel_size"], cfg["kpnet_hidden_channels"], len(cfg["dilations"])
            ld = D * (6 * c * c + 2 * c)
            for B, T in shapes:
                key = f"univnet_{name}_{B}x{T}"
                mel = (1.5 * torch.randn(B, cfg["n_mels"], T, device="cuda", generator=gen) - 3.0).contiguous()
                noise = torch.randn(B, cfg["noise_dim"], T, device="cuda", generator=gen)
                rows = B
                while rows > 1 and voc.workspace_bytes(rows, T) > voc.WORKSPACE_CAP_BYTES:
                    rows = (rows + 1) // 2
                res[key] = {"ours": ev_spread(lambda: voc.vocode(mel, noise=noise)), "rows_per_call": rows, "workspace_bytes": voc.workspace_bytes(rows, T)}
                voc.enable_stage_timing(True)   # the stage times are of one call: the rows of one group
                per = []
                for _ in range(7):
                    voc.vocode(mel[:rows], noise=noise[:rows])
                    per.append(voc.stage_times_ms())
                voc.enable_stage_timing(False)
                stage = [statistics.median(col) for col in zip(*per)]
                res[key]["stage_ms_median_of_one_call"] = [round(v, 3) for v in stage]   # conv_pre, per block predictor then layers, conv_post
                res[key]["stage_ms_range_of_one_call"] = [[round(min(col), 3), round(max(col), 3)] for col in zip(*per)]
                # kernel_conv + bias_conv on its own: the product of one call - M = rows x T, N = ld, K = 3 H, bias - through gvx_train_gemm_nt, whose
                # A rows start H floats apart and are 3 H long, as the implicit k = 3 convolution's are (same launch_gemm and plan; the forward's
                # launch also takes row_len).  Beside it, the same multiply-adds against each predictor's whole time, small convolutions included
                stream = torch.cuda.current_stream().cuda_stream
                kb_flops = 2.0 * rows * T * (3 * h) * ld
                M = rows * T
                ga = torch.randn((M + 2) * h, device="cuda", generator=gen)
                gw = torch.randn(ld, 3 * h, device="cuda", generator=gen) * (3 * h) ** -0.5
                gb = torch.randn(ld, device="cuda", generator=gen)
                gc = torch.empty(M, ld, device="cuda")
                gemm = lambda: _lib.check(lib.gvx_train_gemm_nt(ga.data_ptr(), h, gw.data_ptr(), 3 * h, gc.data_ptr(), ld, M, ld, 3 * h, gb.data_ptr(),
                                                                None, 0, stream))
                t = ev_spread(gemm)
                res[key]["kernel_conv_alone"] = {**t, "M": M, "N": ld, "K": 3 * h, "tflops": round(kb_flops / (t["median_ms"] * 1e-3) / 1e12, 1),
                                                 "fraction_of_157TF_fp32_mfma": round(kb_flops / (t["median_ms"] * 1e-3) / 1e12 / 157.3, 3),
                                                 "GBs_written": round(4.0 * M * ld / t["median_ms"] / 1e6, 1)}
                del ga, gw, gb, gc
                res[key]["kernel_conv_tflops_in_its_predictors_time"] = [round(kb_flops / (stage[1 + 2 * i] * 1e-3) / 1e12, 1) for i in range(len(cfg["strides"]))]
                # the LVC launches on their own, at every block's shape of one call, without a convolution in front (out is a tensor of its own)
                cum, lvc = 1, []
                for s in cfg["strides"]:
                    cum *= s
                    x = torch.randn(rows, T * cum, c, device="cuda", generator=gen)
                    kern = torch.randn(rows, T, ld, device="cuda", generator=gen) * (3 * c) ** -0.5
                    out = torch.empty_like(x)
                    one = lambda: _lib.check(lib.gvx_lvc_gated(x.data_ptr(), kern.data_ptr(), D, 1, None, None, 1, None, rows, T, cum, c, 0.2,
                                                               None, out.data_ptr(), stream))
                    t = ev_spread(one)["median_ms"]
                    flops = 2.0 * rows * T * cum * (3 * c) * (2 * c)
                    lvc.append({"positions_per_frame": cum, "one_launch_ms": t, "launches": D, "ms": round(t * D, 3), "tflops": round(flops / (t * 1e-3) / 1e12, 1),
                                "fraction_of_157TF_fp32_mfma": round(flops / (t * 1e-3) / 1e12 / 157.3, 3),
                                "GBs_weights_read": round(4.0 * rows * T * 6 * c * c / t / 1e6, 1)})
                    del x, kern, out
                res[key]["lvc_launches_of_one_call"] = lvc
                wav = voc.vocode(mel, noise=noise)
                print(json.dumps({key: res[key]}), flush=True)
                with torch.no_grad():
                    torch_rows = min(B, 8)   # the restatement holds a block's kernels AND their unfolded windows: 8 rows at a time
                    run = lambda: [ref(mel[lo:lo + torch_rows], noise[lo:lo + torch_rows])[0] for lo in range(0, B, torch_rows)]
                    res[key]["torch_float32_restatement"] = ev_spread(run, warm=1, reps=7)
                    res[key]["torch_rows_per_call"] = torch_rows
                    want = torch.cat(run())
                res[key]["max_abs_difference_from_torch"] = float((want - wav).abs().max())
                res[key]["verdict"] = "faster" if res[key]["ours"]["median_ms"] < res[key]["torch_float32_restatement"]["median_ms"] else "SLOWER"
                print(json.dumps({key: res[key]}), flush=True)
            del voc, ref
    if "cpu" in which:
        # CPU baselines for configs 3 and 4 (the oracle = CPU restatement of the reference, on this box's host cores):
        # bounded samples, reported beside the GPU figures above; bench.py carries the one for config 2.
        import numpy as np

        from oracle import audio_ref, tacotron2_ref

        n_thr = max(1, min(16, os.cpu_count() or 1, len(os.sched_getaffinity(0))))
        torch.set_num_threads(n_thr)
        sd = gw.generate_state_dict(mc, ac, tc, seed=0)
        steps, L = 40, 128
        tok = torch.from_numpy(gw.synthetic_inputs(1, L, 8, 40, 80, seed=3)["token_padded"])
        masks = torch.from_numpy(gw.prenet_keep_masks(steps, mc.prenet_dim, seed=11)).reshape(2, steps, mc.prenet_dim)
        t0 = time.perf_counter()
        tacotron2_ref.tacotron2_inference(sd, tok, masks, gate_threshold=1.0, max_decoder_steps=steps)
        dt = time.perf_counter() - t0
        res["cpu_autoregressive_b1"] = {"us_per_step": round(dt / steps * 1e6, 1), "rtf_per_utterance_stream": round(dt / steps / (ac.hop_length / ac.sampling_rate), 4),
                                        "cores": n_thr, "sample": f"oracle Tacotron2.inference, batch 1 (the reference's only autoregressive mode), {steps} steps incl. encoder"}
        T, it = 200, 8
        mag = np.abs(np.random.default_rng(0).standard_normal((513, T))).astype(np.float32)
        t0 = time.perf_counter()
        audio_ref.griffin_lim(mag, 1024, 256, n_iter=it)
        dt = time.perf_counter() - t0
        per_frame_it = dt / (T * it)
        res["cpu_griffin_lim"] = {"frames_per_s_at_60it": round(1.0 / (per_frame_it * 60)), "cores": 1,
                                  "sample": f"oracle griffin_lim (numpy, per-frame loops like the reference), {T} frames x {it} iterations, scaled to 60"}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
