#!/usr/bin/env python3
"""Time Tacotron2.train_step on synthetic batches (profiles/r03_train_step_timing.txt).

    train_bench.py [--guided-alpha A] [--steps N] [--shape B L T]

--guided-alpha A > 0: the step under Tacotron2GuidedLoss(alpha=A) - one more pass over the alignments and the decoder BPTT with
an alignment gradient; 0 (default): get_criterion(), the unguided step.  Per shape: every step's wall time between two device
synchronisations (the first two include allocation, code-object loading and the first device-side re-pack), then median and
range of the steps after those two."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from genvox_amd import weights as gw
from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
from genvox_amd.tacotron2 import Tacotron2

ap = argparse.ArgumentParser()
ap.add_argument("--guided-alpha", type=float, default=0.0)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("B", "L", "T"))
args = ap.parse_args()
mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024, hop_length=256, log_func="np.log"), TextConfig(n_tokens=40)
m = Tacotron2(mc, ac, tc)
m.load_state_dict(gw.generate_state_dict(mc, ac, tc, seed=0))
m = m.to("cuda:0")
opt = m.get_optimizer()
crit = m.get_criterion(guided_attention_alpha=args.guided_alpha) if args.guided_alpha else m.get_criterion()
for B, L, T in (args.shape or ((8, 64, 100), (32, 128, 200), (64, 128, 200), (32, 128, 800))):
    batch = {k: torch.from_numpy(v).cuda() for k, v in gw.synthetic_inputs(B, L, T, 40, 80, seed=3).items()}
    times, losses = [], []
    for i in range(args.steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m.train_step(batch, crit, opt)
        torch.cuda.synchronize(); times.append(time.perf_counter() - t0); losses.append(round(m.loss_items["loss"], 4))
    later = times[2:] or times
    print(f"train_step B={B} L={L} T={T} guided_alpha={args.guided_alpha:g}: {[round(t, 3) for t in times]} s per step, loss {losses}, "
          f"grad_norm {m.grad_norm_val:.3f}, peak memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB; after the first two steps: median "
          f"{statistics.median(later) * 1e3:.2f} ms, range {min(later) * 1e3:.2f} .. {max(later) * 1e3:.2f} ms"
          + (f", guided_attention_loss {m.loss_items['guided_attention_loss']:.5f}" if "guided_attention_loss" in m.loss_items else ""))
