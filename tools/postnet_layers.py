#!/usr/bin/env python3
"""Developer tool: the Postnet of the LAST forward in a rocprofv3 --kernel-trace csv directory, launch by launch - everything
between the last two transpose3_kernel launches (to channels-last, residual back to channels-first), with each launch's duration
and the Postnet's span.  With B, T, C as further arguments: per Winograd layer the time, TF of the batched products
(8 x 2 (B T / 4) C C flop) and GB/s of the two transforms (input: reads B (T + 4) C, writes 8 (B T / 4) C floats; output: the
reverse), summed over the groups of tiles a layer ran as.

    python tools/postnet_layers.py <dir> [B T C [layers]]
"""
import csv
import glob
import sys

f = sorted(glob.glob(sys.argv[1] + "/*/*kernel_trace.csv"))[-1]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
short = lambda n: n.replace("gvx::", "").replace("(anonymous namespace)::", "").replace("void ", "")[:70]
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows]
end = max(i for i, e in enumerate(ev) if "transpose3_kernel" in e[2])
begin = max(i for i in range(end) if "transpose3_kernel" in ev[i][2])
post = ev[begin:end + 1]
print(f"Postnet of the last forward: {len(post)} launches, span {(post[-1][1] - post[0][0]) / 1e3:.1f} us")
for s, e, n in post:
    print(f"  {(s - post[0][0]) / 1e3:8.1f} us  +{(e - s) / 1e3:7.1f} us  {n}")
if len(sys.argv) >= 5:
    B, T, C = (int(x) for x in sys.argv[2:5])
    layers = int(sys.argv[5]) if len(sys.argv) > 5 else 3   # square C-channel layers of the Postnet
    tiles = B * ((T + 3) // 4)
    us = lambda key: sum((e - s) / 1e3 for s, e, n in post if key in n)
    wi, wo = us("winograd_input"), us("winograd_output")
    if wi:   # a layer may run as several groups of tiles: sums over the launches, per layer
        inside, g = False, 0.0
        for s, e, n in post:
            inside = "winograd_input" in n or (inside and "winograd_output" not in n)
            if inside and "gemm_f32" in n:
                g += (e - s) / 1e3
        flop, tr_bytes = 16.0 * tiles * C * C, (B * (T + 4) + 8 * tiles) * C * 4.0
        print(f"per Winograd layer ({layers} layers): input transform {wi / layers:.1f} us = {tr_bytes * layers / wi / 1e3:.0f} GB/s, "
              f"batched products {g / layers:.1f} us = {flop * layers / g / 1e6:.1f} TF of {flop / 1e9:.1f} GFLOP, "
              f"output transform {wo / layers:.1f} us = {tr_bytes * layers / wo / 1e3:.0f} GB/s, together {(wi + g + wo) / layers:.1f} us")
    else:
        flop = 2.0 * B * T * C * 5 * C
        big = sorted((e - s) / 1e3 for s, e, n in post if "gemm_f32" in n)[-layers:]
        print(f"direct {C}-channel layer: {flop / 1e9:.1f} GFLOP, big-tile launch {sum(big) / layers:.1f} us (the remainder launch follows it)")
