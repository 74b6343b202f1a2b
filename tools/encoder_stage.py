#!/usr/bin/env python3
"""Developer tool: the encoder stage of the LAST forward in a rocprofv3 --kernel-trace csv directory, launch by launch on both
queues - from the last embed_kernel launch to the start of the resident decoder kernel - with each launch's start, end, queue
and workgroups; then when each queue's chain ends, and per encoder convolution layer the time of the direct GEMM or of the
Winograd form's three parts (input transform, batched products, output transform).

    python tools/encoder_stage.py <dir> [encoder convolution layers, default 3]
"""
import csv
import glob
import sys

f = sorted(glob.glob(sys.argv[1] + "/*/*kernel_trace.csv"))[-1]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
short = lambda n: n.replace("gvx::", "").replace("(anonymous namespace)::", "").replace("void ", "")[:64]
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Queue_Id"]),
       (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])) * int(r["Grid_Size_Y"]), short(r["Kernel_Name"])) for r in rows]
begin = max(i for i, e in enumerate(ev) if "embed_kernel" in e[4])
end = min(i for i in range(begin, len(ev)) if "decoder_resident_kernel" in ev[i][4])
stage = [e for e in ev[begin:end] if "attn_persistent_kernel" not in e[4]]
t0 = stage[0][0]
enc_q = stage[0][2]
print(f"encoder stage of the last forward: {len(stage)} launches, embed to the decoder loop's start {(ev[end][0] - t0) / 1e3:.1f} us")
for s, e, q, wg, n in stage:
    print(f"{(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} us  +{(e - s) / 1e3:6.1f}  q{q:2d}  wg {wg:6d}  {n}")
for q in sorted({e[2] for e in stage}):
    last = max(e[1] for e in stage if e[2] == q)
    print(f"queue {q} ({'encoder chain' if q == enc_q else 'Prenet products'}) ends at {(last - t0) / 1e3:.1f} us")
# the convolution layers: what the encoder's queue runs between the embedding and the LSTM input GEMM (the last GEMM before the recurrence)
chain = [e for e in stage if e[2] == enc_q]
rec = next(i for i, e in enumerate(chain) if "encoder_lstm" in e[4])
gemms = [i for i in range(rec) if "gemm_f32" in chain[i][4]]
convs = chain[1:gemms[-1]]
us = lambda e: (e[1] - e[0]) / 1e3
if any("winograd" in e[4] for e in convs):
    parts = {"in": 0.0, "gemm": 0.0, "out": 0.0}   # (a layer may run as several groups of tiles: sums over the launches)
    for e in convs:
        key = "in" if "winograd_input" in e[4] else "out" if "winograd_output" in e[4] else "gemm" if "gemm_f32" in e[4] else None
        if key:
            parts[key] += us(e)
    n_layers = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    span = (convs[-1][1] - convs[0][0]) / 1e3
    print(f"{n_layers} Winograd layers, {span:.1f} us from the first input transform to the last output transform: per layer input transform "
          f"{parts['in'] / n_layers:.1f} us, batched products {parts['gemm'] / n_layers:.1f} us, output transform {parts['out'] / n_layers:.1f} us, "
          f"together {sum(parts.values()) / n_layers:.1f} us")
    i = 0
    for e in convs:
        if "winograd_input" in e[4]:
            i += 1
            start = e[0]
        if "winograd_output" in e[4]:
            print(f"  layer {i} (group ending at {(e[1] - t0) / 1e3:.1f} us): {(e[1] - start) / 1e3:.1f} us from its input transform's start")
else:
    for i, e in enumerate(x for x in convs if "gemm_f32" in x[4]):
        print(f"  direct layer {i + 1}: {us(e):.1f} us ({(e[0] - t0) / 1e3:.1f} .. {(e[1] - t0) / 1e3:.1f})")
print(f"LSTM input GEMM {us(chain[gemms[-1]]):.1f} us, recurrence {us(chain[rec]):.1f} us ({(chain[rec][0] - t0) / 1e3:.1f} .. {(chain[rec][1] - t0) / 1e3:.1f})")
