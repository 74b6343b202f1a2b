#!/usr/bin/env python3
"""Developer diagnostic (GPU box): batched autoregressive decode (64 rows = two lanes) run several times; where do runs differ?
ar_determinism.py [B [steps [out.pt]]]: out.pt receives the first run's outputs (to compare two builds byte for byte)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from genvox_amd import weights as gw
from genvox_amd.configs import AudioConfig, Tacotron2Config, TextConfig
from genvox_amd.tacotron2 import Tacotron2

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S = int(sys.argv[2]) if len(sys.argv) > 2 else 200
mc, ac, tc = Tacotron2Config(gate_threshold=1.0, max_decoder_steps=S), AudioConfig(filter_length=1024, hop_length=256, log_func="np.log"), TextConfig(n_tokens=40)
m = Tacotron2(mc, ac, tc); m.load_state_dict(gw.generate_state_dict(mc, ac, tc, seed=0)); m = m.to("cuda:0")
tok = torch.from_numpy(gw.synthetic_inputs(B, 128, 8, 40, 80, seed=3)["token_padded"])
masks = torch.from_numpy(gw.prenet_keep_masks(S * B, mc.prenet_dim, seed=11)).reshape(2, S, B, mc.prenet_dim)
runs = [m.inference({"tokens": tok, "prenet_keep_masks": masks}) for _ in range(5)]
mem = [m.encode(tok.cuda()[:32], None).clone() for _ in range(3)]
print("encode() repeat equal:", [bool(torch.equal(mem[0], x)) for x in mem[1:]])
for i in range(1, 5):
    a, b = runs[0]["alignments"], runs[i]["alignments"]
    if torch.equal(a, b):
        print(f"run {i}: identical to run 0"); continue
    d = (a - b).abs()
    rows = (d.amax(dim=(1, 2)) > 0).nonzero().flatten().tolist()
    steps = (d.amax(dim=(0, 2)) > 0).nonzero().flatten()
    print(f"run {i}: differs in {len(rows)} rows (first {rows[:6]}), first differing step {int(steps[0])}, max diff {float(d.max()):.3e}; "
          f"mel diff {float((runs[0]['mel_outputs'] - runs[i]['mel_outputs']).abs().max()):.3e}")
m.check_status()
if len(sys.argv) > 3:
    torch.save({k: v.cpu() for k, v in runs[0].items() if torch.is_tensor(v)}, sys.argv[3])
