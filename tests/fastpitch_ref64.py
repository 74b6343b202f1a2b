"""FastPitch restated in plain torch from include/genvox_amd.h, "FastPitch acoustic model": the oracle of tests/test_fastpitch_*.py and
tests/test_attention_kernel_gpu.py.  It runs in float64 (the reference) and in float32 (the reference's own rounding error, the base of
the tests' bound, and tools/bench_extra.py's "torch" column).  Every row is run alone at its own length and assembled with zeros behind
it.  Nothing here touches the library."""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

LN_EPS = 1e-5

NARROW = dict(n_tokens=24, n_mels=20, d_model=32, enc_n_layers=2, enc_n_head=1, enc_d_head=32, enc_d_inner=64, dec_n_layers=2, dec_n_head=1,
              dec_d_head=32, dec_d_inner=64, predictor_filter_size=32)
TWOHEAD = dict(n_tokens=40, n_mels=80, d_model=128, enc_n_layers=2, enc_n_head=2, enc_d_head=64, enc_d_inner=256, dec_n_layers=2, dec_n_head=2,
               dec_d_head=64, dec_d_inner=256)
DEFAULT = dict(n_tokens=148, n_mels=80)
# unequal stacks, a kernel-1 encoder, three predictor layers, no energy branch; widths whose last 64-lane chunk is partly idle (96, 160)
ASYM = dict(n_tokens=30, n_mels=33, d_model=96, enc_n_layers=1, enc_n_head=1, enc_d_head=32, enc_d_inner=96, enc_kernel_size=1, dec_n_layers=3,
            dec_n_head=4, dec_d_head=32, dec_d_inner=160, dec_kernel_size=3, predictor_filter_size=160, predictor_n_layers=3, energy_conditioning=False)
# the widest model over the narrowest inner widths, a kernel-1 decoder, one predictor layer of 288
WIDE = dict(n_tokens=24, n_mels=7, d_model=512, enc_n_layers=1, enc_n_head=2, enc_d_head=64, enc_d_inner=64, enc_kernel_size=3, dec_n_layers=1,
            dec_n_head=1, dec_d_head=32, dec_d_inner=32, dec_kernel_size=1, predictor_filter_size=288, predictor_n_layers=1)
# n_head * d_head above d_model, 16 heads, min_token_frames above 1 and a max_duration the predicted durations reach
TOPHEAVY = dict(n_tokens=24, n_mels=20, d_model=32, enc_n_layers=2, enc_n_head=2, enc_d_head=64, enc_d_inner=32, dec_n_layers=1, dec_n_head=16,
                dec_d_head=32, dec_d_inner=64, predictor_filter_size=32, min_token_frames=2, max_duration=3)
_DEFAULTS = dict(d_model=384, enc_n_layers=6, enc_n_head=1, enc_d_head=64, enc_d_inner=1536, enc_kernel_size=3, dec_n_layers=6, dec_n_head=1,
                 dec_d_head=64, dec_d_inner=1536, dec_kernel_size=3, predictor_filter_size=256, predictor_n_layers=2, energy_conditioning=True,
                 max_duration=75, min_token_frames=0, max_decoder_steps=2000, max_tokens=512)


def full(cfg):
    return {**_DEFAULTS, **cfg}


def model_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k not in ("n_mels", "n_tokens")}


def position_table(n, d_model, dtype):
    """cat([sin(p f), cos(p f)]), f_i = 10000^(-2 i / d_model), computed in float64."""
    f = 1.0 / (10000.0 ** (torch.arange(0.0, d_model, 2.0, dtype=torch.float64) / d_model))
    a = torch.arange(n, dtype=torch.float64)[:, None] * f[None, :]
    return torch.cat([a.sin(), a.cos()], dim=1).to(dtype)


def attention(qkv, n_head, d_head):
    """One row: qkv [T, 3 H D], columns [q | k | v], each [H][D] -> softmax(q k^T / sqrt(D)) v per head, [T, H D]."""
    T = qkv.shape[0]
    q, k, v = (t.reshape(T, n_head, d_head).transpose(0, 1) for t in qkv.chunk(3, dim=1))   # [H, T, D]
    p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(d_head), dim=-1)
    return (p @ v).transpose(0, 1).reshape(T, n_head * d_head)


def attention_rows(qkv, lens, n_head, d_head):
    """qkv [B, T, 3 H D] -> [B, T, H D]: every row alone over its own keys, zeros behind it; nothing behind a row's length is read."""
    B, T, _ = qkv.shape
    out = torch.zeros(B, T, n_head * d_head, dtype=qkv.dtype)
    for b, n in enumerate([T] * B if lens is None else lens):
        if n > 0:
            out[b, :n] = attention(qkv[b, :n], n_head, d_head)
    return out


def attention_pair(qkv, lens, n_head, d_head):
    """-> (the float64 result, the float32 restatement's largest distance from it)."""
    want = attention_rows(qkv.double(), lens, n_head, d_head)
    got = attention_rows(qkv.float(), lens, n_head, d_head)
    return want, (got.double() - want).abs().max().item()


def plan(dur, pace, min_token_frames, max_decoder_steps):
    """dur [L] (frames, any float dtype) -> the integer plan: reps_l = max(floor(dur_l / pace + 0.5), min_token_frames), a row cut at
    ``max_decoder_steps`` frames, and a row of 0 frames gets one frame of its last token.  -> (reps [L] int64, starts [L] int64)."""
    reps = torch.clamp(torch.floor(dur / pace + 0.5), min=float(min_token_frames)).to(torch.int64)
    ends = torch.clamp(torch.cumsum(reps, 0), max=max_decoder_steps)
    starts = torch.cat([ends.new_zeros(1), ends[:-1]])
    reps = ends - starts
    if int(reps.sum()) == 0:
        reps[-1] = 1
    return reps, starts


class _Attn(nn.Module):
    def __init__(self, d_model, n_head, d_head):
        super().__init__()
        self.n_head, self.d_head = n_head, d_head
        self.qkv_net = nn.Linear(d_model, 3 * n_head * d_head)
        self.o_net = nn.Linear(n_head * d_head, d_model, bias=False)
        self.layer_norm = nn.LayerNorm(d_model, eps=LN_EPS)

    def forward(self, x):   # [T, C]
        return self.layer_norm(x + self.o_net(attention(self.qkv_net(x), self.n_head, self.d_head)))


class _PosFF(nn.Module):
    def __init__(self, d_model, d_inner, k):
        super().__init__()
        self.CoreNet = nn.Sequential(nn.Conv1d(d_model, d_inner, k, padding=k // 2), nn.ReLU(), nn.Conv1d(d_inner, d_model, k, padding=k // 2))
        self.layer_norm = nn.LayerNorm(d_model, eps=LN_EPS)

    def forward(self, x):
        return self.layer_norm(x + self.CoreNet(x.t()[None])[0].t())


class _Layer(nn.Module):
    def __init__(self, d_model, n_head, d_head, d_inner, k):
        super().__init__()
        self.dec_attn = _Attn(d_model, n_head, d_head)
        self.pos_ff = _PosFF(d_model, d_inner, k)

    def forward(self, x):
        return self.pos_ff(self.dec_attn(x))


class _Stack(nn.Module):
    def __init__(self, cfg, s, n_tokens=None):
        super().__init__()
        if n_tokens is not None:
            self.word_emb = nn.Embedding(n_tokens, cfg["d_model"])
        self.layers = nn.ModuleList([_Layer(cfg["d_model"], cfg[f"{s}_n_head"], cfg[f"{s}_d_head"], cfg[f"{s}_d_inner"], cfg[f"{s}_kernel_size"])
                                     for _ in range(cfg[f"{s}_n_layers"])])

    def forward(self, x):
        """x [T, C] with the position table added -> (x, [x after every layer])."""
        stages = []
        for layer in self.layers:
            x = layer(x)
            stages.append(x)
        return x, stages


class _PredLayer(nn.Module):
    def __init__(self, c_in, width):
        super().__init__()
        self.conv = nn.Conv1d(c_in, width, 3, padding=1)
        self.norm = nn.LayerNorm(width, eps=LN_EPS)

    def forward(self, x):   # [T, C]
        return self.norm(F.relu(self.conv(x.t()[None])[0].t()))


class _Predictor(nn.Module):
    def __init__(self, d_model, width, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([_PredLayer(d_model if i == 0 else width, width) for i in range(n_layers)])
        self.fc = nn.Linear(width, 1)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return self.fc(x)[:, 0]


class Model(nn.Module):
    """Random weights under the published names: N(0, 1 / fan_in) products, biases and LayerNorm shifts of 0.1, LayerNorm scales around 1,
    and ``duration_predictor.fc.bias`` at ``dur_bias`` so that a token gets a few frames."""

    def __init__(self, cfg, seed=0, dur_bias=1.2):
        super().__init__()
        cfg = full(cfg)
        self.cfg = cfg
        C_, W, n = cfg["d_model"], cfg["predictor_filter_size"], cfg["predictor_n_layers"]
        self.encoder = _Stack(cfg, "enc", cfg["n_tokens"])
        self.decoder = _Stack(cfg, "dec")
        self.duration_predictor = _Predictor(C_, W, n)
        self.pitch_predictor = _Predictor(C_, W, n)
        self.pitch_emb = nn.Conv1d(1, C_, 3, padding=1)
        if cfg["energy_conditioning"]:
            self.energy_predictor = _Predictor(C_, W, n)
            self.energy_emb = nn.Conv1d(1, C_, 3, padding=1)
        self.proj = nn.Linear(C_, cfg["n_mels"])
        self.register_buffer("pitch_mean", torch.zeros(1))
        self.register_buffer("pitch_std", torch.ones(1))
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if "norm" in name and name.endswith("weight"):
                    p.copy_(0.75 + 0.5 * torch.rand(p.shape, generator=g, dtype=torch.float64))
                elif name.endswith("bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
                elif name.endswith("word_emb.weight"):
                    p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64))
                else:
                    p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * p[0].numel() ** -0.5)
            self.duration_predictor.fc.bias.fill_(dur_bias)
        self.double()   # (the values were drawn into float32 parameters: the restatement holds exactly what the device holds)

    def forward(self, tokens, pace=1.0, durations=None, pitch=None, reps=None):
        """One row: tokens int64 [L] -> a dict of that row's tensors.  ``durations`` [L] replace the predicted ones in front of the plan,
        ``pitch`` [L] replaces the predicted pitch, ``reps`` [L] (int) replaces the plan's result."""
        cfg = self.cfg
        dtype = self.proj.weight.dtype
        L = tokens.shape[0]
        x = self.encoder.word_emb(tokens) + position_table(L, cfg["d_model"], dtype)
        enc_stages = [x]
        x, st = self.encoder(x)
        enc_stages += st
        log_dur = self.duration_predictor(x)
        dur = torch.clamp(torch.exp(log_dur) - 1.0, 0.0, float(cfg["max_duration"]))
        pitch_pred = self.pitch_predictor(x)
        p = pitch_pred if pitch is None else pitch.to(dtype)
        x = x + self.pitch_emb(p[None, None])[0].t()
        if cfg["energy_conditioning"]:
            energy_pred = self.energy_predictor(x)
            x = x + self.energy_emb(energy_pred[None, None])[0].t()
        else:
            energy_pred = torch.zeros_like(pitch_pred)
        if reps is None:
            reps, _ = plan(dur if durations is None else durations.to(dtype), pace, cfg["min_token_frames"], cfg["max_decoder_steps"])
        reps = reps.to(torch.int64)
        T = int(reps.sum())
        y = torch.repeat_interleave(x, reps, dim=0) + position_table(T, cfg["d_model"], dtype)
        dec_stages = [y]
        y, st = self.decoder(y)
        dec_stages += st
        mel = self.proj(y).t()   # [n_mels, T]
        align = torch.repeat_interleave(torch.eye(L, dtype=dtype), reps, dim=0)   # [T, L]
        return {"enc_stages": enc_stages, "log_durations": log_dur, "dur": dur, "pitch_pred": pitch_pred, "energy_pred": energy_pred, "durations": reps,
                "dec_stages": dec_stages, "mel": mel, "alignments": align, "frames": T}


def random_tokens(cfg, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, full(cfg)["n_tokens"], (B, L), generator=g)


def _ragged(module, tokens, lens, pace, durations, pitch, reps):
    """Every row alone at its own length, assembled with zeros behind a row: the stage list in the device's order - x after the embedding
    and after every encoder layer [B, L, C], log_durations, pitch_pred, energy_pred [B, L], the regulated sequence and x after every decoder
    layer [B, T, C], the mel [B, n_mels, T] - and the other per-row tensors."""
    B, L = tokens.shape
    lens = [L] * B if lens is None else list(lens)
    rows = []
    for b, n in enumerate(lens):
        pick = lambda t: None if t is None else t[b, :n]
        rows.append(module(tokens[b, :n], pace, pick(durations), pick(pitch), pick(reps)))
    T = max(r["frames"] for r in rows)
    dtype = rows[0]["mel"].dtype
    pad2 = lambda key, width: [torch.stack([F.pad(r[key][i], (0, 0, 0, width - r[key][i].shape[0])) for r in rows]) for i in range(len(rows[0][key]))]
    pad1 = lambda key: torch.stack([F.pad(r[key], (0, L - r[key].shape[0])) for r in rows])
    mel = torch.stack([F.pad(r["mel"], (0, T - r["frames"])) for r in rows])
    stages = pad2("enc_stages", L) + [pad1("log_durations"), pad1("pitch_pred"), pad1("energy_pred")] + pad2("dec_stages", T) + [mel]
    align = torch.zeros(B, T, L, dtype=dtype)
    for b, r in enumerate(rows):
        align[b, :r["frames"], :lens[b]] = r["alignments"]
    return {"stages": stages, "mel": mel, "alignments": align, "durations": pad1("durations"), "dur": pad1("dur"),
            "frames": [r["frames"] for r in rows]}


def stage_names(cfg):
    cfg = full(cfg)
    return ([f"encoder x{i}" for i in range(cfg["enc_n_layers"] + 1)] + ["log_durations", "pitch_pred", "energy_pred"]
            + [f"decoder x{i}" for i in range(cfg["dec_n_layers"] + 1)] + ["mel"])


def reference_pair(ref, tokens, lens=None, pace=1.0, durations=None, pitch=None, reps=None):
    """-> (the float64 outputs (``_ragged``'s dict), the float32 restatement's largest distance from them per stage tensor, and its
    largest distance on ``dur``).  The float32 restatement decodes the float64 plan's frames, so that both have one shape."""
    with torch.no_grad():
        want = _ragged(ref, tokens, lens, pace, durations, pitch, reps)
        ref32 = copy.deepcopy(ref).float()
        ref32.cfg = ref.cfg
        got = _ragged(ref32, tokens, lens, pace, durations, None if pitch is None else pitch.float(), want["durations"])
    errs = [(g.double() - w).abs().max().item() for g, w in zip(got["stages"], want["stages"])]
    return want, errs, (got["dur"].double() - want["dur"]).abs().max().item()


# ---- the cases tests/test_fastpitch_gpu.py runs, by name: (configuration, B, L, token lengths or None).  tests/test_fastpitch_cpu.py
# asserts for each that no token's duration lies inside the margin of a rounding decision (``undecided``)
ULP = 2.0 ** -23
FACTOR = 8.0
CASES = {"narrow 2 x 5": ("NARROW", 2, 5, None), "twohead ragged": ("TWOHEAD", 3, 33, (33, 2, 17)), "default 1 x 12": ("DEFAULT", 1, 12, None),
         "default 2 x 70": ("DEFAULT", 2, 70, None), "asym ragged": ("ASYM", 3, 17, (17, 1, 16)), "wide 2 x 15": ("WIDE", 2, 15, None),
         "topheavy ragged": ("TOPHEAVY", 2, 33, (33, 31)), "narrow 1 x 1": ("NARROW", 1, 1, None), "narrow long": ("NARROW", 2, 300, (300, 257))}
MODEL_SEED = 11


# "narrow 1 x 1" draws its token from a seed of its own.  With one token log_durations, pitch_pred and energy_pred are ONE number each,
# and the float32 restatement's error on one number is a single draw of its rounding, which depends on the order in which the host's
# library sums: for the token of seed 1011 (id 19, pitch_pred -0.2953) it is 4.6e-07 on one host and 1.1e-08 on another, while float32
# evaluated in 300 summation orders is off by 1.1e-08 .. 2.0e-06 - so the 8 x rule passed or failed by the host.  The rule's other term, one
# ulp at the number's scale, does not depend on the host.  Seed 7 draws id 15, whose three numbers (2.03, 0.87, -1.41) are large against
# what the encoder output's float32 error moves them, so that term decides: tests/test_fastpitch_cpu.py asserts it
# (``one_token_movement``), in float64, for whatever token this seed draws.
TOKEN_SEEDS = {"narrow 1 x 1": 7}


def case_tokens(name):
    cfg_name, B, L, _ = CASES[name]
    return random_tokens(globals()[cfg_name], B, L, seed=TOKEN_SEEDS.get(name, 1000 + 10 * B + L))


def one_token_movement(ref, token, draws=200, seed=0):
    """For a row of ONE token: (the float64 log_durations, pitch_pred and energy_pred [3], and the 90th percentile [3] of how far they move
    when the encoder's output is perturbed, element by element and uniformly, by up to the float32 restatement's largest error on it)."""
    with torch.no_grad():
        tok = torch.tensor([int(token)])
        want = ref(tok)
        ref32 = copy.deepcopy(ref).float()
        ref32.cfg = ref.cfg
        x = want["enc_stages"][-1]
        err = (ref32(tok)["enc_stages"][-1].double() - x).abs().max().item()

        def tail(x):
            log_dur, pitch = ref.duration_predictor(x), ref.pitch_predictor(x)
            out = [log_dur[0], pitch[0]]
            if ref.cfg["energy_conditioning"]:
                out.append(ref.energy_predictor(x + ref.pitch_emb(pitch[None, None])[0].t())[0])
            return torch.stack(out)

        base = tail(x)
        g = torch.Generator().manual_seed(seed)
        moved = torch.stack([(tail(x + (2.0 * torch.rand(x.shape, generator=g, dtype=torch.float64) - 1.0) * err) - base).abs() for _ in range(draws)])
    return base, moved.quantile(0.9, dim=0)


def case_durations(name):
    """The given durations of a case: 0 .. 5 frames a token, int64 [B, L]; a row's first token gets at least one frame."""
    _, B, L, _ = CASES[name]
    g = torch.Generator().manual_seed(77 + L)
    d = torch.randint(0, 6, (B, L), generator=g)
    d[:, 0] += 1
    return d


def undecided(want, err_dur, lens=None, pace=1.0):
    """bool [B, L]: the tokens whose float64 ``dur / pace + 0.5`` lies within FACTOR x max(the float32 restatement's error on dur, one ulp
    at dur's scale) of an integer - where float32 arithmetic may legitimately round the other way."""
    dur = want["dur"]
    margin = FACTOR * max(err_dur, ULP * dur.abs().max().item())
    x = dur / pace + 0.5
    near = (x - torch.round(x)).abs() <= margin
    if lens is not None:
        for b, n in enumerate(lens):
            near[b, n:] = False
    return near
