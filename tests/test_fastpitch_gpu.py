"""GPU: FastPitch (gvx_fastpitch_encode / gvx_fastpitch_decode, csrc/fastpitch.hip, through ``FastPitch``) against the float64 restatement
of tests/fastpitch_ref64.py: every stage tensor - x after the embedding and after every encoder layer, the three predictors' outputs,
the regulated sequence, x after every decoder layer - and the mel, element by element.

Tolerance: the 8 x rule of tests/test_vocos_gpu.py.  Every case evaluates the SAME restatement in float32 on the CPU and takes, tensor by
tensor, its largest distance from float64; the device may differ from float64 by at most 8 times the larger of that number and one
float32 ulp at the tensor's scale.  The ratio is printed.

Discrete decisions: a predicted duration is compared as an integer only where the float64 ``dur / pace + 0.5`` lies farther from an integer
than 8 x max(float32 restatement's error on dur, one ulp at its scale); tests/test_fastpitch_cpu.py asserts that no token of these
cases lies inside that margin, so nothing is excluded unless the device is wrong.  The decoder is then checked on the device's own
durations.

The cases (tests/fastpitch_ref64.py, ``CASES``): NARROW, TWOHEAD and DEFAULT share equal stacks, kernel size 3, two predictor layers,
energy conditioning and widths of 32, 128 and 384.  ASYM (d_model 96: a kernel-1 one-layer encoder, a kernel-3 three-layer decoder of four
heads, inner widths 96 and 160, three predictor layers of 160, no energy branch, 33 mel bins), WIDE (d_model 512: inner widths 64 and 32, a
kernel-1 decoder, one predictor layer of 288, 7 mel bins) and TOPHEAVY (d_model 32 under 2 x 64 and 16 x 32 heads, ``min_token_frames`` 2,
``max_duration`` 3, which the predicted durations reach at both ends) run what those never do: the haloed row offset of ``pad = 0``, the
workspace's maxima over unequal stacks, the blob without the third predictor, the predictors' ping-pong ending in either buffer, and
LayerNorm widths whose last 64-lane chunk is partly idle.  "narrow 1 x 1" is one token (drawn from a seed of its own, ``TOKEN_SEEDS``:
the predictors' outputs are then one number each, and the token is one at which the rule is decided by its ulp term, not by the order in
which the host's library sums in float32); "narrow long" (300 and 257 tokens, 700 - 850
frames) takes the plan kernel's strided loops through a second pass and the attention through 14 key tiles and 7 query tiles.  With
energy conditioning off, ``energy_pred`` is all zeros in float64: the device's must be exact zeros.

Beyond the cases: bit equality of ragged rows with the rows alone (TWOHEAD and ASYM), one token with one frame, a cut on a token boundary
and a cut row beside a whole one, the predicted path at both clamps and through the empty-row rule (``duration_predictor.fc`` set to a
constant), and token ids outside the table.

Largest ratios seen on an MI355X: see README.md, "FastPitch"."""
import functools

import pytest
import torch

from genvox_amd import metrics
from genvox_amd.configs import AudioConfig, FastPitchConfig, TextConfig
from genvox_amd.fastpitch import FastPitch
from tests import fastpitch_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = R.FACTOR
ULP = R.ULP
NAN = float("nan")


def _build(cfg, **more):
    ac = AudioConfig()
    ac.n_mels = cfg["n_mels"]   # WIDE's 7 bins: below what AudioConfig's constructor takes (a mel front end's range), inside the model's [1, 4096]
    return FastPitch(FastPitchConfig(**{**R.model_kwargs(cfg), **more}), ac, TextConfig(n_tokens=cfg["n_tokens"]))


@functools.lru_cache(maxsize=None)
def _net(name):
    """(the restatement's module with random weights, the device module with the same ones)."""
    cfg = getattr(R, name)
    ref = R.Model(cfg, seed=R.MODEL_SEED)
    model = _build(cfg)
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return cfg, ref, model.to(DEV)


@functools.lru_cache(maxsize=None)
def _given(name):
    """A case on its GIVEN durations: (tokens, lens, durations, the float64 outputs, the float32 restatement's error per stage)."""
    cfg_name, B, L, lens = R.CASES[name]
    tokens, durations = R.case_tokens(name), R.case_durations(name)
    want, errs, _ = R.reference_pair(_net(cfg_name)[1], tokens, lens, durations=durations)
    return tokens, lens, durations, want, errs


@functools.lru_cache(maxsize=None)
def _predicted(name):
    cfg_name, B, L, lens = R.CASES[name]
    tokens = R.case_tokens(name)
    return (tokens, lens) + R.reference_pair(_net(cfg_name)[1], tokens, lens)


def _inputs(tokens, lens, **more):
    inputs = {"tokens": tokens.to(DEV), **more}   # durations and pitch from the host: the module checks them there and moves them
    if lens is not None:
        inputs["token_lengths"] = torch.tensor(lens)
    return inputs


def _run(model, inputs, frames=None):
    """-> (outputs, stages).  ``frames`` (the decoder's length, where the caller knows it): the call runs on an exactly sized workspace
    that starts as NaN."""
    ws = None
    if frames is not None:
        B, L = inputs["tokens"].shape
        need = max(model.workspace_bytes(B, L), model.workspace_bytes(B, frames))
        ws = torch.full((need // 4,), NAN, dtype=torch.float32, device=DEV).view(torch.uint8)
    out, stages = model._run(inputs, stage_outputs=True, workspace=ws)
    torch.cuda.synchronize()
    return out, stages


def _compare(got, want, errs, names, what):
    assert len(got) == len(want) == len(names)
    for name, g, w, e in zip(names, got, want, errs):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not w.any():   # (energy_pred without energy conditioning) the rule's base is 0: exact zeros, and no ratio to print
            assert not g.any(), f"{what}: {name} is all zeros in float64 and not on the device"
            print(f"{what}: {name}: all zeros in float64, exact zeros on the device")
            continue
        d = (g.double().cpu() - w).abs().max().item()
        base = max(e, ULP * w.abs().max().item())
        print(f"{what}: {name}: device error {d:.3e}, float32 restatement error {e:.3e}, one ulp at scale {ULP * w.abs().max().item():.3e}, ratio {d / base:.2f}")
        assert d <= FACTOR * base, f"{what}: {name} differs from float64 by {d:.3e}, above {FACTOR} x {base:.3e}"


def _zeros_behind(out, stages, lens, frames, n_enc):
    B, L = out["durations"].shape
    for b in range(B):
        n, t = (L if lens is None else lens[b]), frames[b]
        for s in stages[:n_enc + 4]:   # the encoder's tensors and the predictors'
            assert not s[b, n:].any()
        for s in stages[n_enc + 4:-1]:
            assert not s[b, t:].any()
        assert not out["mel_outputs_postnet"][b, :, t:].any() and not out["alignments"][b, t:].any() and not out["alignments"][b, :, n:].any()
        assert not out["durations"][b, n:].any()
        gate = out["gate_outputs"][b]
        assert (gate[:t - 1] == -1e3).all() and (gate[t - 1:] == 1e3).all()


def _alignment_of(durations, T):
    """The exact 0 / 1 matrix [B, T, L] of integer durations [B, L]."""
    B, L = durations.shape
    a = torch.zeros(B, T, L)
    for b in range(B):
        rows = torch.repeat_interleave(torch.eye(L), durations[b].long().cpu(), dim=0)
        a[b, :rows.shape[0]] = rows
    return a


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_stage_and_the_mel_on_given_durations(name):
    """NARROW 2 x 5: one 32-wide head, half-idle waves in the LayerNorm; TWOHEAD ragged (33, 2, 17); DEFAULT 1 x 12 and 2 x 70: the published
    sizes; ASYM ragged (17, 1, 16), WIDE 2 x 15, TOPHEAVY ragged (33, 31), NARROW 1 x 1 and NARROW long (300, 257): the module docstring.
    The durations are given, so the decoder's length is the plan's."""
    cfg_name = R.CASES[name][0]
    cfg, _, model = _net(cfg_name)
    tokens, lens, durations, want, errs = _given(name)
    T = max(want["frames"])
    out, stages = _run(model, _inputs(tokens, lens, durations=durations), frames=T)
    _compare(stages, want["stages"], errs, R.stage_names(cfg), name)
    _zeros_behind(out, stages, lens, want["frames"], R.full(cfg)["enc_n_layers"])
    assert out["mel_outputs"] is out["mel_outputs_postnet"] and out["mel_outputs"].shape == (tokens.shape[0], cfg["n_mels"], T)
    assert torch.equal(out["durations"].cpu().long(), want["durations"])
    assert torch.equal(out["alignments"].cpu(), _alignment_of(out["durations"], T)) and torch.equal(out["alignments"].cpu().double(), want["alignments"])
    if tokens.shape[0] > 1:
        assert out["mel_lengths"].dtype == torch.int32 and out["mel_lengths"].tolist() == want["frames"]
    else:
        assert "mel_lengths" not in out


@pytest.mark.parametrize("name", list(R.CASES))
def test_predicted_durations_and_the_decoder_on_the_devices_own(name):
    cfg_name = R.CASES[name][0]
    cfg, ref, model = _net(cfg_name)
    tokens, lens, want, errs, err_dur = _predicted(name)
    out, stages = _run(model, _inputs(tokens, lens))
    names = R.stage_names(cfg)
    n_enc = R.full(cfg)["enc_n_layers"]
    _compare(stages[:n_enc + 4], want["stages"][:n_enc + 4], errs[:n_enc + 4], names[:n_enc + 4], name)   # log_durations among them
    decided = ~R.undecided(want, err_dur, lens)
    assert decided.all(), "tests/test_fastpitch_cpu.py asserts that no token lies inside the margin"
    got_dur = out["durations"].cpu().long()
    assert torch.equal(got_dur[decided], want["durations"][decided]), f"{name}: a decided duration differs"
    if not torch.equal(got_dur, want["durations"]):   # (unreachable while the exclusion is empty) the reference on the device's own plan
        want, errs, _ = R.reference_pair(ref, tokens, lens, reps=got_dur)
    _compare(stages[n_enc + 4:], want["stages"][n_enc + 4:], errs[n_enc + 4:], names[n_enc + 4:], name + ", own durations")
    _zeros_behind(out, stages, lens, out["durations"].sum(1).tolist(), n_enc)
    assert torch.equal(out["alignments"].cpu(), _alignment_of(out["durations"], out["alignments"].shape[1]))


def test_ragged_rows_equal_the_rows_alone_bit_for_bit():
    """Through the whole model, on predicted durations: rows of 33, 2 and 17 tokens (TWOHEAD) and of 17, 1 and 16 (ASYM: a kernel-1 and a
    kernel-3 stack, three predictor layers, no energy branch), NaN-free padding tokens that must not matter."""
    for cfg_name, case in (("TWOHEAD", "twohead ragged"), ("ASYM", "asym ragged")):
        cfg, _, model = _net(cfg_name)
        tokens, lens = R.case_tokens(case), R.CASES[case][3]
        out, stages = _run(model, _inputs(tokens, lens))
        other = tokens.clone()
        for b, n in enumerate(lens):
            other[b, n:] = (other[b, n:] + 7) % cfg["n_tokens"]   # the padded tokens are never read
        out2, _ = _run(model, _inputs(other, lens))
        assert torch.equal(out["mel_outputs"], out2["mel_outputs"])
        for b, n in enumerate(lens):
            alone, alone_stages = _run(model, _inputs(tokens[b:b + 1, :n], None))
            t = alone["mel_outputs"].shape[2]
            assert out["mel_lengths"][b].item() == t
            assert torch.equal(out["mel_outputs"][b, :, :t], alone["mel_outputs"][0]), f"{case}: row {b}"
            assert torch.equal(out["durations"][b, :n], alone["durations"][0]) and torch.equal(out["alignments"][b, :t, :n], alone["alignments"][0])
            for s, a in zip(stages[:-1], alone_stages[:-1]):
                assert torch.equal(s[b, :a.shape[1]], a[0]), f"{case}: row {b}"


def test_one_token_one_frame():
    """B = L = T = 1: in every LayerNorm launch one wave writes the position and both halo rows, every product has one row, the softmax one
    key.  Every stage against float64, on a NaN-filled, exactly sized workspace.

    The token is the one "narrow 1 x 1" draws: tests/fastpitch_ref64.py, ``TOKEN_SEEDS``, says why that case has a seed of its own."""
    cfg, ref, model = _net("NARROW")
    tokens = R.case_tokens("narrow 1 x 1")
    durations = torch.tensor([[1]])
    want, errs, _ = R.reference_pair(ref, tokens, None, durations=durations)
    assert want["frames"] == [1]
    out, stages = _run(model, _inputs(tokens, None, durations=durations), frames=1)
    _compare(stages, want["stages"], errs, R.stage_names(cfg), "1 token, 1 frame")
    assert out["mel_outputs"].shape == (1, cfg["n_mels"], 1) and out["durations"].tolist() == [[1]]
    assert out["alignments"].tolist() == [[[1.0]]] and out["gate_outputs"].tolist() == [[1e3]]


def test_a_cut_on_a_token_boundary_and_a_cut_row_beside_a_whole_one():
    cfg, _, shared = _net("NARROW")
    cut_cfg = {**cfg, "max_decoder_steps": 6}
    ref = R.Model(cut_cfg, seed=R.MODEL_SEED)   # (the same weights: the seed draws them in the same order)
    cut = _build(cut_cfg).to(DEV)
    cut.load_state_dict(shared.state_dict())
    tokens = R.random_tokens(cfg, 2, 5, seed=31)
    # the cut lands exactly behind the second token: the third gets nothing
    durations = torch.tensor([[2, 4, 5]])
    assert R.plan(durations[0].double(), 1.0, 0, 6)[0].tolist() == [2, 4, 0]
    out = cut.inference(_inputs(tokens[:1, :3], None, durations=durations))
    assert out["durations"].tolist() == [[2, 4, 0]] and out["mel_outputs"].shape[2] == 6
    assert torch.equal(out["alignments"].cpu(), _alignment_of(out["durations"], 6))
    # a ragged batch: row 0 is cut (on a token boundary as well), row 1 (3 tokens, 4 frames) is not
    lens = (5, 3)
    durations = torch.tensor([[3, 3, 3, 3, 3], [1, 2, 1, 9, 9]])
    want, errs, _ = R.reference_pair(ref, tokens, lens, durations=durations)
    assert want["durations"].tolist() == [[3, 3, 0, 0, 0], [1, 2, 1, 0, 0]] and want["frames"] == [6, 4]
    out, stages = _run(cut, _inputs(tokens, lens, durations=durations), frames=6)
    assert torch.equal(out["durations"].cpu().long(), want["durations"]) and out["mel_lengths"].tolist() == [6, 4]
    assert torch.equal(out["alignments"].cpu(), _alignment_of(out["durations"], 6)) and torch.equal(out["alignments"].cpu().double(), want["alignments"])
    _compare(stages, want["stages"], errs, R.stage_names(cfg), "cut at 6 frames, ragged")
    _zeros_behind(out, stages, lens, want["frames"], R.full(cfg)["enc_n_layers"])


def _constant_log_duration(cfg, shared, b, **more):
    """The model with ``duration_predictor.fc`` at weight 0 and bias ``b``: ``log_durations == b`` on every token."""
    model = _build({**cfg, **more}).to(DEV)
    sd = {k: v.clone() for k, v in shared.state_dict().items()}
    sd["duration_predictor.fc.weight"].zero_()
    sd["duration_predictor.fc.bias"].fill_(b)
    model.load_state_dict(sd)
    return model


def _planned(b, lens, L, pace, cfg):
    """The float64 plan of ``log_durations == fl32(b)`` for rows of ``lens`` tokens -> (durations [B, L] int64, the least distance of
    ``dur / pace + 0.5`` from an integer)."""
    cfg = R.full(cfg)
    b64 = torch.tensor(b, dtype=torch.float32).double()
    dur = torch.clamp(torch.exp(b64) - 1.0, 0.0, float(cfg["max_duration"]))
    x = dur / pace + 0.5
    out = torch.zeros(len(lens), L, dtype=torch.int64)
    for i, n in enumerate(lens):
        out[i, :n] = R.plan(dur.expand(n), pace, cfg["min_token_frames"], cfg["max_decoder_steps"])[0]
    return out, (x - torch.round(x)).abs().item()


def test_both_clamps_and_the_empty_row_on_the_predicted_path():
    """The predicted durations at ``max_duration`` and at 0 (where the last token of each row's own length gets the row's one frame), and a
    duration in between under a pace, with ``min_token_frames`` 0 and 2.  The expected durations are the float64 plan's."""
    import math

    cfg, _, shared = _net("NARROW")
    tokens = R.random_tokens(cfg, 2, 5, seed=32)
    lens = (5, 3)

    def run(b, pace, **more):
        model = _constant_log_duration(cfg, shared, b, **more)
        out = model.inference(_inputs(tokens, lens, pace=pace))
        want, margin = _planned(b, lens, 5, pace, {**cfg, **more})
        assert margin >= 0.1, "float32 arithmetic must not be able to round the other way"
        valid = torch.arange(5)[None, :] < torch.tensor(lens)[:, None]
        assert (out["log_durations"].cpu()[valid] == torch.tensor(b, dtype=torch.float32)).all() and not out["log_durations"].cpu()[~valid].any()
        assert torch.equal(out["durations"].cpu().long(), want), (b, pace, more, out["durations"].tolist())
        T = int(want.sum(1).max())
        assert out["mel_lengths"].tolist() == want.sum(1).tolist() and out["mel_outputs"].shape[2] == T
        assert torch.equal(out["alignments"].cpu(), _alignment_of(out["durations"], T))
        assert torch.isfinite(out["mel_outputs"]).all()
        for i, t in enumerate(want.sum(1).tolist()):
            assert not out["mel_outputs"][i, :, t:].any()
        return want

    assert run(math.log(76.0) + 0.5, 1.0).tolist() == [[75] * 5, [75] * 3 + [0, 0]]      # the clamp at max_duration = 75
    assert run(-2.0, 1.0).tolist() == [[0, 0, 0, 0, 1], [0, 0, 1, 0, 0]]                 # the clamp at 0, then the empty row's one frame
    # exp(0.9) - 1 = 1.4596; under pace 1.25: 1.1677 + 0.5 = 1.6677, 0.33 from an integer
    assert run(0.9, 1.25).tolist() == [[1] * 5, [1] * 3 + [0, 0]]
    assert run(0.9, 1.25, min_token_frames=2).tolist() == [[2] * 5, [2] * 3 + [0, 0]]


def test_a_token_id_outside_the_table_is_read_as_id_0():
    """include/genvox_amd.h: "a token outside [0, n_tokens) reads row 0"."""
    cfg, _, model = _net("NARROW")
    tokens = R.random_tokens(cfg, 2, 5, seed=33)
    tokens[0, 1], tokens[1, 0], tokens[1, 4] = cfg["n_tokens"], -1, 10 ** 6
    zeroed = tokens.clone()
    zeroed[0, 1] = zeroed[1, 0] = zeroed[1, 4] = 0
    out, stages = _run(model, _inputs(tokens, None))
    want, want_stages = _run(model, _inputs(zeroed, None))
    for key in ("mel_outputs", "alignments", "gate_outputs", "log_durations", "pitch_pred", "energy_pred", "durations", "mel_lengths"):
        assert torch.equal(out[key], want[key]), key
    assert all(torch.equal(a, b) for a, b in zip(stages, want_stages)) and torch.isfinite(out["mel_outputs"]).all()


def test_rows_do_not_depend_on_the_gemm_tile_shape():
    """4 rows, three of 110 tokens x 75 frames = 8,250 frames: 33,000 decoder rows, which plan_gemm covers with 128 x 128 tiles for the first
    32,768 and 64 x 64 tiles for the rest (N = 256 and N = 384: remainders of 4 and 6 tiles over whole rounds of 256), while a row alone
    runs on 64 x 64 tiles throughout.  The last row lies across the cut; row 1 is short (2 tokens, 40 frames)."""
    cfg, _, shared = _net("TWOHEAD")
    model = _build(cfg, max_decoder_steps=8250).to(DEV)
    model.load_state_dict(shared.state_dict())
    tokens = R.random_tokens(cfg, 4, 110, seed=8)
    lens = (110, 2, 110, 110)
    durations = torch.full((4, 110), 75)
    durations[1, :2] = 20
    out = model.inference(_inputs(tokens, lens, durations=durations))
    assert out["mel_lengths"].tolist() == [8250, 40, 8250, 8250]
    for b in (1, 3):
        n, t = lens[b], out["mel_lengths"][b].item()
        alone = model.inference(_inputs(tokens[b:b + 1, :n], None, durations=durations[b:b + 1, :n]))
        assert torch.equal(out["mel_outputs"][b, :, :t], alone["mel_outputs"][0]), f"row {b}"
        assert not out["mel_outputs"][b, :, t:].any()


def test_pace_durations_and_pitch_inputs():
    cfg, ref, model = _net("NARROW")
    tokens = R.case_tokens("narrow 2 x 5")
    durations = torch.tensor([[1, 0, 3, 2, 5], [0, 0, 1, 7, 2]])
    for pace, want in ((1.0, durations.tolist()), (0.5, (2 * durations).tolist()), (2.0, [[1, 0, 2, 1, 3], [0, 0, 1, 4, 1]])):   # floor(d / 2 + 0.5)
        out = model.inference(_inputs(tokens, None, durations=durations, pace=pace))
        assert out["durations"].tolist() == want and out["mel_lengths"].tolist() == [sum(r) for r in want]
    # a given pitch replaces the predicted one in front of pitch_emb; pitch_pred stays the prediction
    g = torch.Generator().manual_seed(3)
    pitch = torch.randn(2, 5, generator=g)
    want, errs, _ = R.reference_pair(ref, tokens, None, durations=durations, pitch=pitch.double())
    out, stages = _run(model, _inputs(tokens, None, durations=durations, pitch=pitch), frames=max(want["frames"]))
    _compare(stages, want["stages"], errs, R.stage_names(cfg), "narrow, given pitch")
    plain, _ = _run(model, _inputs(tokens, None, durations=durations))
    assert torch.equal(plain["pitch_pred"], out["pitch_pred"]) and not torch.equal(plain["mel_outputs"], out["mel_outputs"])
    # predicted durations under a pace: the plan of the device's own log-durations
    out = model.inference(_inputs(tokens, None, pace=2.0))
    dur = torch.clamp(torch.exp(out["log_durations"].double().cpu()) - 1.0, 0.0, 75.0)
    x = dur / 2.0 + 0.5
    clear = (x - torch.round(x)).abs() > 1e-4
    assert torch.equal(out["durations"].cpu().long()[clear], torch.floor(x).long()[clear])
    for bad in (dict(pace=0.1), dict(pace=9.0), dict(attention_window=(2, 4)), dict(durations=torch.ones(2, 5)), dict(durations=torch.ones(2, 4, dtype=torch.int64)),
                dict(pitch=torch.zeros(2, 6)), dict(durations=-torch.ones(2, 5, dtype=torch.int64))):
        with pytest.raises(ValueError):
            model.inference(_inputs(tokens, None, **bad))
    with pytest.raises(ValueError):
        model.inference(_inputs(tokens, (5, 6)))


def test_the_cut_the_empty_row_and_monotonic_alignment_search():
    cfg, _, shared = _net("NARROW")
    tokens = R.case_tokens("narrow 2 x 5")
    cut = _build(cfg, max_decoder_steps=6).to(DEV)
    cut.load_state_dict(shared.state_dict())
    out = cut.inference(_inputs(tokens, (5, 3), durations=torch.tensor([[1, 0, 3, 4, 5], [0, 0, 0, 9, 9]])))
    assert out["durations"].tolist() == [[1, 0, 3, 2, 0], [0, 0, 1, 0, 0]]   # cut at 6 frames; a row of 0 frames gets one of its last token
    assert out["mel_lengths"].tolist() == [6, 1] and out["mel_outputs"].shape[2] == 6
    assert torch.equal(out["alignments"].cpu(), _alignment_of(out["durations"], 6))
    # with min_token_frames = 1 every token has a frame, and the search over the 0 / 1 alignment returns the durations exactly
    least = _build(cfg, min_token_frames=1).to(DEV)
    least.load_state_dict(shared.state_dict())
    lens = (5, 3)
    out = least.inference(_inputs(tokens, lens))
    dur = out["durations"]
    assert all((dur[b, :n] >= 1).all() and not dur[b, n:].any() for b, n in enumerate(lens))
    found = metrics.monotonic_align(out["alignments"], out["mel_lengths"], torch.tensor(lens, device=DEV))
    assert found["status"].tolist() == [0, 0] and torch.equal(found["durations"], dur)


def test_workspace_contract_and_a_changed_weight_repacks():
    """A NaN-filled, exactly sized workspace gives the bits of the module's own (dirty) one; one byte short is refused; two calls give the
    same bits; a weight changed in place is packed again."""
    cfg, _, shared = _net("TWOHEAD")
    model = _build(cfg).to(DEV)
    model.load_state_dict(shared.state_dict())
    tokens, lens, durations, want, _ = _given("twohead ragged")
    inputs = _inputs(tokens, lens, durations=durations)
    own = model.inference(inputs)
    again = model.inference(inputs)
    exact, _ = _run(model, inputs, frames=max(want["frames"]))
    for key in ("mel_outputs", "alignments", "gate_outputs", "log_durations", "pitch_pred", "energy_pred", "durations"):
        assert torch.equal(own[key], exact[key]) and torch.equal(own[key], again[key]), key
    B, L = tokens.shape
    short = torch.empty(max(model.workspace_bytes(B, L), model.workspace_bytes(B, max(want["frames"]))) - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        model._run(inputs, workspace=short)
    blob = model._blob
    with torch.no_grad():
        model.proj.bias += 1.0
    moved = model.inference(inputs)
    assert model._blob is not blob
    t = want["frames"][0]
    assert torch.allclose(moved["mel_outputs"][0, :, :t], own["mel_outputs"][0, :, :t] + 1.0, atol=1e-5) and not moved["mel_outputs"][1, :, want["frames"][1]:].any()


def test_stage_timing_gives_four_durations():
    _, _, model = _net("NARROW")
    model.enable_stage_timing(True)
    try:
        model.inference(_inputs(R.case_tokens("narrow 2 x 5"), None))
        times = model.stage_times_ms()
    finally:
        model.enable_stage_timing(False)
    assert len(times) == 4 and all(t >= 0.0 for t in times)
