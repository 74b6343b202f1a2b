"""GPU: the evaluation metrics (gvx_alignment_stats, gvx_mel_project, gvx_dtw_distance) against the float64 restatement of
tests/metrics_ref64.py - integers exactly, every cell of the accumulated-cost table under a bound counted from the roundings on a
path - and the entry points over them: Tacotron2.eval_synthesis, Synthesizer diagnostics, the optimizer's state dict."""
import math

import numpy as np
import pytest
import torch

from genvox_amd import _lib, metrics, weights as gw
from genvox_amd.tacotron2 import Tacotron2
from tests import metrics_ref64 as ref
from tests.golden.cases import AR_CASES, TRAIN_CASE, case_configs
from tests.test_tts_batch_gpu import TEXTS, syn  # noqa: F401  (the module-scoped Synthesizer fixture of the tts_batch tests)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of fp32
DEV = "cuda:0"
INT_KEYS = ("positions", "durations", "monotonic", "max_jump", "covered", "first_pos", "last_pos")


# ---- alignment statistics ---------------------------------------------------------------------------------------------------

def check_alignment(a, mel_lengths, token_lengths):
    """a: float32 numpy [B, T, L]; the lengths: lists or None.  Integers and peaks exactly; focus under its rounding bound."""
    B, T, L = a.shape
    ml = None if mel_lengths is None else torch.tensor(mel_lengths, dtype=torch.int32)
    tl = None if token_lengths is None else torch.tensor(token_lengths, dtype=torch.int64)   # any integer dtype is taken
    got = {k: v.cpu().numpy() for k, v in metrics.alignment_stats(torch.from_numpy(a).to(DEV), ml, tl).items()}
    want = ref.alignment_stats(a, mel_lengths, token_lengths)
    for k in INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (k, T, L)
    assert np.array_equal(got["peaks"], want["peaks"].astype(np.float32), equal_nan=True), (T, L)
    for b in range(B):
        Tb = T if mel_lengths is None else max(0, min(mel_lengths[b], T))
        if not math.isfinite(want["focus"][b]):   # no frames or tokens, a frame of NaNs, infinite peaks: the same non-number
            assert np.array_equal(got["focus"][b], np.float32(want["focus"][b]), equal_nan=True), (b, T, L)
            continue
        # the sum: at most ceil(Tb / 256) - 1 additions in a thread and 8 levels of the pairwise tree; then one division
        bound = (math.ceil(Tb / 256) + 8 + 1) * U * np.abs(want["peaks"][b, :Tb]).sum() / Tb
        assert abs(float(got["focus"][b]) - want["focus"][b]) <= bound, (b, T, L)
        assert abs(got["monotonic_fraction"][b] - want["monotonic_fraction"][b]) <= 2 * U
        assert abs(got["coverage"][b] - want["coverage"][b]) <= 2 * U
    return got


def ragged(n, B, rng):
    """B lengths in [0, n]: n itself, 0 and 1 where they fit, the rest random; one above n and one below 0 to be clamped."""
    lens = [n, 0, 1, n + 3, -2] + [int(rng.integers(0, n + 1)) for _ in range(B)]
    return lens[:B]


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 128, 129, 256, 300])
def test_alignment_stats_equal_the_restatement_at_every_wave_edge(L):
    rng = np.random.default_rng(L)
    for T in (1, 2, 255, 256, 257, 1000):
        B = 7
        soft = torch.softmax(torch.from_numpy(rng.standard_normal((3, T, L)).astype(np.float32)) * 4.0, dim=-1).numpy()   # real softmax rows
        levels = (rng.integers(0, 4, (3, T, L)) / 4.0).astype(np.float32)          # planted ties: four values, many maxima per frame
        levels[1, :, L - 1] = 1.0                                                   # ... a row whose maximum sits on the last token
        wild = rng.standard_normal((1, T, L)).astype(np.float32) * 1e30            # negative maxima, huge values, infinities
        wild[0, ::3, ::5] = -np.inf
        wild[0, 1::7, L // 2] = np.inf
        a = np.concatenate([soft, levels, wild])
        mel_lengths, token_lengths = ragged(T, B, rng), ragged(L, B, rng)[::-1]
        for b in range(B):   # NaN poison behind both lengths
            a[b, max(0, min(mel_lengths[b], T)):] = np.nan
            a[b, :, max(0, min(token_lengths[b], L)):] = np.nan
        check_alignment(a, mel_lengths, token_lengths)
        if T in (2, 257):
            check_alignment(np.concatenate([soft, levels]), None, None)


def test_alignment_frame_of_nans_is_passed_over_as_the_header_says():
    rng = np.random.default_rng(5)
    a = torch.softmax(torch.from_numpy(rng.standard_normal((2, 70, 90)).astype(np.float32)), dim=-1).numpy()
    a[0, 10] = np.nan                  # a frame of nothing but NaNs: pos 0, peak NaN, so focus NaN; the integers stay defined
    a[1, 20, ::2] = np.nan             # NaNs among numbers are passed over
    a[1, 21, :89] = np.nan
    got = check_alignment(a, None, None)
    assert got["positions"][0, 10] == 0 and math.isnan(got["peaks"][0, 10]) and math.isnan(got["focus"][0])
    assert got["positions"][1, 20] % 2 == 1 and got["positions"][1, 21] == 89 and math.isfinite(got["focus"][1])


def test_alignment_stats_many_tokens_and_same_bits_every_run():
    rng = np.random.default_rng(6)
    a = rng.random((2, 300, 5000)).astype(np.float32)    # more tokens than one pass of the frames-per-token table holds
    check_alignment(a, [300, 123], [5000, 4097])
    x = torch.from_numpy(rng.random((32, 1000, 128)).astype(np.float32)).to(DEV)
    one, two = metrics.alignment_stats(x), metrics.alignment_stats(x)
    for k in one:
        assert torch.equal(one[k], two[k]), k


# ---- the projection -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,T", [(80, 13, 1000), (80, 79, 65), (12, 1, 1), (128, 128, 130), (80, 80, 63)])
def test_projection_against_float64(M, K, T):
    rng = np.random.default_rng(M + K)
    mel = (rng.standard_normal((3, M, T)) * 3.0 - 4.0).astype(np.float32)
    P = rng.standard_normal((K, M)).astype(np.float32) if K == M or K == 128 else metrics.dct_rows(M, K).astype(np.float32)
    got = metrics.project(torch.from_numpy(mel).to(DEV), torch.from_numpy(P)).cpu().numpy()
    assert got.shape == (3, T, K)
    want = ref.project(mel, P)
    bound = (M + 1) * U * ref.project(np.abs(mel), np.abs(P))     # M fused multiply-adds, each one rounding
    assert np.all(np.abs(got - want) <= bound)
    if (M, K) == (80, 13):
        assert torch.equal(metrics.mel_cepstra(torch.from_numpy(mel).to(DEV)), torch.from_numpy(got).to(DEV))


# ---- the warp -------------------------------------------------------------------------------------------------------------------

def features(rng, B, T, K):
    """Smooth sequences with jumps, like cepstra of speech: neighbouring frames are close, so branches of the warp compete."""
    walk = np.cumsum(rng.standard_normal((B, T, K)) * 0.3, axis=1) + rng.standard_normal((B, 1, K))
    return walk.astype(np.float32)


def cell_bound(Tp, Tg, K):
    """Relative bound of an accumulated cost: a path has at most Tp + Tg - 1 cells, so as many additions; every d carries the
    roundings of its difference, its K fused multiply-adds and its square root (K + 4 is generous: the root halves them)."""
    return (Tp + Tg + K + 4) * U


def check_dtw(cp, cg, pred_lengths, target_lengths, every_cell=True):
    B, Tp_max, K = cp.shape
    Tg_max = cg.shape[1]
    pl = None if pred_lengths is None else torch.tensor(pred_lengths, dtype=torch.int32)
    tl = None if target_lengths is None else torch.tensor(target_lengths, dtype=torch.int32)
    x, y = torch.from_numpy(cp).to(DEV), torch.from_numpy(cg).to(DEV)
    dist = metrics.dtw_distance(x, y, pl, tl)
    if every_cell:
        # the table is written inside each row's rectangle only: pre-filled through the allocator's reuse it may hold anything
        dist2, acc = metrics.dtw_distance(x, y, pl, tl, return_accumulated=True)
        assert torch.equal(dist, dist2) or (torch.isnan(dist) == torch.isnan(dist2)).all() and torch.equal(dist.nan_to_num(), dist2.nan_to_num())
        acc = acc.cpu().numpy()
    dist = dist.cpu().numpy()
    for b in range(B):
        p = Tp_max if pred_lengths is None else max(0, min(pred_lengths[b], Tp_max))
        g = Tg_max if target_lengths is None else max(0, min(target_lengths[b], Tg_max))
        if p == 0 or g == 0:
            assert math.isnan(dist[b]), (b, p, g)
            continue
        A = ref.dtw_accumulated(cp[b, :p], cg[b, :g])
        bound = cell_bound(p, g, K)
        if every_cell:
            err = np.abs(acc[b, :p, :g] - A)
            assert np.all(err <= bound * A + 1e-45), (b, p, g, K, float((err / np.maximum(A, 1e-30)).max()), bound)
        want = A[-1, -1] / (p + g)
        assert abs(dist[b] - want) <= (bound + U) * want, (b, p, g, K)
    return dist


SIZES = (1, 2, 7, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("K", [1, 13, 80])
def test_dtw_every_cell_of_a_ragged_batch_of_all_size_pairs(K):
    """One call, 81 rows: every (Tp, Tg) of SIZES squared as a row of its own lengths, NaN behind them."""
    rng = np.random.default_rng(K)
    pairs = [(p, g) for p in SIZES for g in SIZES]
    cp, cg = features(rng, len(pairs), 257, K), features(rng, len(pairs), 257, K)
    for b, (p, g) in enumerate(pairs):
        cp[b, p:] = np.nan
        cg[b, g:] = np.nan
    assert _lib.load().gvx_dtw_uses_lds_tables(257, 257, K) == (0 if K == 80 else 1)   # 80 features: also the form without LDS tables
    check_dtw(cp, cg, [p for p, _ in pairs], [g for _, g in pairs])


@pytest.mark.parametrize("Tp,Tg,K", [(1, 1, 13), (2, 7, 1), (65, 64, 13), (257, 255, 13), (300, 37, 13), (37, 300, 13), (64, 257, 80)])
def test_dtw_every_cell_of_full_rows(Tp, Tg, K):
    rng = np.random.default_rng(Tp * 1000 + Tg)
    check_dtw(features(rng, 2, Tp, K), features(rng, 2, Tg, K), None, None)


def test_dtw_long_rows_and_a_ragged_batch_of_32():
    rng = np.random.default_rng(7)
    check_dtw(features(rng, 1, 1000, 13), features(rng, 1, 1000, 13), None, None, every_cell=False)
    check_dtw(features(rng, 1, 1000, 13), features(rng, 1, 37, 13), None, None, every_cell=False)
    B = 32
    pl = [300, 0, 1, 305, -1] + [int(rng.integers(1, 301)) for _ in range(B - 5)]
    tl = [int(rng.integers(1, 281)) for _ in range(B - 2)] + [0, 280]
    cp, cg = features(rng, B, 300, 13), features(rng, B, 280, 13)
    for b in range(B):
        cp[b, max(0, min(pl[b], 300)):] = np.nan
        cg[b, max(0, min(tl[b], 280)):] = np.nan
    d = check_dtw(cp, cg, pl, tl, every_cell=False)
    assert math.isnan(d[1]) and math.isnan(d[4]) and math.isnan(d[30]) and np.isfinite(d[[0, 2, 3, 31]]).all()


def test_dtw_form_that_does_not_fit_the_lds():
    """600 x 500 frames of 80 features: the feature tables are read through the cache and the diagonals live in the workspace."""
    lib = _lib.load()
    assert lib.gvx_dtw_uses_lds_tables(600, 500, 80) == 0 and lib.gvx_dtw_workspace_bytes(3, 600, 500, 80) >= 3 * 3 * 600 * 4
    rng = np.random.default_rng(8)
    cp, cg = features(rng, 3, 600, 80), features(rng, 3, 500, 80)
    cp[1, 411:], cg[1, 77:], cp[2, 1:] = np.nan, np.nan, np.nan
    check_dtw(cp, cg, [600, 411, 1], [500, 77, 500])


def test_dtw_same_bits_every_run_with_and_without_the_table():
    rng = np.random.default_rng(9)
    x, y = torch.from_numpy(features(rng, 8, 400, 13)).to(DEV), torch.from_numpy(features(rng, 8, 350, 13)).to(DEV)
    one = metrics.dtw_distance(x, y)
    two, acc = metrics.dtw_distance(x, y, return_accumulated=True)
    three = metrics.dtw_distance(x, y)
    assert torch.equal(one, two) and torch.equal(one, three) and torch.isfinite(one).all()
    assert torch.equal(acc[:, -1, -1] / 750.0, one)
    same = metrics.dtw_distance(x, x)
    assert torch.equal(same, torch.zeros_like(same))
    doubled = metrics.dtw_distance(x, x.repeat_interleave(2, dim=1))
    assert torch.equal(doubled, torch.zeros_like(doubled))          # a sequence against its own frame-doubled copy
    assert torch.equal(metrics.dtw_distance(y, x), one)              # symmetric: the same sums in the same order


def test_dtw_mel_distance_end_to_end_against_float64():
    rng = np.random.default_rng(10)
    M, K, B = 80, 13, 4
    mel_p = (np.cumsum(rng.standard_normal((B, M, 210)) * 0.2, axis=2) - 3.0).astype(np.float32)
    mel_g = (np.cumsum(rng.standard_normal((B, M, 190)) * 0.2, axis=2) - 3.0).astype(np.float32)
    pl, tl = [210, 150, 33, 1], [190, 190, 61, 5]
    got = metrics.dtw_mel_distance(torch.from_numpy(mel_p).to(DEV), torch.from_numpy(mel_g).to(DEV), torch.tensor(pl), torch.tensor(tl))
    P = ref.dct_rows(M, K)
    P32 = metrics.dct_rows(M, K).astype(np.float32)
    want = ref.dtw_distance(ref.project(mel_p, P), ref.project(mel_g, P), pl, tl)
    # a feature is off by the table's rounding to fp32 and its M fused multiply-adds; a frame distance by at most the norms of
    # both frames' errors; an accumulated cost by that on each of its at most Tp + Tg cells, twice where a cell counts twice
    e = ((M + 2) * U * max(ref.project(np.abs(mel_p), np.abs(P32)).max(), ref.project(np.abs(mel_g), np.abs(P32)).max()))
    for b in range(B):
        bound = cell_bound(pl[b], tl[b], K) * want[b] + 2.0 * (2.0 * math.sqrt(K) * e)
        assert abs(float(got[b]) - want[b]) <= bound, (b, float(got[b]), want[b], bound)

    class Log10:
        log_func = "np.log10"
    assert np.allclose(metrics.mcd_db(got, Log10).cpu().numpy(), ref.mcd_db(got.cpu().numpy(), True), rtol=1e-6)


# ---- Tacotron2.eval_synthesis ------------------------------------------------------------------------------------------------

def small_model(case=AR_CASES["ar_small_gate"]):
    mc, ac, tc = case_configs(case)
    sd = gw.generate_state_dict(mc, ac, tc, seed=case["weight_seed"], peaky_attention=True)
    m = Tacotron2(mc, ac, tc)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), (mc, ac, tc)


def synthesis_batch(B, L, T, mc, ac, tc, seed):
    tl = sorted([L] + [int(v) for v in np.random.default_rng(seed).integers(1, L + 1, B - 1)], reverse=True)
    ml = [T] + [int(v) for v in np.random.default_rng(seed + 1).integers(1, T + 1, B - 1)]
    inp = gw.synthetic_inputs(B, L, T, tc.n_tokens, ac.n_mels, seed=seed, token_lengths=tl, mel_lengths=ml)
    batch = {k: torch.from_numpy(v) for k, v in inp.items()}
    masks = torch.from_numpy(gw.prenet_keep_masks(mc.max_decoder_steps * B, mc.prenet_dim, seed=seed)).reshape(2, mc.max_decoder_steps, B, mc.prenet_dim)
    return batch, masks


@pytest.mark.parametrize("B", [1, 5, 33])
def test_eval_synthesis_numbers_are_the_restatement_on_its_own_inference_outputs(B):
    m, (mc, ac, tc) = small_model()
    L, T, S = 9, 20, mc.max_decoder_steps
    batch, masks = synthesis_batch(B, L, T, mc, ac, tc, seed=40 + B)
    tf = {**batch, "prenet_keep_masks": torch.from_numpy(gw.prenet_keep_masks((T + 1) * B, mc.prenet_dim))}
    m.eval_step(tf)
    before = dict(m.loss_items_eval)
    out = m.eval_synthesis(batch, prenet_keep_masks=masks)
    logs = m.get_synthesis_logs()
    assert set(logs) == {"mcd_dtw_eval", "align_focus_eval", "align_monotonic_eval", "align_coverage_eval", "stopped_fraction_eval", "frame_ratio_eval"}
    assert m.loss_items_eval == before                       # the teacher-forced items are not touched
    m.eval_step(tf)
    assert m.loss_items_eval == before and m.get_eval_priority() == before["loss_eval"] == m.get_eval_priority("loss")
    assert m.get_eval_priority("mcd_dtw") == logs["mcd_dtw_eval"]
    with pytest.raises(ValueError):
        m.get_eval_priority("bleu")
    frames = out["mel_lengths"].cpu().numpy()
    assert frames.shape == (B,) and frames.min() >= 1 and frames.max() == out["alignments"].shape[1] <= S
    tok_len, tgt_len = batch["token_lengths"].tolist(), batch["mel_lengths"].tolist()
    want = ref.alignment_stats(out["alignments"].cpu().numpy(), frames, tok_len)
    st = {k: v.cpu().numpy() for k, v in out["alignment_stats"].items()}
    for k in INT_KEYS:
        assert np.array_equal(st[k], want[k]), k
    assert np.allclose(st["focus"], want["focus"], rtol=1e-6, atol=0)
    P = ref.dct_rows(ac.n_mels, 13)
    post = out["mel_outputs_postnet"].cpu().numpy()
    dist = ref.dtw_distance(ref.project(post, P), ref.project(batch["mel_padded"].numpy(), P), frames, tgt_len)
    got_dist = out["dtw_distance"].cpu().numpy()
    assert np.isfinite(got_dist).all() and np.allclose(got_dist, dist, rtol=1e-4, atol=1e-5)   # (held to its rounding bound in the kernel tests)
    mcd = out["mcd_dtw"].cpu().numpy()
    assert np.allclose(mcd, ref.mcd_db(got_dist, ac.log_func == "np.log10"), rtol=1e-6)
    stopped = out["stopped"].cpu().numpy()
    assert np.array_equal(stopped, frames < S)
    ratio = out["frame_ratio"].cpu().numpy()
    assert np.allclose(ratio, frames / np.asarray(tgt_len, np.float64), rtol=1e-6)
    means = {"mcd_dtw_eval": mcd, "align_focus_eval": st["focus"], "align_monotonic_eval": st["monotonic_fraction"],
             "align_coverage_eval": st["coverage"], "stopped_fraction_eval": stopped.astype(np.float64), "frame_ratio_eval": ratio}
    for k, rows in means.items():
        assert abs(logs[k] - float(np.mean(rows.astype(np.float64)))) <= 1e-5 * max(1.0, abs(logs[k])), k


# ---- Synthesizer diagnostics ---------------------------------------------------------------------------------------------------

def test_tts_batch_diagnostics_add_keys_and_change_nothing_else(syn):  # noqa: F811
    syn.tts_model.model_config.gate_threshold = 1.0
    S = syn.tts_model.model_config.max_decoder_steps
    for texts in (TEXTS, TEXTS[3:4]):
        torch.manual_seed(23)
        plain = syn.tts_batch(texts)
        torch.manual_seed(23)
        diag = syn.tts_batch(texts, diagnostics=True)
        for p, d in zip(plain, diag):
            assert set(d) == set(p) | {"alignment_stats", "stopped"}
            for k in p:
                if k == "sampling_rate":
                    assert d[k] == p[k]
                else:
                    assert d[k].dtype == p[k].dtype and np.array_equal(d[k], p[k]), k
            a = d["alignments"]
            want = ref.alignment_stats(a[None])
            s = d["alignment_stats"]
            assert set(s) == {"focus", "monotonic_fraction", "max_jump", "coverage", "first_pos", "last_pos"}
            assert all(isinstance(s[k], int) for k in ("max_jump", "first_pos", "last_pos")) and isinstance(s["focus"], float)
            assert (s["max_jump"], s["first_pos"], s["last_pos"]) == (want["max_jump"][0], want["first_pos"][0], want["last_pos"][0])
            assert abs(s["focus"] - want["focus"][0]) <= 1e-6 and abs(s["coverage"] - want["coverage"][0]) <= 1e-6
            assert abs(s["monotonic_fraction"] - want["monotonic_fraction"][0]) <= 1e-6
            assert d["stopped"] is (a.shape[0] < S)
    torch.manual_seed(23)
    one = syn.tts(TEXTS[3])
    torch.manual_seed(23)
    one_d = syn.tts(TEXTS[3], diagnostics=True)
    assert set(one_d) == set(one) | {"alignment_stats", "stopped"}
    for k in one:
        assert np.array_equal(one_d[k], one[k]), k
    assert one_d["alignment_stats"] == diag[0]["alignment_stats"] and one_d["stopped"] == diag[0]["stopped"]


# ---- the optimizer's state dict ------------------------------------------------------------------------------------------------

def _grads(m, seed):
    g = torch.Generator().manual_seed(seed)
    return {name: torch.randn(p.shape, generator=g).to(DEV) for name, p in m.named_parameters()}


def test_adam_resumes_bit_for_bit_from_its_state_dict(tmp_path):
    a, _ = small_model(TRAIN_CASE)
    b, _ = small_model(TRAIN_CASE)
    opt_a, opt_b = a.get_optimizer(), b.get_optimizer()
    assert opt_a["optimizer"].state_dict()["state"] == {}
    for step in range(4):
        opt_a["optimizer"].step(_grads(a, step), 0.5)
    for step in range(2):
        opt_b["optimizer"].step(_grads(b, step), 0.5)
    path = str(tmp_path / "checkpoint.pt")
    torch.save(b.get_checkpoint_statedicts(opt_b), path)          # through a file, as a trainer would
    c, _ = small_model(AR_CASES["ar_small_gate"])                # other weights, a fresh optimizer
    opt_c = c.get_optimizer()
    c.load_checkpoint_statedicts(torch.load(path, map_location="cpu"), save_optimizer_dict=True, optimizer=opt_c)
    assert opt_c["optimizer"].step_count == 2
    for (name, p), (_, q) in zip(b.named_parameters(), c.named_parameters()):
        assert torch.equal(p, q), name
        for i in (0, 1):
            assert torch.equal(opt_b["optimizer"].state[name][i], opt_c["optimizer"].state[name][i]), name
            assert opt_c["optimizer"].state[name][i].device == q.device
    for step in range(2, 4):
        opt_c["optimizer"].step(_grads(c, step), 0.5)
    sd_a, sd_c = opt_a["optimizer"].state_dict(), opt_c["optimizer"].state_dict()
    assert sd_a["param_groups"] == sd_c["param_groups"] and list(sd_a["state"]) == list(sd_c["state"])
    for (name, p), (_, q) in zip(a.named_parameters(), c.named_parameters()):
        assert torch.equal(p, q), name                            # four uninterrupted steps == two, save, load, two
    for i in sd_a["state"]:
        assert float(sd_c["state"][i]["step"]) == 4.0
        assert torch.equal(sd_a["state"][i]["exp_avg"], sd_c["state"][i]["exp_avg"])
        assert torch.equal(sd_a["state"][i]["exp_avg_sq"], sd_c["state"][i]["exp_avg_sq"])
    theirs = torch.optim.Adam(c.parameters(), lr=1.0)
    theirs.load_state_dict(sd_c)                                  # and the reference's optimizer takes it
    assert theirs.state_dict()["param_groups"][0]["lr"] == c.model_config.learning_rate
