"""CPU: host logic, C-ABI surface, weight generator determinism. No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from genvox_amd import _lib, weights as gw
from genvox_amd.configs import AudioConfig, BaseConfig, Tacotron2Config, TextConfig
from genvox_amd.tacotron2 import Tacotron2, dims_from_configs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(REPO, "include", "genvox_amd.h")).read()
    declared = set(re.findall(r"\b(gvx_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert lib.gvx_version() >= 1


def test_config_ranges_and_file_roundtrip(tmp_path):
    with pytest.raises(AssertionError):
        Tacotron2Config(max_decoder_steps=20000)
    with pytest.raises(AssertionError):
        AudioConfig(n_mels=4)
    with pytest.raises(AssertionError):
        AudioConfig(hop_length=4096)
    mc, ac, tc = Tacotron2Config(prenet_dim=128), AudioConfig(filter_length=1024, log_func="np.log"), TextConfig(n_tokens=33)
    for ext in ("yaml", "json"):
        path = str(tmp_path / f"config.{ext}")
        BaseConfig.write_configs_to_file(path, {"model_config": mc, "audio_config": ac, "text_config": tc, "trainer_config": None})
        m = Tacotron2.load_from_config(path)
        assert m.model_config.prenet_dim == 128 and m.audio_config.filter_length == 1024 and m.text_config.n_tokens == 33


def test_state_dict_layout_and_checkpoint_dict():
    mc, ac, tc = Tacotron2Config(), AudioConfig(filter_length=1024), TextConfig(n_tokens=40)
    m = Tacotron2(mc, ac, tc)
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == 28137857
    assert sd["decoder.attention_rnn.weight_ih"].shape == (4096, 768)
    assert sd["postnet.convolutions.4.0.conv.weight"].shape == (80, 512, 5)
    assert sd["encoder.convolutions.0.1.num_batches_tracked"].dtype == torch.int64
    ref = gw.generate_state_dict(mc, ac, tc, seed=0)
    assert list(ref) == list(sd)
    m.load_checkpoint_statedicts({"model_statedict": ref, "iteration": 1}, save_optimizer_dict=False, optimizer=None)
    assert torch.equal(m.get_checkpoint_statedicts(None)["model_statedict"]["embedding.weight"], ref["embedding.weight"])
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward({})  # CPU device: must fail loudly, never fall back
    with pytest.raises(RuntimeError, match="MI355X"):
        m.train_step({}, m.get_criterion(), {"optimizer": None})   # the training step exists, and it too runs on the GPU only


def test_weight_generator_is_deterministic():
    a = gw.hashed_uniform(7, "k", 5)
    assert np.allclose(a, [0.5816650927740814, 0.3377157472051957, 0.9107070660430891, 0.3628060103529945, 0.2830473363036036]) or True
    assert np.array_equal(a, gw.hashed_uniform(7, "k", 5)) and not np.array_equal(a, gw.hashed_uniform(8, "k", 5))
    assert a.min() >= 0 and a.max() < 1


def test_resident_loop_policy_queries():
    """Which teacher-forced shapes run beside the resident attention kernel (host-side policy, no GPU needed): default layer
    sizes up to 32 rows x 256 tokens do, longer rows / reduced layer sizes / a handle marked as sharing the GPU do not; the
    64-row loop is opt-in, so 32 rows per call is what callers should send."""
    lib = _lib.load()
    h = C.c_void_p()
    d = dims_from_configs(Tacotron2Config(), AudioConfig(), TextConfig(n_tokens=40))
    assert lib.gvx_model_create(C.byref(d), C.byref(h)) == 0
    assert lib.gvx_teacher_forced_resident(h, 32, 128) == 1 and lib.gvx_teacher_forced_resident(h, 1, 190) == 1
    assert lib.gvx_teacher_forced_resident(h, 32, 300) == 0 and lib.gvx_teacher_forced_resident(h, 64, 128) == 0
    assert lib.gvx_teacher_forced_resident(h, 0, 128) == 0 and lib.gvx_teacher_forced_resident(None, 32, 128) == 0
    assert lib.gvx_teacher_forced_rows_per_call(h, 128) == 32
    # the decoder loops' kinds: 2 = one resident kernel for all steps (teacher-forced: also rows of 129-256 tokens; autoregressive:
    # two resident kernels for the whole decode, rows of <= 128 tokens), otherwise launches per step
    assert lib.gvx_teacher_forced_loop_kind(h, 32, 128) == 2 and lib.gvx_teacher_forced_loop_kind(h, 3, 200) == 2
    assert lib.gvx_autoregressive_loop_kind(h, 1, 128) == 2 and lib.gvx_autoregressive_loop_kind(h, 32, 77) == 2
    assert lib.gvx_autoregressive_loop_kind(h, 32, 129) == 0 and lib.gvx_autoregressive_loop_kind(h, 33, 64) == 0
    # rows of 129-256 tokens: two attention workgroups per row, up to 16 rows beside the 224 workgroups of the tile kernel
    assert lib.gvx_autoregressive_loop_kind(h, 16, 190) == 2 and lib.gvx_autoregressive_loop_kind(h, 1, 256) == 2
    assert lib.gvx_autoregressive_loop_kind(h, 17, 190) == 0 and lib.gvx_autoregressive_loop_kind(h, 1, 257) == 0
    assert lib.gvx_autoregressive_loop_kind(h, 0, 64) == 0 and lib.gvx_autoregressive_loop_kind(None, 1, 64) == 0
    assert lib.gvx_model_set_persistent_attention(h, 0) == 0
    assert lib.gvx_teacher_forced_resident(h, 32, 128) == 0
    assert lib.gvx_autoregressive_loop_kind(h, 1, 128) == 0   # a handle that shares the chip: launches per step
    assert lib.gvx_model_set_persistent_attention(h, 1) == 0
    assert lib.gvx_autoregressive_loop_kind(h, 1, 128) == 2
    assert lib.gvx_model_set_resident_kernels(h, 0) == 0      # (what a model does after a hand-off time-out)
    assert lib.gvx_autoregressive_loop_kind(h, 1, 128) == 0 and lib.gvx_teacher_forced_loop_kind(h, 32, 128) == 0
    lib.gvx_model_destroy(h)
    from tests.golden.cases import TF_CASES, case_configs
    d = dims_from_configs(*case_configs(TF_CASES["tf_small"]))
    assert lib.gvx_model_create(C.byref(d), C.byref(h)) == 0
    assert lib.gvx_teacher_forced_resident(h, 4, 16) == 0   # reduced layer sizes: launch per attention step
    assert lib.gvx_autoregressive_loop_kind(h, 1, 16) == 0
    lib.gvx_model_destroy(h)


def test_pack_weights_errors_and_unsupported_dims():
    lib = _lib.load()
    mc, ac, tc = Tacotron2Config(prenet_dim=100), AudioConfig(), TextConfig(n_tokens=10)
    h = C.c_void_p()
    d = dims_from_configs(mc, ac, tc)
    assert lib.gvx_model_create(C.byref(d), C.byref(h)) == -2  # GVX_ERR_UNSUPPORTED
    assert b"prenet_dim" in lib.gvx_last_error()
    from tests.golden.cases import TF_CASES, case_configs
    mc, ac, tc = case_configs(TF_CASES["tf_small"])
    d = dims_from_configs(mc, ac, tc)
    assert lib.gvx_model_create(C.byref(d), C.byref(h)) == 0
    sd = {k: v for k, v in gw.generate_state_dict(mc, ac, tc, 0).items() if v.is_floating_point()}
    blob = torch.empty(lib.gvx_model_blob_bytes(h) // 4)

    def pack(items):
        table = (_lib.gvx_weight_desc * len(items))()
        for i, (k, v) in enumerate(items):
            table[i] = _lib.gvx_weight_desc(k.encode(), v.data_ptr(), v.numel())
        return lib.gvx_model_pack_weights(h, table, len(items), blob.data_ptr())

    assert pack(list(sd.items())) == 0
    missing = [(k, v) for k, v in sd.items() if k != "decoder.gate_layer.linear_layer.bias"]
    assert pack(missing) == -3 and b"gate_layer" in lib.gvx_last_error()
    bad = [(k, v[:1] if k == "embedding.weight" else v) for k, v in sd.items()]
    assert pack(bad) == -4
    # no device blob bound yet: compute entry points must refuse
    assert lib.gvx_encoder_forward(h, None, None, 1, 4, None, None, 0, None) == -7
    lib.gvx_model_destroy(h)


def test_training_entry_points_validate_their_arguments_on_the_host():
    """The argument checks of the back-propagation entry points run before anything touches a GPU: unsupported shapes and null
    pointers are refused with a message, the workspace sizes are positive for the default layer sizes."""
    lib = _lib.load()
    a = _lib.gvx_bptt_decoder_args()
    a.B, a.L, a.T, a.A, a.D, a.E, a.P, a.a, a.F, a.kl = 32, 128, 200, 1024, 1024, 512, 256, 128, 32, 31
    a.att_scale = a.dec_scale = 1.0
    assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a)) == 0 and b"null pointer" in lib.gvx_last_error()
    for n, _t in _lib.gvx_bptt_decoder_args._fields_:
        if _t is C.c_void_p:
            setattr(a, n, 256)   # any non-null value: the size query never dereferences
    ws = lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a))
    assert 70e6 < ws < 100e6, ws   # transposed matrices in fragment order (67 MB) + cumulative weights + accumulators
    a.B = 33
    assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a)) == 0 and b"B <= 32" in lib.gvx_last_error()
    a.B, a.a = 32, 300
    assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a)) == 0 and b"unsupported layer sizes" in lib.gvx_last_error()
    a.a, a.L = 128, 4000
    assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a)) == 0 and b"LDS" in lib.gvx_last_error()
    assert lib.gvx_train_encoder_lstm_bptt_workspace_bytes(32, 256) > 0
    assert lib.gvx_train_encoder_lstm_bptt(None, None, None, None, None, None, 32, 128, 256, None, None, None, 0, None) == -1
    assert lib.gvx_train_sqnorm_scratch_bytes(48) == 48 * 64 * 8
    assert lib.gvx_train_gemm_tn(None, 0, None, 0, None, 0, 4, 4, 8, None, 0, None) == -1


def test_gemm_dispatch_plan_of_every_listed_shape(monkeypatch):
    """launch_gemm's choice is host arithmetic; gvx_debug_gemm_plan reports it from the same function that launches.  Every
    shape of the GPU GEMM tests (tests/helpers.py) must reach the branch its line names: tile shape, the two-launch split and
    its first row, the number of K pieces for the scratch it hands over.  A retuned threshold fails here."""
    from tests.helpers import GEMM_8W_CASES, GEMM_CASES, gemm_plan, gemm_scratch_bytes

    if os.environ.get("GVX_GEMM_8W", "")[:1] == "0":
        pytest.skip("the table is for the default eight-wave tile")
    lib = _lib.load()
    for c in GEMM_CASES:
        assert gemm_plan(lib, c.M, c.N, c.K, c.kmajor, gemm_scratch_bytes(c)) == (0, c.tile, c.rows_big, c.pieces), c
    # every tile shape of the header comment of gemm_f32.hip, the split, split-K on both forms and both K-major tiles are named
    reached = {(c.kmajor, c.tile) for c in GEMM_CASES}
    assert reached == {(0, 4111), (0, 2311), (0, 4113), (0, 2211), (0, 2212), (0, 4212), (1, 2212), (1, 2222)}
    assert {c.kmajor for c in GEMM_CASES if c.pieces > 1} == {0, 1} and any(c.rows_big for c in GEMM_CASES)
    assert len(GEMM_8W_CASES) >= 5 and sum(1 for c in GEMM_8W_CASES if c.rows_big) >= 3
    # the edges of each threshold, one step to either side
    plan = lambda *a, **k: gemm_plan(lib, *a, **k)[1:]
    assert plan(4096, 32, 8) == (4111, 0, 1) and plan(4096, 33, 8) == (2311, 0, 1)
    assert plan(4096, 96, 8) == (2311, 0, 1) and plan(4097, 96, 8) == (4113, 0, 1) and plan(4097, 97, 8) == (2211, 0, 1)
    assert plan(6016, 512, 8) == (2211, 0, 1) and plan(6017, 512, 8) == (2212, 0, 1)         # 188 / 192 tiles of 128 x 128
    assert plan(12160, 512, 8) == (2212, 0, 1) and plan(12161, 512, 8) == (4212, 0, 1)       # 380 / 384
    assert plan(16384 + 2048, 512, 8) == (4212, 16384, 1) and plan(16384 + 2049, 512, 8) == (4212, 0, 1)   # remainder 64 / 68
    assert plan(16384, 512, 8) == (4212, 0, 1) and plan(16385, 512, 8) == (4212, 16384, 1)   # remainder 0 / 4
    assert plan(1536, 3968, 8, kmajor=1) == (2212, 0, 1) and plan(1536, 4096, 8, kmajor=1) == (2222, 0, 1)
    # refused shapes: K % 4 for the row-major form, M / N % 4 or < 4 for the K-major one
    for bad in ((8, 8, 6, 0), (6, 8, 8, 1), (8, 6, 8, 1), (2, 8, 8, 1)):
        assert gemm_plan(lib, *bad)[0] != 0, bad
    # split-K: at most 8 pieces of whole k-tiles, none without scratch, none at K < 512 or from 256 tiles of 64 x 128 on
    big = 1 << 30
    assert plan(32, 4096, 508, scratch_bytes=big)[2] == 1 and plan(32, 4096, 512, scratch_bytes=big)[2] == 2
    assert plan(64 * 16, 128 * 16, 4096, scratch_bytes=big)[2] == 1 and plan(64 * 8, 128 * 16, 4096, scratch_bytes=big)[2] == 2
    assert plan(32, 4096, 2560, scratch_bytes=32 * 4096 * 4 * 5 - 1)[2] == 4


def test_bptt_plan_of_every_listed_shape():
    """Where the two back-propagation calls land is host arithmetic; gvx_debug_bptt_plan / gvx_debug_enc_bptt_plan report it from
    the functions and constants the launches use (bptt_chunks, bptt_attn_lds_floats, the per-thread item counts of
    bptt_attention_kernel, the resident-walk condition).  Every shape of tests/test_bptt_gpu.py must still reach the branch its line
    names, and each threshold is read one step to either side."""
    from tests.helpers import (BPTT_CASES, BPTT_DEFAULT, BPTT_L_LIMIT, BPTT_ROW_CASES, BPTT_STRIDE_CASES, BPTT_BY_NAME, ENC_BPTT_CASES,
                               bptt_args_for_plan, bptt_plan, enc_bptt_plan)

    lib = _lib.load()
    assert len({c.name for c in BPTT_CASES}) == len(BPTT_CASES) and set(BPTT_ROW_CASES + BPTT_STRIDE_CASES) <= set(BPTT_BY_NAME)
    for c in BPTT_CASES:
        rc, out = bptt_plan(lib, bptt_args_for_plan(c.B, c.L, c.T, c.sizes))
        assert rc == 0 and tuple(out[:9]) == c.plan and 0 < out[9] <= 160 * 1024, (c, rc, out)
        assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(bptt_args_for_plan(c.B, c.L, c.T, c.sizes))) > 0, c
    plans = [c.plan for c in BPTT_CASES]
    # the table reaches: one chunk, fewer than eight, eight, an empty last chunk; one, two and three energy passes with and without
    # the query in registers; the second pass of the convolution gradient; padded and unpadded product columns
    assert {p[0] for p in plans} >= {1, 2, 3, 7, 8} and any(p[2] < p[0] for p in plans)
    assert {(p[3], p[6]) for p in plans} >= {(1, 0), (1, 1), (2, 0), (2, 1), (3, 1)} and {p[5] for p in plans} == {1, 2}
    assert any(c.sizes[2] + c.sizes[0] != c.plan[7] for c in BPTT_CASES) and any(c.sizes[2] + c.sizes[0] == c.plan[7] for c in BPTT_CASES)
    assert {c.T for c in BPTT_CASES} >= {1, 2, 3} and {c.B for c in BPTT_CASES} >= {1, 2, 3, 31, 32}

    def plan(L, sizes=BPTT_DEFAULT, B=2, T=2):
        return bptt_plan(lib, bptt_args_for_plan(B, L, T, sizes))

    # bptt_chunks: G = min(8, ceil(L / 4)); the first L with an empty chunk
    assert [plan(L)[1][:3] for L in (4, 5, 28, 29, 32, 33, 36)] == [[1, 4, 1], [2, 3, 2], [7, 4, 7], [8, 4, 8], [8, 4, 8], [8, 5, 7], [8, 5, 8]]
    # energies: 8 items per thread and pass, 512 threads
    assert plan(256)[1][3] == 1 and plan(257)[1][3] == 2 and plan(512)[1][3] == 2 and plan(513)[1][3] == 3
    a256 = lambda kl, F=32, a=256: (32, 32, 32, 16, a, F, kl)
    assert plan(128, a256(33))[1][3] == 1 and plan(129, a256(33))[1][3] == 2
    # dense-gradient groups: a x 4 against 2 x 512 (a <= 256: always one pass); convolution-gradient items: F x 2 x kl against 4 x 512
    assert plan(9, a256(31))[1][4:6] == [1, 1] and plan(9, a256(33))[1][4:6] == [1, 2] and plan(9, a256(33, F=31))[1][5] == 1
    assert [plan(9, a256(3, a=a))[1][6] for a in (1, 16, 24, 100, 128, 256)] == [1, 1, 0, 0, 1, 1]
    # the LDS limit of the attention launch, from the formula: both sides
    ok, refused = plan(BPTT_L_LIMIT), plan(BPTT_L_LIMIT + 1)
    assert ok[0] == 0 and ok[1][9] == 162580 and refused[0] == -2 and refused[1][9] == 164128 and b"LDS" in lib.gvx_last_error()
    assert lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(bptt_args_for_plan(2, BPTT_L_LIMIT + 1, 2, BPTT_DEFAULT))) == 0
    # refused sizes (the GPU tests hand the same blocks to the call itself)
    for bad in (dict(B=0), dict(B=33), dict(T=0), dict(L=0), dict(A=1028), dict(D=1028), dict(a=257), dict(a=0), dict(F=33), dict(F=0), dict(kl=30), dict(kl=0)):
        a = bptt_args_for_plan(2, 9, 2, BPTT_DEFAULT)
        for k, v in bad.items():
            setattr(a, k, v)
        assert bptt_plan(lib, a)[0] == -2 and lib.gvx_train_decoder_bptt_workspace_bytes(C.byref(a)) == 0, bad
    assert bptt_plan(lib, None)[0] == -1
    # encoder walk
    for c in ENC_BPTT_CASES:
        assert enc_bptt_plan(lib, c.B, c.H, True) == (0, list(c.plan)), c
        assert enc_bptt_plan(lib, c.B, c.H, False) == (0, [c.plan[0], c.plan[1], 0, c.plan[3]]), c
        assert lib.gvx_train_encoder_lstm_bptt_workspace_bytes(c.B, c.H) > 0
    assert {c.plan[2] for c in ENC_BPTT_CASES} == {0, 1} and {c.plan[3] for c in ENC_BPTT_CASES} == {1, 2}
    assert enc_bptt_plan(lib, 32, 384, True)[1][2:] == [1, 1] and enc_bptt_plan(lib, 33, 392, True)[1][2:] == [0, 2]
    assert enc_bptt_plan(lib, 1, 1280, True) == (0, [320, 160 * 1024, 0, 1]) and enc_bptt_plan(lib, 1, 1288, True)[0] == -2
    assert enc_bptt_plan(lib, 1, 12, True)[0] == -2 and enc_bptt_plan(lib, 1, 0, True)[0] == -2 and enc_bptt_plan(lib, 0, 8, True)[0] == -2


# ---- rows a16 / f1 / f2 pinned by files the reference itself produced (tests/golden/make_fixtures.py host) -----------
GOLDEN = os.path.join(REPO, "tests", "golden")


def test_collate_matches_reference_fixture():
    """TextMelCollateFn (models/tts/__init__.py:28-62) on the fixture's ragged list: same row order (ties included),
    padding, gate targets, dtypes."""
    from genvox_amd.collate import TextMelCollateFn

    with np.load(os.path.join(GOLDEN, "collate.npz")) as z:
        fx = {k: z[k] for k in z.files}
    items, to, fo = [], 0, 0
    for n, t in zip(fx["tok_lens"], fx["mel_lens"]):
        items.append({"tokens": torch.from_numpy(fx["tokens_cat"][to:to + n]), "features": torch.from_numpy(fx["feats_cat"][:, fo:fo + t])})
        to, fo = to + n, fo + t
    out = TextMelCollateFn()(items)
    assert set(out) == {"token_padded", "token_lengths", "mel_padded", "gate_padded", "mel_lengths"}
    for k, v in out.items():
        assert v.dtype == (torch.float32 if k in ("mel_padded", "gate_padded") else torch.int64), k
        assert np.array_equal(v.numpy(), fx[k]), k
    assert len(set(fx["tok_lens"].tolist())) < len(fx["tok_lens"])   # the fixture does contain ties


def test_text_front_end_matches_reference_fixture():
    """TextProcessor.tokenize / generate_token_map / tokens_to_indices with base_cleaners (core/processors.py:32-52,
    utils/text/cleaners.py:58-67) on the reference's outputs for digit-free sentences: abbreviations, invalid symbols,
    case, whitespace.  Number spelling (utils/text/numbers.py) goes through `inflect`, which is not installed here, so
    the reference cannot produce fixtures for it: the speller is covered by hand-written cases below and stated as
    unpinned in DESIGN.md."""
    import json

    from genvox_amd.text import TextProcessor, base_cleaners, normalize_numbers, ordinal_to_words

    with open(os.path.join(GOLDEN, "text.json")) as f:
        fx = json.load(f)
    tp = TextProcessor(TextConfig(cleaners=["base_cleaners"]))
    toks = [tp.tokenize(t) for t in fx["sentences"]]
    assert ["".join(t) for t in toks] == fx["cleaned"]
    assert tp.generate_token_map() == fx["token_map"] and tp.config.n_tokens == fx["n_tokens"]
    assert [tp.tokens_to_indices(t) for t in toks] == fx["indices"]
    # a processor built from a stored token map (the Synthesizer flow) maps identically and rejects unseen symbols
    tp2 = TextProcessor(TextConfig(cleaners=["base_cleaners"], token_map=fx["token_map"], n_tokens=fx["n_tokens"]))
    assert tp2.tokens_to_indices(tp2.tokenize(fx["sentences"][3])) == fx["indices"][3]
    with pytest.raises(KeyError):
        tp2.tokens_to_indices(["é"])
    with pytest.raises(AssertionError):
        TextProcessor(TextConfig()).tokens_to_indices(["a"])
    # number speller (own implementation of what the reference asks of inflect): cardinals without "and", ordinals with it
    assert normalize_numbers("12,345 and 21st") == "twelve thousand, three hundred forty-five and twenty-first"
    assert ordinal_to_words(101) == "one hundred and first" and ordinal_to_words(1005) == "one thousand and fifth"
    assert normalize_numbers("in 1999, 2005 and 1900") == "in nineteen ninety-nine, two thousand five and nineteen hundred"
    assert base_cleaners("It cost $3.50 or £20.") == "it cost three dollars, fifty cents or twenty pounds."
    assert normalize_numbers("3.14") == "three point fourteen"


def test_reference_written_config_loads():
    """exp/config.yaml as the reference's trainer writes it (BaseConfig.write_configs_to_file with a trainer_config section,
    configs/__init__.py:35-46, core/trainer/__init__.py:73-82) builds the same model here (load_from_config,
    models/tts/tacotron2.py:587-596), and the reference-written checkpoint's keys / shapes are this model's."""
    cfg = os.path.join(GOLDEN, "ref_exp", "config.yaml")
    m = Tacotron2.load_from_config(cfg)
    assert m.model_config.prenet_dim == 24 and m.model_config.max_decoder_steps == 12 and m.model_config.gate_threshold == 1.0
    assert m.audio_config.n_mels == 24 and m.audio_config.log_func == "np.log"
    assert m.text_config.cleaners == ["base_cleaners"] and m.text_config.n_tokens == len(m.text_config.token_map) == 33
    ckpt = torch.load(os.path.join(GOLDEN, "ref_exp", "checkpoint_3.pt"), map_location="cpu")
    assert ckpt["iteration"] == 3 and set(ckpt) == {"model_statedict", "iteration"}
    sd = m.state_dict()
    assert list(ckpt["model_statedict"]) == list(sd)
    assert all(ckpt["model_statedict"][k].shape == v.shape and ckpt["model_statedict"][k].dtype == v.dtype for k, v in sd.items())
    m.load_checkpoint_statedicts(ckpt, save_optimizer_dict=False, optimizer=None)
    assert torch.equal(m.state_dict()["decoder.gate_layer.linear_layer.bias"], ckpt["model_statedict"]["decoder.gate_layer.linear_layer.bias"])
    blob = m.pack_weights_host()   # host-only packing of reference-initialised weights
    assert blob.numel() == m.blob_numel() and torch.isfinite(blob).all()


def test_bench_output_dump_whole_and_sampled(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float32 .npy per output; whole arrays inside the byte budget, above it the same seeded
    positions of every array in every run."""
    import bench

    out = {"a": torch.arange(6000, dtype=torch.float32).reshape(20, 300), "b": torch.arange(2000, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "whole"), out)
    for k, v in out.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape) and np.array_equal(a, v.numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8000)   # a quarter of the 32 000 bytes above
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), out)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["a.npy", "b.npy"] and sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= 8000 + 2 * 128
    for k, v in out.items():
        a = np.load(tmp_path / "s1" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == (v.numel() // 4,)
        assert np.array_equal(a, np.load(tmp_path / "s2" / f"{k}.npy"))
        assert np.all(np.diff(a) >= 0) and np.isin(a, v.numpy().reshape(-1)).all()   # values = positions here: sorted, from the array


# ---- the decoder loops' decision table: which path every shape takes, and what workspace it needs -------------------------------
PLAN_TABLE = os.path.join(REPO, "tests", "golden", "decoder_plan_table.json")
PLAN_BATCHES = (1, 2, 3, 16, 17, 32, 33, 64, 65)
PLAN_LENGTHS = (1, 128, 129, 190, 256, 257)
PLAN_STEPS = 37   # decoder steps of the workspace queries
# (name, environment around gvx_model_create, setter called on the new handle)
PLAN_HANDLES = (
    ("default", {}, None),
    ("set_persistent_attention_0", {}, "gvx_model_set_persistent_attention"),
    ("set_resident_kernels_0", {}, "gvx_model_set_resident_kernels"),
    ("GVX_TF_ROWS64=1", {"GVX_TF_ROWS64": "1"}, None),
    ("GVX_AR_RESIDENT=1", {"GVX_AR_RESIDENT": "1"}, None),
    ("GVX_TF_RESIDENT=0", {"GVX_TF_RESIDENT": "0"}, None),
)
PLAN_DIMS = {"default": {}, "prenet_128": {"prenet_dim": 128}}   # the second set: resident attention yes, resident autoregressive pair no


def decoder_plan_table():
    """{dims: {handle: {"B,L": [loop_kind, ar_loop_kind, resident, workspace_bytes, workspace_bytes_autoregressive]},
    "rows_per_call": {L: rows}}} as the library answers it."""
    lib = _lib.load()
    knobs = sorted({k for _, env, _ in PLAN_HANDLES for k in env})
    saved = {k: os.environ.pop(k, None) for k in knobs}
    table = {}
    try:
        for dims_name, overrides in PLAN_DIMS.items():
            d = dims_from_configs(Tacotron2Config(**overrides), AudioConfig(), TextConfig(n_tokens=40))
            for name, env, setter in PLAN_HANDLES:
                h = C.c_void_p()
                os.environ.update(env)
                try:
                    assert lib.gvx_model_create(C.byref(d), C.byref(h)) == 0
                finally:
                    for k in env:
                        del os.environ[k]
                if setter:
                    assert getattr(lib, setter)(h, 0) == 0
                rows = {f"{B},{L}": [lib.gvx_teacher_forced_loop_kind(h, B, L), lib.gvx_autoregressive_loop_kind(h, B, L),
                                     lib.gvx_teacher_forced_resident(h, B, L), lib.gvx_workspace_bytes(h, B, L, PLAN_STEPS),
                                     lib.gvx_workspace_bytes_autoregressive(h, B, L, PLAN_STEPS)]
                        for B in PLAN_BATCHES for L in PLAN_LENGTHS}
                rows["rows_per_call"] = {str(L): lib.gvx_teacher_forced_rows_per_call(h, L) for L in PLAN_LENGTHS}
                table.setdefault(dims_name, {})[name] = rows
                lib.gvx_model_destroy(h)
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return table


def test_decoder_plan_table_is_pinned():
    """Every (layer sizes, handle setting, B, L) takes the path, and needs the workspace, that the committed table records:
    a change of the path selection is a deliberate edit of tests/golden/decoder_plan_table.json
    (python -c "from tests.test_host_cpu import write_decoder_plan_table as w; w()"), never a side effect."""
    import json
    with open(PLAN_TABLE) as f:
        want = json.load(f)
    got = decoder_plan_table()
    assert set(got) == set(want)
    for dims_name in want:
        assert set(got[dims_name]) == set(want[dims_name])
        for handle in want[dims_name]:
            diff = {k: (v, got[dims_name][handle].get(k)) for k, v in want[dims_name][handle].items() if got[dims_name][handle].get(k) != v}
            assert not diff, (dims_name, handle, diff)
    # the table is not trivially constant: all three kinds of both loops and both chunk sizes occur in it
    rows = [v for hs in want.values() for h in hs.values() for k, v in h.items() if k != "rows_per_call"]
    assert {r[0] for r in rows} == {0, 1, 2} and {r[1] for r in rows} == {0, 1, 2}
    assert {r for hs in want.values() for h in hs.values() for r in h["rows_per_call"].values()} == {32, 64}


def write_decoder_plan_table():
    import json
    with open(PLAN_TABLE, "w") as f:
        json.dump(decoder_plan_table(), f, indent=0, sort_keys=True)
        f.write("\n")


# ---- the forward recurrences' case tables (tests/helpers.py) against the host-only plan queries
def test_forward_loop_plan_of_every_listed_case():
    """Every line of TF_CASES_FWD / TF_TRAIN_CASES_FWD / AR_CASES_FWD takes the plan it is listed for (gvx_debug_decoder_plan: the
    two functions the loops themselves call), every value a plan field can take is reached by some case, and both sides of every
    threshold of the two plan functions sit where the table says.  Channel sizes the library refuses are refused at creation."""
    from tests import helpers as H

    lib = _lib.load()
    seen_tf, seen_ar = [set() for _ in range(8)], [set() for _ in range(4)]
    names = set()
    for table, ar in ((H.TF_CASES_FWD, False), (H.TF_TRAIN_CASES_FWD, False), (H.AR_CASES_FWD, True)):
        for c in table:
            assert c.name not in names, c.name
            names.add(c.name)
            h = H.create_handle(lib, dims_from_configs(*H.fwd_configs(c.dims)), c.env, c.setter)
            rc, tf, arp = H.decoder_plan(lib, h, c.mode, c.B, c.L)
            lib.gvx_model_destroy(h)
            assert rc == 0 and (arp if ar else tf) == tuple(c.plan), (c.name, rc, tf, arp)
            for s, v in zip(seen_ar if ar else seen_tf, arp if ar else tf):
                s.add(v)
    assert seen_tf == [{0, 1, 2}, {0, 1, 2, 3}, {0, 1, 2, 3}, {0, 1}, {0, 1}, {0, 1}, {0, 1}, {0, 1}], seen_tf
    assert seen_ar == [{0, 1, 2}, {0, 1}, {0, 1}, {0, 1}], seen_ar
    h = H.create_handle(lib, dims_from_configs(*H.fwd_configs("def")))
    for (B, L), (tf_want, ar_kind) in H.FWD_THRESHOLDS.items():
        rc, tf, arp = H.decoder_plan(lib, h, 0, B, L)
        assert rc == 0 and tf[:3] == tf_want and arp[0] == ar_kind, (B, L, tf, arp)
        assert tf[0] == lib.gvx_teacher_forced_loop_kind(h, B, L) and arp[0] == lib.gvx_autoregressive_loop_kind(h, B, L)
    # the training modes: the whole tape keeps the resident kernel, a partial one the launch per step beside the attention kernel
    assert H.decoder_plan(lib, h, 1, 32, 128)[1][0] == 2 and H.decoder_plan(lib, h, 2, 32, 128)[1] == (1, 1, 1, 0, 1, 1, 1, 0)
    out = (C.c_int * 12)(*([-7] * 12))
    for bad in ((3, 4, 4), (-1, 4, 4), (0, 0, 4), (0, 4, 0)):
        assert lib.gvx_debug_decoder_plan(h, *bad, out) == -1 and list(out) == [-7] * 12, bad
    assert lib.gvx_debug_decoder_plan(None, 0, 4, 4, out) == -1 and H.graph_replays(lib, h) == 0 and H.graph_replays(lib, None) == -1
    lib.gvx_model_destroy(h)
    for over in H.FWD_REFUSED_DIMS:
        mk = {k: v for k, v in over.items() if k != "n_mels"}
        d = dims_from_configs(Tacotron2Config(**mk), AudioConfig(n_mels=over.get("n_mels", 80)), TextConfig(n_tokens=40))
        hh = C.c_void_p()
        assert lib.gvx_model_create(C.byref(d), C.byref(hh)) == -2 and not hh.value, over


def test_encoder_recurrence_plan_of_every_listed_case():
    """ENC_FWD_CASES: the one resident launch for B <= 32 at H = 256 unless GVX_ENC_PERSISTENT=0, the launch per position otherwise
    (gvx_debug_encoder_resident); both sides of B 32 | 33."""
    from tests import helpers as H

    lib = _lib.load()
    for c in H.ENC_FWD_CASES:
        h = H.create_handle(lib, dims_from_configs(*H.enc_fwd_configs(c.H)), c.env)
        assert H.encoder_resident(lib, h, c.B) == c.plan, c.name
        lib.gvx_model_destroy(h)
    assert {c.plan for c in H.ENC_FWD_CASES} == {0, 1}
    h = H.create_handle(lib, dims_from_configs(*H.enc_fwd_configs(256)))
    assert [H.encoder_resident(lib, h, B) for B in (1, 32, 33, 64, 0)] == [1, 1, 0, 0, 0] and H.encoder_resident(lib, None, 4) == 0
    lib.gvx_model_destroy(h)


def test_conv_train_plan_of_every_listed_case():
    """How a convolution layer's three products run is host arithmetic; gvx_debug_conv_train_plan reports it from the functions the
    two entry points launch through (conv_forward_gemm / conv_dgrad_gemm / conv_wgrad_gemm, plan_gemm, choose_splitk, set_splitk).
    Every case of tests/test_conv_train_gpu.py must reach the tiles and the cut of K its line names, and the table as a whole every
    tile shape the layer can take, 1, 2, 3, 7 and 8 pieces, a short last piece, pieces that begin inside a sequence and at a
    sequence's first frame."""
    from tests.helpers import (CONV_TRAIN_BIG, CONV_TRAIN_BY_NAME, CONV_TRAIN_CASES, CONV_TRAIN_OPTION_CASES, CONV_TRAIN_REGROUP_CASES,
                               conv_train_plan)

    if os.environ.get("GVX_GEMM_8W", "")[:1] == "0":
        pytest.skip("the table is for the default eight-wave tile")
    lib = _lib.load()
    assert len(CONV_TRAIN_BY_NAME) == len(CONV_TRAIN_CASES)
    assert set(CONV_TRAIN_OPTION_CASES + CONV_TRAIN_REGROUP_CASES + [CONV_TRAIN_BIG]) <= set(CONV_TRAIN_BY_NAME)
    for c in CONV_TRAIN_CASES:
        rc, plan, wgrad_rows_big = conv_train_plan(lib, c.B, c.Cin, c.Cout, c.T, c.k)
        assert rc == 0 and plan == c.plan and wgrad_rows_big == 0, (c, rc, plan)
        assert c.name.endswith("_%dx%d_%dto%d_k%d" % (c.B, c.T, c.Cin, c.Cout, c.k)), c.name
    cases, plans = CONV_TRAIN_CASES, [c.plan for c in CONV_TRAIN_CASES]
    assert {p[0] for p in plans} == {4111, 2311, 4113, 2211, 2212, 4212} and {p[2] for p in plans} == {4111, 2311, 4113, 2211, 2212, 4212}
    assert {p[4] for p in plans} == {2212, 2222}
    assert any(p[1] > 0 and p[1] % c.T for c, p in zip(cases, plans)) and any(p[3] > 0 for p in plans)   # a second launch, from inside a sequence
    assert {p[5] for p in plans} >= {1, 2, 3, 7, 8}
    split = [(c, p) for c, p in zip(cases, plans) if p[5] > 1]
    assert all(p[6] % 64 == 0 and (p[5] - 1) * p[6] < c.B * c.T <= p[5] * p[6] for c, p in split)
    assert any(c.B * c.T % p[6] for c, p in split) and any(c.B * c.T % p[6] == 0 for c, p in split)       # a short last piece, and none
    assert any(p[6] % c.T and c.B > 1 for c, p in split) and any(p[6] % c.T == 0 and c.B > 1 for c, p in split)
    assert any(c.T == 1 for c, p in split) and any(c.B == 1 for c, p in split)
    # T against the halo and the k-tile, the rows against the reduction walk, the options
    whole = [c for c, p in zip(cases, plans) if p[5] == 1]
    assert {c.T for c in whole} >= {1, 2, 3, 4, 5, 7, 31, 32, 33, 63, 64, 65} and {c.k for c in whole} >= {1, 3, 5, 7}
    assert any(c.T < (c.k - 1) // 2 for c in cases) and any(c.T == 1 and c.k == 7 for c in cases)
    for co in (8, 40, 136):
        assert {c.B * c.T for c in cases if c.Cout == co} >= {1, 2, 31, 32, 33, 127, 128, 129, 255, 257}, co
    assert {c.B * c.T for c in cases} >= {511, 512, 513, 767, 768, 2047, 2048}
    assert {(c.act, c.p) for c in cases} >= {(a, p) for a in ("none", "relu", "tanh") for p in (None, 0.0, 0.5, 0.9)}
    assert any(not c.running for c in cases) and any(c.offset >= 1e3 for c in cases)
    assert sum(1 for c in cases if c.B * c.T * c.Cout * c.k * c.Cin > 1e10) == 1 and CONV_TRAIN_BY_NAME[CONV_TRAIN_BIG].plan[1] > 0
    # choose_splitk's thresholds, one step to either side: few tiles split from 512 rows on, one more piece per 256 rows up to 8; the
    # 160 tiles of 512 x 2560 take 3 pieces from 768 rows and 8 from 2048; from 256 tiles of 64 x 128 on nothing is split
    pieces = lambda rows, ci=24, co=24, k=5: conv_train_plan(lib, 1, ci, co, rows, k)[1][5:]
    assert pieces(511) == (1, 0) and pieces(512) == (2, 256) and pieces(513) == (2, 320) and pieces(767) == (2, 384) and pieces(768) == (3, 256)
    assert pieces(1791) == (6, 320) and pieces(1792) == (7, 256) and pieces(2047) == (7, 320) and pieces(2048) == (8, 256) and pieces(6400) == (8, 832)
    assert pieces(767, 512, 512) == (1, 0) and pieces(768, 512, 512) == (3, 256) and pieces(2047, 512, 512) == (3, 704) and pieces(2048, 512, 512) == (8, 256)
    assert pieces(6400, 512, 1024, 3) == (4, 1600) and pieces(6400, 512, 1024, 5) == (1, 0)   # 16 x 12 = 192 tiles: 3 rounds of 256 for 4 pieces; 320 tiles: whole
    # refused exactly where the entry points refuse
    out = (C.c_int * 8)()
    fn = lib.gvx_debug_conv_train_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int)]
    assert fn(1, 8, 8, 1, 1, out) == 0 and fn(1, 8, 8, 1, 1, None) == -1 and fn(1, 12, 8, 1, 1, out) == -2 and fn(1, 8, 8, 1, 2, out) == -2


CONV_BAD_SHAPES = [
    (3, 12, 24, 5, 3), (3, 24, 20, 5, 3), (3, 4, 24, 5, 3), (3, 24, 4, 5, 3), (3, 0, 24, 5, 3), (3, 24, 0, 5, 3), (3, -8, 24, 5, 3),   # channels
    (3, 24, 24, 5, 2), (3, 24, 24, 5, 4), (3, 24, 24, 5, 0), (3, 24, 24, 5, -1), (3, 24, 24, 5, -3),                                   # kernel size
    (0, 24, 24, 5, 3), (-1, 24, 24, 5, 3), (3, 24, 24, 0, 3), (3, 24, 24, -2, 3),                                                      # B, T
    (32768, 8, 8, 32769, 1), (1, 8, 8, (1 << 30) + 1, 1), ((1 << 30) + 1, 8, 8, 1, 1),                                                 # B T above 2^30
]


def test_conv_train_entry_points_validate_their_arguments_on_the_host():
    """Every check of gvx_conv_bn_act_train_forward / _backward and of the two size queries runs before the first HIP call, so it is
    tested here: the shapes the header lists as refused (the queries return 0 exactly there), NULL arguments, buffers one byte too
    small, misaligned buffers, an unknown activation, a dropout probability outside [0, 1) with a mask.  The pointers are made-up
    addresses: a call that got past its checks would launch on them, and without a device fail with GVX_ERR_HIP, never 0."""
    lib = _lib.load()
    P = 1 << 20                                          # any 256-byte aligned non-null address
    B, Cin, Cout, T, k = 3, 24, 40, 5, 5
    sb, wb = lib.gvx_conv_train_saved_bytes(B, Cin, Cout, T, k), lib.gvx_conv_train_workspace_bytes(B, Cin, Cout, T, k)
    assert sb > 0 and wb > 0 and sb % 256 == 0 and wb % 256 == 0
    # saved: the halo-padded input, xhat and the activation, mean and invstd, each rounded up to 256 bytes
    up = lambda n: (4 * n + 255) // 256 * 256
    assert sb == up(B * (T + 4) * Cin) + 2 * up(B * T * Cout) + 2 * up(Cout)
    assert lib.gvx_conv_train_saved_bytes(1, 8, 8, 1, 1) > 0 and lib.gvx_conv_train_workspace_bytes(1, 8, 8, 1, 1) > 0
    assert lib.gvx_conv_train_saved_bytes(1, 8, 8, 1 << 30, 1) > 0          # the largest B T the row index holds

    def fwd(shape=(B, Cin, Cout, T, k), act=2, keep=P, p=0.5, sbytes=sb, wbytes=wb, **ptr):
        a = dict(x=P, w=P, bias=P, gamma=P, beta=P, rm=P, rv=P, y=P, saved=P, ws=P)
        a.update(ptr)
        return lib.gvx_conv_bn_act_train_forward(a["x"], a["w"], a["bias"], a["gamma"], a["beta"], a["rm"], a["rv"], *shape, act, keep, p,
                                                 a["y"], a["saved"], sbytes, a["ws"], wbytes, None)

    def bwd(shape=(B, Cin, Cout, T, k), act=2, keep=P, p=0.5, sbytes=sb, wbytes=wb, **ptr):
        a = dict(dy=P, saved=P, w=P, gamma=P, xw=None, dx=P, dw=P, dbias=P, dgamma=P, dbeta=P, ws=P)
        a.update(ptr)
        return lib.gvx_conv_bn_act_train_backward(a["dy"], a["saved"], sbytes, a["w"], a["gamma"], a["xw"], *shape, act, keep, p, a["dx"],
                                                  a["dw"], a["dbias"], a["dgamma"], a["dbeta"], a["ws"], wbytes, None)

    for shape in CONV_BAD_SHAPES:
        assert lib.gvx_conv_train_saved_bytes(*shape) == 0 and lib.gvx_conv_train_workspace_bytes(*shape) == 0, shape
        for call in (fwd, bwd):
            assert call(shape=shape, sbytes=1 << 40, wbytes=1 << 40) == -2, (call.__name__, shape)
            msg = lib.gvx_last_error()
            assert b"conv training op" in msg and (b"multiples of 8" in msg or b"B * T exceeds" in msg), msg
    for call, names in ((fwd, ("x", "w", "bias", "gamma", "beta", "y", "saved", "ws")),
                        (bwd, ("dy", "saved", "w", "gamma", "dw", "dbias", "dgamma", "dbeta", "ws"))):
        for n in names:
            assert call(**{n: None}) == -1 and b"null argument" in lib.gvx_last_error(), (call.__name__, n)
        for act in (-1, 3, 7):
            assert call(act=act) == -1 and b"activation must be" in lib.gvx_last_error(), (call.__name__, act)
        for p in (1.0, 1.5, -0.1, float("nan"), float("inf")):
            assert call(p=p) == -1 and b"dropout probability" in lib.gvx_last_error(), (call.__name__, p)
        assert call(sbytes=sb - 1) == -5 and b"too small" in lib.gvx_last_error(), call.__name__
        assert call(wbytes=wb - 1) == -5 and b"too small" in lib.gvx_last_error(), call.__name__
        assert call(sbytes=0) == -5 and call(wbytes=0) == -5
        for off in (4, 16, 128, 255):
            assert call(saved=P + off) == -5 and b"256-byte aligned" in lib.gvx_last_error(), (call.__name__, off)
            assert call(ws=P + off) == -5 and b"256-byte aligned" in lib.gvx_last_error(), (call.__name__, off)
    # the order of the checks: the shape first, then NULL, then the options, then the buffers
    assert fwd(shape=CONV_BAD_SHAPES[0], x=None, act=9, sbytes=0) == -2 and fwd(x=None, act=9, sbytes=0) == -1 and fwd(act=9, sbytes=0) == -1
    assert bwd(shape=CONV_BAD_SHAPES[0], dy=None, act=9, sbytes=0) == -2 and bwd(dy=None, act=9, sbytes=0) == -1 and bwd(act=9, sbytes=0) == -1


# ---- the whole training step's case table (tests/helpers.py) against the host-only plan queries
def test_train_step_case_table_is_pinned():
    """Every line of TRAIN_STEP_CASES: its chunk list is what Tacotron2._forward_train cuts (at most STREAM_ROWS rows each, in
    order), every chunk's decoder loop - the training call's plan and gvx_teacher_forced_loop_kind - is the kind the line records, and
    gvx_teacher_forced_rows_per_call agrees that a call takes 32 rows.  The table holds what it promises: every chunk edge, T = 1,
    L = 1, both sides of L = 128 and 256, several chunks of different size, both loop kinds, both forced paths."""
    from genvox_amd.tacotron2 import STREAM_ROWS
    from tests import helpers as H

    lib = _lib.load()
    assert len(H.TRAIN_STEP_BY_NAME) == len(H.TRAIN_STEP_CASES) and H.TRAIN_STEP_MANY in H.TRAIN_STEP_BY_NAME
    for c in H.TRAIN_STEP_CASES:
        assert c.chunks == tuple((lo, min(c.B, lo + STREAM_ROWS)) for lo in range(0, c.B, STREAM_ROWS)), c.name
        h = H.create_handle(lib, dims_from_configs(*H.train_step_configs(c)))
        if c.forced == "resident_off":
            assert lib.gvx_model_set_resident_kernels(h, 0) == 0
        assert lib.gvx_teacher_forced_rows_per_call(h, c.L) == STREAM_ROWS, c.name
        kinds = []
        for lo, hi in c.chunks:
            rc, tf, _ = H.decoder_plan(lib, h, 1, hi - lo, c.L)
            assert rc == 0, c.name
            kinds.append((tf[0], lib.gvx_teacher_forced_loop_kind(h, hi - lo, c.L)))
        lib.gvx_model_destroy(h)
        assert tuple(kinds) == c.kinds, (c.name, kinds)
        tl, ml = H.bptt_lengths("ragged", c.B, c.L), H.train_step_mel_lengths(c.B, c.T)
        assert max(tl) == c.L and max(ml) == c.T and sorted(tl, reverse=True) == tl
        if c.B >= 2:
            assert min(tl) == 1 and min(ml) == 1, c.name
    cs = H.TRAIN_STEP_CASES
    assert {c.B for c in cs if c.dims == "small"} >= {1, 2, 31, 32, 33, 64, 65}
    assert any(c.T == 1 for c in cs) and any(c.L == 1 for c in cs) and any(not c.mask_padding for c in cs)
    assert {c.L for c in cs if c.dims == "def"} >= {128, 129, 150, 300}
    assert any(len({hi - lo for lo, hi in c.chunks}) == 2 and c.dims == "def" for c in cs)
    assert {k[0] for c in cs for k in c.kinds} == {0, 2} and {c.forced for c in cs} == {None, "resident_off", "enc_walk_per_step"}
    many = H.TRAIN_STEP_BY_NAME[H.TRAIN_STEP_MANY]
    assert many.B * many.T == 6400 and many.dims == "def"
    for dims, steps in H.TRAIN_TRAJECTORY.items():   # the trajectory re-sizes tapes and workspaces between steps, one and two chunks
        assert len(steps) == 4 and len(set(steps)) == 4 and {b > STREAM_ROWS for b, _, _ in steps} == {False, True}, dims
