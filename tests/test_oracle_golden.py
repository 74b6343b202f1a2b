"""CPU: the oracle (oracle/) against the golden fixtures produced by the reference itself.
This is what pins the oracle; the GPU parity tests then compare the HIP path with both."""
import numpy as np
import pytest
import torch

from oracle import audio_ref, tacotron2_ref
from tests.golden.cases import AR_CASES, AUDIO_CASE, TF_CASES, case_configs
from tests.helpers import case_state_dict, load_fixture, max_abs_diff, tf_batch, unpack_masks

ORACLE_TOL = 2e-5  # the reference's own fp32-vs-fp64 drift is ~2e-6


@pytest.mark.parametrize("name", list(TF_CASES))
def test_teacher_forced_oracle_matches_reference(name):
    case, fx = TF_CASES[name], load_fixture(name)
    mc, ac, tc = case_configs(case)
    sd = case_state_dict(name)
    B, T = case["B"], case["T"]
    masks = unpack_masks(fx["keep_masks_packed"], (2, (T + 1) * B, mc.prenet_dim))
    out = tacotron2_ref.tacotron2_forward(sd, tf_batch(fx), masks, mask_padding=mc.mask_padding, taps=True)
    for key in ("encoder_outputs", "processed_memory", "prenet_outputs", "attention_contexts",
                "alignments", "gate_outputs", "mel_outputs", "mel_outputs_postnet"):
        d = max_abs_diff(out[key], fx[key])
        assert d <= ORACLE_TOL, f"{name}/{key}: {d}"
    # padding semantics: zero mels, gate 1e3, zero encoder rows past each length
    for b in range(B):
        ml, tl = int(fx["mel_lengths"][b]), int(fx["token_lengths"][b])
        assert torch.all(out["mel_outputs_postnet"][b, :, ml:] == 0)
        assert torch.all(out["gate_outputs"][b, ml:] == 1e3)
        assert torch.all(out["encoder_outputs"][b, tl:] == 0)
        assert torch.all(out["alignments"][b, :, tl:] == 0)


@pytest.mark.parametrize("name", list(AR_CASES))
def test_autoregressive_oracle_matches_reference(name):
    case, fx = AR_CASES[name], load_fixture(name)
    mc, ac, tc = case_configs(case)
    sd = case_state_dict(name)
    steps = int(fx["max_decoder_steps"])
    masks = unpack_masks(fx["keep_masks_packed"], (2, steps, mc.prenet_dim))
    out = tacotron2_ref.tacotron2_inference(sd, torch.from_numpy(fx["tokens"]), masks,
                                            float(fx["gate_threshold"]), steps)
    assert out["mel_outputs"].shape == fx["mel_outputs"].shape
    if case["gate_fires"]:
        assert out["mel_outputs"].shape[2] < steps
    for key in ("alignments", "gate_outputs", "mel_outputs", "mel_outputs_postnet"):
        d = max_abs_diff(out[key], fx[key])
        assert d <= ORACLE_TOL, f"{name}/{key}: {d}"


def test_audio_oracle_matches_reference():
    c, fx = AUDIO_CASE, load_fixture("audio")
    n_fft, hop = c["n_fft"], c["hop"]
    basis = audio_ref.mel_filter(c["fs"], n_fft, c["n_mels"], c["fmin"], c["fmax"])
    assert basis.dtype == np.float32 and np.array_equal(basis, fx["mel_basis"])
    inv = audio_ref.inverse_mel_filter(basis)
    assert max_abs_diff(inv, fx["inverse_mel_basis"]) <= 1e-6
    spec = audio_ref.stft(fx["signal"], n_fft, hop)
    assert spec.dtype == np.complex64
    assert np.array_equal(spec.real, fx["stft_real"]) and np.array_equal(spec.imag, fx["stft_imag"])
    assert np.array_equal(audio_ref.istft(spec, n_fft, hop), fx["istft"])
    mel_db = audio_ref.wav_to_mel(fx["signal"], fx["mel_basis"], n_fft, hop, c["log_func"], c["ref"])
    assert mel_db.dtype == np.float32 and max_abs_diff(mel_db, fx["mel_db"]) <= 1e-6
    mag = np.matmul(fx["inverse_mel_basis"], audio_ref.db_to_amplitude(fx["mel_db"], c["log_func"], c["ref"]))
    assert max_abs_diff(mag, fx["mag"]) <= 1e-6
    for k in (1, 2, 32):
        ph = audio_ref.griffin_lim(fx["mag"], n_fft, hop, n_iter=k)
        # phases are compared on the unit circle (wrap-around safe)
        d = np.abs(np.exp(1j * ph) - np.exp(1j * fx[f"gl_phase_{k}"])).max()
        assert d <= 1e-4, (k, d)
    fs, wav = audio_ref.convert_mel2wav(fx["mel_db"].copy(), fx["inverse_mel_basis"], c["fs"], n_fft, hop,
                                        c["log_func"], c["ref"])
    assert fs == int(fx["fs"]) and wav.shape == fx["wav"].shape and wav.dtype == np.float64
    assert max_abs_diff(wav, fx["wav"]) <= 1e-4


@pytest.mark.parametrize("name", sorted(TF_CASES))
def test_oracle_loss_matches_reference_criterion(name):
    """Tacotron2Loss on the reference's own outputs (fixture values from the reference's criterion)."""
    fx = load_fixture(name)
    batch = {"mel_padded": torch.from_numpy(fx["mel_padded"]), "gate_padded": torch.from_numpy(fx["gate_padded"])}
    outputs = {k: torch.from_numpy(fx[k]) for k in ("mel_outputs", "mel_outputs_postnet", "gate_outputs")}
    got = tacotron2_ref.tacotron2_loss(batch, outputs)
    for k in ("loss", "mel_loss", "gate_loss"):
        assert abs(float(got[k]) - float(fx[k])) <= 2e-6 * max(1.0, abs(float(fx[k]))), k


def test_training_oracle_matches_reference_gradients():
    """oracle/train_ref.py (explicit forward / backward formulas of the training-mode convolution stacks and of the
    criterion) against tests/golden/train_small.npz: the reference's own .train() forward and loss.backward()."""
    import numpy as np

    from genvox_amd import weights as gw
    from oracle import train_ref as tr
    from tests.golden.cases import TRAIN_CASE

    z = load_fixture("train_small")
    mc, ac, tc = case_configs(TRAIN_CASE)
    sd = gw.generate_state_dict(mc, ac, tc, seed=TRAIN_CASE["weight_seed"], peaky_attention=True)
    B, L, T = TRAIN_CASE["B"], TRAIN_CASE["L"], TRAIN_CASE["T"]
    M, C, n, E, ne = ac.n_mels, mc.postnet_embedding_dim, mc.postnet_n_convolutions, mc.encoder_embedding_dim, mc.encoder_n_convolutions

    def unpack(packed, shape):
        k = int(np.prod(shape))
        return torch.from_numpy(np.unpackbits(packed, axis=1)[:, :k].reshape((packed.shape[0],) + tuple(shape)))

    pk, pl = unpack(z["post_keep_packed"], (B, C, T)), unpack(z["post_last_keep_packed"], (B, M, T))
    keeps = [pk[i] for i in range(n - 1)] + [pl[0]]
    x = torch.from_numpy(z["decoder_mel_unmasked"])
    y, saved = tr.convstack_train_forward(sd, "postnet.convolutions", n, tr.postnet_acts(n), x, keeps)
    post = x + y
    for b in range(B):
        post[b, :, int(z["mel_lengths"][b]):] = 0
    assert max_abs_diff(post, z["mel_outputs_postnet"]) <= 1e-5
    outs = {k: torch.from_numpy(z[k]) for k in ("mel_outputs", "mel_outputs_postnet", "gate_outputs")}
    dmel, dpost, dgate = tr.loss_backward({k: torch.from_numpy(z[k]) for k in ("mel_padded", "gate_padded")}, outs)
    assert max_abs_diff(dpost, z["grad_post_out"]) <= 1e-7
    saved[0]["x"] = outs["mel_outputs"]   # masked in place by the reference after its forward (models/tts/tacotron2.py:470)
    dx, grads = tr.convstack_train_backward(sd, "postnet.convolutions", n, tr.postnet_acts(n), dpost, saved, keeps)
    assert max_abs_diff(dmel + dpost + dx, z["grad_mel_outputs"]) <= 1e-6
    ek = unpack(z["enc_keep_packed"], (B, E, L))
    emb = sd["embedding.weight"][torch.from_numpy(z["token_padded"])].transpose(1, 2)
    _, esaved = tr.convstack_train_forward(sd, "encoder.convolutions", ne, tr.encoder_acts(ne), emb, [ek[i] for i in range(ne)])
    _, egrads = tr.convstack_train_backward(sd, "encoder.convolutions", ne, tr.encoder_acts(ne), torch.from_numpy(z["grad_enc_conv_out"]), esaved,
                                            [ek[i] for i in range(ne)])
    for k, v in {**grads, **egrads}.items():
        assert max_abs_diff(v, z["grad." + k]) <= 2e-6, k
    rm, rv = tr.bn_running_update(sd["encoder.convolutions.0.1.running_mean"], sd["encoder.convolutions.0.1.running_var"],
                                  esaved[0]["mean"], esaved[0]["var"], B * L)
    assert max_abs_diff(rm, z["state.encoder.convolutions.0.1.running_mean"]) <= 1e-6
    assert max_abs_diff(rv, z["state.encoder.convolutions.0.1.running_var"]) <= 1e-6


def test_training_step_oracle_matches_reference_backward():
    """oracle/train_ref.py train_forward / train_backward - the whole training step in explicit formulas: BPTT over the decoder
    loop (both LSTM cells with output dropout, location-sensitive attention incl. the cumulative-weights path), Prenet,
    encoder BiLSTM with packed-sequence semantics, convolution stacks, embedding - against the gradient of EVERY parameter
    that the reference's loss.backward() produced (tests/golden/train_small.npz, 48 tensors)."""
    import numpy as np

    from genvox_amd import weights as gw
    from oracle import train_ref as tr
    from tests.golden.cases import TRAIN_CASE

    z = load_fixture("train_small")
    mc, ac, tc = case_configs(TRAIN_CASE)
    sd = gw.generate_state_dict(mc, ac, tc, seed=TRAIN_CASE["weight_seed"], peaky_attention=True)
    B, L, T = TRAIN_CASE["B"], TRAIN_CASE["L"], TRAIN_CASE["T"]
    M, C, n, E = ac.n_mels, mc.postnet_embedding_dim, mc.postnet_n_convolutions, mc.encoder_embedding_dim
    A, D, P = mc.attention_rnn_dim, mc.decoder_rnn_dim, mc.prenet_dim

    def unpack(packed, shape):
        k = int(np.prod(shape))
        return torch.from_numpy(np.unpackbits(packed, axis=1)[:, :k].reshape((packed.shape[0],) + tuple(shape)))

    pk, pl = unpack(z["post_keep_packed"], (B, C, T)), unpack(z["post_last_keep_packed"], (B, M, T))
    masks = {"encoder": list(unpack(z["enc_keep_packed"], (B, E, L))), "prenet": unpack(z["prenet_keep_packed"], (T + 1, B, P)),
             "attention_rnn": unpack(z["att_keep_packed"], (B, A)), "decoder_rnn": unpack(z["dec_keep_packed"], (B, D)),
             "postnet": [pk[i] for i in range(n - 1)] + [pl[0]]}
    batch = {k: torch.from_numpy(z[k]) for k in ("token_padded", "token_lengths", "mel_padded", "gate_padded", "mel_lengths")}
    out, tape = tr.train_forward(sd, batch, masks, mc)
    for k in ("mel_outputs", "mel_outputs_postnet", "gate_outputs", "alignments"):
        assert max_abs_diff(out[k], z[k]) <= ORACLE_TOL, k
    grads = tr.train_backward(sd, batch, masks, mc, out, tape)
    names = [k[5:] for k in z if k.startswith("grad.")]
    assert sorted(grads) == sorted(names)
    for k in names:
        ref = z["grad." + k]
        scale = max(float(np.abs(ref).max()), 1e-6)
        assert max_abs_diff(grads[k], ref) <= max(1e-4 * scale, 2e-6), k


# ---- tests/forward_ref.py: the float64 reference of the forward loops (what tests/test_forward_loops_gpu.py holds the kernels to)
def _ref_encoder_and_weights(sd, tokens, lengths):
    from tests import forward_ref as fr

    sd64 = fr.to_f64(sd)
    return fr, fr.decoder_weights(sd), fr.whole_encoder(sd64, tokens, lengths)


@pytest.mark.parametrize("name", list(TF_CASES))
def test_float64_forward_reference_matches_the_teacher_forced_fixtures(name):
    """whole_encoder + teacher_forced in float64 against the reference's own fp32 outputs, at the bound the fp32 oracle meets."""
    case, fx = TF_CASES[name], load_fixture(name)
    mc, ac, tc = case_configs(case)
    B, T = case["B"], case["T"]
    fr, W, enc = _ref_encoder_and_weights(case_state_dict(name), torch.from_numpy(fx["token_padded"]), fx["token_lengths"])
    masks = unpack_masks(fx["keep_masks_packed"], (2, (T + 1) * B, mc.prenet_dim))
    out = fr.teacher_forced(W, enc["memory"], fx["token_lengths"], torch.from_numpy(fx["mel_padded"]).double(), masks)
    pad = torch.arange(T)[None, :] >= torch.from_numpy(fx["mel_lengths"])[:, None]
    got = {"encoder_outputs": enc["memory"], "processed_memory": out["pm"], "attention_contexts": out["ctx"].transpose(0, 1),
           "alignments": out["w"].transpose(0, 1), "gate_outputs": out["gate"].t().masked_fill(pad, 1e3),
           "mel_outputs": out["mel"].permute(1, 2, 0).masked_fill(pad[:, None, :], 0.0), "prenet_outputs": out["prenet"]}
    for key, g in got.items():
        want = fx[key][:T] if key == "prenet_outputs" else fx[key]
        assert max_abs_diff(g, want) <= ORACLE_TOL, f"{name}/{key}"
    assert out["ga"].dtype == torch.float64 and out["w"].dtype == torch.float64
    assert max_abs_diff(out["w"].sum(-1), torch.ones(T, B)) <= 1e-12


@pytest.mark.parametrize("name", list(AR_CASES))
def test_float64_forward_reference_matches_the_autoregressive_fixtures(name):
    """autoregressive() against the reference's free-running decode: the stop step exactly, every frame at the oracle's bound."""
    case, fx = AR_CASES[name], load_fixture(name)
    mc, ac, tc = case_configs(case)
    steps, thr = int(fx["max_decoder_steps"]), float(fx["gate_threshold"])
    fr, W, enc = _ref_encoder_and_weights(case_state_dict(name), torch.from_numpy(fx["tokens"]), None)
    masks = unpack_masks(fx["keep_masks_packed"], (2, steps, mc.prenet_dim)).reshape(2, steps, 1, mc.prenet_dim)
    out = fr.autoregressive(W, enc["memory"], [case["L"]], steps, thr, masks)
    n = fx["mel_outputs"].shape[2]
    assert int(out["n_frames"][0]) == n and (n < steps) == case["gate_fires"]
    assert 0.0 < out["margin"] < 1.0   # (reported, not bounded: the fixtures' thresholds were not chosen for a margin - ar_small_gate passes 5e-6 from its own)
    assert max_abs_diff(out["mel_out"][:, :, :n], fx["mel_outputs"]) <= ORACLE_TOL
    assert max_abs_diff(out["gate_out"][:, :n], fx["gate_outputs"]) <= ORACLE_TOL
    assert max_abs_diff(out["align_out"][:, :n], fx["alignments"]) <= ORACLE_TOL
    assert bool((out["mel_out"][:, :, n:] == 0).all()) and bool((out["gate_out"][:, n:] == 1e3).all()) and bool((out["align_out"][:, n:] == 0).all())


def test_float64_forward_reference_matches_the_training_fixture():
    """encoder_bilstm + teacher_forced with the hidden-state dropout masks against the reference's .train() forward
    (tests/golden/train_small.npz); the training-mode convolution stack in front is oracle/train_ref.py's."""
    from genvox_amd import weights as gw
    from oracle import train_ref as tr
    from tests import forward_ref as fr
    from tests.golden.cases import TRAIN_CASE

    z = load_fixture("train_small")
    mc, ac, tc = case_configs(TRAIN_CASE)
    sd = gw.generate_state_dict(mc, ac, tc, seed=TRAIN_CASE["weight_seed"], peaky_attention=True)
    B, L, T = TRAIN_CASE["B"], TRAIN_CASE["L"], TRAIN_CASE["T"]
    E, A, D, P, ne = mc.encoder_embedding_dim, mc.attention_rnn_dim, mc.decoder_rnn_dim, mc.prenet_dim, mc.encoder_n_convolutions

    def unpack(packed, shape):
        k = int(np.prod(shape))
        return torch.from_numpy(np.unpackbits(packed, axis=1)[:, :k].reshape((packed.shape[0],) + tuple(shape)))

    emb = sd["embedding.weight"][torch.from_numpy(z["token_padded"])].transpose(1, 2)
    conv, _ = tr.convstack_train_forward(sd, "encoder.convolutions", ne, tr.encoder_acts(ne), emb, list(unpack(z["enc_keep_packed"], (B, E, L))))
    enc = fr.encoder_bilstm(fr.to_f64(sd), conv.double(), z["token_lengths"])
    out = fr.teacher_forced(fr.decoder_weights(sd), enc["memory"], z["token_lengths"], torch.from_numpy(z["mel_padded"]).double(),
                            unpack(z["prenet_keep_packed"], (T + 1, B, P)), unpack(z["att_keep_packed"], (B, A)), unpack(z["dec_keep_packed"], (B, D)),
                            1.0 / (1.0 - mc.p_attention_dropout), 1.0 / (1.0 - mc.p_decoder_dropout))
    assert max_abs_diff(out["mel"].permute(1, 2, 0), z["decoder_mel_unmasked"]) <= ORACLE_TOL
    assert max_abs_diff(out["w"].transpose(0, 1), z["alignments"]) <= ORACLE_TOL
    pad = torch.arange(T)[None, :] >= torch.from_numpy(z["mel_lengths"])[:, None]
    assert max_abs_diff(out["gate"].t().masked_fill(pad, 1e3), z["gate_outputs"]) <= ORACLE_TOL
