"""ctypes binding of libgenvox_amd.so (C ABI declared in include/genvox_amd.h).

There is no fallback: if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("GVX_LIB", "libgenvox_amd.so"))  # GVX_LIB: diagnostic builds only


class GvxError(RuntimeError):
    pass


class gvx_dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_tokens", "embed_dim", "enc_kernel", "enc_n_conv", "prenet_dim", "att_rnn_dim", "dec_rnn_dim", "att_dim",
        "att_loc_filters", "att_loc_kernel", "postnet_dim", "postnet_kernel", "postnet_n_conv", "n_mels")]


class gvx_weight_desc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


_vp, _i, _sz, _f, _l = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_long


class gvx_melgan_dims(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("base_channels", C.c_int32), ("n_stages", C.c_int32), ("ratios", C.c_int32 * 8),
                ("n_residual_layers", C.c_int32), ("dilation_base", C.c_int32), ("slope", C.c_float)]


class gvx_hifigan_dims(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("upsample_initial_channel", C.c_int32), ("n_stages", C.c_int32), ("upsample_rates", C.c_int32 * 8),
                ("upsample_kernel_sizes", C.c_int32 * 8), ("resblock", C.c_int32), ("n_resblocks", C.c_int32), ("n_dilations", C.c_int32),
                ("resblock_kernel_sizes", C.c_int32 * 4), ("resblock_dilation_sizes", (C.c_int32 * 3) * 4), ("slope", C.c_float),
                ("post_slope", C.c_float)]


class gvx_bigvgan_dims(C.Structure):
    _fields_ = [("net", gvx_hifigan_dims), ("snakebeta", C.c_int32), ("tanh_at_final", C.c_int32), ("bias_at_final", C.c_int32)]


class gvx_vocos_dims(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_mels", "dim", "intermediate_dim", "num_layers", "n_fft", "hop_length", "center")]


class gvx_fft_stack_dims(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_layers", "n_head", "d_head", "d_inner", "kernel_size")]


class gvx_fastpitch_dims(C.Structure):
    _fields_ = [("n_tokens", C.c_int32), ("n_mels", C.c_int32), ("d_model", C.c_int32), ("enc", gvx_fft_stack_dims), ("dec", gvx_fft_stack_dims)] + [
        (k, C.c_int32) for k in ("pred_filter", "pred_layers", "energy", "max_tokens", "max_decoder_steps", "max_duration", "min_token_frames")]


class gvx_univnet_dims(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("noise_dim", C.c_int32), ("channel_size", C.c_int32), ("n_dilations", C.c_int32),
                ("dilations", C.c_int32 * 8), ("n_blocks", C.c_int32), ("strides", C.c_int32 * 4), ("kpnet_hidden_channels", C.c_int32),
                ("kpnet_conv_size", C.c_int32), ("slope", C.c_float)]


class gvx_melgan_tape_entry(C.Structure):
    _fields_ = [("byte_offset", C.c_uint64), ("positions_per_frame", C.c_int32), ("channels", C.c_int32)]


gvx_hifigan_tape_entry = gvx_melgan_tape_entry   # the header's typedef


class gvx_vocos_tape_entry(C.Structure):
    _fields_ = [("byte_offset", C.c_uint64), ("rows", C.c_int32), ("channels", C.c_int32)]


class gvx_melgan_disc_dims(C.Structure):
    _fields_ = [("n_scales", C.c_int32), ("base_channels", C.c_int32), ("n_layers", C.c_int32), ("downsampling_factor", C.c_int32),
                ("max_channels", C.c_int32), ("slope", C.c_float)]


class gvx_melgan_disc_entry(C.Structure):
    _fields_ = [("byte_offset", C.c_uint64), ("channels", C.c_int32), ("positions", C.c_int32)]


class gvx_hifigan_mpd_dims(C.Structure):
    _fields_ = [("n_periods", C.c_int32), ("periods", C.c_int32 * 8), ("n_layers", C.c_int32), ("channels", C.c_int32 * 8),
                ("kernel_size", C.c_int32), ("stride", C.c_int32), ("slope", C.c_float)]


class gvx_hifigan_msd_dims(C.Structure):
    _fields_ = [("n_scales", C.c_int32), ("n_layers", C.c_int32), ("channels", C.c_int32 * 8), ("kernel_sizes", C.c_int32 * 8),
                ("strides", C.c_int32 * 8), ("groups", C.c_int32 * 8), ("slope", C.c_float)]


class gvx_hifigan_msd_entry(C.Structure):
    _fields_ = [("byte_offset", C.c_uint64), ("channels", C.c_int32), ("length", C.c_int32),
                ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_l", C.c_int64)]


class gvx_hifigan_mpd_entry(C.Structure):
    _fields_ = [("byte_offset", C.c_uint64), ("channels", C.c_int32), ("height", C.c_int32), ("period", C.c_int32), ("reserved", C.c_int32),
                ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_h", C.c_int64), ("stride_p", C.c_int64)]


class gvx_mrd_dims(C.Structure):
    _fields_ = [("n_resolutions", C.c_int32), ("n_fft", C.c_int32 * 8), ("hop", C.c_int32 * 8), ("win", C.c_int32 * 8),
                ("channels", C.c_int32), ("window", C.c_int32), ("slope", C.c_float)]


class gvx_mrd_entry(C.Structure):
    _fields_ = [("byte_offset", C.c_uint64), ("channels", C.c_int32), ("frames", C.c_int32), ("bins", C.c_int32), ("reserved", C.c_int32),
                ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_w", C.c_int64), ("stride_f", C.c_int64)]


class gvx_stft_resolution(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("win_length", C.c_int32)]


class gvx_stft_loss_debug(C.Structure):
    _fields_ = [("mag_pred", C.c_void_p * 8), ("mag_target", C.c_void_p * 8)]


class gvx_mel_loss_debug(C.Structure):
    _fields_ = [("log_mel_pred", C.c_void_p), ("log_mel_target", C.c_void_p)]


class gvx_pitch_params(C.Structure):
    _fields_ = [("sampling_rate", C.c_int32), ("hop", C.c_int32), ("window", C.c_int32), ("lag_min", C.c_int32), ("lag_max", C.c_int32),
                ("threshold", C.c_float), ("first_centre", C.c_int32)]


class gvx_psola_params(C.Structure):
    _fields_ = [("hop", C.c_int32), ("first_centre", C.c_int32), ("lag_min", C.c_int32), ("lag_max", C.c_int32),
                ("unvoiced_period", C.c_int32)]


class gvx_tensor_ref(C.Structure):
    _fields_ = [("data", C.c_void_p), ("numel", C.c_int64)]


class gvx_adam_ref(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64)]


class gvx_bptt_decoder_args(C.Structure):
    """Argument block of gvx_train_decoder_bptt (include/genvox_amd.h)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "L", "T", "A", "D", "E", "P", "a", "F", "kl")]
                + [("att_scale", C.c_float), ("dec_scale", C.c_float)]
                + [(n, C.c_void_p) for n in ("dhc_all", "pre_a", "pre_d", "c_a_all", "c_d_all", "att_keep", "dec_keep", "q_all", "ctx_all")]
                + [("ctx_ts", C.c_int64), ("ctx_bs", C.c_int64)]
                + [(n, C.c_void_p) for n in ("w_all", "memory", "pm", "w_ih_a", "w_hh_a", "w_ih_d", "w_hh_d", "wq", "v", "loc_conv", "loc_dense",
                                             "dga_all", "dgd_all", "dq_all", "dctx_all", "dpm", "dmemory", "dv", "dloc_dense", "dloc_conv")])


# name -> (restype, argtypes); every symbol include/genvox_amd.h declares
SIGNATURES = {
    "gvx_last_error": (C.c_char_p, []),
    "gvx_version": (_i, []),
    "gvx_model_create": (_i, [C.POINTER(gvx_dims), C.POINTER(_vp)]),
    "gvx_model_destroy": (None, [_vp]),
    "gvx_model_blob_bytes": (_sz, [_vp]),
    "gvx_model_pack_weights": (_i, [_vp, C.POINTER(gvx_weight_desc), _i, _vp]),
    "gvx_model_bind_blob": (_i, [_vp, _vp]),
    "gvx_model_pack_weights_device": (_i, [_vp, C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "gvx_workspace_bytes_autoregressive": (_sz, [_vp, _i, _i, _i]),
    "gvx_workspace_status": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "gvx_encoder_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "gvx_decoder_teacher_forced": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_decoder_autoregressive": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), _vp, _sz, _vp]),
    "gvx_decoder_autoregressive_windowed": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), _vp, _sz, _vp, _i, _i, _vp]),
    "gvx_postnet_workspace_bytes": (_sz, [_vp, _i, _i]),
    "gvx_postnet_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "gvx_mask_padding": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "gvx_tacotron2_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_tacotron2_loss": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "gvx_encoder_lstm_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_decoder_teacher_forced_train": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_train_export": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _vp]),
    "gvx_conv_train_saved_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "gvx_conv_train_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "gvx_conv_bn_act_train_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gvx_conv_bn_act_train_backward": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_tacotron2_loss_backward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gvx_train_gemm_nt": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "gvx_train_gemm_tn": (_i, [_vp, _l, _vp, _l, _vp, _l, _i, _i, _l, _vp, _sz, _vp]),
    "gvx_train_transpose": (_i, [_vp, _l, _vp, _l, _i, _l, _vp]),
    "gvx_train_colsum": (_i, [_vp, _l, _i, _vp, _vp]),
    "gvx_train_axpby": (_i, [_vp, _l, _f, _vp, _l, _f, _vp, _l, _l, _i, _vp]),
    "gvx_train_relu_dropout_backward": (_i, [_vp, _vp, _vp, _f, _l, _vp, _vp]),
    "gvx_train_unblock": (_i, [_vp, _vp, _l, _i, _i, _vp]),
    "gvx_train_embedding_backward": (_i, [_vp, _vp, _l, _i, _i, _vp, _vp]),
    "gvx_train_sqnorm_scratch_bytes": (_sz, [_i]),
    "gvx_train_sqnorm_many": (_i, [_vp, _i, _vp, _vp, _vp]),
    "gvx_train_adam_step_many": (_i, [_vp, _i, _f, _f, _f, _f, _f, _f, _i, _vp]),
    "gvx_train_decoder_bptt_workspace_bytes": (_sz, [C.POINTER(gvx_bptt_decoder_args)]),
    "gvx_train_decoder_bptt": (_i, [C.POINTER(gvx_bptt_decoder_args), _vp, _sz, _vp]),
    "gvx_train_decoder_bptt_ext": (_i, [C.POINTER(gvx_bptt_decoder_args), _vp, C.c_int64, C.c_int64, _vp, _sz, _vp]),
    "gvx_guided_attention_loss_scratch_bytes": (_sz, [_i, _i, _i]),
    "gvx_guided_attention_loss": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "gvx_train_encoder_lstm_bptt_workspace_bytes": (_sz, [_i, _i]),
    "gvx_train_encoder_lstm_bptt": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "gvx_train_encoder_lstm_bptt_resident": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "gvx_train_encoder_lstm_bptt_status": (_i, [_vp, _sz, _i, _i, C.POINTER(_i), _vp]),
    "gvx_prenet_masks_generate": (_i, [_vp, _sz, C.c_uint64, _vp]),
    "gvx_stage_timing_enable": (_i, [_vp, _i]),
    "gvx_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_gl_plan_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "gvx_gl_plan_destroy": (None, [_vp]),
    "gvx_gl_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "gvx_stft": (_i, [_vp, _vp, _vp, _i, C.c_long, _vp, _vp, _sz, _vp]),
    "gvx_istft": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "gvx_mel_to_magnitude": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "gvx_griffin_lim": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "gvx_wav_to_mel": (_i, [_vp, _vp, _vp, _vp, _i, C.c_long, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "gvx_wav_finalize": (_i, [_vp, _i, C.c_long, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _vp, _vp, _vp]),
    "gvx_gl_workspace_bytes_ragged": (_sz, [_vp, _i, _i, _i]),
    "gvx_griffin_lim_ragged": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "gvx_wav_finalize_ragged": (_i, [_vp, _i, C.c_long, _vp, _i, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _vp, _vp, _vp]),
    "gvx_wav_to_mel_ragged_workspace_bytes": (_sz, [_vp, _i, C.c_long, _i]),
    "gvx_wav_trim_bounds": (_i, [_vp, _i, _i, C.c_long, _vp, _i, _f, _vp, _vp]),
    "gvx_wav_to_mel_ragged": (_i, [_vp, _vp, _i, _vp, _vp, _i, C.c_long, _vp, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_resample_uses_lds_table": (_i, [_i, _i, _i]),
    "gvx_resample_block_shape": (_i, [_i, _i, _i, _vp, _vp]),
    "gvx_wav_mixdown": (_i, [_vp, _i, _i, C.c_long, _i, _vp, _vp]),
    "gvx_wav_resample_ragged": (_i, [_vp, _i, _i, C.c_long, _vp, _i, _i, _vp, _i, _vp, C.c_long, _vp, _vp]),
    "gvx_alignment_stats": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gvx_mel_project": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "gvx_dtw_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gvx_dtw_uses_lds_tables": (_i, [_i, _i, _i]),
    "gvx_dtw_distance": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "gvx_monotonic_align_workspace_bytes": (_sz, [_i, _i, _i]),
    "gvx_monotonic_align_uses_lds": (_i, [_i, _i]),
    "gvx_monotonic_align": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_duration_scale": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "gvx_mel_time_warp": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gvx_pitch_frames": (_i, [_l, _i]),
    "gvx_pitch_tile_frames": (_i, [C.POINTER(gvx_pitch_params)]),
    "gvx_pitch_yin": (_i, [_vp, _vp, _i, _l, C.POINTER(gvx_pitch_params), _vp, _vp, _vp, _vp, _vp]),
    "gvx_f0_compare": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gvx_psola_max_marks": (_l, [_l, _i]),
    "gvx_psola_max_grains": (_l, [_l, _i]),
    "gvx_psola_plan": (_i, [_vp, _vp, _vp, _vp, _i, _l, C.POINTER(gvx_psola_params), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gvx_psola_synth": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _l, C.POINTER(gvx_psola_params), _vp, _vp]),
    "gvx_melgan_blob_floats":(_sz, [C.POINTER(gvx_melgan_dims)]),
    "gvx_melgan_workspace_bytes": (_sz, [C.POINTER(gvx_melgan_dims), _i, _i]),
    "gvx_melgan_pack_weights_device": (_i, [C.POINTER(gvx_melgan_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_melgan_create": (_i, [C.POINTER(gvx_melgan_dims), C.POINTER(_vp)]),
    "gvx_melgan_destroy": (None, [_vp]),
    "gvx_melgan_bind": (_i, [_vp, _vp]),
    "gvx_melgan_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_melgan_timing_enable": (_i, [_vp, _i]),
    "gvx_melgan_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_melgan_tape_bytes": (_sz, [C.POINTER(gvx_melgan_dims), _i, _i]),
    "gvx_melgan_tape_layout": (_i, [C.POINTER(gvx_melgan_dims), _i, _i, C.POINTER(gvx_melgan_tape_entry), _i]),
    "gvx_melgan_backward_workspace_bytes": (_sz, [C.POINTER(gvx_melgan_dims), _i, _i]),
    "gvx_melgan_forward_train": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gvx_melgan_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_hifigan_blob_floats": (_sz, [C.POINTER(gvx_hifigan_dims)]),
    "gvx_hifigan_workspace_bytes": (_sz, [C.POINTER(gvx_hifigan_dims), _i, _i]),
    "gvx_hifigan_pack_weights_device": (_i, [C.POINTER(gvx_hifigan_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_hifigan_create": (_i, [C.POINTER(gvx_hifigan_dims), C.POINTER(_vp)]),
    "gvx_hifigan_destroy": (None, [_vp]),
    "gvx_hifigan_bind": (_i, [_vp, _vp]),
    "gvx_hifigan_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_hifigan_timing_enable": (_i, [_vp, _i]),
    "gvx_hifigan_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_hifigan_backward_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_hifigan_tape_bytes": (_sz, [C.POINTER(gvx_hifigan_dims), _i, _i]),
    "gvx_hifigan_tape_layout": (_i, [C.POINTER(gvx_hifigan_dims), _i, _i, C.POINTER(gvx_melgan_tape_entry), _i]),
    "gvx_hifigan_backward_workspace_bytes": (_sz, [C.POINTER(gvx_hifigan_dims), _i, _i]),
    "gvx_hifigan_forward_train": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gvx_hifigan_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_hifigan_layer": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _f, _i, _vp]),
    "gvx_melgan_disc_blob_floats": (_sz, [C.POINTER(gvx_melgan_disc_dims)]),
    "gvx_melgan_disc_pack_weights_device": (_i, [C.POINTER(gvx_melgan_disc_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_melgan_disc_create": (_i, [C.POINTER(gvx_melgan_disc_dims), C.POINTER(_vp)]),
    "gvx_melgan_disc_destroy": (None, [_vp]),
    "gvx_melgan_disc_bind": (_i, [_vp, _vp]),
    "gvx_melgan_disc_layout": (_i, [C.POINTER(gvx_melgan_disc_dims), _i, _i, C.POINTER(gvx_melgan_disc_entry), _i]),
    "gvx_melgan_disc_features_bytes": (_sz, [C.POINTER(gvx_melgan_disc_dims), _i, _i]),
    "gvx_melgan_disc_workspace_bytes": (_sz, [C.POINTER(gvx_melgan_disc_dims), _i, _i, _i]),
    "gvx_melgan_disc_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "gvx_melgan_disc_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_snake_antialiased": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gvx_bigvgan_blob_floats": (_sz, [C.POINTER(gvx_bigvgan_dims)]),
    "gvx_bigvgan_workspace_bytes": (_sz, [C.POINTER(gvx_bigvgan_dims), _i, _i]),
    "gvx_bigvgan_pack_weights_device": (_i, [C.POINTER(gvx_bigvgan_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_bigvgan_create": (_i, [C.POINTER(gvx_bigvgan_dims), C.POINTER(_vp)]),
    "gvx_bigvgan_destroy": (None, [_vp]),
    "gvx_bigvgan_bind": (_i, [_vp, _vp]),
    "gvx_bigvgan_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_bigvgan_timing_enable": (_i, [_vp, _i]),
    "gvx_bigvgan_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_dwconv_layernorm": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp]),
    "gvx_istft_head_workspace_bytes": (_sz, [_i, _i, _i]),
    "gvx_istft_head": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gvx_vocos_blob_floats": (_sz, [C.POINTER(gvx_vocos_dims)]),
    "gvx_vocos_workspace_bytes": (_sz, [C.POINTER(gvx_vocos_dims), _i, _i]),
    "gvx_vocos_pack_weights_device": (_i, [C.POINTER(gvx_vocos_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_vocos_create": (_i, [C.POINTER(gvx_vocos_dims), C.POINTER(_vp)]),
    "gvx_vocos_destroy": (None, [_vp]),
    "gvx_vocos_bind": (_i, [_vp, _vp]),
    "gvx_vocos_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_vocos_timing_enable": (_i, [_vp, _i]),
    "gvx_vocos_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_dwconv_layernorm_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gvx_dwconv_layernorm_backward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gvx_istft_head_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "gvx_istft_head_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _vp]),
    "gvx_vocos_tape_bytes": (_sz, [C.POINTER(gvx_vocos_dims), _i, _i]),
    "gvx_vocos_tape_layout": (_i, [C.POINTER(gvx_vocos_dims), _i, _i, C.POINTER(gvx_vocos_tape_entry), _i]),
    "gvx_vocos_backward_workspace_bytes": (_sz, [C.POINTER(gvx_vocos_dims), _i, _i]),
    "gvx_vocos_forward_train": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gvx_vocos_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, C.POINTER(gvx_weight_desc), _i, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_vocos_backward_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_self_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "gvx_add_layer_norm": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "gvx_fastpitch_blob_floats": (_sz, [C.POINTER(gvx_fastpitch_dims)]),
    "gvx_fastpitch_workspace_bytes": (_sz, [C.POINTER(gvx_fastpitch_dims), _i, _i]),
    "gvx_fastpitch_pack_weights_device": (_i, [C.POINTER(gvx_fastpitch_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_fastpitch_create": (_i, [C.POINTER(gvx_fastpitch_dims), C.POINTER(_vp)]),
    "gvx_fastpitch_destroy": (None, [_vp]),
    "gvx_fastpitch_bind": (_i, [_vp, _vp]),
    "gvx_fastpitch_encode": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_fastpitch_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_fastpitch_timing_enable": (_i, [_vp, _i]),
    "gvx_fastpitch_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_lvc_gated": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "gvx_univnet_blob_floats": (_sz, [C.POINTER(gvx_univnet_dims)]),
    "gvx_univnet_workspace_bytes": (_sz, [C.POINTER(gvx_univnet_dims), _i, _i]),
    "gvx_univnet_pack_weights_device": (_i, [C.POINTER(gvx_univnet_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_univnet_create": (_i, [C.POINTER(gvx_univnet_dims), C.POINTER(_vp)]),
    "gvx_univnet_destroy": (None, [_vp]),
    "gvx_univnet_bind": (_i, [_vp, _vp]),
    "gvx_univnet_forward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "gvx_univnet_timing_enable": (_i, [_vp, _i]),
    "gvx_univnet_stage_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "gvx_hifigan_mpd_blob_floats": (_sz, [C.POINTER(gvx_hifigan_mpd_dims)]),
    "gvx_hifigan_mpd_pack_weights_device": (_i, [C.POINTER(gvx_hifigan_mpd_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_hifigan_mpd_create": (_i, [C.POINTER(gvx_hifigan_mpd_dims), C.POINTER(_vp)]),
    "gvx_hifigan_mpd_destroy": (None, [_vp]),
    "gvx_hifigan_mpd_bind": (_i, [_vp, _vp]),
    "gvx_hifigan_mpd_layout": (_i, [C.POINTER(gvx_hifigan_mpd_dims), _i, _i, C.POINTER(gvx_hifigan_mpd_entry), _i]),
    "gvx_hifigan_mpd_features_bytes": (_sz, [C.POINTER(gvx_hifigan_mpd_dims), _i, _i]),
    "gvx_hifigan_mpd_workspace_bytes": (_sz, [C.POINTER(gvx_hifigan_mpd_dims), _i, _i, _i]),
    "gvx_hifigan_mpd_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "gvx_hifigan_mpd_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_hifigan_mpd_timing_enable": (_i, [_vp, _i]),
    "gvx_hifigan_mpd_layer_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "gvx_mrd_blob_floats": (_sz, [C.POINTER(gvx_mrd_dims)]),
    "gvx_mrd_pack_weights_device": (_i, [C.POINTER(gvx_mrd_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_mrd_create": (_i, [C.POINTER(gvx_mrd_dims), C.POINTER(_vp)]),
    "gvx_mrd_destroy": (None, [_vp]),
    "gvx_mrd_bind": (_i, [_vp, _vp]),
    "gvx_mrd_layout": (_i, [C.POINTER(gvx_mrd_dims), _i, _i, C.POINTER(gvx_mrd_entry), _i]),
    "gvx_mrd_features_bytes": (_sz, [C.POINTER(gvx_mrd_dims), _i, _i]),
    "gvx_mrd_workspace_bytes": (_sz, [C.POINTER(gvx_mrd_dims), _i, _i, _i]),
    "gvx_mrd_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "gvx_mrd_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_mrd_timing_enable": (_i, [_vp, _i]),
    "gvx_mrd_layer_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "gvx_hifigan_msd_blob_floats": (_sz, [C.POINTER(gvx_hifigan_msd_dims)]),
    "gvx_hifigan_msd_pack_weights_device": (_i, [C.POINTER(gvx_hifigan_msd_dims), C.POINTER(gvx_weight_desc), _i, _vp, _vp]),
    "gvx_hifigan_msd_create": (_i, [C.POINTER(gvx_hifigan_msd_dims), C.POINTER(_vp)]),
    "gvx_hifigan_msd_destroy": (None, [_vp]),
    "gvx_hifigan_msd_bind": (_i, [_vp, _vp]),
    "gvx_hifigan_msd_layout": (_i, [C.POINTER(gvx_hifigan_msd_dims), _i, _i, C.POINTER(gvx_hifigan_msd_entry), _i]),
    "gvx_hifigan_msd_features_bytes": (_sz, [C.POINTER(gvx_hifigan_msd_dims), _i, _i]),
    "gvx_hifigan_msd_workspace_bytes": (_sz, [C.POINTER(gvx_hifigan_msd_dims), _i, _i, _i]),
    "gvx_hifigan_msd_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "gvx_hifigan_msd_backward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, C.POINTER(gvx_weight_desc), _i, _vp, _vp, _sz, _vp]),
    "gvx_hifigan_msd_timing_enable": (_i, [_vp, _i]),
    "gvx_hifigan_msd_layer_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "gvx_stft_loss_create": (_i, [C.POINTER(gvx_stft_resolution), _i, _f, _f, _f, C.POINTER(_vp)]),
    "gvx_stft_loss_destroy": (None, [_vp]),
    "gvx_stft_loss_workspace_bytes": (_sz, [_vp, _i, _l]),
    "gvx_stft_loss": (_i, [_vp, _vp, _vp, _vp, _i, _l, _vp, _vp, _vp, C.POINTER(gvx_stft_loss_debug), _vp, _sz, _vp]),
    "gvx_mel_loss_create": (_i, [_i, _i, _i, _i, _vp, _f, _f, C.POINTER(_vp)]),
    "gvx_mel_loss_destroy": (None, [_vp]),
    "gvx_mel_loss_bands": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "gvx_mel_loss_workspace_bytes": (_sz, [_vp, _i, _l]),
    "gvx_mel_loss": (_i, [_vp, _vp, _vp, _vp, _i, _l, _vp, _vp, _vp, C.POINTER(gvx_mel_loss_debug), _vp, _sz, _vp]),
    "gvx_denoise_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "gvx_denoise_destroy": (None, [_vp]),
    "gvx_denoise_workspace_bytes": (_sz, [_vp, _i, _l]),
    "gvx_denoise": (_i, [_vp, _vp, _vp, _i, _l, _vp, _f, _vp, _vp, _vp, _sz, _vp]),
    "gvx_kernel_timing_enable": (_i, [_vp, _i]),
    "gvx_model_set_persistent_attention": (_i, [_vp, _i]),
    "gvx_model_set_resident_kernels": (_i, [_vp, _i]),
    "gvx_model_set_winograd": (_i, [_vp, _i]),
    "gvx_debug_conv_plan": (_i, [_vp, _i, _i, _i]),
    "gvx_teacher_forced_rows_per_call": (_i, [_vp, _i]),
    "gvx_teacher_forced_resident": (_i, [_vp, _i, _i]),
    "gvx_teacher_forced_loop_kind": (_i, [_vp, _i, _i]),
    "gvx_autoregressive_loop_kind": (_i, [_vp, _i, _i]),
    "gvx_autoregressive_windowed_loop_kind": (_i, [_vp, _i, _i]),
    "gvx_kernel_times_ms": (_i, [_vp, C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library once; raise ImportError with the build recipe if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the gfx950 library first (python -m genvox_amd.build, or "
            f"__graft_entry__.build()). genvox_amd has no CPU or eager fallback.")
    # torch ships its own libamdhip64; it must be the one already loaded when this library's dependency on the HIP
    # runtime is resolved, otherwise the process ends up with two runtimes and device pointers / streams do not mix.
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().gvx_last_error()
        raise GvxError(f"genvox_amd error {rc}: {msg.decode() if msg else '?'}")
