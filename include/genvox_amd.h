/*
 * genvox_amd.h — C ABI of the MI355X (gfx950) Tacotron2 text->mel forward path and the
 * batched Griffin-Lim vocoder.
 *
 * The reference (saiakarsh193/GenVox) has no FFI/operator layer: its boundary for this
 * path is the Python class surface.  This header is the boundary a
 * native replacement exposes underneath that surface; every entry point names the
 * reference function it replaces (paths relative to the reference root).  The Python
 * mirror in genvox_amd/ binds these with ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.
 *  - Unless a parameter says "host", every pointer is a DEVICE pointer (e.g. tensor.data_ptr()
 *    of a PyTorch-ROCm tensor).  Outputs and workspaces are caller-allocated; nothing is
 *    retained after a call returns except the blob pointer given to gvx_model_bind_blob and
 *    cached hipGraphs of the step loops, which reference the workspace and the blob by address
 *    (keyed by both; re-binding a blob drops them).
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *    Calls enqueue work and return; they do not synchronise unless stated.
 *  - Every int-returning call returns GVX_OK (0) or a negative gvx_status;
 *    gvx_last_error() gives the message for the calling thread.
 *  - A gvx_model handle is not thread-safe; distinct handles may be used concurrently.
 *  - All floating point data is fp32 (the reference's dtype).  Channel dims must be
 *    multiples of 8 (GVX_ERR_UNSUPPORTED otherwise).
 *  - Workspaces and scratch.  Every `workspace`, `saved`, `scratch` and `scratch_B` argument is memory the CALLER owns and the
 *    library only borrows for the call (and for the replays of a graph captured over it).  What the caller owes:
 *      * a model workspace (the ones sized by gvx_workspace_bytes, gvx_workspace_bytes_autoregressive and
 *        gvx_postnet_workspace_bytes): its first GVX_WORKSPACE_CLEAR_BYTES bytes are zeroed ONCE, before the first call that
 *        sees the buffer.  They hold the sticky status words of gvx_workspace_status (bytes 0 .. 11), which the kernels only
 *        ever raise and gvx_workspace_status clears, and the hand-off time-out word of the call in flight (bytes 12800 ..
 *        12803).  That word is NOT sticky: every decoder loop and every resident encoder launch zeroes it at its start and
 *        copies it into status word [1] at its end; the caller's clear of it only matters to a gvx_workspace_status that runs
 *        before any such call has, so do not look for a status there.  Clearing more is harmless (the host mirror clears
 *        64 KiB); clearing the front again later loses a status that was not read yet;
 *      * nothing else.  Every other byte of a model workspace, and every byte of any other workspace, `saved` buffer or
 *        scratch, may hold ANY bit pattern when a call starts - NaN, the leftovers of a call of another shape, of another
 *        entry point or of another handle.  Each call clears what it accumulates into, inside the call and inside the graph
 *        it captures, and reads no byte it (or, for `saved`, the matching forward call) has not written.
 *    What the library owes: no call writes outside [buffer, buffer + declared bytes), where the declared bytes are the
 *    `*_bytes` argument (for scratch arguments without one: what the matching size query or the parameter's comment states).
 *    A buffer smaller than the size query for the call's shape - by one byte - is GVX_ERR_WORKSPACE, checked before anything is
 *    launched or written; so is a NULL or misaligned one (256 bytes for workspaces and `saved`, 8 for the float64 scratches).
 *    The layout inside a workspace is a function of the call's shape: a buffer that served one shape serves any other shape
 *    it is large enough for, but sizes are NOT monotone in B or L (a region exists only where the shape's plan uses it), so
 *    "large enough" is only ever established by calling the size query for the shape at hand.
 */
#ifndef GENVOX_AMD_H
#define GENVOX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gvx_status {
    GVX_OK = 0,
    GVX_ERR_INVALID_ARG = -1,
    GVX_ERR_UNSUPPORTED = -2,
    GVX_ERR_MISSING_WEIGHT = -3,
    GVX_ERR_SHAPE = -4,
    GVX_ERR_WORKSPACE = -5,
    GVX_ERR_HIP = -6,
    GVX_ERR_STATE = -7
} gvx_status;

/* Hyper-parameters that fix tensor shapes.  Mirrors configs/models.py:10-26 (Tacotron2Config),
 * configs/__init__.py:136 (AudioConfig.n_mels) and TextConfig.n_tokens (configs/__init__.py:81). */
typedef struct gvx_dims {
    int32_t n_tokens;          /* embedding rows                                   */
    int32_t embed_dim;         /* symbols_embedding_dim == encoder_embedding_dim   */
    int32_t enc_kernel;        /* encoder_kernel_size (odd)                        */
    int32_t enc_n_conv;        /* encoder_n_convolutions                           */
    int32_t prenet_dim;
    int32_t att_rnn_dim;
    int32_t dec_rnn_dim;
    int32_t att_dim;
    int32_t att_loc_filters;   /* attention_location_n_filters                     */
    int32_t att_loc_kernel;    /* attention_location_kernel_size (odd)             */
    int32_t postnet_dim;       /* postnet_embedding_dim                            */
    int32_t postnet_kernel;    /* postnet_kernel_size (odd)                        */
    int32_t postnet_n_conv;
    int32_t n_mels;
} gvx_dims;

/* One named fp32 tensor of the reference's state_dict (models/tts/tacotron2.py:574-584). */
typedef struct gvx_weight_desc {
    const char* name;      /* e.g. "decoder.attention_rnn.weight_ih"                      */
    const float* data;     /* HOST pointer (DEVICE for gvx_model_pack_weights_device), contiguous row-major */
    int64_t numel;
} gvx_weight_desc;

typedef struct gvx_model gvx_model;

/* Bytes at the front of a model workspace the caller zeroes once before first use (Conventions, "Workspaces and scratch"). */
#define GVX_WORKSPACE_CLEAR_BYTES 12804

const char* gvx_last_error(void);
int gvx_version(void);

/* ---- model handle + weights: replaces Tacotron2.__init__ / load_state_dict
 *      (models/tts/tacotron2.py:417-448, :581-584).
 * gvx_model_pack_weights folds eval-mode BatchNorm into the conv weights, reorders LSTM gate
 * rows and lays the recurrent matrices out in MFMA-fragment order, writing one contiguous
 * blob of gvx_model_blob_bytes() bytes to HOST memory.  The caller copies the blob to the
 * device (or receives it over RCCL, see gvx_model_blob_bytes) and binds it. */
int gvx_model_create(const gvx_dims* dims, gvx_model** out);
void gvx_model_destroy(gvx_model* model);
size_t gvx_model_blob_bytes(const gvx_model* model);
int gvx_model_pack_weights(gvx_model* model, const gvx_weight_desc* table, int n, void* host_blob);
int gvx_model_bind_blob(gvx_model* model, const void* device_blob);
/* The same packing on the device: `table` holds DEVICE pointers (the parameters where training updates them in place),
 * device_blob receives exactly the bytes gvx_model_pack_weights would produce.  The first call with a given list of
 * (name, numel) builds a gather map - by running the host packer over index-coded stand-ins - and keeps it in device
 * memory owned by the handle (5 bytes per blob float); later calls are one gather launch plus the BatchNorm folds and
 * bias sums.  This is what a training loop calls after every optimizer step (the host packer takes 80 ms per call). */
int gvx_model_pack_weights_device(gvx_model* model, const gvx_weight_desc* table, int n, void* device_blob, void* stream);

/* Bytes of scratch the calls below need for batch B, L tokens and up to T frames.  gvx_workspace_bytes covers every call;
 * gvx_workspace_bytes_autoregressive is the (smaller) amount gvx_encoder_forward + gvx_decoder_autoregressive +
 * gvx_postnet_forward need for max_steps frames (it leaves out the per-step buffers only the teacher-forced loop uses).
 * 0 for B, L or T below 1.  Contents and clearing: Conventions, "Workspaces and scratch" (GVX_WORKSPACE_CLEAR_BYTES once; the
 * rest may hold anything).  Positive multiples of 256 that never shrink with T - and are not monotone in B or L. */
size_t gvx_workspace_bytes(const gvx_model* model, int B, int L, int T);
size_t gvx_workspace_bytes_autoregressive(const gvx_model* model, int B, int L, int max_steps);

/* Device-side status words the kernels raise in the workspace, copied to host_out[2] after synchronising `stream`.  Both
 * are STICKY: they accumulate over every call made with this workspace since the last gvx_workspace_status, which clears them.
 *   [0] != 0: a token id was outside [0, n_tokens) (the reference's nn.Embedding raises IndexError there,
 *             models/tts/tacotron2.py:459; the row is embedded as zeros here) in some gvx_encoder_forward /
 *             gvx_tacotron2_forward call;
 *   [1] != 0: a bounded in-launch wait of a teacher-forced decoder loop gave up (the attention kernel that runs
 *             beside the LSTM launches and those launches hand the query / context over through counters in the
 *             workspace; a wait that is not served within a few hundred ms raises the call's time-out word and every
 *             kernel drains).  The outputs of such a call are NOT results and do not look like results: the call's
 *             last launch overwrites all of them (mel, mel_post, gate, alignments) with NaN.  It cannot happen while
 *             the two kernels run concurrently; the library switches the resident kernel off when the process runs
 *             under AMD_SERIALIZE_KERNEL / HIP_LAUNCH_BLOCKING.
 * Costs a stream synchronisation: meant for tests and for one check after a batch of calls, not for every call. */
int gvx_workspace_status(const gvx_model* model, void* workspace, size_t workspace_bytes, void* stream, int32_t* host_out);

/* Teacher-forced decoder loop: run the attention as ONE kernel that lives beside the step launches (default, used when the
 * shape allows it: B <= 32, L <= 128, default layer sizes) or as a launch per step (enable = 0).  Callers that drive one
 * handle from two streams at once (the host mirror does that for batches above 32 rows) must switch it off: the
 * resident kernel owns the handle's side stream for the whole loop.  Results are identical either way.
 * enable = 0 also marks the handle as one that shares the GPU with concurrent calls: the autoregressive loop then keeps its
 * attention step a launch of its own instead of running it beside 256 partial-sum tiles (two such launches at once queue
 * behind one another); results equal to fp32 rounding (the h_a columns are added in a different order). */
int gvx_model_set_persistent_attention(gvx_model* model, int enable);

/* enable = 0: no kernel of this handle waits for another one inside a launch any more - the encoder recurrence becomes a launch
 * per position, the teacher-forced decoder loop a launch pair per step (no resident attention / decoder kernel).  Same results
 * (to fp32 rounding), slower.  What a caller switches to when a call came back with the hand-off time-out status (NaN outputs,
 * gvx_workspace_status): the resident kernels could not run at the same time on this GPU (CU masking, a serialising profiler, a
 * co-tenant holding CUs) - the host mirror does exactly this and runs the call again (genvox_amd/tacotron2.py, forward(strict=True)).
 * enable = 1 restores the defaults (environment knobs are not re-read). */
int gvx_model_set_resident_kernels(gvx_model* model, int enable);

/* Postnet and encoder convolutions with as many input as output channels and 5 taps (Postnet layers 2-4 and the three encoder
 * layers of the default model) may run as Winograd F(4,5) along time: 8 instead of 20 fp32 products per 4 output frames, against
 * weights transformed when they are packed.  mode 0 = never (every layer the direct implicit GEMM), 1 = by the layer's shape
 * (default: 256 channels and more), 2 = every layer whose shape the form supports (channels a multiple of 32).  The choice
 * depends on (cin, cout, k) alone, never on B, L, T or the lengths, so a row's result does not depend on the batch it runs in.
 * Results differ from the direct form by fp32 rounding only (a few 1e-6 at the layers' output scale).  The environment variable
 * GVX_CONV_WINOGRAD sets the mode a handle starts with.  Workspace sizes do not depend on the mode.  The training forward's
 * convolutions (batch statistics) are not affected. */
int gvx_model_set_winograd(gvx_model* model, int mode);
/* 1 if a Postnet or encoder convolution of this shape runs as Winograd F(4,5) on this handle, 0 if as the direct implicit GEMM,
 * -1 for a null handle or a non-positive size.  Host arithmetic: the question the Postnet and the encoder themselves ask. */
int gvx_debug_conv_plan(const gvx_model* model, int cin, int cout, int k);

/* Batch rows gvx_tacotron2_forward / gvx_decoder_teacher_forced serve best per call for rows of L tokens: 64 where the 64-row
 * loop beside the resident attention kernel applies (default layer sizes, L <= 128, resident attention enabled: one pass over
 * the recurrent weights per step for all 64 rows), else 32 (callers with more rows run 32-row chunks - in turn where gvx_teacher_forced_resident says 1, else on two streams with a
 * handle each, as the host mirror does).  Any B in [1, 64] is accepted by every call regardless. */
int gvx_teacher_forced_rows_per_call(const gvx_model* model, int L);

/* 1 if a teacher-forced call with B rows of L tokens runs its decoder loop beside the resident attention kernel (the fast path:
 * such chunks are best run one after the other on one stream - 2 x 18.7 ms for 64 x 800 frames against 39.3 ms as two
 * concurrent lanes of launch-per-step loops), 0 if it takes a launch per attention step (chunks then gain from two streams). */
int gvx_teacher_forced_resident(const gvx_model* model, int B, int L);

/* How the decoder loop of a teacher-forced inference call with B rows of L tokens runs (models/tts/tacotron2.py:365-388):
 * 2 = ONE resident weight-stationary kernel for all T steps beside the resident attention kernel (dec_resident.hip: default layer
 *     sizes, B <= 32, L <= 128; the LSTM matrices stay in registers and LDS, hand-offs by flags),
 * 1 = one weight-streaming launch per step beside the resident attention kernel, 0 = a launch pair per step. */
int gvx_teacher_forced_loop_kind(const gvx_model* model, int B, int L);

/* How an autoregressive call with B rows of L tokens runs its decode (models/tts/tacotron2.py:390-413 Decoder.inference):
 * 2 = TWO resident kernels for the whole decode (dec_resident.hip decoder_ar_resident_kernel beside attn_persist.hip's rows, which
 *     also sum the frame, test the stop token and run Prenet layer 1; default layer sizes, B <= 32, L <= 128, the handle does not
 *     share the chip): no launch per step, the kernels end the loop themselves,
 * 1 = launches per step beside the resident attention kernel (opt-in, GVX_AR_RESIDENT=1), 0 = launches per step. */
int gvx_autoregressive_loop_kind(const gvx_model* model, int B, int L);
/* ... and how gvx_decoder_autoregressive_windowed runs it.  The resident pair applies the window where one attention workgroup
 * holds a row (L <= 128): 2 there; every other shape - rows of 129-256 tokens, GVX_AR_RESIDENT=1 handles - takes the launches
 * per step, 0, whose attention step applies it.  Never 1. */
int gvx_autoregressive_windowed_loop_kind(const gvx_model* model, int B, int L);

/* ---- Encoder: embedding + conv/BN/relu stack + BiLSTM with packed-sequence semantics.
 * Replaces nn.Embedding + Encoder.forward / Encoder.inference (models/tts/tacotron2.py:459,
 * :231-246, :248-256).  tokens: int64 [B, L]; lengths: int32 [B] or NULL (= all L);
 * memory_out: [B, L, embed_dim], zero past each row's length.
 * For B <= 32 and the default layer sizes the recurrence (:239-245) is ONE resident launch whose 64 workgroups hand the hidden
 * state round through the workspace (bounded waits: a time-out leaves NaN in memory_out and raises status word [1] of
 * gvx_workspace_status); other shapes run a launch per token position.  Same results to fp32 rounding. */
int gvx_encoder_forward(gvx_model* model, const int64_t* tokens, const int32_t* lengths, int B, int L,
                        float* memory_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Teacher-forced decoder: Prenet over all frames, T x (attention LSTM, location-sensitive
 * attention, decoder LSTM), mel/gate projection.  Replaces Decoder.forward
 * (models/tts/tacotron2.py:365-388; decode :333-363; Attention :89-129; Prenet :140-144).
 * memory: [B, L, embed_dim]; lengths: int32 [B] or NULL; mel_in: [B, n_mels, T];
 * keep_masks: uint8 {0,1} [2, (T+1)*B, prenet_dim], row = t*B + b (the two Prenet dropout keep masks);
 * mel_out: [B, n_mels, T]; gate_out: [B, T] (logits); align_out: [B, T, L]. */
int gvx_decoder_teacher_forced(gvx_model* model, const float* memory, const int32_t* lengths, int B, int L,
                               const float* mel_in, int T, const uint8_t* keep_masks,
                               float* mel_out, float* gate_out, float* align_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- Autoregressive decoder, batched.  Replaces Decoder.inference (models/tts/tacotron2.py:390-414),
 * which is batch-1 only; here every row stops on its own: n_frames_out[b] = index of the first step
 * whose sigmoid(gate) > gate_threshold, plus one (or max_steps).  Frames past n_frames_out[b] carry the
 * reference's padding values (mel 0, gate 1e3, alignment 0; mask_padding, :466-473).  keep_masks: uint8 [2, max_steps, B, prenet_dim].  Outputs are sized for max_steps:
 * mel_out [B, n_mels, max_steps], gate_out [B, max_steps], align_out [B, max_steps, L].
 * This call synchronises the stream (it polls the all-rows-finished flag between step chunks).
 * steps_run_out (HOST int) receives the number of steps actually executed. */
int gvx_decoder_autoregressive(gvx_model* model, const float* memory, const int32_t* lengths, int B, int L,
                               int max_steps, float gate_threshold, const uint8_t* keep_masks,
                               float* mel_out, float* gate_out, float* align_out, int32_t* n_frames_out,
                               int* steps_run_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- The same decode with a monotonic attention window: the softmax of every step only sees the tokens near the one the
 * previous step attended most, so a decode cannot skip, repeat or wander by more than the window allows.  Not in the reference;
 * an inference-time device only (teacher-forced and training calls have none).
 *   Row b has a centre c_b(t), c_b(0) = 0.  At step t position l takes part in the softmax iff l < lengths[b] and
 *   c_b(t) - window_back <= l <= c_b(t) + window_ahead; every other position has energy -inf and weight exactly 0.
 *   c_b(t+1) = the lowest index at which the weights of step t are largest (the tie rule of gvx_alignment_stats' positions), so a
 *   centre is always inside its own window and below lengths[b]: no softmax is empty.
 * The cumulative weights, the location features and the context use the windowed weights; nothing else in the step changes, and
 * a window that covers the whole row gives gvx_decoder_autoregressive's mel, gate and alignments bit for bit where both calls
 * take the same loop kind (gvx_autoregressive_windowed_loop_kind / gvx_autoregressive_loop_kind).
 * centres_out: device int32 [B, max_steps], mandatory - it is also where the decode keeps the centres between the steps of the
 * launch-per-step loop (no workspace bytes are added; contents on entry do not matter).  On return centres_out[b][t] = c_b(t+1)
 * for t < n_frames_out[b] and -1 behind: what gvx_alignment_stats gives as positions for the same alignments.  If a hand-off of
 * the resident kernels timed out (gvx_workspace_status), every entry is INT32_MIN beside the NaN outputs.
 * window_back / window_ahead < 0 or centres_out == NULL: GVX_ERR_INVALID_ARG, nothing is launched.  Every other argument, the
 * workspace size and the synchronisation are those of gvx_decoder_autoregressive, which this call leaves as it was. */
int gvx_decoder_autoregressive_windowed(gvx_model* model, const float* memory, const int32_t* lengths, int B, int L,
                                        int max_steps, float gate_threshold, const uint8_t* keep_masks,
                                        float* mel_out, float* gate_out, float* align_out, int32_t* n_frames_out,
                                        int* steps_run_out, void* workspace, size_t workspace_bytes, void* stream,
                                        int window_back, int window_ahead, int32_t* centres_out);

/* ---- Postnet + residual: mel_post_out = mel_in + Postnet(mel_in).  Replaces Postnet.forward and the
 * residual add (models/tts/tacotron2.py:194-200, :464/:491).  Tensors are [B, n_mels, T]; any B (GEMM-only
 * path, no per-call batch limit).  mel_lengths: int32 [B] or NULL.  With lengths, row b is processed as a
 * sequence of mel_lengths[b] frames (the convolutions see zeros from that frame on, as a batch-1 run of the
 * reference sees its zero padding) and mel_post_out is 0 there.  The workspace needs
 * gvx_postnet_workspace_bytes(B, T) bytes (a gvx_workspace_bytes(B, L, T) workspace is always large enough); a model workspace
 * in the sense of the Conventions ("Workspaces and scratch"): GVX_WORKSPACE_CLEAR_BYTES zeroed once, the rest may hold anything. */
size_t gvx_postnet_workspace_bytes(const gvx_model* model, int B, int T);
int gvx_postnet_forward(gvx_model* model, const float* mel_in, const int32_t* mel_lengths, int B, int T, float* mel_post_out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- Output padding mask (models/tts/tacotron2.py:466-473): frames >= mel_lengths[b] get
 * mel = 0, mel_post = 0, gate = 1e3.  mel_lengths: int32 [B], each >= 0 (0 masks the whole row, T or more nothing). In place;
 * live frames are not touched.  mel, mel_post and gate may each be NULL: that tensor is skipped. */
int gvx_mask_padding(float* mel, float* mel_post, float* gate, const int32_t* mel_lengths,
                     int B, int n_mels, int T, void* stream);

/* ---- Whole teacher-forced forward in one call (what Tacotron2.forward does, models/tts/tacotron2.py:450-481).
 * mel_lengths may be NULL (no padding mask).  mel_post_out may be NULL: the call then ends behind the mel / gate projection
 * (mel_out, gate_out, align_out unmasked) and the caller runs gvx_postnet_forward + gvx_mask_padding itself - once over all
 * 32-row chunks of a larger batch, for instance. */
int gvx_tacotron2_forward(gvx_model* model, const int64_t* tokens, const int32_t* token_lengths, int B, int L,
                          const float* mel_in, const int32_t* mel_lengths, int T, const uint8_t* keep_masks,
                          float* mel_out, float* mel_post_out, float* gate_out, float* align_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- Criterion of the evaluation step.  Replaces Tacotron2Loss (models/tts/tacotron2.py:598-615) as called by
 * Tacotron2.eval_step (:524-529): loss_out[3] (device) = {loss, mel_loss, gate_loss} with
 *   mel_loss = mean((mel_out - mel_target)^2) + mean((mel_post_out - mel_target)^2)   over all B*n_mels*T elements,
 *   gate_loss = mean(BCE-with-logits(gate_out, gate_target))                          over all B*T elements,
 *   loss = mel_loss + gate_loss.
 * All tensors are the [B, n_mels, T] / [B, T] device arrays of the forward call; forward only (no gradients).
 * scratch: >= 6144 bytes of device memory, 8-byte aligned (float64 partial sums of the two-stage reduction); it may hold
 * anything and needs no clearing (Conventions, "Workspaces and scratch"); 6143 bytes are GVX_ERR_WORKSPACE. */
int gvx_tacotron2_loss(const float* mel_out, const float* mel_post_out, const float* gate_out, const float* mel_target,
                       const float* gate_target, int B, int n_mels, int T, float* loss_out, void* scratch, size_t scratch_bytes,
                       void* stream);

/* =====================================================================================================
 * Training: the convolution layers of the encoder and Postnet stacks as the
 * reference runs them under .train() - nn.Conv1d + nn.BatchNorm1d with BATCH statistics + activation + F.dropout
 * (models/tts/tacotron2.py:149-199, :207-220, :234-235) - forward and backward, and the backward of Tacotron2Loss
 * (:598-615).  Parameters are taken in the reference's own layout (conv weight [Cout, Cin, k]); activations in its
 * [B, C, T] layout.  act: 0 none, 1 relu, 2 tanh.  keep: uint8 {0,1} [B, Cout, T] (the dropout's keep mask; NULL = no
 * dropout); kept values are scaled by 1 / (1 - p).  Channels must be multiples of 8, k odd.
 * `saved` carries what the backward needs (gvx_conv_train_saved_bytes); both buffers 256-byte aligned.
 * Together with the BPTT primitives further down these make up Tacotron2.train_step of the host mirror
 * (genvox_amd/tacotron2.py, genvox_amd/training.py), which is pinned to the reference's own train_step.
 * ===================================================================================================== */
/* The rest of the training-mode FORWARD (models/tts/tacotron2.py:231-246, :333-363 under .train()): the encoder's BiLSTM on
 * the output of its training-mode convolution stack (conv_out [B, embed_dim, L], reference layout), and the teacher-forced
 * decoder with dropout on the hidden outputs of both LSTM cells (att_keep uint8 [T, B, att_rnn_dim], dec_keep uint8
 * [T, B, dec_rnn_dim]; kept values scaled by 1 / (1 - p); the dropped state is what the next step, the attention query, the
 * other cell and the projection see).  Both read the LSTM / attention / Prenet / projection weights from the bound blob. */
/* Tape outputs (each may be NULL) are what back-propagation through time reads:
 *   cell_states_out [B, L, embed_dim]   the BiLSTM's cell state at every position (forward direction in the first half of
 *                                       the channels, like memory_out), zeros past a row's length;
 *   input_preact_out [B, L, 2 * 4H]     W_ih x + b_ih + b_hh of both directions, gate rows in the library's packed order
 *                                       (row 4 j + gate);
 *   att_hidden_all [T+1][A/8][B][8]     the attention LSTM's dropped hidden state after every step (slot t + 1; slot 0 zeros)
 *                                       as k-group-blocked vectors: element (b, k) at (k / 8) * B * 8 + b * 8 + k % 8;
 *   att_cell_all, dec_cell_all [T+1][B][H]   both cells' states (slot t + 1 = after step t);
 *   dec_hidden_context_all [T+1][(D+E)/8][B][8]   [h_d ; ctx] after every step, blocked as above;
 *   att_preact_all [T][B][A][4], dec_preact_all [T][B][D][4]   gate pre-activations i, f, g, o of every unit and step.
 * gvx_decoder_teacher_forced_train on a handle created under GVX_TF_ROWS64=1 takes at most 32 rows per call where 33 .. 64 rows
 * would run on the 64-row loop (which has neither the dropout nor the tape): GVX_ERR_UNSUPPORTED, nothing written. */
int gvx_encoder_lstm_forward(gvx_model* model, const float* conv_out, const int32_t* lengths, int B, int L, float* memory_out,
                             float* cell_states_out, float* input_preact_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_decoder_teacher_forced_train(gvx_model* model, const float* memory, const int32_t* lengths, int B, int L, const float* mel_in,
                                     int T, const uint8_t* keep_masks, const uint8_t* att_keep, const uint8_t* dec_keep, float p_att,
                                     float p_dec, float* mel_out, float* gate_out, float* align_out, float* att_hidden_all,
                                     float* att_cell_all, float* dec_cell_all, float* dec_hidden_context_all, float* att_preact_all,
                                     float* dec_preact_all, void* workspace, size_t workspace_bytes, void* stream);
/* Copy one of the decoder's per-call buffers out of the workspace of the last gvx_decoder_teacher_forced(_train) call with the
 * same (B, L, T), row-major: what 0 = decoder input frames [(T+1) B, n_mels] (row t B + b; frame 0 = zeros), 1 = Prenet layer-1
 * output [(T+1) B, prenet_dim], 2 = Prenet output [(T+1) B, prenet_dim], 3 = processed memory [B, L, att_dim];
 * 4 = the encoder output [B, L, embed_dim] of the last gvx_tacotron2_forward of that shape (a Postnet of many frames takes the
 * region as scratch: read it behind a call with mel_post_out = NULL). */
int gvx_train_export(const gvx_model* model, const void* workspace, size_t workspace_bytes, int B, int L, int T, int what, float* dst, void* stream);
/* `saved` and the workspace of the two calls below: no clearing, any contents (Conventions, "Workspaces and scratch"); the backward
 * reads of `saved` only what the forward of the same shape wrote there. */
size_t gvx_conv_train_saved_bytes(int B, int Cin, int Cout, int T, int k);
size_t gvx_conv_train_workspace_bytes(int B, int Cin, int Cout, int T, int k);
/* y = dropout(act(BatchNorm_train(conv1d(x, w, bias, padding (k-1)/2)))).  running_mean / running_var (may be NULL) get the
 * momentum-0.1 update of torch.nn.BatchNorm1d (unbiased variance), in place.
 * One value per channel (B * T == 1), where torch.nn.BatchNorm1d raises: the batch variance is 0 and the normalised value 0,
 * so y = dropout(act(beta)), running_mean moves towards the one value and running_var is multiplied by 0.9 (the unbiased
 * variance of one value is taken as 0); the backward then gives dbeta = d loss / d (BatchNorm output) and exact zeros for dx,
 * dw, dbias and dgamma.
 * Both calls and both size queries refuse the same shapes (the queries return 0): GVX_ERR_UNSUPPORTED for B or T < 1, channels
 * that are no positive multiple of 8, an even or non-positive k, B * T above 2^30; GVX_ERR_INVALID_ARG for a NULL argument that
 * may not be NULL, an unknown act, p_drop outside [0, 1) with a mask; GVX_ERR_WORKSPACE for a buffer that is too small or not
 * 256-byte aligned.  Nothing is launched then. */
int gvx_conv_bn_act_train_forward(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, int B, int Cin, int Cout, int T, int k, int act,
                                  const uint8_t* keep, float p_drop, float* y, void* saved, size_t saved_bytes, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* Gradients of one layer given dy = d loss / d y: dx [B, Cin, T] (may be NULL), dw [Cout, Cin, k], dbias, dgamma, dbeta [Cout].
 * x_wgrad (may be NULL): input to use for the weight gradient instead of the saved one - the reference masks the Postnet's
 * input in place after its forward, outside autograd, so its first layer's weight gradient sees the masked tensor. */
int gvx_conv_bn_act_train_backward(const float* dy, const void* saved, size_t saved_bytes, const float* w, const float* gamma,
                                   const float* x_wgrad, int B, int Cin, int Cout, int T, int k, int act, const uint8_t* keep,
                                   float p_drop, float* dx, float* dw, float* dbias, float* dgamma, float* dbeta, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* d loss / d (mel_out [its own MSE term], mel_post_out, gate_out) of Tacotron2Loss on the (masked) outputs of the forward. */
int gvx_tacotron2_loss_backward(const float* mel_out, const float* mel_post_out, const float* gate_out, const float* mel_target,
                                const float* gate_target, int B, int n_mels, int T, float* dmel_out, float* dmel_post_out,
                                float* dgate_out, void* stream);

/* ---- The training step's whole-sequence pieces: primitives the host mirror (genvox_amd/training.py) strings together as
 * oracle/train_ref.py states them (the reference: loss.backward(), clip_grad_norm_, Adam.step, models/tts/tacotron2.py:515-522);
 * the two recurrences are single calls (gvx_train_decoder_bptt, gvx_train_encoder_lstm_bptt below).  Row-major fp32 with
 * explicit leading dimensions; LSTM gates in torch order i, f, g, o. */
/* C[m][n] = sum_k A[m * lda + k] W[n * ldw + k] (+ bias[n]), K % 4 == 0.  scratch (may be NULL): device scratch for split-K
 * partial tiles, used when the product has few output tiles and a long K.  It may hold anything; the call writes at most
 * scratch_bytes of it and takes fewer K pieces (down to no split) when it is small: a short scratch is no error here. */
int gvx_train_gemm_nt(const float* A, long lda, const float* W, long ldw, float* C, long ldc, int M, int N, int K, const float* bias,
                      float* scratch, size_t scratch_bytes, void* stream);
/* C[m][n] = sum_r A[r * lda + m] Bm[r * ldb + n] (a weight gradient: the sum over the rows of two activation matrices, no
 * transposed copies). */
int gvx_train_gemm_tn(const float* A, long lda, const float* Bm, long ldb, float* C, long ldc, int M, int N, long rows, float* scratch,
                      size_t scratch_bytes, void* stream);
int gvx_train_transpose(const float* src, long ld_src, float* dst, long rows, int cols, long rows_padded, void* stream);
int gvx_train_colsum(const float* X, long rows, int C, float* out, void* stream);
int gvx_train_axpby(const float* a, long lda, float alpha, const float* b, long ldb, float beta, float* y, long ldy, long rows, int cols, void* stream);
int gvx_train_relu_dropout_backward(const float* dy, const float* act_out, const uint8_t* keep, float scale, long n, float* dz, void* stream);
int gvx_train_unblock(const float* blocked, float* rows_out, long n_slots, int B, int K, void* stream);
int gvx_train_embedding_backward(const int64_t* tokens, const float* dx, long n_tokens_in_batch, int E, int n_rows, float* demb, void* stream);
/* Many tensors per launch (device arrays of references, built by the caller once per step): sum of squares of all of them -
 * the square of clip_grad_norm_'s total norm, added in a fixed order (scratch: gvx_train_sqnorm_scratch_bytes) - and the Adam
 * update of all of them. */
typedef struct gvx_tensor_ref { const float* data; int64_t numel; } gvx_tensor_ref;
typedef struct gvx_adam_ref { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t numel; } gvx_adam_ref;
size_t gvx_train_sqnorm_scratch_bytes(int n_tensors);   /* any contents, no clearing; the call writes exactly these bytes */
int gvx_train_sqnorm_many(const gvx_tensor_ref* refs_device, int n_tensors, double* scratch, double* sumsq_out, void* stream);
int gvx_train_adam_step_many(const gvx_adam_ref* refs_device, int n_tensors, float grad_scale, float lr, float weight_decay, float beta1,
                             float beta2, float eps, int step, void* stream);

/* ---- Back-propagation through the decoder loop in one call (three launches per step issued by the library instead of ~20
 * primitives per step strung together by the host): d loss / d of both LSTM cells' gates at every step, of the attention
 * queries, of the processed memory, of the memory through the contexts, and of v / location_dense / location_conv
 * (Decoder.forward backwards, models/tts/tacotron2.py:365-388 with :333-363 and Attention :89-129).  What is not on the
 * recurrence (weight gradients as whole-sequence products, the Prenet columns of the attention LSTM) stays with the caller.
 * All pointers device, fp32 row-major, gates in torch order i, f, g, o.
 * There is no `lengths` argument: the masking of padded positions rides on w_all, which must be exactly zero at and past a
 * row's length at every step (as a softmax over -inf energies leaves it); dpm and dmemory are then exactly zero there, and
 * memory / pm past the length are never seen in any output.  dpm is cleared by the call, which then accumulates into it; the
 * workspace needs no clearing either.  L is limited by the LDS of the attention launch (160 KiB for a row's chunk: L <= 664
 * at the default layer sizes); the size query returns 0 and the call GVX_ERR_UNSUPPORTED beyond it. */
typedef struct gvx_bptt_decoder_args {
    int32_t B, L, T;                    /* 1 <= B <= 32, L >= 1, T >= 1 */
    int32_t A, D, E, P, a, F, kl;       /* att_rnn_dim, dec_rnn_dim, embed_dim, prenet_dim, att_dim, location filters / kernel size */
    float att_scale, dec_scale;         /* 1 / (1 - p) of the dropout on each cell's hidden output */
    const float* dhc_all;               /* [T][B][D+E]  d loss / d [h_d(t) ; ctx(t)] through the mel / gate projection */
    const float* pre_a;                 /* [T][B][A][4] gate pre-activations of the attention LSTM as the forward's tape holds them */
    const float* pre_d;                 /* [T][B][D][4] ... of the decoder LSTM */
    const float* c_a_all;               /* [T+1][B][A]  cell states, slot t = before step t */
    const float* c_d_all;               /* [T+1][B][D] */
    const uint8_t* att_keep;            /* [T][B][A]    keep masks of the hidden-output dropouts */
    const uint8_t* dec_keep;            /* [T][B][D] */
    const float* q_all;                 /* [T][B][a]    attention queries W_q h_a(t) */
    const float* ctx_all;               /* context of (step t, row b) at ctx_all + t * ctx_ts + b * ctx_bs, E floats */
    int64_t ctx_ts, ctx_bs;
    const float* w_all;                 /* [T][B][L]    alignments, time-major */
    const float* memory;                /* [B][L][E] */
    const float* pm;                    /* [B][L][a]    processed memory */
    const float* w_ih_a; const float* w_hh_a;   /* attention_rnn.weight_ih [4A][P+E], weight_hh [4A][A] */
    const float* w_ih_d; const float* w_hh_d;   /* decoder_rnn.weight_ih [4D][A+E], weight_hh [4D][D] */
    const float* wq;                    /* query_layer weight [a][A] */
    const float* v;                     /* [a] */
    const float* loc_conv;              /* location_conv weight [F][2][kl] */
    const float* loc_dense;             /* location_dense weight [a][F] */
    float* dga_all;                     /* out [T][B][4A]  d loss / d gate pre-activations of the attention LSTM */
    float* dgd_all;                     /* out [T][B][4D] */
    float* dq_all;                      /* out [T][B][a] */
    float* dctx_all;                    /* out [T][B][E]   total d loss / d ctx(t) */
    float* dpm;                         /* out [B][L][a]   cleared by the call */
    float* dmemory;                     /* out [B][L][E]   context path only: sum_t w_t (x) dctx_t */
    float* dv;                          /* out [a] */
    float* dloc_dense;                  /* out [a][F] */
    float* dloc_conv;                   /* out [F][2][kl] */
} gvx_bptt_decoder_args;
size_t gvx_train_decoder_bptt_workspace_bytes(const gvx_bptt_decoder_args* args);   /* any contents, no clearing (Conventions) */
int gvx_train_decoder_bptt(const gvx_bptt_decoder_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* The same call with a gradient taken DIRECTLY on the alignments (a loss that looks at them, such as the guided attention loss
 * below): dw_ext holds d loss / d w_t[b][l], element (t, b, l) at dw_ext + t * dw_ext_ts + b * dw_ext_bs + l (strides in floats,
 * as ctx_all has them: a row slice of a [B][T][L] tensor goes in with ts = L, bs = T L, a time-major array with ts = B L,
 * bs = L; both >= L where T > 1 / B > 1, GVX_ERR_INVALID_ARG otherwise).  The term enters the softmax backward of step t,
 *   de_l = w_l (dctx . memory_l + dw_l - sum_k w_k dw_k),   dw = previous-weights path + cumulative path + dw_ext[t],
 * and nothing else: the location convolution's gradient to earlier steps is that of the energies alone.  Values at and past a
 * row's length are never seen in an output (they meet w = 0) but must be FINITE - 0 x NaN is NaN.  dw_ext == NULL is
 * gvx_train_decoder_bptt, bit for bit; same argument block, workspace size and limits. */
int gvx_train_decoder_bptt_ext(const gvx_bptt_decoder_args* args, const float* dw_ext, int64_t dw_ext_ts, int64_t dw_ext_bs,
                               void* workspace, size_t workspace_bytes, void* stream);
/* ---- Diagonal guided attention loss (Tachibana et al. 2017; masked mean as in ESPnet's Tacotron2 recipe) on the alignments
 * align [B][T][L] of the teacher-forced forward, and its gradient.  With L_b = token_lengths[b], T_b = mel_lengths[b] (device
 * int32, clamped to [0, L] / [0, T]; summed on the device, no host synchronisation) and N = sum_b T_b L_b:
 *   G[b][t][l] = 1 - exp(-(l / L_b - t / T_b)^2 / (2 sigma^2))   for t < T_b and l < L_b,
 *   loss_out[0] = sum G align / N                                (device fp32; WITHOUT alpha),
 *   dalign[b][t][l] = alpha G[b][t][l] / N                       (may be NULL: loss only; the loss is the same either way).
 * Cells outside a row's T_b x L_b are skipped - align may hold anything there, NaN included - and dalign is exactly 0 in them.
 * N = 0 gives loss 0 and a zero gradient.  Every element of dalign is good to 9 x 2^-24 of ITSELF (l / L_b - t / T_b is formed
 * from the exact integer l T_b - t L_b, G as -expm1(-x)) and exactly 0 on a row's diagonal; the sum runs over float64 partials
 * in a fixed order: two calls are bit-equal.  sigma > 0, alpha >= 0, B, T, L >= 1 (GVX_ERR_INVALID_ARG otherwise, also for a NULL
 * pointer other than dalign); scratch: gvx_guided_attention_loss_scratch_bytes, 8-byte aligned (GVX_ERR_WORKSPACE). */
size_t gvx_guided_attention_loss_scratch_bytes(int B, int T, int L);   /* any contents, no clearing (Conventions) */
int gvx_guided_attention_loss(const float* align, const int32_t* token_lengths, const int32_t* mel_lengths, int B, int T, int L,
                              float sigma, float alpha, float* loss_out, float* dalign, void* scratch, size_t scratch_bytes,
                              void* stream);
/* Back-propagation through the encoder BiLSTM (Encoder.forward, models/tts/tacotron2.py:239-245, packed-sequence semantics),
 * one launch per time step for both directions.  xg [2][B][L][4H] = W_ih x + b_ih + b_hh per direction; memory / cell_states /
 * dmemory [B][L][2H] (forward direction in the first H channels); w_hh [2][4H][H].  Outputs, filed under the POSITION a step
 * belongs to (zeros past a row's length): dg_pos [2][B][L][4H] gate gradients, hprev_pos [2][B][L][H] the step's previous
 * hidden state - the operands of the weight gradients and of d loss / d x.  Any B >= 1 (rows beyond 32 take further trips of
 * the kernels' row loop), lengths in [1, L], H a multiple of 8 up to 1280 (LDS). */
size_t gvx_train_encoder_lstm_bptt_workspace_bytes(int B, int H);   /* any contents, no clearing: both calls reset their flag lines and status word */
int gvx_train_encoder_lstm_bptt(const float* xg, const float* memory, const float* cell_states, const float* dmemory, const float* w_hh,
                                const int32_t* lengths, int B, int L, int H, float* dg_pos, float* hprev_pos, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The same walk as ONE resident launch (its workgroups hand the gate gradients of a step round through the workspace; shapes
 * whose workgroups do not all fit on the GPU at once take the launch per step).  Bounded waits: after a time-out - the workgroups
 * could not run at the same time - both outputs are NaN and the workspace's status word holds the code, which
 * gvx_train_encoder_lstm_bptt_status reads (one stream synchronisation; 0 = fine). */
int gvx_train_encoder_lstm_bptt_resident(const float* xg, const float* memory, const float* cell_states, const float* dmemory,
                                         const float* w_hh, const int32_t* lengths, int B, int L, int H, float* dg_pos,
                                         float* hprev_pos, void* workspace, size_t workspace_bytes, void* stream);
int gvx_train_encoder_lstm_bptt_status(const void* workspace, size_t workspace_bytes, int B, int H, int* code_out, void* stream);

/* ---- Prenet keep-mask generator for callers that do not supply masks (the reference draws them from
 * torch's RNG inside F.dropout, models/tts/tacotron2.py:143).  Writes n bytes of Bernoulli(0.5) {0,1}. */
int gvx_prenet_masks_generate(uint8_t* masks_out, size_t n, uint64_t seed, void* stream);

/* ---- Stage timing (measurement only): when enabled, the whole-forward call records HIP events around
 * each stage on `stream`; gvx_stage_times_ms synchronises and returns encoder, prenet, decoder loop,
 * projection, postnet milliseconds of the last call and the number of decoder-step kernel launches. */
int gvx_stage_timing_enable(gvx_model* model, int enable);
int gvx_stage_times_ms(gvx_model* model, float* times5_out, int* decoder_launches_out);

/* =====================================================================================================
 * Vocoder: mel (dB) -> waveform.  Replaces the mel->wav half of utils/audio/base.py and
 * AudioProcessor.convert_mel2wav (core/processors.py:81-96), batched over utterances.
 * Spectrograms use the reference's layout [B][bins][frames] (bins = n_fft/2 + 1); complex values are
 * interleaved (re, im) floats.  `window` is the float32 periodic Hann window [n_fft] (device).
 * A gvx_gl_plan owns the rocFFT plans (one pair per distinct B*T, created on first use).
 * ===================================================================================================== */
typedef struct gvx_gl_plan gvx_gl_plan;
int gvx_gl_plan_create(int n_fft, int hop, gvx_gl_plan** out);
void gvx_gl_plan_destroy(gvx_gl_plan* plan);
/* Bytes every uniform call below needs for B rows of T frames.  n_mels > 0 includes the amplitudes of gvx_mel_to_magnitude /
 * gvx_wav_to_mel and a region of n_mels * ((bins + 3) & ~3) floats for gvx_wav_to_mel's zero-padded mel basis, whose size does
 * not depend on B*T: gvx_wav_to_mel serves any B*T >= 1 (one file of one frame included).  n_mels = 0 sizes the calls that take
 * no mel (gvx_stft, gvx_istft, gvx_griffin_lim). */
size_t gvx_gl_workspace_bytes(gvx_gl_plan* plan, int B, int T, int n_mels);   /* any contents, no clearing (Conventions, "Workspaces and scratch") */

/* stft (utils/audio/base.py:58-69): signal [B][n_samples] -> spec_out complex [B][bins][T], T = (n_samples-n_fft)/hop+1 */
int gvx_stft(gvx_gl_plan* plan, const float* signal, const float* window, int B, long n_samples, float* spec_out,
             void* workspace, size_t workspace_bytes, void* stream);
/* istft (utils/audio/base.py:71-88): spec complex [B][bins][T] -> signal_out [B][n_fft + (T-1)*hop] */
int gvx_istft(gvx_gl_plan* plan, const float* spec, const float* window, int B, int T, float* signal_out,
              void* workspace, size_t workspace_bytes, void* stream);
/* db_to_amplitude + mel2fft (utils/audio/base.py:38-52 with power=False/scale=1, :143-145):
 * mel_db [B][n_mels][T], inv_basis [bins][n_mels] -> mag_out [B][bins][T].  log10_kind: 0 = np.log, 1 = np.log10. */
int gvx_mel_to_magnitude(gvx_gl_plan* plan, const float* mel_db, const float* inv_basis, int B, int n_mels, int T, int log10_kind,
                         float ref, float* mag_out, void* workspace, size_t workspace_bytes, void* stream);
/* fast Griffin-Lim (utils/audio/base.py:147-162) + final synthesis istft(mag * exp(i phase)) (core/processors.py:89-90).
 * mag [B][bins][T]; phase_out [B][bins][T] or NULL; wav_out [B][n_fft + (T-1)*hop] or NULL. */
int gvx_griffin_lim(gvx_gl_plan* plan, const float* mag, const float* window, int B, int T, int n_iter, float momentum,
                    float* phase_out, float* wav_out, void* workspace, size_t workspace_bytes, void* stream);
/* wav -> mel features (AudioProcessor.convert_wav2mel, core/processors.py:70-79: stft, |.|, fft2mel, amplitude_to_db with
 * power=False/scale=1; utils/audio/base.py:24-36, :58-69, :139-141).  signal [B][n_samples] (already normalised),
 * mel_basis [n_mels][bins] -> mel_db_out [B][n_mels][T], T = (n_samples - n_fft)/hop + 1. */
int gvx_wav_to_mel(gvx_gl_plan* plan, const float* signal, const float* window, const float* mel_basis, int B, long n_samples,
                   int n_mels, int log10_kind, float ref, float* mel_db_out, void* workspace, size_t workspace_bytes, void* stream);
/* tail of convert_mel2wav (core/processors.py:91-95): samples with |y| > 1 -> 0, drop `trim` samples at both ends,
 * divide by the peak (float32), IIR filter b/a (HOST doubles, order+1 each; scipy.signal.lfilter semantics, float64).
 * out: float64 [B][n_samples - 2*trim]; scratch_B: B uint32 of device scratch (any contents; the call clears and writes exactly B words). */
int gvx_wav_finalize(const float* wav, int B, long n_samples, int trim, const double* b_coef, const double* a_coef, int order,
                     double* out, unsigned int* scratch_B, void* stream);

/* ---- Ragged batches: the same stages for rows of different lengths in one call.  Buffers keep the strides of the padded T
 * (mag / phase_out [B][bins][T], wav [B][n_fft + (T-1)*hop]); frame_lengths is a DEVICE int32 [B] (the call stays asynchronous
 * on `stream`), row b having T_b = frame_lengths[b] frames and n_b = n_fft + (T_b-1)*hop samples.  The kernels clamp a length to
 * [0, T] rather than trust it; a row of length 0 yields zeros.  frame_lengths == NULL is GVX_ERR_INVALID_ARG (the uniform calls
 * above exist for that).  Row b's result is, to the bit, what the uniform call gives for that row alone at T = T_b: per frame
 * and per sample the same operations in the same order, frames t >= T_b never added, the window sum of squares that divides the
 * row's last n_fft - hop samples that of T_b frames.  Whatever the padded frames of `mag` hold (inf and NaN included) reaches
 * no valid sample.  gvx_mel_to_magnitude is frame-wise and serves ragged batches as it is.
 *
 * gvx_griffin_lim_ragged: phase_out is 0 in frames t >= T_b, wav_out is 0 in samples i >= n_b (inside the workspace the signal
 * behind n_b is left unwritten and never read).  With n_fft 1024 / hop 256 workgroups that lie wholly behind a row's end return
 * at once, so the cost follows the sum of the rows' frames; other sizes (and GVX_GL_ROCFFT=1) transform the padded frames too
 * and skip them in the overlap-add.  The workspace is that of the uniform call plus the per-row divisors:
 * gvx_gl_workspace_bytes_ragged (a smaller one is GVX_ERR_WORKSPACE).
 *
 * gvx_wav_finalize_ragged: n_samples is the row stride of `wav`; per row the clip, the `trim` samples dropped at both ends of
 * the row's own n_b samples, the peak and the filter (its chunks counted from the row's start) are those of a call on that row
 * alone.  out: float64 [B][n_samples - 2*trim], 0 from n_b - 2*trim on (a row with n_b <= 2*trim is all zeros). */
size_t gvx_gl_workspace_bytes_ragged(gvx_gl_plan* plan, int B, int T, int n_mels);
int gvx_griffin_lim_ragged(gvx_gl_plan* plan, const float* mag, const float* window, int B, int T, const int32_t* frame_lengths,
                           int n_iter, float momentum, float* phase_out, float* wav_out, void* workspace, size_t workspace_bytes,
                           void* stream);
int gvx_wav_finalize_ragged(const float* wav, int B, long n_samples, const int32_t* frame_lengths, int n_fft, int hop, int trim,
                            const double* b_coef, const double* a_coef, int order, double* out, unsigned int* scratch_B, void* stream);

/* ---- Ragged wav -> mel: recordings of different lengths to the mel side of a training batch in one call (the many-files form of
 * AudioProcessor.convert_wav2mel, core/processors.py:70-79, behind the reference's silence trimming, core/processors.py:136-164).
 * pcm is a padded batch of PCM rows [B][n_max], int16 (GVX_PCM_INT16, full scale 32767: what scipy.io.wavfile.read gives) or
 * float32 (GVX_PCM_FLOAT32, full scale 1.0); row b is valid in [0, sample_lengths[b]) and what lies behind is never read as
 * signal.  Lengths and bounds are DEVICE int32 and are clamped to [0, n_max] on the device, so the calls stay asynchronous.
 *
 * gvx_wav_trim_bounds: get_non_silent_boundary (utils/__init__.py:56-76) per row.  Chunks of int(20 * 0.001 * fs) samples are
 * walked from the row's start and, aligned to its last sample, from its end (the last chunk of a walk may be short);
 * bounds_out[b] = {start of the first chunk from the left whose dBFS is >= trim_dbfs, n_b - start of the first such chunk from the
 * right}.  When no chunk passes, a walk ends on its last chunk start as the reference's loop does, so left >= right marks the row
 * as empty.  The decision is sum x^2 >= count * full_scale^2 * 10^(trim_dbfs / 10): for int16 an exact integer sum compared once
 * in double (the reference's float64 decision except on an exact tie).  trim_dbfs NaN: no trimming, bounds_out[b] = {0, n_b}.
 *
 * gvx_wav_to_mel_ragged: row b is the signal pcm[b][left_b, right_b) of bounds [B][2]; with `normalize` every sample is
 * float32(double(y) / double(peak_b)), peak_b = max |y| over the bounds (normalize_signal, utils/audio/base.py:20-22; |-32768| is
 * 32768 here, where the reference's int16 abs wraps).  T_b = (right_b - left_b - n_fft) / hop + 1 frames; the outputs keep the
 * stride T_out: mel_db_out [B][n_mels][T_out] with exact zeros in frames t >= T_b, gate_out [B][T_out] (may be NULL) 1 from
 * frame T_b - 1 on and 0 before, frame_lengths_out [B] = T_b.  row_status_out [B] is 0 or one GVX_WAV_ROW_* word; a row that is
 * EMPTY, SHORT or SILENT has T_b = 0 and zero output (no division by a zero peak, no NaN), a row with more frames than T_out is
 * CUT to T_out.  Row b's mel equals, to the bit, gvx_wav_to_mel on that row's trimmed and normalised signal alone (per frame the
 * same operations in the same order; the mel GEMM runs over all B * T_out padded frames, whose missing rows are zeros).
 * Workspace: gvx_wav_to_mel_ragged_workspace_bytes for T_out <= the frames of n_max samples (a smaller one is GVX_ERR_WORKSPACE). */
enum { GVX_PCM_INT16 = 0, GVX_PCM_FLOAT32 = 1 };
enum { GVX_WAV_ROW_EMPTY = 1,    /* left >= right: nothing left after trimming              */
       GVX_WAV_ROW_SHORT = 2,    /* fewer than n_fft samples: not one frame                 */
       GVX_WAV_ROW_SILENT = 4,   /* every sample is zero: no peak to normalise by           */
       GVX_WAV_ROW_CUT = 8 };    /* more frames than T_out: the first T_out were computed   */
size_t gvx_wav_to_mel_ragged_workspace_bytes(gvx_gl_plan* plan, int B, long n_max, int n_mels);
int gvx_wav_trim_bounds(const void* pcm, int pcm_kind, int B, long n_max, const int32_t* sample_lengths, int fs, float trim_dbfs,
                        int32_t* bounds_out, void* stream);
int gvx_wav_to_mel_ragged(gvx_gl_plan* plan, const void* pcm, int pcm_kind, const float* window, const float* mel_basis, int B,
                          long n_max, const int32_t* bounds, int normalize, int n_mels, int log10_kind, float ref, int T_out,
                          float* mel_db_out, float* gate_out, int32_t* frame_lengths_out, int32_t* row_status_out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- Sample-rate conversion and channel mix-down of PCM batches: the first stage of the reference's data path (format_audio2wav,
 * there an ffmpeg process per file) and the way synthesised audio leaves at another rate.  Asynchronous on `stream`, caller-allocated
 * buffers, no workspace.  GVX_PCM_FLOAT64 (float64 samples, full scale 1.0) is accepted by the calls of this section only.
 *
 * The resampler is filter-agnostic: the caller designs a low-pass prototype h at the rate src * up = dst * down (up / down = dst / src,
 * reduced), centred on index 0, and hands it over as a polyphase table [up][taps_per_phase] (K = taps_per_phase, a multiple of 4 in
 * [4, GVX_RESAMPLE_MAX_TAPS]; float32 for int16 and float32 samples, float64 for float64 samples; 16-byte aligned).  Row b is the
 * signal x = pcm[b][left_b, right_b) of bounds [B][2] (DEVICE int32, clamped to [0, n_max] on the device, as the ragged wav -> mel
 * call takes them), zero outside; with n_b = right_b - left_b it becomes n_out_b = ceil(n_b * up / down) samples.  For output m,
 * 0 <= m < n_out_b, let q = (m * down) / up and p = (m * down) % up:
 *
 *     out[b][m] = sum over k = 0 .. K-1, in ascending k, of  table[p * K + k] * x[q - (K / 2 - 1) + k]
 *
 * (accumulated in the output type, each step one fused multiply-add), which is y[m] = sum_j x[j] * h[m * down - j * up] when
 * table[p * K + k] = h[p + (K / 2 - 1 - k) * up], 0 outside the prototype.  Output 0 sits on input 0: there is no delay.  int16
 * samples are not scaled (full scale stays 32767).  out keeps the stride n_out_stride >= ceil(n_max * up / down) (a smaller one is
 * GVX_ERR_INVALID_ARG): float32 [B][n_out_stride], float64 for float64 samples, exact zeros in [n_out_b, n_out_stride), and
 * out_lengths [B] = n_out_b.  Nothing outside a row's bounds is used as signal, whatever it holds.  A row's result does not depend on
 * the batch it sits in.  up above GVX_RESAMPLE_MAX_UP or down above GVX_RESAMPLE_MAX_DOWN: GVX_ERR_UNSUPPORTED; a NULL pointer, an
 * unknown pcm_kind, up or down < 1, a bad taps_per_phase: GVX_ERR_INVALID_ARG; all of it checked before anything is launched.
 * The kernel stages the table in LDS when it fits beside its input tile and reads it through the cache from global memory when
 * not; the resample_uses_lds_table query says which (1 / 0) for a table of `up` rows and the output type of pcm_kind, and returns -1
 * for an up, taps_per_phase or pcm_kind the call would refuse.  An output block of a workgroup is R * S consecutive samples of a row
 * (S a multiple of up, R in {1, 2, 4}; a function of up, down and taps_per_phase alone): the resample_block_shape query writes S and R
 * and returns 0, or writes nothing and returns -1 for an up, down or taps_per_phase the call would refuse or a NULL pointer.  Neither
 * query makes a HIP call.
 *
 * The mix-down call: interleaved pcm [B][n_max][channels] (what scipy.io.wavfile.read gives per file), channels in [2, 8], to
 * float32 mono_out [B][n_max]: the arithmetic mean of a frame's channels, summed in double in ascending channel order and
 * rounded once (int16 keeps its full scale of 32767). */
enum { GVX_PCM_FLOAT64 = 2 };
enum { GVX_RESAMPLE_MAX_UP = 2048, GVX_RESAMPLE_MAX_DOWN = 2048, GVX_RESAMPLE_MAX_TAPS = 1024 };
int gvx_resample_uses_lds_table(int up, int taps_per_phase, int pcm_kind);
int gvx_resample_block_shape(int up, int down, int taps_per_phase, int* S_out, int* R_out);
int gvx_wav_mixdown(const void* pcm, int pcm_kind, int B, long n_max, int channels, float* mono_out, void* stream);
int gvx_wav_resample_ragged(const void* pcm, int pcm_kind, int B, long n_max, const int32_t* bounds, int up, int down,
                            const void* table, int taps_per_phase, void* out, long n_out_stride, int32_t* out_lengths, void* stream);

/* ---- Evaluation by synthesis: has the model learned to speak?  Two device computations over what the model already leaves on the
 * device (inference: alignments [B][T][L], mel_lengths, padded mels; the batch: target mels and lengths).  Asynchronous on `stream`,
 * caller-allocated outputs, the same bits every run.  Lengths are DEVICE int32 [B], NULL for "every row is full", and are clamped to
 * their range on the device like the ragged vocoder's; nothing behind a row's lengths is read, whatever it holds.
 *
 * Alignment statistics.  alignments is fp32 [B][T][L], dense; T_b = mel_lengths[b] clamped to [0, T], L_b = token_lengths[b] clamped
 * to [0, L].  Per frame t < T_b: peak[t] = max over l < L_b of a[b][t][l] and pos[t] = the LOWEST l that attains it - comparisons of
 * the given values, no arithmetic, so pos is exact.  A NaN never wins a comparison: NaN entries are passed over, and a frame that
 * holds nothing but NaNs yields pos = 0 and peak = NaN (so the row's focus is NaN; its integers stay defined).  Infinities compare
 * as numbers.  Outputs:
 *     positions_out  int32 [B][T]   pos[t]; -1 for t >= T_b
 *     durations_out  int32 [B][L]   #{t < T_b : pos[t] == l}, the frames-per-token table; 0 for l >= L_b
 *     peaks_out      fp32  [B][T]   peak[t]; 0 for t >= T_b
 *     row_ints_out   int32 [B][GVX_ALIGN_ROW_INTS]:
 *         [GVX_ALIGN_MONOTONIC]  #{1 <= t < T_b : pos[t] >= pos[t-1]}
 *         [GVX_ALIGN_MAX_JUMP]   max over 1 <= t < T_b of |pos[t] - pos[t-1]|, 0 if T_b <= 1
 *         [GVX_ALIGN_COVERED]    #{l < L_b : durations[b][l] > 0}
 *         [GVX_ALIGN_FIRST_POS], [GVX_ALIGN_LAST_POS]   pos[0], pos[T_b - 1]
 *     focus_out      fp32  [B]      (sum over t < T_b of peak[t]) / T_b.  The sum has a fixed order: 256 partial sums, number i over
 *                                   the frames i, i + 256, ... in ascending order, then added pairwise at strides 128, 64, ..., 1.
 * A row with T_b == 0 or L_b == 0: its integers 0, its positions -1, its peaks 0, its focus NaN.  Two launches. */
enum { GVX_ALIGN_MONOTONIC = 0, GVX_ALIGN_MAX_JUMP = 1, GVX_ALIGN_COVERED = 2, GVX_ALIGN_FIRST_POS = 3, GVX_ALIGN_LAST_POS = 4,
       GVX_ALIGN_ROW_INTS = 5 };
int gvx_alignment_stats(const float* alignments, const int32_t* mel_lengths, const int32_t* token_lengths, int B, int T, int L,
                        int32_t* positions_out, int32_t* durations_out, float* peaks_out, int32_t* row_ints_out, float* focus_out,
                        void* stream);

/* Features of the warp: out[b][t][k] = sum over m = 0 .. M-1, in ascending m, one fused multiply-add per term, of
 * P[k][m] * mel[b][m][t] - from the [B][M][T] layout the model produces to the [B][T][K] layout the warp reads.  P is any fp32
 * [K][M], 1 <= K <= M (genvox_amd/metrics.py passes rows 1 .. K of the orthonormal DCT-II of size M: mel cepstra without the energy
 * term).  Every frame is projected on its own, so what lies behind a row's length stays behind it.  A P beyond the kernel's LDS tile
 * (K * (M + 1) + 64 * M floats above 160 KiB) is GVX_ERR_UNSUPPORTED. */
int gvx_mel_project(const float* mel, int B, int M, int T, const float* P, int K, float* out, void* stream);

/* Distance under dynamic time warping.  cp is fp32 [B][Tp_max][K], cg fp32 [B][Tg_max][K].  For row b with
 * Tp = pred_lengths[b] (clamped to [0, Tp_max]) frames of cp and Tg = target_lengths[b] (clamped to [0, Tg_max]) frames of cg:
 *
 *     d(i, j) = sqrt( sum over k, in ascending k, of (cp[i][k] - cg[j][k])^2 )       (each term one fused multiply-add)
 *     A[0][0] = 2 d(0, 0)
 *     A[i][0] = A[i-1][0] + d(i, 0)             A[0][j] = A[0][j-1] + d(0, j)
 *     A[i][j] = min( A[i-1][j] + d(i, j),  A[i][j-1] + d(i, j),  A[i-1][j-1] + 2 d(i, j) )
 *     dist_out[b] = A[Tp-1][Tg-1] / (Tp + Tg)
 *
 * the symmetric step pattern, whose normaliser Tp + Tg does not depend on the path taken (a mean over the path jumps where two
 * branches tie to within rounding; this form is continuous in its inputs).  Tp == 0 or Tg == 0: dist_out[b] = NaN.  acc_out, fp32
 * [B][Tp_max][Tg_max] or NULL, receives A[i][j] for i < Tp, j < Tg and is not touched elsewhere; dist_out has the same bits with
 * and without it.  fp32 throughout.
 *
 * One workgroup per row walks the Tp + Tg - 1 anti-diagonals with one barrier each; no workgroup waits for another, and every
 * loop is bounded by Tp + Tg.  When both feature tables and three diagonals fit a CU's LDS
 * (3 * Tp_max + (Tp_max + Tg_max) * (K | 1) floats within 160 KiB; 1000 x 1000 frames of 13 features do) they live there and the
 * call needs no workspace: the size function returns 0 and workspace may be NULL.  Otherwise the features are read through the
 * cache and the diagonals live in the workspace (256-byte aligned, sized by the function below).  The uses_lds_tables query says which
 * (1 / 0; -1 for a shape the call would refuse).  Frames above GVX_DTW_MAX_FRAMES or K above GVX_DTW_MAX_FEATURES:
 * GVX_ERR_UNSUPPORTED (the size function then returns 0); a NULL cp, cg or dist_out, or B, Tp_max, Tg_max or K below 1:
 * GVX_ERR_INVALID_ARG; a missing or short workspace: GVX_ERR_WORKSPACE; all of it checked before anything is launched. */
enum { GVX_DTW_MAX_FRAMES = 32768, GVX_DTW_MAX_FEATURES = 256 };
size_t gvx_dtw_workspace_bytes(int B, int Tp_max, int Tg_max, int K);   /* any contents, no clearing; 0: not needed OR refused (uses_lds_tables: 1 / -1) */
int gvx_dtw_uses_lds_tables(int Tp_max, int Tg_max, int K);
int gvx_dtw_distance(const float* cp, const float* cg, const int32_t* pred_lengths, const int32_t* target_lengths, int B, int Tp_max,
                     int Tg_max, int K, float* dist_out, float* acc_out, void* workspace, size_t workspace_bytes, void* stream);

/* Monotonic alignment search: which frames belong to which token.  alignments is fp32 [B][T][L] (what the decoder loops write).  For
 * row b with T_b = mel_lengths[b] frames (clamped to [0, T]; NULL: T) and L_b = token_lengths[b] tokens (clamped to [0, L]; NULL: L),
 * the path of the highest score among those that start at (0, 0), end at (T_b - 1, L_b - 1) and stay on their token or advance by
 * exactly one token from one frame to the next:
 *
 *     s[t][l] = logf( fmaxf( a[b][t][l], floor ) )          floor in (0, 1]; fmaxf passes over a NaN, which so scores logf(floor)
 *     Q[0][0] = s[0][0]
 *     Q[t][l] = s[t][l] + max( Q[t-1][l], Q[t-1][l-1] )     fp32, plain adds; on a tie the path STAYS (Q[t-1][l] wins)
 *
 * where a predecessor outside the row, or one that no path from (0, 0) reaches (l > t), counts as -inf.  The exact zeros an
 * attention window writes get the finite score logf(floor): no -inf enters a sum from the data.  The path is read back from
 * (T_b - 1, L_b - 1) along the choices made.  Nothing behind a row's lengths is read, whatever it holds.  Outputs:
 *     path_out        int32 [B][T]   the token of frame t: non-decreasing in steps of 0 or 1, 0 at frame 0, L_b - 1 at frame
 *                                    T_b - 1; -1 for t >= T_b                                                       (or NULL)
 *     durations_out   int32 [B][L]   frames on token l: >= 1 for l < L_b, summing to T_b; 0 for l >= L_b
 *     starts_out      int32 [B][L]   first frame of token l; -1 for l >= L_b                                         (or NULL)
 *     score_out       fp32  [B]      Q[T_b - 1][L_b - 1]                                                             (or NULL)
 *     row_status_out  int32 [B]      GVX_MAS_OK; GVX_MAS_EMPTY for T_b == 0 or L_b == 0; GVX_MAS_INFEASIBLE for T_b < L_b (fewer
 *                                    frames than one per token).  A row without a path has path -1, durations 0, starts -1 and
 *                                    score NaN, and nothing of its alignment is read.
 *     scores_out      fp32  [B][T][L] or NULL: receives s[t][l] for t < T_b, l < L_b and is not touched elsewhere; every other
 *                                    output has the same bits with and without it (it lets a test restate the recurrence exactly).
 *
 * One launch, one workgroup per row: the tokens are dealt to the threads, Q of two frames lives in LDS with one barrier per frame,
 * the choices are one bit per cell (a wave's ballot: 64 tokens per 64-bit word, [T][ceil(L / 64)]), and the same workgroup reads the
 * path back and counts the durations.  No workgroup waits for another, and every loop is bounded by T.  When the two Q rows and the
 * bit table fit a CU's LDS (8 L + 8 T ceil(L / 64) bytes within 160 KiB; T = 2000, L = 256 does) the call needs no workspace: the
 * size function returns 0 and workspace may be NULL.  Otherwise the bit table lives in the workspace (256-byte aligned, sized by
 * the function below; any contents).  The uses_lds query says which (1 / 0; -1 for a shape the call would refuse).  T above
 * GVX_MAS_MAX_FRAMES or L above GVX_MAS_MAX_TOKENS: GVX_ERR_UNSUPPORTED (the size function then returns 0); a NULL alignments,
 * durations_out or row_status_out, B, T or L below 1, or a floor outside (0, 1]: GVX_ERR_INVALID_ARG; a missing, misaligned or short
 * workspace: GVX_ERR_WORKSPACE; all of it checked before anything is launched.  Two calls give the same bits. */
enum { GVX_MAS_OK = 0, GVX_MAS_EMPTY = 1, GVX_MAS_INFEASIBLE = 2 };
enum { GVX_MAS_MAX_FRAMES = 32768, GVX_MAS_MAX_TOKENS = 4096 };
size_t gvx_monotonic_align_workspace_bytes(int B, int T, int L);   /* any contents, no clearing; 0: not needed OR refused (uses_lds: 1 / -1) */
int gvx_monotonic_align_uses_lds(int T, int L);
int gvx_monotonic_align(const float* alignments, const int32_t* mel_lengths, const int32_t* token_lengths, int B, int T, int L,
                        float floor, int32_t* path_out, int32_t* durations_out, int32_t* starts_out, float* score_out,
                        int32_t* row_status_out, float* scores_out, void* workspace, size_t workspace_bytes, void* stream);

/* Speaking rate control: a token-wise time warp of a mel, in two calls - the plan (how many frames every token gets) and the warp.
 * Both are asynchronous on `stream`, write caller-allocated outputs only, need no workspace and give the same bits every run; no
 * workgroup waits for another and every loop is bounded by L or M.  For row b, L_b = token_lengths[b] clamped to [0, L] (NULL: L);
 * nothing behind a row's L_b tokens is read, whatever it holds.
 *
 * gvx_duration_scale - the plan.  durations is int32 [B][L] (frames per token, as gvx_monotonic_align writes them), rates fp32
 * [B][L] or NULL for all 1, speed a host float.  Token l is to be spoken e_l = (double)speed * (double)rates[b][l] times as fast:
 *
 *     E_l      = E_{l-1} + (double)d_l / e_l                ascending l from E_{-1} = 0, IEEE double, one rounding per operation
 *     c_l      = llrint(E_l)                                round half to even
 *     S'_0     = 0
 *     S'_{l+1} = max( S'_l + (d_l > 0 ? 1 : 0), c_l )       64-bit integers
 *     d'_l     = S'_{l+1} - S'_l                            T'_b = S'_{L_b}
 *
 * so a spoken token keeps at least one frame, a token without frames gets none, and the rounding error is carried forward
 * instead of piling up: T'_b = llrint(sum d_l / e_l) unless the one-frame minimum binds.  Outputs:
 *     target_durations_out  int32 [B][L]   d'_l; 0 for l >= L_b
 *     target_starts_out     int32 [B][L]   S'_l; -1 for l >= L_b                                                     (or NULL)
 *     out_lengths_out       int32 [B]      T'_b
 *     row_status_out        int32 [B]      decided in this order: GVX_WARP_EMPTY for L_b == 0; GVX_WARP_BAD for a token l < L_b with a
 *                                          negative duration or an e_l that is not inside [GVX_RATE_MIN, GVX_RATE_MAX] = [0.125, 8]
 *                                          (which a non-finite or non-positive rate never is); GVX_WARP_EMPTY for a duration sum
 *                                          of 0; GVX_WARP_BAD for T'_b above GVX_MAS_MAX_FRAMES; else GVX_WARP_OK.  EMPTY and BAD
 *                                          rows have durations 0, starts -1 and length 0.
 * One workgroup per row: the quotients are formed by all threads into LDS (8 L + 4 (L + 1) bytes), one lane walks the sum, the
 * workgroup writes the outputs.  Refused before anything is launched: L above GVX_MAS_MAX_TOKENS: GVX_ERR_UNSUPPORTED; B or L
 * below 1, a speed that is not inside [GVX_RATE_MIN, GVX_RATE_MAX] (NaN and inf are not), a NULL durations, target_durations_out,
 * out_lengths_out or row_status_out: GVX_ERR_INVALID_ARG.
 *
 * gvx_mel_time_warp - the warp.  mel is fp32 [B][M][T], durations and target_durations int32 [B][L].  With the source starts S_l
 * (prefix sums of d, T_b = S_{L_b}) and the target starts S'_l (of d', T'_b = S'_{L_b}), all sums in 64 bits, output frame
 * u < T'_b lies in the token l with S'_l <= u < S'_{l+1} at j = u - S'_l, and maps centre to centre in exact integers:
 *
 *     n    = (2 j + 1) d_l - d'_l
 *     i0   = S_l + floor( n / (2 d'_l) )           rem = n mod 2 d'_l  (in [0, 2 d'_l))
 *     frac = (float)( (double)rem / (double)(2 d'_l) )
 *     i0 < 0: i0 = 0, frac = 0;   i0 >= T_b - 1: i0 = T_b - 1, frac = 0
 *     out[b][m][u] = frac == 0 ? x[b][m][i0] : fmaf( frac, x[b][m][i0 + 1] - x[b][m][i0], x[b][m][i0] )
 *
 * A frame with frac == 0 never reads its neighbour, d' == d returns the input bits, and whatever lies at and behind T_b reaches
 * no output.  Outputs:
 *     mel_out         fp32  [B][M][T_out]  exact zeros for u >= T'_b
 *     src_frame_out   int32 [B][T_out]     i0; -1 for u >= T'_b                                                      (or NULL)
 *     src_frac_out    fp32  [B][T_out]     frac; 0 for u >= T'_b                                                     (or NULL)
 *     row_status_out  int32 [B]            decided in this order: GVX_WARP_BAD for a negative entry of either table, a token with
 *                                          d_l > 0 and d'_l == 0 or the converse, or T_b > T; GVX_WARP_EMPTY for L_b == 0 or
 *                                          T'_b == 0; GVX_WARP_CUT for T'_b > T_out (the first T_out frames are computed); else
 *                                          GVX_WARP_OK.  BAD and EMPTY rows come out as rows of length 0: mel 0, frames -1, fracs 0.
 * mel_out has the same bits with and without the two map outputs; they let a caller warp anything else by the same map, and a
 * test restate the interpolation exactly.  One launch; a workgroup owns a row and GVX_WARP_TILE_FRAMES output frames for all M
 * channels: it builds both prefix sums in LDS (8 (L + 1) bytes), finds every frame's token by bisection once, and streams the
 * channels with loads and stores that run along t.  Refused before anything is launched: L above GVX_MAS_MAX_TOKENS, T or T_out
 * above GVX_MAS_MAX_FRAMES: GVX_ERR_UNSUPPORTED; B, M, T, L or T_out below 1, a NULL mel, durations, target_durations, mel_out or
 * row_status_out: GVX_ERR_INVALID_ARG. */
enum { GVX_WARP_OK = 0, GVX_WARP_EMPTY = 1, GVX_WARP_BAD = 2, GVX_WARP_CUT = 3 };
enum { GVX_WARP_TILE_FRAMES = 64 };
#define GVX_RATE_MIN 0.125f
#define GVX_RATE_MAX 8.0f
int gvx_duration_scale(const int32_t* durations, const int32_t* token_lengths, const float* rates, int B, int L, float speed,
                       int32_t* target_durations_out, int32_t* target_starts_out, int32_t* out_lengths_out, int32_t* row_status_out,
                       void* stream);
int gvx_mel_time_warp(const float* mel, const int32_t* durations, const int32_t* target_durations, const int32_t* token_lengths, int B,
                      int M, int T, int L, int T_out, float* mel_out, int32_t* src_frame_out, float* src_frac_out,
                      int32_t* row_status_out, void* stream);

/* ---- Pitch: YIN F0 contours of waveforms on the device (de Cheveigne and Kawahara 2002, steps 1 - 5, no smoothing: the contour is
 * the raw decision of every frame), and the comparison of two contours - the F0 RMSE, gross pitch error and voicing decision error
 * that accompany the mel-cepstral distance.  Both calls are asynchronous on `stream`, write caller-allocated outputs only, need no
 * workspace and give the same bits every run (fixed summation orders, no atomics); no workgroup waits for another and every loop is
 * bounded by the parameters.
 *
 * gvx_pitch_yin - the tracker.  wav is fp32 [B][N], row b of n_b = sample_lengths[b] samples (clamped to [0, N]; NULL: N); nothing at
 * or behind n_b is read, whatever it holds.  Row b has F_b = gvx_pitch_frames(n_b, hop) = ceil(n_b / hop) frames, and
 * F = gvx_pitch_frames(N, hop) is the stride of the outputs.  With W = window, x = the row with zeros outside [0, n_b), and for
 * frame f
 *
 *     s        = first_centre + f * hop - (W + lag_max) / 2         (integer division; first_centre is the sample index of frame
 *                                                                    0's centre and may be negative: -TRIM for a Griffin-Lim
 *                                                                    waveform that lost TRIM samples at its head)
 *     d(tau)   = sum over j = 0 .. W-1 of (x[s+j] - x[s+j+tau])^2    tau = 0 .. lag_max; fp32, j ascending, each term one
 *                                                                    subtraction and one fused multiply-add
 *     c(0)     = 1
 *     c(tau)   = d(tau) * tau / sum over k = 1 .. tau of d(k)        tau >= 1; 1 where that sum is 0 (digital silence).  The sum's
 *                                                                    order: lag_max lags in 64 runs of ceil(lag_max / 64), each run
 *                                                                    ascending on top of the runs before it
 *     lag      : scan tau from lag_min to lag_max - 1; at the first tau with c(tau) < threshold walk on while c(tau+1) < c(tau) and
 *                tau + 1 <= lag_max - 1, and take that tau.  No such tau: the frame is unvoiced.
 *     den      = c(lag-1) - 2 c(lag) + c(lag+1)
 *     shift    = den > 0 ? clamp( (c(lag-1) - c(lag+1)) / (2 den), -1, 1 ) : 0
 *     f0       = sampling_rate / (lag + shift)
 *
 * d is computed in this form and no other: energy minus autocorrelation, r(0) + r_tau(0) - 2 acf(tau), and every FFT route cancel
 * catastrophically in fp32 on nearly periodic signals, which is where d is small and the decision is made; a sum of squared
 * differences has no cancellation, so |c32 - c| <= (2 W + lag_max + 8) 2^-24 c in any summation order.  Outputs:
 *     f0_out            fp32  [B][F]   Hz; 0 for an unvoiced frame and for f >= F_b
 *     lag_out           int32 [B][F]   the lag; -1 for an unvoiced frame and for f >= F_b
 *     aperiodicity_out  fp32  [B][F]   c(lag); for an unvoiced frame the minimum of c over [lag_min, lag_max); 1 for f >= F_b
 *     cmnd_out          fp32  [B][F][lag_max + 1] or NULL: receives c(0 .. lag_max) of every frame f < F_b, the table the decision ran
 *                                      on, and is not touched elsewhere; every other output has the same bits with and without it
 * One launch.  A workgroup takes one row and gvx_pitch_tile_frames(params) consecutive frames (at most 16; fewer when W + lag_max +
 * (frames - 1) hop samples and four tables of lag_max + 1 floats do not fit 64 KiB of LDS), stages their samples in LDS once, and
 * gives every frame to one wave: lanes across lags, three consecutive lags and a sliding window of samples per lane.  Limits, all
 * checked before anything is launched: a NULL wav, params, f0_out, lag_out or aperiodicity_out, B, N, sampling_rate, hop or window
 * below 1, lag_min below 1 or not below lag_max, a threshold outside (0, 1] (NaN is): GVX_ERR_INVALID_ARG; window outside
 * [GVX_PITCH_MIN_WINDOW, GVX_PITCH_MAX_WINDOW] = [32, 2048], lag_max above GVX_PITCH_MAX_LAG = 1024, B above GVX_PITCH_MAX_ROWS =
 * 65535, F above GVX_PITCH_MAX_FRAMES = 32768: GVX_ERR_UNSUPPORTED (gvx_pitch_tile_frames then returns -1).
 *
 * gvx_f0_compare - two contours on the same frame grid.  f0_a and f0_b are fp32 [B][F] (0 or below: unvoiced, as is NaN); row b is
 * compared over n = min(frames_a[b], frames_b[b]) frames (each clamped to [0, F]; NULL: F).  A frame voiced in both with ratio
 * r = (double)a / (double)b is a gross error if |r - 1| > 0.2 (in double).  Outputs per row:
 *     counts_out      int32 [B][GVX_F0_ROW_INTS]   [GVX_F0_FRAMES] n, [GVX_F0_VOICED_BOTH], [GVX_F0_VOICED_ONE] voiced in exactly one,
 *                                                  [GVX_F0_GROSS]
 *     vde_out         fp32  [B]   (float)voiced_one / (float)n                       NaN for n == 0
 *     gpe_out         fp32  [B]   (float)gross / (float)voiced_both                  NaN for voiced_both == 0
 *     rmse_cents_out  fp32  [B]   sqrt of the mean of (1200 log2 r)^2 over the frames voiced in both and not gross, formed in double
 *                                 and rounded once; NaN when there is no such frame
 * One launch, one workgroup per row: 256 partial results, number i over the frames i, i + 256, ... in ascending order, added
 * pairwise at strides 128, 64, ..., 1.  Contours of different lengths along a warping path are out of scope (gvx_dtw_distance
 * returns no path): the use is copy-synthesis, recording -> mel -> vocoder -> waveform against the recording, both tracked on the
 * mel's frame grid.  A NULL f0_a, f0_b or output, B or F below 1: GVX_ERR_INVALID_ARG; F above
 * GVX_PITCH_MAX_FRAMES: GVX_ERR_UNSUPPORTED. */
typedef struct gvx_pitch_params {
    int32_t sampling_rate;   /* Hz                                                           */
    int32_t hop;             /* samples between frame centres                                */
    int32_t window;          /* W: terms of the difference function                          */
    int32_t lag_min;         /* shortest period searched, samples: floor(rate / fmax)        */
    int32_t lag_max;         /* longest period, samples: ceil(rate / fmin)                   */
    float threshold;         /* of the cumulative-mean-normalised difference; YIN uses 0.1 - 0.15 */
    int32_t first_centre;    /* sample index of frame 0's centre; may be negative            */
} gvx_pitch_params;
enum { GVX_PITCH_MIN_WINDOW = 32, GVX_PITCH_MAX_WINDOW = 2048, GVX_PITCH_MAX_LAG = 1024, GVX_PITCH_MAX_ROWS = 65535,
       GVX_PITCH_MAX_FRAMES = 32768 };
enum { GVX_F0_FRAMES = 0, GVX_F0_VOICED_BOTH = 1, GVX_F0_VOICED_ONE = 2, GVX_F0_GROSS = 3, GVX_F0_ROW_INTS = 4 };
int gvx_pitch_frames(long n, int hop);   /* host arithmetic: ceil(n / hop); 0 for n <= 0 or hop < 1 */
int gvx_pitch_tile_frames(const gvx_pitch_params* params);
int gvx_pitch_yin(const float* wav, const int32_t* sample_lengths, int B, long N, const gvx_pitch_params* params, float* f0_out,
                  int32_t* lag_out, float* aperiodicity_out, float* cmnd_out, void* stream);
int gvx_f0_compare(const float* f0_a, const float* f0_b, const int32_t* frames_a, const int32_t* frames_b, int B, int F,
                   int32_t* counts_out, float* vde_out, float* gpe_out, float* rmse_cents_out, void* stream);

/* ---- Pitch control: time-domain pitch-synchronous overlap-add (TD-PSOLA) of waveforms on the device, in two calls - the plan
 * (where the pitch marks of the input lie and where the grains of the output go) and the synthesis (the overlap-add).  The row
 * keeps its length; its pitch is multiplied by a ratio per frame.  Both calls are asynchronous on `stream`, write caller-allocated
 * outputs only, need no workspace and give the same bits every run (fixed summation orders, no atomics); no workgroup waits for
 * another and every loop is bounded by the capacities below.
 *
 * All quantities are per row b.  The row has n = sample_lengths[b] samples, clamped to [0, N] (NULL: N); x is the row with zeros
 * outside [0, n); nothing at or behind n is read, whatever it holds.  The frame grid is the tracker's: hop, first_centre,
 * F_b = gvx_pitch_frames(n, hop), and F = gvx_pitch_frames(N, hop) is the stride of lag and ratio.
 *
 *     frame_of(t)  = clamp( floordiv(t - first_centre + hop / 2, hop), 0, F_b - 1 )        (hop / 2 by integer division)
 *     lag          int32 [B][F], as gvx_pitch_yin writes it (-1: unvoiced)
 *     voiced_at(t) = lag[frame_of(t)] >= 1
 *     period_at(t) = clamp(lag[frame_of(t)], lag_min, lag_max) when voiced_at(t) (the clamp changes no lag of the tracker's),
 *                    else U = unvoiced_period
 *
 * Analysis marks - integers and comparisons only, hence exact.  m_{-1} = -1.  The candidate is c = 0 for k = 0 and
 * c = m_{k-1} + period_at(m_{k-1}) afterwards; the walk stops when c >= n.  If voiced_at(c):
 *     r   = min(period_at(c), period_at(m_{k-1})) / 4     by integer division; for k = 0, r = period_at(0) / 4
 *     m_k = the lowest index of the largest x over [max(c - r, m_{k-1} + 1), min(c + r, n - 1)]: the first index whose sample
 *           compares greater than everything before it, from -inf (a window of nothing but NaN and -inf, which no waveform
 *           holds, gives m_k = c)
 * otherwise m_k = c.  Recorded: p_k = period_at(m_k) and v_k = voiced_at(m_k).  A step advances by at least ceil(3 p / 4), so a
 * row has at most gvx_psola_max_marks(N, p_min) = N / ceil(3 p_min / 4) + 1 marks, p_min = min(lag_min, U): the loop bound and the
 * capacity K of the mark outputs.
 *
 * Synthesis marks.  ratio is fp32 [B][F] on the same frame grid; ratio > 1 raises the pitch.  s_0 = m_0, a_0 = 0; grain j copies
 * analysis grain a_j:
 *     q_j     = v_{a_j} ? ratio[frame_of(s_j)] : 1                                  unvoiced sound is never repitched
 *     step_j  = max(1, (int)floor((double)p_{a_j} / (double)q_j + 0.5))
 *     s_{j+1} = s_j + step_j                                                        the walk stops when s_{j+1} >= n
 *     a_{j+1} = the k >= a_j with the smallest |m_k - s_{j+1}|, lowest k on a tie    a pointer that only moves forward
 * A row has at most gvx_psola_max_grains(N, p_min) = N / max(1, (p_min + 1) / 2) + 1 grains: the capacity J of the grain outputs.
 * A ratio that is NaN or outside [GVX_PSOLA_RATIO_MIN, GVX_PSOLA_RATIO_MAX] = [0.5, 2] in a frame below F_b gives the row the
 * status GVX_PSOLA_BAD_RATIO: its analysis marks are written, it has no grains, and the synthesis copies it through unchanged.
 * A row with n = 0 (the only rows without marks) has the status GVX_PSOLA_EMPTY.
 *
 * Overlap-add, fp32, every operation rounded once, in this order.  Grain j reaches sample t when u = t - s_j has |u| < p_{a_j}:
 *     v      = 1 - (float)|u| / (float)p_{a_j}
 *     w      = (v * v) * (3 - 2 * v)                    S(v) = v^2 (3 - 2 v): a polynomial window, every bit defined without a device
 *                                                       cosine; like Hann's, S(v) + S(1 - v) = 1: grains at a constant period sum to 1
 *     Num(t) = fmaf(w, x[m_{a_j} + u], Num(t))          D(t) = D(t) + w        both from 0, j ascending
 *     inside [s_0, s_last]:  y = Num / max(D, 0.5)
 *     outside it:            y = D >= 1 ? Num / D : fmaf(1 - D, x[t], Num)     sound before the first and after the last mark is kept
 *     y[t] = 0 for t >= n
 *
 * gvx_psola_plan - one launch, one workgroup (one wave) per row: both walks are sequential by nature.  The wave stages 4096 samples
 * and the periods of their frames in LDS at a time, searches the window of a mark (at most 2 (lag_max / 4) + 1 samples) with all
 * lanes and a lowest-index tie rule, and stores marks and grains 64 at a time.  Outputs:
 *     marks_out       int32 [B][K]   m_k                                   K = gvx_psola_max_marks(N, min(lag_min, U))
 *     periods_out     int32 [B][K]   v_k ? p_k : -p_k
 *     syn_pos_out     int32 [B][J]   s_j                                   J = gvx_psola_max_grains(N, min(lag_min, U))
 *     syn_src_out     int32 [B][J]   a_j
 *     counts_out      int32 [B][GVX_PSOLA_ROW_INTS]   [GVX_PSOLA_MARKS], [GVX_PSOLA_GRAINS]
 *     row_status_out  int32 [B]      GVX_PSOLA_OK / EMPTY / BAD_RATIO
 * Nothing is written behind the counts.
 *
 * gvx_psola_synth - one launch, a workgroup per row and GVX_PSOLA_TILE output samples.  It finds the grains that can reach its tile
 * (s within max(lag_max, U) of it) by bisection over s, keeps their (s, m, p) in LDS (at most GVX_PSOLA_TILE + 2 max(lag_max, U)),
 * and every thread gathers its own sample in ascending j.  marks .. row_status are what the plan wrote (counts and indices that
 * are out of range are clamped, samples outside [0, n) read as 0: no table can make the call read or write out of bounds).
 * wav_out is fp32 [B][N] and may not overlap wav.
 *
 * Refused before anything is launched: a NULL wav, lag, ratio (plan), params, table or output, B, N, hop, lag_min or
 * unvoiced_period below 1, lag_max below lag_min: GVX_ERR_INVALID_ARG; lag_max or unvoiced_period above GVX_PITCH_MAX_LAG, B above
 * GVX_PITCH_MAX_ROWS, more than GVX_PITCH_MAX_FRAMES frames, or more than GVX_PITCH_MAX_FRAMES * GVX_PITCH_MAX_LAG samples at a hop beyond
 * that lag (counts and indices are 32-bit): GVX_ERR_UNSUPPORTED. */
typedef struct gvx_psola_params {
    int32_t hop;               /* samples between frame centres: the tracker's                 */
    int32_t first_centre;      /* sample index of frame 0's centre: the tracker's              */
    int32_t lag_min;           /* shortest and                                                 */
    int32_t lag_max;           /*   longest period the lag table can hold                      */
    int32_t unvoiced_period;   /* U: the spacing of marks where there is no pitch              */
} gvx_psola_params;
enum { GVX_PSOLA_OK = 0, GVX_PSOLA_EMPTY = 1, GVX_PSOLA_BAD_RATIO = 2 };
enum { GVX_PSOLA_MARKS = 0, GVX_PSOLA_GRAINS = 1, GVX_PSOLA_ROW_INTS = 2 };
enum { GVX_PSOLA_TILE = 256 };
#define GVX_PSOLA_RATIO_MIN 0.5f
#define GVX_PSOLA_RATIO_MAX 2.0f
long gvx_psola_max_marks(long N, int p_min);    /* host arithmetic; 0 for N < 1 or p_min < 1 */
long gvx_psola_max_grains(long N, int p_min);   /* host arithmetic; 0 for N < 1 or p_min < 1 */
int gvx_psola_plan(const float* wav, const int32_t* sample_lengths, const int32_t* lag, const float* ratio, int B, long N,
                   const gvx_psola_params* params, int32_t* marks_out, int32_t* periods_out, int32_t* syn_pos_out,
                   int32_t* syn_src_out, int32_t* counts_out, int32_t* row_status_out, void* stream);
int gvx_psola_synth(const float* wav, const int32_t* sample_lengths, const int32_t* marks, const int32_t* periods,
                    const int32_t* syn_pos, const int32_t* syn_src, const int32_t* counts, const int32_t* row_status, int B, long N,
                    const gvx_psola_params* params, float* wav_out, void* stream);

/* ---- Neural vocoder: MelGAN generator, mel -> waveform: inference, and training (behind the inference calls).  The reference promises a vocoder model and ships only its config
 * (configs/models.py:89-121, MelGANConfig); the network below is this project's statement of the MelGAN generator.
 *
 * Input: mel fp32 [B][n_mels][T], as the Tacotron2 calls deliver mel_outputs_postnet (no conversion).  Output: wav fp32 [B][T * hop],
 * hop = the product of the ratios, every sample in (-1, 1).  lrelu(v) = v > 0 ? v : slope * v; "reflect p" mirrors p positions at both
 * ends of the time axis without repeating the edge (torch.nn.functional.pad(mode="reflect")).  C_0 = base_channels, C_{i+1} = C_i / 2.
 *
 *     x = Conv1d(n_mels -> C_0, k = 7)(reflect 3 (mel))
 *     for stage i, r = ratios[i]:
 *         x = ConvTranspose1d(C_i -> C_{i+1}, kernel 2 r, stride r, padding r / 2)(lrelu(x))                 length times r
 *         for j in 0 .. n_residual_layers - 1, d = dilation_base^j:
 *             h = Conv1d(C_{i+1} -> C_{i+1}, k = 3, dilation d)(reflect d (lrelu(x)))
 *             x = Conv1d(k = 1)(x) + Conv1d(k = 1)(lrelu(h))                                                 shortcut + mix
 *     wav = tanh(Conv1d(C_last -> 1, k = 7)(reflect 3 (lrelu(x))))
 *
 * Ragged batches: frame_lengths is int32 [B] on the device, or NULL for all T.  Row b is computed at T_b = min(frame_lengths[b], T)
 * frames: every reflection happens at the row's own end of that stage, so row b has the bits of that row run alone; nothing of mel at
 * or behind frame T_b is read, and wav is exactly 0 from sample T_b * hop on.  A row needs T_b >= GVX_MELGAN_MIN_FRAMES (the first
 * reflection); the host cannot see device lengths, so the CALLER checks them - a shorter row comes out as silence of length 0.
 *
 * Dims are refused (GVX_ERR_INVALID_ARG from create and pack, 0 from the size functions) unless: n_mels, base_channels >= 1; n_stages in
 * [1, GVX_MELGAN_MAX_STAGES]; every ratio even and >= 2, their product <= GVX_MELGAN_MAX_HOP; base_channels divisible by 2^n_stages;
 * n_residual_layers in [1, 8]; dilation_base >= 1 with dilation_base^(n_residual_layers - 1) < 4 * ratios[0] (a reflection stays inside
 * the shortest row); slope in [0, 1].
 *
 * Weights.  gvx_melgan_pack_weights_device reads PyTorch-layout tensors from DEVICE pointers, by name:
 *     pre.weight [C_0][n_mels][7], pre.bias;  ups.<i>.weight [C_i][C_{i+1}][2 r] (ConvTranspose1d: in, out, k), ups.<i>.bias;
 *     res.<i>.<j>.conv.weight [C][C][3], res.<i>.<j>.shortcut.weight [C][C][1], res.<i>.<j>.mix.weight [C][C][1] and their .bias;
 *     post.weight [1][C_last][7], post.bias
 * and writes the blob the kernels read: K-contiguous rows [C_out][taps * C_in] (the first convolution's channels padded with zeros to a
 * multiple of 4), the transposed convolutions split into their r phases [r][C_out][2 C_in], shortcut and mix side by side as one
 * [C][2 C] matrix.  Every tensor of the blob starts at a multiple of 64 floats, so gvx_melgan_blob_floats = the parameter count
 * + 7 * C_0 * (round4(n_mels) - n_mels) + what rounds each of its tensors (the 2 + 2 * n_stages + 5 * n_stages * n_residual_layers + 2
 * listed above, shortcut and mix weights counting as one) up to a multiple of 64 floats.  A missing name is GVX_ERR_MISSING_WEIGHT, a
 * wrong element count GVX_ERR_SHAPE, both before anything is launched.  The blob must be 256-byte aligned; the handle keeps the pointer.
 *
 * Workspace: gvx_melgan_workspace_bytes is host arithmetic (no device, no handle):
 *     B * ( round256(4 * T * round4(n_mels)) + 3 * round256(4 * T * W) ),   W = max(C_0, max_i ratios[0] * .. * ratios[i] * C_{i+1})
 * - the transposed mel and three activation tensors of the widest stage, which the layers rotate through.  With the defaults W = 8192:
 * 98,624 bytes per frame and row.  Linear in B, monotone in T; any contents when the call starts, nothing is cleared; 256-byte aligned;
 * a NULL, misaligned or short one is GVX_ERR_WORKSPACE before anything is launched (the conventions at the top of this header).
 *
 * gvx_melgan_forward is a feed-forward chain of ordinary launches on `stream` (2 + n_stages * (1 + 2 * n_residual_layers) + 1): every
 * layer is one implicit GEMM over channels-last activations on v_mfma_f32_32x32x2_f32 (C_out >= 32) or fmaf dot products (narrower layers
 * and the output layer).  No workgroup waits for another; two calls give the same bits.  stage_out is NULL or a HOST array of n_stages
 * device pointers (16-byte aligned): stage_out[i] receives x after stage i's residual stack, fp32 [B][T * ratios[0] * .. * ratios[i]][C_{i+1}],
 * exact zeros behind a row's own length - for tests that localise a wrong layer; it changes no bit of wav.  T below GVX_MELGAN_MIN_FRAMES,
 * B outside [1, 65535] or a NULL mel / wav_out: GVX_ERR_INVALID_ARG; T above GVX_MELGAN_MAX_FRAMES: GVX_ERR_UNSUPPORTED; no blob bound:
 * GVX_ERR_STATE.
 *
 * Timing (measurement only): with gvx_melgan_timing_enable, a forward records HIP events between the parts; gvx_melgan_stage_times_ms
 * synchronises on the last and returns n_stages + 2 durations: first convolution (with the mel transpose), every stage, output layer. */
enum { GVX_MELGAN_MAX_STAGES = 8, GVX_MELGAN_MIN_FRAMES = 4, GVX_MELGAN_MAX_FRAMES = 32768, GVX_MELGAN_MAX_HOP = 4096 };
typedef struct gvx_melgan_dims {
    int32_t n_mels;
    int32_t base_channels;
    int32_t n_stages;
    int32_t ratios[GVX_MELGAN_MAX_STAGES];
    int32_t n_residual_layers;
    int32_t dilation_base;
    float slope;
} gvx_melgan_dims;
typedef struct gvx_melgan gvx_melgan;
size_t gvx_melgan_blob_floats(const gvx_melgan_dims* dims);
size_t gvx_melgan_workspace_bytes(const gvx_melgan_dims* dims, int B, int T);
int gvx_melgan_pack_weights_device(const gvx_melgan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_melgan_create(const gvx_melgan_dims* dims, gvx_melgan** out);
void gvx_melgan_destroy(gvx_melgan* handle);
int gvx_melgan_bind(gvx_melgan* handle, const float* device_blob);
int gvx_melgan_forward(gvx_melgan* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out,
                       float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_melgan_timing_enable(gvx_melgan* handle, int enable);
int gvx_melgan_stage_times_ms(gvx_melgan* handle, float* ms_out, int* n_out);

/* Training the generator: a forward that keeps a tape, and the backward.  Model, layouts, raggedness and error conventions are those of
 * gvx_melgan_forward above; all arithmetic is fp32.  Training is on plain weights (a weight-normalised checkpoint is folded on load).
 *
 * Tape: the caller's memory, 256-byte aligned, gvx_melgan_tape_bytes (host arithmetic) long.  It holds every tensor the backward reads,
 * in forward order, which gvx_melgan_tape_layout (host arithmetic) lists as (byte offset, positions per frame, channels):
 *     the transposed mel [round4(n_mels) channels];  x after the first convolution;
 *     per stage: the transposed convolution's output, then per residual layer h and the new x.
 * Each is fp32, RAW pre-activation values, channels-last [B][T * positions per frame][channels] with rows strided by the padded T, and
 * starts where the one before it ends: the tape is 4 * B * T * F bytes with F = round4(n_mels) + C_0 + the sum over the stages of
 * (1 + 2 * n_residual_layers) * ratios[0] * .. * ratios[i] * C_{i+1} floats per frame and row.  With the defaults F = 80 + 512 +
 * 7 * (2048 + 3 * 8192) = 186,960 floats, 747,840 bytes per frame and row.  Linear in B and in T.  Behind a row's own length the tape
 * holds whatever it held before: the backward reads nothing there.  The layout call returns the number of entries
 * (2 + n_stages * (1 + 2 * n_residual_layers)) and fills at most max_entries of them (entries may be NULL); both return 0 for refused
 * dims, B outside [1, 65535] or T outside [GVX_MELGAN_MIN_FRAMES, GVX_MELGAN_MAX_FRAMES].
 *
 * gvx_melgan_forward_train is the forward with every layer writing into its own tape slot - the same kernels with the same arguments, so
 * wav_out has the bits of gvx_melgan_forward.  It needs no scratch: workspace may be NULL and workspace_bytes 0.
 *
 * gvx_melgan_backward: d_wav fp32 [B][T * hop], never read at or behind sample T_b * hop.  grads is a HOST table that names DEVICE
 * destinations under the packer's names; every parameter gradient is WRITTEN (not accumulated) in PyTorch's own layout: Conv1d
 * [out][in][k] (the first convolution without padded channels), ConvTranspose1d [in][out][2 r], shortcut and mix as two tensors.
 * d_mel_out is NULL (the first layer's data gradient is skipped; no parameter gradient changes a bit) or fp32 [B][n_mels][T], exactly 0
 * at and behind a row's frames; row b of it has the bits of that row run alone.  Refused before anything is launched: a missing name
 * (GVX_ERR_MISSING_WEIGHT), a wrong element count or NULL destination (GVX_ERR_SHAPE), a NULL, short or misaligned tape or workspace
 * (GVX_ERR_WORKSPACE), T or B as the forward refuses them, B * T * hop above 65535 * 512 positions (GVX_ERR_UNSUPPORTED).
 * gvx_melgan_backward_workspace_bytes is host arithmetic: any contents when the call starts, nothing is cleared; it holds the transposed
 * weights (made from the bound blob at the start of every call, so never stale), the gradient of two activation tensors and of one
 * residual tail, and the partial products of the widest weight gradient.
 *
 * The backward is a chain of ordinary launches.  Data gradients are implicit GEMMs that gather dY on the way into LDS (the reflections
 * and the stride of the forward, transposed), on v_mfma_f32_32x32x2_f32 where the layer has 32 channels or more and fmaf dot products
 * below; weight and bias gradients are reduced over all rows' positions in pieces of 512 positions, whose partial products are added in
 * a fixed order.  No float atomics: two calls give the same bits. */
typedef struct gvx_melgan_tape_entry {
    uint64_t byte_offset;
    int32_t positions_per_frame;
    int32_t channels;
} gvx_melgan_tape_entry;
typedef struct gvx_grad_desc {
    const char* name;   /* a parameter's name, as gvx_melgan_pack_weights_device reads it */
    float* data;        /* DEVICE pointer that receives the gradient */
    int64_t numel;
} gvx_grad_desc;
size_t gvx_melgan_tape_bytes(const gvx_melgan_dims* dims, int B, int T);
int gvx_melgan_tape_layout(const gvx_melgan_dims* dims, int B, int T, gvx_melgan_tape_entry* entries, int max_entries);
size_t gvx_melgan_backward_workspace_bytes(const gvx_melgan_dims* dims, int B, int T);
int gvx_melgan_forward_train(gvx_melgan* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, void* tape,
                             size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_melgan_backward(gvx_melgan* handle, const float* d_wav, const int32_t* frame_lengths, int B, int T, const void* tape,
                        size_t tape_bytes, const gvx_grad_desc* grads, int n_grads, float* d_mel_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- HiFi-GAN generator, mel -> waveform (Kong et al. 2020; its V1, V2 and V3 generators).  The reference ships no such
 * model; the network below is the published implementation's, under its names.  Kernels: csrc/hifigan.hip; all arithmetic is fp32.
 *
 * Input: mel fp32 [B][n_mels][T].  Output: wav fp32 [B][T * hop], hop = the product of upsample_rates, every sample in (-1, 1).
 * lrelu(v, s) = v > 0 ? v : s * v.  Every convolution pads with ZEROS.  C_0 = upsample_initial_channel, C_{i+1} = C_i / 2, n_k =
 * n_resblocks.
 *
 *     x = Conv1d(n_mels -> C_0, k = 7, padding 3)(mel)                                                       conv_pre
 *     for stage i, r = upsample_rates[i]:
 *         x = ConvTranspose1d(C_i -> C_{i+1}, kernel 2 r, stride r, padding r / 2)(lrelu(x, slope))          ups.<i>, length times r
 *         y_j = resblocks.<i * n_k + j>(x) for j = 0 .. n_k - 1;   x = (y_0 + y_1 + ..) / n_k                 added in that order, then divided
 *     wav = tanh(Conv1d(C_last -> 1, k = 7, padding 3)(lrelu(x, post_slope)))                                conv_post
 *
 *     resblock 1, kernel k = resblock_kernel_sizes[j], dilations d_m = resblock_dilation_sizes[j][m], m = 0 .. 2:
 *         x = x + convs2.<m>(lrelu(convs1.<m>(lrelu(x, slope)), slope))      convs1: dilation d_m, padding (k - 1) d_m / 2; convs2: dilation 1
 *     resblock 2, m = 0 .. 1:
 *         x = x + convs.<m>(lrelu(x, slope))                                 dilation d_m, padding (k - 1) d_m / 2
 *
 * Ragged batches: frame_lengths is int32 [B] on the device, or NULL for all T.  Row b is computed at T_b = min(frame_lengths[b], T)
 * frames as that row run alone: at every layer zeros lie beyond the row's own T_b * (rates so far) positions.  Nothing of mel at or
 * behind frame T_b is read, and wav is exactly 0 from sample T_b * hop on.  The shortest row is 1 frame; the host cannot see device
 * lengths, so the CALLER checks them - a row below 1 frame comes out as silence of length 0.
 *
 * Dims are refused (GVX_ERR_INVALID_ARG from create and pack, 0 from the size functions) unless: n_mels >= 1; n_stages in [1,
 * GVX_HIFIGAN_MAX_STAGES]; every rate even and >= 2 with upsample_kernel_sizes[i] == 2 * upsample_rates[i] (the two-tap phase split;
 * it covers the three published configurations), their product <= GVX_HIFIGAN_MAX_HOP; upsample_initial_channel divisible by
 * 2^n_stages and every stage's channel count C_{i+1} a multiple of 4 and >= 4; resblock 1 with n_dilations 3 or resblock 2 with
 * n_dilations 2; n_resblocks in [1, GVX_HIFIGAN_MAX_RESBLOCKS]; every resblock kernel size odd and in [3, 11]; every dilation >= 1 with
 * (k - 1) * d <= GVX_HIFIGAN_MAX_WINDOW (72: V3's k = 7, d = 12); slope and post_slope in [0, 1].
 *
 * Weights.  gvx_hifigan_pack_weights_device reads PyTorch-layout tensors from DEVICE pointers, by the published names:
 *     conv_pre.weight [C_0][n_mels][7];  ups.<i>.weight [C_i][C_{i+1}][2 r] (ConvTranspose1d: in, out, k);
 *     resblocks.<n>.convs1.<m>.weight / .convs2.<m>.weight [C][C][k] (resblock 2: .convs.<m>.weight);  conv_post.weight [1][C_last][7];
 *     and every layer's .bias
 * (plain weights: a weight-normalised checkpoint is folded by the caller) and writes the blob the kernels read: K-contiguous rows
 * [C_out][taps * C_in] (conv_pre's channels padded with zeros to a multiple of 4), the transposed convolutions split into their r
 * phases [r][C_out][2 C_in].  Every tensor of the blob starts at a multiple of 64 floats, so gvx_hifigan_blob_floats = the parameter
 * count + 7 * C_0 * (round4(n_mels) - n_mels) + what rounds each weight and each bias up to a multiple of 64 floats.  A missing name is
 * GVX_ERR_MISSING_WEIGHT, a wrong element count GVX_ERR_SHAPE, both before anything is launched.  The blob must be 256-byte aligned.
 *
 * Workspace: gvx_hifigan_workspace_bytes is host arithmetic (no device, no handle):
 *     B * ( round256(4 * T * round4(n_mels)) + 4 * round256(4 * T * W) ),   W = max(C_0, max_i rates[0] * .. * rates[i] * C_{i+1})
 * - the transposed mel and four activation tensors of the widest stage: a stage's x, a residual block's running value and its inner
 * tensor, and the sum of the blocks.  V1, V2, V3: W = 8192, 2048, 8192 floats.  Linear in B, monotone in T; any contents when the call
 * starts, nothing is cleared; 256-byte aligned; a NULL, misaligned or short one is GVX_ERR_WORKSPACE before anything is launched.
 *
 * gvx_hifigan_forward is a feed-forward chain of ordinary launches on `stream`, one per layer.  A convolution with C_out >= 32 is an
 * implicit GEMM over channels-last activations on v_mfma_f32_32x32x2_f32 whose workgroup holds its input window in LDS once per block
 * of 32 input channels and runs every tap off it; narrower layers and the output layer are fmaf dot products.  The last convolution of
 * resblock j writes (j = 0) or adds (j > 0) y_j into the stage's sum, and the last of them divides: no atomics, no workgroup waits for
 * another, two calls give the same bits.  stage_out is NULL or a HOST array of n_stages device pointers (16-byte aligned):
 * stage_out[i] receives x after stage i's average, fp32 [B][T * rates[0] * .. * rates[i]][C_{i+1}], exact zeros behind a row's own
 * length; it changes no bit of wav.  T below 1, B outside [1, 65535] or a NULL mel / wav_out: GVX_ERR_INVALID_ARG; T above
 * GVX_HIFIGAN_MAX_FRAMES: GVX_ERR_UNSUPPORTED; no blob bound: GVX_ERR_STATE.
 *
 * Timing (measurement only): as gvx_melgan_timing_enable / gvx_melgan_stage_times_ms: n_stages + 2 durations, conv_pre (with the mel
 * transpose), every stage, conv_post. */
enum { GVX_HIFIGAN_MAX_STAGES = 8, GVX_HIFIGAN_MAX_RESBLOCKS = 4, GVX_HIFIGAN_MAX_DILATIONS = 3, GVX_HIFIGAN_MAX_WINDOW = 72,
       GVX_HIFIGAN_MAX_FRAMES = 32768, GVX_HIFIGAN_MAX_HOP = 4096 };
typedef struct gvx_hifigan_dims {
    int32_t n_mels;
    int32_t upsample_initial_channel;
    int32_t n_stages;
    int32_t upsample_rates[GVX_HIFIGAN_MAX_STAGES];
    int32_t upsample_kernel_sizes[GVX_HIFIGAN_MAX_STAGES];
    int32_t resblock;      /* 1 or 2 */
    int32_t n_resblocks;   /* n_k: residual blocks per stage */
    int32_t n_dilations;   /* 3 for resblock 1, 2 for resblock 2 */
    int32_t resblock_kernel_sizes[GVX_HIFIGAN_MAX_RESBLOCKS];
    int32_t resblock_dilation_sizes[GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS];
    float slope;
    float post_slope;
} gvx_hifigan_dims;
typedef struct gvx_hifigan gvx_hifigan;
size_t gvx_hifigan_blob_floats(const gvx_hifigan_dims* dims);
size_t gvx_hifigan_workspace_bytes(const gvx_hifigan_dims* dims, int B, int T);
int gvx_hifigan_pack_weights_device(const gvx_hifigan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_hifigan_create(const gvx_hifigan_dims* dims, gvx_hifigan** out);
void gvx_hifigan_destroy(gvx_hifigan* handle);
int gvx_hifigan_bind(gvx_hifigan* handle, const float* device_blob);
int gvx_hifigan_forward(gvx_hifigan* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out,
                        float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_hifigan_timing_enable(gvx_hifigan* handle, int enable);
int gvx_hifigan_stage_times_ms(gvx_hifigan* handle, float* ms_out, int* n_out);

/* HiFi-GAN generator: training.  A forward that keeps a tape, and the backward: the calls of "Training the generator" above (MelGAN),
 * with their contracts, argument order and error codes, for the network of gvx_hifigan_forward.  Kernels: csrc/hifigan_train.hip and
 * csrc/hifigan_kernels.h; all arithmetic is fp32; training is on plain weights.
 *
 * Tape: the caller's memory, 256-byte aligned, gvx_hifigan_tape_bytes (host arithmetic) long.  It holds every tensor the backward
 * reads, in forward order, which gvx_hifigan_tape_layout (host arithmetic) lists as (byte offset, positions per frame, channels):
 *     the transposed mel [round4(n_mels) channels];  conv_pre's output;
 *     per stage: ups.<i>'s output;  per residual block, per dilation m: the inner tensor (convs1.<m>'s output, resblock 1 only), then the
 *     block's running value after dilation m, for every m but the last;  the stage's average.
 * The last dilation's y_j is not kept: the forward adds it straight into the stage's sum, which is the average's slot, and its gradient
 * is d(sum) / n_k whatever its value.  That is 2 + n_k * (n_dilations * convs per dilation - 1) tensors per stage: 17 for resblock 1 with
 * three kernels, 5 for resblock 2.  Each is fp32, RAW pre-activation values, channels-last [B][T * positions per frame][channels] with
 * rows strided by the padded T, and starts where the one before it ends: the tape is 4 * B * T * F bytes, F = round4(n_mels) + C_0 + the
 * sum over the stages of that count * rates[0] * .. * rates[i] * C_{i+1}.  V1: F = 80 + 512 + 17 * (2048 + 3 * 8192) = 453,200 floats,
 * 1,812,800 bytes per frame and row.  Linear in B and in T.  Behind a row's own length the tape holds whatever it held before: the
 * backward reads nothing there.  The layout call returns the number of entries and fills at most max_entries of them (entries may be
 * NULL); both return 0 for refused dims, B outside [1, 65535] or T outside [1, GVX_HIFIGAN_MAX_FRAMES].
 *
 * gvx_hifigan_forward_train is the forward with every layer writing into its own tape slot - the same kernels with the same arguments
 * (the in-place write of convs2's output becomes a write beside its residual input, which the kernel reads element by element), so
 * wav_out has the bits of gvx_hifigan_forward.  It needs no scratch: workspace may be NULL and workspace_bytes 0.
 *
 * gvx_hifigan_backward: d_wav fp32 [B][T * hop], never read at or behind sample T_b * hop.  grads is a HOST table that names DEVICE
 * destinations under the packer's names; every parameter gradient is WRITTEN (not accumulated) in PyTorch's own layout: Conv1d
 * [out][in][k] (conv_pre without padded channels), ConvTranspose1d [in][out][2 r].  d_mel_out is NULL (the first layer's data gradient is
 * skipped; no parameter gradient changes a bit) or fp32 [B][n_mels][T], exactly 0 at and behind a row's frames; row b of it has the bits
 * of that row run alone.  A LeakyReLU's derivative is decided by `v > 0` on the tape value, as the forward decides it.  Refused before
 * anything is launched: a missing name (GVX_ERR_MISSING_WEIGHT), a wrong element count or NULL destination (GVX_ERR_SHAPE), a NULL,
 * short or misaligned tape or workspace (GVX_ERR_WORKSPACE), T or B as the forward refuses them, B * ceil(T * hop / 512) above
 * GVX_HIFIGAN_MAX_TRAIN_PIECES (GVX_ERR_UNSUPPORTED).  gvx_hifigan_backward_workspace_bytes is host arithmetic and exact: any contents
 * when the call starts, nothing is cleared; it holds the transposed weights (made from the bound blob at the start of every call, so
 * never stale), the waveform and its pre-tanh gradient, five activation-gradient tensors of the widest stage, and the partial products
 * of the widest weight gradient and of the widest bias gradient.
 *
 * The backward is a chain of ordinary launches.  A data gradient is the forward's own windowed kernel with dY as the operand and the
 * transposed, tap-reversed weights (a transposed convolution as a 3-tap convolution over its output read as [len][r C]); the epilogue
 * applies lrelu', the residual path's gradient and the 1 / n_k of a stage's average.  Weight and bias gradients are reduced per row in
 * pieces of 512 positions - a row of T * m positions has ceil(T * m / 512) of them - on v_mfma_f32_32x32x2_f32 where the layer has 32
 * output channels or more, every tap off one activated source window in LDS, and the partial products are added in a fixed order.  No
 * float atomics: two calls give the same bits.
 *
 * Timing (measurement only): with gvx_hifigan_timing_enable on, gvx_hifigan_backward_stage_times_ms gives the last backward call's
 * n_stages + 3 durations in the order they ran: the weight transposes, conv_post, every stage from the last to the first, conv_pre. */
enum { GVX_HIFIGAN_MAX_TRAIN_PIECES = 1 << 24 };
typedef gvx_melgan_tape_entry gvx_hifigan_tape_entry;
size_t gvx_hifigan_tape_bytes(const gvx_hifigan_dims* dims, int B, int T);
int gvx_hifigan_tape_layout(const gvx_hifigan_dims* dims, int B, int T, gvx_hifigan_tape_entry* entries, int max_entries);
size_t gvx_hifigan_backward_workspace_bytes(const gvx_hifigan_dims* dims, int B, int T);
int gvx_hifigan_forward_train(gvx_hifigan* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, void* tape,
                              size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_hifigan_backward(gvx_hifigan* handle, const float* d_wav, const int32_t* frame_lengths, int B, int T, const void* tape,
                         size_t tape_bytes, const gvx_grad_desc* grads, int n_grads, float* d_mel_out, void* workspace,
                         size_t workspace_bytes, void* stream);
int gvx_hifigan_backward_stage_times_ms(gvx_hifigan* handle, float* ms_out, int* n_out);

/* gvx_hifigan_layer is ONE layer of the generators above on its own - the launch that gvx_hifigan_forward, gvx_bigvgan_forward,
 * gvx_univnet_forward's convolutions and gvx_hifigan_backward's data gradients are chains of - with the kernel picked as they have it
 * picked: Cout >= 32 and Cin a multiple of 4 run on v_mfma_f32_32x32x2_f32 with 128 positions x 128 (Cout >= 128), 64 (Cout > 32) or 32
 * channels per workgroup, every other layer on fmaf dot products (8 lanes per element where Cout == 1).  No handle, no workspace; the
 * launch goes to `stream`.  All tensors are fp32, channels-last, on the device, 16-byte aligned; L = T * in_mul positions per row.
 *
 * gradient == 0, a forward layer:  src [B][L][Cin] -> out [B][L * phases][Cout],
 *     out[b][phases q + phase][n] = E( bias[n] + sum over taps tau, channels c of a(src[b][pos(q, phase, tau)][c]) * W[phase][n][tau][c] )
 * with a = lrelu(., slope) if act, else the identity; zeros for positions outside the row's own [0, len_b), len_b = min(lens[b], T) *
 * in_mul (lens int32 [B] on the device, counted in units of in_mul positions; NULL: every row has L); and the epilogue E, in this order:
 * + res[b][q][n] (res [B][L][Cout] or NULL), + what out held (accumulate), / divide (divide > 0), tanh (tanh_out).
 *   phases == 1, a convolution: taps odd, pos = q - (taps - 1) dil / 2 + tau dil.  From PyTorch's Conv1d weight w [Cout][Cin][taps]:
 *       W[0][n][tau][c] = w[n][c][tau], that is w.permute(0, 2, 1).
 *   phases == r > 1, ConvTranspose1d(kernel 2 r, stride r, padding r / 2), r even: taps = 2 (dil is not read); tap 0 reads position q,
 *       tap 1 position q - 1 where phase < r / 2 and q + 1 otherwise.  From PyTorch's weight w [Cin][Cout][2 r]:
 *       W[phase][n][0][c] = w[c][n][phase + r / 2];  W[phase][n][1][c] = w[c][n][phase + r / 2 + r] (phase < r / 2), w[c][n][phase - r / 2] (else).
 * Behind a row (positions >= len_b) out is written with exact zeros if zero_tail, and left as it was otherwise; src, res and out are not
 * read there.  out may be res (an element is read and written by one lane); out must not be src.
 *
 * gradient != 0, a data gradient (phases == 1; bias NULL; act, accumulate, zero_tail, tanh_out 0): src is dY [B][L][Cin], out is dX
 * [B][L][Cout], the same windowed product without a bias on the TRANSPOSED, tap-reversed weights - for a forward convolution w [N][C][k]
 * (dY has Cin = N channels, dX has Cout = C):  W[0][c][tau][n] = w[n][c][k - 1 - tau], that is w.flip(2).permute(1, 2, 0) - and the epilogue
 *     dX = ( (mask ? (mask > 0 ? v : v * slope) : v) + res + add2 ) / divide
 * with mask (the raw tensor whose LeakyReLU the gradient passes through), res and add2 each [B][L][Cout] or NULL; nothing is written
 * behind a row.
 *
 * Refused with GVX_ERR_INVALID_ARG before anything is launched: a NULL src, W or out (or bias, forward); a misaligned pointer; out == src;
 * B outside [1, 65535]; T or in_mul below 1, T * in_mul above 2^24 or T * in_mul * Cout above 2^28; Cin or Cout outside [1, 4096]; phases
 * outside [1, 64] or odd above 1; phases > 1 with taps != 2 or with a residual; phases == 1 with even taps, dil < 1 or (taps - 1) * dil >
 * GVX_HIFIGAN_MAX_WINDOW; slope outside [0, 1]; divide negative or not finite; tanh_out on the matrix kernels (which have none: it is
 * the output layer's); mask or add2 in a forward call; anything a data gradient does not take.  Cin that is no multiple of 4 is NOT
 * refused at any Cout: such a layer runs on the dot-product kernel.  The kernels' dynamic-LDS sizes are set once per process, at the
 * first call and on the device current then: the entry is for one device per process, and if that first preparation fails every later
 * call returns its error. */
int gvx_hifigan_layer(const float* src, const float* W, const float* bias, const float* res, const float* mask, const float* add2, float* out,
                      const int32_t* lens, int B, int T, int in_mul, int Cin, int Cout, int taps, int dil, int phases, int act, int accumulate,
                      float divide, int zero_tail, int tanh_out, float slope, int gradient, void* stream);

/* ---- BigVGAN generator, mel -> waveform (Lee et al. 2023; bigvgan_base_22khz_80band, bigvgan_22khz_80band and their kin): inference.
 * The reference ships no such model; the network below is the published implementation's, under its names.  It is HiFi-GAN's
 * generator (above) with every LeakyReLU replaced by an anti-aliased periodic activation A, and no activation in front of the
 * transposed convolutions.  Kernels: csrc/bigvgan.hip (the activation, the C ABI) on csrc/hifigan_kernels.h (every convolution, with
 * its operand taken as it is); all arithmetic is fp32.  `net` holds the structure with gvx_hifigan_dims's meaning and ranges; its two
 * slopes are not read.
 *
 *     x = Conv1d(n_mels -> C_0, k = 7, padding 3)(mel)                                                       conv_pre
 *     for stage i, r = upsample_rates[i]:
 *         x = ConvTranspose1d(C_i -> C_{i+1}, kernel 2 r, stride r, padding r / 2)(x)                        ups.<i>.0, length times r
 *         y_j = resblocks.<i * n_k + j>(x) for j = 0 .. n_k - 1;   x = (y_0 + y_1 + ..) / n_k                 added in that order, then divided
 *     x = Conv1d(C_last -> 1, k = 7, padding 3)(A_post(x))                                                   activation_post, conv_post
 *     wav = tanh_at_final ? tanh(x) : min(max(x, -1), 1)                 conv_post has no bias when bias_at_final is 0
 *
 *     resblock 1 (AMPBlock1), m = 0 .. 2:  x = x + convs2.<m>(A_{2m+1}(convs1.<m>(A_{2m}(x))))    convs1: dilation d_m; convs2: dilation 1
 *     resblock 2 (AMPBlock2), m = 0 .. 1:  x = x + convs.<m>(A_m(x))                              dilation d_m
 *
 * The activation A, per channel c over a row of n >= 1 positions, with the fixed 12-tap filter f (a Kaiser-windowed sinc of cutoff
 * 0.25 and half-width 0.3, window beta = 0.1102 * (2.285 * 5 * pi * 1.2 + 7.95 - 8.7), normalised to sum 1; the CALLER computes it in
 * float64 and hands it over as fp32):
 *     u[m] = 2 * sum_i xp[i] * f[m + 13 - 2 i],   xp[i] = x[clamp(i - 4, 0, n - 1)],   0 <= m < 2 n         2x upsample, replicate padding
 *     z[m] = u[m] + g_c * sin(a_c * u[m])^2                                                                  Snake
 *     y[t] = sum_{j = 0 .. 11} f[j] * z[clamp(2 t + j - 5, 0, 2 n - 1)],   0 <= t < n                        2x low-pass downsample
 * z is REPEATED beyond the row's ends, not recomputed from padded x.  y[t] depends on x[t - 5 .. t + 5].  a_c and g_c are per-channel
 * constants the caller derives from the checkpoint's alpha and beta: a = exp(alpha) (snake_logscale) or alpha; g = 1 / (a + 1e-9)
 * ("snake") or 1 / (b + 1e-9) with b = exp(beta) or beta ("snakebeta").
 *
 * gvx_snake_antialiased is A on its own: x and out fp32 [B][n_max][C] channels-last (out must not be x), lens int32 [B] on the device
 * or NULL for all n_max, f fp32 [12], a and g fp32 [C], all on the device.  One launch: a workgroup of 256 threads owns
 * GVX_BIGVGAN_ACT_TILE positions of one row by a block of up to 64 channels, lanes along the channels; it stages x[t0 - 6 .. t0 + P + 5]
 * in LDS with both ends clamped to the row, forms the z pairs (2 q, 2 q + 1) of q = t0 - 3 .. t0 + P + 2 ONCE (u polyphase: six taps of f
 * for even m, six for odd m, over seven shared values of x) into LDS, then every y.  No atomics; a row's result depends on that row alone, so a ragged row has the bits of its one-row
 * run, and two calls give the same bits.  out is written as exact ZEROS at and behind a row's length, up to n_max; x is never read there.
 * lens[b] is clamped to [0, n_max].  B outside [1, 65535], n_max < 1, C < 1, n_max above GVX_BIGVGAN_ACT_MAX_POSITIONS or a NULL
 * pointer: GVX_ERR_INVALID_ARG.
 *
 * Weights.  gvx_bigvgan_pack_weights_device reads DEVICE pointers by name: every convolution as gvx_hifigan_pack_weights_device reads
 * it (ups.<i>.weight / .bias: the caller strips the published ".0"; conv_post.bias is zeros when the model has none), and
 *     filter [12];   resblocks.<n>.activations.<p>.a / .g [C];   activation_post.a / .g [C_last]
 * The blob is gvx_hifigan_blob_floats(net) floats in that call's layout - written by that call - followed by the filter and every a and
 * g in network order, each starting at a multiple of 64 floats.  Errors as there.
 *
 * Workspace: gvx_bigvgan_workspace_bytes is host arithmetic:  B * ( round256(4 * T * round4(n_mels)) + 5 * round256(4 * T * W) ), W as
 * for HiFi-GAN: its four tensors and the activation's output.  The same contract: any contents when the call starts, nothing is cleared.
 *
 * gvx_bigvgan_forward: gvx_hifigan_forward's arguments, contracts and error codes; one launch per convolution and one per activation
 * (the clamp of tanh_at_final = 0 is one more).  Ragged rows as there: row b has the bits of that row run alone, wav is exactly 0 from
 * sample T_b * hop on.  Timing as gvx_hifigan_timing_enable / gvx_hifigan_stage_times_ms: n_stages + 2 durations, the last one
 * activation_post with conv_post.  There is no backward. */
enum { GVX_BIGVGAN_FILTER_TAPS = 12, GVX_BIGVGAN_ACT_TILE = 32, GVX_BIGVGAN_ACT_MAX_POSITIONS = 1 << 28 };
typedef struct gvx_bigvgan_dims {
    gvx_hifigan_dims net;
    int32_t snakebeta;       /* 1: "snakebeta", 0: "snake" (names the tensors the caller derives g from; the kernels see a and g) */
    int32_t tanh_at_final;   /* 1: tanh, 0: clamp to [-1, 1] */
    int32_t bias_at_final;   /* 0: conv_post has no bias (the caller hands zeros) */
} gvx_bigvgan_dims;
typedef struct gvx_bigvgan gvx_bigvgan;
int gvx_snake_antialiased(const float* x, const int32_t* lens, int B, int n_max, int C, const float* f, const float* a, const float* g,
                          float* out, void* stream);
size_t gvx_bigvgan_blob_floats(const gvx_bigvgan_dims* dims);
size_t gvx_bigvgan_workspace_bytes(const gvx_bigvgan_dims* dims, int B, int T);
int gvx_bigvgan_pack_weights_device(const gvx_bigvgan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_bigvgan_create(const gvx_bigvgan_dims* dims, gvx_bigvgan** out);
void gvx_bigvgan_destroy(gvx_bigvgan* handle);
int gvx_bigvgan_bind(gvx_bigvgan* handle, const float* device_blob);
int gvx_bigvgan_forward(gvx_bigvgan* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out,
                        float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_bigvgan_timing_enable(gvx_bigvgan* handle, int enable);
int gvx_bigvgan_stage_times_ms(gvx_bigvgan* handle, float* ms_out, int* n_out);

/* ---- Vocos generator, mel -> waveform (Siuzdak 2023; charactr/vocos-mel-24khz): inference.  The reference ships no such model; the
 * network below is the published implementation's mel variant, under its names.  A ConvNeXt backbone at the FRAME rate and an inverse
 * STFT: nothing runs at the sample rate but the transform.  Kernels: csrc/vocos.hip (filter + LayerNorm, the ISTFT frame, the
 * overlap-add, the C ABI) on the dense fp32 GEMM (csrc/gemm_f32.hip: every product) and the in-LDS FFT (csrc/fft_lds.h).  All arithmetic
 * is fp32; every tensor is channels-last [B][T][C].  N = n_fft, H = N / 2, LN = LayerNorm over the channels of a frame with eps 1e-6.
 *
 *     x = LN_norm(Conv1d(n_mels -> dim, k = 7, padding 3)(mel))                                              backbone.embed, backbone.norm
 *     for i < num_layers:   x = x + gamma_i * pwconv2_i(GELU(pwconv1_i(LN_i(dwconv_i(x)))))                  backbone.convnext.<i>
 *             dwconv: Conv1d(dim, dim, 7, padding 3, groups = dim);  pwconv1: Linear(dim, intermediate_dim);  GELU: the erf form
 *     y = Linear(dim -> N + 2)(LN_final(x));   m = y[0 .. H],  p = y[H + 1 .. N + 1]                         backbone.final_layer_norm, head.out
 *     S = min(exp(m), 100) * (cos p + i sin p);   frame = window * irfft(S, N)       (the 1 / N of the backward norm; periodic Hann of N)
 *     wav = overlap-add of the frames at stride hop / overlap-add of window^2, trimmed by `pad` samples at either end:
 *         center = 0 ("same"):   pad = (N - hop) / 2,  a row of T_b frames gives T_b * hop samples
 *         center = 1 ("center"): pad = N / 2,          a row of T_b frames gives (T_b - 1) * hop samples, T_b >= 2   (torch.istft, center = True)
 *
 * Contracts, as for the other generators: every row runs at its own length frame_lengths[b] (NULL: all T); wav [B][T * hop] holds a
 * row's samples in front and exact ZEROS behind them; the padded frames of mel may hold anything, NaN included, and are never read;
 * every stage tensor is zeros at and behind a row's frames; no atomics, and every product sums its k in an order that does not depend
 * on the tile shape or on M, so a row of a ragged batch has, bit for bit, the result of that row run alone.
 *
 * gvx_dwconv_layernorm is "k = 7 channel-wise filter, then LayerNorm" on its own: x and out fp32 [B][T][C] (out must not be x), lens
 * int32 [B] on the device or NULL, taps 7 or 0 (0: the LayerNorm alone; w and b are not read), w fp32 [7][C] TAP-major
 * (w[j][c] multiplies x[t + j - 3][c]), b, ln_w, ln_b fp32 [C].  A workgroup of four waves owns GVX_VOCOS_TILE frames of a row; the
 * tile's P + 6 input frames go into LDS once, with zeros for frames outside [0, T_b); a wave owns one frame at a time, lanes along the
 * channels (lane l holds channels l, l + 64, ..), and forms mean and variance as two passes over its registers (the mean first, then
 * the squared deviations), each a butterfly over the wave.  out is zeros at and behind T_b; x is never read there.  C must be a
 * multiple of 4 in [4, GVX_VOCOS_MAX_DIM], B in [1, 65535], T in [1, GVX_VOCOS_MAX_FRAMES]: GVX_ERR_INVALID_ARG otherwise.
 *
 * gvx_istft_head is the head behind its Linear: coeffs fp32 [B][T][N + 2] -> wav_out fp32 [B][T * hop].  N in {512, 1024, 2048}, hop in
 * [N / 8, N / 2] with N - hop even, center 0 or 1, window fp32 [N] on the device.  vc_istft_kernel takes a frame per wave: exp, the
 * clamp, sincosf and the product in registers, the pack into the H-point complex transform, the inverse transform in LDS, 1 / N and the
 * window; the frame goes to the workspace.  vc_ola_kernel gathers each sample's frames in ascending frame order, divides by the envelope
 * of the row's own T_b frames summed in the same order, applies the trim and writes zeros behind the row's samples.  The workspace holds
 * the frames and the call's twiddle tables (computed in float64 on the device at every call): gvx_istft_head_workspace_bytes =
 * round256(4 * B * T * N) + round256(8 * (N + 1)); 256-byte aligned, any contents.
 *
 * Weights.  gvx_vocos_pack_weights_device copies DEVICE tensors by name into the blob, every tensor starting at a multiple of 64 floats,
 * in this order (Cp = n_mels rounded up to a multiple of 4, L = num_layers, I = intermediate_dim):
 *     embed.weight [dim][7][Cp] (tap-major rows, zero channel padding)   embed.bias [dim]   norm.weight, norm.bias [dim]
 *     per layer i: convnext.<i>.dwconv.weight [7][dim]  .dwconv.bias [dim]  .norm.weight, .norm.bias [dim]  .pwconv1.weight [I][dim]
 *                  .pwconv1.bias [I]  .pwconv2.weight [dim][I]  .pwconv2.bias [dim]    (pwconv2 with gamma_i folded in by the caller)
 *     final_layer_norm.weight, .bias [dim]   head.weight [N + 2][dim]   head.bias [N + 2]
 * followed by the window [N] and the twiddles w_H^m [H] and w_N^k [H + 1] as float2, which the call computes itself in float64:
 *     blob_floats = r(7 dim Cp) + 3 r(dim) + L (r(7 dim) + 4 r(dim) + 2 r(I dim) + r(I)) + 2 r(dim) + r((N + 2) dim) + r(N + 2)
 *                   + r(N) + r(2 H) + r(2 (H + 1)),   r = round up to 64.
 * A missing name: GVX_ERR_MISSING_WEIGHT; a wrong element count: GVX_ERR_SHAPE.
 *
 * Workspace: gvx_vocos_workspace_bytes is host arithmetic:
 *     B * ( round256(4 (T + 6) Cp) + 2 round256(4 T dim) + round256(4 T I) + round256(4 T (N + 2)) + round256(4 T N) )
 * the mel with its 3-frame zero halo, x and the A operand, the MLP's hidden tensor, the head product and the frames: 18,840 bytes per
 * frame and row for the default model with 100 mels (and 2,400 per row for the halo).  Any contents when the call starts, nothing is cleared.
 *
 * gvx_vocos_forward: mel fp32 [B][n_mels][T] -> wav_out [B][T * hop_length].  stage_out, if not NULL: num_layers + 3 device tensors,
 * x after embed + norm, after every block and after the final norm ([B][T][dim] each), then the head product [B][T][N + 2].  T below
 * 1 + center: GVX_ERR_INVALID_ARG; the workspace missing, misaligned or short: GVX_ERR_WORKSPACE.  Launches: one transpose, the embed
 * product, per LayerNorm or filter + LayerNorm one, per product one (two where the GEMM's plan covers the rows with two tile shapes),
 * the frame kernel and the gather.  gvx_vocos_stage_times_ms: four durations - embed + norm, the blocks, final norm + head product,
 * the ISTFT.  Every dims field is checked: a bad one gives blob_floats == 0 and create == GVX_ERR_INVALID_ARG.  The backward is
 * "Vocos generator: training" below. */
enum { GVX_VOCOS_TILE = 16, GVX_VOCOS_MAX_DIM = 512, GVX_VOCOS_MAX_INTERMEDIATE = 8192, GVX_VOCOS_MAX_LAYERS = 64, GVX_VOCOS_MAX_FRAMES = 1 << 20 };
typedef struct gvx_vocos_dims {
    int32_t n_mels;             /* >= 1 */
    int32_t dim;                /* a multiple of 32 in [32, GVX_VOCOS_MAX_DIM]: the filter + LayerNorm tile's LDS */
    int32_t intermediate_dim;   /* a multiple of 32 in [32, GVX_VOCOS_MAX_INTERMEDIATE] */
    int32_t num_layers;         /* in [1, GVX_VOCOS_MAX_LAYERS] */
    int32_t n_fft;              /* 512, 1024 or 2048 */
    int32_t hop_length;         /* in [n_fft / 8, n_fft / 2], n_fft - hop_length even */
    int32_t center;             /* 1: padding "center", 0: padding "same" */
} gvx_vocos_dims;
typedef struct gvx_vocos gvx_vocos;
int gvx_dwconv_layernorm(const float* x, const int32_t* lens, int B, int T, int C, int taps, const float* w, const float* b,
                         const float* ln_w, const float* ln_b, float eps, float* out, void* stream);
size_t gvx_istft_head_workspace_bytes(int B, int T, int n_fft);
int gvx_istft_head(const float* coeffs, const int32_t* lens, int B, int T, int n_fft, int hop, int center, const float* window,
                   void* workspace, float* wav_out, void* stream);
size_t gvx_vocos_blob_floats(const gvx_vocos_dims* dims);
size_t gvx_vocos_workspace_bytes(const gvx_vocos_dims* dims, int B, int T);
int gvx_vocos_pack_weights_device(const gvx_vocos_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_vocos_create(const gvx_vocos_dims* dims, gvx_vocos** out);
void gvx_vocos_destroy(gvx_vocos* handle);
int gvx_vocos_bind(gvx_vocos* handle, const float* device_blob);
int gvx_vocos_forward(gvx_vocos* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out,
                      float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_vocos_timing_enable(gvx_vocos* handle, int enable);
int gvx_vocos_stage_times_ms(gvx_vocos* handle, float* ms_out, int* n_out);

/* Vocos generator: training.  A forward that keeps a tape, and the backward: the calls of "HiFi-GAN generator: training" above, with
 * their argument order and error codes, for the network of gvx_vocos_forward.  Kernels: csrc/vocos_train.hip on the dense fp32 GEMM
 * (csrc/gemm_f32.hip) and the in-LDS FFT (csrc/fft_lds.h); all arithmetic is fp32 (sums ACROSS pieces and launch_col_reduce's add in
 * float64, in a fixed order); no float atomics: two calls give the same bits.  Every launch treats ragged rows as its forward twin
 * does: frames at and behind a row's length are written as exact zeros and nothing is read there, in the activations or in the incoming
 * gradient.  The inference blob, the inference workspace and gvx_vocos_forward are as above, bit for bit.
 *
 * gvx_dwconv_layernorm_backward is the twin of gvx_dwconv_layernorm on its own.  x (the layer's input), dy (the gradient at the
 * LayerNorm's output) and dx fp32 [B][T][C]; d_res (the residual path's gradient, added to dx) [B][T][C] or NULL, and may be dx itself; w
 * fp32 [7][C] TAP-major and b [C] as the forward takes them, ln_w [C]; taps 7 or 0 (0: the plain LayerNorm backward; w, b, d_w, d_b are not
 * used).  It recomputes u = dwconv(x) + b and its statistics with the forward's own two passes over registers (an offset of 1e3 does not
 * cost the digits of xh), forms du = rstd (dxh - mean(dxh) - xh mean(dxh xh)) with dxh = dy ln_w, and writes
 *     dx[t] = d_res[t] + sum_j w[j] du[t + 3 - j],   d_ln_w = sum dy xh,   d_ln_b = sum dy,   d_w[c][0][j] = sum_t du[t] x[t + j - 3],   d_b = sum_t du
 * d_w in PyTorch's layout [C][1][7].  Decomposition: vcb_ln_kernel - a workgroup of four waves per piece of GVX_VOCOS_GRAD_PIECE frames of
 * one row (not per GVX_VOCOS_TILE frames as the forward: the piece's sums stay in registers), wave w taking frames w, w + 4, .. of the
 * piece, lanes along the channels, 1 / 2 / 4 / 8 channels per lane, the filter's inputs read from memory without an LDS tile - writes du
 * (taps 0: dx) and the piece's partial sums; vcb_dw_kernel - a wave per 64 channels of a piece - the filter's adjoint and the piece's d_w;
 * vcb_sum_kernel adds the pieces in piece order.  A piece wholly behind its row writes zeros over whatever the workspace held.
 * GVX_VOCOS_GRAD_PIECE is 128: at 32 x 800 frames that is 224 workgroups for the 256 compute units, where 256 frames would give 128.
 * Workspace (gvx_dwconv_layernorm_backward_workspace_bytes, host arithmetic, exact, 0 for refused shapes):
 *     round256(4 * B * ceil(T / GVX_VOCOS_GRAD_PIECE) * 10 * C) + (taps ? round256(4 * B * T * C) : 0)        the partials, then du
 *
 * gvx_istft_head_backward is the twin of gvx_istft_head on its own: coeffs [B][T][N + 2] and d_wav [B][T * hop] -> d_coeffs [B][T][N + 2].
 * The adjoint of the overlap-add is a gather: vcb_env_kernel writes d_wav / envelope inside a row's delivered samples and 0 behind them
 * (d_wav is not read there); vcb_istft_kernel takes a frame per wave, reads its n_fft positions through the trim of the padding mode,
 * applies the window and 1 / N, runs the forward real transform X in LDS, and with c_0 = c_H = 1, c_k = 2 otherwise
 *     dRe = c_k Re X_k,  dIm = c_k Im X_k (0 at DC and Nyquist);   d p = mag (-dRe sin p + dIm cos p);
 *     d m = (dRe cos p + dIm sin p) mag  where the device's own expf(m) <= 100, else 0                        (torch.clip's gradient)
 * mag, cos and sin recomputed from coeffs as the forward computes them.  No spectrum goes to memory.  Workspace
 * (gvx_istft_head_backward_workspace_bytes): round256(4 * B * T * hop) + round256(8 * (N + 1)), d_wav / envelope and the twiddles.
 *
 * Tape: the caller's memory, 256-byte aligned, gvx_vocos_tape_bytes (host arithmetic, exact) long; gvx_vocos_tape_layout lists its
 * tensors in forward order as (byte offset, rows per batch row, channels), each fp32 [B][rows][channels], one starting where the one
 * before it ends:
 *     the transposed mel with its 3-frame zero halo [T + 6][Cp];  the embedding's output [T][dim];  x in front of the first block [T][dim];
 *     per block: its pre-GELU p [T][I], then x behind it [T][dim];  the head product [T][N + 2]
 *     tape_bytes = 4 * B * ( (T + 6) Cp + T ( (L + 2) dim + L I + N + 2 ) )
 * - 4 + 2 L entries; 74,136 bytes per frame and row for the default model with 100 mels (and 2,400 per row for the halo).  The LayerNorm
 * outputs and h = gelu(p) are NOT kept: the backward recomputes each into its workspace with the forward's own kernel (one more
 * elementwise launch per block, against 8,192 more bytes per frame, row and block).  Every tape tensor holds exact zeros at and behind a
 * row's length.  Both calls return 0 for refused dims, B outside [1, 65535], T outside [1 + center, GVX_VOCOS_MAX_FRAMES].
 *
 * gvx_vocos_forward_train is the forward with every kept tensor written into its tape slot - the same kernels with the same arguments,
 * except that pwconv1 runs with its bias only into the tape and one elementwise launch of the same gelu function (csrc/gelu.h) follows it -
 * so wav_out has the bits of gvx_vocos_forward.  Its workspace is gvx_vocos_workspace_bytes (the LayerNorm output, h and the frames).
 *
 * gvx_vocos_backward: d_wav fp32 [B][T * hop], never read at or behind a row's delivered samples.  grads is a HOST table that names DEVICE
 * destinations under the PUBLISHED state-dict names (backbone.embed.weight .. head.out.bias: what named_parameters() gives); every
 * parameter gradient is WRITTEN (not accumulated) in PyTorch's own layout: embed.weight [dim][n_mels][7] without the channel padding,
 * dwconv.weight [dim][1][7].  The blob holds only gamma (.) pwconv2, so `raw` - a HOST table in front of grads - names the DEVICE tensors
 * of the three unfolded parameters of every block (backbone.convnext.<i>.gamma, .pwconv2.weight, .pwconv2.bias); the products give dW2'
 * and db2' with respect to the folded tensors and vcb_unfold_kernel turns them into
 *     dW2 = gamma (.) dW2',   db2 = gamma (.) db2',   d gamma[c] = sum_i dW2'[c][i] W2[c][i] + db2'[c] b2[c]
 * without a division: a gamma element of 0 gives the right gradient.  d_mel_out is NULL (the embedding's data gradient is skipped; no
 * parameter gradient changes a bit) or fp32 [B][n_mels][T], exactly 0 at and behind a row's frames; row b of it has the bits of that row
 * run alone.  Refused before anything is launched: a missing name (GVX_ERR_MISSING_WEIGHT), a wrong element count or NULL destination
 * (GVX_ERR_SHAPE), a NULL, short or misaligned tape or workspace (GVX_ERR_WORKSPACE), B or T as the forward refuses them, T below
 * 1 + center (GVX_ERR_INVALID_ARG).
 *
 * The backward is a chain of ordinary launches.  Data gradients are launch_gemm with row_len on weights transposed from the bound blob at
 * the start of every call (never stale); the head's K of N + 2 is padded to a multiple of 4 with zero columns in d_coeffs and in the
 * transposed head weight.  Weight gradients are the GEMM's K-major form over all B * T frames with split-K partials in the workspace,
 * added in split order; the embedding's reads the haloed mel through a two-level row map.  Bias gradients are launch_col_reduce.
 * gvx_vocos_backward_workspace_bytes is host arithmetic and exact, any contents when the call starts: with Np = N + 2 rounded up to 4,
 * the transposed weights (dim Np + 2 L dim I + 7 dim Cp floats), d_wav / envelope, d_coeffs [B T][Np], the recomputed LayerNorm output and
 * h, dp, three [B T][dim] gradient tensors, the embedding's gradient with its halo, d_mel channels-last, (L + 2) sets of LayerNorm
 * partials, dW2' and db2' of every block, one padded weight gradient and the split-K partials, each rounded up to 256 bytes.
 *
 * Timing (measurement only): with gvx_vocos_timing_enable on, gvx_vocos_backward_stage_times_ms gives the last backward call's four
 * durations in the order they ran: the weight transposes + ISTFT + head, the blocks, embed + norm, the pieces' sums and the unfold. */
enum { GVX_VOCOS_GRAD_PIECE = 128 };
typedef struct gvx_vocos_tape_entry {
    uint64_t byte_offset;
    int32_t rows;       /* per batch row: T, or T + 6 for the haloed mel */
    int32_t channels;
} gvx_vocos_tape_entry;
size_t gvx_dwconv_layernorm_backward_workspace_bytes(int B, int T, int C, int taps);
int gvx_dwconv_layernorm_backward(const float* x, const float* dy, const float* d_res, const int32_t* lens, int B, int T, int C, int taps,
                                  const float* w, const float* b, const float* ln_w, float eps, float* dx, float* d_w, float* d_b,
                                  float* d_ln_w, float* d_ln_b, void* workspace, size_t workspace_bytes, void* stream);
size_t gvx_istft_head_backward_workspace_bytes(int B, int T, int n_fft, int hop);
int gvx_istft_head_backward(const float* coeffs, const float* d_wav, const int32_t* lens, int B, int T, int n_fft, int hop, int center,
                            const float* window, void* workspace, size_t workspace_bytes, float* d_coeffs, void* stream);
size_t gvx_vocos_tape_bytes(const gvx_vocos_dims* dims, int B, int T);
int gvx_vocos_tape_layout(const gvx_vocos_dims* dims, int B, int T, gvx_vocos_tape_entry* entries, int max_entries);
size_t gvx_vocos_backward_workspace_bytes(const gvx_vocos_dims* dims, int B, int T);
int gvx_vocos_forward_train(gvx_vocos* handle, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, void* tape,
                            size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_vocos_backward(gvx_vocos* handle, const float* d_wav, const int32_t* frame_lengths, int B, int T, const void* tape,
                       size_t tape_bytes, const gvx_weight_desc* raw, int n_raw, const gvx_grad_desc* grads, int n_grads, float* d_mel_out,
                       void* workspace, size_t workspace_bytes, void* stream);
int gvx_vocos_backward_stage_times_ms(gvx_vocos* handle, float* ms_out, int* n_out);

/* ---- UnivNet generator, (mel, noise) -> waveform (Jang et al. 2021; the maum-ai/univnet implementation, c32 and c16): inference.  The
 * reference ships no such model; the network below is a statement of the published implementation, under its names, and the float64
 * restatement tests/univnet_ref64.py is the definition the device is held to.  A time-domain generator that upsamples NOISE at the frame
 * rate and conditions it on the mel through location-variable convolutions (LVC): a small network at the frame rate predicts, for every
 * frame, the weights of the convolutions that run on that frame's positions.  Kernels: csrc/univnet.hip (the LVC layer, the reflecting
 * output layer, the C ABI) on the dense fp32 GEMM (csrc/gemm_f32.hip: conv_pre, kernel_conv + bias_conv) and HiFi-GAN's layer kernels
 * (csrc/hifigan_kernels.h: the transposed and the dilated convolutions, the predictor's small convolutions).  All arithmetic is fp32;
 * every tensor is channels-last [B][len][C].  C = channel_size, H = kpnet_hidden_channels, D = n_dilations, lrelu = LeakyReLU(slope),
 * cum_i = strides[0] * .. * strides[i] positions per frame in block i, hop = cum_last.
 *
 *     x = Conv1d(noise_dim -> C, k = 7)(reflect 3 (z))                                                       conv_pre, at the frame rate
 *     for block i, s = strides[i]:                                                                           res_stack.<i>
 *         x = ConvTranspose1d(C -> C, kernel 2 s, stride s, padding s / 2)(lrelu(x))                         convt_pre.1, length times s
 *         c = lrelu(Conv1d(n_mels -> H, k = 5, padding 2)(mel))                                              kernel_predictor.input_conv.0
 *         for j < 3:  c = c + lrelu(Conv1d(H -> H, 3, padding 1)(lrelu(Conv1d(H -> H, 3, padding 1)(c))))    .residual_convs.<j>.1, .3
 *         kernels = Conv1d(H -> 6 C^2 D, 3, padding 1)(c) viewed as [D][C in][2 C out][3 taps] per frame     .kernel_conv
 *         bias    = Conv1d(H -> 2 C D, 3, padding 1)(c)   viewed as [D][2 C] per frame                       .bias_conv
 *         for m < D, d = dilations[m]:
 *             y = lrelu(Conv1d(C -> C, 3, dilation d, padding d)(lrelu(x)))                                  conv_blocks.<m>.1
 *             o[j][t cum + p] = bias[m][j][t] + sum_{i, k} kernels[m][i][j][k][t] * y[i][t cum + p + k - 1],   0 <= p < cum       the LVC
 *             x = x + sigmoid(o[0 .. C)) * tanh(o[C .. 2 C))
 *     wav = tanh(Conv1d(C -> 1, k = 7)(reflect 3 (lrelu(x))))                                                conv_post.1
 * Zero paddings and the LVC's zero outside [0, T_b cum) fall at a row's own end, and so do both reflections.  A row needs 4 frames:
 * frame_lengths lives on the device, so a value below 4 is the CALLER's to refuse (UnivNetGenerator does, before anything is launched);
 * handed to gvx_univnet_forward it reads or writes nothing out of bounds, that row's wav is silence, and its stage tensors are unspecified.
 *
 * Contracts, as for the other generators: every row runs at its own length frame_lengths[b] (NULL: all T); wav [B][T * hop] holds a
 * row's samples in front and exact ZEROS behind T_b * hop; the padded frames of mel AND noise may hold anything, NaN included, and are
 * never read; every stage tensor is zeros behind a row's positions; no atomics; a row of a ragged batch has, bit for bit, the result of
 * that row run alone, and two calls give the same bits.
 *
 * The device order of a block's prediction, per frame `ld = D (6 C^2 + 2 C)` floats: kernels [D][2 C][3][C] - layer m's operand is a
 * row-major [2 C][3 C] matrix, k = tap * C + i - and then bias [D][2 C].  kernel_conv and bias_conv are ONE product whose output
 * channels the caller permutes into this order when it packs (kernel_predictor.kb.weight [ld][3][H] tap-major, .kb.bias [ld]): the
 * [B][T][ld] result is the LVC kernel's operand as it stands, and nothing is permuted per call.
 *
 * gvx_lvc_gated is one layer on its own: x fp32 [B][T * cum][C] -> out, kern fp32 [B][T][n_layers (6 C^2 + 2 C)] in the device
 * order, of which layer `layer` is used; conv_w fp32 [C][3][C] (tap-major rows) and conv_b [C] of the dilated convolution, or both NULL:
 * then y = lrelu(x).  With a convolution, scratch fp32 [B][T * cum][C] (a tensor of its own) takes its output, and out may be x: an
 * element of x is then read and written by one lane.  Without one the layer reads x at its neighbours' positions, so out == x is refused
 * (GVX_ERR_INVALID_ARG).  lens counts frames, each in [0, T]; a row's positions behind T_b * cum are copied from x to out unread by the layer.  Two LVC kernels, one source
 * (un_lvc_kernel<MFMA>): a workgroup owns up to 128 positions of ONE frame, brings that frame's [2 C][3 C] weights and its window of y
 * (one position either side, lrelu applied, zeros outside the row) into LDS once, and
 *     C == 32 and cum a multiple of 32 (of 128 above 128):  v_mfma_f32_32x32x2_f32, a wave per 32 positions, the 2 C output channels as
 *         two 32-wide tiles whose column r is lane r: o[j] and o[j + C] meet in one lane, and bias, sigmoid * tanh and the residual
 *         add are that lane's epilogue;
 *     otherwise (C == 16; the first block, whose frames have 8 positions):  fmaf code, a thread per (position, gate pair).
 * T in [1, GVX_UNIVNET_MAX_FRAMES], cum in [1, 4096], C a multiple of 4 in [4, 32], dilation in [1, 36], B in [1, 65535]:
 * GVX_ERR_INVALID_ARG otherwise, before anything is launched.
 *
 * Weights.  gvx_univnet_pack_weights_device copies DEVICE tensors by name into the blob, every tensor starting at a multiple of 64
 * floats, in this order (Np = noise_dim and Mp = n_mels rounded up to a multiple of 4; the CALLER brings every tensor into the layout):
 *     conv_pre.weight [C][7][Np]   conv_pre.bias [C]
 *     per block i, res_stack.<i>. in front: convt_pre.weight [s][C][2][C] (phase, out, tap, in: hifigan.hip's two-tap phase split)
 *         convt_pre.bias [C]   kernel_predictor.input_conv.weight [H][5][Mp]  .bias [H]   kernel_predictor.residual_convs.<j>.<1 | 3>.weight
 *         [H][3][H]  .bias [H] for j < 3   kernel_predictor.kb.weight [ld][3][H]  .kb.bias [ld]   conv_blocks.<m>.weight [C][3][C]  .bias [C]
 *     conv_post.weight [7][C]   conv_post.bias [1]
 * A missing name: GVX_ERR_MISSING_WEIGHT; a wrong element count: GVX_ERR_SHAPE.
 *
 * Workspace: gvx_univnet_workspace_bytes is host arithmetic:
 *     B * ( round256(4 T Mp) + round256(4 (T + 6) Np) + 3 round256(4 T H) + round256(4 (T + 2) H) + round256(4 T ld) + 3 round256(4 T hop C) )
 * the transposed mel, the reflected noise, the predictor's three tensors and its zero-haloed output, ONE slot for a block's predicted
 * kernels (reused by every block), and x, its successor and y at the sample rate: 199,312 bytes per frame and row for c32 with 100
 * mels, of which 99,328 are the predicted kernels.  Any contents when the call starts, nothing is cleared; every launch writes all it
 * later reads.
 *
 * gvx_univnet_forward: mel fp32 [B][n_mels][T], noise fp32 [B][noise_dim][T] -> wav_out [B][T * hop].  stage_out, if not NULL:
 * n_blocks + 2 device tensors - x after conv_pre [B][T][C], after every block [B][T cum_i][C], and the output layer before its tanh
 * [B][T hop].  T < 4: GVX_ERR_INVALID_ARG; the workspace missing, misaligned or short: GVX_ERR_WORKSPACE.  gvx_univnet_stage_times_ms:
 * 2 n_blocks + 2 durations - conv_pre, per block its predictor and then its layers, conv_post.  Every dims field is checked: a bad one
 * gives blob_floats == 0 and create == GVX_ERR_INVALID_ARG.  There is no backward yet. */
enum { GVX_UNIVNET_MAX_BLOCKS = 4, GVX_UNIVNET_MAX_DILATIONS = 8, GVX_UNIVNET_MAX_FRAMES = 1 << 16, GVX_UNIVNET_MIN_FRAMES = 4,
       GVX_UNIVNET_MAX_DILATION = 36, GVX_UNIVNET_MAX_HIDDEN = 256 };
typedef struct gvx_univnet_dims {
    int32_t n_mels;                                  /* in [1, 4096] */
    int32_t noise_dim;                               /* in [1, 1024] */
    int32_t channel_size;                            /* a multiple of 4 in [4, 32]; 32 runs the LVC on the matrix pipe */
    int32_t n_dilations;                             /* in [1, GVX_UNIVNET_MAX_DILATIONS] */
    int32_t dilations[GVX_UNIVNET_MAX_DILATIONS];    /* each in [1, GVX_UNIVNET_MAX_DILATION]: HiFi-GAN's window cap of 72 */
    int32_t n_blocks;                                /* in [1, GVX_UNIVNET_MAX_BLOCKS] */
    int32_t strides[GVX_UNIVNET_MAX_BLOCKS];         /* each even and in [2, 64]; their product at most 4096 */
    int32_t kpnet_hidden_channels;                   /* a multiple of 32 in [32, GVX_UNIVNET_MAX_HIDDEN] */
    int32_t kpnet_conv_size;                         /* 3 */
    float slope;                                     /* in [0, 1] */
} gvx_univnet_dims;
typedef struct gvx_univnet gvx_univnet;
int gvx_lvc_gated(const float* x, const float* kern, int n_layers, int layer, const float* conv_w, const float* conv_b, int dilation,
                  const int32_t* lens, int B, int T, int cum, int C, float slope, float* scratch, float* out, void* stream);
size_t gvx_univnet_blob_floats(const gvx_univnet_dims* dims);
size_t gvx_univnet_workspace_bytes(const gvx_univnet_dims* dims, int B, int T);
int gvx_univnet_pack_weights_device(const gvx_univnet_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_univnet_create(const gvx_univnet_dims* dims, gvx_univnet** out);
void gvx_univnet_destroy(gvx_univnet* handle);
int gvx_univnet_bind(gvx_univnet* handle, const float* device_blob);
int gvx_univnet_forward(gvx_univnet* handle, const float* mel, const float* noise, const int32_t* frame_lengths, int B, int T,
                        float* wav_out, float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_univnet_timing_enable(gvx_univnet* handle, int enable);
int gvx_univnet_stage_times_ms(gvx_univnet* handle, float* ms_out, int* n_out);

/* ---- MelGAN discriminators: the multi-scale discriminator a MelGAN generator is trained against (Kumar et al. 2019), forward and
 * backward.  The reference ships the training fields of MelGANConfig and no model; this is a statement of the published architecture.
 * All arithmetic is fp32.  lrelu and "reflect" as for the generator above; s = downsampling_factor.
 *
 * One scale, on a row of n samples:
 *     layer 0:                Conv1d(1 -> c_0 = base_channels, k = 15)(reflect 7 (x)), lrelu                             length n
 *     layers i = 1..n_layers: c_i = min(c_{i-1} s, max_channels);
 *                             Conv1d(c_{i-1} -> c_i, k = 10 s + 1, stride s, zero padding 5 s, groups = c_{i-1} / 4), lrelu
 *                                                                                             length L_i = (L_{i-1} - 1) / s + 1
 *     layer n_layers + 1:     c' = min(2 c_last, max_channels);  Conv1d(c_last -> c', k = 5, zero padding 2), lrelu
 *     layer n_layers + 2:     the score, Conv1d(c' -> 1, k = 3, zero padding 1), no activation
 * and all n_layers + 3 maps are returned (post-activation; the last is the score).  Scale k + 1 sees the waveform of scale k through
 * AvgPool1d(4, stride 2, padding 1, count_include_pad = False): y[j] = the mean of x[2j-1 .. 2j+2] inside [0, n), j < n / 2.
 *
 * Ragged batches: sample_lengths is int32 [B] on the device, or NULL for all n_max.  Row b is computed as if alone at n_b =
 * min(sample_lengths[b], n_max): the reflection, the zero padding, every pooled length n_b >> k and every L_i are its own; nothing of wav
 * at or behind n_b is read; every map is exact zeros behind the row's own length; a ragged row has the bits of its one-row run.  A row
 * needs n_b >= 8 * 2^(n_scales - 1) (the last scale's reflection); the host cannot see device lengths, so the CALLER checks them - a
 * shorter row comes out as all-zero maps.
 *
 * Dims are refused (GVX_ERR_INVALID_ARG from create and pack, 0 from the size functions) unless: n_scales in [1, 4]; base_channels a
 * positive multiple of 4; n_layers in [1, 6]; downsampling_factor in [1, 8]; max_channels in [4, 65536]; slope in [0, 1]; and every
 * grouped layer's input channels are a multiple of 4 and its output channels divisible by its group count.
 *
 * Weights.  gvx_melgan_disc_pack_weights_device reads PyTorch-layout tensors from DEVICE pointers, by name:
 *     scales.<k>.layers.<i>.weight [c_out][c_in / groups][taps], scales.<k>.layers.<i>.bias [c_out],   i = 0 .. n_layers + 2
 * and writes the blob, which keeps those layouts, every tensor starting at a multiple of 64 floats (gvx_melgan_disc_blob_floats).  A
 * missing name is GVX_ERR_MISSING_WEIGHT, a wrong element count GVX_ERR_SHAPE, both before anything is launched.  The blob must be
 * 256-byte aligned; the handle keeps the pointer.
 *
 * Features buffer: the caller's, 256-byte aligned, gvx_melgan_disc_features_bytes long.  gvx_melgan_disc_layout (host arithmetic) lists,
 * scale by scale and layer by layer, (byte offset, channels, positions): map (k, i) is fp32 [B][channels][positions] with positions =
 * L_i of a row of n_max >> k samples, every map starting at a multiple of 256 bytes.  It returns the number of entries,
 * n_scales * (n_layers + 3), and fills at most max_entries of them (entries may be NULL); 0 for refused dims, B or n_max.
 *
 * Workspace: gvx_melgan_disc_workspace_bytes(dims, B, n_max, backward) is host arithmetic; any contents when a call starts, nothing is
 * cleared, 256-byte aligned.  The forward's (backward = 0) holds the pooled waveforms of the scales behind the first.  The backward's
 * holds those again (it recomputes them from wav), their gradients, two activation gradients of the largest map, and the partial
 * weight gradients of the layer that needs most.
 *
 * gvx_melgan_disc_forward: a chain of ordinary launches on `stream`, one per layer and one per pooling; a workgroup computes
 * GVX_MELGAN_DISC_TILE positions of one row.  Refused before anything is launched: a NULL handle, wav or features, B outside [1, 65535],
 * n_max below 8 * 2^(n_scales - 1) (GVX_ERR_INVALID_ARG); n_max above GVX_MELGAN_DISC_MAX_SAMPLES (GVX_ERR_UNSUPPORTED); no blob
 * bound (GVX_ERR_STATE); a misaligned or short features buffer, a NULL, misaligned or short workspace (GVX_ERR_WORKSPACE).
 *
 * gvx_melgan_disc_backward: features is what the forward wrote for the same wav, lengths and weights - it is the tape: a LeakyReLU
 * output is positive exactly where its pre-activation is, so the masks are read off the maps.  d_features has the layout of features
 * and holds the cotangent of EVERY map (a feature-matching loss feeds all of them); nothing of it is read behind a row's own
 * lengths.  grads is a HOST table of n_grads DEVICE destinations under the packer's names, each WRITTEN in PyTorch's layout; n_grads = 0
 * skips every parameter gradient (the generator's step).  d_wav is fp32 [B][n_max], the sum over the scales through the adjoint of the
 * pooling, exactly 0 at and behind n_b, or NULL to skip it (the discriminator's step).  What a call does compute has the bits the full
 * call gives it.  Refused as the forward refuses, and: a missing name (GVX_ERR_MISSING_WEIGHT), a wrong element count or NULL
 * destination (GVX_ERR_SHAPE), a NULL d_features, or neither gradient asked for (GVX_ERR_INVALID_ARG).  Weight gradients are summed
 * over rows and positions in pieces that are added in a fixed order; no float atomics: two calls give the same bits. */
enum { GVX_MELGAN_DISC_MAX_SCALES = 4, GVX_MELGAN_DISC_TILE = 64, GVX_MELGAN_DISC_MAX_SAMPLES = 1 << 24 };
typedef struct gvx_melgan_disc_dims {
    int32_t n_scales;
    int32_t base_channels;
    int32_t n_layers;
    int32_t downsampling_factor;
    int32_t max_channels;
    float slope;
} gvx_melgan_disc_dims;
typedef struct gvx_melgan_disc_entry {
    uint64_t byte_offset;
    int32_t channels;
    int32_t positions;
} gvx_melgan_disc_entry;
typedef struct gvx_melgan_disc gvx_melgan_disc;
size_t gvx_melgan_disc_blob_floats(const gvx_melgan_disc_dims* dims);
int gvx_melgan_disc_pack_weights_device(const gvx_melgan_disc_dims* dims, const gvx_weight_desc* table, int n, float* device_blob,
                                        void* stream);
int gvx_melgan_disc_create(const gvx_melgan_disc_dims* dims, gvx_melgan_disc** out);
void gvx_melgan_disc_destroy(gvx_melgan_disc* handle);
int gvx_melgan_disc_bind(gvx_melgan_disc* handle, const float* device_blob);
int gvx_melgan_disc_layout(const gvx_melgan_disc_dims* dims, int B, int n_max, gvx_melgan_disc_entry* entries, int max_entries);
size_t gvx_melgan_disc_features_bytes(const gvx_melgan_disc_dims* dims, int B, int n_max);
size_t gvx_melgan_disc_workspace_bytes(const gvx_melgan_disc_dims* dims, int B, int n_max, int backward);
int gvx_melgan_disc_forward(gvx_melgan_disc* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_melgan_disc_backward(gvx_melgan_disc* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max,
                             const void* features, const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- HiFi-GAN period discriminators (Kong et al. 2020, the published DiscriminatorP / MultiPeriodDiscriminator): forward, and the
 * backward that reads the forward's own maps as its tape.  The surface mirrors the MelGAN discriminators' above.
 *
 * The model.  For each period p = periods[j] and each row of n_b samples: the row is extended by reflection (sample n_b + i is sample
 * n_b - 2 - i) to H_0 p samples, H_0 = ceil(n_b / p), and read as a grid of H_0 heights and p columns, sample i at (i / p, i % p).
 * Layers i = 0 .. n_layers - 1 convolve along the height only: Conv2d(c_{i-1} -> channels[i], (kernel_size, 1), zero padding
 * (kernel_size / 2, 0), stride (stride, 1) for all but the last, (1, 1) for the last), each followed by LeakyReLU(slope); heights
 * H' = (H - 1) / stride + 1 for the strided layers.  The score is Conv2d(c_last -> 1, (3, 1), padding (1, 0)) without activation.  All
 * n_layers + 1 maps are returned (post-activation; the last is the score).  The p columns of a grid never mix.
 *
 * Ragged batches: sample_lengths is int32 [B] on the device, or NULL for all n_max.  Row b is computed as if alone at n_b =
 * min(sample_lengths[b], n_max): the reflection, the zero padding and every height are its own; nothing of wav at or behind n_b is
 * read; every map is exact zeros behind the row's own height; a ragged row has the bits of its one-row run.  A row needs n_b >= the
 * largest period (its reflection); the host cannot see device lengths, so the CALLER checks them - a shorter row comes out as all-zero
 * maps, never a bad address.
 *
 * Dims are refused (GVX_ERR_INVALID_ARG from create and pack, 0 from the size functions) unless: n_periods in [1, 8]; every period in
 * [1, 64]; n_layers in [2, 8]; every channel count in [1, 4096] and, above 64, a multiple of 32; kernel_size odd and in [1, 15];
 * stride in [1, 8]; slope in [0, 1].
 *
 * Weights.  gvx_hifigan_mpd_pack_weights_device reads PyTorch-layout tensors from DEVICE pointers, by name:
 *     discriminators.<j>.convs.<i>.weight [c_out][c_in][kernel_size] (Conv2d's trailing 1 dropped), .bias [c_out],
 *     discriminators.<j>.conv_post.weight [1][c_last][3], .bias [1]
 * and writes the blob (gvx_hifigan_mpd_blob_floats): every weight twice, as [c_out][tap][c_in] for the forward and as
 * [c_in][tap][c_out] for the data gradient, so that both products read their k index contiguously.  A missing name is
 * GVX_ERR_MISSING_WEIGHT, a wrong element count GVX_ERR_SHAPE, both before anything is launched.  The blob must be 256-byte aligned.
 *
 * Features buffer: the caller's, 256-byte aligned, gvx_hifigan_mpd_features_bytes long.  Maps are CHANNELS-LAST: map (j, i) is fp32
 * [B][height][period][channels], every map starting at a multiple of 256 bytes.  gvx_hifigan_mpd_layout (host arithmetic) lists, period
 * by period and map by map, the byte offset, channels, height (of a row of n_max samples), period, and the strides in floats of the
 * [B, C, H, p] view.  It returns the number of entries, n_periods * (n_layers + 1), and fills at most max_entries of them (entries
 * may be NULL); 0 for refused dims, B or n_max.
 *
 * Workspace: gvx_hifigan_mpd_workspace_bytes(dims, B, n_max, backward) is host arithmetic; any contents when a call starts, nothing is
 * cleared, 256-byte aligned.  The forward needs none beyond the minimum of 256 bytes; the backward's holds two activation gradients of
 * the largest map and the partial weight and bias gradients of the layer that needs most.
 *
 * Kernels.  A workgroup computes GVX_HIFIGAN_MPD_TILE positions (height, column) of one row, in every kernel family; a data gradient's
 * workgroup takes its positions from ONE stride phase (input heights h with the same h mod stride), so that only the taps
 * t = (h + pad) mod stride, + stride, ... are multiplied.  A layer whose two channel counts are multiples of GVX_HIFIGAN_MPD_MFMA_MULT
 * runs - forward, data gradient and weight gradient - as an implicit GEMM on v_mfma_f32_32x32x2_f32, GVX_HIFIGAN_MPD_TILE_N_WIDE
 * output channels per workgroup of the forward and the data gradient where that many are produced, GVX_HIFIGAN_MPD_TILE_N below; the others (the first layer, which absorbs the reflection and the reshape; the score, whose input channels
 * are dealt over the lanes of a wave and added by a fixed butterfly; narrow test layers) are fp32 VALU code.  LeakyReLU and its mask
 * are applied in the epilogues.  Nothing is computed for a tile that lies behind its row.
 *
 * gvx_hifigan_mpd_forward: refused before anything is launched: a NULL handle, wav or features, B outside [1, 65535], n_max below the
 * largest period (GVX_ERR_INVALID_ARG); n_max above GVX_HIFIGAN_MPD_MAX_SAMPLES (GVX_ERR_UNSUPPORTED); no blob bound (GVX_ERR_STATE);
 * a misaligned or short features buffer, a NULL, misaligned or short workspace (GVX_ERR_WORKSPACE).
 *
 * gvx_hifigan_mpd_backward: features is what the forward wrote for the same wav, lengths and weights - it is the tape: a LeakyReLU
 * output is positive exactly where its pre-activation is, so the masks are read off the maps.  d_features has the layout of features
 * and holds the cotangent of EVERY map; nothing of it is read behind a row's own heights.  grads is a HOST table of n_grads DEVICE
 * destinations under the packer's names, each WRITTEN in PyTorch's layout; n_grads = 0 skips every parameter gradient.  d_wav is fp32
 * [B][n_max], the sum over the periods in their order through the adjoint of the reshape and the reflection (a gather: a sample
 * collects its own cell and the reflected cell that copies it), exactly 0 at and behind n_b, or NULL to skip it.  What a call does
 * compute has the bits the full call gives it.  Refused as the forward refuses, and: a missing name (GVX_ERR_MISSING_WEIGHT), a wrong
 * element count or NULL destination (GVX_ERR_SHAPE), a NULL d_features, or neither gradient asked for (GVX_ERR_INVALID_ARG).  Weight
 * and bias gradients are summed over rows and positions in pieces that are added in a fixed order; no atomics: two calls give the
 * same bits. */
enum { GVX_HIFIGAN_MPD_MAX_PERIODS = 8, GVX_HIFIGAN_MPD_MAX_LAYERS = 8, GVX_HIFIGAN_MPD_MAX_PERIOD = 64, GVX_HIFIGAN_MPD_TILE = 64,
       GVX_HIFIGAN_MPD_TILE_N = 64, GVX_HIFIGAN_MPD_TILE_N_WIDE = 128, GVX_HIFIGAN_MPD_MFMA_MULT = 32, GVX_HIFIGAN_MPD_MAX_SAMPLES = 1 << 24 };
typedef struct gvx_hifigan_mpd_dims {
    int32_t n_periods;
    int32_t periods[8];
    int32_t n_layers;
    int32_t channels[8];
    int32_t kernel_size;
    int32_t stride;
    float slope;
} gvx_hifigan_mpd_dims;
typedef struct gvx_hifigan_mpd_entry {
    uint64_t byte_offset;
    int32_t channels;
    int32_t height;
    int32_t period;
    int32_t reserved;
    int64_t stride_b, stride_c, stride_h, stride_p;   /* floats, of the [B, C, H, p] view */
} gvx_hifigan_mpd_entry;
typedef struct gvx_hifigan_mpd gvx_hifigan_mpd;
size_t gvx_hifigan_mpd_blob_floats(const gvx_hifigan_mpd_dims* dims);
int gvx_hifigan_mpd_pack_weights_device(const gvx_hifigan_mpd_dims* dims, const gvx_weight_desc* table, int n, float* device_blob,
                                        void* stream);
int gvx_hifigan_mpd_create(const gvx_hifigan_mpd_dims* dims, gvx_hifigan_mpd** out);
void gvx_hifigan_mpd_destroy(gvx_hifigan_mpd* handle);
int gvx_hifigan_mpd_bind(gvx_hifigan_mpd* handle, const float* device_blob);
int gvx_hifigan_mpd_layout(const gvx_hifigan_mpd_dims* dims, int B, int n_max, gvx_hifigan_mpd_entry* entries, int max_entries);
size_t gvx_hifigan_mpd_features_bytes(const gvx_hifigan_mpd_dims* dims, int B, int n_max);
size_t gvx_hifigan_mpd_workspace_bytes(const gvx_hifigan_mpd_dims* dims, int B, int n_max, int backward);
int gvx_hifigan_mpd_forward(gvx_hifigan_mpd* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_hifigan_mpd_backward(gvx_hifigan_mpd* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max,
                             const void* features, const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Measurement only (tools/bench_extra.py hifigan_mpd): when enabled, the calls record events around every layer;
 * gvx_hifigan_mpd_layer_times_ms synchronises and returns, per layer (the score last; n_layers + 1 of them) and summed over the periods,
 * the time of the last forward and of the last backward (a layer's weight, bias and data gradient together; 0 for a call not made). */
int gvx_hifigan_mpd_timing_enable(gvx_hifigan_mpd* handle, int enable);
int gvx_hifigan_mpd_layer_times_ms(gvx_hifigan_mpd* handle, float* forward_ms, float* backward_ms, int* n_layers_out);

/* ---- Multi-resolution spectrogram discriminator (UnivNet's MRD, Jang et al. 2021; the published BigVGAN recipe trains with it):
 * forward, and the backward that reads the forward's own maps as its tape.  The surface, the contracts and the error codes are the
 * period discriminators' above.  All arithmetic fp32.
 *
 * The model.  One sub-discriminator per resolution (n_fft, hop, win).  A row of n samples is reflect-padded by p = (n_fft - hop) / 2
 * samples at both ends (padded sample -1 - i is sample 1 + i, padded sample n + i is sample n - 2 - i; needs n > p) and framed without
 * centring: frame w starts at padded position w * hop, W_0 = 1 + (n + 2p - n_fft) / hop frames (none if that is negative).  A frame
 * is multiplied by the window - rectangular or periodic Hann of `win` samples, zero-padded to n_fft with left offset (n_fft - win) / 2
 * - and transformed: F = n_fft / 2 + 1 bins, mag[w][f] = sqrt(re^2 + im^2), whose gradient is d_mag (re, im) / mag and exactly 0 where
 * mag == 0.  On the one-channel image mag, with the axes in Conv2d's order (frequency, time): Conv2d(1 -> C, (3, 9), padding (1, 4)),
 * three times Conv2d(C -> C, (3, 9), stride (1, 2), padding (1, 4)), Conv2d(C -> C, (3, 3), padding (1, 1)), each followed by
 * LeakyReLU(slope); the score is Conv2d(C -> 1, (3, 3), padding (1, 1)) without activation.  A strided layer takes W frames to
 * (W - 1) / 2 + 1; F never changes.  All six maps are returned (post-activation; the last is the score).
 *
 * Ragged batches: sample_lengths is int32 [B] on the device, or NULL for all n_max.  Row b is computed as if alone at n_b =
 * min(sample_lengths[b], n_max): the reflection, the frame count and the zero padding in time are its own; nothing of wav at or behind
 * n_b is read; every map is exact zeros behind the row's own frames; a ragged row has the bits of its one-row run.  A row needs
 * n_b >= min_samples = the largest p + 1; the host cannot see device lengths, so the CALLER checks them - a shorter row comes out as
 * all-zero maps, never a bad address.
 *
 * Dims are refused (GVX_ERR_INVALID_ARG from create and pack, 0 from the size functions) unless: n_resolutions in [1, 8]; every n_fft
 * one of 512, 1024, 2048; 1 <= hop <= win <= n_fft; channels a multiple of 32 in [32, 128]; window one of GVX_MRD_WINDOW_*; slope in
 * [0, 1].
 *
 * Weights.  gvx_mrd_pack_weights_device reads PyTorch-layout tensors from DEVICE pointers, by name:
 *     discriminators.<j>.convs.<i>.weight [c_out][c_in][3][9] (i = 4: [c_out][c_in][3][3]), .bias [c_out],
 *     discriminators.<j>.conv_post.weight [1][C][3][3], .bias [1]
 * and writes the blob (gvx_mrd_blob_floats): every weight twice, as [c_out][time tap][frequency tap][c_in] for the forward and as
 * [c_in][time tap][frequency tap, reversed][c_out] for the data gradient - in channels-last storage the three frequency taps of one
 * time tap are one contiguous run of 3 C floats of the operand, and both products read it against a contiguous run of weights - and,
 * behind the weights, every resolution's padded window and twiddle factors (computed in double on the device).  Errors as the period
 * discriminators'.
 *
 * Features buffer: the caller's, 256-byte aligned, gvx_mrd_features_bytes long.  Maps are CHANNELS-LAST: map (j, i) is fp32
 * [B][frames][bins][channels], every map starting at a multiple of 256 bytes, a row's valid part one contiguous run.  gvx_mrd_layout
 * (host arithmetic) lists, resolution by resolution and map by map, the byte offset, channels, frames (of a row of n_max samples),
 * bins, and the strides in floats of the [B, C, W, F] view - frames in front of bins: the transpose of the published [B, C, F, W].
 * It returns the number of entries, 6 n_resolutions, and fills at most max_entries of them; 0 for refused dims, B or n_max.
 *
 * Workspace: gvx_mrd_workspace_bytes(dims, B, n_max, backward) is host arithmetic; any contents when a call starts, nothing is
 * cleared, 256-byte aligned.  The forward's holds the spectrogram of one resolution; the backward's also that spectrogram's gradient,
 * the frame gradients [B][W_0][n_fft], two activation gradients of the largest map and the partial weight and bias gradients.
 *
 * Kernels.  The spectrogram is a wave per frame (GVX_MRD_FRAMES_PER_WORKGROUP frames per workgroup): gather through the reflection,
 * window, real transform in LDS (fft_lds.h), magnitude.  A position is a cell (frame, bin) of a map, numbered frame * F + bin.  The
 * first layer (K = 27) and the score (N = 1) are fp32 VALU code, GVX_MRD_TILE positions per workgroup.  The C -> C layers run -
 * forward, data gradient and weight gradient - as implicit GEMMs on v_mfma_f32_32x32x2_f32 with K = 3 C per time tap: GVX_MRD_TILE
 * positions x 64 channels per workgroup where c_out is a multiple of 64, GVX_MRD_TILE_NARROW positions x 32 channels otherwise;
 * LeakyReLU and its mask are applied in the epilogues, the zero padding is by index at both ends of both axes, and a tile that lies
 * behind its row computes nothing and writes zeros.  A data gradient's workgroup takes its positions from ONE stride phase in time.
 *
 * gvx_mrd_forward / gvx_mrd_backward: the arguments, the refusals before any launch and the results are those of
 * gvx_hifigan_mpd_forward / _backward, with min_samples for the largest period, GVX_MRD_MAX_SAMPLES for the limit of n_max, and
 * GVX_ERR_UNSUPPORTED as well where a map of n_max samples would have more than GVX_MRD_MAX_POSITIONS positions in a row.  The
 * backward recomputes the spectrogram from wav; d_mag goes through (re, im) / mag, the adjoint of the real transform and the window
 * to frame gradients, which are overlap-added as a gather: a sample collects its own padded cell and the reflected cells that copy
 * it, over the frames that cover each.  d_wav is the sum over the resolutions in their order, exactly 0 at and behind n_b.  A weight
 * gradient is summed in pieces of GVX_MRD_PIECE_FRAMES output frames of a row, added in a fixed order; bias gradients in float64
 * slices; no atomics: two calls give the same bits.  n_grads = 0 or d_wav = NULL skips that part; what is still computed keeps its
 * bits. */
enum { GVX_MRD_MAX_RESOLUTIONS = 8, GVX_MRD_MAPS = 6, GVX_MRD_TILE = 64, GVX_MRD_TILE_NARROW = 128, GVX_MRD_PIECE_FRAMES = 16,
       GVX_MRD_FRAMES_PER_WORKGROUP = 4, GVX_MRD_MAX_SAMPLES = 1 << 24, GVX_MRD_MAX_POSITIONS = 1 << 28 };
enum { GVX_MRD_WINDOW_RECTANGULAR = 0, GVX_MRD_WINDOW_HANN = 1 };
typedef struct gvx_mrd_dims {
    int32_t n_resolutions;
    int32_t n_fft[8];
    int32_t hop[8];
    int32_t win[8];
    int32_t channels;
    int32_t window;
    float slope;
} gvx_mrd_dims;
typedef struct gvx_mrd_entry {
    uint64_t byte_offset;
    int32_t channels;
    int32_t frames;
    int32_t bins;
    int32_t reserved;
    int64_t stride_b, stride_c, stride_w, stride_f;   /* floats, of the [B, C, W, F] view */
} gvx_mrd_entry;
typedef struct gvx_mrd gvx_mrd;
size_t gvx_mrd_blob_floats(const gvx_mrd_dims* dims);
int gvx_mrd_pack_weights_device(const gvx_mrd_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_mrd_create(const gvx_mrd_dims* dims, gvx_mrd** out);
void gvx_mrd_destroy(gvx_mrd* handle);
int gvx_mrd_bind(gvx_mrd* handle, const float* device_blob);
int gvx_mrd_layout(const gvx_mrd_dims* dims, int B, int n_max, gvx_mrd_entry* entries, int max_entries);
size_t gvx_mrd_features_bytes(const gvx_mrd_dims* dims, int B, int n_max);
size_t gvx_mrd_workspace_bytes(const gvx_mrd_dims* dims, int B, int n_max, int backward);
int gvx_mrd_forward(gvx_mrd* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                    size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_mrd_backward(gvx_mrd* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max, const void* features,
                     const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Measurement only (tools/bench_extra.py mrd): as gvx_hifigan_mpd_timing_enable / _layer_times_ms; six layers, the score last, summed
 * over the resolutions; the spectrogram and its adjoint count towards layer 0. */
int gvx_mrd_timing_enable(gvx_mrd* handle, int enable);
int gvx_mrd_layer_times_ms(gvx_mrd* handle, float* forward_ms, float* backward_ms, int* n_layers_out);

/* ---- HiFi-GAN scale discriminators (Kong et al. 2020, the published DiscriminatorS / MultiScaleDiscriminator): forward, and the
 * backward that reads the forward's own maps as its tape.  The surface mirrors the period discriminators' above.  All arithmetic fp32.
 *
 * The model.  Scale 0 sees the waveform; scale s + 1 sees the waveform of scale s through AvgPool1d(4, stride 2, padding 2) with
 * count_include_pad: y[j] = (the sum of x[2j - 2 .. 2j + 1] inside [0, n)) / 4 for j = 0 .. n / 2, so n' = n / 2 + 1.  On a row of n
 * samples of its scale, layers i = 0 .. n_layers - 1 are Conv1d(c_{i-1} -> channels[i], kernel_sizes[i], stride strides[i], zero
 * padding kernel_sizes[i] / 2, groups[i]) with c_{-1} = 1, each followed by LeakyReLU(slope); lengths L' = (L - 1) / stride + 1.  The
 * score is Conv1d(c_last -> 1, 3, padding 1) without activation.  All n_layers + 1 maps of a scale are returned (post-activation; the
 * last is the score).  The published shape is channels 128, 128, 256, 512, 1024, 1024, 1024; kernel sizes 15, 41, 41, 41, 41, 41, 5;
 * strides 1, 2, 2, 4, 4, 1, 1; groups 1, 4, 16, 16, 16, 16, 1; three scales; slope 0.1 - 9,870,209 parameters per scale.  Spectral and
 * weight norm are the caller's: the kernels see effective weights.
 *
 * Ragged batches: sample_lengths is int32 [B] on the device, or NULL for all n_max.  Row b is computed as if alone at n_b =
 * min(sample_lengths[b], n_max): the zero padding, every pooled length and every L_i are its own; nothing of wav at or behind n_b is
 * read; every map is exact zeros behind the row's own length; a ragged row has the bits of its one-row run.  There is no reflection:
 * the shortest legal row is 1 sample; a row of fewer comes out as all-zero maps, never a bad address.
 *
 * Dims are refused (GVX_ERR_INVALID_ARG from create and pack, 0 from the size functions) unless: n_scales in [1, 4]; n_layers in
 * [2, 8]; every channel count in [1, 4096]; every kernel size odd and in [1, 41]; every stride in [1, 8]; every group count at least 1
 * and a divisor of both channel counts of its layer; slope in [0, 1].
 *
 * Weights.  gvx_hifigan_msd_pack_weights_device reads PyTorch-layout tensors from DEVICE pointers, by name:
 *     discriminators.<s>.convs.<i>.weight [c_out][c_in / groups][k], .bias [c_out],
 *     discriminators.<s>.conv_post.weight [1][c_last][3], .bias [1]
 * and writes the blob (gvx_hifigan_msd_blob_floats): every weight twice, once for the forward and once for the data gradient, in the
 * order the layer's kernels read them.  A missing name is GVX_ERR_MISSING_WEIGHT, a wrong element count GVX_ERR_SHAPE, both before
 * anything is launched.  The blob must be 256-byte aligned.
 *
 * Features buffer: the caller's, 256-byte aligned, gvx_hifigan_msd_features_bytes long.  Maps are CHANNELS-LAST: map (s, i) is fp32
 * [B][length][channels], every map starting at a multiple of 256 bytes.  gvx_hifigan_msd_layout (host arithmetic) lists, scale by scale
 * and map by map, the byte offset, channels, length (of a row of n_max samples) and the strides in floats of the [B, C, L] view.  It
 * returns the number of entries, n_scales * (n_layers + 1), and fills at most max_entries of them (entries may be NULL); 0 for refused
 * dims, B or n_max.
 *
 * Workspace: gvx_hifigan_msd_workspace_bytes(dims, B, n_max, backward) is host arithmetic; any contents when a call starts, nothing is
 * cleared, 256-byte aligned.  The forward's holds the pooled waveforms; the backward's holds them again, the waveform gradient of every
 * pooled scale, two activation gradients of the largest map and the partial weight and bias gradients of the layer that needs most.
 *
 * Kernels.  A workgroup computes GVX_HIFIGAN_MSD_TILE positions of one row, in every convolution kernel; a data gradient's workgroup
 * takes its positions from ONE stride phase (input positions l with the same l mod stride), so that only the taps
 * t = (l + pad) mod stride, + stride, ... are multiplied.  A layer whose per-group input channels are a multiple of
 * GVX_HIFIGAN_MSD_MFMA_IN_MULT and whose per-group output channels are a multiple of GVX_HIFIGAN_MSD_MFMA_OUT_MULT runs - forward,
 * data gradient and weight gradient - as an implicit GEMM on the fp32 matrix instruction: positions on M, the group's output channels
 * on N, taps x group channels on K; v_mfma_f32_32x32x2_f32 where both per-group counts are multiples of 32, v_mfma_f32_16x16x4_f32
 * otherwise.  The forward and the data gradient stage a tile's input window - (GVX_HIFIGAN_MSD_TILE - 1) * stride + k positions of a
 * block of the group's channels, zeros outside the row - into LDS once and run every tap off row offsets in it.  The weight gradient
 * is a per-group GEMM with positions on K, one piece per row or per run of GVX_HIFIGAN_MSD_WG_RUN positions of a row.  The other
 * layers (the first, the score, narrow test layers), the pooling and its adjoint are fp32 VALU code.  LeakyReLU and its mask are
 * applied in the epilogues.  Every kernel is an ordinary launch.  Nothing is computed for a tile that lies behind its row.
 *
 * gvx_hifigan_msd_forward: refused before anything is launched: a NULL handle, wav or features, B outside [1, 65535], n_max below 1
 * (GVX_ERR_INVALID_ARG); n_max above GVX_HIFIGAN_MSD_MAX_SAMPLES (GVX_ERR_UNSUPPORTED); no blob bound (GVX_ERR_STATE); a misaligned
 * or short features buffer, a NULL, misaligned or short workspace (GVX_ERR_WORKSPACE).
 *
 * gvx_hifigan_msd_backward: features is what the forward wrote for the same wav, lengths and weights - it is the tape: a LeakyReLU
 * output is positive exactly where its pre-activation is, so the masks are read off the maps.  d_features has the layout of features
 * and holds the cotangent of EVERY map; nothing of it is read behind a row's own lengths.  grads is a HOST table of n_grads DEVICE
 * destinations under the packer's names, each WRITTEN in PyTorch's layout; n_grads = 0 skips every parameter gradient.  d_wav is fp32
 * [B][n_max], the sum over the scales through the adjoint of the pooling written as a gather (sample i collects pooled positions i / 2
 * and i / 2 + 1): the last scale's waveform gradient is pooled back into the one before it, and so on down to scale 0 - one fixed
 * order; exactly 0 at and behind n_b, or NULL to skip it.  What a call does compute has the bits the full call gives it.  Refused as
 * the forward refuses, and: a missing name (GVX_ERR_MISSING_WEIGHT), a wrong element count or NULL destination (GVX_ERR_SHAPE), a NULL
 * d_features, or neither gradient asked for (GVX_ERR_INVALID_ARG).  Weight and bias gradients are summed over rows and positions in
 * pieces that are added in a fixed order; no atomics: two calls give the same bits. */
enum { GVX_HIFIGAN_MSD_MAX_SCALES = 4, GVX_HIFIGAN_MSD_MAX_LAYERS = 8, GVX_HIFIGAN_MSD_MAX_KERNEL = 41, GVX_HIFIGAN_MSD_TILE = 64,
       GVX_HIFIGAN_MSD_MFMA_IN_MULT = 8, GVX_HIFIGAN_MSD_MFMA_OUT_MULT = 16, GVX_HIFIGAN_MSD_WG_RUN = 256,
       GVX_HIFIGAN_MSD_MAX_SAMPLES = 1 << 24 };
typedef struct gvx_hifigan_msd_dims {
    int32_t n_scales;
    int32_t n_layers;
    int32_t channels[8];
    int32_t kernel_sizes[8];
    int32_t strides[8];
    int32_t groups[8];
    float slope;
} gvx_hifigan_msd_dims;
typedef struct gvx_hifigan_msd_entry {
    uint64_t byte_offset;
    int32_t channels;
    int32_t length;
    int64_t stride_b, stride_c, stride_l;   /* floats, of the [B, C, L] view */
} gvx_hifigan_msd_entry;
typedef struct gvx_hifigan_msd gvx_hifigan_msd;
size_t gvx_hifigan_msd_blob_floats(const gvx_hifigan_msd_dims* dims);
int gvx_hifigan_msd_pack_weights_device(const gvx_hifigan_msd_dims* dims, const gvx_weight_desc* table, int n, float* device_blob,
                                        void* stream);
int gvx_hifigan_msd_create(const gvx_hifigan_msd_dims* dims, gvx_hifigan_msd** out);
void gvx_hifigan_msd_destroy(gvx_hifigan_msd* handle);
int gvx_hifigan_msd_bind(gvx_hifigan_msd* handle, const float* device_blob);
int gvx_hifigan_msd_layout(const gvx_hifigan_msd_dims* dims, int B, int n_max, gvx_hifigan_msd_entry* entries, int max_entries);
size_t gvx_hifigan_msd_features_bytes(const gvx_hifigan_msd_dims* dims, int B, int n_max);
size_t gvx_hifigan_msd_workspace_bytes(const gvx_hifigan_msd_dims* dims, int B, int n_max, int backward);
int gvx_hifigan_msd_forward(gvx_hifigan_msd* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream);
int gvx_hifigan_msd_backward(gvx_hifigan_msd* handle, const float* wav, const int32_t* sample_lengths, int B, int n_max,
                             const void* features, const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Measurement only (tools/bench_extra.py hifigan_msd): when enabled, the calls record events around every layer;
 * gvx_hifigan_msd_layer_times_ms synchronises and returns, per layer (the score last; n_layers + 1 of them) and summed over the scales,
 * the time of the last forward and of the last backward (a layer's weight, bias and data gradient together; 0 for a call not made). */
int gvx_hifigan_msd_timing_enable(gvx_hifigan_msd* handle, int enable);
int gvx_hifigan_msd_layer_times_ms(gvx_hifigan_msd* handle, float* forward_ms, float* backward_ms, int* n_layers_out);

/* ---- Multi-resolution STFT loss: the distance between a predicted waveform and its target that a vocoder is trained on (spectral
 * convergence plus log-magnitude L1 over several STFT resolutions; Yamamoto et al., Parallel WaveGAN), value and gradient in one call.
 * The reference ships no vocoder loss; this is the standard non-adversarial one, on the in-LDS transforms of the vocoder kernels.
 *
 * Inputs.  pred, target: fp32 [B][n_max].  sample_lengths: int32 [B] on the device or NULL; row b has n_b = sample_lengths[b] samples
 * (n_max without it).  Resolutions r = 0 .. R - 1, each (n_fft, hop, win_length) with 1 <= R <= 8, n_fft in {512, 1024, 2048},
 * 1 <= hop <= n_fft, 2 <= win_length <= n_fft.  Weights w_sc and w_mag, and eps (1e-7 where Parallel WaveGAN's numbers are wanted).
 *
 * Per row b and resolution r - torch.stft with center=True and pad_mode="reflect" of the row cut at its own length:
 *   - F = 1 + n_b / hop frames (integer division); frame t holds the padded samples p = t * hop + k, k in [0, n_fft);
 *   - the source index of p is i = p - n_fft / 2; for i < 0 it is -i, for i >= n_b it is 2 (n_b - 1) - i.  So a row needs
 *     n_b >= n_fft / 2 + 1 for the largest n_fft among the resolutions;
 *   - the window is the periodic Hann 0.5 - 0.5 cos(2 pi k / win_length), centred in the frame at offset (n_fft - win_length) / 2 and
 *     zero outside, computed in double on the host;
 *   - bins 0 .. n_fft / 2; magnitude M = sqrt(max(re^2 + im^2, eps));
 *   - sc[b][r] = ||M_t - M_p||_F / ||M_t||_F over the row's own F frames and all bins;
 *   - mag[b][r] = the mean of |log M_t - log M_p| over the same frames and bins;
 *   loss = (1 / (B R)) sum_b sum_r (w_sc sc[b][r] + w_mag mag[b][r]).
 * The norms and the means are PER ROW, not over the batch as Parallel WaveGAN takes them: a batch-wide norm would make a row's numbers
 * depend on its neighbours, and the ragged contract of this library is that a row's parts - and its gradient, up to the factor
 * 1 / (B R) that the loss itself carries - are the bits of that row run alone, whatever the other rows and n_max are.
 *
 * Gradient with respect to pred (target gets none): the derivative of the above for d loss = 1.  d sqrt(max(P, eps)) is 0 where P < eps;
 * d|u| at u == 0 is 0 (the sign is taken from M_t against M_p, the logarithm being monotone); the spectral-convergence term passes no
 * gradient where ||M_t - M_p||_F == 0 (torch's subgradient of a norm at 0).  d_pred is exact zeros at and behind n_b, and whatever lies
 * at and behind n_b in pred or target is never read.  So pred == target gives loss 0 and an all-zero gradient, and an all-zero pred a
 * finite loss and an all-zero gradient.
 *
 * gvx_stft_loss_create makes the window and twiddle tables in double on the host: an n_fft outside the three sizes is
 * GVX_ERR_UNSUPPORTED, any other value out of range GVX_ERR_INVALID_ARG.  gvx_stft_loss_workspace_bytes is host arithmetic (0 for a
 * NULL plan, B outside [1, GVX_STFT_LOSS_MAX_ROWS] or n_max outside [1, GVX_STFT_LOSS_MAX_SAMPLES]); the workspace follows the
 * conventions above: any contents, 256-byte aligned, nothing cleared.  It holds, per resolution, pred's spectrum, target's magnitudes,
 * the frame gradients and the partial sums - linear in B and in the frames of a row of n_max samples.
 *
 * The call: loss_out [1]; parts_out [B][R][2] = (sc, mag), may be NULL; d_pred [B][n_max], or NULL for the value alone (same loss
 * bits, no spectrum kept); dbg NULL, or for tests device pointers per resolution that receive M_p and M_t as
 * [B][1 + n_max / hop][n_fft / 2 + 1], NaN behind a row's frames (either pointer of a resolution may be NULL).  Refused before
 * anything is launched: NULL arguments and bad B or n_max (GVX_ERR_INVALID_ARG), n_max below n_fft_max / 2 + 1 (GVX_ERR_SHAPE), a
 * NULL, short or misaligned workspace (GVX_ERR_WORKSPACE).  With sample_lengths the rows' lengths are only known on the device: a row
 * with n_b outside [n_fft_max / 2 + 1, n_max] has no frames for the kernels - nothing of it is read, its parts and the loss are NaN -
 * and the call reads the lengths back behind its launches (so with sample_lengths it waits for the stream, once, while the kernels
 * run), zeroes all of d_pred and returns GVX_ERR_SHAPE naming the first such row.  Without sample_lengths the call enqueues and
 * returns.
 *
 * Kernels (all fp32 but the last sums): per resolution one launch transforms both signals, a frame per wave and
 * GVX_STFT_LOSS_FRAMES_PER_WORKGROUP frames per workgroup, as a complex transform of n_fft / 2 points in LDS plus the even/odd split,
 * with the samples gathered through the reflection (no padded copy of the batch exists), and leaves the three sums of its workgroup;
 * one small launch adds the partial sums of every (row, resolution) in a fixed order, in float64; per resolution one launch makes
 * dL/dX = (dL/dM_p) X / M_p from the kept spectrum and applies the adjoint of the real transform (not 1 / n times the inverse: the
 * interior bins count once) and the window; one launch gathers, a thread per sample and GVX_STFT_LOSS_GATHER_SAMPLES per workgroup,
 * the frames that cover the sample and its two reflected images, in ascending frame order, the resolutions in their order.  No
 * atomics: two calls give the same bits. */
enum { GVX_STFT_LOSS_MAX_RESOLUTIONS = 8, GVX_STFT_LOSS_FRAMES_PER_WORKGROUP = 4, GVX_STFT_LOSS_GATHER_SAMPLES = 256,
       GVX_STFT_LOSS_MAX_ROWS = 65535, GVX_STFT_LOSS_MAX_SAMPLES = 1 << 30 };
typedef struct gvx_stft_resolution {
    int32_t n_fft, hop, win_length;
} gvx_stft_resolution;
typedef struct gvx_stft_loss_debug {
    float* mag_pred[GVX_STFT_LOSS_MAX_RESOLUTIONS];
    float* mag_target[GVX_STFT_LOSS_MAX_RESOLUTIONS];
} gvx_stft_loss_debug;
typedef struct gvx_stft_loss_plan gvx_stft_loss_plan;   /* (the bare name is the call's) */
int gvx_stft_loss_create(const gvx_stft_resolution* res, int R, float w_sc, float w_mag, float eps, gvx_stft_loss_plan** out);
void gvx_stft_loss_destroy(gvx_stft_loss_plan* plan);
size_t gvx_stft_loss_workspace_bytes(const gvx_stft_loss_plan* plan, int B, long n_max);
int gvx_stft_loss(gvx_stft_loss_plan* plan, const float* pred, const float* target, const int32_t* sample_lengths, int B, long n_max,
                  float* loss_out, float* parts_out, float* d_pred, const gvx_stft_loss_debug* dbg, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---- Mel-spectrogram L1 loss: the spectral term of HiFi-GAN's generator objective (Kong et al. 2020) - the L1 distance between the
 * log-mel spectrograms of the generated waveform and of the recording, the published mel_spectrogram + F.l1_loss - made ragged the
 * way gvx_stft_loss is, value and gradient in one call.
 *
 * Inputs.  pred, target: fp32 [B][n_max].  sample_lengths: int32 [B] on the device or NULL; row b has n_b = sample_lengths[b] samples
 * (n_max without it).  Plan: n_fft in {512, 1024, 2048}; 1 <= hop <= n_fft with n_fft - hop even; 2 <= win_length <= n_fft;
 * 1 <= n_mels <= GVX_MEL_LOSS_MAX_MELS; mel_basis, a host float matrix [n_mels][n_fft / 2 + 1] - any finite matrix, zero rows and zero
 * columns included; clamp (1e-5 as published) and mag_eps (1e-9 as published), both finite and > 0.
 *
 * Per row b - torch.stft with center=False on the row cut at its own length and reflect-padded by pad = (n_fft - hop) / 2 on both sides:
 *   - F = n_b / hop frames (integer division); frame t holds the padded positions p = t * hop + k, k in [0, n_fft);
 *   - the source index of p is i = p - pad; for i < 0 it is -i, for i >= n_b it is 2 (n_b - 1) - i.  So a row needs
 *     n_b >= max(hop, pad + 1);
 *   - the window is the periodic Hann 0.5 - 0.5 cos(2 pi k / win_length), centred in the frame at offset (n_fft - win_length) / 2 and
 *     zero outside, computed in double on the host (the window of gvx_stft_loss);
 *   - bins k = 0 .. n_fft / 2; S_k = sqrt(re^2 + im^2 + mag_eps): an added epsilon, not a clamp;
 *   - m_j = sum_k mel_basis[j][k] S_k;  l_j = log(max(m_j, clamp)), the natural logarithm;
 *   - part[b] = the mean of |l_t - l_p| over the row's own F n_mels cells;
 *   loss = (1 / B) sum_b part[b].
 * The mean is PER ROW, not over the batch, for the reason given under gvx_stft_loss: a row's part is the bits of that row run alone,
 * and its gradient the bits of that row in any batch of the same B, whatever the other rows and n_max are.
 *
 * Gradient with respect to pred (target gets none), for d loss = 1.  d|u| at u == 0 is 0; the clamp passes gradient where
 * m >= clamp and none below it (torch.clamp); dS_k = sum_j mel_basis[j][k] dm_j; dX_k = dS_k X_k / S_k (S > 0 always); then the
 * adjoint of the real transform and the window.  d_pred is exact zeros at and behind n_b and on samples no frame reaches (with
 * hop > pad the tail behind F hop + pad is never read), and whatever lies at and behind n_b in pred or target is never read.  So
 * pred == target gives loss 0 and an all-zero gradient, and an all-zero pred - every mel of such a row lies under the clamp - a finite
 * loss and an all-zero gradient.
 *
 * gvx_mel_loss_create is host work alone (the first call of a plan moves its tables to the device; calls on one plan are not
 * concurrent): it makes the window and twiddle tables in double and derives the bands of the matrix: per mel the first
 * and last bin with a non-zero entry, per bin the first and last mel (a row with scattered non-zeros has the band min .. max; an
 * all-zero row or column has none).  The kernels run both products off the bands.  gvx_mel_loss_bands is that derivation by
 * itself, host arithmetic that needs no device: from a matrix [n_mels][bins] it fills mel_lo / mel_hi [n_mels] and bin_lo / bin_hi
 * [bins] on the host; hi is inclusive and an empty band has lo = 0, hi = -1.  An n_fft outside the three sizes is GVX_ERR_UNSUPPORTED, any other value out of range
 * GVX_ERR_INVALID_ARG.  gvx_mel_loss_workspace_bytes is host arithmetic (0 for a NULL plan, B outside [1, GVX_MEL_LOSS_MAX_ROWS] or
 * n_max outside [1, GVX_MEL_LOSS_MAX_SAMPLES]); the workspace follows the conventions above: any contents, 256-byte aligned, exactly
 * that size, nothing cleared.  It holds the frame gradients and the partial sums - linear in B and in the frames of a row of n_max.
 *
 * The call: loss_out [1]; parts_out [B], may be NULL; d_pred [B][n_max], or NULL for the value alone (same loss bits); dbg NULL, or
 * for tests two device pointers that receive l_p and l_t as [B][n_max / hop][n_mels], NaN behind a row's frames (either may be
 * NULL).  Refusals are those of gvx_stft_loss: NULL arguments and bad B or n_max (GVX_ERR_INVALID_ARG), n_max below
 * max(hop, pad + 1) (GVX_ERR_SHAPE), a NULL, short or misaligned workspace (GVX_ERR_WORKSPACE), all before anything is launched; with
 * sample_lengths a row with n_b outside [max(hop, pad + 1), n_max] has no frames for the kernels - its part and the loss are NaN - and
 * the call reads the lengths back behind its launches, zeroes all of d_pred and returns GVX_ERR_SHAPE naming the first such row.
 *
 * Kernels (fp32 but the last sums).  One launch does everything of a frame, a frame per wave and GVX_MEL_LOSS_FRAMES_PER_WORKGROUP
 * frames per workgroup: target's transform (samples gathered through the reflection, a complex transform of n_fft / 2 points in LDS,
 * the even/odd split), its magnitudes staged in LDS, the banded mel product and the logarithm; the same for pred with its spectrum
 * kept in registers; the cell's |l_t - l_p|; and, with d_pred, dm from the lengths alone (the coefficient 1 / (B F n_mels) needs no
 * batch sum), the banded transposed product, dX, the adjoint transform and the window - no spectrum goes through the workspace.
 * One launch gathers, a thread per sample and GVX_MEL_LOSS_GATHER_SAMPLES per workgroup, the frames that cover the sample and its
 * two reflected images (p = i + pad; pad - i for 1 <= i <= pad; 2 (n_b - 1) - i + pad for n_b - 1 - pad <= i <= n_b - 2) in
 * ascending frame order.  One small launch adds the workgroups' partial sums per row and the rows, in a fixed order in float64.
 * No atomics: two calls give the same bits. */
enum { GVX_MEL_LOSS_FRAMES_PER_WORKGROUP = 4, GVX_MEL_LOSS_GATHER_SAMPLES = 256, GVX_MEL_LOSS_MAX_MELS = 128,
       GVX_MEL_LOSS_MAX_ROWS = 65535, GVX_MEL_LOSS_MAX_SAMPLES = 1 << 30 };
typedef struct gvx_mel_loss_debug {
    float* log_mel_pred;
    float* log_mel_target;
} gvx_mel_loss_debug;
typedef struct gvx_mel_loss_plan gvx_mel_loss_plan;   /* (the bare name is the call's) */
int gvx_mel_loss_create(int n_fft, int hop, int win_length, int n_mels, const float* mel_basis, float clamp, float mag_eps,
                        gvx_mel_loss_plan** out);
void gvx_mel_loss_destroy(gvx_mel_loss_plan* plan);
int gvx_mel_loss_bands(const float* mel_basis, int n_mels, int bins, int32_t* mel_lo, int32_t* mel_hi, int32_t* bin_lo, int32_t* bin_hi);
size_t gvx_mel_loss_workspace_bytes(const gvx_mel_loss_plan* plan, int B, long n_max);
int gvx_mel_loss(gvx_mel_loss_plan* plan, const float* pred, const float* target, const int32_t* sample_lengths, int B, long n_max,
                 float* loss_out, float* parts_out, float* d_pred, const gvx_mel_loss_debug* dbg, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ---- Vocoder denoiser: the post-filter that the usual neural-vocoder inference scripts apply - take strength times the vocoder's bias
 * spectrum (the magnitudes of what it makes of a constant mel) off the STFT magnitudes of a vocoded waveform, clamp at 0, and transform
 * back with the phase kept.  The reference ships no vocoder and no such filter; the definition is this library's own, on the in-LDS
 * transforms of the two waveform losses.
 *
 * Inputs.  wav: fp32 [B][n_max].  sample_lengths: int32 [B] on the device or NULL; row b has n_b = sample_lengths[b] samples (n_max
 * without it).  Plan: n_fft in {512, 1024, 2048}, 1 <= hop <= n_fft / 2.  bias: fp32 [n_fft / 2 + 1] on the device, or NULL;
 * strength finite and >= 0, and a strength > 0 needs a bias.  With pad = n_fft / 2, per row b:
 *   - frames: F_b = 1 + n_b / hop (integer division); frame t holds the padded positions p = t * hop + j, j in [0, n_fft), through the
 *     single reflection of gvx_stft_loss: the source index of p is i = p - pad; for i < 0 it is -i, for i >= n_b it is 2 (n_b - 1) - i.
 *     So a row needs n_b >= pad + 1.  The window is the periodic Hann 0.5 - 0.5 cos(2 pi j / n_fft); it and the twiddles are made in
 *     double on the host.  This is torch.stft with center=True and pad_mode="reflect" on the row cut at its own length;
 *   - gain, per bin k = 0 .. n_fft / 2 of the frame's spectrum X: M = sqrt(re^2 + im^2) and a = strength * bias[k] (a = 0 without a
 *     bias).  Y = X max(0, M - a) / M where M > 0 and Y = 0 where M == 0; with a == 0, Y is X unchanged;
 *   - inverse: z_t = the inverse real transform of Y_t, the 1 / n_fft included, times the same window;
 *   - out[b][i] = (sum_t z_t[p - t hop]) / (sum_t w^2[p - t hop]) with p = i + pad, both sums in ascending order over the row's own
 *     frames t that cover p: torch.istft with center=True and length=n_b.  The denominator comes from the row's own frames, so the
 *     row's ends are right without a table per length, and it is positive at every sample of the row: the periodic Hann is zero only
 *     at index 0, and with hop <= n_fft / 2 every p in [pad, pad + n_b) lies in two consecutive frames of the row at least - where
 *     one of them has p at its index 0, the frame before it (there is one: p >= pad >= hop) has it at index hop, where w > 0;
 *   - out is exact zeros at and behind n_b; mag_out[b][t][k] = M, exact zeros behind the row's frames.
 * Whatever lies at and behind n_b in wav is never read.  out == wav (in place) is allowed: the first launch only reads wav and the
 * second only writes out.
 *
 * gvx_denoise_create is host work alone (the first call of a plan moves its tables to the device; calls on one plan are not
 * concurrent): an n_fft outside the three sizes is GVX_ERR_UNSUPPORTED, a hop outside [1, n_fft / 2] GVX_ERR_INVALID_ARG.
 * gvx_denoise_workspace_bytes is host arithmetic (0 for a NULL plan, B outside [1, GVX_DENOISE_MAX_ROWS] or n_max outside
 * [1, GVX_DENOISE_MAX_SAMPLES]); the workspace follows the conventions of gvx_mel_loss: any contents, 256-byte aligned, exactly that
 * size, nothing cleared.  It holds the windowed inverse frames [B][1 + n_max / hop][n_fft] - linear in B and in the frames of a row
 * of n_max samples - and is asked for whatever the outputs are.
 *
 * The call: out [B][n_max] or NULL, mag_out [B][1 + n_max / hop][n_fft / 2 + 1] or NULL, one of them at least; without out the
 * inverse half and the second launch are skipped, and either output has the same bits whether or not the other is asked for.  Refused
 * before anything is launched, as gvx_mel_loss has it: NULL arguments, bad B or n_max, a strength that is negative or not finite, a
 * strength > 0 without a bias (GVX_ERR_INVALID_ARG), n_max below pad + 1 (GVX_ERR_SHAPE), a NULL, short or misaligned workspace
 * (GVX_ERR_WORKSPACE).  With sample_lengths a row with n_b outside [pad + 1, n_max] has no frames for the kernels - nothing of it is
 * read, its row of out and its magnitudes are zeros - and the call reads the lengths back behind its launches (so with sample_lengths
 * it waits for the stream, once) and returns GVX_ERR_SHAPE naming the first such row; the other rows are what they are without it.
 *
 * Kernels (fp32).  One launch does everything of a frame, a frame per wave and GVX_DENOISE_FRAMES_PER_WORKGROUP frames per workgroup:
 * the samples gathered through the reflection and windowed, a complex transform of n_fft / 2 points in LDS and the even/odd split,
 * magnitude and gain in registers, the inverse side packed through the wave's LDS row, the inverse transform and the window; the frame
 * goes to the workspace, nothing of the spectrum does.  One launch gathers, a thread per sample and GVX_DENOISE_GATHER_SAMPLES per
 * workgroup, the at most ceil(n_fft / hop) frames that cover the sample, in ascending frame order for both sums, and writes the zeros
 * behind n_b.  No atomics: two calls give the same bits, and a ragged row is the bits of its own one-row run. */
enum { GVX_DENOISE_FRAMES_PER_WORKGROUP = 4, GVX_DENOISE_GATHER_SAMPLES = 256, GVX_DENOISE_MAX_ROWS = 65535, GVX_DENOISE_MAX_SAMPLES = 1 << 30 };
typedef struct gvx_denoise_plan gvx_denoise_plan;
int gvx_denoise_create(int n_fft, int hop, gvx_denoise_plan** out);
void gvx_denoise_destroy(gvx_denoise_plan* plan);
size_t gvx_denoise_workspace_bytes(const gvx_denoise_plan* plan, int B, long n_max);
int gvx_denoise(gvx_denoise_plan* plan, const float* wav, const int32_t* sample_lengths, int B, long n_max, const float* bias, float strength,
                float* out, float* mag_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- FastPitch acoustic model, tokens -> mel (Lancucki 2021; the published NVIDIA implementation, single speaker): inference.  The
 * reference ships no such model; the network below is a statement of the published implementation, under its state-dict names, and the
 * float64 restatement tests/fastpitch_ref64.py is the definition the device is held to.  Kernels: csrc/fastpitch.hip (self-attention,
 * residual + LayerNorm, embedding, the duration plan, the regulator, the C ABI) on the dense fp32 GEMM (csrc/gemm_f32.hip: every
 * product).  All arithmetic is fp32; every tensor is channels-last.  C = d_model, H = n_head, D = d_head, I = d_inner, k = kernel_size,
 * F = pred_filter, LN = LayerNorm over the channels of a position with eps 1e-5, pos[p] = cat(sin(p f), cos(p f)),
 * f_i = 10000^(-2 i / C), i < C / 2.
 *
 *     FFT stack (encoder, decoder), per layer:                                                         <stack>.layers.<i>
 *         qkv = Linear(C -> 3 H D)(x), columns [q | k | v], each [H][D]                                   .dec_attn.qkv_net
 *         a   = softmax(q k^T / sqrt(D)) v over the row's own keys, per head
 *         x   = LN(x + Linear(H D -> C, no bias)(a))                                                      .dec_attn.o_net, .dec_attn.layer_norm
 *         x   = LN(x + Conv1d(I -> C, k)(relu(Conv1d(C -> I, k, padding k / 2)(x))))                      .pos_ff.CoreNet.0, .2, .pos_ff.layer_norm
 *     x = word_emb[tokens] + pos;  x = encoder(x)                                                      encoder.word_emb
 *     predictor(x) = Linear(F -> 1)(n_layers of LN(relu(Conv1d(., F, 3, padding 1)(.))))               <p>.layers.<i>.conv, .norm, <p>.fc
 *     log_dur = duration_predictor(x);  dur = clamp(exp(log_dur) - 1, 0, max_duration)
 *     pitch = pitch_predictor(x);   x = x + Conv1d(1 -> C, 3, padding 1)(pitch)                         pitch_emb
 *     energy = energy_predictor(x); x = x + Conv1d(1 -> C, 3, padding 1)(energy)                        energy_emb   (energy_conditioning)
 *     reps_l = max(floor(dur_l / pace + 0.5), min_token_frames); start = exclusive scan; a row is cut at max_decoder_steps frames, and a
 *         row of 0 frames gets one frame of its last token
 *     y[t] = x[l] + pos[t] for start_l <= t < start_l + reps_l;  y = decoder(y);  mel = Linear(C -> n_mels)(y) as [B][n_mels][T]       proj
 * Every row is the row alone: every convolution sees zeros outside [0, T_b), keys at or behind T_b get weight exactly 0, every tensor is
 * zeros at and behind a row's length, and a row of a ragged batch has, bit for bit, the result of that row run alone.  This is the
 * published single-utterance inference, not its padded batch (which lets a padded row's last positions see non-zero values behind its end).
 *
 * gvx_self_attention is the attention on its own: qkv fp32 [B][T][3 H D] -> out fp32 [B][T][H D], lens int32 [B] on the device or NULL.
 * A workgroup of four waves owns GVX_ATTN_Q_TILE = 128 queries of one (row, head), a wave 32 of them; key / value tiles of
 * GVX_ATTN_K_TILE = 64 positions go through LDS (zeros at and behind T_b: qkv is never read there), the wave forms S^T = K Q^T and
 * O^T = V^T P^T on v_mfma_f32_32x32x2_f32 - so a query is a lane's column in both, and the running maximum, the running sum and the
 * rescale of the online softmax are the lane's own - and a tile wholly behind T_b is not visited.  Queries at or behind T_b are written
 * as zeros.  The order of the sum over keys is the tile walk's: the same row gives the same bits whatever B and T are.  No atomics.
 * D must be 32 or 64, H in [1, GVX_FASTPITCH_MAX_HEADS], B in [1, 65535], T in [1, GVX_FASTPITCH_MAX_POSITIONS]; qkv and out 16-byte aligned.
 *
 * gvx_add_layer_norm is the residual + LayerNorm on its own, the launch both LNs of a layer and every predictor layer are: x fp32
 * [B][N][C], y fp32 [B][N][C] or NULL, lens int32 [B] on the device or NULL, ln_w and ln_b fp32 [C] -> out_haloed fp32 [B][N + 2][C], position
 * t of a row at row t + 1 between two rows of exact zeros (the layout the k-tap products read), and out_plain fp32 [B][N][C] or NULL, the
 * same bits without the halo rows.  out[t] = LN(x[t] + y[t]) * ln_w + ln_b with eps 1e-5; a wave per position, lanes along the channels,
 * the mean, the mean of what is left and the squared deviations as butterflies, GVX_ADD_LN_POSITIONS = 16 positions per workgroup.
 * Positions at or behind N_b are written as zeros in both outputs, and x and y are never read there.  A position depends on nothing but
 * itself: the same row gives the same bits whatever B and N are.  Refused before any launch (GVX_ERR_INVALID_ARG, with the reason): a
 * NULL x, ln_w, ln_b or out_haloed; C that is not a multiple of 32 in [32, GVX_FASTPITCH_MAX_DIM]; B outside [1, 65535], N outside
 * [1, GVX_FASTPITCH_MAX_POSITIONS] or B N beyond 2^24; an output that overlaps x, y, ln_w, ln_b or the other output.
 *
 * Weights.  gvx_fastpitch_pack_weights_device copies DEVICE tensors by name into the blob, every tensor starting at a multiple of 64
 * floats: encoder.word_emb.weight [n_tokens][C]; per stack and layer dec_attn.qkv_net.weight [3 H D][C], .bias, dec_attn.o_net.weight
 * [C][H D], dec_attn.layer_norm.weight, .bias, pos_ff.CoreNet.0.weight [I][k][C] and pos_ff.CoreNet.2.weight [C][k][I] (TAP-major rows:
 * the caller permutes Conv1d's [out][in][k]), their biases, pos_ff.layer_norm.weight, .bias; per predictor and layer layers.<i>.conv.weight
 * [F][3][C_in], .bias, layers.<i>.norm.weight, .bias, then fc.weight [F], fc.bias [1]; pitch_emb.weight [C][3], .bias, energy_emb likewise
 * (energy = 1); proj.weight [n_mels][C], proj.bias.  The position table [max(max_tokens, max_decoder_steps)][C] follows; the call computes
 * it itself in float64.  A missing name: GVX_ERR_MISSING_WEIGHT; a wrong element count: GVX_ERR_SHAPE.
 *
 * A call runs in two phases, because the decoder's length is not known before the durations exist.  gvx_fastpitch_encode: tokens int32
 * [B][L] (a token outside [0, n_tokens) reads row 0), token_lengths int32 [B] or NULL, pace in [0.125, 8], durations_in int32 [B][L] or
 * NULL (used instead of the predicted ones), pitch_in fp32 [B][L] or NULL (used instead of the predicted pitch) -> enc_out fp32
 * [B][L + 2][C] (the conditioned encoder output between two zero halo rows), log_dur, pitch_pred, energy_pred fp32 [B][L], reps and starts
 * int32 [B][L], frame_counts int32 [B].  stage_out, if not NULL: enc_layers + 1 tensors [B][L][C], x after the embedding and after every
 * layer.  gvx_fastpitch_decode: what encode wrote and T >= every frame count -> mel fp32 [B][n_mels][T], gate fp32 [B][T] (-1e3 on a row's
 * frames but its last, +1e3 on the last and behind), alignments fp32 [B][T][L] (exact 0 / 1).  stage_out, if not NULL: dec_layers + 1
 * tensors [B][T][C], the regulated sequence and x after every layer.  The caller reads frame_counts between the two: the one
 * synchronisation of a call.  gvx_fastpitch_workspace_bytes(dims, B, N) is host arithmetic and serves either phase at N positions (L or
 * T); any contents when a call starts, nothing is cleared.  gvx_fastpitch_stage_times_ms: four durations - embedding + encoder,
 * predictors + plan + regulator, decoder, projection.  Every dims field is checked: a bad one gives blob_floats == 0 and
 * create == GVX_ERR_INVALID_ARG with the reason.  There is no backward. */
enum { GVX_ATTN_Q_TILE = 128, GVX_ATTN_K_TILE = 64, GVX_ADD_LN_POSITIONS = 16, GVX_FASTPITCH_MAX_DIM = 512, GVX_FASTPITCH_MAX_INNER = 8192, GVX_FASTPITCH_MAX_LAYERS = 32,
       GVX_FASTPITCH_MAX_HEADS = 16, GVX_FASTPITCH_MAX_TOKENS = 4096, GVX_FASTPITCH_MAX_POSITIONS = 1 << 16 };
typedef struct gvx_fft_stack_dims {
    int32_t n_layers;      /* in [1, GVX_FASTPITCH_MAX_LAYERS] */
    int32_t n_head;        /* in [1, GVX_FASTPITCH_MAX_HEADS] */
    int32_t d_head;        /* 32 or 64 */
    int32_t d_inner;       /* a multiple of 32 in [32, GVX_FASTPITCH_MAX_INNER] */
    int32_t kernel_size;   /* 1 or 3 */
} gvx_fft_stack_dims;
typedef struct gvx_fastpitch_dims {
    int32_t n_tokens;            /* rows of the embedding table, >= 1 */
    int32_t n_mels;              /* in [1, 4096] */
    int32_t d_model;             /* a multiple of 32 in [32, GVX_FASTPITCH_MAX_DIM]: the LayerNorm kernel's limit */
    gvx_fft_stack_dims enc, dec;
    int32_t pred_filter;         /* a multiple of 32 in [32, GVX_FASTPITCH_MAX_DIM] */
    int32_t pred_layers;         /* in [1, 8] */
    int32_t energy;              /* 1: energy_predictor and energy_emb exist */
    int32_t max_tokens;          /* in [1, GVX_FASTPITCH_MAX_TOKENS] */
    int32_t max_decoder_steps;   /* in [1, GVX_FASTPITCH_MAX_POSITIONS] */
    int32_t max_duration;        /* >= 1 */
    int32_t min_token_frames;    /* >= 0 */
} gvx_fastpitch_dims;
typedef struct gvx_fastpitch gvx_fastpitch;
int gvx_self_attention(const float* qkv, const int32_t* lens, int B, int T, int n_head, int d_head, float* out, void* stream);
int gvx_add_layer_norm(const float* x, const float* y, const int32_t* lens, int B, int N, int C, const float* ln_w, const float* ln_b,
                       float* out_haloed, float* out_plain, void* stream);
size_t gvx_fastpitch_blob_floats(const gvx_fastpitch_dims* dims);
size_t gvx_fastpitch_workspace_bytes(const gvx_fastpitch_dims* dims, int B, int N);
int gvx_fastpitch_pack_weights_device(const gvx_fastpitch_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream);
int gvx_fastpitch_create(const gvx_fastpitch_dims* dims, gvx_fastpitch** out);
void gvx_fastpitch_destroy(gvx_fastpitch* handle);
int gvx_fastpitch_bind(gvx_fastpitch* handle, const float* device_blob);
int gvx_fastpitch_encode(gvx_fastpitch* handle, const int32_t* tokens, const int32_t* token_lengths, int B, int L, float pace,
                         const int32_t* durations_in, const float* pitch_in, float* enc_out, float* log_dur, float* pitch_pred,
                         float* energy_pred, int32_t* reps, int32_t* starts, int32_t* frame_counts, float* const* stage_out, void* workspace,
                         size_t workspace_bytes, void* stream);
int gvx_fastpitch_decode(gvx_fastpitch* handle, const float* enc_out, const int32_t* reps, const int32_t* starts, const int32_t* frame_counts,
                         const int32_t* token_lengths, int B, int L, int T, float* mel_out, float* gate_out, float* align_out,
                         float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream);
int gvx_fastpitch_timing_enable(gvx_fastpitch* handle, int enable);
int gvx_fastpitch_stage_times_ms(gvx_fastpitch* handle, float* ms_out, int* n_out);

/* ---- Per-kernel timing of the decoder step (measurement only): when enabled, a teacher-forced call replays the
 * mid-sequence LSTM-step launch and the attention launches 64 times each, back to back, between HIP events on
 * `stream` (after its loop; the call's outputs are not valid afterwards); gvx_kernel_times_ms synchronises and
 * returns the average duration of each (ms) and the number of replays. */
int gvx_kernel_timing_enable(gvx_model* model, int enable);
int gvx_kernel_times_ms(gvx_model* model, float* lstm_avg_ms_out, float* attn_avg_ms_out, int* n_steps_out);

#ifdef __cplusplus
}
#endif
#endif /* GENVOX_AMD_H */
