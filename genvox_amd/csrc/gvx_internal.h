// Internal to the C-ABI layer (gvx_api.hip, gvx_pack.hip, gvx_decoder.hip); not installed.  The model handle with its knobs,
// the layouts of the weight blob and the workspace, the plans of the two decoder loops, error reporting.
#pragma once
#include "../../include/genvox_amd.h"
#include "gvx_kernels.h"
#include "winograd_f45.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace gvx {

int fail(int code, const char* fmt, ...);   // sets gvx_last_error() of this thread, returns `code`

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(GVX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

constexpr int MAX_CONV = 8;
constexpr double BN_EPS = 1e-5;

struct Blob {  // offsets in floats into the packed weight blob
    size_t emb;
    size_t enc_w[MAX_CONV], enc_b[MAX_CONV];
    size_t enc_wih, enc_bih, enc_whh_frag[2];
    size_t pre_w0, pre_w1, pre_w0_t, pre_w1_t;
    size_t att_frag, att_bias, att_wpre, wq_t, wmem, v, loc_conv, loc_dense;
    size_t dec_frag, dec_bias;
    size_t proj_w, proj_b, proj_frag, proj_hd_t, proj_ctx_frag, proj_ctx_t;   // last three: autoregressive split of the projection (see gvx_decoder_autoregressive)
    size_t post_w[MAX_CONV], post_b[MAX_CONV];
    size_t post_u[MAX_CONV];   // Winograd transform U[8][Cout][Cin] = G w of the layers winograd_shape_ok admits (others: unused)
    size_t enc_u[MAX_CONV];    // the same of the encoder's layers (encoder_layer_winograd_shape)
    size_t total;
};
// A convolution layer whose SHAPE admits the Winograd F(4,5) form (winograd_conv.hip): these have U in the blob.
inline bool winograd_shape_ok(int cin, int cout, int k) { return k == WINO_TAPS && cin == cout && cin % 32 == 0; }
// Postnet layer i is such a layer (the first and the last one, n_mels wide on one side, never are)
inline bool postnet_layer_winograd_shape(const gvx_dims& d, int i) {
    return i > 0 && i < d.postnet_n_conv - 1 && winograd_shape_ok(d.postnet_dim, d.postnet_dim, d.postnet_kernel);
}
// Encoder layer i is such a layer (every one of them is embed_dim -> embed_dim: all or none)
inline bool encoder_layer_winograd_shape(const gvx_dims& d, int i) {
    return i >= 0 && i < d.enc_n_conv && winograd_shape_ok(d.embed_dim, d.embed_dim, d.enc_kernel);
}
Blob make_blob_layout(const gvx_dims& d);   // gvx_pack.hip

inline size_t frag_floats(int N, int K) { return (size_t)((N + 31) / 32) * (K / 8) * 64 * 4; }

struct WsPlan {  // byte offsets into the caller's workspace
    size_t xa, xb, xg, enc_h, enc_c, flags, sync, memory;
    size_t pm, frames, pre1, prenet, h_a, c_a, c_d, hc, w_cum, q_slab, proj, energies, align_tm, len_copy, loc, ar_masks, p_slab, p_ctx;
    size_t att_part, dec_part, pre_gate, xchg;
    size_t ya, yb;
    size_t total;
};

}  // namespace gvx

struct gvx_model {
    gvx_dims d;
    gvx::Blob blob;
    const float* dev_blob = nullptr;
    // ---- knobs: every GVX_* variable the C-ABI layer honours, read once per handle by read_knobs (gvx_api.hip) when
    // gvx_model_create runs; gvx_model_set_persistent_attention / gvx_model_set_resident_kernels change some of them later
    bool use_graph = true;        // GVX_NO_GRAPH=1: every launch eagerly, no hipGraph replay of the step loops
    bool capture_first = false;   // GVX_GRAPH_FIRST=1: capture at the first sighting (tests of the replay path)
    bool attn_one_launch = true;  // GVX_ATTN_SPLIT=1: energy + context as two launches (the round-1 step, kept for A/B runs)
    // teacher-forced loop: attention as one kernel that lives beside the LSTM launches (attn_persist.hip) when the shape
    // allows it; GVX_ATTN_PERSISTENT=0 keeps the launch per step
    bool attn_persistent = true;
    // GVX_AR_RESIDENT=1: the autoregressive loop runs beside the resident attention kernel too.  Off by default: measured
    // (round 3, 200-step decodes) 49 vs 47 us per step at batch 1 and no gain at 2 x 32 rows - launch C then has 256 equal
    // tiles for 256 - B free CUs, so one CU streams two of them
    bool ar_resident = false;
    bool enc_persistent = true;   // encoder BiLSTM recurrence as one resident launch (B <= 32, H = 256); GVX_ENC_PERSISTENT=0: launch per position
    bool ar_split_h = true;       // autoregressive step: the h_a(t) columns of both cells as partial sums beside the attention step
                                  // (GVX_AR_SPLIT_H=0: the round-2 schedule, attention as a launch of its own)
    // GVX_TF_ROWS64=1: batches of 33 .. 64 rows run as ONE call beside a 64-CU resident kernel (layout 3).  Off by default:
    // with two batch tiles per workgroup the fp32 matrix pipe sets the launch length (37 us per 64-row step, MFMA pipe 54 %
    // busy on the 192 CUs, round 3) and two 32-row lanes on two streams are faster (40.1 vs 44.4 us per 64-row step)
    bool tf_rows64 = false;
    // teacher-forced loop as ONE resident weight-streaming kernel beside the resident attention kernel (dec_resident.hip):
    // B <= 32, L <= 128, inference mode; GVX_TF_RESIDENT=0 keeps the launch per step
    bool tf_resident = true;
    bool ar_resident_loop = true;   // autoregressive decode as two resident kernels (GVX_AR_RESIDENT_LOOP=0: launches per step)
    bool tf_long_rows_224 = true;   // teacher-forced rows of 129-256 tokens, <= 16 rows: the 224-workgroup deal (GVX_TF_LONG_224=0: 192)
    // the training forward takes the loop beside the resident attention kernel since round 3: the tape - dropped hidden states,
    // cell states, gate pre-activations - is written by the cell epilogues of both launch layouts; GVX_TRAIN_RESIDENT=0 keeps
    // the launch per attention step
    bool train_resident = true;
    bool train_resident_loop = true;   // GVX_TRAIN_RESIDENT_LOOP=0: the training forward's decoder loop as a launch per step
    // launch-per-step loop: the attention launch has the chip to itself: block i pulls the first k-groups of tile i of the NEXT
    // launch into its XCD's L2 (both grids are dealt round-robin over the XCDs) - loop 20.27 -> 20.06 ms at 32 x 800
    // (GVX_ATTN_PREFETCH=0: off); the rotated K walk (GVX_SK_ROT, an A/B knob) is not followed
    bool attn_prefetch = true;
    // Postnet and encoder convolutions with cin = cout, k = 5 as Winograd F(4,5): 0 never, 1 by the layer's shape (the shapes where it was
    // measured faster: at least WINOGRAD_MIN_CHANNELS channels), 2 every shape winograd_shape_ok admits (tests at small sizes).
    // GVX_CONV_WINOGRAD=<mode>, gvx_model_set_winograd.  The choice never looks at B, T or the lengths: a row's bits must not
    // depend on the batch it runs in.
    int winograd = 1;
    int wino_group = 0;                // debug (gvx_debug_set_winograd_group): tiles per Winograd group at most, 0 = as the scratch allows
    int enc_fork_after = 2;            // GVX_ENC_FORK_AFTER=<n>: the caller's Prenet products start behind n encoder convolutions
    int pa_depth = 4;                  // GVX_PA_DEPTH=6: prefetch depth of the launch beside the resident kernel (tests, A/B runs)
    unsigned side_pool = 1;            // GVX_SIDE_POOL=2: this handle's resident kernels are dealt two side streams round-robin (ensure_side_stream)
    unsigned spin_limit = 0;           // GVX_HANDOFF_SPIN_LIMIT: polls before an in-launch wait gives up (0 = the built-in limit)
    int rs_debug = 0;                  // GVX_RS_DEBUG=<bits>: timing experiments of the resident kernels (sleeps between polls)
    bool debug_skip_resident = false;  // GVX_DEBUG_SKIP_RESIDENT=1: never launch the resident attention kernel, so that every
                                       // wait of the loop runs into its limit (test of the time-out reporting only)
    int debug_enc_skip_block = -1;     // GVX_DEBUG_ENC_SKIP_BLOCK=<i>: workgroup i of the resident encoder recurrence leaves at once (tests: forced time-out)
    bool debug_plan = false;           // GVX_DEBUG_PLAN set: print the workspace's byte offsets once (tools/ar_ws_diff.py)
    // ---- state
    bool timing = false;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    int last_decoder_launches = 0;
    // hipGraph caches of the step loops.  A key holds every pointer / size the captured launches bake in - including the
    // weight blob: re-binding weights (load_state_dict -> new blob) must never replay launches that read the old one.
    struct LoopKey {
        const void* ws; const void* memory; const void* blob; int B, L, T; bool has_len;
        float threshold = 0.f;   // autoregressive graphs only
        int variant = 0;         // teacher-forced loop: 1 = with the persistent attention kernel
        // autoregressive graphs of a windowed decode: the caller's centre buffer (the steps' state, baked into the launches) and the window
        const void* centres = nullptr; int win_back = 0, win_ahead = 0;
        bool operator==(const LoopKey& o) const {
            return ws == o.ws && memory == o.memory && blob == o.blob && B == o.B && L == o.L && T == o.T &&
                   has_len == o.has_len && threshold == o.threshold && variant == o.variant && centres == o.centres &&
                   win_back == o.win_back && win_ahead == o.win_ahead;
        }
    };
    // One entry per key: the graphs of its chunks (one for the encoder / teacher-forced loop, one per 16-step chunk of the
    // autoregressive loop).  Policy: the first call with a key launches eagerly and only remembers the key; capture starts at
    // the second sighting (a serving process sees a new (B, L) per request - instantiating ~60 graphs of ~100 nodes for a
    // shape that never comes back costs more than the launches it saves); at most GRAPH_SETS keys per cache, LRU eviction.
    struct GraphSet {
        LoopKey key;
        int sightings = 0;
        uint64_t last_use = 0;
        std::vector<hipGraphExec_t> execs;
    };
    static constexpr size_t GRAPH_SETS = 4;
    std::vector<GraphSet> ar_graphs, loop_graphs, enc_graphs;
    uint64_t use_clock = 0;
    uint64_t graph_replays = 0;   // hipGraphLaunch calls of run_chunk on this handle (gvx_debug_graph_replays: the tests of the replay path)
    hipStream_t pa_stream = nullptr;
    hipEvent_t pa_fork = nullptr, pa_join = nullptr, enc_mid = nullptr;
    // autoregressive loop: the all-rows-finished counter of chunk k is read (pinned slot k & 1, event k & 1) while chunk k + 1 runs
    int32_t* ar_done_host = nullptr;
    hipEvent_t ar_ev[2] = {nullptr, nullptr};
    // device-side re-packing (gvx_model_pack_weights_device): where every float of the blob comes from, built once per
    // state_dict layout by running the HOST packer over index-coded stand-ins of the tensors
    std::vector<std::string> gather_names;
    std::vector<int64_t> gather_numel;
    int32_t* gather_off = nullptr;     // [blob.total] offset inside the source tensor (device)
    uint8_t* gather_tid = nullptr;     // [blob.total] source tensor + 1, 0 = constant zero (device)
    void drop_graphs() {
        for (auto* c : {&ar_graphs, &loop_graphs, &enc_graphs}) {
            for (auto& gs : *c)
                for (auto e : gs.execs)
                    if (e) (void)hipGraphExecDestroy(e);
            c->clear();
        }
    }
    hipStream_t cap_stream = nullptr;  // private stream used only to record captures (the caller's may be the null stream)
    // per-launch timing of the decoder step kernels (measurement only)
    bool ktiming = false;
    std::vector<hipEvent_t> kev;
    int n_lstm_ev = 0, n_attn_ev = 0;
    int reserve_events(size_t n) {
        while (kev.size() < n) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return GVX_ERR_HIP;
            kev.push_back(e);
        }
        return GVX_OK;
    }
    // derived
    int H() const { return d.embed_dim / 2; }
    int PS() const { return (d.n_mels + 1 + 3) & ~3; }  // padded row stride of the mel+gate projection (row-major)
    int PSB() const { return (d.n_mels + 1 + 7) & ~7; } // floats per row of the blocked per-step projection vector
};

namespace gvx {

// ---- how a shape runs.  plan_teacher_forced / plan_autoregressive (gvx_decoder.hip) are the only places where a handle's knobs,
// the layer sizes and (B, L) are combined into a path; the loops, the workspace layout, the fused forward and the query exports
// of the C ABI all read the plan.
enum TfMode : int { TF_INFERENCE = 0, TF_TRAIN_WHOLE_TAPE = 1, TF_TRAIN_PARTIAL_TAPE = 2 };   // (whole: the caller asks for every tape buffer)
struct TfLoopPlan {
    int kind;            // 0: launches per step, attention among them; 1: LSTM launches beside the resident attention kernel
                         // (attn_persist.hip); 2: one resident kernel pair for all steps (+ dec_resident.hip)
    int pa_layout;       // attention_persistent_layout(B, L): 1: L <= 128 (32 CUs, 224 workgroups); 2: L <= 256 (64 CUs, 192
                         // workgroups); 3: 33 .. 64 rows (64 CUs, 384 workgroups, two per CU)
    int tile_layout;     // deal of the resident tile kernel (kind 2), otherwise pa_layout
    bool rows64;         // kind 1 on layout 3: one launch of three jobs per step (launch_skinny_pa64)
    bool pre_gate;       // the shape can run beside the resident attention kernel in SOME mode: the pre_gate buffer exists and its GEMM runs
    bool timeout_check;  // ... and the call ends with the launch that turns a timed-out hand-off into NaN outputs + the sticky status word
    bool side_stream;    // kind != 0: the loop needs the side stream and a turn on the device
    bool graph;          // the step launches may be replayed from a hipGraph
};
struct ArLoopPlan {
    int kind;       // 0: launches per step; 1: step launches beside the resident attention kernel (GVX_AR_RESIDENT=1); 2: two resident kernels
    bool split_h;   // kind 0: the h_a(t) columns of both cells as partial sums beside the attention step
    bool fold;      // the projection's context columns ride on the decoder-LSTM tiles' projection slabs (launch C is exactly 256 tiles)
    bool graph;     // the 16-step chunks may be replayed from hipGraphs
};
TfLoopPlan plan_teacher_forced(const gvx_model* m, int B, int L, TfMode mode);
// windowed: the call carries a monotonic attention window (gvx_decoder_autoregressive_windowed).  The resident pair serves it with one
// attention workgroup per row (L <= 128); every other shape takes the launches per step (kind 0), whose attention step applies it
ArLoopPlan plan_autoregressive(const gvx_model* m, int B, int L, bool windowed = false);

enum WsMode : int { WS_TEACHER_FORCED = 0, WS_AUTOREGRESSIVE = 1 };

// ---- Winograd path of the Postnet and the encoder (gvx_api.hip)
constexpr int WINOGRAD_MIN_CHANNELS = 256;
constexpr size_t WINOGRAD_GROUP_BYTES = (size_t)128 << 20;   // V + M of one group of tiles: half the 256 MiB Infinity Cache
bool conv_uses_winograd(const gvx_model* m, int cin, int cout, int k);
long winograd_group_tiles(long total, long fit, int C);   // tiles per group: where a layer of `total` tiles is cut when `fit` fit the scratch
size_t winograd_scratch_floats(const gvx_model* m, int B, int T); // V + M of one group of tiles; 0: no layer of the model has the shape

// status words at the front of every workspace (int32 indices into `flags`)
constexpr int FLAG_TOKEN = 0;      // sticky: a token id was outside the embedding table
constexpr int FLAG_AR_DONE = 1;    // autoregressive loop: rows finished
constexpr int FLAG_TIMEOUT = 2;    // sticky: a teacher-forced call ended with its hand-off time-out word set
constexpr int FLAG_AR_FRAMES = 64; // autoregressive loop: frame counts [B <= 64]

WsPlan make_ws_plan(const gvx_model* m, int B, int L, int T, int mode = WS_TEACHER_FORCED);
int check_common(const gvx_model* m, int B, int L, int T, void* ws, size_t ws_bytes, int mode = WS_TEACHER_FORCED);

template <typename T>
T* ws_ptr(void* ws, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

inline hipError_t zero_async(void* p, size_t bytes, hipStream_t s) { return hipMemsetAsync(p, 0, bytes, s); }

// Find (or create, evicting the least recently used) the graph set of `key` and count the sighting.
gvx_model::GraphSet* touch_graph_set(gvx_model* m, std::vector<gvx_model::GraphSet>& cache, const gvx_model::LoopKey& key);
std::mutex& capture_mutex();

// Run the launches `enqueue(stream)` issues as chunk `chunk` of graph set `gs`: eagerly at the key's first sighting,
// afterwards from a hipGraph (captured on the model's private stream: the caller's may be the null stream, which
// cannot be captured).
template <class F>
int run_chunk(gvx_model* m, gvx_model::GraphSet* gs, size_t chunk, hipStream_t s, F&& enqueue) {
    if (!m->use_graph || !gs || (gs->sightings < 2 && !m->capture_first)) return enqueue(s);
    if (gs->execs.size() <= chunk) gs->execs.resize(chunk + 1, nullptr);
    hipGraphExec_t exec = gs->execs[chunk];
    if (!exec) {
        // Captures are serialised across handles: the host mirror drives two handles from two threads (chunk lanes), and
        // although each records on its own stream in thread-local mode, concurrent capture / instantiate is not something
        // to lean on in the runtime.  A one-time cost per graph; launches of existing graphs are not serialised.
        std::lock_guard<std::mutex> lock(capture_mutex());
        hipGraph_t graph = nullptr;
        if (!m->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue(m->cap_stream);
        const hipError_t ce = hipStreamEndCapture(m->cap_stream, &graph);
        if (rc != GVX_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        HIP_TRY(ce);
        HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        HIP_TRY(hipGraphDestroy(graph));
        gs->execs[chunk] = exec;
    }
    HIP_TRY(hipGraphLaunch(exec, s));
    ++m->graph_replays;
    return GVX_OK;
}

// ---- the decoder's side of the C-ABI layer (gvx_decoder.hip)
struct DecoderBuffers {
    float *pm, *frames, *pre1, *prenet, *h_a, *c_a, *c_d, *hc, *w_cum, *q_slab, *proj, *energies, *align_tm, *loc, *p_slab, *p_ctx;
    float *att_part, *dec_part, *pre_gate;
    int32_t* len_copy;
};
DecoderBuffers decoder_buffers(void* ws, const WsPlan& wp);

// Training mode (models/tts/tacotron2.py:341, :358): the outputs of both LSTM cells go through dropout before anything uses
// them (next step's recurrence, the attention query, the other cell, the projection).  Explicit keep masks, as for the Prenet.
struct LstmDropout {
    const uint8_t* att_keep; const uint8_t* dec_keep; float att_scale, dec_scale;   // [T][B][A], [T][B][D]
    // tape for back-propagation through time (all may be nullptr): the attention LSTM's (dropped) hidden state of every step as
    // blocked vectors [T+1][A/8][B][8] (slot t + 1 = after step t, slot 0 = zeros) and both cells' states [T+1][B][H] row-major
    float* h_a_all; float* c_a_all; float* c_d_all;
    float* pre_a_all; float* pre_d_all;   // gate pre-activations of every step [T][B][H][4] (gates of a unit together)
};

int ensure_side_stream(gvx_model* m);
int decoder_init_states(gvx_model* m, const float* memory, int B, int L, const DecoderBuffers& db, hipStream_t s);
int decoder_prenet_part(gvx_model* m, int B, int L, const float* mel_in, int T, const uint8_t* keep_masks, void* ws, const WsPlan& wp,
                        hipStream_t s);
int decoder_tf_impl(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, const float* mel_in, int T,
                    const uint8_t* keep_masks, float* mel_out, float* gate_out, float* align_out, void* ws, const WsPlan& wp,
                    hipStream_t s, bool prenet_done = false, const LstmDropout* train = nullptr);
int poison_if_timed_out(const gvx_model* m, int B, int L, void* ws, const WsPlan& wp, float* const* outs, const size_t* counts, int n,
                        hipStream_t s);

}  // namespace gvx
