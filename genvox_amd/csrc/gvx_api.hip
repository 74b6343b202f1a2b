// C-ABI of the MI355X Tacotron2 forward path (include/genvox_amd.h): model handle, host-side weight
// packing (BatchNorm folding, LSTM gate-row permutation, MFMA-fragment layout), workspace planning and
// the launch sequences of the encoder, the teacher-forced / autoregressive decoder and the Postnet.
//
// Data layout in HBM (all fp32):
//   activations are channels-last; conv inputs carry a zero halo of (k-1)/2 rows per sequence
//       encoder   x[B][L+2p][E]         memory[B][L][E]        pm[B][L][a]        xg[B][L][2*4H]
//       decoder   frames[(T+1)*B][M]    prenet[(T+1)*B][P]     (time-major: one step's rows are contiguous)
//                 hc[T+1][B][D+E]       slot s holds [h_d ; ctx] after step s-1 (slot 0 = zeros); it is at
//                                       once the LSTM input of the next step and the A operand of the hoisted
//                                       mel/gate projection GEMM over all T*B rows
//                 h_a[2][B][A] (ping-pong), c_a[B][A], c_d[B][D], w_cum[B][L], q_slab[A/8][B][a]
//       postnet   y[B][T+2p][C]
//   weights live in one packed blob (see pack_weights) so that multi-GPU start-up is a single broadcast.
//
// This file: the model handle and its knobs, workspace planning, the encoder, the Postnet, the fused forward, diagnostics.
// Weight packing is in gvx_pack.hip, the decoder loops and the plans that choose among them in gvx_decoder.hip.
#include "gvx_internal.h"

namespace gvx {
#ifdef GVX_STAMPS
hipError_t read_stamps_skinny(unsigned long long* host96);
hipError_t read_stamps_attention(unsigned long long* host96);
hipError_t read_stamps_persist(unsigned long long* host96);
hipError_t read_wg_spans(unsigned long long* host1024);
hipError_t read_stamps_resident(unsigned long long* host480);
hipError_t read_wg_stamps_resident(unsigned long long* host896);
hipError_t read_wg_stamps_resident_ar(unsigned long long* host896);
hipError_t read_row_stamps_persist_ar(unsigned long long* host256);
hipError_t read_loc_stamps_persist(unsigned long long* host32);
hipError_t read_row_stamps_persist(unsigned long long* host512);
#endif
hipError_t skinny_init();
hipError_t gemm_init();
int gemm_set_parent_epilogue(int on);   // gemm_f32.hip: > 0 every launch takes EPI_PARENT, 0 the kinds, < 0 only asks; returns what it was
int gemm_epilogue_of(int tile, const GemmParams& p);   // the epilogue kind (gemm_f32.hip's Epi) a launch of p on tile shape `tile` takes
hipError_t attention_init();
hipError_t attention_persistent_init();
}  // namespace gvx

using namespace gvx;

namespace {
thread_local std::string g_err;
std::mutex g_capture_mutex;
}
namespace gvx {
int set_error(int code, const char* msg) { g_err = msg; return code; }

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

std::mutex& capture_mutex() { return g_capture_mutex; }

bool conv_uses_winograd(const gvx_model* m, int cin, int cout, int k) {
    if (m->winograd <= 0 || !winograd_shape_ok(cin, cout, k)) return false;
    return m->winograd >= 2 || cin >= WINOGRAD_MIN_CHANNELS;
}

// Scratch of the Postnet's Winograd layers: V and M of one group of tiles, 2 x 8 x C floats per tile.  The whole batch where that
// stays inside WINOGRAD_GROUP_BYTES, else that budget in whole tiles (a layer then runs group after group; a group is any range
// of the batch's tiles, and where it is cut changes no value).  From the shape alone: a workspace amount must not depend on a knob.
size_t winograd_scratch_floats(const gvx_model* m, int B, int T) {
    bool any = false;
    for (int i = 0; i < m->d.postnet_n_conv; ++i) any = any || postnet_layer_winograd_shape(m->d, i);
    if (!any) return 0;
    const size_t tile = (size_t)2 * WINO_PTS * m->d.postnet_dim, all = (size_t)B * ((T + WINO_OUT - 1) / WINO_OUT) * tile;
    const size_t budget = WINOGRAD_GROUP_BYTES / sizeof(float) / tile * tile;
    return all <= budget ? all : budget > tile ? budget : tile;
}

// Tiles per group of a Winograd layer of `total` tiles whose scratch holds `fit` of them (C channels): as few groups as fit, as
// equal as they come - but every group except the last a whole number of rounds of the batched products' 128 x 128 tiles
// (gemm_round_rows), so that only the last group's products end in a remainder launch on a part of the chip.  Where a group ends
// changes no value.  One group where everything fits; where not even one round fits, the equal cut.
long winograd_group_tiles(long total, long fit, int C) {
    if (fit >= total) return total;
    const long groups = (total + fit - 1) / fit, per = (total + groups - 1) / groups;
    GemmParams g{};
    g.M = (int)per; g.N = C; g.K = C; g.slices = WINO_PTS;
    const long unit = gemm_round_rows(g);
    if (unit <= 0) return per;
    // a candidate: whole rounds, and still enough rows for the plan whose rounds they are
    auto whole = [&](long rows) { g.M = (int)rows; return rows > 0 && rows <= fit && rows % unit == 0 && gemm_round_rows(g) == unit; };
    const long down = per / unit * unit, up = (per + unit - 1) / unit * unit, most = fit / unit * unit;
    if (whole(down) && total - (groups - 1) * down <= fit) return down;   // the same number of groups, the last one the largest
    if (whole(up)) return up;                                             // ... the last one the smallest
    return whole(most) ? most : per;                                      // one or two groups more; or no round fits the scratch
}

WsPlan make_ws_plan(const gvx_model* m, int B, int L, int T, int mode) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, H = E / 2, M = d.n_mels, P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    const int pe = (d.enc_kernel - 1) / 2, pp = (d.postnet_kernel - 1) / 2;
    WsPlan w{};
    size_t off = 0;
    auto take = [&](size_t floats) { size_t o = off; off = align_up(off + floats * sizeof(float), 256); return o; };
    // status words first, at a shape-independent offset (gvx_workspace_status)
    w.flags = take(128);  // FLAG_* words; the sticky ones are only cleared by gvx_workspace_status
    w.sync = take(HANDOFF_WORDS);   // hand-off words of the persistent attention kernel (zeroed before every decoder loop)
    w.xa = take((size_t)B * (L + 2 * pe) * E);
    w.xb = take((size_t)B * (L + 2 * pe) * E);
    w.xg = take((size_t)B * L * 8 * H);
    w.enc_h = take((size_t)2 * 2 * B * H);
    w.enc_c = take((size_t)2 * B * H);
    w.memory = take((size_t)B * L * E);  // encoder output of the fused forward
    w.len_copy = take((size_t)B);        // token lengths copied next to the graphs' other operands (offset independent of T)
    w.pm = take((size_t)B * L * d.att_dim);
    w.frames = take((size_t)(T + 1) * B * M);
    w.pre1 = take((size_t)(T + 1) * B * P);
    w.prenet = take((size_t)(T + 1) * B * P);
    w.h_a = take((size_t)RS_HA_SLOTS * B * A);   // ping-pong of the launch-per-step loops; ring of the resident loop (dec_resident.hip)
    w.c_a = take((size_t)B * A);
    w.c_d = take((size_t)B * D);
    w.hc = take((size_t)(T + 1) * B * (D + E));
    w.w_cum = take((size_t)B * L);
    w.q_slab = take((size_t)(A / 8) * B * d.att_dim);
    w.proj = take((size_t)B * T * m->PSB());
    w.energies = take((size_t)B * L);
    w.align_tm = take((size_t)T * B * L);   // alignments of the step loop, time-major [T][B][L]
    w.loc = take((size_t)B * L * d.att_dim);  // location features of the current step
    w.p_slab = take((size_t)(D / 8) * B * m->PSB());   // autoregressive mode: projection partials of the decoder-LSTM tiles
    w.p_ctx = take((size_t)B * m->PSB());            //   and of the context columns (blocked vector)
    w.att_part = take((size_t)2 * B * 4 * A);        // autoregressive mode: partial gate pre-activations [B][4A] / [B][4D] of the
    w.dec_part = take((size_t)2 * B * 4 * D);        //   column slices that are known one launch early (two buffers: the 64-row
                                                     //   teacher-forced loop finishes a decoder cell one launch after its partial)
    // teacher-forced loop beside the persistent attention kernel: Prenet contribution to the attention LSTM's gates, all steps
    // (only where that loop can run: 0.5 GB at B = 32, T = 1000 that the autoregressive / launch-per-step paths never touch)
    w.pre_gate = take(mode == WS_TEACHER_FORCED && plan_teacher_forced(m, B, L, TF_INFERENCE).pre_gate ? (size_t)T * B * 4 * A : 0);
    w.xchg = take(attention_persistent_xchg_floats(B));   // split resident kernel (128 < L <= 256): exchange buffers of the row halves
    w.ar_masks = take(((size_t)2 * T * B * P + 3) / 4);  // autoregressive mode: keep masks copied next to the graphs' operands (bytes)
    const int cmax = d.postnet_dim > M ? d.postnet_dim : M;
    w.ya = take((size_t)B * (T + 2 * pp) * cmax);
    w.yb = take((size_t)B * (T + 2 * pp) * cmax);
    // (the Postnet's Winograd scratch inside the fused forward is [xa, ya): every buffer of the encoder and the decoder is dead
    // once the projection has been split into mel_out and gate_out - the status and hand-off words sit in front of xa)
    w.total = off;
    return w;
}

// Find (or create, evicting the least recently used) the graph set of `key` and count the sighting.
gvx_model::GraphSet* touch_graph_set(gvx_model* m, std::vector<gvx_model::GraphSet>& cache, const gvx_model::LoopKey& key) {
    gvx_model::GraphSet* hit = nullptr;
    for (auto& gs : cache)
        if (gs.key == key) hit = &gs;
    if (!hit) {
        if (cache.size() >= gvx_model::GRAPH_SETS) {
            size_t lru = 0;
            for (size_t i = 1; i < cache.size(); ++i)
                if (cache[i].last_use < cache[lru].last_use) lru = i;
            for (auto e : cache[lru].execs)
                if (e) (void)hipGraphExecDestroy(e);
            cache.erase(cache.begin() + lru);
        }
        cache.emplace_back();
        hit = &cache.back();
        hit->key = key;
    }
    ++hit->sightings;
    hit->last_use = ++m->use_clock;
    return hit;
}

int check_common(const gvx_model* m, int B, int L, int T, void* ws, size_t ws_bytes, int mode) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null model");
    if (!m->dev_blob) return fail(GVX_ERR_STATE, "weights not bound (call gvx_model_bind_blob)");
    if (B < 1 || B > 64) return fail(GVX_ERR_UNSUPPORTED, "batch %d not in [1, 64] (shard larger batches across calls / GPUs)", B);
    if (L < 1 || T < 1) return fail(GVX_ERR_INVALID_ARG, "L and T must be >= 1");
    if (!ws) return fail(GVX_ERR_WORKSPACE, "null workspace");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(GVX_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    const size_t need = make_ws_plan(m, B, L, T, mode).total;
    if (ws_bytes < need) return fail(GVX_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
    if (!attention_supported(L, m->d.att_dim, m->d.att_loc_filters, m->d.att_loc_kernel, m->d.embed_dim))
        return fail(GVX_ERR_UNSUPPORTED, "L = %d is too long for the attention kernels' LDS budget", L);
    return GVX_OK;
}

}  // namespace gvx

namespace {

int check_dims(const gvx_dims& d) {
    if (d.n_tokens < 1) return fail(GVX_ERR_INVALID_ARG, "n_tokens must be >= 1");
    const int dims8[] = {d.embed_dim, d.prenet_dim, d.att_rnn_dim, d.dec_rnn_dim, d.att_dim, d.postnet_dim, d.n_mels};
    const char* names[] = {"embed_dim", "prenet_dim", "att_rnn_dim", "dec_rnn_dim", "att_dim", "postnet_dim", "n_mels"};
    for (int i = 0; i < 7; ++i)
        if (dims8[i] < 8 || dims8[i] % 8) return fail(GVX_ERR_UNSUPPORTED, "%s = %d must be a positive multiple of 8", names[i], dims8[i]);
    if (d.embed_dim % 16) return fail(GVX_ERR_UNSUPPORTED, "embed_dim = %d must be a multiple of 16 (BiLSTM halves are multiples of 8)", d.embed_dim);
    if (d.att_dim > 256) return fail(GVX_ERR_UNSUPPORTED, "att_dim = %d > 256 is not supported", d.att_dim);
    if (d.att_loc_filters < 1 || d.att_loc_filters > 32) return fail(GVX_ERR_UNSUPPORTED, "att_loc_filters = %d must be in [1, 32]", d.att_loc_filters);
    const int ks[] = {d.enc_kernel, d.att_loc_kernel, d.postnet_kernel};
    for (int k : ks)
        if (k < 1 || k % 2 == 0) return fail(GVX_ERR_UNSUPPORTED, "kernel size %d must be odd (the reference pads (k-1)/2 on both sides)", k);
    if (d.enc_n_conv < 1 || d.enc_n_conv > MAX_CONV || d.postnet_n_conv < 1 || d.postnet_n_conv > MAX_CONV)
        return fail(GVX_ERR_UNSUPPORTED, "number of convolutions must be in [1, %d]", MAX_CONV);
    return GVX_OK;
}

// Every GVX_* variable the C-ABI layer honours (meanings: the fields of gvx_model), read when the handle is created.
void read_knobs(gvx_model* m) {
    auto env = [](const char* name) { const char* e = std::getenv(name); return e ? e : ""; };
    auto flag = [&](const char* name, bool dflt) { const char c = env(name)[0]; return c == '\0' ? dflt : dflt ? c != '0' : c == '1'; };   // default on: "0" clears; default off: "1" sets
    auto number = [&](const char* name, int dflt) { const char* e = env(name); return e[0] ? std::atoi(e) : dflt; };
    m->use_graph = !flag("GVX_NO_GRAPH", false);
    m->capture_first = flag("GVX_GRAPH_FIRST", false);
    m->attn_one_launch = !flag("GVX_ATTN_SPLIT", false);
    m->attn_persistent = flag("GVX_ATTN_PERSISTENT", true);
    // the resident attention kernel and the launches it feeds must run at the same time: under kernel serialisation every
    // hand-off would run into its limit
    for (const char* name : {"AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING"})
        if (env(name)[0] != '\0' && env(name)[0] != '0') m->attn_persistent = false;
    m->ar_resident = flag("GVX_AR_RESIDENT", false);
    m->ar_split_h = flag("GVX_AR_SPLIT_H", true);
    m->enc_persistent = flag("GVX_ENC_PERSISTENT", true);
    m->enc_fork_after = number("GVX_ENC_FORK_AFTER", 2);
    m->train_resident = flag("GVX_TRAIN_RESIDENT", true);
    m->train_resident_loop = flag("GVX_TRAIN_RESIDENT_LOOP", true);
    m->tf_rows64 = flag("GVX_TF_ROWS64", false);
    m->tf_resident = flag("GVX_TF_RESIDENT", true);
    m->ar_resident_loop = flag("GVX_AR_RESIDENT_LOOP", true);
    m->tf_long_rows_224 = flag("GVX_TF_LONG_224", true);
    m->attn_prefetch = flag("GVX_ATTN_PREFETCH", true);
    m->pa_depth = number("GVX_PA_DEPTH", 4) == 6 ? 6 : 4;
    m->side_pool = env("GVX_SIDE_POOL")[0] == '2' ? 2u : 1u;
    m->spin_limit = (unsigned)std::strtoul(env("GVX_HANDOFF_SPIN_LIMIT"), nullptr, 10);
    m->rs_debug = number("GVX_RS_DEBUG", 0);
    m->debug_skip_resident = flag("GVX_DEBUG_SKIP_RESIDENT", false);
    m->debug_enc_skip_block = number("GVX_DEBUG_ENC_SKIP_BLOCK", -1);
    m->debug_plan = std::getenv("GVX_DEBUG_PLAN") != nullptr;
    m->winograd = number("GVX_CONV_WINOGRAD", 1);
    if (m->winograd < 0 || m->winograd > 2) m->winograd = 1;
}

}  // namespace

// =====================================================================================================
extern "C" {

const char* gvx_last_error(void) { return g_err.c_str(); }
int gvx_version(void) { return 1; }

int gvx_model_create(const gvx_dims* dims, gvx_model** out) {
    if (!dims || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc = check_dims(*dims);
    if (rc != GVX_OK) return rc;
    gvx_model* m = new gvx_model();
    m->d = *dims;
    m->blob = make_blob_layout(*dims);
    read_knobs(m);
    *out = m;
    return GVX_OK;
}

void gvx_model_destroy(gvx_model* m) {
    if (m) {
        if (m->gather_off) (void)hipFree(m->gather_off);
        if (m->gather_tid) (void)hipFree(m->gather_tid);
    }
    if (!m) return;
    if (m->ev_valid)
        for (auto& e : m->ev) (void)hipEventDestroy(e);
    for (auto& e : m->kev) (void)hipEventDestroy(e);
    m->drop_graphs();
    if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
    // (pa_stream belongs to the process-wide side-stream pool)
    if (m->pa_fork) (void)hipEventDestroy(m->pa_fork);
    if (m->pa_join) (void)hipEventDestroy(m->pa_join);
    if (m->enc_mid) (void)hipEventDestroy(m->enc_mid);
    if (m->ar_done_host) (void)hipHostFree(m->ar_done_host);
    for (hipEvent_t e : m->ar_ev)
        if (e) (void)hipEventDestroy(e);
    delete m;
}

size_t gvx_model_blob_bytes(const gvx_model* m) { return m ? m->blob.total * sizeof(float) : 0; }

int gvx_model_bind_blob(gvx_model* m, const void* device_blob) {
    if (!m || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(device_blob) & 255) return fail(GVX_ERR_INVALID_ARG, "blob must be 256-byte aligned");
    // captured step loops bake blob addresses into their kernel nodes: a new blob invalidates every cached graph (the
    // key carries the blob pointer as well, so a stale graph could not be selected even if one survived)
    if (m->dev_blob != device_blob) m->drop_graphs();
    m->dev_blob = reinterpret_cast<const float*>(device_blob);
    HIP_TRY(gemm_init());
    HIP_TRY(skinny_init());
    HIP_TRY(attention_init());
    HIP_TRY(attention_persistent_init());
    HIP_TRY(decoder_resident_init());
    return GVX_OK;
}

size_t gvx_workspace_bytes(const gvx_model* m, int B, int L, int T) {
    if (!m || B < 1 || L < 1 || T < 1) return 0;
    return make_ws_plan(m, B, L, T).total;
}

size_t gvx_workspace_bytes_autoregressive(const gvx_model* m, int B, int L, int max_steps) {
    if (!m || B < 1 || L < 1 || max_steps < 1) return 0;
    return make_ws_plan(m, B, L, max_steps, WS_AUTOREGRESSIVE).total;
}

}  // extern "C"

// =====================================================================================================
namespace {

// conv stack on channels-last halo buffers: in -> (ping/pong) ; returns pointer of the final output buffer
int conv_layer(const gvx_model* m, const float* in, float* out, int B, int T, int cin, int cout, int k, size_t w_off, size_t b_off,
               int act, int out_halo, hipStream_t s) {
    const int p = (k - 1) / 2;
    GemmParams g{};
    g.A = in; g.amap = RowMap{T, (long)(T + 2 * p) * cin, (long)cin};
    g.W = m->dev_blob + w_off; g.ldw = (long)k * cin;
    g.C = out + (long)out_halo * cout; g.cmap = RowMap{T, (long)(T + 2 * out_halo) * cout, (long)cout};
    g.bias = m->dev_blob + b_off;
    g.M = B * T; g.N = cout; g.K = k * cin; g.act = act;
    HIP_TRY(launch_gemm(g, s));
    return GVX_OK;
}

// One k = 5, C -> C convolution layer as Winograd F(4,5) on the halo buffers cur -> nxt ([B][T + 4][C]): input transform, eight
// products in one batched launch, output transform (bias, act, row_len, the halo rows of nxt).  wino: wino_floats floats of
// scratch; V and M are written whole before they are read, group by group (winograd_group_tiles).
int winograd_layer(const gvx_model* m, const char* who, const float* cur, float* nxt, int B, int T, int C, size_t u_off, size_t b_off,
                   const int32_t* row_len, int act, float* wino, size_t wino_floats, hipStream_t s) {
    const long total = (long)B * ((T + WINO_OUT - 1) / WINO_OUT);
    const size_t tile = (size_t)2 * WINO_PTS * C, budget = WINOGRAD_GROUP_BYTES / sizeof(float);
    long fit = (long)((wino_floats < budget ? wino_floats : budget) / tile);
    if (fit < 1) return fail(GVX_ERR_WORKSPACE, "%s: %zu floats of scratch do not hold one Winograd tile (%zu)", who, wino_floats, tile);
    if (m->wino_group > 0 && m->wino_group < fit) fit = m->wino_group;
    const long per_group = winograd_group_tiles(total, fit, C);
    for (long mt0 = 0, Mt; mt0 < total; mt0 += Mt) {
        Mt = total - mt0 <= fit ? total - mt0 : per_group;   // (the last group takes what is left: at most `fit`, not at most per_group)
        float* V = wino;
        float* Mm = wino + (size_t)WINO_PTS * Mt * C;
        HIP_TRY(launch_winograd_input(cur, V, B, mt0, Mt, T, C, s));
        GemmParams g{};
        g.A = V; g.amap = RowMap{(int)Mt, 0, (long)C};
        g.W = m->dev_blob + u_off; g.ldw = C;
        g.C = Mm; g.cmap = RowMap{(int)Mt, 0, (long)C};
        g.bias = nullptr; g.M = (int)Mt; g.N = C; g.K = C; g.act = ACT_NONE;
        g.slices = WINO_PTS; g.a_slice = Mt * C; g.w_slice = (long)C * C; g.c_slice = Mt * C;
        HIP_TRY(launch_gemm(g, s));
        HIP_TRY(launch_winograd_output(Mm, m->dev_blob + b_off, row_len, nxt, B, mt0, Mt, T, C, act, s));
    }
    return GVX_OK;
}

// Scratch of the encoder's layers that run as Winograd F(4,5) (V and M of a group of tiles): workspace regions that are dead while the
// convolutions run, so that no workspace grows for them.
//   alone == true  (gvx_encoder_forward: nothing else runs on the workspace): everything from xg to the end of the plan the call
//                  checked the workspace against - xg .. pm are written behind the convolutions, the rest belongs to a decoder call.
//   alone == false (the fused forward, whose Prenet products write frames, pre1, prenet and pre_gate on the caller's stream at
//                  the same time - decoder_prenet_part): the larger of [xg, frames) - xg, enc_h, enc_c, memory, len_copy, pm, all
//                  written on the encoder's stream behind the convolutions - and [h_a, pre_gate) - the decoder's states and
//                  step buffers, first touched by decoder_init_states on the encoder's stream behind the encoder.
struct WinoScratch { size_t off, floats; };
WinoScratch encoder_wino_scratch(const WsPlan& wp, bool alone) {
    if (alone) return {wp.xg, (wp.total - wp.xg) / sizeof(float)};
    const size_t front = wp.frames - wp.xg, back = wp.pre_gate - wp.h_a;
    return front >= back ? WinoScratch{wp.xg, front / sizeof(float)} : WinoScratch{wp.h_a, back / sizeof(float)};
}

// conv_out (training mode only): the output of the convolution stack, [B, E, L] in the reference's layout, computed by the
// caller with batch statistics and dropout (gvx_conv_bn_act_train_forward); the embedding and the folded-BatchNorm
// convolutions are then skipped and only the BiLSTM part runs
int encoder_impl(gvx_model* m, const int64_t* tokens, const int32_t* lengths, int B, int L, float* memory_out, void* ws,
                 const WsPlan& wp, const WinoScratch& wsc, hipStream_t s, const float* conv_out = nullptr, float* c_seq_out = nullptr,
                 float* xg_out = nullptr, hipEvent_t dense_done = nullptr) {   // dense_done: recorded on s behind the convolutions (see below)
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, H = E / 2, pe = (d.enc_kernel - 1) / 2;
    float* xa = ws_ptr<float>(ws, wp.xa);
    float* xb = ws_ptr<float>(ws, wp.xb);
    float* xg = ws_ptr<float>(ws, wp.xg);
    float* enc_h = ws_ptr<float>(ws, wp.enc_h);
    float* enc_c = ws_ptr<float>(ws, wp.enc_c);
    int* flags = ws_ptr<int>(ws, wp.flags);
    float* cur = xa;
    float* nxt = xb;
    if (conv_out) {
        HIP_TRY(launch_to_channels_last(conv_out, xa, B, E, L, pe, nullptr, s));
    } else {
        // (the token-error word is sticky: raised here, cleared only by gvx_workspace_status - a later chunk on the same
        // workspace must not wipe an earlier chunk's error)
        HIP_TRY(launch_embed(tokens, m->dev_blob + m->blob.emb, d.n_tokens, xa, xb, B, L, E, pe, flags + FLAG_TOKEN, s));   // (+ the halo rows of xa and xb)
        for (int i = 0; i < d.enc_n_conv; ++i) {
            if (dense_done && i == m->enc_fork_after) { HIP_TRY(hipEventRecord(dense_done, s)); dense_done = nullptr; }
            // (the choice looks at the layer's shape and the handle's mode alone: a row's bits must not depend on B or L)
            const bool wino = encoder_layer_winograd_shape(d, i) && conv_uses_winograd(m, E, E, d.enc_kernel);
            int rc = wino ? winograd_layer(m, "encoder", cur, nxt, B, L, E, m->blob.enc_u[i], m->blob.enc_b[i], nullptr, ACT_RELU,
                                           ws_ptr<float>(ws, wsc.off), wsc.floats, s)
                          : conv_layer(m, cur, nxt, B, L, E, E, d.enc_kernel, m->blob.enc_w[i], m->blob.enc_b[i], ACT_RELU, pe, s);
            if (rc != GVX_OK) return rc;
            float* t = cur; cur = nxt; nxt = t;
        }
    }
    // (the fork event of the caller's other dense products, if the convolution loop has not recorded it: training mode, or
    // GVX_ENC_FORK_AFTER >= the number of convolutions)
    if (dense_done) HIP_TRY(hipEventRecord(dense_done, s));
    {   // LSTM input projection for both directions: xg[b][l][dir*4H + 4j+gate]
        GemmParams g{};
        g.A = cur + (long)pe * E; g.amap = RowMap{L, (long)(L + 2 * pe) * E, (long)E};
        g.W = m->dev_blob + m->blob.enc_wih; g.ldw = E;
        g.C = xg; g.cmap = RowMap{B * L, 0, (long)8 * H};
        g.bias = m->dev_blob + m->blob.enc_bih;
        g.M = B * L; g.N = 8 * H; g.K = E; g.act = ACT_NONE;
        HIP_TRY(launch_gemm(g, s));
    }
    const bool resident = m->enc_persistent && encoder_persistent_supported(B, H);
    if (!resident) HIP_TRY(zero_async(enc_h, (size_t)4 * B * H * sizeof(float), s));
    if (!resident) HIP_TRY(zero_async(enc_c, (size_t)2 * B * H * sizeof(float), s));   // (the resident kernel keeps the cells in registers)
    // The L recurrence launches only reference workspace operands: lengths are copied next to them and the sequence output
    // goes to the workspace-resident memory buffer (copied to the caller's tensor afterwards when that is a different
    // one), so the key of the cached hipGraph does not depend on a freshly allocated output tensor.
    float* mem_ws = ws_ptr<float>(ws, wp.memory);
    if (!resident) HIP_TRY(zero_async(mem_ws, (size_t)B * L * E * sizeof(float), s));   // (the resident kernel writes every position)
    const int32_t* len_ws = nullptr;
    if (lengths) {
        int32_t* lc = ws_ptr<int32_t>(ws, wp.len_copy);
        HIP_TRY(hipMemcpyAsync(lc, lengths, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        len_ws = lc;
    }
    auto enqueue = [&](hipStream_t st) -> int {
        for (int step = 0; step < L; ++step) {
            SkinnyJob jobs[2];
            for (int dir = 0; dir < 2; ++dir) {
                SkinnyJob& J = jobs[dir];
                std::memset(&J, 0, sizeof J);
                float* h_cur = enc_h + ((size_t)dir * 2 + (step & 1)) * B * H;
                float* h_nxt = enc_h + ((size_t)dir * 2 + ((step + 1) & 1)) * B * H;
                J.Wp = m->dev_blob + m->blob.enc_whh_frag[dir];
                J.x[0] = XSeg{h_cur, H};
                J.N = 4 * H; J.nkg = H / 8; J.mode = 0; J.B = B;
                J.c = enc_c + (size_t)dir * B * H;
                J.h_out = h_nxt;
                J.addend = xg + (size_t)dir * 4 * H; J.add_bs = (long)L * 8 * H; J.add_ts = 8 * H;
                J.lengths = len_ws; J.step = step; J.reverse = dir; J.seq_len = L;
                J.seq_out = mem_ws + (size_t)dir * H; J.seq_bs = (long)L * E; J.seq_ts = E;
                if (c_seq_out) J.c_seq_out = c_seq_out + (size_t)dir * H;   // (training tape; the loop is then not replayed from a graph)
                J.h_prev = h_cur;
            }
            HIP_TRY(launch_skinny(jobs, 2, SK_ENCODER, st));
        }
        return GVX_OK;
    };
    if (resident) {
        // one resident launch for the whole recurrence (skinny.hip, encoder_lstm_persistent_kernel); a hand-off that times out
        // leaves NaN in the encoder output and raises the sticky status word, like the resident decoder loops
        unsigned* sync = ws_ptr<unsigned>(ws, wp.sync);
        void* const zp[2] = {enc_h, sync + HANDOFF_TIMEOUT};   // the exchange buffers (generation bits 0), the call's time-out word
        const size_t zb[2] = {(size_t)4 * B * H * sizeof(float), sizeof(unsigned)};
        HIP_TRY(launch_zero_many(zp, zb, 2, s));
        EncPersistParams ep{};
        ep.Wp[0] = m->dev_blob + m->blob.enc_whh_frag[0]; ep.Wp[1] = m->dev_blob + m->blob.enc_whh_frag[1];
        ep.xg = xg; ep.lengths = len_ws; ep.hx = enc_h; ep.seq_out = mem_ws; ep.c_seq_out = c_seq_out;
        ep.sync = sync; ep.spin_limit = m->spin_limit; ep.B = B; ep.L = L; ep.H = H;
        ep.debug_skip_block = m->debug_enc_skip_block;
        HIP_TRY(launch_encoder_persistent(ep, s));
        float* outs[2] = {mem_ws, c_seq_out};
        const size_t counts[2] = {(size_t)B * L * E, (size_t)B * L * E};
        HIP_TRY(launch_poison_on_timeout(sync + HANDOFF_TIMEOUT, flags + FLAG_TIMEOUT, outs, counts, c_seq_out ? 2 : 1, s));
    } else {
        const gvx_model::LoopKey key{ws, mem_ws, m->dev_blob, B, L, 0, lengths != nullptr};
        const int rc = run_chunk(m, m->use_graph && !c_seq_out ? touch_graph_set(m, m->enc_graphs, key) : nullptr, 0, s, enqueue);
        if (rc != GVX_OK) return rc;
    }
    if (xg_out) HIP_TRY(hipMemcpyAsync(xg_out, xg, (size_t)B * L * 8 * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (memory_out != mem_ws)
        HIP_TRY(hipMemcpyAsync(memory_out, mem_ws, (size_t)B * L * E * sizeof(float), hipMemcpyDeviceToDevice, s));
    return GVX_OK;
}

// Postnet + residual on channels-last halo buffers ya / yb (each B * (T + 2p) * max(postnet_dim, n_mels) floats).
// mel_lengths (optional): row b is treated as a sequence of mel_lengths[b] frames - the input and every layer's output
// are zero from that frame on, exactly what the convolutions of a batch-1 run see as padding at the sequence end.
// wino: wino_floats floats of scratch (V and M of one group of tiles) for the layers that run as Winograd F(4,5); at least one
// tile's worth, more than WINOGRAD_GROUP_BYTES is not used.
int postnet_impl(gvx_model* m, const float* mel_in, const int32_t* mel_lengths, int B, int T, float* mel_post_out, float* ya,
                 float* yb, float* wino, size_t wino_floats, hipStream_t s) {
    const gvx_dims& d = m->d;
    const int M = d.n_mels, pp = (d.postnet_kernel - 1) / 2, n = d.postnet_n_conv;
    // every conv input needs zero halo rows in ITS channel layout: the producer of a buffer writes them (the transpose for
    // the first one, the GEMM epilogue of layer i for layer i + 1; a separate launch only when T < halo)
    HIP_TRY(launch_to_channels_last(mel_in, ya, B, M, T, pp, mel_lengths, s));
    float* cur = ya;
    float* nxt = yb;
    for (int i = 0; i < n; ++i) {
        const int cin = i == 0 ? M : d.postnet_dim, cout = i == n - 1 ? M : d.postnet_dim;
        const bool last = i == n - 1;
        if (postnet_layer_winograd_shape(d, i) && conv_uses_winograd(m, cin, cout, d.postnet_kernel)) {
            const int rc = winograd_layer(m, "Postnet", cur, nxt, B, T, cin, m->blob.post_u[i], m->blob.post_b[i], mel_lengths, ACT_TANH, wino, wino_floats, s);
            if (rc != GVX_OK) return rc;
            float* t = cur; cur = nxt; nxt = t;
            continue;
        }
        const int out_halo = last ? 0 : pp;
        const bool fused_halo = out_halo > 0 && T >= out_halo;
        if (out_halo > 0 && !fused_halo) HIP_TRY(launch_zero_halo(nxt, B, T, pp, cout, s));
        GemmParams g{};
        g.A = cur; g.amap = RowMap{T, (long)(T + 2 * pp) * cin, (long)cin};
        g.W = m->dev_blob + m->blob.post_w[i]; g.ldw = (long)d.postnet_kernel * cin;
        g.C = nxt + (long)out_halo * cout; g.cmap = RowMap{T, (long)(T + 2 * out_halo) * cout, (long)cout};
        g.bias = m->dev_blob + m->blob.post_b[i];
        g.M = B * T; g.N = cout; g.K = d.postnet_kernel * cin; g.act = last ? ACT_NONE : ACT_TANH;
        g.row_len = last ? nullptr : mel_lengths;   // the last layer's padding is zeroed by the residual kernel
        g.c_halo = fused_halo ? out_halo : 0;
        HIP_TRY(launch_gemm(g, s));
        float* t = cur; cur = nxt; nxt = t;
    }
    HIP_TRY(launch_residual_to_channels_first(mel_in, cur, mel_post_out, B, M, T, mel_lengths, s));
    return GVX_OK;
}

struct PostnetPlan { size_t ya, yb, wino, wino_floats, total; };
PostnetPlan make_postnet_plan(const gvx_model* m, int B, int T) {
    const gvx_dims& d = m->d;
    const int pp = (d.postnet_kernel - 1) / 2, cmax = d.postnet_dim > d.n_mels ? d.postnet_dim : d.n_mels;
    const size_t buf = align_up((size_t)B * (T + 2 * pp) * cmax * sizeof(float), 256);
    PostnetPlan p;
    p.ya = align_up((128 + HANDOFF_WORDS) * sizeof(float), 256);   // behind the status and hand-off words of the full plan
    p.yb = p.ya + buf;
    p.wino = p.yb + buf;
    // the Winograd scratch, but never more than the model workspaces have in front of their own ya for the shortest row (those
    // promise to hold a Postnet call: gvx_workspace_bytes_autoregressive and gvx_workspace_bytes are not to grow for it)
    const WsPlan w = make_ws_plan(m, B, 1, T, WS_AUTOREGRESSIVE);
    const size_t tile = (size_t)2 * WINO_PTS * d.postnet_dim, room = (w.ya - w.xa) / sizeof(float) / tile * tile;
    p.wino_floats = winograd_scratch_floats(m, B, T);
    if (p.wino_floats > room) p.wino_floats = room > tile ? room : tile;
    p.total = p.wino + align_up(p.wino_floats * sizeof(float), 256);
    return p;
}

}  // namespace

// =====================================================================================================
extern "C" {

int gvx_teacher_forced_rows_per_call(const gvx_model* m, int L) {
    if (!m) return 0;
    return plan_teacher_forced(m, 64, L, TF_INFERENCE).kind != 0 ? 64 : 32;
}

int gvx_teacher_forced_resident(const gvx_model* m, int B, int L) {
    if (!m || B < 1 || L < 1) return 0;
    return plan_teacher_forced(m, B, L, TF_INFERENCE).kind != 0 ? 1 : 0;
}

int gvx_teacher_forced_loop_kind(const gvx_model* m, int B, int L) {
    if (!m || B < 1 || L < 1) return 0;
    return plan_teacher_forced(m, B, L, TF_INFERENCE).kind;
}

int gvx_autoregressive_loop_kind(const gvx_model* m, int B, int L) {
    if (!m || B < 1 || L < 1) return 0;
    return plan_autoregressive(m, B, L).kind;
}

int gvx_autoregressive_windowed_loop_kind(const gvx_model* m, int B, int L) {
    if (!m || B < 1 || L < 1) return 0;
    return plan_autoregressive(m, B, L, true).kind;
}

// Host-only query for the tests (not in the public header): the ArLoopPlan of a windowed autoregressive call,
// out[0..3] = {kind, split_h, fold, graph} - plan_autoregressive(m, B, L, true), the function gvx_decoder_autoregressive_windowed calls.
int gvx_debug_decoder_plan_windowed(const gvx_model* m, int B, int L, int* out) {
    if (!m || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || L < 1) return fail(GVX_ERR_INVALID_ARG, "B, L >= 1 (got %d, %d)", B, L);
    const ArLoopPlan a = plan_autoregressive(m, B, L, true);
    out[0] = a.kind; out[1] = a.split_h; out[2] = a.fold; out[3] = a.graph;
    return GVX_OK;
}

// Host-only queries for the tests, like gvx_debug_gemm_plan / gvx_debug_bptt_plan (not in the public header).  Every field of the
// two loop plans for (B, L) on this handle - the same two functions the loops call, no device touched.  mode: 0 inference, 1 training
// call with the whole tape, 2 training call with a partial tape.  out[0..7] = TfLoopPlan {kind, pa_layout, tile_layout, rows64,
// pre_gate, timeout_check, side_stream, graph}; out[8..11] = ArLoopPlan {kind, split_h, fold, graph}.
int gvx_debug_decoder_plan(const gvx_model* m, int mode, int B, int L, int* out) {
    if (!m || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (mode < 0 || mode > 2 || B < 1 || L < 1) return fail(GVX_ERR_INVALID_ARG, "mode must be 0, 1 or 2 and B, L >= 1 (got %d, %d, %d)", mode, B, L);
    const TfLoopPlan t = plan_teacher_forced(m, B, L, (TfMode)mode);
    const ArLoopPlan a = plan_autoregressive(m, B, L);
    const int v[12] = {t.kind, t.pa_layout, t.tile_layout, t.rows64, t.pre_gate, t.timeout_check, t.side_stream, t.graph,
                       a.kind, a.split_h, a.fold, a.graph};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return GVX_OK;
}

// hipGraph launches this handle has made since it was created (run_chunk: the encoder's launch-per-position loop, the
// teacher-forced step loops, the 16-step chunks of the autoregressive loop).  An eager first sighting and a capture do not count.
long long gvx_debug_graph_replays(const gvx_model* m) { return m ? (long long)m->graph_replays : -1; }

// 1 if gvx_encoder_forward / gvx_encoder_lstm_forward run the recurrence of B rows as the one resident launch on this handle
// (GVX_ENC_PERSISTENT and encoder_persistent_supported: B <= 32, H = 256), 0 for the launch per position.
int gvx_debug_encoder_resident(const gvx_model* m, int B) {
    if (!m || B < 1) return 0;
    return m->enc_persistent && encoder_persistent_supported(B, m->H()) ? 1 : 0;
}

int gvx_model_set_persistent_attention(gvx_model* m, int enable) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null argument");
    m->attn_persistent = enable != 0;
    return GVX_OK;
}

int gvx_model_set_winograd(gvx_model* m, int mode) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (mode < 0 || mode > 2) return fail(GVX_ERR_INVALID_ARG, "winograd mode must be 0, 1 or 2 (got %d)", mode);
    m->winograd = mode;
    return GVX_OK;
}

// 1: a Postnet or encoder convolution layer of this shape runs as Winograd F(4,5) on this handle, 0: as the direct implicit GEMM
// (conv_uses_winograd, the function postnet_impl and encoder_impl ask); host arithmetic only
int gvx_debug_conv_plan(const gvx_model* m, int cin, int cout, int k) {
    if (!m || cin < 1 || cout < 1 || k < 1) return -1;
    return conv_uses_winograd(m, cin, cout, k) ? 1 : 0;
}

// Host-only, for the tests (not in the public header).  Tiles of four frames per Winograd group: 0 = as the scratch allows,
// n > 0 = at most n (where a group ends must not change a bit)
int gvx_debug_set_winograd_group(gvx_model* m, int tiles) {
    if (!m || tiles < 0) return fail(GVX_ERR_INVALID_ARG, "bad argument");
    m->wino_group = tiles;
    return GVX_OK;
}

// Host-only, for the tests (not in the public header): tiles per group of a C-channel Winograd layer of `total` tiles whose scratch
// holds `fit` of them (winograd_group_tiles, the function the layers ask); -1 on a bad argument
long gvx_debug_winograd_group_tiles(long total, long fit, int channels) {
    if (total < 1 || fit < 1 || channels < 4 || total > INT_MAX) return -1;
    return winograd_group_tiles(total, fit, channels);
}

// Host-only, for the tests and A/B runs (not in the public header; process-wide, like GVX_GEMM_8W): on > 0 makes every fp32
// GEMM launch take the epilogue the kernels had before the compile-time kinds (EPI_PARENT), 0 switches back, < 0 only asks.
// Returns the setting as it was.  Starts out as GVX_GEMM_EPILOGUE=parent in the environment says (unset: the kinds).
int gvx_debug_gemm_parent_epilogue(int on) { return gemm_set_parent_epilogue(on); }

// Host-only, for the tests (not in the public header; no device touched): the epilogue kind a launch on tile shape `tile` (four
// digits, as gvx_debug_gemm_plan reports it) takes when its parameters ask for these extras - 0 the parent's epilogue (the
// switch above), 1 general, 2 plain, 3 bias only; the function launch_gemm asks.  -1: a bad argument.
int gvx_debug_gemm_epilogue(int tile, int kmajor, int has_bias, int act, int has_keep, int has_row_len, int c_halo) {
    if (tile < 1111 || tile > 9999 || c_halo < 0) return -1;
    static const float some_bias = 0.f; static const uint8_t some_keep = 0; static const int32_t some_len = 0;
    GemmParams g{};
    g.kmajor = kmajor != 0;
    g.bias = has_bias ? &some_bias : nullptr; g.act = act;
    g.keep = has_keep ? &some_keep : nullptr; g.row_len = has_row_len ? &some_len : nullptr; g.c_halo = c_halo;
    return gemm_epilogue_of(tile, g);
}

// Host-only, for the tests (not in the public header; no device touched): the GEMM epilogue's row walk for one lane and M tile.
// out row q (0..15) is the tile row first_row + (q & 3) + 8 * (q >> 2), reached as the kernel reaches it - row_walk_begin at
// first_row, row_walk_advance by mfma32_row_step(q) from there: off[q], grp[q], idx[q] under the map (R, s1, s0).
int gvx_debug_gemm_row_walk(int R, long s1, long s0, int first_row, long* off, int* grp, int* idx) {
    if (R < 1 || first_row < 0 || !off || !grp || !idx) return GVX_ERR_INVALID_ARG;
    const RowMap map{R, s1, s0};
    RowWalk w = row_walk_begin(map, first_row);
    for (int q = 0; q < 16; ++q) {
        if (q > 0) row_walk_advance(w, map, mfma32_row_step(q));
        off[q] = w.off; grp[q] = w.grp; idx[q] = w.idx;
    }
    return GVX_OK;
}

// The transform matrices of winograd_f45.h as doubles: at[4][8], g[8][5], bt[8][8]
int gvx_debug_winograd_constants(double* at, double* g, double* bt) {
    if (!at || !g || !bt) return fail(GVX_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < WINO_OUT; ++i)
        for (int s = 0; s < WINO_PTS; ++s) at[i * WINO_PTS + s] = wino_AT(i, s);
    for (int s = 0; s < WINO_PTS; ++s) {
        for (int k = 0; k < WINO_TAPS; ++k) g[s * WINO_TAPS + k] = wino_G(s, k);
        for (int i = 0; i < WINO_PTS; ++i) bt[s * WINO_PTS + i] = wino_BT(s, i);
    }
    return GVX_OK;
}

int gvx_model_set_resident_kernels(gvx_model* m, int enable) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null argument");
    m->attn_persistent = m->enc_persistent = m->tf_resident = enable != 0;
    if (!enable) m->ar_resident = false;
    return GVX_OK;
}

int gvx_workspace_status(const gvx_model* m, void* ws, size_t ws_bytes, void* stream, int32_t* host_out) {
    if (!m || !ws || !host_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const WsPlan wp = make_ws_plan(m, 1, 1, 1, WS_AUTOREGRESSIVE);   // the status words sit in front of every shape-dependent region
    if (ws_bytes < wp.flags + 4 * sizeof(int32_t)) return fail(GVX_ERR_WORKSPACE, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int32_t h[4] = {0, 0, 0, 0}, tmo = 0;
    int32_t* flags = ws_ptr<int32_t>(ws, wp.flags);
    HIP_TRY(hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, s));
    if (ws_bytes >= wp.sync + HANDOFF_WORDS * sizeof(unsigned))   // (a Postnet-only workspace ends before the hand-off words)
        HIP_TRY(hipMemcpyAsync(&tmo, reinterpret_cast<const char*>(ws) + wp.sync + HANDOFF_TIMEOUT * sizeof(unsigned), sizeof tmo,
                               hipMemcpyDeviceToHost, s));
    // the sticky words accumulate over every call since the last look: reading them clears them
    HIP_TRY(zero_async(flags + FLAG_TOKEN, sizeof(int32_t), s));
    HIP_TRY(zero_async(flags + FLAG_TIMEOUT, sizeof(int32_t), s));
    if (ws_bytes >= wp.sync + HANDOFF_WORDS * sizeof(unsigned))
        HIP_TRY(zero_async(ws_ptr<unsigned>(ws, wp.sync) + HANDOFF_TIMEOUT, sizeof(unsigned), s));
    HIP_TRY(hipStreamSynchronize(s));
    host_out[0] = h[FLAG_TOKEN];
    host_out[1] = h[FLAG_TIMEOUT] ? h[FLAG_TIMEOUT] : tmo;
    return GVX_OK;
}

int gvx_encoder_forward(gvx_model* m, const int64_t* tokens, const int32_t* lengths, int B, int L, float* memory_out,
                        void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(m, B, L, 1, ws, ws_bytes, WS_AUTOREGRESSIVE);   // (the encoder's buffers precede every mode-dependent one)
    if (rc != GVX_OK) return rc;
    if (!tokens || !memory_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const WsPlan wp = make_ws_plan(m, B, L, 1, WS_AUTOREGRESSIVE);
    return encoder_impl(m, tokens, lengths, B, L, memory_out, ws, wp, encoder_wino_scratch(wp, true), (hipStream_t)stream);
}

int gvx_decoder_teacher_forced(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, const float* mel_in, int T,
                               const uint8_t* keep_masks, float* mel_out, float* gate_out, float* align_out, void* ws,
                               size_t ws_bytes, void* stream) {
    int rc = check_common(m, B, L, T, ws, ws_bytes);
    if (rc != GVX_OK) return rc;
    if (!memory || !mel_in || !keep_masks || !mel_out || !gate_out || !align_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const WsPlan wp = make_ws_plan(m, B, L, T);
    rc = decoder_tf_impl(m, memory, lengths, B, L, mel_in, T, keep_masks, mel_out, gate_out, align_out, ws, wp, (hipStream_t)stream);
    if (rc != GVX_OK) return rc;
    float* outs[3] = {mel_out, gate_out, align_out};
    const size_t counts[3] = {(size_t)B * m->d.n_mels * T, (size_t)B * T, (size_t)B * T * L};
    return poison_if_timed_out(m, B, L, ws, wp, outs, counts, 3, (hipStream_t)stream);
}

int gvx_encoder_lstm_forward(gvx_model* m, const float* conv_out, const int32_t* lengths, int B, int L, float* memory_out,
                             float* cell_states_out, float* input_preact_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(m, B, L, 1, ws, ws_bytes, WS_AUTOREGRESSIVE);
    if (rc != GVX_OK) return rc;
    if (!conv_out || !memory_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (cell_states_out) HIP_TRY(zero_async(cell_states_out, (size_t)B * L * m->d.embed_dim * sizeof(float), (hipStream_t)stream));
    const WsPlan wp = make_ws_plan(m, B, L, 1, WS_AUTOREGRESSIVE);   // (conv_out: the folded convolutions do not run, no scratch is touched)
    return encoder_impl(m, nullptr, lengths, B, L, memory_out, ws, wp, encoder_wino_scratch(wp, true), (hipStream_t)stream, conv_out, cell_states_out,
                        input_preact_out);
}

int gvx_decoder_teacher_forced_train(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, const float* mel_in, int T,
                                     const uint8_t* keep_masks, const uint8_t* att_keep, const uint8_t* dec_keep, float p_att, float p_dec,
                                     float* mel_out, float* gate_out, float* align_out, float* att_hidden_all, float* att_cell_all,
                                     float* dec_cell_all, float* dec_hidden_context_all, float* att_preact_all, float* dec_preact_all,
                                     void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(m, B, L, T, ws, ws_bytes);
    if (rc != GVX_OK) return rc;
    if (!memory || !mel_in || !keep_masks || !att_keep || !dec_keep || !mel_out || !gate_out || !align_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!(p_att >= 0.f && p_att < 1.f && p_dec >= 0.f && p_dec < 1.f)) return fail(GVX_ERR_INVALID_ARG, "dropout probabilities must be in [0, 1)");
    // the 64-row loop (GVX_TF_ROWS64=1 handles, 33 .. 64 rows) wires neither the hidden-state dropout nor the tape: refused before
    // anything is written, rather than an inference-mode result behind GVX_OK
    if (plan_teacher_forced(m, B, L, TF_TRAIN_PARTIAL_TAPE).rows64)
        return fail(GVX_ERR_UNSUPPORTED, "training mode with %d rows on a GVX_TF_ROWS64 handle: the 64-row loop has no dropout and no tape (at most 32 rows per call)", B);
    hipStream_t s = (hipStream_t)stream;
    const int A = m->d.att_rnn_dim, D = m->d.dec_rnn_dim, E = m->d.embed_dim;
    const LstmDropout tr{att_keep, dec_keep, 1.f / (1.f - p_att), 1.f / (1.f - p_dec), att_hidden_all, att_cell_all, dec_cell_all, att_preact_all, dec_preact_all};
    if (att_hidden_all) HIP_TRY(zero_async(att_hidden_all, (size_t)B * A * sizeof(float), s));   // slot 0: the initial (zero) states
    if (att_cell_all) HIP_TRY(zero_async(att_cell_all, (size_t)B * A * sizeof(float), s));
    if (dec_cell_all) HIP_TRY(zero_async(dec_cell_all, (size_t)B * D * sizeof(float), s));
    const WsPlan wp = make_ws_plan(m, B, L, T);
    rc = decoder_tf_impl(m, memory, lengths, B, L, mel_in, T, keep_masks, mel_out, gate_out, align_out, ws, wp, s, false, &tr);
    if (rc != GVX_OK) return rc;
    {   // a hand-off of the resident-attention loop that timed out must not look like a result (NaN outputs + sticky status)
        float* outs[3] = {mel_out, gate_out, align_out};
        const size_t counts[3] = {(size_t)B * m->d.n_mels * T, (size_t)B * T, (size_t)B * T * L};
        rc = poison_if_timed_out(m, B, L, ws, wp, outs, counts, 3, s);
        if (rc != GVX_OK) return rc;
    }
    if (dec_hidden_context_all)   // [T+1] slots of blocked [h_d ; ctx] vectors: slot t + 1 = after step t
        HIP_TRY(hipMemcpyAsync(dec_hidden_context_all, ws_ptr<float>(ws, wp.hc), (size_t)(T + 1) * B * (D + E) * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
    return GVX_OK;
}

int gvx_train_export(const gvx_model* m, const void* ws_c, size_t ws_bytes, int B, int L, int T, int what, float* dst, void* stream) {
    void* ws = const_cast<void*>(ws_c);
    if (!m || !ws || !dst) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const WsPlan wp = make_ws_plan(m, B, L, T);
    if (ws_bytes < wp.total) return fail(GVX_ERR_WORKSPACE, "workspace too small");
    const gvx_dims& d = m->d;
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)(T + 1) * B;
    switch (what) {
        case 0: HIP_TRY(hipMemcpyAsync(dst, ws_ptr<float>(ws, wp.frames), rows * d.n_mels * sizeof(float), hipMemcpyDeviceToDevice, s)); break;
        case 1: HIP_TRY(hipMemcpyAsync(dst, ws_ptr<float>(ws, wp.pre1), rows * d.prenet_dim * sizeof(float), hipMemcpyDeviceToDevice, s)); break;
        case 2: return gvx_train_unblock(ws_ptr<float>(ws, wp.prenet), dst, T + 1, B, d.prenet_dim, stream);
        case 3: HIP_TRY(hipMemcpyAsync(dst, ws_ptr<float>(ws, wp.pm), (size_t)B * L * d.att_dim * sizeof(float), hipMemcpyDeviceToDevice, s)); break;
        case 4: HIP_TRY(hipMemcpyAsync(dst, ws_ptr<float>(ws, wp.memory), (size_t)B * L * d.embed_dim * sizeof(float), hipMemcpyDeviceToDevice, s)); break;
        default: return fail(GVX_ERR_INVALID_ARG, "gvx_train_export: unknown buffer %d", what);
    }
    return GVX_OK;
}

size_t gvx_postnet_workspace_bytes(const gvx_model* m, int B, int T) {
    if (!m || B < 1 || T < 1) return 0;
    return make_postnet_plan(m, B, T).total;
}

int gvx_postnet_forward(gvx_model* m, const float* mel_in, const int32_t* mel_lengths, int B, int T, float* mel_post_out, void* ws,
                        size_t ws_bytes, void* stream) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null model");
    if (!m->dev_blob) return fail(GVX_ERR_STATE, "weights not bound (call gvx_model_bind_blob)");
    if (B < 1 || T < 1) return fail(GVX_ERR_INVALID_ARG, "B and T must be >= 1");
    if ((long)B * T > (1L << 30)) return fail(GVX_ERR_UNSUPPORTED, "B * T = %ld frames exceed the GEMM row index range", (long)B * T);
    if (!ws) return fail(GVX_ERR_WORKSPACE, "null workspace");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(GVX_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    const PostnetPlan pp = make_postnet_plan(m, B, T);
    if (ws_bytes < pp.total) return fail(GVX_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, pp.total);
    if (!mel_in || !mel_post_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    return postnet_impl(m, mel_in, mel_lengths, B, T, mel_post_out, ws_ptr<float>(ws, pp.ya), ws_ptr<float>(ws, pp.yb), ws_ptr<float>(ws, pp.wino), pp.wino_floats,
                        (hipStream_t)stream);
}

int gvx_mask_padding(float* mel, float* mel_post, float* gate, const int32_t* mel_lengths, int B, int n_mels, int T, void* stream) {
    if (!mel_lengths || B < 1 || T < 1 || n_mels < 1) return fail(GVX_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(launch_mask_padding(mel, mel_post, gate, mel_lengths, B, n_mels, T, (hipStream_t)stream));
    return GVX_OK;
}

int gvx_tacotron2_forward(gvx_model* m, const int64_t* tokens, const int32_t* token_lengths, int B, int L, const float* mel_in,
                          const int32_t* mel_lengths, int T, const uint8_t* keep_masks, float* mel_out, float* mel_post_out,
                          float* gate_out, float* align_out, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_common(m, B, L, T, ws, ws_bytes);
    if (rc != GVX_OK) return rc;
    if (!tokens || !mel_in || !keep_masks || !mel_out || !gate_out || !align_out)   // (mel_post_out may be null: no Postnet, no padding mask)
        return fail(GVX_ERR_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const WsPlan wp = make_ws_plan(m, B, L, T);
    const bool timed = m->timing && m->ev_valid;
    float* memory = ws_ptr<float>(ws, wp.memory);
    if (timed) HIP_TRY(hipEventRecord(m->ev[0], s));
    // The Prenet part of the decoder needs the mel input only.  On the persistent-attention path (which owns a high-priority
    // side stream) the ENCODER runs on that stream - its BiLSTM recurrence is 128 small latency-bound launches that leave the
    // chip idle, and at the higher priority they are dispatched ahead of the GEMM workgroups - while the Prenet GEMMs fill
    // the chip from the caller's stream (the other way round the encoder took 2.0 instead of 1.4 ms).
    const bool overlap = plan_teacher_forced(m, B, L, TF_INFERENCE).side_stream;
    if (overlap) {
        rc = ensure_side_stream(m);
        if (rc != GVX_OK) return rc;
        HIP_TRY(hipEventRecord(m->pa_fork, s));
        HIP_TRY(hipStreamWaitEvent(m->pa_stream, m->pa_fork, 0));
        // The Prenet products start behind the SECOND encoder convolution (enc_fork_after): side by side from the start the two sets
        // of GEMMs slow each other and leave the second half of the recurrence - a quarter of the chip, latency bound - alone on
        // an idle GPU; behind all three convolutions the `pre_gate` GEMM outlasts the recurrence.  Encoder stage for the fork behind
        // 3 / 2 / 1 / 0 convolutions, 32 x 800 frames: 1.016 / 1.007 / 1.033 / 1.114 ms with the convolutions as Winograd F(4,5)
        // (medians of three runs, EXPERIMENTS.md; with direct convolutions it was 1.14 / 1.13 / 1.15 / 1.22, and 1 the default)
        rc = encoder_impl(m, tokens, token_lengths, B, L, memory, ws, wp, encoder_wino_scratch(wp, false), m->pa_stream, nullptr, nullptr, nullptr, m->enc_mid);
        if (rc != GVX_OK) return rc;
        // the decoder's zero states and the memory projection (needs the encoder output) right behind the encoder on its stream:
        // they end under the tail of the Prenet products instead of between the join and the first step (~60 us)
        rc = decoder_init_states(m, memory, B, L, decoder_buffers(ws, wp), m->pa_stream);
        if (rc != GVX_OK) return rc;
        HIP_TRY(hipEventRecord(m->pa_join, m->pa_stream));
        HIP_TRY(hipStreamWaitEvent(s, m->enc_mid, 0));
        rc = decoder_prenet_part(m, B, L, mel_in, T, keep_masks, ws, wp, s);
        if (rc != GVX_OK) return rc;
        HIP_TRY(hipStreamWaitEvent(s, m->pa_join, 0));
    } else {
        rc = encoder_impl(m, tokens, token_lengths, B, L, memory, ws, wp, encoder_wino_scratch(wp, false), s);
        if (rc != GVX_OK) return rc;
    }
    if (timed) HIP_TRY(hipEventRecord(m->ev[1], s));
    rc = decoder_tf_impl(m, memory, token_lengths, B, L, mel_in, T, keep_masks, mel_out, gate_out, align_out, ws, wp, s, overlap);
    if (rc != GVX_OK) return rc;
    if (timed) HIP_TRY(hipEventRecord(m->ev[4], s));
    // (mel_post_out == nullptr: the caller runs the Postnet and the padding mask itself - over all chunks of a larger batch in
    // one call, whose GEMMs fill the chip better than a chunk's; a timed-out call's NaN in mel_out reaches them through the Postnet)
    if (mel_post_out) {
        rc = postnet_impl(m, mel_out, nullptr, B, T, mel_post_out, ws_ptr<float>(ws, wp.ya), ws_ptr<float>(ws, wp.yb), ws_ptr<float>(ws, wp.xa),
                          (wp.ya - wp.xa) / sizeof(float), s);
        if (rc != GVX_OK) return rc;
        if (mel_lengths) HIP_TRY(launch_mask_padding(mel_out, mel_post_out, gate_out, mel_lengths, B, m->d.n_mels, T, s));
    }
    float* outs[4] = {mel_out, gate_out, align_out, mel_post_out};
    const size_t nm = (size_t)B * m->d.n_mels * T;
    const size_t counts[4] = {nm, (size_t)B * T, (size_t)B * T * L, nm};
    rc = poison_if_timed_out(m, B, L, ws, wp, outs, counts, mel_post_out ? 4 : 3, s);
    if (rc != GVX_OK) return rc;
    if (timed) HIP_TRY(hipEventRecord(m->ev[5], s));
    return GVX_OK;
}

int gvx_tacotron2_loss(const float* mel_out, const float* mel_post_out, const float* gate_out, const float* mel_target,
                       const float* gate_target, int B, int n_mels, int T, float* loss_out, void* scratch, size_t scratch_bytes,
                       void* stream) {
    if (!mel_out || !mel_post_out || !gate_out || !mel_target || !gate_target || !loss_out || !scratch)
        return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || n_mels < 1 || T < 1) return fail(GVX_ERR_INVALID_ARG, "B, n_mels and T must be >= 1");
    if (scratch_bytes < loss_scratch_bytes() || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return fail(GVX_ERR_WORKSPACE, "scratch too small (%zu bytes needed) or not 8-byte aligned", loss_scratch_bytes());
    HIP_TRY(launch_tacotron2_loss(mel_out, mel_post_out, gate_out, mel_target, gate_target, (long)B * n_mels * T, (long)B * T,
                                  reinterpret_cast<double*>(scratch), loss_out, (hipStream_t)stream));
    return GVX_OK;
}

int gvx_prenet_masks_generate(uint8_t* masks_out, size_t n, uint64_t seed, void* stream) {
    if (!masks_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    HIP_TRY(launch_mask_gen(masks_out, n, seed, (hipStream_t)stream));
    return GVX_OK;
}

int gvx_stage_timing_enable(gvx_model* m, int enable) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null model");
    if (enable && !m->ev_valid) {
        for (auto& e : m->ev) HIP_TRY(hipEventCreate(&e));
        m->ev_valid = true;
    }
    m->timing = enable != 0;
    return GVX_OK;
}

int gvx_kernel_timing_enable(gvx_model* m, int enable) {
    if (!m) return fail(GVX_ERR_INVALID_ARG, "null model");
    m->ktiming = enable != 0;
    return GVX_OK;
}

int gvx_kernel_times_ms(gvx_model* m, float* lstm_avg_ms, float* attn_avg_ms, int* n_steps) {
    if (!m || !lstm_avg_ms || !attn_avg_ms) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (m->n_lstm_ev < 1) return fail(GVX_ERR_STATE, "no timed decoder loop has run");
    HIP_TRY(hipEventSynchronize(m->kev[2]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, m->kev[0], m->kev[1]));
    HIP_TRY(hipEventElapsedTime(&b, m->kev[1], m->kev[2]));
    *lstm_avg_ms = a / m->n_lstm_ev;
    *attn_avg_ms = m->n_attn_ev > 0 ? b / m->n_attn_ev : 0.f;   // 0: the attention ran as one kernel beside the loop
    if (n_steps) *n_steps = m->n_lstm_ev;
    return GVX_OK;
}

int gvx_stage_times_ms(gvx_model* m, float* t5, int* launches) {
    if (!m || !t5) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!m->ev_valid) return fail(GVX_ERR_STATE, "stage timing was not enabled");
    HIP_TRY(hipEventSynchronize(m->ev[5]));
    // ev: 0 start, 1 encoder done, 2 prenet+init done, 3 decoder loop done, 4 projection done, 5 postnet done
    for (int i = 0; i < 5; ++i) HIP_TRY(hipEventElapsedTime(&t5[i], m->ev[i], m->ev[i + 1]));
    if (launches) *launches = m->last_decoder_launches;
    return GVX_OK;
}
#ifdef GVX_STAMPS
int gvx_debug_read_stamps_skinny(unsigned long long* host96) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_stamps_skinny(host96));
    return GVX_OK;
}
int gvx_debug_read_stamps_persist(unsigned long long* host96) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_stamps_persist(host96));
    return GVX_OK;
}
int gvx_debug_read_wg_spans(unsigned long long* host1024) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_wg_spans(host1024));
    return GVX_OK;
}
int gvx_debug_read_stamps_resident(unsigned long long* host480) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_stamps_resident(host480));
    return GVX_OK;
}
int gvx_debug_read_wg_stamps_resident(unsigned long long* host896, unsigned long long* rows512) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_wg_stamps_resident(host896));
    HIP_TRY(gvx::read_row_stamps_persist(rows512));
    return GVX_OK;
}
int gvx_debug_read_loc_stamps(unsigned long long* host32) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_loc_stamps_persist(host32));
    return GVX_OK;
}
int gvx_debug_read_stamps_ar(unsigned long long* host896, unsigned long long* rows256) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(gvx::read_wg_stamps_resident_ar(host896));
    HIP_TRY(gvx::read_row_stamps_persist_ar(rows256));
    return GVX_OK;
}
int gvx_debug_read_stamps(unsigned long long* host96) {
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long tmp[96];
    HIP_TRY(gvx::read_stamps_skinny(host96));       // row 0 is the LSTM kernel's
    HIP_TRY(gvx::read_stamps_attention(tmp));        // rows 1, 2 are the attention kernels'
    for (int i = 32; i < 96; ++i) host96[i] = tmp[i];
    return GVX_OK;
}
#endif

}  // extern "C"
