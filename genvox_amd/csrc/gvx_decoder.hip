// The two decoder loops of the C-ABI layer: how a shape runs (plan_teacher_forced / plan_autoregressive), the argument blocks of
// the step launches and the resident kernels, and one function per loop kind.  Workspace layout: gvx_api.hip.
#include "gvx_internal.h"

using namespace gvx;

namespace gvx {

namespace {
// the resident attention kernel (attn_persist.hip) serves this shape and the handle's layer sizes
bool resident_attention_serves(const gvx_model* m, int B, int L) {
    const gvx_dims& d = m->d;
    return attention_persistent_supported(B, L, d.att_dim, d.att_loc_filters, d.att_loc_kernel, d.embed_dim, d.att_rnn_dim, d.dec_rnn_dim);
}
}  // namespace

TfLoopPlan plan_teacher_forced(const gvx_model* m, int B, int L, TfMode mode) {
    TfLoopPlan p{};
    const bool train = mode != TF_INFERENCE;
    // Persistent attention (attn_persist.hip): the loop is then T + 1 LSTM launches and ONE attention kernel on a forked stream;
    // the LSTM tiles stream the k-groups of the context last and wait for it in the launch.  33 .. 64 rows only on request.
    const bool pa_shape = (B <= 32 || m->tf_rows64) && m->attn_persistent && m->attn_one_launch && resident_attention_serves(m, B, L);
    const bool pa = pa_shape && (!train || m->train_resident);
    p.pa_layout = attention_persistent_layout(B, L);
    // ... and the LSTM launches as ONE resident kernel too (dec_resident.hip): inference mode, one batch tile, L <= 256
    // (training mode: the same kernel with the tape in its cell epilogues, when the caller asks for the whole tape)
    const bool resident = pa && (p.pa_layout == 1 || p.pa_layout == 2) && m->tf_resident &&
                          (!train || (m->train_resident_loop && mode == TF_TRAIN_WHOLE_TAPE)) && decoder_resident_supported(B, L);
    p.kind = resident ? 2 : (pa ? 1 : 0);
    // the resident tile kernel's deal: 224 workgroups beside <= 32 attention workgroups - rows of 129-256 tokens take two each, so
    // up to 16 such rows keep the 224-workgroup deal (its 48-row workgroups are lighter than the pairs of the 192-workgroup one:
    // 15.4 vs 17.3 us per step at 16 x L = 190; not at B <= 2, where the products run on the vector ALUs and the 64 slabs of the
    // 192-workgroup deal win: 13.9 vs 14.2)
    p.tile_layout = resident && p.pa_layout == 2 && B > 2 && B <= 16 && m->tf_long_rows_224 ? 1 : p.pa_layout;
    p.rows64 = p.kind == 1 && p.pa_layout == 3;
    p.pre_gate = p.timeout_check = pa_shape;
    p.side_stream = p.kind != 0;
    // (the training tape is written through per-call pointers: only the 64-row launches, which carry none, are replayed in that mode)
    p.graph = m->use_graph && !m->ktiming && p.kind != 2 && (p.rows64 || !train);
    return p;
}

ArLoopPlan plan_autoregressive(const gvx_model* m, int B, int L, bool windowed) {
    ArLoopPlan p{};
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, D = d.dec_rnn_dim, lay = attention_persistent_layout(B, L);
    // Resident attention (attn_persist.hip) when the shape allows it: ONE attention kernel lives beside the step launches for
    // the whole decode, the context of a step arrives inside launch C (deferred segment) and the attention launch leaves the
    // step's chain.
    const bool pa_any = m->attn_one_launch && resident_attention_serves(m, B, L);
    // ... and when the layer sizes are the default ones, the LSTM cells, the projection and the Prenet live in a second resident
    // kernel as well (dec_resident.hip, decoder_ar_resident_kernel): the whole decode is two launches.  Not on handles that share
    // the chip with other calls (gvx_model_set_persistent_attention(model, 0): the two kernels need all 256 CUs)
    // (rows of 129-256 tokens take two attention workgroups each: 16 rows of them fit beside the 224 workgroups of the tile kernel)
    const bool pair = pa_any && B <= 32 && E / 4 == D / 8 && m->attn_persistent && m->tf_resident && m->ar_resident_loop &&
                      decoder_resident_supported(B, L) && (lay == 1 || (lay == 2 && B <= 16)) && d.prenet_dim == 256 && d.n_mels <= 80 &&
                      m->PSB() <= 96 && d.att_dim == 128;
    p.kind = pair ? 2 : (pa_any && lay == 1 && m->ar_resident ? 1 : 0);
    // A monotonic attention window lives in the resident pair's one-workgroup-per-row attention kernel and in the attention step of the
    // launches per step: rows of 129-256 tokens (two workgroups per row) and the step launches beside the resident attention kernel go
    // to kind 0 when the call carries one
    if (windowed && !(p.kind == 2 && lay == 1)) p.kind = 0;
    // The projection's context columns ride on the decoder-LSTM tiles' projection slabs, so that launch C is exactly 256 tiles.
    p.fold = B <= 32 && E / 4 == D / 8;
    // h_a(t) exists when launch A ends, the context only after the attention step: the h_a columns of both cells (two thirds of
    // what launch C used to stream) are summed by tiles that share the attention step's launch - the step's latency chain
    // hides under 33 MB of weight stream - and launch C is left with the context columns
    // (not on handles that share the chip with other calls - gvx_model_set_persistent_attention(model, 0), the lanes of a
    // batch above 32 rows: two such launches of 512 workgroups each queue behind one another, measured 66 vs 61 us per step)
    p.split_h = p.kind == 0 && m->ar_split_h && m->attn_persistent && m->attn_one_launch && B <= 32 && d.att_dim > 32 && d.att_dim <= 128;
    p.graph = m->use_graph && p.kind != 2;
    return p;
}

DecoderBuffers decoder_buffers(void* ws, const WsPlan& wp) {
    DecoderBuffers b;
    b.pm = ws_ptr<float>(ws, wp.pm); b.frames = ws_ptr<float>(ws, wp.frames); b.pre1 = ws_ptr<float>(ws, wp.pre1);
    b.prenet = ws_ptr<float>(ws, wp.prenet); b.h_a = ws_ptr<float>(ws, wp.h_a); b.c_a = ws_ptr<float>(ws, wp.c_a);
    b.c_d = ws_ptr<float>(ws, wp.c_d); b.hc = ws_ptr<float>(ws, wp.hc); b.w_cum = ws_ptr<float>(ws, wp.w_cum);
    b.q_slab = ws_ptr<float>(ws, wp.q_slab); b.proj = ws_ptr<float>(ws, wp.proj); b.energies = ws_ptr<float>(ws, wp.energies);
    b.align_tm = ws_ptr<float>(ws, wp.align_tm); b.len_copy = ws_ptr<int32_t>(ws, wp.len_copy);
    b.loc = ws_ptr<float>(ws, wp.loc);
    b.p_slab = ws_ptr<float>(ws, wp.p_slab); b.p_ctx = ws_ptr<float>(ws, wp.p_ctx);
    b.att_part = ws_ptr<float>(ws, wp.att_part); b.dec_part = ws_ptr<float>(ws, wp.dec_part);
    b.pre_gate = ws_ptr<float>(ws, wp.pre_gate);
    return b;
}

// Decoder.initialize_decoder_states (models/tts/tacotron2.py:303-315): zero states + memory projection
int decoder_init_states(gvx_model* m, const float* memory, int B, int L, const DecoderBuffers& db, hipStream_t s) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    void* const zp[5] = {db.h_a, db.c_a, db.c_d, db.hc /* slot 0 */, db.w_cum};
    const size_t zb[5] = {(size_t)RS_HA_SLOTS * B * A * sizeof(float), (size_t)B * A * sizeof(float), (size_t)B * D * sizeof(float),
                          (size_t)B * (D + E) * sizeof(float), (size_t)B * L * sizeof(float)};
    HIP_TRY(launch_zero_many(zp, zb, 5, s));
    GemmParams g{};
    g.A = memory; g.amap = RowMap{B * L, 0, (long)E};
    g.W = m->dev_blob + m->blob.wmem; g.ldw = E;
    g.C = db.pm; g.cmap = RowMap{B * L, 0, (long)d.att_dim};
    g.M = B * L; g.N = d.att_dim; g.K = E; g.act = ACT_NONE;
    HIP_TRY(launch_gemm(g, s));
    return GVX_OK;
}

namespace {

// attention LSTM of step t: x = [prenet(t) ; ctx(t-1) ; h_a(t-1)] (all blocked vectors)
void fill_att_job(const gvx_model* m, SkinnyJob& J, const float* prenet_t, int t, int B, const DecoderBuffers& db) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    std::memset(&J, 0, sizeof J);
    const float* hc_t = db.hc + (size_t)t * B * (D + E);
    J.Wp = m->dev_blob + m->blob.att_frag; J.bias = m->dev_blob + m->blob.att_bias;
    J.x[0] = XSeg{prenet_t, P};
    J.x[1] = XSeg{hc_t + (size_t)D * B, E};                   // context part of slot t: k-groups D/8 ...
    J.x[2] = XSeg{db.h_a + (size_t)(t & 1) * B * A, A};       // h_a of step t-1
    J.N = 4 * A; J.nkg = (P + E + A) / 8; J.mode = 0; J.B = B;
    J.c = db.c_a;
    J.h_out = db.h_a + (size_t)((t + 1) & 1) * B * A;
    J.Wq_t = m->dev_blob + m->blob.wq_t; J.q_slab = db.q_slab; J.att_dim = d.att_dim;
}

// decoder LSTM of step t: x = [h_a(t) ; ctx(t) ; h_d(t-1)], writes h_d(t) into hc slot t+1
void fill_dec_job(const gvx_model* m, SkinnyJob& J, int t, int B, const DecoderBuffers& db) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    std::memset(&J, 0, sizeof J);
    const float* hc_t = db.hc + (size_t)t * B * (D + E);
    float* hc_n = db.hc + (size_t)(t + 1) * B * (D + E);
    J.Wp = m->dev_blob + m->blob.dec_frag; J.bias = m->dev_blob + m->blob.dec_bias;
    J.x[0] = XSeg{db.h_a + (size_t)((t + 1) & 1) * B * A, A};
    J.x[1] = XSeg{hc_n + (size_t)D * B, E};
    J.x[2] = XSeg{hc_t, D};
    J.N = 4 * D; J.nkg = (A + E + D) / 8; J.mode = 0; J.B = B;
    J.c = db.c_d;
    J.h_out = hc_n;
}

// location features for step t's attention, computed inside the LSTM launch of step t from attention(t-1)'s outputs
void fill_loc(const gvx_model* m, LocJob& q, int t, int B, int L, const float* align_base, long align_bs, long align_ts,
              const DecoderBuffers& db) {
    const gvx_dims& d = m->d;
    q.w_prev = t > 0 ? align_base + (size_t)(t - 1) * align_ts : nullptr; q.w_prev_bs = align_bs;
    q.w_cum = db.w_cum;
    q.loc_conv_t = m->dev_blob + m->blob.loc_conv; q.loc_dense_t = m->dev_blob + m->blob.loc_dense;
    q.loc_out = db.loc;
    q.pm = m->attn_one_launch ? db.pm : nullptr;
    q.B = B; q.L = L; q.a = d.att_dim; q.kl = d.att_loc_kernel; q.G = attention_groups(B, L);
}

void fill_attn(const gvx_model* m, AttnParams& p, const float* memory, const int32_t* lengths, int t, int B, int L,
               float* align_out, long align_bs, long align_ts, const DecoderBuffers& db) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, D = d.dec_rnn_dim;
    std::memset(&p, 0, sizeof p);
    p.q_slab = db.q_slab; p.n_slabs = d.att_rnn_dim / 8;
    p.w_cum = db.w_cum;
    p.loc = db.loc; p.v = m->dev_blob + m->blob.v;
    p.pm = db.pm; p.memory = memory; p.lengths = lengths;
    p.w_out = align_out + (size_t)t * align_ts; p.w_out_bs = align_bs;
    p.ctx_out = db.hc + (size_t)(t + 1) * B * (D + E) + (size_t)D * B;
    p.energies = db.energies;
    p.B = B; p.L = L; p.a = d.att_dim; p.F = d.att_loc_filters; p.kl = d.att_loc_kernel; p.E = E;
    p.G = m->attn_one_launch ? attention_slices(B, E) : attention_groups(B, L);
}

hipError_t launch_attn(const gvx_model* m, const AttnParams& p, hipStream_t s) {
    return m->attn_one_launch ? launch_attention_step(p, s) : launch_attention(p, s);
}

// Side stream of the resident attention kernels: ONE per device, shared by every handle of the process (GVX_SIDE_POOL=2: two,
// dealt round-robin per call, for concurrent resident loops - the opt-in autoregressive lanes).
// Highest priority: HIP keeps separate hardware queues per priority, so this stream can never be dealt the queue of a
// (normal-priority) stream an LSTM chain runs on - the attention kernel would then sit in front of the launches it waits
// for until its spin limit (observed in a process that had created a dozen streams before).  Shared instead of one per
// handle because a process has only ~4 hardware queues, dealt in order of first use: with the null stream and the host
// mirror's two lane streams in use, a second side stream landed on the queue of a stream that feeds it and every other
// forward took 17 instead of 6.7 ms (tools/queue_probe.py, round 3).  Calls that share the stream only serialise their
// resident kernels (the later one starts when the earlier loop has ended, well inside the spin limit).
struct SidePool { hipStream_t s[2] = {nullptr, nullptr}; unsigned next = 0; };
std::mutex g_pool_mutex;
std::unordered_map<int, SidePool> g_side_pools;

// Resident loops take turns on a device.  A loop whose kernels wait for each other (the resident attention kernel beside LSTM
// launches, or beside the resident decoder kernel: 32 + 224 workgroups that must ALL be on the chip) cannot share the chip with a
// second one: dispatched at the same time from two streams, each could get half of its workgroups a CU and both would spin
// until their limits.  So every such loop is enqueued under this mutex, behind an event the previous one recorded at its join -
// ordering on the device, no host wait - and its kernels reach the shared side stream in turn order.
struct ResidentTurn { hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; unsigned n = 0; };
std::mutex g_turn_mutex;
std::unordered_map<int, ResidentTurn> g_turns;

int turn_begin(hipStream_t s) {   // caller holds g_turn_mutex
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    ResidentTurn& t = g_turns[dev];
    if (!t.ev[0])
        for (auto& e : t.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (t.n > 0) HIP_TRY(hipStreamWaitEvent(s, t.ev[(t.n - 1) & 3], 0));
    return GVX_OK;
}
int turn_end(hipStream_t s) {     // caller holds g_turn_mutex
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    ResidentTurn& t = g_turns[dev];
    HIP_TRY(hipEventRecord(t.ev[t.n & 3], s));
    ++t.n;
    return GVX_OK;
}

}  // namespace

int ensure_side_stream(gvx_model* m) {
    if (!m->pa_fork) {
        HIP_TRY(hipEventCreateWithFlags(&m->pa_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->pa_join, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m->enc_mid, hipEventDisableTiming));
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    SidePool& pool = g_side_pools[dev];
    if (!pool.s[0]) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        for (auto& st : pool.s) HIP_TRY(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest));
    }
    m->pa_stream = pool.s[pool.next++ % m->side_pool];
    return GVX_OK;
}

namespace {

// ---- argument blocks of the resident kernels: what every role shares is filled here, once
AttnPersistParams fill_attn_persist(const gvx_model* m, const DecoderBuffers& db, const float* memory, const int32_t* len_ws,
                                    unsigned* sync, int B, int L, int T) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, D = d.dec_rnn_dim;
    AttnPersistParams pp{};
    pp.q_slab = db.q_slab;
    pp.v = m->dev_blob + m->blob.v; pp.pm = db.pm; pp.memory = memory; pp.lengths = len_ws;
    pp.loc_conv_t = m->dev_blob + m->blob.loc_conv; pp.loc_dense_t = m->dev_blob + m->blob.loc_dense;
    pp.w_out = db.align_tm; pp.w_out_bs = (long)L; pp.w_out_ts = (long)B * L;
    pp.ctx_base = db.hc + (size_t)B * (D + E) + (size_t)D * B; pp.ctx_ts = (long)B * (D + E);   // slot t + 1
    pp.sync = sync; pp.B = B; pp.L = L; pp.T = T; pp.kl = d.att_loc_kernel;
    pp.spin_limit = m->spin_limit;
    return pp;
}
// beside a resident tile kernel: flags per producer instead of the two counters (row b polls replica b % RS_REP1: attn_persist.hip)
void use_resident_flags(const gvx_model* m, AttnPersistParams& pp) {
    pp.q_flags = pp.sync + RS_FLAG_Q; pp.n_q_flags = pp.n_slabs;
    pp.ctx_flags = pp.sync + RS_FLAG_CTX;
    pp.debug = m->rs_debug;
}

// The resident kernel is launched eagerly on the handle's side stream, ordered behind everything already queued on `s`;
// only the LSTM chain is replayed from a graph (a graph that contains both may run its branches one after the other -
// observed: the attention node first, waiting for slabs of launches queued behind it until its spin limit)
int launch_resident_attention(gvx_model* m, const AttnPersistParams& pp, hipStream_t s) {
    HIP_TRY(hipEventRecord(m->pa_fork, s));
    HIP_TRY(hipStreamWaitEvent(m->pa_stream, m->pa_fork, 0));
    if (!m->debug_skip_resident) HIP_TRY(launch_attention_persistent(pp, m->pa_stream));
    HIP_TRY(hipEventRecord(m->pa_join, m->pa_stream));
    return GVX_OK;
}

// weights, state buffers and hand-off words that DecResidentParams and ArResidentParams have in common
template <class P>
void fill_resident_common(const gvx_model* m, const DecoderBuffers& db, unsigned* sync, int B, int T, P& rp) {
    const gvx_dims& d = m->d;
    rp.att_frag = m->dev_blob + m->blob.att_frag; rp.att_bias = m->dev_blob + m->blob.att_bias; rp.wq_t = m->dev_blob + m->blob.wq_t;
    rp.dec_frag = m->dev_blob + m->blob.dec_frag; rp.dec_bias = m->dev_blob + m->blob.dec_bias;
    rp.h_a = db.h_a; rp.hc = db.hc; rp.q_slab = db.q_slab; rp.c_a = db.c_a; rp.c_d = db.c_d;
    rp.sync = sync;
    rp.att_frag_bytes = (unsigned)(frag_floats(4 * d.att_rnn_dim, d.prenet_dim + d.embed_dim + d.att_rnn_dim) * sizeof(float));
    rp.B = B; rp.T = T; rp.spin_limit = m->spin_limit; rp.debug = m->rs_debug;
}

int ensure_ar_host_slots(gvx_model* m) {
    if (m->ar_done_host) return GVX_OK;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&m->ar_done_host), 2 * sizeof(int32_t), hipHostMallocDefault));
    for (auto& e : m->ar_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return GVX_OK;
}

}  // namespace

// Prenet over all T+1 frames at once (models/tts/tacotron2.py:370-373) and, for the persistent-attention loop, the Prenet
// columns of the attention LSTM applied to all steps.  Depends on the mel input and the weights only: the fused forward runs
// it on the side stream while the encoder's (latency-bound) recurrence has the chip to itself.
int decoder_prenet_part(gvx_model* m, int B, int L, const float* mel_in, int T, const uint8_t* keep_masks, void* ws, const WsPlan& wp,
                        hipStream_t s) {
    const gvx_dims& d = m->d;
    const int M = d.n_mels, P = d.prenet_dim;
    const DecoderBuffers db = decoder_buffers(ws, wp);
    HIP_TRY(zero_async(db.frames, (size_t)B * M * sizeof(float), s));  // go-frame
    HIP_TRY(launch_frames_from_mel(mel_in, db.frames, B, M, T, s));
    const int rows = (T + 1) * B;
    GemmParams g{};
    g.A = db.frames; g.amap = RowMap{rows, 0, (long)M};
    g.W = m->dev_blob + m->blob.pre_w0; g.ldw = M;
    g.C = db.pre1; g.cmap = RowMap{rows, 0, (long)P};
    g.keep = keep_masks; g.keep_ld = P;
    g.M = rows; g.N = P; g.K = M; g.act = ACT_RELU;
    HIP_TRY(launch_gemm(g, s));
    g.A = db.pre1; g.amap = RowMap{rows, 0, (long)P};
    g.W = m->dev_blob + m->blob.pre_w1; g.ldw = P;
    g.C = db.prenet; g.cmap = RowMap{B, (long)B * P, 8}; g.c_nblk = (long)B * 8;  // step t: blocked [P/8][B][8]
    g.keep = keep_masks + (size_t)rows * P;
    g.K = P;
    HIP_TRY(launch_gemm(g, s));
    if (plan_teacher_forced(m, B, L, TF_INFERENCE).pre_gate) {   // pre_gate[t][b][:] = W_ih[:, :P] prenet(t)[b]  for all T steps: 4A x P weights read once
        GemmParams h{};
        h.A = db.prenet; h.amap = RowMap{B, (long)B * P, 8}; h.a_kblk = (long)B * 8;
        h.W = m->dev_blob + m->blob.att_wpre; h.ldw = P;
        h.C = db.pre_gate; h.cmap = RowMap{T * B, 0, (long)4 * d.att_rnn_dim};
        h.M = T * B; h.N = 4 * d.att_rnn_dim; h.K = P; h.act = ACT_NONE;
        HIP_TRY(launch_gemm(h, s));
    }
    return GVX_OK;
}

// A hand-off time-out of the resident-attention loop must not return numbers that look like results: the call's last
// launch writes NaN over every output and raises the workspace's sticky status word when the time-out word is set
// (no host synchronisation; a no-op of one word read per workgroup otherwise).  gvx_workspace_status reports it.
int poison_if_timed_out(const gvx_model* m, int B, int L, void* ws, const WsPlan& wp, float* const* outs, const size_t* counts, int n,
                        hipStream_t s) {
    if (!plan_teacher_forced(m, B, L, TF_INFERENCE).timeout_check) return GVX_OK;   // no in-launch hand-off on the other paths
    HIP_TRY(launch_poison_on_timeout(ws_ptr<unsigned>(ws, wp.sync) + HANDOFF_TIMEOUT, ws_ptr<int>(ws, wp.flags) + FLAG_TIMEOUT, outs, counts, n, s));
    return GVX_OK;
}

// ===================================================================================================== teacher-forced loop
namespace {

struct TfLoop {   // one teacher-forced call: what its loop kinds share
    gvx_model* m; TfLoopPlan plan; DecoderBuffers db;
    const float* memory; const int32_t* len_ws; void* ws; unsigned* sync; float* xchg;
    int B, L, T;
    const LstmDropout* train;
};

// A job whose x[1] is the context of step t_ctx, in a loop beside the resident attention kernel: the context arrives in-launch
void defer_context(const TfLoop& c, SkinnyJob& J, int t_ctx, bool first) {
    if (c.plan.kind == 0) return;      // (the deferred k order costs the launch ~0.9 us: only where the context arrives in-launch)
    const gvx_dims& d = c.m->d;
    J.defer_seg = 1;
    if (J.q_slab) {
        // attention LSTM: its Prenet columns were applied to all steps by one GEMM before the loop (pre_gate); the job
        // streams the k-groups of [context ; h_a] only and takes the rest as an addend (step t_ctx + 1)
        const int P = d.prenet_dim, E = d.embed_dim, A = d.att_rnn_dim;
        J.x[0] = XSeg{J.x[1].p, 0};
        J.kg0 = P / 8; J.nkg_w = (P + E + A) / 8; J.nkg = (E + A) / 8;
        J.addend = c.db.pre_gate + (size_t)(t_ctx + 1) * c.B * 4 * A; J.add_bs = 4 * A;
    }
    J.tmo = c.sync + HANDOFF_TIMEOUT;
    J.spin_limit = c.m->spin_limit;
    if (t_ctx >= 0) { J.ctx_cnt = c.sync + HANDOFF_CNT_CTX; J.ctx_target = (unsigned)c.B * (unsigned)(t_ctx + 1); }
    J.start_cnt = c.sync + HANDOFF_CNT_Q;   // every launch of the loop (and the drain launch) announces its start
    if (first) { J.ready_cnt = c.sync + HANDOFF_READY; J.ready_target = (unsigned)attention_persistent_workgroups(c.B, c.L); }
}

// training mode: dropout masks and tape slots of the attention LSTM of step t (att) and the decoder LSTM of step t - 1 (dec)
void wire_tape(const LstmDropout& tr, SkinnyJob* att, SkinnyJob* dec, int t, size_t BA, size_t BD) {
    if (att) {
        att->h_keep = tr.att_keep + (size_t)t * BA; att->h_scale = tr.att_scale;
        if (tr.h_a_all) { att->x[2].p = tr.h_a_all + (size_t)t * BA; att->h_out = tr.h_a_all + (size_t)(t + 1) * BA; }
        if (tr.c_a_all) { att->c = tr.c_a_all + (size_t)t * BA; att->c_out = tr.c_a_all + (size_t)(t + 1) * BA; }
        if (tr.pre_a_all) att->pre_out = tr.pre_a_all + (size_t)t * 4 * BA;
    }
    if (dec) {
        if (tr.pre_d_all) dec->pre_out = tr.pre_d_all + (size_t)(t - 1) * 4 * BD;
        dec->h_keep = tr.dec_keep + (size_t)(t - 1) * BD; dec->h_scale = tr.dec_scale;
        if (tr.h_a_all) dec->x[0].p = tr.h_a_all + (size_t)t * BA;   // h_a(t-1)
        if (tr.c_d_all) { dec->c = tr.c_d_all + (size_t)(t - 1) * BD; dec->c_out = tr.c_d_all + (size_t)t * BD; }
    }
}

// Launch t of the step loops: attention-LSTM(t) together with decoder-LSTM(t-1), which is off the critical chain (only the next
// step's projection needs it); launch T, the drain, is the last decoder LSTM alone.  Returns the number of jobs.
int tf_step_jobs(const TfLoop& c, int t, SkinnyJob* jobs) {
    const gvx_dims& d = c.m->d;
    SkinnyJob* att = t < c.T ? &jobs[0] : nullptr;
    SkinnyJob* dec = t > 0 ? &jobs[att ? 1 : 0] : nullptr;
    if (att) {
        fill_att_job(c.m, *att, c.db.prenet + (size_t)t * c.B * d.prenet_dim, t, c.B, c.db);
        defer_context(c, *att, t - 1, t == 0);
    }
    if (dec) {
        fill_dec_job(c.m, *dec, t - 1, c.B, c.db);
        defer_context(c, *dec, t - 1, false);
    }
    if (c.train) wire_tape(*c.train, att, dec, t, (size_t)c.B * d.att_rnn_dim, (size_t)c.B * d.dec_rnn_dim);
    return (att ? 1 : 0) + (dec ? 1 : 0);
}

// Layout 3 (33 .. 64 rows): every launch has two batch tiles per workgroup, so the matrix pipe, not the weight stream,
// sets its length - and a decoder-LSTM tile (320 k-groups) would take 1.7x an attention-LSTM tile (192).  The decoder cell
// is therefore cut in two along K and finished one launch later:
//   launch t:  att-LSTM(t)            [ctx(t-1) deferred ; h_a(t-1)]            128 tiles x 192 k-groups
//              dec-LSTM(t-1) partial  [h_a(t-1) ; ctx(t-1) deferred] -> sums    128 tiles x 192 k-groups   (mode 2)
//              dec-LSTM(t-2) final    [h_d(t-3)] + those sums of launch t-1     128 tiles x 128 k-groups
// 384 workgroups on the 192 CUs the resident kernel leaves, two per CU; two drain launches end the loop.
int tf_step_jobs64(const TfLoop& c, int t, SkinnyJob* jobs) {
    const gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim, B = c.B, T = c.T;
    const DecoderBuffers& db = c.db;
    float* dec_part2[2] = {db.dec_part, db.dec_part + (size_t)B * 4 * D};
    int n = 0;
    if (t < T) {
        fill_att_job(m, jobs[n], db.prenet + (size_t)t * B * P, t, B, db);
        defer_context(c, jobs[n], t - 1, t == 0);
        ++n;
    }
    if (t >= 1 && t - 1 < T) {
        SkinnyJob& J = jobs[n];
        fill_dec_job(m, J, t - 1, B, db);
        J.x[2] = XSeg{nullptr, 0};
        J.nkg = (A + E) / 8; J.kg0 = 0; J.nkg_w = (A + E + D) / 8;
        J.mode = 2; J.bias = nullptr; J.c = nullptr; J.h_out = nullptr;
        J.y = dec_part2[t & 1];
        defer_context(c, J, t - 1, false);
        ++n;
    }
    if (t >= 2 && t - 2 < T) {
        SkinnyJob& J = jobs[n];
        std::memset(&J, 0, sizeof J);
        const float* hc_t = db.hc + (size_t)(t - 2) * B * (D + E);
        float* hc_n = db.hc + (size_t)(t - 1) * B * (D + E);
        J.Wp = m->dev_blob + m->blob.dec_frag; J.bias = m->dev_blob + m->blob.dec_bias;
        J.x[0] = XSeg{hc_t, D};
        J.N = 4 * D; J.nkg = D / 8; J.kg0 = (A + E) / 8; J.nkg_w = (A + E + D) / 8; J.mode = 0; J.B = B;
        J.c = db.c_d; J.h_out = hc_n;
        J.addend = dec_part2[(t - 1) & 1]; J.add_bs = 4 * D;
        J.start_cnt = c.sync + HANDOFF_CNT_Q;   // (only counts when this job owns block 0: never, a partial job precedes it)
        ++n;
    }
    return n;
}

// the step launches of one call: enqueued, or replayed from the hipGraph of (workspace, weight blob, shape, variant) - the
// loop only touches workspace operands (alignments go to a time-major workspace buffer, the lengths are copied in)
template <class F>
int enqueue_or_replay(const TfLoop& c, int variant, hipStream_t s, F&& enqueue) {
    if (!c.plan.graph) return enqueue(s);
    const gvx_model::LoopKey key{c.ws, c.memory, c.m->dev_blob, c.B, c.L, c.T, c.len_ws != nullptr, 0.f, variant};
    return run_chunk(c.m, touch_graph_set(c.m, c.m->loop_graphs, key), 0, s, enqueue);
}

// kind 2: one launch for the whole loop: attention LSTM (t) and decoder LSTM (t) of every step, hand-offs by flags
int tf_loop_resident(const TfLoop& c, hipStream_t s, int* launches) {
    gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    DecResidentParams rp{};
    fill_resident_common(m, c.db, c.sync, c.B, c.T, rp);
    rp.pre_gate = c.db.pre_gate;
    rp.kg_pre = d.prenet_dim / 8;
    if (const LstmDropout* train = c.train) {
        rp.h_a = train->h_a_all;
        rp.tr_keep_a = train->att_keep; rp.tr_keep_d = train->dec_keep; rp.tr_scale_a = train->att_scale; rp.tr_scale_d = train->dec_scale;
        rp.tr_c_a = train->c_a_all; rp.tr_c_d = train->c_d_all; rp.tr_pre_a = train->pre_a_all; rp.tr_pre_d = train->pre_d_all;
    }
    rp.dec_frag_bytes = (unsigned)(frag_floats(4 * d.dec_rnn_dim, d.att_rnn_dim + d.embed_dim + d.dec_rnn_dim) * sizeof(float));
    rp.layout = c.plan.tile_layout;
    if (m->ktiming) HIP_TRY(hipEventRecord(m->kev[0], s));
    HIP_TRY(launch_decoder_resident(rp, s));
    if (m->ktiming) {
        HIP_TRY(hipEventRecord(m->kev[1], s));
        HIP_TRY(hipEventRecord(m->kev[2], s));
        m->n_lstm_ev = c.T; m->n_attn_ev = 0;   // (the kernel's duration over its T steps)
    }
    *launches = 1;
    return GVX_OK;
}

// kind 1: T + 1 LSTM launches beside the resident attention kernel (layout 3: T + 2 launches of up to three jobs)
int tf_loop_beside_attention(const TfLoop& c, hipStream_t s, int* launches) {
    *launches = c.plan.rows64 ? c.T + 2 : c.T + 1;
    if (c.plan.rows64)
        return enqueue_or_replay(c, 48, s, [&](hipStream_t st) -> int {
            SkinnyJob jobs[3];
            for (int t = 0; t < c.T + 2; ++t) HIP_TRY(launch_skinny_pa64(jobs, tf_step_jobs64(c, t, jobs), st));
            return GVX_OK;
        });
    return enqueue_or_replay(c, c.m->pa_depth + 16 * c.plan.pa_layout, s, [&](hipStream_t st) -> int {
        SkinnyJob jobs[2];
        for (int t = 0; t < c.T; ++t) {
            tf_step_jobs(c, t, jobs);
            HIP_TRY(launch_skinny_pa(jobs[0], t > 0 ? &jobs[1] : nullptr, st, c.m->pa_depth, c.plan.pa_layout));
        }
        tf_step_jobs(c, c.T, jobs);
        HIP_TRY(launch_skinny(jobs, 1, SK_DECODER, st));
        return GVX_OK;
    });
}

// kind 0: launch 1 of step t is the LSTM launch (tf_step_jobs), launch 2 the attention step (energies, softmax, context;
// GVX_ATTN_SPLIT=1: the round-1 energy + context pair); 2T+1 launches
int tf_loop_per_step(const TfLoop& c, hipStream_t s, int* launches) {
    const gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    const int B = c.B, L = c.L, T = c.T;
    *launches = (m->attn_one_launch ? 2 : 3) * T + 1;
    return enqueue_or_replay(c, 0, s, [&](hipStream_t st) -> int {
        SkinnyJob jobs[2];
        for (int t = 0; t < T; ++t) {
            const int n = tf_step_jobs(c, t, jobs);
            LocJob lq;
            fill_loc(m, lq, t, B, L, c.db.align_tm, (long)L, (long)B * L, c.db);
            HIP_TRY(launch_skinny(jobs, n, SK_DECODER, st, &lq));
            AttnParams ap;
            fill_attn(m, ap, c.memory, c.len_ws, t, B, L, c.db.align_tm, (long)L, (long)B * L, c.db);
            if (m->attn_prefetch && m->attn_one_launch && B <= 32) {   // (gvx_model::attn_prefetch)
                ap.pf_w[0] = m->dev_blob + m->blob.att_frag; ap.pf_w[1] = m->dev_blob + m->blob.dec_frag;
                ap.pf_nkg[0] = (d.prenet_dim + d.embed_dim + d.att_rnn_dim) / 8; ap.pf_nkg[1] = (d.att_rnn_dim + d.embed_dim + d.dec_rnn_dim) / 8;
                ap.pf_tiles0 = 4 * d.att_rnn_dim / 32; ap.pf_tiles = ap.pf_tiles0 + 4 * d.dec_rnn_dim / 32;
            }
            HIP_TRY(launch_attn(m, ap, st));
        }
        tf_step_jobs(c, T, jobs);
        HIP_TRY(launch_skinny(jobs, 1, SK_DECODER, st));
        return GVX_OK;
    });
}

// Per-kernel duration for the roofline figure (gvx_kernel_timing_enable): the launch of a mid-sequence step replayed back to
// back between two events on this stream (bracketing every launch of the real loop with events measures launch gaps, not
// the kernel).  The replays scribble over the recurrent state, which nobody reads after this point of an
// instrumented pass except the projection of the already finished outputs' copies.
int tf_time_step_launches(const TfLoop& c, hipStream_t s) {
    gvx_model* m = c.m;
    const int B = c.B, L = c.L, REPS = 64, tm = c.T > 1 ? c.T / 2 : 0;
    SkinnyJob jobs[3];
    fill_att_job(m, jobs[0], c.db.prenet + (size_t)tm * B * m->d.prenet_dim, tm, B, c.db);
    if (tm > 0) fill_dec_job(m, jobs[1], tm - 1, B, c.db);
    m->n_lstm_ev = REPS;
    m->n_attn_ev = 0;
    if (c.plan.kind == 0) {
        LocJob lq;
        fill_loc(m, lq, tm, B, L, c.db.align_tm, (long)L, (long)B * L, c.db);
        AttnParams ap;
        fill_attn(m, ap, c.memory, c.len_ws, tm, B, L, c.db.align_tm, (long)L, (long)B * L, c.db);
        ap.w_out = c.db.energies;  // do not disturb the real alignments / cumulative weights (db.loc is an INPUT of the
        ap.w_cum = c.db.energies;  // one-launch step: it must not be scribbled on)
        HIP_TRY(hipEventRecord(m->kev[0], s));
        for (int i = 0; i < REPS; ++i) HIP_TRY(launch_skinny(jobs, tm > 0 ? 2 : 1, SK_DECODER, s, &lq));
        HIP_TRY(hipEventRecord(m->kev[1], s));
        for (int i = 0; i < REPS; ++i) HIP_TRY(launch_attn(m, ap, s));
        HIP_TRY(hipEventRecord(m->kev[2], s));
        m->n_attn_ev = REPS;
        return GVX_OK;
    }
    // the launch of the loop as it ran: deferred context columns read with sc1 loads; the context counter already
    // stands at its final value, so no replay waits (the attention runs in its own kernel: nothing to time per step)
    HIP_TRY(hipStreamWaitEvent(s, m->pa_join, 0));
    int n = 0;
    if (c.plan.rows64) {
        n = tf_step_jobs64(c, tm > 2 ? tm : 2, jobs);
    } else {
        defer_context(c, jobs[0], tm - 1, false);
        if (tm > 0) defer_context(c, jobs[1], tm - 1, false);
        n = tm > 0 ? 2 : 1;
    }
    for (int i = 0; i < n; ++i) jobs[i].start_cnt = nullptr;
    HIP_TRY(hipEventRecord(m->kev[0], s));
    for (int i = 0; i < REPS; ++i)
        HIP_TRY(c.plan.rows64 ? launch_skinny_pa64(jobs, n, s) : launch_skinny_pa(jobs[0], tm > 0 ? &jobs[1] : nullptr, s, m->pa_depth, c.plan.pa_layout));
    HIP_TRY(hipEventRecord(m->kev[1], s));
    HIP_TRY(hipEventRecord(m->kev[2], s));
    return GVX_OK;
}

}  // namespace

int decoder_tf_impl(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, const float* mel_in, int T,
                    const uint8_t* keep_masks, float* mel_out, float* gate_out, float* align_out, void* ws, const WsPlan& wp,
                    hipStream_t s, bool prenet_done, const LstmDropout* train) {
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, M = d.n_mels, D = d.dec_rnn_dim;
    const DecoderBuffers db = decoder_buffers(ws, wp);
    unsigned* sync = ws_ptr<unsigned>(ws, wp.sync);
    HIP_TRY(zero_async(sync, HANDOFF_WORDS * sizeof(unsigned), s));   // hand-off status of THIS call
    const bool timed = m->timing && m->ev_valid;
    int rc = GVX_OK;
    if (!prenet_done) {   // (the fused forward has run both behind its encoder: the states on the side stream, beside the Prenet products)
        rc = decoder_prenet_part(m, B, L, mel_in, T, keep_masks, ws, wp, s);
        if (rc != GVX_OK) return rc;
        rc = decoder_init_states(m, memory, B, L, db, s);
        if (rc != GVX_OK) return rc;
    }
    if (timed) HIP_TRY(hipEventRecord(m->ev[2], s));
    const int32_t* len_ws = nullptr;
    if (lengths) {
        HIP_TRY(hipMemcpyAsync(db.len_copy, lengths, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        len_ws = db.len_copy;
    }
    if (m->ktiming) {
        rc = m->reserve_events(4);
        if (rc != GVX_OK) return rc;
        m->n_lstm_ev = m->n_attn_ev = 0;
    }
    const bool tape_whole = train && train->h_a_all && train->c_a_all && train->c_d_all && train->pre_a_all && train->pre_d_all;
    const TfLoopPlan plan = plan_teacher_forced(m, B, L, !train ? TF_INFERENCE : (tape_whole ? TF_TRAIN_WHOLE_TAPE : TF_TRAIN_PARTIAL_TAPE));
    const TfLoop c{m, plan, db, memory, len_ws, ws, sync, ws_ptr<float>(ws, wp.xchg), B, L, T, train};
    // ---- the T decoder steps, by the plan's kind.  Beside the resident attention kernel the loop takes a turn on the device:
    // the mutex is held while the loop is enqueued (released on every return path)
    std::unique_lock<std::mutex> turn;
    if (plan.side_stream) {
        if (!prenet_done) {   // (the fused forward has taken a side stream for this call already: the encoder ran on it)
            rc = ensure_side_stream(m);
            if (rc != GVX_OK) return rc;
        }
        turn = std::unique_lock<std::mutex>(g_turn_mutex);
        rc = turn_begin(s);
        if (rc != GVX_OK) return rc;
        AttnPersistParams pp = fill_attn_persist(m, db, memory, len_ws, sync, B, L, T);   // (the hand-off words were zeroed at the top of this call)
        pp.n_slabs = attention_persistent_slabs(plan.tile_layout);
        pp.xchg = c.xchg;
        pp.q_first = 2;   // (launch 0 announces its start too)
        if (plan.kind == 2) use_resident_flags(m, pp);
        rc = launch_resident_attention(m, pp, s);
        if (rc != GVX_OK) return rc;
    }
    int launches = 0;
    switch (plan.kind) {
        case 2: rc = tf_loop_resident(c, s, &launches); break;
        case 1: rc = tf_loop_beside_attention(c, s, &launches); break;
        default: rc = tf_loop_per_step(c, s, &launches); break;
    }
    if (rc != GVX_OK) return rc;
    if (plan.side_stream) {
        HIP_TRY(hipStreamWaitEvent(s, m->pa_join, 0));
        ++launches;
        rc = turn_end(s);
        if (rc != GVX_OK) return rc;
        turn.unlock();
    }
    if (m->ktiming && plan.kind != 2) {   // (measurement, not the loop)
        rc = tf_time_step_launches(c, s);
        if (rc != GVX_OK) return rc;
    }
    // alignments: time-major workspace [T][B][L] -> caller's [B][T][L]
    HIP_TRY(launch_permute01(db.align_tm, align_out, T, B, L, s));
    m->last_decoder_launches = launches;
    if (timed) HIP_TRY(hipEventRecord(m->ev[3], s));
    // ---- mel + gate projection hoisted out of the loop: one GEMM over all T*B rows of hc[1..T]
    {
        const int PS = m->PS();
        GemmParams g{};
        g.A = db.hc + (size_t)B * (D + E); g.amap = RowMap{B, (long)B * (D + E), 8}; g.a_kblk = (long)B * 8;  // slots 1..T, blocked
        g.W = m->dev_blob + m->blob.proj_w; g.ldw = D + E;
        g.C = db.proj; g.cmap = RowMap{B, (long)PS, (long)T * PS};  // row (t,b) -> proj[b][t][:]
        g.bias = m->dev_blob + m->blob.proj_b;
        g.M = T * B; g.N = M + 1; g.K = D + E; g.act = ACT_NONE;
        HIP_TRY(launch_gemm(g, s));
        HIP_TRY(launch_split_projection(db.proj, mel_out, gate_out, B, M, T, s));
    }
    return GVX_OK;
}

// ===================================================================================================== autoregressive loop
namespace {

struct ArLoop {   // one autoregressive call: what its loop kinds share
    gvx_model* m; ArLoopPlan plan; DecoderBuffers db;
    const float* memory_ws; const int32_t* len_ws; const uint8_t* masks_ws; void* ws; unsigned* sync; float* xchg;
    int32_t* n_done; int32_t* n_frames_ws;
    int B, L, T;
    float gate_threshold;
    int32_t* centres; int win_back, win_ahead;   // monotonic attention window (centres == nullptr: none): the caller's [B][T] buffer is the steps' state
};

void print_ws_plan_once(const WsPlan& wp) {   // (diagnostics, tools/ar_ws_diff.py: byte offsets of the workspace buffers)
    static bool printed = false;
    if (printed) return;
    printed = true;
#define GVX_PL(f) std::fprintf(stderr, "wsplan %s %zu\n", #f, wp.f);
    GVX_PL(xa) GVX_PL(xb) GVX_PL(xg) GVX_PL(enc_h) GVX_PL(enc_c) GVX_PL(flags) GVX_PL(sync) GVX_PL(memory) GVX_PL(pm) GVX_PL(frames) GVX_PL(pre1) GVX_PL(prenet) GVX_PL(h_a) GVX_PL(c_a) GVX_PL(c_d)
    GVX_PL(hc) GVX_PL(w_cum) GVX_PL(q_slab) GVX_PL(proj) GVX_PL(energies) GVX_PL(align_tm) GVX_PL(len_copy) GVX_PL(loc) GVX_PL(ar_masks)
    GVX_PL(p_slab) GVX_PL(p_ctx) GVX_PL(att_part) GVX_PL(dec_part) GVX_PL(pre_gate) GVX_PL(xchg) GVX_PL(ya) GVX_PL(yb) GVX_PL(total)
#undef GVX_PL
}

// One step = 5 launches.  In autoregressive mode BOTH cells are on the critical chain (the frame feeds back), and a cell
// alone is only 128 tiles - half the chip.  But most of a cell's input is known one launch early: the attention LSTM's
// [ctx(t-1) ; h_a(t-1)] columns (1536 of 1792) exist before the decoder LSTM of step t-1 runs, the decoder LSTM's h_d(t-1)
// columns (1024 of 2560) before the attention LSTM of step t.  So every LSTM launch runs 128 tiles that FINISH one cell
// (remaining columns + partial sums of the others through `addend`) next to 128 tiles that pre-compute the other cell's
// early columns (mode 2, partial sums to att_part / dec_part): all 256 CUs stream weights in both launches.
//   A(t): attention LSTM final [prenet(t)]            + decoder LSTM partial [h_d(t-1)]      + location features
//   energies(t), context(t)
//   C(t): decoder LSTM final [h_a(t) ; ctx(t)] (+ mel/gate projection partials of its 8 hidden units)
//         + attention LSTM partial for step t+1 [ctx(t) ; h_a(t)] + 3 tiles projecting the context
//   D(t): projection reduction, per-row stop test, whole Prenet of step t+1 on the fresh frame
// db.proj holds one blocked projection vector [PSB/8][B][8] per step.
struct ArStep {   // operands of step t
    const float* hc_t; float* hc_n; float* ctx_n; float* ha_new; float* att_part2; float* dec_part2;
    int kgP, kgE, kgA, kgD;
};
ArStep ar_step(const ArLoop& c, int t) {
    const gvx_dims& d = c.m->d;
    const int E = d.embed_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim, B = c.B;
    ArStep q;
    q.hc_t = c.db.hc + (size_t)t * B * (D + E);
    q.hc_n = c.db.hc + (size_t)(t + 1) * B * (D + E);
    q.ctx_n = q.hc_n + (size_t)D * B;
    q.ha_new = c.db.h_a + (size_t)((t + 1) & 1) * B * A;
    q.att_part2 = c.db.att_part + (size_t)B * 4 * A;
    q.dec_part2 = c.db.dec_part + (size_t)B * 4 * D;
    q.kgP = d.prenet_dim / 8; q.kgE = E / 8; q.kgA = A / 8; q.kgD = D / 8;
    return q;
}

// launch A of step t and, without the resident attention kernel, the attention step behind it
int ar_launch_a(const ArLoop& c, const ArStep& q, int t, hipStream_t st) {
    const gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    const DecoderBuffers& db = c.db;
    const int P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim, B = c.B, L = c.L;
    const int kgP = q.kgP, kgE = q.kgE, kgA = q.kgA, kgD = q.kgD;
    SkinnyJob ja[2];
    std::memset(ja, 0, sizeof ja);
    {   // attention LSTM of step t: final tiles over the Prenet columns
        SkinnyJob& J = ja[0];
        J.Wp = m->dev_blob + m->blob.att_frag; J.bias = m->dev_blob + m->blob.att_bias;
        J.x[0] = XSeg{db.prenet, P};
        J.N = 4 * A; J.nkg = kgP; J.kg0 = 0; J.nkg_w = kgP + kgE + kgA; J.mode = 0; J.B = B;
        J.addend = db.att_part; J.add_bs = 4 * A; J.add_ts = 0;
        J.c = db.c_a; J.h_out = q.ha_new;
        J.Wq_t = m->dev_blob + m->blob.wq_t; J.q_slab = db.q_slab; J.att_dim = d.att_dim;
    }
    {   // decoder LSTM of step t: partial sums over the h_d(t-1) columns
        SkinnyJob& J = ja[1];
        J.Wp = m->dev_blob + m->blob.dec_frag;
        J.x[0] = XSeg{q.hc_t, D};
        J.N = 4 * D; J.nkg = kgD; J.kg0 = kgA + kgE; J.nkg_w = kgA + kgE + kgD; J.mode = 2; J.B = B;
        J.y = db.dec_part;
    }
    if (c.plan.kind != 0) {
        if (t == 0) {   // the first launch does not end before the resident kernel is resident: launch C waits for it
            ja[0].ready_cnt = c.sync + HANDOFF_READY; ja[0].ready_target = (unsigned)B;
            ja[0].tmo = c.sync + HANDOFF_TIMEOUT; ja[0].spin_limit = m->spin_limit;
        }
        HIP_TRY(launch_skinny(ja, 2, SK_AR, st));
        return GVX_OK;
    }
    LocJob lq;
    fill_loc(m, lq, t, B, L, db.align_tm, (long)L, (long)B * L, db);
    HIP_TRY(launch_skinny(ja, 2, SK_AR, st, &lq));
    AttnParams ap;
    fill_attn(m, ap, c.memory_ws, c.len_ws, t, B, L, db.align_tm, (long)L, (long)B * L, db);
    if (c.centres) {   // step t reads the centres step t - 1 stored and stores its own: two addresses, no hand-off inside a launch
        ap.c_prev = t > 0 ? c.centres + (t - 1) : nullptr; ap.c_out = c.centres + t; ap.c_bs = (long)c.T;
        ap.win_back = c.win_back; ap.win_ahead = c.win_ahead;
    }
    if (!c.plan.split_h) {
        HIP_TRY(launch_attn(m, ap, st));
        return GVX_OK;
    }
    SkinnyJob jb[2];
    std::memset(jb, 0, sizeof jb);
    {   // decoder LSTM of step t: partial sums over the h_a(t) columns
        SkinnyJob& J = jb[0];
        J.Wp = m->dev_blob + m->blob.dec_frag;
        J.x[0] = XSeg{q.ha_new, A};
        J.N = 4 * D; J.nkg = kgA; J.kg0 = 0; J.nkg_w = kgA + kgE + kgD; J.mode = 2; J.B = B;
        J.y = q.dec_part2;
    }
    {   // attention LSTM of step t+1: partial sums over the h_a(t) columns
        SkinnyJob& J = jb[1];
        J.Wp = m->dev_blob + m->blob.att_frag;
        J.x[0] = XSeg{q.ha_new, A};
        J.N = 4 * A; J.nkg = kgA; J.kg0 = kgP + kgE; J.nkg_w = kgP + kgE + kgA; J.mode = 2; J.B = B;
        J.y = q.att_part2;
    }
    HIP_TRY(launch_skinny_attn(jb, 2, ap, st));
    return GVX_OK;
}

// launches C and D of step t
int ar_launch_cd(const ArLoop& c, const ArStep& q, int t, hipStream_t st) {
    const gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    const DecoderBuffers& db = c.db;
    const int E = d.embed_dim, M = d.n_mels, P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim, B = c.B, T = c.T, PSB = m->PSB();
    const int kgP = q.kgP, kgE = q.kgE, kgA = q.kgA, kgD = q.kgD;
    const bool fold = c.plan.fold;
    SkinnyJob jc[3];
    std::memset(jc, 0, sizeof jc);
    {   // decoder LSTM of step t: final tiles over [h_a(t) ; ctx(t)]; every tile also emits the mel/gate projection
        // partial products of its 8 hidden units (the attention-query slab mechanism with the projection's h_d columns)
        SkinnyJob& J = jc[0];
        J.Wp = m->dev_blob + m->blob.dec_frag; J.bias = m->dev_blob + m->blob.dec_bias;
        J.x[0] = XSeg{q.ha_new, A};
        J.x[1] = XSeg{q.ctx_n, E};
        J.N = 4 * D; J.nkg = kgA + kgE; J.kg0 = 0; J.nkg_w = kgA + kgE + kgD; J.mode = 0; J.B = B;
        J.addend = db.dec_part; J.add_bs = 4 * D; J.add_ts = 0;
        J.c = db.c_d; J.h_out = q.hc_n;
        J.Wq_t = m->dev_blob + m->blob.proj_hd_t; J.q_slab = db.p_slab; J.att_dim = PSB;
        if (fold) { J.xw = m->dev_blob + m->blob.proj_ctx_t; J.xsrc = q.ctx_n; }
    }
    {   // attention LSTM of step t+1: partial sums over [ctx(t) ; h_a(t)]  (x[0] is an empty segment so that the
        // context is x[1], the segment the deferred order streams last)
        SkinnyJob& J = jc[1];
        J.Wp = m->dev_blob + m->blob.att_frag;
        J.x[0] = XSeg{q.ctx_n, 0};
        J.x[1] = XSeg{q.ctx_n, E};
        J.x[2] = XSeg{q.ha_new, A};
        J.N = 4 * A; J.nkg = kgE + kgA; J.kg0 = kgP; J.nkg_w = kgP + kgE + kgA; J.mode = 2; J.B = B;
        J.y = db.att_part;
    }
    if (c.plan.split_h) {   // launch C streams the context columns only; the h_a columns arrive as sums
        SkinnyJob& Jd = jc[0];
        Jd.x[0] = XSeg{q.ctx_n, E}; Jd.x[1] = XSeg{nullptr, 0};
        Jd.nkg = kgE; Jd.kg0 = kgA;
        Jd.addend2 = q.dec_part2;
        SkinnyJob& Ja = jc[1];
        Ja.x[0] = XSeg{q.ctx_n, E}; Ja.x[1] = XSeg{nullptr, 0}; Ja.x[2] = XSeg{nullptr, 0};
        Ja.nkg = kgE; Ja.kg0 = kgP;
        Ja.addend = q.att_part2; Ja.add_bs = 4 * A;
    }
    if (c.plan.kind != 0)
        for (int i = 0; i < 2; ++i) {   // the context of step t is published by the resident kernel while this launch streams
            SkinnyJob& J = jc[i];
            J.defer_seg = 1;
            J.ctx_cnt = c.sync + HANDOFF_CNT_CTX; J.ctx_target = (unsigned)B * (unsigned)(t + 1);
            J.tmo = c.sync + HANDOFF_TIMEOUT; J.spin_limit = m->spin_limit;
            if (i == 0) J.start_cnt = c.sync + HANDOFF_CNT_Q;   // "launch A of this step has completed: its query slabs are in memory"
        }
    if (!fold) {   // context columns of the mel/gate projection (known before the launch)
        SkinnyJob& J = jc[2];
        J.Wp = m->dev_blob + m->blob.proj_ctx_frag; J.bias = m->dev_blob + m->blob.proj_b;
        J.x[0] = XSeg{q.ctx_n, E};
        J.N = M + 1; J.nkg = kgE; J.mode = 1; J.B = B; J.act = ACT_NONE;
        J.y = db.p_ctx;
    }
    HIP_TRY(launch_skinny(jc, fold ? 2 : 3, SK_AR, st));
    const bool more = t + 1 < T;
    HIP_TRY(launch_ar_project(db.p_slab, D / 8, db.p_ctx, db.proj + (size_t)t * B * PSB, M, c.gate_threshold, t, B, c.n_frames_ws, c.n_done,
                              m->dev_blob + m->blob.pre_w0_t, m->dev_blob + m->blob.pre_w1_t, P,
                              more ? c.masks_ws + (size_t)(t + 1) * B * P : nullptr,
                              more ? c.masks_ws + ((size_t)T + t + 1) * B * P : nullptr, db.prenet, st));
    return GVX_OK;
}

int ar_enqueue_steps(const ArLoop& c, hipStream_t st, int t0, int t1) {
    for (int t = t0; t < t1; ++t) {
        const ArStep q = ar_step(c, t);
        int rc = ar_launch_a(c, q, t, st);
        if (rc == GVX_OK) rc = ar_launch_cd(c, q, t, st);
        if (rc != GVX_OK) return rc;
    }
    return GVX_OK;
}

// kind 2: the whole decode as TWO resident kernels (dec_resident.hip decoder_ar_resident_kernel + attn_persist.hip, AR role): no
// launch per step, no host check - the kernels find the end of the loop themselves (every row's stop token has fired: the
// stop word holds the number of steps that ran) or run into max_steps.  Returns the steps that ran in *steps.
int ar_loop_resident(const ArLoop& c, hipStream_t s, int* steps) {
    gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    const DecoderBuffers& db = c.db;
    const int B = c.B, T = c.T, P = d.prenet_dim, PSB = m->PSB();
    std::unique_lock<std::mutex> turn(g_turn_mutex);   // resident loops take turns on the device
    int rc = turn_begin(s);
    if (rc != GVX_OK) return rc;
    AttnPersistParams pp = fill_attn_persist(m, db, c.memory_ws, c.len_ws, c.sync, B, c.L, T);
    pp.n_slabs = attention_persistent_slabs(1);
    pp.xchg = c.xchg;   // (rows of 129-256 tokens: the halves' exchange buffers)
    pp.q_first = 1;
    use_resident_flags(m, pp);
    pp.p_slab = db.p_slab; pp.PSB = PSB; pp.n_mels = d.n_mels; pp.proj_b = m->dev_blob + m->blob.proj_b; pp.proj_out = db.proj;
    pp.pre_w0_t = m->dev_blob + m->blob.pre_w0_t; pp.keep0 = c.masks_ws; pp.y1 = db.pre1;
    pp.n_frames = c.n_frames_ws; pp.n_done = c.n_done; pp.gate_threshold = c.gate_threshold;
    pp.p_flags = c.sync + RS_FLAG_P; pp.y1_flags = c.sync + RS_FLAG_Y1;
    pp.centres = c.centres; pp.win_back = c.win_back; pp.win_ahead = c.win_ahead;
    rc = launch_resident_attention(m, pp, s);
    if (rc != GVX_OK) return rc;
    ArResidentParams rp{};
    fill_resident_common(m, db, c.sync, B, T, rp);
    rp.proj_hd_t = m->dev_blob + m->blob.proj_hd_t; rp.proj_ctx_t = m->dev_blob + m->blob.proj_ctx_t;
    rp.pre_w1 = m->dev_blob + m->blob.pre_w1; rp.keep1 = c.masks_ws + (size_t)T * B * P;
    rp.prenet = db.prenet; rp.y1 = db.pre1;
    rp.p_slab = db.p_slab;
    rp.n_done = c.n_done;
    rp.PSB = PSB;
    HIP_TRY(launch_decoder_ar_resident(rp, s));
    HIP_TRY(hipStreamWaitEvent(s, m->pa_join, 0));
    rc = turn_end(s);
    if (rc != GVX_OK) return rc;
    turn.unlock();
    rc = ensure_ar_host_slots(m);
    if (rc != GVX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(m->ar_done_host, c.sync + HANDOFF_STOP, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *steps = m->ar_done_host[0] > 0 && m->ar_done_host[0] < T ? m->ar_done_host[0] : T;
    return GVX_OK;
}

// kinds 0 and 1: step launches in chunks of 16 (one hipGraph each), the host reads the all-rows-finished counter between chunks
int ar_loop_chunked(const ArLoop& c, hipStream_t s, int* steps) {
    gvx_model* m = c.m;
    const gvx_dims& d = m->d;
    const DecoderBuffers& db = c.db;
    const int B = c.B, L = c.L, T = c.T;
    if (c.plan.fold) {   // p_ctx = the projection's bias, once: the linear job on the all-zero context of slot 0
        SkinnyJob J;
        std::memset(&J, 0, sizeof J);
        J.Wp = m->dev_blob + m->blob.proj_ctx_frag; J.bias = m->dev_blob + m->blob.proj_b;
        J.x[0] = XSeg{db.hc + (size_t)d.dec_rnn_dim * B, d.embed_dim};
        J.N = d.n_mels + 1; J.nkg = d.embed_dim / 8; J.mode = 1; J.B = B; J.act = ACT_NONE;
        J.y = db.p_ctx;
        HIP_TRY(launch_skinny(&J, 1, SK_AR, s));
    }
    if (c.plan.kind == 1) {   // the resident kernel: launched eagerly on the handle's side stream, behind everything queued on `s` so far
        AttnPersistParams pp = fill_attn_persist(m, db, c.memory_ws, c.len_ws, c.sync, B, L, T);
        pp.n_slabs = d.att_rnn_dim / 8;
        pp.q_first = 1;   // one signalling launch (C) per step
        const int rc = launch_resident_attention(m, pp, s);
        if (rc != GVX_OK) return rc;
    }
    const int CHUNK = 16;  // steps per graph = steps between host checks of the all-rows-finished counter
    gvx_model::GraphSet* gset = nullptr;
    if (c.plan.graph) {
        gvx_model::LoopKey key{c.ws, c.memory_ws, m->dev_blob, B, L, T, c.len_ws != nullptr};
        key.threshold = c.gate_threshold;
        key.variant = c.plan.kind == 1 ? 1 : (c.plan.split_h ? 2 : 0);
        key.centres = c.centres; key.win_back = c.win_back; key.win_ahead = c.win_ahead;
        gset = touch_graph_set(m, m->ar_graphs, key);
    }
    // One chunk of look-ahead: chunk k + 1 is enqueued BEFORE the host reads chunk k's all-rows-finished counter (pinned slot,
    // event), so the GPU never idles for the round trip of the check (~63 of them in a 1000-step decode: 30-40 us each).  When
    // chunk k turns out to have finished every row, the chunk already in flight runs 16 more steps that nobody reads: rows that
    // have fired keep their frame counts, and only the steps up to the end of chunk k are emitted below.
    int rc = ensure_ar_host_slots(m);
    if (rc != GVX_OK) return rc;
    auto enqueue_chunk = [&](int t0, int slot) -> int {
        const int t1 = t0 + CHUNK < T ? t0 + CHUNK : T;
        const int r = run_chunk(m, gset, (size_t)(t0 / CHUNK), s, [&](hipStream_t st) { return ar_enqueue_steps(c, st, t0, t1); });
        if (r != GVX_OK) return r;
        HIP_TRY(hipMemcpyAsync(m->ar_done_host + slot, c.n_done, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(m->ar_ev[slot], s));
        return GVX_OK;
    };
    rc = enqueue_chunk(0, 0);
    if (rc != GVX_OK) return rc;
    int t_enq = CHUNK < T ? CHUNK : T, slot = 0;   // steps enqueued so far; slot of the chunk the host looks at next
    for (;;) {
        const int t_chunk_end = t_enq;   // end of the chunk whose counter is read next
        const bool more = t_enq < T;
        if (more) {
            rc = enqueue_chunk(t_enq, slot ^ 1);
            if (rc != GVX_OK) return rc;
            t_enq = t_enq + CHUNK < T ? t_enq + CHUNK : T;
        }
        HIP_TRY(hipEventSynchronize(m->ar_ev[slot]));
        *steps = t_chunk_end;
        if (m->ar_done_host[slot] >= B || !more) break;
        slot ^= 1;
    }
    if (c.plan.kind == 1) {   // the loop may have ended early: tell the resident kernel (it leaves at its next look), then wait for it
        HIP_TRY(launch_handoff_set(c.sync + HANDOFF_STOP, s));
        HIP_TRY(hipStreamWaitEvent(s, m->pa_join, 0));
    }
    return GVX_OK;
}

// both exports of the autoregressive decode; centres_out == nullptr: no window
int decoder_ar_impl(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, int max_steps, float gate_threshold,
                    const uint8_t* keep_masks, float* mel_out, float* gate_out, float* align_out, int32_t* n_frames_out, int* steps_run_out,
                    void* ws, size_t ws_bytes, void* stream, int window_back, int window_ahead, int32_t* centres_out) {
    int rc = check_common(m, B, L, max_steps, ws, ws_bytes, WS_AUTOREGRESSIVE);
    if (rc != GVX_OK) return rc;
    if (!memory || !keep_masks || !mel_out || !gate_out || !align_out || !n_frames_out)
        return fail(GVX_ERR_INVALID_ARG, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const gvx_dims& d = m->d;
    const int E = d.embed_dim, M = d.n_mels, P = d.prenet_dim, A = d.att_rnn_dim, T = max_steps;
    const WsPlan wp = make_ws_plan(m, B, L, T, WS_AUTOREGRESSIVE);
    const DecoderBuffers db = decoder_buffers(ws, wp);
    if (m->debug_plan) print_ws_plan_once(wp);
    unsigned* sync = ws_ptr<unsigned>(ws, wp.sync);
    HIP_TRY(zero_async(sync, HANDOFF_WORDS * sizeof(unsigned), s));   // hand-off status of THIS call
    int32_t* flags = ws_ptr<int32_t>(ws, wp.flags);
    // Everything a step touches is moved next to the workspace so that the step launches only bake workspace addresses:
    // encoder output, token lengths and keep masks are copied in; alignments / per-step projections stay in workspace
    // buffers and are scattered to the caller's tensors once, after the loop.
    float* memory_ws = ws_ptr<float>(ws, wp.memory);
    if (memory != memory_ws)
        HIP_TRY(hipMemcpyAsync(memory_ws, memory, (size_t)B * L * E * sizeof(float), hipMemcpyDeviceToDevice, s));
    uint8_t* masks_ws = ws_ptr<uint8_t>(ws, wp.ar_masks);
    HIP_TRY(hipMemcpyAsync(masks_ws, keep_masks, (size_t)2 * T * B * P, hipMemcpyDeviceToDevice, s));
    const int32_t* len_ws = nullptr;
    if (lengths) {
        HIP_TRY(hipMemcpyAsync(db.len_copy, lengths, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        len_ws = db.len_copy;
    }
    rc = decoder_init_states(m, memory_ws, B, L, db, s);
    if (rc != GVX_OK) return rc;
    const ArLoop c{m, plan_autoregressive(m, B, L, centres_out != nullptr), db, memory_ws, len_ws, masks_ws, ws, sync, ws_ptr<float>(ws, wp.xchg),
                   flags + FLAG_AR_DONE, flags + FLAG_AR_FRAMES, B, L, T, gate_threshold, centres_out, window_back, window_ahead};
    if (c.plan.kind != 0) {
        rc = ensure_side_stream(m);
        if (rc != GVX_OK) return rc;
    }
    HIP_TRY(zero_async(db.prenet, (size_t)B * P * sizeof(float), s));       // Prenet of the go-frame: no biases, relu(W 0) = 0
    HIP_TRY(zero_async(db.att_part, (size_t)B * 4 * A * sizeof(float), s)); // ctx(-1) = h_a(-1) = 0
    HIP_TRY(zero_async(c.n_done, sizeof(int32_t), s));                       // (the sticky status words in between stay)
    HIP_TRY(zero_async(c.n_frames_ws, (size_t)64 * sizeof(int32_t), s));
    int t = 0;   // steps that ran
    rc = c.plan.kind == 2 ? ar_loop_resident(c, s, &t) : ar_loop_chunked(c, s, &t);
    if (rc != GVX_OK) return rc;
    // rows that never fired ran into the cap ("Warning! Reached max decoder steps", models/tts/tacotron2.py:407-409)
    HIP_TRY(launch_ar_stop(db.proj, M, -1.f, t - 1, B, c.n_frames_ws, c.n_done, s));
    HIP_TRY(hipMemcpyAsync(n_frames_out, c.n_frames_ws, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    // rows that stopped early kept decoding until the last row finished: their frames past n_frames get the reference's
    // padding values (mel 0, gate 1e3, alignment 0 - mask_padding, models/tts/tacotron2.py:466-473)
    HIP_TRY(launch_ar_emit_all(db.proj, mel_out, gate_out, B, M, T, t, c.n_frames_ws, s));
    HIP_TRY(launch_permute01_partial(db.align_tm, align_out, t, T, B, L, c.n_frames_ws, s));
    if (centres_out) HIP_TRY(launch_ar_centres_finish(centres_out, c.n_frames_ws, c.plan.kind != 0 ? sync + HANDOFF_TIMEOUT : nullptr, B, T, s));
    if (c.plan.kind != 0) {   // a hand-off that timed out must not leave numbers that look like results
        float* outs[3] = {mel_out, gate_out, align_out};
        const size_t counts[3] = {(size_t)B * M * T, (size_t)B * T, (size_t)B * T * L};
        HIP_TRY(launch_poison_on_timeout(sync + HANDOFF_TIMEOUT, flags + FLAG_TIMEOUT, outs, counts, 3, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (steps_run_out) *steps_run_out = t;
    return GVX_OK;
}

}  // namespace
}  // namespace gvx

extern "C" int gvx_decoder_autoregressive(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, int max_steps,
                                          float gate_threshold, const uint8_t* keep_masks, float* mel_out, float* gate_out, float* align_out,
                                          int32_t* n_frames_out, int* steps_run_out, void* ws, size_t ws_bytes, void* stream) {
    return decoder_ar_impl(m, memory, lengths, B, L, max_steps, gate_threshold, keep_masks, mel_out, gate_out, align_out, n_frames_out,
                           steps_run_out, ws, ws_bytes, stream, 0, 0, nullptr);
}

extern "C" int gvx_decoder_autoregressive_windowed(gvx_model* m, const float* memory, const int32_t* lengths, int B, int L, int max_steps,
                                                   float gate_threshold, const uint8_t* keep_masks, float* mel_out, float* gate_out,
                                                   float* align_out, int32_t* n_frames_out, int* steps_run_out, void* ws, size_t ws_bytes,
                                                   void* stream, int window_back, int window_ahead, int32_t* centres_out) {
    if (window_back < 0 || window_ahead < 0)
        return fail(GVX_ERR_INVALID_ARG, "window_back and window_ahead must be >= 0 (got %d, %d)", window_back, window_ahead);
    if (!centres_out) return fail(GVX_ERR_INVALID_ARG, "null argument: centres_out is the window's state and is mandatory");
    if (L > 0) {   // (widths past the row change nothing; the kernels add them to a centre)
        window_back = window_back < L ? window_back : L;
        window_ahead = window_ahead < L ? window_ahead : L;
    }
    return decoder_ar_impl(m, memory, lengths, B, L, max_steps, gate_threshold, keep_masks, mel_out, gate_out, align_out, n_frames_out,
                           steps_run_out, ws, ws_bytes, stream, window_back, window_ahead, centres_out);
}
