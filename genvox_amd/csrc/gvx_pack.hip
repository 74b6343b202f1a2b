// Weight packing of the C-ABI layer: the layout of the packed blob and the two ways to fill it - on the host
// (gvx_model_pack_weights: BatchNorm folding, LSTM gate-row permutation, MFMA-fragment layout) and, for re-packing after an
// optimizer step, on the device (gvx_model_pack_weights_device: a gather map built once by the host packer + three small kernels).
#include "gvx_internal.h"

using namespace gvx;

namespace gvx {

Blob make_blob_layout(const gvx_dims& d) {
    Blob b{};
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align_up(off + n, 64); return o; };
    const int E = d.embed_dim, H = E / 2, M = d.n_mels, P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim;
    b.emb = take((size_t)d.n_tokens * E);
    for (int i = 0; i < d.enc_n_conv; ++i) { b.enc_w[i] = take((size_t)E * d.enc_kernel * E); b.enc_b[i] = take(E); }
    b.enc_wih = take((size_t)8 * H * E);
    b.enc_bih = take((size_t)8 * H);
    for (int dir = 0; dir < 2; ++dir) b.enc_whh_frag[dir] = take(frag_floats(4 * H, H));
    b.pre_w0 = take((size_t)P * M); b.pre_w1 = take((size_t)P * P);
    b.pre_w0_t = take((size_t)M * P);   // both Prenet matrices transposed ([in][out]) for the autoregressive step tail
    b.pre_w1_t = take((size_t)P * P);   // (ar_project_kernel)
    b.att_frag = take(frag_floats(4 * A, P + E + A)); b.att_bias = take((size_t)4 * A);
    b.att_wpre = take((size_t)4 * A * P);   // the Prenet columns of the attention LSTM again, plain [4A packed rows][P]: one GEMM per
                                            // teacher-forced loop applies them to all steps at once (persistent-attention path)
    b.wq_t = take((size_t)A * d.att_dim);
    b.wmem = take((size_t)d.att_dim * E); b.v = take(d.att_dim);
    b.loc_conv = take((size_t)2 * d.att_loc_kernel * 32);   // transposed [2][kl][32]
    b.loc_dense = take((size_t)32 * d.att_dim);             // transposed [32/4][a][4]
    b.dec_frag = take(frag_floats(4 * D, A + E + D)); b.dec_bias = take((size_t)4 * D);
    b.proj_w = take((size_t)(M + 1) * (D + E)); b.proj_b = take(M + 1);
    b.proj_frag = take(frag_floats(M + 1, D + E));
    b.proj_hd_t = take((size_t)D * ((M + 1 + 7) & ~7));
    b.proj_ctx_frag = take(frag_floats(M + 1, E));
    b.proj_ctx_t = take((size_t)(E / 4) * ((M + 1 + 7) & ~7) * 4);
    for (int i = 0; i < d.postnet_n_conv; ++i) {
        const int cin = i == 0 ? M : d.postnet_dim, cout = i == d.postnet_n_conv - 1 ? M : d.postnet_dim;
        b.post_w[i] = take((size_t)cout * d.postnet_kernel * cin);
        b.post_b[i] = take(cout);
    }
    // behind everything else (every older offset stays where it was): the Winograd transforms of the layers whose shape admits them
    for (int i = 0; i < d.postnet_n_conv; ++i)
        if (postnet_layer_winograd_shape(d, i)) b.post_u[i] = take((size_t)WINO_PTS * d.postnet_dim * d.postnet_dim);
    for (int i = 0; i < d.enc_n_conv; ++i)
        if (encoder_layer_winograd_shape(d, i)) b.enc_u[i] = take((size_t)WINO_PTS * E * E);
    b.total = off;
    return b;
}

}  // namespace gvx

namespace {

// W: N x K row-major -> [tile][k-group][lane][4]; lane (n = lane&31, half = lane>>5) holds k = 8*kg + 4*half + 0..3
void pack_frag(const std::vector<float>& W, int N, int K, float* out) {
    const int ntiles = (N + 31) / 32, nkg = K / 8;
    for (int t = 0; t < ntiles; ++t)
        for (int kg = 0; kg < nkg; ++kg)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = t * 32 + (lane & 31), k = 8 * kg + 4 * (lane >> 5);
                float* o = out + (((size_t)t * nkg + kg) * 64 + lane) * 4;
                for (int s = 0; s < 4; ++s) o[s] = n < N ? W[(size_t)n * K + k + s] : 0.f;
            }
}

struct WeightTable {
    std::unordered_map<std::string, const gvx_weight_desc*> map;
    const float* get(const std::string& name, int64_t numel, int* rc) const {
        auto it = map.find(name);
        if (it == map.end()) { *rc = fail(GVX_ERR_MISSING_WEIGHT, "missing weight '%s'", name.c_str()); return nullptr; }
        if (it->second->numel != numel) {
            *rc = fail(GVX_ERR_SHAPE, "weight '%s' has %lld elements, expected %lld", name.c_str(), (long long)it->second->numel, (long long)numel);
            return nullptr;
        }
        return it->second->data;
    }
};

// conv (+ eval BatchNorm) -> [Cout][k][Cin] with the BN scale folded in, bias' = (b - mean) * scale + beta
// u_out (optional, k = 5): the Winograd transform of the same folded weights, U[8][Cout][Cin] = G w (winograd_f45.h)
int pack_conv(const WeightTable& wt, const std::string& prefix, int cout, int cin, int k, float* w_out, float* b_out, float* u_out = nullptr) {
    int rc = GVX_OK;
    const float* w = wt.get(prefix + ".0.conv.weight", (int64_t)cout * cin * k, &rc); if (!w) return rc;
    const float* b = wt.get(prefix + ".0.conv.bias", cout, &rc); if (!b) return rc;
    const float* g = wt.get(prefix + ".1.weight", cout, &rc); if (!g) return rc;
    const float* beta = wt.get(prefix + ".1.bias", cout, &rc); if (!beta) return rc;
    const float* mu = wt.get(prefix + ".1.running_mean", cout, &rc); if (!mu) return rc;
    const float* var = wt.get(prefix + ".1.running_var", cout, &rc); if (!var) return rc;
    for (int co = 0; co < cout; ++co) {
        const double scale = (double)g[co] / std::sqrt((double)var[co] + BN_EPS);
        for (int kk = 0; kk < k; ++kk)
            for (int ci = 0; ci < cin; ++ci)
                w_out[((size_t)co * k + kk) * cin + ci] = (float)((double)w[((size_t)co * cin + ci) * k + kk] * scale);
        if (u_out)
            for (int ci = 0; ci < cin; ++ci)
                for (int s = 0; s < WINO_PTS; ++s)
                    u_out[((size_t)s * cout + co) * cin + ci] = wino_weight(w + ((size_t)co * cin + ci) * k, 1, scale, s);
        b_out[co] = (float)(((double)b[co] - (double)mu[co]) * scale + (double)beta[co]);
    }
    return GVX_OK;
}

// LSTM: rows permuted to row' = 4*j + gate, columns = [W_ih | W_hh], bias = b_ih + b_hh
int pack_lstm(const WeightTable& wt, const std::string& wih_name, const std::string& whh_name, const std::string& bih_name,
              const std::string& bhh_name, int Hd, int Kin, std::vector<float>* wcat, float* bias_out) {
    int rc = GVX_OK;
    const float* wih = wt.get(wih_name, (int64_t)4 * Hd * Kin, &rc); if (!wih) return rc;
    const float* whh = wt.get(whh_name, (int64_t)4 * Hd * Hd, &rc); if (!whh) return rc;
    const float* bih = wt.get(bih_name, 4 * Hd, &rc); if (!bih) return rc;
    const float* bhh = wt.get(bhh_name, 4 * Hd, &rc); if (!bhh) return rc;
    const int K = Kin + Hd;
    wcat->assign((size_t)4 * Hd * K, 0.f);
    for (int j = 0; j < Hd; ++j)
        for (int q = 0; q < 4; ++q) {
            const int src = q * Hd + j, dst = 4 * j + q;
            std::memcpy(&(*wcat)[(size_t)dst * K], wih + (size_t)src * Kin, sizeof(float) * Kin);
            std::memcpy(&(*wcat)[(size_t)dst * K + Kin], whh + (size_t)src * Hd, sizeof(float) * Hd);
            bias_out[dst] = bih[src] + bhh[src];
        }
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_model_pack_weights(gvx_model* m, const gvx_weight_desc* table, int n, void* host_blob) {
    if (!m || !table || !host_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    WeightTable wt;
    for (int i = 0; i < n; ++i) wt.map[table[i].name] = &table[i];
    const gvx_dims& d = m->d;
    const Blob& bl = m->blob;
    float* out = reinterpret_cast<float*>(host_blob);
    std::memset(out, 0, bl.total * sizeof(float));
    const int E = d.embed_dim, H = E / 2, M = d.n_mels, P = d.prenet_dim, A = d.att_rnn_dim, D = d.dec_rnn_dim, a = d.att_dim;
    int rc = GVX_OK;
    const float* src;

    if (!(src = wt.get("embedding.weight", (int64_t)d.n_tokens * E, &rc))) return rc;
    std::memcpy(out + bl.emb, src, sizeof(float) * d.n_tokens * E);

    for (int i = 0; i < d.enc_n_conv; ++i) {
        rc = pack_conv(wt, "encoder.convolutions." + std::to_string(i), E, E, d.enc_kernel, out + bl.enc_w[i], out + bl.enc_b[i],
                       encoder_layer_winograd_shape(d, i) ? out + bl.enc_u[i] : nullptr);
        if (rc != GVX_OK) return rc;
    }
    {   // encoder BiLSTM: input projection rows [dir][4*j+gate], recurrent part in fragment order
        const char* sfx[2] = {"", "_reverse"};
        for (int dir = 0; dir < 2; ++dir) {
            std::vector<float> wcat;
            std::vector<float> bias(4 * H);
            rc = pack_lstm(wt, std::string("encoder.lstm.weight_ih_l0") + sfx[dir], std::string("encoder.lstm.weight_hh_l0") + sfx[dir],
                           std::string("encoder.lstm.bias_ih_l0") + sfx[dir], std::string("encoder.lstm.bias_hh_l0") + sfx[dir], H, E, &wcat, bias.data());
            if (rc != GVX_OK) return rc;
            std::vector<float> whh((size_t)4 * H * H);
            for (int r = 0; r < 4 * H; ++r) {
                std::memcpy(out + bl.enc_wih + ((size_t)dir * 4 * H + r) * E, &wcat[(size_t)r * (E + H)], sizeof(float) * E);
                std::memcpy(&whh[(size_t)r * H], &wcat[(size_t)r * (E + H) + E], sizeof(float) * H);
            }
            std::memcpy(out + bl.enc_bih + (size_t)dir * 4 * H, bias.data(), sizeof(float) * 4 * H);
            pack_frag(whh, 4 * H, H, out + bl.enc_whh_frag[dir]);
        }
    }
    {   // Prenet (no bias)
        if (!(src = wt.get("decoder.prenet.layers.0.linear_layer.weight", (int64_t)P * M, &rc))) return rc;
        std::memcpy(out + bl.pre_w0, src, sizeof(float) * P * M);
        for (int j = 0; j < P; ++j)
            for (int k = 0; k < M; ++k) out[bl.pre_w0_t + (size_t)k * P + j] = src[(size_t)j * M + k];
        if (!(src = wt.get("decoder.prenet.layers.1.linear_layer.weight", (int64_t)P * P, &rc))) return rc;
        std::memcpy(out + bl.pre_w1, src, sizeof(float) * P * P);
        for (int j = 0; j < P; ++j)
            for (int k = 0; k < P; ++k) out[bl.pre_w1_t + (size_t)k * P + j] = src[(size_t)j * P + k];
    }
    {   // attention LSTM: x = [prenet ; context ; h_a]
        std::vector<float> wcat;
        rc = pack_lstm(wt, "decoder.attention_rnn.weight_ih", "decoder.attention_rnn.weight_hh", "decoder.attention_rnn.bias_ih",
                       "decoder.attention_rnn.bias_hh", A, P + E, &wcat, out + bl.att_bias);
        if (rc != GVX_OK) return rc;
        pack_frag(wcat, 4 * A, P + E + A, out + bl.att_frag);
        for (int n = 0; n < 4 * A; ++n) std::memcpy(out + bl.att_wpre + (size_t)n * P, &wcat[(size_t)n * (P + E + A)], sizeof(float) * P);
    }
    {   // attention layer
        const std::string att = "decoder.attention_layer.";
        if (!(src = wt.get(att + "query_layer.linear_layer.weight", (int64_t)a * A, &rc))) return rc;
        for (int t = 0; t < A / 8; ++t)
            for (int dd = 0; dd < a; ++dd)
                for (int jj = 0; jj < 8; ++jj) out[bl.wq_t + ((size_t)t * a + dd) * 8 + jj] = src[(size_t)dd * A + t * 8 + jj];
        if (!(src = wt.get(att + "memory_layer.linear_layer.weight", (int64_t)a * E, &rc))) return rc;
        std::memcpy(out + bl.wmem, src, sizeof(float) * a * E);
        if (!(src = wt.get(att + "v.linear_layer.weight", a, &rc))) return rc;
        std::memcpy(out + bl.v, src, sizeof(float) * a);
        const int64_t nconv = (int64_t)d.att_loc_filters * 2 * d.att_loc_kernel;
        if (!(src = wt.get(att + "location_layer.location_conv.conv.weight", nconv, &rc))) return rc;
        for (int c = 0; c < d.att_loc_filters; ++c)
            for (int ck = 0; ck < 2 * d.att_loc_kernel; ++ck) out[bl.loc_conv + (size_t)ck * 32 + c] = src[(size_t)c * 2 * d.att_loc_kernel + ck];
        if (!(src = wt.get(att + "location_layer.location_dense.linear_layer.weight", (int64_t)a * d.att_loc_filters, &rc))) return rc;
        for (int dd = 0; dd < a; ++dd)
            for (int c = 0; c < d.att_loc_filters; ++c) out[bl.loc_dense + ((size_t)(c >> 2) * a + dd) * 4 + (c & 3)] = src[(size_t)dd * d.att_loc_filters + c];
    }
    {   // decoder LSTM: x = [h_a ; context ; h_d]
        std::vector<float> wcat;
        rc = pack_lstm(wt, "decoder.decoder_rnn.weight_ih", "decoder.decoder_rnn.weight_hh", "decoder.decoder_rnn.bias_ih",
                       "decoder.decoder_rnn.bias_hh", D, A + E, &wcat, out + bl.dec_bias);
        if (rc != GVX_OK) return rc;
        pack_frag(wcat, 4 * D, A + E + D, out + bl.dec_frag);
    }
    {   // mel + gate projection, rows 0..M-1 = linear_projection, row M = gate_layer; x = [h_d ; context]
        const int K = D + E;
        std::vector<float> w((size_t)(M + 1) * K);
        if (!(src = wt.get("decoder.linear_projection.linear_layer.weight", (int64_t)M * K, &rc))) return rc;
        std::memcpy(w.data(), src, sizeof(float) * M * K);
        if (!(src = wt.get("decoder.gate_layer.linear_layer.weight", K, &rc))) return rc;
        std::memcpy(w.data() + (size_t)M * K, src, sizeof(float) * K);
        std::memcpy(out + bl.proj_w, w.data(), sizeof(float) * w.size());
        pack_frag(w, M + 1, K, out + bl.proj_frag);
        // autoregressive mode: the h_d columns tile-major [D/8][PSB][8] (rows past M are zero) for the partial products the
        // decoder-LSTM tiles emit, the context columns as their own fragment matrix
        const int PSBp = (M + 1 + 7) & ~7;
        for (int t = 0; t < D / 8; ++t)
            for (int n = 0; n < PSBp; ++n)
                for (int jj = 0; jj < 8; ++jj)
                    out[bl.proj_hd_t + ((size_t)t * PSBp + n) * 8 + jj] = n <= M ? w[(size_t)n * K + t * 8 + jj] : 0.f;
        std::vector<float> wc((size_t)(M + 1) * E);
        for (int n = 0; n <= M; ++n) std::memcpy(&wc[(size_t)n * E], &w[(size_t)n * K + D], sizeof(float) * E);
        pack_frag(wc, M + 1, E, out + bl.proj_ctx_frag);
        // ... and once more tile-major [E/4][PSB][4]: four context columns ride on the projection slab of each decoder-LSTM
        // tile (skinny.hip, extra slab terms) when the tile counts match (E / 4 == D / 8)
        for (int t = 0; t < E / 4; ++t)
            for (int n = 0; n < PSBp; ++n)
                for (int jj = 0; jj < 4; ++jj)
                    out[bl.proj_ctx_t + ((size_t)t * PSBp + n) * 4 + jj] = n <= M ? w[(size_t)n * K + D + t * 4 + jj] : 0.f;
        if (!(src = wt.get("decoder.linear_projection.linear_layer.bias", M, &rc))) return rc;
        std::memcpy(out + bl.proj_b, src, sizeof(float) * M);
        if (!(src = wt.get("decoder.gate_layer.linear_layer.bias", 1, &rc))) return rc;
        out[bl.proj_b + M] = src[0];
    }
    for (int i = 0; i < d.postnet_n_conv; ++i) {
        const int cin = i == 0 ? M : d.postnet_dim, cout = i == d.postnet_n_conv - 1 ? M : d.postnet_dim;
        rc = pack_conv(wt, "postnet.convolutions." + std::to_string(i), cout, cin, d.postnet_kernel, out + bl.post_w[i], out + bl.post_b[i],
                       postnet_layer_winograd_shape(d, i) ? out + bl.post_u[i] : nullptr);
        if (rc != GVX_OK) return rc;
    }
    return GVX_OK;
}

}  // extern "C"

namespace {

constexpr int PACK_MAX_TENSORS = 192;
struct PackSources { const float* p[PACK_MAX_TENSORS]; };

__global__ void pack_gather_kernel(PackSources src, const int32_t* off, const uint8_t* tid, long n, float* blob) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int t = tid[i];
        if (t == 255) continue;   // written by the fold / bias kernels below
        blob[i] = t ? src.p[t - 1][off[i]] : 0.f;
    }
}
// pack_conv on the device: [Cout][Cin][k] -> [Cout][k][Cin] with the eval-mode BatchNorm scale folded in (double, like the host);
// u_out (nullptr: none): the Winograd transform U[8][Cout][Cin] of the same weights, the host's expression (wino_weight)
__global__ void pack_conv_fold_kernel(const float* w, const float* b, const float* g, const float* beta, const float* mu, const float* var,
                                      int cout, int cin, int k, float* w_out, float* b_out, float* u_out) {
    const long n = (long)cout * cin * k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % cin), kk = (int)((i / cin) % k), co = (int)(i / ((long)cin * k));
        const double scale = (double)g[co] / sqrt((double)var[co] + BN_EPS);
        w_out[i] = (float)((double)w[((long)co * cin + ci) * k + kk] * scale);
        if (u_out && kk == 0)
            for (int s = 0; s < WINO_PTS; ++s) u_out[((long)s * cout + co) * cin + ci] = wino_weight(w + ((long)co * cin + ci) * k, 1, scale, s);
        if (ci == 0 && kk == 0) b_out[co] = (float)(((double)b[co] - (double)mu[co]) * scale + (double)beta[co]);
    }
}
// bias of an LSTM in packed row order: out[4 j + q] = b_ih[q H + j] + b_hh[q H + j]
__global__ void pack_lstm_bias_kernel(const float* bih, const float* bhh, int Hd, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * Hd) { const int j = i >> 2, q = i & 3; out[i] = bih[q * Hd + j] + bhh[q * Hd + j]; }
}

struct DevTable {
    std::unordered_map<std::string, int> idx;
    const gvx_weight_desc* t;
    const float* get(const std::string& name, int64_t numel, int* rc) const {
        auto it = idx.find(name);
        if (it == idx.end()) { *rc = fail(GVX_ERR_MISSING_WEIGHT, "missing weight '%s'", name.c_str()); return nullptr; }
        if (t[it->second].numel != numel) { *rc = fail(GVX_ERR_SHAPE, "weight '%s' has %lld elements, expected %lld", name.c_str(), (long long)t[it->second].numel, (long long)numel); return nullptr; }
        return t[it->second].data;
    }
};

// Build (or re-use) the gather map of `table`'s layout.  Two runs of the host packer over stand-ins whose floats carry the
// low / high 12 bits of their own index tell where each blob float comes from; the regions the packer COMPUTES (BatchNorm
// folds, bias sums) are marked 255 and written by their own kernels.
int ensure_gather_map(gvx_model* m, const gvx_weight_desc* table, int n) {
    bool same = m->gather_off && (int)m->gather_names.size() == n;
    for (int i = 0; same && i < n; ++i) same = m->gather_names[i] == table[i].name && m->gather_numel[i] == table[i].numel;
    if (same) return GVX_OK;
    if (n > PACK_MAX_TENSORS || n > 254) return fail(GVX_ERR_UNSUPPORTED, "pack_weights_device: more than %d tensors", 254);
    const size_t total = m->blob.total;
    std::vector<std::vector<float>> lo(n), hi(n);
    std::vector<gvx_weight_desc> tl(n), th(n);
    for (int i = 0; i < n; ++i) {
        if (table[i].numel < 0 || table[i].numel >= (int64_t)1 << 31) return fail(GVX_ERR_UNSUPPORTED, "pack_weights_device: tensor too large");
        lo[i].resize((size_t)table[i].numel); hi[i].resize((size_t)table[i].numel);
        for (int64_t e = 0; e < table[i].numel; ++e) { lo[i][e] = (float)((e & 4095) + 1); hi[i][e] = (float)((e >> 12) * 256 + i + 1); }
        tl[i] = gvx_weight_desc{table[i].name, lo[i].data(), table[i].numel};
        th[i] = gvx_weight_desc{table[i].name, hi[i].data(), table[i].numel};
    }
    std::vector<float> bl(total), bh(total);
    int rc = gvx_model_pack_weights(m, tl.data(), n, bl.data());
    if (rc != GVX_OK) return rc;
    rc = gvx_model_pack_weights(m, th.data(), n, bh.data());
    if (rc != GVX_OK) return rc;
    std::vector<int32_t> off(total);
    std::vector<uint8_t> tid(total);
    for (size_t i = 0; i < total; ++i) {
        if (bl[i] == 0.f && bh[i] == 0.f) { off[i] = 0; tid[i] = 0; continue; }
        const long h = (long)bh[i] - 1, l = (long)bl[i] - 1;
        const int t = (int)(h % 256);
        off[i] = (int32_t)((h / 256) * 4096 + l);
        tid[i] = (uint8_t)(t + 1);
    }
    // computed regions
    const gvx_dims& d = m->d;
    const Blob& b = m->blob;
    auto mark = [&](size_t o, size_t cnt) { std::fill(tid.begin() + o, tid.begin() + o + cnt, (uint8_t)255); };
    const int E = d.embed_dim, H = E / 2, M = d.n_mels;
    for (int i = 0; i < d.enc_n_conv; ++i) {
        mark(b.enc_w[i], (size_t)E * d.enc_kernel * E); mark(b.enc_b[i], E);
        if (encoder_layer_winograd_shape(d, i)) mark(b.enc_u[i], (size_t)WINO_PTS * E * E);
    }
    for (int i = 0; i < d.postnet_n_conv; ++i) {
        const int cin = i == 0 ? M : d.postnet_dim, cout = i == d.postnet_n_conv - 1 ? M : d.postnet_dim;
        mark(b.post_w[i], (size_t)cout * d.postnet_kernel * cin); mark(b.post_b[i], cout);
        if (postnet_layer_winograd_shape(d, i)) mark(b.post_u[i], (size_t)WINO_PTS * cout * cin);
    }
    mark(b.enc_bih, (size_t)8 * H); mark(b.att_bias, (size_t)4 * d.att_rnn_dim); mark(b.dec_bias, (size_t)4 * d.dec_rnn_dim);
    // sanity: every gathered float points inside its tensor
    for (size_t i = 0; i < total; ++i)
        if (tid[i] && tid[i] != 255 && (tid[i] > n || off[i] < 0 || off[i] >= table[tid[i] - 1].numel))
            return fail(GVX_ERR_UNSUPPORTED, "pack_weights_device: gather map is inconsistent at blob float %zu", i);
    if (m->gather_off) { (void)hipFree(m->gather_off); m->gather_off = nullptr; }
    if (m->gather_tid) { (void)hipFree(m->gather_tid); m->gather_tid = nullptr; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->gather_off), total * sizeof(int32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m->gather_tid), total));
    HIP_TRY(hipMemcpy(m->gather_off, off.data(), total * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->gather_tid, tid.data(), total, hipMemcpyHostToDevice));
    m->gather_names.clear(); m->gather_numel.clear();
    for (int i = 0; i < n; ++i) { m->gather_names.push_back(table[i].name); m->gather_numel.push_back(table[i].numel); }
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_model_pack_weights_device(gvx_model* m, const gvx_weight_desc* table, int n, void* device_blob, void* stream) {
    if (!m || !table || !device_blob || n < 1) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(device_blob) & 255) return fail(GVX_ERR_INVALID_ARG, "blob must be 256-byte aligned");
    int rc = ensure_gather_map(m, table, n);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* out = reinterpret_cast<float*>(device_blob);
    PackSources src{};
    for (int i = 0; i < n; ++i) src.p[i] = table[i].data;
    const long total = (long)m->blob.total;
    hipLaunchKernelGGL(pack_gather_kernel, dim3(4096), dim3(256), 0, s, src, m->gather_off, m->gather_tid, total, out);
    DevTable dt; dt.t = table;
    for (int i = 0; i < n; ++i) dt.idx[table[i].name] = i;
    const gvx_dims& d = m->d;
    const Blob& bl = m->blob;
    const int E = d.embed_dim, H = E / 2, M = d.n_mels;
    auto conv = [&](const std::string& prefix, int cout, int cin, int k, size_t w_off, size_t b_off, const size_t* u_off = nullptr) -> int {
        int r = GVX_OK;
        const float* w = dt.get(prefix + ".0.conv.weight", (int64_t)cout * cin * k, &r); if (!w) return r;
        const float* b = dt.get(prefix + ".0.conv.bias", cout, &r); if (!b) return r;
        const float* g = dt.get(prefix + ".1.weight", cout, &r); if (!g) return r;
        const float* beta = dt.get(prefix + ".1.bias", cout, &r); if (!beta) return r;
        const float* mu = dt.get(prefix + ".1.running_mean", cout, &r); if (!mu) return r;
        const float* var = dt.get(prefix + ".1.running_var", cout, &r); if (!var) return r;
        const long cnt = (long)cout * cin * k;
        hipLaunchKernelGGL(pack_conv_fold_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, w, b, g, beta, mu, var, cout, cin, k, out + w_off, out + b_off,
                           u_off ? out + *u_off : (float*)nullptr);
        return GVX_OK;
    };
    for (int i = 0; i < d.enc_n_conv; ++i)
        if ((rc = conv("encoder.convolutions." + std::to_string(i), E, E, d.enc_kernel, bl.enc_w[i], bl.enc_b[i],
                       encoder_layer_winograd_shape(d, i) ? &bl.enc_u[i] : nullptr)) != GVX_OK) return rc;
    for (int i = 0; i < d.postnet_n_conv; ++i) {
        const int cin = i == 0 ? M : d.postnet_dim, cout = i == d.postnet_n_conv - 1 ? M : d.postnet_dim;
        if ((rc = conv("postnet.convolutions." + std::to_string(i), cout, cin, d.postnet_kernel, bl.post_w[i], bl.post_b[i],
                       postnet_layer_winograd_shape(d, i) ? &bl.post_u[i] : nullptr)) != GVX_OK) return rc;
    }
    auto bias = [&](const std::string& bih_n, const std::string& bhh_n, int Hd, size_t o) -> int {
        int r = GVX_OK;
        const float* bih = dt.get(bih_n, 4 * Hd, &r); if (!bih) return r;
        const float* bhh = dt.get(bhh_n, 4 * Hd, &r); if (!bhh) return r;
        hipLaunchKernelGGL(pack_lstm_bias_kernel, dim3((4 * Hd + 255) / 256), dim3(256), 0, s, bih, bhh, Hd, out + o);
        return GVX_OK;
    };
    if ((rc = bias("encoder.lstm.bias_ih_l0", "encoder.lstm.bias_hh_l0", H, bl.enc_bih)) != GVX_OK) return rc;
    if ((rc = bias("encoder.lstm.bias_ih_l0_reverse", "encoder.lstm.bias_hh_l0_reverse", H, bl.enc_bih + (size_t)4 * H)) != GVX_OK) return rc;
    if ((rc = bias("decoder.attention_rnn.bias_ih", "decoder.attention_rnn.bias_hh", d.att_rnn_dim, bl.att_bias)) != GVX_OK) return rc;
    if ((rc = bias("decoder.decoder_rnn.bias_ih", "decoder.decoder_rnn.bias_hh", d.dec_rnn_dim, bl.dec_bias)) != GVX_OK) return rc;
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // extern "C"
