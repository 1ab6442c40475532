// torchMoji feature encoder (include/cookietts_hip.h, "torchMoji feature encoder"): the style input of the T2S server
// (utils/torchmoji/model_def.py:169-253 with feature_output=True).  tanh-embedding gather, two packed bidirectional LSTMs with
// hard-sigmoid gates (ctts_lstm_biseq_hardsig_f32, tacotron_decoder.hip) and the attention pooling (attlayer.py:38-68).
// Everything here is glue around the 2 T dependent LSTM step launches: the path is launch-latency-bound, not arithmetic-bound.
#include "tacotron_plan.h"

namespace ctts {
namespace {

using taco::align_up;
using taco::MAX_BATCH;

constexpr int TM_PAD = 8;          // halo columns of the channel-major inputs of the two input-projection GEMMs
constexpr int TM_MAX_T = 8192;     // the pooling kernel keeps one row's logits in LDS (32 KiB)
constexpr int TM_TT = 32, TM_TC = 64;

inline int tm_ld(int T) { return (T + 127) / 128 * 128 + 2 * TM_PAD; }

// len[b] = index of the last non-zero token of row b, plus one (model_def.py:193); 0 for an all-zero row
__global__ __launch_bounds__(256) void tm_lengths_kernel(const long long* __restrict__ tokens, int* __restrict__ lengths, int T) {
    __shared__ int red[4];
    const int b = blockIdx.x;
    int m = 0;
    for (int t = threadIdx.x; t < T; t += 256)
        if (tokens[(size_t)b * T + t] != 0) m = max(m, t + 1);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) lengths[b] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// One tile of TM_TT padded columns x TM_TC channels, already in `tile` [TM_TT][TM_TC + 1] -> x[b][c0 + cc][col0 + tt]
__device__ __forceinline__ void tm_store_channel_major(const float (*tile)[TM_TC + 1], float* __restrict__ x, int b, int C, int c0,
                                                        int col0, int ld) {
    for (int i = threadIdx.x; i < TM_TT * TM_TC; i += 256) {
        const int cc = i / TM_TT, tt = i % TM_TT;
        const int c = c0 + cc, col = col0 + tt;
        if (c < C && col < ld) x[((size_t)b * C + c) * ld + col] = tile[tt][cc];
    }
}

// v = tanh(embed[tok[b][t]][c]) for t < len[b], else 0 (model_def.py:209-210), written twice:
//   x0[b][c][pad + t]         every column of the padded row (zeros outside [pad, pad + len))
//   feat[b][t][fcol + c]      t < T
// The gather index is clamped to the table: a token outside [0, V) never reads outside it.
__global__ __launch_bounds__(256) void tm_embed_kernel(const float* __restrict__ emb, const long long* __restrict__ tokens,
                                                       const int* __restrict__ lengths, float* __restrict__ x0,
                                                       float* __restrict__ feat, int T, int V, int E, int F, int fcol, int ld, int pad) {
    __shared__ float tile[TM_TT][TM_TC + 1];
    const int col0 = blockIdx.x * TM_TT, c0 = blockIdx.y * TM_TC, b = blockIdx.z;
    const int len = min(max(lengths[b], 0), T);
    for (int i = threadIdx.x; i < TM_TT * TM_TC; i += 256) {
        const int tt = i / TM_TC, cc = i % TM_TC;
        const int c = c0 + cc, t = col0 + tt - pad;
        float v = 0.f;
        if (c < E && t >= 0 && t < T) {
            if (t < len) {
                long long tok = tokens[(size_t)b * T + t];
                tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;
                v = tanhf(emb[(size_t)tok * E + c]);
            }
            feat[((size_t)b * T + t) * F + fcol + c] = v;
        }
        tile[tt][cc] = v;
    }
    __syncthreads();
    tm_store_channel_major(tile, x0, b, E, c0, col0, ld);
}

// Layer hand-over: x1[b][c][pad + t] = t < len[b] ? feat[b][t][fcol + c] : 0, every column of the padded row
__global__ __launch_bounds__(256) void tm_handover_kernel(const float* __restrict__ feat, const int* __restrict__ lengths,
                                                          float* __restrict__ x1, int T, int C, int F, int fcol, int ld, int pad) {
    __shared__ float tile[TM_TT][TM_TC + 1];
    const int col0 = blockIdx.x * TM_TT, c0 = blockIdx.y * TM_TC, b = blockIdx.z;
    const int len = min(max(lengths[b], 0), T);
    for (int i = threadIdx.x; i < TM_TT * TM_TC; i += 256) {
        const int tt = i / TM_TC, cc = i % TM_TC;
        const int c = c0 + cc, t = col0 + tt - pad;
        tile[tt][cc] = (c < C && t >= 0 && t < len) ? feat[((size_t)b * T + t) * F + fcol + c] : 0.f;
    }
    __syncthreads();
    tm_store_channel_major(tile, x1, b, C, c0, col0, ld);
}

// attlayer.py:48-66 for row b = blockIdx.x and output columns [256 blockIdx.y, +256): logits of the row's valid steps (every
// workgroup of a row forms them, in the same order), M = the row's own maximum, w = exp(logit - M), a = w / sum w,
// out[b][d] = sum_t a[t] feat[b][t][d].  len == 0: zeros, no division.
__global__ __launch_bounds__(256) void tm_pool_kernel(const float* __restrict__ feat, const float* __restrict__ vec,
                                                      const int* __restrict__ lengths, float* __restrict__ out,
                                                      float* __restrict__ att, int T, int D) {
    extern __shared__ __attribute__((aligned(16))) float lg[];      // [T]
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = min(max(lengths[b], 0), T);
    const float* fb = feat + (size_t)b * T * D;
    for (int t = wave; t < len; t += 4) {
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) acc = fmaf(fb[(size_t)t * D + d], vec[d], acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) lg[t] = acc;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int t = 0; t < len; ++t) m = fmaxf(m, lg[t]);
    __syncthreads();
    for (int t = threadIdx.x; t < len; t += 256) lg[t] = expf(lg[t] - m);
    __syncthreads();
    float sum = 0.f;
    for (int t = 0; t < len; ++t) sum += lg[t];
    const int d = blockIdx.y * 256 + threadIdx.x;
    if (d < D) {
        float acc = 0.f;
        for (int t = 0; t < len; ++t) acc = fmaf(lg[t] / sum, fb[(size_t)t * D + d], acc);
        out[(size_t)b * D + d] = acc;
    }
    if (att && blockIdx.y == 0)
        for (int t = threadIdx.x; t < T; t += 256) att[(size_t)b * T + t] = t < len ? lg[t] / sum : 0.f;
}

struct TmPlan { int V, E, H, F; size_t embed, vec, lstm[2][2], total; };

int make_tm_plan(const ctts_torchmoji_config* cfg, TmPlan& p) {
    CTTS_CHECK_ARG(cfg != nullptr, "torchmoji: config is NULL");
    CTTS_CHECK_ARG(cfg->nb_tokens >= 1, "torchmoji: nb_tokens=%d", cfg->nb_tokens);
    CTTS_CHECK_ARG(cfg->embedding_dim >= 16 && cfg->embedding_dim % 16 == 0, "torchmoji: embedding_dim=%d (a multiple of 16)",
                   cfg->embedding_dim);
    CTTS_CHECK_ARG(cfg->hidden_size >= 64 && cfg->hidden_size % 64 == 0, "torchmoji: hidden_size=%d (a multiple of 64)",
                   cfg->hidden_size);
    p.V = cfg->nb_tokens; p.E = cfg->embedding_dim; p.H = cfg->hidden_size; p.F = 4 * p.H + p.E;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n); return r; };
    p.embed = take((size_t)p.V * p.E);
    p.vec = take(p.F);
    for (int l = 0; l < 2; ++l)
        for (int k = 0; k < 2; ++k) {
            const size_t n = ctts_lstm_seq_packed_bytes(l ? 2 * p.H : p.E, p.H) / sizeof(float);
            if (!n) return CTTS_E_ARG;
            p.lstm[l][k] = take(n);
        }
    p.total = o;
    return CTTS_OK;
}

struct TmWs { float *x0, *x1, *feat, *hn, *seq[2]; size_t seq_bytes, total; };

int tm_carve(const TmPlan& p, int batch, int T, float* base, TmWs& w) {
    CTTS_CHECK_ARG(batch >= 1 && batch <= MAX_BATCH, "torchmoji: batch=%d (1..%d)", batch, MAX_BATCH);
    CTTS_CHECK_ARG(T >= 1 && T <= TM_MAX_T, "torchmoji: T=%d (1..%d)", T, TM_MAX_T);
    const int ld = tm_ld(T);
    w.seq_bytes = ctts_lstm_seq_workspace_bytes(p.H, batch, ld);
    CTTS_CHECK_ARG(w.seq_bytes > 0, "torchmoji: no packed-sequence LSTM form for hidden_size=%d batch=%d", p.H, batch);
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n); return base ? base + r : nullptr; };
    w.x0 = take((size_t)batch * p.E * ld);
    w.x1 = take((size_t)batch * 2 * p.H * ld);
    w.feat = take((size_t)batch * T * p.F);
    w.hn = take((size_t)batch * 2 * p.H);
    w.seq[0] = take(w.seq_bytes / sizeof(float));
    w.seq[1] = take(w.seq_bytes / sizeof(float));
    w.total = o;
    return CTTS_OK;
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

int ctts_attention_pool_f32(const float* feat, const float* vector, const int32_t* lengths, float* out, float* att, int32_t batch,
                            int32_t T, int32_t D, void* stream) {
    CTTS_CHECK_ARG(feat && vector && lengths && out, "attention_pool: NULL pointer");
    CTTS_CHECK_ARG(batch >= 1 && batch <= 65535 && T >= 1 && T <= TM_MAX_T && D >= 1, "attention_pool: batch=%d T=%d (1..%d) D=%d",
                   batch, T, TM_MAX_T, D);
    hipLaunchKernelGGL(tm_pool_kernel, dim3(batch, (D + 255) / 256), dim3(256), (size_t)T * sizeof(float), as_stream(stream), feat,
                       vector, lengths, out, att, T, D);
    CTTS_CHECK_LAUNCH("attention_pool");
    return CTTS_OK;
}

size_t ctts_torchmoji_packed_bytes(const ctts_torchmoji_config* cfg) {
    TmPlan p;
    if (make_tm_plan(cfg, p)) return 0;
    return p.total * sizeof(float);
}

int ctts_torchmoji_pack_f32(const ctts_torchmoji_config* cfg, const ctts_torchmoji_weights* w, void* packed, void* stream) {
    TmPlan p;
    int rc = make_tm_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(w && w->embed && w->attention_vector && packed, "torchmoji_pack: NULL pointer");
    hipStream_t s = as_stream(stream);
    float* blob = static_cast<float*>(packed);
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + p.embed, w->embed, (size_t)p.V * p.E * sizeof(float), hipMemcpyDeviceToDevice, s));
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + p.vec, w->attention_vector, (size_t)p.F * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int l = 0; l < 2; ++l)
        for (int k = 0; k < 2; ++k)
            if ((rc = ctts_lstm_seq_pack_f32(&w->lstm[l][k], l ? 2 * p.H : p.E, p.H, blob + p.lstm[l][k], stream))) return rc;
    return CTTS_OK;
}

size_t ctts_torchmoji_workspace_bytes(const ctts_torchmoji_config* cfg, int32_t batch, int32_t T) {
    TmPlan p; TmWs w;
    if (make_tm_plan(cfg, p) || tm_carve(p, batch, T, nullptr, w)) return 0;
    return w.total * sizeof(float);
}

int ctts_torchmoji_lengths(const int64_t* tokens, int32_t* lengths, int32_t batch, int32_t T, void* stream) {
    CTTS_CHECK_ARG(tokens && lengths && batch >= 1 && T >= 1, "torchmoji_lengths: bad argument");
    hipLaunchKernelGGL(tm_lengths_kernel, dim3(batch), dim3(256), 0, as_stream(stream), reinterpret_cast<const long long*>(tokens),
                       lengths, T);
    CTTS_CHECK_LAUNCH("torchmoji_lengths");
    return CTTS_OK;
}

int ctts_torchmoji_features_f32(const ctts_torchmoji_config* cfg, const void* packed, const int64_t* tokens, const int32_t* lengths,
                                float* features, float* attention, int32_t batch, int32_t T, void* workspace,
                                size_t workspace_bytes, void* stream) {
    TmPlan p; TmWs w;
    int rc = make_tm_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(packed && tokens && lengths && features && workspace, "torchmoji_features: NULL pointer");
    if ((rc = tm_carve(p, batch, T, static_cast<float*>(workspace), w))) return rc;
    if (w.total * sizeof(float) > workspace_bytes) {
        set_error("torchmoji_features: workspace %zu bytes < required %zu", workspace_bytes, w.total * sizeof(float));
        return CTTS_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    const float* blob = static_cast<const float*>(packed);
    const int H = p.H, E = p.E, F = p.F, ld = tm_ld(T);
    const int ctiles = (ld + TM_TT - 1) / TM_TT;
    // the LSTMs write only t < len[b]: the feature columns they own are zero beyond it
    CTTS_CHECK_HIP(hipMemsetAsync(w.feat, 0, (size_t)batch * T * F * sizeof(float), s));
    hipLaunchKernelGGL(tm_embed_kernel, dim3(ctiles, (E + TM_TC - 1) / TM_TC, batch), dim3(256), 0, s, blob + p.embed,
                       reinterpret_cast<const long long*>(tokens), lengths, w.x0, w.feat, T, p.V, E, F, 4 * H, ld, TM_PAD);
    CTTS_CHECK_LAUNCH("torchmoji_embed");
    // lstm_0 -> feature columns [2H, 4H)
    rc = ctts_lstm_biseq_hardsig_f32(blob + p.lstm[0][0], blob + p.lstm[0][1], w.x0, lengths, w.feat, (int64_t)T * F, F, 2 * H, 3 * H,
                                     w.hn, 2 * H, 0, H, batch, T, E, H, ld, TM_PAD, w.seq[0], w.seq[1], w.seq_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tm_handover_kernel, dim3(ctiles, (2 * H + TM_TC - 1) / TM_TC, batch), dim3(256), 0, s, w.feat, lengths, w.x1,
                       T, 2 * H, F, 2 * H, ld, TM_PAD);
    CTTS_CHECK_LAUNCH("torchmoji_handover");
    // lstm_1 -> feature columns [0, 2H)
    rc = ctts_lstm_biseq_hardsig_f32(blob + p.lstm[1][0], blob + p.lstm[1][1], w.x1, lengths, w.feat, (int64_t)T * F, F, 0, H, w.hn,
                                     2 * H, 0, H, batch, T, 2 * H, H, ld, TM_PAD, w.seq[0], w.seq[1], w.seq_bytes, stream);
    if (rc) return rc;
    return ctts_attention_pool_f32(w.feat, blob + p.vec, lengths, features, attention, batch, T, F, stream);
}

}  // extern "C"
