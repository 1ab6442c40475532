// Tacotron2Loss on the device (_2_ttm/tacotron2_tm/loss_function.py:96-290, no gradient): the validation loss, the per-file
// score table and the inference-style attention score of one teacher-forced pass.  The reference builds the guided-attention
// mask per item in a Python loop on the host (:57-72), makes three masked_select copies of the mels, and reads six .item()
// per row.  Here every per-item number lands in one fp64 table [B][CTTS_TACO_LOSS_COLUMNS] that the host reads once.
//
//   taco_lengths_kernel   grid (B): lengths as fp32 for the metric kernels; the predicted length of :266-269      latency-bound
//   taco_mel_gate_kernel  grid (64-frame tiles, B): a lane owns a frame column, the four waves split the mel
//                         rows and meet in LDS in wave order; five fp64 partials per tile                        memory-bound
//   taco_guided_kernel    grid (32-frame blocks, B): a lane owns encoder columns; the weight of :72 is formed
//                         on the fly, no mask tensor exists; one fp64 partial per block                          memory-bound
//   (the two alignment metrics: csrc/alignment.hip, the second with its validity cut)
//   taco_finalize_kernel  ONE workgroup: tile partials in tile order into the item's row, the score of :276-283
//                         in IEEE double, then every batch term as a sum over items in item order                latency-bound
//
// No kernel waits on another workgroup, no float atomics: every sum has a fixed order and repeats bit for bit.  The score must
// follow Python's arithmetic, so nothing in this file may be contracted into a fused multiply-add (the pragma below; build.py
// adds -ffp-contract=off).
#include "common.h"

#pragma clang fp contract(off)

namespace ctts {
namespace {

constexpr int TL_TILE = 64;                      // frames per mel/gate workgroup: one per lane
constexpr int TL_ROWS = 32;                      // frames per guided-attention workgroup (8 per wave)
constexpr int TL_PART = 5;                       // partials per mel/gate tile
constexpr int TL_K = CTTS_TACO_LOSS_COLUMNS;
constexpr int TL_TERMS = CTTS_TACO_LOSS_TERMS;

// the sections of a workspace
struct LossView {
    float *ilen_f, *olen_f, *plen_f;             // [B] each: text, mel and predicted lengths as the metric kernels read them
    int32_t* plen_i;                             // [B]
    double* mel_part;                            // [B][tiles][TL_PART]
    double* att_part;                            // [B][blocks]
    double *metric_gt, *metric_pred;             // [B][6] each
    void* align_ws;                              // ctts_alignment_workspace_bytes(B, T, enc), shared by the two metric calls
    size_t align_bytes;
    int tiles, blocks;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

size_t loss_layout(int B, int n_mel, int T, int enc, void* ws, LossView* v) {
    if (B < 1 || n_mel < 1 || T < 1 || enc < 1) {
        set_error("taco_loss: batch %d, n_mel %d, T %d, enc %d must all be positive", B, n_mel, T, enc);
        return 0;
    }
    char* base = static_cast<char*>(ws);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = up16(off + bytes); return p; };
    LossView w;
    w.tiles = (T + TL_TILE - 1) / TL_TILE;
    w.blocks = (T + TL_ROWS - 1) / TL_ROWS;
    w.ilen_f = reinterpret_cast<float*>(take((size_t)B * 4));
    w.olen_f = reinterpret_cast<float*>(take((size_t)B * 4));
    w.plen_f = reinterpret_cast<float*>(take((size_t)B * 4));
    w.plen_i = reinterpret_cast<int32_t*>(take((size_t)B * 4));
    w.mel_part = reinterpret_cast<double*>(take((size_t)B * w.tiles * TL_PART * 8));
    w.att_part = reinterpret_cast<double*>(take((size_t)B * w.blocks * 8));
    w.metric_gt = reinterpret_cast<double*>(take((size_t)B * 6 * 8));
    w.metric_pred = reinterpret_cast<double*>(take((size_t)B * 6 * 8));
    w.align_bytes = ctts_alignment_workspace_bytes(B, T, enc);
    w.align_ws = take(w.align_bytes);
    if (v) *v = w;
    return off;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- lengths ------------------------------------------------------------------------------------------------------
// :266-269: sigmoid, the first five frames zeroed, then get_first_over_thresh(., 0.7) (utils.py:47-56): the last frame always
// qualifies.  The sigmoid is float32, as the reference's (get_first_over_thresh casts to float whatever it is handed).
__global__ __launch_bounds__(256) void taco_lengths_kernel(const float* __restrict__ gate, const int32_t* __restrict__ mel_len,
                                                           const int32_t* __restrict__ text_len, LossView v, int T, int enc) {
    __shared__ int red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    int first = T - 1;
    for (int i = 5 + t; i < T - 1; i += 256)
        if (1.0f / (1.0f + expf(-gate[(size_t)b * T + i])) >= 0.7f) { first = i; break; }   // ascending i per thread: its first hit
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if ((t & 63) == 0) red[t >> 6] = first;
    __syncthreads();
    if (t == 0) {
        const int p = min(min(red[0], red[1]), min(red[2], red[3]));
        v.plen_i[b] = p;
        v.plen_f[b] = (float)p;
        v.ilen_f[b] = (float)min(text_len[b], enc);          // a length beyond the tensor reads as the tensor's size, everywhere
        v.olen_f[b] = (float)min(mel_len[b], T);
    }
}

// ---- mel and gate pass --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void taco_mel_gate_kernel(const float* __restrict__ pred, const float* __restrict__ post,
                                                            const float* __restrict__ gt, const float* __restrict__ gate,
                                                            const float* __restrict__ target,
                                                            const int32_t* __restrict__ mel_len, double* __restrict__ part,
                                                            int n_mel, int T, int tiles, double pos_weight) {
    __shared__ double s[4][4][TL_TILE];          // [quantity][wave][frame]
    const int b = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = tile * TL_TILE + lane;
    const bool live = t < T && t < mel_len[b];
    double se0 = 0.0, se1 = 0.0, a0 = 0.0, a1 = 0.0;
    if (live) {
        const size_t base = (size_t)b * n_mel * T + t;
        for (int m = wave; m < n_mel; m += 4) {              // a mel row: 64 consecutive floats per wave
            const size_t i = base + (size_t)m * T;
            const double g = (double)gt[i];
            const double d0 = (double)pred[i] - g, d1 = (double)post[i] - g;
            se0 += d0 * d0; se1 += d1 * d1;
            a0 += fabs(d0); a1 += fabs(d1);
        }
    }
    s[0][wave][lane] = se0; s[1][wave][lane] = se1; s[2][wave][lane] = a0; s[3][wave][lane] = a1;
    __syncthreads();
    if (wave != 0) return;
    double q[TL_PART];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = ((s[k][0][lane] + s[k][1][lane]) + s[k][2][lane]) + s[k][3][lane];   // wave order
    q[2] = q[2] * (q[2] / (double)n_mel);                    // :209: sum_m |d_m| * mean_m |d_m|
    q[3] = q[3] * (q[3] / (double)n_mel);
    q[4] = 0.0;
    if (t < T) {                                             // :216-218: the whole [B, T], not masked by length
        const double x = (double)gate[(size_t)b * T + t], y = (double)target[(size_t)b * T + t];
        const double log_weight = (pos_weight - 1.0) * y + 1.0;
        q[4] = (1.0 - y) * x + log_weight * (log1p(exp(-fabs(x))) + (x < 0.0 ? -x : 0.0));   // the overflow-safe form
    }
#pragma unroll
    for (int k = 0; k < TL_PART; ++k) q[k] = wave_sum_f64(q[k]);
    if (lane == 0) {
        double* o = part + ((size_t)b * tiles + tile) * TL_PART;
#pragma unroll
        for (int k = 0; k < TL_PART; ++k) o[k] = q[k];
    }
}

// ---- guided attention (:37-72, :234-241) -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void taco_guided_kernel(const float* __restrict__ al, const int32_t* __restrict__ mel_len,
                                                          const int32_t* __restrict__ text_len,
                                                          const float* __restrict__ pres, double* __restrict__ part, int T,
                                                          int enc, int blocks, double sigma) {
    __shared__ double red[4];
    const int b = blockIdx.y, blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int olen = min(mel_len[b], T), ilen = min(text_len[b], enc);
    double acc = 0.0;
    if (pres[b] == 0.0f) {                                   // :239-241: items that carry decoder state contribute nothing
        const double two_s2 = 2.0 * (sigma * sigma);
        for (int r = wave; r < TL_ROWS; r += 4) {
            const int t = blk * TL_ROWS + r;
            if (t >= olen) break;
            const float* row = al + ((size_t)b * T + t) * enc;
            const double ty = (double)t / (double)olen;
            for (int e = lane; e < ilen; e += 64) {
                const double d = (double)e / (double)ilen - ty;
                acc += (1.0 - exp(-(d * d) / two_s2)) * (double)row[e];
            }
        }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)b * blocks + blk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- finalize -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }   // Python's max(a, b): a NaN a stays

struct FinalArgs {
    const double *metric_gt, *metric_pred;
    const float *mu, *logvar, *pred_sylps, *gt_sylps, *pres;
    const int32_t *mel_len, *text_len;
    int B, n_mel, T, enc;
};

__global__ __launch_bounds__(256) void taco_finalize_kernel(ctts_taco_loss_params p, LossView v, FinalArgs a, double* table,
                                                            double* __restrict__ terms) {
    __shared__ int s_red[4];
    __shared__ double s_sum[TL_K];
    __shared__ double s_fill;
    const int t = threadIdx.x, B = a.B;
    // max(mel_lengths): the one batch quantity the score reads (:281)
    int mx = 0;
    for (int b = t; b < B; b += 256) mx = max(mx, min(a.mel_len[b], a.T));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if ((t & 63) == 0) s_red[t >> 6] = mx;
    __syncthreads();
    mx = max(max(s_red[0], s_red[1]), max(s_red[2], s_red[3]));

    for (int b = t; b < B; b += 256) {
        double* row = table + (size_t)b * TL_K;
        double q[TL_PART] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < v.tiles; ++k)                     // tile order
            for (int j = 0; j < TL_PART; ++j) q[j] += v.mel_part[((size_t)b * v.tiles + k) * TL_PART + j];
        double att = 0.0;
        for (int k = 0; k < v.blocks; ++k) att += v.att_part[(size_t)b * v.blocks + k];
        const int mlen = min(a.mel_len[b], a.T), tlen = min(a.text_len[b], a.enc);   // as the mel, guided and metric passes read them
        const double len = (double)mlen;
        const bool fresh = a.pres[b] == 0.0f;
        row[0] = len;
        for (int j = 0; j < TL_PART; ++j) row[1 + j] = q[j];
        row[6] = fresh ? att : 0.0;
        row[7] = fresh ? len : 0.0;
        const double m = (double)a.mu[b], lv = (double)a.logvar[b];
        row[8] = ((1.0 + lv) - exp(lv)) - m * m;             // :224
        const double ds = (double)a.pred_sylps[b] - (double)a.gt_sylps[b];
        row[9] = fabs(ds);
        row[10] = ds * ds;
        const double* m1 = a.metric_gt + (size_t)b * 6;
        const double* m2 = a.metric_pred + (size_t)b * 6;
        for (int j = 0; j < 6; ++j) { row[11 + j] = m1[j]; row[18 + j] = m2[j]; }
        row[17] = (double)v.plen_i[b];
        // :276-283; columns 1-5 of a metric row are float32 in the reference, .item() widens them
        const double diag = m2[0], avg_prob = (double)(float)m2[1], emax = (double)(float)m2[2], emin = (double)(float)m2[3];
        const double eavg = (double)(float)m2[4], pmiss = (double)(float)m2[5];
        double w = avg_prob;
        const double p1 = py_max(diag - 1.10, 0.0) * 0.25;
        const double p2 = py_max(emax - 60.0, 0.0) * 0.005;
        const double p3 = py_max(0.00 - emin, 0.0) * 0.5;
        const double p4 = py_max(3.60 - eavg, 0.0);
        const bool cond = tlen > 12 && (double)mlen < (double)mx * 0.75;
        const double p5 = cond ? py_max(pmiss - 0.08, 0.0) : 0.0;
        w -= ((((p1 + p2) + p3) + p4) + p5);
        row[24] = w;
        row[26] = q[0] / (len * (double)a.n_mel);            // :197
    }
    __syncthreads();                                         // the rows are read back by other threads below

    // :286-287: torch.tensor(scores) is float32; NaN entries take the mean of the others (sequential, item order)
    if (t == 0) {
        float sum = 0.f;
        int n = 0;
        for (int b = 0; b < B; ++b) {
            const float sc = (float)table[(size_t)b * TL_K + 24];
            if (sc == sc) { sum += sc; ++n; }
        }
        s_fill = (double)(sum / (float)n);                   // no finite score at all: 0 / 0 = NaN, as the reference's empty mean
    }
    __syncthreads();
    for (int b = t; b < B; b += 256) {
        const double sc = (double)(float)table[(size_t)b * TL_K + 24];
        table[(size_t)b * TL_K + 25] = sc == sc ? sc : s_fill;
    }
    __syncthreads();
    // batch sums: thread k owns column k and walks the items in order
    if (t < TL_K) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += table[(size_t)b * TL_K + t];
        s_sum[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        const double frames = s_sum[0], nB = (double)B, n_el = frames * (double)a.n_mel;
        double o[TL_TERMS];
        o[0] = s_sum[1] / n_el;                              // spec_MSE      (:192)
        o[1] = s_sum[2] / n_el;                              // postnet_MSE   (:202)
        o[2] = s_sum[3] / n_el;                              // spec_MFSE     (:209)
        o[3] = s_sum[4] / n_el;                              // postnet_MFSE  (:213)
        o[4] = s_sum[5] / (nB * (double)a.T);                // gate_loss     (:218)
        o[5] = -0.5 * s_sum[8] / nB;                         // sylps_kld     (:224)
        o[6] = s_sum[9] / nB;                                // sylps_MAE     (:230)
        o[7] = s_sum[10] / nB;                               // sylps_MSE     (:231)
        o[8] = s_sum[6] / s_sum[7];                          // diag_att      (:52)
        double loss = o[0] * p.weights[0];                   // :152-161, dict order
        for (int k = 1; k < 9; ++k) loss += o[k] * p.weights[k];
        o[9] = loss;
        o[10] = s_sum[11] / nB;                              // diagonality       (:254)
        o[11] = s_sum[12] / nB;                              // avg_max_attention (:255)
        o[12] = s_sum[25] / nB;                              // weighted_score    (:288)
        for (int k = 0; k < TL_TERMS; ++k) terms[k] = o[k];
    }
}

int launch_finalize(const ctts_taco_loss_params* p, const LossView& v, const FinalArgs& a, double* table, double* terms,
                    hipStream_t s) {
    hipLaunchKernelGGL(taco_finalize_kernel, dim3(1), dim3(256), 0, s, *p, v, a, table, terms);
    CTTS_CHECK_LAUNCH("taco_finalize");
    return CTTS_OK;
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_taco_loss_workspace_bytes(int32_t batch, int32_t n_mel, int32_t T, int32_t enc) {
    return loss_layout(batch, n_mel, T, enc, nullptr, nullptr);
}

int ctts_taco_loss_f32(const ctts_taco_loss_params* params, const float* pred_mel, const float* pred_mel_postnet,
                       const float* gt_mel, const float* gate_logits, const float* gate_target, const float* alignments,
                       const float* sylps_mu, const float* sylps_logvar, const float* pred_sylps, const float* gt_sylps,
                       const int32_t* mel_lengths, const int32_t* text_lengths, const float* pres_prev_state, int32_t batch,
                       int32_t n_mel, int32_t T, int32_t enc, double* table, double* terms, void* workspace,
                       size_t workspace_bytes, void* stream) {
    CTTS_CHECK_ARG(params && pred_mel && pred_mel_postnet && gt_mel && gate_logits && gate_target && alignments && sylps_mu &&
                       sylps_logvar && pred_sylps && gt_sylps && mel_lengths && text_lengths && pres_prev_state && table &&
                       terms && workspace,
                   "taco_loss: NULL argument");
    LossView v;
    const size_t need = loss_layout(batch, n_mel, T, enc, workspace, &v);
    if (!need) return CTTS_E_ARG;
    CTTS_CHECK_ARG(batch <= 65535, "taco_loss: batch %d: at most 65535 items per call", batch);
    if (workspace_bytes < need) {
        set_error("taco_loss: workspace %zu bytes < required %zu", workspace_bytes, need);
        return CTTS_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(taco_lengths_kernel, dim3(batch), dim3(256), 0, s, gate_logits, mel_lengths, text_lengths, v, T, enc);
    CTTS_CHECK_LAUNCH("taco_lengths");
    hipLaunchKernelGGL(taco_mel_gate_kernel, dim3(v.tiles, batch), dim3(256), 0, s, pred_mel, pred_mel_postnet, gt_mel,
                       gate_logits, gate_target, mel_lengths, v.mel_part, n_mel, T, v.tiles, params->gate_positive_weight);
    CTTS_CHECK_LAUNCH("taco_mel_gate");
    hipLaunchKernelGGL(taco_guided_kernel, dim3(v.blocks, batch), dim3(256), 0, s, alignments, mel_lengths, text_lengths,
                       pres_prev_state, v.att_part, T, enc, v.blocks, params->sigma);
    CTTS_CHECK_LAUNCH("taco_guided");
    int rc = ctts_alignment_metric_f32(alignments, v.ilen_f, v.olen_f, batch, T, enc, 0.7f, v.metric_gt, v.align_ws,
                                       v.align_bytes, stream);                                                  // :251
    if (rc != CTTS_OK) return rc;
    rc = ctts_alignment_metric_masked_f32(alignments, v.ilen_f, v.plen_f, v.olen_f, batch, T, enc, 0.7f, v.metric_pred,
                                          v.align_ws, v.align_bytes, stream);                                   // :270
    if (rc != CTTS_OK) return rc;
    const FinalArgs a = {v.metric_gt, v.metric_pred, sylps_mu, sylps_logvar, pred_sylps, gt_sylps, pres_prev_state,
                         mel_lengths, text_lengths, batch, n_mel, T, enc};
    return launch_finalize(params, v, a, table, terms, s);
}

int ctts_taco_loss_finalize_f32(const ctts_taco_loss_params* params, const double* metric_gt, const double* metric_pred,
                                const float* sylps_mu, const float* sylps_logvar, const float* pred_sylps,
                                const float* gt_sylps, const int32_t* mel_lengths, const int32_t* text_lengths,
                                const float* pres_prev_state, int32_t batch, int32_t n_mel, int32_t T, int32_t enc,
                                double* table, double* terms, const void* workspace, size_t workspace_bytes, void* stream) {
    CTTS_CHECK_ARG(params && sylps_mu && sylps_logvar && pred_sylps && gt_sylps && mel_lengths && text_lengths &&
                       pres_prev_state && table && terms && workspace,
                   "taco_loss_finalize: NULL argument");
    LossView v;
    const size_t need = loss_layout(batch, n_mel, T, enc, const_cast<void*>(workspace), &v);
    if (!need) return CTTS_E_ARG;
    if (workspace_bytes < need) {
        set_error("taco_loss_finalize: workspace %zu bytes < required %zu", workspace_bytes, need);
        return CTTS_E_WORKSPACE;
    }
    const FinalArgs a = {metric_gt ? metric_gt : v.metric_gt, metric_pred ? metric_pred : v.metric_pred, sylps_mu,
                         sylps_logvar, pred_sylps, gt_sylps, pres_prev_state, mel_lengths, text_lengths, batch, n_mel, T, enc};
    return launch_finalize(params, v, a, table, terms, as_stream(stream));
}

}  // extern "C"
