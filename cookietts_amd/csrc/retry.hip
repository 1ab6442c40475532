// The T2S server's retry loop on the device (_5_infer/t2s_server/text2speech.py:548-651, :675-695): after every
// Tacotron pass the reference reads each candidate back to the host - six .item() calls and three isnan().any()
// reductions per row - to score it, keep the best candidate of every text and decide whether to run another pass;
// then it pads the winners for the vocoder and converts the audio to int16 in numpy.  Here:
//
//   ctts_retry_update_f32, three stream-ordered launches per pass
//     retry_flags_kernel    grid (rows, parts): any NaN in the row's mel / gate / alignments (:614)        memory-bound
//     retry_replay_kernel   ONE workgroup: scores every row in IEEE double (:598-605, :615), then replays
//                           :590-625 in the reference's order and writes the status block                 latency-bound
//     retry_gather_kernel   grid (texts, 8): texts whose winner changed copy that row's mel / alignments  memory-bound
//   ctts_retry_vocoder_batch_f32   the padded batch of the winners (:645-651)
//   ctts_pcm16_concat              trim, silence, float -> int16, rows back to back (:675-695)
//
// No kernel waits on another workgroup; every loop bound is an argument.  The score must be the reference's bit for bit,
// so nothing in this file may be contracted into a fused multiply-add (the pragma below; build.py adds -ffp-contract=off).
#include "common.h"

#include <climits>

#pragma clang fp contract(off)

namespace ctts {
namespace {

constexpr int RT_MAX = 4096;                     // texts / rows one state takes
constexpr int RT_PARTS = 8;                      // flag words per row (workgroups that may share one row's scan)
constexpr int RT_THREADS = 1024;                 // the replay workgroup
constexpr int RT_CHUNK = RT_MAX / RT_THREADS;    // consecutive texts per replay thread, at most

// The sections of the state behind the status block (include/cookietts_hip.h), as device pointers.
struct RetryView {
    ctts_retry_status* status;
    double* best_score;                          // [n_texts]
    double* detail;                              // [n_texts][6]
    int32_t *tries, *best_length, *best_T, *best_pass, *best_row, *changed;   // [n_texts] each
    float* best_mel;                             // [n_texts][n_mel][t_cap]
    float* best_al;                              // [n_texts][t_cap][enc_cap]
    double* row_score;                           // [rows]      scratch of the last pass
    double* row_detail;                          // [rows][6]
    int32_t* row_flags;                          // [rows][RT_PARTS]
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// 0 = refused (ctts_last_error says why)
size_t retry_layout(const ctts_retry_config* c, void* state, RetryView* v) {
    if (!c) { set_error("retry: NULL config"); return 0; }
    if (c->n_texts < 1 || c->per_text < 1 || c->n_texts > RT_MAX || (int64_t)c->n_texts * c->per_text > RT_MAX) {
        set_error("retry: n_texts %d x per_text %d: both and their product (rows) must be in [1, %d]", c->n_texts, c->per_text,
                  RT_MAX);
        return 0;
    }
    if (c->n_mel < 1 || c->t_cap < 1 || c->enc_cap < 0) {
        set_error("retry: n_mel %d, t_cap %d, enc_cap %d: need n_mel >= 1, t_cap >= 1, enc_cap >= 0", c->n_mel, c->t_cap,
                  c->enc_cap);
        return 0;
    }
    const size_t N = c->n_texts, R = N * c->per_text;
    char* base = static_cast<char*>(state);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off = up16(off + bytes); return p; };
    RetryView w;
    w.status = reinterpret_cast<ctts_retry_status*>(take(sizeof(ctts_retry_status)));
    w.best_score = reinterpret_cast<double*>(take(N * 8));
    w.detail = reinterpret_cast<double*>(take(N * 6 * 8));
    w.tries = reinterpret_cast<int32_t*>(take(N * 4));
    w.best_length = reinterpret_cast<int32_t*>(take(N * 4));
    w.best_T = reinterpret_cast<int32_t*>(take(N * 4));
    w.best_pass = reinterpret_cast<int32_t*>(take(N * 4));
    w.best_row = reinterpret_cast<int32_t*>(take(N * 4));
    w.changed = reinterpret_cast<int32_t*>(take(N * 4));
    w.best_mel = reinterpret_cast<float*>(take(N * c->n_mel * c->t_cap * 4));
    w.best_al = reinterpret_cast<float*>(take(N * c->t_cap * c->enc_cap * 4));
    w.row_score = reinterpret_cast<double*>(take(R * 8));
    w.row_detail = reinterpret_cast<double*>(take(R * 6 * 8));
    w.row_flags = reinterpret_cast<int32_t*>(take(R * RT_PARTS * 4));
    if (v) *v = w;
    return off;
}

__global__ void retry_reset_kernel(RetryView v, int n_texts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n_texts) {
        v.best_score[j] = -1e5;                              // :548
        for (int i = 0; i < 6; ++i) v.detail[(size_t)j * 6 + i] = 0.0;
        v.tries[j] = 0;                                      // :549
        v.best_length[j] = 0;
        v.best_T[j] = 0;
        v.best_pass[j] = -1;                                 // :550 (no winner yet)
        v.best_row[j] = -1;
        v.changed[j] = -1;
    }
    if (j == 0) {
        ctts_retry_status s;
        s.done = 0; s.n_passes = 0; s.min_best_score = -1e5; s.min_tries = 0; s.n_without_winner = n_texts;
        s.max_best_length = 0; s.max_best_T = 0;
        *v.status = s;
    }
}

// ---- (a) non-finite flags ---------------------------------------------------------------------------------------
// One row of `len` floats, shared by `gstride` threads of which this is number `gid`: a scalar head up to the first
// 16-byte boundary, float4 body, scalar tail (a row start is only 4-byte aligned: T * enc may be odd).
__device__ __forceinline__ bool row_has_nan(const float* __restrict__ p, size_t len, size_t gid, size_t gstride) {
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4;
    if (head > len) head = len;
    bool bad = false;
    if (gid < head) { const float x = p[gid]; bad |= x != x; }
    const float4* q = reinterpret_cast<const float4*>(p + head);
    const size_t nv = (len - head) / 4;
    for (size_t i = gid; i < nv; i += gstride) {
        const float4 x = q[i];
        bad |= (x.x != x.x) | (x.y != x.y) | (x.z != x.z) | (x.w != x.w);
    }
    const size_t tail = head + nv * 4;                       // fewer than 4 elements left
    if (tail + gid < len) { const float x = p[tail + gid]; bad |= x != x; }
    return bad;
}

__global__ __launch_bounds__(256) void retry_flags_kernel(RetryView v, const float* __restrict__ mel,
                                                          const float* __restrict__ gate, const float* __restrict__ al,
                                                          int n_mel, int T, int enc) {
    if (v.status->done != 0) return;                         // sticky verdict: the pass is not looked at
    const size_t row = blockIdx.x, gid = (size_t)blockIdx.y * 256 + threadIdx.x, gstride = (size_t)gridDim.y * 256;
    bool bad = row_has_nan(al + row * T * enc, (size_t)T * enc, gid, gstride);
    bad |= row_has_nan(mel + row * n_mel * T, (size_t)n_mel * T, gid, gstride);
    bad |= row_has_nan(gate + row * T, (size_t)T, gid, gstride);
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x == 0) v.row_flags[row * RT_PARTS + blockIdx.y] = any;
}

// ---- (b) scoring and the running best ---------------------------------------------------------------------------
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }   // Python's max(a, b): NaN a stays
__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }

// text2speech.py:598-605 in IEEE double; d = { weighted_score as score_str prints it, the five punishments }
__device__ double retry_score(const ctts_retry_config& c, const double* __restrict__ m, bool long_text, double* d) {
    const double diag = m[0];                                // float64 in the reference (diagonalitys)
    const double avg_prob = (double)(float)m[1], emax = (double)(float)m[2], emin = (double)(float)m[3];
    const double eavg = (double)(float)m[4], pmiss = (double)(float)m[5];   // .item() of float32 tensors
    double w = avg_prob;
    const double p1 = (py_max(diag, 1.10) - 1.10) * 0.5 * c.diagonality_weighting;
    const double p2 = py_max(emax - 60.0, 0.0) * 0.005 * c.max_focus_weighting;
    const double p3 = py_max(0.00 - emin, 0.0) * c.min_focus_weighting;
    const double p4 = py_max(3.6 - eavg, 0.0) * c.avg_focus_weighting;
    const double p5 = long_text ? py_max(pmiss - 0.08, 0.0) : 0.0;
    w -= ((((p1 + p2) + p3) + p4) + p5);
    d[0] = w; d[1] = p1; d[2] = p2; d[3] = p3; d[4] = p4; d[5] = p5;
    return w;
}

// :616-619 over candidates [0, limit) of one text: the best score and its candidate (-1: the entry best stands)
__device__ __forceinline__ double scan_text(const double* __restrict__ rs, int limit, double best, int* win) {
    int w = -1;
    for (int k = 0; k < limit; ++k) {
        const double s = rs[k];
        if (s > best) { best = s; w = k; }                   // strict: first of equals wins, NaN never does
    }
    *win = w;
    return best;
}

// inclusive running minimum over the RT_THREADS entries of two (double, int) pairs of LDS arrays
__device__ void scan_min2(double* d0, int* i0, double* d1, int* i1, int t) {
    for (int off = 1; off < RT_THREADS; off <<= 1) {
        double a = d0[t], b = d1[t];
        int x = i0[t], y = i1[t];
        if (t >= off) { a = dmin(a, d0[t - off]); b = dmin(b, d1[t - off]); x = min(x, i0[t - off]); y = min(y, i1[t - off]); }
        __syncthreads();
        d0[t] = a; d1[t] = b; i0[t] = x; i1[t] = y;
        __syncthreads();
    }
}

template <class V, class Op>
__device__ V block_reduce(V x, Op op, V* scratch) {          // every thread of the workgroup calls it
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = op(x, __shfl_xor(x, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = x;
    __syncthreads();
    V r = scratch[0];
    for (int w = 1; w < RT_THREADS / 64; ++w) r = op(r, scratch[w]);
    return r;
}

__global__ __launch_bounds__(RT_THREADS) void retry_replay_kernel(ctts_retry_config c, RetryView v,
                                                                  const double* __restrict__ metrics,
                                                                  const int32_t* __restrict__ out_len,
                                                                  const int32_t* __restrict__ text_len, int T, int nparts,
                                                                  double* __restrict__ detail_out) {
    __shared__ double s_pb[RT_THREADS], s_sb[RT_THREADS];
    __shared__ int s_pt[RT_THREADS], s_st[RT_THREADS];
    __shared__ int s_stop;
    const int t = threadIdx.x, N = c.n_texts, P = c.per_text, rows = N * P;
    const int pass = v.status->n_passes;
    if (v.status->done != 0) {                               // sticky verdict: nothing changes, nothing is gathered
        for (int j = t; j < N; j += RT_THREADS) v.changed[j] = -1;
        return;
    }
    if (t == 0) s_stop = INT_MAX;

    // every row's score, in parallel
    for (int row = t; row < rows; row += RT_THREADS) {
        const int j = row / P;
        int flag = 0;
        for (int p = 0; p < nparts; ++p) flag |= v.row_flags[(size_t)row * RT_PARTS + p];
        double d[6];
        double s = retry_score(c, metrics + (size_t)row * 6, text_len[j] > 12, d);
        if (flag) s = 1e-7;                                  // :614-615
        v.row_score[row] = s;
        for (int i = 0; i < 6; ++i) {
            v.row_detail[(size_t)row * 6 + i] = d[i];
            if (detail_out) detail_out[(size_t)row * 6 + i] = d[i];
        }
    }
    __syncthreads();

    // The replay visits texts j ascending, candidates k ascending.  At candidate (j, k) the texts before j have taken their
    // whole pass, the texts behind j none of it; so the minima of :621-625 are a running minimum from the front (state after
    // the pass), one from the back (state at entry) and text j's own running values.  Thread t owns texts [j0, j1).
    const int C = (N + RT_THREADS - 1) / RT_THREADS;         // <= RT_CHUNK
    const int j0 = min(t * C, N), j1 = min(j0 + C, N);
    double eb[RT_CHUNK], fb[RT_CHUNK];
    int et[RT_CHUNK];
    double a_fb = INFINITY, a_eb = INFINITY;
    int a_ft = INT_MAX, a_et = INT_MAX;
    for (int i = 0; j0 + i < j1; ++i) {
        const int j = j0 + i;
        int win;
        eb[i] = v.best_score[j];
        et[i] = v.tries[j];
        fb[i] = scan_text(v.row_score + (size_t)j * P, P, eb[i], &win);
        a_fb = dmin(a_fb, fb[i]); a_ft = min(a_ft, et[i] + P);
        a_eb = dmin(a_eb, eb[i]); a_et = min(a_et, et[i]);
    }
    s_pb[t] = a_fb; s_pt[t] = a_ft;
    s_sb[RT_THREADS - 1 - t] = a_eb; s_st[RT_THREADS - 1 - t] = a_et;
    __syncthreads();
    scan_min2(s_pb, s_pt, s_sb, s_st, t);
    double pre_b = t > 0 ? s_pb[t - 1] : INFINITY;
    int pre_t = t > 0 ? s_pt[t - 1] : INT_MAX;
    const double xsuf_b = t < RT_THREADS - 1 ? s_sb[RT_THREADS - 2 - t] : INFINITY;
    const int xsuf_t = t < RT_THREADS - 1 ? s_st[RT_THREADS - 2 - t] : INT_MAX;

    // first candidate, in the reference's order, at which a stop rule fires
    int stop = INT_MAX;
    for (int i = 0; j0 + i < j1 && stop == INT_MAX; ++i) {
        const int j = j0 + i;
        double ob = dmin(pre_b, xsuf_b);                     // the other texts
        int ot = min(pre_t, xsuf_t);
        for (int i2 = i + 1; j0 + i2 < j1; ++i2) { ob = dmin(ob, eb[i2]); ot = min(ot, et[i2]); }
        if (ot >= c.max_attempts || ot >= c.absolute_maximum_tries) {     // else min(tries) is below both bounds
            const double* rs = v.row_score + (size_t)j * P;
            double rb = eb[i];
            for (int k = 0; k < P; ++k) {
                const double s = rs[k];
                if (s > rb) rb = s;
                const int mt = min(ot, et[i] + k + 1);
                const double mb = dmin(ob, rb);
                int code = 0;
                if (mt >= c.max_attempts && mb > (c.absolutely_required_score - 1.0)) code = 2;      // :621
                else if (mt >= c.absolute_maximum_tries) code = 3;                                    // :623
                if (code) { stop = (j * P + k) * 4 + code; break; }
            }
        }
        pre_b = dmin(pre_b, fb[i]); pre_t = min(pre_t, et[i] + P);
    }
    if (stop != INT_MAX) atomicMin(&s_stop, stop);
    __syncthreads();
    const int S = s_stop;
    const int jS = S == INT_MAX ? N : (S >> 2) / P, kS = S == INT_MAX ? 0 : (S >> 2) % P, code = S == INT_MAX ? 0 : (S & 3);

    // apply the candidates the replay reached
    double m_b = INFINITY;
    int m_t = INT_MAX, n_without = 0, mx_len = 0, mx_T = 0;
    for (int i = 0; j0 + i < j1; ++i) {
        const int j = j0 + i;
        const int limit = j < jS ? P : (j == jS ? kS + 1 : 0);
        int win;
        const double nb = scan_text(v.row_score + (size_t)j * P, limit, eb[i], &win);
        const int nt = et[i] + limit;
        int bp = v.best_pass[j], bl = v.best_length[j], bT = v.best_T[j], row = -1;
        if (win >= 0) {
            row = j * P + win;
            bp = pass; bl = out_len[row]; bT = T;
            v.best_score[j] = nb;
            v.best_pass[j] = bp; v.best_row[j] = row; v.best_length[j] = bl; v.best_T[j] = bT;
            for (int q = 0; q < 6; ++q) v.detail[(size_t)j * 6 + q] = v.row_detail[(size_t)row * 6 + q];
        }
        v.tries[j] = nt;
        v.changed[j] = row;
        m_b = dmin(m_b, nb); m_t = min(m_t, nt);
        n_without += bp < 0; mx_len = max(mx_len, bl); mx_T = max(mx_T, bT);
    }
    double* sd = s_pb;
    int* si = s_pt;
    m_b = block_reduce(m_b, [](double a, double b) { return dmin(a, b); }, sd);
    m_t = block_reduce(m_t, [](int a, int b) { return min(a, b); }, si);
    n_without = block_reduce(n_without, [](int a, int b) { return a + b; }, si);
    mx_len = block_reduce(mx_len, [](int a, int b) { return max(a, b); }, si);
    mx_T = block_reduce(mx_T, [](int a, int b) { return max(a, b); }, si);
    if (t == 0) {                                            // the status block, last
        ctts_retry_status s;
        s.done = code ? code : (m_b >= c.target_score ? 1 : 0);          // :552
        s.n_passes = pass + 1;                                            // :560
        s.min_best_score = m_b; s.min_tries = m_t; s.n_without_winner = n_without;
        s.max_best_length = mx_len; s.max_best_T = mx_T;
        *v.status = s;
    }
}

// ---- (c) winner gather ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retry_gather_kernel(RetryView v, const float* __restrict__ mel,
                                                           const float* __restrict__ al, int n_mel, int T, int enc,
                                                           int t_cap, int enc_cap) {
    const size_t j = blockIdx.x;
    const int row = v.changed[j];
    if (row < 0) return;
    const size_t first = (size_t)blockIdx.y * 256 + threadIdx.x, stride = (size_t)gridDim.y * 256;
    const size_t n = (size_t)n_mel * T;
    const float* src = mel + (size_t)row * n;
    float* dst = v.best_mel + j * n_mel * t_cap;
    for (size_t i = first; i < n; i += stride) {
        const size_t m = i / T, col = i - m * T;
        dst[m * t_cap + col] = src[i];
    }
    if (enc_cap > 0) {
        const size_t n2 = (size_t)T * enc;
        const float* asrc = al + (size_t)row * n2;
        float* adst = v.best_al + j * t_cap * enc_cap;
        for (size_t i = first; i < n2; i += stride) {
            const size_t d = i / enc, e = i - d * enc;
            adst[d * enc_cap + e] = asrc[i];
        }
    }
}

// ---- the vocoder batch (:645-651) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retry_vocoder_batch_kernel(RetryView v, float* __restrict__ out, int n_mel, int t_cap,
                                                                  int t_out, float pad_value) {
    const size_t j = blockIdx.x, m = blockIdx.y;
    const int bT = min(v.best_T[j], t_cap);
    const float* src = v.best_mel + (j * n_mel + m) * t_cap;
    float* dst = out + (j * n_mel + m) * t_out;
    for (int col = threadIdx.x; col < t_out; col += 256) dst[col] = col < bT ? src[col] : pad_value;
}

// ---- int16 PCM (:675-695) ---------------------------------------------------------------------------------------
__device__ __forceinline__ int16_t pcm16(float x) {
    const float p = x * 32768.0f;                            // audio.float() * 2**15
    if (p != p) return 0;                                    // NaN: 0 (numpy: platform-defined)
    if (p >= 32767.0f) return 32767;                         // saturates (numpy: platform-defined outside the range)
    if (p <= -32768.0f) return -32768;
    return (int16_t)(int)p;                                  // toward zero, as astype('int16')
}

__device__ __forceinline__ long long clip_samples(const int32_t* frames, int i, int hop, long long ld) {
    const long long n = (long long)max(frames[i], 0) * hop;
    return n < ld ? n : ld;
}

template <class A>
__global__ __launch_bounds__(256) void pcm16_concat_kernel(const A* __restrict__ audio, const int32_t* __restrict__ frames,
                                                           int batch, long long ld, int hop, int silence,
                                                           int16_t* __restrict__ pcm, long long cap,
                                                           long long* __restrict__ offsets) {
    __shared__ long long s_sum[256];
    const int b = blockIdx.x, t = threadIdx.x;
    long long part = 0;
    for (int i = t; i < b; i += 256) part += clip_samples(frames, i, hop, ld) + silence;
    s_sum[t] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) s_sum[t] += s_sum[t + o];
        __syncthreads();
    }
    const long long off = s_sum[0];
    const long long keep = clip_samples(frames, b, hop, ld), n_b = keep + silence;
    const A* src = audio + (size_t)b * ld;
    for (long long n = (long long)blockIdx.y * 256 + t; n < n_b; n += (long long)gridDim.y * 256) {
        const long long pos = off + n;
        if (pos < cap) pcm[pos] = n < keep ? pcm16((float)src[n]) : (int16_t)0;
    }
    if (blockIdx.y == 0 && t == 0) {
        offsets[b] = off;
        if (b == batch - 1) offsets[batch] = off + n_b > cap ? -(off + n_b) : off + n_b;
    }
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_retry_state_bytes(const ctts_retry_config* cfg) { return retry_layout(cfg, nullptr, nullptr); }

int ctts_retry_state_layout(const ctts_retry_config* cfg, size_t* offsets) {
    RetryView v;
    CTTS_CHECK_ARG(offsets, "retry_state_layout: NULL offsets");
    char* const origin = reinterpret_cast<char*>(uintptr_t(16));          // any non-NULL base: only differences are used
    if (!retry_layout(cfg, origin, &v)) return CTTS_E_ARG;
    const void* sections[CTTS_RETRY_SECTIONS] = {v.status, v.best_score, v.detail, v.tries, v.best_length, v.best_T, v.best_pass,
                                                 v.best_row, v.changed, v.best_mel, v.best_al, v.row_score, v.row_detail,
                                                 v.row_flags};
    for (int i = 0; i < CTTS_RETRY_SECTIONS; ++i) offsets[i] = (size_t)(static_cast<const char*>(sections[i]) - origin);
    return CTTS_OK;
}

int ctts_retry_reset(const ctts_retry_config* cfg, void* state, void* stream) {
    RetryView v;
    CTTS_CHECK_ARG(state, "retry_reset: NULL state");
    if (!retry_layout(cfg, state, &v)) return CTTS_E_ARG;
    hipLaunchKernelGGL(retry_reset_kernel, dim3((cfg->n_texts + 255) / 256), dim3(256), 0, as_stream(stream), v, cfg->n_texts);
    CTTS_CHECK_LAUNCH("retry_reset");
    return CTTS_OK;
}

int ctts_retry_update_f32(const ctts_retry_config* cfg, const float* mel, const float* gate, const float* alignments,
                          const double* metrics, const int32_t* output_lengths, const int32_t* text_lengths, int32_t T,
                          int32_t enc, double* detail, void* state, void* stream) {
    RetryView v;
    CTTS_CHECK_ARG(state && mel && gate && alignments && metrics && output_lengths && text_lengths,
                   "retry_update: NULL argument");
    if (!retry_layout(cfg, state, &v)) return CTTS_E_ARG;
    CTTS_CHECK_ARG(T >= 1 && enc >= 1, "retry_update: T %d, enc %d must be positive", T, enc);
    CTTS_CHECK_ARG(T <= cfg->t_cap, "retry_update: a pass of T = %d steps does not fit t_cap = %d", T, cfg->t_cap);
    CTTS_CHECK_ARG(cfg->enc_cap == 0 || enc <= cfg->enc_cap, "retry_update: enc = %d does not fit enc_cap = %d", enc,
                   cfg->enc_cap);
    hipStream_t s = as_stream(stream);
    const int rows = cfg->n_texts * cfg->per_text;
    int nparts = 512 / rows;                                  // a few hundred workgroups at any row count
    nparts = nparts < 1 ? 1 : (nparts > RT_PARTS ? RT_PARTS : nparts);
    hipLaunchKernelGGL(retry_flags_kernel, dim3(rows, nparts), dim3(256), 0, s, v, mel, gate, alignments, cfg->n_mel, T, enc);
    CTTS_CHECK_LAUNCH("retry_flags");
    hipLaunchKernelGGL(retry_replay_kernel, dim3(1), dim3(RT_THREADS), 0, s, *cfg, v, metrics, output_lengths, text_lengths, T,
                       nparts, detail);
    CTTS_CHECK_LAUNCH("retry_replay");
    hipLaunchKernelGGL(retry_gather_kernel, dim3(cfg->n_texts, 8), dim3(256), 0, s, v, mel, alignments, cfg->n_mel, T, enc,
                       cfg->t_cap, cfg->enc_cap);
    CTTS_CHECK_LAUNCH("retry_gather");
    return CTTS_OK;
}

int ctts_retry_vocoder_batch_f32(const ctts_retry_config* cfg, const void* state, float* mel_out, int32_t t_out,
                                 float pad_value, void* stream) {
    RetryView v;
    CTTS_CHECK_ARG(state && mel_out, "retry_vocoder_batch: NULL argument");
    if (!retry_layout(cfg, const_cast<void*>(state), &v)) return CTTS_E_ARG;
    CTTS_CHECK_ARG(t_out >= 1 && cfg->n_mel <= 65535, "retry_vocoder_batch: t_out %d must be positive (n_mel at most 65535)",
                   t_out);
    hipLaunchKernelGGL(retry_vocoder_batch_kernel, dim3(cfg->n_texts, cfg->n_mel), dim3(256), 0, as_stream(stream), v, mel_out,
                       cfg->n_mel, cfg->t_cap, t_out, pad_value);
    CTTS_CHECK_LAUNCH("retry_vocoder_batch");
    return CTTS_OK;
}

int ctts_pcm16_concat(const void* audio, int32_t is_half, const int32_t* frames, int32_t batch, int64_t ld, int32_t hop,
                      int32_t silence_samples, int16_t* pcm, int64_t pcm_capacity, int64_t* offsets, void* stream) {
    CTTS_CHECK_ARG(audio && frames && pcm && offsets, "pcm16_concat: NULL argument");
    CTTS_CHECK_ARG(batch >= 1 && ld >= 1 && hop >= 1 && silence_samples >= 0 && pcm_capacity >= 0,
                   "pcm16_concat: batch %d, ld %lld, hop %d, silence_samples %d, pcm_capacity %lld", batch, (long long)ld, hop,
                   silence_samples, (long long)pcm_capacity);
    const long long per_row = (ld + silence_samples + 256 * 8 - 1) / (256 * 8);             // ~8 samples per thread
    const dim3 grid(batch, (unsigned)(per_row < 1 ? 1 : (per_row > 256 ? 256 : per_row)));
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are 64-bit");
    if (is_half)
        hipLaunchKernelGGL(pcm16_concat_kernel<_Float16>, grid, dim3(256), 0, as_stream(stream),
                           static_cast<const _Float16*>(audio), frames, batch, (long long)ld, hop, silence_samples, pcm,
                           (long long)pcm_capacity, reinterpret_cast<long long*>(offsets));
    else
        hipLaunchKernelGGL(pcm16_concat_kernel<float>, grid, dim3(256), 0, as_stream(stream), static_cast<const float*>(audio),
                           frames, batch, (long long)ld, hop, silence_samples, pcm, (long long)pcm_capacity,
                           reinterpret_cast<long long*>(offsets));
    CTTS_CHECK_LAUNCH("pcm16_concat");
    return CTTS_OK;
}

}  // extern "C"
