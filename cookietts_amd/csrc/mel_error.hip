// Vocoder validation score on the device: the log-mel error between generated and ground-truth audio at several STFT windows
// (_4_mtw/waveglow/train.py:258-278 per file and window; _4_mtw/hifigan/train.py:205-223 per batch).  The reference scores one
// file at a time on the host and reads two .item() per (file, window); here a ragged batch is scored in one call and every number
// lands in one fp64 table that the host reads once.
//
// Per window, stream-ordered:
//   mel_error_frames_kernel  grid (64-frame columns, 64-sample K groups, signal x item): the k-major frame matrix Xf[2B][N][ld] of
//                            BOTH signals; reflect at each item's own end, the framing rule and the sanitising rule applied at
//                            the read; zeros at and beyond an item's frame count                                  memory-bound
//   launch_gemm_f32(MAG)     the STFT's magnitude GEMM over the batch of 2B, exact fp32 products                  compute-bound
//   mel_error_tile_kernel    grid (64-frame tiles, item): mel projection of both magnitude tiles on
//                            v_mfma_f32_32x32x2_f32 (waves = 2 frame halves x 2 interleaved 32-mel blocks, K ascending over the
//                            block's non-zero band of the filterbank),
//                            log(max(., clamp)), d = pred - gt, fp64 |d| and d^2 per lane, wave, then workgroup in wave
//                            order: one partial pair per (item, window, tile).  Magnitudes and mels stay in registers
//                            unless the maps are asked for                                                        compute-bound
// then
//   mel_error_finalize_kernel ONE workgroup: tile partials in tile order, the pair means, and the batch terms in IEEE double in
//                            the reference's order (item-major, window-minor)                                     latency-bound
//
// No kernel waits on another workgroup, no float atomics.  The finalize arithmetic must equal Python's double arithmetic, so nothing
// in this file may contract into a fused multiply-add (the pragma below; build.py adds -ffp-contract=off).
#include "gemm_f32.h"
#include "waveglow_kernels.h"

#pragma clang fp contract(off)

namespace ctts {
namespace {

constexpr int ME_W = CTTS_MEL_ERROR_MAX_WINDOWS;
constexpr int ME_K = CTTS_MEL_ERROR_COLUMNS;
constexpr int ME_TILE = 64;                      // frames per workgroup of the fused kernel
constexpr int ME_A_TILE = GEMM_KC * GEMM_BM;
constexpr size_t ME_ALIGN = 64;

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline size_t align_f(size_t v) { return (v + ME_ALIGN - 1) / ME_ALIGN * ME_ALIGN; }

struct MeWindow {
    int N, cutoff, kmel, mb_mag, pad;
    size_t basis_A, zero_bias, melT, band;       // float offsets into the packed blob; band: int32 [8][2], see mel_error_band_kernel
};

struct MePlan {
    ctts_mel_error_config c;
    int W, n_mel, mpad;
    MeWindow w[ME_W];
    size_t total;                                // floats
};

int make_plan(const ctts_mel_error_config* cfg, MePlan& p) {
    CTTS_CHECK_ARG(cfg != nullptr, "mel_error: config is NULL");
    p.c = *cfg;
    CTTS_CHECK_ARG(cfg->n_windows >= 1 && cfg->n_windows <= ME_W, "mel_error: n_windows=%d (1 to %d)", cfg->n_windows, ME_W);
    CTTS_CHECK_ARG(cfg->n_mel_channels >= 1 && cfg->n_mel_channels <= 256, "mel_error: n_mel_channels=%d (1 to 256)",
                   cfg->n_mel_channels);
    CTTS_CHECK_ARG(cfg->framing == CTTS_MEL_ERROR_TACOTRON || cfg->framing == CTTS_MEL_ERROR_NV, "mel_error: framing=%d",
                   cfg->framing);
    CTTS_CHECK_ARG(cfg->clamp_val > 0.f, "mel_error: clamp_val=%g must be positive", (double)cfg->clamp_val);
    CTTS_CHECK_ARG(cfg->mag_eps >= 0.f, "mel_error: mag_eps=%g must not be negative", (double)cfg->mag_eps);
    p.W = cfg->n_windows;
    p.n_mel = cfg->n_mel_channels;
    p.mpad = round_up(p.n_mel, 32);
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_f(o + n); return r; };
    for (int i = 0; i < p.W; ++i) {
        const int N = cfg->filter_lengths[i];
        CTTS_CHECK_ARG(N >= 32 && N <= 4096 && N % GEMM_KC == 0, "mel_error: filter_length[%d]=%d (a multiple of 16 in [32, 4096])",
                       i, N);
        CTTS_CHECK_ARG(cfg->hop_length >= 1 && cfg->hop_length <= N, "mel_error: hop_length=%d with filter_length %d",
                       cfg->hop_length, N);
        MeWindow& w = p.w[i];
        w.N = N;
        w.cutoff = N / 2 + 1;
        w.kmel = round_up(w.cutoff, GEMM_KC);
        w.mb_mag = (w.cutoff + 127) / 128;
        w.pad = cfg->framing == CTTS_MEL_ERROR_NV ? (N - cfg->hop_length) / 2 : N / 2;
        w.basis_A = take((size_t)w.mb_mag * (N / GEMM_KC) * ME_A_TILE);
        w.zero_bias = take((size_t)w.mb_mag * GEMM_BM);
        w.melT = take((size_t)w.kmel * p.mpad);
        w.band = take(2 * 8);
    }
    p.total = o;
    return CTTS_OK;
}

__host__ __device__ inline int me_frames(int T, int N, int hop, int pad, int framing) {
    if (framing == CTTS_MEL_ERROR_NV) {
        const int s = T + 2 * pad - N;
        return s >= 0 ? s / hop + 1 : 0;
    }
    return T / hop + 1;
}

// the geometry of one call
struct MeGeom {
    int B, T_pred, T_gt, mel_frames, nsig;
    int F[ME_W], tiles[ME_W], ld[ME_W];          // frame capacity, fused-kernel tiles and Xf row stride per window
    int tiles_max;
    size_t xf, wmag, part, total;                // byte offsets / size of the workspace
};

int make_geom(const MePlan& p, int B, int T_pred, int T_gt, int mel_frames, bool gt_mel, MeGeom& g) {
    CTTS_CHECK_ARG(B >= 1 && B <= 32767, "mel_error: batch=%d (1 to 32767)", B);
    CTTS_CHECK_ARG(T_pred >= 1 && (gt_mel ? mel_frames >= 1 : T_gt >= 1), "mel_error: T_pred=%d T_gt=%d mel_frames=%d", T_pred, T_gt,
                   mel_frames);
    g.B = B; g.T_pred = T_pred; g.T_gt = T_gt; g.mel_frames = mel_frames; g.nsig = gt_mel ? 1 : 2;
    size_t xf = 0, wmag = 0;
    g.tiles_max = 0;
    for (int i = 0; i < p.W; ++i) {
        const MeWindow& w = p.w[i];
        const int pf = me_frames(T_pred, w.N, p.c.hop_length, w.pad, p.c.framing);
        const int gf = gt_mel ? mel_frames : me_frames(T_gt, w.N, p.c.hop_length, w.pad, p.c.framing);
        g.F[i] = pf < gf ? pf : gf;
        CTTS_CHECK_ARG(g.F[i] >= 1, "mel_error: window %d (filter_length %d) has no frame at T_pred=%d, T_gt=%d", i, w.N, T_pred, T_gt);
        g.tiles[i] = (g.F[i] + ME_TILE - 1) / ME_TILE;
        g.ld[i] = round_up(g.F[i], GEMM_BN);
        if (g.tiles[i] > g.tiles_max) g.tiles_max = g.tiles[i];
        const size_t a = (size_t)g.nsig * B * w.N * g.ld[i], m = (size_t)g.nsig * B * w.kmel * g.ld[i];
        if (a > xf) xf = a;
        if (m > wmag) wmag = m;
    }
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = (o + bytes + 255) & ~(size_t)255; return r; };
    g.xf = take(xf * sizeof(float));
    g.wmag = take(wmag * sizeof(float));
    g.part = take((size_t)p.W * B * g.tiles_max * 2 * sizeof(double));
    g.total = o;
    return CTTS_OK;
}

// what the kernels need to find an item's frame count
struct MeItem {
    const int32_t *pred_len, *gt_len;
    int T_pred, T_gt, mel_frames, gt_is_mel;
    int N, hop, pad, framing, F;
};

__device__ __forceinline__ int me_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// n_frames(item): min(ground-truth frames, generated frames), never above the capacity of the launch
__device__ __forceinline__ int me_item_frames(const MeItem& a, int b) {
    const int pf = me_frames(me_clampi(a.pred_len[b], 1, a.T_pred), a.N, a.hop, a.pad, a.framing);
    const int gf = a.gt_is_mel ? me_clampi(a.gt_len[b], 0, a.mel_frames)
                               : me_frames(me_clampi(a.gt_len[b], 1, a.T_gt), a.N, a.hop, a.pad, a.framing);
    return min(min(pf, gf), a.F);
}

// mel_basis [n_mel][cutoff] -> melT[k][mpad] (zero rows / columns from the memset)
__global__ __launch_bounds__(256) void mel_error_pack_mel_kernel(const float* __restrict__ mel, float* __restrict__ melT, int n_mel,
                                                                 int cutoff, int mpad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_mel * cutoff) return;
    const int m = i / cutoff, k = i - m * cutoff;
    melT[(size_t)k * mpad + m] = mel[i];
}

// band[mb] = the even-aligned K range [lo, hi) outside which all 32 mel rows of block mb are zero (a triangular filterbank is a band
// per block of rows).  The fused kernel sums K over that range only: the products it skips are exact zeros, so the sums are the dense
// ones bit for bit, in the same ascending order.
__global__ __launch_bounds__(256) void mel_error_band_kernel(const float* __restrict__ mel, int* __restrict__ band, int n_mel, int cutoff,
                                                             int kmel) {
    __shared__ int lo, hi;
    const int mb = blockIdx.x, t = threadIdx.x;
    if (t == 0) { lo = cutoff; hi = 0; }
    __syncthreads();
    const int m1 = min(mb * 32 + 32, n_mel);
    for (int k = t; k < cutoff; k += 256) {
        bool nz = false;
        for (int m = mb * 32; m < m1; ++m) nz |= mel[(size_t)m * cutoff + k] != 0.f;          // a NaN weight counts as non-zero
        if (nz) { atomicMin(&lo, k); atomicMax(&hi, k + 1); }                                 // integer min / max: order-free
    }
    __syncthreads();
    if (t == 0) {
        band[2 * mb] = hi > 0 ? (lo & ~1) : 0;
        band[2 * mb + 1] = hi > 0 ? min((hi + 1) & ~1, kmel) : 0;
    }
}

// Xf[z][k][n] = x_z[reflect(n * hop + k - pad)], z = signal * B + item; zero at n >= n_frames(item)
__global__ __launch_bounds__(256) void mel_error_frames_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               float* __restrict__ xf, MeItem a, int B, int ld, int sanitize) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63);
    const int k0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 16;
    const int z = blockIdx.z, sig = z / B, b = z - sig * B;
    if (n >= ld || k0 >= a.N) return;
    const int width = sig ? a.T_gt : a.T_pred;
    const int T = me_clampi(sig ? a.gt_len[b] : a.pred_len[b], 1, width);
    const float* x = (sig ? gt : pred) + (size_t)b * width;
    const bool live = n < me_item_frames(a, b);
    const bool clean = sanitize && sig == 0;
    const int period = 2 * (T - 1);
    float* o = xf + ((size_t)z * a.N + k0) * ld + n;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
        float v = 0.f;
        if (live) {
            int j = n * a.hop + k0 + kk - a.pad;
            if (period == 0) j = 0;
            else {
                if (j < 0) j = -j;
                if (j >= T) { j %= period; if (j >= T) j = period - j; }   // folded into [0, T): one reflection where T > pad
            }
            v = x[j];
            if (clean) v = v != v ? 0.f : (v > 0.999f ? 0.999f : (v < -0.999f ? -0.999f : v));   // train.py:259-260
        }
        o[(size_t)kk * ld] = v;
    }
}

struct MeTile {
    MeItem it;
    const float *wmag, *melT, *gt_mel;
    const int* band;                             // [mpad / 32][2]: the K range of each 32-mel block
    double* part;                                // [B][tiles][2] of this window
    float *mae_map, *pred_map, *gt_map;          // at this window's plane: element (b, m, n) at (b * map_bstride + m * map_frames + n)
    long long map_bstride;
    int map_frames;
    int B, n_mel, mpad, cutoff, kmel, ld, tiles;
    float clamp, eps;
};

__device__ __forceinline__ double me_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float me_log_clamp(float v, float clamp) { return logf(v < clamp ? clamp : v); }   // a NaN stays, as torch.clamp's

template <bool GT_MEL, bool EPS, bool MAPS>
__global__ __launch_bounds__(256) void mel_error_tile_kernel(MeTile a) {
    __shared__ double red[2][4];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nf = me_item_frames(a.it, b);
    double* out = a.part + ((size_t)b * a.tiles + tile) * 2;
    if (tile * ME_TILE >= nf) {                                // the whole tile lies beyond the item: uniform exit
        if (threadIdx.x == 0) { out[0] = 0.0; out[1] = 0.0; }
        return;
    }
    const int col = lane & 31, kh = lane >> 5;
    const int n = tile * ME_TILE + (wave & 1) * 32 + col;
    const bool live = n < nf;
    const float* mp = a.wmag + (size_t)b * a.kmel * a.ld + n;
    const float* mg = a.wmag + (size_t)(a.B + b) * a.kmel * a.ld + n;
    double sa = 0.0, ss = 0.0;
    for (int mb = wave >> 1; mb * 32 < a.mpad; mb += 2) {
        f32x16 ap, ag;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ap[r] = 0.f; ag[r] = 0.f; }
        const float* A = a.melT + mb * 32 + col;
        const int klo = a.band[2 * mb], khi = a.band[2 * mb + 1];
#pragma unroll 4
        for (int k = klo; k < khi; k += 2) {                  // K ascending over the block's band: the order never depends on the batch
            const int kk = k + kh;
            const bool in = live && kk < a.cutoff;
            const float av = A[(size_t)kk * a.mpad];
            float bp = in ? mp[(size_t)kk * a.ld] : 0.f;
            if (EPS) bp = sqrtf(bp * bp + a.eps);
            ap = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp, ap, 0, 0, 0);
            if (!GT_MEL) {
                float bg = in ? mg[(size_t)kk * a.ld] : 0.f;
                if (EPS) bg = sqrtf(bg * bg + a.eps);
                ag = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bg, ag, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {                         // D row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column = lane & 31
            const int m = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (live && m < a.n_mel) {
                const float p = me_log_clamp(ap[r], a.clamp);
                const float g = GT_MEL ? a.gt_mel[((size_t)b * a.n_mel + m) * a.it.mel_frames + n] : me_log_clamp(ag[r], a.clamp);
                const double d = (double)p - (double)g;
                sa += fabs(d);
                ss += d * d;
                if (MAPS) {
                    const size_t o = (size_t)b * a.map_bstride + (size_t)m * a.map_frames + n;
                    a.mae_map[o] = fabsf(p - g);
                    a.pred_map[o] = p;
                    a.gt_map[o] = g;
                }
            }
        }
    }
    sa = me_wave_sum(sa);
    ss = me_wave_sum(ss);
    if (lane == 0) { red[0][wave] = sa; red[1][wave] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];   // wave order
        out[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

struct MeFinal {
    const int32_t *pred_len, *gt_len;
    const double* part;                          // [W][B][tiles_max][2]
    int B, W, n_mel, tiles_max, T_pred, T_gt, mel_frames, gt_is_mel, hop, framing;
    int N[ME_W], pad[ME_W], F[ME_W], tiles[ME_W];
};

__global__ __launch_bounds__(256) void mel_error_finalize_kernel(MeFinal a, double* __restrict__ table) {
    const int t = threadIdx.x, pairs = a.B * a.W;
    for (int i = t; i < pairs; i += 256) {
        const int b = i / a.W, w = i - b * a.W;
        MeItem it = {a.pred_len, a.gt_len, a.T_pred, a.T_gt, a.mel_frames, a.gt_is_mel, a.N[w], a.hop, a.pad[w], a.framing, a.F[w]};
        const int nf = me_item_frames(it, b);
        const double* p = a.part + ((size_t)w * a.B + b) * a.tiles_max * 2;
        double sae = 0.0, sse = 0.0;
        for (int k = 0; k < a.tiles[w]; ++k) { sae += p[2 * k]; sse += p[2 * k + 1]; }   // tile order
        const double count = (double)a.n_mel * (double)nf;
        double* row = table + (size_t)i * ME_K;
        row[0] = (double)nf;
        row[1] = sae;
        row[2] = sse;
        row[3] = sae / count;
        row[4] = sse / count;
    }
    __syncthreads();                                          // the rows are read back by other threads below
    double* terms = table + (size_t)pairs * ME_K;
    if (t == 0) {                                             // train.py:276-278, 294-295: file-major, window-minor
        double total_mse = 0.0, total_mae = 0.0, total = 0.0;
        for (int i = 0; i < pairs; ++i) {
            total_mae += table[(size_t)i * ME_K + 3];
            total_mse += table[(size_t)i * ME_K + 4];
            total += 1.0;
        }
        terms[0] = total_mse / total;
        terms[1] = total_mae / total;
    }
    if (t >= 64 && t < 64 + ME_W) {                           // hifigan/train.py:208-210 per window: items in item order
        const int w = t - 64;
        double sae = 0.0, count = 0.0;
        if (w < a.W)
            for (int b = 0; b < a.B; ++b) {
                const double* row = table + ((size_t)b * a.W + w) * ME_K;
                sae += row[1];
                count += (double)a.n_mel * row[0];
            }
        terms[2 + w] = w < a.W ? sae / count : 0.0;
    }
}

template <bool GT_MEL, bool EPS>
void launch_tile(bool maps, dim3 grid, hipStream_t s, const MeTile& t) {
    if (maps) hipLaunchKernelGGL((mel_error_tile_kernel<GT_MEL, EPS, true>), grid, dim3(256), 0, s, t);
    else hipLaunchKernelGGL((mel_error_tile_kernel<GT_MEL, EPS, false>), grid, dim3(256), 0, s, t);
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_mel_error_packed_bytes(const ctts_mel_error_config* cfg) {
    MePlan p;
    if (make_plan(cfg, p)) return 0;
    return p.total * sizeof(float);
}

int ctts_mel_error_pack(const ctts_mel_error_config* cfg, int32_t window, const float* forward_basis, const float* mel_basis,
                        void* packed, void* stream) {
    MePlan p;
    int rc = make_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(window >= 0 && window < p.W, "mel_error_pack: window %d of %d", window, p.W);
    CTTS_CHECK_ARG(forward_basis && mel_basis && packed, "mel_error_pack: NULL pointer");
    const MeWindow& w = p.w[window];
    hipStream_t s = as_stream(stream);
    float* blob = static_cast<float*>(packed);
    const size_t end = window + 1 < p.W ? p.w[window + 1].basis_A : p.total;
    CTTS_CHECK_HIP(hipMemsetAsync(blob + w.basis_A, 0, (end - w.basis_A) * sizeof(float), s));
    rc = launch_pack_a(blob + w.basis_A, forward_basis, GEMM_BM, w.mb_mag, w.N / GEMM_KC, 0, w.N, GEMM_EPI_MAG, w.cutoff, 2 * w.cutoff,
                       0, w.N, 1, s);
    if (rc) return rc;
    const int n = p.n_mel * w.cutoff;
    hipLaunchKernelGGL(mel_error_pack_mel_kernel, dim3((n + 255) / 256), dim3(256), 0, s, mel_basis, blob + w.melT, p.n_mel, w.cutoff,
                       p.mpad);
    CTTS_CHECK_LAUNCH("mel_error_pack_mel");
    hipLaunchKernelGGL(mel_error_band_kernel, dim3(p.mpad / 32), dim3(256), 0, s, mel_basis, reinterpret_cast<int*>(blob + w.band), p.n_mel,
                       w.cutoff, w.kmel);
    CTTS_CHECK_LAUNCH("mel_error_band");
    return CTTS_OK;
}

size_t ctts_mel_error_workspace_bytes(const ctts_mel_error_config* cfg, int32_t batch, int32_t T_pred_max, int32_t T_gt_max) {
    MePlan p; MeGeom g;
    if (make_plan(cfg, p)) return 0;
    const bool gt_mel = T_gt_max == 0;
    // the gt_mel form: the frame capacity is bounded by the generated audio's own count
    if (make_geom(p, batch, T_pred_max, T_gt_max, gt_mel ? (1 << 30) : 0, gt_mel, g)) return 0;
    return g.total;
}

int ctts_mel_error_f32(const ctts_mel_error_config* cfg, const void* packed, const float* pred, const int32_t* pred_lengths,
                       const float* gt, const int32_t* gt_lengths, const float* gt_mel, int32_t flags, int32_t batch,
                       int32_t T_pred, int32_t T_gt, int32_t mel_frames, double* table, float* mae_map, float* pred_map,
                       float* gt_map, int32_t map_frames, void* workspace, size_t workspace_bytes, void* stream) {
    MePlan p; MeGeom g;
    int rc = make_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(packed && pred && pred_lengths && gt_lengths && table && workspace, "mel_error: NULL argument");
    CTTS_CHECK_ARG((gt != nullptr) != (gt_mel != nullptr), "mel_error: exactly one of gt and gt_mel must be given");
    CTTS_CHECK_ARG(!gt_mel || p.W == 1, "mel_error: gt_mel is a single-window input (n_windows=%d)", p.W);
    const bool maps = mae_map || pred_map || gt_map;
    CTTS_CHECK_ARG(!maps || (mae_map && pred_map && gt_map), "mel_error: the three maps come together");
    rc = make_geom(p, batch, T_pred, gt_mel ? 0 : T_gt, mel_frames, gt_mel != nullptr, g); if (rc) return rc;
    for (int i = 0; maps && i < p.W; ++i)
        CTTS_CHECK_ARG(map_frames >= g.F[i], "mel_error: map_frames=%d < %d frames of window %d", map_frames, g.F[i], i);
    if (workspace_bytes < g.total) {
        set_error("mel_error: workspace %zu bytes < required %zu", workspace_bytes, g.total);
        return CTTS_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    const float* blob = static_cast<const float*>(packed);
    char* ws = static_cast<char*>(workspace);
    float* xf = reinterpret_cast<float*>(ws + g.xf);
    float* wmag = reinterpret_cast<float*>(ws + g.wmag);
    double* part = reinterpret_cast<double*>(ws + g.part);
    const int B = batch, nz = g.nsig * B;
    MeFinal f{};
    f.pred_len = pred_lengths; f.gt_len = gt_lengths; f.part = part;
    f.B = B; f.W = p.W; f.n_mel = p.n_mel; f.tiles_max = g.tiles_max; f.T_pred = T_pred; f.T_gt = T_gt; f.mel_frames = mel_frames;
    f.gt_is_mel = gt_mel != nullptr; f.hop = p.c.hop_length; f.framing = p.c.framing;
    for (int i = 0; i < p.W; ++i) {
        const MeWindow& w = p.w[i];
        const int ld = g.ld[i];
        f.N[i] = w.N; f.pad[i] = w.pad; f.F[i] = g.F[i]; f.tiles[i] = g.tiles[i];
        const MeItem it = {pred_lengths, gt_lengths, T_pred, T_gt, mel_frames, f.gt_is_mel, w.N, p.c.hop_length, w.pad, p.c.framing,
                           g.F[i]};
        hipLaunchKernelGGL(mel_error_frames_kernel, dim3(ld / 64, (w.N + 63) / 64, nz), dim3(256), 0, s, pred, gt, xf, it, B, ld,
                           flags & CTTS_MEL_ERROR_SANITIZE);
        CTTS_CHECK_LAUNCH("mel_error_frames");

        GemmArgs a{};
        a.gemm_mode = CTTS_GEMM_F32;   // Fourier sums cancel: exact fp32 products, as ctts_stft_mel_f32
        a.ld = ld; a.pad = 0; a.L = g.F[i]; a.ntiles = ld / GEMM_BN; a.batch = nz;
        a.A = blob + w.basis_A; a.bias = blob + w.zero_bias;
        a.nseg = 1; a.nch_total = w.N / GEMM_KC; a.MB = w.mb_mag;
        a.seg[0] = {xf, (long long)w.N * ld, w.N / GEMM_KC, 0, 0, 0};
        a.M = 2 * w.cutoff; a.pairC = w.cutoff;
        a.dst0 = wmag; a.dst0_bstride = (long long)w.kmel * ld; a.dst_ld = ld; a.dst_pad = 0;
        rc = launch_gemm_f32(GEMM_EPI_MAG, a, s);
        if (rc) return rc;

        MeTile t{};
        t.it = it; t.wmag = wmag; t.melT = blob + w.melT; t.gt_mel = gt_mel; t.band = reinterpret_cast<const int*>(blob + w.band);
        t.part = part + (size_t)i * B * g.tiles_max * 2;
        t.tiles = g.tiles_max;
        if (maps) {
            const size_t plane = (size_t)i * p.n_mel * map_frames;
            t.mae_map = mae_map + plane; t.pred_map = pred_map + plane; t.gt_map = gt_map + plane;
            t.map_bstride = (long long)p.W * p.n_mel * map_frames; t.map_frames = map_frames;
        }
        t.B = B; t.n_mel = p.n_mel; t.mpad = p.mpad; t.cutoff = w.cutoff; t.kmel = w.kmel; t.ld = ld;
        t.clamp = p.c.clamp_val; t.eps = p.c.mag_eps;
        const dim3 grid(g.tiles[i], B);
        const bool eps = p.c.mag_eps > 0.f;
        if (gt_mel) { if (eps) launch_tile<true, true>(maps, grid, s, t); else launch_tile<true, false>(maps, grid, s, t); }
        else { if (eps) launch_tile<false, true>(maps, grid, s, t); else launch_tile<false, false>(maps, grid, s, t); }
        CTTS_CHECK_LAUNCH("mel_error_tile");
    }
    hipLaunchKernelGGL(mel_error_finalize_kernel, dim3(1), dim3(256), 0, s, f, table);
    CTTS_CHECK_LAUNCH("mel_error_finalize");
    return CTTS_OK;
}

}  // extern "C"
