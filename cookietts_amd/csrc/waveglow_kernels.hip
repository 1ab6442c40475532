// Non-GEMM kernels of the WaveGlow path (all HBM-bound byte/float shuffles around the
// MFMA conv-GEMM) and the weight-ingest kernels.  gfx950 only.
#include "waveglow_kernels.h"
#include "tuning.h"

namespace ctts {

namespace {

// ------------------------------------------------------------------ weight ingest ----
// w[o][:] = v[o][:] * (g[o] / ||v[o][:]||): one workgroup per output channel.
__global__ __launch_bounds__(256) void fold_weightnorm_kernel(const float* __restrict__ v,
                                                              const float* __restrict__ g,
                                                              float* __restrict__ w, int fan) {
    __shared__ float red[4];
    const int o = blockIdx.x;
    const float* vr = v + (size_t)o * fan;
    float s = 0.f;
    for (int i = threadIdx.x; i < fan; i += 256) { const float x = vr[i]; s = fmaf(x, x, s); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float tot = red[0] + red[1] + red[2] + red[3];
    const float scale = g[o] / sqrtf(tot);
    float* wr = w + (size_t)o * fan;
    for (int i = threadIdx.x; i < fan; i += 256) wr[i] = vr[i] * scale;
}

// dst packed [MB][nch_total][16][bm];  fills K range [k_off, k_off + ksrc):
//   dst(mb, k, r) = src[(src_row_off + dense_row(mb, r)) * src_row_stride + (k - k_off) * src_k_stride]
__global__ __launch_bounds__(256) void pack_a_kernel(float* __restrict__ dst, const float* __restrict__ src, int bm,
                                                     int nch_total, int k_off, int ksrc, int epi, int C, int M,
                                                     long long src_row_off, long long src_row_stride,
                                                     int src_k_stride, int k_group, int k_member) {
    const int mb = blockIdx.y;
    const int k = blockIdx.x;  // 0..ksrc-1
    const int r = threadIdx.x;
    if (r >= bm) return;
    const int drow = gemm_dense_row(epi, bm, mb, r, C, M);
    // k_group > 1: this source is member k_member of a round-robin group (GemmArgs::interleave): its
    // chunk j lands at chunk j*k_group + k_member of the group's K range starting at k_off
    const int kk = k_group > 1 ? k_off + ((k / GEMM_KC) * k_group + k_member) * GEMM_KC + k % GEMM_KC : k_off + k;
    dst[((size_t)mb * nch_total + kk / GEMM_KC) * (GEMM_KC * bm) + (kk % GEMM_KC) * bm + r] =
        drow >= 0 ? src[(src_row_off + drow) * src_row_stride + (long long)k * src_k_stride] : 0.f;
}

// dst[mb*bm + r] = src0[off0 + dense_row] (+ src1[off1 + dense_row])
__global__ __launch_bounds__(256) void pack_bias_kernel(float* __restrict__ dst, int bm, const float* __restrict__ src0,
                                                        long long off0, const float* __restrict__ src1,
                                                        long long off1, int epi, int C, int M) {
    const int mb = blockIdx.x, r = threadIdx.x;
    if (r >= bm) return;
    const int row = gemm_dense_row(epi, bm, mb, r, C, M);
    float v = 0.f;
    if (row >= 0 && src0) {
        v = src0[off0 + row];
        if (src1) v += src1[off1 + row];
    }
    dst[mb * bm + r] = v;
}

// ------------------------------------------------------------ upsample + squeeze ----
// spect[b][o*G+g][pad + l] = bias[o] + sum_{j<taps} sum_i mel[b][i][q-j] * W[i][o][p + hop*j],
//   t = G*l + g = hop*q + p.            (glow.py:318-324)
// Workgroup: one batch item, UQ consecutive frames q, UO output channels; thread <-> phase p
// (hop == 256 threads).  Each W element is loaded once per (i, j, o) and reused for UQ frames
// from registers; mel values are wave-uniform LDS broadcasts.  The [UO][UQ][256] result is
// transposed through LDS so that every spect row is written as contiguous runs of
// UQ*hop/G time steps.
constexpr int UP_UQ = 8;
constexpr int UP_UO = 8;

template <int HOP, int G>
__global__ __launch_bounds__(HOP) void upsample_squeeze_kernel(const float* __restrict__ mel,
                                                               const float* __restrict__ W,
                                                               const float* __restrict__ bias,
                                                               float* __restrict__ spect, int n_mel, int F,
                                                               int win, int ld, int pad) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int taps = win / HOP;
    const int nfr = UP_UQ + taps - 1;            // frames of mel this block touches
    float* smel = smem;                          // [n_mel][nfr]
    float* stile = smem + n_mel * nfr;           // [UO/2][G][UQ*HOP/G + 8] transposed result
    const int p = threadIdx.x;
    const int q0 = blockIdx.x * UP_UQ;
    const int o0 = blockIdx.y * UP_UO;
    const int b = blockIdx.z;
    const float* melb = mel + (size_t)b * n_mel * F;
    for (int idx = p; idx < n_mel * nfr; idx += HOP) {
        const int i = idx / nfr, ff = idx % nfr;
        const int f = q0 - (taps - 1) + ff;      // frame index, may be <0 or >=F
        smel[idx] = (f >= 0 && f < F) ? melb[(size_t)i * F + f] : 0.f;
    }
    __syncthreads();

    float acc[UP_UO][UP_UQ];
#pragma unroll
    for (int o = 0; o < UP_UO; ++o)
#pragma unroll
        for (int q = 0; q < UP_UQ; ++q) acc[o][q] = 0.f;

    for (int i = 0; i < n_mel; ++i) {
        const float* sm = smel + i * nfr;
        for (int j = 0; j < taps; ++j) {
            float w[UP_UO];
#pragma unroll
            for (int o = 0; o < UP_UO; ++o)
                w[o] = (o0 + o < n_mel) ? W[((size_t)i * n_mel + o0 + o) * win + j * HOP + p] : 0.f;
            // frame q0+q uses mel frame q0+q-j  -> smel index (taps-1) + q - j
#pragma unroll
            for (int q = 0; q < UP_UQ; ++q) {
                const float m = sm[taps - 1 + q - j];
#pragma unroll
                for (int o = 0; o < UP_UO; ++o) acc[o][q] = fmaf(m, w[o], acc[o][q]);
            }
        }
    }
    // transpose through LDS (two passes of UO/2 channels): t = HOP*q + p -> (g = p % G, l_local = q*(HOP/G) + p/G)
    constexpr int LPQ = HOP / G;                 // time steps per frame
    constexpr int ROW = UP_UQ * LPQ;             // time steps per block
    constexpr int ROWP = ROW + 8;                // +8 floats: 2-way (free) instead of 8-way write conflicts
    constexpr int HO = UP_UO / 2;
    const int g = p % G, lq = p / G;
    const int L = F * LPQ;
    const int l0 = q0 * LPQ;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();
#pragma unroll
        for (int o = 0; o < HO; ++o)
#pragma unroll
            for (int q = 0; q < UP_UQ; ++q) stile[(o * G + g) * ROWP + q * LPQ + lq] = acc[half * HO + o][q];
        __syncthreads();
        for (int idx = p; idx < HO * G * ROW; idx += HOP) {
            const int row = idx / ROW, ll = idx % ROW;
            const int o = o0 + half * HO + row / G;
            if (o < n_mel && l0 + ll < L)
                spect[((size_t)b * n_mel * G + (size_t)(o0 + half * HO) * G + row) * ld + pad + l0 + ll] =
                    stile[row * ROWP + ll] + bias[o];
        }
    }
}

// Any hop / n_group (glow.py:226-265 takes them freely; the kernel above is the benchmark's hop 256 / n_group 8): one thread per
// output sample t of (b, o), 256 consecutive t per workgroup - consecutive t are consecutive phases p of W (coalesced) and
// share the mel frames.  ~10x the tuned kernel's time; the upsampling is < 2 % of an inference either way.
__global__ __launch_bounds__(256) void upsample_squeeze_generic_kernel(const float* __restrict__ mel, const float* __restrict__ W,
                                                                       const float* __restrict__ bias, float* __restrict__ spect,
                                                                       int n_mel, int F, int win, int hop, int G, int ld, int pad) {
    const int b = blockIdx.z, o = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int taps = win / hop;
    if (t >= (long long)F * hop) return;
    const int q = (int)(t / hop), p = (int)(t % hop);
    const float* melb = mel + (size_t)b * n_mel * F;
    float acc = bias[o];
    for (int i = 0; i < n_mel; ++i) {
        const float* wr = W + ((size_t)i * n_mel + o) * win + p;
        for (int j = 0; j < taps; ++j)
            if (q - j >= 0) acc = fmaf(melb[(size_t)i * F + q - j], wr[j * hop], acc);
    }
    spect[((size_t)b * n_mel * G + (size_t)o * G + (int)(t % G)) * ld + pad + t / G] = acc;
}

// MFMA form of the benchmark's shape (n_mel 80, hop 256, win 4 hop, n_group 8).  The transposed conv is the GEMM
//   out[(o, p)][(b, q)] = sum_{(i, j)} W[i][o][p + hop j] * mel[b][i][q - j],      M = n_mel hop = 20 480, K = 4 n_mel = 320,
// 11.8 GFLOP per 900-frame utterance - the VALU kernel above runs it at 29 TFLOP/s.  Here W is the STATIONARY operand: a workgroup
// owns one output channel o (256 phases = 16 m-tiles of 16 rows, two per wave) and keeps its 256 x 320 slab in registers as
// `v_mfma_f32_16x16x4_f32` A fragments (160 VGPRs per lane), the mel frames of its chunk sit in LDS ([i][frame], read as B
// fragments: lane (n, j) = frame n - j of channel i, k = 4 i + j), and the chunk's frames stream past 32 at a time.
// Row order of the m-tiles is chosen for the SQUEEZED output: wave g holds the phases p = 8 r + g (r = 0..31), which are the 32
// consecutive time steps of frame q in spect row o G + g - a lane's four accumulators are one aligned float4 of that row and a
// store instruction writes 64-byte runs.  W comes pre-packed in fragment order (upsample_pack_mfma_kernel, at pack time).
constexpr int UM_NMEL = 80, UM_HOP = 256, UM_G = 8, UM_TAPS = 4;
constexpr int UM_KCH = UM_NMEL * UM_TAPS / 4;       // k-chunks of 4 = input channels
constexpr int UM_CHUNK_MAX = 320;                   // frames per workgroup (LDS: n_mel x (320 + 4) floats = 101 KiB)

__global__ __launch_bounds__(256) void upsample_pack_mfma_kernel(const float* __restrict__ W, float* __restrict__ Wp) {
    // Wp[((o G + g) 2 + mt)][q = i / 4][lane][e = i % 4] = W[i][o][hop j + 8 (16 mt + lane % 16) + g],  j = lane / 16
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)UM_NMEL * UM_NMEL * UM_HOP * UM_TAPS) return;
    const int e = idx % 4, lane = (idx / 4) % 64, q = (idx / 256) % (UM_KCH / 4);
    const int mt = (idx / (256 * (UM_KCH / 4))) % 2, g = (idx / (512 * (UM_KCH / 4))) % UM_G;
    const int o = (int)(idx / ((size_t)512 * (UM_KCH / 4) * UM_G));
    const int i = 4 * q + e, j = lane / 16, ph = 8 * (16 * mt + lane % 16) + g;
    Wp[idx] = W[((size_t)i * UM_NMEL + o) * (UM_HOP * UM_TAPS) + UM_HOP * j + ph];
}

__global__ __launch_bounds__(512) void upsample_squeeze_mfma_kernel(const float* __restrict__ mel, const float* __restrict__ Wp,
                                                                    const float* __restrict__ bias, float* __restrict__ spect,
                                                                    int F, int chunk, int nchunks, int srow, int ld, int pad) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float smel[];       // [n_mel][srow]: frame (f0 - 3 + x) at x, zeros outside [0, F)
    const int o = blockIdx.x, b = blockIdx.y / nchunks, f0 = (blockIdx.y % nchunks) * chunk;
    const int fend = min(F, f0 + chunk);
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    // A fragments first: their latency hides behind the staging of the mel chunk
    f32x4 a[2][UM_KCH / 4];
    const f32x4* wp = reinterpret_cast<const f32x4*>(Wp) + ((size_t)(o * UM_G + g) * 2) * (UM_KCH / 4) * 64 + lane;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int q = 0; q < UM_KCH / 4; ++q) a[mt][q] = __builtin_nontemporal_load(wp + (mt * (UM_KCH / 4) + q) * 64);
    const float* melb = mel + (size_t)b * UM_NMEL * F;
    // wave g stages channels g, g + 8, ...: <= 6 independent loads per channel in flight (srow <= 324)
    for (int i = g; i < UM_NMEL; i += 8) {
        float v[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int f = f0 - (UM_TAPS - 1) + lane + 64 * u;
            v[u] = (lane + 64 * u < srow && f >= 0 && f < F) ? melb[(size_t)i * F + f] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 6; ++u)
            if (lane + 64 * u < srow) smel[i * srow + lane + 64 * u] = v[u];
    }
    __syncthreads();
    const float bo = bias[o];
    const int n = lane & 15, jq = lane >> 4;
    const float* sb = smel + (UM_TAPS - 1) + n - jq;                   // B fragment of k-chunk i, frame tile t: sb[i srow + 16 t]
    float* row = spect + ((size_t)b * UM_NMEL * UM_G + (size_t)o * UM_G + g) * ld + pad + 4 * jq;
    for (int t0 = 0; f0 + 16 * t0 < fend; t0 += 2) {
        f32x4 acc[2][2] = {};
        float b0 = sb[16 * t0], b1 = sb[16 * t0 + 16];
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
        for (int i = 0; i < UM_KCH; ++i) {
            const float c0 = b0, c1 = b1;
            if (i + 1 < UM_KCH) { b0 = sb[(i + 1) * srow + 16 * t0]; b1 = sb[(i + 1) * srow + 16 * t0 + 16]; }   // one k-chunk ahead of its use
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][i / 4][i % 4], c0, acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][i / 4][i % 4], c1, acc[mt][1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // the next chunk's fragment read (one ds_read2) ...
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);      // ... ahead of this chunk's four MFMAs
        }
        // D: lane (n, jq) holds rows 4 jq + v of m-tile mt = time steps 32 f + 16 mt + 4 jq + v of frame f = f0 + 16 t + n
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int f = f0 + 16 * (t0 + tt) + n;
            if (f < fend) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    f32x4 v = acc[mt][tt];
                    v.x += bo; v.y += bo; v.z += bo; v.w += bo;
                    *reinterpret_cast<f32x4*>(row + (size_t)f * (UM_HOP / UM_G) + 16 * mt) = v;
                }
            }
        }
    }
}

// --------------------------------------------------------------------- WN start ----
// x[b][c][pad + n] = bs[c] + sum_{j<h} Ws[c][j] * audio[b][ch_off + j][n]     (glow.py:189)
template <int H>
__global__ __launch_bounds__(256) void wn_start_kernel(const float* __restrict__ audio, const float* __restrict__ Ws,
                                                       const float* __restrict__ bs, float* __restrict__ x,
                                                       int C, int G, int ch_off, int L, int ld, int pad) {
    const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int b = blockIdx.z;
    if (n >= L) return;
    float4 a[H];
#pragma unroll
    for (int j = 0; j < H; ++j)
        a[j] = *reinterpret_cast<const float4*>(audio + ((size_t)b * G + ch_off + j) * L + n);
    const int c0 = blockIdx.y * 32;
    float* xb = x + (size_t)b * C * ld + pad + n;
    for (int c = c0; c < c0 + 32 && c < C; ++c) {
        float4 v;
        const float bias = bs[c];
        v.x = v.y = v.z = v.w = bias;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float w = Ws[c * H + j];
            v.x = fmaf(w, a[j].x, v.x); v.y = fmaf(w, a[j].y, v.y);
            v.z = fmaf(w, a[j].z, v.z); v.w = fmaf(w, a[j].w, v.w);
        }
        *reinterpret_cast<float4*>(xb + (size_t)c * ld) = v;
    }
}

// -------------------------------------------------------------------- flow tail ----
// (b, log_s) = (e[:h], e[h:]) of one thread's 4 time steps n..n+3; a1 = (a1 - b) / exp(log_s);
// audio[ch_off : ch_off+2h] = Winv * [a0; a1]; optional un-squeeze to wave.   (glow.py:337-340, 349)
template <int H>
__device__ __forceinline__ void coupling_tail(float4 (&e)[2 * H], const float* sWinv, float* __restrict__ audio,
                                              float* __restrict__ wave, int b, int G, int ch_off, int L, int n) {
    constexpr int E = 2 * H;
    float* ab = audio + ((size_t)b * G + ch_off) * L + n;
    float4 a[E];
#pragma unroll
    for (int j = 0; j < E; ++j) a[j] = *reinterpret_cast<const float4*>(ab + (size_t)j * L);
#pragma unroll
    for (int j = 0; j < H; ++j) {
        a[H + j].x = (a[H + j].x - e[j].x) / expf(e[H + j].x);
        a[H + j].y = (a[H + j].y - e[j].y) / expf(e[H + j].y);
        a[H + j].z = (a[H + j].z - e[j].z) / expf(e[H + j].z);
        a[H + j].w = (a[H + j].w - e[j].w) / expf(e[H + j].w);
    }
    float4 m[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const float w = sWinv[i * E + j];
            s.x = fmaf(w, a[j].x, s.x); s.y = fmaf(w, a[j].y, s.y);
            s.z = fmaf(w, a[j].z, s.z); s.w = fmaf(w, a[j].w, s.w);
        }
        m[i] = s;
    }
    if (wave == nullptr) {
#pragma unroll
        for (int i = 0; i < E; ++i) *reinterpret_cast<float4*>(ab + (size_t)i * L) = m[i];
    } else if constexpr (E % 4 == 0) {
        // un-squeeze: wave[b][G*l + g] = audio[b][g][l]; on the last flow ch_off == 0 and E == G
        float* wb = wave + (size_t)b * G * L + (size_t)n * G;
        const float* mf = reinterpret_cast<const float*>(m);   // m[i].{x,y,z,w} = channel i, step n+{0..3}
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < E; i += 4) {
                float4 v = make_float4(mf[(i + 0) * 4 + s], mf[(i + 1) * 4 + s], mf[(i + 2) * 4 + s], mf[(i + 3) * 4 + s]);
                *reinterpret_cast<float4*>(wb + s * G + i) = v;
            }
    }
}

// The forward direction of the same boundary (glow.py:305-307), for wave 0 of a tail workgroup - all 64 lanes, also those whose four
// steps lie beyond L (they load and store nothing and add 0): a1 = exp(log_s) a1 + b in place (expf, one fma), log_s stored where
// asked, and the workgroup's sum of log_s in fp64 - each lane its <= 4 H values in a fixed order, then the butterfly over the wave -
// to its own slot of `part`.  No atomics: a second stage adds the slots in a fixed order.
template <int H>
__device__ __forceinline__ void coupling_forward(const float4 (&e)[2 * H], float* __restrict__ audio, const CouplingForward& f,
                                                 int b, int G, int ch_off, int L, int n) {
    double s = 0.0;
    if (n < L) {
        float* ab = audio + ((size_t)b * G + ch_off + H) * L + n;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            float4 a = *reinterpret_cast<const float4*>(ab + (size_t)j * L);
            const float4 ls = e[H + j];
            a.x = fmaf(expf(ls.x), a.x, e[j].x); a.y = fmaf(expf(ls.y), a.y, e[j].y);
            a.z = fmaf(expf(ls.z), a.z, e[j].z); a.w = fmaf(expf(ls.w), a.w, e[j].w);
            *reinterpret_cast<float4*>(ab + (size_t)j * L) = a;
            if (f.log_s) *reinterpret_cast<float4*>(f.log_s + (size_t)b * f.ls_bstride + (size_t)j * L + n) = ls;
            s += ((double)ls.x + (double)ls.y) + ((double)ls.z + (double)ls.w);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) f.part[(size_t)b * f.part_bstride + blockIdx.x] = s;
}

// e = Wend * out + bend; (b, log_s) = (e[:h], e[h:]); a1 = (a1 - b) / exp(log_s);
// audio[ch_off : ch_off+2h] = Winv * [a0; a1]; optional un-squeeze to wave.
// (glow.py:222, 337-340, 349).  Workgroup = 4 waves x 256 time steps; each wave reduces a
// quarter of the C skip channels with 16-byte loads, partial sums meet in LDS.
// FWD: the same reduction, then coupling_forward instead (Winv, wave unused).
template <int H, bool FWD>
__global__ __launch_bounds__(256) void flow_tail_kernel(const float* __restrict__ out, float* __restrict__ audio,
                                                        float* __restrict__ wave, const float* __restrict__ Wend,
                                                        const float* __restrict__ bend, const float* __restrict__ Winv,
                                                        int C, int G, int ch_off, int L, int ld, int pad, CouplingForward fw) {
    constexpr int E = 2 * H;
    __shared__ __attribute__((aligned(16))) float part[3][E][256];
    __shared__ float sWinv[E * E];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + lane * 4;
    if (!FWD && threadIdx.x < E * E) sWinv[threadIdx.x] = Winv[threadIdx.x];
    float4 e[E];
#pragma unroll
    for (int j = 0; j < E; ++j) e[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int cq = C / 4;
    const int cbeg = __builtin_amdgcn_readfirstlane(wv * cq);
    // columns beyond L inside the padded row are readable (zero / never stored)
    const float* ob = out + (size_t)b * C * ld + pad + n;
    for (int c = cbeg; c < cbeg + cq; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(ob + (size_t)c * ld);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const float w = Wend[j * C + c];
            e[j].x = fmaf(w, v.x, e[j].x); e[j].y = fmaf(w, v.y, e[j].y);
            e[j].z = fmaf(w, v.z, e[j].z); e[j].w = fmaf(w, v.w, e[j].w);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < E; ++j) *reinterpret_cast<float4*>(&part[wv - 1][j][lane * 4]) = e[j];
    }
    __syncthreads();
    if (wv != 0 || (!FWD && n >= L)) return;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const float bj = bend[j];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 pv = *reinterpret_cast<const float4*>(&part[q][j][lane * 4]);
            e[j].x += pv.x; e[j].y += pv.y; e[j].z += pv.z; e[j].w += pv.w;
        }
        e[j].x += bj; e[j].y += bj; e[j].z += bj; e[j].w += bj;
    }
    if constexpr (FWD) coupling_forward<H>(e, audio, fw, b, G, ch_off, L, n);
    else coupling_tail<H>(e, sWinv, audio, wave, b, G, ch_off, L, n);
}

// ------------------------------------------------------------ forward-direction head and sums ----
// Head of a forward flow (glow.py:294; SQ: with the squeeze of glow.py:284 in front): one thread holds the E rows of four
// consecutive columns, W [E][E] sits in LDS, rows [ch_off, ch_off + E) of z [B][G][L] <- W . rows, in place (a thread reads
// all of its columns before it writes any).  SQ (flow 0, E == G, ch_off == 0): column l of row g is wave[b][G l + g] - the four
// columns are 4 G consecutive floats, read as whole float4s (E % 4 == 0).
template <int E, bool SQ>
__global__ __launch_bounds__(256) void flow_head_forward_kernel(const float* __restrict__ W, const float* __restrict__ wave,
                                                                float* __restrict__ z, int G, int ch_off, int L) {
    __shared__ float sW[E * E];
    for (int i = threadIdx.x; i < E * E; i += 256) sW[i] = W[i];
    __syncthreads();
    const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int b = blockIdx.y;
    if (n >= L) return;
    float* zb = z + ((size_t)b * G + ch_off) * L + n;
    float4 a[E];
    if constexpr (SQ) {
        const float* wb = wave + (size_t)b * G * L + (size_t)n * G;
        float af[E * 4];                                       // af[4 i + s] = channel i, step n + s
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < E; i += 4) {
                const float4 v = *reinterpret_cast<const float4*>(wb + s * E + i);
                af[(i + 0) * 4 + s] = v.x; af[(i + 1) * 4 + s] = v.y; af[(i + 2) * 4 + s] = v.z; af[(i + 3) * 4 + s] = v.w;
            }
#pragma unroll
        for (int i = 0; i < E; ++i) a[i] = make_float4(af[4 * i], af[4 * i + 1], af[4 * i + 2], af[4 * i + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < E; ++j) a[j] = *reinterpret_cast<const float4*>(zb + (size_t)j * L);
    }
#pragma unroll
    for (int i = 0; i < E; ++i) {
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const float w = sW[i * E + j];
            m.x = fmaf(w, a[j].x, m.x); m.y = fmaf(w, a[j].y, m.y);
            m.z = fmaf(w, a[j].z, m.z); m.w = fmaf(w, a[j].w, m.w);
        }
        *reinterpret_cast<float4*>(zb + (size_t)i * L) = m;
    }
}

// fp64 sum over one workgroup: the butterfly over each wave, then the four waves in order (all 256 threads call it)
__device__ __forceinline__ double block_sum_f64(double s, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// part[b][blockIdx.x] = sum of v^2 in fp64 (every square exact) over floats [FWD_SUMSQ_CHUNK blockIdx.x, + FWD_SUMSQ_CHUNK) of item b
__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ z, double* __restrict__ part,
                                                             long long n_item, int nblk) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const float* zb = z + (size_t)b * n_item;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < FWD_SUMSQ_CHUNK / 1024; ++r) {
        const long long i = (long long)blockIdx.x * FWD_SUMSQ_CHUNK + (r * 256 + threadIdx.x) * 4;
        if (i < n_item) {                                      // n_item % 4 == 0: a float4 is all in or all out
            const float4 v = *reinterpret_cast<const float4*>(zb + i);
            s += ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
        }
    }
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) part[(size_t)b * nblk + blockIdx.x] = s;
}

// Second stage of both sums: one wave per (k, b) adds its n slots, lane i the slots i, i + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void sum_partials_kernel(const double* __restrict__ part, long long part_bstride,
                                                          long long part_kstride, int n, double* __restrict__ out,
                                                          int out_bstride) {
    const int k = blockIdx.x, b = blockIdx.y;
    const double* p = part + (size_t)b * part_bstride + (size_t)k * part_kstride;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s += p[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) out[(size_t)b * out_bstride + k] = s;
}


// ------------------------------------------------------------- WN start / end folds ----
// Both 1x1 convolutions at the ends of the WN stack are linear maps beside GEMMs whose outputs are used only through
// them (glow.py:188-222), so they are folded into those GEMMs' weights once per pack, in fp64, rounded to fp32 once:
//   layer 0:  W_in,0[tap] . x_0 = (W_in,0[tap] . [W_start | b_start]) . [a; 1]    (the 1 row is 0 where the conv zero-pads)
//   end:      W_end . sum_i (W_skip,i act_i + b_skip,i) + b_end = sum_i (W_end . W_skip,i) act_i + b'

// dst[o][r][t] (an in_w of FOLD_ROWS input channels): r < H: sum_c W_in[o][c][t] Ws[c][r]; r == H: sum_c W_in[o][c][t] bs[c]; else 0
__global__ __launch_bounds__(256) void fold_in0_kernel(const float* __restrict__ in_w, const float* __restrict__ Ws,
                                                       const float* __restrict__ bs, float* __restrict__ dst, int C, int H,
                                                       int ks, int rows) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * FOLD_ROWS * ks) return;
    const int t = idx % ks, r = (idx / ks) % FOLD_ROWS, o = idx / (ks * FOLD_ROWS);
    double acc = 0.0;
    if (r <= H) {
        const float* wr = in_w + (size_t)o * C * ks + t;
        for (int c = 0; c < C; ++c) acc += (double)wr[(size_t)c * ks] * (double)(r < H ? Ws[c * H + r] : bs[c]);
    }
    dst[idx] = (float)acc;
}

// Wf[c][e] = sum_m W_end[e][m] W_skip[m][c]   (W_skip = rows [row_off, row_off + C) of res_skip_layers.i, [rows][C])
__global__ __launch_bounds__(256) void fold_skend_w_kernel(const float* __restrict__ Wend, const float* __restrict__ rs_w,
                                                           float* __restrict__ Wf, int C, int E, int row_off) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * E) return;
    const int e = idx % E, c = idx / E;
    double acc = 0.0;
    for (int m = 0; m < C; ++m) acc += (double)Wend[(size_t)e * C + m] * (double)rs_w[(size_t)(row_off + m) * C + c];
    Wf[idx] = (float)acc;
}

struct SkipBiasPtrs { const float* p[12]; int row_off[12]; };

// bf[e] = b_end[e] + sum_m W_end[e][m] sum_i b_skip,i[m]
__global__ __launch_bounds__(64) void fold_skend_b_kernel(const float* __restrict__ Wend, const float* __restrict__ bend,
                                                          SkipBiasPtrs sb, int n_layers, float* __restrict__ bf, int C, int E) {
    const int e = threadIdx.x;
    if (e >= E) return;
    double acc = 0.0;
    for (int m = 0; m < C; ++m) {
        double bm = 0.0;
        for (int i = 0; i < n_layers; ++i) bm += (double)sb.p[i][sb.row_off[i] + m];
        acc += (double)Wend[(size_t)e * C + m] * bm;
    }
    bf[e] = (float)(acc + (double)bend[e]);
}

// ----------------------------------------------------- Winograd F(2,3) in-layer form ----
// The 3-tap dilated conv of a WN layer (dilation d) on the output pair (t, t + d):
//   u[t]     = W0 V1 + (G2 V2 + G3 V3),   u[t + d] = (G2 V2 - G3 V3) + (-W2) V4
//   V1 = x[t-d] - x[t+d]   V2 = x[t] + x[t+d]   V3 = x[t+d] - x[t]   V4 = x[t] - x[t+2d]
//   G2 = (W0 + W1 + W2) / 2   G3 = (W0 - W1 + W2) / 2
// 2 C MACs per output and row instead of 3 C.  Pair column j of a batch item stands for t_e = (j / d) 2d + j % d and
// t_o = t_e + d; there are Lp = ceil(L / 2d) d of them.

// dense[0] = G2, dense[1] = G3, dense[2] = -W2 as [rows][C] (in_w: [rows][C][3]); fp64 sums rounded once
__global__ __launch_bounds__(256) void winograd_g_kernel(const float* __restrict__ in_w, float* __restrict__ dense, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const double w0 = in_w[(size_t)idx * 3], w1 = in_w[(size_t)idx * 3 + 1], w2 = in_w[(size_t)idx * 3 + 2];
    dense[idx] = (float)((w0 + w1 + w2) * 0.5);
    dense[(size_t)n + idx] = (float)((w0 - w1 + w2) * 0.5);
    dense[2 * (size_t)n + idx] = -in_w[(size_t)idx * 3 + 2];
}

// x [B][C][ld] and the flow's cond rows h2 [B][H][ld] (natural layout) -> V1..V4 [4][B][C][ldp] and the copies h2e, h2o
// [2][B][H][ldp] in pair order (grid.y = C + H; grid.y = C: no cond rows - the GATE launches read h2 in place).  Everything
// outside [0, L) reads as zero (what the conv's zero padding means; t + 2d can lie beyond the halo), columns [Lp, ncols) are
// written as zeros.  One thread: four pair columns of one row.
// MODE 1: d % 4 == 0 and L % 4 == 0 - the four columns are four consecutive time steps, 16-byte aligned, all inside or all outside
// MODE 2: d == 2 and L % 4 == 0 - pair columns j4 .. j4 + 3 stand for t_e = 2 j4 + {0, 1, 4, 5}, so every tap lies in
//         x[2 j4 - 4 .. 2 j4 + 11]: four aligned 16-byte loads, each all inside or all outside; Lp is even, so the columns
//         j4 + 2, j4 + 3 can lie beyond it on their own
// MODE 0: one column at a time
template <int MODE>
__global__ __launch_bounds__(256) void winograd_transform_kernel(const float* __restrict__ x, long long x_bstride,
                                                                 const float* __restrict__ h2, long long h_bstride,
                                                                 float* __restrict__ V, float* __restrict__ Hc, int C, int H,
                                                                 int d, int L, int Lp, int ld, int pad, int ldp, int ncols) {
    const int j4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (j4 >= ncols) return;
    const int row = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const bool is_x = row < C;
    const float* src = is_x ? x + (size_t)b * x_bstride + (size_t)row * ld + pad
                            : h2 + (size_t)b * h_bstride + (size_t)(row - C) * ld + pad;
    float4 vm = {0.f, 0.f, 0.f, 0.f}, v0 = vm, v1 = vm, v2 = vm;      // x[t_e - d], x[t_e], x[t_e + d], x[t_e + 2d]
    [[maybe_unused]] auto ld4 = [&](int t) { return (t >= 0 && t < L) ? *reinterpret_cast<const float4*>(src + t) : make_float4(0.f, 0.f, 0.f, 0.f); };
    if constexpr (MODE == 1) {
        if (j4 < Lp) {
            const int te = (j4 / d) * 2 * d + j4 % d;
            if (is_x) { vm = ld4(te - d); v2 = ld4(te + 2 * d); }
            v0 = ld4(te); v1 = ld4(te + d);
        }
    } else if constexpr (MODE == 2) {
        if (j4 < Lp) {
            const int t0 = 2 * j4;
            const float4 q = ld4(t0), r = ld4(t0 + 4);
            float4 p = vm, u = vm;                                   // (cond rows: V1, V4 are not formed)
            if (is_x) { p = ld4(t0 - 4); u = ld4(t0 + 8); }
            const bool hi = j4 + 2 < Lp;                             // columns j4 + 2, j4 + 3 (Lp is even)
            vm = make_float4(p.z, p.w, hi ? q.z : 0.f, hi ? q.w : 0.f);
            v0 = make_float4(q.x, q.y, hi ? r.x : 0.f, hi ? r.y : 0.f);
            v1 = make_float4(q.z, q.w, hi ? r.z : 0.f, hi ? r.w : 0.f);
            v2 = make_float4(r.x, r.y, hi ? u.x : 0.f, hi ? u.y : 0.f);
        }
    } else {
        float am[4], a0[4], a1[4], a2[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j4 + e;
            const int te = (j / d) * 2 * d + j % d;
            const bool in = j < Lp;
            auto ld1 = [&](int t) { return (in && t >= 0 && t < L) ? src[t] : 0.f; };
            am[e] = is_x ? ld1(te - d) : 0.f; a2[e] = is_x ? ld1(te + 2 * d) : 0.f;
            a0[e] = ld1(te); a1[e] = ld1(te + d);
        }
        vm = make_float4(am[0], am[1], am[2], am[3]); v0 = make_float4(a0[0], a0[1], a0[2], a0[3]);
        v1 = make_float4(a1[0], a1[1], a1[2], a1[3]); v2 = make_float4(a2[0], a2[1], a2[2], a2[3]);
    }
    if (is_x) {
        const size_t plane = (size_t)B * C * ldp;
        float* o = V + ((size_t)b * C + row) * ldp + j4;
        *reinterpret_cast<float4*>(o) = make_float4(vm.x - v1.x, vm.y - v1.y, vm.z - v1.z, vm.w - v1.w);
        *reinterpret_cast<float4*>(o + plane) = make_float4(v0.x + v1.x, v0.y + v1.y, v0.z + v1.z, v0.w + v1.w);
        *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, v1.w - v0.w);
        *reinterpret_cast<float4*>(o + 3 * plane) = make_float4(v0.x - v2.x, v0.y - v2.y, v0.z - v2.z, v0.w - v2.w);
    } else {
        const size_t plane = (size_t)B * H * ldp;
        float* o = Hc + ((size_t)b * H + (row - C)) * ldp + j4;
        *reinterpret_cast<float4*>(o) = v0;
        *reinterpret_cast<float4*>(o + plane) = v1;
    }
}

// --------------------------------------------------- Winograd F(4,3) in-layer form ----
// The same conv on the output quad t_k = t_0 + k d, k = 0..3, from the six taps x_j = x[t_0 + (j - 1) d], j = 0..5, with the
// interpolation points 0, +-1, +-2, inf:
//   V0 = 4 x0 - 5 x2 + x4          V1 = -4 (x1 + x2) + (x3 + x4)     V2 = 4 (x1 - x2) - (x3 - x4)
//   V3 = -2 (x1 - x3) - (x2 - x4)  V4 = 2 (x1 - x3) - (x2 - x4)      V5 = 4 x1 - 5 x3 + x5
//   U0 = W0 / 4   U1 = -(W0 + W1 + W2) / 6   U2 = -(W0 - W1 + W2) / 6   U3 = W0 / 24 + W1 / 12 + W2 / 6
//   U4 = W0 / 24 - W1 / 12 + W2 / 6   U5 = W2
//   P_j = U_j V_j:  u[t_0] = P0 + (P1 + P2) + (P3 + P4)           u[t_1] = (P1 - P2) + 2 (P3 - P4)
//                   u[t_2] = (P1 + P2) + 4 (P3 + P4)              u[t_3] = (P1 - P2) + 8 (P3 - P4) + P5
// 1.5 C MACs per output and row.  Quad column q of a batch item stands for t_0 = (q / d) 4d + q % d; there are Lq = ceil(L / 4d) d.

// dense[j] = U_j, j = 0..5, as [rows][C] (in_w: [rows][C][3]); fp64 sums rounded once
__global__ __launch_bounds__(256) void winograd_g43_kernel(const float* __restrict__ in_w, float* __restrict__ dense, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const double w0 = in_w[(size_t)idx * 3], w1 = in_w[(size_t)idx * 3 + 1], w2 = in_w[(size_t)idx * 3 + 2];
    dense[idx] = (float)(w0 / 4.0);
    dense[(size_t)n + idx] = (float)(-(w0 + w1 + w2) / 6.0);
    dense[2 * (size_t)n + idx] = (float)(-(w0 - w1 + w2) / 6.0);
    dense[3 * (size_t)n + idx] = (float)(w0 / 24.0 + w1 / 12.0 + w2 / 6.0);
    dense[4 * (size_t)n + idx] = (float)(w0 / 24.0 - w1 / 12.0 + w2 / 6.0);
    dense[5 * (size_t)n + idx] = in_w[(size_t)idx * 3 + 2];
}

// x [B][C][ld] and the flow's cond rows h2 [B][H][ld] -> V0..V5 [6][B][C][ldq] and the copies h(t_0)..h(t_3) [4][B][H][ldq] in
// quad order (grid.y = C + H; grid.y = C: no cond rows - the layer kernel reads h2 in place).  Zero outside [0, L); columns
// [Lq, ncols) are written as zeros.  One thread: four quad columns of one row.
// MODE 1: d % 4 == 0 and L % 4 == 0 - four consecutive time steps per tap, 16-byte aligned, all inside or all outside
// MODE 2: d == 2 and L % 4 == 0 - quad columns q4 .. q4 + 3 stand for t_0 = 4 q4 + {0, 1, 8, 9}: every tap lies in
//         x[4 q4 - 4 .. 4 q4 + 20), six aligned 16-byte loads; Lq is even, so the columns q4 + 2, q4 + 3 can lie beyond it on their own
// MODE 0: one column at a time
template <int MODE>
__global__ __launch_bounds__(256) void winograd_transform_quad_kernel(const float* __restrict__ x, long long x_bstride,
                                                                      const float* __restrict__ h2, long long h_bstride,
                                                                      float* __restrict__ V, float* __restrict__ Hc, int C, int H,
                                                                      int d, int L, int Lq, int ld, int pad, int ldq, int ncols) {
    const int q4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (q4 >= ncols) return;
    const int row = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const bool is_x = row < C;
    const float* src = is_x ? x + (size_t)b * x_bstride + (size_t)row * ld + pad
                            : h2 + (size_t)b * h_bstride + (size_t)(row - C) * ld + pad;
    float tap[6][4];                                                  // tap[j][e] = x[t_0(q4 + e) + (j - 1) d]
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) tap[j][e] = 0.f;
    [[maybe_unused]] auto ld4 = [&](int t) { return (t >= 0 && t < L) ? *reinterpret_cast<const float4*>(src + t) : make_float4(0.f, 0.f, 0.f, 0.f); };
    if constexpr (MODE == 1) {
        if (q4 < Lq) {
            const int t0 = (q4 / d) * 4 * d + q4 % d;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (!is_x && (j == 0 || j == 5)) continue;            // (cond rows: only the four members are copied)
                const float4 v = ld4(t0 + (j - 1) * d);
                tap[j][0] = v.x; tap[j][1] = v.y; tap[j][2] = v.z; tap[j][3] = v.w;
            }
        }
    } else if constexpr (MODE == 2) {
        if (q4 < Lq) {
            float a[24];                                              // x[4 q4 - 4 + i]
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const float4 v = ld4(4 * q4 - 4 + 4 * u);
                a[4 * u] = v.x; a[4 * u + 1] = v.y; a[4 * u + 2] = v.z; a[4 * u + 3] = v.w;
            }
            const bool hi = q4 + 2 < Lq;                              // columns q4 + 2, q4 + 3 (Lq is even)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                tap[j][0] = a[4 + (j - 1) * 2]; tap[j][1] = a[5 + (j - 1) * 2];
                tap[j][2] = hi ? a[12 + (j - 1) * 2] : 0.f; tap[j][3] = hi ? a[13 + (j - 1) * 2] : 0.f;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = q4 + e;
            const int t0 = (q / d) * 4 * d + q % d;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int t = t0 + (j - 1) * d;
                tap[j][e] = (q < Lq && t >= 0 && t < L && (is_x || (j >= 1 && j <= 4))) ? src[t] : 0.f;
            }
        }
    }
    if (is_x) {
        const size_t plane = (size_t)B * C * ldq;
        float* o = V + ((size_t)b * C + row) * ldq + q4;
        float v[6][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x0 = tap[0][e], x1 = tap[1][e], x2 = tap[2][e], x3 = tap[3][e], x4 = tap[4][e], x5 = tap[5][e];
            const float s12 = x1 + x2, d12 = x1 - x2, s34 = x3 + x4, d34 = x3 - x4, d13 = x1 - x3, d24 = x2 - x4;
            v[0][e] = 4.f * x0 - 5.f * x2 + x4;
            v[1][e] = s34 - 4.f * s12;
            v[2][e] = 4.f * d12 - d34;
            v[3][e] = -2.f * d13 - d24;
            v[4][e] = 2.f * d13 - d24;
            v[5][e] = 4.f * x1 - 5.f * x3 + x5;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) *reinterpret_cast<float4*>(o + j * plane) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
    } else {
        const size_t plane = (size_t)B * H * ldq;
        float* o = Hc + ((size_t)b * H + (row - C)) * ldq + q4;
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(o + k * plane) = make_float4(tap[k + 1][0], tap[k + 1][1], tap[k + 1][2], tap[k + 1][3]);
    }
}

// --------------------------------------------------- Winograd F(6,3) in-layer form ----
// The same conv on the output hex t_k = t_0 + k d, k = 0..5, from the eight taps x_j = x[t_0 + (j - 1) d], j = 0..7, with the
// interpolation points 0, +-1, +-2, +-1/2, inf:
//   e = x2 + x6 - 17/4 x4,  o = x1 + x5 - 17/4 x3:                 V1 = e + o,  V2 = e - o
//   e = 1/4 x2 - 5/4 x4 + x6,  o = 1/2 x1 - 5/2 x3 + 2 x5:         V3 = e + o,  V4 = e - o
//   e = 4 x2 - 5 x4 + x6,  o = 2 x1 - 5/2 x3 + 1/2 x5:             V5 = e + o,  V6 = e - o
//   V0 = x0 - x6 + 21/4 (x4 - x2)                                  V7 = x7 - x1 + 21/4 (x3 - x5)
//   U0 = W0   U1, U2 = -2/9 (W0 +- W1 + W2)   U3, U4 = W0 / 90 +- W1 / 45 + 2 W2 / 45   U5, U6 = 32/45 W0 +- 16/45 W1 + 8/45 W2   U7 = W2
//   P_j = U_j V_j, a = P1 + P2, b = P1 - P2, c = P3 + P4, e = P3 - P4, f = P5 + P6, g = P5 - P6:
//   u[t_0] = P0 + a + c + f          u[t_1] = b + 2 e + g / 2         u[t_2] = a + 4 c + f / 4
//   u[t_3] = b + 8 e + g / 8         u[t_4] = a + 16 c + f / 16       u[t_5] = b + 32 e + g / 32 + P7
// 8/6 C MACs per output and row.  Hex column q of a batch item stands for t_0 = (q / d) 6d + q % d; there are Lh = ceil(L / 6d) d.

// dense[j] = U_j, j = 0..7, as [rows][C] (in_w: [rows][C][3]); fp64 sums rounded once
__global__ __launch_bounds__(256) void winograd_g63_kernel(const float* __restrict__ in_w, float* __restrict__ dense, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const double w0 = in_w[(size_t)idx * 3], w1 = in_w[(size_t)idx * 3 + 1], w2 = in_w[(size_t)idx * 3 + 2];
    dense[idx] = in_w[(size_t)idx * 3];
    dense[(size_t)n + idx] = (float)(-2.0 * (w0 + w1 + w2) / 9.0);
    dense[2 * (size_t)n + idx] = (float)(-2.0 * (w0 - w1 + w2) / 9.0);
    dense[3 * (size_t)n + idx] = (float)(w0 / 90.0 + w1 / 45.0 + 2.0 * w2 / 45.0);
    dense[4 * (size_t)n + idx] = (float)(w0 / 90.0 - w1 / 45.0 + 2.0 * w2 / 45.0);
    dense[5 * (size_t)n + idx] = (float)(32.0 * w0 / 45.0 + 16.0 * w1 / 45.0 + 8.0 * w2 / 45.0);
    dense[6 * (size_t)n + idx] = (float)(32.0 * w0 / 45.0 - 16.0 * w1 / 45.0 + 8.0 * w2 / 45.0);
    dense[7 * (size_t)n + idx] = in_w[(size_t)idx * 3 + 2];
}

// x [B][C][ld] -> V0..V7 [8][B][C][ldh] in hex order (grid.y = C: the layer kernel reads the cond rows in place, the form runs
// where d % 4 == 0).  Zero outside [0, L); columns [Lh, ncols) are written as zeros.  One thread: four hex columns of one row.
// MODE 1: d % 4 == 0 and L % 4 == 0 - four consecutive time steps per tap, 16-byte aligned, all inside or all outside
// MODE 0: one column at a time
template <int MODE>
__global__ __launch_bounds__(256) void winograd_transform_hex_kernel(const float* __restrict__ x, long long x_bstride, float* __restrict__ V,
                                                                     int C, int d, int L, int Lh, int ld, int pad, int ldh, int ncols) {
    const int q4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (q4 >= ncols) return;
    const int row = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const float* src = x + (size_t)b * x_bstride + (size_t)row * ld + pad;
    float tap[8][4];                                                  // tap[j][e] = x[t_0(q4 + e) + (j - 1) d]
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) tap[j][e] = 0.f;
    if constexpr (MODE == 1) {
        if (q4 < Lh) {
            const int t0 = (q4 / d) * 6 * d + q4 % d;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = t0 + (j - 1) * d;
                if (t < 0 || t >= L) continue;
                const float4 v = *reinterpret_cast<const float4*>(src + t);
                tap[j][0] = v.x; tap[j][1] = v.y; tap[j][2] = v.z; tap[j][3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = q4 + e;
            const int t0 = (q / d) * 6 * d + q % d;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = t0 + (j - 1) * d;
                tap[j][e] = (q < Lh && t >= 0 && t < L) ? src[t] : 0.f;
            }
        }
    }
    const size_t plane = (size_t)B * C * ldh;
    float* o = V + ((size_t)b * C + row) * ldh + q4;
    float v[8][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x0 = tap[0][e], x1 = tap[1][e], x2 = tap[2][e], x3 = tap[3][e], x4 = tap[4][e], x5 = tap[5][e], x6 = tap[6][e], x7 = tap[7][e];
        const float e1 = (x2 + x6) - 4.25f * x4, o1 = (x1 + x5) - 4.25f * x3;
        const float e2 = (0.25f * x2 + x6) - 1.25f * x4, o2 = (0.5f * x1 + 2.f * x5) - 2.5f * x3;
        const float e3 = (4.f * x2 + x6) - 5.f * x4, o3 = (2.f * x1 + 0.5f * x5) - 2.5f * x3;
        v[0][e] = (x0 - x6) + 5.25f * (x4 - x2);
        v[1][e] = e1 + o1; v[2][e] = e1 - o1;
        v[3][e] = e2 + o2; v[4][e] = e2 - o2;
        v[5][e] = e3 + o3; v[6][e] = e3 - o3;
        v[7][e] = (x7 - x1) + 5.25f * (x3 - x5);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) *reinterpret_cast<float4*>(o + j * plane) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
}

// a16[b][r][:] over the whole padded row: r < H: audio[b][ch_off + r][n], r == H: 1, other rows 0; 0 outside [pad, pad + L)
template <int H>
__global__ __launch_bounds__(256) void wn_start_ones_kernel(const float* __restrict__ audio, float* __restrict__ a16, int G,
                                                            int ch_off, int L, int ld, int pad) {
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int b = blockIdx.z;
    if (col >= ld) return;
    const int n = col - pad;
    const bool in = n >= 0 && n < L;                           // pad, L multiples of 4: a float4 is all in or all out
    float* dst = a16 + (size_t)b * FOLD_ROWS * ld + col;
#pragma unroll
    for (int r = 0; r < FOLD_ROWS; ++r) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in && r < H) v = *reinterpret_cast<const float4*>(audio + ((size_t)b * G + ch_off + r) * L + n);
        else if (in && r == H) v = make_float4(1.f, 1.f, 1.f, 1.f);
        *reinterpret_cast<float4*>(dst + (size_t)r * ld) = v;
    }
}

// Skip/end pass of one skip group: e = sum_{j < nl} Wf_j . act_j over the group's kept gated activations (Wf_j = W_end . W_skip
// of layer j, [C][E]), first group: acc = e; later groups: e += acc, and then either acc = e, or (TAIL, the last group) e += b'
// and the flow tail of flow_tail_kernel.  Same reduction shape as flow_tail_kernel: 4 waves x 256 time steps, each wave a
// quarter of the channels of every layer, NG 16-byte loads in flight per lane, partial sums meet in LDS.  Every workgroup
// owns its columns: deterministic.  TAIL: SKEND_ACC (no tail), SKEND_TAIL, or SKEND_FWD - the forward direction's tail
// (coupling_forward; Winv, wave unused).
enum { SKEND_ACC = 0, SKEND_TAIL = 1, SKEND_FWD = 2 };
template <int H, int TAIL>
__global__ __launch_bounds__(256) void skip_end_kernel(const float* __restrict__ act, long long act_stride, int nl,
                                                       const float* __restrict__ Wf, float* __restrict__ acc, int first,
                                                       const float* __restrict__ bf, const float* __restrict__ Winv,
                                                       float* __restrict__ audio, float* __restrict__ wave,
                                                       int C, int G, int ch_off, int L, int ld, int pad, CouplingForward fw) {
    constexpr int E = 2 * H;
    constexpr int NG = E <= 4 ? 8 : E <= 8 ? 4 : 2;            // 16-byte loads per lane in flight (E x NG weights in SGPRs)
    __shared__ __attribute__((aligned(16))) float part[3][E][256];
    __shared__ float sWinv[E * E];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + lane * 4;
    if (TAIL == SKEND_TAIL && threadIdx.x < E * E) sWinv[threadIdx.x] = Winv[threadIdx.x];
    float4 e[E];
#pragma unroll
    for (int j = 0; j < E; ++j) e[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int cq = C / 4;                                       // a multiple of NG (C % 32 == 0)
    const int cbeg = __builtin_amdgcn_readfirstlane(wv * cq);
    for (int l = 0; l < nl; ++l) {
        // columns beyond L inside the padded row are readable (never used)
        const float* ob = act + (size_t)l * act_stride + (size_t)b * C * ld + pad + n;
        const float* wl = Wf + (size_t)l * C * E;
        for (int c = cbeg; c < cbeg + cq; c += NG) {
            float4 v[NG];
#pragma unroll
            for (int k = 0; k < NG; ++k) v[k] = *reinterpret_cast<const float4*>(ob + (size_t)(c + k) * ld);
#pragma unroll
            for (int k = 0; k < NG; ++k)
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const float w = wl[(c + k) * E + j];
                    e[j].x = fmaf(w, v[k].x, e[j].x); e[j].y = fmaf(w, v[k].y, e[j].y);
                    e[j].z = fmaf(w, v[k].z, e[j].z); e[j].w = fmaf(w, v[k].w, e[j].w);
                }
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < E; ++j) *reinterpret_cast<float4*>(&part[wv - 1][j][lane * 4]) = e[j];
    }
    __syncthreads();
    if (wv != 0 || (TAIL != SKEND_FWD && n >= L)) return;
    float* ab = acc + (size_t)b * E * ld + pad + n;
#pragma unroll
    for (int j = 0; j < E; ++j) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 pv = *reinterpret_cast<const float4*>(&part[q][j][lane * 4]);
            e[j].x += pv.x; e[j].y += pv.y; e[j].z += pv.z; e[j].w += pv.w;
        }
        if (!first) {
            const float4 pv = *reinterpret_cast<const float4*>(ab + (size_t)j * ld);
            e[j].x += pv.x; e[j].y += pv.y; e[j].z += pv.z; e[j].w += pv.w;
        }
    }
    if constexpr (TAIL == SKEND_ACC) {
#pragma unroll
        for (int j = 0; j < E; ++j) *reinterpret_cast<float4*>(ab + (size_t)j * ld) = e[j];
    } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const float bj = bf[j];
            e[j].x += bj; e[j].y += bj; e[j].z += bj; e[j].w += bj;
        }
        if constexpr (TAIL == SKEND_FWD) coupling_forward<H>(e, audio, fw, b, G, ch_off, L, n);
        else coupling_tail<H>(e, sWinv, audio, wave, b, G, ch_off, L, n);
    }
}

}  // namespace

// ----------------------------------------------------------------- host launchers ----

int launch_fold_weightnorm(const float* v, const float* g, float* w, int out_ch, int fan, hipStream_t s) {
    CTTS_CHECK_ARG(out_ch > 0 && fan > 0, "fold_weightnorm: out_ch=%d fan=%d", out_ch, fan);
    hipLaunchKernelGGL(fold_weightnorm_kernel, dim3(out_ch), dim3(256), 0, s, v, g, w, fan);
    CTTS_CHECK_LAUNCH("fold_weightnorm");
    return CTTS_OK;
}

int launch_pack_a(float* dst, const float* src, int bm, int MB, int nch_total, int k_off, int ksrc, int epi, int C, int M,
                  long long src_row_off, long long src_row_stride, int src_k_stride, hipStream_t s, int k_group,
                  int k_member) {
    CTTS_CHECK_ARG(k_off >= 0 && ksrc > 0 && k_off + ksrc * (k_group > 1 ? k_group : 1) <= nch_total * GEMM_KC,
                   "pack_a: k range");
    CTTS_CHECK_ARG(k_group <= 1 || (ksrc % GEMM_KC == 0 && k_member >= 0 && k_member < k_group), "pack_a: k group");
    hipLaunchKernelGGL(pack_a_kernel, dim3(ksrc, MB), dim3(256), 0, s, dst, src, bm, nch_total, k_off, ksrc, epi, C, M,
                       src_row_off, src_row_stride, src_k_stride, k_group, k_member);
    CTTS_CHECK_LAUNCH("pack_a");
    return CTTS_OK;
}

int launch_pack_bias(float* dst, int bm, int MB, const float* src0, long long off0, const float* src1, long long off1,
                     int epi, int C, int M, hipStream_t s) {
    hipLaunchKernelGGL(pack_bias_kernel, dim3(MB), dim3(256), 0, s, dst, bm, src0, off0, src1, off1, epi, C, M);
    CTTS_CHECK_LAUNCH("pack_bias");
    return CTTS_OK;
}

bool upsample_mfma_shape(int n_mel, int win, int hop, int G) {
    return n_mel == UM_NMEL && hop == UM_HOP && win == UM_HOP * UM_TAPS && G == UM_G;
}

int launch_upsample_pack_mfma(const float* W, float* Wp, hipStream_t s) {
    const size_t n = (size_t)UM_NMEL * UM_NMEL * UM_HOP * UM_TAPS;
    hipLaunchKernelGGL(upsample_pack_mfma_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, Wp);
    CTTS_CHECK_LAUNCH("upsample_pack_mfma");
    return CTTS_OK;
}

int launch_upsample_squeeze(const float* mel, const float* W, const float* Wp, const float* bias, float* spect, int batch,
                            int n_mel, int F, int win, int hop, int G, int ld, int pad, hipStream_t s) {
    CTTS_CHECK_ARG(win % hop == 0 && hop % G == 0, "upsample_squeeze: win %d hop %d n_group %d", win, hop, G);
    if (Wp && upsample_mfma_shape(n_mel, win, hop, G) && ld % 4 == 0 && pad % 4 == 0 && (reinterpret_cast<uintptr_t>(spect) & 15) == 0 &&
        !tuning().up_no_mfma) {
        // chunks of <= 320 frames, equal up to a 16-frame tile (900 frames: 304 + 304 + 292): 80 x 3 workgroups per utterance
        const int nchunks = (F + UM_CHUNK_MAX - 1) / UM_CHUNK_MAX;
        const int chunk = ((F + nchunks - 1) / nchunks + 15) / 16 * 16;
        const int srow = (chunk + 31) / 32 * 32 + 4;           // frames f0 - 3 ... f0 + (chunk rounded to a pair of tiles)
        const int lds = UM_NMEL * srow * (int)sizeof(float);
        // the largest chunk's bytes, so that one opt-in serves every length (allow_dynamic_lds)
        int rc;
        if (lds > 64 * 1024 && (rc = CTTS_ALLOW_LDS(upsample_squeeze_mfma_kernel, UM_NMEL * (UM_CHUNK_MAX + 4) * (int)sizeof(float)))) return rc;
        hipLaunchKernelGGL(upsample_squeeze_mfma_kernel, dim3(UM_NMEL, (unsigned)(batch * nchunks)), dim3(512), lds, s, mel, Wp, bias,
                           spect, F, chunk, nchunks, srow, ld, pad);
        CTTS_CHECK_LAUNCH("upsample_squeeze_mfma");
        return CTTS_OK;
    }
    if (hop != 256 || G != 8) {
        dim3 ggrid((unsigned)(((long long)F * hop + 255) / 256), n_mel, batch);
        hipLaunchKernelGGL(upsample_squeeze_generic_kernel, ggrid, dim3(256), 0, s, mel, W, bias, spect, n_mel, F, win, hop, G, ld, pad);
        CTTS_CHECK_LAUNCH("upsample_squeeze_generic");
        return CTTS_OK;
    }
    const int taps = win / hop;
    const size_t smem = ((size_t)n_mel * (UP_UQ + taps - 1) + (size_t)(UP_UO / 2) * G * (UP_UQ * (hop / G) + 8)) * sizeof(float);
    CTTS_CHECK_ARG(smem <= 64 * 1024, "upsample_squeeze: LDS %zu", smem);
    dim3 grid((F + UP_UQ - 1) / UP_UQ, (n_mel + UP_UO - 1) / UP_UO, batch);
    hipLaunchKernelGGL((upsample_squeeze_kernel<256, 8>), grid, dim3(256), smem, s, mel, W, bias, spect, n_mel, F,
                       win, ld, pad);
    CTTS_CHECK_LAUNCH("upsample_squeeze");
    return CTTS_OK;
}

int launch_wn_start(const float* audio, const float* Ws, const float* bs, float* x, int batch, int C, int G,
                    int ch_off, int n_half, int L, int ld, int pad, hipStream_t s) {
    CTTS_CHECK_ARG(L % 4 == 0, "wn_start: L=%d not a multiple of 4", L);
    dim3 grid((L / 4 + 255) / 256, (C + 31) / 32, batch);
#define CTTS_START_CASE(H)                                                                                     \
    case H:                                                                                                    \
        hipLaunchKernelGGL(wn_start_kernel<H>, grid, dim3(256), 0, s, audio, Ws, bs, x, C, G, ch_off, L, ld,   \
                           pad);                                                                               \
        break;
    switch (n_half) {
        CTTS_START_CASE(1) CTTS_START_CASE(2) CTTS_START_CASE(3) CTTS_START_CASE(4)
        CTTS_START_CASE(5) CTTS_START_CASE(6) CTTS_START_CASE(7) CTTS_START_CASE(8)
        default:
            set_error("wn_start: n_half=%d unsupported (1..8)", n_half);
            return CTTS_E_ARG;
    }
#undef CTTS_START_CASE
    CTTS_CHECK_LAUNCH("wn_start");
    return CTTS_OK;
}

int launch_flow_tail(const float* out, float* audio, float* wave, const float* Wend, const float* bend,
                     const float* Winv, int batch, int C, int G, int ch_off, int n_half, int L, int ld, int pad,
                     hipStream_t s, const CouplingForward* fwd) {
    CTTS_CHECK_ARG(L % 4 == 0 && C % 4 == 0, "flow_tail: L=%d C=%d", L, C);
    CTTS_CHECK_ARG(fwd == nullptr || (fwd->part != nullptr && wave == nullptr), "flow_tail: forward direction needs the partial sums");
    const CouplingForward fw = fwd ? *fwd : CouplingForward{};
    CTTS_CHECK_ARG(wave == nullptr || (ch_off == 0 && 2 * n_half == G && G % 4 == 0),
                   "flow_tail: un-squeeze needs the full group (ch_off=%d n_half=%d G=%d)", ch_off, n_half, G);
    dim3 grid((L + 255) / 256, batch);
#define CTTS_TAIL_CASE(H)                                                                                       \
    case H:                                                                                                     \
        if (fwd)                                                                                                \
            hipLaunchKernelGGL((flow_tail_kernel<H, true>), grid, dim3(256), 0, s, out, audio, wave, Wend, bend, Winv, C, G, \
                               ch_off, L, ld, pad, fw);                                                         \
        else                                                                                                    \
            hipLaunchKernelGGL((flow_tail_kernel<H, false>), grid, dim3(256), 0, s, out, audio, wave, Wend, bend, Winv, C, G, \
                               ch_off, L, ld, pad, fw);                                                         \
        break;
    switch (n_half) {
        CTTS_TAIL_CASE(1) CTTS_TAIL_CASE(2) CTTS_TAIL_CASE(3) CTTS_TAIL_CASE(4)
        CTTS_TAIL_CASE(5) CTTS_TAIL_CASE(6) CTTS_TAIL_CASE(7) CTTS_TAIL_CASE(8)
        default:
            set_error("flow_tail: n_half=%d unsupported (1..8)", n_half);
            return CTTS_E_ARG;
    }
#undef CTTS_TAIL_CASE
    CTTS_CHECK_LAUNCH("flow_tail");
    return CTTS_OK;
}

int launch_fold_in0(const float* in_w, const float* Ws, const float* bs, float* dst, int C, int n_half, int ks, hipStream_t s) {
    CTTS_CHECK_ARG(n_half >= 1 && n_half < FOLD_ROWS, "fold_in0: n_half=%d", n_half);
    const int n = 2 * C * FOLD_ROWS * ks;
    hipLaunchKernelGGL(fold_in0_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in_w, Ws, bs, dst, C, n_half, ks, 2 * C);
    CTTS_CHECK_LAUNCH("fold_in0");
    return CTTS_OK;
}

int launch_fold_skend(const float* const* rs_w, const float* const* rs_b, const float* Wend, const float* bend, float* Wf,
                      float* bf, int C, int n_layers, int n_half, hipStream_t s) {
    const int E = 2 * n_half;
    CTTS_CHECK_ARG(n_layers >= 1 && n_layers <= 12 && E <= 64, "fold_skend: n_layers=%d n_half=%d", n_layers, n_half);
    SkipBiasPtrs sb{};
    for (int i = 0; i < n_layers; ++i) {
        CTTS_CHECK_ARG(rs_w[i] && rs_b[i], "fold_skend: NULL layer %d weights", i);
        const int row_off = i < n_layers - 1 ? C : 0;          // skip rows: [C, 2C), or all C rows of the last layer
        sb.p[i] = rs_b[i];
        sb.row_off[i] = row_off;
        hipLaunchKernelGGL(fold_skend_w_kernel, dim3((C * E + 255) / 256), dim3(256), 0, s, Wend, rs_w[i], Wf + (size_t)i * C * E,
                           C, E, row_off);
    }
    hipLaunchKernelGGL(fold_skend_b_kernel, dim3(1), dim3(64), 0, s, Wend, bend, sb, n_layers, bf, C, E);
    CTTS_CHECK_LAUNCH("fold_skend");
    return CTTS_OK;
}

int launch_winograd_g(const float* in_w, float* dense, int rows, int C, hipStream_t s) {
    const int n = rows * C;
    hipLaunchKernelGGL(winograd_g_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in_w, dense, n);
    CTTS_CHECK_LAUNCH("winograd_g");
    return CTTS_OK;
}

int launch_winograd_transform(const float* x, long long x_bstride, const float* h2, long long h_bstride, float* V, float* Hc,
                              int batch, int C, int H, int d, int L, int Lp, int ld, int pad, int ldp, int ncols, bool cond_rows,
                              bool vec_d2, hipStream_t s) {
    CTTS_CHECK_ARG(d >= 1 && Lp % d == 0 && (long long)Lp * 2 >= L && Lp <= ncols && ncols <= ldp && ncols % 4 == 0 && ldp % 4 == 0 &&
                       ld % 4 == 0 && pad % 4 == 0 && pad + L <= ld,
                   "winograd_transform: d=%d L=%d Lp=%d ncols=%d ldp=%d ld=%d pad=%d", d, L, Lp, ncols, ldp, ld, pad);
    dim3 grid((ncols / 4 + 255) / 256, cond_rows ? C + H : C, batch);
    if (d % 4 == 0 && L % 4 == 0)
        hipLaunchKernelGGL(winograd_transform_kernel<1>, grid, dim3(256), 0, s, x, x_bstride, h2, h_bstride, V, Hc, C, H, d, L, Lp,
                           ld, pad, ldp, ncols);
    else if (d == 2 && L % 4 == 0 && vec_d2)
        hipLaunchKernelGGL(winograd_transform_kernel<2>, grid, dim3(256), 0, s, x, x_bstride, h2, h_bstride, V, Hc, C, H, d, L, Lp,
                           ld, pad, ldp, ncols);
    else
        hipLaunchKernelGGL(winograd_transform_kernel<0>, grid, dim3(256), 0, s, x, x_bstride, h2, h_bstride, V, Hc, C, H, d, L, Lp,
                           ld, pad, ldp, ncols);
    CTTS_CHECK_LAUNCH("winograd_transform");
    return CTTS_OK;
}

int launch_winograd_g43(const float* in_w, float* dense, int rows, int C, hipStream_t s) {
    const int n = rows * C;
    hipLaunchKernelGGL(winograd_g43_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in_w, dense, n);
    CTTS_CHECK_LAUNCH("winograd_g43");
    return CTTS_OK;
}

int launch_winograd_transform_quad(const float* x, long long x_bstride, const float* h2, long long h_bstride, float* V, float* Hc,
                                   int batch, int C, int H, int d, int L, int Lq, int ld, int pad, int ldq, int ncols, bool cond_rows,
                                   hipStream_t s) {
    CTTS_CHECK_ARG(d >= 1 && Lq % d == 0 && (long long)Lq * 4 >= L && Lq <= ncols && ncols <= ldq && ncols % 4 == 0 && ldq % 4 == 0 &&
                       ld % 4 == 0 && pad % 4 == 0 && pad + L <= ld && (!cond_rows || Hc != nullptr),
                   "winograd_transform_quad: d=%d L=%d Lq=%d ncols=%d ldq=%d ld=%d pad=%d", d, L, Lq, ncols, ldq, ld, pad);
    dim3 grid((ncols / 4 + 255) / 256, cond_rows ? C + H : C, batch);
    if (d % 4 == 0 && L % 4 == 0)
        hipLaunchKernelGGL(winograd_transform_quad_kernel<1>, grid, dim3(256), 0, s, x, x_bstride, h2, h_bstride, V, Hc, C, H, d, L, Lq,
                           ld, pad, ldq, ncols);
    else if (d == 2 && L % 4 == 0)
        hipLaunchKernelGGL(winograd_transform_quad_kernel<2>, grid, dim3(256), 0, s, x, x_bstride, h2, h_bstride, V, Hc, C, H, d, L, Lq,
                           ld, pad, ldq, ncols);
    else
        hipLaunchKernelGGL(winograd_transform_quad_kernel<0>, grid, dim3(256), 0, s, x, x_bstride, h2, h_bstride, V, Hc, C, H, d, L, Lq,
                           ld, pad, ldq, ncols);
    CTTS_CHECK_LAUNCH("winograd_transform_quad");
    return CTTS_OK;
}

int launch_winograd_g63(const float* in_w, float* dense, int rows, int C, hipStream_t s) {
    const int n = rows * C;
    hipLaunchKernelGGL(winograd_g63_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in_w, dense, n);
    CTTS_CHECK_LAUNCH("winograd_g63");
    return CTTS_OK;
}

int launch_winograd_transform_hex(const float* x, long long x_bstride, float* V, int batch, int C, int d, int L, int Lh, int ld, int pad,
                                  int ldh, int ncols, hipStream_t s) {
    CTTS_CHECK_ARG(d >= 1 && Lh % d == 0 && (long long)Lh * 6 >= L && Lh <= ncols && ncols <= ldh && ncols % 4 == 0 && ldh % 4 == 0 &&
                       ld % 4 == 0 && pad % 4 == 0 && pad + L <= ld,
                   "winograd_transform_hex: d=%d L=%d Lh=%d ncols=%d ldh=%d ld=%d pad=%d", d, L, Lh, ncols, ldh, ld, pad);
    dim3 grid((ncols / 4 + 255) / 256, C, batch);
    if (d % 4 == 0 && L % 4 == 0)
        hipLaunchKernelGGL(winograd_transform_hex_kernel<1>, grid, dim3(256), 0, s, x, x_bstride, V, C, d, L, Lh, ld, pad, ldh, ncols);
    else
        hipLaunchKernelGGL(winograd_transform_hex_kernel<0>, grid, dim3(256), 0, s, x, x_bstride, V, C, d, L, Lh, ld, pad, ldh, ncols);
    CTTS_CHECK_LAUNCH("winograd_transform_hex");
    return CTTS_OK;
}

int launch_wn_start_ones(const float* audio, float* a16, int batch, int G, int ch_off, int n_half, int L, int ld, int pad,
                         hipStream_t s) {
    CTTS_CHECK_ARG(L % 4 == 0 && ld % 4 == 0 && pad % 4 == 0, "wn_start_ones: L=%d ld=%d pad=%d", L, ld, pad);
    dim3 grid((ld / 4 + 255) / 256, 1, batch);
#define CTTS_ONES_CASE(H)                                                                                     \
    case H:                                                                                                   \
        hipLaunchKernelGGL(wn_start_ones_kernel<H>, grid, dim3(256), 0, s, audio, a16, G, ch_off, L, ld, pad); \
        break;
    switch (n_half) {
        CTTS_ONES_CASE(1) CTTS_ONES_CASE(2) CTTS_ONES_CASE(3) CTTS_ONES_CASE(4)
        CTTS_ONES_CASE(5) CTTS_ONES_CASE(6) CTTS_ONES_CASE(7) CTTS_ONES_CASE(8)
        default:
            set_error("wn_start_ones: n_half=%d unsupported (1..8)", n_half);
            return CTTS_E_ARG;
    }
#undef CTTS_ONES_CASE
    CTTS_CHECK_LAUNCH("wn_start_ones");
    return CTTS_OK;
}

int launch_skip_end(const float* act, long long act_stride, int nl, const float* Wf, float* acc, bool first, bool tail,
                    const float* bf, const float* Winv, float* audio, float* wave, int batch, int C, int G, int ch_off,
                    int n_half, int L, int ld, int pad, hipStream_t s, const CouplingForward* fwd) {
    CTTS_CHECK_ARG(fwd == nullptr || (tail && fwd->part != nullptr && wave == nullptr), "skip_end: forward direction on the tail pass only");
    const CouplingForward fw = fwd ? *fwd : CouplingForward{};
    CTTS_CHECK_ARG(L % 4 == 0 && C % 32 == 0 && ld % 4 == 0 && pad % 4 == 0 && nl >= 1, "skip_end: L=%d C=%d nl=%d", L, C, nl);
    CTTS_CHECK_ARG(acc != nullptr || (first && tail), "skip_end: a group after the first needs the accumulator");
    CTTS_CHECK_ARG(!tail || wave == nullptr || (ch_off == 0 && 2 * n_half == G && G % 4 == 0),
                   "skip_end: un-squeeze needs the full group (ch_off=%d n_half=%d G=%d)", ch_off, n_half, G);
    dim3 grid((L + 255) / 256, batch);
    const int fi = first ? 1 : 0;
#define CTTS_SKEND_CASE(H)                                                                                                \
    case H:                                                                                                               \
        if (fwd)                                                                                                          \
            hipLaunchKernelGGL((skip_end_kernel<H, SKEND_FWD>), grid, dim3(256), 0, s, act, act_stride, nl, Wf, acc, fi, bf, Winv, \
                               audio, wave, C, G, ch_off, L, ld, pad, fw);                                                \
        else if (tail)                                                                                                    \
            hipLaunchKernelGGL((skip_end_kernel<H, SKEND_TAIL>), grid, dim3(256), 0, s, act, act_stride, nl, Wf, acc, fi, bf, Winv, \
                               audio, wave, C, G, ch_off, L, ld, pad, fw);                                                \
        else                                                                                                              \
            hipLaunchKernelGGL((skip_end_kernel<H, SKEND_ACC>), grid, dim3(256), 0, s, act, act_stride, nl, Wf, acc, fi, bf, Winv, \
                               audio, wave, C, G, ch_off, L, ld, pad, fw);                                                \
        break;
    switch (n_half) {
        CTTS_SKEND_CASE(1) CTTS_SKEND_CASE(2) CTTS_SKEND_CASE(3) CTTS_SKEND_CASE(4)
        CTTS_SKEND_CASE(5) CTTS_SKEND_CASE(6) CTTS_SKEND_CASE(7) CTTS_SKEND_CASE(8)
        default:
            set_error("skip_end: n_half=%d unsupported (1..8)", n_half);
            return CTTS_E_ARG;
    }
#undef CTTS_SKEND_CASE
    CTTS_CHECK_LAUNCH("skip_end");
    return CTTS_OK;
}

int launch_flow_head_forward(const float* W, const float* wave, float* z, int batch, int G, int ch_off, int n_rem, int L,
                             hipStream_t s) {
    CTTS_CHECK_ARG(L % 4 == 0 && n_rem >= 2 && n_rem % 2 == 0 && ch_off >= 0 && ch_off + n_rem == G,
                   "flow_head_forward: L=%d n_rem=%d ch_off=%d G=%d", L, n_rem, ch_off, G);
    CTTS_CHECK_ARG(wave == nullptr || (ch_off == 0 && G % 4 == 0), "flow_head_forward: the squeeze needs the full group (ch_off=%d G=%d)",
                   ch_off, G);
    dim3 grid((L / 4 + 255) / 256, batch);
#define CTTS_HEAD_LAUNCH(EE, SQ) \
    hipLaunchKernelGGL((flow_head_forward_kernel<EE, SQ>), grid, dim3(256), 0, s, W, wave, z, G, ch_off, L)
#define CTTS_HEAD_CASE(EE)             \
    case EE:                           \
        CTTS_HEAD_LAUNCH(EE, false);   \
        break;
#define CTTS_HEAD_CASE_SQ(EE)                                                       \
    case EE:                                                                        \
        if (wave) CTTS_HEAD_LAUNCH(EE, true); else CTTS_HEAD_LAUNCH(EE, false);     \
        break;
    switch (n_rem) {
        CTTS_HEAD_CASE(2) CTTS_HEAD_CASE_SQ(4) CTTS_HEAD_CASE(6) CTTS_HEAD_CASE_SQ(8)
        CTTS_HEAD_CASE(10) CTTS_HEAD_CASE_SQ(12) CTTS_HEAD_CASE(14) CTTS_HEAD_CASE_SQ(16)
        default:
            set_error("flow_head_forward: n_rem=%d unsupported (2..16, even)", n_rem);
            return CTTS_E_ARG;
    }
#undef CTTS_HEAD_CASE_SQ
#undef CTTS_HEAD_CASE
#undef CTTS_HEAD_LAUNCH
    CTTS_CHECK_LAUNCH("flow_head_forward");
    return CTTS_OK;
}

int launch_sumsq_partials(const float* z, double* part, int batch, long long n_item, int nblk, hipStream_t s) {
    CTTS_CHECK_ARG(n_item > 0 && n_item % 4 == 0 && (long long)nblk * FWD_SUMSQ_CHUNK >= n_item, "sumsq_partials: n=%lld nblk=%d",
                   n_item, nblk);
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3(nblk, batch), dim3(256), 0, s, z, part, n_item, nblk);
    CTTS_CHECK_LAUNCH("sumsq_partials");
    return CTTS_OK;
}

int launch_sum_partials(const double* part, long long part_bstride, long long part_kstride, int n, double* out, int out_bstride,
                        int nk, int batch, hipStream_t s) {
    CTTS_CHECK_ARG(n >= 1 && nk >= 1, "sum_partials: n=%d nk=%d", n, nk);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(nk, batch), dim3(64), 0, s, part, part_bstride, part_kstride, n, out, out_bstride);
    CTTS_CHECK_LAUNCH("sum_partials");
    return CTTS_OK;
}

}  // namespace ctts
