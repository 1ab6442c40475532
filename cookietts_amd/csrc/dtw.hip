// DTW on the device: time-warp a batch of predicted mels onto the ground truth (_4_mtw/waveglow/mel2samp.py:81-118).
//
// For every frame t of an item the reference tries s * r candidates - the zero-padded prediction, linearly interpolated to s times its
// length (F.interpolate, align_corners=False), read at expanded index j + t * s - in ascending j and keeps a candidate only when its
// sum_c |cand - target| is strictly below the running best's, which starts as the unshifted frame.  Here that is ONE launch for the batch:
//
//   * a workgroup owns 64 consecutive frames of one item (lanes along t: target and pred are read coalesced) and its four waves own a
//     quarter of the channels each ("slice");
//   * per channel a wave puts the 64 + r + 1 padded pred values its frames touch into its own LDS row, and every lane forms all s * r
//     candidates from a two-value window that slides over that row (r + 2 LDS reads per channel, the candidates themselves from
//     registers); the L1 of candidate j is summed in accumulator j, channel ascending;
//   * the slices' partial sums meet in LDS and wave 0 adds them slice ascending, selects with the `<` rule and publishes the choice;
//   * every wave then writes its channels of the winning frame, formed by the same two products and one sum as the candidate that was
//     scored (-ffp-contract=off: a fused form would change which candidate wins a tie, and the frame that is written).
//
// No atomics, no second launch, no workspace; the same input gives the same bits on every run.  The (i0 offset, 1 - lambda, lambda) triple
// of each j is formed on the host in fp32 and travels in the kernel arguments; only the two end clamps are decided per frame.
#include "common.h"

#include <cmath>

namespace ctts {
namespace {

constexpr int DTW_MAX_CAND = 64;                       // s * r of an accepted call
constexpr int DTW_WAVES = 4;
constexpr int DTW_ROW = 64 + DTW_MAX_CAND + 4;         // a wave's LDS row: 64 frames + r + 1 neighbours (r <= 63)

struct DtwTable {
    int off[DTW_MAX_CAND];                             // i0 - t: -1 .. r - 1, non-decreasing in j by steps of 0 or 1
    float w0[DTW_MAX_CAND];                            // 1 - lambda
    float w1[DTW_MAX_CAND];                            // lambda
};

struct DtwArgs {
    const float* pred;
    const float* target;
    const int* lengths;
    float* out;
    int* choice;
    float* l1;
    int B, C, T, s, r;
    DtwTable tab;
};

// What mel2samp.py:104-105 hands the interpolation at padded index i of an item of `len` frames: h zero frames, the item, h zero frames;
// i1 = min(i0 + 1, Tp - 1) is the upper end clamp.  Never reads outside [0, len).
__device__ __forceinline__ float dtw_padded(const float* row, int i, int h, int len) {
    i = min(i, len + 2 * h - 1);
    const int q = i - h;
    return (q >= 0 && q < len) ? row[q] : 0.f;
}

// the table's offset of candidate j as integer arithmetic: floor((j + 0.5) / S - 0.5).  The compile-time variants are launched only
// when the host's fp32 table agrees with it at every j.
template <int S>
__host__ __device__ constexpr int dtw_off_exact(int j) {
    return (2 * j + 1 - S) >= 0 ? (2 * j + 1 - S) / (2 * S) : -((S - 2 * j - 1 + 2 * S - 1) / (2 * S));
}

__device__ __forceinline__ void dtw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// S == 0: the generic form (s, r from the arguments, 64 guarded accumulators).  S > 0: s * r accumulators, offsets known to the compiler.
template <int S, int R>
__global__ __launch_bounds__(64 * DTW_WAVES) void mel_dtw_kernel(const DtwArgs a) {
    constexpr int NCMAX = S ? S * R : DTW_MAX_CAND;
    extern __shared__ float part[];                    // [DTW_WAVES - 1][nc + 1][64]: the partial sums of slices 1 .. 3
    __shared__ float rows[DTW_WAVES][DTW_ROW];
    __shared__ int tab_off[DTW_MAX_CAND];
    __shared__ float tab_w0[DTW_MAX_CAND], tab_w1[DTW_MAX_CAND];
    __shared__ int choice_s[64];

    const int s = S ? S : a.s, r = S ? R : a.r;
    const int nc = s * r, nk = nc + 1, h = r / 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, t0 = blockIdx.x * 64, t = t0 + lane;
    const int C = a.C, T = a.T;
    int len = a.lengths ? a.lengths[b] : T;
    len = min(max(len, 1), T);                         // a device-side length nobody could check: the nearest bound
    const bool live = t0 < len;                        // (workgroup-uniform) some frame of this tile belongs to the item
    const bool is0 = t == 0;
    const size_t item = size_t(b) * C * T;
    const int cs = (C + DTW_WAVES - 1) / DTW_WAVES;
    const int c_lo = min(wave * cs, C), c_hi = min(c_lo + cs, C);

    if (threadIdx.x < DTW_MAX_CAND) {
        tab_off[threadIdx.x] = a.tab.off[threadIdx.x];
        tab_w0[threadIdx.x] = a.tab.w0[threadIdx.x];
        tab_w1[threadIdx.x] = a.tab.w1[threadIdx.x];
    }
    if (threadIdx.x < 64) choice_s[threadIdx.x] = -1;
    __syncthreads();

    if (live) {
        float acc[NCMAX + 1];
#pragma unroll
        for (int k = 0; k <= NCMAX; ++k) acc[k] = 0.f;
        float* row = rows[wave];
        // the next channel's values travel while this one's candidates are formed
        float na = 0.f, nb = 0.f, ntg = 0.f;
        if (c_lo < c_hi) {
            const float* pr = a.pred + item + size_t(c_lo) * T;
            na = dtw_padded(pr, t - 1, h, len);
            if (lane < r + 1) nb = dtw_padded(pr, t + 63, h, len);
            if (t < len) ntg = a.target[item + size_t(c_lo) * T + t];
        }
        for (int c = c_lo; c < c_hi; ++c) {
            row[lane] = na;                            // row[k] = padded pred at index t0 - 1 + k
            if (lane < r + 1) row[lane + 64] = nb;
            const float tg = ntg;
            // generic form: the table is re-read from LDS per channel - 192 hoisted scalars would spill
            if (!S) asm volatile("" ::: "memory");
            if (c + 1 < c_hi) {
                const float* pr = a.pred + item + size_t(c + 1) * T;
                na = dtw_padded(pr, t - 1, h, len);
                if (lane < r + 1) nb = dtw_padded(pr, t + 63, h, len);
                if (t < len) ntg = a.target[item + size_t(c + 1) * T + t];
            }
            dtw_wave_sync();
            acc[0] += fabsf(row[lane + h + 1] - tg);   // the unshifted frame
            int cur = S ? dtw_off_exact<S ? S : 1>(0) : __builtin_amdgcn_readfirstlane(tab_off[0]);
            float x0 = row[lane + cur + 1], x1 = row[lane + cur + 2];
            // lower end clamp (src < 0 -> src = 0): frame 0 reads P[0] with weight 1 and P[1] with weight 0
            float xl0 = x0, xl1 = x1;
            if (cur < 0) {
                const float x2 = row[lane + 2];
                xl0 = is0 ? x1 : x0;
                xl1 = is0 ? x2 : x1;
            }
#pragma unroll
            for (int j = 0; j < NCMAX; ++j) {
                if (S || j < nc) {
                    const int o = S ? dtw_off_exact<S ? S : 1>(j) : __builtin_amdgcn_readfirstlane(tab_off[j]);
                    if (o != cur) {
                        x0 = x1;
                        x1 = row[lane + o + 2];
                        cur = o;
                    }
                    float w0 = S ? a.tab.w0[j] : tab_w0[j], w1 = S ? a.tab.w1[j] : tab_w1[j], xa = x0, xb = x1;
                    if (o < 0) {
                        w0 = is0 ? 1.f : w0;
                        w1 = is0 ? 0.f : w1;
                        xa = xl0;
                        xb = xl1;
                    }
                    const float cand = w0 * xa + w1 * xb;
                    acc[j + 1] += fabsf(cand - tg);
                }
            }
            dtw_wave_sync();                           // every read of the row is done before the next channel overwrites it
        }

        if (wave > 0) {
#pragma unroll
            for (int k = 0; k <= NCMAX; ++k)
                if (S || k < nk) part[(size_t(wave - 1) * nk + k) * 64 + lane] = acc[k];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k <= NCMAX; ++k)
                if (S || k < nk)
                    acc[k] = ((acc[k] + part[(size_t(0) * nk + k) * 64 + lane]) + part[(size_t(1) * nk + k) * 64 + lane]) +
                             part[(size_t(2) * nk + k) * 64 + lane];
            float best = acc[0];
            int ch = -1;
#pragma unroll
            for (int j = 0; j < NCMAX; ++j)
                if ((S || j < nc) && acc[j + 1] < best) {      // strictly: pred wins every tie, an earlier j a later one, NaN nothing
                    best = acc[j + 1];
                    ch = j;
                }
            const bool in = t < len;
            if (!in) ch = -1;
            choice_s[lane] = ch;
            if (t < T) {
                if (a.choice) a.choice[size_t(b) * T + t] = ch;
                if (a.l1) {
                    a.l1[(size_t(b) * 2 + 0) * T + t] = in ? acc[0] : 0.f;
                    a.l1[(size_t(b) * 2 + 1) * T + t] = in ? best : 0.f;
                }
            }
        }
    } else if (wave == 0 && t < T) {
        if (a.choice) a.choice[size_t(b) * T + t] = -1;
        if (a.l1) {
            a.l1[(size_t(b) * 2 + 0) * T + t] = 0.f;
            a.l1[(size_t(b) * 2 + 1) * T + t] = 0.f;
        }
    }
    __syncthreads();

    // the winning frame, this wave's channels
    const int ch = choice_s[lane];
    int off = 0;
    float w0 = 1.f, w1 = 0.f;
    if (ch >= 0) {
        off = tab_off[ch];
        w0 = tab_w0[ch];
        w1 = tab_w1[ch];
        if (is0 && off < 0) {
            off = 0;
            w0 = 1.f;
            w1 = 0.f;
        }
    }
    if (t < T) {
        for (int c = c_lo; c < c_hi; ++c) {
            const float* pr = a.pred + item + size_t(c) * T;
            float v = pr[t];
            if (ch >= 0) v = w0 * dtw_padded(pr, t + off, h, len) + w1 * dtw_padded(pr, t + off + 1, h, len);
            a.out[item + size_t(c) * T + t] = v;
        }
    }
}

template <int S, int R>
bool dtw_table_is_exact(const DtwTable& tab) {
    for (int j = 0; j < S * R; ++j)
        if (tab.off[j] != dtw_off_exact<S>(j)) return false;
    return true;
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

int dtw_run(const float* pred, const float* target, const int32_t* lengths, float* out, int32_t* choice, float* l1, int32_t B,
            int32_t C, int32_t T, int32_t scale_factor, int32_t range, void* stream, bool generic) {
    CTTS_CHECK_ARG(pred && target && out, "mel_dtw: NULL argument (pred, target and out are required)");
    CTTS_CHECK_ARG(B >= 1 && B <= 65535, "mel_dtw: batch=%d must lie in [1, 65535]", B);
    CTTS_CHECK_ARG(C >= 1, "mel_dtw: channels=%d must be at least 1", C);
    CTTS_CHECK_ARG(T >= 1, "mel_dtw: frames=%d must be at least 1", T);
    CTTS_CHECK_ARG(scale_factor >= 1, "mel_dtw: scale_factor=%d must be at least 1", scale_factor);
    CTTS_CHECK_ARG(range >= 1 && range % 2 == 1, "mel_dtw: range=%d must be an odd integer >= 1", range);
    CTTS_CHECK_ARG(int64_t(scale_factor) * range <= DTW_MAX_CAND, "mel_dtw: scale_factor * range = %lld candidates exceed %d",
                   (long long)(int64_t(scale_factor) * range), DTW_MAX_CAND);
    CTTS_CHECK_ARG(int64_t(T) + 64 + range < (int64_t(1) << 31) - 64, "mel_dtw: frames=%d too many", T);
    const size_t n = size_t(B) * C * T * sizeof(float);
    CTTS_CHECK_ARG(!overlap(out, n, pred, n), "mel_dtw: out aliases pred");
    CTTS_CHECK_ARG(!overlap(out, n, target, n), "mel_dtw: out aliases target");

    DtwArgs a{pred, target, lengths, out, choice, l1, B, C, T, scale_factor, range, {}};
    const int nc = scale_factor * range;
    const float rs = float(1.0 / double(scale_factor));
    for (int j = 0; j < DTW_MAX_CAND; ++j) {
        a.tab.off[j] = 0;
        a.tab.w0[j] = 1.f;
        a.tab.w1[j] = 0.f;
    }
    for (int j = 0; j < nc; ++j) {
        const float u = rs * (float(j) + 0.5f) - 0.5f;                 // the source index of expanded index j, before the clamp at 0
        const float fl = floorf(u);
        const float lam = u - fl;
        a.tab.off[j] = int(fl);
        a.tab.w1[j] = lam;
        a.tab.w0[j] = 1.f - lam;
        const int step = j ? a.tab.off[j] - a.tab.off[j - 1] : 0;
        if (a.tab.off[j] < -1 || a.tab.off[j] > range - 1 || step < 0 || step > 1) {
            set_error("mel_dtw: internal: offset table of (%d, %d) is not a unit staircase at j=%d", scale_factor, range, j);
            return CTTS_E_ARG;
        }
    }
    const dim3 grid((T + 63) / 64, B), block(64 * DTW_WAVES);
    const size_t lds = size_t(DTW_WAVES - 1) * (nc + 1) * 64 * sizeof(float);
    hipStream_t s = as_stream(stream);
    if (!generic && scale_factor == 8 && range == 5 && dtw_table_is_exact<8, 5>(a.tab))
        hipLaunchKernelGGL((mel_dtw_kernel<8, 5>), grid, block, lds, s, a);
    else if (!generic && scale_factor == 5 && range == 5 && dtw_table_is_exact<5, 5>(a.tab))
        hipLaunchKernelGGL((mel_dtw_kernel<5, 5>), grid, block, lds, s, a);
    else if (!generic && scale_factor == 5 && range == 3 && dtw_table_is_exact<5, 3>(a.tab))
        hipLaunchKernelGGL((mel_dtw_kernel<5, 3>), grid, block, lds, s, a);
    else
        hipLaunchKernelGGL((mel_dtw_kernel<0, 0>), grid, block, lds, s, a);
    CTTS_CHECK_LAUNCH("mel_dtw");
    return CTTS_OK;
}

}  // namespace
}  // namespace ctts

extern "C" {

int ctts_mel_dtw_f32(const float* pred, const float* target, const int32_t* lengths, float* out, int32_t* choice, float* l1,
                     int32_t batch, int32_t channels, int32_t frames, int32_t scale_factor, int32_t range, void* stream) {
    return ctts::dtw_run(pred, target, lengths, out, choice, l1, batch, channels, frames, scale_factor, range, stream, false);
}

int ctts_mel_dtw_generic_f32(const float* pred, const float* target, const int32_t* lengths, float* out, int32_t* choice, float* l1,
                             int32_t batch, int32_t channels, int32_t frames, int32_t scale_factor, int32_t range, void* stream) {
    return ctts::dtw_run(pred, target, lengths, out, choice, l1, batch, channels, frames, scale_factor, range, stream, true);
}

}  // extern "C"
