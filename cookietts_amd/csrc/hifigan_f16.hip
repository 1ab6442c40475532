// HiFi-GAN generator, IEEE-half storage mode (ctts_hifigan_*_f16 in include/cookietts_hip.h): the arithmetic of
// hifigan.hip with weights and every stored activation in IEEE half, products on v_mfma_f32_32x32x16_f16, accumulation,
// bias, residual add, the resblock mean and tanh in fp32, and ONE rounding to half (round-to-nearest-even, IEEE overflow
// to infinity, no clamping) per stored value.  The plan, the refusals, the sequence of launches, the launcher with its
// block shapes and the bodies of the entries are hifigan_plan.h's, shared with the other two formats; only the kernel with its
// half-unit epilogue and the pack kernel live here.
//
// Layout: activations are K8-blocked, [B][ceil(C / 8)][ld][8] halves with ld = L: the 8 channels 8g..8g+7 of one column
// are one 16-byte unit, which is exactly what a lane of the f16 MFMA wants as its 8 consecutive K values.  A workgroup
// stages, per chunk of KC input channels, KC / 8 rows of such units that are (ntap - 1) * dil columns wider than its output
// tile: units outside [0, L) and channels >= Cin (num_mels = 80 against KC = 32; the padding channels of a group of 8,
// which no store ever writes) are staged as exact zeros; LeakyReLU runs here - the stored half widened to fp32, times the
// fp32 slope, rounded once, which is what F.leaky_relu does on a half tensor - and a tap is a column offset of the
// fragment address: every fragment is one ds_read_b128 with consecutive lanes on consecutive units (conflict-free).
// conv_pre reads the fp32 mel rows instead and rounds each value once while staging.  The packed weights of the chunk
// ([ntap][KC / 8][BM] units) are staged beside the tile.
//
// Epilogue.  32x32 C/D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): for a register group q = r >> 2
// the lane holds channels 8q + 4 lhi + 0..3 of one column = half a unit, stored / read (residual, running sum) as 8 bytes.
// A transposed conv's rows are (phase, channel): with cout % 4 == 0 the four rows of a group share the phase and go to
// dst[co / 8][n * up + phase][co % 8 ..+3]; otherwise, and for a ragged last group of rows, the store is per element.
// HG_EPI_RES rounds v = acc + bias + float(res) once for dst0, and the stage's running sum as
// half((float(sum) + v) [/ n_k]) from the unrounded v.  HG_EPI_TANH writes the fp32 waveform.
//
// Block shapes are hifigan_plan.h's (256 threads = 4 waves, wave tile 32 MT x 64); KC = 32 where the two LDS images stay
// under HG_LDS_KC16 bytes, else 16.  A 128-column wave tile (blocks 32 x 512, 64 x 512, 128 x 256: a chunk's weights staged
// once for twice the columns, 6 fragment reads for 8 MFMAs instead of 4 for 4) was measured SLOWER, 25.0 against 20.4 ms at
// 16 x 900 frames: 176 VGPRs halve the workgroups per CU, and with no software pipeline in the main loop it is the other
// workgroups of the CU that cover a workgroup's staging.
// The K order of a column's sum does not depend on the block shape or the launch size
// (chunks in order, taps in order inside a chunk, the MFMA's own order inside a K16 step), so an item of a batch equals
// the same item run alone, bit for bit.
#include "hifigan_plan.h"

namespace ctts {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

using HgConvArgsH = HgConvArgsT<_Float16>;
using HgPackArgsH = HgPackArgsT<_Float16>;

// leaky_relu on a stored half: fp32 product with the fp32 slope, one rounding
__device__ __forceinline__ _Float16 hg_lrelu_h(_Float16 x, float slope) {
    return x >= (_Float16)0.0f ? x : (_Float16)(slope * (float)x);
}

template <int MT, int WM, int KC>
__global__ __launch_bounds__(256, 2) void hg_conv_f16_kernel(const HgConvArgsH a) {
    constexpr int WN = 4 / WM;
    constexpr int BM = 32 * MT * WM;
    constexpr int BN = 64 * WN;
    constexpr int KG = KC / 8;                                 // groups of 8 channels per chunk
    extern __shared__ __attribute__((aligned(16))) f16x8 hg_lds_h[];

    const int t = threadIdx.x;
    const auto [mb, tile, b, wm, wn, l31, lhi] = hg_tile<WM>(a);
    const int n0 = tile * BN;

    const int c0 = n0 - a.left;
    const int XW = BN + (a.ntap - 1) * a.dil;
    const int a_units = a.ntap * KG * BM;
    f16x8* As = hg_lds_h;
    f16x8* Xs = hg_lds_h + a_units;

    const f16x8* Ab = reinterpret_cast<const f16x8*>(a.A) + (size_t)mb * a.nch * a_units;
    const float slope = a.slope;
    const int cin_groups = (a.Cin + 7) >> 3;

    f32x16 acc[MT][2];
    hg_zero(acc);

    const int a_off = wm * (32 * MT) + l31;
    const int x_off = wn * 64 + l31;

    for (int ch = 0; ch < a.nch; ++ch) {
        __syncthreads();                                       // the previous chunk's fragments are read
        {   // weights of the chunk: one contiguous slab
            const f16x8* src = Ab + (size_t)ch * a_units;
            for (int u = t; u < a_units; u += 256) As[u] = src[u];
        }
        // input tile: KG rows x XW units, zeros outside [0, L) and beyond Cin, LeakyReLU applied here
        for (int u = t; u < KG * XW; u += 256) {
            const int g = u / XW;
            const int col = u - g * XW;
            const int cg = ch * KG + g;
            const int c = c0 + col;
            f16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.0f;
            if (cg < cin_groups && c >= 0 && c < a.L) {
                const int live = min(8, a.Cin - cg * 8);
                if (a.xf) {                                    // conv_pre: fp32 mel rows, one rounding each
                    const float* xr = a.xf + (size_t)b * a.x_bs + (size_t)cg * 8 * a.x_ld + c;
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < live) v[e] = (_Float16)xr[(size_t)e * a.x_ld];
                } else {
                    const f16x8 w = reinterpret_cast<const f16x8*>(a.x + (size_t)b * a.x_bs)[(size_t)cg * a.x_ld + c];
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < live) v[e] = hg_lrelu_h(w[e], slope);
                }
            }
            Xs[u] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < a.ntap; ++j) {
            const f16x8* Aj = As + j * (KG * BM) + a_off;
            const f16x8* Xj = Xs + x_off + j * a.dil;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                const int kg = 2 * ks + lhi;
                f16x8 av[MT], bv[2];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[mt] = Aj[kg * BM + mt * 32];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) bv[nt] = Xj[kg * XW + nt * 32];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: four rows m4..m4+3 (one half unit) of one column per step
    const float* bias = a.bias + mb * BM;
    const bool rows_by_4 = a.up > 1 ? (a.cout & 3) == 0 : true;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = n0 + wn * 64 + nt * 32 + l31;
            if (n >= a.L) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = wm * (32 * MT) + mt * 32 + 8 * q + 4 * lhi;
                const int m4 = mb * BM + row;
                if (m4 >= a.M) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[mt][nt][4 * q + e] + bias[row + e];
                if (a.epi == HG_EPI_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (m4 + e < a.M) a.dstf[(size_t)b * a.dst0_bs + (size_t)(m4 + e) * a.dst0_ld + n] = tanhf(v[e]);
                    continue;
                }
                const bool whole = rows_by_4 && m4 + 3 < a.M;
                if (a.epi == HG_EPI_STORE) {
                    if (whole) {
                        int mm = m4, nn = n;
                        if (a.up > 1) { const int ph = m4 / a.cout; mm = m4 - ph * a.cout; nn = n * a.up + ph; }
                        f16x4 h;
#pragma unroll
                        for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[e];
                        *reinterpret_cast<f16x4*>(a.dst0 + (size_t)b * a.dst0_bs + ((size_t)(mm >> 3) * a.dst0_ld + nn) * 8 + (mm & 7)) = h;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (m4 + e >= a.M) continue;
                            int mm = m4 + e, nn = n;
                            if (a.up > 1) { const int ph = mm / a.cout; mm -= ph * a.cout; nn = n * a.up + ph; }
                            a.dst0[(size_t)b * a.dst0_bs + ((size_t)(mm >> 3) * a.dst0_ld + nn) * 8 + (mm & 7)] = (_Float16)v[e];
                        }
                    }
                    continue;
                }
                // HG_EPI_RES: res, dst0 and dst1 share the channel count and the row pitch
                const size_t off = ((size_t)(m4 >> 3) * a.res_ld + n) * 8 + (m4 & 7);
                const _Float16* rp = a.res + (size_t)b * a.res_bs + off;
                _Float16* d0 = a.dst0 ? a.dst0 + (size_t)b * a.dst0_bs + off : nullptr;
                _Float16* d1 = a.dst1 ? a.dst1 + (size_t)b * a.dst1_bs + off : nullptr;
                if (whole) {
                    const f16x4 r4 = *reinterpret_cast<const f16x4*>(rp);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += (float)r4[e];
                    if (d0) {
                        f16x4 h;
#pragma unroll
                        for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[e];
                        *reinterpret_cast<f16x4*>(d0) = h;
                    }
                    if (d1) {
                        f16x4 s4;
                        if (!(a.sum_flags & HG_SUM_FIRST)) s4 = *reinterpret_cast<const f16x4*>(d1);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float s = (a.sum_flags & HG_SUM_FIRST) ? v[e] : (float)s4[e] + v[e];
                            if (a.sum_flags & HG_SUM_LAST) s = s / a.nk;
                            s4[e] = (_Float16)s;
                        }
                        *reinterpret_cast<f16x4*>(d1) = s4;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (m4 + e >= a.M) continue;
                        const float ve = v[e] + (float)rp[e];
                        if (d0) d0[e] = (_Float16)ve;
                        if (d1) {
                            float s = (a.sum_flags & HG_SUM_FIRST) ? ve : (float)d1[e] + ve;
                            if (a.sum_flags & HG_SUM_LAST) s = s / a.nk;
                            d1[e] = (_Float16)s;
                        }
                    }
                }
            }
        }
    }
}

// A [MB][nch][ntap][KC / 8][BM][8]: each folded fp32 weight rounded once, padding exact zeros; bias stays fp32
__global__ void hg_pack_f16_kernel(const HgPackArgsH p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    hg_pack_bias(p, i);
    if (i >= (long long)p.MB * p.nch * p.ntap * p.KC * p.BM) return;
    const auto [e, r, kg, j, ch, mb] = hg_pack_k8(p, i);
    p.A[i] = (_Float16)hg_weight_at(p, mb * p.BM + r, ch * p.KC + kg * 8 + e, j);
}

// the format as hg_launch and the entry bodies of hifigan_plan.h take it
struct HgF16 {
    using T = _Float16;
    static constexpr int kc_lo = 16;
    static constexpr const char* name = "hifigan_f16";
    static constexpr const char* kernel = "hg_conv_f16_kernel";
    static constexpr const char* pack_kernel = "hg_pack_f16_kernel";
    template <int MT, int WM, int KC>
    static void launch(const HgConvArgsH& a, unsigned blocks, int lds, hipStream_t s) {
        hipLaunchKernelGGL((hg_conv_f16_kernel<MT, WM, KC>), dim3(blocks), dim3(256), lds, s, a);
    }
    static void pack(const HgPackArgsH& a, unsigned blocks, hipStream_t s) {
        hipLaunchKernelGGL(hg_pack_f16_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
};

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_hifigan_packed_f16_bytes(const ctts_hifigan_config* cfg) { return hg_packed_bytes<HgF16>(cfg); }

int ctts_hifigan_pack_f16(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed, void* stream) {
    return hg_pack<HgF16>("hifigan_pack_f16", true, cfg, weights, weight_floats, packed, stream);
}

size_t ctts_hifigan_workspace_f16_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    return hg_workspace_bytes<HgF16>(cfg, batch, frames);
}

int ctts_hifigan_forward_f16(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                             int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return hg_forward_entry<HgF16>("hifigan_forward_f16", cfg, packed, mel, mel_ld, audio, batch, frames, workspace, workspace_bytes, stream);
}

}  // extern "C"
