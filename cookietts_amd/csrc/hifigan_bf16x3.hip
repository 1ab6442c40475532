// HiFi-GAN generator, split-bf16 products on fp32 tensors (ctts_hifigan_*_bf16x3 in include/cookietts_hip.h): the tensors,
// the workspace, the epilogues and the launch sequence of hifigan.hip, with every product carried as hi + lo bf16 operands on
// v_mfma_f32_32x32x16_bf16 instead of v_mfma_f32_32x32x2_f32.  The plan is hifigan_plan.h's esz = 4 plan, unchanged.
//
// Arithmetic (bf16_rne = round to nearest even, one v_cvt_pk_bf16_f32):
//   weights      from the folded fp32 value at pack time: w_hi = bf16_rne(w), w_lo = bf16_rne(w - float(w_hi)); biases stay
//                fp32; padding rows, padding channels and the dead taps of a transposed conv's phases are exact zeros in both
//                planes
//   activations  stored fp32 exactly as the fp32 path stores them.  While a tile is staged: v = x >= 0 ? x : slope * x in fp32
//                (hg_conv_kernel's expression), x_hi = bf16_rne(v), x_lo = bf16_rne(v - float(x_hi)); columns outside [0, L)
//                and channels >= Cin are exact zeros in both planes
//   product      acc += w_hi * x_hi, then acc += w_lo * x_hi, then acc += w_hi * x_lo, fp32 accumulation, in that order for
//                every K16 step; there is no lo * lo term
//   epilogue     hg_conv_kernel's: bias, residual, the resblock running sum and 1 / n_k, tanh, interleaved phase store
// A non-finite activation gives NaN, not infinity: v - float(x_hi) is inf - inf in the lo plane.
//
// Layout.  A hi | lo pair is 4 bytes, so the LDS images and the packed blob have the fp32 path's sizes.  Both are K8-blocked
// like hifigan_f16.hip: the 8 channels 8g..8g+7 of one column (one row of A) are one 16-byte unit per plane, a fragment is one
// ds_read_b128 with consecutive lanes on consecutive units, and a tap is a column offset.  Staged tile: [KC / 8][hi, lo][XW]
// units, XW = BN + (ntap - 1) * dil; a unit is split ONCE while it is staged and then read by every tap and every M-wave.
// Packed weights: [MB][nch][ntap][KC / 8][hi, lo][BM] units, a chunk's slab staged beside the tile.
//
// K16 steps.  KC = 16: one step per tap, the two lane halves take channel groups 0 and 1.  KC = 8 (the wide layers, where
// the fp32 plan halves the chunk to fit the LDS): one step per PAIR of taps, lane half h takes tap 2p + h of the 8 channels.
// With an odd tap count the last step's second half is a phantom tap: its A fragment is zeros in registers and its X fragment
// is the last real tap's (staged, finite for finite input) - never unwritten LDS.
// The K order of a column's sum is chunks in order, steps in order inside a chunk, the three products in the order above, the
// MFMA's own order inside a step: a function of the layer and its KC only, never of the block shape, tile count or batch, so an
// item of a batch equals the same item run alone, bit for bit.
//
// Block shapes, the narrow-below-HG_NARROW_BELOW rule and the launch bound are hifigan.hip's.
#include "gemm_bf16.h"       // pack_bf16x2
#include "hifigan_plan.h"

namespace ctts {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

using HgConvArgs = HgConvArgsT<float>;
using HgPackArgs = HgPackArgsT<float>;

// 8 fp32 -> the hi and the lo unit (gemm_f32.hip's split8)
__device__ __forceinline__ void hg_split8(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned int h = pack_bf16x2(v[2 * j], v[2 * j + 1]);
        hi[j] = h;
        lo[j] = pack_bf16x2(v[2 * j] - __builtin_bit_cast(float, h << 16), v[2 * j + 1] - __builtin_bit_cast(float, h & 0xffff0000u));
    }
}

__device__ __forceinline__ f32x16 hg_mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int MT, int WM, int KC>
__global__ __launch_bounds__(256, 2) void hg_conv_bf16x3_kernel(const HgConvArgs a) {
    constexpr int WN = 4 / WM;
    constexpr int BM = 32 * MT * WM;
    constexpr int BN = 64 * WN;
    constexpr int KG = KC / 8;                                 // groups of 8 channels per chunk
    extern __shared__ __attribute__((aligned(16))) u32x4 hg_lds_s[];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lhi = lane >> 5;

    int id = blockIdx.x;
    const int mb = id % a.MB;
    id /= a.MB;
    const int tile = id % a.ntiles;
    const int b = id / a.ntiles;
    const int n0 = tile * BN;

    const int c0 = n0 - a.left;
    const int XW = BN + (a.ntap - 1) * a.dil;
    const int a_units = a.ntap * KG * 2 * BM;
    u32x4* As = hg_lds_s;
    u32x4* Xs = hg_lds_s + a_units;

    const float* xb = a.x + (size_t)b * a.x_bs;
    const u32x4* Ab = reinterpret_cast<const u32x4*>(a.A) + (size_t)mb * a.nch * a_units;
    const float slope = a.slope;

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int a_off = wm * (32 * MT) + l31;
    const int x_off = wn * 64 + l31;
    const int nsteps = KC == 16 ? a.ntap : (a.ntap + 1) >> 1;

    for (int ch = 0; ch < a.nch; ++ch) {
        __syncthreads();                                       // the previous chunk's fragments are read
        {   // weights of the chunk: one contiguous slab, both planes
            const u32x4* src = Ab + (size_t)ch * a_units;
            for (int u = t; u < a_units; u += 256) As[u] = src[u];
        }
        // input tile: KG rows x XW columns of 8 channels, zeros outside [0, L) and beyond Cin; LeakyReLU, then the split
        for (int u = t; u < KG * XW; u += 256) {
            const int g = u / XW;
            const int col = u - g * XW;
            const int ci = (ch * KG + g) * 8;
            const int c = c0 + col;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.0f;
            if (ci < a.Cin && c >= 0 && c < a.L) {
                const float* xr = xb + (size_t)ci * a.x_ld + c;      // eight rows of one column: each load coalesced across lanes
                const int live = min(8, a.Cin - ci);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < live) {
                        const float x = xr[(size_t)e * a.x_ld];
                        v[e] = x >= 0.f ? x : slope * x;
                    }
            }
            u32x4 hi, lo;
            hg_split8(v, hi, lo);
            Xs[(2 * g) * XW + col] = hi;
            Xs[(2 * g + 1) * XW + col] = lo;
        }
        __syncthreads();
#pragma unroll 1
        for (int st = 0; st < nsteps; ++st) {
            // this lane half's 8 K slots: KC = 16: channel group lhi of tap st; KC = 8: the one group of tap 2 st + lhi
            int j, kg;
            bool live = true;
            if constexpr (KC == 16) { j = st; kg = lhi; }
            else { j = 2 * st + lhi; kg = 0; live = j < a.ntap; j = live ? j : a.ntap - 1; }
            const u32x4* Aj = As + (j * KG + kg) * 2 * BM + a_off;
            const u32x4* Xj = Xs + kg * 2 * XW + x_off + j * a.dil;
            u32x4 ah[MT], al[MT], bh[2], bl[2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                ah[mt] = Aj[mt * 32];
                al[mt] = Aj[BM + mt * 32];
                if constexpr (KC == 8)
                    if (!live) { ah[mt] = u32x4{0u, 0u, 0u, 0u}; al[mt] = u32x4{0u, 0u, 0u, 0u}; }
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                bh[nt] = Xj[nt * 32];
                bl[nt] = Xj[XW + nt * 32];
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = hg_mfma_bf16(ah[mt], bh[nt], acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = hg_mfma_bf16(al[mt], bh[nt], acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = hg_mfma_bf16(ah[mt], bl[nt], acc[mt][nt]);
        }
    }

    // ---- epilogue: hg_conv_kernel's.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const float* bias = a.bias + mb * BM;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = n0 + wn * 64 + nt * 32 + l31;
            if (n >= a.L) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * (32 * MT) + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                const int m = mb * BM + row;
                if (m >= a.M) continue;
                float v = acc[mt][nt][r] + bias[row];
                if (a.epi == HG_EPI_STORE) {
                    if (a.up > 1) {
                        const int ph = m / a.cout, co = m - ph * a.cout;
                        a.dst0[(size_t)b * a.dst0_bs + (size_t)co * a.dst0_ld + (size_t)n * a.up + ph] = v;
                    } else {
                        a.dst0[(size_t)b * a.dst0_bs + (size_t)m * a.dst0_ld + n] = v;
                    }
                } else if (a.epi == HG_EPI_RES) {
                    v += a.res[(size_t)b * a.res_bs + (size_t)m * a.res_ld + n];
                    if (a.dst0) a.dst0[(size_t)b * a.dst0_bs + (size_t)m * a.dst0_ld + n] = v;
                    if (a.dst1) {
                        float* d = a.dst1 + (size_t)b * a.dst1_bs + (size_t)m * a.dst1_ld + n;
                        float s = (a.sum_flags & HG_SUM_FIRST) ? v : *d + v;
                        if (a.sum_flags & HG_SUM_LAST) s = s / a.nk;
                        *d = s;
                    }
                } else {
                    a.dst0[(size_t)b * a.dst0_bs + (size_t)m * a.dst0_ld + n] = tanhf(v);
                }
            }
        }
    }
}

// A [MB][nch][ntap][KC / 8][hi, lo][BM][8] bf16: each folded fp32 weight split once, padding exact zeros in both planes; bias
// stays fp32.  One thread per weight writes its hi and its lo.
__global__ void hg_pack_bf16x3_kernel(const HgPackArgs p) {
    const long long total = (long long)p.MB * p.nch * p.ntap * p.KC * p.BM;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long long)p.MB * p.BM) {
        const int m = (int)i;
        p.bias[m] = m < p.M ? p.b[p.kind == HG_CONVT ? m % p.cout : m] : 0.0f;
    }
    if (i >= total) return;
    long long q = i;
    const int e = (int)(q & 7); q >>= 3;
    const int r = (int)(q % p.BM); q /= p.BM;
    const int kg = (int)(q % (p.KC / 8)); q /= (p.KC / 8);
    const int j = (int)(q % p.ntap); q /= p.ntap;
    const int ch = (int)(q % p.nch); q /= p.nch;
    const int mb = (int)q;
    const float w = hg_weight_at(p, mb * p.BM + r, ch * p.KC + kg * 8 + e, j);
    const unsigned int hi = pack_bf16x2(w, 0.0f) & 0xffffu;
    const unsigned int lo = pack_bf16x2(w - __builtin_bit_cast(float, hi << 16), 0.0f) & 0xffffu;
    unsigned short* A = reinterpret_cast<unsigned short*>(p.A);
    const size_t plane = (size_t)p.BM * 8;
    const size_t at = ((((size_t)(mb * p.nch + ch) * p.ntap + j) * (p.KC / 8) + kg) * 2) * plane + (size_t)r * 8 + e;
    A[at] = (unsigned short)hi;
    A[at + plane] = (unsigned short)lo;
}

template <int MT, int WM, int KC>
void hg_launch_shape_s(const HgConvArgs& a, int batch, int lds, hipStream_t s) {
    hipLaunchKernelGGL((hg_conv_bf16x3_kernel<MT, WM, KC>), dim3((unsigned)((size_t)a.MB * a.ntiles * batch)), dim3(256), lds, s, a);
}

int hg_launch_s(const HgLayer& l, HgConvArgs a, const void* packed, int batch, hipStream_t s) {
    a.A = reinterpret_cast<const float*>(static_cast<const char*>(packed) + l.A_off);
    a.bias = reinterpret_cast<const float*>(static_cast<const char*>(packed) + l.bias_off);
    a.Cin = l.Cin; a.ntap = l.ntap; a.dil = l.dil; a.left = l.left;
    a.M = l.M; a.MB = l.MB; a.nch = l.nch;
    // the half-width block of the same M-block height for launches too small to fill the chip (as the fp32 path does)
    int WM = l.WM, MT = l.MT, BN = l.BN;
    if (l.BM >= 64 && (long long)l.MB * ((a.L + BN - 1) / BN) * batch < HG_NARROW_BELOW) { WM *= 2; MT = 1; BN /= 2; }
    a.ntiles = (a.L + BN - 1) / BN;
    a.up = l.up; a.cout = l.cout;
    // the fp32 plan's LDS figure covers this layout: the same weight bytes, and a tile that is no wider (no 16-byte row alignment)
    const int lds = l.lds_bytes(BN);
    const int key = MT * 100 + WM * 10 + (l.KC == 16);
    switch (key) {
        case 110: hg_launch_shape_s<1, 1, 8>(a, batch, lds, s); break;
        case 111: hg_launch_shape_s<1, 1, 16>(a, batch, lds, s); break;
        case 120: hg_launch_shape_s<1, 2, 8>(a, batch, lds, s); break;
        case 121: hg_launch_shape_s<1, 2, 16>(a, batch, lds, s); break;
        case 140: hg_launch_shape_s<1, 4, 8>(a, batch, lds, s); break;
        case 141: hg_launch_shape_s<1, 4, 16>(a, batch, lds, s); break;
        case 210: hg_launch_shape_s<2, 1, 8>(a, batch, lds, s); break;
        case 211: hg_launch_shape_s<2, 1, 16>(a, batch, lds, s); break;
        case 220: hg_launch_shape_s<2, 2, 8>(a, batch, lds, s); break;
        case 221: hg_launch_shape_s<2, 2, 16>(a, batch, lds, s); break;
        default: set_error("hifigan_bf16x3: no kernel shape %d", key); return CTTS_E_ARG;
    }
    CTTS_CHECK_LAUNCH("hg_conv_bf16x3_kernel");
    return CTTS_OK;
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_hifigan_packed_bf16x3_bytes(const ctts_hifigan_config* cfg) {
    HgPlan p;
    if (make_hg_plan(cfg, p, 4) != CTTS_OK) return 0;
    return p.packed_bytes;
}

int ctts_hifigan_pack_bf16x3(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed, void* stream) {
    HgPlan p;
    int rc = make_hg_plan(cfg, p, 4);
    if (rc) return rc;
    CTTS_CHECK_ARG(weights != nullptr && packed != nullptr, "hifigan_pack_bf16x3: NULL pointer");
    CTTS_CHECK_ARG(weight_floats == p.weight_floats, "hifigan_pack_bf16x3: %zu weight floats given, the config has %zu", weight_floats,
                   p.weight_floats);
    CTTS_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "hifigan_pack_bf16x3: packed blob must be 16-byte aligned");
    for (const HgLayer& l : p.layers) {
        const HgPackArgs a = hg_pack_args<float>(l, weights, packed);
        const long long total = (long long)l.packed_elems();     // >= MB * BM
        hipLaunchKernelGGL(hg_pack_bf16x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), a);
        CTTS_CHECK_LAUNCH("hg_pack_bf16x3_kernel");
    }
    return CTTS_OK;
}

size_t ctts_hifigan_workspace_bf16x3_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    HgPlan p;
    HgGeom g;
    if (make_hg_plan(cfg, p, 4) != CTTS_OK || hg_geometry(p, batch, frames, g) != CTTS_OK) return 0;
    return g.total_elems * sizeof(float);
}

int ctts_hifigan_forward_bf16x3(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                                int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    HgPlan p;
    HgGeom g;
    int rc = make_hg_plan(cfg, p, 4);
    if (rc) return rc;
    if ((rc = hg_geometry(p, batch, frames, g))) return rc;
    CTTS_CHECK_ARG(packed != nullptr && mel != nullptr && audio != nullptr && workspace != nullptr, "hifigan_forward_bf16x3: NULL pointer");
    CTTS_CHECK_ARG(mel_ld >= frames, "hifigan_forward_bf16x3: mel_ld=%d < frames=%d", mel_ld, frames);
    CTTS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0,
                   "hifigan_forward_bf16x3: packed blob and workspace must be 16-byte aligned");
    if (workspace_bytes < g.total_elems * sizeof(float)) {
        set_error("hifigan_forward_bf16x3: workspace %zu bytes < required %zu", workspace_bytes, g.total_elems * sizeof(float));
        return CTTS_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    return hg_forward<float>(p, g, mel, mel_ld, audio, frames, static_cast<float*>(workspace),
                             [&](const HgLayer& l, const HgConvArgs& a) { return hg_launch_s(l, a, packed, batch, s); });
}

}  // extern "C"
