// HiFi-GAN generator, split-bf16 products on fp32 tensors (ctts_hifigan_*_bf16x3 in include/cookietts_hip.h): the tensors,
// the workspace, the epilogue and the launch sequence of hifigan.hip, with every product carried as hi + lo bf16 operands on
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
//   epilogue     hg_epilogue_f32, the one hg_conv_kernel calls: bias, residual, the resblock running sum and 1 / n_k, tanh,
//                interleaved phase store
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
// Block shapes and the narrow-below-HG_NARROW_BELOW rule are hifigan_plan.h's (hg_launch); the launch bound is hifigan.hip's.
#include "gemm_bf16.h"       // pack_bf16x2
#include "hifigan_plan.h"

namespace ctts {
namespace {

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
    const HgTile tc = hg_tile<WM>(a);
    const auto& [mb, tile, b, wm, wn, l31, lhi] = tc;
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
    hg_zero(acc);

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

    hg_epilogue_f32<MT, WM>(a, acc, tc, n0);
}

// A [MB][nch][ntap][KC / 8][hi, lo][BM][8] bf16: each folded fp32 weight split once, padding exact zeros in both planes; bias
// stays fp32.  One thread per weight writes its hi and its lo.
__global__ void hg_pack_bf16x3_kernel(const HgPackArgs p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    hg_pack_bias(p, i);
    if (i >= (long long)p.MB * p.nch * p.ntap * p.KC * p.BM) return;
    const auto [e, r, kg, j, ch, mb] = hg_pack_k8(p, i);
    const float w = hg_weight_at(p, mb * p.BM + r, ch * p.KC + kg * 8 + e, j);
    const unsigned int hi = pack_bf16x2(w, 0.0f) & 0xffffu;
    const unsigned int lo = pack_bf16x2(w - __builtin_bit_cast(float, hi << 16), 0.0f) & 0xffffu;
    unsigned short* A = reinterpret_cast<unsigned short*>(p.A);
    const size_t plane = (size_t)p.BM * 8;
    const size_t at = ((((size_t)(mb * p.nch + ch) * p.ntap + j) * (p.KC / 8) + kg) * 2) * plane + (size_t)r * 8 + e;
    A[at] = (unsigned short)hi;
    A[at + plane] = (unsigned short)lo;
}

// the format as hg_launch and the entry bodies of hifigan_plan.h take it: the fp32 element and KC pair
struct HgBf16x3 {
    using T = float;
    static constexpr int kc_lo = 8;
    static constexpr const char* name = "hifigan_bf16x3";
    static constexpr const char* kernel = "hg_conv_bf16x3_kernel";
    static constexpr const char* pack_kernel = "hg_pack_bf16x3_kernel";
    template <int MT, int WM, int KC>
    static void launch(const HgConvArgs& a, unsigned blocks, int lds, hipStream_t s) {
        hipLaunchKernelGGL((hg_conv_bf16x3_kernel<MT, WM, KC>), dim3(blocks), dim3(256), lds, s, a);
    }
    static void pack(const HgPackArgs& a, unsigned blocks, hipStream_t s) {
        hipLaunchKernelGGL(hg_pack_bf16x3_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
};

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_hifigan_packed_bf16x3_bytes(const ctts_hifigan_config* cfg) { return hg_packed_bytes<HgBf16x3>(cfg); }

int ctts_hifigan_pack_bf16x3(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed, void* stream) {
    return hg_pack<HgBf16x3>("hifigan_pack_bf16x3", true, cfg, weights, weight_floats, packed, stream);
}

size_t ctts_hifigan_workspace_bf16x3_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    return hg_workspace_bytes<HgBf16x3>(cfg, batch, frames);
}

int ctts_hifigan_forward_bf16x3(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                                int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return hg_forward_entry<HgBf16x3>("hifigan_forward_bf16x3", cfg, packed, mel, mel_ld, audio, batch, frames, workspace, workspace_bytes,
                                      stream);
}

}  // extern "C"
