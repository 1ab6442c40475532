// HiFi-GAN generator (reference: _4_mtw/hifigan/models.py:35-148 Generator / ResBlock1 / ResBlock2, utils.py get_padding).
// See include/cookietts_hip.h (ctts_hifigan_*).
//
// Every layer of the generator - conv_pre, the transposed upsampling convs, the dilated resblock convs, conv_post - is ONE
// kernel, hg_conv_kernel: an fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32) GEMM
//
//   out[b][m][n] = epi( bias[m] + sum_ci sum_j A[m][ci][j] * lrelu(x[b][ci][n + j * dil - left], slope) )
//
// Layout: activations are dense rows [B][C][ld], ld = roundup(L, 4), NO halo in memory.  A workgroup stages, per chunk of KC
// input channels, one tile of the input rows that is (ntap - 1) * dil columns wider than its output tile; columns outside
// [0, L) are written to LDS as exact zeros (the reference pads every conv with zeros at its own rate), LeakyReLU is applied
// while staging, and all ntap taps read their shifted fragments from that single tile.  The packed weights of the chunk
// ([ntap][KC][BM], k-major like gemm_f32.hip so a fragment is one conflict-free ds_read_b32) are staged beside it.
//
// Transposed conv (stride u, kernel ku, padding p = (ku - u) / 2): out[co][u q + r] = b + sum_ci sum_i x[ci][i] W[ci][co][kk],
// kk = u (q - i) + r + p.  With left = (ku - 1 - p) / u and tap j reading column q + j - left this is kk = u (left - j) + r + p;
// taps whose kk falls outside [0, ku) for a phase carry zero weights (3 taps for the 2 live ones of ku = 2u).
//
// KC = 16 where the two LDS images stay under HG_LDS_KC16 bytes, else 8.  The epilogues, the block shapes with their
// narrow-launch rule, the launcher and the bodies of the entries are hifigan_plan.h's, shared with hifigan_f16.hip and
// hifigan_bf16x3.hip.
#include "hifigan_plan.h"

namespace ctts {
namespace {

using HgConvArgs = HgConvArgsT<float>;

template <int MT, int WM, int KC>
__global__ __launch_bounds__(256, 2) void hg_conv_kernel(const HgConvArgs a) {
    constexpr int WN = 4 / WM;
    constexpr int BM = 32 * MT * WM;
    constexpr int BN = 64 * WN;
    extern __shared__ __attribute__((aligned(16))) float hg_lds[];

    const int t = threadIdx.x;
    const HgTile tc = hg_tile<WM>(a);
    const auto& [mb, tile, b, wm, wn, l31, lhi] = tc;
    const int n0 = tile * BN;

    const int aleft = (a.left + 3) & ~3;                       // tile starts on a 16-byte boundary of the row
    const int c0 = n0 - aleft;
    const int XW = (BN + (a.ntap - 1) * a.dil - a.left + aleft + 3) & ~3;
    const int XW4 = XW >> 2;
    const int a_floats = a.ntap * KC * BM;
    float* As = hg_lds;
    float* Xs = hg_lds + a_floats;

    const float* xb = a.x + (size_t)b * a.x_bs;
    const float* Ab = a.A + (size_t)mb * a.nch * a_floats;
    const float slope = a.slope;

    f32x16 acc[MT][2];
    hg_zero(acc);

    const int a_off = wm * (32 * MT) + l31;
    const int x_off = wn * 64 + l31 + (aleft - a.left);

    for (int ch = 0; ch < a.nch; ++ch) {
        __syncthreads();                                       // the previous chunk's fragments are read
        // weights of the chunk: one contiguous slab
        {
            const float4* src = reinterpret_cast<const float4*>(Ab + (size_t)ch * a_floats);
            float4* dst = reinterpret_cast<float4*>(As);
            for (int u = t; u < (a_floats >> 2); u += 256) dst[u] = src[u];
        }
        // input tile: KC rows x XW columns, zeros outside [0, L) and beyond Cin, LeakyReLU applied here
        for (int u = t; u < KC * XW4; u += 256) {
            const int row = u / XW4;
            const int col = (u - row * XW4) << 2;
            const int ci = ch * KC + row;
            const int c = c0 + col;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ci < a.Cin && c + 3 >= 0 && c < a.L) {
                const float* xr = xb + (size_t)ci * a.x_ld;
                if (a.x_vec && c >= 0 && c + 3 < a.L) {
                    v = *reinterpret_cast<const float4*>(xr + c);
                } else {
                    if (c >= 0) v.x = xr[c];
                    if (c + 1 >= 0 && c + 1 < a.L) v.y = xr[c + 1];
                    if (c + 2 >= 0 && c + 2 < a.L) v.z = xr[c + 2];
                    if (c + 3 < a.L) v.w = xr[c + 3];
                }
                v.x = v.x >= 0.f ? v.x : slope * v.x;
                v.y = v.y >= 0.f ? v.y : slope * v.y;
                v.z = v.z >= 0.f ? v.z : slope * v.z;
                v.w = v.w >= 0.f ? v.w : slope * v.w;
            }
            *reinterpret_cast<float4*>(Xs + row * XW + col) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < a.ntap; ++j) {
            const float* Aj = As + j * (KC * BM) + a_off;
            const float* Xj = Xs + x_off + j * a.dil;
#pragma unroll
            for (int ks = 0; ks < KC / 2; ++ks) {
                const int krow = 2 * ks + lhi;
                float av[MT], bv[2];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[mt] = Aj[krow * BM + mt * 32];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) bv[nt] = Xj[krow * XW + nt * 32];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
            }
        }
    }

    hg_epilogue_f32<MT, WM>(a, acc, tc, n0);
}

using HgPackArgs = HgPackArgsT<float>;

__global__ void hg_pack_kernel(const HgPackArgs p) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    hg_pack_bias(p, i);
    if (i >= (long long)p.MB * p.nch * p.ntap * p.KC * p.BM) return;
    long long q = i;
    const int r = (int)(q % p.BM); q /= p.BM;
    const int kc = (int)(q % p.KC); q /= p.KC;
    const int j = (int)(q % p.ntap); q /= p.ntap;
    const int ch = (int)(q % p.nch); q /= p.nch;
    const int mb = (int)q;
    const int m = mb * p.BM + r, ci = ch * p.KC + kc;
    p.A[i] = hg_weight_at(p, m, ci, j);
}

// the format as hg_launch and the entry bodies of hifigan_plan.h take it
struct HgF32 {
    using T = float;
    static constexpr int kc_lo = 8;
    static constexpr const char* name = "hifigan";
    static constexpr const char* kernel = "hg_conv_kernel";
    static constexpr const char* pack_kernel = "hg_pack_kernel";
    template <int MT, int WM, int KC>
    static void launch(const HgConvArgs& a, unsigned blocks, int lds, hipStream_t s) {
        hipLaunchKernelGGL((hg_conv_kernel<MT, WM, KC>), dim3(blocks), dim3(256), lds, s, a);
    }
    static void pack(const HgPackArgs& a, unsigned blocks, hipStream_t s) {
        hipLaunchKernelGGL(hg_pack_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
};

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_hifigan_weight_floats(const ctts_hifigan_config* cfg) {
    HgPlan p;
    if (make_hg_plan(cfg, p, 4) != CTTS_OK) return 0;
    return p.weight_floats;
}

size_t ctts_hifigan_packed_bytes(const ctts_hifigan_config* cfg) { return hg_packed_bytes<HgF32>(cfg); }

// the one pack entry that takes a blob of any alignment
int ctts_hifigan_pack_f32(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed, void* stream) {
    return hg_pack<HgF32>("hifigan_pack", false, cfg, weights, weight_floats, packed, stream);
}

size_t ctts_hifigan_workspace_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    return hg_workspace_bytes<HgF32>(cfg, batch, frames);
}

int ctts_hifigan_forward_f32(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                             int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return hg_forward_entry<HgF32>("hifigan_forward", cfg, packed, mel, mel_ld, audio, batch, frames, workspace, workspace_bytes, stream);
}

}  // extern "C"
