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
// Epilogues (no stand-alone elementwise launch anywhere in the model):
//   HG_EPI_STORE  dst0 = v; with up > 1 the rows are (phase r, channel co) of a transposed conv and the store is
//                 dst0[co][n * up + r]: the `up` stride-1 phase convolutions of ConvTranspose1d written interleaved
//   HG_EPI_RES    v += res; dst0 = v (when given); dst1 = ((first ? 0 : dst1) + v) [/ nk when last]: the residual add, the sum
//                 over the n_k resblocks of a stage and its 1 / n_k
//   HG_EPI_TANH   dst0 = tanh(v) for rows < M (conv_post; its input slope is F.leaky_relu's default 0.01, models.py:134)
//
// Transposed conv (stride u, kernel ku, padding p = (ku - u) / 2): out[co][u q + r] = b + sum_ci sum_i x[ci][i] W[ci][co][kk],
// kk = u (q - i) + r + p.  With left = (ku - 1 - p) / u and tap j reading column q + j - left this is kk = u (left - j) + r + p;
// taps whose kk falls outside [0, ku) for a phase carry zero weights (3 taps for the 2 live ones of ku = 2u).
//
// Block shapes (256 threads = 4 waves, wave tile 32 MT x 64): BM = 32 MT WM rows, BN = 64 (4 / WM) columns:
//   M <= 32: 32 x 256    M <= 64: 64 x 256    else: 128 x 128 (M-blocks of 128 rows)
// and, for launches too small to fill the chip with those (batch 1), 64 x 128 / 128 x 64 on the same packed weights.
// KC = 16 where the two LDS images stay under HG_LDS_KC16 bytes, else 8.
#include "hifigan_plan.h"    // the layer list, the launch arguments and the launch sequence, shared with hifigan_f16.hip

namespace ctts {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

using HgConvArgs = HgConvArgsT<float>;

template <int MT, int WM, int KC>
__global__ __launch_bounds__(256, 2) void hg_conv_kernel(const HgConvArgs a) {
    constexpr int WN = 4 / WM;
    constexpr int BM = 32 * MT * WM;
    constexpr int BN = 64 * WN;
    extern __shared__ __attribute__((aligned(16))) float hg_lds[];

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
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

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

    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
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

using HgPackArgs = HgPackArgsT<float>;

__global__ void hg_pack_kernel(const HgPackArgs p) {
    const long long total = (long long)p.MB * p.nch * p.ntap * p.KC * p.BM;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long long)p.MB * p.BM) {
        const int m = (int)i;
        p.bias[m] = m < p.M ? p.b[p.kind == HG_CONVT ? m % p.cout : m] : 0.0f;
    }
    if (i >= total) return;
    long long q = i;
    const int r = (int)(q % p.BM); q /= p.BM;
    const int kc = (int)(q % p.KC); q /= p.KC;
    const int j = (int)(q % p.ntap); q /= p.ntap;
    const int ch = (int)(q % p.nch); q /= p.nch;
    const int mb = (int)q;
    const int m = mb * p.BM + r, ci = ch * p.KC + kc;
    p.A[i] = hg_weight_at(p, m, ci, j);
}

template <int MT, int WM, int KC>
void hg_launch_shape(const HgConvArgs& a, int batch, int lds, hipStream_t s) {
    hipLaunchKernelGGL((hg_conv_kernel<MT, WM, KC>), dim3((unsigned)((size_t)a.MB * a.ntiles * batch)), dim3(256), lds, s, a);
}

int hg_launch(const HgLayer& l, HgConvArgs a, const float* packed, int batch, hipStream_t s) {
    a.A = reinterpret_cast<const float*>(reinterpret_cast<const char*>(packed) + l.A_off);
    a.bias = reinterpret_cast<const float*>(reinterpret_cast<const char*>(packed) + l.bias_off);
    a.Cin = l.Cin; a.ntap = l.ntap; a.dil = l.dil; a.left = l.left;
    a.M = l.M; a.MB = l.MB; a.nch = l.nch;
    // a launch that would start fewer than HG_NARROW_BELOW workgroups takes the half-width block of the same M-block height
    // (waves stacked along M): same packed weights, same K order, bit-identical results, twice the workgroups to spread
    int WM = l.WM, MT = l.MT, BN = l.BN;
    if (l.BM >= 64 && (long long)l.MB * ((a.L + BN - 1) / BN) * batch < HG_NARROW_BELOW) { WM *= 2; MT = 1; BN /= 2; }
    a.ntiles = (a.L + BN - 1) / BN;
    a.up = l.up; a.cout = l.cout;
    a.x_vec = (a.x_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 && a.x_bs % 4 == 0) ? 1 : 0;
    const int lds = l.lds_bytes(BN);
    const int key = MT * 100 + WM * 10 + (l.KC == 16);
    switch (key) {
        case 110: hg_launch_shape<1, 1, 8>(a, batch, lds, s); break;
        case 111: hg_launch_shape<1, 1, 16>(a, batch, lds, s); break;
        case 120: hg_launch_shape<1, 2, 8>(a, batch, lds, s); break;
        case 121: hg_launch_shape<1, 2, 16>(a, batch, lds, s); break;
        case 140: hg_launch_shape<1, 4, 8>(a, batch, lds, s); break;
        case 141: hg_launch_shape<1, 4, 16>(a, batch, lds, s); break;
        case 210: hg_launch_shape<2, 1, 8>(a, batch, lds, s); break;
        case 211: hg_launch_shape<2, 1, 16>(a, batch, lds, s); break;
        case 220: hg_launch_shape<2, 2, 8>(a, batch, lds, s); break;
        case 221: hg_launch_shape<2, 2, 16>(a, batch, lds, s); break;
        default: set_error("hifigan: no kernel shape %d", key); return CTTS_E_ARG;
    }
    CTTS_CHECK_LAUNCH("hg_conv_kernel");
    return CTTS_OK;
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

size_t ctts_hifigan_weight_floats(const ctts_hifigan_config* cfg) {
    HgPlan p;
    if (make_hg_plan(cfg, p, 4) != CTTS_OK) return 0;
    return p.weight_floats;
}

size_t ctts_hifigan_packed_bytes(const ctts_hifigan_config* cfg) {
    HgPlan p;
    if (make_hg_plan(cfg, p, 4) != CTTS_OK) return 0;
    return p.packed_bytes;
}

int ctts_hifigan_pack_f32(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed, void* stream) {
    HgPlan p;
    int rc = make_hg_plan(cfg, p, 4);
    if (rc) return rc;
    CTTS_CHECK_ARG(weights != nullptr && packed != nullptr, "hifigan_pack: NULL pointer");
    CTTS_CHECK_ARG(weight_floats == p.weight_floats, "hifigan_pack: %zu weight floats given, the config has %zu", weight_floats,
                   p.weight_floats);
    for (const HgLayer& l : p.layers) {
        const HgPackArgs a = hg_pack_args<float>(l, weights, packed);
        const long long total = (long long)l.MB * l.nch * l.ntap * l.KC * l.BM;     // >= MB * BM
        hipLaunchKernelGGL(hg_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), a);
        CTTS_CHECK_LAUNCH("hg_pack_kernel");
    }
    return CTTS_OK;
}

size_t ctts_hifigan_workspace_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    HgPlan p;
    HgGeom g;
    if (make_hg_plan(cfg, p, 4) != CTTS_OK || hg_geometry(p, batch, frames, g) != CTTS_OK) return 0;
    return g.total_elems * sizeof(float);
}

int ctts_hifigan_forward_f32(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                             int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    HgPlan p;
    HgGeom g;
    int rc = make_hg_plan(cfg, p, 4);
    if (rc) return rc;
    if ((rc = hg_geometry(p, batch, frames, g))) return rc;
    CTTS_CHECK_ARG(packed != nullptr && mel != nullptr && audio != nullptr && workspace != nullptr, "hifigan_forward: NULL pointer");
    CTTS_CHECK_ARG(mel_ld >= frames, "hifigan_forward: mel_ld=%d < frames=%d", mel_ld, frames);
    CTTS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0,
                   "hifigan_forward: packed blob and workspace must be 16-byte aligned");
    if (workspace_bytes < g.total_elems * sizeof(float)) {
        set_error("hifigan_forward: workspace %zu bytes < required %zu", workspace_bytes, g.total_elems * sizeof(float));
        return CTTS_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    const float* pk = static_cast<const float*>(packed);
    return hg_forward<float>(p, g, mel, mel_ld, audio, frames, static_cast<float*>(workspace),
                             [&](const HgLayer& l, const HgConvArgs& a) { return hg_launch(l, a, pk, batch, s); });
}

}  // extern "C"
