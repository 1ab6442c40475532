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
#include <algorithm>
#include <vector>

#include "common.h"

namespace ctts {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { HG_EPI_STORE = 0, HG_EPI_RES = 1, HG_EPI_TANH = 2 };
enum { HG_SUM_FIRST = 1, HG_SUM_LAST = 2 };
enum { HG_CONV = 0, HG_CONVT = 1 };

constexpr int HG_MAX_KERNEL = 11;         // resblock kernel size (odd)
constexpr int HG_MAX_HALO = 128;          // (k - 1) * dilation
constexpr int HG_MAX_UP_TAPS = 5;         // taps of a phase convolution incl. the zero-weight ones
constexpr int HG_LDS_MAX = 64 * 1024;     // dynamic LDS a launch may ask for
constexpr int HG_LDS_KC16 = 40 * 1024;    // KC = 16 only while four workgroups still fit a CU's LDS
constexpr int HG_NARROW_BELOW = 1024;     // workgroups (4 per CU) under which the half-width block shape is launched

struct HgConvArgs {
    const float* A;        // packed [MB][nch][ntap][KC][BM]
    const float* bias;     // [MB * BM]
    const float* x;        // [B][Cin][x_ld]
    long long x_bs;
    int x_ld, x_vec;       // x_vec: rows are 16-byte aligned (float4 staging)
    int Cin, L;            // valid input channels; valid columns (input and output share the column domain)
    int ntap, dil, left;   // tap j reads column n + j * dil - left
    float slope;           // LeakyReLU slope applied to x while staging (1 = none)
    int M, MB, ntiles, nch;
    int epi;
    float* dst0; long long dst0_bs; int dst0_ld;
    int up, cout;          // HG_EPI_STORE: up > 1 = interleaved phase store
    const float* res; long long res_bs; int res_ld;
    float* dst1; long long dst1_bs; int dst1_ld;
    int sum_flags; float nk;
};

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

struct HgPackArgs {
    const float* w;        // HG_CONV: [M][Cin][k]; HG_CONVT: [Cin][cout][ku]
    const float* b;        // [M] / [cout]
    float* A;
    float* bias;
    int kind, Cin, M, cout, up, ku, pad, ntap, left, KC, BM, MB, nch;
};

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
    float v = 0.0f;
    if (m < p.M && ci < p.Cin) {
        if (p.kind == HG_CONV) {
            v = p.w[((size_t)m * p.Cin + ci) * p.ntap + j];
        } else {
            const int ph = m / p.cout, co = m - ph * p.cout;
            const int kk = p.up * (p.left - j) + ph + p.pad;
            if (kk >= 0 && kk < p.ku) v = p.w[((size_t)ci * p.cout + co) * p.ku + kk];
        }
    }
    p.A[i] = v;
}

// ---- plan: the layer list of one config, shared by the size queries, the pack and the forward ----
struct HgLayer {
    int kind, Cin, M, cout, up, ku, pad, ntap, dil, left;
    int MT, WM, KC, BM, BN, MB, nch;
    size_t w_off, b_off;         // floats into the caller's flat folded weights
    size_t A_off, bias_off;      // floats into the packed blob
    int lds_bytes(int bn) const {
        const int aleft = (left + 3) & ~3;
        const int XW = (bn + (ntap - 1) * dil - left + aleft + 3) & ~3;
        return (ntap * KC * BM + KC * XW) * 4;
    }
    int lds_bytes() const { return lds_bytes(BN); }
};

struct HgPlan {
    ctts_hifigan_config c;
    std::vector<HgLayer> layers;     // conv_pre, then per stage: ups_i, its n_k resblocks' convs in module order; conv_post last
    std::vector<int> chans;          // channels after stage i
    int n_steps;                     // convs1/convs2 pairs (ResBlock1: 3) or convs (ResBlock2: 2) per resblock
    long long up_total;              // prod(upsample_rates)
    size_t weight_floats, packed_floats;
};

inline size_t hg_align(size_t v) { return (v + 63) / 64 * 64; }

int hg_add_layer(HgPlan& p, int kind, int Cin, int M, int cout, int up, int ku, int pad, int ntap, int dil, int left, const char* what) {
    HgLayer l{};
    l.kind = kind; l.Cin = Cin; l.M = M; l.cout = cout; l.up = up; l.ku = ku; l.pad = pad; l.ntap = ntap; l.dil = dil; l.left = left;
    if (M <= 32) { l.MT = 1; l.WM = 1; }
    else if (M <= 64) { l.MT = 2; l.WM = 1; }
    else { l.MT = 2; l.WM = 2; }
    l.BM = 32 * l.MT * l.WM;
    l.BN = 64 * (4 / l.WM);
    l.MB = (M + l.BM - 1) / l.BM;
    l.KC = 16;
    if (Cin <= 8 || l.lds_bytes() > HG_LDS_KC16) l.KC = 8;
    CTTS_CHECK_ARG(l.lds_bytes() <= HG_LDS_MAX, "hifigan: %s needs %d bytes of LDS (limit %d)", what, l.lds_bytes(), HG_LDS_MAX);
    l.nch = (Cin + l.KC - 1) / l.KC;
    l.w_off = p.weight_floats;
    const size_t wn = kind == HG_CONV ? (size_t)M * Cin * ntap : (size_t)Cin * cout * ku;
    l.b_off = l.w_off + wn;
    p.weight_floats = l.b_off + (kind == HG_CONV ? M : cout);
    l.A_off = p.packed_floats;
    l.bias_off = l.A_off + hg_align((size_t)l.MB * l.nch * l.ntap * l.KC * l.BM);
    p.packed_floats = l.bias_off + hg_align((size_t)l.MB * l.BM);
    p.layers.push_back(l);
    return CTTS_OK;
}

int make_hg_plan(const ctts_hifigan_config* cfg, HgPlan& p) {
    CTTS_CHECK_ARG(cfg != nullptr, "hifigan: config is NULL");
    p.c = *cfg;
    const auto& c = p.c;
    p.weight_floats = p.packed_floats = 0;
    CTTS_CHECK_ARG(c.num_mels >= 1 && c.num_mels <= 4096, "hifigan: num_mels=%d", c.num_mels);
    CTTS_CHECK_ARG(c.resblock == 1 || c.resblock == 2, "hifigan: resblock=%d ('1' or '2')", c.resblock);
    CTTS_CHECK_ARG(c.n_ups >= 1 && c.n_ups <= CTTS_HIFIGAN_MAX_UPS, "hifigan: upsample_rates has %d entries (1..%d)", c.n_ups,
                   CTTS_HIFIGAN_MAX_UPS);
    CTTS_CHECK_ARG(c.n_kernels >= 1 && c.n_kernels <= CTTS_HIFIGAN_MAX_KERNELS, "hifigan: resblock_kernel_sizes has %d entries (1..%d)",
                   c.n_kernels, CTTS_HIFIGAN_MAX_KERNELS);
    CTTS_CHECK_ARG(c.upsample_initial_channel >= (1 << c.n_ups) && c.upsample_initial_channel % (1 << c.n_ups) == 0 &&
                       c.upsample_initial_channel <= 8192,
                   "hifigan: upsample_initial_channel=%d (a multiple of 2^%d, <= 8192)", c.upsample_initial_channel, c.n_ups);
    p.n_steps = c.resblock == 1 ? 3 : 2;
    p.up_total = 1;
    for (int i = 0; i < c.n_ups; ++i) {
        const int u = c.upsample_rates[i], ku = c.upsample_kernel_sizes[i];
        CTTS_CHECK_ARG(u >= 1 && u <= 64, "hifigan: upsample_rates[%d]=%d (1..64)", i, u);
        CTTS_CHECK_ARG(ku >= u && (ku - u) % 2 == 0, "hifigan: upsample_kernel_sizes[%d]=%d with rate %d (kernel - rate even and >= 0: the output is rate * T long)", i, ku, u);
        p.up_total *= u;
        CTTS_CHECK_ARG(p.up_total <= (1 << 20), "hifigan: upsample_rates multiply to more than 2^20");
    }
    for (int j = 0; j < c.n_kernels; ++j) {
        const int k = c.resblock_kernel_sizes[j];
        CTTS_CHECK_ARG(k >= 1 && k % 2 == 1 && k <= HG_MAX_KERNEL, "hifigan: resblock_kernel_sizes[%d]=%d (odd, <= %d)", j, k, HG_MAX_KERNEL);
        for (int m = 0; m < p.n_steps; ++m) {
            const int d = c.resblock_dilation_sizes[j][m];
            CTTS_CHECK_ARG(d >= 1 && (k - 1) * d <= HG_MAX_HALO, "hifigan: resblock_dilation_sizes[%d][%d]=%d with kernel %d (halo (k-1)*d <= %d)",
                           j, m, d, k, HG_MAX_HALO);
        }
    }
    int rc = hg_add_layer(p, HG_CONV, c.num_mels, c.upsample_initial_channel, 0, 1, 0, 0, 7, 1, 3, "conv_pre");
    if (rc) return rc;
    int C = c.upsample_initial_channel;
    for (int i = 0; i < c.n_ups; ++i) {
        const int u = c.upsample_rates[i], ku = c.upsample_kernel_sizes[i], pad = (ku - u) / 2;
        const int left = (ku - 1 - pad) / u, jhi = (u - 1 + pad) / u;
        CTTS_CHECK_ARG(left + jhi + 1 <= HG_MAX_UP_TAPS, "hifigan: upsample_kernel_sizes[%d]=%d with rate %d (at most %d taps per phase)", i, ku,
                       u, HG_MAX_UP_TAPS - 1);
        if ((rc = hg_add_layer(p, HG_CONVT, C, u * (C / 2), C / 2, u, ku, pad, left + jhi + 1, 1, left, "ups"))) return rc;
        C /= 2;
        p.chans.push_back(C);
        for (int j = 0; j < c.n_kernels; ++j) {
            const int k = c.resblock_kernel_sizes[j];
            // module order: convs1.0-2 then convs2.0-2 (ResBlock1), convs.0-1 (ResBlock2)
            for (int m = 0; m < p.n_steps; ++m) {
                const int d = c.resblock_dilation_sizes[j][m];
                if ((rc = hg_add_layer(p, HG_CONV, C, C, 0, 1, 0, 0, k, d, (k - 1) / 2 * d, "resblock conv"))) return rc;
            }
            if (c.resblock == 1)
                for (int m = 0; m < 3; ++m)
                    if ((rc = hg_add_layer(p, HG_CONV, C, C, 0, 1, 0, 0, k, 1, (k - 1) / 2, "resblock conv"))) return rc;
        }
    }
    return hg_add_layer(p, HG_CONV, C, 1, 0, 1, 0, 0, 7, 1, 3, "conv_post");
}

struct HgGeom { size_t buf_floats; size_t total_floats; };

// five activation buffers (stage input x, resblock sum xs, the c1 output, two ping-pong resblock states), each
// batch * max over the tensors of the call of C * roundup(L, 4) floats
int hg_geometry(const HgPlan& p, int batch, int frames, HgGeom& g) {
    CTTS_CHECK_ARG(batch >= 1 && batch <= 4096, "hifigan: batch=%d (1..4096)", batch);
    CTTS_CHECK_ARG(frames >= 1 && (long long)frames * p.up_total <= (1ll << 30), "hifigan: frames=%d (>= 1, frames * prod(rates) <= 2^30)", frames);
    long long L = frames;
    size_t mx = (size_t)p.c.upsample_initial_channel * round_up((int)L, 4);
    for (int i = 0; i < p.c.n_ups; ++i) {
        L *= p.c.upsample_rates[i];
        mx = std::max(mx, (size_t)p.chans[i] * (size_t)round_up((int)L, 4));
    }
    g.buf_floats = hg_align(mx * (size_t)batch);
    g.total_floats = 5 * g.buf_floats;
    return CTTS_OK;
}

template <int MT, int WM, int KC>
void hg_launch_shape(const HgConvArgs& a, int batch, int lds, hipStream_t s) {
    hipLaunchKernelGGL((hg_conv_kernel<MT, WM, KC>), dim3((unsigned)((size_t)a.MB * a.ntiles * batch)), dim3(256), lds, s, a);
}

int hg_launch(const HgLayer& l, HgConvArgs a, const float* packed, int batch, hipStream_t s) {
    a.A = packed + l.A_off;
    a.bias = packed + l.bias_off;
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
    if (make_hg_plan(cfg, p) != CTTS_OK) return 0;
    return p.weight_floats;
}

size_t ctts_hifigan_packed_bytes(const ctts_hifigan_config* cfg) {
    HgPlan p;
    if (make_hg_plan(cfg, p) != CTTS_OK) return 0;
    return p.packed_floats * sizeof(float);
}

int ctts_hifigan_pack_f32(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed, void* stream) {
    HgPlan p;
    int rc = make_hg_plan(cfg, p);
    if (rc) return rc;
    CTTS_CHECK_ARG(weights != nullptr && packed != nullptr, "hifigan_pack: NULL pointer");
    CTTS_CHECK_ARG(weight_floats == p.weight_floats, "hifigan_pack: %zu weight floats given, the config has %zu", weight_floats,
                   p.weight_floats);
    float* out = static_cast<float*>(packed);
    for (const HgLayer& l : p.layers) {
        HgPackArgs a{};
        a.w = weights + l.w_off; a.b = weights + l.b_off;
        a.A = out + l.A_off; a.bias = out + l.bias_off;
        a.kind = l.kind; a.Cin = l.Cin; a.M = l.M; a.cout = l.cout > 0 ? l.cout : 1; a.up = l.up; a.ku = l.ku; a.pad = l.pad;
        a.ntap = l.ntap; a.left = l.left; a.KC = l.KC; a.BM = l.BM; a.MB = l.MB; a.nch = l.nch;
        const long long total = (long long)l.MB * l.nch * l.ntap * l.KC * l.BM;     // >= MB * BM
        hipLaunchKernelGGL(hg_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), a);
        CTTS_CHECK_LAUNCH("hg_pack_kernel");
    }
    return CTTS_OK;
}

size_t ctts_hifigan_workspace_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    HgPlan p;
    HgGeom g;
    if (make_hg_plan(cfg, p) != CTTS_OK || hg_geometry(p, batch, frames, g) != CTTS_OK) return 0;
    return g.total_floats * sizeof(float);
}

int ctts_hifigan_forward_f32(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                             int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    HgPlan p;
    HgGeom g;
    int rc = make_hg_plan(cfg, p);
    if (rc) return rc;
    if ((rc = hg_geometry(p, batch, frames, g))) return rc;
    CTTS_CHECK_ARG(packed != nullptr && mel != nullptr && audio != nullptr && workspace != nullptr, "hifigan_forward: NULL pointer");
    CTTS_CHECK_ARG(mel_ld >= frames, "hifigan_forward: mel_ld=%d < frames=%d", mel_ld, frames);
    CTTS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0,
                   "hifigan_forward: packed blob and workspace must be 16-byte aligned");
    if (workspace_bytes < g.total_floats * sizeof(float)) {
        set_error("hifigan_forward: workspace %zu bytes < required %zu", workspace_bytes, g.total_floats * sizeof(float));
        return CTTS_E_WORKSPACE;
    }
    const auto& c = p.c;
    hipStream_t s = as_stream(stream);
    const float* pk = static_cast<const float*>(packed);
    float* ws = static_cast<float*>(workspace);
    float* X = ws;
    float* XS = ws + g.buf_floats;
    float* T = ws + 2 * g.buf_floats;
    float* P[2] = {ws + 3 * g.buf_floats, ws + 4 * g.buf_floats};

    size_t li = 0;
    int L = frames, ld = round_up(L, 4);
    int C = c.upsample_initial_channel;
    {   // conv_pre (models.py:122) -> XS
        HgConvArgs a{};
        a.x = mel; a.x_bs = (long long)c.num_mels * mel_ld; a.x_ld = mel_ld; a.L = L; a.slope = 1.0f;
        a.epi = HG_EPI_STORE; a.dst0 = XS; a.dst0_bs = (long long)C * ld; a.dst0_ld = ld;
        if ((rc = hg_launch(p.layers[li++], a, pk, batch, s))) return rc;
    }
    for (int i = 0; i < c.n_ups; ++i) {
        const int u = c.upsample_rates[i];
        const int Lo = L * u, ldo = round_up(Lo, 4), Co = C / 2;
        {   // x = ups[i](leaky_relu(x, 0.1)) (models.py:124-125): XS -> X, phases interleaved by the store
            HgConvArgs a{};
            a.x = XS; a.x_bs = (long long)C * ld; a.x_ld = ld; a.L = L; a.slope = 0.1f;
            a.epi = HG_EPI_STORE; a.dst0 = X; a.dst0_bs = (long long)Co * ldo; a.dst0_ld = ldo;
            if ((rc = hg_launch(p.layers[li++], a, pk, batch, s))) return rc;
        }
        L = Lo; ld = ldo; C = Co;
        const long long bs = (long long)C * ld;
        for (int j = 0; j < c.n_kernels; ++j) {   // every resblock reads the same X (models.py:127-132)
            const size_t first = li;
            li += (c.resblock == 1 ? 2 : 1) * p.n_steps;
            const float* cur = X;
            for (int m = 0; m < p.n_steps; ++m) {
                const bool last = m == p.n_steps - 1;
                const float* in = cur;
                if (c.resblock == 1) {   // xt = c1(leaky_relu(x)) (models.py:60-62) -> T
                    HgConvArgs a{};
                    a.x = cur; a.x_bs = bs; a.x_ld = ld; a.L = L; a.slope = 0.1f;
                    a.epi = HG_EPI_STORE; a.dst0 = T; a.dst0_bs = bs; a.dst0_ld = ld;
                    if ((rc = hg_launch(p.layers[first + m], a, pk, batch, s))) return rc;
                    in = T;
                }
                // x = c(leaky_relu(.)) + x (models.py:63-65 / :88-91); the last step feeds the stage's sum and its 1 / n_k
                HgConvArgs a{};
                a.x = in; a.x_bs = bs; a.x_ld = ld; a.L = L; a.slope = 0.1f;
                a.epi = HG_EPI_RES; a.res = cur; a.res_bs = bs; a.res_ld = ld;
                if (!last) { a.dst0 = P[m & 1]; a.dst0_bs = bs; a.dst0_ld = ld; }
                else {
                    a.dst1 = XS; a.dst1_bs = bs; a.dst1_ld = ld; a.nk = (float)c.n_kernels;
                    a.sum_flags = (j == 0 ? HG_SUM_FIRST : 0) | (j == c.n_kernels - 1 ? HG_SUM_LAST : 0);
                }
                if ((rc = hg_launch(p.layers[first + (c.resblock == 1 ? 3 : 0) + m], a, pk, batch, s))) return rc;
                cur = P[m & 1];
            }
        }
    }
    {   // tanh(conv_post(leaky_relu(x))) with F.leaky_relu's default slope 0.01 (models.py:134-136) -> audio [B][1][L]
        HgConvArgs a{};
        a.x = XS; a.x_bs = (long long)C * ld; a.x_ld = ld; a.L = L; a.slope = 0.01f;
        a.epi = HG_EPI_TANH; a.dst0 = audio; a.dst0_bs = L; a.dst0_ld = L;
        if ((rc = hg_launch(p.layers[li++], a, pk, batch, s))) return rc;
    }
    return CTTS_OK;
}

}  // extern "C"
