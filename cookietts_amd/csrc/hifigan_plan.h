// HiFi-GAN generator: what the fp32 path (hifigan.hip), the IEEE-half path (hifigan_f16.hip) and the split-bf16 path
// (hifigan_bf16x3.hip) share - the layer list of a config with its refusals, the workspace geometry, the launch arguments and
// the sequence of launches of one forward; the kernels' prologue, the fp32 epilogue and the pack helpers; the launcher with its
// block-shape table; the bodies of the extern "C" entries.  A format's .hip file holds its conv kernel, its pack kernel, a
// trait struct that names them (see hg_launch) and twelve one-line entries between the three of them.
//
// `esz` is the size of a stored activation / weight element: 4 = fp32 rows [C][ld], ld = roundup(L, 4); 2 = IEEE half in
// the K8-blocked layout [ceil(C / 8)][ld][8], ld = L (a column of 8 channels is one 16-byte unit).
//
// Split bf16 keeps the fp32 tensors and carries each operand of a product as a hi | lo pair of bf16 - 4 bytes, the fp32
// element's.  It therefore IS the esz = 4 plan: the same layer list, KC (a K16 MFMA step is 16 channels of one tap at KC = 16,
// 8 channels of two taps at KC = 8), lds_bytes(), packed_bytes, offsets, workspace geometry and launch sequence; only the
// arrangement of a layer's packed weights ([MB][nch][ntap][KC / 8][hi, lo][BM][8] bf16) and of the staged tile
// ([KC / 8][hi, lo][BN + (ntap - 1) * dil] units, never wider than the fp32 tile) differ.
//
// Epilogues (no stand-alone elementwise launch anywhere in the model):
//   HG_EPI_STORE  dst0 = v; with up > 1 the rows are (phase r, channel co) of a transposed conv and the store is
//                 dst0[co][n * up + r]: the `up` stride-1 phase convolutions of ConvTranspose1d written interleaved
//   HG_EPI_RES    v += res; dst0 = v (when given); dst1 = ((first ? 0 : dst1) + v) [/ nk when last]: the residual add, the sum
//                 over the n_k resblocks of a stage and its 1 / n_k
//   HG_EPI_TANH   dst0 = tanh(v) for rows < M (conv_post; its input slope is F.leaky_relu's default 0.01, models.py:134)
// hg_epilogue_f32 is the two fp32-tensor formats'; the half format's (hifigan_f16.hip) does the same in half units.
//
// Block shapes (256 threads = 4 waves, wave tile 32 MT x 64): BM = 32 MT WM rows, BN = 64 (4 / WM) columns:
//   M <= 32: 32 x 256    M <= 64: 64 x 256    else: 128 x 128 (M-blocks of 128 rows)
// and, for launches too small to fill the chip with those (batch 1), 64 x 128 / 128 x 64 on the same packed weights.
// The K chunk is the format's high KC (16 fp32 or split rows, 32 half rows) where the two LDS images stay under HG_LDS_KC16
// bytes, else half of it.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"

namespace ctts {
namespace {

enum { HG_EPI_STORE = 0, HG_EPI_RES = 1, HG_EPI_TANH = 2 };
enum { HG_SUM_FIRST = 1, HG_SUM_LAST = 2 };
enum { HG_CONV = 0, HG_CONVT = 1 };

constexpr int HG_MAX_KERNEL = 11;         // resblock kernel size (odd)
constexpr int HG_MAX_HALO = 128;          // (k - 1) * dilation
constexpr int HG_MAX_UP_TAPS = 5;         // taps of a phase convolution incl. the zero-weight ones
constexpr int HG_LDS_MAX = 64 * 1024;     // dynamic LDS a launch may ask for
constexpr int HG_LDS_KC16 = 40 * 1024;    // the larger K chunk only while four workgroups still fit a CU's LDS
constexpr int HG_NARROW_BELOW = 1024;     // workgroups (4 per CU) under which the half-width block shape is launched

// T = float (hifigan.hip, hifigan_bf16x3.hip) or _Float16 (hifigan_f16.hip)
template <typename T>
struct HgConvArgsT {
    const T* A;            // packed weights of the layer
    const float* bias;     // [MB * BM]
    const T* x;            // input activations
    const float* xf;       // half path only: the fp32 mel [B][Cin][x_ld] of conv_pre (x is NULL then)
    long long x_bs;
    int x_ld, x_vec;       // x_vec (read by hg_conv_kernel only): rows are 16-byte aligned (float4 staging)
    int Cin, L;            // valid input channels; valid columns (input and output share the column domain)
    int ntap, dil, left;   // tap j reads column n + j * dil - left
    float slope;           // LeakyReLU slope applied to x while staging (1 = none)
    int M, MB, ntiles, nch;
    int epi;
    T* dst0; long long dst0_bs; int dst0_ld;
    float* dstf;           // half path only: the fp32 waveform of HG_EPI_TANH
    int up, cout;          // HG_EPI_STORE: up > 1 = interleaved phase store
    const T* res; long long res_bs; int res_ld;
    T* dst1; long long dst1_bs; int dst1_ld;
    int sum_flags; float nk;
};

// ---- plan: the layer list of one config, shared by the size queries, the pack and the forward ----
struct HgLayer {
    int kind, Cin, M, cout, up, ku, pad, ntap, dil, left;
    int MT, WM, KC, BM, BN, MB, nch, esz;
    size_t w_off, b_off;         // floats into the caller's flat folded weights
    size_t A_off, bias_off;      // bytes into the packed blob
    int lds_bytes(int bn) const {
        if (esz == 2) return (ntap * KC * BM + KC * (bn + (ntap - 1) * dil)) * 2;
        const int aleft = (left + 3) & ~3;
        const int XW = (bn + (ntap - 1) * dil - left + aleft + 3) & ~3;
        return (ntap * KC * BM + KC * XW) * 4;
    }
    int lds_bytes() const { return lds_bytes(BN); }
    size_t packed_elems() const { return (size_t)MB * nch * ntap * KC * BM; }
};

struct HgPlan {
    ctts_hifigan_config c;
    std::vector<HgLayer> layers;     // conv_pre, then per stage: ups_i, its n_k resblocks' convs in module order; conv_post last
    std::vector<int> chans;          // channels after stage i
    int n_steps;                     // convs1/convs2 pairs (ResBlock1: 3) or convs (ResBlock2: 2) per resblock
    int esz;
    long long up_total;              // prod(upsample_rates)
    size_t weight_floats, packed_bytes;
};

inline size_t hg_align(size_t v) { return (v + 255) / 256 * 256; }      // bytes

int hg_add_layer(HgPlan& p, int kind, int Cin, int M, int cout, int up, int ku, int pad, int ntap, int dil, int left, const char* what) {
    HgLayer l{};
    l.kind = kind; l.Cin = Cin; l.M = M; l.cout = cout; l.up = up; l.ku = ku; l.pad = pad; l.ntap = ntap; l.dil = dil; l.left = left;
    l.esz = p.esz;
    if (M <= 32) { l.MT = 1; l.WM = 1; }
    else if (M <= 64) { l.MT = 2; l.WM = 1; }
    else { l.MT = 2; l.WM = 2; }
    l.BM = 32 * l.MT * l.WM;
    l.BN = 64 * (4 / l.WM);
    l.MB = (M + l.BM - 1) / l.BM;
    // K chunk: 16 / 8 fp32 rows, 32 / 16 half rows (the f16 MFMA step is 16 deep): the same LDS bytes either way
    const int kc_hi = p.esz == 2 ? 32 : 16, kc_lo = kc_hi / 2;
    l.KC = kc_hi;
    if (Cin <= kc_lo || l.lds_bytes() > HG_LDS_KC16) l.KC = kc_lo;
    CTTS_CHECK_ARG(l.lds_bytes() <= HG_LDS_MAX, "hifigan: %s needs %d bytes of LDS (limit %d)", what, l.lds_bytes(), HG_LDS_MAX);
    l.nch = (Cin + l.KC - 1) / l.KC;
    l.w_off = p.weight_floats;
    const size_t wn = kind == HG_CONV ? (size_t)M * Cin * ntap : (size_t)Cin * cout * ku;
    l.b_off = l.w_off + wn;
    p.weight_floats = l.b_off + (kind == HG_CONV ? M : cout);
    l.A_off = p.packed_bytes;
    l.bias_off = l.A_off + hg_align(l.packed_elems() * p.esz);
    p.packed_bytes = l.bias_off + hg_align((size_t)l.MB * l.BM * sizeof(float));
    p.layers.push_back(l);
    return CTTS_OK;
}

int make_hg_plan(const ctts_hifigan_config* cfg, HgPlan& p, int esz) {
    CTTS_CHECK_ARG(cfg != nullptr, "hifigan: config is NULL");
    p.c = *cfg;
    p.esz = esz;
    const auto& c = p.c;
    p.weight_floats = p.packed_bytes = 0;
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

struct HgGeom { size_t buf_elems; size_t total_elems; };

inline int hg_ld(int esz, int L) { return esz == 2 ? L : round_up(L, 4); }          // row pitch in columns
inline int hg_rows(int esz, int C) { return esz == 2 ? round_up(C, 8) : C; }        // stored channel rows

// five activation buffers (stage input x, resblock sum xs, the c1 output, two ping-pong resblock states), each
// batch * max over the tensors of the call of rows(C) * ld(L) elements
int hg_geometry(const HgPlan& p, int batch, int frames, HgGeom& g) {
    CTTS_CHECK_ARG(batch >= 1 && batch <= 4096, "hifigan: batch=%d (1..4096)", batch);
    CTTS_CHECK_ARG(frames >= 1 && (long long)frames * p.up_total <= (1ll << 30), "hifigan: frames=%d (>= 1, frames * prod(rates) <= 2^30)", frames);
    long long L = frames;
    size_t mx = (size_t)hg_rows(p.esz, p.c.upsample_initial_channel) * hg_ld(p.esz, (int)L);
    for (int i = 0; i < p.c.n_ups; ++i) {
        L *= p.c.upsample_rates[i];
        mx = std::max(mx, (size_t)hg_rows(p.esz, p.chans[i]) * (size_t)hg_ld(p.esz, (int)L));
    }
    g.buf_elems = hg_align(mx * (size_t)batch * p.esz) / p.esz;
    g.total_elems = 5 * g.buf_elems;
    return CTTS_OK;
}

// Generator.forward (models.py:121-137) as its sequence of launches; `launch(layer, args)` starts one conv.
template <typename T, typename Launch>
int hg_forward(const HgPlan& p, const HgGeom& g, const float* mel, int mel_ld, float* audio, int frames, T* ws, Launch launch) {
    using Args = HgConvArgsT<T>;
    constexpr bool kF32 = std::is_same<T, float>::value;
    const auto& c = p.c;
    const int esz = p.esz;
    int rc;
    T* X = ws;
    T* XS = ws + g.buf_elems;
    T* Tm = ws + 2 * g.buf_elems;
    T* P[2] = {ws + 3 * g.buf_elems, ws + 4 * g.buf_elems};

    size_t li = 0;
    int L = frames, ld = hg_ld(esz, L);
    int C = c.upsample_initial_channel;
    {   // conv_pre (models.py:122) -> XS
        Args a{};
        if constexpr (kF32) a.x = mel; else a.xf = mel;
        a.x_bs = (long long)c.num_mels * mel_ld; a.x_ld = mel_ld; a.L = L; a.slope = 1.0f;
        a.epi = HG_EPI_STORE; a.dst0 = XS; a.dst0_bs = (long long)hg_rows(esz, C) * ld; a.dst0_ld = ld;
        if ((rc = launch(p.layers[li++], a))) return rc;
    }
    for (int i = 0; i < c.n_ups; ++i) {
        const int u = c.upsample_rates[i];
        const int Lo = L * u, ldo = hg_ld(esz, Lo), Co = C / 2;
        {   // x = ups[i](leaky_relu(x, 0.1)) (models.py:124-125): XS -> X, phases interleaved by the store
            Args a{};
            a.x = XS; a.x_bs = (long long)hg_rows(esz, C) * ld; a.x_ld = ld; a.L = L; a.slope = 0.1f;
            a.epi = HG_EPI_STORE; a.dst0 = X; a.dst0_bs = (long long)hg_rows(esz, Co) * ldo; a.dst0_ld = ldo;
            if ((rc = launch(p.layers[li++], a))) return rc;
        }
        L = Lo; ld = ldo; C = Co;
        const long long bs = (long long)hg_rows(esz, C) * ld;
        for (int j = 0; j < c.n_kernels; ++j) {   // every resblock reads the same X (models.py:127-132)
            const size_t first = li;
            li += (c.resblock == 1 ? 2 : 1) * p.n_steps;
            const T* cur = X;
            for (int m = 0; m < p.n_steps; ++m) {
                const bool last = m == p.n_steps - 1;
                const T* in = cur;
                if (c.resblock == 1) {   // xt = c1(leaky_relu(x)) (models.py:60-62) -> Tm
                    Args a{};
                    a.x = cur; a.x_bs = bs; a.x_ld = ld; a.L = L; a.slope = 0.1f;
                    a.epi = HG_EPI_STORE; a.dst0 = Tm; a.dst0_bs = bs; a.dst0_ld = ld;
                    if ((rc = launch(p.layers[first + m], a))) return rc;
                    in = Tm;
                }
                // x = c(leaky_relu(.)) + x (models.py:63-65 / :88-91); the last step feeds the stage's sum and its 1 / n_k
                Args a{};
                a.x = in; a.x_bs = bs; a.x_ld = ld; a.L = L; a.slope = 0.1f;
                a.epi = HG_EPI_RES; a.res = cur; a.res_bs = bs; a.res_ld = ld;
                if (!last) { a.dst0 = P[m & 1]; a.dst0_bs = bs; a.dst0_ld = ld; }
                else {
                    a.dst1 = XS; a.dst1_bs = bs; a.dst1_ld = ld; a.nk = (float)c.n_kernels;
                    a.sum_flags = (j == 0 ? HG_SUM_FIRST : 0) | (j == c.n_kernels - 1 ? HG_SUM_LAST : 0);
                }
                if ((rc = launch(p.layers[first + (c.resblock == 1 ? 3 : 0) + m], a))) return rc;
                cur = P[m & 1];
            }
        }
    }
    {   // tanh(conv_post(leaky_relu(x))) with F.leaky_relu's default slope 0.01 (models.py:134-136) -> audio [B][1][L]
        Args a{};
        a.x = XS; a.x_bs = (long long)hg_rows(esz, C) * ld; a.x_ld = ld; a.L = L; a.slope = 0.01f;
        a.epi = HG_EPI_TANH;
        if constexpr (kF32) a.dst0 = audio; else a.dstf = audio;
        a.dst0_bs = L; a.dst0_ld = L;
        if ((rc = launch(p.layers[li++], a))) return rc;
    }
    return CTTS_OK;
}

// the pack kernels' arguments (T as above); A is [MB][nch][ntap][KC][BM] in fp32, [MB][nch][ntap][KC / 8][BM][8] in half,
// [MB][nch][ntap][KC / 8][hi, lo][BM][8] bf16 in the split format (T = float: the same bytes)
template <typename T>
struct HgPackArgsT {
    const float* w;        // HG_CONV: [M][Cin][k]; HG_CONVT: [Cin][cout][ku]
    const float* b;        // [M] / [cout]
    T* A;
    float* bias;
    int kind, Cin, M, cout, up, ku, pad, ntap, left, KC, BM, MB, nch;
};

template <typename T>
HgPackArgsT<T> hg_pack_args(const HgLayer& l, const float* weights, void* packed) {
    HgPackArgsT<T> a{};
    char* out = static_cast<char*>(packed);
    a.w = weights + l.w_off; a.b = weights + l.b_off;
    a.A = reinterpret_cast<T*>(out + l.A_off); a.bias = reinterpret_cast<float*>(out + l.bias_off);
    a.kind = l.kind; a.Cin = l.Cin; a.M = l.M; a.cout = l.cout > 0 ? l.cout : 1; a.up = l.up; a.ku = l.ku; a.pad = l.pad;
    a.ntap = l.ntap; a.left = l.left; a.KC = l.KC; a.BM = l.BM; a.MB = l.MB; a.nch = l.nch;
    return a;
}

// the folded weight (m, ci, tap j) of a layer from the caller's flat buffer; 0 outside the layer (padding rows / channels and
// the dead taps of a transposed conv's phase)
template <typename T>
__device__ __forceinline__ float hg_weight_at(const HgPackArgsT<T>& p, int m, int ci, int j) {
    if (m >= p.M || ci >= p.Cin) return 0.0f;
    if (p.kind == HG_CONV) return p.w[((size_t)m * p.Cin + ci) * p.ntap + j];
    const int ph = m / p.cout, co = m - ph * p.cout;
    const int kk = p.up * (p.left - j) + ph + p.pad;
    return (kk >= 0 && kk < p.ku) ? p.w[((size_t)ci * p.cout + co) * p.ku + kk] : 0.0f;
}

// ---- pack kernels: the bias block (thread i < MB * BM writes bias[i]) and the K8 coordinates of element i of a layer's A ----
template <typename T>
__device__ __forceinline__ void hg_pack_bias(const HgPackArgsT<T>& p, long long i) {
    if (i < (long long)p.MB * p.BM) {
        const int m = (int)i;
        p.bias[m] = m < p.M ? p.b[p.kind == HG_CONVT ? m % p.cout : m] : 0.0f;
    }
}

struct HgK8 { int e, r, kg, j, ch, mb; };      // i = ((((mb * nch + ch) * ntap + j) * (KC / 8) + kg) * BM + r) * 8 + e

template <typename T>
__device__ __forceinline__ HgK8 hg_pack_k8(const HgPackArgsT<T>& p, long long q) {
    HgK8 k;
    k.e = (int)(q & 7); q >>= 3;
    k.r = (int)(q % p.BM); q /= p.BM;
    k.kg = (int)(q % (p.KC / 8)); q /= (p.KC / 8);
    k.j = (int)(q % p.ntap); q /= p.ntap;
    k.ch = (int)(q % p.nch); q /= p.nch;
    k.mb = (int)q;
    return k;
}

// ---- conv kernels: where a thread stands, the accumulators, the fp32 epilogue ----
typedef float f32x16 __attribute__((ext_vector_type(16)));

// M-block, column tile and batch item of the workgroup; the wave's place in the WM x (4 / WM) grid of waves; the lane's
// column and half inside the 32x32 MFMA.  The tile's first column, n0 = tile * BN, is formed in the kernel itself: there the
// compiler knows it for a multiple of BN from its first pass on, and folds the bounds tests of the float4 staging on that.
struct HgTile { int mb, tile, b, wm, wn, l31, lhi; };

template <int WM, typename Args>
__device__ __forceinline__ HgTile hg_tile(const Args& a) {
    constexpr int WN = 4 / WM;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    HgTile c;
    c.wm = wave / WN; c.wn = wave % WN;
    c.l31 = lane & 31; c.lhi = lane >> 5;
    int id = blockIdx.x;
    c.mb = id % a.MB;
    id /= a.MB;
    c.tile = id % a.ntiles;
    c.b = id / a.ntiles;
    return c;
}

template <int MT>
__device__ __forceinline__ void hg_zero(f32x16 (&acc)[MT][2]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
}

// fp32 tensors.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
template <int MT, int WM>
__device__ __forceinline__ void hg_epilogue_f32(const HgConvArgsT<float>& a, const f32x16 (&acc)[MT][2], const HgTile c, const int n0) {
    constexpr int BM = 32 * MT * WM;
    const int mb = c.mb, b = c.b, wm = c.wm, wn = c.wn, l31 = c.l31, lhi = c.lhi;
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

// ---- launcher.  Fmt is the trait struct beside a format's kernels:
//   T                       float / _Float16: the element of HgConvArgsT / HgPackArgsT and of the workspace (esz = sizeof(T))
//   kc_lo                   the low K chunk (8 / 16); the high one is twice that
//   name, kernel            "hifigan..." for the no-kernel-shape message, the conv kernel's name for a launch error
//   launch<MT, WM, KC>(args, blocks, lds, stream)     starts the conv kernel of that shape
//   pack_kernel, pack(args, blocks, stream)           the pack kernel's name and its launch
template <typename Fmt>
int hg_launch(const HgLayer& l, HgConvArgsT<typename Fmt::T> a, const void* packed, int batch, hipStream_t s) {
    using T = typename Fmt::T;
    a.A = reinterpret_cast<const T*>(static_cast<const char*>(packed) + l.A_off);
    a.bias = reinterpret_cast<const float*>(static_cast<const char*>(packed) + l.bias_off);
    a.Cin = l.Cin; a.ntap = l.ntap; a.dil = l.dil; a.left = l.left;
    a.M = l.M; a.MB = l.MB; a.nch = l.nch;
    // a launch that would start fewer than HG_NARROW_BELOW workgroups takes the half-width block of the same M-block height
    // (waves stacked along M): same packed weights, same K order, bit-identical results, twice the workgroups to spread
    int WM = l.WM, MT = l.MT, BN = l.BN;
    if (l.BM >= 64 && (long long)l.MB * ((a.L + BN - 1) / BN) * batch < HG_NARROW_BELOW) { WM *= 2; MT = 1; BN /= 2; }
    a.ntiles = (a.L + BN - 1) / BN;
    a.up = l.up; a.cout = l.cout;
    if constexpr (std::is_same<T, float>::value)
        a.x_vec = (a.x_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 && a.x_bs % 4 == 0) ? 1 : 0;
    // split bf16: the fp32 plan's LDS figure covers its layout - the same weight bytes, and a tile that is no wider (no
    // 16-byte row alignment)
    const int lds = l.lds_bytes(BN);
    const unsigned blocks = (unsigned)((size_t)a.MB * a.ntiles * batch);
    constexpr int K0 = Fmt::kc_lo, K1 = 2 * K0;
    const int key = MT * 100 + WM * 10 + (l.KC == K1);
    switch (key) {
        case 110: Fmt::template launch<1, 1, K0>(a, blocks, lds, s); break;
        case 111: Fmt::template launch<1, 1, K1>(a, blocks, lds, s); break;
        case 120: Fmt::template launch<1, 2, K0>(a, blocks, lds, s); break;
        case 121: Fmt::template launch<1, 2, K1>(a, blocks, lds, s); break;
        case 140: Fmt::template launch<1, 4, K0>(a, blocks, lds, s); break;
        case 141: Fmt::template launch<1, 4, K1>(a, blocks, lds, s); break;
        case 210: Fmt::template launch<2, 1, K0>(a, blocks, lds, s); break;
        case 211: Fmt::template launch<2, 1, K1>(a, blocks, lds, s); break;
        case 220: Fmt::template launch<2, 2, K0>(a, blocks, lds, s); break;
        case 221: Fmt::template launch<2, 2, K1>(a, blocks, lds, s); break;
        default: set_error("%s: no kernel shape %d", Fmt::name, key); return CTTS_E_ARG;
    }
    CTTS_CHECK_LAUNCH(Fmt::kernel);
    return CTTS_OK;
}

// ---- the bodies of the extern "C" entries; `entry` is the name the messages carry ("hifigan_pack_f16", ...) ----
template <typename Fmt>
size_t hg_packed_bytes(const ctts_hifigan_config* cfg) {
    HgPlan p;
    if (make_hg_plan(cfg, p, sizeof(typename Fmt::T)) != CTTS_OK) return 0;
    return p.packed_bytes;
}

// one pack launch per layer; aligned16: the blob is refused unless 16-byte aligned
template <typename Fmt>
int hg_pack(const char* entry, bool aligned16, const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed,
            void* stream) {
    using T = typename Fmt::T;
    HgPlan p;
    int rc = make_hg_plan(cfg, p, sizeof(T));
    if (rc) return rc;
    CTTS_CHECK_ARG(weights != nullptr && packed != nullptr, "%s: NULL pointer", entry);
    CTTS_CHECK_ARG(weight_floats == p.weight_floats, "%s: %zu weight floats given, the config has %zu", entry, weight_floats,
                   p.weight_floats);
    CTTS_CHECK_ARG(!aligned16 || (reinterpret_cast<uintptr_t>(packed) & 15) == 0, "%s: packed blob must be 16-byte aligned", entry);
    for (const HgLayer& l : p.layers) {
        const long long total = (long long)l.packed_elems();     // >= MB * BM
        Fmt::pack(hg_pack_args<T>(l, weights, packed), (unsigned)((total + 255) / 256), as_stream(stream));
        CTTS_CHECK_LAUNCH(Fmt::pack_kernel);
    }
    return CTTS_OK;
}

template <typename Fmt>
size_t hg_workspace_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames) {
    HgPlan p;
    HgGeom g;
    if (make_hg_plan(cfg, p, sizeof(typename Fmt::T)) != CTTS_OK || hg_geometry(p, batch, frames, g) != CTTS_OK) return 0;
    return g.total_elems * sizeof(typename Fmt::T);
}

template <typename Fmt>
int hg_forward_entry(const char* entry, const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld, float* audio,
                     int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    using T = typename Fmt::T;
    HgPlan p;
    HgGeom g;
    int rc = make_hg_plan(cfg, p, sizeof(T));
    if (rc) return rc;
    if ((rc = hg_geometry(p, batch, frames, g))) return rc;
    CTTS_CHECK_ARG(packed != nullptr && mel != nullptr && audio != nullptr && workspace != nullptr, "%s: NULL pointer", entry);
    CTTS_CHECK_ARG(mel_ld >= frames, "%s: mel_ld=%d < frames=%d", entry, mel_ld, frames);
    CTTS_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0,
                   "%s: packed blob and workspace must be 16-byte aligned", entry);
    if (workspace_bytes < g.total_elems * sizeof(T)) {
        set_error("%s: workspace %zu bytes < required %zu", entry, workspace_bytes, g.total_elems * sizeof(T));
        return CTTS_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    return hg_forward<T>(p, g, mel, mel_ld, audio, frames, static_cast<T*>(workspace),
                         [&](const HgLayer& l, const HgConvArgsT<T>& a) { return hg_launch<Fmt>(l, a, packed, batch, s); });
}

}  // namespace
}  // namespace ctts
