// The headline launch alone: WaveGlow config 2 in-layer GEMM (M = 1024, K = 3 x 512 + 256 = 112 chunks, 8 x 28 800 columns,
// GATE epilogue), the product kernel of cookietts_amd/csrc/gemm_f32.hip compiled into this file, timed with HIP events
// over 24 launches on rotating weights - the product loop, without the rest of the model around it.  Round 3 used it with
// temporary patches of the main loop to bound what each ingredient costs (profiles/r3_15_headline_gemm_experiments.txt):
// per launch 6.20 ms as shipped (6.28 with the hand-scheduled variant the other figures build on); LDS-DMA issue removed
// 5.86; fragment reads removed 6.26; barrier removed 6.33; all three removed 5.78 ms (0.93 of the fp32 MFMA peak).  A DMA instruction costs the same with 4-byte lanes, with one M0
// value for all pieces, as buffer_load ... lds, and without the vmcnt wait: it is the ISSUE of the six LDS-DMA
// instructions per wave and chunk (~55 matrix-pipe cycles each) that the loop pays, not their data path.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I cookietts_amd/csrc scripts/micro/headline_gemm.hip -o /tmp/headline_gemm
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cookietts_amd/csrc/gemm_f32.hip"
#include "../../cookietts_amd/csrc/wn_winograd_layer.hip"
#include "../../cookietts_amd/csrc/waveglow_kernels.hip"

namespace ctts {
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
bool gemm_f32_small_applies(int, const GemmArgs&) { return false; }
int launch_gemm_f32_small(int, const GemmArgs&, hipStream_t) { return CTTS_E_ARG; }
int wf_row_cus() { return 256; }
// Whole wide rounds below which the F(4,3) layer stays on the 64-column shape (a wide round = one workgroup per CU)
constexpr int WNWG_F43_WIDE_MIN_ROUNDS = 2;

// The F(4,3) launch as the go / no-go of the 128-column shape ran it (HG_F43_WIDE; the library keeps the 64-column shape at every
// size, wn_winograd_layer.hip): a.ntiles counts 64-column tiles, KDN / KDW = chunks per stage of the 64- and of the 128-column
// shape.  narrow / wide: that shape everywhere; neither: by grid size, with the round-aligned peel of the F(2,3) branch.
template <int KDN, int KDW>
int launch_wnwg_f43(const WnWinogradLayerArgs& a, bool narrow, bool wide, bool no_round_split, hipStream_t stream) {
    const int ncb = a.C / 64;
    const long long slots = wf_row_cus();                 // 512 registers per lane: one workgroup per CU
    const int wt = (a.ntiles + 1) / 2;                    // 128-column tiles per batch item
    long long tiles = (long long)wt * a.batch;
    if (!wide && (narrow || ncb * tiles < WNWG_F43_WIDE_MIN_ROUNDS * slots || (long long)wt * 128 > a.ldp)) {
        return launch_wnwg_shape<1, 1, KDN, 1>(a, a.ntiles, (long long)a.ntiles * a.batch, stream);
    }
    CTTS_CHECK_ARG((long long)wt * 128 <= a.ldp, "wn_winograd_layer: %d tiles of 128 quad columns beyond ldp=%d", wt, a.ldp);
    if (!wide && !no_round_split) {
        const long long rounds = ncb * tiles / slots;
        const long long rem_tiles = (ncb * tiles - rounds * slots + ncb - 1) / ncb;
        if (rounds >= 2 && rem_tiles > 0 && rem_tiles * ncb <= slots * 3 / 10 && rem_tiles < wt && (long long)(wt - rem_tiles) * 128 < a.Lp) {
            WnWinogradLayerArgs r = a;
            r.b0 = a.batch - 1;
            r.col0 = (int)(wt - rem_tiles) * 128;
            const int kt = (a.Lp - r.col0 + 63) / 64;
            if (int rc = launch_wnwg_shape<1, 1, KDN, 1>(r, kt, kt, stream)) return rc;
            tiles -= rem_tiles;
        }
    }
    return launch_wnwg_shape<2, 1, KDW, 1>(a, wt, tiles, stream);
}
}  // namespace ctts
using namespace ctts;
// stand-in for the traffic of a Winograd F(2,3) input transform: every thread reads 3 and writes 5 16-byte units
__global__ __launch_bounds__(256) void stream_3r5w_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = src[i], b = src[n + i], c = src[2 * n + i];
    dst[i] = a; dst[n + i] = b; dst[2 * n + i] = c;
    dst[3 * n + i] = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
    dst[4 * n + i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
}
// stand-in for the traffic of the F(4,3) quad transform: six taps read, six V planes written per 16-byte unit
__global__ __launch_bounds__(256) void stream_6r6w_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = src[j * n + i];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float4 p = v[j], q = v[(j + 1) % 6], r = v[(j + 2) % 6];
        dst[j * n + i] = make_float4(p.x - q.x + r.x, p.y - q.y + r.y, p.z - q.z + r.z, p.w - q.w + r.w);
    }
}
// The F(4,3) layer (wn_winograd_layer.h, form = WNWG_F43) straight from its packed operands, one thread per (quad column, channel,
// batch item): what the one-launch kernel's chunk stream, half-panel addressing and quad map have to reproduce.
__global__ __launch_bounds__(256) void f43_reference_kernel(const WnWinogradLayerArgs a, float* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y, b = blockIdx.z;
    if (q >= a.Lp) return;
    const int n1 = a.C / GEMM_KC, n2 = (a.C + a.H) / GEMM_KC, cb = ch >> 6, i = ch & 63;
    auto split = [&](const float* P, int row, int kk) { return P[((size_t)(row >> 8) * n1 + kk / GEMM_KC) * (GEMM_KC * 256) + (kk % GEMM_KC) * 256 + (row & 255)]; };
    auto gate = [&](const float* P, int r, int kk) { return P[((size_t)(cb >> 1) * n2 + kk / GEMM_KC) * (GEMM_KC * 256) + (kk % GEMM_KC) * 256 + (cb & 1) * 128 + r]; };
    auto vq = [&](int j, int kk) { return a.V[j * a.vplane + ((size_t)b * a.C + kk) * a.ldp + q]; };
    const float* U[4] = {a.A_T2, a.A_T3, a.A_T4, a.A_T5};
    float pt[4], pg[4];
    for (int j = 0; j < 4; ++j) {
        float t = 0.f, g = 0.f;
        for (int kk = 0; kk < a.C; ++kk) { const float v = vq(1 + j, kk); t = fmaf(split(U[j], ch, kk), v, t); g = fmaf(split(U[j], a.C + ch, kk), v, g); }
        pt[j] = t; pg[j] = g;
    }
    float y[2][4];
    for (int s = 0; s < 2; ++s) {
        const float* p = s ? pg : pt;
        const float sa = p[0] + p[1], sb = p[0] - p[1], sc = p[2] + p[3], se = p[2] - p[3];
        y[s][0] = sa + sc; y[s][1] = sb + 2.f * se; y[s][2] = sa + 4.f * sc; y[s][3] = sb + 8.f * se;
    }
    for (int k = 0; k < 4; ++k) {
        const int tk = (q / a.d) * (4 * a.d) + q % a.d + k * a.d;
        if (tk >= a.L) continue;
        const float* P = k == 3 ? a.A_o : a.A_e;
        float t = 0.f, g = 0.f;
        if (k == 0 || k == 3)
            for (int kk = 0; kk < a.C; ++kk) { const float v = vq(k == 3 ? 5 : 0, kk); t = fmaf(gate(P, i, kk), v, t); g = fmaf(gate(P, 64 + i, kk), v, g); }
        for (int kk = 0; kk < a.H; ++kk) {
            const float v = a.h2[(size_t)b * a.h_bstride + (size_t)kk * a.ld + a.pad + tk];
            t = fmaf(gate(P, i, a.C + kk), v, t); g = fmaf(gate(P, 64 + i, a.C + kk), v, g);
        }
        const float u0 = y[0][k] + t + a.bias[cb * 128 + i], u1 = y[1][k] + g + a.bias[cb * 128 + 64 + i];
        out[(size_t)b * a.act_bstride + (size_t)ch * a.ld + a.pad + tk] = tanhf(u0) / (1.f + expf(-u1));
    }
}
// The F(6,3) layer (form = WNWG_F63) the same way: six interior products, the hex map, the cond chunks of the first GATE panel for
// the four middle members.
__global__ __launch_bounds__(256) void f63_reference_kernel(const WnWinogradLayerArgs a, float* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y, b = blockIdx.z;
    if (q >= a.Lp) return;
    const int n1 = a.C / GEMM_KC, n2 = (a.C + a.H) / GEMM_KC, cb = ch >> 6, i = ch & 63;
    auto split = [&](const float* P, int row, int kk) { return P[((size_t)(row >> 8) * n1 + kk / GEMM_KC) * (GEMM_KC * 256) + (kk % GEMM_KC) * 256 + (row & 255)]; };
    auto gate = [&](const float* P, int r, int kk) { return P[((size_t)(cb >> 1) * n2 + kk / GEMM_KC) * (GEMM_KC * 256) + (kk % GEMM_KC) * 256 + (cb & 1) * 128 + r]; };
    auto vq = [&](int j, int kk) { return a.V[j * a.vplane + ((size_t)b * a.C + kk) * a.ldp + q]; };
    const float* U[6] = {a.A_T2, a.A_T3, a.A_T4, a.A_T5, a.A_T6, a.A_T7};
    float pt[6], pg[6];
    for (int j = 0; j < 6; ++j) {
        float t = 0.f, g = 0.f;
        for (int kk = 0; kk < a.C; ++kk) { const float v = vq(1 + j, kk); t = fmaf(split(U[j], ch, kk), v, t); g = fmaf(split(U[j], a.C + ch, kk), v, g); }
        pt[j] = t; pg[j] = g;
    }
    float y[2][6];
    for (int s = 0; s < 2; ++s) {
        const float* p = s ? pg : pt;
        const float sa = p[0] + p[1], sb = p[0] - p[1], sc = p[2] + p[3], se = p[2] - p[3], sf = p[4] + p[5], sg = p[4] - p[5];
        y[s][0] = (sa + sc) + sf; y[s][1] = (sb + 2.f * se) + 0.5f * sg; y[s][2] = (sa + 4.f * sc) + 0.25f * sf;
        y[s][3] = (sb + 8.f * se) + 0.125f * sg; y[s][4] = (sa + 16.f * sc) + 0.0625f * sf; y[s][5] = (sb + 32.f * se) + 0.03125f * sg;
    }
    for (int k = 0; k < 6; ++k) {
        const int tk = (q / a.d) * (6 * a.d) + q % a.d + k * a.d;
        if (tk >= a.L) continue;
        const float* P = k == 5 ? a.A_o : a.A_e;
        float t = 0.f, g = 0.f;
        if (k == 0 || k == 5)
            for (int kk = 0; kk < a.C; ++kk) { const float v = vq(k == 5 ? 7 : 0, kk); t = fmaf(gate(P, i, kk), v, t); g = fmaf(gate(P, 64 + i, kk), v, g); }
        for (int kk = 0; kk < a.H; ++kk) {
            const float v = a.h2[(size_t)b * a.h_bstride + (size_t)kk * a.ld + a.pad + tk];
            t = fmaf(gate(P, i, a.C + kk), v, t); g = fmaf(gate(P, 64 + i, a.C + kk), v, g);
        }
        const float u0 = y[0][k] + t + a.bias[cb * 128 + i], u1 = y[1][k] + g + a.bias[cb * 128 + 64 + i];
        out[(size_t)b * a.act_bstride + (size_t)ch * a.ld + a.pad + tk] = tanhf(u0) / (1.f + expf(-u1));
    }
}
// out[0] = max |a - b|, out[1] = max |a| (as the bits of non-negative floats)
__global__ __launch_bounds__(256) void max_diff_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, unsigned* out) {
    float d = 0.f, m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        d = fmaxf(d, fabsf(a[i] - b[i]));
        m = fmaxf(m, fabsf(a[i]));
    }
    atomicMax(out, __float_as_uint(d));
    atomicMax(out + 1, __float_as_uint(m));
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

int main(int argc, char** argv) {
    const char* label = argc > 1 ? argv[1] : "product";
    setenv("CTTS_F32_NO_ROUND_SPLIT", "1", 1);           // this file times ONE large-shape launch (the small shape is not linked in)
    const int C = 512, CC = 256, B = 8, PADC = 128, layers = 8;
    const int L = getenv("HG_L") ? atoi(getenv("HG_L")) : 28800;      // (multiples of 128; 28 672 = exactly 14 rounds of 512 workgroups)
    const int ld = L + 2 * PADC;
    const int nch = 3 * C / GEMM_KC + CC / GEMM_KC;      // 112
    const size_t a_tile = (size_t)GEMM_KC * 256;
    float *x, *h, *act, *A, *bias;
    CK(hipMalloc(&x, (size_t)B * C * ld * 4)); CK(hipMalloc(&h, (size_t)B * CC * ld * 4)); CK(hipMalloc(&act, (size_t)B * C * ld * 4));
    CK(hipMalloc(&A, (size_t)layers * 4 * nch * a_tile * 4)); CK(hipMalloc(&bias, 1024 * 4));
    CK(hipMemset(bias, 0, 1024 * 4)); CK(hipMemset(act, 0, (size_t)B * C * ld * 4));
    {
        std::vector<float> w((size_t)layers * 4 * nch * a_tile);
        unsigned s = 12345u;
        for (auto& v : w) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 9) % 2001 - 1000) * 2e-5f; }
        CK(hipMemcpy(A, w.data(), w.size() * 4, hipMemcpyHostToDevice));
        std::vector<float> hx((size_t)B * C * ld);
        for (auto& v : hx) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 9) % 2001 - 1000) * 1e-3f; }
        CK(hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(h, hx.data(), (size_t)B * CC * ld * 4, hipMemcpyHostToDevice));
    }
    auto args = [&](int layer) {
        GemmArgs a{};
        a.ld = ld; a.pad = PADC; a.L = L; a.ntiles = L / 128; a.batch = B; a.dst_ld = ld; a.dst_pad = PADC; a.bm = 256;
        a.A = A + (size_t)layer * 4 * nch * a_tile; a.bias = bias;
        a.nseg = 4; a.interleave = 3; a.nch_total = nch; a.MB = 4;
        const int dil = 1 << layer;
        for (int t = 0; t < 3; ++t) a.seg[t] = {x, (long long)C * ld, C / GEMM_KC, (t - 1) * dil, 0, 0};
        a.seg[3] = {h, (long long)CC * ld, CC / GEMM_KC, 0, 0, 0};
        a.dst0 = act; a.dst0_bstride = (long long)C * ld; a.M = 2 * C; a.pairC = C;
        a.gemm_mode = CTTS_GEMM_F32;
        return a;
    };
    hipStream_t st; CK(hipStreamCreate(&st));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    if (getenv("HG_WINOGRAD")) {
        // The four launches a Winograd F(2,3) form of this layer would make, in its pair space (half the columns per batch item,
        // HG_WT column tiles, pad 0), and a stand-in for its transform's traffic (profiles/r12_01_winograd_launch_shapes.txt):
        //   2 x (M = 1024, K = C = 32 chunks, SPLIT plain store)  +  2 x (M = 1024, K = C + CC = 48 chunks, GATE with an addend)
        const int wt = getenv("HG_WT") ? atoi(getenv("HG_WT")) : 113;     // (113 x 8 = 904 tiles; 112 x 8 = 7 whole rounds)
        const int ldp = wt * 128, Lp = getenv("HG_LP") ? atoi(getenv("HG_LP")) : L / 2;
        float *V[4], *T[2], *H2[2], *actp;
        for (auto& p : V) CK(hipMalloc(&p, (size_t)B * C * ldp * 4));
        for (auto& p : T) CK(hipMalloc(&p, (size_t)B * 2 * C * ldp * 4));
        for (auto& p : H2) CK(hipMalloc(&p, (size_t)B * CC * ldp * 4));
        CK(hipMalloc(&actp, (size_t)B * C * ldp * 4));
        for (auto& p : V) CK(hipMemcpy(p, x, (size_t)B * C * ldp * 4, hipMemcpyDeviceToDevice));
        for (auto& p : H2) CK(hipMemcpy(p, h, (size_t)B * CC * ldp * 4, hipMemcpyDeviceToDevice));
        auto wargs = [&](int layer, int which) {
            GemmArgs a{};
            a.ld = ldp; a.pad = 0; a.L = Lp; a.ntiles = wt; a.batch = B; a.dst_ld = ldp; a.dst_pad = 0; a.bm = 256; a.MB = 4;
            a.A = A + (size_t)layer * 4 * nch * a_tile; a.bias = bias; a.gemm_mode = CTTS_GEMM_F32;
            if (which < 2) {       // T = G . V
                a.nseg = 1; a.nch_total = C / GEMM_KC; a.seg[0] = {V[1 + which], (long long)C * ldp, C / GEMM_KC, 0, 0, 0};
                a.dst0 = T[which]; a.dst0_bstride = (long long)2 * C * ldp; a.M = 2 * C; a.split = 2 * C;
            } else {               // even / odd
                a.nseg = 2; a.nch_total = (C + CC) / GEMM_KC;
                a.seg[0] = {V[which == 2 ? 0 : 3], (long long)C * ldp, C / GEMM_KC, 0, 0, 0};
                a.seg[1] = {H2[which - 2], (long long)CC * ldp, CC / GEMM_KC, 0, 0, 0};
                a.dst0 = actp; a.dst0_bstride = (long long)C * ldp; a.M = 2 * C; a.pairC = C;
                a.addend = T[which - 2]; a.addend_bstride = (long long)2 * C * ldp;
            }
            return a;
        };
        if (getenv("HG_F43")) {
            // Go / no-go for the F(4,3) form of the one-launch layer: today's layer (the fused F(2,3) launch with its 64-column peel
            // + the 3r5w transform stand-in) against the F(4,3) launch + a stand-in of its quad transform (6 planes of C x L / 4),
            // same process, d = 128 and d = 8 alternating, rotating weights, arms alternated HG_ROUNDS times.  First the new
            // kernel's output is compared with f43_reference_kernel on the same packed operands.
            //   HG_WINOGRAD=1 HG_F43=1 [HG_ROUNDS=5]
            const int slots = 4, n1 = C / GEMM_KC, n2 = (C + CC) / GEMM_KC;
            const int Ln = L;
            auto dil = [&](int i) { return (i & 1) ? 8 : 128; };
            auto Lq_of = [&](int d) { return (Ln + 4 * d - 1) / (4 * d) * d; };
            const int qt_max = (Lq_of(128) + 63) / 64, ldq = qt_max * 64;                // 114 tiles of 64 quad columns
            const size_t vplane = (size_t)B * C * ldp, qplane = (size_t)B * C * ldq;
            const size_t slot_f = (size_t)(16 * n1 + 8 * n2) * a_tile;                   // U1..U4 SPLIT, [U0 | C_i], [U5 | C_i] GATE
            if ((size_t)slots * slot_f > (size_t)layers * 4 * nch * a_tile || 2 * Lp > Ln) return 1;
            float *Vb, *Vq, *act2, *bias2;
            unsigned* dmax;
            CK(hipMalloc(&Vb, 4 * vplane * 4)); CK(hipMalloc(&Vq, 6 * qplane * 4)); CK(hipMalloc(&act2, (size_t)B * C * ld * 4));
            CK(hipMalloc(&bias2, 1024 * 4)); CK(hipMalloc(&dmax, 8));
            for (int p = 0; p < 4; ++p) CK(hipMemcpy(Vb + p * vplane, x + p * 1000, vplane * 4, hipMemcpyDeviceToDevice));
            for (int p = 0; p < 6; ++p) CK(hipMemcpy(Vq + p * qplane, x + p * 1000, qplane * 4, hipMemcpyDeviceToDevice));
            CK(hipMemcpy(bias2, x + 4096, 1024 * 4, hipMemcpyDeviceToDevice));
            auto wslot = [&](int i) { return A + (size_t)(i % slots) * slot_f; };
            auto f23_args = [&](int i) {
                const float* w = wslot(i);
                WnWinogradLayerArgs f{};
                f.A_T2 = w; f.A_T3 = w + (size_t)4 * n1 * a_tile; f.A_e = w + (size_t)8 * n1 * a_tile; f.A_o = f.A_e + (size_t)4 * n2 * a_tile;
                f.bias = bias2; f.V = Vb; f.vplane = (long long)vplane; f.h2 = h; f.h_bstride = (long long)CC * ld;
                f.act = act; f.act_bstride = (long long)C * ld; f.C = C; f.H = CC; f.batch = B;
                f.ldp = ldp; f.Lp = Lp; f.ntiles = wt; f.d = dil(i); f.L = 2 * Lp; f.ld = ld; f.pad = PADC; f.in_place = 1;
                return f;
            };
            auto f43_args = [&](int i) {
                const float* w = wslot(i);
                WnWinogradLayerArgs f{};
                f.form = WNWG_F43;
                f.A_T2 = w; f.A_T3 = w + (size_t)4 * n1 * a_tile; f.A_T4 = w + (size_t)8 * n1 * a_tile; f.A_T5 = w + (size_t)12 * n1 * a_tile;
                f.A_e = w + (size_t)16 * n1 * a_tile; f.A_o = f.A_e + (size_t)4 * n2 * a_tile;
                f.bias = bias2; f.V = Vq; f.vplane = (long long)qplane; f.h2 = h; f.h_bstride = (long long)CC * ld;
                f.act = act2; f.act_bstride = (long long)C * ld; f.C = C; f.H = CC; f.batch = B;
                f.d = dil(i); f.L = Ln; f.ld = ld; f.pad = PADC; f.in_place = 1;
                f.ldp = ldq; f.Lp = Lq_of(f.d); f.ntiles = (f.Lp + 63) / 64;
                return f;
            };
            if (getenv("HG_F63")) {
                // Go / no-go for the F(6,3) form of the layers with d % 4 == 0 (profiles/r34_01_winograd_f63_gonogo.txt): today's layer (the quad transform + the F(4,3) launch)
                // against the hex transform + the F(6,3) launch (64 hex columns = 384 natural columns, 352 chunks), the library's own
                // transform kernels on x, d = 128 and d = 8 alternating over three rotating weight slots, arms alternated HG_ROUNDS
                // times.  First the new kernel's output is compared with f63_reference_kernel on the same packed operands.
                //   HG_WINOGRAD=1 HG_F43=1 HG_F63=1 [HG_ROUNDS=5]
                const int hslots = 3;
                const size_t slot_h = (size_t)(24 * n1 + 8 * n2) * a_tile;                // U1..U6 SPLIT, [U0 | C_i], [U7 | C_i] GATE
                if ((size_t)hslots * slot_h > (size_t)layers * 4 * nch * a_tile) return 1;
                auto Lh_of = [&](int d) { return (Ln + 6 * d - 1) / (6 * d) * d; };
                const int ldh = (Lh_of(128) + 63) / 64 * 64;                              // 76 tiles of 64 hex columns
                const size_t hplane = (size_t)B * C * ldh;
                float* Vh;
                CK(hipMalloc(&Vh, 8 * hplane * 4));
                auto a43 = [&](int i) {
                    WnWinogradLayerArgs f = f43_args(i);
                    const float* w = A + (size_t)(i % hslots) * slot_h;
                    f.A_T2 = w; f.A_T3 = w + (size_t)4 * n1 * a_tile; f.A_T4 = w + (size_t)8 * n1 * a_tile; f.A_T5 = w + (size_t)12 * n1 * a_tile;
                    f.A_e = w + (size_t)16 * n1 * a_tile; f.A_o = f.A_e + (size_t)4 * n2 * a_tile;
                    return f;
                };
                auto a63 = [&](int i) {
                    WnWinogradLayerArgs f = a43(i);
                    const float* w = A + (size_t)(i % hslots) * slot_h;
                    f.form = WNWG_F63;
                    f.A_T6 = w + (size_t)16 * n1 * a_tile; f.A_T7 = w + (size_t)20 * n1 * a_tile;
                    f.A_e = w + (size_t)24 * n1 * a_tile; f.A_o = f.A_e + (size_t)4 * n2 * a_tile;
                    f.V = Vh; f.vplane = (long long)hplane;
                    f.ldp = ldh; f.Lp = Lh_of(f.d); f.ntiles = (f.Lp + 63) / 64;
                    return f;
                };
                auto layer = [&](int arm, int i, bool with_transform) {
                    const WnWinogradLayerArgs f = arm ? a63(i) : a43(i);
                    if (with_transform) {
                        const int rc = arm ? launch_winograd_transform_hex(x, (long long)C * ld, Vh, B, C, f.d, Ln, f.Lp, ld, PADC, ldh, f.ntiles * 64, st)
                                           : launch_winograd_transform_quad(x, (long long)C * ld, h, (long long)CC * ld, Vq, nullptr, B, C, CC, f.d, Ln, f.Lp, ld,
                                                                            PADC, ldq, f.ntiles * 64, false, st);
                        if (rc) return rc;
                    }
                    return launch_wn_winograd_layer(f, st);
                };
                unsetenv("CTTS_F32_NO_ROUND_SPLIT"); reload_tuning();
                const size_t n = (size_t)B * C * ld;
                for (int i = 0; i < 2; ++i) {
                    WnWinogradLayerArgs f = a63(i);
                    CK(hipMemsetAsync(act, 0, n * 4, st)); CK(hipMemsetAsync(act2, 0, n * 4, st)); CK(hipMemsetAsync(dmax, 0, 8, st));
                    if (layer(1, i, true)) return 1;
                    f.act = act;
                    hipLaunchKernelGGL(f63_reference_kernel, dim3((unsigned)((f.Lp + 255) / 256), C, B), dim3(256), 0, st, f, act);
                    hipLaunchKernelGGL(max_diff_kernel, dim3(4096), dim3(256), 0, st, act, act2, n, dmax);
                    unsigned hd[2];
                    CK(hipMemcpyAsync(hd, dmax, 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                    float fd[2]; memcpy(fd, hd, 8);
                    printf("d = %3d, Lh = %d, %d tiles x %d: max |F(6,3) launch - reference| = %.3e, max |reference| = %.3e\n", f.d, f.Lp, f.ntiles, B, fd[0], fd[1]);
                    // (the interior sums enter with multipliers up to 32: fmaf chain against MFMA order at |32 e| ~ 10)
                    if (!(fd[0] <= 1e-4f) || !(fd[1] > 0.01f)) { printf("MISMATCH\n"); return 2; }
                }
                const int rounds = getenv("HG_ROUNDS") ? atoi(getenv("HG_ROUNDS")) : 5, reps = 12;
                float lo[2][2], hi[2][2], sum[2][2];
                for (int arm = 0; arm < 2; ++arm) for (int w = 0; w < 2; ++w) { lo[arm][w] = 1e9f; hi[arm][w] = 0.f; sum[arm][w] = 0.f; }
                static const char* names[2] = {"F(4,3) one launch", "F(6,3) one launch"};
                for (int r = 0; r < rounds; ++r)
                    for (int arm = 0; arm < 2; ++arm)
                        for (int w = 0; w < 2; ++w) {
                            for (int i = 0; i < 4; ++i) if (layer(arm, i, w)) return 1;
                            CK(hipStreamSynchronize(st));
                            CK(hipEventRecord(e0, st));
                            for (int i = 0; i < reps; ++i) if (layer(arm, i, w)) return 1;
                            CK(hipEventRecord(e1, st));
                            CK(hipStreamSynchronize(st));
                            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                            ms /= reps;
                            printf("round %d  %-20s %-22s %.4f ms per layer\n", r, names[arm], w ? "+ its transform" : "launches alone", ms);
                            lo[arm][w] = ms < lo[arm][w] ? ms : lo[arm][w]; hi[arm][w] = ms > hi[arm][w] ? ms : hi[arm][w]; sum[arm][w] += ms;
                        }
                for (int w = 0; w < 2; ++w) {
                    const float s0 = hi[0][w] - lo[0][w], s1 = hi[1][w] - lo[1][w], spread = s0 > s1 ? s0 : s1;
                    const float gain = (sum[0][w] - sum[1][w]) / rounds;
                    printf("%s: F(4,3) %.4f ms (%.4f-%.4f), F(6,3) %.4f ms (%.4f-%.4f): gain %.4f ms = %.1f x the larger spread%s\n",
                           w ? "per layer with its transform" : "layer launches alone", sum[0][w] / rounds, lo[0][w], hi[0][w], sum[1][w] / rounds,
                           lo[1][w], hi[1][w], gain, gain / (spread > 0.f ? spread : 1e-9f), w ? (gain > 10.f * spread ? "  -> GO" : "  -> NO-GO") : "");
                }
                return 0;
            }
            if (getenv("HG_F43_WIDE")) {
                // Go / no-go for the shapes of the F(4,3) layer (profiles/r26_01_f43_wide_gonogo.txt): the parent's kernel (64 quad columns,
                // one chunk per stage, chunk table read by a plain load) against the same shape with the table fetched ahead, with
                // two chunks per stage, and the 128-quad-column one-workgroup-per-CU shape with one and with two chunks per stage (with
                // their round-aligned peel).  Every arm is first compared with f43_reference_kernel and bit for bit with the parent's.
                //   HG_WINOGRAD=1 HG_F43=1 HG_F43_WIDE=1 [HG_ROUNDS=5]
                constexpr int NA = 5;
                static const char* an[NA] = {"64 col, KD 1, plain table (parent)", "64 col, KD 1, table ahead", "64 col, KD 2", "128 col, KD 1 + peel", "128 col, KD 2 + peel"};
                unsetenv("CTTS_F32_NO_ROUND_SPLIT"); reload_tuning();
                auto run_arm = [&](int arm, WnWinogradLayerArgs f) {
                    f.b0 = 0; f.col0 = 0;
                    switch (arm) {
                        case 0: return launch_wnwg_shape<1, 1, 1, 0>(f, f.ntiles, (long long)f.ntiles * f.batch, st);
                        case 1: return launch_wnwg_f43<1, 1>(f, true, false, false, st);
                        case 2: return launch_wnwg_f43<2, 1>(f, true, false, false, st);
                        case 3: return launch_wnwg_f43<1, 1>(f, false, false, false, st);
                        default: return launch_wnwg_f43<1, 2>(f, false, false, false, st);
                    }
                };
                float* act3;
                CK(hipMalloc(&act3, (size_t)B * C * ld * 4));
                const size_t n = (size_t)B * C * ld;
                for (int i = 0; i < 2; ++i) {
                    WnWinogradLayerArgs f = f43_args(i);
                    CK(hipMemsetAsync(act, 0, n * 4, st));
                    f.act = act3; CK(hipMemsetAsync(act3, 0, n * 4, st));
                    if (run_arm(0, f)) return 1;
                    hipLaunchKernelGGL(f43_reference_kernel, dim3((unsigned)((f.Lp + 255) / 256), C, B), dim3(256), 0, st, f43_args(i), act);
                    for (int arm = 0; arm < NA; ++arm) {
                        f.act = act2; CK(hipMemsetAsync(act2, 0, n * 4, st)); CK(hipMemsetAsync(dmax, 0, 8, st));
                        if (run_arm(arm, f)) return 1;
                        unsigned hd[2], hb[2];
                        hipLaunchKernelGGL(max_diff_kernel, dim3(4096), dim3(256), 0, st, act, act2, n, dmax);
                        CK(hipMemcpyAsync(hd, dmax, 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                        CK(hipMemsetAsync(dmax, 0, 8, st));
                        hipLaunchKernelGGL(max_diff_kernel, dim3(4096), dim3(256), 0, st, act3, act2, n, dmax);
                        CK(hipMemcpyAsync(hb, dmax, 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                        float fd[2], fb[2]; memcpy(fd, hd, 8); memcpy(fb, hb, 8);
                        printf("d = %3d  %-36s max |arm - reference| = %.3e (max |reference| %.3e), max |arm - parent's| = %.1e, width %d\n", f.d, an[arm], fd[0],
                               fd[1], fb[0], arm >= 3 ? 128 : 64);
                        if (!(fd[0] <= 2e-5f) || !(fd[1] > 0.01f) || fb[0] != 0.f) { printf("MISMATCH\n"); return 2; }
                    }
                }
                const int rounds = getenv("HG_ROUNDS") ? atoi(getenv("HG_ROUNDS")) : 5, reps = 12;
                float lo[NA], hi[NA], sum[NA];
                for (int arm = 0; arm < NA; ++arm) { lo[arm] = 1e9f; hi[arm] = 0.f; sum[arm] = 0.f; }
                for (int r = 0; r < rounds; ++r)
                    for (int arm = 0; arm < NA; ++arm) {
                        for (int i = 0; i < 4; ++i) if (run_arm(arm, f43_args(i))) return 1;
                        CK(hipStreamSynchronize(st));
                        CK(hipEventRecord(e0, st));
                        for (int i = 0; i < reps; ++i) if (run_arm(arm, f43_args(i))) return 1;
                        CK(hipEventRecord(e1, st));
                        CK(hipStreamSynchronize(st));
                        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                        ms /= reps;
                        printf("round %d  %-36s %.4f ms per layer\n", r, an[arm], ms);
                        lo[arm] = ms < lo[arm] ? ms : lo[arm]; hi[arm] = ms > hi[arm] ? ms : hi[arm]; sum[arm] += ms;
                    }
                for (int arm = 1; arm < NA; ++arm) {
                    const float s0 = hi[0] - lo[0], s1 = hi[arm] - lo[arm], spread = s0 > s1 ? s0 : s1;
                    const float gain = (sum[0] - sum[arm]) / rounds;
                    printf("%-36s %.4f ms (%.4f-%.4f) against the parent's %.4f ms (%.4f-%.4f): gain %.4f ms = %.1f x the larger spread%s\n", an[arm],
                           sum[arm] / rounds, lo[arm], hi[arm], sum[0] / rounds, lo[0], hi[0], gain, gain / (spread > 0.f ? spread : 1e-9f),
                           gain > 10.f * spread && gain >= 0.18f ? "  -> GO" : "  -> NO-GO");
                }
                return 0;
            }
            for (int i = 0; i < 2; ++i) {
                WnWinogradLayerArgs f = f43_args(i);
                CK(hipMemsetAsync(act, 0, (size_t)B * C * ld * 4, st)); CK(hipMemsetAsync(act2, 0, (size_t)B * C * ld * 4, st));
                CK(hipMemsetAsync(dmax, 0, 8, st));
                if (launch_wn_winograd_layer(f, st)) return 1;
                hipLaunchKernelGGL(f43_reference_kernel, dim3((unsigned)((f.Lp + 255) / 256), C, B), dim3(256), 0, st, f, act);
                const size_t n = (size_t)B * C * ld;
                hipLaunchKernelGGL(max_diff_kernel, dim3(4096), dim3(256), 0, st, act, act2, n, dmax);
                unsigned hd[2];
                CK(hipMemcpyAsync(hd, dmax, 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                float fd[2]; memcpy(fd, hd, 8);
                printf("d = %3d, Lq = %d, %d tiles x %d: max |F(4,3) launch - reference| = %.3e, max |reference| = %.3e\n", f.d, f.Lp, f.ntiles, B, fd[0], fd[1]);
                if (!(fd[0] <= 2e-5f) || !(fd[1] > 0.01f)) { printf("MISMATCH\n"); return 2; }
            }
            const size_t sn23 = vplane / 4, sn43 = qplane / 4;                 // 16-byte units of one V plane of either form
            float4 *ssrc, *sdst;
            const size_t sbytes = (5 * sn23 > 6 * sn43 ? 5 * sn23 : 6 * sn43) * 16;
            CK(hipMalloc(&ssrc, sbytes)); CK(hipMalloc(&sdst, sbytes)); CK(hipMemset(ssrc, 0, sbytes));
            unsetenv("CTTS_F32_NO_ROUND_SPLIT"); reload_tuning();              // today's arm with its peel, as the library runs it
            auto layer = [&](int arm, int i, bool with_transform) {
                if (with_transform) {
                    if (arm) hipLaunchKernelGGL(stream_6r6w_kernel, dim3((unsigned)((sn43 + 255) / 256)), dim3(256), 0, st, ssrc, sdst, sn43);
                    else hipLaunchKernelGGL(stream_3r5w_kernel, dim3((unsigned)((sn23 + 255) / 256)), dim3(256), 0, st, ssrc, sdst, sn23);
                }
                return launch_wn_winograd_layer(arm ? f43_args(i) : f23_args(i), st);
            };
            const int rounds = getenv("HG_ROUNDS") ? atoi(getenv("HG_ROUNDS")) : 5, reps = 12;
            // [arm][0 = the layer launches alone, 1 = with the transform stand-in: what a layer costs]
            float lo[2][2], hi[2][2], sum[2][2];
            for (int arm = 0; arm < 2; ++arm) for (int w = 0; w < 2; ++w) { lo[arm][w] = 1e9f; hi[arm][w] = 0.f; sum[arm][w] = 0.f; }
            static const char* names[2] = {"F(2,3) fused + peel", "F(4,3) one launch"};
            for (int r = 0; r < rounds; ++r)
                for (int arm = 0; arm < 2; ++arm)
                    for (int w = 0; w < 2; ++w) {
                        for (int i = 0; i < 4; ++i) if (layer(arm, i, w)) return 1;
                        CK(hipStreamSynchronize(st));
                        CK(hipEventRecord(e0, st));
                        for (int i = 0; i < reps; ++i) if (layer(arm, i, w)) return 1;
                        CK(hipEventRecord(e1, st));
                        CK(hipStreamSynchronize(st));
                        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                        ms /= reps;
                        printf("round %d  %-20s %-22s %.4f ms per layer\n", r, names[arm], w ? "+ transform stand-in" : "launches alone", ms);
                        lo[arm][w] = ms < lo[arm][w] ? ms : lo[arm][w]; hi[arm][w] = ms > hi[arm][w] ? ms : hi[arm][w]; sum[arm][w] += ms;
                    }
            for (int w = 0; w < 2; ++w) {
                const float s0 = hi[0][w] - lo[0][w], s1 = hi[1][w] - lo[1][w], spread = s0 > s1 ? s0 : s1;
                const float gain = (sum[0][w] - sum[1][w]) / rounds;
                printf("%s: F(2,3) %.4f ms (%.4f-%.4f), F(4,3) %.4f ms (%.4f-%.4f): gain %.4f ms = %.1f x the larger spread%s\n",
                       w ? "per layer with the transform stand-in" : "layer launches alone", sum[0][w] / rounds, lo[0][w], hi[0][w], sum[1][w] / rounds,
                       lo[1][w], hi[1][w], gain, gain / (spread > 0.f ? spread : 1e-9f), w ? (gain > 10.f * spread ? "  -> GO" : "  -> NO-GO") : "");
            }
            return 0;
        }
        if (getenv("HG_FUSED")) {
            // The one-launch Winograd layer (wn_winograd_layer.hip) against the two launches it replaces - T2 | T3 and even | odd as
            // the lean form issues them (two parts each, T planes in HBM, second addend, mapped store, cond rows in place) - on the
            // same operands, in this process, alternated HG_ROUNDS times; first the two forms' outputs are compared.
            //   HG_WINOGRAD=1 HG_FUSED=1 [HG_WT=112 HG_LP=14336]  (whole rounds; the default 113 / 14 400 has the 64-workgroup tail;
            //   HG_PEEL=1 lets the fused launcher peel it, the conv-GEMM's peel needs the small shape, which is not linked in here)
            const int slots = 5, n1 = C / GEMM_KC, n2 = (C + CC) / GEMM_KC;
            const int Ln = 2 * Lp;                               // natural columns (ld holds them: Lp <= L / 2)
            const size_t vplane = (size_t)B * C * ldp, tplane = (size_t)B * 2 * C * ldp;
            const size_t slot_f = (size_t)4 * (2 * n1 + 2 * n2) * a_tile;
            float *Vb, *Tb, *act2, *bias2;
            unsigned* dmax;
            CK(hipMalloc(&Vb, 4 * vplane * 4)); CK(hipMalloc(&Tb, 2 * tplane * 4)); CK(hipMalloc(&act2, (size_t)B * C * ld * 4));
            CK(hipMalloc(&bias2, 1024 * 4)); CK(hipMalloc(&dmax, 8));
            for (int p = 0; p < 4; ++p) CK(hipMemcpy(Vb + p * vplane, x + p * 1000, vplane * 4, hipMemcpyDeviceToDevice));
            CK(hipMemcpy(bias2, x + 4096, 1024 * 4, hipMemcpyDeviceToDevice));
            if ((size_t)slots * slot_f > (size_t)layers * 4 * nch * a_tile) return 1;
            auto wslot = [&](int i) { return A + (size_t)(i % slots) * slot_f; };
            auto dil = [&](int i) { return 8 << (i % slots); };                    // d = 8 .. 128: cond rows in place
            auto lean = [&](int i) {
                const float* w = wslot(i);
                GemmArgs a{};
                a.gemm_mode = CTTS_GEMM_F32; a.bm = 256;
                a.ld = ldp; a.pad = 0; a.L = Lp; a.ntiles = wt; a.batch = B; a.MB = 4;
                a.bias = bias; a.nseg = 1; a.nch_total = n1;
                a.dst_ld = ldp; a.dst_pad = 0; a.dst0_bstride = (long long)2 * C * ldp; a.M = 2 * C; a.split = 2 * C;
                a.parts = 2; a.part_A = (long long)4 * n1 * a_tile; a.part_seg[0] = (long long)vplane; a.part_dst0 = (long long)tplane;
                a.A = w; a.seg[0] = {Vb + vplane, (long long)C * ldp, n1, 0, 0, 0}; a.dst0 = Tb;
                if (int rc = launch_gemm_f32(GEMM_EPI_SPLIT, a, st)) return rc;
                a.bias = bias2; a.nseg = 2; a.nch_total = n2; a.split = 0; a.pairC = C;
                a.dst0 = act; a.dst0_bstride = (long long)C * ld; a.dst_ld = ld; a.dst_pad = PADC;
                a.addend = Tb; a.addend2 = Tb + tplane; a.addend_bstride = (long long)2 * C * ldp; a.addend2_sign = 1.0f;
                a.map_d = dil(i); a.map_L = Ln; a.map_par = 0;
                a.part_A = (long long)4 * n2 * a_tile; a.part_seg[0] = (long long)(3 * vplane); a.part_seg[1] = 0; a.part_dst0 = 0;
                a.mseg = 2; a.mseg_ld = ld; a.mseg_pad = PADC;
                a.A = w + (size_t)8 * n1 * a_tile;
                a.seg[0] = {Vb, (long long)C * ldp, n1, 0, 0, 0};
                a.seg[1] = {h, (long long)CC * ld, CC / GEMM_KC, 0, 0, 0};
                return launch_gemm_f32(GEMM_EPI_GATE, a, st);
            };
            auto fused = [&](int i, float* dst) {
                const float* w = wslot(i);
                WnWinogradLayerArgs f{};
                f.A_T2 = w; f.A_T3 = w + (size_t)4 * n1 * a_tile; f.A_e = w + (size_t)8 * n1 * a_tile; f.A_o = f.A_e + (size_t)4 * n2 * a_tile;
                f.bias = bias2; f.V = Vb; f.vplane = (long long)vplane; f.h2 = h; f.h_bstride = (long long)CC * ld;
                f.act = dst; f.act_bstride = (long long)C * ld; f.C = C; f.H = CC; f.batch = B;
                f.ldp = ldp; f.Lp = Lp; f.ntiles = wt; f.d = dil(i); f.L = Ln; f.ld = ld; f.pad = PADC; f.in_place = 1;
                return launch_wn_winograd_layer(f, st);
            };
            for (int i = 0; i < slots; ++i) {                    // the same bits up to the re-ordered sum
                CK(hipMemsetAsync(act, 0, (size_t)B * C * ld * 4, st)); CK(hipMemsetAsync(act2, 0, (size_t)B * C * ld * 4, st));
                CK(hipMemsetAsync(dmax, 0, 8, st));
                setenv("CTTS_F32_NO_ROUND_SPLIT", "1", 1); reload_tuning();
                if (lean(i)) return 1;
                if (getenv("HG_PEEL")) { unsetenv("CTTS_F32_NO_ROUND_SPLIT"); reload_tuning(); }
                if (fused(i, act2)) return 1;
                const size_t n = (size_t)B * C * ld;
                hipLaunchKernelGGL(max_diff_kernel, dim3(4096), dim3(256), 0, st, act, act2, n, dmax);
                unsigned hd[2];
                CK(hipMemcpyAsync(hd, dmax, 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                float fd[2]; memcpy(fd, hd, 8);
                printf("d = %3d: max |fused - lean| = %.3e, max |lean| = %.3e\n", dil(i), fd[0], fd[1]);
                if (!(fd[0] <= 2e-5f) || !(fd[1] > 0.01f)) { printf("MISMATCH\n"); return 2; }
            }
            const int rounds = getenv("HG_ROUNDS") ? atoi(getenv("HG_ROUNDS")) : 5, reps = 12;
            float lo[2] = {1e9f, 1e9f}, hi[2] = {0.f, 0.f}, sum[2] = {0.f, 0.f};
            for (int r = 0; r < rounds; ++r)
                for (int arm = 0; arm < 2; ++arm) {
                    if (arm == 0 || !getenv("HG_PEEL")) setenv("CTTS_F32_NO_ROUND_SPLIT", "1", 1);
                    else unsetenv("CTTS_F32_NO_ROUND_SPLIT");
                    reload_tuning();
                    for (int i = 0; i < 3; ++i) if (arm ? fused(i, act2) : lean(i)) return 1;
                    CK(hipStreamSynchronize(st));
                    CK(hipEventRecord(e0, st));
                    for (int i = 0; i < reps; ++i) if (arm ? fused(i, act2) : lean(i)) return 1;
                    CK(hipEventRecord(e1, st));
                    CK(hipStreamSynchronize(st));
                    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                    ms /= reps;
                    printf("round %d  %-28s %.4f ms per layer\n", r, arm ? "fused (one launch)" : "T2 | T3 + even | odd", ms);
                    lo[arm] = ms < lo[arm] ? ms : lo[arm]; hi[arm] = ms > hi[arm] ? ms : hi[arm]; sum[arm] += ms;
                }
            const float spread = (hi[0] - lo[0]) > (hi[1] - lo[1]) ? hi[0] - lo[0] : hi[1] - lo[1];
            printf("%d tiles x %d, Lp = %d%s: two launches %.4f ms (spread %.4f), fused %.4f ms (spread %.4f): gain %.4f ms = %.1f x the larger spread\n",
                   wt, B, Lp, getenv("HG_PEEL") ? ", fused tail peeled" : "", sum[0] / rounds, hi[0] - lo[0], sum[1] / rounds, hi[1] - lo[1],
                   (sum[0] - sum[1]) / rounds, (sum[0] - sum[1]) / rounds / (spread > 0.f ? spread : 1e-9f));
            return 0;
        }
        const size_t sn = (size_t)B * C * ldp / 4;             // 16-byte units of one V plane: 3 read (0.71 GB), 5 written (1.18 GB)
        float4 *ssrc, *sdst;
        CK(hipMalloc(&ssrc, 3 * sn * 16)); CK(hipMalloc(&sdst, 5 * sn * 16)); CK(hipMemset(ssrc, 0, 3 * sn * 16));
        const int reps = 24;
        float sum = 0.f;
        for (int which = 0; which < 5; ++which) {
            auto go = [&](int i) {
                if (which == 4) { hipLaunchKernelGGL(stream_3r5w_kernel, dim3((unsigned)((sn + 255) / 256)), dim3(256), 0, st, ssrc, sdst, sn); return 0; }
                return launch_gemm_f32(which < 2 ? GEMM_EPI_SPLIT : GEMM_EPI_GATE, wargs(i % layers, which), st);
            };
            for (int i = 0; i < 4; ++i) if (go(i)) return 1;
            CK(hipStreamSynchronize(st));
            CK(hipEventRecord(e0, st));
            for (int i = 0; i < reps; ++i) if (go(i)) return 1;
            CK(hipEventRecord(e1, st));
            CK(hipStreamSynchronize(st));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            ms /= reps;
            sum += ms;
            static const char* names[5] = {"T2 = G2.V2  SPLIT K=32ch", "T3 = G3.V3  SPLIT K=32ch", "even GATE+addend K=48ch", "odd  GATE+addend K=48ch", "transform stand-in 3r5w"};
            if (which < 4) {
                const double flop = 2.0 * 1024 * (which < 2 ? C : C + CC) * (double)B * Lp;
                printf("%-26s %d tiles x 4 = %.3f rounds  %.4f ms  %.4f of 157.3\n", names[which], wt * B, 4.0 * wt * B / 512.0, ms, flop / (ms * 1e-3) / 157.3e12);
            } else {
                printf("%-26s %.2f GB read %.2f GB written  %.4f ms  %.2f TB/s\n", names[which], 3 * sn * 16e-9, 5 * sn * 16e-9, ms, 8 * sn * 16e-12 / (ms * 1e-3));
            }
        }
        printf("sum of the five: %.4f ms per layer\n", sum);
        return 0;
    }
    for (int i = 0; i < 4; ++i) if (launch_gemm_f32(GEMM_EPI_GATE, args(i % layers), st)) return 1;
    CK(hipStreamSynchronize(st));
    const int reps = 24;
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < reps; ++i) if (launch_gemm_f32(GEMM_EPI_GATE, args(i % layers), st)) return 1;
    CK(hipEventRecord(e1, st));
    CK(hipStreamSynchronize(st));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    const double flop = 2.0 * 1024 * (double)(nch * GEMM_KC) * (double)B * L;
    printf("L = %d: %d workgroups = %.3f rounds of 512;  ", L, 4 * (L / 128) * B, 4.0 * (L / 128) * B / 512.0);
    printf("%-34s %.4f ms per launch  %.1f TFLOP/s  %.4f of 157.3\n", label, ms / reps, flop / (ms / reps * 1e-3) / 1e12, flop / (ms / reps * 1e-3) / 157.3e12);
    return 0;
}
