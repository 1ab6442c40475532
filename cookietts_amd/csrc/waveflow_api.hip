// WaveFlow (ax core, waveflow=True) on the fp32 MFMA conv-GEMM.
//
// The height axis (n_group rows) is autoregressive (efficient_modules.py:42-65): row r+1 of a flow
// needs the WN_2d output for row r, so a flow is n_group-1 sequential row passes, each n_layers x
// {in-layer GEMM + gate, res/skip GEMM}.  The (k_h, k_w) Conv2d with dilation (d_h, 2^i) and no
// height padding (glow_ax.py:518-523) is a GEMM whose K axis is [height tap][width tap][channel]:
// height taps read earlier rows' layer inputs from a ring of k_h slots per layer (the reference's
// audio_queues, glow_ax.py:597-602), width taps are column shifts in the padded layout.  Rows
// 0..k_h-2 simply skip the leading (all-zero) height taps via the A-chunk window - no queue
// zero-fill.  Conditioning: interp(Wc*mel + bc) == Wc*interp(mel) + bc (linear interpolation
// commutes with the 1x1 conv), so mel is interpolated ONCE to L steps and the cond layer becomes
// extra K of every in-layer GEMM (the [B, 2*C*n_layers, L] tensor is never materialised).
// PermuteHeight (efficient_modules.py:360-403) is folded into a logical->physical row map.
#include <cstdlib>
#include <algorithm>
#include <vector>

#include "gemm_f32.h"
#include "tuning.h"
#include "waveglow_kernels.h"
#include "waveflow_sep.h"
#include "waveflow_tail.h"

namespace ctts {
namespace {

constexpr size_t ALIGN_F = 64;
inline size_t align_up(size_t v) { return (v + ALIGN_F - 1) / ALIGN_F * ALIGN_F; }
constexpr int WF_BM = 128;

struct WfPlan {
    ctts_waveflow_config c;
    int C, kmel, nch_in, nch_c;      // nch_c = chunks per (tap) segment
    bool sep, precond;               // separable in-layers; conditioning handed over per flow at frame rate
    int taps;                        // GEMM taps: kh*kw, or 1 behind the depthwise stage
    std::vector<int> n_rem;          // active latent rows per flow (early outputs, ax:170-189)
    struct Flow {
        size_t start_w, start_b, end_w, end_b, winv;
        std::vector<size_t> in_A, in_b, rs_A, rs_b, rs_T, rs_Tb, dw_w, dw_b, sA1, sb1, sA2, sb2;
    };
    std::vector<Flow> fl;
    size_t total;
    int ring;                        // ring slots per layer: (kh - 1) * max height dilation + 1 rows of history
    int dh(int i) const { return c.dilation_h_l[i] > 0 ? c.dilation_h_l[i] : c.dilation_h; }
    int dw(int i) const { return c.dilation_w[i] > 0 ? c.dilation_w[i] : 1 << i; }
    // merge_res_skip (glow_ax.py:612-626): no residual into `audio`, so every layer's queue holds the `start` outputs - layer i
    // reads the ring of layer 0 (src), nothing is written to ring i + 1, and all rows of the res/skip GEMM are skip rows (last)
    int src(int i) const { return c.merge_res_skip ? 0 : i; }
    bool last(int i) const { return i == c.n_layers - 1 || c.merge_res_skip; }
    // height tap ah of WN row r reads row r - (kh - 1 - ah) * dh: rows above the first do not exist, taps below a_min are skipped
    int a_min(int r, int i) const { return std::max(0, c.kernel_size_h - 1 - r / dh(i)); }
    int rs_rows(int i) const { return (i < c.n_layers - 1 && !c.merge_res_skip) ? 2 * C : C; }
    int rs_mb(int i) const { return (rs_rows(i) + WF_BM - 1) / WF_BM; }
    int in_mb() const { return (C + 63) / 64; }
    // one 128-row block holds every gate pair: the res/skip GEMM runs inside the in-layer kernel (GEMM_EPI_GATE_RS)
    bool fused() const { return C == 64 && c.gated_unit == 0; }
    // the analysis direction's all-rows form (one launch per layer over every row): the fused dense layer on the fp32 MFMA tile
    bool all_rows() const { return fused() && !sep && !gemm_mode_is_split(c.f32_gemm_mode); }
    // both 1x1 stages of a separable layer in one launch (waveflow_sep.hip): pointwise/gate + res/skip, C = 128
    bool sep_fused() const { return sep && precond && wf_sep_supported(C); }
};

int make_wf_plan(const ctts_waveflow_config* cfg, WfPlan& p) {
    CTTS_CHECK_ARG(cfg != nullptr, "waveflow config is NULL");
    p.c = *cfg;
    const auto& c = p.c;
    CTTS_CHECK_ARG(c.n_flows >= 1 && c.n_layers >= 1 && c.n_layers <= 12, "n_flows=%d n_layers=%d", c.n_flows, c.n_layers);
    CTTS_CHECK_ARG(gemm_mode_valid(c.f32_gemm_mode), "f32_gemm_mode=%d (CTTS_GEMM_DEFAULT / _F32 / _BF16X3 / _BF16X6)", c.f32_gemm_mode);
    CTTS_CHECK_ARG(c.n_group >= 2 && c.n_group <= 64, "n_group=%d", c.n_group);
    CTTS_CHECK_ARG(c.n_channels >= 64 && c.n_channels % 64 == 0, "n_channels=%d (multiple of 64)", c.n_channels);
    CTTS_CHECK_ARG(c.kernel_size_w % 2 == 1 && c.kernel_size_w >= 1 && c.kernel_size_h >= 1, "kernel %dx%d",
                   c.kernel_size_h, c.kernel_size_w);
    CTTS_CHECK_ARG(c.dilation_h >= 1, "dilation_h=%d", c.dilation_h);
    p.ring = 1;
    for (int i = 0; i < c.n_layers; ++i) {
        CTTS_CHECK_ARG(c.dilation_h_l[i] >= 0 && c.dilation_w[i] >= 0, "negative dilation (layer %d)", i);
        p.ring = std::max(p.ring, (c.kernel_size_h - 1) * p.dh(i) + 1);
    }
    CTTS_CHECK_ARG(c.gated_unit >= 0 && c.gated_unit < GATE_KINDS && (c.merge_res_skip == 0 || c.merge_res_skip == 1),
                   "gated_unit=%d merge_res_skip=%d", c.gated_unit, c.merge_res_skip);
    CTTS_CHECK_ARG((c.mixing == CTTS_MIX_PERMUTE || c.mixing == CTTS_MIX_CONV1X1) && (c.mix_first == 0 || c.mix_first == 1) &&
                   c.n_early_every >= 0 && c.n_early_size >= 0, "mixing=%d mix_first=%d early %d/%d", c.mixing, c.mix_first,
                   c.n_early_every, c.n_early_size);
    CTTS_CHECK_ARG(c.mixing != CTTS_MIX_PERMUTE || c.n_flows % 2 == 0 || c.n_flows == 1, "PermuteHeight requires even n_flows");
    {
        int n_rem = c.n_group;
        p.n_rem.clear();
        for (int k = 0; k < c.n_flows; ++k) {
            if (c.n_early_every > 0 && k % c.n_early_every == 0 && k > 0) n_rem -= c.n_early_size;
            CTTS_CHECK_ARG(n_rem >= 2, "flow %d has %d remaining rows (increase n_group or decrease n_early_every/n_early_size)", k, n_rem);
            p.n_rem.push_back(n_rem);
        }
    }
    p.sep = c.seperable_conv != 0 && !(c.kernel_size_h == 1 && c.kernel_size_w == 1);   // glow_ax.py:521
    p.precond = c.cond_precomputed != 0;
    p.taps = p.sep ? 1 : c.kernel_size_h * c.kernel_size_w;
    CTTS_CHECK_ARG(p.taps + 1 <= GEMM_MAX_SEG, "dense kernel %dx%d needs more than %d segments (use seperable_conv)",
                   c.kernel_size_h, c.kernel_size_w, GEMM_MAX_SEG);
    CTTS_CHECK_ARG(c.kernel_size_h <= WF_MAX_KH, "kernel_size_h=%d (<= %d)", c.kernel_size_h, WF_MAX_KH);
    CTTS_CHECK_ARG(p.precond || c.n_mel_channels >= 1, "n_mel_channels=%d", c.n_mel_channels);
    p.C = c.n_channels;
    p.kmel = p.precond ? 0 : round_up(c.n_mel_channels, GEMM_KC);
    p.nch_c = p.C / GEMM_KC;
    p.nch_in = p.taps * p.nch_c + p.kmel / GEMM_KC;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n); return r; };
    p.fl.resize(c.n_flows);
    for (int k = 0; k < c.n_flows; ++k) {
        auto& f = p.fl[k];
        f.start_w = take(p.C); f.start_b = take(p.C);
        f.end_w = take(2 * p.C); f.end_b = take(2);
        f.winv = take(c.mixing == CTTS_MIX_CONV1X1 ? (size_t)p.n_rem[k] * p.n_rem[k] : 0);
        for (int i = 0; i < c.n_layers; ++i) {
            f.in_A.push_back(take((size_t)p.in_mb() * p.nch_in * GEMM_KC * WF_BM));
            f.in_b.push_back(take((size_t)p.in_mb() * WF_BM));
            f.rs_A.push_back(take((size_t)p.rs_mb(i) * p.nch_c * GEMM_KC * WF_BM));
            f.rs_b.push_back(take((size_t)p.rs_mb(i) * WF_BM));
            f.rs_T.push_back(take(p.fused() ? 64 * 128 : 0));
            f.rs_Tb.push_back(take(p.fused() ? 128 : 0));
            f.dw_w.push_back(take(p.sep ? (size_t)p.C * c.kernel_size_h * c.kernel_size_w : 0));
            f.dw_b.push_back(take(p.sep ? p.C : 0));
            f.sA1.push_back(take(p.sep_fused() ? 128 * 256 : 0));
            f.sb1.push_back(take(p.sep_fused() ? 256 : 0));
            f.sA2.push_back(take(p.sep_fused() ? 128 * 256 : 0));
            f.sb2.push_back(take(p.sep_fused() ? 256 : 0));
        }
    }
    p.total = o;
    return CTTS_OK;
}

// res/skip weight [rows][64] -> transposed, row-padded [64][128] (+ bias [128]) for the fused epilogue
__global__ void wf_pack_rs_t_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ wT,
                                    float* __restrict__ bT, int rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 64 * 128) {
        const int ch = i >> 7, row = i & 127;
        wT[i] = row < rows ? w[row * 64 + ch] : 0.0f;
    } else if (i < 64 * 128 + 128) {
        const int row = i - 64 * 128;
        bT[row] = row < rows ? b[row] : 0.0f;
    }
}

struct WfGeom { int L, Lr, ld, pad, ntiles; };   // Lr: row stride of the dense `rows` buffer (16-byte rows)

int make_wf_geom(const WfPlan& p, int samples, WfGeom& g) {
    CTTS_CHECK_ARG(samples >= p.c.n_group && samples % p.c.n_group == 0, "samples=%d not a multiple of n_group=%d",
                   samples, p.c.n_group);
    g.L = samples / p.c.n_group;
    g.Lr = round_up(g.L, 4);
    int maxshift = 0;
    for (int i = 0; i < p.c.n_layers; ++i) maxshift = std::max(maxshift, (p.c.kernel_size_w / 2) * p.dw(i));
    g.pad = round_up(maxshift > 128 ? maxshift : 128, 32);
    const int bn = gemm_bn(WF_BM);
    g.ntiles = (g.L + bn - 1) / bn;
    g.ld = g.ntiles * bn + 2 * g.pad;
    return CTTS_OK;
}

// Row queue (wf_row_persistent_kernel): control words + the layer descriptors of one flow, inside the caller's workspace
struct WfQueueWs {
    unsigned int *abort_word, *counters, *flags;     // [1] | [n_flows * n_group] | [n_group * (n_layers + 1) stages][batch][tiles of 64 columns]
    unsigned int* status;                            // sticky: WF_ABORT_MAGIC once a call on this workspace aborted, until it is reported
    GemmArgs* layers;                                // [n_group][n_layers] of the flow being run
    WfTailDesc* tails;                               // [n_group]
    size_t control_bytes;                            // abort word .. end of the flags: zeroed at the start of every call
};
// Analysis direction (ctts_waveflow_forward_*), behind the inverse's buffers: log_s of one flow, the fp64 partial sums, and - for
// WfPlan::all_rows() models - full-height storage [n_group - 1][B][C][ld] of two layer inputs and the skip sum + the layer descriptors
struct WfFwdWs { float *ls, *XA, *XB, *OUT; double* partials; GemmArgs* desc; int nblk; };
struct WfWs { float *rows, *mel_up, *cond_up, *dwout, *X, *act, *out; size_t total, xslot, cond_slot; WfQueueWs q; WfFwdWs f; };

void wf_carve(const WfPlan& p, const WfGeom& g, int batch, float* base, WfWs& w, bool forward = false) {
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n); return base ? base + r : nullptr; };
    const size_t B = batch;
    w.rows = take(B * p.c.n_group * g.Lr);
    w.mel_up = take(B * p.kmel * g.ld);
    w.cond_slot = align_up(B * 2 * p.C * g.ld);              // upsampled conditioning of one layer
    w.cond_up = take(p.precond ? w.cond_slot * p.c.n_layers : 0);
    w.dwout = take(p.sep ? B * p.C * g.ld : 0);
    w.xslot = align_up(B * p.C * g.ld);
    w.X = take(w.xslot * p.c.n_layers * p.ring);
    w.act = take(B * p.C * g.ld);
    w.out = take(B * p.C * g.ld);
    {
        const size_t n_count = (size_t)p.c.n_flows * p.c.n_group, n_flags = (size_t)p.c.n_group * (p.c.n_layers + 1) * B * wf_row_tiles(g.L, 1);
        const size_t control = align_up(ALIGN_F + n_count + n_flags);                       // in 4-byte words
        float* c = take(control);
        w.q.abort_word = reinterpret_cast<unsigned int*>(c);
        w.q.counters = c ? w.q.abort_word + ALIGN_F : nullptr;
        w.q.flags = c ? w.q.counters + n_count : nullptr;
        w.q.control_bytes = control * sizeof(float);
        w.q.layers = reinterpret_cast<GemmArgs*>(take(((size_t)p.c.n_group * p.c.n_layers * sizeof(GemmArgs) + 3) / 4));
        w.q.tails = reinterpret_cast<WfTailDesc*>(take(((size_t)p.c.n_group * sizeof(WfTailDesc) + 3) / 4));
        w.q.status = reinterpret_cast<unsigned int*>(take(ALIGN_F));   // outside the per-call memset
    }
    w.f = WfFwdWs{};
    if (forward) {
        const size_t rows_h = p.c.n_group - 1;
        w.f.nblk = (g.Lr + 255) / 256;
        w.f.ls = take(B * p.c.n_group * g.Lr);
        w.f.partials = reinterpret_cast<double*>(take(2 * (size_t)p.c.n_flows * B * w.f.nblk));
        const bool ar = p.all_rows();
        w.f.XA = take(ar ? rows_h * w.xslot : 0);
        w.f.XB = take(ar && !p.c.merge_res_skip ? rows_h * w.xslot : 0);       // merge_res_skip reads X0 throughout
        w.f.OUT = take(ar ? rows_h * w.xslot : 0);
        w.f.desc = reinterpret_cast<GemmArgs*>(take(ar ? ((size_t)p.c.n_flows * p.c.n_layers * rows_h * sizeof(GemmArgs) + 3) / 4 : 0));
    }
    w.total = o;
}

// rows[b][g][l] = z[b][G*l + g]   (efficient_model_ax.py:310)
__global__ __launch_bounds__(256) void wf_squeeze_kernel(const float* __restrict__ z, float* __restrict__ rows,
                                                         int G, int L, int Lr) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (l >= Lr) return;
    const float* zb = z + (size_t)b * G * L + (size_t)l * G;
    float* rb = rows + (size_t)b * G * Lr + l;
    for (int g = 0; g < G; ++g) rb[(size_t)g * Lr] = l < L ? zb[g] : 0.f;   // row tail (l >= L) stays zero
}

struct RowMap { int phys[64]; };

// audio[b][G*l + g] = rows[b][phys[g]][l]   (ax:346, with the accumulated PermuteHeight map)
__global__ __launch_bounds__(256) void wf_unsqueeze_kernel(const float* __restrict__ rows, float* __restrict__ audio,
                                                           int G, int L, int Lr, RowMap map) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (l >= L) return;
    const float* rb = rows + (size_t)b * G * Lr + l;
    float* ab = audio + (size_t)b * G * L + (size_t)l * G;
    for (int g = 0; g < G; ++g) ab[g] = rb[(size_t)map.phys[g] * Lr];
}

// rows: NaN -> 0 in place   (ax:13-16, 333-334)
__global__ __launch_bounds__(256) void wf_nan_to_zero_kernel(float* __restrict__ rows, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4*>(rows)[i];
    v.x = (v.x != v.x) ? 0.f : v.x; v.y = (v.y != v.y) ? 0.f : v.y;
    v.z = (v.z != v.z) ? 0.f : v.z; v.w = (v.w != v.w) ? 0.f : v.w;
    reinterpret_cast<float4*>(rows)[i] = v;
}

// mel_up[b][m][pad + l] = linear interpolation (align_corners=True) of mel[b][m][:] to L steps,
// fp32 exactly like ATen's upsample_linear1d (glow_ax.py:545-554)
__global__ __launch_bounds__(256) void wf_interp_kernel(const float* __restrict__ mel, float* __restrict__ up,
                                                        int n_mel, int kmel, int F, int L, int ld, int pad) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y, b = blockIdx.z;
    if (l >= L) return;
    float v;
    const float* src = mel + ((size_t)b * n_mel + m) * F;
    if (F == L) {
        v = src[l];
    } else {
        const float scale = L > 1 ? (float)(F - 1) / (float)(L - 1) : 0.f;
        const float real = scale * (float)l;
        const int i0 = (int)real;
        const int i1 = i0 + 1 < F ? i0 + 1 : F - 1;
        const float l1 = real - (float)i0;
        const float l0 = 1.0f - l1;
        v = gemm_lerp(l0, src[i0], l1, src[i1]);   // explicit contraction: every interpolation in the library rounds the same way
    }
    up[((size_t)b * kmel + m) * ld + pad + l] = v;
}

// X0[b][c][pad + l] = ws[c] * rows[b][row][l] + bs[c]   (Conv2d(1->C, 1x1), glow_ax.py:558)
__global__ __launch_bounds__(256) void wf_start_kernel(const float* __restrict__ rows, const float* __restrict__ ws,
                                                       const float* __restrict__ bs, float* __restrict__ x, int C,
                                                       int G, int row, int L, int Lr, int ld, int pad) {
    const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int b = blockIdx.z;
    if (n >= L) return;
    const float4 a = *reinterpret_cast<const float4*>(rows + ((size_t)b * G + row) * Lr + n);
    const int c0 = blockIdx.y * 16;
    float* xb = x + (size_t)b * C * ld + pad + n;
    const bool k1 = n + 1 < L, k2 = n + 2 < L, k3 = n + 3 < L;      // columns >= L are halo: keep them zero
    for (int c = c0; c < c0 + 16 && c < C; ++c) {
        const float w = ws[c], bias = bs[c];
        float4 v;
        v.x = wf_start_value(w, a.x, bias);
        v.y = k1 ? wf_start_value(w, a.y, bias) : 0.f; v.z = k2 ? wf_start_value(w, a.z, bias) : 0.f; v.w = k3 ? wf_start_value(w, a.w, bias) : 0.f;
        *reinterpret_cast<float4*>(xb + (size_t)c * ld) = v;
    }
}

// e = Wend * out + bend; log_s = e[0], t = e[1]; rows[b][row][l] = (rows[b][row][l] - t) / exp(log_s)
// (glow_ax.py:628, efficient_modules.py:61-62).  4 waves x 256 steps, each wave reduces C/4 channels.
__global__ __launch_bounds__(256) void wf_tail_kernel(const float* __restrict__ out, float* __restrict__ rows,
                                                      const float* __restrict__ Wend, const float* __restrict__ bend,
                                                      int C, int G, int row, int L, int Lr, int ld, int pad) {
    __shared__ __attribute__((aligned(16))) float part[3][2][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + lane * 4;
    float4 e0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = e0;
    const int cq = C / 4;
    const int cbeg = __builtin_amdgcn_readfirstlane(wv * cq);
    const float* ob = out + (size_t)b * C * ld + pad + n;
    for (int c = cbeg; c < cbeg + cq; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(ob + (size_t)c * ld);
        const float w0 = Wend[c], w1 = Wend[C + c];
        e0.x = wf_end_fma(w0, v.x, e0.x); e0.y = wf_end_fma(w0, v.y, e0.y); e0.z = wf_end_fma(w0, v.z, e0.z); e0.w = wf_end_fma(w0, v.w, e0.w);
        e1.x = wf_end_fma(w1, v.x, e1.x); e1.y = wf_end_fma(w1, v.y, e1.y); e1.z = wf_end_fma(w1, v.z, e1.z); e1.w = wf_end_fma(w1, v.w, e1.w);
    }
    if (wv > 0) {
        *reinterpret_cast<float4*>(&part[wv - 1][0][lane * 4]) = e0;
        *reinterpret_cast<float4*>(&part[wv - 1][1][lane * 4]) = e1;
    }
    __syncthreads();
    if (wv != 0 || n >= L) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float4 p0 = *reinterpret_cast<const float4*>(&part[q][0][lane * 4]);
        const float4 p1 = *reinterpret_cast<const float4*>(&part[q][1][lane * 4]);
        e0.x += p0.x; e0.y += p0.y; e0.z += p0.z; e0.w += p0.w;
        e1.x += p1.x; e1.y += p1.y; e1.z += p1.z; e1.w += p1.w;
    }
    const float b0 = bend[0], b1 = bend[1];
    float* rp = rows + ((size_t)b * G + row) * Lr + n;
    float4 a = *reinterpret_cast<const float4*>(rp);
    a.x = wf_row_update(a.x, e0.x, e1.x, b0, b1);
    a.y = n + 1 < L ? wf_row_update(a.y, e0.y, e1.y, b0, b1) : 0.f;       // row tail stays zero
    a.z = n + 2 < L ? wf_row_update(a.z, e0.z, e1.z, b0, b1) : 0.f;
    a.w = n + 3 < L ? wf_row_update(a.w, e0.w, e1.w, b0, b1) : 0.f;
    *reinterpret_cast<float4*>(rp) = a;
}

// Upsampled conditioning of every layer of one flow (glow_ax.py:545-554, 564-592): frames [B][2C*n_layers] rows of a
// padded frame-rate tensor -> up[layer][b][2C][pad + l], linear interpolation with align_corners=True, fp32 like ATen.
__global__ __launch_bounds__(256) void wf_interp_cond_kernel(const float* __restrict__ frames, float* __restrict__ up,
                                                             int rows2c, int n_layers, int F, int f_ld, int f_pad,
                                                             int L, int ld, int pad, size_t slot) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int ch = blockIdx.y, b = blockIdx.z;                 // ch in [0, 2C*n_layers)
    if (l >= L) return;
    const float* src = frames + ((size_t)b * rows2c * n_layers + ch) * f_ld + f_pad;
    float v;
    if (F == L) {
        v = src[l];
    } else {
        const float scale = L > 1 ? (float)(F - 1) / (float)(L - 1) : 0.f;
        const float real = scale * (float)l;
        const int i0 = (int)real;
        const int i1 = i0 + 1 < F ? i0 + 1 : F - 1;
        const float l1 = real - (float)i0;
        const float l0 = 1.0f - l1;
        v = gemm_lerp(l0, src[i0], l1, src[i1]);   // explicit contraction: every interpolation in the library rounds the same way
    }
    const int layer = ch / rows2c, r = ch % rows2c;
    up[(size_t)layer * slot + ((size_t)b * rows2c + r) * ld + pad + l] = v;
}


// Four time steps per thread, one 16-byte store (pad and ld multiples of 4): the scalar form writes its 0.8 GB per flow of the
// author's model with 4-byte stores at 1.6 TB/s.  Same arithmetic per element.
__global__ __launch_bounds__(256) void wf_interp_cond_vec_kernel(const float* __restrict__ frames, float* __restrict__ up,
                                                                 int rows2c, int n_layers, int F, int f_ld, int f_pad,
                                                                 int L, int ld, int pad, size_t slot) {
    const int l4 = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int ch = blockIdx.y, b = blockIdx.z;
    if (l4 >= L) return;
    const float* src = frames + ((size_t)b * rows2c * n_layers + ch) * f_ld + f_pad;
    const float scale = L > 1 ? (float)(F - 1) / (float)(L - 1) : 0.f;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int l = min(l4 + j, L - 1);
        if (F == L) {
            v[j] = src[l];
        } else {
            const float real = scale * (float)l;
            const int i0 = (int)real;
            const int i1 = i0 + 1 < F ? i0 + 1 : F - 1;
            const float l1 = real - (float)i0;
            const float l0 = 1.0f - l1;
            v[j] = gemm_lerp(l0, src[i0], l1, src[i1]);
        }
    }
    const int layer = ch / rows2c, r = ch % rows2c;
    float* dst = up + (size_t)layer * slot + ((size_t)b * rows2c + r) * ld + pad + l4;
    if (l4 + 3 < L) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (l4 + j < L) dst[j] = v[j];
    }
}


// Depthwise stage of a separable in-layer (glow_ax.py:525-527: Conv2d(C, C, (kh, kw), groups=C), width dilation dw,
// causal in height): y[b][c][l] = bias[c] + sum_{a >= a_min} sum_j w[c][a][j] * x_a[b][c][l + (j - kw/2) * dw], where
// x_a is the ring slot of height tap a (taps a < a_min reach above the first row: zeros, skipped).
__global__ __launch_bounds__(256) void wf_depthwise_kernel(WfSlots x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, int C,
                                                           int kh, int kw, int dw, int a_min, int L, int ld, int pad) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (l >= L) return;
    const size_t row = ((size_t)b * C + c) * ld + pad + l;
    const float* wc = w + (size_t)c * kh * kw;
    float acc = bias[c];
    for (int a = a_min; a < kh; ++a) {
        const float* xa = x.p[a] + row;
        for (int j = 0; j < kw; ++j) acc = fmaf(wc[a * kw + j], xa[(j - kw / 2) * dw], acc);
    }
    y[row] = acc;
}

// x[b][row0 + e][pad + t] = table[ids[b]][e]   (speaker embedding repeated over frames and concatenated, ax:286-291)
__global__ __launch_bounds__(256) void embed_rows_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                         float* __restrict__ x, int row0, int E, int C, int T, int ld,
                                                         int pad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const long long id = ids[b];          // an id outside the table poisons the utterance (NaN) instead of reading out of bounds
    x[((size_t)b * C + row0 + e) * ld + pad + t] = (id >= 0 && id < CTTS_N_SPEAKERS) ? table[(size_t)id * E + e] : __builtin_nanf("");
}

// y = alpha * x + r on the valid columns (rezero + residual of the model-level cond stack, ax:299-307)
__global__ __launch_bounds__(256) void scale_add_rows_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                             const float* __restrict__ r, float* __restrict__ y, int C,
                                                             int T, int ld, int pad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const size_t i = ((size_t)b * C + c) * ld + pad + t;
    const float a = alpha ? alpha[0] : 1.0f;
    y[i] = r ? a * x[i] + r[i] : a * x[i];
}

// x = (x + shift) * scale on the valid columns (shift_spect / scale_spect, ax:206-209, 281-284); the halo stays zero
__global__ __launch_bounds__(256) void affine_rows_kernel(float* __restrict__ x, int C, int T, int ld, int pad, float shift,
                                                          float scale) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const size_t i = ((size_t)b * C + c) * ld + pad + t;
    x[i] = (x[i] + shift) * scale;
}

// F.interpolate along time on padded rows, the arithmetic of ATen's upsample kernels:
//   mode 0 = 'linear', align_corners=True  (glow_ax.py:365 / ax:174): src = n * (Tin - 1) / (Tout - 1)
//   mode 1 = 'linear', align_corners=False (TransposedUpsampleNet residual, glow_ax.py:231): src = max((n + .5) * s - .5, 0)
//   mode 2 = 'nearest'                                                          : src = min(floor(n * s), Tin - 1)
// with s = 1 / scale_factor when a scale factor was given (ATen uses the reciprocal of the given factor), else Tin / Tout.
__global__ __launch_bounds__(256) void resample_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int Tin,
                                                            int ld_in, int pad_in, int Tout, int ld_out, int pad_out,
                                                            int mode, float s) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (n >= Tout) return;
    const float* src = x + ((size_t)b * C + c) * ld_in + pad_in;
    float v;
    if (mode == 2) {
        const int i = min((int)floorf((float)n * s), Tin - 1);
        v = src[i];
    } else {
        float real;
        if (mode == 0) real = (Tout > 1 ? (float)(Tin - 1) / (float)(Tout - 1) : 0.f) * (float)n;
        else real = fmaxf(s * ((float)n + 0.5f) - 0.5f, 0.f);
        const int i0 = (int)real;
        const int i1 = i0 + 1 < Tin ? i0 + 1 : Tin - 1;
        const float l1 = real - (float)i0;
        const float l0 = 1.0f - l1;
        v = gemm_lerp(l0, src[i0], l1, src[i1]);   // explicit contraction: every interpolation in the library rounds the same way
    }
    y[((size_t)b * C + c) * ld_out + pad_out + n] = v;
}

// ConvTranspose1d(stride s, padding p) as s stride-1 convolutions (one per output residue r = (n + p) mod s, evaluated
// by ctts_conv1d_f32 over the INPUT positions m): out[n] = phase[r][(n + p) / s].  phases: [s][B][C][ld_in].
__global__ __launch_bounds__(256) void interleave_phases_kernel(const float* __restrict__ ph, float* __restrict__ y, int C,
                                                                int s, int p, int Tin, int ld_in, int pad_in, int Tout,
                                                                int ld_out, int pad_out, size_t phase_stride) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (n >= Tout) return;
    const int q = n + p, r = q % s, m = q / s;
    float v = 0.f;
    if (m < Tin) v = ph[(size_t)r * phase_stride + ((size_t)b * C + c) * ld_in + pad_in + m];
    y[((size_t)b * C + c) * ld_out + pad_out + n] = v;
}

// inverse of the "perceived volume" companding (efficient_model_ax.py:342-344): z > 0 -> 10^log2(z), z < 0 -> -(10^log2(-z))
__global__ __launch_bounds__(256) void vol_unscale_kernel(float* __restrict__ x, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    if (v > 0.f) x[i] = powf(10.0f, log2f(v));
    else if (v < 0.f) x[i] = -powf(10.0f, log2f(-v));
}

// y[n] = x[n] + p * y[n-1], one workgroup per utterance, fp64 state (scipy.signal.lfilter([1],[1,-p]) runs in
// float64 on the reference's CPU path, ax:351-355).  Thread t owns one contiguous span: pass 1 runs the recurrence
// from a zero state to get the span's own contribution, thread 0 chains the 256 span ends
// (carry_out = end + p^len * carry_in), pass 2 re-runs each span from its true incoming state.
// x and y may alias (the host wrapper filters in place): no __restrict__; every thread reads its whole span in pass 1
// before any thread writes (barrier), and pass 2 reads element n before writing element n of its own span only.
__global__ __launch_bounds__(256) void deemphasis_kernel(const float* x, float* y, int T, double p) {
    __shared__ double ends[256], gains[256], carry[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int span = (T + 255) / 256;
    const int n0 = min(t * span, T), n1 = min(n0 + span, T);
    const float* xb = x + (size_t)b * T;
    float* yb = y + (size_t)b * T;
    double s = 0.0, gpow = 1.0;
    for (int n = n0; n < n1; ++n) { s = (double)xb[n] + p * s; gpow *= p; }
    ends[t] = s; gains[t] = gpow;
    __syncthreads();
    if (t == 0) {
        double c = 0.0;
        for (int i = 0; i < 256; ++i) { carry[i] = c; c = ends[i] + gains[i] * c; }
    }
    __syncthreads();
    s = carry[t];
    for (int n = n0; n < n1; ++n) { s = (double)xb[n] + p * s; yb[n] = (float)s; }
}

// Vector form: a thread owns 4 consecutive columns (16-byte aligned) of one channel.  DW = 0 stands for any width
// dilation that is a multiple of 4: every tap is then ONE aligned 16-byte load for the 4 columns; for DW = 1, 2 the
// taps of the 4 columns overlap, so an aligned window [l - 4*HW, l + 4 + 4*HW) is loaded once per height tap and the
// taps are picked out of registers (compile-time indices).
template <int KW, int DW>
__global__ __launch_bounds__(256) void wf_depthwise_vec_kernel(WfSlots x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ y,
                                                               int C, int kh, int dw, int a_min, int L, int ld, int pad) {
    const int l = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int c = blockIdx.y, b = blockIdx.z;
    if (l >= L) return;
    const size_t row = ((size_t)b * C + c) * ld + pad + l;
    const float* wc = w + (size_t)c * kh * KW;
    const float bc = bias[c];
    float acc[4] = {bc, bc, bc, bc};
    for (int a = a_min; a < kh; ++a) {
        const float* xa = x.p[a] + row;
        if constexpr (DW == 0) {
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(xa + (j - KW / 2) * dw);
                const float wj = wc[a * KW + j];
                acc[0] = fmaf(wj, v.x, acc[0]); acc[1] = fmaf(wj, v.y, acc[1]);
                acc[2] = fmaf(wj, v.z, acc[2]); acc[3] = fmaf(wj, v.w, acc[3]);
            }
        } else {
            constexpr int HW = ((KW / 2) * DW + 3) / 4;          // float4s on each side of the centre one
            float win[4 * (2 * HW + 1)];
#pragma unroll
            for (int q = 0; q < 2 * HW + 1; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(xa + 4 * (q - HW));
                win[4 * q] = v.x; win[4 * q + 1] = v.y; win[4 * q + 2] = v.z; win[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < KW; ++j) {
                const float wj = wc[a * KW + j];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(wj, win[4 * HW + e + (j - KW / 2) * DW], acc[e]);
            }
        }
    }
    // columns >= L are halo and must stay zero
    float4 o;
    o.x = acc[0];
    o.y = l + 1 < L ? acc[1] : 0.f; o.z = l + 2 < L ? acc[2] : 0.f; o.w = l + 3 < L ? acc[3] : 0.f;
    *reinterpret_cast<float4*>(y + row) = o;
}

template <int KW>
void launch_depthwise_vec(dim3 grid, hipStream_t s, const WfSlots& xs, const float* w, const float* b, float* y, int C,
                          int kh, int dw, int a_min, int L, int ld, int pad) {
    if (dw == 1) hipLaunchKernelGGL((wf_depthwise_vec_kernel<KW, 1>), grid, dim3(256), 0, s, xs, w, b, y, C, kh, dw, a_min, L, ld, pad);
    else if (dw == 2) hipLaunchKernelGGL((wf_depthwise_vec_kernel<KW, 2>), grid, dim3(256), 0, s, xs, w, b, y, C, kh, dw, a_min, L, ld, pad);
    else hipLaunchKernelGGL((wf_depthwise_vec_kernel<KW, 0>), grid, dim3(256), 0, s, xs, w, b, y, C, kh, dw, a_min, L, ld, pad);
}

// InvertibleConv1x1.inverse over the latent rows (efficient_modules.py:269-286): new[i] = sum_j Winv[i][j] old[j] for
// the n active logical rows, in place (a thread owns its columns), rows addressed through the logical -> physical map
__global__ __launch_bounds__(256) void wf_mix_kernel(float* __restrict__ rows, const float* __restrict__ Winv, RowMap map,
                                                     int n, int G, int Lr) {
    __shared__ float sW[64 * 64];
    for (int i = threadIdx.x; i < n * n; i += 256) sW[i] = Winv[i];
    __syncthreads();
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= Lr) return;
    float v[64];
    float* base = rows + (size_t)b * G * Lr + l;
#pragma unroll 1
    for (int j = 0; j < n; ++j) v[j] = base[(size_t)map.phys[j] * Lr];
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        float acc = 0.f;
#pragma unroll 1
        for (int j = 0; j < n; ++j) acc = fmaf(sW[i * n + j], v[j], acc);
        base[(size_t)map.phys[i] * Lr] = acc;
    }
}

// ---- analysis direction (efficient_model_ax.py:184-277) ----------------------------------------------------------------------
// rows[b][g][l] = y[b][G*l + g], y = PreEmphasis(audio) when p != 0 (efficient_loss.py:16-20: y[t] = x[t] - p x[t-1], reflected
// at t = 0: y[0] = x[0] - p x[1])
__global__ __launch_bounds__(256) void wf_fwd_squeeze_kernel(const float* __restrict__ audio, float* __restrict__ rows, int G,
                                                             int L, int Lr, float p) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (l >= Lr) return;
    const size_t T = (size_t)G * L;
    const float* ab = audio + (size_t)b * T;
    float* rb = rows + (size_t)b * G * Lr + l;
    for (int g = 0; g < G; ++g) {
        float v = 0.f;                                                          // row tail (l >= L) stays zero
        if (l < L) {
            const size_t t = (size_t)l * G + g;
            v = ab[t];
            if (p != 0.f) v = __builtin_fmaf(-p, t > 0 ? ab[t - 1] : ab[T > 1 ? 1 : 0], v);
        }
        rb[(size_t)g * Lr] = v;
    }
}

// X0[r][b][c][pad + l] = ws[c] * rows[b][phys[r]][l] + bs[c] for every WN input row r = 0 .. nrows - 1 of a flow (wf_start_kernel
// over all rows; blockIdx.z = r * batch + b)
__global__ __launch_bounds__(256) void wf_fwd_start_rows_kernel(const float* __restrict__ rows, const float* __restrict__ ws,
                                                                const float* __restrict__ bs, float* __restrict__ x, size_t xslot,
                                                                RowMap map, int C, int G, int batch, int L, int Lr, int ld, int pad) {
    const int n = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int r = blockIdx.z / batch, b = blockIdx.z - r * batch;
    if (n >= L) return;
    const float4 a = *reinterpret_cast<const float4*>(rows + ((size_t)b * G + map.phys[r]) * Lr + n);
    const int c0 = blockIdx.y * 16;
    float* xb = x + (size_t)r * xslot + (size_t)b * C * ld + pad + n;
    const bool k1 = n + 1 < L, k2 = n + 2 < L, k3 = n + 3 < L;      // columns >= L are halo: keep them zero
    for (int c = c0; c < c0 + 16 && c < C; ++c) {
        const float w = ws[c], bias = bs[c];
        float4 v;
        v.x = wf_start_value(w, a.x, bias);
        v.y = k1 ? wf_start_value(w, a.y, bias) : 0.f; v.z = k2 ? wf_start_value(w, a.z, bias) : 0.f; v.w = k3 ? wf_start_value(w, a.w, bias) : 0.f;
        *reinterpret_cast<float4*>(xb + (size_t)c * ld) = v;
    }
}

// e = Wend * out_r + bend; log_s = e[0], t = e[1]; rows[b][phys[r + 1]][l] = rows[..] * exp(log_s) + t; ls[b][r][l] = log_s
// (efficient_modules.py:38) for WN rows r = r0 + blockIdx.z: one row per launch (row-wise form, out_rstride = 0) or all rows of a
// flow (all-rows form).  The end conv sums as wf_tail_kernel does: four fma chains over C / 4 ascending channels, ((p0 + p1) + p2) + p3.
__global__ __launch_bounds__(256) void wf_fwd_tail_kernel(const float* __restrict__ out, size_t out_rstride, float* __restrict__ rows,
                                                          float* __restrict__ ls, const float* __restrict__ Wend,
                                                          const float* __restrict__ bend, RowMap map, int r0, int C, int G, int L,
                                                          int Lr, int ld, int pad) {
    __shared__ __attribute__((aligned(16))) float part[3][2][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, r = r0 + blockIdx.z;
    const int n = blockIdx.x * 256 + lane * 4;
    float4 e0 = make_float4(0.f, 0.f, 0.f, 0.f), e1 = e0;
    const int cq = C / 4;
    const int cbeg = __builtin_amdgcn_readfirstlane(wv * cq);
    const float* ob = out + (size_t)blockIdx.z * out_rstride + (size_t)b * C * ld + pad + n;
    for (int c = cbeg; c < cbeg + cq; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(ob + (size_t)c * ld);
        const float w0 = Wend[c], w1 = Wend[C + c];
        e0.x = wf_end_fma(w0, v.x, e0.x); e0.y = wf_end_fma(w0, v.y, e0.y); e0.z = wf_end_fma(w0, v.z, e0.z); e0.w = wf_end_fma(w0, v.w, e0.w);
        e1.x = wf_end_fma(w1, v.x, e1.x); e1.y = wf_end_fma(w1, v.y, e1.y); e1.z = wf_end_fma(w1, v.z, e1.z); e1.w = wf_end_fma(w1, v.w, e1.w);
    }
    if (wv > 0) {
        *reinterpret_cast<float4*>(&part[wv - 1][0][lane * 4]) = e0;
        *reinterpret_cast<float4*>(&part[wv - 1][1][lane * 4]) = e1;
    }
    __syncthreads();
    if (wv != 0 || n >= L) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float4 p0 = *reinterpret_cast<const float4*>(&part[q][0][lane * 4]);
        const float4 p1 = *reinterpret_cast<const float4*>(&part[q][1][lane * 4]);
        e0.x += p0.x; e0.y += p0.y; e0.z += p0.z; e0.w += p0.w;
        e1.x += p1.x; e1.y += p1.y; e1.z += p1.z; e1.w += p1.w;
    }
    const float b0 = bend[0], b1 = bend[1];
    float* rp = rows + ((size_t)b * G + map.phys[r + 1]) * Lr + n;
    float4 a = *reinterpret_cast<const float4*>(rp);
    const bool k1 = n + 1 < L, k2 = n + 2 < L, k3 = n + 3 < L;      // row tails stay zero
    float4 s;
    s.x = e0.x + b0; s.y = k1 ? e0.y + b0 : 0.f; s.z = k2 ? e0.z + b0 : 0.f; s.w = k3 ? e0.w + b0 : 0.f;
    a.x = wf_row_forward(a.x, s.x, e1.x, b1);
    a.y = k1 ? wf_row_forward(a.y, s.y, e1.y, b1) : 0.f;
    a.z = k2 ? wf_row_forward(a.z, s.z, e1.z, b1) : 0.f;
    a.w = k3 ? wf_row_forward(a.w, s.w, e1.w, b1) : 0.f;
    *reinterpret_cast<float4*>(rp) = a;
    *reinterpret_cast<float4*>(ls + ((size_t)b * G + r) * Lr + n) = s;
}

// Behind a flow's coupling, from its log_s rows ls[b][0 .. nrows)[l]: log_s_sum[b][l] (+)= their fp32 sum in row order
// (ax:269-273), the optional copy into log_s[b][s_off + r][l], and stage one of the fp64 sum: a thread adds its column's rows in
// row order, the block adds its 256 columns as a fixed tree -> partials[b][blockIdx.x].  No atomics: two calls give the same bits,
// and an item's value does not depend on its batch.
__global__ __launch_bounds__(256) void wf_fwd_reduce_kernel(const float* __restrict__ ls, int nrows, int G, int L, int Lr,
                                                            float* __restrict__ log_s, int S, int s_off,
                                                            float* __restrict__ log_s_sum, int first,
                                                            double* __restrict__ partials, int nblk) {
    __shared__ double red[256];
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    double s64 = 0.0;
    if (l < L) {
        float s32 = 0.f;
        const float* lp = ls + (size_t)b * G * Lr + l;
        for (int r = 0; r < nrows; ++r) {
            const float v = lp[(size_t)r * Lr];
            s32 += v;
            s64 += (double)v;
            if (log_s) log_s[((size_t)b * S + s_off + r) * L + l] = v;
        }
        float* o = log_s_sum + (size_t)b * L + l;
        *o = first ? s32 : *o + s32;
    }
    red[threadIdx.x] = s64;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[(size_t)b * nblk + blockIdx.x] = red[0];
}

// stage two: sums[b][k] = the partials of flow k and item b, added in block order (one thread each)
__global__ __launch_bounds__(64) void wf_fwd_sums_kernel(const double* __restrict__ partials, double* __restrict__ sums,
                                                         int n_flows, int batch, int nblk) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_flows * batch) return;
    const int k = i / batch, b = i - k * batch;
    const double* p = partials + ((size_t)k * batch + b) * nblk;
    double s = 0.0;
    for (int j = 0; j < nblk; ++j) s += p[j];
    sums[(size_t)b * n_flows + k] = s;
}

// offsets (floats) of the forward 1x1 matrices W_k in the forward blob; PermuteHeight needs none
size_t wf_fwd_mix_offset(const WfPlan& p, int k) {
    size_t o = 0;
    if (p.c.mixing != CTTS_MIX_CONV1X1) return 0;
    for (int j = 0; j < k; ++j) o = align_up(o + (size_t)p.n_rem[j] * p.n_rem[j]);
    return o;
}

void wf_permutation(int k, int G, int* perm) {
    for (int g = 0; g < G; ++g) perm[g] = G - 1 - g;                       // reverse (k % 4 in {0,1})
    if (k % 4 == 2 || k % 4 == 3) {                                        // reverse each half separately
        const int half = G / 2;
        for (int g = 0; g < half; ++g) perm[g] = half - 1 - g;
        for (int g = half; g < G; ++g) perm[g] = G - 1 - (g - half);
    }
}

}  // namespace
}  // namespace ctts

using namespace ctts;

namespace {

// ---- region split of a fused-layer launch (WfRegionSplit, decided in WfCall::open) ------------------------------------------------
constexpr int WF_TILE = 256;          // columns per region unit: every launch shape's tile width divides it
// only where the launch is the 128 x 256 shape: below 256 blocks - batch <= 4 at 900 frames - a layer lasts ~35-100 us and three
// launches + six event operations per layer make the call host-bound: measured 38.7 -> 78 ms at batch 1
constexpr int WF_SPLIT_MIN_BLOCKS = 256;
constexpr int WF_NBIG = 2;            // big regions per layer (2: A | M | B on three streams)
constexpr int WF_NREG = 2 * WF_NBIG - 1;     // regions incl. the one-tile separators: big 0, sep 0, big 1, sep 1, ...
// The row queue is taken from this many 128-column items per layer on: where the per-layer launches stop being the eight-wave
// split-K tile (gemm_f32_small.hip gate_rs_splitk8_tile, up to GATE_RS_SPLITK_MAX_BLOCKS = 256 items).  Config 4, round 5: batch 1
// (113 items) 30.9 ms per layer against 40.6 queued; batch 2 (226 items) 52.0 against 55.7 (until the eight-wave tile the queue was
// 2 % ahead there: 56.9 against 58.3 ms, and the bound was 200); batch 3 (339 items) 74.4 queued against 92.9.
constexpr int WF_ROW_QUEUE_MIN_ITEMS = 257;
// Upper bound: from ~1250 items per layer on - batch 10 at 900 frames: 204.0 ms queued against 207.6, batch 12: 245.1 against 243.4,
// batch 16: 327 against 319 - the per-layer launches on the 128 x 256 shape with the region split are ahead again: more work per
// workgroup, and a layer's tail is small against it
constexpr int WF_ROW_QUEUE_MAX_ITEMS = 1250;
// Which tile body (measured, profiles/r4_12): below 400 items of 128 columns per layer the split-K body (items of 128 x 64, half the
// serial chain each: 97 -> 77 ms at batch 3 x 900 frames, 95 -> 66 at 8 x 300); the 128 x 128 body from there on
constexpr int WF_ROW_QUEUE_SPLITK_BELOW = 400;
// audio[b][:] = NaN when the row queue's abort word is set, and the workspace's sticky status word says so until a later
// call reports it (CTTS_E_ABORT): the NaN is the in-stream marker, the status the one a caller can act on
constexpr unsigned int WF_ABORT_MAGIC = 0xAB0F7001u;       // a value, not a flag: the workspace may start out as anything
__global__ void wf_abort_poison_kernel(const unsigned int* __restrict__ abort_word, float* __restrict__ audio, long long n,
                                       unsigned int* __restrict__ status) {
    if (*abort_word == 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = WF_ABORT_MAGIC;
    float* a = audio + (size_t)blockIdx.x * n;
    for (long long i = threadIdx.x; i < n; i += 256) a[i] = __builtin_nanf("");
}

// Host side of the row queue's descriptors: a PINNED buffer per host thread, so that the per-flow copies are ordinary stream-ordered
// DMA whatever the runtime does with pageable sources; the buffer is rewritten by the thread's next call only after the event
// recorded behind this call's last copy (normally long past: the wait is a formality).  Never freed (as the helper streams below).
struct WfDescHost {
    char* host = nullptr;                                  // bytes
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false, in_call = false;
    int begin(size_t n) {
        if (in_call) CTTS_CHECK_HIP(hipDeviceSynchronize());     // the previous call failed half-way: its copies may still be queued
        in_call = true;
        if (pending) { CTTS_CHECK_HIP(hipEventSynchronize(done)); pending = false; }
        if (!done) CTTS_CHECK_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (n > cap) {
            if (host) CTTS_CHECK_HIP(hipHostFree(host));
            host = nullptr; cap = 0;
            CTTS_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), n, hipHostMallocDefault));
            cap = n;
        }
        return CTTS_OK;
    }
    int end(hipStream_t s) {
        CTTS_CHECK_HIP(hipEventRecord(done, s));
        pending = true;
        in_call = false;
        return CTTS_OK;
    }
};
thread_local WfDescHost t_wf_desc;

struct WfRegionStreams {              // per host thread: one helper stream per region but the first + double-buffered events
    hipStream_t st[WF_NREG] = {};
    hipEvent_t fork = nullptr, ev[WF_NREG][2] = {};
    bool ready = false;
    int init() {
        if (ready) return CTTS_OK;
        for (int k = 1; k < WF_NREG; ++k) CTTS_CHECK_HIP(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking));
        CTTS_CHECK_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        for (int k = 0; k < WF_NREG; ++k)
            for (int q = 0; q < 2; ++q) CTTS_CHECK_HIP(hipEventCreateWithFlags(&ev[k][q], hipEventDisableTiming));
        ready = true;
        return CTTS_OK;
    }
};
thread_local WfRegionStreams t_wf_streams;

// Region split of the fused layer (round 4): every layer launch used to wait for the slowest of the previous layer's 456
// workgroups although tile t of layer i + 1 needs only tiles t - 1, t, t + 1 of layer i (dilation <= 128 < one 256-column
// tile).  The columns are cut into three regions A | M (one tile) | B launched on three streams: A(i+1) and B(i+1) wait
// for M(i) only, M(i+1) waits for A(i) and B(i), so the two halves drift by up to a layer and each half's tail overlaps
// the other's next layer.  Same kernel, same tiles: bit-identical to the single launch (CTTS_WF_NO_REGION_SPLIT).
struct WfRegionSplit {
    bool on = false;
    int ntiles = 0, L = 0;
    int tile0[WF_NREG + 1] = {};
    void plan() {       // big regions of (ntiles - separators) / WF_NBIG tiles, one-tile separators between them
        const int big = (ntiles - (WF_NBIG - 1)) / WF_NBIG;
        int t = 0;
        for (int k = 0; k < WF_NREG; ++k) { tile0[k] = t; t += (k & 1) ? 1 : big; }
        tile0[WF_NREG] = ntiles;          // the last big region takes the remainder
    }
    static GemmArgs shifted(const GemmArgs& a, int tile0, int nt, int L) {
        GemmArgs r = a;
        const long long co = (long long)tile0 * WF_TILE;
        for (int j = 0; j < r.nseg; ++j) r.seg[j].base += co;
        if (r.dst0) r.dst0 += co;
        if (r.dst1) r.dst1 += co;
        if (r.src0) r.src0 += co;
        if (r.addend) r.addend += co;
        const int cols = L - tile0 * WF_TILE;
        r.L = cols < nt * WF_TILE ? cols : nt * WF_TILE;
        r.ntiles = nt;
        r.shape_blocks = 255;       // every region on the 128 x 128 shape (same K order as the 128 x 256 one; never the split-K shape)
        return r;
    }
    int begin_row(hipStream_t s) {
        auto& t = t_wf_streams;
        int rc = t.init(); if (rc) return rc;
        plan();
        CTTS_CHECK_HIP(hipEventRecord(t.fork, s));                      // the row's start kernel has written every column
        for (int k = 1; k < WF_NREG; ++k) CTTS_CHECK_HIP(hipStreamWaitEvent(t.st[k], t.fork, 0));
        return CTTS_OK;
    }
    // region k of layer i waits for its neighbours' layer i - 1 (its own layer i - 1 precedes it on its stream)
    int layer(const GemmArgs& a, int i, hipStream_t s) {
        auto& t = t_wf_streams;
        const int par = i & 1, prev = par ^ 1;
        for (int k = 0; k < WF_NREG; ++k) {
            hipStream_t st = k == 0 ? s : t.st[k];
            if (i > 0) {
                if (k > 0) CTTS_CHECK_HIP(hipStreamWaitEvent(st, t.ev[k - 1][prev], 0));
                if (k + 1 < WF_NREG) CTTS_CHECK_HIP(hipStreamWaitEvent(st, t.ev[k + 1][prev], 0));
            }
            const int rc = launch_gemm_f32(GEMM_EPI_GATE_RS, shifted(a, tile0[k], tile0[k + 1] - tile0[k], L), st);
            if (rc) return rc;
            CTTS_CHECK_HIP(hipEventRecord(t.ev[k][par], st));
        }
        last_par = par;
        return CTTS_OK;
    }
    int end_row(hipStream_t s) {                                        // the row's tail kernel reads every column
        auto& t = t_wf_streams;
        for (int k = 1; k < WF_NREG; ++k) CTTS_CHECK_HIP(hipStreamWaitEvent(s, t.ev[k][last_par], 0));
        return CTTS_OK;
    }
    int last_par = 0;
};


// Row-queue calls of this thread whose status word has not been looked at yet: (workspace, event recorded behind the call's
// last kernel).  A SET, not the last one: a thread that alternates two workspaces (two batch sizes, two models) must find
// the first one's abort at its next call on THAT workspace; and the event, not the new call's stream, is what is waited for -
// the earlier call may have run on another stream.
struct WfPending {
    static constexpr int N = 16;
    const void* ws[N] = {};
    unsigned int* st[N] = {};                               // the workspace's status word
    hipEvent_t ev[N] = {};
    unsigned long long age[N] = {};
    unsigned long long clock = 0;
    int find(const void* w) const {
        for (int i = 0; i < N; ++i)
            if (ws[i] == w) return i;
        return -1;
    }
};
thread_local WfPending t_wf_pending;

// Reads the workspace's sticky status word and clears it: CTTS_E_ABORT (+ ctts_last_error) if a row-queue call on this
// workspace gave up its bounded wait since the last report.  `done`: the event behind that call (waited for), or NULL (then
// stream `s` is synchronised: the caller says the call ran there).
int wf_report_abort(unsigned int* status, hipEvent_t done, hipStream_t s) {
    unsigned int host = 0;
    if (done) CTTS_CHECK_HIP(hipEventSynchronize(done));
    CTTS_CHECK_HIP(hipMemcpyAsync(&host, status, sizeof host, hipMemcpyDeviceToHost, s));
    CTTS_CHECK_HIP(hipStreamSynchronize(s));
    if (host != WF_ABORT_MAGIC) return CTTS_OK;
    CTTS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof host, s));
    set_error("waveflow: the row queue of an earlier call on this workspace aborted (a bounded wait between workgroups "
              "expired); that call's audio is NaN.  Repeat it - with CTTS_WF_NO_ROW_QUEUE=1 (one launch per layer) if it "
              "happens again");
    return CTTS_E_ABORT;
}

// the pending entry of `workspace`, if any, is checked and removed
int wf_check_pending(const void* workspace, unsigned int* status, hipStream_t s) {
    auto& pd = t_wf_pending;
    const int i = pd.find(workspace);
    if (i < 0) return CTTS_OK;
    pd.ws[i] = nullptr;
    return wf_report_abort(status, pd.ev[i], s);
}

// remember that `workspace` ran the row queue on `s`.  A full table gives up its oldest entry: that workspace's status is read
// now (its call is long done) and an abort found there is reported by THIS call - late and against the wrong call, but not lost.
int wf_note_pending(const void* workspace, unsigned int* status, hipStream_t s) {
    auto& pd = t_wf_pending;
    int i = pd.find(workspace);
    int rc = CTTS_OK;
    if (i < 0) i = pd.find(nullptr);
    if (i < 0) {
        i = 0;
        for (int k = 1; k < WfPending::N; ++k)
            if (pd.age[k] < pd.age[i]) i = k;
        pd.ws[i] = nullptr;
        rc = wf_report_abort(pd.st[i], pd.ev[i], s);
    }
    if (!pd.ev[i]) CTTS_CHECK_HIP(hipEventCreateWithFlags(&pd.ev[i], hipEventDisableTiming));
    CTTS_CHECK_HIP(hipEventRecord(pd.ev[i], s));
    pd.ws[i] = workspace;
    pd.st[i] = status;
    pd.age[i] = ++pd.clock;
    return rc;
}

int wf_launched(const char* what) { CTTS_CHECK_LAUNCH(what); return CTTS_OK; }      // behind a kernel launch: its error, if any

// What an entry point hands to a direction driver: `in` -> `out` is z -> audio (inverse) or audio -> z (analysis).  cond = mel
// [B][n_mel][frames] (dense) when the single linear cond layer is folded into the GEMM, or the per-flow frame-rate conditioning
// [n_flows][B][2C*n_layers][cond_ld] (padded rows).
struct WfIo {
    const ctts_waveflow_config* cfg; const void* packed;
    const float *in, *cond; int cond_ld, cond_pad;
    float* out; int batch, samples, frames;
    void* workspace; size_t workspace_bytes; void* stream;
};

// The analysis direction (ctts_waveflow_forward_*): where everything but the latent goes.  WfCall::open(io, NULL) = the inverse.
struct WfForward {
    const float* mix;            // forward blob: W_k of the 1x1-conv mixing (NULL with PermuteHeight)
    float preemphasis;           // PreEmphasis coefficient applied to the audio first; 0 = none
    int ignore_nan;              // NaN -> 0 behind every coupling (ax:253-254)
    float* log_s;                // [B][S][L] or NULL
    float* log_s_sum;            // [B][L]
    double* sums;                // [B][n_flows]
};

// Logical row g of the current flow lives in physical row phys[g] of w.rows; n rows are active.  With early outputs only the LAST
// n_rem rows of the squeezed latent are active in the last flows (the last split, ax:311-313).
struct WfRowMap {
    int phys[64], n = 0;
    void reset(int G, int active) {                          // the last `active` of G rows, in place
        n = active;
        for (int i = 0; i < n; ++i) phys[i] = G - n + i;
    }
    void permute(int k) {                                    // PermuteHeight of flow k (its own inverse) composes into the map
        int perm[64], tmp[64];
        wf_permutation(k, n, perm);
        for (int i = 0; i < n; ++i) tmp[i] = phys[perm[i]];
        for (int i = 0; i < n; ++i) phys[i] = tmp[i];
    }
    void peel_front(int count, WfRowMap& out) {              // analysis: the first `count` active rows leave, appended to `out`
        for (int i = 0; i < count; ++i) out.phys[out.n++] = phys[i];
        for (int i = count; i < n; ++i) phys[i - count] = phys[i];
        n -= count;
    }
    void rejoin_front(int count, int G) {                    // inverse: the `count` physical rows just before the active block re-join in front
        for (int i = n - 1; i >= 0; --i) phys[i + count] = phys[i];
        for (int i = 0; i < count; ++i) phys[i] = G - n - count + i;
        n += count;
    }
    RowMap device() const {
        RowMap m;
        for (int i = 0; i < 64; ++i) m.phys[i] = i < n ? phys[i] : 0;
        return m;
    }
};

// One call of the runner, the shared body of the two directions: plan, geometry, carved workspace, the caller's tensors, the launch
// forms decided once per call, the row map - and every descriptor and launch that both directions make.
struct WfCall {
    WfPlan p; WfGeom g; WfWs w;
    const float *blob = nullptr, *cond = nullptr;
    int cond_ld = 0, cond_pad = 0, batch = 0, frames = 0;
    hipStream_t s = nullptr;
    bool fuse = false, sep_fuse = false, all_rows = false;
    WfRegionSplit rsplit;
    WfRowMap rows;
    long long cstride() const { return (long long)p.C * g.ld; }
    dim3 lgrid() const { return dim3((g.Lr + 255) / 256, batch); }                  // a thread per column of w.rows
    float* X(int layer, int slot) const { return w.X + ((size_t)layer * p.ring + slot) * w.xslot; }
    // layer `layer`'s input of WN row `row`: the ring slot, or full-height storage
    float* XR(int layer, int row) const {
        return all_rows ? ((layer & 1) ? w.f.XB : w.f.XA) + (size_t)row * w.xslot : X(layer, row % p.ring);
    }
    float* OUT(int row) const { return all_rows ? w.f.OUT + (size_t)row * w.xslot : w.out; }      // the row's skip sum
    // The prologue up to the first launch: plan, geometry, argument checks, carved workspace, launch forms.
    int open(const WfIo& io, const WfForward* fw) {
        int rc = make_wf_plan(io.cfg, p); if (rc) return rc;
        rc = make_wf_geom(p, io.samples, g); if (rc) return rc;
        const char* const what = fw ? "forward" : "inverse";
        CTTS_CHECK_ARG(io.packed && io.in && io.cond && io.out && io.workspace && io.batch >= 1 && io.frames >= 1,
                       "waveflow %s: bad argument", what);
        CTTS_CHECK_ARG(!fw || (fw->log_s_sum && fw->sums && (fw->mix || p.c.mixing != CTTS_MIX_CONV1X1) && io.batch <= 65535 / p.c.n_group),
                       "waveflow forward: bad argument (log_s_sum, sums, the forward blob of a 1x1-conv model; batch * n_group <= 65535)");
        wf_carve(p, g, io.batch, static_cast<float*>(io.workspace), w, fw != nullptr);
        if (w.total * sizeof(float) > io.workspace_bytes) {
            set_error("waveflow %s: workspace %zu bytes < required %zu", what, io.workspace_bytes, w.total * sizeof(float));
            return CTTS_E_WORKSPACE;
        }
        blob = static_cast<const float*>(io.packed); s = as_stream(io.stream);
        cond = io.cond; cond_ld = io.cond_ld; cond_pad = io.cond_pad; batch = io.batch; frames = io.frames;
        fuse = p.fused() && !tuning().wf_no_fuse;
        sep_fuse = p.sep_fused() && !tuning().wf_no_fuse;
        // Analysis direction, all-rows form: every row's WN input is known, so layer i of ALL rows is one launch (gemm_f32_small.hip
        // wf_all_rows_layer_kernel) on full-height storage - layer i reads XA / XB by parity and writes the other (never in place: other
        // rows' height taps read the same input), the skip sum of row r is OUT[r].  The model selects it, CTTS_WF_FWD_ROWWISE (or a knob
        // that takes the DMA-staged small tile away) falls back to the row-wise form.
        all_rows = fw && p.all_rows() && fuse && !tuning().wf_fwd_rowwise && !tuning().f32_no_glds && !tuning().f32_no_small;
        rsplit.on = fuse && !tuning().wf_no_region_split && g.ntiles >= 8 && (long long)g.ntiles * batch >= WF_SPLIT_MIN_BLOCKS &&
                    !tuning().f32_force_small;
        rsplit.ntiles = g.ntiles; rsplit.L = g.L;
        return CTTS_OK;
    }
    // The prologue's launches: w.rows <- the squeezed input (analysis: the pre-emphasised audio), and mel interpolated once to L steps
    // (models whose cond layer is folded into the in-layer GEMM)
    int squeeze(const float* in, const WfForward* fw) const {
        if (fw) hipLaunchKernelGGL(wf_fwd_squeeze_kernel, lgrid(), dim3(256), 0, s, in, w.rows, p.c.n_group, g.L, g.Lr, fw->preemphasis);
        else hipLaunchKernelGGL(wf_squeeze_kernel, lgrid(), dim3(256), 0, s, in, w.rows, p.c.n_group, g.L, g.Lr);
        CTTS_CHECK_LAUNCH("wf_squeeze");
        if (p.precond) return CTTS_OK;
        hipLaunchKernelGGL(wf_interp_kernel, dim3((g.L + 255) / 256, p.c.n_mel_channels, batch), dim3(256), 0, s, cond, w.mel_up,
                           p.c.n_mel_channels, p.kmel, frames, g.L, g.ld, g.pad);
        return wf_launched("wf_interp");
    }
    // this flow's conditioning (cond_precomputed models), upsampled once for all rows and layers
    int flow_cond(int k) const {
        if (!p.precond) return CTTS_OK;
        const int rows2c = 2 * p.C, nl = p.c.n_layers;
        const bool vec = g.pad % 4 == 0 && g.ld % 4 == 0 && w.cond_slot % 4 == 0 && !tuning().wf_no_vec_interp;
        const auto kernel = vec ? wf_interp_cond_vec_kernel : wf_interp_cond_kernel;                // a thread per 4 columns | per column
        hipLaunchKernelGGL(kernel, dim3(((vec ? (g.L + 3) / 4 : g.L) + 255) / 256, rows2c * nl, batch), dim3(256), 0, s,
                           cond + (size_t)k * batch * rows2c * nl * cond_ld, w.cond_up, rows2c, nl, frames, cond_ld, cond_pad, g.L, g.ld,
                           g.pad, w.cond_slot);
        return wf_launched("wf_interp_cond");
    }
    // mixing of flow k on the active rows, either direction: PermuteHeight composes into the map, the 1x1 conv is a pass over the
    // rows with W (the inverse's packed W^-1, or W_k of the forward blob)
    int mix(int k, const float* W) {
        if (p.c.mixing == CTTS_MIX_PERMUTE) { rows.permute(k); return CTTS_OK; }
        hipLaunchKernelGGL(wf_mix_kernel, lgrid(), dim3(256), 0, s, w.rows, W, rows.device(), rows.n, p.c.n_group, g.Lr);
        return wf_launched("wf_mix");
    }
    // the start conv of physical row `row` into ring slot `slot` of layer 0
    int start(const WfPlan::Flow& f, int row, int slot) const {
        hipLaunchKernelGGL(wf_start_kernel, dim3(((g.L + 3) / 4 + 255) / 256, (p.C + 15) / 16, batch), dim3(256), 0, s, w.rows,
                           blob + f.start_w, blob + f.start_b, X(0, slot), p.C, p.c.n_group, row, g.L, g.Lr, g.ld, g.pad);
        return wf_launched("wf_start");
    }
    int nan_to_zero() const {
        const size_t n4 = (size_t)batch * p.c.n_group * g.Lr / 4;
        hipLaunchKernelGGL(wf_nan_to_zero_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, w.rows, n4);
        return wf_launched("wf_nan_to_zero");
    }
    int unsqueeze(float* out, const WfRowMap& map) const {
        hipLaunchKernelGGL(wf_unsqueeze_kernel, dim3((g.L + 255) / 256, batch), dim3(256), 0, s, w.rows, out, p.c.n_group, g.L, g.Lr,
                           map.device());
        return wf_launched("wf_unsqueeze");
    }
    // The in-layer GEMM of flow f, WN row r, layer i - the ONE place its descriptor is made, for every launch form: header, K
    // segments (the dense height x width taps from a_min on, or the depthwise stage's output), conditioning (the upsampled addend, or
    // the mel segment of the folded cond layer) and nseg.  The destinations are the caller's (res_skip, or the gated activations).
    // mark_fresh: 0 no marks (per-layer launches, all-rows form), 1 what the previous layer of the SAME row wrote (row queue, one
    // launch per row), 2 every X segment (whole-flow queue: earlier rows were written inside the same launch too)
    GemmArgs in_gemm(const WfPlan::Flow& f, int r, int i, int mark_fresh) const {
        const int kh = p.c.kernel_size_h, kw = p.c.kernel_size_w;
        GemmArgs a{};
        a.gate = p.c.gated_unit;
        a.gemm_mode = p.c.f32_gemm_mode;
        a.bm = WF_BM;
        a.ld = g.ld; a.pad = g.pad; a.L = g.L; a.ntiles = g.ntiles; a.batch = batch;
        a.dst_ld = g.ld; a.dst_pad = g.pad;
        a.A = blob + f.in_A[i]; a.bias = blob + f.in_b[i];
        a.a_nch_alloc = p.nch_in;
        a.MB = p.in_mb(); a.M = 2 * p.C; a.pairC = p.C;
        int ns = 0;
        if (p.sep) {
            a.seg[ns++] = {w.dwout, cstride(), p.nch_c, 0, 0, 0};
            a.nch_total = p.nch_c;
        } else {
            const int si = p.src(i), dh = p.dh(i), dw = p.dw(i), a_min = p.a_min(r, i);
            a.a_ch_off = a_min * kw * p.nch_c;
            for (int ah = a_min; ah < kh; ++ah) {
                const int src_row = r - (kh - 1 - ah) * dh;
                // the current row's slot of layer i > 0 is what layer i - 1 of this very row wrote
                const int fresh = mark_fresh == 2 || (mark_fresh == 1 && src_row == r && si > 0) ? 1 : 0;
                for (int j = 0; j < kw; ++j) a.seg[ns++] = {XR(si, src_row), cstride(), p.nch_c, (j - kw / 2) * dw, 0, fresh};
            }
            a.nch_total = (kh - a_min) * kw * p.nch_c;
        }
        if (p.precond) {
            a.addend = w.cond_up + (size_t)i * w.cond_slot;
            a.addend_bstride = (long long)2 * p.C * g.ld;
        } else {
            a.seg[ns++] = {w.mel_up, (long long)p.kmel * g.ld, p.kmel / GEMM_KC, 0, 0, 0};
            a.nch_total += p.kmel / GEMM_KC;
        }
        a.nseg = ns;
        return a;
    }
    // Where the res/skip GEMM of row r, layer i goes: x_{i+1}[row r] = x_i[row r] + res -> layer i + 1's input of the row (its ring
    // slot: its queue entry); skip rows (+)= into the row's skip sum.  fused: the GEMM is the in-layer launch's epilogue
    // (GEMM_EPI_GATE_RS, transposed weights); else a launch of its own (GEMM_EPI_SPLIT).
    void res_skip(GemmArgs& a, const WfPlan::Flow& f, int r, int i, bool fused) const {
        if (fused) { a.rs_wT = blob + f.rs_T[i]; a.rs_bias = blob + f.rs_Tb[i]; a.rs_rows = p.rs_rows(i); }
        a.dst0 = p.last(i) ? OUT(r) : XR(i + 1, r); a.dst0_bstride = cstride(); a.acc0 = 1;
        a.src0 = XR(p.src(i), r); a.src0_bstride = cstride();
        a.dst1 = OUT(r); a.dst1_bstride = cstride(); a.acc1 = i > 0 ? 1 : 0;
        a.split = p.last(i) ? 0 : p.C;
    }
    // A fused layer whose tile body is launched without launch_gemm_f32 (row queue, all-rows form): built into the staging buffer,
    // its defaults and checks applied here; max_nseg follows.
    int stage(GemmArgs& a, const WfPlan::Flow& f, int r, int i, int mark_fresh, int& max_nseg, const char* form) const {
        a = in_gemm(f, r, i, mark_fresh);
        res_skip(a, f, r, i, true);
        gemm_apply_defaults(a);
        const int rc = gemm_check_args(GEMM_EPI_GATE_RS, a); if (rc) return rc;
        max_nseg = std::max(max_nseg, a.nseg);
        CTTS_CHECK_ARG(wf_row_persistent_supported(a), "waveflow %s: layer %d not supported by the tile body", form, i);
        return CTTS_OK;
    }
    // depthwise stage of a separable in-layer: the height taps' ring slots -> w.dwout
    int depthwise(const WfPlan::Flow& f, int r, int i) const {
        const int C = p.C, L = g.L, kh = p.c.kernel_size_h, kw = p.c.kernel_size_w, dw = p.dw(i), a_min = p.a_min(r, i);
        const float *wt = blob + f.dw_w[i], *bias = blob + f.dw_b[i];
        WfSlots xs{};
        for (int ah = a_min; ah < kh; ++ah) xs.p[ah] = XR(p.src(i), r - (kh - 1 - ah) * p.dh(i));
        const dim3 vgrid(((L + 3) / 4 + 255) / 256, C, batch);
        const bool vec = g.pad % 4 == 0 && g.ld % 4 == 0 && (dw <= 2 || dw % 4 == 0);
        if (vec && kw == 7) launch_depthwise_vec<7>(vgrid, s, xs, wt, bias, w.dwout, C, kh, dw, a_min, L, g.ld, g.pad);
        else if (vec && kw == 5) launch_depthwise_vec<5>(vgrid, s, xs, wt, bias, w.dwout, C, kh, dw, a_min, L, g.ld, g.pad);
        else if (vec && kw == 3) launch_depthwise_vec<3>(vgrid, s, xs, wt, bias, w.dwout, C, kh, dw, a_min, L, g.ld, g.pad);
        else
            hipLaunchKernelGGL(wf_depthwise_kernel, dim3((L + 255) / 256, C, batch), dim3(256), 0, s, xs, wt, bias, w.dwout, C, kh, kw,
                               dw, a_min, L, g.ld, g.pad);
        return wf_launched("wf_depthwise");
    }
    // both 1x1 stages behind the depthwise stage in one launch (waveflow_sep.hip)
    int sep_layer(const WfPlan::Flow& f, int r, int i) const {
        WfSepArgs q{};
        q.dwout = w.dwout;
        q.A1 = blob + f.sA1[i]; q.b1 = blob + f.sb1[i]; q.A2 = blob + f.sA2[i]; q.b2 = blob + f.sb2[i];
        q.cond = w.cond_up + (size_t)i * w.cond_slot;
        q.xin = XR(p.src(i), r);
        q.xout = p.last(i) ? nullptr : XR(i + 1, r);
        q.gate = p.c.gated_unit;
        q.split_bf16 = gemm_split_level(p.c.f32_gemm_mode) == 3 ? 1 : 0;   // (x6: the fused separable layer stays on fp32 MFMA)
        q.out = w.out; q.acc_out = i > 0 ? 1 : 0; q.rs_rows = p.rs_rows(i);
        q.L = g.L; q.ld = g.ld; q.pad = g.pad; q.ntiles = (g.L + 63) / 64;
        const int rc = launch_wf_sep_layer(q, batch, s); if (rc) return rc;
        note_gemm_loop(q.split_bf16 ? 3 : 0);
        return CTTS_OK;
    }
    // one row of the recurrence as one launch per layer (per-layer GEMM shapes, region split, separable / unfused forms)
    int per_layer_row(const WfPlan::Flow& f, int r) {
        int rc = CTTS_OK;
        if (rsplit.on && (rc = rsplit.begin_row(s))) return rc;
        for (int i = 0; i < p.c.n_layers; ++i) {
            if (p.sep && (rc = depthwise(f, r, i))) return rc;
            if (sep_fuse) {
                rc = sep_layer(f, r, i);
            } else if (fuse) {
                GemmArgs a = in_gemm(f, r, i, 0);
                res_skip(a, f, r, i, true);
                rc = rsplit.on ? rsplit.layer(a, i, s) : launch_gemm_f32(GEMM_EPI_GATE_RS, a, s);
            } else {                                        // gated activations -> w.act, then the res/skip 1x1 over them
                GemmArgs a = in_gemm(f, r, i, 0), q{};
                a.dst0 = w.act; a.dst0_bstride = cstride();
                if ((rc = launch_gemm_f32(GEMM_EPI_GATE, a, s))) return rc;
                q.gemm_mode = p.c.f32_gemm_mode;
                q.bm = WF_BM;
                q.ld = g.ld; q.pad = g.pad; q.L = g.L; q.ntiles = g.ntiles; q.batch = batch;
                q.dst_ld = g.ld; q.dst_pad = g.pad;
                q.A = blob + f.rs_A[i]; q.bias = blob + f.rs_b[i];
                q.nseg = 1; q.nch_total = p.nch_c; q.MB = p.rs_mb(i); q.M = p.rs_rows(i);
                q.seg[0] = {w.act, cstride(), p.nch_c, 0, 0, 0};
                res_skip(q, f, r, i, false);
                rc = launch_gemm_f32(GEMM_EPI_SPLIT, q, s);
            }
            if (rc) return rc;
        }
        if (rsplit.on && (rc = rsplit.end_row(s))) return rc;
        return CTTS_OK;
    }
};

// Row queue (round 4, gemm_f32_small.hip wf_row_persistent_kernel), inverse only: the fused layers of a row as ONE launch whose
// workgroups take (layer, tile) items in order and wait for the three neighbouring tiles of the previous layer only.  Same tile body
// as the per-layer 128 x 128 shape: bit-identical to it (and to the 128 x 256 shape).  Descriptors: the GemmArgs of a whole flow are
// built on the host, copied once per flow, and a row's launch points at its slice.
struct WfRowQueue {
    bool on = false, flow = false; // flow: the whole-flow form - every row of a flow in ONE launch (tail stages between the rows)
    int body = 0, max_nseg = 0;    // tile body; widest descriptor of the flow staged last
    unsigned int n_launch = 0;
    size_t host_off = 0;           // bytes of the pinned host buffer the flows queued so far occupy
    // the call's decisions; when on, the pinned buffer is taken and the control words are zeroed
    int begin(const WfCall& c) {
        const WfPlan& p = c.p;
        const auto& t = tuning();
        const int items = wf_row_tiles(c.g.L, 0) * c.batch;
        const int min_items = t.wf_row_queue_min >= 0 ? t.wf_row_queue_min : WF_ROW_QUEUE_MIN_ITEMS;
        // (the queue's tile bodies are the fp32-MFMA DMA-staged ones: under the split-bf16 modes, CTTS_F32_NO_GLDS or CTTS_F32_NO_SMALL
        // the layers are launched one by one as before)
        on = c.fuse && !p.sep && !t.wf_no_row_queue && items >= min_items && (items < WF_ROW_QUEUE_MAX_ITEMS || t.wf_row_queue_min >= 0) &&
             !gemm_mode_is_split(p.c.f32_gemm_mode) && !t.f32_no_glds && !t.f32_no_small;
        if (!t.f32_no_splitk) body = items < WF_ROW_QUEUE_SPLITK_BELOW ? 1 : 0;
        if (t.wf_queue_debug & 16) body = 0;
        if (t.wf_queue_debug & 32) body = 1;
        for (int i = 0; i < p.c.n_layers && on; ++i)        // a fresh segment may reach one 128-column tile to either side
            on = (p.c.kernel_size_w / 2) * p.dw(i) <= 128;
        flow = on && !(t.wf_queue_debug & 128);              // CTTS_WF_QUEUE_DEBUG=128: one launch per row
        if (!on) return CTTS_OK;
        const int rc = t_wf_desc.begin((size_t)p.c.n_flows * p.c.n_group * (p.c.n_layers * sizeof(GemmArgs) + sizeof(WfTailDesc)));
        if (rc) return rc;
        CTTS_CHECK_HIP(hipMemsetAsync(c.w.q.abort_word, 0, c.w.q.control_bytes, c.s));
        if (t.wf_inject_abort) CTTS_CHECK_HIP(hipMemsetAsync(c.w.q.abort_word, 1, sizeof(unsigned int), c.s));   // (tests)
        return CTTS_OK;
    }
    // this flow's descriptors - and, in the whole-flow form, the tail stage behind every row - one copy each
    int stage_flow(const WfCall& c, const WfPlan::Flow& f) {
        const WfPlan& p = c.p;
        const int nr = c.rows.n - 1;
        GemmArgs* host = reinterpret_cast<GemmArgs*>(t_wf_desc.host + host_off);
        size_t n = 0;
        max_nseg = 0;
        for (int r = 0; r < nr; ++r)
            for (int i = 0; i < p.c.n_layers; ++i)
                if (const int rc = c.stage(host[n++], f, r, i, flow ? 2 : 1, max_nseg, "row queue")) return rc;
        CTTS_CHECK_HIP(hipMemcpyAsync(c.w.q.layers, host, n * sizeof(GemmArgs), hipMemcpyHostToDevice, c.s));
        host_off += n * sizeof(GemmArgs);
        if (!flow) return CTTS_OK;
        WfTailDesc* th = reinterpret_cast<WfTailDesc*>(t_wf_desc.host + host_off);
        for (int r = 0; r < nr; ++r) {
            WfTailDesc d{};
            d.out = c.w.out; d.out_bstride = c.cstride();
            d.rows = c.w.rows; d.Wend = c.blob + f.end_w; d.bend = c.blob + f.end_b;
            d.ws = c.blob + f.start_w; d.bs = c.blob + f.start_b;
            d.x0 = r + 1 < nr ? c.X(0, (r + 1) % p.ring) : nullptr; d.x0_bstride = c.cstride();
            d.C = p.C; d.G = p.c.n_group; d.row = c.rows.phys[r + 1]; d.L = c.g.L; d.Lr = c.g.Lr; d.ld = c.g.ld; d.pad = c.g.pad;
            th[r] = d;
        }
        CTTS_CHECK_HIP(hipMemcpyAsync(c.w.q.tails, th, (size_t)nr * sizeof(WfTailDesc), hipMemcpyHostToDevice, c.s));
        host_off += (size_t)nr * sizeof(WfTailDesc);
        return CTTS_OK;
    }
    // rows r0 .. r0 + nrows - 1 of the staged flow as one launch (whole-flow form: all of them, with the tail stages)
    int launch(const WfCall& c, int r0, int nrows) {
        const unsigned int li = n_launch++;
        const WfQueueWs& q = c.w.q;
        return launch_wf_row_persistent(q.layers + (size_t)r0 * c.p.c.n_layers, flow ? q.tails : nullptr, nrows, c.p.c.n_layers, max_nseg,
                                        c.g.L, c.batch, body, q.counters + li, q.flags, q.abort_word, li + 1, c.s);
    }
    // behind the call's last kernel: release the pinned buffer; a bounded wait of the row queue expired (never, by construction):
    // the audio is NaN, not plausible noise, and this thread's next call on this workspace looks at the status first
    int end(const WfCall& c, float* audio, const void* workspace) {
        int rc = t_wf_desc.end(c.s); if (rc) return rc;
        hipLaunchKernelGGL(wf_abort_poison_kernel, dim3(c.batch), dim3(256), 0, c.s, c.w.q.abort_word, audio,
                           (long long)c.p.c.n_group * c.g.L, c.w.q.status);
        CTTS_CHECK_LAUNCH("wf_abort_poison");
        return wf_note_pending(workspace, c.w.q.status, c.s);
    }
};

// z -> audio (ctts_waveflow_inverse_*, ax:309-346): flows in reverse order, each the row recurrence in the row queue or as per-layer
// launches; the earlier chunks of an early-output model re-join in front, one per n_early_every flows (ax:340-341)
int wf_synthesize(const WfIo& io) {
    WfCall c;
    int rc = c.open(io, nullptr); if (rc) return rc;
    // the previous call of this thread on this workspace used the row queue: if it aborted, say so now instead of computing
    // on top of it (one stream synchronisation + 4 bytes; the caller sees CTTS_E_ABORT once, the call after that runs)
    if ((rc = wf_check_pending(io.workspace, c.w.q.status, c.s))) return rc;
    const WfPlan& p = c.p;
    const int G = p.c.n_group;
    if ((rc = c.squeeze(io.in, nullptr))) return rc;
    c.rows.reset(G, p.n_rem[p.c.n_flows - 1]);
    WfRowQueue q;
    if ((rc = q.begin(c))) return rc;
    for (int k = p.c.n_flows - 1; k >= 0; --k) {
        const auto& f = p.fl[k];
        if (!p.c.mix_first && (rc = c.mix(k, c.blob + f.winv))) return rc;     // ax:324-325
        const int nr = c.rows.n - 1;                                           // WN rows 0 .. n - 2 (efficient_modules.py:42-65)
        if (q.on && (rc = q.stage_flow(c, f))) return rc;
        if ((rc = c.flow_cond(k))) return rc;
        if (q.flow) {                                       // start of row 0, then every row and tail of the flow in one launch
            if ((rc = c.start(f, c.rows.phys[0], 0))) return rc;
            if ((rc = q.launch(c, 0, nr))) return rc;
        }
        for (int r = 0; r < nr && !q.flow; ++r) {
            if ((rc = c.start(f, c.rows.phys[r], r % p.ring))) return rc;
            if ((rc = q.on ? q.launch(c, r, 1) : c.per_layer_row(f, r))) return rc;
            hipLaunchKernelGGL(wf_tail_kernel, c.lgrid(), dim3(256), 0, c.s, c.w.out, c.w.rows, c.blob + f.end_w, c.blob + f.end_b, p.C, G,
                               c.rows.phys[r + 1], c.g.L, c.g.Lr, c.g.ld, c.g.pad);
            CTTS_CHECK_LAUNCH("wf_tail");
        }
        if ((rc = c.nan_to_zero())) return rc;
        if (p.c.mix_first && (rc = c.mix(k, c.blob + f.winv))) return rc;      // ax:337-338
        if (k > 0 && p.n_rem[k - 1] > c.rows.n) c.rows.rejoin_front(p.n_rem[k - 1] - c.rows.n, G);
    }
    if ((rc = c.unsqueeze(io.out, c.rows))) return rc;
    return q.on ? q.end(c, io.out, io.workspace) : CTTS_OK;
}

// ---- analysis direction (ax:234-277) -------------------------------------------------------------------------------------------
// end conv + affine update + log_s of WN rows r0 .. r0 + nrows - 1 from the skip sums at `out` (rstride apart)
int wf_fwd_tail(const WfCall& c, const WfPlan::Flow& f, const RowMap& m, const float* out, size_t rstride, int r0, int nrows) {
    hipLaunchKernelGGL(wf_fwd_tail_kernel, dim3((c.g.Lr + 255) / 256, c.batch, nrows), dim3(256), 0, c.s, out, rstride, c.w.rows, c.w.f.ls,
                       c.blob + f.end_w, c.blob + f.end_b, m, r0, c.p.C, c.p.c.n_group, c.g.L, c.g.Lr, c.g.ld, c.g.pad);
    return wf_launched("wf_fwd_tail");
}

// All-rows form: the descriptors of the whole call - [flow][layer][row], independent of the row map - staged in the calling thread's
// pinned buffer and copied once.  off[k]: first descriptor of flow k.
int wf_stage_all_rows(const WfCall& c, std::vector<size_t>& off, int& max_nseg) {
    const WfPlan& p = c.p;
    for (int k = 0; k < p.c.n_flows; ++k) off[k + 1] = off[k] + (size_t)p.c.n_layers * (p.n_rem[k] - 1);
    if (const int rc = t_wf_desc.begin(off[p.c.n_flows] * sizeof(GemmArgs))) return rc;
    GemmArgs* host = reinterpret_cast<GemmArgs*>(t_wf_desc.host);
    for (int k = 0; k < p.c.n_flows; ++k)
        for (int i = 0; i < p.c.n_layers; ++i)
            for (int r = 0; r < p.n_rem[k] - 1; ++r)
                if (const int rc = c.stage(host[off[k] + (size_t)i * (p.n_rem[k] - 1) + r], p.fl[k], r, i, 0, max_nseg, "forward")) return rc;
    CTTS_CHECK_HIP(hipMemcpyAsync(c.w.f.desc, host, off[p.c.n_flows] * sizeof(GemmArgs), hipMemcpyHostToDevice, c.s));
    return t_wf_desc.end(c.s);
}

// the coupling of one flow, all-rows form: the start conv of every row, one launch per layer, the tail over all rows
int wf_all_rows_flow(const WfCall& c, const WfPlan::Flow& f, const RowMap& m, int nr, const GemmArgs* desc, int max_nseg) {
    const WfGeom& g = c.g;
    hipLaunchKernelGGL(wf_fwd_start_rows_kernel, dim3(((g.L + 3) / 4 + 255) / 256, (c.p.C + 15) / 16, (unsigned)(nr * c.batch)), dim3(256),
                       0, c.s, c.w.rows, c.blob + f.start_w, c.blob + f.start_b, c.w.f.XA, c.w.xslot, m, c.p.C, c.p.c.n_group, c.batch, g.L,
                       g.Lr, g.ld, g.pad);
    CTTS_CHECK_LAUNCH("wf_fwd_start_rows");
    for (int i = 0; i < c.p.c.n_layers; ++i)
        if (const int rc = launch_wf_all_rows_layer(desc + (size_t)i * nr, nr, max_nseg, g.L, c.batch, c.s)) return rc;
    return wf_fwd_tail(c, f, m, c.w.f.OUT, c.w.xslot, 0, nr);
}

// Row-wise form: the inverse's launches in natural row order on the ring; the row's input is the known audio row, so the next row's
// start conv runs BEFORE this row's tail overwrites it (its ring slot is free: this row's layers are queued)
int wf_row_wise_flow(WfCall& c, const WfPlan::Flow& f, const RowMap& m, int nr) {
    int rc = c.start(f, c.rows.phys[0], 0); if (rc) return rc;
    for (int r = 0; r < nr; ++r) {
        if ((rc = c.per_layer_row(f, r))) return rc;
        if (r + 1 < nr && (rc = c.start(f, c.rows.phys[r + 1], (r + 1) % c.p.ring))) return rc;
        if ((rc = wf_fwd_tail(c, f, m, c.w.out, 0, r, 1))) return rc;
    }
    return CTTS_OK;
}

// audio -> z, log_s, log-likelihood sums (ctts_waveflow_forward_*): flows in natural order; the mix is the same row-map composition
// or the same pass over the rows with W_k; an early split peels the first n_early_size active rows off to the output (ax:237-242)
int wf_analyze(const WfIo& io, const WfForward& fw) {
    WfCall c;
    int rc = c.open(io, &fw); if (rc) return rc;
    const WfPlan& p = c.p;
    const WfWs& w = c.w;
    const int G = p.c.n_group, L = c.g.L, batch = c.batch;
    if ((rc = c.squeeze(io.in, &fw))) return rc;
    c.rows.reset(G, G);
    WfRowMap out;                                            // the latent's rows in output order: early outputs first
    int s_off = 0, S = 0, d_max_nseg = 0;
    for (int k = 0; k < p.c.n_flows; ++k) S += p.n_rem[k] - 1;
    std::vector<size_t> d_off(p.c.n_flows + 1, 0);
    if (c.all_rows && (rc = wf_stage_all_rows(c, d_off, d_max_nseg))) return rc;
    for (int k = 0; k < p.c.n_flows; ++k) {
        const auto& f = p.fl[k];
        const float* W = fw.mix + wf_fwd_mix_offset(p, k);
        if (p.n_rem[k] < c.rows.n) c.rows.peel_front(c.rows.n - p.n_rem[k], out);
        if (p.c.mix_first && (rc = c.mix(k, W))) return rc;                    // ax:244-245
        if ((rc = c.flow_cond(k))) return rc;
        const int nr = c.rows.n - 1;                                           // WN rows 0 .. n - 2 (efficient_modules.py:30)
        const RowMap m = c.rows.device();
        if ((rc = c.all_rows ? wf_all_rows_flow(c, f, m, nr, w.f.desc + d_off[k], d_max_nseg) : wf_row_wise_flow(c, f, m, nr))) return rc;
        hipLaunchKernelGGL(wf_fwd_reduce_kernel, dim3(w.f.nblk, batch), dim3(256), 0, c.s, w.f.ls, nr, G, L, c.g.Lr, fw.log_s, S, s_off,
                           fw.log_s_sum, k == 0 ? 1 : 0, w.f.partials + (size_t)k * batch * w.f.nblk, w.f.nblk);
        CTTS_CHECK_LAUNCH("wf_fwd_reduce");
        s_off += nr;
        if (fw.ignore_nan && (rc = c.nan_to_zero())) return rc;
        if (!p.c.mix_first && (rc = c.mix(k, W))) return rc;                   // ax:260-261
    }
    c.rows.peel_front(c.rows.n, out);                                          // ax:276-277
    if ((rc = c.unsqueeze(io.out, out))) return rc;
    hipLaunchKernelGGL(wf_fwd_sums_kernel, dim3((p.c.n_flows * batch + 63) / 64), dim3(64), 0, c.s, w.f.partials, fw.sums, p.c.n_flows,
                       batch, w.f.nblk);
    return wf_launched("wf_fwd_sums");
}

}  // namespace

extern "C" {

size_t ctts_waveflow_packed_bytes(const ctts_waveflow_config* cfg) {
    WfPlan p;
    if (make_wf_plan(cfg, p)) return 0;
    return p.total * sizeof(float);
}

int ctts_waveflow_pack_flow(const ctts_waveflow_config* cfg, int32_t k, const ctts_waveflow_flow_weights* w,
                            void* packed, void* stream) {
    WfPlan p;
    int rc = make_wf_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(k >= 0 && k < p.c.n_flows && w && packed, "waveflow pack_flow: bad argument");
    CTTS_CHECK_ARG(w->start_w && w->start_b && w->in_w && w->in_b && w->rs_w && w->rs_b && w->end_w && w->end_b,
                   "waveflow pack_flow: NULL weight pointer");
    CTTS_CHECK_ARG(p.precond || (w->cond_w && w->cond_b), "waveflow pack_flow: NULL cond layer");
    CTTS_CHECK_ARG(!p.sep || (w->dw_w && w->dw_b), "waveflow pack_flow: NULL depthwise weights");
    hipStream_t s = as_stream(stream);
    float* blob = static_cast<float*>(packed);
    const auto& f = p.fl[k];
    const int C = p.C, kh = p.c.kernel_size_h, kw = p.c.kernel_size_w, nm = p.c.n_mel_channels;
    const int gkh = p.sep ? 1 : kh, gkw = p.sep ? 1 : kw;      // taps of the GEMM stage
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.start_w, w->start_w, C * sizeof(float), hipMemcpyDeviceToDevice, s));
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.start_b, w->start_b, C * sizeof(float), hipMemcpyDeviceToDevice, s));
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.end_w, w->end_w, 2 * C * sizeof(float), hipMemcpyDeviceToDevice, s));
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.end_b, w->end_b, 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (p.c.mixing == CTTS_MIX_CONV1X1) {
        CTTS_CHECK_ARG(w->w_inverse != nullptr, "waveflow pack_flow: 1x1-conv mixing needs w_inverse (flow %d)", k);
        CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.winv, w->w_inverse, (size_t)p.n_rem[k] * p.n_rem[k] * sizeof(float),
                                      hipMemcpyDeviceToDevice, s));
    }
    for (int i = 0; i < p.c.n_layers; ++i) {
        CTTS_CHECK_ARG(w->in_w[i] && w->in_b[i] && w->rs_w[i] && w->rs_b[i], "waveflow pack_flow: NULL layer %d", i);
        CTTS_CHECK_HIP(hipMemsetAsync(blob + f.in_A[i], 0, (size_t)p.in_mb() * p.nch_in * GEMM_KC * WF_BM * sizeof(float), s));
        // K = [height tap a][width tap j][channel] then the cond rows;  in_w[i] is [2C][C][gkh][gkw]
        for (int a = 0; a < gkh; ++a)
            for (int j = 0; j < gkw; ++j)
                if ((rc = launch_pack_a(blob + f.in_A[i], w->in_w[i] + a * gkw + j, WF_BM, p.in_mb(), p.nch_in,
                                        (a * gkw + j) * C, C, GEMM_EPI_GATE, C, 2 * C, 0, (long long)C * gkh * gkw,
                                        gkh * gkw, s))) return rc;
        if (!p.precond)
            if ((rc = launch_pack_a(blob + f.in_A[i], w->cond_w, WF_BM, p.in_mb(), p.nch_in, gkh * gkw * C, nm,
                                    GEMM_EPI_GATE, C, 2 * C, (long long)2 * C * i, nm, 1, s))) return rc;
        if ((rc = launch_pack_bias(blob + f.in_b[i], WF_BM, p.in_mb(), w->in_b[i], 0, p.precond ? nullptr : w->cond_b,
                                   (long long)2 * C * i, GEMM_EPI_GATE, C, 2 * C, s))) return rc;
        if (p.sep) {
            CTTS_CHECK_ARG(w->dw_w[i] && w->dw_b[i], "waveflow pack_flow: NULL depthwise layer %d", i);
            CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.dw_w[i], w->dw_w[i], (size_t)C * kh * kw * sizeof(float),
                                          hipMemcpyDeviceToDevice, s));
            CTTS_CHECK_HIP(hipMemcpyAsync(blob + f.dw_b[i], w->dw_b[i], C * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        const int rows = p.rs_rows(i);
        if ((rc = launch_pack_a(blob + f.rs_A[i], w->rs_w[i], WF_BM, p.rs_mb(i), p.nch_c, 0, C, GEMM_EPI_SPLIT, C, rows,
                                0, C, 1, s))) return rc;
        if ((rc = launch_pack_bias(blob + f.rs_b[i], WF_BM, p.rs_mb(i), w->rs_b[i], 0, nullptr, 0, GEMM_EPI_SPLIT, C,
                                   rows, s))) return rc;
        if (p.fused()) {
            hipLaunchKernelGGL(wf_pack_rs_t_kernel, dim3(33), dim3(256), 0, s, w->rs_w[i], w->rs_b[i], blob + f.rs_T[i],
                               blob + f.rs_Tb[i], rows);
            CTTS_CHECK_LAUNCH("wf_pack_rs_t");
        }
        if (p.sep_fused())
            if ((rc = launch_wf_sep_pack(w->in_w[i], w->in_b[i], w->rs_w[i], w->rs_b[i], blob + f.sA1[i], blob + f.sb1[i],
                                         blob + f.sA2[i], blob + f.sb2[i], rows, s))) return rc;
    }
    return CTTS_OK;
}

size_t ctts_waveflow_workspace_bytes(const ctts_waveflow_config* cfg, int32_t batch, int32_t samples) {
    WfPlan p; WfGeom g; WfWs w;
    if (make_wf_plan(cfg, p) || make_wf_geom(p, samples, g) || batch < 1) return 0;
    wf_carve(p, g, batch, nullptr, w);
    return w.total * sizeof(float);
}

int ctts_waveflow_inverse_f32(const ctts_waveflow_config* cfg, const void* packed, const float* z, const float* mel,
                              float* audio, int32_t batch, int32_t samples, int32_t frames, void* workspace,
                              size_t workspace_bytes, void* stream) {
    CTTS_CHECK_ARG(cfg && !cfg->cond_precomputed, "waveflow inverse: this model takes per-flow conditioning "
                                                  "(ctts_waveflow_inverse_cond_f32)");
    return wf_synthesize({cfg, packed, z, mel, 0, 0, audio, batch, samples, frames, workspace, workspace_bytes, stream});
}

size_t ctts_waveflow_forward_packed_bytes(const ctts_waveflow_config* cfg) {
    WfPlan p;
    if (make_wf_plan(cfg, p)) return 0;
    return wf_fwd_mix_offset(p, p.c.n_flows) * sizeof(float);
}

int ctts_waveflow_pack_forward_mix(const ctts_waveflow_config* cfg, int32_t k, const float* W_k, void* fwd_blob, void* stream) {
    WfPlan p;
    int rc = make_wf_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(k >= 0 && k < p.c.n_flows, "waveflow pack_forward_mix: flow %d", k);
    if (p.c.mixing != CTTS_MIX_CONV1X1) return CTTS_OK;                        // PermuteHeight is its own inverse: nothing to hold
    CTTS_CHECK_ARG(W_k && fwd_blob, "waveflow pack_forward_mix: NULL argument");
    CTTS_CHECK_HIP(hipMemcpyAsync(static_cast<float*>(fwd_blob) + wf_fwd_mix_offset(p, k), W_k,
                                  (size_t)p.n_rem[k] * p.n_rem[k] * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return CTTS_OK;
}

size_t ctts_waveflow_forward_workspace_bytes(const ctts_waveflow_config* cfg, int32_t batch, int32_t samples) {
    WfPlan p; WfGeom g; WfWs w;
    if (make_wf_plan(cfg, p) || make_wf_geom(p, samples, g) || batch < 1) return 0;
    wf_carve(p, g, batch, nullptr, w, true);
    return w.total * sizeof(float);
}

int ctts_waveflow_forward_f32(const ctts_waveflow_config* cfg, const void* packed, const void* fwd_blob, const float* audio,
                              const float* mel, float preemphasis, int32_t ignore_nan, float* z, float* log_s, float* log_s_sum,
                              double* sums, int32_t batch, int32_t samples, int32_t frames, void* workspace,
                              size_t workspace_bytes, void* stream) {
    CTTS_CHECK_ARG(cfg && !cfg->cond_precomputed, "waveflow forward: this model takes per-flow conditioning "
                                                  "(ctts_waveflow_forward_cond_f32)");
    const WfForward fw{static_cast<const float*>(fwd_blob), preemphasis, ignore_nan, log_s, log_s_sum, sums};
    return wf_analyze({cfg, packed, audio, mel, 0, 0, z, batch, samples, frames, workspace, workspace_bytes, stream}, fw);
}

int ctts_waveflow_forward_cond_f32(const ctts_waveflow_config* cfg, const void* packed, const void* fwd_blob, const float* audio,
                                   const float* cond, int32_t cond_ld, int32_t cond_pad, float preemphasis, int32_t ignore_nan,
                                   float* z, float* log_s, float* log_s_sum, double* sums, int32_t batch, int32_t samples,
                                   int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    CTTS_CHECK_ARG(cfg && cfg->cond_precomputed, "waveflow forward_cond: the model folds its cond layer "
                                                 "(ctts_waveflow_forward_f32)");
    CTTS_CHECK_ARG(cond_pad >= 0 && cond_ld >= cond_pad + frames, "waveflow forward_cond: cond_ld=%d pad=%d frames=%d",
                   cond_ld, cond_pad, frames);
    const WfForward fw{static_cast<const float*>(fwd_blob), preemphasis, ignore_nan, log_s, log_s_sum, sums};
    return wf_analyze({cfg, packed, audio, cond, cond_ld, cond_pad, z, batch, samples, frames, workspace, workspace_bytes, stream}, fw);
}

int ctts_waveflow_abort_status(const ctts_waveflow_config* cfg, int32_t batch, int32_t samples, void* workspace,
                               size_t workspace_bytes, void* stream) {
    WfPlan p; WfGeom g; WfWs w;
    int rc = make_wf_plan(cfg, p); if (rc) return rc;
    rc = make_wf_geom(p, samples, g); if (rc) return rc;
    CTTS_CHECK_ARG(workspace && batch >= 1, "waveflow abort_status: bad argument");
    wf_carve(p, g, batch, static_cast<float*>(workspace), w);
    if (w.total * sizeof(float) > workspace_bytes) {
        set_error("waveflow abort_status: workspace %zu bytes < required %zu", workspace_bytes, w.total * sizeof(float));
        return CTTS_E_WORKSPACE;
    }
    {   // the pending entry (if this thread has one) carries the event of the call in question; without one the caller's
        // stream is what the call ran on
        auto& pd = t_wf_pending;
        const int i = pd.find(workspace);
        hipEvent_t done = nullptr;
        if (i >= 0) { pd.ws[i] = nullptr; done = pd.ev[i]; }
        return wf_report_abort(w.q.status, done, as_stream(stream));
    }
}

int ctts_waveflow_inverse_cond_f32(const ctts_waveflow_config* cfg, const void* packed, const float* z,
                                   const float* cond, int32_t cond_ld, int32_t cond_pad, float* audio, int32_t batch,
                                   int32_t samples, int32_t frames, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    CTTS_CHECK_ARG(cfg && cfg->cond_precomputed, "waveflow inverse_cond: the model folds its cond layer "
                                                 "(ctts_waveflow_inverse_f32)");
    CTTS_CHECK_ARG(cond_pad >= 0 && cond_ld >= cond_pad + frames, "waveflow inverse_cond: cond_ld=%d pad=%d frames=%d",
                   cond_ld, cond_pad, frames);
    return wf_synthesize({cfg, packed, z, cond, cond_ld, cond_pad, audio, batch, samples, frames, workspace, workspace_bytes, stream});
}

int ctts_embed_rows_f32(const float* table, const int64_t* ids, float* x, int32_t row0, int32_t embed_dim,
                        int32_t batch, int32_t C, int32_t T, int32_t ld, int32_t pad, void* stream) {
    CTTS_CHECK_ARG(table && ids && x && embed_dim >= 1 && row0 >= 0 && row0 + embed_dim <= C && batch >= 1 && T >= 1 &&
                   ld >= pad + T, "embed_rows: bad argument");
    hipLaunchKernelGGL(embed_rows_kernel, dim3((T + 255) / 256, embed_dim, batch), dim3(256), 0, as_stream(stream), table,
                       ids, x, row0, embed_dim, C, T, ld, pad);
    CTTS_CHECK_LAUNCH("embed_rows");
    return CTTS_OK;
}

int ctts_scale_add_rows_f32(const float* x, const float* alpha_dev, const float* r, float* y, int32_t batch, int32_t C,
                            int32_t T, int32_t ld, int32_t pad, void* stream) {
    CTTS_CHECK_ARG(x && y && batch >= 1 && C >= 1 && T >= 1 && ld >= pad + T, "scale_add_rows: bad argument");
    hipLaunchKernelGGL(scale_add_rows_kernel, dim3((T + 255) / 256, C, batch), dim3(256), 0, as_stream(stream), x,
                       alpha_dev, r, y, C, T, ld, pad);
    CTTS_CHECK_LAUNCH("scale_add_rows");
    return CTTS_OK;
}

int ctts_affine_rows_f32(float* x, int32_t batch, int32_t C, int32_t rows, int32_t T, int32_t ld, int32_t pad, float shift,
                         float scale, void* stream) {
    CTTS_CHECK_ARG(x && batch >= 1 && rows >= 1 && rows <= C && T >= 1 && ld >= pad + T, "affine_rows: bad argument");
    hipLaunchKernelGGL(affine_rows_kernel, dim3((T + 255) / 256, rows, batch), dim3(256), 0, as_stream(stream), x, C, T, ld,
                       pad, shift, scale);
    CTTS_CHECK_LAUNCH("affine_rows");
    return CTTS_OK;
}

int ctts_resample_rows_f32(const float* x, float* y, int32_t batch, int32_t C, int32_t T_in, int32_t ld_in, int32_t pad_in,
                           int32_t T_out, int32_t ld_out, int32_t pad_out, int32_t mode, float scale_factor, void* stream) {
    CTTS_CHECK_ARG(x && y && batch >= 1 && C >= 1 && T_in >= 1 && T_out >= 1 && ld_in >= pad_in + T_in &&
                   ld_out >= pad_out + T_out && mode >= 0 && mode <= 2, "resample_rows: bad argument");
    const float s = scale_factor > 0.f ? 1.0f / scale_factor : (float)T_in / (float)T_out;
    hipLaunchKernelGGL(resample_rows_kernel, dim3((T_out + 255) / 256, C, batch), dim3(256), 0, as_stream(stream), x, y, C,
                       T_in, ld_in, pad_in, T_out, ld_out, pad_out, mode, s);
    CTTS_CHECK_LAUNCH("resample_rows");
    return CTTS_OK;
}

int ctts_interleave_phases_f32(const float* phases, float* y, int32_t batch, int32_t C, int32_t stride, int32_t padding,
                               int32_t T_in, int32_t ld_in, int32_t pad_in, int32_t T_out, int32_t ld_out, int32_t pad_out,
                               void* stream) {
    CTTS_CHECK_ARG(phases && y && batch >= 1 && C >= 1 && stride >= 1 && padding >= 0 && T_in >= 1 && T_out >= 1 &&
                   ld_in >= pad_in + T_in && ld_out >= pad_out + T_out, "interleave_phases: bad argument");
    hipLaunchKernelGGL(interleave_phases_kernel, dim3((T_out + 255) / 256, C, batch), dim3(256), 0, as_stream(stream), phases,
                       y, C, stride, padding, T_in, ld_in, pad_in, T_out, ld_out, pad_out, (size_t)batch * C * ld_in);
    CTTS_CHECK_LAUNCH("interleave_phases");
    return CTTS_OK;
}

int ctts_vol_unscale_f32(float* x, int64_t n, void* stream) {
    CTTS_CHECK_ARG(x && n >= 1, "vol_unscale: bad argument");
    hipLaunchKernelGGL(vol_unscale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, (size_t)n);
    CTTS_CHECK_LAUNCH("vol_unscale");
    return CTTS_OK;
}

int ctts_deemphasis_f32(const float* x, float* y, int32_t batch, int32_t T, double p, void* stream) {
    CTTS_CHECK_ARG(x && y && batch >= 1 && T >= 1, "deemphasis: bad argument");
    hipLaunchKernelGGL(deemphasis_kernel, dim3(batch), dim3(256), 0, as_stream(stream), x, y, T, p);
    CTTS_CHECK_LAUNCH("deemphasis");
    return CTTS_OK;
}

}  // extern "C"
