// Launchers of the non-GEMM WaveGlow kernels (definitions in waveglow_kernels.hip).
#pragma once

#include "common.h"
#include "gemm_f32.h"

namespace ctts {

int launch_fold_weightnorm(const float* v, const float* g, float* w, int out_ch, int fan, hipStream_t s);
int launch_pack_a(float* dst, const float* src, int bm, int MB, int nch_total, int k_off, int ksrc, int epi, int C, int M,
                  long long src_row_off, long long src_row_stride, int src_k_stride, hipStream_t s, int k_group = 1,
                  int k_member = 0);
int launch_pack_bias(float* dst, int bm, int MB, const float* src0, long long off0, const float* src1, long long off1,
                     int epi, int C, int M, hipStream_t s);
// Wp: W in MFMA fragment order (launch_upsample_pack_mfma; only for shapes upsample_mfma_shape accepts) or nullptr = VALU kernels
bool upsample_mfma_shape(int n_mel, int win, int hop, int G);
int launch_upsample_pack_mfma(const float* W, float* Wp, hipStream_t s);
int launch_upsample_squeeze(const float* mel, const float* W, const float* Wp, const float* bias, float* spect, int batch,
                            int n_mel, int F, int win, int hop, int G, int ld, int pad, hipStream_t s);
int launch_wn_start(const float* audio, const float* Ws, const float* bs, float* x, int batch, int C, int G,
                    int ch_off, int n_half, int L, int ld, int pad, hipStream_t s);
// Forward (analysis) direction of a flow boundary, glow.py:305-307: where the tail kernels get one of these they compute
// a_1 = exp(log_s) a_1 + b in place instead of the inverse coupling and mix nothing (the forward mix is the flow's head).
struct CouplingForward {
    float* log_s;             // NULL, or the flow's log_s rows: item b, row j at log_s + b * ls_bstride + j * L
    long long ls_bstride;
    double* part;             // per-workgroup sums of log_s, fp64: item b, 256-column block i at part + b * part_bstride + i
    long long part_bstride;
};
constexpr int FWD_SUMSQ_CHUNK = 4096;     // floats of one item per workgroup of launch_sumsq_partials
int launch_flow_tail(const float* out, float* audio, float* wave, const float* Wend, const float* bend,
                     const float* Winv, int batch, int C, int G, int ch_off, int n_half, int L, int ld, int pad,
                     hipStream_t s, const CouplingForward* fwd = nullptr);
// Head of a forward flow: rows [ch_off, ch_off + n_rem) of z [B][G][L] <- W [n_rem][n_rem] . those rows, in place (glow.py:294).
// wave != NULL (flow 0: ch_off == 0, n_rem == G): the rows are read un-squeezed from wave [B][L*G] instead (glow.py:284).
int launch_flow_head_forward(const float* W, const float* wave, float* z, int batch, int G, int ch_off, int n_rem, int L,
                             hipStream_t s);
// part[b][i] = fp64 sum of squares of floats [i * FWD_SUMSQ_CHUNK, ...) of item b's n_item floats (nblk = ceil(n_item / chunk))
int launch_sumsq_partials(const float* z, double* part, int batch, long long n_item, int nblk, hipStream_t s);
// out[b * out_bstride + k] = sum of the n doubles at part + b * part_bstride + k * part_kstride, always in the same order
int launch_sum_partials(const double* part, long long part_bstride, long long part_kstride, int n, double* out, int out_bstride,
                        int nk, int batch, hipStream_t s);

// WN start / end folds (fp32 WaveGlow): layer 0's in-layer weights on the FOLD_ROWS-row input [audio_0; 1; 0 ...] and the skip rows
// seen through `end` (waveglow_kernels.hip).  Pack time: fp64 products rounded once to fp32.
constexpr int FOLD_ROWS = 16;    // rows of the folded layer-0 input = one K chunk per tap (n_half <= 8 audio rows + the ones row)
int launch_fold_in0(const float* in_w, const float* Ws, const float* bs, float* dst, int C, int n_half, int ks, hipStream_t s);
int launch_fold_skend(const float* const* rs_w, const float* const* rs_b, const float* Wend, const float* bend, float* Wf,
                      float* bf, int C, int n_layers, int n_half, hipStream_t s);
int launch_wn_start_ones(const float* audio, float* a16, int batch, int G, int ch_off, int n_half, int L, int ld, int pad,
                         hipStream_t s);
int launch_skip_end(const float* act, long long act_stride, int nl, const float* Wf, float* acc, bool first, bool tail,
                    const float* bf, const float* Winv, float* audio, float* wave, int batch, int C, int G, int ch_off,
                    int n_half, int L, int ld, int pad, hipStream_t s, const CouplingForward* fwd = nullptr);

// Winograd F(2,3) in-layer form (fp32 WaveGlow; the algebra is at the kernels in waveglow_kernels.hip).  Pack time: dense
// [3][rows][C] = G2, G3, -W2 of in_w [rows][C][3].  Per layer: x and the flow's cond rows -> V1..V4 [4][B][C][ldp] and the copies
// h2e, h2o [2][B][H][ldp] in pair order (Lp pair columns, zeros up to ncols); cond_rows = false: V only (the GATE launches read
// the cond rows in place, GemmArgs.mseg).  vec_d2 = false: d = 2 on the one-column-at-a-time path (CTTS_F32_WINOGRAD_PLAIN).
int launch_winograd_g(const float* in_w, float* dense, int rows, int C, hipStream_t s);
int launch_winograd_transform(const float* x, long long x_bstride, const float* h2, long long h_bstride, float* V, float* Hc,
                              int batch, int C, int H, int d, int L, int Lp, int ld, int pad, int ldp, int ncols, bool cond_rows,
                              bool vec_d2, hipStream_t s);

// Winograd F(4,3) form of the same layers (points 0, +-1, +-2, inf; the algebra is at the kernels).  Pack time: dense [6][rows][C] =
// U0..U5.  Per layer: V0..V5 [6][B][C][ldq] and, with cond_rows, the copies h(t_0)..h(t_3) [4][B][H][ldq] in quad order (Lq quad
// columns, zeros up to ncols).
int launch_winograd_g43(const float* in_w, float* dense, int rows, int C, hipStream_t s);
int launch_winograd_transform_quad(const float* x, long long x_bstride, const float* h2, long long h_bstride, float* V, float* Hc,
                                   int batch, int C, int H, int d, int L, int Lq, int ld, int pad, int ldq, int ncols, bool cond_rows,
                                   hipStream_t s);

// Winograd F(6,3) form of the layers with d % 4 == 0 (points 0, +-1, +-2, +-1/2, inf; the algebra is at the kernels).  Pack time: dense
// [8][rows][C] = U0..U7.  Per layer: V0..V7 [8][B][C][ldh] in hex order (Lh hex columns, zeros up to ncols); the cond rows are read
// in place.
int launch_winograd_g63(const float* in_w, float* dense, int rows, int C, hipStream_t s);
int launch_winograd_transform_hex(const float* x, long long x_bstride, float* V, int batch, int C, int d, int L, int Lh, int ld, int pad,
                                  int ldh, int ncols, hipStream_t s);

}  // namespace ctts
