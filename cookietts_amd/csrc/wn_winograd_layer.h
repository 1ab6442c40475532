// One launch per Winograd F(2,3) in-layer step of the fp32 WaveGlow (wn_winograd_layer.hip): behind the input transform, the four
// products of a pair block
//   S = G2 V2,  D = G3 V3,  (S, D) <- (S + D, S - D),
//   act[t_e] = gate(S + [W0 | C_i] [V1; h(t_e)] + b),   act[t_o] = gate(D + [-W2 | C_i] [V4; h(t_o)] + b)
// run one after the other through ONE chunk stream of a workgroup that owns 128 packed rows (the tanh and the sigmoid rows of 64
// channels) x 128 pair columns; T2 / T3 never leave the registers.  The operands are the panels and planes the lean form
// (waveglow_api.hip, run_in_layer_winograd) already has.
//
// form = WNWG_F43 is the F(4,3) form of the same stream: a workgroup owns 128 packed rows x 64 QUAD columns (256 natural columns);
// quad column q of a batch item stands for the natural columns t_k = (q / d) 4d + q % d + k d, k = 0..3, Lq = ceil(L / 4d) d.
//   P_j = U_j V_j (j = 1..4),  a = P1 + P2, b = P1 - P2, c = P3 + P4, e = P3 - P4,
//   act[t_0] = gate(a + c   + [U0 | C_i] [V0; h(t_0)] + b),   act[t_1] = gate(b + 2 e + C_i h(t_1) + b),
//   act[t_2] = gate(a + 4 c + C_i h(t_2) + b),                act[t_3] = gate(b + 8 e + [U5 | C_i] [V5; h(t_3)] + b)
// with U = G W, V = B^T x of the interpolation points 0, +-1, +-2, inf.  ldp / Lp / ntiles then describe the quad space, in tiles of
// 64 columns.  Three kernels run it, bit-identical like NT = 1 / 2 of the F(2,3) form (every column's products are summed in the same
// order): 64 quad columns with TWO consecutive chunks per stage (32 k-deep stages, half the barriers, the chunk table fetched one
// stage ahead) - what the launcher takes at every size; the same shape with one chunk per stage (CTTS_F32_FORCE_SMALL, the kernel of
// the rounds before); and 128 quad columns = 512 natural columns, whose four accumulator sets are 256 registers: ONE workgroup per CU,
// one wave per SIMD with the whole 512-register file (CTTS_F32_NO_SMALL; slower, profiles/r26_01_f43_wide_gonogo.txt; it needs
// ldp >= 128 ceil(ntiles / 2)).  Two chunks per stage need H % 32 == 0 (C % 128 == 0 holds), so that every phase is whole stages;
// other H keep one chunk per stage.
//
// form = WNWG_F63 is the F(6,3) form: 128 packed rows x 64 HEX columns (384 natural columns); hex column q stands for
// t_k = (q / d) 6d + q % d + k d, k = 0..5, Lh = ceil(L / 6d) d; P_j = U_j V_j (j = 1..6), the six sums of the header of
// wn_winograd_layer.hip, the end products [U0 | C_i] [V0; h(t_0)] and [U7 | C_i] [V7; h(t_5)], and C_i h(t_k) alone for k = 1..4.
// ldp / Lp / ntiles then describe the hex space.  One kernel (64 columns, two chunks per stage); it needs H % 32 == 0 and reads the
// cond rows in place (in_place = 1, d % 4 == 0: no transform makes hex-order copies).
#pragma once

#include "common.h"
#include "gemm_f32.h"

namespace ctts {

constexpr int WNWG_MAX_CHUNKS = 352;      // chunk -> address table entries: 2 C / 16 + 2 (C + H) / 16 chunks (C = 512, H = 256: 160;
                                          // F(4,3): 4 C / 16 + 2 (C + H) / 16 + 2 H / 16 = 256; F(6,3): 6 C / 16 + 2 (C + H) / 16 +
                                          // 4 H / 16 = 352).  The KD = 2 kernels' LDS is then 3 x 24 KiB + 352 x 16 B + 512 B =
                                          // 79 872 B: two workgroups fit a CU's 160 KiB with 4 KiB to spare - nothing else fits
constexpr int WNWG_F23 = 0, WNWG_F43 = 1, WNWG_F63 = 2;

struct WnWinogradLayerArgs {
    // packed weights of the layer, as the lean form's launches take them: G2, G3 in SPLIT packing [2C / 256][C / 16][16][256],
    // [W0 | C_i], [-W2 | C_i] in GATE packing [2C / 256][(C + H) / 16][16][256]; bias in the GATE launch's block-local row order
    // F(4,3): A_T2..A_T5 = U1..U4 (SPLIT), A_e = [U0 | C_i], A_o = [U5 | C_i] (GATE)
    // F(6,3): A_T2..A_T7 = U1..U6 (SPLIT), A_e = [U0 | C_i], A_o = [U7 | C_i] (GATE)
    const float *A_T2, *A_T3, *A_e, *A_o, *bias;
    const float *A_T4, *A_T5;
    const float *A_T6, *A_T7;                 // F(6,3): U5, U6
    const float* V; long long vplane;         // V1..V4 [4][B][C][ldp]; F(4,3): V0..V5 [6][B][C][ldp]; F(6,3): V0..V7 [8][B][C][ldp]
    const float* Hc; long long hplane;        // cond copies h2e, h2o [2][B][H][ldp] (in_place = 0); F(4,3): h(t_0)..h(t_3) [4][B][H][ldp]
    const float* h2; long long h_bstride;     // the flow's cond rows in the natural layout [B][H][ld] (in_place = 1: d % 4 == 0)
    float* act; long long act_bstride;        // [B][C][ld], natural columns
    int C, H, batch;
    int ldp, Lp, ntiles;                      // pair space: row stride, pair columns per batch item, 128-column tiles per batch item
    int d, L, ld, pad;                        // dilation; natural geometry
    int in_place;
    int form;                                 // WNWG_F23 (0), WNWG_F43 or WNWG_F63
    // set by the launcher: column tiles (of the kernel's own width) per batch item and in the launch, first batch item, column origin
    int kt, kt_total, b0, col0;
};

// true when the kernel can run these channel counts (the caller selects the lean form otherwise)
bool wn_winograd_layer_supported(int C, int H);
bool wn_winograd_layer_f43_supported(int C, int H);
bool wn_winograd_layer_f63_supported(int C, int H);
int launch_wn_winograd_layer(const WnWinogradLayerArgs& a, hipStream_t stream);
// quad columns (64 or 128) of the calling thread's most recent F(4,3) layer launch; 0 before the first
int last_wn_winograd_f43_width();

}  // namespace ctts
