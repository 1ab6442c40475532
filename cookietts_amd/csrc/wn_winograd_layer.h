// One launch per Winograd F(2,3) in-layer step of the fp32 WaveGlow (wn_winograd_layer.hip): behind the input transform, the four
// products of a pair block
//   S = G2 V2,  D = G3 V3,  (S, D) <- (S + D, S - D),
//   act[t_e] = gate(S + [W0 | C_i] [V1; h(t_e)] + b),   act[t_o] = gate(D + [-W2 | C_i] [V4; h(t_o)] + b)
// run one after the other through ONE chunk stream of a workgroup that owns 128 packed rows (the tanh and the sigmoid rows of 64
// channels) x 128 pair columns; T2 / T3 never leave the registers.  The operands are the panels and planes the lean form
// (waveglow_api.hip, run_in_layer_winograd) already has.
#pragma once

#include "common.h"
#include "gemm_f32.h"

namespace ctts {

constexpr int WNWG_MAX_CHUNKS = 320;      // chunk -> address table entries: 2 C / 16 + 2 (C + H) / 16 chunks (C = 512, H = 256: 160)

struct WnWinogradLayerArgs {
    // packed weights of the layer, as the lean form's launches take them: G2, G3 in SPLIT packing [2C / 256][C / 16][16][256],
    // [W0 | C_i], [-W2 | C_i] in GATE packing [2C / 256][(C + H) / 16][16][256]; bias in the GATE launch's block-local row order
    const float *A_T2, *A_T3, *A_e, *A_o, *bias;
    const float* V; long long vplane;         // V1..V4 [4][B][C][ldp]
    const float* Hc; long long hplane;        // cond copies h2e, h2o [2][B][H][ldp] (in_place = 0)
    const float* h2; long long h_bstride;     // the flow's cond rows in the natural layout [B][H][ld] (in_place = 1: d % 4 == 0)
    float* act; long long act_bstride;        // [B][C][ld], natural columns
    int C, H, batch;
    int ldp, Lp, ntiles;                      // pair space: row stride, pair columns per batch item, 128-column tiles per batch item
    int d, L, ld, pad;                        // dilation; natural geometry
    int in_place;
    // set by the launcher: column tiles (of the kernel's own width) per batch item and in the launch, first batch item, column origin
    int kt, kt_total, b0, col0;
};

// true when the kernel can run these channel counts (the caller selects the lean form otherwise)
bool wn_winograd_layer_supported(int C, int H);
int launch_wn_winograd_layer(const WnWinogradLayerArgs& a, hipStream_t stream);

}  // namespace ctts
