// Launchers of the bf16 MFMA conv-GEMM for gfx950 (contract: gemm_bf16.h; kernels: gemm_bf16_kernels.h).
#include <cstdlib>

#include "gemm_bf16_kernels.h"
#include "gemm_f32.h"
#include "tuning.h"

namespace ctts {

int launch_pack_a_bf16(bf16_t* dst, const float* src, int MB, int nch_total, int k_off, int ksrc, int epi, int C,
                       int M, long long src_row_off, long long src_row_stride, int src_k_stride, hipStream_t s,
                       int k_group, int k_member, int part, int f16) {
    // a ragged ksrc (e.g. a 20-wide speaker embedding) is zero-filled up to its 32-wide slab boundary
    const int kfill = (ksrc + BGEMM_KC - 1) / BGEMM_KC * BGEMM_KC;
    CTTS_CHECK_ARG(k_off % 8 == 0 && ksrc > 0, "pack_a_bf16: k offset must be 8-aligned");
    CTTS_CHECK_ARG(k_off % BGEMM_KC == 0 || ksrc % 8 == 0, "pack_a_bf16: a ragged k range must start on a slab");
    const int kspan = k_off % BGEMM_KC == 0 ? kfill : ksrc;
    CTTS_CHECK_ARG(k_off + kspan * (k_group > 1 ? k_group : 1) <= nch_total * BGEMM_KC, "pack_a_bf16: k range");
    CTTS_CHECK_ARG(k_group <= 1 || (ksrc % BGEMM_KC == 0 && k_off % BGEMM_KC == 0), "pack_a_bf16: k group");
    hipLaunchKernelGGL(pack_a_bf16_kernel, dim3(kspan / 8, MB), dim3(256), 0, s, dst, src, nch_total, k_off, ksrc, epi, C,
                       M, src_row_off, src_row_stride, src_k_stride, k_group, k_member, part, f16);
    CTTS_CHECK_LAUNCH("pack_a_bf16");
    return CTTS_OK;
}

namespace {
// The four block shapes, in order of preference: persistent (ps, 4 LDS stages), ping-pong (pp, 3 stages), wide 256 x 256, narrow
// 256 x 128 (gemm_bf16_kernels.h).  One list for both operand types: F16 = IEEE half.
// ADD: the GATE epilogue with the fp32 addend - instantiated for IEEE half only (the ax WaveGlow's half-storage path is its one
// user; launch_gemm_bf16 refuses a bf16 launch with an addend instead of quietly dropping it).
template <int EPI, bool F16, bool ADD = false>
void launch_bf16_shape(const BGemmArgs& b, bool ps, bool pp, bool wide, dim3 pg, dim3 grid, hipStream_t stream) {
    if (ps) hipLaunchKernelGGL((conv_gemm_bf16_ps_kernel<EPI, 4, 0, F16, ADD>), pg, dim3(512), 0, stream, b);
    else if (wide && pp) hipLaunchKernelGGL((conv_gemm_bf16_pp_kernel<EPI, 3, F16, ADD>), grid, dim3(512), 0, stream, b);
    else if (wide) hipLaunchKernelGGL((conv_gemm_bf16_kernel<EPI, 4, F16, ADD>), grid, dim3(512), 0, stream, b);
    else hipLaunchKernelGGL((conv_gemm_bf16_kernel<EPI, 2, F16, ADD>), grid, dim3(256), 0, stream, b);
}
}  // namespace

int launch_gemm_bf16(int epi, const BGemmArgs& a, hipStream_t stream) {
    CTTS_CHECK_ARG(a.nseg >= 1 && a.nseg <= BGEMM_MAX_SEG, "gemm_bf16: nseg=%d", a.nseg);
    int nch = 0;
    for (int s = 0; s < a.nseg; ++s) {
        CTTS_CHECK_ARG(a.seg[s].nch > 0 && a.seg[s].base, "gemm_bf16: empty segment %d", s);
        CTTS_CHECK_ARG(a.seg[s].shift >= -a.pad && a.seg[s].shift <= a.pad, "gemm_bf16: shift %d exceeds halo %d",
                       a.seg[s].shift, a.pad);
        nch += a.seg[s].nch;
    }
    CTTS_CHECK_ARG(nch == a.nch_total, "gemm_bf16: chunk count mismatch %d vs %d", nch, a.nch_total);
    if (a.interleave > 1) {
        CTTS_CHECK_ARG(a.interleave <= a.nseg, "gemm_bf16: interleave %d > nseg %d", a.interleave, a.nseg);
        for (int s = 1; s < a.interleave; ++s)
            CTTS_CHECK_ARG(a.seg[s].nch == a.seg[0].nch, "gemm_bf16: interleaved segments must have equal length");
    }
    // block-shape overrides for A/B tests (tuning.h: the environment is read once; ctts_tuning_reload re-reads it)
    const Tuning tune = tuning();
    // wide (256 x 256, 512 threads) tiles when the problem has enough of them (tune.bf16_wide_min: most of one round of the chip)
    const int ntiles_w = (a.L + 255) / 256;
    const bool pp = !tune.bf16_no_pp && a.nch_total + 3 <= BGEMM_PP_MAX_CHUNKS;
    const bool wide = !tune.bf16_no_wide && (long long)a.MB * ntiles_w * a.batch >= tune.bf16_wide_min && ntiles_w * 256 + 2 * a.pad <= a.ld;
    BGemmArgs b = a;
    if (wide) b.ntiles = ntiles_w;
    const int bn = wide ? 256 : BGEMM_BN;
    CTTS_CHECK_ARG(b.ntiles * bn + 2 * b.pad <= b.ld && b.L <= b.ntiles * bn, "gemm_bf16: geometry");
    CTTS_CHECK_ARG(epi == BGEMM_EPI_GATE ? (b.pairC > (b.MB - 1) * 128 && b.pairC <= b.MB * 128)
                                         : (b.M % 32 == 0 && b.split % 32 == 0 && b.M > (b.MB - 1) * BGEMM_BM &&
                                            b.M <= b.MB * BGEMM_BM),
                   "gemm_bf16: M=%d pairC=%d MB=%d split=%d", b.M, b.pairC, b.MB, b.split);
    CTTS_CHECK_ARG(!b.f16 || b.lo_off == 0, "gemm_bf16: the split (hi + lo) form exists for bf16 only");
    // the fp32 addend of the GATE epilogue: whole 32-channel tiles (no row is clamped), frames inside a row of the addend tensor
    CTTS_CHECK_ARG(!b.addend || (epi == BGEMM_EPI_GATE && b.f16 && b.lo_off == 0 && b.pairC % 32 == 0 && b.addend_frames >= 0 && b.addend_pad >= 0 &&
                                 b.addend_ld >= b.addend_pad + (b.addend_frames > 0 ? b.addend_frames : b.L)),
                   "gemm_bf16: addend (GATE in IEEE half only; pairC=%d, frames=%d, ld=%d, pad=%d)", b.pairC, b.addend_frames, b.addend_ld,
                   b.addend_pad);
    long long blocks = (long long)b.MB * b.ntiles * b.batch;
    b.map_mode = 0;
    const long long tiles = (long long)b.ntiles * b.batch;
    // persistent kernel: one workgroup per CU walks its tile sequence (gemm_bf16_kernels.h); K of more than its 4 stages.
    // Default for short K (<= 32 chunks: config 3's res GEMM, K = 512, where a tile's prologue is a large share of its
    // time: 0.729 -> 0.675 ms); on the long-K launches it measures equal (in-layer) or behind (skip) the per-tile kernel
    // (profiles/r5_14_bf16_ps_ab.txt).  CTTS_BF16_PS=1: everywhere it applies; CTTS_BF16_NO_PS: nowhere.
    const bool ps = wide && pp && !tune.bf16_no_ps && (tune.bf16_ps || b.nch_total <= 32) && b.nch_total > 4;
    const int cus = ps ? wf_row_cus() : 0;
    int ps_grid = 0;
    if (b.MB == 4 && !tune.no_xcd_pair) {
        b.map_mode = 1;
        blocks = 16ll * ((tiles + 3) / 4);
        ps_grid = cus / 16 * 16;
    } else if (b.MB == 2 && !tune.no_xcd_pair) {
        b.map_mode = 2;
        blocks = 16ll * ((tiles + 7) / 8);
        ps_grid = cus / 16 * 16;
    } else {
        ps_grid = cus / b.MB * b.MB;
    }
    CTTS_CHECK_ARG(blocks > 0 && blocks < (1ll << 31), "gemm_bf16: grid %lld", blocks);
    const bool use_ps = ps && ps_grid >= 16;
    const dim3 grid((unsigned)blocks), pg((unsigned)(use_ps ? ps_grid : 1));
    if (epi == BGEMM_EPI_GATE) {
        if (b.addend) launch_bf16_shape<BGEMM_EPI_GATE, true, true>(b, use_ps, pp, wide, pg, grid, stream);
        else if (b.f16) launch_bf16_shape<BGEMM_EPI_GATE, true>(b, use_ps, pp, wide, pg, grid, stream);
        else launch_bf16_shape<BGEMM_EPI_GATE, false>(b, use_ps, pp, wide, pg, grid, stream);
    } else {
        if (b.f16) launch_bf16_shape<BGEMM_EPI_SPLIT, true>(b, use_ps, pp, wide, pg, grid, stream);
        else launch_bf16_shape<BGEMM_EPI_SPLIT, false>(b, use_ps, pp, wide, pg, grid, stream);
    }
    CTTS_CHECK_LAUNCH("conv_gemm_bf16");
    return CTTS_OK;
}

}  // namespace ctts
