// Launch-shape overrides for A/B measurements.  The shapes of one GEMM are tested equal within the parity tolerance, not
// all bit-identical: the split-K shape of the fused WaveFlow layer (CTTS_F32_NO_SPLITK turns it off) sums K in a different
// order AND always computes in fp32 MFMA, also under the split-bf16 modes (include/cookietts_hip.h, "Which loop a launch
// really runs"; ctts_last_gemm_loop reports it).
// The environment is read ONCE, at the first launch that asks; ctts_tuning_reload() re-reads it (tests, profiling
// scripts).  Arithmetic choices (fp32 MFMA vs split-bf16 main loop) are NOT here: they travel in the config structs.
#pragma once

namespace ctts {

struct Tuning {
    bool f32_no_glds;      // CTTS_F32_NO_GLDS: fp32 conv-GEMM without the LDS-DMA staging
    bool f32_no_small;     // CTTS_F32_NO_SMALL: never the 128 x 64 small-problem shape (gemm_f32_small.hip)
    bool f32_force_small;  // CTTS_F32_FORCE_SMALL: the small shape whenever it applies, whatever the grid size (A/B, tests)
    bool f32_no_splitk;    // CTTS_F32_NO_SPLITK: never the split-K shape of the fused WaveFlow layer (batch 1-2)
    bool f32_no_round_split;  // CTTS_F32_NO_ROUND_SPLIT: never peel the tiles beyond the last whole round of workgroups off a large-shape launch
    bool no_xcd_pair;      // CTTS_GEMM_NO_XCD_PAIR: plain block id -> tile mapping
    bool bf16_no_wide;     // CTTS_BF16_NO_WIDE: never the 256 x 256 block
    int bf16_wide_min;     // CTTS_BF16_WIDE_MIN: 256 x 256 tiles (m-blocks x column tiles x batch) from which the wide block is taken (default in gemm_f32.hip load_tuning)
    bool bf16_no_pp;       // CTTS_BF16_NO_PP: never the ping-pong kernel
    bool bf16_ps;          // CTTS_BF16_PS: the persistent form of the skewed 8-wave kernel (one workgroup per CU walks a tile sequence) on every wide launch, not only the short-K ones
    bool bf16_no_ps;       // CTTS_BF16_NO_PS: never the persistent form
    bool wf_no_fuse;       // CTTS_WF_NO_FUSE: WaveFlow layer as separate GATE + res/skip launches
    bool taco_poll_delay_set;
    int taco_poll_delay[6];  // CTTS_TACO_POLL_DELAY="a,c,d,e,h,p": persistent decoder, s_sleep(1) units before the first poll of the att_h, ctx, dec_h, d2_h, h1, prenet exchanges (+ 65536: no light phase, straight to the full sweep; default 65572,65632,65548,65556,65544,65544; all 0: the form before round 5)
    bool taco_no_fuse;     // CTTS_TACO_NO_FUSE: per-launch decoder without the fused projection kernel
    bool taco_bg_no_pipe;  // CTTS_TACO_BG_NO_PIPE: batched decoder without the pipelined step (no EARLY cell sums in the small stages' launches)
    bool up_no_mfma;       // CTTS_UP_NO_MFMA: the VALU upsampling kernel also for the shape the MFMA one is built for (A/B)
    bool taco_valu;        // CTTS_TACO_VALU: ctts_taco_decoder_steps_f32 at batch <= 4 on the VALU kernels of rounds 1-3 (six launches per step) instead of the batched MFMA form
    bool f32_no_defer_skip;  // CTTS_F32_NO_DEFER_SKIP: WaveGlow fp32 WN stack with one res/skip GEMM per layer (the form before round 4)
    bool f32_no_wn_fold;   // CTTS_F32_NO_WN_FOLD: WaveGlow fp32 WN stack without the start / end folds (layer 0 on x, C-row skip GEMM, C-row tail)
    bool f32_no_winograd;  // CTTS_F32_NO_WINOGRAD: WaveGlow fp32 WN stack with the direct 3-tap in-layer GEMM at every size (no Winograd F(2,3) form)
    int f32_winograd_min;  // CTTS_F32_WINOGRAD_MIN: take the Winograd form for utterances of at least this many columns (steps per batch item); 0 = always (default in waveglow_api.hip)
    bool f32_winograd_plain;  // CTTS_F32_WINOGRAD_PLAIN: the Winograd form as five launches per layer (cond rows copied into pair order for every layer, T2 / T3 and even / odd as separate launches, d = 2 transform one column at a time): the A/B arm and the tests' reference of the merged form, bit-identical
    int f32_winograd_fused_min;  // CTTS_F32_WINOGRAD_FUSED_MIN: take the one-launch Winograd layer (wn_winograd_layer.hip) for utterances of at least this many columns; 0 = always (default in waveglow_api.hip).  Below it the Winograd form, where it engages, runs as the paired launches
    int f32_winograd_f43_min;  // CTTS_F32_WINOGRAD_F43_MIN: take the F(4,3) form of the one-launch Winograd layer (quad columns, 1.5 C products per output and row) for utterances of at least this many columns; 0 = always (default in waveglow_api.hip).  Below it, and wherever the one-launch layer does not engage, the F(2,3) forms run
    int f32_winograd_f63_min;  // CTTS_F32_WINOGRAD_F63_MIN: where the F(4,3) one-launch layer engages, run its layers with d % 4 == 0 in the F(6,3) form (hex columns, 8/6 C products per output and row) for utterances of at least this many columns; 0 = always (default in waveglow_api.hip)
    bool f32_winograd_no_f63;  // CTTS_F32_WINOGRAD_NO_F63: never the F(6,3) form: the F(4,3) layer wherever it engages (the A/B arm, bit-equal to the library before the F(6,3) form)
    bool f32_winograd_no_f43;  // CTTS_F32_WINOGRAD_NO_F43: never the F(4,3) form: the one-launch F(2,3) layer at every size it engages at (the A/B arm, bit-equal to the library before the F(4,3) form)
    bool f32_winograd_no_fused;  // CTTS_F32_WINOGRAD_NO_FUSED: never the one-launch Winograd layer: T2 | T3 and even | odd as two launches of the conv-GEMM with the T planes in HBM (the A/B arm)
    bool f32_cond_chain;   // CTTS_F32_COND_CHAIN: WaveGlow fp32 conditioning as the chain (upsampling launch, cond layer 0, cond layer 1 through spect / h_tmp) also where the composed form applies (one GEMM from the mel frames, waveglow_api.hip): the A/B arm, bit-equal to the library before the composed form
    bool wf_no_region_split; // CTTS_WF_NO_REGION_SPLIT: the fused WaveFlow layer as ONE launch per layer (no A | M | B regions on three streams)
    bool wf_no_row_queue;  // CTTS_WF_NO_ROW_QUEUE: never the one-launch-per-row work queue of the fused WaveFlow layers
    int wf_row_queue_min;  // CTTS_WF_ROW_QUEUE_MIN: take the row queue from this many 128-column items per layer on (A/B; default in waveflow_api.hip)
    int wf_queue_debug;    // CTTS_WF_QUEUE_DEBUG: 16 / 32 force the 128 x 128 / split-K body, 64 two workgroups per CU at every size, 128 one launch per ROW instead of one per flow
    int wf_inject_abort;   // CTTS_WF_INJECT_ABORT: (tests) start the call with the queue's abort word set
    bool wf_fwd_rowwise;   // CTTS_WF_FWD_ROWWISE: the WaveFlow analysis pass (ctts_waveflow_forward_*) row by row through the inverse's per-layer launches also on models that have the all-rows form (A/B; same tile arithmetic)
    bool wf_no_vec_interp; // CTTS_WF_NO_VEC_INTERP: the scalar form of the WaveFlow conditioning interpolation (bit-identical)
};

Tuning tuning();           // snapshot (by value)
void reload_tuning();      // ctts_tuning_reload

}  // namespace ctts
