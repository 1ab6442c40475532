/*
 * cookietts_hip.h - C ABI of the MI355X (gfx950) mel-to-wave hot path.
 *
 * The reference (CookiePPP/cookietts) has no FFI layer: its hot path sits behind Python
 * nn.Module classes that dispatch stock PyTorch ops.  This header is the
 * boundary those ops are replaced at.  Every entry point cites the reference code it
 * replaces (paths relative to /root/reference/CookieTTS/).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - All data pointers are DEVICE pointers owned by the caller (PyTorch-ROCm in the
 *     Python host).  The library never allocates or frees device memory; scratch is a
 *     caller-provided workspace sized by ctts_*_workspace_bytes().
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All work is
 *     enqueued asynchronously on it; no entry point synchronises.
 *   - Return value: 0 = ok, negative = error (CTTS_E_*); ctts_last_error() returns a
 *     thread-local human-readable message for the last failure on this thread.
 *   - No hidden MODEL state: the immutable pair (config, packed weight blob) is the
 *     "plan" - arithmetic mode, shapes and weights travel in it - and calls are thread-safe
 *     per (workspace, stream).  Process-wide are only the A/B and timing knobs latched from
 *     the environment at the first launch (ctts_tuning_reload / ctts_tuning_flags below:
 *     launch shapes, the persistent decoder's poll delays - never arithmetic except where a
 *     knob's line says "summation order"), and the profiling stamp buffer of
 *     ctts_taco_decoder_persistent_debug.
 *
 * "Padded activation layout": internal activation tensors are [B][rows][ld] fp32 with
 * the L valid time steps of a row at columns [pad, pad+L) and zeros in the halo, so
 * dilated-conv taps read x[l +- d] without bounds checks (ld, pad from
 * ctts_waveglow_geometry()).
 */
#ifndef COOKIETTS_HIP_H
#define COOKIETTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTTS_OK 0
#define CTTS_E_ARG (-1)       /* bad argument / unsupported shape */
#define CTTS_E_LAUNCH (-2)    /* HIP launch or runtime error */
#define CTTS_E_WORKSPACE (-3) /* workspace too small */
#define CTTS_E_ABORT (-4)     /* an earlier call on this workspace gave up a bounded device-side wait (ABI 6; ctts_waveflow_abort_status) */

#define CTTS_ABI_VERSION 7   /* 2: ctts_waveglow_config.speaker_embed_dim, ctts_waveglow_flow_weights.speaker_embed
                              * 3: gated_unit / merge_res_skip in ctts_waveflow_config and ctts_wgax_config
                              * 4: f32_gemm_mode in ctts_waveglow_config, ctts_waveflow_config, ctts_wgax_config and
                              *    ctts_conv1d_desc (the arithmetic mode belongs to the model, not to the process);
                              *    ctts_tuning_reload; the persistent decoder's control words are exactly the last 64 bytes
                              * 5: ctts_set_f32_gemm_mode / ctts_get_f32_gemm_mode speak CTTS_GEMM_* (one encoding for the
                              *    process default and the config structs' field) and are deprecated; ctts_last_gemm_loop
                              * 6: no process-global state behind the ABI: the process-wide GEMM mode is gone (set fails for
                              *    the split modes), profiles are caller-owned handles (ctts_profile_create / _bind /
                              *    _collect(handle, ...) / _destroy replace ctts_profile_enable / _collect(which, ...)), a
                              *    row-queue abort is a status (CTTS_E_ABORT from the next ctts_waveflow_inverse_* on that
                              *    workspace, ctts_waveflow_abort_status) besides the NaN audio; IEEE-half variant of the
                              *    reduced-precision WaveGlow path (ctts_waveglow_pack_flow_f16 / ctts_waveglow_infer_spk_f16)
                              * 7: ctts_set_f32_gemm_mode / ctts_get_f32_gemm_mode are gone (dead since 6); the Tacotron decoder and
                              *    the packed-sequence LSTM take batches up to 256 (ctts_taco_decoder_max_batch, the batched MFMA
                              *    form: larger packed blobs and workspaces - re-query the *_bytes functions); glow.py-class
                              *    WaveGlow: any hop_length, n_group 4 / 8 / 12 / 16 */

/* Main loop of the fp32 conv-GEMM a model's launches use (field f32_gemm_mode of the config structs). */
#define CTTS_GEMM_DEFAULT 0  /* the library default: fp32 MFMA */
#define CTTS_GEMM_F32 1      /* v_mfma_f32_32x32x2_f32: exact fp32 products */
#define CTTS_GEMM_BF16X3 2   /* split bf16: hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulation */
#define CTTS_GEMM_BF16X6 3   /* 3-way split (24 mantissa bits): the six products >= 2^-16 (hh, hm, mh, hl, lh, mm); fp32-grade */
/* `options` of the ctts_waveglow_*_opt entry points (0 = the entry point without the suffix).
 * CTTS_WG_OPT_COMPOSED_COND: the blob holds the composed conditioning ("Composed conditioning" below) and the call may use it. */
#define CTTS_WG_OPT_COMPOSED_COND 1
#define CTTS_N_SPEAKERS 512 /* rows of every speaker-embedding table (glow.py:129, efficient_model_ax.py:60) */

int ctts_abi_version(void);
const char* ctts_last_error(void);

/* Constructor arguments of the reference model that shape the path:
 * _4_mtw/waveglow/glow.py:226-265 (WaveGlow.__init__) and :114-186 (WN.__init__). */
typedef struct ctts_waveglow_config {
    int32_t n_mel_channels; /* 80 */
    int32_t n_group;        /* 8 */
    int32_t n_flows;        /* 12 */
    int32_t n_early_every;  /* 4 */
    int32_t n_early_size;   /* 2 */
    int32_t win_length;     /* 1024: ConvTranspose1d kernel */
    int32_t hop_length;     /* 256: ConvTranspose1d stride */
    int32_t n_layers;       /* 8 WN layers, dilation 2^i */
    int32_t n_channels;     /* 512 WN channels (multiple of 128) */
    int32_t kernel_size;    /* 3 */
    int32_t cond_hidden;    /* 256, hard-coded at glow.py:153 */
    int32_t speaker_embed_dim; /* WN_config['speaker_embed_dim'] (glow.py:116,129-133): 0 = single speaker */
    int32_t f32_gemm_mode;  /* CTTS_GEMM_*: main loop of this model's fp32 GEMMs (fp32 entry points only) */
} ctts_waveglow_config;

typedef struct ctts_waveglow_geometry {
    int32_t steps;          /* L = frames*hop/n_group */
    int32_t ld;             /* row stride of padded activation tensors (floats) */
    int32_t pad;            /* left halo (floats) */
    int32_t n_remaining;    /* channels of the initial latent (glow.py:265) */
} ctts_waveglow_geometry;

int ctts_waveglow_geometry_for(const ctts_waveglow_config* cfg, int32_t frames,
                               ctts_waveglow_geometry* out);

/* ---- weight ingest (replaces torch weight_norm hooks + module construction) ---------- */

/* w[o][:] = v[o][:] * (g[o] / ||v[o][:]||_2): torch.nn.utils.weight_norm as applied at
 * glow.py:135-137,155-165,171-173,184 (checkpoint keys *.weight_g / *.weight_v). */
int ctts_fold_weightnorm_f32(const float* v, const float* g, float* w, int32_t out_ch,
                             int32_t fan, void* stream);

/* Dense (already weight-norm-folded) fp32 weights of ONE flow, in the reference's own
 * tensor layouts (state_dict shapes, glow.py:110-186 / :65-83). */
typedef struct ctts_waveglow_flow_weights {
    const float* start_w;      /* [C][n_half]              WN.k.start */
    const float* start_b;      /* [C] */
    const float* cond_w[3];    /* [H][n_mel*G], [H][H], [2*C*n_layers][H]   WN.k.cond_layers.j */
    const float* cond_b[3];
    const float* const* in_w;  /* n_layers x [2C][C][ks]   WN.k.in_layers.i */
    const float* const* in_b;  /* n_layers x [2C] */
    const float* const* rs_w;  /* n_layers x [2C or C][C]  WN.k.res_skip_layers.i */
    const float* const* rs_b;
    const float* end_w;        /* [2*n_half][C]            WN.k.end */
    const float* end_b;        /* [2*n_half] */
    const float* w_inverse;    /* [c][c] fp32 inverse of convinv.k.conv.weight (glow.py:90-99) */
    const float* speaker_embed;/* [CTTS_N_SPEAKERS][speaker_embed_dim]  WN.k.speaker_embed.weight (glow.py:130-133);
                                  NULL when speaker_embed_dim == 0.  cond_w[0] is then [H][n_mel*G + speaker_embed_dim] */
} ctts_waveglow_flow_weights;

/* Bytes of the packed weight blob (device) for this config. */
size_t ctts_waveglow_packed_bytes(const ctts_waveglow_config* cfg);
/* Pack upsample.{weight [n_mel][n_mel][win], bias [n_mel]} (glow.py:238-241). */
int ctts_waveglow_pack_upsample(const ctts_waveglow_config* cfg, const float* up_w,
                                const float* up_b, void* packed, void* stream);
/* Pack one flow's weights into the MFMA-tile order the kernels stream. */
int ctts_waveglow_pack_flow(const ctts_waveglow_config* cfg, int32_t flow,
                            const ctts_waveglow_flow_weights* w, void* packed, void* stream);

/* ---- the hot path -------------------------------------------------------------------- */

size_t ctts_waveglow_workspace_bytes(const ctts_waveglow_config* cfg, int32_t batch,
                                     int32_t frames);

/* WaveGlow.infer (glow.py:314-350) with the noise made an explicit input.
 *   mel      [B][n_mel][F]      fp32 dense
 *   z_scaled [B][n_group][L]    fp32 dense, sigma already applied: the last n_remaining
 *                               rows are the initial latent (glow.py:326), the rows above
 *                               are the early-output noise in prepend order (glow.py:342-347)
 *   wave     [B][F*hop]         fp32 dense (glow.py:349)
 * workspace must be zero-filled once before its FIRST use with a given (batch, frames)
 * geometry (halo columns are never written afterwards). */
int ctts_waveglow_infer_f32(const ctts_waveglow_config* cfg, const void* packed,
                            const float* mel, const float* z_scaled, float* wave,
                            int32_t batch, int32_t frames, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Multispeaker form (WN_config['speaker_embed_dim'] > 0, glow.py:131-133, 193-196): speaker_ids [B] int64 on the
 * device, each in [0, CTTS_N_SPEAKERS).  Every flow's embedding row is appended under the squeezed spectrogram as extra
 * K rows of that flow's cond layer 0.  speaker_ids == NULL is an error for a multispeaker config and ignored otherwise
 * (ctts_waveglow_infer_f32 is this call with NULL). */
int ctts_waveglow_infer_spk_f32(const ctts_waveglow_config* cfg, const void* packed, const float* mel,
                                const float* z_scaled, const int64_t* speaker_ids, float* wave, int32_t batch,
                                int32_t frames, void* workspace, size_t workspace_bytes, void* stream);

/* bf16 variant (BASELINE config 3): the WN in-layer and res/skip contractions run on bf16 MFMA with
 * fp32 accumulation and the WN activations (residual stream, gated activations, skip sum, conditioning
 * hidden) are stored bf16; upsampling, the two small cond layers, `end`, the coupling and the inverse
 * 1x1 conv stay fp32.  Needs BOTH blobs: `packed` (ctts_waveglow_pack_*: fp32 pieces + biases) and
 * `packed_bf16` (ctts_waveglow_pack_flow_bf16, same dense inputs).  I/O tensors are fp32 as above. */
size_t ctts_waveglow_packed_bf16_bytes(const ctts_waveglow_config* cfg);
int ctts_waveglow_pack_flow_bf16(const ctts_waveglow_config* cfg, int32_t flow,
                                 const ctts_waveglow_flow_weights* w, void* packed_bf16, void* stream);
size_t ctts_waveglow_workspace_bf16_bytes(const ctts_waveglow_config* cfg, int32_t batch,
                                          int32_t frames);
int ctts_waveglow_infer_bf16(const ctts_waveglow_config* cfg, const void* packed,
                             const void* packed_bf16, const float* mel, const float* z_scaled,
                             float* wave, int32_t batch, int32_t frames, void* workspace,
                             size_t workspace_bytes, void* stream);
int ctts_waveglow_infer_spk_bf16(const ctts_waveglow_config* cfg, const void* packed, const void* packed_bf16,
                                 const float* mel, const float* z_scaled, const int64_t* speaker_ids, float* wave,
                                 int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* IEEE-half variant ("f16", ABI 6): the reference's own reduced-precision inference mode (glow.py:343, the notebooks' `.half()`
 * models).  Everything as in the bf16 variant - same layouts, same kernels, same blob and workspace SIZES
 * (ctts_waveglow_packed_bf16_bytes / ctts_waveglow_workspace_bf16_bytes) - but weights and WN activations are rounded to
 * IEEE half (11-bit significands instead of bf16's 8) and the products run on v_mfma_f32_32x32x16_f16, fp32 accumulation.
 * Range: a WN activation beyond 65 504 would become inf (the gated activations are in (-1, 1); the residual stream of the
 * models of this repository stays within a few units).  Same speed as bf16; waveform error against the fp32 reference about
 * 8x smaller (gated in tests/test_waveglow_gpu.py at the fp32 tolerance: RMS rel <= 1e-3). */
int ctts_waveglow_pack_flow_f16(const ctts_waveglow_config* cfg, int32_t flow,
                                const ctts_waveglow_flow_weights* w, void* packed_f16, void* stream);
int ctts_waveglow_infer_spk_f16(const ctts_waveglow_config* cfg, const void* packed, const void* packed_f16,
                                const float* mel, const float* z_scaled, const int64_t* speaker_ids, float* wave,
                                int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Split-bf16 variant ("bf16x3"): the same bf16 MFMA kernels with every GEMM operand carried as a hi + lo PAIR of bf16
 * planes (hi = bf16(v), lo = bf16(v - hi): 16 mantissa bits) and every contraction computed as the three products
 * hi*hi + lo*hi + hi*lo with fp32 accumulation (the lo*lo term, ~2^-16 of a product, is dropped).  Inputs therefore
 * carry a relative error of ~2^-17 instead of bf16's 2^-9, at a third of the bf16 MFMA rate - about three times the
 * fp32 MFMA rate of gfx950.  Same calling convention as the bf16 entry points; `packed_bf16x3` and the workspace have
 * their own sizes.  Waveform error against the fp32 reference goldens is stated in DESIGN.md and gated in the tests
 * at the fp32 tolerance (RMS rel <= 1e-3). */
size_t ctts_waveglow_packed_bf16x3_bytes(const ctts_waveglow_config* cfg);
int ctts_waveglow_pack_flow_bf16x3(const ctts_waveglow_config* cfg, int32_t flow,
                                   const ctts_waveglow_flow_weights* w, void* packed_bf16x3, void* stream);
size_t ctts_waveglow_workspace_bf16x3_bytes(const ctts_waveglow_config* cfg, int32_t batch,
                                            int32_t frames);
int ctts_waveglow_infer_spk_bf16x3(const ctts_waveglow_config* cfg, const void* packed, const void* packed_bf16x3,
                                   const float* mel, const float* z_scaled, const int64_t* speaker_ids, float* wave,
                                   int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* Stage entry points (same kernels, exposed for parity tests and profiling). */

/* upsample (ConvTranspose1d) + trim + squeeze: glow.py:318-324.  spect is padded layout
 * [B][n_mel*G][ld].  n_mel 80 / hop 256 / win 1024 / n_group 8 (the benchmark's): a W-stationary fp32 MFMA GEMM over the
 * fragment-ordered copy of the weights that ctts_waveglow_pack_upsample writes beside the plain one; other shapes: VALU kernels. */
int ctts_upsample_squeeze_f32(const ctts_waveglow_config* cfg, const void* packed,
                              const float* mel, float* spect, int32_t batch, int32_t frames,
                              void* stream);
/* One flow's WN stack: glow.py:188-222 up to (not including) `end`.  Reads audio rows
 * [ch_off, ch_off+n_half) of audio [B][n_group][L] dense and h_all (cond hidden for all
 * flows, from ctts_wn_cond_f32); leaves the skip sum in `out` (padded [B][C][ld]). */
int ctts_wn_cond_f32(const ctts_waveglow_config* cfg, const void* packed, const float* spect,
                     const float* spk_rows, float* h_tmp, float* h_all, int32_t batch, int32_t frames,
                     void* stream);   /* spk_rows [B][n_flows*S][ld] (S = speaker_embed_dim rounded up to 32) or NULL */
int ctts_wn_stack_f32(const ctts_waveglow_config* cfg, const void* packed, int32_t flow,
                      const float* audio, const float* h_all, float* x, float* act, float* out,
                      int32_t batch, int32_t frames, void* stream);
/* ---- Composed conditioning (fp32 entry points) ---------------------------------------------------------------------------
 * On a single-speaker model the conditioning is linear in the mel: a latent column t = P f + p (P = hop / n_group) sees the mel
 * frames f .. f - J + 1 only (J = win / hop), so  h_k[:, P f + p] = A_{k,p} [mel[f]; ..; mel[f-J+1]] + b'_k  with the constant
 * A_{k,p} = (W1_k W0_k) . (the upsampling taps of phase p) and b'_k = W1_k (W0_k b_up + b0_k) + b1_k: upsampling, trim, squeeze and
 * cond layers 0 and 1 of every flow become a padded copy of the mel and ONE GEMM launch, at about a third of the chain's products
 * (n_mel 80, hop 256, win 1024, n_group 8), without the spect and h_tmp buffers.
 * Built where ctts_waveglow_has_composed_cond(cfg) says 1: speaker_embed_dim 0, n_mel % 16 == 0, J <= 4, P a power of two in
 * [4, 256] (the model's f32_gemm_mode is asked at the call: the split-bf16 modes keep the chain).  For a model whose upsampler is
 * the dense ConvTranspose1d.  The caller opts in:
 *   blob of ctts_waveglow_packed_bytes_opt(cfg, CTTS_WG_OPT_COMPOSED_COND) bytes - the blob without it is its prefix, packed by the
 *     same calls; it grows by n_flows * P * 256 * (J * n_mel + 1) floats plus pack-time scratch;
 *   ctts_waveglow_pack_cond_composed(cfg, flow, w, ...) per flow, after ctts_waveglow_pack_upsample (whose weights it reads from the
 *     blob): A and b' formed in double, rounded once;
 *   ctts_waveglow_workspace_bytes_opt / ctts_waveglow_infer_spk_f32_opt with that option.  (The analysis pass,
 *     ctts_waveglow_forward_spk_f32, has no such form: it runs the chain, on either blob.)
 * A call takes the composed form where it issues fewer products than the chain (an utterance of a few frames fills a fraction of
 * the GEMM's 128-frame tile: n_mel 80, P 32: from 45 frames on; a function of the utterance, never of the batch), else the chain;
 * CTTS_F32_COND_CHAIN=1 in the environment: always the chain (A/B).  Not bit-equal to the chain (another summation order).
 * The stage entry runs the composed form whatever the length: mel [B][n_mel][F] dense -> h_all as ctts_wn_cond_f32 writes it;
 * scratch: ctts_wn_cond_composed_scratch_bytes (0 where the config has no composed form), any contents. */
int ctts_waveglow_has_composed_cond(const ctts_waveglow_config* cfg);
size_t ctts_waveglow_packed_bytes_opt(const ctts_waveglow_config* cfg, int32_t options);
int ctts_waveglow_pack_cond_composed(const ctts_waveglow_config* cfg, int32_t flow, const ctts_waveglow_flow_weights* w,
                                     void* packed, void* stream);
size_t ctts_waveglow_workspace_bytes_opt(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames, int32_t options);
int ctts_waveglow_infer_spk_f32_opt(const ctts_waveglow_config* cfg, const void* packed, const float* mel,
                                    const float* z_scaled, const int64_t* speaker_ids, float* wave, int32_t batch,
                                    int32_t frames, void* workspace, size_t workspace_bytes, int32_t options, void* stream);
size_t ctts_wn_cond_composed_scratch_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames);
int ctts_wn_cond_composed_f32(const ctts_waveglow_config* cfg, const void* packed, const float* mel, float* scratch,
                              float* h_all, int32_t batch, int32_t frames, void* stream);
/* `end` 1x1 conv + affine coupling inverse + inverse 1x1 conv (+ un-squeeze on the last
 * flow): glow.py:222,337-340,349.  Updates audio in place; if `wave` is non-NULL the
 * mixed channels are written un-squeezed to wave [B][L*n_group] instead. */
int ctts_flow_tail_f32(const ctts_waveglow_config* cfg, const void* packed, int32_t flow,
                       const float* out, float* audio, float* wave, int32_t batch,
                       int32_t frames, void* stream);

/* One flow exactly as ctts_waveglow_infer_spk_f32 runs it (both share one helper): the form the CTTS_F32_* knobs select at this
 * length - WN start / end folds, deferred skip sum, Winograd F(2,3) in-layers - or the per-layer stack plus the flow tail.
 *   audio [B][n_group][L] dense: rows [ch_off, ch_off + n_remaining) of flow `flow` are updated in place, the others are not
 *         touched (what the infer entry keeps in its workspace between flows);
 *   h_all [B][n_flows*256][ld] padded layout, as ctts_wn_cond_f32 writes it (only the flow's own 256 rows are read);
 *   wave  NULL, or [B][L*n_group]: the mixed rows go there un-squeezed instead (ctts_flow_tail_f32's rule).
 * workspace: ctts_waveglow_workspace_bytes(cfg, batch, frames) bytes, zero-filled once before its first use with this geometry. */
int ctts_waveglow_flow_f32(const ctts_waveglow_config* cfg, const void* packed, int32_t flow, float* audio,
                           const float* h_all, float* wave, int32_t batch, int32_t frames, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- the analysis pass: WaveGlow.forward (glow.py:267-312), fp32 entry only, no gradient -------------------------------
 * audio -> z and log-likelihood terms: voice conversion (z under one speaker id, ctts_waveglow_infer_spk_f32 under another),
 * scoring a checkpoint (WaveGlowLoss, glow.py:51-62) and the invertibility check infer(forward(x)) = x.  The WN stack is the
 * infer path's own (same kernels, same form selection by the CTTS_F32_* knobs and the length, f32_gemm_mode honoured); new are
 * the flow boundaries: a head kernel (forward 1x1 mix; flow 0 reads the waveform un-squeezed) and the forward direction of the
 * tail kernels (a_1 = exp(log_s) a_1 + b with expf, log_s, fp64 partial sums).
 * The forward mix matrices live in a blob of their own; the infer blob (`packed`) is read as it is. */
size_t ctts_waveglow_forward_packed_bytes(const ctts_waveglow_config* cfg);
/* w: [c][c] convinv.flow.conv.weight (c = the flow's remaining channels), fp32 on the device. */
int ctts_waveglow_pack_forward_mix(const ctts_waveglow_config* cfg, int32_t flow, const float* w, void* packed_fwd,
                                   void* stream);
/* The infer workspace plus the fp64 slots of the sums; zero-filled once before its first use with this geometry.  0 with a
 * message (ctts_last_error) for a config or geometry the plan refuses. */
size_t ctts_waveglow_forward_workspace_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames);
/*   mel    [B][n_mel][F]     fp32 dense
 *   audio  [B][F*hop]        fp32 dense (exactly F*hop samples: a shorter waveform moves the WN's zero padding)
 *   speaker_ids              [B] int64 on the device; NULL is an error for a multispeaker config and ignored otherwise
 *   z      [B][n_group][L]   out: early outputs first, in peel order - the row order ctts_waveglow_infer_spk_f32 takes as z_scaled
 *   log_s  NULL, or [B][S][L], S = sum_k n_half_k: flow k's rows at offset sum_{j<k} n_half_j
 *   sums   NULL, or double [B][n_flows + 1] on the device: sums[b][k] = sum of flow k's log_s over item b, sums[b][n_flows] =
 *          sum of z^2 over item b.  Accumulated in fp64 from the stored fp32 values in two stages of fixed order (no atomics):
 *          two calls give the same bits, and an item's sums do not depend on the batch it runs in. */
int ctts_waveglow_forward_spk_f32(const ctts_waveglow_config* cfg, const void* packed, const void* packed_fwd, const float* mel,
                                  const float* audio, const int64_t* speaker_ids, float* z, float* log_s, double* sums,
                                  int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream);
/* One forward flow exactly as ctts_waveglow_forward_spk_f32 runs it (both share one helper), mirroring ctts_waveglow_flow_f32:
 *   z      [B][n_group][L] dense: rows [ch_off, n_group) of flow `flow` are mixed and coupled in place, the rows above stay;
 *   wave   NULL, or (flow 0 only) [B][L*n_group]: the rows are read from there un-squeezed instead of from z;
 *   h_all  as ctts_wn_cond_f32 writes it;
 *   log_s  NULL, or [B][n_half][L] dense: this flow's log_s;   sum_log_s  NULL, or double [B]: its sum per item.
 * workspace: ctts_waveglow_forward_workspace_bytes(cfg, batch, frames) bytes. */
int ctts_waveglow_flow_forward_f32(const ctts_waveglow_config* cfg, const void* packed, const void* packed_fwd, int32_t flow,
                                   float* z, const float* wave, const float* h_all, float* log_s, double* sum_log_s,
                                   int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream);

/* ---- WaveFlow ("ax" core, waveflow=True): _4_mtw/waveglow/efficient_model_ax.py --------- */

/* Constructor arguments that shape the path (efficient_model_ax.py:19-169, glow_ax.py:427-543).
 * Built: PermuteHeight (folded into row addressing) or InvertibleConv1x1 mixing in both orders (mix_first), early
 * outputs, all fourteen gated units, res_skip=True, merge_res_skip, linear upsampling; in-layers dense (kh*kw <= 11 taps) or separable (depthwise kh x kw
 * + pointwise, glow_ax.py:525-531); conditioning either ONE k=1 linear WN cond layer on the mel, folded into the
 * in-layer GEMM (BASELINE config 4), or an arbitrary per-flow stack evaluated by the caller at frame rate and
 * handed over (cond_precomputed; SURVEY 8f.4: speaker embeddings, model-level and WN-level conv stacks with
 * activations - composed from ctts_conv1d_f32 / ctts_embed_rows_f32 / ctts_scale_add_rows_f32). */
/* channel mixing between flows (efficient_model_ax.py:139-165) */
#define CTTS_MIX_PERMUTE 0
#define CTTS_MIX_CONV1X1 1
/* WN_config['gated_unit'] names in the order of get_gate_func (glow_ax.py:168-198) */
#define CTTS_GATE_GTU 0
#define CTTS_GATE_GTRU 1
#define CTTS_GATE_GTLRU 2
#define CTTS_GATE_GLU 3
#define CTTS_GATE_TTU 4
#define CTTS_GATE_STU 5
#define CTTS_GATE_GTSU 6
#define CTTS_GATE_SPTU 7
#define CTTS_GATE_GSIU 8
#define CTTS_GATE_GSIRU 9
#define CTTS_GATE_GTSRU 10
#define CTTS_GATE_GSIRRU 11
#define CTTS_GATE_GSIRLRU 12
#define CTTS_GATE_GSIRRLRU 13
typedef struct ctts_waveflow_config {
    int32_t n_mel_channels;  /* 80 */
    int32_t n_flows;         /* 8 (even) */
    int32_t n_group;         /* 16: height of the squeezed audio */
    int32_t n_layers;        /* 8, width dilation 2^i */
    int32_t n_channels;      /* 64 (multiple of 64) */
    int32_t kernel_size_w;   /* 3 (odd) */
    int32_t kernel_size_h;   /* 3 */
    int32_t dilation_h;      /* height dilation of every layer unless dilation_h_l overrides it (>= 1; config 4: 1) */
    int32_t seperable_conv;  /* 0 | 1  (WN_config['seperable_conv'], the reference's spelling) */
    int32_t cond_precomputed;/* 0: mel + folded cond layer;  1: ctts_waveflow_inverse_cond_f32 */
    int32_t gated_unit;      /* CTTS_GATE_*: WN_config['gated_unit'] (glow_ax.py:168-198); 0 = 'GTU' */
    int32_t merge_res_skip;  /* 0 | 1: WN_config['merge_res_skip'] (glow_ax.py:612-626: every res_skip layer has C rows,
                                all of them skip; the layer input stays the `start` output) */
    int32_t n_early_every;   /* early outputs (ax:170-176, 340-341); 0 or > n_flows: none */
    int32_t n_early_size;    /* rows leaving the latent at every n_early_every-th flow */
    int32_t mixing;          /* CTTS_MIX_PERMUTE (PermuteHeight, folded into row addressing) | CTTS_MIX_CONV1X1 */
    int32_t mix_first;       /* 0 | 1: un-mix after / before the coupling inverse (ax:324-325, 337-338) */
    int32_t dilation_w[12];  /* WN_config['n_layers_dilations_w'] per layer (glow_ax.py:507-509); 0 = the default 2^i */
    int32_t dilation_h_l[12];/* WN_config['n_layers_dilations_h'] per layer (glow_ax.py:510-512); 0 = `dilation_h` */
    int32_t f32_gemm_mode;   /* CTTS_GEMM_*: main loop of this model's GEMMs (dense and fused separable layers) */
} ctts_waveflow_config;

/* Dense, weight-norm-folded fp32 weights of one flow in checkpoint layouts
 * (keys WN.k.WN.*): */
typedef struct ctts_waveflow_flow_weights {
    const float* start_w;      /* [C]                 WN.start (Conv2d 1->C, 1x1) */
    const float* start_b;      /* [C] */
    const float* cond_w;       /* [2*C*n_layers][n_mel]   WN.cond_layers.0 (k=1); NULL if cond_precomputed */
    const float* cond_b;       /* [2*C*n_layers] */
    const float* const* in_w;  /* n_layers x [2C][C][kh][kw]; separable: the pointwise [2C][C] (in_layers.i.1) */
    const float* const* in_b;  /* n_layers x [2C] */
    const float* const* rs_w;  /* n_layers x [2C or C][C] */
    const float* const* rs_b;
    const float* end_w;        /* [2][C] (row 0 = log_s, row 1 = t; efficient_modules.py:61) */
    const float* end_b;        /* [2] */
    const float* const* dw_w;  /* separable only: n_layers x [C][kh][kw]  depthwise (in_layers.i.0), else NULL */
    const float* const* dw_b;  /* n_layers x [C] */
    const float* w_inverse;    /* [n_rem_k][n_rem_k] fp32 inverse of convinv.k.weight (CTTS_MIX_CONV1X1), else NULL */
} ctts_waveflow_flow_weights;

size_t ctts_waveflow_packed_bytes(const ctts_waveflow_config* cfg);
int ctts_waveflow_pack_flow(const ctts_waveflow_config* cfg, int32_t flow,
                            const ctts_waveflow_flow_weights* w, void* packed, void* stream);
size_t ctts_waveflow_workspace_bytes(const ctts_waveflow_config* cfg, int32_t batch,
                                     int32_t samples);
/* WaveGlow.inverse(z, cond) of the ax core (efficient_model_ax.py:279-357) for waveflow=True:
 *   z    [B][T] fp32, sigma applied (T multiple of n_group)      mel [B][n_mel][frames] (as passed
 *   to inverse(), i.e. already padded by infer())                audio [B][T]
 * Includes the per-flow NaN -> 0 (ax:333-334).  Workspace zero-filled once before first use.
 *
 * How a row of the recurrence is launched (C = 64 models; results of the forms agree bit for bit within one tile shape, see
 * "Which loop a launch really runs" below): one launch per fused layer (small sizes: a layer is one wave's serial chain),
 * or - from 200 column tiles of 128 per layer on (batch 2 at 900 frames) up to 1250 - the ROW QUEUE: ALL rows of a flow (each
 * row = its n_layers fused layers + a tail stage: end conv, affine update of the next latent row, the next row's start conv) as
 * ONE launch whose workgroups take (row, stage, tile) items from an atomic counter in order and wait, per item, for the flags
 * of the neighbouring tiles of the previous stage only.  Items are claimed in order, so the oldest unfinished item can
 * always run: the launch cannot deadlock and needs no co-residency.  Its wait is bounded all the same (two periods of 1 s in a
 * row during which no workgroup of the launch claimed an item - time without progress, not wall time); if it ever expires
 * every workgroup leaves, the call fills `audio` with NaN instead of returning plausible noise (stream-ordered, so THIS
 * call's status code cannot report it) and a sticky status word in the workspace is set: the calling thread's NEXT
 * ctts_waveflow_inverse_* on that workspace - whichever workspaces and streams it used in between: the thread keeps an
 * event per not-yet-checked workspace (16 of them; beyond that the oldest is checked early and reported by the call that
 * displaced it) - waits for that event first, returns CTTS_E_ABORT with ctts_last_error() text and clears the word (the call
 * after that runs normally); ctts_waveflow_abort_status asks at once (a workspace about to be freed: ask before).  NaN is also a legal
 * output of this path (ignore_nan, ax:333-334) - the status, not the NaN, is what says "aborted".
 * CTTS_WF_NO_ROW_QUEUE = always one launch per layer.  The queue's control words and layer
 * descriptors live in the caller's workspace (included in ctts_waveflow_workspace_bytes); the descriptors reach it through a
 * pinned staging buffer of the calling host thread, which the thread's NEXT call rewrites only after an event behind this
 * call's last copy - so a call with the row queue may wait on the host for the thread's previous call and must not be recorded
 * into a HIP graph (use CTTS_WF_NO_ROW_QUEUE there). */
int ctts_waveflow_inverse_f32(const ctts_waveflow_config* cfg, const void* packed, const float* z,
                              const float* mel, float* audio, int32_t batch, int32_t samples,
                              int32_t frames, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Synchronises `stream` and reports (and clears) the workspace's row-queue status: CTTS_OK, or CTTS_E_ABORT if a
 * ctts_waveflow_inverse_* call on this workspace (same cfg / batch / samples, which fix its layout) aborted since the last
 * report.  The Python WaveFlow.inverse / infer call it whenever they synchronise anyway and raise. */
int ctts_waveflow_abort_status(const ctts_waveflow_config* cfg, int32_t batch, int32_t samples, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Same, for cond_precomputed models: cond [n_flows][B][2*C*n_layers][cond_ld] fp32 = the output of each flow's
 * WN conditioning stack at FRAME rate (glow_ax.py:566-577), valid frames at columns [cond_pad, cond_pad+frames);
 * upsampling (gax:545-554) and the per-layer slicing (gax:580-592) happen inside. */
int ctts_waveflow_inverse_cond_f32(const ctts_waveflow_config* cfg, const void* packed, const float* z,
                                   const float* cond, int32_t cond_ld, int32_t cond_pad, float* audio,
                                   int32_t batch, int32_t samples, int32_t frames, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- WaveFlow analysis pass: WaveGlow.forward(cond, audio) of the ax core (efficient_model_ax.py:184-277), waveflow=True ----
 * audio [B][T] (T multiple of n_group) -> z [B][T] (the early outputs first, in peel order, then the rest, un-squeezed as ax:277:
 * exactly the latent ctts_waveflow_inverse_* consumes), log_s [B][S][L] with S = sum_k (n_rem_k - 1) and L = T / n_group (flow k's
 * rows at offset sum_{j<k} (n_rem_j - 1); NULL = not wanted), log_s_sum [B][L] fp32 (ax:269-273) and sums [B][n_flows] fp64
 * (per item and flow, the sum of log_s over rows and columns).  No gradient: the analysis pass only.
 * Per flow k: early split (k % n_early_every == 0, k > 0: the first n_early_size active rows leave to the output), the mix before
 * (mix_first) or after the coupling - PermuteHeight composes into the row map (it is its own inverse, 0 bytes of forward blob),
 * the 1x1 conv is one pass over the rows with W_k = convinv.k.weight from the forward blob - and the coupling
 * (efficient_modules.py:28-40): row 0 passes, (log_s_r, t_r) = end(WN_2d(rows 0 .. Ga-2)), out[r+1] = fma(a[r+1], exp(log_s_r), t_r);
 * then NaN -> 0 when `ignore_nan`.  `preemphasis` != 0 applies PreEmphasis (efficient_loss.py:16-20) to the audio first:
 * y[0] = x[0] - p x[1] (the reference's reflection at t = 0, reproduced), y[t] = x[t] - p x[t-1].
 * Summation order: the end conv of a column is four fma chains over C / 4 ascending channels added as ((p0 + p1) + p2) + p3 (as in
 * the inverse); log_s_sum adds a flow's rows in row order and the flows in flow order, in fp32; the fp64 sums are two stages without
 * atomics - a thread adds its column's rows in row order, a block its 256 columns as a fixed tree, one thread the blocks in order - so
 * two calls give the same bits and an item's values do not depend on its batch.
 * Two forms, selected by the model (never by the batch):
 *   row-wise: rows 0 .. Ga-2 in natural order through the launches of the inverse's per-layer form (ring of history slots, every
 *     config ctts_waveflow_inverse_* accepts, the bf16x3 / bf16x6 modes included); the row's input is the known audio row and the
 *     tail multiplies and stores log_s.  The row queue is not used in this direction.
 *   all-rows (C = 64, GTU, dense in-layers, fp32 MFMA mode: config 4): per flow one mix launch, one start launch over all rows, ONE
 *     launch per WN layer over all (row, item, 128-column tile) blocks - each reads its row's descriptor from a device array, the
 *     same segments and a_ch_off the per-layer launch of that row would get - and one tail launch over all rows: n_layers + 3
 *     launches per flow where the row-wise form takes (Ga - 1) (n_layers + 2).  Nothing in it waits on another workgroup.
 *     CTTS_WF_FWD_ROWWISE=1 forces the row-wise form (A/B arm; same tile arithmetic within one tile shape; the row-wise form
 *     may pick the split-K shape at small sizes, which sums K in another order).  ctts_last_gemm_loop() bit 8 = all-rows layer.
 * Workspace (ctts_waveflow_forward_workspace_bytes; zero-filled once before first use, one geometry per workspace): the inverse's
 * buffers, then log_s of one flow [B][n_group][Lr], the fp64 partials, and for all-rows models three full-height tensors
 * [n_group - 1][B][C][ld] (two layer inputs - one with merge_res_skip - and the skip sum; config 4 at B = 8 and 900 frames:
 * 3 x 0.44 GB) + the descriptors, which reach it through the calling thread's pinned staging buffer with one copy per call
 * (so, like the row queue, an all-rows call must not be recorded into a HIP graph). */
size_t ctts_waveflow_forward_packed_bytes(const ctts_waveflow_config* cfg);   /* 0 with PermuteHeight mixing (and on a bad config) */
int ctts_waveflow_pack_forward_mix(const ctts_waveflow_config* cfg, int32_t flow, const float* W_k, void* fwd_blob, void* stream);
size_t ctts_waveflow_forward_workspace_bytes(const ctts_waveflow_config* cfg, int32_t batch, int32_t samples);
int ctts_waveflow_forward_f32(const ctts_waveflow_config* cfg, const void* packed, const void* fwd_blob, const float* audio,
                              const float* mel, float preemphasis, int32_t ignore_nan, float* z, float* log_s, float* log_s_sum,
                              double* sums, int32_t batch, int32_t samples, int32_t frames, void* workspace,
                              size_t workspace_bytes, void* stream);
/* cond_precomputed models: cond as for ctts_waveflow_inverse_cond_f32 */
int ctts_waveflow_forward_cond_f32(const ctts_waveflow_config* cfg, const void* packed, const void* fwd_blob, const float* audio,
                                   const float* cond, int32_t cond_ld, int32_t cond_pad, float preemphasis, int32_t ignore_nan,
                                   float* z, float* log_s, float* log_s_sum, double* sums, int32_t batch, int32_t samples,
                                   int32_t frames, void* workspace, size_t workspace_bytes, void* stream);

/* Small operators the conditioning stacks and the output stage are composed from (padded row layout as for
 * ctts_conv1d_f32: x [B][C][ld], valid columns [pad, pad+T)):
 *   embed_rows:     x[b][row0 + e][pad .. pad+T) = table[ids[b]][e]          (speaker embedding concat, ax:286-291)
 *   scale_add_rows: y = alpha * x + r   (r may be NULL; alpha read from the device: the rezero parameter, ax:299-307)
 *   deemphasis:     y[n] = x[n] + p * y[n-1] per utterance, fp64 recurrence like scipy.signal.lfilter (ax:351-355);
 *                   in place (y == x) allowed
 *   vol_unscale:    x > 0 -> 10^log2(x), x < 0 -> -(10^log2(-x)) in place over n floats (preceived_vol_scaling, ax:342-344)
 *   affine_rows:    x = (x + shift) * scale on rows [0, rows), valid columns only (shift_spect / scale_spect, ax:206-209)
 *   resample_rows:  F.interpolate along time, padded rows in and out: mode 0 'linear' align_corners=True to T_out
 *                   (ax:174, glow_ax.py:365), mode 1 'linear' align_corners=False and mode 2 'nearest' with the given
 *                   scale_factor (TransposedUpsampleNet residual, glow_ax.py:229-231); scale_factor <= 0: T_in / T_out
 *   interleave_phases: ConvTranspose1d(stride, padding) (glow_ax.py:222) = `stride` stride-1 convolutions over the
 *                   input positions, one per output residue r = (n + padding) mod stride, each run with
 *                   ctts_conv1d_f32 into phases[r] ([stride][B][C][ld_in]); this call writes
 *                   y[n] = phases[(n + padding) % stride][(n + padding) / stride] for n in [0, T_out) */
int ctts_vol_unscale_f32(float* x, int64_t n, void* stream);
int ctts_affine_rows_f32(float* x, int32_t batch, int32_t C, int32_t rows, int32_t T, int32_t ld, int32_t pad, float shift,
                         float scale, void* stream);
int ctts_resample_rows_f32(const float* x, float* y, int32_t batch, int32_t C, int32_t T_in, int32_t ld_in, int32_t pad_in,
                           int32_t T_out, int32_t ld_out, int32_t pad_out, int32_t mode, float scale_factor, void* stream);
int ctts_interleave_phases_f32(const float* phases, float* y, int32_t batch, int32_t C, int32_t stride, int32_t padding,
                               int32_t T_in, int32_t ld_in, int32_t pad_in, int32_t T_out, int32_t ld_out, int32_t pad_out,
                               void* stream);
int ctts_embed_rows_f32(const float* table, const int64_t* ids, float* x, int32_t row0, int32_t embed_dim,
                        int32_t batch, int32_t C, int32_t T, int32_t ld, int32_t pad, void* stream);
int ctts_scale_add_rows_f32(const float* x, const float* alpha_dev, const float* r, float* y, int32_t batch,
                            int32_t C, int32_t T, int32_t ld, int32_t pad, void* stream);
int ctts_deemphasis_f32(const float* x, float* y, int32_t batch, int32_t T, double p, void* stream);

/* ---- "ax" WaveGlow core with waveflow=False: AffineCouplingBlock + 1-D WN ------------------- */
/* Replaces, for inference, efficient_model_ax.py:309-346 (the flow loop of WaveGlow.inverse) with
 *   AffineCouplingBlock.inverse   efficient_modules.py:94-105   ((log_s, t) = WN(a0); a1 = (a1 - t) / exp(log_s))
 *   WN.forward (1-D)              glow_ax.py:375-418            (start, dilated in_layers + GTU gate, res/skip, end;
 *                                                               conditioning at frame rate, linearly interpolated
 *                                                               with align_corners=True, glow_ax.py:362-373)
 *   InvertibleConv1x1.inverse     efficient_modules.py:269-286  (W.float().inverse() taken by the caller)
 *   PermuteHeight.inverse         efficient_modules.py:376-403
 *   early outputs                 efficient_model_ax.py:312-316, 340-341;   ignore_nan  :13-16, 333-334
 *   mix_first ordering            efficient_model_ax.py:324-325, 337-338
 * Built: all fourteen gated units, res_skip=True, merge_res_skip, dense in-layers (<= 11 taps) and separable (depthwise +
 * pointwise, glow_ax.py:341-348) in-layers up to 31 taps (the ctts_wgax_sep_* entry points), width dilation 2^i or per layer,
 * the per-flow WN conditioning stack is evaluated by the caller (composed from ctts_conv1d_f32 / ctts_embed_rows_f32 /
 * ctts_scale_add_rows_f32 / ctts_replicate_halo_f32) and handed over, like ctts_waveflow_inverse_cond_f32: at FRAME
 * rate (upsample_first=False; `frames` columns, interpolated to the latent's rate inside the gate epilogue) or already
 * at the latent's rate (upsample_first=True, efficient_model_ax.py:116-126, 174-186: model-level TransposedUpsampleNet
 * via ctts_interleave_phases_f32 + ctts_resample_rows_f32; `frames` == samples / n_group, read as it is). */
typedef struct ctts_wgax_config {
    int32_t n_flows;         /* 48 in the reference's timed notebook config */
    int32_t n_group;         /* 24 (even, <= 32) */
    int32_t n_early_every;   /* 16 */
    int32_t n_early_size;    /* 2 (even) */
    int32_t n_layers;        /* 8 */
    int32_t n_channels;      /* 256 (multiple of 128) */
    int32_t kernel_size;     /* 3 (odd, <= 11): WN_config kernel_size_w or kernel_size */
    int32_t mixing;          /* CTTS_MIX_PERMUTE | CTTS_MIX_CONV1X1 */
    int32_t mix_first;       /* 0 | 1 */
    int32_t ignore_nan;      /* 1: NaN -> 0 on the latent after every coupling (the reference's default) */
    int32_t gated_unit;      /* CTTS_GATE_* (0 = 'GTU') */
    int32_t merge_res_skip;  /* 0 | 1 (glow_ax.py:401-416) */
    int32_t dilation_w[12];  /* WN_config['n_layers_dilations_w'] per layer (glow_ax.py:331-333); 0 = the default 2^i */
    int32_t f32_gemm_mode;   /* CTTS_GEMM_*: main loop of this model's GEMMs */
} ctts_wgax_config;

/* Dense, weight-norm-folded fp32 device weights of one flow in checkpoint layouts (keys WN.k.WN.*, convinv.k.weight) */
typedef struct ctts_wgax_flow_weights {
    const float* start_w;      /* [C][n_half_k] */
    const float* start_b;      /* [C] */
    const float* const* in_w;  /* n_layers x [2C][C][ks] */
    const float* const* in_b;  /* n_layers x [2C] */
    const float* const* rs_w;  /* n_layers x [2C or C][C] */
    const float* const* rs_b;
    const float* end_w;        /* [2*n_half_k][C]: rows [0, h) = log_s, [h, 2h) = t (efficient_modules.py:100) */
    const float* end_b;        /* [2*n_half_k] */
    const float* w_inverse;    /* [n_rem_k][n_rem_k] = convinv.k.weight[:, :, 0].float().inverse(); NULL for PERMUTE */
} ctts_wgax_flow_weights;

size_t ctts_wgax_packed_bytes(const ctts_wgax_config* cfg);
int ctts_wgax_pack_flow(const ctts_wgax_config* cfg, int32_t flow, const ctts_wgax_flow_weights* w,
                        void* packed, void* stream);
size_t ctts_wgax_workspace_bytes(const ctts_wgax_config* cfg, int32_t batch, int64_t samples);
/* The flow loop of WaveGlow.inverse(z, cond):
 *   z     [B][samples] fp32, sigma applied; samples a multiple of n_group; early-output noise is part of z (ax:312-316)
 *   cond  [n_flows][B][2*C*n_layers][cond_ld]: each flow's WN conditioning at frame rate, valid frames at columns
 *         [cond_pad, cond_pad + frames)
 *   audio [B][samples]
 * Workspace zero-filled once before first use (halo columns are never written). */
int ctts_wgax_inverse_f32(const ctts_wgax_config* cfg, const void* packed, const float* z, const float* cond,
                          int32_t cond_ld, int32_t cond_pad, int32_t frames, float* audio, int32_t batch,
                          int64_t samples, void* workspace, size_t workspace_bytes, void* stream);
/* IEEE-half storage form of the same model (what the reference's `.half()` asks for): the C-row tensors x, act and the skip
 * sum live as IEEE half in the K8-blocked layout, in-layer and res/skip products run on the f16 matrix pipe with fp32
 * accumulation; latent rows, start / end weights, biases, coupling, mixing and `cond` stay fp32.  Same arguments as the
 * functions above, its own packed blob and workspace.  gated_unit must be CTTS GTU (0) and kernel_size * n_channels / 32
 * at most 253: the size queries return 0 (ctts_last_error names the reason) and the others CTTS_E_ARG otherwise. */
size_t ctts_wgax_packed_f16_bytes(const ctts_wgax_config* cfg);
int ctts_wgax_pack_flow_f16(const ctts_wgax_config* cfg, int32_t flow, const ctts_wgax_flow_weights* w,
                            void* packed, void* stream);
size_t ctts_wgax_workspace_f16_bytes(const ctts_wgax_config* cfg, int32_t batch, int64_t samples);
int ctts_wgax_inverse_f16(const ctts_wgax_config* cfg, const void* packed, const float* z, const float* cond,
                          int32_t cond_ld, int32_t cond_pad, int32_t frames, float* audio, int32_t batch,
                          int64_t samples, void* workspace, size_t workspace_bytes, void* stream);
/* Separable in-layers (WN_config['seperable_conv'] with kernel_size > 1, glow_ax.py:341-348: weight-normed depthwise
 * Conv1d(C, C, ks, groups=C, dilation=d) then pointwise Conv1d(C, 2C, 1)).  Same config struct - `kernel_size` is the
 * DEPTHWISE width, odd, 3 .. 31 (the dense form's 11-tap limit does not apply) - and the same arguments as the functions
 * above, with an own packed blob and an own workspace (one more C-row tensor).  In ctts_wgax_sep_pack_flow, w->in_w[i] is the
 * pointwise [2C][C], w->in_b[i] its [2C] bias, dw_w[i] the depthwise [C][ks] and dw_b[i] its [C] bias, all weight-norm
 * folded.  Per layer: ctts_depthwise_conv1d_f32's kernel, then the dense form's two GEMMs with K = C in the first;
 * f32_gemm_mode acts on the GEMMs only, the depthwise stage is always an fp32 fma chain.  fp32 storage only. */
size_t ctts_wgax_sep_packed_bytes(const ctts_wgax_config* cfg);
int ctts_wgax_sep_pack_flow(const ctts_wgax_config* cfg, int32_t flow, const ctts_wgax_flow_weights* w,
                            const float* const* dw_w, const float* const* dw_b, void* packed, void* stream);
size_t ctts_wgax_sep_workspace_bytes(const ctts_wgax_config* cfg, int32_t batch, int64_t samples);
int ctts_wgax_sep_inverse_f32(const ctts_wgax_config* cfg, const void* packed, const float* z, const float* cond,
                              int32_t cond_ld, int32_t cond_pad, int32_t frames, float* audio, int32_t batch,
                              int64_t samples, void* workspace, size_t workspace_bytes, void* stream);
/* Depthwise 1-D convolution on padded rows: y[b][c][pad + l] = b[c] + sum_t w[c][t] * x[b][c][pad + l + (t - ks/2) * dil] for
 * l < L, evaluated as acc = b[c]; acc = fmaf(w[c][t], x[..], acc) for t = 0 .. ks-1 in ascending order.  x, y fp32
 * [batch][C][ld] (16-byte aligned, ld and pad multiples of 4), w [C][ks], ks odd <= 31, dil >= 1.  Only columns
 * [pad, pad + L) of y are written.  CTTS_E_ARG for a NULL pointer, x == y (not an in-place operator), an even ks or one above
 * 31, (ks/2) * dil > pad, or a row too short for the taps of its last column (pad + round_up(L, 4) + (ks/2) * dil > ld). */
int ctts_depthwise_conv1d_f32(const float* x, const float* w, const float* b, float* y, int32_t batch, int32_t C, int32_t L,
                              int32_t ld, int32_t pad, int32_t ks, int32_t dil, void* stream);
/* padding_mode='replicate' of the conditioning convs (efficient_model_ax.py:90, glow_ax.py:311): fill the `halo`
 * columns either side of the valid range of x [B][C][ld] with the edge values, before a ctts_conv1d_f32 reads them. */
int ctts_replicate_halo_f32(float* x, int32_t batch, int32_t C, int32_t T, int32_t ld, int32_t pad, int32_t halo,
                            void* stream);

/* ---- HiFi-GAN generator: _4_mtw/hifigan/models.py:35-148 (the vocoder _5_infer/t2s_server/text2speech.py:258-263 loads) ---- */

#define CTTS_HIFIGAN_MAX_UPS 8      /* upsampling stages */
#define CTTS_HIFIGAN_MAX_KERNELS 4  /* resblocks per stage (len(resblock_kernel_sizes)) */
#define CTTS_HIFIGAN_MAX_DILATIONS 3

/* The fields of config.json that shape the generator (models.py:96-119).  Refused (size queries return 0, the other
 * entry points CTTS_E_ARG, ctts_last_error names the field): resblock other than 1 / 2; an even resblock kernel or one
 * above 11; a halo (k - 1) * dilation above 128; upsample kernel - rate odd or negative (the output would not be
 * rate * T long); more than 4 live taps per upsampling phase; more stages / resblocks than the arrays hold;
 * upsample_initial_channel not divisible by 2^n_ups. */
typedef struct ctts_hifigan_config {
    int32_t num_mels;
    int32_t upsample_initial_channel;
    int32_t resblock;                  /* 1: ResBlock1 (three c1 / c2 pairs), 2: ResBlock2 (two convs) */
    int32_t n_ups;                     /* len(upsample_rates) */
    int32_t n_kernels;                 /* len(resblock_kernel_sizes) */
    int32_t upsample_rates[CTTS_HIFIGAN_MAX_UPS];
    int32_t upsample_kernel_sizes[CTTS_HIFIGAN_MAX_UPS];
    int32_t resblock_kernel_sizes[CTTS_HIFIGAN_MAX_KERNELS];
    int32_t resblock_dilation_sizes[CTTS_HIFIGAN_MAX_KERNELS][CTTS_HIFIGAN_MAX_DILATIONS];   /* ResBlock2 reads [j][0..1] */
} ctts_hifigan_config;

/* Floats of the flat folded-weight buffer ctts_hifigan_pack_f32 reads: every conv's (weight, bias) after weight norm is
 * folded (w = g * v / ||v||, models.py:138-146), concatenated in module order: conv_pre; then per stage i: ups.i
 * (ConvTranspose1d weight [C_in][C_out][k]) followed by resblocks.(i * n_kernels + j) for j = 0.., each as convs1.0-2,
 * convs2.0-2 (ResBlock1) or convs.0-1 (ResBlock2); conv_post last. */
size_t ctts_hifigan_weight_floats(const ctts_hifigan_config* cfg);
size_t ctts_hifigan_packed_bytes(const ctts_hifigan_config* cfg);
/* weights: device, `weight_floats` fp32 as described above -> packed: device blob of ctts_hifigan_packed_bytes (the
 * MFMA-tiled weights of every layer; transposed convs as their stride-1 phase convolutions). */
int ctts_hifigan_pack_f32(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed,
                          void* stream);
size_t ctts_hifigan_workspace_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames);
/* Generator.forward (models.py:121-137): mel [B][num_mels][mel_ld] (frames valid columns per row) ->
 * audio [B][1][frames * prod(upsample_rates)] = tanh(conv_post(...)).  One launch per conv; LeakyReLU, residual adds, the
 * sum over a stage's resblocks, its 1 / n_kernels and the tanh run inside those launches (csrc/hifigan.hip).  Arguments
 * are validated before the first launch. */
int ctts_hifigan_forward_f32(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld,
                             float* audio, int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                             void* stream);

/* IEEE-half storage mode of the same generator (csrc/hifigan_f16.hip): weights and every stored activation in IEEE half
 * (K8-blocked [ceil(C / 8)][L][8]), products on the f16 MFMA, accumulation, bias, residual add, the resblock mean and tanh
 * in fp32, one round-to-nearest-even rounding per stored value, IEEE overflow (no clamping).  Rounding points: the weight
 * once from the fp32 folded value (biases stay fp32); the mel once while it is staged; leaky_relu as the stored half times
 * the fp32 slope in fp32, rounded once; a conv's output as half(acc + bias [+ float(residual)]); the sum over a stage's
 * resblocks as half(float(sum) + v) per resblock from the unrounded fp32 v, the last one divided by n_kernels in fp32
 * before its rounding.  pack_f16 reads the same flat fp32 buffer as pack_f32; forward_f16 takes the fp32 mel and writes
 * the fp32 waveform like forward_f32.  Same contract: every argument is validated before the first launch, the size
 * queries return 0 (ctts_last_error names the option) for a config that is refused - exactly the configs the fp32
 * queries refuse. */
size_t ctts_hifigan_packed_f16_bytes(const ctts_hifigan_config* cfg);
int ctts_hifigan_pack_f16(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed,
                          void* stream);
size_t ctts_hifigan_workspace_f16_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames);
int ctts_hifigan_forward_f16(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld,
                             float* audio, int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Split-bf16 products on the fp32 tensors of the same generator (csrc/hifigan_bf16x3.hip): activations, workspace,
 * epilogues and launch sequence are forward_f32's; every product runs as hi + lo bf16 operands on the bf16 MFMA with fp32
 * accumulation.  Weights, once at pack time from the fp32 folded value: w_hi = bf16_rne(w), w_lo = bf16_rne(w - w_hi)
 * (biases stay fp32; padding and dead taps are zeros in both planes).  Activations, while a tile is staged: leaky_relu in
 * fp32 as forward_f32 does, then x_hi = bf16_rne(v), x_lo = bf16_rne(v - x_hi).  Product: acc += w_hi x_hi, + w_lo x_hi,
 * + w_hi x_lo in that order per K16 step; no lo x lo term.  A non-finite activation gives NaN (inf - inf in the lo plane).
 * An item of a batch equals the same item run alone bit for bit.  ctts_hifigan_packed_bf16x3_bytes ==
 * ctts_hifigan_packed_bytes (a hi | lo pair is the 4 bytes of the fp32 weight; the blob's layout differs) and
 * ctts_hifigan_workspace_bf16x3_bytes == ctts_hifigan_workspace_bytes.  pack_bf16x3 reads the same flat fp32 buffer as
 * pack_f32.  Same contract as the _f16 set: every argument is validated before the first launch, the size queries return
 * 0 (ctts_last_error names the option) for exactly the configs the fp32 queries refuse. */
size_t ctts_hifigan_packed_bf16x3_bytes(const ctts_hifigan_config* cfg);
int ctts_hifigan_pack_bf16x3(const ctts_hifigan_config* cfg, const float* weights, size_t weight_floats, void* packed,
                             void* stream);
size_t ctts_hifigan_workspace_bf16x3_bytes(const ctts_hifigan_config* cfg, int32_t batch, int32_t frames);
int ctts_hifigan_forward_bf16x3(const ctts_hifigan_config* cfg, const void* packed, const float* mel, int32_t mel_ld,
                                float* audio, int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ---- Tacotron2-TM decoder loop: _2_ttm/tacotron2_tm/model.py:668-767, 851-916 -------------- */

/* Shapes from hparams.py (:201-258).  Built topology = the repo defaults: attention_type 0 with
 * windowed attention, AttRNN_extra_decoder_input=True, two decoder LSTMs with residual, 2-layer prenet. */
typedef struct ctts_taco_decoder_config {
    int32_t n_mel_channels;        /* 80 */
    int32_t memory_in_dim;         /* 1313 = encoder 1024 + speaker 256 + sylzu 1 + torchMoji 32 */
    int32_t memory_dim;            /* 512  memory_bottleneck_dim */
    int32_t attention_dim;         /* 192 */
    int32_t attention_rnn_dim;     /* 1280 */
    int32_t decoder_rnn_dim;       /* 768 */
    int32_t second_decoder_rnn_dim;/* 768 (== decoder_rnn_dim: residual) */
    int32_t prenet_dim;            /* 256 */
    int32_t location_n_filters;    /* 32 */
    int32_t location_kernel_size;  /* 31 */
    int32_t window_range;          /* 16 */
} ctts_taco_decoder_config;

typedef struct ctts_lstm_weights {   /* torch LSTMCell layout, gate order i,f,g,o (layers.py:308-372) */
    const float* w_ih;  /* [4H][I] */
    const float* w_hh;  /* [4H][H] */
    const float* b_ih;  /* [4H] */
    const float* b_hh;  /* [4H] */
} ctts_lstm_weights;

/* Dense fp32 device pointers in checkpoint layouts (state_dict keys decoder.*). */
typedef struct ctts_taco_decoder_weights {
    const float* bottleneck_w;    /* [memory_dim][memory_in_dim]   memory_bottleneck.bottleneck (no bias) */
    const float* memory_layer_w;  /* [A][memory_dim]               attention_layer.memory_layer */
    const float* query_w;         /* [A][Ra]                       attention_layer.query_layer */
    const float* v_w;             /* [A]                           attention_layer.v */
    const float* loc_conv_w;      /* [F][2][K]                     location_layer.location_conv */
    const float* loc_dense_w;     /* [A][F]                        location_layer.location_dense */
    const float* prenet_w1;       /* [P][n_mel]                    prenet.layers.0 (no bias) */
    const float* prenet_w2;       /* [P][P]                        prenet.layers.1 */
    ctts_lstm_weights att_rnn;    /* I = P + memory_dim + Rd, H = Ra */
    ctts_lstm_weights dec_rnn;    /* I = Ra + memory_dim,     H = Rd */
    ctts_lstm_weights dec2_rnn;   /* I = Rd,                  H = Rd2 */
    const float* proj_w;          /* [n_mel][Rd2 + memory_dim]     linear_projection */
    const float* proj_b;          /* [n_mel] */
    const float* gate_w;          /* [Rd2 + memory_dim]            gate_layer */
    const float* gate_b;          /* [1] */
    float windowed_att_pos_offset;/* attention_layer.windowed_att_pos_offset (learned scalar) */
    float exp_smoothing_factor;   /* decoder.exp_smoothing_factor (raw; sigmoid applied inside) */
} ctts_taco_decoder_weights;

size_t ctts_taco_decoder_packed_bytes(const ctts_taco_decoder_config* cfg);
int ctts_taco_decoder_pack(const ctts_taco_decoder_config* cfg, const ctts_taco_decoder_weights* w,
                           void* packed, void* stream);
/* Largest batch one workspace / one ctts_taco_decoder_steps_f32 call takes for this shape: 256 where the batched MFMA form is
 * built (every cell's K = I + H a multiple of 64, every state width a multiple of 16, the windowed attention's limits: window
 * <= +-16, memory <= 512, attention dim <= 256, <= 32 location filters of <= 31 taps - the repo defaults and every checkpoint
 * shape under tests/golden), else 4; 0 for an invalid config.  The reference's server decodes up to
 * simultaneous_texts x batch_size_per_text = 256 rows per call (_5_infer/t2s_server/text2speech.py:418-424, 537, 554). */
int32_t ctts_taco_decoder_max_batch(const ctts_taco_decoder_config* cfg);
size_t ctts_taco_decoder_workspace_bytes(const ctts_taco_decoder_config* cfg, int32_t batch,
                                         int32_t text_len);
/* Decoder.inference prologue (model.py:866-877): memory bottleneck, processed_memory, zero states.
 *   memory_in [B][text_len][memory_in_dim],  lengths [B] int32 (device). */
int ctts_taco_decoder_init_f32(const ctts_taco_decoder_config* cfg, const void* packed,
                               const float* memory_in, const int32_t* lengths, int32_t batch,
                               int32_t text_len, void* workspace, size_t workspace_bytes,
                               void* stream);
/* Run decoder steps [step0, step0 + n_steps) (model.py:879-883 body = prenet + decode()).
 *   keep_masks [max_steps][2][B][P] uint8: the prenet's always-on dropout keep-masks (model.py:189-190)
 *   mel_out [B][n_mel][max_steps], gate_out [B][max_steps] (logits), align_out [B][max_steps][text_len]
 * The stop rule (model.py:898-904) is evaluated by the caller on gate_out between calls.
 * Where ctts_taco_decoder_max_batch(cfg) is 256 every batch takes the batched form: seven launches per step with the cells /
 * query / projection / prenet as MFMA GEMMs over the whole batch (v_mfma_f32_16x16x4_f32, weights streamed once per step
 * whatever the batch: csrc/tacotron_batched.h).  Other shapes (batch <= 4 only), or CTTS_TACO_VALU: six launches per step on
 * the VALU.  Same state layout in the workspace: the forms (and the persistent one below) can be mixed call by call. */
int ctts_taco_decoder_steps_f32(const ctts_taco_decoder_config* cfg, const void* packed,
                                const uint8_t* keep_masks, float* mel_out, float* gate_out,
                                float* align_out, int32_t batch, int32_t text_len, int32_t step0,
                                int32_t n_steps, int32_t max_steps, void* workspace, void* stream);
/* The same, also recording what Decoder.inference(return_hidden_state=True) returns (model.py:762, 888-889):
 *   hidden_out [B][second_decoder_rnn_dim + memory_dim][max_steps] = [dec_h + d2_h | attention context] per step (NULL = off).
 * (The persistent form has no such output: a caller that wants the hidden states uses this entry point.) */
int ctts_taco_decoder_steps_hidden_f32(const ctts_taco_decoder_config* cfg, const void* packed,
                                       const uint8_t* keep_masks, float* mel_out, float* gate_out,
                                       float* align_out, float* hidden_out, int32_t batch, int32_t text_len,
                                       int32_t step0, int32_t n_steps, int32_t max_steps, void* workspace,
                                       void* stream);

/* Split-bf16 (bf16x3) products for the three LSTM cell GEMMs of the free-running loop above 64 rows (batch >= 65: the plain
 * schedule of the batched form; csrc/tacotron_batched_bf16x3.h).  Tensors, workspace layout and size, launch sequence and every
 * other stage are the fp32 path's.
 *   Weights, once at pack time from the fp32 value: w_hi = bf16_rne(w), w_lo = bf16_rne(w - w_hi).
 *   Activations: the X operand of a cell ([prenet | context | hidden states], fp32 in the workspace) is split as it is read for
 *   the product: x_hi = bf16_rne(x), x_lo = bf16_rne(x - x_hi).
 *   Product, per step of 32 K columns on v_mfma_f32_16x16x32_bf16: acc += w_hi x_hi, then + w_lo x_hi, then + w_hi x_lo, fp32
 *   accumulation; no lo x lo term.  The K slices of a workgroup's waves are summed in a fixed order; biases, gates, cell update,
 *   the residual sum dec_h + d2_h and the hidden record are the fp32 cell epilogue unchanged.
 *   Everything that is not a cell GEMM - query rows, projection row set, second prenet layer, both attention parts, init, the
 *   stop rule (the caller's) - is unchanged and fp32.
 *   An item's result does not depend on the other rows of the batch (one item-tile shape and one K split for every batch above
 *   64 rows); a run is bit-identical to a repeat.
 * Blob: ctts_taco_decoder_pack_bf16x3 writes the fp32 blob of ctts_taco_decoder_pack, byte for byte, followed by the hi | lo planes
 * of the three cells ([m-tile][chunk of 32 K][hi | lo][lane][8 bf16]; a hi | lo pair is the 4 bytes of the fp32 weight), so
 *   ctts_taco_decoder_packed_bf16x3_bytes == ctts_taco_decoder_packed_bytes + 4 * (4 Ra (P + Dm + Rd + Ra) + 4 Rd (Ra + Dm + Rd)
 *                                            + 4 Rd2 (Rd + Rd2))      (+ 108 MB at the default shape)
 * and EVERY other entry point (init, steps_f32 / steps_hidden_f32 / steps_persistent_f32 / steps_forced_f32, prenet_frames,
 * project_frames) accepts the blob and gives the fp32 blob's bits.
 * ctts_taco_decoder_steps_bf16x3 takes the arguments of ctts_taco_decoder_steps_hidden_f32.  At or below 64 rows it runs exactly
 * what that entry point runs, bit for bit: those sizes are bound by the weight stream, not by the matrix pipe, and keep their
 * pipelined schedule.  The persistent form has no split-bf16 variant; the teacher-forced loop's is
 * ctts_taco_decoder_steps_forced_bf16x3, below, under this same contract.
 * Refused before any launch (the size query returns 0, the others CTTS_E_ARG; ctts_last_error names the reason): shapes without
 * the batched form (ctts_taco_decoder_max_batch(cfg) != 256), and shapes in which a K piece of a cell (prenet_dim, memory_dim,
 * decoder_rnn_dim, attention_rnn_dim) is not a multiple of 32 wide - the message names the field.  (Today's conditions of the
 * batched form imply the second: every K a multiple of 64 leaves no piece that is not a multiple of 32.) */
size_t ctts_taco_decoder_packed_bf16x3_bytes(const ctts_taco_decoder_config* cfg);
int ctts_taco_decoder_pack_bf16x3(const ctts_taco_decoder_config* cfg, const ctts_taco_decoder_weights* w,
                                  void* packed, void* stream);
int ctts_taco_decoder_steps_bf16x3(const ctts_taco_decoder_config* cfg, const void* packed,
                                   const uint8_t* keep_masks, float* mel_out, float* gate_out,
                                   float* align_out, float* hidden_out, int32_t batch, int32_t text_len,
                                   int32_t step0, int32_t n_steps, int32_t max_steps, void* workspace,
                                   void* stream);

/* ---- Teacher-forced decoding: Decoder.forward (model.py:769-849) with p_teacher_forcing = 1, what GTA.py runs in eval() mode
 * (_2_ttm/tacotron2_tm/GTA.py:77-117, 264; _3_generate_postnets/GTA.py:192).  Three stages around the workspace, state layout,
 * ctts_taco_decoder_init_f32 prologue and align_out of the free-running steps above.  Built where
 * ctts_taco_decoder_max_batch(cfg) is 256 (the batched form); other shapes are refused with CTTS_E_ARG. */

/* Bytes of prenet_all for `batch` items and n_frames steps: [n_frames][NB][prenet_dim] floats, NB = the padded row count of the
 * workspace (16, 32, then multiples of 64).  0 (and a message) for a shape or batch the batched form does not take. */
size_t ctts_taco_prenet_frames_bytes(const ctts_taco_decoder_config* cfg, int32_t batch, int32_t n_frames);
/* The prenet of EVERY step before the loop (model.py:823 on the frames of :803-813; Prenet.forward :187-190):
 *   prenet_all[t][b][:] = relu(W2 . (relu(W1 . x_t) * keep[t][0][b] * 2)) * keep[t][1][b] * 2,
 *   x_t = frames[b][:][t - 1] for t >= 1 (frames [B][n_mel][n_frames]: the layout of gt_mel), x_0 = the go frame: init_frame
 *   [B][n_mel], or zeros where it is NULL (model.py:805-810)
 *   keep_masks [n_frames][2][B][P] uint8 as in ctts_taco_decoder_steps_f32: index t is the mask of step t's prenet input.
 * Rows [B, NB) of every step are written as zeros.  One launch, both layers on v_mfma_f32_16x16x4_f32. */
int ctts_taco_prenet_frames_f32(const ctts_taco_decoder_config* cfg, const void* packed, const float* frames,
                                const float* init_frame, const uint8_t* keep_masks, float* prenet_all,
                                size_t prenet_all_bytes, int32_t batch, int32_t n_frames, void* stream);
/* Steps [step0, step0 + n_steps) of Decoder.forward's loop (model.py:829-844) under full teacher forcing: step t's prenet input
 * is prenet_all[t] (max_steps steps of the layout above), nothing is projected inside the loop.  Five stream-ordered launches
 * per step: attention RNN (+ the attention's part 1) -> query rows -> attention part 2 -> decoder RNN -> second decoder RNN;
 * above 16 rows four: the second decoder RNN and the NEXT step's attention RNN are two roles of one launch.
 *   align_out  [B][max_steps][text_len]
 *   hidden_out [B][second_decoder_rnn_dim + memory_dim][max_steps] = [dec_h + d2_h | attention context] per step (required:
 *              it is the input of ctts_taco_project_frames_f32 and Decoder.forward's hidden_att_contexts, model.py:761, 843-844)
 * Blocks of steps can be chained like the free-running entry points'. */
int ctts_taco_decoder_steps_forced_f32(const ctts_taco_decoder_config* cfg, const void* packed, const float* prenet_all,
                                       float* align_out, float* hidden_out, int32_t batch, int32_t text_len,
                                       int32_t step0, int32_t n_steps, int32_t max_steps, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* The same loop with split-bf16 (bf16x3) products for the three LSTM cell GEMMs above 64 rows (batch >= 65): the arithmetic
 * contract of ctts_taco_decoder_steps_bf16x3, word for word - weights split once at pack time, X split as it is read, per 32 K
 * columns acc += w_hi x_hi, + w_lo x_hi, + w_hi x_lo with fp32 accumulation, no lo x lo term, the fp32 cell epilogue (biases,
 * gates, cell update, dec_h + d2_h and its hidden_out record) unchanged.  Same arguments and checks as
 * ctts_taco_decoder_steps_forced_f32; `packed` is the blob of ctts_taco_decoder_pack_bf16x3.  The launch sequence is that entry
 * point's four launches per step with the three cell launches on the split planes (the second decoder RNN of step t and the
 * attention RNN of step t + 1 stay two roles of one launch); prenet_all, query rows, both attention parts, the context rows of
 * hidden_out and the two one-shot operators around the loop are fp32 and unchanged.
 *   A cell's bits are the same whether it runs in a launch of its own or as a role, so blocks of steps chain bit for bit; an
 *   item's result does not depend on the other rows of the batch; a run is bit-identical to a repeat.
 *   At or below 64 rows it runs exactly what ctts_taco_decoder_steps_forced_f32 runs, bit for bit.
 *   ctts_taco_decoder_steps_forced_f32 on the bf16x3 blob keeps giving the fp32 bits.
 * Refused before any pointer is touched, with the refusals of the other bf16x3 entry points (no batched form; a K piece of a cell
 * that is not a multiple of 32 wide, named by field). */
int ctts_taco_decoder_steps_forced_bf16x3(const ctts_taco_decoder_config* cfg, const void* packed, const float* prenet_all,
                                          float* align_out, float* hidden_out, int32_t batch, int32_t text_len,
                                          int32_t step0, int32_t n_steps, int32_t max_steps, void* workspace,
                                          size_t workspace_bytes, void* stream);
/* The gate and mel projections of every step after the loop (model.py:763-765), one launch over all B x n_frames columns:
 *   hidden [B][second_decoder_rnn_dim + memory_dim][n_frames] -> mel_out [B][n_mel][n_frames], gate_out [B][n_frames] (logits). */
int ctts_taco_project_frames_f32(const ctts_taco_decoder_config* cfg, const void* packed, const float* hidden,
                                 float* mel_out, float* gate_out, int32_t batch, int32_t n_frames, void* stream);

/* Persistent form of ctts_taco_decoder_steps_f32: ONE launch of 256 resident workgroups (256 threads each, one wave per
 * SIMD) runs all n_steps steps with EVERY LSTM weight resident on the compute units for the whole launch (registers + LDS;
 * the 108 MB of weights are read once, at entry: ask for blocks of >= 32 steps), products on v_mfma_f32_4x4x1, and vectors
 * move between workgroups as granules that carry their own flag (4-byte self-flagging values, 8-byte {tag, value} for the query; no grid barrier, no per-step launches).  Same state (workspace), same outputs, same keep_masks contract as ctts_taco_decoder_steps_f32, so the
 * two can be mixed call by call.  Built for the repo-default decoder shape (attention RNN 1280, decoder RNNs 768,
 * prenet 256, memory 512, window 16), batch <= 4, text_len <= 1024 on a device with >= 256 CUs:
 * ctts_taco_decoder_persistent_bytes returns 0 otherwise, also when the CURRENT device has fewer CUs (use the per-launch
 * form); with no device at all it answers for the shape alone.
 *   exchange: ctts_taco_decoder_persistent_bytes(...) device bytes, zero-filled ONCE by the caller; the call re-initialises the
 *   granule area (everything but the control words) itself before every launch.  The LAST 64 bytes (bytes - 64 .. bytes) are control words (uint32): word 0 stays 0 on success;
 *   non-zero = a bounded wait gave up (words 1..3: workgroup, phase, step), the outputs of that call are invalid and
 *   every later launch on the same buffer returns immediately (sticky) until the caller zeroes the words. */
size_t ctts_taco_decoder_persistent_bytes(const ctts_taco_decoder_config* cfg, int32_t batch, int32_t text_len);
int ctts_taco_decoder_steps_persistent_f32(const ctts_taco_decoder_config* cfg, const void* packed,
                                           const uint8_t* keep_masks, float* mel_out, float* gate_out,
                                           float* align_out, int32_t batch, int32_t text_len, int32_t step0,
                                           int32_t n_steps, int32_t max_steps, void* workspace, void* exchange,
                                           size_t exchange_bytes, void* stream);

/* Profiling aid for the persistent decoder: `stamps` = device buffer of 256 x 64 x 24 uint64 receiving s_memrealtime
 * (100 MHz) at the phase boundaries (slots 0..12) and at the publish instants (13..17) of the first 64 steps of every
 * later launch; NULL switches it off (scripts/profile_persistent.py). */
int ctts_taco_decoder_persistent_debug(void* stamps);

/* ---- Tacotron2-TM one-shot stages: operator-level primitives ------------------------------- */
/* The encoder (model.py:283-316) and postnet (:218-228) are stacks of "same"-padded Conv1d (+ eval-mode
 * BatchNorm1d, folded into the weights at pack time) + LeakyReLU / tanh, a packed-sequence BiLSTM, and a
 * handful of per-utterance vectors.  They are exposed as three primitives the Python host composes in the
 * reference's own order; all arithmetic is in the library.
 * Padded layout here: x [B][C][ld], valid columns [pad, pad+T), zeros elsewhere, ld % 4 == 0,
 * ld >= roundup(T,128) + 2*pad, pad >= kernel_size/2. */
typedef struct ctts_conv1d_desc {
    int32_t c_in;         /* multiple of 16 */
    int32_t c_out;
    int32_t kernel_size;  /* odd, <= 11 */
    int32_t act;          /* 0 none, 1 LeakyReLU(slope), 2 tanh */
    float slope;
    int32_t f32_gemm_mode; /* CTTS_GEMM_*: main loop of this operator's GEMM */
} ctts_conv1d_desc;
size_t ctts_conv1d_packed_bytes(const ctts_conv1d_desc* d);
/* w [c_out][c_in][k], b [c_out]; bn_* [c_out] or all NULL (eval BatchNorm1d folded: w*s, (b-mean)*s+beta). */
int ctts_conv1d_pack_f32(const ctts_conv1d_desc* d, const float* w, const float* b, const float* bn_gamma,
                         const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                         void* packed, void* stream);
/* y = act(conv1d(x)) (accumulate == 0) or y += conv1d(x) (accumulate != 0, act must be 0). */
int ctts_conv1d_f32(const ctts_conv1d_desc* d, const void* packed, const float* x, float* y,
                    int32_t accumulate, int32_t batch, int32_t T, int32_t ld, int32_t pad, void* stream);

/* Packed-sequence LSTM, one direction (nn.LSTM + pack_padded_sequence semantics, model.py:299-309):
 * item b runs len[b] steps (forward: t = 0..len-1, reverse: t = len-1..0); outputs beyond len are untouched. */
size_t ctts_lstm_seq_packed_bytes(int32_t input_size, int32_t hidden_size);
int ctts_lstm_seq_pack_f32(const ctts_lstm_weights* w, int32_t input_size, int32_t hidden_size, void* packed,
                           void* stream);
size_t ctts_lstm_seq_workspace_bytes(int32_t hidden_size, int32_t batch, int32_t ld);
/*   x [B][I][ld] padded; out[b][t][out_col + u] (row stride out_tstride, batch stride out_bstride) = h_t;
 *   hn[b][hn_col + u] (row stride hn_stride) = final hidden state; lengths int32 device.
 *   batch <= 4: one VALU launch per time step; hidden_size % 64 == 0: batch <= 256, the recurrent product of a time step is an
 *   MFMA GEMM over the batch (csrc/tacotron_batched.h, BG_EPI_SEQ) - ctts_lstm_seq_workspace_bytes answers 0 beyond that. */
int ctts_lstm_seq_f32(const void* packed, const float* x, const int32_t* lengths, int32_t reverse, float* out,
                      int64_t out_bstride, int32_t out_tstride, int32_t out_col, float* hn, int32_t hn_stride,
                      int32_t hn_col, int32_t batch, int32_t T, int32_t input_size, int32_t hidden_size, int32_t ld,
                      int32_t pad, void* workspace, size_t workspace_bytes, void* stream);
/* Both directions of a bidirectional layer (nn.LSTM(bidirectional=True), model.py:299-309) in lockstep: ONE launch per time
 * step covers the forward step t and the reverse step of every item, so the layer costs T dependent launches, not 2 T.
 * Same arithmetic and outputs as two ctts_lstm_seq_f32 calls (reverse = 0 into out_col_fwd / hn_col_fwd, reverse = 1 into
 * out_col_bwd / hn_col_bwd); each direction needs its own workspace of ctts_lstm_seq_workspace_bytes. */
int ctts_lstm_biseq_f32(const void* packed_fwd, const void* packed_bwd, const float* x, const int32_t* lengths, float* out,
                        int64_t out_bstride, int32_t out_tstride, int32_t out_col_fwd, int32_t out_col_bwd, float* hn,
                        int32_t hn_stride, int32_t hn_col_fwd, int32_t hn_col_bwd, int32_t batch, int32_t T, int32_t input_size,
                        int32_t hidden_size, int32_t ld, int32_t pad, void* workspace_fwd, void* workspace_bwd,
                        size_t workspace_bytes, void* stream);
/* The same layer with torchMoji's gates (utils/torchmoji/lstm.py:330-357): i, f, o through
 * hard_sigmoid(v) = clamp(0.2 v + 0.5, 0, 1) - one fmaf and a fmaxf / fminf clamp, plain fp32 - and g through tanh;
 * c' = f c + i g, h' = o tanh(c').  Same arguments, packed blobs (ctts_lstm_seq_packed_bytes / _pack_f32), workspaces
 * (ctts_lstm_seq_workspace_bytes), batch forms and packed-sequence semantics as ctts_lstm_biseq_f32; a row of length 0 is idle. */
int ctts_lstm_biseq_hardsig_f32(const void* packed_fwd, const void* packed_bwd, const float* x, const int32_t* lengths, float* out,
                                int64_t out_bstride, int32_t out_tstride, int32_t out_col_fwd, int32_t out_col_bwd, float* hn,
                                int32_t hn_stride, int32_t hn_col_fwd, int32_t hn_col_bwd, int32_t batch, int32_t T,
                                int32_t input_size, int32_t hidden_size, int32_t ld, int32_t pad, void* workspace_fwd,
                                void* workspace_bwd, size_t workspace_bytes, void* stream);

/* ---- torchMoji feature encoder (utils/torchmoji/model_def.py:100-253, feature_output=True) -------------------------------
 * The T2S server's default style input (text2speech.py:497-509).  For tokens [B][T] (int64, device):
 *   len[b]     = index of the last non-zero token of row b, plus one (model_def.py:193); zeros inside a sentence are tokens
 *   x[b][t]    = tanh(embed[tok[b][t]])                                              E wide      (model_def.py:209-210)
 *   lstm_0     packed bidirectional hard-sigmoid LSTM, E -> H per direction, zero initial states (model_def.py:189-190, 220)
 *   lstm_1     the same, 2H -> H per direction, fed with lstm_0's [fwd | bwd]        (model_def.py:221)
 *   feat[b][t] = [lstm_1 out (2H) | lstm_0 out (2H) | x (E)], F = 4H + E wide, zero for t >= len[b]   (model_def.py:224-229)
 *   attention pooling (attlayer.py:48-66): logit = feat . attention_vector; w = exp(logit - M) for t < len[b], else 0;
 *   a = w / sum_t w; out[b] = sum_t a[b][t] feat[b][t].  The reference takes M over the whole padded batch; here M is the
 *   row's own maximum over its valid steps (the same quotient up to rounding, and no row can underflow to 0 / 0).
 * Outputs are in INPUT order: the reference sorts by length for packing, un-sorts the features and returns the attention
 * weights still sorted (model_def.py:194-195, 241-251); the rows here are independent, nothing is sorted.
 * The dropouts are identity in eval(); the classifier head (output_layer) is not part of this.  Products are fp32 MFMA
 * (CTTS_GEMM_DEFAULT); no reduced-precision mode: the call is a chain of 2 T + 12 dependent launches, launch-latency-bound.
 * Limits: embedding_dim % 16 == 0, hidden_size % 64 == 0, batch <= 256 (what ctts_taco_decoder_max_batch answers for the
 * batched form), T <= 8192.  Size queries answer 0 with a ctts_last_error message for a refused shape. */
typedef struct ctts_torchmoji_config {
    int32_t nb_tokens;       /* rows of the embedding table (50000) */
    int32_t embedding_dim;   /* 256 */
    int32_t hidden_size;     /* 512, per direction */
} ctts_torchmoji_config;
typedef struct ctts_torchmoji_weights {   /* device pointers, the checkpoint's own layouts */
    const float* embed;                   /* embed.weight [nb_tokens][E] */
    ctts_lstm_weights lstm[2][2];         /* lstm_{0,1}.{weight_ih,weight_hh,bias_ih,bias_hh}_l0 ([l][0]) and ..._l0_reverse ([l][1]) */
    const float* attention_vector;        /* attention_layer.attention_vector [4H + E] */
} ctts_torchmoji_weights;
size_t ctts_torchmoji_packed_bytes(const ctts_torchmoji_config* cfg);
int ctts_torchmoji_pack_f32(const ctts_torchmoji_config* cfg, const ctts_torchmoji_weights* w, void* packed, void* stream);
size_t ctts_torchmoji_workspace_bytes(const ctts_torchmoji_config* cfg, int32_t batch, int32_t T);
/* lengths[b] (int32, device) = last non-zero index of tokens[b][:] plus one, 0 for an all-zero row */
int ctts_torchmoji_lengths(const int64_t* tokens, int32_t* lengths, int32_t batch, int32_t T, void* stream);
/* features [B][4H + E]; attention [B][T] (zero beyond len[b]) or NULL.  lengths[b] in [0, T]: a row of length 0 yields a zero
 * feature row and zero attention.  A token outside [0, nb_tokens) is clamped into the table on the device (the gather never
 * reads outside it); reporting the range error is the host's business.  Every step of all T columns is issued; rows past
 * their length idle.  Workspace contents: x0 [B][E][ld], x1 [B][2H][ld] (the channel-major padded inputs of the two input
 * projections, zero outside [pad, pad + len[b])), feat [B][T][F], and the two directions' LSTM workspaces. */
int ctts_torchmoji_features_f32(const ctts_torchmoji_config* cfg, const void* packed, const int64_t* tokens,
                                const int32_t* lengths, float* features, float* attention, int32_t batch, int32_t T,
                                void* workspace, size_t workspace_bytes, void* stream);
/* The pooling alone (attlayer.py:48-66 as above): feat [B][T][D], vector [D], lengths int32 [B] in [0, T];
 * out [B][D], att [B][T] or NULL.  T <= 8192 (one row's logits live in LDS). */
int ctts_attention_pool_f32(const float* feat, const float* vector, const int32_t* lengths, float* out, float* att,
                            int32_t batch, int32_t T, int32_t D, void* stream);

/* x0[b][c][pad+t] = c < E ? embedding[text[b][t]][c] : spk_table[speaker[b]][c - E]   (model.py:1049, 284-288) */
int ctts_taco_embed_f32(const float* embedding, const float* spk_table, const int64_t* text,
                        const int64_t* speakers, float* x0, int32_t batch, int32_t T, int32_t E, int32_t S,
                        int32_t ld, int32_t pad, void* stream);
/* Per-utterance memory columns (model.py:1052-1066 + SylpsNet.infer_auto + tm_bn/tm_linear):
 * pred_sylps[b] = sylps_w . hn[b] + sylps_b;  memory_in[b][t][enc_dim:] = [speaker embed | sylzu | torchMoji crushed]. */
typedef struct ctts_taco_memory_weights {
    const float* sylps_w; const float* sylps_b;              /* encoder.sylps_layer [1][enc_dim], [1] */
    const float* speaker_embedding;                          /* [n_speakers][spk_dim] */
    const float* syl_w0; const float* syl_b0;                /* sylps_net.seq_layers.0 [hid][2], [hid] */
    const float* syl_w2; const float* syl_b2;                /* sylps_net.seq_layers.2 [1][hid], [1] */
    const float* syl_res_weight;                             /* [1] */
    const float* tm_gamma; const float* tm_beta; const float* tm_mean; const float* tm_var;  /* tm_bn (or NULL) */
    const float* tm_w; const float* tm_b;                    /* tm_linear [crushed][tm_dim], [crushed] */
} ctts_taco_memory_weights;
int ctts_taco_memory_f32(const ctts_taco_memory_weights* w, const float* hn, const int64_t* speakers,
                         const float* torchmoji, float* memory_in, float* pred_sylps, int32_t batch, int32_t T,
                         int32_t enc_dim, int32_t spk_dim, int32_t syl_hidden, int32_t tm_dim, int32_t tm_crushed,
                         void* stream);
/* The same with the reference's ``gt_sylps`` override (model.py:1044, 1058 "gt_sylps or pred_sylps"): gt_sylps [B] device floats
 * are what SylpsNet.infer_auto reads (NULL = the predicted value, i.e. ctts_taco_memory_f32); pred_sylps is written either way. */
int ctts_taco_memory_sylps_f32(const ctts_taco_memory_weights* w, const float* hn, const int64_t* speakers,
                               const float* torchmoji, const float* gt_sylps, float* memory_in, float* pred_sylps,
                               int32_t batch, int32_t T, int32_t enc_dim, int32_t spk_dim, int32_t syl_hidden,
                               int32_t tm_dim, int32_t tm_crushed, void* stream);
/* dense [B][C][src_ld] (first T columns) <-> padded [B][C][ld] copies */
int ctts_pad_rows_f32(const float* src, int64_t src_bstride, int32_t src_ld, float* dst, int32_t batch,
                      int32_t C, int32_t T, int32_t ld, int32_t pad, void* stream);
int ctts_unpad_rows_f32(const float* src, float* dst, int64_t dst_bstride, int32_t dst_ld, int32_t batch,
                        int32_t C, int32_t T, int32_t ld, int32_t pad, void* stream);

/* ---- STFT / mel frontend (utils/audio/stft.py) ------------------------------------------- */

/* STFT.__init__ (stft.py:46-77) / TacotronSTFT.__init__ (:155-166) arguments that shape the path. */
typedef struct ctts_stft_config {
    int32_t filter_length;   /* 1024 (multiple of 16) */
    int32_t hop_length;      /* 256 */
    int32_t win_length;      /* 1024 (informational: the window is already folded into the basis) */
    int32_t n_mel_channels;  /* 80; 0 = magnitude only */
    float clamp_val;         /* 1e-5: dynamic_range_compression clip (audio_processing.py:78-84) */
} ctts_stft_config;

size_t ctts_stft_packed_bytes(const ctts_stft_config* cfg);
/* forward_basis [2*(N/2+1)][N] = the module buffer of stft.py:60-76 ([Re;Im] DFT rows x window),
 * mel_basis [n_mel][N/2+1] = the buffer of stft.py:163-166 (may be NULL when n_mel_channels == 0). */
int ctts_stft_pack(const ctts_stft_config* cfg, const float* forward_basis, const float* mel_basis,
                   void* packed, void* stream);
size_t ctts_stft_workspace_bytes(const ctts_stft_config* cfg, int32_t batch, int32_t samples);
/* STFT.transform_jit magnitude (stft.py:79-111) and TacotronSTFT.mel_spectrogram (:180-207):
 *   y   [B][T] fp32 in [-1, 1];   frames = T / hop + 1
 *   mag [B][N/2+1][frames]  (may be NULL)      mel [B][n_mel][frames] = log(max(mel_basis @ mag, clamp))
 * workspace zero-filled once before first use (as for WaveGlow). */
int ctts_stft_mel_f32(const ctts_stft_config* cfg, const void* packed, const float* y, float* mag,
                      float* mel, int32_t batch, int32_t samples, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Phase / inverse path (used by the Denoiser, _4_mtw/waveglow/denoiser.py:55-72):
 *   inverse_basis [2*(N/2+1)][N] = the module buffer of stft.py:62-63,74 (pinv of the scaled DFT basis x window),
 *   window_sq [N] = the zero-centre-padded squared window of audio_processing.py:47-50. */
int ctts_stft_pack_inverse(const ctts_stft_config* cfg, const float* inverse_basis, const float* window_sq,
                           void* packed, void* stream);
/* STFT.transform_jit with phase (stft.py:99-111): mag, phase [B][N/2+1][frames] (phase may be NULL). */
int ctts_stft_transform_f32(const ctts_stft_config* cfg, const void* packed, const float* y, float* mag,
                            float* phase, int32_t batch, int32_t samples, void* workspace,
                            size_t workspace_bytes, void* stream);
/* STFT.inverse (stft.py:117-146): conv_transpose1d with the inverse basis, window-sum-square normalisation,
 * N/hop scaling, crop N/2 each side -> out [B][(frames-1)*hop].  If bias_spec [N/2+1] is non-NULL the magnitude
 * is first replaced by max(mag - bias_spec*strength, 0) (Denoiser.forward, denoiser.py:62-67).
 * workspace: ctts_stft_workspace_bytes(cfg, batch, (frames-1)*hop). */
int ctts_stft_inverse_f32(const ctts_stft_config* cfg, const void* packed, const float* mag, const float* phase,
                          const float* bias_spec, float strength, float* out, int32_t batch, int32_t frames,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Same with one bias spectrum PER UTTERANCE: bias_spec [batch][bias_bstride >= N/2+1] (Denoiser(speaker_dependant=True):
 * bias_spec[speaker_ids], denoiser.py:29-45, 65-66); bias_bstride = 0 shares one spectrum like ctts_stft_inverse_f32. */
int ctts_stft_inverse_bias_f32(const ctts_stft_config* cfg, const void* packed, const float* mag, const float* phase,
                               const float* bias_spec, int32_t bias_bstride, float strength, float* out,
                               int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---- attention-alignment scoring (T2S retry loop) -------------------- */

/* utils/model/utils.py:59-120 `alignment_metric(alignments, input_lengths, output_lengths, enc_min_thresh)`:
 * alignments [batch][dec][enc] fp32 (device); lengths are device fp32 [batch] or NULL (reference defaults:
 * enc-1 / dec-1).  out: device double [batch][6] = diagonalitys, avg_prob, encoder_max_focus,
 * encoder_min_focus, encoder_avg_focus, p_missing_enc.  The input is not modified (the reference zeroes the
 * padded decoder steps of its argument in place, :81). */
size_t ctts_alignment_workspace_bytes(int32_t batch, int32_t dec, int32_t enc);
int ctts_alignment_metric_f32(const float* alignments, const float* input_lengths, const float* output_lengths,
                              int32_t batch, int32_t dec, int32_t enc, float enc_min_thresh, double* out,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The same metric with a validity cut: valid_lengths device fp32 [batch] or NULL; decoder steps d >= valid_lengths[b] read as
 * zero (row max 0 at arg-max 0, nothing added to the encoder totals).  This is what the reference's SECOND alignment_metric call
 * of Tacotron2Loss (loss_function.py:270) sees: the first call (:251) zeroed its argument past the ground-truth length in place
 * (utils.py:81).  NULL: ctts_alignment_metric_f32 itself, bit for bit.  Same workspace. */
int ctts_alignment_metric_masked_f32(const float* alignments, const float* input_lengths, const float* output_lengths,
                                     const float* valid_lengths, int32_t batch, int32_t dec, int32_t enc,
                                     float enc_min_thresh, double* out, void* workspace, size_t workspace_bytes,
                                     void* stream);
/* utils/model/utils.py:47-56 (= text2speech.py:152-161) `get_first_over_thresh(x, threshold)`:
 * x [batch][T] fp32 -> out int32 [batch], first step with x >= threshold, else T-1. */
int ctts_first_over_thresh_f32(const float* x, int32_t batch, int32_t T, float threshold, int32_t* out, void* stream);

/* Decoder.inference's stop rule (_2_ttm/tacotron2_tm/model.py:879-904) on the device.  The reference copies every
 * step's gate to the host (:885) and evaluates there; here the rule runs over the gate LOGITS the decoder steps wrote,
 * block of steps by block of steps, and only its verdict (4 bytes) ever crosses to the host.
 *   state: ctts_taco_stop_state_bytes(batch) device bytes = { float sig_max[batch]; int32 break_point; int32 n_total };
 *          ctts_taco_stop_reset sets sig_max = 0, break_point = max_decoder_steps, n_total = -1.
 *   ctts_taco_stop_rule_f32 applies steps [step0, step0 + n_steps) of gate_logits [batch][gate_ld]:
 *          i > 4: sig_max = max(sig_max, sigmoid(gate)); min over the batch > gate_threshold -> break_point =
 *          min(break_point, i + gate_delay); i >= break_point -> n_total = i + 1 (sticky; later calls are no-ops).
 *   n_total is the int32 at byte offset 4 * (batch + 1) of state. */
size_t ctts_taco_stop_state_bytes(int32_t batch);
int ctts_taco_stop_reset(void* state, int32_t batch, int32_t max_decoder_steps, void* stream);
int ctts_taco_stop_rule_f32(const float* gate_logits, int32_t batch, int32_t gate_ld, int32_t step0, int32_t n_steps,
                            float gate_threshold, int32_t gate_delay, void* state, void* stream);

/* ---- the T2S retry loop: best-of-N selection, vocoder batch, int16 PCM ------------------------------------------
 * _5_infer/t2s_server/text2speech.py:548-651 runs Tacotron passes over rows = n_texts * per_text candidates (row =
 * j * per_text + k is candidate k of text j) until every text has a candidate scoring at least target_score or a stop rule
 * fires, reading every candidate back to the host to score it.  These entry points keep that loop's state on the device;
 * the host reads one 32-byte status block per pass.  Caller-owned device memory, nothing allocated or synchronised
 * inside, no kernel waits on another workgroup.  (ABI 7: additions do not bump the version.) */
typedef struct ctts_retry_config {
    double diagonality_weighting, max_focus_weighting, min_focus_weighting, avg_focus_weighting; /* :378-381: 0.5 1.0 0.5 1.0 */
    double target_score, absolutely_required_score;   /* :334: t2s_config.json's 0.75; -1e3 */
    int32_t max_attempts, absolute_maximum_tries;     /* :334: 64; 2048 */
    int32_t n_texts, per_text;                        /* simultaneous_texts, batch_size_per_text; each and their product <= 4096 */
    int32_t n_mel, t_cap, enc_cap;                    /* capacity of the kept winners: [n_mel][t_cap] mel and, when
                                                       * enc_cap > 0, [t_cap][enc_cap] alignments per text */
} ctts_retry_config;

/* The first 32 bytes of the state: what the host reads after a pass. */
typedef struct ctts_retry_status {
    int32_t done;              /* 0 go on; 1 min(best_score) >= target_score (:552); 2 the max_attempts rule (:621);
                                * 3 the absolute_maximum_tries rule (:623).  Sticky: once non-zero, updates are no-ops */
    int32_t n_passes;          /* updates counted (:560), the one a rule fired in included */
    double min_best_score;     /* np.amin(best_score) */
    int32_t min_tries;         /* np.amin(tries) */
    int32_t n_without_winner;  /* texts no candidate has won yet: the reference's assertion at :636 when not 0 */
    int32_t max_best_length;   /* max over texts of the winners' output_length (:650); 0 without winners */
    int32_t max_best_T;        /* max over texts of the winners' pass length */
} ctts_retry_status;

/* State layout: sections in this order, each starting on a 16-byte boundary (N = n_texts, R = rows):
 *   ctts_retry_status status
 *   double  best_score[N]            reset to -1e5 (:548)
 *   double  detail[N][6]             the winner's { weighted_score as score_str prints it (:606, before the 1e-7 of :615),
 *                                    diagonality, max_dur, min_dur, avg_dur, mis_dur punishment }
 *   int32_t tries[N], best_length[N] (the winner's output_length), best_T[N] (its pass's T), best_pass[N] (0-based pass,
 *           -1 = no winner), best_row[N] (row in that pass), changed[N] (row that won in the LAST update, else -1)
 *   float   best_mel[N][n_mel][t_cap]        columns [0, best_T) hold the winner's whole pass-length mel
 *   float   best_alignments[N][t_cap][enc_cap]   rows [0, best_T), columns [0, enc of that pass)
 *   scratch of the last update: double row_score[R] (the score each row entered the replay with), double row_detail[R][6],
 *           int32_t row_flags[R][8]
 * ctts_retry_state_bytes: the size, or 0 (ctts_last_error names the reason) for a config outside the limits above. */
size_t ctts_retry_state_bytes(const ctts_retry_config* cfg);
/* Byte offsets of the CTTS_RETRY_SECTIONS sections above, in that order (status, best_score, detail, tries, best_length,
 * best_T, best_pass, best_row, changed, best_mel, best_alignments, row_score, row_detail, row_flags): host code, no GPU. */
#define CTTS_RETRY_SECTIONS 14
int ctts_retry_state_layout(const ctts_retry_config* cfg, size_t* offsets);
/* :548-551: best_score = -1e5, tries = 0, no winners, status cleared. */
int ctts_retry_reset(const ctts_retry_config* cfg, void* state, void* stream);
/* One pass of :563-625 (and the loop condition of :552), three launches:
 *   (a) one flag per row: any NaN in that row of mel [rows][n_mel][T], gate [rows][T] or alignments [rows][T][enc] (:614);
 *   (b) one workgroup scores every row in IEEE double with the operation order of :598-605 from metrics [rows][6]
 *       (ctts_alignment_metric_f32's out; columns 1-5 are rounded to float32 first, which is what .item() of the reference's
 *       float32 tensors yields), max(a, b) as Python's (a unless b > a: a NaN first argument stays), no fused multiply-add;
 *       the mis_dur punishment only where text_lengths[j] > 12; a flagged row scores 1e-7 (:615; the `== float('nan')` beside
 *       it is always false).  Then :590-625 are replayed in the reference's order, texts ascending, candidates ascending:
 *       score > best_score[j] (strict: the first of equal scores wins, NaN never wins) makes the row text j's winner,
 *       tries[j] += 1, and after every candidate the stop rules of :621-625 look at min(tries) and min(best_score) over all
 *       texts; when one fires the remaining candidates of the pass are not considered (raise StopIteration).  The status
 *       block is written last;
 *   (c) every text whose winner changed copies that row's mel (and alignments when enc_cap > 0) into the state.
 * detail [rows][6] (or NULL) receives every row's six detail doubles.  output_lengths int32 [rows], text_lengths int32
 * [n_texts], both on the device.  CTTS_E_ARG before any launch for T > t_cap or enc > enc_cap > 0. */
int ctts_retry_update_f32(const ctts_retry_config* cfg, const float* mel, const float* gate, const float* alignments,
                          const double* metrics, const int32_t* output_lengths, const int32_t* text_lengths, int32_t T,
                          int32_t enc, double* detail, void* state, void* stream);
/* :645-651: mel_out [n_texts][n_mel][t_out]; element [j][m][c] = best_mel[j][m][c] for c < best_T[j], pad_value beyond (the
 * reference: -11.52).  The reference pads the winners' whole pass-length mels, so frames between a winner's output_length and
 * its pass's T keep the decoder's values.  t_out is the status block's max_best_length.  A text without a winner
 * (n_without_winner > 0) is the caller's error; its rows are all pad_value. */
int ctts_retry_vocoder_batch_f32(const ctts_retry_config* cfg, const void* state, float* mel_out, int32_t t_out,
                                 float pad_value, void* stream);
/* :675-695 for a vocoder batch audio [batch][ld] (fp32, or IEEE half with is_half != 0): of row b the first
 * min(frames[b] * hop, ld) samples (:677-678), then silence_samples zeros (:690-692: behind EVERY clip, the last one too),
 * each sample widened to fp32, multiplied by 32768 in fp32 and truncated toward zero to int16 (:695).  Two deliberate
 * differences: a product outside [-32768, 32767] saturates and NaN gives 0 (numpy's astype('int16') is platform-defined for
 * both).  Rows are written back to back in order (what the sox merge behind :707 produces); offsets [batch + 1] (device
 * int64) receives each row's first sample and the total.  A total above pcm_capacity: nothing is written beyond the
 * capacity and offsets[batch] is minus the total; batch * (ld + silence_samples) always suffices. */
int ctts_pcm16_concat(const void* audio, int32_t is_half, const int32_t* frames, int32_t batch, int64_t ld, int32_t hop,
                      int32_t silence_samples, int16_t* pcm, int64_t pcm_capacity, int64_t* offsets, void* stream);

/* ---- Tacotron2Loss on the outputs of the teacher-forced pass (_2_ttm/tacotron2_tm/loss_function.py:96-290) --------
 * No gradient: the validation loss, the per-file score table and the inference-style attention score.  Every per-item number is
 * summed on the device into one fp64 table [batch][CTTS_TACO_LOSS_COLUMNS]; the batch terms [CTTS_TACO_LOSS_TERMS] are sums over
 * that table in item order.  No float atomics: results repeat bit for bit, and an item's row does not depend on its neighbours
 * except in the two columns marked (batch).  No input is written (the reference overwrites pred_mel_postnet, :200, and the
 * alignments, utils.py:81).
 *
 * table columns:  0 mel_length   1 spec_SE   2 postnet_SE        sum over t < mel_length, m of (pred - gt)^2        (:189-202)
 *                 3 spec_MFSE    4 postnet_MFSE                  sum over t < mel_length of A_t * (A_t / n_mel), A_t = sum_m |d| (:205-213)
 *                 5 gate_BCE     sum over ALL t < T of BCEWithLogits(pos_weight)                                  (:216-218)
 *                 6 diag_att     7 diag_frames                   guided-attention numerator and mel_length; both 0 where
 *                                                                pres_prev_state != 0                              (:234-241)
 *                 8 sylps_kld    1 + logvar - exp(logvar) - mu^2     9 sylps_AE     10 sylps_SE                     (:221-232)
 *                 11-16          alignment_metric against mel_lengths: diagonality, avg_prob, max / min / avg focus, p_missing_enc (:251)
 *                 17 pred_mel_length   first frame >= 5 whose gate sigmoid reaches 0.7, else T - 1                  (:266-269)
 *                 18-23          alignment_metric against pred_mel_length on the alignments cut at mel_length       (:270)
 *                 24 att_score   :276-283 in IEEE double, Python's operation order and max(); may be NaN
 *                 25 att_score_filled  column 24 with NaN replaced by the mean of the others, as float32 (:286-287)  (batch)
 *                 26 spec_MSE    column 1 / (mel_length * n_mel), the file_losses entry (:197)
 *                 the mis_dur punishment of column 24 reads max(mel_lengths)                                          (batch)
 * terms:          0 spec_MSE  1 postnet_MSE  2 spec_MFSE  3 postnet_MFSE  4 gate_loss  5 sylps_kld  6 sylps_MAE  7 sylps_MSE
 *                 8 diag_att  9 loss = sum of terms 0-8 times weights[0-8], in that order (:152-161)
 *                 10 diagonality  11 avg_max_attention  12 weighted_score */
#define CTTS_TACO_LOSS_COLUMNS 27
#define CTTS_TACO_LOSS_TERMS 13
typedef struct {
    double gate_positive_weight;   /* hparams.gate_positive_weight */
    double sigma;                  /* hparams.DiagonalGuidedAttention_sigma */
    double weights[9];             /* the <term>_weight of terms 0-8 after loss_scalars */
} ctts_taco_loss_params;
/* 0 with a ctts_last_error message for a size below 1. */
size_t ctts_taco_loss_workspace_bytes(int32_t batch, int32_t n_mel, int32_t T, int32_t enc);
/* pred_mel, pred_mel_postnet, gt_mel [batch][n_mel][T]; gate_logits, gate_target [batch][T]; alignments [batch][T][enc];
 * sylps_mu, sylps_logvar, pred_sylps, gt_sylps, pres_prev_state fp32 [batch]; mel_lengths, text_lengths int32 [batch]; all on
 * the device, fp32 tensors contiguous.  Lengths must be at least 1; a length beyond T / enc is read as T / enc everywhere (sums,
 * counts, metrics and the score alike).
 * Eight launches: lengths (sigmoid, first five frames zeroed, first over 0.7), mel + gate pass over (64-frame tile, item), guided
 * attention over (32-frame block, item), the two metrics (two launches each), finalize (one workgroup).  A small workspace: CTTS_E_WORKSPACE. */
int ctts_taco_loss_f32(const ctts_taco_loss_params* params, const float* pred_mel, const float* pred_mel_postnet,
                       const float* gt_mel, const float* gate_logits, const float* gate_target, const float* alignments,
                       const float* sylps_mu, const float* sylps_logvar, const float* pred_sylps, const float* gt_sylps,
                       const int32_t* mel_lengths, const int32_t* text_lengths, const float* pres_prev_state, int32_t batch,
                       int32_t n_mel, int32_t T, int32_t enc, double* table, double* terms, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The finalize launch alone, on a workspace a ctts_taco_loss_f32 call of the same geometry has filled (tile partials, predicted
 * lengths).  metric_gt / metric_pred [batch][6]: the two metric tables to score, or NULL for the ones in the workspace. */
int ctts_taco_loss_finalize_f32(const ctts_taco_loss_params* params, const double* metric_gt, const double* metric_pred,
                                const float* sylps_mu, const float* sylps_logvar, const float* pred_sylps,
                                const float* gt_sylps, const int32_t* mel_lengths, const int32_t* text_lengths,
                                const float* pres_prev_state, int32_t batch, int32_t n_mel, int32_t T, int32_t enc,
                                double* table, double* terms, const void* workspace, size_t workspace_bytes, void* stream);

/* ---- Vocoder validation score: paired multi-window log-mel MSE / MAE (_4_mtw/waveglow/train.py:258-278, --------
 * _4_mtw/hifigan/train.py:205-223) ------------------------------------------------------------------------------------
 * For every item b of a batch and every STFT window w, the log-mel of the generated audio is compared with the log-mel of the
 * ground truth (or with an already-computed ground-truth log-mel), over the ground truth's frames.  Both signals are ragged: each
 * item has its own length and is reflect-padded at its own end.  All sums are fp64 in a fixed order, without atomics: results
 * repeat bit for bit and an item's row does not depend on its neighbours.  No input is written.
 *
 * table: double [batch][n_windows][CTTS_MEL_ERROR_COLUMNS] followed by CTTS_MEL_ERROR_TERMS batch terms.
 *   columns:  0 n_frames   1 SAE = sum |d|   2 SSE = sum d^2   3 MAE = SAE / (n_mel * n_frames)   4 MSE = SSE / (n_mel * n_frames)
 *   terms:    0 average_MSE  1 average_MAE: the mean over (item, window) pairs of the pair means, summed item-major and
 *             window-minor (train.py:271-278, 294-295)   2 + w: l1[w] = sum_b SAE / sum_b (n_mel * n_frames)  (hifigan/train.py:208-210)
 * n_frames(b) = min(ground-truth frames, generated frames): callers that validate lengths make that the ground truth's count. */
#define CTTS_MEL_ERROR_MAX_WINDOWS 8
#define CTTS_MEL_ERROR_COLUMNS 5
#define CTTS_MEL_ERROR_TERMS (2 + CTTS_MEL_ERROR_MAX_WINDOWS)
#define CTTS_MEL_ERROR_TACOTRON 0 /* utils/audio/stft.py:79-111: reflect-pad N/2, frames = T / hop + 1 */
#define CTTS_MEL_ERROR_NV 1       /* hifigan/nvSTFT.py:92-101: reflect-pad (N - hop) / 2, no centring, frames = (T + 2 pad - N) / hop + 1 */
#define CTTS_MEL_ERROR_SANITIZE 1 /* flags: the generated audio is read as nan_to_zero(clamp(x, -0.999, 0.999)) (train.py:259-260) */
typedef struct ctts_mel_error_config {
    int32_t n_windows;                                    /* 1 to 8 */
    int32_t filter_lengths[CTTS_MEL_ERROR_MAX_WINDOWS];   /* each a multiple of 16 in [32, 4096] */
    int32_t hop_length;
    int32_t n_mel_channels;                               /* 1 to 256 */
    int32_t framing;                                      /* CTTS_MEL_ERROR_TACOTRON | CTTS_MEL_ERROR_NV */
    float clamp_val;                                      /* log(max(., clamp_val)) */
    float mag_eps;                                        /* 0, or nvSTFT's 1e-9: the magnitude is sqrt(re^2 + im^2 + mag_eps) */
} ctts_mel_error_config;
/* 0 with a ctts_last_error message for a refused config. */
size_t ctts_mel_error_packed_bytes(const ctts_mel_error_config* cfg);
/* One call per window: forward_basis [2*(N/2+1)][N] (window folded in, as ctts_stft_pack takes it), mel_basis [n_mel][N/2+1]. */
int ctts_mel_error_pack(const ctts_mel_error_config* cfg, int32_t window, const float* forward_basis, const float* mel_basis,
                        void* packed, void* stream);
/* T_pred_max / T_gt_max: widths of the two audio tensors; T_gt_max = 0 for the gt_mel form.  0 for a refused config or size. */
size_t ctts_mel_error_workspace_bytes(const ctts_mel_error_config* cfg, int32_t batch, int32_t T_pred_max, int32_t T_gt_max);
/* pred [batch][T_pred], gt [batch][T_gt] fp32; pred_lengths, gt_lengths int32 [batch]; all on the device.  Exactly one of gt and
 * gt_mel ([batch][n_mel][mel_frames], n_windows == 1) is given; with gt_mel, gt_lengths counts FRAMES of gt_mel.  Lengths are
 * read as they are, clamped to the tensor widths; reflect indices are folded into [0, length), so no read leaves an item's row.
 * mae_map, pred_map, gt_map: all three or none; [batch][n_windows][n_mel][map_frames], written only below each item's n_frames
 * (the caller zero-fills).  Per window: framing (one launch, both signals), magnitude GEMM, fused mel-projection + error tiles;
 * then one finalize workgroup.  A small workspace: CTTS_E_WORKSPACE. */
int ctts_mel_error_f32(const ctts_mel_error_config* cfg, const void* packed, const float* pred, const int32_t* pred_lengths,
                       const float* gt, const int32_t* gt_lengths, const float* gt_mel, int32_t flags, int32_t batch,
                       int32_t T_pred, int32_t T_gt, int32_t mel_frames, double* table, float* mae_map, float* pred_map,
                       float* gt_map, int32_t map_frames, void* workspace, size_t workspace_bytes, void* stream);

/* ---- DTW: time-warp predicted mels onto the ground truth (_4_mtw/waveglow/mel2samp.py:81-118) ----------------------------------
 * pred, target, out: fp32 [batch][channels][frames], contiguous, on the device; out may alias neither input.  lengths: int32 [batch]
 * on the device or NULL (every item is `frames` long).  Item b is treated exactly as the reference treats pred[b, :, :len_b] alone
 * (its zero frames begin at len_b); columns t >= len_b of out are copied from pred.  A value of the device array outside [1, frames]
 * is read as the nearest bound (callers that hold the lengths on the host check them there).
 * With s = scale_factor, r = range (odd), h = r / 2: candidate j in [0, s r) at frame t is the zero-padded prediction, linearly
 * interpolated to s times its length (align_corners=False, source index max(0, float(1 / s) (p + 0.5) - 0.5) at p = j + t s, all fp32).
 * The (i0 - t, 1 - lambda, lambda) triple of each j is formed on the host in fp32; a candidate is w0 x0 + w1 x1 with both products rounded.
 * The running best starts as pred itself; candidates are tried in ascending j and replace it only when their sum_c |cand - target| is
 * STRICTLY smaller: pred wins every tie, an earlier candidate wins a tie with a later one, a NaN sum never wins.  The sums are fp32 in a
 * fixed order (channels ascending inside each of four channel slices, slices ascending): results repeat bit for bit.
 * choice (or NULL): int32 [batch][frames], the winning j, or -1 for the unshifted frame and for t >= len_b.
 * l1 (or NULL): fp32 [batch][2][frames], the L1 of the unshifted frame and of the winner (0 for t >= len_b).
 * Accepted: range odd, scale_factor >= 1, scale_factor * range <= 64, batch <= 65535; anything else is CTTS_E_ARG before any launch.
 * One launch, no workspace, no atomics.  (8, 5), (5, 5) and (5, 3) - the reference's three option sets - run compile-time variants of
 * the kernel; ctts_mel_dtw_generic_f32 is the same call held to the generic form (same bits; the tests say so). */
int ctts_mel_dtw_f32(const float* pred, const float* target, const int32_t* lengths, float* out, int32_t* choice, float* l1,
                     int32_t batch, int32_t channels, int32_t frames, int32_t scale_factor, int32_t range, void* stream);
int ctts_mel_dtw_generic_f32(const float* pred, const float* target, const int32_t* lengths, float* out, int32_t* choice, float* l1,
                             int32_t batch, int32_t channels, int32_t frames, int32_t scale_factor, int32_t range, void* stream);

/* ---- main loop of the fp32 conv-GEMM ------------------------------------------------------------------------
 * Every fp32 path of the library (WaveGlow fp32, WaveFlow, the ax WaveGlow, conv1d / LSTM input projections, STFT)
 * goes through one conv-GEMM.  mode 0 (default): v_mfma_f32_32x32x2_f32, exact fp32 products.  mode 1 ("split bf16"):
 * the same kernel, tensors, packed weights and epilogues, but each operand value is split in registers into
 * hi = bf16(v), lo = bf16(v - hi) and each product is computed as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation: operands carry 16 mantissa bits (relative product error ~2^-16), the matrix pipe does
 * 3/16 of the cycles.  mode 2 ("split bf16 x6"): hi + mid + lo (24 mantissa bits = the whole fp32 operand) and the six
 * products of weight >= 2^-16 (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi, accumulated smallest first; the three dropped
 * ones are <= 2^-24 relative): fp32-grade results at 6/16 of the fp32 matrix-pipe cycles (tests/test_gemm_mode.py holds
 * its error against the reference goldens within 2x of the fp32 MFMA path's).
 * The mode is part of each model's config struct (f32_gemm_mode = CTTS_GEMM_F32 | CTTS_GEMM_BF16X3 | CTTS_GEMM_BF16X6), so two models in one
 * process can differ and nothing races with in-flight calls.  The STFT entry points always compute in fp32 MFMA (their
 * sums cancel).
 *
 * Which loop a launch really runs also depends on its SHAPE (all of it deterministic in the arguments, none of it in the
 * environment): the fused WaveFlow layer (C = 64) runs the fp32-MFMA split-K shape whenever ntiles * batch <= 128
 * (B <= 2 at 900 frames) under EVERY mode - and, under fp32 MFMA, as the item body of the row queue while a layer has 200-399
 * column tiles of 128 (B = 2-3 at 900 frames) - and the fused separable layer (C = 128) runs fp32 MFMA under CTTS_GEMM_BF16X6;
 * the split-K shape sums in a different order than the other shapes, so the same utterance is bit-identical across
 * batch sizes only within one shape (CTTS_F32_NO_SPLITK: one K order at every size).  ctts_last_gemm_loop() reports what the most recent conv-GEMM launch of the calling
 * thread ran, so that a benchmark row can label itself: bits 0-3 = split level (0 fp32 MFMA, 3, 6), bit 4 = small shape,
 * bit 5 = split-K shape, bit 6 = the WaveFlow row queue, bit 7 = its whole-flow form (one launch per flow, see ctts_waveflow_inverse_f32),
 * bit 8 = the all-rows layer of the WaveFlow analysis pass (ctts_waveflow_forward_*).
 *
 * REMOVED: the process-wide default of ABI <= 5 (ctts_set_f32_gemm_mode / ctts_get_f32_gemm_mode; no-ops in ABI 6, gone in 7):
 * hidden state shared by every model and thread of a process.  CTTS_GEMM_DEFAULT (0) in a config struct always means fp32
 * MFMA, and so do the two entry points without a config struct (ctts_lstm_seq_f32's input projection,
 * ctts_taco_decoder_init_f32's processed memory). */
int ctts_last_gemm_loop(void);
/* Quad columns per workgroup (64 or 128) of the calling thread's most recent Winograd F(4,3) in-layer launch of the fp32 WaveGlow; 0
 * before the first.  64 always, unless CTTS_F32_NO_SMALL selects the 128-column one-workgroup-per-CU shape (an A/B arm; same bits). */
int ctts_last_winograd_f43_width(void);

/* Launch-shape overrides for A/B measurements (CTTS_F32_NO_GLDS, CTTS_F32_NO_SMALL, CTTS_F32_FORCE_SMALL, CTTS_GEMM_NO_XCD_PAIR, CTTS_BF16_NO_WIDE /
 * _NO_PP / _PS / _NO_PS / _WIDE_MIN, CTTS_WF_NO_FUSE, CTTS_WF_NO_VEC_INTERP, CTTS_WF_NO_REGION_SPLIT, CTTS_WF_NO_ROW_QUEUE, CTTS_F32_NO_ROUND_SPLIT, CTTS_TACO_POLL_DELAY, CTTS_TACO_NO_FUSE, CTTS_TACO_BG_NO_PIPE, CTTS_UP_NO_MFMA, CTTS_F32_NO_WN_FOLD, CTTS_F32_NO_WINOGRAD, CTTS_F32_WINOGRAD_MIN, CTTS_F32_WINOGRAD_PLAIN, CTTS_F32_WINOGRAD_FUSED_MIN, CTTS_F32_WINOGRAD_NO_FUSED, CTTS_F32_WINOGRAD_F43_MIN, CTTS_F32_WINOGRAD_NO_F43, CTTS_F32_WINOGRAD_F63_MIN, CTTS_F32_WINOGRAD_NO_F63) never change results beyond the parity
 * tolerance (CTTS_F32_NO_SPLITK changes the summation order of the fused WaveFlow layer at batch <= 2, see above; CTTS_F32_NO_WN_FOLD
 * brings back the fp32 WaveGlow WN stack without the start / end folds: WN layer 0 on the C-row x, the C-row deferred skip GEMM and the
 * C-row flow tail - the default folds W_in,0 . W_start into layer 0 and W_end . W_skip,i into a 2 n_half-row skip/end pass, which only
 * reorders sums; CTTS_F32_NO_WINOGRAD keeps the direct 3-tap in-layer GEMM of the fp32 WaveGlow at every size - by default
 * ctts_waveglow_infer_*_f32 computes the in-layer conv of the layers that read x as Winograd F(2,3) on output pairs (t, t + d), four
 * short-K launches of the same conv-GEMM behind a transform kernel, for utterances of at least CTTS_F32_WINOGRAD_MIN columns
 * (steps per batch item; 0 = always; only under the fp32 MFMA loop).  The threshold looks at the utterance, not at the batch: an
 * utterance keeps its bits whatever batch it runs in; one just below and one just above the threshold differ within the parity
 * tolerance.  CTTS_F32_WINOGRAD_PLAIN runs that form as the five launches per layer it was first built as - cond rows copied into
 * pair order for every layer, T2 / T3 and even / odd as four launches - where the default reads the cond rows in place and pairs
 * the launches: bit-identical, the A/B arm.  For utterances of at least CTTS_F32_WINOGRAD_FUSED_MIN columns (default: the Winograd
 * form's own default threshold; 0 = always; again the utterance alone decides) a Winograd layer is ONE launch behind the transform
 * kernel: a workgroup runs the four products of a pair block through one chunk stream and T2 / T3 stay in registers -
 * ((S2 +- S3) + products) + b where the paired launches round ((products + b) + T2) +- T3, a re-ordered sum.
 * CTTS_F32_WINOGRAD_NO_FUSED keeps the paired launches at every size: the A/B arm.  Where the one-launch layer engages, utterances
 * of at least CTTS_F32_WINOGRAD_F43_MIN columns (default 28 800; 0 = always; the utterance alone decides) run it as Winograd F(4,3)
 * on output quads (t, t + d, t + 2d, t + 3d), interpolation points 0, +-1, +-2, inf: 1.5 C products per output and row where F(2,3)
 * spends 2 C, four interior products combined in registers with the exact multipliers 1, 2, 4, 8, the transformed filters formed
 * in fp64 and rounded once; the float64 parity of a flow stays inside the bound of the other forms.  CTTS_F32_WINOGRAD_NO_F43
 * keeps the F(2,3) one-launch layer at every size: the A/B arm, bit-equal to the library before the F(4,3) form; whatever
 * switches the one-launch layer off switches the F(4,3) form off with it.  Where the F(4,3) form engages, utterances of at least
 * CTTS_F32_WINOGRAD_F63_MIN columns (default 28 800; 0 = always; the utterance alone decides) run its layers of dilation d % 4 == 0
 * as Winograd F(6,3) on output hexes (t, t + d, .., t + 5d), interpolation points 0, +-1, +-2, +-1/2, inf: 8/6 C products per output
 * and row, six interior products combined in registers with the exact multipliers 2^-5 .. 2^5, the transformed filters formed in fp64
 * and rounded once; the d = 2 layer keeps F(4,3); the float64 parity of a flow stays inside the bound of the other forms.
 * CTTS_F32_WINOGRAD_NO_F63 keeps the F(4,3) layer wherever it engages: the A/B arm, bit-equal to the library before the F(6,3)
 * form).  The environment is read once,
 * at the first launch; this re-reads it (tests and profiling scripts that flip a knob in-process). */
int ctts_tuning_reload(void);
/* The knobs as the library currently sees them: bit 0 CTTS_F32_NO_GLDS, 1 CTTS_GEMM_NO_XCD_PAIR, 2 CTTS_F32_WINOGRAD_FUSED_MIN set,
 * 5 CTTS_F32_WINOGRAD_NO_FUSED, 6 CTTS_F32_WINOGRAD_F43_MIN set, 22 CTTS_F32_WINOGRAD_NO_F43,
 * 3 CTTS_BF16_NO_WIDE, 4 CTTS_BF16_NO_PP, 7 CTTS_WF_NO_FUSE, 8 CTTS_TACO_NO_FUSE,
 * 9 CTTS_F32_NO_SMALL, 10 CTTS_F32_FORCE_SMALL, 11 CTTS_F32_NO_SPLITK, 12 CTTS_WF_NO_VEC_INTERP, 13 CTTS_F32_NO_DEFER_SKIP, 14 CTTS_WF_NO_REGION_SPLIT,
 * 15 CTTS_WF_NO_ROW_QUEUE, 16 CTTS_WF_ROW_QUEUE_MIN set, 17 CTTS_WF_INJECT_ABORT, 18 CTTS_WF_QUEUE_DEBUG != 0, 19 CTTS_F32_NO_ROUND_SPLIT,
 * 20 CTTS_BF16_PS (persistent form of the skewed bf16 kernel on every wide launch), 21 CTTS_BF16_NO_PS, 23 CTTS_TACO_POLL_DELAY set ("a,c,d,e,h,p": 64-cycle units
 * before the first poll of the persistent decoder's six vector exchanges; timing only), 24 CTTS_TACO_VALU
 * (ctts_taco_decoder_steps_f32 at batch <= 4 on the VALU kernels instead of the batched MFMA form), 25 CTTS_UP_NO_MFMA (the VALU upsampling kernel
 * also for the shape the MFMA one is built for: bit-identical), 26 CTTS_F32_NO_WN_FOLD, 27 CTTS_TACO_BG_NO_PIPE (the batched
 * decoder's plain schedule, the default above 64 rows, at every size), 28 CTTS_F32_NO_WINOGRAD, 29 CTTS_F32_WINOGRAD_MIN set, 30 CTTS_F32_WINOGRAD_PLAIN,
 * 31 CTTS_WF_FWD_ROWWISE (the sign bit of the int: the WaveFlow analysis pass row by row, see ctts_waveflow_forward_f32).  Bits 2, 5, 6 and 22 belonged to retired knobs until the one-launch Winograd layer (2, 5) and its F(4,3) form (6, 22) took them.
 * (Tests assert that a knob they set is the one in effect.) */
int ctts_tuning_flags(void);
/* The knobs beyond the int above, counted on: bit 32 CTTS_F32_WINOGRAD_F63_MIN set, 33 CTTS_F32_WINOGRAD_NO_F63 (bit 0 and 1 of this
 * value). */
int ctts_tuning_flags_ext(void);

/* ---- in-library kernel timing (bench.py roofline leg) ---------------------------------
 * A profile is an opaque caller-owned handle (ABI 6; until ABI 5 one set of process-global slots).  A thread that has
 * BOUND a handle brackets every launch of the WN GEMMs it issues (ctts_waveglow_infer_* on that thread) with hipEvents on
 * the launch's stream and files them in the handle; ctts_profile_bind(NULL) stops recording on the calling thread.  Two
 * threads with two handles never see each other's launches.  collect synchronises the recorded events of one slot,
 * returns launches + summed milliseconds and empties the slot.  destroy: no thread may still be bound to the handle. */
#define CTTS_PROF_WN_IN 0
#define CTTS_PROF_WN_RS 1   /* fp32: res/skip GEMM; bf16: res GEMM (x += W_res act) */
#define CTTS_PROF_WN_SKIP 2 /* deferred skip GEMM over K = (layers of the group) * C */
/* fp32 with the WN folds (the default; CTTS_F32_NO_WN_FOLD = slots 0-2 only).  Slot 0 still brackets every in-layer launch, the
 * short folded layer-0 launch included (one entry per layer); slot 3 has that launch alone, so that a reader pricing slot 0 at the
 * full-K FLOP count can take it out.  In the Winograd form (CTTS_F32_NO_WINOGRAD turns it off) a slot-0 entry brackets a layer's
 * transform kernel and its launches (one, two or four), which execute 5/7 of the full-K FLOPs: priced at the full-K count it reads high too.  The skip/end pass and the res GEMM of this form record in slots of their own. */
#define CTTS_PROF_WN_IN0F 3  /* layer 0's in-layer GEMM on the folded start: K = 3 x 16 + cond (also in slot 0) */
#define CTTS_PROF_WN_SKEND 4 /* skip/end pass: 2 n_half rows of W_end . W_skip over a group's kept activations (+ the flow tail) */
#define CTTS_PROF_WN_RES_F 5 /* res GEMM (x += W_res act) of the folded form */
#define CTTS_PROF_N 6
int ctts_profile_create(void** handle);
int ctts_profile_bind(void* handle);
int ctts_profile_collect(void* handle, int32_t which, int64_t* launches, double* total_ms);
int ctts_profile_destroy(void* handle);

#ifdef __cplusplus
}
#endif
#endif /* COOKIETTS_HIP_H */
