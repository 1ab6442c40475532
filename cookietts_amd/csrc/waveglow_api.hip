// C ABI of the WaveGlow (glow.py topology) mel->wave path: packed-weight layout, workspace
// layout and the launch sequence.  See include/cookietts_hip.h for the contract.
#include <mutex>
#include <vector>

#include "gemm_bf16.h"
#include "gemm_f32.h"
#include "tuning.h"
#include "waveglow_kernels.h"
#include "wn_winograd_layer.h"

namespace ctts {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

constexpr size_t ALIGN_F = 64;  // section alignment in floats (256 B)
inline size_t align_up(size_t v) { return (v + ALIGN_F - 1) / ALIGN_F * ALIGN_F; }
constexpr int A_TILE = GEMM_KC * GEMM_BM;

struct FlowDims { int n_rem, n_half, ch_off; };

struct Plan {
    ctts_waveglow_config c;
    int C, H, K0, n_in;                 // WN channels, cond hidden, n_mel*G, flows
    int S;                              // speaker-embedding rows per flow, padded to a multiple of 32 (0: single speaker)
    int nch0, nch1h, nch_in, nch_rs;    // K chunks: cond0, cond1, in-layer, res/skip
    int mb_in;                          // M-blocks of the in-layer GEMM
    int nch_in0f;                       // K chunks of layer 0's in-layer GEMM on the folded start: one per tap + cond
    std::vector<FlowDims> fd;
    // packed blob offsets (floats)
    size_t up_w, up_wp, up_b, cond0_A, cond0_b, cond1_A, cond1_b;
    size_t zero_b;                      // mb_in * GEMM_BM zeros (never written; the blob is zero-filled): bias of the Winograd T launches
    bool up_mfma;
    // Composed conditioning (cond_composed_packed below): upsampling, trim, squeeze and cond layers 0 and 1 are one linear map of the
    // mel frames, packed as ONE conv-GEMM A panel over K = ccJ taps x n_mel, M = n_flows x ccP phases x H.  cc_A [n_flows ccP][nch_cc]
    // A tiles, cc_b [n_flows ccP][GEMM_BM] bias in block-local row order, cc_w10 pack-time scratch: W1 W0 in double [n_flows][H][K0]
    bool cc;                            // the blob holds it (asked for with CTTS_WG_OPT_COMPOSED_COND, and the shape allows it)
    int ccP, ccJ, nch_cc;               // phases per frame hop / n_group, taps win / hop, K chunks ccJ n_mel / 16
    size_t cc_A, cc_b, cc_w10;
    struct Flow {
        size_t start_w, start_b, end_w, end_b, winv, spk_tab;
        std::vector<size_t> in_A, in_b, rs_A, rs_b;
        // deferred-skip form (round 4, profiles/r4_07_res_skip_experiments.txt): res rows per layer, skip rows of a group of
        // up to F32_SKIP_GROUP layers side by side along K
        std::vector<size_t> res_A, res_b, skip_A, skip_b;
        // WN start / end folds (round 7): in0f_w = W_in,0[tap] . [W_start | b_start] as a dense [2C][FOLD_ROWS][ks] in_w, in0f_A its
        // packed GATE matrix (+ the cond slice; bias = in_b[0]); skend_W = W_end . W_skip,i as [n_layers][C][2 n_half], skend_b = b'
        size_t in0f_w, in0f_A, skend_W, skend_b;
        // Winograd F(2,3) in-layer form (round 12): per layer G2 and G3 in SPLIT packing (K = C), [W0 | C_i] and [-W2 | C_i] in
        // GATE packing (K = C + H; bias = in_b[i]); wg_dense = the dense [3][2C][C] G2, G3, -W2 of the layer being packed
        std::vector<size_t> wg_T2_A, wg_T3_A, wg_e_A, wg_o_A;
        size_t wg_dense;
        // Winograd F(4,3) form of the one-launch layer (where wn_winograd_layer_f43_supported; empty otherwise): per layer U1..U4 in
        // SPLIT packing (K = C), [U0 | C_i] and [U5 | C_i] in GATE packing (K = C + H); wg_dense then holds the dense [6][2C][C] U0..U5
        std::vector<size_t> wq_U_A[4], wq_e_A, wq_o_A;
        // Winograd F(6,3) form (where wn_winograd_layer_f63_supported, for the layers it can engage at: d % 4 == 0; 0 elsewhere): U1..U6
        // in SPLIT packing, [U0 | C_i] and [U7 | C_i] in GATE packing; wg_dense then holds the dense [8][2C][C] U0..U7
        std::vector<size_t> wh_U_A[6], wh_e_A, wh_o_A;
    };
    std::vector<Flow> fl;
    size_t total;

    static constexpr int F32_SKIP_GROUP = 4;
    int mb_c() const { return (C + GEMM_BM - 1) / GEMM_BM; }
    int n_groups() const { return (c.n_layers + F32_SKIP_GROUP - 1) / F32_SKIP_GROUP; }
    int group_layers(int g) const { return g + 1 < n_groups() ? F32_SKIP_GROUP : c.n_layers - g * F32_SKIP_GROUP; }
    int rs_rows(int layer) const { return layer < c.n_layers - 1 ? 2 * C : C; }
    int rs_mb(int layer) const { return (rs_rows(layer) + GEMM_BM - 1) / GEMM_BM; }
};

// the layers the F(6,3) form can engage at: the cond rows are read in place through the hex map, four consecutive aligned columns per
// lane (d % 4 == 0); d = 2 keeps F(4,3) (it would need six cond copies and a second transform path)
bool f63_layer(int layer) { return (1 << layer) % 4 == 0; }

// options: CTTS_WG_OPT_* of the `_opt` entry points (0: what the entry points without the argument run)
int make_plan(const ctts_waveglow_config* cfg, Plan& p, int options = 0) {
    CTTS_CHECK_ARG(cfg != nullptr, "config is NULL");
    p.c = *cfg;
    CTTS_CHECK_ARG((options & ~CTTS_WG_OPT_COMPOSED_COND) == 0, "options=%d (CTTS_WG_OPT_*)", options);
    const bool want_cc = (options & CTTS_WG_OPT_COMPOSED_COND) != 0;
    const auto& c = p.c;
    CTTS_CHECK_ARG(c.n_flows >= 1 && c.n_layers >= 1 && c.n_layers <= 12, "n_flows=%d n_layers=%d", c.n_flows, c.n_layers);
    CTTS_CHECK_ARG(gemm_mode_valid(c.f32_gemm_mode), "f32_gemm_mode=%d (CTTS_GEMM_DEFAULT / _F32 / _BF16X3 / _BF16X6)", c.f32_gemm_mode);
    CTTS_CHECK_ARG(c.n_group >= 4 && c.n_group % 4 == 0 && c.n_group <= 16, "n_group=%d (4, 8, 12 or 16)", c.n_group);
    CTTS_CHECK_ARG(c.kernel_size == 3, "kernel_size=%d (only 3 built)", c.kernel_size);
    CTTS_CHECK_ARG(c.n_channels >= 128 && c.n_channels % 128 == 0, "n_channels=%d (multiple of 128)", c.n_channels);
    CTTS_CHECK_ARG(c.cond_hidden == GEMM_BM, "cond_hidden=%d (reference hard-codes 256)", c.cond_hidden);
    CTTS_CHECK_ARG(c.hop_length > 0 && c.win_length % c.hop_length == 0 && c.hop_length % c.n_group == 0,
                   "win=%d hop=%d n_group=%d", c.win_length, c.hop_length, c.n_group);
    CTTS_CHECK_ARG((c.n_mel_channels * c.n_group) % GEMM_KC == 0, "n_mel*n_group=%d not a multiple of 16",
                   c.n_mel_channels * c.n_group);
    CTTS_CHECK_ARG(c.n_early_every >= 1 && c.n_early_size >= 0 && c.n_early_size % 2 == 0, "early outputs");
    CTTS_CHECK_ARG(c.speaker_embed_dim >= 0 && c.speaker_embed_dim <= 1024, "speaker_embed_dim=%d", c.speaker_embed_dim);
    p.C = c.n_channels;
    p.H = c.cond_hidden;
    p.K0 = c.n_mel_channels * c.n_group;
    p.S = round_up(c.speaker_embed_dim, 32);
    CTTS_CHECK_ARG(p.S == 0 || p.K0 % 32 == 0, "multispeaker needs n_mel*n_group %% 32 == 0");
    p.nch0 = (p.K0 + p.S) / GEMM_KC;
    p.nch1h = p.H / GEMM_KC;
    p.nch_in = (c.kernel_size * p.C + p.H) / GEMM_KC;
    p.nch_rs = p.C / GEMM_KC;
    p.mb_in = 2 * p.C / GEMM_BM;
    p.nch_in0f = c.kernel_size + p.nch1h;
    // per-flow channel counts exactly as glow.py:251-265
    int n_half = c.n_group / 2, n_rem = c.n_group;
    p.fd.resize(c.n_flows);
    for (int k = 0; k < c.n_flows; ++k) {
        if (k % c.n_early_every == 0 && k > 0) { n_half -= c.n_early_size / 2; n_rem -= c.n_early_size; }
        CTTS_CHECK_ARG(n_half >= 1 && n_rem == 2 * n_half, "flow %d: n_half=%d n_remaining=%d", k, n_half, n_rem);
        p.fd[k] = {n_rem, n_half, c.n_group - n_rem};
    }
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n); return r; };
    p.up_w = take((size_t)c.n_mel_channels * c.n_mel_channels * c.win_length);
    // the same weights in MFMA fragment order, for the shape the MFMA upsampling kernel is built for (waveglow_kernels.hip)
    p.up_mfma = upsample_mfma_shape(c.n_mel_channels, c.win_length, c.hop_length, c.n_group);
    p.up_wp = p.up_mfma ? take((size_t)c.n_mel_channels * c.n_mel_channels * c.win_length) : 0;
    p.up_b = take(c.n_mel_channels);
    p.cond0_A = take((size_t)c.n_flows * p.nch0 * A_TILE);
    p.cond0_b = take((size_t)c.n_flows * GEMM_BM);
    p.cond1_A = take((size_t)c.n_flows * p.nch1h * A_TILE);
    p.cond1_b = take((size_t)c.n_flows * GEMM_BM);
    p.zero_b = take((size_t)p.mb_in * GEMM_BM);
    p.fl.resize(c.n_flows);
    for (int k = 0; k < c.n_flows; ++k) {
        auto& f = p.fl[k];
        f.start_w = take((size_t)p.C * p.fd[k].n_half);
        f.start_b = take(p.C);
        f.end_w = take((size_t)2 * p.fd[k].n_half * p.C);
        f.end_b = take(2 * p.fd[k].n_half);
        f.winv = take((size_t)p.fd[k].n_rem * p.fd[k].n_rem);
        f.spk_tab = take((size_t)CTTS_N_SPEAKERS * c.speaker_embed_dim);
        for (int i = 0; i < c.n_layers; ++i) {
            f.in_A.push_back(take((size_t)p.mb_in * p.nch_in * A_TILE));
            f.in_b.push_back(take((size_t)p.mb_in * GEMM_BM));
            f.rs_A.push_back(take((size_t)p.rs_mb(i) * p.nch_rs * A_TILE));
            f.rs_b.push_back(take((size_t)p.rs_mb(i) * GEMM_BM));
            f.res_A.push_back(i + 1 < c.n_layers ? take((size_t)p.mb_c() * p.nch_rs * A_TILE) : 0);
            f.res_b.push_back(i + 1 < c.n_layers ? take((size_t)p.mb_c() * GEMM_BM) : 0);
        }
        for (int gi = 0; gi < p.n_groups(); ++gi) {
            f.skip_A.push_back(take((size_t)p.mb_c() * p.group_layers(gi) * p.nch_rs * A_TILE));
            f.skip_b.push_back(take((size_t)p.mb_c() * GEMM_BM));
        }
        f.in0f_w = take((size_t)2 * p.C * FOLD_ROWS * c.kernel_size);
        f.in0f_A = take((size_t)p.mb_in * p.nch_in0f * A_TILE);
        f.skend_W = take((size_t)c.n_layers * p.C * 2 * p.fd[k].n_half);
        f.skend_b = take(2 * p.fd[k].n_half);
        for (int i = 0; i < c.n_layers; ++i) {
            f.wg_T2_A.push_back(take((size_t)p.mb_in * p.nch_rs * A_TILE));
            f.wg_T3_A.push_back(take((size_t)p.mb_in * p.nch_rs * A_TILE));
            f.wg_e_A.push_back(take((size_t)p.mb_in * (p.nch_rs + p.nch1h) * A_TILE));
            f.wg_o_A.push_back(take((size_t)p.mb_in * (p.nch_rs + p.nch1h) * A_TILE));
        }
        const bool f43 = wn_winograd_layer_f43_supported(p.C, p.H);
        for (int i = 0; f43 && i < c.n_layers; ++i) {
            for (auto& u : f.wq_U_A) u.push_back(take((size_t)p.mb_in * p.nch_rs * A_TILE));
            f.wq_e_A.push_back(take((size_t)p.mb_in * (p.nch_rs + p.nch1h) * A_TILE));
            f.wq_o_A.push_back(take((size_t)p.mb_in * (p.nch_rs + p.nch1h) * A_TILE));
        }
        const bool f63 = wn_winograd_layer_f63_supported(p.C, p.H);
        for (int i = 0; f63 && i < c.n_layers; ++i) {
            const bool on = f63_layer(i);
            for (auto& u : f.wh_U_A) u.push_back(on ? take((size_t)p.mb_in * p.nch_rs * A_TILE) : 0);
            f.wh_e_A.push_back(on ? take((size_t)p.mb_in * (p.nch_rs + p.nch1h) * A_TILE) : 0);
            f.wh_o_A.push_back(on ? take((size_t)p.mb_in * (p.nch_rs + p.nch1h) * A_TILE) : 0);
        }
        f.wg_dense = take((size_t)(f63 ? 8 : f43 ? 6 : 3) * 2 * p.C * p.C);
    }
    // composed conditioning, behind everything else (a blob without it is a prefix of one with it): single speaker, whole 16-row K
    // chunks per tap, at most four taps (one K segment each), and P a power of two in [4, 256] - whole 16-byte stores, and an
    // M-block holds whole hidden rows.  (A layout question only: the mode of the model's GEMMs is asked at the call, cond_composed.)
    p.ccP = c.hop_length / c.n_group;
    p.ccJ = c.win_length / c.hop_length;
    p.nch_cc = p.ccJ * c.n_mel_channels / GEMM_KC;
    p.cc = want_cc && p.S == 0 && c.n_mel_channels % GEMM_KC == 0 && p.ccJ >= 1 && p.ccJ <= 4 && p.ccP >= 4 && p.ccP <= GEMM_BM &&
           (p.ccP & (p.ccP - 1)) == 0;
    p.cc_A = p.cc_b = p.cc_w10 = 0;
    if (p.cc) {
        p.cc_A = take((size_t)c.n_flows * p.ccP * p.nch_cc * A_TILE);
        p.cc_b = take((size_t)c.n_flows * p.ccP * GEMM_BM);
        p.cc_w10 = take((size_t)c.n_flows * 2 * p.H * p.K0);
    }
    p.total = o;
    return CTTS_OK;
}

struct Geom { int L, ld, pad, ntiles; };

int make_geom(const Plan& p, int frames, Geom& g) {
    CTTS_CHECK_ARG(frames >= 1, "frames=%d", frames);
    const long long T = (long long)frames * p.c.hop_length;
    g.L = (int)(T / p.c.n_group);
    int maxd = 1 << (p.c.n_layers - 1);
    g.pad = round_up(maxd > 128 ? maxd : 128, 32);
    g.ntiles = (g.L + GEMM_BN - 1) / GEMM_BN;
    g.ld = round_up(g.L, 256) + 2 * g.pad;          // room for the 256-wide tiles of the bf16 GEMM
    return CTTS_OK;
}

// Winograd F(2,3) in-layer form: pair-space geometry of layer i (dilation d = 2^i): Lp = ceil(L / 2d) d pair columns per batch
// item, in ntiles 128-column tiles; every layer uses the row stride ldp of the widest one
struct PairGeom { int d, Lp, ntiles; };
PairGeom pair_geom(const Geom& g, int layer) {
    const int d = 1 << layer;
    const int Lp = (g.L + 2 * d - 1) / (2 * d) * d;
    return {d, Lp, (Lp + GEMM_BN - 1) / GEMM_BN};
}
int pair_ld(const Plan& p, const Geom& g) {
    int nt = 0;
    for (int i = 0; i < p.c.n_layers; ++i) nt = std::max(nt, pair_geom(g, i).ntiles);
    return nt * GEMM_BN;
}
// Winograd F(4,3) form: quad-space geometry of layer i: Lq = ceil(L / 4d) d quad columns per batch item, in ntiles 64-column tiles;
// every layer uses the row stride ldq of the widest one, in whole 128-column tiles (the CTTS_F32_NO_SMALL shape of the layer)
PairGeom quad_geom(const Geom& g, int layer) {
    const int d = 1 << layer;
    const int Lq = (g.L + 4 * d - 1) / (4 * d) * d;
    return {d, Lq, (Lq + 63) / 64};
}
int quad_ld(const Plan& p, const Geom& g) {
    int nt = 0;
    for (int i = 0; i < p.c.n_layers; ++i) nt = std::max(nt, quad_geom(g, i).ntiles);
    return round_up(nt * 64, 128);
}
// Winograd F(6,3) form: hex-space geometry of layer i: Lh = ceil(L / 6d) d hex columns per batch item, in ntiles 64-column tiles
PairGeom hex_geom(const Geom& g, int layer) {
    const int d = 1 << layer;
    const int Lh = (g.L + 6 * d - 1) / (6 * d) * d;
    return {d, Lh, (Lh + 63) / 64};
}
int hex_ld(const Plan& p, const Geom& g) {
    int nt = 0;
    for (int i = 0; i < p.c.n_layers; ++i) nt = std::max(nt, hex_geom(g, i).ntiles);
    return nt * 64;
}
// ---- the in-layer form of a call ---------------------------------------------------
// Decided once from (plan, geometry, one tuning snapshot): carve() sizes the buffers from it and WnCall launches from it.
//   Direct            one GATE launch on the three x taps
//   WinogradSeparate  transform, T2, T3, even, odd as launches of their own, cond rows copied for every layer
//                     (CTTS_F32_WINOGRAD_PLAIN, or the register-staged conv-GEMM): the bit reference of WinogradPaired
//   WinogradPaired    transform, T2 | T3 as the parts of one launch, even | odd as the parts of another
//   WinogradLayer     transform, then the one-launch F(2,3) layer (wn_winograd_layer.hip: T2 / T3 stay in registers).  Not bit-equal
//                     to the paired launches: ((S2 +- S3) + products) + b against ((products + b) + T2) +- T3
//   WinogradLayerF43  quad transform, then the one-launch F(4,3) layer (1.5 C products per output and row where F(2,3) spends 2 C).
//                     Not bit-equal to F(2,3): other products (float64 parity: tests/test_waveglow_winograd_f43_gpu.py)
//   WinogradLayerF63  WinogradLayerF43 whose layers with d % 4 == 0 run the F(6,3) form: hex transform, then the one-launch F(6,3) layer
//                     (8/6 C products per output and row).  Not bit-equal to F(4,3): other products
//                     (float64 parity: tests/test_waveglow_winograd_f63_gpu.py)
// Every test is on the utterance (columns = steps per batch item), never on the batch: an utterance must come out bit for bit the
// same whatever batch it runs in (tests/test_full_size.py), and each form is bit-identical across the kernel shapes a batch picks.
enum class InForm { Direct, WinogradSeparate, WinogradPaired, WinogradLayer, WinogradLayerF43, WinogradLayerF63 };
bool quad_space(InForm in) { return in == InForm::WinogradLayerF43 || in == InForm::WinogradLayerF63; }

// Each threshold is the length its A/B was run at (900 frames).  Winograd at all: profiles/r12_02_winograd_ab.txt,
// r12_04_winograd_sweep.txt; CTTS_F32_WINOGRAD_MIN: another threshold (0 = always), CTTS_F32_NO_WINOGRAD: never.
constexpr long long WINOGRAD_MIN_COLS = 28800;
// The one-launch layer: profiles/r17_01_winograd_fused_ab.txt; shorter utterances keep the paired launches.
// CTTS_F32_WINOGRAD_FUSED_MIN: another threshold; CTTS_F32_WINOGRAD_NO_FUSED, _PLAIN or CTTS_F32_NO_GLDS: never.
constexpr long long WINOGRAD_FUSED_MIN_COLS = 28800;
// Its F(4,3) form: profiles/r23_01_winograd_f43_gonogo.txt.  CTTS_F32_WINOGRAD_F43_MIN: another threshold;
// CTTS_F32_WINOGRAD_NO_F43, and whatever switches the one-launch layer off: never.
constexpr long long WINOGRAD_F43_MIN_COLS = 28800;
// The F(6,3) form of its d % 4 == 0 layers: profiles/r34_01_winograd_f63_gonogo.txt.  CTTS_F32_WINOGRAD_F63_MIN: another threshold;
// CTTS_F32_WINOGRAD_NO_F63, and whatever switches the F(4,3) form off: never.
constexpr long long WINOGRAD_F63_MIN_COLS = 28800;

InForm in_form(const Plan& p, const Geom& g, const Tuning& t) {
    auto long_enough = [&](int knob, long long cols) { return (long long)g.L >= (knob >= 0 ? knob : cols); };
    // only where the in-layer launch runs the fp32 MFMA loop
    if (t.f32_no_winograd || gemm_split_level(p.c.f32_gemm_mode) != 0 || !long_enough(t.f32_winograd_min, WINOGRAD_MIN_COLS))
        return InForm::Direct;
    if (t.f32_winograd_plain || !gemm_f32_dma_staged(p.nch_rs + p.nch1h)) return InForm::WinogradSeparate;
    if (t.f32_winograd_no_fused || t.f32_no_glds || !wn_winograd_layer_supported(p.C, p.H) ||
        !long_enough(t.f32_winograd_fused_min, WINOGRAD_FUSED_MIN_COLS))
        return InForm::WinogradPaired;
    if (t.f32_winograd_no_f43 || !wn_winograd_layer_f43_supported(p.C, p.H) || !long_enough(t.f32_winograd_f43_min, WINOGRAD_F43_MIN_COLS))
        return InForm::WinogradLayer;
    if (t.f32_winograd_no_f63 || !wn_winograd_layer_f63_supported(p.C, p.H) || !long_enough(t.f32_winograd_f63_min, WINOGRAD_F63_MIN_COLS))
        return InForm::WinogradLayerF43;
    return InForm::WinogradLayerF63;
}

// ---- the conditioning form of a call -----------------------------------------------
// Chain: the upsampling launch writes spect, cond layer 0 of every flow writes h_tmp, cond layer 1 writes h_all.
// Composed (where the blob holds the composed matrix; CTTS_F32_COND_CHAIN: never): a copy of the mel frames with a zero left halo,
// then ONE launch of the conv-GEMM whose phase store writes h_all - no spect, no h_tmp.  Not bit-equal to the chain: one sum over
// ccJ n_mel products of a matrix rounded once from double, against K0 + H products through two fp32 roundings.
// Taken where it issues fewer products than the chain.  Both launch whole 128-column tiles - the composed GEMM of frames, P H rows
// over K = ccJ n_mel; the chain of P x as many latent columns, H rows over K0, then over H - so a short utterance, whose frames fill
// a fraction of one tile, keeps the chain (n_mel 80, hop 256, n_group 8: below 45 frames).  A function of the utterance alone.
bool cond_composed(const Plan& p, int frames, const Tuning& t) {
    if (!p.cc || t.f32_cond_chain || gemm_split_level(p.c.f32_gemm_mode) != 0) return false;   // (the split-bf16 loops keep the chain)
    const long long tiles_f = (frames + GEMM_BN - 1) / GEMM_BN, tiles_l = ((long long)frames * p.ccP + GEMM_BN - 1) / GEMM_BN;
    return tiles_f * p.ccP * p.ccJ * p.c.n_mel_channels < tiles_l * (p.K0 + p.H);
}
// the padded mel [B][n_mel][ld]: frames in whole 128-column tiles behind a left halo of `pad` >= ccJ - 1 zero columns
struct MelGeom { int ntiles, pad, ld; };
MelGeom mel_geom(int frames) {
    const int nt = (frames + GEMM_BN - 1) / GEMM_BN;
    return {nt, 4, nt * GEMM_BN + 8};
}

struct Workspace {
    float *audio, *spect, *spk, *h_tmp, *h_all, *x, *act, *out;
    float* melp;        // composed conditioning: the padded mel (then spect and h_tmp are NULL: nothing reads them)
    float* act_all;     // deferred-skip form: the gated activations of every layer of a flow ([n_layers] x act)
    float* a16;         // WN folds: layer 0's input [B][FOLD_ROWS][ld] = [audio_0; 1 on [0, L); 0]
    float* skend;       // WN folds: the skip/end accumulator [B][2 n_half][ld] between the groups of a flow
    // Winograd in-layer forms (NULL in the direct form): V1..V4 [4][B][C][ldp], T2 / T3 [2][B][2C][ldp], h2e / h2o [2][B][H][ldp];
    // the F(4,3) form keeps V0..V5 [6][B][C][ldq] and h(t_0)..h(t_3) [4][B][H][ldq] in the same two buffers (sized for the larger form),
    // the F(6,3) form V0..V7 [8][B][C][ldh] (no cond copies: its layers read the cond rows in place)
    float *wgV, *wgT, *wgH;
    int ldp, ldq, ldh;
    size_t total;  // floats
};

void carve(const Plan& p, const Geom& g, int batch, float* base, InForm in, bool composed, Workspace& w) {
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = align_up(o + n); return base ? base + r : nullptr; };
    const size_t B = batch;
    w.audio = take(B * p.c.n_group * g.L);
    w.spect = composed ? nullptr : take(B * p.K0 * g.ld);
    w.melp = composed ? take(B * p.c.n_mel_channels * mel_geom(g.L / p.ccP).ld) : nullptr;
    w.spk = take(B * p.c.n_flows * p.S * g.ld);          // speaker-embedding rows (glow.py:193-196), per flow
    w.h_tmp = composed ? nullptr : take(B * p.c.n_flows * p.H * g.ld);
    w.h_all = take(B * p.c.n_flows * p.H * g.ld);
    w.x = take(B * p.C * g.ld);
    w.act = take(B * p.C * g.ld);
    w.out = take(B * p.C * g.ld);
    // gated activations of ONE skip group (its skip GEMM runs at the end of the group; the next group reuses the slots)
    w.act_all = take((size_t)std::min(p.c.n_layers, (int)Plan::F32_SKIP_GROUP) * B * p.C * g.ld);
    w.a16 = take(B * FOLD_ROWS * g.ld);
    w.skend = take(B * p.c.n_group * g.ld);
    w.wgV = w.wgT = w.wgH = nullptr;
    w.ldp = w.ldq = w.ldh = 0;
    if (in != InForm::Direct) {
        w.ldp = pair_ld(p, g);
        w.ldq = quad_space(in) ? quad_ld(p, g) : 0;
        w.ldh = in == InForm::WinogradLayerF63 ? hex_ld(p, g) : 0;
        w.wgV = take(std::max({(size_t)4 * w.ldp, (size_t)6 * w.ldq, (size_t)8 * w.ldh}) * B * p.C);
        w.wgT = take((size_t)2 * B * 2 * p.C * w.ldp);
        w.wgH = take(std::max((size_t)2 * w.ldp, (size_t)4 * w.ldq) * B * p.H);
    }
    w.total = o;
}

// ---- profiling hooks ---------------------------------------------------------------
// A profile is a caller-owned handle (ctts_profile_create); a thread records into the handle it bound
// (ctts_profile_bind), so two threads timing two models at once keep disjoint slots.  No process-wide switch.
struct Prof {
    std::mutex mu;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[CTTS_PROF_N];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
};
thread_local Prof* t_prof = nullptr;

struct ProfScope {
    int which; hipStream_t s; hipEvent_t stop = nullptr; bool active = false;
    ProfScope(int which_, hipStream_t s_) : which(which_), s(s_) {
        Prof* pr = t_prof;
        if (!pr) return;
        std::lock_guard<std::mutex> lk(pr->mu);
        std::pair<hipEvent_t, hipEvent_t> e;
        if (!pr->pool.empty()) { e = pr->pool.back(); pr->pool.pop_back(); }
        else { if (hipEventCreate(&e.first) != hipSuccess || hipEventCreate(&e.second) != hipSuccess) return; }
        (void)hipEventRecord(e.first, s);
        stop = e.second;
        pr->ev[which].push_back(e);
        active = true;
    }
    ~ProfScope() { if (active) (void)hipEventRecord(stop, s); }
};

// ---- speaker rows --------------------------------------------------------------------
// spk[b][k*S + e][pad + l] = table_k[ids[b]][e]  (e < sdim), zero rows above: the reference concatenates the speaker
// embedding, repeated over time, under the spectrogram (glow.py:193-196); here it is the second K segment of cond layer 0
__global__ __launch_bounds__(256) void speaker_rows_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                           float* __restrict__ spk, int k, int n_flows, int S, int sdim,
                                                           int L, int ld, int pad) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.y, b = blockIdx.z;
    if (n >= ld) return;
    float v = 0.f;
    if (e < sdim && n >= pad && n < pad + L) {
        const long long id = ids[b];      // an id outside the table poisons the utterance (NaN) instead of reading out of bounds
        v = (id >= 0 && id < CTTS_N_SPEAKERS) ? table[(size_t)id * sdim + e] : __builtin_nanf("");
    }
    spk[((size_t)b * n_flows * S + (size_t)k * S + e) * ld + n] = v;
}

// ---- composed conditioning ----------------------------------------------------------
// glow.py:318-324, 198-199 on a single-speaker model is linear in the mel: the transposed conv (kernel win = J hop, stride hop),
// trimmed to F hop samples, gives sample hop f + u the frames f - j at taps hop j + u (j < J; frames before 0 add nothing); the
// squeeze puts sample G t + s of channel co in row co G + s of latent column t = P f + p; cond layers 0 and 1 follow with nothing
// between them.  So   h_k[:, P f + p] = A_{k,p} [mel[f]; mel[f-1]; ..; mel[f-J+1]] + b'_k   with
//   A_{k,p}[r][j n_mel + ci] = sum_{co,s} (W1_k W0_k)[r][co G + s] w_up[ci][co][hop j + G p + s],   b'_k = W1_k (W0_k b_up~ + b0_k) + b1_k
// (b_up~: b_up[co] in row co G + s).  Formed in double at pack time and rounded once.

// w10 = W1 W0 in double, [H][K0]
__global__ __launch_bounds__(256) void cond_compose_w10_kernel(const float* __restrict__ w1, const float* __restrict__ w0,
                                                               double* __restrict__ w10, int H, int K0) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= K0) return;
    double s = 0.0;
    for (int h = 0; h < H; ++h) s += (double)w1[(size_t)r * H + h] * (double)w0[(size_t)h * K0 + c];
    w10[(size_t)r * K0 + c] = s;
}

// One flow's A panel in pack_a layout [P][nch][GEMM_KC][GEMM_BM]: M-block m holds hidden rows [m HR, (m + 1) HR), HR = GEMM_BM / P,
// block-local row (r % HR) P + p; K index j n_mel + ci.  Thread = block-local row, blockIdx = (K index, M-block).
__global__ __launch_bounds__(GEMM_BM) void cond_compose_A_kernel(const double* __restrict__ w10, const float* __restrict__ up_w,
                                                                 float* __restrict__ A, int n_mel, int G, int hop, int win, int P,
                                                                 int nch) {
    const int rl = threadIdx.x, kidx = blockIdx.x, m = blockIdx.y;
    const int r = m * (GEMM_BM / P) + rl / P, p = rl % P;
    const int j = kidx / n_mel, ci = kidx % n_mel;
    const float* u = up_w + (size_t)ci * n_mel * win + hop * j + G * p;
    const double* wr = w10 + (size_t)r * n_mel * G;
    double s = 0.0;
    for (int co = 0; co < n_mel; ++co)
        for (int q = 0; q < G; ++q) s += wr[co * G + q] * (double)u[(size_t)co * win + q];
    A[(((size_t)m * nch + kidx / GEMM_KC) * GEMM_KC + kidx % GEMM_KC) * GEMM_BM + rl] = (float)s;
}

// One flow's bias [P][GEMM_BM] in the same row order; one workgroup of H = GEMM_BM threads
__global__ __launch_bounds__(GEMM_BM) void cond_compose_bias_kernel(const float* __restrict__ w0, const float* __restrict__ b0,
                                                                    const float* __restrict__ w1, const float* __restrict__ b1,
                                                                    const float* __restrict__ up_b, float* __restrict__ bias, int K0,
                                                                    int G, int P) {
    __shared__ double t0[GEMM_BM];
    const int r = threadIdx.x;
    double s = b0[r];
    for (int c = 0; c < K0; ++c) s += (double)w0[(size_t)r * K0 + c] * (double)up_b[c / G];
    t0[r] = s;
    __syncthreads();
    s = b1[r];
    for (int h = 0; h < GEMM_BM; ++h) s += (double)w1[(size_t)r * GEMM_BM + h] * t0[h];
    const int HR = GEMM_BM / P;
    for (int p = 0; p < P; ++p) bias[(size_t)(r / HR) * GEMM_BM + (r % HR) * P + p] = (float)s;
}

// melp[b][c][pad + f] = mel[b][c][f], zero everywhere else
__global__ __launch_bounds__(256) void mel_pad_kernel(const float* __restrict__ mel, float* __restrict__ melp, int frames, int ld, int pad) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const size_t row = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (n >= ld) return;
    const int f = n - pad;
    melp[row * ld + n] = f >= 0 && f < frames ? mel[row * frames + f] : 0.0f;
}

// ---- forward (analysis) direction, glow.py:267-312: what it adds to the blob and the workspace ------------------------------
// The forward mix matrices W_k [n_rem][n_rem] live in a blob of their own (the infer blob holds their inverses only).
size_t fwd_mix_off(const Plan& p, int k) {
    size_t o = 0;
    for (int j = 0; j < k; ++j) o += align_up((size_t)p.fd[j].n_rem * p.fd[j].n_rem);
    return o;
}
int fwd_log_s_rows(const Plan& p, int k) {
    int r = 0;
    for (int j = 0; j < k; ++j) r += p.fd[j].n_half;
    return r;
}

// Behind the infer workspace: the fp64 slots of the two-stage sums - ls_part [B][n_flows][nblk_ls] (one per tail workgroup) and
// z_part [B][nblk_z]; total = both together, in floats
struct FwdSums { double *ls_part, *z_part; int nblk_ls, nblk_z; size_t total; };

void carve_fwd(const Plan& p, const Geom& g, int batch, float* base, InForm in, bool composed, Workspace& w, FwdSums& f) {
    carve(p, g, batch, base, in, composed, w);
    f.nblk_ls = (g.L + 255) / 256;
    f.nblk_z = (int)(((long long)p.c.n_group * g.L + FWD_SUMSQ_CHUNK - 1) / FWD_SUMSQ_CHUNK);
    size_t o = w.total;                                 // a multiple of ALIGN_F floats = 256 bytes
    auto take = [&](size_t doubles) { size_t r = o; o = align_up(o + 2 * doubles); return base ? reinterpret_cast<double*>(base + r) : nullptr; };
    f.ls_part = take((size_t)batch * p.c.n_flows * f.nblk_ls);
    f.z_part = take((size_t)batch * f.nblk_z);
    f.total = o;
}

int workspace_fits(const char* what, size_t have, size_t need) {
    if (need <= have) return CTTS_OK;
    set_error("%s: workspace %zu bytes < required %zu", what, have, need);
    return CTTS_E_WORKSPACE;
}

// ---- the fp32 runner ---------------------------------------------------------------
// The WN stack of one flow comes in three forms (all the same products; the skip sum is summed in another order in each):
//   PerLayer  one res/skip launch per layer (x += res rows, out (+)= skip rows), then the flow tail.  CTTS_F32_NO_DEFER_SKIP, and
//             what ctts_wn_stack_f32 runs on the caller's buffers
//   Deferred  every layer's gated activation is kept, the per-layer launch computes the res rows only, and the skip rows of up to
//             F32_SKIP_GROUP layers are ONE contraction with K = 4 C behind the group; then the flow tail.  CTTS_F32_NO_WN_FOLD
//   Folded    (the default) Deferred with the WN start / end folds: layer 0 reads the FOLD_ROWS-row [audio_0; 1; 0] instead of x, and
//             the skip sum is never formed - a skip/end pass per group accumulates its 2 n_half-row image through `end`, and the
//             last one of a flow is also the flow tail
enum class StackForm { PerLayer, Deferred, Folded };

// What a call decides once, the one builder of every launch descriptor, and a driver per stack form.
struct WnCall {
    Plan p; Geom g; Tuning t;
    const float* blob = nullptr;
    int batch = 0, frames = 0;
    hipStream_t s = nullptr;
    Workspace w{};                      // carved (take_workspace), or the caller's x / act / out alone (ctts_wn_stack_f32)
    FwdSums sums{};                     // forward direction only
    long long cstride = 0, hstride = 0; // batch-item strides of a C-row tensor and of the cond hidden of all flows
    StackForm stack = StackForm::PerLayer;
    InForm in = InForm::Direct;
    bool composed = false;              // the conditioning form (cond_composed)
    float* audio = nullptr;             // [B][n_group][L], updated in place flow by flow (forward: z)
    const float* h_all = nullptr;       // cond hidden of all flows

    // ---- opening: plan and geometry, then (behind the entry's own checks) the workspace of its kind and the forms
    int begin(const ctts_waveglow_config* cfg, const void* packed, int batch_, int frames_, void* stream, int options = 0) {
        int rc = make_plan(cfg, p, options); if (rc) return rc;
        rc = make_geom(p, frames_, g); if (rc) return rc;
        t = tuning();
        blob = static_cast<const float*>(packed); batch = batch_; frames = frames_; s = as_stream(stream);
        cstride = (long long)p.C * g.ld;
        hstride = (long long)p.c.n_flows * p.H * g.ld;
        return CTTS_OK;
    }
    // the forms, the workspace carved for them, its size refusal; audio and h_all default to the workspace's own
    int take_workspace(const char* what, void* workspace, size_t workspace_bytes, bool forward) {
        in = in_form(p, g, t);
        stack = t.f32_no_defer_skip ? StackForm::PerLayer : t.f32_no_wn_fold ? StackForm::Deferred : StackForm::Folded;
        composed = cond_composed(p, frames, t);
        if (forward) carve_fwd(p, g, batch, static_cast<float*>(workspace), in, composed, w, sums);
        else carve(p, g, batch, static_cast<float*>(workspace), in, composed, w);
        audio = w.audio; h_all = w.h_all;
        return workspace_fits(what, workspace_bytes, (forward ? sums.total : w.total) * sizeof(float));
    }

    // ---- accessors
    const float* h(int k) const { return h_all + (size_t)k * p.H * g.ld; }            // flow k's cond rows
    size_t act_stride() const { return (size_t)batch * p.C * g.ld; }
    // layer i's gated activation: the one buffer of the per-layer form, else the layer's slot of its skip group (the skip launch
    // runs behind the group; the next group reuses the slots)
    float* act(int i) const { return stack == StackForm::PerLayer ? w.act : w.act_all + (size_t)(i % Plan::F32_SKIP_GROUP) * act_stride(); }
    bool group_ends(int i) const { return i == p.c.n_layers - 1 || (i + 1) % Plan::F32_SKIP_GROUP == 0; }
    // Winograd forms: layer i (d = 2^i) reads the cond rows where they lie in h_all, through the launch's pair map (GemmArgs.mseg),
    // where d % 4 == 0; d = 2 (and d = 1, layer 0 without the start fold) and every layer of WinogradSeparate read the copies
    // h2e / h2o the transform makes
    bool in_place(int i) const { return in != InForm::WinogradSeparate && (1 << i) % 4 == 0; }
    bool hex(int i) const { return in == InForm::WinogradLayerF63 && f63_layer(i); }      // layer i runs the F(6,3) form
    size_t plane(int rows) const { return (size_t)batch * rows * w.ldp; }           // one [B][rows][ldp] plane of wgV / wgT / wgH

    // ---- descriptor builders: no GemmArgs or WnWinogradLayerArgs field is assigned anywhere else in the fp32 path
    GemmArgs header() const {
        GemmArgs a{};
        a.gemm_mode = p.c.f32_gemm_mode;
        a.ld = g.ld; a.pad = g.pad; a.L = g.L; a.ntiles = g.ntiles; a.batch = batch;
        a.dst_ld = g.ld; a.dst_pad = g.pad;
        return a;
    }
    // the GATE launch of layer i on three taps at dilation 2^i + the cond rows: taps of x, or (layer 0 of the folded stack) of
    // a16 - K = 3 taps x FOLD_ROWS + cond, same epilogue and bias
    GemmArgs in_gemm(int k, int i) const {
        const auto& f = p.fl[k];
        const bool fold0 = stack == StackForm::Folded && i == 0;
        const int dil = 1 << i, nch = fold0 ? 1 : p.nch_rs;
        const float* taps = fold0 ? w.a16 : w.x;
        const long long tstride = fold0 ? (long long)FOLD_ROWS * g.ld : cstride;
        GemmArgs a = header();
        a.A = blob + (fold0 ? f.in0f_A : f.in_A[i]); a.bias = blob + f.in_b[i];
        a.nseg = 4; a.interleave = 3; a.nch_total = fold0 ? p.nch_in0f : p.nch_in; a.MB = p.mb_in;
        for (int tap = 0; tap < 3; ++tap) a.seg[tap] = {taps, tstride, nch, (tap - 1) * dil, 0, 0};
        a.seg[3] = {h(k), hstride, p.nch1h, 0, 0, 0};
        a.dst0 = act(i); a.dst0_bstride = cstride;
        a.M = 2 * p.C; a.pairC = p.C;
        return a;
    }
    // The SPLIT launches behind a layer contract `n` kept activations, from `acts` on, side by side along K, with a packed matrix of
    // `rows` rows: rows below `split` add to x, the rest go to (acc1: add to) the skip sum
    GemmArgs behind(size_t A, size_t bias, int rows, const float* acts, int n, int split, bool acc1) const {
        GemmArgs a = header();
        a.A = blob + A; a.bias = blob + bias;
        a.nseg = n; a.nch_total = n * p.nch_rs; a.MB = (rows + GEMM_BM - 1) / GEMM_BM;
        for (int j = 0; j < n; ++j) a.seg[j] = {acts + (size_t)j * act_stride(), cstride, p.nch_rs, 0, 0, 0};
        a.M = rows; a.split = split;
        a.dst0 = w.x; a.dst0_bstride = cstride; a.acc0 = 1;
        a.dst1 = w.out; a.dst1_bstride = cstride; a.acc1 = acc1 ? 1 : 0;
        return a;
    }
    // deferred forms, layers before the last: x += W_res,i act(i) + b
    GemmArgs res(int k, int i) const { return behind(p.fl[k].res_A[i], p.fl[k].res_b[i], p.C, act(i), 1, p.C, false); }
    // Deferred: the skip rows of group gi's layers, over the group's kept activations, in one contraction
    GemmArgs skip_group(int k, int gi) const { return behind(p.fl[k].skip_A[gi], p.fl[k].skip_b[gi], p.C, w.act_all, p.group_layers(gi), 0, gi > 0); }
    // PerLayer: res rows and skip rows of layer i in one launch (the last layer has skip rows only)
    GemmArgs res_skip(int k, int i) const {
        return behind(p.fl[k].rs_A[i], p.fl[k].rs_b[i], p.rs_rows(i), act(i), 1, i == p.c.n_layers - 1 ? 0 : p.C, i > 0);
    }
    // cond layer 0 of every flow in one launch (M-block k = flow k, which reads its own S speaker rows as a second K segment)
    GemmArgs cond0(const float* spect, const float* spk, float* h_tmp) const {
        GemmArgs a = header();
        a.A = blob + p.cond0_A; a.bias = blob + p.cond0_b;
        a.nseg = 1; a.nch_total = p.nch0; a.MB = p.c.n_flows;
        a.seg[0] = {spect, (long long)p.K0 * g.ld, p.K0 / GEMM_KC, 0, 0, 0};
        if (p.S) {
            a.nseg = 2;
            a.seg[1] = {spk, (long long)p.c.n_flows * p.S * g.ld, p.S / GEMM_KC, 0, p.S, 0};
        }
        a.dst0 = h_tmp; a.dst0_bstride = hstride; a.acc0 = 0;
        a.dst1 = h_tmp; a.dst1_bstride = hstride; a.acc1 = 0;
        a.split = p.c.n_flows * GEMM_BM;
        a.M = p.c.n_flows * GEMM_BM;
        return a;
    }
    // cond layer 1: that launch again with its own matrix, K = flow k's H rows of h_tmp, into h_all
    GemmArgs cond1(const float* spect, const float* spk, float* h_tmp, float* h_out) const {
        GemmArgs a = cond0(spect, spk, h_tmp);
        a.A = blob + p.cond1_A; a.bias = blob + p.cond1_b;
        a.nseg = 1; a.nch_total = p.nch1h;
        a.seg[0] = {h_tmp, hstride, p.nch1h, 0, GEMM_BM, 0};
        a.dst0 = h_out; a.dst1 = h_out;
        return a;
    }
    // The composed conditioning: columns are FRAMES of the padded mel (its own geometry), K = tap j of every mel channel as segment j
    // at shift -j, M-block m = (flow m / P, hidden rows (m % P) 256 / P ..) x P phases; the phase store expands it into h_out
    GemmArgs cond_composed_gemm(const float* melp, float* h_out) const {
        const MelGeom mg = mel_geom(frames);
        GemmArgs a{};
        a.gemm_mode = p.c.f32_gemm_mode;
        a.ld = mg.ld; a.pad = mg.pad; a.L = frames; a.ntiles = mg.ntiles; a.batch = batch;
        a.A = blob + p.cc_A; a.bias = blob + p.cc_b;
        a.nseg = p.ccJ; a.nch_total = p.nch_cc; a.MB = p.c.n_flows * p.ccP;
        for (int j = 0; j < p.ccJ; ++j)
            a.seg[j] = {melp, (long long)p.c.n_mel_channels * mg.ld, p.c.n_mel_channels / GEMM_KC, -j, 0, 0};
        a.M = a.MB * GEMM_BM; a.split = a.M;
        a.phase = p.ccP;
        a.dst0 = h_out; a.dst0_bstride = hstride; a.dst_ld = g.ld; a.dst_pad = g.pad;
        return a;
    }
    // Winograd F(2,3) as launches of the conv-GEMM in pair space (ld = ldp, no halo):
    //   T2 = G2 V2, T3 = G3 V3,   act[t_e] = gate([W0 | C_i] [V1; h(t_e)] + b + T2 + T3),   act[t_o] = gate([-W2 | C_i] [V4; h(t_o)] + b + T2 - T3)
    // WinogradPaired: T2 | T3 are the two parts of launch j = 0 and so are even | odd (GemmArgs.parts: one round peel per pair);
    // WinogradSeparate: launches j = 0, 1.  Same bits either way: the same products summed in the same order.
    GemmArgs wg_header(int i) const {
        const PairGeom pg = pair_geom(g, i);
        GemmArgs a{};
        a.gemm_mode = p.c.f32_gemm_mode;
        a.ld = w.ldp; a.pad = 0; a.L = pg.Lp; a.ntiles = pg.ntiles; a.batch = batch; a.MB = p.mb_in;
        a.M = 2 * p.C;
        if (in == InForm::WinogradPaired) a.parts = 2;
        return a;
    }
    GemmArgs wg_T(int k, int i, int j) const {
        const auto& f = p.fl[k];
        GemmArgs a = wg_header(i);
        a.A = blob + (j == 0 ? f.wg_T2_A[i] : f.wg_T3_A[i]); a.bias = blob + p.zero_b;
        a.nseg = 1; a.nch_total = p.nch_rs;
        a.seg[0] = {w.wgV + (1 + j) * plane(p.C), (long long)p.C * w.ldp, p.nch_rs, 0, 0, 0};
        a.split = 2 * p.C;
        a.dst0 = w.wgT + j * plane(2 * p.C); a.dst0_bstride = (long long)2 * p.C * w.ldp; a.dst_ld = w.ldp; a.dst_pad = 0;
        if (a.parts == 2) {
            a.part_A = (long long)f.wg_T3_A[i] - (long long)f.wg_T2_A[i];
            a.part_seg[0] = (long long)plane(p.C);
            a.part_dst0 = (long long)plane(2 * p.C);
        }
        return a;
    }
    // (stores to act's natural columns, through the pair map of parity j)
    GemmArgs wg_gate(int k, int i, int j) const {
        const auto& f = p.fl[k];
        GemmArgs a = wg_header(i);
        a.A = blob + (j == 0 ? f.wg_e_A[i] : f.wg_o_A[i]); a.bias = blob + f.in_b[i];
        a.nseg = 2; a.nch_total = p.nch_rs + p.nch1h;
        a.seg[0] = {w.wgV + (j == 0 ? 0 : 3) * plane(p.C), (long long)p.C * w.ldp, p.nch_rs, 0, 0, 0};
        if (in_place(i)) {
            a.seg[1] = {h(k), hstride, p.nch1h, 0, 0, 0};
            a.mseg = 2; a.mseg_ld = g.ld; a.mseg_pad = g.pad;
        } else {
            a.seg[1] = {w.wgH + j * plane(p.H), (long long)p.H * w.ldp, p.nch1h, 0, 0, 0};
        }
        a.split = 0; a.pairC = p.C;
        a.dst0 = act(i); a.dst0_bstride = cstride; a.dst_ld = g.ld; a.dst_pad = g.pad;
        a.addend = w.wgT; a.addend2 = w.wgT + plane(2 * p.C); a.addend_bstride = (long long)2 * p.C * w.ldp;
        a.addend2_sign = j == 0 ? 1.0f : -1.0f;
        a.map_d = 1 << i; a.map_L = g.L; a.map_par = j;
        if (a.parts == 2) {
            a.part_A = (long long)f.wg_o_A[i] - (long long)f.wg_e_A[i];
            a.part_seg[0] = (long long)(3 * plane(p.C));
            a.part_seg[1] = in_place(i) ? 0 : (long long)plane(p.H);
        }
        return a;
    }
    // the one-launch layer behind the transform (wn_winograd_layer.hip), F(2,3) in pair space, F(4,3) in quad or F(6,3) in hex space
    WnWinogradLayerArgs wg_layer(int k, int i) const {
        const auto& f = p.fl[k];
        const bool f43 = quad_space(in) && !hex(i);
        const PairGeom sg = hex(i) ? hex_geom(g, i) : f43 ? quad_geom(g, i) : pair_geom(g, i);
        const int ldw = hex(i) ? w.ldh : f43 ? w.ldq : w.ldp;
        WnWinogradLayerArgs a{};
        if (hex(i)) {
            a.form = WNWG_F63;
            a.A_T2 = blob + f.wh_U_A[0][i]; a.A_T3 = blob + f.wh_U_A[1][i]; a.A_T4 = blob + f.wh_U_A[2][i]; a.A_T5 = blob + f.wh_U_A[3][i];
            a.A_T6 = blob + f.wh_U_A[4][i]; a.A_T7 = blob + f.wh_U_A[5][i];
            a.A_e = blob + f.wh_e_A[i]; a.A_o = blob + f.wh_o_A[i];
        } else if (f43) {
            a.form = WNWG_F43;
            a.A_T2 = blob + f.wq_U_A[0][i]; a.A_T3 = blob + f.wq_U_A[1][i]; a.A_T4 = blob + f.wq_U_A[2][i]; a.A_T5 = blob + f.wq_U_A[3][i];
            a.A_e = blob + f.wq_e_A[i]; a.A_o = blob + f.wq_o_A[i];
        } else {
            a.A_T2 = blob + f.wg_T2_A[i]; a.A_T3 = blob + f.wg_T3_A[i]; a.A_e = blob + f.wg_e_A[i]; a.A_o = blob + f.wg_o_A[i];
        }
        a.bias = blob + f.in_b[i];
        a.V = w.wgV; a.vplane = (long long)batch * p.C * ldw;
        a.Hc = w.wgH; a.hplane = (long long)batch * p.H * ldw;
        a.h2 = h(k); a.h_bstride = hstride;
        a.act = act(i); a.act_bstride = cstride;
        a.C = p.C; a.H = p.H; a.batch = batch;
        a.ldp = ldw; a.Lp = sg.Lp; a.ntiles = sg.ntiles;
        a.d = sg.d; a.L = g.L; a.ld = g.ld; a.pad = g.pad;
        a.in_place = in_place(i);
        return a;
    }

    // ---- launches
    int gemm(int prof_slot, int epi, const GemmArgs& a) const {
        ProfScope ps(prof_slot, s);
        return launch_gemm_f32(epi, a, s);
    }
    // x -> V (and, unless the layer reads them in place, the cond rows in pair / quad order).  WinogradSeparate: the d = 2 transform
    // one column at a time; F(4,3): V0..V5 (1.5 C L floats), and the 128-column arm of the layer (CTTS_F32_NO_SMALL) reads whole
    // 128-column tiles, so the transform fills them
    int wg_transform(int k, int i) const {
        if (hex(i)) {
            const PairGeom hg = hex_geom(g, i);
            return launch_winograd_transform_hex(w.x, cstride, w.wgV, batch, p.C, hg.d, g.L, hg.Lp, g.ld, g.pad, w.ldh, hg.ntiles * 64, s);
        }
        if (quad_space(in)) {
            const PairGeom qg = quad_geom(g, i);
            const int ncols = t.f32_no_small ? round_up(qg.ntiles * 64, 128) : qg.ntiles * 64;
            return launch_winograd_transform_quad(w.x, cstride, h(k), hstride, w.wgV, w.wgH, batch, p.C, p.H, qg.d, g.L, qg.Lp, g.ld, g.pad,
                                                  w.ldq, ncols, !in_place(i), s);
        }
        const PairGeom pg = pair_geom(g, i);
        return launch_winograd_transform(w.x, cstride, h(k), hstride, w.wgV, w.wgH, batch, p.C, p.H, pg.d, g.L, pg.Lp, g.ld, g.pad, w.ldp,
                                         pg.ntiles * GEMM_BN, !in_place(i), in != InForm::WinogradSeparate, s);
    }
    // x (layer 0 of the folded stack: a16) -> act(i).  Slot CTTS_PROF_WN_IN has one entry per layer, around the transform and every
    // launch behind it; slot WN_IN0F has the folded layer 0 alone.
    int in_layer(int k, int i) const {
        ProfScope ps(CTTS_PROF_WN_IN, s);
        if (stack == StackForm::Folded && i == 0) return gemm(CTTS_PROF_WN_IN0F, GEMM_EPI_GATE, in_gemm(k, i));
        int rc = in == InForm::Direct ? CTTS_OK : wg_transform(k, i);
        if (rc) return rc;
        switch (in) {
        case InForm::Direct:
            return launch_gemm_f32(GEMM_EPI_GATE, in_gemm(k, i), s);
        case InForm::WinogradLayer:
        case InForm::WinogradLayerF43:
        case InForm::WinogradLayerF63:
            return launch_wn_winograd_layer(wg_layer(k, i), s);
        case InForm::WinogradSeparate:
        case InForm::WinogradPaired:
            const int np = in == InForm::WinogradPaired ? 1 : 2;          // launches per pair
            for (int j = 0; j < np; ++j)
                if ((rc = launch_gemm_f32(GEMM_EPI_SPLIT, wg_T(k, i, j), s))) return rc;
            for (int j = 0; j < np; ++j)
                if ((rc = launch_gemm_f32(GEMM_EPI_GATE, wg_gate(k, i, j), s))) return rc;
        }
        return rc;
    }
    // x_0 = W_start a_0 + b_start (glow.py:189)
    int start(int k, const float* a_in) const {
        const auto& f = p.fl[k];
        const auto& d = p.fd[k];
        return launch_wn_start(a_in, blob + f.start_w, blob + f.start_b, w.x, batch, p.C, p.c.n_group, d.ch_off, d.n_half, g.L, g.ld, g.pad, s);
    }
    // Folded: W_end . (skip rows of group gi) over the group's kept activations, accumulated in skend; `tail`: the flow's last pass
    // also adds b', couples, mixes and stores to audio (or un-squeezed to `wave`)
    int skip_end(int k, int gi, bool tail, float* wave, const CouplingForward* fwd) const {
        const auto& f = p.fl[k];
        const auto& d = p.fd[k];
        ProfScope ps(CTTS_PROF_WN_SKEND, s);
        return launch_skip_end(w.act_all, (long long)act_stride(), p.group_layers(gi),
                               blob + f.skend_W + (size_t)gi * Plan::F32_SKIP_GROUP * p.C * 2 * d.n_half, w.skend, gi == 0, tail,
                               blob + f.skend_b, blob + f.winv, audio, wave, batch, p.C, p.c.n_group, d.ch_off, d.n_half, g.L, g.ld,
                               g.pad, s, tail ? fwd : nullptr);
    }
    // end conv on the skip sum, coupling, inverse 1x1 (+ un-squeeze into `wave`); `fwd`: the forward coupling instead, nothing mixed
    int flow_tail(int k, const float* out, float* a_io, float* wave, const CouplingForward* fwd) const {
        const auto& f = p.fl[k];
        const auto& d = p.fd[k];
        return launch_flow_tail(out, a_io, wave, blob + f.end_w, blob + f.end_b, blob + f.winv, batch, p.C, p.c.n_group, d.ch_off,
                                d.n_half, g.L, g.ld, g.pad, s, fwd);
    }

    // ---- one driver per stack form
    // Folded.  1. start: x_0 is still formed, the res path x_1 = x_0 + W_res,0 act_0 needs it
    //          2. ones rows: a16 = [audio_0; 1 on [0, L); 0]
    //          3. per layer: in-layer; before the last layer: res rows
    //          4. behind each skip group: its skip/end pass; the last one is the flow's tail
    int flow_folded(int k, float* wave, const CouplingForward* fwd) const {
        const auto& d = p.fd[k];
        int rc = start(k, audio);
        if (rc) return rc;
        if ((rc = launch_wn_start_ones(audio, w.a16, batch, p.c.n_group, d.ch_off, d.n_half, g.L, g.ld, g.pad, s))) return rc;
        for (int i = 0; i < p.c.n_layers; ++i) {
            const bool last = i == p.c.n_layers - 1;
            if ((rc = in_layer(k, i))) return rc;
            if (!last && (rc = gemm(CTTS_PROF_WN_RES_F, GEMM_EPI_SPLIT, res(k, i)))) return rc;
            if (group_ends(i) && (rc = skip_end(k, i / Plan::F32_SKIP_GROUP, last, wave, fwd))) return rc;
        }
        return CTTS_OK;
    }
    // Deferred (x, out <- the stack on a_in; the flow tail follows).  1. start
    //          2. per layer: in-layer; before the last layer: res rows
    //          3. behind each skip group: its skip rows, one contraction into out
    int stack_deferred(int k, const float* a_in) const {
        int rc = start(k, a_in);
        if (rc) return rc;
        for (int i = 0; i < p.c.n_layers; ++i) {
            if ((rc = in_layer(k, i))) return rc;
            if (i < p.c.n_layers - 1 && (rc = gemm(CTTS_PROF_WN_RS, GEMM_EPI_SPLIT, res(k, i)))) return rc;
            if (group_ends(i) && (rc = gemm(CTTS_PROF_WN_SKIP, GEMM_EPI_SPLIT, skip_group(k, i / Plan::F32_SKIP_GROUP)))) return rc;
        }
        return CTTS_OK;
    }
    // PerLayer (likewise).  1. start
    //          2. per layer: in-layer; res and skip rows
    int stack_per_layer(int k, const float* a_in) const {
        int rc = start(k, a_in);
        if (rc) return rc;
        for (int i = 0; i < p.c.n_layers; ++i) {
            if ((rc = in_layer(k, i))) return rc;
            if ((rc = gemm(CTTS_PROF_WN_RS, GEMM_EPI_SPLIT, res_skip(k, i)))) return rc;
        }
        return CTTS_OK;
    }
    // One flow of the infer loop: rows of `audio` updated in place (or, with `wave`, the mixed rows go there un-squeezed).  The
    // whole-infer entry and the one-flow stage entry both run exactly this.  `fwd`: the forward direction - the same stack on rows
    // a_0, and the tail, whichever kernel it is, does the forward coupling instead.
    int run_flow(int k, float* wave, const CouplingForward* fwd) const {
        if (stack == StackForm::Folded) return flow_folded(k, wave, fwd);
        const int rc = stack == StackForm::Deferred ? stack_deferred(k, audio) : stack_per_layer(k, audio);
        return rc ? rc : flow_tail(k, w.out, audio, wave, fwd);
    }
    // One flow of the forward loop: the head (forward 1x1 mix of the rows still in play; flow 0 reads the waveform un-squeezed),
    // then run_flow with the forward tail.  audio = z is updated in place; rows above ch_off are early outputs and stay.
    // log_s_flow: NULL or this flow's rows (item stride ls_bstride).  The whole-model entry and the stage entry both run exactly this.
    int run_flow_forward(const float* fwd_blob, int k, const float* wave, float* log_s_flow, long long ls_bstride) const {
        const auto& d = p.fd[k];
        int rc = launch_flow_head_forward(fwd_blob + fwd_mix_off(p, k), wave, audio, batch, p.c.n_group, d.ch_off, d.n_rem, g.L, s);
        if (rc) return rc;
        const CouplingForward cf{log_s_flow, ls_bstride, sums.ls_part + (size_t)k * sums.nblk_ls, (long long)p.c.n_flows * sums.nblk_ls};
        return run_flow(k, nullptr, &cf);
    }

    // ---- conditioning: mel -> spect (upsampling + squeeze), the speaker rows, cond layers 0 and 1 of every flow
    int upsample(const float* mel, float* spect) const {
        return launch_upsample_squeeze(mel, blob + p.up_w, p.up_mfma ? blob + p.up_wp : nullptr, blob + p.up_b, spect, batch,
                                       p.c.n_mel_channels, frames, p.c.win_length, p.c.hop_length, p.c.n_group, g.ld, g.pad, s);
    }
    int speaker_rows(const int64_t* ids, float* spk) const {
        if (p.S == 0) return CTTS_OK;
        CTTS_CHECK_ARG(ids != nullptr, "multispeaker model (speaker_embed_dim=%d) needs speaker ids (glow.py:193)", p.c.speaker_embed_dim);
        for (int k = 0; k < p.c.n_flows; ++k)
            hipLaunchKernelGGL(speaker_rows_kernel, dim3((g.ld + 255) / 256, p.S, batch), dim3(256), 0, s, blob + p.fl[k].spk_tab, ids,
                               spk, k, p.c.n_flows, p.S, p.c.speaker_embed_dim, g.L, g.ld, g.pad);
        CTTS_CHECK_LAUNCH("speaker_rows");
        return CTTS_OK;
    }
    int cond(const float* spect, const float* spk, float* h_tmp, float* h_out) const {
        CTTS_CHECK_ARG(p.S == 0 || spk != nullptr, "wn_cond: multispeaker model needs the speaker rows");
        const int rc = launch_gemm_f32(GEMM_EPI_SPLIT, cond0(spect, spk, h_tmp), s);
        return rc ? rc : launch_gemm_f32(GEMM_EPI_SPLIT, cond1(spect, spk, h_tmp, h_out), s);
    }
    // mel -> h_out in the composed form: the padded copy, then the one launch
    int cond_from_mel(const float* mel, float* melp, float* h_out) const {
        CTTS_CHECK_ARG(p.cc, "wn_cond_composed: the packed model holds no composed conditioning matrix");
        const MelGeom mg = mel_geom(frames);
        hipLaunchKernelGGL(mel_pad_kernel, dim3((mg.ld + 255) / 256, p.c.n_mel_channels, batch), dim3(256), 0, s, mel, melp, frames, mg.ld, mg.pad);
        CTTS_CHECK_LAUNCH("mel_pad");
        return launch_gemm_f32(GEMM_EPI_PHASE, cond_composed_gemm(melp, h_out), s);
    }
    int conditioning(const float* mel, const int64_t* ids) const {
        if (composed) return cond_from_mel(mel, w.melp, w.h_all);
        int rc = upsample(mel, w.spect);
        if (rc) return rc;
        if ((rc = speaker_rows(ids, w.spk))) return rc;
        return cond(w.spect, w.spk, w.h_tmp, w.h_all);
    }
};

// ======================================================================================
// bf16 variant (BASELINE config 3): WN in-layer / res-skip GEMMs on bf16 MFMA with fp32 accumulation,
// WN activations (x, act, skip sum, cond hidden) stored bf16 in the K8-blocked layout; upsampling, the
// two small cond layers, the `end` conv, the coupling and the inverse 1x1 conv stay fp32.
// The res and skip halves of res_skip_layers are separate GEMMs here: the res rows update x after every layer
// (x feeds the next layer), the skip rows are deferred - every layer's gated activation stays in HBM and the skip
// sum is ONE contraction over K = n_layers * C at the end of the stack, BF_SKIP_GROUP layers per launch.  The
// per-layer form re-read and re-wrote the skip sum (2 x B*C*L bf16) in all but one of its n_layers epilogues.
constexpr int BF_SKIP_GROUP = 4;                   // 4 layers x 3 products = BGEMM_MAX_SEG segments in the split form
struct BfPlan {
    std::vector<std::vector<size_t>> in_A, rs_A;   // [flow][layer] offsets in bf16 elements (rs_A: res rows, layers < last)
    std::vector<std::vector<size_t>> skip_A;       // [flow][group]: skip rows of the group's layers side by side along K
    std::vector<size_t> skip_b;                    // [flow]: fp32 [2][mb_c*256] = {sum of the skip biases, zeros}
    size_t cond0_A, cond1_A;                       // flow-batched cond layers 0 / 1 (M-block k = flow k)
    size_t total;
    int nch_in, nch_rs, nch_c0, nch_c1;
    int mb_c, n_groups;                            // M-blocks of a C-row GEMM; skip launches per flow
    int P;                                         // K products per operand pair: 1 = bf16, 3 = split bf16 (hi*hi + lo*hi + hi*lo)
    int f16;                                       // 1: IEEE-half storage and MFMA operands instead of bf16 (P == 1 only)
    int group_layers(int g, int n_layers) const { return std::min(BF_SKIP_GROUP, n_layers - g * BF_SKIP_GROUP); }
};

void make_bf_plan(const Plan& p, BfPlan& q, int P, int f16 = 0) {
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = (o + n + 127) / 128 * 128; return r; };
    q.P = P;
    q.f16 = f16;
    q.nch_in = P * (p.c.kernel_size * p.C + p.H) / BGEMM_KC;
    q.nch_rs = P * p.C / BGEMM_KC;
    q.nch_c0 = P * (p.K0 + p.S) / BGEMM_KC;
    q.nch_c1 = P * p.H / BGEMM_KC;
    q.cond0_A = take((size_t)p.c.n_flows * q.nch_c0 * BGEMM_KC * BGEMM_BM);
    q.cond1_A = take((size_t)p.c.n_flows * q.nch_c1 * BGEMM_KC * BGEMM_BM);
    q.mb_c = (p.C + BGEMM_BM - 1) / BGEMM_BM;
    q.n_groups = (p.c.n_layers + BF_SKIP_GROUP - 1) / BF_SKIP_GROUP;
    q.in_A.assign(p.c.n_flows, {});
    q.rs_A.assign(p.c.n_flows, {});
    q.skip_A.assign(p.c.n_flows, {});
    for (int k = 0; k < p.c.n_flows; ++k) {
        for (int i = 0; i < p.c.n_layers; ++i) {
            q.in_A[k].push_back(take((size_t)p.mb_in * q.nch_in * BGEMM_KC * BGEMM_BM));
            q.rs_A[k].push_back(i < p.c.n_layers - 1 ? take((size_t)q.mb_c * q.nch_rs * BGEMM_KC * BGEMM_BM) : 0);
        }
        for (int gi = 0; gi < q.n_groups; ++gi)
            q.skip_A[k].push_back(take((size_t)q.mb_c * q.group_layers(gi, p.c.n_layers) * q.nch_rs * BGEMM_KC * BGEMM_BM));
        q.skip_b.push_back(take((size_t)2 * 2 * q.mb_c * BGEMM_BM));        // fp32 pairs of bf16 slots
    }
    q.total = o;
}

// bf16 tensors of the split form are PAIRS of planes: hi at the pointer, lo at pointer + *_lo elements (0 = plain bf16)
struct BfWs {
    float *audio, *spect, *spk;
    bf16_t *spect_bf, *spk_bf, *h_tmp_bf, *h_bf, *x, *act, *out;
    long long spect_lo, spk_lo, h_lo, x_lo, act_lo;
    size_t total_bytes;
};

void carve_bf(const Plan& p, const Geom& g, int batch, char* base, BfWs& w, int P) {
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = (o + bytes + 255) / 256 * 256; return base ? base + r : nullptr; };
    const size_t B = batch;
    const size_t planes = P == 3 ? 2 : 1;
    w.audio = (float*)take(B * p.c.n_group * g.L * 4);
    w.spect = (float*)take(B * p.K0 * g.ld * 4);
    w.spect_bf = (bf16_t*)take(planes * B * p.K0 * g.ld * 2);
    w.spk = (float*)take(B * p.c.n_flows * p.S * g.ld * 4);
    w.spk_bf = (bf16_t*)take(planes * B * p.c.n_flows * p.S * g.ld * 2);
    w.h_tmp_bf = (bf16_t*)take(planes * B * p.c.n_flows * p.H * g.ld * 2);
    w.h_bf = (bf16_t*)take(planes * B * p.c.n_flows * p.H * g.ld * 2);
    w.x = (bf16_t*)take(planes * B * p.C * g.ld * 2);
    w.act = (bf16_t*)take(planes * B * p.C * g.ld * 2 * std::min(p.c.n_layers, BF_SKIP_GROUP));   // one buffer per layer of a skip group
    w.out = (bf16_t*)take(planes * B * p.C * g.ld * 2);
    const long long on = P == 3 ? 1 : 0;
    w.spect_lo = on * (long long)(B * p.K0 * g.ld);
    w.spk_lo = on * (long long)(B * p.c.n_flows * p.S * g.ld);
    w.h_lo = on * (long long)(B * p.c.n_flows * p.H * g.ld);
    w.x_lo = on * (long long)(B * p.C * g.ld);
    w.act_lo = on * (long long)(B * p.C * g.ld) * std::min(p.c.n_layers, BF_SKIP_GROUP);
    w.total_bytes = o;
}

// K segments of one operand: bf16 = the tensor itself; split bf16 = (hi, lo, hi) against the packed (W_hi, W_hi, W_lo)
int push_segs(BGemmArgs& a, int idx, int P, const bf16_t* base, long long lo_off, long long bstride, int nch, int shift,
              int mb_rows) {
    for (int pi = 0; pi < P; ++pi) a.seg[idx++] = {pi == 1 ? base + lo_off : base, bstride, nch, shift, mb_rows};
    return idx;
}

// fp32 padded [B][rows][ld] -> bf16 K8 [B][rows/8][ld][8]
__device__ __forceinline__ unsigned int pack_bf16x2_residual(float v0, float v1, unsigned int hi) {
    return pack_bf16x2(v0 - __builtin_bit_cast(float, hi << 16), v1 - __builtin_bit_cast(float, hi & 0xffff0000u));
}

__global__ __launch_bounds__(256) void cvt_f32_to_k8_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst,
                                                            int rows, int ld, long long lo_off, int f16) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int grp = blockIdx.y, b = blockIdx.z;
    if (n >= ld) return;
    const float* s = src + ((size_t)b * rows + (size_t)grp * 8) * ld + n;
    unsigned int pk[4], pl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v0 = s[(size_t)(2 * j) * ld], v1 = s[(size_t)(2 * j + 1) * ld];
        pk[j] = f16 ? pack_f16x2(v0, v1) : pack_bf16x2(v0, v1);
        pl[j] = pack_bf16x2_residual(v0, v1, pk[j]);        // (only stored in the split-bf16 form: lo_off != 0)
    }
    bf16_t* d = dst + (((size_t)b * (rows / 8) + grp) * ld + n) * 8;
    *reinterpret_cast<uint4*>(d) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    if (lo_off) *reinterpret_cast<uint4*>(d + lo_off) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
}

// x[b][c][n] = bf16(bs[c] + sum_j Ws[c][j] * audio[b][ch_off + j][n]), K8 layout   (glow.py:189)
template <int H>
__global__ __launch_bounds__(256) void wn_start_bf16_kernel(const float* __restrict__ audio, const float* __restrict__ Ws,
                                                            const float* __restrict__ bs, bf16_t* __restrict__ x, int C,
                                                            int G, int ch_off, int L, int ld, int pad, long long lo_off, int f16) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int grp = blockIdx.y, b = blockIdx.z;
    if (n >= L) return;
    float a[H];
#pragma unroll
    for (int j = 0; j < H; ++j) a[j] = audio[((size_t)b * G + ch_off + j) * L + n];
    unsigned int pk[4], pl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = grp * 8 + 2 * q + e;
            float acc = bs[c];
#pragma unroll
            for (int j = 0; j < H; ++j) acc = fmaf(Ws[c * H + j], a[j], acc);
            v[e] = acc;
        }
        pk[q] = f16 ? pack_f16x2(v[0], v[1]) : pack_bf16x2(v[0], v[1]);
        pl[q] = pack_bf16x2_residual(v[0], v[1], pk[q]);
    }
    bf16_t* d = x + (((size_t)b * (C / 8) + grp) * ld + pad + n) * 8;
    *reinterpret_cast<uint4*>(d) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    if (lo_off) *reinterpret_cast<uint4*>(d + lo_off) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
}

// end 1x1 conv on the bf16 skip sum + coupling inverse + inverse 1x1 (+ un-squeeze), fp32 math
// FMT: 0 = bf16, 1 = split bf16 (hi + lo planes), 2 = IEEE half - a compile-time choice: with `lo_off` tested at run time the
// compiler put a branch and a full `vmcnt(0)` behind every 16-byte load of the skip sum (0.97 ms per launch at config 3 = 1 TB/s;
// round 5).  Eight groups of loads are in flight before the first is used.
template <int H, int FMT>
__global__ __launch_bounds__(256) void flow_tail_bf16_kernel(const bf16_t* __restrict__ out, float* __restrict__ audio,
                                                             float* __restrict__ wave, const float* __restrict__ Wend,
                                                             const float* __restrict__ bend, const float* __restrict__ Winv,
                                                             int C, int G, int ch_off, int L, int ld, int pad,
                                                             long long lo_off) {
    constexpr int E = 2 * H;
    constexpr int NG = 8;                                    // groups (of 8 channels) per batch of loads
    __shared__ float sW[E * 512 + E * E + E];
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    for (int i = threadIdx.x; i < E * C; i += 256) sW[i] = Wend[i];
    if (threadIdx.x < E * E) sW[E * C + threadIdx.x] = Winv[threadIdx.x];
    if (threadIdx.x < E) sW[E * C + E * E + threadIdx.x] = bend[threadIdx.x];
    __syncthreads();
    if (n >= L) return;
    float e[E];
#pragma unroll
    for (int j = 0; j < E; ++j) e[j] = sW[E * C + E * E + j];
    const uint4* ob = reinterpret_cast<const uint4*>(out) + ((size_t)b * (C / 8)) * ld + pad + n;
    auto accumulate = [&](const uint4& uu, const uint4& ll, int grp) {
        const unsigned int w4[4] = {uu.x, uu.y, uu.z, uu.w}, l4[4] = {ll.x, ll.y, ll.z, ll.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v0, v1;
            if constexpr (FMT == 2) {
                v0 = f16_to_f32((bf16_t)(w4[q] & 0xffff));
                v1 = f16_to_f32((bf16_t)(w4[q] >> 16));
            } else {
                v0 = bf16_to_f32((bf16_t)(w4[q] & 0xffff));
                v1 = bf16_to_f32((bf16_t)(w4[q] >> 16));
                if constexpr (FMT == 1) {
                    v0 += bf16_to_f32((bf16_t)(l4[q] & 0xffff));
                    v1 += bf16_to_f32((bf16_t)(l4[q] >> 16));
                }
            }
            const int c = grp * 8 + 2 * q;
#pragma unroll
            for (int j = 0; j < E; ++j) e[j] = fmaf(sW[j * C + c + 1], v1, fmaf(sW[j * C + c], v0, e[j]));
        }
    };
    auto load_lo = [&](int grp) -> uint4 {
        if constexpr (FMT == 1)
            return *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(ob + (size_t)grp * ld) + lo_off);
        else
            return make_uint4(0u, 0u, 0u, 0u);
    };
    int g0 = 0;
    for (; g0 + NG <= C / 8; g0 += NG) {                     // whole batches: all NG loads issued before the first use
        uint4 u[NG], ul[NG];
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            u[k] = ob[(size_t)(g0 + k) * ld];
            ul[k] = load_lo(g0 + k);
        }
#pragma unroll
        for (int k = 0; k < NG; ++k) accumulate(u[k], ul[k], g0 + k);
    }
    for (; g0 < C / 8; ++g0) accumulate(ob[(size_t)g0 * ld], load_lo(g0), g0);   // narrow test widths
    float* ab = audio + ((size_t)b * G + ch_off) * L + n;
    float a[E];
#pragma unroll
    for (int j = 0; j < E; ++j) a[j] = ab[(size_t)j * L];
#pragma unroll
    for (int j = 0; j < H; ++j) a[H + j] = (a[H + j] - e[j]) / expf(e[H + j]);
    float m[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < E; ++j) s = fmaf(sW[E * C + i * E + j], a[j], s);
        m[i] = s;
    }
    if (wave == nullptr) {
#pragma unroll
        for (int i = 0; i < E; ++i) ab[(size_t)i * L] = m[i];
    } else {
        float* wb = wave + (size_t)b * G * L + (size_t)n * G;
#pragma unroll
        for (int i = 0; i < E; ++i) wb[i] = m[i];
    }
}

// dst[0 .. n) (+)= src[0 .. C) for rows < C; first call clears the whole array (incl. the zero half)
__global__ __launch_bounds__(256) void skip_bias_kernel(float* __restrict__ dst, const float* __restrict__ src, int C, int n,
                                                        int first) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = i < C ? src[i] : 0.f;
    dst[i] = first ? v : dst[i] + v;
}

int run_wn_stack_bf16(const Plan& p, const BfPlan& q, const Geom& g, const float* blob, const bf16_t* bblob, int k,
                      const BfWs& w, int batch, hipStream_t s) {
    const auto& f = p.fl[k];
    const auto& d = p.fd[k];
    const long long cstride = (long long)p.C * g.ld;                 // elements per batch item (K8: (C/8)*ld*8)
    const long long hstride = (long long)p.c.n_flows * p.H * g.ld;
    dim3 sgrid((g.L + 255) / 256, p.C / 8, batch);
#define CTTS_BSTART(HH)                                                                                       \
    case HH:                                                                                                  \
        hipLaunchKernelGGL(wn_start_bf16_kernel<HH>, sgrid, dim3(256), 0, s, w.audio, blob + f.start_w,       \
                           blob + f.start_b, w.x, p.C, p.c.n_group, d.ch_off, g.L, g.ld, g.pad, w.x_lo, q.f16); \
        break;
    switch (d.n_half) {
        CTTS_BSTART(1) CTTS_BSTART(2) CTTS_BSTART(3) CTTS_BSTART(4)
        default: set_error("wn_start_bf16: n_half=%d", d.n_half); return CTTS_E_ARG;
    }
#undef CTTS_BSTART
    CTTS_CHECK_LAUNCH("wn_start_bf16");
    const int ncx = p.C / BGEMM_KC, P = q.P, ks = p.c.kernel_size;
    const size_t act_layer = (size_t)batch * cstride;
    int rc;
    const float* skip_b = reinterpret_cast<const float*>(bblob + q.skip_b[k]);
    // skip sum = sum_i W_skip_i act_i + sum_i b_skip_i: K = n_layers * C, fp32 accumulation inside a launch (one launch at the
    // end of each group of BF_SKIP_GROUP layers, over the group's kept activations - the next group reuses their slots), one
    // rounding of the running sum per group of BF_SKIP_GROUP layers
    auto skip_group = [&](int gi) -> int {
        const int nl = q.group_layers(gi, p.c.n_layers);
        BGemmArgs a{};
        a.f16 = q.f16;
        a.ld = g.ld; a.pad = g.pad; a.L = g.L; a.ntiles = g.ntiles; a.batch = batch;
        a.A = bblob + q.skip_A[k][gi]; a.bias = skip_b + (gi == 0 ? 0 : q.mb_c * BGEMM_BM);
        int ns = 0;
        for (int j = 0; j < nl; ++j)
            ns = push_segs(a, ns, P, w.act + (size_t)j * act_layer, w.act_lo, cstride, ncx, 0, 0);
        a.nseg = ns; a.nch_total = nl * q.nch_rs; a.MB = q.mb_c;
        a.M = p.C; a.split = p.C;
        a.dst0 = w.out; a.dst0_bstride = cstride; a.acc0 = gi > 0 ? 1 : 0;
        a.dst1 = w.out; a.dst1_bstride = cstride; a.acc1 = a.acc0;
        a.lo_off = w.x_lo;
        ProfScope ps(CTTS_PROF_WN_SKIP, s);
        return launch_gemm_bf16(BGEMM_EPI_SPLIT, a, s);
    };
    for (int i = 0; i < p.c.n_layers; ++i) {
        const int dil = 1 << i;
        bf16_t* act = w.act + (size_t)(i % BF_SKIP_GROUP) * act_layer;
        {
            BGemmArgs a{};
            a.f16 = q.f16;
            a.ld = g.ld; a.pad = g.pad; a.L = g.L; a.ntiles = g.ntiles; a.batch = batch;
            a.A = bblob + q.in_A[k][i]; a.bias = blob + f.in_b[i];
            int ns = 0;
            for (int t = 0; t < ks; ++t) ns = push_segs(a, ns, P, w.x, w.x_lo, cstride, ncx, (t - ks / 2) * dil, 0);
            a.interleave = ns;                                        // taps (x products) round-robin per 32-channel slab
            ns = push_segs(a, ns, P, w.h_bf + (size_t)k * p.H * g.ld, w.h_lo, hstride, p.H / BGEMM_KC, 0, 0);
            a.nseg = ns; a.nch_total = q.nch_in; a.MB = p.mb_in;
            a.M = 2 * p.C; a.pairC = p.C;
            a.dst0 = act; a.dst0_bstride = cstride; a.lo_off = w.act_lo;
            ProfScope ps(CTTS_PROF_WN_IN, s);
            if ((rc = launch_gemm_bf16(BGEMM_EPI_GATE, a, s))) return rc;
        }
        if (i < p.c.n_layers - 1) {
            // x += W_res act + b_res   (glow.py:213-217; the skip rows wait for the end of the stack)
            BGemmArgs a{};
            a.f16 = q.f16;
            a.ld = g.ld; a.pad = g.pad; a.L = g.L; a.ntiles = g.ntiles; a.batch = batch;
            a.A = bblob + q.rs_A[k][i]; a.bias = blob + f.rs_b[i];
            a.nseg = push_segs(a, 0, P, act, w.act_lo, cstride, ncx, 0, 0); a.nch_total = q.nch_rs; a.MB = q.mb_c;
            a.M = p.C; a.split = p.C;
            a.dst0 = w.x; a.dst0_bstride = cstride; a.acc0 = 1;
            a.dst1 = w.x; a.dst1_bstride = cstride; a.acc1 = 1;
            a.lo_off = w.x_lo;
            ProfScope ps(CTTS_PROF_WN_RS, s);
            if ((rc = launch_gemm_bf16(BGEMM_EPI_SPLIT, a, s))) return rc;
        }
        if (i == p.c.n_layers - 1 || (i + 1) % BF_SKIP_GROUP == 0) {
            if ((rc = skip_group(i / BF_SKIP_GROUP))) return rc;
        }
    }
    return CTTS_OK;
}

}  // namespace
}  // namespace ctts

using namespace ctts;

extern "C" {

int ctts_abi_version(void) { return CTTS_ABI_VERSION; }
const char* ctts_last_error(void) { return g_err; }

int ctts_waveglow_geometry_for(const ctts_waveglow_config* cfg, int32_t frames, ctts_waveglow_geometry* out) {
    Plan p; Geom g;
    int rc = make_plan(cfg, p); if (rc) return rc;
    rc = make_geom(p, frames, g); if (rc) return rc;
    CTTS_CHECK_ARG(out != nullptr, "geometry out is NULL");
    out->steps = g.L; out->ld = g.ld; out->pad = g.pad; out->n_remaining = p.fd.back().n_rem;
    return CTTS_OK;
}

int ctts_fold_weightnorm_f32(const float* v, const float* g, float* w, int32_t out_ch, int32_t fan, void* stream) {
    CTTS_CHECK_ARG(v && g && w, "fold_weightnorm: NULL pointer");
    return launch_fold_weightnorm(v, g, w, out_ch, fan, as_stream(stream));
}

size_t ctts_waveglow_packed_bytes(const ctts_waveglow_config* cfg) {
    Plan p;
    if (make_plan(cfg, p)) return 0;
    return p.total * sizeof(float);
}

int ctts_waveglow_pack_upsample(const ctts_waveglow_config* cfg, const float* up_w, const float* up_b, void* packed,
                                void* stream) {
    Plan p;
    int rc = make_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(up_w && up_b && packed, "pack_upsample: NULL pointer");
    float* blob = static_cast<float*>(packed);
    const size_t nw = (size_t)p.c.n_mel_channels * p.c.n_mel_channels * p.c.win_length;
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + p.up_w, up_w, nw * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    CTTS_CHECK_HIP(hipMemcpyAsync(blob + p.up_b, up_b, p.c.n_mel_channels * sizeof(float), hipMemcpyDeviceToDevice,
                                  as_stream(stream)));
    if (p.up_mfma) return launch_upsample_pack_mfma(up_w, blob + p.up_wp, as_stream(stream));
    return CTTS_OK;
}

int ctts_waveglow_pack_flow(const ctts_waveglow_config* cfg, int32_t k, const ctts_waveglow_flow_weights* w,
                            void* packed, void* stream) {
    Plan p;
    int rc = make_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(k >= 0 && k < p.c.n_flows, "pack_flow: flow %d", k);
    CTTS_CHECK_ARG(w && packed, "pack_flow: NULL pointer");
    hipStream_t s = as_stream(stream);
    float* blob = static_cast<float*>(packed);
    const auto& f = p.fl[k];
    const auto& d = p.fd[k];
    const int C = p.C, H = p.H, ks = p.c.kernel_size;
    auto d2d = [&](size_t off, const float* src, size_t n) -> int {
        CTTS_CHECK_ARG(src != nullptr, "pack_flow: NULL weight pointer");
        CTTS_CHECK_HIP(hipMemcpyAsync(blob + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return CTTS_OK;
    };
    if ((rc = d2d(f.start_w, w->start_w, (size_t)C * d.n_half))) return rc;
    if ((rc = d2d(f.start_b, w->start_b, C))) return rc;
    if ((rc = d2d(f.end_w, w->end_w, (size_t)2 * d.n_half * C))) return rc;
    if ((rc = d2d(f.end_b, w->end_b, 2 * d.n_half))) return rc;
    if ((rc = d2d(f.winv, w->w_inverse, (size_t)d.n_rem * d.n_rem))) return rc;
    // cond layers 0/1: this flow is M-block k of the flow-batched GEMMs
    CTTS_CHECK_ARG(w->cond_w[0] && w->cond_w[1] && w->cond_w[2] && w->cond_b[0] && w->cond_b[1] && w->cond_b[2],
                   "pack_flow: NULL cond weights");
    // cond layer 0 is [H][n_mel*G + speaker_embed_dim] (glow.py:155): spectrogram columns, then the embedding columns
    // (K rows [K0 + sdim, K0 + S) stay zero from the blob's zero fill)
    const int sdim = p.c.speaker_embed_dim;
    if ((rc = launch_pack_a(blob + p.cond0_A + (size_t)k * p.nch0 * A_TILE, w->cond_w[0], GEMM_BM, 1, p.nch0, 0, p.K0,
                            GEMM_EPI_SPLIT, C, H, 0, p.K0 + sdim, 1, s))) return rc;
    if (sdim) {
        if ((rc = launch_pack_a(blob + p.cond0_A + (size_t)k * p.nch0 * A_TILE, w->cond_w[0] + p.K0, GEMM_BM, 1, p.nch0,
                                p.K0, sdim, GEMM_EPI_SPLIT, C, H, 0, p.K0 + sdim, 1, s))) return rc;
        if ((rc = d2d(f.spk_tab, w->speaker_embed, (size_t)CTTS_N_SPEAKERS * sdim))) return rc;
    }
    if ((rc = launch_pack_bias(blob + p.cond0_b + (size_t)k * GEMM_BM, GEMM_BM, 1, w->cond_b[0], 0, nullptr, 0,
                               GEMM_EPI_SPLIT, C, H, s))) return rc;
    if ((rc = launch_pack_a(blob + p.cond1_A + (size_t)k * p.nch1h * A_TILE, w->cond_w[1], GEMM_BM, 1, p.nch1h, 0, H,
                            GEMM_EPI_SPLIT, C, H, 0, H, 1, s))) return rc;
    if ((rc = launch_pack_bias(blob + p.cond1_b + (size_t)k * GEMM_BM, GEMM_BM, 1, w->cond_b[1], 0, nullptr, 0,
                               GEMM_EPI_SPLIT, C, H, s))) return rc;
    for (int i = 0; i < p.c.n_layers; ++i) {
        CTTS_CHECK_ARG(w->in_w[i] && w->in_b[i] && w->rs_w[i] && w->rs_b[i], "pack_flow: NULL layer %d weights", i);
        // in-layer: K = [per 16-channel slab: tap0, tap1, tap2] then [cond];  in_w[i] is [2C][C][ks]
        for (int t = 0; t < ks; ++t)
            if ((rc = launch_pack_a(blob + f.in_A[i], w->in_w[i] + t, GEMM_BM, p.mb_in, p.nch_in, 0, C, GEMM_EPI_GATE, C,
                                    2 * C, 0, (long long)C * ks, ks, s, ks, t))) return rc;
        // cond layer 2 rows [2C*i, 2C*(i+1)) of [2C*n_layers][H]
        if ((rc = launch_pack_a(blob + f.in_A[i], w->cond_w[2], GEMM_BM, p.mb_in, p.nch_in, ks * C, H, GEMM_EPI_GATE, C,
                                2 * C, (long long)2 * C * i, H, 1, s))) return rc;
        if ((rc = launch_pack_bias(blob + f.in_b[i], GEMM_BM, p.mb_in, w->in_b[i], 0, w->cond_b[2], (long long)2 * C * i,
                                   GEMM_EPI_GATE, C, 2 * C, s))) return rc;
        const int rows = p.rs_rows(i);
        if ((rc = launch_pack_a(blob + f.rs_A[i], w->rs_w[i], GEMM_BM, p.rs_mb(i), p.nch_rs, 0, C, GEMM_EPI_SPLIT, C, rows,
                                0, C, 1, s))) return rc;
        if ((rc = launch_pack_bias(blob + f.rs_b[i], GEMM_BM, p.rs_mb(i), w->rs_b[i], 0, nullptr, 0, GEMM_EPI_SPLIT, C, rows,
                                   s))) return rc;
        // deferred-skip form: res rows [0, C) alone; skip rows ([C, 2C), or [0, C) of the last layer) at K offset
        // (member of the group) * C of the group's matrix, skip biases summed per group
        const bool last = i == p.c.n_layers - 1;
        const int gi = i / Plan::F32_SKIP_GROUP, gj = i % Plan::F32_SKIP_GROUP;
        if (!last) {
            if ((rc = launch_pack_a(blob + f.res_A[i], w->rs_w[i], GEMM_BM, p.mb_c(), p.nch_rs, 0, C, GEMM_EPI_SPLIT, C, C,
                                    0, C, 1, s))) return rc;
            if ((rc = launch_pack_bias(blob + f.res_b[i], GEMM_BM, p.mb_c(), w->rs_b[i], 0, nullptr, 0, GEMM_EPI_SPLIT, C, C,
                                       s))) return rc;
        }
        if ((rc = launch_pack_a(blob + f.skip_A[gi], w->rs_w[i], GEMM_BM, p.mb_c(), p.group_layers(gi) * p.nch_rs, gj * C, C,
                                GEMM_EPI_SPLIT, C, C, last ? 0 : C, C, 1, s))) return rc;
        hipLaunchKernelGGL(skip_bias_kernel, dim3((p.mb_c() * GEMM_BM + 255) / 256), dim3(256), 0, s, blob + f.skip_b[gi],
                           w->rs_b[i] + (last ? 0 : C), C, p.mb_c() * GEMM_BM, gj == 0 ? 1 : 0);
        CTTS_CHECK_LAUNCH("skip_bias_f32");
    }
    // one [U | C_i] GATE matrix of the Winograd forms (pair rows, like in_A; K = C + H): U [2C][C] with row stride u_ld and element
    // stride u_step, then the cond slice of layer i
    auto pack_gate = [&](size_t A, const float* U, long long u_ld, int u_step, int i) -> int {
        const int nch = p.nch_rs + p.nch1h;
        const int rc = launch_pack_a(blob + A, U, GEMM_BM, p.mb_in, nch, 0, C, GEMM_EPI_GATE, C, 2 * C, 0, u_ld, u_step, s);
        return rc ? rc : launch_pack_a(blob + A, w->cond_w[2], GEMM_BM, p.mb_in, nch, C, H, GEMM_EPI_GATE, C, 2 * C, (long long)2 * C * i, H, 1, s);
    };
    // Winograd F(2,3) in-layer form: G2, G3 (dense rows: T2 / T3 are addends in dense row order) and [W0 | C_i], [-W2 | C_i];
    // the dense scratch is reused layer by layer (one stream)
    for (int i = 0; i < p.c.n_layers; ++i) {
        float* dense = blob + f.wg_dense;
        const size_t dn = (size_t)2 * C * C;
        if ((rc = launch_winograd_g(w->in_w[i], dense, 2 * C, C, s))) return rc;
        if ((rc = launch_pack_a(blob + f.wg_T2_A[i], dense, GEMM_BM, p.mb_in, p.nch_rs, 0, C, GEMM_EPI_SPLIT, C, 2 * C, 0, C, 1, s))) return rc;
        if ((rc = launch_pack_a(blob + f.wg_T3_A[i], dense + dn, GEMM_BM, p.mb_in, p.nch_rs, 0, C, GEMM_EPI_SPLIT, C, 2 * C, 0, C, 1, s))) return rc;
        if ((rc = pack_gate(f.wg_e_A[i], w->in_w[i], (long long)C * ks, ks, i))) return rc;          // W0: tap 0 of in_w
        if ((rc = pack_gate(f.wg_o_A[i], dense + 2 * dn, C, 1, i))) return rc;
    }
    // Winograd F(4,3) form: U1..U4 (dense rows, SPLIT) and [U0 | C_i], [U5 | C_i] (pair rows, GATE) through the same dense scratch
    for (int i = 0; i < (f.wq_e_A.empty() ? 0 : p.c.n_layers); ++i) {
        float* dense = blob + f.wg_dense;
        const size_t dn = (size_t)2 * C * C;
        if ((rc = launch_winograd_g43(w->in_w[i], dense, 2 * C, C, s))) return rc;
        for (int j = 0; j < 4; ++j)
            if ((rc = launch_pack_a(blob + f.wq_U_A[j][i], dense + (1 + j) * dn, GEMM_BM, p.mb_in, p.nch_rs, 0, C, GEMM_EPI_SPLIT, C, 2 * C, 0, C, 1, s))) return rc;
        if ((rc = pack_gate(f.wq_e_A[i], dense, C, 1, i))) return rc;
        if ((rc = pack_gate(f.wq_o_A[i], dense + 5 * dn, C, 1, i))) return rc;
    }
    // Winograd F(6,3) form of the layers it can engage at: U1..U6 (SPLIT) and [U0 | C_i], [U7 | C_i] (GATE) through the same dense scratch
    for (int i = 0; i < (f.wh_e_A.empty() ? 0 : p.c.n_layers); ++i) {
        if (!f63_layer(i)) continue;
        float* dense = blob + f.wg_dense;
        const size_t dn = (size_t)2 * C * C;
        if ((rc = launch_winograd_g63(w->in_w[i], dense, 2 * C, C, s))) return rc;
        for (int j = 0; j < 6; ++j)
            if ((rc = launch_pack_a(blob + f.wh_U_A[j][i], dense + (1 + j) * dn, GEMM_BM, p.mb_in, p.nch_rs, 0, C, GEMM_EPI_SPLIT, C, 2 * C, 0, C, 1, s))) return rc;
        if ((rc = pack_gate(f.wh_e_A[i], dense, C, 1, i))) return rc;
        if ((rc = pack_gate(f.wh_o_A[i], dense + 7 * dn, C, 1, i))) return rc;
    }
    // WN start / end folds: layer 0 on [audio_0; 1] (K = [tap0, tap1, tap2] of one FOLD_ROWS chunk each, then the cond slice of
    // layer 0; bias in_b[0] as packed above) and the skip rows seen through `end`
    if ((rc = launch_fold_in0(w->in_w[0], w->start_w, w->start_b, blob + f.in0f_w, C, d.n_half, ks, s))) return rc;
    for (int t = 0; t < ks; ++t)
        if ((rc = launch_pack_a(blob + f.in0f_A, blob + f.in0f_w + t, GEMM_BM, p.mb_in, p.nch_in0f, 0, FOLD_ROWS, GEMM_EPI_GATE, C,
                                2 * C, 0, (long long)FOLD_ROWS * ks, ks, s, ks, t))) return rc;
    if ((rc = launch_pack_a(blob + f.in0f_A, w->cond_w[2], GEMM_BM, p.mb_in, p.nch_in0f, ks * FOLD_ROWS, H, GEMM_EPI_GATE, C,
                            2 * C, 0, H, 1, s))) return rc;
    return launch_fold_skend(w->rs_w, w->rs_b, w->end_w, w->end_b, blob + f.skend_W, blob + f.skend_b, C, p.c.n_layers, d.n_half, s);
}

size_t ctts_waveglow_packed_bytes_opt(const ctts_waveglow_config* cfg, int32_t options) {
    Plan p;
    if (make_plan(cfg, p, options)) return 0;
    return p.total * sizeof(float);
}

int ctts_waveglow_has_composed_cond(const ctts_waveglow_config* cfg) {
    Plan p;
    return make_plan(cfg, p, CTTS_WG_OPT_COMPOSED_COND) == CTTS_OK && p.cc ? 1 : 0;
}

// this flow's ccP M-blocks of the composed conditioning, from the dense cond layers and the upsampling weights the blob already holds
int ctts_waveglow_pack_cond_composed(const ctts_waveglow_config* cfg, int32_t k, const ctts_waveglow_flow_weights* w, void* packed,
                                     void* stream) {
    Plan p;
    int rc = make_plan(cfg, p, CTTS_WG_OPT_COMPOSED_COND); if (rc) return rc;
    CTTS_CHECK_ARG(p.cc, "pack_cond_composed: this config has no composed conditioning (ctts_waveglow_has_composed_cond)");
    CTTS_CHECK_ARG(k >= 0 && k < p.c.n_flows, "pack_cond_composed: flow %d", k);
    CTTS_CHECK_ARG(w && packed && w->cond_w[0] && w->cond_w[1] && w->cond_b[0] && w->cond_b[1], "pack_cond_composed: NULL pointer");
    hipStream_t s = as_stream(stream);
    float* blob = static_cast<float*>(packed);
    const int H = p.H;
    double* w10 = reinterpret_cast<double*>(blob + p.cc_w10) + (size_t)k * H * p.K0;
    hipLaunchKernelGGL(cond_compose_w10_kernel, dim3((p.K0 + 255) / 256, H), dim3(256), 0, s, w->cond_w[1], w->cond_w[0], w10, H, p.K0);
    hipLaunchKernelGGL(cond_compose_A_kernel, dim3(p.ccJ * p.c.n_mel_channels, p.ccP), dim3(GEMM_BM), 0, s, w10, blob + p.up_w,
                       blob + p.cc_A + (size_t)k * p.ccP * p.nch_cc * A_TILE, p.c.n_mel_channels, p.c.n_group, p.c.hop_length,
                       p.c.win_length, p.ccP, p.nch_cc);
    hipLaunchKernelGGL(cond_compose_bias_kernel, dim3(1), dim3(GEMM_BM), 0, s, w->cond_w[0], w->cond_b[0], w->cond_w[1], w->cond_b[1],
                       blob + p.up_b, blob + p.cc_b + (size_t)k * p.ccP * GEMM_BM, p.K0, p.c.n_group, p.ccP);
    CTTS_CHECK_LAUNCH("cond_compose");
    return CTTS_OK;
}

size_t ctts_waveglow_workspace_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames) {
    return ctts_waveglow_workspace_bytes_opt(cfg, batch, frames, 0);
}

size_t ctts_waveglow_workspace_bytes_opt(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames, int32_t options) {
    Plan p; Geom g; Workspace w;
    if (make_plan(cfg, p, options) || make_geom(p, frames, g) || batch < 1) return 0;
    const Tuning t = tuning();
    carve(p, g, batch, nullptr, in_form(p, g, t), cond_composed(p, frames, t), w);
    return w.total * sizeof(float);
}

int ctts_upsample_squeeze_f32(const ctts_waveglow_config* cfg, const void* packed, const float* mel, float* spect,
                              int32_t batch, int32_t frames, void* stream) {
    WnCall c;
    const int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    CTTS_CHECK_ARG(packed && mel && spect && batch >= 1, "upsample_squeeze: bad argument");
    return c.upsample(mel, spect);
}

int ctts_wn_cond_f32(const ctts_waveglow_config* cfg, const void* packed, const float* spect, const float* spk_rows,
                     float* h_tmp, float* h_all, int32_t batch, int32_t frames, void* stream) {
    WnCall c;
    const int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    CTTS_CHECK_ARG(packed && spect && h_tmp && h_all && batch >= 1, "wn_cond: bad argument");
    return c.cond(spect, spk_rows, h_tmp, h_all);
}

size_t ctts_wn_cond_composed_scratch_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames) {
    Plan p;
    if (make_plan(cfg, p, CTTS_WG_OPT_COMPOSED_COND) || !p.cc || batch < 1 || frames < 1) return 0;
    return (size_t)batch * p.c.n_mel_channels * mel_geom(frames).ld * sizeof(float);
}

// (the composed form on the caller's buffers, whatever the knob says)
int ctts_wn_cond_composed_f32(const ctts_waveglow_config* cfg, const void* packed, const float* mel, float* scratch, float* h_all,
                              int32_t batch, int32_t frames, void* stream) {
    WnCall c;
    const int rc = c.begin(cfg, packed, batch, frames, stream, CTTS_WG_OPT_COMPOSED_COND); if (rc) return rc;
    CTTS_CHECK_ARG(packed && mel && scratch && h_all && batch >= 1, "wn_cond_composed: bad argument");
    return c.cond_from_mel(mel, scratch, h_all);
}

// (the per-layer stack with direct in-layers on the caller's buffers, whatever the knobs say)
int ctts_wn_stack_f32(const ctts_waveglow_config* cfg, const void* packed, int32_t flow, const float* audio,
                      const float* h_all, float* x, float* act, float* out, int32_t batch, int32_t frames,
                      void* stream) {
    WnCall c;
    const int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    CTTS_CHECK_ARG(flow >= 0 && flow < c.p.c.n_flows, "wn_stack: flow %d", flow);
    CTTS_CHECK_ARG(packed && audio && h_all && x && act && out && batch >= 1, "wn_stack: bad argument");
    c.w.x = x; c.w.act = act; c.w.out = out; c.h_all = h_all;
    return c.stack_per_layer(flow, audio);
}

int ctts_flow_tail_f32(const ctts_waveglow_config* cfg, const void* packed, int32_t flow, const float* out,
                       float* audio, float* wave, int32_t batch, int32_t frames, void* stream) {
    WnCall c;
    const int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    CTTS_CHECK_ARG(flow >= 0 && flow < c.p.c.n_flows, "flow_tail: flow %d", flow);
    CTTS_CHECK_ARG(packed && out && audio && batch >= 1, "flow_tail: bad argument");
    return c.flow_tail(flow, out, audio, wave, nullptr);
}

int ctts_waveglow_flow_f32(const ctts_waveglow_config* cfg, const void* packed, int32_t flow, float* audio,
                           const float* h_all, float* wave, int32_t batch, int32_t frames, void* workspace,
                           size_t workspace_bytes, void* stream) {
    WnCall c;
    int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    CTTS_CHECK_ARG(flow >= 0 && flow < c.p.c.n_flows, "waveglow_flow: flow %d", flow);
    CTTS_CHECK_ARG(packed && audio && h_all && workspace && batch >= 1, "waveglow_flow: bad argument");
    if ((rc = c.take_workspace("waveglow_flow", workspace, workspace_bytes, false))) return rc;
    c.audio = audio; c.h_all = h_all;
    return c.run_flow(flow, wave, nullptr);
}

size_t ctts_waveglow_forward_packed_bytes(const ctts_waveglow_config* cfg) {
    Plan p;
    if (make_plan(cfg, p)) return 0;
    return fwd_mix_off(p, p.c.n_flows) * sizeof(float);
}

int ctts_waveglow_pack_forward_mix(const ctts_waveglow_config* cfg, int32_t flow, const float* w, void* packed_fwd,
                                   void* stream) {
    Plan p;
    int rc = make_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(flow >= 0 && flow < p.c.n_flows, "pack_forward_mix: flow %d", flow);
    CTTS_CHECK_ARG(w && packed_fwd, "pack_forward_mix: NULL pointer");
    const size_t n = (size_t)p.fd[flow].n_rem * p.fd[flow].n_rem;
    CTTS_CHECK_HIP(hipMemcpyAsync(static_cast<float*>(packed_fwd) + fwd_mix_off(p, flow), w, n * sizeof(float),
                                  hipMemcpyDeviceToDevice, as_stream(stream)));
    return CTTS_OK;
}

size_t ctts_waveglow_forward_workspace_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames) {
    Plan p; Geom g; Workspace w; FwdSums f;
    if (make_plan(cfg, p) || make_geom(p, frames, g)) return 0;
    if (batch < 1) { set_error("forward_workspace_bytes: batch=%d", batch); return 0; }
    const Tuning t = tuning();
    carve_fwd(p, g, batch, nullptr, in_form(p, g, t), cond_composed(p, frames, t), w, f);
    return f.total * sizeof(float);
}

int ctts_waveglow_flow_forward_f32(const ctts_waveglow_config* cfg, const void* packed, const void* packed_fwd, int32_t flow,
                                   float* z, const float* wave, const float* h_all, float* log_s, double* sum_log_s,
                                   int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    WnCall c;
    int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    CTTS_CHECK_ARG(flow >= 0 && flow < c.p.c.n_flows, "waveglow_flow_forward: flow %d", flow);
    CTTS_CHECK_ARG(packed && packed_fwd && z && h_all && workspace && batch >= 1, "waveglow_flow_forward: bad argument");
    CTTS_CHECK_ARG(wave == nullptr || flow == 0, "waveglow_flow_forward: only flow 0 reads the waveform (flow %d)", flow);
    if ((rc = c.take_workspace("waveglow_flow_forward", workspace, workspace_bytes, true))) return rc;
    c.audio = z; c.h_all = h_all;
    rc = c.run_flow_forward(static_cast<const float*>(packed_fwd), flow, wave, log_s, (long long)c.p.fd[flow].n_half * c.g.L);
    if (rc || !sum_log_s) return rc;
    const FwdSums& f = c.sums;
    return launch_sum_partials(f.ls_part + (size_t)flow * f.nblk_ls, (long long)c.p.c.n_flows * f.nblk_ls, 0, f.nblk_ls, sum_log_s, 1, 1,
                               batch, c.s);
}

int ctts_waveglow_forward_spk_f32(const ctts_waveglow_config* cfg, const void* packed, const void* packed_fwd, const float* mel,
                                  const float* audio, const int64_t* speaker_ids, float* z, float* log_s, double* sums,
                                  int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    WnCall c;
    int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    const Plan& p = c.p;
    CTTS_CHECK_ARG(packed && packed_fwd && mel && audio && z && workspace && batch >= 1, "forward: bad argument");
    CTTS_CHECK_ARG(p.S == 0 || speaker_ids != nullptr, "multispeaker model (speaker_embed_dim=%d) needs speaker ids (glow.py:193)",
                   p.c.speaker_embed_dim);
    if ((rc = c.take_workspace("forward", workspace, workspace_bytes, true))) return rc;
    c.audio = z;
    // glow.py:276-282 with audio.size(1) == frames * hop keeps the columns infer's trim keeps: the same conditioning
    if ((rc = c.conditioning(mel, speaker_ids))) return rc;
    const int L = c.g.L, S = fwd_log_s_rows(p, p.c.n_flows);
    for (int k = 0; k < p.c.n_flows; ++k) {
        float* ls = log_s ? log_s + (size_t)fwd_log_s_rows(p, k) * L : nullptr;
        rc = c.run_flow_forward(static_cast<const float*>(packed_fwd), k, k == 0 ? audio : nullptr, ls, (long long)S * L);
        if (rc) return rc;
    }
    if (!sums) return CTTS_OK;
    const FwdSums& f = c.sums;
    rc = launch_sum_partials(f.ls_part, (long long)p.c.n_flows * f.nblk_ls, f.nblk_ls, f.nblk_ls, sums, p.c.n_flows + 1, p.c.n_flows,
                             batch, c.s);
    if (rc) return rc;
    rc = launch_sumsq_partials(z, f.z_part, batch, (long long)p.c.n_group * L, f.nblk_z, c.s);
    if (rc) return rc;
    return launch_sum_partials(f.z_part, f.nblk_z, 0, f.nblk_z, sums + p.c.n_flows, p.c.n_flows + 1, 1, batch, c.s);
}

int ctts_waveglow_infer_f32(const ctts_waveglow_config* cfg, const void* packed, const float* mel,
                            const float* z_scaled, float* wave, int32_t batch, int32_t frames, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return ctts_waveglow_infer_spk_f32(cfg, packed, mel, z_scaled, nullptr, wave, batch, frames, workspace,
                                       workspace_bytes, stream);
}

int ctts_waveglow_infer_spk_f32(const ctts_waveglow_config* cfg, const void* packed, const float* mel,
                                const float* z_scaled, const int64_t* speaker_ids, float* wave, int32_t batch,
                                int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return ctts_waveglow_infer_spk_f32_opt(cfg, packed, mel, z_scaled, speaker_ids, wave, batch, frames, workspace, workspace_bytes, 0,
                                           stream);
}

int ctts_waveglow_infer_spk_f32_opt(const ctts_waveglow_config* cfg, const void* packed, const float* mel,
                                    const float* z_scaled, const int64_t* speaker_ids, float* wave, int32_t batch,
                                    int32_t frames, void* workspace, size_t workspace_bytes, int32_t options, void* stream) {
    WnCall c;
    int rc = c.begin(cfg, packed, batch, frames, stream, options); if (rc) return rc;
    CTTS_CHECK_ARG(packed && mel && z_scaled && wave && workspace && batch >= 1, "infer: bad argument");
    if ((rc = c.take_workspace("infer", workspace, workspace_bytes, false))) return rc;
    CTTS_CHECK_HIP(hipMemcpyAsync(c.audio, z_scaled, (size_t)batch * c.p.c.n_group * c.g.L * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    if ((rc = c.conditioning(mel, speaker_ids))) return rc;
    for (int k = c.p.c.n_flows - 1; k >= 0; --k)
        if ((rc = c.run_flow(k, k == 0 ? wave : nullptr, nullptr))) return rc;
    return CTTS_OK;
}


int ctts_last_gemm_loop(void) { return last_gemm_loop(); }
int ctts_last_winograd_f43_width(void) { return last_wn_winograd_f43_width(); }
int ctts_tuning_reload(void) { reload_tuning(); return CTTS_OK; }
// the knobs beyond the 32 bits of ctts_tuning_flags: bit 0 here is bit 32 there
int ctts_tuning_flags_ext(void) {
    const Tuning t = tuning();
    return (t.f32_winograd_f63_min >= 0 ? 1 : 0) | (t.f32_winograd_no_f63 ? 2 : 0);
}
int ctts_tuning_flags(void) {
    const Tuning t = tuning();
    return (t.f32_no_glds ? 1 : 0) | (t.no_xcd_pair ? 2 : 0) | (t.bf16_no_wide ? 8 : 0) | (t.bf16_no_pp ? 16 : 0) |
           (t.wf_no_fuse ? 128 : 0) | (t.taco_no_fuse ? 256 : 0) | (t.f32_no_small ? 512 : 0) | (t.f32_force_small ? 1024 : 0) |
           (t.f32_no_splitk ? 2048 : 0) | (t.wf_no_vec_interp ? 4096 : 0) | (t.f32_no_defer_skip ? 8192 : 0) |
           (t.wf_no_region_split ? 16384 : 0) | (t.wf_no_row_queue ? 32768 : 0) | (t.wf_row_queue_min >= 0 ? 65536 : 0) |
           (t.wf_inject_abort ? 131072 : 0) | (t.wf_queue_debug ? 262144 : 0) | (t.f32_no_round_split ? 524288 : 0) |
           (t.bf16_ps ? (1 << 20) : 0) | (t.bf16_no_ps ? (1 << 21) : 0) | (t.taco_poll_delay_set ? (1 << 23) : 0) |
           (t.taco_valu ? (1 << 24) : 0) | (t.up_no_mfma ? (1 << 25) : 0) | (t.f32_no_wn_fold ? (1 << 26) : 0) |
           (t.taco_bg_no_pipe ? (1 << 27) : 0) | (t.f32_no_winograd ? (1 << 28) : 0) | (t.f32_winograd_min >= 0 ? (1 << 29) : 0) |
           (t.f32_winograd_plain ? (1 << 30) : 0) | (t.f32_winograd_fused_min >= 0 ? 4 : 0) | (t.f32_winograd_no_fused ? 32 : 0) |
           (t.f32_winograd_f43_min >= 0 ? (1 << 6) : 0) | (t.f32_winograd_no_f43 ? (1 << 22) : 0) |
           (t.wf_fwd_rowwise ? (int)(1u << 31) : 0);
}

int ctts_profile_create(void** handle) {
    CTTS_CHECK_ARG(handle, "profile_create: NULL");
    *handle = new Prof();
    return CTTS_OK;
}

int ctts_profile_bind(void* handle) {
    t_prof = static_cast<Prof*>(handle);
    return CTTS_OK;
}

int ctts_profile_collect(void* handle, int32_t which, int64_t* launches, double* total_ms) {
    Prof* pr = static_cast<Prof*>(handle);
    CTTS_CHECK_ARG(pr && which >= 0 && which < CTTS_PROF_N && launches && total_ms, "profile_collect: bad argument");
    std::lock_guard<std::mutex> lk(pr->mu);
    double tot = 0.0;
    int64_t n = 0;
    for (auto& e : pr->ev[which]) {
        float ms = 0.f;
        CTTS_CHECK_HIP(hipEventSynchronize(e.second));
        CTTS_CHECK_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        tot += ms; ++n;
        pr->pool.push_back(e);
    }
    pr->ev[which].clear();
    *launches = n; *total_ms = tot;
    return CTTS_OK;
}

int ctts_profile_destroy(void* handle) {
    Prof* pr = static_cast<Prof*>(handle);
    if (!pr) return CTTS_OK;
    if (t_prof == pr) t_prof = nullptr;
    {
        std::lock_guard<std::mutex> lk(pr->mu);
        for (int w = 0; w < CTTS_PROF_N; ++w)
            for (auto& e : pr->ev[w]) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        for (auto& e : pr->pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    }
    delete pr;
    return CTTS_OK;
}

// ---- bf16 MFMA variants: P = 1 (bf16 storage, config 3) and P = 3 (split bf16: every operand is a hi + lo pair of
// bf16 planes, every contraction three bf16 MFMA products hi*hi + lo*hi + hi*lo with fp32 accumulation - inputs carry
// 16 mantissa bits instead of 8, at a third of the bf16 rate) ------------------------------------------------------
static size_t packed_bf16_bytes_impl(const ctts_waveglow_config* cfg, int P) {   // (the same for f16)
    Plan p; BfPlan q;
    if (make_plan(cfg, p)) return 0;
    if (p.C % BGEMM_KC != 0 || p.H % BGEMM_KC != 0) { set_error("bf16: channels must be multiples of 32"); return 0; }
    make_bf_plan(p, q, P);
    return q.total * sizeof(bf16_t);
}

static int pack_flow_bf16_impl(const ctts_waveglow_config* cfg, int32_t k, const ctts_waveglow_flow_weights* w,
                               void* packed_bf16, void* stream, int P, int f16 = 0) {
    Plan p; BfPlan q;
    int rc = make_plan(cfg, p); if (rc) return rc;
    CTTS_CHECK_ARG(k >= 0 && k < p.c.n_flows && w && packed_bf16, "pack_flow_bf16: bad argument");
    CTTS_CHECK_ARG(p.C % BGEMM_KC == 0 && p.H % BGEMM_KC == 0, "pack_flow_bf16: channels must be multiples of 32");
    CTTS_CHECK_ARG(!f16 || P == 1, "pack_flow: the split form exists for bf16 only");
    make_bf_plan(p, q, P, f16);
    CTTS_CHECK_ARG(q.nch_in <= BGEMM_MAX_CHUNKS && BF_SKIP_GROUP * q.nch_rs <= BGEMM_MAX_CHUNKS,
                   "pack_flow_bf16: K of %d chunks exceeds the chunk table", q.nch_in);
    hipStream_t s = as_stream(stream);
    bf16_t* bb = static_cast<bf16_t*>(packed_bf16);
    const int C = p.C, H = p.H, ks = p.c.kernel_size;
    CTTS_CHECK_ARG(w->cond_w[0] && w->cond_w[1] && p.K0 % BGEMM_KC == 0, "pack_flow_bf16: cond weights / n_mel*n_group %% 32");
    const int sdim = p.c.speaker_embed_dim;
    bf16_t* c0 = bb + q.cond0_A + (size_t)k * q.nch_c0 * BGEMM_KC * BGEMM_BM;
    bf16_t* c1 = bb + q.cond1_A + (size_t)k * q.nch_c1 * BGEMM_KC * BGEMM_BM;
    // product pi of an operand pair uses W_hi for pi = 0, 1 (against x_hi, x_lo) and W_lo for pi = 2 (against x_hi)
    for (int pi = 0; pi < P; ++pi) {
        const int part = pi == 2;
        if ((rc = launch_pack_a_bf16(c0, w->cond_w[0], 1, q.nch_c0, pi * p.K0, p.K0, BGEMM_EPI_SPLIT, C, H, 0, p.K0 + sdim, 1,
                                     s, 1, 0, part, q.f16))) return rc;
        if (sdim && (rc = launch_pack_a_bf16(c0, w->cond_w[0] + p.K0, 1, q.nch_c0, P * p.K0 + pi * p.S, sdim, BGEMM_EPI_SPLIT,
                                             C, H, 0, p.K0 + sdim, 1, s, 1, 0, part, q.f16))) return rc;
        if ((rc = launch_pack_a_bf16(c1, w->cond_w[1], 1, q.nch_c1, pi * H, H, BGEMM_EPI_SPLIT, C, H, 0, H, 1, s, 1, 0,
                                     part, q.f16))) return rc;
    }
    for (int i = 0; i < p.c.n_layers; ++i) {
        CTTS_CHECK_ARG(w->in_w[i] && w->rs_w[i] && w->cond_w[2] && w->rs_b[i], "pack_flow_bf16: NULL layer %d weights", i);
        // res_skip_layers.i is [2C][C] = {res rows, skip rows} for i < last, [C][C] = skip rows for the last layer
        const bool last = i == p.c.n_layers - 1;
        const int gi = i / BF_SKIP_GROUP, j = i % BF_SKIP_GROUP;
        for (int pi = 0; pi < P; ++pi) {
            const int part = pi == 2;
            // in-layer K = [per 32-channel slab: (tap, product) round-robin] then [cond products]
            for (int t = 0; t < ks; ++t)
                if ((rc = launch_pack_a_bf16(bb + q.in_A[k][i], w->in_w[i] + t, p.mb_in, q.nch_in, 0, C, BGEMM_EPI_GATE, C,
                                             2 * C, 0, (long long)C * ks, ks, s, ks * P, t * P + pi, part, q.f16))) return rc;
            if ((rc = launch_pack_a_bf16(bb + q.in_A[k][i], w->cond_w[2], p.mb_in, q.nch_in, ks * P * C + pi * H, H,
                                         BGEMM_EPI_GATE, C, 2 * C, (long long)2 * C * i, H, 1, s, 1, 0, part, q.f16))) return rc;
            if (!last && (rc = launch_pack_a_bf16(bb + q.rs_A[k][i], w->rs_w[i], q.mb_c, q.nch_rs, pi * C, C, BGEMM_EPI_SPLIT,
                                                  C, C, 0, C, 1, s, 1, 0, part, q.f16))) return rc;
            if ((rc = launch_pack_a_bf16(bb + q.skip_A[k][gi], w->rs_w[i], q.mb_c, q.group_layers(gi, p.c.n_layers) * q.nch_rs,
                                         (j * P + pi) * C, C, BGEMM_EPI_SPLIT, C, C, last ? 0 : C, C, 1, s, 1, 0,
                                         part, q.f16))) return rc;
        }
        hipLaunchKernelGGL(skip_bias_kernel, dim3((2 * q.mb_c * BGEMM_BM + 255) / 256), dim3(256), 0, s,
                           reinterpret_cast<float*>(bb + q.skip_b[k]), w->rs_b[i] + (last ? 0 : C), C,
                           2 * q.mb_c * BGEMM_BM, i == 0 ? 1 : 0);
        CTTS_CHECK_LAUNCH("skip_bias");
    }
    return CTTS_OK;
}

static size_t workspace_bf16_bytes_impl(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames, int P) {
    Plan p; Geom g; BfWs w;
    if (make_plan(cfg, p) || make_geom(p, frames, g) || batch < 1) return 0;
    carve_bf(p, g, batch, nullptr, w, P);
    return w.total_bytes;
}

static int infer_bf16_impl(const ctts_waveglow_config* cfg, const void* packed, const void* packed_bf16, const float* mel,
                           const float* z_scaled, const int64_t* speaker_ids, float* wave, int32_t batch, int32_t frames,
                           void* workspace, size_t workspace_bytes, void* stream, int P, int f16 = 0) {
    WnCall c; BfWs w; BfPlan q;
    int rc = c.begin(cfg, packed, batch, frames, stream); if (rc) return rc;
    const Plan& p = c.p;
    const Geom& g = c.g;
    CTTS_CHECK_ARG(packed && packed_bf16 && mel && z_scaled && wave && workspace && batch >= 1, "infer_bf16: bad argument");
    CTTS_CHECK_ARG(p.C % BGEMM_KC == 0 && p.C <= 512, "infer_bf16: n_channels=%d (multiple of 32, <= 512)", p.C);
    CTTS_CHECK_ARG(p.c.n_group <= 8, "infer_bf16: n_group=%d (the reduced-precision flow boundaries hold <= 8 channels; fp32 takes 16)", p.c.n_group);
    make_bf_plan(p, q, P, f16);
    carve_bf(p, g, batch, static_cast<char*>(workspace), w, P);
    if ((rc = workspace_fits("infer_bf16", workspace_bytes, w.total_bytes))) return rc;
    hipStream_t s = c.s;
    const float* blob = c.blob;
    const bf16_t* bblob = static_cast<const bf16_t*>(packed_bf16);
    CTTS_CHECK_HIP(hipMemcpyAsync(w.audio, z_scaled, (size_t)batch * p.c.n_group * g.L * sizeof(float),
                                  hipMemcpyDeviceToDevice, s));
    if ((rc = c.upsample(mel, w.spect))) return rc;
    // cond layers 0 / 1 for all flows on bf16 MFMA: spect -> bf16 K8, then two flow-batched GEMMs whose
    // epilogues write the conditioning hidden directly in bf16 K8
    hipLaunchKernelGGL(cvt_f32_to_k8_kernel, dim3((g.ld + 255) / 256, p.K0 / 8, batch), dim3(256), 0, s, w.spect,
                       w.spect_bf, p.K0, g.ld, w.spect_lo, q.f16);
    CTTS_CHECK_LAUNCH("cvt_f32_to_k8");
    if (p.S) {
        if ((rc = c.speaker_rows(speaker_ids, w.spk))) return rc;
        hipLaunchKernelGGL(cvt_f32_to_k8_kernel, dim3((g.ld + 255) / 256, p.c.n_flows * p.S / 8, batch), dim3(256), 0, s,
                           w.spk, w.spk_bf, p.c.n_flows * p.S, g.ld, w.spk_lo, q.f16);
        CTTS_CHECK_LAUNCH("cvt_f32_to_k8(speaker rows)");
    }
    {
        const long long hstride = (long long)p.c.n_flows * p.H * g.ld;
        BGemmArgs a{};
        a.f16 = q.f16;
        a.ld = g.ld; a.pad = g.pad; a.L = g.L; a.ntiles = g.ntiles; a.batch = batch;
        a.A = bblob + q.cond0_A; a.bias = blob + p.cond0_b;
        a.nch_total = q.nch_c0; a.MB = p.c.n_flows; a.M = p.c.n_flows * BGEMM_BM;
        int ns = push_segs(a, 0, P, w.spect_bf, w.spect_lo, (long long)p.K0 * g.ld, p.K0 / BGEMM_KC, 0, 0);
        if (p.S) ns = push_segs(a, ns, P, w.spk_bf, w.spk_lo, (long long)p.c.n_flows * p.S * g.ld, p.S / BGEMM_KC, 0, p.S);
        a.nseg = ns;
        a.dst0 = w.h_tmp_bf; a.dst0_bstride = hstride; a.acc0 = 0;
        a.dst1 = w.h_tmp_bf; a.dst1_bstride = hstride; a.acc1 = 0;
        a.split = a.M; a.lo_off = w.h_lo;
        if ((rc = launch_gemm_bf16(BGEMM_EPI_SPLIT, a, s))) return rc;
        a.A = bblob + q.cond1_A; a.bias = blob + p.cond1_b;
        a.nch_total = q.nch_c1;
        a.nseg = push_segs(a, 0, P, w.h_tmp_bf, w.h_lo, hstride, p.H / BGEMM_KC, 0, BGEMM_BM);
        a.dst0 = w.h_bf; a.dst1 = w.h_bf;
        if ((rc = launch_gemm_bf16(BGEMM_EPI_SPLIT, a, s))) return rc;
    }
    for (int k = p.c.n_flows - 1; k >= 0; --k) {
        rc = run_wn_stack_bf16(p, q, g, blob, bblob, k, w, batch, s);
        if (rc) return rc;
        const auto& f = p.fl[k];
        const auto& d = p.fd[k];
        float* wv = k == 0 ? wave : nullptr;
        dim3 tgrid((g.L + 255) / 256, batch);
#define CTTS_BTAIL1(HH, FF)                                                                                           \
        hipLaunchKernelGGL((flow_tail_bf16_kernel<HH, FF>), tgrid, dim3(256), 0, s, w.out, w.audio, wv, blob + f.end_w,   \
                           blob + f.end_b, blob + f.winv, p.C, p.c.n_group, d.ch_off, g.L, g.ld, g.pad, w.x_lo)
#define CTTS_BTAIL(HH)                                                                                            \
    case HH:                                                                                                      \
        if (q.f16) CTTS_BTAIL1(HH, 2); else if (w.x_lo) CTTS_BTAIL1(HH, 1); else CTTS_BTAIL1(HH, 0);              \
        break;
        switch (d.n_half) {
            CTTS_BTAIL(1) CTTS_BTAIL(2) CTTS_BTAIL(3) CTTS_BTAIL(4)
            default: set_error("flow_tail_bf16: n_half=%d", d.n_half); return CTTS_E_ARG;
        }
#undef CTTS_BTAIL
#undef CTTS_BTAIL1
        CTTS_CHECK_LAUNCH("flow_tail_bf16");
    }
    return CTTS_OK;
}

size_t ctts_waveglow_packed_bf16_bytes(const ctts_waveglow_config* cfg) { return packed_bf16_bytes_impl(cfg, 1); }
int ctts_waveglow_pack_flow_bf16(const ctts_waveglow_config* cfg, int32_t k, const ctts_waveglow_flow_weights* w,
                                 void* packed_bf16, void* stream) {
    return pack_flow_bf16_impl(cfg, k, w, packed_bf16, stream, 1);
}
size_t ctts_waveglow_workspace_bf16_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames) {
    return workspace_bf16_bytes_impl(cfg, batch, frames, 1);
}
int ctts_waveglow_infer_bf16(const ctts_waveglow_config* cfg, const void* packed, const void* packed_bf16,
                             const float* mel, const float* z_scaled, float* wave, int32_t batch, int32_t frames,
                             void* workspace, size_t workspace_bytes, void* stream) {
    return infer_bf16_impl(cfg, packed, packed_bf16, mel, z_scaled, nullptr, wave, batch, frames, workspace, workspace_bytes,
                           stream, 1);
}
int ctts_waveglow_infer_spk_bf16(const ctts_waveglow_config* cfg, const void* packed, const void* packed_bf16,
                                 const float* mel, const float* z_scaled, const int64_t* speaker_ids, float* wave,
                                 int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return infer_bf16_impl(cfg, packed, packed_bf16, mel, z_scaled, speaker_ids, wave, batch, frames, workspace,
                           workspace_bytes, stream, 1);
}

// IEEE-half variant: the layouts, sizes and kernels of the bf16 variant with half storage and v_mfma_f32_32x32x16_f16
int ctts_waveglow_pack_flow_f16(const ctts_waveglow_config* cfg, int32_t k, const ctts_waveglow_flow_weights* w,
                                void* packed_f16, void* stream) {
    return pack_flow_bf16_impl(cfg, k, w, packed_f16, stream, 1, 1);
}
int ctts_waveglow_infer_spk_f16(const ctts_waveglow_config* cfg, const void* packed, const void* packed_f16,
                                const float* mel, const float* z_scaled, const int64_t* speaker_ids, float* wave,
                                int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return infer_bf16_impl(cfg, packed, packed_f16, mel, z_scaled, speaker_ids, wave, batch, frames, workspace,
                           workspace_bytes, stream, 1, 1);
}

size_t ctts_waveglow_packed_bf16x3_bytes(const ctts_waveglow_config* cfg) { return packed_bf16_bytes_impl(cfg, 3); }
int ctts_waveglow_pack_flow_bf16x3(const ctts_waveglow_config* cfg, int32_t k, const ctts_waveglow_flow_weights* w,
                                   void* packed_bf16x3, void* stream) {
    return pack_flow_bf16_impl(cfg, k, w, packed_bf16x3, stream, 3);
}
size_t ctts_waveglow_workspace_bf16x3_bytes(const ctts_waveglow_config* cfg, int32_t batch, int32_t frames) {
    return workspace_bf16_bytes_impl(cfg, batch, frames, 3);
}
int ctts_waveglow_infer_spk_bf16x3(const ctts_waveglow_config* cfg, const void* packed, const void* packed_bf16x3,
                                   const float* mel, const float* z_scaled, const int64_t* speaker_ids, float* wave,
                                   int32_t batch, int32_t frames, void* workspace, size_t workspace_bytes, void* stream) {
    return infer_bf16_impl(cfg, packed, packed_bf16x3, mel, z_scaled, speaker_ids, wave, batch, frames, workspace,
                           workspace_bytes, stream, 3);
}

}  // extern "C"
