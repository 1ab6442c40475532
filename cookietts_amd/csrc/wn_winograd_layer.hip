// One launch per Winograd F(2,3) in-layer step of the fp32 WaveGlow (see wn_winograd_layer.h for the contract).
//
// Workgroup = 256 threads = 4 waves (2 x 2) on 128 packed rows x BN = 64 NT pair columns of one batch item; a wave holds the 32 tanh
// and the 32 sigmoid rows of 32 channels x 32 NT columns in TWO accumulator sets S and D (2 x 32 NT VGPRs).  The main loop is the
// conv-GEMM's (gemm_f32.hip): three LDS stages filled by global_load_lds two chunks ahead, one DMA piece per k-step behind that
// k-step's MFMAs, counted vmcnt + raw s_barrier, fragments of k-step ks + 1 read while ks runs - run over ONE stream of
// 2 n1 + 2 n2 chunks (n1 = C / 16, n2 = (C + H) / 16):
//   [0, n1)            S += G2 . V2
//   [n1, 2 n1)         D += G3 . V3             then (S, D) <- (S + D, S - D)
//   [2 n1, 2 n1 + n2)  S += [W0 | C_i] . [V1; h(t_e)]    then act[t_e] = gate(S + b)
//   [.., 2 n1 + 2 n2)  D += [-W2 | C_i] . [V4; h(t_o)]   then act[t_o] = gate(D + b)
// The DMA cursor runs through the even phase's epilogue (gfx9 counts stores on vmcnt too: the wait behind the next chunk then also
// drains them, which is merely conservative - loads return in order among themselves).
// A chunk -> (A address, B address) table is built once per workgroup.  The weights are read where the lean form's launches read
// them: a GATE-packed panel holds this workgroup's 128 rows as one half of every 256-row k-row, a SPLIT-packed one (dense row order)
// as two 64-row runs of two M-blocks - the lanes carry that, no second copy of the weights exists.
// NT = 2 (128 columns) and NT = 1 (64 columns, for small grids and the tiles beyond the last whole round) sum every column's
// products in the same order with the same instruction: bit-identical.
//
// F43 = 1 is the F(4,3) form on the same main-loop body (NT = 1 only): 64 QUAD columns = 256 natural columns, FOUR accumulator sets
// (the 128 VGPRs S and D cost at NT = 2) and one stream of 4 n1 + 2 n2 + 2 nh chunks (nh = H / 16):
//   [0, 4 n1)          X_j += U_(j+1) . V_(j+1), j = 0..3
//                      then a = X0 + X1, b = X0 - X1, c = X2 + X3, e = X2 - X3, (X0..X3) <- (a + c, b + 2 e, a + 4 c, b + 8 e)
//   [.., + n2)         X0 += [U0 | C_i] . [V0; h(t_0)]   then act[t_0] = gate(X0 + b)
//   [.., + nh)         X1 += C_i . h(t_1)                then act[t_1]      (the cond chunks of the [U0 | C_i] panel: no third C_i)
//   [.., + nh)         X2 += C_i . h(t_2)                then act[t_2]
//   [.., + n2)         X3 += [U5 | C_i] . [V5; h(t_3)]   then act[t_3]
// (interpolation points 0, +-1, +-2, inf: the output-side multipliers 1, 2, 4, 8 are exact scalings).
// The F(4,3) form also runs with KD = 2: a stage holds two consecutive chunks (every phase is an even number of chunks), 16 k-step
// regions and 32 NT MFMAs per wave between two barriers, and with NT = 2 (128 quad columns, 256 accumulator registers pinned to the
// accumulator half of the file, one workgroup per CU).  Same products in the same order per accumulator element: bit-identical.
//
// F43 = 2 is the F(6,3) form on that main-loop body (NT = 1, KD = 2 only): 64 HEX columns = 384 natural columns, SIX accumulator sets
// (192 VGPRs; 256 in all, no scratch, two workgroups per CU: profiles/r34_02_f63_resource_usage.txt) and one stream of
// 6 n1 + 2 n2 + 4 nh chunks (C = 512, H = 256: 352 for 384 columns where F(4,3) runs 256 for 256):
//   [0, 6 n1)          X_j += U_(j+1) . V_(j+1), j = 0..5
//                      then a = X0 + X1, b = X0 - X1, c = X2 + X3, e = X2 - X3, f = X4 + X5, g = X4 - X5,
//                      (X0..X5) <- (a + c + f, b + 2 e + g / 2, a + 4 c + f / 4, b + 8 e + g / 8, a + 16 c + f / 16, b + 32 e + g / 32)
//   [.., + n2)         X0 += [U0 | C_i] . [V0; h(t_0)]   then act[t_0] = gate(X0 + b)
//   4 x [.., + nh)     X_k += C_i . h(t_k), k = 1..4     then act[t_k]      (the cond chunks of the [U0 | C_i] panel)
//   [.., + n2)         X5 += [U7 | C_i] . [V7; h(t_5)]   then act[t_5]
// (interpolation points 0, +-1, +-2, +-1/2, inf: every output-side multiplier is a power of two).
#include "wn_winograd_layer.h"
#include "tuning.h"

namespace ctts {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned wg_u32x4 __attribute__((ext_vector_type(4)));

namespace {

// the GATE epilogue's gate math (gemm_f32.hip): exp via v_exp_f32, reciprocal via v_rcp_f32
__device__ __forceinline__ float wg_sigmoid(float u) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f));
}
__device__ __forceinline__ float wg_tanh(float u) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * 2.8853900817779268f));
}

}  // namespace

template <int NT, int F43, int KD, int TP>
__global__ __launch_bounds__(256, (F43 && NT == 2) ? 1 : 2) void wn_winograd_layer_f32_kernel(const WnWinogradLayerArgs a) {
    static_assert(KD == 1 || (KD == 2 && F43 && TP), "two chunks per stage: the F(4,3) form (its phases are whole stages, see the launcher)");
    static_assert(F43 <= 1 || (NT == 1 && KD == 2), "the F(6,3) form: 64 hex columns, two chunks per stage");
    constexpr int NI = 2 + 2 * F43;                       // interior products = accumulator sets = natural columns per packed column
    constexpr int BN = 64 * NT;
    constexpr int A_ST = GEMM_KC * 128;                   // floats of a chunk's A part
    constexpr int CST = A_ST + GEMM_KC * BN;              // floats per chunk
    constexpr int STG = KD * CST;                         // floats per stage: KD consecutive chunks of the stream
    constexpr int NP = 2 + NT;                            // DMA pieces per wave and chunk
    constexpr int TAB = 3 * STG;                          // chunk table: {A address, B address} = 4 dwords per chunk
    constexpr int BIAS = TAB + 4 * WNWG_MAX_CHUNKS;
    constexpr int UPR = BN / 4;                           // 16-byte units per k-row of the B stage
    constexpr int RPP = 64 / UPR;                         // k-rows per B piece (2 or 4)
    __shared__ __attribute__((aligned(16))) float lds[BIAS + 128];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lhi = lane >> 5;

    // block -> (channel block, column tile, batch item).  Dispatch places block id on XCD id % 8: an XCD runs all the channel
    // blocks of a column tile back to back, so the tile's B rows are fetched into one L2 and every XCD streams the same weights
    const int ncb = a.C >> 6;
    const int jx = blockIdx.x >> 3;
    const int cb = jx % ncb;
    const int gt = (jx / ncb) * 8 + (blockIdx.x & 7);
    if (gt >= a.kt_total) return;                         // whole workgroup: the grid is rounded up to 8 tiles
    const int b = a.b0 + gt / a.kt;
    const int n0 = a.col0 + (gt % a.kt) * BN;             // first pair column (of the batch item)

    const int n1 = a.C / GEMM_KC, n2 = (a.C + a.H) / GEMM_KC, nh = a.H / GEMM_KC;
    // the phases behind the interior products: the first and the last carry an end product (n2 chunks), the others cond rows alone
    const int c_e = NI * n1;
    int ps[NI + 1];
    ps[0] = c_e;
#pragma unroll
    for (int k = 0; k < NI; ++k) ps[k + 1] = ps[k] + (k == 0 || k == NI - 1 ? n2 : nh);
    const int nch = ps[NI];

    // SPLIT-packed panels: this block's tanh rows are dense rows 64 cb .., its sigmoid rows dense rows C + 64 cb ..
    const int mb_t = (64 * cb) >> 8, loc_t = (64 * cb) & 255;
    const int mb_s = (a.C + 64 * cb) >> 8, loc_s = (a.C + 64 * cb) & 255;
    {
        uint4* tab = reinterpret_cast<uint4*>(lds + TAB);
        for (int c = t; c < nch; c += 256) {
            const float *ap, *bp;
            if (c < c_e) {
                const int ph = F43 ? c / n1 : (int)(c >= n1), loc = c - ph * n1;
                ap = (ph == 0 ? a.A_T2 : ph == 1 ? a.A_T3 : ph == 2 ? a.A_T4 : ph == 3 ? a.A_T5 : ph == 4 ? a.A_T6 : a.A_T7) +
                     ((size_t)mb_t * n1 + loc) * (GEMM_KC * 256) + loc_t;
                bp = a.V + (1 + ph) * a.vplane + ((size_t)b * a.C + (size_t)loc * GEMM_KC) * a.ldp + n0;
            } else {
                int ph = 0;
#pragma unroll
                for (int k = 1; k < NI; ++k) ph += c >= ps[k];
                const bool last = ph == NI - 1;
                const int loc = c - ps[ph] + (ph == 0 || last ? 0 : n1);      // k-chunk of the GATE panel (a middle phase: its cond chunks)
                ap = (last ? a.A_o : a.A_e) + ((size_t)(cb >> 1) * n2 + loc) * (GEMM_KC * 256) + (cb & 1) * 128;
                if (loc < n1) bp = a.V + (last ? NI + 1 : 0) * a.vplane + ((size_t)b * a.C + (size_t)loc * GEMM_KC) * a.ldp + n0;
                else if (a.in_place) bp = a.h2 + (size_t)b * a.h_bstride + (size_t)(loc - n1) * GEMM_KC * a.ld;   // the lanes carry pad and column
                else bp = a.Hc + ph * a.hplane + ((size_t)b * a.H + (size_t)(loc - n1) * GEMM_KC) * a.ldp + n0;
            }
            const unsigned long long ua = reinterpret_cast<unsigned long long>(ap), ub = reinterpret_cast<unsigned long long>(bp);
            tab[c] = make_uint4((unsigned)ua, (unsigned)(ua >> 32), (unsigned)ub, (unsigned)(ub >> 32));
        }
        if (t < 128) lds[BIAS + t] = a.bias[cb * 128 + t];
    }

    // 32-bit lane byte offsets of the DMA pieces.  A piece j of wave w = k-rows 2 (w + 4 j), + 1 of the stage (256 floats, lane order)
    unsigned offa_g[2], offa_s[2], offb[NT], offb_m[NI][NT];
    {
        const int col = (lane & 31) * 4;
        const long long delta = ((long long)(mb_s - mb_t) * n1) * (GEMM_KC * 256) + (loc_s - loc_t);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int krow = 2 * (wave + 4 * j) + (lane >> 5);
            offa_g[j] = (unsigned)((krow * 256 + col) * 4);
            offa_s[j] = (unsigned)((krow * 256 + (col < 64 ? (long long)col : col - 64 + delta)) * 4);
        }
        const int bcol = (lane % UPR) * 4;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int krow = (wave + 4 * j) * RPP + lane / UPR;
            offb[j] = (unsigned)(((size_t)krow * a.ldp + bcol) * 4);
#pragma unroll
            for (int k = 0; k < NI; ++k) offb_m[k][j] = 0;
            if (a.in_place) {
                // the lane's unit starts at packed column q and is read at the natural column of q: four consecutive, 16-byte aligned
                // columns (d % 4 == 0), clamped to the row's last aligned unit (those outputs are dropped by the L / Lp tests)
                const int q = n0 + bcol;
                const int te = (q / a.d) * (NI * a.d) + q % a.d;
                const int lim = (a.ld - a.pad - 4) & ~3;
#pragma unroll
                for (int k = 0; k < NI; ++k) offb_m[k][j] = (unsigned)(((size_t)krow * a.ld + a.pad + min(te + k * a.d, lim)) * 4);
            }
        }
    }
    int m_lo[NI];                                         // mapped cond chunks of phase k: [m_lo[k], ps[k + 1])
#pragma unroll
    for (int k = 0; k < NI; ++k) m_lo[k] = a.in_place ? ps[k] + (k == 0 || k == NI - 1 ? n1 : 0) : 0x7fffffff;

    wg_f32x16 X[NI][2][NT];
#pragma unroll
    for (int k = 0; k < NI; ++k)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) X[k][i][j][r] = 0.0f;
    __syncthreads();                                      // table and bias visible

    typedef __attribute__((address_space(3))) float* lds_fptr;
    typedef const __attribute__((address_space(1))) float* gfloat_ptr;
    typedef const __attribute__((address_space(1))) char* gbyte_ptr;
    const wg_u32x4* ctab = reinterpret_cast<const wg_u32x4*>(lds + TAB);
    // Every DMA address is a wave-uniform 64-bit base (SGPR pair) + a 32-bit lane offset laundered through an empty asm, so that
    // the compiler keeps the global_load_lds_dwordx4 v, s[a:b] form (gemm_f32.hip, CTTS_GLDS_PIECE)
    // TP = 1: the table entries of a stage are fetched one iteration AHEAD by an asm read the compiler does not see, and waited for
    // in front of the barrier.  Read as a plain load (TP = 0), the table makes the compiler drain EVERY DMA in flight first - it
    // cannot tell the table from the stages the DMA writes - i.e. an s_waitcnt vmcnt(0) at the head of every chunk, which gives the
    // two-chunks-ahead staging away.  (LDS returns in order, so an uncounted read only makes the compiler's own counted waits
    // conservative; nothing touches tn_ between its read and its wait.)
    wg_u32x4 tn_[KD];
    const unsigned tab_lds = (unsigned)reinterpret_cast<uintptr_t>((lds_fptr)(lds + TAB));
#define WNWG_TAB_ISSUE(c)                                                                                   \
    _Pragma("unroll") for (int j = 0; j < KD; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(tn_[j]) : "v"(tab_lds + 16u * (unsigned)((c) + j)));
#define WNWG_TAB_WAIT()                                                                                     \
    do {                                                                                                    \
        if constexpr (KD == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tn_[0]), "+v"(tn_[KD - 1]) : : "memory"); \
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tn_[0]) : : "memory");                              \
    } while (0)
#define WNWG_ADDR(buf, c)                                                                                   \
    lds_fptr la_ = (lds_fptr)(lds + (buf) * STG + wave * 256);                                              \
    wg_u32x4 e_[KD];                                                                                        \
    _Pragma("unroll") for (int j = 0; j < KD; ++j) {                                                        \
        if constexpr (TP) e_[j] = tn_[j];                                                                   \
        else e_[j] = ctab[(c) + j];                                                                         \
    }                                                                                                       \
    const bool as_ = (c) < c_e;                                      /* wave-uniform: SPLIT-packed panel */ \
    bool mk_[NI];                                                    /* wave-uniform: mapped cond chunk */ \
    _Pragma("unroll") for (int k = 0; k < NI; ++k) mk_[k] = (c) >= m_lo[k] && (c) < ps[k + 1];
#define WNWG_BASES()                                                                                        \
    gbyte_ptr ac_[KD], bp_[KD];                                                                             \
    _Pragma("unroll") for (int j = 0; j < KD; ++j) {                                                        \
        ac_[j] = reinterpret_cast<gbyte_ptr>(                                                               \
            ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)e_[j].y) << 32) |            \
            (unsigned)__builtin_amdgcn_readfirstlane((int)e_[j].x));                                        \
        bp_[j] = reinterpret_cast<gbyte_ptr>(                                                               \
            ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)e_[j].w) << 32) |            \
            (unsigned)__builtin_amdgcn_readfirstlane((int)e_[j].z));                                        \
    }
    // piece p of a stage: piece p % NP of its chunk p / NP
#define WNWG_PIECE(p)                                                                                       \
    do {                                                                                                    \
        if constexpr ((p) < KD * NP) {                                                                      \
            constexpr int sj_ = (p) / NP, q_ = (p) % NP;                                                    \
            if constexpr (q_ < 2) {                                                                         \
                unsigned o_ = as_ ? offa_s[q_] : offa_g[q_];                                                \
                asm volatile("" : "+v"(o_));                                                                \
                __builtin_amdgcn_global_load_lds((gfloat_ptr)(ac_[sj_] + o_), la_ + sj_ * CST + 1024 * q_, 16, 0, 0); \
            } else {                                                                                        \
                unsigned o_ = offb[q_ - 2];                                                                 \
                _Pragma("unroll") for (int k = 0; k < NI; ++k) o_ = mk_[k] ? offb_m[k][q_ - 2] : o_;        \
                asm volatile("" : "+v"(o_));                                                                \
                __builtin_amdgcn_global_load_lds((gfloat_ptr)(bp_[sj_] + o_), la_ + sj_ * CST + A_ST + 1024 * (q_ - 2), 16, 0, 0); \
            }                                                                                               \
        }                                                                                                   \
    } while (0)
#define WNWG_WAIT()                                                                                         \
    do {                                                                                                    \
        if constexpr (KD * NP == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                        \
        else if constexpr (KD * NP == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                   \
        else if constexpr (KD * NP == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                   \
        else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");                                               \
    } while (0)

    // KD (2 + NT) DMAs per thread per stage, in order: vmcnt(that) = "everything but the newest stage has landed" (the last two
    // iterations re-issue the final stage into a stage nobody reads any more: the DMA count per iteration stays constant)
    {
        if constexpr (TP) { WNWG_TAB_ISSUE(0) WNWG_TAB_WAIT(); }
        { WNWG_ADDR(0, 0) WNWG_BASES() WNWG_PIECE(0); WNWG_PIECE(1); WNWG_PIECE(2); WNWG_PIECE(3); WNWG_PIECE(4); WNWG_PIECE(5); WNWG_PIECE(6); WNWG_PIECE(7); }
        if constexpr (TP) { WNWG_TAB_ISSUE(KD) WNWG_TAB_WAIT(); }
        { WNWG_ADDR(1, KD) WNWG_BASES() WNWG_PIECE(0); WNWG_PIECE(1); WNWG_PIECE(2); WNWG_PIECE(3); WNWG_PIECE(4); WNWG_PIECE(5); WNWG_PIECE(6); WNWG_PIECE(7); }
        if constexpr (TP) { WNWG_TAB_ISSUE(2 * KD < nch ? 2 * KD : nch - KD) WNWG_TAB_WAIT(); }
        WNWG_WAIT();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }

    int cur = 0;
    // one chunk into accumulator set X: per k-step one fenced region [fragments of k-step ks + 1 | 2 NT MFMAs of ks | one DMA piece]
#define WNWG_READ_FRAGS(ks)                                                                                 \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) av[ks][mt] = As[(2 * (ks) + lhi) * 128 + mt * 64];     \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) bv[ks][nt] = Bs[(2 * (ks) + lhi) * BN + nt * 32];
#define WNWG_MFMA(Y, ks)                                                                                    \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                                        \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                   \
            Y[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks][mt], bv[ks][nt], Y[mt][nt], 0, 0, 0);
#define WNWG_REGION(Y, ks, p)                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    if constexpr ((ks) + 1 < GEMM_KC / 2) { WNWG_READ_FRAGS((ks) + 1) }                                     \
    WNWG_MFMA(Y, ks)                                                                                        \
    WNWG_PIECE(p);
#define WNWG_CHUNK1(Y)                                                                                      \
    {                                                                                                       \
        const float* As = lds + cur * STG + wm * 32 + l31;                                                  \
        const float* Bs = lds + cur * STG + A_ST + wn * (32 * NT) + l31;                                    \
        float av[GEMM_KC / 2][2], bv[GEMM_KC / 2][NT];                                                      \
        const int nb = cur >= 1 ? cur - 1 : 2;              /* (cur + 2) % 3: the stage of chunk ch - 1 */  \
        const int cn = ch + 2 < nch ? ch + 2 : nch - 1;                                                     \
        WNWG_ADDR(nb, cn)                                                                                   \
        WNWG_READ_FRAGS(0)                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        WNWG_BASES()                                                                                        \
        WNWG_REGION(Y, 0, 0) WNWG_REGION(Y, 1, 1) WNWG_REGION(Y, 2, 2) WNWG_REGION(Y, 3, 3)                 \
        WNWG_REGION(Y, 4, 4)                                                                                \
        if constexpr (TP) { WNWG_TAB_ISSUE(ch + 3 < nch ? ch + 3 : nch - 1) }                               \
        WNWG_REGION(Y, 5, 4) WNWG_REGION(Y, 6, 4) WNWG_REGION(Y, 7, 4)                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        if constexpr (TP) WNWG_TAB_WAIT();                                                                  \
        WNWG_WAIT();                                        /* chunk ch + 1 landed, the newest in flight */ \
        __builtin_amdgcn_s_barrier();                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        cur = cur == 2 ? 0 : cur + 1;                                                                       \
    }
    // KD = 2: a stage is two chunks = 16 k-step regions between two barriers.  The fragments run one region ahead ACROSS the chunk
    // and the stage boundary: the wait for the next stage's landing and the barrier stand in front of the LAST region (technique of
    // the hand-written small loop, gemm_f32_small.hip), which reads the next stage's first fragments under its own MFMAs.  Every
    // fragment read of this stage has returned before the barrier (lgkmcnt(0): issued a whole region earlier), so the DMA that
    // the next iteration aims at this stage's successor-but-one - the stage two barriers back - never meets a pending read.
    // Same products, same order per accumulator element as KD = 1: bit-identical.
    float fa[8 * KD][2], fb[8 * KD][NT];
#define WNWG_RD(r, Ap, Bp)                                                                                  \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) fa[r][mt] = (Ap)[((r) >> 3) * CST + (2 * ((r) & 7) + lhi) * 128 + mt * 64]; \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) fb[r][nt] = (Bp)[((r) >> 3) * CST + (2 * ((r) & 7) + lhi) * BN + nt * 32];
#define WNWG_MM(Y, r)                                                                                       \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                                        \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                   \
            Y[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[r][mt], fb[r][nt], Y[mt][nt], 0, 0, 0);
#define WNWG_R2(Y, r)                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    WNWG_RD((r) + 1, As, Bs)                                                                                \
    WNWG_MM(Y, r)                                                                                           \
    WNWG_PIECE(r);
#define WNWG_CHUNK2(Y)                                                                                      \
    {                                                                                                       \
        const float* As = lds + cur * STG + wm * 32 + l31;                                                  \
        const float* Bs = lds + cur * STG + A_ST + wn * (32 * NT) + l31;                                    \
        const int nx = cur == 2 ? 0 : cur + 1;                                                              \
        const float* An = lds + nx * STG + wm * 32 + l31;                                                   \
        const float* Bn = lds + nx * STG + A_ST + wn * (32 * NT) + l31;                                     \
        const int nb = cur >= 1 ? cur - 1 : 2;              /* the stage of chunks ch - 2, ch - 1 */        \
        const int cn = ch + 2 * KD < nch ? ch + 2 * KD : nch - KD;                                          \
        WNWG_ADDR(nb, cn)                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        WNWG_BASES()                                                                                        \
        WNWG_R2(Y, 0) WNWG_R2(Y, 1) WNWG_R2(Y, 2) WNWG_R2(Y, 3) WNWG_R2(Y, 4) WNWG_R2(Y, 5) WNWG_R2(Y, 6) WNWG_R2(Y, 7)   \
        WNWG_R2(Y, 8) WNWG_R2(Y, 9)                                                                         \
        WNWG_TAB_ISSUE(ch + 3 * KD < nch ? ch + 3 * KD : nch - KD)                                          \
        WNWG_R2(Y, 10) WNWG_R2(Y, 11) WNWG_R2(Y, 12) WNWG_R2(Y, 13) WNWG_R2(Y, 14)                          \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        WNWG_TAB_WAIT();                                    /* ... and this stage is read out */            \
        WNWG_WAIT();                                        /* the next stage landed, the newest in flight */ \
        __builtin_amdgcn_s_barrier();                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        WNWG_RD(0, An, Bn)                                                                                  \
        WNWG_MM(Y, 15)                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        cur = nx;                                                                                           \
    }
#define WNWG_CHUNK(Y)                                                                                       \
    if constexpr (KD == 1) WNWG_CHUNK1(Y) else WNWG_CHUNK2(Y)
    if constexpr (KD == 2) {
        const float* As = lds + wm * 32 + l31;
        const float* Bs = lds + A_ST + wn * (32 * NT) + l31;
        WNWG_RD(0, As, Bs)
    }

    // gate and store one accumulator set: packed column n of the batch item -> natural column (n / d) NI d + n % d + par d
    float* dst = a.act + (size_t)b * a.act_bstride + (size_t)(cb * 64 + wm * 32) * a.ld + a.pad;
    const float* bias = lds + BIAS + wm * 32;
#define WNWG_GATE(Y, par)                                                                                   \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                                     \
        const int n = n0 + wn * (32 * NT) + nt * 32 + l31;                                                  \
        const int ns = (n / a.d) * (NI * a.d) + n % a.d + (par) * a.d;                                      \
        if (n < a.Lp && ns < a.L) {                                                                         \
            _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                \
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lhi;                                           \
                const float u0 = Y[0][nt][r] + bias[row];                                                   \
                const float u1 = Y[1][nt][r] + bias[64 + row];                                              \
                dst[(size_t)row * a.ld + ns] = wg_tanh(u0) * wg_sigmoid(u1);                                \
            }                                                                                               \
        }                                                                                                   \
    }

#define WNWG_RUN(k, end) for (; ch < (end); ch += KD) WNWG_CHUNK(X[k])
#define WNWG_DRAIN()                                                                                        \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      /* the re-issued tail DMAs still target LDS */    \
    __builtin_amdgcn_s_barrier();
    int ch = 0;
    if constexpr (!F43) {
        WNWG_RUN(0, n1)
        WNWG_RUN(1, c_e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = X[0][i][j][r], dd = X[1][i][j][r];
                    X[0][i][j][r] = s + dd;
                    X[1][i][j][r] = s - dd;
                }
        WNWG_RUN(0, ps[1])
        WNWG_GATE(X[0], 0)
        WNWG_RUN(1, nch)
        WNWG_DRAIN()
        WNWG_GATE(X[1], 1)
    } else if constexpr (F43 == 1) {
        WNWG_RUN(0, n1)
        WNWG_RUN(1, 2 * n1)
        WNWG_RUN(2, 3 * n1)
        WNWG_RUN(3, c_e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (NT == 2)
                        if (r == 0) asm volatile("" : "+a"(X[0][i][j]), "+a"(X[1][i][j]), "+a"(X[2][i][j]), "+a"(X[3][i][j]));
                    const float p1 = X[0][i][j][r], p2 = X[1][i][j][r], p3 = X[2][i][j][r], p4 = X[3][i][j][r];
                    const float sa = p1 + p2, sb = p1 - p2, sc = p3 + p4, se = p3 - p4;
                    X[0][i][j][r] = sa + sc;
                    X[1][i][j][r] = sb + 2.0f * se;
                    X[2][i][j][r] = sa + 4.0f * sc;
                    X[3][i][j][r] = sb + 8.0f * se;
                    // (128 quad columns: one 16-register block of the four sets at a time, so that the butterfly never holds more)
                    if constexpr (NT == 2)
                        if (r == 15) asm volatile("" : "+a"(X[0][i][j]), "+a"(X[1][i][j]), "+a"(X[2][i][j]), "+a"(X[3][i][j]));
                }
        // the four sums exist HERE, in the accumulators' own registers: left to itself the compiler forms Y1..Y3 only in front of their
        // phases and holds a, c and the four products until then (224 registers where 128 do)
#pragma unroll
        for (int k = 0; k < NI; ++k)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                // (128 quad columns: 256 accumulator registers - the accumulator half of the one-wave-per-SIMD register file)
                if constexpr (NT == 2) { asm volatile("" : "+a"(X[k][i][0])); asm volatile("" : "+a"(X[k][i][1])); }
                else asm volatile("" : "+v"(X[k][i][0]));
            }
        WNWG_RUN(0, ps[1])
        WNWG_GATE(X[0], 0)
        WNWG_RUN(1, ps[2])
        WNWG_GATE(X[1], 1)
        WNWG_RUN(2, ps[3])
        WNWG_GATE(X[2], 2)
        WNWG_RUN(3, nch)
        WNWG_DRAIN()
        WNWG_GATE(X[3], 3)
    } else {
        WNWG_RUN(0, n1)
        WNWG_RUN(1, 2 * n1)
        WNWG_RUN(2, 3 * n1)
        WNWG_RUN(3, 4 * n1)
        WNWG_RUN(4, 5 * n1)
        WNWG_RUN(5, c_e)
        // one 16-register block of the six sets at a time, the six sums pinned where the accumulators are (see the F(4,3) form)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            asm volatile("" : "+v"(X[0][i][0]), "+v"(X[1][i][0]), "+v"(X[2][i][0]), "+v"(X[3][i][0]), "+v"(X[4][i][0]), "+v"(X[5][i][0]));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p1 = X[0][i][0][r], p2 = X[1][i][0][r], p3 = X[2][i][0][r], p4 = X[3][i][0][r], p5 = X[4][i][0][r], p6 = X[5][i][0][r];
                const float sa = p1 + p2, sb = p1 - p2, sc = p3 + p4, se = p3 - p4, sf = p5 + p6, sg = p5 - p6;
                float y0 = (sa + sc) + sf, y1 = (sb + 2.0f * se) + 0.5f * sg, y2 = (sa + 4.0f * sc) + 0.25f * sf;
                float y3 = (sb + 8.0f * se) + 0.125f * sg, y4 = (sa + 16.0f * sc) + 0.0625f * sf, y5 = (sb + 32.0f * se) + 0.03125f * sg;
                // (one element of the six sets at a time: the file holds 192 accumulators, the main loop's state and six sums, no more)
                asm volatile("" : "+v"(y0), "+v"(y1), "+v"(y2), "+v"(y3), "+v"(y4), "+v"(y5));
                X[0][i][0][r] = y0; X[1][i][0][r] = y1; X[2][i][0][r] = y2; X[3][i][0][r] = y3; X[4][i][0][r] = y4; X[5][i][0][r] = y5;
            }
            asm volatile("" : "+v"(X[0][i][0]), "+v"(X[1][i][0]), "+v"(X[2][i][0]), "+v"(X[3][i][0]), "+v"(X[4][i][0]), "+v"(X[5][i][0]));
        }
        WNWG_RUN(0, ps[1])
        WNWG_GATE(X[0], 0)
        WNWG_RUN(1, ps[2])
        WNWG_GATE(X[1], 1)
        WNWG_RUN(2, ps[3])
        WNWG_GATE(X[2], 2)
        WNWG_RUN(3, ps[4])
        WNWG_GATE(X[3], 3)
        WNWG_RUN(4, ps[5])
        WNWG_GATE(X[4], 4)
        WNWG_RUN(5, nch)
        WNWG_DRAIN()
        WNWG_GATE(X[5], 5)
    }
#undef WNWG_DRAIN
#undef WNWG_RUN
#undef WNWG_GATE
#undef WNWG_CHUNK
#undef WNWG_CHUNK2
#undef WNWG_R2
#undef WNWG_MM
#undef WNWG_RD
#undef WNWG_CHUNK1
#undef WNWG_REGION
#undef WNWG_MFMA
#undef WNWG_READ_FRAGS
#undef WNWG_WAIT
#undef WNWG_PIECE
#undef WNWG_BASES
#undef WNWG_TAB_WAIT
#undef WNWG_TAB_ISSUE
#undef WNWG_ADDR
}

bool wn_winograd_layer_supported(int C, int H) {
    return C >= 128 && C % 128 == 0 && H > 0 && H % GEMM_KC == 0 && 2 * (C / GEMM_KC) + 2 * ((C + H) / GEMM_KC) <= WNWG_MAX_CHUNKS;
}

bool wn_winograd_layer_f43_supported(int C, int H) {
    return wn_winograd_layer_supported(C, H) && 4 * (C / GEMM_KC) + 2 * ((C + H) / GEMM_KC) + 2 * (H / GEMM_KC) <= WNWG_MAX_CHUNKS;
}

// (two chunks per stage only: every phase - n1, n2 or nh chunks - a whole number of stages)
bool wn_winograd_layer_f63_supported(int C, int H) {
    return wn_winograd_layer_f43_supported(C, H) && H % (2 * GEMM_KC) == 0 &&
           6 * (C / GEMM_KC) + 2 * ((C + H) / GEMM_KC) + 4 * (H / GEMM_KC) <= WNWG_MAX_CHUNKS;
}

namespace {
thread_local int t_last_f43_width = 0;

template <int NT, int F43, int KD, int TP>
int launch_wnwg_shape(WnWinogradLayerArgs a, int kt, long long kt_total, hipStream_t stream) {
    a.kt = kt;
    a.kt_total = (int)kt_total;
    const long long blocks = 8ll * (a.C / 64) * ((kt_total + 7) / 8);
    CTTS_CHECK_ARG(blocks > 0 && blocks < (1ll << 31) && kt_total < (1ll << 31), "wn_winograd_layer: grid %lld", blocks);
    hipLaunchKernelGGL((wn_winograd_layer_f32_kernel<NT, F43, KD, TP>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
    CTTS_CHECK_LAUNCH("wn_winograd_layer");
    return CTTS_OK;
}

}  // namespace

int last_wn_winograd_f43_width() { return t_last_f43_width; }

int launch_wn_winograd_layer(const WnWinogradLayerArgs& a_in, hipStream_t stream) {
    WnWinogradLayerArgs a = a_in;
    CTTS_CHECK_ARG(wn_winograd_layer_supported(a.C, a.H), "wn_winograd_layer: C=%d H=%d", a.C, a.H);
    CTTS_CHECK_ARG(a.A_T2 && a.A_T3 && a.A_e && a.A_o && a.bias && a.V && a.act && a.batch >= 1, "wn_winograd_layer: operand not set");
    const bool f43 = a.form == WNWG_F43, f63 = a.form == WNWG_F63;
    const int tw = f43 || f63 ? 64 : 128;                 // columns of a tile that ntiles counts
    CTTS_CHECK_ARG(a.form == WNWG_F23 || (f43 && wn_winograd_layer_f43_supported(a.C, a.H) && a.A_T4 && a.A_T5) ||
                       (f63 && wn_winograd_layer_f63_supported(a.C, a.H) && a.A_T4 && a.A_T5 && a.A_T6 && a.A_T7 && a.in_place),
                   "wn_winograd_layer: form %d", a.form);
    CTTS_CHECK_ARG(a.d >= 1 && a.L >= 1 && a.Lp >= 1 && a.ntiles >= 1 && a.Lp <= a.ntiles * tw && a.ntiles * tw <= a.ldp && a.ldp % 4 == 0 &&
                       a.ld % 4 == 0 && a.pad >= 0 && a.pad % 4 == 0 && a.L + a.pad <= a.ld,
                   "wn_winograd_layer: geometry d=%d L=%d Lp=%d ntiles=%d ldp=%d ld=%d pad=%d", a.d, a.L, a.Lp, a.ntiles, a.ldp, a.ld, a.pad);
    // in place: a lane's four pair columns must be four consecutive, 16-byte aligned natural columns
    CTTS_CHECK_ARG(a.in_place ? (a.h2 && a.d % 4 == 0 && a.ld - a.pad >= 4 && a.h_bstride % 4 == 0 && reinterpret_cast<uintptr_t>(a.h2) % 16 == 0)
                              : a.Hc != nullptr,
                   "wn_winograd_layer: cond rows (in_place=%d d=%d)", a.in_place, a.d);
    a.b0 = 0;
    a.col0 = 0;
    const Tuning tn = tuning();
    // F(6,3): 64 hex columns = 384 natural columns, two chunks per stage - the F(4,3) kernel's tile, main-loop body and occupancy
    if (f63) return launch_wnwg_shape<1, 2, 2, 1>(a, a.ntiles, (long long)a.ntiles * a.batch, stream);
    if (f43) {
        // 64 quad columns with two chunks per stage at every grid size: 3.786 ms per config-2 layer where the parent's kernel (one chunk
        // per stage, table read by a plain load: kept as the CTTS_F32_FORCE_SMALL arm) takes 4.002 and the 128-column shape 4.233
        // (profiles/r26_01_f43_wide_gonogo.txt).  The 128-column shape stays reachable as the CTTS_F32_NO_SMALL arm; all three sum
        // every column's products in the same order: bit-identical.
        // (two chunks per stage: every phase - n1, n2 or nh chunks - must be a whole number of stages; C % 128 == 0 already holds)
        const bool kd2 = a.H % (2 * GEMM_KC) == 0;
        if (tn.f32_no_small && kd2) {
            const int wt = (a.ntiles + 1) / 2;            // 128-column tiles per batch item
            CTTS_CHECK_ARG((long long)wt * 128 <= a.ldp, "wn_winograd_layer: %d tiles of 128 quad columns beyond ldp=%d", wt, a.ldp);
            t_last_f43_width = 128;
            return launch_wnwg_shape<2, 1, 2, 1>(a, wt, (long long)wt * a.batch, stream);
        }
        t_last_f43_width = 64;
        if (tn.f32_force_small || !kd2) return launch_wnwg_shape<1, 1, 1, 0>(a, a.ntiles, (long long)a.ntiles * a.batch, stream);
        return launch_wnwg_shape<1, 1, 2, 1>(a, a.ntiles, (long long)a.ntiles * a.batch, stream);
    }
    const int ncb = a.C / 64;
    const long long slots = 2ll * wf_row_cus();
    const int kt_narrow = (a.Lp + 63) / 64;
    long long tiles = (long long)a.ntiles * a.batch;
    // the narrow shape where the wide one would run fewer than two whole rounds (the role of gemm_f32_small_applies): no peel exists
    // there, and three narrow workgroups fit a CU.  Measured at one 900-frame utterance (904 wide workgroups): 72.2 against 73.2 ms
    // per step (profiles/r17_01_winograd_fused_ab.txt); from four utterances on the wide shape with its peel is level or ahead
    if (!tn.f32_no_small && (tn.f32_force_small || ncb * tiles < 2 * slots)) return launch_wnwg_shape<1, 0, 1, 0>(a, kt_narrow, (long long)kt_narrow * a.batch, stream);
    // Round-aligned launch (gemm_f32.hip, launch_gemm_f32): the tiles beyond the last whole round of 2 x CUs workgroups - they lie at
    // the end of the last batch item - go to a launch of the narrow shape FIRST, and the wide launch covers the rest
    if (!tn.f32_no_round_split && !tn.f32_no_small) {
        const long long rounds = ncb * tiles / slots;
        const long long rem_tiles = (ncb * tiles - rounds * slots + ncb - 1) / ncb;
        if (rounds >= 2 && rem_tiles > 0 && rem_tiles * ncb <= slots * 3 / 10 && rem_tiles < a.ntiles &&
            (long long)(a.ntiles - rem_tiles) * 128 < a.Lp) {
            WnWinogradLayerArgs r = a;
            r.b0 = a.batch - 1;
            r.col0 = (int)(a.ntiles - rem_tiles) * 128;
            const int kt = (a.Lp - r.col0 + 63) / 64;
            if (int rc = launch_wnwg_shape<1, 0, 1, 0>(r, kt, kt, stream)) return rc;
            tiles -= rem_tiles;
        }
    }
    return launch_wnwg_shape<2, 0, 1, 0>(a, a.ntiles, tiles, stream);
}

}  // namespace ctts
