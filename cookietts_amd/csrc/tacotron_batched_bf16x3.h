// Split-bf16 (bf16x3) form of the batched decoder's three LSTM cell GEMMs (tacotron_batched.h, bg_body<..., BG_EPI_CELL>) for
// the plain schedule above 64 rows, on v_mfma_f32_16x16x32_bf16.  Arithmetic (the contract is at ctts_taco_decoder_steps_bf16x3):
//   weights, once at pack time:   w_hi = bf16_rne(w), w_lo = bf16_rne(w - w_hi)
//   X, as it is read for a product: x_hi = bf16_rne(x), x_lo = bf16_rne(x - x_hi)   (X stays fp32 in the workspace)
//   per chunk of 32 K columns:    acc += w_hi x_hi;  acc += w_lo x_hi;  acc += w_hi x_lo      (fp32 accumulate, no lo x lo term)
// The machinery is bg_body's: K split over the waves of a workgroup (one contiguous slice of the chunks each, summed through LDS
// in a fixed order at the end), a wave-private LDS ring filled by global_load_lds with counted vmcnt and no barrier in the K loop,
// X read item-major from the workspace pieces.  What differs:
//   * chunk = 32 K columns.  Weights are packed (bgx_pack_kernel) as [m-tile][chunk][hi | lo][lane][8 bf16]: lane (row = lane % 16,
//     kq = lane / 16) holds K columns 8 kq .. 8 kq + 7 - the A operand of the 16x16x32 MFMA.  A hi | lo pair is the 4 bytes of the
//     fp32 weight, so the planes are as large as the fp32 tiles: 2 KiB per m-tile and chunk.
//   * X: lane (item = lane % 16, kq) needs the 32 bytes x[item][32 c + 8 kq ..]: two 16-byte DMA units per item tile and chunk
//     (elements 0-3, 4-7), split into hi / lo in registers (v_cvt_pk_bf16_f32, an exact fp32 subtraction) - the B operand.
//   * a stage therefore holds 2 MTW + 2 NT KiB; (S - 1) x units <= 60 (vmcnt) and the CU's 160 KiB of LDS bound S.
//   * the D layout is the 16x16x4 form's (lane (j, col): rows 4 j .. 4 j + 3 of column col), so the cell update is BG_EPI_CELL's.
//   * the three products of a chunk chain on one accumulator: each is issued for all (m-tile, item tile) pairs before the next, so
//     a dependent MFMA is MTW x NT issues behind the one it waits for.
// The item-tile shape (NT) and the number of waves (the K split) are the same for every batch above 64 rows: an item's bits do
// not depend on the batch it is decoded in.  Included by tacotron_decoder.hip after tacotron_batched.h.
#pragma once

typedef __bf16 bgx_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int BGX_KC = 32;

// two fp32 -> packed bf16, round to nearest even (one v_cvt_pk_bf16_f32); the low half is `a`
__device__ __forceinline__ unsigned bgx_pack2(float a, float b) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
}
// (a, b) -> hi pair, lo pair: hi = bf16_rne(x), lo = bf16_rne(x - hi) (the subtraction is exact in fp32)
__device__ __forceinline__ void bgx_split2(float a, float b, unsigned& hi, unsigned& lo) {
    hi = bgx_pack2(a, b);
    lo = bgx_pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

// dst (32-bit words) [((tile * nchunks + c) * 2 + plane) * 64 + lane][4]: word e holds W'[16 tile + lane % 16][32 c + 8 (lane / 16) +
// 2 e, + 1] of plane hi (0) / lo (1); W' as in bg_pack_kernel (column concatenation of the segments, gate-interleaved rows)
struct BgxPackArgs { BgSeg seg[4]; int nseg, rows, tiles, nchunks, interleave_H; unsigned* dst; };
__global__ __launch_bounds__(256) void bgx_pack_kernel(const BgxPackArgs a) {
    const size_t total = (size_t)a.tiles * a.nchunks * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int e = i & 3, lane = (i >> 2) & 63;
        const size_t tc = i >> 8;
        const int c = (int)(tc % a.nchunks), tile = (int)(tc / a.nchunks);
        const int r = BG_MT * tile + (lane & 15);
        float v[2] = {0.f, 0.f};
        if (r < a.rows) {
            const int src_row = a.interleave_H ? (r & 3) * a.interleave_H + (r >> 2) : r;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int k = BGX_KC * c + 8 * (lane >> 4) + 2 * e + u;
                for (int s = 0; s < a.nseg; ++s) {
                    if (k < a.seg[s].width) { v[u] = a.seg[s].ptr[(size_t)src_row * a.seg[s].ld + a.seg[s].col0 + k]; break; }
                    k -= a.seg[s].width;
                }
            }
        }
        unsigned hi, lo;
        bgx_split2(v[0], v[1], hi, lo);
        a.dst[((tc * 2 + 0) * 64 + lane) * 4 + e] = hi;
        a.dst[((tc * 2 + 1) * 64 + lane) * 4 + e] = lo;
    }
}

template <int MTW, int NT, int S, int WAVES>
constexpr int bgx_lds_bytes() { return WAVES * S * 2 * (MTW + NT) * 1024; }

// BgArgs as for bg_body, with W = the split planes and nchunks / cend[] counted in chunks of 32; the whole K in one launch
// (pmode 0).  blk = which group of MTW m-tiles, ngrp = which group of 16 NT items.
template <int MTW, int NT, int S, int WAVES>
__device__ __forceinline__ void bgx_cell_body(const BgArgs& a, bg_u4* lds, int blk, int ngrp) {
    constexpr int UNITS = 2 * (MTW + NT);                 // 1 KiB units per stage: per m-tile hi, lo; per item tile elements 0-3, 4-7
    static_assert(S >= 2 && (S - 1) * UNITS <= 60, "vmcnt is a 6-bit counter");
    static_assert(S * UNITS >= MTW * NT, "the ring also holds the waves' partial sums");
    static_assert(WAVES == 2 || WAVES == 4, "cross-wave sum");
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile0 = blk * MTW, n0 = ngrp * (16 * NT);
    const int per = (a.nchunks + WAVES - 1) / WAVES;
    const int c0 = min(wave * per, a.nchunks), cpw = min(per, a.nchunks - c0);      // this wave's chunks [c0, c0 + cpw)
    bg_u4* ring = lds + wave * (S * UNITS * 64);

    const float* wl[MTW];                                  // weight cursor: tile, chunk c0, plane hi, this lane (lo: + 256 floats)
#pragma unroll
    for (int m = 0; m < MTW; ++m) wl[m] = a.W + (((size_t)min(tile0 + m, a.tiles - 1) * a.nchunks + c0) * 128 + lane) * 4;
    const int item = n0 + (lane & 15), kq8 = 8 * (lane >> 4);
    int pi = (c0 >= a.cend[0]) + (c0 >= a.cend[1]) + (c0 >= a.cend[2]);
    int xwidth = a.x[pi].width;
    int left = a.cend[pi] - c0;
    const float* xp = a.x[pi].ptr + (size_t)item * xwidth + (c0 - (pi ? a.cend[pi - 1] : 0)) * BGX_KC + kq8;

    auto issue = [&](int st) {                            // the next chunk of this wave's slice -> stage st
        bg_lptr dst = (bg_lptr)(ring + st * UNITS * 64);
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            __builtin_amdgcn_global_load_lds((bg_gptr)wl[m], dst + (2 * m) * 64, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((bg_gptr)(wl[m] + 256), dst + (2 * m + 1) * 64, 16, 0, 0);
            wl[m] += 512;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float* xq = xp + (size_t)(16 * nt) * xwidth;
            __builtin_amdgcn_global_load_lds((bg_gptr)xq, dst + (2 * MTW + 2 * nt) * 64, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((bg_gptr)(xq + 4), dst + (2 * MTW + 2 * nt + 1) * 64, 16, 0, 0);
        }
        xp += BGX_KC;
        if (--left == 0 && pi < 3) {                       // wave-uniform, a few times per launch
            ++pi;
            xwidth = a.x[pi].width;
            left = a.cend[pi] - a.cend[pi - 1];
            xp = a.x[pi].ptr + (size_t)item * xwidth + kq8;
        }
    };

    bg_f4 acc[MTW][NT];
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = bg_f4{0.f, 0.f, 0.f, 0.f};

    int ist = 0;                                          // stage the next issue goes to
#pragma unroll
    for (int i = 0; i < S - 1; ++i)
        if (i < cpw) { issue(ist); ist = ist == S - 1 ? 0 : ist + 1; }
    // the cell's own operands of this wave's FIRST (m-tile, item tile) pair, requested behind the ring's first DMAs (as bg_body)
    float e_pre[4] = {0.f, 0.f, 0.f, 0.f};
    float e_c = 0.f;
    {
        const int tile = tile0 + wave / NT, it = n0 + 16 * (wave % NT) + (lane & 15), j = lane >> 4;
        if (wave < MTW * NT && it < a.batch && tile < a.tiles) {
            const int unit = 4 * tile + j;
#pragma unroll
            for (int g = 0; g < 4; ++g) e_pre[g] = a.bih[g * a.H + unit] + a.bhh[g * a.H + unit];
            e_c = a.c[(size_t)it * a.H + unit];
        }
    }

    bg_u4 opA[UNITS], opB[UNITS];
    auto read_ops = [&](bg_u4 (&op)[UNITS], int st) {
        const bg_u4* sp = ring + st * UNITS * 64 + lane;
#pragma unroll
        for (int u = 0; u < UNITS; ++u) op[u] = sp[u * 64];
    };
    auto mfmas = [&](const bg_u4 (&op)[UNITS]) {
        bg_u4 xh[NT], xl[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bg_u4& src = op[2 * MTW + 2 * nt + (e >> 1)];
                unsigned hi, lo;
                bgx_split2(__uint_as_float(src[2 * (e & 1)]), __uint_as_float(src[2 * (e & 1) + 1]), hi, lo);
                xh[nt][e] = hi; xl[nt][e] = lo;
            }
#define BGX_PRODUCT(A_, B_)                                                                                                       \
    _Pragma("unroll") for (int m = 0; m < MTW; ++m) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                             \
        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bgx_bf16x8, A_), __builtin_bit_cast(bgx_bf16x8, B_), acc[m][nt], 0, 0, 0);
        BGX_PRODUCT(op[2 * m], xh[nt])                    // w_hi x_hi
        BGX_PRODUCT(op[2 * m + 1], xh[nt])                // w_lo x_hi
        BGX_PRODUCT(op[2 * m], xl[nt])                    // w_hi x_lo
#undef BGX_PRODUCT
    };
    if (cpw > 0) {
        if (cpw >= S - 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 2) * UNITS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        read_ops(opA, 0);
    }
    int rst = 1 % S;                                      // stage of chunk i + 1
    auto step = [&](int i, bg_u4 (&cur)[UNITS], bg_u4 (&nxt)[UNITS]) {
        if (i + S - 1 < cpw) { issue(ist); ist = ist == S - 1 ? 0 : ist + 1; }
        if (i + 1 < cpw) {
            if (i + S - 1 < cpw) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 2) * UNITS) : "memory");   // chunk i + 1 landed
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            read_ops(nxt, rst);
            rst = rst == S - 1 ? 0 : rst + 1;
        }
        mfmas(cur);
    };
    for (int i = 0; i < cpw; i += 2) {
        step(i, opA, opB);
        if (i + 1 < cpw) step(i + 1, opB, opA);
    }

    // cross-wave sum of the K slices, fixed order: (w0 + w1) + (w2 + w3)
    __syncthreads();
    bg_f4* red = reinterpret_cast<bg_f4*>(lds);
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) red[((wave * MTW + m) * NT + nt) * 64 + lane] = acc[m][nt];
    __syncthreads();
    constexpr int NK = (MTW * NT + WAVES - 1) / WAVES;     // (m-tile, item tile) pairs per wave
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int idx = wave + k * WAVES;
        if (idx >= MTW * NT) continue;
        const int m = idx / NT, nt = idx % NT;
        bg_f4 pw[WAVES];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) pw[w] = red[((w * MTW + m) * NT + nt) * 64 + lane];
        bg_f4 sum = pw[0] + pw[1];
        if constexpr (WAVES == 4) sum += pw[2] + pw[3];
        const int tile = tile0 + m;
        const int it = n0 + 16 * nt + (lane & 15);
        const int j = lane >> 4;
        if (it >= a.batch || tile >= a.tiles) continue;
        const bool first = k == 0;                         // operands prefetched above
        // LSTMCell, exactly BG_EPI_CELL's epilogue
        const int unit = 4 * tile + j, H = a.H;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = sum[g] + (first ? e_pre[g] : a.bih[g * H + unit] + a.bhh[g * H + unit]);
        const size_t ix = (size_t)it * H + unit;
        const float ig = bg_sigmoid(pre[0]), fg = bg_sigmoid(pre[1]), gg = tanhf(pre[2]), og = bg_sigmoid(pre[3]);
        const float cy = fg * (first ? e_c : a.c[ix]) + ig * gg;
        const float hy = og * tanhf(cy);
        a.c[ix] = cy;
        a.h_new[ix] = hy;
        if (a.hsum) {
            const float hs = hy + a.hres[ix];
            a.hsum[ix] = hs;
            if (a.hid) a.hid[((size_t)it * a.hid_D + unit) * a.max_steps + a.step] = hs;
        }
    }
}

template <int MTW, int NT, int S, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void bgx_cell_kernel(const BgArgs a) {
    extern __shared__ __attribute__((aligned(16))) bg_u4 bg_lds[];
    bgx_cell_body<MTW, NT, S, WAVES>(a, bg_lds, blockIdx.x, blockIdx.y);
}

// the attention RNN's launch: workgroups [0, nblk) are the cell's, [nblk, nblk + batch) (of grid row 0) the attention's part 1
template <int MTW, int NT, int S, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void bgx_cell_attn_kernel(const BgArgs a, int nblk, const AttnArgs at, float* apre, int* astart) {
    extern __shared__ __attribute__((aligned(16))) bg_u4 bg_lds[];
    static_assert(sizeof(BgAttnLds) <= bgx_lds_bytes<MTW, NT, S, WAVES>(), "the attention scratch shares the ring");
    if ((int)blockIdx.x < nblk) bgx_cell_body<MTW, NT, S, WAVES>(a, bg_lds, blockIdx.x, blockIdx.y);
    else if (blockIdx.y == 0) attn_pre_body(at, apre, astart, *reinterpret_cast<BgAttnLds*>(bg_lds), blockIdx.x - nblk);
}

// two independent cells in one launch (teacher-forced loop: the attention RNN of step t + 1 and the second decoder RNN of step t):
// workgroups [0, nblk0) of every grid row are a0's, [nblk0, gridDim.x) a1's.  The body is the one of the launches above, so a
// cell's bits are the same alone and as a role.  (Two kernel parameters, not an array of roles: see bg_multi8_kernel.)
template <int MTW, int NT, int S, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void bgx_cell2_kernel(const BgArgs a0, int nblk0, const BgArgs a1) {
    extern __shared__ __attribute__((aligned(16))) bg_u4 bg_lds[];
    if ((int)blockIdx.x < nblk0) bgx_cell_body<MTW, NT, S, WAVES>(a0, bg_lds, blockIdx.x, blockIdx.y);
    else bgx_cell_body<MTW, NT, S, WAVES>(a1, bg_lds, blockIdx.x - nblk0, blockIdx.y);
}

template <int MTW, int NT, int S, int WAVES>
int bgx_launch_shape2(const BgArgs& a0, const BgArgs& a1, int nb_pad, hipStream_t s) {
    constexpr int LDS = bgx_lds_bytes<MTW, NT, S, WAVES>();
    static_assert(LDS <= 160 * 1024, "LDS of a CU");
    CTTS_CHECK_ARG(nb_pad % (16 * NT) == 0 && a0.pmode == 0 && a0.c_end == 0 && a1.pmode == 0 && a1.c_end == 0,
                   "bf16x3 cell pair: %d rows are not whole item groups of %d", nb_pad, 16 * NT);
    const int nblk0 = (a0.tiles + MTW - 1) / MTW, nblk1 = (a1.tiles + MTW - 1) / MTW, ny = nb_pad / (16 * NT);
    int rc;
    if ((rc = CTTS_ALLOW_LDS((bgx_cell2_kernel<MTW, NT, S, WAVES>), LDS))) return rc;
    hipLaunchKernelGGL((bgx_cell2_kernel<MTW, NT, S, WAVES>), dim3(nblk0 + nblk1, ny), dim3(64 * WAVES), LDS, s, a0, nblk0, a1);
    CTTS_CHECK_LAUNCH("bgx_cell2");
    return CTTS_OK;
}

// nb_pad: a multiple of 16 NT; attn != NULL: the attention's part 1 rides along
template <int MTW, int NT, int S, int WAVES>
int bgx_launch_shape(const BgArgs& a, int nb_pad, const AttnArgs* attn, float* apre, int* astart, int batch, hipStream_t s) {
    constexpr int LDS = bgx_lds_bytes<MTW, NT, S, WAVES>();
    static_assert(LDS <= 160 * 1024, "LDS of a CU");
    CTTS_CHECK_ARG(nb_pad % (16 * NT) == 0 && a.pmode == 0 && a.c_end == 0, "bf16x3 cell: %d rows are not whole item groups of %d", nb_pad, 16 * NT);
    const int nblk = (a.tiles + MTW - 1) / MTW, ny = nb_pad / (16 * NT);
    int rc;
    if (attn) {
        if ((rc = CTTS_ALLOW_LDS((bgx_cell_attn_kernel<MTW, NT, S, WAVES>), LDS))) return rc;
        hipLaunchKernelGGL((bgx_cell_attn_kernel<MTW, NT, S, WAVES>), dim3(nblk + batch, ny), dim3(64 * WAVES), LDS, s, a, nblk, *attn, apre, astart);
    } else {
        if ((rc = CTTS_ALLOW_LDS((bgx_cell_kernel<MTW, NT, S, WAVES>), LDS))) return rc;
        hipLaunchKernelGGL((bgx_cell_kernel<MTW, NT, S, WAVES>), dim3(nblk, ny), dim3(64 * WAVES), LDS, s, a);
    }
    CTTS_CHECK_LAUNCH("bgx_cell");
    return CTTS_OK;
}

// `a` as the fp32 launch would get it (bg_set_x: chunks of 16) -> the split planes, chunks of 32.  Every X piece is a multiple of
// 32 wide (DecPlan::x3_ok), so every chunk boundary of a piece is even.
inline BgArgs bgx_args(BgArgs a, const float* planes) {
    a.W = planes;
    a.nchunks /= 2;
    for (int i = 0; i < 4; ++i) a.cend[i] /= 2;
    return a;
}
