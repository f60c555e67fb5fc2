// kernels_match.hip — dense correspondence (gfx950): for every patch row of image A the best-matching patch row of image B, by the
// inner product of their 16-bit images.  Contract: include/vithip.h, "Dense correspondence"; DESIGN.md 4.32.
//
//   match_prep_kernel   a wave per patch row, on the steps of feat_row.h (row_load, row_stats, piece_norm: the bits of the token
//                       features): x = hi + lo as the forward left it, optionally through the final LayerNorm, rounded to the operand
//                       type -- the operand of VH_MATCH_DOT.  VH_MATCH_COSINE divides the ROUNDED row by its L2 norm and rounds again:
//                       S = sum of x16^2 in fp32, lane l of 64 adding its pieces (8 consecutive elements) l, l + 64, .. in that order
//                       from +0, each piece as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) of the rounded squares, then the xor
//                       butterfly of wave_sum; n = sqrtf(S); y = RNE_T16(x16 / n), one correctly rounded fp32 quotient per element.
//                       S = 0: the row stays zero.  The rows of image b land at out16 + b * NP * D, class-token and register rows skipped.
//   match_kernel        S = A B^T per pair on the matrix cores with an epilogue that never stores S.  A workgroup of four waves owns one
//                       pair and QB = 64 QT query rows (QT = 1 or 2), walks B in key tiles of 64 rows and the width in chunks of 64
//                       elements.  One (key tile, chunk) step = QB + 64 rows of 128 bytes in one slot of a three-slot LDS ring, moved by
//                       LDS-DMA in pieces of 8 rows (1 KiB), every wave (QB + 64) / 32 pieces; the query block is streamed again for every
//                       key tile (it comes from L2: a pair's rows are a few hundred KiB), so any width runs in the same 36 / 72 KiB.  Per
//                       step: a counted vmcnt leaves the next step's pieces in flight, the ring barrier, the refill of the slot read
//                       two steps ago, then four k-steps of v_mfma_f32_32x32x16.  The LDS row image: 16-byte chunk c of row r sits at
//                       128 r + 16 (c ^ ((r >> 1) & 7)); an operand read (lane l: row l & 31, chunk 2 ks + (l >> 5)) puts 16 consecutive
//                       rows on the 16 different 16-byte columns of the 256-byte bank span.  The DMA lands lane-linear: the
//                       permutation goes on the lane's global source address.
//                       Waves 2 x 2: wave w takes query rows 32 QT (w >> 1) .. and keys 32 (w & 1) .. 32 (w & 1) + 31 of the tile, the keys
//                       as the A operand: the 16 accumulator values of a lane belong to ONE query (column l & 31) and keys 8 (j / 4) +
//                       4 (l >> 5) + j % 4, ascending in j.  Selection: after a tile's last chunk the lane folds its 16 values into its
//                       running (score, key) with a strict > over ascending keys, a key >= nb never entering (by index: the clamped rows
//                       behind nb replicate row nb - 1).  After the last tile the four candidates of a query -- two lane halves x two key
//                       waves -- meet in LDS and one thread per query takes the first under (score descending, key ascending).
//                       Rows behind na are computed from the clamped row na - 1 and not stored.  All offsets of a pair are 64-bit.
// No atomics, no scratch, no allocation, no counter: nothing but the arguments; a pair's result depends on its own rows alone.
#include <limits.h>
#include <math.h>

#include "attn_common.h"
#include "feat_row.h"
#include "vh_kernels.h"

namespace vh {

namespace {

constexpr int kMtKeys = 64;      // key rows of a tile
constexpr int kMtChunk = 64;     // elements of the width per ring step: 128 bytes of a row
constexpr int kMtSlots = 3;      // ring depth in steps

__device__ __forceinline__ bool mt_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

template <typename T, typename IN>
__global__ void __launch_bounds__(256)
match_prep_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int64_t rows, int np, int tokens, int lead, int dim,
                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int norm, int cosine,
                  typename T::elem* __restrict__ out16) {
#pragma clang fp contract(off)
    using V4 = typename T::vec4;
    using V8 = typename T::vec8;
    const int lane = threadIdx.x & 63, npiece = dim >> 3;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;   // whole waves
    const int64_t img = m / np;
    float v[4][8];
    row_load<IN, 4>(hi, lo, img * tokens + lead + (m - img * np), dim, lane, v);
    if (norm) {
        float mean, rstd;
        row_stats<4>(v, dim, lane, eps, mean, rstd);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (lane + 64 * i < npiece) piece_norm(v[i], lane + 64 * i, mean, rstd, gamma, beta);
    }
    V8 x16[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const V4 a = pack4<T>(v[i][0], v[i][1], v[i][2], v[i][3]), b = pack4<T>(v[i][4], v[i][5], v[i][6], v[i][7]);
        x16[i] = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
        if (lane + 64 * i < npiece) {
            float q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float x = (float)x16[i][j]; v[i][j] = x; q[j] = x * x; }
            s += ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
        }
    }
    if (cosine) {
        s = wave_sum(s);
        if (s > 0.f) {
            const float n = sqrtf(s);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const V4 a = pack4<T>(v[i][0] / n, v[i][1] / n, v[i][2] / n, v[i][3] / n);
                const V4 b = pack4<T>(v[i][4] / n, v[i][5] / n, v[i][6] / n, v[i][7] / n);
                x16[i] = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
            }
        }
    }
    V8* const o = (V8*)(out16 + m * dim);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < npiece) o[lane + 64 * i] = x16[i];
}

// pair p: images pairs[2 p], pairs[2 p + 1] of [images][na][W] rows (the context: A and B are one array), or with pairs == nullptr
// image p of both arrays (the tap).  An image index outside 0 .. images - 1 (device pairs only: host pairs are refused before the
// launch) gives index -1 and score -inf for the pair's rows and reads nothing.
template <typename T, int QT>
__global__ void __launch_bounds__(256)
match_kernel(const typename T::elem* __restrict__ a16, const typename T::elem* __restrict__ b16, const int32_t* __restrict__ pairs, int images,
             int na, int nb, int W, int qblocks, int32_t* __restrict__ idx, float* __restrict__ score) {
    using E = typename T::elem;
    using V8 = typename T::vec8;
    constexpr int QB = 64 * QT, kRows = QB + kMtKeys, kStep = kRows * 128, kPieces = kRows / 8, kPerWave = kPieces / 4;
    extern __shared__ __attribute__((aligned(16))) char mt_smem[];
    uint2* const red = (uint2*)(mt_smem + kMtSlots * kStep);   // [key wave][lane half][QB]: x = the score's bits, y = the key
    const uint32_t lds0 = (uint32_t)(uintptr_t)mt_smem;
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hl = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wq = wave >> 1, wk = wave & 1;
    const int pair = blockIdx.x / qblocks, q0 = (blockIdx.x - pair * qblocks) * QB;
    const int64_t obase = (int64_t)pair * na + q0;

    int ia = pair, ib = pair;
    if (pairs) { ia = pairs[2 * pair]; ib = pairs[2 * pair + 1]; }
    if ((unsigned)ia >= (unsigned)images || (unsigned)ib >= (unsigned)images) {   // workgroup-uniform
        if (t < QB && q0 + t < na) { idx[obase + t] = -1; score[obase + t] = -INFINITY; }
        return;
    }
    const E* const A = a16 + (int64_t)ia * na * W;
    const E* const B = b16 + (int64_t)ib * nb * W;
    const int nkc = W / kMtChunk, ntiles = (nb + kMtKeys - 1) / kMtKeys, nsteps = ntiles * nkc;

    // step s = (key tile s / nkc, chunk s % nkc) into slot s % kMtSlots: pieces g = wave, wave + 4, .. of 8 rows; rows 0 .. QB - 1 of a
    // step are the query block, the rest the key tile.  Lane ln of a piece lands at 16 ln: row 8 g + (ln >> 3), physical chunk ln & 7.
    // Byte offsets from A / B stay below 2^32: row < 4096, W <= 2048.
    auto issue = [&](int s) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of kept in registers across the loop
        const int kt = s / nkc, kc = s - kt * nkc;
        const uint32_t slot = lds0 + (uint32_t)(s % kMtSlots) * kStep;
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) {
            const int g = wave + 4 * i, r = 8 * g + (ln >> 3);
            const int c = (ln & 7) ^ ((r >> 1) & 7);
            const bool is_q = g < QB / 8;   // wave-uniform
            int row = is_q ? q0 + r : kt * kMtKeys + (r - QB);
            const int last = is_q ? na - 1 : nb - 1;
            row = row < last ? row : last;
            const uint32_t off = ((uint32_t)row * (uint32_t)W + (uint32_t)(kc * kMtChunk + 8 * c)) * 2u;
            asm_lds_dma16(is_q ? (const void*)A : (const void*)B, off, slot + (uint32_t)g * 1024u);
        }
    };

    for (int s = 0; s < kMtSlots - 1 && s < nsteps; ++s) issue(s);

    // this lane's operand rows in a step and their swizzles
    const int krow = QB + 32 * wk + l31, kswz = (krow >> 1) & 7;
    int qrow[QT], qswz[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) { qrow[i] = 32 * QT * wq + 32 * i + l31; qswz[i] = (qrow[i] >> 1) & 7; }

    f32x16 acc[QT];
    float best[QT];
    int bj[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        best[i] = -INFINITY;
        bj[i] = INT_MAX;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    }

    int kc = 0, kt = 0;
    for (int s = 0; s < nsteps; ++s) {
        // this wave's pieces of step s have landed (step s + 1 may stay in flight), then everyone's; step s - 1 has been read
        wait_vm<8>(s + 1 < nsteps ? kPerWave : 0);
        ring_barrier();
        if (s + kMtSlots - 1 < nsteps) issue(s + kMtSlots - 1);   // into step s - 1's slot
        const char* const st = mt_smem + (s % kMtSlots) * kStep;
#pragma unroll
        for (int ks = 0; ks < kMtChunk / 16; ++ks) {
            const int c = 2 * ks + hl;
            const V8 kf = *(const V8*)(st + krow * 128 + ((c ^ kswz) << 4));
#pragma unroll
            for (int i = 0; i < QT; ++i) {
                const V8 qf = *(const V8*)(st + qrow[i] * 128 + ((c ^ qswz[i]) << 4));
                acc[i] = T::mfma32(kf, qf, acc[i]);
            }
        }
        if (++kc == nkc) {   // the tile's scores are complete: fold them into the running best, keys ascending
            const int key0 = kt * kMtKeys + 32 * wk + 4 * hl;
#pragma unroll
            for (int i = 0; i < QT; ++i)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int key = key0 + 8 * (j >> 2) + (j & 3);
                    const float v = acc[i][j];
                    if (key < nb && v > best[i]) { best[i] = v; bj[i] = key; }
                    acc[i][j] = 0.f;
                }
            kc = 0;
            ++kt;
        }
    }

#pragma unroll
    for (int i = 0; i < QT; ++i) red[(2 * wk + hl) * QB + qrow[i]] = make_uint2(__float_as_uint(best[i]), (uint32_t)bj[i]);
    __syncthreads();
    if (t < QB && q0 + t < na) {
        float bs = -INFINITY;
        int bi = INT_MAX;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint2 e = red[c * QB + t];
            if (mt_before(__uint_as_float(e.x), (int)e.y, bs, bi)) { bs = __uint_as_float(e.x); bi = (int)e.y; }
        }
        idx[obase + t] = bi == INT_MAX ? 0 : bi;   // (no finite score at all: index 0, score -inf)
        score[obase + t] = bs;
    }
}

template <typename T, int QT>
hipError_t match_launch(const MatchArgs& a, hipStream_t s) {
    constexpr int QB = 64 * QT;
    const size_t lds = (size_t)kMtSlots * (QB + kMtKeys) * 128 + (size_t)4 * QB * 8;
    auto kern = match_kernel<T, QT>;
    static LdsDone lds_done;   // per instantiation, per device
    if (hipError_t e = ensure_dynamic_lds((const void*)kern, lds, lds_done); e != hipSuccess) return e;
    const int qblocks = (a.na + QB - 1) / QB;
    hipLaunchKernelGGL(kern, dim3((unsigned)a.npairs * (unsigned)qblocks), dim3(256), lds, s, (const typename T::elem*)a.a16,
                       (const typename T::elem*)a.b16, a.pairs, a.images, a.na, a.nb, a.width, qblocks, a.idx, a.score);
    return hipGetLastError();
}

}  // namespace

// 64 query rows per workgroup up to 256 workgroups' worth of pairs, 128 beyond: the smaller block fills the device at few pairs, the
// larger one halves the key traffic per query (DESIGN.md 4.32 has the measurement)
int match_query_rows(int npairs, int na) {
    const int force = env_int("VH_MATCH_QB", 0);   // read per call: tools/match_bench.py measures both in one process
    if (force == 64 || force == 128) return force;
    return (int64_t)npairs * ((na + 127) / 128) >= 256 && na > 64 ? 128 : 64;
}

const char* match_check(const MatchArgs& a) {
    if (!a.a16 || !a.b16) return "match: null rows";
    if (!a.idx || !a.score) return "match: null output (idx and score are both required)";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "match: dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.metric != VH_MATCH_COSINE && a.metric != VH_MATCH_DOT) return "match: metric is not VH_MATCH_COSINE or VH_MATCH_DOT";
    if (a.npairs < 1 || a.npairs > VH_MATCH_MAX_PAIRS) return "match: npairs is outside 1..65536";
    if (a.na < 1 || a.na > VH_MATCH_MAX_ROWS || a.nb < 1 || a.nb > VH_MATCH_MAX_ROWS) return "match: na or nb is outside 1..4096 rows";
    if (a.width < 64 || a.width > VH_MATCH_MAX_WIDTH || a.width % 64) return "match: width is not a multiple of 64 in 64..2048";
    if (a.pairs ? a.images < 1 : a.images != a.npairs) return "match: images does not cover the pairs";
    if (((uintptr_t)a.a16 | (uintptr_t)a.b16 | (uintptr_t)a.pairs | (uintptr_t)a.idx | (uintptr_t)a.score) & 15)
        return "match: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_match(const MatchArgs& a, hipStream_t s) {
    if (match_check(a)) return hipErrorInvalidValue;
    const int qb = match_query_rows(a.npairs, a.na);
    return dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        return qb == 128 ? match_launch<T, 2>(a, s) : match_launch<T, 1>(a, s);
    });
}

const char* match_prep_check(const MatchPrepArgs& a) {
    if (!a.hi || !a.out16) return "match_prep: null rows or output";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "match_prep: dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.form != VH_FEAT_FORM_F32 && a.form != a.dtype) return "match_prep: the rows are split planes of the operand type or fp32 rows";
    if ((a.form == a.dtype) != (a.lo != nullptr)) return "match_prep: split planes, and only they, take a lo plane";
    if (a.dim < 64 || a.dim > VH_MATCH_MAX_WIDTH || a.dim % 64) return "match_prep: dim is not a multiple of 64 in 64..2048";
    if (a.np < 1 || a.np > VH_MATCH_MAX_ROWS || a.lead < 0 || a.tokens != a.lead + a.np) return "match_prep: tokens must be lead + np, np in 1..4096";
    if (a.batch < 1 || a.batch > (1 << 20)) return "match_prep: batch outside 1..2^20";
    if (a.norm != VH_FEAT_NORM && a.norm != VH_FEAT_RAW) return "match_prep: norm must be VH_FEAT_NORM or VH_FEAT_RAW";
    if (a.norm == VH_FEAT_NORM && (!a.gamma || !a.beta || !(a.eps > 0.f))) return "match_prep: VH_FEAT_NORM needs gamma, beta and a positive eps";
    if (a.metric != VH_MATCH_COSINE && a.metric != VH_MATCH_DOT) return "match_prep: metric is not VH_MATCH_COSINE or VH_MATCH_DOT";
    if (((uintptr_t)a.hi | (uintptr_t)a.lo | (uintptr_t)a.gamma | (uintptr_t)a.beta | (uintptr_t)a.out16) & 15)
        return "match_prep: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_match_prep(const MatchPrepArgs& a, hipStream_t s) {
    if (match_prep_check(a)) return hipErrorInvalidValue;
    const int64_t rows = (int64_t)a.batch * a.np;
    return dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
        const int norm = a.norm == VH_FEAT_NORM, cosine = a.metric == VH_MATCH_COSINE;
        if (a.form == VH_FEAT_FORM_F32)
            hipLaunchKernelGGL((match_prep_kernel<T, InF32>), grid, block, 0, s, a.hi, a.lo, rows, a.np, a.tokens, a.lead, a.dim, a.gamma, a.beta,
                               a.eps, norm, cosine, (typename T::elem*)a.out16);
        else
            hipLaunchKernelGGL((match_prep_kernel<T, InSplit16<T>>), grid, block, 0, s, a.hi, a.lo, rows, a.np, a.tokens, a.lead, a.dim, a.gamma,
                               a.beta, a.eps, norm, cosine, (typename T::elem*)a.out16);
        return hipGetLastError();
    });
}

}  // namespace vh
