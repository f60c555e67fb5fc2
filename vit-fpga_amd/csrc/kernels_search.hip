// kernels_search.hip — embedding search (gfx950): the k best rows of a device-resident bank for every query row, by the
// inner product of their 16-bit images.  Contract: include/vithip.h, "Embedding search"; DESIGN.md 4.31.
//
//   search_prep_kernel   q16[i][j] = RNE_T16(q[i][j] * r_i), a wave per query row; r_i = 1 or 1 / sqrt(sum_j q^2) with the row-sum
//                        order of kernels_rows.hip: lane l adds its float4 chunks l, l + 64, .. in that order, each as
//                        (a + b) + (c + d) of the rounded squares, then the xor butterfly of wave_sum.  A row whose sum is 0 keeps
//                        r = 1 (it stays zero).  Rows nq .. nq_pad - 1 are written as zeros: the scan never checks a query bound
//                        when it loads.
//   search_scan_kernel   score = Bank . Q^T on the matrix cores with the selection run on the accumulators.  The grid is (bank slabs)
//                        x (query blocks), the query block fastest: the workgroups that share a slab are neighbours in launch order.
//                        A workgroup of four waves keeps its QL query rows resident in LDS for its whole life, in the image
//                        [k / 8][query][8 elements]: lane l of an operand read takes query l & 31 at k = 16 ks + 8 (l >> 5), so 16
//                        consecutive lanes read 256 consecutive bytes -- conflict-free at any W.  QL = 64 up to W = 768, 32 up to
//                        2048, 16 beyond (the upper half of the 32 MFMA columns is then zero), which keeps image + lists inside
//                        160 KiB.  The bank never passes through LDS: a workgroup walks its slab in rounds of 256 rows, wave w owns
//                        rows 64 w .. 64 w + 63 of the round as two 32-row tiles, and a lane loads its A fragment (row l & 31,
//                        16 bytes at k = 16 ks + 8 (l >> 5)) straight from global memory, four k-steps ahead in a second register
//                        set.  No other wave of the workgroup needs those bytes, so an LDS copy would buy no reuse.  Per k-step a
//                        wave issues QL / 32 LDS reads of 1 KiB and 2 QL / 32 MFMAs: 512 bytes of LDS per v_mfma_f32_32x32x16.
//                        The 16 accumulator values of a lane belong to ONE query (column l & 31), bank rows 8 (j / 4) + 4 (l >> 5)
//                        + j % 4 of the tile.
//                        Selection: per query an LDS list of kSrCap = 96 (score, index) entries, its fill counter, and tau = the
//                        k-th best entry (score and index) at the last compaction (-inf before).  A lane compares its values with
//                        tau under the total order -- an equal score passes only with a smaller index, which a retry inside a round
//                        can have -- and appends survivors through the counter.  A survivor that finds the list full stays pending in the lane; the
//                        workgroup learns of it in the round's one barrier (__syncthreads_or), compacts, and the lane retries against
//                        the refreshed tau.  Compaction: a wave per query ranks every entry by the total order (score descending,
//                        index ascending) -- each lane counts, over a broadcast walk of the list, the entries in front of its own
//                        two -- and writes rank r < k to slot r.  A store's address depends on every load of the walk, so the
//                        in-place permutation needs no second buffer.  The kept set is the k first of everything seen so far
//                        whatever the push order: the result is one array whatever the geometry.
//                        End of slab: one more compaction, then the sorted k (tail: -inf, -1) go to the workspace
//                        [nq][slabs][k], or with one slab straight to the outputs.
//   search_merge_kernel  a wave per query: lane l holds the heads of slab lists l, l + 64, .. (at most four: slabs <= 256), each
//                        round takes the best head of the wave under the same order (a butterfly over (score, index)) and
//                        advances its list.
// No global atomics, no work-queue counter, no scratch, no allocation: nothing but the arguments, safe beside a graph replay.
#include <limits.h>
#include <math.h>

#include "vh_kernels.h"

namespace vh {

namespace {

constexpr int kSrCap = 96;          // list entries per query: k <= 32 kept + at least 64 candidates
constexpr int kSrRound = 256;       // bank rows a workgroup takes per round: 4 waves x 2 tiles x 32 rows
constexpr int kSrMinSlab = 2048;    // no slab shorter than this
constexpr int kSrTargetWgs = 256;   // workgroups the split aims at (the CU count of the one device this library targets)

__device__ __forceinline__ bool sr_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

template <typename T>
__global__ void __launch_bounds__(256)
search_prep_kernel(const float* __restrict__ rows, int64_t row_stride, int nq, int nq_pad, int W, int normalise,
                   typename T::elem* __restrict__ q16) {
#pragma clang fp contract(off)
    using V4 = typename T::vec4;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), nchunk = W >> 2;
    if (row >= nq_pad) return;
    V4* const out = (V4*)(q16 + (int64_t)row * W);
    if (row >= nq) {
        for (int c = lane; c < nchunk; c += 64) out[c] = V4{};
        return;
    }
    const f32x4* const x = (const f32x4*)(rows + (int64_t)row * row_stride);
    float r = 1.f;
    if (normalise) {
        float s = 0.f;
        for (int c = lane; c < nchunk; c += 64) {
            const f32x4 v = x[c];
            const float a = v[0] * v[0], b = v[1] * v[1], cc = v[2] * v[2], d = v[3] * v[3];
            s += (a + b) + (cc + d);
        }
        s = wave_sum(s);
        if (s > 0.f) r = 1.0f / sqrtf(s);
    }
    for (int c = lane; c < nchunk; c += 64) {
        const f32x4 v = x[c];
        out[c] = pack4<T>(v[0] * r, v[1] * r, v[2] * r, v[3] * r);
    }
}

// the lists of a workgroup, behind the query image in its dynamic LDS
struct SrLists {
    uint2* list;   // [QL][kSrCap]: x = the score's bits, y = the bank row
    float* tau;    // [QL]: (tau, taui) = the k-th best entry at the last compaction; (-inf, INT_MAX) while fewer than k are kept
    int* taui;     // [QL]
    int* cnt;      // [QL]: entries appended since the last compaction on top of those kept; may run past kSrCap (failed appends)
};

// every wave: queries wave, wave + 4, ..  Between two workgroup barriers.
template <int QL>
__device__ __forceinline__ void sr_compact(const SrLists& S, int k, int wave, int lane) {
    for (int q = wave; q < QL; q += 4) {
        int c = __builtin_amdgcn_readfirstlane(S.cnt[q]);
        if (c == 0) continue;
        if (c > kSrCap) c = kSrCap;
        uint2* const L = S.list + q * kSrCap;
        const bool h0 = lane < c, h1 = lane + 64 < c;
        const uint2 e0 = h0 ? L[lane] : make_uint2(0u, 0u), e1 = h1 ? L[lane + 64] : make_uint2(0u, 0u);
        const float s0 = __uint_as_float(e0.x), s1 = __uint_as_float(e1.x);
        int r0 = 0, r1 = 0;
        for (int j = 0; j < c; ++j) {
            const uint2 o = L[j];
            const float so = __uint_as_float(o.x);
            r0 += sr_before(so, (int)o.y, s0, (int)e0.y) ? 1 : 0;
            r1 += sr_before(so, (int)o.y, s1, (int)e1.y) ? 1 : 0;
        }
        if (h0 && r0 < k) L[r0] = e0;
        if (h1 && r1 < k) L[r1] = e1;
        if (h0 && r0 == k - 1) { S.tau[q] = s0; S.taui[q] = (int)e0.y; }
        if (h1 && r1 == k - 1) { S.tau[q] = s1; S.taui[q] = (int)e1.y; }
        if (lane == 0) S.cnt[q] = c < k ? c : k;
    }
}

template <typename T, int QL>
__global__ void __launch_bounds__(256)
search_scan_kernel(const typename T::elem* __restrict__ q16, const typename T::elem* __restrict__ bank, int64_t n, int W, int nq, int k,
                   int64_t slab_len, int slabs, int qblocks, uint2* __restrict__ part, int32_t* __restrict__ index_out,
                   float* __restrict__ score_out) {
    using E = typename T::elem;
    using V8 = typename T::vec8;
    constexpr int NQS = QL >= 32 ? QL / 32 : 1;   // 32-query MFMA column blocks
    extern __shared__ __attribute__((aligned(16))) char sr_smem[];
    E* const Qs = (E*)sr_smem;
    SrLists S;
    S.list = (uint2*)(sr_smem + (size_t)QL * W * 2);
    S.tau = (float*)(S.list + QL * kSrCap);
    S.taui = (int*)(S.tau + QL);
    S.cnt = S.taui + QL;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, col = lane & 31;
    const int slab = blockIdx.x / qblocks, q0 = (blockIdx.x - slab * qblocks) * QL;
    const int64_t slab_begin = (int64_t)slab * slab_len;
    const int64_t slab_end = slab_begin + slab_len < n ? slab_begin + slab_len : n;
    const int W8 = W >> 3, steps = W >> 4;

    // the query block -> its LDS image [k / 8][query][8]; q16 holds whole blocks of 64 rows (zeros behind nq)
    for (int idx = t; idx < QL * W8; idx += 256) {
        const int q = idx / W8, k8 = idx - q * W8;
        *(V8*)(Qs + ((size_t)k8 * QL + q) * 8) = *(const V8*)(q16 + (int64_t)(q0 + q) * W + 8 * k8);
    }
    if (t < QL) { S.tau[t] = -INFINITY; S.taui[t] = INT_MAX; S.cnt[t] = 0; }
    __syncthreads();

    const bool col_live = QL >= 32 || col < 16;   // QL = 16: MFMA columns 16 .. 31 are zeros
    for (int64_t round0 = slab_begin; round0 < slab_end; round0 += kSrRound) {
        const int64_t base = round0 + wave * 64;
        f32x16 acc[2][NQS];
        uint64_t pend = 0;
        if (base < slab_end) {   // wave-uniform
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int s = 0; s < NQS; ++s)
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[i][s][j] = 0.f;
            const E* bp[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int64_t row = base + 32 * i + col;
                if (row > n - 1) row = n - 1;   // rows behind the bank read its last row; the selection drops them
                bp[i] = bank + row * W + 8 * half;
            }
            V8 fa[4][2] = {}, fb[4][2] = {};
            auto load4 = [&](V8 (&f)[4][2], int c) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * c + j < steps) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) f[j][i] = *(const V8*)(bp[i] + 16 * (4 * c + j));
                    }
            };
            auto mma4 = [&](const V8 (&f)[4][2], int c) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ks = 4 * c + j;
                    if (ks < steps) {
                        V8 b[NQS];
#pragma unroll
                        for (int s = 0; s < NQS; ++s) {
                            if constexpr (QL >= 32) b[s] = *(const V8*)(Qs + ((size_t)(2 * ks + half) * QL + 32 * s + col) * 8);
                            else b[s] = col_live ? *(const V8*)(Qs + ((size_t)(2 * ks + half) * QL + col) * 8) : V8{};
                        }
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int s = 0; s < NQS; ++s) acc[i][s] = T::mfma32(f[j][i], b[s], acc[i][s]);
                    }
                }
            };
            const int nch = (steps + 3) >> 2;
            load4(fa, 0);
            for (int c = 0; c < nch; c += 2) {
                if (c + 1 < nch) load4(fb, c + 1);
                mma4(fa, c);
                if (c + 1 < nch) {
                    if (c + 2 < nch) load4(fa, c + 2);
                    mma4(fb, c + 1);
                }
            }
            // the lane's values that pass tau: bit (i NQS + s) 16 + j
#pragma unroll
            for (int s = 0; s < NQS; ++s) {
                const int q = 32 * s + col;
                if (col_live && q0 + q < nq) {
                    const float tau = S.tau[q];
                    const int taui = S.taui[q];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const int64_t row = base + 32 * i + 8 * (j >> 2) + 4 * half + (j & 3);
                            if (row < slab_end && sr_before(acc[i][s][j], (int)row, tau, taui)) pend |= 1ull << ((i * NQS + s) * 16 + j);
                        }
                }
            }
        }
        for (;;) {
            if (pend) {
#pragma unroll
                for (int s = 0; s < NQS; ++s) {
                    const int q = 32 * s + col;   // (a lane with pending bits passed col_live and the nq bound)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if ((pend >> ((i * NQS + s) * 16)) & 0xFFFFull) {
                            const float tau = S.tau[q];
                            const int taui = S.taui[q];
#pragma unroll
                            for (int j = 0; j < 16; ++j) {
                                const uint64_t bit = 1ull << ((i * NQS + s) * 16 + j);
                                if (pend & bit) {
                                    const float v = acc[i][s][j];
                                    const int row = (int)(base + 32 * i + 8 * (j >> 2) + 4 * half + (j & 3));
                                    if (sr_before(v, row, tau, taui)) {
                                        const int slot = atomicAdd(&S.cnt[q], 1);
                                        if (slot < kSrCap) {
                                            S.list[q * kSrCap + slot] = make_uint2(__float_as_uint(v), (uint32_t)row);
                                            pend &= ~bit;
                                        }
                                    } else pend &= ~bit;
                                }
                            }
                        }
                    }
                }
            }
            if (!__syncthreads_or(pend != 0)) break;   // the round's barrier; nobody was turned away: on to the next round
            sr_compact<QL>(S, k, wave, lane);
            __syncthreads();
        }
    }
    sr_compact<QL>(S, k, wave, lane);
    __syncthreads();
    for (int idx = t; idx < QL * k; idx += 256) {
        const int q = idx / k, j = idx - q * k;
        if (q0 + q >= nq) continue;
        const bool has = j < S.cnt[q];
        const uint2 e = has ? S.list[q * kSrCap + j] : make_uint2(__float_as_uint(-INFINITY), 0xFFFFFFFFu);
        if (slabs == 1) {
            index_out[(int64_t)(q0 + q) * k + j] = (int32_t)e.y;
            score_out[(int64_t)(q0 + q) * k + j] = __uint_as_float(e.x);
        } else part[((int64_t)(q0 + q) * slabs + slab) * k + j] = e;
    }
}

__global__ void __launch_bounds__(256)
search_merge_kernel(const uint2* __restrict__ part, int nq, int slabs, int k, int32_t* __restrict__ index_out, float* __restrict__ score_out) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;   // whole waves
    const uint2* const P = part + (int64_t)q * slabs * k;
    int head[4] = {0, 0, 0, 0};
    for (int r = 0; r < k; ++r) {
        float bs = -INFINITY;
        int bi = INT_MAX, mu = -1;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int l = lane + 64 * u;
            if (l < slabs && head[u] < k) {
                const uint2 e = P[(int64_t)l * k + head[u]];
                if ((int)e.y >= 0 && sr_before(__uint_as_float(e.x), (int)e.y, bs, bi)) { bs = __uint_as_float(e.x); bi = (int)e.y; mu = u; }
            }
        }
        const int mine = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o);
            const int oi = __shfl_xor(bi, o);
            if (sr_before(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        const bool won = bi != INT_MAX && mine == bi;
#pragma unroll
        for (int u = 0; u < 4; ++u) head[u] += (won && u == mu) ? 1 : 0;
        if (lane == 0) {
            index_out[(int64_t)q * k + r] = bi == INT_MAX ? -1 : bi;
            score_out[(int64_t)q * k + r] = bi == INT_MAX ? -INFINITY : bs;
        }
    }
}

int sr_query_rows(int W) { return W <= 768 ? 64 : W <= 2048 ? 32 : 16; }
size_t sr_partial_bytes(int nq_pad, int slabs, int k) { return (((size_t)nq_pad * slabs * k * 8) + 255) & ~(size_t)255; }

template <typename T, int QL>
hipError_t search_scan_launch(const SearchArgs& a, const SearchPlan& p, const void* q16, uint2* part, hipStream_t s) {
    const size_t lds = (size_t)QL * a.width * 2 + (size_t)QL * kSrCap * 8 + (size_t)QL * 12;
    auto kern = search_scan_kernel<T, QL>;
    static LdsDone lds_done;   // per instantiation, per device
    if (hipError_t e = ensure_dynamic_lds((const void*)kern, lds, lds_done); e != hipSuccess) return e;
    const int qblocks = (a.nq + QL - 1) / QL;
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.slabs * qblocks)), dim3(256), lds, s, (const typename T::elem*)q16,
                       (const typename T::elem*)a.bank16, a.n, a.width, a.nq, a.k, p.slab_len, p.slabs, qblocks, part, a.index, a.score);
    return hipGetLastError();
}

}  // namespace

// the split, from n and nq alone: as many slabs as give kSrTargetWgs workgroups of 64 queries, none shorter than kSrMinSlab rows,
// each a multiple of the round
SearchPlan search_plan(int nq, int64_t n) {
    SearchPlan p;
    p.nq_pad = (nq + 63) / 64 * 64;
    const int64_t want = (kSrTargetWgs + p.nq_pad / 64 - 1) / (p.nq_pad / 64), most = (n + kSrMinSlab - 1) / kSrMinSlab;
    int64_t slabs = want < most ? want : most;
    if (slabs < 1) slabs = 1;
    p.slab_len = ((n + slabs - 1) / slabs + kSrRound - 1) / kSrRound * kSrRound;
    p.slabs = (int)((n + p.slab_len - 1) / p.slab_len);
    return p;
}

// partial lists [nq_pad][slabs][k] (score, index), then the queries' 16-bit image at the widest width
size_t search_workspace_bytes(int nq, int64_t n, int k) {
    if (nq < 1 || nq > VH_SEARCH_MAX_QUERIES || n < 1 || n > VH_SEARCH_MAX_ROWS || k < 1 || k > VH_SEARCH_MAX_K) return 0;
    const SearchPlan p = search_plan(nq, n);
    return sr_partial_bytes(p.nq_pad, p.slabs, k) + (size_t)p.nq_pad * VH_SEARCH_MAX_WIDTH * 2;
}

const char* search_check(const SearchArgs& a) {
    if (!a.rows) return "search: null query rows";
    if (!a.bank16) return "search: null bank";
    if (!a.workspace) return "search: null workspace";
    if (!a.index || !a.score) return "search: null output (index and score are both required)";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "search: dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.width < 16 || a.width > VH_SEARCH_MAX_WIDTH || a.width % 16) return "search: width is not a multiple of 16 in 16..4096";
    if (a.n < 1 || a.n > VH_SEARCH_MAX_ROWS) return "search: n is outside 1..2^28 bank rows";
    if (a.nq < 1 || a.nq > VH_SEARCH_MAX_QUERIES) return "search: nq is outside 1..4096 query rows";
    if (a.k < 1 || a.k > VH_SEARCH_MAX_K) return "search: k is outside 1..32";
    if (a.normalise != 0 && a.normalise != 1) return "search: normalise is not 0 or 1";
    if (a.row_stride < a.width || a.row_stride % 4) return "search: the query row stride is below the width or not a multiple of 4 floats";
    if (((uintptr_t)a.rows | (uintptr_t)a.bank16 | (uintptr_t)a.workspace | (uintptr_t)a.index | (uintptr_t)a.score) & 15)
        return "search: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_search(const SearchArgs& a, hipStream_t s) {
    const SearchPlan p = search_plan(a.nq, a.n);
    if (p.slabs > 256) return hipErrorInvalidValue;   // the merge holds four list heads per lane
    uint2* const part = (uint2*)a.workspace;
    void* const q16 = (char*)a.workspace + sr_partial_bytes(p.nq_pad, p.slabs, a.k);
    const int ql = sr_query_rows(a.width);
    return dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        hipLaunchKernelGGL((search_prep_kernel<T>), dim3((unsigned)(p.nq_pad / 4)), dim3(256), 0, s, a.rows, a.row_stride, a.nq, p.nq_pad,
                           a.width, a.normalise, (typename T::elem*)q16);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipError_t e = ql == 64 ? search_scan_launch<T, 64>(a, p, q16, part, s)
                     : ql == 32 ? search_scan_launch<T, 32>(a, p, q16, part, s)
                                : search_scan_launch<T, 16>(a, p, q16, part, s);
        if (e != hipSuccess || p.slabs == 1) return e;
        hipLaunchKernelGGL(search_merge_kernel, dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, part, a.nq, p.slabs, a.k, a.index, a.score);
        return hipGetLastError();
    });
}

}  // namespace vh
