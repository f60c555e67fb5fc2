// kernels_propagate.hip — label propagation (gfx950): for every patch row of a target image the k best patch rows among the patches of up
// to 8 source images, optionally inside a square window around the patch, and the softmax-weighted sum of those patches' label vectors.
// Contract: include/vithip.h, "Label propagation"; DESIGN.md 4.35.  The operand rows are the match's (kernels_match.hip, match_prep_kernel).
//
//   propagate_kernel    A workgroup of four waves owns one item (t, s_0 .. s_{S-1}) and 64 query rows of t.  It walks the present source
//                       slots in order, each slot's key tiles of 64 rows from the first to the last tile the window of the block admits
//                       (radius 0: all of them), and the width in chunks of 64 elements.  The operand movement is match_kernel's: one
//                       (tile, chunk) step = 64 query + 64 key rows of 128 bytes in one slot of a three-slot LDS ring, moved by LDS-DMA in
//                       pieces of 8 rows (1 KiB), four pieces per wave, under one counted vmcnt; 16-byte chunk c of row r sits at
//                       128 r + 16 (c ^ ((r >> 1) & 7)), the permutation on the lane's global source address.  Two cursors (issue, compute)
//                       step through (slot, tile, chunk); both are workgroup-uniform and live in scalar registers.
//                       Waves 2 x 2: wave w takes query rows 32 (w >> 1) .. and keys 32 (w & 1) .. of the tile, the keys as the MFMA A
//                       operand: the 16 accumulator values of a lane belong to ONE query (column l & 31) and keys 8 (j / 4) + 4 (l >> 5) +
//                       j % 4, ascending in j.
//   window              The admitted keys of a query block lie in the patch range [(qy_min - r) gw, (qy_max + r + 1) gw): tiles outside it
//                       are neither moved nor multiplied.  The exact |dy| <= r, |dx| <= r test and key < NP are applied per element BY
//                       INDEX when a tile's scores are complete (the rows behind NP replicate row NP - 1 and never enter).  key / gw is a
//                       multiply-high by ceil(2^32 / gw), exact for key * gw < 2^32.
//   running top-k       A lane keeps K (score, id) pairs sorted under (score descending, id ascending) in registers, K = 1, 4, 8 or 16 >=
//                       the caller's k.  A lane meets its ids in ascending order (slots, tiles, j), so a value enters only with a score
//                       strictly above the lane's K-th and lands behind every equal score; the insertion network runs under a wave-level
//                       any().  After the last tile the four lists of a query (two lane halves x two key waves) meet in LDS, in the ring's
//                       place, and every entry counts the entries in front of it under the same order (empty entries by position): ranks
//                       0 .. K - 1 are the final list.  The kept set is the first k of ALL candidates under the total order, whatever the
//                       tile geometry.
//   epilogue            A wave per query row: lane e holds entry e, its weight exp2((s_e - s_0) c) (v_exp_f32) and its label row; Z and the
//                       fused multiply-add chain run ascending in e over broadcast values, lanes spanning the classes (coalesced gathers),
//                       one correctly rounded division.  idx / score are the first k entries, tails -1 / -inf.
// No atomics, no scratch, no allocation, no counter; all per-item offsets are 64-bit; an item's result depends on its own rows, labels and
// parameters alone.
#include <limits.h>
#include <math.h>

#include "attn_common.h"
#include "vh_kernels.h"

namespace vh {

namespace {

constexpr int kPrQ = 64;        // query rows of a workgroup
constexpr int kPrKeys = 64;     // key rows of a tile
constexpr int kPrChunk = 64;    // elements of the width per ring step: 128 bytes of a row
constexpr int kPrSlots = 3;     // ring depth in steps
constexpr int kPrRows = kPrQ + kPrKeys, kPrStep = kPrRows * 128, kPrPerWave = kPrRows / 8 / 4;
constexpr int kPrRing = kPrSlots * kPrStep;

// (slot, tile, chunk) of a step; workgroup-uniform
struct PrCursor { int sigma, img, kt, kc; };

__device__ __forceinline__ int pr_next_slot(const int32_t* src, int from, int S) {
    while (from < S && src[from] < 0) ++from;
    return from;
}
__device__ __forceinline__ void pr_advance(PrCursor& c, const int32_t* src, int S, int t0, int t1, int nkc) {
    if (++c.kc < nkc) return;
    c.kc = 0;
    if (++c.kt <= t1) return;
    c.kt = t0;
    c.sigma = pr_next_slot(src, c.sigma + 1, S);
    c.img = c.sigma < S ? src[c.sigma] : 0;
}

// labels and out carry no __restrict__: out may be a slot of the label array that is no source of the call (vithip.h)
template <typename T, int K>
__global__ void __launch_bounds__(256)
propagate_kernel(const typename T::elem* __restrict__ rows16, const int32_t* __restrict__ items, int images, int np, int gw, int W,
                 int qblocks, int S, int kk, int radius, uint32_t gw_magic, float c2, const float* labels, int C, float* out,
                 int32_t* __restrict__ idx, float* __restrict__ score) {
#pragma clang fp contract(off)
    using E = typename T::elem;
    using V8 = typename T::vec8;
    extern __shared__ __attribute__((aligned(16))) char pr_smem[];
    uint2* const lists = (uint2*)pr_smem;               // [4 K][64] after the last step, in the ring's place: x = the score's bits, y = the id
    uint2* const fin = (uint2*)(pr_smem + kPrRing);     // [64][K], sorted
    const uint32_t lds0 = (uint32_t)(uintptr_t)pr_smem;
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hl = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wq = wave >> 1, wk = wave & 1;
    const int item = blockIdx.x / qblocks, q0 = (blockIdx.x - item * qblocks) * kPrQ;
    const int32_t* const it = items + (int64_t)item * (S + 1);
    const int32_t* const src = it + 1;
    const int64_t obase = (int64_t)item * np + q0;

    // an image outside 0 .. images - 1 (device items only): the item is marked and nothing is read for it.  Workgroup-uniform.
    const int ti = it[0];
    bool known = (unsigned)ti < (unsigned)images;
    int npresent = 0;
    for (int s = 0; s < S; ++s) {
        const int v = src[s];
        if (v >= 0) { ++npresent; known = known && v < images; }
    }
    if (!known) {
        for (int i = t; i < kPrQ * kk; i += 256) {
            const int r = i / kk;
            if (q0 + r < np) {
                if (idx) idx[(obase + r) * kk + (i - r * kk)] = -1;
                if (score) score[(obase + r) * kk + (i - r * kk)] = -INFINITY;
            }
        }
        for (int i = t; i < kPrQ * C; i += 256) {
            const int r = i / C;
            if (q0 + r < np) out[(obase + r) * C + (i - r * C)] = 0.f;
        }
        return;
    }

    // the tile range the block's window admits
    int t0 = 0, t1 = (np - 1) / kPrKeys;
    if (radius > 0) {
        const int qlast = q0 + kPrQ - 1 < np - 1 ? q0 + kPrQ - 1 : np - 1, gh = np / gw;
        const int ylo = q0 / gw - radius, yhi = qlast / gw + radius + 1;
        const int lo = (ylo > 0 ? ylo : 0) * gw, hi = (yhi < gh ? yhi : gh) * gw;
        t0 = lo / kPrKeys;
        t1 = (hi - 1) / kPrKeys;
    }
    const int nkc = W / kPrChunk, nsteps = npresent * (t1 - t0 + 1) * nkc;
    const E* const A = rows16 + (int64_t)ti * np * W;

    // step c into ring slot `ring`: pieces g = wave, wave + 4, .. of 8 rows; rows 0 .. 63 of a step are the query block, the rest the key
    // tile.  Lane ln of a piece lands at 16 ln: row 8 g + (ln >> 3), physical chunk ln & 7.  Rows are clamped to NP - 1: nothing outside the
    // two images is read.  Byte offsets from A / B stay below 2^32: row < 4096, W <= 2048.
    auto issue = [&](const PrCursor& c, int ring) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of kept in registers across the loop
        const E* const B = rows16 + (int64_t)c.img * np * W;
        const uint32_t slot = lds0 + (uint32_t)ring * kPrStep;
#pragma unroll
        for (int i = 0; i < kPrPerWave; ++i) {
            const int g = wave + 4 * i, r = 8 * g + (ln >> 3);
            const int ch = (ln & 7) ^ ((r >> 1) & 7);
            const bool is_q = g < kPrQ / 8;   // wave-uniform
            int row = is_q ? q0 + r : c.kt * kPrKeys + (r - kPrQ);
            row = row < np - 1 ? row : np - 1;
            const uint32_t off = ((uint32_t)row * (uint32_t)W + (uint32_t)(c.kc * kPrChunk + 8 * ch)) * 2u;
            asm_lds_dma16(is_q ? (const void*)A : (const void*)B, off, slot + (uint32_t)g * 1024u);
        }
    };

    PrCursor cur, nxt;
    cur.sigma = pr_next_slot(src, 0, S);
    cur.img = cur.sigma < S ? src[cur.sigma] : 0;
    cur.kt = t0;
    cur.kc = 0;
    nxt = cur;
    for (int s = 0; s < kPrSlots - 1 && s < nsteps; ++s) {
        issue(nxt, s);
        pr_advance(nxt, src, S, t0, t1, nkc);
    }

    // this lane's operand rows in a step and their swizzles; its query and the query's place in the grid
    const int krow = kPrQ + 32 * wk + l31, kswz = (krow >> 1) & 7;
    const int qrow = 32 * wq + l31, qswz = (qrow >> 1) & 7;
    const int qy = (q0 + qrow) / gw, qx = (q0 + qrow) - qy * gw;

    f32x16 acc;
    float ls[K];
    int li[K];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll
    for (int p = 0; p < K; ++p) { ls[p] = -INFINITY; li[p] = INT_MAX; }

    for (int s = 0; s < nsteps; ++s) {
        // this wave's pieces of step s have landed (step s + 1 may stay in flight), then everyone's; step s - 1 has been read
        wait_vm<8>(s + 1 < nsteps ? kPrPerWave : 0);
        ring_barrier();
        if (s + kPrSlots - 1 < nsteps) {   // into step s - 1's slot
            issue(nxt, (s + kPrSlots - 1) % kPrSlots);
            pr_advance(nxt, src, S, t0, t1, nkc);
        }
        const char* const st = pr_smem + (s % kPrSlots) * kPrStep;
#pragma unroll
        for (int ks = 0; ks < kPrChunk / 16; ++ks) {
            const int ch = 2 * ks + hl;
            const V8 kf = *(const V8*)(st + krow * 128 + ((ch ^ kswz) << 4));
            const V8 qf = *(const V8*)(st + qrow * 128 + ((ch ^ qswz) << 4));
            acc = T::mfma32(kf, qf, acc);
        }
        if (cur.kc == nkc - 1) {   // the tile's scores are complete: push the admitted ones, ids ascending
            const int key0 = cur.kt * kPrKeys + 32 * wk + 4 * hl, g0 = cur.sigma * np;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int key = key0 + 8 * (j >> 2) + (j & 3);
                bool ok = key < np;
                if (radius > 0) {   // workgroup-uniform
                    const int jy = gw_magic ? (int)__umulhi((uint32_t)key, gw_magic) : key, jx = key - jy * gw;
                    const int dy = jy - qy, dx = jx - qx;
                    ok = ok && dy <= radius && -dy <= radius && dx <= radius && -dx <= radius;
                }
                const float v = ok ? acc[j] : -INFINITY;
                acc[j] = 0.f;
                if (__any(v > ls[K - 1])) {
                    const int g = g0 + key;
#pragma unroll
                    for (int p = K - 1; p > 0; --p) {
                        const bool up = v > ls[p - 1], here = v > ls[p];
                        li[p] = up ? li[p - 1] : (here ? g : li[p]);
                        ls[p] = up ? ls[p - 1] : (here ? v : ls[p]);
                    }
                    const bool first = v > ls[0];
                    li[0] = first ? g : li[0];
                    ls[0] = first ? v : ls[0];
                }
            }
        }
        pr_advance(cur, src, S, t0, t1, nkc);
    }

    // the four lists of a query meet in the ring's place (every DMA has landed: the last wait was vmcnt(0)); entry p of list c of query q
    // sits at [(c K + p)][q]
    __syncthreads();
#pragma unroll
    for (int p = 0; p < K; ++p) lists[((2 * wk + hl) * K + p) * kPrQ + qrow] = make_uint2(__float_as_uint(ls[p]), (uint32_t)li[p]);
    __syncthreads();
    {
        // thread (q, w) ranks entries w, w + 4, .. of query q among all 4 K: rank = the number of entries in front under (score
        // descending, id ascending); ids are unique but for the empty entries (-inf, INT_MAX), which go by position
        const int q = t & 63, w = t >> 6;
        float os[K];
        int oi[K], rank[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const uint2 e = lists[(w + 4 * i) * kPrQ + q];
            os[i] = __uint_as_float(e.x);
            oi[i] = (int)e.y;
            rank[i] = 0;
        }
        for (int p = 0; p < 4 * K; ++p) {
            const uint2 e = lists[p * kPrQ + q];
            const float es = __uint_as_float(e.x);
            const int ei = (int)e.y;
#pragma unroll
            for (int i = 0; i < K; ++i)
                rank[i] += es > os[i] || (es == os[i] && (ei < oi[i] || (ei == oi[i] && p < w + 4 * i))) ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (rank[i] < K) fin[q * K + rank[i]] = make_uint2(__float_as_uint(os[i]), (uint32_t)oi[i]);
    }
    __syncthreads();

    // a wave per query row; lane e holds entry e of the final list
    for (int r = wave; r < kPrQ; r += 4) {
        if (q0 + r >= np) break;   // wave-uniform
        uint2 e = make_uint2(__float_as_uint(-INFINITY), (uint32_t)INT_MAX);
        if (lane < K) e = fin[r * K + lane];
        const bool valid = lane < kk && (int)e.y != INT_MAX;
        const int cnt = __builtin_amdgcn_readfirstlane(__popcll(__ballot(valid)));   // the valid entries are a prefix: the list is sorted
        const float sc = __uint_as_float(e.x);
        const int g = (int)e.y;
        int img = 0, j = 0;
        if (valid) {
            const int sg = g / np;
            j = g - sg * np;
            img = src[sg];
        }
        const int64_t orow = obase + r;
        if (lane < kk) {
            if (idx) idx[orow * kk + lane] = valid ? g : -1;
            if (score) score[orow * kk + lane] = valid ? sc : -INFINITY;
        }
        const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), 0));
        const float wgt = valid ? __builtin_amdgcn_exp2f((sc - s0) * c2) : 0.f;
        float z = 0.f, a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int en = 0; en < K; ++en) {
            if (en < cnt) {   // wave-uniform
                const float we = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wgt), en));
                const int ie = __builtin_amdgcn_readlane(img, en), je = __builtin_amdgcn_readlane(j, en);
                const float* const lr = labels + ((int64_t)ie * np + je) * C;
                z = en ? z + we : we;
#pragma unroll
                for (int ci = 0; ci < 4; ++ci)
                    if (lane + 64 * ci < C) a[ci] = fmaf(we, lr[lane + 64 * ci], a[ci]);
            }
        }
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
            if (lane + 64 * ci < C) out[orow * C + lane + 64 * ci] = cnt ? a[ci] / z : 0.f;
    }
}

template <typename T, int K>
hipError_t propagate_launch(const PropagateArgs& a, hipStream_t s) {
    const size_t lds = (size_t)kPrRing + (size_t)kPrQ * K * 8;
    static_assert(4 * K * kPrQ * 8 <= kPrRing, "the four lists of every query fit in the ring's place");
    auto kern = propagate_kernel<T, K>;
    static LdsDone lds_done;   // per instantiation, per device
    if (hipError_t e = ensure_dynamic_lds((const void*)kern, lds, lds_done); e != hipSuccess) return e;
    const int np = a.gh * a.gw, qblocks = (np + kPrQ - 1) / kPrQ;
    const uint32_t magic = a.gw > 1 ? (uint32_t)(0x100000000ull / (uint32_t)a.gw) + 1u : 0u;   // key / gw = umulhi(key, magic); gw 1: key
    const float c2 = (float)(1.4426950408889634 / (double)a.tau);                              // log2(e) / tau
    hipLaunchKernelGGL(kern, dim3((unsigned)a.nitems * (unsigned)qblocks), dim3(256), lds, s, (const typename T::elem*)a.rows16, a.items,
                       a.images, np, a.gw, a.width, qblocks, a.nsrc, a.k, a.radius, magic, c2, a.labels, a.classes, a.out, a.idx, a.score);
    return hipGetLastError();
}

}  // namespace

const char* propagate_check(const PropagateArgs& a) {
    if (!a.rows16) return "propagate: null rows";
    if (!a.items) return "propagate: null item list";
    if (!a.labels || !a.out) return "propagate: null labels or out (idx and score may be null)";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "propagate: dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.images < 1 || a.images > (1 << 20)) return "propagate: images is outside 1..2^20";
    if (a.gh < 1 || a.gw < 1 || (int64_t)a.gh * a.gw > VH_MATCH_MAX_ROWS) return "propagate: gh or gw is below 1, or gh * gw is above 4096 patches";
    if (a.width < 64 || a.width > VH_MATCH_MAX_WIDTH || a.width % 64) return "propagate: width is not a multiple of 64 in 64..2048";
    if (a.nitems < 1 || a.nitems > VH_MATCH_MAX_PAIRS) return "propagate: nitems is outside 1..65536";
    if (a.nsrc < 1 || a.nsrc > VH_PROP_MAX_SOURCES) return "propagate: nsrc is outside 1..8";
    if (a.k < 1 || a.k > VH_PROP_MAX_K) return "propagate: k is outside 1..16";
    if (a.radius < 0 || a.radius > 4096) return "propagate: radius is outside 0..4096";
    if (!(a.tau > 0.f) || !isfinite(a.tau)) return "propagate: tau is not finite and positive";
    if (a.classes < 1 || a.classes > VH_PROP_MAX_CLASSES) return "propagate: classes is outside 1..256";
    if (((uintptr_t)a.rows16 | (uintptr_t)a.items | (uintptr_t)a.labels | (uintptr_t)a.out | (uintptr_t)a.idx | (uintptr_t)a.score) & 15)
        return "propagate: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_propagate(const PropagateArgs& a, hipStream_t s) {
    if (propagate_check(a)) return hipErrorInvalidValue;
    return dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        if (a.k == 1) return propagate_launch<T, 1>(a, s);
        if (a.k <= 4) return propagate_launch<T, 4>(a, s);
        if (a.k <= 8) return propagate_launch<T, 8>(a, s);
        return propagate_launch<T, 16>(a, s);
    });
}

}  // namespace vh
