// kernels_moments.hip — feature moments (gfx950): column sums and the second-moment matrix G = X^T X of 16-bit operand rows.
// Contract: include/vithip.h, "Feature moments"; DESIGN.md 4.34.
//
//   moments_list_kernel   one wave: the listed images that lie inside the last batch, in list order, packed to the front of `list`, and
//                         their number (ballot + popcount, 64 entries per round).  The context form only.
//   moments_kernel        a symmetric rank-R update with the ROW index contracted.  A workgroup of four waves owns ONE upper-triangle
//                         output tile (I <= J, 128 x 128, a tile = two column blocks of 64) and ONE row slab (MomentsPlan: a function
//                         of (R, W) alone, evaluated by the host for the grid and by every workgroup for its rows -- the context form
//                         learns R from the list kernel).  One step = 32 rows of up to four column blocks (I lo, I hi, J lo, J hi; a
//                         diagonal tile moves the first two only) in one slot of a three-slot LDS ring, 4 KiB per block, moved by
//                         LDS-DMA in pieces of 8 rows (1 KiB), a wave 2 or 4 pieces; the match's step loop: a counted vmcnt leaves the
//                         next step in flight, the ring barrier, the refill of the slot read two steps ago.  The LDS row image is the
//                         k-means update's: 16-byte chunk c of row r of a block at 128 r + 16 (c ^ 4 ((r >> 1) & 1)), the image the
//                         transposing read wants.  BOTH MFMA operands come from ds_read_b64_tr_b16: a fragment is 32 columns x 16
//                         rows, element e of a lane = row 16 ks + 8 (e / 4) + 4 (l >> 5) + e % 4 of the step, in both operands alike.
//                         Waves 2 x 2: wave (wi, wj) owns columns 64 wi .. of I against 64 wj .. of J, four v_mfma_f32_32x32x16
//                         accumulators; a lane's value e of accumulator (a, b) is G[64 wi + 32 a + 8 (e / 4) + 4 (l >> 5) + e % 4]
//                         [64 wj + 32 b + (l & 31)] of the tile.  A wave whose column block lies behind W, and wave (1, 0) of a
//                         diagonal tile (below the diagonal), moves its pieces and multiplies nothing.
//       gather            row r of the list form is patch r % NP of image list[r / NP]: the piece's first row is divided once
//                         (wave-uniform), eight list entries come by a scalar load, the lane picks its own.  No copy pass.
//       tail rows         the DMA clamps rows behind the last one to row R - 1 (real data); the J-side fragment of a step that
//                         reaches behind the slab's last row is zeroed BY INDEX, so those rows add exactly +0.
//       column sums       the waves (0, wj) of the diagonal tiles run two more MFMAs per group on an all-ones A operand against the same
//                         J-side fragments: sum[w] in the gram's own order (groups of 16 ascending from +0), row 0 of the result.
//       partials          fp32, to the workspace: tiles [slab][tile][128][128], sums [slab][W].
//   moments_merge_kernel  slabs ascending from +0, then the old value under `accumulate` (one addition), gram[i][j] and gram[j][i] from
//                         the same value for i <= j only; the sums likewise; count = (old +) R.
// No atomics on global memory, no scratch; the result depends on the rows, R and W alone.
#include "attn_common.h"
#include "vh_kernels.h"

namespace vh {

namespace {

constexpr int kMoRows = 32;                 // rows of a step
constexpr int kMoSlots = 3;                 // ring depth in steps
constexpr int kMoBlock = kMoRows * 128;     // bytes of a column block of a step
constexpr int kMoStep = 4 * kMoBlock;       // bytes of a slot
constexpr int kMoTile = 128 * 128;          // floats of a partial tile

// tile t of the row-major upper triangle of nb x nb -> (I, J), I <= J
__device__ __forceinline__ void mo_tile(int t, int nb, int& I, int& J) {
    I = 0;
    while (t >= nb - I) { t -= nb - I; ++I; }
    J = I + t;
}

__global__ void __launch_bounds__(64) moments_list_kernel(const int32_t* __restrict__ images, int n, int nimg, int32_t* __restrict__ list,
                                                          int32_t* __restrict__ nvalid) {
    const int lane = threadIdx.x;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int v = i < n ? images[i] : -1;
        const bool ok = (unsigned)v < (unsigned)nimg;
        const uint64_t m = __ballot(ok);
        if (ok) list[base + __popcll(m & ((1ull << lane) - 1))] = v;
        base += __popcll(m);
    }
    if (lane == 0) *nvalid = base;
}

template <typename T>
__global__ void __launch_bounds__(256)
moments_kernel(const typename T::elem* __restrict__ x16, const int32_t* __restrict__ list, const int32_t* __restrict__ nvalid, int rows_arg,
               int np, int W, int tiles, float* __restrict__ ws_sum, float* __restrict__ ws_tile) {
    using V4 = typename T::vec4;
    using V8 = typename T::vec8;
    extern __shared__ __attribute__((aligned(16))) char mo_smem[];
    const uint32_t lds0 = (uint32_t)(uintptr_t)mo_smem;
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hl = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), wi = wave >> 1, wj = wave & 1;
    const int R = list ? *nvalid * np : rows_arg;
    const MomentsPlan pl = moments_plan(R, W);
    const int slab = blockIdx.x / tiles, tile = blockIdx.x - slab * tiles;
    if (slab >= pl.slabs) return;   // workgroup-uniform: the grid is sized for the largest R the list can give
    int I, J;
    mo_tile(tile, pl.nb, I, J);
    const bool diag = I == J;
    const int ncb = W >> 6;
    const int row0 = slab * pl.slab_rows, rend = R < row0 + pl.slab_rows ? R : row0 + pl.slab_rows;
    const int nsteps = (rend - row0 + kMoRows - 1) / kMoRows, npw = diag ? 2 : 4;

    // step s into slot s % 3: piece g = wave + 4 i is rows 8 (g & 3) .. + 7 of column block g >> 2 (0, 1: I lo, hi; 2, 3: J lo, hi; a block
    // behind W is clamped to the last one and never multiplied).  Byte offsets from x16 stay below 2^32 (moments_check).
    auto issue = [&](int s) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of kept in registers across the loop
        const uint32_t slot = lds0 + (uint32_t)(s % kMoSlots) * kMoStep;
        const int rs = row0 + s * kMoRows;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= npw) break;   // wave-uniform
            const int g = wave + 4 * i, cb = g >> 2, rg = g & 3;
            int gcb = cb < 2 ? 2 * I + cb : 2 * J + cb - 2;
            gcb = gcb < ncb ? gcb : ncb - 1;
            const int q = ln >> 3, c = (ln & 7) ^ (((q >> 1) & 1) << 2);
            int rp = rs + 8 * rg, row = rp + q;
            rp = rp < R - 1 ? rp : R - 1;
            row = row < R - 1 ? row : R - 1;
            uint32_t srow = (uint32_t)row;
            if (list) {   // wave-uniform
                const uint32_t i0 = (uint32_t)rp / (uint32_t)np;
                uint32_t p = (uint32_t)rp - i0 * (uint32_t)np + (uint32_t)(row - rp);
                const int32_t* const lp = list + __builtin_amdgcn_readfirstlane(i0);
                int ent[8];   // eight entries by scalar loads (wave-uniform addresses; the list is padded by eight)
#pragma unroll
                for (int d = 0; d < 8; ++d) ent[d] = lp[d];
                int img = ent[0];
#pragma unroll
                for (int d = 1; d < 8; ++d)
                    if (p >= (uint32_t)np) { p -= (uint32_t)np; img = ent[d]; }
                srow = (uint32_t)img * (uint32_t)np + p;
            }
            const uint32_t off = (srow * (uint32_t)W + (uint32_t)(gcb * 64 + 8 * c)) * 2u;
            asm_lds_dma16((const void*)x16, off, slot + (uint32_t)g * 1024u);
        }
    };

    for (int s = 0; s < kMoSlots - 1 && s < nsteps; ++s) issue(s);

    // the transposing read of the k-means update: the lane's address inside a block, columns 0 .. 31 (db = 0) or 32 .. 63
    const int g4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int vlane = (4 * hl + tq) * 128 + (((16 * (g4 & 1) + 4 * tp) * 2) ^ (((tq >> 1) & 1) << 6));
    auto frag = [&](const char* blk, int ks, int db) {
        const char* const pa = blk + ks * 2048 + (vlane ^ (db << 6));
        const V4 a = T::tr_read(pa), c = T::tr_read(pa + 1024);
        return __builtin_shufflevector(a, c, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    const bool ex_i = 2 * I + wi < ncb, ex_j = 2 * J + wj < ncb;
    const bool active = ex_i && ex_j && !(diag && wi > wj);   // wave-uniform
    const bool sums = diag && wi == 0 && ex_j;
    const int blk_a = wi * kMoBlock, blk_b = ((diag ? 0 : 2) + wj) * kMoBlock;

    f32x16 acc[2][2], sacc[2];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        acc[0][0][j] = 0.f; acc[0][1][j] = 0.f; acc[1][0][j] = 0.f; acc[1][1][j] = 0.f;
        sacc[0][j] = 0.f; sacc[1][j] = 0.f;
    }
    V8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (typename T::elem)1.f;

    for (int s = 0; s < nsteps; ++s) {
        // this wave's pieces of step s have landed (step s + 1 may stay in flight), then everyone's; step s - 1 has been read
        wait_vm<8>(s + 1 < nsteps ? npw : 0);
        ring_barrier();
        if (s + kMoSlots - 1 < nsteps) issue(s + kMoSlots - 1);   // into step s - 1's slot
        if (!active) continue;
        const char* const st = mo_smem + (s % kMoSlots) * kMoStep;
        const int rs = row0 + s * kMoRows;
        const bool tail = rs + kMoRows > rend;   // wave-uniform: the slab's last step only
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const V8 a0 = frag(st + blk_a, ks, 0), a1 = frag(st + blk_a, ks, 1);
            V8 b0 = frag(st + blk_b, ks, 0), b1 = frag(st + blk_b, ks, 1);
            if (tail) {
                const int rb = rs + 16 * ks + 4 * hl;   // element e is row rb + 8 (e / 4) + e % 4
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (rb + 8 * (e >> 2) + (e & 3) >= rend) { b0[e] = (typename T::elem)0.f; b1[e] = (typename T::elem)0.f; }
            }
            acc[0][0] = T::mfma32(a0, b0, acc[0][0]);
            acc[0][1] = T::mfma32(a0, b1, acc[0][1]);
            acc[1][0] = T::mfma32(a1, b0, acc[1][0]);
            acc[1][1] = T::mfma32(a1, b1, acc[1][1]);
            if (sums) {
                sacc[0] = T::mfma32(ones, b0, sacc[0]);
                sacc[1] = T::mfma32(ones, b1, sacc[1]);
            }
        }
    }

    if (!active) return;
    float* const pt = ws_tile + ((int64_t)slab * tiles + tile) * kMoTile;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                pt[(64 * wi + 32 * a + 8 * (e >> 2) + 4 * hl + (e & 3)) * 128 + 64 * wj + 32 * b + l31] = acc[a][b][e];
    if (sums && hl == 0) {   // every row of the ones product is the column sum: row 0 lives in element 0 of lanes 0 .. 31
        float* const ps = ws_sum + (int64_t)slab * W + 128 * J + 64 * wj + l31;
        ps[0] = sacc[0][0];
        ps[32] = sacc[1][0];
    }
}

// blocks 0 .. 16 tiles - 1: 256 float4 of a tile each; the blocks behind them: 256 columns of the sums each, the first also the count
__global__ void __launch_bounds__(256)
moments_merge_kernel(const float* __restrict__ ws_sum, const float* __restrict__ ws_tile, const int32_t* __restrict__ nvalid, int rows_arg, int np,
                     int W, int tiles, int accumulate, float* sum, float* gram, int64_t* count) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    const int R = nvalid ? *nvalid * np : rows_arg;
    const MomentsPlan pl = moments_plan(R, W);
    const int tb = tiles * 16;
    if ((int)blockIdx.x >= tb) {
        const int w = ((int)blockIdx.x - tb) * 256 + t;
        if (w < W) {
            float v = 0.f;
            for (int s = 0; s < pl.slabs; ++s) v += ws_sum[(int64_t)s * W + w];
            if (accumulate) v += sum[w];
            sum[w] = v;
        }
        if ((int)blockIdx.x == tb && t == 0) *count = (accumulate ? *count : 0) + (int64_t)R;
        return;
    }
    const int tile = blockIdx.x >> 4, q = ((blockIdx.x & 15) << 8) + t;   // float4 q of the tile: row q / 32, columns 4 (q % 32) ..
    int I, J;
    mo_tile(tile, pl.nb, I, J);
    const int i = q >> 5, j4 = (q & 31) << 2, gi = 128 * I + i, gj0 = 128 * J + j4;
    if (gi >= W || gj0 >= W || gj0 + 3 < gi) return;   // W is a multiple of 64: a float4 is inside or outside as a whole
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < pl.slabs; ++s) v += ((const f32x4*)(ws_tile + ((int64_t)s * tiles + tile) * kMoTile))[q];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int gj = gj0 + e;
        if (gj < gi) continue;   // the upper triangle only: nobody reads or owns an element below the diagonal
        float x = v[e];
        if (accumulate) x += gram[(int64_t)gi * W + gj];
        gram[(int64_t)gi * W + gj] = x;
        gram[(int64_t)gj * W + gi] = x;
    }
}

}  // namespace

size_t moments_workspace_bytes(int64_t rows, int width) {
    const MomentsPlan pl = moments_plan(rows, width);
    return (size_t)pl.smax * ((size_t)width * 4 + (size_t)pl.tiles * kMoTile * 4);
}

const char* moments_check(const MomentsArgs& a) {
    if (!a.x16) return "moments: null rows";
    if (!a.sum || !a.gram || !a.count) return "moments: null output (sum, gram and count are all required)";
    if (!a.workspace) return "moments: null workspace";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "moments: dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.width < 64 || a.width > VH_MOMENTS_MAX_WIDTH || a.width % 64) return "moments: width is not a multiple of 64 in 64..2048";
    if (a.accumulate != 0 && a.accumulate != 1) return "moments: accumulate is not 0 or 1";
    if (a.list) {
        if (!a.nvalid || a.np < 1 || a.nimg < 1 || a.n < 1) return "moments: the image list needs its count, np, nimg and n";
        if ((int64_t)a.nimg * a.np * a.width * 2 > (int64_t)UINT32_MAX) return "moments: the operand rows exceed 4 GiB";
        if ((int64_t)a.n * a.np > INT32_MAX) return "moments: more than 2^31 - 1 rows";
    } else {
        if (a.rows < 1 || a.rows > INT32_MAX) return "moments: rows is outside 1..2^31-1";
        if (a.rows * a.width * 2 > (int64_t)UINT32_MAX) return "moments: the operand rows exceed 4 GiB";
    }
    if (((uintptr_t)a.x16 | (uintptr_t)a.list | (uintptr_t)a.nvalid | (uintptr_t)a.sum | (uintptr_t)a.gram | (uintptr_t)a.count | (uintptr_t)a.workspace) & 15)
        return "moments: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_moments_list(const int32_t* images, int n, int nimg, int32_t* list, int32_t* nvalid, hipStream_t s) {
    if (!images || !list || !nvalid || n < 1 || nimg < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(moments_list_kernel, dim3(1), dim3(64), 0, s, images, n, nimg, list, nvalid);
    return hipGetLastError();
}

hipError_t launch_moments(const MomentsArgs& a, hipStream_t s) {
    if (moments_check(a)) return hipErrorInvalidValue;
    const int64_t rmax = a.list ? (int64_t)a.n * a.np : a.rows;
    const MomentsPlan pl = moments_plan(rmax, a.width);
    float* const ws_sum = (float*)a.workspace;
    float* const ws_tile = ws_sum + (size_t)pl.smax * a.width;
    const int np = a.list ? a.np : 1;
    const hipError_t e = dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        const size_t lds = (size_t)kMoSlots * kMoStep;
        auto kern = moments_kernel<T>;
        static LdsDone lds_done;   // per instantiation, per device
        if (hipError_t e = ensure_dynamic_lds((const void*)kern, lds, lds_done); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)(pl.smax * pl.tiles)), dim3(256), lds, s, (const typename T::elem*)a.x16, a.list, a.nvalid,
                           (int)rmax, np, a.width, pl.tiles, ws_sum, ws_tile);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(moments_merge_kernel, dim3((unsigned)(pl.tiles * 16 + (a.width + 255) / 256)), dim3(256), 0, s, (const float*)ws_sum,
                       (const float*)ws_tile, a.list ? a.nvalid : nullptr, (int)rmax, np, a.width, pl.tiles, a.accumulate, a.sum, a.gram, a.count);
    return hipGetLastError();
}

}  // namespace vh
