// kernels_swiglu_ln.hip — the gate pass of a SwiGLU MLP with its inner LayerNorm (vithip.h VH_FLAG_SUB_LN; EVA-02's scale_mlp):
//   h = LN_n(silu(g) * u) * w + b    behind fc1, in front of fc2.
//
// One pass over what fc1 left in memory, gu [rows][2 M] row-major (g = columns 0 .. M - 1, u = columns M .. 2 M - 1): every g and u is read
// once, every h written once; the statistics are taken from the fp32 products while they sit in registers.  No scratch buffer, no second
// global pass.  The LayerNorm runs over the model's TRUE gated width n <= M (columns n .. M - 1 are the converter's padding: not in the
// sums, written as +0; never read from the first whole chunk behind n on -- the columns that share n's 16-byte chunk are read and masked).
//   A WAVE owns a row.  Lane l holds the 16-byte chunks c = l + 64 i (i = 0 .. NCH - 1, NCH = ceil(M / 512) <= 8) of its row as 8 NCH fp32
//   products; a load instruction of the wave reads one contiguous 1 KiB of g or of u.  Sum and centred square sum: the lane walks its
//   chunks in ascending order (elements of a chunk in ascending order), then the xor butterfly (32, 16, ... 1) -- an order that depends on
//   M alone, so a row's bits do not depend on rows, grid, stream or replay.
//   row-major h [rows][M]:   4 waves per workgroup, grid-stride over rows; a store instruction of the wave writes one contiguous 1 KiB.
//   tiled h [rows / 16][M / 8][16][8] (fc2's ab_tiled operand layout): a wave-per-row lane would scatter its 16-byte pieces 256 B apart.
//                            A 1024-thread workgroup owns one 16-row block (wave r = row r).  Per phase i the 16 waves put their
//                            normalised chunks 64 i .. 64 i + 63 into an LDS tile [16][64 chunks] (row pitch 1040 B: the 16 lanes that
//                            read one chunk column later hit 16 different bank groups), one barrier, and thread t = 16 cb + r picks up
//                            chunk cb of row r: in memory the 64 blocks [16][8] of a phase are one contiguous 16 KiB, thread t's 16 bytes
//                            at 16 t, so a store instruction of a wave is again one contiguous 1 KiB.  Two tiles, used alternately by a
//                            phase counter that runs on across row blocks: a tile is rewritten two phases -- one barrier -- after it was
//                            read.  M / 8 is a multiple of 8, so a partly filled last phase switches whole pairs of waves off.
// w and b (fp32 [M]) are read by every row: 8 M bytes per row from the cache, none of it from memory after the first rows.
// Every index is 64-bit; both kernels walk their items in a grid-stride loop.  No allocation, no host state.
// ARITHMETIC (vithip.h, for bits): the products are swiglu8's operations (kernels_swiglu.hip), kept in fp32; contraction is off in this
// file, and the two fused operations of the contract are written as fma.
#include "vh_kernels.h"

#pragma clang fp contract(off)

namespace vh {

constexpr int kSubLnMaxWidth = 4096, kSubLnPitch = 1040;   // bytes between rows of an LDS tile: 64 chunks + one chunk of padding

// The lane index again, behind a statement hipcc cannot look through.  Everything a stage derives from the lane (chunk addresses, the masks
// of the partial chunk) is loop-invariant, and hipcc hoists all of it out of the grid-stride loop and keeps it for every stage: at M = 4096
// that is 60 mask pairs and 40 address pairs, and the kernel spills.  Each stage derives them from fresh(lane) where it needs them: a few
// VALU operations per row, no scratch.
__device__ __forceinline__ int fresh(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// A chunk is whole (live = n - 8 c >= 8), dead (live <= 0: its g and u are not read, its products are 0) or -- one chunk of a row, where n
// is no multiple of 8 -- partial (read whole; the columns >= n masked).  Only the partial chunk pays for per-column masks, under a branch of its own: masks of every chunk,
// kept for three uses, are 64 register pairs that hipcc spills.
// The lane's products p[i][j] of chunk c = lane + 64 i (0 for columns >= n) and their sum.
template <typename T, int NCH>
__device__ __forceinline__ float gated_products(const typename T::elem* __restrict__ gr, int M, int n, int lane, float (&p)[NCH][8]) {
    using vec8 = typename T::vec8;
    constexpr int G = 4;   // chunks loaded ahead of their arithmetic: 8 loads in flight, 32 registers of raw g and u beside the products
    float s = 0.f;
#pragma unroll
    for (int i0 = 0; i0 < NCH; i0 += G) {
        vec8 g[G], u[G];
#pragma unroll
        for (int k = 0; k < G && i0 + k < NCH; ++k) {
            const int c = lane + 64 * (i0 + k);
            if (c * 8 < n) {
                g[k] = *(const vec8*)(gr + c * 8);
                u[k] = *(const vec8*)(gr + M + c * 8);
            } else {
                g[k] = vec8{};
                u[k] = vec8{};
            }
        }
#pragma unroll
        for (int k = 0; k < G && i0 + k < NCH; ++k) {
            const int i = i0 + k, live = n - (lane + 64 * i) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {   // (a dead chunk: g = u = 0 gives (0 * 0.5) * 0 = +0)
                const float gf = (float)g[k][j], uf = (float)u[k][j];
                const float r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gf * -1.44269504088896341f));
                p[i][j] = (gf * r) * uf;
            }
            if (live > 0 && live < 8) {
#pragma unroll
                for (int j = 1; j < 8; ++j) p[i][j] = j < live ? p[i][j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += p[i][j];
        }
    }
    return s;
}

// (mean, rstd) of the row over its n columns: both sums through the butterfly, the squares centred
template <int NCH>
__device__ __forceinline__ void row_moments(const float (&p)[NCH][8], float lane_sum, int n, int lane, float eps, float& mean, float& rstd) {
    mean = wave_sum(lane_sum) / (float)n;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int live = n - (lane + 64 * i) * 8;
        if (live >= 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = p[i][j] - mean; q = __builtin_fmaf(d, d, q); }
        } else if (live > 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = p[i][j] - mean; q = j < live ? __builtin_fmaf(d, d, q) : q; }
        }
    }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)n + eps);
}

// chunk c of the output row: fma((p - mean) * rstd, w, b) rounded once; +0 in the columns >= n
template <typename T>
__device__ __forceinline__ typename T::vec8 normalised8(const float (&p)[8], int c, int n, float mean, float rstd, const float* __restrict__ w,
                                                        const float* __restrict__ b) {
    const int live = n - c * 8;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = 0.f;
    if (live > 0) {
        const f32x4 w0 = *(const f32x4*)(w + c * 8), w1 = *(const f32x4*)(w + c * 8 + 4);
        const f32x4 b0 = *(const f32x4*)(b + c * 8), b1 = *(const f32x4*)(b + c * 8 + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = __builtin_fmaf((p[j] - mean) * rstd, j < 4 ? w0[j & 3] : w1[j & 3], j < 4 ? b0[j & 3] : b1[j & 3]);
        if (live < 8) {
#pragma unroll
            for (int j = 1; j < 8; ++j) y[j] = j < live ? y[j] : 0.f;
        }
    }
    const typename T::vec4 lo = pack4<T>(y[0], y[1], y[2], y[3]), hi = pack4<T>(y[4], y[5], y[6], y[7]);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// row-major h: one wave per row, 4 rows per workgroup
template <typename T, int NCH>
__global__ void __launch_bounds__(256)
swiglu_ln_rows_kernel(const typename T::elem* __restrict__ gu, const float* __restrict__ w, const float* __restrict__ b,
                      typename T::elem* __restrict__ h, int64_t rows, int M, int n, float eps) {
    using vec8 = typename T::vec8;
    const int lane = threadIdx.x & 63, cpr = M >> 3;
    const int64_t step = (int64_t)gridDim.x * 4;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += step) {
        float p[NCH][8], mean, rstd;
        const float s = gated_products<T, NCH>(gu + row * 2 * M, M, n, fresh(lane), p);
        row_moments<NCH>(p, s, n, fresh(lane), eps, mean, rstd);
        typename T::elem* const hr = h + row * M;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = fresh(lane) + 64 * i;
            if (c < cpr) *(vec8*)(hr + c * 8) = normalised8<T>(p[i], c, n, mean, rstd, w, b);
        }
    }
}

// tiled h: one workgroup per 16-row block, wave r = row r; the normalised chunks turn through LDS (see the head of this file)
template <typename T, int NCH>
__global__ void __launch_bounds__(1024)
swiglu_ln_tiled_kernel(const typename T::elem* __restrict__ gu, const float* __restrict__ w, const float* __restrict__ b,
                       typename T::elem* __restrict__ h, int64_t row_blocks, int M, int n, float eps) {
    using vec8 = typename T::vec8;
    __shared__ __attribute__((aligned(16))) char tile[2][16 * kSubLnPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cpr = M >> 3;
    const int tr = threadIdx.x & 15, tcb = threadIdx.x >> 4;   // the store side: row tr of block 64 i + tcb
    unsigned phase = 0;
    for (int64_t rb = blockIdx.x; rb < row_blocks; rb += gridDim.x) {
        float p[NCH][8], mean, rstd;
        const float s = gated_products<T, NCH>(gu + (rb * 16 + wave) * 2 * M, M, n, fresh(lane), p);
        row_moments<NCH>(p, s, n, fresh(lane), eps, mean, rstd);
        typename T::elem* const hb = h + rb * 16 * M;   // this row block's M / 8 blocks [16][8]
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (64 * i < cpr) {   // (uniform: every wave of the workgroup takes the same phases)
                char* const t = tile[phase++ & 1];
                const int l = fresh(lane), c = l + 64 * i, cb = tcb + 64 * i;
                if (c < cpr) *(vec8*)(t + wave * kSubLnPitch + l * 16) = normalised8<T>(p[i], c, n, mean, rstd, w, b);
                __syncthreads();
                if (cb < cpr) *(vec8*)(hb + ((int64_t)cb * 16 + tr) * 8) = *(const vec8*)(t + tr * kSubLnPitch + tcb * 16);
            }
        }
    }
}

const char* swiglu_ln_check(const void* gu16, int dtype, int64_t rows, int mlp_dim, int width, const float* weight, const float* bias,
                            float eps, const void* h16, int out_tiled) {
    if (!gu16 || !h16) return "null gu16 or h16";
    if (!weight || !bias) return "null weight or bias";
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return "dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (rows <= 0 || rows > (4097ll << 20)) return "rows outside 1 .. 4097 * 2^20";
    if (mlp_dim <= 0 || mlp_dim % 64) return "mlp_dim must be a positive multiple of 64";
    if (mlp_dim > kSubLnMaxWidth) return "mlp_dim above 4096: a lane holds at most 64 products of its row";
    if (width < 1 || width > mlp_dim) return "width outside 1 .. mlp_dim";
    if (!(eps > 0.f) || !(eps < __builtin_inff())) return "eps must be positive and finite";
    if (out_tiled != 0 && out_tiled != 1) return "out_tiled must be 0 or 1";
    if (out_tiled && rows % 16) return "the tiled output needs rows to be a multiple of 16";
    if (((uintptr_t)gu16 | (uintptr_t)h16) & 15) return "gu16 and h16 must be 16-byte aligned";
    if (((uintptr_t)weight | (uintptr_t)bias) & 15) return "weight and bias must be 16-byte aligned";
    return nullptr;
}

namespace {
struct SubLnArgs {
    const void* gu16; const float *w, *b; void* h16;
    int64_t rows; int M, n; float eps; int out_tiled; hipStream_t s;
};
template <typename T, int NCH>
hipError_t launch_swiglu_ln_n(const SubLnArgs& a) {
    constexpr int64_t kMaxGrid = 1 << 24;   // beyond it the grid-stride loop takes over
    using elem = typename T::elem;
    if (a.out_tiled) {
        const int64_t blocks = a.rows / 16;
        hipLaunchKernelGGL((swiglu_ln_tiled_kernel<T, NCH>), dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(1024), 0, a.s,
                           (const elem*)a.gu16, a.w, a.b, (elem*)a.h16, blocks, a.M, a.n, a.eps);
    } else {
        const int64_t blocks = (a.rows + 3) / 4;
        hipLaunchKernelGGL((swiglu_ln_rows_kernel<T, NCH>), dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(256), 0, a.s,
                           (const elem*)a.gu16, a.w, a.b, (elem*)a.h16, a.rows, a.M, a.n, a.eps);
    }
    return hipGetLastError();
}
template <typename T>
hipError_t launch_swiglu_ln_t(const SubLnArgs& a) {
    switch ((a.M + 511) / 512) {   // chunks per lane
        case 1: return launch_swiglu_ln_n<T, 1>(a);
        case 2: return launch_swiglu_ln_n<T, 2>(a);
        case 3: return launch_swiglu_ln_n<T, 3>(a);
        case 4: return launch_swiglu_ln_n<T, 4>(a);
        case 5: return launch_swiglu_ln_n<T, 5>(a);
        case 6: return launch_swiglu_ln_n<T, 6>(a);
        case 7: return launch_swiglu_ln_n<T, 7>(a);
        case 8: return launch_swiglu_ln_n<T, 8>(a);
    }
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t launch_swiglu_ln(const void* gu16, int dtype, int64_t rows, int mlp_dim, int width, const float* weight, const float* bias, float eps,
                            void* h16, int out_tiled, hipStream_t s) {
    if (swiglu_ln_check(gu16, dtype, rows, mlp_dim, width, weight, bias, eps, h16, out_tiled)) return hipErrorInvalidValue;
    const SubLnArgs a{gu16, weight, bias, h16, rows, mlp_dim, width, eps, out_tiled, s};
    return dtype == VH_DTYPE_BF16 ? launch_swiglu_ln_t<BF16>(a) : launch_swiglu_ln_t<FP16>(a);
}

}  // namespace vh
