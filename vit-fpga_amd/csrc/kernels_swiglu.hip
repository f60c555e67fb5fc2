// kernels_swiglu.hip — the gate pass of a SwiGLU MLP (vithip.h VH_FLAG_SWIGLU): h = silu(g) * u behind fc1, in front of fc2.
//
// One pass over what fc1 left in memory, gu [rows][2 M] row-major (g = columns 0 .. M - 1, u = columns M .. 2 M - 1); both GEMMs stay as
// they are.  Memory-bound: 4 M bytes read and 2 M written per row, no reuse, no LDS, no scratch.  A lane owns 16-byte chunks (8 elements):
// one of g, the same one of u, one of h.  Every index is 64-bit (rows reaches 2^20 * 4097, 2 M reaches 2^17), and every kernel walks its
// items in a grid-stride loop, so the grid stays a 32-bit count at any size.
//   row-major h [rows][M]:  consecutive lanes take consecutive chunks of a row, then the next row: the g reads, the u reads and the h
//                           stores of a wave are each one contiguous 1 KiB run (M / 8 >= 8 chunks per row: whole 128 B lines per row).
//   tiled h [rows / 16][M / 8][16][8] (fc2's ab_tiled operand layout; what the activation epilogues write): a WAVE owns 16 rows x 8
//                           neighbouring chunks, a lane (r = lane & 15, cc = lane >> 4) the chunks cc and cc + 4 of row r.  A [16][8] block
//                           is the 16 lanes of one cc: 256 B, and the four blocks of one store instruction are neighbours: one contiguous
//                           1 KiB run per store.  On the read side the 16 rows are 4 M bytes apart, so a load instruction reads 64 B of each
//                           of 16 rows, and the lane's second chunk is the other half of the same 128 B line: the two g loads (and the two
//                           u loads) of a wave together fetch whole, aligned 128 B lines, issued back to back.  No LDS transpose: the
//                           alternative (row-major reads, a [16][64] tile turned in LDS) adds a barrier and two LDS passes to save nothing
//                           the cache line granularity does not already give.
// ARITHMETIC (vithip.h, for bits): g and u widened to fp32; r = rcp(1 + exp2(g * -log2(e))) on v_exp_f32 / v_rcp_f32; h = (g * r) * u in
// fp32; ONE rounding (RNE) to the element type.
#include "vh_kernels.h"

namespace vh {

template <typename T>
__device__ __forceinline__ typename T::vec8 swiglu8(typename T::vec8 g, typename T::vec8 u) {
    typename T::vec8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float gf = (float)g[j], uf = (float)u[j];
        const float r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gf * -1.44269504088896341f));
        h[j] = (typename T::elem)((gf * r) * uf);
    }
    return h;
}

// row-major h: item = one 16-byte chunk of h; cpr = M / 8 chunks per row
template <typename T>
__global__ void __launch_bounds__(256)
swiglu_rows_kernel(const typename T::elem* __restrict__ gu, typename T::elem* __restrict__ h, int64_t items, int cpr) {
    using vec8 = typename T::vec8;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += step) {
        const int64_t row = i / cpr;
        const int64_t c = i - row * cpr;
        const typename T::elem* const gp = gu + (row * 2 * cpr + c) * 8;
        const vec8 g = *(const vec8*)gp, u = *(const vec8*)(gp + (int64_t)cpr * 8);
        *(vec8*)(h + i * 8) = swiglu8<T>(g, u);
    }
}

// tiled h: unit = (16-row block rb, group cg of 8 chunks), one per wave; gpr = M / 64 groups per row block
template <typename T>
__global__ void __launch_bounds__(256)
swiglu_tiled_kernel(const typename T::elem* __restrict__ gu, typename T::elem* __restrict__ h, int64_t units, int gpr) {
    using vec8 = typename T::vec8;
    const int lane = threadIdx.x & 63, r = lane & 15, cc = lane >> 4;
    const int64_t step = (int64_t)gridDim.x * 4;
    const int64_t M = (int64_t)gpr * 64;
    for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < units; w += step) {
        const int64_t rb = w / gpr;
        const int64_t cg = w - rb * gpr;
        const typename T::elem* const gp = gu + (rb * 16 + r) * 2 * M + (cg * 8 + cc) * 8;
        const vec8 g0 = *(const vec8*)gp, g1 = *(const vec8*)(gp + 32);
        const vec8 u0 = *(const vec8*)(gp + M), u1 = *(const vec8*)(gp + M + 32);
        // block (rb, cb) starts at ((rb * (M / 8) + cb) * 16) * 8 elements; row r of it at + r * 8
        typename T::elem* const hp = h + ((rb * (M / 8) + cg * 8 + cc) * 16 + r) * 8;
        *(vec8*)hp = swiglu8<T>(g0, u0);
        *(vec8*)(hp + 4 * 128) = swiglu8<T>(g1, u1);
    }
}

const char* swiglu_check(const void* gu16, int dtype, int64_t rows, int mlp_dim, const void* h16, int out_tiled) {
    if (!gu16 || !h16) return "null pointer";
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return "dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (rows <= 0 || rows > (4097ll << 20)) return "rows outside 1 .. 4097 * 2^20";
    if (mlp_dim <= 0 || mlp_dim % 64 || mlp_dim > (1 << 16)) return "mlp_dim must be a multiple of 64, at most 2^16";
    if (out_tiled != 0 && out_tiled != 1) return "out_tiled must be 0 or 1";
    if (out_tiled && rows % 16) return "the tiled output needs rows to be a multiple of 16";
    if (((uintptr_t)gu16 | (uintptr_t)h16) & 15) return "gu16 and h16 must be 16-byte aligned";
    return nullptr;
}

template <typename T>
static hipError_t launch_swiglu_t(const void* gu16, int64_t rows, int mlp_dim, void* h16, int out_tiled, hipStream_t s) {
    constexpr int64_t kMaxGrid = 1 << 24;   // beyond it the grid-stride loop takes over
    if (out_tiled) {
        const int64_t units = rows / 16 * (mlp_dim / 64), blocks = (units + 3) / 4;
        hipLaunchKernelGGL(swiglu_tiled_kernel<T>, dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(256), 0, s,
                           (const typename T::elem*)gu16, (typename T::elem*)h16, units, mlp_dim / 64);
    } else {
        const int64_t items = rows * (mlp_dim / 8), blocks = (items + 255) / 256;
        hipLaunchKernelGGL(swiglu_rows_kernel<T>, dim3((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid)), dim3(256), 0, s,
                           (const typename T::elem*)gu16, (typename T::elem*)h16, items, mlp_dim / 8);
    }
    return hipGetLastError();
}

hipError_t launch_swiglu(const void* gu16, int dtype, int64_t rows, int mlp_dim, void* h16, int out_tiled, hipStream_t s) {
    if (swiglu_check(gu16, dtype, rows, mlp_dim, h16, out_tiled)) return hipErrorInvalidValue;
    return dtype == VH_DTYPE_BF16 ? launch_swiglu_t<BF16>(gu16, rows, mlp_dim, h16, out_tiled, s)
                                  : launch_swiglu_t<FP16>(gu16, rows, mlp_dim, h16, out_tiled, s);
}

}  // namespace vh
