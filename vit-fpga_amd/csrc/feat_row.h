// feat_row.h — the residual stream's rows as the feature kernels read them (kernels_features.hip, kernels_dense.hip): the three forms of
// a row, x = hi + lo, the LayerNorm element, and the three steps of one row in one wave.  ONE place, so that every kernel that
// normalises a row of the residual gives the bits of include/vithip.h "Token features".  Internal linkage: each file that includes
// this instantiates its own copies.
#pragma once
#include <type_traits>

#include "vh_kernels.h"

namespace vh {
namespace {

// ---- the three forms of a residual row ---------------------------------------------------------------------------------
template <typename T> struct InSplit16 { using hi_t = T; };   // T = BF16 / FP16: 16-bit hi plane + one scaled e4m3 byte (Lo8<T>)
struct InSplit8 {};                                           // e4m3 hi plane + bf16 lo plane (VH_DTYPE_FP8 contexts)
struct InF32 {};                                              // the fp32 array

typedef float f32x2 __attribute__((ext_vector_type(2)));

// N = 8 or 4 consecutive elements starting at element `e` (a multiple of N) -> fp32; x = hi + lo with ONE fp32 add (the
// lo byte's scale is a power of two: decoding it is exact)
template <typename IN, int N>
__device__ __forceinline__ void load_x(const void* __restrict__ hi, const void* __restrict__ lo, int64_t e, float* v) {
    static_assert(N == 8 || N == 4, "pieces of 8 or 4 elements");
    if constexpr (std::is_same<IN, InF32>::value) {
        const f32x4* p = (const f32x4*)((const float*)hi + e);
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f32x4 a = p[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = a[j];
        }
    } else if constexpr (std::is_same<IN, InSplit8>::value) {
        const uint32_t* hp = (const uint32_t*)((const uint8_t*)hi + e);
        uint32_t hw[N / 4];
        if constexpr (N == 8) { const u32x2 t = *(const u32x2*)hp; hw[0] = t[0]; hw[1] = t[1]; }
        else hw[0] = *hp;
        using lvec = typename std::conditional<N == 8, bf16x8, bf16x4>::type;
        const lvec l = *(const lvec*)((const __bf16*)lo + e);
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)hw[q], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)hw[q], true);
            v[4 * q + 0] = a[0] + (float)l[4 * q + 0];
            v[4 * q + 1] = a[1] + (float)l[4 * q + 1];
            v[4 * q + 2] = b[0] + (float)l[4 * q + 2];
            v[4 * q + 3] = b[1] + (float)l[4 * q + 3];
        }
    } else {
        using T = typename IN::hi_t;
        using hvec = typename std::conditional<N == 8, typename T::vec8, typename T::vec4>::type;
        const hvec h = *(const hvec*)((const typename T::elem*)hi + e);
        const uint32_t* lp = (const uint32_t*)((const uint8_t*)lo + e);
        uint32_t lw[N / 4];
        if constexpr (N == 8) { const u32x2 t = *(const u32x2*)lp; lw[0] = t[0]; lw[1] = t[1]; }
        else lw[0] = *lp;
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f32x4 l = lo8_unpack4<T>(lw[q]);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * q + j] = (float)h[4 * q + j] + l[j];
        }
    }
}

__device__ __forceinline__ float feat_norm(float x, float mean, float rstd, float g, float b) {
    return __builtin_fmaf((x - mean) * rstd, g, b);
}

// ---- one row in one wave: the three steps both row kernels are made of ---------------------------------------------------------
// Lane `lane` holds pieces lane, lane + 64, .. of the row (a piece = 8 consecutive elements); pieces beyond dim hold zeros.
template <typename IN, int CH>
__device__ __forceinline__ void row_load(const void* __restrict__ hi, const void* __restrict__ lo, int64_t row, int dim, int lane,
                                         float (&v)[CH][8]) {
    const int npiece = dim >> 3;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + 64 * i;
        if (c < npiece) load_x<IN, 8>(hi, lo, row * dim + 8 * c, v[i]);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
        }
    }
}

// (mean, rstd) of the row, two passes over the registers; the order of both sums depends on dim alone
template <int CH>
__device__ __forceinline__ void row_stats(const float (&v)[CH][8], int dim, int lane, float eps, float& mean, float& rstd) {
    const int npiece = dim >> 3;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i)
        sum += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    mean = sum / (float)dim;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (lane + 64 * i < npiece) {
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; q = __builtin_fmaf(d, d, q); }
            var += q;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o);
    rstd = 1.0f / sqrtf(var / (float)dim + eps);
}

// piece i of the row through feat_norm, in place
__device__ __forceinline__ void piece_norm(float (&p)[8], int c, float mean, float rstd, const float* __restrict__ gamma,
                                           const float* __restrict__ beta) {
    const f32x4 g0 = ((const f32x4*)gamma)[2 * c], g1 = ((const f32x4*)gamma)[2 * c + 1];
    const f32x4 b0 = ((const f32x4*)beta)[2 * c], b1 = ((const f32x4*)beta)[2 * c + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        p[j] = feat_norm(p[j], mean, rstd, g0[j], b0[j]);
        p[4 + j] = feat_norm(p[4 + j], mean, rstd, g1[j], b1[j]);
    }
}

}  // namespace
}  // namespace vh
