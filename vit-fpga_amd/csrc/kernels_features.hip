// kernels_features.hip — token features of the residual stream a forward left in HBM (gfx950): the rows as they are or
// through the model's final LayerNorm, written in the caller's element type, and the mean over the patch tokens.
// Contract: include/vithip.h, "Token features"; DESIGN.md 4.19.
//
//   feat_rows_kernel   one wave per row, four rows per workgroup.  The row's planes are read ONCE, 8 elements per lane and
//                      piece (16-bit split path: 16 B of the hi plane + 8 B of the lo plane; fp8 split path: 8 B of e4m3 +
//                      16 B of bf16; plain path: two 16-byte fp32 loads), the row stays in registers between the two
//                      statistic passes, and each lane stores 16 bytes (fp32 results: two such stores).
//   feat_mean_kernel   one thread per image and FOUR neighbouring columns, walking the patch tokens in ascending order: the
//                      serial fp32 chain the contract names, independent of any launch geometry.  It reads the planes
//                      again (coalesced across columns) and takes (mean, rstd) of a row from the statistics the row kernel
//                      wrote, so the value it adds is, bit for bit, the fp32 value the row kernel converted and stored.
//   feat_nchw_kernel   the patch rows channels-first ([batch][dim][np]): 32 tokens of one image per workgroup, each row through the
//                      row kernel's own three steps (row_load, row_stats, piece_norm), transposed through LDS.
//   pool_rows_kernel   the same mean in ONE pass over the planes, inside the forward of a VH_FLAG_POOL context: one workgroup per
//                      image, a row per wave through the row kernel's steps, the rows of a group added from LDS in token order.
//   map_pool_kernel    the softmax-weighted sums of the attention-pooling head (VH_FLAG_MAP_HEAD) in the same ONE pass: the pool
//                      kernel's skeleton with the rows' scores against the folded query and an online softmax per group.
//   feat_capture_kernel  the copy of a tapped layer's rows into the capture store ("Layer features"), both planes in one launch.
// (The normalised class-token rows of the final state are the ones the head multiplied: a conversion copy of clsn32, made by launch_cast.)
//
// The arithmetic that both kernels must agree on lives in ONE place each: load_x (x = hi + lo, one fp32 add) and
// feat_norm (fmaf((x - mean) * rstd, gamma, beta), explicit fmaf).  The row sums use explicit operations in an order that
// depends on dim alone: per lane the pieces ascending (inside a piece a fixed tree), then the xor butterfly over the wave.
#include <cstdio>
#include <cstring>
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

// ---- the three element types of a result: F32OUT, FP16, BF16 (vh_common.h); 16-bit results round to nearest even ---------
template <typename OUT>
__device__ __forceinline__ void store4(typename OUT::elem* p, const float* v) {
    *(typename OUT::vec4*)p = pack4<OUT>(v[0], v[1], v[2], v[3]);
}
template <typename OUT>
__device__ __forceinline__ void store8(typename OUT::elem* p, const float* v) {
    if constexpr (std::is_same<OUT, F32OUT>::value) {
        ((f32x4*)p)[0] = f32x4{v[0], v[1], v[2], v[3]};
        ((f32x4*)p)[1] = f32x4{v[4], v[5], v[6], v[7]};
    } else {
        const typename OUT::vec4 a = pack4<OUT>(v[0], v[1], v[2], v[3]), b = pack4<OUT>(v[4], v[5], v[6], v[7]);
        *(typename OUT::vec8*)p = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
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

// rows = batch * tokens.  Row r = image r / tokens, token r % tokens: token 0 goes to cls_out [batch][dim], tokens 1 .. lead - 1
// (register tokens) to reg_out [batch][lead - 1][dim], token t >= lead to patch_out [batch][tokens - lead][dim]; any may be null.
// norm != 0: the row passes LayerNorm(gamma, beta, eps), and stats (optional) receives (mean, rstd) of every patch row.  A wave
// whose row has nothing to write leaves at once.  ncls = 1; 0 for the rows of a context without a class token (FeatureArgs::no_cls):
// tokens 0 .. lead - 1 are then all register rows, reg_out [batch][lead][dim], and lead may be 0.
template <typename IN, typename OUT, int CH>   // CH = pieces of 8 elements per lane (dim <= 512 * CH)
__global__ void __launch_bounds__(256)
feat_rows_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int64_t rows, int tokens, int lead, int ncls, int dim,
                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int norm,
                 typename OUT::elem* __restrict__ cls_out, typename OUT::elem* __restrict__ reg_out,
                 typename OUT::elem* __restrict__ patch_out, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t img = row / tokens;
    const int t = (int)(row - img * tokens);
    typename OUT::elem* out = nullptr;
    if (t < ncls) { if (cls_out) out = cls_out + img * dim; }
    else if (t < lead) { if (reg_out) out = reg_out + (img * (lead - ncls) + (t - ncls)) * dim; }
    else if (patch_out) out = patch_out + (img * (tokens - lead) + (t - lead)) * dim;
    const bool want_stats = norm && stats && t >= lead;
    if (!out && !want_stats) return;   // wave-uniform
    const int npiece = dim >> 3;
    float v[CH][8];
    row_load<IN, CH>(hi, lo, row, dim, lane, v);
    float mean = 0.f, rstd = 1.f;
    if (norm) {
        row_stats<CH>(v, dim, lane, eps, mean, rstd);
        if (want_stats && lane == 0) *(f32x2*)(stats + 2 * row) = f32x2{mean, rstd};
    }
    if (!out) return;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = lane + 64 * i;
        if (c < npiece) {
            if (norm) piece_norm(v[i], c, mean, rstd, gamma, beta);
            store8<OUT>(out + 8 * c, v[i]);
        }
    }
}

// The patch rows channels-first: out[b][k][p] = v of row b * tokens + lead + p, element k -- [batch][dim][np], np = tokens - lead,
// the map a convolutional head takes.  One workgroup (16 waves) takes kNchwTile consecutive patch tokens of one image and all dim
// columns; a wave takes two of the rows, one after the other through the steps of feat_rows_kernel, and keeps both in registers.
// Then half a chunk of 512 columns at a time (elements 4 h .. 4 h + 3 of the pieces i of every lane: 256 columns) passes through
// LDS: a wave writes element 4 h + j of its piece at [row][64 j + lane] (row stride 257 dwords: conflict-free dword stores), the
// workgroup reads it back with the token index fastest across lanes ([p][..] at p * 257: 32 lanes, 32 banks) and stores runs of 32
// consecutive p per channel.  33 KB of LDS: two workgroups (32 waves) per CU.  An output row is np elements long and np *
// sizeof(elem) is no multiple of anything in particular: element stores, only `out` itself is aligned.  stats as in
// feat_rows_kernel.  Tokens beyond np (the ragged last tile) are neither read nor written.
constexpr int kNchwTile = 32, kNchwStride = 257;
template <typename IN, typename OUT, int CH>
__global__ void __launch_bounds__(1024)
feat_nchw_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int tokens, int lead, int dim,
                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int norm,
                 typename OUT::elem* __restrict__ out, float* __restrict__ stats) {
    __shared__ float tile[kNchwTile * kNchwStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int np = tokens - lead, npiece = dim >> 3;
    const int tiles = (np + kNchwTile - 1) / kNchwTile;   // workgroup blockIdx.x = image * tiles + tile
    const int64_t img = blockIdx.x / tiles;
    const int p0 = (int)(blockIdx.x - img * tiles) * kNchwTile;
    float v[2][CH][8];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int p = p0 + wave + 16 * q;
        if (p < np) {   // wave-uniform
            const int64_t row = img * tokens + lead + p;
            row_load<IN, CH>(hi, lo, row, dim, lane, v[q]);
            if (norm) {
                float mean, rstd;
                row_stats<CH>(v[q], dim, lane, eps, mean, rstd);
                if (stats && lane == 0) *(f32x2*)(stats + 2 * row) = f32x2{mean, rstd};
#pragma unroll
                for (int i = 0; i < CH; ++i)
                    if (lane + 64 * i < npiece) piece_norm(v[q][i], lane + 64 * i, mean, rstd, gamma, beta);
            }
        }
    }
    // the read side: token pl of the tile; positions ks, ks + 32, .. of the 256 of a half chunk.  Position kk holds element
    // 4 h + (kk >> 6) of the piece of lane kk & 63: column 512 i + 8 (kk & 63) + 4 h + (kk >> 6)
    const int pl = threadIdx.x & 31, ks = threadIdx.x >> 5;
    const bool p_ok = p0 + pl < np;
    typename OUT::elem* const obase = out + (img * dim) * np + p0 + pl;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (i || h) __syncthreads();   // the previous half chunk has been read
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (p0 + wave + 16 * q < np && lane + 64 * i < npiece) {
                    float* const w = tile + (wave + 16 * q) * kNchwStride + lane;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[64 * j] = v[q][i][4 * h + j];
                }
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int kk = ks + 32 * m;
                if (p_ok && (kk & 63) + 64 * i < npiece) {
                    const float x = tile[pl * kNchwStride + kk];
                    obase[(int64_t)(512 * i + 8 * (kk & 63) + 4 * h + (kk >> 6)) * np] = (typename OUT::elem)x;
                }
            }
        }
    }
}

// One launch that copies the real rows of a part's residual into the capture store of a tapped layer (vithip.h "Layer features"):
// n_hi units of 16 bytes of the hi plane (or of the fp32 array), then n_lo of the lo plane.  1024 units per workgroup.
__global__ void __launch_bounds__(256)
feat_capture_kernel(const u32x4* __restrict__ src_hi, u32x4* __restrict__ dst_hi, int64_t n_hi, const u32x4* __restrict__ src_lo,
                    u32x4* __restrict__ dst_lo, int64_t n_lo) {
    const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    u32x4 t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t u = base + 256 * k;
        if (u < n_hi) t[k] = src_hi[u];
        else if (u - n_hi < n_lo) t[k] = src_lo[u - n_hi];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t u = base + 256 * k;
        if (u < n_hi) dst_hi[u] = t[k];
        else if (u - n_hi < n_lo) dst_lo[u - n_hi] = t[k];
    }
}

// mean_out[b][k] = (((0 + v[b,lead,k]) + v[b,lead+1,k]) + ... + v[b,tokens-1,k]) * inv, v as feat_rows_kernel writes it in fp32.
// One thread per image and four columns; n4 = batch * dim / 4 threads.
template <typename IN, typename OUT>
__global__ void __launch_bounds__(256)
feat_mean_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int64_t n4, int tokens, int lead, int dim,
                 const float* __restrict__ gamma, const float* __restrict__ beta, int norm, const float* __restrict__ stats,
                 float inv, typename OUT::elem* __restrict__ mean_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n4) return;
    const int q4 = dim >> 2;
    const int64_t img = idx / q4;
    const int k = (int)(idx - img * q4) * 4;
    f32x4 g = {1.f, 1.f, 1.f, 1.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (norm) { g = *(const f32x4*)(gamma + k); b = *(const f32x4*)(beta + k); }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int64_t row0 = img * tokens;
#pragma unroll 4
    for (int t = lead; t < tokens; ++t) {
        const int64_t row = row0 + t;
        float x[4];
        load_x<IN, 4>(hi, lo, row * dim + k, x);
        if (norm) {
            const f32x2 st = *(const f32x2*)(stats + 2 * row);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = feat_norm(x[j], st[0], st[1], g[j], b[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += x[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] *= inv;
    store4<OUT>(mean_out + img * dim + k, acc);
}

template <typename IN, typename OUT>
hipError_t feat_launch(const FeatureArgs& a, hipStream_t s) {
    using E = typename OUT::elem;
    const int64_t rows = (int64_t)a.batch * a.tokens;
    const int norm = a.norm == VH_FEAT_NORM ? 1 : 0;   // the kernels' flag: 1 = through the LayerNorm
    const bool mean_norm = a.mean && norm;
    // channels-first patch rows: their own kernel, which also writes the patch rows' statistics; the row kernel then serves cls / reg
    const bool nchw = a.patch && a.patch_layout == VH_FEAT_NCHW;
    if (nchw) {
        const dim3 grid((unsigned)((a.tokens - a.lead + kNchwTile - 1) / kNchwTile) * (unsigned)a.batch), block(1024);
        float* st = mean_norm ? a.stats : nullptr;
#define VH_FEAT_NCHW_L(CH) hipLaunchKernelGGL((feat_nchw_kernel<IN, OUT, CH>), grid, block, 0, s, a.hi, a.lo, a.tokens, a.lead, a.dim, \
                                              a.gamma, a.beta, a.eps, norm, (E*)a.patch, st)
        if (a.dim <= 512) VH_FEAT_NCHW_L(1);
        else if (a.dim <= 1024) VH_FEAT_NCHW_L(2);
        else if (a.dim <= 1536) VH_FEAT_NCHW_L(3);
        else VH_FEAT_NCHW_L(4);
#undef VH_FEAT_NCHW_L
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    void* const patch_rows = nchw ? nullptr : a.patch;
    const bool stats_rows = mean_norm && !nchw;
    if (a.cls || a.reg || patch_rows || stats_rows) {   // (a raw mean needs no row pass: nothing to normalise, no statistics)
        const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
        float* st = stats_rows ? a.stats : nullptr;
#define VH_FEAT_ROWS_L(CH) hipLaunchKernelGGL((feat_rows_kernel<IN, OUT, CH>), grid, block, 0, s, a.hi, a.lo, rows, a.tokens, a.lead, \
                                              a.no_cls ? 0 : 1, a.dim, a.gamma, a.beta, a.eps, norm, (E*)a.cls, (E*)a.reg, (E*)patch_rows, st)
        if (a.dim <= 512) VH_FEAT_ROWS_L(1);
        else if (a.dim <= 1024) VH_FEAT_ROWS_L(2);
        else if (a.dim <= 1536) VH_FEAT_ROWS_L(3);
        else VH_FEAT_ROWS_L(4);
#undef VH_FEAT_ROWS_L
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.mean) {
        const int64_t n4 = (int64_t)a.batch * (a.dim >> 2);
        const float inv = (float)(1.0 / (double)(a.tokens - a.lead));
        hipLaunchKernelGGL((feat_mean_kernel<IN, OUT>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.hi, a.lo, n4, a.tokens, a.lead, a.dim,
                           a.gamma, a.beta, norm, a.stats, inv, (E*)a.mean);
        return hipGetLastError();
    }
    return hipSuccess;
}

template <typename IN>
hipError_t feat_launch_in(const FeatureArgs& a, hipStream_t s) {
    if (a.elem == VH_ELEM_F32) return feat_launch<IN, F32OUT>(a, s);
    if (a.elem == VH_ELEM_F16) return feat_launch<IN, FP16>(a, s);
    if (a.elem == VH_ELEM_BF16) return feat_launch<IN, BF16>(a, s);
    return hipErrorInvalidValue;
}

// ---- the pooled head's input (VH_FLAG_POOL; vithip.h): the mean over an image's patch rows in ONE pass over the planes ----------
// out[b][k] = (((0 + v[b,lead,k]) + v[b,lead+1,k]) + ... + v[b,tokens-1,k]) * inv: the bits feat_rows_kernel + feat_mean_kernel give,
// because a row goes through the same row_load / row_stats / piece_norm and a column's chain is the same serial fp32 adds in
// ascending token order.  One workgroup (16 waves) per image.  A group = `group` consecutive patch rows (min(16, 16384 / dim):
// 64 KiB of LDS at most, two workgroups per CU): wave w < group takes row w of the group, keeps it in registers, normalises it and
// parks the fp32 row in LDS; then thread t, which owns columns t and t + 1024, adds the group's values of its columns in row
// order.  Nothing depends on the batch, on `group` or on which workgroup an image gets.  cls_in (optional, VH_POOL_CLS_AVG):
// cls_out[b][0 .. dim) <- cls_in[b][0 .. dim).  One workgroup per image: a small batch of long sequences pools on few CUs.
constexpr int kPoolWaves = 16, kPoolLdsFloats = 16384;
template <typename IN, int CH>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(CH <= 2 ? 8 : 4)))   // dim <= 1024: 64 VGPRs, two workgroups per CU
pool_rows_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int tokens, int lead, int dim, const float* __restrict__ gamma,
                 const float* __restrict__ beta, float eps, int norm, int group, float inv, float* __restrict__ out, int64_t out_stride,
                 const float* __restrict__ cls_in, float* __restrict__ cls_out) {
    __shared__ __attribute__((aligned(16))) float park[kPoolLdsFloats];   // [group][dim]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int np = tokens - lead, npiece = dim >> 3;
    const int64_t img = blockIdx.x;
    const int64_t row0 = img * tokens + lead;
    const bool loader = wave < group;   // wave-uniform
    float acc[2] = {0.f, 0.f};
    // CH == 1: the next group's row is loaded before the barrier (with the second register copy of the row 50 - 52 VGPRs, profiles/pool_isa.txt).  Wider rows
    // load at the top of their group: two workgroups per CU hide each other's latency instead, which the second copy would forbid.
    constexpr bool AHEAD = CH == 1;
    float v[CH][8], vn[AHEAD ? CH : 1][8];
    if (AHEAD && loader && wave < np) row_load<IN, CH>(hi, lo, row0 + wave, dim, lane, v);
    for (int p0 = 0; p0 < np; p0 += group) {
        const int p = p0 + wave;
        const bool next = AHEAD && loader && p + group < np;
        if constexpr (AHEAD) {
            if (next) row_load<IN, CH>(hi, lo, row0 + p + group, dim, lane, vn);
        } else {
            if (loader && p < np) row_load<IN, CH>(hi, lo, row0 + p, dim, lane, v);
        }
        if (loader && p < np) {
            float mean = 0.f, rstd = 1.f;
            if (norm) row_stats<CH>(v, dim, lane, eps, mean, rstd);
            float* const w = park + wave * dim;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int c = lane + 64 * i;
                if (c < npiece) {
                    if (norm) piece_norm(v[i], c, mean, rstd, gamma, beta);
                    ((f32x4*)(w + 8 * c))[0] = f32x4{v[i][0], v[i][1], v[i][2], v[i][3]};
                    ((f32x4*)(w + 8 * c))[1] = f32x4{v[i][4], v[i][5], v[i][6], v[i][7]};
                }
            }
        }
        __syncthreads();
        const int n = np - p0 < group ? np - p0 : group;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = threadIdx.x + 1024 * j;
            if (col < dim)
                for (int g = 0; g < n; ++g) acc[j] += park[g * dim + col];
        }
        __syncthreads();   // the group has been added: its LDS rows are free
        if constexpr (AHEAD) {
            if (next) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[0][j] = vn[0][j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = threadIdx.x + 1024 * j;
        if (col < dim) {
            out[img * out_stride + col] = acc[j] * inv;
            if (cls_in) cls_out[img * out_stride + col] = cls_in[img * dim + col];
        }
    }
}

template <typename IN>
hipError_t pool_launch(const PoolArgs& a, hipStream_t s) {
    const int norm = a.norm == VH_FEAT_NORM ? 1 : 0;
    const int group = kPoolLdsFloats / a.dim < kPoolWaves ? kPoolLdsFloats / a.dim : kPoolWaves;
    const float inv = (float)(1.0 / (double)(a.tokens - a.lead));
    const int64_t stride = a.out_stride ? a.out_stride : a.dim;
#define VH_POOL_L(CH) hipLaunchKernelGGL((pool_rows_kernel<IN, CH>), dim3((unsigned)a.batch), dim3(1024), 0, s, a.hi, a.lo, a.tokens, a.lead, a.dim, \
                                         a.gamma, a.beta, a.eps, norm, group, inv, a.out, stride, a.cls_in, a.cls_out)
    if (a.dim <= 512) VH_POOL_L(1);
    else if (a.dim <= 1024) VH_POOL_L(2);
    else if (a.dim <= 1536) VH_POOL_L(3);
    else VH_POOL_L(4);
#undef VH_POOL_L
    return hipGetLastError();
}

// ---- the token-sized pass of the attention-pooling head (VH_FLAG_MAP_HEAD; vithip.h): z[b][h][k] = sum_t softmax_t(qk[h] . y_t) y_t[k] -----
// over the patch rows of image b, y_t = the row through the final LayerNorm.  The skeleton is pool_rows_kernel's: one workgroup (16
// waves) per image, a group of `group` consecutive patch rows at a time, wave w < group takes row w through row_load / row_stats /
// piece_norm, parks the fp32 row in LDS -- and, here, computes the row's `heads` scores against qk (read through L1 / L2: heads x dim
// floats, the same for every row and image) by wave reductions, in the log2 domain.  Then three steps per group, a barrier between them:
//   1. thread (g, h) of the first 256 finds the new running maximum m[h] = max(m[h], max_g s[g][h]) and writes p[g][h] = exp2(s[g][h] -
//      m[h]); thread (0, h) also updates the running sum l[h] and leaves the group's rescale factor f[h] = exp2(m_old - m_new) -- 0 for
//      the first group, stated, so that (-inf) - (-inf) is never formed;
//   2. thread t, which owns column t (and t + 1024, .. where dim is wider than the workgroup), multiplies its accumulators by f[h] ONCE and adds p[g][h] * y[g][col]
//      for the group's rows in ascending order.  acc[NCOL][HB] is fully unrolled (HB = the head bucket: 4, 12 or 16): registers.
//   3. the group's LDS rows are free.
// The end divides by l[h].  Every sum has one order, which depends on dim, heads and the token index alone: an image's bits do not depend
// on the batch, the workgroup or the stream.  Heads h >= heads of a bucket keep p = f = 0 and are never written.
// NW = waves per workgroup: 16, as the pool kernel; 8 for the widest instantiation (dim > 1536 with more than 12 heads), whose row, 32
// accumulators and addresses are a few VGPRs more than the 128 a wave of a 1024-thread workgroup has -- 512 threads own four columns each
// and a group is at most 8 rows (map_pool_group), which is what 16384 / dim allows at 2048 anyway.
constexpr int kMapHeadSlots = VH_MAP_MAX_HEADS;
constexpr int map_pool_waves(int ch, int hb) { return ch == 4 && hb == 16 ? 8 : kPoolWaves; }
template <typename IN, int CH, int HB, int NW>
__global__ void __launch_bounds__(NW * 64)
map_pool_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int tokens, int lead, int dim, const float* __restrict__ gamma,
                const float* __restrict__ beta, float eps, int group, const float* __restrict__ qk, int heads, float* __restrict__ out) {
    static_assert(HB % 4 == 0 && HB <= kMapHeadSlots, "head bucket: a multiple of 4, at most 16");
    __shared__ __attribute__((aligned(16))) float park[kPoolLdsFloats];                  // [group][dim]
    __shared__ __attribute__((aligned(16))) float sc[kPoolWaves * kMapHeadSlots];        // [group][16] scores, log2 domain
    __shared__ __attribute__((aligned(16))) float pw[kPoolWaves * kMapHeadSlots];        // [group][16] softmax numerators of the group
    __shared__ __attribute__((aligned(16))) float fsc[kMapHeadSlots];                    // the group's rescale factors
    __shared__ float mrun[2][kMapHeadSlots], lrun[kMapHeadSlots];                        // running maximum (by group parity) and sum
    constexpr int NT = NW * 64, NCOL = (CH * 512 + NT - 1) / NT;   // columns per thread: t, t + NT, ..
    constexpr float kLog2e = 1.44269504088896341f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int np = tokens - lead, npiece = dim >> 3;
    const int64_t img = blockIdx.x;
    const int64_t row0 = img * tokens + lead;
    const bool loader = wave < group;   // wave-uniform
    float acc[NCOL][HB];
#pragma unroll
    for (int j = 0; j < NCOL; ++j)
#pragma unroll
        for (int h = 0; h < HB; ++h) acc[j][h] = 0.f;
    if (threadIdx.x < kPoolWaves * kMapHeadSlots) pw[threadIdx.x] = 0.f;
    if (threadIdx.x < kMapHeadSlots) {
        mrun[0][threadIdx.x] = -INFINITY;
        lrun[threadIdx.x] = 0.f;
        fsc[threadIdx.x] = 0.f;
    }
    int par = 0;
    for (int p0 = 0; p0 < np; p0 += group) {
        const int p = p0 + wave;
        if (loader && p < np) {
            float v[CH][8];
            row_load<IN, CH>(hi, lo, row0 + p, dim, lane, v);
            float mean, rstd;
            row_stats<CH>(v, dim, lane, eps, mean, rstd);
            float* const w = park + wave * dim;
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int c = lane + 64 * i;
                if (c < npiece) {
                    piece_norm(v[i], c, mean, rstd, gamma, beta);
                    ((f32x4*)(w + 8 * c))[0] = f32x4{v[i][0], v[i][1], v[i][2], v[i][3]};
                    ((f32x4*)(w + 8 * c))[1] = f32x4{v[i][4], v[i][5], v[i][6], v[i][7]};
                }
            }
            // the row's scores: per lane its pieces ascending (an fmaf chain over a piece's 8 elements), then the xor butterfly
#pragma unroll 1
            for (int h = 0; h < heads; ++h) {   // (one head at a time: unrolled, the loads of several heads cost the registers the accumulators live in)
                const f32x4* const q = (const f32x4*)(qk + (int64_t)h * dim);
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int c = lane + 64 * i;
                    if (c < npiece) {
                        const f32x4 q0 = q[2 * c], q1 = q[2 * c + 1];
#pragma unroll
                        for (int j = 0; j < 4; ++j) s = __builtin_fmaf(v[i][j], q0[j], s);
#pragma unroll
                        for (int j = 0; j < 4; ++j) s = __builtin_fmaf(v[i][4 + j], q1[j], s);
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == 0) sc[wave * kMapHeadSlots + h] = s * kLog2e;
            }
        }
        __syncthreads();   // the group's rows and scores are parked (and, first group, the running state is initialised)
        const int n = np - p0 < group ? np - p0 : group;
        if (threadIdx.x < kPoolWaves * kMapHeadSlots) {
            const int g = threadIdx.x >> 4, h = threadIdx.x & (kMapHeadSlots - 1);
            if (g < n && h < heads) {
                const float m_old = mrun[par][h];
                float m_new = m_old;
                for (int gg = 0; gg < n; ++gg) m_new = fmaxf(m_new, sc[gg * kMapHeadSlots + h]);
                pw[threadIdx.x] = __builtin_amdgcn_exp2f(sc[threadIdx.x] - m_new);
                if (g == 0) {
                    float sum = 0.f;
                    for (int gg = 0; gg < n; ++gg) sum += __builtin_amdgcn_exp2f(sc[gg * kMapHeadSlots + h] - m_new);
                    const float f = p0 == 0 ? 0.f : __builtin_amdgcn_exp2f(m_old - m_new);   // first group: nothing to rescale, no inf - inf
                    lrun[h] = __builtin_fmaf(lrun[h], f, sum);
                    fsc[h] = f;
                    mrun[par ^ 1][h] = m_new;
                }
            }
        }
        __syncthreads();   // p, f and l of the group are in LDS
        if ((int)threadIdx.x < dim) {
#pragma unroll
            for (int q = 0; q < HB / 4; ++q) {
                const f32x4 f4 = ((const f32x4*)fsc)[q];
#pragma unroll
                for (int j = 0; j < NCOL; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[j][4 * q + k] *= f4[k];
            }
#pragma unroll 1
            for (int g = 0; g < n; ++g) {
                float x[NCOL];
#pragma unroll
                for (int j = 0; j < NCOL; ++j) {
                    const int col = threadIdx.x + NT * j;
                    x[j] = col < dim ? park[g * dim + col] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < HB / 4; ++q) {
                    const f32x4 p4 = ((const f32x4*)(pw + g * kMapHeadSlots))[q];
#pragma unroll
                    for (int j = 0; j < NCOL; ++j)
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[j][4 * q + k] = __builtin_fmaf(p4[k], x[j], acc[j][4 * q + k]);
                }
            }
        }
        __syncthreads();   // the group has been added: its LDS rows, scores and numerators are free
        par ^= 1;
    }
#pragma unroll
    for (int j = 0; j < NCOL; ++j) {
        const int col = threadIdx.x + NT * j;
        if (col < dim) {
#pragma unroll
            for (int h = 0; h < HB; ++h)
                if (h < heads) out[(img * heads + h) * dim + col] = acc[j][h] / lrun[h];
        }
    }
}

template <typename IN>
hipError_t map_pool_launch(const PoolArgs& a, const float* qk, int heads, hipStream_t s) {
    const int group = map_pool_group(a.dim, heads);
#define VH_MAP_L(CH, HB) hipLaunchKernelGGL((map_pool_kernel<IN, CH, HB, map_pool_waves(CH, HB)>), dim3((unsigned)a.batch), dim3(map_pool_waves(CH, HB) * 64), 0, s, a.hi, a.lo, a.tokens, a.lead, \
                                            a.dim, a.gamma, a.beta, a.eps, group, qk, heads, a.out)
#define VH_MAP_H(CH) do { if (heads <= 4) VH_MAP_L(CH, 4); else if (heads <= 12) VH_MAP_L(CH, 12); else VH_MAP_L(CH, 16); } while (0)
    if (a.dim <= 512) VH_MAP_H(1);
    else if (a.dim <= 1024) VH_MAP_H(2);
    else if (a.dim <= 1536) VH_MAP_H(3);
    else VH_MAP_H(4);
#undef VH_MAP_H
#undef VH_MAP_L
    return hipGetLastError();
}

}  // namespace

int map_pool_group(int dim, int heads) {
    const int waves = map_pool_waves(dim > 1536 ? 4 : 1, heads > 12 ? 16 : 4);
    return kPoolLdsFloats / dim < waves ? kPoolLdsFloats / dim : waves;
}

const char* map_pool_check(const PoolArgs& a, const float* qk, int heads) {
    if (const char* why = pool_check(a)) {   // the rows, the LayerNorm and the output are pool_rows' own arguments: its reasons, under this tap's name
        static thread_local char text[160];
        const char* colon = strchr(why, ':');
        snprintf(text, sizeof text, "map_pool%s", colon ? colon : why);
        return text;
    }
    if (a.norm != VH_FEAT_NORM) return "map_pool: the rows pass the LayerNorm (norm must be VH_FEAT_NORM)";
    if (a.out_stride || a.cls_in || a.cls_out) return "map_pool: no output stride and no class rows";
    if (!qk) return "map_pool: null qk";
    if ((uintptr_t)qk & 15) return "map_pool: a device pointer is not 16-byte aligned";
    if (heads < 1 || heads > VH_MAP_MAX_HEADS) return "map_pool: heads outside 1..16";
    return nullptr;
}

hipError_t launch_map_pool(const PoolArgs& a, const float* qk, int heads, hipStream_t s) {
    if (map_pool_check(a, qk, heads)) return hipErrorInvalidValue;
    if (a.form == VH_FEAT_FORM_F32) return map_pool_launch<InF32>(a, qk, heads, s);
    if (a.form == VH_DTYPE_FP8) return map_pool_launch<InSplit8>(a, qk, heads, s);
    return a.form == VH_DTYPE_BF16 ? map_pool_launch<InSplit16<BF16>>(a, qk, heads, s) : map_pool_launch<InSplit16<FP16>>(a, qk, heads, s);
}

const char* pool_check(const PoolArgs& a) {
    if (!a.hi) return "pool_rows: null input";
    if (a.form != VH_FEAT_FORM_F32 && a.form != VH_DTYPE_BF16 && a.form != VH_DTYPE_FP16 && a.form != VH_DTYPE_FP8)
        return "pool_rows: form must be VH_DTYPE_BF16, VH_DTYPE_FP16, VH_DTYPE_FP8 (split planes) or -1 (fp32 rows)";
    if (a.form == VH_FEAT_FORM_F32 && a.lo) return "pool_rows: fp32 rows take no lo plane";
    if (a.form != VH_FEAT_FORM_F32 && !a.lo) return "pool_rows: split planes need the lo plane";
    if (a.batch <= 0 || a.batch > (1 << 20)) return "pool_rows: batch outside 1..2^20";
    if (a.tokens < 1) return "pool_rows: tokens below 1 (no patch token)";
    if (a.tokens > kAttnStreamMaxTokens) return "pool_rows: tokens above 4097";
    if (a.lead < 0 || a.lead >= a.tokens) return "pool_rows: lead rows outside 0 .. tokens - 1";
    if (a.dim < 64) return "pool_rows: dim below 64";
    if (a.dim > 2048) return "pool_rows: dim above 2048";
    if (a.dim % 8) return "pool_rows: dim must be a multiple of 8";
    if (!a.out) return "pool_rows: null output";
    if (a.norm != VH_FEAT_NORM && a.norm != VH_FEAT_RAW) return "pool_rows: norm must be VH_FEAT_NORM or VH_FEAT_RAW";
    if (a.norm == VH_FEAT_NORM) {
        if (!a.gamma || !a.beta) return "pool_rows: VH_FEAT_NORM needs gamma and beta";
        if (!(a.eps > 0.f)) return "pool_rows: eps must be positive";
    }
    if (a.out_stride && a.out_stride < a.dim) return "pool_rows: the output's row stride is below dim";
    if ((a.cls_in != nullptr) != (a.cls_out != nullptr)) return "pool_rows: cls_in and cls_out go together";
    const uintptr_t al = (uintptr_t)a.hi | (uintptr_t)a.lo | (uintptr_t)a.gamma | (uintptr_t)a.beta | (uintptr_t)a.out | (uintptr_t)a.cls_in |
                         (uintptr_t)a.cls_out;
    if (al & 15) return "pool_rows: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_pool_rows(const PoolArgs& a, hipStream_t s) {
    if (pool_check(a)) return hipErrorInvalidValue;
    if (a.form == VH_FEAT_FORM_F32) return pool_launch<InF32>(a, s);
    if (a.form == VH_DTYPE_FP8) return pool_launch<InSplit8>(a, s);
    return a.form == VH_DTYPE_BF16 ? pool_launch<InSplit16<BF16>>(a, s) : pool_launch<InSplit16<FP16>>(a, s);
}

const char* features_check(const FeatureArgs& a) {
    if (!a.hi) return "token_features: null input";
    if (a.form != VH_FEAT_FORM_F32 && a.form != VH_DTYPE_BF16 && a.form != VH_DTYPE_FP16 && a.form != VH_DTYPE_FP8)
        return "token_features: form must be VH_DTYPE_BF16, VH_DTYPE_FP16, VH_DTYPE_FP8 (split planes) or -1 (fp32 rows)";
    if (a.form == VH_FEAT_FORM_F32 && a.lo) return "token_features: fp32 rows take no lo plane";
    if (a.form != VH_FEAT_FORM_F32 && !a.lo) return "token_features: split planes need the lo plane";
    if (a.batch <= 0 || a.batch > (1 << 20)) return "token_features: batch outside 1..2^20";
    if (a.no_cls) {   // internal launches of a VH_FLAG_NO_CLS context only: no public tap sets it
        if (a.tokens < 1) return "token_features: tokens below 1 (no patch token)";
        if (a.lead < 0 || a.lead >= a.tokens) return "token_features: lead rows outside 0 .. tokens - 1";
        if (a.cls) return "token_features: class-token rows requested where there is no class token";
    } else {
        if (a.tokens < 2) return "token_features: tokens below 2 (no patch token)";
        if (a.lead < 1 || a.lead >= a.tokens) return "token_features: lead rows outside 1 .. tokens - 1";
    }
    if (a.tokens > kAttnStreamMaxTokens) return "token_features: tokens above 4097";
    if (a.dim < 64) return "token_features: dim below 64";
    if (a.dim > 2048) return "token_features: dim above 2048";
    if (a.dim % 8) return "token_features: dim must be a multiple of 8";
    if (!a.cls && !a.patch && !a.mean && !a.reg) return "token_features: no output requested";
    if (a.reg && a.no_cls && a.lead < 1) return "token_features: register rows requested where lead is 0 (no register rows)";
    if (a.reg && !a.no_cls && a.lead < 2) return "token_features: register rows requested where lead is 1 (no register rows)";
    if (a.patch_layout != VH_FEAT_ROWS && a.patch_layout != VH_FEAT_NCHW) return "token_features: patch_layout must be VH_FEAT_ROWS or VH_FEAT_NCHW";
    if (a.elem != VH_ELEM_F32 && a.elem != VH_ELEM_F16 && a.elem != VH_ELEM_BF16)
        return "token_features: elem must be VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16";
    if (a.norm != VH_FEAT_NORM && a.norm != VH_FEAT_RAW) return "token_features: norm must be VH_FEAT_NORM or VH_FEAT_RAW";
    if (a.norm == VH_FEAT_NORM) {
        if (!a.gamma || !a.beta) return "token_features: VH_FEAT_NORM needs gamma and beta";
        if (!(a.eps > 0.f)) return "token_features: eps must be positive";
    }
    const uintptr_t al = (uintptr_t)a.hi | (uintptr_t)a.lo | (uintptr_t)a.gamma | (uintptr_t)a.beta | (uintptr_t)a.cls | (uintptr_t)a.patch |
                         (uintptr_t)a.mean | (uintptr_t)a.reg;
    if (al & 15) return "token_features: a device pointer is not 16-byte aligned";
    if ((uintptr_t)a.stats & 7) return "token_features: the row statistics buffer is not 8-byte aligned";
    return nullptr;
}

hipError_t launch_token_features(const FeatureArgs& a, hipStream_t s) {
    if (features_check(a)) return hipErrorInvalidValue;
    if (a.mean && a.norm == VH_FEAT_NORM && !a.stats) return hipErrorInvalidValue;   // the normalised mean needs the statistics scratch
    if (a.form == VH_FEAT_FORM_F32) return feat_launch_in<InF32>(a, s);
    if (a.form == VH_DTYPE_FP8) return feat_launch_in<InSplit8>(a, s);
    return a.form == VH_DTYPE_BF16 ? feat_launch_in<InSplit16<BF16>>(a, s) : feat_launch_in<InSplit16<FP16>>(a, s);
}

hipError_t launch_feature_capture(const void* src_hi, void* dst_hi, size_t bytes_hi, const void* src_lo, void* dst_lo, size_t bytes_lo,
                                  hipStream_t s) {
    const uintptr_t al = (uintptr_t)src_hi | (uintptr_t)dst_hi | (uintptr_t)src_lo | (uintptr_t)dst_lo | bytes_hi | bytes_lo;
    if (!src_hi || !dst_hi || !bytes_hi || (bytes_lo && (!src_lo || !dst_lo)) || (al & 15)) return hipErrorInvalidValue;
    const int64_t n_hi = (int64_t)(bytes_hi / 16), n_lo = (int64_t)(bytes_lo / 16);
    hipLaunchKernelGGL(feat_capture_kernel, dim3((unsigned)((n_hi + n_lo + 1023) / 1024)), dim3(256), 0, s, (const u32x4*)src_hi, (u32x4*)dst_hi,
                       n_hi, (const u32x4*)src_lo, (u32x4*)dst_lo, n_lo);
    return hipGetLastError();
}

}  // namespace vh
