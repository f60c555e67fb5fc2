// kernels_rows.hip — the one-wave-per-row kernels around the GEMMs (gfx950): LayerNorm, the row-statistics cast / split, the
// pre-LayerNorm, the LayerNorm of the split planes, the statistics finalizer and the guards, the LayerNorm weight folds and the
// e4m3 row quantisers.  Helpers, then kernels, then launchers.
// (per-element tests on exactly predictable rows: tests/rows_exact.py, test_rows_exact.py, test_gpu_rows_exact.py)
#include <type_traits>
#include <utility>

#include "vh_kernels.h"

namespace vh {

// ---- helpers ---------------------------------------------------------------------------------------------------------------
// The run-time check on the folded LayerNorm.  The folded GEMM multiplies the rounded UNCENTRED rows, so its
// rounding error relative to the centred signal grows with sqrt(1 + (mean/sigma)^2); every row of the first `guard_rows` rows
// (the real ones: rows behind them are tile padding) contributes |mean| * rstd to a running maximum kept as the bits of a
// non-negative float (ordered like unsigned integers; a NaN ranks above everything and trips the guard too).  A wave first READS
// the word (an L2 hit shared by everybody) and issues its atomic only when it would raise it: after the first forward the
// maximum stands and no atomic is issued at all (one atomic per wave unconditionally -- 1 576 on one address per launch --
// tripled the kernel's time).  WHOLE waves call this: no early return in front of it that splits a wave.
__device__ __forceinline__ void ln_guard_update(float ratio, unsigned int* guard) {
    const unsigned int b = wave_max(__float_as_uint(ratio) & 0x7FFFFFFFu);
    if ((threadIdx.x & 63) == 0 && b > __hip_atomic_load(guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(guard, b);
}

// One row of `dim` floats in the registers of one wave: lane l holds the float4 chunks l + 64 i, i < CH (dim <= 256 CH, 4 | dim);
// chunks beyond the row are zeros.  The statistics are the two-pass ones, in one fixed order: per lane in chunk order, then the
// butterfly.  A zero chunk adds nothing to a sum that starts at +0 and the deviation loop skips it, so the CH class a row runs
// in does not show in the bits.
template <int CH>
struct RowRegs {
    f32x4 v[CH];
    int lane, nchunk, dim;

    __device__ __forceinline__ RowRegs(int dim_) : lane(threadIdx.x & 63), nchunk(dim_ >> 2), dim(dim_) {}
    // this lane's part of the row sum after chunk i (and, AMAX, of max |x|): called in chunk order
    template <bool AMAX>
    __device__ __forceinline__ void add_chunk(int i, float& sum, float& amax) const {
        sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        if constexpr (AMAX) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v[i][0]), fabsf(v[i][1]))), fmaxf(fabsf(v[i][2]), fabsf(v[i][3])));
    }
    // chunk i <- chunk lane + 64 i of the row at xr (zeros beyond the row), and add_chunk.  The kernels call this for i = 0 ..
    // CH - 1 in a loop of their own: with the loop in here hipcc packs the additions across chunks and then waits for each
    // chunk's load before it issues the next (layernorm_kernel ran 3 to 9 % longer).
    template <bool AMAX = false>
    __device__ __forceinline__ void load_chunk(int i, const float* xr, float& sum, float& amax) {
        const int c = lane + 64 * i;
        v[i] = c < nchunk ? ((const f32x4*)xr)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        add_chunk<AMAX>(i, sum, amax);
    }
    __device__ __forceinline__ float mean(float lane_sum) const { return wave_sum(lane_sum) / (float)dim; }
    // rstd from the squared deviations of the real chunks; per_chunk(i, c) runs inside that loop for chunk c = lane + 64 i
    template <typename F>
    __device__ __forceinline__ float rstd(float mean, float eps, F&& per_chunk) const {
        float var = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + 64 * i;
            if (c < nchunk) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; var += d * d; }
                per_chunk(i, c);
            }
        }
        var = wave_sum(var);
        return 1.0f / sqrtf(var / (float)dim + eps);
    }
    __device__ __forceinline__ float rstd(float mean, float eps) const { return rstd(mean, eps, [](int, int) {}); }
    // (x - mean) * rstd * gamma + beta of chunk i = columns 4 c .. 4 c + 3
    __device__ __forceinline__ f32x4 normalised(int i, int c, float mean, float rstd, const float* gamma, const float* beta) const {
        const f32x4 gm = ((const f32x4*)gamma)[c], bt = ((const f32x4*)beta)[c];
        return f32x4{(v[i][0] - mean) * rstd * gm[0] + bt[0], (v[i][1] - mean) * rstd * gm[1] + bt[1],
                     (v[i][2] - mean) * rstd * gm[2] + bt[2], (v[i][3] - mean) * rstd * gm[3] + bt[3]};
    }
};

// four values x of a row -> the planes of the split residual at element offset `off`: hi = T(x); lo (optional) = what that
// rounding dropped -- 16-bit T: one scaled e4m3 byte (Lo8<T>); T = e4m3: bf16
template <typename T>
__device__ __forceinline__ void store_planes(typename T::elem* hi, void* lo_, int64_t off, f32x4 x) {
    const typename T::vec4 hq = pack4<T>(x[0], x[1], x[2], x[3]);
    *(typename T::vec4*)(hi + off) = hq;
    if constexpr (!std::is_same<T, E4M3>::value) {
        uint8_t* const lo = (uint8_t*)lo_;
        if (lo) *(uint32_t*)(lo + off) = lo8_pack4<T>(x[0] - (float)hq[0], x[1] - (float)hq[1], x[2] - (float)hq[2], x[3] - (float)hq[3]);
    } else {
        typename BF16::elem* const lo = (typename BF16::elem*)lo_;
        if (lo) {
            const uint32_t w = (uint32_t)hq;
            *(typename BF16::vec4*)(lo + off) =
                pack4<BF16>(x[0] - __builtin_amdgcn_cvt_f32_fp8((int)w, 0), x[1] - __builtin_amdgcn_cvt_f32_fp8((int)w, 1),
                            x[2] - __builtin_amdgcn_cvt_f32_fp8((int)w, 2), x[3] - __builtin_amdgcn_cvt_f32_fp8((int)w, 3));
        }
    }
}

// What leaves a row that is in the registers besides its fp32 values: (mean, rstd) -> stats, the planes (hi, lo), and the guard
// quantities of the real rows (row < guard_rows): max |mean| * rstd (`guard`) and, e4m3 planes, max |x| (`amax_guard`: the raw
// rows are the q|k|v / fc1 operand of the folded fp8 path and e4m3 saturates at 448).  lane_sum / lane_amax: what add_chunk
// gathered over the row.  hi, stats and both guards are optional; all of them are kernel arguments, and a wave is one row, so
// every branch here is uniform.
template <typename T, int CH>
__device__ __forceinline__ void row_stats_planes(const RowRegs<CH>& r, int64_t row, float eps, float lane_sum, float lane_amax,
                                                 typename T::elem* hi, void* lo, float* stats, int64_t guard_rows, unsigned int* guard,
                                                 unsigned int* amax_guard) {
    if constexpr (std::is_same<T, E4M3>::value) {
        if (amax_guard) ln_guard_update(row < guard_rows ? lane_amax : 0.f, amax_guard);
    }
    const float mean = r.mean(lane_sum);
    const float rstd = r.rstd(mean, eps, [&](int i, int c) {
        if (hi) store_planes<T>(hi, lo, row * r.dim + 4 * c, r.v[i]);
    });
    if (stats && r.lane == 0) *(float2*)(stats + 2 * row) = make_float2(mean, rstd);
    if (guard) ln_guard_update(row < guard_rows ? fabsf(mean) * rstd : 0.f, guard);
}

// e4m3 row quantiser: s0 = amax_r * (1/448) (1 if the row is all zero) of the row whose float4 chunk c is chunk(c); the bytes
// are q = rne_e4m3(w / s0) (IEEE division: the oracle's quantiser divides too, so both produce the same byte)
template <typename F>
__device__ __forceinline__ float e4m3_row_scale(int lane, int n4, F&& chunk) {
    float amax = 0.f;
    for (int c = lane; c < n4; c += 64) {
        const f32x4 v = chunk(c);
        amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    amax = wave_max(amax);
    return amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
}
__device__ __forceinline__ uint32_t e4m3_quantise4(f32x4 v, float s0) {
    return pack4_e4m3(__fdiv_rn(v[0], s0), __fdiv_rn(v[1], s0), __fdiv_rn(v[2], s0), __fdiv_rn(v[3], s0));
}

// ---- kernels: one wave per row, four rows per block ------------------------------------------------------------------------
// y[r,:] = (x[r,:] - mean) * rstd * gamma + beta  -> 16-bit, e4m3 or fp32
template <typename T, int CH>
__global__ void __launch_bounds__(256)
layernorm_kernel(const float* __restrict__ x, int64_t rows, int dim, int64_t row_stride,
                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                 typename T::elem* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    RowRegs<CH> r(dim);
    float sum = 0.f, amax = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) r.load_chunk(i, x + row * row_stride, sum, amax);
    const float mean = r.mean(sum);
    const float rstd = r.rstd(mean, eps);
    typename T::elem* orow = out + row * dim;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int c = r.lane + 64 * i;
        if (c < r.nchunk) {
            const f32x4 y = r.normalised(i, c, mean, rstd, gamma, beta);
            *(typename T::vec4*)(orow + 4 * c) = pack4<T>(y[0], y[1], y[2], y[3]);
        }
    }
}

// x fp32 [rows, dim] -> plain 16-bit / e4m3 cast + (mean, rstd) per row, and with xlo the split residual's lo plane.
// Used once per forward (first layer: its input comes from the patch embedding, not from a RESID_LN epilogue).
template <typename T, int CH>
__global__ void __launch_bounds__(256)
rowstats_cast_kernel(const float* __restrict__ x, int64_t rows, int dim, float eps, typename T::elem* __restrict__ x16,
                     float* __restrict__ stats, void* __restrict__ xlo, int64_t guard_rows, unsigned int* __restrict__ amax_guard) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    RowRegs<CH> r(dim);
    float sum = 0.f, amax = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) r.template load_chunk<std::is_same<T, E4M3>::value>(i, x + row * dim, sum, amax);
    row_stats_planes<T, CH>(r, row, eps, sum, amax, x16, xlo, stats, guard_rows, nullptr, amax_guard);
}

// ---- pre-LayerNorm (VH_FLAG_PRE_LN, CLIP's ln_pre): the embedded rows, normalised BEFORE layer 0 ---------------------------
// One pass, the row in registers (nothing goes through LDS): y = LN(x) * gamma + beta in fp32, layernorm_kernel's expression.
// y leaves in the forms the forward's paths consume, each optional: the fp32 residual (y32, may alias x: a lane reads its
// chunks before it writes them) and, through row_stats_planes on the NORMALISED row, what rowstats_cast_kernel run on y32 would
// leave -- the hi / lo planes (or the plain operand copy: lo == NULL), layer 0's LN1 statistics and the guards -- without the
// second pass over memory.
template <typename T, int CH>
__global__ void __launch_bounds__(256)
pre_layernorm_kernel(const float* x, int64_t rows, int dim, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                     float* y32, typename T::elem* __restrict__ hi, void* __restrict__ lo, float* __restrict__ stats,
                     int64_t guard_rows, unsigned int* __restrict__ guard, unsigned int* __restrict__ amax_guard) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    RowRegs<CH> r(dim);
    float sum = 0.f, ysum = 0.f, amax = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) r.load_chunk(i, x + row * dim, sum, amax);
    const float mean = r.mean(sum);
    const float rstd = r.rstd(mean, eps);
#pragma unroll
    for (int i = 0; i < CH; ++i) {   // the normalised row replaces the raw one in the registers; its own sum on the way
        const int c = r.lane + 64 * i;
        if (c < r.nchunk) {
            r.v[i] = r.normalised(i, c, mean, rstd, gamma, beta);
            if (y32) *(f32x4*)(y32 + row * dim + 4 * c) = r.v[i];
        }
        r.template add_chunk<std::is_same<T, E4M3>::value>(i, ysum, amax);   // (chunks beyond the row are zero)
    }
    if (!hi && !stats) return;   // (kernel arguments: uniform)
    row_stats_planes<T, CH>(r, row, eps, ysum, amax, hi, lo, stats, guard_rows, guard, amax_guard);
}

// LayerNorm of selected rows of the SPLIT residual (x = hi + lo: a 16-bit plane and a one-byte plane, Lo8<T>) -> fp32: the final
// LayerNorm of the CLS rows in front of the fp32 head.  Two-pass statistics like layernorm_kernel, one element per lane and step.
template <typename T>
__global__ void __launch_bounds__(256)
layernorm_split_kernel(const typename T::elem* __restrict__ hi, const void* __restrict__ lo_, int64_t rows, int dim,
                       int64_t row_stride, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                       float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const typename T::elem* hr = hi + row * row_stride;
    // x[k] = hi + lo: 16-bit hi + scaled e4m3 byte, or (fp8 path) e4m3 hi + bf16 lo
    auto xk = [&](int k) {
        if constexpr (std::is_same<T, E4M3>::value)
            return __builtin_amdgcn_cvt_f32_fp8((int)hr[k], 0) + (float)((const typename BF16::elem*)lo_ + row * row_stride)[k];
        else
            return (float)hr[k] + lo8_unpack1<T>(((const uint8_t*)lo_ + row * row_stride)[k]);
    };
    float sum = 0.f;
    for (int k = lane; k < dim; k += 64) sum += xk(k);
    const float mean = wave_sum(sum) / (float)dim;
    float var = 0.f;
    for (int k = lane; k < dim; k += 64) { const float d = (xk(k)) - mean; var += d * d; }
    var = wave_sum(var);
    const float rstd = 1.0f / sqrtf(var / (float)dim + eps);
    for (int k = lane; k < dim; k += 64) out[row * dim + k] = ((xk(k)) - mean) * rstd * gamma[k] + beta[k];
}

// partials [nblk][rows][2] = (sum, sum of squares) over 64-column blocks -> stats [rows][2] = (mean, rstd); one THREAD per row.
// Fixed summation order (block 0, 1, ...) keeps the result independent of how the producing tiles were scheduled.
// `guard` (optional): ln_guard_update's check.  `amax_guard` (optional; the fp8 path, whose folded operand is the RAW row as
// e4m3, saturating at 448): running maximum of an upper bound of |x| over the real rows -- the square root of the largest
// 64-column block's sum of squares (>= the block's largest element, <= 8 x its rms: it overshoots only where a block already
// carries several large elements).
__global__ void __launch_bounds__(256)
finalize_stats_kernel(const float* __restrict__ partials, int nblk, int64_t rows, int dim, float eps, float* __restrict__ stats,
                      int64_t guard_rows, unsigned int* __restrict__ guard, unsigned int* __restrict__ amax_guard) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float ratio = 0.f, bound = 0.f;
    if (r < rows) {
        float s1 = 0.f, s2 = 0.f, b2 = 0.f;
        // Sixteen blocks' pairs are requested TOGETHER, then added in block order.  Written as "load, add" per block the loop was
        // a chain of nblk dependent round trips to memory (the compiler cannot unroll a run-time trip count past its waits):
        // 11.5 us per launch for 10 MB, twenty-four launches per forward = 1.4 % of it (round 4: ~3 us).  Missing blocks read as
        // (0, 0): adding zero changes no sum, so the bits are the ones of the sequential loop.
        constexpr int U = 16;
        for (int b0 = 0; b0 < nblk; b0 += U) {
            float2 p[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                p[u] = b0 + u < nblk ? *(const float2*)(partials + 2 * ((int64_t)(b0 + u) * rows + r)) : make_float2(0.f, 0.f);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s1 += p[u].x;
                s2 += p[u].y;
                b2 = fmaxf(b2, p[u].y);
            }
        }
        const float mean = s1 / (float)dim;
        const float var = fmaxf(s2 / (float)dim - mean * mean, 0.f);
        const float rstd = 1.0f / sqrtf(var + eps);
        *(float2*)(stats + 2 * r) = make_float2(mean, rstd);
        if (r < guard_rows) { ratio = fabsf(mean) * rstd; bound = sqrtf(b2); }
    }
    if (guard) ln_guard_update(ratio, guard);   // (whole waves reach this: no early return above)
    if (amax_guard) ln_guard_update(bound, amax_guard);
}
// the same check on statistics that already exist (layer 0: written by the rowstats kernels)
__global__ void __launch_bounds__(256)
ln_guard_kernel(const float* __restrict__ stats, int64_t rows, unsigned int* __restrict__ guard) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float ratio = 0.f;
    if (r < rows) {
        const float2 st = *(const float2*)(stats + 2 * r);
        ratio = fabsf(st.x) * st.y;
    }
    ln_guard_update(ratio, guard);
}

// ---- folded LayerNorm: the weight side (the GEMM epilogues LNFOLD / RESID_LN of gemm_epilogue.h are the other half) ---------
// one wave per weight row n: W'[n,k] = T(scale*gamma[k]*W[n,k]); c[n] = sum_k float(W'[n,k]) (of the ROUNDED
// values, so that mean*c cancels exactly what the MFMA accumulates); d[n] = scale*(sum_k beta[k]*W[n,k] + b[n])
template <typename T>
__global__ void __launch_bounds__(256)
fold_ln_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
               const float* __restrict__ beta, int rows, int dim, float scale, typename T::elem* __restrict__ w16,
               float* __restrict__ c, float* __restrict__ d) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= rows) return;
    const float* wr = w + (int64_t)n * dim;
    float cs = 0.f, ds = 0.f;
    for (int k = lane; k < dim; k += 64) {
        const float wv = wr[k];
        const typename T::elem q = (typename T::elem)(scale * gamma[k] * wv);
        w16[(int64_t)n * dim + k] = q;
        cs += (float)q;
        ds = fmaf(beta[k], wv, ds);
    }
    cs = wave_sum(cs), ds = wave_sum(ds);
    if (lane == 0) { c[n] = cs; d[n] = scale * (ds + b[n]); }
}
// The same fold for e4m3 weights (fp8 path): W'[n,:] = scale * gamma o W[n,:] goes through the row quantiser; wscale[n] = s0;
// c[n] = s0 * sum_k decode(byte_k) (the sum of what the scaled MFMA multiplies, so that mean * c cancels it exactly); d[n] as
// above.  dim % 4 == 0.
__global__ void __launch_bounds__(256)
fold_ln_f8_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma,
                  const float* __restrict__ beta, int rows, int dim, float scale, uint8_t* __restrict__ w8,
                  float* __restrict__ wscale, float* __restrict__ c, float* __restrict__ d) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= rows) return;
    const f32x4* wr = (const f32x4*)(w + (int64_t)n * dim);
    const f32x4* gr = (const f32x4*)gamma;
    const f32x4* br = (const f32x4*)beta;
    const int n4 = dim >> 2;
    auto folded = [&](int k) {
        const f32x4 wv = wr[k], g = gr[k];
        return f32x4{scale * g[0] * wv[0], scale * g[1] * wv[1], scale * g[2] * wv[2], scale * g[3] * wv[3]};
    };
    const float s0 = e4m3_row_scale(lane, n4, folded);
    uint32_t* orow = (uint32_t*)(w8 + (int64_t)n * dim);
    float cs = 0.f, ds = 0.f;
    for (int k = lane; k < n4; k += 64) {
        const f32x4 wv = wr[k], be = br[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) ds = fmaf(be[j], wv[j], ds);
        const int q = (int)e4m3_quantise4(folded(k), s0);
        orow[k] = (uint32_t)q;
        cs += (__builtin_amdgcn_cvt_f32_fp8(q, 0) + __builtin_amdgcn_cvt_f32_fp8(q, 1)) +
              (__builtin_amdgcn_cvt_f32_fp8(q, 2) + __builtin_amdgcn_cvt_f32_fp8(q, 3));
    }
    cs = wave_sum(cs), ds = wave_sum(ds);
    if (lane == 0) { wscale[n] = s0; c[n] = s0 * cs; d[n] = scale * (ds + b[n]); }
}

// ---- fp8 weight quantisation: bytes + scale[r] = s0 * post ------------------------------------------------------------------
__global__ void __launch_bounds__(256)
quantize_rows_kernel(const float* __restrict__ w, int rows, int cols, float post, uint8_t* __restrict__ w8,
                     float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const f32x4* wr = (const f32x4*)(w + (int64_t)r * cols);
    const int n4 = cols >> 2;
    const float s0 = e4m3_row_scale(lane, n4, [&](int c) { return wr[c]; });
    uint32_t* orow = (uint32_t*)(w8 + (int64_t)r * cols);
    for (int c = lane; c < n4; c += 64) orow[c] = e4m3_quantise4(wr[c], s0);
    if (lane == 0) scale[r] = s0 * post;
}
// Weight-only e4m3 (VH_FLAG_W8_E4M3): out[r, :] = decode(quantise(w[r, :])) * s0 with the quantiser above -- the values
// a GEMM would see if the weight matrix were stored as e4m3 bytes + one scale per output channel and dequantised on its
// way to the matrix core.  The 16-bit weight preparation (cast / q|k|v packing / LayerNorm fold) then runs on `out`.
__global__ void __launch_bounds__(256)
fake_quant_rows_kernel(const float* __restrict__ w, int rows, int cols, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const f32x4* wr = (const f32x4*)(w + (int64_t)r * cols);
    const int n4 = cols >> 2;
    const float s0 = e4m3_row_scale(lane, n4, [&](int c) { return wr[c]; });
    f32x4* orow = (f32x4*)(out + (int64_t)r * cols);
    for (int c = lane; c < n4; c += 64) {
        const int q = (int)e4m3_quantise4(wr[c], s0);
        orow[c] = f32x4{__builtin_amdgcn_cvt_f32_fp8(q, 0) * s0, __builtin_amdgcn_cvt_f32_fp8(q, 1) * s0,
                        __builtin_amdgcn_cvt_f32_fp8(q, 2) * s0, __builtin_amdgcn_cvt_f32_fp8(q, 3) * s0};
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
static dim3 row_grid(int64_t rows) { return dim3((unsigned)((rows + 3) / 4)); }   // one wave per row, four per block

// (dtype, dim) -> launch(T{}, integral_constant<int, CH>{}): T as dispatch_dtype finds it, CH the first class of the ONE ladder
// that holds the row (dim <= 256 CH).  A dim beyond the ladder is hipErrorInvalidValue.
using RowClasses = std::integer_sequence<int, 1, 2, 3, 4, 5, 8>;
template <typename T, typename F, int... CH>
static bool dispatch_ch(int dim, F& launch, std::integer_sequence<int, CH...>) {
    return ((dim <= 256 * CH ? (launch(T{}, std::integral_constant<int, CH>{}), true) : false) || ...);
}
template <typename... Ts, typename F>
static hipError_t dispatch_row(int dtype, int dim, F&& launch) {
    return dispatch_dtype<Ts...>(dtype, [&](auto t) {
        return dispatch_ch<decltype(t)>(dim, launch, RowClasses{}) ? hipGetLastError() : hipErrorInvalidValue;
    });
}

hipError_t launch_layernorm(const float* x, int64_t rows, int dim, int64_t row_stride, const float* gamma,
                            const float* beta, float eps, void* out16, int dtype, hipStream_t s) {
    if (rows <= 0 || dim <= 0 || (dim & 3) || (row_stride & 3)) return hipErrorInvalidValue;
    return dispatch_row<F32OUT, E4M3, BF16, FP16>(dtype, dim, [&](auto t, auto ch) {
        using T = decltype(t);
        hipLaunchKernelGGL((layernorm_kernel<T, decltype(ch)::value>), row_grid(rows), dim3(256), 0, s, x, rows, dim, row_stride, gamma, beta,
                           eps, (typename T::elem*)out16);
    });
}

// lo == NULL: the plain cast.  e4m3: a copy of the raw rows (fp8 path, folded LN), with lo the bf16 plane; amax_guard belongs to
// e4m3 rows, the 16-bit kernels do not look at it.
static hipError_t rowstats(const float* x, int64_t rows, int dim, float eps, void* hi, void* lo, float* stats, int dtype, hipStream_t s,
                           int64_t guard_rows, unsigned int* amax_guard) {
    if (rows <= 0 || dim <= 0 || (dim & 3)) return hipErrorInvalidValue;
    return dispatch_row<E4M3, BF16, FP16>(dtype, dim, [&](auto t, auto ch) {
        using T = decltype(t);
        hipLaunchKernelGGL((rowstats_cast_kernel<T, decltype(ch)::value>), row_grid(rows), dim3(256), 0, s, x, rows, dim, eps,
                           (typename T::elem*)hi, stats, lo, guard_rows, amax_guard);
    });
}
hipError_t launch_rowstats_cast(const float* x, int64_t rows, int dim, float eps, void* x16, float* stats, int dtype,
                                hipStream_t s, int64_t guard_rows, unsigned int* amax_guard) {
    return rowstats(x, rows, dim, eps, x16, nullptr, stats, dtype, s, guard_rows, amax_guard);
}
hipError_t launch_rowstats_split(const float* x, int64_t rows, int dim, float eps, void* hi, void* lo, float* stats, int dtype,
                                 hipStream_t s, int64_t guard_rows, unsigned int* amax_guard) {
    if (!lo) return hipErrorInvalidValue;
    return rowstats(x, rows, dim, eps, hi, lo, stats, dtype, s, guard_rows, amax_guard);
}

hipError_t launch_pre_layernorm(const float* x, int64_t rows, int dim, const float* gamma, const float* beta, float eps, float* y32,
                                void* hi, void* lo, float* stats, int dtype, hipStream_t s, int64_t guard_rows, unsigned int* guard,
                                unsigned int* amax_guard) {
    if (rows <= 0 || dim <= 0 || (dim & 3) || !x || !gamma || !beta || (!y32 && !hi) || (lo && !hi)) return hipErrorInvalidValue;
    return dispatch_row<E4M3, BF16, FP16>(dtype, dim, [&](auto t, auto ch) {
        using T = decltype(t);
        hipLaunchKernelGGL((pre_layernorm_kernel<T, decltype(ch)::value>), row_grid(rows), dim3(256), 0, s, x, rows, dim, gamma, beta, eps,
                           y32, (typename T::elem*)hi, lo, stats, guard_rows, guard, amax_guard);
    });
}

hipError_t launch_layernorm_split(const void* hi, const void* lo, int64_t rows, int dim, int64_t row_stride, const float* gamma,
                                  const float* beta, float eps, float* out32, int dtype, hipStream_t s) {
    if (rows <= 0 || dim <= 0) return hipErrorInvalidValue;
    return dispatch_dtype<E4M3, BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(layernorm_split_kernel<T>, row_grid(rows), dim3(256), 0, s, (const typename T::elem*)hi, lo, rows, dim,
                           row_stride, gamma, beta, eps, out32);
        return hipGetLastError();
    });
}

hipError_t launch_finalize_stats(const float* partials, int nblk, int64_t rows, int dim, float eps, float* stats, hipStream_t s,
                                 int64_t guard_rows, unsigned int* guard, unsigned int* amax_guard) {
    if (rows <= 0 || nblk <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(finalize_stats_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, partials, nblk, rows, dim, eps, stats,
                       guard_rows, guard, amax_guard);
    return hipGetLastError();
}
hipError_t launch_ln_guard(const float* stats, int64_t rows, unsigned int* guard, hipStream_t s) {
    if (rows <= 0 || !guard) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ln_guard_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, stats, rows, guard);
    return hipGetLastError();
}

hipError_t launch_fold_ln(const float* w, const float* b, const float* gamma, const float* beta, int rows, int dim,
                          float scale, void* w16, float* c, float* d, int dtype, hipStream_t s) {
    if (rows <= 0 || dim <= 0) return hipErrorInvalidValue;
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(fold_ln_kernel<T>, row_grid(rows), dim3(256), 0, s, w, b, gamma, beta, rows, dim, scale, (typename T::elem*)w16, c, d);
        return hipGetLastError();
    });
}
hipError_t launch_fold_ln_f8(const float* w, const float* b, const float* gamma, const float* beta, int rows, int dim,
                             float scale, void* w8, float* wscale, float* c, float* d, hipStream_t s) {
    if (rows <= 0 || dim <= 0 || (dim & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fold_ln_f8_kernel, row_grid(rows), dim3(256), 0, s, w, b, gamma, beta, rows, dim, scale, (uint8_t*)w8, wscale, c, d);
    return hipGetLastError();
}

hipError_t launch_quantize_rows(const float* w, int rows, int cols, float post, void* w8, float* scale, hipStream_t s) {
    if (rows <= 0 || cols <= 0 || (cols & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(quantize_rows_kernel, row_grid(rows), dim3(256), 0, s, w, rows, cols, post, (uint8_t*)w8, scale);
    return hipGetLastError();
}
hipError_t launch_fake_quant_rows(const float* w, int rows, int cols, float* out, hipStream_t s) {
    if (rows <= 0 || cols <= 0 || (cols & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fake_quant_rows_kernel, row_grid(rows), dim3(256), 0, s, w, rows, cols, out);
    return hipGetLastError();
}

}  // namespace vh
