// kernels_misc.hip — the small pieces around the GEMMs (gfx950) that are no one-wave-per-row kernel (those: kernels_rows.hip):
// patch gather (im2col + cast), the leading rows of every image, casts and weight re-layout, the synthetic-data fill, MLP mode,
// the 3x3 filter and the fp32 head.
#include "vh_kernels.h"

namespace vh {

// ---- im2col + cast: NHWC fp32 image -> patch matrix [batch*np, patch*patch*ch] 16-bit -------
// one float4 per thread; a patch row is `patch*ch` contiguous floats of the image, and lands as
// `patch*ch` contiguous 16-bit elements of the patch matrix, so both sides are coalesced.
template <typename T>
__global__ void __launch_bounds__(256)
im2col_kernel(const float* __restrict__ in, typename T::elem* __restrict__ out, int64_t n4, int image,
              int patch, int ch) {
    const int rowf4 = image * ch / 4;      // float4 per image row
    const int prf4 = patch * ch / 4;       // float4 per patch row
    const int g = image / patch;
    const int kp = patch * patch * ch;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n4; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rowidx = f / rowf4;  // b*image + y
        const int q = (int)(f - rowidx * rowf4);
        const int64_t b = rowidx / image;
        const int y = (int)(rowidx - b * image);
        const int px = q / prf4, r = q - px * prf4;
        const int py = y / patch, ky = y - py * patch;
        const f32x4 v = ((const f32x4*)in)[f];
        const int64_t orow = (b * g + py) * g + px;
        *(typename T::vec4*)(out + orow * kp + ky * patch * ch + r * 4) = pack4<T>(v[0], v[1], v[2], v[3]);
    }
}

// ---- im2col + cast into a row padded to kpad columns (any patch * ch; kpad >= patch^2 * ch, 8 | kpad) ---------------------
// one thread owns 8 consecutive output elements and stores them as one 16-byte vector; consecutive lanes own consecutive
// chunks of a row.  Element k is (ky, kx, c) of the same k order as im2col_kernel; columns kp <= k < kpad are written as
// zero on every call (the patch-matrix buffer is scratch for the class-token tail in between).
template <typename T>
__global__ void __launch_bounds__(256)
im2col_pad_kernel(const float* __restrict__ in, typename T::elem* __restrict__ out, int64_t n8, int image, int patch,
                  int ch, int kpad) {
    const int pc = patch * ch;               // floats per patch row: contiguous in the image
    const int kp = patch * pc;
    const int cpr = kpad / 8;                // chunks per output row
    const int g = image / patch;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n8; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t orow = f / cpr;        // (b * g + py) * g + px
        const int k0 = (int)(f - orow * cpr) * 8;
        const int64_t b = orow / (g * g);
        const int p = (int)(orow - b * g * g);
        const int py = p / g, px = p - py * g;
        const float* src = in + ((b * image + (int64_t)py * patch) * image + (int64_t)px * patch) * ch;
        int ky = k0 / pc, r = k0 - ky * pc;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = k0 + i < kp ? src[((int64_t)ky * image) * ch + r] : 0.f;
            if (++r == pc) { r = 0; ++ky; }
        }
        const typename T::vec4 lo = pack4<T>(v[0], v[1], v[2], v[3]), hi = pack4<T>(v[4], v[5], v[6], v[7]);
        *(typename T::vec8*)(out + f * 8) = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

hipError_t launch_im2col(const float* in, int batch, int image, int patch, int channels, int kpad, void* out16, int dtype,
                         hipStream_t s) {
    if (patch <= 0 || image % patch) return hipErrorInvalidValue;
    const int kp = patch * patch * channels;
    if (kpad != kp || (patch * channels) % 4) {
        if (kpad < kp || kpad % 8) return hipErrorInvalidValue;
        const int g = image / patch;
        const int64_t n8 = (int64_t)batch * g * g * (kpad / 8);
        const unsigned grid = (unsigned)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384);
        return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(im2col_pad_kernel<T>, dim3(grid), dim3(256), 0, s, in, (typename T::elem*)out16, n8, image, patch, channels, kpad);
            return hipGetLastError();
        });
    }
    const int64_t n4 = (int64_t)batch * image * image * channels / 4;
    const unsigned grid = (unsigned)((n4 + 255) / 256 < 16384 ? (n4 + 255) / 256 : 16384);
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(im2col_kernel<T>, dim3(grid), dim3(256), 0, s, in, (typename T::elem*)out16, n4, image, patch, channels);
        return hipGetLastError();
    });
}

// ---- im2col of 8-bit NHWC images with the input normalisation fused in ---------------------------------------------------
// Pixel p (0..255) of channel c enters as x = fmaf((float)p, scale[c], shift[c]) -- ONE rounding, written as the builtin so
// that nothing depends on contraction -- and is then rounded by the same pack4<T> as in the kernels above: the patch matrix has
// the bits launch_im2col produces from the host-computed fp32 array x.  Same thread mapping, k order and zero padding as
// im2col_pad_kernel.  VEC8 (8 | patch * ch, 8 | image * ch, 8-byte aligned base): the 8 source bytes of a chunk are contiguous
// and 8-byte aligned in the image, one load; otherwise byte loads with the per-element (ky, r) walk.  The channel of element k
// is k % ch (patch * ch is a multiple of ch).  scale | shift arrive as kernel arguments and are put in LDS once per block.
struct U8Norm { float scale[kMaxChannels], shift[kMaxChannels]; };

template <typename T, bool VEC8>
__global__ void __launch_bounds__(256)
im2col_u8_kernel(const uint8_t* __restrict__ in, typename T::elem* __restrict__ out, int64_t n8, int image, int patch,
                 int ch, int kpad, const U8Norm norm) {
    __shared__ float s_scale[kMaxChannels], s_shift[kMaxChannels];
    if ((int)threadIdx.x < ch) {
        s_scale[threadIdx.x] = norm.scale[threadIdx.x];
        s_shift[threadIdx.x] = norm.shift[threadIdx.x];
    }
    __syncthreads();
    const int pc = patch * ch;               // bytes per patch row: contiguous in the image
    const int kp = patch * pc;
    const int cpr = kpad / 8;                // chunks per output row
    const int g = image / patch;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n8; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t orow = f / cpr;        // (b * g + py) * g + px
        const int k0 = (int)(f - orow * cpr) * 8;
        const int64_t b = orow / (g * g);
        const int p = (int)(orow - b * g * g);
        const int py = p / g, px = p - py * g;
        const uint8_t* src = in + ((b * image + (int64_t)py * patch) * image + (int64_t)px * patch) * ch;
        int ky = k0 / pc, r = k0 - ky * pc;
        int c = k0 % ch;
        float v[8];
        if constexpr (VEC8) {                // 8 | pc and 8 | kp: the chunk lies inside one patch row, or wholly in the padding
            u32x2 w{0u, 0u};
            if (k0 < kp) w = *(const u32x2*)(src + ((int64_t)ky * image) * ch + r);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float pix = (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
                v[i] = k0 < kp ? __builtin_fmaf(pix, s_scale[c], s_shift[c]) : 0.f;
                if (++c == ch) c = 0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[i] = k0 + i < kp ? __builtin_fmaf((float)src[((int64_t)ky * image) * ch + r], s_scale[c], s_shift[c]) : 0.f;
                if (++r == pc) { r = 0; ++ky; }
                if (++c == ch) c = 0;
            }
        }
        const typename T::vec4 lo = pack4<T>(v[0], v[1], v[2], v[3]), hi = pack4<T>(v[4], v[5], v[6], v[7]);
        *(typename T::vec8*)(out + f * 8) = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

hipError_t launch_im2col_u8(const uint8_t* in, int batch, int image, int patch, int channels, int kpad, const float* scale,
                            const float* shift, void* out16, int dtype, hipStream_t s) {
    if (patch <= 0 || image % patch || channels < 1 || channels > kMaxChannels || batch < 1) return hipErrorInvalidValue;
    const int kp = patch * patch * channels;
    if (kpad < kp || kpad % 8) return hipErrorInvalidValue;
    U8Norm norm;
    for (int c = 0; c < kMaxChannels; ++c) {
        norm.scale[c] = c < channels ? scale[c] : 0.f;
        norm.shift[c] = c < channels ? shift[c] : 0.f;
    }
    const int g = image / patch;
    const int64_t n8 = (int64_t)batch * g * g * (kpad / 8);
    const unsigned grid = (unsigned)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384);
    const bool vec8 = (patch * channels) % 8 == 0 && (image * channels) % 8 == 0 && ((uintptr_t)in & 7) == 0;
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, in, (typename T::elem*)out16, n8, image, patch, channels, kpad, norm); };
        if (vec8) go(im2col_u8_kernel<T, true>);
        else go(im2col_u8_kernel<T, false>);
        return hipGetLastError();
    });
}

// ---- the leading rows of every image: x[b, 0, :] = cls + pos[0], x[b, 1 + r, :] = reg[r] (register tokens) ----
// lead = NCLS + R rows per image; reg is not read when lead == NCLS.  NCLS = 0 (VH_FLAG_NO_CLS): every leading row is a register
// row, cls and pos are not read
template <int NCLS>
__global__ void lead_rows_kernel(float* __restrict__ x, const float* __restrict__ cls, const float* __restrict__ pos,
                                 const float* __restrict__ reg, int lead, int batch, int tokens, int dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)lead * dim;
    if (i >= (int64_t)batch * per) return;
    const int b = (int)(i / per);
    const int e = (int)(i - (int64_t)b * per);   // row j = e / dim of the image, column e % dim: the rows are contiguous
    if constexpr (NCLS) x[(int64_t)b * tokens * dim + e] = e < dim ? cls[e] + pos[e] : reg[e - dim];
    else x[(int64_t)b * tokens * dim + e] = reg[e];
}
hipError_t launch_lead_rows(float* x, const float* cls, const float* pos, const float* reg, int lead, int batch, int tokens, int dim,
                            hipStream_t s) {
    const int ncls = cls ? 1 : 0;
    if (batch <= 0 || lead < ncls || lead >= tokens + ncls || (lead > ncls && !reg) || (cls && !pos)) return hipErrorInvalidValue;
    if (lead == 0) return hipSuccess;   // no class token, no register: the patch rows are the whole image
    const int64_t n = (int64_t)batch * lead * dim;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (cls) hipLaunchKernelGGL(lead_rows_kernel<1>, grid, dim3(256), 0, s, x, cls, pos, reg, lead, batch, tokens, dim);
    else hipLaunchKernelGGL(lead_rows_kernel<0>, grid, dim3(256), 0, s, x, cls, pos, reg, lead, batch, tokens, dim);
    return hipGetLastError();
}

// the same rows for the SPLIT residual (PATCH_SPLIT path): planes hi = T(x), lo = lo8(x - hi) of x = cls + pos[0] or reg[r], and
// the row's (sum, sum of squares) per 64-column block -- what the patch GEMM's epilogue writes for every other row.  One wave
// per (image, leading row); a lane owns column 64 * blk + lane of every block; fixed-order butterfly sums.
// NCLS = 0 (VH_FLAG_NO_CLS): every leading row is a register row (row j = reg[j]), cls and pos are not read.
template <typename T, int NCLS>
__global__ void __launch_bounds__(256)
lead_rows_split_kernel(typename T::elem* __restrict__ hi, uint8_t* __restrict__ lo, float* __restrict__ partials, int64_t prow,
                       const float* __restrict__ cls, const float* __restrict__ pos, const float* __restrict__ reg, int lead,
                       int batch, int tokens, int dim) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = w / lead, j = w - b * lead;
    if (b >= batch) return;
    const int64_t row = (int64_t)b * tokens + j;
    const bool is_reg = NCLS == 0 || j != 0;
    const float* const src = is_reg ? reg + (int64_t)(j - NCLS) * dim : cls;
    for (int blk = 0; blk * 64 < dim; ++blk) {
        const int d = blk * 64 + lane;
        float v = 0.f;
        if (d < dim) {
            v = is_reg ? src[d] : src[d] + pos[d];
            const typename T::elem h = (typename T::elem)v;
            hi[row * dim + d] = h;
            lo[row * dim + d] = lo8_pack1<T>(v - (float)h);
        }
        const float s1 = wave_sum(v), s2 = wave_sum(v * v);
        if (lane == 0) *(float2*)(partials + 2 * ((int64_t)blk * prow + row)) = make_float2(s1, s2);
    }
}
hipError_t launch_lead_rows_split(void* hi, void* lo, float* partials, int64_t prow, const float* cls, const float* pos, const float* reg,
                                  int lead, int batch, int tokens, int dim, int dtype, hipStream_t s) {
    const int ncls = cls ? 1 : 0;
    if (batch <= 0 || dim % 64 || lead < ncls || lead >= tokens + ncls || (lead > ncls && !reg) || (cls && !pos) || prow < (int64_t)batch * tokens)
        return hipErrorInvalidValue;
    if (lead == 0) return hipSuccess;   // no class token, no register: the patch rows are the whole image
    const dim3 grid((unsigned)(((int64_t)batch * lead + 3) / 4));
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        if (cls) hipLaunchKernelGGL((lead_rows_split_kernel<T, 1>), grid, dim3(256), 0, s, (typename T::elem*)hi, (uint8_t*)lo, partials, prow, cls, pos, reg, lead, batch, tokens, dim);
        else hipLaunchKernelGGL((lead_rows_split_kernel<T, 0>), grid, dim3(256), 0, s, (typename T::elem*)hi, (uint8_t*)lo, partials, prow, cls, pos, reg, lead, batch, tokens, dim);
        return hipGetLastError();
    });
}

// ---- fp32 -> 16-bit cast -----------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cast_kernel(const float* __restrict__ in, typename T::elem* __restrict__ out, int64_t n4) {
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n4; f += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 v = ((const f32x4*)in)[f];
        ((typename T::vec4*)out)[f] = pack4<T>(v[0], v[1], v[2], v[3]);
    }
}
hipError_t launch_cast(const float* in, void* out16, int64_t n, int dtype, hipStream_t s) {
    if (n <= 0 || (n & 3)) return hipErrorInvalidValue;
    const int64_t n4 = n / 4;
    const unsigned grid = (unsigned)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
    return dispatch_dtype<E4M3, BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(cast_kernel<T>, dim3(grid), dim3(256), 0, s, in, (typename T::elem*)out16, n4);
        return hipGetLastError();
    });
}

// W fp32 [rows, cols] -> 16-bit in the TILED layout the MLP hidden activation has (gemm_epilogue.h OTILED, kernels_gemm5.hip AT):
// [row / 16][cols / 8 chunks][16 rows][8 values], natural column order.  One thread per destination chunk.
template <typename T>
__global__ void __launch_bounds__(256) cast_tiled_w_kernel(const float* __restrict__ w, typename T::elem* __restrict__ out, int rows, int cols) {
    const int64_t nchunk = (int64_t)rows * (cols >> 3);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * blockDim.x) {
        const int r16 = (int)(i & 15);
        const int64_t bc = i >> 4;                        // block * (cols / 8) + chunk
        const int chunk = (int)(bc % (cols >> 3)), block = (int)(bc / (cols >> 3));
        const float* src = w + (int64_t)(block * 16 + r16) * cols + chunk * 8;
        const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
        const typename T::vec4 lo = pack4<T>(a[0], a[1], a[2], a[3]), hi = pack4<T>(b[0], b[1], b[2], b[3]);
        *(typename T::vec8*)(out + i * 8) = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
hipError_t launch_cast_tiled_w(const float* w, int rows, int cols, void* w16, int dtype, hipStream_t s) {
    if (rows <= 0 || cols <= 0 || (rows & 15) || (cols & 7)) return hipErrorInvalidValue;
    const int64_t nchunk = (int64_t)rows * (cols >> 3);
    const unsigned grid = (unsigned)((nchunk + 255) / 256 < 8192 ? (nchunk + 255) / 256 : 8192);
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(cast_tiled_w_kernel<T>, dim3(grid), dim3(256), 0, s, w, (typename T::elem*)w16, rows, cols);
        return hipGetLastError();
    });
}

// e4m3 weights (one byte per element, rows of `cols` bytes) once more in the tiled layout of the e4m3 operand:
// [rows / 16][cols / 16 chunks][16 rows][16 B] -- a copy of 16-byte pieces, nothing is converted
__global__ void __launch_bounds__(256) tile_bytes_kernel(const u32x4* __restrict__ w, u32x4* __restrict__ out, int rows, int cols) {
    const int cpr = cols >> 4;   // chunks per row
    const int64_t nchunk = (int64_t)rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * blockDim.x) {
        const int r16 = (int)(i & 15);
        const int64_t bc = i >> 4;                        // block * cpr + chunk
        const int chunk = (int)(bc % cpr), block = (int)(bc / cpr);
        out[i] = w[(int64_t)(block * 16 + r16) * cpr + chunk];
    }
}
hipError_t launch_tile_bytes(const void* w8, int rows, int cols, void* out, hipStream_t s) {
    if (rows <= 0 || cols <= 0 || (rows & 15) || (cols & 15)) return hipErrorInvalidValue;
    const int64_t nchunk = (int64_t)rows * (cols >> 4);
    const unsigned grid = (unsigned)((nchunk + 255) / 256 < 8192 ? (nchunk + 255) / 256 : 8192);
    hipLaunchKernelGGL(tile_bytes_kernel, dim3(grid), dim3(256), 0, s, (const u32x4*)w8, (u32x4*)out, rows, cols);
    return hipGetLastError();
}

// ---- synthetic data ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fill_kernel(float* __restrict__ out, int64_t n, uint64_t stream, int kind,
                                                   double scale, float offset) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float v;
        if (kind == 0) v = rng_uniform(stream, (uint64_t)i);
        else if (kind == 1) v = rng_ih4(stream, (uint64_t)i, scale, offset);
        else v = offset;
        out[i] = v;
    }
}
hipError_t launch_fill(float* out, int64_t n, uint64_t seed, uint32_t tensor_id, int kind, float sigma, float offset,
                       hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
    hipLaunchKernelGGL(fill_kernel, dim3(grid), dim3(256), 0, s, out, n, rng_stream(seed, tensor_id), kind,
                       (double)sigma / kIH4Std, offset);
    return hipGetLastError();
}

// ---- weight re-layout ---------------------------------------------------------------------------
// Wqkv[3D, D] = [q * q_scale ; k ; v] (16-bit), bqkv[3D] = [bq * q_scale ; bk ; bv] (fp32).
// q_scale = 64^-1/2 = 0.125 is a power of two, so folding it into the weights is exact.
template <typename T>
__global__ void __launch_bounds__(256)
pack_qkv_kernel(const float* __restrict__ qw, const float* __restrict__ qb, const float* __restrict__ kw,
                const float* __restrict__ kb, const float* __restrict__ vw, const float* __restrict__ vb, int dim,
                float q_scale, typename T::elem* __restrict__ w16, float* __restrict__ b32) {
    const int64_t dd = (int64_t)dim * dim;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * dd) {
        const int which = (int)(i / dd);
        const int64_t j = i - which * dd;
        const float v = which == 0 ? qw[j] * q_scale : (which == 1 ? kw[j] : vw[j]);
        w16[i] = (typename T::elem)v;
    }
    if (i < 3 * dim) {
        const int which = (int)(i / dim), j = (int)(i - (int64_t)which * dim);
        b32[i] = which == 0 ? qb[j] * q_scale : (which == 1 ? kb[j] : vb[j]);
    }
}
hipError_t launch_pack_qkv(const float* qw, const float* qb, const float* kw, const float* kb, const float* vw,
                           const float* vb, int dim, float q_scale, void* w16, float* b32, int dtype, hipStream_t s) {
    const int64_t n = 3 * (int64_t)dim * dim;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(pack_qkv_kernel<T>, grid, block, 0, s, qw, qb, kw, kb, vw, vb, dim, q_scale, (typename T::elem*)w16, b32);
        return hipGetLastError();
    });
}

// conv kernel [D][c][ky][kx] fp32 -> [D][(ky*P + kx)*C + c] 16-bit: the k-order of an NHWC patch
template <typename T>
__global__ void __launch_bounds__(256)
permute_patch_kernel(const float* __restrict__ w, int dim, int ch, int patch, typename T::elem* __restrict__ o) {
    const int kp = patch * patch * ch;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)dim * kp) return;
    const int d = (int)(i / kp), k = (int)(i - (int64_t)d * kp);
    const int c = k % ch, kx = (k / ch) % patch, ky = k / (ch * patch);
    o[i] = (typename T::elem)w[(((int64_t)d * ch + c) * patch + ky) * patch + kx];
}
// the same into rows of kpad columns, zeros in the columns kp <= k < kpad
template <typename T>
__global__ void __launch_bounds__(256)
permute_patch_pad_kernel(const float* __restrict__ w, int dim, int ch, int patch, int kpad, typename T::elem* __restrict__ o) {
    const int kp = patch * patch * ch;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)dim * kpad) return;
    const int d = (int)(i / kpad), k = (int)(i - (int64_t)d * kpad);
    const int c = k % ch, kx = (k / ch) % patch, ky = k / (ch * patch);
    o[i] = (typename T::elem)(k < kp ? w[(((int64_t)d * ch + c) * patch + ky) * patch + kx] : 0.f);
}
hipError_t launch_permute_patch(const float* w, int dim, int channels, int patch, int kpad, void* w16, int dtype, hipStream_t s) {
    if (kpad != patch * patch * channels || (patch * channels) % 4) {
        if (kpad < patch * patch * channels) return hipErrorInvalidValue;
        const int64_t n = (int64_t)dim * kpad;
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(permute_patch_pad_kernel<T>, grid, block, 0, s, w, dim, channels, patch, kpad, (typename T::elem*)w16);
            return hipGetLastError();
        });
    }
    const int64_t n = (int64_t)dim * patch * patch * channels;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(permute_patch_kernel<T>, grid, block, 0, s, w, dim, channels, patch, (typename T::elem*)w16);
        return hipGetLastError();
    });
}

// ---- MLP mode: one dense layer, fp32 exact products, one wave per output neuron ----------------------
// y[v, j] = act(b[j] + sum_k W[j, k] x[v, k]) — the body of the reference's network_v1 layer loop
// (argument layout netFPGA.cpp:427-436; weights row-major [n_out, n_in], netFPGA.cpp:94-105).
__device__ __forceinline__ float act_apply(int act, float v) {
    switch (act) {
    case VH_ACT_RELU2: return fminf(fmaxf(v, 0.f), 1.f);
    case VH_ACT_RELU: return fmaxf(v, 0.f);
    case VH_ACT_HARDTANH: return fminf(fmaxf(v, -1.f), 1.f);
    case VH_ACT_GELU: return gelu_erf(v);
    default: return v;
    }
}
// `z` (optional): the pre-activations, kept for the backward pass of MLP-mode training
__global__ void __launch_bounds__(256)
dense_layer_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ x,
                   float* __restrict__ y, int n_in, int n_out, int n_vec, int act, float* __restrict__ z) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_out) return;
    const float* wr = w + (int64_t)j * n_in;
    for (int v = 0; v < n_vec; ++v) {
        const float* xv = x + (int64_t)v * n_in;
        float s = 0.f;
        for (int k = lane; k < n_in; k += 64) s = fmaf(wr[k], xv[k], s);
        s = wave_sum(s);
        if (lane == 0) {
            const float pre = s + b[j];
            if (z) z[(int64_t)v * n_out + j] = pre;
            y[(int64_t)v * n_out + j] = act_apply(act, pre);
        }
    }
}
hipError_t launch_dense_layer(const float* w, const float* b, const float* x, float* y, int n_in, int n_out, int n_vec,
                              int activation, hipStream_t s, float* z) {
    hipLaunchKernelGGL(dense_layer_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, s, w, b, x, y, n_in, n_out,
                       n_vec, activation, z);
    return hipGetLastError();
}

// ---- MLP-mode training (init_gradient / launch_gradient, netFPGA.cpp:518-580: commented-out code in the reference; the
// definitions are this build's -- include/vithip.h, oracle/mlp_oracle.c).  Small fp32 kernels, every sum in a fixed order.
__device__ __forceinline__ float act_deriv(int act, float z) {
    switch (act) {
    case VH_ACT_RELU2: return (z > 0.f && z < 1.f) ? 1.f : 0.f;
    case VH_ACT_RELU: return z > 0.f ? 1.f : 0.f;
    case VH_ACT_HARDTANH: return (z > -1.f && z < 1.f) ? 1.f : 0.f;
    case VH_ACT_GELU: return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
    default: return 1.f;
    }
}
// last layer: d = (a - t) * act'(z); err = sum |a - t| over all sets and outputs.  ONE workgroup: every thread adds its
// elements in index order, then a fixed tree -- the same bits on every run.
__global__ void __launch_bounds__(1024)
mlp_out_delta_kernel(const float* __restrict__ a, const float* __restrict__ z, const float* __restrict__ t, float* __restrict__ d,
                     int64_t n, int act, float* __restrict__ err) {
    __shared__ float part[1024];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const float e = a[i] - t[i];
        s += fabsf(e);
        d[i] = e * act_deriv(act, z[i]);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *err = part[0];
}
// hidden layer: d_prev[j][i] = act'(z_prev[j][i]) * sum_o W[o][i] d[j][o]   (W of the layer ABOVE, before its update)
__global__ void __launch_bounds__(256)
mlp_back_delta_kernel(const float* __restrict__ w, const float* __restrict__ d, const float* __restrict__ z_prev,
                      float* __restrict__ d_prev, int n_in, int n_out, int act) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= n_in) return;
    const float* dj = d + (int64_t)j * n_out;
    float s = 0.f;
    for (int o = 0; o < n_out; ++o) s = fmaf(w[(int64_t)o * n_in + i], dj[o], s);
    d_prev[(int64_t)j * n_in + i] = s * act_deriv(act, z_prev[(int64_t)j * n_in + i]);
}
// W[o][k] -= scale * sum_j d[j][o] x[j][k];  b[o] -= scale * sum_j d[j][o]     (scale = multiplier / n_sets)
__global__ void __launch_bounds__(256)
mlp_update_kernel(float* __restrict__ w, float* __restrict__ b, const float* __restrict__ d, const float* __restrict__ x,
                  int n_in, int n_out, int n_sets, float scale) {
    const int k = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
    if (k < n_in) {
        float g = 0.f;
        for (int j = 0; j < n_sets; ++j) g = fmaf(d[(int64_t)j * n_out + o], x[(int64_t)j * n_in + k], g);
        w[(int64_t)o * n_in + k] -= scale * g;
    }
    if (k == 0) {
        float gb = 0.f;
        for (int j = 0; j < n_sets; ++j) gb += d[(int64_t)j * n_out + o];
        b[o] -= scale * gb;
    }
}
hipError_t launch_mlp_out_delta(const float* a, const float* z, const float* t, float* d, int64_t n, int act, float* err, hipStream_t s) {
    hipLaunchKernelGGL(mlp_out_delta_kernel, dim3(1), dim3(1024), 0, s, a, z, t, d, n, act, err);
    return hipGetLastError();
}
hipError_t launch_mlp_back_delta(const float* w, const float* d, const float* z_prev, float* d_prev, int n_in, int n_out, int n_sets,
                                 int act, hipStream_t s) {
    hipLaunchKernelGGL(mlp_back_delta_kernel, dim3((unsigned)((n_in + 255) / 256), (unsigned)n_sets), dim3(256), 0, s, w, d, z_prev, d_prev,
                       n_in, n_out, act);
    return hipGetLastError();
}
hipError_t launch_mlp_update(float* w, float* b, const float* d, const float* x, int n_in, int n_out, int n_sets, float scale, hipStream_t s) {
    hipLaunchKernelGGL(mlp_update_kernel, dim3((unsigned)((n_in + 255) / 256), (unsigned)n_out), dim3(256), 0, s, w, b, d, x, n_in, n_out,
                       n_sets, scale);
    return hipGetLastError();
}

// ---- 3x3 image filter on 8-bit single-channel frames (the reference's filter_image pipeline) --------------------
// The reference's kernel `image_process` is absent (netFPGA.cpp:305 names it, no source, no bitstream), so its
// arithmetic is a documented choice here: KIND 0 = 3x3 binomial blur (1 2 1 / 2 4 2 / 1 2 1, +8 >> 4), KIND 1 =
// Sobel |gx| + |gy| saturated to 255; borders replicate the edge pixel.  Integer arithmetic: bit-exact against
// the oracle.  HBM-bound (1 byte in + 1 byte out per pixel); a thread produces 4 adjacent pixels from 3 x 6 inputs.
template <int KIND>
__global__ void __launch_bounds__(256) filter3x3_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int h, int w) {
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x0 >= w) return;
    int p[3][6];
    const bool fast = (w & 3) == 0 && x0 >= 4 && x0 + 8 <= w;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        int yy = y + r - 1;
        yy = yy < 0 ? 0 : (yy >= h ? h - 1 : yy);
        const uint8_t* row = in + (int64_t)yy * w;
        if (fast) {
            const uint32_t a = *(const uint32_t*)(row + x0 - 4), b = *(const uint32_t*)(row + x0), c = *(const uint32_t*)(row + x0 + 4);
            p[r][0] = a >> 24;
            p[r][1] = b & 0xFF; p[r][2] = (b >> 8) & 0xFF; p[r][3] = (b >> 16) & 0xFF; p[r][4] = b >> 24;
            p[r][5] = c & 0xFF;
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                int xx = x0 + i - 1;
                xx = xx < 0 ? 0 : (xx >= w ? w - 1 : xx);
                p[r][i] = row[xx];
            }
        }
    }
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int v;
        if (KIND == 0) {
            v = (p[0][i] + 2 * p[0][i + 1] + p[0][i + 2] + 2 * (p[1][i] + 2 * p[1][i + 1] + p[1][i + 2]) + p[2][i] + 2 * p[2][i + 1] + p[2][i + 2] + 8) >> 4;
        } else {
            const int gx = (p[0][i + 2] + 2 * p[1][i + 2] + p[2][i + 2]) - (p[0][i] + 2 * p[1][i] + p[2][i]);
            const int gy = (p[2][i] + 2 * p[2][i + 1] + p[2][i + 2]) - (p[0][i] + 2 * p[0][i + 1] + p[0][i + 2]);
            v = (gx < 0 ? -gx : gx) + (gy < 0 ? -gy : gy);
            v = v > 255 ? 255 : v;
        }
        packed |= (uint32_t)v << (8 * i);
    }
    uint8_t* o = out + (int64_t)y * w + x0;
    if ((w & 3) == 0) *(uint32_t*)o = packed;
    else
        for (int i = 0; i < 4 && x0 + i < w; ++i) o[i] = (uint8_t)(packed >> (8 * i));
}
hipError_t launch_filter3x3(const uint8_t* in, uint8_t* out, int h, int w, int kind, hipStream_t s) {
    if (h <= 0 || w <= 0 || (kind != 0 && kind != 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((w + 1023) / 1024), (unsigned)h), block(256);
    if (kind == 0) hipLaunchKernelGGL(filter3x3_kernel<0>, grid, block, 0, s, in, out, h, w);
    else hipLaunchKernelGGL(filter3x3_kernel<1>, grid, block, 0, s, in, out, h, w);
    return hipGetLastError();
}

// ---- classifier head in fp32 --------------------------------------------------------------------------------------
//   logits[b, c] = sum_k y[b, k] * W[c, k] + bias[c]        y = final-LayerNorm'd CLS rows (fp32), W / bias = the canonical
// fp32 tensors of the blob, read in place.
// The head is 0.002 % of a forward's FLOPs but the LAST rounding point in front of the logits: with 16-bit operands its
// two roundings (CLS rows, head weights) alone were 7 % + of the logit error variance (tools/parity_attribution.py).
// v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain (k-ordered), so this GEMM adds no operand rounding at all.
// One wave = 16 images x 64 classes: the W rows are the MFMA "A" operand, so a lane ends up with 4 consecutive classes of
// one image (one 16-byte store).  A lane's float4 load covers k = kb + 4 (lane >> 4) + {0..3}; element j of the A and of
// the B load go into MFMA j of the group, so both operands see the same k: the 4 x 4 (lane group, j) pairs cover
// kb .. kb + 15 exactly once.
__global__ void __launch_bounds__(256)
head_f32_kernel(const float* __restrict__ y, const float* __restrict__ w, const float* __restrict__ bias,
                float* __restrict__ out, int batch, int classes, int dim, int ncg, int64_t ldy, int64_t y_step, int64_t ldo,
                const float* __restrict__ add) {
    // blockIdx.y = the group of launch_head_f32_groups (0 for the head itself, where ldy = dim, ldo = classes and add is null)
    y += blockIdx.y * y_step;
    w += (int64_t)blockIdx.y * classes * dim;
    bias += blockIdx.y * classes;
    out += blockIdx.y * classes;
    if (add) add += blockIdx.y * classes;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int bb = gw / ncg, cg = gw - bb * ncg;
    if (bb * 16 >= batch) return;
    const int r = lane & 15, g = lane >> 4;
    int b = bb * 16 + r;
    b = b < batch ? b : batch - 1;
    const float* yp = y + (int64_t)b * ldy + 4 * g;
    const float* wp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = cg * 64 + i * 16 + r;
        c = c < classes ? c : classes - 1;
        wp[i] = w + (int64_t)c * dim + 4 * g;
    }
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < dim; kb += 16) {
        const f32x4 yv = *(const f32x4*)(yp + kb);
        f32x4 wv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wv[i] = *(const f32x4*)(wp[i] + kb);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[i][j], yv[j], acc[i], 0, 0, 0);
    }
    // D[row = class (lane >> 4) * 4 + reg][col = image lane & 15]
    const int bo = bb * 16 + r;
    if (bo < batch) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = cg * 64 + i * 16 + 4 * g;
            if (c < classes) {   // classes % 4 == 0: a quad is inside or outside as a whole
                const f32x4 bv = *(const f32x4*)(bias + c);
                f32x4 r4 = acc[i] + bv;
                if (add) r4 = r4 + *(const f32x4*)(add + (int64_t)bo * ldo + c);
                *(f32x4*)(out + (int64_t)bo * ldo + c) = r4;
            }
        }
    }
}

hipError_t launch_head_f32(const float* y, const float* w, const float* bias, float* out, int batch, int classes, int dim,
                           hipStream_t s) {
    if (batch <= 0 || classes <= 0 || (classes & 3) || dim <= 0 || (dim & 15)) return hipErrorInvalidValue;
    const int ncg = (classes + 63) / 64, nb = (batch + 15) / 16;
    const int waves = ncg * nb;
    hipLaunchKernelGGL(head_f32_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, y, w, bias, out, batch, classes, dim, ncg, (int64_t)dim,
                       (int64_t)0, (int64_t)classes, (const float*)nullptr);
    return hipGetLastError();
}

hipError_t launch_head_f32_groups(const float* y, int64_t ldy, int64_t y_step, const float* w, const float* bias, float* out, int64_t ldo,
                                  const float* add, int batch, int classes, int dim, int groups, hipStream_t s) {
    if (batch <= 0 || classes <= 0 || (classes & 3) || dim <= 0 || (dim & 15) || groups <= 0 || groups > 65535) return hipErrorInvalidValue;
    if (ldy < dim || (ldy & 3) || (y_step & 3) || ldo < (int64_t)classes * groups || (ldo & 3)) return hipErrorInvalidValue;
    const int ncg = (classes + 63) / 64, nb = (batch + 15) / 16;
    const int waves = ncg * nb;
    hipLaunchKernelGGL(head_f32_kernel, dim3((waves + 3) / 4, groups), dim3(256), 0, s, y, w, bias, out, batch, classes, dim, ncg, ldy, y_step,
                       ldo, add);
    return hipGetLastError();
}

// ---- the MAP head's activation on its fp32 hidden rows: the defining expressions, libm accuracy ------------------------------------
__global__ void __launch_bounds__(256) act_f32_kernel(float* __restrict__ x, int64_t n, int act) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    float r;
    if (act == 1) r = v / (1.0f + expf(-1.702f * v));
    else if (act == 2) r = 0.5f * v * (1.0f + tanhf(0.79788456080286536f * (v + 0.044715f * v * v * v)));
    else r = gelu_erf(v);
    x[i] = r;
}
hipError_t launch_act_f32(float* x, int64_t n, int act, hipStream_t s) {
    if (!x || n <= 0 || act < 0 || act > 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(act_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, act);
    return hipGetLastError();
}

}  // namespace vh
