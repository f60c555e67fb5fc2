// kernels_gather.hip — the patch gather for image TENSORS (gfx950): one element type (fp32 / fp16 / bf16 / u8) and one layout
// (NHWC / NCHW) per call; contract: vithip.h, "Image tensors".  Every kernel here writes the patch matrix [batch*np][kpad] of
// im2col_pad_kernel (kernels_misc.hip): k order (ky, kx, c), columns kp <= k < kpad zero on every call, one 16-byte store per
// 8-element chunk, nothing behind the matrix.  Element (b, y, x, c) enters as the fp32 value v -- the element itself, a 16-bit
// float widened exactly, or fmaf((float)p, scale[c], shift[c]) for a byte -- and v takes the pack4<T> of the fp32 kernels, so
// the matrix has the bits launch_im2col gives for the NHWC fp32 array of v.
//
//   gather_direct_kernel   one thread per output chunk, element (or one 16-byte) loads straight from the image: im2col_pad_kernel
//                          with a 16-bit source for NHWC, and the NCHW form for patches too large for the LDS strip
//   gather_nchw_kernel     NCHW: a workgroup takes a strip (b, py, npx patches): it copies the patch * ch plane-row segments of
//                          the strip into LDS as they lie in memory (contiguous along x: coalesced, 16-byte loads where the
//                          alignment allows), then every thread builds output chunks from LDS, which is where (x, c) transposes
//
// (NHWC, fp32) and (NHWC, u8) are launch_im2col and launch_im2col_u8, unchanged.
#include "vh_kernels.h"

namespace vh {

namespace {

// source element types: `raw` as stored, widen() = the exact fp32 value of one element (u8: the pixel, before the fma)
struct SrcF32 {
    using raw = float;
    static constexpr bool is_u8 = false;
    static __device__ __forceinline__ float widen(raw e) { return e; }
};
struct SrcF16 {
    using raw = _Float16;
    static constexpr bool is_u8 = false;
    static __device__ __forceinline__ float widen(raw e) { return (float)e; }   // v_cvt_f32_f16: exact, subnormals kept
};
struct SrcBF16 {
    using raw = uint16_t;
    static constexpr bool is_u8 = false;
    static __device__ __forceinline__ float widen(raw e) { return __builtin_bit_cast(float, (uint32_t)e << 16); }
};
struct SrcU8 {
    using raw = uint8_t;
    static constexpr bool is_u8 = true;
    static __device__ __forceinline__ float widen(raw e) { return (float)e; }
};

struct GatherNorm { float scale[kMaxChannels], shift[kMaxChannels]; };

// v of one element of channel c: u8 takes the one-rounding fma with the constants in LDS, floats pass through
template <typename E>
__device__ __forceinline__ float enter(typename E::raw e, int c, const float* s_scale, const float* s_shift) {
    if constexpr (E::is_u8) return __builtin_fmaf(E::widen(e), s_scale[c], s_shift[c]);
    else return E::widen(e);
}

template <typename T>
__device__ __forceinline__ void store_chunk(typename T::elem* dst, const float (&v)[8]) {
    const typename T::vec4 lo = pack4<T>(v[0], v[1], v[2], v[3]), hi = pack4<T>(v[4], v[5], v[6], v[7]);
    *(typename T::vec8*)dst = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- one thread per output chunk ---------------------------------------------------------------------------------------------
// Same thread mapping as im2col_pad_kernel.  NCHW = false: the 8 sources of a chunk walk (ky, r) through patch rows that are
// contiguous in the image; VEC (8 | patch * ch, 8 | image * ch, base aligned to 8 elements): they are contiguous and aligned, one
// load.  NCHW = true: element (ky, kx, c) lies at ((b * ch + c) * image + y) * image + x; element loads only.
template <typename T, typename E, bool NCHW, bool VEC>
__global__ void __launch_bounds__(256)
gather_direct_kernel(const typename E::raw* __restrict__ in, typename T::elem* __restrict__ out, int64_t n8, int image, int patch,
                     int ch, int kpad, const GatherNorm norm) {
    static_assert(!(NCHW && VEC), "the vector path is NHWC only");
    using raw = typename E::raw;
    __shared__ float s_scale[E::is_u8 ? kMaxChannels : 1], s_shift[E::is_u8 ? kMaxChannels : 1];
    if constexpr (E::is_u8) {
        if ((int)threadIdx.x < ch) {
            s_scale[threadIdx.x] = norm.scale[threadIdx.x];
            s_shift[threadIdx.x] = norm.shift[threadIdx.x];
        }
        __syncthreads();
    }
    const int pc = patch * ch;
    const int kp = patch * pc;
    const int cpr = kpad / 8;                // chunks per output row
    const int g = image / patch;
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n8; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t orow = f / cpr;        // (b * g + py) * g + px
        const int k0 = (int)(f - orow * cpr) * 8;
        const int64_t b = orow / (g * g);
        const int p = (int)(orow - b * g * g);
        const int py = p / g, px = p - py * g;
        int ky = k0 / pc, r = k0 - ky * pc;
        int c = r % ch;
        float v[8];
        if constexpr (NCHW) {
            const raw* src = in + (b * ch * image + (int64_t)py * patch) * image + (int64_t)px * patch;   // (b, c = 0, y0, x0)
            int kx = r / ch;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[i] = k0 + i < kp ? enter<E>(src[((int64_t)c * image + ky) * image + kx], c, s_scale, s_shift) : 0.f;
                if (++c == ch) { c = 0; if (++kx == patch) { kx = 0; ++ky; } }
            }
        } else {
            const raw* src = in + ((b * image + (int64_t)py * patch) * image + (int64_t)px * patch) * ch;
            if constexpr (VEC) {             // 8 | pc and 8 | kp: the chunk lies inside one patch row, or wholly in the padding
                raw e[8] = {};
                if (k0 < kp) __builtin_memcpy(e, __builtin_assume_aligned(src + ((int64_t)ky * image) * ch + r, 8 * sizeof(raw)), 8 * sizeof(raw));
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] = k0 < kp ? enter<E>(e[i], c, s_scale, s_shift) : 0.f;
                    if (++c == ch) c = 0;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] = k0 + i < kp ? enter<E>(src[((int64_t)ky * image) * ch + r], c, s_scale, s_shift) : 0.f;
                    if (++r == pc) { r = 0; ++ky; }
                    if (++c == ch) c = 0;
                }
            }
        }
        store_chunk<T>(out + f * 8, v);
    }
}

// ---- NCHW through LDS ----------------------------------------------------------------------------------------------------------
// Strip = (b, py, px0 .. px0 + npx): grid = batch * g * spr blocks, spr = strips per patch row.  LDS image: patch * ch rows in
// (ky, c) order, each the W = npx * patch source elements of plane row (b, c, py * patch + ky) from x = px0 * patch on, `pitch`
// BYTES apart; pitch = 16 mod 32, so a row starts 16-byte aligned and consecutive rows start 4 banks (mod 8) apart.
//   copy in   consecutive lanes take consecutive 16-byte vectors (VEC) or elements of a row: global reads are contiguous along
//             x, and a wave's LDS writes cover consecutive banks
//   build     thread <-> chunk (pxl, k0) as in the direct kernel; element (ky, kx, c) is LDS row ky * ch + c, column
//             pxl * patch + kx.  A wave's lanes step 8 k = 8 / ch pixels, so at ch = 3 the lanes that share a row read columns
//             8 apart, and the padded pitch spreads the 16 - 18 rows a 32-lane group touches over 8 bank offsets: 2 LDS cycles
//             per read where the natural pitch takes 3 - 12 (tools/gather_lds_banks.py; DESIGN.md 4.18 has the counts)
// VEC needs: 16-byte aligned base, 16 | image * sizeof(raw), 16 | patch * sizeof(raw) (every row segment then starts and ends on
// a 16-byte boundary); element loads otherwise.
template <typename T, typename E, bool VEC>
__global__ void __launch_bounds__(256)
gather_nchw_kernel(const typename E::raw* __restrict__ in, typename T::elem* __restrict__ out, int image, int patch, int ch,
                   int kpad, int npx, int spr, int pitch, const GatherNorm norm) {
    using raw = typename E::raw;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_img[];
    __shared__ float s_scale[E::is_u8 ? kMaxChannels : 1], s_shift[E::is_u8 ? kMaxChannels : 1];
    if constexpr (E::is_u8) {
        if ((int)threadIdx.x < ch) {
            s_scale[threadIdx.x] = norm.scale[threadIdx.x];
            s_shift[threadIdx.x] = norm.shift[threadIdx.x];
        }
    }
    const int g = image / patch;
    const int pc = patch * ch;               // LDS rows of a strip; elements per (ky) of a patch
    const int kp = patch * pc;
    const int cpr = kpad / 8;
    const int strip = (int)(blockIdx.x % (unsigned)spr);
    const int64_t bp = blockIdx.x / (unsigned)spr;       // b * g + py
    const int64_t b = bp / g;
    const int py = (int)(bp - b * g);
    const int px0 = strip * npx;
    const int n = px0 + npx <= g ? npx : g - px0;         // patches of this strip
    const int W = n * patch;                              // source elements per LDS row
    const raw* src = in + (b * ch * image + (int64_t)py * patch) * image + (int64_t)px0 * patch;   // (b, c = 0, y0, x0)
    if constexpr (VEC) {
        const int vpr = W * (int)sizeof(raw) / 16;        // vectors per row
        for (int i = threadIdx.x; i < pc * vpr; i += 256) {
            const int row = i / vpr, j = i - row * vpr;
            const int ky = row / ch, c = row - ky * ch;
            *(u32x4*)(s_img + row * pitch + 16 * j) = *((const u32x4*)(src + ((int64_t)c * image + ky) * image) + j);
        }
    } else {
        for (int i = threadIdx.x; i < pc * W; i += 256) {
            const int row = i / W, x = i - row * W;
            const int ky = row / ch, c = row - ky * ch;
            *((raw*)(s_img + row * pitch) + x) = src[((int64_t)c * image + ky) * image + x];
        }
    }
    __syncthreads();
    typename T::elem* orow0 = out + (bp * g + px0) * (int64_t)kpad;
    for (int f = threadIdx.x; f < n * cpr; f += 256) {
        const int pxl = f / cpr;
        const int k0 = (f - pxl * cpr) * 8;
        int ky = k0 / pc, r = k0 - ky * pc;
        int kx = r / ch, c = r - kx * ch;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = k0 + i < kp ? enter<E>(*((const raw*)(s_img + (ky * ch + c) * pitch) + pxl * patch + kx), c, s_scale, s_shift) : 0.f;
            if (++c == ch) { c = 0; if (++kx == patch) { kx = 0; ++ky; } }
        }
        store_chunk<T>(orow0 + (int64_t)f * 8, v);
    }
}

constexpr int kStripLdsBudget = 32 * 1024;   // bytes of LDS image a strip aims for: five workgroups per CU
constexpr int kStripLdsMax = 64 * 1024;      // and what a one-patch strip may take before the direct kernel runs instead

// LDS row pitch in bytes of a strip of npx patches: a multiple of 16 that is 16 mod 32
inline int strip_pitch(int npx, int patch, int esz) {
    const int w = (npx * patch * esz + 15) / 16 * 16;
    return w % 32 ? w : w + 16;
}

template <typename T, typename E>
hipError_t gather_t(const void* in_v, int layout, int batch, int image, int patch, int ch, int kpad, const GatherNorm& norm,
                    void* out16, hipStream_t s) {
    using raw = typename E::raw;
    const raw* in = (const raw*)in_v;
    auto* out = (typename T::elem*)out16;
    const int g = image / patch, esz = (int)sizeof(raw);
    const int64_t n8 = (int64_t)batch * g * g * (kpad / 8);
    const unsigned dgrid = (unsigned)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384);
    auto direct = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(dgrid), dim3(256), 0, s, in, out, n8, image, patch, ch, kpad, norm); };
    if (layout == VH_LAYOUT_NHWC) {
        if constexpr (sizeof(raw) == 2) {    // fp32 and u8 never come here (launch_im2col_tensor)
            const bool vec = (patch * ch) % 8 == 0 && (image * ch) % 8 == 0 && ((uintptr_t)in & 15) == 0;
            if (vec) direct(gather_direct_kernel<T, E, false, true>);
            else direct(gather_direct_kernel<T, E, false, false>);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    const int64_t rows = (int64_t)patch * ch;
    if (rows * strip_pitch(1, patch, esz) > kStripLdsMax) {   // one patch does not fit: no strip
        direct(gather_direct_kernel<T, E, true, false>);
        return hipGetLastError();
    }
    int npx = g;
    while (npx > 1 && rows * strip_pitch(npx, patch, esz) > kStripLdsBudget) npx = (npx + 1) / 2;
    const int spr = (g + npx - 1) / npx;
    const int pitch = strip_pitch(npx, patch, esz);
    const int64_t blocks = (int64_t)batch * g * spr;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const size_t lds = (size_t)rows * pitch;
    const bool vec = ((uintptr_t)in & 15) == 0 && (image * esz) % 16 == 0 && (patch * esz) % 16 == 0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, s, in, out, image, patch, ch, kpad, npx, spr, pitch, norm);
    };
    if (vec) go(gather_nchw_kernel<T, E, true>);
    else go(gather_nchw_kernel<T, E, false>);
    return hipGetLastError();
}

template <typename T>
hipError_t gather_e(const void* in, int elem, int layout, int batch, int image, int patch, int ch, int kpad, const GatherNorm& norm,
                    void* out16, hipStream_t s) {
    switch (elem) {
        case VH_ELEM_F32: return gather_t<T, SrcF32>(in, layout, batch, image, patch, ch, kpad, norm, out16, s);
        case VH_ELEM_F16: return gather_t<T, SrcF16>(in, layout, batch, image, patch, ch, kpad, norm, out16, s);
        case VH_ELEM_BF16: return gather_t<T, SrcBF16>(in, layout, batch, image, patch, ch, kpad, norm, out16, s);
        case VH_ELEM_U8: return gather_t<T, SrcU8>(in, layout, batch, image, patch, ch, kpad, norm, out16, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_im2col_tensor(const void* in, int elem, int layout, int batch, int image, int patch, int channels, int kpad,
                                const float* scale, const float* shift, void* out16, int dtype, hipStream_t s) {
    if (elem < VH_ELEM_F32 || elem > VH_ELEM_U8 || (layout != VH_LAYOUT_NHWC && layout != VH_LAYOUT_NCHW)) return hipErrorInvalidValue;
    if (!in || !out16 || batch < 1 || image < 1 || patch < 1 || patch > 256 || image % patch || channels < 1 || channels > kMaxChannels)
        return hipErrorInvalidValue;
    const int kp = patch * patch * channels;
    if (kpad < kp || kpad % 8 || (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16)) return hipErrorInvalidValue;
    if (elem == VH_ELEM_U8 && (!scale || !shift)) return hipErrorInvalidValue;
    // the two pairs the library already had keep their kernels
    if (layout == VH_LAYOUT_NHWC && elem == VH_ELEM_F32) return launch_im2col((const float*)in, batch, image, patch, channels, kpad, out16, dtype, s);
    if (layout == VH_LAYOUT_NHWC && elem == VH_ELEM_U8)
        return launch_im2col_u8((const uint8_t*)in, batch, image, patch, channels, kpad, scale, shift, out16, dtype, s);
    GatherNorm norm;
    for (int c = 0; c < kMaxChannels; ++c) {
        norm.scale[c] = elem == VH_ELEM_U8 && c < channels ? scale[c] : 0.f;
        norm.shift[c] = elem == VH_ELEM_U8 && c < channels ? shift[c] : 0.f;
    }
    return dtype == VH_DTYPE_BF16 ? gather_e<BF16>(in, elem, layout, batch, image, patch, channels, kpad, norm, out16, s)
                                  : gather_e<FP16>(in, elem, layout, batch, image, patch, channels, kpad, norm, out16, s);
}

}  // namespace vh
