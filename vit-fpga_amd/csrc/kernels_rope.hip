// kernels_rope.hip — rotary position embedding (vithip.h VH_FLAG_ROPE): the in-place rotation of q and k of the patch rows.
//
// One pass over what the q|k|v projection left in memory, in front of the attention kernels, which stay as they are.  Memory-bound: q
// and k are read and written once (v, the lead rows and the tile-padding rows are not touched); the tables [NP][hd / 2] fp32 stay
// cache-resident (50 KB at ViT-B/16).
//
// A lane owns chunk c (8 elements, 16 B) of the low half and chunk c of the high half of ONE (patch row, q or k, head): two 16-byte
// loads, four 32-byte table reads, two 16-byte stores.  Consecutive lanes take consecutive chunks, then
//   row-major  [rows][3 D]:               consecutive heads, then q | k, then patch rows -- the q and k of a row are one 4 D-byte run;
//   head-major [3][heads][hm_rows][64]:   consecutive patch rows of one (q or k, head) plane -- a row's 128 B line is filled by the
//                                         low-half and the high-half access of four neighbouring lanes.
// ARITHMETIC (vithip.h, for bits): lo' = fmaf(lo, c, -(hi * s)), hi' = fmaf(hi, c, lo * s) in fp32, one RNE to the element type.
#include "vh_kernels.h"

namespace vh {

// C = hd / 16: 16-byte chunks per half row.  HM: head-major addressing (C == 4).
template <typename T, int C, bool HM>
__global__ void __launch_bounds__(256)
rope_kernel(typename T::elem* qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t, uint32_t items, uint32_t prows, int np,
            int tokens, int lead, int heads, int64_t hm_rows) {
    using vec8 = typename T::vec8;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    constexpr int HALF = C * 8, HD = 2 * HALF;
    const uint32_t c = i % C, t1 = i / C;
    uint32_t prow, head, which;
    if constexpr (HM) {
        prow = t1 % prows;
        const uint32_t t2 = t1 / prows;
        head = t2 % (uint32_t)heads;
        which = t2 / (uint32_t)heads;
    } else {
        head = t1 % (uint32_t)heads;
        const uint32_t t2 = t1 / (uint32_t)heads;
        which = t2 & 1u;
        prow = t2 >> 1;
    }
    const uint32_t b = prow / (uint32_t)np, p = prow - b * (uint32_t)np;
    const int64_t row = (int64_t)b * tokens + lead + p;
    const int64_t D = (int64_t)heads * HD;
    typename T::elem* const lo_p = HM ? qkv + (((int64_t)which * heads + head) * hm_rows + row) * 64 + c * 8
                                      : qkv + row * 3 * D + which * D + (int64_t)head * HD + c * 8;
    typename T::elem* const hi_p = lo_p + HALF;
    const vec8 lo = *(const vec8*)lo_p, hi = *(const vec8*)hi_p;
    const f32x4* const cp = (const f32x4*)(cos_t + (size_t)p * HALF + c * 8);
    const f32x4* const sp = (const f32x4*)(sin_t + (size_t)p * HALF + c * 8);
    const f32x4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
    vec8 olo, ohi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float cj = j < 4 ? c0[j & 3] : c1[j & 3], sj = j < 4 ? s0[j & 3] : s1[j & 3];
        const float a = (float)lo[j], h = (float)hi[j];
        olo[j] = (typename T::elem)fmaf(a, cj, -(h * sj));
        ohi[j] = (typename T::elem)fmaf(h, cj, a * sj);
    }
    *(vec8*)lo_p = olo;
    *(vec8*)hi_p = ohi;
}

const char* rope_check(const void* qkv16, int dtype, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows,
                       const float* cos_t, const float* sin_t) {
    if (!qkv16 || !cos_t || !sin_t) return "null pointer";
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return "dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (batch <= 0) return "batch must be positive";
    if (tokens < 1 || tokens > kAttnStreamMaxTokens) return "tokens outside 1..4097";
    if (!attention_hd_supported(head_dim)) return "head_dim must be 32, 48, ..., 128";
    if (heads <= 0 || heads > kAttnHdMaxWidth / head_dim) return "heads * head_dim outside 1..2048";
    if (lead < 0 || lead >= tokens) return "lead outside 0..tokens-1";
    if (hm_rows < 0) return "hm_rows is negative";
    if (hm_rows && head_dim != 64) return "head-major q|k|v exists at head_dim 64 only";
    if (hm_rows && hm_rows < (int64_t)batch * tokens) return "hm_rows holds fewer than batch * tokens rows";
    if (((uintptr_t)qkv16 | (uintptr_t)cos_t | (uintptr_t)sin_t) & 15) return "qkv16, cos and sin must be 16-byte aligned";
    // one lane per 16-byte chunk pair: 2 (q, k) * heads * head_dim / 16 of them per patch row, a 32-bit count
    if ((int64_t)batch * (tokens - lead) * (heads * head_dim / 8) > 0x7fffff00ll) return "batch * patch rows * heads * head_dim / 8 is too large";
    return nullptr;
}

template <typename T, int C>
static hipError_t launch_rope_c(void* qkv16, int batch, int tokens, int heads, int lead, int64_t hm_rows, const float* cos_t, const float* sin_t,
                                hipStream_t s) {
    const int np = tokens - lead;
    const uint32_t prows = (uint32_t)batch * (uint32_t)np, items = prows * 2u * (uint32_t)heads * C;
    const dim3 grid((items + 255u) / 256u);
    auto go = [&](auto k) {
        hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (typename T::elem*)qkv16, cos_t, sin_t, items, prows, np, tokens, lead, heads, hm_rows);
        return hipGetLastError();
    };
    if constexpr (C == 4) { if (hm_rows) return go(rope_kernel<T, C, true>); }
    return go(rope_kernel<T, C, false>);
}
template <typename T>
static hipError_t launch_rope_t(void* qkv16, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows, const float* cos_t,
                                const float* sin_t, hipStream_t s) {
    switch (head_dim) {
        case 32: return launch_rope_c<T, 2>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
        case 48: return launch_rope_c<T, 3>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
        case 64: return launch_rope_c<T, 4>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
        case 80: return launch_rope_c<T, 5>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
        case 96: return launch_rope_c<T, 6>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
        case 112: return launch_rope_c<T, 7>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
        case 128: return launch_rope_c<T, 8>(qkv16, batch, tokens, heads, lead, hm_rows, cos_t, sin_t, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_rope(void* qkv16, int dtype, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows, const float* cos_t,
                       const float* sin_t, hipStream_t s) {
    if (rope_check(qkv16, dtype, batch, tokens, heads, head_dim, lead, hm_rows, cos_t, sin_t)) return hipErrorInvalidValue;
    return dtype == VH_DTYPE_BF16 ? launch_rope_t<BF16>(qkv16, batch, tokens, heads, head_dim, lead, hm_rows, cos_t, sin_t, s)
                                  : launch_rope_t<FP16>(qkv16, batch, tokens, heads, head_dim, lead, hm_rows, cos_t, sin_t, s);
}

}  // namespace vh
