// kernels_attn_bias.hip — attention with an additive per-head bias, softmax(q k^T / sqrt(hd) + B[h]) v: BEiT / data2vec-vision
// relative position bias, timm's vit_relpos_*, any fixed additive mask (gfx950).
//
// The kernel is attn_hd_kernel.h's skeleton with BIAS on (the design is written there): same row-major q|k|v and output, same head
// dims, same masks, rescale, sums and stores as launch_attention_hd.  What this file adds:
//   * the fragment image of B (bias_image_kernel): fp32 bias * log2(e) -- the scores live in the exp2 domain --, rounded once,
//     queries and keys zero-padded to multiples of 32, in the order
//         [head][query block qb][key tile kt][piece g = 0..3][lane = 32 hl + l31][j = 0..3]
//             = B[head][32 qb + l31][32 kt + 8 g + 4 hl + j] * log2(e)
//     -- element r = 4 g + j of lane (l31, hl)'s 32x32 MFMA accumulator.  A (head, query block, key tile) is 4 KiB contiguous
//     and each of its four 1 KiB pieces is lane-linear: one LDS-DMA instruction reads 1 KiB of consecutive bytes and the lane
//     reads its four values back with one ds_read_b128 at lane * 16.  Padded keys are masked by the tail tile, padded queries
//     are never stored.
//   * the launcher: work item = (head, query slab of 4 waves, image) with the IMAGES of a (head, slab) as neighbours in the grid:
//     they read the same bias tiles, which then meet in L2 whatever the image's size is (71 MB per layer at 1025 tokens and 16
//     heads).  VH_ATTN_BIAS_ORDER=0 (read at each launch; measurement only) keeps the unbiased kernel's (image, head, slab) order.
// Bias entries are finite (vithip.h): a large negative entry masks its key through the rescale path like any low score.
#include <cstdlib>

#include "attn_hd_kernel.h"

namespace vh {
namespace {

template <int NB16> using BiasShape = HdShape<NB16, true>;

// one thread per (head, qb, kt, g, lane): four consecutive keys of one query
__global__ void __launch_bounds__(256)
bias_image_kernel(const float* __restrict__ bias, int tokens, int nb, int64_t nquads, f32x4* __restrict__ image) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nquads) return;
    const int lane = (int)(i & 63), g = (int)((i >> 6) & 3);
    const int64_t tile = i >> 8;
    const int kt = (int)(tile % nb), qb = (int)((tile / nb) % nb);
    const int64_t h = tile / ((int64_t)nb * nb);
    const int q = 32 * qb + (lane & 31), k0 = 32 * kt + 8 * g + 4 * (lane >> 5);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q < tokens) {
        const float* row = bias + (h * tokens + q) * (int64_t)tokens;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k0 + j < tokens) v[j] = row[k0 + j] * 1.4426950408889634f;
    }
    image[i] = v;
}

template <int NB16, typename T>
hipError_t launch_bias_t(const void* qkv, int batch, int tokens, int heads, const float* image, void* out, hipStream_t s) {
    constexpr int maxw = BiasShape<NB16>::kMaxWaves;
    const int nqb = (tokens + 31) / 32;
    const int slabs = (nqb + maxw - 1) / maxw;
    const int nw = (nqb + slabs - 1) / slabs;
    const int64_t nitems = (int64_t)batch * heads * slabs;
    if (nitems > INT_MAX) return hipErrorInvalidValue;
    const char* e = getenv("VH_ATTN_BIAS_ORDER");
    const int inner = (e && e[0] == '0') ? 0 : batch;
    hipLaunchKernelGGL((attention_hd_kernel<NB16, T, T, const float*, int>), dim3((unsigned)nitems), dim3(nw * 64), 0, s,
                       (const typename T::elem*)qkv, (typename T::elem*)out, tokens, heads, slabs, nqb, image, inner);
    return hipGetLastError();
}

template <int NB16>
hipError_t launch_bias_dt(const void* qkv, int batch, int tokens, int heads, const float* image, void* out, int dtype, hipStream_t s) {
    if (dtype == VH_DTYPE_BF16) return launch_bias_t<NB16, BF16>(qkv, batch, tokens, heads, image, out, s);
    if (dtype == VH_DTYPE_FP16) return launch_bias_t<NB16, FP16>(qkv, batch, tokens, heads, image, out, s);
    return hipErrorInvalidValue;
}

}  // namespace

size_t attention_bias_image_bytes(int heads, int tokens) {
    if (heads <= 0 || heads > kAttnHdMaxWidth / 32 || tokens <= 0 || tokens > kAttnStreamMaxTokens) return 0;
    const size_t nb = (size_t)(tokens + 31) / 32;
    return (size_t)heads * nb * nb * kBiasTile;
}

const char* attention_bias_check(int batch, int tokens, int heads, int head_dim, int dtype) {
    if (tokens < 1 || tokens > kAttnStreamMaxTokens) return "tokens outside 1..4097";
    if (!attention_hd_supported(head_dim)) return "head_dim must be 32, 48, ..., 128";
    if (heads <= 0 || heads > kAttnHdMaxWidth / head_dim) return "heads * head_dim outside 1..2048";
    if (batch <= 0) return "batch must be positive";
    if (dtype == VH_DTYPE_FP8) return "VH_DTYPE_FP8 is not supported (bf16 and fp16 only)";
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return "dtype must be VH_DTYPE_BF16 or VH_DTYPE_FP16";
    return nullptr;
}

hipError_t launch_attention_bias_image(const float* bias, int heads, int tokens, float* image, hipStream_t s) {
    const size_t bytes = attention_bias_image_bytes(heads, tokens);
    if (!bias || !image || !bytes) return hipErrorInvalidValue;
    const int64_t nquads = (int64_t)(bytes / 16);
    const int64_t blocks = (nquads + 255) / 256;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bias_image_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bias, tokens, (tokens + 31) / 32, nquads, (f32x4*)image);
    return hipGetLastError();
}

hipError_t launch_attention_bias(const void* qkv16, int batch, int tokens, int heads, int head_dim, const float* image, void* out16,
                                 int dtype, hipStream_t s) {
    if (!qkv16 || !out16 || !image || attention_bias_check(batch, tokens, heads, head_dim, dtype)) return hipErrorInvalidValue;
    switch (head_dim / 16) {
        case 2: return launch_bias_dt<2>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        case 3: return launch_bias_dt<3>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        case 4: return launch_bias_dt<4>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        case 5: return launch_bias_dt<5>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        case 6: return launch_bias_dt<6>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        case 7: return launch_bias_dt<7>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        case 8: return launch_bias_dt<8>(qkv16, batch, tokens, heads, image, out16, dtype, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vh
