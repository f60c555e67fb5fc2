// kernels_attn_hd.hip — the K/V-streaming multi-head attention kernel without a bias: the instantiations of attn_hd_kernel.h's
// skeleton for every head dim 32, 48, ..., 128 and their launcher (the biased ones: kernels_attn_bias.hip).
#include "attn_hd_kernel.h"

namespace vh {
namespace {

template <int NB16, typename T, typename TO>
hipError_t launch_hd_t(const void* qkv, int batch, int tokens, int heads, void* out, hipStream_t s) {
    constexpr int maxw = HdShape<NB16>::kMaxWaves;
    const int nqb = (tokens + 31) / 32;
    const int slabs = (nqb + maxw - 1) / maxw;
    const int nw = (nqb + slabs - 1) / slabs;
    const int64_t nitems = (int64_t)batch * heads * slabs;
    if (nitems > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL((attention_hd_kernel<NB16, T, TO>), dim3((unsigned)nitems), dim3(nw * 64), 0, s,
                       (const typename T::elem*)qkv, (typename TO::elem*)out, tokens, heads, slabs, nqb);
    return hipGetLastError();
}

template <int NB16>
hipError_t launch_hd_dt(const void* qkv, int batch, int tokens, int heads, void* out, int dtype, hipStream_t s) {
    if (dtype == VH_DTYPE_FP8) return launch_hd_t<NB16, BF16, E4M3>(qkv, batch, tokens, heads, out, s);   // bf16 in, e4m3 out
    if (dtype == VH_DTYPE_BF16) return launch_hd_t<NB16, BF16, BF16>(qkv, batch, tokens, heads, out, s);
    if (dtype == VH_DTYPE_FP16) return launch_hd_t<NB16, FP16, FP16>(qkv, batch, tokens, heads, out, s);
    return hipErrorInvalidValue;
}

}  // namespace

bool attention_hd_supported(int head_dim) { return head_dim >= 32 && head_dim <= 128 && head_dim % 16 == 0; }

hipError_t launch_attention_hd(const void* qkv16, int batch, int tokens, int heads, int head_dim, void* out16, int dtype,
                               hipStream_t s) {
    if (!qkv16 || !out16 || batch <= 0 || tokens <= 0 || tokens > kAttnStreamMaxTokens || heads <= 0 ||
        !attention_hd_supported(head_dim) || heads * head_dim > kAttnHdMaxWidth)
        return hipErrorInvalidValue;
    switch (head_dim / 16) {
        case 2: return launch_hd_dt<2>(qkv16, batch, tokens, heads, out16, dtype, s);
        case 3: return launch_hd_dt<3>(qkv16, batch, tokens, heads, out16, dtype, s);
        case 4: return launch_hd_dt<4>(qkv16, batch, tokens, heads, out16, dtype, s);
        case 5: return launch_hd_dt<5>(qkv16, batch, tokens, heads, out16, dtype, s);
        case 6: return launch_hd_dt<6>(qkv16, batch, tokens, heads, out16, dtype, s);
        case 7: return launch_hd_dt<7>(qkv16, batch, tokens, heads, out16, dtype, s);
        case 8: return launch_hd_dt<8>(qkv16, batch, tokens, heads, out16, dtype, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vh
