// kernels_attn_maps.hip — attention maps (vithip.h "Attention maps"): the softmax rows of an image's first Q queries, and their read-out.
//
// The three attention kernels keep the probabilities in registers or LDS and store only P V.  This file computes the rows a caller
// asks for on their own, from the q|k|v the projection wrote: Q * tokens * head_dim MACs per (image, head) -- nothing beside the
// forward -- so no MFMA and no LDS; the cost is reading K once.
#include "vh_kernels.h"

namespace vh {

// ---- capture: probs[b][h][r][t] = softmax_t(q_r . k_t), r < Q ----------------------------------------------------------------
// One wave per (image, head), four per workgroup.  A key row is HD / 8 sixteen-byte chunks; LPR = the next power of two lanes share a
// row (lane = LPR * g + c reads chunk c of row (64 / LPR) * step + g; lanes c >= HD / 8 hold zeros), so head dims that are no power
// of two keep 16-byte loads and one wave instruction covers 64 / LPR whole rows.  U row groups per step = U independent loads in
// flight per lane: the walk is latency-bound (attention_cls_kernel).  The lane keeps chunk c of all Q query rows in registers as the
// 16-bit values they arrive in (4 registers per query), so K is read once whatever Q is.
//
// ARITHMETIC (vithip.h, for bits).  s[r][t]: eight fmaf over the lane's chunk in ascending k from 0.f, then the xor butterfly 1, 2, ..
// over the row's LPR lanes -- a function of HD alone.  The raw scores go to the output slot itself (no LDS bound on Q * tokens; the
// slot is L2-hot), the row maximum travels in registers.  l: lane i adds e[t] = exp2(s[t] - m) (exp2_full) for t = i, i + 64, ... in ascending
// order from 0.f, then the wave butterfly 32, 16, .. -- a function of tokens alone.  p = e / l, the IEEE division, recomputing e from
// the staged score (the instruction is deterministic), written in place.

// v_exp_f32 behind the compiler's denormal-range scaling (an argument below -126 runs as exp2(x + 64) * 2^-64: the add is exact, the
// scaling rounds once, into the denormal range): a probability below 2^-126 is its denormal, not a flushed zero
__device__ __forceinline__ float exp2_full(float x) { return __builtin_exp2f(x); }

template <typename T, int HD, int QMAX>
__global__ void __launch_bounds__(256)
attention_probs_kernel(const typename T::elem* __restrict__ qkv, float* probs, int batch, int tokens, int heads, int Q, int64_t ld,
                       int64_t koff, int64_t hm_rows) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    constexpr int C = HD / 8;                                   // 16-byte chunks of a row
    constexpr int LPR = C <= 4 ? 4 : C <= 8 ? 8 : 16;           // lanes per row
    constexpr int RPI = 64 / LPR;                               // rows per wave instruction
    constexpr int U = 4;                                        // row groups (key walk) / 64-key groups (row passes) per step
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wv;
    if (item >= batch * heads) return;
    const int b = item / heads, h = item - b * heads;
    // row-major [rows][3 D]: q of head h at column h * HD, k at + D;  head-major [3][heads][hm_rows][64]: q at (h * hm_rows + row) * 64
    const elem* const base = hm_rows ? qkv + ((int64_t)h * hm_rows + (int64_t)b * tokens) * 64 : qkv + (int64_t)b * tokens * ld + h * HD;
    const int g = lane / LPR, c = lane % LPR;
    const bool cv = c < C;
    const int cc = cv ? c : 0;
    vec8 zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (elem)0.f;
    vec8 q[QMAX];
    float mx[QMAX];
#pragma unroll
    for (int r = 0; r < QMAX; ++r) {
        const int rr = r < Q ? r : Q - 1;
        const vec8 v = *(const vec8*)(base + (int64_t)rr * ld + cc * 8);
        q[r] = cv ? v : zero;
        mx[r] = -INFINITY;
    }
    float* const out = probs + (int64_t)item * Q * tokens;
    for (int t0 = 0; t0 < tokens; t0 += RPI * U) {
        vec8 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + RPI * u + g;
            v[u] = *(const vec8*)(base + (int64_t)(t < tokens ? t : tokens - 1) * ld + koff + cc * 8);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + RPI * u + g;
            float kf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) kf[j] = (float)v[u][j];
#pragma unroll
            for (int r = 0; r < QMAX; ++r) {
                float sv = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) sv = fmaf((float)q[r][j], kf[j], sv);
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) sv += __shfl_xor(sv, o);
                if (t < tokens && r < Q) {
                    if (c == 0) out[(int64_t)r * tokens + t] = sv;
                    mx[r] = fmaxf(mx[r], sv);
                }
            }
        }
    }
    // the wave's own score stores are visible to its loads below (one CU, one wave: a workgroup-scope fence is a wait)
    __threadfence_block();
    // lane r keeps the maximum of row r: the row loop below has a runtime trip count and cannot index the register array
    float mrow = 0.f;
#pragma unroll
    for (int r = 0; r < QMAX; ++r) {
        const float m = wave_max(mx[r]);
        mrow = lane == r ? m : mrow;
    }
    for (int r = 0; r < Q; ++r) {
        const float m = __shfl(mrow, r);
        float* const row = out + (int64_t)r * tokens;
        float sum = 0.f;
        for (int t0 = 0; t0 < tokens; t0 += 64 * U) {
            float sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 64 * u + lane;
                sv[u] = row[t < tokens ? t : tokens - 1];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (t0 + 64 * u + lane < tokens) sum += exp2_full(sv[u] - m);
        }
        const float l = wave_sum(sum);
        for (int t0 = 0; t0 < tokens; t0 += 64 * U) {
            float sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 64 * u + lane;
                sv[u] = row[t < tokens ? t : tokens - 1];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 64 * u + lane;
                if (t < tokens) row[t] = exp2_full(sv[u] - m) / l;
            }
        }
    }
}

template <typename T, int HD>
static hipError_t launch_probs_q(const void* qkv, int64_t hm_rows, int batch, int tokens, int heads, int Q, float* probs, hipStream_t s) {
    const int64_t D = (int64_t)heads * HD;
    const int64_t ld = hm_rows ? 64 : 3 * D, koff = hm_rows ? hm_rows * D : D;
    const dim3 grid((unsigned)(((int64_t)batch * heads + 3) / 4));
    // the query rows are register arrays: three sizes (the class token; DINOv2's 1 + 4; up to 1 + 16)
    auto go = [&](auto k) {
        hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (const typename T::elem*)qkv, probs, batch, tokens, heads, Q, ld, koff, hm_rows);
        return hipGetLastError();
    };
    if (Q == 1) return go(attention_probs_kernel<T, HD, 1>);
    if (Q <= 5) return go(attention_probs_kernel<T, HD, 5>);
    return go(attention_probs_kernel<T, HD, kAttnMapsMaxQueries>);
}
template <typename T>
static hipError_t launch_probs_hd(const void* qkv, int64_t hm_rows, int batch, int tokens, int heads, int head_dim, int Q, float* probs,
                                  hipStream_t s) {
    switch (head_dim) {
        case 32: return launch_probs_q<T, 32>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
        case 48: return launch_probs_q<T, 48>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
        case 64: return launch_probs_q<T, 64>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
        case 80: return launch_probs_q<T, 80>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
        case 96: return launch_probs_q<T, 96>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
        case 112: return launch_probs_q<T, 112>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
        case 128: return launch_probs_q<T, 128>(qkv, hm_rows, batch, tokens, heads, Q, probs, s);
    }
    return hipErrorInvalidValue;
}

const char* attention_probs_check(int64_t in_hm_rows, int batch, int tokens, int heads, int head_dim, int Q, int dtype) {
    if (batch <= 0) return "batch must be positive";
    if (tokens < 1 || tokens > kAttnStreamMaxTokens) return "tokens outside 1..4097";
    if (!attention_hd_supported(head_dim)) return "head_dim must be 32, 48, ..., 128";
    if (heads <= 0 || heads > kAttnHdMaxWidth / head_dim) return "heads * head_dim outside 1..2048";
    if (Q < 1 || Q > kAttnMapsMaxQueries) return "queries outside 1..17";
    if (Q > tokens) return "more queries than tokens";
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return "dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (in_hm_rows < 0) return "in_hm_rows is negative";
    if (in_hm_rows && head_dim != 64) return "head-major q|k|v exists at head_dim 64 only";
    if (in_hm_rows && in_hm_rows < (int64_t)batch * tokens) return "in_hm_rows holds fewer than batch * tokens rows";
    if ((int64_t)batch * heads > 0x7fffffffll - 4) return "batch * heads is too large";
    return nullptr;
}
hipError_t launch_attention_probs(const void* qkv16, int64_t in_hm_rows, int batch, int tokens, int heads, int head_dim, int Q, int dtype,
                                  float* probs, hipStream_t s) {
    if (!qkv16 || !probs || attention_probs_check(in_hm_rows, batch, tokens, heads, head_dim, Q, dtype)) return hipErrorInvalidValue;
    return dtype == VH_DTYPE_BF16 ? launch_probs_hd<BF16>(qkv16, in_hm_rows, batch, tokens, heads, head_dim, Q, probs, s)
                                  : launch_probs_hd<FP16>(qkv16, in_hm_rows, batch, tokens, heads, head_dim, Q, probs, s);
}

// ---- read-out: a store slot [batch][heads][Q][tokens] fp32 -> the caller's buffers ------------------------------------------------
// One thread per (image, query, key column k0 + k) walks the heads in ascending order: probs_out[b][h][r][k] = the element (16-bit:
// its RNE), head_mean[b][r][k] = (((0 + p[0]) + p[1]) + ... + p[H - 1]) * (float)(1.0 / H) of the unrounded values.  Consecutive
// threads take consecutive columns.
template <typename TO>
__global__ void __launch_bounds__(256)
attention_readout_kernel(const float* __restrict__ store, int batch, int heads, int Q, int tokens, int k0, typename TO::elem* probs_out,
                         typename TO::elem* mean_out, float inv_heads) {
    using elem = typename TO::elem;
    const int K = tokens - k0;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)batch * Q * K) return;
    const int k = (int)(i % K);
    const int64_t br = i / K;
    const int r = (int)(br % Q);
    const int64_t b = br / Q;
    float acc = 0.f;
    for (int h = 0; h < heads; ++h) {
        const int64_t row = (b * heads + h) * Q + r;
        const float p = store[row * tokens + k0 + k];
        if (probs_out) probs_out[row * K + k] = (elem)p;
        acc += p;
    }
    if (mean_out) mean_out[i] = (elem)(acc * inv_heads);
}

const char* attention_readout_check(int batch, int heads, int Q, int tokens, int lead, int elem, int keys) {
    if (batch <= 0) return "batch must be positive";
    if (heads <= 0 || heads > kAttnHdMaxWidth / 32) return "heads outside 1..64";
    if (tokens < 1 || tokens > kAttnStreamMaxTokens) return "tokens outside 1..4097";
    if (Q < 1 || Q > kAttnMapsMaxQueries || Q > tokens) return "queries outside 1..min(17, tokens)";
    if (elem != VH_ELEM_F32 && elem != VH_ELEM_F16 && elem != VH_ELEM_BF16) return "elem is not VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16";
    if (keys != VH_ATTN_KEYS_ALL && keys != VH_ATTN_KEYS_PATCH) return "keys is not VH_ATTN_KEYS_ALL or VH_ATTN_KEYS_PATCH";
    if (lead < 0 || lead >= tokens) return "lead outside 0..tokens-1";
    if (((int64_t)batch * Q * tokens + 255) / 256 > 0x7fffffffll) return "batch * queries * tokens is too large";
    return nullptr;
}
hipError_t launch_attention_readout(const float* store, int batch, int heads, int Q, int tokens, int lead, int elem, int keys, void* probs_out,
                                    void* mean_out, hipStream_t s) {
    if (!store || (!probs_out && !mean_out) || attention_readout_check(batch, heads, Q, tokens, lead, elem, keys)) return hipErrorInvalidValue;
    const int k0 = keys == VH_ATTN_KEYS_PATCH ? lead : 0;
    const int64_t n = (int64_t)batch * Q * (tokens - k0);
    const dim3 grid((unsigned)((n + 255) / 256));
    const float inv = (float)(1.0 / heads);
    auto go = [&](auto t) {
        using TO = decltype(t);
        hipLaunchKernelGGL(attention_readout_kernel<TO>, grid, dim3(256), 0, s, store, batch, heads, Q, tokens, k0, (typename TO::elem*)probs_out,
                           (typename TO::elem*)mean_out, inv);
        return hipGetLastError();
    };
    if (elem == VH_ELEM_F32) return go(F32OUT{});
    return elem == VH_ELEM_F16 ? go(FP16{}) : go(BF16{});
}

}  // namespace vh
