// kernels_attn_stream.hip — K/V-streaming multi-head attention for any token count 1..kAttnStreamMaxTokens (gfx950).
//
// Same operation and layouts as kernels_attn.hip (row-major q|k|v [batch*T][3*H*64] 16-bit with q pre-scaled by
// VH_ATTN_Q_SCALE, row-major output [batch*T][H*64]), without the resident forms' bound: those keep a whole head's K and V
// in LDS (ceil(T/32) * 8 KiB <= 160 KiB, T <= 640).  Here K and V pass through a fixed LDS ring of kSlots 32-key tiles
// (kSlots * 8 KiB = 24 KiB per workgroup, whatever T is), so two workgroups share a CU at every token count.
//
// Design (CDNA4), the resident ring kernel's idioms on a streamed image:
//   * work item = (image, head, query slab of nw*32 rows), one workgroup per item (nw <= kMaxWaves waves), blockIdx.x =
//     (image * heads + head) * slabs + slab: the slabs of a head are neighbours in the grid, so their K/V reads meet in L2.
//     No work-queue counter, no allocation: safe in a captured graph and when a batch is split across streams.
//   * key tile t lives in slot t % kSlots.  Its 8 pieces (8 rows x 128 B of K and of V) are moved by LDS-DMA
//     (asm_lds_dma16: hipcc does not see the transfer, so it never drains vmcnt in front of ds_read_b64_tr_b16) by waves
//     0..3, or by fewer waves several pieces each when nw < 4.  K is XOR-swizzled for ds_read_b128 row reads, V for the
//     transposing reads; both swizzles go on the lane's global source address (the DMA destination is lane-linear).
//   * per tile t: wait until this wave's pieces of tile t have landed (a counted vmcnt that leaves tile t+1 in flight),
//     barrier (every wave's pieces visible; every wave is done with tile t-1), refill tile t-1's slot with tile t+2, compute.
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (a query's scores in one lane pair), row max / sum finished with
//     v_permlane32_swap, exp2-domain online softmax with the deferred rescale (the shift moves only when a tile's scores
//     exceed it by 2^kTau; O and l are rescaled once, no probabilities are pending), the converted accumulator is the B
//     operand of O^T = V^T P^T, V^T from ds_read_b64_tr_b16, widened output stores.
//   * keys >= T in the last tile are masked (their rows replicate row T-1: finite data under zero probabilities); query
//     rows >= T are computed from the clamped row T-1 and not stored.  Image, head and plane bases are 64-bit.
#include <climits>
#include <type_traits>

#include "vh_kernels.h"

namespace vh {
namespace {

constexpr float kTau = 8.0f;     // as kernels_attn.hip
constexpr int kSlots = 3;        // ring depth in 32-key tiles
constexpr int kMaxWaves = 8;     // waves per workgroup: two workgroups of 8 fill a CU at 128 VGPRs

// lanes l and l^32 hold the two halves of a query's row (kernels_attn.hip swap_halves: one asm statement, the two
// results in different registers, s_nop for the VALU -> v_permlane hazard)
__device__ __forceinline__ void stream_swap_halves(float v, float& lo_everywhere, float& hi_everywhere) {
    float a = v, b;
    asm volatile("v_mov_b32 %1, %0\n\ts_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "=&v"(b));
    lo_everywhere = a;
    hi_everywhere = b;
}
__device__ __forceinline__ float stream_half_max(float v) {
    float a, b;
    stream_swap_halves(v, a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float stream_half_sum(float v) {
    float a, b;
    stream_swap_halves(v, a, b);
    return a + b;
}
// s_waitcnt vmcnt(n) for a wave-uniform n in 0..8 (a wave moves at most 8 pieces per tile)
__device__ __forceinline__ void stream_wait_vm(int n) {
#define VH_W(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (n) {
        VH_W(1) VH_W(2) VH_W(3) VH_W(4) VH_W(5) VH_W(6) VH_W(7) VH_W(8)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef VH_W
}
__device__ __forceinline__ void stream_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's LDS reads of the slot about to be refilled are done
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

template <typename T, typename TO>
__global__ void __launch_bounds__(kMaxWaves * 64, 4)
attention_stream_kernel(const typename T::elem* __restrict__ qkv, typename TO::elem* __restrict__ out,
                        int tokens, int heads, int slabs, int ntiles) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    using vec4 = typename T::vec4;
    __shared__ __attribute__((aligned(16))) char smem[2 * kSlots * 4096];   // K slots, then V slots
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    constexpr int kV = kSlots * 4096;   // offset of the V slots

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int l31 = lane & 31, hl = lane >> 5;
    const int D = heads * 64;
    const int64_t ld = 3 * (int64_t)D;

    const int item = blockIdx.x;
    const int bh = item / slabs, slab = item - bh * slabs;
    const int b = bh / heads, h = bh - b * heads;
    const elem* const base = qkv + (int64_t)b * tokens * ld + (int64_t)h * 64;   // q of (b, h); K at + D, V at + 2 D
    const int q0 = (slab * nw + wave) * 32;

    // ---- DMA of key tile t into slot t % kSlots: pieces g = wave, wave + nw, ... < 4 of K and of V --------------------
    // Byte offsets from `base` stay below 2^32: row < 4097, row pitch 3 D * 2 <= 12 KiB.
    const int npieces = wave < 4 ? (4 - wave + nw - 1) / nw : 0;   // per matrix and tile, wave-uniform
    auto issue_tile = [&](int t) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of hoisted into registers across the tile loop
        const int lr_ = ln >> 3, pc_ = ln & 7;
        const uint32_t slot = (uint32_t)(t % kSlots) * 4096u;
        for (int g = wave; g < 4; g += nw) {
            const int row = t * 32 + g * 8 + lr_;
            const int r = row < tokens ? row : tokens - 1;   // rows >= tokens replicate the last row
            const int ck = pc_ ^ ((row >> 1) & 7);
            const int cv = pc_ ^ (((row >> 1) & 1) << 2);
            const uint32_t ok = (uint32_t)(r * (int)ld + ck * 8) * 2u + (uint32_t)D * 2u;
            const uint32_t ov = (uint32_t)(r * (int)ld + cv * 8) * 2u + (uint32_t)D * 4u;
            asm_lds_dma16(base, ok, lds0 + slot + g * 1024);
            asm_lds_dma16(base, ov, lds0 + kV + slot + g * 1024);
        }
    };

    // this wave's Q fragments (rows >= tokens: the last row), then the first kSlots - 1 tiles
    vec8 qf[4];
    {
        int qrow = q0 + l31;
        qrow = qrow < tokens ? qrow : tokens - 1;
        const elem* qp = base + (int64_t)qrow * ld + 8 * hl;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const vec8*)(qp + 16 * ks);
    }
    for (int t = 0; t < kSlots - 1 && t < ntiles; ++t) issue_tile(t);

    // per-lane LDS offsets (kernels_attn.hip, ring form): K row reads, the other chunks are XORs (bits 4-5); V transposed
    // reads, the second 32-column block flips bit 6
    const int kswz = (l31 >> 1) & 7;
    const int g4 = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
    const int vrow0 = 4 * (g4 >> 1) + tq;
    const int vcolb = (16 * (g4 & 1) + 4 * tp) * 2;
    const int k0 = l31 * 128 + ((hl ^ kswz) << 4);
    const int vx = ((vrow0 >> 1) & 1) << 6;
    const int v0 = kV + vrow0 * 128 + (vcolb ^ vx);

    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float negm = 0.f;   // - (shift of this lane's query row), exp2 domain
    float lsum = 0.f;   // this lane's half of the row sum

    struct VFrag { vec8 f[2][2]; };   // V^T fragments of one tile: [k-step][column block]
    auto tile = [&](int kt, auto first_c, auto tail_c) {
        constexpr bool FIRST = decltype(first_c)::value, TAIL = decltype(tail_c)::value;
        // this wave's pieces of tile kt have landed (tile kt + 1 may stay in flight), then everyone's; tile kt - 1 is done
        stream_wait_vm(kt + 1 < ntiles ? 2 * npieces : 0);
        stream_barrier();
        if (kt + kSlots - 1 < ntiles) issue_tile(kt + kSlots - 1);   // into tile kt - 1's slot
        const int so = (kt % kSlots) * 4096;

        VFrag vfr;   // requested first: they arrive during the score MFMAs and the softmax
        {
            const char* p0 = smem + (v0 + so);
            const char* p1 = smem + ((v0 + so) ^ 64);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const vec4 a0 = T::tr_read(p0 + ks * 2048), c0 = T::tr_read(p0 + ks * 2048 + 1024);
                const vec4 a1 = T::tr_read(p1 + ks * 2048), c1 = T::tr_read(p1 + ks * 2048 + 1024);
#pragma unroll
                for (int j = 0; j < 4; ++j) { vfr.f[ks][0][j] = a0[j]; vfr.f[ks][0][4 + j] = c0[j]; vfr.f[ks][1][j] = a1[j]; vfr.f[ks][1][4 + j] = c1[j]; }
            }
        }
        // S^T tile: 32 keys x 32 queries, accumulators start at -shift (tile 0: at 0)
        f32x16 s;
        {
            const int ka = k0 + so;
            vec8 kf[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const vec8*)(smem + (ka ^ (ks << 5)));
            __builtin_amdgcn_sched_barrier(0);
            const float init = FIRST ? 0.f : negm;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = init;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = T::mfma32(kf[ks], qf[ks], s);
        }
        if constexpr (TAIL) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl >= tokens) s[r] = -INFINITY;
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = stream_half_max(mx);   // finite: every tile holds at least one key < tokens
        if constexpr (FIRST) {
            negm = -mx;             // the row's shift = its maximum over tile 0
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] -= mx;
        } else if (__builtin_amdgcn_ballot_w64(mx > kTau)) {   // rare: some row outgrew its shift by 2^kTau
            const float delta = fmaxf(mx, 0.f);
            const float alpha = __builtin_amdgcn_exp2f(-delta);
            negm -= delta;
            lsum *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; s[r] -= delta; }
        }
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        f32x2 psum = {0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[4 * g + j] = __builtin_amdgcn_exp2f(s[4 * g + j]);
            psum += f32x2{s[4 * g], s[4 * g + 1]};
            psum += f32x2{s[4 * g + 2], s[4 * g + 3]};
        }
        lsum += psum[0] + psum[1];
        // ---- O^T += V^T P^T ------------------------------------------------------------------------------------------
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            vec8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (elem)s[8 * ks + j];
            o0 = T::mfma32(vfr.f[ks][0], pf, o0);
            o1 = T::mfma32(vfr.f[ks][1], pf, o1);
        }
    };

    if (ntiles == 1) {
        tile(0, std::true_type{}, std::true_type{});
    } else {
        tile(0, std::true_type{}, std::false_type{});
        for (int kt = 1; kt + 1 < ntiles; ++kt) tile(kt, std::false_type{}, std::false_type{});
        tile(ntiles - 1, std::false_type{}, std::true_type{});
    }

    // ---- normalise and store: lane holds O[q][32*db + 8*rg + 4*hl + 0..3] (widened as in the ring form) -------------
    const float ltot = stream_half_sum(lsum);
    const float inv = __builtin_amdgcn_rcpf(ltot);
    const int q = q0 + l31;
    const int64_t mrow = (int64_t)b * tokens + (q < tokens ? q : tokens - 1);
    typename TO::elem* const op = out + mrow * D + (int64_t)h * 64 + 8 * hl;
    if constexpr (sizeof(typename TO::elem) == 2) {
        // a permlane32_swap per packed dword on a pair of 8-column groups: lanes 0-31 end with group rg, lanes 32-63 with
        // rg + 1 -- 4 x 16 bytes per lane
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const f32x16& o = db ? o1 : o0;
#pragma unroll
            for (int rg = 0; rg < 4; rg += 2) {
                const u32x2 ga = __builtin_bit_cast(u32x2, pack4<TO>(o[4 * rg] * inv, o[4 * rg + 1] * inv, o[4 * rg + 2] * inv, o[4 * rg + 3] * inv));
                const u32x2 gb = __builtin_bit_cast(u32x2, pack4<TO>(o[4 * rg + 4] * inv, o[4 * rg + 5] * inv, o[4 * rg + 6] * inv, o[4 * rg + 7] * inv));
                const auto sx = __builtin_amdgcn_permlane32_swap(ga[0], gb[0], false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(ga[1], gb[1], false, false);
                if (q < tokens) *(u32x4*)(op + (4 * db + rg) * 8) = u32x4{sx[0], sy[0], sx[1], sy[1]};
            }
        }
    } else {
        // e4m3: a lane's quad is one dword; the same exchange gives 4 x 8 bytes per lane
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const f32x16& o = db ? o1 : o0;
#pragma unroll
            for (int rg = 0; rg < 4; rg += 2) {
                const uint32_t ga = pack4<TO>(o[4 * rg] * inv, o[4 * rg + 1] * inv, o[4 * rg + 2] * inv, o[4 * rg + 3] * inv);
                const uint32_t gb = pack4<TO>(o[4 * rg + 4] * inv, o[4 * rg + 5] * inv, o[4 * rg + 6] * inv, o[4 * rg + 7] * inv);
                const auto sx = __builtin_amdgcn_permlane32_swap(ga, gb, false, false);
                if (q < tokens) *(u32x2*)(op + 32 * db + 8 * rg) = u32x2{sx[0], sx[1]};
            }
        }
    }
}

template <typename T, typename TO>
hipError_t launch_stream_t(const void* qkv, int batch, int tokens, int heads, void* out, hipStream_t s) {
    const int nqb = (tokens + 31) / 32;
    const int slabs = (nqb + kMaxWaves - 1) / kMaxWaves;
    const int nw = (nqb + slabs - 1) / slabs;
    const int64_t nitems = (int64_t)batch * heads * slabs;
    if (nitems > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL((attention_stream_kernel<T, TO>), dim3((unsigned)nitems), dim3(nw * 64), 0, s,
                       (const typename T::elem*)qkv, (typename TO::elem*)out, tokens, heads, slabs, nqb);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_attention_stream(const void* qkv16, int batch, int tokens, int heads, void* out16, int dtype, hipStream_t s) {
    if (!qkv16 || !out16 || batch <= 0 || tokens <= 0 || tokens > kAttnStreamMaxTokens || heads <= 0 || heads > 32)
        return hipErrorInvalidValue;
    if (dtype == VH_DTYPE_FP8) return launch_stream_t<BF16, E4M3>(qkv16, batch, tokens, heads, out16, s);   // bf16 in, e4m3 out
    if (dtype == VH_DTYPE_BF16) return launch_stream_t<BF16, BF16>(qkv16, batch, tokens, heads, out16, s);
    if (dtype == VH_DTYPE_FP16) return launch_stream_t<FP16, FP16>(qkv16, batch, tokens, heads, out16, s);
    return hipErrorInvalidValue;
}

}  // namespace vh
