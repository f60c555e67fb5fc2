// kernels_attn_hd.hip — K/V-streaming multi-head attention for head dims 32, 48, ..., 128 (gfx950).
//
// The operation of kernels_attn_stream.hip at any head dim hd = 16 * NB16 (NB16 = 2..8): row-major q|k|v
// [batch*T][3*H*hd] 16-bit with q pre-scaled by hd^-1/2 * log2(e), row-major output [batch*T][H*hd], any token count
// 1..kAttnStreamMaxTokens.  The forward sends every model whose head dim is not 64 here (head dim 64 keeps its kernels).
//
// Differences from the 64-wide streaming kernel (same ring, DMA, wait / barrier and online-softmax structure):
//   * S^T = K Q^T contracts over NB16 k-steps of v_mfma_f32_32x32x16 (Q fragments qf[NB16]); O^T = V^T P^T keeps
//     NDB = ceil(hd / 32) 32x32 accumulators.  For hd = 48, 80, 112 the last block covers 16 real V columns: its other 16
//     A rows re-read the real ones (same LDS addresses, a broadcast) and their output rows are not stored.  An MFMA output
//     row depends only on its own A row, so they cannot touch the stored rows.
//   * K/V tile image in LDS (one function for K and V, NB16 KiB per matrix and tile): the 32 x hd tile is cut into
//     8-row x 16-column subtiles of 256 B -- exactly one bank row -- in the order [row group rg = row / 8][column pair
//     p = chunk / 2]; inside a subtile, 16-byte chunk (row, chunk) sits at
//         32 * ((row & 7) ^ 4 * (p & 1)) + 16 * ((chunk & 1) ^ (rg & 1)).
//     ds_read_b128 of the K operand (16 lanes, one chunk, 16 rows that are distinct mod 16) lands on 16 distinct slots;
//     ds_read_b64_tr_b16 of the V operand (a 32-lane half: 4 rows x 4 chunks x 2 halves in two neighbouring subtiles)
//     lands on 32 distinct 8-byte pieces, the XOR by 4 * (p & 1) putting the odd subtile's rows on the other half of the
//     bank row.  Conflict-free at every hd, with no assumption on the row pitch (160 B at hd 80).
//   * LDS-DMA stays lane-linear: one 1 KiB instruction fills four consecutive subtiles, the permutation goes on the
//     lane's global source address.  With NB16 >= 4 a DMA reads 8 rows x 128 contiguous bytes.
//   * LDS per workgroup: kSlots * 2 * NB16 KiB (48 KiB at hd 128): at least three workgroups per CU at every hd.
// Query rows >= T and keys >= T as in the 64-wide kernel; image, head and plane bases are 64-bit.
#include <climits>
#include <type_traits>

#include "vh_kernels.h"

namespace vh {
namespace {

constexpr float kTau = 8.0f;     // as kernels_attn.hip
constexpr int kSlots = 3;        // ring depth in 32-key tiles

// waves per workgroup and the register budget: up to hd 64, 8 waves at <= 128 VGPRs (two workgroups per CU, as the
// 64-wide kernel); beyond, the accumulators and fragments need more (hd 80 spills at 128), so 4 waves at <= 256 VGPRs
// (at least two workgroups per CU)
template <int NB16> struct HdShape {
    static constexpr int kMaxWaves = NB16 <= 4 ? 8 : 4;
    static constexpr int kWavesPerEU = NB16 <= 4 ? 4 : 2;
};

// lanes l and l^32 hold the two halves of a query's row.  The builtin, not an asm statement as in the 64-wide kernel: with
// a half last block the rows 16..31 of its accumulator are dead after the last MFMA, the register allocator reuses them, and
// hipcc pads no wait states inside an asm string -- an asm write there races the MFMA's late result writes (WAW).  Same
// values, same sums: lo + hi in every lane.
__device__ __forceinline__ void hd_swap_halves(float v, float& lo_everywhere, float& hi_everywhere) {
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, v), __builtin_bit_cast(uint32_t, v), false, false);
    lo_everywhere = __builtin_bit_cast(float, (uint32_t)r[0]);
    hi_everywhere = __builtin_bit_cast(float, (uint32_t)r[1]);
}
__device__ __forceinline__ float hd_half_max(float v) {
    float a, b;
    hd_swap_halves(v, a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float hd_half_sum(float v) {
    float a, b;
    hd_swap_halves(v, a, b);
    return a + b;
}
// s_waitcnt vmcnt(n) for a wave-uniform n in 0..16 (a wave moves at most 2 * 8 pieces per tile)
__device__ __forceinline__ void hd_wait_vm(int n) {
#define VH_W(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (n) {
        VH_W(1) VH_W(2) VH_W(3) VH_W(4) VH_W(5) VH_W(6) VH_W(7) VH_W(8)
        VH_W(9) VH_W(10) VH_W(11) VH_W(12) VH_W(13) VH_W(14) VH_W(15) VH_W(16)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef VH_W
}
__device__ __forceinline__ void hd_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's LDS reads of the slot about to be refilled are done
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

template <int NB16, typename T, typename TO>
__global__ void __launch_bounds__(HdShape<NB16>::kMaxWaves * 64, HdShape<NB16>::kWavesPerEU)
attention_hd_kernel(const typename T::elem* __restrict__ qkv, typename TO::elem* __restrict__ out,
                    int tokens, int heads, int slabs, int ntiles) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    using vec4 = typename T::vec4;
    constexpr int HD = 16 * NB16;
    constexpr int NDB = (NB16 + 1) / 2;          // 32-column output blocks
    constexpr bool HALF_LAST = (NB16 & 1) != 0;  // the last block holds 16 real columns
    constexpr int kTile = NB16 * 1024;           // bytes of one matrix tile (32 rows x hd)
    constexpr int kV = kSlots * kTile;           // offset of the V slots
    __shared__ __attribute__((aligned(16))) char smem[2 * kSlots * kTile];   // K slots, then V slots
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int l31 = lane & 31, hl = lane >> 5;
    const int D = heads * HD;
    const int64_t ld = 3 * (int64_t)D;

    const int item = blockIdx.x;
    const int bh = item / slabs, slab = item - bh * slabs;
    const int b = bh / heads, h = bh - b * heads;
    const elem* const base = qkv + (int64_t)b * tokens * ld + (int64_t)h * HD;   // q of (b, h); K at + D, V at + 2 D
    const int q0 = (slab * nw + wave) * 32;

    // ---- DMA of key tile t into slot t % kSlots: pieces g = wave, wave + nw, ... < NB16 of K and of V ------------------
    // Piece g = subtiles 4 g .. 4 g + 3 of the image; lane -> (row, chunk) inverts the layout above.  Byte offsets from
    // `base` stay below 2^32: row < 4097, row pitch 3 D * 2 <= 12 KiB.
    const int npieces = wave < NB16 ? (NB16 - wave + nw - 1) / nw : 0;   // per matrix and tile, wave-uniform
    auto issue_tile = [&](int t) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of hoisted into registers across the tile loop
        const uint32_t slot = (uint32_t)(t % kSlots) * (uint32_t)kTile;
        for (int g = wave; g < NB16; g += nw) {
            const int st = 4 * g + (ln >> 4), w = ln & 15;
            const int rg = st / NB16, p = st - rg * NB16;
            const int row = t * 32 + rg * 8 + ((w >> 1) ^ ((p & 1) << 2));
            const int r = row < tokens ? row : tokens - 1;   // rows >= tokens replicate the last row
            const int ch = 2 * p + ((w & 1) ^ (rg & 1));
            const uint32_t ok = (uint32_t)(r * (int)ld + ch * 8) * 2u + (uint32_t)D * 2u;
            asm_lds_dma16(base, ok, lds0 + slot + g * 1024);
            asm_lds_dma16(base, ok + (uint32_t)D * 2u, lds0 + kV + slot + g * 1024);
        }
    };

    // this wave's Q fragments (rows >= tokens: the last row), then the first kSlots - 1 tiles
    vec8 qf[NB16];
    {
        int qrow = q0 + l31;
        qrow = qrow < tokens ? qrow : tokens - 1;
        const elem* qp = base + (int64_t)qrow * ld + 8 * hl;
#pragma unroll
        for (int ks = 0; ks < NB16; ++ks) qf[ks] = *(const vec8*)(qp + 16 * ks);
    }
    for (int t = 0; t < kSlots - 1 && t < ntiles; ++t) issue_tile(t);

    // per-lane LDS offsets.  K (row l31, chunk 2 ks + hl): kb0 + 256 ks, bit 7 flipped on odd ks.  V^T (rows 4 hl + tq of
    // row group rg, chunk 4 db + 2 (g4 & 1) + (tp >> 1), half tp & 1): vb[rg & 1] + 256 (NB16 rg + 2 db); the half last
    // block reads through vh[], which drops the (g4 & 1) part (columns 16..31 of the block re-read columns 0..15)
    const int g4 = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
    const int kb0 = (l31 >> 3) * kTile / 4 + ((l31 & 7) << 5) + ((hl ^ ((l31 >> 3) & 1)) << 4);
    const int kb1 = kb0 ^ 128;
    const int vlo = (((tp >> 1)) << 4) + 8 * (tp & 1);
    const int vb0 = kV + (g4 & 1) * 256 + (((4 * hl + tq) ^ ((g4 & 1) << 2)) << 5) + vlo;
    const int vb1 = vb0 ^ 16;
    const int vh0 = kV + ((4 * hl + tq) << 5) + vlo;
    const int vh1 = vh0 ^ 16;

    f32x16 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float negm = 0.f;   // - (shift of this lane's query row), exp2 domain
    float lsum = 0.f;   // this lane's half of the row sum

    struct VFrag { vec8 f[2][NDB]; };   // V^T fragments of one tile: [k-step][column block]
    auto tile = [&](int kt, auto first_c, auto tail_c) {
        constexpr bool FIRST = decltype(first_c)::value, TAIL = decltype(tail_c)::value;
        // this wave's pieces of tile kt have landed (tile kt + 1 may stay in flight), then everyone's; tile kt - 1 is done
        hd_wait_vm(kt + 1 < ntiles ? 2 * npieces : 0);
        hd_barrier();
        if (kt + kSlots - 1 < ntiles) issue_tile(kt + kSlots - 1);   // into tile kt - 1's slot
        const int so = (kt % kSlots) * kTile;

        VFrag vfr;   // requested first: they arrive during the score MFMAs and the softmax
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const bool half = HALF_LAST && db == NDB - 1;
                const int rga = 2 * ks, rgc = 2 * ks + 1;   // keys 16 ks + 0..7 and 16 ks + 8..15
                const char* pa = smem + so + (half ? vh0 : vb0) + 256 * (NB16 * rga + 2 * db);
                const char* pc = smem + so + (half ? vh1 : vb1) + 256 * (NB16 * rgc + 2 * db);
                const vec4 a = T::tr_read(pa), c = T::tr_read(pc);
#pragma unroll
                for (int j = 0; j < 4; ++j) { vfr.f[ks][db][j] = a[j]; vfr.f[ks][db][4 + j] = c[j]; }
            }
        }
        // S^T tile: 32 keys x 32 queries, accumulators start at -shift (tile 0: at 0)
        f32x16 s;
        {
            vec8 kf[NB16];
#pragma unroll
            for (int ks = 0; ks < NB16; ++ks) kf[ks] = *(const vec8*)(smem + so + ((ks & 1) ? kb1 : kb0) + 256 * ks);
            __builtin_amdgcn_sched_barrier(0);
            const float init = FIRST ? 0.f : negm;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = init;
#pragma unroll
            for (int ks = 0; ks < NB16; ++ks) s = T::mfma32(kf[ks], qf[ks], s);
        }
        if constexpr (TAIL) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl >= tokens) s[r] = -INFINITY;
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = hd_half_max(mx);   // finite: every tile holds at least one key < tokens
        if constexpr (FIRST) {
            negm = -mx;         // the row's shift = its maximum over tile 0
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] -= mx;
        } else if (__builtin_amdgcn_ballot_w64(mx > kTau)) {   // rare: some row outgrew its shift by 2^kTau
            const float delta = fmaxf(mx, 0.f);
            const float alpha = __builtin_amdgcn_exp2f(-delta);
            negm -= delta;
            lsum *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int db = 0; db < NDB; ++db) o[db][r] *= alpha;
                s[r] -= delta;
            }
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
#pragma unroll
            for (int db = 0; db < NDB; ++db) o[db] = T::mfma32(vfr.f[ks][db], pf, o[db]);
        }
    };

    if (ntiles == 1) {
        tile(0, std::true_type{}, std::true_type{});
    } else {
        tile(0, std::true_type{}, std::false_type{});
        for (int kt = 1; kt + 1 < ntiles; ++kt) tile(kt, std::false_type{}, std::false_type{});
        tile(ntiles - 1, std::false_type{}, std::true_type{});
    }

    // ---- normalise and store: lane holds O[q][32*db + 8*rg + 4*hl + 0..3] (widened as in the 64-wide kernel) ----------
    const float ltot = hd_half_sum(lsum);
    const float inv = __builtin_amdgcn_rcpf(ltot);
    const int q = q0 + l31;
    const int64_t mrow = (int64_t)b * tokens + (q < tokens ? q : tokens - 1);
    typename TO::elem* const op = out + mrow * D + (int64_t)h * HD + 8 * hl;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
        const f32x16& ob = o[db];
        constexpr int kLast = HALF_LAST ? 2 : 4;   // 8-column groups stored in the last block
#pragma unroll
        for (int rg = 0; rg < (db == NDB - 1 ? kLast : 4); rg += 2) {
            if constexpr (sizeof(typename TO::elem) == 2) {
                // a permlane32_swap per packed dword on a pair of 8-column groups: lanes 0-31 end with group rg, lanes
                // 32-63 with rg + 1 -- 16 bytes per lane and pair
                const u32x2 ga = __builtin_bit_cast(u32x2, pack4<TO>(ob[4 * rg] * inv, ob[4 * rg + 1] * inv, ob[4 * rg + 2] * inv, ob[4 * rg + 3] * inv));
                const u32x2 gb = __builtin_bit_cast(u32x2, pack4<TO>(ob[4 * rg + 4] * inv, ob[4 * rg + 5] * inv, ob[4 * rg + 6] * inv, ob[4 * rg + 7] * inv));
                const auto sx = __builtin_amdgcn_permlane32_swap(ga[0], gb[0], false, false);
                const auto sy = __builtin_amdgcn_permlane32_swap(ga[1], gb[1], false, false);
                if (q < tokens) *(u32x4*)(op + (4 * db + rg) * 8) = u32x4{sx[0], sy[0], sx[1], sy[1]};
            } else {
                // e4m3: a lane's quad is one dword; the same exchange gives 8 bytes per lane and pair
                const uint32_t ga = pack4<TO>(ob[4 * rg] * inv, ob[4 * rg + 1] * inv, ob[4 * rg + 2] * inv, ob[4 * rg + 3] * inv);
                const uint32_t gb = pack4<TO>(ob[4 * rg + 4] * inv, ob[4 * rg + 5] * inv, ob[4 * rg + 6] * inv, ob[4 * rg + 7] * inv);
                const auto sx = __builtin_amdgcn_permlane32_swap(ga, gb, false, false);
                if (q < tokens) *(u32x2*)(op + 32 * db + 8 * rg) = u32x2{sx[0], sx[1]};
            }
        }
    }
}

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
