// kernels_attn_hd.hip — the K/V-streaming multi-head attention kernel, for every head dim 32, 48, ..., 128 (gfx950).
//
// Same operation as kernels_attn.hip at any head dim hd = 16 * NB16 (NB16 = 2..8): row-major q|k|v [batch*T][3*H*hd] 16-bit
// with q pre-scaled by hd^-1/2 * log2(e), row-major output [batch*T][H*hd], any token count 1..kAttnStreamMaxTokens, without
// the resident forms' bound (those keep a whole head's K and V in LDS: ceil(T/32) * 8 KiB <= 160 KiB, T <= 640).  Here K and
// V pass through a fixed LDS ring of kSlots 32-key tiles, whatever T is.  The forward sends every model whose head dim is
// not 64 here; head dim 64 arrives here beyond 640 tokens (launch_attention's fallback) and through the two taps.
//
// Design (CDNA4), the resident ring kernel's idioms on a streamed image:
//   * work item = (image, head, query slab of nw*32 rows), one workgroup per item (nw <= kMaxWaves waves), blockIdx.x =
//     (image * heads + head) * slabs + slab: the slabs of a head are neighbours in the grid, so their K/V reads meet in L2.
//     No work-queue counter, no allocation: safe in a captured graph and when a batch is split across streams.
//   * key tile t lives in slot t % kSlots.  Its 2 * NB16 pieces of 1 KiB (K and V) are moved by LDS-DMA (asm_lds_dma16:
//     hipcc does not see the transfer, so it never drains vmcnt in front of ds_read_b64_tr_b16) by waves 0..NB16-1, or by
//     fewer waves several pieces each.  The DMA destination is lane-linear; the tile image's permutation goes on the lane's
//     global source address.
//   * per tile t: wait until this wave's pieces of tile t have landed (a counted vmcnt that leaves tile t+1 in flight),
//     barrier (every wave's pieces visible; every wave is done with tile t-1), refill tile t-1's slot with tile t+2, compute.
//   * S^T = K Q^T contracts over NB16 k-steps of v_mfma_f32_32x32x16 (a query's scores in one lane pair), row max / sum
//     finished with v_permlane32_swap, exp2-domain online softmax with the deferred rescale (the shift moves only when a
//     tile's scores exceed it by 2^kTau; O and l are rescaled once, no probabilities are pending), the converted accumulator
//     is the B operand of O^T = V^T P^T (NDB = ceil(hd / 32) 32x32 accumulators), V^T from ds_read_b64_tr_b16, widened
//     output stores.  For hd = 48, 80, 112 the last block covers 16 real V columns: its other 16 A rows re-read the real
//     ones (same LDS addresses, a broadcast) and their output rows are not stored.  An MFMA output row depends only on its
//     own A row, so they cannot touch the stored rows.
//   * keys >= T in the last tile are masked (their rows replicate row T-1: finite data under zero probabilities); query
//     rows >= T are computed from the clamped row T-1 and not stored.  Image, head and plane bases are 64-bit.
//   * LDS per workgroup: kSlots * 2 * NB16 KiB (24 KiB at hd 64, 48 KiB at hd 128): at least three workgroups per CU.
// One skeleton, two tile images (TileImage below): the 128-byte-row image at head dim 64, the subtile image elsewhere.
#include <climits>
#include <type_traits>

#include "attn_common.h"

namespace vh {
namespace {

constexpr int kSlots = 3;        // ring depth in 32-key tiles

// Per head dim: waves per workgroup and the register budget, the counted wait's range and the form of the half exchange.
//   * up to hd 64, 8 waves at <= 128 VGPRs (two workgroups of 8 fill a CU); beyond, the accumulators and fragments need more
//     (hd 80 spills at 128), so 4 waves at <= 256 VGPRs (at least two workgroups per CU).
//   * a wave moves at most 2 * NB16 pieces per tile.  Head dim 64 switches over exactly its 8 counts; the others keep one
//     switch of 16.
//   * head dim 64 exchanges the lane halves with the asm statement, every other head dim with the builtin (attn_common.h:
//     a half last block needs the builtin).
template <int NB16> struct HdShape {
    static constexpr int kMaxWaves = NB16 <= 4 ? 8 : 4;
    static constexpr int kWavesPerEU = NB16 <= 4 ? 4 : 2;
    static constexpr int kWaitCases = NB16 == 4 ? 8 : 16;
    static constexpr bool kAsmSwap = NB16 == 4;
};

// The image of one 32-key x hd tile of K or V in LDS (NB16 KiB per matrix and tile; K slots first, the V slots at kV), as
// three answers, all static and inlined:
//   * dma_piece: which global (row, K chunk, V chunk) lane ln of DMA piece g moves (16-byte chunks of the head's row; rows >=
//     tokens replicate the last row), and the two transfers themselves; the piece lands lane-linear at g * 1024 in its slot.
//     Byte offsets from `base` stay below 2^32: row < 4097, row pitch 3 D * 2 <= 12 KiB;
//   * k_lane / k_odd, v_lane / v_second: this lane's offsets in a slot -- K for even k-steps and, from it, for odd ones; V for
//     piece c = 0 of a k-step (keys 16 ks + 8 c + 0..7) in a whole or in a half last block and, from it, for piece 1;
//     l31 = lane & 31 and hl = lane >> 5 are the kernel's own values (handing them in, not recomputing them, keeps hipcc's code);
//   * k_frag / v_frag: from such an offset, the K fragment of k-step ks and the V^T piece c of (k-step ks, column block db).
// `ring` is the start of the ring, `so` the slot's byte offset in it.  The kernel keeps the six lane offsets in registers
// across the tile loop and has no image arithmetic of its own.
//
// Every head dim but 64: the tile is cut into 8-row x 16-column subtiles of 256 B -- exactly one bank row -- in the order
// [row group rg = row / 8][column pair p = chunk / 2]; inside a subtile, 16-byte chunk (row, chunk) sits at
//     32 * ((row & 7) ^ 4 * (p & 1)) + 16 * ((chunk & 1) ^ (rg & 1)).
// ds_read_b128 of the K operand (16 lanes, one chunk, 16 rows that are distinct mod 16) lands on 16 distinct slots;
// ds_read_b64_tr_b16 of the V operand (a 32-lane half: 4 rows x 4 chunks x 2 halves in two neighbouring subtiles) lands on
// 32 distinct 8-byte pieces, the XOR by 4 * (p & 1) putting the odd subtile's rows on the other half of the bank row.
// Conflict-free at every hd, with no assumption on the row pitch (160 B at hd 80).  One 1 KiB DMA fills four consecutive
// subtiles (piece g = subtiles 4 g .. 4 g + 3); with NB16 >= 4 it reads 8 rows x 128 contiguous bytes.
template <int NB16> struct TileImage {
    static constexpr int kTile = NB16 * 1024;   // bytes of one matrix tile
    static constexpr int kV = kSlots * kTile;   // offset of the V slots
    static __device__ __forceinline__ void dma_piece(const void* base, uint32_t lds_k, uint32_t lds_v, int t, int g, int ln,
                                                     int tokens, int64_t ld, int D) {
        const int st = 4 * g + (ln >> 4), w = ln & 15;   // lane -> (row, chunk) inverts the layout above
        const int rg = st / NB16, p = st - rg * NB16;
        const int row = t * 32 + rg * 8 + ((w >> 1) ^ ((p & 1) << 2));
        const int r = row < tokens ? row : tokens - 1;
        const int ch = 2 * p + ((w & 1) ^ (rg & 1));
        const uint32_t ok = (uint32_t)(r * (int)ld + ch * 8) * 2u + (uint32_t)D * 2u;
        asm_lds_dma16(base, ok, lds_k + g * 1024);
        asm_lds_dma16(base, ok + (uint32_t)D * 2u, lds_v + g * 1024);
    }
    // K (row l31, chunk 2 ks + hl): k_lane + 256 ks, bit 7 flipped on odd ks.  V^T (rows 4 hl + tq of row group rg = 2 ks + c,
    // chunk 4 db + 2 (g4 & 1) + (tp >> 1), half tp & 1): v_lane + 256 (NB16 rg + 2 db), bit 4 flipped for c = 1; the half last
    // block's offset drops the (g4 & 1) part (columns 16..31 of the block re-read columns 0..15)
    static __device__ __forceinline__ int k_lane(int l31, int hl) {
        return (l31 >> 3) * kTile / 4 + ((l31 & 7) << 5) + ((hl ^ ((l31 >> 3) & 1)) << 4);
    }
    static __device__ __forceinline__ int k_odd(int kl) { return kl ^ 128; }
    static __device__ __forceinline__ int v_lane(int lane, int hl, bool half) {
        const int g4 = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
        const int vlo = (((tp >> 1)) << 4) + 8 * (tp & 1);
        if (half) return kV + ((4 * hl + tq) << 5) + vlo;
        return kV + (g4 & 1) * 256 + (((4 * hl + tq) ^ ((g4 & 1) << 2)) << 5) + vlo;
    }
    static __device__ __forceinline__ int v_second(int vl) { return vl ^ 16; }
    static __device__ __forceinline__ const char* k_frag(const char* ring, int so, int kl, int ks) { return ring + so + kl + 256 * ks; }
    static __device__ __forceinline__ const char* v_frag(const char* ring, int so, int vl, int ks, int db, int c) {
        return ring + so + vl + 256 * (NB16 * (2 * ks + c) + 2 * db);
    }
};

// Head dim 64: K and V rows of 128 bytes (piece g = rows 8 g .. 8 g + 7), a K chunk XOR-swizzled by (row >> 1) & 7 for the
// ds_read_b128 row reads, a V chunk by ((row >> 1) & 1) << 2 for the transposing reads -- the image of the resident ring form
// (kernels_attn.hip).  One lane offset serves every k-step and both pieces: the other K chunks are XORs (bits 4-5), the
// second 32-column block of V flips bit 6.  Kept beside the subtile image because that one is slower here: 0.976x at 257 and
// 0.989x at 1025 tokens (profiles/headdim_bench.txt), 1213 against 1128 instructions (profiles/attn_stream_merge_isa.txt).
template <> struct TileImage<4> {
    static constexpr int kTile = 4096;
    static constexpr int kV = kSlots * kTile;
    static __device__ __forceinline__ void dma_piece(const void* base, uint32_t lds_k, uint32_t lds_v, int t, int g, int ln,
                                                     int tokens, int64_t ld, int D) {
        const int lr_ = ln >> 3, pc_ = ln & 7;
        const int row = t * 32 + g * 8 + lr_;
        const int r = row < tokens ? row : tokens - 1;
        const int ck = pc_ ^ ((row >> 1) & 7);
        const int cv = pc_ ^ (((row >> 1) & 1) << 2);
        const uint32_t ok = (uint32_t)(r * (int)ld + ck * 8) * 2u + (uint32_t)D * 2u;
        const uint32_t ov = (uint32_t)(r * (int)ld + cv * 8) * 2u + (uint32_t)D * 4u;
        asm_lds_dma16(base, ok, lds_k + g * 1024);
        asm_lds_dma16(base, ov, lds_v + g * 1024);
    }
    static __device__ __forceinline__ int k_lane(int l31, int hl) {
        const int kswz = (l31 >> 1) & 7;
        return l31 * 128 + ((hl ^ kswz) << 4);
    }
    static __device__ __forceinline__ int k_odd(int kl) { return kl; }
    static __device__ __forceinline__ int v_lane(int lane, int, bool) {
        const int g4 = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;
        const int vrow0 = 4 * (g4 >> 1) + tq;
        const int vcolb = (16 * (g4 & 1) + 4 * tp) * 2;
        const int vx = ((vrow0 >> 1) & 1) << 6;
        return kV + vrow0 * 128 + (vcolb ^ vx);
    }
    static __device__ __forceinline__ int v_second(int vl) { return vl; }
    static __device__ __forceinline__ const char* k_frag(const char* ring, int so, int kl, int ks) { return ring + ((kl + so) ^ (ks << 5)); }
    static __device__ __forceinline__ const char* v_frag(const char* ring, int so, int vl, int ks, int db, int c) {
        return ring + ((vl + so) ^ (db << 6)) + ks * 2048 + c * 1024;
    }
};

template <int NB16, typename T, typename TO>
__global__ void __launch_bounds__(HdShape<NB16>::kMaxWaves * 64, HdShape<NB16>::kWavesPerEU)
attention_hd_kernel(const typename T::elem* __restrict__ qkv, typename TO::elem* __restrict__ out,
                    int tokens, int heads, int slabs, int ntiles) {
    using elem = typename T::elem;
    using vec8 = typename T::vec8;
    using vec4 = typename T::vec4;
    using Image = TileImage<NB16>;
    constexpr int HD = 16 * NB16;
    constexpr int NDB = (NB16 + 1) / 2;          // 32-column output blocks
    constexpr bool HALF_LAST = (NB16 & 1) != 0;  // the last block holds 16 real columns
    constexpr bool ASM_SWAP = HdShape<NB16>::kAsmSwap;
    static_assert(!(ASM_SWAP && HALF_LAST), "a half last block needs the builtin half exchange");
    constexpr int kTile = Image::kTile, kV = Image::kV;
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
    const int npieces = wave < NB16 ? (NB16 - wave + nw - 1) / nw : 0;   // per matrix and tile, wave-uniform
    auto issue_tile = [&](int t) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of hoisted into registers across the tile loop
        const uint32_t slot = (uint32_t)(t % kSlots) * (uint32_t)kTile;
        for (int g = wave; g < NB16; g += nw) Image::dma_piece(base, lds0 + slot, lds0 + kV + slot, t, g, ln, tokens, ld, D);
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

    // this lane's fragment offsets in a slot: K for even / odd k-steps, V for the two pieces of a k-step, whole and half block
    const int ke = Image::k_lane(l31, hl), ko = Image::k_odd(ke);
    const int v0 = Image::v_lane(lane, hl, false), v1 = Image::v_second(v0);
    const int h0 = Image::v_lane(lane, hl, true), h1 = Image::v_second(h0);

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
        wait_vm<HdShape<NB16>::kWaitCases>(kt + 1 < ntiles ? 2 * npieces : 0);
        ring_barrier();
        if (kt + kSlots - 1 < ntiles) issue_tile(kt + kSlots - 1);   // into tile kt - 1's slot
        const int so = (kt % kSlots) * kTile;

        VFrag vfr;   // requested first: they arrive during the score MFMAs and the softmax
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                const bool half = HALF_LAST && db == NDB - 1;
                const char* pa = Image::v_frag(smem, so, half ? h0 : v0, ks, db, 0);   // keys 16 ks + 0..7
                const char* pc = Image::v_frag(smem, so, half ? h1 : v1, ks, db, 1);   // keys 16 ks + 8..15
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
            for (int ks = 0; ks < NB16; ++ks) kf[ks] = *(const vec8*)Image::k_frag(smem, so, (ks & 1) ? ko : ke, ks);
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
        mx = cross_half_max<ASM_SWAP>(mx);   // finite: every tile holds at least one key < tokens
        if constexpr (FIRST) {
            negm = -mx;                      // the row's shift = its maximum over tile 0
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

    // ---- normalise and store: lane holds O[q][32*db + 8*rg + 4*hl + 0..3] (widened as in the resident ring form) -------
    const float ltot = cross_half_sum<ASM_SWAP>(lsum);
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
