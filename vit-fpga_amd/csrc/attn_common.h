// attn_common.h — what the attention kernels of kernels_attn.hip (K/V resident in LDS) and kernels_attn_hd.hip (K/V streamed)
// share: the rescale threshold of the online softmax, the exchange of a wave's halves, the tile barrier and the counted
// vmcnt wait.  Device code only; everything is inlined.
#pragma once

#include "vh_kernels.h"

namespace vh {

// the running shift of a query row is re-centred only when a tile's scores exceed it by more than 2^kTau: between
// re-centrings p = exp2(s - shift) <= 2^kTau, which fp32 sums and 16-bit P operands (fp16 max 65504) hold easily
constexpr float kTau = 8.0f;

// lanes l and l^32 hold the two halves of a query's row: combine them with one v_permlane32_swap
// (a VALU exchange of the wave's halves) instead of a ds_bpermute round trip through the LDS crossbar
// v_permlane32_swap vdst, src exchanges lanes 32-63 of vdst with lanes 0-31 of src IN PLACE, so the two
// operands must be different registers: with one register it degenerates to a plain half swap.  The copy is
// made opaque so the compiler cannot fold the operands back together.
template <bool ASM = true>
__device__ __forceinline__ void swap_halves(float v, float& lo_everywhere, float& hi_everywhere) {
    if constexpr (ASM) {
        // Whole exchange in one asm statement (hipcc 7.2 returned the same register for both results of
        // __builtin_amdgcn_permlane32_swap here).  s_nop 1 = the 2 wait states of the "VALU write ->
        // v_permlane read" hazard, which nobody pads inside inline asm; the trailing one covers the readers.
        float a = v, b;
        asm volatile("v_mov_b32 %1, %0\n\ts_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "=&v"(b));
        lo_everywhere = a;  // {v[0..31], v[0..31]}
        hi_everywhere = b;  // {v[32..63], v[32..63]}
    } else {
        // The builtin, for kernels in which an accumulator's registers die early (the half last block of kernels_attn_hd.hip:
        // rows 16..31 of its accumulator are dead after the last MFMA, the register allocator reuses them, and hipcc pads no
        // wait states inside an asm string -- an asm write there races the MFMA's late result writes, WAW).  Same values,
        // same sums: lo + hi in every lane.
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, v), __builtin_bit_cast(uint32_t, v), false, false);
        lo_everywhere = __builtin_bit_cast(float, (uint32_t)r[0]);
        hi_everywhere = __builtin_bit_cast(float, (uint32_t)r[1]);
    }
}
template <bool ASM = true>
__device__ __forceinline__ float cross_half_max(float v) {
    float a, b;
    swap_halves<ASM>(v, a, b);
    return fmaxf(a, b);
}
template <bool ASM = true>
__device__ __forceinline__ float cross_half_sum(float v) {
    float a, b;
    swap_halves<ASM>(v, a, b);
    return a + b;
}

// the barrier at the top of a key tile: every wave's DMA pieces of the tile are visible, every wave is done with the tile before
__device__ __forceinline__ void ring_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): this wave's LDS reads of the slot about to be refilled are done
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// s_waitcnt vmcnt(n) for a wave-uniform run-time n in 0..MAXN (the counter is an immediate, hence the switch); MAXN <= 40.
// Cases above MAXN fall into the default, so an instantiation's jump table ends at its own largest case.
template <int MAXN>
__device__ __forceinline__ void wait_vm(int n) {
    static_assert(MAXN >= 1 && MAXN <= 40, "extend the switch");
#define VH_W(N) case N: if constexpr (N <= MAXN) { asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break; } [[fallthrough]];
    switch (n) {
        VH_W(1) VH_W(2) VH_W(3) VH_W(4) VH_W(5) VH_W(6) VH_W(7) VH_W(8) VH_W(9) VH_W(10) VH_W(11) VH_W(12) VH_W(13) VH_W(14)
        VH_W(15) VH_W(16) VH_W(17) VH_W(18) VH_W(19) VH_W(20) VH_W(21) VH_W(22) VH_W(23) VH_W(24) VH_W(25) VH_W(26) VH_W(27)
        VH_W(28) VH_W(29) VH_W(30) VH_W(31) VH_W(32) VH_W(33) VH_W(34) VH_W(35) VH_W(36) VH_W(37) VH_W(38) VH_W(39) VH_W(40)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef VH_W
}

}  // namespace vh
