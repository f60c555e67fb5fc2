// kernels_kmeans.hip — patch clustering (gfx950): k-means of the 16-bit operand rows of every listed image, each image on its own.
// Contract: include/vithip.h, "Patch clustering"; DESIGN.md 4.33.
//
//   kmeans_kernel   ONE workgroup of four waves per image, alive across all iterations; its phases are separated by workgroup
//                   barriers, nothing is shared between workgroups.  The centroids live in the caller's cent16 [n][k][W] (working
//                   state and result), the labels as bytes in LDS, the counts in LDS.
//     init          centroid j <- operand row floor((2 j + 1) np / (2 k)) of the image, or row j of init16; 16-byte copies.
//     half norms    VH_KMEANS_L2: h_j = 0.5 * sum of c_j^2, a wave per centroid in the piece order of the match's prepare pass
//                   (lane l adds its pieces of 8 elements l, l + 64, .., each as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)),
//                   then the xor butterfly); VH_KMEANS_COSINE: h_j = 0.
//     assign        the match kernel's step loop.  One step = (row tile of 128 patches, 64-element chunk of the width): 128 patch
//                   rows and 32 KB centroid rows (KB = 1 for k <= 32, else 2) of 128 bytes in one slot of a three-slot ring, moved
//                   by LDS-DMA in 1 KiB pieces (4 + KB per wave), the counted vmcnt and one barrier per step, the XOR row image of
//                   the match (16-byte chunk c of row r at 128 r + 16 (c ^ ((r >> 1) & 7))).  Wave w owns patches 32 w .. 32 w + 31
//                   of the tile against ALL centroids, the centroids as the MFMA's A operand: a lane's 16 accumulator values of
//                   block kb are one patch against centroids 32 kb + 8 (j / 4) + 4 (l >> 5) + j % 4, ascending in j.  After the
//                   tile's last chunk the lane folds s = acc - h_j with a strict > over ascending j, a centroid >= k never entering
//                   (by index: the clamped rows behind k replicate row k - 1), the two lane halves meet through one exchange, and
//                   the label lands in LDS as a byte (0xFF behind np) with an LDS add into its count.
//     update        sum^T [64 columns][k] = X^T [64][rows] onehot [rows][k] on v_mfma_f32_32x32x16, the patch index contracted.
//                   The waves split the 64-element chunks of the width among them and need no barrier: every wave streams the
//                   patch rows of its chunk through a ring of its own (three slots of 32 rows, 4 pieces each, counted vmcnt), X^T
//                   comes from the transposing LDS read of the attention kernels' V operand (same chunk swizzle), the one-hot
//                   operand is made in registers from eight label bytes and never exists in memory.  A lane ends with 16 columns
//                   (four runs of four) of one centroid per accumulator: L2 divides by the count, COSINE by sqrtf(S_j), rounds and
//                   stores 8 bytes per run.  S_j needs the whole unrounded row: COSINE runs the pass twice -- first only the piece
//                   sums of squares into LDS (k W / 8 floats) and, behind a barrier, S_j a wave per centroid in the piece order
//                   above; then the same sums again (same order, same bits), divided and stored.  An empty cluster, or S_j = 0,
//                   stores nothing: the centroid stays.
//     The hazard    the centroids are written by this workgroup's vector stores and read back by its own DMA and loads.  Every
//                   update and the init end with __threadfence() (agent scope: vmcnt(0) -- the stores have reached L2 -- and an
//                   L1 invalidate), the barrier, and __threadfence() again on the reading side, so that no line cached by the last
//                   assignment is served stale.  Inside the update a wave drains vmcnt after its stores: stores and DMA loads
//                   share the counter, so the counted wait of the next chunk starts from zero.
// No atomics on global memory, no scratch, no allocation, no counter; an image's result depends on its own rows alone.
#include <limits.h>
#include <math.h>

#include "attn_common.h"
#include "vh_kernels.h"

namespace vh {

namespace {

constexpr int kKmRows = 128;      // patch rows of an assignment tile
constexpr int kKmSlots = 3;       // ring depth in steps (both rings)
constexpr int kKmURows = 32;      // patch rows of an update step
constexpr int kKmUStep = kKmURows * 128;
constexpr int kKmLab = VH_MATCH_MAX_ROWS;   // label bytes

__device__ __forceinline__ bool km_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) of the squares of 8 consecutive elements
template <typename T>
__device__ __forceinline__ float km_piece_sq(typename T::vec8 v) {
#pragma clang fp contract(off)
    float q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float x = (float)v[j]; q[j] = x * x; }
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
}

template <typename T, int KB>
__global__ void __launch_bounds__(256)
kmeans_kernel(const typename T::elem* __restrict__ x16, const int32_t* __restrict__ images, int nimg, int np, int W, int k, int iters, int l2,
              const typename T::elem* __restrict__ init16, int32_t* __restrict__ labels, typename T::elem* cent16, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
    using E = typename T::elem;
    using V4 = typename T::vec4;
    using V8 = typename T::vec8;
    constexpr int kRows = kKmRows + 32 * KB, kStep = kRows * 128, kPieces = kRows / 8, kPerWave = kPieces / 4;
    extern __shared__ __attribute__((aligned(16))) char km_smem[];
    uint8_t* const lab = (uint8_t*)(km_smem + kKmSlots * kStep);
    float* const hs = (float*)(lab + kKmLab);   // [64] half norms
    float* const sj = hs + 64;                  // [64] S_j
    int* const cnt = (int*)(sj + 64);           // [64] counts
    float* const qs = (float*)(cnt + 64);       // [k][W / 8] piece sums of squares (COSINE)
    const uint32_t lds0 = (uint32_t)(uintptr_t)km_smem;
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hl = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int slot_img = blockIdx.x;
    int img = slot_img;
    if (images) img = images[slot_img];
    if ((unsigned)img >= (unsigned)nimg) {   // workgroup-uniform; device lists only: nothing is read, the centroids are not written
        for (int p = t; p < np; p += 256) labels[(int64_t)slot_img * np + p] = -1;
        if (counts && t < k) counts[(int64_t)slot_img * k + t] = 0;
        return;
    }
    const E* const X = x16 + (int64_t)img * np * W;
    E* const Cn = cent16 + (int64_t)slot_img * k * W;
    const int nkc = W / 64, npiece = W / 8;

    // ---- init: 16-byte copies, k * npiece of them
    for (int i = t; i < k * npiece; i += 256) {
        const int j = i / npiece, c = i - j * npiece;
        const E* const src = init16 ? init16 + (int64_t)j * W : X + (int64_t)(int)(((int64_t)(2 * j + 1) * np) / (2 * k)) * W;
        ((V8*)(Cn + (int64_t)j * W))[c] = ((const V8*)src)[c];
    }
    if (t < 64) { hs[t] = 0.f; sj[t] = 0.f; }

    // ---- assignment step s = (row tile s / nkc, chunk s % nkc) into slot s % 3: pieces g = wave, wave + 4, .. of 8 rows; rows
    // 0 .. 127 of a step are the patch tile, the rest the centroids.  Byte offsets from X / Cn stay below 2^32.
    const int ntiles = (np + kKmRows - 1) / kKmRows, nsteps = ntiles * nkc;
    auto issue = [&](int s) {
        int ln = lane;
        asm volatile("" : "+v"(ln));   // recomputed per issue instead of kept in registers across the loop
        const int rt = s / nkc, kc = s - rt * nkc;
        const uint32_t slot = lds0 + (uint32_t)(s % kKmSlots) * kStep;
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) {
            const int g = wave + 4 * i, r = 8 * g + (ln >> 3);
            const int c = (ln & 7) ^ ((r >> 1) & 7);
            const bool is_x = g < kKmRows / 8;   // wave-uniform
            int row = is_x ? rt * kKmRows + r : r - kKmRows;
            const int last = is_x ? np - 1 : k - 1;
            row = row < last ? row : last;
            const uint32_t off = ((uint32_t)row * (uint32_t)W + (uint32_t)(kc * 64 + 8 * c)) * 2u;
            asm_lds_dma16(is_x ? (const void*)X : (const void*)Cn, off, slot + (uint32_t)g * 1024u);
        }
    };
    const int xrow = 32 * wave + l31, xswz = (xrow >> 1) & 7;
    int crow[KB], cswz[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) { crow[kb] = kKmRows + 32 * kb + l31; cswz[kb] = (crow[kb] >> 1) & 7; }

    // ---- update: this wave's ring and its lane offsets.  A piece of 8 rows lands lane-linear; 16-byte chunk c of row r sits at
    // 128 r + 16 (c ^ 4 ((r >> 1) & 1)), the image the transposing read wants (attn_hd_kernel.h, TileImage<4>).
    const uint32_t uring = (uint32_t)wave * (kKmSlots * kKmUStep);
    const int nrt = (np + kKmURows - 1) / kKmURows;
    const int g4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int vlane = (4 * hl + tq) * 128 + (((16 * (g4 & 1) + 4 * tp) * 2) ^ (((tq >> 1) & 1) << 6));
    auto uissue = [&](int ch, int rt) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t slot = lds0 + uring + (uint32_t)(rt % kKmSlots) * kKmUStep;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int r = 8 * g + (ln >> 3);
            const int c = (ln & 7) ^ (((r >> 1) & 1) << 2);
            int row = rt * kKmURows + r;
            row = row < np - 1 ? row : np - 1;
            const uint32_t off = ((uint32_t)row * (uint32_t)W + (uint32_t)(ch * 64 + 8 * c)) * 2u;
            asm_lds_dma16((const void*)X, off, slot + (uint32_t)g * 1024u);
        }
    };
    // pass 0 of COSINE: only the piece sums of squares; otherwise divide, round and store
    auto update = [&](bool squares_only) {
        for (int ch = wave; ch < nkc; ch += 4) {
            f32x16 o[2][KB];
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int j = 0; j < 16; ++j) o[db][kb][j] = 0.f;
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the last chunk's reads of the ring are done
            __builtin_amdgcn_sched_barrier(0);
            for (int s = 0; s < kKmSlots - 1 && s < nrt; ++s) uissue(ch, s);
            for (int rt = 0; rt < nrt; ++rt) {
                wait_vm<8>(rt + 1 < nrt ? 4 : 0);   // this step's pieces have landed; the next step's may stay in flight
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);   // the reads of the slot about to be refilled are done
                __builtin_amdgcn_sched_barrier(0);
                if (rt + kKmSlots - 1 < nrt) uissue(ch, rt + kKmSlots - 1);
                const char* const st = km_smem + uring + (rt % kKmSlots) * kKmUStep;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    // element e of a fragment is patch 32 rt + 16 ks + 8 (e / 4) + 4 hl + e % 4
                    const uint8_t* const lp = lab + rt * kKmURows + 16 * ks + 4 * hl;
                    const uint32_t la = *(const uint32_t*)lp, lb = *(const uint32_t*)(lp + 8);
                    V8 pf[KB];
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) {
                        const uint32_t me = (uint32_t)(32 * kb + l31);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            pf[kb][e] = (E)(((la >> (8 * e)) & 0xFFu) == me ? 1.f : 0.f);
                            pf[kb][4 + e] = (E)(((lb >> (8 * e)) & 0xFFu) == me ? 1.f : 0.f);
                        }
                    }
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        const char* const pa = st + ((vlane ^ (db << 6)) + ks * 2048);
                        const V4 a = T::tr_read(pa), c = T::tr_read(pa + 1024);
                        V8 vf;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { vf[j] = a[j]; vf[4 + j] = c[j]; }
#pragma unroll
                        for (int kb = 0; kb < KB; ++kb) o[db][kb] = T::mfma32(vf, pf[kb], o[db][kb]);
                    }
                }
            }
            // o[db][kb][j]: centroid 32 kb + l31, column 64 ch + 32 db + 8 (j / 4) + 4 hl + j % 4
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const int cj = 32 * kb + l31;
                const int cjc = cj < k ? cj : k - 1;
                const int n = cnt[cjc];
                const float den = l2 ? (float)n : sqrtf(sj[cjc]);
                const bool live = cj < k && n > 0 && den > 0.f;
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) {
                        const float a0 = o[db][kb][4 * rg], a1 = o[db][kb][4 * rg + 1], a2 = o[db][kb][4 * rg + 2], a3 = o[db][kb][4 * rg + 3];
                        if (squares_only) {
                            const float h = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                            const float piece = h + __shfl_xor(h, 32);   // low half + high half of the 8 columns
                            if (hl == 0 && cj < k) qs[cj * npiece + ch * 8 + 4 * db + rg] = piece;
                        } else if (live) {
                            *(V4*)(Cn + (int64_t)cj * W + ch * 64 + 32 * db + 8 * rg + 4 * hl) = pack4<T>(a0 / den, a1 / den, a2 / den, a3 / den);
                        }
                    }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // stores share the counter with the next chunk's DMA
        }
    };

    for (int it = 0; it <= iters; ++it) {
        // the centroids' stores (init or update) are complete, then everyone's; nothing cached of the old ones is read
        __threadfence();
        __syncthreads();
        __threadfence();
        if (l2)
            for (int j = wave; j < k; j += 4) {
                float s = 0.f;
                for (int p = lane; p < npiece; p += 64) s += km_piece_sq<T>(((const V8*)(Cn + (int64_t)j * W))[p]);
                s = wave_sum(s);
                if (lane == 0) hs[j] = 0.5f * s;
            }
        if (t < 64) cnt[t] = 0;
        __syncthreads();

        // ---- assign
        for (int s = 0; s < kKmSlots - 1 && s < nsteps; ++s) issue(s);
        f32x16 acc[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[kb][j] = 0.f;
        int kc = 0, rt = 0;
        for (int s = 0; s < nsteps; ++s) {
            wait_vm<8>(s + 1 < nsteps ? kPerWave : 0);
            ring_barrier();
            if (s + kKmSlots - 1 < nsteps) issue(s + kKmSlots - 1);   // into step s - 1's slot
            const char* const st = km_smem + (s % kKmSlots) * kStep;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int c = 2 * ks + hl;
                const V8 xf = *(const V8*)(st + xrow * 128 + ((c ^ xswz) << 4));
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    const V8 cf = *(const V8*)(st + crow[kb] * 128 + ((c ^ cswz[kb]) << 4));
                    acc[kb] = T::mfma32(cf, xf, acc[kb]);
                }
            }
            if (++kc == nkc) {   // the tile's scores are complete
                float best = -INFINITY;
                int bj = INT_MAX;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int key = 32 * kb + 8 * (j >> 2) + 4 * hl + (j & 3);
                        const float v = acc[kb][j] - hs[key];
                        if (key < k && v > best) { best = v; bj = key; }
                        acc[kb][j] = 0.f;
                    }
                const float ob = __shfl_xor(best, 32);
                const int oj = __shfl_xor(bj, 32);
                if (km_before(ob, oj, best, bj)) bj = oj;
                if (bj == INT_MAX) bj = 0;   // (no finite score at all)
                const int p = rt * kKmRows + xrow;
                if (hl == 0) {
                    lab[p] = p < np ? (uint8_t)bj : (uint8_t)0xFF;
                    if (p < np) atomicAdd(&cnt[bj], 1);
                }
                kc = 0;
                ++rt;
            }
        }
        __syncthreads();
        if (it == iters) break;

        // ---- update
        if (!l2) {
            update(true);
            __syncthreads();
            for (int j = wave; j < k; j += 4) {
                float s = 0.f;
                for (int p = lane; p < npiece; p += 64) s += qs[j * npiece + p];
                s = wave_sum(s);
                if (lane == 0) sj[j] = s;
            }
            __syncthreads();
        }
        update(false);
    }

    for (int p = t; p < np; p += 256) labels[(int64_t)slot_img * np + p] = lab[p];
    if (counts && t < k) counts[(int64_t)slot_img * k + t] = cnt[t];
}

// fp32 <-> the operand type, 4 elements per thread: the given init on its way in (RNE), the centroids on their way out (exact)
template <typename T>
__global__ void __launch_bounds__(256) kmeans_round_kernel(const float* __restrict__ in, typename T::elem* __restrict__ out, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = ((const f32x4*)in)[i];
    ((typename T::vec4*)out)[i] = pack4<T>(v[0], v[1], v[2], v[3]);
}
template <typename T>
__global__ void __launch_bounds__(256) kmeans_widen_kernel(const typename T::elem* __restrict__ in, float* __restrict__ out, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const typename T::vec4 v = ((const typename T::vec4*)in)[i];
    ((f32x4*)out)[i] = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

template <typename T, int KB>
hipError_t kmeans_launch(const KmeansArgs& a, hipStream_t s) {
    const size_t lds = (size_t)kKmSlots * (kKmRows + 32 * KB) * 128 + kKmLab + 3 * 64 * 4 +
                       (a.metric == VH_KMEANS_COSINE && a.iters > 0 ? (size_t)a.k * (a.width / 8) * 4 : 0);
    auto kern = kmeans_kernel<T, KB>;
    static LdsDone lds_done;   // per instantiation, per device
    if (hipError_t e = ensure_dynamic_lds((const void*)kern, lds, lds_done); e != hipSuccess) return e;
    using E = typename T::elem;
    hipLaunchKernelGGL(kern, dim3((unsigned)a.n), dim3(256), lds, s, (const E*)a.x16, a.images, a.images ? a.nimg : a.n, a.np, a.width, a.k,
                       a.iters, a.metric == VH_KMEANS_L2 ? 1 : 0, (const E*)a.init16, a.labels, (E*)a.cent16, a.counts);
    return hipGetLastError();
}

}  // namespace

const char* kmeans_check(const KmeansArgs& a) {
    if (!a.x16) return "kmeans: null rows";
    if (!a.labels || !a.cent16) return "kmeans: null output (labels and cent16 are both required)";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "kmeans: dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.metric != VH_KMEANS_COSINE && a.metric != VH_KMEANS_L2) return "kmeans: metric is not VH_KMEANS_COSINE or VH_KMEANS_L2";
    if (a.n < 1 || a.n > VH_MATCH_MAX_PAIRS) return "kmeans: n is outside 1..65536";
    if (a.np < 1 || a.np > VH_MATCH_MAX_ROWS) return "kmeans: np is outside 1..4096 rows";
    if (a.width < 64 || a.width > VH_MATCH_MAX_WIDTH || a.width % 64) return "kmeans: width is not a multiple of 64 in 64..2048";
    if (a.k < 2 || a.k > VH_KMEANS_MAX_K) return "kmeans: k is outside 2..64";
    if (a.k > a.np) return "kmeans: k exceeds np (more centroids than rows)";
    if (a.iters < 0 || a.iters > VH_KMEANS_MAX_ITERS) return "kmeans: iters is outside 0..64";
    if (a.images && a.nimg < 1) return "kmeans: images does not cover the list";
    if (((uintptr_t)a.x16 | (uintptr_t)a.images | (uintptr_t)a.init16 | (uintptr_t)a.labels | (uintptr_t)a.cent16 | (uintptr_t)a.counts) & 15)
        return "kmeans: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_kmeans(const KmeansArgs& a, hipStream_t s) {
    if (kmeans_check(a)) return hipErrorInvalidValue;
    return dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        return a.k <= 32 ? kmeans_launch<T, 1>(a, s) : kmeans_launch<T, 2>(a, s);
    });
}

hipError_t launch_kmeans_round(const float* in, void* out16, int dtype, int64_t n, hipStream_t s) {
    if (n < 4 || n % 4) return hipErrorInvalidValue;
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto tt) {
        using T = decltype(tt);
        hipLaunchKernelGGL((kmeans_round_kernel<T>), dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, in, (typename T::elem*)out16, n / 4);
        return hipGetLastError();
    });
}
hipError_t launch_kmeans_widen(const void* in16, float* out, int dtype, int64_t n, hipStream_t s) {
    if (n < 4 || n % 4) return hipErrorInvalidValue;
    return dispatch_dtype<BF16, FP16>(dtype, [&](auto tt) {
        using T = decltype(tt);
        hipLaunchKernelGGL((kmeans_widen_kernel<T>), dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, (const typename T::elem*)in16, out, n / 4);
        return hipGetLastError();
    });
}

}  // namespace vh
