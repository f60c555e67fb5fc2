// kernels_rollout.hip — attention rollout (gfx950): one step of the chain R_l = rownorm(fuse_h P_h + I) R_(l-1) per launch, and the
// read-out of the result.  Contract: include/vithip.h, "Attention rollout"; DESIGN.md 4.36.
//
//   rollout_kernel   A workgroup of four waves owns one image and 64 query rows.  Nothing T x T ever leaves the chip but R itself.
//     Scores.  One STEP = (head h, 64-key chunk c): the K rows of the chunk go global -> registers -> LDS (two buffers, the loads of
//       step s + 1 in flight under the arithmetic of step s, one barrier per step); the lane's q fragments come straight from global
//       into registers the same way (no other wave reads them).  An LDS K row is hd rounded up to 32 elements (zero-filled) plus 16
//       bytes, so the 16 rows of an operand read fall on the 16 different 16-byte columns of the 256-byte bank span.  Wave w takes
//       queries 16 w .. 16 w + 15 as the B operand and the chunk's four 16-key tiles as the A operand of v_mfma_f32_16x16x32: lane
//       l ends with ONE query (l & 15) and keys 16 kt + 4 (l >> 4) + r -- row statistics are in-lane folds plus the xor butterfly
//       16, 32.  Keys >= tokens are masked by index (their rows are clamped replicas of row tokens - 1).
//     Pass 1, head outer, chunk inner: the running row maximum m and the lane's share of l = sum 2^(s - m), rescaled when m moves;
//       after the head's last chunk (m, 1 / l) goes to an LDS table [heads][64].
//     Pass 2, chunk outer, head inner: the scores again, p = exp2(s - m) * (1 / l), fused over ascending heads in registers (mean:
//       serial adds, then * (float)(1 / H); max: fmaxf), + 1 where key == query, the lane's share of the row sum of A.  Then
//       - r_prev != null: the 64 x 64 fp32 chunk of A goes to LDS (row stride 68 floats) and every wave contracts all 64 rows of it
//         against rows `chunk` of R_prev on v_mfma_f32_16x16x4_f32 into ITS column tiles of the 64 x T accumulator -- tile ct * 4 + w,
//         ct < CT (CT = 1, 4, 7, 10: up to 160 accumulator registers at 640 tokens).  MFMA step j of a chunk sums keys 16 g + j, g =
//         0..3: per group of four steps the lane reads its A values as one float4 per row tile and its B values from global, 16 consecutive
//         columns of one R_prev row per quarter wave (64-byte segments out of L2: no wave shares a column tile with another, so LDS
//         would add a copy and save no traffic).  Rows and columns >= tokens enter as zeros, by index.
//       - r_prev == null (the identity): the lane stores its unnormalised values to R_new and rescales them in place at the end (it
//         re-reads only addresses it wrote itself).
//     The division by the row sum of A happens once, at the store: the scaling is linear.
//   rollout_readout_kernel   out[b][r][k] = R[b][r][k0 + k] (16-bit: its RNE), one thread per output element.
// No atomics, no scratch, no allocation: an image's result depends on its own rows alone.
#include <math.h>

#include "vh_kernels.h"

namespace vh {

namespace {

constexpr int kRoAStride = 68;   // floats per row of the A chunk in LDS

template <typename T, int CT>
__global__ void __launch_bounds__(256)
rollout_kernel(const typename T::elem* __restrict__ qkv, const float* __restrict__ r_prev, float* r_new, int tokens, int heads, int hd,
               int64_t ld, int64_t koff, int64_t hstep, int qblocks, int fuse_max, float inv_heads) {
    using E = typename T::elem;
    using V8 = typename T::vec8;
    extern __shared__ __attribute__((aligned(16))) char ro_smem[];
    const int nks = (hd + 31) >> 5, c8n = 4 * nks, kst = 64 * nks + 16;   // k-steps of 32; 16-byte pieces and bytes of an LDS K row
    char* const kbuf = ro_smem;                                           // [2][64][kst]
    float* const albs = (float*)(ro_smem + 2 * 64 * kst);                 // [64][kRoAStride]
    float* const rsum = albs + 64 * kRoAStride;                           // [64]
    float2* const tab = (float2*)(rsum + 64);                             // [heads][64]: (m, 1 / l)

    const int t = threadIdx.x, lane = t & 63, li = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int T_ = tokens, b = blockIdx.x / qblocks, q0 = (blockIdx.x - b * qblocks) * 64;
    const int nch = (T_ + 63) >> 6, npass = heads * nch, nsteps = 2 * npass;
    const E* const img = qkv + (int64_t)b * T_ * ld;
    const float* const rp = r_prev ? r_prev + (int64_t)b * T_ * T_ : nullptr;
    float* const rn = r_new + (int64_t)b * T_ * T_;
    const int qglob = q0 + 16 * wave + li, qrow = qglob < T_ ? qglob : T_ - 1;

    V8 zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (E)0.f;

    // the loads of one step (head h, chunk c): this thread's pieces p = t, t + 256, .. of the K chunk (row p / c8n, piece p % c8n), and the
    // lane's q fragments
    V8 kpre[4], qpre[4];
    auto load_k = [&](int h, int c) {
        const E* const hb = img + (int64_t)h * hstep + koff;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = t + 256 * i, row = p / c8n, pc = p - row * c8n;
            int key = c * 64 + row;
            key = key < T_ ? key : T_ - 1;
            kpre[i] = zero;
            if (p < 64 * c8n && pc * 8 < hd) kpre[i] = *(const V8*)(hb + (int64_t)key * ld + pc * 8);
        }
    };
    auto load_q = [&](int h) {
        const E* const hb = img + (int64_t)h * hstep + (int64_t)qrow * ld;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int pc = 4 * ks + g;
            qpre[ks] = zero;
            if (pc * 8 < hd) qpre[ks] = *(const V8*)(hb + pc * 8);
        }
    };

    f32x4 acc[4][CT];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 fz[4];             // the fused values of the chunk: key 16 kt + 4 g + r of query li
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) fz[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f, rs_part = 0.f;

    // step s = (head h, chunk c): pass 1 (s < npass) walks a head's chunks, pass 2 a chunk's heads
    int h = 0, c = 0;
    load_k(0, 0);
    load_q(0);
    for (int s = 0; s < nsteps; ++s) {
        char* const kb = kbuf + (s & 1) * 64 * kst;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = t + 256 * i, row = p / c8n, pc = p - row * c8n;
            if (p < 64 * c8n) *(V8*)(kb + row * kst + pc * 16) = kpre[i];
        }
        __syncthreads();   // this step's K is in place; the buffer written next was read two steps ago, in front of the last barrier
        int hn = h, cn = c;
        if (s + 1 < npass) { if (++cn == nch) { cn = 0; ++hn; } }
        else if (s + 1 == npass) { hn = 0; cn = 0; }
        else if (++hn == heads) { hn = 0; ++cn; }
        if (s + 1 < nsteps) load_k(hn, cn);

        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            if (ks < nks) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const V8 kf = *(const V8*)(kb + (16 * kt + li) * kst + (4 * ks + g) * 16);
                    sc[kt] = T::mfma16(kf, qpre[ks], sc[kt]);
                }
            }
        if (s + 1 < nsteps) load_q(hn);   // behind the last use of this step's fragments
        const int key0 = c * 64 + 4 * g;   // + 16 kt + r
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key0 + 16 * kt + r >= T_) sc[kt][r] = -INFINITY;

        if (s < npass) {
            // pass 1: key 0 of chunk 0 is never masked, so m is finite from the first chunk on
            float cm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) cm = fmaxf(cm, sc[kt][r]);
            cm = fmaxf(cm, __shfl_xor(cm, 16));
            cm = fmaxf(cm, __shfl_xor(cm, 32));
            const float mn = fmaxf(m_run, cm);
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) sum += __builtin_amdgcn_exp2f(sc[kt][r] - mn);
            l_run = l_run * __builtin_amdgcn_exp2f(m_run - mn) + sum;
            m_run = mn;
            if (c == nch - 1) {
                float l = l_run + __shfl_xor(l_run, 16);
                l += __shfl_xor(l, 32);
                if (g == 0) tab[h * 64 + 16 * wave + li] = make_float2(m_run, 1.0f / l);
                m_run = -INFINITY;
                l_run = 0.f;
            }
        } else {
            // pass 2 (the table entries are this wave's own; the barrier above ordered them)
            const float2 ml = tab[h * 64 + 16 * wave + li];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sc[kt][r] - ml.x) * ml.y;
                    fz[kt][r] = h == 0 ? p : fuse_max ? fmaxf(fz[kt][r], p) : fz[kt][r] + p;
                }
            if (h == heads - 1) {
                // the chunk of A = F + I, and the lane's share of its row sums
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float a = fuse_max ? fz[kt][r] : fz[kt][r] * inv_heads;
                        if (key0 + 16 * kt + r == qglob) a += 1.0f;
                        fz[kt][r] = a;
                        rs_part += a;
                    }
                if (!rp) {   // R_prev = I: A itself, normalised below
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int key = key0 + 16 * kt + r;
                            if (qglob < T_ && key < T_) rn[qglob * T_ + key] = fz[kt][r];
                        }
                } else {
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) *(f32x4*)(albs + (16 * wave + li) * kRoAStride + 16 * kt + 4 * g) = fz[kt];
                    __syncthreads();   // (uniform: h, heads and rp are the workgroup's)  The next write of albs lies behind the next step's barrier.
                    // MFMA step j = 4 jj + i sums keys 16 g + j of the chunk, g = 0..3
#pragma unroll 1
                    for (int jj = 0; jj < 4; ++jj) {
                        f32x4 af[4];    // row 16 rt + li, keys 16 g + 4 jj .. + 3
#pragma unroll
                        for (int rt = 0; rt < 4; ++rt) af[rt] = *(const f32x4*)(albs + (16 * rt + li) * kRoAStride + 16 * g + 4 * jj);
                        const int krow = c * 64 + 16 * g + 4 * jj;
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct) {
                            const int col0 = (ct * 4 + wave) * 16, col = col0 + li;
                            if (col0 < T_) {   // wave-uniform
                                float bv[4];
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
                                    const bool ok = krow + i < T_ && col < T_;
                                    const float v = rp[ok ? (krow + i) * T_ + col : 0];
                                    bv[i] = ok ? v : 0.f;
                                }
#pragma unroll
                                for (int i = 0; i < 4; ++i)
#pragma unroll
                                    for (int rt = 0; rt < 4; ++rt) acc[rt][ct] = mfma_f32(af[rt][i], bv[i], acc[rt][ct]);
                            }

                        }
                    }
                }
            }
        }
        h = hn;
        c = cn;
    }

    float rs = rs_part + __shfl_xor(rs_part, 16);
    rs += __shfl_xor(rs, 32);
    if (!rp) {
        if (qglob < T_)
            for (int c = 0; c < nch; ++c)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = c * 64 + 16 * kt + 4 * g + r;
                        if (key < T_) rn[qglob * T_ + key] = rn[qglob * T_ + key] / rs;
                    }
        return;
    }
    if (g == 0) rsum[16 * wave + li] = rs;
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int col = (ct * 4 + wave) * 16 + li;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + 4 * g + r;
                if (q0 + row < T_ && col < T_) rn[(q0 + row) * T_ + col] = acc[rt][ct][r] / rsum[row];
            }
    }
}

size_t rollout_lds_bytes(int heads, int hd) {
    const int kst = 64 * ((hd + 31) / 32) + 16;
    return (size_t)2 * 64 * kst + (size_t)64 * kRoAStride * 4 + 64 * 4 + (size_t)heads * 64 * 8;
}

template <typename T, int CT>
hipError_t rollout_launch(const RolloutArgs& a, hipStream_t s) {
    const size_t lds = rollout_lds_bytes(a.heads, a.head_dim);
    auto kern = rollout_kernel<T, CT>;
    static LdsDone lds_done;   // per instantiation, per device
    if (hipError_t e = ensure_dynamic_lds((const void*)kern, lds, lds_done); e != hipSuccess) return e;
    const int64_t D = (int64_t)a.heads * a.head_dim;
    const int64_t ld = a.in_hm_rows ? 64 : 3 * D, koff = a.in_hm_rows ? a.in_hm_rows * D : D, hstep = a.in_hm_rows ? a.in_hm_rows * 64 : a.head_dim;
    const int qblocks = (a.tokens + 63) / 64;
    hipLaunchKernelGGL(kern, dim3((unsigned)a.batch * (unsigned)qblocks), dim3(256), lds, s, (const typename T::elem*)a.qkv16, a.r_prev, a.r_new,
                       a.tokens, a.heads, a.head_dim, ld, koff, hstep, qblocks, a.fusion == VH_ROLLOUT_MAX ? 1 : 0, (float)(1.0 / a.heads));
    return hipGetLastError();
}

template <typename TO>
__global__ void __launch_bounds__(256)
rollout_readout_kernel(const float* __restrict__ store, int batch, int tokens, int rows, int k0, typename TO::elem* __restrict__ out) {
    const int K = tokens - k0;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)batch * rows * K) return;
    const int k = (int)(i % K);
    const int64_t br = i / K;
    const int r = (int)(br % rows);
    const int64_t b = br / rows;
    out[i] = (typename TO::elem)store[(b * tokens + r) * tokens + k0 + k];
}

}  // namespace

const char* rollout_check(const RolloutArgs& a) {
    if (!a.qkv16 || !a.r_new) return "null q|k|v or r_new";
    if (a.batch <= 0) return "batch must be positive";
    if (a.tokens < 1 || a.tokens > kRolloutMaxTokens) return "tokens outside 1..640";
    if (!attention_hd_supported(a.head_dim)) return "head_dim must be 32, 48, ..., 128";
    if (a.heads <= 0 || a.heads > kAttnHdMaxWidth / a.head_dim) return "heads * head_dim outside 1..2048";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "dtype is not VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.fusion != VH_ROLLOUT_MEAN && a.fusion != VH_ROLLOUT_MAX) return "fusion is not VH_ROLLOUT_MEAN or VH_ROLLOUT_MAX";
    if (a.in_hm_rows < 0) return "in_hm_rows is negative";
    if (a.in_hm_rows && a.head_dim != 64) return "head-major q|k|v exists at head_dim 64 only";
    if (a.in_hm_rows && a.in_hm_rows < (int64_t)a.batch * a.tokens) return "in_hm_rows holds fewer than batch * tokens rows";
    if ((int64_t)a.batch * ((a.tokens + 63) / 64) > 0x7fffffffll) return "batch * query blocks is too large";
    if ((uintptr_t)a.qkv16 & 15) return "qkv16 is not 16-byte aligned";
    // R is read and written as single floats at image offsets b * tokens^2, which are no multiple of four floats at odd token counts
    if (((uintptr_t)a.r_prev | (uintptr_t)a.r_new) & 3) return "r_prev or r_new is not 4-byte aligned";
    if (a.r_prev) {
        const uintptr_t n = (uintptr_t)a.batch * a.tokens * a.tokens * sizeof(float), p = (uintptr_t)a.r_prev, q = (uintptr_t)a.r_new;
        if (p < q + n && q < p + n) return "r_prev and r_new overlap";
    }
    return nullptr;
}

hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s) {
    if (rollout_check(a)) return hipErrorInvalidValue;
    const int ct = ((a.tokens + 15) / 16 + 3) / 4;   // column tiles per wave
    return dispatch_dtype<BF16, FP16>(a.dtype, [&](auto tt) {
        using T = decltype(tt);
        if (ct <= 1) return rollout_launch<T, 1>(a, s);
        if (ct <= 4) return rollout_launch<T, 4>(a, s);
        if (ct <= 7) return rollout_launch<T, 7>(a, s);
        return rollout_launch<T, 10>(a, s);
    });
}

const char* rollout_readout_check(int batch, int tokens, int rows, int k0, int elem) {
    if (batch <= 0) return "batch must be positive";
    if (tokens < 1 || tokens > kRolloutMaxTokens) return "tokens outside 1..640";
    if (rows < 1 || rows > tokens) return "rows outside 1..tokens";
    if (k0 < 0 || k0 >= tokens) return "first key column outside 0..tokens-1";
    if (elem != VH_ELEM_F32 && elem != VH_ELEM_F16 && elem != VH_ELEM_BF16) return "elem is not VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16";
    if (((int64_t)batch * rows * tokens + 255) / 256 > 0x7fffffffll) return "batch * rows * tokens is too large";
    return nullptr;
}

hipError_t launch_rollout_readout(const float* store, int batch, int tokens, int rows, int k0, int elem, void* out, hipStream_t s) {
    if (!store || !out || rollout_readout_check(batch, tokens, rows, k0, elem)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)batch * rows * (tokens - k0);
    const dim3 grid((unsigned)((n + 255) / 256));
    auto go = [&](auto t) {
        using TO = decltype(t);
        hipLaunchKernelGGL(rollout_readout_kernel<TO>, grid, dim3(256), 0, s, store, batch, tokens, rows, k0, (typename TO::elem*)out);
        return hipGetLastError();
    };
    if (elem == VH_ELEM_F32) return go(F32OUT{});
    return elem == VH_ELEM_F16 ? go(FP16{}) : go(BF16{});
}

}  // namespace vh
