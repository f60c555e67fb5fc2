// kernels_dense.hip — dense linear heads on the patch rows a forward left in HBM (gfx950): per-patch logits, channels first, and
// the upsampled class map.  Contract: include/vithip.h, "Dense heads"; DESIGN.md 4.30.
//
//   dense_head_kernel    out[img][c][p] = bias[c] + sum_k a16[img * np + p][k] * w16[c][k]: a skinny GEMM, N = C <= 256 columns against
//                        M = batch * np rows, memory-bound on the rows.  One workgroup of four waves owns 64 patch rows and ALL C
//                        columns, so a row is read from HBM once; w16 (2 C dim bytes, the same for every workgroup) comes from L2.
//                        K runs in chunks of 64: the workgroup loads the chunk of both operands into registers one chunk ahead,
//                        turns the A pieces into the operand type (residual rows: x = hi + lo, optionally through the final LayerNorm,
//                        rounded to nearest even -- the steps of feat_row.h, so the bits are those of the token features) and parks both
//                        in LDS.  Wave w takes row half w & 1 (32 rows) and the 32-column blocks (w >> 1), (w >> 1) + 2, ..: at most
//                        four 32x32 fp32 accumulators (64 registers), one v_mfma_f32_32x32x16 per block and 16 k.  Columns C .. the
//                        next multiple of 32 exist in LDS (zeros) and in registers only.
//                        LDS image of both operands: [row or column][64 k + 8 pad] 16-bit elements, a row stride of 144 bytes.  An MFMA
//                        operand read is 16 bytes per lane, lane l reading row l & 31 at k = 16 ks + 8 (l >> 5); the hardware serves a
//                        16-byte read 16 lanes at a time, and 16 consecutive rows at 144 r bytes land on the 16 different 16-byte
//                        columns of the 256-byte bank span (9 r mod 16 is a permutation): conflict-free, for 12.5 % padding.
//                        Epilogue: the accumulators turn through LDS as [column][64 rows + 4 pad] fp32 (16-byte stores, four consecutive
//                        rows of a lane; 128 columns per pass), are read back with the ROW index fastest across lanes, take the bias and
//                        go out along the patch index of [C][np]: 64 consecutive elements per column where a block lies in one image.
//                        With VH_FEAT_NORM a first pass takes (mean, rstd) of the 64 rows, a wave per row, row_load / row_stats as the
//                        feature kernels run them; the K loop reads the rows a second time (L2 / MALL).
//                        No scratch, no allocation, no counter: nothing but its arguments, safe beside a graph replay.
//   dense_argmax_kernel  classes_out[img][y][x] = argmax_c of the bilinear interpolation (align_corners = False, source coordinate
//                        clamped at 0, the second tap clamped at the border) of logits [img][C][gh][gw] at out_h x out_w; ties and
//                        NaNs: the lowest index with the largest value wins (a strict > over ascending c, from -inf at index 0).
//                        One workgroup owns a 16 x 64 output tile of one image: it stages the [c][rows][cols] source window the tile's
//                        taps touch in LDS, as many channels at a time as fit 32 KiB (a window is at most gh x gw <= 4096 floats), and
//                        each thread walks the staged channels of its four pixels (x fixed, y = y0 + wave + 4 q) keeping (max, index).
//                        The interpolation is plain fp32 without contraction, in the order the header states.
#include <type_traits>

#include "feat_row.h"
#include "vh_kernels.h"

namespace vh {

namespace {

template <typename T> struct InRows16 {};   // the head's own operand form: plain rows of T (the tap)

constexpr int kDhRows = 64, kDhKc = 64, kDhStride = kDhKc + 8 /* 16-bit elements: 144 bytes */, kDhTileStride = kDhRows + 4 /* floats */;

template <typename T, typename IN> struct DhPiece { float v[8]; };                      // 8 elements of a residual row, fp32
template <typename T> struct DhPiece<T, InRows16<T>> { typename T::vec8 h; };           // 8 elements of the operand type

template <typename T, typename IN>
__device__ __forceinline__ void dh_load(DhPiece<T, IN>& p, const void* __restrict__ hi, const void* __restrict__ lo, int64_t e, bool ok) {
    if constexpr (std::is_same<IN, InRows16<T>>::value) {
        if (ok) p.h = *(const typename T::vec8*)((const typename T::elem*)hi + e);
        else p.h = typename T::vec8{};
    } else {
        if (ok) load_x<IN, 8>(hi, lo, e, p.v);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) p.v[j] = 0.f;
        }
    }
}

// the operand piece: a residual piece through the LayerNorm (norm, piece c of a row with statistics mean / rstd) and rounded RNE
template <typename T, typename IN>
__device__ __forceinline__ typename T::vec8 dh_operand(DhPiece<T, IN>& p, bool norm, int c, float mean, float rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta) {
    if constexpr (std::is_same<IN, InRows16<T>>::value) return p.h;
    else {
        if (norm) piece_norm(p.v, c, mean, rstd, gamma, beta);
        const typename T::vec4 a = pack4<T>(p.v[0], p.v[1], p.v[2], p.v[3]), b = pack4<T>(p.v[4], p.v[5], p.v[6], p.v[7]);
        return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

// M = images * np patch rows; patch row m = image m / np, patch m % np, lives in source row (m / np) * tokens + lead + m % np.
// NCB = 32-column blocks per wave: 1, 2 or 4 (C <= 64, 128, 256).  out [images][C][np] of `elem` (VH_ELEM_*).
template <typename T, typename IN, int NCB>
__global__ void __launch_bounds__(256)
dense_head_kernel(const void* __restrict__ hi, const void* __restrict__ lo, int64_t M, int np, int tokens, int lead, int dim,
                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int norm,
                  const typename T::elem* __restrict__ w16, const float* __restrict__ bias, int C, void* __restrict__ out, int elem) {
    using E = typename T::elem;
    using V8 = typename T::vec8;
    constexpr bool kRows16 = std::is_same<IN, InRows16<T>>::value;
    constexpr int kWCols = NCB * 64, kTileCols = kWCols < 128 ? kWCols : 128;
    constexpr int kABytes = kDhRows * kDhStride * 2, kWBytes = kWCols * kDhStride * 2, kTileBytes = kTileCols * kDhTileStride * 4;
    __shared__ __attribute__((aligned(16))) char smem[kABytes + kWBytes > kTileBytes ? kABytes + kWBytes : kTileBytes];
    __shared__ float stat[kDhRows][2];
    E* const As = (E*)smem;
    E* const Ws = (E*)(smem + kABytes);
    float* const tile = (float*)smem;   // the epilogue's image: behind the K loop's last barrier
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * kDhRows;

    if (!kRows16 && norm) {   // (mean, rstd) of the block's rows: wave w takes rows 16 w .. 16 w + 15, one after the other
        if constexpr (!kRows16) {
#pragma unroll 1
            for (int j = 0; j < 16; ++j) {
                const int r = wave * 16 + j;
                const int64_t m = m0 + r;
                if (m < M) {   // wave-uniform
                    const int64_t img = m / np;
                    float v[4][8];   // pieces beyond dim hold zeros: the sums are those of the feature kernels' narrower instantiations
                    row_load<IN, 4>(hi, lo, img * tokens + lead + (m - img * np), dim, lane, v);
                    float mean, rstd;
                    row_stats<4>(v, dim, lane, eps, mean, rstd);
                    if (lane == 0) { stat[r][0] = mean; stat[r][1] = rstd; }
                }
            }
        }
        __syncthreads();
    }

    // the loads of a chunk: thread t takes piece pc = t & 7 (k = 64 kc + 8 pc ..) of rows r0, r0 + 32 of A and of columns r0 + 32 i of W
    const int pc = t & 7, r0 = t >> 3;
    int64_t a_off[2];
    bool a_ok[2];
    float a_mean[2] = {0.f, 0.f}, a_rstd[2] = {1.f, 1.f};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t m = m0 + r0 + 32 * i;
        a_ok[i] = m < M;
        const int64_t img = a_ok[i] ? m / np : 0;
        a_off[i] = a_ok[i] ? (img * tokens + lead + (m - img * np)) * dim : 0;
        if (!kRows16 && norm && a_ok[i]) { a_mean[i] = stat[r0 + 32 * i][0]; a_rstd[i] = stat[r0 + 32 * i][1]; }
    }
    DhPiece<T, IN> ap[2];
    V8 wp[2 * NCB];
    auto load_chunk = [&](int kc) {
        const int k = kc * kDhKc + 8 * pc;
        const bool k_ok = k < dim;   // dim is a multiple of 8: a piece is inside or outside
#pragma unroll
        for (int i = 0; i < 2; ++i) dh_load<T, IN>(ap[i], hi, lo, a_off[i] + k, a_ok[i] && k_ok);
#pragma unroll
        for (int i = 0; i < 2 * NCB; ++i) {
            const int col = r0 + 32 * i;
            if (col < C && k_ok) wp[i] = *(const V8*)(w16 + (int64_t)col * dim + k);
            else wp[i] = V8{};
        }
    };

    const int rh = wave & 1, cp = wave >> 1, nblk = (C + 31) >> 5;
    f32x16 acc[NCB];
#pragma unroll
    for (int i = 0; i < NCB; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;

    const int nk = (dim + kDhKc - 1) / kDhKc;
    load_chunk(0);
    for (int kc = 0; kc < nk; ++kc) {
        const int k = kc * kDhKc + 8 * pc;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool nrm = !kRows16 && norm && a_ok[i] && k < dim;   // (outside: the piece is zeros and gamma has no such element)
            *(V8*)(As + (r0 + 32 * i) * kDhStride + 8 * pc) = dh_operand<T, IN>(ap[i], nrm, k >> 3, a_mean[i], a_rstd[i], gamma, beta);
        }
#pragma unroll
        for (int i = 0; i < 2 * NCB; ++i) *(V8*)(Ws + (r0 + 32 * i) * kDhStride + 8 * pc) = wp[i];
        __syncthreads();
        if (kc + 1 < nk) load_chunk(kc + 1);
#pragma unroll
        for (int ks = 0; ks < kDhKc / 16; ++ks) {
            const int ko = 16 * ks + 8 * (lane >> 5);
            const V8 av = *(const V8*)(As + (rh * 32 + (lane & 31)) * kDhStride + ko);
#pragma unroll
            for (int i = 0; i < NCB; ++i) {
                const int blk = cp + 2 * i;
                if (blk < nblk) {   // wave-uniform
                    const V8 bv = *(const V8*)(Ws + (blk * 32 + (lane & 31)) * kDhStride + ko);
                    acc[i] = T::mfma32(av, bv, acc[i]);
                }
            }
        }
        __syncthreads();   // the chunk has been read: its LDS image is free
    }

    // epilogue.  Register j of lane l of a 32x32 accumulator is row 8 (j / 4) + 4 (l >> 5) + j % 4, column l & 31.
    constexpr int kPasses = NCB == 4 ? 2 : 1;
    const int r = t & 63;
    const int64_t m = m0 + r, img = m < M ? m / np : 0;
    const int64_t obase = img * C * (int64_t)np + (m - img * np);
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        if (p) __syncthreads();   // the previous pass has been read
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
            const int i = 2 * p + ii;
            if (i < NCB) {
                const int blk = cp + 2 * i;
                if (blk < nblk) {
                    float* const w = tile + ((blk & 3) * 32 + (lane & 31)) * kDhTileStride + rh * 32 + 4 * (lane >> 5);
#pragma unroll
                    for (int g = 0; g < 4; ++g) *(f32x4*)(w + 8 * g) = f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
                }
            }
        }
        __syncthreads();
        if (m < M) {
            for (int cl = wave; cl < kTileCols; cl += 4) {
                const int c = p * 128 + cl;
                if (c >= C) break;
                float v = tile[cl * kDhTileStride + r];
                if (bias) v += bias[c];
                const int64_t o = obase + (int64_t)c * np;
                if (elem == VH_ELEM_F32) ((float*)out)[o] = v;
                else if (elem == VH_ELEM_F16) ((_Float16*)out)[o] = (_Float16)v;
                else ((__bf16*)out)[o] = (__bf16)v;
            }
        }
    }
}

template <typename T, typename IN>
hipError_t dense_head_launch_in(const DenseHeadArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + kDhRows - 1) / kDhRows)), block(256);
    const int norm = a.norm == VH_FEAT_NORM ? 1 : 0;
#define VH_DH_L(NCB) hipLaunchKernelGGL((dense_head_kernel<T, IN, NCB>), grid, block, 0, s, a.hi, a.lo, a.rows, a.group, a.tokens, a.lead, a.dim, a.gamma, \
                                        a.beta, a.eps, norm, (const typename T::elem*)a.w16, a.bias, a.classes, a.out, a.elem)
    if (a.classes <= 64) VH_DH_L(1);
    else if (a.classes <= 128) VH_DH_L(2);
    else VH_DH_L(4);
#undef VH_DH_L
    return hipGetLastError();
}

template <typename T>
hipError_t dense_head_launch(const DenseHeadArgs& a, hipStream_t s) {
    if (a.form == VH_DENSE_FORM_ROWS16) return dense_head_launch_in<T, InRows16<T>>(a, s);
    if (a.form == VH_FEAT_FORM_F32) return dense_head_launch_in<T, InF32>(a, s);
    return dense_head_launch_in<T, InSplit16<T>>(a, s);
}

// ---- upsample + argmax -------------------------------------------------------------------------------------------------------------
constexpr int kAmTileH = 16, kAmTileW = 64, kAmLdsFloats = 8192;

struct AxisTap { int i0, i1; float l0, l1; };
// output index d of an axis of n source samples: s = max(scale * (d + 0.5) - 0.5, 0), taps floor(s) and min(floor(s) + 1, n - 1),
// weights 1 - frac(s) and frac(s); scale = (float)n / (float)n_out.  Every operation rounds once (no contraction).
__device__ __forceinline__ AxisTap axis_tap(int d, float scale, int n) {
#pragma clang fp contract(off)
    float s = scale * ((float)d + 0.5f);
    s = s - 0.5f;
    if (s < 0.f) s = 0.f;
    int i0 = (int)s;
    if (i0 > n - 1) i0 = n - 1;
    const int i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    const float l1 = s - (float)i0;
    return AxisTap{i0, i1, 1.f - l1, l1};
}
__device__ __forceinline__ float bilinear(float v00, float v01, float v10, float v11, float lx0, float lx1, float ly0, float ly1) {
#pragma clang fp contract(off)
    const float a = lx0 * v00, b = lx1 * v01, c = lx0 * v10, d = lx1 * v11;
    const float top = a + b, bot = c + d;
    const float e = ly0 * top, f = ly1 * bot;
    return e + f;
}

__global__ void __launch_bounds__(256)
dense_argmax_kernel(const float* __restrict__ logits, int C, int gh, int gw, int oh, int ow, float sy, float sx, int tiles_x, int tiles_y,
                    uint8_t* __restrict__ cls_out, float* __restrict__ score_out) {
    __shared__ float win[kAmLdsFloats];
    const int t = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, img = b / tiles_y;
    const int x0 = tx * kAmTileW, y0 = ty * kAmTileH;
    const int x1 = x0 + kAmTileW < ow ? x0 + kAmTileW : ow, y1 = y0 + kAmTileH < oh ? y0 + kAmTileH : oh;
    // the window: the taps are monotonic in the output index, so the first pixel's first tap and the last pixel's second bound it
    const int c_lo = axis_tap(x0, sx, gw).i0, c_hi = axis_tap(x1 - 1, sx, gw).i1;
    const int r_lo = axis_tap(y0, sy, gh).i0, r_hi = axis_tap(y1 - 1, sy, gh).i1;
    const int wc = c_hi - c_lo + 1, wr = r_hi - r_lo + 1, wsz = wr * wc;   // <= gh * gw <= 4096
    int cc = kAmLdsFloats / wsz;
    if (cc > C) cc = C;

    const int x = x0 + (t & 63);
    const bool x_ok = x < x1;
    const AxisTap ax = axis_tap(x_ok ? x : x0, sx, gw);
    const int o0 = ax.i0 - c_lo, o1 = ax.i1 - c_lo;
    AxisTap ay[4];
    bool ok[4];
    float best[4];
    int arg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = y0 + (t >> 6) + 4 * q;
        ok[q] = x_ok && y < y1;
        ay[q] = axis_tap(y < y1 ? y : y0, sy, gh);
        best[q] = -INFINITY;
        arg[q] = 0;
    }
    const float* const src = logits + (int64_t)img * C * gh * gw;
    for (int c0 = 0; c0 < C; c0 += cc) {
        const int n = C - c0 < cc ? C - c0 : cc;
        if (c0) __syncthreads();   // the previous channels have been read
        for (int e = t; e < n * wsz; e += 256) {
            const int c = e / wsz, rem = e - c * wsz, rr = rem / wc, col = rem - rr * wc;
            win[e] = src[((int64_t)(c0 + c) * gh + r_lo + rr) * gw + c_lo + col];
        }
        __syncthreads();
        for (int c = 0; c < n; ++c) {
            const float* const wch = win + c * wsz;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (ok[q]) {
                    const float* const ra = wch + (ay[q].i0 - r_lo) * wc;
                    const float* const rb = wch + (ay[q].i1 - r_lo) * wc;
                    const float v = bilinear(ra[o0], ra[o1], rb[o0], rb[o1], ax.l0, ax.l1, ay[q].l0, ay[q].l1);
                    if (v > best[q]) { best[q] = v; arg[q] = c0 + c; }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (ok[q]) {
            const int64_t o = ((int64_t)img * oh + y0 + (t >> 6) + 4 * q) * ow + x;
            cls_out[o] = (uint8_t)arg[q];
            if (score_out) score_out[o] = best[q];
        }
    }
}

}  // namespace

const char* dense_head_check(const DenseHeadArgs& a) {
    if (!a.hi) return "dense_head: null rows";
    if (!a.w16) return "dense_head: null weights";
    if (!a.out) return "dense_head: null output";
    if (a.dtype != VH_DTYPE_BF16 && a.dtype != VH_DTYPE_FP16) return "dense_head: dtype must be VH_DTYPE_BF16 or VH_DTYPE_FP16";
    if (a.form != VH_DENSE_FORM_ROWS16 && a.form != VH_FEAT_FORM_F32 && a.form != a.dtype)
        return "dense_head: the rows are plain rows of the operand type, split planes of the operand type or fp32 rows";
    if (a.form == a.dtype && !a.lo) return "dense_head: split planes need the lo plane";
    if (a.form != a.dtype && a.lo) return "dense_head: only split planes take a lo plane";
    if (a.classes < 1 || a.classes > VH_DENSE_MAX_CLASSES) return "dense_head: classes outside 1..256";
    if (a.dim < 64) return "dense_head: dim below 64";
    if (a.dim > 2048) return "dense_head: dim above 2048";
    if (a.dim % 16) return "dense_head: dim must be a multiple of 16";
    if (a.group < 1 || a.group > kAttnStreamMaxTokens - 1) return "dense_head: group (rows per image) outside 1..4096";
    if (a.rows < 1 || a.rows > ((int64_t)1 << 30)) return "dense_head: rows outside 1..2^30";
    if (a.rows % a.group) return "dense_head: rows must be a multiple of group";
    if (a.lead < 0 || a.tokens != a.lead + a.group) return "dense_head: tokens must be lead + group";
    if (a.elem != VH_ELEM_F32 && a.elem != VH_ELEM_F16 && a.elem != VH_ELEM_BF16) return "dense_head: elem must be VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16";
    if (a.norm != VH_FEAT_NORM && a.norm != VH_FEAT_RAW) return "dense_head: norm must be VH_FEAT_NORM or VH_FEAT_RAW";
    if (a.norm == VH_FEAT_NORM) {
        if (a.form == VH_DENSE_FORM_ROWS16) return "dense_head: rows of the operand type pass no LayerNorm";
        if (!a.gamma || !a.beta) return "dense_head: VH_FEAT_NORM needs gamma and beta";
        if (!(a.eps > 0.f)) return "dense_head: eps must be positive";
    }
    const uintptr_t al = (uintptr_t)a.hi | (uintptr_t)a.lo | (uintptr_t)a.gamma | (uintptr_t)a.beta | (uintptr_t)a.w16 | (uintptr_t)a.bias | (uintptr_t)a.out;
    if (al & 15) return "dense_head: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_dense_head(const DenseHeadArgs& a, hipStream_t s) {
    if (dense_head_check(a)) return hipErrorInvalidValue;
    return a.dtype == VH_DTYPE_BF16 ? dense_head_launch<BF16>(a, s) : dense_head_launch<FP16>(a, s);
}

const char* dense_argmax_check(const float* logits, int batch, int classes, int gh, int gw, int out_h, int out_w, const uint8_t* classes_out,
                               const float* score_out) {
    if (!logits) return "dense_argmax: null logits";
    if (!classes_out) return "dense_argmax: null class map";
    if (batch < 1 || batch > (1 << 20)) return "dense_argmax: batch outside 1..2^20";
    if (classes < 1 || classes > VH_DENSE_MAX_CLASSES) return "dense_argmax: classes outside 1..256";
    if (gh < 1 || gh > 64 || gw < 1 || gw > 64) return "dense_argmax: the patch grid is outside 1..64 per side";
    if (out_h < 1 || out_h > VH_DENSE_MAX_SIDE || out_w < 1 || out_w > VH_DENSE_MAX_SIDE) return "dense_argmax: the output size is outside 1..4096 per side";
    const int64_t tiles = (int64_t)((out_w + kAmTileW - 1) / kAmTileW) * ((out_h + kAmTileH - 1) / kAmTileH) * batch;
    if (tiles > 0x7fffffff) return "dense_argmax: batch x output tiles exceeds 2^31 - 1 workgroups";
    if (((uintptr_t)logits | (uintptr_t)classes_out | (uintptr_t)score_out) & 15) return "dense_argmax: a device pointer is not 16-byte aligned";
    return nullptr;
}

hipError_t launch_dense_argmax(const float* logits, int batch, int classes, int gh, int gw, int out_h, int out_w, uint8_t* classes_out,
                               float* score_out, hipStream_t s) {
    if (dense_argmax_check(logits, batch, classes, gh, gw, out_h, out_w, classes_out, score_out)) return hipErrorInvalidValue;
    const int tiles_x = (out_w + kAmTileW - 1) / kAmTileW, tiles_y = (out_h + kAmTileH - 1) / kAmTileH;
    hipLaunchKernelGGL(dense_argmax_kernel, dim3((unsigned)(tiles_x * tiles_y) * (unsigned)batch), dim3(256), 0, s, logits, classes, gh, gw, out_h, out_w,
                       (float)gh / (float)out_h, (float)gw / (float)out_w, tiles_x, tiles_y, classes_out, score_out);
    return hipGetLastError();
}

}  // namespace vh
