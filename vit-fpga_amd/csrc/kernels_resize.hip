// kernels_resize.hip — antialiased resize + crop of 8-bit interleaved frames in front of the u8 forward.
//
// CONTRACT (include/vithip.h, "8-bit frames").  Per axis, with n the source length, [lo, hi) the box, S outputs,
// scale = (hi - lo) / S and sup = max(scale, 1), output i has the centre c = lo + (i + 0.5) scale, the taps
// j in [max(floor(c - sup + 0.5), 0), min(floor(c + sup + 0.5), n)) and the weights max(0, 1 - |(j + 0.5 - c) / sup|), zero
// weights dropped, the rest divided by their sum -- all in double on the host (resize_axis_table), each weight then rounded ONCE to
// fp32.  The kernel runs the horizontal pass, then the vertical pass, each an fp32 __builtin_fmaf chain in ascending tap order from
// 0, no rounding in between; the byte is rintf(min(max(v, 0), 255)).
//
// KERNEL.  One launch for the whole batch.  A workgroup owns a tile of one frame's output: `band_rows` output rows x `tile_cols`
// output columns (tile_cols = S unless not even one output row's source rows fit).  It runs the horizontal pass over the source
// rows its band needs -- fp32 into LDS, [source row][column][channel] -- and then the vertical pass out of LDS: the source is read
// from HBM about once (neighbouring bands share sup rows, which the L2 serves), and no fp32 intermediate image exists in HBM.  The
// host picks band_rows and tile_cols per frame so that rows_needed x tile_cols x channels floats fit kResizeLdsFloats; the kernel
// recomputes rows_needed from the table and does nothing if it would not fit (it cannot, short of a corrupted table).
// Loads: bytes; one 32-bit load per tap and pixel for 4-channel frames whose offset and row stride are multiples of 4.  Stores:
// 16 bytes per thread where S * channels is a multiple of 16 and the tile spans whole rows; bytes otherwise.  No atomics, no work
// queue, no allocation.
#include <cmath>
#include <cstring>

#include "vh_kernels.h"

namespace vh {

// ---- host: the table of one axis -------------------------------------------------------------------------------------------
// Every expression is written as the contract states it and evaluated in IEEE double with no contraction, so that a numpy
// float64 transcription gives the same first / count and, after the one rounding, the same fp32 weights.
#pragma clang fp contract(off)
int resize_axis_table(int n_in, double lo, double hi, int n_out, int32_t* first, int32_t* count, float* weights, int max_taps) {
    return resize_axis_table_over(n_in, lo, hi, 0.0, n_out, first, count, weights, max_taps);
}

// the same table with a box that may overhang the last sample by `over` (kernels_resize_nv12.hip: left-sited chroma, a quarter of
// a sample); the tap clamp and the renormalisation below are what handles the overhang
int resize_axis_table_over(int n_in, double lo, double hi, double over, int n_out, int32_t* first, int32_t* count, float* weights,
                           int max_taps) {
    if (n_in < 1 || n_in > kResizeMaxSide || n_out < 1 || !first || !count || !weights || max_taps < 1) return 1;
    if (!(lo >= 0.0 && lo < hi && hi <= (double)n_in + over)) return 1;   // written so that a NaN fails
    const double scale = (hi - lo) / (double)n_out;
    if (!(scale <= (double)kResizeMaxScale)) return 1;
    const double sup = scale > 1.0 ? scale : 1.0;
    double w[kResizeMaxTaps + 2];
    for (int i = 0; i < n_out; ++i) {
        const double c = lo + ((double)i + 0.5) * scale;
        int j0 = (int)std::floor(c - sup + 0.5), j1 = (int)std::floor(c + sup + 0.5);
        if (j0 < 0) j0 = 0;
        if (j1 > n_in) j1 = n_in;
        if (j1 - j0 > kResizeMaxTaps + 2) return 1;
        int a = -1, b = -1;   // first and last tap with a non-zero weight
        for (int j = j0; j < j1; ++j) {
            const double d = std::fabs(((double)j + 0.5 - c) / sup);
            const double v = d < 1.0 ? 1.0 - d : 0.0;
            w[j - j0] = v;
            if (v != 0.0) { if (a < 0) a = j; b = j; }
        }
        if (a < 0 || b - a + 1 > max_taps) return 1;
        double sum = 0.0;
        for (int j = a; j <= b; ++j) sum += w[j - j0];
        first[i] = a;
        count[i] = b - a + 1;
        float* wi = weights + (size_t)i * max_taps;
        for (int t = 0; t < max_taps; ++t) wi[t] = t < b - a + 1 ? (float)(w[a + t - j0] / sum) : 0.f;
    }
    return 0;
}

// ---- host: descriptors + tables of one call --------------------------------------------------------------------------------
// words = [batch x RzFrame][tables]; a table is first[S] | count[S] | weights[S][stride], stride = the largest count of that axis.
// Frames that share (length, lo, hi) on an axis share the table (a batch from one camera builds two tables, or one).
struct RzFrame {
    uint64_t off;
    int32_t h, w, stride;
    int32_t xt, yt;            // word offsets of the two tables
    int32_t xs, ys;            // their weight strides
    int32_t band_rows, tile_cols;
    int32_t vec4;              // 4 channels, offset and row stride multiples of 4: one 32-bit load per tap and pixel
    int32_t pad[4];
};
static_assert(sizeof(RzFrame) == 4 * kResizeFrameWords, "RzFrame layout");

namespace {

struct AxisKey { int n; double lo, hi; int32_t at, stride, band_rows, tile_cols; };

// source rows the band [r0, r1) reads
inline int band_need(const int32_t* first, const int32_t* count, int r0, int r1) {
    int lo = first[r0], hi = first[r0] + count[r0];
    for (int r = r0 + 1; r < r1; ++r) {
        if (first[r] < lo) lo = first[r];
        if (first[r] + count[r] > hi) hi = first[r] + count[r];
    }
    return hi - lo;
}

int worst_need(const int32_t* first, const int32_t* count, int S, int k) {
    int need = 0;
    for (int r0 = 0; r0 < S; r0 += k) {
        const int n = band_need(first, count, r0, r0 + k < S ? r0 + k : S);
        if (n > need) need = n;
    }
    return need;
}

}  // namespace

const char* resize_plan_build(const vh_frame* desc, int batch, int channels, int S, size_t nbytes, bool base_aligned4,
                              std::vector<uint32_t>* words, int* max_tiles) {
    if (!desc || batch < 1 || channels < 1 || channels > kMaxChannels || S < 1 || S > 4096) return "resize: bad batch, channel count or output size";
    std::vector<AxisKey> keys;
    std::vector<int32_t> first(S), count(S);
    std::vector<float> wts((size_t)S * kResizeMaxTaps);
    words->assign((size_t)batch * kResizeFrameWords, 0u);
    *max_tiles = 1;
    // the table of one axis: found among those built for this call, or built and appended
    auto axis = [&](int n, double lo, double hi, bool vertical, AxisKey* out) -> const char* {
        for (const AxisKey& k : keys)
            if (k.n == n && k.lo == lo && k.hi == hi && (!vertical || k.band_rows > 0)) { *out = k; return nullptr; }
        if (resize_axis_table(n, lo, hi, S, first.data(), count.data(), wts.data(), kResizeMaxTaps)) return "resize: box outside the frame, empty, or scale > 32";
        AxisKey k{n, lo, hi, (int32_t)words->size(), 1, 0, 0};
        for (int i = 0; i < S; ++i) if (count[i] > k.stride) k.stride = count[i];
        if (vertical) {
            // band height: the most output rows whose source rows fit the LDS at full width; else one row and fewer columns
            const int fit = kResizeLdsFloats / (S * channels);   // LDS rows at full width
            const int need1 = worst_need(first.data(), count.data(), S, 1);
            if (need1 > fit) {
                k.band_rows = 1;
                k.tile_cols = kResizeLdsFloats / (need1 * channels);   // >= 1: 65 taps x 64 channels = 4160 floats
            } else {
                const double scale = (hi - lo) / S;
                int kk = (int)((fit - need1) / (scale > 0.03125 ? scale : 0.03125)) + 1;
                if (kk > S) kk = S;
                while (kk > 1 && worst_need(first.data(), count.data(), S, kk) > fit) --kk;
                // a small batch: at least ~64 workgroups, while bands stay a few rows high
                const int want = (64 + batch - 1) / batch;
                const int cap = S / want > 1 ? S / want : 1;
                k.band_rows = kk < cap ? kk : cap;
                k.tile_cols = S;
            }
        }
        const size_t at = words->size();
        words->resize(at + 2 * (size_t)S + (size_t)S * k.stride);
        uint32_t* t = words->data() + at;
        memcpy(t, first.data(), 4 * (size_t)S);
        memcpy(t + S, count.data(), 4 * (size_t)S);
        for (int i = 0; i < S; ++i) memcpy(t + 2 * (size_t)S + (size_t)i * k.stride, wts.data() + (size_t)i * kResizeMaxTaps, 4 * (size_t)k.stride);
        keys.push_back(k);
        *out = k;
        return nullptr;
    };
    for (int b = 0; b < batch; ++b) {
        const vh_frame& d = desc[b];
        if (d.width < 1 || d.width > kResizeMaxSide || d.height < 1 || d.height > kResizeMaxSide) return "resize: width and height must be 1..8192";
        if ((int64_t)d.row_stride < (int64_t)d.width * channels) return "resize: row_stride < width * channels";
        const uint64_t span = (uint64_t)(d.height - 1) * (uint64_t)d.row_stride + (uint64_t)d.width * channels;
        if (d.offset > nbytes || span > nbytes - d.offset) return "resize: a frame ends beyond nbytes";
        AxisKey kx, ky;
        if (const char* e = axis(d.width, (double)d.box[0], (double)d.box[2], false, &kx)) return e;
        if (const char* e = axis(d.height, (double)d.box[1], (double)d.box[3], true, &ky)) return e;
        RzFrame f{};
        f.off = d.offset; f.h = d.height; f.w = d.width; f.stride = d.row_stride;
        f.xt = kx.at; f.xs = kx.stride; f.yt = ky.at; f.ys = ky.stride;
        f.band_rows = ky.band_rows; f.tile_cols = ky.tile_cols;
        f.vec4 = channels == 4 && base_aligned4 && d.offset % 4 == 0 && d.row_stride % 4 == 0;
        memcpy(words->data() + (size_t)b * kResizeFrameWords, &f, sizeof f);
        const int tiles = ((S + f.band_rows - 1) / f.band_rows) * ((S + f.tile_cols - 1) / f.tile_cols);
        if (tiles > *max_tiles) *max_tiles = tiles;
    }
    if ((int64_t)batch * *max_tiles > 0x7fffffffll) return "resize: too many tiles";
    return nullptr;
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)rintf(fminf(fmaxf(v, 0.f), 255.f)); }

__global__ void __launch_bounds__(256)
resize_u8_kernel(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ plan, uint8_t* __restrict__ out, int S, int C,
                 int max_tiles, int out_vec16) {
    __shared__ __attribute__((aligned(16))) float lds[kResizeLdsFloats];
    const int f = blockIdx.x / max_tiles, tile = blockIdx.x - f * max_tiles;
    const RzFrame d = *(const RzFrame*)(plan + (size_t)f * kResizeFrameWords);
    const int nc = (S + d.tile_cols - 1) / d.tile_cols, nb = (S + d.band_rows - 1) / d.band_rows;
    if (tile >= nb * nc) return;
    const int band = tile / nc;
    const int r0 = band * d.band_rows, r1 = min(r0 + d.band_rows, S);
    const int c0 = (tile - band * nc) * d.tile_cols, c1 = min(c0 + d.tile_cols, S);
    const int32_t* xfirst = (const int32_t*)(plan + d.xt);
    const int32_t* xcount = xfirst + S;
    const float* xw = (const float*)(xcount + S);
    const int32_t* yfirst = (const int32_t*)(plan + d.yt);
    const int32_t* ycount = yfirst + S;
    const float* yw = (const float*)(ycount + S);
    int ylo = yfirst[r0], yhi = ylo + ycount[r0];
    for (int r = r0 + 1; r < r1; ++r) {
        ylo = min(ylo, yfirst[r]);
        yhi = max(yhi, yfirst[r] + ycount[r]);
    }
    const int rows = yhi - ylo, cols = c1 - c0, cw = cols * C;   // LDS: [rows][cols][C] floats
    if (rows * cw > kResizeLdsFloats || ylo < 0 || yhi > d.h) return;
    const uint8_t* src = frames + d.off;
    const int tid = threadIdx.x;

    // horizontal pass: source rows ylo .. yhi-1, output columns c0 .. c1-1
    if (d.vec4) {
        for (int e = tid; e < rows * cols; e += 256) {
            const int y = e / cols, x = c0 + (e - y * cols);
            const int n = xcount[x];
            const float* w = xw + (size_t)x * d.xs;
            const uint8_t* p = src + (size_t)(ylo + y) * d.stride + (size_t)xfirst[x] * 4;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            for (int t = 0; t < n; ++t) {
                const uint32_t q = *(const uint32_t*)(p + 4 * t);
                const float wt = w[t];
                a0 = __builtin_fmaf(wt, (float)(q & 0xffu), a0);
                a1 = __builtin_fmaf(wt, (float)((q >> 8) & 0xffu), a1);
                a2 = __builtin_fmaf(wt, (float)((q >> 16) & 0xffu), a2);
                a3 = __builtin_fmaf(wt, (float)(q >> 24), a3);
            }
            *(f32x4*)(lds + (size_t)e * 4) = f32x4{a0, a1, a2, a3};
        }
    } else {
        for (int e = tid; e < rows * cw; e += 256) {
            const int y = e / cw, rem = e - y * cw;
            const int xl = rem / C, ch = rem - xl * C, x = c0 + xl;
            const int n = xcount[x];
            const float* w = xw + (size_t)x * d.xs;
            const uint8_t* p = src + (size_t)(ylo + y) * d.stride + (size_t)xfirst[x] * C + ch;
            float acc = 0.f;
            for (int t = 0; t < n; ++t) acc = __builtin_fmaf(w[t], (float)p[(size_t)t * C], acc);
            lds[e] = acc;
        }
    }
    __syncthreads();

    // vertical pass: output rows r0 .. r1-1 out of LDS
    uint8_t* o = out + (((size_t)f * S + r0) * S + c0) * C;   // row r of the tile: o + (r - r0) * S * C
    if (out_vec16 && cols == S) {
        const int q = cw / 16;
        for (int e = tid; e < (r1 - r0) * q; e += 256) {
            const int rl = e / q, k = (e - rl * q) * 16, r = r0 + rl;
            const int n = ycount[r];
            const float* w = yw + (size_t)r * d.ys;
            const float* col = lds + (size_t)(yfirst[r] - ylo) * cw + k;
            f32x4 a[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            for (int t = 0; t < n; ++t) {
                const float wt = w[t];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v = *(const f32x4*)(col + (size_t)t * cw + 4 * i);
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[i][j] = __builtin_fmaf(wt, v[j], a[i][j]);
                }
            }
            u32x4 pk;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                pk[i] = to_byte(a[i][0]) | (to_byte(a[i][1]) << 8) | (to_byte(a[i][2]) << 16) | (to_byte(a[i][3]) << 24);
            *(u32x4*)(o + (size_t)rl * cw + k) = pk;
        }
    } else {
        for (int e = tid; e < (r1 - r0) * cw; e += 256) {
            const int rl = e / cw, rem = e - rl * cw, r = r0 + rl;
            const int n = ycount[r];
            const float* w = yw + (size_t)r * d.ys;
            const float* col = lds + (size_t)(yfirst[r] - ylo) * cw + rem;
            float acc = 0.f;
            for (int t = 0; t < n; ++t) acc = __builtin_fmaf(w[t], col[(size_t)t * cw], acc);
            o[(size_t)rl * S * C + rem] = (uint8_t)to_byte(acc);
        }
    }
}

hipError_t launch_resize_u8(const uint8_t* frames, const uint32_t* plan_dev, int batch, int channels, int S, int max_tiles,
                            uint8_t* out, hipStream_t s) {
    if (!frames || !plan_dev || !out || batch < 1 || channels < 1 || S < 1 || max_tiles < 1 || (int64_t)batch * max_tiles > 0x7fffffffll)
        return hipErrorInvalidValue;
    const int out_vec16 = (S * channels) % 16 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)(batch * max_tiles)), dim3(256), 0, s, frames, plan_dev, out, S, channels,
                       max_tiles, out_vec16);
    return hipGetLastError();
}

}  // namespace vh
