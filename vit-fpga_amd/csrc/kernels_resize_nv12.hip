// kernels_resize_nv12.hip — NV12 video frames: antialiased resize + crop of both planes and the colour conversion in one launch,
// in front of the u8 forward.
//
// CONTRACT (include/vithip.h, "NV12 frames").  The Y plane (height x width bytes) and the UV plane (height/2 rows of width/2
// interleaved (U, V) pairs) are each resampled with the axis contract of the 8-bit frames (resize_axis_table: the same doubles,
// one rounding to fp32): Y over the box as given, UV as a 2-channel image of width/2 x height/2 over (lo/2 + delta, hi/2 + delta),
// delta = 0.25 horizontally for left-sited chroma and 0 otherwise.  Each plane runs the horizontal pass, then the vertical pass,
// each an fp32 __builtin_fmaf chain in ascending tap order from 0, nothing rounded in between -- the arithmetic of
// resize_u8_kernel.  The unrounded y, u, v of an output pixel then pass the 3 x 4 matrix m,
//     out[k] = fmaf(m[4k], y, fmaf(m[4k+1], u, fmaf(m[4k+2], v, m[4k+3]))),
// and the byte is rintf(min(max(out[k], 0), 255)): ONE rounding for resize and conversion together.
//
// KERNEL.  One launch for the whole batch, the structure of resize_u8_kernel: a 256-thread workgroup owns `band_rows` output rows x
// `tile_cols` output columns of one frame.  It runs the horizontal pass of the luma rows AND of the chroma rows its band needs
// into LDS as fp32 (UV [rows_c][cols][2] first, so that a pair is 8-byte aligned, then Y [rows_y][cols]), and after one barrier the
// vertical pass of both planes out of LDS, the matrix, and three bytes per pixel.  The source is read from HBM about once; no fp32
// and no YUV or RGB intermediate exists in HBM.  The host picks band_rows and tile_cols so that (rows_y + 2 rows_c) x cols floats
// fit kResizeLdsFloats; the kernel recomputes both row ranges from the tables and does nothing if they would not fit the LDS or
// either plane (they cannot, short of a corrupted table).  Loads: Y bytes; one 16-bit load per UV pair where uv_offset, uv_stride
// and the base are even, two bytes otherwise.  Stores: bytes.  No atomics, no work queue, no allocation.
//
// PLANAR YUV (include/vithip.h, "Planar YUV frames").  The same body with the chroma source a template parameter:
// U and V are two byte planes of cw x ch, cw = ceil(width / sub_x), ch = ceil(height / sub_y), sub 1 or 2 per axis, any parity of
// width and height.  Only the chroma half of the horizontal loop differs (p_u[t] and p_v[t] instead of the pair p[2t], p[2t+1]);
// the (u, v) pair lies in LDS as above, so the vertical pass, the matrix and the stores are shared.  With sub == 1 on an axis the
// chroma table of that axis IS the luma table (same key).  The body is a __host__ __device__ function of (block, thread) with the
// barrier passed in, so that tools/yuv_host_check.hip runs the very same text on the CPU under the sanitizers.
//
// 16-BIT SAMPLES (include/vithip.h, "16-bit YUV frames").  The same body again with the sample type T a template
// parameter beside PLANAR: P010 / P012 / P016 (T = uint16_t, semi-planar) and yuv4xxpNNle (T = uint16_t, planar).  Only the loads
// of the horizontal pass differ: a sample is one UNSIGNED 16-bit word that enters the fmaf chain as (float)word, unshifted and
// unmasked (depth and alignment live in the matrix); a semi-planar (U, V) pair is one 32-bit load where uv_offset, uv_stride and
// the base are multiples of 4 (the record's uv16 field) and two 16-bit loads otherwise.  The planner takes the sample width for
// its stride, span and evenness checks; the tables, the bands, the LDS layout (fp32 either way), the vertical pass, the matrix and
// the byte stores are those of the 8-bit instantiations, whose text is unchanged.
//
// PACKED 4:2:2 (include/vithip.h, "Packed 4:2:2 frames").  The body once more with the memory layout a third template
// parameter, PACKED: YUY2 / UYVY / YVYU / VYUY (T = uint8_t), Y210 / Y216 (T = uint16_t) and v210 (T = uint16_t, the record's layout
// = VH_422_V210).  A packed frame IS the planar 4:2:2 frame (sub_x = 2, sub_y = 1) of its de-interleaved planes: the planner feeds
// plan_frames that YuvSrc, so tables and bands are the planar ones, and only the loads of the horizontal pass differ.  Luma sample j
// is sample 2j + (layout & 1) of the row; a chroma tap takes its (U, V) from one macropixel, one 32-bit (64-bit) load where the
// record's uv16 says that base + offset and stride are multiples of the macropixel, single samples otherwise.  v210: sample slot s of
// a row is bits 10 (s % 3) .. 10 (s % 3) + 9 of 32-bit word s / 3 (three codes per word, four words per block of twelve slots); luma j
// is slot 2j + 1, U k slot 4k, V k slot 4k + 2; a code enters the arithmetic as (float)code * 64.0f, the Y210 word of that code.
//
// PACKED 4:4:4 (include/vithip.h, "Packed 4:4:4 frames").  BGR / BGRA / RGBA / ARGB, YUV24 / VUYA / AYUV (T = uint8_t),
// Y416 / AYUV64 and Y410 / v410 (T = uint16_t).  A packed 4:4:4 frame IS the planar 4:4:4 frame (sub_x = sub_y = 1) of its
// de-interleaved samples: the planner feeds plan_frames that YuvSrc, so tables and bands are the planar ones (one table per axis, three
// floats per column and source row).  The body is a text of its own, resize_packed444_body, because here ONE work item of the
// horizontal pass computes all three sums of a pixel: one 32-bit (64-bit) load per tap where the record's uv16 says the pixel is
// naturally aligned, single samples otherwise and always for 3-sample pixels (a wide load at the last pixel would leave the frame).
// Positions and shifts come from the record's layout word (VH_444: p0 | p1 << 2 | p2 << 4 | four << 6 | yuv << 7; bit 8: one 32-bit
// word of three 10-bit codes per pixel, bit 9: those codes start at bit 2); no branch names a format.  LDS: fp32 [rows][cols][3].
#include <cmath>
#include <cstring>
#include <type_traits>

#include "vh_kernels.h"

namespace vh {

// ---- host: descriptors + tables of one call --------------------------------------------------------------------------------
// words = [batch x RzNv12][tables]; a table is first[S] | count[S] | weights[S][stride], as in kernels_resize.hip.  Frames that
// share (length, lo, hi) on an axis share the table: a batch from one decoder builds four tables (luma x, luma y, chroma x,
// chroma y).
struct RzNv12 {
    uint64_t y_off, uv_off;        // planar: uv_off = the U plane
    int32_t h, w, y_stride, uv_stride;
    int32_t xt, yt, cxt, cyt;      // word offsets of the tables: luma x, luma y, chroma x, chroma y
    int32_t xs, ys, cxs, cys;      // their weight strides
    int32_t band_rows, tile_cols;
    int32_t uv16;                  // semi-planar: uv_offset, uv_stride and the base multiples of one (U, V) pair: one load per pair
                                   // (packed: of one macropixel)
    int32_t ch;                    // rows of the chroma plane(s): h / 2 (NV12), ceil(h / sub_y) (planar)
    uint64_t v_off;                // planar: the V plane, rows v_stride apart
    int32_t v_stride;
    int32_t layout;                // packed 4:2:2: VH_422_*; y_off = uv_off = the frame, y_stride = uv_stride = row_stride, ch = h
                                   // (packed 4:4:4: VH_444_*, the same fields; uv16: one load per pixel)
};
static_assert(sizeof(RzNv12) == 4 * kResizeNv12FrameWords, "RzNv12 layout");

namespace {

struct TableKey { int n; double lo, hi; int32_t at, stride; };
struct BandKey { int32_t yt, cyt, band_rows, tile_cols; };

// the most floats per output column any band of k rows keeps in LDS: luma rows + 2 x chroma rows
int worst_cost(const int32_t* yf, const int32_t* yc, const int32_t* cf, const int32_t* cc, int S, int k) {
    int worst = 0;
    for (int r0 = 0; r0 < S; r0 += k) {
        const int r1 = r0 + k < S ? r0 + k : S;
        int ylo = yf[r0], yhi = yf[r0] + yc[r0], clo = cf[r0], chi = cf[r0] + cc[r0];
        for (int r = r0 + 1; r < r1; ++r) {
            if (yf[r] < ylo) ylo = yf[r];
            if (yf[r] + yc[r] > yhi) yhi = yf[r] + yc[r];
            if (cf[r] < clo) clo = cf[r];
            if (cf[r] + cc[r] > chi) chi = cf[r] + cc[r];
        }
        const int cost = (yhi - ylo) + 2 * (chi - clo);
        if (cost > worst) worst = cost;
    }
    return worst;
}

// one frame of either layout, checked by its caller: what the shared planner reads
struct YuvSrc {
    uint64_t y_off, u_off, v_off;   // NV12: u_off = the UV plane, v_off unused
    int32_t h, w, cw, ch;           // luma size and the size of the chroma plane(s) in chroma samples
    int32_t y_stride, u_stride, v_stride;
    int32_t sub_x, sub_y;
    int32_t uv16;
    int32_t layout;                 // packed 4:2:2 only
    double box[4];
};

// tables, band heights and frame records of one call (both layouts); box_msg: the refusal when a table cannot be built
const char* plan_frames(const std::vector<YuvSrc>& src, int S, int chroma_site, const char* box_msg, std::vector<uint32_t>* words,
                        int* max_tiles) {
    const int batch = (int)src.size();
    std::vector<TableKey> keys;
    std::vector<BandKey> bands;
    std::vector<int32_t> first(S), count(S);
    std::vector<float> wts((size_t)S * kResizeMaxTaps);
    words->assign((size_t)batch * kResizeNv12FrameWords, 0u);
    *max_tiles = 1;
    // the table of one axis: found among those built for this call, or built and appended.  `over`: how far the box may overhang
    // the last sample (a quarter of a chroma sample with left siting; the tap clamp and the renormalisation take it)
    auto axis = [&](int n, double lo, double hi, double over, TableKey* out) -> const char* {
        for (const TableKey& k : keys)
            if (k.n == n && k.lo == lo && k.hi == hi) { *out = k; return nullptr; }
        if (resize_axis_table_over(n, lo, hi, over, S, first.data(), count.data(), wts.data(), kResizeMaxTaps)) return box_msg;
        TableKey k{n, lo, hi, (int32_t)words->size(), 1};
        for (int i = 0; i < S; ++i) if (count[i] > k.stride) k.stride = count[i];
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
        const YuvSrc& d = src[b];
        const double x0 = d.box[0], y0 = d.box[1], x1 = d.box[2], y1 = d.box[3];
        // horizontally sub-sampled, left-sited chroma: sample k sits on luma sample 2k
        const double dx = d.sub_x == 2 && chroma_site == VH_CHROMA_LEFT ? 0.25 : 0.0;
        const double sx = (double)d.sub_x, sy = (double)d.sub_y;
        TableKey kx, ky, kcx, kcy;
        if (const char* e = axis(d.w, x0, x1, 0.0, &kx)) return e;
        if (const char* e = axis(d.h, y0, y1, 0.0, &ky)) return e;
        if (const char* e = axis(d.cw, x0 / sx + dx, x1 / sx + dx, dx, &kcx)) return e;   // sub == 1: the luma key, the luma table
        if (const char* e = axis(d.ch, y0 / sy, y1 / sy, 0.0, &kcy)) return e;
        // band height of this pair of vertical tables: the most output rows whose luma + chroma source rows fit the LDS at full
        // width; else one row and fewer columns
        BandKey bk{ky.at, kcy.at, 0, 0};
        for (const BandKey& k : bands)
            if (k.yt == ky.at && k.cyt == kcy.at) bk = k;
        if (!bk.band_rows) {
            const int32_t* yf = (const int32_t*)(words->data() + ky.at);
            const int32_t* cf = (const int32_t*)(words->data() + kcy.at);
            const int fit = kResizeLdsFloats / S;   // floats per output column at full width
            const int cost1 = worst_cost(yf, yf + S, cf, cf + S, S, 1);
            if (cost1 > fit) {
                bk.band_rows = 1;
                bk.tile_cols = kResizeLdsFloats / cost1;   // >= 1: at most 3 x 65 floats per column (4:4:4 at scale 32)
            } else {
                // a further output row costs about scale luma rows + 2 x scale / sub_y chroma rows
                const double scale = (y1 - y0) / S;
                int kk = (int)((fit - cost1) / ((1.0 + 2.0 / sy) * (scale > 0.03125 ? scale : 0.03125))) + 1;
                if (kk > S) kk = S;
                while (kk > 1 && worst_cost(yf, yf + S, cf, cf + S, S, kk) > fit) --kk;
                // a small batch: at least ~64 workgroups, while bands stay a few rows high
                const int want = (64 + batch - 1) / batch;
                const int cap = S / want > 1 ? S / want : 1;
                bk.band_rows = kk < cap ? kk : cap;
                bk.tile_cols = S;
            }
            bands.push_back(bk);
        }
        RzNv12 f{};
        f.y_off = d.y_off; f.uv_off = d.u_off; f.v_off = d.v_off; f.h = d.h; f.w = d.w; f.ch = d.ch;
        f.y_stride = d.y_stride; f.uv_stride = d.u_stride; f.v_stride = d.v_stride;
        f.xt = kx.at; f.xs = kx.stride; f.yt = ky.at; f.ys = ky.stride;
        f.cxt = kcx.at; f.cxs = kcx.stride; f.cyt = kcy.at; f.cys = kcy.stride;
        f.band_rows = bk.band_rows; f.tile_cols = bk.tile_cols;
        f.uv16 = d.uv16; f.layout = d.layout;
        memcpy(words->data() + (size_t)b * kResizeNv12FrameWords, &f, sizeof f);
        const int tiles = ((S + f.band_rows - 1) / f.band_rows) * ((S + f.tile_cols - 1) / f.tile_cols);
        if (tiles > *max_tiles) *max_tiles = tiles;
    }
    return nullptr;
}

}  // namespace

// sample_bytes 1: NV12.  2: P010 / P012 / P016, whose offsets, strides and base must be even; base_mod4 = the base address & 3
// (0 for a host buffer, which is copied).  A message per refusal and per sample width.
const char* resize_plan_build_nv12(const vh_frame_nv12* desc, int batch, int S, size_t nbytes, unsigned base_mod4, int chroma_site,
                                   int sample_bytes, std::vector<uint32_t>* words, int* max_tiles) {
    const bool wide = sample_bytes == 2;
    if (sample_bytes != 1 && !wide) return "resize_nv12: sample_bytes must be 1 or 2";
    if (!desc || batch < 1 || S < 1 || S > 4096) return wide ? "resize_p016: bad batch or output size" : "resize_nv12: bad batch or output size";
    if (chroma_site != VH_CHROMA_CENTER && chroma_site != VH_CHROMA_LEFT)
        return wide ? "resize_p016: chroma_site must be VH_CHROMA_CENTER or VH_CHROMA_LEFT" : "resize_nv12: chroma_site must be VH_CHROMA_CENTER or VH_CHROMA_LEFT";
    if (wide && base_mod4 % 2) return "resize_p016: the device frames pointer is odd; 16-bit samples need a 2-byte aligned base";
    const unsigned pair = 2u * (unsigned)sample_bytes;   // bytes of one (U, V) pair
    std::vector<YuvSrc> src((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        const vh_frame_nv12& d = desc[b];
        if (d.width < 2 || d.width > kResizeMaxSide || d.height < 2 || d.height > kResizeMaxSide || d.width % 2 || d.height % 2)
            return wide ? "resize_p016: width and height must be even and 2..8192" : "resize_nv12: width and height must be even and 2..8192";
        if (wide && (d.y_offset % 2 || d.uv_offset % 2)) return "resize_p016: y_offset or uv_offset is odd; 16-bit samples need even byte offsets";
        if (wide && (d.y_stride % 2 || d.uv_stride % 2)) return "resize_p016: y_stride or uv_stride is odd; 16-bit samples need even byte strides";
        if (d.y_stride < sample_bytes * d.width || d.uv_stride < sample_bytes * d.width)
            return wide ? "resize_p016: y_stride or uv_stride < 2 * width bytes" : "resize_nv12: y_stride or uv_stride < width";
        const uint64_t yspan = (uint64_t)(d.height - 1) * (uint64_t)d.y_stride + (uint64_t)sample_bytes * (uint64_t)d.width;
        const uint64_t cspan = (uint64_t)(d.height / 2 - 1) * (uint64_t)d.uv_stride + (uint64_t)sample_bytes * (uint64_t)d.width;
        if (d.y_offset > nbytes || yspan > nbytes - d.y_offset) return wide ? "resize_p016: a Y plane ends beyond nbytes" : "resize_nv12: a Y plane ends beyond nbytes";
        if (d.uv_offset > nbytes || cspan > nbytes - d.uv_offset) return wide ? "resize_p016: a UV plane ends beyond nbytes" : "resize_nv12: a UV plane ends beyond nbytes";
        YuvSrc& s = src[b];
        s.y_off = d.y_offset; s.u_off = d.uv_offset; s.v_off = 0;
        s.h = d.height; s.w = d.width; s.cw = d.width / 2; s.ch = d.height / 2;
        s.y_stride = d.y_stride; s.u_stride = d.uv_stride; s.v_stride = 0;
        s.sub_x = 2; s.sub_y = 2;
        s.uv16 = base_mod4 % pair == 0 && d.uv_offset % pair == 0 && (unsigned)d.uv_stride % pair == 0;
        s.layout = 0;
        for (int i = 0; i < 4; ++i) s.box[i] = (double)d.box[i];
    }
    if (const char* e = plan_frames(src, S, chroma_site, wide ? "resize_p016: box outside the frame, empty, or scale > 32" : "resize_nv12: box outside the frame, empty, or scale > 32",
                                    words, max_tiles))
        return e;
    if ((int64_t)batch * *max_tiles > 0x7fffffffll) return wide ? "resize_p016: too many tiles" : "resize_nv12: too many tiles";
    return nullptr;
}

// every refusal of the planar contract has a message of its own, in the order the header lists them.  sample_bytes 1: byte planes.
// 2: yuv4xxpNNle, whose offsets, strides and base (base_even) must be even.
const char* resize_plan_build_yuv(const vh_frame_yuv* desc, int batch, int S, size_t nbytes, bool base_even, int chroma_site, int sample_bytes,
                                  std::vector<uint32_t>* words, int* max_tiles) {
    const bool wide = sample_bytes == 2;
    if (sample_bytes != 1 && !wide) return "resize_yuv: sample_bytes must be 1 or 2";
    if (!desc || batch < 1 || S < 1 || S > 4096) return wide ? "resize_yuv16: bad batch or output size" : "resize_yuv: bad batch or output size";
    if (chroma_site != VH_CHROMA_CENTER && chroma_site != VH_CHROMA_LEFT)
        return wide ? "resize_yuv16: chroma_site must be VH_CHROMA_CENTER or VH_CHROMA_LEFT" : "resize_yuv: chroma_site must be VH_CHROMA_CENTER or VH_CHROMA_LEFT";
    if (wide && !base_even) return "resize_yuv16: the device frames pointer is odd; 16-bit samples need a 2-byte aligned base";
    std::vector<YuvSrc> src((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        const vh_frame_yuv& d = desc[b];
        if (d.width < 1 || d.width > kResizeMaxSide || d.height < 1 || d.height > kResizeMaxSide)
            return wide ? "resize_yuv16: width and height must be 1..8192" : "resize_yuv: width and height must be 1..8192";
        if ((d.sub_x != 1 && d.sub_x != 2) || (d.sub_y != 1 && d.sub_y != 2))
            return wide ? "resize_yuv16: sub_x and sub_y must be 1 or 2" : "resize_yuv: sub_x and sub_y must be 1 or 2";
        const int cw = (d.width + d.sub_x - 1) / d.sub_x, ch = (d.height + d.sub_y - 1) / d.sub_y;
        if (wide && (d.y_offset % 2 || d.u_offset % 2 || d.v_offset % 2)) return "resize_yuv16: y_offset, u_offset or v_offset is odd; 16-bit samples need even byte offsets";
        if (wide && (d.y_stride % 2 || d.u_stride % 2 || d.v_stride % 2)) return "resize_yuv16: y_stride, u_stride or v_stride is odd; 16-bit samples need even byte strides";
        if (d.y_stride < sample_bytes * d.width) return wide ? "resize_yuv16: y_stride < 2 * width bytes" : "resize_yuv: y_stride < width";
        if (d.u_stride < sample_bytes * cw || d.v_stride < sample_bytes * cw)
            return wide ? "resize_yuv16: u_stride or v_stride < 2 * cw bytes, cw = ceil(width / sub_x)" : "resize_yuv: u_stride or v_stride < the chroma width, ceil(width / sub_x)";
        const uint64_t yspan = (uint64_t)(d.height - 1) * (uint64_t)d.y_stride + (uint64_t)sample_bytes * (uint64_t)d.width;
        const uint64_t uspan = (uint64_t)(ch - 1) * (uint64_t)d.u_stride + (uint64_t)sample_bytes * (uint64_t)cw;
        const uint64_t vspan = (uint64_t)(ch - 1) * (uint64_t)d.v_stride + (uint64_t)sample_bytes * (uint64_t)cw;
        if (d.y_offset > nbytes || yspan > nbytes - d.y_offset) return wide ? "resize_yuv16: a Y plane ends beyond nbytes" : "resize_yuv: a Y plane ends beyond nbytes";
        if (d.u_offset > nbytes || uspan > nbytes - d.u_offset) return wide ? "resize_yuv16: a U plane ends beyond nbytes" : "resize_yuv: a U plane ends beyond nbytes";
        if (d.v_offset > nbytes || vspan > nbytes - d.v_offset) return wide ? "resize_yuv16: a V plane ends beyond nbytes" : "resize_yuv: a V plane ends beyond nbytes";
        YuvSrc& s = src[b];
        for (int i = 0; i < 4; ++i) s.box[i] = (double)d.box[i];
        // written so that a NaN fails
        if (!(s.box[0] >= 0.0 && s.box[0] < s.box[2] && s.box[2] <= (double)d.width && s.box[1] >= 0.0 && s.box[1] < s.box[3] &&
              s.box[3] <= (double)d.height))
            return wide ? "resize_yuv16: box outside the frame, or empty" : "resize_yuv: box outside the frame, or empty";
        if (!((s.box[2] - s.box[0]) / (double)S <= (double)kResizeMaxScale && (s.box[3] - s.box[1]) / (double)S <= (double)kResizeMaxScale))
            return wide ? "resize_yuv16: scale > 32 on an axis" : "resize_yuv: scale > 32 on an axis";
        s.y_off = d.y_offset; s.u_off = d.u_offset; s.v_off = d.v_offset;
        s.h = d.height; s.w = d.width; s.cw = cw; s.ch = ch;
        s.y_stride = d.y_stride; s.u_stride = d.u_stride; s.v_stride = d.v_stride;
        s.sub_x = d.sub_x; s.sub_y = d.sub_y;
        s.uv16 = 0; s.layout = 0;
    }
    if (const char* e = plan_frames(src, S, chroma_site, wide ? "resize_yuv16: a table of the box could not be built" : "resize_yuv: a table of the box could not be built",
                                    words, max_tiles))
        return e;
    if ((int64_t)batch * *max_tiles > 0x7fffffffll) return wide ? "resize_yuv16: too many tiles" : "resize_yuv: too many tiles";
    return nullptr;
}

// packed 4:2:2: every refusal of the contract has a message of its own, in the order the header lists them.  sample_bytes 1: YUY2 and
// its three permutations.  2: Y210 / Y216 (layouts 0..3; offset, stride and base even) and v210 (multiples of 4).  base_mod8 = the
// base address & 7 (0 for a host buffer, which is copied).  The YuvSrc is the planar 4:2:2 frame of the de-interleaved planes.
const char* resize_plan_build_yuy2(const vh_frame_yuy2* desc, int batch, int S, size_t nbytes, unsigned base_mod8, int chroma_site,
                                   int sample_bytes, std::vector<uint32_t>* words, int* max_tiles) {
    const bool wide = sample_bytes == 2;
    if (sample_bytes != 1 && !wide) return "resize_yuy2: sample_bytes must be 1 or 2";
    if (!desc || batch < 1 || S < 1 || S > 4096) return wide ? "resize_y210: bad batch or output size" : "resize_yuy2: bad batch or output size";
    if (chroma_site != VH_CHROMA_CENTER && chroma_site != VH_CHROMA_LEFT)
        return wide ? "resize_y210: chroma_site must be VH_CHROMA_CENTER or VH_CHROMA_LEFT" : "resize_yuy2: chroma_site must be VH_CHROMA_CENTER or VH_CHROMA_LEFT";
    std::vector<YuvSrc> src((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        const vh_frame_yuy2& d = desc[b];
        if (d.width < 1 || d.width > kResizeMaxSide || d.height < 1 || d.height > kResizeMaxSide)
            return wide ? "resize_y210: width and height must be 1..8192" : "resize_yuy2: width and height must be 1..8192";
        if (!wide && d.layout == VH_422_V210) return "resize_yuy2: VH_422_V210 is a 10-bit layout; it goes to the 16-bit (_y210) entry points";
        if (d.layout < VH_422_YUYV || d.layout > VH_422_V210) return wide ? "resize_y210: layout must be one of VH_422_*" : "resize_yuy2: layout must be VH_422_YUYV, _UYVY, _YVYU or _VYUY";
        const bool v210 = d.layout == VH_422_V210;
        const int cw = (d.width + 1) / 2;
        // bytes of one row, and of the unit whose multiple base + offset and stride must be for the one-load chroma tap
        const int64_t row = v210 ? 16 * (int64_t)((d.width + 5) / 6) : 4 * (int64_t)sample_bytes * cw;
        const unsigned macro = 4u * (unsigned)sample_bytes;
        if (d.row_stride < row)
            return v210 ? "resize_y210: row_stride < 16 * ceil(width / 6) bytes (v210)" : wide ? "resize_y210: row_stride < 8 * cw bytes, cw = (width + 1) / 2"
                                                                                               : "resize_yuy2: row_stride < 4 * cw bytes, cw = (width + 1) / 2";
        if (v210) {
            if (d.offset % 4) return "resize_y210: offset is no multiple of 4; v210 words need 4-byte aligned offsets";
            if (d.row_stride % 4) return "resize_y210: row_stride is no multiple of 4; v210 words need 4-byte aligned rows";
            if (base_mod8 % 4) return "resize_y210: the device frames pointer is no multiple of 4; v210 words need a 4-byte aligned base";
        } else if (wide) {
            if (d.offset % 2) return "resize_y210: offset is odd; 16-bit samples need even byte offsets";
            if (d.row_stride % 2) return "resize_y210: row_stride is odd; 16-bit samples need even byte strides";
            if (base_mod8 % 2) return "resize_y210: the device frames pointer is odd; 16-bit samples need a 2-byte aligned base";
        }
        const uint64_t span = (uint64_t)(d.height - 1) * (uint64_t)d.row_stride + (uint64_t)row;
        if (d.offset > nbytes || span > nbytes - d.offset) return wide ? "resize_y210: a frame ends beyond nbytes" : "resize_yuy2: a frame ends beyond nbytes";
        YuvSrc& s = src[b];
        for (int i = 0; i < 4; ++i) s.box[i] = (double)d.box[i];
        // written so that a NaN fails
        if (!(s.box[0] >= 0.0 && s.box[0] < s.box[2] && s.box[2] <= (double)d.width && s.box[1] >= 0.0 && s.box[1] < s.box[3] &&
              s.box[3] <= (double)d.height))
            return wide ? "resize_y210: box outside the frame, or empty" : "resize_yuy2: box outside the frame, or empty";
        if (!((s.box[2] - s.box[0]) / (double)S <= (double)kResizeMaxScale && (s.box[3] - s.box[1]) / (double)S <= (double)kResizeMaxScale))
            return wide ? "resize_y210: scale > 32 on an axis" : "resize_yuy2: scale > 32 on an axis";
        s.y_off = s.u_off = s.v_off = d.offset;
        s.h = d.height; s.w = d.width; s.cw = cw; s.ch = d.height;
        s.y_stride = s.u_stride = s.v_stride = d.row_stride;
        s.sub_x = 2; s.sub_y = 1;
        s.uv16 = !v210 && (base_mod8 + d.offset) % macro == 0 && (unsigned)d.row_stride % macro == 0;
        s.layout = d.layout;
    }
    if (const char* e = plan_frames(src, S, chroma_site, wide ? "resize_y210: a table of the box could not be built" : "resize_yuy2: a table of the box could not be built",
                                    words, max_tiles))
        return e;
    if ((int64_t)batch * *max_tiles > 0x7fffffffll) return wide ? "resize_y210: too many tiles" : "resize_yuy2: too many tiles";
    return nullptr;
}

// packed 4:4:4: every refusal of the contract has a message of its own, in the order the header lists them.  sample_bytes 1: three or
// four bytes per pixel.  2: four 16-bit words per pixel (offset, stride and base even) or one 32-bit word of three 10-bit codes
// (multiples of 4), told apart per frame by the layout word.  base_mod8 = the base address & 7 (0 for a host buffer, which is copied).  The YuvSrc is the planar 4:4:4 frame of the de-interleaved samples; siting has nothing to act on.
const char* resize_plan_build_bgra(const vh_frame_bgra* desc, int batch, int S, size_t nbytes, unsigned base_mod8, int sample_bytes,
                                   std::vector<uint32_t>* words, int* max_tiles) {
    const bool wide = sample_bytes == 2;
    if (sample_bytes != 1 && !wide) return "resize_bgra: sample_bytes must be 1 or 2";
    if (!desc || batch < 1 || S < 1 || S > 4096) return wide ? "resize_y410: bad batch or output size" : "resize_bgra: bad batch or output size";
    std::vector<YuvSrc> src((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        const vh_frame_bgra& d = desc[b];
        if (d.width < 1 || d.width > kResizeMaxSide || d.height < 1 || d.height > kResizeMaxSide)
            return wide ? "resize_y410: width and height must be 1..8192" : "resize_bgra: width and height must be 1..8192";
        if (d.layout < 0 || (d.layout & ~0x3ff) || ((d.layout & 0x200) && !(d.layout & 0x100)))
            return wide ? "resize_y410: layout has bits outside those of VH_444 and the two 10-bit words" : "resize_bgra: layout has bits outside those of VH_444";
        const bool four = d.layout & 64, yuv = d.layout & 128, w10 = d.layout & 0x100;
        if (!four && ((d.layout & 3) == 3 || ((d.layout >> 2) & 3) == 3 || ((d.layout >> 4) & 3) == 3))
            return wide ? "resize_y410: position 3 in a pixel of three samples" : "resize_bgra: position 3 in a pixel of three samples";
        if (!wide && w10) return "resize_bgra: VH_444_Y410 / VH_444_V410 are 10-bit layouts; they go to the 16-bit (_y410) entry points";
        if (wide && w10 && d.layout != VH_444_Y410 && d.layout != VH_444_V410) return "resize_y410: a 10-bit layout must be VH_444_Y410 or VH_444_V410";
        if (wide && !w10 && !yuv) return "resize_y410: RGB words of 10 / 16 bits are not taken; the layout must have the yuv bit";
        if (wide && !w10 && !four) return "resize_y410: a pixel of 16-bit words has four samples; the layout must have the four bit";
        // bytes of one pixel; the unit whose multiple base + offset and stride must be for the one-load tap
        const int64_t px = w10 ? 4 : (four ? 4 : 3) * (int64_t)sample_bytes;
        const int64_t row = px * d.width;
        if (d.row_stride < row)
            return w10 ? "resize_y410: row_stride < 4 * width bytes (Y410 / V410)" : wide ? "resize_y410: row_stride < 8 * width bytes"
                       : four ? "resize_bgra: row_stride < 4 * width bytes" : "resize_bgra: row_stride < 3 * width bytes";
        if (w10) {
            if (d.offset % 4) return "resize_y410: offset is no multiple of 4; Y410 / V410 words need 4-byte aligned offsets";
            if (d.row_stride % 4) return "resize_y410: row_stride is no multiple of 4; Y410 / V410 words need 4-byte aligned rows";
            if (base_mod8 % 4) return "resize_y410: the device frames pointer is no multiple of 4; Y410 / V410 words need a 4-byte aligned base";
        } else if (wide) {
            if (d.offset % 2) return "resize_y410: offset is odd; 16-bit samples need even byte offsets";
            if (d.row_stride % 2) return "resize_y410: row_stride is odd; 16-bit samples need even byte strides";
            if (base_mod8 % 2) return "resize_y410: the device frames pointer is odd; 16-bit samples need a 2-byte aligned base";
        }
        const uint64_t span = (uint64_t)(d.height - 1) * (uint64_t)d.row_stride + (uint64_t)row;
        if (d.offset > nbytes || span > nbytes - d.offset) return wide ? "resize_y410: a frame ends beyond nbytes" : "resize_bgra: a frame ends beyond nbytes";
        YuvSrc& s = src[b];
        for (int i = 0; i < 4; ++i) s.box[i] = (double)d.box[i];
        // written so that a NaN fails
        if (!(s.box[0] >= 0.0 && s.box[0] < s.box[2] && s.box[2] <= (double)d.width && s.box[1] >= 0.0 && s.box[1] < s.box[3] &&
              s.box[3] <= (double)d.height))
            return wide ? "resize_y410: box outside the frame, or empty" : "resize_bgra: box outside the frame, or empty";
        if (!((s.box[2] - s.box[0]) / (double)S <= (double)kResizeMaxScale && (s.box[3] - s.box[1]) / (double)S <= (double)kResizeMaxScale))
            return wide ? "resize_y410: scale > 32 on an axis" : "resize_bgra: scale > 32 on an axis";
        s.y_off = s.u_off = s.v_off = d.offset;
        s.h = d.height; s.w = d.width; s.cw = d.width; s.ch = d.height;
        s.y_stride = s.u_stride = s.v_stride = d.row_stride;
        s.sub_x = 1; s.sub_y = 1;
        // one load per pixel: a 10-bit pixel IS one aligned word; 3-sample pixels never (the load would leave the frame at its last pixel)
        s.uv16 = w10 || (four && (base_mod8 + d.offset) % (uint64_t)px == 0 && (int64_t)d.row_stride % px == 0);
        s.layout = d.layout;
    }
    if (const char* e = plan_frames(src, S, VH_CHROMA_CENTER, wide ? "resize_y410: a table of the box could not be built" : "resize_bgra: a table of the box could not be built",
                                    words, max_tiles))
        return e;
    if ((int64_t)batch * *max_tiles > 0x7fffffffll) return wide ? "resize_y410: too many tiles" : "resize_bgra: too many tiles";
    return nullptr;
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------
struct Nv12Matrix { float m[12]; };
typedef __attribute__((ext_vector_type(2))) float f32x2;

__host__ __device__ __forceinline__ uint32_t nv12_byte(float v) { return (uint32_t)rintf(fminf(fmaxf(v, 0.f), 255.f)); }

// sample slot s of a v210 row, as the Y210 word of its code: exact (code < 2^10)
__host__ __device__ __forceinline__ float v210_sample(const uint32_t* __restrict__ row, uint32_t s) {
    const uint32_t wd = s / 3u;
    return (float)((row[wd] >> (10u * (s - 3u * wd))) & 0x3ffu) * 64.0f;
}

// The work of thread `tid` of workgroup `block`.  PLANAR: U and V are two planes, else one plane of (U, V) pairs.  T: the sample,
// uint8_t or uint16_t (unsigned: a word above 0x7fff must not sign-extend); strides and offsets are bytes either way.  `barrier`
// is __syncthreads() on the device; every return in front of it is taken by the whole workgroup.  PACKED: one plane of 4:2:2
// macropixels (PLANAR is then not read); its loads are the only text the other instantiations do not share.
template <bool PLANAR, class T, bool PACKED = false, class Barrier>
__host__ __device__ __forceinline__ void resize_yuv_body(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ plan,
                                                         uint8_t* __restrict__ out, int S, int max_tiles, const Nv12Matrix& mat, float* lds,
                                                         int block, int tid, Barrier barrier) {
    const int f = block / max_tiles, tile = block - f * max_tiles;
    const RzNv12 d = *(const RzNv12*)(plan + (size_t)f * kResizeNv12FrameWords);
    const int nc = (S + d.tile_cols - 1) / d.tile_cols, nb = (S + d.band_rows - 1) / d.band_rows;
    if (tile >= nb * nc) return;
    const int band = tile / nc;
    const int r0 = band * d.band_rows, r1 = r0 + d.band_rows < S ? r0 + d.band_rows : S;
    const int c0 = (tile - band * nc) * d.tile_cols, c1 = c0 + d.tile_cols < S ? c0 + d.tile_cols : S;
    const int32_t* xfirst = (const int32_t*)(plan + d.xt);
    const int32_t* xcount = xfirst + S;
    const float* xw = (const float*)(xcount + S);
    const int32_t* yfirst = (const int32_t*)(plan + d.yt);
    const int32_t* ycount = yfirst + S;
    const float* yw = (const float*)(ycount + S);
    const int32_t* cxfirst = (const int32_t*)(plan + d.cxt);
    const int32_t* cxcount = cxfirst + S;
    const float* cxw = (const float*)(cxcount + S);
    const int32_t* cyfirst = (const int32_t*)(plan + d.cyt);
    const int32_t* cycount = cyfirst + S;
    const float* cyw = (const float*)(cycount + S);
    int ylo = yfirst[r0], yhi = ylo + ycount[r0], clo = cyfirst[r0], chi = clo + cycount[r0];
    for (int r = r0 + 1; r < r1; ++r) {
        ylo = yfirst[r] < ylo ? yfirst[r] : ylo;
        yhi = yfirst[r] + ycount[r] > yhi ? yfirst[r] + ycount[r] : yhi;
        clo = cyfirst[r] < clo ? cyfirst[r] : clo;
        chi = cyfirst[r] + cycount[r] > chi ? cyfirst[r] + cycount[r] : chi;
    }
    const int rows_y = yhi - ylo, rows_c = chi - clo, cols = c1 - c0;
    if ((rows_y + 2 * rows_c) * cols > kResizeLdsFloats || ylo < 0 || yhi > d.h || clo < 0 || chi > d.ch) return;
    float* ldc = lds;                             // [rows_c][cols][2]
    float* ldy = lds + 2 * rows_c * cols;         // [rows_y][cols]
    const uint8_t* ysrc = frames + d.y_off;
    const uint8_t* csrc = frames + d.uv_off;
    const uint8_t* vsrc = frames + d.v_off;       // PLANAR only

    // horizontal pass: luma rows ylo .. yhi-1 and chroma rows clo .. chi-1, output columns c0 .. c1-1
    const int ny = rows_y * cols, nuv = rows_c * cols;
    for (int e = tid; e < ny + nuv; e += 256) {
        if (e < ny) {
            const int y = e / cols, x = c0 + (e - y * cols);
            const int n = xcount[x];
            const float* w = xw + (size_t)x * d.xs;
            float acc = 0.f;
            if constexpr (PACKED) {
                const uint8_t* row = ysrc + (size_t)(ylo + y) * d.y_stride;
                if (sizeof(T) == 2 && d.layout == VH_422_V210) {
                    const uint32_t s0 = 2u * (uint32_t)xfirst[x] + 1u;
                    for (int t = 0; t < n; ++t) acc = __builtin_fmaf(w[t], v210_sample((const uint32_t*)row, s0 + 2u * (uint32_t)t), acc);
                } else {
                    const T* p = (const T*)row + 2 * (size_t)xfirst[x] + (d.layout & 1);
                    for (int t = 0; t < n; ++t) acc = __builtin_fmaf(w[t], (float)p[2 * t], acc);
                }
            } else {
                const T* p = (const T*)(ysrc + (size_t)(ylo + y) * d.y_stride) + xfirst[x];
                for (int t = 0; t < n; ++t) acc = __builtin_fmaf(w[t], (float)p[t], acc);
            }
            ldy[e] = acc;
        } else {
            const int ec = e - ny;
            const int y = ec / cols, x = c0 + (ec - y * cols);
            const int n = cxcount[x];
            const float* w = cxw + (size_t)x * d.cxs;
            float u = 0.f, v = 0.f;
            if constexpr (PACKED) {
                // positions of U and V among the four samples of a macropixel: YUYV 1 3, UYVY 0 2, YVYU 3 1, VYUY 2 0
                const int upos = (d.layout ^ 1) & 3, vpos = upos ^ 2;
                const uint8_t* row = csrc + (size_t)(clo + y) * d.uv_stride;
                if (sizeof(T) == 2 && d.layout == VH_422_V210) {
                    const uint32_t s0 = 4u * (uint32_t)cxfirst[x];
                    for (int t = 0; t < n; ++t) {
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, v210_sample((const uint32_t*)row, s0 + 4u * (uint32_t)t), u);
                        v = __builtin_fmaf(wt, v210_sample((const uint32_t*)row, s0 + 4u * (uint32_t)t + 2u), v);
                    }
                } else if (d.uv16) {
                    typedef typename std::conditional<sizeof(T) == 2, uint64_t, uint32_t>::type Q;   // one macropixel
                    const Q* p = (const Q*)row + cxfirst[x];
                    const int ush = 8 * (int)sizeof(T) * upos, vsh = 8 * (int)sizeof(T) * vpos;
                    for (int t = 0; t < n; ++t) {
                        const Q q = p[t];
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, (float)(T)(q >> ush), u);
                        v = __builtin_fmaf(wt, (float)(T)(q >> vsh), v);
                    }
                } else {
                    const T* p = (const T*)row + 4 * (size_t)cxfirst[x];
                    for (int t = 0; t < n; ++t) {
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, (float)p[4 * t + upos], u);
                        v = __builtin_fmaf(wt, (float)p[4 * t + vpos], v);
                    }
                }
            } else if constexpr (PLANAR) {
                const T* pu = (const T*)(csrc + (size_t)(clo + y) * d.uv_stride) + cxfirst[x];
                const T* pv = (const T*)(vsrc + (size_t)(clo + y) * d.v_stride) + cxfirst[x];
                for (int t = 0; t < n; ++t) {
                    const float wt = w[t];
                    u = __builtin_fmaf(wt, (float)pu[t], u);
                    v = __builtin_fmaf(wt, (float)pv[t], v);
                }
            } else if constexpr (sizeof(T) == 2) {
                const uint8_t* p = csrc + (size_t)(clo + y) * d.uv_stride + (size_t)cxfirst[x] * 4;
                if (d.uv16) {
                    for (int t = 0; t < n; ++t) {
                        const uint32_t q = *(const uint32_t*)(p + 4 * t);
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, (float)(q & 0xffffu), u);
                        v = __builtin_fmaf(wt, (float)(q >> 16), v);
                    }
                } else {
                    const uint16_t* p16 = (const uint16_t*)p;
                    for (int t = 0; t < n; ++t) {
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, (float)p16[2 * t], u);
                        v = __builtin_fmaf(wt, (float)p16[2 * t + 1], v);
                    }
                }
            } else {
                const uint8_t* p = csrc + (size_t)(clo + y) * d.uv_stride + (size_t)cxfirst[x] * 2;
                if (d.uv16) {
                    for (int t = 0; t < n; ++t) {
                        const uint32_t q = *(const uint16_t*)(p + 2 * t);
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, (float)(q & 0xffu), u);
                        v = __builtin_fmaf(wt, (float)(q >> 8), v);
                    }
                } else {
                    for (int t = 0; t < n; ++t) {
                        const float wt = w[t];
                        u = __builtin_fmaf(wt, (float)p[2 * t], u);
                        v = __builtin_fmaf(wt, (float)p[2 * t + 1], v);
                    }
                }
            }
            *(f32x2*)(ldc + (size_t)ec * 2) = f32x2{u, v};
        }
    }
    barrier();

    // vertical pass of both planes out of LDS, the matrix, three bytes per pixel
    for (int e = tid; e < (r1 - r0) * cols; e += 256) {
        const int rl = e / cols, xl = e - rl * cols, r = r0 + rl;
        float y = 0.f, u = 0.f, v = 0.f;
        {
            const int n = ycount[r];
            const float* w = yw + (size_t)r * d.ys;
            const float* col = ldy + (size_t)(yfirst[r] - ylo) * cols + xl;
            for (int t = 0; t < n; ++t) y = __builtin_fmaf(w[t], col[(size_t)t * cols], y);
        }
        {
            const int n = cycount[r];
            const float* w = cyw + (size_t)r * d.cys;
            const float* col = ldc + ((size_t)(cyfirst[r] - clo) * cols + xl) * 2;
            for (int t = 0; t < n; ++t) {
                const f32x2 q = *(const f32x2*)(col + (size_t)t * cols * 2);
                const float wt = w[t];
                u = __builtin_fmaf(wt, q[0], u);
                v = __builtin_fmaf(wt, q[1], v);
            }
        }
        uint8_t* o = out + (((size_t)f * S + r) * S + c0 + xl) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = __builtin_fmaf(mat.m[4 * k], y, __builtin_fmaf(mat.m[4 * k + 1], u, __builtin_fmaf(mat.m[4 * k + 2], v, mat.m[4 * k + 3])));
            o[k] = (uint8_t)nv12_byte(c);
        }
    }
}

// Packed 4:4:4: the work of thread `tid` of workgroup `block`.  T: the sample, uint8_t (3 or 4 per pixel) or uint16_t (4 words per
// pixel, or one 32-bit word of three 10-bit codes).  All three components share the x and the y table of the record (xt, yt), so one
// item of the horizontal pass takes one pixel per tap and feeds three fmaf chains; LDS holds fp32 [rows][cols][3].  The branches on
// the layout word and on uv16 are uniform over the workgroup (one frame per workgroup), so a batch may mix layouts.
template <class T, class Barrier>
__host__ __device__ __forceinline__ void resize_packed444_body(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ plan,
                                                               uint8_t* __restrict__ out, int S, int max_tiles, const Nv12Matrix& mat, float* lds,
                                                               int block, int tid, Barrier barrier) {
    const int f = block / max_tiles, tile = block - f * max_tiles;
    const RzNv12 d = *(const RzNv12*)(plan + (size_t)f * kResizeNv12FrameWords);
    const int nc = (S + d.tile_cols - 1) / d.tile_cols, nb = (S + d.band_rows - 1) / d.band_rows;
    if (tile >= nb * nc) return;
    const int band = tile / nc;
    const int r0 = band * d.band_rows, r1 = r0 + d.band_rows < S ? r0 + d.band_rows : S;
    const int c0 = (tile - band * nc) * d.tile_cols, c1 = c0 + d.tile_cols < S ? c0 + d.tile_cols : S;
    const int32_t* xfirst = (const int32_t*)(plan + d.xt);
    const int32_t* xcount = xfirst + S;
    const float* xw = (const float*)(xcount + S);
    const int32_t* yfirst = (const int32_t*)(plan + d.yt);
    const int32_t* ycount = yfirst + S;
    const float* yw = (const float*)(ycount + S);
    int ylo = yfirst[r0], yhi = ylo + ycount[r0];
    for (int r = r0 + 1; r < r1; ++r) {
        ylo = yfirst[r] < ylo ? yfirst[r] : ylo;
        yhi = yfirst[r] + ycount[r] > yhi ? yfirst[r] + ycount[r] : yhi;
    }
    const int rows = yhi - ylo, cols = c1 - c0;
    if (3 * rows * cols > kResizeLdsFloats || ylo < 0 || yhi > d.h) return;   // what plan_frames prices at sub 1, 1: rows + 2 rows
    const uint8_t* src = frames + d.y_off;
    // the sample of the pixel that becomes output component k
    const int p0 = d.layout & 3, p1 = (d.layout >> 2) & 3, p2 = (d.layout >> 4) & 3;

    // horizontal pass: source rows ylo .. yhi-1, output columns c0 .. c1-1, three sums per item
    for (int e = tid; e < rows * cols; e += 256) {
        const int y = e / cols, x = c0 + (e - y * cols);
        const int n = xcount[x];
        const float* w = xw + (size_t)x * d.xs;
        const uint8_t* row = src + (size_t)(ylo + y) * d.y_stride;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (sizeof(T) == 2 && (d.layout & 0x100)) {
            // one 32-bit word per pixel, 10-bit codes at bits 10 p (+ 2); a code enters as the 16-bit word code << 6 (exact)
            const int lsb = (d.layout & 0x200) ? 2 : 0;
            const int s0 = 10 * p0 + lsb, s1 = 10 * p1 + lsb, s2 = 10 * p2 + lsb;
            const uint32_t* p = (const uint32_t*)row + xfirst[x];
            for (int t = 0; t < n; ++t) {
                const uint32_t q = p[t];
                const float wt = w[t];
                a0 = __builtin_fmaf(wt, (float)((q >> s0) & 0x3ffu) * 64.0f, a0);
                a1 = __builtin_fmaf(wt, (float)((q >> s1) & 0x3ffu) * 64.0f, a1);
                a2 = __builtin_fmaf(wt, (float)((q >> s2) & 0x3ffu) * 64.0f, a2);
            }
        } else if (d.uv16) {
            typedef typename std::conditional<sizeof(T) == 2, uint64_t, uint32_t>::type Q;   // one pixel of four samples
            const int s0 = 8 * (int)sizeof(T) * p0, s1 = 8 * (int)sizeof(T) * p1, s2 = 8 * (int)sizeof(T) * p2;
            const Q* p = (const Q*)row + xfirst[x];
            for (int t = 0; t < n; ++t) {
                const Q q = p[t];
                const float wt = w[t];
                a0 = __builtin_fmaf(wt, (float)(T)(q >> s0), a0);
                a1 = __builtin_fmaf(wt, (float)(T)(q >> s1), a1);
                a2 = __builtin_fmaf(wt, (float)(T)(q >> s2), a2);
            }
        } else {
            const int ns = (d.layout & 64) ? 4 : 3;   // samples per pixel
            const T* p = (const T*)row + (size_t)ns * xfirst[x];
            for (int t = 0; t < n; ++t) {
                const float wt = w[t];
                a0 = __builtin_fmaf(wt, (float)p[ns * t + p0], a0);
                a1 = __builtin_fmaf(wt, (float)p[ns * t + p1], a1);
                a2 = __builtin_fmaf(wt, (float)p[ns * t + p2], a2);
            }
        }
        float* l = lds + (size_t)e * 3;
        l[0] = a0; l[1] = a1; l[2] = a2;
    }
    barrier();

    // vertical pass out of LDS, the matrix (YUV layouts) or the samples as they are (RGB layouts), three bytes per pixel
    const bool yuv = d.layout & 128;
    for (int e = tid; e < (r1 - r0) * cols; e += 256) {
        const int rl = e / cols, xl = e - rl * cols, r = r0 + rl;
        const int n = ycount[r];
        const float* w = yw + (size_t)r * d.ys;
        const float* col = lds + ((size_t)(yfirst[r] - ylo) * cols + xl) * 3;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int t = 0; t < n; ++t) {
            const float* q = col + (size_t)t * cols * 3;
            const float wt = w[t];
            a0 = __builtin_fmaf(wt, q[0], a0);
            a1 = __builtin_fmaf(wt, q[1], a1);
            a2 = __builtin_fmaf(wt, q[2], a2);
        }
        uint8_t* o = out + (((size_t)f * S + r) * S + c0 + xl) * 3;
        if (yuv) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float c = __builtin_fmaf(mat.m[4 * k], a0, __builtin_fmaf(mat.m[4 * k + 1], a1, __builtin_fmaf(mat.m[4 * k + 2], a2, mat.m[4 * k + 3])));
                o[k] = (uint8_t)nv12_byte(c);
            }
        } else {
            o[0] = (uint8_t)nv12_byte(a0);
            o[1] = (uint8_t)nv12_byte(a1);
            o[2] = (uint8_t)nv12_byte(a2);
        }
    }
}

#ifndef VH_HOST_CHECK   // tools/yuv_host_check.hip takes the planner and the body above and no device code
template <bool PLANAR, class T>
__global__ void __launch_bounds__(256)
resize_yuv_kernel(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ plan, uint8_t* __restrict__ out, int S, int max_tiles,
                  Nv12Matrix mat) {
    __shared__ __attribute__((aligned(16))) float lds[kResizeLdsFloats];
    resize_yuv_body<PLANAR, T>(frames, plan, out, S, max_tiles, mat, lds, (int)blockIdx.x, (int)threadIdx.x, [] { __syncthreads(); });
}

// the one launcher of the four instantiations; planar: three planes, not Y + interleaved UV.  wide: 16-bit samples
hipError_t launch_resize_yuv_any(bool planar, bool wide, const uint8_t* frames, const uint32_t* plan_dev, int batch, int S, int max_tiles,
                                 const float* m12, uint8_t* out, hipStream_t s) {
    if (!frames || !plan_dev || !out || !m12 || batch < 1 || S < 1 || max_tiles < 1 || (int64_t)batch * max_tiles > 0x7fffffffll)
        return hipErrorInvalidValue;
    Nv12Matrix mat;
    memcpy(mat.m, m12, sizeof mat.m);
    const dim3 grid((unsigned)(batch * max_tiles));
    if (planar && wide)
        hipLaunchKernelGGL((resize_yuv_kernel<true, uint16_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    else if (planar)
        hipLaunchKernelGGL((resize_yuv_kernel<true, uint8_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    else if (wide)
        hipLaunchKernelGGL((resize_yuv_kernel<false, uint16_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    else
        hipLaunchKernelGGL((resize_yuv_kernel<false, uint8_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    return hipGetLastError();
}

// packed 4:2:2: the same body behind a kernel of its own, so that the four instantiations above keep their names and their code
template <class T>
__global__ void __launch_bounds__(256)
resize_packed422_kernel(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ plan, uint8_t* __restrict__ out, int S, int max_tiles,
                        Nv12Matrix mat) {
    __shared__ __attribute__((aligned(16))) float lds[kResizeLdsFloats];
    resize_yuv_body<true, T, true>(frames, plan, out, S, max_tiles, mat, lds, (int)blockIdx.x, (int)threadIdx.x, [] { __syncthreads(); });
}

// wide: the 16-bit layouts (Y210 / Y216 and v210, told apart per frame by the record's layout); a plan of resize_plan_build_yuy2
hipError_t launch_resize_yuy2(bool wide, const uint8_t* frames, const uint32_t* plan_dev, int batch, int S, int max_tiles, const float* m12,
                              uint8_t* out, hipStream_t s) {
    if (!frames || !plan_dev || !out || !m12 || batch < 1 || S < 1 || max_tiles < 1 || (int64_t)batch * max_tiles > 0x7fffffffll)
        return hipErrorInvalidValue;
    Nv12Matrix mat;
    memcpy(mat.m, m12, sizeof mat.m);
    const dim3 grid((unsigned)(batch * max_tiles));
    if (wide)
        hipLaunchKernelGGL((resize_packed422_kernel<uint16_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    else
        hipLaunchKernelGGL((resize_packed422_kernel<uint8_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    return hipGetLastError();
}

// packed 4:4:4: a body and a kernel of its own; the six kernels above keep their names and their code
template <class T>
__global__ void __launch_bounds__(256)
resize_packed444_kernel(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ plan, uint8_t* __restrict__ out, int S, int max_tiles,
                        Nv12Matrix mat) {
    __shared__ __attribute__((aligned(16))) float lds[kResizeLdsFloats];
    resize_packed444_body<T>(frames, plan, out, S, max_tiles, mat, lds, (int)blockIdx.x, (int)threadIdx.x, [] { __syncthreads(); });
}

// wide: the 16-bit layouts (Y416 / AYUV64 and Y410 / V410, told apart per frame by the record's layout); a plan of resize_plan_build_bgra
hipError_t launch_resize_bgra(bool wide, const uint8_t* frames, const uint32_t* plan_dev, int batch, int S, int max_tiles, const float* m12,
                              uint8_t* out, hipStream_t s) {
    if (!frames || !plan_dev || !out || !m12 || batch < 1 || S < 1 || max_tiles < 1 || (int64_t)batch * max_tiles > 0x7fffffffll)
        return hipErrorInvalidValue;
    Nv12Matrix mat;
    memcpy(mat.m, m12, sizeof mat.m);
    const dim3 grid((unsigned)(batch * max_tiles));
    if (wide)
        hipLaunchKernelGGL((resize_packed444_kernel<uint16_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    else
        hipLaunchKernelGGL((resize_packed444_kernel<uint8_t>), grid, dim3(256), 0, s, frames, plan_dev, out, S, max_tiles, mat);
    return hipGetLastError();
}
#endif

// ---- host: the colour matrix -----------------------------------------------------------------------------------------------
// Every expression is written as include/vithip.h states it and evaluated in IEEE double with no contraction, so that a numpy
// float64 transcription gives, after the one rounding, the same fp32 entries.
#pragma clang fp contract(off)
// The matrix of 16-bit words: `bits` significant bits, in the high bits of the word (msb_aligned: P010 / P012 / P016) or the low
// ones (yuv4xxpNNle).
int yuv_matrix16(int standard, int full_range, int bits, int msb_aligned, float m[12]) {
    double kr, kb;
    switch (standard) {
        case VH_YUV_BT601: kr = 0.299; kb = 0.114; break;
        case VH_YUV_BT709: kr = 0.2126; kb = 0.0722; break;
        case VH_YUV_BT2020: kr = 0.2627; kb = 0.0593; break;
        default: return 1;
    }
    if (!m || (full_range != 0 && full_range != 1) || bits < 8 || bits > 16 || (msb_aligned != 0 && msb_aligned != 1)) return 1;
    const double kg = 1.0 - kr - kb;
    const double a = msb_aligned ? (double)(1 << (16 - bits)) : 1.0;   // word = code * a
    const double q = (double)(1 << (bits - 8));
    const double sy = full_range ? 255.0 / (((double)(1 << bits) - 1.0) * a) : 255.0 / (219.0 * q * a);
    const double sc = full_range ? sy : 255.0 / (224.0 * q * a);
    const double oy = full_range ? 0.0 : 16.0 * q * a;
    const double mid = (double)(1 << (bits - 1)) * a;
    const double rv = 2.0 * (1.0 - kr) * sc;
    const double bu = 2.0 * (1.0 - kb) * sc;
    const double gu = -(2.0 * kb * (1.0 - kb) / kg) * sc;
    const double gv = -(2.0 * kr * (1.0 - kr) / kg) * sc;
    const double yo = -(sy * oy);
    const double v[12] = {sy, 0.0, rv, yo - mid * rv,
                          sy, gu, gv, yo - mid * gu - mid * gv,
                          sy, bu, 0.0, yo - mid * bu};
    for (int i = 0; i < 12; ++i) m[i] = (float)v[i];
    return 0;
}

// The matrix of bytes is the one of 8-bit codes in the low bits of the word, bit for bit: every factor yuv_matrix16 adds (a, q) is
// then exactly 1, mid is exactly 128 and 2^8 - 1 is exactly 255, so each double expression has the value it had without them.
int yuv_matrix(int standard, int full_range, float m[12]) { return yuv_matrix16(standard, full_range, 8, 0, m); }

}  // namespace vh
