// vithip_api.hip — the C ABI of libvithip.so (declared in include/vithip.h).
//
// Host-side runtime of the hot path: device/stream ownership, the HBM layout (canonical fp32
// weight blob + 16-bit compute copies + one activation arena sized for max_batch), weight
// preparation, and the launch sequence of one ViT forward.  Takes over the jobs of the
// reference's _init_program/_init_kernel/_load_params/launch_forward/cleanup
// (/root/reference/src/netFPGA.cpp:239-290, 367-515, 639-651) — see the per-function notes in
// the header.  No CPU fallback exists: without a gfx950 device every compute entry point
// fails with VH_ERR_NO_DEVICE / VH_ERR_HIP.
#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "vh_kernels.h"

using namespace vh;

namespace {

thread_local std::string g_err;

int fail(std::string* ctx_err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    if (ctx_err) *ctx_err = buf;
    return code;
}

#define HIPCHK(ctxerr, expr)                                                                   \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctxerr, VH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

struct BlobHeader {
    char magic[8];
    int32_t image_size, patch_size, channels, dim, heads, mlp_dim, layers, classes;
    float ln_eps;
    // on-disk files only (vh_save_weights_file): FNV-1a 64 of the parameter bytes, flags bit 0 = checksum present.
    // Blobs built in memory leave the two checksum words, bit 0 and the padding 0.  flags bits 1 and 2 describe the MODEL, in
    // memory and on disk alike: bit 1 = pre-LayerNorm (VH_FLAG_PRE_LN: two more tensors), bit 2 = QuickGELU (VH_FLAG_QUICK_GELU),
    // bits 9 .. 13 = the number of register tokens (VH_FLAG_REGISTERS: the tensor reg), in the bits vh_config.flags keeps it in;
    // bit 15 = no class token (VH_FLAG_NO_CLS), bits 16 .. 17 = the pooling mode (VH_FLAG_POOL), bit 19 = the attention-pooling head
    // (VH_FLAG_MAP_HEAD: eleven more tensors), bit 21 = tanh GELU (VH_FLAG_TANH_GELU), bit 23 = rotary position embedding (VH_FLAG_ROPE: two
    // more tensors, at the very end), bit 25 = SwiGLU MLP (VH_FLAG_SWIGLU: fc1 of every layer is [2 M][D] + [2 M]), likewise.
    uint32_t sum_lo, sum_hi, flags, pad[2];
};
static_assert(sizeof(BlobHeader) == 64, "blob header is 64 bytes");
constexpr uint32_t kBlobSum = 1, kBlobPreLn = 2, kBlobQuickGelu = 4, kBlobRegisters = VH_FLAG_REGISTERS_MASK,
                   kBlobNoCls = VH_FLAG_NO_CLS, kBlobPool = VH_FLAG_POOL_MASK, kBlobMapHead = VH_FLAG_MAP_HEAD, kBlobTanhGelu = VH_FLAG_TANH_GELU, kBlobRope = VH_FLAG_ROPE, kBlobSwiglu = VH_FLAG_SWIGLU,
                   kBlobSameBits = kBlobRegisters | kBlobNoCls | kBlobPool | kBlobMapHead | kBlobTanhGelu | kBlobRope | kBlobSwiglu,   // at their vh_config.flags positions
                   kBlobModelBits = kBlobPreLn | kBlobQuickGelu | kBlobSameBits;
uint32_t blob_model_bits(const vh_config& c) {
    return ((c.flags & VH_FLAG_PRE_LN) ? kBlobPreLn : 0u) | ((c.flags & VH_FLAG_QUICK_GELU) ? kBlobQuickGelu : 0u) |
           ((uint32_t)c.flags & kBlobSameBits);
}
// the model flags of a header's flags word (vh_blob_file_config)
int32_t blob_model_flags(uint32_t bits) {
    return ((bits & kBlobPreLn) ? VH_FLAG_PRE_LN : 0) | ((bits & kBlobQuickGelu) ? VH_FLAG_QUICK_GELU : 0) | (int32_t)(bits & kBlobSameBits);
}

uint64_t fnv1a64(const void* data, size_t n, uint64_t h = 0xCBF29CE484222325ull) {
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}

struct LayerOff {  // offsets in floats from the start of the parameter region
    size_t ln1w, ln1b, qw, qb, kw, kb, vw, vb, ow, ob, ln2w, ln2b, f1w, f1b, f2w, f2b;
};

struct Layout {
    int T, NP, KP;   // KP = patch^2 * channels: the patch vector in the blob
    int R = 0, lead = 1;   // VH_FLAG_REGISTERS: register tokens; lead = 1 + R rows in front of an image's patch rows, T = NP + lead
    // VH_FLAG_NO_CLS: no class-token row (ncls = 0: lead = R, no tensor cls, pos [NP][D]); VH_FLAG_POOL: the head's input and its
    // width HW (D; 2 D for VH_POOL_CLS_AVG: headw [C][HW])
    int ncls = 1, pool = VH_POOL_CLS, HW = 0;
    int KPA;         // KP rounded up to 64: the compute width of the 16-bit patch operands (wp16, col16, the patch GEMM's K)
    size_t patch_w, patch_b, cls, pos, lnfw, lnfb, headw, headb, total;
    size_t reg = 0;              // VH_FLAG_REGISTERS: reg [R][D], directly after pos ([(NP + 1)][D]: registers carry no position row)
    size_t prew = 0, preb = 0;   // VH_FLAG_PRE_LN: pre_ln.weight / pre_ln.bias [D], directly after pos / reg
    // VH_FLAG_MAP_HEAD: the attention-pooling head's tensors, directly after head.bias (vithip.h): qk [H][D], v / o [D][D] + [D], the
    // block's LayerNorm, fc1 [M][D] + [M], fc2 [D][M] + [D]
    bool map = false;
    size_t map_qk = 0, map_vw = 0, map_vb = 0, map_ow = 0, map_ob = 0, map_lnw = 0, map_lnb = 0, map_f1w = 0, map_f1b = 0, map_f2w = 0, map_f2b = 0;
    // VH_FLAG_ROPE: rope.cos / rope.sin [NP][hd / 2], the last two tensors of the blob (vithip.h)
    bool rope = false;
    size_t rope_cos = 0, rope_sin = 0;
    // VH_FLAG_SWIGLU: fc1 of every layer is [M1][D] + [M1] with M1 = 2 M (gate rows, then value rows); M1 = M otherwise
    bool swiglu = false;
    int M1 = 0;
    std::vector<LayerOff> layer;
};

Layout make_layout(const vh_config& c) {
    Layout L;
    const size_t D = c.dim, M = c.mlp_dim, C = c.classes;
    const int g = c.image_size / c.patch_size;
    L.NP = g * g;
    L.R = VH_FLAG_REGISTERS_OF(c.flags);
    L.ncls = (c.flags & VH_FLAG_NO_CLS) ? 0 : 1;
    L.pool = VH_FLAG_POOL_OF(c.flags);
    L.HW = L.pool == VH_POOL_CLS_AVG ? 2 * c.dim : c.dim;
    L.lead = L.ncls + L.R;
    L.T = L.NP + L.lead;
    L.swiglu = (c.flags & VH_FLAG_SWIGLU) != 0;
    L.M1 = L.swiglu ? 2 * c.mlp_dim : c.mlp_dim;
    const size_t M1 = (size_t)L.M1;
    L.KP = c.patch_size * c.patch_size * c.channels;
    L.KPA = (L.KP + 63) / 64 * 64;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += n; return r; };
    L.patch_w = take(D * L.KP); L.patch_b = take(D); L.cls = L.ncls ? take(D) : 0; L.pos = take((size_t)(L.NP + L.ncls) * D);
    if (L.R) L.reg = take((size_t)L.R * D);
    if (c.flags & VH_FLAG_PRE_LN) { L.prew = take(D); L.preb = take(D); }
    L.layer.resize(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        LayerOff& p = L.layer[l];
        p.ln1w = take(D); p.ln1b = take(D);
        p.qw = take(D * D); p.qb = take(D); p.kw = take(D * D); p.kb = take(D);
        p.vw = take(D * D); p.vb = take(D); p.ow = take(D * D); p.ob = take(D);
        p.ln2w = take(D); p.ln2b = take(D);
        p.f1w = take(M1 * D); p.f1b = take(M1); p.f2w = take(D * M); p.f2b = take(D);
    }
    L.lnfw = take(D); L.lnfb = take(D); L.headw = take(C * (size_t)L.HW); L.headb = take(C);
    L.map = (c.flags & VH_FLAG_MAP_HEAD) != 0;
    if (L.map) {
        L.map_qk = take((size_t)c.heads * D); L.map_vw = take(D * D); L.map_vb = take(D); L.map_ow = take(D * D); L.map_ob = take(D);
        L.map_lnw = take(D); L.map_lnb = take(D); L.map_f1w = take(M * D); L.map_f1b = take(M); L.map_f2w = take(D * M); L.map_f2b = take(D);
    }
    L.rope = (c.flags & VH_FLAG_ROPE) != 0;
    if (L.rope) { const size_t n = (size_t)L.NP * (size_t)(c.dim / c.heads / 2); L.rope_cos = take(n); L.rope_sin = take(n); }
    L.total = o;
    return L;
}

// expected blob size of a configuration computed WITHOUT building the layout (no allocation): used on untrusted headers
size_t blob_bytes_of(const vh_config& c) {
    const size_t D = c.dim, M = c.mlp_dim, C = c.classes, g = (size_t)(c.image_size / c.patch_size);
    const size_t ncls = (c.flags & VH_FLAG_NO_CLS) ? 0 : 1, HW = VH_FLAG_POOL_OF(c.flags) == VH_POOL_CLS_AVG ? 2 * D : D;
    const size_t T = g * g + ncls + (size_t)VH_FLAG_REGISTERS_OF(c.flags), KP = (size_t)c.patch_size * c.patch_size * c.channels;   // (pos rows + reg rows)
    const size_t M1 = (c.flags & VH_FLAG_SWIGLU) ? 2 * M : M;   // fc1's width (VH_FLAG_SWIGLU: gate and value rows)
    const size_t per_layer = 2 * D + 4 * (D * D + D) + 2 * D + (M1 * D + M1) + (D * M + D);
    const size_t pre_ln = (c.flags & VH_FLAG_PRE_LN) ? 2 * D : 0;
    const size_t map = (c.flags & VH_FLAG_MAP_HEAD) ? (size_t)c.heads * D + 2 * (D * D + D) + 2 * D + (M * D + M) + (D * M + D) : 0;
    const size_t rope = (c.flags & VH_FLAG_ROPE) ? 2 * g * g * (D / (size_t)c.heads / 2) : 0;
    return sizeof(BlobHeader) + 4 * (D * KP + D + ncls * D + T * D + pre_ln + (size_t)c.layers * per_layer + 2 * D + C * HW + C + map + rope);
}

const char* check_config(const vh_config& c) {
    if (c.image_size <= 0 || c.patch_size <= 0 || c.image_size % c.patch_size) return "image_size must be a positive multiple of patch_size";
    if (c.channels <= 0) return "channels must be positive";
    if (c.dim <= 0 || c.dim % 64) return "dim must be a multiple of 64";
    if (c.heads <= 0 || c.dim % c.heads) return "dim must be a multiple of heads";
    if (!attention_hd_supported(c.dim / c.heads)) return "head dim (dim/heads) must be 32, 48, 64, 80, 96, 112 or 128";
    if (c.mlp_dim <= 0 || c.mlp_dim % 64) return "mlp_dim must be a multiple of 64";
    if (c.dim > 2048) return "dim > 2048 unsupported";
    if (c.layers <= 0) return "layers must be positive";
    if (c.classes <= 0 || c.classes % 4) return "classes must be a positive multiple of 4";
    if (c.dtype != VH_DTYPE_BF16 && c.dtype != VH_DTYPE_FP16 && c.dtype != VH_DTYPE_FP8) return "dtype must be VH_DTYPE_BF16, VH_DTYPE_FP16 or VH_DTYPE_FP8";
    if (c.dtype == VH_DTYPE_FP8 && (c.dim % 128 || c.mlp_dim % 128)) return "VH_DTYPE_FP8 needs dim and mlp_dim to be multiples of 128";
    if (c.max_batch <= 0) return "max_batch must be positive";
    if (!(c.ln_eps > 0.f)) return "ln_eps must be positive";
    if (c.flags & ~(VH_FLAG_LN_FOLD_OFF | VH_FLAG_LN_FOLD_ON | VH_FLAG_W8_E4M3 | VH_FLAG_CLS_TAIL | VH_FLAG_PRE_LN | VH_FLAG_QUICK_GELU | VH_FLAG_REGISTERS_MASK |
                    VH_FLAG_NO_CLS | VH_FLAG_POOL_MASK | VH_FLAG_MAP_HEAD | VH_FLAG_TANH_GELU | VH_FLAG_ROPE | VH_FLAG_SWIGLU)) return "unknown bits in flags";
    if (c.flags & VH_FLAG_SWIGLU) {
        if (c.flags & (VH_FLAG_QUICK_GELU | VH_FLAG_TANH_GELU)) return "flags: VH_FLAG_SWIGLU excludes VH_FLAG_QUICK_GELU and VH_FLAG_TANH_GELU (one MLP activation)";
        if (c.flags & VH_FLAG_MAP_HEAD) return "flags: VH_FLAG_SWIGLU excludes VH_FLAG_MAP_HEAD (the head's own MLP block is not gated)";
        if (c.flags & VH_FLAG_CLS_TAIL) return "flags: VH_FLAG_SWIGLU excludes VH_FLAG_CLS_TAIL (the tail's class-row MLP has no gate pass)";
        if (c.flags & VH_FLAG_W8_E4M3) return "flags: VH_FLAG_SWIGLU excludes VH_FLAG_W8_E4M3 (fc1's e4m3 scales are mlp_dim wide)";
        if (c.dtype == VH_DTYPE_FP8) return "flags: VH_FLAG_SWIGLU excludes VH_DTYPE_FP8 (an e4m3 gated h has no rounding contract yet)";
    }
    if ((c.flags & VH_FLAG_ROPE) && (c.flags & VH_FLAG_CLS_TAIL)) return "flags: VH_FLAG_ROPE excludes VH_FLAG_CLS_TAIL (the tail's one-query attention kernel reads unrotated q and k)";
    if ((c.flags & VH_FLAG_TANH_GELU) && (c.flags & VH_FLAG_QUICK_GELU)) return "flags: VH_FLAG_TANH_GELU and VH_FLAG_QUICK_GELU exclude each other (one MLP activation)";
    if (c.flags & VH_FLAG_MAP_HEAD) {   // (in front of the VH_FLAG_NO_CLS rules: NO_CLS + POOL_CLS is this head's own combination)
        if (!(c.flags & VH_FLAG_NO_CLS)) return "flags: VH_FLAG_MAP_HEAD needs VH_FLAG_NO_CLS (the head pools the patch rows; its towers have no class token)";
        if (VH_FLAG_POOL_OF(c.flags)) return "flags: VH_FLAG_MAP_HEAD excludes VH_FLAG_POOL (the attention pooling is the head's input)";
        if (VH_FLAG_REGISTERS_OF(c.flags)) return "flags: VH_FLAG_MAP_HEAD excludes VH_FLAG_REGISTERS";
        if (c.flags & VH_FLAG_CLS_TAIL) return "flags: VH_FLAG_MAP_HEAD excludes VH_FLAG_CLS_TAIL (there is no class token)";
        if (c.heads > VH_MAP_MAX_HEADS) return "flags: VH_FLAG_MAP_HEAD takes at most 16 heads";
    }
    const int R = VH_FLAG_REGISTERS_OF(c.flags);
    if (R > VH_MAX_REGISTERS) return "flags: VH_FLAG_REGISTERS takes 0 .. 16 register tokens";
    const int ncls = (c.flags & VH_FLAG_NO_CLS) ? 0 : 1, pool = VH_FLAG_POOL_OF(c.flags);
    if (!ncls && !(c.flags & VH_FLAG_MAP_HEAD) && (pool == VH_POOL_CLS || pool == VH_POOL_CLS_AVG))
        return pool == VH_POOL_CLS ? "flags: VH_FLAG_NO_CLS needs VH_FLAG_POOL(VH_POOL_AVG_NORM) or VH_FLAG_POOL(VH_POOL_AVG_FCNORM): VH_POOL_CLS reads the class token"
                                   : "flags: VH_FLAG_NO_CLS excludes VH_POOL_CLS_AVG: its first half is the class token";
    if ((c.flags & VH_FLAG_CLS_TAIL) && !ncls) return "flags: VH_FLAG_CLS_TAIL excludes VH_FLAG_NO_CLS (its last layer computes the class-token rows only)";
    if ((c.flags & VH_FLAG_CLS_TAIL) && pool != VH_POOL_CLS) return "flags: VH_FLAG_CLS_TAIL excludes VH_FLAG_POOL (its last layer does not update the patch rows)";
    if ((c.flags & VH_FLAG_W8_E4M3) && c.dtype == VH_DTYPE_FP8) return "flags: VH_FLAG_W8_E4M3 is for the 16-bit dtypes (VH_DTYPE_FP8 quantises both operands)";
    if ((c.flags & VH_FLAG_W8_E4M3) && (c.dim % 4 || c.mlp_dim % 4)) return "flags: VH_FLAG_W8_E4M3 needs dim and mlp_dim multiples of 4";
    if ((c.flags & VH_FLAG_LN_FOLD_OFF) && (c.flags & VH_FLAG_LN_FOLD_ON)) return "flags: VH_FLAG_LN_FOLD_OFF and VH_FLAG_LN_FOLD_ON exclude each other";
    // bounds that keep every size computation below far from overflow (and a crafted file header from driving an
    // allocation: vh_blob_file_config feeds this function)
    if (c.image_size > 4096 || c.patch_size > 256 || c.channels > 64) return "image_size <= 4096, patch_size <= 256, channels <= 64";
    if (c.layers > 4096 || c.classes > (1 << 20) || c.mlp_dim > (1 << 16) || c.max_batch > (1 << 20)) return "layers <= 4096, classes <= 2^20, mlp_dim <= 2^16, max_batch <= 2^20";
    // tokens: up to 64 x 64 patches + the class token (the K/V-streaming attention's range); rows: at most 640 x 2^20, the
    // largest row count (max_batch x tokens) any model reached while the attention was bounded at 640 tokens
    const int g = c.image_size / c.patch_size;
    if (g > 64) return "tokens <= 4097 (image_size / patch_size <= 64)";
    if (g * g + ncls + R > 4097)
        return ncls ? "tokens <= 4097: a 64 x 64 patch grid + the class token leaves no room for register tokens"
                    : "tokens <= 4097: a 64 x 64 patch grid without a class token leaves room for one register token";
    if ((int64_t)c.max_batch * (g * g + ncls + R) > (640ll << 20)) return "max_batch x tokens <= 640 x 2^20";
    return nullptr;
}

enum Stage { ST_IM2COL, ST_PATCH, ST_CLS, ST_LN, ST_QKV, ST_ATTN, ST_PROJ, ST_FC1, ST_FC2, ST_LNF, ST_HEAD, ST_LNSTATS, ST_PRELN, ST_RESIZE, ST_COUNT };
// ST_RESIZE is no stage of enqueue_forward: the frames entry points launch it in front of the forward.  vh_profile_forward (an
// fp32 forward) keeps reporting the kProfiledStages stages before it, in the slot layout its callers were built against.
constexpr int kProfiledStages = ST_RESIZE;
const char* kStageNames[ST_COUNT] = {"im2col", "patch_gemm", "cls_rows", "layernorm", "qkv_gemm", "attention",
                                     "proj_gemm", "fc1_gemm", "fc2_gemm", "final_layernorm", "head_gemm", "ln_stats", "pre_layernorm", "resize"};

}  // namespace

// The images of one forward: a dense tensor of one element type (VH_ELEM_*: floats the caller has normalised, or 8-bit pixels
// that the gather normalises) in one layout (VH_LAYOUT_*).  Only the im2col call site of enqueue_forward looks at the kind.
struct ImgIn {
    const void* p;
    int kind = VH_ELEM_F32;      // VH_ELEM_*
    int layout = VH_LAYOUT_NHWC; // VH_LAYOUT_*
    bool u8() const { return kind == VH_ELEM_U8; }
    bool nhwc_f32() const { return kind == VH_ELEM_F32 && layout == VH_LAYOUT_NHWC; }
    size_t elem() const { return kind == VH_ELEM_F32 ? 4 : kind == VH_ELEM_U8 ? 1 : 2; }
    // the same kind of tensor `elements` further on: a whole number of images (the batch split), hence right for both layouts
    ImgIn skip(size_t elements) const { return ImgIn{(const char*)p + elements * elem(), kind, layout}; }
    bool operator==(const ImgIn& o) const { return p == o.p && kind == o.kind && layout == o.layout; }
};
constexpr int kU8 = VH_ELEM_U8;   // ImgIn{p, kU8}: NHWC bytes, the 8-bit entry points and the resized frames

// The buffers ONE forward in flight owns: enqueue_forward takes its part's slices of one set.  A context has two sets and two
// compute streams, so that two forwards that do not depend on each other -- consecutive steps of vh_forward_device_async,
// consecutive submits of an image ring -- share the chip: the partly filled last round of tiles of one forward's GEMM runs
// beside the other forward's kernels (DESIGN.md section 7 "Two forwards in flight").  Set 0 lives in the arena; set 1 is its
// own allocation, made the first time it is needed (second_set).  Shared by both: the weights (LayerW), guard_dev (an
// atomic max, order-free), in_dev, logits_dev, the feature and attention stores.
struct ActSet {
    char* base = nullptr;     // set 1: its allocation (set 0: null, the arena owns the bytes)
    unsigned int* tickets = nullptr;   // [max_batch][layers] work-queue counters of the attention kernel (launch_attention)
    float* x = nullptr;       // residual stream [B*T, D] fp32
    void* xn16 = nullptr;     // LN output       [B*T, D]
    void* xlo16 = nullptr;    // [B*T, D] bytes: the split residual's lo plane
    void* qkv16 = nullptr;    //                 [B*T, 3D]
    void* att16 = nullptr;    //                 [B*T, D]
    void* h16 = nullptr;      //                 [B*T, M]
    void* gu16 = nullptr;     // VH_FLAG_SWIGLU contexts only: fc1's output [B*T, 2 M] (gate | value), the gate pass's input
    void* col16 = nullptr;    // patch matrix    [B*NP, KPA]
    float* clsn32 = nullptr;  // the head's input [B, W] fp32: the final-LN'd CLS rows (W = D), or what the VH_FLAG_POOL mode computes (W = L.HW)
    float* pool32 = nullptr;  // [B, D] fp32 scratch of the pooled modes: CLS_AVG's LN'd class rows, AVG_FCNORM's raw mean
    float* stats = nullptr;   // [B*T][2] (mean, rstd) of the current residual rows
    float* partials = nullptr;// [D/64][B*T][2]
    // VH_FLAG_MAP_HEAD contexts only: z [B][H][D] (the kernel's weighted sums; reused as [B][D] scratch behind the V product), the
    // block's hidden rows [B][M], and [2][B][D]: a (the V product), then o (the out-projection) of every image
    float *mapz32 = nullptr, *maph32 = nullptr, *mapa32 = nullptr;
};

// One layer's compute weights: pointers into the w16 arena, built once by vh_create.  prepare_weights fills what they point to, the
// layer loops read it.
struct LayerW {
    void *qkv = nullptr, *o = nullptr, *fc1 = nullptr, *fc2 = nullptr;   // the GEMMs' weight operands: 16-bit, or e4m3 bytes (VH_DTYPE_FP8)
    // fc2's weights once more in the 16-row-blocked layout of the tiled hidden activation (h_tiled; folded path): the MLP hidden
    // activation then leaves fc1's epilogue straight from the registers (gemm_epilogue.h OTILED) and fc2's operand DMA reads both
    // operands in that layout -- same values, same k order, same bits as the row-major path.  The out-projection's likewise:
    // attention writes its output tiled as well (att_tiled).  Null where the shape or VH_H_TILED=0 rules the layout out.
    void *fc2_t = nullptr, *o_t = nullptr;
    // VH_DTYPE_FP8: one fp32 scale per output channel of the four e4m3 matrices; null on 16-bit contexts
    float *s_qkv = nullptr, *s_o = nullptr, *s_fc1 = nullptr, *s_fc2 = nullptr;
    float* bqkv = nullptr;   // [3 D]: the plain path's q|k|v bias (q's part scaled like Wq)
    // LayerNorm fold constants: c = row sums of W', d = beta.W + b, for q|k|v [3 D] and fc1 [M1] (M1 = fc1's width: M, or 2 M with VH_FLAG_SWIGLU)
    float *c_qkv = nullptr, *d_qkv = nullptr, *c_fc1 = nullptr, *d_fc1 = nullptr;
};

// The residual stream's rows where a forward left them, in one of three forms: fp32 rows in hi (VH_FEAT_FORM_F32, lo null); a 16-bit
// hi plane plus one scaled e4m3 byte per element (VH_DTYPE_BF16 / VH_DTYPE_FP16: vh_common.h Lo8); on fp8 contexts an e4m3 hi plane
// -- the GEMM operand itself -- plus a bf16 lo plane (VH_DTYPE_FP8).  The planes hold 3 bytes per element either way.
struct ResidView { const void* hi; const void* lo; int form; };
static size_t hi_bytes(int form) { return form == VH_FEAT_FORM_F32 ? 4 : form == VH_DTYPE_FP8 ? 1 : 2; }
static size_t lo_bytes(int form) { return form == VH_FEAT_FORM_F32 ? 0 : form == VH_DTYPE_FP8 ? 2 : 1; }

struct vh_ctx {
    vh_config cfg;
    int device;
    Layout L;
    hipStream_t stream = nullptr;
    // optional extra streams: the batch is split into `nstreams` contiguous parts that run concurrently
    static constexpr int kMaxStreams = 4;
    hipStream_t xstream[kMaxStreams - 1] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kMaxStreams - 1] = {nullptr, nullptr, nullptr};
    int nstreams = 1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool weights_ready = false;
    int run_layers = -1;
    // HBM: canonical blob (header + fp32 params) and the 16-bit compute copies
    char* blob = nullptr;
    float* params = nullptr;  // blob + 64
    char* w16 = nullptr;      // arena of 16-bit matrices
    void* wp16 = nullptr;     // [D, KPA]
    std::vector<LayerW> layer;   // the per-layer matrices, scales and constants in the arena
    bool h_tiled = false;     // VH_H_TILED=0 (read when the context is created) keeps the row-major h (A/B, tests)
    bool att_tiled = true;    // VH_ATT_TILED=0 (read when the context is created) keeps the attention output row-major
    bool qkv_hm = true;       // VH_QKV_HM=0 keeps q|k|v row-major ([rows][3 D]) instead of head-major ([3][heads][rows][64]; needs att_tiled)
    bool swiglu_skip = false; // VH_SWIGLU_SKIP=1 (measurement only, tools/swiglu_bench.py): a VH_FLAG_SWIGLU context leaves the gate pass out
    bool weights_ready_tiled = false;   // the tiled copies exist for the CURRENT weights (prepared with the fold on)
    // VH_DTYPE_FP8: the four per-layer matrices hold e4m3 bytes (in the same arena) + one fp32 scale per output channel;
    // everything 16-bit (patch embedding, qkv, head) is bf16
    bool fp8 = false;
    int dt16 = VH_DTYPE_BF16;
    // LayerNorm folded into the q|k|v and fc1 GEMMs (dim and mlp_dim multiples of 256):
    bool ln_fold = false;
    // with the fold: the residual stream lives as two planes, x = hi + lo (ResidView: hi = the xn16 buffer = the GEMMs' A operand,
    // lo = xlo16 = what that rounding dropped): a residual GEMM then moves 3 B per element each way instead of the fp32 array plus
    // its 16-bit copy.  VH_RESID_SPLIT=0 (A/B tools) keeps the fp32 array.
    bool split = false;
    bool cls_tail = false;    // VH_FLAG_CLS_TAIL: the last layer computes the class-token rows only (folded 16-bit path, head dim 64)
    int head_dim = 64;        // dim / heads: 64 takes launch_attention and its layouts, any other launch_attention_hd (row-major)
    float q_scale = kAttnQScale;   // head_dim^-1/2 * log2(e), folded into Wq and bq (attention_q_scale)
    // Run-time guard on the fold: the kernels that produce the row statistics keep a running maximum of
    // |mean| * rstd over the REAL rows (guard_dev: the bits of a non-negative float); every forward ends with an
    // asynchronous copy of that word into pinned host memory, and every forward entry point looks at the copy before it
    // enqueues anything (no synchronisation: the value is the one of the most recently COMPLETED forward).  Beyond
    // guard_thresh the folded operand's rounding error leaves the budget of the 1e-3 tolerance; a context whose flags
    // left the choice to the library (guard_auto) then switches to the stand-alone LayerNorm for good -- the weights are
    // prepared again in the plain layout -- and the synchronous vh_forward repeats the forward that tripped it.
    bool ln_fold_cfg = false, split_cfg = false;   // what configuration + flags chose at creation (restored by a weight load)
    unsigned int* guard_dev = nullptr;
    float* guard_host = nullptr;
    float guard_thresh = 0.5f;
    bool guard_auto = false, guard_tripped = false;
    // activations (sized for max_batch): the arena holds set 0 and what both sets share
    char* arena = nullptr;
    ActSet act[2];
    size_t act_bytes = 0;          // the size of one set (bind_set)
    int last_set = 0;              // the set of the most recently enqueued forward: what the read-outs of "the last forward" read
    // two forwards in flight: the second compute stream, fork / join with c->stream, and per set the event behind its last head
    // launch (consecutive steps write the caller's logits in step order).  inflight_max: 2, or 1 with VH_INFLIGHT=1 (read when
    // the context is created, for A/B runs) or once the second set could not be allocated.  ring_flip: the set of the next
    // image-ring submit.  s2_open: stream2 holds ring forwards that c->stream has not joined (sync_compute)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork2 = nullptr, ev_join2 = nullptr, ev_head[2] = {nullptr, nullptr};
    int inflight_max = 2, ring_flip = 0;
    bool s2_open = false;
    float* in_dev = nullptr;  // staging for the host-pointer forward (fp32 images; vh_forward_u8 stages its bytes in the same buffer)
    // Input normalisation of the 8-bit entry points (vh_set_input_norm): pixel p of channel c enters the model as
    // fmaf((float)p, in_scale[c], in_shift[c]).  Passed to im2col_u8_kernel by value, so captured graphs hold a copy.
    float in_scale[kMaxChannels], in_shift[kMaxChannels];
    float* logits_dev = nullptr;
    // 8-bit frames (vh_forward_frames_u8, the frames ring; kernels_resize.hip).  All of it is allocated at the first frames call
    // and grown only when a call needs more than any before it: rz_u8 = the resized images [max_batch][S][S][C] the forward then
    // reads through ImgIn{rz_u8, u8}; rz_plan_dev = descriptors + tables in HBM (uploaded on the stream that runs the resize, so one
    // buffer serves every ring slot); rz_plan_host = their pinned staging for the synchronous entry points (a ring slot has its own);
    // rz_frames = device staging of vh_forward_frames_u8's host frames; rz_words = the host scratch the plan is built in.
    uint8_t* rz_u8 = nullptr;
    uint32_t *rz_plan_dev = nullptr, *rz_plan_host = nullptr;
    size_t rz_plan_dev_cap = 0, rz_plan_host_cap = 0;   // words
    uint8_t* rz_frames = nullptr;
    size_t rz_frames_cap = 0;
    std::vector<uint32_t> rz_words;
    // colour[0]: NV12 and planar YUV frames (vh_set_frame_colour): the 3 x 4 matrix and the chroma siting of both kinds of entry
    // points.  The matrix travels to resize_yuv_kernel by value at each launch, outside any captured graph.
    // colour[1]: 16-bit YUV frames (vh_set_frame_colour16): a second state, because one frames ring interleaves 8-bit and 16-bit submits
    struct FrameColour { float m[12]; int site = VH_CHROMA_LEFT; };
    FrameColour colour[2];
    int64_t last_us = 0;
    bool timed = false;
    int last_batch = 0;
    // Layer features (vh_set_feature_layers): the listed layers and ONE capture store, a slot of feat_slot bytes for every listed
    // layer below cfg.layers in list order.  A slot holds [max_batch * T][D] rows as the path keeps them (slot_view; sized once, at
    // the call).  What the LAST forward captured (enqueue_forward records it; the list call clears it): cap_n listed layers
    // cap_layers[], cap_nl = layers it ran, cap_form = the ResidView form of the rows it copied.
    int feat_layers[VH_MAX_FEATURE_LAYERS] = {0}, feat_n = 0;
    char* feat_store = nullptr;
    size_t feat_slot = 0;
    int cap_layers[VH_MAX_FEATURE_LAYERS] = {0}, cap_n = 0, cap_nl = -1, cap_form = VH_FEAT_FORM_F32;
    // Attention maps (vh_set_attention_layers): the listed layers, the query rows Q of the list (attn_q; attn_mode = VH_ATTN_Q_*) and
    // ONE store of fp32 probabilities, a slot of attn_slot bytes = [max_batch][heads][Q][T] per listed layer in list order.  What the
    // LAST forward captured (enqueue_forward records it; the list call clears it): acap_n listed layers acap_layers[], acap_nl = layers it ran.
    int attn_layers[VH_MAX_ATTENTION_LAYERS] = {0}, attn_n = 0, attn_q = 0, attn_mode = VH_ATTN_Q_CLS;
    char* attn_store = nullptr;
    size_t attn_slot = 0;
    int acap_layers[VH_MAX_ATTENTION_LAYERS] = {0}, acap_n = 0, acap_nl = -1;
    // pipelined host path (vh_ring_*): slots of pinned host staging + device buffers, copies on their own streams
    struct RingSlot {
        float *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;   // h_in / d_in hold bytes in a u8 ring
        hipEvent_t in_done = nullptr, fwd_done = nullptr, out_done = nullptr;
        int batch = 0;
        uint32_t* h_plan = nullptr;   // frames ring: pinned staging of the slot's descriptors + tables
        size_t plan_cap = 0;          // words
    };
    std::vector<RingSlot> ring;
    // what the slots stage: fp32 images, 8-bit images (a quarter of the pinned and device memory), or 8-bit frames of any size
    // (ring_slot_bytes each; resized on the context's stream in front of the forward)
    // or image tensors of one element type and layout (ring_elem, ring_layout; slots sized by the element type)
    enum RingKind { RING_F32, RING_U8, RING_FRAMES, RING_TENSOR };
    RingKind ring_kind = RING_F32;
    int ring_elem = VH_ELEM_F32, ring_layout = VH_LAYOUT_NHWC;   // what a slot holds: fixed by the kind, chosen for RING_TENSOR
    size_t ring_slot_bytes = 0;
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    int ring_batch = 0, ring_wr = 0, ring_rd = 0, ring_used = 0;
    bool last_h_tiled = false;   // debug tap 3
    bool last_qkv_hm = false;    // debug tap 4
    int num_cu = 256;
    // optional hipGraph replay of the forward's launch sequence (vh_set_graph): one instantiated graph per
    // (input pointer, input kind, logits pointer, batch); a batch size runs eagerly once before it is captured
    bool use_graph = false;
    struct GraphEntry { ImgIn in; float* out; int batch; hipGraph_t graph; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    std::vector<int> graph_warm;   // batch sizes that have run eagerly (kernel attributes are set)
    // optional per-launch timing of ONE stage inside the timed region (bench.py's roofline)
    int timing_stage = -1;
    std::vector<hipEvent_t> tev;  // pool: pairs (start, stop)
    size_t tev_used = 0;
    // optional per-STEP events of the last vh_forward_device_async call (vh_set_step_timing): K + 1 boundaries
    bool step_timing = false;
    std::vector<hipEvent_t> sev;
    size_t sev_used = 0;
    std::string err;
};

// filter_image pipeline: a ring of in-flight 8-bit frames (reference: 24 slots, netFPGA.cpp:47-56, 292-365)
struct vh_filter {
    int device, height, width, kind;
    struct Slot {
        uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
        hipEvent_t in_done = nullptr, k_done = nullptr, out_done = nullptr;
    };
    std::vector<Slot> slot;
    hipStream_t copy_in = nullptr, compute = nullptr, copy_out = nullptr;
    int wr = 0, rd = 0, used = 0;
    std::string err;
};

struct vh_mlp {
    int device, n_ins, n_layers, activation;
    std::vector<int> npl;
    size_t n_params = 0, n_neurons = 0;
    int widest = 0, max_vec = 0;
    hipStream_t stream = nullptr;
    float *params = nullptr, *bias = nullptr, *buf0 = nullptr, *buf1 = nullptr;
    bool loaded = false;
    int64_t last_us = 0;
    // training (vh_mlp_init_gradient / vh_mlp_launch_gradient): the sets and, per set and neuron, pre-activation,
    // activation and delta
    int n_sets = 0;
    float *set_ins = nullptr, *set_outs = nullptr, *tz = nullptr, *ta = nullptr, *td = nullptr, *terr = nullptr;
    int64_t last_gradient_us = 0;
    std::string err;
};

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- the buffers of an activation set: ONE table ------------------------------------------------------------------------------
// A row per ActSet member, in the arena's carve order.  Allocation and stride differ where a path stores
// narrower elements than the buffer is sized for (e4m3 operands on fp8 contexts, the one-byte lo plane on 16-bit ones); partials
// has one spare 64-column block, clsn32 room for the widest head input (2 D), mapa32 two [max_batch][D] arrays, a then o.
// PER_ROW: max_batch * T + 256 token rows, a part starts at row img0 * T.  The 256 are room for whole 256-row GEMM tiles behind the
// LAST part of a forward (enqueue_forward, rows_g): its rows start anywhere, so the padding may reach up to 255 rows past the last
// real row.  PER_IMAGE: max_batch images, a part starts at img0.
enum ActUnit { PER_ROW, PER_IMAGE };
template <class Row> void for_each_act_buffer(const vh_ctx* c, Row&& row) {
    const vh_config& f = c->cfg;
    const Layout& L = c->L;
    const size_t D = f.dim, M = f.mlp_dim, op = c->fp8 ? 1 : 2;   // op: bytes of a GEMM A-operand element
    const size_t tk = 4 * (size_t)(f.layers > 0 ? f.layers : 1);  // attention work-queue counters: one word per image and layer, a part uses its first image's
    //  member             counted in  allocated                     stride                        exists
    row(&ActSet::x,        PER_ROW,    D * 4,                        D * 4,                        true);
    row(&ActSet::xn16,     PER_ROW,    D * 2,                        D * op,                       true);
    row(&ActSet::qkv16,    PER_ROW,    3 * D * 2,                    3 * D * 2,                    true);
    row(&ActSet::att16,    PER_ROW,    D * 2,                        D * op,                       true);
    row(&ActSet::h16,      PER_ROW,    M * 2,                        M * op,                       true);
    row(&ActSet::col16,    PER_IMAGE,  L.NP * (size_t)L.KPA * 2,     L.NP * (size_t)L.KPA * 2,     true);
    row(&ActSet::clsn32,   PER_IMAGE,  2 * D * 4,                    (size_t)L.HW * 4,             true);
    row(&ActSet::pool32,   PER_IMAGE,  D * 4,                        D * 4,                        true);
    row(&ActSet::stats,    PER_ROW,    2 * 4,                        2 * 4,                        true);
    row(&ActSet::partials, PER_ROW,    (D / 64 + 1) * 2 * 4,         D / 64 * 2 * 4,               true);
    row(&ActSet::xlo16,    PER_ROW,    D * 2,                        D * (c->fp8 ? 2 : 1),         true);
    row(&ActSet::tickets,  PER_IMAGE,  tk,                           tk,                           true);
    row(&ActSet::mapz32,   PER_IMAGE,  (size_t)f.heads * D * 4,      (size_t)f.heads * D * 4,      L.map);
    row(&ActSet::maph32,   PER_IMAGE,  (M > D ? M : D) * 4,          (M > D ? M : D) * 4,          L.map);
    row(&ActSet::mapa32,   PER_IMAGE,  2 * D * 4,                    D * 4,                        L.map);
    row(&ActSet::gu16,     PER_ROW,    2 * M * 2,                    2 * M * 2,                    L.swiglu);
}
size_t act_units(const vh_ctx* c, ActUnit u) { return u == PER_ROW ? (size_t)c->cfg.max_batch * c->L.T + 256 : (size_t)c->cfg.max_batch; }
template <class T> void set_ptr(T*& dst, char* p) { dst = (T*)p; }
// a set's buffers at `base`, in table order, each on a 256-byte boundary; returns the set's size (a null: the size only)
size_t bind_set(const vh_ctx* c, ActSet* a, char* base) {
    size_t at = 0;
    for_each_act_buffer(c, [&](auto member, ActUnit u, size_t allocated, size_t, bool exists) {
        if (!exists) return;
        if (a) set_ptr(a->*member, base + at);
        at += align_up(act_units(c, u) * allocated, 256);
    });
    return at;
}
// the slices of `whole` that belong to the part of a forward that starts at image img0 (a buffer the context lacks stays null)
ActSet part_set(const vh_ctx* c, const ActSet& whole, int img0) {
    ActSet part;
    for_each_act_buffer(c, [&](auto member, ActUnit u, size_t, size_t stride, bool exists) {
        if (exists) set_ptr(part.*member, (char*)(whole.*member) + (size_t)img0 * (u == PER_ROW ? c->L.T : 1) * stride);
    });
    return part;
}
// allocated bytes of one buffer of a set, named by its member (members of other types cannot be it)
template <class T> size_t act_buffer_bytes(const vh_ctx* c, T* ActSet::*which) {
    size_t bytes = 0;
    for_each_act_buffer(c, [&](auto member, ActUnit u, size_t allocated, size_t, bool exists) {
        if constexpr (std::is_same_v<decltype(member), T * ActSet::*>)
            if (exists && member == which) bytes = act_units(c, u) * allocated;
    });
    return bytes;
}

// ---- the residual stream of a forward ----------------------------------------------------------------------------------------
int layers_to_run(const vh_ctx* c) { return (c->run_layers < 0 || c->run_layers > c->cfg.layers) ? c->cfg.layers : c->run_layers; }
// the form a forward over nl layers leaves the rows in on this context: the two planes from the first layer of the split path on
int resid_form(const vh_ctx* c, int nl) { return c->split && nl > 0 ? (c->fp8 ? VH_DTYPE_FP8 : c->dt16) : VH_FEAT_FORM_F32; }
// ... and where, in buffer set (or part) `a`
ResidView resid_view(const vh_ctx* c, const ActSet& a, int nl) {
    const int form = resid_form(c, nl);
    return form == VH_FEAT_FORM_F32 ? ResidView{a.x, nullptr, form} : ResidView{a.xn16, a.xlo16, form};
}
// slot `i` of the layer-feature capture store, holding rows of `form`: [max_batch * T][D] hi elements, the lo plane behind them
ResidView slot_view(const vh_ctx* c, int i, int form) {
    const char* const base = c->feat_store + (size_t)i * c->feat_slot;
    const size_t all = (size_t)c->cfg.max_batch * c->L.T * c->cfg.dim;
    return ResidView{base, lo_bytes(form) ? base + all * hi_bytes(form) : nullptr, form};
}

// records the next event of a grow-only pool on `s` (the stage-timing and step-timing events: created once, reused by every call)
int record_next(vh_ctx* c, std::vector<hipEvent_t>& pool, size_t& used, hipStream_t s) {
    if (used == pool.size()) {
        hipEvent_t e;
        HIPCHK(&c->err, hipEventCreate(&e));
        pool.push_back(e);
    }
    HIPCHK(&c->err, hipEventRecord(pool[used++], s));
    return VH_OK;
}

int set_device(std::string* err, int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(err, VH_ERR_NO_DEVICE, "no HIP device visible (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(err, VH_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    HIPCHK(err, hipSetDevice(device));
    return VH_OK;
}

// convert the fp32 blob resident in ctx->blob into the compute layout
int prepare_weights(vh_ctx* c) {
    const vh_config& f = c->cfg;
    const Layout& L = c->L;
    const int D = f.dim, M = f.mlp_dim, M1 = L.M1;   // M1: fc1's width (2 M on a VH_FLAG_SWIGLU context, which is never fp8 / W8)
    hipStream_t s = c->stream;
    const float* P = c->params;
    HIPCHK(&c->err, launch_permute_patch(P + L.patch_w, D, f.channels, f.patch_size, L.KPA, c->wp16, c->dt16, s));
    for (int l = 0; l < f.layers && c->fp8 && c->ln_fold; ++l) {
        // folded LayerNorm on e4m3 operands: W' = gamma o W through the row quantiser, its scales, c and d (launch_fold_ln_f8)
        const LayerOff& o = L.layer[l];
        const LayerW& w = c->layer[l];
        char* wq = (char*)w.qkv;
        const size_t dd = (size_t)D * D;
        HIPCHK(&c->err, launch_fold_ln_f8(P + o.qw, P + o.qb, P + o.ln1w, P + o.ln1b, D, D, c->q_scale, wq, w.s_qkv, w.c_qkv, w.d_qkv, s));
        HIPCHK(&c->err, launch_fold_ln_f8(P + o.kw, P + o.kb, P + o.ln1w, P + o.ln1b, D, D, 1.0f, wq + dd, w.s_qkv + D, w.c_qkv + D, w.d_qkv + D, s));
        HIPCHK(&c->err, launch_fold_ln_f8(P + o.vw, P + o.vb, P + o.ln1w, P + o.ln1b, D, D, 1.0f, wq + 2 * dd, w.s_qkv + 2 * D, w.c_qkv + 2 * D, w.d_qkv + 2 * D, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.ow, D, D, 1.0f, w.o, w.s_o, s));
        if (c->h_tiled && w.o_t) HIPCHK(&c->err, launch_tile_bytes(w.o, D, D, w.o_t, s));   // (att_tiled)
        HIPCHK(&c->err, launch_fold_ln_f8(P + o.f1w, P + o.f1b, P + o.ln2w, P + o.ln2b, M1, D, 1.0f, w.fc1, w.s_fc1, w.c_fc1, w.d_fc1, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.f2w, D, M, 1.0f, w.fc2, w.s_fc2, s));
        if (c->h_tiled && w.fc2_t) HIPCHK(&c->err, launch_tile_bytes(w.fc2, D, M, w.fc2_t, s));   // the same bytes, tiled (h_tiled)
    }
    for (int l = 0; l < f.layers && c->fp8 && !c->ln_fold; ++l) {
        const LayerOff& o = L.layer[l];
        const LayerW& w = c->layer[l];
        // bias [bq/8 ; bk ; bv] from the 16-bit packer (its 16-bit matrix is overwritten right after), then
        // e4m3 rows + scales; the softmax scale head_dim^-1/2 * log2(e) (q_scale) goes into the q rows' fp32 scales
        HIPCHK(&c->err, launch_pack_qkv(P + o.qw, P + o.qb, P + o.kw, P + o.kb, P + o.vw, P + o.vb, D, c->q_scale, w.qkv, w.bqkv, c->dt16, s));
        char* wq = (char*)w.qkv;
        const size_t dd = (size_t)D * D;
        HIPCHK(&c->err, launch_quantize_rows(P + o.qw, D, D, c->q_scale, wq, w.s_qkv, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.kw, D, D, 1.0f, wq + dd, w.s_qkv + D, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.vw, D, D, 1.0f, wq + 2 * dd, w.s_qkv + 2 * D, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.ow, D, D, 1.0f, w.o, w.s_o, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.f1w, M1, D, 1.0f, w.fc1, w.s_fc1, s));
        HIPCHK(&c->err, launch_quantize_rows(P + o.f2w, D, M, 1.0f, w.fc2, w.s_fc2, s));
    }
    // VH_FLAG_W8_E4M3: the six matrices of a layer pass through the e4m3 quantiser (one scale per output channel) and back
    // before the 16-bit preparation -- weight-only fp8 with dequantisation at load (SURVEY.md section 7 option (a))
    float* w8tmp = nullptr;
    struct FreeOnExit { float*& p; ~FreeOnExit() { if (p) { hipFree(p); p = nullptr; } } } w8tmp_guard{w8tmp};   // every early return below frees the scratch
    const size_t dd1 = (size_t)D * D, md1 = (size_t)M * D;
    if (!c->fp8 && (f.flags & VH_FLAG_W8_E4M3)) { HIPCHK(&c->err, hipMalloc((void**)&w8tmp, (4 * dd1 + 2 * md1) * sizeof(float))); }
    for (int l = 0; l < f.layers && !c->fp8; ++l) {
        LayerOff o = L.layer[l];
        const float* P = c->params;
        if (w8tmp) {
            const size_t src[6] = {o.qw, o.kw, o.vw, o.ow, o.f1w, o.f2w};
            const int rows[6] = {D, D, D, D, M, D}, cols[6] = {D, D, D, D, D, M};
            size_t at = 0;
            for (int i = 0; i < 6; ++i) {
                HIPCHK(&c->err, launch_fake_quant_rows(c->params + src[i], rows[i], cols[i], w8tmp + at, s));
                at += (size_t)rows[i] * cols[i];
            }
            // the matrix offsets now point into w8tmp (relative to P = w8tmp - 0): rebase through pointer arithmetic
            P = w8tmp;
            o.qw = 0; o.kw = dd1; o.vw = 2 * dd1; o.ow = 3 * dd1; o.f1w = 4 * dd1; o.f2w = 4 * dd1 + md1;
        }
        const float* B = c->params;   // biases and LayerNorm parameters stay where they are
        const LayerW& w = c->layer[l];
        if (c->ln_fold) {
            // W' = gamma o W (q rows also carry the softmax scale q_scale), c = row sums of W', d = beta.W + b
            char* wq = (char*)w.qkv;
            const size_t dd2 = (size_t)D * D * 2;
            HIPCHK(&c->err, launch_fold_ln(P + o.qw, B + o.qb, B + o.ln1w, B + o.ln1b, D, D, c->q_scale, wq, w.c_qkv, w.d_qkv, f.dtype, s));
            HIPCHK(&c->err, launch_fold_ln(P + o.kw, B + o.kb, B + o.ln1w, B + o.ln1b, D, D, 1.0f, wq + dd2, w.c_qkv + D, w.d_qkv + D, f.dtype, s));
            HIPCHK(&c->err, launch_fold_ln(P + o.vw, B + o.vb, B + o.ln1w, B + o.ln1b, D, D, 1.0f, wq + 2 * dd2, w.c_qkv + 2 * D, w.d_qkv + 2 * D, f.dtype, s));
            HIPCHK(&c->err, launch_fold_ln(P + o.f1w, B + o.f1b, B + o.ln2w, B + o.ln2b, M1, D, 1.0f, w.fc1, w.c_fc1, w.d_fc1, f.dtype, s));
        } else {
            HIPCHK(&c->err, launch_pack_qkv(P + o.qw, B + o.qb, P + o.kw, B + o.kb, P + o.vw, B + o.vb, D, c->q_scale, w.qkv, w.bqkv, f.dtype, s));
            HIPCHK(&c->err, launch_cast(P + o.f1w, w.fc1, (int64_t)M1 * D, f.dtype, s));
        }
        HIPCHK(&c->err, launch_cast(P + o.ow, w.o, (int64_t)D * D, f.dtype, s));
        HIPCHK(&c->err, launch_cast(P + o.f2w, w.fc2, (int64_t)D * M, f.dtype, s));
        if (c->h_tiled && w.fc2_t) HIPCHK(&c->err, launch_cast_tiled_w(P + o.f2w, D, M, w.fc2_t, f.dtype, s));
        if (c->h_tiled && w.o_t) HIPCHK(&c->err, launch_cast_tiled_w(P + o.ow, D, D, w.o_t, f.dtype, s));
        if (w8tmp) { HIPCHK(&c->err, hipStreamSynchronize(s)); }   // the scratch is reused by the next layer
    }
    HIPCHK(&c->err, hipStreamSynchronize(s));
    c->weights_ready = true;
    c->weights_ready_tiled = c->h_tiled && (!c->fp8 || c->ln_fold);   // (e4m3 operands: prepared in the folded branch only)
    return VH_OK;
}

// new weights: the guard starts over and the path is the configured one again
void drop_graphs(vh_ctx* c);
hipError_t sync_compute(vh_ctx* c);
int guard_reset(vh_ctx* c) {
    HIPCHK(&c->err, sync_compute(c));   // no forward in flight still writes the words
    HIPCHK(&c->err, hipMemsetAsync(c->guard_dev, 0, 2 * sizeof(unsigned int), c->stream));
    c->guard_host[0] = c->guard_host[1] = 0.f;
    c->guard_tripped = false;
    c->ln_fold = c->ln_fold_cfg;
    c->split = c->split_cfg;
    // Captured launch sequences belong to the path (and the weight layout) they were captured on: a context whose guard had
    // tripped holds graphs of the stand-alone-LayerNorm sequence, and replaying those against re-folded weights would be
    // silently wrong.  New weights, new graphs.
    drop_graphs(c);
    return VH_OK;
}

int check_blob_header(vh_ctx* c, const BlobHeader& h) {
    const vh_config& f = c->cfg;
    if (memcmp(h.magic, "VHBLOB1", 8) != 0) return fail(&c->err, VH_ERR_INVALID, "weight blob: bad magic");
    if (h.image_size != f.image_size || h.patch_size != f.patch_size || h.channels != f.channels || h.dim != f.dim ||
        h.heads != f.heads || h.mlp_dim != f.mlp_dim || h.layers != f.layers || h.classes != f.classes)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: shape differs from the context's vh_config");
    const uint32_t want = blob_model_bits(f);
    if ((h.flags ^ want) & kBlobPreLn)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 1 (pre-LayerNorm) is %d, the context's VH_FLAG_PRE_LN is %d",
                    (h.flags & kBlobPreLn) != 0, (want & kBlobPreLn) != 0);
    if ((h.flags ^ want) & kBlobQuickGelu)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 2 (QuickGELU) is %d, the context's VH_FLAG_QUICK_GELU is %d",
                    (h.flags & kBlobQuickGelu) != 0, (want & kBlobQuickGelu) != 0);
    if ((h.flags ^ want) & kBlobRegisters)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bits 9..13 say %d register tokens, the context's VH_FLAG_REGISTERS says %d",
                    (int)VH_FLAG_REGISTERS_OF(h.flags), (int)VH_FLAG_REGISTERS_OF(want));
    if ((h.flags ^ want) & kBlobNoCls)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 15 (no class token) is %d, the context's VH_FLAG_NO_CLS is %d",
                    (h.flags & kBlobNoCls) != 0, (want & kBlobNoCls) != 0);
    if ((h.flags ^ want) & kBlobPool)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bits 16..17 say pooling mode %d, the context's VH_FLAG_POOL says %d",
                    (int)VH_FLAG_POOL_OF(h.flags), (int)VH_FLAG_POOL_OF(want));
    if ((h.flags ^ want) & kBlobMapHead)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 19 (attention-pooling head) is %d, the context's VH_FLAG_MAP_HEAD is %d",
                    (h.flags & kBlobMapHead) != 0, (want & kBlobMapHead) != 0);
    if ((h.flags ^ want) & kBlobTanhGelu)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 21 (tanh GELU) is %d, the context's VH_FLAG_TANH_GELU is %d",
                    (h.flags & kBlobTanhGelu) != 0, (want & kBlobTanhGelu) != 0);
    if ((h.flags ^ want) & kBlobSwiglu)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 25 (SwiGLU MLP) is %d, the context's VH_FLAG_SWIGLU is %d",
                    (h.flags & kBlobSwiglu) != 0, (want & kBlobSwiglu) != 0);
    if ((h.flags ^ want) & kBlobRope)
        return fail(&c->err, VH_ERR_INVALID, "weight blob: header bit 23 (rotary position embedding) is %d, the context's VH_FLAG_ROPE is %d",
                    (h.flags & kBlobRope) != 0, (want & kBlobRope) != 0);
    return VH_OK;
}

// the launch sequence of ONE forward; `ev` (optional) receives an event after every stage
// `img0`: first image of this part inside the activation arena (a batch can be split into parts that run on
// different streams: rows of different images never interact), `s`: the stream to enqueue on.
// `A`: the buffer set this forward owns; `head_wait` (optional): the final LayerNorm / pooling and the head -- the launches that
// end in the write of `logits` -- wait for it (two forwards in flight: the step before this one wrote the same logits first).
int enqueue_forward(vh_ctx* c, ImgIn in, int batch, float* logits, std::vector<std::pair<int, hipEvent_t>>* ev,
                    hipStream_t s, int img0, bool may_pad = true, int set = 0, hipEvent_t head_wait = nullptr) {
    // This part's slices of the set.  Parts take disjoint slices; a part's partial-sum block is (D/64) * rows * 2 floats, laid out
    // for ITS row count.
    const ActSet A = part_set(c, c->act[set], img0);
    c->last_set = set;
    const vh_config& f = c->cfg;
    const Layout& L = c->L;
    const int D = f.dim, M = f.mlp_dim, M1 = L.M1, T = L.T;   // M1: fc1's width (2 M on a VH_FLAG_SWIGLU context)
    const int64_t rows = (int64_t)batch * T;
    // Row count of the per-token GEMMs of the folded layer loop: rounded up to whole 256-row tiles when nothing lives behind
    // this part's rows in the arena (a single part, or the last of several; the arena itself is padded).  The persistent
    // GEMM form runs full tiles only, and a ragged last row of tiles would send the launch to the one-tile form.  The
    // padding rows hold whatever the arena holds: rows never mix in a GEMM, the attention kernel and the head read real
    // rows only, so nothing of them reaches a logit.
    // Worth it from about two full rounds of tiles per GEMM on (measured, ViT-B bf16: batch 300 +2.5 %, batch 128 -2 %:
    // with fewer tiles the one-tile form's dynamic placement wins).
    const int64_t row_tiles = (rows + 255) / 256;
    const int64_t rows_g = (may_pad && c->ln_fold && row_tiles * ((D + 255) / 256) >= 2 * (int64_t)c->num_cu) ? row_tiles * 256 : rows;
    const float* P = c->params;
    const size_t r0 = (size_t)img0 * T, esz = 2;   // r0: this part's first row of a capture slot; esz: a 16-bit element
    const int dt16 = c->dt16;
    // VH_FLAG_NO_CLS: no class-token row.  The patch GEMM's epilogue adds "pos row 1 + p", so a context without pos[0] hands it the
    // table one row early (inside the resident blob: the header and the patch tensors precede pos); the leading rows are all registers.
    const float* const cls_p = L.ncls ? P + L.cls : nullptr;
    const float* const pos_p = P + L.pos - (L.ncls ? 0 : D);
    // the attention launches' work-queue counters: one word per layer, all zeroed by ONE memset per forward (a memset per
    // launch is a 5 us fill kernel in front of every attention kernel)
    if (f.layers > 0) HIPCHK(&c->err, hipMemsetAsync(A.tickets, 0, sizeof(unsigned int) * f.layers, s));
    // fp8 operands: the folded GEMMs multiply the RAW residual rows as e4m3, which saturates at 448 -- the statistics kernels
    // keep a running maximum of |x| (a bound of it) in the guard's second word
    unsigned int* const amax_guard = c->fp8 ? c->guard_dev + 1 : nullptr;
    auto mark = [&](int stage) -> int {
        if (!ev) return VH_OK;
        hipEvent_t e;
        HIPCHK(&c->err, hipEventCreate(&e));
        HIPCHK(&c->err, hipEventRecord(e, s));
        ev->push_back({stage, e});
        return VH_OK;
    };
    // hip events around every launch of the stage selected by vh_set_stage_timing()
    auto tmark = [&](int stage) -> int { return stage == c->timing_stage ? record_next(c, c->tev, c->tev_used, s) : VH_OK; };
    // The one GemmArgs builder of this part.  It sets what every launch shares: the operand dtype (op_dt in the layer loops, dt16 for
    // the patch GEMM) and this part's statistics slices (LNFOLD* reads stats, RESID_* / PATCH_SPLIT write partials, the others ignore
    // both).  A launch adds what its epilogue and layout need: out16, wscale (null on the 16-bit paths), a layout flag, a tile range.
    const int op_dt = c->fp8 ? VH_DTYPE_FP8 : dt16;   // type of the GEMM A operands produced by LN / attention / fc1
    auto gemm_args = [&](int dtype, const void* a, const void* w, const float* bias, void* out, int64_t Mr, int N, int K, int epi,
                         const float* aux = nullptr, int aux_i = 0) {
        GemmArgs g{a, w, bias, out, Mr, N, K, epi, aux, aux_i, dtype, 0};
        g.stats = A.stats;
        g.partials = A.partials;
        return g;
    };
    // the tiled layouts exist in the persistent form only, and a launch that asks for one names that form (gemm_check)
    auto set_tiled = [](GemmArgs& g, bool out_tiled, bool ab_tiled) {
        g.out_tiled = out_tiled;
        g.ab_tiled = ab_tiled;
        if (out_tiled || ab_tiled) g.variant = 6;
    };
    // the stage bracket: the stage-timing events around one launch, then the stage's profile event
    auto stage = [&](int st, auto&& launch) -> int {
        int r;
        if ((r = tmark(st))) return r;
        HIPCHK(&c->err, launch());
        if ((r = tmark(st))) return r;
        return mark(st);
    };
    int rc;
    if ((rc = mark(-1))) return rc;
    const int nl = layers_to_run(c);
    // where this part's residual rows live behind every layer, and at the end of the forward
    const ResidView resid = resid_view(c, A, nl);
    // Layer features: behind fc2 of layer l, when l + 1 is listed and more layers follow, this part's real rows go to the capture
    // store in the form the path holds them, at the part's row offset -- one launch.  (The listed layer that equals nl needs no copy:
    // the live residual serves it.)  What was captured is recorded for the read-out; every part records the same values.
    c->cap_nl = nl;
    c->cap_form = resid.form;
    c->cap_n = c->feat_n;
    for (int i = 0; i < c->cap_n; ++i) c->cap_layers[i] = c->feat_layers[i];
    auto capture = [&](int l) -> int {
        if (!c->feat_store || l + 1 >= nl) return VH_OK;
        for (int i = 0; i < c->feat_n; ++i) {
            if (c->feat_layers[i] != l + 1) continue;
            const ResidView slot = slot_view(c, i, resid.form);
            const size_t n = (size_t)rows * D, hb = hi_bytes(resid.form), lb = lo_bytes(resid.form);
            HIPCHK(&c->err, launch_feature_capture(resid.hi, (char*)slot.hi + r0 * D * hb, n * hb, resid.lo, resid.lo ? (char*)slot.lo + r0 * D * lb : nullptr, n * lb, s));
        }
        return VH_OK;
    };
    // Attention maps: behind the q|k|v projection of layer l, when l + 1 is listed, the softmax rows of this part's first attn_q
    // queries go to the store at the part's image offset -- one launch, from the layout this part holds (hm_rows != 0: head-major).
    // Head-major layout and rows_g are this part's own, which is why the capture is a push from here and not a later read of q|k|v.
    c->acap_nl = nl;
    c->acap_n = c->attn_n;
    for (int i = 0; i < c->acap_n; ++i) c->acap_layers[i] = c->attn_layers[i];
    auto capture_attention = [&](int l, int64_t hm_rows) -> int {
        if (!c->attn_store) return VH_OK;
        for (int i = 0; i < c->attn_n; ++i) {
            if (c->attn_layers[i] != l + 1) continue;
            float* const slot = (float*)(c->attn_store + (size_t)i * c->attn_slot) + (size_t)img0 * f.heads * c->attn_q * T;
            HIPCHK(&c->err, launch_attention_probs(A.qkv16, hm_rows, batch, T, f.heads, c->head_dim, c->attn_q, dt16, slot, s));
        }
        return VH_OK;
    };
    // VH_FLAG_ROPE: behind the q|k|v projection and in front of the capture above and of attention, q and k of this part's patch rows
    // are rotated in place by the blob's tables -- one launch per layer, in the layout this part holds (hm_rows != 0: head-major).
    // Without the flag: no launch.  (No stage of its own: it is neither the projection's time nor attention's.)
    auto rope = [&](int64_t hm_rows) -> int {
        if (!L.rope) return VH_OK;
        HIPCHK(&c->err, launch_rope(A.qkv16, dt16, batch, T, f.heads, c->head_dim, L.lead, hm_rows, P + L.rope_cos, P + L.rope_sin, s));
        return VH_OK;
    };
    // VH_FLAG_SWIGLU: behind fc1, which wrote gu16 [rows][2 M] row-major, the gate pass leaves h16 = silu(g) * u in the layout fc2 reads
    // (tiled under h_tiled's condition) -- one launch per layer.  Without the flag: no launch.  (No stage of its own, as for the rotation:
    // the stage table is pinned; tools/swiglu_bench.py reports the pass as a step difference.  VH_SWIGLU_SKIP=1, read when the context
    // is created, is that tool's switch: fc2 then reads whatever h16 holds, and the logits mean nothing.)
    auto gate = [&](int64_t nrows, bool tiled) -> int {
        if (!L.swiglu || c->swiglu_skip) return VH_OK;
        HIPCHK(&c->err, launch_swiglu(A.gu16, dt16, nrows, M, A.h16, tiled ? 1 : 0, s));
        return VH_OK;
    };
    // Patch embedding: the im2col pass + the persistent GEMM.
    // VH_FLAG_PRE_LN: a LayerNorm needs whole rows, which no patch-GEMM tile holds -- such a context embeds through the fp32-x branch
    // and one pre_layernorm_kernel pass turns x into what its path consumes (no PATCH_SPLIT, no rowstats pass)
    const bool pre_ln = (f.flags & VH_FLAG_PRE_LN) != 0;
    const bool quick = (f.flags & VH_FLAG_QUICK_GELU) != 0, tanh_gelu = (f.flags & VH_FLAG_TANH_GELU) != 0;
    // VH_FLAG_SWIGLU: fc1 keeps the GEMMs' plain epilogues (no activation) and writes gu16 row-major; the gate pass behind it makes h16
    const bool swiglu = L.swiglu;
    const int epi_fc1 = swiglu ? VH_EPI_LNFOLD : quick ? VH_EPI_LNFOLD_QGELU : tanh_gelu ? VH_EPI_LNFOLD_TGELU : VH_EPI_LNFOLD_GELU;          // folded layer loop
    const int epi_fc1_plain = swiglu ? VH_EPI_BIAS : quick ? VH_EPI_BIAS_QGELU : tanh_gelu ? VH_EPI_BIAS_TGELU : VH_EPI_BIAS_GELU;       // plain layer loop
    // the patch embedding lands directly in the split residual's planes (below): the 16-bit split path without a pre-LayerNorm
    const bool patch_split = c->split && !c->fp8 && nl > 0 && !pre_ln;
    // (no stage bracket: the profile event is recorded once, behind the pass)
    if ((rc = tmark(ST_IM2COL))) return rc;
    if (in.layout == VH_LAYOUT_NHWC && in.u8())
        HIPCHK(&c->err, launch_im2col_u8((const uint8_t*)in.p, batch, f.image_size, f.patch_size, f.channels, L.KPA, c->in_scale, c->in_shift,
                                         A.col16, dt16, s));
    else if (in.nhwc_f32())
        HIPCHK(&c->err, launch_im2col((const float*)in.p, batch, f.image_size, f.patch_size, f.channels, L.KPA, A.col16, dt16, s));
    else   // every other (element type, layout): kernels_gather.hip
        HIPCHK(&c->err, launch_im2col_tensor(in.p, in.kind, in.layout, batch, f.image_size, f.patch_size, f.channels, L.KPA, c->in_scale,
                                             c->in_shift, A.col16, dt16, s));
    if ((rc = tmark(ST_IM2COL))) return rc;
    if ((rc = mark(ST_IM2COL))) return rc;
    if (patch_split) {
        // Split residual: the patch embedding lands DIRECTLY in the two 16-bit planes, with the first row statistics'
        // partial sums (PATCH_SPLIT epilogue; the class-token rows from their own small kernel) -- no fp32
        // x, no separate row-statistics pass over it (round 3: -0.1 ms per forward).  The partial sums are laid out for rows_g
        // rows, like every later layer's.
        GemmArgs g = gemm_args(dt16, A.col16, c->wp16, P + L.patch_b, A.xn16, (int64_t)batch * L.NP, D, L.KPA, VH_EPI_PATCH_SPLIT, pos_p, L.NP);
        g.out16 = A.xlo16;
        g.prow = rows_g;
        g.lead = L.lead;
        if ((rc = stage(ST_PATCH, [&] { return launch_gemm(g, s); }))) return rc;
        if ((rc = stage(ST_CLS, [&] {
                 return launch_lead_rows_split(A.xn16, A.xlo16, A.partials, rows_g, cls_p, pos_p, P + L.reg, L.lead, batch, T, D, dt16, s);
             })))
            return rc;
        HIPCHK(&c->err, launch_finalize_stats(A.partials, D / 64, rows_g, D, f.ln_eps, A.stats, s, rows, c->guard_dev, amax_guard));
        if ((rc = mark(ST_LNSTATS))) return rc;   // (no tmark: ST_LNSTATS has no stage timing)
    } else {
        GemmArgs g = gemm_args(dt16, A.col16, c->wp16, P + L.patch_b, A.x, (int64_t)batch * L.NP, D, L.KPA, VH_EPI_PATCH, pos_p, L.NP);
        g.lead = L.lead;
        if ((rc = stage(ST_PATCH, [&] { return launch_gemm(g, s); }))) return rc;
        if ((rc = stage(ST_CLS, [&] { return launch_lead_rows(A.x, cls_p, pos_p, P + L.reg, L.lead, batch, T, D, s); }))) return rc;
        if (pre_ln) {
            // x <- LN(x) pre_ln.weight + pre_ln.bias, in the form the path consumes: the fp32 array (plain loop, non-split fold, no
            // layer at all), the 16-bit operand copy / the split planes, layer 0's LN1 statistics of the normalised rows and the guards
            const bool fold0 = c->ln_fold && nl > 0;
            if ((rc = stage(ST_PRELN, [&] {
                     return launch_pre_layernorm(A.x, fold0 ? rows_g : rows, D, P + L.prew, P + L.preb, f.ln_eps, fold0 && c->split ? nullptr : A.x,
                                                 fold0 ? A.xn16 : nullptr, fold0 && c->split ? A.xlo16 : nullptr, fold0 ? A.stats : nullptr, op_dt, s,
                                                 rows, fold0 ? c->guard_dev : nullptr, fold0 ? amax_guard : nullptr);
                 })))
                return rc;
        } else if (c->ln_fold && nl > 0) {
            // layer 0's LN1 statistics: its input comes from the patch embedding, not from a RESID_LN epilogue
            // (fp8 path with the split residual: the patch embedding stays the bf16 fp32-out GEMM; this pass makes the planes)
            if (c->split) HIPCHK(&c->err, launch_rowstats_split(A.x, rows_g, D, f.ln_eps, A.xn16, A.xlo16, A.stats, op_dt, s, rows, amax_guard));
            else HIPCHK(&c->err, launch_rowstats_cast(A.x, rows_g, D, f.ln_eps, A.xn16, A.stats, op_dt, s, rows, amax_guard));
            HIPCHK(&c->err, launch_ln_guard(A.stats, rows, c->guard_dev, s));   // real rows only (rows_g - rows are tile padding)
            if ((rc = mark(ST_LNSTATS))) return rc;   // (no tmark, as above)
        }
    }
    // the class-token tail needs the split planes of the folded 16-bit path, the whole model, and room in the patch-matrix buffer
    // (head dim 64 only: the class-row kernel is 64 wide; other head dims run the full last layer)
    const bool hd64 = c->head_dim == 64;
    const bool tail = c->cls_tail && hd64 && c->ln_fold && c->split && !c->fp8 && nl == f.layers && c->run_layers < 0 && T <= 1024 &&
                      (size_t)L.NP * L.KPA * esz >= 2 * ((size_t)D * esz + 256);
    // tiled hidden activation (16-bit or e4m3, in the operand's own tiled layout: fc1's epilogue writes it, fc2's DMA reads it): both
    // MLP GEMMs must take the persistent form (whole 256-row tiles, enough of them), the split path
    const bool h_tiled = c->h_tiled && c->split && c->weights_ready_tiled && gemm_tiled_applies(rows_g, M, D, op_dt) && gemm_tiled_applies(rows_g, D, M, op_dt);
    // the attention output likewise (ring forms -> the out-projection's tiled operand DMA); VH_ATT_TILED=0 keeps it row-major
    // (both 64-wide forms: any other head dim keeps q|k|v and the attention output row-major; the class-token tail, a 16-bit path, too)
    const bool att_tiled = hd64 && h_tiled && c->att_tiled && gemm_tiled_applies(rows_g, D, D, op_dt) && attention_tiled_applies(batch, T, f.heads) && !tail;
    // q|k|v head-major between the projection's epilogue and attention's operand DMA (same condition + the persistent form for N = 3 D)
    const bool qkv_hm = c->qkv_hm && att_tiled && gemm_tiled_applies(rows_g, 3 * D, D, op_dt);
    c->last_h_tiled = h_tiled && nl > 0 && c->ln_fold;
    c->last_qkv_hm = qkv_hm && nl > 0 && c->ln_fold;
    for (int l = 0; l < nl && c->ln_fold; ++l) {
        const LayerOff& o = L.layer[l];
        const LayerW& w = c->layer[l];
        const int nblk = D / 64;
        GemmArgs gq = gemm_args(op_dt, A.xn16, w.qkv, w.d_qkv, A.qkv16, rows_g, 3 * D, D, VH_EPI_LNFOLD, w.c_qkv);
        gq.wscale = w.s_qkv;
        set_tiled(gq, qkv_hm, false);
        if ((rc = stage(ST_QKV, [&] { return launch_gemm(gq, s); }))) return rc;
        if ((rc = rope(qkv_hm ? (int64_t)rows_g : 0))) return rc;
        if ((rc = capture_attention(l, qkv_hm ? (int64_t)rows_g : 0))) return rc;
        if (tail && l + 1 == nl) {
            // VH_FLAG_CLS_TAIL, last layer: only the class-token row of every image reaches the head, so attention runs for that
            // one query (all keys and values), and out-proj, fc1 and fc2 run on the `batch` class rows, gathered into compact
            // planes (the idle patch-matrix buffer).  Same kernels, same per-row arithmetic as the full layer, except the
            // attention row (a VALU kernel with another summation order): logits agree to rounding, not bitwise.
            // (no stage bracket in this branch: the tail has no stage timing, only the profile events)
            char* const hc = (char*)A.col16;
            char* const lc = hc + (((size_t)batch * D * esz + 255) & ~(size_t)255);
            HIPCHK(&c->err, launch_attention_cls(A.qkv16, batch, T, f.heads, A.att16, dt16, s));
            if ((rc = mark(ST_ATTN))) return rc;
            HIPCHK(&c->err, hipMemcpy2DAsync(hc, (size_t)D * esz, A.xn16, (size_t)T * D * esz, (size_t)D * esz, batch, hipMemcpyDeviceToDevice, s));
            HIPCHK(&c->err, hipMemcpy2DAsync(lc, (size_t)D, A.xlo16, (size_t)T * D, (size_t)D, batch, hipMemcpyDeviceToDevice, s));
            GemmArgs gp = gemm_args(op_dt, A.att16, w.o, P + o.ob, hc, batch, D, D, VH_EPI_RESID_SPLIT);
            gp.out16 = lc;
            HIPCHK(&c->err, launch_gemm(gp, s));
            if ((rc = mark(ST_PROJ))) return rc;
            HIPCHK(&c->err, launch_finalize_stats(A.partials, nblk, batch, D, f.ln_eps, A.stats, s, batch, c->guard_dev));
            if ((rc = mark(ST_LNSTATS))) return rc;
            const GemmArgs g1 = gemm_args(op_dt, hc, w.fc1, w.d_fc1, A.h16, batch, M1, D, epi_fc1, w.c_fc1);   // (no gate pass: M1 = M here, check_config)
            HIPCHK(&c->err, launch_gemm(g1, s));
            if ((rc = mark(ST_FC1))) return rc;
            GemmArgs g2 = gemm_args(op_dt, A.h16, w.fc2, P + o.f2b, hc, batch, D, M, VH_EPI_RESID_SPLIT);
            g2.out16 = lc;
            HIPCHK(&c->err, launch_gemm(g2, s));
            if ((rc = mark(ST_FC2))) return rc;
            if (head_wait) HIPCHK(&c->err, hipStreamWaitEvent(s, head_wait, 0));
            HIPCHK(&c->err, launch_layernorm_split(hc, lc, batch, D, D, P + L.lnfw, P + L.lnfb, f.ln_eps, A.clsn32, dt16, s));
            if ((rc = mark(ST_LNF))) return rc;
            HIPCHK(&c->err, launch_head_f32(A.clsn32, P + L.headw, P + L.headb, logits, batch, f.classes, D, s));
            if ((rc = mark(ST_HEAD))) return rc;
            c->last_batch = batch;
            return VH_OK;
        }
        if ((rc = stage(ST_ATTN, [&] {
                 return hd64 ? launch_attention(A.qkv16, batch, T, f.heads, A.att16, op_dt, A.tickets + l, s, true, att_tiled, qkv_hm ? (int64_t)rows_g : 0)
                             : launch_attention_hd(A.qkv16, batch, T, f.heads, c->head_dim, A.att16, op_dt, s);
             })))
            return rc;
        // out-projection and fc2 add to the residual.  Split: (out, out16) = its (hi, lo) planes; otherwise the fp32 x and, with RESID_LN,
        // the operand copy of the updated rows.  A tiled A operand goes with the weights' tiled copy.
        GemmArgs go = gemm_args(op_dt, A.att16, att_tiled ? w.o_t : w.o, P + o.ob, c->split ? A.xn16 : A.x, rows_g, D, D,
                                c->split ? VH_EPI_RESID_SPLIT : VH_EPI_RESID_LN);
        go.out16 = c->split ? A.xlo16 : A.xn16;
        go.wscale = w.s_o;
        set_tiled(go, false, att_tiled);
        if ((rc = stage(ST_PROJ, [&] { return launch_gemm(go, s); }))) return rc;
        HIPCHK(&c->err, launch_finalize_stats(A.partials, nblk, rows_g, D, f.ln_eps, A.stats, s, rows, c->guard_dev, amax_guard));
        if ((rc = mark(ST_LNSTATS))) return rc;   // (no tmark, as above)
        // h in its tiled layout: written straight from fc1's registers, read by fc2's DMA (same values, same bits)
        GemmArgs g1 = gemm_args(op_dt, A.xn16, w.fc1, w.d_fc1, swiglu ? A.gu16 : A.h16, rows_g, M1, D, epi_fc1, w.c_fc1);
        g1.wscale = w.s_fc1;
        set_tiled(g1, h_tiled && !swiglu, false);
        if ((rc = stage(ST_FC1, [&] { return launch_gemm(g1, s); }))) return rc;
        if ((rc = gate(rows_g, h_tiled))) return rc;
        GemmArgs g2 = gemm_args(op_dt, A.h16, h_tiled ? w.fc2_t : w.fc2, P + o.f2b, c->split ? A.xn16 : A.x, rows_g, D, M,
                                c->split ? VH_EPI_RESID_SPLIT : (l + 1 < nl ? VH_EPI_RESID_LN : VH_EPI_BIAS_RESID));
        g2.out16 = c->split ? A.xlo16 : A.xn16;
        g2.wscale = w.s_fc2;
        set_tiled(g2, false, h_tiled);
        if ((rc = stage(ST_FC2, [&] { return launch_gemm(g2, s); }))) return rc;
        if ((rc = capture(l))) return rc;
        if (l + 1 < nl) {
            HIPCHK(&c->err, launch_finalize_stats(A.partials, nblk, rows_g, D, f.ln_eps, A.stats, s, rows, c->guard_dev, amax_guard));
            if ((rc = mark(ST_LNSTATS))) return rc;   // (no tmark, as above)
        }
    }
    // ---- the plain layer loop (bf16 / fp16 / fp8 operands) -----------------------------------------------------
    const bool plain = !c->ln_fold;
    auto ln_rows = [&](const float* w, const float* b) { return launch_layernorm(A.x, rows, D, D, w, b, f.ln_eps, A.xn16, op_dt, s); };
    // Residual GEMM (x += A W^T + bias) followed by the LayerNorm of the updated rows
    auto resid_gemm_ln = [&](const void* a, const void* w, const float* bias, const float* scale, int K, const float* lnw,
                             const float* lnb, int st_gemm) -> int {
        GemmArgs g = gemm_args(op_dt, a, w, bias, A.x, rows, D, K, VH_EPI_BIAS_RESID);
        g.wscale = scale;
        if (int r = stage(st_gemm, [&] { return launch_gemm(g, s); })) return r;
        return lnw ? stage(ST_LN, [&] { return ln_rows(lnw, lnb); }) : VH_OK;
    };
    if (plain && nl > 0) {
        const LayerOff& o0 = L.layer[0];
        if ((rc = stage(ST_LN, [&] { return ln_rows(P + o0.ln1w, P + o0.ln1b); }))) return rc;
    }
    for (int l = 0; l < nl && plain; ++l) {
        const LayerOff& o = L.layer[l];
        const LayerW& w = c->layer[l];
        GemmArgs gq = gemm_args(op_dt, A.xn16, w.qkv, w.bqkv, A.qkv16, rows, 3 * D, D, VH_EPI_BIAS);
        gq.wscale = w.s_qkv;
        if ((rc = stage(ST_QKV, [&] { return launch_gemm(gq, s); }))) return rc;
        if ((rc = rope(0))) return rc;
        if ((rc = capture_attention(l, 0))) return rc;
        if ((rc = stage(ST_ATTN, [&] {
                 return hd64 ? launch_attention(A.qkv16, batch, T, f.heads, A.att16, op_dt, A.tickets + l, s, true)
                             : launch_attention_hd(A.qkv16, batch, T, f.heads, c->head_dim, A.att16, op_dt, s);
             })))
            return rc;
        if ((rc = resid_gemm_ln(A.att16, w.o, P + o.ob, w.s_o, D, P + o.ln2w, P + o.ln2b, ST_PROJ))) return rc;
        GemmArgs g1 = gemm_args(op_dt, A.xn16, w.fc1, P + o.f1b, swiglu ? A.gu16 : A.h16, rows, M1, D, epi_fc1_plain);
        g1.wscale = w.s_fc1;
        if ((rc = stage(ST_FC1, [&] { return launch_gemm(g1, s); }))) return rc;
        if ((rc = gate(rows, false))) return rc;
        const bool more = l + 1 < nl;   // the next layer's LN1 follows this layer's fc2
        if ((rc = resid_gemm_ln(A.h16, w.fc2, P + o.f2b, w.s_fc2, M, more ? P + L.layer[l + 1].ln1w : nullptr,
                                more ? P + L.layer[l + 1].ln1b : nullptr, ST_FC2))) return rc;
        if ((rc = capture(l))) return rc;   // behind both launches of resid_gemm_ln: x is complete and nothing writes it
    }
    // The head's input [batch][W] (vithip.h VH_FLAG_POOL).  VH_POOL_CLS: the final LayerNorm of row 0, as ever.  VH_POOL_CLS_AVG: the
    // same launch into scratch, which the pool kernel copies into columns 0 .. D - 1 beside its own D .. 2 D - 1.  The pooled modes
    // read the patch rows where the path left them (planes or the fp32 array) ONCE.  All of it under the final-LayerNorm stage.
    if (head_wait) HIPCHK(&c->err, hipStreamWaitEvent(s, head_wait, 0));
    if (L.map) {
        // VH_FLAG_MAP_HEAD (vithip.h "THE FUNCTION"): ONE pass over the patch rows leaves z [batch][H][D]; everything behind it is fp32
        // on `batch` rows through the head's own exact-fp32 kernel: the per-head V product (H groups in one launch), the
        // out-projection, the block's LayerNorm, fc1, the activation, fc2 + the residual.  u lands in clsn32, the head's input.
        const int H = f.heads, hd = D / H;
        float *const z = A.mapz32, *const hid = A.maph32;
        float* const a32 = A.mapa32;                                // a [batch][D]
        float* const o32 = A.mapa32 + (size_t)f.max_batch * D;      // o [batch][D]: the buffer's second array
        float* const lnrow = z;                                     // [batch][D]: z is dead once a exists
        const PoolArgs pa{resid.hi, resid.lo, resid.form, batch, T, L.lead, D, P + L.lnfw, P + L.lnfb, f.ln_eps, VH_FEAT_NORM, z};
        HIPCHK(&c->err, launch_map_pool(pa, P + L.map_qk, H, s));
        HIPCHK(&c->err, launch_head_f32_groups(z, (int64_t)H * D, D, P + L.map_vw, P + L.map_vb, a32, D, nullptr, batch, hd, D, H, s));
        HIPCHK(&c->err, launch_head_f32(a32, P + L.map_ow, P + L.map_ob, o32, batch, D, D, s));
        HIPCHK(&c->err, launch_layernorm(o32, batch, D, D, P + L.map_lnw, P + L.map_lnb, f.ln_eps, lnrow, VH_DTYPE_F32_INTERNAL, s));
        HIPCHK(&c->err, launch_head_f32(lnrow, P + L.map_f1w, P + L.map_f1b, hid, batch, M, D, s));
        HIPCHK(&c->err, launch_act_f32(hid, (int64_t)batch * M, quick ? 1 : tanh_gelu ? 2 : 0, s));
        HIPCHK(&c->err, launch_head_f32_groups(hid, M, 0, P + L.map_f2w, P + L.map_f2b, A.clsn32, D, o32, batch, D, M, 1, s));
    } else if (L.pool == VH_POOL_CLS || L.pool == VH_POOL_CLS_AVG) {
        float* const cls_ln = L.pool == VH_POOL_CLS ? A.clsn32 : A.pool32;
        if (resid.lo)
            HIPCHK(&c->err, launch_layernorm_split(resid.hi, resid.lo, batch, D, (int64_t)T * D, P + L.lnfw, P + L.lnfb, f.ln_eps, cls_ln, resid.form, s));
        else
            HIPCHK(&c->err, launch_layernorm(A.x, batch, D, (int64_t)T * D, P + L.lnfw, P + L.lnfb, f.ln_eps, cls_ln, VH_DTYPE_F32_INTERNAL, s));
    }
    if (!L.map && L.pool != VH_POOL_CLS) {
        PoolArgs pa{resid.hi, resid.lo, resid.form, batch, T, L.lead, D, P + L.lnfw, P + L.lnfb, f.ln_eps,
                    L.pool == VH_POOL_AVG_FCNORM ? VH_FEAT_RAW : VH_FEAT_NORM, A.clsn32};
        if (L.pool == VH_POOL_CLS_AVG) { pa.out = A.clsn32 + D; pa.out_stride = 2 * D; pa.cls_in = A.pool32; pa.cls_out = A.clsn32; }
        if (L.pool == VH_POOL_AVG_FCNORM) pa.out = A.pool32;   // LN(mean x): the raw mean, then the fp32 LayerNorm over [batch][D]
        HIPCHK(&c->err, launch_pool_rows(pa, s));
        if (L.pool == VH_POOL_AVG_FCNORM)
            HIPCHK(&c->err, launch_layernorm(A.pool32, batch, D, D, P + L.lnfw, P + L.lnfb, f.ln_eps, A.clsn32, VH_DTYPE_F32_INTERNAL, s));
    }
    if ((rc = mark(ST_LNF))) return rc;
    HIPCHK(&c->err, launch_head_f32(A.clsn32, P + L.headw, P + L.headb, logits, batch, f.classes, L.HW, s));
    if ((rc = mark(ST_HEAD))) return rc;
    c->last_batch = batch;
    return VH_OK;
}

// end of a forward: the guard word travels to pinned host memory behind the forward's kernels (stream order)
// (`s`: the stream that ran the forward.  With two forwards in flight two copies of the word may land in either order: it is a
// running maximum, so the later value is never the smaller one by more than the forward still running will add.)
int guard_publish(vh_ctx* c, hipStream_t s) {
    if (c->ln_fold) HIPCHK(&c->err, hipMemcpyAsync(c->guard_host, c->guard_dev, 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    return VH_OK;
}
// top of every forward entry point: has a COMPLETED forward seen rows beyond the guard's threshold?  (NaN trips it too.)
// Second word, fp8 operands only: rows whose raw values leave e4m3's range (the folded operand would clip them).
constexpr float kE4M3Max = 448.f;
bool guard_exceeded(const vh_ctx* c) {
    if (!c->ln_fold || !c->guard_host) return false;
    const volatile float* g = c->guard_host;
    return !(g[0] <= c->guard_thresh) || (c->fp8 && !(g[1] <= kE4M3Max));
}
int prepare_weights(vh_ctx* c);
void drop_graphs(vh_ctx* c);
int guard_poll(vh_ctx* c) {
    if (!guard_exceeded(c)) return VH_OK;
    c->guard_tripped = true;
    if (!c->guard_auto) return VH_OK;   // VH_FLAG_LN_FOLD_ON: the caller's explicit choice stands; vh_get_ln_guard reports
    c->ln_fold = false;
    c->split = false;
    drop_graphs(c);
    // prepare_weights rewrites the compute copies on c->stream: a forward in flight on the second stream still reads them
    if (c->stream2) HIPCHK(&c->err, hipStreamSynchronize(c->stream2));
    return prepare_weights(c);          // the plain (unfolded) 16-bit / e4m3 weights, from the resident blob
}

// one complete forward of `batch` images on the context's stream(s): the (optional) concurrent parts are forked
// from and joined back into c->stream, so everything that follows on c->stream sees the finished logits.
// `set` 1 (two forwards in flight, never with parts): the whole forward on the second stream with the second buffer set.
int enqueue_step(vh_ctx* c, ImgIn in, int batch, float* logits, int set = 0, hipEvent_t head_wait = nullptr) {
    const size_t img_elems = (size_t)c->cfg.image_size * c->cfg.image_size * c->cfg.channels;
    const int parts = set ? 1 : batch < c->nstreams ? batch : c->nstreams;
    int rc;
    if (parts > 1) {
        // contiguous parts of the batch on different streams: the HBM-bound stages and the partly filled
        // tail rounds of one part overlap the MFMA-bound stages of another (identical results: images
        // are independent and every per-row reduction has a fixed order)
        HIPCHK(&c->err, hipEventRecord(c->ev_fork, c->stream));
        int b0 = 0;
        for (int p = 0; p < parts; ++p) {
            const int nb = batch / parts + (p < batch % parts ? 1 : 0);
            hipStream_t st = p == 0 ? c->stream : c->xstream[p - 1];
            if (p) HIPCHK(&c->err, hipStreamWaitEvent(st, c->ev_fork, 0));
            if ((rc = enqueue_forward(c, in.skip((size_t)b0 * img_elems), nb, logits + (size_t)b0 * c->cfg.classes, nullptr, st, b0,
                                      /*may_pad: only the last part has nothing behind its rows*/ p == parts - 1))) return rc;
            if (p) {
                HIPCHK(&c->err, hipEventRecord(c->ev_join[p - 1], st));
                HIPCHK(&c->err, hipStreamWaitEvent(c->stream, c->ev_join[p - 1], 0));
            }
            b0 += nb;
        }
        c->last_batch = batch;
        return guard_publish(c, c->stream);
    }
    hipStream_t const st = set ? c->stream2 : c->stream;
    if ((rc = enqueue_forward(c, in, batch, logits, nullptr, st, 0, true, set, head_wait))) return rc;
    return guard_publish(c, st);
}

void drop_graphs(vh_ctx* c) {
    for (auto& g : c->graphs) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
    }
    c->graphs.clear();
}

// enqueue_step, or the replay of its captured launch sequence.  Small batches are launch-bound (ViT-B/16 at
// batch 1: ~100 launches, 1.27 ms eager): the graph removes the per-launch API cost and the gaps between kernels.
// (`set`, `head_wait`: enqueue_step's; a caller passes them only where two_in_flight() holds, which graph replay rules out)
int run_step(vh_ctx* c, ImgIn in, int batch, float* logits, int set = 0, hipEvent_t head_wait = nullptr) {
    if (int rc = guard_poll(c)) return rc;
    if (!c->use_graph || c->timing_stage >= 0) return enqueue_step(c, in, batch, logits, set, head_wait);
    for (auto& g : c->graphs)
        if (g.in == in && g.out == logits && g.batch == batch) {
            HIPCHK(&c->err, hipGraphLaunch(g.exec, c->stream));
            c->last_batch = batch;
            c->last_set = 0;
            return VH_OK;
        }
    bool warm = false;
    for (int b : c->graph_warm) warm |= b == batch;
    if (!warm) {  // first forward at this batch size: eager, so every kernel it uses has its attributes set
        c->graph_warm.push_back(batch);
        return enqueue_step(c, in, batch, logits);
    }
    if (c->graphs.size() >= 128) drop_graphs(c);
    vh_ctx::GraphEntry g{in, logits, batch, nullptr, nullptr};
    HIPCHK(&c->err, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_step(c, in, batch, logits);
    const hipError_t e = hipStreamEndCapture(c->stream, &g.graph);   // always close the capture
    if (rc) { if (g.graph) hipGraphDestroy(g.graph); return rc; }
    if (e != hipSuccess) return fail(&c->err, VH_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    const hipError_t ei = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
    if (ei != hipSuccess) { hipGraphDestroy(g.graph); return fail(&c->err, VH_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ei)); }
    c->graphs.push_back(g);
    HIPCHK(&c->err, hipGraphLaunch(g.exec, c->stream));
    c->last_batch = batch;
    return VH_OK;
}

// Weight-load time: decide the guarded fold BEFORE the first caller's forward.  A checkpoint's common-mode offset (position
// embedding, biases) and its massive activations are properties of the weights far more than of the image, so ONE seeded
// calibration image through the freshly prepared folded path measures them; if the guard trips, the context switches to
// the stand-alone LayerNorm here, and the asynchronous entry points (vh_forward_device_async, the ring, the groups) never
// return a batch computed on a tripped fold because of the WEIGHTS.  The per-forward guard stays as the backstop for what
// only the data can cause.  ~1.5 ms per weight load (a batch-1 forward).
int guard_calibrate(vh_ctx* c) {
    if (!c->guard_auto || !c->ln_fold) return VH_OK;
    const vh_config& f = c->cfg;
    const int64_t n = (int64_t)f.image_size * f.image_size * f.channels;
    HIPCHK(&c->err, launch_fill(c->in_dev, n, 0xCA11B8A7Eull, TID_IMAGES, 0, 0.f, 0.f, c->stream));
    const int keep_stage = c->timing_stage;
    c->timing_stage = -1;
    const int rc = enqueue_step(c, ImgIn{c->in_dev}, 1, c->logits_dev);
    c->timing_stage = keep_stage;
    if (rc) return rc;
    HIPCHK(&c->err, sync_compute(c));
    return guard_poll(c);
}

// ---- two forwards in flight ---------------------------------------------------------------------------------------------
// The second buffer set, allocated the first time it is needed (callers are outside any stream capture: graph replay is
// single-flight).  No memory for it: the context stays single-flight for good and reports no error.
bool second_set(vh_ctx* c) {
    if (c->act[1].base) return true;
    if (c->inflight_max < 2) return false;
    char* p = nullptr;
    if (hipMalloc((void**)&p, c->act_bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->inflight_max = 1;
        return false;
    }
    c->act[1].base = p;
    bind_set(c, &c->act[1], p);
    return true;
}
// May consecutive forwards of this context run two at a time?  Not where a launch is timed (a duration beside another forward's
// kernels measures neither), a graph replays (captured on one stream), the batch runs as parts (vh_set_streams), or a layer
// list is set (the feature and attention stores are one per context).
bool two_in_flight_allowed(const vh_ctx* c) {
    return c->inflight_max == 2 && c->timing_stage < 0 && !c->step_timing && !c->use_graph && c->nstreams == 1 && c->feat_n == 0 &&
           c->attn_n == 0;
}
bool two_in_flight(vh_ctx* c) { return two_in_flight_allowed(c) && second_set(c); }
// every compute stream of the context idle: c->stream, and the second stream where ring submits left forwards on it that
// c->stream has not joined (vh_forward_device_async joins its own before it returns)
hipError_t sync_compute(vh_ctx* c) {
    if (c->s2_open) {
        const hipError_t e = hipStreamSynchronize(c->stream2);
        if (e != hipSuccess) return e;
        c->s2_open = false;
    }
    return hipStreamSynchronize(c->stream);
}

int check_forward_args(vh_ctx* c, const void* in, int batch, const void* out) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (!in || !out) return fail(&c->err, VH_ERR_INVALID, "null buffer");
    if (batch <= 0 || batch > c->cfg.max_batch)
        return fail(&c->err, VH_ERR_INVALID, "batch %d outside 1..max_batch=%d", batch, c->cfg.max_batch);
    if (!c->weights_ready) return fail(&c->err, VH_ERR_STATE, "forward before weights were loaded");
    return VH_OK;
}

// elem / layout of the tensor entry points
int check_tensor_kind(std::string* err, int elem, int layout) {
    if (elem < VH_ELEM_F32 || elem > VH_ELEM_U8) return fail(err, VH_ERR_INVALID, "unknown elem %d (VH_ELEM_F32 .. VH_ELEM_U8 = 0..3)", elem);
    if (layout != VH_LAYOUT_NHWC && layout != VH_LAYOUT_NCHW) return fail(err, VH_ERR_INVALID, "unknown layout %d (VH_LAYOUT_NHWC = 0, VH_LAYOUT_NCHW = 1)", layout);
    return VH_OK;
}

int check_tensor_ptr(vh_ctx* c, const void* in_dev) {
    if ((uintptr_t)in_dev & 15) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "tensor device input %p is not 16-byte aligned", in_dev);
    return VH_OK;
}

int check_u8_ptr(vh_ctx* c, const void* in_dev) {
    if (c && ((uintptr_t)in_dev & 15)) return fail(&c->err, VH_ERR_INVALID, "8-bit device input %p is not 16-byte aligned", in_dev);
    return VH_OK;
}

// ---- 8-bit frames: plan, buffers, the resize launch ---------------------------------------------------------------------------
// One row per frame format: what differs between the formats, and nothing else.  Adding a format = one planner, one kernel
// instantiation (or kernel), one row here and five one-line exports.
// plan: checks `batch` descriptors of the row's type and builds the plan in `words`; nullptr, or why the call is refused.  base:
// the device address of the frames, 0 for a host buffer or a ring slot (copied into hipMalloc'ed, hence aligned, memory).
// launch: the one resize launch; m12: the matrix of the row's colour state.
struct FrameFormat {
    const char* tag;      // prefix of the operator tap's messages
    const char* label;    // "<label> frames need a model with 3 channels"
    const char* op_null;  // the tap's null-argument message: RGB and NV12 carry no tag
    bool three_channels;  // the model must take 3 channels (a colour matrix has three rows)
    int colour;           // index into vh_ctx::colour, -1: the format takes no matrix and no siting
    const char* (*plan)(const void* desc, int batch, int channels, int S, size_t nbytes, uintptr_t base, int chroma_site,
                        std::vector<uint32_t>* words, int* max_tiles);
    hipError_t (*launch)(const uint8_t* frames, const uint32_t* plan_dev, int batch, int channels, int S, int max_tiles, const float* m12,
                         uint8_t* out, hipStream_t stream);
};

template <int SAMPLE_BYTES>
const char* plan_semi_planar(const void* desc, int batch, int, int S, size_t nbytes, uintptr_t base, int chroma_site, std::vector<uint32_t>* words,
                             int* max_tiles) {
    return resize_plan_build_nv12((const vh_frame_nv12*)desc, batch, S, nbytes, (unsigned)(base & 3), chroma_site, SAMPLE_BYTES, words, max_tiles);
}
template <int SAMPLE_BYTES>
const char* plan_planar(const void* desc, int batch, int, int S, size_t nbytes, uintptr_t base, int chroma_site, std::vector<uint32_t>* words,
                        int* max_tiles) {
    return resize_plan_build_yuv((const vh_frame_yuv*)desc, batch, S, nbytes, (base & 1) == 0, chroma_site, SAMPLE_BYTES, words, max_tiles);
}
template <bool PLANAR, bool WIDE>
hipError_t launch_yuv(const uint8_t* frames, const uint32_t* plan_dev, int batch, int, int S, int max_tiles, const float* m12, uint8_t* out,
                      hipStream_t stream) {
    return launch_resize_yuv_any(PLANAR, WIDE, frames, plan_dev, batch, S, max_tiles, m12, out, stream);
}

template <int SAMPLE_BYTES>
const char* plan_packed422(const void* desc, int batch, int, int S, size_t nbytes, uintptr_t base, int chroma_site, std::vector<uint32_t>* words,
                           int* max_tiles) {
    return resize_plan_build_yuy2((const vh_frame_yuy2*)desc, batch, S, nbytes, (unsigned)(base & 7), chroma_site, SAMPLE_BYTES, words, max_tiles);
}
template <bool WIDE>
hipError_t launch_packed422(const uint8_t* frames, const uint32_t* plan_dev, int batch, int, int S, int max_tiles, const float* m12, uint8_t* out,
                            hipStream_t stream) {
    return launch_resize_yuy2(WIDE, frames, plan_dev, batch, S, max_tiles, m12, out, stream);
}

template <int SAMPLE_BYTES>
const char* plan_packed444(const void* desc, int batch, int, int S, size_t nbytes, uintptr_t base, int, std::vector<uint32_t>* words, int* max_tiles) {
    return resize_plan_build_bgra((const vh_frame_bgra*)desc, batch, S, nbytes, (unsigned)(base & 7), SAMPLE_BYTES, words, max_tiles);
}
template <bool WIDE>
hipError_t launch_packed444(const uint8_t* frames, const uint32_t* plan_dev, int batch, int, int S, int max_tiles, const float* m12, uint8_t* out,
                            hipStream_t stream) {
    return launch_resize_bgra(WIDE, frames, plan_dev, batch, S, max_tiles, m12, out, stream);
}

const char* plan_rgb(const void* desc, int batch, int channels, int S, size_t nbytes, uintptr_t base, int, std::vector<uint32_t>* words, int* max_tiles) {
    return resize_plan_build((const vh_frame*)desc, batch, channels, S, nbytes, (base & 3) == 0, words, max_tiles);
}
hipError_t launch_rgb(const uint8_t* frames, const uint32_t* plan_dev, int batch, int channels, int S, int max_tiles, const float*, uint8_t* out,
                      hipStream_t stream) {
    return launch_resize_u8(frames, plan_dev, batch, channels, S, max_tiles, out, stream);
}

const FrameFormat kFramesRGB = {"resize_u8", "", "null buffer", false, -1, plan_rgb, launch_rgb};
const FrameFormat kFramesNV12 = {"resize_nv12", "NV12", "null buffer", true, 0, plan_semi_planar<1>, launch_yuv<false, false>};
// (the planar planner reads base_even only for 16-bit samples: whichever address reaches this row, its plan is the same)
const FrameFormat kFramesYUV = {"resize_yuv", "planar YUV", "resize_yuv: null buffer", true, 0, plan_planar<1>, launch_yuv<true, false>};
const FrameFormat kFramesP016 = {"resize_p016", "P016", "resize_p016: null buffer", true, 1, plan_semi_planar<2>, launch_yuv<false, true>};
const FrameFormat kFramesYUV16 = {"resize_yuv16", "planar 16-bit YUV", "resize_yuv16: null buffer", true, 1, plan_planar<2>, launch_yuv<true, true>};
const FrameFormat kFramesYUY2 = {"resize_yuy2", "packed 4:2:2", "resize_yuy2: null buffer", true, 0, plan_packed422<1>, launch_packed422<false>};
const FrameFormat kFramesY210 = {"resize_y210", "packed 16-bit 4:2:2", "resize_y210: null buffer", true, 1, plan_packed422<2>, launch_packed422<true>};
const FrameFormat kFramesBGRA = {"resize_bgra", "packed 4:4:4", "resize_bgra: null buffer", true, 0, plan_packed444<1>, launch_packed444<false>};
const FrameFormat kFramesY410 = {"resize_y410", "packed 16-bit 4:4:4", "resize_y410: null buffer", true, 1, plan_packed444<2>, launch_packed444<true>};

// One resize in front of a forward: the frames in HBM and the descriptors + tables (c->rz_words) in pinned memory.
struct FrameJob {
    const FrameFormat& fmt;
    const uint8_t* frames_dev;
    const uint32_t* plan_host;   // pinned; stays untouched until the upload below has run
    size_t words;
    int max_tiles;
};

// checks the descriptors of one call and builds its plan in c->rz_words; nothing is enqueued
int frames_plan(vh_ctx* c, const FrameFormat& fmt, const void* desc, int batch, size_t nbytes, uintptr_t base, int* max_tiles) {
    if (!desc) return fail(&c->err, VH_ERR_INVALID, "null frame descriptors");
    if (fmt.three_channels && c->cfg.channels != 3)
        return fail(&c->err, VH_ERR_INVALID, "%s frames need a model with 3 channels, this one has %d", fmt.label, c->cfg.channels);
    const int site = fmt.colour < 0 ? 0 : c->colour[fmt.colour].site;
    const char* why = fmt.plan(desc, batch, c->cfg.channels, c->cfg.image_size, nbytes, base, site, &c->rz_words, max_tiles);
    if (why) return fail(&c->err, VH_ERR_INVALID, "%s", why);
    return VH_OK;
}

// grow-only: the resized images (once), and room for `plan_words` words in HBM (and, host_too, in the context's pinned staging)
// and for `frame_bytes` of staged host frames.  A buffer is replaced only after the stream that may still read it has drained.
int frames_reserve(vh_ctx* c, size_t plan_words, bool host_too, size_t frame_bytes) {
    const vh_config& f = c->cfg;
    if (!c->rz_u8) HIPCHK(&c->err, hipMalloc((void**)&c->rz_u8, (size_t)f.max_batch * f.image_size * f.image_size * f.channels));
    if (plan_words > c->rz_plan_dev_cap) {
        HIPCHK(&c->err, sync_compute(c));
        if (c->rz_plan_dev) hipFree(c->rz_plan_dev);
        c->rz_plan_dev = nullptr; c->rz_plan_dev_cap = 0;
        const size_t cap = plan_words * 2 > 16384 ? plan_words * 2 : 16384;
        HIPCHK(&c->err, hipMalloc((void**)&c->rz_plan_dev, cap * 4));
        c->rz_plan_dev_cap = cap;
    }
    if (host_too && plan_words > c->rz_plan_host_cap) {
        HIPCHK(&c->err, sync_compute(c));
        if (c->rz_plan_host) hipHostFree(c->rz_plan_host);
        c->rz_plan_host = nullptr; c->rz_plan_host_cap = 0;
        const size_t cap = plan_words * 2 > 16384 ? plan_words * 2 : 16384;
        HIPCHK(&c->err, hipHostMalloc((void**)&c->rz_plan_host, cap * 4, hipHostMallocDefault));
        c->rz_plan_host_cap = cap;
    }
    if (frame_bytes > c->rz_frames_cap) {
        HIPCHK(&c->err, sync_compute(c));
        if (c->rz_frames) hipFree(c->rz_frames);
        c->rz_frames = nullptr; c->rz_frames_cap = 0;
        const size_t cap = frame_bytes + frame_bytes / 2;
        HIPCHK(&c->err, hipMalloc((void**)&c->rz_frames, cap));
        c->rz_frames_cap = cap;
    }
    return VH_OK;
}

// plan upload + the one resize launch, on the context's stream (ahead of the fork of vh_set_streams); c->rz_u8 then holds the
// batch the forward reads.  Stage "resize" of vh_set_stage_timing brackets the launch.
int enqueue_resize(vh_ctx* c, const FrameJob& j, int batch) {
    auto tmark = [&]() -> int { return c->timing_stage == ST_RESIZE ? record_next(c, c->tev, c->tev_used, c->stream) : VH_OK; };
    int rc;
    HIPCHK(&c->err, hipMemcpyAsync(c->rz_plan_dev, j.plan_host, j.words * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = tmark())) return rc;
    HIPCHK(&c->err, j.fmt.launch(j.frames_dev, c->rz_plan_dev, batch, c->cfg.channels, c->cfg.image_size, j.max_tiles,
                                 j.fmt.colour < 0 ? nullptr : c->colour[j.fmt.colour].m, c->rz_u8, c->stream));
    return tmark();
}

// the bodies of vh_forward_device_async / vh_forward_device / vh_forward for either kind of input; `job`: the resize that
// fills `in` (= c->rz_u8) first
int forward_device_async(vh_ctx* c, ImgIn in, int batch, float* logits, int steps, const FrameJob* job = nullptr) {
    int rc = check_forward_args(c, in.p, batch, logits);
    if (rc) return rc;
    if (steps <= 0) return fail(&c->err, VH_ERR_INVALID, "steps must be positive");
    HIPCHK(&c->err, hipSetDevice(c->device));
    c->tev_used = 0;
    c->sev_used = 0;
    auto step_mark = [&]() -> int { return c->step_timing ? record_next(c, c->sev, c->sev_used, c->stream) : VH_OK; };
    HIPCHK(&c->err, hipEventRecord(c->ev0, c->stream));
    if ((rc = step_mark())) return rc;
    if (job && (rc = enqueue_resize(c, *job, batch))) return rc;
    // Steps do not depend on each other: even ones run on c->stream with buffer set 0, odd ones on the second stream with set 1.
    // The second stream starts behind everything the caller (and the resize) put on c->stream, and c->stream ends behind it, so
    // ev1, vh_synchronize and whatever the caller enqueues next see every step finished.  Every step writes the caller's
    // logits: the final LayerNorm + head of step i wait for the head of step i - 1 (about 0.2 % of a forward), which keeps the
    // writes in step order.
    const bool two = steps > 1 && two_in_flight(c);
    if (two) {
        c->s2_open = true;   // (until the join below: an error return in between leaves the second stream to sync_compute)
        HIPCHK(&c->err, hipEventRecord(c->ev_fork2, c->stream));
        HIPCHK(&c->err, hipStreamWaitEvent(c->stream2, c->ev_fork2, 0));
    }
    for (int i = 0; i < steps; ++i) {
        const int set = two ? i & 1 : 0;
        if ((rc = run_step(c, in, batch, logits, set, two && i > 0 ? c->ev_head[set ^ 1] : nullptr))) return rc;
        if (two) HIPCHK(&c->err, hipEventRecord(c->ev_head[set], set ? c->stream2 : c->stream));
        if ((rc = step_mark())) return rc;
    }
    if (two) {
        HIPCHK(&c->err, hipEventRecord(c->ev_join2, c->stream2));
        HIPCHK(&c->err, hipStreamWaitEvent(c->stream, c->ev_join2, 0));
        c->s2_open = false;
    }
    HIPCHK(&c->err, hipEventRecord(c->ev1, c->stream));
    c->timed = true;
    return VH_OK;
}

int forward_device(vh_ctx* c, ImgIn in, int batch, float* logits, const FrameJob* job = nullptr) {
    const auto t0 = std::chrono::high_resolution_clock::now();
    int rc = forward_device_async(c, in, batch, logits, 1, job);
    if (rc) return rc;
    rc = vh_synchronize(c);
    if (rc) return rc;
    c->last_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - t0).count();
    return VH_OK;
}

// `job`: in_host holds `frame_bytes` of frames, staged in c->rz_frames (= job->frames_dev) and resized into c->rz_u8
int forward_host(vh_ctx* c, ImgIn in_host, int batch, float* logits_host, const FrameJob* job = nullptr, size_t frame_bytes = 0) {
    int rc = check_forward_args(c, in_host.p, batch, logits_host);
    if (rc) return rc;
    const vh_config& f = c->cfg;
    // same timing window as the reference: H2D + device work + blocking D2H (netFPGA.cpp:262-284)
    const auto t0 = std::chrono::high_resolution_clock::now();
    HIPCHK(&c->err, hipSetDevice(c->device));
    const size_t in_bytes = job ? frame_bytes : (size_t)batch * f.image_size * f.image_size * f.channels * in_host.elem();
    const ImgIn staged = job ? ImgIn{c->rz_u8, kU8} : ImgIn{c->in_dev, in_host.kind, in_host.layout};
    HIPCHK(&c->err, hipMemcpyAsync(job ? (void*)c->rz_frames : (void*)c->in_dev, in_host.p, in_bytes, hipMemcpyHostToDevice, c->stream));
    rc = forward_device_async(c, staged, batch, c->logits_dev, 1, job);
    if (rc) return rc;
    HIPCHK(&c->err, hipMemcpyAsync(logits_host, c->logits_dev, (size_t)batch * f.classes * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, sync_compute(c));
    if (c->guard_auto && guard_exceeded(c)) {
        // this (synchronous) forward itself ran folded on rows beyond the guard: run it again, now with the stand-alone LayerNorm
        rc = forward_device_async(c, staged, batch, c->logits_dev, 1);   // (its run_step polls the guard and switches; resized frames are still in place)
        if (rc) return rc;
        HIPCHK(&c->err, hipMemcpyAsync(logits_host, c->logits_dev, (size_t)batch * f.classes * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(&c->err, sync_compute(c));
    }
    c->last_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - t0).count();
    return VH_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int vh_ring_destroy(vh_ctx* c);

int vh_abi_version(void) { return VH_ABI_VERSION; }

int vh_device_count(int* count) {
    if (!count) return fail(nullptr, VH_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(nullptr, VH_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return VH_OK;
}

const char* vh_last_error(const vh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int vh_malloc(int device, size_t nbytes, void** p) {
    if (!p || !nbytes) return fail(nullptr, VH_ERR_INVALID, "vh_malloc: bad argument");
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    HIPCHK(nullptr, hipMalloc(p, nbytes));
    return VH_OK;
}
int vh_free(int device, void* p) {
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    HIPCHK(nullptr, hipFree(p));
    return VH_OK;
}
int vh_memcpy_h2d(int device, void* d, const void* h, size_t n) {
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    HIPCHK(nullptr, hipMemcpy(d, h, n, hipMemcpyHostToDevice));
    return VH_OK;
}
int vh_memcpy_d2h(int device, void* h, const void* d, size_t n) {
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    HIPCHK(nullptr, hipMemcpy(h, d, n, hipMemcpyDeviceToHost));
    return VH_OK;
}
int vh_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes) {
    if (!free_bytes || !total_bytes) return fail(nullptr, VH_ERR_INVALID, "null argument");
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    HIPCHK(nullptr, hipMemGetInfo(free_bytes, total_bytes));
    return VH_OK;
}
int vh_device_synchronize(int device) {
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    HIPCHK(nullptr, hipDeviceSynchronize());
    return VH_OK;
}

size_t vh_weight_blob_bytes(const vh_config* cfg) {
    if (!cfg || check_config(*cfg)) return 0;
    return blob_bytes_of(*cfg);
}

int vh_create(const vh_config* cfg, int device, vh_ctx** out) {
    if (!cfg || !out) return fail(nullptr, VH_ERR_INVALID, "vh_create: null argument");
    *out = nullptr;
    if (const char* why = check_config(*cfg)) return fail(nullptr, VH_ERR_INVALID, "vh_create: %s", why);
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, VH_ERR_NO_DEVICE, "device %d is %s; libvithip is built for gfx950 only", device, prop.gcnArchName);

    vh_ctx* c = nullptr;
    try {
        c = new vh_ctx();
        c->cfg = *cfg;
        c->L = make_layout(*cfg);
    } catch (const std::exception& ex) {   // nothing may leave an extern "C" entry point as a C++ exception
        delete c;
        return fail(nullptr, VH_ERR_INVALID, "vh_create: %s", ex.what());
    }
    c->device = device;
    const Layout& L = c->L;
    const size_t D = cfg->dim, M = cfg->mlp_dim, M1 = (size_t)L.M1, C = cfg->classes, B = cfg->max_batch;   // M1: fc1's width (2 M with VH_FLAG_SWIGLU)
    auto bail = [&](int code) { vh_destroy(c); return code; };
#define CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fail(nullptr, VH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); return bail(VH_ERR_HIP); } } while (0)
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < vh_ctx::kMaxStreams - 1; ++i) {
        CK(hipStreamCreateWithFlags(&c->xstream[i], hipStreamNonBlocking));
        CK(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    {
        const char* e = getenv("VH_STREAMS");
        c->nstreams = e ? atoi(e) : 1;
        if (c->nstreams < 1) c->nstreams = 1;
        if (c->nstreams > vh_ctx::kMaxStreams) c->nstreams = vh_ctx::kMaxStreams;
    }
    CK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    CK(hipEventCreateWithFlags(&c->ev_fork2, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming));
    for (hipEvent_t& e : c->ev_head) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    {
        const char* e = getenv("VH_INFLIGHT");   // VH_INFLIGHT=1: one forward at a time, as before the second set existed (A/B runs)
        c->inflight_max = e && e[0] == '1' && !e[1] ? 1 : 2;
    }
    c->num_cu = prop.multiProcessorCount;
    {
        const char* e = getenv("VH_GRAPH");
        c->use_graph = e && e[0] == '1';
    }
    CK(hipEventCreate(&c->ev0));
    CK(hipEventCreate(&c->ev1));
    // canonical blob
    CK(hipMalloc((void**)&c->blob, sizeof(BlobHeader) + 4 * L.total));
    c->params = (float*)(c->blob + sizeof(BlobHeader));
    // the weight arena: offsets first; the layer records below, once it is allocated
    size_t w16_bytes = 0;
    auto carve16 = [&](size_t elems) { size_t o = w16_bytes; w16_bytes += align_up(elems * 2, 256); return o; };
    const size_t o_wp = carve16(D * L.KPA);
    struct MatOff { size_t qkv, o, fc1, fc2, fc2_t, o_t; };
    std::vector<MatOff> off(cfg->layers);
    const bool want_tiled_any = D % 256 == 0 && M % 256 == 0 && !(getenv("VH_H_TILED") && getenv("VH_H_TILED")[0] == '0');
    const bool want_tiled = cfg->dtype != VH_DTYPE_FP8 && want_tiled_any;
    const bool want_tiled8 = cfg->dtype == VH_DTYPE_FP8 && want_tiled_any;   // e4m3 operands: fc2's weights (bytes) in the tiled e4m3 layout
    for (auto& o : off) {
        o.qkv = carve16(3 * D * D); o.o = carve16(D * D); o.fc1 = carve16(M1 * D); o.fc2 = carve16(D * M);
        o.fc2_t = want_tiled ? carve16(D * M) : want_tiled8 ? carve16((D * M + 1) / 2) : 0;
    }
    for (auto& o : off) o.o_t = want_tiled ? carve16(D * D) : want_tiled8 ? carve16((D * D + 1) / 2) : 0;
    {
        // LayerNorm folded into the neighbouring GEMMs: a property of the MODEL SHAPE and of vh_config.flags only -- never of
        // max_batch, so that a context sized for 1 image and one sized for 512 give the same logit bits for the same image
        // (and hip::net_hip, which re-creates its context when a larger batch arrives, keeps its numerics).  On by default
        // where the shapes allow it.  VH_LN_FOLD=0 / 1 (environment, A/B tools) applies only when the flags leave the choice
        // to the library.
        const bool eligible = (cfg->dim % 256 == 0) && (cfg->mlp_dim % 256 == 0);
        bool want = true;
        if (cfg->flags & VH_FLAG_LN_FOLD_OFF) want = false;
        else if (!(cfg->flags & VH_FLAG_LN_FOLD_ON)) { const char* e = getenv("VH_LN_FOLD"); if (e) want = e[0] == '1'; }
        c->ln_fold = eligible && want;
        // the library's own default (no flag, no VH_LN_FOLD in the environment) is the GUARDED fold
        c->guard_auto = c->ln_fold && !(cfg->flags & (VH_FLAG_LN_FOLD_ON | VH_FLAG_LN_FOLD_OFF)) && !getenv("VH_LN_FOLD");
        if (const char* e = getenv("VH_LN_GUARD")) { const float t = (float)atof(e); if (t > 0.f) c->guard_thresh = t; }
    }
    c->fp8 = cfg->dtype == VH_DTYPE_FP8;
    c->dt16 = c->fp8 ? VH_DTYPE_BF16 : cfg->dtype;
    for (int i = 0; i < kMaxChannels; ++i) {   // 8-bit input: x = p / 255 until vh_set_input_norm says otherwise
        c->in_scale[i] = i < cfg->channels ? 1.0f / 255.0f : 0.f;
        c->in_shift[i] = 0.f;
    }
    yuv_matrix(VH_YUV_BT709, 0, c->colour[0].m);   // NV12 frames: what an HD video decoder emits, until vh_set_frame_colour says otherwise
    yuv_matrix16(VH_YUV_BT709, 0, 10, 1, c->colour[1].m);   // 16-bit frames: P010 as VCN writes it, until vh_set_frame_colour16 says otherwise
    {
        const char* e = getenv("VH_RESID_SPLIT");
        c->split = c->ln_fold && !(e && e[0] == '0');
        c->ln_fold_cfg = c->ln_fold;
        c->split_cfg = c->split;
        c->cls_tail = (cfg->flags & VH_FLAG_CLS_TAIL) != 0;
        c->head_dim = cfg->dim / cfg->heads;
        c->q_scale = attention_q_scale(c->head_dim);
        c->h_tiled = want_tiled || want_tiled8;
        { const char* e = getenv("VH_ATT_TILED"); c->att_tiled = !(e && e[0] == '0'); }
        { const char* e = getenv("VH_QKV_HM"); c->qkv_hm = !(e && e[0] == '0'); }
        { const char* e = getenv("VH_SWIGLU_SKIP"); c->swiglu_skip = e && e[0] == '1'; }
    }
    CK(hipHostMalloc((void**)&c->guard_host, 64, hipHostMallocDefault));
    *c->guard_host = 0.f;
    // per layer: the fold constants c_qkv[3D] d_qkv[3D] c_fc1[M1] d_fc1[M1]; on fp8 contexts the scales s_qkv[3D] s_o[D] s_fc1[M1] s_fc2[D]
    const size_t cd_per_layer = 6 * D + 2 * M1, sc_per_layer = 5 * D + M1, nl = cfg->layers;   // in floats = two 16-bit elements
    const size_t o_bqkv = carve16(nl * 3 * D * 2), o_cd = carve16(nl * cd_per_layer * 2), o_sc = c->fp8 ? carve16(nl * sc_per_layer * 2) : 0;
    CK(hipMalloc((void**)&c->w16, w16_bytes));
    c->wp16 = c->w16 + o_wp;
    c->layer.resize(cfg->layers);
    for (int l = 0; l < cfg->layers; ++l) {
        LayerW& w = c->layer[l];
        const MatOff& o = off[l];
        w.qkv = c->w16 + o.qkv; w.o = c->w16 + o.o; w.fc1 = c->w16 + o.fc1; w.fc2 = c->w16 + o.fc2;
        if (want_tiled || want_tiled8) { w.fc2_t = c->w16 + o.fc2_t; w.o_t = c->w16 + o.o_t; }
        w.bqkv = (float*)(c->w16 + o_bqkv) + (size_t)l * 3 * D;
        w.c_qkv = (float*)(c->w16 + o_cd) + (size_t)l * cd_per_layer;
        w.d_qkv = w.c_qkv + 3 * D; w.c_fc1 = w.d_qkv + 3 * D; w.d_fc1 = w.c_fc1 + M1;
        if (c->fp8) {
            w.s_qkv = (float*)(c->w16 + o_sc) + (size_t)l * sc_per_layer;
            w.s_o = w.s_qkv + 3 * D; w.s_fc1 = w.s_o + D; w.s_fc2 = w.s_fc1 + M1;
        }
    }
    // activation arena: buffer set 0 (the table serves the second set too), then what both sets share
    size_t a = c->act_bytes = bind_set(c, nullptr, nullptr);
    auto carve = [&](size_t bytes) { size_t o = a; a += align_up(bytes, 256); return o; };
    const size_t o_in = carve(B * (size_t)cfg->image_size * cfg->image_size * cfg->channels * 4), o_lg = carve(B * C * 4),
                 o_gd = carve(256);     // the LayerNorm-fold guard word
    CK(hipMalloc((void**)&c->arena, a));
    c->guard_dev = (unsigned int*)(c->arena + o_gd);
    CK(hipMemsetAsync(c->guard_dev, 0, 256, c->stream));
    bind_set(c, &c->act[0], c->arena);
    c->in_dev = (float*)(c->arena + o_in); c->logits_dev = (float*)(c->arena + o_lg);
#undef CK
    *out = c;
    return VH_OK;
}

int vh_destroy(vh_ctx* c) {
    if (!c) return VH_OK;
    hipSetDevice(c->device);
    vh_ring_destroy(c);
    if (c->stream) sync_compute(c);
    drop_graphs(c);
    if (c->guard_host) hipHostFree(c->guard_host);
    if (c->rz_plan_host) hipHostFree(c->rz_plan_host);
    if (c->rz_plan_dev) hipFree(c->rz_plan_dev);
    if (c->rz_frames) hipFree(c->rz_frames);
    if (c->rz_u8) hipFree(c->rz_u8);
    if (c->arena) hipFree(c->arena);
    if (c->act[1].base) hipFree(c->act[1].base);
    if (c->feat_store) hipFree(c->feat_store);
    if (c->attn_store) hipFree(c->attn_store);
    if (c->w16) hipFree(c->w16);
    if (c->blob) hipFree(c->blob);
    for (hipEvent_t e : c->tev) hipEventDestroy(e);
    for (hipEvent_t e : c->sev) hipEventDestroy(e);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    for (int i = 0; i < vh_ctx::kMaxStreams - 1; ++i) {
        if (c->xstream[i]) { hipStreamSynchronize(c->xstream[i]); hipStreamDestroy(c->xstream[i]); }
        if (c->ev_join[i]) hipEventDestroy(c->ev_join[i]);
    }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_fork2) hipEventDestroy(c->ev_fork2);
    if (c->ev_join2) hipEventDestroy(c->ev_join2);
    for (hipEvent_t e : c->ev_head) if (e) hipEventDestroy(e);
    if (c->stream2) hipStreamDestroy(c->stream2);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return VH_OK;
}

int vh_get_config(const vh_ctx* c, vh_config* out) {
    if (!c || !out) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *out = c->cfg;
    return VH_OK;
}

int vh_get_register_tokens(const vh_ctx* c) { return c ? c->L.R : -1; }
int vh_get_ln_fold(const vh_ctx* c, int* on) {
    if (!c || !on) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *on = c->ln_fold ? 1 : 0;
    return VH_OK;
}

int vh_get_ln_guard(vh_ctx* c, float* max_ratio, float* threshold, int* tripped) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    float seen[2] = {0.f, 0.f};
    HIPCHK(&c->err, hipMemcpy(seen, c->guard_dev, sizeof seen, hipMemcpyDeviceToHost));
    if ((!(seen[0] <= c->guard_thresh) || (c->fp8 && !(seen[1] <= kE4M3Max))) && c->ln_fold_cfg) c->guard_tripped = true;
    if (max_ratio) *max_ratio = seen[0];
    if (threshold) *threshold = c->guard_thresh;
    if (tripped) *tripped = c->guard_tripped ? 1 : 0;
    return VH_OK;
}

int vh_get_fp8_guard(vh_ctx* c, float* max_abs, float* limit) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    float seen[2] = {0.f, 0.f};
    HIPCHK(&c->err, hipMemcpy(seen, c->guard_dev, sizeof seen, hipMemcpyDeviceToHost));
    if (max_abs) *max_abs = c->fp8 ? seen[1] : 0.f;
    if (limit) *limit = kE4M3Max;
    return VH_OK;
}

int vh_load_weights(vh_ctx* c, const void* host_blob, size_t nbytes) {
    if (!c || !host_blob) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "vh_load_weights: null argument");
    const size_t need = sizeof(BlobHeader) + 4 * c->L.total;
    if (nbytes != need) return fail(&c->err, VH_ERR_INVALID, "weight blob is %zu bytes, expected %zu", nbytes, need);
    BlobHeader h;
    memcpy(&h, host_blob, sizeof h);
    int rc = check_blob_header(c, h);
    if (rc) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    c->weights_ready = false;
    HIPCHK(&c->err, hipMemcpyAsync(c->blob, host_blob, nbytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = guard_reset(c))) return rc;
    if ((rc = prepare_weights(c))) return rc;
    return guard_calibrate(c);
}

int vh_load_weights_device(vh_ctx* c, const void* dev_blob, size_t nbytes) {
    if (!c || !dev_blob) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "vh_load_weights_device: null argument");
    const size_t need = sizeof(BlobHeader) + 4 * c->L.total;
    if (nbytes != need) return fail(&c->err, VH_ERR_INVALID, "weight blob is %zu bytes, expected %zu", nbytes, need);
    HIPCHK(&c->err, hipSetDevice(c->device));
    BlobHeader h;
    HIPCHK(&c->err, hipMemcpy(&h, dev_blob, sizeof h, hipMemcpyDeviceToHost));
    int rc = check_blob_header(c, h);
    if (rc) return rc;
    c->weights_ready = false;
    if (dev_blob != c->blob) HIPCHK(&c->err, hipMemcpyAsync(c->blob, dev_blob, nbytes, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = guard_reset(c))) return rc;
    if ((rc = prepare_weights(c))) return rc;
    return guard_calibrate(c);
}

int vh_init_weights_seeded(vh_ctx* c, uint64_t seed) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    HIPCHK(&c->err, hipSetDevice(c->device));
    const vh_config& f = c->cfg;
    const Layout& L = c->L;
    BlobHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, "VHBLOB1", 8);
    h.image_size = f.image_size; h.patch_size = f.patch_size; h.channels = f.channels; h.dim = f.dim;
    h.heads = f.heads; h.mlp_dim = f.mlp_dim; h.layers = f.layers; h.classes = f.classes; h.ln_eps = f.ln_eps;
    h.flags = blob_model_bits(f);
    c->weights_ready = false;
    HIPCHK(&c->err, hipMemcpy(c->blob, &h, sizeof h, hipMemcpyHostToDevice));
    const size_t D = f.dim, M = f.mlp_dim, C = f.classes;
    const float sw = 0.02f, sb = 0.02f, sg = 0.05f;
    float* P = c->params;
    hipStream_t s = c->stream;
#define GEN(off, count, tid, sigma, offs) HIPCHK(&c->err, launch_fill(P + (off), (int64_t)(count), seed, (tid), 1, (sigma), (offs), s))
    GEN(L.patch_w, D * L.KP, TID_PATCH_W, sw, 0.f);
    GEN(L.patch_b, D, TID_PATCH_B, sb, 0.f);
    if (L.ncls) GEN(L.cls, D, TID_CLS, sw, 0.f);
    GEN(L.pos, (size_t)(L.NP + L.ncls) * D, TID_POS, sw, 0.f);
    if (L.R) GEN(L.reg, (size_t)L.R * D, TID_REG, sw, 0.f);
    if (f.flags & VH_FLAG_PRE_LN) { GEN(L.prew, D, TID_PRE_LN_W, sg, 1.f); GEN(L.preb, D, TID_PRE_LN_B, sb, 0.f); }
    for (int l = 0; l < f.layers; ++l) {
        const LayerOff& o = L.layer[l];
        const uint32_t t = TID_LAYER0 + 16u * (uint32_t)l;
        GEN(o.ln1w, D, t + 0, sg, 1.f); GEN(o.ln1b, D, t + 1, sb, 0.f);
        GEN(o.qw, D * D, t + 2, sw, 0.f); GEN(o.qb, D, t + 3, sb, 0.f);
        GEN(o.kw, D * D, t + 4, sw, 0.f); GEN(o.kb, D, t + 5, sb, 0.f);
        GEN(o.vw, D * D, t + 6, sw, 0.f); GEN(o.vb, D, t + 7, sb, 0.f);
        GEN(o.ow, D * D, t + 8, sw, 0.f); GEN(o.ob, D, t + 9, sb, 0.f);
        GEN(o.ln2w, D, t + 10, sg, 1.f); GEN(o.ln2b, D, t + 11, sb, 0.f);
        GEN(o.f1w, (size_t)L.M1 * D, t + 12, sw, 0.f); GEN(o.f1b, (size_t)L.M1, t + 13, sb, 0.f);   // (VH_FLAG_SWIGLU: 2 M rows, same tensor ids)
        GEN(o.f2w, D * M, t + 14, sw, 0.f); GEN(o.f2b, D, t + 15, sb, 0.f);
    }
    GEN(L.lnfw, D, TID_FINAL + 0, sg, 1.f); GEN(L.lnfb, D, TID_FINAL + 1, sb, 0.f);
    GEN(L.headw, C * (size_t)L.HW, TID_FINAL + 2, sw, 0.f); GEN(L.headb, C, TID_FINAL + 3, sb, 0.f);
    if (L.map) {
        GEN(L.map_qk, (size_t)f.heads * D, TID_MAP + 0, sw, 0.f);
        GEN(L.map_vw, D * D, TID_MAP + 1, sw, 0.f); GEN(L.map_vb, D, TID_MAP + 2, sb, 0.f);
        GEN(L.map_ow, D * D, TID_MAP + 3, sw, 0.f); GEN(L.map_ob, D, TID_MAP + 4, sb, 0.f);
        GEN(L.map_lnw, D, TID_MAP + 5, sg, 1.f); GEN(L.map_lnb, D, TID_MAP + 6, sb, 0.f);
        GEN(L.map_f1w, M * D, TID_MAP + 7, sw, 0.f); GEN(L.map_f1b, M, TID_MAP + 8, sb, 0.f);
        GEN(L.map_f2w, D * M, TID_MAP + 9, sw, 0.f); GEN(L.map_f2b, D, TID_MAP + 10, sb, 0.f);
    }
#undef GEN
    if (L.rope) {
        // angles of the generator's uniform stream, a = pi u; the tables are their cosine and sine, made on the host in double and
        // rounded once (the device holds no trigonometry): a synthetic model is a true rotation
        const size_t n = (size_t)L.NP * (size_t)(c->head_dim / 2);
        std::vector<float> cs(2 * n);
        const uint64_t stream = rng_stream(seed, TID_ROPE);
        for (size_t i = 0; i < n; ++i) {
            const double a = 3.14159265358979323846 * (double)rng_uniform(stream, i);
            cs[i] = (float)cos(a);
            cs[n + i] = (float)sin(a);
        }
        HIPCHK(&c->err, hipMemcpyAsync(P + L.rope_cos, cs.data(), n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(&c->err, hipMemcpyAsync(P + L.rope_sin, cs.data() + n, n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(&c->err, hipStreamSynchronize(s));   // cs leaves scope
    }
    if (int rc = guard_reset(c)) return rc;
    if (int rc = prepare_weights(c)) return rc;
    return guard_calibrate(c);
}

int vh_export_weights(vh_ctx* c, void* host_blob, size_t nbytes) {
    if (!c || !host_blob) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (!c->weights_ready) return fail(&c->err, VH_ERR_STATE, "no weights loaded");
    const size_t need = sizeof(BlobHeader) + 4 * c->L.total;
    if (nbytes != need) return fail(&c->err, VH_ERR_INVALID, "buffer is %zu bytes, blob is %zu", nbytes, need);
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, hipMemcpy(host_blob, c->blob, need, hipMemcpyDeviceToHost));
    return VH_OK;
}

// ---- weight blob on disk ---------------------------------------------------------------------
// The file IS the canonical blob (64-byte header + fp32 tensors in the fixed order of make_layout), with a
// checksum of the parameter bytes in the header words a memory blob leaves zero.  It is what vh_load_weights
// takes, what vh_export_weights returns and what the multi-GPU path broadcasts.
static int blob_file_header(const char* path, vh_config* cfg, size_t* need_out) {
    FILE* f = fopen(path, "rb");
    if (!f) return fail(nullptr, VH_ERR_INVALID, "cannot open %s", path);
    BlobHeader h;
    const size_t got = fread(&h, 1, sizeof h, f);
    long long fsize = -1;
    if (fseek(f, 0, SEEK_END) == 0) fsize = ftell(f);
    fclose(f);
    if (got != sizeof h || memcmp(h.magic, "VHBLOB1", 8) != 0) return fail(nullptr, VH_ERR_INVALID, "%s: not a VHBLOB1 file", path);
    vh_config c;
    memset(&c, 0, sizeof c);
    c.image_size = h.image_size; c.patch_size = h.patch_size; c.channels = h.channels; c.dim = h.dim; c.heads = h.heads;
    c.mlp_dim = h.mlp_dim; c.layers = h.layers; c.classes = h.classes; c.ln_eps = h.ln_eps;
    c.dtype = VH_DTYPE_BF16; c.max_batch = 1;
    if (h.flags & ~(kBlobSum | kBlobModelBits)) return fail(nullptr, VH_ERR_INVALID, "%s: unknown bits in the header's flags word", path);
    c.flags = blob_model_flags(h.flags);
    // check_config bounds every field, so the size arithmetic below cannot overflow and nothing is allocated from the header
    if (const char* why = check_config(c)) return fail(nullptr, VH_ERR_INVALID, "%s: header describes an unsupported model (%s)", path, why);
    const size_t need = blob_bytes_of(c);
    if (fsize != (long long)need) return fail(nullptr, VH_ERR_INVALID, "%s: %lld bytes, the header implies %zu", path, fsize, need);
    *cfg = c;
    if (need_out) *need_out = need;
    return VH_OK;
}

int vh_blob_file_config(const char* path, vh_config* cfg) {
    if (!path || !cfg) return fail(nullptr, VH_ERR_INVALID, "null argument");
    return blob_file_header(path, cfg, nullptr);
}

int vh_blob_file_read(const char* path, void* host_blob, size_t nbytes) {
    if (!path || !host_blob) return fail(nullptr, VH_ERR_INVALID, "null argument");
    vh_config c;
    size_t need = 0;
    int rc = blob_file_header(path, &c, &need);
    if (rc) return rc;
    if (nbytes != need) return fail(nullptr, VH_ERR_INVALID, "%s is %zu bytes, the buffer %zu", path, need, nbytes);
    FILE* f = fopen(path, "rb");
    if (!f) return fail(nullptr, VH_ERR_INVALID, "cannot open %s", path);
    const size_t got = fread(host_blob, 1, need, f);
    fclose(f);
    if (got != need) return fail(nullptr, VH_ERR_INVALID, "%s: short read", path);
    BlobHeader h;
    memcpy(&h, host_blob, sizeof h);
    if (h.flags & kBlobSum) {
        const uint64_t sum = fnv1a64((const char*)host_blob + sizeof h, need - sizeof h);
        if ((uint32_t)sum != h.sum_lo || (uint32_t)(sum >> 32) != h.sum_hi)
            return fail(nullptr, VH_ERR_INVALID, "%s: checksum mismatch (file damaged)", path);
    }
    h.sum_lo = h.sum_hi = 0;   // memory form: the model bits stay
    h.flags &= kBlobModelBits;
    h.pad[0] = h.pad[1] = 0;
    memcpy(host_blob, &h, sizeof h);
    return VH_OK;
}

int vh_save_weights_file(vh_ctx* c, const char* path) {
    if (!c || !path) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (!c->weights_ready) return fail(&c->err, VH_ERR_STATE, "no weights loaded");
    const size_t need = sizeof(BlobHeader) + 4 * c->L.total;
    std::vector<char> buf(need);
    int rc = vh_export_weights(c, buf.data(), need);
    if (rc) return rc;
    BlobHeader h;
    memcpy(&h, buf.data(), sizeof h);
    const uint64_t sum = fnv1a64(buf.data() + sizeof h, need - sizeof h);
    h.sum_lo = (uint32_t)sum; h.sum_hi = (uint32_t)(sum >> 32); h.flags = kBlobSum | blob_model_bits(c->cfg); h.pad[0] = h.pad[1] = 0;
    memcpy(buf.data(), &h, sizeof h);
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(&c->err, VH_ERR_INVALID, "cannot create %s", tmp.c_str());
    const size_t put = fwrite(buf.data(), 1, need, f);
    const int bad = fclose(f);
    if (put != need || bad) { remove(tmp.c_str()); return fail(&c->err, VH_ERR_INVALID, "short write to %s", tmp.c_str()); }
    if (rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); return fail(&c->err, VH_ERR_INVALID, "cannot rename %s to %s", tmp.c_str(), path); }
    return VH_OK;
}

int vh_load_weights_file(vh_ctx* c, const char* path) {
    if (!c || !path) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    const size_t need = sizeof(BlobHeader) + 4 * c->L.total;
    FILE* f = fopen(path, "rb");
    if (!f) return fail(&c->err, VH_ERR_INVALID, "cannot open %s", path);
    std::vector<char> buf(need + 1);
    const size_t got = fread(buf.data(), 1, need + 1, f);
    fclose(f);
    if (got != need) return fail(&c->err, VH_ERR_INVALID, "%s holds %s%zu bytes, this model's blob is %zu", path, got > need ? "more than " : "", got > need ? need : got, need);
    BlobHeader h;
    memcpy(&h, buf.data(), sizeof h);
    int rc = check_blob_header(c, h);
    if (rc) return rc;
    if (h.flags & kBlobSum) {
        const uint64_t sum = fnv1a64(buf.data() + sizeof h, need - sizeof h);
        if ((uint32_t)sum != h.sum_lo || (uint32_t)(sum >> 32) != h.sum_hi)
            return fail(&c->err, VH_ERR_INVALID, "%s: checksum mismatch (file damaged)", path);
    }
    // the resident blob is the memory form: checksum words cleared, so export == what make_blob-style writers produce
    h.sum_lo = h.sum_hi = 0;
    h.flags &= kBlobModelBits;
    memcpy(buf.data(), &h, sizeof h);
    return vh_load_weights(c, buf.data(), need);
}

int vh_export_weights_device(vh_ctx* c, void* dev_blob, size_t nbytes) {
    if (!c || !dev_blob) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (!c->weights_ready) return fail(&c->err, VH_ERR_STATE, "no weights loaded");
    const size_t need = sizeof(BlobHeader) + 4 * c->L.total;
    if (nbytes != need) return fail(&c->err, VH_ERR_INVALID, "buffer is %zu bytes, blob is %zu", nbytes, need);
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, hipMemcpy(dev_blob, c->blob, need, hipMemcpyDeviceToDevice));
    return VH_OK;
}

int vh_forward_device_async(vh_ctx* c, const float* in, int batch, float* logits, int steps) {
    return forward_device_async(c, ImgIn{in}, batch, logits, steps);
}

int vh_forward_device_u8_async(vh_ctx* c, const uint8_t* in, int batch, float* logits, int steps) {
    if (int rc = check_u8_ptr(c, in)) return rc;
    return forward_device_async(c, ImgIn{in, kU8}, batch, logits, steps);
}

int vh_synchronize(vh_ctx* c) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    // everything enqueued has completed: if one of those forwards tripped the fold's guard, switch NOW rather than at the
    // next forward's entry (vh_get_ln_guard reports it; the results already delivered came from the folded path)
    if (c->weights_ready) return guard_poll(c);
    return VH_OK;
}

int vh_forward_device(vh_ctx* c, const float* in, int batch, float* logits) { return forward_device(c, ImgIn{in}, batch, logits); }

int vh_forward_device_u8(vh_ctx* c, const uint8_t* in, int batch, float* logits) {
    if (int rc = check_u8_ptr(c, in)) return rc;
    return forward_device(c, ImgIn{in, kU8}, batch, logits);
}

int vh_forward(vh_ctx* c, const float* in_host, int batch, float* logits_host) { return forward_host(c, ImgIn{in_host}, batch, logits_host); }

int vh_forward_u8(vh_ctx* c, const uint8_t* in_host, int batch, float* logits_host) { return forward_host(c, ImgIn{in_host, kU8}, batch, logits_host); }

// Image tensors: the forward entry points for any (element type, layout)
int vh_forward_device_tensor_async(vh_ctx* c, const void* in, int elem, int layout, int batch, float* logits, int steps) {
    if (int rc = check_tensor_kind(c ? &c->err : nullptr, elem, layout)) return rc;
    if (int rc = check_tensor_ptr(c, in)) return rc;
    return forward_device_async(c, ImgIn{in, elem, layout}, batch, logits, steps);
}
int vh_forward_device_tensor(vh_ctx* c, const void* in, int elem, int layout, int batch, float* logits) {
    if (int rc = check_tensor_kind(c ? &c->err : nullptr, elem, layout)) return rc;
    if (int rc = check_tensor_ptr(c, in)) return rc;
    return forward_device(c, ImgIn{in, elem, layout}, batch, logits);
}
int vh_forward_tensor(vh_ctx* c, const void* in_host, int elem, int layout, int batch, float* logits_host) {
    if (int rc = check_tensor_kind(c ? &c->err : nullptr, elem, layout)) return rc;
    return forward_host(c, ImgIn{in_host, elem, layout}, batch, logits_host);
}

// Frames of any format: check + plan on the host (nothing enqueued on a refusal), then resize -> u8 forward on the context's stream.
// The plan sees the device address, because the alignment of the frames decides which loads the kernel may use.
static int forward_frames_device(vh_ctx* c, const FrameFormat& fmt, const uint8_t* frames_dev, size_t nbytes, const void* desc, int batch,
                                 float* logits_dev) {
    int rc = check_forward_args(c, frames_dev, batch, logits_dev);
    if (rc) return rc;
    int max_tiles = 0;
    if ((rc = frames_plan(c, fmt, desc, batch, nbytes, (uintptr_t)frames_dev, &max_tiles))) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    if ((rc = frames_reserve(c, c->rz_words.size(), true, 0))) return rc;
    memcpy(c->rz_plan_host, c->rz_words.data(), c->rz_words.size() * 4);
    const FrameJob job{fmt, frames_dev, c->rz_plan_host, c->rz_words.size(), max_tiles};
    return forward_device(c, ImgIn{c->rz_u8, kU8}, batch, logits_dev, &job);
}

// the same from host memory: the frames are staged in c->rz_frames, whose base (hipMalloc) is aligned for any sample: base 0
static int forward_frames_host(vh_ctx* c, const FrameFormat& fmt, const uint8_t* frames_host, size_t nbytes, const void* desc, int batch,
                               float* logits_host) {
    int rc = check_forward_args(c, frames_host, batch, logits_host);
    if (rc) return rc;
    int max_tiles = 0;
    if ((rc = frames_plan(c, fmt, desc, batch, nbytes, 0, &max_tiles))) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    if ((rc = frames_reserve(c, c->rz_words.size(), true, nbytes))) return rc;
    memcpy(c->rz_plan_host, c->rz_words.data(), c->rz_words.size() * 4);
    const FrameJob job{fmt, c->rz_frames, c->rz_plan_host, c->rz_words.size(), max_tiles};
    return forward_host(c, ImgIn{frames_host, kU8}, batch, logits_host, &job, nbytes);
}

// 8-bit interleaved frames (kernels_resize.hip)
int vh_forward_device_frames_u8(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesRGB, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_u8(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesRGB, frames_host, nbytes, desc, batch, logits_host);
}
// NV12 frames: the plan of resize_plan_build_nv12 (both planes + the colour matrix in one launch)
int vh_forward_device_frames_nv12(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesNV12, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_nv12(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesNV12, frames_host, nbytes, desc, batch, logits_host);
}
// planar YUV frames: the plan of resize_plan_build_yuv
int vh_forward_device_frames_yuv(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesYUV, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_yuv(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesYUV, frames_host, nbytes, desc, batch, logits_host);
}
// 16-bit YUV frames: the same two descriptor types and planners, the uint16_t instantiations of the kernel, the second colour state
int vh_forward_device_frames_p016(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesP016, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_p016(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesP016, frames_host, nbytes, desc, batch, logits_host);
}
int vh_forward_device_frames_yuv16(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesYUV16, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_yuv16(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesYUV16, frames_host, nbytes, desc, batch, logits_host);
}
// packed 4:2:2 frames: the plan of resize_plan_build_yuy2; 8-bit layouts under the first colour state, Y210 / Y216 / v210 under the second
int vh_forward_device_frames_yuy2(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesYUY2, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_yuy2(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesYUY2, frames_host, nbytes, desc, batch, logits_host);
}
int vh_forward_device_frames_y210(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesY210, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_y210(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesY210, frames_host, nbytes, desc, batch, logits_host);
}
// packed 4:4:4 frames: the plan of resize_plan_build_bgra; 8-bit layouts under the first colour state (RGB layouts read none), Y416 /
// AYUV64 / Y410 / V410 under the second
int vh_forward_device_frames_bgra(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesBGRA, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_bgra(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesBGRA, frames_host, nbytes, desc, batch, logits_host);
}
int vh_forward_device_frames_y410(vh_ctx* c, const uint8_t* frames_dev, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_dev) {
    return forward_frames_device(c, kFramesY410, frames_dev, nbytes, desc, batch, logits_dev);
}
int vh_forward_frames_y410(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_host) {
    return forward_frames_host(c, kFramesY410, frames_host, nbytes, desc, batch, logits_host);
}

int vh_yuv_matrix(int standard, int full_range, float m[12]) {
    if (yuv_matrix(standard, full_range, m))
        return fail(nullptr, VH_ERR_INVALID, "yuv matrix: standard must be VH_YUV_BT601, _BT709 or _BT2020, full_range 0 or 1, m not NULL");
    return VH_OK;
}

int vh_yuv_matrix16(int standard, int full_range, int bits, int msb_aligned, float m[12]) {
    if (yuv_matrix16(standard, full_range, bits, msb_aligned, m))
        return fail(nullptr, VH_ERR_INVALID, "yuv matrix16: standard must be VH_YUV_BT601, _BT709 or _BT2020, full_range 0 or 1, bits 8..16, msb_aligned 0 or 1, m not NULL");
    return VH_OK;
}

// Colour matrix and chroma siting of one of the two colour states.  The resize runs outside the captured graph and takes the matrix
// by value at each launch: no graph to drop, nothing in flight to wait for.  m NULL: `dflt`, left siting.  word: "" or "16-bit ".
static int set_frame_colour(vh_ctx* c, int which, const float m[12], int chroma_site, const float dflt[12], const char* word) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (m) {
        if (chroma_site != VH_CHROMA_CENTER && chroma_site != VH_CHROMA_LEFT) return fail(&c->err, VH_ERR_INVALID, "chroma_site %d is neither VH_CHROMA_CENTER nor VH_CHROMA_LEFT", chroma_site);
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(m[i])) return fail(&c->err, VH_ERR_INVALID, "%scolour matrix entry %d is not finite", word, i);
    }
    memcpy(c->colour[which].m, m ? m : dflt, sizeof c->colour[which].m);
    c->colour[which].site = m ? chroma_site : VH_CHROMA_LEFT;
    return VH_OK;
}

static int get_frame_colour(const vh_ctx* c, int which, float m[12], int* chroma_site) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (m) memcpy(m, c->colour[which].m, sizeof c->colour[which].m);
    if (chroma_site) *chroma_site = c->colour[which].site;
    return VH_OK;
}

// the state of the NV12 and planar YUV entry points; default: BT.709 limited range
int vh_set_frame_colour(vh_ctx* c, const float m[12], int chroma_site) {
    float dflt[12];
    yuv_matrix(VH_YUV_BT709, 0, dflt);
    return set_frame_colour(c, 0, m, chroma_site, dflt, "");
}
int vh_get_frame_colour(const vh_ctx* c, float m[12], int* chroma_site) { return get_frame_colour(c, 0, m, chroma_site); }

// The second colour state: matrix and siting of the 16-bit entry points, under the same rules; default: the same for P010.  Neither
// call touches the other's state.
int vh_set_frame_colour16(vh_ctx* c, const float m[12], int chroma_site) {
    float dflt[12];
    yuv_matrix16(VH_YUV_BT709, 0, 10, 1, dflt);
    return set_frame_colour(c, 1, m, chroma_site, dflt, "16-bit ");
}
int vh_get_frame_colour16(const vh_ctx* c, float m[12], int* chroma_site) { return get_frame_colour(c, 1, m, chroma_site); }

int vh_resize_table(int n_in, double lo, double hi, int n_out, int32_t* first, int32_t* count, float* weights, int max_taps) {
    if (resize_axis_table(n_in, lo, hi, n_out, first, count, weights, max_taps))
        return fail(nullptr, VH_ERR_INVALID, "resize table: bad argument, box outside 0..n_in or empty, scale > %d, or more than max_taps taps", kResizeMaxScale);
    return VH_OK;
}

// Input normalisation of the 8-bit entry points.  The constants travel to the im2col kernel as launch arguments, which a captured
// graph holds by value: like a weight load, a change waits for the stream and drops the cached graphs.
int vh_set_input_norm(vh_ctx* c, const float* scale, const float* shift) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if ((scale == nullptr) != (shift == nullptr)) return fail(&c->err, VH_ERR_INVALID, "scale and shift: give both, or NULL for both (the default)");
    const int ch = c->cfg.channels;
    for (int i = 0; scale && i < ch; ++i)
        if (!std::isfinite(scale[i]) || !std::isfinite(shift[i])) return fail(&c->err, VH_ERR_INVALID, "scale / shift of channel %d is not finite", i);
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    for (int i = 0; i < kMaxChannels; ++i) {
        c->in_scale[i] = i < ch ? (scale ? scale[i] : 1.0f / 255.0f) : 0.f;
        c->in_shift[i] = i < ch && shift ? shift[i] : 0.f;
    }
    drop_graphs(c);
    return VH_OK;
}

int vh_get_input_norm(const vh_ctx* c, float* scale, float* shift) {
    if (!c || !scale || !shift) return fail(nullptr, VH_ERR_INVALID, "null argument");
    for (int i = 0; i < c->cfg.channels; ++i) { scale[i] = c->in_scale[i]; shift[i] = c->in_shift[i]; }
    return VH_OK;
}

int vh_fill_input_seeded(vh_ctx* c, uint64_t seed, int batch, float* in_dev) {
    if (!c || !in_dev || batch <= 0) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "bad argument");
    HIPCHK(&c->err, hipSetDevice(c->device));
    const int64_t n = (int64_t)batch * c->cfg.image_size * c->cfg.image_size * c->cfg.channels;
    HIPCHK(&c->err, launch_fill(in_dev, n, seed, TID_IMAGES, 0, 0.f, 0.f, c->stream));
    HIPCHK(&c->err, sync_compute(c));
    return VH_OK;
}

int vh_last_forward_us(const vh_ctx* c, int64_t* us) {
    if (!c || !us) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *us = c->last_us;
    return VH_OK;
}

int vh_last_kernel_ms(vh_ctx* c, double* ms) {
    if (!c || !ms) return fail(nullptr, VH_ERR_INVALID, "null argument");
    if (!c->timed) return fail(&c->err, VH_ERR_STATE, "no forward has been enqueued yet");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, hipEventSynchronize(c->ev1));
    float t = 0.f;
    HIPCHK(&c->err, hipEventElapsedTime(&t, c->ev0, c->ev1));
    *ms = t;
    return VH_OK;
}

const char* vh_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

int vh_profile_forward(vh_ctx* c, const float* in, int batch, float* logits, double* stage_ms, int n_slots, int* n_written) {
    int rc = check_forward_args(c, in, batch, logits);
    if (rc) return rc;
    if (!stage_ms || n_slots < 2 * kProfiledStages) return fail(&c->err, VH_ERR_INVALID, "need %d stage slots (ms then launch counts)", 2 * kProfiledStages);
    HIPCHK(&c->err, hipSetDevice(c->device));
    std::vector<std::pair<int, hipEvent_t>> ev;
    rc = enqueue_forward(c, ImgIn{in}, batch, logits, &ev, c->stream, 0);
    if (!rc) { hipError_t e = sync_compute(c); if (e != hipSuccess) rc = fail(&c->err, VH_ERR_HIP, "sync: %s", hipGetErrorString(e)); }
    for (int i = 0; i < 2 * kProfiledStages; ++i) stage_ms[i] = 0.0;
    if (!rc)
        for (size_t i = 1; i < ev.size(); ++i) {
            float t = 0.f;
            hipEventElapsedTime(&t, ev[i - 1].second, ev[i].second);
            stage_ms[ev[i].first] += t;
            stage_ms[kProfiledStages + ev[i].first] += 1.0;
        }
    for (auto& p : ev) hipEventDestroy(p.second);
    if (n_written) *n_written = kProfiledStages;
    return rc;
}

// ---- pipelined host path: a ring of in-flight batches ---------------------------------------------------------------
// Modelled on the one asynchronous pattern the reference has, the 24-slot image ring of filter_image /
// get_filtered_image (netFPGA.cpp:292-365, ring state :47-56): submit enqueues H2D copy -> forward -> D2H copy of
// one batch into the next free slot and returns; collect waits for the OLDEST slot.  The copies run on their own
// streams, so the upload of batch i+1 and the download of batch i-1 overlap the forward of batch i.  A full ring on
// submit / an empty ring on collect are reported as errors (the reference prints "PILA LLENA" / "PILA VACIA" and
// drops the frame, :330-333, :358-361).
int vh_ring_destroy(vh_ctx* c) {
    if (!c) return VH_OK;
    if (c->ring.empty() && !c->copy_in) return VH_OK;
    hipSetDevice(c->device);
    if (c->stream) sync_compute(c);
    if (c->copy_in) hipStreamSynchronize(c->copy_in);
    if (c->copy_out) hipStreamSynchronize(c->copy_out);
    for (auto& s : c->ring) {
        if (s.h_in) hipHostFree(s.h_in);
        if (s.h_out) hipHostFree(s.h_out);
        if (s.h_plan) hipHostFree(s.h_plan);
        if (s.d_in) hipFree(s.d_in);
        if (s.d_out) hipFree(s.d_out);
        if (s.in_done) hipEventDestroy(s.in_done);
        if (s.fwd_done) hipEventDestroy(s.fwd_done);
        if (s.out_done) hipEventDestroy(s.out_done);
    }
    c->ring.clear();
    if (c->copy_in) hipStreamDestroy(c->copy_in);
    if (c->copy_out) hipStreamDestroy(c->copy_out);
    c->copy_in = c->copy_out = nullptr;
    c->ring_batch = c->ring_wr = c->ring_rd = c->ring_used = 0;
    c->ring_kind = vh_ctx::RING_F32;
    c->ring_elem = VH_ELEM_F32;
    c->ring_layout = VH_LAYOUT_NHWC;
    c->ring_slot_bytes = 0;
    return VH_OK;
}

static const char* ring_kind_name(vh_ctx::RingKind k) {
    return k == vh_ctx::RING_FRAMES ? "8-bit frames" : k == vh_ctx::RING_U8 ? "8-bit images" : k == vh_ctx::RING_TENSOR ? "image tensors" : "fp32 images";
}

// elem / layout: what a slot of an image ring holds (RING_F32: NHWC fp32, RING_U8: NHWC bytes, RING_TENSOR: the caller's choice)
static int ring_create(vh_ctx* c, int slots, int batch_per_slot, vh_ctx::RingKind kind, size_t slot_bytes = 0, int elem = VH_ELEM_F32,
                       int layout = VH_LAYOUT_NHWC) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (slots < 1 || slots > 64) return fail(&c->err, VH_ERR_INVALID, "slots must be 1..64");
    if (batch_per_slot < 1 || batch_per_slot > c->cfg.max_batch)
        return fail(&c->err, VH_ERR_INVALID, "batch_per_slot %d outside 1..max_batch=%d", batch_per_slot, c->cfg.max_batch);
    const bool frames = kind == vh_ctx::RING_FRAMES;
    if (frames && slot_bytes < 1) return fail(&c->err, VH_ERR_INVALID, "slot_bytes must be positive");
    vh_ring_destroy(c);
    HIPCHK(&c->err, hipSetDevice(c->device));
    const size_t in_bytes = frames ? slot_bytes : (size_t)batch_per_slot * c->cfg.image_size * c->cfg.image_size * c->cfg.channels * ImgIn{nullptr, elem, layout}.elem();
    // frames: the resized-image buffer and a first plan buffer now, and per slot room for a plan of two tables of ~8 taps
    const size_t plan_words = (size_t)batch_per_slot * kResizeFrameWords + 2 * (size_t)c->cfg.image_size * 10;
    if (frames)
        if (int rc = frames_reserve(c, plan_words, false, 0)) return rc;
    const size_t out_bytes = (size_t)batch_per_slot * c->cfg.classes * 4;
    HIPCHK(&c->err, hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking));
    HIPCHK(&c->err, hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking));
    c->ring.resize(slots);
    for (auto& s : c->ring) {
        hipError_t e = hipHostMalloc((void**)&s.h_in, in_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_out, out_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void**)&s.d_in, in_bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&s.d_out, out_bytes);
        if (e == hipSuccess && frames) {
            e = hipHostMalloc((void**)&s.h_plan, plan_words * 4, hipHostMallocDefault);
            if (e == hipSuccess) s.plan_cap = plan_words;
        }
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.fwd_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.out_done, hipEventDisableTiming);
        if (e != hipSuccess) {
            vh_ring_destroy(c);
            return fail(&c->err, VH_ERR_HIP, "vh_ring_create: %s", hipGetErrorString(e));
        }
    }
    if (!frames && two_in_flight_allowed(c)) second_set(c);   // here rather than inside the first submits
    c->ring_flip = 0;
    c->ring_batch = batch_per_slot;
    c->ring_kind = kind;
    c->ring_elem = elem;
    c->ring_layout = layout;
    c->ring_slot_bytes = frames ? slot_bytes : kind == vh_ctx::RING_TENSOR ? in_bytes : 0;
    return VH_OK;
}

int vh_ring_create(vh_ctx* c, int slots, int batch_per_slot) { return ring_create(c, slots, batch_per_slot, vh_ctx::RING_F32); }
int vh_ring_create_u8(vh_ctx* c, int slots, int batch_per_slot) { return ring_create(c, slots, batch_per_slot, vh_ctx::RING_U8, 0, VH_ELEM_U8); }
int vh_ring_create_tensor(vh_ctx* c, int slots, int batch_per_slot, int elem, int layout) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (int rc = check_tensor_kind(&c->err, elem, layout)) return rc;
    return ring_create(c, slots, batch_per_slot, vh_ctx::RING_TENSOR, 0, elem, layout);
}
int vh_ring_create_frames(vh_ctx* c, int slots, int batch_per_slot, size_t slot_bytes) {
    return ring_create(c, slots, batch_per_slot, vh_ctx::RING_FRAMES, slot_bytes);
}

int vh_ring_free_slots(const vh_ctx* c, int* n) {
    if (!c || !n) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *n = (int)c->ring.size() - c->ring_used;
    return VH_OK;
}

static int ring_input(vh_ctx* c, void** pinned_in, vh_ctx::RingKind kind) {
    if (!c || !pinned_in) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "no ring: call vh_ring_create first");
    if (c->ring_kind != kind) return fail(&c->err, VH_ERR_STATE, "this ring stages %s", ring_kind_name(c->ring_kind));
    if (c->ring_used == (int)c->ring.size()) return fail(&c->err, VH_ERR_RING_FULL, "ring full (PILA LLENA)");
    *pinned_in = c->ring[c->ring_wr].h_in;
    return VH_OK;
}

int vh_ring_input(vh_ctx* c, float** pinned_in) { return ring_input(c, (void**)pinned_in, vh_ctx::RING_F32); }
int vh_ring_input_u8(vh_ctx* c, uint8_t** pinned_in) { return ring_input(c, (void**)pinned_in, vh_ctx::RING_U8); }
int vh_ring_input_tensor(vh_ctx* c, void** pinned, size_t* capacity_bytes) {
    if (!capacity_bytes) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (int rc = ring_input(c, pinned, vh_ctx::RING_TENSOR)) return rc;
    *capacity_bytes = c->ring_slot_bytes;
    return VH_OK;
}
int vh_ring_input_frames(vh_ctx* c, uint8_t** pinned, size_t* capacity) {
    if (!capacity) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (int rc = ring_input(c, (void**)pinned, vh_ctx::RING_FRAMES)) return rc;
    *capacity = c->ring_slot_bytes;
    return VH_OK;
}

// frames ring: in_host holds `frame_bytes` of frames described by `desc`; the slot's upload is followed by the resize into
// c->rz_u8 on the context's stream (forwards are ordered on that stream, so one resized buffer serves every slot)
// (`desc` points to descriptors of the type `fmt` plans; a slot is raw bytes, so one frames ring takes every format.  A slot's
// device buffer comes from hipMalloc, so its base is aligned for any sample: base 0)
static int ring_submit(vh_ctx* c, const void* in_host, int batch, vh_ctx::RingKind kind, size_t frame_bytes = 0, const void* desc = nullptr,
                       const FrameFormat& fmt = kFramesRGB) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "no ring: call vh_ring_create first");
    if (c->ring_kind != kind) return fail(&c->err, VH_ERR_STATE, "this ring stages %s", ring_kind_name(c->ring_kind));
    if (!c->weights_ready) return fail(&c->err, VH_ERR_STATE, "submit before weights were loaded");
    if (batch < 1 || batch > c->ring_batch) return fail(&c->err, VH_ERR_INVALID, "batch %d outside 1..%d", batch, c->ring_batch);
    if (c->ring_used == (int)c->ring.size()) return fail(&c->err, VH_ERR_RING_FULL, "ring full (PILA LLENA)");
    const bool frames = kind == vh_ctx::RING_FRAMES;
    int rc, max_tiles = 0;
    if (frames) {   // every check, and the plan, before anything is enqueued or the slot is touched
        if (frame_bytes < 1 || frame_bytes > c->ring_slot_bytes) return fail(&c->err, VH_ERR_INVALID, "nbytes %zu outside 1..slot_bytes=%zu", frame_bytes, c->ring_slot_bytes);
        if ((rc = frames_plan(c, fmt, desc, batch, frame_bytes, 0, &max_tiles))) return rc;
    }
    HIPCHK(&c->err, hipSetDevice(c->device));
    vh_ctx::RingSlot& s = c->ring[c->ring_wr];
    const ImgIn slot_in{s.d_in, c->ring_elem, c->ring_layout};   // an image ring's slot
    const size_t in_bytes = frames ? frame_bytes : (size_t)batch * c->cfg.image_size * c->cfg.image_size * c->cfg.channels * slot_in.elem();
    if (frames) {
        const size_t words = c->rz_words.size();
        if (words > s.plan_cap) {   // a free slot: its last upload ran before its batch was collected
            if (s.h_plan) hipHostFree(s.h_plan);
            s.h_plan = nullptr; s.plan_cap = 0;
            HIPCHK(&c->err, hipHostMalloc((void**)&s.h_plan, words * 8, hipHostMallocDefault));
            s.plan_cap = words * 2;
        }
        if ((rc = frames_reserve(c, words, false, 0))) return rc;
        memcpy(s.h_plan, c->rz_words.data(), words * 4);
    }
    if (in_host && in_host != s.h_in) memcpy(s.h_in, in_host, in_bytes);  // NULL / the slot's own buffer: already filled in place
    s.batch = batch;
    HIPCHK(&c->err, hipMemcpyAsync(s.d_in, s.h_in, in_bytes, hipMemcpyHostToDevice, c->copy_in));
    HIPCHK(&c->err, hipEventRecord(s.in_done, c->copy_in));
    // Image rings: consecutive submits alternate between the two compute streams and buffer sets, so the forward of batch i + 1
    // runs beside that of batch i; every slot has its own logits buffer, so nothing orders their heads.  The frames ring stays
    // on c->stream: its resize writes the one rz_u8 buffer that the forward's first kernel reads.
    const int set = !frames && two_in_flight(c) ? c->ring_flip : 0;
    hipStream_t const st = set ? c->stream2 : c->stream;
    c->ring_flip = set ^ 1;
    if (set) c->s2_open = true;
    HIPCHK(&c->err, hipStreamWaitEvent(st, s.in_done, 0));
    if (frames) {
        const FrameJob job{fmt, (const uint8_t*)s.d_in, s.h_plan, c->rz_words.size(), max_tiles};
        if ((rc = enqueue_resize(c, job, batch))) return rc;
    }
    rc = run_step(c, frames ? ImgIn{c->rz_u8, kU8} : slot_in, batch, s.d_out, set);
    if (rc) return rc;
    HIPCHK(&c->err, hipEventRecord(s.fwd_done, st));
    HIPCHK(&c->err, hipStreamWaitEvent(c->copy_out, s.fwd_done, 0));
    HIPCHK(&c->err, hipMemcpyAsync(s.h_out, s.d_out, (size_t)batch * c->cfg.classes * 4, hipMemcpyDeviceToHost, c->copy_out));
    HIPCHK(&c->err, hipEventRecord(s.out_done, c->copy_out));
    c->ring_wr = (c->ring_wr + 1) % (int)c->ring.size();
    ++c->ring_used;
    return VH_OK;
}

int vh_ring_submit(vh_ctx* c, const float* in_host, int batch) { return ring_submit(c, in_host, batch, vh_ctx::RING_F32); }
int vh_ring_submit_u8(vh_ctx* c, const uint8_t* in_host, int batch) { return ring_submit(c, in_host, batch, vh_ctx::RING_U8); }
int vh_ring_submit_tensor(vh_ctx* c, const void* in_host, int batch) { return ring_submit(c, in_host, batch, vh_ctx::RING_TENSOR); }
int vh_ring_submit_frames(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesRGB);
}
int vh_ring_submit_frames_nv12(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesNV12);
}
int vh_ring_submit_frames_yuv(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesYUV);
}
int vh_ring_submit_frames_p016(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesP016);
}
int vh_ring_submit_frames_yuv16(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesYUV16);
}
int vh_ring_submit_frames_yuy2(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesYUY2);
}
int vh_ring_submit_frames_y210(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesY210);
}
int vh_ring_submit_frames_bgra(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesBGRA);
}
int vh_ring_submit_frames_y410(vh_ctx* c, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch) {
    return ring_submit(c, frames_host, batch, vh_ctx::RING_FRAMES, nbytes, desc, kFramesY410);
}

int vh_ring_collect(vh_ctx* c, float* logits_host, int* batch) {
    if (!c || !logits_host) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "no ring: call vh_ring_create first");
    if (c->ring_used == 0) return fail(&c->err, VH_ERR_RING_EMPTY, "ring empty (PILA VACIA)");
    HIPCHK(&c->err, hipSetDevice(c->device));
    vh_ctx::RingSlot& s = c->ring[c->ring_rd];
    HIPCHK(&c->err, hipEventSynchronize(s.out_done));
    memcpy(logits_host, s.h_out, (size_t)s.batch * c->cfg.classes * 4);
    if (batch) *batch = s.batch;
    c->ring_rd = (c->ring_rd + 1) % (int)c->ring.size();
    --c->ring_used;
    return VH_OK;
}

int vh_set_streams(vh_ctx* c, int n) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (n < 1 || n > vh_ctx::kMaxStreams) return fail(&c->err, VH_ERR_INVALID, "streams must be 1..%d", vh_ctx::kMaxStreams);
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    c->nstreams = n;
    drop_graphs(c);
    return VH_OK;
}

int vh_set_graph(vh_ctx* c, int enable) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    c->use_graph = enable != 0;
    if (!c->use_graph) drop_graphs(c);
    return VH_OK;
}

int vh_get_graph(const vh_ctx* c, int* enabled, int* cached) {
    if (!c || !enabled) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *enabled = c->use_graph ? 1 : 0;
    if (cached) *cached = (int)c->graphs.size();
    return VH_OK;
}

int vh_get_streams(const vh_ctx* c, int* n) {
    if (!c || !n) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *n = c->nstreams;
    return VH_OK;
}

int vh_get_inflight(const vh_ctx* c, int* n) {
    if (!c || !n) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *n = two_in_flight_allowed(c) ? 2 : 1;
    return VH_OK;
}

int vh_set_stage_timing(vh_ctx* c, int stage) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    if (stage < -1 || stage >= ST_COUNT) return fail(&c->err, VH_ERR_INVALID, "unknown stage %d", stage);
    c->timing_stage = stage;
    c->tev_used = 0;
    return VH_OK;
}

int vh_get_stage_timing(vh_ctx* c, double* avg_ms, double* min_ms, int* launches) {
    if (!c || !avg_ms || !launches) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    double sum = 0.0, mn = 1e30;
    int n = 0;
    for (size_t i = 0; i + 1 < c->tev_used; i += 2) {
        float t = 0.f;
        HIPCHK(&c->err, hipEventElapsedTime(&t, c->tev[i], c->tev[i + 1]));
        sum += t; if (t < mn) mn = t; ++n;
    }
    *avg_ms = n ? sum / n : 0.0;
    if (min_ms) *min_ms = n ? mn : 0.0;
    *launches = n;
    return VH_OK;
}

int vh_set_step_timing(vh_ctx* c, int enable) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    c->step_timing = enable != 0;
    c->sev_used = 0;
    return VH_OK;
}

int vh_get_step_timing(vh_ctx* c, double* step_ms, int max_steps, int* steps) {
    if (!c || !steps || (max_steps > 0 && !step_ms)) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    int n = 0;
    for (size_t i = 0; i + 1 < c->sev_used; ++i) {
        float t = 0.f;
        HIPCHK(&c->err, hipEventElapsedTime(&t, c->sev[i], c->sev[i + 1]));
        if (n < max_steps) step_ms[n] = t;
        ++n;
    }
    *steps = n;
    return VH_OK;
}

int vh_debug_read(vh_ctx* c, int what, float* host_out, size_t n_floats) {
    if (!c || !host_out) return fail(c ? &c->err : nullptr, VH_ERR_INVALID, "null argument");
    if (c->last_batch <= 0) return fail(&c->err, VH_ERR_STATE, "no forward has run");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    const size_t D = c->cfg.dim;
    if (what == 0) {
        const size_t n = (size_t)c->last_batch * c->L.T * D;
        if (n_floats != n) return fail(&c->err, VH_ERR_INVALID, "expected %zu floats", n);
        const ResidView v = resid_view(c, c->act[c->last_set], layers_to_run(c));
        if (!v.lo) {
            HIPCHK(&c->err, hipMemcpy(host_out, v.hi, n * 4, hipMemcpyDeviceToHost));
            return VH_OK;
        }
        // two planes, x = hi + lo, decoded on the host: the view of the planes that shares no code with the kernels that read them
        auto f = [&](const uint8_t* p, int dt) {   // two bytes of a 16-bit plane -> float
            uint16_t b; memcpy(&b, p, 2);
            if (dt == VH_DTYPE_BF16) { uint32_t u = (uint32_t)b << 16; float x; memcpy(&x, &u, 4); return x; }
            _Float16 hv; memcpy(&hv, &b, 2); return (float)hv;
        };
        auto g = [&](uint8_t b) {   // OCP e4m3fn -> float
            const int e = (b >> 3) & 15, m = b & 7;
            float x = e ? ldexpf(1.f + m / 8.f, e - 7) : ldexpf(m / 8.f, -6);
            return (b & 0x80) ? -x : x;
        };
        std::vector<uint8_t> hi(n * hi_bytes(v.form)), lo(n * lo_bytes(v.form));
        HIPCHK(&c->err, hipMemcpy(hi.data(), v.hi, hi.size(), hipMemcpyDeviceToHost));
        HIPCHK(&c->err, hipMemcpy(lo.data(), v.lo, lo.size(), hipMemcpyDeviceToHost));
        if (v.form == VH_DTYPE_FP8) {   // e4m3 hi plane (the GEMM operand) + bf16 lo plane
            for (size_t i = 0; i < n; ++i) host_out[i] = g(hi[i]) + f(&lo[2 * i], VH_DTYPE_BF16);
            return VH_OK;
        }
        const float inv = v.form == VH_DTYPE_BF16 ? Lo8<BF16>::inv : Lo8<FP16>::inv;   // the byte plane's scale
        for (size_t i = 0; i < n; ++i) host_out[i] = f(&hi[2 * i], v.form) + g(lo[i]) * inv;
        return VH_OK;
    }
    if (what == 1) {
        const size_t n = (size_t)c->last_batch * c->L.HW;   // the head's input [batch][W]
        if (n_floats != n) return fail(&c->err, VH_ERR_INVALID, "expected %zu floats", n);
        HIPCHK(&c->err, hipMemcpy(host_out, c->act[c->last_set].clsn32, n * 4, hipMemcpyDeviceToHost));
        return VH_OK;
    }
    if (what == 3) {   // 1 when the last forward kept the MLP hidden activation in its tiled layout (h_tiled)
        if (n_floats != 1) return fail(&c->err, VH_ERR_INVALID, "expected 1 float");
        host_out[0] = c->last_h_tiled ? 1.f : 0.f;
        return VH_OK;
    }
    if (what == 4) {   // 1 when the last forward kept q|k|v head-major (qkv_hm)
        if (n_floats != 1) return fail(&c->err, VH_ERR_INVALID, "expected 1 float");
        host_out[0] = c->last_qkv_hm ? 1.f : 0.f;
        return VH_OK;
    }
    return fail(&c->err, VH_ERR_INVALID, "unknown tap %d", what);
}

int vh_debug_set_layers(vh_ctx* c, int n_layers) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "null context");
    c->run_layers = n_layers;
    if (c->stream) sync_compute(c);
    drop_graphs(c);
    return VH_OK;
}

// ---- token features (vithip.h "Token features"; kernels_features.hip) ---------------------------------------------------
// A pull interface: these calls read what the last forward left in the arena -- the residual stream in the form its path keeps it
// (the same choice vh_debug_read makes), clsn32, the final LayerNorm's parameters in the blob -- and no forward knows of them.
// The normalised mean's row statistics go through the last set's stats, which are free between forwards (every path that reads it writes it
// first); everything is enqueued on the context's main stream, where a forward on several streams has already joined.
static int features_check_call(vh_ctx* c, const vh_features* f, bool device) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "read_features: null context");
    if (!f) return fail(&c->err, VH_ERR_INVALID, "read_features: null descriptor");
    if (!f->cls && !f->patch && !f->mean) return fail(&c->err, VH_ERR_INVALID, "read_features: no output requested (cls, patch and mean are all NULL)");
    if (f->elem != VH_ELEM_F32 && f->elem != VH_ELEM_F16 && f->elem != VH_ELEM_BF16)
        return fail(&c->err, VH_ERR_INVALID, "read_features: elem %d is not VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16", f->elem);
    if (f->norm != VH_FEAT_NORM && f->norm != VH_FEAT_RAW) return fail(&c->err, VH_ERR_INVALID, "read_features: norm %d is not VH_FEAT_NORM (0) or VH_FEAT_RAW (1)", f->norm);
    if (device && (((uintptr_t)f->cls | (uintptr_t)f->patch | (uintptr_t)f->mean) & 15))
        return fail(&c->err, VH_ERR_INVALID, "read_features: a device output pointer is not 16-byte aligned (cls %p, patch %p, mean %p)", f->cls, f->patch, f->mean);
    if (c->cfg.flags & VH_FLAG_CLS_TAIL)
        return fail(&c->err, VH_ERR_UNSUPPORTED, "read_features: a VH_FLAG_CLS_TAIL context's last layer updates the class-token rows only");
    if (f->cls && !c->L.ncls) return fail(&c->err, VH_ERR_UNSUPPORTED, "read_features: cls on a context without a class token (VH_FLAG_NO_CLS)");
    if (!c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "read_features: a ring exists on this context (its forwards belong to slots); vh_ring_destroy first");
    if (c->last_batch <= 0) return fail(&c->err, VH_ERR_STATE, "read_features: no forward has run");
    return VH_OK;
}
// where the rows of a read-out live, and whether its normalised class-token rows are the head's (the final state: clsn32)
struct FeatSource : ResidView { bool head_cls; };
static FeatSource features_live(const vh_ctx* c) {
    // the final layer's rows are the live residual of the most recently enqueued forward
    return FeatSource{resid_view(c, c->act[c->last_set], layers_to_run(c)), c->L.pool == VH_POOL_CLS};   // (a pooled head's input is not LN(row 0))
}
static int features_enqueue(vh_ctx* c, const vh_layer_features& f, const FeatSource& src, const char* who) {
    const vh_config& g = c->cfg;
    const bool norm = f.norm == VH_FEAT_NORM;
    FeatureArgs a{};
    a.hi = src.hi; a.lo = src.lo; a.form = src.form;
    a.batch = c->last_batch; a.tokens = c->L.T; a.lead = c->L.lead; a.dim = g.dim;
    a.gamma = c->params + c->L.lnfw; a.beta = c->params + c->L.lnfb; a.eps = g.ln_eps;
    a.elem = f.elem; a.norm = f.norm;
    const bool copy_cls = norm && src.head_cls;   // the normalised class-token rows the head multiplied: a conversion copy of clsn32
    a.cls = copy_cls ? nullptr : f.cls;
    a.patch = f.patch; a.mean = f.mean; a.stats = c->act[c->last_set].stats;
    a.reg = f.reg; a.patch_layout = f.patch_layout;
    a.no_cls = c->L.ncls ? 0 : 1;   // VH_FLAG_NO_CLS: lead = R rows, all of them registers (an internal form: the public taps keep lead >= 1)
    if (a.cls || a.patch || a.mean || a.reg) {
        if (const char* why = features_check(a)) return fail(&c->err, VH_ERR_INVALID, "%s: %s", who, why);
        HIPCHK(&c->err, launch_token_features(a, c->stream));
    }
    if (copy_cls && f.cls) {
        const int64_t n = (int64_t)c->last_batch * g.dim;
        if (f.elem == VH_ELEM_F32) HIPCHK(&c->err, hipMemcpyAsync(f.cls, c->act[c->last_set].clsn32, n * 4, hipMemcpyDeviceToDevice, c->stream));
        else HIPCHK(&c->err, launch_cast(c->act[c->last_set].clsn32, f.cls, n, f.elem == VH_ELEM_BF16 ? VH_DTYPE_BF16 : VH_DTYPE_FP16, c->stream));
    }
    return VH_OK;
}
// the host form: the outputs are staged in the q|k|v buffer -- scratch between forwards (every forward writes its rows before
// attention reads them), and at 6 bytes per row element always large enough for fp32 rows of every token + the two [batch][D] outputs
struct Staging {
    char* base;
    size_t cap, at = 0;
    explicit Staging(const vh_ctx* c) : base((char*)c->act[c->last_set].qkv16), cap(act_buffer_bytes(c, &ActSet::qkv16)) {}
    void* take(const void* want, size_t bytes) {
        if (!want) return nullptr;
        void* const p = base + at;
        at += align_up(bytes, 256);
        return p;
    }
};
static int features_read_host(vh_ctx* c, const vh_layer_features& f, const FeatSource& src, const char* who) {
    const size_t es = f.elem == VH_ELEM_F32 ? 4 : 2, D = c->cfg.dim, B = c->last_batch;
    const size_t n_row = B * D * es, n_patch = B * (size_t)c->L.NP * D * es, n_reg = B * (size_t)c->L.R * D * es;
    Staging st(c);
    vh_layer_features d = f;
    d.patch = st.take(f.patch, n_patch);
    d.cls = st.take(f.cls, n_row);
    d.mean = st.take(f.mean, n_row);
    d.reg = st.take(f.reg, n_reg);
    if (st.at > st.cap) return fail(&c->err, VH_ERR_STATE, "%s: staging needs %zu bytes, the scratch holds %zu", who, st.at, st.cap);
    if (int rc = features_enqueue(c, d, src, who)) return rc;
    if (f.patch) HIPCHK(&c->err, hipMemcpyAsync(f.patch, d.patch, n_patch, hipMemcpyDeviceToHost, c->stream));
    if (f.cls) HIPCHK(&c->err, hipMemcpyAsync(f.cls, d.cls, n_row, hipMemcpyDeviceToHost, c->stream));
    if (f.mean) HIPCHK(&c->err, hipMemcpyAsync(f.mean, d.mean, n_row, hipMemcpyDeviceToHost, c->stream));
    if (f.reg) HIPCHK(&c->err, hipMemcpyAsync(f.reg, d.reg, n_reg, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, sync_compute(c));
    return VH_OK;
}
static vh_layer_features features_final(const vh_features& f) {
    return vh_layer_features{f.cls, f.patch, f.mean, nullptr, f.elem, f.norm, -1, VH_FEAT_ROWS};
}
int vh_features_dims(const vh_ctx* c, int* batch, int* tokens, int* patches, int* dim) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "features_dims: null context");
    if (batch) *batch = c->last_batch;
    if (tokens) *tokens = c->L.T;
    if (patches) *patches = c->L.NP;
    if (dim) *dim = c->cfg.dim;
    return VH_OK;
}
int vh_read_features_device_async(vh_ctx* c, const vh_features* f) {
    if (int rc = features_check_call(c, f, true)) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    return features_enqueue(c, features_final(*f), features_live(c), "read_features");
}
int vh_read_features_device(vh_ctx* c, const vh_features* f) {
    if (int rc = vh_read_features_device_async(c, f)) return rc;
    HIPCHK(&c->err, sync_compute(c));
    return VH_OK;
}
int vh_read_features(vh_ctx* c, const vh_features* f) {
    if (int rc = features_check_call(c, f, false)) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    return features_read_host(c, features_final(*f), features_live(c), "read_features");
}

// ---- layer features (vithip.h "Layer features") ---------------------------------------------------------------------------
// The list and the capture store; enqueue_forward copies into the store and records what it captured (cap_*).
// a layer list of `who` (the call's name in the messages): at most max_n entries, each 1 .. layers, strictly ascending
static int check_layer_list(vh_ctx* c, const char* who, const int* layers, int n, int max_n) {
    if (n < 0 || n > max_n) return fail(&c->err, VH_ERR_INVALID, "%s: %d layers, outside 0..%d", who, n, max_n);
    if (n > 0 && !layers) return fail(&c->err, VH_ERR_INVALID, "%s: null list", who);
    for (int i = 0; i < n; ++i) {
        if (layers[i] < 1 || layers[i] > c->cfg.layers)
            return fail(&c->err, VH_ERR_INVALID, "%s: entry %d is layer %d, outside 1..%d", who, i, layers[i], c->cfg.layers);
        if (i && layers[i] <= layers[i - 1])
            return fail(&c->err, VH_ERR_INVALID, "%s: the list must be strictly ascending (entry %d is %d after %d)", who, i, layers[i], layers[i - 1]);
    }
    return VH_OK;
}
int vh_set_feature_layers(vh_ctx* c, const int* layers, int n) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "set_feature_layers: null context");
    if (int rc = check_layer_list(c, "set_feature_layers", layers, n, VH_MAX_FEATURE_LAYERS)) return rc;
    if (n > 0 && (c->cfg.flags & VH_FLAG_CLS_TAIL))
        return fail(&c->err, VH_ERR_UNSUPPORTED, "set_feature_layers: a VH_FLAG_CLS_TAIL context's last layer updates the class-token rows only");
    if (!c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "set_feature_layers: a ring exists on this context; vh_ring_destroy first");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    int slots = 0;
    for (int i = 0; i < n; ++i) slots += layers[i] < c->cfg.layers;
    // sized for the planes where the residual stays two planes for good (the configured split, no guard that may leave it: split then
    // equals split_cfg, so resid_form gives the planes' form); for fp32 rows where it is, or may become, the fp32 array
    const int form = c->split_cfg && !c->guard_auto ? resid_form(c, c->cfg.layers) : VH_FEAT_FORM_F32;
    const size_t slot = align_up((size_t)c->cfg.max_batch * c->L.T * c->cfg.dim * (hi_bytes(form) + lo_bytes(form)), 256);
    char* store = nullptr;
    if (slots) {
        const hipError_t e = hipMalloc((void**)&store, slot * slots);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(&c->err, VH_ERR_HIP, "set_feature_layers: no room for the capture store (%d layers x %zu bytes): %s; the previous list stays",
                        slots, slot, hipGetErrorString(e));
        }
    }
    drop_graphs(c);   // captured launch sequences hold the old list's copies and the old store
    if (c->feat_store) hipFree(c->feat_store);
    c->feat_store = store;
    c->feat_slot = slot;
    c->feat_n = n;
    for (int i = 0; i < n; ++i) c->feat_layers[i] = layers[i];
    c->cap_n = 0;     // what the last forward captured lived in the old store
    return VH_OK;
}
int vh_get_feature_layers(const vh_ctx* c, int* layers, int* n) {
    if (!c || !n) return fail(nullptr, VH_ERR_INVALID, "get_feature_layers: null argument");
    *n = c->feat_n;
    for (int i = 0; layers && i < c->feat_n; ++i) layers[i] = c->feat_layers[i];
    return VH_OK;
}

// every refusal of the three read calls; on success *src says where the layer's rows live
static int layer_features_check_call(vh_ctx* c, const vh_layer_features* f, bool device, FeatSource* src) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "read_layer_features: null context");
    if (!f) return fail(&c->err, VH_ERR_INVALID, "read_layer_features: null descriptor");
    if (!f->cls && !f->patch && !f->mean && !f->reg)
        return fail(&c->err, VH_ERR_INVALID, "read_layer_features: no output requested (cls, patch, mean and reg are all NULL)");
    if (f->elem != VH_ELEM_F32 && f->elem != VH_ELEM_F16 && f->elem != VH_ELEM_BF16)
        return fail(&c->err, VH_ERR_INVALID, "read_layer_features: elem %d is not VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16", f->elem);
    if (f->norm != VH_FEAT_NORM && f->norm != VH_FEAT_RAW)
        return fail(&c->err, VH_ERR_INVALID, "read_layer_features: norm %d is not VH_FEAT_NORM (0) or VH_FEAT_RAW (1)", f->norm);
    if (f->patch_layout != VH_FEAT_ROWS && f->patch_layout != VH_FEAT_NCHW)
        return fail(&c->err, VH_ERR_INVALID, "read_layer_features: patch_layout %d is not VH_FEAT_ROWS (0) or VH_FEAT_NCHW (1)", f->patch_layout);
    const int layers = c->cfg.layers;
    if (f->layer != -1 && (f->layer < 1 || f->layer > layers))
        return fail(&c->err, VH_ERR_INVALID, "read_layer_features: layer %d is not -1 or 1..%d", f->layer, layers);
    if (device && (((uintptr_t)f->cls | (uintptr_t)f->patch | (uintptr_t)f->mean | (uintptr_t)f->reg) & 15))
        return fail(&c->err, VH_ERR_INVALID, "read_layer_features: a device output pointer is not 16-byte aligned (cls %p, patch %p, mean %p, reg %p)",
                    f->cls, f->patch, f->mean, f->reg);
    if (f->reg && c->L.R == 0) return fail(&c->err, VH_ERR_INVALID, "read_layer_features: reg on a context without register tokens (VH_FLAG_REGISTERS)");
    if (c->cfg.flags & VH_FLAG_CLS_TAIL)
        return fail(&c->err, VH_ERR_UNSUPPORTED, "read_layer_features: a VH_FLAG_CLS_TAIL context's last layer updates the class-token rows only");
    if (f->cls && !c->L.ncls) return fail(&c->err, VH_ERR_UNSUPPORTED, "read_layer_features: cls on a context without a class token (VH_FLAG_NO_CLS)");
    if (!c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "read_layer_features: a ring exists on this context (its forwards belong to slots); vh_ring_destroy first");
    if (c->last_batch <= 0) return fail(&c->err, VH_ERR_STATE, "read_layer_features: no forward has run");
    if (f->layer == -1) { *src = features_live(c); return VH_OK; }
    int slot = -1;
    for (int i = 0; i < c->cap_n; ++i) if (c->cap_layers[i] == f->layer) slot = i;
    if (f->layer < layers && slot < 0)
        return fail(&c->err, VH_ERR_STATE, "read_layer_features: layer %d was not in the list when the last forward was enqueued (vh_set_feature_layers)", f->layer);
    if (f->layer > c->cap_nl)
        return fail(&c->err, VH_ERR_STATE, "read_layer_features: the last forward ran %d layers and did not reach layer %d (vh_debug_set_layers)", c->cap_nl, f->layer);
    if (f->layer == c->cap_nl) {   // the live residual; its normalised class-token rows are the head's for the whole model only
        *src = features_live(c);
        src->head_cls = src->head_cls && f->layer == layers;
        return VH_OK;
    }
    *src = FeatSource{slot_view(c, slot, c->cap_form), false};
    return VH_OK;
}
int vh_read_layer_features_device_async(vh_ctx* c, const vh_layer_features* f) {
    FeatSource src{};
    if (int rc = layer_features_check_call(c, f, true, &src)) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    return features_enqueue(c, *f, src, "read_layer_features");
}
int vh_read_layer_features_device(vh_ctx* c, const vh_layer_features* f) {
    if (int rc = vh_read_layer_features_device_async(c, f)) return rc;
    HIPCHK(&c->err, sync_compute(c));
    return VH_OK;
}
int vh_read_layer_features(vh_ctx* c, const vh_layer_features* f) {
    FeatSource src{};
    if (int rc = layer_features_check_call(c, f, false, &src)) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    return features_read_host(c, *f, src, "read_layer_features");
}

// ---- attention maps (vithip.h "Attention maps"; kernels_attn_maps.hip) -------------------------------------------------------
// The list and the store; enqueue_forward runs the capture kernel into the store and records what it captured (acap_*).
int vh_set_attention_layers(vh_ctx* c, const int* layers, int n, int queries) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "set_attention_layers: null context");
    if (int rc = check_layer_list(c, "set_attention_layers", layers, n, VH_MAX_ATTENTION_LAYERS)) return rc;
    if (queries != VH_ATTN_Q_CLS && queries != VH_ATTN_Q_LEAD)
        return fail(&c->err, VH_ERR_INVALID, "set_attention_layers: queries %d is not VH_ATTN_Q_CLS (0) or VH_ATTN_Q_LEAD (1)", queries);
    if (n > 0 && queries == VH_ATTN_Q_CLS && !c->L.ncls)
        return fail(&c->err, VH_ERR_INVALID, "set_attention_layers: VH_ATTN_Q_CLS on a context without a class token (VH_FLAG_NO_CLS)");
    if (n > 0 && queries == VH_ATTN_Q_LEAD && c->L.lead < 1)
        return fail(&c->err, VH_ERR_INVALID, "set_attention_layers: VH_ATTN_Q_LEAD on a context without leading rows (no class token, no registers)");
    const int Q = queries == VH_ATTN_Q_CLS ? 1 : c->L.lead;
    if (n > 0 && Q > kAttnMapsMaxQueries)
        return fail(&c->err, VH_ERR_INVALID, "set_attention_layers: %d leading rows, the capture kernel takes at most %d", Q, kAttnMapsMaxQueries);
    if (n > 0 && (c->cfg.flags & VH_FLAG_CLS_TAIL))
        return fail(&c->err, VH_ERR_UNSUPPORTED, "set_attention_layers: a VH_FLAG_CLS_TAIL context's last layer runs the class-token attention kernel");
    if (!c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "set_attention_layers: a ring exists on this context; vh_ring_destroy first");
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, sync_compute(c));
    const size_t slot = align_up((size_t)c->cfg.max_batch * c->cfg.heads * Q * c->L.T * sizeof(float), 256);
    char* store = nullptr;
    if (n) {
        const hipError_t e = hipMalloc((void**)&store, slot * n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(&c->err, VH_ERR_HIP, "set_attention_layers: no room for the store (%d layers x %zu bytes): %s; the previous list stays",
                        n, slot, hipGetErrorString(e));
        }
    }
    drop_graphs(c);   // captured launch sequences hold the old list's launches and the old store
    if (c->attn_store) hipFree(c->attn_store);
    c->attn_store = store;
    c->attn_slot = slot;
    c->attn_n = n;
    c->attn_q = n ? Q : 0;
    c->attn_mode = queries;
    for (int i = 0; i < n; ++i) c->attn_layers[i] = layers[i];
    c->acap_n = 0;    // what the last forward captured lived in the old store
    return VH_OK;
}
int vh_get_attention_layers(const vh_ctx* c, int* layers, int* n, int* queries) {
    if (!c || !n) return fail(nullptr, VH_ERR_INVALID, "get_attention_layers: null argument");
    *n = c->attn_n;
    if (queries) *queries = c->attn_mode;
    for (int i = 0; layers && i < c->attn_n; ++i) layers[i] = c->attn_layers[i];
    return VH_OK;
}
int vh_attention_dims(const vh_ctx* c, int* batch, int* heads, int* queries, int* tokens, int* patches) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "attention_dims: null context");
    if (batch) *batch = c->last_batch;
    if (heads) *heads = c->cfg.heads;
    if (queries) *queries = c->attn_q;
    if (tokens) *tokens = c->L.T;
    if (patches) *patches = c->L.NP;
    return VH_OK;
}
// every refusal of the three read calls; on success *slot is the layer's slot of the store
static int attention_check_call(vh_ctx* c, const vh_attention_maps* f, bool device, const float** slot) {
    if (!c) return fail(nullptr, VH_ERR_INVALID, "read_attention: null context");
    if (!f) return fail(&c->err, VH_ERR_INVALID, "read_attention: null descriptor");
    if (!f->probs && !f->head_mean) return fail(&c->err, VH_ERR_INVALID, "read_attention: no output requested (probs and head_mean are both NULL)");
    if (f->elem != VH_ELEM_F32 && f->elem != VH_ELEM_F16 && f->elem != VH_ELEM_BF16)
        return fail(&c->err, VH_ERR_INVALID, "read_attention: elem %d is not VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16", f->elem);
    if (f->keys != VH_ATTN_KEYS_ALL && f->keys != VH_ATTN_KEYS_PATCH)
        return fail(&c->err, VH_ERR_INVALID, "read_attention: keys %d is not VH_ATTN_KEYS_ALL (0) or VH_ATTN_KEYS_PATCH (1)", f->keys);
    const int layers = c->cfg.layers;
    if (f->layer != -1 && (f->layer < 1 || f->layer > layers))
        return fail(&c->err, VH_ERR_INVALID, "read_attention: layer %d is not -1 or 1..%d", f->layer, layers);
    if (f->reserved != 0) return fail(&c->err, VH_ERR_INVALID, "read_attention: reserved is %d, not 0", f->reserved);
    if (device && (((uintptr_t)f->probs | (uintptr_t)f->head_mean) & 15))
        return fail(&c->err, VH_ERR_INVALID, "read_attention: a device output pointer is not 16-byte aligned (probs %p, head_mean %p)", f->probs, f->head_mean);
    if (c->cfg.flags & VH_FLAG_CLS_TAIL)
        return fail(&c->err, VH_ERR_UNSUPPORTED, "read_attention: a VH_FLAG_CLS_TAIL context's last layer runs the class-token attention kernel");
    if (!c->ring.empty()) return fail(&c->err, VH_ERR_STATE, "read_attention: a ring exists on this context (its forwards belong to slots); vh_ring_destroy first");
    if (c->last_batch <= 0) return fail(&c->err, VH_ERR_STATE, "read_attention: no forward has run");
    const int layer = f->layer == -1 ? layers : f->layer;
    int at = -1;
    for (int i = 0; i < c->acap_n; ++i) if (c->acap_layers[i] == layer) at = i;
    if (at < 0)
        return fail(&c->err, VH_ERR_STATE, "read_attention: layer %d was not in the list when the last forward was enqueued (vh_set_attention_layers)", layer);
    if (layer > c->acap_nl)
        return fail(&c->err, VH_ERR_STATE, "read_attention: the last forward ran %d layers and did not reach layer %d (vh_debug_set_layers)", c->acap_nl, layer);
    *slot = (const float*)(c->attn_store + (size_t)at * c->attn_slot);
    return VH_OK;
}
static int attention_enqueue(vh_ctx* c, const vh_attention_maps& f, const float* slot) {
    HIPCHK(&c->err, launch_attention_readout(slot, c->last_batch, c->cfg.heads, c->attn_q, c->L.T, c->L.lead, f.elem, f.keys, f.probs, f.head_mean, c->stream));
    return VH_OK;
}
int vh_read_attention_device_async(vh_ctx* c, const vh_attention_maps* f) {
    const float* slot = nullptr;
    if (int rc = attention_check_call(c, f, true, &slot)) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    return attention_enqueue(c, *f, slot);
}
int vh_read_attention_device(vh_ctx* c, const vh_attention_maps* f) {
    if (int rc = vh_read_attention_device_async(c, f)) return rc;
    HIPCHK(&c->err, sync_compute(c));
    return VH_OK;
}
// the host form: staged in the q|k|v buffer, as features_read_host does (scratch between forwards)
int vh_read_attention(vh_ctx* c, const vh_attention_maps* f) {
    const float* slot = nullptr;
    if (int rc = attention_check_call(c, f, false, &slot)) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    const size_t es = f->elem == VH_ELEM_F32 ? 4 : 2, B = c->last_batch, Q = c->attn_q;
    const size_t K = f->keys == VH_ATTN_KEYS_PATCH ? c->L.NP : c->L.T;
    const size_t n_probs = B * c->cfg.heads * Q * K * es, n_mean = B * Q * K * es;
    Staging st(c);
    vh_attention_maps d = *f;
    d.probs = st.take(f->probs, n_probs);
    d.head_mean = st.take(f->head_mean, n_mean);
    if (st.at > st.cap) return fail(&c->err, VH_ERR_STATE, "read_attention: staging needs %zu bytes, the scratch holds %zu", st.at, st.cap);
    if (int rc = attention_enqueue(c, d, slot)) return rc;
    if (f->probs) HIPCHK(&c->err, hipMemcpyAsync(f->probs, d.probs, n_probs, hipMemcpyDeviceToHost, c->stream));
    if (f->head_mean) HIPCHK(&c->err, hipMemcpyAsync(f->head_mean, d.head_mean, n_mean, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, sync_compute(c));
    return VH_OK;
}

// ---- operator-level entry points ------------------------------------------------------------------
#define OPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(nullptr, VH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// ---- the six GEMM taps.  Each fills a GemmArgs from its parameters; this one body checks (gemm_check: the reason, before a device
// is touched), launches, synchronises and maps the error.  `tag` names the tap: in "<tag> failed", and in front of gemm_check's reason
// for e4m3 operands.  `offered8`: the e4m3 epilogues the tap has parameters for, a bit per VH_EPI_* code (0: a 16-bit tap, which has
// no scale parameter and refuses e4m3 operands).
constexpr unsigned kEpiPlain8 = 1u << VH_EPI_BIAS | 1u << VH_EPI_BIAS_GELU | 1u << VH_EPI_BIAS_QGELU | 1u << VH_EPI_BIAS_TGELU | 1u << VH_EPI_BIAS_RESID | 1u << VH_EPI_BIAS_F32;
constexpr unsigned kEpiFold8 = 1u << VH_EPI_LNFOLD | 1u << VH_EPI_LNFOLD_GELU | 1u << VH_EPI_LNFOLD_QGELU | 1u << VH_EPI_LNFOLD_TGELU | 1u << VH_EPI_RESID_LN | 1u << VH_EPI_RESID_SPLIT;
static int op_gemm_run(const char* tag, const GemmArgs& g, unsigned offered8, void* stream) {
    const bool f8 = g.dtype == VH_DTYPE_FP8;
    GemmArgs h = g;
    if (f8 && !offered8) h.dtype = -1;   // no dtype of a 16-bit tap: the 16-bit rules speak, "gemm: dtype" in its turn
    // an epilogue the tap lacks: the operands and the shape are judged first, as for the plainest launch, then the epilogue is unsupported
    const bool lacks = f8 && offered8 && (g.epilogue < 0 || g.epilogue > VH_EPI_LNFOLD_TGELU || !(offered8 >> g.epilogue & 1));
    if (lacks) { h.epilogue = VH_EPI_BIAS; h.out_tiled = h.ab_tiled = h.tile_begin = h.tile_count = 0; }
    if (const char* why = gemm_check(h))
        return f8 && offered8 ? fail(nullptr, VH_ERR_INVALID, "%s%s", tag, strchr(why, ':')) : fail(nullptr, VH_ERR_INVALID, "%s", why);
    if (lacks) return fail(nullptr, VH_ERR_UNSUPPORTED, "%s: epilogue %d not available", tag, g.epilogue);
    hipError_t e = launch_gemm(g, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? VH_ERR_INVALID : VH_ERR_HIP, "%s failed: %s", tag, hipGetErrorString(e));
    return VH_OK;
}
int vh_op_gemm(const void* a, const void* w, const float* bias, void* out, int64_t M, int N, int K, int epi,
               const float* aux, int aux_i, int dtype, int variant, void* stream) {
    const GemmArgs g{a, w, bias, out, M, N, K, epi, aux, aux_i, dtype, variant};
    return op_gemm_run("gemm", g, 0, stream);
}
int vh_op_gemm_ex(const void* a, const void* w, const float* bias, void* out, int64_t M, int N, int K, int epi,
                  const float* aux, int aux_i, const float* stats, void* out16, float* partials, int dtype, int variant,
                  void* stream) {
    GemmArgs g{a, w, bias, out, M, N, K, epi, aux, aux_i, dtype, variant};
    g.stats = stats; g.out16 = out16; g.partials = partials;
    return op_gemm_run("gemm_ex", g, 0, stream);
}
// test taps: the tiled / head-major layouts and tile ranges (GemmArgs::out_tiled, ab_tiled, tile_begin, tile_count)
int vh_op_gemm_layout(const void* a, const void* w, const float* bias, void* out, int64_t M, int N, int K, int epi,
                      const float* aux, int aux_i, const float* stats, void* out16, float* partials, int dtype, int variant,
                      int out_tiled, int ab_tiled, int tile_begin, int tile_count, void* stream) {
    GemmArgs g{a, w, bias, out, M, N, K, epi, aux, aux_i, dtype, variant};
    g.stats = stats; g.out16 = out16; g.partials = partials;
    g.out_tiled = out_tiled; g.ab_tiled = ab_tiled; g.tile_begin = tile_begin; g.tile_count = tile_count;
    return op_gemm_run("gemm_layout", g, 0, stream);
}
// test taps of the register-token assembly: the PATCH / PATCH_SPLIT epilogues with `lead` rows in front of an image's patch rows
// (GemmArgs::lead; prow = row stride of `partials`, 0 = images x (aux_i + lead)), and the lead-row kernels on the caller's buffers
int vh_op_gemm_lead(const void* a, const void* w, const float* bias, void* out, int64_t M, int N, int K, int epi, const float* aux,
                    int aux_i, int lead, void* out16, float* partials, int64_t prow, int dtype, int variant, void* stream) {
    if (epi != VH_EPI_PATCH && epi != VH_EPI_PATCH_SPLIT) return fail(nullptr, VH_ERR_INVALID, "gemm_lead: epilogue must be VH_EPI_PATCH or VH_EPI_PATCH_SPLIT");
    if (aux_i > 0 && M % aux_i) return fail(nullptr, VH_ERR_INVALID, "gemm_lead: M must be a whole number of images (M %% aux_i == 0)");
    GemmArgs g{a, w, bias, out, M, N, K, epi, aux, aux_i, dtype, variant};
    g.out16 = out16; g.partials = partials; g.prow = prow; g.lead = lead;
    if (epi == VH_EPI_PATCH_SPLIT && aux_i > 0 && prow && prow < (M / aux_i) * (int64_t)(aux_i + lead))
        return fail(nullptr, VH_ERR_INVALID, "gemm_lead: prow is below images x (aux_i + lead)");
    return op_gemm_run("gemm_lead", g, 0, stream);
}
int vh_op_lead_rows(void* x_or_hi, void* lo, float* partials, int64_t prow, const float* cls, const float* pos, const float* reg, int lead,
                    int batch, int tokens, int dim, int dtype, void* stream) {
    // cls NULL (with pos NULL): the form of a VH_FLAG_NO_CLS context, whose `lead` rows are all register rows (1 <= lead <= 16, reg needed)
    const bool no_cls = !cls && !pos;
    if (!x_or_hi || (!no_cls && (!cls || !pos)) || batch <= 0 || dim <= 0 || dim % 64 || lead < 1 || lead > (no_cls ? 0 : 1) + VH_MAX_REGISTERS ||
        lead >= tokens || ((no_cls || lead > 1) && !reg))
        return fail(nullptr, VH_ERR_INVALID, "lead_rows: bad argument (dim %% 64 == 0, 1 <= lead <= 17, lead < tokens, reg for lead > 1)");
    hipError_t e;
    if (lo) {   // the split form: planes + partial sums
        if (!partials || (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) || prow < (int64_t)batch * tokens)
            return fail(nullptr, VH_ERR_INVALID, "lead_rows: the split form needs partials, a 16-bit dtype and prow >= batch x tokens");
        e = launch_lead_rows_split(x_or_hi, lo, partials, prow, cls, pos, reg, lead, batch, tokens, dim, dtype, (hipStream_t)stream);
    } else {
        e = launch_lead_rows((float*)x_or_hi, cls, pos, reg, lead, batch, tokens, dim, (hipStream_t)stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "lead_rows failed: %s", hipGetErrorString(e));
    return VH_OK;
}
// e4m3 operands: w_scale = the per-output-channel weight scales (GemmArgs::wscale), c_dev = the LNFOLD* epilogues' c_n (`aux`)
int vh_op_gemm_fp8(const void* a8, const void* w8, const float* w_scale, const float* bias, void* out, int64_t M, int N, int K,
                   int epi, int variant, void* stream) {
    GemmArgs g{a8, w8, bias, out, M, N, K, epi, nullptr, 0, VH_DTYPE_FP8, variant};
    g.wscale = w_scale;
    return op_gemm_run("gemm_fp8", g, kEpiPlain8, stream);
}
int vh_op_gemm_fp8_ex(const void* a8, const void* w8, const float* w_scale, const float* bias, void* out, int64_t M, int N, int K,
                      int epi, const float* c_dev, const float* stats, void* out16, float* partials, int variant, void* stream) {
    GemmArgs g{a8, w8, bias, out, M, N, K, epi, c_dev, 0, VH_DTYPE_FP8, variant};
    g.wscale = w_scale; g.stats = stats; g.out16 = out16; g.partials = partials;
    return op_gemm_run("gemm_fp8_ex", g, kEpiFold8, stream);
}
int vh_op_gemm_fp8_layout(const void* a8, const void* w8, const float* w_scale, const float* bias, void* out, int64_t M, int N, int K,
                          int epi, const float* c_dev, const float* stats, void* out16, float* partials, int variant,
                          int out_tiled, int ab_tiled, int tile_begin, int tile_count, void* stream) {
    GemmArgs g{a8, w8, bias, out, M, N, K, epi, c_dev, 0, VH_DTYPE_FP8, variant};
    g.wscale = w_scale; g.stats = stats; g.out16 = out16; g.partials = partials;
    g.out_tiled = out_tiled; g.ab_tiled = ab_tiled; g.tile_begin = tile_begin; g.tile_count = tile_count;
    return op_gemm_run("gemm_fp8_layout", g, kEpiPlain8 | kEpiFold8, stream);
}
int vh_op_quantize_rows(const float* w, int rows, int cols, float post_scale, void* w8, float* scale, void* stream) {
    if (!w || !w8 || !scale || rows <= 0 || cols <= 0 || cols % 4) return fail(nullptr, VH_ERR_INVALID, "quantize_rows: bad argument");
    OPCHK(launch_quantize_rows(w, rows, cols, post_scale, w8, scale, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_tile_rows(const void* in, int rows, int cols, void* out, int dtype, void* stream) {
    if (!in || !out) return fail(nullptr, VH_ERR_INVALID, "tile_rows: null pointer");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16 && dtype != VH_DTYPE_FP8) return fail(nullptr, VH_ERR_INVALID, "tile_rows: dtype");
    const int chunk = dtype == VH_DTYPE_FP8 ? 16 : 8;
    if (rows <= 0 || cols <= 0 || rows % 16 || cols % chunk)
        return fail(nullptr, VH_ERR_INVALID, "tile_rows: need rows %% 16 == 0 and cols %% %d == 0", chunk);
    hipError_t e = dtype == VH_DTYPE_FP8 ? launch_tile_bytes(in, rows, cols, out, (hipStream_t)stream)
                                         : launch_cast_tiled_w((const float*)in, rows, cols, out, dtype, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? VH_ERR_INVALID : VH_ERR_HIP, "tile_rows failed: %s", hipGetErrorString(e));
    return VH_OK;
}
// ---- the row-kernel taps (kernels_rows.hip: one wave per row).  Every tap judges pointers, shape and dtype here, before a launch.
static bool row_dt16(int dtype) { return dtype == VH_DTYPE_BF16 || dtype == VH_DTYPE_FP16; }
static bool row_dt(int dtype) { return row_dt16(dtype) || dtype == VH_DTYPE_FP8; }
static bool row_shape(int64_t rows, int dim) { return rows > 0 && dim > 0 && dim % 4 == 0 && dim <= 2048; }
int vh_op_rowstats_cast(const float* x, int64_t rows, int dim, float eps, void* x16, float* stats, int dtype, void* stream) {
    return vh_op_rowstats_guard(x, rows, dim, eps, x16, nullptr, stats, dtype, 0, nullptr, stream);
}
int vh_op_rowstats_split(const float* x, int64_t rows, int dim, float eps, void* hi, void* lo, float* stats, int dtype, void* stream) {
    if (!lo) return fail(nullptr, VH_ERR_INVALID, "rowstats_split: bad argument");
    return vh_op_rowstats_guard(x, rows, dim, eps, hi, lo, stats, dtype, 0, nullptr, stream);
}
int vh_op_rowstats_guard(const float* x, int64_t rows, int dim, float eps, void* hi, void* lo, float* stats, int dtype, int64_t guard_rows,
                         unsigned int* amax_guard, void* stream) {
    if (!x || !hi || !stats || !row_shape(rows, dim)) return fail(nullptr, VH_ERR_INVALID, "rowstats: bad argument (rows > 0, dim %% 4 == 0, dim <= 2048)");
    if (!row_dt(dtype)) return fail(nullptr, VH_ERR_INVALID, "rowstats: dtype");
    if (guard_rows < 0 || guard_rows > rows) return fail(nullptr, VH_ERR_INVALID, "rowstats: guard_rows outside 0..rows");
    if (amax_guard && dtype != VH_DTYPE_FP8) return fail(nullptr, VH_ERR_INVALID, "rowstats: amax_guard belongs to VH_DTYPE_FP8");
    OPCHK(lo ? launch_rowstats_split(x, rows, dim, eps, hi, lo, stats, dtype, (hipStream_t)stream, guard_rows, amax_guard)
             : launch_rowstats_cast(x, rows, dim, eps, hi, stats, dtype, (hipStream_t)stream, guard_rows, amax_guard));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_pre_layernorm(const float* x, int64_t rows, int dim, const float* gamma, const float* beta, float eps, float* y32, void* hi,
                        void* lo, float* stats, int dtype, void* stream) {
    return vh_op_pre_layernorm_guard(x, rows, dim, gamma, beta, eps, y32, hi, lo, stats, dtype, 0, nullptr, nullptr, stream);
}
int vh_op_pre_layernorm_guard(const float* x, int64_t rows, int dim, const float* gamma, const float* beta, float eps, float* y32, void* hi,
                              void* lo, float* stats, int dtype, int64_t guard_rows, unsigned int* guard, unsigned int* amax_guard,
                              void* stream) {
    if (!x || !gamma || !beta) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: null pointer");
    if (!y32 && !hi) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: one of y32 / hi is needed");
    if (lo && !hi) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: the lo plane needs the hi plane");
    if (!row_shape(rows, dim)) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: need rows > 0, dim %% 4 == 0, dim <= 2048");
    if (!(eps > 0.f)) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: eps must be positive");
    if (!row_dt(dtype)) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: dtype");
    if (guard_rows < 0 || guard_rows > rows) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: guard_rows outside 0..rows");
    if (amax_guard && dtype != VH_DTYPE_FP8) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: amax_guard belongs to VH_DTYPE_FP8");
    if ((guard || amax_guard) && !hi && !stats) return fail(nullptr, VH_ERR_INVALID, "pre_layernorm: the guards need hi or stats");
    OPCHK(launch_pre_layernorm(x, rows, dim, gamma, beta, eps, y32, hi, lo, stats, dtype, (hipStream_t)stream, guard_rows, guard, amax_guard));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_finalize_stats(const float* partials, int nblk, int64_t rows, int dim, float eps, float* stats, void* stream) {
    return vh_op_finalize_stats_guard(partials, nblk, rows, dim, eps, stats, 0, nullptr, nullptr, stream);
}
int vh_op_finalize_stats_guard(const float* partials, int nblk, int64_t rows, int dim, float eps, float* stats, int64_t guard_rows,
                               unsigned int* guard, unsigned int* amax_guard, void* stream) {
    if (!partials || !stats || nblk <= 0 || rows <= 0 || dim <= 0) return fail(nullptr, VH_ERR_INVALID, "finalize_stats: bad argument");
    if (guard_rows < 0 || guard_rows > rows) return fail(nullptr, VH_ERR_INVALID, "finalize_stats: guard_rows outside 0..rows");
    OPCHK(launch_finalize_stats(partials, nblk, rows, dim, eps, stats, (hipStream_t)stream, guard_rows, guard, amax_guard));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_ln_guard(const float* stats, int64_t rows, unsigned int* guard, void* stream) {
    if (!stats || !guard || rows <= 0) return fail(nullptr, VH_ERR_INVALID, "ln_guard: bad argument");
    OPCHK(launch_ln_guard(stats, rows, guard, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_fold_ln(const float* w, const float* b, const float* gamma, const float* beta, int rows, int dim, float scale,
                  void* w16, float* c, float* d, int dtype, void* stream) {
    if (!w || !b || !gamma || !beta || !w16 || !c || !d || rows <= 0 || dim <= 0) return fail(nullptr, VH_ERR_INVALID, "fold_ln: bad argument");
    if (!row_dt16(dtype)) return fail(nullptr, VH_ERR_INVALID, "fold_ln: dtype (e4m3 weights: vh_op_fold_ln_f8)");
    OPCHK(launch_fold_ln(w, b, gamma, beta, rows, dim, scale, w16, c, d, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_fold_ln_f8(const float* w, const float* b, const float* gamma, const float* beta, int rows, int dim, float scale,
                     void* w8, float* wscale, float* c, float* d, void* stream) {
    if (!w || !b || !gamma || !beta || !w8 || !wscale || !c || !d || rows <= 0 || dim <= 0 || dim % 4)
        return fail(nullptr, VH_ERR_INVALID, "fold_ln_f8: bad argument (dim %% 4 == 0)");
    OPCHK(launch_fold_ln_f8(w, b, gamma, beta, rows, dim, scale, w8, wscale, c, d, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_fake_quant_rows(const float* w, int rows, int cols, float* out, void* stream) {
    if (!w || !out || rows <= 0 || cols <= 0 || cols % 4) return fail(nullptr, VH_ERR_INVALID, "fake_quant_rows: bad argument (cols %% 4 == 0)");
    OPCHK(launch_fake_quant_rows(w, rows, cols, out, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_layernorm(const float* x, int64_t rows, int dim, int64_t row_stride, const float* gamma, const float* beta,
                    float eps, void* out16, int dtype, void* stream) {
    if (!x || !gamma || !beta || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (!row_shape(rows, dim) || row_stride % 4) return fail(nullptr, VH_ERR_INVALID, "layernorm: unsupported shape");
    if (!row_dt(dtype)) return fail(nullptr, VH_ERR_INVALID, "layernorm: dtype (the fp32 result: vh_op_layernorm_f32)");
    OPCHK(launch_layernorm(x, rows, dim, row_stride, gamma, beta, eps, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_layernorm_f32(const float* x, int64_t rows, int dim, int64_t row_stride, const float* gamma, const float* beta,
                        float eps, float* out32, void* stream) {
    if (!x || !gamma || !beta || !out32) return fail(nullptr, VH_ERR_INVALID, "layernorm_f32: null pointer");
    if (!row_shape(rows, dim) || row_stride % 4 || row_stride < dim) return fail(nullptr, VH_ERR_INVALID, "layernorm_f32: unsupported shape");
    OPCHK(launch_layernorm(x, rows, dim, row_stride, gamma, beta, eps, out32, VH_DTYPE_F32_INTERNAL, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_layernorm_split(const void* hi, const void* lo, int64_t rows, int dim, int64_t row_stride, const float* gamma,
                          const float* beta, float eps, float* out32, int dtype, void* stream) {
    if (!hi || !lo || !gamma || !beta || !out32) return fail(nullptr, VH_ERR_INVALID, "layernorm_split: null pointer");
    if (!row_shape(rows, dim) || row_stride < dim) return fail(nullptr, VH_ERR_INVALID, "layernorm_split: unsupported shape");
    if (!row_dt(dtype)) return fail(nullptr, VH_ERR_INVALID, "layernorm_split: dtype");
    OPCHK(launch_layernorm_split(hi, lo, rows, dim, row_stride, gamma, beta, eps, out32, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_head_f32(const float* y, const float* w, const float* bias, float* out, int batch, int classes, int dim, void* stream) {
    if (!y || !w || !bias || !out) return fail(nullptr, VH_ERR_INVALID, "head_f32: null pointer");
    if (batch <= 0 || classes <= 0 || classes % 4 || dim <= 0 || dim % 16)
        return fail(nullptr, VH_ERR_INVALID, "head_f32: need batch > 0, classes %% 4 == 0, dim %% 16 == 0");
    OPCHK(launch_head_f32(y, w, bias, out, batch, classes, dim, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_attention(const void* qkv16, int batch, int tokens, int heads, void* out16, int dtype, void* stream) {
    if (!qkv16 || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (batch <= 0 || tokens <= 0 || heads <= 0 || tokens > kAttnStreamMaxTokens ||
        (attention_lds_bytes(tokens) > 160 * 1024 && heads > 32))
        return fail(nullptr, VH_ERR_INVALID, "attention: unsupported shape");
    // The work-queue counter is owned by THIS call (allocated, used, freed): taps may run concurrently from several host
    // threads, and a context carries its own counters in its arena.
    unsigned int* ticket = nullptr;
    OPCHK(hipMalloc((void**)&ticket, 256));
    hipError_t e = launch_attention(qkv16, batch, tokens, heads, out16, dtype, ticket, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    hipFree(ticket);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "attention failed: %s", hipGetErrorString(e));
    return VH_OK;
}
int vh_op_attention_stream(const void* qkv16, int batch, int tokens, int heads, void* out16, int dtype, void* stream) {
    if (!qkv16 || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (batch <= 0 || tokens <= 0 || tokens > kAttnStreamMaxTokens || heads <= 0 || heads > 32)
        return fail(nullptr, VH_ERR_INVALID, "attention_stream: unsupported shape");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16 && dtype != VH_DTYPE_FP8)
        return fail(nullptr, VH_ERR_INVALID, "attention_stream: unsupported dtype");
    OPCHK(launch_attention_hd(qkv16, batch, tokens, heads, 64, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_attention_hd(const void* qkv16, int batch, int tokens, int heads, int head_dim, void* out16, int dtype, void* stream) {
    if (!qkv16 || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (!attention_hd_supported(head_dim)) return fail(nullptr, VH_ERR_INVALID, "attention_hd: head_dim must be 32, 48, ..., 128");
    if (batch <= 0 || tokens <= 0 || tokens > kAttnStreamMaxTokens || heads <= 0 || heads > kAttnHdMaxWidth / head_dim)
        return fail(nullptr, VH_ERR_INVALID, "attention_hd: unsupported shape");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16 && dtype != VH_DTYPE_FP8)
        return fail(nullptr, VH_ERR_INVALID, "attention_hd: unsupported dtype");
    OPCHK(launch_attention_hd(qkv16, batch, tokens, heads, head_dim, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_attention_cls(const void* qkv16, int batch, int tokens, int heads, void* out16, int dtype, void* stream) {
    if (!qkv16 || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (batch <= 0 || tokens <= 0 || tokens > 1024 || heads <= 0) return fail(nullptr, VH_ERR_INVALID, "attention_cls: unsupported shape");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return fail(nullptr, VH_ERR_INVALID, "attention_cls: unsupported dtype");
    OPCHK(launch_attention_cls(qkv16, batch, tokens, heads, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_attention_layout(const void* qkv16, int batch, int tokens, int heads, void* out16, int dtype, int out_tiled, int64_t in_hm_rows,
                           void* stream) {
    if (!qkv16 || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (batch <= 0 || tokens <= 0 || heads <= 0 || tokens > kAttnStreamMaxTokens ||
        (attention_lds_bytes(tokens) > 160 * 1024 && heads > 32))
        return fail(nullptr, VH_ERR_INVALID, "attention_layout: unsupported shape");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16 && dtype != VH_DTYPE_FP8)
        return fail(nullptr, VH_ERR_INVALID, "attention_layout: unsupported dtype");
    // what launch_attention refuses, refused here with a reason and before anything is allocated
    if (in_hm_rows < 0 || (in_hm_rows && !out_tiled)) return fail(nullptr, VH_ERR_INVALID, "attention_layout: head-major q|k|v needs the tiled output");
    if (in_hm_rows && (in_hm_rows < (int64_t)batch * tokens || in_hm_rows * heads * 64 * 4 >= (1ll << 32)))
        return fail(nullptr, VH_ERR_INVALID, "attention_layout: in_hm_rows must hold batch * tokens rows (and 4 * in_hm_rows * heads * 64 < 2^32)");
    if (out_tiled && !attention_tiled_applies(batch, tokens, heads))
        return fail(nullptr, VH_ERR_INVALID, "attention_layout: the tiled output exists in the ring forms with an even head count only");
    unsigned int* ticket = nullptr;   // owned by this call, as in vh_op_attention
    OPCHK(hipMalloc((void**)&ticket, 256));
    hipError_t e = launch_attention(qkv16, batch, tokens, heads, out16, dtype, ticket, (hipStream_t)stream, false, out_tiled != 0, in_hm_rows);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    hipFree(ticket);
    if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? VH_ERR_INVALID : VH_ERR_HIP, "attention_layout failed: %s", hipGetErrorString(e));
    return VH_OK;
}
int vh_op_attention_probs(const void* qkv16, int batch, int tokens, int heads, int head_dim, int queries, int64_t in_hm_rows, int dtype,
                          float* probs, void* stream) {
    if (!qkv16 || !probs) return fail(nullptr, VH_ERR_INVALID, "attention_probs: null pointer");
    if (batch <= 0) return fail(nullptr, VH_ERR_INVALID, "attention_probs: batch %d must be positive", batch);
    if (tokens < 1 || tokens > kAttnStreamMaxTokens) return fail(nullptr, VH_ERR_INVALID, "attention_probs: tokens %d outside 1..%d", tokens, kAttnStreamMaxTokens);
    if (!attention_hd_supported(head_dim)) return fail(nullptr, VH_ERR_INVALID, "attention_probs: head_dim %d is not 32, 48, ..., 128", head_dim);
    if (heads <= 0 || heads > kAttnHdMaxWidth / head_dim)
        return fail(nullptr, VH_ERR_INVALID, "attention_probs: heads %d x head_dim %d outside 1..%d", heads, head_dim, kAttnHdMaxWidth);
    if (queries < 1 || queries > kAttnMapsMaxQueries || queries > tokens)
        return fail(nullptr, VH_ERR_INVALID, "attention_probs: queries %d outside 1..min(%d, tokens)", queries, kAttnMapsMaxQueries);
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return fail(nullptr, VH_ERR_INVALID, "attention_probs: dtype %d is not VH_DTYPE_BF16 or VH_DTYPE_FP16", dtype);
    if (in_hm_rows && head_dim != 64) return fail(nullptr, VH_ERR_INVALID, "attention_probs: head-major q|k|v (in_hm_rows != 0) exists at head_dim 64 only, not %d", head_dim);
    if (in_hm_rows && in_hm_rows < (int64_t)batch * tokens)
        return fail(nullptr, VH_ERR_INVALID, "attention_probs: in_hm_rows %lld holds fewer than batch * tokens = %lld rows", (long long)in_hm_rows, (long long)batch * tokens);
    if (((uintptr_t)qkv16 | (uintptr_t)probs) & 15)
        return fail(nullptr, VH_ERR_INVALID, "attention_probs: a pointer is not 16-byte aligned (qkv16 %p, probs %p)", qkv16, (void*)probs);
    if (const char* why = attention_probs_check(in_hm_rows, batch, tokens, heads, head_dim, queries, dtype)) return fail(nullptr, VH_ERR_INVALID, "attention_probs: %s", why);
    OPCHK(launch_attention_probs(qkv16, in_hm_rows, batch, tokens, heads, head_dim, queries, dtype, probs, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_attention_readout(const float* store, int batch, int heads, int queries, int tokens, int lead, int elem, int keys, void* probs_out,
                            void* head_mean_out, void* stream) {
    if (!store) return fail(nullptr, VH_ERR_INVALID, "attention_readout: null store");
    if (!probs_out && !head_mean_out) return fail(nullptr, VH_ERR_INVALID, "attention_readout: no output requested (probs_out and head_mean_out are both NULL)");
    if (batch <= 0) return fail(nullptr, VH_ERR_INVALID, "attention_readout: batch %d must be positive", batch);
    if (heads <= 0 || heads > kAttnHdMaxWidth / 32) return fail(nullptr, VH_ERR_INVALID, "attention_readout: heads %d outside 1..%d", heads, kAttnHdMaxWidth / 32);
    if (tokens < 1 || tokens > kAttnStreamMaxTokens) return fail(nullptr, VH_ERR_INVALID, "attention_readout: tokens %d outside 1..%d", tokens, kAttnStreamMaxTokens);
    if (queries < 1 || queries > kAttnMapsMaxQueries || queries > tokens)
        return fail(nullptr, VH_ERR_INVALID, "attention_readout: queries %d outside 1..min(%d, tokens)", queries, kAttnMapsMaxQueries);
    if (lead < 0 || lead >= tokens) return fail(nullptr, VH_ERR_INVALID, "attention_readout: lead %d outside 0..tokens-1", lead);
    if (elem != VH_ELEM_F32 && elem != VH_ELEM_F16 && elem != VH_ELEM_BF16)
        return fail(nullptr, VH_ERR_INVALID, "attention_readout: elem %d is not VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16", elem);
    if (keys != VH_ATTN_KEYS_ALL && keys != VH_ATTN_KEYS_PATCH)
        return fail(nullptr, VH_ERR_INVALID, "attention_readout: keys %d is not VH_ATTN_KEYS_ALL (0) or VH_ATTN_KEYS_PATCH (1)", keys);
    if (((uintptr_t)store | (uintptr_t)probs_out | (uintptr_t)head_mean_out) & 15)
        return fail(nullptr, VH_ERR_INVALID, "attention_readout: a pointer is not 16-byte aligned (store %p, probs_out %p, head_mean_out %p)", (const void*)store,
                    probs_out, head_mean_out);
    if (const char* why = attention_readout_check(batch, heads, queries, tokens, lead, elem, keys)) return fail(nullptr, VH_ERR_INVALID, "attention_readout: %s", why);
    OPCHK(launch_attention_readout(store, batch, heads, queries, tokens, lead, elem, keys, probs_out, head_mean_out, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_im2col(const float* in, int batch, int image, int patch, int channels, void* out16, int dtype, void* stream) {
    if (!in || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (batch <= 0 || patch <= 0 || image <= 0 || image % patch || (patch * channels) % 4)
        return fail(nullptr, VH_ERR_INVALID, "im2col: unsupported shape");
    OPCHK(launch_im2col(in, batch, image, patch, channels, patch * patch * channels, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_im2col_padded(const float* in, int batch, int image, int patch, int channels, int kpad, void* out16, int dtype,
                        void* stream) {
    if (!in || !out16) return fail(nullptr, VH_ERR_INVALID, "null pointer");
    if (batch <= 0 || patch <= 0 || image <= 0 || image % patch || channels <= 0 || patch > 256 || channels > 64 ||
        kpad < patch * patch * channels || kpad % 8)
        return fail(nullptr, VH_ERR_INVALID, "im2col_padded: unsupported shape");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return fail(nullptr, VH_ERR_INVALID, "im2col_padded: unsupported dtype");
    OPCHK(launch_im2col(in, batch, image, patch, channels, kpad, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_im2col_u8(const uint8_t* in, int batch, int image, int patch, int channels, int kpad, const float* scale_host,
                    const float* shift_host, void* out16, int dtype, void* stream) {
    if (!in || !out16 || !scale_host || !shift_host) return fail(nullptr, VH_ERR_INVALID, "null buffer");
    if (batch <= 0 || patch <= 0 || image <= 0 || image % patch || channels <= 0 || patch > 256 || channels > kMaxChannels ||
        kpad < patch * patch * channels || kpad % 8)
        return fail(nullptr, VH_ERR_INVALID, "im2col_u8: unsupported shape");
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return fail(nullptr, VH_ERR_INVALID, "im2col_u8: unsupported dtype");
    if ((uintptr_t)in & 15) return fail(nullptr, VH_ERR_INVALID, "im2col_u8: input %p is not 16-byte aligned", (const void*)in);
    for (int i = 0; i < channels; ++i)
        if (!std::isfinite(scale_host[i]) || !std::isfinite(shift_host[i])) return fail(nullptr, VH_ERR_INVALID, "im2col_u8: scale / shift of channel %d is not finite", i);
    OPCHK(launch_im2col_u8(in, batch, image, patch, channels, kpad, scale_host, shift_host, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
int vh_op_im2col_tensor(const void* in, int elem, int layout, int batch, int image, int patch, int channels, int kpad, const float* scale_host,
                        const float* shift_host, void* out16, int dtype, void* stream) {
    if (int rc = check_tensor_kind(nullptr, elem, layout)) return rc;
    if (!in || !out16 || (elem == VH_ELEM_U8 && (!scale_host || !shift_host))) return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: null buffer");
    if (batch <= 0) return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: batch %d must be positive", batch);
    if (patch <= 0 || patch > 256 || image <= 0 || image % patch)
        return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: image %d is no multiple of patch %d (1..256)", image, patch);
    if (channels <= 0 || channels > kMaxChannels) return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: channels %d outside 1..%d", channels, kMaxChannels);
    if (kpad < patch * patch * channels || kpad % 8)
        return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: kpad %d must be a multiple of 8 and at least patch * patch * channels = %d", kpad, patch * patch * channels);
    if (dtype != VH_DTYPE_BF16 && dtype != VH_DTYPE_FP16) return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: unsupported dtype %d", dtype);
    if ((uintptr_t)in & 15) return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: input %p is not 16-byte aligned", in);
    if (elem == VH_ELEM_U8)
        for (int i = 0; i < channels; ++i)
            if (!std::isfinite(scale_host[i]) || !std::isfinite(shift_host[i])) return fail(nullptr, VH_ERR_INVALID, "im2col_tensor: scale / shift of channel %d is not finite", i);
    OPCHK(launch_im2col_tensor(in, elem, layout, batch, image, patch, channels, kpad, scale_host, shift_host, out16, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}

// The resize of one format on its own: plan, upload, launch, wait.  m12 and chroma_site: of the formats that have a colour state.
static int op_resize(const FrameFormat& fmt, const uint8_t* frames, size_t nbytes, const void* desc, int batch, int channels, int out_size,
                     const float* m12, int chroma_site, uint8_t* out, void* stream) {
    // every check before a device is touched
    const bool colour = fmt.colour >= 0;
    if (!frames || !desc || !out || (colour && !m12)) return fail(nullptr, VH_ERR_INVALID, "%s", fmt.op_null);
    for (int i = 0; colour && i < 12; ++i)
        if (!std::isfinite(m12[i])) return fail(nullptr, VH_ERR_INVALID, "%s: colour matrix entry %d is not finite", fmt.tag, i);
    std::vector<uint32_t> words;
    int max_tiles = 0;
    if (const char* why = fmt.plan(desc, batch, channels, out_size, nbytes, (uintptr_t)frames, chroma_site, &words, &max_tiles))
        return fail(nullptr, VH_ERR_INVALID, "%s", why);
    uint32_t* plan = nullptr;
    OPCHK(hipMalloc((void**)&plan, words.size() * 4));
    hipError_t e = hipMemcpyAsync(plan, words.data(), words.size() * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = fmt.launch(frames, plan, batch, channels, out_size, max_tiles, m12, out, (hipStream_t)stream);
    const hipError_t es = hipStreamSynchronize((hipStream_t)stream);
    hipFree(plan);
    OPCHK(e);
    OPCHK(es);
    return VH_OK;
}

int vh_op_resize_u8(const uint8_t* frames, size_t nbytes, const vh_frame* desc, int batch, int channels, int out_size, uint8_t* out,
                    void* stream) {
    return op_resize(kFramesRGB, frames, nbytes, desc, batch, channels, out_size, nullptr, 0, out, stream);
}
int vh_op_resize_nv12(const uint8_t* frames, size_t nbytes, const vh_frame_nv12* desc, int batch, int out_size, const float* m12,
                      int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesNV12, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_yuv(const uint8_t* frames, size_t nbytes, const vh_frame_yuv* desc, int batch, int out_size, const float* m12,
                     int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesYUV, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_p016(const uint8_t* frames, size_t nbytes, const vh_frame_nv12* desc, int batch, int out_size, const float* m12,
                      int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesP016, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_yuv16(const uint8_t* frames, size_t nbytes, const vh_frame_yuv* desc, int batch, int out_size, const float* m12,
                       int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesYUV16, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_yuy2(const uint8_t* frames, size_t nbytes, const vh_frame_yuy2* desc, int batch, int out_size, const float* m12,
                      int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesYUY2, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_y210(const uint8_t* frames, size_t nbytes, const vh_frame_yuy2* desc, int batch, int out_size, const float* m12,
                      int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesY210, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_bgra(const uint8_t* frames, size_t nbytes, const vh_frame_bgra* desc, int batch, int out_size, const float* m12,
                      int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesBGRA, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}
int vh_op_resize_y410(const uint8_t* frames, size_t nbytes, const vh_frame_bgra* desc, int batch, int out_size, const float* m12,
                      int chroma_site, uint8_t* out, void* stream) {
    return op_resize(kFramesY410, frames, nbytes, desc, batch, 3, out_size, m12, chroma_site, out, stream);
}

int vh_op_cast(const float* in, void* out16, int64_t n, int dtype, void* stream) {
    if (!in || !out16 || n <= 0 || n % 4) return fail(nullptr, VH_ERR_INVALID, "cast: bad argument");
    OPCHK(launch_cast(in, out16, n, dtype, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}
// the token-feature kernels on caller-made rows; the normalised mean's row statistics take a scratch of the tap's own (a test
// and measurement tap: the context calls use the context's statistics buffer and allocate nothing)
static int op_token_features_run(FeatureArgs a, void* stream) {
    if (const char* why = features_check(a)) return fail(nullptr, VH_ERR_INVALID, "%s", why);
    if (a.mean && a.norm == VH_FEAT_NORM) OPCHK(hipMalloc((void**)&a.stats, (size_t)a.batch * a.tokens * 2 * sizeof(float)));
    hipError_t e = launch_token_features(a, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (a.stats) hipFree(a.stats);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "token_features failed: %s", hipGetErrorString(e));
    return VH_OK;
}
int vh_op_token_features(const void* hi, const void* lo, int form, int batch, int tokens, int dim, const float* gamma, const float* beta,
                         float eps, int elem, int norm, void* patch_out, void* mean_out, void* stream) {
    return op_token_features_run(FeatureArgs{hi, lo, form, batch, tokens, dim, gamma, beta, eps, elem, norm, nullptr, patch_out, mean_out, nullptr}, stream);
}
int vh_op_token_features2(const void* hi, const void* lo, int form, int batch, int tokens, int lead, int dim, const float* gamma,
                          const float* beta, float eps, int elem, int norm, void* patch_out, int patch_layout, void* mean_out, void* reg_out,
                          void* stream) {
    FeatureArgs a{hi, lo, form, batch, tokens, dim, gamma, beta, eps, elem, norm, nullptr, patch_out, mean_out, nullptr};
    a.lead = lead;
    a.reg = reg_out;
    a.patch_layout = patch_layout;
    return op_token_features_run(a, stream);
}
// the pooled head's one-pass kernel on caller-made rows (VH_FLAG_POOL)
int vh_op_pool_rows(const void* hi, const void* lo, int form, int batch, int tokens, int lead, int dim, const float* gamma, const float* beta,
                    float eps, int norm, float* mean_out, void* stream) {
    const PoolArgs a{hi, lo, form, batch, tokens, lead, dim, gamma, beta, eps, norm, mean_out};
    if (const char* why = pool_check(a)) return fail(nullptr, VH_ERR_INVALID, "%s", why);
    hipError_t e = launch_pool_rows(a, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "pool_rows failed: %s", hipGetErrorString(e));
    return VH_OK;
}
// the attention-pooling head's one-pass kernel on caller-made rows (VH_FLAG_MAP_HEAD)
int vh_op_map_pool(const void* hi, const void* lo, int form, int batch, int tokens, int lead, int dim, const float* gamma, const float* beta,
                   float eps, const float* qk, int heads, float* z_out, void* stream) {
    const PoolArgs a{hi, lo, form, batch, tokens, lead, dim, gamma, beta, eps, VH_FEAT_NORM, z_out};
    if (const char* why = map_pool_check(a, qk, heads)) return fail(nullptr, VH_ERR_INVALID, "%s", why);
    hipError_t e = launch_map_pool(a, qk, heads, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "map_pool failed: %s", hipGetErrorString(e));
    return VH_OK;
}
// the VH_FLAG_ROPE rotation on caller-made q|k|v
int vh_op_rope(void* qkv16, int dtype, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows, const float* cos_t,
               const float* sin_t, void* stream) {
    if (const char* why = rope_check(qkv16, dtype, batch, tokens, heads, head_dim, lead, hm_rows, cos_t, sin_t)) return fail(nullptr, VH_ERR_INVALID, "rope: %s", why);
    hipError_t e = launch_rope(qkv16, dtype, batch, tokens, heads, head_dim, lead, hm_rows, cos_t, sin_t, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "rope failed: %s", hipGetErrorString(e));
    return VH_OK;
}
// the VH_FLAG_SWIGLU gate pass on caller-made fc1 output
int vh_op_swiglu(const void* gu16, int dtype, int64_t rows, int mlp_dim, void* h16, int out_tiled, void* stream) {
    if (const char* why = swiglu_check(gu16, dtype, rows, mlp_dim, h16, out_tiled)) return fail(nullptr, VH_ERR_INVALID, "swiglu: %s", why);
    hipError_t e = launch_swiglu(gu16, dtype, rows, mlp_dim, h16, out_tiled, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, VH_ERR_HIP, "swiglu failed: %s", hipGetErrorString(e));
    return VH_OK;
}
int vh_op_fill(float* out, int64_t n, uint64_t seed, uint32_t tensor_id, int kind, float sigma, void* stream) {
    if (!out || n <= 0 || kind < 0 || kind > 2) return fail(nullptr, VH_ERR_INVALID, "fill: bad argument");
    OPCHK(launch_fill(out, n, seed, tensor_id, kind, kind == 2 ? 0.f : sigma, kind == 2 ? sigma : 0.f, (hipStream_t)stream));
    OPCHK(hipStreamSynchronize((hipStream_t)stream));
    return VH_OK;
}

// micro-benchmark of one GEMM shape: synthetic operands generated in HBM, `iters` back-to-back
// launches between two hip events; returns the average launch time
int vh_bench_gemm(int device, int64_t M, int N, int K, int epilogue, int dtype, int variant, int iters, double* avg_ms) {
    if (!avg_ms || iters <= 0) return fail(nullptr, VH_ERR_INVALID, "vh_bench_gemm: bad argument");
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    float *a32 = nullptr, *w32 = nullptr, *bias = nullptr, *aux = nullptr, *stats = nullptr, *partials = nullptr;
    void *a16 = nullptr, *w16 = nullptr, *out = nullptr, *out16 = nullptr;
    const int aux_i = 196;
    // the layer epilogues of the folded path: LNFOLD* read per-row (mean, rstd) and c_n (`aux`), RESID_LN / RESID_SPLIT
    // write a second 16-bit plane and the per-64-column row sums
    const bool fold = epilogue == VH_EPI_LNFOLD || epilogue == VH_EPI_LNFOLD_GELU || epilogue == VH_EPI_LNFOLD_QGELU || epilogue == VH_EPI_LNFOLD_TGELU;
    const bool resid2 = epilogue == VH_EPI_RESID_LN || epilogue == VH_EPI_RESID_SPLIT || epilogue == VH_EPI_PATCH_SPLIT;
    const size_t out_rows = (epilogue == VH_EPI_PATCH || epilogue == VH_EPI_PATCH_SPLIT) ? (size_t)(M / aux_i + 1) * (aux_i + 1) : (size_t)M;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        hipFree(a32); hipFree(w32); hipFree(bias); hipFree(aux); hipFree(a16); hipFree(w16); hipFree(out);
        hipFree(stats); hipFree(partials); hipFree(out16);
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
    };
#define BCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail(nullptr, VH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } } while (0)
    BCHK(hipMalloc((void**)&a32, (size_t)M * K * 4));
    BCHK(hipMalloc((void**)&w32, (size_t)N * K * 4));
    BCHK(hipMalloc((void**)&bias, (size_t)N * 4));
    BCHK(hipMalloc((void**)&aux, (size_t)(aux_i + 1) * N * 4));
    BCHK(hipMalloc(&a16, (size_t)M * K * 2));
    BCHK(hipMalloc(&w16, (size_t)N * K * 2));
    BCHK(hipMalloc(&out, out_rows * N * 4));
    BCHK(hipMemset(out, 0, out_rows * N * 4));
    BCHK(launch_fill(a32, (int64_t)M * K, 1, 1, 0, 0.f, 0.f, nullptr));
    BCHK(launch_fill(w32, (int64_t)N * K, 1, 2, 1, 0.02f, 0.f, nullptr));
    BCHK(launch_fill(bias, N, 1, 3, 1, 0.02f, 0.f, nullptr));
    BCHK(launch_fill(aux, (int64_t)(aux_i + 1) * N, 1, 4, 1, 0.02f, 0.f, nullptr));
    BCHK(launch_cast(a32, a16, (int64_t)M * K, dtype, nullptr));
    BCHK(launch_cast(w32, w16, (int64_t)N * K, dtype, nullptr));
    GemmArgs g{a16, w16, bias, out, M, N, K, epilogue, aux, aux_i, dtype, variant};
    if (fold) {   // (mean, rstd) ~ (0.02 sigma, 1 + 0.02 sigma): the values do not matter for the time
        BCHK(hipMalloc((void**)&stats, (size_t)M * 2 * 4));
        BCHK(launch_fill(stats, (int64_t)M * 2, 1, 5, 1, 0.02f, 0.f, nullptr));
        g.stats = stats;
    }
    if (resid2) {
        BCHK(hipMalloc(&out16, out_rows * N * 2));
        BCHK(hipMemset(out16, 0, out_rows * N * 2));
        BCHK(hipMalloc((void**)&partials, (size_t)((N + 63) / 64) * out_rows * 2 * 4));
        if (epilogue == VH_EPI_PATCH_SPLIT) g.prow = (int64_t)out_rows;
        g.out16 = out16;
        g.partials = partials;
    }
    if (const char* why = gemm_check(g)) { cleanup(); return fail(nullptr, VH_ERR_INVALID, "%s", why); }
    BCHK(hipEventCreate(&e0));
    BCHK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) BCHK(launch_gemm(g, nullptr));
    BCHK(hipDeviceSynchronize());
    BCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) BCHK(launch_gemm(g, nullptr));
    BCHK(hipEventRecord(e1, nullptr));
    BCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    BCHK(hipEventElapsedTime(&ms, e0, e1));
#undef BCHK
    *avg_ms = ms / iters;
    cleanup();
    return VH_OK;
}

// ---- MLP mode ------------------------------------------------------------------------------------
// ---- filter_image pipeline --------------------------------------------------------------------------------------
// submit: H2D of one frame -> 3x3 filter -> D2H, all asynchronous, chained by events (the reference's
// clEnqueueWriteBuffer -> clEnqueueTask -> clEnqueueReadBuffer chain, netFPGA.cpp:323-329); collect: wait for the
// OLDEST frame (clWaitForEvents on g_im_read_event[rd], :350).  Full / empty ring = VH_ERR_RING_FULL / _EMPTY.
int vh_filter_destroy(vh_filter* f) {
    if (!f) return VH_OK;
    hipSetDevice(f->device);
    if (f->copy_in) hipStreamSynchronize(f->copy_in);
    if (f->compute) hipStreamSynchronize(f->compute);
    if (f->copy_out) hipStreamSynchronize(f->copy_out);
    for (auto& s : f->slot) {
        if (s.h_in) hipHostFree(s.h_in);
        if (s.h_out) hipHostFree(s.h_out);
        if (s.d_in) hipFree(s.d_in);
        if (s.d_out) hipFree(s.d_out);
        if (s.in_done) hipEventDestroy(s.in_done);
        if (s.k_done) hipEventDestroy(s.k_done);
        if (s.out_done) hipEventDestroy(s.out_done);
    }
    if (f->copy_in) hipStreamDestroy(f->copy_in);
    if (f->compute) hipStreamDestroy(f->compute);
    if (f->copy_out) hipStreamDestroy(f->copy_out);
    delete f;
    return VH_OK;
}

int vh_filter_create(int device, int height, int width, int slots, int kind, vh_filter** out) {
    if (!out) return fail(nullptr, VH_ERR_INVALID, "vh_filter_create: null argument");
    *out = nullptr;
    if (height <= 0 || width <= 0 || height > 16384 || width > 16384) return fail(nullptr, VH_ERR_INVALID, "vh_filter_create: frame size outside 1..16384");
    if (slots < 1 || slots > 64) return fail(nullptr, VH_ERR_INVALID, "vh_filter_create: slots must be 1..64");
    if (kind != VH_FILTER_BLUR3 && kind != VH_FILTER_SOBEL3) return fail(nullptr, VH_ERR_INVALID, "vh_filter_create: unknown filter kind %d", kind);
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    vh_filter* f = new vh_filter();
    f->device = device; f->height = height; f->width = width; f->kind = kind;
    const size_t n = (size_t)height * width;
    hipError_t e = hipStreamCreateWithFlags(&f->copy_in, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->compute, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->copy_out, hipStreamNonBlocking);
    f->slot.resize(slots);
    for (auto& s : f->slot) {
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_in, n, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s.h_out, n, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void**)&s.d_in, n);
        if (e == hipSuccess) e = hipMalloc((void**)&s.d_out, n);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.k_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.out_done, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        vh_filter_destroy(f);
        return fail(nullptr, VH_ERR_HIP, "vh_filter_create: %s", hipGetErrorString(e));
    }
    *out = f;
    return VH_OK;
}

const char* vh_filter_last_error(const vh_filter* f) { return f ? f->err.c_str() : g_err.c_str(); }

int vh_filter_free_slots(const vh_filter* f, int* n) {
    if (!f || !n) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *n = (int)f->slot.size() - f->used;
    return VH_OK;
}

int vh_filter_submit(vh_filter* f, const uint8_t* frame) {
    if (!f || !frame) return fail(f ? &f->err : nullptr, VH_ERR_INVALID, "null argument");
    if (f->used == (int)f->slot.size()) return fail(&f->err, VH_ERR_RING_FULL, "ring full (PILA LLENA)");
    HIPCHK(&f->err, hipSetDevice(f->device));
    vh_filter::Slot& s = f->slot[f->wr];
    const size_t n = (size_t)f->height * f->width;
    memcpy(s.h_in, frame, n);
    HIPCHK(&f->err, hipMemcpyAsync(s.d_in, s.h_in, n, hipMemcpyHostToDevice, f->copy_in));
    HIPCHK(&f->err, hipEventRecord(s.in_done, f->copy_in));
    HIPCHK(&f->err, hipStreamWaitEvent(f->compute, s.in_done, 0));
    HIPCHK(&f->err, launch_filter3x3(s.d_in, s.d_out, f->height, f->width, f->kind, f->compute));
    HIPCHK(&f->err, hipEventRecord(s.k_done, f->compute));
    HIPCHK(&f->err, hipStreamWaitEvent(f->copy_out, s.k_done, 0));
    HIPCHK(&f->err, hipMemcpyAsync(s.h_out, s.d_out, n, hipMemcpyDeviceToHost, f->copy_out));
    HIPCHK(&f->err, hipEventRecord(s.out_done, f->copy_out));
    f->wr = (f->wr + 1) % (int)f->slot.size();
    ++f->used;
    return VH_OK;
}

int vh_filter_collect(vh_filter* f, uint8_t* frame) {
    if (!f || !frame) return fail(f ? &f->err : nullptr, VH_ERR_INVALID, "null argument");
    if (f->used == 0) return fail(&f->err, VH_ERR_RING_EMPTY, "ring empty (PILA VACIA)");
    HIPCHK(&f->err, hipSetDevice(f->device));
    vh_filter::Slot& s = f->slot[f->rd];
    HIPCHK(&f->err, hipEventSynchronize(s.out_done));
    memcpy(frame, s.h_out, (size_t)f->height * f->width);
    f->rd = (f->rd + 1) % (int)f->slot.size();
    --f->used;
    return VH_OK;
}

int vh_mlp_create(int device, int n_ins, int n_layers, const int* n_p_l, int activation, vh_mlp** out) {
    if (!out || !n_p_l || n_ins <= 0 || n_layers <= 0) return fail(nullptr, VH_ERR_INVALID, "vh_mlp_create: bad argument");
    if (activation < VH_ACT_IDENTITY || activation > VH_ACT_GELU) return fail(nullptr, VH_ERR_INVALID, "unknown activation %d", activation);
    *out = nullptr;
    int rc = set_device(nullptr, device);
    if (rc) return rc;
    vh_mlp* m = new vh_mlp();
    m->device = device; m->n_ins = n_ins; m->n_layers = n_layers; m->activation = activation;
    m->widest = n_ins;
    int fan = n_ins;
    for (int l = 0; l < n_layers; ++l) {
        if (n_p_l[l] <= 0) { delete m; return fail(nullptr, VH_ERR_INVALID, "n_p_l[%d] must be positive", l); }
        m->npl.push_back(n_p_l[l]);
        m->n_params += (size_t)n_p_l[l] * fan;   // netFPGA.cpp:68-76
        m->n_neurons += (size_t)n_p_l[l];
        fan = n_p_l[l];
        if (fan > m->widest) m->widest = fan;
    }
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&m->params, m->n_params * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&m->bias, m->n_neurons * 4);
    if (e != hipSuccess) { vh_mlp_destroy(m); return fail(nullptr, VH_ERR_HIP, "vh_mlp_create: %s", hipGetErrorString(e)); }
    *out = m;
    return VH_OK;
}

int vh_mlp_load_params(vh_mlp* m, const float* params, size_t n_params, const float* bias, size_t n_neurons) {
    if (!m || !params || !bias) return fail(m ? &m->err : nullptr, VH_ERR_INVALID, "null argument");
    if (n_params != m->n_params || n_neurons != m->n_neurons)
        return fail(&m->err, VH_ERR_INVALID, "expected %zu params / %zu neurons, got %zu / %zu", m->n_params, m->n_neurons, n_params, n_neurons);
    HIPCHK(&m->err, hipSetDevice(m->device));
    // same order as the reference: params, then bias (netFPGA.cpp:506-509)
    HIPCHK(&m->err, hipMemcpyAsync(m->params, params, n_params * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(&m->err, hipMemcpyAsync(m->bias, bias, n_neurons * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(&m->err, hipStreamSynchronize(m->stream));
    m->loaded = true;
    return VH_OK;
}

int vh_mlp_forward(vh_mlp* m, const float* in, int n_vec, float* outp) {
    if (!m || !in || !outp || n_vec <= 0) return fail(m ? &m->err : nullptr, VH_ERR_INVALID, "bad argument");
    if (!m->loaded) return fail(&m->err, VH_ERR_STATE, "forward before params were loaded");
    const auto t0 = std::chrono::high_resolution_clock::now();
    HIPCHK(&m->err, hipSetDevice(m->device));
    if (n_vec > m->max_vec) {
        if (m->buf0) hipFree(m->buf0);
        if (m->buf1) hipFree(m->buf1);
        m->buf0 = m->buf1 = nullptr; m->max_vec = 0;
        HIPCHK(&m->err, hipMalloc((void**)&m->buf0, (size_t)n_vec * m->widest * 4));
        HIPCHK(&m->err, hipMalloc((void**)&m->buf1, (size_t)n_vec * m->widest * 4));
        m->max_vec = n_vec;
    }
    HIPCHK(&m->err, hipMemcpyAsync(m->buf0, in, (size_t)n_vec * m->n_ins * 4, hipMemcpyHostToDevice, m->stream));
    float *cur = m->buf0, *nxt = m->buf1;
    size_t woff = 0, boff = 0;
    int fan = m->n_ins;
    for (int l = 0; l < m->n_layers; ++l) {
        HIPCHK(&m->err, launch_dense_layer(m->params + woff, m->bias + boff, cur, nxt, fan, m->npl[l], n_vec, m->activation, m->stream));
        woff += (size_t)m->npl[l] * fan; boff += (size_t)m->npl[l]; fan = m->npl[l];
        std::swap(cur, nxt);
    }
    HIPCHK(&m->err, hipMemcpyAsync(outp, cur, (size_t)n_vec * fan * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(&m->err, hipStreamSynchronize(m->stream));
    m->last_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - t0).count();
    return VH_OK;
}

// ---- MLP-mode training (netFPGA.cpp:518-580 is commented-out code: the definitions are in include/vithip.h)
int vh_mlp_init_gradient(vh_mlp* m, const float* set_ins, const float* set_outs, int n_sets) {
    if (!m || !set_ins || !set_outs || n_sets <= 0) return fail(m ? &m->err : nullptr, VH_ERR_INVALID, "vh_mlp_init_gradient: bad argument");
    if (!m->loaded) return fail(&m->err, VH_ERR_STATE, "init_gradient before params were loaded");
    if (n_sets > 65535) return fail(&m->err, VH_ERR_INVALID, "at most 65535 sets");
    for (int n : m->npl) if (n > 65535) return fail(&m->err, VH_ERR_INVALID, "training supports layers of at most 65535 neurons");
    HIPCHK(&m->err, hipSetDevice(m->device));
    for (float** p : {&m->set_ins, &m->set_outs, &m->tz, &m->ta, &m->td, &m->terr}) { if (*p) hipFree(*p); *p = nullptr; }
    m->n_sets = 0;
    const size_t n_out = (size_t)m->npl.back();
    HIPCHK(&m->err, hipMalloc((void**)&m->set_ins, (size_t)n_sets * m->n_ins * 4));
    HIPCHK(&m->err, hipMalloc((void**)&m->set_outs, (size_t)n_sets * n_out * 4));
    HIPCHK(&m->err, hipMalloc((void**)&m->tz, m->n_neurons * n_sets * 4));
    HIPCHK(&m->err, hipMalloc((void**)&m->ta, m->n_neurons * n_sets * 4));
    HIPCHK(&m->err, hipMalloc((void**)&m->td, m->n_neurons * n_sets * 4));
    HIPCHK(&m->err, hipMalloc((void**)&m->terr, 4));
    HIPCHK(&m->err, hipMemcpyAsync(m->set_ins, set_ins, (size_t)n_sets * m->n_ins * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(&m->err, hipMemcpyAsync(m->set_outs, set_outs, (size_t)n_sets * n_out * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(&m->err, hipStreamSynchronize(m->stream));
    m->n_sets = n_sets;
    return VH_OK;
}

int vh_mlp_launch_gradient(vh_mlp* m, int iterations, float error_threshold, float multiplier, float* errors) {
    if (!m || iterations < 0 || (iterations > 0 && !errors)) return fail(m ? &m->err : nullptr, VH_ERR_INVALID, "vh_mlp_launch_gradient: bad argument");
    if (m->n_sets <= 0) return fail(&m->err, VH_ERR_STATE, "launch_gradient before init_gradient");
    const auto t0 = std::chrono::high_resolution_clock::now();
    HIPCHK(&m->err, hipSetDevice(m->device));
    const int S = m->n_sets, L = m->n_layers;
    const float scale = multiplier / (float)S;
    // layer l's slices of the per-set buffers start at noff[l] * S floats
    std::vector<size_t> woff(L), noff(L);
    { size_t w = 0, n = 0; int fan = m->n_ins; for (int l = 0; l < L; ++l) { woff[l] = w; noff[l] = n; w += (size_t)m->npl[l] * fan; n += (size_t)m->npl[l]; fan = m->npl[l]; } }
    auto fan_in = [&](int l) { return l == 0 ? m->n_ins : m->npl[l - 1]; };
    auto act_in = [&](int l) -> const float* { return l == 0 ? m->set_ins : m->ta + noff[l - 1] * S; };
    for (int it = 0; it < iterations; ++it) errors[it] = 0.f;
    for (int it = 0; it < iterations; ++it) {
        for (int l = 0; l < L; ++l)
            HIPCHK(&m->err, launch_dense_layer(m->params + woff[l], m->bias + noff[l], act_in(l), m->ta + noff[l] * S, fan_in(l), m->npl[l], S,
                                               m->activation, m->stream, m->tz + noff[l] * S));
        const int n_out = m->npl[L - 1];
        HIPCHK(&m->err, launch_mlp_out_delta(m->ta + noff[L - 1] * S, m->tz + noff[L - 1] * S, m->set_outs, m->td + noff[L - 1] * S,
                                             (int64_t)S * n_out, m->activation, m->terr, m->stream));
        // the error decides whether this iteration updates: one 4-byte read back per iteration (the reference's loop is
        // host-driven as well, netFPGA.cpp:552-565)
        HIPCHK(&m->err, hipMemcpyAsync(&errors[it], m->terr, 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(&m->err, hipStreamSynchronize(m->stream));
        if (errors[it] <= error_threshold) break;
        for (int l = L - 1; l >= 1; --l)   // deltas back to front, all with the parameters of THIS iteration
            HIPCHK(&m->err, launch_mlp_back_delta(m->params + woff[l], m->td + noff[l] * S, m->tz + noff[l - 1] * S, m->td + noff[l - 1] * S,
                                                  m->npl[l - 1], m->npl[l], S, m->activation, m->stream));
        for (int l = 0; l < L; ++l)
            HIPCHK(&m->err, launch_mlp_update(m->params + woff[l], m->bias + noff[l], m->td + noff[l] * S, act_in(l), fan_in(l), m->npl[l], S,
                                              scale, m->stream));
    }
    HIPCHK(&m->err, hipStreamSynchronize(m->stream));
    m->last_gradient_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - t0).count();
    return VH_OK;
}

int vh_mlp_read_params(vh_mlp* m, float* params, size_t n_params, float* bias, size_t n_neurons) {
    if (!m || !params || !bias) return fail(m ? &m->err : nullptr, VH_ERR_INVALID, "null argument");
    if (n_params != m->n_params || n_neurons != m->n_neurons)
        return fail(&m->err, VH_ERR_INVALID, "expected %zu params / %zu neurons, got %zu / %zu", m->n_params, m->n_neurons, n_params, n_neurons);
    if (!m->loaded) return fail(&m->err, VH_ERR_STATE, "no params loaded");
    HIPCHK(&m->err, hipSetDevice(m->device));
    HIPCHK(&m->err, hipMemcpyAsync(params, m->params, n_params * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(&m->err, hipMemcpyAsync(bias, m->bias, n_neurons * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(&m->err, hipStreamSynchronize(m->stream));
    return VH_OK;
}

int vh_mlp_last_gradient_us(const vh_mlp* m, int64_t* us) {
    if (!m || !us) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *us = m->last_gradient_us;
    return VH_OK;
}

int vh_mlp_last_forward_us(const vh_mlp* m, int64_t* us) {
    if (!m || !us) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *us = m->last_us;
    return VH_OK;
}
const char* vh_mlp_last_error(const vh_mlp* m) { return m ? m->err.c_str() : g_err.c_str(); }

int vh_mlp_destroy(vh_mlp* m) {
    if (!m) return VH_OK;
    hipSetDevice(m->device);
    if (m->stream) hipStreamSynchronize(m->stream);
    if (m->params) hipFree(m->params);
    if (m->bias) hipFree(m->bias);
    if (m->buf0) hipFree(m->buf0);
    if (m->buf1) hipFree(m->buf1);
    for (float* p : {m->set_ins, m->set_outs, m->tz, m->ta, m->td, m->terr}) if (p) hipFree(p);
    if (m->stream) hipStreamDestroy(m->stream);
    delete m;
    return VH_OK;
}

}  // extern "C"

// ---- device group: N GPUs of one node from ONE process ---------------------------------------------
// The reference drives exactly one device (clGetDeviceIDs(ACCELERATOR), netFPGA.cpp:376) with one input per call
// (:266-277); nothing to mirror, so the contract is the survey's: single process, one host thread + one context (own
// stream) per device, ncclCommInitAll, ONE ncclBroadcast of the canonical weight blob (what _load_params uploads per
// device, netFPGA.cpp:484-515) from member 0, contiguous image ranges per member, per-member D2H straight into the
// caller's logits; no collective on the data path.  RCCL is bound at run time (dlopen) and only when a group has more
// than one distinct device, so libvithip.so itself carries no RCCL dependency.
struct vh_group {
    struct Member {
        int device = 0;
        vh_ctx* ctx = nullptr;
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::function<int()> job;   // pending command (empty = none)
        bool quit = false, busy = false;
        int rc = VH_OK;
        float *in_dev = nullptr, *out_dev = nullptr;   // device-resident benchmark buffers
        int resident_batch = 0;
    };
    vh_config cfg;
    std::vector<std::unique_ptr<Member>> m;
    bool same_device = false;   // rehearsal: duplicate ordinals, broadcast by D2D copy instead of RCCL
    void* rccl = nullptr;       // dlopen handle
    std::vector<void*> comms;   // ncclComm_t per member
    std::string err;
};

namespace {

struct RcclApi {
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;

int bind_rccl(vh_group* g) {
    if (g->rccl) return VH_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) { g->rccl = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (g->rccl) break; }
    if (!g->rccl) return fail(&g->err, VH_ERR_UNSUPPORTED, "vh_group: cannot load librccl.so (%s)", dlerror());
    auto sym = [&](const char* n) { return dlsym(g->rccl, n); };
    g_rccl.CommInitAll = (int (*)(void**, int, const int*))sym("ncclCommInitAll");
    g_rccl.CommDestroy = (int (*)(void*))sym("ncclCommDestroy");
    g_rccl.Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))sym("ncclBroadcast");
    g_rccl.GroupStart = (int (*)())sym("ncclGroupStart");
    g_rccl.GroupEnd = (int (*)())sym("ncclGroupEnd");
    g_rccl.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
    if (!g_rccl.CommInitAll || !g_rccl.CommDestroy || !g_rccl.Broadcast || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.GetErrorString)
        return fail(&g->err, VH_ERR_UNSUPPORTED, "vh_group: librccl.so lacks a required symbol");
    return VH_OK;
}

void member_loop(vh_group::Member* m) {
    hipSetDevice(m->device);
    std::unique_lock<std::mutex> lk(m->mu);
    for (;;) {
        m->cv.wait(lk, [&] { return m->quit || (bool)m->job; });
        if (m->quit) return;
        std::function<int()> job = std::move(m->job);
        m->job = nullptr;
        lk.unlock();
        const int rc = job();
        lk.lock();
        m->rc = rc;
        m->busy = false;
        m->cv.notify_all();
    }
}

// run one command per member concurrently, wait for all; returns the first failure
int run_all(vh_group* g, const std::function<int(int)>& cmd) {
    for (size_t i = 0; i < g->m.size(); ++i) {
        vh_group::Member* m = g->m[i].get();
        std::lock_guard<std::mutex> lk(m->mu);
        m->busy = true;
        m->job = [cmd, i]() { return cmd((int)i); };
        m->cv.notify_all();
    }
    int rc = VH_OK;
    for (size_t i = 0; i < g->m.size(); ++i) {
        vh_group::Member* m = g->m[i].get();
        std::unique_lock<std::mutex> lk(m->mu);
        m->cv.wait(lk, [&] { return !m->busy; });
        if (m->rc != VH_OK && rc == VH_OK) {
            rc = m->rc;
            g->err = std::string("member ") + std::to_string(i) + " (device " + std::to_string(m->device) + "): " + m->ctx->err;
        }
    }
    if (rc != VH_OK) g_err = g->err;
    return rc;
}

}  // namespace

extern "C" {

void vh_group_shard_bounds(int batch, int n, int r, int* lo, int* hi) {
    // contiguous image range of member r; the first (batch % n) members take one extra image
    const int base = batch / n, extra = batch % n;
    const int l = r * base + (r < extra ? r : extra);
    if (lo) *lo = l;
    if (hi) *hi = l + base + (r < extra ? 1 : 0);
}

const char* vh_group_last_error(const vh_group* g) { return g ? g->err.c_str() : g_err.c_str(); }

int vh_group_destroy(vh_group* g) {
    if (!g) return VH_OK;
    for (auto& mp : g->m) {
        vh_group::Member* m = mp.get();
        if (m->th.joinable()) {
            { std::lock_guard<std::mutex> lk(m->mu); m->quit = true; m->cv.notify_all(); }
            m->th.join();
        }
    }
    for (size_t i = 0; i < g->comms.size(); ++i)
        if (g->comms[i] && g_rccl.CommDestroy) { hipSetDevice(g->m[i]->device); g_rccl.CommDestroy(g->comms[i]); }
    for (auto& mp : g->m) {
        hipSetDevice(mp->device);
        if (mp->in_dev) hipFree(mp->in_dev);
        if (mp->out_dev) hipFree(mp->out_dev);
        if (mp->ctx) vh_destroy(mp->ctx);
    }
    delete g;
    return VH_OK;
}

int vh_group_create(const vh_config* cfg, const int* devices, int n, vh_group** out) {
    if (!cfg || !devices || !out || n < 1 || n > 64) return fail(nullptr, VH_ERR_INVALID, "vh_group_create: bad argument");
    *out = nullptr;
    vh_group* g = new vh_group();
    g->cfg = *cfg;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) g->same_device |= devices[i] == devices[j];
    for (int i = 0; i < n; ++i) {
        std::unique_ptr<vh_group::Member> m(new vh_group::Member());
        m->device = devices[i];
        const int rc = vh_create(cfg, devices[i], &m->ctx);
        g->m.push_back(std::move(m));
        if (rc != VH_OK) { vh_group_destroy(g); return rc; }
    }
    // RCCL serves groups of DISTINCT devices only (a communicator cannot hold one device twice): a group that lists an
    // ordinal more than once -- the one-GPU rehearsal of the N > 1 code path -- always broadcasts by device-to-device copy.
    // VH_GROUP_FORCE_RCCL=1 makes a group of ONE go through ncclCommInitAll / ncclBroadcast as well (a smoke test of the
    // run-time binding); it has no effect on a rehearsal group.
    const char* force = getenv("VH_GROUP_FORCE_RCCL");
    if ((n > 1 && !g->same_device) || (force && force[0] == '1' && !g->same_device)) {
        int rc = bind_rccl(g);
        if (rc == VH_OK) {
            g->comms.assign(n, nullptr);
            const int r = g_rccl.CommInitAll(g->comms.data(), n, devices);
            if (r != 0) rc = fail(&g->err, VH_ERR_HIP, "ncclCommInitAll: %s", g_rccl.GetErrorString(r));
        }
        if (rc != VH_OK) { const std::string e = g->err; vh_group_destroy(g); g_err = e; return rc; }
    }
    for (auto& mp : g->m) mp->th = std::thread(member_loop, mp.get());
    *out = g;
    return VH_OK;
}

int vh_group_size(const vh_group* g, int* n) {
    if (!g || !n) return fail(nullptr, VH_ERR_INVALID, "null argument");
    *n = (int)g->m.size();
    return VH_OK;
}

int vh_group_member(vh_group* g, int i, vh_ctx** ctx, int* device) {
    if (!g || i < 0 || i >= (int)g->m.size()) return fail(g ? &g->err : nullptr, VH_ERR_INVALID, "vh_group_member: bad index");
    if (ctx) *ctx = g->m[i]->ctx;
    if (device) *device = g->m[i]->device;
    return VH_OK;
}

// member 0's resident canonical blob -> every other member's blob buffer (one ncclBroadcast over xGMI), then every other
// member converts it to its compute layout (vh_load_weights_device, the same code path a blob from an RCCL broadcast of
// the multi-process form takes)
int vh_group_broadcast_weights(vh_group* g) {
    if (!g) return fail(nullptr, VH_ERR_INVALID, "null group");
    vh_ctx* root = g->m[0]->ctx;
    if (!root->weights_ready) return fail(&g->err, VH_ERR_STATE, "vh_group_broadcast_weights: member 0 has no weights");
    const size_t nbytes = sizeof(BlobHeader) + 4 * root->L.total;
    const int n = (int)g->m.size();
    if (!g->comms.empty()) {
        HIPCHK(&g->err, hipSetDevice(g->m[0]->device));
        HIPCHK(&g->err, hipStreamSynchronize(root->stream));
        // Whatever fails between GroupStart and GroupEnd, the group is still ENDED before this function returns: leaving it
        // open would leave the other members' streams with a half-enqueued collective.
        int r = g_rccl.GroupStart();
        hipError_t he = hipSuccess;
        for (int i = 0; i < n && r == 0 && he == hipSuccess; ++i) {
            he = hipSetDevice(g->m[i]->device);
            if (he != hipSuccess) break;
            vh_ctx* c = g->m[i]->ctx;
            r = g_rccl.Broadcast(root->blob, c->blob, nbytes, /*ncclUint8*/ 1, 0, g->comms[i], c->stream);
        }
        const int r2 = g_rccl.GroupEnd();
        if (he != hipSuccess) return fail(&g->err, VH_ERR_HIP, "vh_group_broadcast_weights: hipSetDevice: %s", hipGetErrorString(he));
        if (r == 0) r = r2;
        if (r != 0) return fail(&g->err, VH_ERR_HIP, "ncclBroadcast: %s", g_rccl.GetErrorString(r));
        for (int i = 0; i < n; ++i) {
            HIPCHK(&g->err, hipSetDevice(g->m[i]->device));
            HIPCHK(&g->err, hipStreamSynchronize(g->m[i]->ctx->stream));
        }
    } else if (n > 1) {   // rehearsal group on one device: the broadcast is a device-to-device copy
        HIPCHK(&g->err, hipSetDevice(g->m[0]->device));
        HIPCHK(&g->err, hipStreamSynchronize(root->stream));
        for (int i = 1; i < n; ++i) HIPCHK(&g->err, hipMemcpy(g->m[i]->ctx->blob, root->blob, nbytes, hipMemcpyDeviceToDevice));
    }
    return run_all(g, [g, nbytes](int i) { return i == 0 ? VH_OK : vh_load_weights_device(g->m[i]->ctx, g->m[i]->ctx->blob, nbytes); });
}

int vh_group_load_weights(vh_group* g, const void* host_blob, size_t nbytes) {
    if (!g || !host_blob) return fail(g ? &g->err : nullptr, VH_ERR_INVALID, "null argument");
    int rc = vh_load_weights(g->m[0]->ctx, host_blob, nbytes);
    if (rc != VH_OK) { g->err = g->m[0]->ctx->err; return rc; }
    return vh_group_broadcast_weights(g);
}

int vh_group_init_weights_seeded(vh_group* g, uint64_t seed) {
    if (!g) return fail(nullptr, VH_ERR_INVALID, "null group");
    int rc = vh_init_weights_seeded(g->m[0]->ctx, seed);
    if (rc != VH_OK) { g->err = g->m[0]->ctx->err; return rc; }
    return vh_group_broadcast_weights(g);
}

// The hot path over the group: `batch` images in host memory, member r takes the contiguous range vh_group_shard_bounds
// gives it and writes its logits straight into the caller's buffer.  Every member runs its vh_forward (H2D, kernels,
// blocking D2H: the reference's launch_forward window, netFPGA.cpp:262-284) on its own host thread and stream.
int vh_group_forward(vh_group* g, const float* in_host, int batch, float* logits_host) {
    if (!g || !in_host || !logits_host) return fail(g ? &g->err : nullptr, VH_ERR_INVALID, "null argument");
    const int n = (int)g->m.size();
    if (batch < 1) return fail(&g->err, VH_ERR_INVALID, "batch must be positive");
    if ((batch + n - 1) / n > g->cfg.max_batch)
        return fail(&g->err, VH_ERR_INVALID, "batch %d over %d devices exceeds max_batch=%d per device", batch, n, g->cfg.max_batch);
    const size_t img = (size_t)g->cfg.image_size * g->cfg.image_size * g->cfg.channels, cls = (size_t)g->cfg.classes;
    return run_all(g, [=](int i) {
        int lo, hi;
        vh_group_shard_bounds(batch, n, i, &lo, &hi);
        if (hi == lo) return VH_OK;   // fewer images than members
        return vh_forward(g->m[i]->ctx, in_host + (size_t)lo * img, hi - lo, logits_host + (size_t)lo * cls);
    });
}

// ---- device-resident measurement path (bench.py --group): inputs generated in each member's HBM -----------------------
int vh_group_fill_inputs_seeded(vh_group* g, uint64_t seed, int batch_per_device) {
    if (!g || batch_per_device < 1 || batch_per_device > g->cfg.max_batch) return fail(g ? &g->err : nullptr, VH_ERR_INVALID, "bad argument");
    const size_t in_bytes = (size_t)batch_per_device * g->cfg.image_size * g->cfg.image_size * g->cfg.channels * 4;
    const size_t out_bytes = (size_t)batch_per_device * g->cfg.classes * 4;
    return run_all(g, [=](int i) {
        vh_group::Member* m = g->m[i].get();
        if (m->resident_batch < batch_per_device) {
            if (m->in_dev) hipFree(m->in_dev);
            if (m->out_dev) hipFree(m->out_dev);
            m->in_dev = m->out_dev = nullptr; m->resident_batch = 0;
            if (hipMalloc((void**)&m->in_dev, in_bytes) != hipSuccess || hipMalloc((void**)&m->out_dev, out_bytes) != hipSuccess)
                return fail(&m->ctx->err, VH_ERR_HIP, "vh_group_fill_inputs_seeded: out of device memory");
            m->resident_batch = batch_per_device;
        }
        return vh_fill_input_seeded(m->ctx, seed + (uint64_t)i, batch_per_device, m->in_dev);   // member i = rank i's shard
    });
}

int vh_group_forward_resident(vh_group* g, int batch_per_device, int steps) {
    if (!g || steps < 1) return fail(g ? &g->err : nullptr, VH_ERR_INVALID, "bad argument");
    for (auto& mp : g->m)
        if (mp->resident_batch < batch_per_device) return fail(&g->err, VH_ERR_STATE, "call vh_group_fill_inputs_seeded first");
    return run_all(g, [=](int i) {
        vh_group::Member* m = g->m[i].get();
        int rc = vh_forward_device_async(m->ctx, m->in_dev, batch_per_device, m->out_dev, steps);
        return rc != VH_OK ? rc : vh_synchronize(m->ctx);
    });
}

int vh_group_read_logits(vh_group* g, int batch_per_device, float* logits_host) {
    if (!g || !logits_host) return fail(g ? &g->err : nullptr, VH_ERR_INVALID, "null argument");
    const size_t per = (size_t)batch_per_device * g->cfg.classes;
    return run_all(g, [=](int i) {
        vh_group::Member* m = g->m[i].get();
        if (m->resident_batch < batch_per_device) return fail(&m->ctx->err, VH_ERR_STATE, "no resident batch");
        hipError_t e = hipMemcpy(logits_host + (size_t)i * per, m->out_dev, per * 4, hipMemcpyDeviceToHost);
        return e == hipSuccess ? VH_OK : fail(&m->ctx->err, VH_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(e));
    });
}

}  // extern "C"
