// vh_kernels.h — internal launch API between the C-ABI layer (vithip_api.hip) and the kernels.
#pragma once

#include <atomic>
#include <cstdlib>
#include <vector>

#include "vh_common.h"

namespace vh {

// One GEMM launch: out = epilogue(A[M,K] x W[N,K]^T).  `dtype` selects the operand form inside launch_gemm: VH_DTYPE_BF16 / FP16
// (kernels_gemm.hip, kernels_gemm5.hip) or VH_DTYPE_FP8 = OCP e4m3 bytes with one fp32 scale per output channel (kernels_gemm5.hip:
// K % 128 == 0, variants 0 / 5 / 6 / 7, 16-bit results are bf16, the activation epilogues write e4m3, no PATCH / PATCH_SPLIT).
// gemm_check says what a launch accepts; launch_gemm asks it first.
struct GemmArgs {
    const void* a;      // [M, K], K contiguous
    const void* w;      // [N, K], K contiguous
    const float* bias;  // [N]
    void* out;          // 16-bit, e4m3 or fp32 [M(or remapped rows), N]
    int64_t M;
    int N, K;
    int epilogue;       // VH_EPI_*
    const float* aux;   // what the EPILOGUE defines, whatever the operands: PATCH / PATCH_SPLIT pos-emb [tokens, N]; LNFOLD* c_n [N]
    int aux_i;          // PATCH / PATCH_SPLIT: patches per image
    int dtype;          // VH_DTYPE_* of the operands
    int variant;        // 0 auto, 1 = 128x128, 2 = 256x256 two-stage, 5 = ping-pong, 6 = persistent ping-pong, 7 = ping-pong, three A stages
    const float* stats = nullptr;  // LNFOLD*: [M][2] (mean, rstd)
    void* out16 = nullptr;         // RESID_LN: 16-bit (e4m3 operands: e4m3) copy of the updated rows; RESID_SPLIT / PATCH_SPLIT: the lo plane
    float* partials = nullptr;     // RESID_LN / RESID_SPLIT / PATCH_SPLIT: [N/64][M][2]
    const float* wscale = nullptr; // e4m3 operands: the per-output-channel weight scales [N], with every epilogue; unused with 16-bit operands
    // ping-pong forms 5 / 7 only: launch tiles [tile_begin, tile_begin + tile_count) of the n-fastest 256x256 tile order
    // (tile t = (t / tiles_n, t % tiles_n)); tile_count == 0 = all tiles.
    int tile_begin = 0, tile_count = 0;
    // PATCH_SPLIT: row stride of `partials` = number of TOKEN rows the statistics buffer is laid out for (0 = images x tokens)
    int64_t prow = 0;
    // The TILED layouts (gemm_epilogue.h, OTILED; persistent form only, so variant 6 is spelled out and the shape is one
    // gemm_tiled_applies accepts).  out_tiled: an activation epilogue writes the MLP hidden activation tiled, LNFOLD / 16-bit BIAS
    // write q|k|v head-major; ab_tiled: A and W of this launch are both in the tiled layout (16-row blocks).
    int out_tiled = 0, ab_tiled = 0;
    // PATCH / PATCH_SPLIT: rows in front of an image's patch rows (the class token + the register tokens): GEMM row m = img * aux_i + p
    // lands on output row m + img * lead + lead and adds pos row 1 + p.  Every public vh_op_gemm* tap keeps 1.
    int lead = 1;
};
// does a GEMM of this shape and operand dtype take the persistent form, the only one that reads / writes the tiled layouts?
bool gemm_tiled_applies(int64_t M, int N, int K, int dtype);
// W fp32 [rows, cols] -> 16-bit in the tiled layout (16-row blocks, natural column order); e4m3: the byte matrix -> tiled copy
hipError_t launch_cast_tiled_w(const float* w, int rows, int cols, void* w16, int dtype, hipStream_t stream);
hipError_t launch_tile_bytes(const void* w8, int rows, int cols, void* out, hipStream_t stream);

// row stride of the partial-sum buffer a launch writes: PATCH_SPLIT lands on token rows (images x (patches + lead) unless the
// caller's buffer is laid out for more, e.g. rows padded to whole tiles); the other forms use their own M inside the kernel
inline int64_t gemm_prow(const GemmArgs& g) {
    if (g.epilogue != VH_EPI_PATCH_SPLIT) return g.M;
    return g.prow > 0 ? g.prow : (g.M / g.aux_i) * (int64_t)(g.aux_i + g.lead);
}

// every launcher only enqueues on `stream`; returns hipSuccess or the launch error (hipErrorInvalidValue: gemm_check refuses)
hipError_t launch_gemm(const GemmArgs& g, hipStream_t stream);
const char* gemm_check(const GemmArgs& g);  // NULL if the launch is accepted, else the reason; host arithmetic only, no HIP call
int gemm_pick_variant(int64_t M, int N, int epilogue);
int gemm_pp_variant(int epilogue);  // 5, 6 or 7 (default 6 = persistent; env VH_GEMM_PP forces one)

hipError_t launch_layernorm(const float* x, int64_t rows, int dim, int64_t row_stride,
                            const float* gamma, const float* beta, float eps, void* out16,
                            int dtype, hipStream_t stream);
// dtype = VH_DTYPE_* (16-bit / e4m3 result) or VH_DTYPE_F32_INTERNAL (vh_common.h; fp32 result: the final LayerNorm in front of the head)
// classifier head, fp32 operands (exact-fp32 MFMA): logits[b, c] = y[b, :] . w[c, :] + bias[c]; classes % 4 == 0, dim % 16 == 0
hipError_t launch_head_f32(const float* y, const float* w, const float* bias, float* out, int batch, int classes, int dim,
                           hipStream_t stream);
// The same kernel as `groups` independent products in one launch (the MAP head's per-head V product): group g reads y + g * y_step
// (row stride ldy), w + g * classes * dim, bias + g * classes and writes out + g * classes (row stride ldo); `add` (optional,
// [batch][ldo] like out) is added to the result (the MAP head's residual).  launch_head_f32 is groups = 1, ldy = dim, ldo = classes.
hipError_t launch_head_f32_groups(const float* y, int64_t ldy, int64_t y_step, const float* w, const float* bias, float* out, int64_t ldo,
                                  const float* add, int batch, int classes, int dim, int groups, hipStream_t stream);
// x[i] <- act(x[i]) in fp32, act = 0 erf GELU, 1 QuickGELU, 2 tanh GELU, each as its defining expression (the MAP head's hidden rows)
hipError_t launch_act_f32(float* x, int64_t n, int act, hipStream_t stream);
// q columns of qkv16 arrive scaled by kAttnQScale = 64^-1/2 * log2(e) (folded into Wq and bq when the weights are
// prepared): the score MFMAs then produce log2-domain scores and the softmax is exp2 without a multiply per score
constexpr float kAttnQScale = 0.125f * 1.4426950408889634f;
// ticket: 4 bytes of device scratch owned by the caller's stream (work-queue counter of the staged ring form; zeroed by
// the launch unless the caller says it already is: a forward zeroes one word per layer with ONE memset), or nullptr for
// equal static shares per workgroup
// out_tiled (16-bit results, ring forms: ask attention_tiled_applies): the output in the 16-row-blocked layout the out-projection's
// tiled operand DMA reads ([rows / 16][dim / 8][16][8], rows = batch * tokens rounded up to 16 by the caller's buffer)
hipError_t launch_attention(const void* qkv16, int batch, int tokens, int heads, void* out16,
                            int dtype, unsigned int* ticket, hipStream_t stream, bool ticket_zeroed = false, bool out_tiled = false,
                            int64_t in_hm_rows = 0);   // in_hm_rows != 0: q|k|v is head-major, [3][heads][in_hm_rows][64] (needs out_tiled)
bool attention_tiled_applies(int batch, int tokens, int heads);
// class-token query only: out16 [batch][heads * 64] (VH_FLAG_CLS_TAIL); 16-bit dtypes, tokens <= 1024
hipError_t launch_attention_cls(const void* qkv16, int batch, int tokens, int heads, void* out16, int dtype, hipStream_t stream);
size_t attention_lds_bytes(int tokens);
// K/V-streaming attention at head dims 32, 48, ..., 128 (kernels_attn_hd.hip): the same operation in a fixed LDS ring (24 KiB at head
// dim 64), row-major q|k|v [batch*tokens][3*heads*head_dim] with q pre-scaled by head_dim^-1/2 * log2(e) (attention_q_scale) ->
// row-major [batch*tokens][heads*head_dim]; tokens 1..kAttnStreamMaxTokens, heads * head_dim <= kAttnHdMaxWidth (heads <= 32 at
// head dim 64); dtype VH_DTYPE_FP8 = bf16 in, e4m3 out.  No work-queue counter and no allocation (graph capture, split batches).
// The forward uses it for every head dim other than 64; at head dim 64 launch_attention sends a row-major call here when the
// resident forms cannot hold the head (attention_lds_bytes(tokens) > 160 KiB).
constexpr int kAttnStreamMaxTokens = 4097;   // 64 x 64 patches + the class token
constexpr int kAttnHdMaxWidth = 2048;
bool attention_hd_supported(int head_dim);
hipError_t launch_attention_hd(const void* qkv16, int batch, int tokens, int heads, int head_dim, void* out16, int dtype,
                               hipStream_t stream);
// Attention maps (kernels_attn_maps.hip; contract: vithip.h, "Attention maps").  launch_attention_probs: the softmax rows of the first
// Q queries of every (image, head) -> probs [batch][heads][Q][tokens] fp32, from the q|k|v a projection wrote: row-major
// [batch*tokens][3*heads*head_dim] (in_hm_rows == 0; head dims 32, 48, ..., 128) or head-major [3][heads][in_hm_rows][64] (head dim 64);
// bf16 / fp16 elements, q pre-scaled by attention_q_scale.  tokens 1..kAttnStreamMaxTokens, Q 1..min(kAttnMapsMaxQueries, tokens),
// heads * head_dim <= kAttnHdMaxWidth.  The raw scores are staged in probs itself: no LDS, no other scratch.
// launch_attention_readout: such a store -> probs_out [batch][heads][Q][K] and / or mean_out [batch][Q][K] (the serial fp32 chain over
// ascending heads, times (float)(1.0 / heads)) in `elem` (VH_ELEM_F32 / F16 / BF16); keys VH_ATTN_KEYS_ALL: K = tokens,
// VH_ATTN_KEYS_PATCH: columns lead .. tokens - 1.  The *_check functions: nullptr, or why the launch is refused; host arithmetic only.
constexpr int kAttnMapsMaxQueries = 17;   // the class token + up to 16 register tokens
const char* attention_probs_check(int64_t in_hm_rows, int batch, int tokens, int heads, int head_dim, int Q, int dtype);
hipError_t launch_attention_probs(const void* qkv16, int64_t in_hm_rows, int batch, int tokens, int heads, int head_dim, int Q, int dtype,
                                  float* probs, hipStream_t stream);
// Rotary position embedding (kernels_rope.hip; contract: vithip.h VH_FLAG_ROPE, vh_op_rope): q and k of rows lead .. tokens - 1 of
// every image and head are rotated in place by cos_t / sin_t [tokens - lead][head_dim / 2] fp32 (16-byte aligned, like qkv16).  The
// layouts are launch_attention_probs's: row-major (hm_rows == 0) at head dims 32, 48, ..., 128, head-major at head dim 64.  v, the lead
// rows and rows beyond batch * tokens are never written.  No allocation (graph capture, split batches).  rope_check: nullptr, or why.
const char* rope_check(const void* qkv16, int dtype, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows,
                       const float* cos_t, const float* sin_t);
hipError_t launch_rope(void* qkv16, int dtype, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows, const float* cos_t,
                       const float* sin_t, hipStream_t stream);
// The gate pass of a SwiGLU MLP (kernels_swiglu.hip; contract: vithip.h VH_FLAG_SWIGLU, vh_op_swiglu): gu16 [rows][2 mlp_dim] row-major
// (what fc1 writes with VH_EPI_LNFOLD / VH_EPI_BIAS and out_tiled = 0; gate columns first) -> h16 [rows][mlp_dim] = silu(g) * u, row-major
// (out_tiled = 0) or in fc2's tiled operand layout [rows / 16][mlp_dim / 8][16][8] (out_tiled = 1: rows a multiple of 16).  Both
// 16-byte aligned, mlp_dim a multiple of 64.  No allocation (graph capture, split batches).  swiglu_check: nullptr, or why.
const char* swiglu_check(const void* gu16, int dtype, int64_t rows, int mlp_dim, const void* h16, int out_tiled);
hipError_t launch_swiglu(const void* gu16, int dtype, int64_t rows, int mlp_dim, void* h16, int out_tiled, hipStream_t stream);
const char* attention_readout_check(int batch, int heads, int Q, int tokens, int lead, int elem, int keys);
hipError_t launch_attention_readout(const float* store, int batch, int heads, int Q, int tokens, int lead, int elem, int keys, void* probs_out,
                                    void* mean_out, hipStream_t stream);
// the factor folded into Wq and bq: head_dim^-1/2 * log2(e); exactly kAttnQScale at head dim 64
inline float attention_q_scale(int head_dim) {
    return head_dim == 64 ? kAttnQScale : (float)(1.4426950408889634 / __builtin_sqrt((double)head_dim));
}
// patch matrix [batch*np, kpad] of NHWC fp32 images.  kpad == patch^2 * channels with 4 | patch * channels: im2col_kernel
// (one float4 per thread); otherwise im2col_pad_kernel (kpad >= patch^2 * channels, 8 | kpad, zeros in the pad columns)
hipError_t launch_im2col(const float* in_nhwc, int batch, int image, int patch, int channels, int kpad,
                         void* out16, int dtype, hipStream_t stream);
// The same patch matrix from 8-bit NHWC images: pixel p of channel c enters as fmaf((float)p, scale[c], shift[c]) (one
// rounding) and takes the same RNE conversion, so the matrix has the bits launch_im2col gives for that fp32 array.  Any
// patch / channel count, kpad >= patch^2 * channels, 8 | kpad, pad columns zero; scale / shift: host arrays [channels].
// 8-byte loads where 8 | patch * channels, 8 | image * channels and the base is 8-byte aligned, byte loads otherwise.
constexpr int kMaxChannels = 64;
hipError_t launch_im2col_u8(const uint8_t* in_nhwc, int batch, int image, int patch, int channels, int kpad,
                            const float* scale, const float* shift, void* out16, int dtype, hipStream_t stream);
// The same patch matrix from an image TENSOR (kernels_gather.hip; contract: vithip.h, "Image tensors"): elem VH_ELEM_*, layout
// VH_LAYOUT_*; the bits launch_im2col gives for the NHWC fp32 array of the widened (u8: normalised) elements.  (NHWC, F32) and
// (NHWC, U8) ARE launch_im2col / launch_im2col_u8; NHWC 16-bit floats take the padded gather with a 16-bit source, NCHW a
// gather that transposes (x, c) through LDS.  scale / shift: host arrays [channels], read for VH_ELEM_U8 only.
// hipErrorInvalidValue for an unknown elem / layout / dtype, a null pointer or a shape the other two launches refuse.
hipError_t launch_im2col_tensor(const void* in, int elem, int layout, int batch, int image, int patch, int channels, int kpad,
                                const float* scale, const float* shift, void* out16, int dtype, hipStream_t stream);
// Antialiased resize + crop of 8-bit interleaved frames to S x S (kernels_resize.hip; contract: vithip.h, "8-bit frames").
// resize_axis_table: the table of one axis (host, double, one rounding to fp32; weights [n_out][max_taps], zero padded); 0 = ok.
// resize_plan_build: checks every descriptor and fills `words` with [batch x 16-word frame record][tables] as the kernel reads
// them; returns nullptr, or why the call is refused.  launch_resize_u8: one launch for the batch; plan_dev = those words in HBM.
constexpr int kResizeMaxTaps = 65, kResizeMaxScale = 32, kResizeMaxSide = 8192;
constexpr int kResizeLdsFloats = 16384;   // 64 KiB: two workgroups per CU
constexpr int kResizeFrameWords = 16;
int resize_axis_table(int n_in, double lo, double hi, int n_out, int32_t* first, int32_t* count, float* weights, int max_taps);
const char* resize_plan_build(const vh_frame* desc, int batch, int channels, int S, size_t nbytes, bool base_aligned4,
                              std::vector<uint32_t>* words, int* max_tiles);
hipError_t launch_resize_u8(const uint8_t* frames, const uint32_t* plan_dev, int batch, int channels, int S, int max_tiles,
                            uint8_t* out_u8, hipStream_t stream);
// NV12 frames (kernels_resize_nv12.hip; contract: vithip.h, "NV12 frames"): both planes resampled with the tables above and the
// 3 x 4 colour matrix applied to the unrounded y, u, v, one launch for the batch -> [batch][S][S][3] bytes.
// resize_axis_table_over: resize_axis_table with hi <= n_in + over (left-sited chroma overhangs the last sample by 0.25).
// resize_plan_build_nv12: checks every descriptor and fills `words` with [batch x 24-word frame record][tables]; nullptr, or why
// the call is refused.  yuv_matrix: the matrix of a standard (VH_YUV_*) and range, host only; 0 = ok.
constexpr int kResizeNv12FrameWords = 24;
int resize_axis_table_over(int n_in, double lo, double hi, double over, int n_out, int32_t* first, int32_t* count, float* weights,
                           int max_taps);
const char* resize_plan_build_nv12(const vh_frame_nv12* desc, int batch, int S, size_t nbytes, unsigned base_mod4, int chroma_site,
                                   int sample_bytes, std::vector<uint32_t>* words, int* max_tiles);
int yuv_matrix(int standard, int full_range, float m[12]);
// Planar YUV frames (the same file and kernel body; contract: vithip.h, "Planar YUV frames"): three byte planes, chroma
// sub-sampled by 1 or 2 per axis, any parity of the luma size.  resize_plan_build_yuv: as resize_plan_build_nv12, the same record
// and tables; every refusal has a message of its own.
const char* resize_plan_build_yuv(const vh_frame_yuv* desc, int batch, int S, size_t nbytes, bool base_even, int chroma_site, int sample_bytes,
                                  std::vector<uint32_t>* words, int* max_tiles);
// 16-bit YUV frames (the same file, planners and kernel body; contract: vithip.h, "16-bit YUV frames").  Both planners take the
// sample width: sample_bytes 1 = the byte layouts above, 2 = little-endian 16-bit words (P010 / P012 / P016, yuv4xxpNNle), whose
// strides and spans are checked in bytes and whose offsets, strides and base must be even.  base_mod4: the frames address & 3 (0
// for a host buffer); base_even: the same address is even.
// yuv_matrix16: the matrix of `bits`-bit codes in the high (msb_aligned) or low bits of the word, host only; 0 = ok.
int yuv_matrix16(int standard, int full_range, int bits, int msb_aligned, float m[12]);
// launch_resize_yuv_any: one launch for the batch of any of the four layouts; planar picks the three-plane instantiations (a plan of
// resize_plan_build_yuv) over the Y + UV ones (resize_plan_build_nv12), wide the uint16_t ones (plans built with sample_bytes 2).
hipError_t launch_resize_yuv_any(bool planar, bool wide, const uint8_t* frames, const uint32_t* plan_dev, int batch, int S, int max_tiles,
                                 const float* m12_host, uint8_t* out_u8, hipStream_t stream);
// Packed 4:2:2 frames (the same file, record and kernel body; contract: vithip.h, "Packed 4:2:2 frames"): YUY2 / UYVY / YVYU / VYUY
// (sample_bytes 1), Y210 / Y216 and v210 (sample_bytes 2).  resize_plan_build_yuy2 plans the planar 4:2:2 frame of the de-interleaved
// planes (the same tables and bands) and puts the layout into the record; base_mod8: the frames address & 7 (0 for a host buffer).
// launch_resize_yuy2: one launch for the batch; wide: a plan built with sample_bytes 2.
const char* resize_plan_build_yuy2(const vh_frame_yuy2* desc, int batch, int S, size_t nbytes, unsigned base_mod8, int chroma_site,
                                   int sample_bytes, std::vector<uint32_t>* words, int* max_tiles);
hipError_t launch_resize_yuy2(bool wide, const uint8_t* frames, const uint32_t* plan_dev, int batch, int S, int max_tiles,
                              const float* m12_host, uint8_t* out_u8, hipStream_t stream);
// Packed 4:4:4 frames (the same file and record, a body of its own; contract: vithip.h, "Packed 4:4:4 frames"): BGR / BGRA / RGBA /
// ARGB, YUV24 / VUYA / AYUV (sample_bytes 1), Y416 / AYUV64 and Y410 / V410 (sample_bytes 2).  resize_plan_build_bgra plans the planar
// 4:4:4 frame of the de-interleaved samples (the same tables and bands) and puts the layout word into the record; base_mod8: the frames
// address & 7 (0 for a host buffer).  launch_resize_bgra: one launch for the batch; wide: a plan built with sample_bytes 2.
const char* resize_plan_build_bgra(const vh_frame_bgra* desc, int batch, int S, size_t nbytes, unsigned base_mod8, int sample_bytes,
                                   std::vector<uint32_t>* words, int* max_tiles);
hipError_t launch_resize_bgra(bool wide, const uint8_t* frames, const uint32_t* plan_dev, int batch, int S, int max_tiles,
                              const float* m12_host, uint8_t* out_u8, hipStream_t stream);
// the `lead` = 1 + R leading rows of every image (R register tokens, reg [R][dim], unread when lead == 1): row 0 = cls + pos[0],
// row 1 + r = reg[r].  cls == nullptr (VH_FLAG_NO_CLS): no class-token row, rows 0 .. lead - 1 = reg[r], pos unread; lead == 0 then
// makes no launch at all.  Both launchers.
hipError_t launch_lead_rows(float* x, const float* cls, const float* pos, const float* reg, int lead, int batch, int tokens,
                            int dim, hipStream_t stream);
// the same rows of the SPLIT residual: their (hi, lo) planes and their per-64-column partial sums
hipError_t launch_lead_rows_split(void* hi, void* lo, float* partials, int64_t prow, const float* cls, const float* pos,
                                  const float* reg, int lead, int batch, int tokens, int dim, int dtype, hipStream_t stream);
hipError_t launch_cast(const float* in, void* out16, int64_t n, int dtype, hipStream_t stream);
hipError_t launch_fill(float* out, int64_t n, uint64_t seed, uint32_t tensor_id, int kind,
                       float sigma, float offset, hipStream_t stream);
// fp8 weight quantisation: w fp32 [rows, cols] -> e4m3 [rows, cols] with scale[r] = post * amax_r / 448 (amax 0 -> post),
// q = rne_e4m3(w / (amax_r / 448)); `post` folds a constant factor into the scale (the q rows' softmax scale)
// out = decode(e4m3(w / s0)) * s0 per row, s0 = amax_row / 448: the values of a weight-only e4m3 matrix (VH_FLAG_W8_E4M3)
hipError_t launch_fake_quant_rows(const float* w, int rows, int cols, float* out, hipStream_t stream);
hipError_t launch_quantize_rows(const float* w, int rows, int cols, float post, void* w8, float* scale, hipStream_t stream);
// weight preparation (fp32 canonical tensors -> compute layout)
hipError_t launch_pack_qkv(const float* qw, const float* qb, const float* kw, const float* kb,
                           const float* vw, const float* vb, int dim, float q_scale, void* w16,
                           float* b32, int dtype, hipStream_t stream);
// conv weight [D][C][P][P] -> [D][kpad] in the im2col k order; the same two forms as launch_im2col
hipError_t launch_permute_patch(const float* w_nchw, int dim, int channels, int patch, int kpad, void* w16,
                                int dtype, hipStream_t stream);
// folded LayerNorm helpers
// amax_guard (optional, e4m3 rows only): running maximum of |x| over the first guard_rows rows, as float bits
hipError_t launch_rowstats_cast(const float* x, int64_t rows, int dim, float eps, void* x16, float* stats, int dtype,
                                hipStream_t stream, int64_t guard_rows = 0, unsigned int* amax_guard = nullptr);
// guard (optional): running maximum of |mean| * rstd over the first `guard_rows` rows, as float bits (kernels_rows.hip)
// amax_guard (optional): running maximum of an upper bound of |x| (largest 64-column block's root sum of squares)
hipError_t launch_finalize_stats(const float* partials, int nblk, int64_t rows, int dim, float eps, float* stats,
                                 hipStream_t stream, int64_t guard_rows = 0, unsigned int* guard = nullptr,
                                 unsigned int* amax_guard = nullptr);
hipError_t launch_ln_guard(const float* stats, int64_t rows, unsigned int* guard, hipStream_t stream);
// split residual (x = hi + lo, two 16-bit planes; gemm_epilogue.h RESID_SPLIT): fp32 rows -> planes + row statistics, and
// the fp32 LayerNorm of selected rows (the CLS rows) of the planes
hipError_t launch_rowstats_split(const float* x, int64_t rows, int dim, float eps, void* hi, void* lo, float* stats, int dtype,
                                 hipStream_t stream, int64_t guard_rows = 0, unsigned int* amax_guard = nullptr);
// pre-LayerNorm of VH_FLAG_PRE_LN contexts (kernels_rows.hip): y = LN(x) gamma + beta -> fp32 rows (y32, may alias x), the split
// residual's planes / the plain operand copy (hi, lo) and layer 0's row statistics of y; every output is optional, one of
// y32 / hi is needed.  guard / amax_guard as launch_finalize_stats / launch_rowstats_cast, over the first guard_rows rows.
hipError_t launch_pre_layernorm(const float* x, int64_t rows, int dim, const float* gamma, const float* beta, float eps, float* y32,
                                void* hi, void* lo, float* stats, int dtype, hipStream_t stream, int64_t guard_rows = 0,
                                unsigned int* guard = nullptr, unsigned int* amax_guard = nullptr);
hipError_t launch_layernorm_split(const void* hi, const void* lo, int64_t rows, int dim, int64_t row_stride, const float* gamma,
                                  const float* beta, float eps, float* out32, int dtype, hipStream_t stream);
// Token features (kernels_features.hip; contract: vithip.h, "Token features"): the rows of a residual stream [batch * tokens, dim]
// -> the caller's element type (VH_ELEM_F32 / F16 / BF16), as they are (VH_FEAT_RAW) or through LayerNorm(gamma, beta, eps)
// (VH_FEAT_NORM), and the mean over an image's patch tokens (tokens lead .. tokens - 1, a serial fp32 chain in that order; lead = 1 + the register
// tokens, which go to `reg`).
// form: VH_DTYPE_BF16 / FP16 = split planes (hi 16-bit, lo one scaled e4m3 byte), VH_DTYPE_FP8 = e4m3 hi + bf16 lo,
// VH_FEAT_FORM_F32 = fp32 rows in `hi`, lo null.  cls [batch][dim] <- token 0, patch [batch][tokens - lead][dim] <- tokens lead .., mean
// [batch][dim]; any may be null, not all.  stats [batch * tokens][2]: scratch of the normalised mean (row kernel writes, mean
// kernel reads).  features_check: nullptr, or why the launch is refused; host arithmetic only.
constexpr int VH_FEAT_FORM_F32 = -1;
struct FeatureArgs {
    const void* hi;
    const void* lo;
    int form;
    int batch, tokens, dim;
    const float* gamma;
    const float* beta;
    float eps;
    int elem, norm;
    void* cls;
    void* patch;
    void* mean;
    float* stats;
    int lead = 1;   // rows in front of an image's patch rows: 1 .. tokens - 1
    void* reg = nullptr;               // [batch][lead - 1][dim] <- tokens 1 .. lead - 1 (the register rows); needs lead >= 2
    int patch_layout = VH_FEAT_ROWS;   // VH_FEAT_NCHW: patch is [batch][dim][tokens - lead] (feat_nchw_kernel), the same elements transposed
    // the rows of a VH_FLAG_NO_CLS context (internal launches only; the public taps leave it 0 and keep their bounds): no class-token
    // row, lead = 0 .. tokens - 1 rows that are ALL register rows (reg [batch][lead][dim]), cls refused
    int no_cls = 0;
};
const char* features_check(const FeatureArgs& a);
hipError_t launch_token_features(const FeatureArgs& a, hipStream_t stream);
// The pooled head's input in one pass (kernels_features.hip pool_rows_kernel; contract: vithip.h VH_FLAG_POOL, vh_op_pool_rows):
// out[b][0 .. dim) (row stride out_stride, 0 = dim) <- the fp32 mean over rows lead .. tokens - 1 of image b, the bits
// launch_token_features gives for `mean`.  lead = 0 .. tokens - 1.  cls_in / cls_out (both or neither; VH_POOL_CLS_AVG): the same
// launch copies cls_in [batch][dim] into cls_out [batch][0 .. dim) (row stride out_stride).  pool_check: nullptr, or why refused.
struct PoolArgs {
    const void* hi;
    const void* lo;
    int form;
    int batch, tokens, lead, dim;
    const float* gamma;
    const float* beta;
    float eps;
    int norm;
    float* out;
    int64_t out_stride = 0;
    const float* cls_in = nullptr;
    float* cls_out = nullptr;
};
const char* pool_check(const PoolArgs& a);
hipError_t launch_pool_rows(const PoolArgs& a, hipStream_t stream);
// The token-sized pass of the VH_FLAG_MAP_HEAD head (kernels_features.hip map_pool_kernel; contract: vithip.h VH_FLAG_MAP_HEAD,
// vh_op_map_pool): z [batch][heads][dim] <- the softmax(qk[h] . LN(row))-weighted sum of the normalised patch rows.  The PoolArgs
// fields mean what they mean to launch_pool_rows (norm must be VH_FEAT_NORM; out = z; out_stride, cls_in, cls_out unused).
// map_pool_check: nullptr, or why refused.  map_pool_group: the rows per group at this dim and head count (tests sit on its edges).
const char* map_pool_check(const PoolArgs& a, const float* qk, int heads);
hipError_t launch_map_pool(const PoolArgs& a, const float* qk, int heads, hipStream_t stream);
int map_pool_group(int dim, int heads);
// The rows of a tapped layer into the capture store (vithip.h "Layer features"): bytes_hi of the hi plane (or the fp32 array), then
// bytes_lo of the lo plane (0: none), in ONE launch.  Pointers and byte counts are multiples of 16.
hipError_t launch_feature_capture(const void* src_hi, void* dst_hi, size_t bytes_hi, const void* src_lo, void* dst_lo, size_t bytes_lo,
                                  hipStream_t stream);
// fp8 path: the folded weights as e4m3 rows + scales (wscale), c = wscale * sum of the decoded row, d as launch_fold_ln
hipError_t launch_fold_ln_f8(const float* w, const float* b, const float* gamma, const float* beta, int rows, int dim,
                             float scale, void* w8, float* wscale, float* c, float* d, hipStream_t stream);
hipError_t launch_fold_ln(const float* w, const float* b, const float* gamma, const float* beta, int rows, int dim,
                          float scale, void* w16, float* c, float* d, int dtype, hipStream_t stream);
// MLP mode: y = act(W x + b), W [n_out, n_in] fp32
hipError_t launch_dense_layer(const float* w, const float* b, const float* x, float* y, int n_in,
                              int n_out, int n_vec, int activation, hipStream_t stream, float* z = nullptr);
// MLP-mode training (kernels_misc.hip): last-layer delta + error, hidden-layer delta, parameter update
hipError_t launch_mlp_out_delta(const float* a, const float* z, const float* t, float* d, int64_t n, int act, float* err,
                                hipStream_t stream);
hipError_t launch_mlp_back_delta(const float* w, const float* d, const float* z_prev, float* d_prev, int n_in, int n_out,
                                 int n_sets, int act, hipStream_t stream);
hipError_t launch_mlp_update(float* w, float* b, const float* d, const float* x, int n_in, int n_out, int n_sets, float scale,
                             hipStream_t stream);

// 3x3 filter on 8-bit frames (filter_image): kind 0 = binomial blur, 1 = Sobel |gx|+|gy|
hipError_t launch_filter3x3(const uint8_t* in, uint8_t* out, int h, int w, int kind, hipStream_t stream);

// ---- launcher-side caches: reached concurrently from the device-group member threads (vh_group_*, one host thread per
// device), so none of them is a plain static.  Environment knobs are function-local `static const` values (C++11: the
// initialiser runs exactly once, other threads wait for it); per-device facts are tables of relaxed atomics indexed by
// the device ordinal (every writer stores the same value).
constexpr int kMaxDevices = 64;
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// number of CUs of the CURRENT device (0 on error)
inline int device_num_cu() {
    static std::atomic<int> table[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
    int n = table[dev].load(std::memory_order_relaxed);
    if (n) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
    table[dev].store(n, std::memory_order_relaxed);
    return n;
}
// Opt a kernel in to `bytes` of dynamic LDS on the CURRENT device.  The attribute is per device, so the record of
// what has been set is too: `done[d]` = bytes already granted on device d (one table per kernel instantiation).
using LdsDone = std::atomic<int>[kMaxDevices];
inline hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes, LdsDone& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    if ((size_t)done[dev].load(std::memory_order_acquire) >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done[dev].store((int)bytes, std::memory_order_release);
    return e;
}

}  // namespace vh
