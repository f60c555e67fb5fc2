/*
 * vithip.h — C ABI of libvithip.so, the MI355X (gfx950) backend that replaces the
 * device side of LimpBunion22/VIT-FPGA's `fpga::net_fpga`.
 *
 * The reference has no FFI layer of its own: `src/netFPGA.cpp` talks to OpenCL
 * directly.  Every entry point below therefore cites the reference *call site*
 * (file:line under /root/reference) whose job it takes over.  Signatures carry only
 * plain pointers, sizes and PODs (no HIP, torch or C++ types) so the header is usable
 * from C, from plain g++ (host/netHIP.cpp), and from ctypes/cgo/JNI style bindings
 * (INTEGRATION.md shows the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - every function returns VH_OK (0) or a VH_ERR_* code; the human-readable reason is
 *     available through vh_last_error().  Nothing here calls exit(): the reference's
 *     fatal-on-error convention (aocl_utils::checkError -> cleanup() -> exit,
 *     netFPGA.cpp:274-278) is re-created, if wanted, by the C++ class above this ABI.
 *   - "dev" pointers are device (HBM) addresses of the context's GPU, "host" pointers are
 *     ordinary process memory.  The caller owns every buffer it passes in.
 *   - a context is not re-entrant; distinct contexts may be used from distinct threads.
 */
#ifndef VITHIP_H
#define VITHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VH_ABI_VERSION 1

/* status codes */
#define VH_OK 0
#define VH_ERR_INVALID 1     /* bad argument / shape the kernels do not support       */
#define VH_ERR_HIP 2         /* a HIP runtime call failed (message has hipGetErrorString) */
#define VH_ERR_STATE 3       /* call order violated (e.g. forward before weights)     */
#define VH_ERR_UNSUPPORTED 4 /* valid request that this build does not implement      */
#define VH_ERR_NO_DEVICE 5   /* no gfx950 device visible                              */
#define VH_ERR_RING_FULL 6   /* vh_ring_submit: every slot is in flight (reference: "PILA LLENA") */
#define VH_ERR_RING_EMPTY 7  /* vh_ring_collect: nothing in flight (reference: "PILA VACIA")      */

/* arithmetic type of the dense contractions (MFMA operand type; accumulation is fp32) */
#define VH_DTYPE_BF16 0
#define VH_DTYPE_FP16 1
/* fp8 GEMMs (BASELINE config 5): the four per-layer GEMMs run on v_mfma_scale_f32_16x16x128_f8f6f4 with OCP
 * e4m3 operands -- weights quantised at load with one fp32 scale per output channel, activations cast unscaled
 * (saturating at +-448) by the kernel that produces them; fp32 accumulation, fp32 residual stream; patch embedding,
 * attention and the head stay bf16.  Needs dim % 128 == 0 and mlp_dim % 128 == 0. */
#define VH_DTYPE_FP8 2

/* activation selector of MLP mode.  The reference stores `activations = 1 // RELU2`
 * (netFPGA.cpp:79) but never defines it (the network_v1 kernel source is absent), so the
 * numeric codes below are this build's definition; see DESIGN.md "parity unpinned". */
#define VH_ACT_IDENTITY 0
#define VH_ACT_RELU2 1    /* min(max(x,0), MAX_RANGE=1)  (def/defines.h:11-12 value range) */
#define VH_ACT_RELU 2
#define VH_ACT_HARDTANH 3 /* clamp(x, MIN_RANGE=-1, MAX_RANGE=1) */
#define VH_ACT_GELU 4     /* exact erf GELU */

/* Vision-Transformer shape.  Replaces the role `net::net_data` (def/defines.h:14-23) plays
 * for the MLP: it is what sizes the device buffers (_init_kernel, netFPGA.cpp:402-441). */
typedef struct vh_config {
    int32_t image_size; /* square input side, e.g. 224; tokens = (image_size / patch_size)^2 + 1 + registers <= 4097, and
                         * max_batch x tokens <= 640 x 2^20                                                   */
    int32_t patch_size; /* any divisor of image_size up to 256, e.g. 14 or 16 (the patch GEMM runs on the patch
                         * vector patch^2 * channels zero-padded to a multiple of 64)                         */
    int32_t channels;   /* 1..64, e.g. 3                                   */
    int32_t dim;        /* D, hidden size (multiple of 64)                 */
    int32_t heads;      /* H, divides dim; head dim dim/heads is 32, 48, 64, 80, 96, 112 or 128 */
    int32_t mlp_dim;    /* M (multiple of 64)                              */
    int32_t layers;     /* L                                               */
    int32_t classes;    /* C (multiple of 4)                               */
    int32_t dtype;      /* VH_DTYPE_*                                      */
    int32_t max_batch;  /* workspace is sized for this many images         */
    float ln_eps;       /* 1e-6 for the canonical ViT                      */
    int32_t flags;      /* VH_FLAG_* (0 = library defaults); unknown bits are rejected */
} vh_config;

/* vh_config.flags.  LayerNorm folding: with dim and mlp_dim multiples of 256 the two LayerNorms of a layer can be folded
 * into the neighbouring GEMMs (DESIGN.md "LayerNorm folded into the GEMMs"): the GEMM then multiplies the RAW
 * 16-bit-rounded residual rows, whose rounding error relative to the centred signal grows with
 * sqrt(1 + (row mean / row sigma)^2).  Three settings:
 *   flags == 0 (default)   the GUARDED fold: folded, and every forward measures max |mean| / sigma over its rows
 *                          (vh_get_ln_guard).  The decision is taken first WHEN THE WEIGHTS ARE LOADED: every vh_load_weights* /
 *                          vh_init_weights_seeded ends with one calibration forward of a seeded image, and a checkpoint whose
 *                          rows exceed the threshold (0.5; environment VH_LN_GUARD) -- a property of the weights far more than
 *                          of the image -- leaves the load on the stand-alone LayerNorm, so no entry point, asynchronous
 *                          ones included, ever returns a batch from a fold the weights had tripped.  Behind that, every
 *                          forward still measures: once a COMPLETED forward has exceeded the threshold because of its DATA
 *                          the context switches for good (the weights are prepared again from the resident blob) at the
 *                          next forward entry or vh_synchronize; the synchronous vh_forward repeats the very forward that
 *                          tripped it, the asynchronous entry points have by then delivered that batch from the folded
 *                          path (vh_get_ln_guard reports `tripped`), and from then on logit bits differ from a context
 *                          that never tripped -- bit-reproducibility across runs holds for ON / OFF, and for the default
 *                          as long as no input trips the backstop.
 *                          VH_DTYPE_FP8 contexts guard a second quantity: the folded GEMMs multiply the RAW residual rows
 *                          as e4m3, which saturates at 448, so the statistics kernels also track max |x| (vh_get_fp8_guard)
 *                          and rows beyond 448 switch the context to the stand-alone LayerNorm operand (normalised values
 *                          fit e4m3) in the same way, calibration forward included.
 *   VH_FLAG_LN_FOLD_ON     always folded: the explicit throughput choice.  The guard still measures, never switches.
 *   VH_FLAG_LN_FOLD_OFF    always the stand-alone LayerNorm kernel.
 * With ON or OFF the path depends on the model shape and the flags ONLY (never on max_batch or on the data), so a given
 * image gives the same logit bits from every context of one configuration; with the default it depends, in addition, on
 * whether the guard has tripped (vh_get_ln_fold tells).  Environment overrides, honoured only when flags == 0 and meant
 * for A/B tools: VH_LN_FOLD=0|1 (forces the path and disables the switch), VH_RESID_SPLIT=0 (fp32 residual stream instead
 * of the two 16-bit planes). */
#define VH_FLAG_LN_FOLD_OFF 1 /* always run the stand-alone LayerNorm kernel                */
#define VH_FLAG_LN_FOLD_ON 2  /* always fold where the shapes allow it (no run-time switch)  */
/* Weight-only e4m3 (16-bit dtypes only): the q, k, v, out-projection, fc1 and fc2 matrices are quantised to OCP e4m3
 * with one fp32 scale per output channel when the weights are loaded and dequantised again before the 16-bit
 * preparation, so the GEMMs multiply 16-bit activations with e4m3-valued weights (SURVEY.md section 7 option (a); the
 * other reading of "fp8", both operands e4m3 on the scaled-MFMA path, is VH_DTYPE_FP8).  Throughput is that of the
 * 16-bit dtype: at batch 512 the weights are 0.3 % of a forward's HBM traffic, which is all a 1-byte copy would save. */
#define VH_FLAG_W8_E4M3 4
/* Class-token tail (opt-in): the logits depend on the LAST layer's class-token row only, so with this flag the last layer runs
 * attention for that one query (all keys / values) and out-proj, fc1, fc2, the final LayerNorm and the head on `batch` rows
 * instead of batch x tokens.  Logits agree with the default path to rounding (not bitwise: the one-query attention is a
 * different kernel); the residual rows of the other tokens are NOT updated by the last layer (vh_debug_read of the hidden
 * state returns them as of the layer before).  Folded 16-bit path only (ignored elsewhere).  Never used by the default bench
 * line: a forward that skips rows is reported as its own `cls_tail` object. */
#define VH_FLAG_CLS_TAIL 8
/* The two places where CLIP's vision towers differ from the canonical ViT block; independent of each other and of every flag above
 * (OpenAI CLIP sets both, the LAION / OpenCLIP towers the first only).  They describe the MODEL, so the weight blob's header carries
 * them too (flags word bit 1 = pre-LN, bit 2 = QuickGELU) and a blob whose bits differ from the context's is refused.
 *   VH_FLAG_PRE_LN      a LayerNorm over the embedded tokens (patch embedding + class token + position embedding) in front of
 *                       layer 0, CLIP's `ln_pre`.  The blob gains pre_ln.weight [D] and pre_ln.bias [D] directly after `pos`.
 *   VH_FLAG_QUICK_GELU  the MLP activation is x * sigmoid(1.702 x) instead of erf GELU.  No tensor of its own.
 * With patch.bias = 0, the final LayerNorm = ln_post and head = the visual projection (classes = embedding width, head.bias = 0)
 * the logits of such a context are the CLIP image embedding. */
#define VH_FLAG_PRE_LN 16
#define VH_FLAG_QUICK_GELU 32
/* Register tokens (DINOv2 "with registers" and every tower trained like it): R learned rows between the class token and the patch
 * rows of every image.  The count travels in bits 9 .. 13 of flags (bit 8 stays an unknown bit, as it was), 0 .. 16 (17 .. 31 are refused); it describes the MODEL, so the
 * blob header's flags word carries it in the same bits and a blob whose count differs from the context's is refused.  Independent
 * of every other flag and of the dtype.
 *   tokens T = (image_size / patch_size)^2 + 1 + R; the bounds on tokens (<= 4097, max_batch x tokens <= 640 x 2^20) apply to that
 *   number, so a 64 x 64 grid takes no register.  VH_FLAG_CLS_TAIL keeps its T <= 1024 condition.
 *   Blob: `pos` stays [(NP + 1)][D] (registers carry no position embedding); a tensor `reg` [R][D] follows it directly, in front
 *   of pre_ln.* when both are present.  vh_init_weights_seeded: tensor id 7, sigma as `cls`, offset 0.
 *   Row order of the residual stream (Hugging Face's hidden_states order), NP = patches per image:
 *     row 0          = cls + pos[0]                      (one fp32 addition)
 *     rows 1 .. R    = reg[r]                            (the fp32 value as it is)
 *     row 1 + R + p  = patch embedding of p + pos[1 + p] (the bits of an R = 0 context's row 1 + p)
 *   On the fp32 residual paths the leading rows hold exactly those fp32 numbers.  On the split-residual path (folded 16-bit, dim %
 *   256 == 0) a leading row of value x is stored like every other row: hi = the 16-bit rounding of x, lo = the scaled e4m3 byte of
 *   x - hi, with the per-64-column (sum, sum of squares) of the fp32 x beside it -- vh_debug_read returns hi + decode(lo).
 *   With R = 0 every kernel writes the bytes it wrote before the flag existed.
 * Token features skip the register rows: cls <- row 0, patch[b][p] <- row 1 + R + p, mean over those NP rows.  The register rows
 * themselves (DINOv2's x_norm_regtokens) are not a field of vh_features, a fixed 32-byte struct: vh_layer_features.reg ("Layer
 * features") returns them. */
#define VH_FLAG_REGISTERS(n) (((n) & 31) << 9)
#define VH_FLAG_REGISTERS_MASK (31 << 9)
#define VH_FLAG_REGISTERS_OF(flags) (((flags) & VH_FLAG_REGISTERS_MASK) >> 9)
#define VH_MAX_REGISTERS 16

/* Pooled heads and models without a class token (I-JEPA, DINOv2's ImageNet linear classifiers, timm's global_pool='avg', BEiT's
 * pooler).  Two MODEL switches, in bits 15 .. 17 of flags and, with the same values, of the blob header's flags word; a blob whose
 * bits differ from the context's is refused.  With both clear nothing changes: every kernel gets the arguments it got before.
 *   VH_FLAG_POOL(m): what the head multiplies, [batch][W] fp32 (vh_debug_read(ctx, 1)); p runs over the NP patch rows ONLY, never
 *   over the class token or the register rows; the LayerNorm is the blob's lnf.* in every mode.
 *     VH_POOL_CLS         head(LN(row 0))                                W = D   (the default)
 *     VH_POOL_AVG_NORM    head(mean_p LN(x_p))                           W = D   I-JEPA; timm global_pool='avg' with fc_norm=False
 *     VH_POOL_AVG_FCNORM  head(LN(mean_p x_p))                           W = D   timm global_pool='avg' + fc_norm, BEiT's pooler
 *     VH_POOL_CLS_AVG     head(concat(LN(row 0), mean_p LN(x_p)))        W = 2 D head.weight [C][2 D], class-token half first
 *   ARITHMETIC, for bits ("Token features" below): the AVG_NORM vector is what vh_read_features(mean, VH_FEAT_NORM, VH_ELEM_F32)
 *   returns after the same forward -- the two-pass fp32 row statistics, fmaf((x - mean) * rstd, gamma, beta), the serial fp32 chain
 *   over the patch rows ascending, times (float)(1.0 / NP).  AVG_FCNORM: the VH_FEAT_RAW mean of the same definition, then the fp32
 *   LayerNorm of vh_op_layernorm_f32 over [batch][D].  CLS_AVG: columns 0 .. D - 1 are the vector VH_POOL_CLS computes (the same
 *   launch), columns D .. 2 D - 1 the AVG_NORM vector.  logits = the fp32 head over W columns.  The result never depends on the
 *   batch, the launch geometry or the stream part an image runs in.
 *   VH_FLAG_NO_CLS: the model has no class token.  tokens T = NP + R; the blob has no `cls` tensor and `pos` is [NP][D]; row order
 *   reg[0 .. R - 1], then patch p + pos[p] (the bits of the class-token context's patch rows for the same tensors).  The pooling
 *   mode must be VH_POOL_AVG_NORM or VH_POOL_AVG_FCNORM.
 *   Refused by vh_create / vh_weight_blob_bytes, each with a message of its own: VH_FLAG_NO_CLS with VH_POOL_CLS or VH_POOL_CLS_AVG;
 *   VH_FLAG_CLS_TAIL with either switch (its last layer does not update the patch rows).  The token bounds apply to the new T.
 *   vh_init_weights_seeded keeps every tensor id; `head` is id "head" with its [C][W] shape. */
#define VH_FLAG_NO_CLS (1 << 15)
#define VH_FLAG_POOL(m) (((m) & 3) << 16)
#define VH_FLAG_POOL_MASK (3 << 16)
#define VH_FLAG_POOL_OF(flags) (((flags) & VH_FLAG_POOL_MASK) >> 16)
#define VH_POOL_CLS 0
#define VH_POOL_AVG_NORM 1
#define VH_POOL_AVG_FCNORM 2
#define VH_POOL_CLS_AVG 3

/* SigLIP's vision towers (SigLIP, SigLIP 2 fixed-size, PaliGemma's tower; timm's global_pool='map'): two MODEL switches, independent of
 * each other, in bits 19 and 21 of flags and, at the same positions, of the blob header's flags word; a blob whose bits differ from
 * the context's is refused with a message that names the bit.  With both clear nothing changes.
 *   VH_FLAG_TANH_GELU  the MLP activation is 0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3))) ("gelu_pytorch_tanh") instead of erf
 *                      GELU.  No tensor of its own; excludes VH_FLAG_QUICK_GELU.  With VH_FLAG_NO_CLS | VH_FLAG_POOL(VH_POOL_AVG_NORM)
 *                      such a context is SiglipForImageClassification; vh_read_features gives a SigLIP tower's patch features.
 *   VH_FLAG_MAP_HEAD   the head's input is the multihead attention-pooling block ("MAP"): ONE learned query attends over the NP
 *                      patch rows, followed by a LayerNorm + MLP with a residual.  With an identity head (classes = D) the logits
 *                      are SiglipVisionModel's pooler_output.  Needs VH_FLAG_NO_CLS; excludes a non-zero VH_FLAG_POOL field,
 *                      register tokens and VH_FLAG_CLS_TAIL; heads <= 16.  Each refusal has a message of its own.
 *   Blob tensors of a MAP context, all fp32, directly after head.bias (no other offset moves), H = heads, M = mlp_dim:
 *     map.qk [H][D], map.v.weight [D][D], map.v.bias [D], map.o.weight [D][D], map.o.bias [D], map.ln.weight [D], map.ln.bias [D],
 *     map.fc1.weight [M][D], map.fc1.bias [M], map.fc2.weight [D][M], map.fc2.bias [D].
 *     map.qk[h] = W_k,h^T (W_q,h probe + b_q,h) / sqrt(hd): the query is the same for every image, so the CONVERTER folds it through
 *     the key projection (in float64; vithip.py blob_from_siglip_state_dict); the key bias adds a per-head constant to every score,
 *     which the softmax cancels exactly.  The library holds no fold code.  vh_init_weights_seeded: tensor ids 0x7010 .. 0x701A in
 *     this order, sigma 0.02 (map.ln.weight: 0.05 around 1).
 *   THE FUNCTION, per image; t runs over the NP patch rows, x_t = the final residual row:
 *     y_t    = LN(x_t; lnf)                        fp32, the row arithmetic of "Token features" (VH_FEAT_NORM)
 *     s[h,t] = qk[h] . y_t
 *     p[h,.] = softmax_t s[h,.]
 *     z[h]   = sum_t p[h,t] y_t                    [H][D]  (sum_t p (W_v y_t + b_v) = W_v z + b_v: the weights sum to 1, so V is
 *                                                           never projected per token; vh_op_map_pool is this step alone)
 *     a[h hd + j] = v.weight[h hd + j] . z[h] + v.bias[h hd + j]
 *     o      = o.weight a + o.bias
 *     u      = o + fc2(act(fc1(LN(o; map.ln))))    act = the context's activation (erf, quick or tanh), evaluated in fp32
 *     vh_debug_read(ctx, 1) = u [batch][D];  logits = head(u), the fp32 head over W = D columns.
 *   Everything behind z is fp32 arithmetic on [batch] rows.  An image's bits depend on its rows alone: never on the batch, the
 *   stream part or graph replay. */
#define VH_FLAG_MAP_HEAD (1 << 19)
#define VH_FLAG_TANH_GELU (1 << 21)
#define VH_MAP_MAX_HEADS 16

/* Rotary position embedding (DINOv3 ViT-S/B/L; the mechanism of EVA-02 and Pixtral-style towers): ONE MODEL switch, in bit 23 of
 * flags and, at the same position, of the blob header's flags word; a blob whose bit differs from the context's is refused with a
 * message that names the bit.  With the bit clear nothing changes: not one launch.
 *   VH_FLAG_ROPE   q and k of every patch row are rotated by per-position angles in every layer, in front of attention.  The library
 *                  holds no trigonometry: the angles are DATA.  Excludes VH_FLAG_CLS_TAIL (its one-query kernel reads q and k of the
 *                  last layer on a path of its own), with a message of its own.  Every accepted head dim has hd / 2 a multiple of 8.
 *   Blob tensors of a ROPE context, both fp32, at the VERY END of the blob (behind head.bias, and behind the map.* tensors where
 *   there are any: no other offset moves), NP = patch rows, hd = dim / heads:
 *     rope.cos [NP][hd / 2], rope.sin [NP][hd / 2].
 *     vh_init_weights_seeded: tensor id 0x7030 (the ANGLES a[i] = pi * uniform[-1, 1) of the generator, i = p * hd / 2 + d); rope.cos =
 *     (float)cos((double)a), rope.sin = (float)sin((double)a): a synthetic model is a true rotation.  pos stays in the blob (a
 *     converter of a model without a position table writes zeros; a model with both kinds of position needs nothing more).
 *   THE FUNCTION, per layer, per image and per head, on q and on k alike (v is not touched).  Row lead + p is patch row p; the `lead`
 *   rows in front (class token, registers) pass through untouched, bit for bit.  For d < hd / 2, c = rope.cos[p][d], s = rope.sin[p][d]:
 *     out[d]          = x[d] c - x[d + hd / 2] s
 *     out[d + hd / 2] = x[d + hd / 2] c + x[d] s            (Hugging Face's rotate_half form)
 *   The softmax scale the library folds into q is a scalar and commutes with the rotation.
 *   ROUNDING: x is the STORED 16-bit q or k the projection wrote (one rounding, as in every model); it is widened to fp32, rotated in
 *   fp32 as fmaf(x[d], c, -(x[d + hd/2] s)) and fmaf(x[d + hd/2], c, x[d] s), and rounded ONCE (RNE) back to the same 16-bit type, in
 *   place.  A ROPE model's q and k therefore carry one rounding more than another model's.  fp8 contexts keep q|k|v in bf16.
 *   Attention maps of a ROPE context are of the rotated q and k: the model's own.  An image's bits depend on its rows alone. */
#define VH_FLAG_ROPE (1 << 23)

/* SwiGLU MLP (DINOv2-g/14, DINOv3 ViT-H+/16 and 7B; the gated MLP of many later towers): ONE MODEL switch, in bit 25 of flags and, at
 * the same position, of the blob header's flags word; a blob whose bit differs from the context's is refused with a message that names
 * the bit.  With the bit clear nothing changes: not one launch.
 *   VH_FLAG_SWIGLU  the MLP of every layer is gated.  mlp_dim = M is the GATED width: fc2's K (4096 for DINOv2-g/14).  Excludes, each
 *                   with a message of its own (vh_weight_blob_bytes returns 0): VH_FLAG_QUICK_GELU and VH_FLAG_TANH_GELU (one MLP
 *                   activation), VH_FLAG_MAP_HEAD (the head's own MLP block is not gated), VH_FLAG_CLS_TAIL, VH_FLAG_W8_E4M3 and
 *                   VH_DTYPE_FP8 (an e4m3 h needs a rounding contract of its own and fc1 scales of width 2 M: the open step).
 *   Blob tensors of a SWIGLU context: l{l}.fc1.weight is [2 M][D] and l{l}.fc1.bias is [2 M]; rows 0 .. M - 1 are the GATE (Hugging Face:
 *   the first half of weights_in, or gate_proj), rows M .. 2 M - 1 the VALUE (the second half of weights_in, or up_proj).  fc2 stays
 *   [D][M] + [D]; no other offset rule changes.  vh_init_weights_seeded fills the longer tensors from the same tensor ids (t + 12, t + 13).
 *   THE FUNCTION, per layer and per row, with z = LN2(x) W1^T + b1 [2 M], g = z[0 .. M - 1], u = z[M .. 2 M - 1]:
 *     x += (silu(g) * u) W2^T + b2,      silu(g) = g * sigmoid(g)
 *   ROUNDING: fc1 stores z as 16-bit (one rounding MORE than a GELU model has: there the activation is applied to the fp32 accumulator);
 *   the gate pass widens the stored g and u to fp32, computes r = rcp(1 + exp2(g * -log2(e))) on the hardware exp2 / rcp the QuickGELU
 *   epilogue uses (1 ulp each) and h = (g * r) * u in fp32, and rounds ONCE (RNE) to the same 16-bit type: the h that fc2 reads.  g = 0
 *   gives h = 0 for every finite u.  A row's bits depend on that row alone. */
#define VH_FLAG_SWIGLU (1 << 25)

typedef struct vh_ctx vh_ctx; /* opaque ViT context (device, stream, weights, workspace) */
typedef struct vh_mlp vh_mlp; /* opaque MLP-mode context (the reference's real semantics)  */

/* ---- library / device ---------------------------------------------------------------- */
int vh_abi_version(void);
/* replaces clGetPlatformIDs/clGetDeviceIDs (netFPGA.cpp:371-377) */
int vh_device_count(int* count);
/* last error of the calling thread (ctx may be NULL) or of that context */
const char* vh_last_error(const vh_ctx* ctx);

/* ---- raw device memory helpers (so that bindings need no HIP of their own) ------------ */
int vh_malloc(int device, size_t nbytes, void** dev_ptr);
int vh_free(int device, void* dev_ptr);
int vh_memcpy_h2d(int device, void* dev_dst, const void* host_src, size_t nbytes);
int vh_memcpy_d2h(int device, void* host_dst, const void* dev_src, size_t nbytes);
int vh_device_synchronize(int device);
int vh_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes);   /* hipMemGetInfo */

/* ---- ViT context ---------------------------------------------------------------------- */
/* replaces _init_program + _init_kernel(const char*) (netFPGA.cpp:367-441): device,
 * stream and every device buffer, sized from the net shape. */
int vh_create(const vh_config* cfg, int device, vh_ctx** out);
/* replaces cleanup() + ~net_fpga (netFPGA.cpp:613-651); frees ALL device memory. */
int vh_destroy(vh_ctx* ctx);
int vh_get_config(const vh_ctx* ctx, vh_config* out);
/* the number of register tokens of the context (VH_FLAG_REGISTERS_OF(flags)); -1 for a NULL context */
int vh_get_register_tokens(const vh_ctx* ctx);
/* *on = 1 when this context folds its LayerNorms into the GEMMs (vh_config.flags, model shape, dtype) */
int vh_get_ln_fold(const vh_ctx* ctx, int* on);
/* the fold's run-time guard (see VH_FLAG_LN_FOLD_*): *max_ratio = the largest |row mean| / row sigma any LayerNorm input
 * row has shown since the weights were loaded (0 when the context never folded), *threshold = the switch point,
 * *tripped = 1 once it was exceeded.  Synchronises the context's stream.  Any pointer may be NULL. */
int vh_get_ln_guard(vh_ctx* ctx, float* max_ratio, float* threshold, int* tripped);
/* VH_DTYPE_FP8 contexts: *max_abs = the largest |x| (an upper bound of it: the root sum of squares of a row's largest
 * 64-column block; exact for layer 0) any residual row has shown since the weights were loaded, *limit = 448 (e4m3).  Beyond
 * the limit the guarded fold switches to the stand-alone LayerNorm (vh_get_ln_guard reports `tripped`).  0 for 16-bit
 * contexts.  Synchronises the context's stream.  Either pointer may be NULL. */
int vh_get_fp8_guard(vh_ctx* ctx, float* max_abs, float* limit);

/* Weight blob = fp32 tensors in canonical order (DESIGN.md "weight blob") preceded by a
 * 64-byte header (its flags word: bit 0 = file checksum present, bit 1 = VH_FLAG_PRE_LN model, bit 2 = VH_FLAG_QUICK_GELU model, bits 9 .. 13 = the register-token count, bit 15 = VH_FLAG_NO_CLS model, bits 16 .. 17 = its VH_FLAG_POOL mode, bit 19 = VH_FLAG_MAP_HEAD model, bit 21 = VH_FLAG_TANH_GELU model, bit 23 = VH_FLAG_ROPE model, bit 25 = VH_FLAG_SWIGLU model).  Replaces _load_params (netFPGA.cpp:484-515): uploads, converts to the
 * MFMA operand type, permutes the patch kernel to NHWC order and fuses q|k|v. */
size_t vh_weight_blob_bytes(const vh_config* cfg);
int vh_load_weights(vh_ctx* ctx, const void* host_blob, size_t nbytes);
/* same, blob already resident on this context's GPU (e.g. after an RCCL broadcast) */
int vh_load_weights_device(vh_ctx* ctx, const void* dev_blob, size_t nbytes);
/* deterministic synthetic weights generated on the device (generator: DESIGN.md "synthetic
 * data"); replaces the reference's `random` ctor branch (netFPGA.cpp:82-88) for ViT mode. */
int vh_init_weights_seeded(vh_ctx* ctx, uint64_t seed);
/* canonical fp32 blob currently loaded, copied back to the host / to a device buffer
 * (the inverse direction of the ctor flatten, cf. get_net_data netFPGA.cpp:206-237) */
int vh_export_weights(vh_ctx* ctx, void* host_blob, size_t nbytes);
int vh_export_weights_device(vh_ctx* ctx, void* dev_blob, size_t nbytes);

/* Weight blob on disk (the reference's own attempt at reading weights back, get_net_data
 * netFPGA.cpp:206-237, is a broken TODO and it has no file format).  The file is the canonical blob byte for
 * byte, plus an FNV-1a-64 checksum of the parameter bytes in header words that memory blobs leave zero.
 *   vh_blob_file_config: host only (no device needed) -- validates magic / shape / file length and fills the model
 *                        fields of *cfg (dtype = VH_DTYPE_BF16, max_batch = 1: set what you need before vh_create;
 *                        cfg->flags = the model bits of the header: VH_FLAG_PRE_LN, VH_FLAG_QUICK_GELU, VH_FLAG_REGISTERS(n), VH_FLAG_NO_CLS,
 *                        VH_FLAG_POOL(m), VH_FLAG_MAP_HEAD, VH_FLAG_TANH_GELU, VH_FLAG_ROPE, VH_FLAG_SWIGLU);
 *   vh_save_weights_file: writes <path>.tmp then renames; vh_load_weights_file: verifies length, shape, checksum. */
int vh_blob_file_config(const char* path, vh_config* cfg);
/* host only: the file as a MEMORY blob (what vh_load_weights takes): length, header and checksum verified, checksum
 * words cleared.  nbytes must equal vh_weight_blob_bytes of the file's configuration. */
int vh_blob_file_read(const char* path, void* host_blob, size_t nbytes);
int vh_save_weights_file(vh_ctx* ctx, const char* path);
int vh_load_weights_file(vh_ctx* ctx, const char* path);

/* The hot path.  Replaces launch_forward's device section (netFPGA.cpp:262-284):
 * in  = batch x image x image x channels fp32, NHWC, host memory;
 * out = batch x classes fp32 logits, host memory.  Synchronous, like the blocking read. */
int vh_forward(vh_ctx* ctx, const float* in_nhwc_host, int batch, float* logits_host);
/* same with both buffers resident in HBM (zero-copy boundary used by bench.py). Enqueues on
 * the context's stream and waits for completion. */
int vh_forward_device(vh_ctx* ctx, const float* in_nhwc_dev, int batch, float* logits_dev);
/* enqueue only; pair with vh_synchronize().  `steps` back-to-back forwards of the same
 * buffers are enqueued (the timed region of bench.py).
 * TWO FORWARDS IN FLIGHT.  The steps of one call do not depend on each other, and neither do consecutive submits of an image
 * ring (vh_ring_create, _u8, _tensor).  A context therefore has two compute streams and two sets of activation buffers: even
 * steps / submits run on the context's stream with the first set, odd ones on the second stream with the second set, and the
 * partly filled last round of tiles of one forward's GEMMs runs beside the other forward's kernels.  Same kernels, same launch
 * order inside a forward: logits are bit-identical.  The second stream starts behind everything already on the context's
 * stream, and the context's stream ends behind it, so vh_synchronize, vh_last_kernel_ms and whatever the caller enqueues on
 * the context's stream afterwards see every step finished; the steps write `logits_dev` in step order.  The read-outs of "the
 * last forward" (token and layer features, vh_debug_read) read the set of the step enqueued last.  A ring's collects keep
 * their order and results.
 *   memory: the second set is as large as the first without the input staging and the logits (about 2 GB at ViT-B/16, batch
 *   512; all of it scales with max_batch).  It is allocated at the first call with steps > 1 or at vh_ring_create /
 *   vh_ring_create_u8 / vh_ring_create_tensor, never inside a stream capture.  If that allocation fails the context stays
 *   single-flight and reports no error.
 *   one forward at a time, exactly as before, while any of these holds: steps == 1; stage or step timing is on
 *   (vh_set_stage_timing, vh_set_step_timing: a duration taken beside another forward's kernels measures neither); graph replay
 *   is on; vh_set_streams(n > 1); a feature-layer or attention-layer list is set (their stores are one per context); the
 *   environment had VH_INFLIGHT=1 when the context was created (A/B runs).  The frames ring (vh_ring_create_frames) is
 *   single-flight as well: its resize writes the one resized-image buffer that the forward's first kernel reads.
 * vh_get_inflight: 2 when the next steps > 1 call or image-ring submit would run two at a time, else 1. */
int vh_forward_device_async(vh_ctx* ctx, const float* in_nhwc_dev, int batch,
                            float* logits_dev, int steps);
int vh_synchronize(vh_ctx* ctx);

/* ---- 8-bit images -------------------------------------------------------------------------------------------------
 * What a decoder, a camera or a dataloader emits: batch x image x image x channels bytes, NHWC.  CONTRACT: pixel p
 * (0..255) of channel c enters the model as the fp32 value
 *       x = fmaf((float)p, scale[c], shift[c])                       (ONE rounding)
 * computed inside the patch gather and then rounded to the MFMA operand type exactly as an fp32 input is.  The logits of
 * a u8 forward are therefore BIT-IDENTICAL to those of the fp32 entry point given the host-computed array x, on every
 * path (folded, plain, split, fp8, pre-LN, any patch size and head dim, VH_FLAG_CLS_TAIL, graphs, streams): everything
 * behind the patch matrix is the same code.  The input crosses PCIe and is read by the gather at 1 byte per element
 * instead of 4.
 *   vh_set_input_norm   scale, shift: [channels] floats each, all finite (else VH_ERR_INVALID); NULL, NULL restores the
 *                       default scale = 1/255, shift = 0; exactly one NULL is VH_ERR_INVALID.  For the usual
 *                       (p / 255 - mean) / std: scale = 1 / (255 std), shift = -mean / std.  Per-context state; the call waits
 *                       for the context's stream and drops the cached graphs (vh_set_graph), as a weight load does.
 *   vh_get_input_norm   the pair in force: [channels] floats each.
 *   vh_forward_u8, vh_forward_device_u8, vh_forward_device_u8_async: vh_forward, vh_forward_device and
 *                       vh_forward_device_async under the contract above.  A device input pointer that is not 16-byte
 *                       aligned is VH_ERR_INVALID. */
int vh_set_input_norm(vh_ctx* ctx, const float* scale, const float* shift);
int vh_get_input_norm(const vh_ctx* ctx, float* scale, float* shift);
int vh_forward_u8(vh_ctx* ctx, const uint8_t* in_nhwc_host, int batch, float* logits_host);
int vh_forward_device_u8(vh_ctx* ctx, const uint8_t* in_nhwc_dev, int batch, float* logits_dev);
int vh_forward_device_u8_async(vh_ctx* ctx, const uint8_t* in_nhwc_dev, int batch, float* logits_dev, int steps);
/* ---- Image tensors ------------------------------------------------------------------------------------------------
 * The image batch as PyTorch, ONNX, torchvision and rocJPEG hold it, taken as it is.  An image tensor is DENSE and has one
 * ELEMENT TYPE and one LAYOUT (S = image_size, C = channels):
 *       VH_ELEM_F32, VH_ELEM_F16, VH_ELEM_BF16, VH_ELEM_U8       4, 2, 2, 1 bytes per element
 *       VH_LAYOUT_NHWC  [batch][S][S][C]                          VH_LAYOUT_NCHW  [batch][C][S][S]
 * CONTRACT: element (b, y, x, c) enters the model as the fp32 value v,
 *       F32          the element itself;
 *       F16 / BF16   the element widened exactly (no rounding; infinities, signed zeros and subnormals kept);
 *       U8           fmaf((float)p, scale[c], shift[c]) with the context's vh_set_input_norm state, as on the 8-bit path;
 * and v is then rounded to the MFMA operand type exactly as an fp32 input is.  Float elements are taken as already
 * normalised: vh_set_input_norm does not touch them.  The logits are therefore BIT-IDENTICAL to vh_forward of the NHWC fp32
 * array of v, on every path (folded, plain, split, fp8, pre-LN, any patch size and head dim, VH_FLAG_CLS_TAIL, graphs,
 * streams): only the gather in front of the patch GEMM looks at the element type and the layout.  (NHWC, F32) and (NHWC, U8)
 * are vh_forward and vh_forward_u8.
 *   vh_forward_tensor, vh_forward_device_tensor, vh_forward_device_tensor_async: vh_forward, vh_forward_device and
 *                       vh_forward_device_async under the contract above.  VH_ERR_INVALID for an unknown elem or layout, a
 *                       null pointer, a batch outside 1..max_batch, or a device input pointer that is not 16-byte aligned. */
#define VH_ELEM_F32 0
#define VH_ELEM_F16 1
#define VH_ELEM_BF16 2
#define VH_ELEM_U8 3
#define VH_LAYOUT_NHWC 0
#define VH_LAYOUT_NCHW 1
int vh_forward_tensor(vh_ctx* ctx, const void* in_host, int elem, int layout, int batch, float* logits_host);
int vh_forward_device_tensor(vh_ctx* ctx, const void* in_dev, int elem, int layout, int batch, float* logits_dev);
int vh_forward_device_tensor_async(vh_ctx* ctx, const void* in_dev, int elem, int layout, int batch, float* logits_dev, int steps);
/* ---- 8-bit frames: antialiased resize + crop on the GPU in front of the u8 forward -----------------------------------
 * What a decoder or a camera emits is not image x image.  A FRAME is 8-bit interleaved pixels, height x width x channels
 * (channels = the context's), rows row_stride bytes apart, starting `offset` bytes into the buffer of the call.  A BOX
 * (x0, y0, x1, y1) = box[0..3] is given in source pixel coordinates, pixel j covering [j, j+1); it may be fractional and
 * need not be square; 0 <= x0 < x1 <= width, and the same in y.  The box is resampled to S x S, S = image_size, with the
 * antialiased triangle filter of torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False).
 * CONTRACT, per axis, with n the source length, [lo, hi) the box, scale = (hi - lo) / S, sup = max(scale, 1): output i has
 *       centre   c = lo + (i + 0.5) scale
 *       taps     j in [max(floor(c - sup + 0.5), 0), min(floor(c + sup + 0.5), n))
 *       weights  w_j = max(0, 1 - |(j + 0.5 - c) / sup|), zero weights dropped, the rest divided by their sum
 * all in double on the host, each weight then rounded ONCE to fp32 (vh_resize_table returns exactly this table).  The
 * kernel runs the horizontal pass, then the vertical pass; each accumulates in fp32 with fmaf in ascending tap order
 * starting from 0, with no rounding between the passes; the result byte is rintf(min(max(v, 0), 255)).  From there on the
 * forward IS vh_forward_u8 of that S x S x channels byte image: fmaf(p, scale[c], shift[c]) in the patch gather and
 * vh_set_input_norm apply unchanged, and the logits are BIT-IDENTICAL to feeding vh_op_resize_u8's output to the u8 entry
 * point.  Refused with VH_ERR_INVALID before anything is enqueued: width or height outside 1..8192; row_stride <
 * width * channels; scale > 32 on an axis (at most 65 taps); a box outside the frame, or empty; a frame whose last byte
 * lies beyond nbytes.  Frames of one call may all differ in size, stride and box; the descriptors are copied at the call.
 *   vh_resize_table     host only, no device: first[n_out], count[n_out], weights[n_out][max_taps] (zero padded) of one
 *                       axis; VH_ERR_INVALID for a bad box, scale > 32 or a row with more than max_taps taps.
 *   vh_forward_frames_u8, vh_forward_device_frames_u8: vh_forward_u8 / vh_forward_device_u8 of the resized boxes;
 *                       `nbytes` is the size of the frames buffer (host: copied whole; any alignment, any offsets).  The
 *                       resize runs once on the context's stream before the forward (before the fork of vh_set_streams);
 *                       stage "resize" of vh_set_stage_timing times it. */
typedef struct vh_frame {
    uint64_t offset;
    int32_t height, width, row_stride;
    float box[4];
} vh_frame;
int vh_resize_table(int n_in, double lo, double hi, int n_out, int32_t* first, int32_t* count, float* weights, int max_taps);
int vh_forward_frames_u8(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame* desc, int batch, float* logits_host);
int vh_forward_device_frames_u8(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame* desc, int batch, float* logits_dev);
/* ---- NV12 frames: colour conversion fused into the GPU resize ----------------------------------------------------------
 * What a hardware video decoder (VCN through rocDecode or VA-API) and most camera stacks emit: 12 bits per pixel in two
 * planes.  An NV12 FRAME is
 *       a Y plane    height x width bytes, rows y_stride bytes apart, at y_offset, and
 *       a UV plane   height/2 rows of width/2 interleaved (U, V) byte pairs, rows uv_stride bytes apart, at uv_offset,
 * both offsets relative to the buffer of the call.  width and height are even and within 2..8192; y_stride >= width and
 * uv_stride >= width; the last byte of each plane lies within nbytes; the planes need not be adjacent or aligned.  `box`
 * means what it means in vh_frame: LUMA pixel coordinates, fractional allowed, 0 <= x0 < x1 <= width and the same in y.  The
 * context must have channels == 3 (else VH_ERR_INVALID).
 * RESAMPLING.  Each plane is resampled to S x S under the axis contract of "8-bit frames" (the same doubles, one rounding to
 * fp32 per weight; vh_resize_table returns the luma tables): Y with n = width (height) and the box as given; UV as a
 * 2-channel image of width/2 x height/2 whose box per axis is (lo / 2 + delta, hi / 2 + delta).  VH_CHROMA_CENTER (JPEG,
 * MPEG-1): delta = 0 on both axes.  VH_CHROMA_LEFT (MPEG-2, H.264, HEVC default): delta = 0.25 horizontally, 0 vertically; the
 * chroma box may then overhang the last chroma column by up to 0.25, which the tap clamp [max(.., 0), min(.., n)) and the
 * renormalisation of the axis contract take (only this internal table relaxes hi <= n, by that quarter sample).  Each plane
 * runs the horizontal pass, then the vertical pass, each an fp32 fmaf chain in ascending tap order from 0 with nothing
 * rounded in between.
 * CONVERSION.  With the UNROUNDED fp32 y, u, v of an output pixel and a row-major 3 x 4 fp32 matrix m,
 *       out[k] = fmaf(m[4k], y, fmaf(m[4k+1], u, fmaf(m[4k+2], v, m[4k+3]))),   k = 0, 1, 2
 * and the byte is rintf(min(max(out[k], 0), 255)): ONE rounding for resize and conversion together.  From there on the
 * forward IS vh_forward_u8 of that S x S x 3 byte image: vh_set_input_norm applies unchanged and the logits are
 * BIT-IDENTICAL to feeding vh_op_resize_nv12's output to the u8 entry point.
 *   vh_yuv_matrix       host only, no device.  standard VH_YUV_BT601 (Kr 0.299, Kb 0.114), VH_YUV_BT709 (0.2126, 0.0722) or
 *                       VH_YUV_BT2020 (0.2627, 0.0593); full_range 0 or 1; anything else is VH_ERR_INVALID.  Evaluated in
 *                       double, no contraction, in exactly this order, each entry then rounded once to fp32:
 *                           kg = 1.0 - kr - kb
 *                           sy = 255.0 / 219.0, sc = 255.0 / 224.0, oy = 16.0     (full range: sy = sc = 1.0, oy = 0.0)
 *                           rv = 2.0 * (1.0 - kr) * sc
 *                           bu = 2.0 * (1.0 - kb) * sc
 *                           gu = -(2.0 * kb * (1.0 - kb) / kg) * sc
 *                           gv = -(2.0 * kr * (1.0 - kr) / kg) * sc
 *                           yo = -(sy * oy)
 *                           m  = { sy, 0.0, rv, yo - 128.0 * rv,
 *                                  sy, gu,  gv, yo - 128.0 * gu - 128.0 * gv,
 *                                  sy, bu, 0.0, yo - 128.0 * bu }                  (rows R, G, B; columns y, u, v, 1)
 *   vh_set_frame_colour m: 12 floats, all finite (else VH_ERR_INVALID), any matrix (not only vh_yuv_matrix's); chroma_site
 *                       VH_CHROMA_CENTER or VH_CHROMA_LEFT (else VH_ERR_INVALID).  m = NULL restores the default: BT.709
 *                       limited range with left siting (chroma_site is ignored then), what an HD video decoder emits.
 *                       Per-context state.  The resize runs outside the captured graph, so no graph is dropped.
 *   vh_get_frame_colour the matrix and the siting in force (either pointer may be NULL).
 *   vh_forward_frames_nv12, vh_forward_device_frames_nv12: vh_forward_frames_u8 / vh_forward_device_frames_u8 for NV12
 *                       frames.  Every descriptor and argument is checked before anything is enqueued.  Stage "resize" of
 *                       vh_set_stage_timing times this launch too. */
#define VH_CHROMA_CENTER 0
#define VH_CHROMA_LEFT 1
#define VH_YUV_BT601 0
#define VH_YUV_BT709 1
#define VH_YUV_BT2020 2
typedef struct vh_frame_nv12 {
    uint64_t y_offset, uv_offset;
    int32_t height, width, y_stride, uv_stride;
    float box[4];
} vh_frame_nv12;
int vh_yuv_matrix(int standard, int full_range, float m[12]);
int vh_set_frame_colour(vh_ctx* ctx, const float m[12], int chroma_site);
int vh_get_frame_colour(const vh_ctx* ctx, float m[12], int* chroma_site);
int vh_forward_frames_nv12(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_host);
int vh_forward_device_frames_nv12(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_dev);
/* ---- Planar YUV frames: I420 / YV12 and JPEG's 4:4:4, 4:2:2, 4:2:0, 4:4:0 planes ------------------------------------------
 * What software video decoders (ffmpeg's yuv420p, libvpx, dav1d, libde265) and JPEG decoders in raw-data mode (libjpeg-turbo,
 * TurboJPEG tjDecompressToYUVPlanes, rocJPEG) emit: three separate byte planes.  A PLANAR FRAME is
 *       a Y plane    height x width bytes, rows y_stride bytes apart, at y_offset,
 *       a U plane    ch x cw bytes, rows u_stride bytes apart, at u_offset, and
 *       a V plane    ch x cw bytes, rows v_stride bytes apart, at v_offset,
 * cw = (width + sub_x - 1) / sub_x, ch = (height + sub_y - 1) / sub_y (the JPEG and ffmpeg rule for odd sizes), all offsets
 * relative to the buffer of the call.  width and height are within 1..8192 and of ANY parity; sub_x and sub_y are 1 or 2:
 * 4:4:4 = (1, 1), 4:2:2 = (2, 1), 4:2:0 = (2, 2), 4:4:0 = (1, 2).  y_stride >= width, u_stride >= cw, v_stride >= cw; the last
 * byte of each plane lies within nbytes; the planes may lie in any order, need not be adjacent or aligned.  YV12 is I420 with
 * u_offset and v_offset exchanged: no separate mode.  `box` means what it means in vh_frame: LUMA pixel coordinates, fractional
 * allowed, 0 <= x0 < x1 <= width and the same in y.  The context must have channels == 3 (else VH_ERR_INVALID).
 * Layout: sizeof(vh_frame_yuv) == 72; y_offset 0, u_offset 8, v_offset 16, height 24, width 28, y_stride 32, u_stride 36,
 * v_stride 40, sub_x 44, sub_y 48, box 52, reserved 68 (ignored).
 * RESAMPLING.  Each plane goes through the axis contract of "8-bit frames" unchanged (the same doubles, one rounding to fp32
 * per weight): Y with n = width (height) and the box as given; U and V each as a 1-channel image of cw x ch whose box per axis
 * is (lo / sub + delta, hi / sub + delta), delta = 0.25 on the horizontal axis only when sub_x == 2 and the context's siting is
 * VH_CHROMA_LEFT, 0 otherwise.  With sub == 1 on an axis the chroma table of that axis is the luma table.  The only relaxation
 * of hi <= n is the quarter-sample overhang of left siting (even widths), as in "NV12 frames"; with centre siting and odd sizes
 * hi / 2 <= cw holds by construction.  Each plane runs the horizontal pass, then the vertical pass, each an fp32 fmaf chain in
 * ascending tap order from 0 with nothing rounded in between.
 * CONVERSION AND STATE are those of "NV12 frames", word for word: the unrounded y, u, v pass the 3 x 4 matrix with the same nested
 * fmaf expression, the byte is rintf(min(max(out[k], 0), 255)), and the matrix and the siting are the context's
 * (vh_set_frame_colour): there is no second colour state.  The default (BT.709 limited range, left siting) is the VIDEO one.  A
 * JPEG caller sets vh_yuv_matrix(VH_YUV_BT601, 1, m) with VH_CHROMA_CENTER: JFIF is full-range BT.601 with centre-sited chroma.
 * From there on the forward IS vh_forward_u8 of that S x S x 3 byte image, and the logits are BIT-IDENTICAL to feeding
 * vh_op_resize_yuv's output to the u8 entry point.  An I420 frame of even size gives the bytes vh_op_resize_nv12 gives for
 * the same planes interleaved.
 * REFUSED with VH_ERR_INVALID before a device is touched or anything is enqueued, each with a message of its own: width or
 * height outside 1..8192; sub_x or sub_y not 1 or 2; y_stride < width; u_stride < cw or v_stride < cw; a plane whose last byte
 * lies beyond nbytes; a box outside the frame, or empty; scale > 32 on an axis; channels != 3; null pointers.
 *   vh_forward_frames_yuv, vh_forward_device_frames_yuv: vh_forward_frames_nv12 / vh_forward_device_frames_nv12 for planar
 *                       frames.  Stage "resize" of vh_set_stage_timing times this launch too. */
typedef struct vh_frame_yuv {
    uint64_t y_offset, u_offset, v_offset;
    int32_t height, width;
    int32_t y_stride, u_stride, v_stride;
    int32_t sub_x, sub_y;
    float box[4];
    int32_t reserved;
} vh_frame_yuv;
int vh_forward_frames_yuv(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_host);
int vh_forward_device_frames_yuv(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_dev);
/* ---- 16-bit YUV frames: P010 / P012 / P016 and planar yuv4xxpNNle ----------------------------------------------------------
 * What a 10-bit stream decodes to.  HEVC Main10, AV1 and VP9 profile 2 come out of VCN (rocDecode, VA-API) as P010: NV12's
 * layout with 16-bit little-endian words, the code in the HIGH bits.  Software decoders (ffmpeg's yuv420p10le, yuv422p10le,
 * yuv444p12le; dav1d, libde265) emit the planar equivalent with the code in the LOW bits.  A 16-BIT FRAME is an NV12 frame
 * (vh_frame_nv12) or a planar frame (vh_frame_yuv) whose samples are 16-bit little-endian words; both descriptor structs are
 * reused unchanged:
 *       width, height, sub_x, sub_y and box count SAMPLES, as in the 8-bit layouts;
 *       every *_offset and *_stride is in BYTES and must be even;
 *       y_stride >= 2 * width; semi-planar: uv_stride >= 2 * width (a chroma row holds width / 2 pairs of 4 bytes); planar:
 *       u_stride >= 2 * cw and v_stride >= 2 * cw;
 *       the last byte of each plane lies within nbytes;
 *       a DEVICE frames pointer must be 2-byte aligned; a host pointer may have any alignment, because it is copied.
 * Parity and size rules are those of the 8-bit layout: semi-planar needs even sizes within 2..8192, planar takes any parity
 * within 1..8192.  Big-endian words are not taken; packed 4:2:2 words (Y210, Y216, v210) go to "Packed 4:2:2 frames" below; packed
 * 4:4:4 words (Y410, Y416) go to "Packed 4:4:4 frames".
 * SAMPLE VALUES.  The word enters the arithmetic AS IS, as the fp32 value of the unsigned integer 0..65535 (exact).  The kernel
 * does not shift, mask or scale: depth and alignment live in the matrix alone.  A P010 word with non-zero low bits is simply a
 * P016 value.
 * RESAMPLING and CONVERSION are those of "NV12 frames" and "Planar YUV frames", word for word: the same axis tables
 * (vh_resize_table) and the same chroma boxes and siting rule; horizontal then vertical fp32 fmaf chains in ascending tap order
 * from 0, nothing rounded in between; the same nested-fmaf matrix expression; the byte is rintf(min(max(out[k], 0), 255)).
 * The output is still an S x S x 3 BYTE image, and from there on the forward IS vh_forward_u8: the logits are BIT-IDENTICAL
 * to feeding vh_op_resize_p016's / vh_op_resize_yuv16's output to the u8 entry point.  Scaling by a power of two commutes with
 * every rounding of the chain, so a P010 frame holding (byte << 8) under the default 16-bit state gives the bytes of the NV12
 * frame under the default 8-bit state.
 * TRANSFER FUNCTIONS are not part of this: a PQ or HLG stream is converted with the linear matrix, as swscale does without a
 * tone-mapping filter.  Top-left siting (BT.2020's vertical 0.25 offset) is not offered either; VH_CHROMA_* is unchanged.
 *   vh_yuv_matrix16     host only, no device.  standard and full_range as in vh_yuv_matrix; bits 8..16; msb_aligned 0 or 1
 *                       (P010, P012 and P016: 1; yuv4xxpNNle: 0); anything else is VH_ERR_INVALID.  Evaluated in double, no
 *                       contraction, in exactly this order, each entry then rounded once to fp32 (kr, kb as in vh_yuv_matrix):
 *                           kg  = 1.0 - kr - kb
 *                           a   = msb_aligned ? 2^(16 - bits) : 1.0                   (word = code * a)
 *                           q   = 2^(bits - 8)
 *                           limited range:  sy = 255.0 / (219.0 * q * a), sc = 255.0 / (224.0 * q * a), oy = 16.0 * q * a
 *                           full range:     sy = sc = 255.0 / ((2^bits - 1.0) * a),   oy = 0.0
 *                           mid = 2^(bits - 1) * a
 *                           rv = 2.0 * (1.0 - kr) * sc
 *                           bu = 2.0 * (1.0 - kb) * sc
 *                           gu = -(2.0 * kb * (1.0 - kb) / kg) * sc
 *                           gv = -(2.0 * kr * (1.0 - kr) / kg) * sc
 *                           yo = -(sy * oy)
 *                           m  = { sy, 0.0, rv, yo - mid * rv,
 *                                  sy, gu,  gv, yo - mid * gu - mid * gv,
 *                                  sy, bu, 0.0, yo - mid * bu }
 *                       bits = 8, msb_aligned = 0 gives vh_yuv_matrix bit for bit; the limited-range bits = 10, msb_aligned = 1
 *                       matrix is the 8-bit one with its first three columns multiplied by 2^-8, bit for bit.
 *   vh_set_frame_colour16, vh_get_frame_colour16: a SECOND colour state, for the 16-bit entry points alone, under the rules of
 *                       vh_set_frame_colour (one frames ring interleaves 8-bit and 16-bit submits, so one matrix cannot serve
 *                       both).  Default, and what m = NULL restores: BT.709 limited range, 10 bits, MSB-aligned, left siting:
 *                       P010 as VCN writes it.  The two states do not touch each other.
 *   vh_forward_frames_p016, vh_forward_device_frames_p016: vh_forward_frames_nv12 / vh_forward_device_frames_nv12 for
 *                       semi-planar 16-bit frames (P010, P012, P016), the same argument list.
 *   vh_forward_frames_yuv16, vh_forward_device_frames_yuv16: vh_forward_frames_yuv / vh_forward_device_frames_yuv for planar
 *                       16-bit frames.  Stage "resize" of vh_set_stage_timing times these launches too; the resize runs before
 *                       the fork of vh_set_streams and outside the captured graph.
 * REFUSED with VH_ERR_INVALID before a device is touched or anything is enqueued, each with a message of its own: an odd offset;
 * an odd stride; a stride below the byte widths above; a plane whose last byte lies beyond nbytes; an odd device frames pointer;
 * and every refusal of the 8-bit twin (sizes, sub_x / sub_y, box, scale > 32, channels != 3, null pointers). */
int vh_yuv_matrix16(int standard, int full_range, int bits, int msb_aligned, float m[12]);
int vh_set_frame_colour16(vh_ctx* ctx, const float m[12], int chroma_site);
int vh_get_frame_colour16(const vh_ctx* ctx, float m[12], int* chroma_site);
int vh_forward_frames_p016(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_host);
int vh_forward_device_frames_p016(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_nv12* desc, int batch, float* logits_dev);
int vh_forward_frames_yuv16(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_host);
int vh_forward_device_frames_yuv16(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuv* desc, int batch, float* logits_dev);
/* ---- Packed 4:2:2 frames: YUY2 / UYVY, Y210 / Y216 and v210 ---------------------------------------------------------------------
 * What cameras and capture cards deliver: UVC webcams and V4L2 write YUYV (YUY2); HDMI / SDI capture cards (DeckLink, AJA,
 * Magewell) and AVFoundation write UYVY (2vuy) in 8 bit and v210 in 10 bit; D3D / VA-API surfaces and ffmpeg's y210le are Y210 /
 * Y216.  A PACKED FRAME is ONE plane of macropixels at `offset`, rows row_stride bytes apart; all formats share vh_frame_yuy2.
 * MACROPIXEL.  A row is cw = (width + 1) / 2 macropixels of two luma samples and one (U, V) pair.  width and height count luma
 * SAMPLES, are within 1..8192 and of ANY parity; an odd width leaves the second luma of the last macropixel unread (it must still
 * lie within the row and within nbytes).  `box` means what it means in vh_frame_yuv: luma pixel coordinates.  The context must have
 * channels == 3.  Layout: sizeof(vh_frame_yuy2) == 40; offset 0, height 8, width 12, row_stride 16, layout 20, box 24.
 * 8-BIT ENTRY POINTS (_yuy2).  A macropixel is 4 bytes in the order of `layout`: VH_422_YUYV = Y0 U Y1 V, VH_422_UYVY = U Y0 V Y1,
 * VH_422_YVYU = Y0 V Y1 U, VH_422_VYUY = V Y0 U Y1.  row_stride >= 4 * cw.  Base, offset and stride may have any alignment.  The
 * matrix and the siting are those of vh_set_frame_colour.  VH_422_V210 is refused.
 * 16-BIT ENTRY POINTS (_y210), layouts 0..3.  A macropixel is four little-endian 16-bit words in the order of `layout`: Y210 / Y212 /
 * Y216 with VH_422_YUYV.  row_stride >= 8 * cw; offset and row_stride must be even and a DEVICE frames pointer 2-byte aligned (a
 * host pointer may have any alignment, because it is copied).  The word enters the arithmetic AS IS, as in P016 ("16-bit YUV
 * frames", SAMPLE VALUES).  The matrix and the siting are those of vh_set_frame_colour16, whose default, 10 bits MSB-aligned, is
 * Y210 as drivers write it.
 * VH_422_V210 (16-bit entry points only).  A row is ceil(width / 6) blocks of four little-endian 32-bit words.  The twelve 10-bit
 * codes of a block sit in bits 0-9, 10-19 and 20-29 of the successive words, in the order
 *       U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5;
 * bits 30-31 are ignored.  row_stride >= 16 * ceil(width / 6); offset and row_stride must be multiples of 4 and a device frames
 * pointer 4-byte aligned.  A code enters the arithmetic as the fp32 value code * 64 (exact): the Y210 / P010 word of that code.  A
 * v210 frame and the Y210 frame of the same codes therefore share the colour state and give the SAME BYTES.
 * EVERYTHING ELSE is "Planar YUV frames" / "16-bit YUV frames" with sub_x = 2, sub_y = 1, word for word: the luma box as given, the
 * chroma box (lo / 2 + delta, hi / 2 + delta) with delta = 0.25 under VH_CHROMA_LEFT and the quarter-sample overhang that goes with
 * it, the axis tables (vh_resize_table), horizontal then vertical fp32 fmaf chains in ascending tap order from 0 with nothing rounded
 * in between, the nested-fmaf matrix expression and the one rounding rintf(min(max(out[k], 0), 255)).  EQUIVALENCE: the output bytes
 * are those of vh_op_resize_yuv (vh_op_resize_yuv16) on the de-interleaved planes (Y height x width, U and V height x cw, sub_x = 2,
 * sub_y = 1), BIT FOR BIT, and the logits are BIT-IDENTICAL to vh_forward_u8 of vh_op_resize_yuy2's (vh_op_resize_y210's) output.
 * Packed 4:4:4 (AYUV, Y410, v410) goes to "Packed 4:4:4 frames" below; 4:1:1 and big-endian words are not taken.
 * REFUSED with VH_ERR_INVALID before a device is touched or anything is enqueued, each with a message of its own: width or height
 * outside 1..8192; a layout that is none of VH_422_*, or VH_422_V210 on the 8-bit entry points; row_stride below the widths above;
 * an offset, a stride or a device frames pointer that is odd (16-bit words) or no multiple of 4 (v210); a frame whose last byte
 * lies beyond nbytes; a box outside the frame, or empty; scale > 32 on an axis; channels != 3; null pointers.
 *   vh_forward_frames_yuy2, vh_forward_device_frames_yuy2: vh_forward_frames_yuv / vh_forward_device_frames_yuv for 8-bit packed
 *                       frames, the same argument list with vh_frame_yuy2 descriptors.
 *   vh_forward_frames_y210, vh_forward_device_frames_y210: vh_forward_frames_yuv16 / vh_forward_device_frames_yuv16 for Y210 /
 *                       Y216 / v210 frames.  Stage "resize" of vh_set_stage_timing times these launches too. */
#define VH_422_YUYV 0   /* Y0 U Y1 V   (YUY2, V4L2 YUYV)            */
#define VH_422_UYVY 1   /* U Y0 V Y1   (UYVY, 2vuy, HDYC)           */
#define VH_422_YVYU 2   /* Y0 V Y1 U                                */
#define VH_422_VYUY 3   /* V Y0 U Y1                                */
#define VH_422_V210 4   /* 10-bit, three codes per 32-bit word; 16-bit entry points only */
typedef struct vh_frame_yuy2 {
    uint64_t offset;
    int32_t height, width, row_stride;   /* samples, samples, bytes */
    int32_t layout;                      /* VH_422_*               */
    float box[4];
} vh_frame_yuy2;
int vh_forward_frames_yuy2(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_host);
int vh_forward_device_frames_yuy2(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_dev);
int vh_forward_frames_y210(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_host);
int vh_forward_device_frames_y210(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuy2* desc, int batch, float* logits_dev);
/* ---- Packed 4:4:4 frames: BGR / BGRA / RGBA / ARGB, YUV24 / AYUV and Y410 / Y416 ------------------------------------------------------
 * What most callers hold: OpenCV's Mat is BGR, screen and window capture, GPU colour converters and VA-API / D3D / AMF RGB surfaces
 * are BGRA / RGBA / ARGB; 4:4:4 HEVC / AV1 decode surfaces, screen-content codecs and SDI 4:4:4 capture are AYUV, Y410, v410 and Y416.
 * A PACKED 4:4:4 FRAME is ONE plane of pixels at `offset`, rows row_stride bytes apart; all formats share vh_frame_bgra.  width and
 * height count PIXELS, are within 1..8192 and of ANY parity; `box` is in pixel coordinates as in vh_frame.  The context must have
 * channels == 3.  Layout: sizeof(vh_frame_bgra) == 40; offset 0, height 8, width 12, row_stride 16, layout 20, box 24.
 * LAYOUT WORD.  VH_444(p0, p1, p2, four, yuv) = p0 | p1 << 2 | p2 << 4 | (four ? 64 : 0) | (yuv ? 128 : 0): p_k is the index (0..3)
 * within the pixel of the sample that becomes output component k (R, G, B; with `yuv`: Y, U, V); `four`: the pixel has four samples,
 * else three; `yuv`: the three samples pass the colour matrix.  Any such word is taken, named or not; the named ones carry the MEMORY
 * ORDER in the name.  The 4th sample (A or X) is never read as data.  Bits 8 and 9 belong to the two 10-bit layouts alone.
 * 8-BIT ENTRY POINTS (_bgra).  A pixel is 3 or 4 bytes: VH_444_RGB, _BGR; _RGBA, _BGRA, _ARGB, _ABGR (RGBX, BGRX, XRGB, XBGR are the
 * same layouts); VH_444_YUV24 = Y U V (V4L2 YUV24); VH_444_VUYA = V U Y A (Microsoft's AYUV FourCC, ffmpeg vuya / vuyx); VH_444_AYUV =
 * A Y U V (ffmpeg ayuv).  Row bytes R = 3 * width or 4 * width; row_stride >= R.  Base, offset and stride may have any alignment.
 * YUV layouts use the matrix of vh_set_frame_colour.
 * 16-BIT ENTRY POINTS (_y410), YUV only.  VH_444_Y416 = U Y V A (Y416 / Y412, XV36) and VH_444_AYUV64 = A Y U V (ffmpeg ayuv64le):
 * four little-endian 16-bit words per pixel, R = 8 * width; offset and row_stride must be even and a DEVICE frames pointer 2-byte
 * aligned (a host pointer may have any alignment, because it is copied).  The word enters the arithmetic AS IS ("16-bit YUV frames",
 * SAMPLE VALUES).  A layout word names positions, not a width: VH_444_Y416 on the _bgra entry points is the 8-bit pixel U Y V A.
 * VH_444_Y410 (ffmpeg xv30le) and VH_444_V410: ONE little-endian 32-bit word per pixel, R = 4 * width; Y410 holds U in bits 0-9, Y in
 * 10-19, V in 20-29 and ignores bits 30-31; V410 holds U in bits 2-11, Y in 12-21, V in 22-31 and ignores bits 0-1.  offset and
 * row_stride must be multiples of 4 and a device frames pointer 4-byte aligned.  A 10-bit code enters the arithmetic as the fp32 value
 * code * 64 (exact), as a v210 code does: the Y416 / P010 word of that code.  The matrix is that of vh_set_frame_colour16, whose
 * default, 10 bits MSB-aligned, is Y410 under this rule.
 * SPAN.  The frame's span is (height - 1) * row_stride + R <= nbytes - offset, and no load touches a byte outside it.
 * RESAMPLING.  All three components use the ONE table pair (x, y) of the box: the axis contract's tables (vh_resize_table).  The
 * horizontal pass runs first, then the vertical pass, each an fp32 fmaf chain in ascending tap order from 0, nothing rounded in
 * between.  Chroma siting has no effect: nothing is sub-sampled.  YUV layouts: the unrounded y, u, v pass the nested-fmaf 3 x 4 matrix
 * of "NV12 frames" and the byte is rintf(min(max(out[k], 0), 255)).  RGB layouts: no matrix and no colour state; the byte of output
 * channel k is rintf(min(max(v_k, 0), 255)) of the resampled sample p_k.
 * EQUIVALENCES, BIT FOR BIT.  An RGB layout gives the bytes of vh_op_resize_u8 (channels 3) on the frame with its pixels rewritten
 * as tight R G B.  A YUV layout gives the bytes of vh_op_resize_yuv (vh_op_resize_yuv16) on the de-interleaved planes with sub_x =
 * sub_y = 1 and the same matrix.  A Y410 and a V410 frame give the bytes of the Y416 frame holding code << 6.  The logits are
 * BIT-IDENTICAL to vh_forward_u8 of vh_op_resize_bgra's (vh_op_resize_y410's) output.
 * NOT TAKEN: RGB words of 10 / 16 bits (x2rgb10, rgb48, rgba64), big-endian words, alpha blending (A is skipped, not applied).
 * REFUSED with VH_ERR_INVALID before a device is touched or anything is enqueued, each with a message of its own; per descriptor
 * the checks run in this order: width or height outside 1..8192; a layout with bits outside the defined ones; a position 3 in a
 * three-sample pixel; a 10-bit layout on the _bgra entry points; on the _y410 entry points a 10-bit layout that is neither
 * VH_444_Y410 nor VH_444_V410, or a word layout without `yuv` or without `four`; row_stride < R; an offset, a stride or a device
 * frames pointer (each separately) that is odd (16-bit words) or no multiple of 4 (Y410 / V410); a frame whose span ends beyond
 * nbytes; a box outside the frame, or empty; scale > 32 on an axis.  Ahead of the descriptors: null pointers, a bad batch, channels
 * != 3.
 *   vh_forward_frames_bgra, vh_forward_device_frames_bgra: vh_forward_frames_yuy2 / vh_forward_device_frames_yuy2 for 8-bit packed
 *                       4:4:4 frames, the same argument list with vh_frame_bgra descriptors.
 *   vh_forward_frames_y410, vh_forward_device_frames_y410: vh_forward_frames_y210 / vh_forward_device_frames_y210 for Y416 /
 *                       AYUV64 / Y410 / V410 frames.  Stage "resize" of vh_set_stage_timing times these launches too. */
#define VH_444(p0, p1, p2, four, yuv) ((p0) | (p1) << 2 | (p2) << 4 | ((four) ? 64 : 0) | ((yuv) ? 128 : 0))
#define VH_444_RGB VH_444(0, 1, 2, 0, 0)      /* R G B                                   */
#define VH_444_BGR VH_444(2, 1, 0, 0, 0)      /* B G R        (OpenCV)                   */
#define VH_444_RGBA VH_444(0, 1, 2, 1, 0)     /* R G B A      (RGBX)                     */
#define VH_444_BGRA VH_444(2, 1, 0, 1, 0)     /* B G R A      (BGRX; D3D, GDI, VA-API)   */
#define VH_444_ARGB VH_444(1, 2, 3, 1, 0)     /* A R G B      (XRGB)                     */
#define VH_444_ABGR VH_444(3, 2, 1, 1, 0)     /* A B G R      (XBGR)                     */
#define VH_444_YUV24 VH_444(0, 1, 2, 0, 1)    /* Y U V        (V4L2 YUV24)               */
#define VH_444_VUYA VH_444(2, 1, 0, 1, 1)     /* V U Y A      (the AYUV FourCC; vuya, vuyx) */
#define VH_444_AYUV VH_444(1, 2, 3, 1, 1)     /* A Y U V      (ffmpeg ayuv)              */
#define VH_444_Y416 VH_444(1, 0, 2, 1, 1)     /* U Y V A, 16-bit words (Y416, Y412, XV36); _y410 entry points */
#define VH_444_AYUV64 VH_444(1, 2, 3, 1, 1)   /* A Y U V, 16-bit words (ayuv64le);         _y410 entry points */
#define VH_444_Y410 (VH_444(1, 0, 2, 1, 1) | 256)         /* one 32-bit word: U 0-9, Y 10-19, V 20-29; _y410 entry points */
#define VH_444_V410 (VH_444(1, 0, 2, 1, 1) | 256 | 512)   /* one 32-bit word: U 2-11, Y 12-21, V 22-31; _y410 entry points */
typedef struct vh_frame_bgra {
    uint64_t offset;
    int32_t height, width, row_stride;   /* pixels, pixels, bytes */
    int32_t layout;                      /* VH_444_*             */
    float box[4];
} vh_frame_bgra;
int vh_forward_frames_bgra(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_host);
int vh_forward_device_frames_bgra(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_dev);
int vh_forward_frames_y410(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_host);
int vh_forward_device_frames_y410(vh_ctx* ctx, const uint8_t* frames_dev, size_t nbytes, const vh_frame_bgra* desc, int batch, float* logits_dev);
/* uniform[-1,1) synthetic images written straight into HBM (value range of the reference,
 * def/defines.h:11-12) */
int vh_fill_input_seeded(vh_ctx* ctx, uint64_t seed, int batch, float* in_nhwc_dev);

/* ---- pipelined host path ------------------------------------------------------------------------------------
 * A ring of in-flight batches, modelled on the reference's only asynchronous pattern: the 24-slot ring of
 * filter_image / get_filtered_image (netFPGA.cpp:292-365, ring state :47-56).  vh_ring_submit enqueues
 * H2D copy -> forward -> D2H copy of one batch into the next free slot and returns at once; vh_ring_collect waits
 * for the OLDEST submitted batch and copies its logits out (FIFO).  Copies run on their own streams from pinned
 * staging buffers, so the upload of batch i+1 and the download of batch i-1 overlap the forward of batch i and the
 * host-pointer rate approaches the device-resident rate.  Full ring / empty ring are returned as
 * VH_ERR_RING_FULL / VH_ERR_RING_EMPTY (the reference prints and drops the frame, :330-333, :358-361).
 *   vh_ring_input gives the pinned staging buffer of the slot the next submit will use: fill it in place and
 *   submit with in_nhwc_host = NULL to skip the extra host copy.
 *   Consecutive submits of the image rings (this one, _u8, _tensor) run two at a time on two compute streams and two buffer
 *   sets ("TWO FORWARDS IN FLIGHT" at vh_forward_device_async: memory, fall-backs, VH_INFLIGHT); collect order and results
 *   are unchanged.  The frames ring runs one forward at a time. */
int vh_ring_create(vh_ctx* ctx, int slots, int batch_per_slot);
int vh_ring_destroy(vh_ctx* ctx);
int vh_ring_free_slots(const vh_ctx* ctx, int* n);
int vh_ring_input(vh_ctx* ctx, float** pinned_in_nhwc);
int vh_ring_submit(vh_ctx* ctx, const float* in_nhwc_host, int batch);
int vh_ring_collect(vh_ctx* ctx, float* logits_host, int* batch);
/* The same ring with slots that stage 8-bit images (a quarter of the pinned and of the device memory, a quarter of the
 * bytes per upload).  Each pixel enters as fmaf((float)p, scale[c], shift[c]) (vh_set_input_norm; one rounding), so a
 * collected batch has the bits vh_forward_u8 / vh_forward of that fp32 array return.  vh_ring_collect,
 * vh_ring_free_slots and vh_ring_destroy serve both kinds of ring; a context has one ring at a time.  The input calls
 * are per kind: vh_ring_input / vh_ring_submit on a u8 ring, and vh_ring_input_u8 / vh_ring_submit_u8 on an fp32 ring,
 * return VH_ERR_STATE. */
int vh_ring_create_u8(vh_ctx* ctx, int slots, int batch_per_slot);
int vh_ring_input_u8(vh_ctx* ctx, uint8_t** pinned_in_nhwc);
int vh_ring_submit_u8(vh_ctx* ctx, const uint8_t* in_nhwc_host, int batch);
/* The same ring with slots that stage FRAMES ("8-bit frames" above): each slot holds slot_bytes of pinned and of device
 * memory for the frames of one submit, any sizes.  vh_ring_input_frames: the pinned buffer the next submit uploads and
 * its capacity (= slot_bytes).  vh_ring_submit_frames: frames_host NULL (or the slot's own buffer) = filled in place;
 * nbytes <= slot_bytes; the descriptors are checked and copied before anything is enqueued, and a refused submit leaves
 * the ring as it was.  A collected batch has the bits vh_forward_frames_u8 returns.  vh_ring_collect, vh_ring_free_slots
 * and vh_ring_destroy serve this kind too; the input and submit calls of the other kinds return VH_ERR_STATE on a
 * frames ring, and the frames calls return VH_ERR_STATE on the other kinds. */
int vh_ring_create_frames(vh_ctx* ctx, int slots, int batch_per_slot, size_t slot_bytes);
int vh_ring_input_frames(vh_ctx* ctx, uint8_t** pinned, size_t* capacity);
int vh_ring_submit_frames(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame* desc, int batch);
/* NV12 frames ("NV12 frames" above) on the SAME frames ring: a slot is raw bytes, so one ring takes vh_ring_submit_frames and
 * vh_ring_submit_frames_nv12 interleaved; vh_ring_input_frames and vh_ring_collect are unchanged.  The context must have
 * channels == 3.  Checked and copied before anything is enqueued; a refused submit leaves the ring as it was; VH_ERR_STATE on
 * the other kinds of ring.  A collected batch has the bits vh_forward_frames_nv12 returns. */
int vh_ring_submit_frames_nv12(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch);
/* Planar YUV frames ("Planar YUV frames" above) on the SAME frames ring: RGB, NV12 and planar submits interleave on one ring.
 * The context must have channels == 3.  Checked and copied before anything is enqueued; a refused submit leaves the ring as it
 * was; VH_ERR_STATE on the other kinds of ring.  A collected batch has the bits vh_forward_frames_yuv returns. */
int vh_ring_submit_frames_yuv(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch);
/* 16-bit YUV frames ("16-bit YUV frames" above) on the SAME frames ring: RGB, NV12, planar, P016 and planar 16-bit submits
 * interleave on one ring; the 16-bit ones use the second colour state.  The same rules: checked and copied before anything is
 * enqueued; a refused submit leaves the ring as it was; VH_ERR_STATE on the other kinds of ring.  A collected batch has the
 * bits vh_forward_frames_p016 / vh_forward_frames_yuv16 returns. */
int vh_ring_submit_frames_p016(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_nv12* desc, int batch);
int vh_ring_submit_frames_yuv16(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuv* desc, int batch);
/* Packed 4:2:2 frames ("Packed 4:2:2 frames" above) on the SAME frames ring, interleaved with every other kind of submit; _yuy2
 * uses the first colour state, _y210 (Y210 / Y216 / v210) the second.  The same rules: checked and copied before anything is
 * enqueued; a refused submit leaves the ring as it was; VH_ERR_STATE on the other kinds of ring.  A collected batch has the
 * bits vh_forward_frames_yuy2 / vh_forward_frames_y210 returns. */
int vh_ring_submit_frames_yuy2(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch);
int vh_ring_submit_frames_y210(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_yuy2* desc, int batch);
/* Packed 4:4:4 frames ("Packed 4:4:4 frames" above) on the SAME frames ring, interleaved with every other kind of submit; _bgra
 * uses the first colour state (YUV layouts; RGB layouts use none), _y410 (Y416 / AYUV64 / Y410 / V410) the second.  The same rules:
 * checked and copied before anything is enqueued; a refused submit leaves the ring as it was; VH_ERR_STATE on the other kinds
 * of ring.  A collected batch has the bits vh_forward_frames_bgra / vh_forward_frames_y410 returns. */
int vh_ring_submit_frames_bgra(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch);
int vh_ring_submit_frames_y410(vh_ctx* ctx, const uint8_t* frames_host, size_t nbytes, const vh_frame_bgra* desc, int batch);
/* The same ring with slots that stage IMAGE TENSORS ("Image tensors" above) of ONE element type and layout, fixed when the ring
 * is created: a slot holds batch_per_slot * S * S * C * sizeof(element) bytes of pinned and of device memory.
 * vh_ring_input_tensor: the pinned buffer the next submit uploads and its capacity in bytes.  vh_ring_submit_tensor: in_host
 * NULL (or the slot's own buffer) = filled in place.  A collected batch has the bits vh_forward_tensor returns.
 * vh_ring_collect, vh_ring_free_slots and vh_ring_destroy serve this kind too; the input and submit calls of the other three
 * kinds return VH_ERR_STATE on a tensor ring, and the tensor calls return VH_ERR_STATE on the other kinds. */
int vh_ring_create_tensor(vh_ctx* ctx, int slots, int batch_per_slot, int elem, int layout);
int vh_ring_input_tensor(vh_ctx* ctx, void** pinned, size_t* capacity_bytes);
int vh_ring_submit_tensor(vh_ctx* ctx, const void* in_host, int batch);

/* hipGraph replay.  With enable != 0 the launch sequence of a forward is captured once per (input pointer, logits
 * pointer, batch) and replayed with hipGraphLaunch; the first forward at a given batch size still runs eagerly.
 * Results are bit-identical.  This is for small batches, which are launch-bound (ViT-B/16, batch 1: ~100 launches);
 * at batch 512 it changes nothing.  Stage timing (vh_set_stage_timing) bypasses the graph.  Environment default:
 * VH_GRAPH=1.  Counterpart in the reference: none (one clEnqueueTask per forward, netFPGA.cpp:275). */
int vh_set_graph(vh_ctx* ctx, int enable);
int vh_get_graph(const vh_ctx* ctx, int* enabled, int* cached_graphs);

/* Concurrency inside one forward: the batch is split into `n` contiguous parts (1..4, default 1, environment
 * VH_STREAMS) that are enqueued on separate streams and joined at the end of every forward.  Images are
 * independent, so the logits are bit-identical for every n; with n = 2 the HBM-bound stages and the partly
 * filled last tile round of one half overlap the MFMA-bound stages of the other (+5 % images/s at ViT-B b512).
 * Off by default: two kernels then share the device, so a per-launch duration no longer measures one kernel. */
int vh_set_streams(vh_ctx* ctx, int n);
int vh_get_streams(const vh_ctx* ctx, int* n);
int vh_get_inflight(const vh_ctx* ctx, int* n);

/* observability: replaces forward_performance / get_forward_performance
 * (netFPGA.cpp:262-264,280-284,603-611).  us = host wall time of the last vh_forward*,
 * kernel_ms = device time between hip events around the last forward's kernels. */
int vh_last_forward_us(const vh_ctx* ctx, int64_t* us);
int vh_last_kernel_ms(vh_ctx* ctx, double* ms);
/* device time of ONE launch of the dominant GEMM kernel class, averaged over the launches
 * of the last forward (hip events on the context's stream); used for bench.py's roofline */
int vh_profile_forward(vh_ctx* ctx, const float* in_nhwc_dev, int batch, float* logits_dev,
                       double* stage_ms, int n_stage_slots, int* n_stages_written);
const char* vh_stage_name(int stage_index);
/* Time every launch of ONE stage (index as in vh_stage_name; -1 = off; the last index, "resize", is the resize launch of
 * the frames entry points, which vh_profile_forward -- an fp32 forward -- never runs and does not report) with hip events on the
 * context's stream during the following vh_forward_device_async calls, then read the average /
 * minimum launch duration and the number of launches measured. */
int vh_set_stage_timing(vh_ctx* ctx, int stage_index);
int vh_get_stage_timing(vh_ctx* ctx, double* avg_ms, double* min_ms, int* launches);
/* Per-STEP device times of the last vh_forward_device_async call: with step timing enabled the call records one hip
 * event at every step boundary (K + 1 for K steps, on the context's stream); vh_get_step_timing synchronises and writes
 * the first min(*steps, max_steps) step durations in ms (bench.py: median and min beside the mean). */
int vh_set_step_timing(vh_ctx* ctx, int enable);
int vh_get_step_timing(vh_ctx* ctx, double* step_ms, int max_steps, int* steps);

/* debug taps: copy an internal activation of the LAST forward to the host as fp32.
 * what: 0 = residual stream x [batch*T, D] after the last layer run,
 *       1 = the head's input [batch, W]: the final-LN'd CLS rows (W = D), or what the context's VH_FLAG_POOL mode computes
 *           (W = D; 2 D for VH_POOL_CLS_AVG), or the attention-pooling block's result u of a VH_FLAG_MAP_HEAD context (W = D),
 *       (2 is unused: VH_ERR_INVALID, like any other value not listed here,)
 *       3 = one float: 1 when the last forward kept the MLP hidden activation in its tiled (16-row-blocked) layout -- the
 *           default wherever both MLP GEMMs take the persistent form (16-bit folded path, whole 256-row tiles; VH_H_TILED=0 at
 *           context creation keeps it row-major): same values, same logit bits, fc1's result leaves the registers without an
 *           LDS transposition,
 *       4 = one float: 1 when the last forward kept q|k|v head-major ([3][heads][rows][64]) between the projection's epilogue
 *           and the attention kernel (default where the attention output is tiled; VH_QKV_HM=0 keeps [rows][3 D]; same bits). */
int vh_debug_read(vh_ctx* ctx, int what, float* host_out, size_t n_floats);
/* run only the first `n_layers` encoder layers on the next forwards (-1 = all) */
int vh_debug_set_layers(vh_ctx* ctx, int n_layers);

/* ---- Token features ----------------------------------------------------------------------
 * What a feature backbone returns (DINOv2's x_norm_clstoken / x_norm_patchtokens, the linear probe's concat(cls, mean of
 * the patch tokens), a CLIP tower's pre-projection vector and its raw penultimate-layer rows): the residual stream the LAST
 * forward enqueued on the context left in HBM, written on the GPU into the caller's buffers, in the caller's element
 * type, through the model's final LayerNorm or as it is.  A PULL interface: the calls read the state a forward left, and no
 * forward entry point knows of them.
 *
 *   cls    [batch][D]        the class-token row of every image
 *   patch  [batch][NP][D]    the patch rows, NP = (image_size / patch_size)^2 = tokens - 1 - R (R register tokens: rows 1 .. R of
 *                            an image are skipped, VH_FLAG_REGISTERS)
 *   mean   [batch][D]        the mean of an image's patch rows
 * D = vh_config.dim, tokens = NP + 1 + R, batch = the last forward's (vh_features_dims).  A NULL pointer:
 * that output is not wanted and nothing is written for it.
 *
 * WHICH FORWARD.  The last one enqueued on the context through any entry point (fp32, 8-bit, tensor, any frames format; eager or
 * graph replay; 1..4 streams); after vh_forward_device_async(.., steps) the last step.  A weight load on a context whose LayerNorm
 * fold is guarded (the default flags) runs one calibration image, which counts as a forward of batch 1, as it does for
 * vh_debug_read.  With vh_debug_set_layers(n) the features are those after n layers: one layer at a time that is DINOv2's
 * get_intermediate_layers(norm=True), and with VH_FEAT_RAW the penultimate-layer rows CLIP consumers take.  The calls read the
 * context's arena and write the caller's buffers (vh_read_features stages through activation scratch that every forward
 * rewrites before it reads it): logits, guards, cached graphs and a following forward are unaffected, and calling twice gives
 * the same bits.
 *
 * ARITHMETIC, for bits.  x[r][k] = the residual element vh_debug_read(ctx, 0) returns: the fp32 element, or on the split paths
 * (float)hi + lo with ONE fp32 add (16-bit hi + the decoded lo byte; VH_DTYPE_FP8: e4m3 + bf16).
 *   VH_FEAT_RAW    v = x.
 *   VH_FEAT_NORM   fp32, two passes: mean = sum(x) / D, var = sum((x - mean)^2) / D, rstd = 1 / sqrtf(var + ln_eps),
 *                  v = fmaf((x - mean) * rstd, gamma[k], beta[k]) with the final LayerNorm's gamma / beta.  The order of the two
 *                  row sums depends on D alone: never on the batch, the row, the element type or the outputs requested.
 *   patch[b][p]    v of row b * tokens + 1 + R + p.
 *   cls[b]         RAW: v of row b * tokens.  NORM: the vector the head multiplied (vh_debug_read(ctx, 1)), so that head(cls)
 *                  reproduces the logits.
 *   mean[b][k]     (((0 + v[b,1+R,k]) + v[b,2+R,k]) + ... + v[b,NP+R,k]) * inv: plain fp32 adds over the NP patch rows ascending, of the
 *                  UNROUNDED fp32 v, inv = (float)(1.0 / NP).
 *   elem           a 16-bit output is the round-to-nearest-even of exactly the fp32 value VH_ELEM_F32 would have written.
 * Image i's outputs never depend on the other images or on the batch size.
 *
 * REFUSED, each with a message of its own, nothing enqueued and no output touched.  VH_ERR_INVALID: a null context or
 * descriptor; all three pointers NULL; elem not VH_ELEM_F32 / F16 / BF16; norm not 0 or 1; a device output pointer that is
 * not 16-byte aligned.  VH_ERR_STATE: no forward has run; a ring exists on the context (its forwards belong to slots).
 * VH_ERR_UNSUPPORTED: a VH_FLAG_CLS_TAIL context (its last layer does not update the other rows).
 *
 * POOLED AND CLASS-TOKEN-FREE CONTEXTS (VH_FLAG_POOL, VH_FLAG_NO_CLS).  On a VH_FLAG_NO_CLS context tokens = NP + R, patch[b][p] <- row
 * b * tokens + R + p, mean over those rows, reg <- rows 0 .. R - 1; a non-NULL cls is refused (VH_ERR_UNSUPPORTED, nothing enqueued).
 * On a pooled context WITH a class token cls stays LN(row 0) (RAW: row 0): the head's input no longer is that vector, so the
 * feature kernels compute it with the arithmetic above.
 *
 *   vh_features_dims               any of the four may be NULL; *batch = 0 before the first forward; *tokens = NP + 1 + R, or NP + R
 *                                  on a VH_FLAG_NO_CLS context; *patches = NP
 *   vh_read_features               host buffers; synchronous
 *   vh_read_features_device        device buffers; enqueues on the context's stream and waits
 *   vh_read_features_device_async  device buffers; enqueues only (vh_synchronize, or stream order with a following call) */
#define VH_FEAT_NORM 0   /* rows pass the model's final LayerNorm (lnf gamma/beta, cfg.ln_eps) */
#define VH_FEAT_RAW  1   /* the residual stream as it is                                      */
typedef struct vh_features {       /* sizeof == 32: cls 0, patch 8, mean 16, elem 24, norm 28 */
    void* cls;     /* [batch][D]        or NULL: not wanted */
    void* patch;   /* [batch][NP][D]    or NULL             */
    void* mean;    /* [batch][D]        or NULL             */
    int32_t elem;  /* VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16 */
    int32_t norm;  /* VH_FEAT_NORM or VH_FEAT_RAW              */
} vh_features;
int vh_features_dims(const vh_ctx* ctx, int* batch, int* tokens, int* patches, int* dim);
int vh_read_features(vh_ctx* ctx, const vh_features* out_host);
int vh_read_features_device(vh_ctx* ctx, const vh_features* out_dev);
int vh_read_features_device_async(vh_ctx* ctx, const vh_features* out_dev);

/* ---- Layer features ------------------------------------------------------------------------
 * What a dense head takes from a backbone (DINOv2's get_intermediate_layers(x, n, reshape=True, return_class_token=True) in front
 * of its DPT and linear heads, ViT-Adapter / Mask2Former-style decoders, a LLaVA-style consumer of layer -2): the residual stream
 * after SEVERAL layers of ONE forward, each read out like the token features, the patch rows optionally channels-first, and the
 * register rows.  Capture is a push -- the forward copies rows it has finished -- and the read-out is the pull interface above.
 *
 * THE LIST.  vh_set_feature_layers(ctx, layers, n): n <= VH_MAX_FEATURE_LAYERS entries, strictly ascending, each 1 .. cfg.layers;
 * entry k = the residual stream after k layers (Hugging Face's hidden_states[k]).  n == 0 clears the list and frees the store.  The
 * call waits for the context's stream, drops the cached graphs and allocates ONE capture store for the listed layers below
 * cfg.layers: max_batch x tokens x dim elements per such layer, of 3 bytes where the context keeps the residual as two planes for
 * good (folded LayerNorm with VH_FLAG_LN_FOLD_ON: 16-bit hi + one lo byte, VH_DTYPE_FP8: e4m3 hi + bf16 lo) and of 4 bytes
 * everywhere else -- the fp32 residual, and every context whose guarded fold may still fall back to it (the default flags): the
 * size is decided once, for the widest form.  ViT-B/16 at max_batch 512: 232 MB (3 bytes) / 310 MB (4 bytes) per layer.  When the
 * allocation fails the call returns VH_ERR_HIP and the previous list stays in force.  vh_get_feature_layers reads the list back
 * (layers: room for VH_MAX_FEATURE_LAYERS ints, or NULL).
 *
 * CAPTURE.  Every forward enqueued while a list is set copies, behind the second MLP GEMM of layer k - 1 for every listed k below
 * the number of layers it runs, the real rows of its batch into the store in the form its path holds them (both planes, or the
 * fp32 array): one small launch per listed layer, on the stream of the batch part, captured into graphs like every other launch,
 * inside the profile event of the stage that follows.  A listed layer equal to the number of layers run is served from the live
 * residual and costs nothing.  With an empty list a forward enqueues exactly what it enqueued before this section existed; with
 * any list the logits keep their bits.
 *
 * READ-OUT.  vh_layer_features = vh_features + reg, layer and patch_layout:
 *   layer         -1 or cfg.layers: the final state -- the values and bits of vh_read_features, the NORM class-token rows being the
 *                 vector the head multiplied.  1 .. cfg.layers - 1: that layer of the LAST forward; it must have been in the list when
 *                 that forward was enqueued, and the forward must have reached it (vh_debug_set_layers).  Its NORM class-token
 *                 row is v of row b * tokens like any other row.
 *   reg           [batch][R][D]: v of rows b * tokens + 1 .. b * tokens + R (DINOv2's x_norm_regtokens), R = vh_get_register_tokens.
 *   patch_layout  VH_FEAT_ROWS: patch is [batch][NP][D].  VH_FEAT_NCHW: [batch][D][gh][gw], gh = gw = image_size / patch_size,
 *                 out[b][k][p] = rows[b][p][k] (DINOv2's reshape=True): bit for bit the elements of the VH_FEAT_ROWS output,
 *                 transposed.  Only the base pointer needs the 16-byte alignment.
 * ARITHMETIC: exactly "Token features" -- x = hi + lo with one fp32 add, the two-pass fp32 LayerNorm whose sum order depends on D
 * alone, with the model's FINAL LayerNorm parameters for every layer (DINOv2's norm=True), the serial fp32 mean chain over the NP
 * patch rows, 16-bit outputs = the RNE of the fp32 ones.  A captured layer has the bits vh_read_features gives after
 * vh_debug_set_layers(k) and a forward of the same images.  Image i's outputs never depend on the other images.
 *
 * REFUSED, each with a message of its own, nothing enqueued and no output touched.  VH_ERR_INVALID: a null context or descriptor;
 * all four pointers NULL; elem, norm or patch_layout outside their values; layer outside -1, 1 .. cfg.layers; a device pointer
 * that is not 16-byte aligned; reg on a context without register tokens.  VH_ERR_STATE: no forward has run; a ring exists; the
 * layer was not in the list when the last forward was enqueued; the last forward did not reach the layer.  VH_ERR_UNSUPPORTED: a
 * VH_FLAG_CLS_TAIL context (vh_set_feature_layers too).  vh_set_feature_layers: VH_ERR_INVALID for a null context, a bad count or
 * a list that is not strictly ascending within 1 .. cfg.layers; VH_ERR_STATE while a ring exists.
 * Not covered: rings, device groups, layer 0 (the embedding output). */
#define VH_MAX_FEATURE_LAYERS 8
#define VH_FEAT_ROWS 0   /* patch [batch][NP][D]                                  */
#define VH_FEAT_NCHW 1   /* patch [batch][D][gh][gw]: the same elements, transposed */
typedef struct vh_layer_features { /* sizeof == 48: cls 0, patch 8, mean 16, reg 24, elem 32, norm 36, layer 40, patch_layout 44 */
    void* cls;            /* [batch][D]      or NULL: not wanted */
    void* patch;          /* [batch][NP][D] / [batch][D][gh][gw] or NULL */
    void* mean;           /* [batch][D]      or NULL             */
    void* reg;            /* [batch][R][D]   or NULL             */
    int32_t elem;         /* VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16 */
    int32_t norm;         /* VH_FEAT_NORM or VH_FEAT_RAW              */
    int32_t layer;        /* -1 / cfg.layers: the final state; 1 .. cfg.layers - 1: a listed layer */
    int32_t patch_layout; /* VH_FEAT_ROWS or VH_FEAT_NCHW             */
} vh_layer_features;
int vh_set_feature_layers(vh_ctx* ctx, const int* layers, int n);
int vh_get_feature_layers(const vh_ctx* ctx, int* layers, int* n);
int vh_read_layer_features(vh_ctx* ctx, const vh_layer_features* out_host);
int vh_read_layer_features_device(vh_ctx* ctx, const vh_layer_features* out_dev);
int vh_read_layer_features_device_async(vh_ctx* ctx, const vh_layer_features* out_dev);

/* ---- Attention maps --------------------------------------------------------------------------
 * Where the model looked: the softmax rows of the class token (DINO's get_last_selfattention, class-attention token pruning) and of
 * the register tokens, per head, for SEVERAL layers of ONE forward -- Hugging Face's attentions[k - 1][:, :, :Q, :].  The attention
 * kernels keep their probabilities on chip; a listed layer runs one more small kernel behind its q|k|v projection that computes
 * these rows on their own.  Capture is a push, the read-out a pull, as with "Layer features".
 *
 * THE LIST.  vh_set_attention_layers(ctx, layers, n, queries): n <= VH_MAX_ATTENTION_LAYERS entries, strictly ascending, each
 * 1 .. cfg.layers; entry k = the attention of the k-th encoder layer.  queries: VH_ATTN_Q_CLS = row 0 only (Q = 1; refused on a
 * VH_FLAG_NO_CLS context), VH_ATTN_Q_LEAD = every leading row, the class token and the registers (Q = 1 + R, or R without a class
 * token; refused where there is none).  n == 0 clears the list and frees the store.  The call waits for the context's stream,
 * drops the cached graphs and allocates ONE store [n][max_batch][heads][Q][tokens] of fp32 in 256-byte aligned slots: ViT-B/16 at
 * max_batch 512, Q = 1: 4.8 MB per layer.  When the allocation fails the call returns VH_ERR_HIP and the previous list stays in
 * force.  vh_get_attention_layers reads the list back (layers: room for VH_MAX_ATTENTION_LAYERS ints, or NULL; queries may be NULL).
 *
 * CAPTURE.  Every forward enqueued while a list is set runs, behind the q|k|v projection of every listed layer it reaches, one
 * launch per batch part on that part's stream, captured into graphs like every other launch, inside the profile event of the
 * attention stage.  It reads the q rows of the Q queries and the K third of q|k|v once, in the layout the part holds them.  With an
 * empty list a forward enqueues exactly what it enqueued before this section existed; with any list the logits keep their bits.
 *
 * ARITHMETIC, for bits.  q arrives scaled by head_dim^-1/2 * log2(e), so everything is in the exp2 domain.  For query r, key t of
 * one (image, head):
 *   s[t] = the fp32 dot product q_r . k_t: per 8-column chunk an fmaf chain in ascending column order from 0, the chunks added by an
 *          xor butterfly (1, 2, 4, 8) over the next power of two of head_dim / 8 lanes, absent chunks being 0 -- a function of
 *          head_dim alone;
 *   m = max_t s[t];  e[t] = exp2(s[t] - m) by v_exp_f32, arguments below -126 as exp2(x + 64) * 2^-64 (denormals are kept);
 *   l = sum_t e[t]: lane i of 64 adds t = i, i + 64, ... in ascending order from 0, then the xor butterfly 32, 16, .., 1 -- a function
 *          of tokens alone;
 *   p[t] = e[t] / l, the IEEE fp32 division.
 * An image's map therefore has the same bits whatever the batch, the batch part and stream, the q|k|v layout, eager or graph replay.
 *
 * READ-OUT.  vh_attention_maps, of the LAST forward; B = its batch (vh_attention_dims), H = cfg.heads:
 *   probs      [B][H][Q][K] or NULL;  head_mean [B][Q][K] or NULL: (((0 + p[h=0]) + p[1]) + ... + p[H-1]) * (float)(1.0 / H), plain fp32
 *              adds of the unrounded values in ascending head order (the serial-chain convention of the token features' mean).
 *   elem       VH_ELEM_F32, or VH_ELEM_F16 / VH_ELEM_BF16 = the round-to-nearest-even of exactly the fp32 value.
 *   layer      -1 = cfg.layers, or 1 .. cfg.layers: it must have been in the list when the last forward was enqueued, and that
 *              forward must have reached it (vh_debug_set_layers).
 *   keys       VH_ATTN_KEYS_ALL: K = tokens.  VH_ATTN_KEYS_PATCH: K = NP, key columns lead .. tokens - 1 (lead = the leading rows), so
 *              probs is [B][H][Q][gh][gw] as it lies (DINO's attentions[:, :, 0, 1:] reshaped).  The values are NOT renormalised.
 * vh_read_attention writes host buffers (staged through activation scratch) and waits; _device enqueues on the context's stream and
 * waits; _device_async only enqueues.  Device pointers are 16-byte aligned.
 *
 * REFUSED, each with a message of its own, nothing enqueued and no output touched.  VH_ERR_INVALID: a null context or descriptor;
 * both pointers NULL; elem, keys or layer outside their values; reserved != 0; a device pointer that is not 16-byte aligned.
 * VH_ERR_UNSUPPORTED: a VH_FLAG_CLS_TAIL context, whose last layer runs another attention kernel (vh_set_attention_layers too).
 * VH_ERR_STATE: a ring exists; no forward has run; the layer was not in the list when the last forward was enqueued; the last
 * forward did not reach it.  vh_set_attention_layers: VH_ERR_INVALID for a null context, a bad count, a list that is not strictly
 * ascending within 1 .. cfg.layers, a queries value that is neither constant or that the context has no rows for; VH_ERR_STATE
 * while a ring exists.
 * Not covered: all-query maps [tokens][tokens] (attention rollout), rings, device groups. */
#define VH_MAX_ATTENTION_LAYERS 64
#define VH_ATTN_Q_CLS 0      /* the class token's row                                      */
#define VH_ATTN_Q_LEAD 1     /* every leading row: the class token and the register tokens */
#define VH_ATTN_KEYS_ALL 0   /* all `tokens` key columns                                   */
#define VH_ATTN_KEYS_PATCH 1 /* the NP patch columns                                       */
typedef struct vh_attention_maps { /* sizeof == 32: probs 0, head_mean 8, elem 16, layer 20, keys 24, reserved 28 */
    void* probs;          /* [batch][heads][Q][K] or NULL: not wanted */
    void* head_mean;      /* [batch][Q][K]        or NULL             */
    int32_t elem;         /* VH_ELEM_F32, VH_ELEM_F16 or VH_ELEM_BF16 */
    int32_t layer;        /* -1 / cfg.layers: the last layer; 1 .. cfg.layers: a listed layer */
    int32_t keys;         /* VH_ATTN_KEYS_ALL or VH_ATTN_KEYS_PATCH   */
    int32_t reserved;     /* 0 */
} vh_attention_maps;
int vh_set_attention_layers(vh_ctx* ctx, const int* layers, int n, int queries);
int vh_get_attention_layers(const vh_ctx* ctx, int* layers, int* n, int* queries);
/* any of the five may be NULL; *batch = 0 before the first forward; *queries = the Q of the list in force (0: none);
 * *tokens = all key columns, *patches = NP */
int vh_attention_dims(const vh_ctx* ctx, int* batch, int* heads, int* queries, int* tokens, int* patches);
int vh_read_attention(vh_ctx* ctx, const vh_attention_maps* out_host);
int vh_read_attention_device(vh_ctx* ctx, const vh_attention_maps* out_dev);
int vh_read_attention_device_async(vh_ctx* ctx, const vh_attention_maps* out_dev);

/* ---- operator-level entry points (device pointers, dtype = VH_DTYPE_*) ----------------- */
/* Each is the kernel the forward uses, exposed so that parity tests and micro-benchmarks
 * can drive it alone.  `stream` is a hipStream_t passed as void* (NULL = default stream);
 * the call returns after the kernel has completed. */
#define VH_EPI_BIAS 0        /* out16[m,n]  = acc + bias[n]                               */
#define VH_EPI_BIAS_GELU 1   /* out16[m,n]  = gelu(acc + bias[n])                          */
#define VH_EPI_BIAS_RESID 2  /* out32[m,n] += acc + bias[n]        (fp32 residual stream)  */
#define VH_EPI_BIAS_F32 3    /* out32[m,n]  = acc + bias[n]                                */
#define VH_EPI_PATCH 4       /* out32[row(m),n] = acc + bias[n] + pos[tok(m),n]            */
#define VH_EPI_LNFOLD 5      /* out16[m,n]  = rstd[m]*(acc - mean[m]*c[n]) + d[n]   (LayerNorm folded: bias = d, aux = c) */
#define VH_EPI_LNFOLD_GELU 6 /* gelu of the above                                          */
#define VH_EPI_RESID_LN 7    /* out32 += acc + bias; out16 = 16-bit copy; partials[N/64][M][2] = row (sum, sumsq) */
#define VH_EPI_RESID_SPLIT 8 /* residual kept as TWO planes, x = hi + lo: (hi, lo) += acc + bias with hi = T(x) (16 bit) and lo = what that
                                rounding dropped, ONE byte per element: e4m3((x - hi) * 32) for bf16, * 256 for fp16 (12 / 15
                                significant bits of x in the pair).  out = hi plane (the next GEMM's A operand), out16 = lo plane
                                [M,N] bytes, partials as RESID_LN.  3 B per element each way instead of 4 B + the 2 B copy of RESID_LN */
#define VH_EPI_PATCH_SPLIT 9 /* the patch embedding written directly as the split residual: row(m) of (hi, lo) = the planes of
                                acc + bias + pos[tok(m)], plus that row's partial sums (partials[N/64][R][2], R = token rows) --
                                EPI_PATCH and the first row-statistics pass in one epilogue.  out = hi, out16 = lo, aux /
                                aux_i as EPI_PATCH; the class-token rows are not touched (vh_op_gemm_ex: R = images x tokens) */
#define VH_EPI_BIAS_QGELU 10   /* out16[m,n] = qgelu(acc + bias[n]),  qgelu(v) = v * sigmoid(1.702 v); accepted wherever
                                  VH_EPI_BIAS_GELU is, with the same shape rules                                           */
#define VH_EPI_LNFOLD_QGELU 11 /* qgelu of VH_EPI_LNFOLD; accepted wherever VH_EPI_LNFOLD_GELU is                          */
/* (12 is no code: the taps keep refusing it, as the refusal tests expect) */
#define VH_EPI_BIAS_TGELU 13   /* out16[m,n] = tgelu(acc + bias[n]),  tgelu(v) = 0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3)));
                                  accepted wherever VH_EPI_BIAS_GELU is, with the same shape rules                         */
#define VH_EPI_LNFOLD_TGELU 14 /* tgelu of VH_EPI_LNFOLD; accepted wherever VH_EPI_LNFOLD_GELU is                          */
/* out = epilogue(A[M,K] * W[N,K]^T); A and W hold `dtype` elements, K contiguous.
 * aux: EPI_PATCH -> pos-emb fp32 [tokens, N] with aux_i = patches per image.
 * variant: 0 = auto, 1 = 128x128 tile, 2 = 256x256 two-stage, 5 = 256x256 ping-pong, 6 = persistent ping-pong. */
int vh_op_gemm(const void* a16_dev, const void* w16_dev, const float* bias_dev, void* out_dev,
               int64_t M, int N, int K, int epilogue, const float* aux_dev, int aux_i,
               int dtype, int variant, void* stream);

/* fp8 GEMM (VH_DTYPE_FP8 path): a8 [M,K], w8 [N,K] OCP e4m3 bytes, w_scale [N] fp32 (per output channel),
 * out = epilogue(w_scale[n] * sum_k a8[m,k] w8[n,k] + bias[n]);  VH_EPI_BIAS -> bf16, VH_EPI_BIAS_GELU -> e4m3
 * (saturating), VH_EPI_BIAS_RESID (out += ...) / VH_EPI_BIAS_F32 -> fp32.  K % 128 == 0, N % 4 == 0. */
int vh_op_gemm_fp8(const void* a8, const void* w8, const float* w_scale, const float* bias, void* out, int64_t M,
                   int N, int K, int epilogue, int variant /* 0 auto, 5, 7 */, void* stream);
/* the same kernel with the epilogues of the folded-LayerNorm layer loop of the fp8 path (operator tests):
 *   VH_EPI_LNFOLD / VH_EPI_LNFOLD_GELU  out (bf16 / e4m3) = [gelu](rstd[m] * (w_scale[n] * acc - mean[m] * c[n]) + bias[n]);
 *                                       c_dev [N], stats_dev [M][2] = (mean, rstd); N % 256 == 0 for the GELU form
 *   VH_EPI_RESID_LN     out fp32 [M,N] += w_scale * acc + bias; out16 = its e4m3 copy; partials [N/64][M][2]
 *   VH_EPI_RESID_SPLIT  the residual kept as an e4m3 plane (out: hi = e4m3(x), the next GEMM's operand) and a bf16 plane
 *                       (out16: lo = bf16(x - hi)): (hi, lo) += w_scale * acc + bias; partials as above.  N % 256 == 0 */
int vh_op_gemm_fp8_ex(const void* a8, const void* w8, const float* w_scale, const float* bias, void* out, int64_t M,
                      int N, int K, int epilogue, const float* c_dev, const float* stats_dev, void* out16,
                      float* partials, int variant, void* stream);
/* the load-time weight quantiser: s0 = amax(row)/448 (1 for an all-zero row), w8 = rne_e4m3(w / s0),
 * scale[row] = s0 * post_scale */
int vh_op_quantize_rows(const float* w, int rows, int cols, float post_scale, void* w8, float* scale, void* stream);

/* same with the operands of the LayerNorm-folding epilogues: stats [M][2] = (mean, rstd) for LNFOLD*,
 * out16 [M,N] and partials [N/64][M][2] for RESID_LN / RESID_SPLIT (N must be a multiple of 256) */
int vh_op_gemm_ex(const void* a16_dev, const void* w16_dev, const float* bias_dev, void* out_dev,
                  int64_t M, int N, int K, int epilogue, const float* aux_dev, int aux_i,
                  const float* stats_dev, void* out16_dev, float* partials_dev,
                  int dtype, int variant, void* stream);
/* Test and measurement taps: the forms of the GEMM that only a whole forward reaches otherwise (tests/gemm_exact.py).
 * vh_op_gemm_layout is vh_op_gemm_ex, vh_op_gemm_fp8_layout is vh_op_gemm_fp8_ex (which here takes the epilogues of vh_op_gemm_fp8 as
 * well: c_dev / stats_dev / out16 / partials may be NULL where the epilogue does not use them), plus
 *   out_tiled != 0   activation epilogues (*_GELU, *_QGELU, *_TGELU): the result in the 16-row-blocked layout of the MLP hidden activation,
 *                    [M / 16][N / 8][16 rows][8 values] (e4m3 results: [M / 16][N / 16][16 rows][16 B]);
 *                    VH_EPI_LNFOLD and 16-bit VH_EPI_BIAS: the result head-major, [N / 64][M][64] (the q|k|v projection)
 *   ab_tiled != 0    A and W are both read from the 16-row-blocked layout ([rows / 16][K / 8][16][8]; e4m3: [rows / 16][K / 16][16][16 B]):
 *                    VH_EPI_RESID_SPLIT, and VH_EPI_BIAS with 16-bit operands
 *   tile_begin, tile_count   launch only tiles [tile_begin, tile_begin + tile_count) of the 256 x 256 tiles in n-fastest order,
 *                    tile t = (t / tiles_n, t % tiles_n), tiles_n = ceil(N / 256); tile_count == 0 (with tile_begin == 0) = all tiles
 * With all four 0 they are the calls they extend.  VH_ERR_INVALID, with a message and before a device is touched, for anything
 * the launchers refuse: a tiled flag needs variant 6, M and N multiples of 256, at least two K-tiles (four with an LN-fold epilogue,
 * except the e4m3-operand activation forms; a K-tile is 64 16-bit or 128 e4m3 elements), one of the epilogues named above, and
 * excludes the other flag and a tile range; a tile range needs variant 5 or 7, tile_begin >= 0, tile_count >= 0,
 * tile_begin + tile_count <= tiles, and tile_count > 0 where tile_begin != 0. */
int vh_op_gemm_layout(const void* a16_dev, const void* w16_dev, const float* bias_dev, void* out_dev,
                      int64_t M, int N, int K, int epilogue, const float* aux_dev, int aux_i,
                      const float* stats_dev, void* out16_dev, float* partials_dev, int dtype, int variant,
                      int out_tiled, int ab_tiled, int tile_begin, int tile_count, void* stream);
/* Test taps of the register-token assembly (VH_FLAG_REGISTERS; every vh_op_gemm* tap above keeps lead = 1).
 *   vh_op_gemm_lead  the VH_EPI_PATCH / VH_EPI_PATCH_SPLIT epilogues with `lead` = 1 + R rows in front of an image's patch rows:
 *                    GEMM row m = img * aux_i + p lands on output row m + img * lead + lead and adds pos row 1 + p (aux_dev
 *                    [(aux_i + 1)][N]).  M a whole number of images, 1 <= lead <= 17; out_dev (and out16_dev) hold
 *                    (M / aux_i) * (aux_i + lead) rows; PATCH_SPLIT: partials_dev [N/64][prow][2], prow = 0 for that row count.
 *   vh_op_lead_rows  the kernels that write the `lead` leading rows of every image: row 0 = cls + pos[0], row 1 + r = reg[r].
 *                    lo_dev NULL: fp32 rows x_or_hi_dev [batch * tokens][dim] (partials_dev, prow, dtype unused); otherwise the
 *                    split planes (hi 16-bit of `dtype`, lo one scaled e4m3 byte) and the rows' per-64-column (sum, sum of
 *                    squares) in partials_dev [dim/64][prow][2], prow >= batch * tokens.  dim % 64 == 0, lead < tokens.
 *                    cls_dev and pos_dev both NULL: the form of a VH_FLAG_NO_CLS context, whose `lead` rows (1 .. 16) are all
 *                    register rows, row r = reg[r].  (vh_op_gemm_lead takes lead = 0 .. 17: with no row in front of the patch rows
 *                    such a context hands the epilogue its [NP][D] position table one row early.) */
int vh_op_gemm_lead(const void* a16_dev, const void* w16_dev, const float* bias_dev, void* out_dev, int64_t M, int N, int K,
                    int epilogue, const float* aux_dev, int aux_i, int lead, void* out16_dev, float* partials_dev, int64_t prow,
                    int dtype, int variant, void* stream);
int vh_op_lead_rows(void* x_or_hi_dev, void* lo_dev, float* partials_dev, int64_t prow, const float* cls_dev, const float* pos_dev,
                    const float* reg_dev, int lead, int batch, int tokens, int dim, int dtype, void* stream);
int vh_op_gemm_fp8_layout(const void* a8, const void* w8, const float* w_scale, const float* bias, void* out, int64_t M,
                          int N, int K, int epilogue, const float* c_dev, const float* stats_dev, void* out16,
                          float* partials, int variant, int out_tiled, int ab_tiled, int tile_begin, int tile_count,
                          void* stream);
/* Test tap: the kernels that put a weight matrix into the 16-row-blocked layout ab_tiled reads, on their own.
 * dtype VH_DTYPE_BF16 / VH_DTYPE_FP16: in = fp32 [rows, cols] -> out = `dtype` [rows / 16][cols / 8][16][8] (round to nearest even);
 * dtype VH_DTYPE_FP8: in = bytes [rows, cols] -> out = the same bytes [rows / 16][cols / 16][16][16].
 * rows % 16 == 0 and cols % 8 == 0 (bytes: cols % 16 == 0), else VH_ERR_INVALID. */
int vh_op_tile_rows(const void* in_dev, int rows, int cols, void* out_dev, int dtype, void* stream);
/* row statistics helpers of the folded LayerNorm:
 *   vh_op_rowstats_cast: x fp32 [rows, dim] -> x16 [rows, dim] (plain cast) and stats [rows][2] = (mean, rstd)
 *   vh_op_finalize_stats: partials [nblk][rows][2] (sum, sumsq over 64-column blocks) -> stats [rows][2] */
int vh_op_rowstats_cast(const float* x_dev, int64_t rows, int dim, float eps, void* x16_dev, float* stats_dev,
                        int dtype, void* stream);
int vh_op_finalize_stats(const float* partials_dev, int nblk, int64_t rows, int dim, float eps, float* stats_dev,
                         void* stream);
/* x fp32 [rows, dim] -> the two planes of the split residual (hi = T(x), 16 bit; lo = one scaled e4m3 byte per element, see
 * VH_EPI_RESID_SPLIT) and stats [rows][2] */
int vh_op_rowstats_split(const float* x_dev, int64_t rows, int dim, float eps, void* hi_dev, void* lo_dev, float* stats_dev,
                         int dtype, void* stream);
/* W'[n,k] = dtype(scale * gamma[k] * W[n,k]); c[n] = sum_k W'[n,k]; d[n] = scale * (sum_k beta[k] W[n,k] + b[n]) */
int vh_op_fold_ln(const float* w_dev, const float* b_dev, const float* gamma_dev, const float* beta_dev, int rows,
                  int dim, float scale, void* w16_dev, float* c_dev, float* d_dev, int dtype, void* stream);
/* y16[r,:] = LN(x[r*row_stride : +dim]) * gamma + beta */
int vh_op_layernorm(const float* x_dev, int64_t rows, int dim, int64_t row_stride,
                    const float* gamma_dev, const float* beta_dev, float eps, void* out16_dev,
                    int dtype, void* stream);
/* The pre-LayerNorm of VH_FLAG_PRE_LN contexts on its own: y = LN(x[r, :]) * gamma + beta in fp32 for x fp32 [rows, dim]
 * (dim % 4 == 0, dim <= 2048), written in the forms the forward's paths consume; each output pointer may be NULL, one of
 * y32 / hi must be given, x may alias y32:
 *   y32_dev   fp32 [rows, dim]                      the fp32 residual stream
 *   hi_dev    `dtype` [rows, dim]                   T(y): the 16-bit (VH_DTYPE_FP8: e4m3) plane / operand copy
 *   lo_dev    bytes [rows, dim] (VH_DTYPE_FP8: bf16) what that rounding dropped, as VH_EPI_RESID_SPLIT keeps it (needs hi_dev)
 *   stats_dev [rows][2]                             (mean, rstd) of the NORMALISED row y: layer 0's LN1 statistics */
int vh_op_pre_layernorm(const float* x_dev, int64_t rows, int dim, const float* gamma_dev, const float* beta_dev, float eps,
                        float* y32_dev, void* hi_dev, void* lo_dev, float* stats_dev, int dtype, void* stream);
/* ---- Test taps of the row kernels (tests/rows_exact.py, tests/test_gpu_rows_exact.py).  Every tap checks pointers, shape and
 * dtype on the host and returns VH_ERR_INVALID before anything is launched; dim % 4 == 0 and dim <= 2048 wherever a row is kept
 * in registers; a dtype other than the ones named is VH_ERR_INVALID (vh_op_layernorm, vh_op_rowstats_cast / _split: VH_DTYPE_BF16,
 * VH_DTYPE_FP16, VH_DTYPE_FP8; vh_op_fold_ln: the two 16-bit types).  They synchronise the stream like their neighbours.
 * Guard words: one unsigned 32-bit word on the device that holds the bits of a non-negative float, raised by an atomic maximum
 * over the first guard_rows rows (0 <= guard_rows <= rows; the rows behind them are tile padding and never count); a NaN's
 * bits rank above +Inf's.  A word keeps a value that is already larger.
 *   vh_op_rowstats_guard        vh_op_rowstats_cast (lo_dev NULL) / vh_op_rowstats_split with the guard: amax_guard_dev
 *                               (VH_DTYPE_FP8 only, may be NULL) = max |x| of the guarded rows.  VH_DTYPE_FP8: hi = e4m3 bytes,
 *                               lo = bf16 of the remainder.
 *   vh_op_pre_layernorm_guard   vh_op_pre_layernorm with guard_dev = max |ymean| * yrstd of the normalised guarded rows and
 *                               amax_guard_dev (VH_DTYPE_FP8 only) = max |y|; both may be NULL; they need hi_dev or stats_dev.
 *   vh_op_finalize_stats_guard  vh_op_finalize_stats with guard_dev = max |mean| * rstd and amax_guard_dev = max over the
 *                               guarded rows of sqrt(the largest block's sum of squares); both may be NULL.
 *   vh_op_ln_guard              guard_dev = max(guard_dev, max_r |stats[r][0]| * stats[r][1]) over stats [rows][2].
 *   vh_op_layernorm_f32         vh_op_layernorm with the fp32 result out32 [rows, dim] (the final LayerNorm of the plain path).
 *   vh_op_layernorm_split       out32[r, :] = LN(hi[r * row_stride + k] + lo[r * row_stride + k]) * gamma + beta for the split
 *                               residual's planes: dtype VH_DTYPE_BF16 / VH_DTYPE_FP16 = 16-bit hi + one scaled e4m3 byte,
 *                               VH_DTYPE_FP8 = e4m3 hi + bf16 lo; row_stride >= dim, in elements.
 *   vh_op_head_f32              logits[b, c] = sum_k y[b, k] * w[c, k] + bias[c], all fp32; classes % 4 == 0, dim % 16 == 0.
 *   vh_op_fold_ln_f8            vh_op_fold_ln for e4m3 weights: w8 [rows, dim] bytes = e4m3(scale * gamma o W / s0), wscale[n] = s0
 *                               = amax / 448 (1 for an all-zero row), c[n] = s0 * sum_k decode(w8[n, k]), d as vh_op_fold_ln.
 *   vh_op_fake_quant_rows       out[r, :] = decode(e4m3(w[r, :] / s0)) * s0 with the same row quantiser; cols % 4 == 0. */
int vh_op_rowstats_guard(const float* x_dev, int64_t rows, int dim, float eps, void* hi_dev, void* lo_dev, float* stats_dev,
                         int dtype, int64_t guard_rows, unsigned int* amax_guard_dev, void* stream);
int vh_op_pre_layernorm_guard(const float* x_dev, int64_t rows, int dim, const float* gamma_dev, const float* beta_dev, float eps,
                              float* y32_dev, void* hi_dev, void* lo_dev, float* stats_dev, int dtype, int64_t guard_rows,
                              unsigned int* guard_dev, unsigned int* amax_guard_dev, void* stream);
int vh_op_finalize_stats_guard(const float* partials_dev, int nblk, int64_t rows, int dim, float eps, float* stats_dev,
                               int64_t guard_rows, unsigned int* guard_dev, unsigned int* amax_guard_dev, void* stream);
int vh_op_ln_guard(const float* stats_dev, int64_t rows, unsigned int* guard_dev, void* stream);
int vh_op_layernorm_f32(const float* x_dev, int64_t rows, int dim, int64_t row_stride, const float* gamma_dev,
                        const float* beta_dev, float eps, float* out32_dev, void* stream);
int vh_op_layernorm_split(const void* hi_dev, const void* lo_dev, int64_t rows, int dim, int64_t row_stride,
                          const float* gamma_dev, const float* beta_dev, float eps, float* out32_dev, int dtype, void* stream);
int vh_op_head_f32(const float* y_dev, const float* w_dev, const float* bias_dev, float* out_dev, int batch, int classes,
                   int dim, void* stream);
int vh_op_fold_ln_f8(const float* w_dev, const float* b_dev, const float* gamma_dev, const float* beta_dev, int rows, int dim,
                     float scale, void* w8_dev, float* wscale_dev, float* c_dev, float* d_dev, void* stream);
int vh_op_fake_quant_rows(const float* w_dev, int rows, int cols, float* out_dev, void* stream);
/* qkv16 [batch*tokens, 3*heads*64] -> out16 [batch*tokens, heads*64].  The q columns arrive pre-scaled by
 * VH_ATTN_Q_SCALE = 64^-1/2 * log2(e) (the forward folds it into Wq/bq): the kernel's softmax works in the exp2 domain. */
#define VH_ATTN_Q_SCALE 0.18033688011112042f
int vh_op_attention(const void* qkv16_dev, int batch, int tokens, int heads, void* out16_dev,
                    int dtype, void* stream);
/* The K/V-streaming attention kernel on its own: the same operation as vh_op_attention, for any tokens in 1..4097 and
 * heads <= 32 (vh_op_attention uses it itself above 640 tokens, where a head's K and V no longer fit in LDS; this tap
 * runs it at every token count).  dtype VH_DTYPE_FP8: bf16 q|k|v in, e4m3 out [batch*tokens, heads*64]. */
int vh_op_attention_stream(const void* qkv16_dev, int batch, int tokens, int heads, void* out16_dev,
                           int dtype, void* stream);
/* Attention at head dims 32, 48, ..., 128 (the kernel the forward runs for every head dim other than 64; this tap runs it
 * at 64 as well): qkv16 [batch*tokens, 3*heads*head_dim] -> out16 [batch*tokens, heads*head_dim], q pre-scaled by
 * head_dim^-1/2 * log2(e), tokens 1..4097, heads*head_dim <= 2048.  dtype VH_DTYPE_FP8: bf16 q|k|v in, e4m3 out. */
int vh_op_attention_hd(const void* qkv16_dev, int batch, int tokens, int heads, int head_dim, void* out16_dev,
                       int dtype, void* stream);
/* Test tap: the one-query attention kernel of VH_FLAG_CLS_TAIL on its own.  qkv16 [batch*tokens, 3*heads*64] (q pre-scaled as
 * above) -> out16 [batch, heads*64]: attention of every image's row 0 over all its keys / values.  tokens 1..1024, dtype
 * VH_DTYPE_BF16 or VH_DTYPE_FP16; anything else is VH_ERR_INVALID. */
int vh_op_attention_cls(const void* qkv16_dev, int batch, int tokens, int heads, void* out16_dev,
                        int dtype, void* stream);
/* Test tap: vh_op_attention with the two layouts the forward uses between the projections:
 *   out_tiled != 0   the result in the 16-row-blocked layout [rows / 16][heads*64 / 8][16 rows][8 values] (VH_DTYPE_FP8: e4m3,
 *                    [rows / 16][heads*64 / 16][16 rows][16 B]); out16 holds batch*tokens rounded up to 16 rows, and the rows
 *                    beyond batch*tokens are not written.  Ring forms with an even head count only.
 *   in_hm_rows != 0  q|k|v arrives head-major, [3][heads][in_hm_rows][64] with in_hm_rows >= batch*tokens (needs out_tiled).
 * With both 0 it is vh_op_attention.  VH_ERR_INVALID wherever the launch would refuse: the tiled output at a shape that does not
 * run a ring form or with an odd head count, head-major input without the tiled output, in_hm_rows < batch*tokens. */
int vh_op_attention_layout(const void* qkv16_dev, int batch, int tokens, int heads, void* out16_dev,
                           int dtype, int out_tiled, int64_t in_hm_rows, void* stream);
/* The capture kernel of "Attention maps" on its own: the softmax rows of the first `queries` (1..17, <= tokens) rows of every image
 * -> probs_f32 [batch][heads][queries][tokens], by the arithmetic stated there.  qkv16 is row-major [batch*tokens, 3*heads*head_dim]
 * (in_hm_rows == 0; head_dim 32, 48, ..., 128) or head-major [3][heads][in_hm_rows][64] (head_dim 64, in_hm_rows >= batch*tokens), q
 * pre-scaled by head_dim^-1/2 * log2(e); tokens 1..4097, heads*head_dim <= 2048, dtype VH_DTYPE_BF16 or VH_DTYPE_FP16, both pointers
 * 16-byte aligned.  Nothing outside [b][h][r][0 .. tokens) is written.  Every other argument is VH_ERR_INVALID, with a message of its
 * own, before a device is touched. */
int vh_op_attention_probs(const void* qkv16_dev, int batch, int tokens, int heads, int head_dim, int queries, int64_t in_hm_rows,
                          int dtype, float* probs_f32_dev, void* stream);
/* The read-out kernel of "Attention maps" on its own: store_f32 [batch][heads][queries][tokens] -> probs_out [batch][heads][queries][K]
 * and / or head_mean_out [batch][queries][K] (either may be NULL, not both) in `elem`; keys VH_ATTN_KEYS_ALL: K = tokens,
 * VH_ATTN_KEYS_PATCH: K = tokens - lead, columns lead .. tokens - 1 (lead 0 .. tokens-1).  Pointers 16-byte aligned. */
int vh_op_attention_readout(const float* store_f32_dev, int batch, int heads, int queries, int tokens, int lead, int elem, int keys,
                            void* probs_out_dev, void* head_mean_out_dev, void* stream);
/* NHWC fp32 images -> patch matrix [batch*np, patch*patch*channels] in `dtype` */
int vh_op_im2col(const float* in_nhwc_dev, int batch, int image, int patch, int channels,
                 void* out16_dev, int dtype, void* stream);
/* The same for any patch and channel count: patch matrix [batch*np, kpad] in `dtype` (VH_DTYPE_BF16 or VH_DTYPE_FP16),
 * columns patch*patch*channels .. kpad-1 zero.  kpad >= patch*patch*channels and a multiple of 8 (the forward uses the
 * patch vector rounded up to 64).  vh_op_im2col needs patch*channels to be a multiple of 4 and writes no padding. */
int vh_op_im2col_padded(const float* in_nhwc_dev, int batch, int image, int patch, int channels, int kpad,
                        void* out16_dev, int dtype, void* stream);
/* The patch gather of the 8-bit entry points on its own: NHWC bytes -> patch matrix [batch*np, kpad] in `dtype`
 * (VH_DTYPE_BF16 or VH_DTYPE_FP16), element = dtype(fmaf((float)p, scale[c], shift[c])) with ONE rounding before the
 * conversion, i.e. the bits vh_op_im2col_padded gives for that fp32 array; columns patch*patch*channels .. kpad-1 zero.
 * Any patch <= 256 and channels <= 64, kpad >= patch*patch*channels and a multiple of 8; scale_host / shift_host: HOST
 * arrays [channels], finite; in_nhwc_dev 16-byte aligned (else VH_ERR_INVALID). */
int vh_op_im2col_u8(const uint8_t* in_nhwc_dev, int batch, int image, int patch, int channels, int kpad,
                    const float* scale_host, const float* shift_host, void* out16_dev, int dtype, void* stream);
/* The patch gather of the tensor entry points on its own ("Image tensors"): in_dev of elem VH_ELEM_* and layout VH_LAYOUT_* ->
 * patch matrix [batch*np, kpad] in `dtype` (VH_DTYPE_BF16 or VH_DTYPE_FP16): the bits vh_op_im2col_padded gives for the NHWC
 * fp32 array of the contract's values v; columns patch*patch*channels .. kpad-1 zero.  Any patch <= 256 and channels <= 64, kpad
 * >= patch*patch*channels and a multiple of 8; scale_host / shift_host: HOST arrays [channels], finite, read for VH_ELEM_U8
 * only (may be NULL otherwise); in_dev 16-byte aligned (else VH_ERR_INVALID).  Every argument is checked before a device is
 * touched. */
int vh_op_im2col_tensor(const void* in_dev, int elem, int layout, int batch, int image, int patch, int channels, int kpad,
                        const float* scale_host, const float* shift_host, void* out16_dev, int dtype, void* stream);
/* The resize of the frames entry points on its own ("8-bit frames"): frames_dev (any alignment, any offsets) ->
 * out_u8_dev [batch][out_size][out_size][channels] bytes.  desc_host: HOST array [batch]; channels 1..64, out_size
 * 1..4096.  Allocates and frees its table buffer: a test and measurement tap, not a hot path. */
int vh_op_resize_u8(const uint8_t* frames_dev, size_t nbytes, const vh_frame* desc_host, int batch, int channels,
                    int out_size, uint8_t* out_u8_dev, void* stream);
/* The resize + colour conversion of the NV12 entry points on its own ("NV12 frames"): frames_dev (any alignment, any
 * offsets) -> out_u8_dev [batch][out_size][out_size][3] bytes.  desc_host: HOST array [batch]; m12_host: HOST row-major
 * 3 x 4 matrix, all finite; chroma_site VH_CHROMA_*; out_size 1..4096.  Every argument and descriptor is checked before a
 * device is touched.  Allocates and frees its table buffer: a test and measurement tap, not a hot path. */
int vh_op_resize_nv12(const uint8_t* frames_dev, size_t nbytes, const vh_frame_nv12* desc_host, int batch, int out_size,
                      const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
/* The same tap for planar frames ("Planar YUV frames"): the arguments of vh_op_resize_nv12 with vh_frame_yuv descriptors.
 * Every argument and descriptor is checked before a device is touched. */
int vh_op_resize_yuv(const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuv* desc_host, int batch, int out_size,
                     const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
/* The same two taps for 16-bit samples ("16-bit YUV frames"): the arguments of their 8-bit twins; frames_dev must be 2-byte
 * aligned, offsets and strides even.  Every argument and descriptor is checked before a device is touched. */
int vh_op_resize_p016(const uint8_t* frames_dev, size_t nbytes, const vh_frame_nv12* desc_host, int batch, int out_size,
                      const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
int vh_op_resize_yuv16(const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuv* desc_host, int batch, int out_size,
                       const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
/* The same tap for packed 4:2:2 frames ("Packed 4:2:2 frames"): the arguments of vh_op_resize_yuv / vh_op_resize_yuv16 with
 * vh_frame_yuy2 descriptors.  _yuy2: any alignment.  _y210: frames_dev 2-byte aligned, offsets and strides even (v210: multiples
 * of 4).  Every argument and descriptor is checked before a device is touched. */
int vh_op_resize_yuy2(const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuy2* desc_host, int batch, int out_size,
                      const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
int vh_op_resize_y210(const uint8_t* frames_dev, size_t nbytes, const vh_frame_yuy2* desc_host, int batch, int out_size,
                      const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
/* The same tap for packed 4:4:4 frames ("Packed 4:4:4 frames"): the arguments of vh_op_resize_yuy2 / vh_op_resize_y210 with
 * vh_frame_bgra descriptors.  m12_host must be given and finite even where every layout is RGB (it is then unused); chroma_site is
 * accepted and has no effect.  _bgra: any alignment.  _y410: frames_dev 2-byte aligned, offsets and strides even (Y410 / V410:
 * multiples of 4).  Every argument and descriptor is checked before a device is touched. */
int vh_op_resize_bgra(const uint8_t* frames_dev, size_t nbytes, const vh_frame_bgra* desc_host, int batch, int out_size,
                      const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
int vh_op_resize_y410(const uint8_t* frames_dev, size_t nbytes, const vh_frame_bgra* desc_host, int batch, int out_size,
                      const float* m12_host, int chroma_site, uint8_t* out_u8_dev, void* stream);
/* fp32 -> dtype cast of n elements (n multiple of 4) */
int vh_op_cast(const float* in_dev, void* out16_dev, int64_t n, int dtype, void* stream);
/* The token-feature kernels on their own ("Token features"; the kernels vh_read_features* run): rows [batch * tokens, dim] given as
 * split planes (form VH_DTYPE_BF16 / VH_DTYPE_FP16: 16-bit hi + one scaled e4m3 byte per element in lo_dev; VH_DTYPE_FP8: e4m3 hi +
 * bf16 lo) or as fp32 rows (form -1, lo_dev NULL) -> patch_out_dev [batch][tokens - 1][dim] and mean_out_dev [batch][dim] of
 * `elem` (VH_ELEM_F32 / F16 / BF16); either may be NULL, not both.  norm VH_FEAT_NORM: through LayerNorm(gamma_dev, beta_dev, eps);
 * VH_FEAT_RAW: as they are (gamma_dev / beta_dev may be NULL).  dim % 8 == 0, 64 <= dim <= 2048, tokens 2..4097; every pointer
 * 16-byte aligned.  Every argument is checked before a device is touched, each refusal with a message of its own. */
int vh_op_token_features(const void* hi_or_x32_dev, const void* lo_dev, int form, int batch, int tokens, int dim,
                         const float* gamma_dev, const float* beta_dev, float eps, int elem, int norm, void* patch_out_dev,
                         void* mean_out_dev, void* stream);
/* vh_op_token_features with the rest of "Layer features": `lead` = 1 + the register rows in front of an image's patch rows (1 ..
 * tokens - 1; patch and mean cover rows lead .. tokens - 1), reg_out_dev [batch][lead - 1][dim] <- rows 1 .. lead - 1 (refused where
 * lead is 1), patch_layout VH_FEAT_ROWS ([batch][tokens - lead][dim]) or VH_FEAT_NCHW ([batch][dim][tokens - lead], the same elements
 * transposed; only the base pointer's alignment matters).  Any of the three outputs may be NULL, not all.  Every argument is checked
 * before a device is touched. */
int vh_op_token_features2(const void* hi_or_x32_dev, const void* lo_dev, int form, int batch, int tokens, int lead, int dim,
                          const float* gamma_dev, const float* beta_dev, float eps, int elem, int norm, void* patch_out_dev,
                          int patch_layout, void* mean_out_dev, void* reg_out_dev, void* stream);
/* The pooling kernel of the VH_FLAG_POOL modes on its own: mean_out_dev [batch][dim] fp32 <- the mean over rows lead .. tokens - 1
 * of every image, of the rows as they are (VH_FEAT_RAW) or through LayerNorm(gamma_dev, beta_dev, eps) (VH_FEAT_NORM), with the
 * arithmetic of "Token features": the bits vh_op_token_features2 writes into mean_out_dev for VH_ELEM_F32.  ONE pass over the rows
 * (one workgroup per image; a wave keeps a row in registers, the rows of a group meet in LDS and are added in ascending token order).
 * form / hi / lo as vh_op_token_features; lead 0 .. tokens - 1 (0: every row is a patch row, VH_FLAG_NO_CLS without registers),
 * tokens 1 .. 4097, dim % 8 == 0, 64 <= dim <= 2048, every pointer 16-byte aligned.  Every argument is checked before a device is
 * touched, each refusal with a message of its own. */
int vh_op_pool_rows(const void* hi_or_x32_dev, const void* lo_dev, int form, int batch, int tokens, int lead, int dim,
                    const float* gamma_dev, const float* beta_dev, float eps, int norm, float* mean_out_dev, void* stream);
/* The token-sized pass of the VH_FLAG_MAP_HEAD head on its own (the step z of "THE FUNCTION" at VH_FLAG_MAP_HEAD):
 * z_out_dev [batch][heads][dim] fp32 <- sum_t softmax_t(qk[h] . y_t) y_t over rows lead .. tokens - 1 of every image, y_t = the row
 * through LayerNorm(gamma_dev, beta_dev, eps).  qk_dev [heads][dim] fp32.  ONE pass over the rows: one workgroup per image, a wave
 * normalises a row in registers and computes its `heads` scores, the rows of a group meet in LDS and enter an online softmax in
 * ascending token order (exp2 of log2(e)-scaled scores, one rescale per group).  form / hi / lo / lead / tokens / dim and the
 * alignment rule as vh_op_pool_rows; heads 1 .. 16.  Every argument is checked before a device is touched, each refusal with a
 * message of its own. */
int vh_op_map_pool(const void* hi_or_x32_dev, const void* lo_dev, int form, int batch, int tokens, int lead, int dim,
                   const float* gamma_dev, const float* beta_dev, float eps, const float* qk_dev, int heads, float* z_out_dev,
                   void* stream);
/* The rotation of a VH_FLAG_ROPE context on its own ("THE FUNCTION" at VH_FLAG_ROPE), in place on caller-made q|k|v of `dtype`
 * (VH_DTYPE_BF16 / VH_DTYPE_FP16) elements: q and k of rows lead .. tokens - 1 of every image and head are rotated by cos_dev / sin_dev
 * [tokens - lead][head_dim / 2] fp32; v, the lead rows and every row beyond batch * tokens are never written.
 * hm_rows = 0: row-major [batch * tokens][3 * heads * head_dim], head_dim 32, 48, .. 128;  hm_rows != 0: head-major
 * [3][heads][hm_rows][64], head_dim 64 only, hm_rows >= batch * tokens.  16-byte accesses: qkv16_dev is 16-byte aligned.  Every argument
 * is checked before a device is touched, each refusal with a message of its own. */
int vh_op_rope(void* qkv16_dev, int dtype, int batch, int tokens, int heads, int head_dim, int lead, int64_t hm_rows,
               const float* cos_dev, const float* sin_dev, void* stream);
/* The gate pass of a VH_FLAG_SWIGLU context on its own ("THE FUNCTION" at VH_FLAG_SWIGLU): gu16_dev [rows][2 * mlp_dim] row-major `dtype`
 * (VH_DTYPE_BF16 / VH_DTYPE_FP16) elements, gate columns first -> h16_dev [rows][mlp_dim] = silu(g) * u of the same type: row-major
 * (out_tiled = 0) or the 16-row-blocked operand layout [rows / 16][mlp_dim / 8][16][8] (out_tiled = 1; rows a multiple of 16).  mlp_dim is a
 * multiple of 64; 16-byte accesses: both pointers are 16-byte aligned.  Nothing outside h16's rows * mlp_dim elements is written.  Every
 * argument is checked before a device is touched, each refusal with a message of its own. */
int vh_op_swiglu(const void* gu16_dev, int dtype, int64_t rows, int mlp_dim, void* h16_dev, int out_tiled, void* stream);
/* synthetic-data generator on the device: kind 0 = uniform[-1,1), 1 = Irwin-Hall(4) * sigma,
 * 2 = constant `sigma` */
int vh_op_fill(float* out_dev, int64_t n, uint64_t seed, uint32_t tensor_id, int kind,
               float sigma, void* stream);

/* micro-benchmark: average device time (ms) of one launch of the GEMM kernel on synthetic operands
 * generated in HBM (uniform[-1,1) activations, sigma=0.02 weights), `iters` launches between events */
int vh_bench_gemm(int device, int64_t M, int N, int K, int epilogue, int dtype, int variant, int iters,
                  double* avg_ms);

/* ---- device group: the N GPUs of one node from ONE process ---------------------------------------------------------
 * The reference drives a single device (clGetDeviceIDs(CL_DEVICE_TYPE_ACCELERATOR), netFPGA.cpp:376) with one input
 * vector per call (:266-277) and has no multi-device code; this is the C-ABI form of the image sharding the north star
 * asks for: one context + one host thread + one stream per device, ncclCommInitAll, ONE ncclBroadcast of the canonical
 * weight blob from member 0 over xGMI (the per-device upload of _load_params, netFPGA.cpp:484-515), contiguous image
 * ranges per member, per-member D2H into the caller's logits buffer; no collective on the data path.  RCCL is loaded at
 * run time and only for groups of more than one distinct device.  Listing one ordinal several times gives a REHEARSAL
 * group on one GPU (same threads, shards and blob path; the broadcast is a device-to-device copy).
 * cfg->max_batch is the per-device capacity.  A group is not re-entrant. */
typedef struct vh_group vh_group;
int vh_group_create(const vh_config* cfg, const int* devices, int n, vh_group** out);
int vh_group_destroy(vh_group* g);
int vh_group_size(const vh_group* g, int* n);
int vh_group_member(vh_group* g, int i, vh_ctx** ctx, int* device); /* the member's own context (borrowed) */
const char* vh_group_last_error(const vh_group* g);
/* image range [lo, hi) of member r for a batch split over n members (the first batch % n members take one extra) */
void vh_group_shard_bounds(int batch, int n, int r, int* lo, int* hi);
/* weights: loaded / generated on member 0, then broadcast; vh_group_broadcast_weights re-sends member 0's resident blob */
int vh_group_load_weights(vh_group* g, const void* host_blob, size_t nbytes);
int vh_group_init_weights_seeded(vh_group* g, uint64_t seed);
int vh_group_broadcast_weights(vh_group* g);
/* the hot path over the group (same buffers and meaning as vh_forward): synchronous, all members run concurrently */
int vh_group_forward(vh_group* g, const float* in_nhwc_host, int batch, float* logits_host);
/* measurement path with the inputs resident in every member's HBM (member i = shard i, seed + i) */
int vh_group_fill_inputs_seeded(vh_group* g, uint64_t seed, int batch_per_device);
int vh_group_forward_resident(vh_group* g, int batch_per_device, int steps);
int vh_group_read_logits(vh_group* g, int batch_per_device, float* logits_host); /* [n * batch_per_device, classes] */

/* ---- filter_image pipeline -------------------------------------------------------------------
 * The reference's second device entry: single-channel 8-bit frames (1080 x 1920, defines.h:31-38) pushed through
 * a kernel `image_process` with a 24-slot ring of in-flight frames (netFPGA.cpp:47-56, 292-365).  That kernel's
 * source and bitstream are absent, so WHAT it computed is unknown; the ring mechanics are reproduced and the
 * arithmetic is a documented choice: a 3x3 filter with replicated borders, integer arithmetic, bit-exact against
 * oracle_filter3x3.  Frames are `height * width` bytes, row-major. */
#define VH_FILTER_BLUR3 0   /* (1 2 1 / 2 4 2 / 1 2 1) / 16, rounded half up */
#define VH_FILTER_SOBEL3 1  /* min(255, |gx| + |gy|) */
typedef struct vh_filter vh_filter;
int vh_filter_create(int device, int height, int width, int slots, int kind, vh_filter** out);
int vh_filter_destroy(vh_filter* f);
int vh_filter_free_slots(const vh_filter* f, int* n);
int vh_filter_submit(vh_filter* f, const uint8_t* frame);   /* VH_ERR_RING_FULL when every slot is in flight */
int vh_filter_collect(vh_filter* f, uint8_t* frame);        /* oldest frame; VH_ERR_RING_EMPTY when none */
const char* vh_filter_last_error(const vh_filter* f);

/* ---- MLP mode: the reference's actual launch_forward semantics -------------------------- */
/* y_l = act(W_l y_{l-1} + b_l), weights row-major [n_out, n_in] per layer, layers and biases
 * concatenated exactly as the ctor flattens them (netFPGA.cpp:68-76, 91-106); kernel
 * argument list of network_v1 (netFPGA.cpp:427-436, 499-502). */
int vh_mlp_create(int device, int n_ins, int n_layers, const int* n_p_l, int activation,
                  vh_mlp** out);
int vh_mlp_load_params(vh_mlp* mlp, const float* params_host, size_t n_params,
                       const float* bias_host, size_t n_neurons);
/* n_vec input vectors of n_ins floats -> n_vec output vectors of n_p_l[n_layers-1] floats */
int vh_mlp_forward(vh_mlp* mlp, const float* inputs_host, int n_vec, float* outputs_host);
int vh_mlp_last_forward_us(const vh_mlp* mlp, int64_t* us);
/* Training of the dense chain: the device side of init_gradient / launch_gradient (netAbstract.h:14-15).  PARITY
 * UNPINNED: the reference's bodies are commented-out code (netFPGA.cpp:518-580) on a vector library that is not in the
 * repository.  Their loop shape is kept -- per iteration every set is back-propagated, its output error summed in
 * absolute value, the sets' gradients accumulated, normalised, applied, the accumulator reset (:552-565) -- and what
 * they leave undefined is fixed here:
 *   loss of a set       1/2 |a_L - t|^2   (delta of the last layer = (a_L - t) * act'(z_L))
 *   normalize_1         mean over the sets
 *   update              p -= multiplier * mean gradient, all layers from the deltas of the SAME parameters
 *   errors[it]          sum over sets and outputs of |a_L - t|, taken BEFORE the update of iteration `it`
 *   error_threshold     an iteration with errors[it] <= error_threshold ends the loop; later entries stay 0 (the value
 *                       the reference initialises its result with, :550)
 *   act'                identity 1; RELU2 1 on (0, 1); RELU 1 on z > 0; HARDTANH 1 on (-1, 1); GELU Phi(z) + z phi(z)
 * set_ins [n_sets][n_ins], set_outs [n_sets][n_p_l[n_layers-1]] (host); at most 65535 sets and neurons per layer.
 * vh_mlp_read_params copies the (trained) parameters back in the layout vh_mlp_load_params takes. */
int vh_mlp_init_gradient(vh_mlp* mlp, const float* set_ins_host, const float* set_outs_host, int n_sets);
int vh_mlp_launch_gradient(vh_mlp* mlp, int iterations, float error_threshold, float multiplier, float* errors_host);
int vh_mlp_read_params(vh_mlp* mlp, float* params_host, size_t n_params, float* bias_host, size_t n_neurons);
int vh_mlp_last_gradient_us(const vh_mlp* mlp, int64_t* us);
const char* vh_mlp_last_error(const vh_mlp* mlp);
int vh_mlp_destroy(vh_mlp* mlp);

#ifdef __cplusplus
}
#endif
#endif /* VITHIP_H */
