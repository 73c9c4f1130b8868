/*
 * adm_hip.h -- C ABI of libadm_hip.so: the MI355X (gfx950) kernels behind
 * AutoDiffusion's candidate-evaluation hot path.
 *
 * The reference (lilijiangg/AutoDiffusion) is 100 % Python on stock PyTorch
 * ops: it has NO plugin / FFI interface for this path (SURVEY.md section 2.2,
 * 8b).  The entry points below are therefore the build's own boundary; each
 * one cites the reference Python call site it replaces.  A maintainer binds
 * them with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes; every pointer is a DEVICE pointer unless the
 *     name ends in _host; no torch types, no allocation, no ownership transfer
 *     (workspaces are caller-owned), no hidden synchronisation;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return value: 0 = ok, negative = invalid argument (see ADM_E_*),
 *     positive = hipError_t from the launch; adm_last_error() returns a
 *     thread-local description of the last failure;
 *   - activations between kernels are bf16 NHWC ("pixel-major": [N][H][W][C]);
 *     the UNet's external input / output stay fp32 NCHW as in the reference;
 *   - safe to call concurrently on different streams / devices.
 */
#ifndef ADM_HIP_H
#define ADM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADM_ABI_VERSION 10  /* 2: adm_conv_args gained in_up / res_up; 3: ksplit / ws; 4: the Inception layer entry points; 5: up_phase; 6: geglu;
                               7: adm_gn_finalize_add gained stats, adm_gn_bwd_finalize gained add / add_stride; the classifier's other heads;
                               8: adm_conv_args gained fold0 / fold1 / fc0 / fc1;
                               9: adm_conv_args gained out_scale; CU-partitioned streams (adm_stream_create_cumask / _set_cus / _destroy);
                               10: the evaluation suite's k-NN entry points (adm_knn_smallest / adm_knn_cover);
                               still 10 (additive, nothing existing changed): the VAE decoder's adm_attention_1h512 / adm_vae_latent_in / adm_vae_image_out
                               and the KID sums adm_poly3_sums / adm_poly3_work_elems; the CMMD sums adm_rbf_sums / adm_rbf_work_elems */

#define ADM_E_ARG      (-1)  /* bad pointer / size / flag combination          */
#define ADM_E_SHAPE    (-2)  /* shape not supported by the gfx950 tiling       */
#define ADM_E_ALIGN    (-3)  /* pointer not 16-byte aligned                    */

typedef uint16_t adm_bf16;   /* raw bfloat16 bits */

int adm_abi_version(void);
const char* adm_last_error(void);

/* ---------------------------------------------------------------- CU-partitioned streams
 * The reference runs eps(x_t) and the guidance gradient one after the other on one CUDA stream
 * (gaussian_diffusion.py:381-393 condition_score after p_mean_variance); both depend on x_t only, so this build overlaps them
 * on two streams -- and may give each network its OWN compute units instead of time-sharing all of them:
 * adm_stream_create_cumask creates a HIP stream whose kernels run only on the CUs named by `mask` (`words` x 32 bits, bit i = CU i
 * in the driver's numbering: on an 8-XCD device consecutive bits go round-robin over the XCDs) and registers its CU count, which the
 * persistent kernels (adm_conv) read to size their grids.  adm_stream_set_cus(stream, n) registers / updates (n = 0: forgets) the
 * budget of a stream created elsewhere.  Results never depend on the partition.                                                  */
int adm_stream_create_cumask(const uint32_t* mask, int words, void** stream_out);
int adm_stream_set_cus(void* stream, int ncu);
int adm_stream_destroy(void* stream);
/* diagnostic: out_dev[b] = XCC_ID | HW_ID << 8 of block b of a grid of `nblocks` blocks launched on `stream` (which CUs a mask selects) */
int adm_stream_probe(uint32_t* out_dev, int nblocks, void* stream);

/* ---------------------------------------------------------------- sampler (K9, A7, A10)
 * Per-step scalars = the reference's float64 tables cast to float32 exactly as
 * _extract_into_tensor does (gaussian_diffusion.py:910-923).                           */
typedef struct adm_step_coefs {
  float sqrt_recip_ac;    /* sqrt(1/abar_i)            */
  float sqrt_recipm1_ac;  /* sqrt(1/abar_i - 1)        */
  float ac;               /* abar_i                    */
  float ac_prev;          /* abar_{i-1} (1.0 at i = 0) */
  float coef1, coef2;     /* posterior_mean_coef1/2    */
  float log_var_lo;       /* posterior_log_variance_clipped_i (LEARNED_RANGE min) or fixed log-variance */
  float log_var_hi;       /* log(beta_i) (LEARNED_RANGE max); unused for fixed variance   */
  float fixed_var;        /* fixed variance (FIXED_SMALL/LARGE); unused for learned range */
  float eta;              /* DDIM eta                  */
  int32_t nonzero;        /* 0 at i == 0, else 1       */
  int32_t learned_range;  /* model_out carries 2C channels (eps | v)      */
  int32_t predict_xstart; /* model output is x0 instead of eps            */
  int32_t clip_denoised;  /* clamp pred_xstart to [-1, 1]                 */
} adm_step_coefs;

/* ddim_sample: p_mean_variance + condition_score + eq. 12 update, one pass per pixel.
 * Replaces gaussian_diffusion.py:258-326, :381-393, :565-584.
 * x, noise, grad, x_prev, pred_xstart: fp32 [N,C,H,W]; model_out fp32 [N,C or 2C,H,W];
 * grad / noise / pred_xstart / u8_nhwc may be NULL.  If u8_nhwc != NULL the final image is
 * also packed as ((s+1)*127.5).clamp(0,255) truncated to uint8, NHWC
 * (search_imagenet64_classifier_guidance.py:352-354).                                   */
int adm_ddim_step(const float* x, const float* model_out, const float* grad, const float* noise,
                  float* x_prev, float* pred_xstart, uint8_t* u8_nhwc,
                  int n, int c, int h, int w, const adm_step_coefs* coefs_host, void* stream);

/* p_sample: p_mean_variance + condition_mean + ancestral update.
 * Replaces gaussian_diffusion.py:258-326, :365-369, :430-439.                           */
int adm_ddpm_step(const float* x, const float* model_out, const float* grad, const float* noise,
                  float* x_prev, float* pred_xstart, uint8_t* u8_nhwc,
                  int n, int c, int h, int w, const adm_step_coefs* coefs_host, void* stream);

/* fp32 NCHW in [-1,1] -> uint8 NHWC (truncation), search_...guidance.py:352-354.       */
int adm_pack_u8_nhwc(const float* x, uint8_t* out, int n, int c, int h, int w, void* stream);

/* ---------------------------------------------------------------- embeddings (K1, A4)
 * timestep_embedding (nn.py:103-121): t fp32 [N] -> [N, dim] = cos | sin (| 0 if dim odd). */
int adm_timestep_embedding(const float* t, float* out, int n, int dim, float max_period, void* stream);

/* out[n, o] = sum_k act(in[n, k]) * w[o, k] + bias[o] (+ table[idx[n], o]);  fp32.
 * act = SiLU if silu_in.  Replaces time_embed / label_emb / every ResBlock emb_layers
 * (unet.py:470-478, 199-205, 245, 648-654); all emb_layers are batched in one call by
 * concatenating their weights along o.                                                  */
int adm_linear_f32(const float* in, const float* w, const float* bias, const float* table,
                   const int64_t* idx, float* out, int n, int k, int o, int silu_in, void* stream);

/* ---------------------------------------------------------------- stem (A5, first conv)
 * input_blocks.0.0: conv3x3 pad 1 on the fp32 NCHW image -> bf16 NHWC (unet.py:480-483, 656-658).
 * cin <= 8, cout % 8 == 0, cout <= 512, and the weights and bias must fit the 64 KB of dynamic LDS the
 * kernel is launched with: (cin * 9 + 1) * cout * 4 <= 65536 (cin 3: any cout; cin 8: cout <= 224);
 * a larger shape is refused with ADM_E_SHAPE before the launch.                                    */
int adm_stem_conv3x3(const float* x_nchw, const float* w /*[Cout,Cin,3,3]*/, const float* bias,
                     adm_bf16* out_nhwc, int n, int cin, int h, int w_, int cout, void* stream);

/* The same layer on the MFMA path (what the engine uses): cast the image to bf16 NHWC with the channels
 * zero-padded to cpad = 32, then run adm_conv (3x3, raw prologue) with the stem weight zero-padded to 32
 * input channels.  The image is rounded to bf16 like every other activation (the reference rounds it to
 * fp16, unet.py:656).                                                                              */
int adm_nchw_to_nhwc_pad(const float* x_nchw, adm_bf16* out_nhwc, int n, int c, int h, int w, int cpad,
                         void* stream);

/* ---------------------------------------------------------------- GroupNorm (K2/K3 statistics)
 * GroupNorm32(32, C) statistics over a (virtually concatenated) bf16 NHWC tensor, in fp32 /
 * fp64 (nn.py:17-19).  Two launches:
 *   adm_gn_partial : per (image, pixel slab, channel) sum and sum of squares
 *                    -> partial fp32 [N][slabs][C][2]
 *   adm_gn_finalize: per (image, channel) affine  y = a*x + b  with
 *        a = rstd*gamma*(1+scale),  b = (beta - mean*rstd*gamma)*(1+scale) + shift
 *      (scale/shift = the ResBlock's FiLM pair, unet.py:248-252; NULL -> plain GN).
 *      film points at scale[0] of image 0; shift = film + C; film_stride = row stride.   */
int adm_gn_partial(const adm_bf16* in0, int c0, const adm_bf16* in1, int c1, float* partial,
                   int n, int hw, int slabs, void* stream);
int adm_gn_finalize(const float* partial, const float* gamma, const float* beta,
                    const float* film, int film_stride, float* aff_a, float* aff_b,
                    float* stats /* nullable: [N][32][2] = (mean, rstd), kept for adm_gn_bwd_* */,
                    int n, int c, int hw, int slabs, float eps, void* stream);
/* Same for a virtual concat whose two parts carry their own partial sums (e.g. from adm_conv's out_stats):
 * partial0 fp32 [N][slabs0][c0][2], partial1 fp32 [N][slabs1][c1][2] (NULL / 0 when there is one part). */
int adm_gn_finalize2(const float* partial0, int c0, int slabs0, const float* partial1, int c1, int slabs1,
                     const float* gamma, const float* beta, const float* film, int film_stride,
                     float* aff_a, float* aff_b, float* stats, int n, int hw, float eps, void* stream);

/* h_upd / x_upd of an up/down ResBlock (unet.py:190-195, 237-242):
 * out = resample(act(a*in + b)), act = SiLU when aff_a != NULL, identity copy otherwise.
 * mode 1 = AvgPool2d(2) (H,W -> H/2,W/2), mode 2 = nearest x2, mode 3 = every second pixel
 * (turns a stride-1 3x3 conv into the stride-2 Downsample of the latent UNet), mode 4 = zero-insert x2
 * (out[2y][2x] = in[y][x], 0 elsewhere, no affine: the backward-data conv of a stride-2 3x3 conv -- the classifier's
 * Downsample with classifier_resblock_updown = False, unet.py:115-140 -- is the stride-1 conv with transposed, flipped
 * weights over this tensor), mode 5 = the odd pixels (out[y][x] = act(in[2y+1][2x+1]), H and W even, the affine as mode 3:
 * the KL-f8 encoder's Downsample -- pad (0,1,0,1), then a stride-2 pad-0 3x3 conv, model.py:60-79 -- is the pad-1 stride-1
 * conv sampled at these pixels).                                                            */
int adm_resample(const adm_bf16* in, const float* aff_a, const float* aff_b, adm_bf16* out,
                 int n, int h, int w, int c, int mode, void* stream);

/* ---------------------------------------------------------------- fused conv / GEMM (K2,K3,K4,K7,K8)
 * Implicit-GEMM 3x3 (pad 1) or 1x1 convolution on MFMA, bf16 in / fp32 accumulate:
 *   out[p, o] = bias[o] + sum_{tap, c} act(a[n,c]*in[p+tap, c] + b[n,c]) * w[o, c, tap] (+ res[p, o])
 * with the input a virtual concat of (in0 | in1) along channels (th.cat, unet.py:662),
 * prologue: 0 = raw input, 1 = affine (GroupNorm, attention norm), 2 = affine + SiLU
 * (in_layers / out_layers / out, unet.py:182-186, 206-222, 612-616); zero padding is applied
 * AFTER the activation, as in the reference.  res (bf16 NHWC [.., cout]) may be NULL
 * (skip_connection(x) + h, unet.py:256; x + h, unet.py:305).
 * out_mode 0: bf16 NHWC; 1: fp32 NCHW (the UNet head, unet.py:664-665).
 * w_packed comes from adm_pack_conv_weight.  cin (= c0 + c1), c0, c1 % 32 == 0.          */
typedef struct adm_conv_args {
  const adm_bf16* in0; const adm_bf16* in1;
  const adm_bf16* w_packed; const float* bias;
  const float* aff_a; const float* aff_b;
  const adm_bf16* res; void* out;
  int32_t n, h, w, c0, c1, cout;
  int32_t taps;      /* 9 or 1 */
  int32_t prologue;  /* 0 raw, 1 affine, 2 affine + SiLU; 3 = raw input + GroupNorm-backward EPILOGUE (backward-data convs): with res = x
                        (the GroupNorm input in front, same shape as out; not added) and aff_a / aff_b its affine,
                        out = acc * SiLU'(a x + b) and out_stats = (sum out, sum out * x): adm_gn_bwd_partial is then not needed */
  int32_t out_mode;  /* 0,1    */
  int32_t variant;   /* tiling variant: 0 = auto (5 or 6 by least Cout padding, 3 for cout <= 16); 5 = 192-wide and
                        6 = 128-wide 8-wave tiles; 3 = 16-wide (output head / stem backward); 7 = 32x32x16 MFMA kernel;
                        10 = 1x1 with the activation tile resident in LDS (auto for 1x1, cin % 64 == 0, cout >= 256) */
  float* out_stats;  /* optional: fp32 [N][slabs][cout][2] = per-(image, slab, channel) sum and sum of squares of
                        the bf16 OUTPUT, accumulated in the epilogue (slabs = adm_conv_stat_slabs(args)); the
                        consumer's GroupNorm then needs no adm_gn_partial pass over the tensor */
  const adm_bf16* w_packed32; /* optional: the same weight in the 32x32x16 fragment order
                                 (adm_pack_conv_weight32); enables variant 7, the v_mfma_f32_32x32x16_bf16
                                 kernel for 3x3 convs on maps >= 16x16 */
  int32_t in_up;     /* 1: in0 is [n][h/2][w/2][c0] and is read through a virtual nearest-neighbour 2x upsample (the
                        prologue is applied on the way): ResBlock(up=True)'s h_upd(in_layers[:-1](x)) without the
                        upsampled tensor ever existing.  3x3, bf16 output, c1 == 0, variant 0/5/6 only */
  int32_t res_up;    /* 1: res is [n][h/2][w/2][cout], added through the same virtual upsample (x_upd(x)) */
  int32_t ksplit;    /* > 1: split-K for small batches (3x3 or 1x1, bf16 output, variant 5 / 6): the K loop of every output tile is
                        cut into `ksplit` runs of (c0 + c1) / 32 / ksplit chunks (an even count) that run as separate
                        tiles into `ws`, and a reduce pass adds them in index order with bias, residual and the output
                        statistics.  Deterministic; the result depends on ksplit (fp32 summation order), not on n */
  float* ws;         /* split-K workspace: fp32 [ksplit][n*h*w][cout], caller-owned */
  int32_t up_phase;  /* 1..4 = phase (py, px) = ((up_phase-1) >> 1, (up_phase-1) & 1) of conv3x3(nearest-upsample-2x(in0)): in0 is
                        the half-resolution [n][h][w][c0] source, `out` the [n][2h][2w][cout] tensor of which this launch writes
                        the pixels (2y + py, 2x + px).  Each phase is a 2x2-tap conv of the source: w_packed holds its pre-summed
                        weights embedded in a 3x3 window (adm_pack_conv_weight of the host-made 3x3 tensor: rows {w0, w1 + w2, 0}
                        for py = 0, {0, w0 + w1, w2} for py = 1, likewise for columns); the 5 zero taps are skipped: 4/9 of the
                        MACs of in_up = 1.  up_phase = 5 runs all four phases in ONE launch: w_packed then holds the four packed weights
                        back to back (phase-major) and the phase is part of the tile index (4 x as many tiles: small batches
                        still fill the chip).  out_stats has adm_conv_stat_slabs = 4 x (h / 16) x (w / 16) slabs, one per
                        (source tile, phase).  3x3, bf16 output, c1 == 0, no residual, source >= 16x16, variant 0/5/6            */
  int32_t geglu;     /* 1: GEGLU epilogue (Stable-Diffusion feed-forward, ldm/modules/attention.py:37-44: `x, gate = proj(x).chunk(2);
                        return x * gelu(gate)`): w_packed / bias hold the projection with its output rows INTERLEAVED (row 2m = value
                        m = reference row m, row 2m + 1 = gate m = reference row cout/2 + m), and `out` is [n][h][w][cout / 2] =
                        value * gelu(gate) (exact erf GELU on the fp32 accumulators): the [.., cout] tensor is never written.  1x1 on the
                        resident-tile kernel only: raw input, no res / out_stats, cout %% 16 == 0, cout > 192                      */
  const adm_bf16* fold0;  /* non-NULL: the ResBlock's `skip_connection(x) + h` (unet.py:216-222, 256) inside this out_layers conv: after the
                             nine-tap K loop, (fc0 + fc1) / 32 one-tap raw K-steps over the block's INPUT x = (fold0 | fold1) [n][h][w][fc]
                             with the skip_connection's 1x1 weights, which follow the 3x3 weights in w_packed (adm_pack_conv_weight of
                             each, concatenated); bias = conv bias + skip bias.  3x3, prologue 2, bf16 output, no res, map 8x8 or >= 16x16,
                             variant 0 / 5 / 6.  The 1x1 launch, its output tensor and the residual read of these tiles disappear.   */
  const adm_bf16* fold1;
  int32_t fc0, fc1;
  float out_scale;   /* fp32 NCHW output (out_mode 1) only: out = (acc + bias) * out_scale, applied in fp32 in the epilogue; 0 = 1.0.
                        The classifier's LAST backward-data conv (the stem's) undoes the static 2^10 scale of an fp16 backward
                        network here -- in fp32, not in its fp16 weights, where 2^-10 pushed a quarter of them into subnormals */
} adm_conv_args;
/* Which maps adm_conv takes.  What it accepts it computes on every pixel; anything else is refused with ADM_E_SHAPE / ADM_E_ARG before
 * the first launch, and nothing is written (tests/test_hip_conv_envelope.py walks 121 maps from 1x1 to 64x64 per family):
 *   3x3, variants 0 / 5 / 6      h and w multiples of 16 (16 x 16 tiles of one image), or the 8x8 map (two images per tile); so with a
 *                                residual, out_stats, ksplit and fold0.  prologue 3, in_up / res_up, up_phase, the fp32 NCHW output
 *                                and variants 3 / 7 / 8: h and w multiples of 16 only
 *   1x1 on the staged kernel     h * w = 64, 128 or a multiple of 256 -- and 32 on variants 0 / 5 / 6 with cout > 16 -- at any h and w
 *   (variants 0 / 3 / 5 / 6,     with that product: a 1x1 conv has no neighbours, so a map that does not tile as h x w (8x32, 1x64,
 *   ksplit, fp32 NCHW output)    24x32) is tiled as the (h w / 16) x 16 map of the same pixels.  4x48, 8x48, 24x24 are refused
 *   1x1 on the resident kernel   h * w a multiple of 64 (it indexes flat pixels); with variant 0 the other maps go to the staged kernel,
 *   (variant 10; variant 0 at    with variant 10 or geglu they are refused
 *   cout >= 256, cin % 64 == 0)
 *   out_stats                    adm_conv_stat_slabs > 0 exactly where adm_conv takes the request with out_stats: h and w multiples of
 *                                16; the 64-pixel maps a 1x1 conv takes (3x3: 8x8 only) except on variant 3; the resident kernel's maps */
int adm_conv(const adm_conv_args* args_host, void* stream);
/* slabs of out_stats for these arguments (0 = fused statistics not offered for this shape / variant). */
int adm_conv_stat_slabs(const adm_conv_args* args_host);
/* the tiling variant adm_conv will run for these arguments (resolves variant 0; 10 = resident-tile 1x1 kernel) */
int adm_conv_pick_variant(const adm_conv_args* args_host);

/* fp32 [cout, cin, kh, kw] (kh*kw = taps) -> bf16 fragment-ordered image
 * [cin/32][taps][ceil(cout/16)][64 lanes][8]; out must hold adm_packed_weight_elems().   */
int64_t adm_packed_weight_elems(int cout, int cin, int taps);
/* 32x32x16 fragment order [cin/32][taps][ceil(cout/32)][2][64 lanes][8]. */
int64_t adm_packed_weight32_elems(int cout, int cin, int taps);
int adm_pack_conv_weight32(const float* w, adm_bf16* out, int cout, int cin, int taps, void* stream);
int adm_pack_conv_weight(const float* w, adm_bf16* out, int cout, int cin, int taps, void* stream);

/* ---------------------------------------------------------------- attention (K5)
 * QKVAttention / QKVAttentionLegacy (unet.py:361-393 / 328-358) as a flash-style MFMA kernel:
 * qkv bf16 [N][T][3*H*D] (token-major, the 1x1 qkv conv's NHWC output) -> out bf16 [N][T][H*D];
 * softmax in fp32 over all T keys, logits scaled by 1/sqrt(D) (= the reference's
 * ch^-1/4 on q and on k).  new_order 1: channels are [3][H][D]; 0 (legacy): [H][3][D].
 * D in {32, 48, 64, 80, 96, 128} (tuned path; 48 / 80 add one 16-deep MFMA step) or {160, 192, 256} (ADM-128 / SD wide heads: sized to fit, not tuned). */
int adm_attention(const adm_bf16* qkv, adm_bf16* out, int n, int t, int heads, int d,
                  int new_order, void* stream);

/* Same, also writing the log2-domain log-sum-exp of the scaled logits, fp32 [N][H][T] (nullable):
 * P = exp2(s * log2(e)/sqrt(D) - lse).  Needed by adm_attention_bwd.                          */
int adm_attention_lse(const adm_bf16* qkv, adm_bf16* out, float* lse, int n, int t, int heads, int d,
                      int new_order, void* stream);

/* Attention with separate query and key/value tensors, heads of any supported width laid out (h d), and an explicit
 * logit scale: the SpatialTransformer's CrossAttention ("Stable Diffusion"/ldm/modules/attention.py:152-194:
 * softmax(q k^T * dim_head^-0.5) v; self-attention when kv aliases the query tensor).
 *   q   bf16 [N][tq][q_stride]       head h = columns h*d .. h*d+d
 *   kv  bf16 [N][kv_rows][kv_stride] K head h = columns h*d .., V head h = columns heads*d + h*d ..; only the first
 *                                    tk rows of every image are attended to (kv_rows >= tk is the row pitch)
 *   out bf16 [N][tq][heads*d];  scale <= 0 selects 1/sqrt(d).  d in {32, 48, 64, 80, 96, 128, 160, 192, 256}: other reference
 *   head widths (SD's 40 channels) are zero-padded by the caller's projection weights, with scale = true_dim^-0.5.     */
int adm_attention_cross(const adm_bf16* q, int q_stride, const adm_bf16* kv, int kv_stride, int kv_rows,
                        adm_bf16* out, int n, int tq, int tk, int heads, int d, float scale, void* stream);

/* ---------------------------------------------------------------- Stable-Diffusion latent UNet
 * LayerNorm over the channels of every token (torch.nn.LayerNorm(C), attention.py:205-207): bf16 [rows][C] -> bf16.  */
int adm_layernorm(const adm_bf16* x, const float* gamma, const float* beta, adm_bf16* out, int64_t rows, int c,
                  float eps, void* stream);
/* GEGLU gate (attention.py:36-44): out[r][i] = u[r][i] * gelu(u[r][inner+i]), u bf16 [rows][2*inner], exact GELU. */
int adm_geglu(const adm_bf16* u, adm_bf16* out, int64_t rows, int inner, void* stream);
/* GroupNorm affine of (x + e[n, c]) applied to the STORED x (ResBlock without scale-shift norm, openaimodel.py:253-258:
 * h = h + emb_out; h = out_layers(h)): statistics of x + e are derived from the partial sums of x, and
 * a = rstd*gamma, b = beta + (e - mean)*rstd*gamma.  add fp32 [N][add_stride].                                   */
int adm_gn_finalize_add(const float* partial, const float* gamma, const float* beta, const float* add, int add_stride,
                        float* aff_a, float* aff_b, float* stats /* nullable: (mean, rstd) of x + e per (image, group), for the backward pass */,
                        int n, int c, int hw, int slabs, float eps, void* stream);

/* One DDIM / PLMS update of the latent samplers (ddim.py:165-203, plms.py:195-258), fp32 tensors of numel elements:
 *   e     = eps_uncond ? eps_uncond + cfg_scale*(eps_cond - eps_uncond) : eps_cond        (written to e_out if given)
 *   e'    = w[0]*e + w[1]*h1 + w[2]*h2 + w[3]*h3                        (h* nullable: PLMS's old_eps, newest first)
 *   x0    = (x - sqrt_one_minus_at*e') / sqrt_at
 *   x_prev = sqrt_a_prev*x0 + dir_coef*e' + sigma*noise                 (dir_coef = sqrt(1 - a_prev - sigma^2))  */
typedef struct adm_sd_step_coefs {
  float cfg_scale;
  float w[4];
  float sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef, sigma;
} adm_sd_step_coefs;
int adm_sd_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* h1, const float* h2,
                const float* h3, const float* noise, float* x_prev, float* pred_x0, float* e_out, int64_t numel,
                const adm_sd_step_coefs* coefs_host, void* stream);

/* One multistep DPM-Solver++ update in data-prediction form (dpm_solver/dpm_solver.py:700-735, 755-810 with
 * model_wrapper's classifier-free guidance :289-330): e = guided eps, m = (x - sigma_s*e)/alpha_s (written to m_out, the
 * next step's model_prev), x_next = a*x + b0*m + b1*m_prev (m_prev nullable: first-order step).  fp32, numel elements. */
int adm_dpm_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* m_prev, float* x_next,
                 float* m_out, int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float a, float b0, float b1,
                 void* stream);

/* The same two updates (and adm_unipc_step_p below) for a model that predicts something other than eps (Stable Diffusion 2.x:
 * v).  `param` names what the model output is; any other value is refused before the launch.  The guidance combine is applied to
 * the RAW output, o = out_uncond ? out_uncond + cfg_scale*(out_cond - out_uncond) : out_cond, as SD 2's samplers do; with
 * ADM_PARAM_EPS each symbol launches exactly what its eps-only twin launches.  Each line below is one fp32 operation, rounded on
 * its own (no contraction), in this order:
 *   adm_sd_step_p   V   t1 = sqrt_at*o;  t2 = sqrt_one_minus_at*x;  e = t1 + t2
 *                   X0  t1 = sqrt_at*o;  t2 = x - t1;  e = t2 / sqrt_one_minus_at        (refused: sqrt_one_minus_at <= 0)
 *                   e_out holds e (the PLMS history is eps, as in SD 2's plms.py); e', x0 and x_prev are adm_sd_step's from e.
 *                   pred_x0 when h1 = h2 = h3 = NULL and w[0] == 1 (DDIM) is the direct form instead:
 *                   V   s1 = sqrt_at*x;  s2 = sqrt_one_minus_at*o;  x0 = s1 - s2           (predict_start_from_z_and_v)
 *                   X0  x0 = o
 *   adm_dpm_step_p  V   t1 = alpha_s*x;  t2 = sigma_s*o;  m = t1 - t2                      (dpm_solver.py:297-306 noise_pred_fn
 *                   X0  m = o                                                               folded into data_prediction_fn)
 *                   x_next from m as adm_dpm_step's.
 * Refusals are those of the eps-only symbols.  THE STREAM IS THE SECOND-TO-LAST ARGUMENT and `param` the last, as for
 * adm_poly3_sums: their per-element float64 checks live in tests/test_hip_sd_param.py.                                       */
#define ADM_PARAM_EPS 0
#define ADM_PARAM_X0 1
#define ADM_PARAM_V 2
int adm_sd_step_p(const float* x, const float* out_uncond, const float* out_cond, const float* h1, const float* h2,
                  const float* h3, const float* noise, float* x_prev, float* pred_x0, float* e_out, int64_t numel,
                  const adm_sd_step_coefs* coefs_host, void* stream, int param);
int adm_dpm_step_p(const float* x, const float* out_uncond, const float* out_cond, const float* m_prev, float* x_next,
                   float* m_out, int64_t numel, float cfg_scale, float sigma_s, float alpha_s, float a, float b0, float b1,
                   void* stream, int param);

/* ---------------------------------------------------------------- classifier guidance, backward-data (K10, A9)
 * The reference gets grad_x log p(y|x,t) from torch.autograd over EncoderUNetModel
 * (search_imagenet64_classifier_guidance.py:319-326, unet.py:685-896).  Here the backward network
 * is explicit; only data gradients exist (no weight gradients).
 *
 * Attention backward (flash-style recomputation; unet.py:297 re-runs the forward too):
 * qkv / dqkv bf16 [N][T][3*H*D], out / dout bf16 [N][T][H*D], lse from adm_attention_lse,
 * delta_ws fp32 [N][H][T] workspace.  D in {32, 64}.                                          */
int adm_attention_bwd(const adm_bf16* qkv, const adm_bf16* out, const adm_bf16* dout, const float* lse,
                      float* delta_ws, adm_bf16* dqkv, int n, int t, int heads, int d, int new_order,
                      void* stream);

/* GroupNorm(+FiLM)(+SiLU) backward for y = act(a*x + b) with (a, b, stats) from adm_gn_finalize:
 *   dx = a*dz + k1*x + k0 (+ add),  dz = dy * SiLU'(a*x+b)  (dz = dy when silu == 0).
 * partial: fp32 [N][slabs][C][2]; k1/k0: fp32 [N][C].  dy_half / add_half: that tensor lives at
 * (h/2, w/2) and is read as 0.25 * t[y/2, x/2] (AvgPool2d backward of down ResBlocks).          */
int adm_gn_bwd_partial(const adm_bf16* x, const adm_bf16* dy, const float* aff_a, const float* aff_b,
                       float* partial, int n, int h, int w, int c, int slabs, int silu, int dy_half,
                       void* stream);
/* add (nullable, fp32 [N][add_stride]): the layer normalised x + add[n, c] (adm_gn_finalize_add) while x is what was stored and
 * summed; the sums are corrected (sum dz (x + e) = sum dz x + e sum dz) and k0 absorbs k1 * e, so adm_gn_bwd_apply runs unchanged. */
int adm_gn_bwd_finalize(const float* partial, const float* aff_a, const float* stats, const float* add, int add_stride,
                        float* k1, float* k0, int n, int c, int hw, int slabs, void* stream);
int adm_gn_bwd_apply(const adm_bf16* x, const adm_bf16* dy, const float* aff_a, const float* aff_b,
                     const float* k1, const float* k0, const adm_bf16* add, adm_bf16* out,
                     int n, int h, int w, int c, int silu, int dy_half, int add_half, void* stream);
/* out = a + (b_half ? 0.25 * b[y/2, x/2] : b): gradient accumulation at a fan-out; with b_half,
 * b is [n, h/2, w/2, c] and h, w must be even (ADM_E_SHAPE otherwise).                          */
int adm_grad_add(const adm_bf16* a, const adm_bf16* b, adm_bf16* out, int n, int h, int w, int c,
                 int b_half, void* stream);

/* dlogits = scale * (onehot(y) - softmax(logits)) = scale * d/dlogits sum_n log_softmax[n, y_n];
 * logp_sel (nullable) receives log_softmax[n, y_n].  fp32 [N][K].                              */
int adm_logsoftmax_grad(const float* logits, const int64_t* y, float* dlogits, float* logp_sel,
                        int n, int k, float scale, void* stream);

/* AttentionPool2d (unet.py:22-51) around its single used query (token 0):
 *   adm_pool_prep     tok[n,0,:] = mean_p act + pos[:,0]; tok[n,1+p,:] = act[n,p,:] + pos[:,1+p],
 *                     act = SiLU(a*h + b); tok bf16 [N][tpad][C] (rows >= HW+1 zero); pos fp32 [C][HW+1]
 *   (qkv_proj = adm_conv 1x1 on tok viewed as 8x8 maps)
 *   adm_pool_attn_fwd a0[n,:] = attention output of token 0 (fp32 [N][C]); wts fp32 [N][H][tpad]
 *   (c_proj = adm_linear_f32)
 *   adm_pool_attn_bwd dqkv bf16 [N][tpad][3C] from da0 fp32 [N][C]
 *   adm_pool_prep_bwd d_act[n,p,:] = dtok[n,1+p,:] + dtok[n,0,:]/HW                               */
int adm_pool_prep(const adm_bf16* h, const float* aff_a, const float* aff_b, const float* pos, adm_bf16* tok,
                  int n, int hw, int c, int tpad, void* stream);
int adm_pool_attn_fwd(const adm_bf16* qkv, float* a0, float* wts, int n, int t, int tpad, int heads, int d,
                      void* stream);
int adm_pool_attn_bwd(const adm_bf16* qkv, const float* wts, const float* da0, adm_bf16* dqkv, int n, int t,
                      int tpad, int heads, int d, void* stream);
int adm_pool_prep_bwd(const adm_bf16* dtok, adm_bf16* dact, int n, int hw, int c, int tpad, void* stream);

/* Backward-data weight image for adm_conv: the conv with cin' = cout, cout' = cin and
 * w'[ci][co][t] = w[co][ci][taps-1-t].  out holds adm_packed_weight_elems(cin, cout, taps).     */
int adm_pack_conv_weight_bwd(const float* w, adm_bf16* out, int cout, int cin, int taps, void* stream);

/* ---------------------------------------------------------------- FID statistics (K11, A11)
 * Streaming float64 accumulation of s1[j] += sum_n a[n][j], s2[i][j] += sum_n a[n][i]*a[n][j] over a
 * batch of fp32 activations [n][d] (np.mean / np.cov, evaluations/evaluator_v1.py:218-221).
 * s1 fp64 [d], s2 fp64 [d][d], zero-initialised by the caller before the first batch.        */
int adm_fid_accumulate(const float* acts, double* s1, double* s2, int n, int d, void* stream);

/* ---------------------------------------------------------------- Inception-v3 pool3 features (K12, A11 compute_activations)
 * The layers of the FID feature extractor the reference runs through third-party code: a frozen TensorFlow graph
 * (evaluations/evaluator_v1.py:263-269, 665-679) / pytorch_fid.inception.InceptionV3 (Stable Diffusion
 * scripts/search_ea.py:95-127, 171-182).  BasicConv2d = conv(no bias) + BatchNorm(eps 1e-3) + ReLU: the caller folds the
 * BatchNorm scale into the packed weights and passes the shift as `bias`.
 *
 * adm_conv2d: general 2-D convolution, NHWC.  `in` = [n][h][w_in][in_stride] elements of which channels [0, cin_pad) are
 * read (cin_pad % 32 == 0; channels beyond the layer's real cin must hold zeros or meet zero weights); `w` from
 * adm_pack_conv2d_weight = [cout][kh*kw][cin_pad]; `out` = [n][oh][ow][out_stride] of which channels [0, cout) are written
 * -- point it at a channel slice of a concatenated tensor (cout % 4 == 0, 8-byte aligned).
 *
 * What adm_conv2d and adm_pool2d take.  What they accept they compute on every output element; anything else is refused with
 * ADM_E_ARG / ADM_E_SHAPE / ADM_E_ALIGN before any launch, and nothing is written (tests/test_hip_conv2d_envelope.py walks the
 * tables of tests/conv2d_envelope.py: every kernel pick at 1 .. 196 K-steps, M = n oh ow around the 64 / 128 / 256-pixel tiles,
 * partial channel tiles, odd geometry and every layout below, and one request per refusal):
 *   output size     the window must fit the padded image, h + 2 pad_h >= kh and w + 2 pad_w >= kw (pool: pad and k on both axes);
 *                   then oh = floor((h + 2 pad_h - kh) / stride) + 1 >= 1, likewise ow.  A window that does not fit is
 *                   ADM_E_SHAPE at every stride: no division is taken of a negative numerator
 *   adm_conv2d      accepted: n, h, w_in, kh, kw, stride >= 1 and pad_h, pad_w >= 0, in any combination -- windows larger than the
 *                   image, pads beyond the window, strides that do not divide the map; cin_pad a multiple of 32 with
 *                   in_stride >= cin_pad a multiple of 8 (channels cin_pad .. in_stride are never read, `in` may be a channel
 *                   slice at a multiple of 8 channels); cout a multiple of 4 with out_stride >= cout a multiple of 4; bias or
 *                   none; operands below 2 GiB.  Refused: anything else (ADM_E_ARG: null in / w / out, a size or stride < 1, a
 *                   negative pad; ADM_E_SHAPE: the channel rules, the output size, the 2 GiB limit; ADM_E_ALIGN: in, w or bias
 *                   off 16 bytes, out off 8)
 *   adm_pool2d      accepted: n, h, w, k, stride >= 1, 0 <= pad < k (so every window holds a tap inside the image, also at pads
 *                   torch refuses), mode 0 / 1, c a multiple of 8 within in_stride and out_stride, multiples of 8.  Refused:
 *                   anything else (ADM_E_ARG: null pointers, sizes, pad >= k, another mode; ADM_E_SHAPE: the channel rules, the
 *                   output size; ADM_E_ALIGN: in or out off 16 bytes)                                                            */
typedef struct adm_conv2d_args {
  const adm_bf16* in; const adm_bf16* w; const float* bias; adm_bf16* out;
  int32_t n, h, w_in, cin_pad, in_stride, cout, out_stride, kh, kw, stride, pad_h, pad_w;
  int32_t relu;      /* 1: max(x, 0) after the bias */
} adm_conv2d_args;
int adm_conv2d(const adm_conv2d_args* args, void* stream);
/* fp32 [cout][cin][kh][kw] (torch Conv2d.weight), optionally times scale[cout], -> the 16-bit layout above */
int adm_pack_conv2d_weight(const float* w, const float* scale, adm_bf16* out, int cout, int cin, int kh, int kw, int cin_pad,
                           void* stream);
/* k x k pooling of a channel slice (c % 8 == 0).  mode 0: max (F.max_pool2d), 1: average over the taps inside the image
 * (F.avg_pool2d(count_include_pad=False), the FID variant of the Inception blocks)                                        */
int adm_pool2d(const adm_bf16* in, adm_bf16* out, int n, int h, int w, int c, int in_stride, int out_stride, int k, int stride,
               int pad, int mode, void* stream);
/* mean over the hw pixels: [n][hw][c] -> fp32 [n][c] (the pool3 features)                                                 */
int adm_global_avgpool_f32(const adm_bf16* in, float* out, int n, int hw, int c, void* stream);
/* 3-channel images -> [n][oh][ow][cpad] (channels 3.. zero), value * scale + shift.  kind 0: uint8 NHWC, 1: fp32 NCHW,
 * 2: fp32 NHWC.  half_pixel 1: torch bilinear, align_corners=False (pytorch_fid); 0: TensorFlow-1 ResizeBilinear;
 * 2: torch BICUBIC, align_corners=True (the CLIP image entry): src = dst (in - 1) / (out - 1), 0 where out == 1, cubic
 * convolution with A = -0.75 over four border-clamped taps per axis, fp32, scale and shift on the interpolated value, one
 * rounding.  Any other half_pixel: ADM_E_ARG.                                                                             */
int adm_resize_bilinear(const void* in, adm_bf16* out, int n, int h, int w, int oh, int ow, int cpad, int kind, int half_pixel,
                        float scale, float shift, void* stream);

/* ---------------------------------------------------------------- the classifier's other heads (A9 variants)
 * EncoderUNetModel pool = "adaptive" | "spatial" | "spatial_v2" (guided_diffusion/unet.py:826-856, 880-896); create_classifier's
 * default and every launch script use "attention" (above).  The Linear layers between these are adm_linear_f32.
 *   adm_channel_mean  out[n][ch] = mean_p act(h[n][p][ch]), act = SiLU(a h + b) with the affine (adaptive: GN -> SiLU -> AvgPool),
 *                     identity without (spatial: h.mean(dim=(2, 3)) of every block, written at a column offset of the feature row)
 *   adm_bcast_add     out[n][p][ch] = (add ? add[n][p][ch] : 0) + v[n][ch] * scale: the backward of a pixel mean (scale = 1 / HW)
 *                     accumulated into the gradient that flows through the same tensor
 *   adm_vec_act       mode 1 SiLU, 2 ReLU on fp32 vectors: out = act(x), or with dy: out = dy * act'(x);
 *                     mode 3 the std of a diagonal Gaussian posterior from its log-variance (distributions.py:28-30):
 *                     out = expf(0.5f * clamp(x, -30, 20)), or with dy: out = dy * that (noise x std);
 *                     mode 4 the clamped log-variance itself, out = clamp(x, -30, 20) (dy must be NULL)
 *   adm_vec_gn(_bwd)  GroupNorm32(32, C) of fp32 [N][C] rows (spatial_v2's normalization(2048): no spatial axis), stats fp32
 *                     [N][32][2] = (mean, rstd); backward-data dx from dz = d(loss)/d(y)                                    */
int adm_channel_mean(const adm_bf16* h, const float* aff_a, const float* aff_b, float* out, int out_stride, int n, int hw, int c,
                     void* stream);
int adm_bcast_add(const float* v, int v_stride, float scale, const adm_bf16* add, adm_bf16* out, int n, int hw, int c, void* stream);
int adm_vec_act(const float* x, const float* dy, float* out, int64_t items, int mode, void* stream);
int adm_vec_gn(const float* x, const float* gamma, const float* beta, float* y, float* stats, int n, int c, float eps, void* stream);
int adm_vec_gn_bwd(const float* x, const float* gamma, const float* stats, const float* dz, float* dx, int n, int c, void* stream);

/* ---------------------------------------------------------------- k-NN precision / recall (K13, the ADM evaluation suite)
 * ManifoldEstimator of evaluations/evaluator.py (:319-352 manifold_radii, :396-430 evaluate_pr, :458-500 DistanceBlock) as one
 * fp16 GEMM per call with the selection / comparison in its epilogue (no distance matrix in memory).  Features are IEEE half
 * rows [n][d] (the reference's tf.float16 cast, in both builds of the library), d % 64 == 0, 16-byte aligned; norms are fp32
 * [n] squared norms of the SAME half rows; dist(i, j) = max(|p_i|^2 + |x_j|^2 - 2 p_i . x_j, 0) with an fp32 dot product.
 *   adm_knn_smallest  out[c][0..kk) = the kk smallest dist(q_c, x_j) over all j < nx, ascending (x may be q itself: then the
 *                     point's own ~0 distance is one of them, as in the reference); 1 <= kk <= 8, nx >= kk.  The rows of x
 *                     are split over `splits` blocks per 128 queries (1 <= splits <= ceil(nx / 128)); splits > 1 needs the
 *                     caller's workspace ws fp32 [splits][nq][kk].  Bitwise independent of `splits`.
 *   adm_knn_cover     a_in[i][k] = 1 if dist(a_i, b_j) <= rb[j][k] for some j; b_in[j][k] = 1 if dist(a_i, b_j) <= ra[i][k] for
 *                     some i; radii fp32 [n][K], 1 <= K <= 8; flags uint8 [n][K], ZEROED BY THE CALLER (only 1s are stored). */
int adm_knn_smallest(const void* q, int nq, const float* qnorm, const void* x, int nx, const float* xnorm, int d, int kk,
                     float* out, float* ws, int splits, void* stream);
int adm_knn_cover(const void* a, int na, const float* anorm, const float* ra, const void* b, int nb, const float* bnorm,
                  const float* rb, int d, int K, uint8_t* a_in, uint8_t* b_in, void* stream);

/* ---------------------------------------------------------------- KL-f8 VAE decoder (K14: Stable Diffusion first stage)
 * The decoder (ldm/modules/diffusionmodules/model.py:462-568) runs on adm_conv / adm_gn_* / adm_attention; these are the three
 * pieces those do not cover.
 *   adm_attention_1h512  single-head attention of width 512 (AttnBlock, model.py:186-198): qkv 16-bit [n][t][1536] with q | k | v
 *                        at columns 0 / 512 / 1024 -> out 16-bit [n][t][512] = softmax(q k^T * 512^-1/2) v.  One launch, fp32
 *                        online softmax, no [t][t] tensor in memory; any t >= 1 (rows beyond t are read as zeros, never written);
 *                        an image's result does not depend on n.
 *   adm_vae_latent_in    z fp32 NCHW [n][e][h][w] -> out 16-bit NHWC [n][h][w][32]: channels [0, zc) = post_quant_conv(inv_scale * z)
 *                        (the 1x1 Conv2d(e, zc) of ldm/models/autoencoder.py:303, 330-331 after ddpm.py:713; weight fp32 [zc][e],
 *                        bias fp32 [zc], fp32 math), channels [zc, 32) = 0: the operand of the decoder's conv_in.  zc <= 32, e <= 16.
 *   adm_vae_image_out    x fp32 NCHW [n][3][h][w] -> unit fp32 NCHW = min(max((x + 1) / 2, 0), 1) (scripts/search_ea.py:540) and / or
 *                        u8 uint8 NHWC = (uint8)(255 * unit), truncated (scripts/txt2img.py:337-339).  Either output may be NULL,
 *                        not both.                                                                                              */
int adm_attention_1h512(const adm_bf16* qkv, adm_bf16* out, int n, int t, void* stream);
int adm_vae_latent_in(const float* z, const float* w, const float* b, float inv_scale, adm_bf16* out, int n, int zc, int e, int h,
                      int w_, void* stream);
int adm_vae_image_out(const float* x, float* unit, uint8_t* u8, int n, int h, int w, void* stream);

/* ---------------------------------------------------------------- CLIP text transformer (K15: Stable Diffusion cond stage)
 * FrozenCLIPEmbedder (ldm/modules/encoders/modules.py:137-162) = transformers' CLIPTextModel: pre-LN layers of causal
 * self-attention and a quick_gelu MLP.  The projections are adm_conv 1x1 launches over the token rows of a prompt laid out as a
 * pixel map of `pitch` >= t rows, the inner LayerNorms adm_layernorm; these are the four pieces those do not cover.
 *   adm_clip_embed        out 16-bit [n][pitch][c]: row r < t of prompt i = tok[ids[i][r]] + pos[r] (fp32 add, one rounding), rows
 *                         t .. pitch-1 = 0.  ids int64 [n][t], tok fp32 [vocab][c], pos fp32 [positions][c], t <= positions,
 *                         c % 8 == 0.  An id outside [0, vocab) is the caller's error; the kernel clamps it into the table.
 *   adm_attention_causal  qkv 16-bit [n][pitch][3*heads*64], q | k | v thirds with head h at columns h*64 of each -> out 16-bit
 *                         [n][pitch][heads*64], rows < t only: softmax(q k^T * 64^-1/2 + causal mask) v, key j visible to query i
 *                         iff j <= i.  d must be 64, 1 <= t <= 256.  fp32 logits and online softmax; masked weights are exactly 0;
 *                         rows >= t of qkv are never read and rows >= t of out never written; a prompt's result does not depend
 *                         on n.
 *   adm_quick_gelu        16-bit [rows][inner] -> u * sigmoid(1.702 u) in fp32, same type (inner % 8 == 0)
 *   adm_gelu              16-bit [rows][inner] -> 0.5 u (1 + erf(u / sqrt 2)) in fp32, rounded once to the same type (inner % 8 == 0):
 *                         the exact GELU of the OpenCLIP text tower (Stable Diffusion 2.x); checks as adm_quick_gelu's.  THE STREAM
 *                         IS ITS SECOND-TO-LAST ARGUMENT and `flags` (0) the last, as for adm_poly3_sums: its per-element float64
 *                         check lives in tests/test_hip_sd_param.py
 *   adm_layernorm_f32out  LayerNorm (fp32 two-pass statistics) of rows < t of x 16-bit [n][pitch][c] -> fp32 [n][t][c]        */
int adm_clip_embed(const int64_t* ids, const float* tok, const float* pos, adm_bf16* out, int n, int t, int pitch, int c, int vocab,
                   int positions, void* stream);
int adm_attention_causal(const adm_bf16* qkv, adm_bf16* out, int n, int t, int pitch, int heads, int d, void* stream);
int adm_quick_gelu(const adm_bf16* u, adm_bf16* out, int64_t rows, int inner, void* stream);
int adm_gelu(const adm_bf16* u, adm_bf16* out, int64_t rows, int inner, void* stream, int flags);
int adm_layernorm_f32out(const adm_bf16* x, const float* gamma, const float* beta, float* out, int n, int t, int pitch, int c,
                         float eps, void* stream);

/* ---------------------------------------------------------------- Kernel Inception Distance (K16: the cubic-kernel sums)
 * Project-defined (the reference has no KID; the convention is Binkowski et al. 2018 / torch-fidelity's defaults):
 *   k(a, b) = (a . b / d + 1)^3 over fp32 rows x [n][d], y [m][d] (d % 4 == 0, 16-byte aligned; fp32 in both builds of the library).
 *   self_pairs = 0:  out[0] = sum_i sum_j k(x_i, y_j)
 *   self_pairs = 1:  out[0] = sum_{i != j} k(x_i, x_j)   (y == x or NULL, m == n; the diagonal is left out, not subtracted)
 * One f64 matrix-core GEMM (fp32 operands widened: exact products, f64 accumulation) with the cube and the reduction in its
 * epilogue: the n x m matrix never exists in memory.  Every sum is f64; one partial per block goes to the caller's workspace
 * `work` (f64, at least adm_poly3_work_elems(n, m, self_pairs) elements, -1 for a shape it refuses; nothing is allocated) and a
 * single-block pass adds them in a fixed order -- no atomics, two calls on the same inputs are bitwise equal.  Only out[0] and
 * the first adm_poly3_work_elems elements of work are written.
 * THE STREAM IS THE SECOND-TO-LAST ARGUMENT and the integer mode the last: tests/launch_replay.py counts every symbol whose
 * LAST argument is the stream pointer into its replay census; this symbol's per-element float64 check lives in
 * tests/test_hip_kid.py instead (a later change to that table should list it there).                                       */
int64_t adm_poly3_work_elems(int64_t n, int64_t m, int self_pairs);
int adm_poly3_sums(const float* x, int64_t n, const float* y, int64_t m, int d, double* work, int64_t work_elems, double* out,
                   void* stream, int self_pairs);

/* ---------------------------------------------------------------- CMMD (K18: the Gaussian RBF kernel sums on CLIP embeddings)
 * Still ABI 10 (additive).  Project-defined (the reference has no CMMD; after Jayasumana et al., "Rethinking FID", CVPR 2024):
 * over fp32 rows x [n][d], y [m][d] (NOT normalised; d % 4 == 0, 16-byte aligned; fp32 in both builds of the library), all in f64,
 *   r_i = |x_i|^2, s_j = |y_j|^2, c_ij = x_i . y_j / sqrt(r_i s_j), D_ij = max(2 - 2 c_ij, 0), kappa_ij = expm1(-gamma D_ij)
 *   self_pairs = 0:  out[0] = sum_i sum_j kappa_ij
 *   self_pairs = 1:  out[0] = sum_{i != j} kappa_ij   (y == x or NULL, m == n; the diagonal is skipped by index)
 * kappa = k - 1 <= 0 for the kernel k = exp(-gamma |a - b|^2) on unit vectors: the ones cancel in the estimator, not in the sum.
 * Three launches: the row norms (one wave per row), the 64 x 64 f64 matrix-core Gram tiles with the normalisation, expm1 and the
 * reduction in their epilogue (the n x m matrix never exists), and a single-block pass over the per-block partials -- no atomics,
 * two calls on the same inputs are bitwise equal.  `work` (f64) holds at least adm_rbf_work_elems(n, m, self_pairs) = blocks + n + m
 * elements (-1 for a shape it refuses; nothing is allocated): the partials, then r[n], then s[m], which the caller may read (a row
 * of norm 0 makes out[0] NaN).  Only out[0] and those elements of work are written.  Refused before any launch: null pointers,
 * misalignment, n or m < 1, d < 4 or d % 4 != 0, gamma not finite or <= 0, a workspace that is too small, self_pairs with m != n or
 * y != x.  THE STREAM IS THE SECOND-TO-LAST ARGUMENT and the integer mode the last, as for adm_poly3_sums: the per-element float64
 * check lives in tests/test_hip_cmmd.py.                                                                                        */
int64_t adm_rbf_work_elems(int64_t n, int64_t m, int self_pairs);
int adm_rbf_sums(const float* x, int64_t n, const float* y, int64_t m, int d, double gamma, double* work, int64_t work_elems,
                 double* out, void* stream, int self_pairs);

/* ---------------------------------------------------------------- DPM-Solver on the pixel (ADM) path (K17)
 * Still ABI 10 (additive).  Reference: ldm/models/diffusion/dpm_solver/dpm_solver.py -- model_wrapper's classifier guidance
 * :312-335, data_prediction_fn with Imagen's dynamic thresholding :386-399, the multistep updates :504-549 and :755-857.
 *
 * adm_abs_quantile: out[i] = torch.quantile(v[i].abs(), q) ('linear') of the fp32 rows v [n][per], exactly: the rank is
 * float32(q) * (per - 1) in float32, its floor and ceil pick two order statistics by radix selection over the bit patterns of |v|
 * (the elements a sort would give; -0 is 0), torch's lerp joins them.  Integer LDS atomics only: two calls are bitwise equal.  No
 * host synchronisation, nothing allocated: `work` (16-byte aligned) holds at least adm_abs_quantile_work_bytes(n, per) bytes (-1
 * for sizes it refuses).  0 < q < 1.  NaN inputs sort above +inf; where both order statistics are the same value the result is that
 * value (torch answers NaN for inf - inf).  Only out[0 .. n) and the first adm_abs_quantile_work_bytes bytes of work are written.
 *
 * adm_pix_dpm_step: one model evaluation of the solver on fp32 NCHW tensors, in the reference's order of operations:
 *   eps = model_out[:, :C]  (start_x: eps = (x_eval - alpha_s out) / sigma_s);   grad: eps -= sigma_s grad  (grad carries the
 *   classifier scale);   predict_x0: m = (x_eval - sigma_s eps) / alpha_s, thresholding: s = max(quantile_q |m|, max_val) per image,
 *   m = clamp(m, -s, s) / s;   else m = eps;   x_next = a x_base + b0 m + b1 h1 + b2 h2.
 * Required: x_eval, model_out (model_channels = C or 2C), m_out; x_base with x_next.  grad, h1, h2 (their terms are skipped),
 * x_next, u8_nhwc (the pack of adm_ddim_step, of x_next, or of m where x_next is NULL) and s_out (written with thresholding only)
 * may be NULL.  Without thresholding: one launch, work unused.  With it (predict_x0 required): the selection over |x0| computed on
 * the fly, then the update, which recomputes the same x0; work as for adm_abs_quantile(n, C h w).
 * Both refuse (nonzero, adm_last_error, nothing launched): null required pointers, thresholding without predict_x0, q outside
 * (0, 1), max_val <= 0, a work buffer that is too small, sizes whose products overflow.
 * THE STREAM IS THE SECOND-TO-LAST ARGUMENT of both and `flags` (0) the last, as for adm_poly3_sums: their per-element float64
 * checks live in tests/test_hip_adm_dpm.py.                                                                                  */
typedef struct adm_pix_dpm_args {
  const float* x_eval;
  const float* model_out;
  const float* grad;
  const float* x_base;
  const float* h1;
  const float* h2;
  float* m_out;
  float* x_next;
  uint8_t* u8_nhwc;
  float* s_out;
  void* work;
  int64_t work_bytes;
  int32_t n, c, h, w;
  int32_t model_channels, start_x, predict_x0, thresholding;
  float alpha_s, sigma_s, a, b0, b1, b2, q, max_val;
} adm_pix_dpm_args;
int64_t adm_abs_quantile_work_bytes(int64_t n, int64_t per);
int adm_abs_quantile(const float* v, int64_t n, int64_t per, float q, void* work, int64_t work_bytes, float* out, void* stream,
                     int flags);
int adm_pix_dpm_step(const adm_pix_dpm_args* args, void* stream, int flags);

/* ---------------------------------------------------------------- UniPC (Zhao et al., NeurIPS 2023) on both paths (K18)
 * Still ABI 10 (additive).  The reference tree has no UniPC: the algorithm is stated in DESIGN.md section 11.1 and
 * autodiffusion_amd/unipc.py, whose float64 coefficients these kernels apply.  One model evaluation yields two states:
 *
 * adm_pix_unipc_step (fp32 NCHW), with m exactly adm_pix_dpm_step's model value (the same inlined function; with thresholding the
 * same selection launch first, then one update launch):
 *   x_c    = x_corr given ? ac x_base + c0 m + c1 h1 + c2 h2 + c3 h3 : x_eval      the corrector of the update that arrived at x_eval
 *   x_pred = ap x_c + p0 m + p1 h1 + p2 h2                                          the predictor of the next update
 * fp32, left to right, no contraction; the term of a NULL history pointer is skipped.  Required: x_eval, model_out (C or 2C
 * channels), m_out; x_base with x_corr.  grad, h1, h2, h3, x_corr, x_pred, u8_nhwc and s_out (written with thresholding only) may be
 * NULL.  u8_nhwc is the pack of x_pred, of x_corr where x_pred is NULL, of m where both are (the denoise evaluation).  work as for
 * adm_pix_dpm_step.  Refuses (nonzero, adm_last_error, nothing launched, nothing written) what adm_pix_dpm_step refuses, and x_corr
 * without x_base.
 *
 * adm_unipc_step (fp32, numel elements), the guided data prediction of adm_dpm_step:
 *   e = eps_uncond ? eps_uncond + cfg_scale (eps_cond - eps_uncond) : eps_cond;   m = (x_eval - sigma_s e) / alpha_s
 * and the same x_c / x_pred.  Required: x_eval, eps_cond, m_out; x_base with x_corr; numel > 0, alpha_s > 0.
 * THE STREAM IS THE SECOND-TO-LAST ARGUMENT of both and `flags` (0) the last: their per-element float64 checks live in
 * tests/test_hip_unipc.py and tests/test_hip_sd_unipc.py.                                                                    */
typedef struct adm_pix_unipc_args {
  const float* x_eval;
  const float* model_out;
  const float* grad;
  const float* x_base;
  const float* h1;
  const float* h2;
  const float* h3;
  float* m_out;
  float* x_corr;
  float* x_pred;
  uint8_t* u8_nhwc;
  float* s_out;
  void* work;
  int64_t work_bytes;
  int32_t n, c, h, w;
  int32_t model_channels, start_x, predict_x0, thresholding;
  float alpha_s, sigma_s, ac, c0, c1, c2, c3, ap, p0, p1, p2, q, max_val;
} adm_pix_unipc_args;
typedef struct adm_unipc_args {
  const float* x_eval;
  const float* eps_uncond;
  const float* eps_cond;
  const float* x_base;
  const float* h1;
  const float* h2;
  const float* h3;
  float* m_out;
  float* x_corr;
  float* x_pred;
  int64_t numel;
  float cfg_scale, sigma_s, alpha_s, ac, c0, c1, c2, c3, ap, p0, p1, p2;
} adm_unipc_args;
int adm_pix_unipc_step(const adm_pix_unipc_args* args, void* stream, int flags);
int adm_unipc_step(const adm_unipc_args* args, void* stream, int flags);
/* adm_unipc_step for a model output named by `param` (ADM_PARAM_*, above): m as adm_dpm_step_p's with x = x_eval (V: t1 =
 * alpha_s*x_eval; t2 = sigma_s*o; m = t1 - t2.  X0: m = o), everything after m unchanged; `param` stands where `flags` does. */
int adm_unipc_step_p(const adm_unipc_args* args, void* stream, int param);

#ifdef __cplusplus
}
#endif
#endif /* ADM_HIP_H */
