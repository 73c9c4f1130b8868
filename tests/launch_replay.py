"""Launch recorder, float64 restatements and per-element error bounds for tests/test_hip_launch_replay.py and, for the KL-f8 VAE
encoder's launches and head, tests/test_hip_vae_encoder_replay.py.

Recording, at two levels.  Census: every exported symbol of autodiffusion_amd/_lib.SIGNATURES whose last argument is the stream
pointer is a launch (launch_symbols; the adm_stream_* calls manage streams and launch nothing); each is wrapped on both loaded
libraries and notes (symbol, library) -- nothing more.  SYMBOL_COVERAGE maps every launch symbol to the record kind(s) that replay
it here or to the test that holds it elsewhere, so "every launch" is checked, not assumed.  Records: every adm_conv call is
captured as a copy of its adm_conv_args without the pointers, plus which optional pointers were set (those are flags); the
attention, GroupNorm, token (LayerNorm, GEGLU, quick-GELU, embedding), resample, layout, VAE entry / exit and stride-2 conv2d calls
are captured at the ops level by shape and flags, and so are the classifier heads: the attention pool's four kernels, the
adaptive / spatial / spatial_v2 heads' channel mean, broadcast add, vector activation and vector GroupNorm, and the loss
gradient, and the fp32 embedding path: adm_linear_f32 (time_embed, every emb_layers, the heads' Linear layers) by (n, k, o),
SiLU, the bias / table flags and the operands' alignment, adm_timestep_embedding by (n, dim, max_period) -- their restatements
and bounds are tests/f32_kernels.py's.  The sampler-step kernels (adm_ddim_step, adm_ddpm_step, adm_sd_step, adm_dpm_step) are
not launched by a model evaluation: tests/test_hip_f32_kernels.py holds them.

Restatement: the op in float64 on the operands exactly as the kernel sees them -- 16-bit inputs, weights and residuals; the
GroupNorm affine (+ SiLU) prologue in fp32, rounded once to the 16-bit type T.

Per-element bounds, u = 2^-8 (bf16) or 2^-11 (fp16), ulp_T(v) = 2u * 2^floor(log2 |v|):
  conv       |got - ref| <= ulp_T(|ref|) + [residual / GroupNorm-backward epilogue] ulp_T(|A|) / 2
                            + Σ_k ulp_T(h_k) |w_k| [h_k within PRO_ULPS fp32 ulps of a T rounding midpoint]
                            + (K + ksplit + 2) 2^-24 Σ_k |w_k h_k|
             A = acc + bias is rounded to T before the residual is added (the reference's T-typed add); the third term is the
             c u max_k |w_k h_k| term made exact: only a prologue value whose fp32 computation (fma, approximate exp / rcp on the
             GPU, PRO_ULPS = 8 fp32 ulps of slack) straddles a rounding midpoint can round the other way, by one ulp_T; the last
             term is fp32 accumulation over K products.  fp32 NCHW output: no ulp_T term, a 2^-24 |ref| one instead.
             The last term is the worst case of fp32 summation: on deep convs (K ~ 9216) it reaches a few % of |ref|, ~30 fp16
             ulps, so there the per-element check is loose and a small worst ratio does not mean near-ulp agreement; the Frobenius
             bound below is the tight check on those launches.
  attention  |got - ref| <= ulp_T(|ref|) + C_ATTN u max_j |v_j| + fp32 terms (logits, PV accumulation; fp16: underflow of P)
             C_ATTN = 2: P is rounded to T before the PV product (numerator) and the row sum (denominator) -- u each.
  causal     adm_attention_causal: the same bound with the logits above the diagonal at -inf; the key count and max_j |v_j| are
             taken over the keys j <= query.  Rows >= t of `out` and a guard behind it keep their sentinel.
  attn bwd   dq / dk: ulp_T(|ref|) + 4 u scale Σ_j P_j (|dP_j| + |δ|) |k_j| (resp. |q_i|); dv: ulp_T(|ref|) + 2 u Σ_i P_i |do_i|
             -- P and dS = P (dP - δ) are rounded to T before their products (u each, and dS inherits P's), fp32 terms far below.
  lse        log2-domain log-sum-exp of the scaled logits: |got - ref| <= u / ln 2 + 2^-18 (1 + |ref| + max_j |s_j c|): the row sum
             adds P after its rounding to T (relative u, log2(1 + u) <= u / ln 2), the rest is fp32 exp2 / log2.
  gn_bwd     dx = a dz + k1 (x + e) + k0 (+ add): ulp_T(|ref|) + 2^-20 (|a dz| + |k1 (x + e)| + |k0| + |add|) + |x + e| E1 + E0,
             E1 / E0 the fp32 slab sums' worst case (hw 2^-24 Σ|terms|) carried through k1 / k0.
  gn_affine  y = a x + b against float64 GroupNorm (+ FiLM / + add) of the stored tensor: u / 8 (1 + |y|), well below the
             rounding to T that the consuming conv's prologue applies next.
  "half ulp" below is one round-to-nearest of an fp32 value v to T: |got - ref| <= ulp_T(|ref|) / 2 + |v - ref|; where v and ref
             lie on the two sides of a binade edge the result is the edge itself, within the lower binade's half ulp of ref.
  layernorm  y = ŷ γ + β, ŷ = (x - mean) rstd, two-pass as the kernel: ulp_T(|ref|) / 2 + k rstd |γ| mean|x| + (k + 2^-21) |ŷ γ|
             + 2^-23 |ref|, k = (8 SEGS + 8) 2^-24, SEGS = ceil(c / 512): a lane adds its 8 SEGS values and six butterfly steps
             follow, for the mean (times the fp32 1 / c: k mean|x| on the mean, carried by rstd |γ|) and again for the variance
             (relative k on rstd, with rsqrt, the subtraction and the two multiplies inside 2^-21); 2^-23 |ref| is the final
             multiply-add.  Frobenius <= fro_bound(1, u).  layernorm_f32out: the same without the ulp_T / 2 term, on the rows < t
             of every prompt; the rows >= t are fed NaN and must not be read.
  geglu      v gelu_erf(g) on T values: ulp_T(|ref|) / 2 + SILU_REL (|ref| + |v|), the last term of the fused GEGLU bound.
  quick_gelu a sigmoid(1.702 a): ulp_T(|ref|) / 2 + SILU_REL (1 + |1.702 a|) |ref|: the fp32 product in front of exp2 has a
             relative error 2^-24 of an argument that grows with |a|, and d log sigmoid(z) / dz <= 1.
  clip_embed round_T(tok[ids] + pos[:t]) with the add in fp32, pad rows zero: bitwise.
  resample   'up' / 'stride2' / 'stride2_odd' / 'zero2' without the affine are copies and zeros: bitwise.  'down' is the mean of four taps:
             ulp_T(|ref|) / 2 + 4 x 2^-24 mean|x| (three fp32 adds, an exact 1 / 4).  With the affine the taps are
             s = silu(a x + b): the mean (the tap) of SILU_REL |s| + 2^-23 (|a x| + |b|) is added -- approximate exp / rcp, and
             the fp32 multiply-add in front through silu' <= 1.1.
  nchw_to_nhwc_pad   round_T(x) transposed, pad channels zero: bitwise.
  vae_latent_in      Σ_j w_cj (inv z_j) + b_c: ulp_T(|ref|) / 2 + (e + 3) 2^-24 (Σ_j |w_cj inv z_j| + |b_c|): the product inv z_j, e
             multiply-adds and the bias add.  Pad channels exactly zero.
  vae_image_out      clamp((x + 1) / 2, 0, 1) in fp32 and trunc(255 unit): bitwise.
  conv2d     the UNets' stride-2 convs on adm_conv2d: inception_replay's restatement, bound and comparison, imported.
  The classifier heads, e = 2^-24 (one fp32 add or multiply, relative to the summed magnitudes); SILU_REL also stands for one
             library expf / logf / rsqrtf / sqrtf / division; F32_MIN = 2^-126 is added where a result may leave fp32's normal
             range.  E_s = 2 e (|a h| + |b|) + SILU_REL (1 + |z|) |s| is the error of s = adm_silu(z), z = a h + b: the
             multiply-add in front (SiLU' <= 1.1) and an exp2 whose argument carries a relative e, so a relative |z| e on it.
  pool_prep  rows 1 + p: ulp_T(|ref|) / 2 + E_s + e (|s| + |pos|); row 0: ulp_T(|ref|) / 2 + mean_p E_s + (hw + 2) e mean_p |s|
             + SILU_REL |mean s| + e (|mean s| + |pos_0|) -- hw sequential adds, the division by hw, the add of pos.  Rows
             hw + 1 .. tpad: exactly zero.
  pool_attn_fwd   logit_j: δ_j = (d + c1) e Σ |q k_j| / sqrt(d), c1 = 4 (d multiply-adds, the product with the scale, rsqrtf
             of d within an ulp = 2 e); w_j relative: 2 max_j δ_j (its own logit and the sum's) + e (span_j + Σ w span), span_j
             = max logit - logit_j (the subtraction in front of expf, for w_j and for the sum) + 3 SILU_REL (expf of w_j, of
             the sum's terms, the division) + (ceil(T / 64) + 7) e (a lane's adds, six butterfly steps, of positive terms) --
             plus F32_MIN: a weight below fp32's range is 0.  wts[t:tpad] exactly zero.  a0: Σ_s bound(w_s) |v_s| +
             (T + c2) e Σ_s w_s |v_s|, c2 = 1: T sequential multiply-adds.
  pool_attn_bwd   on the stored fp32 weights w.  dw_s = Σ_j da_j v_sj: E_dw = (d + 1) e Σ_j |da_j v_sj|; δ = Σ_s w_s dw_s:
             E_δ = Σ_s w_s E_dw_s + (ceil(T / 64) + 7) e Σ_s w_s |dw_s|; dlogit_s = w_s (dw_s - δ) / sqrt(d): E_dl =
             w_s / sqrt(d) (E_dw_s + E_δ + 5 e (|dw_s| + |δ|)) -- the subtraction cancels, so its operands' errors and
             roundings are carried at |dw| + |δ|.  dK = round_T(dlogit q): ulp_T(|ref|) / 2 + |q| E_dl + e |ref|; dV =
             round_T(w da): ulp_T(|ref|) / 2 + e |ref|; dQ row 0 = round_T(Σ_s dlogit_s k_s): ulp_T(|ref|) / 2 +
             Σ_s E_dl_s |k_s| + (T + 1) e Σ_s |dlogit_s k_s|.  dQ rows > 0 and every row >= T: exactly zero.
  pool_prep_bwd   round_T(dtok[1 + p] + dtok[0] / hw): ulp_T(|ref|) / 2 + SILU_REL |dtok_0 / hw| + e (|dtok[1 + p]| + |dtok_0 / hw|).
  channel_mean    fp32: (ceil(hw / 4) + 3) e mean |v| (a lane's adds, three adds of the four lanes) + SILU_REL |ref| (the
             division) + mean E_s with the affine.
  bcast_add  without add: round_T of the fp32 product v scale, bitwise.  With add: ulp_T(|ref|) / 2 + e (2 |v scale| + |add|).
  vec_act    SiLU: SILU_REL |ref| + F32_MIN (expf, an add, a division; below z = -88.7 expf overflows and the result is -0).
             SiLU': dy s (1 + z (1 - s)): SILU_REL |dy| s (1 + |z|) + F32_MIN -- 1 - s cancels for large z, absolute e there.
             ReLU and ReLU': exact, ReLU'(0) = 0.  gauss_std / gauss_logvar (modes 3 / 4, the KL-f8 posterior's): the restatements
             and bounds of tests/f32_vae_kernels.py; the clamped log-variance is compared bitwise.
  vec_gn     k = (ceil(cpg / 8) + 3) e, cpg = c / 32: a lane's adds and three butterfly steps.  E_m = k mean|x| + SILU_REL
             |mean|; d = x - mean carries E_m + e |d|, so E_v = 2 mean|d| E_m + E_m^2 + (k + 4 e + SILU_REL) var and rstd is
             relative rel_r = E_v / (2 (var + eps)) + e + 2 SILU_REL (the add of eps, sqrtf, the division).  y: |γ| rstd E_m +
             |γ d rstd| (rel_r + 4 e) + e |y|.  mean: E_m; rstd: rstd rel_r.  cpg = 1: y = β exactly.
  vec_gn_bwd on the stored (mean, rstd): g = γ dz, xh = (x - mean) rstd, s1 = mean g, s2 = mean g xh: E_1 = (k + e) mean|g| +
             SILU_REL |s1|, E_2 = (k + 4 e) mean|g xh| + SILU_REL |s2|; dx = rstd (g - s1 - xh s2): rstd (E_1 + |xh| E_2 +
             4 e (|g| + |s1| + |xh s2|)) + e |ref|.  cpg = 1: dx = 0 exactly.
  logsoftmax_grad   softmax_i relative: e dist_i (dist = max - logit, the subtraction) + 3 SILU_REL (expf, the sum's expf,
             the division) + (ceil(k / 256) + 8) e (a thread's adds, the eight steps of the block tree) + e Σ softmax dist;
             dl = scale (onehot - softmax): |scale| (rel softmax + F32_MIN) + 2 e |ref|.  logp_sel = l_y - max - logf(sum):
             e dist_y + SILU_REL (1 + |log sum|) + the sum's relative error + 2 e |ref|.
  grad_add   round_T(a + s b), s = 1 or an exact 1 / 4: ulp_T(|ref|) / 2 + e (|a| + |s b|).
  linear_f32, timestep_embedding   fp32 throughout: f32_kernels.linear_restate / timestep_restate (derived in that module's docstring).
  stem_conv3x3   adm_stem_conv3x3, the KL-f8 encoder's conv_in from the fp32 NCHW image: f32_kernels.stem_restate (derived there).
  head       the KL-f8 encoder's head as a composite (Encoder._head, both routes; head_restate): float64 GroupNorm + SiLU of the
             stored map, s = SiLU(z), z = γ ŷ + β, ŷ = (h - mean) rstd, rounded once to T; then the pad-1 3x3 conv of the unpadded
             map with round_T weights and an fp32 bias, under the conv bound above for fp32 NCHW output.  The midpoint-straddle
             term is taken with the window the composite needs (head_window): the kernels form z = a h + b from fp32 statistics,
             which the GroupNorm replay keeps within 2^-20 (|mean| + 1 / rstd) of the mean and 2^-20 rstd of rstd: through γ rstd
             and γ ŷ that is 2^-20 |γ| (|mean| rstd + 1 + |ŷ|); the fp32 roundings of a = γ rstd, of mean a, of b and of the
             multiply-add add 2^-22 |γ| (|mean| rstd + |ŷ|) + 2^-23 (|β| + |z|).  So |z_kernel - z| <= dz = (2^-20 + 2^-22) |γ|
             (|mean| rstd + 1 + |ŷ|) + 2^-23 (|β| + |z|), and s moves by at most 1.1 dz (SiLU' <= 1.1) + PRO_ULPS 2^-23 |s| (the
             conv bound's own slack for the approximate exp / rcp).  An s within that window of a rounding midpoint may round the
             other way: its step to the other T neighbour times |w| enters the bound.
  folded     Encoder.folded_head: W' = wq Wout per tap and b' = wq b_out + bq in fp32, W' then rounded to T.  The reference is
  head       quant_conv(conv_out(act)) in float64 from the unfolded fp32 weights, W'_64 = Σ_m wq_m Wout_m.  An fp32 dot product of
             length m (torch's einsum / matmul, any order, with or without fma) is within (m + 1) 2^-24 Σ_m |wq_m Wout_mk| of W'_64
             to first order (m products, m - 1 adds, one of each per term: m + 1 covers every order); rounding that to T adds
             ulp_T(|W'_k|) / 2 (at a binade edge the result is the edge itself, inside the lower binade's half ulp).  So the conv
             bound widens by Σ_k |act_k| dW_k, dW_k = ulp_T(|W'_k|) / 2 + (m + 1) 2^-24 Σ_m |wq_m Wout_mk|, and its magnitude sums
             take |W'_k| + dW_k.  The bias is a dot product of length m plus the add of bq: (m + 2) 2^-24 (Σ_m |wq_m b_out_m| + |bq|).
  Frobenius  ||got - ref|| / ||ref|| <= FRO_U u sqrt(r), FRO_U = 0.6: one rounding to T has an RMS relative error of at most
             u / sqrt(3) ~ 0.58 u; r roundings in sequence (A, then A + residual; dz, then dz SiLU'; P, then the output) add in
             quadrature.

Elementwise and row-wise records are compared on every element; above 2^25 elements, on every element of the first, the last
and one seeded image (a condition, not a tolerance: these kernels index by flat element, so no tile position goes unvisited).
"""
from __future__ import annotations

import math

import torch

from f32_kernels import linear_path, linear_restate, stem_restate, timestep_restate   # noqa: F401  (the fp32 record kinds of the embedding path, the direct stem)
from f32_vae_kernels import GAUSS_SPECIALS, gauss_logvar_restate, gauss_std_restate   # noqa: F401  (adm_vec_act modes 3 / 4)

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
KIND_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
KIND_OF_DTYPE = {v: k for k, v in KIND_DTYPE.items()}
PRO_ULPS = 8
C_ATTN = 2.0
FRO_U = 0.6
SILU_REL = 2.0 ** -20   # fp32 SiLU' / GELU on the accumulators: approximate exp / rcp / erf, a few fp32 ulps


def fro_bound(roundings: int, u: float) -> float:
    return FRO_U * u * math.sqrt(roundings)


def conv_roundings(d: dict) -> int:
    """Roundings to T in sequence on a conv's output: one, two where A is rounded before the residual / SiLU' epilogue."""
    if d["out_mode"] == 1:
        return 1
    return 2 if (d["has_res"] or d["prologue"] == 3) else 1


CONV_PTR_FLAGS = ("in1", "res", "aff_a", "fold0", "fold1", "out_stats", "w_packed32", "ws")
_CONV_SKIP = {"in0", "in1", "w_packed", "bias", "aff_a", "aff_b", "res", "out", "out_stats", "w_packed32", "ws", "fold0", "fold1"}


# ------------------------------------------------------------------ recording
def conv_record(kind: str, a) -> tuple:
    """Hashable record of one adm_conv_args: every non-pointer field, and which optional pointers were non-null."""
    d = {name: getattr(a, name) for name, _ in a._fields_ if name not in _CONV_SKIP}
    d["out_scale"] = float(a.out_scale)
    for f in CONV_PTR_FLAGS:
        d["has_" + f] = bool(getattr(a, f))
    return ("conv", kind) + tuple(sorted(d.items()))


def record_dict(rec: tuple) -> dict:
    return dict(rec[2:])


def launch_symbols() -> list:
    """The exported symbols that launch: the last argument is the stream pointer.  The adm_stream_* calls (create / resize /
    destroy / probe a stream) end in a pointer too; they are stream management, not launches."""
    from autodiffusion_amd import _lib
    return [name for name, (_, args) in _lib.SIGNATURES.items()
            if args and args[-1] is _lib._P and not name.startswith("adm_stream_")]


def _e(test: str) -> tuple:
    return ("elsewhere", test)


# launch symbol -> the record kinds that replay it here, or ("elsewhere", "tests/<file>.py::<test>") for what stays where it is:
# the weight packers (every conv replay compares against round_t(w), so a mis-packed weight fails there too), the sampler steps
# (tests/test_hip_f32_kernels.py), and the evaluation-side kernels of the Inception replay and the FID /
# precision-recall tests.
SYMBOL_COVERAGE = {
    "adm_conv": ("conv",),
    "adm_attention_lse": ("attention",),
    "adm_attention_1h512": ("attention",),
    "adm_attention_cross": ("attention_cross",),
    "adm_attention_bwd": ("attention_bwd",),
    "adm_gn_partial": ("gn_affine",),
    "adm_gn_finalize": ("gn_affine",),
    "adm_gn_finalize2": ("gn_affine",),
    "adm_gn_finalize_add": ("gn_affine",),
    "adm_gn_bwd_partial": ("gn_bwd",),
    "adm_gn_bwd_finalize": ("gn_bwd",),
    "adm_gn_bwd_apply": ("gn_bwd",),
    "adm_layernorm": ("layernorm",),
    "adm_layernorm_f32out": ("layernorm_f32out",),
    "adm_geglu": ("geglu",),
    "adm_quick_gelu": ("quick_gelu",),
    "adm_attention_causal": ("attention_causal",),
    "adm_clip_embed": ("clip_embed",),
    "adm_resample": ("resample",),
    "adm_nchw_to_nhwc_pad": ("nchw_to_nhwc_pad",),
    "adm_vae_latent_in": ("vae_latent_in",),
    "adm_vae_image_out": ("vae_image_out",),
    "adm_conv2d": ("conv2d",),
    # the classifier's heads: the attention pool, the fp32 vector kernels of the other three, the loss gradient
    "adm_pool_prep": ("pool_prep",),
    "adm_pool_attn_fwd": ("pool_attn_fwd",),
    "adm_pool_attn_bwd": ("pool_attn_bwd",),
    "adm_pool_prep_bwd": ("pool_prep_bwd",),
    "adm_channel_mean": ("channel_mean",),
    "adm_bcast_add": ("bcast_add",),
    "adm_vec_act": ("vec_act",),
    "adm_vec_gn": ("vec_gn",),
    "adm_vec_gn_bwd": ("vec_gn_bwd",),
    "adm_logsoftmax_grad": ("logsoftmax_grad",),
    # no caller in the package: held by its direct test
    "adm_grad_add": _e("tests/test_hip_launch_replay.py::test_grad_add_at_edges"),
    # fp32 embedding path: record kinds
    "adm_linear_f32": ("linear_f32",),
    "adm_timestep_embedding": ("timestep_embedding",),
    # the direct stem is the KL-f8 encoder's conv_in (3 -> 128 on the image): a record kind, replayed by
    # tests/test_hip_vae_encoder_replay.py at the shapes the model launches; tests/test_hip_f32_kernels.py::test_stem_conv_at_edges
    # holds its edge shapes
    "adm_stem_conv3x3": ("stem_conv3x3",),
    # weight packers
    "adm_pack_conv_weight": _e("tests/test_hip_kernels.py::test_conv_fused"),
    "adm_pack_conv_weight32": _e("tests/test_hip_kernels.py::test_conv_fused"),
    "adm_pack_conv_weight_bwd": _e("tests/test_hip_classifier.py::test_conv_backward_data_weights"),
    "adm_pack_conv2d_weight": _e("tests/test_hip_inception_replay.py::test_conv_launches_match_float64"),
    # sampler steps: not launched by a model evaluation
    "adm_ddim_step": _e("tests/test_hip_f32_kernels.py::test_sampler_step_flag_product"),
    "adm_ddpm_step": _e("tests/test_hip_f32_kernels.py::test_sampler_step_flag_product"),
    "adm_pack_u8_nhwc": _e("tests/test_hip_f32_kernels.py::test_pack_u8_bitwise"),
    "adm_sd_step": _e("tests/test_hip_f32_kernels.py::test_sd_step_every_operand_subset"),
    "adm_dpm_step": _e("tests/test_hip_f32_kernels.py::test_dpm_step_every_operand_subset"),
    # evaluation side (the shapes the extractor launches are held by the tests named here; adm_conv2d, adm_pool2d,
    # adm_global_avgpool_f32 and adm_resize_bilinear at the shapes no model launches, and their refusals, besides by
    # tests/test_hip_conv2d_envelope.py::test_conv2d_envelope)
    "adm_pool2d": _e("tests/test_hip_inception_replay.py::test_pool_launches_match_float64"),
    "adm_global_avgpool_f32": _e("tests/test_hip_inception_replay.py::test_global_avgpool_launches_match_float64"),
    "adm_resize_bilinear": _e("tests/test_hip_inception_replay.py::test_resize_launches_match_float64"),
    "adm_fid_accumulate": _e("tests/test_fid.py::test_gram_kernel_ragged_shapes_and_symmetry"),
    "adm_knn_smallest": _e("tests/test_hip_f32_kernels.py::test_knn_smallest_at_narrow_widths"),
    "adm_knn_cover": _e("tests/test_hip_f32_kernels.py::test_knn_cover_at_narrow_widths"),
    # no caller in the package (ops.attention always asks adm_attention_lse): only its export is held
    "adm_attention": _e("tests/test_cabi.py::test_library_loads_and_exports_every_symbol"),
}


def coverage_gaps(census, records, replayed) -> list:
    """What the coverage guard reports: census symbols missing from SYMBOL_COVERAGE, and symbols mapped to record kinds of which
    none was recorded (on the library that made the call) or which the replay does not take."""
    have = {(r[0], r[1]) for r in records}
    gaps = []
    for sym, kind in sorted(census):
        cov = SYMBOL_COVERAGE.get(sym)
        if cov is None:
            gaps.append(f"{sym} ({kind}) is launched but has no entry in SYMBOL_COVERAGE")
        elif cov[0] != "elsewhere":
            if not any((k, kind) in have for k in cov):
                gaps.append(f"{sym} ({kind}) was launched but no {' / '.join(cov)} record was taken")
            if not set(cov) <= set(replayed):
                gaps.append(f"{sym}: record kinds {sorted(set(cov) - set(replayed))} are not replayed")
    return gaps


def kind_of(t) -> str:
    return "f16" if t.dtype == torch.float16 else "bf16"


RESAMPLE_MODES = {"down": 1, "up": 2, "stride2": 3, "zero2": 4, "stride2_odd": 5}


class Recorder:
    """Patches (through pytest's monkeypatch) every launch symbol on both libraries -- the census, and adm_conv's record -- and
    the attention / GroupNorm / token / resample / layout / VAE / conv2d / classifier-head / embedding wrappers of ops (the other
    records)."""

    def __init__(self, monkeypatch):
        from autodiffusion_amd import _lib, ops
        self.records = set()
        self.counts = {}
        self.orig = {}
        self.census = set()
        self._cin = {}
        for kind in ("bf16", "f16"):
            lib = _lib.load(kind)
            fn = lib.adm_conv
            self.orig[kind] = fn

            def wrapped(args, stream, _fn=fn, _kind=kind):
                a = args._obj if hasattr(args, "_obj") else args.contents
                self.census.add(("adm_conv", _kind))
                self._add(conv_record(_kind, _lib.ConvArgs.from_buffer_copy(a)))
                return _fn(args, stream)
            monkeypatch.setattr(lib, "adm_conv", wrapped)
            for name in launch_symbols():
                if name == "adm_conv":
                    continue

                def noted(*args, _fn=getattr(lib, name), _key=(name, kind)):
                    self.census.add(_key)
                    return _fn(*args)
                monkeypatch.setattr(lib, name, noted)

        o_att, o_cross, o_bwd, o_gn, o_gnb = ops.attention, ops.attention_cross, ops.attention_bwd, ops.gn_affine, ops.gn_bwd

        def attention(qkv, heads, new_order, want_lse=False):
            n, t, c3 = qkv.shape
            self._add(("attention", kind_of(qkv), n, t, c3, heads, bool(new_order), bool(want_lse)))
            return o_att(qkv, heads, new_order, want_lse)

        def attention_cross(q, kv, heads, d, tk, scale, q_cols=None):
            self._add(("attention_cross", kind_of(q), q.shape[0], q.shape[1], q.stride(1), kv.shape[1], kv.stride(1), tk, heads, d,
                       float(scale)))
            return o_cross(q, kv, heads, d, tk, scale, q_cols)

        def attention_bwd(qkv, out, dout, lse, heads, new_order):
            n, t, c3 = qkv.shape
            self._add(("attention_bwd", kind_of(qkv), n, t, c3, heads, bool(new_order)))
            return o_bwd(qkv, out, dout, lse, heads, new_order)

        def gn_affine(x0, gamma, beta, x1=None, film=None, film_stride=0, partial=None, want_stats=False, eps=None, add=None):
            n, h, w, c0 = x0.shape
            self._add(("gn_affine", kind_of(x0), n, h, w, c0, 0 if x1 is None else x1.shape[3], film is not None, add is not None,
                       getattr(x0, "_adm_stats", None) is not None, bool(want_stats), float(ops.GN_EPS if eps is None else eps)))
            return o_gn(x0, gamma, beta, x1, film, film_stride, partial, want_stats, eps, add)

        def gn_bwd(x, dy, aff, stats, silu, dy_half=False, add=None, add_half=False, partial=None, norm_add=None):
            n, h, w, c = x.shape
            self._add(("gn_bwd", kind_of(x), n, h, w, c, bool(silu), bool(dy_half), add is not None, bool(add_half),
                       partial is not None, norm_add is not None))
            return o_gnb(x, dy, aff, stats, silu, dy_half, add, add_half, partial, norm_add)

        o_ln, o_lnf, o_gg, o_qg, o_cau, o_emb = (ops.layernorm, ops.layernorm_f32out, ops.geglu, ops.quick_gelu, ops.attention_causal,
                                                 ops.clip_embed)
        o_res, o_pad, o_lat, o_img, o_c2d = ops.resample, ops.nchw_to_nhwc_pad, ops.vae_latent_in, ops.vae_image_out, ops.conv2d
        o_stem = ops.stem_conv3x3

        def stem_conv3x3(x_nchw, w, b, dtype=torch.bfloat16):
            n, cin, h, wd = x_nchw.shape
            self._add(("stem_conv3x3", KIND_OF_DTYPE[dtype], n, cin, h, wd, w.shape[0]))
            return o_stem(x_nchw, w, b, dtype)

        def layernorm(x, gamma, beta, eps=1e-5):
            c = x.shape[-1]
            self._add(("layernorm", kind_of(x), x.numel() // c, c, float(eps)))
            return o_ln(x, gamma, beta, eps)

        def layernorm_f32out(x, t, gamma, beta, eps=1e-5):
            n, pitch, c = x.shape
            self._add(("layernorm_f32out", kind_of(x), n, int(t), pitch, c, float(eps)))
            return o_lnf(x, t, gamma, beta, eps)

        def geglu(u):
            inner = u.shape[-1] // 2
            self._add(("geglu", kind_of(u), u.numel() // (2 * inner), inner))
            return o_gg(u)

        def quick_gelu(u):
            inner = u.shape[-1]
            self._add(("quick_gelu", kind_of(u), u.numel() // inner, inner))
            return o_qg(u)

        def attention_causal(qkv, heads, t=None, out=None):
            n, pitch, _ = qkv.shape
            self._add(("attention_causal", kind_of(qkv), n, pitch if t is None else int(t), pitch, heads))
            return o_cau(qkv, heads, t, out)

        def clip_embed(ids, tok, pos, pitch, dtype=torch.bfloat16):
            self._add(("clip_embed", KIND_OF_DTYPE[dtype], ids.shape[0], ids.shape[1], int(pitch), tok.shape[1], tok.shape[0], pos.shape[0]))
            return o_emb(ids, tok, pos, pitch, dtype)

        def resample(x, mode, aff=None):
            n, h, w, c = x.shape
            self._add(("resample", kind_of(x), n, h, w, c, RESAMPLE_MODES[mode], aff is not None))
            return o_res(x, mode, aff)

        def nchw_to_nhwc_pad(x_nchw, cpad=32, dtype=torch.bfloat16):
            n, c, h, w = x_nchw.shape
            self._add(("nchw_to_nhwc_pad", KIND_OF_DTYPE[dtype], n, c, h, w, int(cpad)))
            return o_pad(x_nchw, cpad, dtype)

        def vae_latent_in(z, w, b, inv_scale=1.0, dtype=torch.bfloat16):
            n, e, h, wd = z.shape
            self._add(("vae_latent_in", KIND_OF_DTYPE[dtype], n, w.shape[0], e, h, wd))
            return o_lat(z, w, b, inv_scale, dtype)

        def vae_image_out(x, want_unit=True, want_u8=False, unit_out=None):
            n, _, h, w = x.shape   # one fp32 kernel, launched from the bf16 library whatever the torso
            self._add(("vae_image_out", "bf16", n, h, w, bool(want_unit) or unit_out is not None, bool(want_u8)))
            return o_img(x, want_unit, want_u8, unit_out)

        def conv2d(x, w_packed, bias, kh, kw, stride=1, pad=(0, 0), relu=True, out=None):
            import inception_replay as ir
            self._add(ir.conv2d_record(self._cin, x, w_packed, bias, kh, kw, stride, pad, relu, out))
            return o_c2d(x, w_packed, bias, kh, kw, stride, pad, relu, out)

        o_pp, o_pf, o_pb, o_ppb = ops.pool_prep, ops.pool_attn_fwd, ops.pool_attn_bwd, ops.pool_prep_bwd
        o_cm, o_ba, o_va, o_vg, o_vgb, o_lsg = ops.channel_mean, ops.bcast_add, ops.vec_act, ops.vec_gn, ops.vec_gn_bwd, ops.logsoftmax_grad

        def pool_prep(h, aff, pos, tpad):
            n, hh, ww, c = h.shape
            self._add(("pool_prep", kind_of(h), n, hh * ww, c, int(tpad)))
            return o_pp(h, aff, pos, tpad)

        def pool_attn_fwd(qkv, t, heads):
            n, tpad, c3 = qkv.shape
            self._add(("pool_attn_fwd", kind_of(qkv), n, int(t), tpad, heads, c3 // 3 // heads))
            return o_pf(qkv, t, heads)

        def pool_attn_bwd(qkv, wts, da0, t, heads):
            n, tpad, c3 = qkv.shape
            self._add(("pool_attn_bwd", kind_of(qkv), n, int(t), tpad, heads, c3 // 3 // heads))
            return o_pb(qkv, wts, da0, t, heads)

        def pool_prep_bwd(dtok, hh, ww):
            n, tpad, c = dtok.shape
            self._add(("pool_prep_bwd", kind_of(dtok), n, hh * ww, c, tpad))
            return o_ppb(dtok, hh, ww)

        def channel_mean(h, aff=None, out=None, col=0):
            n, hh, ww, c = h.shape
            self._add(("channel_mean", kind_of(h), n, hh * ww, c, aff is not None, int(col) if out is not None else 0,
                       c if out is None else out.shape[1]))
            return o_cm(h, aff, out, col)

        def bcast_add(v, shape, dtype, scale, add=None, col=0):
            n, hh, ww, c = shape
            self._add(("bcast_add", KIND_OF_DTYPE[dtype], n, hh * ww, c, add is not None, int(col), v.shape[1]))
            return o_ba(v, shape, dtype, scale, add, col)

        # the four below are fp32 kernels that ops launches from the bf16 library whatever the torso
        def vec_act(x, mode, dy=None):
            self._add(("vec_act", "bf16", x.numel(), VEC_ACT_MODES[mode], dy is not None))
            return o_va(x, mode, dy)

        def vec_gn(x, gamma, beta, eps=ops.GN_EPS):
            self._add(("vec_gn", "bf16", x.shape[0], x.shape[1], float(eps)))
            return o_vg(x, gamma, beta, eps)

        def vec_gn_bwd(x, gamma, stats, dz):
            self._add(("vec_gn_bwd", "bf16", x.shape[0], x.shape[1]))
            return o_vgb(x, gamma, stats, dz)

        def logsoftmax_grad(logits, y, scale):
            self._add(("logsoftmax_grad", "bf16", logits.shape[0], logits.shape[1], float(scale)))
            return o_lsg(logits, y, scale)

        o_lin, o_temb = ops.linear_f32, ops.timestep_embedding

        # fp32 kernels that ops launches from the bf16 library whatever the torso
        def linear_f32(x, w, b=None, silu_in=False, table=None, idx=None, out=None):
            aligned = x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
            self._add(("linear_f32", "bf16", x.shape[0], x.shape[1], w.shape[0], bool(silu_in), b is not None, table is not None, aligned))
            return o_lin(x, w, b, silu_in, table, idx, out)

        def timestep_embedding(t, dim, max_period=10000.0):
            self._add(("timestep_embedding", "bf16", t.shape[0], int(dim), float(max_period)))
            return o_temb(t, dim, max_period)

        for name, fn in (("stem_conv3x3", stem_conv3x3), ("linear_f32", linear_f32), ("timestep_embedding", timestep_embedding), ("attention", attention), ("attention_cross", attention_cross), ("attention_bwd", attention_bwd),
                         ("gn_affine", gn_affine), ("gn_bwd", gn_bwd), ("layernorm", layernorm), ("layernorm_f32out", layernorm_f32out),
                         ("geglu", geglu), ("quick_gelu", quick_gelu), ("attention_causal", attention_causal), ("clip_embed", clip_embed),
                         ("resample", resample), ("nchw_to_nhwc_pad", nchw_to_nhwc_pad), ("vae_latent_in", vae_latent_in),
                         ("vae_image_out", vae_image_out), ("conv2d", conv2d), ("pool_prep", pool_prep),
                         ("pool_attn_fwd", pool_attn_fwd), ("pool_attn_bwd", pool_attn_bwd), ("pool_prep_bwd", pool_prep_bwd),
                         ("channel_mean", channel_mean), ("bcast_add", bcast_add), ("vec_act", vec_act), ("vec_gn", vec_gn),
                         ("vec_gn_bwd", vec_gn_bwd), ("logsoftmax_grad", logsoftmax_grad)):
            monkeypatch.setattr(ops, name, fn)

    def _add(self, rec):
        self.records.add(rec)
        self.counts[rec[0]] = self.counts.get(rec[0], 0) + 1


# ------------------------------------------------------------------ families (coverage guard)
def families(rec: tuple) -> set:
    """The (library, family) labels a record belongs to."""
    kind, op = rec[1], rec[0]
    out = set()
    if op == "conv":
        d = record_dict(rec)
        out.add(f"variant {d['variant']}")
        if d["ksplit"] > 1:
            out.add("ksplit > 1")
        if d["up_phase"] == 5:
            out.add("up_phase 5")
        if d["has_fold0"]:
            out.add("fold")
        if d["prologue"] == 3:
            out.add("prologue 3")
        if d["geglu"]:
            out.add("geglu")
        if d["out_mode"] == 1:
            out.add("out_mode 1 + out_scale" if d["out_scale"] != 0.0 else "out_mode 1")
        if d["h"] != d["w"]:
            out.add("non-square map")   # the CLIP text transformer's 8x16 token map
        else:
            out.add("8x8 map" if d["h"] * d["w"] <= 64 else ">= 16x16 map")
    elif op == "attention":
        _, _, n, t, c3, heads, new_order, lse = rec
        out.add(f"attention d {c3 // 3 // heads}")
    elif op == "attention_cross":
        _, _, n, tq, qs, rows, kvs, tk, heads, d, scale = rec
        out.add(f"attention_cross d {d} ({'self' if tk == tq and qs == kvs else 'cross'})")
    elif op == "linear_f32":
        _, _, n, k, o, silu_in, has_bias, has_table, aligned = rec
        out.update({op, f"linear_f32 {linear_path(k, aligned)}"})   # which of the three kernels ran: by k and alignment alone
        if has_table:
            out.add("linear_f32 table")
    else:
        out.add(op)
    return {(kind, f) for f in out}


# variant 7 (the 32x32x16 kernel) needs w_packed32, which no shipped model passes: tests/test_hip_kernels.py covers it
REQUIRED_FAMILIES = (["variant 3", "variant 5", "variant 6", "variant 10", "ksplit > 1", "up_phase 5", "fold",
                      "prologue 3", "geglu", "out_mode 1", "out_mode 1 + out_scale", "8x8 map", ">= 16x16 map"]
                     + [f"attention d {d}" for d in (64, 128, 192, 256)]
                     + [f"attention_cross d {d} ({k})" for d in (48, 80, 160) for k in ("self", "cross")]
                     + ["attention_bwd", "gn_bwd"]
                     + ["attention d 512", "non-square map"]
                     + ["layernorm", "layernorm_f32out", "geglu", "quick_gelu", "attention_causal", "clip_embed", "resample",
                        "nchw_to_nhwc_pad", "vae_latent_in", "vae_image_out", "conv2d"])
# families one library alone reaches: the 2^10 gradient scale is the fp16 classifier's; adm_vae_image_out, the vector kernels of
# the classifier heads and the loss gradient are fp32 kernels that ops launches from the bf16 library whatever the torso
ONE_LIBRARY_FAMILIES = {"out_mode 1 + out_scale": "f16", "vae_image_out": "bf16", "vec_act": "bf16", "vec_gn": "bf16",
                        "vec_gn_bwd": "bf16", "logsoftmax_grad": "bf16"}
TOKEN_KINDS = ("layernorm", "layernorm_f32out", "geglu", "quick_gelu", "attention_causal", "clip_embed", "resample",
               "nchw_to_nhwc_pad", "vae_latent_in", "vae_image_out", "conv2d")
# the classifier heads: the attention pool (every shipped classifier), the adaptive / spatial / spatial_v2 heads, the loss gradient
HEAD_KINDS = ("pool_prep", "pool_attn_fwd", "pool_attn_bwd", "pool_prep_bwd", "channel_mean", "bcast_add", "vec_act", "vec_gn",
              "vec_gn_bwd", "logsoftmax_grad")
NEW_KINDS = TOKEN_KINDS + HEAD_KINDS
REQUIRED_FAMILIES += list(HEAD_KINDS)
# the fp32 embedding path: the two kinds, the linear kernels the models reach -- the matrix pipe (k % 16 == 0: time_embed, every
# emb_layers) and the GEMV (k % 4 == 0, k % 16 != 0: the attention pool's 1000-wide backward projection); no model reaches the
# 64x64 tile kernel (k % 4 != 0, or misaligned operands) -- and the label table's gather-add
EMBED_KINDS = ("linear_f32", "timestep_embedding")
EMBED_FAMILIES = EMBED_KINDS + ("linear_f32 mfma", "linear_f32 gemv", "linear_f32 table")
REQUIRED_FAMILIES += list(EMBED_FAMILIES)
ONE_LIBRARY_FAMILIES.update({f: "bf16" for f in EMBED_FAMILIES})
# the KL-f8 encoder's own kind: recorded and replayed by tests/test_hip_vae_encoder_replay.py, whose guard asserts its presence --
# not a required family of the big recording above, which does not run the encoder
ENCODER_KINDS = ("stem_conv3x3",)
REPLAYED = {"conv", "attention", "attention_cross", "attention_bwd", "gn_bwd", "gn_affine"} | set(NEW_KINDS) | set(EMBED_KINDS) | set(ENCODER_KINDS)


def missing_families(records) -> list:
    """The (library, family) pairs of REQUIRED_FAMILIES that no record belongs to."""
    fams = set()
    for r in records:
        fams |= families(r)
    return [(k, f) for k in ("bf16", "f16") for f in REQUIRED_FAMILIES
            if (k, f) not in fams and ONE_LIBRARY_FAMILIES.get(f, k) == k]


# ------------------------------------------------------------------ arithmetic helpers
def round_t(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(dtype).to(x.dtype)


def ulp_t(v: torch.Tensor, dtype) -> torch.Tensor:
    """One unit in the last place of T at |v| (float64); fp16's subnormal spacing 2^-24 below 2^-14."""
    v = v.abs().double()
    _, e = torch.frexp(v)
    ul = torch.ldexp(torch.full_like(v, 2.0 * U[dtype]), (e - 1).to(torch.int32))
    floor = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    return torch.where(v == 0, torch.full_like(v, floor), ul.clamp_min(floor))


def prologue(x32: torch.Tensor, a32, b32, mode: int, dtype):
    """fp32 GroupNorm affine (+ SiLU) as the kernel's prologue computes it, rounded once to T; also the rounding-risk tensor: the
    step to the other T neighbour where the fp32 value lies within PRO_ULPS fp32 ulps of a T rounding midpoint, else 0."""
    if mode == 0:
        return x32, torch.zeros_like(x32)
    z = torch.addcmul(b32, a32, x32)
    if mode == 2:
        z = z * torch.sigmoid(z)
    r = round_t(z, dtype)
    # perturb by the slack and see whether the rounding moves (at a binade boundary the step below is half the step above)
    dz = PRO_ULPS * 2.0 ** -23 * z.abs()
    risk = torch.maximum((round_t(z - dz, dtype) - r).abs(), (round_t(z + dz, dtype) - r).abs())
    return r, risk


def sample_pixels(n: int, h: int, w: int, seed: int, extra: int = 16):
    """Output pixels (img, y, x) to restate: all of them on maps of <= 256 pixels; else the four corners of every 16x16
    (8x8 below 16) output tile of every image plus `extra` seeded random pixels per image."""
    if h * w <= 256:
        img, y, x = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing="ij")
        return img.reshape(-1), y.reshape(-1), x.reshape(-1)
    tile = 16 if h >= 16 and w >= 16 else 8

    def corners(size):
        s = set()
        for t0 in range(0, size, tile):
            s.update((t0, min(size, t0 + tile) - 1))
        return torch.tensor(sorted(s))
    cy, cx = corners(h), corners(w)
    gy, gx = torch.meshgrid(cy, cx, indexing="ij")
    gy, gx = gy.reshape(-1), gx.reshape(-1)
    g = torch.Generator().manual_seed(seed)
    ry, rx = torch.randint(0, h, (n, extra), generator=g), torch.randint(0, w, (n, extra), generator=g)
    img = torch.cat([torch.arange(n).repeat_interleave(gy.numel()), torch.arange(n).repeat_interleave(extra)])
    y = torch.cat([gy.repeat(n), ry.reshape(-1)])
    x = torch.cat([gx.repeat(n), rx.reshape(-1)])
    return img, y, x


# ------------------------------------------------------------------ conv restatement
def conv_restate(d: dict, dtype, t: dict, img, oy, ox):
    """float64 restatement of one adm_conv launch at output pixels (img, oy, ox) -> (ref [P, cout_out], bound [P, cout_out]).

    d: the record's fields; t: the operands as float32 tensors holding T values (x0, x1, a, b, w, w1, f0, f1, bias, res,
    gnb_a, gnb_b): w is [cout, cin, k, k] -- for up_phase 5 the [4, cout, cin, 3, 3] T-rounded phase weights -- and w1 the
    folded skip connection's [cout, fc]."""
    dev = t["x0"].device
    taps, pro = d["taps"], d["prologue"]
    src = t["x0"] if t.get("x1") is None else torch.cat([t["x0"], t["x1"]], 3)
    imgs = torch.unique(img)
    loc = torch.empty(int(img.max()) + 1, dtype=torch.long)
    loc[imgs] = torch.arange(imgs.numel())
    sub = src[imgs.to(dev)].float()
    if pro in (1, 2):
        act, risk = prologue(sub, t["a"][imgs.to(dev)][:, None, None, :].float(), t["b"][imgs.to(dev)][:, None, None, :].float(),
                             pro, dtype)
    else:
        act, risk = sub, torch.zeros_like(sub)
    n_, hs, ws_, cin = act.shape
    li = loc[img].to(dev)
    oy, ox = oy.to(dev), ox.to(dev)
    if d["up_phase"]:
        sy, sx, up = oy // 2, ox // 2, False
    elif d["in_up"]:
        sy, sx, up = oy, ox, True
    else:
        sy, sx, up = oy, ox, False
    offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] if taps == 9 else [(0, 0)]
    lim_y, lim_x = (2 * hs, 2 * ws_) if up else (hs, ws_)
    pa, pr = [], []
    for dy, dx in offs:
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < lim_y) & (xx >= 0) & (xx < lim_x)
        yi, xi = yy.clamp(0, lim_y - 1), xx.clamp(0, lim_x - 1)
        if up:
            yi, xi = yi // 2, xi // 2
        m = ok[:, None].to(act.dtype)
        pa.append(act[li, yi, xi] * m)
        pr.append(risk[li, yi, xi] * m)
    pa = torch.stack(pa, 1).reshape(li.numel(), -1).double()   # [P, taps * cin], tap-major
    pr = torch.stack(pr, 1).reshape(li.numel(), -1).double()
    w = t["w"].double()
    if d["up_phase"]:
        ph = (oy % 2) * 2 + (ox % 2)
        wm = w.permute(0, 1, 3, 4, 2).reshape(4, w.shape[1], -1)   # [4, cout, 9 * cin]
        acc = torch.empty((li.numel(), wm.shape[1]), dtype=torch.float64, device=dev)
        sab, srk = torch.empty_like(acc), torch.empty_like(acc)
        for p_ in range(4):
            s_ = ph == p_
            acc[s_] = pa[s_] @ wm[p_].T
            sab[s_] = pa[s_].abs() @ wm[p_].abs().T
            srk[s_] = pr[s_] @ wm[p_].abs().T
    else:
        wm = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)          # [cout, taps * cin]
        acc, sab, srk = pa @ wm.T, pa.abs() @ wm.abs().T, pr @ wm.abs().T
    kk = pa.shape[1]
    if d["has_fold0"]:
        fs = t["f0"] if t.get("f1") is None else torch.cat([t["f0"], t["f1"]], 3)
        pf = fs[img.to(dev), oy, ox].double()
        w1 = t["w1"].double()
        acc, sab = acc + pf @ w1.T, sab + pf.abs() @ w1.abs().T
        kk += pf.shape[1]
    bias = t["bias"].double()
    A = acc + bias
    E = srk + (kk + max(1, d["ksplit"]) + 2) * 2.0 ** -24 * (sab + bias.abs())
    if d["geglu"]:
        v, g = A[:, 0::2], A[:, 1::2]
        gel = 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))
        ref = v * gel
        bound = ulp_t(ref, dtype) + gel.abs() * E[:, 0::2] + 1.13 * v.abs() * E[:, 1::2] + SILU_REL * (ref.abs() + v.abs())
        return ref, bound
    if d["out_mode"] == 1:
        s = d["out_scale"] if d["out_scale"] != 0.0 else 1.0
        return A * s, s * (E + 2.0 ** -24 * A.abs())
    if pro == 3:
        xg = t["res"][img.to(dev), oy, ox].double()
        z = t["gnb_a"][img.to(dev)].double() * xg + t["gnb_b"][img.to(dev)].double()
        sg = torch.sigmoid(z)
        dsl = sg * (1 + z * (1 - sg))
        ref = A * dsl
        return ref, ulp_t(ref, dtype) + dsl.abs() * (0.5 * ulp_t(A, dtype) + E) + SILU_REL * (ref.abs() + A.abs())
    if d["has_res"]:
        r = t["res"][img.to(dev), oy // 2, ox // 2] if d["res_up"] else t["res"][img.to(dev), oy, ox]
        ref = A + r.double()
        return ref, ulp_t(ref, dtype) + 0.5 * ulp_t(A, dtype) + E
    return A, ulp_t(A, dtype) + E


# ------------------------------------------------------------------ attention restatement
def attention_restate(q, k, v, scale: float, dtype, causal: bool = False):
    """float64 softmax(q k^T scale) v for q [B, tq, d], k / v [B, tk, d] holding T values -> (ref, bound) [B, tq, d].
    causal (tq == tk): the logits above the diagonal are -inf; the bound's key count and max_j |v_j| run over the keys j <= query."""
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.transpose(1, 2)) * scale
    tk, d = k.shape[1], q.shape[2]
    ds = (d + 2) * 2.0 ** -24 * (q.abs() @ k.abs().transpose(1, 2)) * scale + 2.0 ** -22 * s.abs()
    if causal:
        if q.shape[1] != tk:
            raise NotImplementedError("causal attention: one query per key")
        above = torch.ones(tk, tk, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(above, float("-inf"))
        ds = ds.masked_fill(above, 0.0)
        vmax = torch.cummax(v.abs(), 1).values                        # [B, tq, d]: max over the keys <= query
        keys = torch.arange(1, tk + 1, dtype=torch.float64, device=q.device)[None, :, None]
    else:
        vmax = v.abs().amax(1, keepdim=True)                             # [B, 1, d]
        keys = float(tk)
    p = torch.softmax(s, -1)
    ref = p @ v
    bound = ulp_t(ref, dtype) + (C_ATTN * U[dtype] + 2.0 * ds.amax(-1, keepdim=True) + (keys + 2) * 2.0 ** -24) * vmax
    if dtype == torch.float16:
        bound = bound + keys * 2.0 ** -25 * vmax                      # P below fp16's normal range: absolute spacing 2^-24
    return ref, bound


def split_qkv(qkv, heads: int, new_order: bool):
    """[N, T, 3 H D] (ops.attention's layout) -> q, k, v [N * H, T, D] (the reference's qkv order: new or legacy)."""
    n, t, c3 = qkv.shape
    d = c3 // 3 // heads
    if new_order:
        x = qkv.reshape(n, t, 3, heads, d).permute(2, 0, 3, 1, 4)
    else:
        x = qkv.reshape(n, t, heads, 3, d).permute(3, 0, 2, 1, 4)
    q, k, v = (x[i].reshape(n * heads, t, d) for i in range(3))
    return q, k, v


def merge_heads(o, n: int, heads: int):
    """[N * H, T, D] -> [N, T, H D]."""
    _, t, d = o.shape
    return o.reshape(n, heads, t, d).permute(0, 2, 1, 3).reshape(n, t, heads * d)


def lse_restate(q, k, scale: float, dtype):
    """log2-domain log-sum-exp of the scaled logits (what adm_attention_lse stores) -> (ref, bound) [B, tq]."""
    s = (q.double() @ k.double().transpose(1, 2)) * scale
    ref = torch.logsumexp(s, -1) / math.log(2.0)
    return ref, U[dtype] / math.log(2.0) + 2.0 ** -18 * (1 + ref.abs() + (s.abs().amax(-1) / math.log(2.0)))


def attention_bwd_restate(q, k, v, o, do, scale: float, dtype):
    """float64 backward of softmax(q k^T scale) v with the forward output o as the kernel is given it (δ = rowsum(do o)):
    -> ((dq, dk, dv), (bound_q, bound_k, bound_v)), each [B, t, d]."""
    q, k, v, o, do = (x.double() for x in (q, k, v, o, do))
    p = torch.softmax((q @ k.transpose(1, 2)) * scale, -1)
    dp = do @ v.transpose(1, 2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq, dk, dv = (ds @ k) * scale, (ds.transpose(1, 2) @ q) * scale, p.transpose(1, 2) @ do
    u = U[dtype]
    a = p * (dp.abs() + delta.abs())
    bq = ulp_t(dq, dtype) + 4 * u * scale * (a @ k.abs())
    bk = ulp_t(dk, dtype) + 4 * u * scale * (a.transpose(1, 2) @ q.abs())
    bv = ulp_t(dv, dtype) + 2 * u * (p.transpose(1, 2) @ do.abs())
    return (dq, dk, dv), (bq, bk, bv)


def _half_up(t, h, w):
    """[n, h/2, w/2, c] read through the nearest 2x upsample with the AvgPool2d backward's 1/4."""
    return 0.25 * t.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w]


def gn_bwd_restate(x, dy, a, b, stats, silu: bool, dy_half: bool, add, add_half: bool, e, dtype):
    """float64 dx of y = act(a x + b) through the GroupNorm whose (mean, rstd) = stats [n, 32, 2] (of x + e when e is given),
    as adm_gn_bwd_* state it: dz = dy act'(a x + b); dx = a dz + k1 (x + e) + k0 (+ add) -> (ref, bound) [n, h, w, c]."""
    n, h, w, c = x.shape
    x, a, b = x.double(), a.double()[:, None, None, :], b.double()[:, None, None, :]
    dz = _half_up(dy.double(), h, w) if dy_half else dy.double()
    if silu:
        z = a * x + b
        sg = torch.sigmoid(z)
        dz = dz * sg * (1 + z * (1 - sg))
    xe = x if e is None else x + e.double()[:, None, None, :]
    cpg = c // 32
    mean = stats[..., 0].double().repeat_interleave(cpg, 1)[:, None, None, :]
    r = stats[..., 1].double().repeat_interleave(cpg, 1)[:, None, None, :]
    m = cpg * h * w

    def gsum(t):   # per (image, group) sum, broadcast back to channels
        return t.sum((1, 2)).reshape(n, 32, cpg).sum(-1).repeat_interleave(cpg, 1)[:, None, None, :]
    s1 = gsum(a * dz) / r
    s2 = gsum(a * dz * (xe - mean))
    k1 = -r * r * s2 / m
    k0 = -r * s1 / m - mean * k1
    ad = 0.0 if add is None else (_half_up(add.double(), h, w) if add_half else add.double())
    ref = a * dz + k1 * xe + k0 + ad
    acc = h * w * 2.0 ** -24
    e1 = r * r / m * gsum((a * dz).abs() * (xe.abs() + mean.abs())) * acc
    e0 = r / m * gsum((a * dz).abs()) / r * acc + mean.abs() * e1
    bound = (ulp_t(ref, dtype) + 2.0 ** -20 * ((a * dz).abs() + (k1 * xe).abs() + k0.abs() + (ad.abs() if add is not None else 0.0))
             + xe.abs() * e1 + e0)
    return ref, bound


def gn_affine_restate(x, gamma, beta, eps: float, film=None, add=None):
    """float64 GroupNorm32 (+ FiLM (1 + scale), shift) of x [n, h, w, c] (+ add[:, None, None, :]) -> (y, mean [n, 32], rstd)."""
    n, h, w, c = x.shape
    xe = x.double() if add is None else x.double() + add.double()[:, None, None, :]
    g = xe.reshape(n, h * w, 32, c // 32)
    mean = g.mean((1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((g - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(n, h, w, c) * gamma.double() + beta.double()
    if film is not None:
        y = y * (1 + film[:, None, None, :c].double()) + film[:, None, None, c:2 * c].double()
    return y, mean, rstd


# ------------------------------------------------------------------ token, resample, layout and VAE entry / exit restatements
def half_ulp(ref, dtype):
    return 0.5 * ulp_t(ref, dtype)


def layernorm_restate(x, gamma, beta, eps: float, dtype, f32out: bool = False):
    """float64 two-pass LayerNorm over the last dimension of x [rows, c] holding T values -> (ref, bound); f32out: the kernel
    stores fp32, so no rounding to T."""
    x, g, b = x.double(), gamma.double(), beta.double()
    c = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    yg = xc * rstd * g
    ref = yg + b
    k = (8 * ((c + 511) // 512) + 8) * 2.0 ** -24
    bound = k * rstd * g.abs() * x.abs().mean(-1, keepdim=True) + (k + 2.0 ** -21) * yg.abs() + 2.0 ** -23 * ref.abs()
    return ref, (bound if f32out else bound + half_ulp(ref, dtype))


def gelu_erf(g):
    return 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))


def geglu_restate(u, dtype):
    """u [rows, 2 inner] holding T values (values, then gates) -> (v gelu_erf(g), bound) [rows, inner]."""
    inner = u.shape[-1] // 2
    v, g = u[..., :inner].double(), u[..., inner:].double()
    ref = v * gelu_erf(g)
    return ref, half_ulp(ref, dtype) + SILU_REL * (ref.abs() + v.abs())


def quick_gelu_restate(a, dtype):
    a = a.double()
    ref = a * torch.sigmoid(1.702 * a)
    return ref, half_ulp(ref, dtype) + SILU_REL * (1 + (1.702 * a).abs()) * ref.abs()


def clip_embed_restate(ids, tok, pos, pitch: int, dtype):
    """round_T(tok[ids] + pos[:t]) with the add in fp32, rows t .. pitch zero -> [n, pitch, c] of T (compared bitwise)."""
    n, t = ids.shape
    out = torch.zeros((n, pitch, tok.shape[1]), dtype=dtype, device=tok.device)
    out[:, :t] = (tok.float()[ids] + pos.float()[:t]).to(dtype)
    return out


def resample_restate(x, mode: int, aff, dtype):
    """x [n, h, w, c] holding T values; mode 1 AvgPool2d(2), 2 nearest x2, 3 every second pixel, 4 zero-insert x2, 5 the odd pixels; aff = (a, b)
    fp32 [n, c]: silu(a x + b) first -> (ref, bound); the bound is None where the result is a copy (compared bitwise)."""
    n, h, w, c = x.shape
    s = x.double()
    e = None
    if aff is not None:
        a, b = aff[0].double()[:, None, None, :], aff[1].double()[:, None, None, :]
        z = a * s + b
        e = 2.0 ** -23 * ((a * s).abs() + b.abs())
        s = z * torch.sigmoid(z)
        e = e + SILU_REL * s.abs()
    if mode == 1:
        def pool(t):
            return t.reshape(n, h // 2, 2, w // 2, 2, c).mean((2, 4))
        ref = pool(s)
        bound = half_ulp(ref, dtype) + 4 * 2.0 ** -24 * pool(s.abs())
        return ref, (bound if e is None else bound + pool(e))
    if mode == 2:
        ref = s.repeat_interleave(2, 1).repeat_interleave(2, 2)
        e = None if e is None else e.repeat_interleave(2, 1).repeat_interleave(2, 2)
    elif mode == 3:
        ref = s[:, ::2, ::2]
        e = None if e is None else e[:, ::2, ::2]
    elif mode == 5:
        ref = s[:, 1::2, 1::2]
        e = None if e is None else e[:, 1::2, 1::2]
    elif mode == 4:
        if aff is not None:
            raise NotImplementedError("zero-insert takes no affine")
        ref = torch.zeros((n, 2 * h, 2 * w, c), dtype=s.dtype, device=s.device)
        ref[:, ::2, ::2] = s
    else:
        raise NotImplementedError(f"resample mode {mode}")
    return ref, (None if e is None else half_ulp(ref, dtype) + e)


def nchw_to_nhwc_pad_restate(x, cpad: int, dtype):
    n, c, h, w = x.shape
    out = torch.zeros((n, h, w, cpad), dtype=dtype, device=x.device)
    out[..., :c] = x.float().permute(0, 2, 3, 1).to(dtype)
    return out


def vae_latent_in_restate(z, w, b, inv_scale: float, dtype):
    """z fp32 [n, e, h, w], w [zc, e], b [zc], inv_scale as the fp32 value the kernel is passed -> (ref, bound) [n, h, w, zc]."""
    e = z.shape[1]
    zs = z.double().permute(0, 2, 3, 1) * float(inv_scale)                  # [n, h, w, e]
    wd = w.double().reshape(w.shape[0], e)
    ref = zs @ wd.T + b.double()
    mag = zs.abs() @ wd.abs().T + b.double().abs()
    return ref, half_ulp(ref, dtype) + (e + 3) * 2.0 ** -24 * mag


def vae_image_out_restate(x):
    """x fp32 NCHW -> (unit fp32 NCHW = clamp((x + 1) / 2, 0, 1) in fp32, uint8 NHWC = trunc(255 unit)); compared bitwise."""
    unit = torch.clamp((x.float() + 1.0) / 2.0, min=0.0, max=1.0)
    return unit, (255.0 * unit).permute(0, 2, 3, 1).to(torch.uint8)


IMAGE_OUT_SPECIALS = (1.0, -1.0, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, -1e-45, 0.9999999, -0.9999999, 1.0000001, 0.003921569)
QUICK_GELU_SPECIALS = (-12.0, 12.0, 0.0, -0.0, 1e-3, -1e-3, 1.0, -1.0)
BIG = 1 << 25


def compared_images(n: int, numel: int, seed: int) -> list:
    """The images (first index) of an elementwise record to compare: all of them up to 2^25 elements, else the first, the last
    and one seeded image."""
    if numel <= BIG:
        return list(range(n))
    g = torch.Generator().manual_seed(seed)
    return sorted({0, n - 1, int(torch.randint(0, n, (1,), generator=g))})


def worst_ratio(got, ref, bound):
    """(worst err / bound, sum err^2, sum ref^2, report of the worst element) of one compared block."""
    err = (got.double() - ref).abs()
    r = err / bound
    r = torch.where(torch.isfinite(got.double()) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    j = int(r.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(j), r.shape))
    rep = f"index {idx}: got {got.double().flatten()[j].item():.8g} ref {ref.flatten()[j].item():.8g} bound {bound.expand_as(r).flatten()[j].item():.4g}"
    return r.flatten()[j].item(), (err ** 2).sum().item(), (ref ** 2).sum().item(), rep


# ------------------------------------------------------------------ classifier heads and gradient helpers
F32_MIN = 2.0 ** -126   # below fp32's normal range a result may be flushed or lose bits: an absolute floor, not a tolerance
E24 = 2.0 ** -24


def f32c(x: float) -> float:
    """The fp32 value a C `float` argument receives."""
    return float(torch.tensor(x, dtype=torch.float32))


def silu_terms(h, a, b):
    """float64 s = SiLU(a h + b) of T values h through the fp32 affine (a, b) and the error of the kernels' adm_silu."""
    ah = a.double() * h.double()
    z = ah + b.double()
    s = z * torch.sigmoid(z)
    return s, 2.0 ** -23 * (ah.abs() + b.double().abs()) + SILU_REL * (1 + z.abs()) * s.abs()


def pool_prep_restate(h, a, b, pos, tpad: int, dtype):
    """h [n, hw, c] of T, a / b fp32 [n, c], pos fp32 [c, hw + 1] -> (ref, bound) [n, hw + 1, c]; rows hw + 1 .. tpad are zero."""
    n, hw, c = h.shape
    s, e = silu_terms(h, a[:, None, :], b[:, None, :])
    p = pos.double().t()                                                   # [T, c]
    m = s.mean(1, keepdim=True)
    ref = torch.cat([m + p[None, :1], s + p[None, 1:]], 1)
    b0 = (e.mean(1, keepdim=True) + (hw + 2) * E24 * s.abs().mean(1, keepdim=True) + SILU_REL * m.abs()
          + E24 * (m.abs() + p[None, :1].abs()))
    b1 = e + E24 * (s.abs() + p[None, 1:].abs())
    return ref, half_ulp(ref, dtype) + torch.cat([b0, b1], 1)


def pool_split(qkv, t: int, heads: int):
    """qkv [n, tpad, 3 C] ([q | k | v], heads inside each) -> q0 [n, H, d], k / v [n, H, t, d] in float64."""
    n, _, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    x = qkv[:, :t].double().reshape(n, t, 3, heads, d)
    return x[:, 0, 0], x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)


POOL_C1, POOL_C2 = 4, 1


def pool_attn_fwd_restate(qkv, t: int, heads: int):
    """Attention of token 0 over the first t rows -> ((wts [n, H, t], a0 [n, C]), (bound_w, bound_a))."""
    q0, k, v = pool_split(qkv, t, heads)
    n, _, d = q0.shape
    scale = d ** -0.5
    s = torch.einsum("nhd,nhtd->nht", q0, k) * scale
    ds = (d + POOL_C1) * E24 * torch.einsum("nhd,nhtd->nht", q0.abs(), k.abs()) * scale
    w = torch.softmax(s, -1)
    span = s.amax(-1, keepdim=True) - s
    rel = (2 * ds.amax(-1, keepdim=True) + E24 * (span + (w * span).sum(-1, keepdim=True)) + 3 * SILU_REL
           + ((t + 63) // 64 + 7) * E24)
    bw = rel * w + F32_MIN
    a0 = torch.einsum("nht,nhtd->nhd", w, v)
    ba = torch.einsum("nht,nhtd->nhd", bw, v.abs()) + (t + POOL_C2) * E24 * torch.einsum("nht,nhtd->nhd", w, v.abs())
    return (w, a0.reshape(n, heads * d)), (bw, ba.reshape(n, heads * d))


def pool_attn_bwd_restate(qkv, wts, da0, t: int, heads: int, dtype):
    """Backward of the above with the stored weights wts [n, H, tpad] and da0 fp32 [n, C] -> (ref, bound) [n, t, 3 C]: dQ on
    row 0 only (the rows above are zero), dK, dV on the rows < t."""
    q0, k, v = pool_split(qkv, t, heads)
    n, _, d = q0.shape
    scale = d ** -0.5
    w = wts[:, :, :t].double()
    da = da0.double().reshape(n, heads, d)
    dw = torch.einsum("nhd,nhtd->nht", da, v)
    e_dw = (d + 1) * E24 * torch.einsum("nhd,nhtd->nht", da.abs(), v.abs())
    delta = (w * dw).sum(-1, keepdim=True)
    e_delta = (w * e_dw).sum(-1, keepdim=True) + ((t + 63) // 64 + 7) * E24 * (w * dw.abs()).sum(-1, keepdim=True)
    dlg = w * (dw - delta) * scale
    e_dlg = w * scale * (e_dw + e_delta + 5 * E24 * (dw.abs() + delta.abs()))
    dk = dlg[..., None] * q0[:, :, None, :]
    bk = e_dlg[..., None] * q0.abs()[:, :, None, :] + E24 * dk.abs()
    dv = w[..., None] * da[:, :, None, :]
    bv = E24 * dv.abs()
    dq = torch.zeros_like(dk)
    bq = torch.zeros_like(dk)
    dq[:, :, 0] = torch.einsum("nht,nhtd->nhd", dlg, k)
    bq[:, :, 0] = (torch.einsum("nht,nhtd->nhd", e_dlg, k.abs())
                   + (t + 1) * E24 * torch.einsum("nht,nhtd->nhd", dlg.abs(), k.abs()))
    ref = torch.stack([dq, dk, dv], 1)                                     # [n, 3, H, t, d]
    bound = torch.stack([bq, bk, bv], 1)
    ref = ref.permute(0, 3, 1, 2, 4).reshape(n, t, 3 * heads * d)
    bound = bound.permute(0, 3, 1, 2, 4).reshape(n, t, 3 * heads * d)
    return ref, half_ulp(ref, dtype) + bound


def pool_prep_bwd_restate(dtok, hw: int, dtype):
    """dtok [n, tpad, c] of T -> d_act [n, hw, c] = dtok[:, 1 + p] + dtok[:, 0] / hw."""
    x = dtok.double()
    m = x[:, :1] / hw
    ref = x[:, 1:hw + 1] + m
    return ref, half_ulp(ref, dtype) + SILU_REL * m.abs() + E24 * (x[:, 1:hw + 1].abs() + m.abs())


def channel_mean_restate(h, aff):
    """h [n, hw, c] of T; aff = (a, b) fp32 [n, c] or None -> fp32 mean over the pixels (ref, bound) [n, c]."""
    hw = h.shape[1]
    if aff is None:
        v, e = h.double(), None
    else:
        v, e = silu_terms(h, aff[0][:, None, :], aff[1][:, None, :])
    ref = v.mean(1)
    bound = ((hw + 3) // 4 + 3) * E24 * v.abs().mean(1) + SILU_REL * ref.abs() + F32_MIN
    return ref, (bound if e is None else bound + e.mean(1))


def bcast_add_restate(v, scale: float, add, hw: int, dtype):
    """v fp32 [n, c] (the column window), add [n, hw, c] of T or None -> (ref, bound) [n, hw, c]; bound None without add: the
    result is round_T of the fp32 product, compared bitwise."""
    if add is None:
        return (v.float() * torch.tensor(scale, dtype=torch.float32)).to(dtype)[:, None, :].expand(-1, hw, -1).contiguous(), None
    vs = v.double()[:, None, :] * f32c(scale)
    ref = add.double() + vs
    return ref, half_ulp(ref, dtype) + E24 * (2 * vs.abs() + add.double().abs())


VEC_ACT_MODES = {"silu": 1, "relu": 2, "gauss_std": 3, "gauss_logvar": 4}


def vec_act_restate(x, mode: int, dy=None):
    """fp32 x (and dy): act(x) or dy act'(x) -> (ref, bound); ReLU is exact (bound None: equal as values), ReLU'(0) = 0.  Modes
    3 / 4 are f32_vae_kernels': exp(0.5 clamp(x)) (times dy), and the clamped log-variance as an fp32 tensor (bound None: bitwise)."""
    if mode == 3:
        return gauss_std_restate(x, dy)
    if mode == 4:
        if dy is not None:
            raise NotImplementedError("gauss_logvar takes no dy")
        return gauss_logvar_restate(x), None
    z = x.double()
    if mode == 2:
        return (torch.clamp(z, min=0.0) if dy is None else dy.double() * (z > 0).double()), None
    s = torch.sigmoid(z)
    if dy is None:
        ref = z * s
        return ref, SILU_REL * ref.abs() + F32_MIN
    ref = dy.double() * s * (1 + z * (1 - s))
    return ref, SILU_REL * dy.double().abs() * s * (1 + z.abs()) + F32_MIN


def _vec_k(c: int) -> float:
    cpg = c // 32
    return ((cpg + 7) // 8 + 3) * E24     # a lane's adds and the three butterfly steps


def vec_gn_restate(x, gamma, beta, eps: float):
    """GroupNorm32 of fp32 rows x [n, c] -> ((y, mean [n, 32], rstd), (bound_y, bound_mean, bound_rstd))."""
    n, c = x.shape
    cpg = c // 32
    k = _vec_k(c)
    g = x.double().reshape(n, 32, cpg)
    mean = g.mean(-1, keepdim=True)
    e_m = k * g.abs().mean(-1, keepdim=True) + SILU_REL * mean.abs()
    d = g - mean
    var = (d * d).mean(-1, keepdim=True)
    e_v = 2 * d.abs().mean(-1, keepdim=True) * e_m + e_m * e_m + (k + 4 * E24 + SILU_REL) * var
    eps = f32c(eps)
    rstd = 1.0 / torch.sqrt(var + eps)
    rel_r = e_v / (2 * (var + eps)) + E24 + 2 * SILU_REL
    gm, bt = gamma.double().reshape(1, 32, cpg), beta.double().reshape(1, 32, cpg)
    yg = gm * d * rstd
    y = yg + bt
    by = gm.abs() * rstd * e_m + yg.abs() * (rel_r + 4 * E24) + E24 * y.abs() + F32_MIN
    return (y.reshape(n, c), mean[..., 0], rstd[..., 0]), (by.reshape(n, c), (e_m + F32_MIN)[..., 0], (rstd * rel_r)[..., 0])


def vec_gn_bwd_restate(x, gamma, stats, dz):
    """dx = rstd (g - mean_g(g) - xhat mean_g(g xhat)), g = gamma dz, xhat = (x - mean) rstd with the stored stats [n, 32, 2]."""
    n, c = x.shape
    cpg = c // 32
    k = _vec_k(c)
    mean, rstd = stats[..., :1].double(), stats[..., 1:].double()
    g = (gamma.double()[None] * dz.double()).reshape(n, 32, cpg)
    xh = (x.double().reshape(n, 32, cpg) - mean) * rstd
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    e1 = (k + E24) * g.abs().mean(-1, keepdim=True) + SILU_REL * s1.abs()
    e2 = (k + 4 * E24) * (g * xh).abs().mean(-1, keepdim=True) + SILU_REL * s2.abs()
    ref = rstd * (g - s1 - xh * s2)
    bound = rstd * (e1 + xh.abs() * e2 + 4 * E24 * (g.abs() + s1.abs() + (xh * s2).abs())) + E24 * ref.abs() + F32_MIN
    return ref.reshape(n, c), bound.reshape(n, c)


def logsoftmax_grad_restate(logits, y, scale: float):
    """scale (onehot(y) - softmax(logits)) and log_softmax[n, y_n] -> ((dl [n, k], logp [n]), (bound_dl, bound_logp))."""
    n, k = logits.shape
    l = logits.double()
    sc = f32c(scale)
    lsm = torch.log_softmax(l, -1)
    sm = lsm.exp()
    one = torch.zeros_like(sm)
    one[torch.arange(n, device=l.device), y] = 1.0
    dist = l.amax(-1, keepdim=True) - l
    tree = ((k + 255) // 256 + 8) * E24
    rel = E24 * dist + 3 * SILU_REL + tree + (sm * dist).sum(-1, keepdim=True) * E24
    ref = sc * (one - sm)
    bound = abs(sc) * (rel * sm + F32_MIN) + 2 * E24 * ref.abs()
    logp = lsm[torch.arange(n, device=l.device), y]
    dy = dist[torch.arange(n, device=l.device), y]
    logsum = torch.logsumexp(l - l.amax(-1, keepdim=True), -1)
    bl = E24 * dy + SILU_REL * (1 + logsum.abs()) + tree + (sm * dist).sum(-1) * E24 + 2 * E24 * logp.abs() + F32_MIN
    return (ref, logp), (bound, bl)


def grad_add_restate(a, b, b_half: bool, dtype):
    """a [n, h, w, c], b the same or [n, h/2, w/2, c] read through the nearest 2x upsample times 1/4 -> (ref, bound)."""
    n, h, w, c = a.shape
    sb = _half_up(b.double(), h, w) if b_half else b.double()
    ref = a.double() + sb
    return ref, half_ulp(ref, dtype) + E24 * (a.double().abs() + sb.abs())


def pool_zero_rows_ok(dqkv, t: int) -> bool:
    """adm_pool_attn_bwd's zeros: the rows >= t, and the dQ columns of the rows 1 .. t, hold only zero bit patterns."""
    c = dqkv.shape[2] // 3
    return not bool(dqkv[:, t:].contiguous().view(torch.int16).any()) and not bool(dqkv[:, 1:t, :c].contiguous().view(torch.int16).any())


# ------------------------------------------------------------------ the KL-f8 encoder's head as a composite
def head_window(h, gamma, beta, eps: float):
    """float64 GroupNorm32 of the stored map h [n, hh, ww, c] -> (z, dz): z = γ ŷ + β in front of the SiLU and the distance dz
    that a z formed from fp32 statistics may lie from it (module docstring)."""
    n, hh, ww, c = h.shape
    z, mean, rstd = gn_affine_restate(h, gamma, beta, eps)
    cpg = c // 32
    m = mean.repeat_interleave(cpg, 1)[:, None, None, :]
    r = rstd.repeat_interleave(cpg, 1)[:, None, None, :]
    g = gamma.double().abs()
    yh = ((h.double() - m) * r).abs()
    dz = (2.0 ** -20 + 2.0 ** -22) * g * (m.abs() * r + 1 + yh) + 2.0 ** -23 * (beta.double().abs() + z.abs())
    return z, dz


def head_activation(h, gamma, beta, eps: float, dtype):
    """-> (act, risk) [n, hh, ww, c] float64: SiLU(GroupNorm(h)) rounded once to T, and the step to the other T neighbour where s
    lies within 1.1 dz + PRO_ULPS 2^-23 |s| of a rounding midpoint (else 0)."""
    z, dz = head_window(h, gamma, beta, eps)
    s = z * torch.sigmoid(z)
    ds = 1.1 * dz + PRO_ULPS * 2.0 ** -23 * s.abs()
    r = round_t(s, dtype)
    risk = torch.maximum((round_t(s - ds, dtype) - r).abs(), (round_t(s + ds, dtype) - r).abs())
    return r, risk


def head_restate(h, gamma, beta, w, bias, eps: float, dtype, wq=None, bq=None):
    """Encoder._head on the stored 16-bit map h [n, hh, ww, c] -> (ref, bound) fp32-NCHW-shaped [n, cout, hh, ww] in float64: the
    pad-1 3x3 conv of head_activation on the unpadded map, w fp32 [cout, c, 3, 3] rounded to T, bias fp32.  With wq [o, cout, 1, 1]
    and bq [o] (Encoder.folded_head) the reference is wq (conv(act) + bias) + bq in float64 from the unfolded fp32 weights and the
    bound carries the fold's terms (module docstring)."""
    import torch.nn.functional as F
    n, hh, ww, c = h.shape
    act, risk = head_activation(h, gamma, beta, eps, dtype)
    cols = F.unfold(act.permute(0, 3, 1, 2), 3, padding=1)              # [n, c * 9, hh * ww], zeros outside the map
    rcols = F.unfold(risk.permute(0, 3, 1, 2), 3, padding=1)
    kk = c * 9
    if wq is None:
        wm = round_t(w.double(), dtype).reshape(w.shape[0], kk)
        wmag, bd = wm.abs(), bias.double()
        extra, bextra = 0.0, 0.0
    else:
        q = wq.double().reshape(wq.shape[0], -1)                            # [o, m]
        m = q.shape[1]
        w64 = w.double().reshape(w.shape[0], kk)
        wm = q @ w64
        dw = half_ulp(wm, dtype) + (m + 1) * E24 * (q.abs() @ w64.abs())
        wmag = wm.abs() + dw
        bd = q @ bias.double() + bq.double()
        extra = dw @ cols.abs()
        bextra = ((m + 2) * E24 * (q.abs() @ bias.double().abs() + bq.double().abs()))[:, None]
    ref = wm @ cols + bd[:, None]
    e = wmag @ rcols + (kk + 1 + 2) * E24 * (wmag @ cols.abs() + bd.abs()[:, None]) + extra + bextra
    bound = e + E24 * ref.abs()
    shape = (n, wm.shape[0], hh, ww)
    return ref.reshape(shape), bound.reshape(shape)


HEAD_OFFSET = -4.0   # mean / std of the head tests' maps (head_operands)


def head_operands(n: int, side: int, c: int, cout: int, dtype, seed: int) -> dict:
    """Seeded host operands of one head case: the 16-bit mid map h [n, side, side, c], norm_out's (gamma, beta), conv_out's fp32
    (w, bias) and a 1x1 (wq [cout, cout, 1, 1], bq) to fold.  The map is N(HEAD_OFFSET, 1): with a mean four standard deviations
    below zero the GroupNorm shift is b = β - γ mean rstd ~ +4, so a pixel that is zero BEFORE the activation (padding activated
    too late) becomes SiLU(b) ~ 3.9 where the conv must read 0 -- an error of order Σ |w| 3.9 over a row of taps, thousands of
    times the bound, on the last row and column only.  At a mean of zero the same defect would hide inside SiLU(β) ~ β / 2."""
    g = torch.Generator().manual_seed(seed)
    return {"h": (torch.randn(n, side, side, c, generator=g) + HEAD_OFFSET).to(dtype),
            "gamma": 1 + 0.2 * torch.randn(c, generator=g), "beta": 0.2 * torch.randn(c, generator=g),
            "w": torch.randn(cout, c, 3, 3, generator=g) * (9 * c) ** -0.5, "bias": 0.1 * torch.randn(cout, generator=g),
            "wq": torch.randn(cout, cout, 1, 1, generator=g) * cout ** -0.5, "bq": 0.1 * torch.randn(cout, generator=g)}
