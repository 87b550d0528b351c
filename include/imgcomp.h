/*
 * imgcomp.h — C ABI of libimgcomp.so, the MI355X (gfx950) kernels behind the
 * Balle-2018 scale-hyperprior hot path of hieu1999210/image_compression.
 *
 * Every entry point:
 *   - takes raw device pointers (fp32), plain sizes and a hipStream_t
 *     (passed as void* so this header needs no HIP include);
 *   - launches asynchronously on that stream; never allocates, frees or
 *     synchronises (graph-capturable); keeps no pointer after it returns;
 *   - returns 0 on success, a hipError_t value on a launch failure, or
 *     IC_ERR_ARG (1001) / IC_ERR_WORKSPACE (1002).  The Python host layer
 *     turns any non-zero status into RuntimeError (reference error
 *     behaviour: torch raises RuntimeError on bad shapes).
 *   - Ops that need scratch take (ws, ws_bytes); the matching *_ws() query
 *     returns the byte count for the same arguments.
 *
 * Activations are described by ic_act: logical [n][c][h][w] with arbitrary
 * element strides.  The GEMM fast paths want channel stride 1 (NHWC,
 * torch.channels_last); other layouts take the generic gather path.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   conv2d_*            torch.nn.Conv2d in modelling/blocks/analysis.py:55,
 *                       modelling/blocks/prior_analysis.py:54-56
 *   conv_transpose2d_*  torch.nn.ConvTranspose2d in modelling/blocks/synthesis.py:55-57,
 *                       modelling/blocks/prior_synthesis.py:54-56
 *   gdn_*               modelling/layers/gdn.py:79-88 (GDN.forward)
 *   nonneg_*            modelling/layers/gdn.py:59-62 (NonNegativeParam.forward)
 *   bound_*             modelling/layers/bound.py:28-59 (LowerBound / UpperBound)
 *   relu_*, abs_*       nn.ReLU (prior_*.py), torch.abs (meta_arch/bmshl2018.py:72)
 *   exp_clamp_*         modelling/blocks/prior_synthesis.py:72
 *   factorized_*        modelling/blocks/entropy_model.py:204-269 (EntropyModel)
 *   conditional_*       modelling/blocks/entropy_model.py:280-378 (Laplacian/Gaussian)
 *   ce_loss_*           modelling/blocks/entropy_model.py:171-185 (_ce_loss)
 *   mse_*, sqdiff_*     nn.MSELoss(reduction="mean"/"none") in modelling/loss.py:25
 *   msssim_*            modelling/loss.py:48-188 (SSIMLoss, MS_SSIMLoss)
 *   adamw_step          torch.optim.AdamW of solver/optim.py:20-45 + clip_grad_value_ of
 *                       engine/trainer.py:189-190 (the training step around the path)
 */
#ifndef IMGCOMP_H
#define IMGCOMP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IC_ERR_ARG 1001
#define IC_ERR_WORKSPACE 1002

typedef struct ic_act {
  float* data;
  int n, c, h, w;
  long long sn, sc, sh, sw; /* element strides */
} ic_act;

/* ---- library ---- */
int ic_version(void);                 /* ABI version (monotonic; 3: ic_fact_net with IC_FACT_NET_MAXL layers; 4: ic_codec_*;
                                         additive to 4: ic_codec_*_seg, ic_pad_edge / ic_crop_clamp, and the mean-scale ops
                                         ic_codec_symbolize_mean*, ic_center_round, ic_add_mean, and every later section
                                         marked "additive to version 4") */
int ic_device_sync_check(void* stream); /* hipStreamQuery-free no-op launch test */

/* ---- Conv2d (k x k, stride, zero pad): y = conv(x, w) + b, act 0=none 1=relu
 *      w: [Cout][Cin][k][k]; b: [Cout] or NULL; y->c = Cout, y->h = (x->h+2pad-k)/stride+1 */
size_t ic_conv2d_fwd_ws(const ic_act* x, int k, int stride, int pad, const ic_act* y);
int ic_conv2d_fwd(const ic_act* x, const float* w, const float* b, int k, int stride, int pad,
                  const ic_act* y, int act, void* ws, size_t ws_bytes, void* stream);
/* dx = conv2d input-gradient of dy (no bias); dx->c = Cin */
size_t ic_conv2d_dgrad_ws(const ic_act* dy, int k, int stride, int pad, const ic_act* dx);
int ic_conv2d_dgrad(const ic_act* dy, const float* w, int k, int stride, int pad, const ic_act* dx,
                    void* ws, size_t ws_bytes, void* stream);
/* dw [Cout][Cin][k][k] = weight gradient; db [Cout] (optional, NULL to skip) */
size_t ic_conv2d_wgrad_ws(const ic_act* x, const ic_act* dy, int k, int stride, int pad);
int ic_conv2d_wgrad(const ic_act* x, const ic_act* dy, int k, int stride, int pad, float* dw,
                    float* db, void* ws, size_t ws_bytes, void* stream);

/* ---- ConvTranspose2d: w [Cin][Cout][k][k]; y->h = (x->h-1)*stride - 2pad + k + output_padding */
size_t ic_conv_transpose2d_fwd_ws(const ic_act* x, int k, int stride, int pad, const ic_act* y);
int ic_conv_transpose2d_fwd(const ic_act* x, const float* w, const float* b, int k, int stride,
                            int pad, const ic_act* y, int act, void* ws, size_t ws_bytes,
                            void* stream);
size_t ic_conv_transpose2d_dgrad_ws(const ic_act* dy, int k, int stride, int pad, const ic_act* dx);
int ic_conv_transpose2d_dgrad(const ic_act* dy, const float* w, int k, int stride, int pad,
                              const ic_act* dx, void* ws, size_t ws_bytes, void* stream);
size_t ic_conv_transpose2d_wgrad_ws(const ic_act* x, const ic_act* dy, int k, int stride, int pad);
int ic_conv_transpose2d_wgrad(const ic_act* x, const ic_act* dy, int k, int stride, int pad,
                              float* dw, float* db, void* ws, size_t ws_bytes, void* stream);

/* ---- math modes of the conv fwd / dgrad "_ex" variants (the plain entry points are math 0).
 *      IC_MATH_BF16: operands rounded to bf16 (round-to-nearest-even), fp32 accumulation on
 *      v_mfma_f32_32x32x16_bf16 — the bf16 configuration of BASELINE config C3 — for layers
 *      whose reduction channel count is a multiple of 64; others (the 3-channel image edges)
 *      and all weight gradients / GDN stay fp32. */
#define IC_MATH_FP32 0
#define IC_MATH_BF16 1
/*      IC_MATH_SPLIT: fp32 arithmetic on the bf16 MFMA — each fp32 operand split exactly into
 *      three bf16 terms, six cross products accumulated in fp32 (error of an fp32 fma chain,
 *      3/8 of the native fp32 MFMA's cycles per MAC); layers with reduction channels % 32 == 0
 *      and >= 64 output channels, others run the native fp32 kernel. */
#define IC_MATH_SPLIT 2
/*      IC_MATH_WPACKED (conv / transposed-conv forward only, or-ed into a math mode): the workspace
 *      already holds this weight's pack, written by an earlier forward with the same weight
 *      values, activation shapes / strides, math mode and workspace; the pack launch is skipped
 *      (eval-mode weight caching, functional.py).  Paths whose pack is not kept in the workspace
 *      (the im2col fallback, the row-stationary transposed edge) ignore it.  The caller owns the invalidation: any change of
 *      the weight needs a forward without the flag first. */
#define IC_MATH_WPACKED 4
/*      IC_MATH_XB (or-ed into IC_MATH_BF16, in the workspace query of a conv / transposed conv forward or
 *      input gradient whose caller passes the input's bf16 copy to the matching *_xb entry point): the
 *      workspace leaves out the space the conversion of x would take. */
#define IC_MATH_XB 8
size_t ic_conv2d_fwd_ws_ex(const ic_act* x, int k, int stride, int pad, const ic_act* y, int math);
int ic_conv2d_fwd_ex(const ic_act* x, const float* w, const float* b, int k, int stride, int pad,
                     const ic_act* y, int act, int math, void* ws, size_t ws_bytes, void* stream);
size_t ic_conv2d_dgrad_ws_ex(const ic_act* dy, int k, int stride, int pad, const ic_act* dx, int math);
int ic_conv2d_dgrad_ex(const ic_act* dy, const float* w, int k, int stride, int pad, const ic_act* dx,
                       int math, void* ws, size_t ws_bytes, void* stream);
size_t ic_conv_transpose2d_fwd_ws_ex(const ic_act* x, int k, int stride, int pad, const ic_act* y, int math);
int ic_conv_transpose2d_fwd_ex(const ic_act* x, const float* w, const float* b, int k, int stride, int pad,
                               const ic_act* y, int act, int math, void* ws, size_t ws_bytes, void* stream);
size_t ic_conv_transpose2d_dgrad_ws_ex(const ic_act* dy, int k, int stride, int pad, const ic_act* dx,
                                       int math);
int ic_conv_transpose2d_dgrad_ex(const ic_act* dy, const float* w, int k, int stride, int pad,
                                 const ic_act* dx, int math, void* ws, size_t ws_bytes, void* stream);

/* weight gradients with a math mode: IC_MATH_SPLIT runs the split kernel on 192-channel-tile NHWC
 * operands (>= 128 channels each side), the fp32 kernel otherwise; IC_MATH_BF16 runs bf16 operands with
 * fp32 accumulation on the same operands where the two-wave kernel applies (output maps >= 16 wide,
 * row-aligned 32-pixel steps) and falls back to split arithmetic (when IC_MATH_SPLIT is also set) or
 * fp32 elsewhere. */
size_t ic_conv2d_wgrad_ws_ex(const ic_act* x, const ic_act* dy, int k, int stride, int pad, int math);
int ic_conv2d_wgrad_ex(const ic_act* x, const ic_act* dy, int k, int stride, int pad, float* dw, float* db,
                       int math, void* ws, size_t ws_bytes, void* stream);
size_t ic_conv_transpose2d_wgrad_ws_ex(const ic_act* x, const ic_act* dy, int k, int stride, int pad, int math);
int ic_conv_transpose2d_wgrad_ex(const ic_act* x, const ic_act* dy, int k, int stride, int pad, float* dw,
                                 float* db, int math, void* ws, size_t ws_bytes, void* stream);

/* ---- GDN: norm = beta + conv1x1(x^2, gamma); y = x / sqrt(norm) (inverse: x * sqrt(norm)).
 *      gamma [C][C], beta [C] (already re-parameterised); x, y, norm share one layout. */
size_t ic_gdn_fwd_ws(const ic_act* x);
int ic_gdn_fwd(const ic_act* x, const float* gamma, const float* beta, int inverse,
               const ic_act* y, float* norm, void* ws, size_t ws_bytes, void* stream);
size_t ic_gdn_bwd_ws(const ic_act* x);
int ic_gdn_bwd(const ic_act* x, const float* norm, const float* dy, const float* gamma, int inverse,
               const ic_act* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
               void* stream);
/* math = IC_MATH_SPLIT (C % 32 == 0, C >= 64, channel-contiguous): the forward runs in split arithmetic —
 * the fused kernel for NHWC-dense C = 192, otherwise the split implicit GEMM (x^2 squared in its staging,
 * the divide in its epilogue) where x takes its fast form (16-byte aligned base and pixel strides), fp32 where
 * not.  NHWC-dense: channel stride 1 and pixel stride C over every dimension above size 1 (the stride of a
 * dimension of size 1 is not looked at, here and for the compact NHWC copies below). */
size_t ic_gdn_fwd_ws_ex(const ic_act* x, int math);
int ic_gdn_fwd_ex(const ic_act* x, const float* gamma, const float* beta, int inverse, const ic_act* y, float* norm,
                  int math, void* ws, size_t ws_bytes, void* stream);
/* math = IC_MATH_SPLIT: the fused backward (C = 192) forms dgamma in split arithmetic (fp32 via three bf16
 * terms on the bf16 MFMA), dx on the fp32 MFMA.  math = IC_MATH_BF16 (C = 192, config C3): both of its
 * GEMMs (dx's q.gamma and dgamma's q^T x^2) on bf16 operands with fp32 accumulation.  Other shapes stay
 * on the fp32 MFMA. */
int ic_gdn_bwd_ex(const ic_act* x, const float* norm, const float* dy, const float* gamma, int inverse,
                  const ic_act* dx, float* dgamma, float* dbeta, int math, void* ws, size_t ws_bytes, void* stream);
/* ic_gdn_bwd_ex plus dxsum[c] = sum over all pixels of dx[.,c,.,.] (C floats): the bias gradient of
 * the convolution that produced the GDN input (reference analysis.py / synthesis.py: conv -> GDN),
 * formed by the fused backward from its dx tiles instead of a separate pass over dx.  Same workspace
 * as ic_gdn_bwd_ws. */
int ic_gdn_bwd_sum_ex(const ic_act* x, const float* norm, const float* dy, const float* gamma, int inverse,
                      const ic_act* dx, float* dgamma, float* dbeta, float* dxsum, int math, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- bf16 activation copies (config C3, round 5): a GDN forward / backward whose output feeds a
 *      192 -> 192 conv forward / transposed-conv input gradient on the bf16 DMA tiles also writes that
 *      output as a compact NHWC bf16 copy (round to nearest even: the operand the conv would form);
 *      the conv reads the copy (2 B per element, nothing converted).  y / dx must be compact NHWC
 *      (channel stride 1), C % 8 == 0.  Replace (reference modelling/layers/gdn.py:79-88 feeding
 *      modelling/blocks/analysis.py:55, synthesis.py:55-57) the plain forms above. */
int ic_gdn_fwd_xb(const ic_act* x, const float* gamma, const float* beta, int inverse, const ic_act* y, float* norm,
                  void* yb, int math, void* ws, size_t ws_bytes, void* stream);
int ic_gdn_bwd_sum_xb(const ic_act* x, const float* norm, const float* dy, const float* gamma, int inverse,
                      const ic_act* dx, float* dgamma, float* dbeta, float* dxsum, void* dxb, int math, void* ws,
                      size_t ws_bytes, void* stream);
/* ---- norm recomputed (config C3, round 6): the GDN forward with bf16 operands (IC_MATH_BF16 | IC_MATH_SPLIT,
 *      C = 192, NHWC-dense) can leave norm = beta + Gamma x^2 out, and the backward forms it again per tile
 *      from x, Gamma and beta -- the forward's operands, products and order, so bitwise the same norm.  Both
 *      kernels are HBM-bound there; together they move 24 instead of 32 bytes per element.  yb / dxb: the
 *      optional bf16 copies of ic_gdn_fwd_xb / ic_gdn_bwd_sum_xb (NULL: none).  Any other math mode, C or
 *      layout is IC_ERR_ARG.  Workspaces: ic_gdn_fwd_ws_ex / ic_gdn_bwd_ws.  Replace (reference
 *      modelling/layers/gdn.py:79-88) ic_gdn_fwd_xb / ic_gdn_bwd_sum_xb in C3's training step. */
int ic_gdn_fwd_rn(const ic_act* x, const float* gamma, const float* beta, int inverse, const ic_act* y, void* yb,
                  int math, void* ws, size_t ws_bytes, void* stream);
int ic_gdn_bwd_sum_rn(const ic_act* x, const float* beta, const float* dy, const float* gamma, int inverse,
                      const ic_act* dx, float* dgamma, float* dbeta, float* dxsum, void* dxb, int math, void* ws,
                      size_t ws_bytes, void* stream);
/* xb / dyb: the input's bf16 copy (NULL is an error; the workspace from *_ws_ex with math | IC_MATH_XB) */
int ic_conv2d_fwd_xb(const ic_act* x, const void* xb, const float* w, const float* b, int k, int stride, int pad,
                     const ic_act* y, int act, int math, void* ws, size_t ws_bytes, void* stream);
int ic_conv_transpose2d_dgrad_xb(const ic_act* dy, const void* dyb, const float* w, int k, int stride, int pad,
                                 const ic_act* dx, int math, void* ws, size_t ws_bytes, void* stream);
/* the same for the phases of a transposed conv forward / conv input gradient (stride-2 sub-pixel phases on
 * the DMA tiles where every phase has >= 256 tiles of 256 rows) */
int ic_conv_transpose2d_fwd_xb(const ic_act* x, const void* xb, const float* w, const float* b, int k, int stride,
                               int pad, const ic_act* y, int act, int math, void* ws, size_t ws_bytes, void* stream);
int ic_conv2d_dgrad_xb(const ic_act* dy, const void* dyb, const float* w, int k, int stride, int pad,
                       const ic_act* dx, int math, void* ws, size_t ws_bytes, void* stream);
/* weight gradients reading both operands' bf16 copies (x's from its producer's forward, dy's from its
 * producer's backward); workspace from *_wgrad_ws_ex */
int ic_conv2d_wgrad_xb(const ic_act* x, const void* xb, const ic_act* dy, const void* dyb, int k, int stride, int pad,
                       float* dw, float* db, int math, void* ws, size_t ws_bytes, void* stream);
int ic_conv_transpose2d_wgrad_xb(const ic_act* x, const void* xb, const ic_act* dy, const void* dyb, int k,
                                 int stride, int pad, float* dw, float* db, int math, void* ws, size_t ws_bytes,
                                 void* stream);

/* ---- launch-plan query: which kernel instance, tile and K / pixel split a conv or GDN op would launch
 *      for these shapes (no launch, no device access; the same decision code as the launching entry
 *      points).  op selects the entry point and the meaning of (a, b):
 *        IC_OP_CONV2D_FWD   a = x,  b = y     IC_OP_TCONV_FWD    a = x,  b = y
 *        IC_OP_CONV2D_DGRAD a = dy, b = dx    IC_OP_TCONV_DGRAD  a = dy, b = dx
 *        IC_OP_CONV2D_WGRAD a = x,  b = dy    IC_OP_TCONV_WGRAD  a = x,  b = dy
 *        IC_OP_GDN_FWD      a = x (b unused; k, stride, pad ignored)    IC_OP_GDN_BWD  likewise
 *      Returns 0 and fills *out, or IC_ERR_ARG for shapes the launch would reject (including tensors
 *      whose element offsets exceed the kernels' 32-bit indexing).  Used by the parity tests to prove
 *      they reach the kernel instances the benchmark runs. */
#define IC_OP_CONV2D_FWD 0
#define IC_OP_CONV2D_DGRAD 1
#define IC_OP_CONV2D_WGRAD 2
#define IC_OP_TCONV_FWD 3
#define IC_OP_TCONV_DGRAD 4
#define IC_OP_TCONV_WGRAD 5
#define IC_OP_GDN_FWD 6
#define IC_OP_GDN_BWD 7
/* kernel ids */
#define IC_KERNEL_IG_FP32 1         /* ig_kernel: implicit GEMM on the fp32 MFMA */
#define IC_KERNEL_IG_FP32_GATHER 2  /* ig_kernel, flattened (tap, channel) gather */
#define IC_KERNEL_IG_BF16 3         /* ig_kernel_bf16: bf16 operands, 64-channel chunks */
#define IC_KERNEL_IG_SPLIT 4        /* ig_kernel_x3s: fp32 by the exact three-term bf16 split */
#define IC_KERNEL_IG_SPLIT_BF16 5   /* ig_kernel_x3s with one bf16 product (bf16 operands) */
#define IC_KERNEL_EDGE_CONV 6       /* edge_conv_kernel: few-channel image -> wide map */
#define IC_KERNEL_IM2COL_GEMM 7     /* im2col columns + ig_kernel */
#define IC_KERNEL_TCONV_FEW 8       /* tconv_few_kernel: wide map -> few-channel image, output-row stationary */
#define IC_KERNEL_TCONV_FEW_ROWS 9  /* tconv_few2_kernel: the same, input-row stationary */
#define IC_KERNEL_GEMM_COL2IM 10    /* ig_kernel + col2im gather */
#define IC_KERNEL_WG_FP32 11        /* wg_kernel: weight gradient on the fp32 MFMA */
#define IC_KERNEL_WG_FP32_GATHER 12 /* wg_kernel, flattened (tap, channel) columns */
#define IC_KERNEL_WG_LDSDMA 13      /* wg_glds_kernel: fp32 MFMA, LDS-DMA staged */
#define IC_KERNEL_WG_SPLIT 14       /* wg_x3d_kernel (two waves per SIMD, maps >= 32 wide) / wg_x3_kernel:
                                       weight gradient in split arithmetic */
#define IC_KERNEL_EDGE_WGRAD 15     /* edge_wgrad_kernel */
#define IC_KERNEL_GDN_FUSED 16      /* gdn_fwd_fused_kernel / gdn_bwd_fused_kernel (fp32 dx) */
#define IC_KERNEL_GDN_FUSED_SPLIT 17 /* gdn_fwd_x3s_kernel / gdn_bwd_fused_kernel with split dgamma */
#define IC_KERNEL_GDN_GEMM 18       /* GDN on the implicit GEMM (+ wgrad kernel for dgamma) */
/* 19: retired (a halo-reusing split kernel, measured slower) */
#define IC_KERNEL_WG_BF16 20        /* wg_x3d_kernel with bf16 operands (one product), fp32 accumulation */
#define IC_KERNEL_GDN_FUSED_BF16 21 /* gdn_bwd_fused_kernel with bf16 operands in both GEMMs */
#define IC_KERNEL_IG_SPLIT_DMA 22   /* ig_kernel_x3d: split arithmetic, 256-row tiles, operands by LDS-DMA */
#define IC_KERNEL_EDGE_CONV_BF16 23 /* edge_conv_x3_kernel with bf16 operands (one product), fp32 accumulation */
#define IC_KERNEL_TCONV_FEW_ROWS_BF16 24 /* tconv_few2_kernel with bf16 operands (one product) */
#define IC_KERNEL_EDGE_WGRAD_BF16 25 /* edge_wgrad_kernel with bf16 operands (one product) */
#define IC_KERNEL_IG_BF16_DMA 26    /* ig_kernel_b16d: bf16 operands, 256-row tiles, operands by LDS-DMA (C3) */
typedef struct ic_plan {
  int kernel;        /* IC_KERNEL_* of the main launch */
  int bm, bn;        /* block tile: output rows (pixels; weight-gradient: G channels) x columns */
  int ksplit;        /* implicit GEMM K splits (1 = none; > 1 adds a deterministic partial-sum pass) */
  int nsplit;        /* weight gradient pixel splits (0 for other ops) */
  int im2col;        /* 1 when a column buffer is materialised in HBM */
  int variant;       /* kernel-specific template variant (weight gradient: 1 = row-fast addressing;
                        edge conv, edge weight gradient, input-row transposed conv: 1 = split arithmetic) */
  long long blocks;  /* workgroups of the main launch (-1 when not reported) */
} ic_plan;
int ic_conv_plan(int op, const ic_act* a, const ic_act* b, int k, int stride, int pad, int math, ic_plan* out);

/* ---- elementwise on dense storage of n elements ---- */
/* NonNegativeParam: v = max(p, bound); out = v*v - ped */
int ic_nonneg_fwd(const float* p, long long n, float bound, float ped, float* out, void* stream);
int ic_nonneg_bwd(const float* p, const float* gout, long long n, float bound, float* gin, void* stream);
/* NonNegativeParam of several tensors in one launch (a training step's GDN gamma / beta:
 * reference gdn.py:59-62, called once per GDN layer): per tensor, backward = 0 -> out = max(p,
 * bound)^2 - pedestal; backward = 1 -> gin = the gradient of ic_nonneg_bwd given gout.  Bitwise the
 * per-tensor entry points. */
typedef struct ic_nonneg_tensor {
  const float* p;
  float* out;          /* forward output (unused in the backward) */
  const float* gout;   /* backward: dL/dout */
  float* gin;          /* backward: dL/dp */
  long long n;
  float bound;
  float pedestal;
} ic_nonneg_tensor;
int ic_nonneg_multi(const ic_nonneg_tensor* tensors, int ntensors, int backward, void* stream);
/* LowerBound (upper=0): max(x,b); UpperBound (upper=1): min(x,b) — with the reference's
 * pass-through gradients */
int ic_bound_fwd(const float* x, long long n, float bound, int upper, float* y, void* stream);
int ic_bound_bwd(const float* x, const float* g, long long n, float bound, int upper, float* gx,
                 void* stream);
int ic_relu_fwd(const float* x, long long n, float* y, void* stream);
int ic_relu_bwd(const float* y, const float* g, long long n, float* gx, void* stream);
int ic_abs_fwd(const float* x, long long n, float* y, void* stream);
int ic_abs_bwd(const float* x, const float* g, long long n, float* gx, void* stream);
/* sigma = clamp(exp(v), lo, hi); saves e = exp(v) for the backward */
int ic_exp_clamp_fwd(const float* v, long long n, float lo, float hi, float* sigma, float* e,
                     void* stream);
int ic_exp_clamp_bwd(const float* e, const float* g, long long n, float lo, float hi, float* gv,
                     void* stream);

/* ---- reductions (deterministic, two-level) ---- */
size_t ic_reduce_ws(long long n);
/* out[0] = sum clamp(-ln(p+1e-10)/ln2, 0, 50) */
int ic_ce_loss_fwd(const float* p, long long n, float* out, void* ws, size_t ws_bytes, void* stream);
/* gp = gout[0] * d/dp (gout: device scalar) */
int ic_ce_loss_bwd(const float* p, const float* gout, long long n, float* gp, void* stream);
/* out[0] = mean((a-b)^2) */
int ic_mse_fwd(const float* a, const float* b, long long n, float* out, void* ws, size_t ws_bytes,
               void* stream);
/* ga = gout*2(a-b)/n (NULL to skip), gb = -ga (NULL to skip) */
int ic_mse_bwd(const float* a, const float* b, const float* gout, long long n, float* ga, float* gb,
               void* stream);

/* ---- noise: the training-noise stream (replaces torch.rand_like of entropy_model.py:230,333).
 *      Element i of stream `seed` is word (i & 3) of Philox4x32-10(counter {i >> 2 as 64 bits, 0, 0},
 *      key {seed lo, seed hi}), mapped to U[0,1) by its top 24 bits: u[i] = element offset + i.
 *      offset must be a multiple of 4 (whole Philox blocks; IC_ERR_ARG otherwise). */
int ic_uniform(float* u, long long n, unsigned long long seed, unsigned long long offset,
               void* stream);
/* raw Philox4x32-10 for known-answer tests: in (device) holds n items {c0, c1, c2, c3, k0, k1},
 * out (device) receives n items {r0, r1, r2, r3} */
int ic_philox_kat(const unsigned* in, unsigned* out, int n, void* stream);
/* graph-safe noise stream: a device-resident state {seed, base}; quantizers in
 * mode 3 draw elements base + offset + i of stream seed.  Advancing the base by the
 * elements one training step consumed is itself a kernel, so a captured
 * hipGraph replays with fresh noise every time.  state[1] += n rounded up to a multiple of 4 */
int ic_philox_advance(unsigned long long* state, unsigned long long n, void* stream);

/* ---- factorized entropy model (z): C channels, elements e with channel c = idx % C
 *      (channels-last storage). params (device, fp32, reference shapes flattened):
 *      w0[C*3] b0[C*3] f0[C*3] w1[C*9] b1[C*3] f1[C*3] w2[C*9] b2[C*3] f2[C*3] w3[C*3] b3[C]
 *      mode: 0 = noise with given u (u in [0,1), y = z + (u - 0.5)), 1 = round,
 *            2 = noise from Philox(seed, offset),
 *            3 = noise from Philox(state[0], state[1] + offset) with `u` pointing to the
 *                device state {seed, base} of ic_philox_advance (`seed` ignored).
 *      Modes 2 and 3 take a 4-aligned offset only (IC_ERR_ARG otherwise) and mode 3 a
 *      4-aligned state[1] (ic_philox_advance keeps it so; a caller writing the state
 *      itself must too): every draw is then whole Philox blocks and every quantizer
 *      kernel maps element i to the same counter */
typedef struct ic_fact_params {
  const float *w0, *b0, *f0, *w1, *b1, *f1, *w2, *b2, *f2, *w3, *b3;
} ic_fact_params;
int ic_factorized_fwd(const float* z, long long n, int C, const ic_fact_params* prm, int mode,
                      const float* u, unsigned long long seed, unsigned long long offset,
                      float* q, float* p, void* stream);
/* given dq (NULL = 0) and dp (NULL = 0): dz (= dq + through p) and per-channel
 * parameter gradients (same layout as params; written, not accumulated) */
typedef struct ic_fact_grads {
  float *w0, *b0, *f0, *w1, *b1, *f1, *w2, *b2, *f2, *w3, *b3;
} ic_fact_grads;
int ic_factorized_bwd(const float* q, long long n, int C, const ic_fact_params* prm,
                      const float* dq, const float* dp, float* dz, const ic_fact_grads* grd,
                      void* stream);

/* ---- factorized entropy model, any CDF MLP (cfg.MODEL.ENTROPY_MODEL.DIMS) and BIN
 *      (modelling/blocks/entropy_model.py:88-99 CDFEstimator, :198 / :229-232 / :259-269 BIN):
 *      layer l maps dims[l] -> dims[l+1] channels-wise, dims = {1, DIMS..., 1}; per layer
 *      w[l] [C][dims[l+1]][dims[l]], b[l] [C][dims[l+1]], f[l] [C][dims[l+1]] (NULL on the last
 *      layer: no gate).  Noise u - bin/2, mass between q -+ bin/2.  Modes as ic_factorized_fwd. */
#define IC_FACT_MAXL 6   /* layers (len(DIMS) + 1) the register kernels take */
#define IC_FACT_MAXW 8   /* hidden width the register kernels take */
#define IC_FACT_NET_MAXL 32   /* layers of ic_fact_net: the wide kernels' limit */
#define IC_FACT_WIDE_MAXW 256 /* hidden width of the wide kernels */
typedef struct ic_fact_net {
  int nlayers;
  int dims[IC_FACT_NET_MAXL + 1];
  const float* w[IC_FACT_NET_MAXL];
  const float* b[IC_FACT_NET_MAXL];
  const float* f[IC_FACT_NET_MAXL];
} ic_fact_net;
typedef struct ic_fact_net_grads {
  float* w[IC_FACT_NET_MAXL];
  float* b[IC_FACT_NET_MAXL];
  float* f[IC_FACT_NET_MAXL];
} ic_fact_net_grads;
/* Geometries within IC_FACT_MAXL layers of width <= IC_FACT_MAXW run the register kernels and need no
 * workspace; larger ones (up to IC_FACT_NET_MAXL layers of width <= IC_FACT_WIDE_MAXW) run the wide
 * kernels, whose workspace ic_factorized_net_ws gives (bwd: 0 forward, 1 backward).  The plain entry
 * points are the _ex ones without a workspace (IC_ERR_WORKSPACE on a wide geometry). */
size_t ic_factorized_net_ws(long long n, int C, const ic_fact_net* net, int bwd);
int ic_factorized_fwd_net(const float* z, long long n, int C, const ic_fact_net* net, float bin, int mode,
                          const float* u, unsigned long long seed, unsigned long long offset, float* q, float* p,
                          void* stream);
int ic_factorized_bwd_net(const float* q, long long n, int C, const ic_fact_net* net, float bin, const float* dq,
                          const float* dp, float* dz, const ic_fact_net_grads* grd, void* stream);
int ic_factorized_fwd_net_ex(const float* z, long long n, int C, const ic_fact_net* net, float bin, int mode,
                             const float* u, unsigned long long seed, unsigned long long offset, float* q, float* p,
                             void* ws, size_t ws_bytes, void* stream);
int ic_factorized_bwd_net_ex(const float* q, long long n, int C, const ic_fact_net* net, float bin, const float* dq,
                             const float* dp, float* dz, const ic_fact_net_grads* grd, void* ws, size_t ws_bytes,
                             void* stream);

/* ---- quantization of the conditional model alone (entropy_model.py:331-336): q = y + (u - bin/2)
 *      (modes 0 / 2 / 3 as ic_conditional_fwd, the same draws element for element) or round(y) (mode 1) */
int ic_quantize(const float* y, long long n, int mode, const float* u, unsigned long long seed,
                unsigned long long offset, float bin, float* q, void* stream);

/* ---- conditional (Laplacian kind=0 / Gaussian kind=1), mean = 0 or tensor ----
 *      q = y + (u - 0.5) (mode 0), round(y) (mode 1), Philox (mode 2), Philox on the
 *      device state `u` (mode 3, as for ic_factorized_fwd)
 *      p = F((0.5-|q-mean|)/scale) - F((-0.5-|q-mean|)/scale) */
int ic_conditional_fwd(const float* y, const float* scale, const float* mean, long long n, int kind,
                       int mode, const float* u, unsigned long long seed,
                       unsigned long long offset, float* q, float* p, void* stream);
int ic_conditional_bwd(const float* q, const float* scale, const float* mean, long long n, int kind,
                       const float* dq, const float* dp, float* dy, float* dscale, float* dmean,
                       void* stream);
/* the same with the quantization bin of cfg.MODEL.ENTROPY_MODEL.BIN (the plain entry points: 1):
 * noise u - bin/2, p = F((bin/2-|q-mean|)/scale) - F((-bin/2-|q-mean|)/scale)
 * (entropy_model.py:278, :331-334, :343-350) */
/* mode 4 (the _bin entry points): y is already quantized, q = y -- the likelihood half of the model
 * after ic_quantize (the model runs the hyperprior on a second stream meanwhile) */
int ic_conditional_fwd_bin(const float* y, const float* scale, const float* mean, long long n, int kind, int mode,
                           const float* u, unsigned long long seed, unsigned long long offset, float bin, float* q,
                           float* p, void* stream);
int ic_conditional_bwd_bin(const float* q, const float* scale, const float* mean, long long n, int kind, float bin,
                           const float* dq, const float* dp, float* dy, float* dscale, float* dmean, void* stream);

/* ---- optimizer: multi-tensor AdamW with fused clip_grad_value_ ----
 * torch.optim.AdamW (solver/optim.py:20-45: per-parameter lr / weight_decay
 * groups) preceded by clip_grad_value_(clip) (engine/trainer.py:189-190; clip
 * <= 0 disables it; clipped gradients are written back).  `step` is the
 * 1-based step count used for the bias corrections (betas in double, like the
 * reference's Python floats).  All pointers device fp32. */
typedef struct ic_adamw_tensor {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long n;
  float lr;
  float weight_decay;
} ic_adamw_tensor;
int ic_adamw_step(const ic_adamw_tensor* tensors, int ntensors, double beta1, double beta2, float eps,
                  float clip, long long step, void* stream);

/* ---- SSIM / MS-SSIM (modelling/loss.py:48-188) on [N][C][H][W] contiguous images in [0,1].
 *      nlev levels (MS-SSIM: 5, weights[nlev] host array; single=1 for SSIMLoss, nlev=1).
 *      out: log_scale && single -> out[N] = -log(max(ssim_n, eps)); else out[0] = loss.
 *      single = 2 (with log_scale = 0, eps = 0): the evaluation metric of
 *      utils/metric.py:100-124 — out[N] = -10 log10(1 - prod_l max(cs_l,0)^w_l * max(ssim,0)^w_L)
 *      per image (MS_SSIM(in_dB=True), images scaled by max_val); forward only.
 *      `state` (ic_msssim_state_bytes) is written by fwd and read by bwd. */
size_t ic_msssim_state_bytes(int N, int C, int H, int W, int nlev, int filter_size);
size_t ic_msssim_ws(int N, int C, int H, int W, int nlev, int filter_size);
int ic_msssim_fwd(const float* a, const float* b, int N, int C, int H, int W, int nlev, int filter_size,
                  float filter_sigma, float max_val, int log_scale, int single, float k1, float k2,
                  float eps, const float* weights, float* out, float* state, void* ws, size_t ws_bytes,
                  void* stream);
int ic_msssim_bwd(int N, int C, int H, int W, int nlev, int filter_size, float filter_sigma,
                  float max_val, int log_scale, int single, float k1, float k2, float eps,
                  const float* weights, const float* gout, const float* state, float* ga, float* gb,
                  void* ws, size_t ws_bytes, void* stream);

/* ---- evaluation metric: per-image PSNR in dB (utils/metric.py:26-36) of images scaled by
 *      max_val: out[n] = 10 (2 log10(max_val) - log(mse_n) / ln 10), a, b [N][per_image] ---- */
int ic_psnr(const float* a, const float* b, int N, long long per_image, float max_val, float* out, void* stream);
/* the same over 128 blocks per image: partials in ws (ic_psnr_ws bytes), summed in fixed order
 * (deterministic); N <= 65535 */
size_t ic_psnr_ws(int N, long long per_image);
int ic_psnr_ex(const float* a, const float* b, int N, long long per_image, float max_val, float* out, void* ws,
               size_t ws_bytes, void* stream);

/* ---- host data path: uint8 HWC images (byte strides sn, sh, sw; channel stride 1) -> fp32
 *      NCHW model input (x/255 - mean[c]) / std[c] (transforms.py ToTensor, ChannelFirst,
 *      Normalize; mean/std host arrays of C <= 3 values or NULL for 0 / 1) ---- */
int ic_images_u8_to_input(const unsigned char* x, long long sn, long long sh, long long sw, int N, int C, int H,
                          int W, const float* mean, const float* std, float* y, void* stream);

/* ---- elementwise squared difference (MSE with reduction="none") ---- */
int ic_sqdiff_fwd(const float* a, const float* b, long long n, float* out, void* stream);
int ic_sqdiff_bwd(const float* a, const float* b, const float* g, long long n, float* ga, float* gb,
                  void* stream);

/* ---- entropy coder: wave64-interleaved rANS over quantized CDF tables (the bitstream format is
 *      specified in image_compression_amd/codec.py, the table rule in DESIGN.md).  Symbols are
 *      int32 k in [-K, K], K <= IC_CODEC_KMAX; a table is [rows][2K+2] cumulative counts, 0 first,
 *      strictly increasing, 65536 last.  A chunk is 64 * steps_per_chunk consecutive symbols coded
 *      by one wavefront.  These entry points serve compress / decompress, not the training step;
 *      ic_codec_symbolize is the one entry point of the library that waits for its stream. ---- */
#define IC_CODEC_KMAX 2047  /* 2K+1 <= 4095 counts >= 1 inside a 16-bit total */
#define IC_CODEC_MAXL 256   /* scale-table rows (uint8 row indices) */
#define IC_CODEC_MAXR 65536 /* steps per chunk */
/* sym[i] = (int)rintf(x[i]) and *kmax_dev = max |sym| (device int); copies it to *kmax_host and
 * waits for the stream.  IC_ERR_ARG (with *kmax_host set) when it exceeds IC_CODEC_KMAX. */
int ic_codec_symbolize(const float* x, long long n, int* sym, int* kmax_dev, int* kmax_host, void* stream);
/* rows[i] = number of mids[0 .. L-2] (host fp32, ascending) strictly below sigma[i]: the nearest of L
 * table scales when mids are the midpoints of neighbouring scales */
int ic_codec_scale_index(const float* sigma, long long n, const float* mids, int L, unsigned char* rows,
                         void* stream);
/* pmf [rows][2K+1] fp32 -> cdf [rows][2K+2] uint32 (normalise, floor with every count >= 1,
 * the remainder to the largest count) */
int ic_codec_build_tables(const float* pmf, int rows, int K, unsigned int* cdf, void* stream);
long long ic_codec_chunks(long long n, int steps_per_chunk);     /* ceil(n / (64 * steps_per_chunk)); 0: bad arguments */
size_t ic_codec_encode_ws(long long n, int steps_per_chunk);     /* chunks * (2 * 64 * steps_per_chunk + 256) bytes */
size_t ic_codec_compact_bytes(long long n, int steps_per_chunk); /* 4 * chunks + the encode workspace: the worst case */
/* The row of symbol i is rows[i], or i % C where rows is NULL.  Each chunk is coded into its own slot of
 * ws, ending at the slot's end; lengths[chunk] (device) = its bytes. */
int ic_codec_encode(const int* sym, long long n, const unsigned char* rows, int C, const unsigned int* cdf,
                    int nrows, int K, int steps_per_chunk, void* ws, size_t ws_bytes, unsigned int* lengths,
                    void* stream);
/* out = [lengths: chunks x u32 little endian][chunk 0][chunk 1]... (offsets: exclusive scan of lengths) */
int ic_codec_compact(const void* ws, const unsigned int* lengths, long long n, int steps_per_chunk, void* out,
                     size_t out_bytes, void* stream);
/* in = the layout ic_codec_compact writes, in_bytes long (device); out[i] = symbol i as a float.  Reads of
 * `in` stay inside each chunk's [begin, end) clamped to in_bytes, table searches inside the row: any
 * payload decodes to some symbols in [-K, K]. */
int ic_codec_decode(const void* in, size_t in_bytes, long long n, const unsigned char* rows, int C,
                    const unsigned int* cdf, int nrows, int K, int steps_per_chunk, float* out, void* stream);

/* ---- segmented entropy coder (per-image streams; additive to version 4).  nseg segments (images) of
 *      seg_len symbols each lie back to back; segment s has its own K = seg_k[s] and its own table
 *      [nrows][2 seg_k[s] + 2] at word offset seg_off[s] of `pool` (device, pool_words uint32 long; segments
 *      with the same K may share a table).  seg_k / seg_off are host arrays, checked before any launch and
 *      then copied as (K, offset) pairs into seg_dev (device, 2 * nseg ints).  Chunks never straddle a
 *      segment: each has ceil(seg_len / (64 * steps_per_chunk)) chunks, the last possibly short, and the
 *      bytes of segment s are exactly what ic_codec_encode writes for its symbols alone.  Row of symbol g
 *      (index over all segments): rows[g], or g % C where rows is NULL (then seg_len % C must be 0). ---- */
long long ic_codec_seg_chunks(int nseg, long long seg_len, int steps_per_chunk);      /* nseg * chunks per segment; 0: bad arguments */
size_t ic_codec_encode_seg_ws(int nseg, long long seg_len, int steps_per_chunk);      /* chunks * (2 * 64 * steps_per_chunk + 256) bytes */
size_t ic_codec_compact_seg_bytes(int nseg, long long seg_len, int steps_per_chunk);  /* 4 * chunks + the encode workspace */
/* sym = rint(x) and kmax_dev[s] = max |sym| of segment s (device, nseg ints; integer atomic maximum); one
 * copy of the nseg maxima to kmax_host and one wait for the stream.  IC_ERR_ARG (with kmax_host filled)
 * when any exceeds IC_CODEC_KMAX. */
int ic_codec_symbolize_seg(const float* x, int nseg, long long seg_len, int* sym, int* kmax_dev, int* kmax_host,
                           void* stream);
/* One wavefront per chunk over all nseg * chunks-per-segment chunks, (segment, chunk) order; a block stages
 * its own segment's table in LDS when nrows * (2K + 2) * 4 <= 48 KiB and reads it from `pool` otherwise. */
int ic_codec_encode_seg(const int* sym, int nseg, long long seg_len, const unsigned char* rows, int C,
                        const unsigned int* pool, size_t pool_words, int nrows, const int* seg_k,
                        const long long* seg_off, int* seg_dev, int steps_per_chunk, void* ws, size_t ws_bytes,
                        unsigned int* lengths, void* stream);
/* ic_codec_compact for an explicit chunk count: out = [all chunk lengths][all chunk bytes] */
int ic_codec_compact_seg(const void* ws, const unsigned int* lengths, long long chunks, int steps_per_chunk, void* out,
                         size_t out_bytes, void* stream);
/* in = [the segments' chunk lengths, (segment, chunk) order][their chunk bytes, same order]: the streams of
 * nseg images of one tensor kind, concatenated.  The guarantees of ic_codec_decode hold per segment: any
 * bytes decode to some symbols in [-seg_k[s], seg_k[s]]. */
int ic_codec_decode_seg(const void* in, size_t in_bytes, int nseg, long long seg_len, const unsigned char* rows, int C,
                        const unsigned int* pool, size_t pool_words, int nrows, const int* seg_k,
                        const long long* seg_off, int* seg_dev, int steps_per_chunk, float* out, void* stream);

/* ---- image borders of the per-image streams.  ic_pad_edge: x (N, C, h, w) dense NCHW -> y (N, C, Hp, Wp)
 *      dense NCHW, y[n,c,i,j] = x[n,c,min(i,h-1),min(j,w-1)].  ic_crop_clamp: x (any strides) -> y (N, C, h, w)
 *      dense NCHW, y = max(min(x, 1), 0) on the top-left h x w: ic_bound_fwd upper 1 then lower 0, cropped. ---- */
int ic_pad_edge(const float* x, int N, int C, int h, int w, int Hp, int Wp, float* y, void* stream);
int ic_crop_clamp(const ic_act* x, int h, int w, float* y, void* stream);

/* ---- mean-scale hyperprior (additive to version 4): y is coded about a mean mu = h_s(z_hat).  y and mu are
 *      dense storage of the same n elements in the same order (the caller checks the counts).  d = y - mu is
 *      one fp32 subtraction and y_hat = r + mu one fp32 addition, neither contracted with anything, so
 *      ic_add_mean gives the bits ic_center_round gives for the same r and mu. ---- */
/* ic_codec_symbolize with sym[i] = the symbol of y[i] - mu[i] (same clamp-and-NaN rule, same kmax contract) */
int ic_codec_symbolize_mean(const float* y, const float* mu, long long n, int* sym, int* kmax_dev, int* kmax_host,
                            void* stream);
/* ic_codec_symbolize_seg likewise: kmax_dev[s] / kmax_host[s] = max |sym| of segment s */
int ic_codec_symbolize_mean_seg(const float* y, const float* mu, int nseg, long long seg_len, int* sym, int* kmax_dev,
                                int* kmax_host, void* stream);
/* r[i] = rintf(y[i] - mu[i]) as the float the decoder will hold (a -0.0 is written as +0.0), y_hat[i] = r[i] + mu[i]:
 * the eval-mode quantiser (r and y_hat distinct buffers) */
int ic_center_round(const float* y, const float* mu, long long n, float* r, float* y_hat, void* stream);
/* y_hat[i] = r[i] + mu[i]: the decoder's reconstruction from the float integers r it decoded */
int ic_add_mean(const float* r, const float* mu, long long n, float* y_hat, void* stream);

/* ---- checkerboard context model (additive to version 4).  Every tensor is dense channels-last storage
 *      (n, i, j, c) of N x H x W x C elements (H, W: the latent map's), indexed in 64 bits; position (i, j) is an
 *      anchor when i + j is even, whatever n and c.  `parity` 0 names the anchors, 1 the non-anchors.  IC_ERR_ARG
 *      before any launch for a null pointer, a size below 1, N H W C past 2^63 - 1, a parity outside {0, 1} or
 *      outputs that share a buffer.  None of them allocates or waits for its stream. ---- */
/* the context convs' inputs: u = y and v = |y - mu| (one fp32 subtraction) at the anchors, +0.0 elsewhere */
int ic_ckbd_input_fwd(const float* y, const float* mu, int N, int H, int W, int C, float* u, float* v, void* stream);
/* with s = sign(y - mu) (0 at 0) at the anchors: dy = du + s dv, dmu = -s dv; +0.0 elsewhere */
int ic_ckbd_input_bwd(const float* y, const float* mu, const float* du, const float* dv, int N, int H, int W, int C,
                      float* dy, float* dmu, void* stream);
/* mu = mu_h + a and sigma = sigma_h expf(clamp(b, -4, 4)) at the non-anchors; mu_h and sigma_h, bit for bit, at the
 * anchors */
int ic_ckbd_params_fwd(const float* mu_h, const float* sigma_h, const float* a, const float* b, int N, int H, int W, int C,
                       float* mu, float* sigma, void* stream);
/* dmu_h = dmu; with e = expf(clamp(b)) at the non-anchors da = dmu, dsigma_h = dsigma e, db = dsigma sigma_h e where
 * -4 <= b <= 4 and 0 beyond; at the anchors da = db = 0, dsigma_h = dsigma */
int ic_ckbd_params_bwd(const float* sigma_h, const float* b, const float* dmu, const float* dsigma, int N, int H, int W,
                       int C, float* dmu_h, float* dsigma_h, float* da, float* db, void* stream);
/* positions of that parity in one H x W map (any H, W >= 1); -1: bad arguments */
long long ic_ckbd_count(int H, int W, int parity);
/* dst = the elements (elem_bytes 1 or 4 wide) of src at the positions of that parity, packed in ascending
 * (n, i, j, c) order: N * ic_ckbd_count(H, W, parity) * C elements */
int ic_ckbd_gather(const void* src, int elem_bytes, int N, int H, int W, int C, int parity, void* dst, void* stream);
/* the inverse for floats: writes the packed half to its positions of `full`, the other parity untouched */
int ic_ckbd_scatter(const float* half, int N, int H, int W, int C, int parity, float* full, void* stream);

/* ---- the checkerboard context in one batch-invariant launch (additive to version 4; csrc/ckbd_context.hip).
 *      y_in, mu_h, sigma_h, mu, sigma: N x H x W x C as above; w_mean, w_scale: (C, C, 5, 5) and b_mean, b_scale: (C),
 *      as a Conv2d holds them.  At the anchors mu = mu_h and sigma = sigma_h bit for bit.  At a non-anchor, over the
 *      12 taps (ky, kx) with (ky-2) + (kx-2) odd in ascending order, a neighbour outside the map contributing 0:
 *          a[o] = b_mean[o]  + sum_t sum_c w_mean[o,c,ky,kx]  y_in[c, nbr]
 *          b[o] = b_scale[o] + sum_t sum_c w_scale[o,c,ky,kx] |y_in[c, nbr] - mu_h[c, nbr]|
 *          mu = mu_h + a,  sigma = sigma_h expf(clamp(b, -4, 4))            (ic_ckbd_params_fwd's rule)
 *      in exact fp32 products with fp32 accumulation (fp32 MFMA) whatever the model's arithmetic.  The other 13
 *      taps and the non-anchors of y_in are never read.  Image n's outputs depend on image n's inputs, the
 *      weights and (H, W, C) only -- bit for bit, whatever N and wherever in the batch the image lies: tiles are
 *      cut per image, every sum runs in one fixed order, nothing is split by the launch size, no atomics.
 *      `ws`: 16-byte aligned, at least ic_context_ws(C) bytes; it receives the repacked live taps, and with
 *      `packed` != 0 it already holds them (from an earlier call with these weights) and is only read.
 *      IC_ERR_ARG before any launch for a null pointer, a size below 1, C > IC_CONTEXT_MAXC, N H W C past
 *      2^63 - 1, or an output that shares a buffer with the other output or an input; IC_ERR_WORKSPACE for a short
 *      workspace.  A 1 x 1 map has no non-anchor: nothing is packed and the launch only copies.  Neither allocates
 *      or waits for its stream. ---- */
#define IC_CONTEXT_MAXC 4096
/* bytes of the packed weights; 0: C outside 1 .. IC_CONTEXT_MAXC */
size_t ic_context_ws(int C);
int ic_context_fwd(const float* y_in, const float* mu_h, const float* sigma_h, const float* w_mean,
                        const float* b_mean, const float* w_scale, const float* b_scale, int N, int H, int W, int C,
                        float* mu, float* sigma, void* ws, size_t ws_bytes, int packed, void* stream);

/* ---- h_s as batch-invariant layers (additive to version 4; csrc/hs_invariant.hip).  One call computes one layer
 *      ConvTranspose2d(Cin, Cout, k, stride=s, padding=p=k/2, output_padding=s-1, bias) on x: N x H x W x Cin, dense
 *      channels-last fp32, into out: N x sH x sW x Cout; w: (Cin, Cout, k, k) and b: (Cout) as the module holds them:
 *          out[n,o,i,j] = b[o] + sum_(ky,kx) sum_c w[c,o,ky,kx] x[n,c,(i+p-ky)/s,(j+p-kx)/s]
 *      over the taps whose two quotients are exact; a neighbour outside the map contributes a product with +0.0.
 *      Exact fp32 products with fp32 accumulation (fp32 MFMA) whatever the model's arithmetic.  Every accumulator
 *      starts from the bias and sums in one order that depends on (k, s, Cin) only: the live taps of the output's
 *      phase (i % s, j % s) in ascending (ky, kx); inside a tap the channel groups of 8 in ascending order; inside a
 *      group the channels +0, +4, +1, +5, +2, +6, +3, +7.  No split of K, no atomics, nothing reduced across blocks;
 *      tiles (32 positions of one phase of one image) are cut per image.  So an output's bits depend on the values
 *      its taps see, the weights and (k, s, Cin) only: not on N, H, W, the image's index, or its place in the map.
 *      `epilogue`: IC_HS_NONE; IC_HS_RELU (ic_relu_fwd's bits on the plain output); IC_HS_EXP_CLAMP
 *      (ic_exp_clamp_fwd's bits: expf, then max with lo, then min with hi).  A second head (w2, b2, epilogue2, out2:
 *      all null / 0, or all set; same Cout) on the same input runs in the same launch.
 *      `ws`: 16-byte aligned, at least ic_hs_ws(Cin, Cout, k, s, heads) bytes; it receives the repacked taps, and
 *      with `packed` != 0 it already holds them (from an earlier call with these weights) and is only read.
 *      Served: k odd and <= 5, s 1 or 2, 1 <= Cin, Cout <= IC_HS_MAXC.  IC_ERR_ARG before any launch for anything
 *      else, a null pointer, a size below 1, an unknown epilogue, an element count past 2^63 - 1, or an output of which
 *      any byte lies in an input, the workspace or the other output; IC_ERR_WORKSPACE for a short workspace.  Neither
 *      allocates or waits for its stream. ---- */
#define IC_HS_MAXC 4096
#define IC_HS_NONE 0
#define IC_HS_RELU 1
#define IC_HS_EXP_CLAMP 2
/* bytes of the packed weights of `heads` (1 or 2) heads; 0: a geometry that is not served */
size_t ic_hs_ws(int Cin, int Cout, int k, int s, int heads);
int ic_hs_layer(const float* x, int N, int H, int W, int Cin, int Cout, int k, int s, const float* w, const float* b,
                int epilogue, float* out, const float* w2, const float* b2, int epilogue2, float* out2, float lo,
                float hi, void* ws, size_t ws_bytes, int packed, void* stream);

/* ---- gain units (additive to version 4; GainedMeanScaleCompressor2018).  The gain-vector rule: for a table t
 *      (S, C), S >= 2, and a quality q in [0, S-1] held as fp32: s = min((int)floorf(q), S-2), f = q - s,
 *      a = fma(f, t[s+1][c], fl((1-f) t[s][c])): 1-f and the lower level's product rounded once each, the upper
 *      level's product fused with the sum and rounded once; g[c] = 1.0f where a == 0 and expf(a) elsewhere.  `q` is a host array.  IC_ERR_ARG before any launch for a null pointer, S < 2, C or
 *      nq < 1, or a quality that is NaN or outside [0, S-1].  None of them allocates or waits for its stream. ---- */
/* out[k][c] = the gain of channel c at quality q[k]: (nq, C) */
int ic_gain_vector(const float* table, int S, int C, const float* q, int nq, float* out, void* stream);
/* dtable (S, C) from g = ic_gain_vector's output and dout, both (nq, C): one thread per (s, c) sums over k in
 * ascending order */
int ic_gain_vector_bwd(const float* g, const float* dout, int S, int C, const float* q, int nq, float* dtable,
                       void* stream);
/* x, out: dense (N, P, C) storage, P positions per image, channel fastest; g: (g_rows, C) with g_rows 1 (one gain
 * for every image) or N (image n takes row n); 1 <= N <= 65535.  out[n,p,c] = x[n,p,c] * g[g_rows == 1 ? 0 : n][c],
 * one fp32 multiplication */
int ic_channel_scale(const float* x, const float* g, long long N, long long P, int C, int g_rows, float* out,
                     void* stream);
/* dx = dy * g (the forward's multiplication) and dg[row][c] = the sum of dy x over the positions (and the images,
 * when the row is shared): partial sums per block of positions in `ws`, then one thread per (row, c) over them in
 * ascending order -- no atomics, bitwise the same from run to run.  The query returns 0 for a shape the call refuses */
size_t ic_channel_scale_bwd_ws(long long N, long long P, int C, int g_rows);
int ic_channel_scale_bwd(const float* x, const float* g, const float* dy, long long N, long long P, int C, int g_rows,
                         float* dx, float* dg, void* ws, size_t ws_bytes, void* stream);

/* ---- region-of-interest coding (additive to version 4; RegionGainedMeanScaleCompressor2018).  A block map `idx`
 *      holds one uint8 rank per block of 2^shift x 2^shift positions, (N, ceil(Hm / 2^shift), ceil(Wm / 2^shift)):
 *      position (i, j) of image n takes row idx[n, i >> shift, j >> shift] of R rows, 1 <= R <= 256.  A rank >= R is
 *      clamped to R - 1.  IC_ERR_ARG before any launch for a null pointer, R outside 1 .. 256, N outside 1 .. 65535,
 *      an extent below 1, Hm Wm C >= 2^31 or a shift outside 0 .. 6.  None of them allocates or waits for its stream; no
 *      floating-point atomics, every sum in a fixed order. ---- */
/* x, out: dense (N, Hm, Wm, C) storage, channel fastest; g: (R, C).  out[n,i,j,c] = x[n,i,j,c] * g[rank][c], one
 * fp32 multiplication */
int ic_block_scale(const float* x, const float* g, int R, const unsigned char* idx, int N, int Hm, int Wm, int C,
                   int shift, float* out, void* stream);
/* dx = dy * g[rank] and dg[r][c] = the sum of dy x over the positions whose block has rank r (+0.0 for a rank no
 * block has): per block over its positions in ascending (i, j) into `ws`, then one thread per (r, c) over the blocks
 * in ascending (n, bi, bj).  The query returns 0 for a shape the call refuses */
size_t ic_block_scale_bwd_ws(int N, int Hm, int Wm, int C, int shift);
int ic_block_scale_bwd(const float* x, const float* g, int R, const unsigned char* idx, const float* dy, int N, int Hm,
                       int Wm, int C, int shift, float* dx, float* dg, void* ws, size_t ws_bytes, void* stream);
/* a, b: images (N, C, H, W) that share the strides (sn, sc, sh, sw), each >= 1, C H W < 2^31; w: R weights on the
 * device; idx: the pixel block map, shift 6.  out[0] = sum of w[rank] (a-b)^2 / n, out[1] = sum of (a-b)^2 / n,
 * n = N C H W, from one pass */
size_t ic_block_mse_ws(int N, int C, int H, int W);
int ic_block_mse_fwd(const float* a, const float* b, const float* w, int R, const unsigned char* idx, int N, int C, int H,
                     int W, long long sn, long long sc, long long sh, long long sw, float* out, void* ws, size_t ws_bytes,
                     void* stream);
/* ga = gout[0] 2 w[rank] (a-b) / n (NULL to skip), gb = -ga (NULL to skip; not both), with the inputs' strides */
int ic_block_mse_bwd(const float* a, const float* b, const float* w, int R, const unsigned char* idx, const float* gout,
                     int N, int C, int H, int W, long long sn, long long sc, long long sh, long long sw, float* ga,
                     float* gb, void* stream);

/* ---- rate and distortion maps (additive to version 4; inference only).  One value per block of 2^shift x 2^shift
 *      positions of every image: out (N, ceil(H / 2^shift), ceil(W / 2^shift)) dense; the blocks of the last row and
 *      column may be partial.  A tensor is the logical (N, C, H, W) with element strides; inside an image its storage
 *      is dense channels-last (sc 1, sw C, sh W C) or dense NCHW (sw 1, sh W, sc H W), the stride of an extent of 1 is
 *      not looked at, sn >= 0 is free.  IC_ERR_ARG before any launch for a null pointer, another layout, N outside
 *      1 .. 65535, an extent below 1, C H W >= 2^31 or a shift outside 0 .. 6.  One launch each; neither allocates or
 *      waits for its stream; no atomics.  The order of every sum is a function of (C, H, W, shift, layout) alone:
 *      image n's map has the same bits whatever N, n, the pointers' alignment (16-byte loads are used where an
 *      address allows them and change no bit) and the run. ---- */
/* out[n,bi,bj] = the sum over the block and all channels of clamp(-log2(p + 1e-10), 0, 50), the term of
 * ic_ce_loss_fwd; with `add` (the shape of out; NULL for none) out = add + that sum, one fp32 addition */
int ic_block_bits(const float* p, int N, int C, int Hm, int Wm, long long sn, long long sc, long long sh, long long sw,
                  int shift, const float* add, float* out, void* stream);
/* out[n,bi,bj] = the sum over the block and all channels of (a - b)^2: d = a - b rounded once, s = fma(d, d, s) (the
 * square fused with the accumulation, rounded once); a is walked along its storage, b at its own strides (an, ...) /
 * (bn, ...) */
int ic_block_sse(const float* a, const float* b, int N, int C, int H, int W, long long an, long long ac, long long ah,
                 long long aw, long long bn, long long bc, long long bh, long long bw, int shift, float* out,
                 void* stream);

/* ---- coding to a byte budget (additive to version 4; GainedMeanScaleCompressor2018.compress_each_to).  The sizes
 *      of candidate streams without their bytes, and the symbols of y for many (image, quality) candidates in one
 *      launch.  IC_ERR_ARG before any launch for anything the text below excludes; no floating-point atomics. ---- */
/* ic_codec_encode_seg without its output: lengths[segment * chunks per segment + chunk] = the byte count that call
 * writes there for the same arguments, from the same per-step arithmetic (state update, ballot of the emitting
 * lanes, popcount), with no store of a word or a state and so no workspace.  The same checks, the same LDS-or-pool
 * rule per segment.  Neither allocates device memory nor waits for its stream. */
int ic_codec_measure_seg(const int* sym, int nseg, long long seg_len, const unsigned char* rows, int C,
                         const unsigned int* pool, size_t pool_words, int nrows, const int* seg_k,
                         const long long* seg_off, int* seg_dev, int steps_per_chunk, unsigned int* lengths,
                         void* stream);
/* y: the latent of N images, dense (N, P, C) storage, channel fastest, read in place; candidate m of nseg
 * (1 .. 65535) names its image img[m] in [0, N) (host array, checked, then copied to img_dev: nseg ints on the
 * device), its gain row g[m] of g (nseg, C) and its mean mu[m] of mu (nseg, P, C):
 *     sym[m][p][c] = the symbol of (y[img[m]][p][c] * g[m][c]) - mu[m][p][c]
 * the product ic_channel_scale's one fp32 multiplication, the difference and the symbol those of
 * ic_codec_symbolize_mean_seg: bit for bit these two calls on the gathered batch y[img].  kmax_dev / kmax_host as
 * there: the maximum |symbol| of every candidate, one copy of the nseg maxima and one wait for the stream,
 * IC_ERR_ARG (with kmax_host filled) when any exceeds IC_CODEC_KMAX. */
int ic_gain_symbolize_seg(const float* y, long long N, long long P, int C, const float* g, const float* mu, int nseg,
                          const int* img, int* img_dev, int* sym, int* kmax_dev, int* kmax_host, void* stream);

/* ---- encode-time latent refinement (additive to version 4; Compressor2018.compress_each_refined).  The bookkeeping
 *      of the loop that moves the coded latent v by Adam steps on every image's own R + lambda D and keeps the best
 *      integers it saw.  IC_ERR_ARG before any launch for a null pointer, N outside 1 .. 65535, an extent below 1 or
 *      anything the text below excludes.  None of them allocates, copies to the host or waits for its stream; no
 *      floating-point atomics, every sum in one fixed order. ---- */
/* v, m, u, g, mu, sym, y_hat: dense (N, P, C) storage, channel fastest.  With g: the Adam step on v in place (moments
 * m, u in place; lr finite and positive, c1 = 1 / (1 - 0.9^t) and c2 = 1 / (1 - 0.999^t) as fp32, both >= 1), every
 * fp32 operation rounded once and none contracted (the order: csrc/refine.hip):
 *     m = 0.9f m + 0.1f g;  u = 0.999f u + 0.001f (g g);  v = v - (lr (m c1)) / (sqrtf(u c2) + 1e-8f)
 * g NULL: no step, v, m and u are not written (m and u may be NULL).  Then the Evaluate rule on v:
 *     sym = the symbol of v - mu (ic_codec_symbolize_mean_seg's);  y_hat = (float)sym + mu (ic_add_mean's)
 * mu NULL: neither the subtraction nor the addition is performed. */
int ic_refine_update(float* v, float* m, float* u, const float* g, const float* mu, long long N, long long P, int C,
                     float lr, float c1, float c2, int* sym, float* y_hat, void* stream);
/* gx = (float)(2 w[n]) * (x_hat - x) over the `len` elements of image n: the gradient of sum_n w[n] D_n at x_hat */
int ic_refine_dist_grad(const float* x, const float* x_hat, const double* w, int N, long long len, float* gx,
                        void* stream);
/* bits, sse: the maps of ic_block_bits / ic_block_sse, (N, nb) dense.  out (3, N) fp64: out[0][n] = B_n and
 * out[1][n] = D_n, each the sum of image n's nb values in ascending order in fp64, out[2][n] = J_n = B_n + w[n] D_n
 * (one fp64 product, one fp64 sum) */
int ic_refine_objective(const float* bits, const float* sse, const double* w, int N, long long nb, double* out,
                        void* stream);
/* obj, best: (3, N) fp64 as ic_refine_objective writes them.  mode 0: image n's `len` symbols of sym are copied to
 * best_sym where obj[2][n] < best[2][n] (strict; false for a NaN on either side); obj and best are only read.
 * mode 1 (a second launch, after mode 0): where the same comparison holds, best[.][n] = obj[.][n] and
 * best_step[n] = step (>= 0); sym and best_sym are not looked at. */
int ic_refine_keep(const int* sym, int* best_sym, const double* obj, double* best, int* best_step, int step, int N,
                   long long len, int mode, void* stream);
/* kmax[n] = the maximum |symbol| of image n's `len` symbols (INT_MAX for INT_MIN), on the device: one integer
 * atomicMax per block after a memset on the stream */
int ic_refine_kmax(const int* sym, int N, long long len, int* kmax, void* stream);

/* ---- decoding a window of a latent (additive to version 4; Compressor2018.decompress_window).  The chunks of a
 *      segment's bitstream are decodable alone and its symbols lie in (row, column, channel) order, so a band of rows
 *      is a range of chunks: only those are decoded, and only the symbols inside the window are stored. ---- */
/* One window: a rectangle of latent positions of one segment (an image's y). */
typedef struct ic_window {
  long long base;  /* index of the segment's first symbol in rows / mu */
  long long table; /* word offset of the segment's table in the pool */
  int hy, wy;      /* the segment is hy rows of wy positions of C channels: hy * wy * C symbols, below 2^31 */
  int K;           /* the segment's K */
  int r0, c0;      /* the window's first row and column; it ends at r0 + rh <= hy and c0 + rw <= wy */
  int k0, k1;      /* the chunks [k0, k1) of the segment, k1 <= its chunk count, that the call brings: they must
                      hold every symbol of rows [r0, r0 + rh) */
} ic_window;
/* bytes of the device workspace of ic_codec_decode_window (its descriptors); 0 for counts below 1 */
size_t ic_codec_window_ws(int nwin, long long nblocks);
/* Decodes nwin (1 .. 65535) windows of one latent shape rh x rw in one launch, block = one wavefront = one
 * (window, chunk) pair in (window, chunk) order: nblocks = the sum of k1 - k0.  in: 16-bit words, in_bytes of them
 * counted in bytes; spans (host): for every block the (begin, end) of its chunk in `in`, in words, 0 <= begin <= end
 * <= in_bytes / 2: the caller brings the payload of the spanned chunks alone and no block reads a length table.  A
 * chunk is decoded by the arithmetic of ic_codec_decode_seg with its guards (no read outside [begin, end), no search
 * outside the symbol's row), the table staged in LDS where nrows * (2K + 2) * 4 <= 48 KiB, the row of symbol g (its
 * index in rows: base + its index in the segment) rows[g], or g % C where rows is NULL (then base % C == 0 and
 * C <= nrows).  Every symbol of a chunk is decoded, the states being serial; the symbol q at (row, column, channel)
 * is stored where the window holds it:
 *     out[window][row - r0][column - c0][channel] = (float)q, or with mu: (float)q + mu[g], ic_add_mean's addition
 * out: (nwin, rh, rw, C) dense, every element written.  rows and mu, where given, hold nsym elements.  ws: 8-byte aligned device
 * memory of ic_codec_window_ws bytes (IC_ERR_WORKSPACE below that), written by one copy from host arrays that are
 * consumed before the call returns.  Every descriptor is checked before anything touches the device -- the window
 * inside its segment, the chunk range inside the segment's chunk count and over the window's rows, the spans inside
 * the buffer, K and the table inside the pool, the segment inside rows / mu -- IC_ERR_ARG otherwise: they come from
 * untrusted streams.  Neither allocates device memory nor waits for its stream. */
int ic_codec_decode_window(const void* in, size_t in_bytes, const ic_window* win, int nwin, int rh, int rw,
                           const long long* spans, long long nblocks, const unsigned char* rows, const float* mu,
                           long long nsym, int C, const unsigned int* pool, size_t pool_words, int nrows,
                           int steps_per_chunk, void* ws, size_t ws_bytes, float* out, void* stream);
/* ic_crop_clamp at an offset: y (N, C, h, w dense) = min(max(x, 0), 1) as ic_crop_clamp computes it, of
 * x[:, :, top : top + h, left : left + w] (any strides >= 0); one pass, bit for bit the two bounds then the slice */
int ic_crop_clamp_at(const ic_act* x, int top, int left, int h, int w, float* y, void* stream);

/* ---- transcoding in the latent domain (additive to version 4; Compressor2018.transcode_each,
 *      GainedMeanScaleCompressor2018.transcode_each_to).  The symbols of y at other qualities from the decoded integers
 *      of a stream, without y_hat or any scaled latent in memory.  IC_ERR_ARG before any launch for a null pointer, N
 *      or nseg outside 1 .. 65535, P or C below 1, an extent beyond 2^63 or an img entry outside [0, N); no
 *      floating-point atomics. ---- */
/* r, mu1: the decoded float integers of y of N source streams and their means, dense (N, P, C) storage, channel
 * fastest, read in place; a (N, C): the sources' inverse gains.  Target m of nseg names its source img[m] (host array,
 * checked, then copied to img_dev: nseg ints on the device), its gain row b[m] of b (nseg, C) and its mean mu2[m] of
 * mu2 (nseg, P, C):
 *     sym[m][p][c] = the symbol of (((r[img[m]][p][c] + mu1[img[m]][p][c]) * a[img[m]][c]) * b[m][c]) - mu2[m][p][c]
 * the sum ic_add_mean's one fp32 addition, each product ic_channel_scale's one fp32 multiplication, the difference and
 * the symbol those of ic_codec_symbolize_mean_seg, none contracted: bit for bit those four calls on the gathered
 * batch.  kmax_dev / kmax_host as in ic_gain_symbolize_seg: the maximum |symbol| of every target, one copy of the nseg
 * maxima and one wait for the stream, IC_ERR_ARG (with kmax_host filled) when any exceeds IC_CODEC_KMAX. */
int ic_requant_seg(const float* r, const float* mu1, long long N, long long P, int C, const float* a, const float* b,
                   const float* mu2, int nseg, const int* img, int* img_dev, int* sym, int* kmax_dev, int* kmax_host,
                   void* stream);

/* ---- choosing a quality map under a byte budget (additive to version 4;
 *      RegionGainedMeanScaleCompressor2018.compress_each_map_to).  The per-block level choice of many (image, weight)
 *      candidates in one launch, and the symbols of y for many (image, level map) candidates in one launch.
 *      IC_ERR_ARG before any launch for a null pointer or anything the text below excludes; neither allocates; no
 *      floating-point atomics. ---- */
/* bits, sse: the tables (N, L, nb) dense, fp32: level l of image n is nb per-block values (the maps of ic_block_bits /
 * ic_block_sse at that level), 1 <= N <= 65535, 2 <= L <= 16, nb >= 1.  Candidate m of M (1 .. 65535) names its image
 * img[m] in [0, N) and its weight w[m], finite and >= 0 (host arrays, checked, then copied to cand_dev: M ints and M
 * floats, 8 M bytes on the device).  For block b of candidate m, every operation one fp32 operation rounded once:
 *     J[l] = bits[img[m]][l][b] + w[m] * sse[img[m]][l][b];  best = 0, then l = 1 .. L-1 ascending replaces best iff
 *     J[l] < J[best] (strict: a tie keeps the lower level, a NaN never wins)
 *     ranks[m][b] = best;  codes[m][b] = level_codes[best]   (level_codes: L bytes on the host)
 *     sums[0][m] = the sum over b of bits[img[m]][best(b)][b], sums[1][m] the same of sse, in fp64; sums is (2, M)
 * The order of the sums is a function of nb alone: one HIP block of 256 threads per candidate, thread t adds the
 * values of blocks t, t + 256, ... in ascending order, then partial[t] += partial[t + s] for s = 128, 64, ..., 1; two
 * runs agree bit for bit.  Does not wait for its stream. */
int ic_block_allocate(const float* bits, const float* sse, int N, int L, long long nb, int M, const int* img,
                      const float* w, const unsigned char* level_codes, void* cand_dev, unsigned char* ranks,
                      unsigned char* codes, double* sums, void* stream);
/* ic_gain_symbolize_seg with a gain row per block: y the latent of N images, dense (N, Hm, Wm, C) storage, channel
 * fastest, read in place; g (R, C), 1 <= R <= 256; rank: uint8 (nseg, ceil(Hm / 2^shift), ceil(Wm / 2^shift)) on the
 * device, a rank >= R clamped to R - 1; candidate m of nseg (1 .. 65535) names its image img[m] in [0, N) (host array,
 * checked, then copied to img_dev: nseg ints on the device), its rank map rank[m] and its mean mu[m] of mu (nseg, Hm,
 * Wm, C):
 *     sym[m][i][j][c] = the symbol of (y[img[m]][i][j][c] * g[rank[m][i >> shift][j >> shift]][c]) - mu[m][i][j][c]
 * the product ic_block_scale's one fp32 multiplication, the difference and the symbol those of
 * ic_codec_symbolize_mean_seg: bit for bit these two calls on the gathered batch y[img].  Hm Wm C < 2^31, shift in
 * 0 .. 6.  kmax_dev / kmax_host as in ic_gain_symbolize_seg: the maximum |symbol| of every candidate, one copy of the
 * nseg maxima and one wait for the stream, IC_ERR_ARG (with kmax_host filled) when any exceeds IC_CODEC_KMAX. */
int ic_block_gain_symbolize_seg(const float* y, int N, int Hm, int Wm, int C, const float* g, int R,
                                const unsigned char* rank, int shift, const float* mu, int nseg, const int* img,
                                int* img_dev, int* sym, int* kmax_dev, int* kmax_host, void* stream);

/* ---- layered per-image streams (additive to version 4; Compressor2018.compress_each_layered /
 *      decompress_each_layered; the rule: image_compression_amd/codec.py, "Layered per-image containers").  y's C
 *      channels form G layers (1 <= G <= C, C % G == 0, Cg = C / G) in an order every image brings: order is a host
 *      array (N, C), row n a permutation of 0 .. C-1, and layer g of image n holds the channels
 *      order[n][g Cg .. (g + 1) Cg - 1].  All three work on dense (N, P, C) storage, channel fastest.  IC_ERR_ARG,
 *      before any copy or launch, for a null pointer, N, P, C or G below 1, G > C, C % G != 0, N P C beyond 2^60 (its
 *      byte offsets stay below 2^63), an order row that is not a permutation and what the text below excludes: the
 *      descriptors come from untrusted streams.  The host arrays are checked, copied into the caller's device ints and
 *      consumed before the call returns.  None allocates device memory or waits for its stream; no floating-point
 *      atomics.  Indices are 64-bit, 32-bit where every element count is below 2^31. ---- */
/* energy[n][c] = the sum over p of (long long)sym[n][p][c]^2: (N, C) on the device, set to 0 on the stream and then
 * added to by integer atomics, so exact in any order. */
int ic_layer_energy(const int* sym, int N, long long P, int C, unsigned long long* energy, void* stream);
/* src: elements of elem_bytes bytes, 4 (int32 symbols) or 1 (uint8 table rows).  seg: a host array of nseg (image,
 * layer) pairs, 1 <= nseg <= 65535, image in [0, N), layer in [0, G), any subset in any order; dst: nseg segments of
 * P Cg elements, the layout ic_codec_encode_seg / ic_codec_decode_seg take as sym and as rows:
 *     dst[s][p][j] = src[image_s][p][order[image_s][layer_s Cg + j]]
 * order_dev: N C ints on the device; seg_dev: 4 nseg + N + 1 ints on the device (the pairs, and every image's list
 * of its segments).  src and dst do not overlap. */
int ic_layer_gather(const void* src, int elem_bytes, int N, long long P, int C, int G, const int* order, int* order_dev,
                    const int* seg, int* seg_dev, int nseg, void* dst, void* stream);
/* q: the float output of ic_codec_decode_seg, its segments in (image, layer) ascending order, image n bringing its
 * layers 0 .. nlayers[n]-1; nlayers: a host array, 0 <= nlayers[n] <= G (q may be NULL when all are 0).  Every element
 * of y_hat (N, P, C) is written; with i the place of channel c = order[n][i] in the image's order:
 *     i <  nlayers[n] Cg:  y_hat[n][p][c] = q[base_n + (i / Cg) P Cg + p Cg + i % Cg] + mu[n][p][c]
 *                          (ic_add_mean's one fp32 addition, never contracted), or without mu the value of q itself
 *     i >= nlayers[n] Cg:  y_hat[n][p][c] = mu[n][p][c] bit for bit, or +0.0f without mu
 * base_n = P Cg (nlayers[0] + ... + nlayers[n-1]).  mu: NULL or (N, P, C).  order_dev: N C ints on the device;
 * nl_dev: 2 N ints on the device. */
int ic_layer_scatter(const float* q, const float* mu, int N, long long P, int C, int G, const int* order, int* order_dev,
                     const int* nlayers, int* nl_dev, float* y_hat, void* stream);

#ifdef __cplusplus
}
#endif
#endif
