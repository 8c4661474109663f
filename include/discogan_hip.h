/*
 * discogan_hip.h -- C ABI of the MI355X (gfx950) DiscoGAN training-step kernels.
 *
 * The reference (fasion-image-generator-project/discogan_modernized) has no FFI of its own: its
 * hot path is `torch.nn` calls made from model.py / image_translation.py.  Each entry point below
 * replaces the ATen/cuDNN op the cited reference line dispatches; a binding is a ctypes stub
 * (see INTEGRATION.md and discogan_modernized_amd/_lib.py).
 *
 * Conventions
 *   - every function returns 0 on success, a negative DG_ERR_* code otherwise; the message is
 *     available from dg_last_error() (thread-local).  Nothing aborts or throws across the ABI.
 *   - all pointers are DEVICE pointers to fp32 unless stated; the caller owns every buffer
 *     (parameters, activations, gradients, workspace).  The library never allocates or frees device
 *     memory and keeps no pointer past a call.
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (no synchronisation) and
 *     are capturable into a hipGraph.
 *   - ACTIVATION LAYOUT: interior feature maps are "NHWC" = [N][H][W][C] contiguous (the physical
 *     layout of a torch channels_last tensor of logical shape [N,C,H,W]).  The 3-channel image side
 *     (network input / output, model.py:8,80,142) stays NCHW exactly as the reference hands it over.
 *   - WEIGHT LAYOUT: a Conv2d weight of logical shape [K,C,4,4] (model.py:11...) is stored "KRSC" =
 *     [K][4][4][C]; a ConvTranspose2d weight of logical shape [Cin,Cout,4,4] (model.py:118...) is
 *     stored [Cin][4][4][Cout] (the same rule: dim1 moved innermost).  The 3-channel edge weights
 *     ([64,3,4,4]) stay in logical contiguous order.
 *   - spatial sizes must be powers of two; channel counts multiples of 4.
 */
#ifndef DISCOGAN_HIP_H
#define DISCOGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DG_OK 0
#define DG_ERR_INVALID (-1)     /* bad argument / unsupported shape */
#define DG_ERR_WORKSPACE (-2)   /* workspace too small            */
#define DG_ERR_HIP (-3)         /* HIP runtime error              */

#define DG_ACT_NONE 0
#define DG_ACT_LEAKY 1   /* LeakyReLU(slope)   model.py:9      */
#define DG_ACT_RELU 2    /* ReLU               model.py:116    */
#define DG_ACT_SIGMOID 3 /* Sigmoid            model.py:36,143 */

typedef void* dg_stream_t;

/* Arithmetic of the conv products, a PER-CALL argument of the *_g / *_p entry points ("dtype enum"):
 *   DG_PREC_F32   exact fp32 MFMA (v_mfma_f32_32x32x2_f32);
 *   DG_PREC_BF16  operands rounded to bf16 (RNE), bf16 MFMA, fp32 accumulation (BASELINE configs[4]);
 *   DG_PREC_F32X3 fp32-accurate products on the bf16 MFMA: every operand value as three bf16 pieces (24 significand bits), six MFMAs
 *                 per product block, fp32 accumulation.
 * Entry points WITHOUT the argument use the process default (dg_set_option("bf16", n); 0 unless set), kept for tools and tests. */
#define DG_PREC_DEFAULT (-1)  /* "whatever the process default is" (tools / tests that flip dg_set_option("bf16")) */
#define DG_PREC_F32 0
#define DG_PREC_BF16 1
#define DG_PREC_F32X3 2

/* Grouped launches (round 4).  The reference issues the passes of an iteration in independent pairs of identical shape --
 * G_B(A) | G_A(B), G_A(AB) | G_B(BA), D_A(A) | D_B(B), D_A(BA) | D_B(AB) (image_translation.py:342-361) -- and each discriminator
 * sees real and fake images with the SAME weights (:353-354,360-361).  A *_g entry point takes `groups` (1..DG_MAX_GROUPS) such
 * problems -- identical geometry, one pointer per problem in every pointer table -- and issues ONE launch per kernel of the op
 * (a block index selects the problem); each problem's result is bitwise what the one-problem call computes.  Where several problems
 * accumulate into the same tensor (`share`: a discriminator's real and fake pass into one weight / BatchNorm-parameter gradient) the
 * final reduction adds them in problem order, bitwise what consecutive accumulating calls leave. */
#define DG_MAX_GROUPS 4

/* 101: exported symbols were removed (dg_adam_advance_c, dg_adam_step_flat_c / _bf16 / _x3: dg_adam_advance and dg_adam_step_flat take
 * their arguments), and those two changed their argument lists. */
int dg_version(void);
/* 0 = the product library.  bit 0: experiments build (csrc/Makefile EXPERIMENTS=1: kernels that lost their A/B, behind options "x3_mfma",
 * "dgw_persist" and the window-forward / plane-reader planner codes); bit 1: timing build (TIMING=1: option "dbg_zero"). */
int dg_build_flags(void);
const char* dg_last_error(void);

/* ---- tuning knobs (process-global, for benchmarking and tests; 0 = heuristic) ----------------
 * "kt" 16|32: K-tile of the conv kernels;  "splitk" n: force n K-splits;  "target_wgs" n: workgroups a split
 * grid aims for (512);  "split_below" n: split K only when the tile grid has fewer workgroups (256);
 * "pointer_path" 1: use the 64-bit addressing kernels that tensors >= 2 GiB fall back to;
 * "no_xcd_group" 1: plain blockIdx -> tile order (default: workgroups sharing operand rows are placed on one XCD); 3: only the
 *   row-tile blocks per XCD of single-column forward convs off (same-box A/B);
 * "bf16" 1: the interior conv GEMMs (dg_conv_fwd/_dgrad/_wgrad and their named wrappers) round both operands to
 * bf16 and multiply on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; every tensor stays fp32 (BASELINE
 * configs[4]).  The result equals the fp32 op applied to the rounded operands up to summation order.  With "bf16" 1 the
 * 3-channel edge layers also round their operands and run on the bf16 MFMA ("kt" 16 keeps their fp32-MFMA kernels);
 * "bf16" 2: fp32-accurate products from three bf16 planes per operand (f32x3);
 * "no_dma" 1: convolutions with two bf16 operands stay on the register-staged tiles instead of the LDS-DMA kernel;
 * "bn_items" 1: the fp32 BatchNorm apply passes (forward and backward) on the per-item kernels instead of the row-geometry ones
 *   (same results bit for bit; same-box A/B and the test that says so); read once per call, where a dg_bn_act_* call enters the library;
 * "dma_mfma" 32: the LDS-DMA kernel's 32x32x16 body instead of the default 16x16x32 one; 1: keep the input-grads with <= 128
 *   output channels on the register-staged tiles instead of the window kernels (same-box A/B);
 * (experiments library only, csrc/Makefile EXPERIMENTS=1: "x3_mfma" 16 = the paired-plane 16x16x32 body of the f32x3 plane kernel,
 *   "dgw_persist" 1 = the persistent form of the f32x3 window input-grad kernel -- both measured not faster, DESIGN.md 3.1;
 *   "understory" = probe forms of dg_act_fwd for tools/probe_corun.py);
 * (The operand-dropping timing switch of earlier rounds exists only in the separate timing build, csrc/Makefile TIMING=1; the product
 *   library has no option that changes results.) */
int dg_set_option(const char* name, int value);

/* ---- interior convolutions: implicit GEMM on v_mfma_f32_32x32x2_f32 --------------------------
 * Geometry is that of the *Conv2d*: x[N,H,W,C] --(k4, stride, pad)--> y[N,Ho,Wo,K].
 * Supported: (stride 2, pad 1)  Ho=H/2      -- nn.Conv2d(C,K,4,2,1)      model.py:11-31,83-103
 *            (stride 1, pad 0)  H=W=4,Ho=1  -- nn.Conv2d(C,K,4,1,0)      model.py:35,107
 * ConvTranspose2d(Cin,Cout,4,s,p) (model.py:114-142) is the dgrad of that Conv2d with the same
 * weight tensor: forward = dg_conv_dgrad, input-grad = dg_conv_fwd, weight-grad = dg_conv_wgrad
 * with the roles (x := grad_out, dy := input).  The named wrappers below spell this out.
 */
size_t dg_conv_workspace_bytes(int op /*0 fwd,1 dgrad,2 wgrad*/, int N, int H, int W, int C, int K,
                               int stride, int pad);
int dg_conv_fwd(const float* x, const float* w, float* y, int N, int H, int W, int C, int K,
                int stride, int pad, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K,
                  int stride, int pad, void* ws, size_t ws_bytes, dg_stream_t stream);
/* dw (+)= sum_pixels dy (x) im2col(x); accumulate!=0 adds into dw */
int dg_conv_wgrad(const float* dy, const float* x, float* dw, int N, int H, int W, int C, int K,
                  int stride, int pad, int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream);

/* Grouped forms with the arithmetic as an argument.  stat (may be NULL): fused BatchNorm partial statistics, one buffer of
 * dg_conv_bnstats_rows_p(...) x (3 * columns + 4) floats per problem; ws: one workspace of ws_bytes >= dg_conv_workspace_bytes_p(...)
 * per problem (NULL entries allowed when that is 0).  dg_conv_wgrad_g: share > 1 = every `share` consecutive problems name the same dw.
 * plan_groups: 1 = every problem gets the split-K plan of a launch of its own (results bitwise those of the one-problem call);
 * `groups` = the plan is sized for the whole launch -- the group fills the chip, so each problem is cut into fewer K-slabs (less slab
 * traffic, shorter reduction): the same products in another, equally fixed, summation order. */
/* Shapes without a plan.  The launch entry points refuse: a forward with C % 32 != 0, a stride-2 input gradient with K % 32 != 0, K neither 1 nor
 * a multiple of 4, C % 4 != 0, an op outside 0..2 and every geometry dg_conv_fwd refuses (the plane forms dg_conv_*_x3 apply the same channel
 * rules).  For such a shape, and for the K == 1 head (plain reductions), EVERY planning query (dg_conv_workspace_bytes[_p],
 * dg_conv_plan_splits[_p], dg_conv_bnstats_rows[_p], dg_conv_bf16_operands_ok, dg_conv_x3_planes_ok, dg_conv_x3_bnstats_rows,
 * dg_conv_mixed_bnstats_rows) answers "nothing": 0 bytes, 0 rows, not ok (0), 1 split.  No query plans a shape that cannot be launched, and
 * none fails for any argument tuple; the refusal itself, with its message, comes from the launch entry point. */
size_t dg_conv_workspace_bytes_p(int op, int N, int H, int W, int C, int K, int stride, int pad, int prec, int plan_groups);
int dg_conv_bnstats_rows_p(int op, int N, int H, int W, int C, int K, int stride, int pad, int prec);
int dg_conv_plan_splits_p(int op, int N, int H, int W, int C, int K, int stride, int pad, int prec, int plan_groups);
/* The whole plan of one request, for tests that must know which code a shape runs (host only: no device call; nothing in the product path
 * asks).  a_form / b_form: 0 fp32 tensor, 1 bf16 tensor, 3 three bf16 planes.  The same planner and the same options as a launch (splitk, kt,
 * no_dma, dma_mfma, pointer_path, no_xcd_group, target_wgs, split_below).  Returns DG_PLAN_FIELDS and writes the first n_out fields, in this
 * order:  0 mode (0 forward, 1 stride-2 input gradient, 2 plain-GEMM input gradient of the 4x4 layers, 3 weight gradient)   1 the arithmetic
 * actually used (DG_PREC_*: exact fp32 where the asked-for one has no kernel for the shape)   2 wm  3 wn (waves per tile)   4 kt (K-tile)
 * 5 kernel family (0 register-staged tiles, 1 bf16 LDS-DMA, 2 f32x3 plane, 3 f32x3 window input gradient, 4 bf16 window input gradient)
 * 6 ncls (parity classes per workgroup of the window kernels, else 0)   7 M  8 Ng (GEMM rows, columns)   9 BM  10 BN (tile)   11 tilesM
 * 12 tilesN   13 zmul (4 parity classes of the stride-2 input gradient, else 1)   14 nIt (K-tiles)   15 splits   16 itPerSplit
 * 17 xcd_group (blockIdx-to-tile order 0..3; the two window kernels ignore it)   18 stat_rows (partial rows of the fused BatchNorm
 * statistics, 0: none)   19 addressing (0 buffer descriptors, 1 64-bit pointers).  A request without a plan (see above) returns 0 and
 * writes nothing. */
#define DG_PLAN_FIELDS 20
int dg_conv_plan_describe(int op, int N, int H, int W, int C, int K, int stride, int pad, int prec, int plan_groups, int a_form, int b_form,
                          int* out, int n_out);
int dg_conv_fwd_g(int groups, const float* const* x, const float* const* w, float* const* y, int N, int H, int W, int C, int K, int stride,
                  int pad, int prec, int plan_groups, float* const* stat, size_t stat_floats, void* const* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_dgrad_g(int groups, const float* const* dy, const float* const* w, float* const* dx, int N, int H, int W, int C, int K, int stride,
                    int pad, int prec, int plan_groups, float* const* stat, size_t stat_floats, void* const* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_wgrad_g(int groups, int share, const float* const* dy, const float* const* x, float* const* dw, int N, int H, int W, int C, int K,
                    int stride, int pad, int prec, int plan_groups, int accumulate, void* const* ws, size_t ws_bytes, dg_stream_t stream);

/* Inference path (inference.py:149,172-187: generator.eval() forward): [Conv2d | ConvTranspose2d] -> BatchNorm2d(eval)
 * -> LeakyReLU/ReLU as ONE kernel.  The caller folds the BatchNorm scale into the weights (w * gamma*invstd per output
 * channel) and passes the shift as bias[out channels] = beta - running_mean*gamma*invstd; y = act(conv(x, w) + bias).
 * Same geometry / layouts as dg_conv_fwd / dg_conv_dgrad (dgrad = ConvTranspose2d forward); bias may be NULL. */
int dg_conv_fwd_bias_act(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int K,
                         int stride, int pad, int act, float slope, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_dgrad_bias_act(const float* dy, const float* w, const float* bias, float* dx, int N, int H, int W, int C, int K,
                           int stride, int pad, int act, float slope, void* ws, size_t ws_bytes, dg_stream_t stream);

/* Stride-2 conv forward / dgrad (= ConvTranspose2d forward) that ALSO emit BatchNorm partial statistics
 * of the output from the kernel epilogue (or from the split-K reduction), saving the separate read
 * pass of dg_bn_train_stats.  stat: [rows][3*cols + 4] floats with rows = dg_conv_bnstats_rows(op,...)
 * and cols = K (op 0, fwd) or C (op 1, dgrad); consume with dg_bn_stats_from_partials. */
int dg_conv_bnstats_rows(int op, int N, int H, int W, int C, int K, int stride, int pad);
/* number of K splits the plan for this shape uses (1 = no split-K reduction kernel, also for a shape without a plan: see above) */
int dg_conv_plan_splits(int op, int N, int H, int W, int C, int K, int stride, int pad);
int dg_conv_fwd_bnstats(const float* x, const float* w, float* y, int N, int H, int W, int C, int K,
                        float* stat, size_t stat_floats, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_dgrad_bnstats(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K,
                          float* stat, size_t stat_floats, void* ws, size_t ws_bytes, dg_stream_t stream);

/* named wrappers; H,W always name the LARGER spatial side of the layer */
int dg_conv4x4s2_fwd(const float* x, const float* w, float* y, int N, int H, int W, int C, int K,
                     void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4s2_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K,
                       void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4s2_wgrad(const float* dy, const float* x, float* dw, int N, int H, int W, int C, int K,
                       int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4_valid_fwd(const float* x, const float* w, float* y, int N, int C, int K,
                         void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4_valid_dgrad(const float* dy, const float* w, float* dx, int N, int C, int K,
                           void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4_valid_wgrad(const float* dy, const float* x, float* dw, int N, int C, int K,
                           int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);
/* ConvTranspose2d(Cin,Cout,4,2,1): x[N,Hin,Win,Cin] -> y[N,2Hin,2Win,Cout]; w [Cin][4][4][Cout] */
int dg_convT4x4s2_fwd(const float* x, const float* w, float* y, int N, int Hin, int Win, int Cin, int Cout,
                      void* ws, size_t ws_bytes, dg_stream_t s);
int dg_convT4x4s2_dgrad(const float* dy, const float* w, float* dx, int N, int Hin, int Win, int Cin, int Cout,
                        void* ws, size_t ws_bytes, dg_stream_t s);
int dg_convT4x4s2_wgrad(const float* dy, const float* x, float* dw, int N, int Hin, int Win, int Cin, int Cout,
                        int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);
/* ConvTranspose2d(Cin,Cout,4,1,0) on a 1x1 input: x[N,Cin] -> y[N,4,4,Cout] */
int dg_convT4x4_1to4_fwd(const float* x, const float* w, float* y, int N, int Cin, int Cout,
                         void* ws, size_t ws_bytes, dg_stream_t s);
int dg_convT4x4_1to4_dgrad(const float* dy, const float* w, float* dx, int N, int Cin, int Cout,
                           void* ws, size_t ws_bytes, dg_stream_t s);
int dg_convT4x4_1to4_wgrad(const float* dy, const float* x, float* dw, int N, int Cin, int Cout,
                           int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);

/* ---- 3-channel edge layers (image side stays NCHW) ------------------------------------------
 * w is the logical contiguous [K][3][4][4] tensor in all three (Conv2d(3,K) weight, model.py:8,80;
 * ConvTranspose2d(K,3) weight, model.py:142).
 * c3_fwd  : y_nhwc[N,H/2,W/2,K] = act(conv_s2(x_nchw[N,3,H,W], w))        conv1 forward (act=LEAKY)
 *                                                                        / last-convT input-grad
 * c3_dgrad: dx_nchw[N,3,H,W] = act(conv_s2_dgrad(dy_nhwc[N,H/2,W/2,K], w)) last-convT forward
 *                                                                        (act=SIGMOID) / conv1 dgrad
 * c3_wgrad: dw[K][3][4][4] (+)= sum dy_nhwc (x) im2col(x_nchw)
 */
int dg_conv4x4s2_c3_fwd(const float* x_nchw, const float* w, float* y_nhwc, int N, int H, int W, int K,
                        int act, float slope, dg_stream_t s);
size_t dg_c3_dgrad_workspace_bytes(int K);
int dg_conv4x4s2_c3_dgrad(const float* dy_nhwc, const float* w, float* dx_nchw, int N, int H, int W, int K,
                          int act, void* ws, size_t ws_bytes, dg_stream_t s);
size_t dg_c3_wgrad_workspace_bytes(int N, int H, int W, int K);
int dg_conv4x4s2_c3_wgrad(const float* dy_nhwc, const float* x_nchw, float* dw, int N, int H, int W, int K,
                          int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);
/* Same, with the backward of the layer's fused LeakyReLU/ReLU applied to dy on the fly:
 * dy_eff = dy * act'(act_out), act_out = the saved forward output (model.py:8-9, 80-81: Conv2d + in-place
 * LeakyReLU).  Saves the separate dg_act_bwd pass when only the weight gradient is needed. */
int dg_conv4x4s2_c3_wgrad_act(const float* dy_nhwc, const float* act_out_nhwc, int act, float slope,
                              const float* x_nchw, float* dw, int N, int H, int W, int K, int accumulate,
                              void* ws, size_t ws_bytes, dg_stream_t s);

/* Grouped forms of the three edge ops (K == 64: the streaming / scatter / per-wave kernels), arithmetic as an argument.
 * dg_conv4x4s2_c3_wgrad_g: act_out_nhwc NULL with act NONE; share > 1 = every `share` consecutive problems name the same dw;
 * ws: one workspace of ws_bytes >= dg_c3_wgrad_workspace_bytes(...) per problem. */
/* one-problem forms with the arithmetic as an argument (y_bf16 / dy_bf16 / io_bf16: the 64-channel NHWC side is bf16, see the *_t forms) */
int dg_conv4x4s2_c3_fwd_p(const float* x_nchw, const float* w, void* y_nhwc, int y_bf16, int N, int H, int W, int K,
                          int act, float slope, int prec, dg_stream_t s);
int dg_conv4x4s2_c3_dgrad_p(const void* dy_nhwc, int dy_bf16, const float* w, float* dx_nchw, int N, int H, int W, int K,
                            int act, int prec, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4s2_c3_wgrad_p(const void* dy_nhwc, const void* act_out_nhwc, int io_bf16, int act, float slope,
                            const float* x_nchw, float* dw, int N, int H, int W, int K, int prec, int accumulate,
                            void* ws, size_t ws_bytes, dg_stream_t s);
/* The input-gradient of nn.Conv2d(3,K,4,2,1) (model.py:8,80) with the backward of the layer's in-place LeakyReLU (model.py:9,81) applied to
 * dy on the way in -- dx = dgrad(dy * (act_out > 0 ? 1 : slope)), act_out = the layer's saved output (same layout and type as dy),
 * in_act = DG_ACT_LEAKY -- instead of a stand-alone dg_act_bwd pass in front of dg_conv4x4s2_c3_dgrad_p; bitwise the unfused result.
 * Exists where dg_c3_dgrad_act_ok(N, H, W, K, dy_bf16) returns 1: K == 64 on the scatter kernel, which takes dy up to 2^31 bytes
 * (N * H/2 * W/2 * 64 elements of dy's type); other arguments as dg_conv4x4s2_c3_dgrad_p. */
int dg_c3_dgrad_act_ok(int N, int H, int W, int K, int dy_bf16);
int dg_conv4x4s2_c3_dgrad_act_p(const void* dy_nhwc, int dy_bf16, const void* act_out_nhwc, int in_act, float slope, const float* w,
                                float* dx_nchw, int N, int H, int W, int K, int act, int prec, void* ws, size_t ws_bytes, dg_stream_t s);
/* The last decoder group [BatchNorm2d(K)][ReLU][ConvTranspose2d(K,3,4,2,1)][Sigmoid] (model.py:140-143) without the BatchNorm apply pass: the
 * two kernels that read the BatchNorm's output z take its INPUT y_nhwc[N,H/2,W/2,K] (fp32) instead and evaluate
 * z = relu((y - mean) * (gamma * invstd) + beta), saved = [mean | invstd] (dg_bn_train_stats / dg_bn_stats_from_partials), on the values they
 * load -- the expression of dg_bn_act_fwd, so both are bitwise dg_conv4x4s2_c3_dgrad_p / dg_conv4x4s2_c3_wgrad_p on dg_bn_act_fwd's output.
 * bn_act = DG_ACT_RELU.  They exist where dg_c3_dgrad_bn_ok / dg_c3_wgrad_bn_ok (host only) return 1: K == 64, y under 2^31 bytes (weight
 * gradient: both tensors under 1 GiB and W >= 32), prec exact fp32 or f32x3; elsewhere the caller keeps the apply pass. */
int dg_c3_dgrad_bn_ok(int N, int H, int W, int K, int prec);
int dg_conv4x4s2_c3_dgrad_bn_p(const float* y_nhwc, const float* saved, const float* gamma, const float* beta, int bn_act, const float* w,
                               float* dx_nchw, int N, int H, int W, int K, int act, int prec, dg_stream_t s);
int dg_c3_wgrad_bn_ok(int N, int H, int W, int K, int prec);
int dg_conv4x4s2_c3_wgrad_bn_p(const float* y_nhwc, const float* saved, const float* gamma, const float* beta, int bn_act, const float* x_nchw,
                               float* dw, int N, int H, int W, int K, int prec, int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4s2_c3_fwd_g(int groups, const float* const* x_nchw, const float* const* w, float* const* y_nhwc, int N, int H, int W, int K,
                          int act, float slope, int prec, dg_stream_t s);
int dg_conv4x4s2_c3_dgrad_g(int groups, const float* const* dy_nhwc, const float* const* w, float* const* dx_nchw, int N, int H, int W, int K,
                            int act, int prec, dg_stream_t s);
int dg_conv4x4s2_c3_wgrad_g(int groups, int share, const float* const* dy_nhwc, const float* const* act_out_nhwc, int act, float slope,
                            const float* const* x_nchw, float* const* dw, int N, int H, int W, int K, int prec, int accumulate,
                            void* const* ws, size_t ws_bytes, dg_stream_t s);

/* ---- BatchNorm2d (training mode) + activation, NHWC [M][C], M = N*H*W ------------------------
 * nn.BatchNorm2d (model.py:12...; eps 1e-5, momentum 0.1, biased batch var for normalisation,
 * unbiased for running_var, num_batches_tracked int64 += 1) fused with the in-place
 * LeakyReLU(0.2)/ReLU that follows it (model.py:13,116).
 * saved: [2][C] = mean, invstd (kept for backward).
 */
size_t dg_bn_workspace_bytes(int M, int C);
int dg_bn_train_stats(const float* y, int M, int C, float eps, float momentum,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      float* saved, void* ws, size_t ws_bytes, dg_stream_t s);
/* same outputs as dg_bn_train_stats, from partial rows written by dg_conv_*_bnstats (M = N*H*W rows total).
 * ws: dg_bn_partials_workspace_bytes(P, C) bytes (0 for P < 4096 rows) -- with it many rows are merged in two short launches
 * (row blocks, then channels) instead of one latency-bound one; NULL / too small: the one-launch form. */
size_t dg_bn_partials_workspace_bytes(int P, int C);
int dg_bn_stats_from_partials(const float* stat, int P, int M, int C, float eps, float momentum,
                              float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              float* saved, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_bn_act_fwd(const float* y, float* z, int M, int C, const float* saved, const float* gamma,
                  const float* beta, int act, float slope, dg_stream_t s);
/* dy = BN'(act'(dz)); dgamma/dbeta (+)= ; dy may alias dz */
int dg_bn_act_bwd(const float* dz, const float* y, float* dy, int M, int C, const float* saved,
                  const float* gamma, const float* beta, int act, float slope,
                  float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, dg_stream_t s);

/* Grouped forms (fp32 tensors).  share > 1: every `share` consecutive problems are passes through the SAME BatchNorm module (a
 * discriminator's real and fake pass, image_translation.py:353-361): they name the same running_mean / running_var /
 * num_batches_tracked (dg_bn_train_stats_g) or the same dgamma / dbeta (dg_bn_act_bwd_g), and the finalize kernel applies their
 * updates one after the other in problem order.  ws: one workspace of ws_bytes >= dg_bn_workspace_bytes(M, C) per problem; the
 * backward keeps its coefficients there between its three kernels. */
int dg_bn_train_stats_g(int groups, int share, const float* const* y, int M, int C, float eps, float momentum, float* const* running_mean,
                        float* const* running_var, int64_t* const* num_batches_tracked, float* const* saved, void* const* ws, size_t ws_bytes,
                        dg_stream_t s);
int dg_bn_act_fwd_g(int groups, const float* const* y, float* const* z, int M, int C, const float* const* saved, const float* const* gamma,
                    const float* const* beta, int act, float slope, dg_stream_t s);
int dg_bn_act_bwd_g(int groups, int share, const float* const* dz, const float* const* y, float* const* dy, int M, int C,
                    const float* const* saved, const float* const* gamma, const float* const* beta, int act, float slope,
                    float* const* dgamma, float* const* dbeta, int accumulate, void* const* ws, size_t ws_bytes, dg_stream_t s);

/* ---- stand-alone activations ------------------------------------------------------------------ */
int dg_act_fwd(const float* x, float* y, size_t n, int act, float slope, dg_stream_t s);
/* out = output of the activation (in-place semantics of the reference, model.py:9,36) */
int dg_act_bwd(const float* dy, const float* out, float* dx, size_t n, int act, float slope, dg_stream_t s);
int dg_act_fwd_g(int groups, const float* const* x, float* const* y, size_t n, int act, float slope, dg_stream_t s);
int dg_act_bwd_g(int groups, const float* const* dy, const float* const* out, float* const* dx, size_t n, int act, float slope, dg_stream_t s);

/* ---- losses: scalars stay in device memory ----------------------------------------------------
 * gout points to the upstream gradient scalar (device).  ws: >= dg_loss_workspace_bytes().
 */
size_t dg_loss_workspace_bytes(void);
/* nn.MSELoss()  image_translation.py:267,349 */
int dg_mse_fwd(const float* x, const float* t, size_t n, float* loss, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_mse_bwd(const float* x, const float* t, size_t n, const float* gout, float* dx, dg_stream_t s);
/* nn.BCELoss() against a constant label (image_translation.py:157-166), log clamped at -100 */
int dg_bce_fwd(const float* p, int n, float label, float* loss, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_bce_bwd(const float* p, int n, float label, const float* gout, float* dp, dg_stream_t s);
/* one layer of get_fm_loss (image_translation.py:136-144): mean_j (mean_n real - mean_n fake)^2,
 * real/fake [N][J]; diff[J] kept for backward; ws >= dg_fm_workspace_bytes(N, J) */
size_t dg_fm_workspace_bytes(int N, size_t J);
int dg_fm_fwd(const float* real, const float* fake, int N, size_t J, float* diff, float* loss,
              void* ws, size_t ws_bytes, dg_stream_t s);
int dg_fm_bwd(const float* diff, int N, size_t J, const float* gout, float* dreal, float* dfake, dg_stream_t s);
/* Grouped forms: the A-side and B-side term of each loss in one launch per kernel (image_translation.py:349-350,353-365).  label: one
 * host float per problem.  dg_fm_bwd_g: dreal / dfake tables may be NULL (that side takes no gradient). */
int dg_mse_fwd_g(int groups, const float* const* x, const float* const* t, size_t n, float* const* loss, void* const* ws, size_t ws_bytes, dg_stream_t s);
int dg_mse_bwd_g(int groups, const float* const* x, const float* const* t, size_t n, const float* const* gout, float* const* dx, dg_stream_t s);
int dg_bce_fwd_g(int groups, const float* const* p, int n, const float* label, float* const* loss, dg_stream_t s);
int dg_bce_bwd_g(int groups, const float* const* p, int n, const float* label, const float* const* gout, float* const* dp, dg_stream_t s);
int dg_fm_fwd_g(int groups, const float* const* real, const float* const* fake, int N, size_t J, float* const* diff, float* const* loss,
                void* const* ws, size_t ws_bytes, dg_stream_t s);
int dg_fm_bwd_g(int groups, const float* const* diff, int N, size_t J, const float* const* gout, float* const* dreal, float* const* dfake,
                dg_stream_t s);

/* Profiling hook: the next implicit-GEMM launches write 8 int64 per workgroup into buf ({wall0, cyc0, cyc after
 * prologue, cyc after the K loop, cyc after the epilogue stores are issued, wall1, XCC<<32|HW_ID, cyc end});
 * (NULL, 0) switches it off.  wall = 100 MHz constant clock, cyc = shader clock. */
int dg_debug_igemm_stamps(void* buf, size_t bytes);

/* number of compute units of the current device (host planning aid) */
int dg_device_cu_count(void);

/* Curriculum loss mix (image_translation.py:162-166,367-382) over a vector of loss scalars, and the
 * gradient seeds of every term, each in ONE launch.  lossvec: [0,1] recon A,B; [2..4] BCE(D_A real,1),
 * BCE(D_A fake,0), BCE(D_A fake,1); [5..7] same for D_B; [8..8+nfm) FM layers of D_A; [8+nfm..8+2nfm) of D_B.
 * out8: gen_loss_A, gen_loss_B, fm_loss_A, fm_loss_B, dis_loss_A, dis_loss_B, gen_loss, dis_loss.
 * arch 0 discogan, 1 recongan, 2 gan.  which: 6 = backward of gen_loss, 7 = backward of dis_loss. */
int dg_loss_mix_fwd(const float* lossvec, float* out8, int nfm, float rate, int arch, dg_stream_t s);
int dg_loss_mix_bwd(const float* gout, float* gvec, int nfm, float rate, int arch, int which, dg_stream_t s);

/* ---- Adam over flat buffers (optim.Adam, image_translation.py:275-287) ------------------------
 * state (device, 4 x float64): [0] step count, [1] lr/(1-b1^t), [2] sqrt(1-b2^t), [3] spare.
 * dg_adam_advance increments the step and refreshes the scalars ON DEVICE (graph-capturable).  ctl: NULL, or the control block of
 *   the gradient statistics below: state is left untouched when ctl[3] != 0.
 * dg_adam_step_flat: the one step of a flat range.  form 0: p, m, v only (28 B/param), out unused; 1: out = the bf16 shadow of p
 *   (+2 B/param); 3: out = plane 0 of the range's three bf16 planes, plane_elems elements apart (>= n, % 8 == 0; +6 B/param).
 *   ctl == NULL: the host's grad_scale.  Otherwise grad_scale is ignored and the scale is (float)ctl[2]; when ctl[3] != 0 every thread
 *   returns before its first load: p, m, v, the shadow and the planes keep their bits.  A step that is taken is bitwise the
 *   host-scaled call with grad_scale = (float)ctl[2].  n == 0 launches nothing. */
int dg_adam_advance(double* state, double lr, double beta1, double beta2, const double* ctl, dg_stream_t s);
int dg_adam_step_flat(float* p, const float* g, float* m, float* v, size_t n, const double* state,
                      float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                      const double* ctl, void* out, int form, size_t plane_elems, dg_stream_t s);
/* Exponential moving average of a flat parameter buffer: ema += (p - ema) * w, w = 1 - decay in [0, 1], the three operations
 * rounded one by one (p == ema leaves ema bitwise unchanged for every w).  dg_swap_flat exchanges the contents of two buffers
 * bit for bit; a == b is a no-op, ranges that overlap otherwise are refused.  Pointers 16-byte aligned; n == 0 launches nothing. */
int dg_ema_update_flat(float* ema, const float* p, size_t n, float w, dg_stream_t s);
int dg_swap_flat(float* a, float* b, size_t n, dg_stream_t s);

/* ---- Gradient norm, clipping by it and the non-finite guard of an Adam step (optim.Adam.enable_grad_control) --------------------
 * Everything stays on the device and on one stream: partials of every stepped flat range, one finalize, then the Adam entry points above
 * with ctl, which take their gradient scale and their go / no-go from the control block the finalize wrote.
 *
 * dg_grad_sumsq_partial: sum of squares of g[0..n), every element widened to double BEFORE it is squared (an exact product, so a finite
 *   fp32 gradient can neither overflow nor underflow the sum: only inf / NaN elements make it non-finite).  Grid of at most 4096 blocks
 *   x 256 threads, 4 elements (16 bytes) per thread and trip, a tail of n % 4 elements by one thread; block b writes ONE fp64 partial
 *   to ws[slot0 + b].  No atomics, fixed summation order: the same input gives the same bits on every run.  *slots_used = blocks
 *   launched (n == 0: none, nothing is launched).  g 16-byte aligned; (slot0 + blocks) * 8 <= ws_bytes.  Ranges of one step use
 *   consecutive slots: slot0 of the next call = slot0 + *slots_used.  dg_grad_stats_workspace_bytes() holds four full-grid ranges.
 * dg_grad_clip_finalize: one workgroup sums ws[0..slots) in a fixed order and writes ctl (device, 8 x float64):
 *   [0] sumsq   [1] norm = sqrt(sumsq) * pre_scale   [2] scale = pre_scale * min(1, max_norm / (norm + 1e-6))   [3] skip (0 / 1)
 *   [4] steps seen   [5] steps clipped   [6] steps skipped   [7] largest finite norm seen        ([4..7] accumulate: zero them once)
 *   pre_scale is the factor the step would have passed as grad_scale (data parallel: 1 / world size behind a SUM all-reduce, so norm
 *   is the norm of the averaged gradient).  max_norm <= 0: no clipping, scale = pre_scale.  The coefficient is
 *   torch.nn.utils.clip_grad_norm_'s; with error_if_nonfinite=False semantics when guard == 0: an infinite norm gives scale 0, a NaN
 *   norm a NaN scale, and the step is taken.  guard != 0: skip = !isfinite(sumsq). */
size_t dg_grad_stats_workspace_bytes(void);
int dg_grad_sumsq_partial(const float* g, size_t n, double* ws, size_t ws_bytes, int slot0, int* slots_used, dg_stream_t s);
int dg_grad_clip_finalize(const double* ws, int slots, double pre_scale, double max_norm, int guard, double* ctl, dg_stream_t s);

/* nn.BCELoss against a target TENSOR (image_translation.py:157-166 materialises ones / zeros label tensors);
 * same -100 log clamp and 1e-12 backward guard as dg_bce_fwd/_bwd.  p, target: [n]. */
int dg_bce_target_fwd(const float* p, const float* target, int n, float* loss, dg_stream_t s);
int dg_bce_target_bwd(const float* p, const float* target, int n, const float* gout, float* dp, dg_stream_t s);
/* nn.HingeEmbeddingLoss(margin, mean) for targets in {+1, -1} (image_translation.py:141-142,269; with the
 * reference's all-ones targets it is x.mean()).  ws >= dg_loss_workspace_bytes(). */
int dg_hinge_fwd(const float* x, const float* y, size_t n, float margin, float* loss, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_hinge_bwd(const float* x, const float* y, size_t n, float margin, const float* gout, float* dx, dg_stream_t s);
/* ---- adversarial objectives on LOGITS (trainer.py --gan_loss; csrc/ganloss.hip).  logit: float [n], the discriminator's head conv
 * output in front of its sigmoid.  Per problem  loss = mean_i f(x_i)  and  dlogit_i = gout f'(x_i) / n  (gout a device scalar), with the
 * target tau by role -- D_REAL: real_label (one-sided label smoothing, in (0.5, 1]), D_FAKE: 0, G_FAKE: 1 -- and by kind
 *     BCE_LOGITS  f = tau sp(-x) + (1 - tau) sp(x)    f' = sigmoid(x) - tau     sp(x) = max(x, 0) + log1p(exp(-|x|))
 *     LSGAN       f = (x - tau)^2                     f' = 2 (x - tau)          (no 1/2, as CycleGAN has it)
 *     HINGE       D_REAL max(0, 1 - x), D_FAKE max(0, 1 + x), G_FAKE -x         f' = -[x < 1], +[x > -1], -1; 0 at the kink x = +-1
 * sp and sigmoid are formed from exp(-|x|) (tau = 1: f' = -sigmoid(-x); tau = 0: sigmoid(x)), so a saturated logit keeps a relatively
 * accurate, non-zero gradient; nothing is clamped.  HINGE takes real_label 1 only.  A NaN logit gives a NaN loss and a NaN in that
 * element of dlogit, in every kind and role.  fwd: one workgroup per problem, fp64 partial sums in a fixed order, no atomics, no
 * workspace: bitwise repeatable.  The *_g forms run `groups` (1..DG_MAX_GROUPS) problems of one (n, kind, real_label), each with its own
 * role, in ONE launch, bitwise the single calls.  Refused with DG_ERR_INVALID and nothing launched: groups out of range, a null table or
 * pointer, n < 1, an unknown kind or role, a real_label that is not finite or not in (0.5, 1], HINGE with real_label != 1. */
#define DG_GAN_BCE_LOGITS 0
#define DG_GAN_LSGAN 1
#define DG_GAN_HINGE 2
#define DG_GAN_D_REAL 0
#define DG_GAN_D_FAKE 1
#define DG_GAN_G_FAKE 2
int dg_gan_loss_fwd(const float* logit, int n, int kind, int role, float real_label, float* loss, dg_stream_t s);
int dg_gan_loss_bwd(const float* logit, int n, int kind, int role, float real_label, const float* gout, float* dlogit, dg_stream_t s);
int dg_gan_loss_fwd_g(int groups, const float* const* logit, int n, int kind, const int* role /* host [groups] */, float real_label,
                      float* const* loss, dg_stream_t s);
int dg_gan_loss_bwd_g(int groups, const float* const* logit, int n, int kind, const int* role /* host [groups] */, float real_label,
                      const float* const* gout, float* const* dlogit, dg_stream_t s);

/* ---- data-parallel exchange group over RCCL / xGMI ---------------------------------------------
 * Replaces dist.init_process_group("nccl") (distributed_image_translation.py:31-38), DistributedDataParallel's
 * gradient all-reduce (:401-404,513-518), dist.barrier() (:398,573-574), destroy_process_group (:42-46).
 * One communicator per process (one process per GPU; the current HIP device at dg_dp_init is the rank's GPU).
 * Bootstrap: rank 0 calls dg_dp_get_unique_id into a HOST buffer of dg_dp_unique_id_bytes() bytes, ships it to the
 * other ranks out of band (the host layer uses the c10d TCP store), every rank calls dg_dp_init with it.
 * Collectives are in place, fp32, enqueued on the CALLER's stream (no internal stream, no synchronisation);
 * all-reduce is a SUM -- DDP's division by the world size is folded into dg_adam_step_flat's grad_scale.
 * The communicator handle is the only state the library keeps between calls.  RCCL is dlopen'ed on first use.
 * dg_dp_init is COLLECTIVE (ncclCommInitRank blocks until every rank has entered it): the host layer therefore first
 * calls dg_dp_ready on every rank -- purely local: binds RCCL, checks that a HIP device is current and that no
 * communicator exists -- and lets the ranks VOTE on the outcome out of band (dp.guarded_bootstrap: c10d store keys, no
 * collective) before any rank enters dg_dp_init, which it runs under a deadline (DG_COMM_INIT_TIMEOUT_S). */
int dg_dp_ready(int* device_out /* the current HIP device ordinal; may be NULL */);
int dg_dp_unique_id_bytes(void);
int dg_dp_get_unique_id(void* id_out_host, size_t bytes);
int dg_dp_init(int rank, int world, const void* unique_id_host, size_t bytes);
int dg_dp_world_size(void);   /* ranks in the communicator; 0 before dg_dp_init */
int dg_dp_rank(void);         /* -1 before dg_dp_init */
int dg_dp_allreduce_sum(float* buf, size_t n, dg_stream_t stream);
int dg_dp_allreduce_max(float* buf, size_t n, dg_stream_t stream);   /* in place, fp32 MAX (max-over-ranks timings) */
int dg_dp_broadcast(float* buf, size_t n, int root, dg_stream_t stream);
int dg_dp_barrier(float* scratch1 /* one device float owned by the caller */, dg_stream_t stream);
int dg_dp_destroy(void);

/* ---- image ingest (dataset.py:62-66): uint8 [N][H][W][3] -> float [N][3][H][W] = pixel / 255 -------------
 * bgr != 0 swaps the channel order (cv2.imread-style BGR sources).  H*W must be a multiple of 4. */
int dg_u8hwc_to_f32chw(const uint8_t* src, float* dst, int N, int H, int W, int bgr, dg_stream_t s);
/* ---- image preparation (dataset.py:52-66 read_images, :239-254 DiscoGANDataset._load_and_process_image) ----------------
 * uint8 [N][H][W][3] decoded rows -> float [N][3][S][S]: crop columns [x0, x0 + cw) (edges2*: the left / right half,
 * dataset.py:54,59), optional 3x3 erosion = 255 - cv2.dilate(255 - x, ones(3,3)) (domain 'A', dataset.py:53-57; neighbours
 * outside the crop do not count, like cv2's default border), cv2.resize(..., (S, S)) = INTER_LINEAR with half-pixel centres
 * and edge clamp (dataset.py:62), / 255 and CHW (dataset.py:65-66).  mode 0: float arithmetic, unrounded (what the
 * reference's float64 domain-'A' image gets); mode 1: cv2's 8-bit fixed-point path, result rounded to uint8 before / 255. */
int dg_image_prep(const uint8_t* src, float* dst, int N, int H, int W, int x0, int cw, int erode, int mode, int S, dg_stream_t s);
/* ---- training augmentation: random mirror (DG_AUG_FLIP) and scale-jitter crop (DG_AUG_CROP), on the device ----------------
 * One training image, output size S: prepare it at L >= S exactly as dg_image_prep does (same crop, erosion, mode), take the window
 * [oy, oy + S) x [ox, ox + S), 0 <= ox, oy <= L - S, and mirror it left-right when flip.  dg_image_prep_aug computes only the S x S output:
 * its pixel (y, x) is pixel (oy + y, ox + (flip ? S - 1 - x : x)) of the size-L preparation, bitwise what dg_image_prep at L followed by
 * the slice and the mirror gives; with L = S and a zero record it is bitwise dg_image_prep at S.
 * A record is four int32 (ox, oy, flip, 0); a table is device int32 [n][4], 16-byte aligned.
 *
 * dg_augment_draw fills a table: record j is a pure function of (seed, rank, iteration, domain 0 = A | 1 = B, j) -- no generator state, no
 * host value, no copy, no synchronisation.  With mix = the SplitMix64 output function (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 * z *= 0x94D049BB133111EB; z ^= z >> 31), G = 0x9E3779B97F4A7C15 and all arithmetic modulo 2^64:
 *   k = mix(seed + G); k = mix(k ^ (uint64(uint32(rank)) << 32 | uint32(domain))); k = mix(k ^ uint64(iteration));
 *   a = mix(k + G (2j + 1)); b = mix(k + G (2j + 2)); w0 = a >> 32, w1 = low 32 bits of a, w2 = b >> 32;
 *   flip = w0 >> 31 (0 without DG_AUG_FLIP); ox = (uint64(w1) (L - S + 1)) >> 32, oy likewise from w2 (both 0 without DG_AUG_CROP).
 *
 * dg_image_prep_aug: sample i uses recs[rec_index[i]], or recs[i] when rec_index is NULL (rec_index: device int32 [N]; a launch over the
 * images of one size out of a mixed-size batch passes their batch positions).  Every rec_index value must name a row of `recs`.  The
 * record VALUES need no trust: offsets are clamped to [0, L - S], and every source coordinate is clamped into the cropped image.
 * dg_augment_f32: the same on a resident float batch [N][3][S][S] -> [N][3][S][S] (no overlap): float bilinear resize S -> L (the sampling
 * and float arithmetic of mode 0, no / 255; a tap of weight exactly 0 is left out), window, mirror; L = S with a zero record copies bitwise. */
#define DG_AUG_FLIP 1
#define DG_AUG_CROP 2
int dg_augment_draw(uint64_t seed, int rank, int64_t iteration, int domain, int n, int S, int L, int flags,
                    int32_t* recs /* device [n][4]: ox, oy, flip, 0 */, dg_stream_t s);
int dg_image_prep_aug(const uint8_t* src, float* dst, int N, int H, int W, int x0, int cw, int erode, int mode, int S, int L,
                      const int32_t* recs, const int32_t* rec_index /* or NULL */, dg_stream_t s);
int dg_augment_f32(const float* src, float* dst, int N, int S, int L, const int32_t* recs, dg_stream_t s);
/* ---- image history pool of the discriminators (Shrivastava et al. 2017; CycleGAN's ImagePool.query) ----------------------
 * A pool is a buffer of P image slots of `elems` floats for one domain, `filled` of them in use (0 <= filled <= P).  A batch x[0..n) is
 * processed IN ORDER; sample j does one of three things:
 *   insert (filled + j < P):  pool[filled + j] = x[j], out[j] = x[j];
 *   otherwise one bit and one slot s uniform in [0, P) are drawn --
 *   swap (bit set):  out[j] = pool[s], then pool[s] = x[j];        pass (bit clear):  out[j] = x[j];
 * afterwards filled = min(P, filled + n).  A later sample of the batch that draws a slot an earlier sample i touched receives x[i].
 *
 * The draw is a pure function of (seed, rank, iteration, domain 0 = A | 1 = B, j): the key chain of dg_augment_draw (mix, G as above) with
 * one more link, so that a pool draw never coincides with an augmentation draw of the same (seed, rank, iteration, domain):
 *   k = mix(seed + G); k = mix(k ^ (uint64(uint32(rank)) << 32 | uint32(domain))); k = mix(k ^ uint64(iteration)); k = mix(k ^ 0x706F6F6C);
 *   a = mix(k + G (j + 1));  swap = a >> 63;  s = (uint64(low 32 bits of a) P) >> 32.
 *
 * dg_pool_draw resolves the in-order semantics of one batch into a record table, device int32 [n][4] = (src, slot, st_src, 0), 16-byte
 * aligned, which one parallel launch can apply without a read / write race on a slot:
 *   out[j] = pool_before[slot] if src == -1, else x[src];
 *   if slot >= 0: pool[slot] = x[st_src], written by the thread(s) of sample j, after their read of that slot where they read it.
 * With "touch" = insert or swap, prev(j) = the largest i < j touching j's slot (-1: none) and last(j) = the largest i >= j touching it:
 *   pass (j, -1, j, 0);  insert (j, s, last, 0);  swap with prev < 0 (-1, s, last, 0);  swap with prev >= 0 (prev, -1, j, 0).
 * So only the first toucher of a slot carries its store, the stored image is the last toucher's, and no slot is read by one record and
 * written by another.  Rows past n are left untouched.  1 <= n <= 4096 (every thread scans the batch), P >= 1, 0 <= filled <= P.
 *
 * dg_pool_exchange applies a table in ONE launch: x, out [n][elems] and pool [P][elems] floats (elems = 3 S S), pairwise disjoint.  A copy:
 * every bit pattern (NaN payloads, denormals) survives; 16 bytes per lane where the three bases are 16-byte aligned and elems % 4 == 0,
 * else 4.  The record VALUES need no trust: a record with a field out of range (src outside [-1, n), slot outside [-1, P), st_src outside
 * [0, n), or src == -1 without a slot) is applied as the pass record (j, -1, j, 0).  A hand-made table that names one slot twice is
 * memory-safe, but which writer wins is unspecified.  The caller advances `filled`. */
int dg_pool_draw(uint64_t seed, int rank, int64_t iteration, int domain, int n, int P, int filled,
                 int32_t* recs /* device [n][4]: src, slot, st_src, 0 */, dg_stream_t s);
int dg_pool_exchange(const float* x, float* pool, float* out, int n, int P, size_t elems, const int32_t* recs, dg_stream_t s);
/* ---- differentiable augmentation of the discriminators' inputs (Zhao et al., NeurIPS 2020, "DiffAugment") ----------------------
 * One random, differentiable transform per sample on everything a discriminator sees.  The published policy color,translation,cutout is
 * defined on x' = 2x - 1 in [-1, 1]; images here live in [0, 1], so it is implemented CONJUGATED by x = (x' + 1) / 2: the brightness
 * amplitude is halved, and translation padding and cutout fill with 0.5 instead of 0.  x, z: float [n][3][S][S] (NCHW).
 *
 * With T = floor(S / 8 + 0.5) and cs = floor(S / 2 + 0.5), the record of a sample is eight int32
 *   (tx, ty, cx0, cy0, bits(b), bits(s), bits(c), 0);        a table is device int32 [n][8], 16-byte aligned.
 * Stages, in this order; a stage outside `flags` is not evaluated at all (its record fields are not read), so a geometry-only policy is
 * a pure copy of bit patterns:
 *   DG_DIFFAUG_COLOR, fp32:  brightness v = x + b;  saturation m1 = (v0 + v1 + v2) / 3 per pixel, v = (v - m1) s + m1;
 *                            contrast m2 = mean of v over the sample's 3 S S values, v = (v - m2) c + m2.
 *                            (Saturation keeps each pixel's channel mean and brightness shifts it by b: m2 = mean(x) + b.)
 *   DG_DIFFAUG_TRANSLATION, DG_DIFFAUG_CUTOUT:
 *                            z(ch, y, x) = v(ch, y + ty, x + tx) where (y + ty, x + tx) lies inside the image and (y, x) is not in the
 *                            cut square [cy0, cy0 + cs) x [cx0, cx0 + cs) (clipped by the image; cx0, cy0 may be negative), else 0.5.
 * Backward = the adjoint of the linear part (the op is affine in x: nothing of x is saved), a gather, no float atomics:
 *   g(ch, y', x') = dz(ch, y' - ty, x' - tx) where that position is inside the image and not in the cut square, else 0;
 *   with COLOR  dx = s c g + (1 - s) c chanmean(g) + (1 - c) G,  G = the sample's mean of g;  without, dx = g.
 *
 * dg_diffaug_draw fills a table: record j is a pure function of (seed, rank, iteration, domain 0 = A | 1 = B, role 0 = real batch |
 * 1 = fake batch, j).  The key chain of dg_augment_draw (mix, G as above) with one more link:
 *   k = mix(seed + G); k = mix(k ^ (uint64(uint32(rank)) << 32 | uint32(domain))); k = mix(k ^ uint64(iteration));
 *   k = mix(k ^ (0x6469666600000000 | role));        q_i = mix(k + G (4j + i)), i = 1..4;
 *   unit(w) = float(w >> 8) 2^-24;  range(w, lo, count) = lo + ((uint64(w) count) >> 32);  hi / lo = the high / low 32 bits;
 *   b = (unit(hi q_1) - 0.5) 0.5;  s = 2 unit(lo q_1);  c = unit(hi q_2) + 0.5   (fp32 arithmetic);
 *   tx = range(lo q_2, -T, 2T + 1);  ty = range(hi q_3, -T, 2T + 1);
 *   cx0 = range(lo q_3, 0, S + 1 - cs % 2) - cs / 2;  cy0 likewise from hi q_4   (the published offset, uniform over S + 1 - cs % 2 values).
 * Fields of stages outside `flags` hold their neutral values (0, 0, 0, 0, 0.0f, 1.0f, 1.0f).  Rows past n are left untouched.
 *
 * The record VALUES need no trust: any int32 in tx / ty / cx0 / cy0 (INT_MIN and INT_MAX included) is memory-safe -- coordinates are
 * computed in 64 bits --, and any float bits are allowed as factors; a NaN factor or pixel poisons its own sample only.
 *
 * Launches: one gather pass; with COLOR a statistics pass in front of it, which leaves parts(S) = min(64, ceil(3 S S / 8192)) fp64 partial
 * sums per sample in the workspace (forward: of x; backward: of g) -- a fixed partition of the sample, fixed summation order inside a
 * block and over the partials, no atomics: bitwise repeatable, independent of stream, of the batch and of the grouping.  The workspace is
 * dg_diffaug_workspace_bytes(n, S, flags) = n parts(S) 8 bytes per problem (0 without COLOR), 8-byte aligned.  16 bytes per lane where
 * every base is 16-byte aligned and S % 4 == 0 (a sample whose tx is no multiple of 4 reads its shifted rows in 4-byte pieces and still
 * stores 16), else 4.  1 <= n <= 4096, 2 <= S <= 32768; no output may overlap an input or another output of the launch.
 * The *_g forms run `groups` (1..DG_MAX_GROUPS) problems of one (n, S, flags) in ONE launch per pass, bitwise the single calls. */
#define DG_DIFFAUG_COLOR 1
#define DG_DIFFAUG_TRANSLATION 2
#define DG_DIFFAUG_CUTOUT 4
#define DG_DIFFAUG_ALL 7
int dg_diffaug_draw(uint64_t seed, int rank, int64_t iteration, int domain, int role, int n, int S, int flags,
                    int32_t* recs /* device [n][8] */, dg_stream_t s);
size_t dg_diffaug_workspace_bytes(int n, int S, int flags);
int dg_diffaug_fwd(const float* x, float* z, int n, int S, int flags, const int32_t* recs, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_diffaug_bwd(const float* dz, float* dx, int n, int S, int flags, const int32_t* recs, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_diffaug_fwd_g(int groups, const float* const* x, float* const* z, int n, int S, int flags, const int32_t* const* recs,
                     void* const* ws, size_t ws_bytes, dg_stream_t s);
int dg_diffaug_bwd_g(int groups, const float* const* dz, float* const* dx, int n, int S, int flags, const int32_t* const* recs,
                     void* const* ws, size_t ws_bytes, dg_stream_t s);
/* ---- adaptive discriminator augmentation (Karras et al., NeurIPS 2020, "ADA"): p, r_t and the controller on the device ----------------
 * Every stage of the differentiable augmentation is applied to a sample with a probability p, and a controller moves p by an overfitting
 * measure of the discriminator, r_t = E[sign(D(real) - threshold)], towards a target.  p, the window of signs and the controller live in
 * device memory: the host never reads them to drive a launch.  State per discriminator:
 *   ctl: device double[8], 8-byte aligned = (p, r_t of the last closed window (NaN before the first), updates done, real outputs counted
 *        in total, the last adjustment, 0, 0, 0);
 *   acc: device float[2] = (window sum of signs, window count).  Both are integer-valued: exact below 2^24, and a SUM all-reduce of them
 *        over data-parallel ranks is order-independent.
 *
 * dg_diffaug_draw_p fills the table of dg_diffaug_draw with each stage in `flags` kept, per sample and independently, with probability
 * (float)*p (one rounding of the device double, read BY THE KERNEL).  The gate words come from one more link of dg_diffaug_draw's key
 * chain (the per-sample stride of q_1..q_4 is 4, so they are no further q_i):
 *   k2 = mix(k ^ 0x6164610000000000);  g_1 = mix(k2 + G (2j + 1));  g_2 = mix(k2 + G (2j + 2));
 *   u_color = unit(hi g_1);  u_translation = unit(lo g_1);  u_cutout = unit(hi g_2);       a stage is kept iff u < (float)p,
 * so p = 1 keeps every stage (the table is dg_diffaug_draw's bit for bit) and p = 0 keeps none.  A stage that is not kept writes its
 * neutral fields: colour (0.0f, 1.0f, 1.0f), translation (0, 0), cutout (cx0, cy0) = (S, S) -- an EMPTY square, because the apply kernels
 * still evaluate the stage.  Arguments are refused as by dg_diffaug_draw; p must be non-null and 8-byte aligned.
 *
 * dg_ada_accumulate adds one batch of discriminator outputs to a window: acc[0] += sum over i < n of ((v_i > thr) - (v_i < thr)),
 * acc[1] += n.  The sign comes from the two comparisons: a NaN and v == thr add 0 to the sum and 1 to the count.  1 <= n <= 65536; ONE
 * workgroup, integer partials in a fixed tree, no atomics, one lane updates acc.  thr: 0.5 on sigmoid outputs, 0 on logits
 * (real label / 2 for the least-squares objective).
 *
 * dg_ada_update closes a window, in one lane.  acc[1] == 0: nothing changes.  Otherwise, in this order, every operation rounded once:
 *   rt = double(acc[0]) / double(acc[1]);   adj = double(acc[1]) step_per_image;
 *   a = +adj if rt > target, -adj if rt < target, 0 if equal;   p = min(p_max, max(0, p + a));
 *   ctl[1] = rt;  ctl[2] += 1;  ctl[3] += acc[1];  ctl[4] = a;   acc[0] = acc[1] = 0.
 * -1 < target < 1, 0 <= step_per_image <= 1, 0 <= p_max <= 1. */
int dg_diffaug_draw_p(uint64_t seed, int rank, int64_t iteration, int domain, int role, int n, int S, int flags,
                      const double* p /* device, 8-byte aligned */, int32_t* recs /* device [n][8] */, dg_stream_t s);
int dg_ada_accumulate(const float* d_out, int n, float threshold, float* acc /* device [2] */, dg_stream_t s);
int dg_ada_update(double* ctl /* device [8] */, float* acc /* device [2] */, double target, double step_per_image, double p_max,
                  dg_stream_t s);
/* ---- sample grids (image_translation.py:170-209): the inverse of the ingest, tiled -------------------------
   src: HOST table of `cols` device pointers, each a float batch [n_c][3][S][S] (NCHW, n_c >= rows).
   canvas: device uint8 [Hc][Wc][3], Hc = rows*(S+gap)+gap, Wc = cols*(S+gap)+gap.
   Cell (r, c) holds image r of src[c]; every byte outside the cells is `bg`.
   pixel = (uint8) rintf(clamp(x, 0, 1) * 255.0f)   (round half to even; NaN -> 0)
   1 <= cols <= 8, rows >= 1, S >= 1 (any S), gap >= 0, 0 <= bg <= 255.  One launch writes the whole canvas, gutters included.
   cols = 1, gap = 0 is float [n][3][S][S] -> uint8 [n][S][S][3], the inverse of dg_u8hwc_to_f32chw for all 256 values. */
int dg_sample_grid_u8(const float* const* src, int cols, int rows, int S, int gap, int bg, uint8_t* canvas, dg_stream_t s);
/* ---- held-out image metrics (evaluate.py): per image pair MSE, MAE and SSIM of two float batches [n][3][S][S] (NCHW, any 4-byte
   alignment), values taken as they are (no clamp, no quantisation; data range 1).
   out: device float [n][3] = { mean (x-y)^2, mean |x-y|, SSIM }.  SSIM (Wang et al. 2004): 11 x 11 Gaussian window, sigma 1.5
   (normalised in double, rounded once to fp32, 2-D weight g[i] g[j]), the (S-10)^2 "valid" windows per channel, C1 = 0.01^2,
   C2 = 0.03^2, mean over the 3 channels and all windows.  S >= 11, n >= 1.
   ws: dg_image_metrics_workspace_bytes(n, S) bytes, 8-byte aligned (fp64 partials, n times a function of S).
   fp32 inside a thread, fp64 from the wave sum on, fixed order, no atomics: bitwise repeatable, and row i does not depend on n or on
   the other pairs (a NaN / inf in pair i reaches row i only). */
size_t dg_image_metrics_workspace_bytes(int n, int S);
int dg_image_metrics(const float* x, const float* y, int n, int S, float* out /* [n][3] */, void* ws, size_t ws_bytes, dg_stream_t s);
/* ---- reconstruction loss (trainer.py --recon_loss; csrc/recon.hip): the trainable form of the numbers above.  x (the reconstruction)
   and t (the real image): float [n][3][S][S] (NCHW, any 4-byte alignment); w: three HOST floats (w_mse, w_l1, w_ssim), finite, >= 0,
   not all 0.
     loss = w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ssim (1 - mean over the n 3 (S - 10)^2 valid windows of SSIM)
   SSIM is exactly the quantity of dg_image_metrics (same window, constants, data range 1); the mean over all windows equals the mean of
   the per-image values.  S >= 11 when w_ssim > 0; a term of weight 0 is not evaluated (w_ssim == 0: a plain streaming pass, any S >= 1).
   loss: one device float per problem, written once (fp32 inside a thread, fp64 from the wave sum on, fixed order: bitwise repeatable).
   ws: dg_recon_loss_workspace_bytes(n, S) bytes per problem, 8-byte aligned.
   bwd: the gradient with respect to x only (t is data), gout a device scalar:
     dx = gout ( w_mse 2 (x - t) / N + w_l1 sign(x - t) / N - w_ssim d(mean SSIM) / dx ),  N = 3 n S^2,  sign(0) = 0
   in one pass that overwrites dx; the combination is formed in double and rounded once.  With A1 = 2 mx my + C1, A2 = 2 sxy + C2,
   B1 = mx^2 + my^2 + C1, B2 = sx2 + sy2 + C2 per window p:
     dmu = 2 my A2 / (B1 B2) - 2 mx A1 A2 / (B1^2 B2),  dsig = -A1 A2 / (B1 B2^2),  dc = 2 A1 / (B1 B2)
     a = dmu - 2 mx dsig - my dc,  b = 2 dsig,  c = dc
     d(mean SSIM) / dx(q) = [ (w * a)(q) + x(q) (w * b)(q) + t(q) (w * c)(q) ] / (3 n (S - 10)^2)
   where (w * f)(q) sums w(q - p) f(p) over the valid windows p that contain pixel q.  The maps a, b, c are recomputed by the backward
   (nothing is saved by the forward); each output pixel gathers its windows: no atomics, two calls give the same bits, and a NaN / inf in
   one image stays in that image's rows of dx.  16-byte loads when S % 4 == 0 and every pointer is 16-byte aligned, scalar loads
   otherwise.  No host synchronisation, no allocation: capturable.  The *_g forms run `groups` (1..DG_MAX_GROUPS) problems of one (n, S, w)
   in one launch per kernel, bitwise the single calls. */
size_t dg_recon_loss_workspace_bytes(int n, int S);
int dg_recon_loss_fwd(const float* x, const float* t, int n, int S, const float* w /* host [3] */, float* loss, void* ws, size_t ws_bytes,
                      dg_stream_t s);
int dg_recon_loss_bwd(const float* x, const float* t, int n, int S, const float* w /* host [3] */, const float* gout, float* dx, dg_stream_t s);
int dg_recon_loss_fwd_g(int groups, const float* const* x, const float* const* t, int n, int S, const float* w /* host [3] */,
                        float* const* loss, void* const* ws, size_t ws_bytes, dg_stream_t s);
int dg_recon_loss_bwd_g(int groups, const float* const* x, const float* const* t, int n, int S, const float* w /* host [3] */,
                        const float* const* gout, float* const* dx, dg_stream_t s);
/* ---- multi-scale SSIM (trainer.py --recon_loss ms_ssim / l1_ms_ssim, evaluate.py --ms_ssim; csrc/msssim.hip; Wang, Simoncelli, Bovik
   2003).  x, t: float [n][3][S][S] (NCHW, any 4-byte alignment); M scales; level 0 is the image.
   Pyramid.  Level j + 1 has side S_{j+1} = floor(S_j / 2); its pixel (y, x) is 0.25f * ((a + b) + (c + d)) of the 2 x 2 block
   a = (2y, 2x), b = (2y, 2x + 1), c = (2y + 1, 2x), d = (2y + 1, 2x + 1) of level j, in fp32 in that order; a last odd row or column is
   dropped.
   Scales.  Every scale needs S_j >= 11: dg_ms_ssim_max_scales(S) = min(5, number of j with S >> j >= 11) (0 for S < 11; 11 -> 1,
   22 -> 2, 64 -> 3, 176 and more -> 5), and 1 <= M <= that maximum.
   Per scale j, image i and channel c, with the window, the constants, the "valid" corners and the factors A1, A2, B1, B2 of the
   reconstruction loss above:
     V_j = mean over the (S_j - 10)^2 windows of A2 / B2             for j < M - 1   (contrast-structure)
     V_{M-1} = mean over the (S_{M-1} - 10)^2 windows of (A1 A2) / (B1 B2)            (the full SSIM at the coarsest scale)
   Exponents: beta_j = the first M of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) divided by their sum, the division in double, rounded once
   to fp32.
     ms(i, c) = prod_j V_j^beta_j  if every V_j > 0;  otherwise ms(i, c) = 0 and its gradient is exactly 0 (the clamp of the usual
     implementations with the subgradient fixed); a NaN V_j gives NaN.
   dg_image_ms_ssim: out[i] = mean over c of ms(i, c); row i does not depend on n or on the other pairs.
     loss = w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ms (1 - mean over i, c of ms(i, c))
   w: three HOST floats (w_mse, w_l1, w_ms), finite, >= 0, not all 0; a term of weight 0 is not evaluated.  loss: one device float per
   problem, written once (fp32 inside a thread, fp64 from the wave sum on, fixed order, no atomics: bitwise repeatable).
   bwd: the gradient with respect to x only, gout a device scalar.  With k_j(i, c) = beta_j ms / V_j (0 for a channel with ms = 0) the
   gradient at scale j is
     g_j(q) = -w_ms k_j / (3 n (S_j - 10)^2) [ (w * a)(q) + x_j(q) (w * b)(q) + t_j(q) (w * c)(q) ]
   in the gather form of the reconstruction loss above (a = dmu - 2 mx dsig - my dc, b = 2 dsig, c = dc), where the last scale uses that
   loss's dmu, dsig, dc and a scale j < M - 1 those of A2 / B2 alone:  dmu = 0,  dsig = -A2 / B2^2,  dc = 2 / B2;
     dx(q) = gout ( w_mse 2 (x - t) / N + w_l1 sign(x - t) / N + sum_j g_j(q >> j) / 4^j ),  N = 3 n S^2,
   the term of scale j for q inside the 2^j S_j square only.  One pass overwrites dx; the combination is formed in double and rounded
   once; gather only: no atomics, two calls give the same bits, a NaN / inf in image i stays in image i's rows of dx.
   save: the forward fills this caller-owned buffer of dg_ms_ssim_save_bytes(n, S, M) bytes (16-byte aligned) with the pyramid levels of x
   and t and the table k [n][3][M]; the backward reads it (and x, t).  ws: per problem, 16-byte aligned, dg_ms_ssim_workspace_bytes(n, S,
   M) bytes for the forward and the metric, dg_ms_ssim_bwd_workspace_bytes(n, S, M) (one float per pixel of levels 1 .. M-1) for the
   backward.  w_ms == 0: no pyramid is built, no stencil runs in either direction, save is neither written nor read.  No host synchronisation, no allocation: capturable.  The *_g forms run `groups` (1..DG_MAX_GROUPS)
   problems of one (n, S, M, w) in one launch per kernel, bitwise the single calls.  Refused with a message and nothing launched: null or
   misaligned pointers, n < 1, S < 11, M out of range, a short workspace or save buffer, bad weights. */
int dg_ms_ssim_max_scales(int S);
size_t dg_ms_ssim_workspace_bytes(int n, int S, int M);
size_t dg_ms_ssim_bwd_workspace_bytes(int n, int S, int M);
size_t dg_ms_ssim_save_bytes(int n, int S, int M);
int dg_ms_ssim_loss_fwd(const float* x, const float* t, int n, int S, int M, const float* w /* host [3] */, float* loss, void* save,
                        size_t save_bytes, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_ms_ssim_loss_bwd(const float* x, const float* t, int n, int S, int M, const float* w /* host [3] */, const float* gout, const void* save,
                        size_t save_bytes, float* dx, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_ms_ssim_loss_fwd_g(int groups, const float* const* x, const float* const* t, int n, int S, int M, const float* w /* host [3] */,
                          float* const* loss, void* const* save, size_t save_bytes, void* const* ws, size_t ws_bytes, dg_stream_t s);
int dg_ms_ssim_loss_bwd_g(int groups, const float* const* x, const float* const* t, int n, int S, int M, const float* w /* host [3] */,
                          const float* const* gout, const void* const* save, size_t save_bytes, float* const* dx, void* const* ws,
                          size_t ws_bytes, dg_stream_t s);
int dg_image_ms_ssim(const float* x, const float* y, int n, int S, int M, float* out /* [n] */, void* ws, size_t ws_bytes, dg_stream_t s);
/* ---- sliced Wasserstein distance on Laplacian-pyramid patches (evaluate.py; Karras et al., ICLR 2018, "Progressive Growing of GANs",
 * section 5): a score for UNPAIRED sets, no network.  x, y: float [n][3][S][S] (NCHW), values as they are (no clamp), S >= 16.
 *
 * Levels.  R_0 = S; level l + 1 exists while R_l is even and R_l / 2 >= 16, with R_{l+1} = R_l / 2; L = dg_swd_levels(S) levels
 * (16 -> 1, 32 -> 2, 34 -> 2 (34, 17), 48 -> 2, 64 -> 3, 96 -> 3, 512 -> 6; 0 for S < 16).  An odd R occurs only at the last level.
 * Pyramid.  w = [1 4 6 4 1] / 16, separable; MIRROR border (index -1 -> 1, R -> R - 2: no edge repeat; scipy.ndimage mode='mirror', not
 * 'reflect').  down(a) = filter, then every second row and column from 0.  up(a) = a at the even positions of a zero image of twice the
 * size, filtered with 4 w (x) w.  G_0 = x, G_{l+1} = down(G_l); level l < L - 1 is G_l - up(G_{l+1}), level L - 1 is G_{L-1}.
 *   dg_lap_pyramid writes all levels into `out`, level l as [n][3][R_l][R_l] at float offset 3 n (R_0^2 + ... + R_{l-1}^2);
 *   dg_lap_pyramid_elems(n, S) floats in all.  x and out do not overlap; any 4-byte alignment (16-byte lanes where alignment and R % 4
 *   allow, the same bits either way).  fp32.
 * Patches.  P patches of 7 x 7 x 3 per image and level, top-left (oy, ox) uniform in [0, R - 7]^2, a pure function of (seed, level,
 * image j, patch p): the key chain of dg_augment_draw (mix, G as above) with a link of its own --
 *   k = mix(seed + G); k = mix(k ^ (0x7377640000000000 | level)); q = mix(k + G (j P + p + 1));
 *   oy = (uint64(high 32 bits of q) (R - 6)) >> 32; ox likewise from the low 32 bits.
 * No rank, no iteration: every event scores the same patches, and one table serves both sets.  dg_swd_draw fills device int32
 * [n][P][2] = (oy, ox), 8-byte aligned; rows past n are untouched.  R >= 7.
 * Descriptors.  dg_swd_descriptors gathers desc [n P][147], a descriptor ordered [channel][dy][dx], as a bit copy of `level`
 * ([n][3][R][R]); the record VALUES need no trust: offsets are clamped to [0, R - 7].  stats: device double [3][2] = per channel the
 * mean and the population standard deviation (ddof 0) of its n P 49 descriptor values, fp64, two passes, fixed partition and order.
 * ws: dg_swd_descriptors_workspace_bytes(n P) bytes, 8-byte aligned.
 * Projection.  dg_swd_project: xhat = (v - mean_c) / std_c (all zeros for a channel whose std is exactly 0 -- the publication divides by
 * zero there), proj[d][i] = sum_k xhat[i][k] dirs[d][k]: float [D][M], M = n P, fp32 fma chain in ascending k (no bf16 rounding).
 * dirs: float [D][147], unit vectors made by the caller (evaluate.py: standard normal from torch.Generator().manual_seed(seed), scaled
 * to unit length in float64, rounded once).
 * Distance.  dg_swd_sort_rows sorts every row of [D][M] ascending in place; dg_swd_row_distance sorts a copy of each row of `proj` and
 * writes out[d] = mean_i |a_(i) - ref_sorted[d][i]| (double [D]; fp32 terms, fp64 from the wave sum on, fixed order, no atomics: the
 * same input gives the same bits, and exchanging the two sets gives the same bits); the sorted row goes to sorted_out[d] unless that is
 * NULL.  SWD_l = 1000 mean_d out[d] is the caller's.  One workgroup sorts one row in LDS, so 1 <= M <= DG_SWD_MAX_ROW (32768 floats =
 * 128 KiB of the CU's 160 KiB), D >= 1.  The order is total on the bit patterns: -inf first, +inf last, NaNs beyond them; a NaN anywhere
 * in a row makes that row's distance NaN and no other's. */
#define DG_SWD_MAX_ROW 32768
int dg_swd_max_row(void);
int dg_swd_levels(int S);
size_t dg_lap_pyramid_elems(int n, int S);
int dg_lap_pyramid(const float* x, int n, int S, float* out, dg_stream_t s);
int dg_swd_draw(uint64_t seed, int level, int n, int R, int P, int32_t* recs /* device [n][P][2]: oy, ox */, dg_stream_t s);
size_t dg_swd_descriptors_workspace_bytes(int M);
int dg_swd_descriptors(const float* level, int n, int R, int P, const int32_t* recs, float* desc /* [n P][147] */, double* stats /* [3][2] */,
                       void* ws, size_t ws_bytes, dg_stream_t s);
int dg_swd_project(const float* desc, const double* stats, int M, const float* dirs /* [D][147] */, int D, float* proj /* [D][M] */,
                   dg_stream_t s);
int dg_swd_sort_rows(float* proj /* [D][M] */, int D, int M, dg_stream_t s);
int dg_swd_row_distance(const float* proj, const float* ref_sorted, int D, int M, double* out /* [D] */, float* sorted_out /* or NULL */,
                        dg_stream_t s);

/* ---- bf16 shadow operands for the bf16 matrix path (option "bf16" = 1; BASELINE configs[4]) ---------------------
 * A shadow is a bf16 (RNE) copy of an fp32 tensor with the same logical layout, written by the tensor's PRODUCER so that
 * the conv kernels read half the operand bytes and convert nothing: dg_adam_step_flat form 1 (weights, +2 B/param),
 * dg_bn_act_fwd_bf16 / dg_bn_act_bwd_bf16 (activations / gradients: +2 B/element on passes of 8 / 12 B/element),
 * dg_f32_to_bf16 (initial weight shadow; the first layer's output).  The *_mixed convolutions take either operand as fp32 (flag 0) or bf16 (flag 1)
 * and return the fp32 convolution of the RNE-rounded operands (same summation order per output element whichever operand
 * form is passed).  With BOTH operands bf16 and a GEMM of at least 192 rows and columns the work goes to the LDS-DMA kernel
 * (csrc/igemm_dma.hip: 256x256 tile, operand tiles global -> LDS by `buffer_load ... lds`; option "no_dma" 1 keeps the
 * register-staged tiles).  dg_conv_bf16_operands_ok: 0 = the shape has no bf16 kernel, 1 = register-staged bf16 tiles,
 * 2 = the LDS-DMA kernel when both operands are bf16.  A bf16 operand is read in 16-byte granules of 8 elements, which must not
 * straddle a row of its GEMM operand: a bf16 dy (input gradient, weight gradient) needs K % 8 == 0, a bf16 x of the weight gradient
 * C % 8 == 0 -- otherwise that operand flag is refused (pass the fp32 tensor: the kernel rounds it itself, the same values). */
int dg_f32_to_bf16(const float* x, void* y_bf16, size_t n, dg_stream_t s);
int dg_bn_act_fwd_bf16(const float* y, float* z, void* z_bf16, int M, int C, const float* saved, const float* gamma,
                       const float* beta, int act, float slope, dg_stream_t stream);
int dg_bn_act_bwd_bf16(const float* dz, const float* y, float* dy, void* dy_bf16, int M, int C, const float* saved,
                       const float* gamma, const float* beta, int act, float slope, float* dgamma, float* dbeta,
                       int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_bf16_operands_ok(int op, int N, int H, int W, int C, int K, int stride, int pad);
/* stat (may be NULL): fused BatchNorm partial statistics of the OUTPUT, taken from the fp32 accumulators before the output is
 * rounded: dg_conv_mixed_bnstats_rows(op, ..., operand flags) rows of 3 * columns + 4 floats (0 rows: this plan emits none),
 * merged by dg_bn_stats_from_partials */
int dg_conv_mixed_bnstats_rows(int op, int N, int H, int W, int C, int K, int stride, int pad, int a_bf16, int b_bf16);
int dg_conv_fwd_mixed(const void* x, int x_bf16, const void* w, int w_bf16, void* y, int y_bf16, int N, int H, int W, int C, int K,
                      int stride, int pad, float* stat, size_t stat_floats, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_dgrad_mixed(const void* dy, int dy_bf16, const void* w, int w_bf16, void* dx, int dx_bf16, int N, int H, int W, int C, int K,
                        int stride, int pad, float* stat, size_t stat_floats, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_wgrad_mixed(const void* dy, int dy_bf16, const void* x, int x_bf16, float* dw, int N, int H, int W, int C, int K,
                        int stride, int pad, int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream);

/* ---- fp32 operands as THREE bf16 PLANES for the f32x3 matrix path (option "bf16" = 2; DiscoGANTrainer(mfma_dtype="f32x3")) ----
 * A plane triple of an fp32 tensor v: hi = bf16(v) (RNE), mid = bf16(v - hi), lo = bf16(v - hi - mid) -- 24 significand
 * bits of v (both subtractions are exact in fp32).  Layout: plane-major, each plane in the tensor's own logical layout;
 * `*_plane` = distance between planes in BYTES (multiple of 16, >= 2 * numel; a weight inside a flat parameter group uses
 * the group's distance), dg_f32_to_bf16x3 / dg_adam_step_flat take it in ELEMENTS (multiple of 8).  Written by the
 * tensor's producer: dg_adam_step_flat form 3 (weights, +6 B/param), dg_bn_act_fwd_x3 / dg_bn_act_bwd_x3 (activations /
 * gradients), dg_f32_to_bf16x3 (everything else).  The *_x3 convolutions return the fp32 convolution with the same six
 * bf16 MFMAs per product block and the same reduction order as the fp32-pointer entry points under option "bf16" = 2
 * (bit-identical on an unsplit GEMM), without the per-element split in the conv kernel: csrc/igemm_dma_x3.hip, operand
 * planes global -> LDS by `buffer_load ... lds`, 256x256 tile.  dg_conv_x3_planes_ok: 1 = the shape has the plane kernel
 * (GEMM of at least 192 rows and columns, C % 16 == 0 forward / K % 16 == 0 input-grad; weight gradients from 96 rows; stride-2
 * input-grads with C <= 128 and a 32..128 pixel wide gradient map: csrc/igemm_dma_x3_dgw.hip), 0 = use dg_conv_fwd / _dgrad /
 * _wgrad.  Outputs are fp32; the caller keeps the fp32 tensors for BatchNorm and the element-wise kernels.
 * dg_conv_fwd_x3 with w_transposed != 0 reads the weight planes as wT[(r, s, c)][k] (k contiguous): a K-tile of the weight
 * operand is then 16 rows of 512 contiguous bytes instead of 256 pieces of 32 bytes (forward K loop 49-81 % -> ~90 % of the
 * matrix rate).  dg_x3_transpose_planes writes that copy for n conv weights of a plane buffer in one launch per 48 weights
 * ([K][J] images, J = 16 C, at element offsets w_off inside each plane; host arrays, any order; the whole table is checked
 * before the first launch). */
int dg_f32_to_bf16x3(const float* x, void* y_planes, size_t n, size_t plane_elems, dg_stream_t s);
int dg_x3_transpose_planes(const void* src_planes, void* dst_planes, size_t plane_elems, const int64_t* w_off, const int* w_K,
                           const int* w_J, int n, dg_stream_t s);
/* One f32x3 Adam step of a whole flat group of `numel` parameters that also writes the transposed weight planes: the bits of
 * dg_adam_step_flat form 3 (ctl == NULL: the host's grad_scale; otherwise scale and go / no-go from ctl) followed by
 * dg_x3_transpose_planes, without reading the plain planes back (40 instead of 34 + 12 B/param).  The group is given as two host
 * lists, each ascending and disjoint in itself and the two disjoint from each other (an overlap is refused): n_w conv weights ([K][J] images at element offsets w_off; K % 64 == 0, J % 64 == 0,
 * w_off % 8 == 0), stepped by 64 x 128 tiles (64 x 64 where J % 128 != 0) that store p, m, v, the plain planes and the [J][K] planes in pt_planes; and n_r plain
 * ranges [r_off, r_off + r_len) (r_off % 8 == 0: BatchNorm vectors, every other weight), stepped in ONE launch per 64 ranges with plain
 * planes only.  Parameters in neither list keep their bits.  All buffers 16-byte aligned; p_planes and pt_planes are [3][plane_elems]. */
int dg_adam_step_group_x3(float* p, const float* g, float* m, float* v, size_t numel, const double* state, float beta1, float beta2,
                          float eps, float weight_decay, float grad_scale, const double* ctl, void* p_planes, void* pt_planes,
                          size_t plane_elems, const int64_t* w_off, const int* w_K, const int* w_J, int n_w, const int64_t* r_off,
                          const int64_t* r_len, int n_r, dg_stream_t s);
/* plane_layout / dy_layout: 0 = pixel-major planes [M][C] (the tensor's own NHWC order); 1 = QUAD-CHUNK planes
 * [M / 4][C / 16][4 pixels][16 channels] (C % 64 == 0, M % 4 == 0): the 16-channel chunk of 4 consecutive pixels is one
 * 128-byte line, a 4-pixel block of all channels stays one contiguous run.  The window input-grad kernel fetches a 16-channel
 * chunk of whole image rows per step: pixel-major that is 32 bytes of every 256- or 512-byte pixel row (each 128-byte line
 * crossed the fabric four times, PMC: 8x the algorithmic bytes); in the quad-chunk layout every fetched line is used whole.
 * Producers: the BatchNorm kernels below, for the two layer shapes per network whose input-grad dg_conv_x3_planes_ok reports
 * as 2; readers: dg_conv_dgrad_x3 (window kernel) and dg_conv_wgrad_x3 (the dy operand: its 16-pixel tile is the same block of
 * bytes, permuted).  Same products in the same order: results are bit-identical to layout 0.
 * z / dy may be NULL in the two *_x3 functions: the planes ARE the tensor (hi + mid + lo reproduces every fp32 value exactly), so
 * when all readers of the result are plane kernels the fp32 copy is not written (14 -> 10 and 26 -> 22 bytes per element). */
int dg_bn_act_fwd_x3(const float* y, float* z, void* z_planes, size_t plane_elems, int plane_layout, int M, int C, const float* saved,
                     const float* gamma, const float* beta, int act, float slope, dg_stream_t stream);
int dg_bn_act_bwd_x3(const float* dz, const float* y, float* dy, void* dy_planes, size_t plane_elems, int plane_layout, int M, int C,
                     const float* saved, const float* gamma, const float* beta, int act, float slope, float* dgamma,
                     float* dbeta, int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream);
/* conv1 forward (+ fused activation) on the f32x3 path that also writes the plane triple of its output (pixel-major), so the next
 * layer's weight-gradient needs no separate split pass over the largest activation of the network (K == 64, tensors < 1 GiB) */
int dg_conv4x4s2_c3_fwd_x3(const float* x_nchw, const float* w, float* y_nhwc, void* y_planes, size_t plane_elems, int N, int H, int W,
                           int K, int act, float slope, dg_stream_t stream);
/* 0: no plane kernel for this (op, shape); 1: yes; 2: yes -- the window input-grad kernel, which prefers dy_layout 1 */
int dg_conv_x3_planes_ok(int op, int N, int H, int W, int C, int K, int stride, int pad);
/* stat (may be NULL): fused BatchNorm partial statistics of the OUTPUT, dg_conv_x3_bnstats_rows(op, ...) rows of 3 * columns + 4
 * floats in the layout of dg_conv_fwd_bnstats (merged by dg_bn_stats_from_partials): the plane kernels' epilogues (or their split-K
 * reduction) sum the fp32 accumulators per column, which removes the separate read pass of dg_bn_train_stats over the conv output. */
int dg_conv_x3_bnstats_rows(int op, int N, int H, int W, int C, int K, int stride, int pad);
int dg_conv_fwd_x3(const void* x_planes, int64_t x_plane, const void* w_planes, int64_t w_plane, int w_transposed, float* y,
                   int N, int H, int W, int C, int K, int stride, int pad, float* stat, size_t stat_floats, void* ws, size_t ws_bytes,
                   dg_stream_t stream);
int dg_conv_dgrad_x3(const void* dy_planes, int64_t dy_plane, int dy_layout, const void* w_planes, int64_t w_plane, float* dx, int N, int H, int W,
                     int C, int K, int stride, int pad, float* stat, size_t stat_floats, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_conv_wgrad_x3(const void* dy_planes, int64_t dy_plane, int dy_layout, const void* x_planes, int64_t x_plane, float* dw, int N, int H, int W,
                     int C, int K, int stride, int pad, int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream);

/* ---- bf16 ACTIVATION STORAGE (option "bf16" = 1; DiscoGANTrainer(mfma_dtype="bf16", act_dtype="bf16")) --------------------
 * Feature maps and their gradients live in HBM as bf16 ONLY (no fp32 copy): the conv epilogues round the fp32
 * accumulators once (y_bf16 / dx_bf16 of the *_mixed convolutions above; never the weight gradient), BatchNorm reads
 * bf16, keeps statistics / normalisation / the backward expression in fp32 / fp64 exactly as the fp32 kernels do and
 * rounds what it stores ("bf16 MFMA + fp32 BatchNorm accum", BASELINE configs[4]).  Per element: forward 8 B instead of
 * 18 (fp32 + shadow), backward 10 B instead of 22.  `io_bf16` = every activation tensor of the call is bf16 (C % 8 == 0);
 * 0 = the fp32 kernels.  The image side (NCHW, 3 channels), weights, BatchNorm parameters / statistics, every gradient
 * of a parameter, losses and Adam stay fp32.  The K == 1 head takes a bf16 x / dx through the *_mixed entry points. */
int dg_bn_train_stats_t(const void* y, int io_bf16, int M, int C, float eps, float momentum, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, float* saved, void* ws, size_t ws_bytes,
                        dg_stream_t stream);
int dg_bn_act_fwd_t(const void* y, void* z, int io_bf16, int M, int C, const float* saved, const float* gamma,
                    const float* beta, int act, float slope, dg_stream_t stream);
int dg_bn_act_bwd_t(const void* dz, const void* y, void* dy, int io_bf16, int M, int C, const float* saved,
                    const float* gamma, const float* beta, int act, float slope, float* dgamma, float* dbeta,
                    int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream);
int dg_act_bwd_t(const void* dy, const void* out, void* dx, int io_bf16, size_t n, int act, float slope, dg_stream_t stream);
/* 3-channel edge layers with the 64-channel NHWC side in bf16 (K == 64 only; the NCHW image side stays fp32) */
int dg_conv4x4s2_c3_fwd_t(const float* x_nchw, const float* w, void* y_nhwc, int y_bf16, int N, int H, int W, int K,
                          int act, float slope, dg_stream_t s);
int dg_conv4x4s2_c3_dgrad_t(const void* dy_nhwc, int dy_bf16, const float* w, float* dx_nchw, int N, int H, int W, int K,
                            int act, void* ws, size_t ws_bytes, dg_stream_t s);
int dg_conv4x4s2_c3_wgrad_t(const void* dy_nhwc, const void* act_out_nhwc /* or NULL with act NONE */, int io_bf16, int act,
                            float slope, const float* x_nchw, float* dw, int N, int H, int W, int K, int accumulate,
                            void* ws, size_t ws_bytes, dg_stream_t s);
/* feature matching on bf16 discriminator features (sums in fp32; dreal / dfake written as bf16) */
int dg_fm_fwd_t(const void* real, const void* fake, int io_bf16, int N, size_t J, float* diff, float* loss, void* ws,
                size_t ws_bytes, dg_stream_t stream);
int dg_fm_bwd_t(const float* diff, int N, size_t J, const float* gout, void* dreal, void* dfake, int io_bf16, dg_stream_t stream);

/* ---- layout helpers ---------------------------------------------------------------------------
 * fp32, N < 65536, C*H*W of one image <= 2^31 - 1 and ceil(C/32) * ceil(H*W/32) <= 16777215 (one image's 32 x 32 tiles lie along
 * grid.x); anything else is refused before a launch. */
int dg_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, dg_stream_t s);
int dg_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, dg_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* DISCOGAN_HIP_H */
