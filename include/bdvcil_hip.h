/*
 * bdvcil_hip.h -- C ABI of libbdvcil_hip.so: MI355X (gfx950) kernels for the TSM
 * class-incremental training hot path of NinV/Background-Debiased-Video-CIL.
 *
 * The reference has NO FFI for this path: its hot path is `mmaction.models` Python executed by
 * PyTorch/cuDNN.  Each entry point below therefore names the reference
 * call site (file:line under /root/reference, or UPSTREAM mmaction2 0.24 / torch op) whose
 * arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative BDV_E* code for argument errors or a positive
 *     hipError_t for launch errors; nothing throws; bdv_last_error() gives a thread-local message.
 *   - the caller owns every buffer (incl. workspaces); pointers are device pointers unless noted;
 *     kernels are enqueued on `stream` (a hipStream_t passed as void*) and never synchronise.
 *   - no global mutable state: re-entrant, thread-safe, hipGraph-capturable.
 *   - activations are fp32 NHWC: [N][H][W][C], N = clips * segments (frames), C % 4 == 0,
 *     16-byte aligned.  Conv weights are [Cout][R][S][Cin] (the storage of a torch
 *     channels_last OIHW tensor).  All arithmetic is fp32 (f32-input MFMA, exact fp32 FMA chains).
 */
#ifndef BDVCIL_HIP_H
#define BDVCIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDV_OK 0
#define BDV_EINVAL (-1)   /* bad shape / alignment / null pointer */
#define BDV_EWORKSPACE (-2) /* workspace too small */

/* Activation storage (`act_dtype` arguments, bdv_conv_geom.act_dtype).  BDV_ACT_F32: every activation / gradient tensor is
 * fp32 (the reference's arithmetic, libs/cil/cil.py:744-756 precision 32; the default and the headline metric).
 * BDV_ACT_BF16: activations, conv outputs and their gradients are stored as bf16 (BASELINE config 5, the reference's
 * `precision=16` counterpart; bf16 instead of fp16: same MFMA rate on gfx950, fp32's exponent range, no loss scaler).  Values
 * widen exactly on load, arithmetic and accumulators stay fp32, stores round to nearest-even; BatchNorm statistics, weights,
 * weight gradients, ReLU masks and everything after the average pool stay fp32.  Convolutions then run the single-product bf16
 * MFMA kernels (pieces = 1) only, and a temporal shift needs fold % 8 == 0 there (fp32 tensors: fold % 4 == 0): the loaders move
 * 16-byte units, eight bf16 channels, under one shift class; bdv_conv_plan_query refuses other folds. */
#define BDV_ACT_F32 0
#define BDV_ACT_BF16 1

/* Geometry of one 2-D convolution site (UPSTREAM mmaction ResNet ConvModule.conv). */
typedef struct bdv_conv_geom {
  int32_t N;      /* frames = clips * T */
  int32_t H, W;   /* input spatial size */
  int32_t Cin;    /* input channels, multiple of 4 */
  int32_t Ho, Wo; /* output spatial size */
  int32_t Cout;   /* output channels, multiple of 64 */
  int32_t R, S;   /* filter size */
  int32_t stride; /* 1 or 2 */
  int32_t pad;
  int32_t T;      /* num_segments (frames per clip); used only when fold > 0 */
  int32_t fold;   /* temporal-shift fold = Cin / shift_div, multiple of 4 (of 8 under BDV_ACT_BF16); 0 = no shift */
  int32_t pad_w;  /* column padding when it differs from `pad` (then `pad` pads rows only); < 0: same as `pad`.
                   * A k x 1 x 1 temporal convolution of an I3D block (UPSTREAM mmaction ResNet3d Bottleneck3d.conv1,
                   * configs/_base_/models/i3d_r50.py:13) runs as a k x 1 conv on the [B][T][H*W][C] view of the same NHWC
                   * storage: N = B, H = T, W = H*W, R = k, S = 1, pad = k / 2, pad_w = 0. */
  int32_t Rt;     /* temporal filter taps of the I3D stem (UPSTREAM ResNet3d.conv1, conv1_kernel = (5, 7, 7),
                   * configs/_base_/models/i3d_r50.py:7); 0 or 1 = a 2-D convolution.  Rt > 1: Cin = 4 only, the bf16-piece
                   * kernels only (bdv_conv_fprop_pl, bdv_conv_wgrad_partial_pl).  N = OUTPUT frames, T = output frames per
                   * clip; the input holds N * st_t frames and output frame n reads the input frames n * st_t + dt - Rt / 2 of
                   * its clip (zeros outside).  Weights [Cout][Rt][R][S][4]. */
  int32_t st_t;   /* temporal stride (1 or 2) when Rt > 1 */
  int32_t act_dtype; /* BDV_ACT_F32 | BDV_ACT_BF16: element type of x / y / dy / dx / add_src and of the fused-statistics `y`
                      * (the plane kernels bdv_conv_fprop_pl / _dgrad_pl / _wgrad_partial_pl with pieces = 1 only; Cin % 32 == 0) */
} bdv_conv_geom;

const char* bdv_last_error(void);
int bdv_abi_version(void);
/* sha256 (hex) of the sources this library was built from, in the Makefile's HASHED order; the binding compares it with
 * the sources it finds in-tree and refuses a stale build. */
const char* bdv_source_hash(void);

/* ---- convolution = implicit GEMM on the MFMA pipes ------------------------------------------
 * fprop replaces F.conv2d inside ConvModule (+ UPSTREAM TemporalShift.shift when fold > 0:
 * channels [0,fold) read frame t+1, [fold,2fold) read frame t-1, zero at clip ends).
 * x [N,H,W,Cin], w [Cout,R,S,Cin], y [N,Ho,Wo,Cout].
 *
 * Two sets of entry points, one per arithmetic:
 *   bdv_conv_fprop / _dgrad / _wgrad / _wgrad_partial        fp32 MFMA (v_mfma_f32_32x32x2_f32, an exact fp32 FMA chain);
 *   bdv_conv_fprop_pl / _dgrad_pl / _wgrad_partial_pl        the bf16-piece entry points (`pieces` = 3, 2 or 1, below).
 * Which kernel a call runs, whether it reads the weight planes and how large its side buffers are is ONE decision,
 * bdv_conv_plan_query; the launches follow the same plan, so a buffer sized from the query is the buffer the kernel writes.
 *
 * Workspaces: bdv_conv_workspace_bytes(g, kind) with kind 0 = fprop, 1 = dgrad, 2 = wgrad (the fp32-MFMA bdv_conv_wgrad), for
 * every arithmetic.  fprop/dgrad use it for the K-split partial accumulators of the remainder tiles (tile counts that do not
 * fill whole rounds of co-resident workgroups on the 256 CUs); passing NULL disables the split (correct, slower on such shapes). */
size_t bdv_conv_workspace_bytes(const bdv_conv_geom* g, int kind);

/* The plan of one call.  kind: 0 fprop, 1 dgrad, 2 wgrad.  arith: 0 = the fp32-MFMA entry points, 1 / 2 / 3 = the bf16-piece
 * entry points with that many pieces, 4 (BDV_ARITH_F16X2) = the two-fp16-piece entry points (bdv_conv_*_f16x2, below).
 * pre: the producer's BatchNorm is applied in the loader (pre_scale, below).
 * Returns BDV_EINVAL (reason in bdv_last_error) where the library has no kernel for the request: dgrad of the Cin = 4 stem,
 * bf16 storage (g->act_dtype) outside pieces = 1 or on a geometry without a plane kernel, pre on a shifted site, ... */
#define BDV_CONV_F32 0       /* 4 waves, fp32 MFMA, 128 x 128 / 128 x 64 tiles */
#define BDV_CONV_C4 1        /* the stem (Cin = 4) on fp32 MFMA */
#define BDV_CONV_C4_X3 2     /* the stem on the bf16-piece K loop (also its temporal taps, Rt > 1) */
#define BDV_CONV_X3 3        /* 4 waves, two workgroups per CU, bf16 pieces, the weight operand from the planes */
#define BDV_CONV_PL 4        /* the plane kernels (8 waves, or the 4-wave 64 x 128 / 128 x 128 tiles) */
#define BDV_CONV_WGRAD_F32 5 /* weight gradient on fp32 MFMA */
#define BDV_CONV_WGRAD_PL 6  /* weight gradient, bf16 pieces split in the loader */
typedef struct bdv_conv_plan {
  int32_t family;       /* BDV_CONV_* */
  int32_t reads_planes; /* fprop / dgrad: the launch needs planes_fprop / planes_dgrad (else they may be NULL and w is read) */
  int32_t stat_rows;    /* fprop / dgrad: rows of the fused-statistics partial, float[2][stat_rows][C] (one per row tile of the
                         * kernel that runs; a stride-2 dgrad has one block of rows per input-parity class) */
  int32_t splits;       /* wgrad: the slab holds this many partial products of dw's size */
  int32_t pre_ok;       /* fprop / wgrad: the same call with pre = 1 is available */
  char kernel[128];     /* the main kernel as a profiler prints it, without the namespace (wgrad: up to the tile size) */
} bdv_conv_plan;
int bdv_conv_plan_query(const bdv_conv_geom* g, int kind, int arith, int pre, bdv_conv_plan* out);

/* bn_partial (optional): float[2][stat_rows][Cout].  When given, the epilogue also writes per-row-tile column sums of y and
 * y*y (the BatchNorm batch statistics, fused: y is not re-read); bdv_bn_train_finalize reduces them in fixed order.
 * affine (optional, excludes bn_partial): eval-mode BatchNorm folded into the epilogue,
 * y = relu?(conv * scale[c] + shift[c] (+ residual)) with scale/shift from bdv_bn_eval_params: the inference and
 * frozen-teacher forwards (UPSTREAM Recognizer2D._do_test, libs/cil/cil.py:520-522) then have no bn_apply pass. */
typedef struct bdv_conv_affine {
  const float* scale;    /* [Cout] */
  const float* shift;    /* [Cout] */
  const void* residual;  /* [N,Ho,Wo,Cout] or NULL (element type: the geometry's act_dtype) */
  int32_t relu;
} bdv_conv_affine;
int bdv_conv_fprop(const float* x, const float* w, float* y, const bdv_conv_geom* g, float* bn_partial,
                   const bdv_conv_affine* affine, void* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm-backward statistics fused into dgrad: dx (the gradient w.r.t. the BN(+ReLU) output of the PREVIOUS conv unit,
 * whose saved conv output is y) is reduced in the dgrad epilogue to partial[0][r][c] = sum(g), partial[1][r][c] =
 * sum(g * xhat) per row tile r (g = dx * mask, xhat = (y - mean) * invstd; stat_rows of the plan);
 * bdv_bn_backward(stat_partial = ...) then skips its own statistics pass.  Stride 2 needs a filter that
 * reaches every input pixel (R, S >= 2); the partial then has one block of rows per input-parity class and is zeroed by the call. */
typedef struct bdv_bn_stat_fuse {
  const void* y;             /* [N,H,W,Cin] conv output of the previous unit (element type: the geometry's act_dtype) */
  const uint32_t* relu_mask; /* 1 bit per element of dx, or NULL (no ReLU, or the sign is derived: relu_scale) */
  const float* mean;         /* [Cin] saved batch mean */
  const float* invstd;       /* [Cin] */
  float* partial;            /* float[2][stat_rows][Cin] */
  const float* relu_scale;   /* optional [Cin] pair with relu_mask == NULL: the unit's ReLU sign is y * relu_scale + relu_shift > 0 */
  const float* relu_shift;   /* (units whose activation and mask were never written: bdv_conv_fprop_pl(pre_scale)) */
} bdv_bn_stat_fuse;

/* dgrad: dx[N,H,W,Cin] = unshift(conv_transpose(dy, w)) + (add_src ? add_src * mask : 0),
 * mask = bit e of add_mask_src (the ReLU sign mask written by bdv_bn_apply) when add_mask_src != NULL
 * (fused ReLU-backward of the identity path).
 * Replaces autograd of F.conv2d w.r.t. its input and of TemporalShift.shift. */
int bdv_conv_dgrad(const float* dy, const float* w, float* dx, const float* add_src,
                   const uint32_t* add_mask_src, const bdv_conv_geom* g, const bdv_bn_stat_fuse* bn_stat, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Weights as bf16 planes for the default conv arithmetic (every fp32 product from three bf16 pieces per operand, six
 * v_mfma_f32_32x32x16_bf16 products, fp32 accumulate; replaces the same F.conv2d / autograd call sites as bdv_conv_fprop and
 * bdv_conv_dgrad).  bdv_conv_split_weights cuts w [Cout,R,S,Cin] once per optimizer step into hi / mid / lo planes
 * (hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid), round to nearest), each of
 * bdv_conv_weight_planes_bytes(g) / 3 bytes, in the two layouts the kernels stream:
 *   planes_fprop  [piece][K-step = (ci / 32) * R*S + tap][co][ci % 32]
 *   planes_dgrad  [piece][tap][co / 32][ci][co % 32]
 * (either may be NULL; Cin and Cout multiples of 32).  bdv_conv_fprop_pl / bdv_conv_dgrad_pl take the planes beside w and
 * behave like bdv_conv_fprop / bdv_conv_dgrad (same epilogues, workspace = bdv_conv_workspace_bytes).  They are THE bf16-piece
 * entry points: sites without a plane kernel (the stem, 64 columns behind a 1x1 filter) run the bf16-piece stem kernel resp. the
 * fp32-MFMA kernels on w, and for those (reads_planes = 0) the planes may be NULL -- what the former bdv_conv_*_x3 aliases ran.
 * pieces = 3 is the arithmetic described above.  pieces = 1 is the REDUCED-PRECISION arithmetic of BASELINE config 5 ("MFMA
 * fp16 tiles"; the reference's trainer is precision 32, libs/cil/cil.py:744-756, so there are no reference numerics for it):
 * each operand value is rounded to bf16 (only the hi plane is used), one v_mfma_f32_32x32x16_bf16 product per step, fp32
 * accumulate, fp32 tensors in HBM -- what torch.autocast(bfloat16) computes for a convolution, without the bf16 output rounding.
 * Error of a result: ~2^-9 relative per product, i.e. ~1e-3 .. 1e-2 of the output scale (tests/test_bf16x1_gpu.py).
 * pieces = 2 is the arithmetic in between ("bf16x2"): the hi and mid planes of each operand (16 significand bits) and the three
 * products hi*hi + hi*mid + mid*hi per step, fp32 accumulate, fp32 tensors; dropped terms <= 2^-15 relative per product (five more
 * bits than TF32, the conv arithmetic torch.backends.cudnn.allow_tf32 gives the reference on its GPUs); never the default, the
 * plane kernels only (other shapes run the pieces = 3 kernels), no bf16 storage (tests/test_bf16x2_gpu.py). */
size_t bdv_conv_weight_planes_bytes(const bdv_conv_geom* g);
int bdv_conv_split_weights(const float* w, const bdv_conv_geom* g, void* planes_fprop, void* planes_dgrad, void* stream);
/* Test / A-B hook, process-wide and not thread-safe: force the tile configuration of the two entry points below
 * (0 = 128x256, 1 = 256x128, 2 = 256x256, 3 = 256x64, 4 = 64x128 (dgrad, stride 1), 5 = 128x128 with four waves and two
 * workgroups per CU, where the tile divides the column count; 6 = none of them; -1 = the planner's rules). */
int bdv_conv_debug_force_tile(int cfg);
/* Test / A-B hook, process-wide and not thread-safe: on = 1 (the default) lets the 3x3 stride-1 sites of the 256x64 tile (fp32
 * tensors, two or three pieces) stage each activation run once per filter row and read the three taps from that one LDS image;
 * on = 0 routes the same kernel instantiation through the per-tap loader.  Both give the same output bits
 * (tests/test_conv_row_run_gpu.py). */
int bdv_conv_debug_row_run(int on);
/* pre_scale / pre_shift (optional, [Cin] each): x is then the RAW output of the producing conv and the producer's train-mode
 * BatchNorm + ReLU, a = max(x * pre_scale[ci] + pre_shift[ci], 0), is applied in the loader (the same fused multiply-add as
 * bdv_bn_apply, bit-identical activations; halo / ragged lanes stay zero): the apply pass between the two convs, the activation
 * tensor and its ReLU mask are not needed for this consumer (UPSTREAM ConvModule conv -> bn -> relu chains inside Bottleneck /
 * BasicBlock).  Needs pieces = 3, no temporal shift, and a plan with pre = 1 (pre_ok), which also gives the statistics rows. */
/* g->act_dtype = BDV_ACT_BF16: x, y and affine->residual are bf16 tensors (pieces = 1 only; the accumulators, the fused batch
 * statistics and the folded BatchNorm arithmetic stay fp32, y is rounded to nearest-even on store); same for dy / dx / add_src /
 * bn_stat->y of bdv_conv_dgrad_pl and dy / x of bdv_conv_wgrad_partial_pl (weight-gradient slabs stay fp32). */
int bdv_conv_fprop_pl(const void* x, const float* w, const void* planes_fprop, void* y, const bdv_conv_geom* g,
                      float* bn_partial, const bdv_conv_affine* affine, void* workspace, size_t workspace_bytes, int pieces,
                      const float* pre_scale, const float* pre_shift, void* stream);
int bdv_conv_dgrad_pl(const void* dy, const float* w, const void* planes_dgrad, void* dx, const void* add_src,
                      const uint32_t* add_mask_src, const bdv_conv_geom* g, const bdv_bn_stat_fuse* bn_stat, void* workspace,
                      size_t workspace_bytes, int pieces, void* stream);

/* "f16x2": fp32-level products from TWO fp16 pieces per operand and three MFMA products (arith code BDV_ARITH_F16X2 of
 * bdv_conv_plan_query).  Every operand tensor t has a device-resident amax word: the bits of an fp32 upper bound of max|t|
 * (bdv_f16x2_amax writes the maximum itself; nothing is read back to the host).  The kernels derive the scale
 *   S_t = 2^(14 - floor(log2 amax)), exponent clamped to [-113, 126]; S_t = 1 for amax = 0     (bdv_f16x2_scale on the host)
 * so that max|t| * S_t lies in [2^14, 2^15) -- at 2^15 the leading piece could round to infinity -- and form
 *   x = t * S_t,  hi = f16(x),  lo = f16(x - hi)   (round to nearest even; 11 + 11 significand bits and a sign),
 *   hi_a * hi_w + hi_a * lo_w + lo_a * hi_w per K-step on v_mfma_f32_32x32x16_f16, smallest first, fp32 accumulate,
 * and multiply the accumulators once by 1 / (S_a * S_w) (exponent clamped to the normal range) before the statistics rows, the
 * affine / residual epilogue, the dgrad scatter and the K-split partials: a power of two, so it commutes with the fp32 fix-up adds.
 * Error of a result: ~1e-7 of the output's scale, finer than an fp32 FMA chain.  Its one weakness: entries more than ~2^14 below
 * the tensor's maximum fall into fp16's subnormal range after scaling and lose bits relative to their own size (DESIGN.md
 * section 4).  Inf / NaN operands give Inf / NaN results.
 * Scope, as pieces = 2: the plane kernels (and the 128 x 128 four-wave tile where the three-piece rules pick the conv_*_x3 kernels),
 * fp32 tensors.  The stem, 64 GEMM columns behind a 1x1 filter and calls with pre_scale run the pieces = 3 kernels, bit-identical to
 * the *_pl entry points with pieces = 3 (the plan's kernel name says which: the fp16 kernels end in "F16Pieces>").
 * bdv_conv_split_weights_f16x2 takes the weight's maximum itself and writes hi / lo as planes 0 and 1 of the two layouts of
 * bdv_conv_split_weights (buffers of bdv_conv_weight_planes_bytes(g) each); the third plane's place starts with the amax word.
 * The planes of the two arithmetics cannot share a buffer.  x's amax serves fprop and wgrad, dy's dgrad and wgrad. */
#define BDV_ARITH_F16X2 4
int bdv_f16x2_amax(const float* t, int64_t n, void* amax, void* stream);   /* t 16-byte aligned, any n > 0; amax: 4 bytes */
float bdv_f16x2_scale(float amax);                                          /* host: S_t of a tensor with this maximum */
int bdv_conv_split_weights_f16x2(const float* w, const bdv_conv_geom* g, void* planes_fprop, void* planes_dgrad, void* stream);
int bdv_conv_fprop_f16x2(const void* x, const void* amax_x, const float* w, const void* planes_fprop, void* y,
                         const bdv_conv_geom* g, float* bn_partial, const bdv_conv_affine* affine, void* workspace,
                         size_t workspace_bytes, const float* pre_scale, const float* pre_shift, void* stream);
int bdv_conv_dgrad_f16x2(const void* dy, const void* amax_dy, const float* w, const void* planes_dgrad, void* dx,
                         const void* add_src, const uint32_t* add_mask_src, const bdv_conv_geom* g,
                         const bdv_bn_stat_fuse* bn_stat, void* workspace, size_t workspace_bytes, void* stream);
int bdv_conv_wgrad_partial_f16x2(const void* dy, const void* amax_dy, const void* x, const void* amax_x, const bdv_conv_geom* g,
                                 void* slab, size_t slab_bytes, const float* pre_scale, const float* pre_shift, void* stream);

/* wgrad: dw[Cout,R,S,Cin] = beta * dw + sum_pixels dy (x) shift(x).  Deterministic split-K:
 * partial slabs go to `workspace`, a second kernel reduces them in fixed order. */
int bdv_conv_wgrad(const float* dy, const float* x, float* dw, float beta, const bdv_conv_geom* g, void* workspace,
                   size_t workspace_bytes, void* stream);
/* The same weight gradient in two steps, so that the split-K reductions of several layers run as ONE launch (a ResNet
 * stage's backward issues one instead of up to 19): bdv_conv_wgrad_partial leaves the plan's `splits` partial
 * products of dw's size in `slab` (caller-owned, alive until reduced); bdv_wgrad_reduce_batched computes
 * dws[k] = beta * dws[k] + sum of the splits[k] slices of slabs[k] for n <= BDV_MAX_REDUCE_ITEMS items (HOST arrays;
 * numels[k] = elements of dws[k], a multiple of 4), with the per-element summation order of bdv_conv_wgrad. */
#define BDV_MAX_REDUCE_ITEMS 32
int bdv_conv_wgrad_partial(const float* dy, const float* x, const bdv_conv_geom* g, void* slab, size_t slab_bytes,
                           void* stream);
int bdv_wgrad_reduce_batched(const float* const* slabs, float* const* dws, const int* splits, const int64_t* numels, int n,
                             float beta, void* stream);
/* The weight gradient's main kernel of the bf16-piece arithmetic: 8 waves per workgroup, tiles of 128 / 256 output channels x
 * 128 / 256 input channels of one tap (4-wave forms for the 64-channel layers and the stem), both operand tiles split into bf16
 * pieces in the loader and read from LDS with ds_read_b64_tr_b16; geometries without such a tile run bdv_conv_wgrad_partial's
 * kernels.  The slab holds the plan's `splits` partial products of dw's size; reduce with bdv_wgrad_reduce_batched.
 * pre_scale / pre_shift as for bdv_conv_fprop_pl: x is the producer's raw conv output and the activation
 * max(x * pre_scale[ci] + pre_shift[ci], 0) is formed in the loader (a plan with pre = 1). */
int bdv_conv_wgrad_partial_pl(const void* dy, const void* x, const bdv_conv_geom* g, void* slab, size_t slab_bytes,
                              int pieces, const float* pre_scale, const float* pre_shift, void* stream);

/* ---- BatchNorm2d (train + eval), fused with ReLU / residual add --------------------------
 * Replaces UPSTREAM ConvModule.bn (+ .activate, + block `out + identity`) and their autograd.
 * y is [M][C] (M = N*Ho*Wo). */
size_t bdv_bn_workspace_bytes(int64_t M, int C);
/* train: batch mean / biased var -> scale = gamma*invstd, shift = beta - mean*scale; saves mean and
 * invstd; running_mean/var updated with `momentum` (unbiased var), num_batches_tracked handled by
 * the caller. */
int bdv_bn_train_stats(const float* y, int64_t M, int C, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var,
                       float* save_mean, float* save_invstd, float* scale, float* shift,
                       void* workspace, size_t workspace_bytes, void* stream);
/* same outputs as bdv_bn_train_stats, from the partial sums written by bdv_conv_fprop(bn_partial) */
int bdv_bn_train_finalize(const float* partial, int rows, int64_t M, int C, const float* gamma, const float* beta,
                          float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                          float* save_invstd, float* scale, float* shift, void* stream);
/* eval: scale/shift from running statistics. */
int bdv_bn_eval_params(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, void* stream);
/* out = act(y*scale[c] + shift[c] + r), act = ReLU if relu != 0; r = 0 without res, res itself, or -- with
 * res_scale/res_shift -- res*res_scale[c] + res_shift[c] (the block's downsample conv output gets its own BatchNorm
 * here instead of in a separate pass).  relu_mask (optional, needs C % 32 == 0): bit e of relu_mask[] = (out[e] > 0)
 * for flat element index e -- the 1-bit-per-element ReLU sign mask the backward kernels read instead of the fp32
 * activation. */
/* act_dtype (BDV_ACT_F32 | BDV_ACT_BF16): element type of y, res and out. */
int bdv_bn_apply(const void* y, const float* scale, const float* shift, const void* res, const float* res_scale,
                 const float* res_shift, void* out, uint32_t* relu_mask, int64_t M, int C, int relu, int act_dtype, void* stream);
/* backward of (BN-train -> +res -> ReLU): g = dout * (relu_mask bit if relu), dgamma = sum g*xhat,
 * dbeta = sum g, dy = gamma*invstd*(g - dbeta/M - xhat*dgamma/M).  dgamma/dbeta are written as
 * beta_acc*old + new.  The residual-path gradient is g itself; consumers re-derive it from
 * (dout, relu_mask) -- see bdv_conv_dgrad(add_src, add_mask_src) and bdv_relu_bwd. */
/* stat_partial (optional): float[2][stat_rows][C] written by bdv_conv_dgrad(bn_stat); the statistics pass is skipped. */
/* relu_scale / relu_shift (optional [C] pair, with relu != 0 and relu_mask == NULL): the ReLU sign is derived from y as
 * y * relu_scale + relu_shift > 0, the forward's own expression, for units whose mask was never written. */
/* act_dtype: element type of dout, y and dy (statistics, dgamma / dbeta and the coefficients stay fp32). */
int bdv_bn_backward(const void* dout, const uint32_t* relu_mask, const void* y, const float* gamma,
                    const float* save_mean, const float* save_invstd, void* dy, float* dgamma,
                    float* dbeta, float beta_acc, int64_t M, int C, int relu, const float* stat_partial, int stat_rows,
                    const float* relu_scale, const float* relu_shift, void* workspace, size_t workspace_bytes, int act_dtype,
                    void* stream);
/* ---- finalize on more CUs, same bits ------------------------------------------------------
 * The two finalize kernels (batch statistics; dgamma / dbeta / coefficients) sum a channel's partial rows in 256 row-lanes, 16
 * groups of 16 lanes, then the 16 group sums, in fp64 and fixed order.  The *_split entry points can run the lanes of a channel
 * group on `splits` blocks (1, 2, 4, 8 or 16; 0 = bdv_bn_finalize_splits(rows, C), or 1 when fin_scratch is NULL): every lane
 * does the same chain, each block publishes its group sums, and the last block to arrive (one ticket, nobody waits) adds the 16
 * group sums in index order -- the same additions, bit-identical outputs for every `splits`.  splits = 1 is the kernel behind
 * the entry points above and needs no scratch.
 * fin_scratch: bdv_bn_finalize_scratch_bytes(C) bytes (4096 bytes of ticket words, then 2 x 16 x C doubles; C <= 4096), 16-byte
 * aligned, ZERO-FILLED ONCE by the caller when allocated: the last arriver stores 0 back to its ticket, so no per-call memset is
 * needed.  The tickets' place does not depend on C: a buffer sized for the widest C serves every launch.  Launches that may
 * overlap (different streams) must not share a fin_scratch; launches of one stream may. */
size_t bdv_bn_finalize_scratch_bytes(int C);
int bdv_bn_finalize_splits(int rows, int C);
int bdv_bn_train_finalize_split(const float* partial, int rows, int64_t M, int C, const float* gamma, const float* beta,
                                float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                float* save_invstd, float* scale, float* shift, int splits, void* fin_scratch,
                                size_t fin_scratch_bytes, void* stream);
int bdv_bn_backward_split(const void* dout, const uint32_t* relu_mask, const void* y, const float* gamma,
                          const float* save_mean, const float* save_invstd, void* dy, float* dgamma,
                          float* dbeta, float beta_acc, int64_t M, int C, int relu, const float* stat_partial, int stat_rows,
                          const float* relu_scale, const float* relu_shift, void* workspace, size_t workspace_bytes, int act_dtype,
                          int splits, void* fin_scratch, size_t fin_scratch_bytes, void* stream);
/* Backward of the two BatchNorms that the masked gradient g = dout * relu_mask of a block with a downsample branch enters: `a` =
 * the block's last main unit, `b` = the downsample BatchNorm (UPSTREAM Bottleneck.forward `out = conv3(..) + downsample(x)`).
 * dout and the mask are read once per pass instead of once per BatchNorm; dya, dyb, dgamma_*, dbeta_* are bit-identical to two
 * bdv_bn_backward(relu = 1) calls.  stat_partial_a as bdv_bn_backward's stat_partial (then only b's statistics are taken here).
 * workspace = bdv_bn_pair_workspace_bytes(M, C); splits / fin_scratch as above. */
size_t bdv_bn_pair_workspace_bytes(int64_t M, int C);
int bdv_bn_backward_pair(const void* dout, const uint32_t* relu_mask, const void* ya, const float* gamma_a,
                         const float* mean_a, const float* invstd_a, const float* stat_partial_a, int stat_rows_a,
                         void* dya, float* dgamma_a, float* dbeta_a, const void* yb, const float* gamma_b,
                         const float* mean_b, const float* invstd_b, void* dyb, float* dgamma_b, float* dbeta_b,
                         int64_t M, int C, void* workspace, size_t workspace_bytes, int act_dtype, int splits,
                         void* fin_scratch, size_t fin_scratch_bytes, void* stream);
/* Backward through an EVAL-mode BatchNorm (+res -> ReLU): UPSTREAM ResNet(norm_eval=True) / ResNet._freeze_stages /
 * ResNetTSM(partial_bn=True) put BatchNorms into .eval() inside a training step; the reference then differentiates
 * F.batch_norm(training=False) through cuDNN.  With scale = gamma * invstd_running (bdv_bn_eval_params) the forward is
 * a = relu?(y*scale + shift (+res)), and
 *   dz = dout * sign,  dy = dz * scale,  dbeta = sum dz,  dgamma = sum dz * (y - running_mean) * invstd
 * -- one pass: dy does not depend on the sums.  Nothing is ever divided by gamma or scale (gamma = 0 and gamma < 0 are legal).
 * sign: relu_mask (the bits of bdv_bn_apply, C % 32 == 0), or relu_act (an activation tensor of the call's act_dtype: act > 0),
 * or neither (no ReLU); at most one of the two.
 * dz (optional): the masked gradient itself, for the identity path and the downsample BatchNorm of a block.
 * dgamma / dbeta (optional, each): when one is given the pass also reads y and leaves per-row-block partial sums that the
 * train-mode finalize reduces in fixed order in fp64 (run-to-run bit-identical; written as beta_acc*old + new); this needs y,
 * running_mean, invstd and workspace = bdv_bn_workspace_bytes(M, C); splits / fin_scratch as above.  When both are NULL, y,
 * running_mean, invstd, workspace and fin_scratch are not read: dy = dz * scale alone.
 * act_dtype: element type of dout, relu_act, y, dy and dz.  dy, dz, dout and y must be distinct buffers. */
int bdv_bn_eval_backward(const void* dout, const uint32_t* relu_mask, const void* relu_act, const void* y,
                         const float* scale, const float* running_mean, const float* invstd, void* dy, void* dz,
                         float* dgamma, float* dbeta, float beta_acc, int64_t M, int C, void* workspace,
                         size_t workspace_bytes, int act_dtype, int splits, void* fin_scratch, size_t fin_scratch_bytes,
                         void* stream);
/* g = dout * relu_mask (+ add) : masked gradient for an identity path that has no conv behind it */
int bdv_relu_bwd(const void* dout, const uint32_t* relu_mask, const void* add, void* g, int64_t numel, int act_dtype, void* stream);
/* out = a + b (gradient junctions) */
int bdv_add(const void* a, const void* b, void* out, int64_t numel, int act_dtype, void* stream);

/* ---- stem helpers ------------------------------------------------------------------------ */
/* (N,3,H,W) fp32 -> (N,H,W,4) fp32, 4th channel 0: boundary layout change for the NCHW batch
 * the reference hands over (libs/cil/cil.py:514-516). */
int bdv_nchw3_to_nhwc4(const float* x, float* out, int N, int H, int W, void* stream);
/* UPSTREAM ResNet.maxpool: MaxPool2d(3, stride 2, pad 1) on NHWC; idx holds the winning tap (0..8)
 * per output element (first maximum in scan order, as torch). */
/* out_dtype: element type of `out` (x is the fp32 stem activation): the pooled tensor is the first one stored in the activation
 * storage type.  bdv_maxpool_bwd: dout_dtype is the type of dout, dx is fp32. */
int bdv_maxpool_fwd(const float* x, void* out, uint8_t* idx, int N, int H, int W, int C, int out_dtype, void* stream);
int bdv_maxpool_bwd(const void* dout, const uint8_t* idx, float* dx, int N, int H, int W, int C, int dout_dtype, void* stream);
/* MaxPool3d((2,1,1), stride (2,1,1)) -- pool2 of UPSTREAM mmaction ResNet3d (I3D, configs/_base_/models/i3d_r50.py:1-27): the
 * element-wise larger of frames 2t and 2t+1 of x [2*frames_out][frame_elems] (frame_elems % 32 == 0; an even number of frames
 * per clip keeps pairs inside a clip).  sel: 1 bit per output element (second frame won); the backward fills dx completely. */
int bdv_maxpool_t2_fwd(const float* x, float* out, uint32_t* sel, int64_t frames_out, int64_t frame_elems, void* stream);
int bdv_maxpool_t2_bwd(const float* dout, const uint32_t* sel, float* dx, int64_t frames_out, int64_t frame_elems, void* stream);
/* The same pool2 on tensors of either storage type (act_dtype: BDV_ACT_F32 | BDV_ACT_BF16 = element type of x and out, resp.
 * dout and dx): I3D under bf16 storage, where layer1's output and layer2's input gradient are bf16 (UPSTREAM ResNet3d.forward,
 * `if i == 0 and self.with_pool2: x = self.pool2(x)`).  sel is the same word for word as for the same values in fp32; ties go to
 * the first frame; BDV_ACT_F32 is the two entry points above. */
int bdv_maxpool_t2_fwd_act(const void* x, void* out, uint32_t* sel, int64_t frames_out, int64_t frame_elems, int act_dtype,
                           void* stream);
int bdv_maxpool_t2_bwd_act(const void* dout, const uint32_t* sel, void* dx, int64_t frames_out, int64_t frame_elems, int act_dtype,
                           void* stream);
/* Stem tail of a training forward in one pass (UPSTREAM ConvModule norm+act, then ResNet.maxpool): a = relu(y * scale +
 * shift), out = maxpool(a), idx as bdv_maxpool_fwd, relu_mask = 1 bit per element of a (a > 0) as bdv_bn_apply writes it.
 * The activation a itself is not materialised. */
/* Backward of the same stem tail: BatchNorm(+ReLU) backward whose incoming gradient is the MaxPool2d(3,2,1) backward of
 * dpool [N,Ho,Wo,C]; that gradient is gathered on the fly in both passes (statistics, apply) and never materialised.
 * dy [N,H,W,C]; dgamma/dbeta as bdv_bn_backward; workspace = bdv_bn_workspace_bytes(N*H*W, C). */
/* The stem conv output y and its gradient dy are fp32 in every storage mode (the stem reads the fp32 NHWC4 frames); the pooled
 * tensor `out` and its gradient `dpool` carry the activation storage type (out_dtype / dpool_dtype). */
int bdv_bn_backward_maxpool(const void* dpool, const uint8_t* pool_idx, const uint32_t* relu_mask, const float* y,
                            const float* gamma, const float* save_mean, const float* save_invstd, float* dy, float* dgamma,
                            float* dbeta, float beta_acc, int N, int H, int W, int C, void* workspace,
                            size_t workspace_bytes, int dpool_dtype, void* stream);
/* bdv_bn_backward_maxpool with the finalize split (splits / fin_scratch: see bdv_bn_train_finalize_split) */
int bdv_bn_backward_maxpool_split(const void* dpool, const uint8_t* pool_idx, const uint32_t* relu_mask, const float* y,
                                  const float* gamma, const float* save_mean, const float* save_invstd, float* dy, float* dgamma,
                                  float* dbeta, float beta_acc, int N, int H, int W, int C, void* workspace,
                                  size_t workspace_bytes, int dpool_dtype, int splits, void* fin_scratch,
                                  size_t fin_scratch_bytes, void* stream);
int bdv_bn_relu_maxpool_fwd(const float* y, const float* scale, const float* shift, void* out, uint8_t* idx,
                            uint32_t* relu_mask, int N, int H, int W, int C, int out_dtype, void* stream);
/* UPSTREAM TSMHead.avg_pool = AdaptiveAvgPool2d(1): [N,HW,C] -> [N,C] */
/* act_dtype: element type of x / dx; the pooled features and their gradient are fp32. */
int bdv_avgpool_fwd(const void* x, float* out, int N, int HW, int C, int act_dtype, void* stream);
int bdv_avgpool_bwd(const float* dout, void* dx, int N, int HW, int C, int act_dtype, void* stream);

/* ---- fused background-mix / normalize front-end -------------------------------------------
 * libs/loader/comix_loader.py:72-75,138-145 + UPSTREAM Normalize (img_norm_cfg, config :121-122).
 * frames (B,T,H,W,3) uint8 RGB, bg (B,H,W,3) uint8 -- or fp32 pixel values in [0,255] when bg_f32 != 0 (the
 * output of bdv_bg_resize_crop_u8) --, mix (B) uint8 {0,1};
 * out_nhwc4 (B*T,H,W,4) and/or out_nchw (B,T,3,H,W) (either may be NULL).
 * frame: (x-mean)*inv_std ; bg: (x-mean)/std ; blend x*(1-alpha)+bg*alpha where mix[b] != 0. */
int bdv_bgmix_normalize_u8(const uint8_t* frames, const void* bg, int bg_f32, const uint8_t* mix, float alpha,
                           const float mean[3], const float std[3], const float inv_std[3],
                           float* out_nhwc4, float* out_nchw, int B, int T, int H, int W, void* stream);
/* The stages of BackgroundMixDataset.bg_pipeline before Normalize (libs/loader/comix_loader.py:72-73): torchvision
 * Resize(bg_resize) of the float image (smaller edge -> bg_resize; bilinear, align_corners=False, no antialias filter:
 * the same values as the antialiased form when the image is enlarged) and RandomCrop(bg_crop_size) at the offsets the
 * caller drew.  src: B uint8 RGB images (Hs,Ws,3) of one size; (Hr,Wr): the resized size; top / left: (B) int32 on the
 * device; out: (B,crop_h,crop_w,3) fp32 pixel values in [0,255] (not rounded, as the reference's float image). */
int bdv_bg_resize_crop_u8(const uint8_t* src, int B, int Hs, int Ws, int Hr, int Wr, const int32_t* top,
                          const int32_t* left, int crop_h, int crop_w, float* out, void* stream);
/* Test-time crops + normalize (val/test pipelines, configs/...bgmix_plus_randAug.py:140-171): CenterCrop / ThreeCrop /
 * TenCrop as emitted by the crop transforms (the reference's own libs/pipelines/five_crops.py:77-100 shows the offset
 * rule and the crop-major order; TenCrop adds the horizontally flipped copy of each crop right after it).
 * frames (B,T,H,W,3) uint8; crops = ncrops x (x_offset, y_offset, flip) HOST table, ncrops <= BDV_MAX_CROPS;
 * out_nhwc4 (B*ncrops*T, crop_h, crop_w, 4) and/or out_nchw (B, ncrops*T, 3, crop_h, crop_w): frame (b, k, t) is
 * frame t of sample b cropped by entry k, values (x-mean)*inv_std. */
#define BDV_MAX_CROPS 12
int bdv_crop_normalize_u8(const uint8_t* frames, const int32_t* crops, int ncrops, int crop_h, int crop_w,
                          const float mean[3], const float inv_std[3], float* out_nhwc4, float* out_nchw, int B, int T,
                          int H, int W, void* stream);
/* ActorCutMix composite (libs/loader/actor_cut_mix_loader.py:135-164 with libs/pipelines/box.py:176-207, :116-159,
 * :339-379): for every ActorCutMix clip of a batch, FlipWithBox + ResizeWithBox((Wd, Hd)) of the actor and of the scene
 * frames, BuildHumanMask from the actor's boxes, ActorCutOut(127) of the scene's own boxes, actor * mask + scene * (1 - mask)
 * and Normalize, in one launch.  actor (n_actor, T, Ha, Wa, 3) / scene (n_scene, T, Hs, Ws, 3) uint8: the clips after
 * Resize(-1, 256) (scene may be NULL when n_scene == 0).  plan: nclips*T frames, int32, on the device (read by the kernel) AND
 * on the host (every index validated before the launch), plan_len ints:
 *   nclips x (out_row, actor_row, actor_flip, scene_row, scene_flip)   scene_row = -1 only for a clip without actor boxes
 *   actor box offsets (nclips*T + 1), scene box offsets (nclips*T + 1)  frame f = clip * T + t; at most BDV_ACM_MAX_BOXES per frame
 *   actor boxes, then scene boxes: x0 y0 x1 y1 each, 0 <= x <= Wd, 0 <= y <= Hd (the .astype(int) of the final boxes; the pixels
 *   [y0, y1) x [x0, x1), an inverted box is empty)
 * A clip with no actor box in any frame is all actor (mask 1).  out (B_out, T, 3, Hd, Wd) fp32, 16-byte aligned: rows out_row of
 * the clips, values (x - mean) * inv_std; the other rows are not touched.  counts (nclips) int32: mask pixels per clip. */
#define BDV_ACM_MAX_BOXES 256
int bdv_actor_cut_mix_u8(const uint8_t* actor, int n_actor, int Ha, int Wa, const uint8_t* scene, int n_scene, int Hs, int Ws,
                         const int32_t* plan, const int32_t* plan_host, int64_t plan_len, int nclips, int T, int Hd, int Wd,
                         const float mean[3], const float inv_std[3], float* out, int B_out, int32_t* counts, void* stream);

/* ---- classifier heads ---------------------------------------------------------------------- */
/* libs/models/cil_heads/cosine_linear.py:27-43 (LSC): sim[n,k] = sum_p softmax_p(c)[p]*c[p],
 * c[p] = cos(x_n, w_{k,p}) with torch>=2 eps semantics (each norm clamped at 1e-8).
 * x (N,D), w (K,P*D), sim (N,K); xnorm (N), wnorm (K*P), cosbuf (N,K*P) are saved for backward. */
int bdv_lsc_fwd(const float* x, const float* w, float* sim, float* xnorm, float* wnorm, float* cosbuf,
                int N, int D, int K, int P, void* stream);
int bdv_lsc_bwd(const float* dsim, const float* x, const float* w, const float* xnorm, const float* wnorm,
                const float* cosbuf, float* dx, float* dw, float beta_w, float* dcos_ws,
                int N, int D, int K, int P, void* stream);
/* libs/models/cil_heads/inc_net.py:36-37 (IncrementalNet): out = x W^T + b */
int bdv_linear_fwd(const float* x, const float* w, const float* b, float* out, int N, int D, int K, void* stream);
int bdv_linear_bwd(const float* dout, const float* x, const float* w, float* dx, float* dw, float* db,
                   float beta_w, int N, int D, int K, void* stream);
/* UPSTREAM AvgConsensus(dim=1): (B*T,K) -> (B,K) mean over T, and its backward */
int bdv_consensus_fwd(const float* s, float* out, int B, int T, int K, void* stream);
int bdv_consensus_bwd(const float* dout, float* ds, int B, int T, int K, void* stream);
/* UPSTREAM TSMHead.dropout: mask from a counter-based hash of (seed, element index); same call
 * with the same seed reproduces the mask, so backward = forward applied to the gradient. */
int bdv_dropout(const float* x, float* out, int64_t numel, float p, uint64_t seed, void* stream);

/* ---- fused losses -------------------------------------------------------------------------- */
/* libs/losses/lsc_loss.py:30-58 (exclude_pos_denominator, optional hinge).  Writes loss (1),
 * dsim (B,K) and deta (1) for upstream gradient 1; callers scale.  `class_weights` (K) or NULL:
 * lsc_loss.py:50-51, the row's term is scaled by class_weights[target] before the negation and the hinge. */
int bdv_lsc_loss(const float* sim, const int64_t* targets, const float* eta, float margin, int hinge,
                 const float* class_weights, float* loss, float* dsim, float* deta, int B, int K, void* stream);
/* libs/cil/icarl.py:123-125 soft-target CE: loss = mean_b(-sum_k tgt*log_softmax(score)).
 * `soft_targets` (B,K) or NULL with integer `labels` (B) (= plain mean cross-entropy). */
int bdv_softce_loss(const float* score, const float* soft_targets, const int64_t* labels, float* loss,
                    float* dscore, int B, int K, void* stream);
/* icarl.py:101-120: targets = base_targets (the foreground-ratio soft labels of :103-111, built by bdv_acm_targets with
 * alpha = 4) or, when base_targets is NULL, onehot(label); rows with label < prev_K <- softmax(prev_logits). */
int bdv_icarl_targets(const int64_t* labels, const float* prev_logits, int prev_K, const float* base_targets,
                      float* targets, int B, int K, void* stream);
/* libs/losses/acm_smooth_ce.py:18-28 (ACMSmoothCE smooth labels): targets = onehot(label) * lam + (1 - lam) *
 * onehot(background_label), lam = 1 - (1 - foreground_ratio)^alpha; background label -1 counts as class 0. */
int bdv_acm_targets(const int64_t* labels, const int64_t* background_labels, const float* foreground_ratio, float alpha,
                    float* targets, int B, int K, void* stream);
/* UPSTREAM Recognizer2D average_clip('prob'): (B*n,K) -> softmax over K, mean over n -> (B,K) */
int bdv_softmax_mean(const float* s, float* out, int B, int n, int K, int apply_softmax, void* stream);
/* UPSTREAM top_k_accuracy: acc[0]=top-1, acc[1]=top-5 hit rates, computed on device (no D2H sync) */
int bdv_topk_acc(const float* score, const int64_t* labels, float* acc, int B, int K, void* stream);
/* libs/cil/cil.py:519-541 feature distillation: mse = mean((cur-prev)^2); dcur = gscale*2*(cur-prev)/numel */
size_t bdv_reduce_workspace_bytes(void);
/* act_dtype: element type of cur / prev / dcur (the hooked stage outputs carry the activation storage type; the avg_pool
 * features are fp32 in every mode). */
int bdv_kd_mse_fwd(const void* cur, const void* prev, float* mse, int64_t numel, void* workspace,
                   size_t workspace_bytes, int act_dtype, void* stream);
int bdv_kd_mse_bwd(const void* cur, const void* prev, const float* gscale_dev, float gscale_host,
                   void* dcur, int64_t numel, int act_dtype, void* stream);

/* ---- pooled-output distillation (csrc/pod_kd.hip) ---------------------------------------------
 * UPSTREAM, unpinned: PODNet (Douillard et al., "PODNet: Pooled Outputs Distillation for Small-Tasks Incremental Learning",
 * ECCV 2020), its pod(collapse_channels='spatial', normalize=True) and embeddings_similarity restated from the paper; the
 * reference has no such loss.  Each entry point stands in for the nn.MSELoss of libs/cil/cil.py:519-541, per hooked module.
 * Tensors are NHWC (N, H, W, C) in the activation storage type act_dtype; C % 4 == 0, H <= 64, W <= 64, N <= 65535. */
/* libs/cil/cil.py:519-541 (site), PODNet POD-spatial: bytes of workspace for bdv_pod_spatial_fwd(N, C, H, W); bdv_pod_flat(N, D)
 * takes bdv_pod_workspace_bytes(N, D, 1, 1).  0 for a non-positive size. */
size_t bdv_pod_workspace_bytes(int N, int C, int H, int W);
/* libs/cil/cil.py:519-541 (site), PODNet POD-spatial: p_n = concat(sum_w cur^2 (H, C), sum_h cur^2 (W, C)), q_n from
 * prev, loss = mean_n | p_n / max(|p_n|, 1e-12) - q_n / max(|q_n|, 1e-12) |.  Writes loss[0] and the profile gradient
 * G (N, H+W, C) fp32 = d loss / d p, which is all bdv_pod_spatial_bwd needs besides cur. */
int bdv_pod_spatial_fwd(const void* cur, const void* prev, float* loss, float* G, int N, int C, int H, int W, void* workspace,
                        size_t workspace_bytes, int act_dtype, void* stream);
/* libs/cil/cil.py:519-541 (site), PODNet POD-spatial: dcur[n,h,w,c] = gscale_dev[0] * 2 * cur * (G[n,h,c] + G[n,H+w,c]); prev is not read. */
int bdv_pod_spatial_bwd(const void* cur, const float* G, const float* gscale_dev, void* dcur, int N, int C, int H, int W,
                        int act_dtype, void* stream);
/* libs/cil/cil.py:519-541 (site), PODNet POD-flat, F.cosine_embedding_loss with target 1 on (N, D) rows:
 * loss = mean_n (1 - cur.prev / sqrt((|cur|^2 + 1e-12)(|prev|^2 + 1e-12))); dcur_unit (N, D) fp32 = d loss / d cur. */
int bdv_pod_flat(const void* cur, const void* prev, float* loss, float* dcur_unit, int N, int D, void* workspace,
                 size_t workspace_bytes, int act_dtype, void* stream);

/* ---- time-channel importance distillation (csrc/tc_kd.hip) ------------------------------------
 * UPSTREAM, unpinned: TCD (Park, Kang, Han, "Class-Incremental Learning for Action Recognition in Videos", ICCV 2021), the
 * importance-weighted feature distillation and its gradient-based estimator as DESIGN 4.12 defines them; the reference has no
 * such code.  Tensors are NHWC (N, H, W, C), N = B * T frames with row n = b * T + t; importance and S are (T, C) fp32.
 * C % 4 == 0, N % T == 0, H * W * C / 4 <= 2^30, N / T * H * W <= 2^30. */
/* libs/cil/cil.py:519-541 (site): bytes of workspace for bdv_kd_tc_fwd and bdv_tc_sqgrad_accum at these sizes (the larger of the
 * forward's per-block partials and the accumulator's fp64 (T, C) slabs).  0 for a size either would refuse. */
size_t bdv_kd_tc_workspace_bytes(int N, int T, int C, int H, int W);
/* libs/cil/cil.py:519-541 (site), the nn.MSELoss weighted per (segment, channel):
 * loss = 1 / (N C H W) * sum importance[n mod T, c] * (cur - prev)^2.  importance == 1 is bdv_kd_mse_fwd's value (another
 * summation order).  act_dtype: element type of cur / prev. */
int bdv_kd_tc_fwd(const void* cur, const void* prev, const float* importance, float* loss, int N, int T, int C, int H, int W,
                  void* workspace, size_t workspace_bytes, int act_dtype, void* stream);
/* libs/cil/cil.py:519-541 (site): dcur = gscale_dev[0] * 2 / (N C H W) * importance[n mod T, c] * (cur - prev), in the element
 * type of cur; importance == 1 gives bdv_kd_mse_bwd's bits. */
int bdv_kd_tc_bwd(const void* cur, const void* prev, const float* importance, const float* gscale_dev, void* dcur, int N, int T,
                  int C, int H, int W, int act_dtype, void* stream);
/* libs/cil/cil.py:519-541 (site), the estimator of the importance map: S[t, c] += scale^2 * sum_{b,h,w} grad[b*T+t, h, w, c]^2
 * for an fp32 gradient at a hooked module; two stages, a fixed summation order, squares and sums in fp64 (S is rounded once
 * per call).  Calling it again adds to S. */
int bdv_tc_sqgrad_accum(const float* grad, float* S, float scale, int N, int T, int C, int H, int W, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- representation path: clip representations, NME classifier, class means, herding --------- */
/* libs/cil/cil.py:501-506 (_extract_repr) + :564-571 (predict_step, extract_repr): feat = the hooked
 * cls_head.avg_pool output flattened to (B*crops*T, D); repr (B*crops, D) = F.normalize(mean over the T segments);
 * mean_crops (B, D) = mean over crops of repr. */
int bdv_repr_from_features(const float* feat, float* repr, float* mean_crops, int B, int crops, int T, int D,
                           void* stream);
/* libs/cil/cil.py:945-960 (NME): similarity (S,K) = mean over crops of F.cosine_similarity(repr, class_means)
 * (each norm clamped at 1e-8), pred (S) = first arg-max over K.  repr (S*crops, D), class_means (K, D). */
size_t bdv_nme_workspace_bytes(int K, int D);
int bdv_nme_classify(const float* repr, const float* class_means, float* similarity, int64_t* pred, int S,
                     int crops, int D, int K, void* workspace, size_t workspace_bytes, void* stream);
/* libs/cil/cil.py:1079-1083: means[k] = mean of the rows of repr (n, D) whose label is k (NaN for an empty class,
 * like torch.mean of an empty selection). */
int bdv_class_means(const float* repr, const int64_t* labels, float* means, int n, int D, int K, void* stream);
/* libs/cil/memory_selection.py:70-92 + :150-164 (Herding, one class): greedy selection of num_exemplars rows of
 * features (n, D) whose running mean stays closest to the class mean (cosine: 1 - cos, else pairwise L2 distance with
 * torch's 1e-6).  class_mean (D) is what calc_mean_features returns; indices are positions in `features` in
 * selection order (ties -> lowest index, like argmin on the shrinking tensor); dist are the winning distances. */
size_t bdv_herding_workspace_bytes(int n, int D);
int bdv_herding_select(const float* features, int n, int D, int num_exemplars, int cosine_distance,
                       float* class_mean, int64_t* indices, float* dist, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- data path: RandAugment on uint8 frames ---------------------
 * libs/pipelines/rand_augment.py:17-160 as applied by RandAugment._rand_aug (:237-264): ONE operation per clip (the
 * same for each of its T frames), bit-identical to the Pillow routines the reference calls.  in / out: (B, T, H, W, 3)
 * uint8 RGB, distinct buffers.  op_i (B, 8) int32 and op_d (B, 4) float64 are device tables, one row per clip:
 *   op_i[0] = operation: 0 Identity | 1 AutoContrast | 2 Equalize | 3 Solarize (op_d[0] = threshold) |
 *             4 Posterize (op_i[1] = bits) | 5 Color | 6 Contrast | 7 Brightness | 8 Sharpness (op_d[0] = factor in [0,1]) |
 *             9 affine, nearest, 16.16 fixed point: ShearX / ShearY / Rotate (op_i[1..6] = FIX(a0) FIX(a1)
 *               FIX(a2 + a0/2 + a1/2) FIX(a3) FIX(a4) FIX(a5 + a3/2 + a4/2), FIX(v) = floor(v * 65536 + 0.5)) |
 *            10 affine without cross terms: TranslateX / TranslateY (op_d[0..3] = a0 a2 a4 a5) |
 *            11 CutoutAbs (op_i[1..4] = x0 y0 x1 y1, inclusive)
 *   op_i[7] = fill colour 0xRRGGBB for operations 9-11 (FILL_COLOR (124,116,104), rand_augment.py:15).
 * Three launches per call (histograms, per-frame tables, apply); call once per operation slot (n = 2 in every config). */
size_t bdv_randaug_workspace_bytes(int B, int T, int H, int W);
int bdv_randaug_apply(const uint8_t* in, uint8_t* out, const int32_t* op_i, const double* op_d, int B, int T, int H,
                      int W, void* workspace, size_t workspace_bytes, void* stream);

/* Resize / MultiScaleCrop + Resize of the frame pipeline (configs/ucf101/bgmix_plus_randAug/...py:127-136; UPSTREAM mmaction2
 * Resize -> mmcv.imresize('bilinear') -> cv2.resize(INTER_LINEAR) on uint8 images): OpenCV's published fixed-point arithmetic
 * (11-bit weights, horizontal then vertical pass, the 2x2 box mean for an exact 2x shrink), PARITY UNPINNED -- cv2 is in neither
 * the reference tree nor this image (oracle/resize_oracle.py).  src (N,Hs,Ws,3) uint8 -> dst (N,Hd,Wd,3) uint8.  boxes: NULL (the
 * whole frame) or one (x0, y0, w, h) int32 quadruple per group of frames_per_box consecutive frames (a clip shares its crop), given
 * on the device (read by the kernel) AND on the host (validated against the frame before the launch). */
int bdv_resize_linear_u8(const uint8_t* src, int N, int Hs, int Ws, const int32_t* boxes, int frames_per_box,
                         const int32_t* boxes_host, uint8_t* dst, int Hd, int Wd, void* stream);

/* The same stages for a batch whose clips differ in size (configs/HMDB51/bgmix_seed_1000_inc_5_stages_bgmix_plus_randAug.py:125
 * Resize(-1, 256), :128-134 MultiScaleCrop + Resize(224, 224), :143-144 / :175-176 Resize + CenterCrop, :159-162 Resize + TenCrop;
 * configs/sth-sthv2/seed_1000_inc_9_stages_bgmix_plus_randAug.py:131, :134-140, :149-150, :166-167, :182-183; the reference runs
 * them per sample in its DataLoader workers, so a batch never holds two sizes there).  The clips lie in one packed byte buffer, T consecutive (H, W, 3) uint8 frames each.
 * bdv_resize_linear_ragged_u8: one launch for the whole batch, per output pixel exactly bdv_resize_linear_u8.  table: nclips rows of
 * BDV_RAGGED_RESIZE_COLS int64 -- source byte offset, Hs, Ws, box x0, y0, w, h (the whole frame: 0, 0, Ws, Hs), destination byte
 * offset, Hd, Wd -- on the device (read by the kernel) AND on the host, where every row is validated before the launch: the box inside
 * its frame, both byte ranges inside their buffers (src_bytes, dst_bytes), the destination ranges of different clips disjoint, clip
 * starts 16-byte aligned (frames inside a clip need not be).  The destination is a second packed buffer (Resize: Hd, Wd differ per
 * clip) or the uniform (nclips, T, S, S, 3) tensor (destination offsets clip * T * S * S * 3). */
#define BDV_RAGGED_RESIZE_COLS 10
int bdv_resize_linear_ragged_u8(const uint8_t* src, int64_t src_bytes, const int64_t* table, const int64_t* table_host, int nclips,
                                int T, uint8_t* dst, int64_t dst_bytes, void* stream);
/* bdv_crop_normalize_u8 over such a buffer: clips = B rows (byte offset, H, W) int64, crops = (B, ncrops, (x_offset, y_offset, flip))
 * int32 -- the offsets of CenterCrop / ThreeCrop / FiveCrop / TenCrop depend on each clip's size -- both on the device AND on the host
 * (byte ranges and crops validated before the launch).  Outputs as bdv_crop_normalize_u8: out_nhwc4 (B*ncrops*T, crop_h, crop_w, 4)
 * and/or out_nchw (B, ncrops*T, 3, crop_h, crop_w), crop-major, values (x-mean)*inv_std. */
int bdv_crop_normalize_ragged_u8(const uint8_t* src, int64_t src_bytes, const int64_t* clips, const int64_t* clips_host,
                                 const int32_t* crops, const int32_t* crops_host, int ncrops, int crop_h, int crop_w,
                                 const float mean[3], const float inv_std[3], float* out_nhwc4, float* out_nchw, int B, int T,
                                 void* stream);

/* ---- JPEG frame decode ----------------------------------------------
 * The first stage of every pipeline of the configs: RawFrameDecode (configs/ucf101/bgmix_plus_randAug/
 * bgmix_seed_1000_inc_10_stages_bgmix_plus_randAug.py:126, :144, :160; UPSTREAM mmaction2 RawFrameDecode ->
 * mmcv.imfrombytes(channel_order='rgb') -> cv2.imdecode), i.e. libjpeg(-turbo) with its default ISLOW inverse DCT, fancy
 * chroma upsampling and fixed-point YCbCr -> RGB: reproduced bit for bit (oracle/jpeg_oracle.py, pinned by Pillow's
 * libjpeg-turbo).  Baseline / extended-sequential Huffman streams, 8-bit, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, restart
 * intervals, interleaved or per-component scans; anything else returns BDV_EINVAL with the reason in bdv_last_error().
 *   1. bdv_jpeg_parse          (host) header -> bdv_jpeg_info: sizes, sampling, block grids, the components' quantisation tables
 *   2. bdv_jpeg_entropy_decode (host, thread-safe: call it from one thread per image) Huffman-decodes the stream into
 *      QUANTISED coefficients, info->coef_count shorts: per component a raster of 64-short blocks in natural (row-major)
 *      order over the MCU-padded block grid, component c at coef_offset[c]
 *   3. bdv_jpeg_reconstruct_u8 (device) a batch of B images of ONE geometry (everything in `info` but the tables): coefs
 *      (B, coef_count) int16 and qts (B, 3, 64) uint16 on the device -> rgb (B, height, width, 3) uint8; workspace =
 *      bdv_jpeg_workspace_bytes(info, B) bytes (the component planes).  Two launches: dequantise + inverse DCT, then
 *      upsample + colour conversion. */
typedef struct {
  int32_t width, height, ncomp;          /* ncomp: 1 (grey, written to all three output channels) or 3 (YCbCr) */
  int32_t h[3], v[3];                    /* sampling factors */
  int32_t blocks_w[3], blocks_h[3];      /* block grid of each component, padded to whole MCUs */
  int32_t down_w[3], down_h[3];          /* real sample size of each component: ceil(width * h / hmax), ceil(height * v / vmax) */
  uint16_t qt[3][64];                    /* each component's quantisation table, natural order */
  int64_t coef_offset[3], coef_count;    /* in shorts, inside one image's coefficient buffer */
} bdv_jpeg_info;
int bdv_jpeg_parse(const unsigned char* data, size_t n, bdv_jpeg_info* info);
int bdv_jpeg_entropy_decode(const unsigned char* data, size_t n, const bdv_jpeg_info* info, short* coefs);
/* Step 2 for n streams of ONE geometry on `threads` host threads (std::thread; the caller's thread is one of them): coefs
 * (n, coef_count) int16 and qts (n, 3, 64) uint16 are HOST buffers (pinned, for the upload); returns the first failing image's
 * error.  What decode.JpegDecoder calls per batch. */
int bdv_jpeg_entropy_decode_batch(const unsigned char* const* data, const size_t* sizes, int n, const bdv_jpeg_info* info,
                                  short* coefs, unsigned short* qts, int threads);
size_t bdv_jpeg_workspace_bytes(const bdv_jpeg_info* info, int B);
int bdv_jpeg_reconstruct_u8(const short* coefs, const unsigned short* qts, const bdv_jpeg_info* info, int B, void* workspace,
                            size_t workspace_bytes, unsigned char* rgb, void* stream);

/* ---- background extraction --------------------------------------------
 * BackgroundMixDataset.__init__ with extract_bg_if_not_found=True (libs/loader/comix_loader.py:60-100) makes every missing
 * bg_dir/<video>.jpg with bg_extraction_tmf (:148-164): the per-pixel np.median of the video's frames, .astype(np.uint8),
 * written by cv2.imwrite -- a baseline JPEG with libjpeg-turbo's defaults (quality 95, 4:2:0, ISLOW DCT, standard Huffman tables).
 *
 * bdv_temporal_median_u8 (device): V videos of one frame geometry; frames (total_frames, H, W, 3) uint8 holds their frames back
 * to back, video v at frames first[v] .. first[v] + counts[v] - 1 (first int64, counts int32: device arrays, and the same values on
 * the host in first_host / counts_host, checked against total_frames before the launch; 1..65535 frames per video).
 * out (V, H, W, 3) uint8 = np.median(frames of v, axis=0).astype(uint8): the middle order statistic for an odd count, the floor
 * of the mean of the two middle ones for an even count.  One launch; the frame stack is read twice. */
int bdv_temporal_median_u8(const uint8_t* frames, int64_t total_frames, const int64_t* first, const int32_t* counts,
                           const int64_t* first_host, const int32_t* counts_host, int V, int H, int W, uint8_t* out, void* stream);
/* Person-masked backgrounds: the reference filters extracted backgrounds with a Mask-RCNN person detector and keeps those in which
 * no person is left (cil_tools/type_b_and_c_bg.py:47-54), because the temporal median of bg_extraction_tmf
 * (libs/loader/comix_loader.py:148-164) keeps a person who covers a pixel in half or more of the frames.  The substitute here
 * needs no detector: the median over the frames in which the pixel lies outside every person box of the ActorCutMix detection
 * file, and the number of such frames per pixel.
 *
 * bdv_temporal_masked_median_u8 (device): frames / first / counts / V / H / W as for bdv_temporal_median_u8.  The boxes are a CSR
 * table over the batch's frames: box_first (total_frames + 1) int32, boxes (num_boxes, 4) int32 rows x0, y0, x1, y1, half-open
 * (pixel (x, y) is covered when x0 <= x < x1 and y0 <= y < y1, as mask[y0:y1, x0:x1] of BuildHumanMask); frame f of the batch owns
 * rows box_first[f] .. box_first[f + 1] - 1.  Both are device arrays (boxes 16-byte aligned) with the same values on the host in
 * box_first_host / boxes_host, checked before the launch: box_first monotone within 0..num_boxes, 0 <= x0 <= x1 <= W,
 * 0 <= y0 <= y1 <= H.  num_boxes may be 0 (boxes then unused).  min_visible >= 1.
 * visible (V, H, W) uint16 = the number of the video's frames none of whose boxes covers the pixel.  out (V, H, W, 3) uint8: where
 * visible >= min_visible, np.median over those frames, .astype(uint8) (the middle value for an odd count, the floor of the mean of
 * the two middle ones for an even count); elsewhere (a hole) np.median over ALL the video's frames, bdv_temporal_median_u8's value.
 * With no boxes out is bdv_temporal_median_u8's, byte for byte, and visible the frame count.  One launch; the stack is read twice,
 * and twice more by the waves that own a hole. */
int bdv_temporal_masked_median_u8(const uint8_t* frames, int64_t total_frames, const int64_t* first, const int32_t* counts,
                                  const int64_t* first_host, const int32_t* counts_host, int V, int H, int W,
                                  const int32_t* box_first, const int32_t* boxes, const int32_t* box_first_host,
                                  const int32_t* boxes_host, int64_t num_boxes, int min_visible, uint8_t* out, uint16_t* visible,
                                  void* stream);
/* Simulated-camera-motion backgrounds: sim_cam_motion_bg_extract (cil_tools/extract_background.py:78-99) passes every frame, as
 * a float image, through torchvision's RandomResizedCrop(size=100), sets exact zeros to NaN and takes np.nanmedian / np.nanmean
 * over time, .astype(np.uint8).
 *
 * bdv_resized_crop_f32 (device): frames (F, H, W, 3) uint8; boxes (F, 4) int32 [top, left, h, w] on the device and the same values
 * on the host in boxes_host (every box is checked against the frame before the launch).  out (F, out_h, out_w, 3) fp32 = the box
 * of each frame resized as torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=antialias) resizes the
 * float crop on the CPU: antialias 0 = ATen's 2 x 2 bilinear (source index (dst + 0.5) * scale - 0.5, clamped at 0), 1 = its
 * separable triangle filter (support widened by the scale when reducing, weights normalised to sum 1, horizontal pass first).
 * Scales h / out_h and w / out_w are independent; no fused multiply-add.  A pixel whose source pixels are all 0 is exactly 0.0f. */
int bdv_resized_crop_f32(const uint8_t* frames, int F, int H, int W, const int32_t* boxes, const int32_t* boxes_host, int out_h,
                         int out_w, int antialias, float* out, void* stream);
/* bdv_temporal_nanreduce_f32 (device): V stacks of fp32 frames of P elements each, laid out and described as for
 * bdv_temporal_median_u8 (first / counts on the device and on the host; 1..65535 frames per video).  An element is missing when it
 * is NaN, or when it is 0 and zero_is_missing is set.  out (V, P) uint8, per position over the n present values: mode 0 = the
 * median (the middle one for odd n, (a + b) * 0.5f of the two middle ones for even n), mode 1 = the mean (fp32 sum in frame order,
 * divided by n); the float is truncated to uint8 and saturated to 0..255; n = 0 gives 0.  Exactly np.nanmedian / np.nanmean
 * (axis 0, float32) followed by .astype(np.uint8).  One launch; the median reads the stack eight times (a radix select on the
 * floats' bits, most significant nibble first), the mean once. */
int bdv_temporal_nanreduce_f32(const float* frames, int64_t total_frames, const int64_t* first, const int32_t* counts,
                               const int64_t* first_host, const int32_t* counts_host, int V, int64_t P, int mode, int zero_is_missing,
                               uint8_t* out, void* stream);
/* The encoder's side of the bdv_jpeg_info struct, on the host: geometry of a YCbCr 4:2:0 stream of width x height (the layout
 * bdv_jpeg_entropy_decode produces) and the quantisation tables of jpeg_set_quality(quality) (tables 0 / 1 for Y / CbCr).
 * quality 25..100 (no entry exceeds 255 there, so force_baseline cannot matter); else BDV_EINVAL. */
int bdv_jpeg_encode_info(int width, int height, int quality, bdv_jpeg_info* info);
/* cv2.imwrite's forward stage (device): rgb (B, height, width, 3) uint8 -> coefs (B, coef_count) int16, quantised, per
 * component a raster of 64-short blocks in natural order over the MCU-padded grid, exactly what bdv_jpeg_entropy_decode returns
 * for libjpeg-turbo's file: fixed-point RGB -> YCbCr (jccolor.c), edge replication, h2v2 downsampling (jcsample.c), ISLOW forward
 * DCT (jfdctint.c), quantisation on divisors qt << 3 (jcdctmgr.c), dummy blocks as jccoefct.c makes them.  coefs 16-byte aligned. */
int bdv_jpeg_forward_u8(const uint8_t* rgb, int B, int height, int width, int quality, short* coefs, void* stream);
/* Host side of cv2.imwrite: coefs (HOST, coef_count int16 as above) -> the whole file (SOI, APP0 JFIF 1.01, DQT 0, DQT 1, SOF0,
 * DHT DC0 / AC0 / DC1 / AC1 with the standard tables, SOS, entropy-coded data, EOI) into out[0 .. capacity); *size = its length
 * (also when capacity is too small, which returns BDV_EINVAL).  Thread-safe.  bdv_jpeg_encode_bound(width, height) bytes always
 * suffice.  The _batch form encodes n images of one size on `threads` std::thread workers (the caller's thread is one of them):
 * image i from coefs + i * coef_count into out + i * stride, its length in sizes[i]. */
size_t bdv_jpeg_encode_bound(int width, int height);
int bdv_jpeg_entropy_encode(const short* coefs, int width, int height, int quality, unsigned char* out, size_t capacity, size_t* size);
int bdv_jpeg_entropy_encode_batch(const short* coefs, int n, int width, int height, int quality, unsigned char* out, size_t stride,
                                  size_t* sizes, int threads);

/* ---- Grad-CAM ----------------------------------------------------------
 * UPSTREAM mmaction2 GradCAM (mmaction/utils/gradcam_utils.py, _calculate_localization_map and __call__, for a 2D recognizer);
 * the reference repository has no counterpart and mmaction2 is not vendored: restated from memory, PARITY UNPINNED.  All tensors
 * fp32; no float atomics, every result is bit-identical from run to run.
 *
 * bdv_gradcam_map (device): act (N, HW, C) -- the tapped activation in NHWC storage -- and wgt (N, C), the spatial mean of the
 * gradient (bdv_avgpool_fwd on it) -> map (N, HW) = max(0, sum_c wgt[n, c] * act[n, p, c]).  C % 4 == 0, act and wgt 16-byte
 * aligned.  One wave per pixel: fmaf in channel order inside a lane (channels 4l .. 4l+3, 4(l+64) .., ...), then a fixed butterfly
 * over the 64 lanes.  -0 and NaN sums are written as +0. */
int bdv_gradcam_map(const float* act, const float* wgt, float* map, int N, int HW, int C, void* stream);
/* bdv_gradcam_minmax (device): map (B*T, h, w), non-negative -> minmax (2, B): row 0 the minimum, row 1 the maximum over all T*H*W
 * values of clip b's map after each frame is upsampled to (H, W) as torch.nn.functional.interpolate(mode='bilinear',
 * align_corners=False) does (UPSTREAM normalises after the interpolation, per sample and not per frame; the temporal interpolation
 * is the identity).  Indices and fractions as bdv_bg_resize_crop_u8: source index (dst + 0.5) * (in / out) - 0.5 clamped at 0, second
 * tap clamped to the edge (the coordinate in fp64, its fraction rounded to fp32), columns before rows, no fused multiply-add; two taps a, b with fraction l give a + l * (b - a),
 * which is exactly a on a constant map.  The upsampled map is not stored.  B <= 65535. */
int bdv_gradcam_minmax(const float* map, int B, int T, int h, int w, int H, int W, float* minmax, void* stream);
/* bdv_gradcam_render (device): recomputes the upsampled value u of every output pixel (the same bits as bdv_gradcam_minmax saw) and
 * writes whichever outputs are given:
 *   v_out (B, T, H, W) = (u - min_b) / (max_b - min_b + 1e-20f) (UPSTREAM's delta; an all-zero or constant clip gives zeros);
 *   overlay (B, T, H, W, 3) uint8 = rint(255 * clamp(alpha * lut[idx] + (1 - alpha) * img01, 0, 1)), idx = min(255, floor(256 * v))
 *     (matplotlib's colormap lookup), lut (256, 3) in [0, 1], img01 = (x * std + mean) / 255 with x = frames_nhwc4 (B*T, H, W, 4), the
 *     model's normalised input (16-byte aligned); 0 <= alpha <= 1;
 *   sums (B, 2) = (sum of v, sum of v over the pixels whose centre (x + 0.5, y + 0.5) lies in the union of that frame's boxes:
 *     x0 <= x + 0.5 < x1 and y0 <= y + 0.5 < y1), accumulated in fp64 in a fixed order (per output row, then one block per clip) and
 *     rounded once.  Boxes: box_off (B*T + 1) int32 offsets per frame and boxes (nbox, 4) fp32 rows x0 y0 x1 y1 in output-pixel
 *     coordinates (any finite values: a box may leave the frame or be empty), on the device AND on the host, where the offsets
 *     (start at 0, do not decrease, end at nbox) and the rows (no NaN) are checked before the launch.  workspace: at least
 *     bdv_gradcam_workspace_bytes(B, T, H) bytes, 8-byte aligned; needed for sums only. */
size_t bdv_gradcam_workspace_bytes(int B, int T, int H);
int bdv_gradcam_render(const float* map, const float* minmax, int B, int T, int h, int w, int H, int W, float* v_out,
                       const float* frames_nhwc4, const float* lut, float alpha, const float mean[3], const float std[3],
                       uint8_t* overlay, const int32_t* box_off, const int32_t* box_off_host, const float* boxes,
                       const float* boxes_host, int nbox, float* sums, void* workspace, size_t workspace_bytes, void* stream);

/* ---- clip blending: train_cfg.blending (Mixup / CutMix) and VideoMix ---------------------------------------------------------
 * A sample is one contiguous blob of outer x H x W x inner floats, the pixel grid in the middle: (B, T, 3, H, W) has outer = T * 3,
 * inner = 1; the NHWC4 frames (B * T, H, W, 4) have outer = T, inner = 4; the 3-D recognizer's (B, clips, 3, T, H, W) has outer =
 * clips * 3 * T, inner = 1.  perm: device int64 (B), every entry in [0, B) (the caller checks its host copy before the upload).
 * Sample bases and box rows need only 4-byte alignment: 16-byte accesses are used where an address allows them.
 *
 * UPSTREAM mmaction/datasets/blending_utils.py MixupBlending.do_blending (`lam * imgs + (1 - lam) * imgs[rand_index, :]`; reached
 * from configs/recognition/tsm/tsm_r50_mixup_1x1x8_50e_sthv1_rgb.py:24-25): out[b] = lam * x[b] + (1 - lam) * x[perm[b]], 1 - lam
 * formed in fp32, both products and the sum rounded to fp32 (no fused multiply-add): torch's expression bit for bit.  out must not
 * overlap x. */
int bdv_blend_mix_f32(const float* x, const int64_t* perm, float lam, float* out, int B, int64_t sample_elems, void* stream);
/* UPSTREAM CutmixBlending.do_blending (`imgs[:, ..., bby1:bby2, bbx1:bbx2] = imgs[rand_index, ..., bby1:bby2, bbx1:bbx2]`;
 * configs/recognition/tsm/tsm_r50_cutmix_1x1x8_50e_sthv1_rgb.py:25-26) and tubemix (libs/cil/icarl_video_mix.py:59), in place:
 * afterwards x[b, :, r1:r2, c1:c2, :] holds what x[perm[b], :, r1:r2, c1:c2, :] held BEFORE the call, for any index vector (cycles of
 * any length, repeats; perm[b] == b costs nothing).  Two launches: the source boxes are packed into `scratch` per destination, then
 * written into the boxes: 4 x the box bytes.  0 <= r1 <= r2 <= H, 0 <= c1 <= c2 <= W; an empty box returns at once.  inner: 1 | 4.
 * scratch: 16-byte aligned, at least bdv_blend_box_scratch_bytes(...) bytes (0 for an empty box). */
size_t bdv_blend_box_scratch_bytes(int B, int outer, int inner, int r1, int c1, int r2, int c2);
int bdv_blend_box_f32(float* x, const int64_t* perm, int B, int outer, int H, int W, int inner, int r1, int c1, int r2, int c2,
                      void* scratch, size_t scratch_bytes, void* stream);

/* ---- foreground merging (FAME-style): motion masks + in-place merge ---------------------------------------------------------------
 * BEYOND THE REFERENCE: the reference has no such augmentation.  UPSTREAM, unpinned: FAME (Ding et al., "Motion-aware Contrastive
 * Video Representation Learning via Foreground-background Merging", CVPR 2022), restated from memory and fixed in DESIGN.md 4.11.
 * A clip batch is fp32 in one of three layouts: BDV_FG_TCHW (B, T, 3, H, W), BDV_FG_THWC4 the NHWC4 frames (B * T, H, W, 4) whose
 * fourth lane takes no part in the mask and moves with its pixel, BDV_FG_CTHW (B, 3, T, H, W).  All arithmetic is fp32, sums in the
 * stated order, no fused multiply-add.  B <= 65535, H * W <= 2^24, T * H * W <= 2^28.  Bases need 4-byte alignment only. */
#define BDV_FG_TCHW 0
#define BDV_FG_THWC4 1
#define BDV_FG_CTHW 2
/* beyond the reference (FAME stages 1-3): d[b,p] = (sum_{t<T-1} sum_c |x[b,t+1,c,p] - x[b,t,c,p]|) / (T - 1); tmp = d blurred along W,
 * g = tmp blurred along H with the k taps taps_host (HOST floats, k odd, 1 <= k <= 129, k / 2 < min(H, W); reflect border, edge not
 * repeated, taps added in ascending order); minmax[b] = {bits of min g[b], bits of max g[b]}; q = (uint8)floor(255 * (g - lo) /
 * (hi - lo + 1e-8f) + 0.5), 0 everywhere when hi == lo.  d, tmp, g: (B, H*W) fp32; partials: workspace of B * ceil(H*W / 256) * 2
 * uint32 (the per-workgroup min / max: no atomics); minmax: (B, 2) uint32; q: (B, H*W).  T >= 2. */
int bdv_fg_motion_q(const float* x, int B, int T, int H, int W, int layout, const float* taps_host, int k, float* d, float* tmp,
                    float* g, uint32_t* partials, uint32_t* minmax, uint8_t* q, void* stream);
/* beyond the reference (FAME stages 4-5): bin_c = clamp((int)floor((x_c - lo_host[c]) * scale_host[c]), 0, bins - 1) (a NaN: 0),
 * i = (bin_0 * bins + bin_1) * bins + bin_2; F[b,i] = sum of q over the (t,p) in bin i, N[b,i] their count, both uint32 by integer
 * atomics (cleared here); idx (B, T, HWp) uint16 with HWp = H*W rounded up to 4, 8-byte aligned, holds i; s[b,p] = (sum_t
 * float(F[b,i_t]) / (255.0f * float(N[b,i_t]))) / T.  bins 2..16; refuses 255 * T * H * W >= 2^32. */
int bdv_fg_hist_refine(const float* x, const uint8_t* q, int B, int T, int H, int W, int layout, int bins, const float lo_host[3],
                       const float scale_host[3], uint16_t* idx, uint32_t* F, uint32_t* N, float* s, void* stream);
/* beyond the reference (FAME stage 6): v[b] = the k_fg-th largest value of the non-negative map s[b] (B, HW), exactly (radix select
 * on the float bits, one workgroup per clip); mask[b,p] = (s >= v[b] and s > 0), so ties at the threshold are all foreground;
 * count[b] = its size.  1 <= k_fg <= HW. */
int bdv_fg_select(const float* s, int B, int HW, int k_fg, float* v, uint8_t* mask, int32_t* count, void* stream);
/* beyond the reference (FAME stage 7), in place: for every b with apply[b] != 0, perm[b] != b and count[b] > 0, every pixel with
 * mask[b,p] == 0 takes, in every frame and channel, the value it had in clip perm[b] BEFORE the call (gather-then-assign for any
 * index vector, as bdv_blend_box_f32); all other clips are neither read nor written.  perm: device int64 (B) in [0, B) (checked by
 * the caller on its host copy); apply: device uint8 (B); slot: device int32 (B), a distinct index in [0, nslots) for every b whose
 * source may itself be merged (apply[b], perm[b] != b, apply[perm[b]], perm[perm[b]] != perm[b]), else -1; scratch: 16-byte aligned,
 * nslots samples (T * H * W * 3 or 4 floats each). */
int bdv_fg_merge(float* x, const uint8_t* mask, const int32_t* count, const int64_t* perm, const uint8_t* apply, const int32_t* slot,
                 int nslots, int B, int T, int H, int W, int layout, void* scratch, size_t scratch_bytes, void* stream);

/* ---- optimizer: multi-tensor global-norm clip + SGD(momentum, wd) ---------------------------
 * torch.optim.SGD built at libs/cil/cil.py:467 with the groups of libs/models/cil_heads/tsm.py:273-303
 * and PL gradient_clip_val (cil.py:743).  Tables are device arrays, one entry per tensor. */
int bdv_multi_sqnorm(const float* const* grads, const int64_t* numels, int ntensors, float* out_sqnorm,
                     void* workspace, size_t workspace_bytes, void* stream);
/* clip_coef (device scalar) = min(1, max_norm / (sqrt(sqnorm)*grad_scale + 1e-6)); max_norm <= 0 -> 1 */
int bdv_clip_coef(const float* sqnorm, float grad_scale, float max_norm, float* clip_coef, void* stream);
/* g = grad*grad_scale*clip_coef + wd*p ; buf = momentum*buf + g ; p -= lr*buf */
int bdv_multi_sgd(float* const* params, const float* const* grads, float* const* bufs,
                  const int64_t* numels, const float* lrs, const float* wds, int ntensors,
                  float momentum, float grad_scale, const float* clip_coef, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BDVCIL_HIP_H */
