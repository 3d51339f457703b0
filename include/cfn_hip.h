/* cfn_hip.h -- C ABI of libcfn_hip.so: the MI355X (gfx950) kernels behind the Coarse-Fine hot path.
 *
 * The reference (kkahatapitiya/Coarse-Fine-Networks) is pure Python/PyTorch: it has no FFI of its
 * own, every heavy op is an ATen call.  Each entry point below therefore names the reference CALL
 * SITE (file:line under the reference tree) whose ATen op(s) it replaces; INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers to DEVICE memory + sizes; no torch types.  Tensors are dense NCDHW fp32 (the *_bf16 entry points
 *     at the end of this file take bf16 activations as `unsigned short*`).
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); kernels are enqueued on it and
 *     the call returns immediately; no allocation, no synchronisation, no host<->device copy inside
 *     (graph-capture safe).
 *   - return 0 on success, otherwise an error code (1 bad argument, 2 launch failure, 3 unsupported
 *     shape); cfn_last_error() returns a thread-local message.  Nothing ever aborts.
 *   - "prologue": many ops read their input x through  a = act(A[n,c]*x + B[n,c])  where A/B (float,
 *     N*C, may be NULL = identity) carry the folded SubBatchNorm3d scale/shift (+ BN affine + SE gate)
 *     and act is 0 none / 1 ReLU / 2 Swish / 3 sigmoid (sigmoid: cfn_affine_act_* only).  This is how SubBatchNorm3d.forward (x3d_fine.py:51-62),
 *     relu_ (:151), Swish (:74-86) and the SE multiply (:163) disappear into the next conv.
 *   - "stats": fp64 accumulators per (n,c) that the caller zero-fills; kernels atomically add
 *     per-workgroup partial sums.  sum/sumsq of a conv output are what batch_norm (train) and the SE
 *     average pool (x3d_fine.py:158) need; gsum/gsumsq are the gradients flowing back into them.
 */
#ifndef CFN_HIP_H
#define CFN_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* cfn_last_error(void);
const char* cfn_version(void);
int cfn_device_info(int* cus, int* lds_per_cu, char* name, int name_len);

/* opt-in HIP-event timing per kernel family (bench.py roofline leg). family: 0 dwconv fwd, 1 dwconv
 * bwd-data, 2 pwconv fwd, 3 pwconv bwd-data, 4 gridpool, 5 elementwise, 6 stem, 7 fusion, 8 pwconv bwd-weight,
 * 9 dwconv bwd-weight, 10 dense (Grid Pool saliency) conv fwd, 11 gridpool bwd (family 4 = Grid Pool resampler fwd).  collect() sums and
 * clears: total device ms between the bracketing events, launches, algorithmic bytes. */
int cfn_prof_enable(int family, int on);
int cfn_prof_collect(int family, double* total_ms, long* launches, double* total_bytes);

/* ---- depthwise 3x3x3, pad 1, stride (1,s,s): conv3x3x3 x3d_fine.py:89-97 used at :117 / x3d_coarse.py:87-95 ----
 * fwd   y[N,C,T,Ho,Wo] = dwconv(act(A x + B)); sum/sumsq[N*C] += sum y, sum y^2 (NULL to skip)
 * bwd_data   g' = gy + gsum[n,c] + 2 y gsumsq[n,c];  da = dwconv^T(g');  gx = da*act'(A x+B)*A;
 *            gA[N*C] += sum da*act'*x, gB += sum da*act'   (autograd of F.conv3d + batch_norm + relu_)
 * bwd_weight gw[C*27] (fp64, zero-filled by caller) += sum g' * act(A x + B)[tap] */
int cfn_dwconv3d_fwd(const float* x, const double* A, const double* B, int act, const float* w, float* y, double* sum,
                     double* sumsq, int N, int C, int T, int Hi, int Wi, int stride, void* stream);
int cfn_dwconv3d_bwd_data(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                          const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB,
                          int N, int C, int T, int Hi, int Wi, int stride, void* stream);
int cfn_dwconv3d_bwd_weight(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* x,
                            const double* A, const double* B, int act, double* gw, int N, int C, int T, int Hi, int Wi,
                            int stride, void* stream);
/* stride-1 data AND weight gradient in one pass over gy, y, x (4 tensor passes instead of 7): same outputs as the two
 * calls above.  Returns -1 without launching when the geometry is not handled (small planes): call the two kernels. */
int cfn_dwconv3d_bwd_fused(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                           const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB,
                           double* gw, int N, int C, int T, int H, int W, void* stream);
/* the same for the STRIDE-2 conv (H, W: input size; x is read once instead of twice).  Returns -1 without launching when the
 * geometry is not handled (handled: 112 -> 56, 56 -> 28, 28 -> 14 with a none / ReLU prologue): call the two kernels. */
int cfn_dwconv3d_bwd_fused_s2(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                              const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB,
                              double* gw, int N, int C, int T, int H, int W, void* stream);

/* Which kernel serves a depthwise 3x3x3 conv call, asked on the host (no GPU, no launch): the routing function the entry points above and their
 * _bf16 / _f16 versions call (csrc/dwroute.hip).  op: 0 forward, 1 data gradient, 2 weight gradient, 3 one-pass backward (stride 1:
 * cfn_dwconv3d_bwd_fused, stride 2: cfn_dwconv3d_bwd_fused_s2).  dtype: 0 fp32, 1 bf16, 2 fp16.  Hi, Wi: the conv's input plane.  flags: 1 prologue
 * A, B given, 2 forward: statistics asked for, backward: gsum given, 4 gsumsq and y given, 16 every tensor aligned to its element only (the plans
 * then see no wider alignment).  Writes "family kernel<template arguments> grid=.. wg=.. lds=..": the kernel as a kernel trace prints it, the grid in
 * workgroups ("AxBxC" when it has more than one dimension), workgroup size, dynamic LDS bytes; "declined" where op 3 would return -1.  A shape the
 * entry point refuses (output wider than 512, ...) returns the entry point's error. */
int cfn_dwconv3d_route(int op, int dtype, int N, int C, int T, int Hi, int Wi, int stride, int act, int flags, char* out, int cap);

/* ---- depthwise 5x1x1, pad (2,0,0): conv1_t x3d_fine.py:216-222 / x3d_coarse.py:502-508 ; plane = H*W ---- */
int cfn_dwconv_t5_fwd(const float* x, const float* w, float* y, double* sum, double* sumsq, int N, int C, int T,
                      long plane, void* stream);
int cfn_dwconv_t5_bwd_data(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                           float* gx, int N, int C, int T, long plane, void* stream);
int cfn_dwconv_t5_bwd_weight(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* x,
                             double* gw, int N, int C, int T, long plane, void* stream);
/* data AND weight gradient of conv1_t in one pass over gy, y, x (4 tensor passes instead of 6).  Returns -1 without launching
 * when the plane is not a whole number of float4s: call the two entry points above. */
int cfn_dwconv_t5_bwd_fused(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                            const float* x, float* gx, double* gw, int N, int C, int T, long plane, void* stream);

/* ---- pointwise 1x1x1, spatial stride s in {1,2}: conv1x1x1 x3d_fine.py:100-105 (conv1 :115, conv3 :119,
 * shortcut :284-287), conv5 :245-250, fc1 :256; fp32 MFMA (v_mfma_f32_32x32x2_f32).  w is (Cout,Cin).
 * bwd_data with stride 2 writes only the strided positions: caller zero-fills gx.
 * bwd_weight accumulates into gw (Cout,Cin) fp64, zero-filled by the caller (one atomic per element per workgroup). ---- */
int cfn_pwconv_fwd(const float* x, const double* A, const double* B, int act, const float* w, float* y, double* sum,
                   double* sumsq, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride, void* stream);
int cfn_pwconv_bwd_data(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                        const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB, int N,
                        int Cin, int Cout, int T, int Hi, int Wi, int stride, void* stream);
/* same, plus `acc`: compact gradient (N,Cin,T,ceil(Hi/acc_stride),ceil(Wi/acc_stride)) of a spatially strided shortcut conv
 * over the same input (x3d_fine.py:284-287), added on its lattice before the act' epilogue (requires stride == 1);
 * and `gscale` (N,Cout) fp64, may be NULL: gy is the UNSCALED gradient of a block tail (cfn_bn_add_relu_bwd_g) and stands
 * for gscale[n,c] * gy, i.e. g' = gscale*gy + gsum + 2*y*gsumsq */
int cfn_pwconv_bwd_data_acc(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                        const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB, int N,
                        int Cin, int Cout, int T, int Hi, int Wi, int stride, const float* acc, int acc_stride,
                        const double* gscale, void* stream);
int cfn_pwconv_bwd_weight(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* x,
                          const double* A, const double* B, int act, double* gw, int N, int Cin, int Cout, int T, int Hi,
                          int Wi, int stride, const double* gscale, void* stream);

/* Arithmetic of the fp32 pointwise contractions with >= 48 channels on both sides (layers 2-4; conv1x1x1 x3d_fine.py:100-105):
 * 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32), 3 / 6 = split-bf16: fp32 tensors, each operand split into 2 / 3 bf16 terms on load,
 * 3 / 6 v_mfma_f32_32x32x16_bf16 per k-block with fp32 accumulation (relative error of a product <= 3*2^-18 / 3*2^-27).
 * Default 6 (env CFN_PW_SPLIT).  -1 only queries.  Returns the previous setting.  Host-side, no stream. */
int cfn_pw_split_terms(int terms);

/* Which kernel a pointwise conv call would launch: op 0 cfn_pwconv_fwd, 1 cfn_pwconv_bwd_data_acc, 2 cfn_pwconv_bwd_weight, 3 cfn_pwconv_bwd_fused,
 * 4 cfn_pwconv_short_bwd -- the same routing function as the entry point, asked without a device or a stream.  flags: 1 = prologue A, B present,
 * 2 = statistics (forward: sum, sumsq; backward: gsum, and gsumsq where y is present too), 4 = y present, 8 = compact shortcut gradient acc present
 * (stride-2 lattice), 16 = tensors misaligned by 4 bytes.  Writes one line into out: family, kernel with the selected template arguments, grid,
 * workgroup size, dynamic LDS bytes, workspace bytes, "+lattice_add" where the shortcut gradient is added behind the contraction; "declined" where
 * the entry point would return -1 (ops 3, 4) or refuse the shape. */
int cfn_pwconv_route(int op, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride, int act, int flags, char* out, int cap);

/* Deterministic mode ("Threading / streams": "deterministic reductions preferred for parity tests (atomics order) -- offer a
 * deterministic mode"; the reference's own reductions are PyTorch's, train_fine.py:199-226 runs them in whatever mode torch is in).
 * on = 1: every cross-workgroup fp64 accumulation of the library (BN statistics, coefficient / weight gradients: ~100 sites) is recorded as an
 * (address, addend) pair instead of being added atomically; at the end of each entry point's launches the records are sorted by (address, addend
 * bits) and committed in that order, so results do not depend on the order in which workgroups finish: two identical calls give identical bits by
 * construction.  Costs a device synchronisation and a sort per entry point (parity runs, not benchmarks); not usable during hipGraph capture.
 * on = 0: fp64 atomics (default; env CFN_DETERMINISTIC=1 switches the mode on when the library is loaded by cfn_hip).  -1 only queries.
 * Returns the previous setting, < 0 on error.  Per process, bound to the device that is current at the call.  Host-side, no stream. */
int cfn_deterministic(int on);

/* Data AND weight gradient of a stride-1 pointwise conv in ONE pass: gy, y, x leave HBM once for both products.  Windows taken
 * (T*H*W a multiple of 4; gy, y, x 16-byte aligned; a prologue act of none / ReLU / swish):
 *   fp32 kernel (pwfused.hip): Cin, Cout <= 64 and not both > 32 -- X3D layer 1 (24 -> 54, 54 -> 24), with or without a prologue;
 *   split-bf16 kernel (pwfuseds.hip), no prologue: 33..64 -> 65..128 (layer 2 conv1, 48 -> 108), 16..32 -> 65..128 (its first
 *   block, 24 -> 108), 65..128 -> 33..64; with CFN_PWF_SPLIT=2 the same windows with a prologue (layer 2 conv3, 108 -> 48);
 *   layer-3 variant, no prologue: 33..96 -> 193..224 (layer 3 conv1, 96 -> 216, and its first block, 48 -> 216); with
 *   CFN_PWF_L3E=1 also 193..224 -> 65..96 behind a prologue, without `acc` (layer 3 conv3, 216 -> 96).
 * Same arguments and results as cfn_pwconv_bwd_data_acc (stride 1) + cfn_pwconv_bwd_weight (gw, gA, gB are added into); x is
 * always required.  Returns -1 WITHOUT launching when the shape / alignment is not handled (callers then use the two separate
 * entry points). */
int cfn_pwconv_bwd_fused(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                         const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB,
                         double* gw, int N, int Cin, int Cout, int T, int Hi, int Wi, const float* acc, int acc_stride,
                         const double* gscale, void* stream);

/* Backward of the spatially strided shortcut conv of a stage-first block (x3d_fine.py:284-287) in ONE pass over gy, y and the stride
 * lattice of x (pwshort.hip, fp32 MFMA): with g' = gscale*gy + gsum + 2*y*gsumsq on the output grid (Ho, Wo) = ((Hi-1)/2+1, (Wi-1)/2+1)
 *   da (N,Cin,T,Ho,Wo) = W^T g'        the COMPACT data gradient (no act' epilogue, no statistics: the `acc` of cfn_pwconv_bwd_data_acc /
 *                                      cfn_pwconv_bwd_fused, which conv1's backward adds on the lattice);
 *   gw (Cout,Cin) fp64 += g' a^T       a = act(A x + B) at (t, 2 oh, 2 ow); A, B (N,Cin) may be NULL; act none / ReLU.
 * gsum, gsumsq, gscale may each be NULL (y only with gsumsq).  The same results as cfn_pwconv_bwd_data_acc on the output grid +
 * cfn_pwconv_bwd_weight(stride 2).  Cout <= 192, Cin <= 96, any plane size.  Returns -1 WITHOUT launching (nothing is written) for any
 * other stride, width or activation, and when CFN_PW_SHORT=0 (read per call): callers then use the two separate entry points. */
int cfn_pwconv_short_bwd(const float* gy, const float* y, const double* gsum, const double* gsumsq, const double* gscale,
                         const float* w, const float* x, const double* A, const double* B, int act, float* da, double* gw,
                         int N, int Cin, int Cout, int T, int Hi, int Wi, int stride, void* stream);

/* ---- stem 1x3x3 stride (1,2,2) pad (0,1,1) dense conv: conv1_s x3d_fine.py:210-215 (im2col view on MFMA);
 * gw is fp64 (Cout, Cimg*9), zero-filled by caller.  The clip needs no gradient. ---- */
int cfn_stem_conv_fwd(const float* x, const float* w, float* y, int N, int Cimg, int Cout, int T, int Hi, int Wi,
                      void* stream);
int cfn_stem_conv_bwd_weight(const float* gy, const float* x, double* gw, int N, int Cimg, int Cout, int T, int Hi, int Wi,
                             void* stream);

/* ---- the stem pair conv1_s -> conv1_t (nothing sits between them, x3d_fine.py:334-335) as one kernel each way (csrc/stempair.hip).
 *   cfn_stem_pair_fwd: xs = cfn_stem_conv_fwd(x, w_s) and y, sum, sumsq = cfn_dwconv_t5_fwd(xs, w_t) with xs written once and not read back
 *     (xs and y bit-identical to the two entry points; sum / sumsq (N, 24) fp64 zero-filled by the caller, both or neither).
 *   cfn_stem_pair_bwd: gw_t (24, 5) and gw_s (24, 27), fp64, zero-filled by the caller = cfn_dwconv_t5_bwd_fused(gy, y, gsum, gsumsq, w_t, xs)
 *     followed by cfn_stem_conv_bwd_weight(gxs, x), without the tensor gxs.  gsum, gsumsq may be NULL (y only with gsumsq).
 * Workgroups walk runs of `run_frames` consecutive frames of one (sample, band of 2 output rows); 0 = the planner's choice (a run re-reads
 * (backward) or recomputes (forward) two halo frames on either side).  Both return -1 WITHOUT launching for anything but a 3 -> 24 channel
 * stem at 224 x 224 with 16-byte aligned tensors whose samples stay inside the 2 GiB buffer-descriptor range: callers then use the
 * separate entry points. ---- */
int cfn_stem_pair_fwd(const float* x, const float* w_s, const float* w_t, float* xs, float* y, double* sum, double* sumsq, int N,
                      int Cimg, int Cout, int T, int Hi, int Wi, int run_frames, void* stream);
int cfn_stem_pair_bwd(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w_t, const float* xs,
                      const float* x, double* gw_t, double* gw_s, int N, int Cimg, int Cout, int T, int Hi, int Wi, int run_frames,
                      void* stream);

/* ---- uint8 video frames, normalised on the GPU.  Replaces the host side ToTensor(255) + Normalize(mean, std) per frame
 * (spatial_transforms.py:46-85, :108-118) and the stack + permute per clip (charades_fine.py:170-173).
 * `unsigned char*` = uint8 tensor.  frames (N, T, H, W, 3) channels last, contiguous; lut (3, 256) fp32 = the normalised value of
 * every byte per channel, built on the host with the reference's operations (the converted clip is bit-identical to the
 * reference's); lengths (N) int32 or NULL (= all frames valid): frame t >= lengths[n] is zero padding and reads as 0.0.
 *   cfn_clip_u8_to_f32: x (N, 3, T, H, W) fp32, any H and W.
 *   cfn_stem_conv_u8_fwd / _bwd_weight: cfn_stem_conv_fwd / _bwd_weight of that clip without materialising it (Cimg must be 3;
 *   the forward is bit-identical: one kernel body serves both kinds of clip).  They return -1, with nothing launched, for a shape the
 *   fused kernels do not take (forward: Cout > 32, W % 4, odd H, frames off a 4-byte boundary, band image + table beyond 64 KiB of LDS;
 *   weight gradient: anything but 24 channels at 224 x 224): convert, then use the fp32 entry point.  cfn_conv3d_dense_route, ops 5 and 6,
 *   tells which on the host. ---- */
int cfn_clip_u8_to_f32(const unsigned char* frames, const float* lut, const int* lengths, float* x, int N, int T, int H, int W,
                       void* stream);
int cfn_stem_conv_u8_fwd(const unsigned char* frames, const float* lut, const int* lengths, const float* w, float* y, int N,
                         int Cimg, int Cout, int T, int Hi, int Wi, void* stream);
int cfn_stem_conv_u8_bwd_weight(const float* gy, const unsigned char* frames, const float* lut, const int* lengths, double* gw,
                                int N, int Cimg, int Cout, int T, int Hi, int Wi, void* stream);

/* ---- SubBatchNorm3d statistics -> (A,B) prologue, fused with the SE gate: SubBatchNorm3d.forward x3d_fine.py:51-62
 * (split groups, shared affine), nn.BatchNorm3d running-stat update, SE branch x3d_fine.py:157-163.
 * training: s,q (N,C) fp64 sums over `count` positions; run_mean/run_var = split_bn buffers (S*C) updated in place,
 * nbt = num_batches_tracked.  eval: run_mean/run_var = bn buffers (C).  Wd>0 enables SE (fc1 (Wd,C), fc2 (C,Wd),
 * pool_count = positions of the SE average).  Saved tensors (mean,rstd (S,C) fp64; A0,B0,gate,pooled (N,C); hbuf (N,Wd))
 * feed cfn_bn_fold_bwd, which returns gs,gq (N,C) fp64 (eval mode with SE: gs alone -- the gate still depends on sum(y) --,
 * gq NULL) and the parameter gradients (all overwritten). ---- */
int cfn_bn_fold_fwd(const double* s, const double* q, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    long* nbt, int training, int N, int C, int S, double count, double eps, double momentum, const float* w1,
                    const float* b1, const float* w2, const float* b2, int Wd, double pool_count, double* A, double* B,
                    double* mean, double* rstd, float* A0, float* B0, float* gate, float* hbuf, float* pooled, void* stream);
int cfn_bn_fold_bwd(const double* gA, const double* gB, const double* s, const float* gamma, const double* mean,
                    const double* rstd, const float* A0, const float* B0, const float* gate, const float* hbuf,
                    const float* pooled, const float* w1, const float* w2, int training, int N, int C, int S, int Wd,
                    double count, double pool_count, double* gs, double* gq, float* ggamma, float* gbeta, float* gw1,
                    float* gb1, float* gw2, float* gb2, double* tA, double* tB, void* stream);

/* ---- dense 3-D convolution as implicit GEMM (no im2col buffer): Grid Pool saliency convs x3d_coarse.py:362-366,
 * :379-381 (and the stem, which is the geom {1,3,3, 1,2,2, 0,1,1} case).  geom = int[9] {kT,kH,kW, sT,sH,sW, pT,pH,pW}
 * in HOST memory.  w (Cout, Cin*kT*kH*kW); no bias (a bias is algebraically folded into the next prologue / the
 * statistics by the caller).  Prologue act: none or relu; zero padding is applied after the prologue. ---- */
int cfn_conv3d_dense_fwd(const float* x, const double* A, const double* B, int act, const float* w, float* y, double* sum,
                         double* sumsq, int N, int Cin, int Cout, int T, int Hi, int Wi, const int* geom, void* stream);
int cfn_conv3d_dense_bwd_data(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w,
                              const float* x, const double* A, const double* B, int act, float* gx, double* gA, double* gB,
                              int N, int Cin, int Cout, int T, int Hi, int Wi, const int* geom, void* stream);
int cfn_conv3d_dense_bwd_weight(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* x,
                                const double* A, const double* B, int act, double* gw, int N, int Cin, int Cout, int T, int Hi,
                                int Wi, const int* geom, void* stream);
/* Which kernel a dense conv call would launch: op 0 cfn_conv3d_dense_fwd, 1 _bwd_data, 2 _bwd_weight, 3 cfn_stem_conv_fwd, 4 cfn_stem_conv_bwd_weight,
 * 5 cfn_stem_conv_u8_fwd, 6 cfn_stem_conv_u8_bwd_weight (geom ignored for 3 .. 6) -- the plan functions the launchers call, asked without a device or a stream.  flags: 1 = prologue A, B present (ReLU;
 * with 32: Swish), 2 = statistics (forward: sum, sumsq; backward: gsum), 4 = gsumsq and y present, 16 = every tensor misaligned by 4 bytes; one alone:
 * 64 = x, 128 = gy and y, 256 = the output (y / gx); ops 5, 6: 16 and 64 = the frames are off a 4-byte boundary.  cus: the
 * number of CUs to plan for, 0 = those of the current device (256 where there is none).  Writes one line into out: family, kernel with its
 * template arguments, grid= (workgroups), wg=, lds= (dynamic LDS bytes); the saliency kernels add bands= chunk= nchunks= last= (length of the last chunk) items=, the
 * stem kernels bands= chunk= (rows per band / items per workgroup) items=; "declined" where the entry point would refuse the call.  Ops 5, 6 where
 * the uint8 kernel does not take the call (the entry point returns -1): "convert " + the line of op 3 / 4 for the converted clip, a new, aligned
 * allocation -- what ops.stem_conv_u8 and torch.ops.cfn.stem_conv_u8 then run. */
int cfn_conv3d_dense_route(int op, int N, int Cin, int Cout, int T, int Hi, int Wi, const int* geom, int flags, int cus, char* out, int cap);

/* ---- Gaussian temporal alignment: Gaussian.forward x3d_coarse.py:256-286 (called at :651 / :657).
 * meta (B,4) int64 [start, frames, nf, step] (only columns 0 and 3 are read), mask (B,Tf), gx (B*crops,K) CDF knots or NULL
 * (tl = arange(K), the non-grid modes); tx = coarse clip length.  crops > 1 = validation-time multi-crop: row r = b*crops + j
 * starts at meta[b,0] + meta[b,3]*j (:264-266).  GX (B*crops,Tf,K).  bwd: ggx (B*crops,K) = d loss / d gx. ---- */
int cfn_gauss_align_fwd(const long* meta, const float* mask, const float* gx, double tx, double ratio, float* GX, int B, int crops,
                        int Tf, int K, void* stream);
int cfn_gauss_align_bwd(const float* gGX, const long* meta, const float* mask, const float* gx, double tx, double ratio,
                        float* ggx, int B, int crops, int Tf, int K, void* stream);

/* ---- Multi-stage Fusion temporal-alignment gather: RewightLayer.forward x3d_coarse.py:209-223 at the fine
 * features' native resolution, with the attention sigmoid (:219), the mask multiply (:213-216) and the multi-crop
 * repeat (:209-211) folded in.  x (B,C,Tf,P) fine features, at_raw (B,Tf,P) attention logits (at = sigmoid(at_raw +
 * at_bias[0]); at_bias may be NULL), GX (B*crops,Tf,K), mask (B,Tf);  row r = b*crops + j:
 *   z[r,c,k,p] = sum_t x[b] at[b] GX[r] mask[b] / (sum_t at GX mask + 1e-6), den (B*crops,K,P) saved for the backward.
 * bwd: gx (B,C,Tf,P), gat (B,Tf,P) = d loss / d at_raw, gGX (B*crops,Tf,K) (each may be NULL);
 * dw (B*crops,Tf,K,P) is scratch. ---- */
int cfn_fusion_gather_fwd(const float* x, const float* at_raw, const float* at_bias, const float* GX, const float* mask, float* z,
                          float* den, int B, int crops, int C, int Tf, int K, int P, void* stream);
int cfn_fusion_gather_bwd(const float* gz, const float* z, const float* den, const float* x, const float* at_raw,
                          const float* at_bias, const float* GX, const float* mask, float* gx, float* gat, float* gGX, float* dw,
                          int B, int crops, int C, int Tf, int K, int P, void* stream);

/* ---- block tail  out = relu(A y + B + (Ar res + Br)) : bn3 + (downsample bn) + `out += residual` + relu,
 * x3d_fine.py:167-173.  Ar/Br NULL = identity shortcut.  vol = T*H*W, NC = N*C.  bwd: gout2 (may be NULL) is a second
 * upstream gradient of the same output (the block output feeds the next conv1 AND the next residual); it is added to
 * gout on the fly. ---- */
int cfn_bn_add_relu_fwd(const float* y, const double* A, const double* B, const float* res, const double* Ar, const double* Br,
                        float* out, int* mask, long NC, long vol, void* stream);
int cfn_bn_add_relu_bwd(const float* gout, const float* gout2, const float* out, const float* y, const double* A, const float* res,
                        const double* Ar, float* gy, float* gres, double* gA, double* gB, double* gAr, long NC, long vol,
                        void* stream);
/* The tail's backward as ONE output tensor: g = (gout [+ gout2]) * (out > 0) serves as d/dy (the conv3 backward applies A
 * through `gscale`) and as d/dres (identity shortcut: exact; conv shortcut: `gscale` = Ar) -- 4 tensor passes instead of
 * 6-7.  The ReLU mask is either `out` or the bit mask cfn_bn_add_relu_fwd wrote (`mask`, cfn_bn_add_relu_mask_words(NC,
 * vol) 32-bit words, 0 = shape has no mask; bit layout private to the two kernels): exactly one of the two is given.
 * gA += sum g*y, gB += sum g, gAr += sum g*res (gAr may be NULL). */
long cfn_bn_add_relu_mask_words(long NC, long vol);
int cfn_bn_add_relu_bwd_g(const float* gout, const float* gout2, const float* out, const int* mask, const float* y,
                          const float* res, float* g, double* gA, double* gB, double* gAr, long NC, long vol, void* stream);

/* ---- materialised prologue out = act(A x + B) (SubBatchNorm3d.forward on its own, x3d_fine.py:51-62) and
 * per-(n,c) sum / sumsq of a tensor (batch statistics of an arbitrary input) ---- */
int cfn_affine_act_fwd(const float* x, const double* A, const double* B, int act, float* out, long NC, long vol, void* stream);
int cfn_affine_act_bwd(const float* gout, const float* x, const double* A, const double* B, int act, float* gx, double* gA,
                       double* gB, long NC, long vol, void* stream);
int cfn_channel_stats(const float* x, double* sum, double* sumsq, long NC, long vol, void* stream);

/* ---- adaptive spatial mean of act(A x + B) to (OH,OW): adaptive_avg_pool3d((None,1,1)) x3d_fine.py:255/366 and
 * ((None,7,7)) :345-363 (ATen window rule: [floor(o*S/O), ceil((o+1)*S/O)) ) ---- */
int cfn_pool_hw_fwd(const float* x, const double* A, const double* B, int act, float* out, long NC, int T, int H, int W, int OH,
                    int OW, void* stream);
int cfn_pool_hw_bwd(const float* gout, const float* x, const double* A, const double* B, int act, float* gx, double* gA,
                    double* gB, long NC, int T, int H, int W, int OH, int OW, void* stream);

/* ---- FiLM x*m + c with (H/f x W/f)-block-constant m, c: `x = x * m2 + c2` x3d_coarse.py:663-679 after the
 * fusion branch was evaluated at its native 7x7 ---- */
int cfn_film_fwd(const float* x, const float* m, const float* c, float* out, long NC, int T, int H, int W, int f,
                 void* stream);
int cfn_film_bwd(const float* g, const float* x, const float* m, float* gx, float* gm, float* gc, long NC, int T, int H,
                 int W, int f, void* stream);

/* ---- Grid Pool / Unpool resampler: 5-D F.grid_sample(align_corners=True) of x3d_coarse.py:403 / :447 as a
 * 2-tap lerp along t at i_t = ((2(cdf-0.5)+1)/2)(Tin-1).  i0 = floor(i_t) is bit-exact w.r.t. ATen.
 * x (B,C,Tin,P), cdf (B,K) -> out (B,C,K,P).  bwd: gx (B,C,Tin,P) fully written, gcdf (B,K) fp64 zero-filled
 * by the caller; either may be NULL. ---- */
int cfn_grid_time_index(const float* cdf, int n, int Tin, int* i0, float* w1, void* stream);
/* saliency logits g (B,Kin) (+ bias[0], may be NULL) -> CDF knots (B,Kin+1): x3d_coarse.py:384-392
 * (1 - sigmoid(g/2), normalise, cumsum in fp64, leading 0).  bwd: gg (B,Kin) from gcdf (B,Kin+1). */
int cfn_grid_cdf_fwd(const float* g, const float* bias, float* cdf, int B, int Kin, void* stream);
int cfn_grid_cdf_bwd(const float* gcdf, const float* g, const float* bias, float* gg, int B, int Kin, void* stream);
int cfn_time_sample_fwd(const float* x, const float* cdf, float* out, int B, int C, int Tin, int K, long P, void* stream);
int cfn_time_sample_bwd(const float* g, const float* x, const float* cdf, float* gx, double* gcdf, int B, int C, int Tin,
                        int K, long P, void* stream);

/* ---- fixed temporal pooling t_pool = 'avg' (mode 0) | 'max' (mode 1): nn.AvgPool3d / nn.MaxPool3d((R,1,1), stride (R,1,1))
 * x3d_coarse.py:489-492 / :640-643.  x (BC,Tin,P) -> out (BC,floor(Tin/R),P); bwd writes all of gx (max: first maximal frame) ---- */
int cfn_time_pool_fwd(const float* x, float* out, int mode, long BC, int Tin, int R, long P, void* stream);
int cfn_time_pool_bwd(const float* g, const float* x, float* gx, int mode, long BC, int Tin, int R, long P, void* stream);

/* ---- Interp1d.forward interp1d.py:8-147: x,y (B or 1 rows, N), xnew (B or 1 rows, Pq) -> ynew (B,Pq), ind int64
 * (searchsorted-left - 1, clamped to [0,N-2]).  *row flags: 1 = one row per batch entry, 0 = shared row.
 * bwd overwrites gx/gy/gq (any may be NULL) in gather form: every sum has a fixed order (reproducible). ---- */
int cfn_interp1d_fwd(const float* x, const float* y, const float* xnew, float* ynew, long* ind, int B, int N, int Pq,
                     int xrow, int yrow, int qrow, void* stream);
int cfn_interp1d_bwd(const float* g, const float* x, const float* y, const float* xnew, const long* ind, float* gx, float* gy,
                     float* gq, int B, int N, int Pq, int xrow, int yrow, int qrow, void* stream);

/* ---- linear resize along t: F.interpolate(mode='linear') x3d_coarse.py:725, the t axis of :449 (align_corners=1) and
 * the loss upsampling train_coarse_fineFEAT.py:226 / train_fine.py:204 (align_corners=0, half-pixel centres).
 * x (BC,Kin,P) -> out (BC,Lout,P) ---- */
int cfn_time_resize_fwd(const float* x, float* out, long BC, int Kin, int Lout, long P, int align_corners, void* stream);
int cfn_time_resize_bwd(const float* g, float* gx, long BC, int Kin, int Lout, long P, int align_corners, void* stream);

/* ---- detection loss, fused (opt-in; csrc/detloss.hip): train_fine.py:199-213 (align_corners=1) / train_coarse_fineFEAT.py:226-240
 * (align_corners=0), n = crops per video (train_fine.py:204-207: max over the crops' sigmoids).
 * logits (B*n,C,T), labels (B,C,TL), masks (B,TL) fp32 -> probs (B,C,TL) = max_n sigmoid(resize(logits)) * masks (NULL: not stored),
 * cls = mean_BC BCE(max_t probs, max_t labels), loc = sum BCE(probs, labels) / norm * world; norm: device scalar, NULL = C * sum(masks).
 * BCE as ATen: on the fp32 probability, logs clamped at -100.  Kept for the backward: jstar (BC) first frame of the row maximum,
 * ymax (BC) = max_t labels, norm_used (1); rows (2*BC) is scratch.  Fixed-order fp64 sums, no atomics: bit-reproducible.
 * bwd: g_cls, g_loc device scalars (the fp16 path's loss scale lives on the device); recomputes the probabilities from the logits and
 * overwrites all of gx (B*n,C,T); a crop that never held the maximum gets zeros.  n*T <= 6144. ---- */
int cfn_detloss_fwd(const float* logits, const float* labels, const float* masks, const float* norm, double world, float* probs,
                    float* cls, float* loc, int* jstar, float* ymax, double* rows, double* norm_used, int B, int C, int T, int TL,
                    int n, int align_corners, void* stream);
int cfn_detloss_bwd(const float* g_cls, const float* g_loc, const float* logits, const float* labels, const float* masks,
                    const int* jstar, const float* ymax, const double* norm_used, double world, float* gx, int B, int C, int T,
                    int TL, int n, int align_corners, void* stream);

/* =====================================================================================================================
 * bf16 activation path (BASELINE.json configs[1] "X3D-M fwd+bwd bf16"; the reference itself is fp32 only: these entry
 * points are the same call sites with activations and activation gradients stored as bf16 in HBM).
 *   - `unsigned short*` = bf16 tensor (round to nearest even on store); weights, prologue coefficients, statistics and
 *     every reduction stay fp32 / fp64 exactly as in the fp32 entry points; all arithmetic is fp32.
 *   - pointwise contractions run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; BN statistics are taken over the
 *     ROUNDED outputs (what the consumer reads back).
 *   - the stem conv (fp32 clip in) keeps an fp32 output; conv1_t (cfn_dwconv_t5_*_bf16) reads fp32 and writes bf16, and
 *     returns an fp32 input gradient.  Pooled head / feature-tower tensors are fp32 (cfn_pool_hw_*_bf16 leaves the
 *     bf16 domain).
 *   - shape limits: pointwise needs T*H*W even (fwd / bwd_data) and a multiple of 8 (bwd_weight); a spatially strided
 *     pointwise conv = cfn_subsample_hw_bf16 + the stride-1 contraction on the compact tensor.
 * ===================================================================================================================== */
/* conv1x1x1 x3d_fine.py:100-105 (stride 1; Q = T*H*W positions per (n, channel) row) */
int cfn_pwconv_fwd_bf16(const unsigned short* x, const double* A, const double* B, int act, const float* w, unsigned short* y,
                        double* sum, double* sumsq, int N, int Cin, int Cout, long Q, void* stream);
/* as cfn_pwconv_bwd_data_acc: acc = compact (N,Cin,T,ceil(H/s),ceil(W/s)) gradient of a strided second consumer, gscale (N,Cout) */
int cfn_pwconv_bwd_data_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                             const float* w, const unsigned short* x, const double* A, const double* B, int act,
                             unsigned short* gx, double* gA, double* gB, int N, int Cin, int Cout, int T, int H, int W,
                             const unsigned short* acc, int acc_stride, const double* gscale, void* stream);
int cfn_pwconv_bwd_weight_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                               const unsigned short* x, const double* A, const double* B, int act, double* gw, int N, int Cin,
                               int Cout, long Q, const double* gscale, void* stream);
/* x[..., ::s, ::s] of (planes = N*C*T, H, W): the gather in front of a strided shortcut conv (x3d_fine.py:284-287) */
int cfn_subsample_hw_bf16(const unsigned short* x, unsigned short* out, long planes, int H, int W, int s, void* stream);

/* conv3x3x3 depthwise x3d_fine.py:89-97: cfn_dwconv3d_* with bf16 tensors (same kernels compiled for 2-byte elements) */
int cfn_dwconv3d_fwd_bf16(const unsigned short* x, const double* A, const double* B, int act, const float* w, unsigned short* y,
                          double* sum, double* sumsq, int N, int C, int T, int Hi, int Wi, int stride, void* stream);
int cfn_dwconv3d_bwd_data_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                               const float* w, const unsigned short* x, const double* A, const double* B, int act,
                               unsigned short* gx, double* gA, double* gB, int N, int C, int T, int Hi, int Wi, int stride,
                               void* stream);
int cfn_dwconv3d_bwd_weight_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                 const unsigned short* x, const double* A, const double* B, int act, double* gw, int N, int C,
                                 int T, int Hi, int Wi, int stride, void* stream);
int cfn_dwconv3d_bwd_fused_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                const float* w, const unsigned short* x, const double* A, const double* B, int act,
                                unsigned short* gx, double* gA, double* gB, double* gw, int N, int C, int T, int H, int W,
                                void* stream);
int cfn_dwconv3d_bwd_fused_s2_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                   const float* w, const unsigned short* x, const double* A, const double* B, int act,
                                   unsigned short* gx, double* gA, double* gB, double* gw, int N, int C, int T, int H, int W,
                                   void* stream);

/* conv1_t depthwise 5x1x1 x3d_fine.py:216-222: x / gx fp32, y / gy bf16 */
int cfn_dwconv_t5_fwd_bf16(const float* x, const float* w, unsigned short* y, double* sum, double* sumsq, int N, int C, int T,
                           long plane, void* stream);
int cfn_dwconv_t5_bwd_data_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                const float* w, float* gx, int N, int C, int T, long plane, void* stream);
int cfn_dwconv_t5_bwd_weight_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                  const float* x, double* gw, int N, int C, int T, long plane, void* stream);
int cfn_dwconv_t5_bwd_fused_bf16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                 const float* w, const float* x, float* gx, double* gw, int N, int C, int T, long plane,
                                 void* stream);

/* block tail x3d_fine.py:167-173 (cfn_bn_add_relu_fwd / _bwd_g) and spatial pooling :255,:345-366 (bf16 in, fp32 pooled) */
long cfn_bn_add_relu_mask_words_bf16(long NC, long vol);
int cfn_bn_add_relu_fwd_bf16(const unsigned short* y, const double* A, const double* B, const unsigned short* res,
                             const double* Ar, const double* Br, unsigned short* out, int* mask, long NC, long vol, void* stream);
int cfn_bn_add_relu_bwd_g_bf16(const unsigned short* gout, const unsigned short* gout2, const unsigned short* out, const int* mask,
                               const unsigned short* y, const unsigned short* res, unsigned short* g, double* gA, double* gB,
                               double* gAr, long NC, long vol, void* stream);
int cfn_pool_hw_fwd_bf16(const unsigned short* x, const double* A, const double* B, int act, float* out, long NC, int T, int H,
                         int W, int OH, int OW, void* stream);
int cfn_pool_hw_bwd_bf16(const float* gout, const unsigned short* x, const double* A, const double* B, int act,
                         unsigned short* gx, double* gA, double* gB, long NC, int T, int H, int W, int OH, int OW, void* stream);

/* =====================================================================================================================
 * fp16 activation path (BASELINE configs[4]: "fp16 MFMA pointwise"; the reference itself is fp32 only, x3d_fine.py:100-105).
 * The entry points of the bf16 path above with IEEE-half tensors: `unsigned short*` = fp16 tensor (round to nearest even on
 * store), pointwise contractions on v_mfma_f32_32x32x16_f16 with fp32 accumulation, everything else exactly as for bf16
 * (csrc/h16.h: the same sources compiled for the other 2-byte element kind).  fp16 has 3 more mantissa bits than bf16 and 5 exponent
 * bits: activation GRADIENTS need a loss scale (train_joint.py LOSS_SCALE; weight gradients accumulate in fp64 and are unscaled there).
 * The weight gradient keeps the direct-operand kernel (the LDS-staged one of pwsplitw.hip serves fp32 and bf16 tensors).
 * ===================================================================================================================== */
/* conv1x1x1 x3d_fine.py:100-105 (stride 1; Q = T*H*W positions per (n, channel) row) */
int cfn_pwconv_fwd_f16(const unsigned short* x, const double* A, const double* B, int act, const float* w, unsigned short* y,
                        double* sum, double* sumsq, int N, int Cin, int Cout, long Q, void* stream);
/* as cfn_pwconv_bwd_data_acc: acc = compact (N,Cin,T,ceil(H/s),ceil(W/s)) gradient of a strided second consumer, gscale (N,Cout) */
int cfn_pwconv_bwd_data_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                             const float* w, const unsigned short* x, const double* A, const double* B, int act,
                             unsigned short* gx, double* gA, double* gB, int N, int Cin, int Cout, int T, int H, int W,
                             const unsigned short* acc, int acc_stride, const double* gscale, void* stream);
int cfn_pwconv_bwd_weight_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                               const unsigned short* x, const double* A, const double* B, int act, double* gw, int N, int Cin,
                               int Cout, long Q, const double* gscale, void* stream);
/* x[..., ::s, ::s] of (planes = N*C*T, H, W): the gather in front of a strided shortcut conv (x3d_fine.py:284-287) */
int cfn_subsample_hw_f16(const unsigned short* x, unsigned short* out, long planes, int H, int W, int s, void* stream);

/* conv3x3x3 depthwise x3d_fine.py:89-97: cfn_dwconv3d_* with fp16 tensors (same kernels compiled for 2-byte elements) */
int cfn_dwconv3d_fwd_f16(const unsigned short* x, const double* A, const double* B, int act, const float* w, unsigned short* y,
                          double* sum, double* sumsq, int N, int C, int T, int Hi, int Wi, int stride, void* stream);
int cfn_dwconv3d_bwd_data_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                               const float* w, const unsigned short* x, const double* A, const double* B, int act,
                               unsigned short* gx, double* gA, double* gB, int N, int C, int T, int Hi, int Wi, int stride,
                               void* stream);
int cfn_dwconv3d_bwd_weight_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                 const unsigned short* x, const double* A, const double* B, int act, double* gw, int N, int C,
                                 int T, int Hi, int Wi, int stride, void* stream);
int cfn_dwconv3d_bwd_fused_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                const float* w, const unsigned short* x, const double* A, const double* B, int act,
                                unsigned short* gx, double* gA, double* gB, double* gw, int N, int C, int T, int H, int W,
                                void* stream);
int cfn_dwconv3d_bwd_fused_s2_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                   const float* w, const unsigned short* x, const double* A, const double* B, int act,
                                   unsigned short* gx, double* gA, double* gB, double* gw, int N, int C, int T, int H, int W,
                                   void* stream);

/* conv1_t depthwise 5x1x1 x3d_fine.py:216-222: x / gx fp32, y / gy fp16 */
int cfn_dwconv_t5_fwd_f16(const float* x, const float* w, unsigned short* y, double* sum, double* sumsq, int N, int C, int T,
                           long plane, void* stream);
int cfn_dwconv_t5_bwd_data_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                const float* w, float* gx, int N, int C, int T, long plane, void* stream);
int cfn_dwconv_t5_bwd_weight_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                  const float* x, double* gw, int N, int C, int T, long plane, void* stream);
int cfn_dwconv_t5_bwd_fused_f16(const unsigned short* gy, const unsigned short* y, const double* gsum, const double* gsumsq,
                                 const float* w, const float* x, float* gx, double* gw, int N, int C, int T, long plane,
                                 void* stream);

/* block tail x3d_fine.py:167-173 (cfn_bn_add_relu_fwd / _bwd_g) and spatial pooling :255,:345-366 (fp16 in, fp32 pooled) */
long cfn_bn_add_relu_mask_words_f16(long NC, long vol);
int cfn_bn_add_relu_fwd_f16(const unsigned short* y, const double* A, const double* B, const unsigned short* res,
                             const double* Ar, const double* Br, unsigned short* out, int* mask, long NC, long vol, void* stream);
int cfn_bn_add_relu_bwd_g_f16(const unsigned short* gout, const unsigned short* gout2, const unsigned short* out, const int* mask,
                               const unsigned short* y, const unsigned short* res, unsigned short* g, double* gA, double* gB,
                               double* gAr, long NC, long vol, void* stream);
int cfn_pool_hw_fwd_f16(const unsigned short* x, const double* A, const double* B, int act, float* out, long NC, int T, int H,
                         int W, int OH, int OW, void* stream);
int cfn_pool_hw_bwd_f16(const float* gout, const unsigned short* x, const double* A, const double* B, int act,
                         unsigned short* gx, double* gA, double* gB, long NC, int T, int H, int W, int OH, int OW, void* stream);

/* =====================================================================================================================
 * Spatial augmentation of uint8 frames on the GPU (csrc/aug_u8.hip): square crop, antialiased bilinear resize and horizontal
 * flip, bit-exact to PIL's 8-bit Image.resize(BILINEAR).  Replaces the reference's per-frame CPU transforms
 * MultiScaleRandomCropMultigrid + RandomHorizontalFlip (train_fine.py:74-77, train_coarse_fineFEAT.py:79-82;
 * transforms/spatial_transforms.py:480-510, :339-357) and CenterCropScaled (train_fine.py:78, extract_fineFEAT.py:76;
 * spatial_transforms.py:201-230).
 *   src (N,T,Hs,Ws,3) uint8, each clip's picture in the top-left corner; box (N,4) = x1, y1, c, flip; bounds (N,S,2) = xmin, n and
 *   coef (N,S,K) = 22-bit fixed-point taps of the c -> S resize, zero behind n (cfn_hip/u8aug.py builds them on the host; one table
 *   serves both axes); dst (N,T,S,S,3); lengths (N) or NULL: frames t >= lengths[n] are written as zero bytes.
 * Horizontal pass first, rounded to uint8, then the vertical pass on those bytes; int32 accumulators.  One launch on `stream`, no
 * allocation (capturable).  Every source read is checked against the extent of src: a bad box gives wrong bytes, never a fault.
 * Returns 1 for null pointers / non-positive sizes, -1 with nothing launched for K > 9 (c > 4 * S) or an S too wide for the
 * kernel's LDS image (64 KB: S <= 312 at K = 9).
 * ===================================================================================================================== */
int cfn_crop_resize_flip_u8(const unsigned char* src, const int* lengths, const int* box, const int* bounds, const int* coef,
                            unsigned char* dst, int N, int T, int Hs, int Ws, int S, int K, void* stream);

/* =====================================================================================================================
 * Per-class average precision on the GPU (csrc/apmeter.hip): the device-resident form of apmeter.APMeter (reference
 * apmeter.py:22-136).  Per class: a STABLE descending sort of the scores in insertion order (numpy's order on special values:
 * +0.0 and -0.0 tie, denormals are distinct, every NaN sorts behind -inf), AP = (sum over the positive ranks r of tp_r / r) /
 * max(npos, 1).
 *   scores (K, cap) fp32 and targets (K, cap) uint8: class-major stores, row i of class k at k * cap + i (64-bit offsets);
 *   count: ONE int on the device, the rows held; flags: one int on the device, bit 0 = a label that is neither 0 nor 1 was
 *   appended, bit 1 = a batch did not fit into cap (nothing of it was written, count unchanged).
 * No entry point reads count on the host; no grid size depends on it; each is capturable (no allocation, no synchronisation,
 * also in deterministic mode: nothing here accumulates in floating point across workgroups).  Results are bit-identical from
 * run to run.
 *   cfn_ap_append: probs, labels (B, K, TL) fp32; valid (B) int32 or NULL (= TL frames each).  Video b contributes frames
 *     0 .. min(valid[b], TL) - 1 of every class, videos in batch order, frames ascending; target byte = label != 0.
 *   cfn_ap_sort: rows 0 .. count - 1 of every class of scores / targets -> sorted_scores / sorted_targets (K, cap), the rows
 *     behind count untouched; tmp_keys (K, cap) int32 and tmp_targets (K, cap) uint8 are scratch.  LSD radix sort, 8-bit digits,
 *     one workgroup per class.  The sorted scores are canonical: +0.0 for -0.0, one NaN pattern for every NaN.
 *   cfn_ap_reduce: sorted target bytes -> ap (K) fp32; a class without a positive gives 0.  fp64 sums in a fixed order.
 *   cfn_ap_sort_tile: rows per tile of the sort (host only).
 * Return 1 for null pointers and for K, cap, TL, B <= 0 (cap must be below 2^31 less one tile; K, B <= 65535).
 * ===================================================================================================================== */
int cfn_ap_append(const float* probs, const float* labels, const int* valid, float* scores, unsigned char* targets, int* count,
                  int* flags, int B, int K, int TL, long cap, void* stream);
int cfn_ap_sort(const float* scores, const unsigned char* targets, const int* count, float* sorted_scores,
                unsigned char* sorted_targets, int* tmp_keys, unsigned char* tmp_targets, int K, long cap, void* stream);
int cfn_ap_reduce(const unsigned char* sorted_targets, const int* count, float* ap, int K, long cap, void* stream);
int cfn_ap_sort_tile(void);

/* =====================================================================================================================
 * Packed 16-bit fine features (csrc/featpack.hip; the record format and the batch type: cfn_hip/featpack.py).  The five feature
 * maps of the Fine stream (reference extract_fineFEAT.py:153-173, read back by charades_coarse_fineFEAT.py:84-87) are stored
 * and moved as fp16 (_f16) or bf16 (_bf16), unpadded and time-major: per video and key a block (T', C_k, 49).
 *   cfn_feat_unpack: data = `total` 16-bit elements starting on a 16-byte boundary; offsets (B, 5) = first element of every
 *     block, multiples of 8; lengths (B).  out_k (B, C_k, t_max, 49) fp32:
 *       out_k[b, c, t, p] = t < lengths[b] ? widen(data[offsets[b, k] + (t * C_k + c) * 49 + p]) : 0.0f
 *     EVERY element of the five outputs is written; widening is exact (fp16 subnormals included).  offsets and lengths are read
 *     on the device only: a length is clamped to [0, t_max], an offset is rounded down to a multiple of 8 and every read is
 *     checked against `total` (a bad offset gives wrong values, never a fault).
 *   cfn_feat_pack: x_k (C_k, T, 49) fp32, the maps of ONE video -> dst = its payload, the five blocks (T, C_k, 49) back to
 *     back in key order, starting on a 16-byte boundary.  Round to nearest even, bit-identical to the CPU's tensor.to(dtype)
 *     for every finite value (fp16 overflow -> inf); a NaN stays a NaN.
 * One launch each on `stream`, no allocation, no synchronisation (capturable).  Return 1 for null pointers, B < 1, t_max / T < 1,
 * a channel count that is not a positive multiple of 8, or a misaligned 16-bit buffer.
 * ===================================================================================================================== */
int cfn_feat_unpack_f16(const unsigned short* data, const long* offsets, const int* lengths, float* out0, float* out1, float* out2,
                        float* out3, float* out4, int B, int t_max, int c0, int c1, int c2, int c3, int c4, long total, void* stream);
int cfn_feat_unpack_bf16(const unsigned short* data, const long* offsets, const int* lengths, float* out0, float* out1, float* out2,
                         float* out3, float* out4, int B, int t_max, int c0, int c1, int c2, int c3, int c4, long total, void* stream);
int cfn_feat_pack_f16(const float* x0, const float* x1, const float* x2, const float* x3, const float* x4, unsigned short* dst, int T,
                      int c0, int c1, int c2, int c3, int c4, void* stream);
int cfn_feat_pack_bf16(const float* x0, const float* x1, const float* x2, const float* x3, const float* x4, unsigned short* dst, int T,
                       int c0, int c1, int c2, int c3, int c4, void* stream);

/* =====================================================================================================================
 * Baseline JPEG frames decoded on the GPU (csrc/jpegdec.hip; the host side and the batch type: cfn_hip/jpegdec.py), bit for bit
 * what PIL with libjpeg gives.  Replaces the reference's per-frame host decode Image.open(f).convert('RGB') in pil_loader /
 * video_loader of charades_fine.py and charades_coarse_fineFEAT.py.  Baseline sequential DCT, 8 bit, one interleaved scan; gray
 * or YCbCr 4:4:4 / 4:2:2 / 4:2:0; restart intervals.
 *   data: `data_bytes` bytes, every frame's entropy-coded segment (stuffed zeros and RSTn kept), each on a 4-byte boundary and
 *     followed by >= 8 zero bytes.  frames (rows, 8) int32 per frame: clip, t, offset, bytes, table set, restart interval, first
 *     decoder lane, decoder lanes (= restart intervals).  tables (sets, 3456) int32: 2 quantisation tables in natural order
 *     (component 0; components 1 and 2), then DC0, DC1, AC0, AC1 as look[512] (9-bit lookahead: length << 8 | symbol), maxcode[32],
 *     valoff[32] (both indexed by code length), huffval[256].  geom (N, 4) int32 per clip: h, w, luma sampling (h << 4 | v),
 *     components.  lengths (N) int32.
 *   out (N, Tmax, Hmax, Wmax, 3) uint8: EVERY byte is written -- the h x w picture of frame (clip, t) in the top-left corner,
 *     zero bytes beside and below it and in frames no row of `frames` names.  status (rows) int32, zeroed by the call: 0 = decoded,
 *     bit 0 = the frame's record disagrees with the batch, bit 1 = ran out of data / a restart marker is missing, bit 2 = invalid
 *     Huffman code.  Such a frame stops where it is; every other frame is unaffected.
 *   ws: cfn_jpeg_workspace_bytes(rows, N * Tmax, lanes, blocks_max) bytes on a 16-byte boundary (lanes = sum of the frames' decoder
 *     lanes, blocks_max = most 8 x 8 blocks of one frame): int16 coefficients [frame][component][block row][block column][64],
 *     planar 8-bit samples, interval starts.  The library keeps no state; the caller owns the buffer until the stream has passed.
 * Entropy decode runs one lane per (frame, restart interval); dequantise + jidctint ("islow", int32) one lane per block; "fancy"
 * upsampling + YCbCr -> RGB one lane per 4 pixels.  Records, tables and geometry are DATA read on the device: every index derived
 * from them is checked or masked, every loop bound is independent of the bit stream (a bad batch sets status, never faults or
 * spins).  3 memsets + 4 launches on `stream`, no allocation, no synchronisation.  Returns 1 for null pointers, non-positive
 * sizes, data of 2 GiB or more, misaligned buffers or a workspace that is too small; cfn_jpeg_workspace_bytes -1 for
 * non-positive sizes.
 * ===================================================================================================================== */
long cfn_jpeg_workspace_bytes(int rows, long slots, int lanes, int blocks_max);
int cfn_jpeg_decode_u8(const unsigned char* data, const int* frames, const int* tables, const int* geom, const int* lengths,
                       unsigned char* out, int* status, void* ws, long ws_bytes, long data_bytes, int rows, int sets, int N,
                       int Tmax, int Hmax, int Wmax, int lanes, int blocks_max, void* stream);

/* =====================================================================================================================
 * cfn_jpeg_decode_u8 with the SYNC entropy mode (csrc/jpegdec.hip jpeg_entropy_sync_kernel; stated on the CPU by
 * cfn_hip/jpegdec.py decode_coefficients_sync): the same replacement of the reference's per-frame host decode,
 * Image.open(f).convert('RGB') in pil_loader / video_loader of charades_fine.py and charades_coarse_fineFEAT.py, bit for bit, for
 * data sets whose frames carry no restart markers (Charades_v1_rgb), where one lane per restart interval means one lane per frame.
 * Huffman-coded data self-synchronises (Weissenberger & Schmidt, "Accelerating JPEG Decompression on GPUs"): a frame with restart
 * interval 0, more than `sub_bytes` bytes and at most `max_subs` subsequences of `sub_bytes` raw bytes is decoded by one workgroup,
 * one lane per subsequence: speculative decodes in rounds until no exit state changes (at most as many rounds as subsequences,
 * which always reaches the true states), a scan of block counts and DC sums, one write pass.  Every other frame of the batch
 * (restart markers, short, too many subsequences) is decoded one lane per restart interval by the same call.  Arguments, output,
 * status bits, workspace (cfn_jpeg_workspace_bytes: it does not grow, the per-subsequence records live in 32 * max_subs bytes of
 * LDS) and checks are those of cfn_jpeg_decode_u8; only the write pass sets status bits.  sub_bytes: a multiple of 4 in
 * [16, 1024], so that a symbol and its value (<= 31 bits, stuffing included) end inside the next subsequence; max_subs in
 * [1, 1536]; anything else returns 1 naming the argument.  3 memsets + 5 launches on `stream`.
 * ===================================================================================================================== */
int cfn_jpeg_decode_u8_sync(const unsigned char* data, const int* frames, const int* tables, const int* geom, const int* lengths,
                            unsigned char* out, int* status, void* ws, long ws_bytes, long data_bytes, int rows, int sets, int N,
                            int Tmax, int Hmax, int Wmax, int lanes, int blocks_max, int sub_bytes, int max_subs, void* stream);

/* =====================================================================================================================
 * Frame labels from annotation segments (csrc/seglabels.hip; the sample record and the batch type: cfn_hip/seglabels.py).
 * Replaces, on the GPU, the dense label array the reference builds per video in make_dataset (charades_fine.py:110-117,
 * the same loop in charades_coarse_fineFEAT.py:115-122), slices per sample in Charades.__getitem__ (charades_fine.py:149-165,
 * :188) and zero-pads per batch in mt_collate_fn (charades_fine.py:214-220) -- bit for bit.
 *   seg (n_seg, 3) fp64 rows [class, start_s, end_s]; offsets (B + 1) int32: video b owns rows offsets[b] .. offsets[b + 1] - 1;
 *   fps (B) fp64 = num_frames / duration as the host computed it; window (B, 2) int32 = first frame (start_f - 1), length.
 *     len = clamp(window[b, 1], 0, t_max),  fr = window[b, 0] + t
 *     labels[b, c, t] = t < len && exists (c, s, e) of video b: fr / fps[b] > s && fr / fps[b] < e   ? 1.0f : 0.0f     (B, C, t_max)
 *     mask[b, t]      = t < len ? 1.0f : 0.0f                                                                           (B, t_max)
 *     valid_t[b]      = len                                                                                             (B) int32
 *   fr / fps is one correctly rounded fp64 division and both inequalities are strict, as in the reference.  EVERY element of the
 *   three outputs is written.  Same-class segments may overlap, a video may own no row; rows no offset range covers are ignored.
 *   Everything but B, C, t_max and n_seg is read on the device only: an offset range is clamped to [0, n_seg], and a class that is
 *   not an integer of [0, C) selects no row (a bad batch gives wrong values, never a store outside the outputs).
 * One launch on `stream`, no allocation, no synchronisation (capturable); nothing accumulates, so the deterministic mode changes
 * nothing.  Returns 1 for null pointers, B, C or t_max < 1, n_seg < 0, B > 65535, C >= 2^19 or t_max >= 2^24.
 * ===================================================================================================================== */
int cfn_seg_labels(const double* seg, const int* offsets, const double* fps, const int* window, float* labels, float* mask,
                   int* valid_t, int B, int C, int t_max, long n_seg, void* stream);

/* =====================================================================================================================
 * Activity segments from per-frame scores (csrc/detections.hip; the batch type, the host reference and the writer:
 * cfn_hip/detections.py).  The reference stops at probs (B, C, TL) (train_fine.py:199-206, the same lines in
 * train_coarse_fineFEAT.py); this replaces the per-video Python decode every caller writes after them (threshold, find the
 * runs, frames -> seconds) by one device-side step, and is the inverse of cfn_seg_labels.
 *   probs (B, C, TL) fp32; valid_t (B) int32; fps (B) fp64; start (B) int32 = first frame of each window; thr (C) fp32.
 *     1. frame t of row (b, c) is active iff t < min(valid_t[b], TL) and probs[b, c, t] > thr[c] (strict: NaN is never active)
 *     2. active frames t < u with only inactive frames between them and u - t - 1 <= max_gap are joined
 *     3. a segment is a maximal run [t0, t1] after 2; runs with t1 - t0 + 1 < min_len are dropped
 *     4. start_s = ((double)(start[b] + t0) - 0.5) / fps[b], end_s = ((double)(start[b] + t1) + 0.5) / fps[b]  (IEEE fp64)
 *     5. max (fp32) and mean (fp64 sum in a fixed order / count, rounded to fp32) over the ACTIVE frames of the run only
 *     6. rows are ordered by (b, c, t0), through counts and prefix sums: no atomics, the same bits in every run
 *   seg (cap, 3) fp64 rows [class, start_s, end_s] (the layout of cfn_seg_labels' seg); frames (cap, 3) int32 [t0, t1, n_active];
 *   score (cap, 2) fp32 [max, mean]; offsets (B + 1) int32: sample b owns rows offsets[b] .. offsets[b + 1] - 1; total (1) int32 =
 *   offsets[B].  offsets and total are the TRUE counts, not clamped by cap; rows >= cap are not written, rows of the three
 *   buffers behind min(total, cap) are not touched.  cap = B * C * ((TL + 1) / 2) can never overflow.
 *   workspace: cfn_decode_segments_workspace_bytes(B, C, TL) bytes on an 8-byte boundary (the rows' bit masks, TL / 8 bytes per
 *   row, and B * C + 1 counts); the library keeps no state, the caller owns the buffer until the stream has passed.
 * Everything but B, C, TL, max_gap, min_len and cap is read on the device only.  3 launches on `stream` ordered by the stream
 * alone, no allocation, no synchronisation (capturable); nothing accumulates across workgroups, so the deterministic mode
 * changes nothing.  Returns 1 for null pointers, B, C or TL < 1, B > 65535, C >= 2^19, TL > 65536, B * C * TL >= 2^31,
 * max_gap < 0, min_len < 1, cap outside [1, 2^31) or a misaligned workspace; cfn_decode_segments_workspace_bytes -1 for the
 * same shapes.
 * ===================================================================================================================== */
long cfn_decode_segments_workspace_bytes(int B, int C, int TL);
int cfn_decode_segments(const float* probs, const int* valid_t, const double* fps, const int* start, const float* thr, double* seg,
                        int* frames, float* score, int* offsets, int* total, void* workspace, int B, int C, int TL, int max_gap,
                        int min_len, long cap, void* stream);

/* =====================================================================================================================
 * Activity proposals: candidates at K threshold levels, then temporal non-maximum suppression (csrc/detections.hip,
 * csrc/segnms.hip; the rules, the host references and propose(): cfn_hip/detections.py).
 * cfn_decode_segments_levels: cfn_decode_segments with levels (C, K) fp32, 1 <= K <= 16, in place of thr; row c holds class c's K
 * thresholds in the caller's order (they need not be sorted).
 *     L1. candidate row (b, c, k) is rules 1-5 above applied to probs[b, c, :] with the threshold levels[c, k]
 *     L2. the class column of seg holds c; level (cap) uint8 holds k
 *     L3. rows are ordered by (b, c, k, t0), through counts and prefix sums; offsets and total are TRUE counts, rows >= cap are
 *         not written
 *     L4. cap = B * C * K * ((TL + 1) / 2) can never overflow; K = 1 gives cfn_decode_segments' result bit for bit
 *   The candidates of a (video, class) group are contiguous and the class column does not decrease inside a video: all
 *   cfn_segap_match and cfn_nms_segments need.  workspace: cfn_decode_segments_levels_workspace_bytes(B, C, K, TL) bytes on an
 *   8-byte boundary.  3 launches.  Returns 1 as cfn_decode_segments does, and for K outside [1, 16], B * C * K * TL >= 2^31 or a null
 *   level; the workspace query -1 for the same shapes.
 * cfn_nms_segments: seg (cap_in, 3) fp64, frames (cap_in, 3) int32, score (cap_in, 2) fp32, offsets (B + 1) int32 grouped like that;
 * nms_thr a double of [0, 1]; score_col 0 = max, 1 = mean.
 *     N1. groups are (video, class) row ranges, found as cfn_segap_match finds them (offsets clamped to [0, cap_in])
 *     N2. order inside a group: score[:, score_col] descending (fp32), ties by row ascending; a NaN score ranks as -inf.  Nested
 *         candidates share their maximum, so with score_col = 0 the caller's LEVEL ORDER decides those ties
 *     N3. tIoU of (s0, e0) and (s1, e1): inter = min(e0, e1) - max(s0, s1); 0 unless inter > 0, otherwise
 *         inter / ((e0 - s0) + (e1 - s1) - inter): IEEE fp64, no product, one division
 *     N4. greedy in that order: a candidate is KEPT iff no candidate kept before it has tIoU with it > nms_thr (strict); a
 *         suppressed candidate suppresses nothing
 *     N5. stable compaction: kept rows in input order, out_seg / out_frames / out_score copied bit for bit; out_offsets (B + 1) and
 *         out_total (1) are TRUE counts; rows >= cap_out are not written
 *     N6. keep (cap_in) uint8, written for the rows of the batch's groups only; src (cap_out) int32 = the input row of each output row
 *     N7. nms_thr = 1 keeps everything; below 1 exact duplicates (tIoU exactly 1.0) collapse to the first in the order
 *   3 launches (select: one wave per group, O(nd^2 / 64) ranking and O(kept * nd / 64) suppression; groups of up to
 *   cfn_nms_det_tile() = 1024 candidates in LDS, larger ones through the workspace; scan; write).  workspace:
 *   cfn_nms_segments_workspace_bytes(B, C, cap_in) bytes on an 8-byte boundary.  The outputs must not be the inputs.
 * Both: everything but the shapes, score_col, nms_thr and the caps is read on the device only and clamped: a bad batch gives wrong
 * values, never a store outside the outputs.  Ordered by the stream alone, no atomics, no allocation, no synchronisation
 * (capturable).  cfn_nms_segments returns 1 for null pointers, B or C outside [1, 65535], cap_in or cap_out outside [1, 2^31),
 * score_col outside {0, 1}, nms_thr outside [0, 1] (a NaN included), a misaligned workspace or an output that is an input.
 * cfn_soft_nms_segments: soft-NMS over the same inputs and outputs.  Nothing is deleted by overlap: a candidate's score is decayed by
 * its overlap with every candidate ranked in front of it, and the list is cut by a score floor or a count.  Host parameters beside
 * cfn_nms_segments': method 0 = linear, 1 = gaussian; nms_thr in [0, 1] (linear only); sigma in [1/64, 2^20] (gaussian only);
 * min_score in [0, 1]; max_keep >= 0 (0 = no limit).
 *     S1. groups are rule N1's
 *     S2. row i gets w_i = (double)score[i, score_col]; a row whose score is NaN or infinite is out of the group from the start: never
 *         selected, never decayed, keep 0
 *     S3. rounds: among the rows not yet selected m = the one with the largest w, ties to the lowest row.  Stop when no row is left,
 *         when !(w_m >= min_score), or when max_keep > 0 and max_keep rows are selected; otherwise m is selected, final_m = w_m.
 *         Selected finals never increase: the selected set is the rows whose final is at least min_score, cut at max_keep
 *     S4. decay of every row j not yet selected, iou = tIoU(m, j) by rule N3 unchanged.  linear: if iou > nms_thr (strict)
 *         w_j = w_j * (1.0 - iou).  gaussian: if iou > 0, w_j = w_j * E((iou * iou) / sigma).  One fp64 subtraction or one E, then
 *         one fp64 product; the decays are applied in selection order
 *     S5. E(t) = exp(-t) for t in [0, 64], spelled so that device and host compute the same double: y = -(t * 2^-10); p = c8, then
 *         p = p * y + c_k for k = 7 .. 0 with c_k = 1.0 / k! (one IEEE fp64 division each); then p = p * p ten times.  Every product
 *         and sum is rounded separately (no fused multiply-add); fp64 subnormals follow IEEE.  Within 1.6e-13 relative of exp(-t),
 *         E(0) = 1.0 exactly
 *     S6. stable compaction of the selected rows in input order: out_seg, out_frames and the other score column copied bit for
 *         bit, out_score[:, score_col] = (float)final (round to nearest); out_offsets and out_total are TRUE counts; rows >= cap_out
 *         are not written; keep (cap_in) uint8 and src (cap_out) int32 as in N6
 *     S7. linear with nms_thr = 1, min_score = 0, max_keep = 0 returns its input bit for bit; a single-level decode passes through
 *         either method unchanged when min_score is not above its scores; max_keep = 1 leaves each group's first row in the order
 *         of N2; the first selected row of every group is cfn_nms_segments' first kept row
 *   3 launches (soft_select: one wave per group, candidate j owned by lane j & 63, a round = per-lane maximum, wave reduction of the
 *   (w, row) pair, decay of the own entries: O(selected * nd / 64), no barrier, fence or atomic inside the rounds; groups of up to
 *   cfn_nms_det_tile() candidates in LDS, larger ones keep w in the workspace; cfn_nms_segments' scan; a write that takes column
 *   score_col from the finals).  workspace: cfn_soft_nms_segments_workspace_bytes(B, C, cap_in) bytes on an 8-byte boundary (8 + 4
 *   bytes per input row and B * C + 1 counts).  Clamped, ordered by the stream alone, no allocation, no synchronisation (capturable)
 *   like cfn_nms_segments.  Returns 1 for everything cfn_nms_segments refuses, and for method outside {0, 1}, sigma outside
 *   [1/64, 2^20], min_score outside [0, 1] (NaNs included) or max_keep < 0; the workspace query -1 for cfn_nms_segments' shapes.
 * ===================================================================================================================== */
long cfn_decode_segments_levels_workspace_bytes(int B, int C, int K, int TL);
int cfn_decode_segments_levels(const float* probs, const int* valid_t, const double* fps, const int* start, const float* levels,
                               double* seg, int* frames, float* score, unsigned char* level, int* offsets, int* total,
                               void* workspace, int B, int C, int K, int TL, int max_gap, int min_len, long cap, void* stream);
long cfn_nms_segments_workspace_bytes(int B, int C, long cap_in);
int cfn_nms_det_tile(void);
int cfn_nms_segments(const double* seg, const int* frames, const float* score, const int* offsets, double* out_seg, int* out_frames,
                     float* out_score, int* out_offsets, int* out_total, unsigned char* keep, int* src, void* workspace, int B,
                     int C, int score_col, double nms_thr, long cap_in, long cap_out, void* stream);
long cfn_soft_nms_segments_workspace_bytes(int B, int C, long cap_in);
int cfn_soft_nms_segments(const double* seg, const int* frames, const float* score, const int* offsets, double* out_seg, int* out_frames,
                          float* out_score, int* out_offsets, int* out_total, unsigned char* keep, int* src, void* workspace, int B,
                          int C, int score_col, double nms_thr, int method, double sigma, double min_score, int max_keep, long cap_in,
                          long cap_out, void* stream);

/* =====================================================================================================================
 * Temporal filtering of per-frame scores in front of the decode (csrc/scorefilter.hip; the rule, the numpy reference and the
 * ScoreFilter type: cfn_hip/scorefilter.py).  Raw sigmoid scores flicker from frame to frame and rule 1 of cfn_decode_segments
 * then breaks one activity into many runs; this is the box, Gaussian or median filter a caller would otherwise write in torch
 * with an edge rule of their own.  probs (B, C, TL) fp32; valid_t (B) int32; radius (C) int32; weights (C, R + 1) fp64; host ints
 * R in [0, 32] (windows of at most 65 frames) and method (0 = weighted mean, 1 = median) -> out (B, C, TL) fp32, not probs.
 *     F1. n = min(max(valid_t[b], 0), TL), r = min(max(radius[c], 0), R).  Frames t >= n are copied from probs bit for bit; r = 0
 *         copies every frame bit for bit, under either method
 *     F2. the window of frame t < n is u in [max(0, t - r), min(n - 1, t + r)]: truncated at the valid range, no padding, no
 *         reflection
 *     F3. a window that holds a non-finite value gives the canonical quiet NaN 0x7fc00000 (cfn_decode_segments never activates
 *         such a frame); so does a weighted mean whose quotient is a NaN (weights other than the documented table)
 *     F4. weighted mean, u ascending throughout: num = the sum of weights[c, |u - t|] * (double)probs[b, c, u], den = the sum of
 *         weights[c, |u - t|], both from 0.0; every product and every sum is rounded separately (no fused multiply-add); then ONE
 *         IEEE fp64 division and ONE rounding to fp32.  The box filter is the table of ones; a Gaussian table is made on the HOST
 *         (exp(-d * d / (2 sigma^2)), weights[c, 0] == 1.0), so no device exp is involved.  Weights are expected finite and
 *         non-negative with weights[c, 0] > 0
 *     F5. median: the window ordered by (value, u): rank(u) = #{v : p[v] < p[u] or (p[v] == p[u] and v < u)}, a stable sort, so
 *         +0 / -0 ties are decided.  m window frames, m odd: the element of rank (m - 1) / 2; m even:
 *         (float)(((double)a + (double)b) * 0.5) with a, b the elements of ranks m / 2 - 1 and m / 2
 *     F6. no atomics, nothing is read back: the same bits in every run
 *   1 launch, grid (tile of cfn_score_filter_tile() = 256 frames, class, video), one thread per frame; the tile, a halo of 32
 *   frames on each side and the class's weight row are staged in LDS by bounds-checked loads that never leave row (b, c).  The
 *   median ranks by counting over the LDS window: O(window^2) per frame.  valid_t, radius and weights are read on the device
 *   only and the first two are clamped: a bad batch gives wrong values, never an access outside the buffers.  No allocation, no
 *   synchronisation (capturable); nothing accumulates across threads, so the deterministic mode changes nothing.
 * Returns 1 for null pointers, B or C outside [1, 65535], TL outside [1, 65536], R outside [0, 32], method outside {0, 1} or
 * out == probs.
 * ===================================================================================================================== */
int cfn_score_filter_tile(void);
int cfn_score_filter(const float* probs, const int* valid_t, const int* radius, const double* weights, float* out, int B, int C,
                     int TL, int R, int method, void* stream);

/* =====================================================================================================================
 * Segment-level average precision at temporal-IoU thresholds (csrc/segap.hip; the host reference and the meter:
 * cfn_hip/segap.py).  The first consumer of the pair cfn_seg_labels' seg / cfn_decode_segments' seg; the reference stops at probs
 * (train_fine.py:199-222), so the rule is stated here once:
 *   detections det_seg (det_cap, 3) fp64, det_score (det_cap, 2) fp32, det_offsets (B + 1) int32 (cfn_decode_segments' outputs);
 *   ground truth seg (n_seg, 3) fp64, offsets (B + 1) int32, fps (B) fp64, window (B, 2) int32 (cfn_seg_labels' inputs);
 *   tiou (n_thr) fp64, 1 <= n_thr <= 8, each in (0, 1]; score_col 0 = max, 1 = mean.
 *     1. n = clamp(window[b,1], 0, t_max), w0 = ((double)window[b,0] - 0.5) / fps[b], w1 = ((double)(window[b,0] + n) - 0.5) / fps[b]
 *        (the extent cfn_decode_segments gives a detection over the whole window); s' = max(s, w0), e' = min(e, w1) (a NaN bound
 *        gives way to the window's).  A row PARTICIPATES iff n > 0, its class is an integer of [0, C) and e' > s'.  n_gt[c] counts
 *        participating rows.
 *     2. tIoU of (sd, ed) and (s', e'): inter = min(ed, e') - max(sd, s'); 0 unless inter > 0, otherwise
 *        inter / ((ed - sd) + (e' - s') - inter): IEEE fp64, no product, one division.
 *     3. within a (video, class) group the detections are taken by det_score[:, score_col] descending (fp32), ties by row ascending.
 *     4. greedy, independently per threshold k: a detection takes the participating row of its video and class that is not used up
 *        at k with the largest tIoU among those with tIoU >= tiou[k]; ties go to the lowest row.  It is then a true positive at k
 *        and the row is used up at k; otherwise a false positive.
 *     5. tp (det_cap) uint8: bit k = true positive at k; match (n_thr, det_cap) int32 or NULL: the row index or -1.  Only the rows
 *        of the batch's detections are written.
 *     6. class c's store receives the batch's detections of class c in (video, row) order behind the rows it holds: scores (C, cap)
 *        fp32 and tps (C, cap) uint8, class major; counts (C) and n_gt (C) int32 advance.  A batch that would push ANY class past
 *        cap writes nothing, changes no count and sets bit 1 of flags (cfn_ap_append's rule).
 *     7. cfn_ap_sort_counts: cfn_ap_sort (stable, descending, its order of special values) with one count per class, the tp byte as
 *        the payload.  ap (n_thr, C) fp32: ap[k, c] = (sum over the ranks r whose bit k is set of tp_cum_r / r) / n_gt[c], fp64 in a
 *        fixed order, 0 where n_gt[c] == 0; map (n_thr) fp32 = the mean over the classes with n_gt > 0, fp64 in class order.
 *   cfn_segap_match (1 launch, one wave per (video, class)): rules 1-5; leaves the groups' ranges and counts in `workspace`
 *     (cfn_segap_workspace_bytes(B, C, det_cap, n_seg) bytes on an 8-byte boundary; the caller owns it until cfn_segap_append of
 *     the same batch has passed on the stream).  Lanes hold ground-truth rows, cfn_segap_gt_tile() = 64 per tile; the score order
 *     of a group lives in LDS up to cfn_segap_det_tile() = 1024 detections; larger videos / groups take a general path through
 *     the workspace, so no size is undefined.  The order is rank by counting: O(nd^2 / 64) per group of nd detections.
 *   cfn_segap_append (2 launches): rule 6 from the workspace cfn_segap_match left.
 *   cfn_segap_reduce (2 launches): rule 7 behind cfn_ap_sort_counts.
 * Everything but B, C, t_max, n_thr, score_col, det_cap, n_seg and cap is read on the device only and clamped: a bad batch gives
 * wrong values, never a store outside the outputs.  Ordered by the stream alone; no allocation, no synchronisation (capturable);
 * nothing accumulates in floating point across workgroups.  Return 1 for null pointers (match may be NULL), B or C outside
 * [1, 65535], t_max < 1, n_thr outside [1, 8], score_col outside {0, 1}, det_cap, n_seg or cap outside [1, 2^31) (the sort:
 * cap < 2^31 less one tile) or a misaligned workspace; cfn_segap_workspace_bytes -1 for the same shapes.
 * ===================================================================================================================== */
long cfn_segap_workspace_bytes(int B, int C, long det_cap, long n_seg);
int cfn_segap_gt_tile(void);
int cfn_segap_det_tile(void);
int cfn_segap_match(const double* det_seg, const float* det_score, const int* det_offsets, const double* seg, const int* offsets,
                    const double* fps, const int* window, const double* tiou, unsigned char* tp, int* match, void* workspace, int B,
                    int C, int t_max, int n_thr, int score_col, long det_cap, long n_seg, void* stream);
int cfn_segap_append(const float* det_score, const unsigned char* tp, void* workspace, float* scores, unsigned char* tps,
                     int* counts, int* n_gt, int* flags, int B, int C, int score_col, long det_cap, long cap, void* stream);
int cfn_ap_sort_counts(const float* scores, const unsigned char* targets, const int* counts, float* sorted_scores,
                       unsigned char* sorted_targets, int* tmp_keys, unsigned char* tmp_targets, int K, long cap, void* stream);
int cfn_segap_reduce(const unsigned char* sorted_tps, const int* counts, const int* n_gt, float* ap, float* map, int C, int n_thr,
                     long cap, void* stream);

/* =====================================================================================================================
 * Per-class decode thresholds calibrated from the sorted AP rows (csrc/apcal.hip; the rule, the numpy reference and the
 * Calibration that owns the tensors: cfn_hip/calibrate.py).  The thresholds cfn_decode_segments (thr (C)) and
 * cfn_decode_segments_levels (levels (C, K)) take are typed constants otherwise; here they come from the rows cfn_ap_sort left:
 *   sorted_scores (C, cap) fp32 descending and canonical (NaN last, -inf just in front), sorted_targets (C, cap) uint8 (positive
 *   iff != 0), count ONE int on the device; per class the first n = clamp(count, 0, cap) rows.  kinds (K) int32 and values (K)
 *   fp64 on the DEVICE, 1 <= K <= 16: kind 0 = f1 (value unused), 1 = precision p, 2 = recall q, p and q in (0, 1].
 *     1. P = positives among the n rows; m = rows with score > -inf (fp32 compare, a NaN fails): a prefix.  Rows behind m can never
 *        be active under the decode's strict probs > thr; their positives still count in P.
 *     2. tp(r) = positives among rows 0 .. r - 1, tp(0) = 0.
 *     3. a cut r of 1 .. m is ADMISSIBLE iff r == m or score[r - 1] > score[r] (strict): a threshold cannot separate equal scores.
 *     4. f1: over r = 0 and the admissible cuts, maximise 2 tp(r) / (r + P), compared EXACTLY in unsigned 64-bit integers: a beats b
 *        iff tp(a) * (b + P) > tp(b) * (a + P); start from r = 0, replace on strict improvement only (ties: the smallest r).
 *        precision p: the LARGEST admissible r with (double)tp(r) >= p * (double)r (one fp64 multiply, one compare); none: r = 0.
 *        recall q: P == 0 gives r = 0; otherwise the SMALLEST admissible r with (double)tp(r) >= q * (double)P; none (positives
 *        behind m): r = m.
 *        ok[c, k] = 1 iff the criterion was met: f1: tp > 0; precision, recall: the inequality holds at the returned r > 0.
 *     5. the threshold of a cut: r == 0: +inf; 0 < r < m: score[r], the largest score NOT taken, so the decode's strict rule
 *        activates exactly rows 0 .. r - 1 of the calibration data; r == m > 0: -inf.
 *     6. thr (C, K) fp32 (the layout of levels; K = 1: a contiguous (C) thr), cut (C, K) int32, tp (C, K) int32, ok (C, K) uint8,
 *        stat (C, 2) int32 = [P, m].
 *   Recall criteria listed with ascending q give non-increasing thresholds: the high-to-low level order of rule N2.
 * cfn_ap_calibrate: 1 launch, one workgroup per class; two walks (P and m; then the rows in front of m in tiles of
 *   cfn_ap_calibrate_tile() rows with the running tp of cfn_ap_reduce's scan, every criterion against the tile's admissible cuts);
 *   one fixed-shape reduction per criterion (argmax with ties to the smaller r, max, min: independent of the order).  count, kinds
 *   and values are read on the device only and clamped: an unknown kind or a value outside (0, 1] gives r = 0, ok = 0; every
 *   output index is in range by construction.  No atomics, no floating-point accumulation, no allocation, no synchronisation
 *   (capturable); bit-identical from run to run.  16-byte loads where a class row is aligned, scalar loads otherwise (odd cap).
 * Returns 1 for null pointers, C outside [1, 65535], K outside [1, 16], cap outside [1, 2^31).
 * ===================================================================================================================== */
int cfn_ap_calibrate(const float* sorted_scores, const unsigned char* sorted_targets, const int* count, const int* kinds,
                     const double* values, float* thr, int* cut, int* tp, unsigned char* ok, int* stat, int C, int K, long cap,
                     void* stream);
int cfn_ap_calibrate_tile(void);

/* =====================================================================================================================
 * Proposal recall at N per video, AR@N (csrc/segrecall.hip; the rule, the numpy reference and the meter: cfn_hip/recall.py).
 * How many ground-truth segments at least one of the N best candidates of their video covers at a tIoU threshold: what a
 * proposal stage (cfn_decode_segments_levels, cfn_nms_segments, cfn_soft_nms_segments) is judged by.  Inputs as cfn_segap_match
 * takes them: det_seg (det_cap, 3) fp64, det_score (det_cap, 2) fp32, det_offsets (B + 1) int32; seg (n_seg, 3) fp64, offsets
 * (B + 1) int32, fps (B) fp64, window (B, 2) int32, t_max; tiou (n_thr) fp64 on the device, 1 <= n_thr <= 16, each in (0, 1], any
 * order; n_max in [1, 1024]; score_col 0 = max, 1 = mean.
 *     R1. participation and window clip: rule 1 of segment AP above, to the bit.  Row g belongs to video b iff offsets[b] <= g <
 *         offsets[b + 1] (clamped to [0, n_seg], expected not to decrease; found by binary search).
 *     R2. tIoU: rule 2 of segment AP.
 *     R3. video rank: the candidates of video b are the rows det_offsets[b] .. det_offsets[b + 1], clamped to [0, det_cap], ALL
 *         classes together, ranked by det_score[:, score_col] descending (fp32), a NaN taken as -inf, ties to the lower row: a
 *         permutation of 0 .. n_b - 1.
 *     R4. first hit: for a participating row g (video b, class c) and threshold k, hit[k, g] = the smallest video rank among the
 *         candidates of the SAME video and class whose tIoU with g is > 0 and >= tiou[k]; n_max when there is none or the smallest
 *         is >= n_max; -1 for a row that does not participate.  No one-to-one matching.
 *     R5. state: int64 hist (n_thr, n_max), then n_gt, n_videos, n_props (n_thr * n_max + 3 values).  hist[k, hit[k, g]] += 1 for
 *         every participating g with hit < n_max; n_gt += the participating rows; n_videos += B; n_props += the sum of the clamped
 *         n_b.  Integer adds only: the same in every run, and additive over batches and over data-parallel ranks.
 *     R6. value, fp64: recall[k, n] = (double)(hist[k, 0] + .. + hist[k, n]) / (double)n_gt (N = n + 1; 0 when n_gt == 0);
 *         ar[n] = (recall[0, n] + .. + recall[n_thr - 1, n]) / n_thr in k order; auc = (ar[0] + .. + ar[n_max - 1]) / n_max in n
 *         order; avg_props = n_props / n_videos (0 without videos).  No product: bit-equal to the numpy reference.
 *   cfn_seg_recall_add (3 launches): R1-R5.  hit (n_thr, n_seg) int32 is written whole; state advances in place; `workspace`:
 *     cfn_seg_recall_workspace_bytes(B, C, det_cap, n_seg, n_thr) bytes on an 8-byte boundary (the video ranks).  The rank is by
 *     counting through LDS tiles of cfn_seg_recall_rank_tile() = 256 scores, a grid over (tile of rows, video): O(n_b^2) per video.
 *     The first hit takes one wave per ground-truth row; the histogram one workgroup per threshold (LDS integer atomics).
 *   cfn_seg_recall_value (1 launch): R6 into out (n_thr * n_max + n_max + 2) fp64: recall, ar, auc, avg_props.
 * Everything but the host ints is read on the device only and clamped: a bad batch gives wrong values, never an access outside
 * the buffers.  Ordered by the stream alone; no allocation, no synchronisation (capturable).  Return 1 for null pointers, B or C
 * outside [1, 65535], t_max < 1, n_thr outside [1, 16], n_max outside [1, 1024], score_col outside {0, 1}, det_cap or n_seg outside
 * [1, 2^31) or a misaligned workspace; cfn_seg_recall_workspace_bytes -1 for the same shapes and n_thr.
 * ===================================================================================================================== */
long cfn_seg_recall_workspace_bytes(int B, int C, long det_cap, long n_seg, int n_thr);
int cfn_seg_recall_rank_tile(void);
int cfn_seg_recall_add(const double* det_seg, const float* det_score, const int* det_offsets, const double* seg, const int* offsets,
                       const double* fps, const int* window, const double* tiou, int* hit, long* state, void* workspace, int B, int C,
                       int t_max, int n_thr, int n_max, int score_col, long det_cap, long n_seg, void* stream);
int cfn_seg_recall_value(const long* state, double* out, int n_thr, int n_max, void* stream);

/* =====================================================================================================================
 * Merge class-major AP stores (csrc/apmerge.hip; the rule, the numpy reference, the gather over data-parallel ranks:
 * cfn_hip/apmerge.py).  cfn_ap_append's stores (ONE count for all classes) and cfn_segap_append's (one count per class plus
 * n_gt) share one layout; AP is not additive, but the sort behind it is stable and breaks ties in insertion order, so stores
 * appended in a FIXED order give every rank the bits one process would have produced, fed the parts' batches one part after
 * another.
 *   destination: scores (C, cap_d) fp32, payload (C, cap_d) uint8, counts (n_cnt) int32 with n_cnt == 1 (one count for all
 *     classes) or C, extra (n_extra) int32 (additive integers carried along: n_gt; NULL with n_extra == 0), ONE flags word.
 *   sources: R >= 1 parts in one call: scores (R, C, cap_s), payload (R, C, cap_s), counts (R, n_cnt), extra (R, n_extra),
 *     flags (R).  Sources and destination do not overlap.
 *     M1. a source count outside [0, cap_s] makes the call a refusal: nothing is written, no count or extra changes, and flag
 *         bit 2 (value 4, "malformed source") is set.
 *     M2. totals in 64-bit integers: tot[c] = counts_d[c] + sum_r counts_s[r][c].  Any tot[c] > cap_d (or a destination count
 *         below 0) is a refusal: nothing is written, nothing changes, the overflow bit (value 2, cfn_ap_append's) is set.  Any
 *         summed extra that leaves int32 is a refusal in the same way.  All or nothing, as cfn_ap_append.
 *     M3. otherwise row i of part r, class c goes to destination row counts_d[c] + sum_{q<r} counts_s[q][c] + i.  Scores and
 *         payload are copied as BITS (NaN payloads, -0.0 and denormals stay as they are); counts and extras advance by the
 *         sums; rows behind the new counts are untouched.
 *     M4. in every case, refusals included, flags |= OR_r flags_s[r]: a batch dropped on any rank taints the merged value.
 * cfn_ap_merge: 2 launches.  plan (one workgroup) validates, takes the per-count prefix sums over the parts into `workspace`
 *   (cfn_ap_merge_workspace_bytes(R, C) bytes on an 8-byte boundary, caller owned until the call has passed on the stream),
 *   decides refusal and commits counts, extras and flags.  copy: a grid over (tile of cfn_ap_merge_tile() = 2048 rows of cap_s,
 *   class, part) that reads only the workspace's verdict, bases and counts, never the destination counts; tiles behind a
 *   part's count exit, so no grid size depends on a device value.  Scores go as dwords, as 16-byte vectors where both sides
 *   share their phase; the payload is right at every (source, destination) byte alignment: head and tail bytes singly, the
 *   body as destination-aligned dwords assembled from the source, and nothing outside a tile's source rows is read.
 * Ordered by the stream alone; no atomics, no allocation, no synchronisation, no read-back (capturable).  Counts are DATA:
 * what plan leaves in the workspace is clamped where copy reads it, so nothing is stored outside the destination.  Returns
 * 1 for null pointers (the extras may be NULL with n_extra == 0), C or R outside [1, 65535], cap_s or cap_d outside
 * [1, 2^31), n_cnt not in {1, C}, n_extra < 0, or a misaligned workspace; cfn_ap_merge_workspace_bytes -1 for such R or C.
 * ===================================================================================================================== */
long cfn_ap_merge_workspace_bytes(int R, int C);
int cfn_ap_merge_tile(void);
int cfn_ap_merge(float* dst_scores, unsigned char* dst_payload, int* dst_counts, int* dst_extra, int* dst_flags,
                 const float* src_scores, const unsigned char* src_payload, const int* src_counts, const int* src_extra,
                 const int* src_flags, void* workspace, int R, int C, int n_cnt, int n_extra, long cap_s, long cap_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
