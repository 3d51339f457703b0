// hipcc-flags: -fno-slp-vectorize
// (packed fp32 arithmetic behind an LDS read is the documented hazard of this tree; nothing here needs packed math)
//
// Detection loss of train_fine.py:199-213 / train_coarse_fineFEAT.py:226-240 as ONE forward and ONE backward kernel:
//
//     logits (B*n, C, T) --linear resize to TL--> sigmoid --max over the n crops--> * masks (B, TL) = probs (B, C, TL)
//     cls = BCE(max_t probs, max_t labels)  (mean over B*C)          loc = sum BCE(probs, labels) / norm * world
//
// The composed path runs this as ~20 ATen launches over (B, C, TL) fp32 intermediates that autograd keeps alive; here a workgroup owns one
// (b, c) row, keeps its n*T logits in LDS, and touches HBM for `labels` (read), `masks` (read) and `probs` (one optional write).  The backward
// recomputes z, s and p from the logits: nothing of size (B, C, TL) is saved.
//
// Numerics follow ATen: sigmoid = 1 / (1 + exp(-z)) in fp32, p = s * mask rounded to fp32, BCE evaluated ON p with both logs clamped at -100
// (not a softplus of z: with saturated logits p is exactly 0 or 1 and the clamp is what the reference computes), BCE backward with the
// 1e-12 floor under p (1 - p).  Sums run in fp64 in a fixed order (no atomics): two runs give the same bits.
#include "cfn_common.h"
#include "resize_src.h"

extern __shared__ __attribute__((aligned(16))) unsigned char dl_smem[];

namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_JT = 2048;          // backward: frames of the resized row staged in LDS per pass
constexpr int DL_MAX_ROW = 6144;     // n * T logits of one (b, c) row kept in LDS (24 KB; backward: a second array of that size)
constexpr int DL_RED_BYTES = 96;     // reduction scratch in front of the row (a multiple of 16: the row stays 16-byte aligned)

__device__ __forceinline__ float dl_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// -(y log p + (1 - y) log(1 - p)), logs clamped at -100 (ATen binary_cross_entropy), on the fp32 value p; the products in fp64
__device__ __forceinline__ double dl_bce(float p, float y) {
    const float lp = fmaxf(logf(p), -100.0f), lq = fmaxf(log1pf(-p), -100.0f);
    return -((double)y * (double)lp + (1.0 - (double)y) * (double)lq);
}

// d BCE / dp without the upstream factor (ATen binary_cross_entropy_backward)
__device__ __forceinline__ float dl_bce_grad(float p, float y) { return (p - y) / fmaxf((1.0f - p) * p, 1e-12f); }

// the n*T logits of row (b, c) -> LDS, crop-major
__device__ __forceinline__ void dl_load_row(const float* __restrict__ x, float* xs, int b, int c, int C, int T, int n) {
    for (int e = threadIdx.x; e < n * T; e += DL_THREADS) {
        const int i = e / T, k = e - i * T;
        xs[e] = x[(((long)b * n + i) * C + c) * T + k];
    }
}

// s = max_i sigmoid(l0 x_i[i0] + l1 x_i[i1]); the lowest crop index wins a tie
__device__ __forceinline__ float dl_prob(const float* xs, int T, int n, int i0, int i1, float l0, float l1, int& win) {
    float s = dl_sigmoid(l0 * xs[i0] + l1 * xs[i1]);
    win = 0;
    for (int i = 1; i < n; ++i) {
        const float si = dl_sigmoid(l0 * xs[i * T + i0] + l1 * xs[i * T + i1]);
        if (si > s) { s = si; win = i; }
    }
    return s;
}

// one workgroup per (b, c) row.  rows: [0, BC) loc partials, [BC, 2 BC) cls terms
__global__ __launch_bounds__(DL_THREADS) void detloss_fwd_kernel(const float* __restrict__ x, const float* __restrict__ labels,
                                                                 const float* __restrict__ masks, float* __restrict__ probs,
                                                                 double* __restrict__ rows, int* __restrict__ jstar,
                                                                 float* __restrict__ ymax, int BC, int C, int T, int TL, int n, int ac) {
    double* red_d = (double*)dl_smem;                     // [DL_WAVES]
    float* red_p = (float*)(dl_smem + 32);                // [DL_WAVES]
    int* red_j = (int*)(dl_smem + 48);                    // [DL_WAVES]
    float* red_y = (float*)(dl_smem + 64);                // [DL_WAVES]
    float* xs = (float*)(dl_smem + DL_RED_BYTES);         // [n * T]
    const int row = blockIdx.x, b = row / C, c = row - b * C, tid = threadIdx.x;
    dl_load_row(x, xs, b, c, C, T, n);
    __syncthreads();
    const float* yr = labels + (long)row * TL;
    const float* mr = masks + (long)b * TL;
    float* pr = probs ? probs + (long)row * TL : nullptr;
    double acc = 0.0;
    float pm = -INFINITY, ym = -INFINITY;
    int pj = 0x7fffffff;
    for (int j = tid; j < TL; j += DL_THREADS) {
        int i0, i1, win; float l0, l1;
        resize_src(j, T, TL, ac, i0, i1, l0, l1);
        const float p = dl_prob(xs, T, n, i0, i1, l0, l1, win) * mr[j];
        const float y = yr[j];
        if (pr) pr[j] = p;
        acc += dl_bce(p, y);
        if (p > pm) { pm = p; pj = j; }      // j ascends: the first maximal frame of this thread
        ym = fmaxf(ym, y);
    }
    // fixed-order reduction: xor tree inside a wave, the waves in index order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        const float op = __shfl_xor(pm, o, 64);
        const int oj = __shfl_xor(pj, o, 64);
        if (op > pm || (op == pm && oj < pj)) { pm = op; pj = oj; }
        ym = fmaxf(ym, __shfl_xor(ym, o, 64));
    }
    if ((tid & 63) == 0) { red_d[tid >> 6] = acc; red_p[tid >> 6] = pm; red_j[tid >> 6] = pj; red_y[tid >> 6] = ym; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DL_WAVES; ++w) {
            acc += red_d[w];
            if (red_p[w] > pm || (red_p[w] == pm && red_j[w] < pj)) { pm = red_p[w]; pj = red_j[w]; }
            ym = fmaxf(ym, red_y[w]);
        }
        if (pj >= TL) pj = 0;                // (a row of NaNs: keep the index inside the row)
        rows[row] = acc;
        rows[BC + row] = dl_bce(pm, ym);
        jstar[row] = pj;
        ymax[row] = ym;
    }
}

// one workgroup: cls = sum(cls rows) / BC, loc = sum(loc rows) / norm * world; norm = *norm_in, or C * sum(masks) when norm_in is null.
// Every thread adds a contiguous run of rows in index order (masks: a fixed stride), then the fixed tree of the forward kernel.
__global__ __launch_bounds__(DL_THREADS) void detloss_fin_kernel(const double* __restrict__ rows, const float* __restrict__ masks,
                                                                 const float* __restrict__ norm_in, double world, float* __restrict__ cls,
                                                                 float* __restrict__ loc, double* __restrict__ norm_used, int BC, int C,
                                                                 long BTL) {
    double* red = (double*)dl_smem;          // [3][DL_WAVES]
    const int tid = threadIdx.x;
    const int chunk = (BC + DL_THREADS - 1) / DL_THREADS;
    const int lo = tid * chunk < BC ? tid * chunk : BC, hi = lo + chunk < BC ? lo + chunk : BC;
    double sl = 0.0, sc = 0.0, sm = 0.0;
    for (int r = lo; r < hi; ++r) { sl += rows[r]; sc += rows[BC + r]; }
    if (!norm_in)
        for (long e = tid; e < BTL; e += DL_THREADS) sm += (double)masks[e];
    sl = cfn_wave_sum_d(sl); sc = cfn_wave_sum_d(sc); sm = cfn_wave_sum_d(sm);
    if ((tid & 63) == 0) { red[tid >> 6] = sl; red[DL_WAVES + (tid >> 6)] = sc; red[2 * DL_WAVES + (tid >> 6)] = sm; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DL_WAVES; ++w) { sl += red[w]; sc += red[DL_WAVES + w]; sm += red[2 * DL_WAVES + w]; }
        const double nrm = norm_in ? (double)*norm_in : (double)C * sm;
        *norm_used = nrm;
        *cls = (float)(sc / (double)BC);
        *loc = (float)(sl / nrm * world);
    }
}

// one workgroup per (b, c) row: recomputes p per frame, forms gz (the gradient at the winning crop's resized logit) for DL_JT frames at a time
// in LDS, and gathers the transposed resize gx[k] = sum_j w_jk gz_j in ascending j into an LDS accumulator per (crop, k)
__global__ __launch_bounds__(DL_THREADS) void detloss_bwd_kernel(const float* __restrict__ g_cls, const float* __restrict__ g_loc,
                                                                 const float* __restrict__ x, const float* __restrict__ labels,
                                                                 const float* __restrict__ masks, const int* __restrict__ jstar,
                                                                 const float* __restrict__ ymax, const double* __restrict__ norm_used,
                                                                 double world, float* __restrict__ gx, int BC, int C, int T, int TL, int n,
                                                                 int ac, int JT) {
    float* xs = (float*)dl_smem;             // [n * T] logits
    float* ga = xs + n * T;                  // [n * T] gradient accumulators
    float* gz = ga + n * T;                  // [JT]
    int* wn = (int*)(gz + JT);               // [JT] winning crop
    const int row = blockIdx.x, b = row / C, c = row - b * C, tid = threadIdx.x;
    dl_load_row(x, xs, b, c, C, T, n);
    for (int e = tid; e < n * T; e += DL_THREADS) ga[e] = 0.0f;
    const float a_loc = (float)((double)*g_loc * world / *norm_used);
    const float a_cls = (float)((double)*g_cls / (double)BC);
    const int js = jstar[row];
    const float ym = ymax[row];
    const float* yr = labels + (long)row * TL;
    const float* mr = masks + (long)b * TL;
    __syncthreads();
    for (int t0 = 0; t0 < TL; t0 += JT) {
        const int tn = TL - t0 < JT ? TL - t0 : JT;
        for (int jl = tid; jl < tn; jl += DL_THREADS) {
            const int j = t0 + jl;
            int i0, i1, win; float l0, l1;
            resize_src(j, T, TL, ac, i0, i1, l0, l1);
            const float s = dl_prob(xs, T, n, i0, i1, l0, l1, win);
            const float m = mr[j];
            const float p = s * m;
            float gp = a_loc * dl_bce_grad(p, yr[j]);
            if (j == js) gp += a_cls * dl_bce_grad(p, ym);
            gz[jl] = (gp * m) * ((1.0f - s) * s);
            wn[jl] = win;
        }
        __syncthreads();
        for (int e = tid; e < n * T; e += DL_THREADS) {
            const int i = e / T, k = e - i * T;
            int jlo, jhi;
            resize_gather_range(k, T, TL, ac, jlo, jhi);
            if (jlo < t0) jlo = t0;
            if (jhi > t0 + tn - 1) jhi = t0 + tn - 1;
            float a = ga[e];
            for (int j = jlo; j <= jhi; ++j) {
                int i0, i1; float l0, l1;
                resize_src(j, T, TL, ac, i0, i1, l0, l1);
                if ((i0 != k && i1 != k) || wn[j - t0] != i) continue;
                const float gv = gz[j - t0];
                if (i0 == k) a = fmaf(gv, l0, a);
                if (i1 == k) a = fmaf(gv, l1, a);
            }
            ga[e] = a;
        }
        __syncthreads();
    }
    for (int e = tid; e < n * T; e += DL_THREADS) {       // (each thread reads back its own accumulators)
        const int i = e / T, k = e - i * T;
        gx[(((long)b * n + i) * C + c) * T + k] = ga[e];
    }
}

}  // namespace

#define DL_CHECK_DIMS(name)                                                                                                        \
    CFN_REQUIRE(B >= 1 && C >= 1 && T >= 1 && TL >= 1 && n >= 1, name ": B, C, T, TL, n must be >= 1 (got %d, %d, %d, %d, %d)", B, C, T, TL, n); \
    CFN_REQUIRE((long)n * T <= DL_MAX_ROW, name ": crops * T = %ld logits per row exceed the %d this kernel keeps in LDS", (long)n * T, DL_MAX_ROW); \
    CFN_REQUIRE((long)B * C <= 0x7fffffffL, name ": B * C = %ld rows exceed the grid", (long)B * C)

// train_fine.py:199-213 / train_coarse_fineFEAT.py:226-240 (see include/cfn_hip.h)
extern "C" int cfn_detloss_fwd(const float* logits, const float* labels, const float* masks, const float* norm, double world, float* probs,
                               float* cls, float* loc, int* jstar, float* ymax, double* rows, double* norm_used, int B, int C, int T, int TL,
                               int n, int align_corners, void* stream) {
    CFN_REQUIRE(logits && labels && masks && cls && loc && jstar && ymax && rows && norm_used, "cfn_detloss_fwd: null tensor");
    DL_CHECK_DIMS("cfn_detloss_fwd");
    hipStream_t st = (hipStream_t)stream;
    const int BC = B * C;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 4.0 * ((double)BC * TL * (probs ? 2 : 1) + (double)B * TL + (double)BC * n * T));
    hipLaunchKernelGGL(detloss_fwd_kernel, dim3(BC), dim3(DL_THREADS), DL_RED_BYTES + (size_t)n * T * sizeof(float), st, logits, labels, masks,
                       probs, rows, jstar, ymax, BC, C, T, TL, n, align_corners ? 1 : 0);
    hipLaunchKernelGGL(detloss_fin_kernel, dim3(1), dim3(DL_THREADS), DL_RED_BYTES, st, (const double*)rows, masks, norm, world, cls, loc,
                       norm_used, BC, C, (long)B * TL);
    return cfn_check_launch("detloss_fwd");
}

extern "C" int cfn_detloss_bwd(const float* g_cls, const float* g_loc, const float* logits, const float* labels, const float* masks,
                               const int* jstar, const float* ymax, const double* norm_used, double world, float* gx, int B, int C, int T,
                               int TL, int n, int align_corners, void* stream) {
    CFN_REQUIRE(g_cls && g_loc && logits && labels && masks && jstar && ymax && norm_used && gx, "cfn_detloss_bwd: null tensor");
    DL_CHECK_DIMS("cfn_detloss_bwd");
    hipStream_t st = (hipStream_t)stream;
    const int BC = B * C, JT = TL < DL_JT ? TL : DL_JT;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 4.0 * ((double)BC * TL + (double)B * TL + 2.0 * BC * n * T));
    hipLaunchKernelGGL(detloss_bwd_kernel, dim3(BC), dim3(DL_THREADS), (size_t)(2 * n * T + 2 * JT) * sizeof(float), st, g_cls, g_loc, logits,
                       labels, masks, jstar, ymax, norm_used, world, gx, BC, C, T, TL, n, align_corners ? 1 : 0, JT);
    return cfn_check_launch("detloss_bwd");
}
