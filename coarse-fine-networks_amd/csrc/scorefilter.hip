// Temporal filtering of per-frame scores in front of the decode (cfn_hip/scorefilter.py apply / filter_reference): probs (B, C, TL) fp32 ->
// out (B, C, TL) fp32, a weighted mean (box, Gaussian) or a median over a per-class window.  The rule (cfn_hip/scorefilter.py and
// include/cfn_hip.h spell the same):
//
//   F1. n = min(max(valid_t[b], 0), TL), r = min(max(radius[c], 0), R).  Frames t >= n are copied from probs bit for bit; r = 0 copies every
//       frame bit for bit, under either method.
//   F2. the window of frame t < n is u in [max(0, t - r), min(n - 1, t + r)]: truncated at the valid range, no padding, no reflection.
//   F3. a window that holds a non-finite value gives the canonical quiet NaN 0x7fc00000 (the decode never activates such a frame); so does a
//       weighted mean whose quotient is a NaN (weights that are not the documented non-negative finite table).
//   F4. weighted mean, u ascending: num = sum of weights[c, |u - t|] * (double)probs[b, c, u], den = sum of weights[c, |u - t|], both from
//       0.0, every product and every sum rounded separately (no fused multiply-add); then ONE IEEE fp64 division and ONE rounding to fp32.
//   F5. median: the window ordered by (value, u): rank(u) = #{v : p[v] < p[u] or (p[v] == p[u] and v < u)} (a stable sort, so +0 / -0
//       ties are decided).  m frames, m odd: the element of rank (m - 1) / 2; m even: (float)(((double)a + (double)b) * 0.5) with a, b the elements
//       of ranks m / 2 - 1 and m / 2.
//   F6. no atomics, nothing is read back, nothing accumulates across threads: the same bits in every run.
//
// One launch, grid (tile of SF_TILE frames, class, video), one thread per frame.  The tile and a halo of SF_MAX_R frames on each side are
// staged in LDS by bounds-checked loads that never leave row (b, c) (a frame outside [0, TL) is staged as 0 and never read by a window,
// which F2 keeps inside [0, n)); the class's weight row is staged beside it.  The median ranks by counting over the LDS window:
// O(window^2) LDS reads per frame (65 * 65 at r = 32), the price of having no per-thread array (nothing is indexed at run time in registers,
// so nothing spills: scratch 0, tools/kernel_resources.sh).  valid_t, radius and weights are DATA: both are clamped, every index is in range
// whatever they hold.
#include "cfn_common.h"

#define SF_TILE 256
#define SF_MAX_R 32
#define SF_SPAN (SF_TILE + 2 * SF_MAX_R)
#define SF_QNAN 0x7fc00000u

__device__ __forceinline__ bool sf_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// grid (ceil(TL / SF_TILE), C, B), SF_TILE threads
__global__ __launch_bounds__(SF_TILE) void score_filter_kernel(const float* __restrict__ probs, const int* __restrict__ valid_t,
                                                               const int* __restrict__ radius, const double* __restrict__ weights,
                                                               float* __restrict__ out, int C, int TL, int R, int method) {
#pragma clang fp contract(off)
    __shared__ float s_p[SF_SPAN];                                         // frame u of the row at u - t0 + SF_MAX_R
    __shared__ double s_w[SF_MAX_R + 1];
    const int tid = threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    const int t0 = blockIdx.x * SF_TILE;
    const long row = ((long)b * C + c) * TL;
    const int n = min(max(valid_t[b], 0), TL);                             // rule F1
    const int r = min(max(radius[c], 0), R);
    for (int i = tid; i < SF_SPAN; i += SF_TILE) {
        const int u = t0 - SF_MAX_R + i;
        s_p[i] = (u >= 0 && u < TL) ? probs[row + u] : 0.0f;
    }
    if (tid <= SF_MAX_R) s_w[tid] = tid <= R ? weights[(long)c * (R + 1) + tid] : 0.0;
    __syncthreads();
    const int t = t0 + tid;
    if (t >= TL) return;
    const float* p = s_p;
    const int o =SF_MAX_R - t0;                                           // frame u is p[o + u], u in [t0 - SF_MAX_R, t0 + SF_TILE + SF_MAX_R)
    unsigned bits = __float_as_uint(p[o + t]);
    if (t < n && r > 0) {
        const int lo = max(0, t - r), hi = min(n - 1, t + r);              // rule F2: t0 - SF_MAX_R <= lo <= t <= hi < t0 + SF_TILE + SF_MAX_R
        bool finite = true;
        for (int u = lo; u <= hi; ++u) finite = finite && sf_finite(p[o + u]);
        if (!finite) {
            bits = SF_QNAN;                                                // rule F3
        } else if (method == 0) {                                          // rule F4
            double num = 0.0, den = 0.0;
            for (int u = lo; u <= hi; ++u) {
                const double w = s_w[u < t ? t - u : u - t];
                const double term = w * (double)p[o + u];
                num = num + term;
                den = den + w;
            }
            const float q = (float)(num / den);
            bits = q != q ? SF_QNAN : __float_as_uint(q);
        } else {                                                           // rule F5
            const int m = hi - lo + 1;
            const int ka = (m - 1) >> 1, kb = m >> 1;                      // m odd: ka == kb; m even: m / 2 - 1 and m / 2
            float a = 0.0f, bv = 0.0f;
            for (int u = lo; u <= hi; ++u) {
                const float pu = p[o + u];
                int rank = 0;
                for (int v = lo; v <= hi; ++v) {
                    const float pv = p[o + v];
                    rank += (pv < pu || (pv == pu && v < u)) ? 1 : 0;
                }
                a = rank == ka ? pu : a;
                bv = rank == kb ? pu : bv;
            }
            const float med = (m & 1) ? a : (float)(((double)a + (double)bv) * 0.5);
            bits = __float_as_uint(med);
        }
    }
    reinterpret_cast<unsigned*>(out)[row + t] = bits;
}

extern "C" int cfn_score_filter_tile(void) { return SF_TILE; }

extern "C" int cfn_score_filter(const float* probs, const int* valid_t, const int* radius, const double* weights, float* out, int B, int C, int TL,
                                int R, int method, void* stream) {
    const char* what = "cfn_score_filter";
    CFN_REQUIRE(probs && valid_t && radius && weights && out, "%s: null tensor", what);
    CFN_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 65535, "%s: B and C in [1, 65535] expected, got %d and %d", what, B, C);
    CFN_REQUIRE(TL >= 1 && TL <= 65536, "%s: TL in [1, 65536] expected, got %d", what, TL);
    CFN_REQUIRE(R >= 0 && R <= SF_MAX_R, "%s: R in [0, %d] expected (windows of at most %d frames), got %d", what, SF_MAX_R, 2 * SF_MAX_R + 1, R);
    CFN_REQUIRE(method == 0 || method == 1, "%s: method 0 (weighted mean) or 1 (median) expected, got %d", what, method);
    CFN_REQUIRE((const void*)out != (const void*)probs, "%s: out must not be probs (a window reads frames another thread has written)", what);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cfn_cdiv(TL, SF_TILE), (unsigned)C, (unsigned)B);
    CfnProfScope prof(CFN_K_ELEMWISE, st, (double)B * C * TL * 8.0);
    hipLaunchKernelGGL(score_filter_kernel, grid, dim3(SF_TILE), 0, st, probs, valid_t, radius, weights, out, C, TL, R, method);
    return cfn_check_launch(what);
}
