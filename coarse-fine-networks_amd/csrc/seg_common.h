// The rules that the segment kernels share, stated once: detections.hip (decode), segnms.hip (NMS, Soft-NMS), segap.hip (segment AP) and
// segrecall.hip (proposal recall) all work on Detections (seg (cap, 3) fp64 rows [class, start_s, end_s], score (cap, 2) fp32, offsets (B + 1,) int32) and on their
// (video, class) groups.  These rules are bit-exact statements that the numpy references spell too (cfn_hip/detections.py, cfn_hip/segap.py):
// change one here and every kernel follows.  Everything is __forceinline__, so a kernel pays nothing for sharing them (tools/kernel_resources.sh).
#pragma once
#include "cfn_common.h"

__device__ __forceinline__ long seg_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first row i of [lo, hi) whose class is not below key (all lanes walk the same way; at most 32 steps whatever the data)
__device__ __forceinline__ long seg_lower(const double* __restrict__ seg, long lo, long hi, double key) {
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (seg[3 * mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The rows [d0, d0 + nd) of group (b, c) (rule N1 of segnms.hip, the detections of a group in segap.hip): the rows offsets[b] ..
// offsets[b + 1] of the video, clamped to [0, cap], whose class column is c -- two binary searches, as the class column does not decrease
// inside a video (decode orders by (b, c, t0)).  offsets are DATA: whatever they hold, 0 <= d0 <= d0 + nd <= cap.
__device__ __forceinline__ long seg_group(const double* __restrict__ seg, const int* __restrict__ offsets, int b, int c, long cap, int& nd) {
    const long o0 = seg_clampl(offsets[b], 0, cap);
    const long o1 = seg_clampl(offsets[b + 1], o0, cap);
    const long d0 = seg_lower(seg, o0, o1, (double)c);
    const long d1 = seg_lower(seg, d0, o1, (double)c + 1.0);
    nd = (int)(d1 - d0);
    return d0;
}

// tIoU of (s0, e0) and (s1, e1) (rule N3 of segnms.hip, rule 2 of segap.hip; tiou_reference on the host): inter = min(e0, e1) - max(s0, s1);
// 0 unless inter > 0, otherwise inter / ((e0 - s0) + (e1 - s1) - inter).  Plain IEEE fp64, no product (nothing can contract), ONE division.
__device__ __forceinline__ double seg_tiou(double s0, double e0, double s1, double e1) {
    const double inter = (e0 < e1 ? e0 : e1) - (s0 > s1 ? s0 : s1);
    if (!(inter > 0.0)) return 0.0;
    return inter / ((e0 - s0) + (e1 - s1) - inter);
}

// Rule 1 of segap.hip for ground-truth row g (R1 of segrecall.hip): the bounds clipped to the window (w0, w1) -- max / min, a NaN bound gives way
// to the window's; true iff the row participates in class cd: g < g1, n > 0, the class column equals cd and e' > s'.
__device__ __forceinline__ bool seg_gt_row(const double* __restrict__ gseg, long g, long g1, double cd, int n, double w0, double w1, double& sp,
                                           double& ep) {
    sp = 0.0; ep = 0.0;
    if (g >= g1) return false;
    const double cls = gseg[3 * g], s = gseg[3 * g + 1], e = gseg[3 * g + 2];
    sp = s > w0 ? s : w0;
    ep = e < w1 ? e : w1;
    return n > 0 && cls == cd && ep > sp;
}

// Rank by counting (rule N2 of segnms.hip, rule 3 of segap.hip): the rank of row i among the nd rows of a group, key descending (fp32),
// ties by row index ascending; key(j) loads row j's key.  O(nd) per row, O(nd^2 / 64) per group and wave.  The one place where the order is
// spelled: the LDS paths (key reads LDS) and the workspace paths (key reads the score column from memory) both come here.
// The two NaN conventions stay apart, in the callers' key():
//   NMS          maps a NaN to -inf with seg_nan_low() where it loads a score, so the ranks of a group are a permutation of 0 .. nd - 1
//                whatever the data.
//   segment AP   compares the raw scores.  A NaN is neither above nor equal to anything, so with NaN scores two rows can get one rank and a
//                rank can stay empty: the ranks are then NOT a permutation, and segap_match_kernel only clamps what it reads back from
//                order[].  Whether it should rank NaNs like NMS is a question of behaviour, left as it is here.
// The result is < nd (at most nd - 1 rows are in front of one); the min() is the identity and makes it an index whatever the data.
// A caller whose order[] goes through memory keeps its release fence, barrier and acquire fence between its last store of a rank and its first
// read of one: other lanes wrote what a lane reads back.
__device__ __forceinline__ float seg_nan_low(float s) { return s != s ? -INFINITY : s; }

template <class Key>
__device__ __forceinline__ int seg_rank(Key key, int i, int nd) {
    const float si = key(i);
    int r = 0;
    for (int j = 0; j < nd; ++j) {
        const float sj = key(j);
        r += (sj > si || (sj == si && j < i)) ? 1 : 0;
    }
    return min(r, nd - 1);
}

// exclusive scan of one int per thread over a workgroup of whole waves (wave scans + the wave totals in s_wave[blockDim.x / 64]); total = the
// sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ int seg_block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                                       // (s_wave may still be read from the scan before)
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, sum = 0;
    for (int i = 0; i < nw; ++i) {
        const int x = s_wave[i];
        if (i < wave) before += x;
        sum += x;
    }
    total = sum;
    return before + inc - v;
}

// One launch of one workgroup (seg_scan_kernel, defined once in detections.hip: this build has no relocatable device code, so a kernel in a
// header that two sources include would be a duplicate symbol): counts[0 .. n), each clamped to [0, count_max], -> exclusive sums in place,
// counts[n] = offsets[B] = total[0] = the sum, and offsets[i / C] = the sum in front of row i for every i that is a multiple of C (the rows
// of a video are C consecutive counts).  The second of the three launches of decode, NMS and Soft-NMS.
void seg_launch_scan(int* counts, int* offsets, int* total, long n, int B, int C, long count_max, hipStream_t st);
