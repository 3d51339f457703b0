// Proposal recall at N per video, AR@N (cfn_hip/recall.py): how many ground-truth segments at least one of the N best candidates of their video
// covers.  The rule is stated once (cfn_hip/recall.py's docstring; recall_reference spells the same on the host):
//
//   R1. participation and window clip: rule 1 of segap.hip to the bit (seg_gt_row of seg_common.h; the class test is "an integer of [0, C)").
//       Row g belongs to video b iff offsets[b] <= g < offsets[b + 1] (offsets clamped to [0, n_seg] and expected not to decrease; the video
//       is found by a binary search, so malformed offsets give wrong values, never an access outside the buffers).
//   R2. tIoU: seg_tiou of seg_common.h.
//   R3. video rank: the candidates of video b are the rows det_offsets[b] .. det_offsets[b + 1], clamped to [0, det_cap], ALL classes together,
//       ranked by det_score[:, score_col] descending (fp32), a NaN taken as -inf (seg_nan_low), ties to the lower row: a permutation of
//       0 .. n_b - 1 whatever the data.
//   R4. first hit: for a participating row g (video b, class c) and threshold k, hit[k, g] = the smallest video rank among the candidates of
//       the SAME video and class whose tIoU with g is > 0 and >= tiou[k]; n_max when there is none or the smallest is >= n_max; -1 for a row
//       that does not participate.  No one-to-one matching: a candidate may recall several rows.
//   R5. state (int64): hist (n_thr, n_max), then n_gt, n_videos, n_props.  hist[k, hit[k, g]] += 1 for every participating g with
//       hit < n_max; n_gt += the participating rows; n_videos += B; n_props += the sum of the clamped n_b.  Integer adds only.
//   R6. value (fp64): recall[k, n] = (double)(hist[k, 0] + .. + hist[k, n]) / (double)n_gt, 0 when n_gt == 0; ar[n] = (recall[0, n] + .. +
//       recall[n_thr - 1, n]) / n_thr, added in k order; auc = (ar[0] + .. + ar[n_max - 1]) / n_max, added in n order; avg_props =
//       n_props / n_videos (0 without videos).  No product, so nothing contracts: bit-equal to numpy.
//
// Launches of cfn_seg_recall_add, ordered by the stream alone (no allocation, no synchronisation, nothing in floating point is accumulated):
//   rank        grid (tiles of SR_TILE rows, video).  A thread owns one row of its video and counts the rows in front of it while the video's
//               scores pass through an LDS tile of SR_TILE floats (coalesced fill, then every lane reads the same word: a broadcast).
//               O(n_b^2) per video, O(n_b^2 / SR_TILE) per workgroup; workgroups behind the video's last row leave at once.
//   first hit   one wave per ground-truth row, SR_WAVES rows per workgroup.  The row's video by binary search, its (video, class) group by
//               seg_group; the 64 lanes stride over the group's candidates with n_thr running minima in registers, then a butterfly of
//               shuffles.  No LDS, no barrier: the ranks come from the launch before.
//   accumulate  one workgroup per threshold counts its row of hit in LDS (LDS integer atomics) and adds the counts to its own row of
//               hist; workgroup 0 also advances n_gt, n_videos and n_props.
// cfn_seg_recall_value is one workgroup: wave k scans hist[k, :] in int64, then thread n takes ar[n], then one thread takes auc.
#include "seg_common.h"

#define SR_MAX_THR 16
#define SR_MAX_N 1024
#define SR_TILE 256
#define SR_WAVES 4
#define SR_ATHREADS 256

// grid (cdiv(det_cap, SR_TILE), B)
__global__ __launch_bounds__(SR_TILE) void seg_video_rank_kernel(const float* __restrict__ dscore, const int* __restrict__ doff, int* __restrict__ rank,
                                                                 int score_col, long dcap) {
    __shared__ float s_score[SR_TILE];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const long o0 = seg_clampl(doff[b], 0, dcap);
    const long o1 = seg_clampl(doff[b + 1], o0, dcap);
    const long nb = o1 - o0;
    const long first = (long)blockIdx.x * SR_TILE;
    if (first >= nb) return;                                               // (the whole workgroup: no barrier is left waiting)
    const long li = first + tid;                                           // the thread's row inside the video
    const bool mine = li < nb;
    const float si = mine ? seg_nan_low(dscore[2 * (o0 + li) + score_col]) : 0.0f;
    int r = 0;
    for (long j0 = 0; j0 < nb; j0 += SR_TILE) {
        const long lj = j0 + tid;
        s_score[tid] = lj < nb ? seg_nan_low(dscore[2 * (o0 + lj) + score_col]) : -INFINITY;
        __syncthreads();
        const int m = (int)(nb - j0 < SR_TILE ? nb - j0 : SR_TILE);
#pragma unroll 8
        for (int j = 0; j < m; ++j) {
            const float sj = s_score[j];
            r += (sj > si || (sj == si && j0 + j < li)) ? 1 : 0;
        }
        __syncthreads();                                                   // the tile is refilled
    }
    if (mine) rank[o0 + li] = r;
}

// grid (cdiv(n_seg, SR_WAVES)), one wave per ground-truth row
__global__ __launch_bounds__(64 * SR_WAVES) void seg_first_hit_kernel(const double* __restrict__ dseg, const int* __restrict__ doff,
                                                                      const int* __restrict__ rank, const double* __restrict__ gseg,
                                                                      const int* __restrict__ goff, const double* __restrict__ fps,
                                                                      const int* __restrict__ window, const double* __restrict__ tiou,
                                                                      int* __restrict__ hit, int B, int C, int t_max, int n_thr, int n_max, long dcap,
                                                                      long S) {
    const int lane = threadIdx.x & 63;
    const long g = cfn_uni((long)blockIdx.x * SR_WAVES + (threadIdx.x >> 6));
    if (g >= S) return;

    // R1: the row's video -- the last b of [0, B) whose clamped offset is not above g
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_clampl(goff[mid], 0, S) <= g) lo = mid; else hi = mid - 1;
    }
    const int b = lo;
    const long g0 = seg_clampl(goff[b], 0, S);
    const long g1 = seg_clampl(goff[b + 1], g0, S);
    const long wfirst = window[2 * b];
    const int n = min(max(window[2 * b + 1], 0), t_max);
    const double f = fps[b];
    const double w0 = ((double)wfirst - 0.5) / f, w1 = ((double)(wfirst + n) - 0.5) / f;
    const double cls = gseg[3 * g];
    const bool is_class = cls >= 0.0 && cls < (double)C && cls == floor(cls);
    const int c = is_class ? (int)cls : 0;
    double sp, ep;
    const bool part = g >= g0 && is_class && seg_gt_row(gseg, g, g1, (double)c, n, w0, w1, sp, ep);
    if (!part) {
        if (lane < n_thr) hit[(long)lane * S + g] = -1;
        return;
    }

    double thr[SR_MAX_THR];
#pragma unroll
    for (int k = 0; k < SR_MAX_THR; ++k) thr[k] = k < n_thr ? tiou[k] : 2.0;                  // (a tIoU never reaches 2)
    int best[SR_MAX_THR];
#pragma unroll
    for (int k = 0; k < SR_MAX_THR; ++k) best[k] = n_max;

    int nd;
    const long d0 = seg_group(dseg, doff, b, c, dcap, nd);                 // R4: the candidates of the row's video and class
    for (int i = lane; i < nd; i += 64) {
        const long di = d0 + i;
        const double v = seg_tiou(dseg[3 * di + 1], dseg[3 * di + 2], sp, ep);
        if (v > 0.0) {
            const int r = rank[di];
#pragma unroll
            for (int k = 0; k < SR_MAX_THR; ++k)
                if (v >= thr[k]) best[k] = min(best[k], r);
        }
    }
    int mine = n_max;
#pragma unroll
    for (int k = 0; k < SR_MAX_THR; ++k) {
        if (k < n_thr) {                                                   // (uniform)
            int m = best[k];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = min(m, __shfl_xor(m, d, 64));
            if (lane == k) mine = m;
        }
    }
    if (lane < n_thr) hit[(long)lane * S + g] = min(max(mine, 0), n_max);
}

// grid (n_thr)
__global__ __launch_bounds__(SR_ATHREADS) void seg_recall_accumulate_kernel(const int* __restrict__ hit, const int* __restrict__ doff, long* __restrict__ state,
                                                                            int B, int n_thr, int n_max, long dcap, long S) {
    __shared__ int s_cnt[SR_MAX_N];
    __shared__ int s_part;
    __shared__ unsigned long long s_props;
    const int tid = threadIdx.x, k = blockIdx.x;
    for (int i = tid; i < n_max; i += SR_ATHREADS) s_cnt[i] = 0;
    if (tid == 0) { s_part = 0; s_props = 0ull; }
    __syncthreads();
    const int* row = hit + (long)k * S;
    int part = 0;
    for (long g = tid; g < S; g += SR_ATHREADS) {
        const int h = row[g];
        if (h >= 0) {
            ++part;
            if (h < n_max) atomicAdd(&s_cnt[h], 1);
        }
    }
    if (k == 0) {
        if (part) atomicAdd(&s_part, part);
        unsigned long long props = 0ull;
        for (int b = tid; b < B; b += SR_ATHREADS) {
            const long o0 = seg_clampl(doff[b], 0, dcap);
            props += (unsigned long long)(seg_clampl(doff[b + 1], o0, dcap) - o0);
        }
        if (props) atomicAdd(&s_props, props);
    }
    __syncthreads();
    long* hist = state + (long)k * n_max;                                  // this workgroup's own row: plain adds
    for (int i = tid; i < n_max; i += SR_ATHREADS) {
        const int cnt = s_cnt[i];
        if (cnt) hist[i] += (long)cnt;
    }
    if (k == 0 && tid == 0) {
        long* tail = state + (long)n_thr * n_max;
        tail[0] += (long)s_part;
        tail[1] += (long)B;
        tail[2] += (long)s_props;
    }
}

// one workgroup of SR_MAX_THR waves.  out: recall (n_thr, n_max), ar (n_max), auc, avg_props
__global__ __launch_bounds__(64 * SR_MAX_THR) void seg_recall_value_kernel(const long* __restrict__ state, double* __restrict__ out, int n_thr, int n_max) {
    __shared__ double s_ar[SR_MAX_N];
    const int tid = threadIdx.x, lane = tid & 63, k = cfn_uni(tid >> 6);
    const long* tail = state + (long)n_thr * n_max;
    const long n_gt = tail[0];
    double* recall = out;
    double* ar = out + (long)n_thr * n_max;
    if (k < n_thr) {                                                       // R6: an inclusive scan of hist[k, :] in int64, 64 columns at a time
        long long carry = 0;
        for (int n0 = 0; n0 < n_max; n0 += 64) {
            const int n = n0 + lane;
            long long incl = n < n_max ? (long long)state[(long)k * n_max + n] : 0ll;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            incl += carry;
            if (n < n_max) recall[(long)k * n_max + n] = n_gt > 0 ? (double)incl / (double)n_gt : 0.0;
            carry = __shfl(incl, 63, 64);
        }
    }
    __syncthreads();                                                       // (the workgroup's own stores to recall are visible behind it)
    for (int n = tid; n < n_max; n += 64 * SR_MAX_THR) {
        double s = 0.0;
        for (int j = 0; j < n_thr; ++j) s += recall[(long)j * n_max + n];  // k order
        s = s / (double)n_thr;
        ar[n] = s;
        s_ar[n] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int n = 0; n < n_max; ++n) s += s_ar[n];                      // n order
        ar[n_max] = s / (double)n_max;
        const long vids = tail[1];
        ar[n_max + 1] = vids > 0 ? (double)tail[2] / (double)vids : 0.0;
    }
}

static inline bool sr_shape_ok(int B, int C, long det_cap, long n_seg) {
    return B >= 1 && C >= 1 && B <= 65535 && C <= 65535 && (long)B * C < (1L << 31) && det_cap >= 1 && det_cap < (1L << 31) && n_seg >= 1 &&
           n_seg < (1L << 31);
}

// workspace: int32 rank [det_cap]
extern "C" long cfn_seg_recall_workspace_bytes(int B, int C, long det_cap, long n_seg, int n_thr) {
    if (!sr_shape_ok(B, C, det_cap, n_seg) || n_thr < 1 || n_thr > SR_MAX_THR) return -1;
    return (det_cap * 4 + 7) & ~7L;
}

extern "C" int cfn_seg_recall_rank_tile(void) { return SR_TILE; }

extern "C" int cfn_seg_recall_add(const double* det_seg, const float* det_score, const int* det_offsets, const double* seg, const int* offsets,
                                  const double* fps, const int* window, const double* tiou, int* hit, long* state, void* workspace, int B, int C,
                                  int t_max, int n_thr, int n_max, int score_col, long det_cap, long n_seg, void* stream) {
    const char* what = "cfn_seg_recall_add";
    CFN_REQUIRE(det_seg && det_score && det_offsets && seg && offsets && fps && window && tiou && hit && state && workspace, "%s: null tensor", what);
    CFN_REQUIRE(sr_shape_ok(B, C, det_cap, n_seg), "%s: bad shape (B %d, C %d <= 65535; det_cap %ld, n_seg %ld in [1, 2^31))", what, B, C, det_cap, n_seg);
    CFN_REQUIRE(t_max >= 1, "%s: t_max >= 1 expected, got %d", what, t_max);
    CFN_REQUIRE(n_thr >= 1 && n_thr <= SR_MAX_THR, "%s: n_thr in [1, %d] expected, got %d", what, SR_MAX_THR, n_thr);
    CFN_REQUIRE(n_max >= 1 && n_max <= SR_MAX_N, "%s: n_max in [1, %d] expected, got %d", what, SR_MAX_N, n_max);
    CFN_REQUIRE(score_col == 0 || score_col == 1, "%s: score_col 0 (max) or 1 (mean) expected, got %d", what, score_col);
    CFN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace on an 8-byte boundary expected", what);
    hipStream_t st = (hipStream_t)stream;
    int* rank = (int*)workspace;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(seg_video_rank_kernel, dim3((unsigned)cfn_cdiv(det_cap, SR_TILE), (unsigned)B), dim3(SR_TILE), 0, st, det_score, det_offsets, rank,
                       score_col, det_cap);
    hipLaunchKernelGGL(seg_first_hit_kernel, dim3((unsigned)cfn_cdiv(n_seg, SR_WAVES)), dim3(64 * SR_WAVES), 0, st, det_seg, det_offsets, (const int*)rank,
                       seg, offsets, fps, window, tiou, hit, B, C, t_max, n_thr, n_max, det_cap, n_seg);
    hipLaunchKernelGGL(seg_recall_accumulate_kernel, dim3((unsigned)n_thr), dim3(SR_ATHREADS), 0, st, (const int*)hit, det_offsets, state, B, n_thr, n_max,
                       det_cap, n_seg);
    return cfn_launch_ok(what);
}

extern "C" int cfn_seg_recall_value(const long* state, double* out, int n_thr, int n_max, void* stream) {
    const char* what = "cfn_seg_recall_value";
    CFN_REQUIRE(state && out, "%s: null tensor", what);
    CFN_REQUIRE(n_thr >= 1 && n_thr <= SR_MAX_THR, "%s: n_thr in [1, %d] expected, got %d", what, SR_MAX_THR, n_thr);
    CFN_REQUIRE(n_max >= 1 && n_max <= SR_MAX_N, "%s: n_max in [1, %d] expected, got %d", what, SR_MAX_N, n_max);
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(seg_recall_value_kernel, dim3(1), dim3(64 * SR_MAX_THR), 0, st, state, out, n_thr, n_max);
    return cfn_launch_ok(what);
}
