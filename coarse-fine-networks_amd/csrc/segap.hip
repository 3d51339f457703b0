// Segment-level average precision at temporal-IoU thresholds (cfn_hip/segap.py): the first consumer of the pair SegLabels / Detections.
// The reference stops at probs (train_fine.py:199-222), so there is nothing to copy; the rule is stated once (cfn_hip/segap.py
// ap_reference spells the same on the host):
//
//   1. window clip of the ground truth: n = clamp(window[b,1], 0, t_max), w0 = ((double)window[b,0] - 0.5) / fps[b],
//      w1 = ((double)(window[b,0] + n) - 0.5) / fps[b];  s' = s > w0 ? s : w0,  e' = e < w1 ? e : w1 (max / min; a NaN bound gives way to the
//      window's).  A row PARTICIPATES iff n > 0, its class is an integer of [0, C) and e' > s'.  n_gt[c] counts participating rows.
//   2. tIoU of a detection (sd, ed) and a clipped row (s', e'): inter = min(ed, e') - max(sd, s'); 0 unless inter > 0, otherwise
//      inter / ((ed - sd) + (e' - s') - inter).  Plain IEEE fp64, no product (nothing can contract), ONE division (seg_tiou of seg_common.h).
//   3. within a (video, class) group the detections are taken by score[:, score_col] descending (fp32), ties by row index ascending
//      (seg_rank of seg_common.h on the raw scores: see there for NaN).
//   4. greedy matching, independently per threshold k: a detection takes the participating row of its group that is not used up at k and has
//      the largest tIoU among those with tIoU >= tiou[k] (and > 0); ties go to the lowest row index.  It is then a true positive at k and
//      the row is used up at k; otherwise it is a false positive at k.
//   5. per detection: one byte tp (bit k = true positive at k) and optionally match (n_thr, det_cap) int32 = the row index or -1.
//   6. class c's store receives the batch's detections of class c in (video, row) order behind the rows it holds; counts[c] and n_gt[c]
//      advance.  A batch that would push ANY class past cap writes nothing, changes no count and sets flag bit 1 (cfn_ap_append's rule).
//   7. per class a stable descending sort by score in insertion order (cfn_ap_sort_counts: cfn_ap_sort's ordering of special values, the tp
//      byte is the payload);  ap[k, c] = (sum over the ranks r whose bit k is set of tp_cum_r / r) / n_gt[c], fp64 in a fixed order, rounded
//      to fp32, 0 where n_gt[c] == 0;  map[k] = the mean of ap[k, c] over the classes with n_gt[c] > 0 (fp64 in class order, rounded to fp32).
//
// Launches, ordered by the stream alone (no atomics except one flag bit, no allocation, no synchronisation, no floating-point accumulation
// across workgroups):
//   match    one wave per (video, class) group.  The group's detections are a contiguous range of the video's rows (decode orders by
//            (b, c, t0)): two binary searches on the class column (seg_group of seg_common.h).  Lanes hold the video's ground-truth rows, SA_GT_TILE = 64 at a time;
//            a lane computes the tIoU of its row ONCE per detection for all thresholds, a ballot finds the candidates at k (none: a false
//            positive; one: the match), a wave argmax on (tIoU, lane) otherwise.  A video of at most one tile keeps its rows and the byte of
//            used-up thresholds in registers; a larger one (the general path) walks its tiles per detection, carries the best (tIoU, row)
//            per threshold across them and keeps the bytes in the workspace (a row belongs to one group, and is always held by the same lane).
//            The score order is rank by counting, O(nd^2 / 64) per group: ranks and scores of up to SA_DET_TILE = 1024 detections live in
//            LDS; a larger group (the general path) reads the scores from memory and keeps its order in the workspace.
//   plan     one workgroup: per class the batch's total against cap; then either every class's counts advance and every group gets its
//            base row in the stores, or the flag is set.
//   copy     one wave per group: score and tp byte to base + i.
//   reduce   grid (C, n_thr): the walk of cfn_ap_reduce over bit k of the sorted bytes, divided by n_gt[c]; then one wave for map.
// Everything but B, C, t_max, n_thr, score_col and the capacities is DATA read on the device: offsets, counts and orders are clamped, so a
// bad batch gives wrong values, never a store outside the outputs.
#include "seg_common.h"

#define SA_FLAG_OVERFLOW 2
#define SA_GT_TILE 64
#define SA_DET_TILE 1024
#define SA_MAX_THR 8
#define SA_RTHREADS 256
#define SA_RPT 16
#define SA_RTILE (SA_RTHREADS * SA_RPT)

// workspace: int32 dstart, dcount, gcount, base [B * C] each, fit [2], order [det_cap]; then n_seg bytes
struct SaWs { int *dstart, *dcount, *gcount, *base, *fit, *order; unsigned char* used; };
static inline long sa_ws_ints(long groups, long det_cap) { return 4 * groups + 2 + det_cap; }
static inline SaWs sa_carve(void* ws, long groups, long det_cap) {
    SaWs w;
    w.dstart = (int*)ws; w.dcount = w.dstart + groups; w.gcount = w.dcount + groups; w.base = w.gcount + groups;
    w.fit = w.base + groups; w.order = w.fit + 2;
    w.used = (unsigned char*)(w.order + det_cap);
    return w;
}

// the candidate lane with the largest v, the lowest such lane on a tie; at least one lane is a candidate.  Every lane gets (lane, value).
__device__ __forceinline__ int sa_argmax(double v, bool cand, int lane, double& best) {
    double bv = cand ? v : -1.0;
    int bl = cand ? lane : 64;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(bv, d, 64);
        const int ol = __shfl_xor(bl, d, 64);
        if (ov > bv || (ov == bv && ol < bl)) { bv = ov; bl = ol; }
    }
    best = bv;
    return bl;
}

// grid (B * C), one wave each
__global__ __launch_bounds__(64) void segap_match_kernel(const double* __restrict__ dseg, const float* __restrict__ dscore, const int* __restrict__ doff,
                                                         const double* __restrict__ gseg, const int* __restrict__ goff, const double* __restrict__ fps,
                                                         const int* __restrict__ window, const double* __restrict__ tiou, unsigned char* __restrict__ tp,
                                                         int* __restrict__ match, int* __restrict__ ws_dstart, int* __restrict__ ws_dcount,
                                                         int* __restrict__ ws_gcount, int* __restrict__ ws_order, unsigned char* __restrict__ ws_used,
                                                         int C, int t_max, int n_thr, int score_col, long dcap, long S) {
    __shared__ float s_score[SA_DET_TILE];
    __shared__ int s_order[SA_DET_TILE];
    const int lane = threadIdx.x;
    const long grp = blockIdx.x;
    const int b = (int)(grp / C), c = (int)(grp - (long)b * C);
    const double cd = (double)c;

    // the group's detections: rows [d0, d1) of the video's range
    int nd;
    const long d0 = seg_group(dseg, doff, b, c, dcap, nd);

    // the video's ground truth and window (rule 1)
    const long g0 = seg_clampl(goff[b], 0, S);
    const long g1 = seg_clampl(goff[b + 1], g0, S);
    const bool one = g1 - g0 <= SA_GT_TILE;
    const long wfirst = window[2 * b];
    const int n = min(max(window[2 * b + 1], 0), t_max);
    const double f = fps[b];
    const double w0 = ((double)wfirst - 0.5) / f, w1 = ((double)(wfirst + n) - 0.5) / f;

    int ng = 0;
    for (long t0 = g0; t0 < g1; t0 += SA_GT_TILE) {
        double sp, ep;
        const bool part = seg_gt_row(gseg, t0 + lane, g1, cd, n, w0, w1, sp, ep);
        if (!one && part) ws_used[t0 + lane] = 0;                          // (a row belongs to one group; the same lane reads it back below)
        ng += __popcll(__ballot(part));
    }
    if (lane == 0) {
        ws_dstart[grp] = (int)d0;
        ws_dcount[grp] = nd;
        ws_gcount[grp] = ng;
    }
    if (nd <= 0) return;
    if (ng == 0) {                                                         // every detection is a false positive at every threshold
        for (int i = lane; i < nd; i += 64) {
            tp[d0 + i] = 0;
            if (match)
                for (int k = 0; k < n_thr; ++k) match[(long)k * dcap + d0 + i] = -1;
        }
        return;
    }

    // rule 3: rank by counting; order[rank] = row of the group
    const bool small = nd <= SA_DET_TILE;
    int* order = small ? s_order : ws_order + d0;
    if (small) {
        for (int i = lane; i < nd; i += 64) s_score[i] = dscore[2 * (d0 + i) + score_col];
        __syncthreads();
        for (int i = lane; i < nd; i += 64) s_order[seg_rank([&](int j) { return s_score[j]; }, i, nd)] = i;
        __syncthreads();
    } else {
        for (int i = lane; i < nd; i += 64) order[seg_rank([&](int j) { return dscore[2 * (d0 + j) + score_col]; }, i, nd)] = i;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                 // the other lanes' ranks are read back through memory
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }

    double thr[SA_MAX_THR];
#pragma unroll
    for (int k = 0; k < SA_MAX_THR; ++k) thr[k] = k < n_thr ? tiou[k] : 2.0;

    if (one) {                                                             // rule 4, the video's rows in one tile of lanes
        double sp, ep;
        const bool part = seg_gt_row(gseg, g0 + lane, g1, cd, n, w0, w1, sp, ep);
        unsigned used = 0u;                                                // bit k: the lane's row is used up at threshold k
        for (int r = 0; r < nd; ++r) {
            const int i = cfn_uni(min(max(order[r], 0), nd - 1));          // (NaN scores may leave a rank empty: any row of the group then)
            const long di = d0 + i;
            const double sd = dseg[3 * di + 1], ed = dseg[3 * di + 2];
            const double v = part ? seg_tiou(sd, ed, sp, ep) : 0.0;
            unsigned tpb = 0u;
            int mine = -1;                                                 // lane k: the match at threshold k
#pragma unroll
            for (int k = 0; k < SA_MAX_THR; ++k) {
                if (k < n_thr) {
                    const bool cand = part && v > 0.0 && v >= thr[k] && !((used >> k) & 1u);
                    const unsigned long long m = __ballot(cand);
                    if (m) {
                        double best;
                        const int win = __popcll(m) == 1 ? (int)__builtin_ctzll(m) : sa_argmax(v, cand, lane, best);
                        if (lane == win) used |= 1u << k;
                        if (lane == k) mine = (int)(g0 + win);
                        tpb |= 1u << k;
                    }
                }
            }
            if (lane == 0) tp[di] = (unsigned char)tpb;
            if (match && lane < n_thr) match[(long)lane * dcap + di] = mine;
        }
        return;
    }

    for (int r = 0; r < nd; ++r) {                                         // rule 4, the general path: the video's rows tile by tile
        const int i = cfn_uni(min(max(order[r], 0), nd - 1));
        const long di = d0 + i;
        const double sd = dseg[3 * di + 1], ed = dseg[3 * di + 2];
        double bv[SA_MAX_THR];
        long bi[SA_MAX_THR];
#pragma unroll
        for (int k = 0; k < SA_MAX_THR; ++k) { bv[k] = 0.0; bi[k] = -1; }
        for (long t0 = g0; t0 < g1; t0 += SA_GT_TILE) {
            double sp, ep;
            const bool part = seg_gt_row(gseg, t0 + lane, g1, cd, n, w0, w1, sp, ep);
            const double v = part ? seg_tiou(sd, ed, sp, ep) : 0.0;
            const unsigned used = part ? ws_used[t0 + lane] : 0u;
#pragma unroll
            for (int k = 0; k < SA_MAX_THR; ++k) {
                if (k < n_thr) {
                    const bool cand = part && v > 0.0 && v >= thr[k] && !((used >> k) & 1u);
                    if (__ballot(cand)) {
                        double best;
                        const int win = sa_argmax(v, cand, lane, best);
                        if (best > bv[k]) { bv[k] = best; bi[k] = t0 + win; }      // (strict: an earlier tile keeps a tie, its rows are lower)
                    }
                }
            }
        }
        unsigned tpb = 0u;
        int mine = -1;
#pragma unroll
        for (int k = 0; k < SA_MAX_THR; ++k) {
            if (k < n_thr && bi[k] >= 0) {
                if (lane == (int)((bi[k] - g0) & 63)) ws_used[bi[k]] |= (unsigned char)(1u << k);      // the lane that holds the row in its tile
                if (lane == k) mine = (int)bi[k];
                tpb |= 1u << k;
            }
        }
        if (lane == 0) tp[di] = (unsigned char)tpb;
        if (match && lane < n_thr) match[(long)lane * dcap + di] = mine;
    }
}

// one workgroup.  Rule 6: the batch fits, counts and n_gt advance and every group gets its base -- or nothing changes but the flag.
__global__ __launch_bounds__(1024) void segap_plan_kernel(const int* __restrict__ ws_dcount, const int* __restrict__ ws_gcount, int* __restrict__ ws_base,
                                                          int* __restrict__ ws_fit, int* __restrict__ counts, int* __restrict__ n_gt,
                                                          int* __restrict__ flags, int B, int C, long dcap, long cap) {
    const int tid = threadIdx.x;
    int over = 0;
    for (int c = tid; c < C; c += 1024) {
        long total = seg_clampl(counts[c], 0, cap);
        for (int b = 0; b < B; ++b) total += seg_clampl(ws_dcount[(long)b * C + c], 0, dcap);
        if (total > cap) over = 1;
    }
    over = __syncthreads_or(over);                                         // (also: every count has been read before one is advanced)
    if (tid == 0) {
        ws_fit[0] = over ? 0 : 1;
        if (over) atomicOr(flags, SA_FLAG_OVERFLOW);
    }
    if (over) return;
    for (int c = tid; c < C; c += 1024) {
        long run = seg_clampl(counts[c], 0, cap), gt = 0;
        for (int b = 0; b < B; ++b) {
            ws_base[(long)b * C + c] = (int)run;
            run += seg_clampl(ws_dcount[(long)b * C + c], 0, dcap);
            gt += max(ws_gcount[(long)b * C + c], 0);
        }
        counts[c] = (int)run;
        n_gt[c] = (int)min((long)n_gt[c] + gt, 0x7fffffffL);
    }
}

// grid (B * C), one wave each
__global__ __launch_bounds__(64) void segap_copy_kernel(const float* __restrict__ dscore, const unsigned char* __restrict__ tp,
                                                        const int* __restrict__ ws_dstart, const int* __restrict__ ws_dcount,
                                                        const int* __restrict__ ws_base, const int* __restrict__ ws_fit, float* __restrict__ scores,
                                                        unsigned char* __restrict__ tps, int C, int score_col, long dcap, long cap) {
    if (ws_fit[0] != 1) return;
    const long grp = blockIdx.x;
    const int c = (int)(grp % C);
    const long d0 = seg_clampl(ws_dstart[grp], 0, dcap);
    const long nd = seg_clampl(ws_dcount[grp], 0, dcap - d0);
    const long base = seg_clampl(ws_base[grp], 0, cap);
    for (long i = threadIdx.x; i < nd && base + i < cap; i += 64) {
        const long dst = (long)c * cap + base + i;
        scores[dst] = dscore[2 * (d0 + i) + score_col];
        tps[dst] = tp[d0 + i];
    }
}

// grid (C, n_thr).  A thread owns SA_RPT consecutive rows of a tile; the true positives in front of them: a scan of the threads' counts
// on top of the count the earlier tiles left (the walk of ap_reduce_kernel, on bit k).
__global__ __launch_bounds__(SA_RTHREADS) void segap_reduce_kernel(const unsigned char* __restrict__ sorted_tps, const int* __restrict__ counts,
                                                                   const int* __restrict__ n_gt, float* __restrict__ ap, int C, long cap) {
    __shared__ unsigned wtot[SA_RTHREADS / 64];
    __shared__ double wsum[SA_RTHREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x, k = blockIdx.y;
    const unsigned char* tg = sorted_tps + (long)c * cap;
    const long n = seg_clampl(counts[c], 0, cap);
    unsigned seen = 0u;
    double acc = 0.0;
    for (long base = 0; base < n; base += SA_RTILE) {
        const long e0 = base + (long)tid * SA_RPT;
        unsigned bits = 0u;
#pragma unroll
        for (int i = 0; i < SA_RPT; ++i)
            if (e0 + i < n) bits |= (unsigned)((tg[e0 + i] >> k) & 1) << i;
        const unsigned own = (unsigned)__popc(bits);
        unsigned incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned front = seen, all = 0u;
#pragma unroll
        for (int w = 0; w < SA_RTHREADS / 64; ++w) {
            const unsigned x = wtot[w];
            if (w < wave) front += x;
            all += x;
        }
        unsigned t = front + incl - own;
        for (int i = 0; i < SA_RPT; ++i) {                                 // row order
            if ((bits >> i) & 1u) {
                ++t;
                acc += (double)t / (double)(e0 + i + 1);
            }
        }
        seen += all;
        __syncthreads();                                                   // wtot is rewritten by the next tile
    }
    acc = cfn_wave_sum_d(acc);                                             // a fixed butterfly, then the wave sums in wave order
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < SA_RTHREADS / 64; ++w) s += wsum[w];
        const int g = n_gt[c];
        ap[(long)k * C + c] = g > 0 ? (float)(s / (double)g) : 0.0f;
    }
}

// one wave: lane k sums ap[k, :] over the classes with ground truth, in class order
__global__ __launch_bounds__(64) void segap_map_kernel(const float* __restrict__ ap, const int* __restrict__ n_gt, float* __restrict__ map, int C,
                                                       int n_thr) {
    const int k = threadIdx.x;
    if (k >= n_thr) return;
    double s = 0.0;
    int cnt = 0;
    for (int c = 0; c < C; ++c)
        if (n_gt[c] > 0) { s += (double)ap[(long)k * C + c]; ++cnt; }
    map[k] = cnt > 0 ? (float)(s / (double)cnt) : 0.0f;
}

static inline bool sa_shape_ok(int B, int C, long det_cap, long n_seg) {
    return B >= 1 && C >= 1 && B <= 65535 && C <= 65535 && (long)B * C < (1L << 31) && det_cap >= 1 && det_cap < (1L << 31) && n_seg >= 1 &&
           n_seg < (1L << 31);
}

extern "C" long cfn_segap_workspace_bytes(int B, int C, long det_cap, long n_seg) {
    if (!sa_shape_ok(B, C, det_cap, n_seg)) return -1;
    return sa_ws_ints((long)B * C, det_cap) * 4 + ((n_seg + 7) & ~7L);
}

extern "C" int cfn_segap_gt_tile(void) { return SA_GT_TILE; }
extern "C" int cfn_segap_det_tile(void) { return SA_DET_TILE; }

extern "C" int cfn_segap_match(const double* det_seg, const float* det_score, const int* det_offsets, const double* seg, const int* offsets,
                               const double* fps, const int* window, const double* tiou, unsigned char* tp, int* match, void* workspace, int B, int C,
                               int t_max, int n_thr, int score_col, long det_cap, long n_seg, void* stream) {
    const char* what = "cfn_segap_match";
    CFN_REQUIRE(det_seg && det_score && det_offsets && seg && offsets && fps && window && tiou && tp && workspace, "%s: null tensor", what);
    CFN_REQUIRE(sa_shape_ok(B, C, det_cap, n_seg), "%s: bad shape (B %d, C %d <= 65535; det_cap %ld, n_seg %ld in [1, 2^31))", what, B, C, det_cap, n_seg);
    CFN_REQUIRE(t_max >= 1, "%s: t_max >= 1 expected, got %d", what, t_max);
    CFN_REQUIRE(n_thr >= 1 && n_thr <= SA_MAX_THR, "%s: n_thr in [1, %d] expected, got %d", what, SA_MAX_THR, n_thr);
    CFN_REQUIRE(score_col == 0 || score_col == 1, "%s: score_col 0 (max) or 1 (mean) expected, got %d", what, score_col);
    CFN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace on an 8-byte boundary expected", what);
    hipStream_t st = (hipStream_t)stream;
    const long groups = (long)B * C;
    const SaWs w = sa_carve(workspace, groups, det_cap);
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(segap_match_kernel, dim3((unsigned)groups), dim3(64), 0, st, det_seg, det_score, det_offsets, seg, offsets, fps, window, tiou, tp,
                       match, w.dstart, w.dcount, w.gcount, w.order, w.used, C, t_max, n_thr, score_col, det_cap, n_seg);
    return cfn_launch_ok(what);
}

extern "C" int cfn_segap_append(const float* det_score, const unsigned char* tp, void* workspace, float* scores, unsigned char* tps, int* counts,
                                int* n_gt, int* flags, int B, int C, int score_col, long det_cap, long cap, void* stream) {
    const char* what = "cfn_segap_append";
    CFN_REQUIRE(det_score && tp && workspace && scores && tps && counts && n_gt && flags, "%s: null tensor", what);
    CFN_REQUIRE(sa_shape_ok(B, C, det_cap, 1), "%s: bad shape (B %d, C %d <= 65535; det_cap %ld in [1, 2^31))", what, B, C, det_cap);
    CFN_REQUIRE(cap >= 1 && cap < (1L << 31), "%s: bad shape (cap %ld in [1, 2^31))", what, cap);
    CFN_REQUIRE(score_col == 0 || score_col == 1, "%s: score_col 0 (max) or 1 (mean) expected, got %d", what, score_col);
    CFN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace on an 8-byte boundary expected", what);
    hipStream_t st = (hipStream_t)stream;
    const long groups = (long)B * C;
    const SaWs w = sa_carve(workspace, groups, det_cap);
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(segap_plan_kernel, dim3(1), dim3(1024), 0, st, (const int*)w.dcount, (const int*)w.gcount, w.base, w.fit, counts, n_gt, flags, B, C,
                       det_cap, cap);
    hipLaunchKernelGGL(segap_copy_kernel, dim3((unsigned)groups), dim3(64), 0, st, det_score, tp, (const int*)w.dstart, (const int*)w.dcount,
                       (const int*)w.base, (const int*)w.fit, scores, tps, C, score_col, det_cap, cap);
    return cfn_launch_ok(what);
}

extern "C" int cfn_segap_reduce(const unsigned char* sorted_tps, const int* counts, const int* n_gt, float* ap, float* map, int C, int n_thr, long cap,
                                void* stream) {
    const char* what = "cfn_segap_reduce";
    CFN_REQUIRE(sorted_tps && counts && n_gt && ap && map, "%s: null tensor", what);
    CFN_REQUIRE(C >= 1 && C <= 65535 && cap >= 1 && cap < (1L << 31), "%s: bad shape (C %d in [1, 65535], cap %ld in [1, 2^31))", what, C, cap);
    CFN_REQUIRE(n_thr >= 1 && n_thr <= SA_MAX_THR, "%s: n_thr in [1, %d] expected, got %d", what, SA_MAX_THR, n_thr);
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(segap_reduce_kernel, dim3((unsigned)C, (unsigned)n_thr), dim3(SA_RTHREADS), 0, st, sorted_tps, counts, n_gt, ap, C, cap);
    hipLaunchKernelGGL(segap_map_kernel, dim3(1), dim3(64), 0, st, (const float*)ap, n_gt, map, C, n_thr);
    return cfn_launch_ok(what);
}
