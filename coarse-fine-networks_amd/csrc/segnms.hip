// Temporal non-maximum suppression of a batch's Detections (cfn_hip/detections.py nms / nms_reference): the stage between the level decode
// (csrc/detections.hip, cfn_decode_segments_levels) and the writer / the segment-AP meter.  The rules (cfn_hip/detections.py spells the same):
//
//   N1. groups are (video, class) row ranges: the rows offsets[b] .. offsets[b + 1] (clamped to [0, cap_in]) whose class column is c, found by
//       two binary searches on the class column (seg_group of seg_common.h; the class column does not decrease inside a video).
//   N2. order inside a group: score[:, score_col] descending (fp32), ties by row index ascending (segap.py rule 3).  A NaN score ranks as
//       -inf, so the ranks are a permutation of the group whatever the data (seg_nan_low and seg_rank of seg_common.h).
//   N3. tIoU of (s0, e0) and (s1, e1): inter = min(e0, e1) - max(s0, s1); 0 unless inter > 0, otherwise inter / ((e0 - s0) + (e1 - s1) - inter):
//       plain IEEE fp64, no product, ONE division (segap.py rule 2; seg_tiou of seg_common.h).
//   N4. greedy: walk the group in the order of N2; a candidate is KEPT iff no candidate kept before it has tIoU with it > nms_thr (strict).  A
//       suppressed candidate suppresses nothing.
//   N5. the output is a stable compaction: kept rows in their input order, seg / frames / score copied bit for bit; offsets and total are the
//       true counts, rows >= cap_out are not written.
//   N6. keep (cap_in) uint8 (written for the rows of the batch's groups only) and src (cap_out) int32 = the input row of each output row.
//
// Three launches, ordered by the stream alone; no atomics, no allocation, nothing is read back:
//   select   one wave per group.  Rank by counting (O(nd^2 / 64), seg_rank).  The walk: the candidate at rank r is skipped if its
//            suppressed flag is set; otherwise it is kept and the lanes take the ranks above r, 64 at a time in tiles aligned to 64, and set
//            the flag where the tIoU is above nms_thr: O(kept * nd / 64).  The flag of rank j belongs to lane j & 63 and to no other: a lane
//            reads back only what it wrote itself, the flag of rank r reaches the wave through a ballot.  Up to NMS_DET_TILE = 1024 candidates
//            the start / end (in rank order), the scores and the order live in LDS and the flags in one register per lane (16 bits); a larger
//            group (the general path) keeps its order and its flag bytes in the workspace: the ORDER is written by one lane and read by
//            others, so it passes a release / acquire fence pair around the barrier (see seg_rank); the flags stay lane-owned.
//   scan     one workgroup: the groups' kept counts -> bases in place, offsets[b], total (seg_launch_scan of seg_common.h).
//   write    one wave per group: 64 rows at a time, a kept row goes to base + the number of kept rows in front of it (ballot / popcount).
// offsets, classes, ranks and counts are DATA: every index is clamped, so a bad batch gives wrong values, never a store outside the outputs.
#include "seg_common.h"

#define NMS_DET_TILE 1024
#define NMS_FLAG_WORDS (NMS_DET_TILE / 64)

// grid (B * C), one wave each
__global__ __launch_bounds__(64) void nms_select_kernel(const double* __restrict__ seg, const float* __restrict__ score, const int* __restrict__ offsets,
                                                        unsigned char* __restrict__ keep, int* __restrict__ counts, int* __restrict__ ws_order,
                                                        unsigned char* __restrict__ ws_flag, int C, int score_col, double nms_thr, long cap_in) {
    __shared__ double s_start[NMS_DET_TILE];                               // in rank order
    __shared__ double s_end[NMS_DET_TILE];
    __shared__ float s_key[NMS_DET_TILE];                                  // in row order
    __shared__ int s_order[NMS_DET_TILE];                                  // rank -> row of the group
    const int lane = threadIdx.x;
    const long grp = blockIdx.x;
    const int b = (int)(grp / C), c = (int)(grp - (long)b * C);
    int nd;
    const long d0 = seg_group(seg, offsets, b, c, cap_in, nd);
    if (nd <= 0) {
        if (lane == 0) counts[grp] = 0;
        return;
    }

    if (nd <= NMS_DET_TILE) {
        for (int i = lane; i < nd; i += 64) s_key[i] = seg_nan_low(score[2 * (d0 + i) + score_col]);
        __syncthreads();
        for (int i = lane; i < nd; i += 64) {                              // rule N2: rank by counting, a permutation
            const int r = seg_rank([&](int j) { return s_key[j]; }, i, nd);
            s_order[r] = i;
            s_start[r] = seg[3 * (d0 + i) + 1];
            s_end[r] = seg[3 * (d0 + i) + 2];
        }
        __syncthreads();
        unsigned sup = 0u;                                                 // bit t: rank 64 * t + lane is suppressed
        for (int r = 0; r < nd; ++r) {                                     // rule N4 (r and everything derived from it are wave uniform)
            const unsigned owner = (unsigned)__shfl((int)sup, r & 63, 64);
            if ((owner >> (r >> 6)) & 1u) continue;
            const double s0 = s_start[r], e0 = s_end[r];
            for (int t = (r + 1) >> 6; 64 * t < nd; ++t) {
                const int j = 64 * t + lane;
                if (j > r && j < nd && seg_tiou(s0, e0, s_start[j], s_end[j]) > nms_thr) sup |= 1u << t;
            }
        }
        int kept = 0;
        for (int t = 0; 64 * t < nd; ++t) {
            const int j = 64 * t + lane;
            const bool k = j < nd && !((sup >> t) & 1u);
            if (j < nd) keep[d0 + min(max(s_order[j], 0), nd - 1)] = k ? 1 : 0;
            kept += __popcll(__ballot(k));
        }
        if (lane == 0) counts[grp] = kept;
        return;
    }

    // the general path: order and flags in the workspace (the group's own range [d0, d0 + nd) of both)
    int* order = ws_order + d0;
    unsigned char* flag = ws_flag + d0;
    for (int i = lane; i < nd; i += 64) {
        order[seg_rank([&](int j) { return seg_nan_low(score[2 * (d0 + j) + score_col]); }, i, nd)] = i;
        flag[i] = 0;                                                       // (rank i's flag: lane i & 63 = this lane owns it)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                     // the other lanes' ranks are read back through memory
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int r = 0; r < nd; ++r) {
        const bool mine = lane == (r & 63) && flag[r] != 0;
        if (__ballot(mine)) continue;
        const long ri = d0 + min(max(order[r], 0), nd - 1);
        const double s0 = seg[3 * ri + 1], e0 = seg[3 * ri + 2];
        for (int j = ((r + 1) >> 6) * 64 + lane; j < nd; j += 64) {
            if (j <= r || flag[j]) continue;
            const long rj = d0 + min(max(order[j], 0), nd - 1);
            if (seg_tiou(s0, e0, seg[3 * rj + 1], seg[3 * rj + 2]) > nms_thr) flag[j] = 1;
        }
    }
    int kept = 0;
    for (int j0 = 0; j0 < nd; j0 += 64) {
        const int j = j0 + lane;
        const bool k = j < nd && flag[j] == 0;
        if (j < nd) keep[d0 + min(max(order[j], 0), nd - 1)] = k ? 1 : 0;
        kept += __popcll(__ballot(k));
    }
    if (lane == 0) counts[grp] = kept;
}

// grid (B * C), one wave each: the stable compaction of rules N5 / N6 and S6.  FINALS (Soft-NMS): column score_col of the output comes from
// ws_final, the other column and everything else are copied; otherwise both score columns are copied (ws_final and score_col are not read)
template <bool FINALS>
__global__ __launch_bounds__(64) void nms_write_kernel(const double* __restrict__ seg, const int* __restrict__ frames, const float* __restrict__ score,
                                                       const int* __restrict__ offsets, const unsigned char* __restrict__ keep,
                                                       const int* __restrict__ bases, const float* __restrict__ ws_final, double* __restrict__ out_seg,
                                                       int* __restrict__ out_frames, float* __restrict__ out_score, int* __restrict__ src, int C,
                                                       int score_col, long cap_in, long cap_out) {
    const int lane = threadIdx.x;
    const long grp = blockIdx.x;
    long base = bases[grp];
    if (bases[grp + 1] - base <= 0 || base < 0 || base >= cap_out) return; // (wave uniform) nothing kept, or all of it behind cap_out
    const int b = (int)(grp / C), c = (int)(grp - (long)b * C);
    int nd;
    const long d0 = seg_group(seg, offsets, b, c, cap_in, nd);
    for (int i0 = 0; i0 < nd && base < cap_out; i0 += 64) {
        const long i = d0 + i0 + lane;
        const bool k = i0 + lane < nd && keep[i] != 0;
        const unsigned long long m = __ballot(k);
        const long dst = base + __popcll(m & ((1ull << lane) - 1));
        if (k && dst < cap_out) {
            out_seg[3 * dst + 0] = seg[3 * i + 0]; out_seg[3 * dst + 1] = seg[3 * i + 1]; out_seg[3 * dst + 2] = seg[3 * i + 2];
            out_frames[3 * dst + 0] = frames[3 * i + 0]; out_frames[3 * dst + 1] = frames[3 * i + 1]; out_frames[3 * dst + 2] = frames[3 * i + 2];
            if (FINALS) {
                out_score[2 * dst + score_col] = ws_final[i];
                out_score[2 * dst + 1 - score_col] = score[2 * i + 1 - score_col];
            } else {
                out_score[2 * dst + 0] = score[2 * i + 0]; out_score[2 * dst + 1] = score[2 * i + 1];
            }
            src[dst] = (int)i;
        }
        base += __popcll(m);
    }
}

static inline bool nms_shape_ok(int B, int C, long cap_in) {
    return B >= 1 && C >= 1 && B <= 65535 && C <= 65535 && (long)B * C < (1L << 31) && cap_in >= 1 && cap_in < (1L << 31);
}

// workspace: int32 counts / bases [B * C + 1], order [cap_in]; then cap_in flag bytes
static inline long nms_ws_ints(long groups, long cap_in) { return groups + 1 + cap_in; }

extern "C" long cfn_nms_segments_workspace_bytes(int B, int C, long cap_in) {
    if (!nms_shape_ok(B, C, cap_in)) return -1;
    return nms_ws_ints((long)B * C, cap_in) * 4 + ((cap_in + 7) & ~7L);
}

extern "C" int cfn_nms_det_tile(void) { return NMS_DET_TILE; }

// the argument checks that cfn_nms_segments and cfn_soft_nms_segments share
static int nms_check(const char* what, const void* seg, const void* frames, const void* score, const void* offsets, const void* out_seg,
                     const void* out_frames, const void* out_score, const void* out_offsets, const void* out_total, const void* keep, const void* src,
                     const void* workspace, int B, int C, int score_col, double nms_thr, long cap_in, long cap_out) {
    CFN_REQUIRE(seg && frames && score && offsets && out_seg && out_frames && out_score && out_offsets && out_total && keep && src && workspace,
                "%s: null tensor", what);
    CFN_REQUIRE(nms_shape_ok(B, C, cap_in), "%s: bad shape (B %d, C %d in [1, 65535]; cap_in %ld in [1, 2^31))", what, B, C, cap_in);
    CFN_REQUIRE(cap_out >= 1 && cap_out < (1L << 31), "%s: cap_out in [1, 2^31) expected, got %ld", what, cap_out);
    CFN_REQUIRE(score_col == 0 || score_col == 1, "%s: score_col 0 (max) or 1 (mean) expected, got %d", what, score_col);
    CFN_REQUIRE(nms_thr >= 0.0 && nms_thr <= 1.0, "%s: nms_thr in [0, 1] expected, got %g", what, nms_thr);
    CFN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace on an 8-byte boundary expected", what);
    CFN_REQUIRE(seg != out_seg && frames != out_frames && score != out_score, "%s: the outputs must not be the inputs", what);
    return CFN_OK;
}

extern "C" int cfn_nms_segments(const double* seg, const int* frames, const float* score, const int* offsets, double* out_seg, int* out_frames,
                                float* out_score, int* out_offsets, int* out_total, unsigned char* keep, int* src, void* workspace, int B, int C,
                                int score_col, double nms_thr, long cap_in, long cap_out, void* stream) {
    const char* what = "cfn_nms_segments";
    if (const int bad = nms_check(what, seg, frames, score, offsets, out_seg, out_frames, out_score, out_offsets, out_total, keep, src, workspace, B, C,
                                  score_col, nms_thr, cap_in, cap_out))
        return bad;
    hipStream_t st = (hipStream_t)stream;
    const long groups = (long)B * C;
    int* counts = (int*)workspace;
    int* order = counts + groups + 1;
    unsigned char* flag = (unsigned char*)(order + cap_in);
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(nms_select_kernel, dim3((unsigned)groups), dim3(64), 0, st, seg, score, offsets, keep, counts, order, flag, C, score_col, nms_thr, cap_in);
    seg_launch_scan(counts, out_offsets, out_total, groups, B, C, cap_in, st);
    hipLaunchKernelGGL(nms_write_kernel<false>, dim3((unsigned)groups), dim3(64), 0, st, seg, frames, score, offsets, (const unsigned char*)keep,
                       (const int*)counts, (const float*)nullptr, out_seg, out_frames, out_score, src, C, score_col, cap_in, cap_out);
    return cfn_check_launch(what);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Soft-NMS (cfn_hip/detections.py soft_nms / soft_nms_reference): nothing is deleted by overlap; a candidate's score is decayed by its
// overlap with every candidate ranked in front of it, and the list is cut by a score floor or a count.  The rules (cfn_hip/detections.py
// and include/cfn_hip.h spell the same):
//
//   S1. groups are rule N1's.
//   S2. row i gets w_i = (double)score[i, score_col]; a row whose score is NaN or infinite is out of the group from the start (never selected,
//       never decayed, keep 0).
//   S3. rounds: among the rows not yet selected, m = the one with the largest w, ties to the lowest row.  Stop when no row is left, when
//       !(w_m >= min_score), or when max_keep > 0 rows are already selected; otherwise m is selected and final_m = w_m.
//   S4. decay of every row j not yet selected, iou = tIoU(m, j) by rule N3:  linear: if iou > nms_thr (strict) w_j = w_j * (1.0 - iou);
//       gaussian: if iou > 0, w_j = w_j * E((iou * iou) / sigma).  One fp64 subtraction or one E, then one fp64 product, in selection order.
//   S5. E(t) = exp(-t) on [0, 64]: y = -(t * 2^-10); p = c8, p = p * y + c_k for k = 7 .. 0 with c_k = 1.0 / k! (one IEEE fp64 division);
//       p = p * p ten times; every product and sum rounded separately (no fused multiply-add), so the host computes the same double.
//   S6. the output is a stable compaction of the selected rows in input order: seg, frames and the other score column copied bit for bit,
//       score[:, score_col] = (float)final (round to nearest); offsets / total true counts; rows >= cap_out not written; keep and src as N6.
//
// Three launches, ordered by the stream alone; no atomics, no allocation, nothing is read back:
//   soft_select   one wave per group.  Candidate j belongs to lane j & 63 and to no other: only that lane reads or writes w_j, retires it
//                 (w_j = -inf: a working score is finite, so -inf marks "selected or out") and writes its keep byte and its final.  A round
//                 is a per-lane maximum over the lane's own entries (taken in the same pass that decays them), a wave reduction of the
//                 (w, row) pair by shuffles, which leaves m in every lane, and the pass over the own entries.  No barrier, no fence inside
//                 the rounds.  Up to NMS_DET_TILE candidates start, end and w live in LDS (24 KB; start and end are written once, before
//                 the one barrier in front of the rounds); a larger group keeps w in the workspace (8 bytes per candidate, still lane
//                 owned) and reads seg, which nobody writes, from memory.  O(selected * nd / 64) per group; max_keep bounds it.
//   scan          seg_launch_scan, as hard NMS.
//   write         nms_write_kernel<true>: column score_col from the finals.
#define SOFT_NONE 0x7fffffff

// rule S5 (the constants fold at compile time: one correctly rounded division each)
__device__ __forceinline__ double soft_decay_exp(double t) {
#pragma clang fp contract(off)
    const double y = -(t * 0x1p-10);
    double p = 1.0 / 40320.0;
    p = p * y + 1.0 / 5040.0;
    p = p * y + 1.0 / 720.0;
    p = p * y + 1.0 / 120.0;
    p = p * y + 1.0 / 24.0;
    p = p * y + 1.0 / 6.0;
    p = p * y + 1.0 / 2.0;
    p = p * y + 1.0 / 1.0;
    p = p * y + 1.0 / 1.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) p = p * p;
    return p;
}

// rule S4: the working score of a row behind the selected one
__device__ __forceinline__ double soft_decay(double w, double iou, int method, double nms_thr, double sigma) {
#pragma clang fp contract(off)
    if (method == 0) {
        if (iou > nms_thr) w = w * (1.0 - iou);
    } else if (iou > 0.0) {
        const double t = (iou * iou) / sigma;
        w = w * soft_decay_exp(t);
    }
    return w;
}

// rule S3's order on (w, row) pairs: the larger w, then the lower row; the same pair in every lane afterwards
__device__ __forceinline__ void soft_wave_max(double& w, int& j) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double ow = __shfl_xor(w, d, 64);
        const int oj = __shfl_xor(j, d, 64);
        const bool take = (ow > w) | ((ow == w) & (oj < j));              // (selects, not branches: the chain of six steps is the round's latency)
        w = take ? ow : w;
        j = take ? oj : j;
    }
}

// the rounds of one group of nd >= 1 candidates, rows d0 .. d0 + nd - 1 -> the number selected.  TILE: start, end and w in LDS (nd <= NMS_DET_TILE);
// otherwise w_own is the group's own range of the workspace and start / end are read from seg
template <bool TILE>
__device__ __forceinline__ int soft_group(const double* __restrict__ seg, const float* __restrict__ score, unsigned char* __restrict__ keep,
                                          float* __restrict__ fin, double* s_start, double* s_end, double* w_own, long d0, int nd, int score_col,
                                          int method, double nms_thr, double sigma, double min_score, int max_keep) {
    const int lane = threadIdx.x;
    // rule S2, and the first round's per-lane maximum
    double bw = -INFINITY;
    int bj = SOFT_NONE;
    for (int j = lane; j < nd; j += 64) {
        const float s = score[2 * (d0 + j) + score_col];
        const double w = (s - s == 0.0f) ? (double)s : -INFINITY;          // NaN - NaN and inf - inf are NaN
        w_own[j] = w;
        keep[d0 + j] = 0;
        if (TILE) {
            s_start[j] = seg[3 * (d0 + j) + 1];
            s_end[j] = seg[3 * (d0 + j) + 2];
        }
        if (w > bw) { bw = w; bj = j; }
    }
    if (TILE) __syncthreads();                                             // start / end of the other lanes' rows; nothing behind this line waits

    int selected = 0;
    for (int round = 0; round < nd; ++round) {                             // rule S3 (everything the branches look at is wave uniform)
        double mw = bw;
        int m = bj;
        soft_wave_max(mw, m);
        if (m == SOFT_NONE || !(mw >= min_score) || (max_keep > 0 && selected >= max_keep)) break;
        m = min(max(m, 0), nd - 1);
        if ((m & 63) == lane) {                                            // the owner retires it
            w_own[m] = -INFINITY;
            keep[d0 + m] = 1;
            fin[m] = (float)mw;
        }
        ++selected;
        const double s0 = TILE ? s_start[m] : seg[3 * (d0 + m) + 1];
        const double e0 = TILE ? s_end[m] : seg[3 * (d0 + m) + 2];
        bw = -INFINITY;
        bj = SOFT_NONE;
        for (int j = lane; j < nd; j += 64) {                              // rule S4 and the next round's per-lane maximum in one pass
            double w = w_own[j];
            if (!(w > -INFINITY)) continue;                                // selected, or out from the start
            const double s1 = TILE ? s_start[j] : seg[3 * (d0 + j) + 1];
            const double e1 = TILE ? s_end[j] : seg[3 * (d0 + j) + 2];
            w = soft_decay(w, seg_tiou(s0, e0, s1, e1), method, nms_thr, sigma);
            w_own[j] = w;
            if (w > bw) { bw = w; bj = j; }
        }
    }
    return selected;
}

// grid (B * C), one wave each
__global__ __launch_bounds__(64) void soft_select_kernel(const double* __restrict__ seg, const float* __restrict__ score, const int* __restrict__ offsets,
                                                         unsigned char* __restrict__ keep, int* __restrict__ counts, double* __restrict__ ws_w,
                                                         float* __restrict__ ws_final, int C, int score_col, int method, double nms_thr, double sigma,
                                                         double min_score, int max_keep, long cap_in) {
    __shared__ double s_start[NMS_DET_TILE];                               // in row order
    __shared__ double s_end[NMS_DET_TILE];
    __shared__ double s_w[NMS_DET_TILE];                                   // entry j: lane j & 63 only
    const long grp = blockIdx.x;
    const int b = (int)(grp / C), c = (int)(grp - (long)b * C);
    int nd;
    const long d0 = seg_group(seg, offsets, b, c, cap_in, nd);
    int selected = 0;
    if (nd > NMS_DET_TILE)                                                 // (wave uniform)
        selected = soft_group<false>(seg, score, keep, ws_final + d0, nullptr, nullptr, ws_w + d0, d0, nd, score_col, method, nms_thr, sigma, min_score,
                                     max_keep);
    else if (nd > 0)
        selected = soft_group<true>(seg, score, keep, ws_final + d0, s_start, s_end, s_w, d0, nd, score_col, method, nms_thr, sigma, min_score, max_keep);
    if (threadIdx.x == 0) counts[grp] = selected;
}

// workspace: fp64 working scores [cap_in]; then fp32 finals [cap_in] and int32 counts / bases [B * C + 1]; rounded up to 8 bytes
extern "C" long cfn_soft_nms_segments_workspace_bytes(int B, int C, long cap_in) {
    if (!nms_shape_ok(B, C, cap_in)) return -1;
    return cap_in * 8 + ((cap_in * 4 + ((long)B * C + 1) * 4 + 7) & ~7L);
}

extern "C" int cfn_soft_nms_segments(const double* seg, const int* frames, const float* score, const int* offsets, double* out_seg, int* out_frames,
                                     float* out_score, int* out_offsets, int* out_total, unsigned char* keep, int* src, void* workspace, int B, int C,
                                     int score_col, double nms_thr, int method, double sigma, double min_score, int max_keep, long cap_in, long cap_out,
                                     void* stream) {
    const char* what = "cfn_soft_nms_segments";
    CFN_REQUIRE(method == 0 || method == 1, "%s: method 0 (linear) or 1 (gaussian) expected, got %d", what, method);
    CFN_REQUIRE(sigma >= 0x1p-6 && sigma <= 0x1p20, "%s: sigma in [1/64, 2^20] expected, got %g", what, sigma);
    CFN_REQUIRE(min_score >= 0.0 && min_score <= 1.0, "%s: min_score in [0, 1] expected, got %g", what, min_score);
    CFN_REQUIRE(max_keep >= 0, "%s: max_keep >= 0 expected (0: no limit), got %d", what, max_keep);
    if (const int bad = nms_check(what, seg, frames, score, offsets, out_seg, out_frames, out_score, out_offsets, out_total, keep, src, workspace, B, C,
                                  score_col, nms_thr, cap_in, cap_out))
        return bad;
    hipStream_t st = (hipStream_t)stream;
    const long groups = (long)B * C;
    double* ws_w = (double*)workspace;
    float* ws_final = (float*)(ws_w + cap_in);
    int* counts = (int*)(ws_final + cap_in);
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(soft_select_kernel, dim3((unsigned)groups), dim3(64), 0, st, seg, score, offsets, keep, counts, ws_w, ws_final, C, score_col, method,
                       nms_thr, sigma, min_score, max_keep, cap_in);
    seg_launch_scan(counts, out_offsets, out_total, groups, B, C, cap_in, st);
    hipLaunchKernelGGL(nms_write_kernel<true>, dim3((unsigned)groups), dim3(64), 0, st, seg, frames, score, offsets, (const unsigned char*)keep, (const int*)counts,
                       (const float*)ws_final, out_seg, out_frames, out_score, src, C, score_col, cap_in, cap_out);
    return cfn_check_launch(what);
}
