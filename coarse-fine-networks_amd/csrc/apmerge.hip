// Merge class-major AP stores (cfn_hip/apmerge.py): append R source stores behind the rows a destination store holds, in part order, under
// cfn_ap_append's all-or-nothing rule.  The frame meter (apmeter.DeviceAPMeter: ONE count for all classes) and the segment meter
// (cfn_hip/segap.py SegmentAPMeter: one count per class plus n_gt) keep one layout, so one kernel family with a count stride serves both, as
// cfn_ap_sort_counts does for the sort.  The rule, stated once (merge_reference of cfn_hip/apmerge.py spells the same in numpy):
//
//   destination  scores (C, cap_d) fp32, payload (C, cap_d) uint8, counts (n_cnt) int32 with n_cnt == 1 (one count for all classes) or C,
//                extra (n_extra) int32 (additive integers carried along: n_gt of segment AP; n_extra == 0: none), ONE flags word.
//   sources      R >= 1 parts: scores (R, C, cap_s), payload (R, C, cap_s), counts (R, n_cnt), extra (R, n_extra), flags (R).  Sources and
//                destination do not overlap.
//   M1. a source count outside [0, cap_s] makes the call a refusal: nothing is written, no count or extra changes, flag bit 2 (value 4,
//       "malformed source") is set.
//   M2. totals in 64-bit integers: tot[c] = counts_d[c] + sum_r counts_s[r][c].  Any tot[c] > cap_d (or a destination count below 0): a
//       refusal, nothing is written, nothing changes, the overflow bit (value 2) is set.  Any summed extra that leaves int32: the same.
//   M3. otherwise row i of part r, class c goes to destination row counts_d[c] + sum_{q<r} counts_s[q][c] + i; scores and payload are copied
//       as BITS (NaN payloads, -0.0 and denormals stay as they are); counts and extras advance by the sums; rows behind the new counts are
//       untouched.
//   M4. in every case, refusals included, flags |= OR_r flags_s[r]: a batch dropped on any rank taints the merged value.
//   The destination is then, bit for bit, the store of one meter that was fed the destination's batches, then part 0's, then part 1's, ...
//
// Two launches, ordered by the stream alone (no atomics, no allocation, no synchronisation, no read-back):
//   plan   one workgroup: validates (M1), takes the per-count prefix sums over the parts into the workspace (base and clamped count of every
//          (part, count)), decides refusal (M2) and commits counts, extras and flags (M3, M4).  Every destination count is read before one is
//          advanced (a barrier stands in between).
//   copy   grid (tile of cap_s, class, part), AM_TILE rows per workgroup; it reads ONLY the workspace's verdict, bases and counts -- never the
//          destination counts, which plan has already advanced.  Tiles behind a part's count exit, so the grid depends on no device value.
//          Scores go as whole dwords, as 16-byte vectors where source and destination share their phase within 16 bytes.  The payload
//          offset of a class is arbitrary: head and tail bytes up to the destination's 4-byte boundaries are stored singly, the body goes as
//          destination-aligned dwords -- loaded whole where the source shares the phase, funnel-shifted from two aligned source dwords where
//          both lie inside the tile's source rows, and assembled from four source bytes otherwise (the edge dwords: nothing outside the
//          rows is ever read).  Bases and counts are clamped where they are read back: a damaged workspace gives wrong values, never a
//          store outside the destination.
#include "cfn_common.h"

#define AM_FLAG_OVERFLOW 2
#define AM_FLAG_BAD_SOURCE 4
#define AM_TILE 2048
#define AM_THREADS 256
#define AM_PTHREADS 1024

// workspace: int32 verdict [2] (verdict[0] == 1: copy; [1] pads to 8 bytes), base [R * n_cnt], cnt [R * n_cnt]
static inline long am_ws_bytes(long R, long C) { return 8 + 8 * R * C; }

__device__ __forceinline__ long am_clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bitwise OR over the workgroup (whole waves); every thread calls it
__device__ __forceinline__ int am_block_or(int v, int* s_wave) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    int all = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) all |= s_wave[i];
    return all;
}

__global__ __launch_bounds__(AM_PTHREADS) void ap_merge_plan_kernel(int* __restrict__ counts_d, int* __restrict__ extra_d, int* __restrict__ flags_d,
                                                                    const int* __restrict__ counts_s, const int* __restrict__ extra_s,
                                                                    const int* __restrict__ flags_s, int* __restrict__ ws, int R, int n_cnt,
                                                                    int n_extra, long cap_s, long cap_d) {
    __shared__ int s_wave[AM_PTHREADS / 64];
    const int tid = threadIdx.x;
    int* __restrict__ ws_base = ws + 2;
    int* __restrict__ ws_cnt = ws_base + (long)R * n_cnt;
    int bad = 0, over = 0, fl = 0;
    for (int j = tid; j < n_cnt; j += AM_PTHREADS) {
        const long d = counts_d[j];
        long tot = d;
        for (int r = 0; r < R; ++r) {
            const long s = counts_s[(long)r * n_cnt + j];
            if (s < 0 || s > cap_s) bad = 1;
            tot += am_clampl(s, 0, cap_s);                                 // (R * cap_s < 2^47: no wrap; the sum is moot when bad)
        }
        if (d < 0 || tot > cap_d) over = 1;
    }
    for (int e = tid; e < n_extra; e += AM_PTHREADS) {
        long tot = extra_d[e];
        for (int r = 0; r < R; ++r) tot += extra_s[(long)r * n_extra + e];
        if (tot < -2147483648L || tot > 2147483647L) over = 1;
    }
    for (int r = tid; r < R; r += AM_PTHREADS) fl |= flags_s[r];
    bad = __syncthreads_or(bad);
    over = __syncthreads_or(over);                                         // (also: every count and extra has been read before one is advanced)
    fl = am_block_or(fl, s_wave);
    const bool commit = !bad && !over;
    if (tid == 0) {
        ws[0] = commit ? 1 : 0;
        ws[1] = 0;
        flags_d[0] = flags_d[0] | fl | (bad ? AM_FLAG_BAD_SOURCE : (over ? AM_FLAG_OVERFLOW : 0));   // one thread, a plain store: no atomic
    }
    if (!commit) return;
    for (int j = tid; j < n_cnt; j += AM_PTHREADS) {
        long run = counts_d[j];
        for (int r = 0; r < R; ++r) {
            const int s = counts_s[(long)r * n_cnt + j];
            ws_base[(long)r * n_cnt + j] = (int)run;
            ws_cnt[(long)r * n_cnt + j] = s;
            run += s;
        }
        counts_d[j] = (int)run;
    }
    for (int e = tid; e < n_extra; e += AM_PTHREADS) {
        long tot = extra_d[e];
        for (int r = 0; r < R; ++r) tot += extra_s[(long)r * n_extra + e];
        extra_d[e] = (int)tot;
    }
}

// grid (tiles of cap_s, C, R)
__global__ __launch_bounds__(AM_THREADS) void ap_merge_copy_kernel(unsigned* __restrict__ dst_scores, unsigned char* __restrict__ dst_payload,
                                                                   const unsigned* __restrict__ src_scores,
                                                                   const unsigned char* __restrict__ src_payload, const int* __restrict__ ws, int R,
                                                                   int C, int n_cnt, long cap_s, long cap_d) {
    if (ws[0] != 1) return;
    const int c = blockIdx.y, r = blockIdx.z, tid = threadIdx.x;
    const long slot = (long)r * n_cnt + (n_cnt == 1 ? 0 : c);
    const long base = am_clampl(ws[2 + slot], 0, cap_d);
    const long n = am_clampl(ws[2 + (long)R * n_cnt + slot], 0, min(cap_s, cap_d - base));
    const long row0 = (long)blockIdx.x * AM_TILE;
    if (row0 >= n) return;
    const int len = (int)min((long)AM_TILE, n - row0);
    const long so = ((long)r * C + c) * cap_s + row0, dofs = (long)c * cap_d + base + row0;

    // scores: dwords; 16-byte vectors where both sides share the phase
    {
        const unsigned* __restrict__ S = src_scores + so;
        unsigned* __restrict__ D = dst_scores + dofs;
        if ((((uintptr_t)S ^ (uintptr_t)D) & 15) == 0) {
            const int head = min(len, (int)(((16 - ((uintptr_t)D & 15)) & 15) >> 2));
            const int nv = (len - head) >> 2;
            if (tid < head) D[tid] = S[tid];
            const uint4* __restrict__ S4 = (const uint4*)(S + head);
            uint4* __restrict__ D4 = (uint4*)(D + head);
            for (int v = tid; v < nv; v += AM_THREADS) D4[v] = S4[v];
            const int done = head + 4 * nv;
            if (tid < len - done) D[done + tid] = S[done + tid];
        } else {
            for (int i = tid; i < len; i += AM_THREADS) D[i] = S[i];
        }
    }
    // payload: head and tail bytes singly, the body as destination-aligned dwords
    {
        const unsigned char* __restrict__ S = src_payload + so;
        unsigned char* __restrict__ D = dst_payload + dofs;
        const int head = min(len, (int)((4 - ((uintptr_t)D & 3)) & 3));
        const int nw = (len - head) >> 2;
        if (tid < head) D[tid] = S[tid];
        const unsigned char* __restrict__ Sb = S + head;                   // the body's first source byte
        unsigned* __restrict__ Dw = (unsigned*)(D + head);
        const int a = (int)((uintptr_t)Sb & 3);
        if (a == 0) {
            const unsigned* __restrict__ Sw = (const unsigned*)Sb;
            for (int w = tid; w < nw; w += AM_THREADS) Dw[w] = Sw[w];
        } else {
            const unsigned* __restrict__ Sw = (const unsigned*)(Sb - a);   // aligned; dword w of the body spans Sw[w] and Sw[w + 1]
            const int sh = 8 * a;
            for (int w = tid; w < nw; w += AM_THREADS) {
                const unsigned char* p = Sb + 4 * w;
                unsigned x;
                if (p - a >= S && p - a + 8 <= S + len) {                  // both aligned dwords inside the tile's source rows
                    x = (Sw[w] >> sh) | (Sw[w + 1] << (32 - sh));
                } else {
                    x = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
                }
                Dw[w] = x;
            }
        }
        const int done = head + 4 * nw;
        if (tid < len - done) D[done + tid] = S[done + tid];
    }
}

static inline bool am_shape_ok(int R, int C) { return R >= 1 && R <= 65535 && C >= 1 && C <= 65535; }

extern "C" long cfn_ap_merge_workspace_bytes(int R, int C) {
    if (!am_shape_ok(R, C)) return -1;
    return am_ws_bytes(R, C);
}

extern "C" int cfn_ap_merge_tile(void) { return AM_TILE; }

extern "C" int cfn_ap_merge(float* dst_scores, unsigned char* dst_payload, int* dst_counts, int* dst_extra, int* dst_flags, const float* src_scores,
                            const unsigned char* src_payload, const int* src_counts, const int* src_extra, const int* src_flags, void* workspace,
                            int R, int C, int n_cnt, int n_extra, long cap_s, long cap_d, void* stream) {
    const char* what = "cfn_ap_merge";
    CFN_REQUIRE(dst_scores && dst_payload && dst_counts && dst_flags && src_scores && src_payload && src_counts && src_flags && workspace,
                "%s: null tensor", what);
    CFN_REQUIRE(am_shape_ok(R, C), "%s: bad shape (R %d, C %d in [1, 65535])", what, R, C);
    CFN_REQUIRE(cap_s >= 1 && cap_s < (1L << 31) && cap_d >= 1 && cap_d < (1L << 31), "%s: bad shape (cap_s %ld, cap_d %ld in [1, 2^31))", what, cap_s,
                cap_d);
    CFN_REQUIRE(n_cnt == 1 || n_cnt == C, "%s: n_cnt 1 (one count for all classes) or C = %d expected, got %d", what, C, n_cnt);
    CFN_REQUIRE(n_extra >= 0, "%s: n_extra >= 0 expected, got %d", what, n_extra);
    CFN_REQUIRE(n_extra == 0 || (dst_extra && src_extra), "%s: null extra with n_extra %d", what, n_extra);
    CFN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace on an 8-byte boundary expected", what);
    CFN_REQUIRE((((uintptr_t)dst_scores | (uintptr_t)src_scores) & 3) == 0, "%s: scores on 4-byte boundaries expected", what);
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(ap_merge_plan_kernel, dim3(1), dim3(AM_PTHREADS), 0, st, dst_counts, dst_extra, dst_flags, src_counts, src_extra, src_flags,
                       (int*)workspace, R, n_cnt, n_extra, cap_s, cap_d);
    const unsigned tiles = (unsigned)((cap_s + AM_TILE - 1) / AM_TILE);
    hipLaunchKernelGGL(ap_merge_copy_kernel, dim3(tiles, (unsigned)C, (unsigned)R), dim3(AM_THREADS), 0, st, (unsigned*)dst_scores, dst_payload,
                       (const unsigned*)src_scores, src_payload, (const int*)workspace, R, C, n_cnt, cap_s, cap_d);
    return cfn_launch_ok(what);
}
