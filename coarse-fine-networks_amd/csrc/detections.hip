// Activity segments from per-frame scores (cfn_hip/detections.py): the decode that every caller of the reference writes in Python behind
// train_fine.py:199-206 (threshold probs per class, find the runs, turn frames into seconds) as one device-side step, and the inverse of
// csrc/seglabels.hip: it writes [class, start_s, end_s] rows in the record layout of SegLabels.seg, and rasterising them again accepts
// exactly the frames of each run.  The definition (cfn_hip/detections.py decode_reference spells the same on the host):
//
//   1. frame t of row (b, c) is ACTIVE iff  t < min(valid_t[b], TL)  and  probs[b, c, t] > thr[c]     (fp32, strict: a NaN is never active)
//   2. two active frames t < u with only inactive frames between them and  u - t - 1 <= max_gap  are joined (the gap belongs to the run)
//   3. a segment is a maximal run [t0, t1] after 2 (both ends active); runs with t1 - t0 + 1 < min_len are dropped
//   4. start_s = ((double)(start[b] + t0) - 0.5) / fps[b],  end_s = ((double)(start[b] + t1) + 0.5) / fps[b]: one fp64 add and ONE IEEE fp64
//      division each (no reciprocal; this build has no fast-math flag).  The half frame outward is what seg_labels' strict inequalities need.
//   5. score_max = fp32 max, score_mean = (float)(fp64 sum / count) over the ACTIVE frames of the run only, n_active = that count
//   6. output order: lexicographic in (b, c, t0), from counts and prefix sums alone: bit-identical from run to run
//
// Three launches on one stream; order between them is launch order, no workgroup waits for another:
//   count   one workgroup (4 waves) per row.  A pass covers DS_PASS = 1024 frames: a wave loads 256 of them, 16 bytes per lane when the rows
//           are 16-byte aligned (TL % 4 == 0), and turns the four comparisons into four 64-bit mask words with __ballot (the 16-byte form
//           interleaves the ballots' bits: a 16 -> 64 bit spread on four lanes).  The mask (TL / 8 bytes per row) goes to LDS and to the
//           workspace.  A row without an active frame ends here.  Otherwise det_plan() marks run starts and ends per word (gap closing looks
//           at most max_gap / 64 + 1 words back / ahead and stops at the first word with a bit), scans the end counts, finds each start's end
//           (same word, or a binary search in the scanned counts) for min_len, and the row's count of kept runs goes to the workspace.
//   scan    one workgroup turns the B * C counts into row bases (in place), offsets[b] and total (seg_launch_scan of seg_common.h: NMS and
//           Soft-NMS launch the same kernel, which is defined here).
//   write   a row with a non-zero count loads its mask from the workspace, repeats det_plan(), scans the kept starts, and its waves take the
//           kept runs in turn: 64 frames per step, only active frames are read again, wave reductions (fp64 butterfly: a fixed order),
//           lane 0 stores the record at base + rank if that is < cap.
// valid_t, fps, start and thr are DATA read on the device; every index is derived from B, C, TL and the mask, so a bad batch gives wrong
// values, never an access outside the tensors.  LDS: 40 bytes per 64 frames (dynamic), 40 KB at TL = 65536.
//
// Levels (cfn_decode_segments_levels; the rules L1-L4 are in cfn_hip/detections.py): the same three kernels with a level count K.  A row is
// (b, c, k): it reads probs row / K against levels[row % (C * K)] (levels (C, K), row c = class c's thresholds in the caller's order), the
// scan's offsets boundary sits at C * K, and the write stores c in seg and k in level (cap) uint8.  Output order (b, c, k, t0);
// cfn_decode_segments is K = 1 without the level column: its results and its workspace are what they were.
#include "seg_common.h"

#define DS_THREADS 256
#define DS_PASS 1024                 // frames per pass of a workgroup (4 waves x 64 lanes x 4 frames)
#define DS_MAX_TL 65536

typedef float __attribute__((ext_vector_type(4))) ds_f4;
typedef unsigned long long ds_u64;

// bit i of the low 16 bits -> bit 4 * i
__device__ __forceinline__ ds_u64 ds_spread16(ds_u64 x) {
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

__device__ __forceinline__ ds_u64 ds_uni(ds_u64 v) {
    const unsigned lo = cfn_uni((unsigned)v), hi = cfn_uni((unsigned)(v >> 32));
    return ((ds_u64)hi << 32) | lo;
}

struct DsRow {                       // the row's words in LDS: masks [nwords], exclusive counts [nwords + 1]
    ds_u64 *M, *S, *E, *K;
    int *PE, *PK;
};

__device__ __forceinline__ DsRow ds_carve(unsigned char* smem, int nwords) {
    DsRow r;
    r.M = reinterpret_cast<ds_u64*>(smem);
    r.S = r.M + nwords; r.E = r.S + nwords; r.K = r.E + nwords;
    r.PE = reinterpret_cast<int*>(r.K + nwords);
    r.PK = r.PE + nwords + 1;
    return r;
}

static inline size_t ds_lds_bytes(int nwords) { return (size_t)nwords * 32 + (size_t)(nwords + 1) * 8; }

// last frame of the run that starts at bit a of word w (S[w] has it): the first end at or behind it
__device__ __forceinline__ int ds_run_end(const DsRow& r, int nwords, int w, int a) {
    const ds_u64 e = r.E[w] & (~0ull << a);
    if (e) return 64 * w + __builtin_ctzll(e);
    const int target = r.PE[w + 1];                                        // ends in words <= w all belong to earlier runs
    int lo = w + 1, hi = nwords - 1;                                       // smallest w' with PE[w' + 1] > target
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r.PE[mid + 1] > target) hi = mid; else lo = mid + 1;
    }
    lo = min(lo, nwords - 1);
    const ds_u64 e2 = r.E[lo];
    return e2 ? 64 * lo + __builtin_ctzll(e2) : 64 * w + a;                // (every start has an end; never taken)
}

// M[0 .. nwords) is in LDS (all threads have passed a barrier behind its last write).  Fills S (run starts after gap closing), E (run ends),
// PE (exclusive scan of popc(E)), K (starts of runs with >= min_len frames); returns this thread's count of kept starts (its words are
// [w_lo, w_hi)).  All threads of the workgroup call it.
__device__ __forceinline__ int ds_plan(const DsRow& r, int nwords, int max_gap, int min_len, int* s_wave, int w_lo, int w_hi) {
    int n_end = 0;
    for (int w = w_lo; w < w_hi; ++w) {
        const ds_u64 m = r.M[w];
        ds_u64 s = 0, e = 0;
        if (m) {
            const ds_u64 left = w > 0 ? r.M[w - 1] >> 63 : 0ull, right = w + 1 < nwords ? r.M[w + 1] << 63 : 0ull;
            ds_u64 rs = m & ~((m << 1) | left);                            // first frames of the raw runs of this word
            ds_u64 re = m & ~((m >> 1) | right);                           // last frames
            if (max_gap == 0) {
                s = rs; e = re;
            } else {
                while (rs) {
                    const int a = __builtin_ctzll(rs);
                    rs &= rs - 1;
                    const ds_u64 below = m & ((1ull << a) - 1);
                    long prev = -(1L << 40);                               // the active frame before a, in row frames
                    if (below) prev = 64 * w + 63 - __builtin_clzll(below);
                    else
                        for (int v = w - 1; v >= 0 && 64 * (w - v - 1) + a <= max_gap; --v) {      // (frames between word v's last and a)
                            const ds_u64 mv = r.M[v];
                            if (mv) { prev = 64 * v + 63 - __builtin_clzll(mv); break; }
                        }
                    if (64L * w + a - prev - 1 > max_gap) s |= 1ull << a;
                }
                while (re) {
                    const int a = __builtin_ctzll(re);
                    re &= re - 1;
                    const ds_u64 above = a < 63 ? m & (~0ull << (a + 1)) : 0ull;
                    long next = 1L << 40;
                    if (above) next = 64 * w + __builtin_ctzll(above);
                    else
                        for (int v = w + 1; v < nwords && 64 * (v - w - 1) + (63 - a) <= max_gap; ++v) {
                            const ds_u64 mv = r.M[v];
                            if (mv) { next = 64 * v + __builtin_ctzll(mv); break; }
                        }
                    if (next - (64L * w + a) - 1 > max_gap) e |= 1ull << a;
                }
            }
        }
        r.S[w] = s; r.E[w] = e;
        n_end += __builtin_popcountll(e);
    }
    int total;
    int run = seg_block_scan(n_end, s_wave, total);
    if (threadIdx.x == 0) r.PE[0] = 0;
    for (int w = w_lo; w < w_hi; ++w) {
        run += __builtin_popcountll(r.E[w]);
        r.PE[w + 1] = run;
    }
    __syncthreads();
    int n_keep = 0;
    for (int w = w_lo; w < w_hi; ++w) {
        ds_u64 s = r.S[w], k = 0;
        if (min_len <= 1) k = s;
        else
            while (s) {
                const int a = __builtin_ctzll(s);
                s &= s - 1;
                if (ds_run_end(r, nwords, w, a) - (64 * w + a) + 1 >= min_len) k |= 1ull << a;
            }
        r.K[w] = k;
        n_keep += __builtin_popcountll(k);
    }
    return n_keep;
}

template <bool VEC>
__global__ __launch_bounds__(DS_THREADS) void det_count_kernel(const float* __restrict__ probs, const int* __restrict__ valid_t,
                                                               const float* __restrict__ thr, ds_u64* __restrict__ masks, int* __restrict__ counts,
                                                               int C, int K, int TL, int nwords, int max_gap, int min_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ds_smem[];
    __shared__ int s_wave[DS_THREADS / 64];
    const DsRow r = ds_carve(ds_smem, nwords);
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6);
    const long row = blockIdx.x;                                           // (b * C + c) * K + k
    const long srow = row / K;                                             // b * C + c: the row of probs
    const int b = (int)(srow / C);
    const int vlen = min(max(valid_t[b], 0), TL);
    const float th = thr[row - (long)b * C * K];                           // thr (C, K): c * K + k
    const float* src = probs + srow * TL;
    ds_u64* mrow = masks + row * nwords;
    bool any = false;
    for (int f0 = wave * 256; f0 < TL; f0 += DS_PASS) {                    // (wave uniform: every lane reaches the ballots)
        ds_u64 bal[4];
        if (VEC) {
            const int t = f0 + 4 * lane;
            ds_f4 v = {0.f, 0.f, 0.f, 0.f};
            if (t < TL) v = *reinterpret_cast<const ds_f4*>(src + t);      // (TL % 4 == 0: all four inside)
            bal[0] = __ballot(t + 0 < vlen && v.x > th);
            bal[1] = __ballot(t + 1 < vlen && v.y > th);
            bal[2] = __ballot(t + 2 < vlen && v.z > th);
            bal[3] = __ballot(t + 3 < vlen && v.w > th);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = f0 + 64 * j + lane;
                float v = 0.f;
                if (t < TL) v = src[t];
                bal[j] = __ballot(t < vlen && v > th);
            }
        }
        any = any || (bal[0] | bal[1] | bal[2] | bal[3]) != 0;
        const int w = (f0 >> 6) + lane;                                    // lanes 0..3 assemble the wave's four words
        if (lane < 4 && w < nwords) {
            ds_u64 word;
            if (VEC) {
                const int sh = 16 * lane;
                word = ds_spread16(bal[0] >> sh) | ds_spread16(bal[1] >> sh) << 1 | ds_spread16(bal[2] >> sh) << 2 | ds_spread16(bal[3] >> sh) << 3;
            } else {
                word = lane == 0 ? bal[0] : lane == 1 ? bal[1] : lane == 2 ? bal[2] : bal[3];
            }
            r.M[w] = word;
            mrow[w] = word;
        }
    }
    if (!__syncthreads_or(any)) {                                          // no active frame: most rows
        if (tid == 0) counts[row] = 0;
        return;
    }
    const int wpt = (nwords + DS_THREADS - 1) / DS_THREADS;
    const int w_lo = min(tid * wpt, nwords), w_hi = min(w_lo + wpt, nwords);
    const int n_keep = ds_plan(r, nwords, max_gap, min_len, s_wave, w_lo, w_hi);
    int total;
    seg_block_scan(n_keep, s_wave, total);
    if (tid == 0) counts[row] = total;
}

// seg_launch_scan of seg_common.h: counts[0 .. n), clamped to [0, count_max], -> exclusive sums in place, counts[n] = total;
// offsets[b] = the sum of the rows of samples < b; one workgroup
__global__ __launch_bounds__(1024) void seg_scan_kernel(int* __restrict__ counts, int* __restrict__ offsets, int* __restrict__ total_out, long n, int B,
                                                        int C, long count_max) {
    __shared__ int s_wave[16];
    const int tid = threadIdx.x;
    int carry = 0;
    for (long i0 = 0; i0 < n; i0 += 1024) {
        const long i = i0 + tid;
        const int v = i < n ? (int)seg_clampl(counts[i], 0, count_max) : 0;
        int total;
        const int ex = carry + seg_block_scan(v, s_wave, total);
        if (i < n) {
            counts[i] = ex;
            if (i % C == 0) offsets[i / C] = ex;
        }
        carry += total;
    }
    if (tid == 0) {
        counts[n] = carry;
        offsets[B] = carry;
        total_out[0] = carry;
    }
}

void seg_launch_scan(int* counts, int* offsets, int* total, long n, int B, int C, long count_max, hipStream_t st) {
    hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, st, counts, offsets, total, n, B, C, count_max);
}

__global__ __launch_bounds__(DS_THREADS) void det_write_kernel(const float* __restrict__ probs, const double* __restrict__ fps, const int* __restrict__ start,
                                                               const ds_u64* __restrict__ masks, const int* __restrict__ bases, double* __restrict__ seg,
                                                               int* __restrict__ frames, float* __restrict__ score, unsigned char* __restrict__ level,
                                                               int C, int K, int TL, int nwords, int max_gap, int min_len, long cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ds_smem[];
    __shared__ int s_wave[DS_THREADS / 64];
    const long row = blockIdx.x;
    const long base = bases[row];
    if (bases[row + 1] - base <= 0 || base >= cap) return;                 // (workgroup uniform) nothing kept, or all of it behind cap
    const DsRow r = ds_carve(ds_smem, nwords);
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6);
    const long srow = row / K;
    const int b = (int)(srow / C), c = (int)(srow - (long)b * C), lev = (int)(row - srow * K);
    const ds_u64* mrow = masks + row * nwords;
    for (int w = tid; w < nwords; w += DS_THREADS) r.M[w] = mrow[w];
    __syncthreads();
    const int wpt = (nwords + DS_THREADS - 1) / DS_THREADS;
    const int w_lo = min(tid * wpt, nwords), w_hi = min(w_lo + wpt, nwords);
    const int n_keep = ds_plan(r, nwords, max_gap, min_len, s_wave, w_lo, w_hi);
    int total;
    int run = seg_block_scan(n_keep, s_wave, total);
    for (int w = w_lo; w < w_hi; ++w) {
        r.PK[w] = run;
        run += __builtin_popcountll(r.K[w]);
    }
    __syncthreads();
    const float* src = probs + srow * TL;
    const double f = fps[b];
    const long first = start[b];
    for (int w = wave; w < nwords; w += DS_THREADS / 64) {                 // (wave uniform from here on)
        const ds_u64 kw = ds_uni(r.K[w]);
        ds_u64 k = kw;
        const int pk = cfn_uni(r.PK[w]);
        while (k) {
            const int a = __builtin_ctzll(k);
            k &= k - 1;
            const long idx = base + pk + __builtin_popcountll(kw & ((1ull << a) - 1));
            if (idx >= cap) break;                                         // ranks only grow
            const int t0 = 64 * w + a;
            const int t1 = min(cfn_uni(ds_run_end(r, nwords, w, a)), TL - 1);
            float mx = -INFINITY;
            double sum = 0.0;
            int n = 0;
            for (int f0 = t0 & ~63; f0 <= t1; f0 += 64) {
                const int t = f0 + lane;
                const bool act = t >= t0 && t <= t1 && ((r.M[f0 >> 6] >> lane) & 1ull);
                if (act) {
                    const float v = src[t];
                    mx = fmaxf(mx, v);
                    sum += (double)v;
                }
                n += __builtin_popcountll(__ballot(act));
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {                            // a butterfly: every lane adds the same pairs, a fixed order
                mx = fmaxf(mx, __shfl_xor(mx, d, 64));
                sum += __shfl_xor(sum, d, 64);
            }
            if (lane == 0) {
                seg[3 * idx + 0] = (double)c;
                seg[3 * idx + 1] = ((double)(first + t0) - 0.5) / f;
                seg[3 * idx + 2] = ((double)(first + t1) + 0.5) / f;
                frames[3 * idx + 0] = t0; frames[3 * idx + 1] = t1; frames[3 * idx + 2] = n;
                score[2 * idx + 0] = mx;
                score[2 * idx + 1] = (float)(sum / (double)n);
                if (level) level[idx] = (unsigned char)lev;
            }
        }
    }
}

static inline long ds_mask_words(long B, long C, long TL) { return B * C * ((TL + 63) / 64); }

#define DS_MAX_LEVELS 16

static inline bool ds_shape_ok(int B, int C, int K, int TL) {
    return B >= 1 && C >= 1 && TL >= 1 && B <= 65535 && C < (1 << 19) && TL <= DS_MAX_TL && K >= 1 && K <= DS_MAX_LEVELS && (long)B * C * K * TL < (1L << 31);
}

// workspace: the rows' 64-bit mask words, then B * C * K + 1 int32 (counts, then bases)
static inline long ds_workspace_bytes(int B, int C, int K, int TL) { return ds_mask_words(B, (long)C * K, TL) * 8 + ((long)B * C * K + 1) * 4; }

extern "C" long cfn_decode_segments_workspace_bytes(int B, int C, int TL) { return ds_shape_ok(B, C, 1, TL) ? ds_workspace_bytes(B, C, 1, TL) : -1; }

extern "C" long cfn_decode_segments_levels_workspace_bytes(int B, int C, int K, int TL) {
    return ds_shape_ok(B, C, K, TL) ? ds_workspace_bytes(B, C, K, TL) : -1;
}

// rows are (b, c, k); thr (C, K); level may be null (K = 1: cfn_decode_segments)
static int ds_decode(const char* what, const float* probs, const int* valid_t, const double* fps, const int* start, const float* thr, double* seg,
                     int* frames, float* score, unsigned char* level, int* offsets, int* total, void* workspace, int B, int C, int K, int TL,
                     int max_gap, int min_len, long cap, void* stream) {
    CFN_REQUIRE(probs && valid_t && fps && start && thr && seg && frames && score && offsets && total && workspace, "%s: null tensor", what);
    CFN_REQUIRE(B >= 1 && C >= 1 && TL >= 1, "%s: bad shape (B %d, C %d, TL %d)", what, B, C, TL);
    CFN_REQUIRE(K >= 1 && K <= DS_MAX_LEVELS, "%s: levels: K in [1, %d] expected, got %d", what, DS_MAX_LEVELS, K);
    CFN_REQUIRE(ds_shape_ok(B, C, K, TL), "%s: too large (B %d, C %d, K %d, TL %d; B * C * K * TL < 2^31)", what, B, C, K, TL);
    CFN_REQUIRE(max_gap >= 0, "%s: max_gap >= 0 expected, got %d", what, max_gap);
    CFN_REQUIRE(min_len >= 1, "%s: min_len >= 1 expected, got %d", what, min_len);
    CFN_REQUIRE(cap >= 1 && cap < (1L << 31), "%s: cap in [1, 2^31) expected, got %ld", what, cap);
    CFN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace on an 8-byte boundary expected", what);
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * C * K;
    const int nwords = (TL + 63) / 64;
    ds_u64* masks = (ds_u64*)workspace;
    int* counts = (int*)(masks + ds_mask_words(B, (long)C * K, TL));
    const size_t lds = ds_lds_bytes(nwords);
    const bool vec = TL % 4 == 0 && ((uintptr_t)probs & 15) == 0;
    if (max_gap > DS_MAX_TL) max_gap = DS_MAX_TL;                                   // (a gap is shorter than the row: the same result, no overflow)
    CfnProfScope prof(CFN_K_ELEMWISE, st, (double)rows * TL * 4.0);
    if (vec) hipLaunchKernelGGL(det_count_kernel<true>, dim3((unsigned)rows), dim3(DS_THREADS), lds, st, probs, valid_t, thr, masks, counts, C, K, TL, nwords, max_gap, min_len);
    else hipLaunchKernelGGL(det_count_kernel<false>, dim3((unsigned)rows), dim3(DS_THREADS), lds, st, probs, valid_t, thr, masks, counts, C, K, TL, nwords, max_gap, min_len);
    seg_launch_scan(counts, offsets, total, rows, B, C * K, 0x7fffffffL, st);                    // (det_count_kernel's counts are in [0, 32768] already)
    hipLaunchKernelGGL(det_write_kernel, dim3((unsigned)rows), dim3(DS_THREADS), lds, st, probs, fps, start, (const ds_u64*)masks, (const int*)counts, seg, frames, score, level,
                       C, K, TL, nwords, max_gap, min_len, cap);
    return cfn_check_launch(what);
}

extern "C" int cfn_decode_segments(const float* probs, const int* valid_t, const double* fps, const int* start, const float* thr, double* seg,
                                   int* frames, float* score, int* offsets, int* total, void* workspace, int B, int C, int TL, int max_gap,
                                   int min_len, long cap, void* stream) {
    return ds_decode("cfn_decode_segments", probs, valid_t, fps, start, thr, seg, frames, score, nullptr, offsets, total, workspace, B, C, 1, TL, max_gap,
                     min_len, cap, stream);
}

extern "C" int cfn_decode_segments_levels(const float* probs, const int* valid_t, const double* fps, const int* start, const float* levels, double* seg,
                                          int* frames, float* score, unsigned char* level, int* offsets, int* total, void* workspace, int B, int C, int K,
                                          int TL, int max_gap, int min_len, long cap, void* stream) {
    const char* what = "cfn_decode_segments_levels";
    CFN_REQUIRE(level, "%s: null tensor", what);
    return ds_decode(what, probs, valid_t, fps, start, levels, seg, frames, score, level, offsets, total, workspace, B, C, K, TL, max_gap, min_len, cap,
                     stream);
}
