// Per-class average precision on the GPU: the device-resident form of apmeter.APMeter (reference apmeter.py:22-136; the definition is
// apmeter.py:39-58 of this tree: per class a STABLE descending sort of the scores, AP = mean over the positive ranks r of tp_r / r).
//
// Storage is class major: scores (K, cap) fp32 and targets (K, cap) uint8, row i of class k at k * cap + i (64-bit offsets); the number of
// rows held lives on the device (`count`, one int) next to a flag word (bit 0: a label that is neither 0 nor 1, bit 1: a batch that did
// not fit).  Nothing below takes a row count from the host: no grid size and no host branch depends on it.
//
//   cfn_ap_append   probs / labels (B, K, TL) -> rows count .. count + sum_b v_b - 1 of every class, v_b = clamp(valid[b], 0, TL), videos in
//                   batch order and frames ascending (train_fine._ap_rows + concatenate).  Two launches on the stream: the copy kernel, whose
//                   workgroups all READ count, then a one-thread kernel that advances it -- no workgroup can see the advanced value.
//   cfn_ap_sort     LSD radix sort, 8-bit digits, 4 passes, on an order-preserving key of the bit pattern (descending score = ascending key;
//                   -0.0 is +0.0, every NaN is the last key, denormals are what they are: integer arithmetic only).  ONE persistent workgroup
//                   per class walks the class's tiles in order, so the running per-digit offsets live in its LDS and no workgroup waits for
//                   another.  Inside a tile a wave ranks its lanes by a match on the digit (8 ballots; rank = popcount of the peers below the
//                   lane) on top of the wave's own digit counts, and the waves' counts are scanned in wave order: equal digits leave a tile in
//                   the order they came in, which is what makes every pass stable.  All counters are 32 bits wide.
//   cfn_ap_reduce   the same walk over the sorted target bytes: running positive count across tiles, tp / rank in fp64 at each positive,
//                   summed per thread in row order, then one fixed-shape block reduction; AP as fp32.  No floating-point atomics anywhere:
//                   results are bit-identical from run to run and independent of cfn_deterministic.
#include "cfn_common.h"

#define AP_FLAG_NONBINARY 1
#define AP_FLAG_OVERFLOW 2

#define AP_THREADS 1024
#define AP_WAVES (AP_THREADS / 64)
#define AP_IPT 8                                  // rows per thread and tile of the sort
#define AP_TILE (AP_THREADS * AP_IPT)
#define AP_RPT 16                                 // rows per thread and tile of the reduction
#define AP_RTILE (AP_THREADS * AP_RPT)

typedef unsigned __attribute__((ext_vector_type(4))) apu4;

// -----------------------------------------------------------------------------------------------------------------------------------------
// append
// -----------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ap_valid(const int* valid, int b, int TL) { return valid ? min(max(valid[b], 0), TL) : TL; }

// grid (cdiv(TL, 256), K, B).  Every workgroup derives the batch's total and its video's offset from valid[] itself (B is a batch size).
__global__ __launch_bounds__(256) void ap_append_kernel(const float* __restrict__ probs, const float* __restrict__ labels, const int* __restrict__ valid,
                                                        float* __restrict__ scores, unsigned char* __restrict__ targets, const int* __restrict__ count,
                                                        int* __restrict__ flags, int B, int K, int TL, long cap) {
    const int b = blockIdx.z, k = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    long before = 0, total = 0;
    for (int i = 0; i < B; ++i) {
        const int v = ap_valid(valid, i, TL);
        if (i < b) before += v;
        total += v;
    }
    const long n0 = min(max((long)*count, 0L), cap);
    if (n0 + total > cap) return;                                         // the batch does not fit: nothing is written (ap_advance_kernel flags it)
    if (t >= ap_valid(valid, b, TL)) return;
    const long src = ((long)b * K + k) * TL + t, dst = (long)k * cap + n0 + before + t;
    const float lab = labels[src];
    scores[dst] = probs[src];
    targets[dst] = lab != 0.0f ? 1 : 0;
    if (lab != 0.0f && lab != 1.0f) atomicOr(flags, AP_FLAG_NONBINARY);    // (a NaN label too, as target * target == target on the host)
}

__global__ void ap_advance_kernel(const int* __restrict__ valid, int* __restrict__ count, int* __restrict__ flags, int B, int TL, long cap) {
    long total = 0;
    for (int i = 0; i < B; ++i) total += ap_valid(valid, i, TL);
    const long n0 = min(max((long)*count, 0L), cap);
    if (n0 + total > cap) atomicOr(flags, AP_FLAG_OVERFLOW);
    else *count = (int)(n0 + total);
}

extern "C" int cfn_ap_append(const float* probs, const float* labels, const int* valid, float* scores, unsigned char* targets, int* count,
                             int* flags, int B, int K, int TL, long cap, void* stream) {
    CFN_REQUIRE(probs && labels && scores && targets && count && flags, "cfn_ap_append: null tensor");
    CFN_REQUIRE(B > 0 && K > 0 && TL > 0 && cap > 0, "cfn_ap_append: bad shape");
    CFN_REQUIRE(cap <= 0x7fffffffL && K <= 65535 && B <= 65535, "cfn_ap_append: bad shape (cap < 2^31, K and B <= 65535)");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, (double)B * K * TL * 13.0);
    hipLaunchKernelGGL(ap_append_kernel, dim3((unsigned)cfn_cdiv(TL, 256), (unsigned)K, (unsigned)B), dim3(256), 0, st, probs, labels, valid, scores,
                       targets, (const int*)count, flags, B, K, TL, cap);
    hipLaunchKernelGGL(ap_advance_kernel, dim3(1), dim3(1), 0, st, valid, count, flags, B, TL, cap);
    return cfn_launch_ok("ap_append");
}

// -----------------------------------------------------------------------------------------------------------------------------------------
// sort
// -----------------------------------------------------------------------------------------------------------------------------------------
// ascending key <=> descending score, ties = equal keys
__device__ __forceinline__ unsigned ap_key(unsigned u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;              // every NaN: behind -inf
    if (u == 0x80000000u) u = 0u;                                         // -0.0 ties with +0.0
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}
__device__ __forceinline__ unsigned ap_unkey(unsigned key) {             // (the NaN key decodes to the all-ones NaN)
    const unsigned asc = ~key;
    return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}

// lanes of the wave that are `live` and hold the same 8-bit digit
__device__ __forceinline__ unsigned long long ap_match(unsigned d, unsigned long long live) {
    unsigned long long peers = live;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// one pass: src keys (or, FIRST, the raw scores) + target bytes -> dst, stable on digit `shift / 8`; LAST writes the scores back as floats.
// off[256]: the class's running per-digit offsets (exclusive scan of the digit histogram on entry); wh[AP_WAVES][256]: per-wave counts.
template <bool FIRST, bool LAST>
__device__ __forceinline__ void ap_sort_pass(const unsigned* src, const unsigned char* tsrc, unsigned* dst, unsigned char* tdst, int n, int shift,
                                             unsigned* off, unsigned* wh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned* mine = wh + wave * 256;
    for (int base = 0; base < n; base += AP_TILE) {                       // (n <= cap < 2^31 - AP_TILE is required by the entry point)
#pragma unroll
        for (int j = 0; j < 4; ++j) mine[lane + 64 * j] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        unsigned key[AP_IPT], loc[AP_IPT];
        unsigned char tg[AP_IPT];
#pragma unroll
        for (int i = 0; i < AP_IPT; ++i) {                                 // the wave's rows: AP_IPT runs of 64 consecutive rows, in order
            const int e = base + wave * (64 * AP_IPT) + i * 64 + lane;
            const bool live = e < n;
            key[i] = 0u; tg[i] = 0;
            if (live) {
                key[i] = FIRST ? ap_key(src[e]) : src[e];
                tg[i] = tsrc[e];
            }
        }
#pragma unroll
        for (int i = 0; i < AP_IPT; ++i) {
            const int e = base + wave * (64 * AP_IPT) + i * 64 + lane;
            const bool live = e < n;
            const unsigned d = (key[i] >> shift) & 255u;
            const unsigned long long peers = ap_match(d, __ballot(live));
            const unsigned rank = (unsigned)__popcll(peers & below);
            loc[i] = mine[d] + rank;                                       // rows of this digit earlier in the wave's part of the tile
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");         // every peer has read the count before its first lane advances it
            __builtin_amdgcn_wave_barrier();
            if (live && rank == 0u) mine[d] += (unsigned)__popcll(peers);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        if (tid < 256) {                                                   // digit tid: the waves' counts -> their start offsets in dst, in wave order
            unsigned c[AP_WAVES];
#pragma unroll
            for (int w = 0; w < AP_WAVES; ++w) c[w] = wh[w * 256 + tid];
            unsigned run = off[tid];
#pragma unroll
            for (int w = 0; w < AP_WAVES; ++w) { wh[w * 256 + tid] = run; run += c[w]; }
            off[tid] = run;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < AP_IPT; ++i) {
            const int e = base + wave * (64 * AP_IPT) + i * 64 + lane;
            if (e < n) {
                const unsigned p = mine[(key[i] >> shift) & 255u] + loc[i];
                if (p < (unsigned)n) {                                     // (always: the offsets are a permutation of 0 .. n - 1)
                    dst[p] = LAST ? ap_unkey(key[i]) : key[i];
                    tdst[p] = tg[i];
                }
            }
        }
        __syncthreads();                                                   // wh is zeroed again at the top
    }
}

// between two passes: the rows this workgroup scattered are read back by its other waves (release, barrier, then acquire: the buffer a
// pass writes was read two passes earlier and may still sit in the CU's vector cache)
__device__ __forceinline__ void ap_pass_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// grid (K): workgroup k sorts rows 0 .. n - 1 of class k, n = count[k * count_stride].  The two buffers alternate: scores -> tmp -> out -> tmp -> out.
__global__ __launch_bounds__(AP_THREADS) void ap_sort_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ targets,
                                                             const int* __restrict__ count, float* __restrict__ out_scores,
                                                             unsigned char* __restrict__ out_targets, int* __restrict__ tmp_keys,
                                                             unsigned char* __restrict__ tmp_targets, long cap, int count_stride) {
    __shared__ unsigned hist[4 * 256];
    __shared__ unsigned wh[AP_WAVES * 256];
    const int tid = threadIdx.x, lane = tid & 63;
    const long cls = (long)blockIdx.x * cap;
    const int n = (int)min(max((long)count[(long)blockIdx.x * count_stride], 0L), cap);      // (stride 0: one count for every class)
    const unsigned* s0 = reinterpret_cast<const unsigned*>(scores) + cls;
    const unsigned char* t0 = targets + cls;
    unsigned* ka = reinterpret_cast<unsigned*>(tmp_keys) + cls;
    unsigned char* ta = tmp_targets + cls;
    unsigned* kb = reinterpret_cast<unsigned*>(out_scores) + cls;
    unsigned char* tb = out_targets + cls;

    // the four digit histograms of the class in one read (the passes permute the same keys).  Lanes with the same digit are counted by a
    // match and added once: scores of one sign and magnitude share their top byte, and 64 LDS atomics on one address would serialise.
    hist[tid] = 0u;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < n; base += AP_THREADS) {
        const int e = base + tid;
        const bool live = e < n;
        const unsigned key = live ? ap_key(s0[e]) : 0u;
        const unsigned long long lv = __ballot(live);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned d = (key >> (8 * p)) & 255u;
            const unsigned long long peers = ap_match(d, lv);
            if (live && (peers & below) == 0ull) atomicAdd(&hist[p * 256 + d], (unsigned)__popcll(peers));
        }
    }
    __syncthreads();
    if (tid < 4) {                                                         // exclusive scan, one thread per pass (4 x 256 LDS words, once per class)
        unsigned run = 0u;
        for (int d = 0; d < 256; ++d) { const unsigned c = hist[tid * 256 + d]; hist[tid * 256 + d] = run; run += c; }
    }
    __syncthreads();
    ap_sort_pass<true, false>(s0, t0, ka, ta, n, 0, hist, wh);
    ap_pass_sync();
    ap_sort_pass<false, false>(ka, ta, kb, tb, n, 8, hist + 256, wh);
    ap_pass_sync();
    ap_sort_pass<false, false>(kb, tb, ka, ta, n, 16, hist + 512, wh);
    ap_pass_sync();
    ap_sort_pass<false, true>(ka, ta, kb, tb, n, 24, hist + 768, wh);
}

extern "C" int cfn_ap_sort(const float* scores, const unsigned char* targets, const int* count, float* sorted_scores,
                           unsigned char* sorted_targets, int* tmp_keys, unsigned char* tmp_targets, int K, long cap, void* stream) {
    CFN_REQUIRE(scores && targets && count && sorted_scores && sorted_targets && tmp_keys && tmp_targets, "cfn_ap_sort: null tensor");
    CFN_REQUIRE(K > 0 && cap > 0, "cfn_ap_sort: bad shape");
    CFN_REQUIRE(cap <= 0x7fffffffL - AP_TILE, "cfn_ap_sort: bad shape (cap < 2^31 - tile)");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);                            // (the row count is on the device: tools/ap_meter_bench.py states the bytes)
    hipLaunchKernelGGL(ap_sort_kernel, dim3((unsigned)K), dim3(AP_THREADS), 0, st, scores, targets, count, sorted_scores, sorted_targets, tmp_keys,
                       tmp_targets, cap, 0);
    return cfn_launch_ok("ap_sort");
}

// cfn_ap_sort with one count per class: counts (K) int32 (the stores of cfn_segap_append)
extern "C" int cfn_ap_sort_counts(const float* scores, const unsigned char* targets, const int* counts, float* sorted_scores,
                                  unsigned char* sorted_targets, int* tmp_keys, unsigned char* tmp_targets, int K, long cap, void* stream) {
    CFN_REQUIRE(scores && targets && counts && sorted_scores && sorted_targets && tmp_keys && tmp_targets, "cfn_ap_sort_counts: null tensor");
    CFN_REQUIRE(K > 0 && cap > 0, "cfn_ap_sort_counts: bad shape");
    CFN_REQUIRE(cap <= 0x7fffffffL - AP_TILE, "cfn_ap_sort_counts: bad shape (cap < 2^31 - tile)");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(ap_sort_kernel, dim3((unsigned)K), dim3(AP_THREADS), 0, st, scores, targets, counts, sorted_scores, sorted_targets, tmp_keys,
                       tmp_targets, cap, 1);
    return cfn_launch_ok("ap_sort_counts");
}

extern "C" int cfn_ap_sort_tile(void) { return AP_TILE; }

// -----------------------------------------------------------------------------------------------------------------------------------------
// reduce
// -----------------------------------------------------------------------------------------------------------------------------------------
// grid (K).  A thread owns AP_RPT consecutive rows of a tile; the positives in front of them: a scan of the threads' counts (wave shuffles,
// then the 16 wave totals through LDS) on top of the count the earlier tiles left.
__global__ __launch_bounds__(AP_THREADS) void ap_reduce_kernel(const unsigned char* __restrict__ sorted_targets, const int* __restrict__ count,
                                                               float* __restrict__ ap, long cap) {
    __shared__ unsigned wtot[AP_WAVES];
    __shared__ double wsum[AP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char* tg = sorted_targets + (long)blockIdx.x * cap;
    const int n = (int)min(max((long)*count, 0L), cap);
    const bool aligned = (((uintptr_t)tg) & 15) == 0;
    unsigned seen = 0u;                                                    // positives in the tiles behind us
    double acc = 0.0;
    for (long base = 0; base < n; base += AP_RTILE) {
        const long e0 = base + (long)tid * AP_RPT;
        unsigned bits = 0u;                                                // bit i: row e0 + i is a positive
        if (aligned && e0 + AP_RPT <= n) {
            const apu4 v = *reinterpret_cast<const apu4*>(tg + e0);
#pragma unroll
            for (int i = 0; i < AP_RPT; ++i) bits |= (((v[i >> 2] >> (8 * (i & 3))) & 255u) != 0u ? 1u : 0u) << i;
        } else {
#pragma unroll
            for (int i = 0; i < AP_RPT; ++i)
                if (e0 + i < n) bits |= (tg[e0 + i] != 0 ? 1u : 0u) << i;
        }
        const unsigned own = (unsigned)__popc(bits);
        unsigned incl = own;                                               // inclusive scan over the wave's lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned front = seen, all = 0u;
#pragma unroll
        for (int w = 0; w < AP_WAVES; ++w) {
            const unsigned c = wtot[w];
            if (w < wave) front += c;
            all += c;
        }
        unsigned tp = front + incl - own;
        for (int i = 0; i < AP_RPT; ++i) {                                 // row order
            if ((bits >> i) & 1u) {
                ++tp;
                acc += (double)tp / (double)(e0 + i + 1);
            }
        }
        seen += all;
        __syncthreads();                                                   // wtot is rewritten by the next tile
    }
    acc = cfn_wave_sum_d(acc);                                             // a fixed butterfly, then the 16 wave sums in wave order
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < AP_WAVES; ++w) s += wsum[w];
        ap[blockIdx.x] = (float)(s / (double)(seen > 0u ? seen : 1u));
    }
}

extern "C" int cfn_ap_reduce(const unsigned char* sorted_targets, const int* count, float* ap, int K, long cap, void* stream) {
    CFN_REQUIRE(sorted_targets && count && ap, "cfn_ap_reduce: null tensor");
    CFN_REQUIRE(K > 0 && cap > 0, "cfn_ap_reduce: bad shape");
    CFN_REQUIRE(cap <= 0x7fffffffL, "cfn_ap_reduce: bad shape (cap < 2^31)");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);
    hipLaunchKernelGGL(ap_reduce_kernel, dim3((unsigned)K), dim3(AP_THREADS), 0, st, sorted_targets, count, ap, cap);
    return cfn_launch_ok("ap_reduce");
}
