// Per-class decode thresholds from the sorted AP rows (the rule: cfn_hip/calibrate.py and include/cfn_hip.h; the numpy statement:
// cfn_hip.calibrate.thresholds_reference).  The rows are what cfn_ap_sort (csrc/apmeter.hip) leaves: per class the scores descending and
// canonical (NaN last, -inf just in front), the target byte beside each; an operating point per criterion is one more walk over them.
//
//   cfn_ap_calibrate   ONE launch, one workgroup per class, as cfn_ap_reduce: the row count is read on the device only.
//     walk 1  every row of the class: P = positives (target bytes), m = rows with score > -inf (a prefix of the sorted row)
//     walk 2  rows 0 .. m - 1 in tiles of AP_CTILE: a thread owns AP_CPT consecutive rows; the running tp in front of them is the scan of
//             cfn_ap_reduce (thread counts, wave scan by shuffles, the 16 wave totals through LDS, the count of the tiles behind).  A cut
//             behind row e is ADMISSIBLE iff e + 1 == m or score[e] > score[e + 1]: the right neighbour of a thread's last row is read from
//             memory (one more load per thread), so no edge of a thread, a wave or a tile is special; the edge at m is the first clause.
//             The admissible cuts of the tile are a bit mask; the criteria then run over it one after the other (a loop, not unrolled: the
//             body exists once).  A thread's best candidate (r, tp) of the tile goes through a fixed wave butterfly at once, and lane k of
//             the wave keeps the wave's best of criterion k so far: two registers, no array that a run-time k would index.
//     reduce  per criterion the 16 wave results through LDS, merged in wave order.  Every merge is an argmax under the exact 64-bit integer
//             comparison with ties to the smaller r (f1), a max of r (precision) or a min of r (recall): independent of the order.
// No atomics, no floating-point accumulation, no allocation, no synchronisation with the host.
#include "cfn_common.h"

#define AP_CTHREADS 1024
#define AP_CWAVES (AP_CTHREADS / 64)
#define AP_CPT 8                                  // rows per thread and tile (16 spill at 1024 threads)
#define AP_CTILE (AP_CTHREADS * AP_CPT)
#define AP_CMAXK 16
#define AP_CNONE 0xffffffffu                      // recall: no cut found yet (above every r)

#define AP_KIND_F1 0
#define AP_KIND_PRECISION 1
#define AP_KIND_RECALL 2

typedef float __attribute__((ext_vector_type(4))) apcf4;

// the rows of a thread in front of row n: scores (rows at or behind n read as -inf) and the positives' bit mask
template <int N>
__device__ __forceinline__ void apc_load(const float* sc, const unsigned char* tg, long e0, int n, bool sc16, bool tg8, float (&v)[N], unsigned& bits) {
    static_assert(N >= AP_CPT && AP_CPT == 8, "room for the thread's rows; the target bytes of a thread are one 8-byte load");
    bits = 0u;
    const bool full = e0 + AP_CPT <= n;
    if (full && sc16) {
#pragma unroll
        for (int j = 0; j < AP_CPT / 4; ++j) {
            const apcf4 q = *reinterpret_cast<const apcf4*>(sc + e0 + 4 * j);
            v[4 * j] = q[0]; v[4 * j + 1] = q[1]; v[4 * j + 2] = q[2]; v[4 * j + 3] = q[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < AP_CPT; ++i) v[i] = e0 + i < n ? sc[e0 + i] : -INFINITY;
    }
    if (full && tg8) {
        const unsigned long long b = *reinterpret_cast<const unsigned long long*>(tg + e0);      // the thread's AP_CPT = 8 target bytes
#pragma unroll
        for (int i = 0; i < AP_CPT; ++i) bits |= (((b >> (8 * i)) & 255ull) != 0ull ? 1u : 0u) << i;
    } else {
#pragma unroll
        for (int i = 0; i < AP_CPT; ++i)
            if (e0 + i < n) bits |= (tg[e0 + i] != 0 ? 1u : 0u) << i;
    }
}

// a beats b: 2 tp / (r + P) strictly larger, compared exactly (both factors are below 2^32); equal values: the smaller r
__device__ __forceinline__ bool apc_f1_better(unsigned ra, unsigned ta, unsigned rb, unsigned tb, unsigned P) {
    const unsigned long long x = (unsigned long long)ta * ((unsigned long long)rb + P), y = (unsigned long long)tb * ((unsigned long long)ra + P);
    return x > y || (x == y && ra < rb);
}

// the merge of two candidates of one criterion (order-independent: argmax with a total tie rule, max, min)
__device__ __forceinline__ void apc_merge(int kind, unsigned P, unsigned& r, unsigned& t, unsigned r2, unsigned t2) {
    bool take;
    if (kind == AP_KIND_F1) take = apc_f1_better(r2, t2, r, t, P);
    else if (kind == AP_KIND_PRECISION) take = r2 > r;
    else take = r2 < r;
    if (take) { r = r2; t = t2; }
}

// grid (C).  kinds (K) / values (K): the criteria, read on the device.
__global__ __launch_bounds__(AP_CTHREADS) void ap_calibrate_kernel(const float* __restrict__ sorted_scores, const unsigned char* __restrict__ sorted_targets,
                                                                   const int* __restrict__ count, const int* __restrict__ kinds,
                                                                   const double* __restrict__ values, float* __restrict__ thr, int* __restrict__ cut,
                                                                   int* __restrict__ tp_out, unsigned char* __restrict__ ok, int* __restrict__ stat,
                                                                   int K, long cap) {
    __shared__ unsigned wtot[AP_CWAVES], wtot2[AP_CWAVES];
    __shared__ unsigned red_r[AP_CMAXK][AP_CWAVES], red_t[AP_CMAXK][AP_CWAVES];
    __shared__ int s_kind[AP_CMAXK];
    __shared__ double s_val[AP_CMAXK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long cls = (long)blockIdx.x * cap;
    const float* sc = sorted_scores + cls;
    const unsigned char* tg = sorted_targets + cls;
    const int n = (int)min(max((long)*count, 0L), cap);
    const bool sc16 = (((uintptr_t)sc) & 15) == 0, tg8 = (((uintptr_t)tg) & 7) == 0;
    if (tid < AP_CMAXK) {                                                  // an unknown kind or a value outside (0, 1] (a NaN too): kind -1, never met
        int kd = -1;
        double vl = 0.0;
        if (tid < K) {
            kd = kinds[tid];
            vl = values[tid];
            if (kd == AP_KIND_F1) vl = 0.0;
            else if (!((kd == AP_KIND_PRECISION || kd == AP_KIND_RECALL) && vl > 0.0 && vl <= 1.0)) kd = -1;
        }
        s_kind[tid] = kd;
        s_val[tid] = vl;
    }

    // ---- walk 1: P and m --------------------------------------------------------------------------------------------------------------
    unsigned pos = 0u, fin = 0u;
    for (long base = 0; base < n; base += AP_CTILE) {
        const long e0 = base + (long)tid * AP_CPT;
        float v[AP_CPT];
        unsigned bits;
        apc_load(sc, tg, e0, n, sc16, tg8, v, bits);
        pos += (unsigned)__popc(bits);
#pragma unroll
        for (int i = 0; i < AP_CPT; ++i) fin += v[i] > -INFINITY ? 1u : 0u;       // (a NaN fails; rows at or behind n were read as -inf)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pos += __shfl_xor(pos, o, 64);
        fin += __shfl_xor(fin, o, 64);
    }
    if (lane == 0) { wtot[wave] = pos; wtot2[wave] = fin; }
    __syncthreads();
    unsigned P = 0u, mu = 0u;
#pragma unroll
    for (int w = 0; w < AP_CWAVES; ++w) { P += wtot[w]; mu += wtot2[w]; }
    const int m = (int)min(mu, (unsigned)n);                               // (always mu: at most n rows were counted)
    __syncthreads();                                                       // wtot is rewritten by the first tile

    // ---- walk 2: the admissible cuts of rows 0 .. m - 1 against every criterion ----------------------------------------------------------
    // the wave's best (r, tp) of criterion k so far lives in its lane k: no per-thread array, nothing indexed at run time
    unsigned run_r = lane < K && s_kind[lane & (AP_CMAXK - 1)] == AP_KIND_RECALL ? AP_CNONE : 0u, run_t = 0u;
    unsigned seen = 0u;                                                    // positives in the tiles behind us
    for (long base = 0; base < m; base += AP_CTILE) {
        const long e0 = base + (long)tid * AP_CPT;
        unsigned bits, adm = 0u;                                           // bit i: row e0 + i is a positive / the cut behind row e0 + i is admissible
        {
            float v[AP_CPT + 1];
            apc_load(sc, tg, e0, m, sc16, tg8, v, bits);                  // (rows at or behind m: -inf and no bit -- their positives count in P only)
            v[AP_CPT] = e0 + AP_CPT < m ? sc[e0 + AP_CPT] : -INFINITY;     // the right neighbour of the thread's last row
#pragma unroll
            for (int i = 0; i < AP_CPT; ++i) {
                const long e = e0 + i;
                if (e < m && (e + 1 == m || v[i] > v[i + 1])) adm |= 1u << i;
            }
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
        for (int w = 0; w < AP_CWAVES; ++w) {
            const unsigned c = wtot[w];
            if (w < wave) front += c;
            all += c;
        }
        const unsigned tp0 = front + incl - own;                           // tp(e0)
        if (__ballot(adm != 0u) != 0ull) {                                 // (a wave inside one long run of equal scores has no cut to offer)
            for (int k = 0; k < K; ++k) {                                  // (uniform; the body exists once)
                const int kind = s_kind[k];
                if (kind < 0) continue;
                const double val = s_val[k], need = val * (double)P;       // recall: q * P, one fp64 multiply
                unsigned br = kind == AP_KIND_RECALL ? AP_CNONE : 0u, bt = 0u, t = tp0;      // the thread's best of this tile
#pragma unroll
                for (int i = 0; i < AP_CPT; ++i) {                         // row order: r ascending
                    t += (bits >> i) & 1u;
                    if (!((adm >> i) & 1u)) continue;
                    const unsigned r = (unsigned)(e0 + i + 1);
                    if (kind == AP_KIND_F1) {
                        if ((unsigned long long)t * ((unsigned long long)br + P) > (unsigned long long)bt * ((unsigned long long)r + P)) { br = r; bt = t; }
                    } else if (kind == AP_KIND_PRECISION) {
                        if ((double)t >= val * (double)r) { br = r; bt = t; }      // the largest: the last one met
                    } else {
                        if (br == AP_CNONE && P > 0u && (double)t >= need) { br = r; bt = t; }      // the smallest: the first one met
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {                         // a fixed butterfly: every lane ends with the wave's best of this tile
                    const unsigned r2 = __shfl_xor(br, o, 64), t2 = __shfl_xor(bt, o, 64);
                    apc_merge(kind, P, br, bt, r2, t2);
                }
                if (lane == k) apc_merge(kind, P, run_r, run_t, br, bt);
            }
        }
        seen += all;
        __syncthreads();                                                   // wtot is rewritten by the next tile
    }

    // ---- one fixed-shape reduction per criterion ---------------------------------------------------------------------------------------------
    if (lane < K) { red_r[lane][wave] = run_r; red_t[lane][wave] = run_t; }
    __syncthreads();
    if (tid < K) {                                                         // thread k: criterion k of this class
        const int k = tid, kind = s_kind[k];
        unsigned r = red_r[k][0], t = red_t[k][0];
        for (int w = 1; w < AP_CWAVES; ++w) apc_merge(kind, P, r, t, red_r[k][w], red_t[k][w]);
        unsigned char met = 0;
        if (kind == AP_KIND_F1) met = t > 0u;
        else if (kind == AP_KIND_PRECISION) met = r > 0u;
        else if (kind == AP_KIND_RECALL) {
            if (P == 0u) { r = 0u; t = 0u; }
            else if (r == AP_CNONE) { r = (unsigned)m; t = seen; }         // positives behind m: every active row, still short of q
            else met = 1;
        } else { r = 0u; t = 0u; }
        r = min(r, (unsigned)m);                                           // (always r: a cut is a row count of 0 .. m)
        float th = INFINITY;                                               // r == 0: nothing is active
        if (r > 0u) th = r < (unsigned)m ? sc[r] : -INFINITY;              // the largest score NOT taken; r == m: everything a strict compare can take
        const long o = (long)blockIdx.x * K + k;
        thr[o] = th;
        cut[o] = (int)r;
        tp_out[o] = (int)t;
        ok[o] = met;
    }
    if (tid == 0) {
        stat[2 * (long)blockIdx.x] = (int)P;
        stat[2 * (long)blockIdx.x + 1] = m;
    }
}

extern "C" int cfn_ap_calibrate(const float* sorted_scores, const unsigned char* sorted_targets, const int* count, const int* kinds,
                                const double* values, float* thr, int* cut, int* tp, unsigned char* ok, int* stat, int C, int K, long cap,
                                void* stream) {
    CFN_REQUIRE(sorted_scores && sorted_targets && count && kinds && values && thr && cut && tp && ok && stat, "cfn_ap_calibrate: null tensor");
    CFN_REQUIRE(C >= 1 && C <= 65535, "cfn_ap_calibrate: bad shape (C in [1, 65535])");
    CFN_REQUIRE(K >= 1 && K <= AP_CMAXK, "cfn_ap_calibrate: bad criteria (K in [1, 16])");
    CFN_REQUIRE(cap >= 1 && cap <= 0x7fffffffL, "cfn_ap_calibrate: bad cap (in [1, 2^31))");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, 0.0);                            // (the row count is on the device: tools/calibrate_bench.py states the bytes)
    hipLaunchKernelGGL(ap_calibrate_kernel, dim3((unsigned)C), dim3(AP_CTHREADS), 0, st, sorted_scores, sorted_targets, count, kinds, values, thr, cut,
                       tp, ok, stat, K, cap);
    return cfn_launch_ok("ap_calibrate");
}

extern "C" int cfn_ap_calibrate_tile(void) { return AP_CTILE; }
