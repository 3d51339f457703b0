// The stem pair conv1_s (dense 1x3x3, stride 2, 3 -> 24) + conv1_t (depthwise 5x1x1) of x3d_fine.py:210-222 as ONE kernel each way, for a 224 x 224
// fp32 clip with fp32 activations.  conv1_s's output xs stays in HBM (the forward writes it once and does not read it back, the backward reads it
// once); its gradient gxs never exists as a tensor.  Backward first, forward below (stem_pair_fwd_kernel).  DESIGN.md 4.19 has the measurements.
//
// The reference puts nothing between the two convs, so the gradient gxs of conv1_s's output xs is written by conv1_t's backward
// (dwt5_bwd_flat_kernel) and read by exactly one kernel, conv1_s's weight gradient (stem_wgrad_kernel), whose only output is a 24 x 27 tile: the
// clip gets no gradient.  Here gxs never leaves the chip:
//   g'(t)   = gy(t) + gs + 2 gq y(t)                        (zero outside the clip)
//   gxs(t)  = sum_k g'(t - 2 + k) w_t[4 - k]                (dwt5_bwd_flat_kernel's expression, tap for tap)
//   gw_t[k] += sum xs(s) g'(s + 2 - k)                      (re-indexed by the frame of xs: xs needs no halo)
//   gw_s[co][(ci,kh,kw)] += sum gxs x im2col(x)             (stem_wgrad_kernel's 28-column MFMA tile)
// Structure: stem_wgrad_kernel's persistent 8-wave workgroup, with a band of TWO output rows: a thread then owns 3 float4 positions of the
// 24-channel band, and the 5-frame window of g' that the temporal conv needs is 60 registers (with 4-row bands it is 120, next to the loads in
// flight and the accumulators that does not fit).  A workgroup walks RUNS of consecutive frames of one (sample, band): every step loads gy / y of
// frame t + 2 and xs / the clip band of frame t, completes gxs(t) into the LDS image that the MFMAs read as their A operand (where
// stem_wgrad_kernel stages gy), and multiplies while the next step's loads are in flight.  A run starts with four load-only steps (frames
// ta - 2 .. ta + 1 of g'; the first two are the halo, re-read once per run), so the window restarts at every run and at every sample.
// Every global access is an unconditional buffer load; what must not be read gets an out-of-range offset and reads as zero (dwt5.hip).
#include "cfn_common.h"
#include <stdlib.h>

typedef float __attribute__((ext_vector_type(16))) sp16;
typedef float __attribute__((ext_vector_type(4))) sp4;
typedef float __attribute__((ext_vector_type(2))) sp2;

struct StemPairBwdArgs {
    const float* gy; const float* y; const double* gs; const double* gq; const float* wt; const float* xs; const float* x;
    double* gwt; double* gws;
    int N, T, R, nch, runs, per_block;
};

namespace {
constexpr int SP_WI = 224, SP_WO = 112, SP_RB = 2, SP_RIN = 2 * SP_RB + 1, SP_PITCH = 228;
constexpr int SP_CIS = SP_RIN * SP_PITCH + 24;      // 1164 = 12 mod 64: the 27 operand columns start in 27 different banks (stem.hip)
constexpr int SP_GP = 2 * SP_WO + 2;                // 226: the 24 operand rows start in 24 different even banks
constexpr int SP_P = SP_WI * SP_WI, SP_PO = SP_WO * SP_WO, SP_BANDS = SP_WO / SP_RB, SP_OOB = 0x7fff0000;
constexpr int SP_XU = 3 * SP_RIN * (SP_WI / 4), SP_NXU = (SP_XU + 511) / 512;       // float4 units of the clip band per step and thread
constexpr int SP_GU = 24 * SP_RB * (SP_WO / 4), SP_NGU = (SP_GU + 511) / 512;       // float4 units of a 24-channel band
constexpr int SP_UPC = SP_RB * (SP_WO / 4);                                         // units per channel (the band's rows are contiguous in memory)

// position of a workgroup's walk: run = ((n * nch + chunk) * BANDS + band), frames [ta, tb) of it, t from ta - 4 (four load-only steps)
struct SpCur {
    int run, n, band, ta, tb, t;
    __device__ __forceinline__ void start(int r, int R, int nch, int T) {
        run = r;
        band = r % SP_BANDS;
        const int q = r / SP_BANDS, chunk = q % nch;
        n = q / nch;
        ta = chunk * R;
        tb = min(ta + R, T);
        t = ta - 4;
    }
    __device__ __forceinline__ void next(int R, int nch, int T) {
        if (++t == tb) start(run + 1, R, nch, T);
    }
};
}  // namespace

// The 5-tap sum  a0 w0 + a1 w1 + a2 w2 + a3 w3 + a4 w4  with the roundings that the compiler's contraction gives dwt5.hip's flat kernels for that
// expression (the a1 w1 product rounded on its own, the other four taps fused multiply-adds in the order 0, 2, 3, 4), spelled out so that y and
// gxs here keep the bits of those kernels whatever the contraction does with the expression in this file.  Nothing in the source GUARANTEES the
// equality: dwt5.hip leaves the contraction to the compiler, and another compiler may choose another one there.  For y it is pinned by
// tests/test_hip_stem_pair.py::test_forward, which asserts bit-identity with dwt5_fwd_flat_kernel and fails if the two drift apart (then copy
// the new contraction here).  For gxs it cannot be asserted, there is no gxs tensor: it is held through the 1e-4 bound on gw_s only.
__device__ __forceinline__ float sp_taps(float a0, float a1, float a2, float a3, float a4, float w0, float w1, float w2, float w3, float w4) {
    return __builtin_fmaf(a4, w4, __builtin_fmaf(a3, w3, __builtin_fmaf(a2, w2, __builtin_fmaf(a0, w0, __fmul_rn(a1, w1)))));
}

template <bool HASY>
__global__ __launch_bounds__(512) void stem_pair_bwd_kernel(const StemPairBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[3 * SP_CIS + 24 * SP_GP];
    float* const img = lds;                                                  // clip band [3][RIN][PITCH] (+24), data at column 4, column 3 = halo
    float* const gbuf = lds + 3 * SP_CIS;                                    // gxs band [24][GP]
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6), h = lane >> 5, p = lane & 31;
    const int T = a.T, R = a.R, nch = a.nch;

    for (int i = tid; i < 3 * SP_CIS; i += 512) img[i] = 0.0f;               // the halo column stays zero for good

    // staging units of this thread (the same for every step; the step adds a frame / row offset)
    int xo[SP_NXU], xl[SP_NXU], xr[SP_NXU];
#pragma unroll
    for (int k = 0; k < SP_NXU; ++k) {
        const int e = k * 512 + tid;
        const int rowid = e / (SP_WI / 4), c4 = e - rowid * (SP_WI / 4), ci = rowid / SP_RIN, r = rowid - ci * SP_RIN;
        const bool in = e < SP_XU;
        xo[k] = in ? (int)(((long)ci * T * SP_P + (long)r * SP_WI + c4 * 4) * 4) : SP_OOB;
        xl[k] = in ? ci * SP_CIS + r * SP_PITCH + 4 + c4 * 4 : -1;
        xr[k] = r;
    }
    int go[SP_NGU], gl[SP_NGU], gc[SP_NGU];
    float wk[SP_NGU][5];
#pragma unroll
    for (int k = 0; k < SP_NGU; ++k) {
        const int e = k * 512 + tid;
        const int co = e / SP_UPC, rem = e - co * SP_UPC;
        const bool in = e < SP_GU;
        go[k] = in ? (int)(((long)co * T * SP_PO + rem * 4) * 4) : SP_OOB;
        gl[k] = in ? co * SP_GP + rem * 4 : -1;
        gc[k] = in ? co : 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) wk[k][j] = a.wt[gc[k] * 5 + 4 - j];      // flipped taps
    }
    // operands of this lane: A row co = p (rows 24-31 repeat row 23 and are dropped), B column (ci, kh, kw) = p (columns 27-31 repeat column 0)
    const int ohl = wave >> 2, ow0 = (wave & 3) * 28;
    const int colp = p < 27 ? p : 0;
    const int ci = colp / 9, kh = (colp - ci * 9) / 3, kw = colp - ci * 9 - kh * 3;
    const float* bp = img + ci * SP_CIS + (2 * ohl + kh) * SP_PITCH + 2 * ow0 + kw + 3 + 2 * h;
    const float* ap = gbuf + min(p, 23) * SP_GP + ohl * SP_WO + ow0 + h;

    sp16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
    float acct[SP_NGU][5];
#pragma unroll
    for (int k = 0; k < SP_NGU; ++k)
#pragma unroll
        for (int j = 0; j < 5; ++j) acct[k][j] = 0.0f;

    // (each XCD walks one contiguous eighth of the runs: the halo frames and clip rows that neighbouring runs share hit ITS L2)
    const int first = (int)cfn_xcd_remap(blockIdx.x, gridDim.x) * a.per_block, last = min(first + a.per_block, a.runs);
    const unsigned gbytes = (unsigned)((long)24 * T * SP_PO * 4), xbytes = (unsigned)((long)3 * T * SP_P * 4);
    sp4 fg[SP_NGU], fy[SP_NGU], fs[SP_NGU], fx[SP_NXU];
    auto fetch = [&](const SpCur& c) {
        const bool on = c.run < last;
        const int n = on ? c.n : 0, f = c.t + 2;
        const bool fv = on && f >= 0 && f < T, xv = on && c.t >= c.ta;
        // (one descriptor per tensor over the whole sample: n's 24 channels are T * PO apart, its three clip channels T * P)
        __amdgpu_buffer_rsrc_t rg = cfn_rsrc(a.gy + (long)n * 24 * T * SP_PO, gbytes);
        __amdgpu_buffer_rsrc_t ry = cfn_rsrc((HASY ? a.y : a.gy) + (long)n * 24 * T * SP_PO, gbytes);
        __amdgpu_buffer_rsrc_t rs = cfn_rsrc(a.xs + (long)n * 24 * T * SP_PO, gbytes);
        __amdgpu_buffer_rsrc_t rx = cfn_rsrc(a.x + (long)n * 3 * T * SP_P, xbytes);
        // (the scalar offset is not range checked and must not be negative: the band's first input row, -1 for band 0, goes into the vector offset)
        const int ih0 = 2 * c.band * SP_RB - 1;
        const int sg = cfn_uni(fv ? (f * SP_PO + c.band * SP_RB * SP_WO) * 4 : 0);
        const int ss = cfn_uni(xv ? (c.t * SP_PO + c.band * SP_RB * SP_WO) * 4 : 0);
        const int sx = cfn_uni(xv ? c.t * SP_P * 4 : 0), rowoff = cfn_uni(ih0 * SP_WI * 4);
#pragma unroll
        for (int k = 0; k < SP_NGU; ++k) {
            fg[k] = __builtin_bit_cast(sp4, __builtin_amdgcn_raw_buffer_load_b128(rg, fv ? go[k] : SP_OOB, sg, 0));
            if (HASY) fy[k] = __builtin_bit_cast(sp4, __builtin_amdgcn_raw_buffer_load_b128(ry, fv ? go[k] : SP_OOB, sg, 0));
        }
#pragma unroll
        for (int k = 0; k < SP_NGU; ++k)
            fs[k] = __builtin_bit_cast(sp4, __builtin_amdgcn_raw_buffer_load_b128(rs, xv ? go[k] : SP_OOB, ss, 0));
#pragma unroll
        for (int k = 0; k < SP_NXU; ++k)
            fx[k] = __builtin_bit_cast(sp4, __builtin_amdgcn_raw_buffer_load_b128(rx, (xv && xo[k] != SP_OOB && ih0 + xr[k] >= 0) ? xo[k] + rowoff : SP_OOB, sx, 0));
    };

    const sp4 zero = {0.f, 0.f, 0.f, 0.f};
    sp4 W[5][SP_NGU];                                                         // g' of frames t - 2 .. t + 2
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int k = 0; k < SP_NGU; ++k) W[i][k] = zero;
    float gsv[SP_NGU], gqv[SP_NGU];
#pragma unroll
    for (int k = 0; k < SP_NGU; ++k) gsv[k] = gqv[k] = 0.0f;

    SpCur cc, fc;
    cc.start(first, R, nch, T);
    fc = cc;
    __syncthreads();
    fetch(fc);
    fc.next(R, nch, T);
    while (cc.run < last) {
        if (cc.t == cc.ta - 4) {                                               // a new run: the sample may have changed
#pragma unroll
            for (int k = 0; k < SP_NGU; ++k) {
                gsv[k] = a.gs ? (float)a.gs[cc.n * 24 + gc[k]] : 0.0f;
                gqv[k] = (HASY && a.gq) ? 2.0f * (float)a.gq[cc.n * 24 + gc[k]] : 0.0f;
            }
        }
        const bool mm = cc.t >= cc.ta;                                         // a frame of the run (not one of its four load-only steps)
        const float m = (cc.t + 2 >= 0 && cc.t + 2 < T) ? 1.0f : 0.0f;
#pragma unroll
        for (int k = 0; k < SP_NGU; ++k) {                                     // g'(t + 2), zero outside the clip
            sp4 v = fg[k] + gsv[k];
            if (HASY) v = __builtin_elementwise_fma(fy[k], (sp4){gqv[k], gqv[k], gqv[k], gqv[k]}, v);
            W[4][k] = v * m;
        }
        if (mm) {
#pragma unroll
            for (int k = 0; k < SP_NGU; ++k) {
                sp4 gx;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    gx[i] = sp_taps(W[0][k][i], W[1][k][i], W[2][k][i], W[3][k][i], W[4][k][i], wk[k][0], wk[k][1], wk[k][2], wk[k][3], wk[k][4]);
                if (gl[k] >= 0) {
                    *reinterpret_cast<sp2*>(gbuf + gl[k]) = (sp2){gx.x, gx.y};
                    *reinterpret_cast<sp2*>(gbuf + gl[k] + 2) = (sp2){gx.z, gx.w};
                }
                // xs(s), s = t: g'(s + 2 - j) = W[4 - j]
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const sp4 pr = fs[k] * W[4 - j][k];
                    acct[k][j] += (pr.x + pr.y) + (pr.z + pr.w);
                }
            }
#pragma unroll
            for (int k = 0; k < SP_NXU; ++k)                                   // rows above the image were not read: zeros
                if (xl[k] >= 0) *reinterpret_cast<sp4*>(img + xl[k]) = fx[k];
            __syncthreads();
        }
        fetch(fc);                                                             // in flight while this step is multiplied
        fc.next(R, nch, T);
        if (mm) {
#pragma unroll
            for (int j = 0; j < 14; j += 2) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j], bp[4 * j], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j + 2], bp[4 * j + 4], acc1, 0, 0, 0);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < SP_NGU; ++k) W[i][k] = W[i + 1][k];
        cc.next(R, nch, T);
    }

    // gw_t: the threads' partials meet through LDS, in a fixed order (channel co owns units [co UPC, (co + 1) UPC))
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SP_NGU; ++k)
        if (gl[k] >= 0) {
#pragma unroll
            for (int j = 0; j < 5; ++j) lds[(k * 512 + tid) * 5 + j] = acct[k][j];
        }
    __syncthreads();
    if (tid < 24 * 5) {
        const int co = tid / 5, j = tid - co * 5;
        float s = 0.0f;
        for (int u = 0; u < SP_UPC; ++u) s += lds[(co * SP_UPC + u) * 5 + j];
        cfn_add64(&a.gwt[co * 5 + j], (double)s);
    }
    __syncthreads();
    // gw_s: reduce the 8 waves' tiles through LDS (8 x 16 x 64 floats of the 8916)
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[(wave * 16 + r) * 64 + lane] = acc0[r] + acc1[r];
    __syncthreads();
    for (int e = tid; e < 16 * 64; e += 512) {
        const int r = e >> 6, l = e & 63, hh = l >> 5, col = l & 31;
        const int co = (r & 3) + 8 * (r >> 2) + 4 * hh;
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) s += lds[(w * 16 + r) * 64 + l];
        if (co < 24 && col < 27) cfn_add64(&a.gws[co * 27 + col], (double)s);
    }
}

// frames per run: the split of T that gives the shortest walk per workgroup (a run costs its frames + the halo re-read)
static int stem_pair_plan(int N, int T, int wgs) {
    int best = T;
    long best_cost = -1;
    for (int nch = 1; nch == 1 || T / nch >= 32; ++nch) {
        const int R = cfn_cdiv(T, nch);
        const long runs = (long)N * cfn_cdiv(T, R) * SP_BANDS, per = (runs + wgs - 1) / wgs, cost = per * (R + 2);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = R; }
    }
    return best;
}

static int stem_pair_cus() {
    static int cus = 0;
    if (!cus) { int dev = 0; hipDeviceProp_t pr; cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) ? pr.multiProcessorCount : 256; }
    return cus;
}

static bool stem_pair_shape_ok(int Cimg, int Cout, int T, int Hi, int Wi) {
    return Cimg == 3 && Cout == 24 && Hi == SP_WI && Wi == SP_WI && (long)24 * T * SP_PO * 4 < 0x7fff0000L;
}

extern "C" int cfn_stem_pair_bwd(const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w_t, const float* xs,
                                 const float* x, double* gw_t, double* gw_s, int N, int Cimg, int Cout, int T, int Hi, int Wi, int run_frames,
                                 void* stream) {
    CFN_REQUIRE(gy && w_t && xs && x && gw_t && gw_s, "cfn_stem_pair_bwd: null tensor");
    CFN_REQUIRE(gsumsq == nullptr || y != nullptr, "cfn_stem_pair_bwd: gsumsq needs y");
    CFN_REQUIRE(N > 0 && Cimg > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0 && run_frames >= 0, "cfn_stem_pair_bwd: bad shape");
    if (!stem_pair_shape_ok(Cimg, Cout, T, Hi, Wi)) return -1;
    const bool hasy = y != nullptr && gsumsq != nullptr;
    if ((((uintptr_t)gy | (uintptr_t)xs | (uintptr_t)x | (uintptr_t)(hasy ? y : gy)) & 15) != 0) return -1;
    const int wgs = stem_pair_cus();                                           // one persistent workgroup per CU
    const int R = run_frames > 0 ? (run_frames < T ? run_frames : T) : stem_pair_plan(N, T, wgs);
    const int nch = cfn_cdiv(T, R);
    const long runs = (long)N * nch * SP_BANDS;
    if (runs >= (1L << 30)) return -1;
    long blocks = runs < wgs ? runs : wgs;
    const long per = (runs + blocks - 1) / blocks;
    blocks = (runs + per - 1) / per;
    StemPairBwdArgs a = {gy, hasy ? y : nullptr, gsum, hasy ? gsumsq : nullptr, w_t, xs, x, gw_t, gw_s, N, T, R, nch, (int)runs, (int)per};
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, 4.0 * N * T * ((double)3 * SP_P + (double)24 * SP_PO * (hasy ? 3 : 2)));
    if (hasy) hipLaunchKernelGGL(stem_pair_bwd_kernel<true>, dim3((unsigned)blocks), dim3(512), 0, st, a);
    else hipLaunchKernelGGL(stem_pair_bwd_kernel<false>, dim3((unsigned)blocks), dim3(512), 0, st, a);
    return cfn_check_launch("stem_pair_bwd");
}

// ---- forward: xs = conv1_s(x) is written once and NOT read back: conv1_t reads it from a 5-frame register window --------------------------------
// A workgroup of 7 waves owns one run of frames [ta, tb) of one (sample, band of 2 output rows): 224 positions = 7 MFMA tiles of 32, wave w = tile w.
// Step s (s = ta - 2 .. tb + 1) computes xs(s) exactly as stem_fwd_kernel does (the same 14 v_mfma_f32_32x32x2 in the same k order, so the same
// bits; lane <-> position, register <-> channel), stores it if s is a frame of the run, and emits y(s - 2) = sum_k xs(s - 4 + k) w_t[k] with
// dwt5_fwd_flat_kernel's expression.  The two halo frames on either side of a run are recomputed from the clip (4 / R extra stem work); frames
// outside the clip are zero clip frames, whose conv is zero.  The clip band (3 x 5 rows) is double buffered in LDS: frame s + 1 is written while
// frame s is multiplied and frame s + 2 is in flight, one barrier per step.  Per-(n, c) sum / sumsq of y: fp32 per lane over the run, then
// lanes -> waves -> one fp64 accumulation per channel and workgroup.
// LDS offset of im2col row k = (ci, kh, kw) relative to the output position's first tap; k = 27 is the zero-weight pad of the 14th k-pair
static constexpr __host__ __device__ int sp_tap(int k) { return k < 27 ? (k / 9) * SP_CIS + ((k % 9) / 3) * SP_PITCH + k % 3 : 0; }

struct StemPairFwdArgs {
    const float* x; const float* ws; const float* wt; float* xs; float* y; double* s1; double* s2;
    int N, T, R, nch, runs;
};

__global__ __launch_bounds__(448, 4) void stem_pair_fwd_kernel(const StemPairFwdArgs a) {
    constexpr int NT = 448, NXU = (SP_XU + NT - 1) / NT, KP = 14;
    __shared__ __attribute__((aligned(16))) float img[2][3 * SP_CIS];
    __shared__ __attribute__((aligned(16))) float wts[24 * 8];
    __shared__ float wsl[14 * 64];                                             // conv1_s weight operand, [k-pair][lane]
    __shared__ float red[2][7][24];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6), half = lane >> 5, col = lane & 31;
    const int T = a.T;
    SpCur c;
    c.start((int)cfn_xcd_remap(blockIdx.x, gridDim.x), a.R, a.nch, T);
    const int n = c.n, band = c.band, ta = c.ta, tb = c.tb;

    for (int i = tid; i < 2 * 3 * SP_CIS; i += NT) (&img[0][0])[i] = 0.0f;    // the halo column stays zero for good
    if (tid < 24 * 5) wts[(tid / 5) * 8 + tid % 5] = a.wt[tid];

    const int ih0 = 2 * band * SP_RB - 1;                                      // the band's first input row (-1 for band 0: not read, stays zero)
    int xo[NXU], xl[NXU];
#pragma unroll
    for (int k = 0; k < NXU; ++k) {
        const int e = k * NT + tid;
        const int rowid = e / (SP_WI / 4), c4 = e - rowid * (SP_WI / 4), ci = rowid / SP_RIN, r = rowid - ci * SP_RIN;
        const bool in = e < SP_XU;
        xo[k] = (in && ih0 + r >= 0) ? (int)(((long)ci * T * SP_P + (long)(ih0 + r) * SP_WI + c4 * 4) * 4) : SP_OOB;
        xl[k] = in ? ci * SP_CIS + r * SP_PITCH + 4 + c4 * 4 : -1;
    }
    // weight operand: lane (co = col, k = 2s + half), as in stem_fwd_kernel (kept in LDS: 14 registers less, the window needs them)
    if (wave == 0) {
#pragma unroll
        for (int s = 0; s < KP; ++s) {
            const int k = 2 * s + half;
            wsl[s * 64 + lane] = (k < 27 && col < 24) ? a.ws[col * 27 + k] : 0.0f;
        }
    }
    const int pos = wave * 32 + col, ohl = pos / SP_WO, ow = pos - ohl * SP_WO;
    const int lboff = 2 * ohl * SP_PITCH + 2 * ow + 3;                         // tap (ci, kh, kw): + ci CIS + kh PITCH + kw

    const unsigned gbytes = (unsigned)((long)24 * T * SP_PO * 4), xbytes = (unsigned)((long)3 * T * SP_P * 4);
    __amdgpu_buffer_rsrc_t rx = cfn_rsrc(a.x + (long)n * 3 * T * SP_P, xbytes);
    __amdgpu_buffer_rsrc_t rs = cfn_rsrc(a.xs + (long)n * 24 * T * SP_PO, gbytes);
    __amdgpu_buffer_rsrc_t ry = cfn_rsrc(a.y + (long)n * 24 * T * SP_PO, gbytes);
    // output element of register r: channel (r & 3) + 8 (r >> 2) + 4 half; the channel's uniform part goes into the scalar offset
    const int vout = (half * 4 * T * SP_PO + band * SP_RB * SP_WO + pos) * 4;

    sp4 fx[NXU];
    auto fetch = [&](int s) {
        const bool fv = s >= 0 && s < T && s <= tb + 1;
        const int sx = cfn_uni(fv ? s * SP_P * 4 : 0);
#pragma unroll
        for (int k = 0; k < NXU; ++k)
            fx[k] = __builtin_bit_cast(sp4, __builtin_amdgcn_raw_buffer_load_b128(rx, fv ? xo[k] : SP_OOB, sx, 0));
    };
    auto put = [&](int b) {                                                    // rows above the image and frames outside the clip were not read: zeros
#pragma unroll
        for (int k = 0; k < NXU; ++k)
            if (xl[k] >= 0) *reinterpret_cast<sp4*>(&img[b][xl[k]]) = fx[k];
    };

    float W[5][12], st1[12], st2[12];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        st1[r] = st2[r] = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) W[i][r] = 0.0f;
    }

    fetch(ta - 2);
    __syncthreads();
    put(0);
    fetch(ta - 1);
    __syncthreads();
    int b = 0;
    for (int s = ta - 2; s <= tb + 1; ++s, b ^= 1) {
        put(b ^ 1);                                                            // frame s + 1 (its readers of step s - 1 are behind the barrier)
        fetch(s + 2);
        const float* lb = &img[b][lboff];
        int hsel = half;                                                       // (opaque: the 14 tap offsets of this lane's k = 2 s + half are then one
        asm volatile("" : "+v"(hsel));                                         // select each per step instead of 14 registers for the whole walk)
        sp16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int k = 0; k < KP; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wsl[k * 64 + lane], lb[hsel ? sp_tap(2 * k + 1) : sp_tap(2 * k)], acc, 0, 0, 0);
        const bool own = s >= ta && s < tb, emit = s - 2 >= ta;                // (s - 2 < tb by the loop bound)
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            const int cr = (r & 3) + 8 * (r >> 2);
            W[4][r] = acc[r];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, W[4][r]), rs, own ? vout : SP_OOB, cfn_uni(own ? (cr * T + s) * SP_PO * 4 : 0), 0);
        }
        if (emit) {
#pragma unroll
            for (int r = 0; r < 12; ++r) {
                const int cr = (r & 3) + 8 * (r >> 2);
                const float* wk = wts + (cr + 4 * half) * 8;
                const float yv = sp_taps(W[0][r], W[1][r], W[2][r], W[3][r], W[4][r], wk[0], wk[1], wk[2], wk[3], wk[4]);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), ry, vout, cfn_uni((cr * T + s - 2) * SP_PO * 4), 0);
                st1[r] += yv;
                st2[r] += yv * yv;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 12; ++r) W[i][r] = W[i + 1][r];
        __syncthreads();
    }
    if (a.s1) {
#pragma unroll
        for (int r = 0; r < 12; ++r) {
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) { st1[r] += __shfl_xor(st1[r], o, 64); st2[r] += __shfl_xor(st2[r], o, 64); }
            if (col == 0) {
                const int co = (r & 3) + 8 * (r >> 2) + 4 * half;
                red[0][wave][co] = st1[r];
                red[1][wave][co] = st2[r];
            }
        }
        __syncthreads();
        if (tid < 48) {
            const int which = tid / 24, co = tid - which * 24;
            float v = 0.0f;
#pragma unroll
            for (int w = 0; w < 7; ++w) v += red[which][w][co];
            cfn_add64((which ? a.s2 : a.s1) + n * 24 + co, (double)v);
        }
    }
}

// frames per run of the forward: a run costs its frames + 4 recomputed halo frames, `slots` workgroups run at a time; runs stay >= 32 frames
static int stem_pair_fwd_plan(int N, int T, int slots) {
    int best = T;
    long best_cost = -1;
    for (int nch = 1; nch == 1 || T / nch >= 32; ++nch) {
        const int R = cfn_cdiv(T, nch);
        const long runs = (long)N * cfn_cdiv(T, R) * SP_BANDS, rounds = (runs + slots - 1) / slots, cost = rounds * (R + 4);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = R; }
    }
    return best;
}

extern "C" int cfn_stem_pair_fwd(const float* x, const float* w_s, const float* w_t, float* xs, float* y, double* sum, double* sumsq, int N,
                                 int Cimg, int Cout, int T, int Hi, int Wi, int run_frames, void* stream) {
    CFN_REQUIRE(x && w_s && w_t && xs && y, "cfn_stem_pair_fwd: null tensor");
    CFN_REQUIRE((sum == nullptr) == (sumsq == nullptr), "cfn_stem_pair_fwd: sum/sumsq mismatch");
    CFN_REQUIRE(N > 0 && Cimg > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0 && run_frames >= 0, "cfn_stem_pair_fwd: bad shape");
    if (!stem_pair_shape_ok(Cimg, Cout, T, Hi, Wi)) return -1;
    if ((((uintptr_t)x | (uintptr_t)xs | (uintptr_t)y) & 15) != 0) return -1;
    const int R = run_frames > 0 ? (run_frames < T ? run_frames : T) : stem_pair_fwd_plan(N, T, 2 * stem_pair_cus());
    const int nch = cfn_cdiv(T, R);
    const long runs = (long)N * nch * SP_BANDS;
    if (runs >= (1L << 30)) return -1;
    StemPairFwdArgs a = {x, w_s, w_t, xs, y, sum, sumsq, N, T, R, nch, (int)runs};
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, 4.0 * N * T * ((double)3 * SP_P + (double)24 * SP_PO * 2));
    hipLaunchKernelGGL(stem_pair_fwd_kernel, dim3((unsigned)runs), dim3(448), 0, st, a);
    return cfn_check_launch("stem_pair_fwd");
}
