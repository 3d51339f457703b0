// Weight-STREAMING launcher of pws_kernel (pws_kernel.h, KCH = 3) for the deep pointwise contractions of layer 4 (x3d_fine.py:100-105: conv3
// 432 -> 192 forward, the data gradient of conv1 192 -> 432 = a contraction over its 432 output channels, conv5's data gradient).
//
// Why: the split-bf16 product wants every activation converted ONCE (prologue + 3-term split = ~12 VALU instructions per element, and these
// kernels are instruction-issue bound), i.e. a wave that owns ALL output rows of its positions -- pws_kernel's structure.  Its weight images
// are resident in LDS, and three images of 192 x 432 are 498 KB: at K = 432 a slab is 32 rows, six slabs convert every activation six times
// and the shape stayed on the fp32-MFMA pw_deep_kernel (64-row weight image, 52 TFLOP/s, 0.21-0.23 ms).  pwq_kernel (round 5, measured, not
// in the tree: DESIGN 4.4) kept the weights in registers instead -- three slabs of 64 rows, four k slices -- and was issue bound at 0.20 ms.
// Here the weights are split ONCE per launch into a workspace by pws_presplit_kernel (the byte image of the LDS chunk buffers, 580 KB,
// L2 resident) and stream through two LDS chunk buffers of 3 k-blocks while the waves multiply: 192 rows per slab, one conversion per element.
#include "pws_kernel.h"
#include <map>
#include <mutex>
#include <utility>

#define PWT_KCH 3                 // k-blocks per chunk = one trip of pws_kernel's operand ring
#define PWT_ROWB (PWT_KCH * 32 + 16)

// out[slab][chunk][term][BM][PWT_ROWB bytes]: term s of W[m0 + m][48 c + kk] (FWD: w is (M, K)) or W[48 c + kk][m0 + m] (DGRAD: w is (K, M)),
// zero beyond M / K.  grid (chunks, slabs, PWT_PRE_Z pieces of a chunk: one pair per thread and trip -- 9 workgroups of 18 dependent load -> store
// trips each took 14-17 us per launch); the 16 pad bytes of a row are never read
#define PWT_PRE_Z 8
template <int MODE>
__global__ __launch_bounds__(256) void pws_presplit_kernel(const float* __restrict__ w, int pitch, int M, int K, int BM, unsigned char* __restrict__ out) {
    const int c = blockIdx.x, slab = blockIdx.y, nchunks = gridDim.x, m0 = slab * BM;
    unsigned char* blob = out + ((size_t)slab * nchunks + c) * 3 * BM * PWT_ROWB;
    const int total = BM * (PWT_KCH * 8);                                  // pairs of one chunk
    for (int e = blockIdx.z * 256 + threadIdx.x; e < total; e += 256 * PWT_PRE_Z) {
        int m, kk;
        if (MODE == PW_FWD) { m = e / (PWT_KCH * 8); kk = (e - m * (PWT_KCH * 8)) * 2; }      // consecutive threads along k (w rows)
        else { kk = (e / BM) * 2; m = e - (e / BM) * BM; }                                     // consecutive threads along m (w rows)
        const int k = c * (PWT_KCH * 16) + kk;
        float v0 = 0.0f, v1 = 0.0f;
        if (m0 + m < M) {
            if (MODE == PW_FWD) {
                if (k < K) v0 = w[(long)(m0 + m) * pitch + k];
                if (k + 1 < K) v1 = w[(long)(m0 + m) * pitch + k + 1];
            } else {
                if (k < K) v0 = w[(long)k * pitch + m0 + m];
                if (k + 1 < K) v1 = w[(long)(k + 1) * pitch + m0 + m];
            }
        }
        unsigned p[3];
        pws_split<3>(v0, v1, p);
#pragma unroll
        for (int s = 0; s < 3; ++s) *reinterpret_cast<unsigned*>(blob + ((size_t)s * BM + m) * PWT_ROWB + kk * 2) = p[s];
    }
}

// One workspace per (device, stream), grown geometrically, never freed (a captured graph may have the address baked in); no allocation
// while the stream is being captured: the call is then declined and the fp32-MFMA kernel runs.  Launches on one stream run in order, so
// the next conv's pre-split cannot overtake this conv's contraction.  A hipGraph bakes the address in at capture time: it has to be REPLAYED ON THE
// STREAM IT WAS CAPTURED ON (cfn_hip/graph.py GraphedStep._replay does), otherwise eager work on the capture stream -- or a second graph captured
// on it and replayed elsewhere -- overwrites the split weights mid-contraction; the same holds for pwss_workspace (pwsplitw.hip).  Retired
// buffers stay allocated on purpose (a captured graph may still hold them); geometric growth bounds them by the size of the live one.
static unsigned char* pwt_workspace(size_t bytes, hipStream_t st) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, std::pair<unsigned char*, size_t>> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> lk(mu);
    auto& b = bufs[std::make_pair(dev, st)];
    if (b.second >= bytes) return b.first;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    const size_t want = bytes > 2 * b.second ? bytes : 2 * b.second;
    unsigned char* p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    b = {p, want};
    return p;
}

static size_t pwt_lds(int BM, int Kp) {
    const size_t red = (size_t)PWS_WAVES * 4 * (BM * 2 > 32 * 20 ? BM * 2 : 32 * 20);
    return (size_t)2 * 3 * BM * PWT_ROWB + (size_t)Kp * 16 + (size_t)BM * 8 + red;
}

template <int MODE, bool STATS, int ACT, bool TWO>
static int pwt_go_mt(const PwPlan& p, const PwArgs& a, hipStream_t st) {
#define PWT_GO(MTV) cfn_launch(pws_kernel<MTV, 1, MODE, STATS, ACT, TWO, 3, PWT_KCH>, p.blocks, p.threads, p.lds, st, a)
    switch (p.MT) { case 3: PWT_GO(3); break; case 4: PWT_GO(4); break; case 5: PWT_GO(5); break; default: PWT_GO(6); break; }
#undef PWT_GO
    return cfn_check_launch("pwconv(split bf16, streamed weights)");
}

template <int MODE, bool STATS, bool TWO>
static int pwt_go_act(const PwPlan& p, const PwArgs& a, hipStream_t st) {
    if constexpr (MODE == PW_DGRAD && !STATS) {
        return pwt_go_mt<MODE, STATS, CFN_ACT_NONE, TWO>(p, a, st);
    } else {
        switch (p.act) {
            case CFN_ACT_RELU: return pwt_go_mt<MODE, STATS, CFN_ACT_RELU, TWO>(p, a, st);
            case CFN_ACT_SWISH: return pwt_go_mt<MODE, STATS, CFN_ACT_SWISH, TWO>(p, a, st);
            default: return pwt_go_mt<MODE, STATS, CFN_ACT_NONE, TWO>(p, a, st);
        }
    }
}

// false when the shape is not handled.  DGRAD: stats == (ea != nullptr), i.e. with the act' epilogue
bool pwt_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p) {
    if (sw.split_terms != 6 || a.stem || a.stride != 1 || a.acc) return false;
    const bool deep = a.K >= 400, epi = mode == PW_DGRAD && stats && a.K >= 160 && a.M > 256;      // (why: the table of pwroute.hip)
    // whole 16-byte groups per row (Q % 4 == 0) are only needed by the forward's transposed epilogue (16-byte stores); the data gradient moves 4-byte
    // elements both ways -- the coarse stream's layer 4 (65 x 7 x 7 = 3,185 positions per row) runs its data gradients here
    if (!(deep || epi) || a.M <= 32 || (mode == PW_FWD && (a.Q & 3))) return false;
    if (a.act != CFN_ACT_NONE && a.act != CFN_ACT_RELU && a.act != CFN_ACT_SWISH) return false;
    if ((long)a.K * a.Q * 4 >= 0x3ffffff0L || (long)a.M * a.Q * 4 >= 0x3ffffff0L) return false;
    if ((p.align_io | p.align_ex) & (mode == PW_FWD ? 15 : 3)) return false;
    PwArgs& b = p.a;
    b = a;
    b.Kpad = (a.K + 47) / 48 * 48;
    if (mode == PW_DGRAD && !stats) b.act = CFN_ACT_NONE;
    // rows per slab: 6 row tiles (two chunk buffers of 7 do not fit LDS); as few slabs as possible, then as even as possible
    int slabs = cfn_cdiv(a.M, 32 * 6);
    int MT = cfn_cdiv(cfn_cdiv(a.M, slabs), 32);
    if (MT < 3) MT = 3;
    slabs = cfn_cdiv(a.M, 32 * MT);
    const int BM = 32 * MT, nchunks = b.Kpad / (16 * PWT_KCH);
    const size_t lds = pwt_lds(BM, b.Kpad);
    if (lds > 160 * 1024) return false;
    b.mtiles = slabs;
    b.kres = PWT_ROWB;
    const int ntiles = cfn_cdiv(a.Q, 32);
    const long groups = (long)a.N * slabs;
    long wgs = 256 / groups;                        // one 8-wave workgroup per CU, never more than one round of the chip
    const long maxw = cfn_cdiv(ntiles, PWS_WAVES);
    if (wgs > maxw) wgs = maxw;
    if (wgs < 1) wgs = 1;
    b.nstrips = (int)wgs;
    p.family = PW_FAM_PWT; p.mode = mode; p.stats = stats; p.two = a.src2 != nullptr; p.act = b.act;
    p.MT = MT; p.NP = 1; p.NS = 3;
    p.blocks = (unsigned)(groups * wgs); p.threads = 64 * PWS_WAVES; p.lds = lds;
    p.ws_bytes = (size_t)slabs * nchunks * 3 * BM * PWT_ROWB;
    return true;
}

// -1: no workspace (nothing launched)
int pwt_launch(const PwPlan& p, hipStream_t st) {
    unsigned char* ws = pwt_workspace(p.ws_bytes, st);
    if (!ws) return -1;
    PwArgs b = p.a;
    const int BM = 32 * p.MT, nchunks = b.Kpad / (16 * PWT_KCH);
    if (p.mode == PW_FWD) hipLaunchKernelGGL(pws_presplit_kernel<PW_FWD>, dim3(nchunks, b.mtiles, PWT_PRE_Z), dim3(256), 0, st, b.w, b.Cin, b.M, b.K, BM, ws);
    else hipLaunchKernelGGL(pws_presplit_kernel<PW_DGRAD>, dim3(nchunks, b.mtiles, PWT_PRE_Z), dim3(256), 0, st, b.w, b.Cin, b.M, b.K, BM, ws);
    { const int rc = cfn_check_launch("pwconv(split bf16, streamed weights) pre-split"); if (rc) return rc; }
    b.w = reinterpret_cast<const float*>(ws);
    if (p.mode == PW_FWD) return p.stats ? pwt_go_act<PW_FWD, true, false>(p, b, st) : pwt_go_act<PW_FWD, false, false>(p, b, st);
    if (p.two) return p.stats ? pwt_go_act<PW_DGRAD, true, true>(p, b, st) : pwt_go_act<PW_DGRAD, false, true>(p, b, st);
    return p.stats ? pwt_go_act<PW_DGRAD, true, false>(p, b, st) : pwt_go_act<PW_DGRAD, false, false>(p, b, st);
}
