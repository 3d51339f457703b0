// hipcc-flags: -fno-slp-vectorize
// One-pass backward of the spatially strided 1x1x1 shortcut conv of a stage-first block (Bottleneck.downsample, x3d_fine.py:284-287;
// 24->24 @112->56, 24->48 @56->28, 48->96 @28->14, 96->192 @14->7): the COMPACT data gradient and the weight gradient from one read of
// gy and y.  Run as two kernels (cfn_pwconv_bwd_data_acc on the output grid + cfn_pwconv_bwd_weight with stride 2) gy and y leave HBM twice
// and x is gathered element by element; here, per sample and strip of OUTPUT positions q = (t, oh, ow):
//   G'[m][q] = gsc*gy + gs + 2*gq*y                               (formed on load, staged in LDS as [row][stage + 1])
//   xl[k][q] = x[k][t][2 oh][2 ow]                                (even input rows only: one 16-byte load = two lattice elements)
//   da[k][q]  = sum_m W[m][k] G'[m][q]                            (compact, no act' epilogue: conv1's backward adds it on the lattice)
//   gw[m][k] += sum_q G'[m][q] act(A xl + B)[k][q]                (one fp64 accumulation per element per workgroup: cfn_add64)
// A workgroup of WM x WP waves walks its strip in stages of 64 positions (32 for 192x96) (global loads one stage ahead in registers, two LDS images, one
// barrier per stage).  Wave (wm, wp) owns the positions [wp*PT/WP, (wp+1)*PT/WP) of a stage and
//   weight gradient: the 32-row tiles i = wm*MT/WM .. of G' against all NT 32-row tiles of xl (v_mfma_f32_32x32x2, lane <-> channel row,
//                    k <-> position pair), prologue applied to the x operand as it is read;
//   data gradient:   the 16-row tiles t = wm*KT16/WM .. of da (v_mfma_f32_16x16x4, W^T resident in registers, B operand = G' rows),
//                    stored as 64-byte row segments.
// All arithmetic is fp32 MFMA.  Shapes with few channels split the POSITIONS over the waves (WM = 1: the layer-1 / layer-2 widths, as
// pw_bwd_fused_kernel does), the wide ones split the CHANNEL tiles (96x48: 3 x 2 waves, 192x96: 6 x 1), which keeps the accumulators of a
// wave at 32-48 registers.
#include "cfn_common.h"
#include <stdlib.h>

#include "pw_common.h"

typedef float __attribute__((ext_vector_type(4))) sf4;


struct PshArgs {
    const float* gy; const float* y; const double* gs; const double* gq; const double* gsc;
    const float* w;                       // (Cout, Cin) row major
    const float* x; const double* pa; const double* pb;
    float* da; double* gw;
    int N, M, K, Q, P;                    // M = Cout, K = Cin, Q = T*Ho*Wo, P = T*Hi*Wi
    int HiWi, Wi, HoWo, Wo, nstrips, stages;
};

// MT / NT: 32-row tiles of G' / xl;  KT16 = ceil(K / 16);  KS = ceil(M / 4);  VEC: 2 = 16-byte loads of gy, y and x (Q % 4 == 0, Wo even,
// even input rows 16-byte aligned), 1 = of gy and y only (odd Wo: layer 4's 7 x 7), 0 = every element is one dword load;  ACT: CFN_ACT_NONE (affine prologue or none) / CFN_ACT_RELU
template <int MT, int NT, int KT16, int KS, int WM, int WP, int PSH_PT, int VEC, int ACT, int OCC>
__global__ __launch_bounds__(64 * WM * WP, OCC) void pw_short_bwd_kernel(const PshArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTHR = 64 * WM * WP, PSH_PITCH = PSH_PT + 1;
    constexpr int BM = 32 * MT, BN = 32 * NT;
    constexpr int MTW = MT / WM, NTW16 = KT16 / WM;        // tiles of this wave
    constexpr int PW = PSH_PT / WP, NGRP = PW / 16;        // positions of this wave per stage, 16-position groups
    constexpr int GTR = PSH_PT / 4, XTR = PSH_PT / 2;                   // threads per staged row
    constexpr int GRS = NTHR / GTR, NG = (BM + GRS - 1) / GRS;          // G' staging: a float4 per thread
    constexpr int XRS = NTHR / XTR, NX = (16 * KT16 + XRS - 1) / XRS;   // xl staging: a position pair per thread
    static_assert(MT % WM == 0 && KT16 % WM == 0 && PSH_PT % (16 * WP) == 0 && 4 * KS <= BM && 16 * KT16 <= BN, "tile split");
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int wave = cfn_uni(tid >> 6), wm = wave / WP, wp = wave - wm * WP;
    const int m16 = lane & 15, kq = lane >> 4;
    const unsigned L = cfn_xcd_remap(blockIdx.x, gridDim.x);
    const int strip = L % a.nstrips;
    const int n = L / a.nstrips;
    const int M = a.M, K = a.K, Q = a.Q;

    constexpr int IMG = (BM + BN) * PSH_PITCH;         // one staged image: G' rows [BM][PT + 1] then xl rows [BN][PT + 1]
    float* img0 = smem;                                // two images (double buffer)
    float* sCg = smem + 2 * IMG;                       // [BM][2]  (gs, 2gq)
    float* sCz = sCg + 2 * BM;                         // [BM]     gsc
    for (int e = tid; e < 2 * IMG; e += NTHR) smem[e] = 0.0f;      // (xl rows >= 16*KT16 are never staged: they stay zero)
    for (int m = tid; m < BM; m += NTHR) {
        const bool ok = m < M;
        sCg[2 * m] = (ok && a.gs) ? (float)a.gs[(long)n * M + m] : 0.0f;
        sCg[2 * m + 1] = (ok && a.gq && a.y) ? 2.0f * (float)a.gq[(long)n * M + m] : 0.0f;
        sCz[m] = (ok && a.gsc) ? (float)a.gsc[(long)n * M + m] : 1.0f;
    }
    // W^T operand of the data gradient, resident: lane (ci = t*16 + m16, co = 4s + kq)
    float wq[NTW16][KS];
#pragma unroll
    for (int t = 0; t < NTW16; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int ci = (wm * NTW16 + t) * 16 + m16, co = 4 * s + kq;
            wq[t][s] = (ci < K && co < M) ? a.w[(long)co * K + ci] : 0.0f;
        }
    // prologue coefficients of this lane's xl rows in the weight-gradient operand (row j*32 + col)
    float ca[NT], cb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int k = j * 32 + col;
        const bool ok = a.pa != nullptr && k < K;
        ca[j] = ok ? (float)a.pa[(long)n * K + k] : 1.0f;
        cb[j] = ok ? (float)a.pb[(long)n * K + k] : 0.0f;
    }
    f16v acc[MTW][NT];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    __syncthreads();

    // Every global access of the stage loop is an UNCONDITIONAL buffer load / store (unwanted ones get an out-of-range offset: loads
    // return 0, stores are dropped), as in pw_bwd_fused_kernel.
    constexpr int OOB = 0x7ffffff0;
    __amdgpu_buffer_rsrc_t rg = cfn_rsrc(const_cast<float*>(a.gy + (long)n * M * Q), (unsigned)((long)M * Q * 4));
    __amdgpu_buffer_rsrc_t ry = cfn_rsrc(const_cast<float*>((a.y ? a.y : a.gy) + (long)n * M * Q), a.y ? (unsigned)((long)M * Q * 4) : 0u);
    __amdgpu_buffer_rsrc_t rx = cfn_rsrc(const_cast<float*>(a.x + (long)n * K * a.P), (unsigned)((long)K * a.P * 4));
    __amdgpu_buffer_rsrc_t rd = cfn_rsrc(a.da + (long)n * K * Q, (unsigned)((long)K * Q * 4));
    const int lrow = tid / GTR, c4 = (tid % GTR) * 4;
    const int xrow = tid / XTR, pp = (tid % XTR) * 2;
    sf4 pg[NG], py[NG];
    float px0[NX], px1[NX];
    int vog[NG], vox[NX];                                    // byte offsets of this thread's rows (position 0)
#pragma unroll
    for (int it = 0; it < NG; ++it) vog[it] = (it * GRS + lrow) < M ? ((it * GRS + lrow) * Q + c4) * 4 : OOB;
#pragma unroll
    for (int it = 0; it < NX; ++it) vox[it] = (it * XRS + xrow) < K ? (it * XRS + xrow) * a.P * 4 : OOB;
    // lattice offset (elements, inside one channel of x) of output position q
    auto xlat = [&](int q) {
        const int t = q / a.HoWo, r = q - t * a.HoWo;
        const int oh = r / a.Wo, ow = r - oh * a.Wo;
        return t * a.HiWi + 2 * oh * a.Wi + 2 * ow;
    };
    auto prefetch = [&](int q0) {
        if (VEC >= 1) {
            const bool inq = q0 + c4 < Q;
#pragma unroll
            for (int it = 0; it < NG; ++it) {
                const int vo = inq ? vog[it] : OOB;
                pg[it] = __builtin_bit_cast(sf4, __builtin_amdgcn_raw_buffer_load_b128(rg, vo, q0 * 4, 0));
                py[it] = __builtin_bit_cast(sf4, __builtin_amdgcn_raw_buffer_load_b128(ry, vo, q0 * 4, 0));
            }
        } else {
#pragma unroll
            for (int it = 0; it < NG; ++it) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int vo = (q0 + c4 + e < Q && vog[it] != OOB) ? vog[it] + 4 * e : OOB;
                    pg[it][e] = pw_bload(rg, vo, q0 * 4);
                    py[it][e] = pw_bload(ry, vo, q0 * 4);
                }
            }
        }
        const int qx = q0 + pp;
        if (VEC == 2) {
            // q0 + pp is even and Wo is even: both positions lie in one row, at even ow -> elements 0 and 2 of one aligned float4
            const int xo = qx < Q ? xlat(qx) * 4 : OOB;
#pragma unroll
            for (int it = 0; it < NX; ++it) {
                const sf4 v = __builtin_bit_cast(sf4, __builtin_amdgcn_raw_buffer_load_b128(rx, (xo == OOB || vox[it] == OOB) ? OOB : vox[it] + xo, 0, 0));
                px0[it] = v.x; px1[it] = v.z;
            }
        } else {
            const int xo0 = qx < Q ? xlat(qx) * 4 : OOB;
            const int xo1 = qx + 1 < Q ? xlat(qx + 1) * 4 : OOB;
#pragma unroll
            for (int it = 0; it < NX; ++it) {
                px0[it] = pw_bload(rx, (xo0 == OOB || vox[it] == OOB) ? OOB : vox[it] + xo0, 0);
                px1[it] = pw_bload(rx, (xo1 == OOB || vox[it] == OOB) ? OOB : vox[it] + xo1, 0);
            }
        }
    };
    auto stage = [&](int q0, float* sG, float* sX) {
#pragma unroll
        for (int it = 0; it < NG; ++it) {
            const int row = it * GRS + lrow;
            if (NG * GRS > BM && row >= BM) continue;
            const float cs = cfn_settle(sCg[2 * row]), cq = cfn_settle(sCg[2 * row + 1]), cz = cfn_settle(sCz[row]);
            const bool rok = row < M;
            float* d = sG + row * PSH_PITCH + c4;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (rok && q0 + c4 + e < Q) ? fmaf(py[it][e], cq, fmaf(pg[it][e], cz, cs)) : 0.0f;
        }
#pragma unroll
        for (int it = 0; it < NX; ++it) {
            const int row = it * XRS + xrow;
            if (NX * XRS > 16 * KT16 && row >= 16 * KT16) continue;
            float* d = sX + row * PSH_PITCH + pp;            // raw x; rows >= K and positions >= Q were loaded as 0
            d[0] = px0[it]; d[1] = px1[it];
        }
    };

    const int qbeg = strip * a.stages * PSH_PT;
    const int nst = min(a.stages, (Q - qbeg + PSH_PT - 1) / PSH_PT);
    if (nst > 0) {
        prefetch(qbeg);
        stage(qbeg, img0, img0 + BM * PSH_PITCH);
        if (nst > 1) prefetch(qbeg + PSH_PT);
    }
    __syncthreads();
    const int pbase = wp * PW;
    for (int st = 0; st < nst; ++st) {
        const int q0 = qbeg + st * PSH_PT;
        float* cur = img0 + (st & 1) * IMG;
        float* nxt = img0 + ((st + 1) & 1) * IMG;
        if (st + 1 < nst) {
            stage(q0 + PSH_PT, nxt, nxt + BM * PSH_PITCH);
            if (st + 2 < nst) prefetch(q0 + 2 * PSH_PT);
        }
        const float* sG = cur;
        const float* sX = cur + BM * PSH_PITCH;
        // ---- weight gradient: this wave's positions, its G' tiles against every xl tile ------------------------------
#pragma unroll
        for (int s = 0; s < PW / 2; ++s) {
            const int p = pbase + 2 * s + half;
            float av[MTW], bv[NT];
#pragma unroll
            for (int i = 0; i < MTW; ++i) av[i] = sG[((wm * MTW + i) * 32 + col) * PSH_PITCH + p];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float xr = cfn_settle(sX[(j * 32 + col) * PSH_PITCH + p]);
                bv[j] = cfn_act<ACT>(fmaf(xr, ca[j], cb[j]));
            }
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // (keeps the LDS reads of later steps from piling up in registers)
        }
        // ---- compact data gradient of the same positions, this wave's 16-row tiles ------------------------------------
        sf4 dv[NGRP][NTW16];
#pragma unroll
        for (int g = 0; g < NGRP; ++g)
#pragma unroll
            for (int t = 0; t < NTW16; ++t) dv[g][t] = (sf4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int g = 0; g < NGRP; ++g) {
                const float b = sG[(4 * s + kq) * PSH_PITCH + pbase + 16 * g + m16];
#pragma unroll
                for (int t = 0; t < NTW16; ++t) dv[g][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[t][s], b, dv[g][t], 0, 0, 0);
            }
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int g = 0; g < NGRP; ++g) {
            const int pl = pbase + 16 * g + m16;
            const bool qv = q0 + pl < Q;
#pragma unroll
            for (int t = 0; t < NTW16; ++t) {
                const sf4 v = dv[g][t];      // (components through scalars: indexing dv[g][t][r] in the unrolled loop stored component 0 four times)
                const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ci = (wm * NTW16 + t) * 16 + 4 * kq + r;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ve[r]), rd, (qv && ci < K) ? (ci * Q + pl) * 4 : OOB,
                                                          q0 * 4, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- weight gradient: combine the WP position groups through LDS in a fixed order, one fp64 accumulation per element ----
    constexpr int CWP = BN + 1;
    float* cw = smem + wp * (BM * CWP);        // [WP][BM][BN+1] over the (idle) images
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (wm * MTW + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                cw[ml * CWP + j * 32 + col] = acc[i][j][r];
            }
    __syncthreads();
    for (int e = tid; e < BM * BN; e += NTHR) {
        const int ml = e / BN, kl = e - ml * BN;
        const int o = ml * CWP + kl;
        float v = smem[o];
#pragma unroll
        for (int p = 1; p < WP; ++p) v += smem[p * BM * CWP + o];
        if (ml < M && kl < K) cfn_add64(&a.gw[(long)ml * K + kl], (double)v);
    }
}

template <int MT, int NT, int KT16, int KS, int WM, int WP, int PSH_PT, int OCC>
static int psh_go(const PshArgs& a, const PwBwdPlan& p, hipStream_t st) {
    const unsigned blocks = p.blocks;
    const size_t lds = p.lds;
#define CFN_PSH_GO(VECV, ACTV) cfn_launch(pw_short_bwd_kernel<MT, NT, KT16, KS, WM, WP, PSH_PT, VECV, ACTV, OCC>, blocks, 64 * WM * WP, lds, st, a)
    const bool relu = p.act == CFN_ACT_RELU;
    if (p.vec == 2) { if (relu) CFN_PSH_GO(2, CFN_ACT_RELU); else CFN_PSH_GO(2, CFN_ACT_NONE); }
    else if (p.vec == 1) { if (relu) CFN_PSH_GO(1, CFN_ACT_RELU); else CFN_PSH_GO(1, CFN_ACT_NONE); }
    else { if (relu) CFN_PSH_GO(0, CFN_ACT_RELU); else CFN_PSH_GO(0, CFN_ACT_NONE); }
#undef CFN_PSH_GO
    return cfn_check_launch("pwconv_short_bwd");
}

// false = declined (callers use the two separate entry points).  t[] = MT NT KT16 KS WM WP PT OCC of the variant
bool psh_plan(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p) {
    if (s.stride != 2) return false;
    if (!sw.pw_short) return false;      // 0 = the two separate kernels
    if (s.pro && s.act != CFN_ACT_NONE && s.act != CFN_ACT_RELU) return false;
    if (s.Cout > 192 || s.Cin > 96) return false;
    const int Ho = (s.Hi - 1) / 2 + 1, Wo = (s.Wi - 1) / 2 + 1;
    const long Ql = (long)s.T * Ho * Wo, Pl = (long)s.T * s.Hi * s.Wi;
    const int big = s.Cout > s.Cin ? s.Cout : s.Cin;
    if ((long)big * Pl * 4 >= 0x7ffffff0L || s.N > 65535) return false;       // 32-bit buffer offsets per sample
    if ((s.align_g | s.align_x | s.align_out) & 3) return false;
    // 16-byte loads: rows of gy / y start on 16 bytes (Q % 4); for x also: a position pair never straddles a row (Wo even), even input
    // rows start on 16 bytes (Wi even, Hi*Wi % 4) and every fourth column holds two lattice points
    const bool gvec = Ql % 4 == 0 && (s.align_g & 15) == 0;
    const bool xvec = Wo % 2 == 0 && s.Wi % 2 == 0 && ((long)s.Hi * s.Wi) % 4 == 0 && (s.align_x & 15) == 0;
    //                                 MT NT KT16 KS WM WP PT OCC
    static const int variants[4][8] = {{1, 1, 2, 6, 1, 4, 64, 3},        // layer 1: 24 -> 24
                                       {2, 1, 2, 12, 1, 4, 64, 2},       // layer 2: 24 -> 48
                                       {3, 2, 3, 24, 3, 2, 64, 1},       // layer 3: 48 -> 96
                                       {6, 3, 6, 48, 6, 1, 32, 1}};      // layer 4: 96 -> 192
    const int v = s.Cout <= 24 && s.Cin <= 32 ? 0 : (s.Cout <= 48 && s.Cin <= 32 ? 1 : (s.Cout <= 96 && s.Cin <= 48 ? 2 : 3));
    const int* t = variants[v];
    for (int i = 0; i < 8; ++i) p.t[i] = t[i];
    const int BM = 32 * t[0], BN = 32 * t[1], WP = t[5], PT = t[6], OCC = t[7];
    size_t lds = ((size_t)2 * (BM + BN) * (PT + 1) + 3 * BM) * sizeof(float);
    const size_t lds_cw = (size_t)WP * BM * (BN + 1) * sizeof(float);
    if (lds_cw > lds) lds = lds_cw;
    // whole rounds of the 256 CUs (OCC workgroups resident per CU): two rounds where a workgroup still gets >= 16 stages, else one;
    // a partly filled extra round costs a full one (pwfused.hip)
    const long nst = cfn_cdiv(Ql, PT);
    const long slots = 256L * OCC;
    const long rounds = (nst * s.N >= slots * 2 * 16) ? 2 : 1;
    long want = slots * rounds / s.N;
    if (want < 1) want = 1;
    long stages = cfn_cdiv(nst, want);
    if (stages < 4) stages = 4;
    p.family = PW_FAM_PSH; p.variant = v;
    p.stages = (int)stages;
    p.nstrips = (int)cfn_cdiv(nst, stages);
    p.blocks = (unsigned)((long)s.N * p.nstrips); p.threads = 64 * t[4] * t[5]; p.lds = lds;
    p.vec = gvec ? (xvec ? 2 : 1) : 0;
    p.act = s.pro && s.act == CFN_ACT_RELU ? CFN_ACT_RELU : CFN_ACT_NONE;
    return true;
}

static int psh_launch(const PwBwdPlan& p, const PshArgs& a, hipStream_t st) {
    switch (p.variant) {
        case 0: return psh_go<1, 1, 2, 6, 1, 4, 64, 3>(a, p, st);
        case 1: return psh_go<2, 1, 2, 12, 1, 4, 64, 2>(a, p, st);
        case 2: return psh_go<3, 2, 3, 24, 3, 2, 64, 1>(a, p, st);
        default: return psh_go<6, 3, 6, 48, 6, 1, 32, 1>(a, p, st);
    }
}

extern "C" int cfn_pwconv_short_bwd(const float* gy, const float* y, const double* gsum, const double* gsumsq, const double* gscale,
                                    const float* w, const float* x, const double* A, const double* B, int act, float* da, double* gw,
                                    int N, int Cin, int Cout, int T, int Hi, int Wi, int stride, void* stream) {
    CFN_REQUIRE(gy && w && x && da && gw, "cfn_pwconv_short_bwd: null tensor");
    CFN_REQUIRE((A == nullptr) == (B == nullptr), "cfn_pwconv_short_bwd: A/B mismatch");
    CFN_REQUIRE(gsumsq == nullptr || y != nullptr, "cfn_pwconv_short_bwd: gsumsq needs y");
    CFN_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0 && stride >= 1, "cfn_pwconv_short_bwd: bad shape");
    PwBwdShape s = {N, Cin, Cout, T, Hi, Wi, stride, act};
    s.pro = A != nullptr;
    s.align_g = (unsigned)(((uintptr_t)gy | (uintptr_t)(y ? y : gy)) & 15); s.align_x = (unsigned)((uintptr_t)x & 15); s.align_out = (unsigned)((uintptr_t)da & 15);
    PwBwdPlan p = {};
    if (!pw_route_short(s, pw_switches_now(true), p)) return -1;
    const int Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1;
    const long Ql = (long)T * Ho * Wo, Pl = (long)T * Hi * Wi;
    PshArgs a = {};
    a.gy = gy; a.y = gsumsq ? y : nullptr; a.gs = gsum; a.gq = gsumsq; a.gsc = gscale; a.w = w; a.x = x; a.pa = A; a.pb = B;
    a.da = da; a.gw = gw;
    a.N = N; a.M = Cout; a.K = Cin; a.Q = (int)Ql; a.P = (int)Pl;
    a.HiWi = Hi * Wi; a.Wi = Wi; a.HoWo = Ho * Wo; a.Wo = Wo;
    a.stages = p.stages; a.nstrips = p.nstrips;
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_PWCONV_BWD, st, 4.0 * N * ((double)Cout * Ql * (a.y ? 2 : 1) + (double)Cin * Ql * 3));
    return psh_launch(p, a, st);
}
