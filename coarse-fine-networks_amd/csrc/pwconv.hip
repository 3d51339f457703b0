// Pointwise (1x1x1) channel contractions of X3D (conv1/conv3/downsample/conv5/fc1:
// x3d_fine.py:100-105, :115, :119, :245-250, :256, :286) on the CDNA4 matrix cores.
//
// NCDHW keeps positions contiguous, so per sample the op is  Y[M x Q] = Wm[M x K] * X[K x Q].
// fp32 operands use v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, k-ordered):
//   A operand (weights, tiny, shared by the 4 waves)  -> LDS image As[k][m], conflict-free rows
//   B operand (activations, streamed once from HBM)    -> straight global->VGPR: lane (j=l&31,
//     kk=l>>5) reads X[k0+kk][q0+j], i.e. two fully used 128-byte lines per instruction, gets the
//     load-time prologue in registers and feeds the MFMA without touching LDS.
//   C: lane l holds position q0+(l&31) for 16 rows -> every store instruction writes 2 full lines.
// Modes:
//   PW_FWD    y = W * act(A x + B)            (+ per-(n,m) sum / sum-of-squares of y)
//   PW_DGRAD  da = W^T * (gy + gs + 2 y gq);  gx = da * act'(A x + B) * A  (+ sum(dz x), sum(dz))
//   pw_wgrad_kernel   gW[m][k] += (gy + gs + 2 y gq)[m,:] . act(A x + B)[k,:]   (both through LDS)
// Spatial stride 2 (shortcut conv, x3d_fine.py:284-287) is a position map on the strided side.
#include "cfn_common.h"
#include <stdlib.h>

#include "pw_common.h"

__device__ __forceinline__ int pw_pmap(int q, int Ho, int Wo, int Hi, int Wi, int stride) {
    if (stride == 1) return q;
    const int hw = Ho * Wo;
    const int t = q / hw, r = q - t * hw;
    const int oh = r / Wo, ow = r - oh * Wo;
    return (t * Hi + oh * stride) * Wi + ow * stride;
}

// One workgroup = 4 waves = a strip of `tpb` tiles of 128 positions x BM = 32*MT output rows.  The inner
// loop is branch-free: a unit of 8 input channels = 4 buffer loads per lane (SGPR row offset, one VGPR
// position offset, out-of-range rows read as 0 through the buffer bounds check) whose successors are
// already in flight while the 4*MT MFMAs of the current unit issue.
template <int MT, int MODE, bool STATS, int ACT, bool STEM>
__global__ __launch_bounds__(256) void pw_gemm_kernel(const PwArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BM = 32 * MT;
    constexpr int NU = PW_UNIT / 2;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int K = a.K, M = a.M, Q = a.Q, Kpad = a.Kpad, kres = a.kres;

    unsigned L = cfn_xcd_remap(blockIdx.x, gridDim.x);
    const int mtile = L % a.mtiles; L /= a.mtiles;
    const int strip = L % a.nstrips;
    const int n = L / a.nstrips;
    const int m0 = mtile * BM;

    float* As = smem;                                     // [kres][BM]
    float4* sP = reinterpret_cast<float4*>(As + kres * BM);   // [Kpad + PW_UNIT] prologue coefficients (FWD: A, B; DGRAD: gs, 2gq, gsc)
    float2* sE = reinterpret_cast<float2*>(sP + Kpad + PW_UNIT);   // [BM] epilogue coefficients (DGRAD)
    float* sSt = reinterpret_cast<float*>(sE + BM);       // [BM][2]
    float* red = sSt + 2 * BM + wave * (32 * PW_RED_PITCH);
    int2* sK = reinterpret_cast<int2*>(sSt + 2 * BM + 4 * (32 * PW_RED_PITCH));   // [Kpad + PW_UNIT] im2col row table (STEM)
    const int KV = STEM ? a.kT * a.kH * a.kW : 1;

    for (int k = tid; k < Kpad + PW_UNIT; k += 256) {
        float4 c;
        c.z = 1.0f; c.w = 0.0f;
        if (STEM) {
            const int ci = k / KV, r = k - ci * KV;
            const int kt = r / (a.kH * a.kW), r2 = r - kt * a.kH * a.kW, kh = r2 / a.kW, kw = r2 - kh * a.kW;
            c.x = (k < K && a.pa) ? a.pa[(long)n * a.Cimg + ci] : 1.0f;
            c.y = (k < K && a.pb) ? a.pb[(long)n * a.Cimg + ci] : 0.0f;
            int2 e;   // .x: element offset relative to the output position's base, .y: kt | kh<<8 | kw<<16 | valid<<24
            e.x = (int)((long)min(ci, a.Cimg - 1) * a.Pin) + ((kt - a.pT) * a.Hi + (kh - a.pH)) * a.Wi + (kw - a.pW);
            e.y = kt | (kh << 8) | (kw << 16) | ((k < K ? 1 : 0) << 24);
            sK[k] = e;
        } else if (MODE == PW_FWD) {
            c.x = (k < K && a.pa) ? a.pa[(long)n * K + k] : 1.0f;
            c.y = (k < K && a.pb) ? a.pb[(long)n * K + k] : 0.0f;
        } else {
            c.x = (k < K && a.gs) ? (float)a.gs[(long)n * K + k] : 0.0f;
            c.y = (k < K && a.gq && a.src2) ? 2.0f * (float)a.gq[(long)n * K + k] : 0.0f;
            c.z = (k < K && a.gsc) ? (float)a.gsc[(long)n * K + k] : 1.0f;
        }
        sP[k] = c;
    }
    for (int m = tid; m < BM; m += 256) {
        const bool ok = (m0 + m) < M && MODE == PW_DGRAD && a.ea;
        float2 c;
        c.x = ok ? a.ea[(long)n * M + m0 + m] : 1.0f;
        c.y = ok ? a.eb[(long)n * M + m0 + m] : 0.0f;
        sE[m] = c;
        sSt[2 * m] = 0.0f; sSt[2 * m + 1] = 0.0f;
    }
    auto load_w = [&](int kbase, int rows) {   // As[kk][m] = Wm[m0+m][kbase+kk], zero padded
        for (int e = tid; e < rows * BM; e += 256) {
            const int kk = e / BM, m = e - kk * BM;
            const int k = kbase + kk, mm = m0 + m;
            float v = 0.0f;
            if (k < K && mm < M) v = (MODE == PW_FWD) ? a.w[(long)mm * a.Cin + k] : a.w[(long)k * a.Cin + mm];
            As[e] = v;
        }
    };
    const bool resident = kres >= Kpad;
    if (resident) load_w(0, Kpad);
    __syncthreads();

    const bool two_src = MODE == PW_DGRAD && a.src2 != nullptr;
    const int src_pitch = MODE == PW_FWD ? a.Pin : Q;
    const int dst_pitch = MODE == PW_FWD ? Q : a.Pin;
    const long src_n = STEM ? (long)n * a.Cimg * a.Pin : (long)n * K * src_pitch;
    const long dst_n = (long)n * M * dst_pitch;
    const int row_bytes = src_pitch * 4;
    __amdgpu_buffer_rsrc_t r1 = cfn_rsrc(const_cast<float*>(a.src + src_n), STEM ? 0 : K * row_bytes);
    __amdgpu_buffer_rsrc_t r2 = cfn_rsrc(const_cast<float*>((two_src ? a.src2 : a.src) + src_n), STEM ? 0 : K * row_bytes);
    __amdgpu_buffer_rsrc_t rd = cfn_rsrc(a.dst + dst_n, M * dst_pitch * 4);
    __amdgpu_buffer_rsrc_t rx = cfn_rsrc(const_cast<float*>((a.ex ? a.ex : a.src) + (a.ex ? dst_n : 0)), a.ex ? M * dst_pitch * 4 : 0);
    __amdgpu_buffer_rsrc_t racc = cfn_rsrc(const_cast<float*>(MODE == PW_DGRAD && a.acc ? a.acc + (long)n * M * ((long)(a.Pin / (a.Hi * a.Wi)) * a.acc_Ho * a.acc_Wo) : a.src), MODE == PW_DGRAD && a.acc ? (unsigned)((long)M * (a.Pin / (a.Hi * a.Wi)) * a.acc_Ho * a.acc_Wo * 4) : 0u);
    float sacc[MT], qacc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) { sacc[i] = 0.0f; qacc[i] = 0.0f; }

    for (int tile = 0; tile < a.tpb; ++tile) {
        const int qt = (strip * a.tpb + tile) * 128;
        if (qt >= Q) break;
        const int q = qt + wave * 32 + col;
        const bool valid = q < Q;
        const int qc = valid ? q : Q - 1;
        const int pm = pw_pmap(qc, a.Ho, a.Wo, a.Hi, a.Wi, a.stride);
        const int in_pos = MODE == PW_FWD ? pm : qc;
        const int out_pos = MODE == PW_FWD ? qc : pm;
        const int voff = (half * src_pitch + in_pos) * 4;
        // implicit GEMM: input coordinates of this lane's output position (before adding the tap)
        int s_t = 0, s_h = 0, s_w = 0, s_pos = 0;
        const float* s_base = a.src + src_n;
        if (STEM) {
            const int hw = a.Ho * a.Wo;
            const int tq = qc / hw, rq = qc - tq * hw;
            const int oh = rq / a.Wo, ow = rq - oh * a.Wo;
            s_t = tq * a.sT; s_h = oh * a.sH; s_w = ow * a.sW;
            s_pos = (s_t * a.Hi + s_h) * a.Wi + s_w;
        }
        // rows k0 + 2j + half, j < NU; returns the in-bounds mask of the taps (STEM)
        auto bload = [&](int k0, float (&d)[NU], float (&d2)[NU]) -> unsigned {
            unsigned msk = 0;
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                if (STEM) {
                    const int2 e = sK[min(k0 + 2 * j + half, Kpad + PW_UNIT - 1)];
                    const int it = s_t + (e.y & 255) - a.pT, ih = s_h + ((e.y >> 8) & 255) - a.pH, iw = s_w + ((e.y >> 16) & 255) - a.pW;
                    const bool inb = (e.y >> 24) && it >= 0 && it < a.Ti && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi;
                    d[j] = s_base[inb ? (long)(s_pos + e.x) : 0];
                    msk |= (inb ? 1u : 0u) << j;
                } else {
                    d[j] = pw_bload(r1, voff, (k0 + 2 * j) * row_bytes);
                    if (MODE == PW_DGRAD) d2[j] = two_src ? pw_bload(r2, voff, (k0 + 2 * j) * row_bytes) : 0.0f;
                }
            }
            return msk;
        };

        f16v acc[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

        for (int kc0 = 0; kc0 < Kpad; kc0 += kres) {
            const int rows = min(kres, Kpad - kc0);
            if (!resident) {
                __syncthreads();
                load_w(kc0, rows);
                __syncthreads();
            }
            // two register sets ping-pong over the units: a set is reloaded right after it is consumed and is not touched
            // again for a whole unit, so no register copy (and no wait) sits at the end of a unit
            float ra[NU], ra2[NU], rb[NU], rb2[NU];
            auto unit = [&](const float (&cur)[NU], const float (&cur2)[NU], unsigned curm, int u) {
#pragma unroll
                for (int j = 0; j < NU; ++j) {
                    const int kl = u + 2 * j + half;
                    float v;
                    if (MODE == PW_FWD) {
                        const float2 c = *reinterpret_cast<const float2*>(&sP[kc0 + kl]);
                        v = cfn_act<ACT>(fmaf(cur[j], c.x, c.y));
                    } else {
                        const float4 c = sP[kc0 + kl];
                        v = fmaf(cur2[j], c.y, fmaf(cur[j], c.z, c.x));
                    }
                    if (STEM) v = ((curm >> j) & 1u) ? v : 0.0f;   // zero padding is applied after the prologue
                    const float* ar = As + kl * BM + col;
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[i * 32], v, acc[i], 0, 0, 0);
                }
            };
            unsigned ma = bload(kc0, ra, ra2), mb = bload(kc0 + PW_UNIT, rb, rb2);   // past the end reads 0 (bounds check)
            int u = 0;
            for (; u + 2 * PW_UNIT <= rows; u += 2 * PW_UNIT) {
                unit(ra, ra2, ma, u);
                ma = bload(kc0 + u + 2 * PW_UNIT, ra, ra2);
                __builtin_amdgcn_sched_barrier(0);
                unit(rb, rb2, mb, u + PW_UNIT);
                mb = bload(kc0 + u + 3 * PW_UNIT, rb, rb2);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (u < rows) unit(ra, ra2, ma, u);                   // odd number of units
        }

        // ---- epilogue ---------------------------------------------------------------------------
        // branch-free stores: rows >= M fall outside the per-sample buffer descriptor and are dropped by the
        // bounds check; lanes of a partial tile get an out-of-range offset.
        const float vm = valid ? 1.0f : 0.0f;
        const int dvoff = valid ? (4 * half * dst_pitch + out_pos) * 4 : 0x7fffffff;
        int avoff = 0x7fffffff;                                // compact offset of this lane's position on the acc lattice
        long acc_pitch = 0;
        if (MODE == PW_DGRAD && a.acc) {
            const int hw = a.Hi * a.Wi;
            const int tq = out_pos / hw, rq = out_pos - tq * hw;
            const int hq = rq / a.Wi, wq = rq - hq * a.Wi;
            acc_pitch = (long)(a.Pin / hw) * a.acc_Ho * a.acc_Wo;
            if (valid && hq % a.acc_s == 0 && wq % a.acc_s == 0)
                avoff = (int)((4 * half * acc_pitch + ((long)tq * a.acc_Ho + hq / a.acc_s) * a.acc_Wo + wq / a.acc_s) * 4);
        }
        const bool any_acc = MODE == PW_DGRAD && a.acc && __any(avoff != 0x7fffffff);   // tiles inside odd rows skip the loads
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            float t1[16], t2[16];
            float xe[16];
            if (MODE == PW_DGRAD && STATS) {   // STATS <=> the forward conv had a prologue (A,B given)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    xe[r] = pw_bload(rx, dvoff, (m0 + i * 32 + (r & 3) + 8 * (r >> 2)) * dst_pitch * 4);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                float v = acc[i][r];
                if (any_acc)
                    v += pw_bload(racc, avoff, (int)((m0 + i * 32 + (r & 3) + 8 * (r >> 2)) * acc_pitch * 4));
                if (MODE == PW_FWD) {
                    t1[r] = v * vm;
                } else if (STATS) {
                    const float2 c = sE[ml];
                    const float dz = v * cfn_act_grad<ACT>(fmaf(xe[r], c.x, c.y)) * vm;
                    t1[r] = dz * xe[r];
                    t2[r] = dz;
                    v = dz * c.x;
                }
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rd, dvoff,
                                                      (m0 + i * 32 + (r & 3) + 8 * (r >> 2)) * dst_pitch * 4, 0);
            }
            if (STATS) {
                // wave-private transpose through LDS (in-order per wave): lane -> (row lane&31, 16 of 32 columns)
#pragma unroll
                for (int pass = 0; pass < (MODE == PW_FWD ? 1 : 2); ++pass) {
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        red[((r & 3) + 8 * (r >> 2) + 4 * half) * PW_RED_PITCH + col] = pass == 0 ? t1[r] : t2[r];
                    asm volatile("" ::: "memory");
                    float s = 0.0f, qq = 0.0f;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const float v = red[col * PW_RED_PITCH + half * 16 + j];
                        s += v;
                        qq = fmaf(v, v, qq);
                    }
                    if (MODE == PW_FWD) { sacc[i] += s; qacc[i] += qq; }
                    else if (pass == 0) sacc[i] += s;
                    else qacc[i] += s;
                    asm volatile("" ::: "memory");
                }
            }
        }
    }

    if (STATS) {
        // per-wave slots in the (now idle) transpose scratch, then one fp64 atomic per row per workgroup
        __syncthreads();
        float* slot = sSt + 2 * BM;            // [4 waves][BM][2]  (4*BM*2 <= 4*32*33 floats)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const float s = sacc[i] + __shfl_xor(sacc[i], 32, 64);
            const float qq = qacc[i] + __shfl_xor(qacc[i], 32, 64);
            if (half == 0) { slot[(wave * BM + i * 32 + col) * 2] = s; slot[(wave * BM + i * 32 + col) * 2 + 1] = qq; }
        }
        __syncthreads();
        for (int m = tid; m < BM; m += 256) {
            if (m0 + m < M) {
                const float s = (slot[m * 2] + slot[(BM + m) * 2]) + (slot[(2 * BM + m) * 2] + slot[(3 * BM + m) * 2]);
                const float qq = (slot[m * 2 + 1] + slot[(BM + m) * 2 + 1]) + (slot[(2 * BM + m) * 2 + 1] + slot[(3 * BM + m) * 2 + 1]);
                cfn_add64(&a.s1[(long)n * M + m0 + m], (double)s);
                cfn_add64(&a.s2[(long)n * M + m0 + m], (double)qq);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// weight gradient: gW[m][k] = sum_{n,q} G[n,m,q] * Aop[n,k,p(q)]
//   block = (row tile of <=96 output channels) x (col tile of <=64 input channels) x one strip
//   of positions of one sample; positions are staged 64 at a time in LDS as [channel][65], the
//   4 waves split each stage's positions (in-block split-K), partials are combined through LDS
//   and leave the block as one fp64 atomic per element.
// ---------------------------------------------------------------------------------------------
#define WG_PT 64
#define WG_PITCH 65

struct WgArgs {
    const float* gy;     // (N,M,Q)
    const float* y;      // (N,M,Q) raw conv output, for the gq term (may be null)
    const double* gs; const double* gq;   // [n,m] (may be null)
    const double* gsc;                    // [n,m] scale of gy (null = 1)
    const float* x;      // (N,K,Pin) forward input raw
    const double* pa; const double* pb;     // forward prologue [n,k] (null = identity)
    double* gw;          // (M,K) fp64 accumulators, zero-filled by the caller
    int N, M, K, Q, Pin, Hi, Wi, Ho, Wo, stride, act;
    int mtiles, ktiles, nstrips, stages;   // stages = LDS stages (of 64 positions) per block
    int stem, Cimg, kT, kH, kW, sT, sH, sW, pT, pH, pW, Ti, To;   // stem != 0: x rows are im2col rows (see PwArgs)
};

template <int MTW, int NTW>
__global__ __launch_bounds__(256) void pw_wgrad_kernel(const WgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int BM = 32 * MTW, BN = 32 * NTW;
    constexpr int NG = BM / 16, NX = BN / 16;      // float4 per thread per stage (G rows / X rows)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    unsigned L = cfn_xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L % a.mtiles; L /= a.mtiles;
    const int kt = L % a.ktiles; L /= a.ktiles;
    const int strip = L % a.nstrips;
    const int n = L / a.nstrips;
    const int m0 = mt * BM, k0 = kt * BN;
    const int M = a.M, K = a.K, Q = a.Q;

    constexpr int IMG = (BM + BN) * WG_PITCH;          // one staged image: G rows [BM][65] then X rows [BN][65]
    float* img0 = smem;                                // two images (double buffer)
    float* sCg = smem + 2 * IMG;                       // [BM][2]  (gs, 2gq)
    float* sCx = sCg + 2 * BM;                         // [BN][2]  (A, B)
    float* sCz = sCx + 2 * BN;                         // [BM]     gsc
    for (int m = tid; m < BM; m += 256) {
        const bool ok = m0 + m < M;
        sCg[2 * m] = (ok && a.gs) ? (float)a.gs[(long)n * M + m0 + m] : 0.0f;
        sCg[2 * m + 1] = (ok && a.gq && a.y) ? 2.0f * (float)a.gq[(long)n * M + m0 + m] : 0.0f;
        sCz[m] = (ok && a.gsc) ? (float)a.gsc[(long)n * M + m0 + m] : 1.0f;
    }
    for (int k = tid; k < BN; k += 256) {
        const bool ok = k0 + k < K && a.pa;
        const long ci = a.stem ? (long)n * a.Cimg + (k0 + k) / (a.kT * a.kH * a.kW) : (long)n * K + k0 + k;
        sCx[2 * k] = ok ? a.pa[ci] : 1.0f;
        sCx[2 * k + 1] = ok ? a.pb[ci] : 0.0f;
    }
    f16v acc[MTW][NTW];
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    __syncthreads();

    // fast path: contiguous positions, float4 rows, next stage's global loads in flight during the MFMAs
    // (any Q: rows of an odd-sized volume -- 65 x 7 x 7 in the coarse stream -- start on 4-byte boundaries only; gfx950 takes 16-byte global
    // loads at any dword address, and the one float4 that straddles the end of a row is fetched element by element)
    const bool fast0 = a.stride == 1 && !a.stem;
    const int lrow = tid >> 4, c4 = (tid & 15) * 4;          // 16 lanes cover one 64-position row segment
    // unconditional raw buffer loads over the sample's block (range checked per dword: what lies beyond the block reads 0; the elements of a
    // straddling float4 that belong to the next row are masked when the stage is written)
    const bool big = (long)M * Q * 4 >= 0x7fff0000L || (long)K * Q * 4 >= 0x7fff0000L;      // (then: the gather path)
    __amdgpu_buffer_rsrc_t rbg = cfn_rsrc(a.gy + (long)n * M * Q, (unsigned)((long)M * Q * 4));
    __amdgpu_buffer_rsrc_t rby = cfn_rsrc((a.y ? a.y : a.gy) + (long)n * M * Q, a.y ? (unsigned)((long)M * Q * 4) : 0u);
    __amdgpu_buffer_rsrc_t rbx = cfn_rsrc(a.x + (long)n * K * a.Pin, (unsigned)((long)K * Q * 4));
    const bool fast = fast0 && !big;
    f4v pg[NG], py[NG], px[NX];
    auto prefetch = [&](int q0) {
        constexpr int OOBW = 0x7fffff00;
        const bool inq = q0 + c4 < Q;
#pragma unroll
        for (int it = 0; it < NG; ++it) {
            const int ch = m0 + it * 16 + lrow;
            const int vo = (ch < M && inq) ? (ch * Q + q0 + c4) * 4 : OOBW;
            pg[it] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rbg, vo, 0, 0));
            py[it] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rby, vo, 0, 0));
        }
#pragma unroll
        for (int it = 0; it < NX; ++it) {
            const int ch = k0 + it * 16 + lrow;
            px[it] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rbx, (ch < K && inq) ? (ch * Q + q0 + c4) * 4 : OOBW, 0, 0));
        }
    };
    auto stage_fast = [&](int q0, float* sG, float* sX) {
        const int qa = q0 + c4;                                  // element u is inside the row when qa + u < Q (the constant terms must not leak past it)
#pragma unroll
        for (int it = 0; it < NG; ++it) {
            const int row = it * 16 + lrow;
            const float cs = cfn_settle(sCg[2 * row]), cq = cfn_settle(sCg[2 * row + 1]), cz = cfn_settle(sCz[row]);      // (an LDS pair in front of packed FMAs: DESIGN 4.1; found by the per-half scan)
            const bool ok = m0 + row < M;
            float* d = sG + row * WG_PITCH + c4;
            d[0] = (ok && qa < Q) ? fmaf(py[it].x, cq, fmaf(pg[it].x, cz, cs)) : 0.0f;
            d[1] = (ok && qa + 1 < Q) ? fmaf(py[it].y, cq, fmaf(pg[it].y, cz, cs)) : 0.0f;
            d[2] = (ok && qa + 2 < Q) ? fmaf(py[it].z, cq, fmaf(pg[it].z, cz, cs)) : 0.0f;
            d[3] = (ok && qa + 3 < Q) ? fmaf(py[it].w, cq, fmaf(pg[it].w, cz, cs)) : 0.0f;
        }
#pragma unroll
        for (int it = 0; it < NX; ++it) {
            const int row = it * 16 + lrow;
            const float ca = sCx[2 * row], cb = sCx[2 * row + 1];
            const bool ok = k0 + row < K;
            float* d = sX + row * WG_PITCH + c4;
            d[0] = (ok && qa < Q) ? cfn_act_rt(fmaf(px[it].x, ca, cb), a.act) : 0.0f;
            d[1] = (ok && qa + 1 < Q) ? cfn_act_rt(fmaf(px[it].y, ca, cb), a.act) : 0.0f;
            d[2] = (ok && qa + 2 < Q) ? cfn_act_rt(fmaf(px[it].z, ca, cb), a.act) : 0.0f;
            d[3] = (ok && qa + 3 < Q) ? cfn_act_rt(fmaf(px[it].w, ca, cb), a.act) : 0.0f;
        }
    };
    auto stage_slow = [&](int q0, float* sG, float* sX) {          // strided / im2col / ragged positions: element-wise gather
        for (int e = tid; e < (BM + BN) * (WG_PT / 4); e += 256) {
            const int row = e / (WG_PT / 4), cc = (e - row * (WG_PT / 4)) * 4;
            const bool isg = row < BM;
            const int ch = isg ? m0 + row : k0 + row - BM;
            const bool chok = isg ? ch < M : ch < K;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (chok) {
                if (isg) {
                    const long base = ((long)n * M + ch) * Q + q0 + cc;
                    const float cs = cfn_settle(sCg[2 * row]), cq = cfn_settle(sCg[2 * row + 1]), cz = cfn_settle(sCz[row]);      // (an LDS pair in front of packed FMAs: DESIGN 4.1; found by the per-half scan)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (q0 + cc + u < Q) v[u] = fmaf(a.y ? a.y[base + u] : 0.0f, cq, fmaf(a.gy[base + u], cz, cs));
                } else {
                    const int kr = row - BM;
                    const float ca = sCx[2 * kr], cb = sCx[2 * kr + 1];
                    if (a.stem) {
                        const int KV = a.kT * a.kH * a.kW;
                        const int ci = ch / KV, r = ch - ci * KV;
                        const int kt = r / (a.kH * a.kW), r2 = r - kt * a.kH * a.kW, kh = r2 / a.kW, kw = r2 - kh * a.kW;
                        const int hw = a.Ho * a.Wo;
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int qq = q0 + cc + u;
                            if (qq < Q) {
                                const int tq = qq / hw, rq = qq - tq * hw;
                                const int oh = rq / a.Wo, ow = rq - oh * a.Wo;
                                const int it = tq * a.sT + kt - a.pT, ih = oh * a.sH + kh - a.pH, iw = ow * a.sW + kw - a.pW;
                                if (it >= 0 && it < a.Ti && ih >= 0 && ih < a.Hi && iw >= 0 && iw < a.Wi)
                                    v[u] = cfn_act_rt(fmaf(a.x[((long)n * a.Cimg + ci) * a.Pin + ((long)it * a.Hi + ih) * a.Wi + iw], ca, cb), a.act);
                            }
                        }
                    } else {
                        const long base = ((long)n * K + ch) * a.Pin;
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (q0 + cc + u < Q)
                                v[u] = cfn_act_rt(fmaf(a.x[base + pw_pmap(q0 + cc + u, a.Ho, a.Wo, a.Hi, a.Wi, a.stride)], ca, cb), a.act);
                    }
                }
            }
            float* d = (isg ? sG + row * WG_PITCH : sX + (row - BM) * WG_PITCH) + cc;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
        }
    };

    // Double-buffered images, ONE barrier per stage: inside a stage the LDS writes of stage s+1 (from registers
    // loaded one stage earlier) and the global loads of stage s+2 sit in the same basic block as the MFMAs of
    // stage s, so the compiler interleaves the staging VALU/LDS work under the matrix pipe.
    const int qbeg = strip * a.stages * WG_PT;
    const int nst = min(a.stages, (Q - qbeg + WG_PT - 1) / WG_PT);
    if (nst > 0) {
        if (fast) {
            prefetch(qbeg);
            stage_fast(qbeg, img0, img0 + BM * WG_PITCH);
            if (nst > 1) prefetch(qbeg + WG_PT);
        } else {
            stage_slow(qbeg, img0, img0 + BM * WG_PITCH);
        }
    }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int q0 = qbeg + st * WG_PT;
        float* cur = img0 + (st & 1) * IMG;
        float* nxt = img0 + ((st + 1) & 1) * IMG;
        if (st + 1 < nst) {
            if (fast) {
                stage_fast(q0 + WG_PT, nxt, nxt + BM * WG_PITCH);
                if (st + 2 < nst) prefetch(q0 + 2 * WG_PT);
            } else {
                stage_slow(q0 + WG_PT, nxt, nxt + BM * WG_PITCH);
            }
        }
        // ---- each wave contracts its 16 positions of the stage ---------------------------------
        const float* sG = cur;
        const float* sX = cur + BM * WG_PITCH;
        const int pbase = wave * (WG_PT / 4);
#pragma unroll
        for (int s = 0; s < WG_PT / 8; ++s) {
            const int p = pbase + 2 * s + half;
            float av[MTW], bv[NTW];
#pragma unroll
            for (int i = 0; i < MTW; ++i) av[i] = sG[(i * 32 + col) * WG_PITCH + p];
#pragma unroll
            for (int j = 0; j < NTW; ++j) bv[j] = sX[(j * 32 + col) * WG_PITCH + p];
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // ---- combine the 4 waves through LDS (plain stores into per-wave images: LDS float atomics from 4 waves on
    // the same addresses cost ~1 us per instruction), then one fp64 atomic per element per workgroup --------------
    constexpr int CWP = BN + 1;
    float* cw = smem + wave * (BM * CWP);      // [4][BM][BN+1]
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                cw[ml * CWP + j * 32 + col] = acc[i][j][r];
            }
    __syncthreads();
    for (int e = tid; e < BM * BN; e += 256) {
        const int ml = e / BN, kl = e - ml * BN;
        const int o = ml * CWP + kl;
        const float v = (smem[o] + smem[BM * CWP + o]) + (smem[2 * BM * CWP + o] + smem[3 * BM * CWP + o]);
        if (m0 + ml < M && k0 + kl < K) cfn_add64(&a.gw[(long)(m0 + ml) * K + k0 + kl], (double)v);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <int MODE, bool STATS, int ACT, bool STEM>
static int pw_launch_mt(const PwArgs& a, int MT, unsigned blocks, size_t lds, hipStream_t st) {
#define CFN_PW_GO(MTV) cfn_launch(pw_gemm_kernel<MTV, MODE, STATS, ACT, STEM>, blocks, 256, lds, st, a)
    switch (MT) {
        case 1: CFN_PW_GO(1); break;
        case 2: CFN_PW_GO(2); break;
        case 3: CFN_PW_GO(3); break;
        default: CFN_PW_GO(4); break;
    }
#undef CFN_PW_GO
    return cfn_check_launch("pwconv");
}

template <int MODE, bool STATS>
static int pw_launch(const PwArgs& a, int act, int MT, unsigned blocks, size_t lds, hipStream_t st) {
    switch (act) {
        case CFN_ACT_RELU: return pw_launch_mt<MODE, STATS, CFN_ACT_RELU, false>(a, MT, blocks, lds, st);
        case CFN_ACT_SWISH: return pw_launch_mt<MODE, STATS, CFN_ACT_SWISH, false>(a, MT, blocks, lds, st);
        default: return pw_launch_mt<MODE, STATS, CFN_ACT_NONE, false>(a, MT, blocks, lds, st);
    }
}

// false: a sample's tensor is beyond the 2 GiB buffer-descriptor range (pw_too_large reports it)
static bool pw_plan(PwArgs& a, int& MT, unsigned& blocks, size_t& lds) {
    a.Kpad = (a.K + PW_UNIT - 1) / PW_UNIT * PW_UNIT;
    a.kres = a.Kpad <= PW_KRES_MAX ? a.Kpad : PW_KRES_MAX;
    const int M32 = cfn_cdiv(a.M, 32);
    // rows per workgroup: as many 32-row tiles as keep the resident weight image <= 64 KiB (max 4),
    // then the smallest tile that covers M with that number of row tiles
    int mt_fit = (64 * 1024 / 4 / a.kres) / 32;
    // measured: occupancy beats register tiling here -- 32-row tiles when the weight image is deep (K >= 96, the
    // MFMA-bound layers 3-4), at most 64 rows otherwise
    if (mt_fit > 2) mt_fit = 2;
    if (a.K >= 96 && !a.stem) mt_fit = 1;
    if (a.ea && mt_fit > 2) mt_fit = 2;   // DGRAD with the act' epilogue: keep the register footprint spill-free
    if (mt_fit < 1) mt_fit = 1;
    const int ntile = cfn_cdiv(M32, mt_fit);
    MT = cfn_cdiv(M32, ntile);
    a.mtiles = cfn_cdiv(a.M, 32 * MT);
    const int BM = 32 * MT;
    const long tiles = cfn_cdiv(a.Q, 128);
    // ~4 workgroups per CU (measured 512 / 768 / 1024 / 1536 / 2048: 24->54 @112 2.00 / 1.90 / 1.82 / 1.85 / 1.84 ms): long strips amortise the per-workgroup statistics atomics (all workgroups of one
    // (n, row) hit the same fp64 address) and the weight staging
    long tpb = (tiles * a.N * a.mtiles + 1023) / 1024;
    if (tpb < 1) tpb = 1;
    a.tpb = (int)tpb;
    a.nstrips = cfn_cdiv(tiles, tpb);
    blocks = (unsigned)((long)a.N * a.nstrips * a.mtiles);
    lds = ((size_t)a.kres * BM + 4 * (a.Kpad + PW_UNIT) + 2 * BM + 2 * BM + 4 * 32 * PW_RED_PITCH + (a.stem ? 2 * (a.Kpad + PW_UNIT) : 0)) * sizeof(float);
    return !((!a.stem && ((long)a.K * a.Pin * 4 >= (1L << 31) || (long)a.K * a.Q * 4 >= (1L << 31))) ||
             (long)a.M * a.Pin * 4 >= (1L << 31) || (long)a.M * a.Q * 4 >= (1L << 31));
}

static int pw_too_large(const PwArgs& a) {
    const long span = (long)a.K * (a.stem ? 1 : (a.src2 || a.gs || a.gq || a.ex ? a.Q : a.Pin)) * 4;
    return cfn_fail(CFN_ERR_UNSUPPORTED, "pwconv: one sample's K x positions x 4 B = %ld exceeds the 2 GiB buffer-descriptor range", span);
}

bool pw_gemm_plan(const PwArgs& a, int mode, bool stats, const PwSwitches&, PwPlan& p) {
    p.a = a;
    size_t lds;
    if (!pw_plan(p.a, p.MT, p.blocks, lds)) return false;
    if (mode == PW_DGRAD && !stats) p.a.act = CFN_ACT_NONE;
    p.family = PW_FAM_GEMM; p.mode = mode; p.stats = stats; p.two = a.src2 != nullptr;
    p.act = p.a.act == CFN_ACT_RELU || p.a.act == CFN_ACT_SWISH ? p.a.act : CFN_ACT_NONE;
    p.threads = 256; p.lds = lds;
    return true;
}

int pw_gemm_launch(const PwPlan& p, hipStream_t st) {
    if (p.mode == PW_FWD)
        return p.stats ? pw_launch<PW_FWD, true>(p.a, p.act, p.MT, p.blocks, p.lds, st) : pw_launch<PW_FWD, false>(p.a, p.act, p.MT, p.blocks, p.lds, st);
    if (!p.stats) return pw_launch<PW_DGRAD, false>(p.a, p.act, p.MT, p.blocks, p.lds, st);
    return pw_launch<PW_DGRAD, true>(p.a, p.act, p.MT, p.blocks, p.lds, st);
}

static void pw_geom(PwArgs& a, int T, int Hi, int Wi, int stride) {
    a.Hi = Hi; a.Wi = Wi; a.stride = stride;
    a.Ho = (Hi - 1) / stride + 1;
    a.Wo = (Wi - 1) / stride + 1;
    a.Pin = T * Hi * Wi;
    a.Q = T * a.Ho * a.Wo;
}

// gx (N*M, T, Hi, Wi) += acc (N*M, T, Ho, Wo) on the lattice h % s == w % s == 0: the compact gradient of the strided shortcut conv of a stage's
// first block, for the data gradients WITHOUT act' epilogue whose contraction runs on a split-bf16 kernel (those decline `acc`: the
// lattice loads cost their many-row variants 90+ registers).  Without an epilogue "W^T g' + acc" is the same fp32 sum whether the second
// term is added before the store or after it.  One thread = one compact element, rows of the lattice in order.
__global__ __launch_bounds__(256) void pw_lattice_add_kernel(float* __restrict__ gx, const float* __restrict__ acc, long total, int Ho, int Wo,
                                                             int Hi, int Wi, int s) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int wo = (int)(e % Wo);
    const long r = e / Wo;
    const int ho = (int)(r % Ho);
    const long plane = r / Ho;                                              // (n, m, t)
    float* p = gx + (plane * Hi + (long)ho * s) * Wi + (long)wo * s;
    *p += acc[e];
}

// Route (pwroute.hip), then launch: the first family whose plan accepts and whose launcher gets its workspace.  Where the plan says lattice_add, the
// contraction ran without the compact shortcut gradient a.acc and pw_lattice_add_kernel adds it behind it.
static int pw_run(const PwArgs& a, int mode, bool stats, hipStream_t st) {
    const PwSwitches sw = pw_switches_now(false);
    PwPlan p = {};
    p.align_io = (unsigned)(((uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.src2) & 15);
    p.align_ex = (unsigned)((uintptr_t)a.ex & 15);
    for (int from = 0; mode == PW_FWD ? pw_route_fwd(a, stats, sw, p, from) : pw_route_dgrad(a, stats, sw, p, from); from = p.slot + 1) {
        int rc;
        switch (p.family) {
            case PW_FAM_PWK: rc = pwk_launch(p, st); break;
            case PW_FAM_PWT: rc = pwt_launch(p, st); break;
            case PW_FAM_PWS: rc = pws_launch(p, st); break;
            case PW_FAM_PWD: rc = pwd_launch(p, st); break;
            default: rc = pw_gemm_launch(p, st); break;
        }
        if (rc < 0) continue;
        if (rc > 0 || !p.lattice_add) return rc;
        const long total = (long)a.N * a.M * (a.Pin / (a.Hi * a.Wi)) * a.acc_Ho * a.acc_Wo;
        hipLaunchKernelGGL(pw_lattice_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.dst, a.acc, total, a.acc_Ho, a.acc_Wo, a.Hi, a.Wi,
                           a.acc_s);
        return cfn_check_launch("pwconv_bwd_data(lattice add)");
    }
    return pw_too_large(a);
}

extern "C" int cfn_pwconv_fwd(const float* x, const double* A, const double* B, int act, const float* w, float* y,
                              double* sum, double* sumsq, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride,
                              void* stream) {
    CFN_REQUIRE(x && w && y, "cfn_pwconv_fwd: null tensor");
    CFN_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_pwconv_fwd: bad shape");
    CFN_REQUIRE(stride == 1 || stride == 2, "cfn_pwconv_fwd: stride must be 1 or 2");
    CFN_REQUIRE((A == nullptr) == (B == nullptr), "cfn_pwconv_fwd: A/B mismatch");
    CFN_REQUIRE((sum == nullptr) == (sumsq == nullptr), "cfn_pwconv_fwd: sum/sumsq mismatch");
    PwArgs a = {};
    a.src = x; a.pa = A; a.pb = B; a.act = act; a.w = w; a.dst = y; a.s1 = sum; a.s2 = sumsq;
    a.N = N; a.M = Cout; a.K = Cin; a.Cin = Cin;
    pw_geom(a, T, Hi, Wi, stride);
    CFN_REQUIRE((long)T * Hi * Wi < (1L << 31), "cfn_pwconv_fwd: per-sample volume too large");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_PWCONV_FWD, st, 4.0 * N * ((double)Cin * a.Q + (double)Cout * a.Q) + 4.0 * Cin * Cout);
    return pw_run(a, PW_FWD, sum != nullptr, st);
}

// gx must be zero-filled by the caller when stride == 2 (only the strided positions are written)
// acc (optional): compact gradient (N,Cin,T,acc_Ho,acc_Wo) of a stride-acc_stride shortcut conv over the same input,
// added on its lattice before the act' epilogue (stride must be 1 then)
extern "C" int cfn_pwconv_bwd_data_acc(const float* gy, const float* y, const double* gsum, const double* gsumsq,
                                   const float* w, const float* x, const double* A, const double* B, int act, float* gx,
                                   double* gA, double* gB, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride,
                                   const float* acc, int acc_stride, const double* gscale, void* stream) {
    CFN_REQUIRE(gy && w && gx, "cfn_pwconv_bwd_data: null tensor");
    CFN_REQUIRE(stride == 1 || stride == 2, "cfn_pwconv_bwd_data: stride must be 1 or 2");
    CFN_REQUIRE((A == nullptr) == (B == nullptr), "cfn_pwconv_bwd_data: A/B mismatch");
    CFN_REQUIRE(A == nullptr || (x && gA && gB), "cfn_pwconv_bwd_data: prologue needs x, gA, gB");
    CFN_REQUIRE(gsumsq == nullptr || y != nullptr, "cfn_pwconv_bwd_data: gsumsq needs y");
    CFN_REQUIRE(acc == nullptr || (stride == 1 && acc_stride >= 1), "cfn_pwconv_bwd_data_acc: acc needs stride 1");
    PwArgs a = {};
    a.src = gy; a.src2 = gsumsq ? y : nullptr; a.gs = gsum; a.gq = gsumsq; a.gsc = gscale; a.w = w; a.dst = gx;
    a.ex = x; a.ea = A; a.eb = B; a.act = act; a.s1 = gA; a.s2 = gB;
    a.N = N; a.M = Cin; a.K = Cout; a.Cin = Cin;
    pw_geom(a, T, Hi, Wi, stride);
    if (acc) { a.acc = acc; a.acc_s = acc_stride; a.acc_Ho = (Hi - 1) / acc_stride + 1; a.acc_Wo = (Wi - 1) / acc_stride + 1; }
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_PWCONV_BWD, st, 4.0 * N * ((double)Cout * a.Q * (a.src2 ? 2 : 1) + (double)Cin * a.Q * (A ? 2 : 1)));
    return pw_run(a, PW_DGRAD, A != nullptr, st);
}

extern "C" int cfn_pwconv_bwd_data(const float* gy, const float* y, const double* gsum, const double* gsumsq,
                                   const float* w, const float* x, const double* A, const double* B, int act, float* gx,
                                   double* gA, double* gB, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride,
                                   void* stream) {
    return cfn_pwconv_bwd_data_acc(gy, y, gsum, gsumsq, w, x, A, B, act, gx, gA, gB, N, Cin, Cout, T, Hi, Wi, stride, nullptr, 1, nullptr, stream);
}

static void wg_plan(WgArgs& a, int& MTW, int& NTW) {
    // tile shape: rows <= 64, cols <= 64 (register footprint of the prefetch + accumulators: 2 waves / SIMD)
    const int M32 = cfn_cdiv(a.M, 32), K32 = cfn_cdiv(a.K, 32);
    MTW = cfn_cdiv(M32, cfn_cdiv(M32, 2));
    NTW = cfn_cdiv(K32, cfn_cdiv(K32, 2));
    a.mtiles = cfn_cdiv(a.M, 32 * MTW);
    a.ktiles = cfn_cdiv(a.K, 32 * NTW);
    // ~2.5 workgroups per CU over (samples x tiles x position strips)
    const long nst = cfn_cdiv(a.Q, WG_PT);
    long want = 640 / ((long)a.N * a.mtiles * a.ktiles);
    if (want < 1) want = 1;
    int stages = cfn_cdiv(nst, want);
    if (stages < 4) stages = 4;
    a.stages = stages;
    a.nstrips = cfn_cdiv(nst, stages);
}

static unsigned wg_blocks(const WgArgs& a) { return (unsigned)((long)a.N * a.nstrips * a.mtiles * a.ktiles); }
static size_t wg_lds(int MTW, int NTW) {
    size_t lds = ((size_t)2 * (32 * MTW + 32 * NTW) * WG_PITCH + 2 * (32 * MTW + 32 * NTW) + 32 * MTW) * sizeof(float);
    const size_t lds_cw = (size_t)4 * 32 * MTW * (32 * NTW + 1) * sizeof(float);
    return lds_cw > lds ? lds_cw : lds;
}

static int wg_launch(const WgArgs& a, int MTW, int NTW, hipStream_t st) {
    const unsigned blocks = wg_blocks(a);
    const size_t lds = wg_lds(MTW, NTW);
#define CFN_WG_GO(MW, NW) cfn_launch(pw_wgrad_kernel<MW, NW>, blocks, 256, lds, st, a)
    if (MTW == 1 && NTW == 1) CFN_WG_GO(1, 1);
    else if (MTW == 1) CFN_WG_GO(1, 2);
    else if (NTW == 1) CFN_WG_GO(2, 1);
    else CFN_WG_GO(2, 2);
#undef CFN_WG_GO
    return cfn_check_launch("pwconv_bwd_weight");
}

static void wg_geom(WgArgs& a, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride) {
    a.N = N; a.M = Cout; a.K = Cin; a.Hi = Hi; a.Wi = Wi; a.stride = stride;
    a.Ho = (Hi - 1) / stride + 1; a.Wo = (Wi - 1) / stride + 1;
    a.Pin = T * Hi * Wi; a.Q = T * a.Ho * a.Wo;
}

extern "C" int cfn_pwconv_bwd_weight(const float* gy, const float* y, const double* gsum, const double* gsumsq,
                                     const float* x, const double* A, const double* B, int act, double* gw, int N,
                                     int Cin, int Cout, int T, int Hi, int Wi, int stride, const double* gscale, void* stream) {
    CFN_REQUIRE(gy && x && gw, "cfn_pwconv_bwd_weight: null tensor");
    CFN_REQUIRE(stride == 1 || stride == 2, "cfn_pwconv_bwd_weight: stride must be 1 or 2");
    CFN_REQUIRE((A == nullptr) == (B == nullptr), "cfn_pwconv_bwd_weight: A/B mismatch");
    CFN_REQUIRE(gsumsq == nullptr || y != nullptr, "cfn_pwconv_bwd_weight: gsumsq needs y");
    WgArgs a = {};
    a.gy = gy; a.y = gsumsq ? y : nullptr; a.gs = gsum; a.gq = gsumsq; a.gsc = gscale; a.x = x; a.pa = A; a.pb = B; a.act = act;
    a.gw = gw;
    wg_geom(a, N, Cin, Cout, T, Hi, Wi, stride);
    PwBwdShape s = {N, Cin, Cout, T, Hi, Wi, stride, act};
    s.pro = A != nullptr; s.two = a.y != nullptr;
    s.align_g = (unsigned)(((uintptr_t)gy | (uintptr_t)(a.y ? a.y : gy)) & 15); s.align_x = (unsigned)((uintptr_t)x & 15);
    PwBwdPlan p = {};
    if (!pw_route_wgrad(s, pw_switches_now(true), p, 0)) return cfn_fail(CFN_ERR_UNSUPPORTED, "cfn_pwconv_bwd_weight: no kernel for this shape");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_PWCONV_WGRAD, st, 4.0 * N * ((double)Cout * a.Q * (a.y ? 2 : 1) + (double)Cin * a.Q));
    if (p.family == PW_FAM_PSS) return pws_wgrad_launch(p, gy, a.y, gsum, gsumsq, gscale, x, A, B, act, gw, N, Cout, Cin, a.Q, st);
    if (p.family == PW_FAM_WD) return pwd_wgrad_launch(p, gy, a.y, gsum, gsumsq, gscale, x, A, B, act, gw, N, Cout, Cin, T, Hi, Wi, stride, st);
    int MTW, NTW;
    wg_plan(a, MTW, NTW);
    return wg_launch(a, MTW, NTW, st);
}

// the LDS-staged fp32 weight gradient takes every shape.  t[] = row / column tiles
bool pw_wg_plan(const PwBwdShape& s, const PwSwitches&, PwBwdPlan& p) {
    WgArgs a = {};
    wg_geom(a, s.N, s.Cin, s.Cout, s.T, s.Hi, s.Wi, s.stride);
    wg_plan(a, p.t[0], p.t[1]);
    p.family = PW_FAM_WG; p.stages = a.stages; p.nstrips = a.nstrips; p.threads = 256;
    p.blocks = wg_blocks(a); p.lds = wg_lds(p.t[0], p.t[1]);
    return true;
}

// ---------------------------------------------------------------------------------------------
// Dense 3-D convolution as an implicit GEMM on the same MFMA kernels (no im2col buffer in HBM): the X3D stem
// conv1_s (1x3x3, stride (1,2,2), pad (0,1,1), x3d_fine.py:210-215) and the Grid Pool saliency convolutions
// (3x3x3 stride 2 and 1x3x3 stride (1,2,2), x3d_coarse.py:362-366).  geom = {kT,kH,kW,sT,sH,sW,pT,pH,pW}.
// ---------------------------------------------------------------------------------------------
template <typename ARGS>
static int dense_geom(ARGS& a, int Cimg, int T, int Hi, int Wi, const int* g) {
    a.stem = 1; a.Cimg = Cimg;
    a.kT = g[0]; a.kH = g[1]; a.kW = g[2]; a.sT = g[3]; a.sH = g[4]; a.sW = g[5]; a.pT = g[6]; a.pH = g[7]; a.pW = g[8];
    if (a.kT < 1 || a.kH < 1 || a.kW < 1 || a.kT > 7 || a.kH > 7 || a.kW > 7 || a.sT < 1 || a.sH < 1 || a.sW < 1)
        return cfn_fail(CFN_ERR_ARG, "conv3d_dense: unsupported kernel / stride");
    a.Ti = T; a.Hi = Hi; a.Wi = Wi; a.stride = 1;
    a.To = (T + 2 * a.pT - a.kT) / a.sT + 1;
    a.Ho = (Hi + 2 * a.pH - a.kH) / a.sH + 1;
    a.Wo = (Wi + 2 * a.pW - a.kW) / a.sW + 1;
    if (a.To < 1 || a.Ho < 1 || a.Wo < 1) return cfn_fail(CFN_ERR_ARG, "conv3d_dense: empty output");
    a.Pin = T * Hi * Wi; a.Q = a.To * a.Ho * a.Wo;
    if ((long)Cimg * a.Pin >= (1L << 31)) return cfn_fail(CFN_ERR_UNSUPPORTED, "conv3d_dense: sample too large for 32-bit offsets");
    return CFN_OK;
}

// The implicit-GEMM forward of a dense conv: tile plan (pw_plan patches `a`) and template choice.  v = {MT, mode, STATS, ACT}; false: beyond the
// descriptor range
static bool dense_gemm_pick(PwArgs& a, bool stats, DensePlan& p) {
    p = DensePlan{};
    if (!pw_plan(a, p.v[0], p.grid[0], p.lds)) return false;
    p.family = DN_GEMM; p.v[1] = PW_FWD; p.v[2] = stats; p.v[3] = a.act == CFN_ACT_RELU ? CFN_ACT_RELU : CFN_ACT_NONE;
    p.grid[1] = p.grid[2] = 1; p.wg = 256;
    return true;
}

// The LDS-staged weight gradient of a dense conv: every shape.  v = {MTW, NTW}
static void dense_wg_pick(WgArgs& a, DensePlan& p) {
    p = DensePlan{};
    wg_plan(a, p.v[0], p.v[1]);
    p.family = DN_WG; p.grid[0] = wg_blocks(a); p.grid[1] = p.grid[2] = 1; p.wg = 256; p.lds = wg_lds(p.v[0], p.v[1]);
}

extern "C" int cfn_conv3d_dense_fwd(const float* x, const double* A, const double* B, int act, const float* w, float* y,
                                    double* sum, double* sumsq, int N, int Cin, int Cout, int T, int Hi, int Wi,
                                    const int* geom, void* stream) {
    CFN_REQUIRE(x && w && y && geom, "cfn_conv3d_dense_fwd: null tensor");
    CFN_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_conv3d_dense_fwd: bad shape");
    CFN_REQUIRE((A == nullptr) == (B == nullptr), "cfn_conv3d_dense_fwd: A/B mismatch");
    CFN_REQUIRE((sum == nullptr) == (sumsq == nullptr), "cfn_conv3d_dense_fwd: sum/sumsq mismatch");
    CFN_REQUIRE(act == CFN_ACT_NONE || act == CFN_ACT_RELU, "cfn_conv3d_dense_fwd: prologue act must be none or relu");
    PwArgs a = {};
    a.src = x; a.pa = A; a.pb = B; a.act = act; a.w = w; a.dst = y; a.s1 = sum; a.s2 = sumsq;
    int rc = dense_geom(a, Cin, T, Hi, Wi, geom);
    if (rc) return rc;
    a.N = N; a.M = Cout; a.K = Cin * a.kT * a.kH * a.kW; a.Cin = a.K;
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_DENSE_FWD, st, 4.0 * N * ((double)Cin * a.Pin + (double)Cout * a.Q));
    {   // Grid Pool saliency shapes (24 channels, 3x3x3 stride 2, 56 / 28 wide planes): the split-bf16 kernel of salconvb.hip (round 6), then the
        // exact-fp32 LDS-tiled kernel of salconv.hip
        const int rb = salb_fwd_try_launch(x, A, B, act, w, y, sum, sumsq, N, Cin, Cout, T, Hi, Wi, geom, st);
        if (rb >= 0) return rb;
        const int rs = sal_fwd_try_launch(x, A, B, act, w, y, sum, sumsq, N, Cin, Cout, T, Hi, Wi, geom, st);
        if (rs >= 0) return rs;
    }
    DensePlan p;
    if (!dense_gemm_pick(a, sum != nullptr, p)) return pw_too_large(a);
    const int MT = p.v[0];
    const unsigned blocks = p.grid[0];
    const size_t lds = p.lds;
    if (p.v[2]) {
        if (p.v[3] == CFN_ACT_RELU) return pw_launch_mt<PW_FWD, true, CFN_ACT_RELU, true>(a, MT, blocks, lds, st);
        return pw_launch_mt<PW_FWD, true, CFN_ACT_NONE, true>(a, MT, blocks, lds, st);
    }
    if (p.v[3] == CFN_ACT_RELU) return pw_launch_mt<PW_FWD, false, CFN_ACT_RELU, true>(a, MT, blocks, lds, st);
    return pw_launch_mt<PW_FWD, false, CFN_ACT_NONE, true>(a, MT, blocks, lds, st);
}

extern "C" int cfn_conv3d_dense_bwd_weight(const float* gy, const float* y, const double* gsum, const double* gsumsq,
                                           const float* x, const double* A, const double* B, int act, double* gw, int N,
                                           int Cin, int Cout, int T, int Hi, int Wi, const int* geom, void* stream) {
    CFN_REQUIRE(gy && x && gw && geom, "cfn_conv3d_dense_bwd_weight: null tensor");
    CFN_REQUIRE((A == nullptr) == (B == nullptr), "cfn_conv3d_dense_bwd_weight: A/B mismatch");
    CFN_REQUIRE(gsumsq == nullptr || y != nullptr, "cfn_conv3d_dense_bwd_weight: gsumsq needs y");
    WgArgs a = {};
    a.gy = gy; a.y = gsumsq ? y : nullptr; a.gs = gsum; a.gq = gsumsq; a.x = x; a.pa = A; a.pb = B; a.act = act; a.gw = gw;
    int rc = dense_geom(a, Cin, T, Hi, Wi, geom);
    if (rc) return rc;
    a.N = N; a.M = Cout; a.K = Cin * a.kT * a.kH * a.kW;
    DensePlan pg;
    dense_wg_pick(a, pg);
    const int MTW = pg.v[0], NTW = pg.v[1];
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, 4.0 * N * ((double)Cin * a.Pin + (double)Cout * a.Q));
    {   // LDS-tiled persistent kernel (salconv.hip) for the Grid Pool saliency shapes
        const int rs = sal_wgrad_try_launch(gy, a.y, gsum, gsumsq, x, A, B, act, gw, N, Cin, Cout, T, Hi, Wi, geom, st);
        if (rs >= 0) return rs;
    }
    {
        const int rd = pwd_wgrad_try_dense(gy, a.y, gsum, gsumsq, x, A, B, act, gw, N, Cout, Cin, T, Hi, Wi, geom, st);
        if (rd >= 0) return rd;
    }
    return wg_launch(a, MTW, NTW, st);
}

extern "C" int cfn_stem_conv_fwd(const float* x, const float* w, float* y, int N, int Cimg, int Cout, int T, int Hi, int Wi,
                                 void* stream) {
    CFN_REQUIRE(x && w && y, "cfn_stem_conv_fwd: null tensor");
    CFN_REQUIRE(N > 0 && Cimg > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_stem_conv_fwd: bad shape");
    {   // LDS-tiled kernel (stem.hip) for the X3D shape family; anything else runs as an implicit GEMM
        const int rc = stem_fwd_try_launch(x, w, y, N, Cimg, Cout, T, Hi, Wi, (hipStream_t)stream);
        if (rc >= 0) return rc;
    }
    return cfn_conv3d_dense_fwd(x, nullptr, nullptr, CFN_ACT_NONE, w, y, nullptr, nullptr, N, Cimg, Cout, T, Hi, Wi, kStemGeom, stream);
}

extern "C" int cfn_stem_conv_bwd_weight(const float* gy, const float* x, double* gw, int N, int Cimg, int Cout, int T,
                                        int Hi, int Wi, void* stream) {
    CFN_REQUIRE(gy && x && gw, "cfn_stem_conv_bwd_weight: null tensor");
    CFN_REQUIRE(N > 0 && Cimg > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_stem_conv_bwd_weight: bad shape");
    {   // LDS-staged persistent MFMA kernel (stem.hip) for the 224x224 clip; anything else runs as an implicit GEMM
        hipStream_t st = (hipStream_t)stream;
        if (stem_wgrad_try_launch(gy, x, gw, N, Cimg, Cout, T, Hi, Wi, st, true) == 0) {
            CfnProfScope prof(CFN_K_STEM, st, 4.0 * N * T * ((double)Cimg * Hi * Wi + (double)Cout * (Hi / 2) * (Wi / 2)));
            return stem_wgrad_try_launch(gy, x, gw, N, Cimg, Cout, T, Hi, Wi, st, false);
        }
    }
    return cfn_conv3d_dense_bwd_weight(gy, nullptr, nullptr, nullptr, x, nullptr, nullptr, CFN_ACT_NONE, gw, N, Cimg, Cout, T, Hi, Wi,
                                       kStemGeom, stream);
}

// ---- the same arithmetic for the host-only query (cfn_conv3d_dense_route, denseroute.hip) ----
// the implicit-GEMM forward of a dense conv.  v = {MT, mode, STATS, ACT}; false: beyond the descriptor range (the entry point fails)
bool dense_gemm_plan(const DenseShape& s, DensePlan& p) {
    PwArgs a = {};
    a.act = s.act;
    if (dense_geom(a, s.Cin, s.T, s.Hi, s.Wi, s.g)) return false;
    a.N = s.N; a.M = s.Cout; a.K = s.Cin * a.kT * a.kH * a.kW; a.Cin = a.K;
    return dense_gemm_pick(a, s.stats, p);
}

// the LDS-staged weight gradient of a dense conv: every shape.  v = {MTW, NTW}
bool dense_wg_plan(const DenseShape& s, DensePlan& p) {
    WgArgs a = {};
    if (dense_geom(a, s.Cin, s.T, s.Hi, s.Wi, s.g)) return false;
    a.N = s.N; a.M = s.Cout; a.K = s.Cin * a.kT * a.kH * a.kW;
    dense_wg_pick(a, p);
    return true;
}
