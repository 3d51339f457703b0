// The two kernel bodies of the stem conv1_s (x3d_fine.py:210-215): Conv3d(3, 24, (1,3,3), stride (1,2,2), pad (0,1,1), bias=False), forward
// and weight gradient, each written once.  A source policy SRC supplies what depends on the clip's storage: fp32 (N, 3, T, H, W) in stem.hip,
// uint8 (N, T, H, W, 3) frames decoded through a table in stem_u8.hip.  Both sources build the SAME fp32 LDS image; operand reads, MFMA order,
// epilogue and fp64 commits are this file's, so the uint8 forward is bit-identical to the fp32 forward of the converted clip.
#pragma once
#include "dense_plan.h"
#include <stdlib.h>

typedef float __attribute__((ext_vector_type(16))) st16;
typedef float __attribute__((ext_vector_type(4))) st4;
typedef float __attribute__((ext_vector_type(2))) st2;

#define U8_LUT 768                                                        // the uint8 source's table: 3 x 256 floats = 3 KB of LDS

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// HBM bound (one 3-channel frame in, one 24-channel quarter-resolution frame out), but as a gather-form implicit GEMM it
// runs at 2.6 TB/s: every lane fetches its 27 taps from global memory through a tap table.  Here a workgroup stages a band
// of input rows of one frame in LDS once (coalesced rows, zero halo) and the im2col operand of the MFMA comes out of
// LDS:  Y[co][pos] = sum_k W[co][k] * X[k][pos],  k = (ci,kh,kw) -> v_mfma_f32_32x32x2 with the 32 x 28 weight operand
// resident in registers (14 k-pairs), lane <-> output position, so every store instruction writes full 128-byte lines.
// SRC::CI: input channels;  SRC::stage(a, img, n, t, ih0, tid): rows ih0 .. ih0 + RIN - 1 of frame (n, t) -> img, rows outside the image and
// columns 0..3 zero (no barrier behind the last write: the body has one)
template <class SRC, class Args>
__device__ __forceinline__ void stem_fwd_body(const Args& a, float* img) {       // img [CI][RIN][WPAD], data at column 4, left halo at 3
    constexpr int CI = SRC::CI, KP = (CI * 9 + 1) / 2;                 // k-pairs
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    unsigned L = cfn_xcd_remap(blockIdx.x, gridDim.x);
    const int band = L % a.bands; L /= a.bands;
    const int t = L % a.T;
    const int n = L / a.T;
    const int RIN = a.RIN, WPAD = a.WPAD, Wo = a.Wo, Ho = a.Ho;
    const int oh0 = band * a.RB, ih0 = 2 * oh0 - 1;
    SRC::stage(a, img, n, t, ih0, tid);
    // weight operand: lane (co = col, k = 2s + half)
    float wreg[KP];
    int offk[KP];
#pragma unroll
    for (int s = 0; s < KP; ++s) {
        const int k = 2 * s + half;
        const bool kv = k < CI * 9;
        const int ci = k / 9, r9 = k - ci * 9, kh = r9 / 3, kw = r9 - kh * 3;
        wreg[s] = (kv && col < a.Cout) ? a.w[col * (CI * 9) + k] : 0.0f;
        offk[s] = kv ? (ci * RIN + kh) * WPAD + kw : 0;
    }
    __syncthreads();

    const int npos = min(a.RB, Ho - oh0) * Wo;                        // output rows of a band are contiguous in memory
    const long ybase = (((long)n * a.Cout) * a.T + t) * (long)Ho * Wo + (long)oh0 * Wo;
    const long cstride = (long)a.T * Ho * Wo;
    for (int tile = wave; tile * 32 < npos; tile += 4) {
        const int pos = tile * 32 + col;
        const bool valid = pos < npos;
        const int pc = valid ? pos : 0;
        const int ohl = pc / Wo, ow = pc - ohl * Wo;
        const float* lb = img + (2 * ohl) * WPAD + 2 * ow + 3;        // tap (kh, kw) of channel ci: + (ci*RIN + kh)*WPAD + kw
        st16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KP; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wreg[s], lb[offk[s]], acc, 0, 0, 0);
        if (valid) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < a.Cout) a.y[ybase + co * cstride + pos] = acc[r];
            }
        }
    }
}

// ---- weight gradient at 224x224:  gw[co][(ci,kh,kw)] = sum over (n, t, oh, ow) of gy x im2col(x) -----------------------------------------
// HBM bound: gy (24 channels, 112x112) and x (3 channels, 224x224) are read once: 144 KB + 58 KB per frame; the product is ONE 24 x 27 tile
// whose K dimension (the output positions) is as long as the tensors.  The gather-form kernel (pw_wgrad_direct_kernel: every lane fetches
// its im2col operand from global memory) ran at 2.7 TB/s.  Here a persistent workgroup of 8 waves walks a contiguous run of (frame, band of
// 4 output rows) items: the band's 9 input rows x 3 channels and its 24 x 4 rows of gy are staged in LDS by coalesced loads (the
// loads of the NEXT item are in flight while the current one is multiplied), wave w multiplies positions [56 w, 56 w + 56) of the band:
// 28 v_mfma_f32_32x32x2 with A = gy (row co, k = position) and B = x (column (ci, kh, kw), k = position) both ds_read_b32 with immediate
// offsets; fp32 accumulators per wave, reduced through LDS at the end, one fp64 atomic per element and workgroup.
// LDS: x image [3][9][228] (+8 floats per channel: the 27 operand columns then start in 27 different banks), data at column 4, column 3 =
// the zero halo of input column -1; gy image [24][450].
struct StemWg {       // the geometry both sources share
    static constexpr int WI = 224, WO = 112, RB = 4, RIN = 9, PITCH = 228, CIS = RIN * PITCH + 8, GP = 450, W4 = 56, G4 = 28;
    static constexpr int P = WI * WI, PO = WO * WO, BANDS = WO / RB, OOB = 0x7fff0000;
};

// SRC (an object: it keeps the thread's clip staging units and what it fetched), besides StemWg's constants:
//   PAD                          frames may be padding (a lengths array): items of padded frames load nothing and are not multiplied
//   init(a, tid)                 the staging units of this thread (the same for every item) and whatever else the source keeps in LDS
//   live(a, on, n, t)            the item is to be loaded: it exists (on) and its frame is no padding
//   fetch(a, ld, n, t, ih0)      issue the loads of the thread's units of the band's 9 input rows (none where !ld)
//   put(img)                     what was fetched -> the fp32 image; rows above the image and items not loaded: zeros
template <class SRC, class Args>
__device__ __forceinline__ void stem_wgrad_body(const Args& a) {
    constexpr int WO = SRC::WO, RB = SRC::RB, PITCH = SRC::PITCH, CIS = SRC::CIS, GP = SRC::GP, G4 = SRC::G4, PO = SRC::PO, BANDS = SRC::BANDS, OOB = SRC::OOB;
    constexpr int GU = 24 * RB * G4, NGU = (GU + 511) / 512;               // float4 units of gy per item and thread
    __shared__ __attribute__((aligned(16))) float img[3 * CIS];
    __shared__ __attribute__((aligned(16))) float gbuf[24 * GP];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6), h = lane >> 5, p = lane & 31;
    const int T = a.T;

    for (int i = tid; i < 3 * CIS; i += 512) img[i] = 0.0f;                // the halo column stays zero for good
    SRC src;
    src.init(a, tid);
    int go[NGU], gl[NGU];
#pragma unroll
    for (int k = 0; k < NGU; ++k) {
        const int e = k * 512 + tid;
        const int co = e / (RB * G4), rem = e - co * (RB * G4);           // rem = row * 28 + c4: the band's rows are contiguous in memory
        const bool in = e < GU;
        go[k] = in ? (int)(((long)co * T * PO + rem * 4) * 4) : OOB;
        gl[k] = in ? co * GP + rem * 4 : -1;
    }
    // operands of this lane: A row co = p (rows 24-31 repeat row 23 and are dropped), B column (ci, kh, kw) = p (columns 27-31 repeat column 0)
    const int ohl = wave >> 1, ow0 = (wave & 1) * 56;
    const int colp = p < 27 ? p : 0;
    const int ci = colp / 9, kh = (colp - ci * 9) / 3, kw = colp - ci * 9 - kh * 3;
    const float* bp = img + ci * CIS + (2 * ohl + kh) * PITCH + 2 * ow0 + kw + 3 + 2 * h;
    const float* ap = gbuf + min(p, 23) * GP + ohl * WO + ow0 + h;

    st16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;

    const int first = blockIdx.x * a.per_block, last = min(first + a.per_block, a.items);
    bool flive;                                                             // of the fetched item
    st4 fg[NGU];
    auto fetch = [&](int item) {
        const bool on = item < last;
        const int band = item % BANDS, ft = item / BANDS;                  // ft = n * T + t
        const int nn = ft / T, t = ft - nn * T;
        const int n = (SRC::PAD && !on) ? 0 : nn;                           // (behind the last item: lengths[n] is read, n stays inside)
        const int ih0 = 2 * band * RB - 1;
        flive = src.live(a, on, n, t);
        src.fetch(a, flive, n, t, ih0);
        // (gy: n's 24 channels T * PO apart: one descriptor over the whole sample)
        __amdgpu_buffer_rsrc_t rg = cfn_rsrc(a.gy + (long)n * 24 * T * PO, (unsigned)((long)24 * T * PO * 4));
        // (the scalar offset is not range checked and must not be negative)
        const int sg = cfn_uni(on ? (t * PO + band * RB * WO) * 4 : 0);
#pragma unroll
        for (int k = 0; k < NGU; ++k)
            fg[k] = __builtin_bit_cast(st4, __builtin_amdgcn_raw_buffer_load_b128(rg, flive ? go[k] : OOB, sg, 0));
    };
    auto put = [&]() {
        src.put(img);
#pragma unroll
        for (int k = 0; k < NGU; ++k)
            if (gl[k] >= 0) {
                *reinterpret_cast<st2*>(gbuf + gl[k]) = (st2){fg[k].x, fg[k].y};
                *reinterpret_cast<st2*>(gbuf + gl[k] + 2) = (st2){fg[k].z, fg[k].w};
            }
    };
    __syncthreads();
    fetch(first);
    put();
    bool live = flive;
    __syncthreads();
    for (int item = first; item < last; ++item) {
        fetch(item + 1);                                                    // in flight while this item is multiplied
        if (!SRC::PAD || live) {
#pragma unroll
            for (int j = 0; j < 28; j += 2) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j], bp[4 * j], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j + 2], bp[4 * j + 4], acc1, 0, 0, 0);
            }
        }
        __syncthreads();
        put();
        live = flive;
        __syncthreads();
    }
    // reduce the 8 waves' tiles through LDS (the gy image is free now: 8 x 16 x 64 floats = 32 KB of its 43 KB)
#pragma unroll
    for (int r = 0; r < 16; ++r) gbuf[(wave * 16 + r) * 64 + lane] = acc0[r] + acc1[r];
    __syncthreads();
    for (int e = tid; e < 16 * 64; e += 512) {
        const int r = e >> 6, l = e & 63, hh = l >> 5, col = l & 31;
        const int co = (r & 3) + 8 * (r >> 2) + 4 * hh;
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) s += gbuf[(w * 16 + r) * 64 + l];
        if (co < 24 && col < 27) cfn_add64(&a.gw[co * 27 + col], (double)s);
    }
}
