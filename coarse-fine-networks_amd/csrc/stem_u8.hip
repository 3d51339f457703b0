// uint8 video frames in, normalised on the GPU (the reference normalises on the CPU: ToTensor + Normalize per frame,
// spatial_transforms.py:46-85,108-118, stack + permute per clip, charades_fine.py:170-173).
//
// frames (N, T, H, W, 3) uint8, channels last, as the decoder and the crop / flip transforms leave them.  The normalised value of a
// byte is LOOKED UP in a (3, 256) fp32 table the host built with the reference's own operations (ops.clip_lut): the converted clip
// is then bit-identical to the reference's, which a multiply-add form is not.  lengths (N) int32 or NULL: frame t >= lengths[n] of
// sample n is zero padding (collate pads AFTER normalisation, and no byte normalises to 0.0) -- it reads as 0.0 in all channels.
//
//   cfn_clip_u8_to_f32           frames -> (N, 3, T, H, W) fp32: any shape; the fallback in front of the fp32 stem kernels
//   cfn_stem_conv_u8_fwd         twin of stem_fwd_kernel   (stem.hip): the band of input rows is ONE contiguous run of bytes
//   cfn_stem_conv_u8_bwd_weight  twin of stem_wgrad_kernel (stem.hip)
// The twins decode while they stage and build the SAME fp32 LDS image as the fp32 kernels; operand reads, MFMA order, epilogue and
// fp64 commits are those of stem.hip, so the forward output is bit-identical to cfn_stem_conv_fwd on the converted clip.
// A thread stages 4 pixels = 12 consecutive bytes (3 dwords, dword aligned for every W % 4 == 0) and writes one float4 per channel.
#include "cfn_common.h"
#include <stdlib.h>

typedef float __attribute__((ext_vector_type(16))) st16;
typedef float __attribute__((ext_vector_type(4))) st4;
typedef float __attribute__((ext_vector_type(2))) st2;
typedef unsigned __attribute__((ext_vector_type(4))) su4;

#define U8_LUT 768                                                        // 3 x 256 floats = 3 KB of LDS

// byte k (0..11) of 12 interleaved bytes held in three little-endian dwords: pixel k / 3, channel k % 3
__device__ __forceinline__ unsigned u8_byte(unsigned d0, unsigned d1, unsigned d2, int k) {
    const unsigned d = (k >> 2) == 0 ? d0 : ((k >> 2) == 1 ? d1 : d2);
    return (d >> (8 * (k & 3))) & 255u;
}
// 4 pixels of channel ci through the LDS table
__device__ __forceinline__ st4 u8_decode(const float* lut, unsigned d0, unsigned d1, unsigned d2, int ci) {
    st4 v;
    v.x = lut[ci * 256 + u8_byte(d0, d1, d2, ci)];
    v.y = lut[ci * 256 + u8_byte(d0, d1, d2, 3 + ci)];
    v.z = lut[ci * 256 + u8_byte(d0, d1, d2, 6 + ci)];
    v.w = lut[ci * 256 + u8_byte(d0, d1, d2, 9 + ci)];
    return v;
}

// ---- frames -> fp32 clip ------------------------------------------------------------------------------------------------------------
// One workgroup = 1024 consecutive pixels of one frame (P = H * W pixels = 3 P contiguous bytes in, three runs of P floats out).
// The 3072 bytes go to LDS as they are (LV-byte loads: 16 when P % 16 == 0, 4 when P % 4 == 0, else 1), then thread q takes
// pixels 4q .. 4q + 3 back out of LDS (3 dwords, lane stride 3 dwords: conflict free) and stores one float4 per plane: every
// store instruction of a wave writes 1 KB of one plane.  P % 4 != 0: scalar stores with a bound per pixel.
struct ClipU8Args {
    const unsigned char* f; const float* lut; const int* len; float* x;
    int T, P, tiles;
};

template <int LV>
__global__ __launch_bounds__(256) void clip_u8_kernel(const ClipU8Args a) {
    __shared__ __attribute__((aligned(16))) unsigned raw[768];
    __shared__ float lut[U8_LUT];
    const int tid = threadIdx.x;
    unsigned L = blockIdx.x;
    const int tile = L % a.tiles; L /= a.tiles;
    const int t = L % a.T, n = L / a.T;
    const int P = a.P, p0 = tile * 1024, np = min(1024, P - p0);          // pixels of this tile
    const bool live = !a.len || t < a.len[n];
    const long xb = ((long)n * 3 * a.T + t) * P + p0;                       // channel ci: + ci * T * P
    const long cs = (long)a.T * P;
    if (live) {
        const unsigned char* src = a.f + ((long)n * a.T + t) * 3 * P + (long)p0 * 3;
        const int nb = 3 * np;
        if (LV == 16) {
            if (tid * 16 < nb) reinterpret_cast<su4*>(raw)[tid] = *reinterpret_cast<const su4*>(src + tid * 16);
        } else if (LV == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if ((tid + k * 256) * 4 < nb) raw[tid + k * 256] = *reinterpret_cast<const unsigned*>(src + (tid + k * 256) * 4);
        } else {
            unsigned char* rb = reinterpret_cast<unsigned char*>(raw);
            for (int i = tid; i < nb; i += 256) rb[i] = src[i];
            for (int i = nb + tid; i < ((nb + 11) / 12) * 12; i += 256) rb[i] = 0;      // the last thread's unit is decoded whole: no unwritten byte
        }
        for (int i = tid; i < U8_LUT; i += 256) lut[i] = a.lut[i];
    }
    __syncthreads();
    const int q = tid * 4;
    if (q >= np) return;
    st4 v[3];
    if (live) {
        const unsigned d0 = raw[3 * tid], d1 = raw[3 * tid + 1], d2 = raw[3 * tid + 2];   // (P % 4 != 0: the bytes behind 3 * np were zeroed, their values are dropped below)
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) v[ci] = u8_decode(lut, d0, d1, d2, ci);
    } else {
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) v[ci] = (st4){0.f, 0.f, 0.f, 0.f};
    }
    if (LV >= 4) {                                                          // P % 4 == 0: whole float4s, 16-byte aligned
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) *reinterpret_cast<st4*>(a.x + xb + ci * cs + q) = v[ci];
    } else {
#pragma unroll
        for (int ci = 0; ci < 3; ++ci)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (q + j < np) a.x[xb + ci * cs + q + j] = v[ci][j];
    }
}

extern "C" int cfn_clip_u8_to_f32(const unsigned char* frames, const float* lut, const int* lengths, float* x, int N, int T, int H,
                                  int W, void* stream) {
    CFN_REQUIRE(frames && lut && x, "cfn_clip_u8_to_f32: null tensor");
    CFN_REQUIRE(N > 0 && T > 0 && H > 0 && W > 0, "cfn_clip_u8_to_f32: bad shape");
    const long P = (long)H * W;
    CFN_REQUIRE(P < (1L << 28), "cfn_clip_u8_to_f32: frame too large");
    ClipU8Args a = {frames, lut, lengths, x, T, (int)P, cfn_cdiv(P, 1024)};
    const long blocks = (long)N * T * a.tiles;
    CFN_REQUIRE(blocks < (1L << 31), "cfn_clip_u8_to_f32: clip too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, (double)N * T * P * 3 * (1.0 + 4.0));
    const bool al16 = !(((uintptr_t)frames | (uintptr_t)x) & 15), al4 = !((uintptr_t)frames & 3) && !((uintptr_t)x & 15);
    if (P % 16 == 0 && al16) hipLaunchKernelGGL(clip_u8_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else if (P % 4 == 0 && al4) hipLaunchKernelGGL(clip_u8_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(clip_u8_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return cfn_check_launch("clip_u8_to_f32");
}

// ---- conv1_s forward on uint8 frames (twin of stem_fwd_kernel<3>) --------------------------------------------------------------------
struct StemU8Args {
    const unsigned char* f; const float* lut; const int* len; const float* w; float* y;
    int N, Cout, T, Hi, Wi, Ho, Wo, RB, RIN, WPAD, bands;
};

__global__ __launch_bounds__(256) void stem_u8_fwd_kernel(const StemU8Args a) {
    extern __shared__ __attribute__((aligned(16))) float img[];      // [3][RIN][WPAD], data at column 4, left halo at 3; then the table
    constexpr int CI = 3, KP = (CI * 9 + 1) / 2;                      // k-pairs
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    unsigned L = cfn_xcd_remap(blockIdx.x, gridDim.x);
    const int band = L % a.bands; L /= a.bands;
    const int t = L % a.T;
    const int n = L / a.T;
    const int RIN = a.RIN, WPAD = a.WPAD, Wi = a.Wi, Hi = a.Hi, Wo = a.Wo, Ho = a.Ho;
    const int oh0 = band * a.RB, ih0 = 2 * oh0 - 1;
    float* lut = img + CI * RIN * WPAD;
    const bool live = !a.len || t < a.len[n];                          // a padded frame: a zero image, nothing is loaded

    // ---- stage the band: RIN rows of Wi pixels x 3 bytes, 12 bytes (4 pixels) per thread, rows outside the image are zero ----
    const int w4 = Wi >> 2, per_row = w4 + 1;                         // + one slot that carries the left halo
    const int total = RIN * per_row, chs = RIN * WPAD;
    const unsigned char* fr = a.f + ((long)n * a.T + t) * (long)Hi * Wi * 3;
    if (live)
        for (int i = tid; i < U8_LUT; i += 256) lut[i] = a.lut[i];
    // (all loads of a batch are issued before the table is waited for and before the first LDS write)
    for (int b0 = 0; b0 < total; b0 += 256 * 4) {
        unsigned d[4][3];
        bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = b0 + tid + u * 256;
            const int r = e / per_row, c4 = e - r * per_row;
            const int ih = ih0 + r;
            in[u] = live && e < total && c4 > 0 && ih >= 0 && ih < Hi;
            d[u][0] = d[u][1] = d[u][2] = 0u;
            if (in[u]) {
                const unsigned* p = reinterpret_cast<const unsigned*>(fr + ((long)ih * Wi + (c4 - 1) * 4) * 3);
                d[u][0] = p[0]; d[u][1] = p[1]; d[u][2] = p[2];
            }
        }
        if (b0 == 0) __syncthreads();                                  // the table is in LDS
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = b0 + tid + u * 256;
            const int r = e / per_row, c4 = e - r * per_row;
            if (e < total) {
#pragma unroll
                for (int ci = 0; ci < CI; ++ci)                         // c4 == 0: columns 0..3 (3 = halo of iw = -1) zero
                    *reinterpret_cast<st4*>(img + ci * chs + r * WPAD + c4 * 4) =
                        in[u] ? u8_decode(lut, d[u][0], d[u][1], d[u][2], ci) : (st4){0.f, 0.f, 0.f, 0.f};
            }
        }
    }
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

// -1 = shape not handled: the caller converts (cfn_clip_u8_to_f32) and runs cfn_stem_conv_fwd
extern "C" int cfn_stem_conv_u8_fwd(const unsigned char* frames, const float* lut, const int* lengths, const float* w, float* y, int N,
                                    int Cimg, int Cout, int T, int Hi, int Wi, void* stream) {
    CFN_REQUIRE(frames && lut && w && y, "cfn_stem_conv_u8_fwd: null tensor");
    CFN_REQUIRE(N > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_stem_conv_u8_fwd: bad shape");
    CFN_REQUIRE(Cimg == 3, "cfn_stem_conv_u8_fwd: uint8 frames have 3 interleaved channels, got Cimg = %d", Cimg);
    if (Cout > 32 || (Wi & 3) || (Hi & 1) || ((uintptr_t)frames & 3)) return -1;
    StemU8Args a = {frames, lut, lengths, w, y, N, Cout, T, Hi, Wi, Hi / 2, Wi / 2};
    a.RB = (a.Ho % 8 == 0) ? 8 : 4;
    a.RIN = 2 * a.RB + 1;
    a.WPAD = Wi + 8;
    a.bands = cfn_cdiv(a.Ho, a.RB);
    const size_t lds = ((size_t)3 * a.RIN * a.WPAD + U8_LUT) * sizeof(float);
    if (lds > 64 * 1024) return -1;
    const long blocks = (long)N * T * a.bands;
    if (blocks >= (1L << 31)) return -1;
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, (double)N * T * (3.0 * Hi * Wi + 4.0 * Cout * a.Ho * a.Wo));
    auto k = stem_u8_fwd_kernel;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), lds, st, a);
    return cfn_check_launch("stem_conv_u8_fwd");
}

// ---- weight gradient of conv1_s at 224x224 on uint8 frames (twin of stem_wgrad_kernel) ------------------------------------------------
// Same persistent walk over (frame, band of 4 output rows) items, same LDS images, same MFMA order and reduction.  The band's 9
// input rows are 9 x 672 contiguous bytes: 504 units of 12 bytes, one per thread (the fp32 kernel: 3 float4 units per thread).
// The bytes of the NEXT item are in flight while the current one is multiplied; they are decoded when they are put into LDS.
// Items of padded frames load nothing and are not multiplied.
struct StemWgU8Args {
    const float* gy; const unsigned char* f; const float* lut; const int* len; double* gw;
    int N, T, items, per_block;
};

__global__ __launch_bounds__(512, 2) void stem_u8_wgrad_kernel(const StemWgU8Args a) {
    constexpr int WI = 224, WO = 112, RB = 4, RIN = 9, PITCH = 228, CIS = RIN * PITCH + 8, GP = 450, W4 = 56, G4 = 28;
    constexpr int P = WI * WI, PO = WO * WO, BANDS = WO / RB, OOB = 0x7fff0000;
    constexpr int XU = RIN * W4;                                           // 12-byte units of the frames per item: 504 <= 512
    constexpr int GU = 24 * RB * G4, NGU = (GU + 511) / 512;               // float4 units of gy per item and thread
    __shared__ __attribute__((aligned(16))) float img[3 * CIS];
    __shared__ __attribute__((aligned(16))) float gbuf[24 * GP];
    __shared__ float lut[U8_LUT];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6), h = lane >> 5, p = lane & 31;
    const int T = a.T;

    for (int i = tid; i < 3 * CIS; i += 512) img[i] = 0.0f;                // the halo column stays zero for good
    for (int i = tid; i < U8_LUT; i += 512) lut[i] = a.lut[i];

    // staging unit of this thread (the same for every item; the item adds a frame / row offset)
    const int xr = tid / W4, xc4 = tid - xr * W4;
    const bool xin = tid < XU;
    const int xo = xin ? (xr * WI + xc4 * 4) * 3 : OOB;
    const int xl = xin ? xr * PITCH + 4 + xc4 * 4 : -1;
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
    unsigned fx0, fx1, fx2;
    bool fxin, flive;                                                       // of the fetched item: this thread's row is inside the image; the frame is not padding
    st4 fg[NGU];
    auto fetch = [&](int item) {
        const bool on = item < last;
        const int band = item % BANDS, ft = item / BANDS;                  // ft = n * T + t
        const int n = ft / T, t = ft - n * T;
        const int ih0 = 2 * band * RB - 1;
        flive = cfn_uni((int)(on && (!a.len || t < a.len[on ? n : 0]))) != 0;
        // (frames: n's T frames of 3 P bytes; gy: n's 24 channels T * PO apart: one descriptor per tensor over the whole sample)
        __amdgpu_buffer_rsrc_t rx = cfn_rsrc(a.f + (long)(on ? n : 0) * T * P * 3, (unsigned)((long)T * P * 3));
        __amdgpu_buffer_rsrc_t rg = cfn_rsrc(a.gy + (long)(on ? n : 0) * 24 * T * PO, (unsigned)((long)24 * T * PO * 4));
        // (the scalar offset is not range checked and must not be negative: the band's first input row, -1 for band 0, goes into the vector offset)
        const int sx = cfn_uni(on ? t * P * 3 : 0), sg = cfn_uni(on ? (t * PO + band * RB * WO) * 4 : 0), rowoff = cfn_uni(ih0 * WI * 3);
        fxin = flive && xin && ih0 + xr >= 0;
        const int vo = fxin ? xo + rowoff : OOB;
        fx0 = __builtin_amdgcn_raw_buffer_load_b32(rx, vo, sx, 0);
        fx1 = __builtin_amdgcn_raw_buffer_load_b32(rx, fxin ? vo + 4 : OOB, sx, 0);
        fx2 = __builtin_amdgcn_raw_buffer_load_b32(rx, fxin ? vo + 8 : OOB, sx, 0);
#pragma unroll
        for (int k = 0; k < NGU; ++k)
            fg[k] = __builtin_bit_cast(st4, __builtin_amdgcn_raw_buffer_load_b128(rg, flive ? go[k] : OOB, sg, 0));
    };
    auto put = [&]() {                                                      // rows above the image and padded frames: zeros
        if (xl >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<st4*>(img + c * CIS + xl) = fxin ? u8_decode(lut, fx0, fx1, fx2, c) : (st4){0.f, 0.f, 0.f, 0.f};
        }
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
        if (live) {
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

// -1 = shape not handled: the caller converts (cfn_clip_u8_to_f32) and runs cfn_stem_conv_bwd_weight
extern "C" int cfn_stem_conv_u8_bwd_weight(const float* gy, const unsigned char* frames, const float* lut, const int* lengths, double* gw,
                                           int N, int Cimg, int Cout, int T, int Hi, int Wi, void* stream) {
    CFN_REQUIRE(gy && frames && lut && gw, "cfn_stem_conv_u8_bwd_weight: null tensor");
    CFN_REQUIRE(N > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_stem_conv_u8_bwd_weight: bad shape");
    CFN_REQUIRE(Cimg == 3, "cfn_stem_conv_u8_bwd_weight: uint8 frames have 3 interleaved channels, got Cimg = %d", Cimg);
    if (Cout != 24 || Hi != 224 || Wi != 224 || ((uintptr_t)gy & 15) || ((uintptr_t)frames & 3)) return -1;
    if ((long)24 * T * 112 * 112 * 4 >= 0x7fff0000L) return -1;
    const long items = (long)N * T * 28;
    if (items >= (1L << 30)) return -1;
    hipStream_t st = (hipStream_t)stream;
    static int cus = 0;
    if (!cus) { int dev = 0; hipDeviceProp_t pr; cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) ? pr.multiProcessorCount : 256; }
    long blocks = (long)cus * 2;                                           // persistent workgroups per CU, as stem_wgrad_kernel
    if (blocks > items) blocks = items;
    const long per = (items + blocks - 1) / blocks;
    blocks = (items + per - 1) / per;
    CfnProfScope prof(CFN_K_STEM, st, (double)N * T * (3.0 * Hi * Wi + 4.0 * Cout * (Hi / 2) * (Wi / 2)));
    StemWgU8Args a = {gy, frames, lut, lengths, gw, N, T, (int)items, (int)per};
    hipLaunchKernelGGL(stem_u8_wgrad_kernel, dim3((unsigned)blocks), dim3(512), 0, st, a);
    return cfn_check_launch("stem_conv_u8_wgrad");
}
