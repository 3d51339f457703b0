// uint8 video frames in, normalised on the GPU (the reference normalises on the CPU: ToTensor + Normalize per frame,
// spatial_transforms.py:46-85,108-118, stack + permute per clip, charades_fine.py:170-173).
//
// frames (N, T, H, W, 3) uint8, channels last, as the decoder and the crop / flip transforms leave them.  The normalised value of a
// byte is LOOKED UP in a (3, 256) fp32 table the host built with the reference's own operations (ops.clip_lut): the converted clip
// is then bit-identical to the reference's, which a multiply-add form is not.  lengths (N) int32 or NULL: frame t >= lengths[n] of
// sample n is zero padding (collate pads AFTER normalisation, and no byte normalises to 0.0) -- it reads as 0.0 in all channels.
//
//   cfn_clip_u8_to_f32           frames -> (N, 3, T, H, W) fp32: any shape; the fallback in front of the fp32 stem kernels
//   cfn_stem_conv_u8_fwd         stem_fwd_body   (stem_kernel.h) on the uint8 source: the band of input rows is ONE contiguous run of bytes
//   cfn_stem_conv_u8_bwd_weight  stem_wgrad_body (stem_kernel.h) on the uint8 source
// The uint8 source decodes while it stages and builds the SAME fp32 LDS image as the fp32 source (stem.hip); everything behind the image is
// the one body both share, so the forward output is bit-identical to cfn_stem_conv_fwd on the converted clip.  Which shapes the kernels
// take is decided by stem_fwd_plan / stem_wgrad_plan (stem.hip) for both sources.
// A thread stages 4 pixels = 12 consecutive bytes (3 dwords, dword aligned for every W % 4 == 0) and writes one float4 per channel.
#include "stem_kernel.h"

typedef unsigned __attribute__((ext_vector_type(4))) su4;

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

// ---- conv1_s forward on uint8 frames ---------------------------------------------------------------------------------------------------
struct StemU8Args {
    const unsigned char* f; const float* lut; const int* len; const float* w; float* y;
    int N, Cout, T, Hi, Wi, Ho, Wo, RB, RIN, WPAD, bands;
};

struct StemU8 {
    static constexpr int CI = 3;
    // RIN rows of Wi pixels x 3 bytes, 12 bytes (4 pixels) per thread; the table sits in LDS behind the image
    static __device__ __forceinline__ void stage(const StemU8Args& a, float* img, int n, int t, int ih0, int tid) {
        const int RIN = a.RIN, WPAD = a.WPAD, Wi = a.Wi, Hi = a.Hi;
        float* lut = img + CI * RIN * WPAD;
        const bool live = !a.len || t < a.len[n];                          // a padded frame: a zero image, nothing is loaded
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
    }
};

__global__ __launch_bounds__(256) void stem_u8_fwd_kernel(const StemU8Args a) {
    extern __shared__ __attribute__((aligned(16))) float img[];
    stem_fwd_body<StemU8>(a, img);
}

// -1 = shape not handled: the caller converts (cfn_clip_u8_to_f32) and runs cfn_stem_conv_fwd
extern "C" int cfn_stem_conv_u8_fwd(const unsigned char* frames, const float* lut, const int* lengths, const float* w, float* y, int N,
                                    int Cimg, int Cout, int T, int Hi, int Wi, void* stream) {
    CFN_REQUIRE(frames && lut && w && y, "cfn_stem_conv_u8_fwd: null tensor");
    CFN_REQUIRE(N > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_stem_conv_u8_fwd: bad shape");
    CFN_REQUIRE(Cimg == 3, "cfn_stem_conv_u8_fwd: uint8 frames have 3 interleaved channels, got Cimg = %d", Cimg);
    DenseShape s = dense_shape(N, Cimg, Cout, T, Hi, Wi, kStemGeom, CFN_ACT_NONE);
    s.u8 = true; s.align_x = (unsigned)((uintptr_t)frames & 15);
    DensePlan p;
    if (!stem_fwd_plan(s, p)) return -1;
    StemU8Args a = {frames, lut, lengths, w, y, N, Cout, T, Hi, Wi, Hi / 2, Wi / 2, p.chunk, 2 * p.chunk + 1, Wi + 8, p.bands};
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, (double)N * T * (3.0 * Hi * Wi + 4.0 * Cout * a.Ho * a.Wo));
    auto k = stem_u8_fwd_kernel;
    if (p.lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    hipLaunchKernelGGL(k, dim3(p.grid[0]), dim3(256), p.lds, st, a);
    return cfn_check_launch("stem_conv_u8_fwd");
}

// ---- weight gradient of conv1_s at 224x224 on uint8 frames -----------------------------------------------------------------------------
// The band's 9 input rows are 9 x 672 contiguous bytes: 504 units of 12 bytes, one per thread (the fp32 source: 3 float4 units per thread).
// The bytes of the NEXT item are in flight while the current one is multiplied; they are decoded when they are put into LDS.
struct StemWgU8Args {
    const float* gy; const unsigned char* f; const float* lut; const int* len; double* gw;
    int N, T, items, per_block;
};

struct StemWgU8 : StemWg {
    static constexpr bool PAD = true;
    static constexpr int XU = RIN * W4;                                    // 12-byte units of the frames per item: 504 <= 512
    const float* lut;
    int xr, xo, xl;
    bool xin, fxin;                                                         // fxin, of the fetched item: this thread's row is inside the image
    unsigned fx0, fx1, fx2;
    __device__ __forceinline__ void init(const StemWgU8Args& a, int tid) {
        __shared__ float tab[U8_LUT];
        for (int i = tid; i < U8_LUT; i += 512) tab[i] = a.lut[i];
        lut = tab;
        xr = tid / W4;
        const int xc4 = tid - xr * W4;
        xin = tid < XU;
        xo = xin ? (xr * WI + xc4 * 4) * 3 : OOB;
        xl = xin ? xr * PITCH + 4 + xc4 * 4 : -1;
    }
    __device__ __forceinline__ bool live(const StemWgU8Args& a, bool on, int n, int t) const {
        return cfn_uni((int)(on && (!a.len || t < a.len[n]))) != 0;
    }
    __device__ __forceinline__ void fetch(const StemWgU8Args& a, bool ld, int n, int t, int ih0) {
        // (n's T frames of 3 P bytes: one descriptor over the whole sample)
        __amdgpu_buffer_rsrc_t rx = cfn_rsrc(a.f + (long)n * a.T * P * 3, (unsigned)((long)a.T * P * 3));
        // (the scalar offset is not range checked and must not be negative: the band's first input row, -1 for band 0, goes into the vector offset)
        const int sx = cfn_uni(ld ? t * P * 3 : 0), rowoff = cfn_uni(ih0 * WI * 3);
        fxin = ld && xin && ih0 + xr >= 0;
        const int vo = fxin ? xo + rowoff : OOB;
        fx0 = __builtin_amdgcn_raw_buffer_load_b32(rx, vo, sx, 0);
        fx1 = __builtin_amdgcn_raw_buffer_load_b32(rx, fxin ? vo + 4 : OOB, sx, 0);
        fx2 = __builtin_amdgcn_raw_buffer_load_b32(rx, fxin ? vo + 8 : OOB, sx, 0);
    }
    __device__ __forceinline__ void put(float* img) const {
        if (xl >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<st4*>(img + c * CIS + xl) = fxin ? u8_decode(lut, fx0, fx1, fx2, c) : (st4){0.f, 0.f, 0.f, 0.f};
        }
    }
};

__global__ __launch_bounds__(512, 2) void stem_u8_wgrad_kernel(const StemWgU8Args a) { stem_wgrad_body<StemWgU8>(a); }

// -1 = shape not handled: the caller converts (cfn_clip_u8_to_f32) and runs cfn_stem_conv_bwd_weight
extern "C" int cfn_stem_conv_u8_bwd_weight(const float* gy, const unsigned char* frames, const float* lut, const int* lengths, double* gw,
                                           int N, int Cimg, int Cout, int T, int Hi, int Wi, void* stream) {
    CFN_REQUIRE(gy && frames && lut && gw, "cfn_stem_conv_u8_bwd_weight: null tensor");
    CFN_REQUIRE(N > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0, "cfn_stem_conv_u8_bwd_weight: bad shape");
    CFN_REQUIRE(Cimg == 3, "cfn_stem_conv_u8_bwd_weight: uint8 frames have 3 interleaved channels, got Cimg = %d", Cimg);
    DenseShape s = dense_shape(N, Cimg, Cout, T, Hi, Wi, kStemGeom, CFN_ACT_NONE);
    s.u8 = true; s.align_x = (unsigned)((uintptr_t)frames & 15); s.align_g = (unsigned)((uintptr_t)gy & 15);
    DensePlan p;
    if (!stem_wgrad_plan(s, 0, p)) return -1;
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_STEM, st, (double)N * T * (3.0 * Hi * Wi + 4.0 * Cout * (Hi / 2) * (Wi / 2)));
    StemWgU8Args a = {gy, frames, lut, lengths, gw, N, T, p.items, p.chunk};
    hipLaunchKernelGGL(stem_u8_wgrad_kernel, dim3(p.grid[0]), dim3(512), 0, st, a);
    return cfn_check_launch("stem_conv_u8_wgrad");
}
