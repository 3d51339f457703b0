// X3D stem conv1_s on an fp32 clip (N, 3, T, H, W): the fp32 source of the two kernel bodies of stem_kernel.h, the plans of BOTH sources
// (shape gates, band height, LDS, grid: stem_u8.hip calls them too) and the fp32 launchers.
#include "stem_kernel.h"

struct StemArgs {
    const float* x; const float* w; float* y;
    int N, Cout, T, Hi, Wi, Ho, Wo, RB, RIN, WPAD, bands;
};

template <int CI_>
struct StemF32 {
    static constexpr int CI = CI_;
    // CI x RIN rows of Wi floats, float4 per thread
    static __device__ __forceinline__ void stage(const StemArgs& a, float* img, int n, int t, int ih0, int tid) {
        const int RIN = a.RIN, WPAD = a.WPAD, Wi = a.Wi, Hi = a.Hi;
        const int w4 = Wi >> 2, per_row = w4 + 1;                         // + one float4 slot that carries the left halo
        const int total = CI * RIN * per_row;
        // (all loads of a batch are issued before the first LDS write: a load -> store loop would pay one HBM round trip per
        // iteration)
        for (int e0 = tid; e0 < total; e0 += 256 * 8) {
            st4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * 256;
                const int rowid = e / per_row, c4 = e - rowid * per_row;
                const int ci = rowid / RIN, r = rowid - ci * RIN;
                const int ih = ih0 + r;
                v[u] = (st4){0.f, 0.f, 0.f, 0.f};
                if (e < total && c4 > 0 && ih >= 0 && ih < Hi)
                    v[u] = *reinterpret_cast<const st4*>(a.x + (((long)n * CI + ci) * a.T + t) * (long)Hi * Wi + (long)ih * Wi + (c4 - 1) * 4);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * 256;
                const int rowid = e / per_row, c4 = e - rowid * per_row;
                if (e < total) *reinterpret_cast<st4*>(img + rowid * WPAD + c4 * 4) = v[u];   // c4 == 0: columns 0..3 (3 = halo of iw = -1) zero
            }
        }
    }
};

template <int CI>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const StemArgs a) {
    extern __shared__ __attribute__((aligned(16))) float img[];
    stem_fwd_body<StemF32<CI>>(a, img);
}

// false = shape not handled (fp32: the implicit GEMM runs; uint8: the caller converts the clip).  v = {3}; chunk = RB, the band's output rows.
// s.u8: the frames are read 4 bytes at a time (fp32: 16) and the table sits behind the image
bool stem_fwd_plan(const DenseShape& s, DensePlan& p) {
    if (s.Cin != 3 || s.Cout > 32 || (s.Wi & 3) || (s.Hi & 1) || (s.align_x & (s.u8 ? 3 : 15))) return false;
    const int Ho = s.Hi / 2;
    p = DensePlan{};
    p.chunk = (Ho % 8 == 0) ? 8 : 4;
    p.bands = cfn_cdiv(Ho, p.chunk);
    p.lds = ((size_t)3 * (2 * p.chunk + 1) * (s.Wi + 8) + (s.u8 ? U8_LUT : 0)) * sizeof(float);
    if (p.lds > 64 * 1024) return false;
    const long blocks = (long)s.N * s.T * p.bands;
    if (blocks >= (1L << 31)) return false;
    p.family = s.u8 ? DN_STEM_U8_FWD : DN_STEM_FWD; p.v[0] = 3;
    p.items = (int)blocks; p.grid[0] = (unsigned)blocks; p.grid[1] = p.grid[2] = 1; p.wg = 256;
    return true;
}

// -1 = shape not handled (the caller uses the implicit-GEMM path)
int stem_fwd_try_launch(const float* x, const float* w, float* y, int N, int Cimg, int Cout, int T, int Hi, int Wi, hipStream_t st) {
    DenseShape s = dense_shape(N, Cimg, Cout, T, Hi, Wi, kStemGeom, CFN_ACT_NONE);
    s.align_x = (unsigned)((uintptr_t)x & 15);
    DensePlan p;
    if (!stem_fwd_plan(s, p)) return -1;
    StemArgs a = {x, w, y, N, Cout, T, Hi, Wi, Hi / 2, Wi / 2};
    a.RB = p.chunk;
    a.RIN = 2 * a.RB + 1;
    a.WPAD = Wi + 8;
    a.bands = p.bands;
    const size_t lds = p.lds;
    const long blocks = p.grid[0];
    auto k = stem_fwd_kernel<3>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), lds, st, a);
    return cfn_check_launch("stem_conv_fwd");
}

// ---- weight gradient of conv1_s at 224x224 ----
struct StemWgArgs {
    const float* gy; const float* x; double* gw;
    int N, T, items, per_block;
};

struct StemWgF32 : StemWg {
    static constexpr bool PAD = false;
    static constexpr int XU = 3 * RIN * W4, NXU = (XU + 511) / 512;       // float4 units of x per item and thread
    int xo[NXU], xl[NXU], xr[NXU];
    st4 fx[NXU];
    __device__ __forceinline__ void init(const StemWgArgs& a, int tid) {
#pragma unroll
        for (int k = 0; k < NXU; ++k) {
            const int e = k * 512 + tid;
            const int rowid = e / W4, c4 = e - rowid * W4, ci = rowid / RIN, r = rowid - ci * RIN;
            const bool in = e < XU;
            xo[k] = in ? (int)(((long)ci * a.T * P + (long)r * WI + c4 * 4) * 4) : OOB;
            xl[k] = in ? ci * CIS + r * PITCH + 4 + c4 * 4 : -1;
            xr[k] = r;
        }
    }
    __device__ __forceinline__ bool live(const StemWgArgs&, bool on, int, int) const { return on; }
    __device__ __forceinline__ void fetch(const StemWgArgs& a, bool ld, int n, int t, int ih0) {
        // (n's three channels are T * P apart: one descriptor over the whole sample)
        __amdgpu_buffer_rsrc_t rx = cfn_rsrc(a.x + (long)n * 3 * a.T * P, (unsigned)((long)3 * a.T * P * 4));
        // (the scalar offset is not range checked and must not be negative: the band's first input row, -1 for band 0, goes into the vector offset)
        const int sx = cfn_uni(ld ? t * P * 4 : 0), rowoff = cfn_uni(ih0 * WI * 4);
#pragma unroll
        for (int k = 0; k < NXU; ++k)
            fx[k] = __builtin_bit_cast(st4, __builtin_amdgcn_raw_buffer_load_b128(rx, (ld && xo[k] != OOB && ih0 + xr[k] >= 0) ? xo[k] + rowoff : OOB, sx, 0));
    }
    __device__ __forceinline__ void put(float* img) const {
#pragma unroll
        for (int k = 0; k < NXU; ++k)
            if (xl[k] >= 0) *reinterpret_cast<st4*>(img + xl[k]) = fx[k];
    }
};

__global__ __launch_bounds__(512, 2) void stem_wgrad_kernel(const StemWgArgs a) { stem_wgrad_body<StemWgF32>(a); }

// false = shape not handled.  cus < 0: the shape gates only; 0: the current device's CUs (asked once per process).  chunk = items per workgroup.
// s.u8: as in stem_fwd_plan
bool stem_wgrad_plan(const DenseShape& s, int cus, DensePlan& p) {
    if (s.Cin != 3 || s.Cout != 24 || s.Hi != 224 || s.Wi != 224 || (s.align_x & (s.u8 ? 3 : 15)) || (s.align_g & 15)) return false;
    if ((long)24 * s.T * 112 * 112 * 4 >= 0x7fff0000L) return false;
    const long items = (long)s.N * s.T * 28;
    if (items >= (1L << 30)) return false;
    p = DensePlan{};
    p.family = s.u8 ? DN_STEM_U8_WGRAD : DN_STEM_WGRAD; p.items = (int)items; p.bands = 28;
    if (cus < 0) return true;
    static int dev_cus = 0;
    if (cus == 0) { if (!dev_cus) dev_cus = dense_cu_count(); cus = dev_cus; }
    long blocks = (long)cus * 2;      // persistent workgroups per CU (8 x 256 x 224 x 224: 1: 726 us, 2: 655 us; gather-form kernel 1346)
    if (blocks > items) blocks = items;
    const long per = (items + blocks - 1) / blocks;
    blocks = (items + per - 1) / per;
    p.chunk = (int)per; p.nchunks = (int)blocks; p.last = (int)(items - (blocks - 1) * per);
    p.grid[0] = (unsigned)blocks; p.grid[1] = p.grid[2] = 1; p.wg = 512;
    p.lds = 0;      // no dynamic LDS: the kernel's images are static __shared__ arrays
    return true;
}

// -1 = shape not handled (the caller uses the implicit-GEMM path); probe: 0 = handled, nothing launched
int stem_wgrad_try_launch(const float* gy, const float* x, double* gw, int N, int Cimg, int Cout, int T, int Hi, int Wi, hipStream_t st, bool probe) {
    DenseShape s = dense_shape(N, Cimg, Cout, T, Hi, Wi, kStemGeom, CFN_ACT_NONE);
    s.align_x = (unsigned)((uintptr_t)x & 15); s.align_g = (unsigned)((uintptr_t)gy & 15);
    DensePlan p;
    if (!stem_wgrad_plan(s, probe ? -1 : 0, p)) return -1;
    if (probe) return 0;
    const long blocks = p.grid[0];
    StemWgArgs a = {gy, x, gw, N, T, p.items, p.chunk};
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3((unsigned)blocks), dim3(512), 0, st, a);
    return cfn_check_launch("stem_conv_wgrad");
}
