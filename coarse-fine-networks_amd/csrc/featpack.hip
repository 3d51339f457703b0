// Packed 16-bit fine features (cfn_hip/featpack.py): the five multi-level feature maps the Fine stream extracts per video
// (extract_fineFEAT.py:153-173 of the reference; read back by charades_coarse_fineFEAT.py:84-87) travel as fp16 or bf16, unpadded and
// TIME-MAJOR -- per video and key a block (T', C_k, 49) -- and are widened into the padded fp32 maps {k: (B, C_k, t_max, 7, 7)} the
// fusion layers take only here, on the GPU.
//
//   unpack:  out_k[b, c, t, p] = t < lengths[b] ? widen(data[offsets[b, k] + (t * C_k + c) * 49 + p]) : 0.0f        (one launch, all keys)
//   pack:    dst[blk_k + (t * C_k + c) * 49 + p] = round_to_nearest_even(x_k[c, t, p]),  blk_k = T' * 49 * (C_0 + .. + C_{k-1})
//
// Both are a (t, c) transpose at the granularity of one 49-value plane (98 bytes on the 16-bit side, 196 on the fp32 side).  One
// workgroup (4 waves) moves a tile of 8 channels x 16 frames of one (video, key) through LDS, which holds the tile as it lies on the
// 16-bit side: [frame][8 channels x 49] = rows of 784 bytes.  Channel counts are multiples of 8 and block offsets multiples of 8
// elements, so every such row starts on a 16-byte boundary of the 16-bit buffer and moves as 49 16-byte units; on the fp32 side a
// channel's frames of the tile are one contiguous run (up to 16 * 49 floats) that a wave walks with consecutive lanes on consecutive
// dwords (the run starts on a 16-byte boundary only when (c * t_max + t0) * 49 is a multiple of 4: dword accesses).
// offsets and lengths are DATA, read on the device: a length is clamped to [0, t_max], an offset is rounded down to a multiple of 8 and
// every 16-byte read is checked against the extent of `data` -- a bad offset gives zeros or wrong values, never a fault.  The grid comes
// from the OUTPUT: sum_k B * C_k / 8 * ceil(t_max / 16) workgroups, every output element written exactly once.
#include "h16.h"

typedef unsigned __attribute__((ext_vector_type(4))) fp_u4;

#define FP_TT 16                     // frames per tile
#define FP_CT 8                      // channels per tile
#define FP_P 49                      // 7 x 7 positions
#define FP_ROW (FP_CT * FP_P)        // 16-bit elements of one frame of the tile: 784 bytes = 49 units of 16 bytes
#define FP_KEYS 5

struct FeatArgs {
    const unsigned short* data; const long* off; const int* len;          // unpack: the flat 16-bit buffer, (B, 5) element offsets, (B) lengths
    unsigned short* dst;                                                   // pack: the payload
    float* f[FP_KEYS];                                                     // the fp32 maps: unpack's outputs (B, C_k, T, 49) / pack's inputs (C_k, T, 49)
    long blk[FP_KEYS];                                                     // pack: first element of key k's block in dst
    int C[FP_KEYS];
    unsigned first[FP_KEYS + 1];                                           // first workgroup of key k
    int B, T, ttiles;
    long total;                                                            // elements of data
};

struct FeatTile { int k, b, c0, t0, C; float* f; long blk; };

// workgroup -> (key, video, 8 channels, 16 frames); everything here is wave uniform.  The per-key entries are read from the kernel's
// argument block where it lies (the kernarg segment starts with the explicit arguments: the one FeatArgs) with the key as a scalar
// index -- indexing the by-value copy makes the compiler keep a private (scratch) copy of the tables per lane.
typedef const __attribute__((address_space(4))) FeatArgs* FeatArgsK;
__device__ __forceinline__ FeatTile feat_tile(const FeatArgs& a) {
    const FeatArgsK ka = (FeatArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    const unsigned L = blockIdx.x;
    FeatTile q;
    q.k = (L >= a.first[1]) + (L >= a.first[2]) + (L >= a.first[3]) + (L >= a.first[4]);
    q.C = ka->C[q.k]; q.f = ka->f[q.k]; q.blk = ka->blk[q.k];
    const unsigned base = ka->first[q.k];
    unsigned r = L - base;
    const unsigned cts = (unsigned)q.C / FP_CT;
    q.t0 = (int)(r % (unsigned)a.ttiles) * FP_TT; r /= (unsigned)a.ttiles;
    q.c0 = (int)(r % cts) * FP_CT;
    q.b = (int)(r / cts);
    return q;
}

// fp32 -> 16 bits, round to nearest even; what tensor.to(dtype) gives on the CPU for every finite value (bf16 in integer arithmetic, so
// that fp32 subnormals round like every other value whatever the denormal mode; fp16: v_cvt_f16_f32, overflow -> inf)
template <int KIND>
__device__ __forceinline__ unsigned short feat_round(float v) {
    if (KIND == H16_BF16) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);      // a NaN stays a (quiet) NaN
        return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}

template <int KIND>
__global__ __launch_bounds__(256) void feat_unpack_kernel(const FeatArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[FP_TT * FP_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6);
    const FeatTile q = feat_tile(a);
    const int nt = min(FP_TT, a.T - q.t0);                                 // frames of the tile inside t_max
    const int len = min(max(a.len[q.b], 0), a.T);
    const int live = min(max(len - q.t0, 0), nt);                          // ... of which the video has this many
    const long off = a.off[(long)q.b * FP_KEYS + q.k] & ~7L;
    for (int i = tid; i < live * FP_P; i += 256) {                         // 49 aligned 16-byte units per live frame
        const int tt = i / FP_P, u = i - tt * FP_P;
        const long e = off + ((long)(q.t0 + tt) * q.C + q.c0) * FP_P + 8 * u;
        fp_u4 v = {0u, 0u, 0u, 0u};
        if (e >= 0 && e <= a.total - 8) v = *reinterpret_cast<const fp_u4*>(a.data + e);
        *reinterpret_cast<fp_u4*>(tile + tt * FP_ROW + 8 * u) = v;
    }
    __syncthreads();
    for (int cl = wave; cl < FP_CT; cl += 4) {                             // a wave per channel: one contiguous run of nt * 49 floats
        float* dst = q.f + (((long)q.b * q.C + q.c0 + cl) * a.T + q.t0) * FP_P;
        for (int r = lane; r < nt * FP_P; r += 64) {
            const int tt = r / FP_P, p = r - tt * FP_P;
            float v = 0.0f;                                                // padding behind the video's own length
            if (tt < live) v = h16k_lo<KIND>((unsigned)tile[tt * FP_ROW + cl * FP_P + p]);
            dst[r] = v;
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void feat_pack_kernel(const FeatArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[FP_TT * FP_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6);
    const FeatTile q = feat_tile(a);
    const int nt = min(FP_TT, a.T - q.t0);
    for (int cl = wave; cl < FP_CT; cl += 4) {
        const float* src = q.f + ((long)(q.c0 + cl) * a.T + q.t0) * FP_P;
        for (int r = lane; r < nt * FP_P; r += 64) {
            const int tt = r / FP_P, p = r - tt * FP_P;
            tile[tt * FP_ROW + cl * FP_P + p] = feat_round<KIND>(src[r]);
        }
    }
    __syncthreads();
    for (int i = tid; i < nt * FP_P; i += 256) {
        const int tt = i / FP_P, u = i - tt * FP_P;
        const long e = q.blk + ((long)(q.t0 + tt) * q.C + q.c0) * FP_P + 8 * u;
        *reinterpret_cast<fp_u4*>(a.dst + e) = *reinterpret_cast<const fp_u4*>(tile + tt * FP_ROW + 8 * u);
    }
}

// channel counts, tile counts and the workgroup ranges of the keys; the number of workgroups, or -1 when it does not fit a grid
static long feat_plan(FeatArgs& a, int B, int T, const int* C) {
    a.B = B; a.T = T; a.ttiles = cfn_cdiv(T, FP_TT);
    long n = 0, blk = 0;
    for (int k = 0; k < FP_KEYS; ++k) {
        a.C[k] = C[k];
        a.first[k] = (unsigned)n;
        a.blk[k] = blk;
        n += (long)B * (C[k] / FP_CT) * a.ttiles;
        blk += (long)T * C[k] * FP_P;
        if (n >= (1L << 31)) return -1;
    }
    a.first[FP_KEYS] = (unsigned)n;
    return n;
}

static bool feat_channels_ok(const int* C) {
    for (int k = 0; k < FP_KEYS; ++k)
        if (C[k] < FP_CT || C[k] % FP_CT != 0) return false;
    return true;
}

template <int KIND>
static int feat_unpack(const unsigned short* data, const long* offsets, const int* lengths, float* const* out, int B, int t_max, const int* C,
                       long total, void* stream, const char* what) {
    CFN_REQUIRE(data && offsets && lengths && out[0] && out[1] && out[2] && out[3] && out[4], "%s: null tensor", what);
    CFN_REQUIRE(B >= 1 && t_max >= 1 && total >= 0, "%s: bad shape (B %d, t_max %d, %ld elements)", what, B, t_max, total);
    CFN_REQUIRE(feat_channels_ok(C), "%s: channel counts must be positive multiples of 8, got %d %d %d %d %d", what, C[0], C[1], C[2], C[3], C[4]);
    CFN_REQUIRE(((uintptr_t)data & 15) == 0, "%s: data must start on a 16-byte boundary", what);
    FeatArgs a = {};
    a.data = data; a.off = offsets; a.len = lengths; a.total = total;
    for (int k = 0; k < FP_KEYS; ++k) a.f[k] = out[k];
    const long blocks = feat_plan(a, B, t_max, C);
    CFN_REQUIRE(blocks > 0, "%s: too many tiles for one grid", what);
    hipStream_t st = (hipStream_t)stream;
    double elems = 0.0;
    for (int k = 0; k < FP_KEYS; ++k) elems += (double)B * C[k] * t_max * FP_P;
    CfnProfScope prof(CFN_K_ELEMWISE, st, elems * 6.0);
    hipLaunchKernelGGL(feat_unpack_kernel<KIND>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return cfn_check_launch(what);
}

template <int KIND>
static int feat_pack(const float* const* x, unsigned short* dst, int T, const int* C, void* stream, const char* what) {
    CFN_REQUIRE(x[0] && x[1] && x[2] && x[3] && x[4] && dst, "%s: null tensor", what);
    CFN_REQUIRE(T >= 1, "%s: bad shape (%d frames)", what, T);
    CFN_REQUIRE(feat_channels_ok(C), "%s: channel counts must be positive multiples of 8, got %d %d %d %d %d", what, C[0], C[1], C[2], C[3], C[4]);
    CFN_REQUIRE(((uintptr_t)dst & 15) == 0, "%s: dst must start on a 16-byte boundary", what);
    FeatArgs a = {};
    a.dst = dst;
    for (int k = 0; k < FP_KEYS; ++k) a.f[k] = const_cast<float*>(x[k]);
    const long blocks = feat_plan(a, 1, T, C);
    CFN_REQUIRE(blocks > 0, "%s: too many tiles for one grid", what);
    hipStream_t st = (hipStream_t)stream;
    double elems = 0.0;
    for (int k = 0; k < FP_KEYS; ++k) elems += (double)C[k] * T * FP_P;
    CfnProfScope prof(CFN_K_ELEMWISE, st, elems * 6.0);
    hipLaunchKernelGGL(feat_pack_kernel<KIND>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return cfn_check_launch(what);
}

extern "C" int cfn_feat_unpack_f16(const unsigned short* data, const long* offsets, const int* lengths, float* out0, float* out1, float* out2,
                                   float* out3, float* out4, int B, int t_max, int c0, int c1, int c2, int c3, int c4, long total, void* stream) {
    float* const out[FP_KEYS] = {out0, out1, out2, out3, out4};
    const int C[FP_KEYS] = {c0, c1, c2, c3, c4};
    return feat_unpack<H16_F16>(data, offsets, lengths, out, B, t_max, C, total, stream, "cfn_feat_unpack_f16");
}

extern "C" int cfn_feat_unpack_bf16(const unsigned short* data, const long* offsets, const int* lengths, float* out0, float* out1, float* out2,
                                    float* out3, float* out4, int B, int t_max, int c0, int c1, int c2, int c3, int c4, long total, void* stream) {
    float* const out[FP_KEYS] = {out0, out1, out2, out3, out4};
    const int C[FP_KEYS] = {c0, c1, c2, c3, c4};
    return feat_unpack<H16_BF16>(data, offsets, lengths, out, B, t_max, C, total, stream, "cfn_feat_unpack_bf16");
}

extern "C" int cfn_feat_pack_f16(const float* x0, const float* x1, const float* x2, const float* x3, const float* x4, unsigned short* dst, int T,
                                 int c0, int c1, int c2, int c3, int c4, void* stream) {
    const float* const x[FP_KEYS] = {x0, x1, x2, x3, x4};
    const int C[FP_KEYS] = {c0, c1, c2, c3, c4};
    return feat_pack<H16_F16>(x, dst, T, C, stream, "cfn_feat_pack_f16");
}

extern "C" int cfn_feat_pack_bf16(const float* x0, const float* x1, const float* x2, const float* x3, const float* x4, unsigned short* dst, int T,
                                  int c0, int c1, int c2, int c3, int c4, void* stream) {
    const float* const x[FP_KEYS] = {x0, x1, x2, x3, x4};
    const int C[FP_KEYS] = {c0, c1, c2, c3, c4};
    return feat_pack<H16_BF16>(x, dst, T, C, stream, "cfn_feat_pack_bf16");
}
