// Crop + antialiased bilinear resize + horizontal flip of uint8 frames on the GPU, bit-exact to PIL's 8-bit Image.resize(BILINEAR).
// The reference does this per frame on the CPU: MultiScaleRandomCropMultigrid + RandomHorizontalFlip (train_fine.py:74-77,
// train_coarse_fineFEAT.py:79-82; transforms/spatial_transforms.py:480-510, :339-357) and CenterCropScaled (train_fine.py:78,
// extract_fineFEAT.py:76; spatial_transforms.py:201-230).
//
// src (N, T, Hs, Ws, 3) uint8, every clip's picture in the top-left corner of a common Hs x Ws; box (N, 4) = x1, y1, c, flip; the
// host built the fixed-point tap tables of the c -> S resize (cfn_hip/u8aug.py: bounds (N, S, 2) = xmin, n; coef (N, S, K) with 22
// fractional bits, zero behind n) -- the square crop into a square output uses ONE table for both axes.  dst (N, T, S, S, 3).
//   pass 1 (horizontal): tmp[y][xx] = clip8((2^21 + sum_k src[y1 + y][x1 + xmin(xx) + k] * coef[xx][k]) >> 22)     rounded to uint8
//   pass 2 (vertical):   out[yy][xx] = clip8((2^21 + sum_k tmp[xmin(yy) + k][xx] * coef[yy][k]) >> 22)
// int32 accumulators; c == S has the table [2^22, 0]: the identity, exactly.  The flip mirrors the output columns: pass 1 writes
// pixel xx to column S - 1 - xx.  Frames t >= lengths[n] are written as zero bytes (the U8Clips contract).
//
// One workgroup (4 waves) = a band of RB = 8 output rows of one frame.  The rows of the crop the band needs -- at most
// (RB + 1) * fs + 1 of them, fs = max(c / S, 1) <= K / 2 -- go through pass 1 into an LDS image of uint8 rows of S * 3 bytes;
// neighbouring bands recompute the few rows they share.  A wave takes one source row at a time: the row starts at byte
// (y * Ws + x1) * 3, at any alignment, so it is fetched as the 16-byte aligned units that cover it (the ragged head and tail are
// part of their units; a unit that is not wholly inside the src buffer is read byte by byte, every byte checked against the
// buffer's extent) into the wave's own LDS staging row, while the previous row is being filtered.  Pass 2 runs out of LDS and
// writes the band, which is one contiguous run of dst, as aligned 16-byte stores (bytes in front of / behind the run: byte stores);
// where the rows of dst start on dword boundaries (S * 3 % 4 == 0, the usual case) it filters 4 bytes per LDS read.
// The tables, the box and the lengths are DATA: whatever they hold, indices are clamped to what was staged and nothing outside
// src / dst is touched -- a bad box gives wrong bytes, not a fault.
#include "cfn_common.h"

typedef unsigned __attribute__((ext_vector_type(4))) au4;

#define AUG_RB 8                 // output rows per workgroup
#define AUG_KMAX 9               // widest table: c <= 4 * S
#define AUG_UPL_MAX 5            // 16-byte units per lane and source row the kernel is built for
#define AUG_LDS_MAX (64 * 1024)

struct AugArgs {
    const unsigned char* src; const int* len; const int* box; const int* bounds; const int* coef; unsigned char* dst;
    int T, Hs, Ws, S, K, bands, rows, pitch, stg, cmax;
    long total;                                                           // bytes of src
};

__device__ __forceinline__ unsigned aug_clip8(int acc) {
    const int v = acc >> 22;
    return (unsigned)min(max(v, 0), 255);
}

template <int UPL>
__global__ __launch_bounds__(256) void aug_u8_kernel(const AugArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6);
    unsigned L = cfn_xcd_remap(blockIdx.x, gridDim.x);
    const int band = L % a.bands; L /= a.bands;
    const int t = L % a.T, n = L / a.T;
    const int S = a.S, K = a.K, pitch = a.pitch;
    unsigned char* img = lds;                                             // [rows][pitch]: pass 1's output
    unsigned char* stage = lds + a.rows * pitch + wave * a.stg;           // this wave's source row
    int* tb = reinterpret_cast<int*>(lds + a.rows * pitch + 4 * a.stg);   // [S][2] xmin, n
    int* tc = tb + 2 * S;                                                 // [S][K]
    const int oh0 = band * AUG_RB, nro = min(AUG_RB, S - oh0);
    const bool live = !a.len || t < a.len[n];

    // the band in dst: nb contiguous bytes
    const long dband = (((long)n * a.T + t) * S + oh0) * (long)S * 3;
    const int rb = S * 3, nb = nro * rb;
    const int dhead = (int)((uintptr_t)(a.dst + dband) & 15);
    const int nunits = (dhead + nb + 15) >> 4;

    int y0 = 0, nrows = 0;
    if (live) {
        for (int i = tid; i < 2 * S; i += 256) tb[i] = a.bounds[(long)n * 2 * S + i];
        for (int i = tid; i < S * K; i += 256) tc[i] = a.coef[(long)n * S * K + i];
        __syncthreads();
        const int x1 = a.box[4 * n], y1 = a.box[4 * n + 1], flip = a.box[4 * n + 3];
        const int cc = min(max(a.box[4 * n + 2], 0), a.cmax);             // what the staging row holds
        y0 = tb[2 * oh0];
        int yend = y0;
        for (int r = 0; r < nro; ++r) yend = max(yend, tb[2 * (oh0 + r)] + tb[2 * (oh0 + r) + 1]);
        nrows = min(max(yend - y0, 0), a.rows);

        // ---- pass 1: source rows y0 .. y0 + nrows - 1 of the crop, one per wave at a time ----
        const long fbase = ((long)n * a.T + t) * (long)a.Hs * a.Ws * 3;
        au4 pf[UPL];
        int head = 0;
        auto fetch = [&](int r) {
            const long off = fbase + (((long)y1 + y0 + r) * a.Ws + x1) * 3;
            head = (int)(((uintptr_t)a.src + (unsigned long)off) & 15);
            const long o0 = off - head;
            const int nu = (head + cc * 3 + 15) >> 4;
#pragma unroll
            for (int i = 0; i < UPL; ++i) {
                const int u = lane + 64 * i;
                const long o = o0 + 16L * u;
                au4 v = {0u, 0u, 0u, 0u};
                if (u < nu) {
                    if (o >= 0 && o + 16 <= a.total) {
                        v = *reinterpret_cast<const au4*>(a.src + o);
                    } else {                                              // the buffer's first / last bytes, or a box outside it
#pragma unroll
                        for (int b = 0; b < 16; ++b) {
                            const long ob = o + b;
                            const unsigned byte = (ob >= 0 && ob < a.total) ? a.src[ob] : 0u;
                            v[b >> 2] |= byte << (8 * (b & 3));
                        }
                    }
                }
                pf[i] = v;
            }
        };
        int r = wave;
        if (r < nrows) fetch(r);
        for (; r < nrows; r += 4) {
            const int hd = head;
#pragma unroll
            for (int i = 0; i < UPL; ++i) {
                const int u = lane + 64 * i;
                if (16 * u + 16 <= a.stg) *reinterpret_cast<au4*>(stage + 16 * u) = pf[i];
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");        // the wave's staging row is written (one wave: no barrier)
            __builtin_amdgcn_wave_barrier();
            if (r + 4 < nrows) fetch(r + 4);                              // in flight while this row is filtered
            unsigned char* orow = img + r * pitch;
            for (int xx = lane; xx < S; xx += 64) {
                const int2 bn = reinterpret_cast<const int2*>(tb)[xx];
                const int xmin = bn.x, nn = min(bn.y, K);
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                for (int k = 0; k < nn; ++k) {
                    const int xi = xmin + k;
                    if ((unsigned)xi < (unsigned)cc) {
                        const unsigned char* p = stage + hd + xi * 3;
                        const int w = tc[xx * K + k];
                        a0 += p[0] * w; a1 += p[1] * w; a2 += p[2] * w;
                    }
                }
                unsigned char* q = orow + (flip ? S - 1 - xx : xx) * 3;
                q[0] = (unsigned char)aug_clip8(a0); q[1] = (unsigned char)aug_clip8(a1); q[2] = (unsigned char)aug_clip8(a2);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");        // the staging row is read before it is overwritten
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
    }

    // ---- pass 2 and the store: 16 aligned bytes of dst per thread ----
    const bool fast = ((rb | dhead) & 3) == 0;                            // rows and the band start on dword boundaries of dst
    for (int u = tid; u < nunits; u += 256) {
        const int f0 = 16 * u - dhead;                                    // byte f0 + b of the band
        unsigned word[4] = {0u, 0u, 0u, 0u};
        if (live && fast) {                                              // whole dwords of one row: 4 bytes per LDS read and table lookup
            const int fs = max(f0, 0);
            int row = fs / rb, col = fs - row * rb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = f0 + 4 * j;
                if (f >= 0 && f < nb) {
                    const int oy = oh0 + row;
                    const int2 bn = reinterpret_cast<const int2*>(tb)[oy];
                    const int ym = bn.x - y0, nn = min(bn.y, K);
                    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
                    for (int k = 0; k < nn; ++k) {
                        const int li = ym + k;
                        if ((unsigned)li < (unsigned)nrows) {
                            const unsigned d = *reinterpret_cast<const unsigned*>(img + li * pitch + col);
                            const int w = tc[oy * K + k];
                            a0 += (int)(d & 255u) * w; a1 += (int)((d >> 8) & 255u) * w;
                            a2 += (int)((d >> 16) & 255u) * w; a3 += (int)(d >> 24) * w;
                        }
                    }
                    word[j] = aug_clip8(a0) | (aug_clip8(a1) << 8) | (aug_clip8(a2) << 16) | (aug_clip8(a3) << 24);
                    col += 4;
                    if (col == rb) { col = 0; ++row; }
                }
            }
        } else if (live) {
            const int fs = max(f0, 0);
            int row = fs / rb, col = fs - row * rb;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const int f = f0 + b;
                if (f >= 0 && f < nb) {
                    const int oy = oh0 + row;
                    const int ym = tb[2 * oy] - y0, nn = min(tb[2 * oy + 1], K);
                    int acc = 1 << 21;
                    for (int k = 0; k < nn; ++k) {
                        const int li = ym + k;
                        if ((unsigned)li < (unsigned)nrows) acc += img[li * pitch + col] * tc[oy * K + k];
                    }
                    word[b >> 2] |= aug_clip8(acc) << (8 * (b & 3));
                    if (++col == rb) { col = 0; ++row; }
                }
            }
        }
        unsigned char* d = a.dst + dband + f0;
        if (f0 >= 0 && f0 + 16 <= nb) {
            *reinterpret_cast<au4*>(d) = (au4){word[0], word[1], word[2], word[3]};
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (f0 + b >= 0 && f0 + b < nb) d[b] = (unsigned char)(word[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// -1 = not handled, nothing launched: a table wider than 9 taps (c > 4 * S) or an output too wide for the LDS image
extern "C" int cfn_crop_resize_flip_u8(const unsigned char* src, const int* lengths, const int* box, const int* bounds, const int* coef,
                                       unsigned char* dst, int N, int T, int Hs, int Ws, int S, int K, void* stream) {
    CFN_REQUIRE(src && box && bounds && coef && dst, "cfn_crop_resize_flip_u8: null tensor");
    CFN_REQUIRE(N > 0 && T > 0 && Hs > 0 && Ws > 0 && S > 0 && K > 0, "cfn_crop_resize_flip_u8: bad shape");
    if (K > AUG_KMAX) return -1;
    const int half = K / 2 > 1 ? K / 2 : 1;                               // fs <= half: the largest crop is half * S pixels
    AugArgs a = {src, lengths, box, bounds, coef, dst, T, Hs, Ws, S, K};
    a.bands = cfn_cdiv(S, AUG_RB);
    a.rows = (AUG_RB + 1) * half + 2;                                     // >= (RB + 1) * fs + 1
    a.pitch = (S * 3 + 15) & ~15;
    if ((long)S * half > (1 << 20)) return -1;
    a.cmax = S * half;
    a.stg = (a.cmax * 3 + 32 + 15) & ~15;                                 // head (<= 15) + row + the tail of the last unit
    const long lds = (long)a.rows * a.pitch + 4L * a.stg + (long)S * (2 + K) * 4;
    const int upl = cfn_cdiv(a.stg, 1024);
    if (lds > AUG_LDS_MAX || upl > AUG_UPL_MAX) return -1;
    const long blocks = (long)N * T * a.bands;
    if (blocks >= (1L << 31)) return -1;
    a.total = (long)N * T * Hs * Ws * 3;
    hipStream_t st = (hipStream_t)stream;
    CfnProfScope prof(CFN_K_ELEMWISE, st, (double)a.total + (double)N * T * S * S * 3);
    void (*k)(const AugArgs) = upl <= 1 ? aug_u8_kernel<1> : upl == 2 ? aug_u8_kernel<2> : upl == 3 ? aug_u8_kernel<3> : aug_u8_kernel<5>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), (size_t)lds, st, a);
    return cfn_check_launch("crop_resize_flip_u8");
}
