// Frame labels from annotation segments (cfn_hip/seglabels.py): a batch carries every video's [class, start_s, end_s] triples and its label
// window instead of the dense (C, TL) fp32 array the reference builds per video with a Python loop over frames and actions
// (charades_fine.py:110-117, charades_coarse_fineFEAT.py:115-122), slices per sample (charades_fine.py:149-165, :188) and pads per batch
// (mt_collate_fn, charades_fine.py:214-220).  One launch writes what those three steps give, bit for bit:
//
//   fr = window[b, 0] + t,  len = clamp(window[b, 1], 0, t_max)
//   labels[b, c, t] = t < len and some segment (c, s, e) of video b has  fr / fps[b] > s  and  fr / fps[b] < e   ? 1.0f : 0.0f
//   mask[b, t]      = t < len ? 1.0f : 0.0f
//   valid_t[b]      = len
//
// fr / fps is ONE correctly rounded fp64 division of the exact integer by the fps the host computed (num_frames / duration in Python), the
// inequalities are strict: the reference's expression, not fr * (1 / fps) or fr * duration / num_frames, which round differently on frame
// times that meet a segment bound.  (This build has no fast-math flag; a per-file one would break the equality.)
//
// Store bound: B * (C + 1) * t_max * 4 bytes out, a few hundred bytes in.  The mask is row C of a virtual (C + 1)-row map.  A workgroup
// (4 waves) owns 256 frames x 16 rows of one video; a wave owns 4 of the rows and all 256 frames: each lane divides its 4 frames once, walks
// the video's segments in LDS (wave-uniform reads; a segment of another wave's rows costs one scalar compare) and keeps one hit bit per
// (row, frame).  With t_max a multiple of 4 a lane's frames are consecutive and leave as one 16-byte store per row (a wave writes 1 KiB
// contiguous); otherwise lanes take consecutive frames and store dwords.  offsets, fps and window are DATA, read on the device: an
// offset range is clamped to [0, n_seg], a length to [0, t_max], and a class that is not an integer of [0, C) selects no row -- a bad
// batch gives wrong values, never a store outside the outputs.  Every element of the three outputs is written exactly once.
#include "cfn_common.h"

#define SL_FRAMES 256                // frames per workgroup
#define SL_ROWS 16                   // rows (classes, then the mask) per workgroup
#define SL_WROWS (SL_ROWS / 4)       // ... per wave
#define SL_CHUNK 128                 // segments held in LDS at a time

typedef float __attribute__((ext_vector_type(4))) sl_f4;

template <bool VEC>
__global__ __launch_bounds__(256) void seg_labels_kernel(const double* __restrict__ seg, const int* __restrict__ offsets, const double* __restrict__ fps,
                                                         const int* __restrict__ window, float* __restrict__ labels, float* __restrict__ mask,
                                                         int* __restrict__ valid_t, int C, int t_max, long n_seg) {
    __shared__ int s_cls[SL_CHUNK];
    __shared__ double s_lo[SL_CHUNK], s_hi[SL_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = cfn_uni(tid >> 6);
    const int b = blockIdx.z, t0 = blockIdx.x * SL_FRAMES;
    const int row0 = blockIdx.y * SL_ROWS + wave * SL_WROWS;               // this wave's rows: row0 .. row0 + 3 of the C + 1
    const int len = min(max(window[2 * b + 1], 0), t_max);
    const long start = window[2 * b];
    const double f = fps[b];
    long s0 = offsets[b], s1 = offsets[b + 1];
    s0 = min(max(s0, 0L), n_seg); s1 = min(max(s1, s0), n_seg);
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) valid_t[b] = len;

    int t[4];
    double x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[j] = VEC ? t0 + 4 * lane + j : t0 + lane + 64 * j;
        x[j] = (double)(start + t[j]) / f;                                 // the reference's fr / fps
    }
    unsigned hits = 0;                                                     // bit 4 * (row - row0) + j
    for (long base = s0; base < s1; base += SL_CHUNK) {
        const int n = (int)min((long)SL_CHUNK, s1 - base);
        __syncthreads();
        if (tid < n) {
            const double* r = seg + 3 * (base + tid);
            const double cd = r[0];
            int cls = -1;
            if (cd >= 0.0 && cd < (double)C && (double)(int)cd == cd) cls = (int)cd;
            s_cls[tid] = cls; s_lo[tid] = r[1]; s_hi[tid] = r[2];
        }
        __syncthreads();
        for (int s = 0; s < n; ++s) {
            const unsigned ci = (unsigned)(cfn_uni(s_cls[s]) - row0);      // wave uniform
            if (ci < (unsigned)SL_WROWS) {
                const double lo = s_lo[s], hi = s_hi[s];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x[j] > lo && x[j] < hi) hits |= 1u << (4 * ci + j);
            }
        }
    }
#pragma unroll
    for (int ci = 0; ci < SL_WROWS; ++ci) {
        const int row = row0 + ci;
        if (row > C) break;
        const bool is_mask = row == C;
        float* dst = is_mask ? mask + (long)b * t_max : labels + ((long)b * C + row) * t_max;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (t[j] < len && (is_mask || ((hits >> (4 * ci + j)) & 1u))) ? 1.0f : 0.0f;
        if (VEC) {
            if (t[0] < t_max) *reinterpret_cast<sl_f4*>(dst + t[0]) = sl_f4{v[0], v[1], v[2], v[3]};      // (t_max % 4 == 0: all four inside)
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t[j] < t_max) dst[t[j]] = v[j];
        }
    }
}

extern "C" int cfn_seg_labels(const double* seg, const int* offsets, const double* fps, const int* window, float* labels, float* mask, int* valid_t,
                              int B, int C, int t_max, long n_seg, void* stream) {
    const char* what = "cfn_seg_labels";
    CFN_REQUIRE(seg && offsets && fps && window && labels && mask && valid_t, "%s: null tensor", what);
    CFN_REQUIRE(B >= 1 && C >= 1 && t_max >= 1 && n_seg >= 0, "%s: bad shape (B %d, C %d, t_max %d, %ld segments)", what, B, C, t_max, n_seg);
    CFN_REQUIRE(B <= 65535 && C < (1 << 19) && t_max < (1 << 24) && n_seg < (1L << 31), "%s: too large (B %d, C %d, t_max %d, %ld segments)", what, B,
                C, t_max, n_seg);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cfn_cdiv(t_max, SL_FRAMES), (unsigned)cfn_cdiv((long)C + 1, SL_ROWS), (unsigned)B);
    const bool vec = t_max % 4 == 0 && (((uintptr_t)labels | (uintptr_t)mask) & 15) == 0;
    CfnProfScope prof(CFN_K_ELEMWISE, st, (double)B * (C + 1) * t_max * 4.0);
    if (vec) hipLaunchKernelGGL(seg_labels_kernel<true>, grid, dim3(256), 0, st, seg, offsets, fps, window, labels, mask, valid_t, C, t_max, n_seg);
    else hipLaunchKernelGGL(seg_labels_kernel<false>, grid, dim3(256), 0, st, seg, offsets, fps, window, labels, mask, valid_t, C, t_max, n_seg);
    return cfn_check_launch(what);
}
