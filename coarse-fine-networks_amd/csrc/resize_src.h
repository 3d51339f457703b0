// Index arithmetic of the temporal linear resize (F.interpolate mode='linear'), shared by the resize kernels of gridpool.hip and the
// fused detection loss of detloss.hip: one definition, so both see the same taps and weights bit for bit.
#pragma once
#include "cfn_common.h"

// ---- temporal linear resize: align_corners=True (F.interpolate 'linear' x3d_coarse.py:725 and the t-axis of
// 'trilinear' :449 when h,w keep their size) or half-pixel centres (align_corners=False: the loss upsampling of
// train_coarse_fineFEAT.py:226) -- ATen's area_pixel_compute_scale / _source_index in the same operation order
__device__ __forceinline__ void resize_src(int j, int Kin, int Lout, int ac, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    float src;
    if (ac) {
        const float scale = Lout > 1 ? (float)(Kin - 1) / (float)(Lout - 1) : 0.0f;
        src = scale * (float)j;
    } else {
        const float scale = (float)Kin / (float)Lout;
        src = fmaf(scale, (float)j + 0.5f, -0.5f);   // ATen's CPU build contracts this expression into one FMA (checked
        if (src < 0.0f) src = 0.0f;                  // against F.interpolate: 2e-7 with, 1e-5 without)
    }
    i0 = (int)src;
    i1 = i0 + (i0 < Kin - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// the outputs j whose source interval can touch input k, as a (generous) closed range [jlo, jhi] within [0, Lout-1]: the caller still
// checks i0 / i1 of every j in it exactly.  (src(j) = j*(Kin-1)/(Lout-1) in [k-1, k+1]  =>  j in [(k-1)/scale, (k+1)/scale])
__device__ __forceinline__ void resize_gather_range(int k, int Kin, int Lout, int ac, int& jlo, int& jhi) {
    jlo = 0, jhi = Lout - 1;
    if (!ac) {              // src(j) = (j + 0.5) * Kin / Lout - 0.5 (clamped at 0) within [k-1, k+1]
        const double inv = (double)Lout / (double)Kin;
        jlo = k == 0 ? 0 : (int)floor((k - 0.5) * inv - 0.5) - 1;
        jhi = (int)ceil((k + 1.5) * inv - 0.5) + 1;
        if (jlo < 0) jlo = 0;
        if (jhi > Lout - 1) jhi = Lout - 1;
    } else if (Kin > 1 && Lout > 1) {
        const double inv = (double)(Lout - 1) / (double)(Kin - 1);
        jlo = (int)floor((k - 1) * inv) - 1;
        jhi = (int)ceil((k + 1) * inv) + 1;
        if (jlo < 0) jlo = 0;
        if (jhi > Lout - 1) jhi = Lout - 1;
    }
}
