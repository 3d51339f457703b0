// Depthwise 3x3x3 conv (cfn_dwconv3d_fwd / _bwd_data / _bwd_weight / _bwd_fused / _bwd_fused_s2, every element type): what a plan sees of a
// call and what it decides.  Host arithmetic only.  Every family's X_plan sits next to its kernel, in the fp32 compilation of its source
// (#ifndef DW_BF16: the element type enters only as the element size `es`, so the library holds each gate once), with its shape gates and
// its chunk / grid arithmetic; X_launch (one per element type) fills the argument struct from the route and launches.  dwroute.hip holds
// the order in which the plans are asked and cfn_dwconv3d_route, the same decision as a query that needs no device.
#pragma once
#include "cfn_common.h"
#include "h16.h"
#include <stdint.h>

struct DwShape {
    int N, C, T, Hi, Wi, stride, act;      // Hi, Wi: the conv's INPUT plane (x / gx)
    bool pro, stats, y;                    // prologue A, B present; forward: sum / sumsq asked for, backward: gsum present; gsumsq and y present
    bool yptr;                             // backward: y was passed (the byte figures count it), with or without gsumsq
    int es;                                // element size of the activation tensors: 4 (fp32) or 2 (bf16 and fp16 alike)
    unsigned align_x, align_g, align_out;  // low 4 address bits of x, of gy | y (y where passed), of the output (y, gx)
};

// tensors of a call, element type erased (the launchers of one element type cast them back)
struct DwFwdPtrs { const void* x; const double* A; const double* B; const float* w; void* y; double* sum; double* sumsq; };
struct DwBwdPtrs {
    const void* gy; const void* y; const double* gs; const double* gq; const float* w; const void* x;
    const double* A; const double* B; void* gx; double* gA; double* gB; double* gw;
};

enum { DW_FWD = 0, DW_DGRAD = 1, DW_WGRAD = 2 };      // MODE of dw3d_kernel
enum { DW_FAM_FLAT = 1, DW_FAM_FLAT_S2, DW_FAM_FLAT14TO7, DW_FAM_CP, DW_FAM_SMALL, DW_FAM_BAND, DW_FAM_DGRAD_S2,
       DW_FAM_FLATB, DW_FAM_CPBX, DW_FAM_BANDF, DW_FAM_FLATB_S2, DW_FAM_CPB2X };

struct DwRoute {
    int family;
    int v[6];                  // the template arguments the host selects, in the family's order (see each X_plan)
    unsigned grid[3], wg;
    size_t lds;                // dynamic LDS (the band kernels; the wave kernels' images are static)
    int TT, nchunks;           // frames per t-chunk (flat kernels: the template's TO), chunks (flat backward: wave items) per (sample, channel)
    int subs;                  // flat backward: consecutive chunks per wave item
    long items;                // work items / waves over the whole grid (flat, cp, small: `total` / `total_waves` of the argument struct)
    int Ho, Wo, CG, ngroups, GB, nbands, IPCb, IPCp, RIN, WP, XO;      // band kernels: the geometry fields of DwArgs / DwFusedArgs
    int PB, CPB, pblocks, PBLK;                                         // stride-2 data gradient: DwS2Args
    double bytes;              // tensor traffic of the call, for CfnProfScope
    int rc;                    // plan returned false: CFN_OK = not this family's shape, otherwise the error the entry point returns
};

typedef bool (*DwPlanFn)(const DwShape&, DwRoute&);
// forward
bool dw_flat_plan(const DwShape& s, DwRoute& r);         // dwflat.hip   stride 1, 56 / 28: v = {W, RB, TO}; 14: dw3d_flat14_fwd_kernel, v = {TO}
bool dw_flat_s2_plan(const DwShape& s, DwRoute& r);      //              stride 2, 112 / 56 / 28: v = {Wo, RB, TO}
bool dw_flat14to7_plan(const DwShape& s, DwRoute& r);    //              stride 2, 14 -> 7: v = {TO}
bool dw_cp_plan(const DwShape& s, DwRoute& r);           // dwcp.hip     v = {Wo, S, HS, RG, D, OCC}
bool dw_small_plan(const DwShape& s, DwRoute& r);        // dwsmall.hip  v = {7, 1}
bool dw_band_fwd_plan(const DwShape& s, DwRoute& r);     // dwconv3d.hip v = {MODE, S, HS, VEC, MAXLD, UNIW}; false with rc set: unsupported
// data gradient, weight gradient
bool dw_band_dgrad_plan(const DwShape& s, DwRoute& r);   //              stride 1
bool dw_dgrad_s2_plan(const DwShape& s, DwRoute& r);     //              stride 2: v = {fast, PACKED}
bool dw_band_wgrad_plan(const DwShape& s, DwRoute& r);
// one-pass backward
bool dw_flatb_plan(const DwShape& s, DwRoute& r);        // dwflatb.hip  7x7: v = {TO, HASY}
bool dw_cpbx_plan(const DwShape& s, DwRoute& r);         // dwcpbx.hip   v = {W, HS, RG, D, OCC, HASY}
bool dw_bandf_plan(const DwShape& s, DwRoute& r);        // dwconv3d.hip v = {HS, VEC, MAXLD, UNIW}
bool dw_flatb_s2_plan(const DwShape& s, DwRoute& r);     // dwflatb.hip  14 -> 7: v = {TO, HASY}
bool dw_cpb2x_plan(const DwShape& s, DwRoute& r);        // dwcpb2x.hip  v = {Wo, RG, OCC, HASY}

// dwroute.hip: the first plan of the op's chain that accepts.  CFN_OK: r holds the route; -1: nothing accepts (one-pass backward: the caller
// uses the two separate entry points); otherwise the error of the plan that refused the call
enum { DW_OP_FWD = 0, DW_OP_DGRAD = 1, DW_OP_WGRAD = 2, DW_OP_FUSED = 3 };
int dw_route(int op, const DwShape& s, DwRoute& r);

// the launchers of the wave kernels, one set per element type (the sources are compiled again through <name>_bf16.hip / <name>_f16.hip)
#ifdef DW_BF16
#define DWN(name) H16N(name)
int DWN(dw_cp_launch)(const DwFwdPtrs& p, const DwShape& s, const DwRoute& r, hipStream_t st);       // dwcp.hip: 2-byte elements only
#else
#define DWN(name) name
int dw_flat_launch(const DwFwdPtrs& p, const DwShape& s, const DwRoute& r, hipStream_t st);          // dwflat.hip: fp32 only, all three families
#endif
int DWN(dw_small_launch)(const DwFwdPtrs& p, const DwShape& s, const DwRoute& r, hipStream_t st);    // dwsmall.hip
int DWN(dw_flatb_launch)(const DwBwdPtrs& p, const DwShape& s, const DwRoute& r, hipStream_t st);    // dwflatb.hip: flatb and flatb_s2
int DWN(dw_cpbx_launch)(const DwBwdPtrs& p, const DwShape& s, const DwRoute& r, hipStream_t st);     // dwcpbx.hip

inline unsigned dw_low4(const void* p) { return (unsigned)((uintptr_t)p & 15); }
inline DwShape dw_fwd_shape(const DwFwdPtrs& p, int N, int C, int T, int Hi, int Wi, int stride, int act, int es) {
    DwShape s = {N, C, T, Hi, Wi, stride, act};
    s.pro = p.A != nullptr; s.stats = p.sum != nullptr; s.es = es;
    s.align_x = dw_low4(p.x); s.align_out = dw_low4(p.y);
    return s;
}
inline DwShape dw_bwd_shape(const DwBwdPtrs& p, int N, int C, int T, int Hi, int Wi, int stride, int act, int es) {
    DwShape s = {N, C, T, Hi, Wi, stride, act};
    s.pro = p.A != nullptr; s.stats = p.gs != nullptr; s.y = p.gq != nullptr && p.y != nullptr; s.yptr = p.y != nullptr; s.es = es;
    s.align_x = dw_low4(p.x); s.align_g = dw_low4(p.gy) | dw_low4(p.y); s.align_out = dw_low4(p.gx);
    return s;
}
