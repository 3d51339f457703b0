// cfn_conv3d_dense_route: which kernel serves a dense conv call (cfn_conv3d_dense_fwd / _bwd_data / _bwd_weight, cfn_stem_conv_fwd /
// _bwd_weight, cfn_stem_conv_u8_fwd / _bwd_weight), asked on the host.  No kernel, no stream: the X_plan functions the launchers call (dense_plan.h), in the launchers' order.
//
//  op 0 forward:          salb (split bf16; cfn_pw_split_terms == 6)  ->  sal_fwd (fp32 MFMA)  ->  implicit GEMM (pw_gemm_kernel, STEM = true)
//  op 1 data gradient:    sal_dgrad  ->  all input channels in one thread (Cin <= 32, weights <= 64 KiB)  ->  one input channel per grid row
//  op 2 weight gradient:  sal_wgrad  ->  direct operands (Wo % 4 == 0, Q % 4 == 0, aligned gy)  ->  LDS-staged (every shape)
//  op 3 stem forward:     stem_fwd   ->  op 0 with the stem geometry
//  op 4 stem weight gradient:  stem_wgrad (224 x 224)  ->  op 2 with the stem geometry
//  op 5 uint8 stem forward:          stem_u8_fwd    ->  "convert " + op 3: the entry point returns -1, the caller converts the frames
//  op 6 uint8 stem weight gradient:  stem_u8_wgrad  ->  "convert " + op 4       (cfn_clip_u8_to_f32) and calls the fp32 entry point
#include "pw_common.h"
#include <cstdio>

// "family kernel<template arguments> grid=.. wg=.. lds=.." -- the kernel spelled as a kernel trace prints it; the sal kernels add
// "bands=.. chunk=.. nchunks=.. last=.. items=..", the stem kernels "bands=.. chunk=.." (rows per band / items per workgroup) and "items=.."
static void dense_route_line(const DensePlan& p, char* out, int cap) {
    const char* const tf[] = {"false", "true"};
    const int* v = p.v;
    char k[128], g[48];
    bool sal = false, stem = false;
    switch (p.family) {
        case DN_SALB: snprintf(k, sizeof k, "salb sal_fwdb_kernel<%d, %s>", v[0], tf[v[1]]); sal = true; break;
        case DN_SAL_FWD: snprintf(k, sizeof k, "sal sal_fwd_kernel<%d, %d, %s>", v[0], v[1], tf[v[2]]); sal = true; break;
        case DN_SAL_DGRAD: snprintf(k, sizeof k, "sal sal_dgrad_kernel<%d, %s, %s>", v[0], tf[v[1]], tf[v[2]]); sal = true; break;
        case DN_SAL_WGRAD: snprintf(k, sizeof k, "sal sal_wgrad_kernel<%d, %s, %s>", v[0], tf[v[1]], tf[v[2]]); sal = true; break;
        case DN_ALLCI: snprintf(k, sizeof k, "allci conv3d_dense_bwd_data_allci_kernel<%d>", v[0]); break;
        case DN_PERCH: snprintf(k, sizeof k, "perch conv3d_dense_bwd_data_kernel"); break;
        case DN_GEMM: snprintf(k, sizeof k, "pw_gemm pw_gemm_kernel<%d, %d, %s, %d, true>", v[0], v[1], tf[v[2]], v[3]); break;
        case DN_WD: snprintf(k, sizeof k, "wd pw_wgrad_direct_kernel<%d, %d, %d, %d>", v[0], v[1], v[2], v[3]); break;
        case DN_WG: snprintf(k, sizeof k, "wg pw_wgrad_kernel<%d, %d>", v[0], v[1]); break;
        case DN_STEM_FWD: snprintf(k, sizeof k, "stem stem_fwd_kernel<%d>", v[0]); stem = true; break;
        case DN_STEM_U8_FWD: snprintf(k, sizeof k, "stem stem_u8_fwd_kernel"); stem = true; break;
        case DN_STEM_U8_WGRAD: snprintf(k, sizeof k, "stem stem_u8_wgrad_kernel"); stem = true; break;
        default: snprintf(k, sizeof k, "stem stem_wgrad_kernel"); stem = true; break;
    }
    if (p.grid[1] > 1 || p.grid[2] > 1) snprintf(g, sizeof g, "%ux%ux%u", p.grid[0], p.grid[1], p.grid[2]);
    else snprintf(g, sizeof g, "%u", p.grid[0]);
    int n = snprintf(out, cap, "%s grid=%s wg=%u lds=%zu", k, g, p.wg, p.lds);
    if (n < 0 || n >= cap) return;
    if (sal) snprintf(out + n, cap - n, " bands=%d chunk=%d nchunks=%d last=%d items=%d", p.bands, p.chunk, p.nchunks, p.last, p.items);
    else if (stem) snprintf(out + n, cap - n, " bands=%d chunk=%d items=%d", p.bands, p.chunk, p.items);
}

// flags: 1 prologue (ReLU; with 32: Swish), 2 forward: statistics, backward: gsum, 4 gsumsq and y, 16 every tensor 4 bytes off a 16-byte boundary;
// one tensor alone: 64 x, 128 gy and y, 256 the output (y / gx).  Ops 5, 6: 16 and 64 put the frames off a 4-byte boundary; the clip a declined
// call is converted into is a new allocation and aligned.
// cus: CUs to plan for; 0 = those of the current device (256 where there is none)
extern "C" int cfn_conv3d_dense_route(int op, int N, int Cin, int Cout, int T, int Hi, int Wi, const int* geom, int flags, int cus, char* out, int cap) {
    CFN_REQUIRE(out && cap > 0, "cfn_conv3d_dense_route: no output buffer");
    CFN_REQUIRE(op >= 0 && op <= 6, "cfn_conv3d_dense_route: op must be 0 .. 6");
    CFN_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0 && cus >= 0, "cfn_conv3d_dense_route: bad shape");
    CFN_REQUIRE(op >= 3 || geom, "cfn_conv3d_dense_route: ops 0 .. 2 need a geometry");
    const bool pro = flags & 1, u8 = op >= 5;
    if (u8) op -= 2;
    DenseShape s = dense_shape(N, Cin, Cout, T, Hi, Wi, op >= 3 ? kStemGeom : geom, pro ? (flags & 32 ? CFN_ACT_SWISH : CFN_ACT_RELU) : CFN_ACT_NONE);
    s.pro = pro;
    if (op == 0) s.stats = flags & 2;
    if (op == 1 || op == 2) { s.gs = flags & 2; s.y = flags & 4; }
    s.align_x = flags & (16 | 64) ? 4 : 0;
    s.align_g = flags & (16 | 128) ? 4 : 0;
    s.align_out = flags & (16 | 256) ? 4 : 0;
    if (op == 1 && !pro) s.align_x = 0;      // the data gradient reads x only for the prologue
    if (op == 1 && !dense_dgrad_fits(N, Cin)) { snprintf(out, cap, "declined"); return CFN_OK; }      // the entry point refuses it, whatever the kernel
    if (cus == 0) cus = dense_cu_count();
    DensePlan p = {};
    bool ok;
    if (u8) {
        if (Cin != 3) { snprintf(out, cap, "declined"); return CFN_OK; }      // uint8 frames have 3 interleaved channels: the entry point fails
        s.u8 = true;
        if (s.align_x) s.align_x = 1;
        if (op == 3 ? stem_fwd_plan(s, p) : stem_wgrad_plan(s, cus, p)) { dense_route_line(p, out, cap); return CFN_OK; }
        s.u8 = false; s.align_x = 0;
        const int n = snprintf(out, cap, "convert ");
        if (n >= cap) return CFN_OK;
        out += n; cap -= n;
    }
    switch (op == 3 ? (stem_fwd_plan(s, p) ? -1 : 0) : (op == 4 ? (stem_wgrad_plan(s, cus, p) ? -1 : 2) : op)) {
        case -1: ok = true; break;
        case 0: ok = s.act != CFN_ACT_SWISH && (salb_fwd_plan(s, cus, p) || sal_fwd_plan(s, cus, p) || dense_gemm_plan(s, p)); break;      // (the forward's prologue is ReLU or none)
        case 1: ok = sal_dgrad_plan(s, cus, p) || dense_dgrad_plan(s, p); break;
        default: ok = sal_wgrad_plan(s, cus, p) || dense_wd_plan(s, p) || dense_wg_plan(s, p); break;
    }
    if (!ok) { snprintf(out, cap, "declined"); return CFN_OK; }      // no kernel: the entry point fails
    dense_route_line(p, out, cap);
    return CFN_OK;
}
