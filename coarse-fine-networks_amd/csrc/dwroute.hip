// Which kernel serves a depthwise 3x3x3 conv call -- forward, data gradient, weight gradient, one-pass backward at stride 1 and 2, for 4-byte and
// 2-byte elements -- is decided HERE, apart from launching it.  Host arithmetic only: no kernel, no HIP call.  Every family's X_plan (next to its
// kernel, dw_plan.h) holds its own shape gates and chunk / grid arithmetic; this file holds the ORDER in which the plans are asked and
// cfn_dwconv3d_route, the same decision as a query that needs no device.  No depthwise source reads an environment switch.
//
// The first plan that accepts wins, so the regions below are what is LEFT by the families in front.  Every wave family (all but band, bandf and
// dgrad_s2) needs a square plane, a prologue that is ReLU or none (branch-free prologue; act' from the sign of a), and one sample's channel
// volume T x H x W within a buffer descriptor's range.  Measured: one box, 8 clips x 256 frames, unless said otherwise.
//
//  op, element       slot family     takes                                                    why
//  ----------------- ---- ---------- -------------------------------------------------------- ------------------------------------------------------
//  forward, 4-byte   0    flat       stride 1 onto 56 / 28 / 14, x and y 16-byte aligned      every load of a work item issued up front, items in
//                    1    flat_s2    stride 2, 112 -> 56, 56 -> 28, 28 -> 14, same            memory order: 56x56 586 us on the column-pair kernel ->
//                    2    flat14to7  stride 2, 14 -> 7, same                                  515-523 (5.3-5.4 TB/s), 28x28 293 -> 257-261; stride 2
//                                                                                             (cp / flat at TO = 8): 112 -> 56 1373 / 1211 us, 56 -> 28
//                                                                                             686 / 622, 28 -> 14 358 / 309.  Power bound.
//  forward, 2-byte   0    cp         stride 1 and 2 onto 56 / 28 / 14, x and y 8-byte aligned  a wave per (channel, t-chunk, band), two columns per lane:
//                                                                                             2 rows per lane, 93 VGPRs, 5 waves per SIMD: 5.1 TB/s
//                                                                                             against 3.5 with the band kernel's 7 rows (168 VGPRs).
//  forward, both     +1   small      7x7, stride 1                                            a wave per (channel, t-chunk), weights in SGPRs: 142 ->
//                                                                                             96 us (2.4 -> 3.6 TB/s) against the band kernel.
//                    +2   band       everything else (Wo <= 512, the plane fits the LDS band   dw3d_kernel: CG channels x a band of rows x a t-chunk per
//                                    scheme); refuses otherwise: the entry point fails        workgroup.  2-byte 14 -> 7 runs here (no flat14to7).
//  data gradient     0    dgrad_s2   stride 2; fast: even width, prologue, gsumsq + y,         gather form, 256 positions per workgroup; PACKED: planes
//                                    CPB channel volumes within the descriptor range          of <= 128 positions share a workgroup.
//                    1    band       stride 1                                                 2-row strips on planes <= 14 rows (4 clips: 14x14 0.31 ->
//                                                                                             0.25 ms, 7x7 0.25 -> 0.16 with 4-wave workgroups).
//  weight gradient   0    band       everything                                               stride 2: one row per thread (4 clips, 112 -> 56:
//                                                                                             1.17 -> 0.77 ms against 7-row strips).
//  one pass, s 1     0    flatb      7x7                                                      a lane per position, 49 of 64 lanes (a column-pair kernel
//                                                                                             keeps 28 busy: 2.4 TB/s); `subs` = 8 chunks per wave: one
//                                                                                             chunk per wave was 2.6 x slower (27 fp64 atomics each).
//                    1    cpbx       56 / 28 / 14; gy, y, x, gx aligned to 4 elements          one LDS image, x / a in registers: 5 tensor passes instead
//                                                                                             of the two kernels' 7; 56x56 1.20 ms at 64-frame chunks.
//                    2    bandf      wave-uniform channels, float4 rows, MAXLD != 8, 4-row     dw3d_bwd_fused_kernel: 56x56 1.92 ms with 4-row strips
//                                    strips, else 7-row strips; dynamic LDS <= 150 KiB        (164 VGPRs, 3 waves per SIMD), 2.18 with 7, 2.35 for the
//                                                                                             two separate kernels; no gain on 14x14 / 7x7 planes.
//                         declined   everything else: the entry point returns -1 and the caller uses the data-gradient and weight-gradient entry points
//  one pass, s 2     0    flatb_s2   14 -> 7; x and gx aligned to 2 elements                   the flat backward's scheme on the 2 x 2 input blocks.
//                    1    cpb2x      112 -> 56, 56 -> 28, 28 -> 14; aligned to 4 elements      x read once, gx written once: the two kernels read x twice;
//                                                                                             112 -> 56 2.68 ms at 24-frame chunks.
//                         declined   everything else, as above
#include "dw_plan.h"
#include <cstdio>

static const DwPlanFn kFwd4[] = {dw_flat_plan, dw_flat_s2_plan, dw_flat14to7_plan, dw_small_plan, dw_band_fwd_plan, nullptr};
static const DwPlanFn kFwd2[] = {dw_cp_plan, dw_small_plan, dw_band_fwd_plan, nullptr};
static const DwPlanFn kDgrad[] = {dw_dgrad_s2_plan, dw_band_dgrad_plan, nullptr};
static const DwPlanFn kWgrad[] = {dw_band_wgrad_plan, nullptr};
static const DwPlanFn kFused[] = {dw_flatb_plan, dw_cpbx_plan, dw_bandf_plan, nullptr};
static const DwPlanFn kFusedS2[] = {dw_flatb_s2_plan, dw_cpb2x_plan, nullptr};

// tensor traffic of a call for CfnProfScope: the tensors at input resolution, those at output resolution, the forward's weights
// (the data and weight gradient entry points have always counted 4 bytes per element, whatever the element type)
static double dw_bytes(int op, const DwShape& s) {
    const double in = (double)s.Hi * s.Wi, out = ((s.Hi - 1) / s.stride + 1.0) * ((s.Wi - 1) / s.stride + 1.0), nct = (double)s.N * s.C * s.T;
    switch (op) {
        case DW_OP_FWD: return s.es * nct * (in + out) + 4.0 * s.C * 27;
        case DW_OP_DGRAD: return 4.0 * nct * (in * (s.pro ? 2 : 1) + out * (s.yptr ? 2 : 1));
        case DW_OP_WGRAD: return 4.0 * nct * (in + out * (s.y ? 2 : 1));
        default: return s.es * nct * (2.0 * in + out * (s.yptr ? 2 : 1));
    }
}

int dw_route(int op, const DwShape& s, DwRoute& r) {
    const DwPlanFn* chain = op == DW_OP_FWD ? (s.es == 4 ? kFwd4 : kFwd2) : op == DW_OP_DGRAD ? kDgrad : op == DW_OP_WGRAD ? kWgrad : (s.stride == 1 ? kFused : kFusedS2);
    for (; *chain; ++chain) {
        r = DwRoute{};
        if ((*chain)(s, r)) { r.bytes = dw_bytes(op, s); return CFN_OK; }
        if (r.rc) return r.rc;
    }
    return -1;
}

// ---- the same decision as a host-only query ----------------------------------------------------------------------------------------------
// "family kernel<template arguments> grid=.. wg=.. lds=.." -- the kernel spelled as a kernel trace prints it, the grid in workgroups
static void dw_route_line(const DwRoute& r, char* out, int cap) {
    const char* const tf[] = {"false", "true"};
    const int* v = r.v;
    char k[128], g[48];
    switch (r.family) {
        case DW_FAM_FLAT: if (v[1]) snprintf(k, sizeof k, "flat dw3d_flat_fwd_kernel<%d, %d, %d>", v[0], v[1], v[2]);
                          else snprintf(k, sizeof k, "flat dw3d_flat14_fwd_kernel<%d>", v[0]); break;
        case DW_FAM_FLAT_S2: snprintf(k, sizeof k, "flat_s2 dw3d_flat_s2_fwd_kernel<%d, %d, %d>", v[0], v[1], v[2]); break;
        case DW_FAM_FLAT14TO7: snprintf(k, sizeof k, "flat14to7 dw3d_flat14to7_fwd_kernel<%d>", v[0]); break;
        case DW_FAM_CP: snprintf(k, sizeof k, "cp dw3d_cp_fwd_kernel<%d, %d, %d, %d, %d, %d>", v[0], v[1], v[2], v[3], v[4], v[5]); break;
        case DW_FAM_SMALL: snprintf(k, sizeof k, "small dw3d_small_fwd_kernel<%d, %d>", v[0], v[1]); break;
        case DW_FAM_BAND: snprintf(k, sizeof k, "band dw3d_kernel<%d, %d, %d, %d, %d, %s>", v[0], v[1], v[2], v[3], v[4], tf[v[5]]); break;
        case DW_FAM_DGRAD_S2: snprintf(k, sizeof k, "dgrad_s2 dw3d_dgrad_s2%s_kernel<%s>", v[0] ? "_fast" : "", tf[v[1]]); break;
        case DW_FAM_FLATB: snprintf(k, sizeof k, "flatb dw3d_flat7_bwd_kernel<%d, %s>", v[0], tf[v[1]]); break;
        case DW_FAM_CPBX: snprintf(k, sizeof k, "cpbx dw3d_cpx_bwd_kernel<%d, %d, %d, %d, %d, %s>", v[0], v[1], v[2], v[3], v[4], tf[v[5]]); break;
        case DW_FAM_BANDF: snprintf(k, sizeof k, "bandf dw3d_bwd_fused_kernel<%d, %d, %d, %s>", v[0], v[1], v[2], tf[v[3]]); break;
        case DW_FAM_FLATB_S2: snprintf(k, sizeof k, "flatb_s2 dw3d_flat14to7_bwd_kernel<%d, %s>", v[0], tf[v[1]]); break;
        default: snprintf(k, sizeof k, "cpb2x dw3d_cpx_bwd_s2_kernel<%d, %d, %d, %s>", v[0], v[1], v[2], tf[v[3]]); break;
    }
    if (r.grid[1] > 1 || r.grid[2] > 1) snprintf(g, sizeof g, "%ux%ux%u", r.grid[0], r.grid[1], r.grid[2]);
    else snprintf(g, sizeof g, "%u", r.grid[0]);
    snprintf(out, cap, "%s grid=%s wg=%u lds=%zu", k, g, r.wg, r.lds);
}

// op: 0 forward, 1 data gradient, 2 weight gradient, 3 one-pass backward (its stride: cfn_dwconv3d_bwd_fused or _bwd_fused_s2).  dtype: 0 fp32,
// 1 bf16, 2 fp16.  flags: 1 prologue, 2 forward: statistics, backward: gsum, 4 gsumsq and y, 16 every tensor aligned to its element only
extern "C" int cfn_dwconv3d_route(int op, int dtype, int N, int C, int T, int Hi, int Wi, int stride, int act, int flags, char* out, int cap) {
    CFN_REQUIRE(out && cap > 0, "cfn_dwconv3d_route: no output buffer");
    CFN_REQUIRE(op >= 0 && op <= 3, "cfn_dwconv3d_route: op must be 0 .. 3");
    CFN_REQUIRE(dtype >= 0 && dtype <= 2, "cfn_dwconv3d_route: dtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
    CFN_REQUIRE(N > 0 && C > 0 && T > 0 && Hi > 0 && Wi > 0 && (stride == 1 || stride == 2), "cfn_dwconv3d_route: bad shape");
    DwShape s = {N, C, T, Hi, Wi, stride, act};
    s.es = dtype == 0 ? 4 : 2;
    s.pro = flags & 1; s.stats = flags & 2;
    if (op != DW_OP_FWD) s.y = s.yptr = flags & 4;
    s.align_x = s.align_g = s.align_out = flags & 16 ? s.es : 0;
    DwRoute r;
    const int rc = dw_route(op, s, r);
    if (rc == -1) { snprintf(out, cap, "declined"); return CFN_OK; }
    if (rc) return rc;
    dw_route_line(r, out, cap);
    return CFN_OK;
}
