// Which kernel serves a pointwise (1x1x1) conv call -- forward and data gradient (below), weight gradient, one-pass backward and strided-shortcut
// backward (further down) -- is decided HERE, apart from launching it.  Host arithmetic only: no kernel, no HIP call.  Every family's X_plan (next to its kernel) holds its own shape predicate and tile / grid arithmetic; this file holds the ORDER in which the
// plans are asked, the one reader of the switches, and cfn_pwconv_route, the same decision as a query that needs no device.
//
// The first plan that accepts wins, so the regions below are what is LEFT by the families in front.  M = output rows of the contraction (forward:
// Cout, data gradient: Cin), K = contraction length (forward: Cin, data gradient: Cout), Q = positions per sample.  All split-bf16 families need
// stride 1, CFN_PW_SPLIT = 6 (pws: 3 or 6), no compact shortcut gradient `acc` in the kernel, and 16-byte aligned tensors (pwt's data gradient: 4).
//
//  slot family  takes                                                                     why (measured, 8 clips x 256 frames unless said otherwise)
//  ---- ------- ------------------------------------------------------------------------- ---------------------------------------------------------
//  0, 1 pwk,pwt data gradient with `acc` and NO act' epilogue: planned without `acc`,      stage-first conv1 of layers 3 / 4: 0.77 ms on pw_deep_kernel
//               pw_lattice_add_kernel behind the contraction (plan.lattice_add)            with the in-kernel lattice loads.  The split-bf16 kernels
//                                                                                         decline `acc` themselves: its lattice loads cost their
//                                                                                         many-row variants 90+ registers.  Without an epilogue
//                                                                                         "W^T g' + acc" is the same fp32 sum either way.
//  2    pwk     Q % 4 == 0 and either                                                      register-resident weights.  The act' epilogue at 192 -> 432
//               two k slices: 128 < K <= 224, 32 < M <= 128, even number of 16-blocks;     rows needs 256 VGPRs + 63 spilled dwords, 0.256 vs 0.260 ms
//               one slice:    48 <= K <= 112 (192 when M > 256), 128 < M <= 512,           for pw_deep_kernel: not instantiated (M <= 256 there).
//                             forward or act' epilogue (then M <= 256)
//  3    pwt     M > 32 and (K >= 400, or act' epilogue with K >= 160 and M > 256);         weights streamed through LDS.  K >= 400, every mode, @7x7
//               forward: Q % 4 == 0                                                        against pw_deep_kernel: forward 432 -> 192 0.223 -> 0.142 ms,
//                                                                                         data gradient with two staged operands 0.229 -> 0.161, 432
//                                                                                         rows 0.50 -> 0.31, 96 rows @14x14 0.54 -> 0.37.  The act'
//                                                                                         epilogue into more than 256 rows also from K = 160 (layer-4
//                                                                                         conv3: contraction over 192, 432 rows in three slabs: 0.273
//                                                                                         -> 0.223 ms; pwk takes the shapes of up to 256 rows first).
//                                                                                         Needs its workspace: none (stream capture) = next family.
//  4    pws     48 <= K <= 128, M > 32, Q % 4 == 0, at most two slabs                      weight images resident in LDS.  The split costs VALU work
//                                                                                         per CONTRACTION-side element (prologue + 9 instructions per
//                                                                                         pair for three terms) and saves matrix time per product:
//                                                                                         measured (profiles/r03_microbench_b8.txt) it wins up to
//                                                                                         K = 108 (layer 2 both convs, layer 3 conv1 forward 0.18 vs
//                                                                                         0.21 ms, conv3 data gradient 0.24 vs 0.33 ms) and loses from
//                                                                                         K = 216 on (layer 3 conv3 forward 0.22-0.26 vs 0.20 ms).
//                                                                                         Three or more slabs re-read every activation that often:
//                                                                                         0.19-0.31 vs 0.20-0.24 ms for the fp32-MFMA kernel.
//  5    pwd     stride 1, K >= 48, M > 32, two or more row tiles under a 120 KiB image     fp32 MFMA, 8 waves, one deep resident weight image; also the
//                                                                                         data gradients WITH `acc` and an act' epilogue.
//  6    gemm    everything else (stride 2, K < 48, M <= 32, odd Q ...)                     fp32 MFMA; refuses only tensors beyond the 2 GiB descriptor
//                                                                                         range.
#include "pw_common.h"
#include <cstdio>
#include <cstdlib>

// The only reader of the pointwise switches.  CFN_PW_SPLIT once per process (cfn_pw_split_terms changes it afterwards); the others per call: tests and
// A/B harnesses switch them inside one process.  Only the backward chains' plans use those three, so the forward and the data gradient (backward =
// false) pay no getenv per call.
static int pw_int(const char* e, int unset) { return e ? atoi(e) : unset; }

static int g_pws_terms = -1;      // 0 = off (fp32 MFMA kernels), 3 / 6 = MFMAs per k-block

PwSwitches pw_switches_now(bool backward) {
    if (g_pws_terms < 0) {
        g_pws_terms = pw_int(getenv("CFN_PW_SPLIT"), 6);
        if (g_pws_terms != 0 && g_pws_terms != 3 && g_pws_terms != 6) g_pws_terms = 6;
    }
    PwSwitches sw = {g_pws_terms, 1, 0, 1};
    if (!backward) return sw;
    sw.pwf_split = pw_int(getenv("CFN_PWF_SPLIT"), 1);      // default 1: the no-prologue shapes (measured in the step: -1.3 .. -1.9 ms; level 2 loses 0.5 ms of it)
    sw.pwf_l3e = pw_int(getenv("CFN_PWF_L3E"), 0);          // while it is being measured: off unless set
    const char* e = getenv("CFN_PW_SHORT");                 // 0 = the two separate kernels
    sw.pw_short = !(e && e[0] && atoi(e) == 0);
    return sw;
}
int pws_terms_now() { return pw_switches_now(false).split_terms; }

extern "C" int cfn_pw_split_terms(int terms) {
    const int prev = pws_terms_now();
    if (terms == 0 || terms == 3 || terms == 6) g_pws_terms = terms;
    else if (terms != -1) return cfn_fail(CFN_ERR_ARG, "cfn_pw_split_terms: terms must be 0 (fp32 MFMA), 3 or 6 (or -1 to query)"), -2;
    return prev;
}

typedef bool (*PwPlanFn)(const PwArgs&, int, bool, const PwSwitches&, PwPlan&);
static const PwPlanFn kChain[] = {pwk_plan, pwt_plan, pwk_plan, pwt_plan, pws_plan, pwd_plan, pw_gemm_plan};

static bool pw_route(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p, int from) {
    const unsigned io = p.align_io, ex = p.align_ex;
    // slots 0 and 1 are entered only when `lattice` holds: `noacc` is read there and nowhere else
    const bool lattice = mode == PW_DGRAD && a.acc && !a.ea;
    PwArgs noacc;
    if (lattice) { noacc = a; noacc.acc = nullptr; }
    for (int slot = from < 2 && !lattice ? 2 : from; slot < 7; ++slot) {
        p = PwPlan{};
        p.align_io = io; p.align_ex = ex; p.slot = slot;
        if (slot < 2 ? kChain[slot](noacc, mode, false, sw, p) : kChain[slot](a, mode, stats, sw, p)) {
            p.lattice_add = slot < 2;
            return true;
        }
    }
    return false;
}

bool pw_route_fwd(const PwArgs& a, bool stats, const PwSwitches& sw, PwPlan& p, int from) { return pw_route(a, PW_FWD, stats, sw, p, from); }
bool pw_route_dgrad(const PwArgs& a, bool stats, const PwSwitches& sw, PwPlan& p, int from) { return pw_route(a, PW_DGRAD, stats, sw, p, from); }

// ---- the backward chains ----------------------------------------------------------------------------------------------------------------------
//  weight gradient (M = Cout, K = Cin):
//   0  pss  stride 1, split 3 or 6, M, K >= 48, 16-byte aligned: staged split-bf16 kernel + fixed-order reduce (no workspace: fp64 atomics)
//   1  wd   stride 1: M, K >= 48, Q % 4 == 0, aligned (only what pss left: split 0); stride 2: Wo % 4 == 0 -- direct operands
//   2  wg   everything else (layer 1, odd planes): LDS-staged fp32
//  one-pass backward (data + weight gradient; stride 1, Q % 4 == 0, 16-byte aligned, CFN_PWF_SPLIT >= 1 and split 6 for the first three):
//   0  pf3  no prologue, 192 < Cout <= 224, 32 < Cin <= 96 (layer 3's conv1); needs its workspace
//   1  pf3e CFN_PWF_L3E, prologue, no acc, 64 < Cout <= 96, 192 < Cin <= 224 (layer 3's conv3); needs its workspace
//   2  pfs  64 < Cout <= 128 with 16 <= Cin <= 64, or 64 < Cin <= 128 with 32 < Cout <= 64; with a prologue only at CFN_PWF_SPLIT >= 2 (layer 2)
//   3  pf   Cin, Cout <= 64 and not both > 32 (layer 1), fp32
//      nothing accepts: the entry point returns -1 and the caller uses the data-gradient and weight-gradient entry points
//  strided-shortcut backward: psh alone (stride 2, CFN_PW_SHORT != 0, Cout <= 192, Cin <= 96, 4-byte aligned), else -1
static bool pw_route_bwd(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p, int from, int n, bool (*plan)(const PwBwdShape&, const PwSwitches&, int, PwBwdPlan&)) {
    for (int slot = from; slot < n; ++slot) {
        p = PwBwdPlan{};
        p.slot = slot;
        if (plan(s, sw, slot, p)) return true;
    }
    return false;
}
bool pw_route_wgrad(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p, int from) {
    return pw_route_bwd(s, sw, p, from, 3, [](const PwBwdShape& s, const PwSwitches& sw, int slot, PwBwdPlan& p) {
        return slot == 0 ? pws_wgrad_plan(s, sw, p) : (slot == 1 ? pwd_wgrad_plan(s, sw, p) : pw_wg_plan(s, sw, p)); });
}
bool pw_route_fused(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p, int from) {
    return pw_route_bwd(s, sw, p, from, 4, [](const PwBwdShape& s, const PwSwitches& sw, int slot, PwBwdPlan& p) {
        static const int fam[3] = {PW_FAM_PF3, PW_FAM_PF3E, PW_FAM_PFS};
        return slot < 3 ? pwfs_plan(s, sw, fam[slot], p) : pf_plan(s, sw, p); });
}
bool pw_route_short(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p) {
    p = PwBwdPlan{};
    return psh_plan(s, sw, p);
}

// ---- the same decision as a host-only query ----------------------------------------------------------------------------------------------
// "family kernel<template arguments> grid=.. wg=.. lds=.. ws=.." -- the kernel spelled as a kernel trace prints it
static int pw_route_line(const PwPlan& p, char* out, int cap) {
    const char* const tf[] = {"false", "true"};
    char k[128];
    switch (p.family) {
        case PW_FAM_PWK: snprintf(k, sizeof k, "pwk pwk_kernel<%d, %d, %d, %d, %s, %s>", p.nkb, p.KS, p.mode, p.act, tf[p.stats], tf[p.mode == PW_DGRAD && p.two]); break;
        case PW_FAM_PWT:
        case PW_FAM_PWS: snprintf(k, sizeof k, "%s pws_kernel<%d, %d, %d, %s, %d, %s, %d, %d>", p.family == PW_FAM_PWT ? "pwt" : "pws", p.MT, p.NP, p.mode, tf[p.stats],
                                  p.act, tf[p.mode == PW_DGRAD && p.two], p.NS, p.family == PW_FAM_PWT ? 3 : 0); break;
        case PW_FAM_PWD: snprintf(k, sizeof k, "pwd pw_deep_kernel<%d, %d, %s, %d, 8>", p.MT, p.mode, tf[p.stats], p.act); break;
        default: snprintf(k, sizeof k, "pw_gemm pw_gemm_kernel<%d, %d, %s, %d, false>", p.MT, p.mode, tf[p.stats], p.act); break;
    }
    return snprintf(out, cap, "%s grid=%u wg=%u lds=%zu ws=%zu%s", k, p.blocks, p.threads, p.lds, p.ws_bytes, p.lattice_add ? " +lattice_add" : "");
}

static int pw_bwd_line(const PwBwdPlan& p, char* out, int cap) {
    const char* const tf[] = {"false", "true"};
    const int* t = p.t;
    char k[160];
    switch (p.family) {
        case PW_FAM_PSS: snprintf(k, sizeof k, "pss pws_wgrad_staged_kernel<%d, %d, %d, %s, %d, %d, %d, %d, %s>", t[0], t[1], p.act, tf[p.two], t[2], t[3], t[4], t[5], tf[t[6]]); break;
        case PW_FAM_WD: snprintf(k, sizeof k, "wd pw_wgrad_direct_kernel<%d, %d, %d, %d>", p.act, t[0], t[1], t[2]); break;
        case PW_FAM_WG: snprintf(k, sizeof k, "wg pw_wgrad_kernel<%d, %d>", t[0], t[1]); break;
        case PW_FAM_PF3: snprintf(k, sizeof k, "pf3 pw_bwd_fused_split3_kernel<%d, %d>", t[0], t[1]); break;
        case PW_FAM_PF3E: snprintf(k, sizeof k, "pf3e pw_bwd_fused_split3e_kernel<%d, %d, %d>", t[0], t[1], p.act); break;
        case PW_FAM_PFS: snprintf(k, sizeof k, "pfs pw_bwd_fused_split_kernel<%d, %d, %d>", t[0], t[1], p.act); break;
        case PW_FAM_PF: snprintf(k, sizeof k, "pf pw_bwd_fused_kernel<%d, %d, %d>", t[0], t[1], p.act); break;
        default: snprintf(k, sizeof k, "psh pw_short_bwd_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d>", t[0], t[1], t[2], t[3], t[4], t[5], t[6], p.vec, p.act, t[7]); break;
    }
    return snprintf(out, cap, "%s grid=%u wg=%u lds=%zu ws=%zu", k, p.blocks, p.threads, p.lds, p.ws_bytes);
}

extern "C" int cfn_pwconv_route(int op, int N, int Cin, int Cout, int T, int Hi, int Wi, int stride, int act, int flags, char* out, int cap) {
    CFN_REQUIRE(out && cap > 0, "cfn_pwconv_route: no output buffer");
    CFN_REQUIRE(op >= 0 && op <= 4, "cfn_pwconv_route: op must be 0 .. 4");
    CFN_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && T > 0 && Hi > 0 && Wi > 0 && (stride == 1 || stride == 2), "cfn_pwconv_route: bad shape");
    CFN_REQUIRE((long)T * Hi * Wi < (1L << 31), "cfn_pwconv_route: per-sample volume too large");
    static const double some[2] = {0.0, 0.0};      // stands for "this tensor is present": plans look at null-ness only
    const float* f = reinterpret_cast<const float*>(some);
    double* d = const_cast<double*>(some);
    const bool pro = flags & 1, stat = flags & 2, yp = flags & 4, accp = flags & 8;
    if (op >= 2) {
        PwBwdShape s = {N, Cin, Cout, T, Hi, Wi, stride, act};
        s.pro = pro; s.two = stat && yp; s.acc = accp; s.acc_stride = 2;
        s.align_g = s.align_x = s.align_out = flags & 16 ? 4 : 0;
        PwBwdPlan bp = {};
        CFN_REQUIRE(op != 3 || stride == 1, "cfn_pwconv_route: the one-pass backward has no stride");
        const PwSwitches sw = pw_switches_now(true);
        const bool ok = op == 2 ? pw_route_wgrad(s, sw, bp, 0) : (op == 3 ? pw_route_fused(s, sw, bp, 0) : pw_route_short(s, sw, bp));
        if (!ok) { snprintf(out, cap, "declined"); return CFN_OK; }
        pw_bwd_line(bp, out, cap);
        return CFN_OK;
    }
    PwArgs a = {};
    a.src = f; a.w = f; a.dst = const_cast<float*>(f); a.act = act;
    a.N = N; a.Cin = Cin; a.Hi = Hi; a.Wi = Wi; a.stride = stride;
    a.Ho = (Hi - 1) / stride + 1; a.Wo = (Wi - 1) / stride + 1;
    a.Pin = T * Hi * Wi; a.Q = T * a.Ho * a.Wo;
    if (op == 0) {
        a.M = Cout; a.K = Cin;
        if (pro) { a.pa = some; a.pb = some; }
        if (stat) { a.s1 = d; a.s2 = d; }
    } else {
        a.M = Cin; a.K = Cout; a.ex = f;
        if (stat) { a.gs = some; if (yp) { a.src2 = f; a.gq = some; } }      // gsumsq comes with y; gsum alone stages one operand
        if (pro) { a.ea = some; a.eb = some; a.s1 = d; a.s2 = d; }
        if (accp) {
            CFN_REQUIRE(stride == 1, "cfn_pwconv_route: acc needs stride 1");
            a.acc = f; a.acc_s = 2; a.acc_Ho = (Hi - 1) / 2 + 1; a.acc_Wo = (Wi - 1) / 2 + 1;
        }
    }
    PwPlan p = {};
    p.align_io = p.align_ex = flags & 16 ? 4 : 0;
    const bool ok = op == 0 ? pw_route_fwd(a, stat, pw_switches_now(false), p, 0) : pw_route_dgrad(a, pro, pw_switches_now(false), p, 0);
    if (!ok) { snprintf(out, cap, "declined"); return CFN_OK; }      // (ops 0 / 1: only a tensor beyond the 2 GiB descriptor range; the entry point fails)
    pw_route_line(p, out, cap);
    return CFN_OK;
}
