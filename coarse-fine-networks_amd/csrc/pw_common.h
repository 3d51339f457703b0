// Shared declarations of the pointwise-contraction kernels (pwconv.hip, pwdeep.hip).
#pragma once
#include "cfn_common.h"

typedef float __attribute__((ext_vector_type(16))) f16v;
typedef float __attribute__((ext_vector_type(4))) f4v;

enum { PW_FWD = 0, PW_DGRAD = 1 };
#define PW_KC 32
#define PW_RED_PITCH 33

struct PwArgs {
    const float* src;    // FWD: x raw (N,K,Pin)          DGRAD: gy (N,K,Q)
    const float* src2;   // DGRAD: y raw (N,K,Q) for the 2*y*gq term (may be null)
    const double* pa;     // FWD: prologue A[n,k] (null = identity)
    const double* pb;
    const double* gs;    // DGRAD: d/d sum(y)   [n,k]  (may be null)
    const double* gq;    // DGRAD: d/d sum(y^2) [n,k]  (may be null)
    const double* gsc;   // DGRAD: per-(n,k) scale of the incoming gradient: g' = gsc*gy + gs + 2*y*gq  (null = 1)
    const float* w;      // (Cout, Cin) row major
    float* dst;          // FWD: y (N,M,Q)                DGRAD: gx (N,M,Pin)
    const float* ex;     // DGRAD: forward input x raw (N,M,Pin) (needed when ea != null)
    const double* ea;     // DGRAD: forward prologue A[n,m] (null = identity => gx = da)
    const double* eb;
    // DGRAD: optional compact gradient (N, M, T, acc_Ho, acc_Wo) of a second, spatially strided consumer of the same
    // input (the stride-s shortcut conv of a stage's first block): added to W^T g' on the lattice h % s == w % s == 0
    // BEFORE the act' epilogue, so the zero-filled sparse tensor and the dense add kernel never exist
    const float* acc; int acc_s, acc_Ho, acc_Wo;
    double* s1;          // FWD: sum(y) [n,m]             DGRAD: sum(dz*x) [n,m]
    double* s2;          // FWD: sum(y^2)                 DGRAD: sum(dz)
    int N, M, K, Q, Pin, Hi, Wi, Ho, Wo, stride, act;
    int Cin;             // row pitch of w
    int mtiles, nstrips, tpb, kres, Kpad;   // kres: weight rows resident in LDS per pass (multiple of 8)
    // stem != 0: dense convolution as an implicit GEMM -- the B operand is the im2col view of a (N,Cimg,Ti,Hi,Wi)
    // tensor for a (kT,kH,kW) kernel with strides (sT,sH,sW) and zero padding (pT,pH,pW); K = Cimg*kT*kH*kW
    int stem, Cimg, kT, kH, kW, sT, sH, sW, pT, pH, pW, Ti, To;
};

#define PW_UNIT 8        // input channels per pipelined unit (4 MFMA k-steps)
#define PW_KRES_MAX 512  // weight rows kept in LDS at once (K > 512 streams the weights in chunks)

__device__ __forceinline__ float pw_bload(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}


// One launch helper for the pointwise launchers: raises the dynamic-LDS limit where the kernel needs more than 48 KiB, then launches.
template <typename Kern, typename Args>
static inline void cfn_launch(Kern kernel, unsigned blocks, unsigned threads, size_t lds, hipStream_t st, const Args& args) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, st, args);
}

// ---- deciding apart from launching (router: pwroute.hip) --------------------------------------------------------------------------------
// The switches a plan may depend on, read in ONE place (pw_switches_now): CFN_PW_SPLIT once per process (cfn_pw_split_terms changes it later),
// CFN_PWF_SPLIT / CFN_PWF_L3E / CFN_PW_SHORT per call.
struct PwSwitches {
    int split_terms;     // 0 = fp32 MFMA kernels, 3 / 6 = bf16 MFMAs per k-block
    int pwf_split;       // one-pass backward on the split-bf16 pipe: 0 off, 1 = shapes without a prologue, 2 = also with one
    int pwf_l3e;         // layer-3 conv3 one-pass backward (off unless set)
    int pw_short;        // 0 = the strided shortcut's backward as two separate kernels
};
PwSwitches pw_switches_now(bool backward);      // backward = false: split_terms alone (cached; the forward / data-gradient plans use nothing else)
int pws_terms_now();     // split_terms alone, for the families outside the router (salconvb.hip)

enum { PW_FAM_PWK = 1, PW_FAM_PWT, PW_FAM_PWS, PW_FAM_PWD, PW_FAM_GEMM,                 // forward / data gradient
       PW_FAM_PSS, PW_FAM_WD, PW_FAM_WG,                                                // weight gradient: staged split-bf16, direct operand, LDS-staged fp32
       PW_FAM_PF3, PW_FAM_PF3E, PW_FAM_PFS, PW_FAM_PF,                                  // one-pass backward
       PW_FAM_PSH };                                                                    // strided-shortcut backward

// What X_plan decides and X_launch launches.  X_plan is host arithmetic on numbers: no HIP call, no getenv, no allocation; it reads the null-ness of
// the PwArgs pointers, never what they point to.  The caller fills align_io / align_ex before planning.
struct PwPlan {
    unsigned align_io;   // in: low 4 bits of (src | dst | src2)
    unsigned align_ex;   // in: low 4 bits of ex (0 when null)
    int slot;            // position in the router's order: the entry point continues behind it when the launcher returns -1 (no workspace)
    int family, mode, act;            // act: the kernel's ACT template argument
    bool stats, two, lattice_add;     // two: second staged operand (y); lattice_add: pw_lattice_add_kernel behind the contraction
    int MT, NP, NS, KS, nkb;          // template arguments the host selects (0 = not a parameter of this family)
    unsigned blocks, threads;
    size_t lds, ws_bytes;             // ws_bytes: what the launcher asks its workspace for
    PwArgs a;                         // the patched copy the kernel gets (Kpad, kres, mtiles, nstrips, tpb, act)
};

// -1 from a launcher = no workspace (stream capture / out of memory): nothing was launched, the entry point goes on to the next family
bool pwk_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p);      // pwregk.hip: split bf16, register-resident weights
int pwk_launch(const PwPlan& p, hipStream_t st);
bool pwt_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p);      // pwstream.hip: split bf16, weights streamed through LDS
int pwt_launch(const PwPlan& p, hipStream_t st);
bool pws_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p);      // pwsplit.hip: split bf16, weight images resident in LDS
int pws_launch(const PwPlan& p, hipStream_t st);
bool pwd_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p);      // pwdeep.hip: fp32 MFMA, 8 waves, deep weight image
int pwd_launch(const PwPlan& p, hipStream_t st);
bool pw_gemm_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p);  // pwconv.hip: fp32 MFMA, every shape; false = beyond 2 GiB
int pw_gemm_launch(const PwPlan& p, hipStream_t st);

// pwroute.hip: the families' plans in order, first that accepts; from = first slot to consider (0 on the first try)
bool pw_route_fwd(const PwArgs& a, bool stats, const PwSwitches& sw, PwPlan& p, int from);
bool pw_route_dgrad(const PwArgs& a, bool stats, const PwSwitches& sw, PwPlan& p, int from);

// ---- the backward chains: weight gradient, one-pass backward, strided-shortcut backward ----------------------------------------------------
// What their plans see of a call: numbers and presence flags.
struct PwBwdShape {
    int N, Cin, Cout, T, Hi, Wi, stride, act;
    bool pro, two, acc;      // prologue A, B present; y staged (gsumsq and y present); compact shortcut gradient present
    int acc_stride;
    unsigned align_g, align_x, align_out;      // low 4 bits of gy | y (y where the entry point looks at it), of x, of the output (short: da)
};
struct PwBwdPlan {
    int slot, family, variant;      // variant: the launcher's index of the template instance
    int t[8];                       // the template arguments the host selects, in the family's order (see each X_plan)
    int act, vec;                   // ACT template argument (-1: no act' epilogue); short: vector width class of the loads
    bool two;
    unsigned blocks, threads;
    size_t lds, ws_bytes;           // ws_bytes: what the launcher asks its workspace for (pss: 0 = fp64 atomics)
    int stages, nstrips, per, mgroups, kgroups, mtg, ktg;      // what the launcher patches into the kernel's arguments
};
bool pws_wgrad_plan(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p);      // pwsplitw.hip: staged split-bf16 weight gradient (stride 1, M, K >= 48)
int pws_wgrad_launch(const PwBwdPlan& p, const float* gy, const float* y, const double* gs, const double* gq, const double* gsc, const float* x,
                     const double* pa, const double* pb, int act, double* gw, int N, int M, int K, int Q, hipStream_t st);
bool pwd_wgrad_plan(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p);      // pwwgrad.hip: direct-operand weight gradient (stride 1: M, K >= 48; stride 2)
int pwd_wgrad_launch(const PwBwdPlan& p, const float* gy, const float* y, const double* gs, const double* gq, const double* gsc, const float* x,
                     const double* pa, const double* pb, int act, double* gw, int N, int M, int K, int T, int Hi, int Wi, int stride, hipStream_t st);
bool pw_wg_plan(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p);          // pwconv.hip: LDS-staged fp32 weight gradient, every shape
bool pwfs_plan(const PwBwdShape& s, const PwSwitches& sw, int which, PwBwdPlan& p);   // pwfuseds.hip: one-pass backward, split bf16 (which: PF3 / PF3E / PFS)
int pwfs_launch(const PwBwdPlan& p, const float* gy, const float* y, const double* gsum, const double* gsumsq, const float* w, const float* x, const double* A,
                const double* B, int act, float* gx, double* gA, double* gB, double* gw, int N, int Cin, int Cout, int T, int Hi, int Wi,
                const float* acc, int acc_stride, const double* gscale, hipStream_t st);
bool pf_plan(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p);             // pwfused.hip: one-pass backward, fp32 (layer-1 widths)
bool psh_plan(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p);            // pwshort.hip: strided-shortcut backward
bool pw_route_wgrad(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p, int from);
bool pw_route_fused(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p, int from);      // false: cfn_pwconv_bwd_fused returns -1
bool pw_route_short(const PwBwdShape& s, const PwSwitches& sw, PwBwdPlan& p);                // false: cfn_pwconv_short_bwd returns -1

// the LDS-staged weight gradient of pwsplitw.hip on bf16 tensors (one bf16 term per operand); -1 = not handled
int pwss_wgrad_try_bf16(const uint16_t* gy, const uint16_t* y, const double* gs, const double* gq, const double* gsc, const uint16_t* x,
                        const double* pa, const double* pb, int act, double* gw, int N, int M, int K, int Q, hipStream_t st);

// ---- dense convs (stem, saliency): the plans live in dense_plan.h, the launchers below call them ---------------------------------------------
#include "dense_plan.h"

// pwwgrad.hip: the direct-operand weight gradient of a dense conv (stem, saliency); -1 = shape not handled
int pwd_wgrad_try_dense(const float* gy, const float* y, const double* gs, const double* gq, const float* x, const double* pa,
                        const double* pb, int act, double* gw, int N, int M, int Cimg, int T, int Hi, int Wi, const int* g,
                        hipStream_t st);

// stem.hip: LDS-tiled forward of the 1x3x3 stride-(1,2,2) stem conv (Cimg == 3, Cout <= 32, Wi % 4 == 0, Hi even); -1 = not handled
int stem_fwd_try_launch(const float* x, const float* w, float* y, int N, int Cimg, int Cout, int T, int Hi, int Wi, hipStream_t st);
int stem_wgrad_try_launch(const float* gy, const float* x, double* gw, int N, int Cimg, int Cout, int T, int Hi, int Wi, hipStream_t st, bool probe);

// salconv.hip: LDS-tiled fp32-MFMA kernels for the Grid Pool saliency convs (Cin == 24, Cout <= 32, 3x3x3, stride 2, pad 1, input
// planes 56 or 28 wide, even height); -1 = not handled
int sal_fwd_try_launch(const float* x, const double* A, const double* B, int act, const float* w, float* y, double* sum,
                       double* sumsq, int N, int Cin, int Cout, int T, int Hi, int Wi, const int* g, hipStream_t st);
// salconvb.hip: the forward of the same shapes on the split-bf16 matrix pipe (6 bf16 MFMAs per k-block, fp32-accurate); -1 = not handled / switched off
int salb_fwd_try_launch(const float* x, const double* A, const double* B, int act, const float* w, float* y, double* sum,
                        double* sumsq, int N, int Cin, int Cout, int T, int Hi, int Wi, const int* g, hipStream_t st);
int sal_wgrad_try_launch(const float* gy, const float* y, const double* gs, const double* gq, const float* x, const double* A,
                         const double* B, int act, double* gw, int N, int Cin, int Cout, int T, int Hi, int Wi, const int* g,
                         hipStream_t st);
