// Dense 3-D convs (Grid Pool saliency convs, stem conv1_s, generic shapes): what a plan sees of a call and what it decides.  Host arithmetic
// only.  Every family's X_plan sits next to its kernel and holds its shape gates and its chunk / grid arithmetic; the launcher of the family
// and the host-only query cfn_conv3d_dense_route (denseroute.hip) both call it, so the decision exists once.
#pragma once
#include "cfn_common.h"

struct DenseShape {
    int N, Cin, Cout, T, Hi, Wi;
    int g[9];                  // kT, kH, kW, sT, sH, sW, pT, pH, pW
    int act;                   // the prologue's activation (CFN_ACT_NONE without a prologue)
    bool pro, stats, gs, y;    // prologue A, B present; forward: sum / sumsq asked for; backward: gsum present; gsumsq and y present
    unsigned align_x, align_g, align_out;      // low 4 address bits of x, of gy | y (y where the entry point looks at it), of the output (y, gx)
    bool u8;                   // the stem plans: x is uint8 frames (N, T, H, W, 3), decoded through a table while they are staged
};

enum { DN_SALB = 1, DN_SAL_FWD, DN_SAL_DGRAD, DN_SAL_WGRAD, DN_ALLCI, DN_PERCH, DN_GEMM, DN_WD, DN_WG, DN_STEM_FWD, DN_STEM_WGRAD, DN_STEM_U8_FWD,
       DN_STEM_U8_WGRAD };

struct DensePlan {
    int family;
    int v[4];                  // the template arguments the host selects, in the family's order (see each X_plan)
    unsigned grid[3], wg;
    size_t lds;
    // the sal kernels: bands of output rows, chunk length (forward: output frames TO; data gradient: input frame pairs CH; weight gradient:
    // output frames CH), number of chunks, length of the last one, work items (forward: workgroups; data gradient: half-workgroup groups;
    // weight gradient: items of the persistent loop).  stem_wgrad, stem_u8_wgrad: items, chunk = items per workgroup.  stem_fwd, stem_u8_fwd: bands, chunk = RB
    int bands, chunk, nchunks, last, items;
};

static const int kStemGeom[9] = {1, 3, 3, 1, 2, 2, 0, 1, 1};      // conv1_s

inline DenseShape dense_shape(int N, int Cin, int Cout, int T, int Hi, int Wi, const int* g, int act) {
    DenseShape s = {N, Cin, Cout, T, Hi, Wi};
    for (int i = 0; i < 9; ++i) s.g[i] = g[i];
    s.act = act;
    return s;
}

// cfn_conv3d_dense_bwd_data asks this of every call: the per-channel kernel puts (sample, input channel) on grid.y
inline bool dense_dgrad_fits(int N, int Cin) { return (long)N * Cin <= 65535; }

// CUs of the current device; 256 where there is none
inline int dense_cu_count() {
    int dev = 0; hipDeviceProp_t pr;
    return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) ? pr.multiProcessorCount : 256;
}

// what all four sal kernels ask of a call: 24 input channels, 3x3x3 stride 2 pad 1, planes 56 or 28 wide and of even height, ReLU prologue or none
inline bool sal_common_ok(const DenseShape& s) {
    static const int want[9] = {3, 3, 3, 2, 2, 2, 1, 1, 1};
    for (int i = 0; i < 9; ++i) if (s.g[i] != want[i]) return false;
    if (s.Cin != 24 || (s.Wi != 56 && s.Wi != 28) || (s.Hi & 1) || s.Hi < 2) return false;
    return s.pro ? s.act == CFN_ACT_RELU : s.act == CFN_ACT_NONE;
}

// chunk length of the two forward kernels: whole rounds of two workgroups per CU where possible (a 1.25-round grid costs a full second round)
inline int sal_fwd_chunk(int N, int bands, int To, int cus) {
    int best = 4; double bestc = 1e30;
    for (int to = 2; to <= 16; ++to) {
        const long blocks = (long)N * bands * cfn_cdiv(To, to);
        const double rounds = (double)cfn_cdiv(blocks, (long)cus * 2);
        const double cost = rounds * (3.0 * to + 1.0);          // MFMA sets per block: 3 per output frame + the halo frame's one
        if (cost < bestc - 1e-9) { bestc = cost; best = to; }
    }
    return best;
}

// cus: CUs to plan for; <= 0 = those of the current device, asked only once the shape gates have passed.  false = not handled
bool salb_fwd_plan(const DenseShape& s, int cus, DensePlan& p);        // salconvb.hip  v = {WI, PRO}
bool sal_fwd_plan(const DenseShape& s, int cus, DensePlan& p);         // salconv.hip   v = {WI, NT, PRO}
bool sal_dgrad_plan(const DenseShape& s, int cus, DensePlan& p);       //               v = {WI, PRO, HASY}
bool sal_wgrad_plan(const DenseShape& s, int cus, DensePlan& p);       //               v = {WI, PRO, HASY}
bool dense_dgrad_plan(const DenseShape& s, DensePlan& p);              // fusion.hip    all-channel (v = {CI}) or per-channel kernel; false: too large
bool dense_gemm_plan(const DenseShape& s, DensePlan& p);               // pwconv.hip    v = {MT, mode, STATS, ACT}; false: beyond the descriptor range
bool dense_wg_plan(const DenseShape& s, DensePlan& p);                 // pwconv.hip    v = {MTW, NTW}
bool dense_wd_plan(const DenseShape& s, DensePlan& p);                 // pwwgrad.hip   v = {ACT, 2, TM, TN}
bool stem_fwd_plan(const DenseShape& s, DensePlan& p);                 // stem.hip      v = {3}; s.u8: the uint8 family (launched by stem_u8.hip)
bool stem_wgrad_plan(const DenseShape& s, int cus, DensePlan& p);      // stem.hip; cus < 0: the shape gates only; s.u8 as above
