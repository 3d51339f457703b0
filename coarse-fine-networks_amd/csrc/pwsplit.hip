// Host side of the split-bf16 pointwise contractions with RESIDENT weight images (kernel: pws_kernel.h; the weight-streaming launcher for
// the deep contractions of layer 4 is pwstream.hip).
#include "pws_kernel.h"

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static size_t pws_lds(int BM, int Kp, int rowb, int NS) {
    const size_t red = (size_t)PWS_WAVES * 4 * (BM * 2 > 32 * 20 ? BM * 2 : 32 * 20);
    return (size_t)NS * BM * rowb + (size_t)Kp * 16 + (size_t)BM * 8 + red;
}

template <int MODE, bool STATS, int ACT, bool TWO, int NS>
static int pws_go_mt(const PwPlan& p, hipStream_t st) {
#define PWS_GO(MTV, NPV) cfn_launch(pws_kernel<MTV, NPV, MODE, STATS, ACT, TWO, NS>, p.blocks, p.threads, p.lds, st, p.a)
    // pws_plan reaches exactly these tiles.  64 positions (NP = 2): one slab of more than 32 rows, or two slabs of more than
    // 32 * mt2 rows together, so MT >= 2.  32 positions (NP = 1) are chosen only where they save a slab over NP = 2: with one staged tensor
    // that takes more than 96 rows (MT >= 4), with two more than 64 (MT >= 3).
    const int MT = p.MT;
    if (p.NP == 1) {      // 32-position tiles: the many-row slabs
        if constexpr (MODE == PW_DGRAD && TWO) {
            switch (MT) { case 3: PWS_GO(3, 1); break; case 4: PWS_GO(4, 1); break; case 5: PWS_GO(5, 1); break; default: PWS_GO(6, 1); break; }
        } else {
            switch (MT) { case 4: PWS_GO(4, 1); break; case 5: PWS_GO(5, 1); break; case 6: PWS_GO(6, 1); break; default: PWS_GO(7, 1); break; }
        }
    } else if constexpr (MODE == PW_DGRAD && TWO) {
        PWS_GO(2, 2);
    } else {
        if (MT == 2) PWS_GO(2, 2); else PWS_GO(3, 2);
    }
#undef PWS_GO
    return cfn_check_launch("pwconv(split bf16)");
}

template <int MODE, bool STATS, bool TWO, int NS>
static int pws_go_act(const PwPlan& p, hipStream_t st) {
    if constexpr (MODE == PW_DGRAD && !STATS) {
        return pws_go_mt<MODE, STATS, CFN_ACT_NONE, TWO, NS>(p, st);
    } else {
        switch (p.act) {
            case CFN_ACT_RELU: return pws_go_mt<MODE, STATS, CFN_ACT_RELU, TWO, NS>(p, st);
            case CFN_ACT_SWISH: return pws_go_mt<MODE, STATS, CFN_ACT_SWISH, TWO, NS>(p, st);
            default: return pws_go_mt<MODE, STATS, CFN_ACT_NONE, TWO, NS>(p, st);
        }
    }
}

template <int NS>
static int pws_go(const PwPlan& p, hipStream_t st) {
    if (p.mode == PW_FWD) return p.stats ? pws_go_act<PW_FWD, true, false, NS>(p, st) : pws_go_act<PW_FWD, false, false, NS>(p, st);
    if (p.two) return p.stats ? pws_go_act<PW_DGRAD, true, true, NS>(p, st) : pws_go_act<PW_DGRAD, false, true, NS>(p, st);
    return p.stats ? pws_go_act<PW_DGRAD, true, false, NS>(p, st) : pws_go_act<PW_DGRAD, false, false, NS>(p, st);
}

// false when the shape is not handled (the fp32-MFMA kernels take it).
// FWD prologue: pa == nullptr means A = 1, B = 0 (act still applies, as in the fp32-MFMA kernels); DGRAD: stats == (ea != nullptr)
bool pws_plan(const PwArgs& a, int mode, bool stats, const PwSwitches& sw, PwPlan& p) {
    const int terms = sw.split_terms;
    if (terms == 0) return false;
    // (why K <= 128, M > 32 and no `acc`: the table of pwroute.hip)
    if (a.stem || a.stride != 1 || a.K < 48 || a.M <= 32 || (a.Q & 3) || a.acc) return false;      // Q % 4: whole 16-byte groups
    if (a.act != CFN_ACT_NONE && a.act != CFN_ACT_RELU && a.act != CFN_ACT_SWISH) return false;
    if (a.K > 128) return false;
    if ((long)a.K * a.Q * 4 >= 0x3ffffff0L || (long)a.M * a.Q * 4 >= 0x3ffffff0L) return false;
    if ((p.align_io | p.align_ex) & 15) return false;
    const int NS = terms == 3 ? 2 : 3;
    PwArgs& b = p.a;
    b = a;
    b.Kpad = (a.K + 47) / 48 * 48;
    b.kres = b.Kpad * 2 + 16;
    if (((b.kres / 16) & 1) == 0) b.kres += 16;                          // odd number of 16-byte slots per row
    if (mode == PW_DGRAD && !stats) b.act = CFN_ACT_NONE;
    // rows per slab, limited by registers (accumulators + the 3-set operand ring; measured with -Rpass-analysis: the next size
    // spills 50-230 bytes per lane).  64-position tiles (NP = 2): 96 rows forward, 96 / 64 backward (one / two staged tensors).
    // 32-position tiles (NP = 1): 224 rows, 192 backward with two staged tensors.  The NS weight images of a slab must fit
    // LDS.  Fewer slabs win (every extra slab re-reads the activations), then the wider tile.
    auto fit = [&](int mt) { while (mt > 0 && pws_lds(32 * mt, b.Kpad, b.kres, NS) > 160 * 1024) --mt; return mt; };
    const int mt2 = fit(mode == PW_FWD ? 3 : (a.src2 ? 2 : 3)), mt1 = fit(mode == PW_DGRAD && a.src2 ? 6 : 7);
    if (mt2 < 1) return false;
    int NP = 2, mt_max = mt2;
    if (mt1 >= 3 && cfn_cdiv(a.M, 32 * mt1) < cfn_cdiv(a.M, 32 * mt2)) { NP = 1; mt_max = mt1; }
    int slabs = cfn_cdiv(a.M, 32 * mt_max);
    const int per = cfn_cdiv(a.M, slabs);
    int MT = cfn_cdiv(per, 32);
    if (NP == 1 && MT < 3) MT = 3;
    slabs = cfn_cdiv(a.M, 32 * MT);
    // three or more slabs (X3D layer 4: the weight images of 432 x 192 do not fit LDS in fewer) re-read every activation that
    // often: measured slower than the fp32-MFMA kernel with its 4-byte weight image (0.19-0.31 vs 0.20-0.24 ms) -- declined
    if (slabs > 2) return false;
    b.mtiles = slabs;
    const int ntiles = cfn_cdiv(a.Q, 32 * NP);
    const long groups = (long)a.N * slabs;
    long wgs = cfn_cdiv(256, groups);              // one 8-wave workgroup per CU (up to 256 VGPRs)
    const long maxw = cfn_cdiv(ntiles, PWS_WAVES);
    if (wgs > maxw) wgs = maxw;
    if (wgs < 1) wgs = 1;
    b.nstrips = (int)wgs;
    p.family = PW_FAM_PWS; p.mode = mode; p.stats = stats; p.two = a.src2 != nullptr; p.act = b.act;
    p.MT = MT; p.NP = NP; p.NS = NS;
    p.blocks = (unsigned)(groups * wgs); p.threads = 64 * PWS_WAVES; p.lds = pws_lds(32 * MT, b.Kpad, b.kres, NS);
    return true;
}

int pws_launch(const PwPlan& p, hipStream_t st) { return p.NS == 2 ? pws_go<2>(p, st) : pws_go<3>(p, st); }
