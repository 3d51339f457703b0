"""fp64 references of the Multi-stage Fusion kernels of csrc/fusion.hip -- gauss_align (fwd, bwd) and fusion_gather (fwd tiled <4,13|9|8> and
one-output, bwd_x, bwd_w tiled <8,8> and one-output, bwd_reduce) -- in plain torch on the CPU (test infrastructure), and the inputs of the
cases tests/test_hip_fusion.py runs them at.  Res, bound() and ratio() are the ones of tests/temporal_ref64.py; where an error is a
composition of several kernels' errors the reference returns the bound tensor itself: Bnd(val, bnd), judged by worst().  u = 2^-24.

fusion_gather.  Everything in fp64 from the fp32 inputs (the expression of x3d_coarse.py:209-223, crop repeat r = b * crops + j):
    at = sigmoid(at_raw + bias), w[r,t,k,p] = at[b,t,p] GX[r,t,k] mask[b,t], den = sum_t w + 1e-6, z = sum_t x w / den.
Roundings, counted in the kernel text (FL = 2^-126 is an underflow allowance on `at`: a logit below -87 gives a sigmoid under the fp32
normal range, which a kernel may flush to zero; it is multiplied by what multiplies `at` in the output, the mask included):
    den   Tf additions of positive terms (+1e-6 among them); per term the sigmoid (expf, an addition, a reciprocal: <= 4u relative) and
          the two products of w:  (Tf + 16) u den + FL sum_t GX mask
    z     num: Tf FMAs, den: as above, one division; A = sum_t |x| w:  (2 Tf + 16) u A / den + FL sum_t (|x| + |z|) GX mask / den
    dw    dw[r,t,k,p] = sum_c gz (x - z) / den (the scratch tensor of cfn_fusion_gather_bwd): C FMAs, one subtraction each, 1 / den and the
          product; the kernel subtracts its own fp32 z, which carries z's bound:  n = C + 2 Tf, slack 16,
          mag = sum_c |gz| (|x| + A_c / den) / den
    gx    gx[b,c,t,p] = at mask sum_{j,k} (gz / den) GX: crops K FMAs of a quotient by the kernel's den, times mask / (1 + expf):
          n = crops K + 2 Tf, slack 16, mag = at mask sum_{j,k} |gz / den| GX (+ FL mask sum |gz / den| GX).  mask = 0: exact zero
    gat   at (1 - at) mask sum_{j,k} dw GX: the dw bound contracted with the same non-negative weights + (crops K + 8) u times the
          contraction of |dw|.  ONE term beyond the issue's count: 1 - a is taken from the kernel's fp32 a, whose own error (<= 4u a) does
          not shrink with 1 - a, so the slope a (1 - a) is off by up to 6u at in absolute terms: + 6u at mask |sum dw GX| (a logit of 8
          has 1 - a = 3e-4: without the term plain fp32 torch leaves the bound as well).  mask = 0: exact zero
    gGX   mask sum_p dw at: the dw bound contracted with at + (P + 8) u sum_p |dw| at (+ FL mask sum_p |dw|).  mask = 0: exact zero
    gb    gat.sum(), torch's reduction of the kernel's gat (it nearly cancels: never held relative to |gb|):
          sum of the gat bounds + (log2(B Tf P) + 8) u sum |gat|

gauss_align.  Everything in fp64 from the fp32 inputs, mu included; the one integer decision is the argmax frame (the FIRST maximal frame).
The inputs make it unambiguous: frac(mu) is exactly 0.5 (built from values exact in fp32) or at least 2^-10 away from it (ga_margin_ok).
    GX    with d = t - mu, den = 2 std^2 + 1e-16, a = d^2 / den, s = |2 d / den|, m the argmax frame, dn = f_m + 1e-16:
          |err| <= [(4 a + 4 a_m + 16) u + (s + s_m) dmu] GX + 2^-126 / dn,   dmu = 3u (|tl| + |st|) / |ratio|
          (the expf argument known to 4u, the rounding of mu, and an allowance for exp results under the fp32 normal range)
    ggx   measured, not derived: kernel error <= 4 x (error of the same expression in plain fp32 torch on the CPU) + 2^-23, both relative
          to the tensor's max (the rule of grid_cdf and the bn_fold gate); a knot whose gGX column is all zero gets an exact zero

dtype=torch.float32 evaluates the same expressions the way a plain fp32 implementation would.  mutant names ONE deliberate error (MUTANTS):
a mutated fp64 result must leave the bound of every case that names it (tests/test_fusion_ref64_cpu.py)."""
import collections
import functools
import math

import torch

from temporal_ref64 import Res, bound, ratio, maxrel, U24, _seed      # noqa: F401  (bound, maxrel: for the tests)

FL = 2.0 ** -126
SLACK = 16
Bnd = collections.namedtuple('Bnd', 'val bnd')

MUTANTS = {
    'fusion_gather': ('crop0_GX', 'no_mask', 'no_eps', 'drop_last_ktile', 'drop_last_channel_block', 'x_minus_z_sign', 'den_once',
                      'gat_no_sigmoid_slope', 'gGX_first_p_only'),
    'gauss_align': ('crop0_start', 'argmax_last', 'ratio_ignored', 'std_from_Tf'),
}


def worst(got, b):
    """ratio() of temporal_ref64 against an explicit bound tensor: (0 + 8) u * (bnd * 2^21) is bnd exactly"""
    val = b.val.double()
    return ratio(got, Res(val, torch.zeros_like(val), (b.bnd.double() * 2.0 ** 21).expand_as(val)))


def _bnd(val, n, mag, extra=None):
    b = (float(n) + SLACK) * U24 * mag.double()
    return Bnd(val.double(), (b if extra is None else b + extra.double()).expand_as(val))


# ---- fusion_gather ------------------------------------------------------------------------------------------------------------------------
def fwd_ktile(K):
    """the k tile cfn_fusion_gather_fwd picks: the one of 13, 9, 8 that wastes the fewest slots (ties to the larger)"""
    w13, w9, w8 = -(-K // 13) * 13 - K, -(-K // 9) * 9 - K, -(-K // 8) * 8 - K
    return 13 if (w13 <= w9 and w13 <= w8) else (9 if w9 <= w8 else 8)


def fusion_gather_ref64(x, at_raw, bias, GX, mask, gz, crops, dtype=torch.float64, mutant=None):
    """x (B, C, Tf, P), at_raw (B, Tf, P), bias (1,) or None, GX (B * crops, Tf, K), mask (B, Tf), gz (B * crops, C, K, P) ->
    {'z', 'den', 'dw', 'gx', 'gat', 'gGX', 'gb' (None without a bias): Bnd}"""
    assert mutant is None or mutant in MUTANTS['fusion_gather'], mutant
    B, C, Tf, P = x.shape
    R, _, K = GX.shape
    assert R == B * crops
    d = lambda v: v.detach().to(dtype)
    rep = lambda v: v.repeat_interleave(crops, 0)
    xs, gzs, mk, G = d(x), d(gz), d(mask), d(GX)
    if mutant == 'no_mask':
        mk = torch.ones_like(mk)
    if mutant == 'crop0_GX':
        G = G.view(B, crops, Tf, K)[:, :1].expand(B, crops, Tf, K).reshape(R, Tf, K)
    at = torch.sigmoid(d(at_raw) if bias is None else d(at_raw) + d(bias))                    # B Tf P
    xr, atr, mr = rep(xs), rep(at), rep(mk)
    gm = G * mr.unsqueeze(2)                                                                   # R Tf K    GX mask
    w = atr.unsqueeze(2) * gm.unsqueeze(3)                                                     # R Tf K P
    den = w.sum(1) + (0.0 if mutant == 'no_eps' else 1e-6)                                     # R K P
    z = torch.einsum('rctp,rtkp->rckp', xr, w) / den.unsqueeze(1)
    A = torch.einsum('rctp,rtkp->rckp', xr.abs(), w)
    Aq = A / den.unsqueeze(1)
    gmsum = gm.sum(1).unsqueeze(2)                                                             # R K 1
    out = {'den': _bnd(den, Tf, den, FL * gmsum),
           'z': _bnd(z, 2 * Tf, Aq, FL * (torch.einsum('rctp,rtk->rckp', xr.abs(), gm) + z.abs() * gmsum.unsqueeze(1)) / den.unsqueeze(1))}

    gzd = gzs / den.unsqueeze(1)                                                               # R C K P
    gzw = gzs if mutant == 'den_once' else gzd
    sgn = -1.0 if mutant == 'x_minus_z_sign' else 1.0
    dw = torch.einsum('rckp,rctp->rtkp', gzw, xr) - sgn * (gzw * z).sum(1).unsqueeze(1)        # R Tf K P
    dwmag = torch.einsum('rckp,rctp->rtkp', gzd.abs(), xr.abs()) + (gzd.abs() * Aq).sum(1).unsqueeze(1)
    out['dw'] = _bnd(dw, C + 2 * Tf, dwmag)
    dwb, dwa = out['dw'].bnd, dw.abs()

    mk4 = mk.view(B, 1, Tf, 1)
    fold = lambda v: v.reshape((B, crops) + tuple(v.shape[1:])).sum(1)                         # the sum over the crops of a video
    S = fold(torch.einsum('rckp,rtk->rctp', gzd, G))
    Sa = fold(torch.einsum('rckp,rtk->rctp', gzd.abs(), G.abs()))
    out['gx'] = _bnd(at.unsqueeze(1) * mk4 * S, crops * K + 2 * Tf, at.unsqueeze(1) * mk4 * Sa, FL * mk4 * Sa)

    slope = torch.ones_like(at) if mutant == 'gat_no_sigmoid_slope' else at * (1 - at)
    mk3 = mk.unsqueeze(2)
    Cd = fold(torch.einsum('rtkp,rtk->rtp', dw, G))
    Cb = fold(torch.einsum('rtkp,rtk->rtp', dwb.to(dtype), G.abs()))
    Ca = fold(torch.einsum('rtkp,rtk->rtp', dwa, G.abs()))
    gat = slope * mk3 * Cd
    gatb = (slope * mk3).double() * (Cb.double() + (crops * K + 8) * U24 * Ca.double()) \
        + 6 * U24 * (at * mk3 * Cd.abs()).double() + FL * (mk3 * Ca).double()
    out['gat'] = Bnd(gat.double(), gatb)

    mr3 = mr.unsqueeze(2)
    if mutant == 'gGX_first_p_only':
        gGX = mr3 * (dw[..., 0] * atr[..., :1])
    else:
        gGX = mr3 * torch.einsum('rtkp,rtp->rtk', dw, atr)
    gGXb = mr3.double() * (torch.einsum('rtkp,rtp->rtk', dwb, atr.double()) + (P + 8) * U24 * torch.einsum('rtkp,rtp->rtk', dwa, atr).double()) \
        + FL * (mr3 * dwa.sum(3)).double()
    out['gGX'] = Bnd(gGX.double(), gGXb)
    out['gb'] = None if bias is None else Bnd(gat.sum().double().view(1),
                                              (gatb.sum() + (math.log2(B * Tf * P) + 8) * U24 * gat.abs().sum().double()).view(1))
    if mutant == 'drop_last_ktile':                     # what a skipped last k tile leaves behind (zeros): forward tile, backward tile 8
        kf, kb = fwd_ktile(K) * (K // fwd_ktile(K)), 8 * (K // 8)
        zz, dd, ww = out['z'].val.clone(), out['den'].val.clone(), out['dw'].val.clone()
        zz[:, :, kf:], dd[:, kf:], ww[:, :, kb:] = 0, 0, 0
        out.update(z=Bnd(zz, out['z'].bnd), den=Bnd(dd, out['den'].bnd), dw=Bnd(ww, out['dw'].bnd))
    if mutant == 'drop_last_channel_block':             # channels of the last block of (256 // P) * 4 (P <= 256)
        per = (256 // P) * 4
        zz = out['z'].val.clone()
        zz[:, (-(-C // per) - 1) * per:] = 0
        out['z'] = Bnd(zz, out['z'].bnd)
    return out


# ---- gauss_align --------------------------------------------------------------------------------------------------------------------------
def gaussian_expr(meta, mask, gx, tx, ratio_=1, dtype=torch.float32):
    """oracle.x3d_ref.gaussian (x3d_coarse.py:256-286) with the dtype given instead of hard-coded float32; differentiable in gx"""
    st, step = meta[:, 0], meta[:, 3]
    b, b2, len_f = meta.shape[0], gx.shape[0], mask.shape[1]
    st = st.to(dtype)
    if b2 != b:
        off = step.view(-1, 1) * torch.arange(0, b2 // b).to(dtype).view(1, -1).repeat(b, 1)
        st = (st.view(-1, 1).repeat(1, b2 // b) + off).view(-1, 1)
    if tx is not None:
        len_x = gx.shape[1]
        tl = (gx * tx).unsqueeze(1)
    else:
        len_x = gx.shape[2]
        tl = torch.arange(0, len_x).to(dtype).view(1, 1, -1).repeat(b2, 1, 1)
    mu = (tl + st.view(b2, 1, 1)) / ratio_
    t = torch.arange(0, len_f).to(dtype).view(1, -1, 1).repeat(b2, 1, 1)
    std = (1 / 8 * torch.sum(mask, dim=1)).view(-1, 1).repeat(1, b2 // b).view(-1, 1)
    t = t - mu
    f = t ** 2 / (2 * (std ** 2).view(b2, 1, 1).repeat(1, len_f, len_x) + 1e-16)
    f = torch.exp(-f)
    f = f / (torch.max(f, dim=1)[0].view(b2, 1, len_x) + 1e-16)
    return f.view(b2, len_f, len_x)


def gauss_align_ref64(meta, mask, gx, tx, ratio_, crops, K, gGX=None, dtype=torch.float64, mutant=None):
    """meta (B, 4) int64, mask (B, Tf), gx (B * crops, K) or None (tl = k), gGX (B * crops, Tf, K) or None ->
    {'GX': Bnd, 'ggx': tensor of dtype or None, 'mu': (R, K), 'tm': int64 (R, K) the argmax frame, 'f': (R, Tf, K)}"""
    assert mutant is None or mutant in MUTANTS['gauss_align'], mutant
    B, Tf = mask.shape
    R = B * crops
    crop = torch.arange(crops).to(dtype).view(1, crops)
    st = meta[:, 0:1].to(dtype) + (0 if mutant == 'crop0_start' else meta[:, 3:4].to(dtype) * crop)
    st = st.expand(B, crops).reshape(R, 1)
    txv = 1.0 if tx is None else float(tx)
    tl = torch.arange(K).to(dtype).view(1, K).expand(R, K) if gx is None else gx.detach().to(dtype) * txv
    rt = 1.0 if mutant == 'ratio_ignored' else float(ratio_)
    mu = (tl + st) / rt
    nvalid = torch.full((B,), float(Tf), dtype=dtype) if mutant == 'std_from_Tf' else mask.detach().to(dtype).sum(1)
    std = (nvalid * 0.125).repeat_interleave(crops).view(R, 1, 1)
    den = 2 * (std * std) + 1e-16
    t = torch.arange(Tf).to(dtype).view(1, Tf, 1)
    dd = t - mu.unsqueeze(1)                                               # R Tf K
    a = dd * dd / den
    f = torch.exp(-a)
    m = f.max(1)[0]
    eq = f == m.unsqueeze(1)
    if mutant == 'argmax_last':
        pick = eq & (eq.flip(1).cumsum(1).flip(1) == 1)
    else:
        pick = eq & (eq.cumsum(1) == 1)                                    # the first maximal frame
    tm = (pick.long() * torch.arange(Tf).view(1, Tf, 1)).sum(1)
    at_m = lambda v: (v * pick.to(v.dtype)).sum(1)
    dn = m + 1e-16
    GXv = f / dn.unsqueeze(1)
    s = (2 * dd / den)                                                     # df/dmu = f s
    dmu = 3 * U24 * (tl.abs() + st.abs()).double() / abs(rt)
    a64, s64 = a.double(), s.abs().double()
    bnd = ((4 * a64 + 4 * at_m(a64).unsqueeze(1) + 16) * U24 + (s64 + at_m(s64).unsqueeze(1)) * dmu.unsqueeze(1)) * GXv.double() \
        + FL / dn.double().unsqueeze(1)
    out = {'GX': Bnd(GXv.double(), bnd), 'ggx': None, 'mu': mu, 'tm': tm, 'f': f}
    if gGX is not None and gx is not None:
        g = gGX.detach().to(dtype)
        gmu = ((g / dn.unsqueeze(1)) * f * s).sum(1) - ((g * f).sum(1) / (dn * dn)) * m * at_m(s)
        out['ggx'] = gmu / rt * txv
    return out


def ga_margin_ok(mu):
    """every mu has frac(mu) exactly 0.5 (a designated tie) or at least 2^-10 away from it: the argmax frame is the same in any precision"""
    fr = (mu.double() - torch.floor(mu.double()) - 0.5).abs()
    return bool(((fr == 0) | (fr >= 2.0 ** -10)).all())


# ==== the cases of tests/test_hip_fusion.py (inputs on the CPU, shared, never modified) =======================================================
# (B, crops, C, Tf, K, P) -> what the shape reaches
FG_SHAPES = {
    (2, 1, 5, 7, 5, 49): 'KT = 8 ragged; C = 5: the clamped channel pointer, idle channel groups; 2 backward tiles < G = 5 (r >= rows)',
    (1, 2, 24, 9, 17, 49): 'KT = 9, two k groups; cblocks = 2, crops = 2; Tf = 9: tgroups = 2, kgroups = 3 (each with a one-wide last group)',
    (1, 1, 4, 3, 65, 49): 'KT = 13 exact (the T = 256 instance)',
    (1, 1, 4, 3, 20, 49): 'K = 20: the launch rule picks KT = 8 here (waste 4 against 6 for 13), three tiles, the last of 4',
    (1, 1, 4, 3, 25, 49): 'KT = 13 ragged: two tiles, the last of 12 (K = 12, 25, 38 are the ragged sizes that pick 13)',
    (3, 2, 9, 4, 3, 1): 'P = 1, G = 256',
    (1, 1, 3, 2, 2, 256): 'G = 1, no idle lane',
    (1, 1, 6, 3, 4, 100): 'G = 2, 56 idle lanes',
    (1, 2, 3, 5, 4, 260): 'P > 256: both one-output kernels, two rounds of the reduce kernel\'s p += 256 loop',
}
FG_KTILE = {5: 8, 17: 9, 65: 13, 20: 8, 25: 13, 3: 8, 2: 8, 4: 8}
# regimes: 'oracle' mixed-sign x, logits of scale 3, bias 0.3, GX from oracle.x3d_ref.gaussian with knots k % 5 in (1, 3) far outside the
# window, the last video's last two frames masked (Tf >= 4); 'masked' the same behind a fully masked video (B + 1 videos: the dead one is
# b = 0); 'sat' a tenth of the logits at +-100; 'nobias' at_bias = None; 'bias' another tensor bias (-1.5)
FG_REGIMES = ('oracle', 'masked', 'sat', 'nobias', 'bias')
FG_CASES = [(s, r) for s in FG_SHAPES for r in FG_REGIMES if r == 'oracle' or s[5] == 49]
FG_KEYS = ('z', 'den', 'dw', 'gx', 'gat', 'gGX', 'gb')


def fg_mutants(shape, regime):
    """the mutants the inputs of a case can show: crop0_GX needs crops > 1; no_eps a den near 1e-6 (every case has an outside knot);
    drop_last_ktile a ragged tile forward or backward; drop_last_channel_block more than one block; gGX_first_p_only P > 1"""
    B, crops, C, Tf, K, P = shape
    m = ['no_eps', 'x_minus_z_sign', 'den_once', 'gat_no_sigmoid_slope']
    if crops > 1:
        m.append('crop0_GX')
    if Tf >= 4 or regime == 'masked':
        m.append('no_mask')
    if K % fwd_ktile(K) or K % 8:
        m.append('drop_last_ktile')
    if P <= 256 and C > (256 // P) * 4:
        m.append('drop_last_channel_block')
    if P > 1:
        m.append('gGX_first_p_only')
    return tuple(m)


def _oracle_GX(mask, crops, K, gen):
    """GX (B * crops, Tf, K) fp32 from the oracle's gaussian: mu uniform in [-1, Tf], knots k % 5 == 1 / 3 so far left / right of the window
    that their whole column underflows against the 1e-16 of the normalisation (den of the gather ~ 1e-6) -> (GX, mu)"""
    from oracle import x3d_ref as R
    B, Tf = mask.shape
    Rr = B * crops
    std = mask.sum(1) / 8
    far = (torch.sqrt(60 * 2 * std * std) + 1).repeat_interleave(crops).view(Rr, 1)
    u = torch.rand(Rr, K, generator=gen)
    mu = u * (Tf + 1) - 1
    k = torch.arange(K).view(1, K)
    mu = torch.where(k % 5 == 1, -far - u, mu)
    mu = torch.where(k % 5 == 3, Tf - 1 + far + u, mu)
    meta = torch.zeros(B, 4, dtype=torch.int64)
    return R.gaussian(meta, mask, mu.float().contiguous(), 1.0).contiguous(), mu


@functools.lru_cache(maxsize=None)
def fg_inputs(shape, regime):
    """-> dict(x, at_raw, bias, GX, mask, gz, crops): fp32 CPU tensors"""
    B, crops, C, Tf, K, P = shape
    gen = _seed(6, FG_REGIMES.index(regime), *shape)
    if regime == 'masked':
        B += 1
    x, at_raw = torch.randn(B, C, Tf, P, generator=gen), 3 * torch.randn(B, Tf, P, generator=gen)
    gz = torch.randn(B * crops, C, K, P, generator=gen)
    mask = torch.ones(B, Tf)
    if Tf >= 4:
        mask[-1, -2:] = 0
    if regime == 'masked':
        mask[0] = 0
    if regime == 'sat':
        sel = torch.rand(B, Tf, P, generator=gen)
        at_raw = torch.where(sel < 0.05, torch.full_like(at_raw, 100.0), torch.where(sel > 0.95, torch.full_like(at_raw, -100.0), at_raw))
    bias = None if regime == 'nobias' else torch.tensor([-1.5 if regime == 'bias' else 0.3])
    GX, _ = _oracle_GX(mask, crops, K, gen)
    assert bool(torch.isfinite(GX).all())
    return dict(x=x, at_raw=at_raw.contiguous(), bias=bias, GX=GX, mask=mask, gz=gz, crops=crops)


def fg_ref_of(inp, **kw):
    return fusion_gather_ref64(inp['x'], inp['at_raw'], inp['bias'], inp['GX'], inp['mask'], inp['gz'], inp['crops'], **kw)


@functools.lru_cache(maxsize=None)
def fg_reference(shape, regime):
    return fg_ref_of(fg_inputs(shape, regime))


def fg_slice(inp, P=None, K=None, crop=None):
    """the inputs restricted to the first P positions, the first K knots or one crop of every video (the metamorphic checks)"""
    out = dict(inp)
    if P is not None:
        out.update(x=inp['x'][..., :P].contiguous(), at_raw=inp['at_raw'][..., :P].contiguous(), gz=inp['gz'][..., :P].contiguous())
    if K is not None:
        out.update(GX=inp['GX'][..., :K].contiguous(), gz=inp['gz'][:, :, :K].contiguous())
    if crop is not None:
        c = inp['crops']
        out.update(GX=inp['GX'][crop::c].contiguous(), gz=inp['gz'][crop::c].contiguous(), crops=1)
    return out


# gauss_align: name -> (B, crops, Tf, K, tx, ratio)
GA_CASES = {
    'wg2': (2, 2, 12, 65, 256, 256 / 12),         # 260 threads: a second, ragged workgroup
    't64': (3, 1, 40, 17, 64, 1.6),
    'half': (1, 1, 128, 17, 64, 0.5),
    'masked': (2, 1, 7, 5, 16, 16 / 7),           # the second video fully masked: std = 0
    'knots1': (2, 2, 9, 6, None, 1),              # gx = None: tl = k
    'knots2': (2, 2, 9, 6, None, 2),              # ... at ratio 2: every other mu is an exact half-integer
    'tie': (2, 1, 12, 8, 16, 2),                  # exact half-integer mu: two bit-equal maxima, the gradient to the first
    'edges': (1, 1, 10, 4, 1, 1),                 # mu left and right of the window: argmax at frame 0 and at frame Tf - 1
    'underflow': (1, 1, 6, 4, 1, 1),              # std = 1/8 and every mu >= 5 frames away: every f underflows (in fp64 too)
    'step': (2, 3, 20, 9, 32, 1.6),               # crops = 3 with meta[:, 3] = 2, 3
    'chain': (2, 2, 10, 9, 32, 3.2),              # the Gaussian of the chained case
}
GA_TIE_J = [[1, 3, 4, 7, 9, 12, 15, 21], [0, 2, 3, 4, 6, 8, 11, 14]]      # gx = j / 16, st = 0 / 3: mu = (j + st) / 2
GA_TIE_TM = [[0, 1, 2, 3, 4, 6, 7, 10], [1, 2, 3, 3, 4, 5, 7, 8]]           # by hand: floor(mu) for a half-integer (the first of the two)
GA_EDGES_GX = [[-3.2, -0.7, 9.8, 13.3]]
GA_EDGES_TM = [[0, 0, 9, 9]]
GA_UNDERFLOW_GX = [[-6.0, -7.3, 11.2, 12.6]]
GA_MUTANTS = {'wg2': ('crop0_start', 'ratio_ignored', 'std_from_Tf'), 't64': ('ratio_ignored', 'std_from_Tf'), 'half': ('ratio_ignored',),
              'masked': ('std_from_Tf',), 'knots2': ('ratio_ignored', 'crop0_start'), 'tie': ('argmax_last', 'ratio_ignored'),
              'step': ('crop0_start', 'std_from_Tf'), 'chain': ('crop0_start',)}


@functools.lru_cache(maxsize=None)
def ga_inputs(name):
    """-> dict(meta, mask, gx (None in the knots cases), tx, ratio, crops, K, gGX): meta = [3 b, 64, Tf, 1 + b]; the last video's last
    frames masked where the case does not say otherwise; gx sorted rand, moved by 2^-6 frames where frac(mu) is within 2^-9 of 0.5; gGX
    randn with every fourth knot's column zero"""
    B, crops, Tf, K, tx, rt = GA_CASES[name]
    gen = _seed(7, *[ord(ch) for ch in name])
    R = B * crops
    meta = torch.stack([torch.tensor([3 * i, 64, Tf, 1 + i]) for i in range(B)]).to(torch.int64)
    mask = torch.ones(B, Tf)
    if Tf > 8:
        mask[-1, Tf - 3:] = 0
    gx = None
    if name == 'masked':
        mask[1] = 0
    if name == 'tie':
        mask = torch.ones(B, Tf)
        gx = torch.tensor(GA_TIE_J, dtype=torch.float32) / 16
    elif name == 'edges':
        meta[:, 0] = 0
        gx = torch.tensor(GA_EDGES_GX, dtype=torch.float32)
    elif name == 'underflow':
        meta[:, 0] = 0
        mask = torch.zeros(B, Tf)
        mask[:, 0] = 1
        gx = torch.tensor(GA_UNDERFLOW_GX, dtype=torch.float32)
    elif tx is not None:
        if name == 'step':
            meta[:, 3] = torch.tensor([2, 3])
        gx = torch.sort(torch.rand(R, K, generator=gen), 1)[0]
        mu = gauss_align_ref64(meta, mask, gx, tx, rt, crops, K)['mu']
        near = ((mu - torch.floor(mu) - 0.5).abs() < 2.0 ** -9)
        gx = torch.where(near, gx + (2.0 ** -6) * rt / tx, gx.double()).float().contiguous()
    gGX = torch.randn(R, Tf, K, generator=gen)
    gGX[:, :, ::4] = 0
    return dict(meta=meta, mask=mask, gx=gx, tx=tx, ratio=rt, crops=crops, K=K, gGX=gGX)


def ga_ref_of(inp, **kw):
    return gauss_align_ref64(inp['meta'], inp['mask'], inp['gx'], inp['tx'], inp['ratio'], inp['crops'], inp['K'], inp['gGX'], **kw)


@functools.lru_cache(maxsize=None)
def ga_reference(name):
    return ga_ref_of(ga_inputs(name))


@functools.lru_cache(maxsize=None)
def ga_baseline(name):
    """the same expression in plain fp32 torch: the yardstick of the measured ggx rule"""
    return ga_ref_of(ga_inputs(name), dtype=torch.float32)


# ---- the chained case: gauss_align into fusion_gather at (B, crops, C, Tf, K, P) = (2, 2, 6, 10, 9, 49) -----------------------------------------
CHAIN_SHAPE = (2, 2, 6, 10, 9, 49)
CHAIN_KEYS = ('z', 'gcdf', 'gx', 'gat')


@functools.lru_cache(maxsize=None)
def chain_inputs():
    g = ga_inputs('chain')
    B, crops, C, Tf, K, P = CHAIN_SHAPE
    gen = _seed(8, *CHAIN_SHAPE)
    return dict(g, x=torch.randn(B, C, Tf, P, generator=gen), at_raw=3 * torch.randn(B, Tf, P, generator=gen), bias=torch.tensor([0.3]),
                gz=torch.randn(B * crops, C, K, P, generator=gen))


def gather_expr(x, at_raw, bias, GX, mask, crops):
    """the einsum form of x3d_coarse.py:209-223 (as in tests/test_hip_fullsize_coarse.py) in the dtype of its inputs, differentiable"""
    rep = lambda v: v.unsqueeze(1).repeat((1, crops) + (1,) * (v.dim() - 1)).view((v.shape[0] * crops,) + tuple(v.shape[1:]))
    at = rep(torch.sigmoid(at_raw if bias is None else at_raw + bias))
    wgt = at.unsqueeze(2) * (GX * rep(mask).unsqueeze(2)).unsqueeze(3)                       # B2 Tf K P
    return torch.einsum('bctp,btkp->bckp', rep(x), wgt) / (wgt.sum(1) + 1e-6).unsqueeze(1), wgt


@functools.lru_cache(maxsize=None)
def chain_reference(dtype=torch.float64):
    """autograd through gaussian_expr and gather_expr in `dtype` -> {'z', 'gcdf', 'gx', 'gat'}: fp64 tensors"""
    c = chain_inputs()
    leaf = lambda v: v.detach().to(dtype).requires_grad_(True)
    cdf, x, at_raw = leaf(c['gx']), leaf(c['x']), leaf(c['at_raw'])
    GX = gaussian_expr(c['meta'], c['mask'].to(dtype), cdf, c['tx'], c['ratio'], dtype=dtype)
    z, _ = gather_expr(x, at_raw, c['bias'].to(dtype), GX, c['mask'].to(dtype), c['crops'])
    grads = torch.autograd.grad((z * c['gz'].to(dtype)).sum(), [cdf, x, at_raw])
    return dict(zip(CHAIN_KEYS, [v.detach().double() for v in (z,) + tuple(grads)]))
