"""fp64 references of the streaming kernels of csrc/elementwise.hip and csrc/streambf16.hip (built a second time as streamf16.hip) -- the block
tail bn_add_relu (forward, one-tensor backward bwd_g, two-tensor backward), affine_act, channel_stats, pool_hw (general and global-mean
kernel) and film -- in plain torch on the CPU (test infrastructure), and the inputs of the cases tests/test_hip_elementwise.py runs them at.

Every reference returns, per output, Res(val, n, mag) of tests/temporal_ref64.py: the kernel is held to |kernel - val| <= (n + 8) 2^-24 mag
elementwise, and an element with mag = 0 must be an exact zero.  Per-channel coefficients are arbitrary doubles which the kernels round to
fp32 once (one rounding of one summand: inside the slack of 8).
    tail forward     z = A y + Ar res + (B + Br): n = 3, mag = |A y| + |Ar res| + |B + Br|; out = relu(z)
    g                (gout [+ gout2]) (z > 0): n = the number of gradients present, mag = |gout| + |gout2| (with one gradient the tests ask for
                     bit equality on top of that)
    gy, gres         g A, g Ar: one more rounding
    gA, gB, gAr      sum g y, sum g, sum g res over the channel: n = one thread's share (32 on the float4 and 16-bit vector routes, 8 on the
                     scalar routes) + 8 for the wave and block tree, mag = the sum of the absolute summands.  (The 16-bit scalar kernel gives a
                     thread 32 elements; its inputs are multiples of 2^-6 whose products and per-thread sums are exact in fp32, so the 8 holds.)
    mask             fp32: bit 4k+e of word (nc nchunks + chunk) 256 + tid is element chunk 8192 + k 1024 + 4 tid + e; 16-bit: bit 8k+j is
                     element chunk 8192 + k 2048 + 8 tid + j; bits past vol are 0; compared exactly
    pool             n = the window size; backward n = the windows that contain the pixel; gA, gB: n = one thread's share + 8
    film             out n = 2; gx one product; gm, gc n = f^2
ReLU decisions are taken from the fp64 z, so the inputs hold no element with 0 < |z| <= bound (tail_inputs and friends move such elements
away; `amb` counts what is left: 0 in every case, asserted by tests/test_elementwise_ref64_cpu.py).  Exact zeros (z = 0 in both precisions)
are planted on purpose: out = 0, mask bit 0, g = 0.

16-bit tensors (store=torch.bfloat16 / torch.float16): y, res, gout, gout2 are multiples of 2^-6 below 4 (exact in both formats, their sums
exact in fp32); out gets the fp32 bound plus half a storage ulp of val (key 'out_extra'; fp16: at least 2^-25); g is the reference rounded
once to the storage type, bit-equal (n = -8), and the reductions run over the rounded g, as the kernel documents.

Swish and sigmoid (act 2, 3) go through the hardware exp and rcp: per element ACT_SCALE[act] (|z| + 8) 2^-23 |val| (one ulp each for exp and
rcp and one rounding of z log2(e), ACT_SCALE = 1; scaled by a power of two only if a measurement on the GPU says so, see
tests/test_hip_elementwise.py) plus the bound of z times |act'(z)|.  Their derivatives, by the same assumptions: sigmoid s has the absolute error e_s = (|z| + 8) 2^-23 s (1 - s) + 2^-22 s (the relative error of exp(-z) reaches s
through ds/de = -s^2, then the rounding of 1 + e and the rcp); act' = s (1 - s) or s (1 + z (1 - s)) takes e_s |d act'/d s| + 4 2^-24 mag'
+ the bound of z times |act''(z)|.

dtype=torch.float32 evaluates the same expression as plain fp32 torch would (it must lie within the bound); mutant names ONE deliberate
error (MUTANTS): the mutated fp64 result must leave the bound of every case that names it."""
import collections
import functools
import math

import torch

from temporal_ref64 import Res, bound, ratio, U24

MUTANTS = ('relu_ge', 'drop_gout2', 'drop_br', 'gar_from_y', 'mask_nibble_reversed', 'mask_tail_bits_set', 'last_chunk_dropped',
           'pool_end_floor', 'pool_swap_hw', 'pool1_first_sweep_only', 'film_swap_hw', 'film_block_f_minus_1')
ACT_SCALE = {2: 1.0, 3: 1.0}
WG = 8192                               # elements per workgroup of the vector routes (fp32: 256 x 8 float4; 16-bit: 256 x 4 x 8)
STORE = {'f32': None, 'bf16': torch.bfloat16, 'f16': torch.float16}


def _res(val, n, mag):
    val = val.double()
    n = n if isinstance(n, torch.Tensor) else torch.full((), float(n), dtype=torch.float64)
    return Res(val, n.double().expand_as(val), mag.double().expand_as(val))


def _res_bound(val, bnd):
    """a Res whose bound() is bnd: n = -7 makes the factor 2^-24"""
    return _res(val, -7, bnd.double() / U24)


def _seed(*ints):
    s = 23
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def half_ulp(val, store):
    """half a unit in the last place of the storage type at |val| (subnormal spacing below the smallest normal)"""
    if store is None:
        return torch.zeros_like(val, dtype=torch.float64)
    bits, emin = (7, -126) if store == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(val.double().abs().clamp_min(2.0 ** -140))).clamp_min(emin)
    return 0.5 * torch.pow(torch.full_like(e, 2.0), e - bits)


def ratio_x(got, r, extra):
    """ratio() with an absolute allowance `extra` added to the bound of every element"""
    if got is None or tuple(got.shape) != tuple(r.val.shape) or not bool(torch.isfinite(got).all()):
        return math.inf
    err, b = (got.detach().double().cpu() - r.val).abs(), bound(r) + extra
    zero = b == 0
    if bool((err[zero] > 0).any()):
        return math.inf
    return float((err[~zero] / b[~zero]).max()) if bool((~zero).any()) else 0.0


# ---- the block tail -------------------------------------------------------------------------------------------------------------------------
def mask_words(pos, per, tail_ones=False, reverse=False):
    """pos (NC, vol) bool -> the int64 words (NC * nchunks * 256,) of the ReLU bit mask; per = elements per access (4 fp32, 8 16-bit):
    bit per*k + e of word (nc nchunks + chunk) 256 + tid = element chunk 8192 + k 256 per + tid per + e"""
    NC, vol = pos.shape
    nch, items = -(-vol // WG), 32 // per
    full = torch.full((NC, nch * WG), bool(tail_ones), dtype=torch.bool)
    full[:, :vol] = pos
    bits = full.view(NC, nch, items, 256, per).permute(0, 1, 3, 2, 4)
    if reverse:
        bits = bits.flip(4)
    w = 2 ** torch.arange(32, dtype=torch.int64)
    return (bits.reshape(NC, nch, 256, 32).long() * w).sum(3).reshape(-1)


def tail_ref64(y, res, A, B, Ar, Br, gout, gout2, share, per=None, store=None, dtype=torch.float64, mutant=None):
    """y, res, gout, gout2 (None: absent) (NC, vol); A, B, Ar, Br (None: plain residual) (NC,) fp64; share: a thread's elements in the
    reductions; per: elements per vector access where the route emits a mask (None: no mask) -> dict of Res (out, g, gy, gres, gA, gB, gAr),
    'out_extra', 'mask' (int64 words or None), 'pos', 'amb' (the number of ambiguous ReLU decisions)"""
    assert mutant is None or mutant in MUTANTS, mutant
    NC, vol = y.shape
    col = lambda v: v.double().to(dtype).view(NC, 1)
    a = col(A)
    ar = col(Ar) if Ar is not None else torch.ones(NC, 1, dtype=dtype)
    b = col(B.double() + (Br.double() if Br is not None and mutant != 'drop_br' else 0.0))
    bt = col(B.double() + (Br.double() if Br is not None else 0.0))
    yv, rv = y.detach().to(dtype), res.detach().to(dtype)
    z = a * yv + (ar * rv + b)
    zmag = (a * yv).abs() + (ar * rv).abs() + bt.abs()
    pos = z >= 0 if mutant == 'relu_ge' else z > 0
    keep = torch.ones(vol, dtype=torch.bool)
    if mutant == 'last_chunk_dropped':
        keep = torch.arange(vol) < (-(-vol // WG) - 1) * WG
    out = torch.where(pos & keep, z, torch.zeros_like(z))
    if store is not None and dtype != torch.float64:
        out = out.to(store).to(dtype)
    zr = _res(z, 3, zmag)
    extra = half_ulp(out, store)
    amb = int(((z != 0) & (z.double().abs() <= bound(zr) + extra)).sum())
    two = gout2 is not None
    gs = gout.detach().to(dtype) + (gout2.detach().to(dtype) if two and mutant != 'drop_gout2' else 0.0)
    gmag = gout.detach().double().abs() + (gout2.detach().double().abs() if two else 0.0)
    g = torch.where(pos & keep, gs, torch.zeros_like(gs))
    if store is not None:
        g = g.to(store).to(dtype)
    ng = -8 if store is not None else (2 if two else 1)
    red = lambda v: v.sum(1)
    rn = share + 8
    r = {'out': _res(out, 3, zmag), 'out_extra': extra, 'g': _res(g, ng, gmag), 'pos': pos, 'amb': amb, 'z': z.double(),
         'gy': _res(g * a, ng + 1, (g * a).abs()), 'gres': _res(g * ar, ng + 1, (g * ar).abs()),
         'gA': _res(red(g * yv), rn, red((g * yv).abs())), 'gB': _res(red(g), rn, red(g.abs())), 'gAr': None, 'mask': None}
    if store is not None:                                  # the 16-bit kernels write g only
        r['gy'] = r['gres'] = None
    if Ar is not None:
        src = yv if mutant == 'gar_from_y' else rv
        r['gAr'] = _res(red(g * src), rn, red((g * rv).abs()))
    if per is not None:
        r['mask'] = mask_words(pos & keep, per, tail_ones=(mutant == 'mask_tail_bits_set'), reverse=(mutant == 'mask_nibble_reversed'))
    return r


TAIL_KEYS = ('out', 'g', 'gy', 'gres', 'gA', 'gB', 'gAr')


def tail_worst(got, ref):
    """worst err / bound over the outputs both sides have; a differing mask counts as inf"""
    worst = 0.0
    for k in TAIL_KEYS:
        if ref.get(k) is None or got.get(k) is None:
            continue
        v = got[k].val if isinstance(got[k], Res) else got[k]
        worst = max(worst, ratio_x(v, ref[k], ref['out_extra']) if k == 'out' else ratio(v, ref[k]))
    if ref['mask'] is not None and got.get('mask') is not None and not torch.equal(got['mask'], ref['mask']):
        worst = math.inf
    return worst


Tail = collections.namedtuple('Tail', 'NC vol ar two misaligned')
# fp32.  float4 volumes 4, 1020, 1024, 1028 (around one 1024-element item), 8188, 8192, 8196 (around one workgroup), 16388 (three workgroups,
# the last with one active thread); scalar volumes 5, 2047, 2049 (around one 2048-element scalar workgroup); m1024: a view 4 bytes into its
# allocation (the scalar route although vol % 4 == 0).  NC * ceil(vol / 8192) = the flat grid: 1, 7, 8 (q = 1, r = 0), 9, 15, 26 (q = 3,
# r = 2) and 2, 3; all four (Ar/Br, gout2) combinations at 8196 and 5
TAIL_F32 = {
    'v4': Tail(1, 4, False, False, False), 'v1020': Tail(7, 1020, True, True, False), 'v1024': Tail(8, 1024, False, True, False),
    'v1028': Tail(9, 1028, True, False, False), 'v8188': Tail(3, 8188, False, False, False), 'v8192': Tail(2, 8192, True, True, False),
    'v8196-00': Tail(13, 8196, False, False, False), 'v8196-01': Tail(4, 8196, False, True, False),
    'v8196-10': Tail(4, 8196, True, False, False), 'v8196-11': Tail(4, 8196, True, True, False),
    'v16388': Tail(5, 16388, True, True, False),
    's5-00': Tail(3, 5, False, False, False), 's5-01': Tail(3, 5, False, True, False), 's5-10': Tail(3, 5, True, False, False),
    's5-11': Tail(3, 5, True, True, False), 's2047': Tail(2, 2047, True, False, False), 's2049': Tail(3, 2049, False, True, False),
    'm1024': Tail(2, 1024, True, True, True),
}
# 16-bit.  vector volumes 8, 2040, 2048, 2056 (around one 2048-element item), 8192, 8200; scalar 7, 8193; m2048 misaligned by one element
TAIL_H16 = {
    'v8': Tail(1, 8, False, False, False), 'v2040': Tail(3, 2040, True, True, False), 'v2048': Tail(3, 2048, False, True, False),
    'v2056': Tail(3, 2056, True, False, False), 'v8192': Tail(2, 8192, True, True, False),
    'v8200-00': Tail(3, 8200, False, False, False), 'v8200-01': Tail(3, 8200, False, True, False),
    'v8200-10': Tail(3, 8200, True, False, False), 'v8200-11': Tail(3, 8200, True, True, False),
    's7-00': Tail(3, 7, False, False, False), 's7-01': Tail(3, 7, False, True, False), 's7-10': Tail(3, 7, True, False, False),
    's7-11': Tail(3, 7, True, True, False), 's8193': Tail(2, 8193, True, True, False), 'm2048': Tail(2, 2048, True, True, True),
}
TAIL_CASES = {'f32': TAIL_F32, 'bf16': TAIL_H16, 'f16': TAIL_H16}
PLANT = (1, 2)                           # positions, in the LAST channel, of the planted exact zeros


def tail_route(kind, name):
    """-> (vector route?, share, per): what cfn_bn_add_relu_* picks for the case"""
    c = TAIL_CASES[kind][name]
    per = 4 if kind == 'f32' else 8
    vec = c.vol % per == 0 and not c.misaligned
    return vec, (32 if vec else 8), (per if vec else None)


def tail_mutants(kind, name):
    c = TAIL_CASES[kind][name]
    vec = tail_route(kind, name)[0]
    m = ['relu_ge']
    if c.two:
        m.append('drop_gout2')
    if c.ar:
        m += ['drop_br', 'gar_from_y']
    if vec:
        if c.vol >= 64:                  # (a handful of elements can be a palindrome, or all negative)
            m += ['last_chunk_dropped', 'mask_nibble_reversed']
        if c.vol % WG:
            m.append('mask_tail_bits_set')
    return tuple(m)


@functools.lru_cache(maxsize=None)
def tail_inputs(kind, name):
    """-> dict y, res, gout, gout2 (fp32 (NC, vol); 16-bit kinds: multiples of 2^-6, |k| < 256), A, B, Ar, Br (fp64 (NC,)); absent ones None.
    With three channels or more, A[0] = 0 and A[1] < 0.  The last channel has A = Ar = 1, B = Br = 0 and two planted exact zeros at PLANT:
    y = -res = 0.5, and y = -0.0 with res = 0; their gout (and gout2) are non-zero.  Elements whose |z| lies within 4 x the bound of 0 are
    moved away (y towards 0 by 2^-6, res where A = 0)"""
    c = TAIL_CASES[kind][name]
    NC, vol = c.NC, c.vol
    gen = _seed(1, len(kind), *[ord(ch) for ch in kind + name])
    if kind == 'f32':
        draw = lambda: torch.randn(NC, vol, generator=gen)
    else:
        draw = lambda: torch.randint(-255, 256, (NC, vol), generator=gen).float() / 64
    y, res, gout, gout2 = draw(), draw(), draw(), draw()
    dbl = lambda s: torch.randn(NC, generator=gen, dtype=torch.float64) * s
    A, B, Ar, Br = 1 + dbl(0.2), dbl(0.2), 1 + dbl(0.3), dbl(0.1)
    if NC >= 3:
        A[0], A[1] = 0.0, -0.75 - A[1].abs()
    p = NC - 1
    A[p], B[p], Ar[p], Br[p] = 1.0, 0.0, 1.0, 0.0
    y[p, PLANT[0]], res[p, PLANT[0]], y[p, PLANT[1]], res[p, PLANT[1]] = 0.5, -0.5, -0.0, 0.0
    gout[p, list(PLANT)], gout2[p, list(PLANT)] = 1.5, 0.25
    if not c.ar:
        Ar = Br = None
    if not c.two:
        gout2 = None
    store = STORE[kind]
    for _ in range(20):
        r = tail_ref64(y, res, A, B, Ar, Br, gout, gout2, 8, store=store)
        near = (r['z'] != 0) & (r['z'].abs() <= 4 * (bound(r['out']) + r['out_extra']))
        if not bool(near.any()):
            break
        mv_y = near & (A != 0).view(NC, 1)
        step = lambda v: torch.where(v > 0, v - 2.0 ** -6, v + 2.0 ** -6)
        y = torch.where(mv_y, step(y), y)
        res = torch.where(near & ~mv_y, step(res), res)
    else:
        raise AssertionError('ambiguous ReLU decisions left in %s %s' % (kind, name))
    return dict(y=y, res=res, gout=gout, gout2=gout2, A=A, B=B, Ar=Ar, Br=Br)


def tail_args(kind, name):
    v = tail_inputs(kind, name)
    return v['y'], v['res'], v['A'], v['B'], v['Ar'], v['Br'], v['gout'], v['gout2']


@functools.lru_cache(maxsize=None)
def tail_reference(kind, name):
    _, share, per = tail_route(kind, name)
    return tail_ref64(*tail_args(kind, name), share, per=per, store=STORE[kind])


F16_TINY = (2.0 ** -26, 2.0 ** -25, 1.5 * 2.0 ** -25)


def f16_tiny_inputs():
    """fp16 only: z = A y with y = 1, res = 0, B = 0 and A = 2^-26, 2^-25 (both store as +0: the second is a tie, rounded to even) and
    1.5 2^-25 (stores as 2^-24); vol 8, gout = 1.5 -> (y, res, A, B, gout, stored out > 0 per channel)"""
    n = len(F16_TINY)
    A = torch.tensor(F16_TINY, dtype=torch.float64)
    stored = torch.tensor(F16_TINY, dtype=torch.float32).half()
    return torch.ones(n, 8), torch.zeros(n, 8), A, torch.zeros(n, dtype=torch.float64), torch.full((n, 8), 1.5), stored > 0


# ---- activations ----------------------------------------------------------------------------------------------------------------------------
def act_ref(z, zb, act, dtype=torch.float64):
    """z in dtype, zb its fp64 bound -> (val, bound of val, act'(z), bound of act'(z), mag of act'(z)); act 0 none, 1 relu, 2 swish, 3 sigmoid.
    For act 0 and 1 the bounds returned are zb |act'| and 0: the caller's (n + 8) 2^-24 mag term carries the roundings"""
    zd = z.double()
    if act == 0:
        return z, zb, torch.ones_like(z), torch.zeros_like(zd), torch.ones_like(zd)
    if act == 1:
        d = (z > 0).to(dtype)
        return z * d, zb * d.double(), d, torch.zeros_like(zd), d.double()
    s = torch.sigmoid(z)
    sd = torch.sigmoid(zd)
    e_s = (zd.abs() + 8) * 2.0 ** -23 * sd * (1 - sd) + 2.0 ** -22 * sd
    if act == 3:
        val, d = s, s * (1 - s)
        dd = sd * (1 - sd)
        d2 = dd * (1 - 2 * sd)
        db = e_s * (1 - 2 * sd).abs() + 4 * U24 * dd + zb * d2.abs()
        dmag = dd
    else:
        val, d = z * s, s * (1 + z * (1 - s))
        dd = sd * (1 + zd * (1 - sd))
        d2 = sd * (1 - sd) * (2 + zd * (1 - 2 * sd))
        dmag = sd * (1 + zd.abs() * (1 - sd))
        db = e_s * (1 + zd.abs() * (1 - 2 * sd).abs()) + 4 * U24 * dmag + zb * d2.abs()
    vb = ACT_SCALE[act] * (zd.abs() + 8) * 2.0 ** -23 * val.double().abs() + zb * dd.abs()
    return val, vb, d, db, dmag


def affine_ref64(x, A, B, act, g, share, dtype=torch.float64):
    """x, g (NC, vol), A, B (NC,) fp64 -> out, gx, gA, gB (Res), sum, sumsq (channel_stats; Res), amb"""
    NC, vol = x.shape
    a, b = A.double().to(dtype).view(NC, 1), B.double().to(dtype).view(NC, 1)
    xv, gv = x.detach().to(dtype), g.detach().to(dtype)
    z = a * xv + b
    zmag = (a * xv).abs().double() + b.abs().double()
    zb = 10 * U24 * zmag                                   # n = 2
    val, vb, d, db, dmag = act_ref(z, zb, act, dtype)
    amb = int(((z != 0) & (z.double().abs() <= zb)).sum()) if act == 1 else 0
    out = _res(val, 2, zmag) if act < 2 else _res_bound(val, vb + 2 * U24 * val.double().abs())
    dz = gv * d
    dzb = gv.double().abs() * db + 2 * U24 * dz.double().abs()
    gx = _res_bound(dz * a, dzb * a.double().abs() + 2 * U24 * (dz * a).double().abs())
    rb = (share + 16) * U24
    gA = _res_bound((dz * xv).sum(1), (dzb * xv.double().abs()).sum(1) + rb * (dz * xv).double().abs().sum(1))
    gB = _res_bound(dz.sum(1), dzb.sum(1) + rb * dz.double().abs().sum(1))
    return {'out': out, 'gx': gx, 'gA': gA, 'gB': gB, 'amb': amb,
            'sum': _res(xv.sum(1), share + 8, xv.abs().sum(1)), 'sumsq': _res((xv * xv).sum(1), share + 8, (xv * xv).sum(1))}


AFF_VOLS = (4, 5, 8192, 8196, 2049)
AFF_NC = 3


@functools.lru_cache(maxsize=None)
def aff_inputs(vol, act):
    """x uniform over [-12, 12] (z = A x + B spreads over that range, so the |z| term of the bound matters), A = 1 +- 0.05 with A[1] < 0,
    B = 0.2 randn, g randn; ReLU: elements near z = 0 moved by 2^-6"""
    gen = _seed(2, vol)
    x = (torch.rand(AFF_NC, vol, generator=gen) * 2 - 1) * 11.5
    g = torch.randn(AFF_NC, vol, generator=gen)
    A = 1 + torch.randn(AFF_NC, generator=gen, dtype=torch.float64) * 0.02
    A[1] = -A[1]
    B = torch.randn(AFF_NC, generator=gen, dtype=torch.float64) * 0.2
    if act == 1:
        for _ in range(20):
            z = A.view(-1, 1) * x.double() + B.view(-1, 1)
            near = (z != 0) & (z.abs() <= 40 * U24 * ((A.view(-1, 1) * x.double()).abs() + B.abs().view(-1, 1)))
            if not bool(near.any()):
                break
            x = torch.where(near, x + 2.0 ** -6, x)
    return x, A, B, g


def aff_share(vol):
    return 32 if vol % 4 == 0 else 8


@functools.lru_cache(maxsize=None)
def aff_reference(vol, act):
    x, A, B, g = aff_inputs(vol, act)
    return affine_ref64(x, A, B, act, g, aff_share(vol))


# ---- pool_hw ----------------------------------------------------------------------------------------------------------------------------------
def _windows(O, S, floor_end=False):
    return [((o * S) // O, ((o + 1) * S) // O if floor_end else -(-((o + 1) * S) // O)) for o in range(O)]


def pool_ref64(x, A, B, act, OH, OW, g, share, store=None, dtype=torch.float64, mutant=None):
    """x (NC, T, H, W), A, B (NC,) fp64 or None, g (NC, T, OH, OW) -> out, gx (Res), 'gx_extra', gA, gB (Res or None), amb.
    Windows [floor(o S / O), ceil((o + 1) S / O)) as in ATen's adaptive pooling"""
    assert mutant is None or mutant in MUTANTS, mutant
    NC, T, H, W = x.shape
    one, zero = torch.ones(NC, dtype=torch.float64), torch.zeros(NC, dtype=torch.float64)
    a = (A if A is not None else one).double().to(dtype).view(NC, 1, 1, 1)
    b = (B if B is not None else zero).double().to(dtype).view(NC, 1, 1, 1)
    xv, gv = x.detach().to(dtype), g.detach().to(dtype)
    z = a * xv + b
    zmag = (a * xv).abs().double() + b.abs().double()
    zb = 10 * U24 * zmag
    v, vb, d, db, dmag = act_ref(z, zb, act, dtype)
    amb = int(((z != 0) & (z.double().abs() <= zb)).sum()) if act == 1 else 0
    if act < 2:
        vb = torch.zeros_like(zb)                           # the roundings of z are inside the slack of the sum
    smag = zmag * dmag if act < 2 else v.double().abs()     # a summand z = a x + b counts as |a x| + |b|
    fl = mutant == 'pool_end_floor'
    if mutant == 'pool_swap_hw':
        wh = [(s, min(e, H)) for s, e in _windows(OH, W)]
        ww = [(s, min(e, W)) for s, e in _windows(OW, H)]
    else:
        wh, ww = _windows(OH, H, fl), _windows(OW, W, fl)
    out = torch.zeros(NC, T, OH, OW, dtype=dtype)
    omag, ob, on = (torch.zeros(NC, T, OH, OW, dtype=torch.float64) for _ in range(3))
    gp, gpmag, gpn = torch.zeros_like(xv), torch.zeros(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.float64)
    for oh, (h0, h1) in enumerate(wh):
        for ow, (w0, w1) in enumerate(ww):
            cnt = (h1 - h0) * (w1 - w0)
            if cnt <= 0:
                out[:, :, oh, ow] = float('nan')
                continue
            out[:, :, oh, ow] = v[:, :, h0:h1, w0:w1].sum((2, 3)) / cnt
            omag[:, :, oh, ow] = smag[:, :, h0:h1, w0:w1].sum((2, 3)) / cnt
            ob[:, :, oh, ow] = vb[:, :, h0:h1, w0:w1].sum((2, 3)) / cnt
            on[:, :, oh, ow] = cnt
            gp[:, :, h0:h1, w0:w1] += (gv[:, :, oh, ow] / cnt).view(NC, T, 1, 1)
            gpmag[:, :, h0:h1, w0:w1] += (gv[:, :, oh, ow].double().abs() / cnt).view(NC, T, 1, 1)
            gpn[:, :, h0:h1, w0:w1] += 1
    if mutant == 'pool1_first_sweep_only':
        out[:, 512:] = 0
    gpb = (gpn + 8) * U24 * gpmag
    dz = gp * d
    dzb = gpb * dmag + gp.double().abs() * db + 2 * U24 * dz.double().abs()
    gx = dz * a
    r = {'out': _res_bound(out, (on + 8) * U24 * omag + ob), 'amb': amb, 'gA': None, 'gB': None,
         'gx': _res_bound(gx, dzb * a.double().abs() + 2 * U24 * gx.double().abs()), 'gx_extra': half_ulp(gx, store)}
    if A is not None:
        rb = (share + 16) * U24
        r['gA'] = _res_bound((dz * xv).sum((1, 2, 3)), (dzb * xv.double().abs()).sum((1, 2, 3)) + rb * (dz * xv).double().abs().sum((1, 2, 3)))
        r['gB'] = _res_bound(dz.sum((1, 2, 3)), dzb.sum((1, 2, 3)) + rb * dz.double().abs().sum((1, 2, 3)))
    return r


POOL_GENERAL = [(6, 10, 3, 7), (5, 9, 2, 4), (16, 16, 7, 7), (8, 8, 7, 7), (3, 5, 7, 7), (5, 13, 1, 1), (14, 14, 1, 1)]     # (H, W, OH, OW)
POOL_T = (1, 6)
POOL1_PLANES = [(1, 1), (7, 7), (7, 9), (8, 8)]           # H * W <= 64: the global-mean wave kernel (fp32 only); 7 x 9 = 63, 8 x 8 = a full wave
POOL1_T = (1, 8, 9, 33, 520, 1030)
POOL_NC = 3


def pool_share(T, H, W, OH, OW, kind='f32'):
    """a thread's elements in the gA / gB sums: the global-mean backward walks its row with 256 threads, the general one has one each"""
    if kind == 'f32' and OH == 1 and OW == 1 and H * W <= 64:
        return -(-T * H * W // 256)
    return 1


def pool_mutants(T, H, W, OH, OW, kind='f32'):
    m = []
    wave = kind == 'f32' and OH == 1 and OW == 1 and H * W <= 64
    if not wave and (H % OH or W % OW):
        m.append('pool_end_floor')
    if not wave and H != W:
        m.append('pool_swap_hw')
    if wave and T > 512:
        m.append('pool1_first_sweep_only')
    return tuple(m)


@functools.lru_cache(maxsize=None)
def pool_inputs(kind, T, H, W, OH, OW, pro, act):
    """x randn * 2 (16-bit kinds: multiples of 2^-6 below 4), g randn, A = 1 +- 0.2 with A[1] < 0, B = 0.2 randn (pro False: None);
    ReLU: elements near z = 0 moved by 2^-6"""
    gen = _seed(3, len(kind), T, H, W, OH, OW)
    if kind == 'f32':
        x = torch.randn(POOL_NC, T, H, W, generator=gen) * 2
    else:
        x = torch.randint(-255, 256, (POOL_NC, T, H, W), generator=gen).float() / 64
    g = torch.randn(POOL_NC, T, OH, OW, generator=gen)
    A = 1 + torch.randn(POOL_NC, generator=gen, dtype=torch.float64) * 0.2
    A[1] = -A[1]
    B = torch.randn(POOL_NC, generator=gen, dtype=torch.float64) * 0.2
    if not pro:
        A = B = None
    if act == 1:
        for _ in range(20):
            a = (A if pro else torch.ones(POOL_NC, dtype=torch.float64)).view(-1, 1, 1, 1)
            b = (B if pro else torch.zeros(POOL_NC, dtype=torch.float64)).view(-1, 1, 1, 1)
            z = a * x.double() + b
            near = (z != 0) & (z.abs() <= 40 * U24 * ((a * x.double()).abs() + b.abs()))
            if not bool(near.any()):
                break
            x = torch.where(near, x + 2.0 ** -6, x)
    return x, A, B, g


@functools.lru_cache(maxsize=None)
def pool_reference(kind, T, H, W, OH, OW, pro, act):
    x, A, B, g = pool_inputs(kind, T, H, W, OH, OW, pro, act)
    return pool_ref64(x, A, B, act, OH, OW, g, pool_share(T, H, W, OH, OW, kind), store=STORE[kind])


# ---- film -------------------------------------------------------------------------------------------------------------------------------------
def film_ref64(x, m, c, f, g, dtype=torch.float64, mutant=None):
    """x, g (NC, T, H, W), m, c (NC, T, H / f, W / f) -> out, gx, gm, gc (Res)"""
    assert mutant is None or mutant in MUTANTS, mutant
    NC, T, H, W = x.shape
    Hs, Ws = H // f, W // f
    xv, mv, cv, gv = (t.detach().to(dtype) for t in (x, m, c, g))
    if mutant == 'film_swap_hw':                           # the cell of pixel (h, w) looked up as (h / f) Hs + w / f
        hh, ww = torch.arange(H).view(H, 1) // f, torch.arange(W).view(1, W) // f
        idx = (hh * Hs + ww).clamp_max(Hs * Ws - 1).view(-1)
        up = lambda t: t.reshape(NC, T, Hs * Ws)[:, :, idx].view(NC, T, H, W)
    else:
        up = lambda t: t.repeat_interleave(f, 2).repeat_interleave(f, 3)
    out = xv * up(mv) + up(cv)
    gx = gv * up(mv)
    keep = torch.ones(f, f, dtype=dtype)
    if mutant == 'film_block_f_minus_1':
        keep[f - 1, :] = 0
        keep[:, f - 1] = 0
    blk = lambda t: (t.view(NC, T, Hs, f, Ws, f) * keep.view(1, 1, 1, f, 1, f)).sum((3, 5))
    full = lambda t: t.view(NC, T, Hs, f, Ws, f).sum((3, 5))
    return {'out': _res(out, 2, (xv * up(mv)).abs() + up(cv).abs()), 'gx': _res(gx, 1, gx.abs()),
            'gm': _res(blk(gv * xv), f * f, full((gv * xv).abs())), 'gc': _res(blk(gv), f * f, full(gv.abs()))}


FILM_CASES = [(7, 7, 1), (14, 14, 2), (8, 12, 4), (56, 56, 8), (28, 14, 2)]      # (H, W, f); T = 6: 294, 294, 36, 294, 588 cells per channel
FILM_T = (1, 6)
FILM_NC = 3
FILM_KEYS = ('out', 'gx', 'gm', 'gc')


def film_mutants(H, W, f):
    return ('film_block_f_minus_1',) + (('film_swap_hw',) if H != W else ())


@functools.lru_cache(maxsize=None)
def film_inputs(T, H, W, f):
    gen = _seed(4, T, H, W, f)
    r = lambda *s: torch.randn(*s, generator=gen)
    return r(FILM_NC, T, H, W), 1 + 0.5 * r(FILM_NC, T, H // f, W // f), r(FILM_NC, T, H // f, W // f), r(FILM_NC, T, H, W)


@functools.lru_cache(maxsize=None)
def film_reference(T, H, W, f):
    x, m, c, g = film_inputs(T, H, W, f)
    return film_ref64(x, m, c, f, g)
