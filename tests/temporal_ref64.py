"""fp64 references of the temporal resampling kernels of csrc/gridpool.hip -- time_sample, interp1d, time_resize, time_pool, grid_cdf -- in plain
torch on the CPU (test infrastructure), and the inputs of the cases tests/test_hip_temporal.py runs them at.

Every reference returns, per output, Res(val, n, mag):
    val   the fp64 result
    n     the number of fp32 summands the kernel adds into that element
    mag   the same sum with every summand replaced by its absolute value (a summand that is a difference a - b counts as |a| + |b|)
and the kernel is held to |kernel - val| <= (n + 8) * 2^-24 * mag elementwise (bound()): n roundings of the running sum plus the few
roundings inside one summand (weight, product, the final store).  Where n = 0, mag = 0: the element must be an exact zero.

Integer decisions and the fp32 coordinates they are taken from are part of the kernels' contract (pinned bit-exactly by the index tests of
tests/test_hip_ops.py), so the references take them in fp32, in the kernel's documented operation order, and everything else in fp64:
    time_sample   it = (((cdf - 0.5) * 2 + 1) / 2) * (Tin - 1) in fp32 (oracle.x3d_ref.grid_sample_time_index), i0 = floor(it);
                  w1 = it - i0, w0 = 1 - w1 in fp64
    interp1d      ind = searchsorted-left - 1 clamped to [0, N-2]; den = fp32(eps + (x1 - x0))
    time_resize   src, i0, i1, l1 = src - i0 in fp32 as in csrc/resize_src.h (the half-pixel FMA as an fp64 product-sum rounded once);
                  l0 = 1 - l1 in fp64
    time_pool     max is exact; the gradient goes to the FIRST maximal frame
    grid_cdf      no integer decision: the expression of x3d_coarse.py:384-392 entirely in fp64, gradient by autograd

dtype=torch.float32 evaluates the same expression the way a plain fp32 implementation would (the result must lie within the bound:
tests/test_temporal_ref64_cpu.py).  mutant names ONE deliberate error (see MUTANTS): a mutated fp64 result must fall outside the bound of
every case that names the mutant, or that case's inputs do not discriminate."""
import collections
import functools
import math

import torch

U24 = 2.0 ** -24
EPS32 = 1.1920928955078125e-07          # torch.finfo(torch.float32).eps (interp1d.py:37)

Res = collections.namedtuple('Res', 'val n mag')

MUTANTS = {
    'time_sample': ('swap_w', 'clamp_border', 'cdf_row0', 'drop_k64', 'no_zero_fill', 'gcdf_first_chunk', 'gcdf_no_scale'),
    'interp1d': ('right', 'bcast_b0'),
    'time_pool': ('last_max',),
    'time_resize': ('no_clamp0', 'no_clamp_i1'),
}


def bound(r, slack=8):
    """(n + slack) * 2^-24 * mag, elementwise"""
    return (r.n.double() + slack) * U24 * r.mag.double()


def ratio(got, r, slack=8):
    """worst |got - val| / bound over the elements; inf if an element with bound 0 is not an exact zero error, if got is not finite or has
    another shape"""
    if got is None or tuple(got.shape) != tuple(r.val.shape) or not bool(torch.isfinite(got).all()):
        return math.inf
    err, b = (got.detach().double().cpu() - r.val).abs(), bound(r, slack).expand_as(r.val)
    zero = b == 0
    if bool((err[zero] > 0).any()):
        return math.inf
    return float((err[~zero] / b[~zero]).max()) if bool((~zero).any()) else 0.0


def _res(val, n, mag):
    val = val.double()
    n = n if isinstance(n, torch.Tensor) else torch.full((), float(n), dtype=torch.float64)
    return Res(val, n.double().expand_as(val), mag.double().expand_as(val))


# ---- time_sample --------------------------------------------------------------------------------------------------------------------------
def time_index_fp32(cdf, Tin):
    """the fp32 frame coordinate ATen's grid_sampler derives from a CDF knot (align_corners=True), in its operation order"""
    coord = (cdf.float() - 0.5) * 2
    return ((coord + 1) / 2) * (Tin - 1)


def time_sample_cchunk(C, P):
    """channels per workgroup of time_sample_bwd_cdf_kernel (the launch rule of cfn_time_sample_bwd)"""
    cchunk = 1
    while cchunk * P < 16384 and cchunk < C:
        cchunk *= 2
    return cchunk


def time_sample_ref64(x, cdf, g, dtype=torch.float64, mutant=None):
    """x (B, C, Tin, *), cdf (B, K), g (B, C, K, *) -> {'y', 'gx', 'gcdf': Res, 'i0': int64 (B, K), 'it': fp32 (B, K)}
    y = w0 x[i0] + w1 x[i0+1] (frames outside [0, Tin) read as zero); gx its adjoint; gcdf = (Tin-1) sum_{c,p} g (x[i0+1] - x[i0]) (the
    slope of the floor-side segment, also when `it` is an integer)"""
    assert mutant is None or mutant in MUTANTS['time_sample'], mutant
    B, C, Tin = x.shape[:3]
    K = cdf.shape[1]
    xs, gs = x.detach().reshape(B, C, Tin, -1).to(dtype), g.detach().reshape(B, C, K, -1).to(dtype)
    P = xs.shape[3]
    cd = cdf.detach().float()
    if mutant == 'cdf_row0':
        cd = cd[:1].expand(B, K)
    it = time_index_fp32(cd, Tin)
    fl = torch.floor(it)
    i0 = fl.long()
    w1 = it.to(dtype) - fl.to(dtype)
    w0 = 1 - w1
    if mutant == 'swap_w':
        w0, w1 = w1, w0
    y, ymag = torch.zeros(B, C, K, P, dtype=dtype), torch.zeros(B, C, K, P, dtype=dtype)
    gx, gxmag = torch.zeros(B, C, Tin, P, dtype=dtype), torch.zeros(B, C, Tin, P, dtype=dtype)
    ntap = torch.zeros(B, Tin, dtype=torch.float64)
    kk = torch.arange(K).view(1, K)
    frames = []
    for idx, w in ((i0, w0), (i0 + 1, w1)):
        ok = (idx >= 0) & (idx < Tin)
        idc = idx.clamp(0, Tin - 1)
        if mutant == 'clamp_border':
            ok = torch.ones_like(ok)
        fr = torch.gather(xs, 2, idc.view(B, 1, K, 1).expand(B, C, K, P)) * ok.to(dtype).view(B, 1, K, 1)
        frames.append(fr)
        wv = w.view(B, 1, K, 1)
        y += wv * fr
        ymag += wv.abs() * fr.abs()
        hit = ok & (kk < 64) if mutant == 'drop_k64' else ok
        contrib = (w * hit.to(dtype)).view(B, 1, K, 1) * gs
        for b in range(B):
            gx[b].index_add_(1, idc[b], contrib[b])
            gxmag[b].index_add_(1, idc[b], contrib[b].abs())
            ntap[b].index_add_(0, idc[b], hit[b].double())
    ngx = ntap.view(B, 1, Tin, 1).expand(B, C, Tin, P)
    if mutant == 'no_zero_fill':
        gx = torch.where(ngx == 0, torch.ones_like(gx), gx)
    cs = slice(0, time_sample_cchunk(C, P)) if mutant == 'gcdf_first_chunk' else slice(None)
    scale = 1 if mutant == 'gcdf_no_scale' else Tin - 1
    gcdf = scale * (gs * (frames[1] - frames[0]))[:, cs].sum((1, 3))
    gcmag = (Tin - 1) * (gs.abs() * (frames[1].abs() + frames[0].abs())).sum((1, 3))
    osh = tuple(g.shape)
    return {'y': _res(y.view(osh), 2, ymag.view(osh)), 'gx': _res(gx.view(x.shape), ngx.reshape(x.shape), gxmag.view(x.shape)),
            'gcdf': _res(gcdf, -(-C * P // 256) + 8, gcmag), 'i0': i0, 'it': it}


# ---- interp1d -----------------------------------------------------------------------------------------------------------------------------
def interp1d_ref64(x, y, q, g, rows=None, dtype=torch.float64, mutant=None):
    """x, y (B or 1, N), q (B or 1, Pq), g (B, Pq) -> {'ynew': fp64 (B, Pq), 'ind': int64 (B, Pq), 'gx', 'gy', 'gq': Res shaped like the
    inputs}.  ynew = y0 + (y1 - y0) / den * (q - x0), gradients with `ind` held constant; rows = (xrow, yrow, qrow): 0 marks a one-row
    tensor that broadcasts over the B rows of g and whose gradient sums over them"""
    assert mutant is None or mutant in MUTANTS['interp1d'], mutant
    B, Pq = g.shape
    N = x.shape[1]
    if rows is None:
        rows = tuple(int(v.shape[0] > 1) for v in (x, y, q))
    X, Y, Q = x.detach().float().expand(B, N), y.detach().float().expand(B, N), q.detach().float().expand(B, Pq)
    ind = (torch.searchsorted(X.contiguous(), Q.contiguous(), right=(mutant == 'right')) - 1).clamp(0, N - 2)
    x0f, x1f = torch.gather(X, 1, ind), torch.gather(X, 1, ind + 1)
    den = (EPS32 + (x1f - x0f)).to(dtype)                  # the kernel's fp32 denominator: both operations in fp32
    x0, y0, y1 = x0f.to(dtype), torch.gather(Y, 1, ind).to(dtype), torch.gather(Y, 1, ind + 1).to(dtype)
    qv, gv = Q.to(dtype), g.detach().to(dtype)
    dy, dq = y1 - y0, qv - x0
    slope, w1, t = dy / den, dq / den, dy * dq / (den * den)
    ga = gv.abs()

    def knots(left, right):
        out = torch.zeros(B, N, dtype=left.dtype)
        out.scatter_add_(1, ind, left)
        out.scatter_add_(1, ind + 1, right)
        return out

    def fold(v, full):
        return v if full else (v[:1].clone() if mutant == 'bcast_b0' else v.sum(0, keepdim=True))

    def count(v, full):
        return v if full else v.sum(0, keepdim=True)

    one = torch.ones(B, Pq, dtype=torch.float64)
    nk = knots(one, one)
    return {'ynew': (y0 + slope * dq).double(), 'ind': ind,
            'gx': _res(fold(knots(gv * (t - slope), -gv * t), rows[0]), count(nk, rows[0]),
                       count(knots(ga * (t.abs() + slope.abs()), ga * t.abs()), rows[0])),
            'gy': _res(fold(knots(gv * (1 - w1), gv * w1), rows[1]), count(nk, rows[1]),
                       count(knots(ga * (1 + w1.abs()), ga * w1.abs()), rows[1])),
            'gq': _res(fold(gv * slope, rows[2]), count(one, rows[2]), count(ga * slope.abs(), rows[2]))}


# ---- time_resize --------------------------------------------------------------------------------------------------------------------------
def resize_src_fp32(Kin, L, ac, clamp0=True):
    """the fp32 source coordinate of every output frame, as resize_src() of csrc/resize_src.h computes it -> fp32 (L,)"""
    j = torch.arange(L)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    if ac:
        scale = f32(Kin - 1) / f32(L - 1) if L > 1 else f32(0)
        return scale * j.float()
    scale = f32(Kin) / f32(L)
    src = (scale.double() * (j.double() + 0.5) - 0.5).float()          # one FMA: the exact product-sum rounded once
    return src.clamp_min(0) if clamp0 else src


def time_resize_ref64(x, L, ac, g, dtype=torch.float64, mutant=None):
    """x (B, C, Kin, *), g (B, C, L, *) -> {'y', 'gx': Res, 'src': fp32 (L,), 'i0', 'i1': int64 (L,)}: y = l0 x[i0] + l1 x[i1]"""
    assert mutant is None or mutant in MUTANTS['time_resize'], mutant
    B, C, Kin = x.shape[:3]
    xs, gs = x.detach().reshape(B, C, Kin, -1).to(dtype), g.detach().reshape(B, C, L, -1).to(dtype)
    src = resize_src_fp32(Kin, L, ac, clamp0=(mutant != 'no_clamp0'))
    i0 = src.long()                                        # C's float -> int conversion: towards zero
    i1 = i0 + (i0 < Kin - 1).long()
    ok1 = torch.ones(L, dtype=dtype)
    if mutant == 'no_clamp_i1':                            # the frame past the end reads as zero
        ok1 = (i0 + 1 < Kin).to(dtype)
    l1 = (src - i0.float()).to(dtype)
    l0 = 1 - l1
    l1 = l1 * ok1
    v = lambda w: w.view(1, 1, L, 1)
    y = v(l0) * xs[:, :, i0] + v(l1) * xs[:, :, i1]
    ymag = v(l0.abs()) * xs[:, :, i0].abs() + v(l1.abs()) * xs[:, :, i1].abs()
    gx, gxmag, n = torch.zeros_like(xs), torch.zeros_like(xs), torch.zeros(Kin, dtype=torch.float64)
    for idx, w, cnt in ((i0, l0, torch.ones(L, dtype=torch.float64)), (i1, l1, ok1.double())):
        gx.index_add_(2, idx, v(w) * gs)
        gxmag.index_add_(2, idx, v(w.abs()) * gs.abs())
        n.index_add_(0, idx, cnt)
    return {'y': _res(y.view(g.shape), 2, ymag.view(g.shape)),
            'gx': _res(gx.view(x.shape), n.view(1, 1, Kin, 1).expand_as(xs).reshape(x.shape), gxmag.view(x.shape)),
            'src': src, 'i0': i0, 'i1': i1}


# ---- time_pool ----------------------------------------------------------------------------------------------------------------------------
def time_pool_ref64(x, mode, R, g, dtype=torch.float64, mutant=None):
    """x (B, C, T, *), g (B, C, T // R, *) -> {'y', 'gx': Res, 'ties': bool (B, C, T // R, *), windows whose maximum is reached more than
    once}.  avg: n = R + 1 (R - 1 additions, the division, the store) for y, one rounding of g / R for gx (n = -7: (n + 8) 2^-24 is half an
    ulp); max: exact (n = -8: the bound is zero), the gradient to the first maximal frame; frames beyond R (T // R) get zero"""
    assert mode in ('avg', 'max') and (mutant is None or mutant in MUTANTS['time_pool']), (mode, mutant)
    B, C, T = x.shape[:3]
    K = T // R
    sp = tuple(x.shape[3:])
    xs = x.detach()[:, :, :K * R].reshape((B, C, K, R) + sp).to(dtype)
    gs = g.detach().to(dtype).unsqueeze(3)
    gx = torch.zeros(x.shape, dtype=dtype)
    top = xs.max(3, keepdim=True).values
    eq = xs == top
    ties = eq.sum(3) > 1
    if mode == 'avg':
        y, ymag = xs.sum(3) / R, xs.abs().sum(3) / R
        gx[:, :, :K * R] = (gs / R).expand_as(xs).reshape((B, C, K * R) + sp)
        return {'y': _res(y, R + 1, ymag), 'gx': _res(gx, -7, gx.abs()), 'ties': ties}
    if mutant == 'last_max':
        first = eq & (eq.flip(3).cumsum(3).flip(3) == 1)
    else:
        first = eq & (eq.cumsum(3) == 1)
    gx[:, :, :K * R] = (first.to(dtype) * gs).reshape((B, C, K * R) + sp)
    y = top.squeeze(3)
    return {'y': _res(y, -8, y.abs()), 'gx': _res(gx, -8, gx.abs()), 'ties': ties}


# ---- grid_cdf -----------------------------------------------------------------------------------------------------------------------------
def grid_cdf_expr(z):
    """x3d_coarse.py:384-392 (= oracle.x3d_ref.grid_cdf) in the dtype of z, differentiable"""
    p = 1. - torch.sigmoid(z * 5e-1)
    p = p / (torch.sum(p, dim=1, keepdim=True) + 1e-16)
    return torch.cat([torch.zeros(z.shape[0], 1, dtype=z.dtype), torch.cumsum(p, dim=1)], dim=1)


def grid_cdf_ref64(g, bias, gc, dtype=torch.float64, expr=grid_cdf_expr):
    """g (B, Kin) logits, bias (1,) or None, gc (B, Kin + 1) -> {'cdf', 'gg', 'gb' (None without a bias)}: fp64 tensors.  dtype=float32 with
    expr=oracle.x3d_ref.grid_cdf is the fp32 CPU expression the kernel's error is measured against"""
    gl = g.detach().to(dtype).requires_grad_(True)
    bl = None if bias is None else bias.detach().to(dtype).requires_grad_(True)
    cdf = expr(gl if bl is None else gl + bl)
    grads = torch.autograd.grad((cdf * gc.detach().to(dtype)).sum(), [gl] if bl is None else [gl, bl])
    return {'cdf': cdf.detach().double(), 'gg': grads[0].double(), 'gb': None if bl is None else grads[1].double()}


# ==== the cases of tests/test_hip_temporal.py (inputs on the CPU, shared, never modified) =====================================================
def _seed(*ints):
    s = 17
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# name -> (B, C, Tin, K, trailing dims); P = their product
TS_CASES = {
    'A': (3, 2, 16, 5, (30,)),          # scalar route, one ballot round (the gridsample_ulp shape)
    'B': (2, 3, 8, 17, (4, 4)),         # float4 route, 5-D input
    'C': (1, 2, 6, 3, (1028,)),         # float4, two workgroups per plane, the second with one active thread
    'D': (1, 2, 6, 3, (257,)),          # scalar, two workgroups
    'E': (2, 2, 5, 64, (4,)),           # exactly one ballot round
    'F': (2, 2, 5, 65, (4,)),           # two rounds, the second with one lane
    'G': (1, 1, 7, 130, (3,)),          # three rounds, ragged; a dozen or more taps per frame
    'H': (2, 2, 40, 3, (8,)),           # most frames have no tap
    'I': (1, 2, 6, 8, (4,)),            # taps outside [0, Tin), exact knots at both ends
    'J': (1, 2, 9, 12, (4,)),           # runs of equal CDF values: all taps on one frame pair
    'K1': (2, 2, 1, 4, (4,)),           # Tin = 1: gcdf exactly 0
    'K2': (1, 2, 2, 3, (8,)),           # Tin = 2
    'L': (2, 2, 5, 1, (4,)),            # K = 1
    'M': (1, 5, 3, 2, (4096,)),         # cchunk = 4: two chunks, the second holding one channel
    'M1': (1, 2, 2, 2, (16384,)),       # cchunk = 1
}
TS_CDF = {'I': [[-0.5, -0.1, 0.0, 0.3, 1.0, 1.0 + 2.0 ** -23, 1.1, 1.7]], 'J': [[0.3] * 5 + [0.35] * 7]}
TS_I0 = {'I': [[-3, -1, 0, 1, 5, 5, 5, 8]], 'J': [[2] * 12]}           # checked by hand
TS_MUTANTS = {'A': ('swap_w', 'cdf_row0', 'gcdf_no_scale'), 'B': ('swap_w', 'cdf_row0'), 'F': ('drop_k64',), 'G': ('drop_k64',),
              'H': ('no_zero_fill',), 'I': ('clamp_border',), 'M': ('gcdf_first_chunk',)}


@functools.lru_cache(maxsize=None)
def ts_inputs(name):
    """-> (x, cdf, g) fp32: x and g randn; CDF rows (different per batch row) 0 = c_0 < c_1 < ... ~ 1, sorted rand for K <= 2, or the
    case's own knots"""
    B, C, Tin, K, sp = TS_CASES[name]
    gen = _seed(1, *[ord(ch) for ch in name])
    x, g = torch.randn((B, C, Tin) + sp, generator=gen), torch.randn((B, C, K) + sp, generator=gen)
    if name in TS_CDF:
        cdf = torch.tensor(TS_CDF[name], dtype=torch.float32)
    elif K <= 2:                        # too few knots for a leading 0 and a trailing 1: they would all sit exactly on frames
        cdf = torch.sort(torch.rand(B, K, generator=gen), 1)[0]
    else:
        p = torch.rand(B, K - 1, generator=gen) + 0.05
        cdf = torch.cat([torch.zeros(B, 1), torch.cumsum((p / p.sum(1, keepdim=True)).double(), 1).float()], 1)
    assert tuple(cdf.shape) == (B, K) and bool(torch.isfinite(cdf).all())
    return x, cdf, g


@functools.lru_cache(maxsize=None)
def ts_reference(name):
    return time_sample_ref64(*ts_inputs(name))


# interp1d: N knots, Pq queries, B = 4 rows (or 1)
I1_N, I1_PQ, I1_B = (2, 17, 65), (1, 23, 300), 4
I1_KNOTS = ('random', 'runs')
I1_ROWS = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]      # (0, 0, 0): B = 1


def i1_mutants(N, Pq, rows):
    """'right' needs queries on interior knots (N = 2 clamps every index to 0; Pq = 1 puts its on-knot query on knot 0, where both sides
    clamp to the same bin); 'bcast_b0' needs a broadcast row"""
    m = []
    if N > 2 and Pq > 1:
        m.append('right')
    if 0 in rows and any(rows):
        m.append('bcast_b0')
    return tuple(m)


@functools.lru_cache(maxsize=None)
def i1_inputs(N, Pq, kind, rows):
    """-> (x, y, q, g) fp32.  Knots: sorted rand ('random') or the same with runs of equal knots, at both ends too ('runs'); y randn;
    queries cycle through: inside the range, exactly on a knot (the first, the last, then random ones), below the first knot, above the
    last one (a one-query row starts the cycle at its row number); g randn"""
    B = I1_B if any(rows) else 1
    gen = _seed(2, N, Pq, I1_KNOTS.index(kind))
    X = torch.sort(torch.rand(I1_B, N, generator=gen), 1)[0]
    if kind == 'runs':
        X = X[:, torch.arange(N) * 3 // 5]
        X[:, -1] = X[:, -2]
    Y = torch.randn(I1_B, N, generator=gen)
    Q = torch.empty(I1_B, Pq)
    u = torch.rand(I1_B, Pq, generator=gen)
    pick = torch.randint(0, N, (I1_B, Pq), generator=gen)
    for b in range(I1_B):
        kn = X[b if rows[0] else 0]
        lo, hi = float(kn[0]), float(kn[-1])
        for j in range(Pq):
            what, m = (j + b) % 4, j // 4
            if what == 0:
                Q[b, j] = lo + (hi - lo) * float(u[b, j])
            elif what == 1:
                Q[b, j] = kn[0 if m == 0 else (N - 1 if m == 1 else int(pick[b, j]))]
            elif what == 2:
                Q[b, j] = lo - 0.01 - 0.3 * float(u[b, j])
            else:
                Q[b, j] = hi + 0.01 + 0.3 * float(u[b, j])
    g = torch.randn(I1_B, Pq, generator=gen)[:B]
    take = lambda v, full: v[:B].contiguous() if full else v[:1].contiguous()
    return take(X, rows[0]), take(Y, rows[1]), take(Q, rows[2]), g.contiguous()


@functools.lru_cache(maxsize=None)
def i1_reference(N, Pq, kind, rows):
    return interp1d_ref64(*i1_inputs(N, Pq, kind, rows), rows=rows)


# time_resize: (input shape, L), each with align_corners True and False
TR_CASES = [((1, 2, 1), 5), ((2, 3, 7), 1), ((1, 2, 64), 3), ((1, 1, 2), 1000), ((1, 2, 5, 3, 3), 12), ((2, 7, 17), 64)]


def tr_mutants(shape, L, ac):
    """'no_clamp0': half-pixel upsampling puts the first source coordinate below 0; 'no_clamp_i1': half-pixel puts the last one past
    Kin - 1 (with align_corners the weight of the frame past the end is 0 or a rounding of it: not visible, by design)"""
    Kin = shape[2]
    return () if ac or not L > Kin > 1 else ('no_clamp0', 'no_clamp_i1')      # Kin = 1: both taps are frame 0 and l0 + l1 = 1 either way


@functools.lru_cache(maxsize=None)
def tr_inputs(shape, L):
    gen = _seed(3, L, *shape)
    return torch.randn(shape, generator=gen), torch.randn(tuple(shape[:2]) + (L,) + tuple(shape[3:]), generator=gen)


@functools.lru_cache(maxsize=None)
def tr_reference(shape, L, ac):
    x, g = tr_inputs(shape, L)
    return time_resize_ref64(x, L, ac, g)


# time_pool: (B, C, T, H, W, R)
TP_CASES = [(2, 3, 14, 5, 7, 4), (1, 2, 4, 1, 1, 4), (1, 2, 9, 17, 17, 4), (1, 1, 6, 3, 3, 1), (1, 2, 7, 3, 3, 3)]
# seed offsets: the smallest at which a quarter of the max windows hold a tie (the rate of this distribution is ~0.3; the first case has two
# windows only and none ties at offset 0, the second has 36 and 7 tie at offset 0)
TP_SEED = {(1, 2, 4, 1, 1, 4): 1, (1, 2, 7, 3, 3, 3): 1}


@functools.lru_cache(maxsize=None)
def tp_inputs(case):
    """relu(randn) rounded to multiples of 0.5 (post-ReLU activations are full of exact zeros: ties are the normal case), g randn"""
    B, C, T, H, W, R = case
    gen = _seed(4, TP_SEED.get(case, 0), *case)
    x = torch.round(torch.relu(torch.randn(B, C, T, H, W, generator=gen)) * 2) / 2
    return x, torch.randn(B, C, T // R, H, W, generator=gen)


@functools.lru_cache(maxsize=None)
def tp_reference(case, mode):
    x, g = tp_inputs(case)
    return time_pool_ref64(x, mode, case[5], g)


# grid_cdf: (B, Kin), each with a bias tensor and with bias=None
GC_CASES = [(65, 4), (130, 33), (3, 1)]
GC_BIAS = 0.25


@functools.lru_cache(maxsize=None)
def gc_inputs(B, Kin, with_bias):
    """logits randn * 2 clamped to [-6, 6], gc randn"""
    gen = _seed(5, B, Kin)
    g = (torch.randn(B, Kin, generator=gen) * 2).clamp(-6, 6)
    gc = torch.randn(B, Kin + 1, generator=gen)
    return g, (torch.tensor([GC_BIAS]) if with_bias else None), gc


@functools.lru_cache(maxsize=None)
def gc_reference(B, Kin, with_bias):
    return grid_cdf_ref64(*gc_inputs(B, Kin, with_bias))


@functools.lru_cache(maxsize=None)
def gc_baseline(B, Kin, with_bias):
    """the fp32 CPU expression oracle.x3d_ref.grid_cdf (autograd for the gradients): its distance from the fp64 reference is the fp32 error
    of the operation itself, the yardstick the kernel's expf arithmetic is judged by"""
    from oracle import x3d_ref as R
    return grid_cdf_ref64(*gc_inputs(B, Kin, with_bias), dtype=torch.float32, expr=R.grid_cdf)


def maxrel(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.detach().double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-300))
