"""tests/temporal_ref64.py (the fp64 references csrc/gridpool.hip is checked against by tests/test_hip_temporal.py) pinned to stock torch in
float64, and its elementwise bounds shown to discriminate.  CPU only.

Pinning.  Both sides are fp64 and differ in summation order only: 1e-12 relative to each tensor's max.  That needs both sides to take the same
fp32-derived decisions AND coordinates:
    time_sample   F.grid_sample(align_corners=True) on a 5-D input of height and width 1 (the plane positions ride in the batch), fed the
                  temporal coordinate 2 it / (Tin - 1) - 1 rebuilt in fp64 from the reference's own fp32 `it`; d/d cdf = (Tin - 1) d/d it.
                  (Feeding the fp64 CDF instead moves `it` by an fp32 rounding: 5e-7.)
    time_resize   F.interpolate on doubles at sizes whose scale is a power of two, so that the fp32 source coordinate IS the fp64 one
                  (asserted, with the weaker condition that both floor to the same frame)
    time_pool     F.avg_pool3d / F.max_pool3d on doubles, on the tie-laden inputs of the GPU cases
    interp1d      autograd of the oracle.x3d_ref.interp1d expression in float64 on row-expanded inputs.  The oracle takes eps from the dtype, so
                  the expression is restated here with the fp32 eps (and shown bit-equal to the oracle on fp32 inputs); knots are multiples
                  of 2^-8, which makes the fp32 denominator eps + (x1 - x0) exact
    grid_cdf      the reference IS autograd of the oracle's expression in fp64 (restated, because the oracle stores into an fp32 buffer; shown
                  bit-equal to it on fp32 inputs); its gradient is pinned to the closed form the kernel uses

Bounds are not too tight: the same expression in plain fp32 torch lies within the bound of every GPU case.
Bounds are not too loose: each mutant of temporal_ref64.MUTANTS, applied to the fp64 reference, leaves the bound of every case that names it."""
import pytest
import torch
import torch.nn.functional as F

import temporal_ref64 as T
from oracle import x3d_ref as R

TOL = 1e-12


def _close(name, got, ref):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    err, top = float((got - ref).detach().abs().max()), float(ref.detach().abs().max())
    assert err <= TOL * top, (name, err, top)


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- pinning ------------------------------------------------------------------------------------------------------------------------------
def _grid_sample_time(x, it, g):
    """F.grid_sample in fp64 along t only -> (y, gx, gcdf); x (B, C, Tin, P), it (B, K) fp32 frame coordinates, g (B, C, K, P)"""
    B, C, Tin, P = x.shape
    K = it.shape[1]
    x5 = x.double().permute(0, 3, 1, 2).reshape(B * P, C, Tin, 1, 1).requires_grad_(True)
    itl = it.double().requires_grad_(True)
    z = (2 * itl / (Tin - 1) - 1).repeat_interleave(P, 0)
    grid = torch.stack([torch.zeros_like(z), torch.zeros_like(z), z], -1).view(B * P, K, 1, 1, 3)
    y = F.grid_sample(x5, grid, align_corners=True).view(B, P, C, K).permute(0, 2, 3, 1)
    gx5, git = torch.autograd.grad((y * g.double()).sum(), [x5, itl])
    return y.detach(), gx5.view(B, P, C, Tin).permute(0, 2, 3, 1), git * (Tin - 1)


@pytest.mark.parametrize('B,C,Tin,K,P,lo,hi', [(2, 3, 6, 5, 7, 0.0, 1.0), (1, 2, 9, 70, 3, 0.0, 1.0), (1, 1, 7, 130, 2, 0.0, 1.0),
                                               (2, 2, 5, 9, 4, -0.3, 1.3)])
def test_time_sample_ref64_matches_grid_sample(B, C, Tin, K, P, lo, hi):
    """K = 70 and 130 (several ballot rounds in the kernel) and taps outside [0, Tin) included; the first and the last knot sit exactly on
    frames 0 and Tin - 1 (cdf 0 and 1), where the slope is the one of the floor-side segment on both sides"""
    x, g = _rnd(1, B, C, Tin, P), _rnd(2, B, C, K, P)
    cdf = torch.sort(torch.rand(B, K, generator=torch.Generator().manual_seed(3)) * (hi - lo) + lo, 1)[0]
    if lo == 0.0:
        cdf[:, 0], cdf[:, -1] = 0.0, 1.0
    else:
        cdf[:, 0], cdf[:, -1] = -0.45, 1.4
    ref = T.time_sample_ref64(x, cdf, g)
    i0, w1 = R.grid_sample_time_index(cdf, Tin)          # the reference's fp32 index arithmetic is the oracle's
    assert torch.equal(ref['i0'], i0.long()) and torch.equal(ref['it'] - torch.floor(ref['it']), w1)
    if lo < 0.0:
        assert bool((ref['i0'] < -1).any()) and bool((ref['i0'] >= Tin).any())
    y, gx, gcdf = _grid_sample_time(x, ref['it'], g)
    _close('y', ref['y'].val, y)
    _close('gx', ref['gx'].val, gx)
    _close('gcdf', ref['gcdf'].val, gcdf)


def test_time_sample_ref64_single_frame():
    """Tin = 1 (grid_sample's normalised coordinate does not exist): every tap is frame 0 with weight 1, gcdf is exactly zero"""
    x, cdf, g = T.ts_inputs('K1')
    ref = T.ts_reference('K1')
    assert torch.equal(ref['y'].val, x.double().expand(-1, -1, 4, -1).contiguous())
    _close('gx', ref['gx'].val, g.double().sum(2, keepdim=True))
    assert bool((ref['gcdf'].val == 0).all()) and bool((ref['gcdf'].mag == 0).all())


TR_PIN = [((2, 3, 5), 17, True), ((1, 2, 17), 5, True), ((1, 2, 9, 2, 2), 3, True), ((1, 2, 1), 4, True), ((1, 2, 6), 1, True),
          ((2, 3, 4), 16, False), ((1, 2, 16), 4, False), ((1, 2, 3), 12, False), ((1, 2, 8), 2, False), ((1, 2, 5), 5, False),
          ((1, 2, 3, 2, 2), 6, False)]


@pytest.mark.parametrize('shape,L,ac', TR_PIN)
def test_time_resize_ref64_matches_interpolate(shape, L, ac):
    Kin = shape[2]
    x, g = _rnd(4, *shape), _rnd(5, *(shape[:2] + (L,) + shape[3:]))
    ref = T.time_resize_ref64(x, L, ac, g)
    j = torch.arange(L, dtype=torch.float64)
    src64 = j * ((Kin - 1) / (L - 1) if L > 1 else 0.0) if ac else ((j + 0.5) * (Kin / L) - 0.5).clamp_min(0)
    assert torch.equal(torch.floor(ref['src'].double()), torch.floor(src64)), 'fp32 and fp64 source coordinates floor to different frames'
    assert torch.equal(ref['src'].double(), src64), 'not a power-of-two scale: the fp32 weights differ from the fp64 ones by a rounding'
    xl = x.double().requires_grad_(True)
    if len(shape) == 3:
        y = F.interpolate(xl, L, mode='linear', align_corners=ac)
    else:
        y = F.interpolate(xl, (L,) + shape[3:], mode='trilinear', align_corners=ac)
    (gx,) = torch.autograd.grad((y * g.double()).sum(), [xl])
    _close('y', ref['y'].val, y.detach())
    _close('gx', ref['gx'].val, gx)


@pytest.mark.parametrize('mode', ['avg', 'max'])
@pytest.mark.parametrize('case', T.TP_CASES)
def test_time_pool_ref64_matches_pool3d(case, mode):
    """on the GPU cases' own inputs: at least a quarter of the max windows hold a tie (R > 1), and stock torch routes the gradient of a tie
    to the first maximal frame"""
    x, g = T.tp_inputs(case)
    R_ = case[5]
    ref = T.tp_reference(case, mode)
    if R_ > 1:
        assert float(ref['ties'].double().mean()) >= 0.25, float(ref['ties'].double().mean())
    xl = x.double().requires_grad_(True)
    pool = F.avg_pool3d if mode == 'avg' else F.max_pool3d
    y = pool(xl, (R_, 1, 1), stride=(R_, 1, 1))
    (gx,) = torch.autograd.grad((y * g.double()).sum(), [xl])
    _close('y', ref['y'].val, y.detach())
    _close('gx', ref['gx'].val, gx)
    if mode == 'max':
        assert torch.equal(ref['y'].val, y.detach()) and torch.equal(ref['gx'].val, gx)
        assert bool((ref['gx'].val[:, :, R_ * (case[2] // R_):] == 0).all())


def _interp1d_expr(X, Y, Q, eps):
    """oracle.x3d_ref.interp1d (interp1d.py:100-141) on row-expanded 2-D inputs, with eps given instead of taken from the dtype"""
    ind = (torch.searchsorted(X.detach().contiguous(), Q.detach().contiguous()) - 1).clamp(0, X.shape[1] - 2)
    sel = lambda v: torch.gather(v, 1, ind)
    slopes = (Y[:, 1:] - Y[:, :-1]) / (eps + (X[:, 1:] - X[:, :-1]))
    return sel(Y) + sel(slopes) * (Q - sel(X)), ind


@pytest.mark.parametrize('rows', T.I1_ROWS)
def test_interp1d_ref64_matches_oracle_expression(rows):
    B, N, Pq = (3 if any(rows) else 1), 9, 11
    gen = torch.Generator().manual_seed(6)
    X = torch.sort(torch.randint(0, 256, (3, N), generator=gen), 1)[0].float() / 256       # repeated knots occur
    X[:, 3] = X[:, 4]
    Y, g = torch.randn(3, N, generator=gen), torch.randn(3, Pq, generator=gen)[:B]
    Q = torch.rand(3, Pq, generator=gen) * 1.2 - 0.1
    Q[:, 2], Q[:, 5], Q[:, 7] = X[:, 0], X[:, 4], X[:, -1]                                 # queries exactly on knots
    take = lambda v, full: v[:B].contiguous() if full else v[:1].contiguous()
    x, y, q = take(X, rows[0]), take(Y, rows[1]), take(Q, rows[2])
    d32 = T.EPS32 + (X[:, 1:] - X[:, :-1])
    assert torch.equal(d32.double(), T.EPS32 + (X[:, 1:].double() - X[:, :-1].double())), 'the fp32 denominator is not exact on these knots'
    ref = T.interp1d_ref64(x, y, q, g, rows=rows)
    ex = [v.expand(B, v.shape[1]).contiguous() for v in (x, y, q)]
    y32, i32 = _interp1d_expr(*ex, torch.finfo(torch.float32).eps)
    yo, io = R.interp1d(*ex)
    assert torch.equal(y32, yo) and torch.equal(i32, io), 'the restated expression is not the oracle'
    leaves = [v.double().requires_grad_(True) for v in ex]
    y64, i64 = _interp1d_expr(*leaves, T.EPS32)
    assert torch.equal(i64, ref['ind']) and torch.equal(i32, ref['ind'])
    grads = torch.autograd.grad((y64 * g.double()).sum(), leaves)
    _close('ynew', ref['ynew'], y64.detach())
    for k, gr, full in zip(('gx', 'gy', 'gq'), grads, rows):
        _close(k, ref[k].val, gr if full else gr.sum(0, keepdim=True))


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('B,Kin', T.GC_CASES)
def test_grid_cdf_ref64_matches_oracle_expression(B, Kin, with_bias):
    g, bias, gc = T.gc_inputs(B, Kin, with_bias)
    z = g if bias is None else g + bias
    assert torch.equal(T.grid_cdf_expr(z), R.grid_cdf(z)), 'the restated expression is not the oracle'
    ref = T.gc_reference(B, Kin, with_bias)
    z64 = z.double() if bias is None else g.double() + bias.double()
    q = 1.0 - torch.sigmoid(0.5 * z64)
    dn = q.sum(1, keepdim=True) + 1e-16
    _close('cdf', ref['cdf'], torch.cat([torch.zeros(B, 1, dtype=torch.float64), torch.cumsum(q / dn, 1)], 1))
    suf = gc.double()[:, 1:].flip(1).cumsum(1).flip(1)               # d loss / d p_i = sum_{k > i} gc_k
    gq = suf / dn - (suf * q).sum(1, keepdim=True) / dn ** 2
    gg = gq * (-0.5 * (1.0 - q) * q)
    if Kin > 1:                                                      # Kin = 1: p = q / (q + 1e-16), the gradient is cancellation noise ~1e-16
        _close('gg', ref['gg'], gg)
    else:
        assert float(ref['gg'].abs().max()) <= 1e-13 * float(gc.abs().max())
    assert bool((ref['cdf'][:, 0] == 0).all()) and bool((ref['cdf'][:, 1:] >= ref['cdf'][:, :-1]).all())
    if with_bias and Kin > 1:
        _close('gb', ref['gb'], gg.sum().view(1))


def test_grid_cdf_cpu_expression_saturates_exactly():
    """the two saturated inputs of the GPU test on the fp32 CPU expression: +200 gives q = 0 (every knot 0), -200 gives q = 1 exactly"""
    assert bool((R.grid_cdf(torch.full((3, 5), 200.0)) == 0).all())
    lo = R.grid_cdf(torch.full((3, 5), -200.0))
    assert float(lo[0, -1]) == 1.0 and torch.equal(lo[:, 1], torch.full((3,), 0.2))


# ---- the bounds: the fp32 expression inside, every mutant outside ---------------------------------------------------------------------------
def _inside(tag, got, ref, keys):
    for k in keys:
        r = T.ratio(got[k].val, ref[k])
        assert r <= 1.0, ('plain fp32 torch is outside the bound', tag, k, r)


def _outside(tag, got, ref, keys):
    worst = max(T.ratio(got[k].val, ref[k]) for k in keys)
    assert worst > 1.0, ('mutant within the bound: the inputs of this case do not discriminate', tag, worst)


TS_KEYS = ('y', 'gx', 'gcdf')


@pytest.mark.parametrize('name', sorted(T.TS_CASES))
def test_time_sample_bounds(name):
    x, cdf, g = T.ts_inputs(name)
    ref = T.ts_reference(name)
    if name in T.TS_I0:
        assert ref['i0'].tolist() == T.TS_I0[name]
    B, C, Tin, K, sp = T.TS_CASES[name]
    taps = ref['gx'].n[:, 0, :, 0]
    if name == 'G':
        assert float(taps.min()) >= 12
    if name == 'H':
        assert float((taps == 0).double().mean()) > 0.5
    if name == 'M':
        assert T.time_sample_cchunk(C, sp[0]) == 4
    if name == 'M1':
        assert T.time_sample_cchunk(C, sp[0]) == 1
    if B > 1 and K > 1:
        assert not torch.equal(cdf[0], cdf[1])
    _inside(name, T.time_sample_ref64(x, cdf, g, dtype=torch.float32), ref, TS_KEYS)
    for m in T.TS_MUTANTS.get(name, ()):
        _outside((name, m), T.time_sample_ref64(x, cdf, g, mutant=m), ref, TS_KEYS)


def test_time_sample_every_mutant_is_named():
    assert set(m for v in T.TS_MUTANTS.values() for m in v) == set(T.MUTANTS['time_sample'])


I1_KEYS = ('gx', 'gy', 'gq')


@pytest.mark.parametrize('kind', T.I1_KNOTS)
@pytest.mark.parametrize('Pq', T.I1_PQ)
@pytest.mark.parametrize('N', T.I1_N)
def test_interp1d_bounds(N, Pq, kind):
    named = set()
    for rows in T.I1_ROWS:
        x, y, q, g = T.i1_inputs(N, Pq, kind, rows)
        ref = T.i1_reference(N, Pq, kind, rows)
        assert tuple(ref['gx'].val.shape) == tuple(x.shape) and tuple(ref['gq'].val.shape) == tuple(q.shape)
        _inside((N, Pq, kind, rows), T.interp1d_ref64(x, y, q, g, rows=rows, dtype=torch.float32), ref, I1_KEYS)
        for m in T.i1_mutants(N, Pq, rows):
            named.add(m)
            _outside((N, Pq, kind, rows, m), T.interp1d_ref64(x, y, q, g, rows=rows, mutant=m), ref, I1_KEYS)
    if N > 2 and Pq > 1:
        assert named == set(T.MUTANTS['interp1d'])


@pytest.mark.parametrize('ac', [True, False])
@pytest.mark.parametrize('shape,L', T.TR_CASES)
def test_time_resize_bounds(shape, L, ac):
    x, g = T.tr_inputs(shape, L)
    ref = T.tr_reference(shape, L, ac)
    _inside((shape, L, ac), T.time_resize_ref64(x, L, ac, g, dtype=torch.float32), ref, ('y', 'gx'))
    for m in T.tr_mutants(shape, L, ac):
        _outside((shape, L, ac, m), T.time_resize_ref64(x, L, ac, g, mutant=m), ref, ('y', 'gx'))


def test_time_resize_every_mutant_is_named():
    assert set(m for (s, L) in T.TR_CASES for ac in (True, False) for m in T.tr_mutants(s, L, ac)) == set(T.MUTANTS['time_resize'])


@pytest.mark.parametrize('case', T.TP_CASES)
def test_time_pool_bounds(case):
    x, g = T.tp_inputs(case)
    Rr = case[5]
    ref = T.tp_reference(case, 'avg')
    _inside((case, 'avg'), T.time_pool_ref64(x, 'avg', Rr, g, dtype=torch.float32), ref, ('y', 'gx'))
    ref = T.tp_reference(case, 'max')
    _inside((case, 'max'), T.time_pool_ref64(x, 'max', Rr, g, dtype=torch.float32), ref, ('y', 'gx'))
    if Rr > 1:
        _outside((case, 'last_max'), T.time_pool_ref64(x, 'max', Rr, g, mutant='last_max'), ref, ('gx',))
