"""The temporal resampling kernels of csrc/gridpool.hip -- time_sample (fwd, bwd_x, bwd_cdf), interp1d (fwd, bwd), time_resize (fwd, bwd),
time_pool (fwd, bwd), grid_cdf (fwd, bwd) -- against the fp64 references of tests/temporal_ref64.py (pinned to stock torch, and their bounds
shown to discriminate, by tests/test_temporal_ref64_cpu.py), at the shapes that reach every branch of the kernels.  The cases and what each
one reaches are listed next to their inputs in temporal_ref64.py.

Bounds.  Unless stated, elementwise: |kernel - ref| <= (n + 8) * 2^-24 * mag, with n the number of fp32 summands of the element and mag the
sum of their absolute values; an element without a summand must be an exact zero.  The worst err / bound of every case goes to the junit
report (temporal_fp64).  grid_cdf goes through expf, so its bound is measured: 4 x the error of the fp32 CPU expression against the fp64
reference + 2^-23, relative to each tensor's max (the bn_fold gate rule).

Largest err / bound seen on an MI355X, per op and output (1.0 is the bound): time_sample y 0.18, gx 0.18, gcdf 0.12; interp1d gx 0.32,
gy 0.17, gq 0.27 (the same bits as the plain fp32 torch expression on the CPU); time_resize y 0.19, gx 0.15; time_pool avg y 0.05, gx 0.63
(its bound is half an ulp), max bit-equal.  grid_cdf, kernel error / fp32 CPU expression's error, max-normalised: cdf 2.4e-7 / 1.3e-7
(130 x 33; 0.37 of the allowance), 1.0e-7 / 1.0e-7 (65 x 4: the same bits); gg 4.1e-7 / 4.1e-7 (65 x 4), 2.0e-7 / 1.9e-7 (130 x 33);
gb 1.8e-6 / 9.9e-6 (130 x 33), 7.1e-8 / 2.0e-7 (65 x 4).

The checks were also run once against a kernel build with four deliberate errors (taps k >= 64 left out of gx, the max gradient to the last
maximal frame, a broadcast query row's gradient from b = 0 only, gcdf scaled by Tin): every one was caught, at 3e2 .. 1e6 x the bound."""
import pytest
import torch

import temporal_ref64 as T

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U23 = 2.0 ** -23
NAN = float('nan')


def ops():
    from cfn_hip import ops as o
    return o


def dv(v, grad=False):
    return v.clone().to(DEV).requires_grad_(grad)


def check(record, tag, got, ref, keys):
    """every output in keys within its elementwise bound; the worst err / bound per output goes to the junit report"""
    worst = {k: T.ratio(got[k], ref[k]) for k in keys}
    if record is not None:
        record('temporal_fp64', repr(dict(case=tag, worst=worst)))
    for k in keys:
        assert got[k].dtype == torch.float32, (tag, k, got[k].dtype)
        assert worst[k] <= 1.0, (tag, k, worst[k])
    return worst


# ---- time_sample --------------------------------------------------------------------------------------------------------------------------
def ts_run(name, need_x=True, need_cdf=True):
    x, cdf, g = T.ts_inputs(name)
    xg, cg = dv(x, need_x), dv(cdf, need_cdf)
    y = ops().time_sample(xg, cg)
    grads = torch.autograd.grad(y, [v for v in (xg, cg) if v.requires_grad], dv(g))
    got = {'y': y.detach()}
    got.update(zip([k for k, need in (('gx', need_x), ('gcdf', need_cdf)) if need], grads))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize('name', sorted(T.TS_CASES))
def test_time_sample_fp64(name, record_property):
    """forward, gx and gcdf of every case of temporal_ref64.TS_CASES: the float4 and the scalar route, planes of more than one workgroup,
    one / two / three ballot rounds of the tap compaction (K = 64, 65, 130), a dozen taps on a frame, frames without a tap (exact zeros),
    taps outside [0, Tin), exact knots, Tin = 1 (gcdf exactly 0) and 2, K = 1, one / two ragged / single-channel chunks of the gcdf kernel.
    y: n = 2; gx: n = the taps on the frame; gcdf: n = ceil(C P / 256) + 8 (one thread's share + the wave tree),
    mag = (Tin - 1) sum |g| (|x1| + |x0|)"""
    ref = T.ts_reference(name)
    if name in T.TS_I0:
        assert ref['i0'].tolist() == T.TS_I0[name]
        i0, _ = ops().grid_time_index(dv(T.ts_inputs(name)[1]), T.TS_CASES[name][2])
        assert i0.cpu().tolist() == T.TS_I0[name]
    check(record_property, name, ts_run(name), ref, ('y', 'gx', 'gcdf'))


@pytest.mark.parametrize('name', ['A', 'B'])
def test_time_sample_gradient_subsets(name, record_property):
    """only x, then only cdf, requiring a gradient (gcdf / gx null in cfn_time_sample_bwd): the same bounds, and bit-equal to the run that
    asks for both (the kernels use no fp32 atomics)"""
    ref, both = T.ts_reference(name), ts_run(name)
    only_x, only_c = ts_run(name, need_cdf=False), ts_run(name, need_x=False)
    assert set(only_x) == {'y', 'gx'} and set(only_c) == {'y', 'gcdf'}
    check(record_property, name + '-x', only_x, ref, ('y', 'gx'))
    check(record_property, name + '-cdf', only_c, ref, ('y', 'gcdf'))
    assert torch.equal(only_x['gx'], both['gx']) and torch.equal(only_c['gcdf'], both['gcdf'])


@pytest.mark.parametrize('name', ['H', 'F', 'K1'])
def test_time_sample_bwd_writes_every_element(name, record_property):
    """cfn_time_sample_bwd through the C ABI with gx prefilled with NaN (ops hands it torch.empty_like): frames without a tap come back as
    exact zeros, nothing is left unwritten; then gx alone and gcdf alone"""
    import cfn_hip
    B, C, Tin, K, sp = T.TS_CASES[name]
    x, cdf, g = (dv(v) for v in T.ts_inputs(name))
    ref = T.ts_reference(name)
    P = sp[0]
    for want_x, want_c in ((True, True), (True, False), (False, True)):
        gx = torch.full(x.shape, NAN, dtype=torch.float32, device=DEV) if want_x else None
        g64 = torch.zeros(B, K, dtype=torch.float64, device=DEV) if want_c else None
        cfn_hip.call('cfn_time_sample_bwd', g, x, cdf, gx, g64, B, C, Tin, K, P)
        torch.cuda.synchronize()
        got = {}
        if want_x:
            got['gx'] = gx
        if want_c:
            got['gcdf'] = g64.float()
        check(record_property, '%s-abi-%d%d' % (name, want_x, want_c), got, ref, tuple(got))


# ---- interp1d -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', T.I1_KNOTS)
@pytest.mark.parametrize('Pq', T.I1_PQ)
@pytest.mark.parametrize('N', T.I1_N)
def test_interp1d_fp64(N, Pq, kind, record_property):
    """B = 4 rows in all seven combinations of full and broadcast x / y / q, and B = 1; sorted random knots and knots with runs of equal
    values (at both ends too); queries inside the range, exactly on knots, beyond both ends.  4 x 300 queries make several workgroups;
    N = 65 with Pq = 1 lets the knot side decide the launch size.  Forward: ind and ynew bit-equal to oracle.x3d_ref.interp1d on
    row-expanded fp32 inputs.  Backward: gx, gy, gq within the bound with n = the queries contributing to the element (a broadcast row sums
    over the B rows); once with all three gradients requested, once with x alone (GridUnpool's own case)"""
    from oracle import x3d_ref as R
    worst = {}
    for rows in T.I1_ROWS:
        x, y, q, g = T.i1_inputs(N, Pq, kind, rows)
        ref = T.i1_reference(N, Pq, kind, rows)
        B = g.shape[0]
        yo, io = R.interp1d(*[v.expand(B, v.shape[1]).contiguous() for v in (x, y, q)])
        xg, yg, qg = dv(x, True), dv(y, True), dv(q, True)
        ynew, ind = ops().interp1d(xg, yg, qg)
        assert torch.equal(ind.cpu(), io) and torch.equal(io, ref['ind']), (rows, 'ind')
        assert torch.equal(ynew.detach().cpu(), yo), (rows, 'ynew', float((ynew.detach().cpu() - yo).abs().max()))
        got = dict(zip(('gx', 'gy', 'gq'), torch.autograd.grad(ynew, [xg, yg, qg], dv(g))))
        for k, v in zip(('gx', 'gy', 'gq'), (x, y, q)):
            assert tuple(got[k].shape) == tuple(v.shape), (rows, k)
        w = check(None, (N, Pq, kind, rows), got, ref, ('gx', 'gy', 'gq'))
        xg = dv(x, True)
        ynew, _ = ops().interp1d(xg, dv(y), dv(q))
        (gx,) = torch.autograd.grad(ynew, [xg], dv(g))
        check(None, (N, Pq, kind, rows, 'x only'), {'gx': gx}, ref, ('gx',))
        assert torch.equal(gx, got['gx']), (rows, 'gx alone differs from gx with gy and gq')
        worst = {k: max(worst.get(k, 0.0), w[k]) for k in w}
    record_property('temporal_fp64', repr(dict(case=('interp1d', N, Pq, kind), worst=worst)))


# ---- time_resize --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ac', [True, False], ids=['align', 'halfpixel'])
@pytest.mark.parametrize('shape,L', T.TR_CASES)
def test_time_resize_fp64(shape, L, ac, record_property):
    """both conventions at Kin = 1, Lout = 1, strong down- and upsampling, a 5-D input: forward n = 2; backward n = the outputs touching the
    input frame, and input frames no output touches get exact zeros (64 -> 3 leaves most of them untouched)"""
    x, g = T.tr_inputs(shape, L)
    ref = T.tr_reference(shape, L, ac)
    xg = dv(x, True)
    y = ops().time_resize(xg, L, ac)
    (gx,) = torch.autograd.grad(y, [xg], dv(g))
    if shape[2] == 64:
        assert float((ref['gx'].n == 0).double().mean()) > 0.5
    check(record_property, ('time_resize', shape, L, ac), {'y': y.detach(), 'gx': gx}, ref, ('y', 'gx'))


# ---- time_pool ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['avg', 'max'])
@pytest.mark.parametrize('case', T.TP_CASES)
def test_time_pool_fp64(case, mode, record_property):
    """post-ReLU-like inputs (multiples of 0.5, mostly exact zeros): at least a quarter of the max windows hold a tie (where R > 1: a window
    of one frame cannot).  max: forward and
    backward bit-equal to the reference (the gradient goes to the FIRST maximal frame, frames beyond R (T // R) get zero); avg: forward
    n = R + 1, backward one rounding of g / R"""
    x, g = T.tp_inputs(case)
    R_ = case[5]
    ref = T.tp_reference(case, mode)
    if R_ > 1:
        assert float(ref['ties'].double().mean()) >= 0.25
    xg = dv(x, True)
    y = ops().time_pool(xg, mode, R_)
    (gx,) = torch.autograd.grad(y, [xg], dv(g))
    got = {'y': y.detach(), 'gx': gx}
    if mode == 'max':
        assert torch.equal(got['y'].cpu(), ref['y'].val.float()) and torch.equal(got['gx'].cpu(), ref['gx'].val.float())
    check(record_property, ('time_pool', case, mode), got, ref, ('y', 'gx'))


# ---- grid_cdf -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('B,Kin', T.GC_CASES)
def test_grid_cdf_fp64(B, Kin, with_bias, record_property):
    """65 rows (a second 64-thread workgroup with one row), 130 x 33, Kin = 1; with a bias tensor and with bias=None.  cdf, gg and gb each
    within 4 x the fp32 CPU expression's own error + 2^-23 of the fp64 reference, relative to the tensor's max; first knot exactly 0,
    knots non-decreasing.  Kernel error and CPU error go to the junit report.  (gb is gg.sum(), torch's reduction of the kernel's gg: at
    130 x 33 a sum of condition sum|gg| / |gb| = 324, 1.8e-6 here against 9.9e-6 for the CPU expression.)

    Saturated-but-nonzero saliency rows are left out on purpose: 1 - sigmoid cancels to multiples of 2^-24 there, in the reference's
    fp32 yardstick as well, so an fp64 reference would measure the conditioning of the formula and not the kernel.  Kin = 1 is that
    case for the gradient: p = q / (q + 1e-16) is 1 up to 1e-16, its gradient is cancellation noise on every side, and what is asserted
    beside the rule is that it stays noise (<= 1e-13 max|gc|).  (Measured there, relative to the reference's max of ~1e-16: the kernel's
    gg 0.51 with a bias and 0.94 without, the fp32 CPU expression's 1e8 and 1.0 -- its gradient is fp32 noise or exactly zero -- so
    the rule itself says nothing at Kin = 1.)"""
    g, bias, gc = T.gc_inputs(B, Kin, with_bias)
    ref, base = T.gc_reference(B, Kin, with_bias), T.gc_baseline(B, Kin, with_bias)
    gg, bg = dv(g, True), (None if bias is None else dv(bias, True))
    out = ops().grid_cdf(gg, bg)
    grads = torch.autograd.grad(out, [gg] if bg is None else [gg, bg], dv(gc))
    got = {'cdf': out.detach(), 'gg': grads[0], 'gb': grads[1] if with_bias else None}
    errs = {}
    for k in ('cdf', 'gg') + (('gb',) if with_bias else ()):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == tuple(ref[k].shape) and bool(torch.isfinite(got[k]).all()), k
        errs[k] = (T.maxrel(got[k], ref[k]), T.maxrel(base[k], ref[k]))
    record_property('temporal_fp64', repr(dict(case=('grid_cdf', B, Kin, with_bias), kernel_vs_cpu=errs)))
    assert float(out[:, 0].abs().max()) == 0.0 and bool((out[:, 1:] >= out[:, :-1]).all())
    if Kin == 1:
        assert float(got['gg'].abs().max()) <= 1e-13 * float(gc.abs().max())
    for k, (e, b) in errs.items():
        assert e <= 4.0 * b + U23, (k, e, b)


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('B,Kin', [(65, 4), (3, 1)])
def test_grid_cdf_saturated(B, Kin, with_bias):
    """every logit +200: q = 0, all knots 0 and all gradients 0, all finite.  Every logit -200: q = 1 exactly, here and in the fp32 CPU
    expression, so the CDF is bit-equal to it, and the gradient is exactly 0 (sigmoid' = 0)"""
    from oracle import x3d_ref as R
    _, bias, gc = T.gc_inputs(B, Kin, with_bias)
    for level in (200.0, -200.0):
        g = torch.full((B, Kin), level)
        gg, bg = dv(g, True), (None if bias is None else dv(bias, True))
        out = ops().grid_cdf(gg, bg)
        grads = torch.autograd.grad(out, [gg] if bg is None else [gg, bg], dv(gc))
        assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(v).all()) for v in grads)
        assert all(bool((v == 0).all()) for v in grads), level
        if level > 0:
            assert bool((out == 0).all())
        else:
            assert torch.equal(out.detach().cpu(), R.grid_cdf(g if bias is None else g + bias))
