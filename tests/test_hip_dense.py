"""The dense conv kernels -- salconvb.hip, salconv.hip, the data-gradient kernels of fusion.hip, the implicit GEMM and the weight gradients of
pwconv.hip / pwwgrad.hip, stem.hip -- through the C ABI against the fp64 reference of tests/dense_ref64.py (pinned to fp64 autograd, and its
bounds shown to discriminate, by tests/test_dense_ref64_cpu.py).  The cases, and the kernel, template arguments and branch each one reaches,
are listed in dense_ref64.py; every case first asks cfn_conv3d_dense_route with the device's CU count and ASSERTS that kernel and branch
(tests/test_dense_route_cpu.py asserts the same at 256 CUs without a GPU).

Every output is prefilled with NaN (gw, gA, gB, s, q with zeros: the ABI accumulates into them) and sits inside a larger allocation whose
sentinel guards on both sides are checked afterwards: the sal kernels use out-of-range buffer offsets as their bounds check.  A MISALIGNED
case starts every activation tensor one element past a 16-byte boundary; the MIS_X, MIS_G and MIS_OUT cases move one tensor alone (x; gy and
y; the output y / gx), for the saliency, the generic and the stem shapes, and assert the kernel each gate clause leads to.  The backward gets the reference's y rounded to fp32, so a forward
error cannot hide in it.  Bounds: dense_ref64's docstring; the worst err / bound of every case and output goes to the junit report
(dense_fp64).

Reached: sal_fwdb_kernel<56 | 28, false | true>, sal_fwd_kernel<56 | 28, 1, false | true> (cfn_pw_split_terms = 0 on the same inputs),
sal_dgrad_kernel and sal_wgrad_kernel <56, false, true>, <56, true, false>, <28, true, true>, <28, false, false>, sal_dgrad_kernel<56, true, true>
(the other instantiations differ from these in one template argument at a time and share every line of code with them);
conv3d_dense_bwd_data_allci_kernel<8 | 24 | 32> (the 24 one also between 48 and 64 KiB of weights), conv3d_dense_bwd_data_kernel;
pw_gemm_kernel<1 | 2, 0, stats, none | relu, true>; pw_wgrad_direct_kernel<., 2, 1, 1> and <., 2, 3, 3>; pw_wgrad_kernel<1 | 2, 1 | 2>;
stem_fwd_kernel<3> with bands of 8 and of 4 rows; stem_wgrad_kernel.  Chunks: forward TO = 2, 3 (full and short last chunk) and 8 (the
benchmark's plan, at N = 8: 29 frames); data gradient CH = 2 and 4 (even and odd group count); weight gradient CH = 2 and 4, the persistent
loop with one trip, and with two trips in some workgroups only.
Not reached: the data gradient's CH = 16 of the benchmark (8 x 56 x 56 needs more than 100 MB of input for it at 256 CUs: test_dense_route_cpu
shows that no T up to 41 gives it); the weight gradient's CH = 8; sal_fwd_kernel's NT = 2 and 4 (not instantiated by the launcher);
pw_gemm_kernel<3 | 4, ...> (a dense conv's weight image allows two row tiles at most).  There is no hook to force them.

Finding: sal_dgrad_kernel moves g', y, x and gx eight bytes at a time and its launcher checked no alignment (sal_fwd, sal_wgrad and the stem
kernels decline a misaligned x; sal_wgrad checked x but not gy / y, which it also reads in 8-byte units).  Both plans now decline tensors
that do not start on an 8-byte boundary; w28_mis_x, w28_mis_x_plain, w28_mis_g and w28_mis_out move one tensor at a time and assert what each
clause of the gates leads to (the generic kernels; the sal kernel where the tensor is not read, or is stored one element at a time).  The
gates are a precaution: the ungated kernels were never run on such a tensor, so that they would misbehave is supposed, not shown.

Largest err / bound seen on an MI355X, per kernel family and output (1.0 is the bound; n is the worst summation order, so a correct kernel
stays far below it):
    sal_fwdb (split bf16)   y 0.0026, s 1.2e-4, q 1.2e-4          sal_fwd (fp32)   y 0.0039, s 2.0e-4, q 1.9e-4
    sal_dgrad               gx 0.0099, gA 1.4e-4, gB 1.1e-4       sal_wgrad        gw 0.033
    pw_gemm (STEM = true)   y 0.095, s 0.022, q 0.031             all-channel / per-channel data gradient   gx 0.030, gA 8.6e-4, gB 1.1e-3
    pw_wgrad_direct / pw_wgrad (dense)   gw 0.21                  stem_fwd   y 0.16          stem_wgrad   gw 2.2e-4

The checks were also run once against a scratch build of salconvb.hip, salconv.hip and fusion.hip with planted errors in the kernels
themselves, one switched on at a time (the same build with none switched on passes all cases).  Every one was caught; factor over the bound:
temporal tap 0 lost at the first frame of a chunk, in sal_fwdb 3.1e3 .. 4.4e3 and in sal_fwd 4.9e3 .. 6.8e3 (w56_T5, fwd_TO3_full, fwd_TO3_short,
fwd_bench_TO8: the cases with a chunk seam); the halo row above a band lost in sal_fwd 4.3e3 .. 8.3e3; G' without 2 gq y in sal_dgrad 1.0e2
.. 2.1e2 (w28_pro_T4, dg_CH4, dg_odd); G' without gs in sal_dgrad 3.2e2 .. 4.9e2, in the all-channel kernel 3.2e2 (w28_misaligned; every
generic case fails as well); gA without its x factor 43 .. 5.4e2; the persistent loop of sal_wgrad stopping after its first item 1.4e3
(wg_persistent alone: the one case with a second trip); its last, shorter chunk skipped 4.9e2 .. 1.4e5 (wg_CH4, wg_persistent, the T = 1 and
T = 2 cases); kh and kw exchanged in gw 3.1e3 .. 1.7e5 and inf; relu(B) left in the padding rows of sal_wgrad 9.3e2 .. 2.1e4 and inf; ReLU'
taken at z >= 0 in sal_dgrad inf, by
w28_pro_z0 alone (no other case holds an exact zero; before that case existed this error passed).  Not built into a kernel: tap 2 from the
wrong frame, five of the six split terms, and the errors of the generic forward and weight-gradient kernels; the reference-side mutants of
tests/test_dense_ref64_cpu.py stand for them.
"""
import pytest
import torch

import dense_ref64 as R
from dense_ref64 import DGRAD, FWD, MIS_G, MIS_OUT, MIS_X, MISALIGNED, NONE, PRO, RELU, STATS, STEM, STEM_FWD, STEM_WGRAD, WGRAD, Y

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
SENT = -7777.0
GUARD = 64


def lib():
    import cfn_hip
    from cfn_hip import ops  # noqa: F401
    return cfn_hip


class Guarded(object):
    """n elements inside a larger allocation: GUARD + off sentinel elements before, GUARD after; off = 1: one element past a 16-byte boundary"""

    def __init__(self, n, dtype=torch.float32, fill=NAN, src=None, off=0):
        self.buf = torch.full((2 * GUARD + off + n,), SENT, dtype=dtype, device=DEV)
        self.lo, self.n = GUARD + off, n
        self.t = self.buf[self.lo:self.lo + n]
        if src is not None:
            self.t.copy_(src.reshape(-1).to(dtype))
        else:
            self.t.fill_(fill)
        assert self.t.is_contiguous() and (self.t.data_ptr() % 16 == 0) == (off == 0)

    def intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.lo + self.n:] == SENT).all())


def put(v, off=0):
    return None if v is None else Guarded(v.numel(), v.dtype, src=v, off=off).t.view(v.shape)


def offs(flags):
    """elements past a 16-byte boundary at which x, gy and y, and the output (y / gx) start: MISALIGNED moves all, MIS_X / MIS_G / MIS_OUT one"""
    return (int(bool(flags & (MISALIGNED | MIS_X))), int(bool(flags & (MISALIGNED | MIS_G))), int(bool(flags & (MISALIGNED | MIS_OUT))))


def route(op, N, Ci, Co, T, H, W, g, flags):
    return lib().ops.conv3d_dense_route(op, N, Ci, Co, T, H, W, g, flags, 0)


def claim(claims, op, line):
    """assert -- not skip -- that the kernel and branch the case is about is what runs on this device"""
    if op in claims:
        kernel, pred = claims[op]
        f = R.fields(line)
        assert f['kernel'] == kernel and (pred is None or pred(f)), line


def report(record, tag, worst):
    record('dense_fp64', repr(dict(case=tag, worst=worst)))
    print(tag, {k: '%.3g' % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1.0, (tag, k, v)


def run_forward(tag, claims, op, i, dev, act, g, dims, flags, off, ref, worst, sfx=''):
    N, Ci, Co, T, H, W = dims
    line = route(op, N, Ci, Co, T, H, W, g, flags & ~Y)
    claim(claims, op, line)
    osz = R.out_shape(T, H, W, g)
    y = Guarded(N * Co * osz[0] * osz[1] * osz[2], off=off)
    s = q = None
    if op == STEM_FWD:
        lib().call('cfn_stem_conv_fwd', dev['x'], dev['w'], y.t, N, Ci, Co, T, H, W)
    else:
        if flags & STATS:
            s, q = Guarded(N * Co, torch.float64, 0.0), Guarded(N * Co, torch.float64, 0.0)
        lib().call('cfn_conv3d_dense_fwd', dev['x'], dev['A'], dev['B'], act, dev['w'], y.t, s and s.t, q and q.t, N, Ci, Co, T, H, W,
                   lib().ops._geom(g[0:3], g[3:6], g[6:9]))
    torch.cuda.synchronize()
    for k, gd in (('y', y), ('s', s), ('q', q)):
        assert gd is None or gd.intact(), (tag, k, 'a guard element next to the output was overwritten')
    n = R.roundings(op, line, N, Ci, Co, T, H, W, g)
    b = R.forward_bounds(ref, n['n_y'], n['n_s'], n['split'])
    worst['y' + sfx] = R.worst(y.t.view(ref['y'].shape), ref['y'], b['y'])
    if s is not None:
        worst['s' + sfx] = R.worst(s.t.view(N, Co), ref['s'], b['s'])
        worst['q' + sfx] = R.worst(q.t.view(N, Co), ref['q'], b['q'])


def run_case(record, name, g, N, Ci, Co, T, H, W, flags, claims, which):
    cfn = lib()
    ox, og, oo = offs(flags)
    pro = bool(flags & PRO)
    act = RELU if pro else NONE
    i = R.make_inputs(R.seed_of(name), N, Ci, Co, T, H, W, g, pro, exact_zero=name.endswith('_z0'))
    dev = {k: put(i[k], {'x': ox, 'gy': og}.get(k, 0)) for k in ('x', 'w', 'A', 'B', 'gy', 'gs', 'gq')}
    if pro:
        assert int(R.ambiguous(dev['x'], dev['A'], dev['B']).sum()) == 0      # the share of skipped elements is 0: nothing is skipped
    dims = (N, Ci, Co, T, H, W)
    worst = {}
    ref = R.forward(dev['x'], dev['A'], dev['B'], act, dev['w'], g)
    if FWD in which:
        run_forward(name, claims, FWD, i, dev, act, g, dims, flags, oo, ref, worst)
        if FWD in claims and claims[FWD][0].startswith('sal_fwdb'):      # the exact-fp32 kernel on the same inputs
            prev = cfn.query('cfn_pw_split_terms', 0)
            try:
                kernel = 'sal_fwd_kernel<%d, 1, %s>' % (W, 'true' if pro else 'false')
                pred = claims[FWD][1] if FWD in claims else None
                run_forward(name, {FWD: (kernel, pred)}, FWD, i, dev, act, g, dims, flags, oo, ref, worst, '_fp32')
            finally:
                cfn.query('cfn_pw_split_terms', prev)
    if DGRAD in which or WGRAD in which:
        gs = dev['gs'] if flags & STATS else None
        gq = dev['gq'] if flags & Y else None
        yin = put(ref['y'].float(), og) if flags & Y else None
        want = tuple(k for k, op in (('gx', DGRAD), ('gw', WGRAD)) if op in which)
        bw = R.backward(dev['gy'], yin, gs, gq, dev['w'], dev['x'], dev['A'], dev['B'], act, g, want=want)
        geom = cfn.ops._geom(g[0:3], g[3:6], g[6:9])
        n = {}
        if DGRAD in which:
            line = route(DGRAD, N, Ci, Co, T, H, W, g, flags)
            claim(claims, DGRAD, line)
            n.update(R.roundings(DGRAD, line, N, Ci, Co, T, H, W, g))
            gx = Guarded(N * Ci * T * H * W, off=oo)
            gA = Guarded(N * Ci, torch.float64, 0.0) if pro else None
            gB = Guarded(N * Ci, torch.float64, 0.0) if pro else None
            cfn.call('cfn_conv3d_dense_bwd_data', dev['gy'], yin, gs, gq, dev['w'], dev['x'], dev['A'], dev['B'], act, gx.t,
                     gA and gA.t, gB and gB.t, N, Ci, Co, T, H, W, geom)
            torch.cuda.synchronize()
            for k, gd in (('gx', gx), ('gA', gA), ('gB', gB)):
                assert gd is None or gd.intact(), (name, k, 'a guard element next to the output was overwritten')
        if WGRAD in which:
            line = route(WGRAD, N, Ci, Co, T, H, W, g, flags)
            claim(claims, WGRAD, line)
            n.update(R.roundings(WGRAD, line, N, Ci, Co, T, H, W, g))
            gw = Guarded(Co * dev['w'].shape[1], torch.float64, 0.0)
            cfn.call('cfn_conv3d_dense_bwd_weight', dev['gy'], yin, gs, gq, dev['x'], dev['A'], dev['B'], act, gw.t, N, Ci, Co, T, H, W, geom)
            torch.cuda.synchronize()
            assert gw.intact(), (name, 'gw', 'a guard element next to the output was overwritten')
        b = R.backward_bounds(bw, dev['x'], dev['A'], n.get('n_d', 0), n.get('n_w', 0))
        if DGRAD in which:
            worst['gx'] = R.worst(gx.t.view(bw['gx'].shape), bw['gx'], b['gx'])
            if pro:
                worst['gA'] = R.worst(gA.t.view(N, Ci), bw['gA'], b['gA'])
                worst['gB'] = R.worst(gB.t.view(N, Ci), bw['gB'], b['gB'])
        if WGRAD in which:
            worst['gw'] = R.worst(gw.t.view(bw['gw'].shape), bw['gw'], b['gw'])
    report(record, name, worst)


@pytest.mark.parametrize('case', R.SAL_CASES, ids=[c[0] for c in R.SAL_CASES])
def test_saliency(record_property, case):
    name, g, N, Ci, Co, T, H, W, flags, claims = case
    run_case(record_property, name, g, N, Ci, Co, T, H, W, flags, claims, (FWD, DGRAD, WGRAD) if Co == 24 else (FWD,))


@pytest.mark.parametrize('case', R.LONG_CASES, ids=[c[0] for c in R.LONG_CASES])
def test_saliency_long_chunks(record_property, case):
    name, g, N, Ci, Co, T, H, W, flags, claims = case
    run_case(record_property, name, g, N, Ci, Co, T, H, W, flags, claims, tuple(claims))


@pytest.mark.parametrize('case', R.GENERIC_CASES, ids=[c[0] for c in R.GENERIC_CASES])
def test_generic(record_property, case):
    name, g, N, Ci, Co, T, H, W, flags, claims = case
    run_case(record_property, name, g, N, Ci, Co, T, H, W, flags, claims, (FWD, DGRAD, WGRAD))


@pytest.mark.parametrize('case', R.STEM_CASES, ids=[c[0] for c in R.STEM_CASES])
def test_stem(record_property, case):
    name, N, Co, T, H, W, mis, claims = case
    cfn = lib()
    ox, og, oo = offs(mis)
    i = R.make_inputs(R.seed_of('stem_' + name), N, 3, Co, T, H, W, STEM, False)
    dev = {'x': put(i['x'], ox), 'w': put(i['w']), 'gy': put(i['gy'], og), 'A': None, 'B': None}
    worst = {}
    ref = R.forward(dev['x'], None, None, NONE, dev['w'], STEM)
    run_forward(name, claims, STEM_FWD, i, dev, NONE, STEM, (N, 3, Co, T, H, W), mis, oo, ref, worst)
    line = route(STEM_WGRAD, N, 3, Co, T, H, W, None, mis)
    claim(claims, STEM_WGRAD, line)
    bw = R.backward(dev['gy'], None, None, None, dev['w'], dev['x'], None, None, NONE, STEM, want=('gw',))
    gw = Guarded(Co * 27, torch.float64, 0.0)
    cfn.call('cfn_stem_conv_bwd_weight', dev['gy'], dev['x'], gw.t, N, 3, Co, T, H, W)
    torch.cuda.synchronize()
    assert gw.intact(), (name, 'gw', 'a guard element next to the output was overwritten')
    n = R.roundings(STEM_WGRAD, line, N, 3, Co, T, H, W, STEM)
    worst['gw'] = R.worst(gw.t.view(Co, 27), bw['gw'], R.backward_bounds(bw, dev['x'], None, 0, n['n_w'])['gw'])
    report(record_property, 'stem_' + name, worst)
