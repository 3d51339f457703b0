"""tests/dense_ref64.py pinned without a GPU: the reference equals fp64 autograd of F.conv3d to 1e-12, plain fp32 torch lies inside every
bound, every planted error (MUTANTS) lies outside the bound of the output meant to catch it, and no committed case holds a ReLU decision
that fp32 could take the other way."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref64 as R      # noqa: E402
from dense_ref64 import RELU, NONE, SAL, STEM      # noqa: E402

# (name, geom, N, Cin, Cout, T, H, W, prologue)
SMALL = [('sal28', SAL, 2, 24, 24, 5, 8, 28, True), ('sal28_plain', SAL, 1, 24, 20, 4, 6, 28, False), ('g1_odd', STEM, 2, 3, 5, 2, 9, 7, True),
         ('g3_ci9', SAL, 1, 9, 7, 3, 9, 9, False), ('g1_T1', STEM, 1, 25, 33, 1, 8, 6, True)]
_cache = {}


def small(name):
    """inputs, reference and fp64 autograd of F.conv3d of one small case, computed once"""
    if name in _cache:
        return _cache[name]
    _, g, N, Ci, Co, T, H, W, pro = next(c for c in SMALL if c[0] == name)
    i = R.make_inputs(11, N, Ci, Co, T, H, W, g, pro)
    act = RELU if pro else NONE
    fw = R.forward(i['x'], i['A'], i['B'], act, i['w'], g)
    bw = R.backward(i['gy'], fw['y'].float(), i['gs'], i['gq'], i['w'], i['x'], i['A'], i['B'], act, g)
    _cache[name] = (g, (N, Ci, Co, T, H, W), act, i, fw, bw)
    return _cache[name]


def autograd(i, g, act, dtype):
    """y, s, q and the gradients of <gy, y> + <gs, s> + <gq, q> by F.conv3d in `dtype`; the backward's y is the fp32 tensor the reference got"""
    x, w = i['x'].to(dtype).requires_grad_(True), i['w'].to(dtype).view(i['w'].shape[0], x_c(i), g[0], g[1], g[2]).requires_grad_(True)
    A = i['A'].to(dtype).requires_grad_(True) if i['A'] is not None else None
    B = i['B'].to(dtype).requires_grad_(True) if i['B'] is not None else None
    a = x
    if A is not None:
        a = A.view(A.shape[0], -1, 1, 1, 1) * x + B.view(B.shape[0], -1, 1, 1, 1)
        if act == RELU:
            a = a.clamp(min=0)
    y = F.conv3d(a, w, stride=g[3:6], padding=g[6:9])
    s, q = y.sum((2, 3, 4)), (y * y).sum((2, 3, 4))
    # G' = gy + gs + 2 gq y with the forward's y held fixed: the gradient of <gy, y> + <gs, s> + <gq, q>
    loss = (y * i['gy'].to(dtype)).sum() + (s * i['gs'].to(dtype)).sum() + (q * i['gq'].to(dtype)).sum()
    ins = [x, w] + ([A, B] if A is not None else [])
    gr = torch.autograd.grad(loss, ins)
    return y.detach(), s.detach(), q.detach(), [t.detach() for t in gr]


def x_c(i):
    return i['x'].shape[1]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-300))


@pytest.mark.parametrize('name', [c[0] for c in SMALL])
def test_reference_equals_fp64_autograd(name):
    g, sh, act, i, fw, _ = small(name)
    y, s, q, gr = autograd(i, g, act, torch.float64)
    # the backward reference at the fp64 y, so that both sides differentiate the same function
    bw = R.backward(i['gy'], y, i['gs'], i['gq'], i['w'], i['x'], i['A'], i['B'], act, g)
    assert rel(fw['y'], y) < 1e-12 and rel(fw['s'], s) < 1e-12 and rel(fw['q'], q) < 1e-12
    assert rel(bw['gx'], gr[0]) < 1e-12 and rel(bw['gw'], gr[1].reshape(gr[1].shape[0], -1)) < 1e-12
    if i['A'] is not None:
        assert rel(bw['gA'], gr[2]) < 1e-12 and rel(bw['gB'], gr[3]) < 1e-12


@pytest.mark.parametrize('name', [c[0] for c in SMALL])
def test_fp32_torch_is_inside_every_bound(name):
    g, (N, Ci, Co, T, H, W), act, i, fw, _ = small(name)
    K, Q = Ci * g[0] * g[1] * g[2], int(torch.tensor(R.out_shape(T, H, W, g)).prod())
    y, s, q, gr = autograd(i, g, act, torch.float32)
    fb = R.forward_bounds(fw, K + 4, Q)
    assert R.worst(y, fw['y'], fb['y']) <= 1 and R.worst(s, fw['s'], fb['s']) <= 1 and R.worst(q, fw['q'], fb['q']) <= 1
    # backward: autograd's G' is built from ITS y; give the reference the same fp32 y
    bw = R.backward(i['gy'], y, i['gs'], i['gq'], i['w'], i['x'], i['A'], i['B'], act, g)
    bb = R.backward_bounds(bw, i['x'], i['A'], Co * g[0] * g[1] * g[2] + 4, N * Q, n_acc=T * H * W)
    assert R.worst(gr[0], bw['gx'], bb['gx']) <= 1
    assert R.worst(gr[1].reshape(Co, -1), bw['gw'], bb['gw']) <= 1
    if i['A'] is not None:
        assert R.worst(gr[2], bw['gA'], bb['gA']) <= 1 and R.worst(gr[3], bw['gB'], bb['gB']) <= 1


# The case meant to catch each mutant: a saliency shape, 28 wide, with the plan cfn_conv3d_dense_route gives for it, so that the seam mutants sit
# on the kernels' real chunk and band seams.  At 256 CUs: To = 3 in chunks of 2 (last 1) in both kernels, Ho = 4 in bands of 2 rows (forward) /
# one band of 4 rows (weight gradient).  A second trip of the persistent loop needs fewer workgroups than items: planned for 1 CU the weight
# gradient has 2 items (one per sample) on a grid of 1.
def plan_of(op, dims, flags, cus):
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'coarse-fine-networks_amd')) if p not in sys.path]
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    from cfn_hip import ops
    line = ops.conv3d_dense_route(op, *dims, SAL, flags, cus)
    f = R.fields(line)
    Ho = dims[4] // 2
    return line, dict(f, rb=-(-Ho // f['bands']))


@pytest.mark.parametrize('mutant', sorted(R.MUTANTS))
def test_every_mutant_leaves_its_bound(mutant):
    which, out = R.MUTANTS[mutant]
    dims = N, Ci, Co, T, H, W = 2, 24, 24, 5, 8, 28
    i = R.make_inputs(5, N, Ci, Co, T, H, W, SAL, True, exact_zero=True)
    fw = R.forward(i['x'], i['A'], i['B'], RELU, i['w'], SAL)
    if which == 'fwd':
        line, plan = plan_of(R.FWD, dims, R.PRO | R.STATS, 256)
        assert plan['nchunks'] > 1 and plan['bands'] > 1 and plan['rb'] == 2, line
    else:
        line, plan = plan_of(R.WGRAD, dims, R.PRO | R.STATS | R.Y, 1 if mutant == 'skip_second_item' else 256)
        assert (plan['items'] > plan['grid']) if mutant == 'skip_second_item' else (plan['last'] < plan['chunk'] and plan['rb'] == 4), line
    if which == 'fwd':
        # the tightest bound a forward kernel gets is the fp32 kernels'; five_terms is salconvb's and meets its wider bound
        b = R.forward_bounds(fw, 6 * 168 + 4 if mutant == 'five_terms' else 648 + 4, plan['chunk'] + 6, split=mutant == 'five_terms')
        m = R.forward(i['x'], i['A'], i['B'], RELU, i['w'], SAL, mutant=mutant, plan=plan)
        assert R.worst(m[out], fw[out], b[out]) > 1
        return
    y = fw['y'].float()
    bw = R.backward(i['gy'], y, i['gs'], i['gq'], i['w'], i['x'], i['A'], i['B'], RELU, SAL)
    b = R.backward_bounds(bw, i['x'], i['A'], 648 + 4, R.roundings(R.WGRAD, line, N, Ci, Co, T, H, W, SAL)['n_w'])
    m = R.backward(i['gy'], y, i['gs'], i['gq'], i['w'], i['x'], i['A'], i['B'], RELU, SAL, mutant=mutant, plan=plan)
    assert R.worst(m[out], bw[out], b[out]) > 1
    if mutant == 'relu_ge':      # ... and it is caught where the pre-activation is exactly 0, nowhere else
        z = R.prologue(i['x'], i['A'], i['B'], RELU)[1]
        assert bool(((m['gx'] != bw['gx']) <= (z == 0)).all()) and int((z == 0).sum()) > 0


def _all_cases():
    for name, g, N, Ci, Co, T, H, W, flags, _ in R.SAL_CASES + R.LONG_CASES + R.GENERIC_CASES:
        if flags & R.PRO:
            yield pytest.param(name, g, N, Ci, Co, T, H, W, id=name)


@pytest.mark.parametrize('name,g,N,Ci,Co,T,H,W', list(_all_cases()))
def test_no_case_holds_an_ambiguous_relu(name, g, N, Ci, Co, T, H, W):
    i = R.make_inputs(R.seed_of(name), N, Ci, Co, T, H, W, g, True, exact_zero=name.endswith('_z0'))
    assert int(R.ambiguous(i['x'], i['A'], i['B']).sum()) == 0
    if name.endswith('_z0'):      # ... while exact zeros, which both arithmetics decide alike, are there on purpose
        assert int((R.prologue(i['x'], i['A'], i['B'], RELU)[1] == 0).sum()) > 0
