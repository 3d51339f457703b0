"""tests/bnfold_ref64.py (the fp64 reference csrc/bnfold.hip is checked against) pinned to the module-level expression the kernel claims to
reproduce, in float64 on a real y of shape (N, C, T, H, W): F.batch_norm over y.view(N//S, C*S, T, H, W) with running buffers, the shared
affine, then the squeeze-excite branch (global average pool -> fc1 -> ReLU -> fc2 -> sigmoid -> scale).  Compared: A*y + B with (A, B) from
the reference fed s = sum y, q = sum y^2; the running buffers; and the gradients w.r.t. y (through s and q), gamma, beta and the four SE
tensors.  Both sides are fp64 and differ in summation order only: 1e-12 relative to each tensor's max.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from bnfold_ref64 import bnfold_ref64

TOL = 1e-12


def _rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _module(y, gamma, beta, run_mean, run_var, training, S, eps, momentum, se):
    """SubBatchNorm3d.forward + the SE branch of the bottleneck, on private copies of the buffers -> (out, run_mean', run_var', gate)"""
    N, C, T, H, W = y.shape
    rm, rv = run_mean.clone(), run_var.clone()
    if training:
        x = F.batch_norm(y.view(N // S, C * S, T, H, W), rm, rv, None, None, True, momentum, eps).view(N, C, T, H, W)
    else:
        x = F.batch_norm(y, rm, rv, None, None, False, momentum, eps)
    if gamma is not None:
        x = x * gamma.view(-1, 1, 1, 1)
        x = x + beta.view(-1, 1, 1, 1)
    g = None
    if se is not None:
        w1, b1, w2, b2 = se
        g = F.adaptive_avg_pool3d(x, 1)
        g = torch.sigmoid(F.conv3d(torch.relu(F.conv3d(g, w1, b1)), w2, b2))
        x = x * g
    return x, rm, rv, g


def _close(name, got, ref):
    assert got.dtype == torch.float64 and got.shape == ref.shape, name
    err, top = float((got - ref).detach().abs().max()), float(ref.detach().abs().max())
    assert err <= TOL * top, (name, err, top)


@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('S', [1, 2, 4])
def test_bnfold_ref64_matches_module_expression(S, gated, training, affine):
    N, C, Wd, T, H, W = 8, 6, 4, 3, 5, 4
    eps, momentum = 1e-3, 0.37
    count = T * H * W
    y = (_rnd(1, N, C, T, H, W) * (0.5 + _rnd(2, C).abs()).view(1, C, 1, 1, 1) + _rnd(3, C).view(1, C, 1, 1, 1)).requires_grad_(True)
    gamma = (1.0 + _rnd(4, C, scale=0.2)).requires_grad_(True) if affine else None
    beta = _rnd(5, C, scale=0.3).requires_grad_(True) if affine else None
    se = None
    if gated:
        se = tuple(v.requires_grad_(True) for v in (_rnd(6, Wd, C, 1, 1, 1, scale=(2.0 / C) ** 0.5), _rnd(7, Wd, scale=0.1),
                                                    _rnd(8, C, Wd, 1, 1, 1, scale=(2.0 / Wd) ** 0.5), _rnd(9, C, scale=0.1)))
    Se = S if training else 1
    run_mean, run_var = _rnd(10, Se * C), 0.5 + _rnd(11, Se * C).abs()
    nbt = torch.tensor(3)
    r = _rnd(12, N, C, T, H, W)
    leaves = [v for v in (y, gamma, beta) + (se or ()) if v is not None]
    names = ['y'] + (['gamma', 'beta'] if affine else []) + (['w1', 'b1', 'w2', 'b2'] if gated else [])

    want, want_rm, want_rv, want_gate = _module(y, gamma, beta, run_mean, run_var, training, S, eps, momentum, se)
    want_g = torch.autograd.grad((want * r).sum(), leaves)

    s, q = y.sum((2, 3, 4)), (y * y).sum((2, 3, 4))
    rm0, rv0 = run_mean.clone(), run_var.clone()
    out = bnfold_ref64(s, q, gamma, beta, (run_mean, run_var, nbt), training, N, C, S, count, eps, momentum, se=se, pool_count=count)
    assert torch.equal(run_mean, rm0) and torch.equal(run_var, rv0) and int(nbt) == 3          # the buffers are read, never written
    got = out.A.view(N, C, 1, 1, 1) * y + out.B.view(N, C, 1, 1, 1)
    got_g = torch.autograd.grad((got * r).sum(), leaves)

    _close('A*y + B', got, want)
    _close('running_mean', out.run_mean, want_rm)
    _close('running_var', out.run_var, want_rv)
    assert int(out.nbt) == (4 if training else 3)
    assert out.mean.shape == (Se, C) and out.rstd.shape == (Se, C)
    for name, g, w in zip(names, got_g, want_g):
        _close('grad ' + name, g, w)
    if not training:
        assert torch.equal(out.run_mean, run_mean) and torch.equal(out.run_var, run_var)
    if gated:       # the saved intermediates are those of the module: pooled is the global mean of bn(y), A / A0 the gate
        x0 = _module(y, gamma, beta, run_mean, run_var, training, S, eps, momentum, None)[0]
        _close('pooled', out.pooled, x0.mean((2, 3, 4)))
        _close('gate', out.gate, want_gate.view(N, C))
        _close('h', out.h, torch.relu(out.pre))
        assert out.pre.shape == (N, Wd)


def test_bnfold_ref64_variance_clamp_passes_the_gradient():
    """a slightly negative qq/cnt - mean^2 is clamped to 0 in the value, and the gradient is that of the unclamped expression"""
    N, C, count = 2, 3, 10.0
    mean = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
    s = (mean * count).repeat(N, 1).requires_grad_(True)
    q = (mean * mean * count * (1.0 - 1e-12)).repeat(N, 1).requires_grad_(True)
    bufs = (torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), torch.tensor(0))
    out = bnfold_ref64(s, q, None, None, bufs, True, N, C, 1, count, 1e-5, 0.1)
    assert torch.equal(out.rstd, torch.full((1, C), 1e-5, dtype=torch.float64) ** -0.5)
    assert float(out.run_var.min()) == 0.9
    gs, gq = torch.autograd.grad(out.A.sum(), (s, q))
    rstd3 = float(out.rstd.detach()[0, 0]) ** 3
    assert torch.allclose(gq, torch.full_like(gq, -0.5 * rstd3 / (count * N) * N), rtol=1e-12)
    assert torch.allclose(gs, (mean * rstd3 / (count * N) * N).repeat(N, 1), rtol=1e-12)


def test_bnfold_ref64_fp32_gate_and_dropped_terms():
    """gate_dtype=float32 changes the gate arithmetic only (statistics stay fp64), and every term `drop` names changes what it feeds"""
    from bnfold_ref64 import TERMS, bnfold_grads
    N, C, Wd, S, count = 4, 6, 4, 2, 12.0
    s = (_rnd(1, N, C) * 3.0).requires_grad_(True)
    q = (s.detach() ** 2 / count + count * (0.5 + _rnd(2, N, C).abs())).requires_grad_(True)
    gamma, beta = (1.0 + _rnd(4, C, scale=0.2)).requires_grad_(True), _rnd(5, C, scale=0.3).requires_grad_(True)
    se = tuple(v.requires_grad_(True) for v in (_rnd(6, Wd, C, scale=(2.0 / C) ** 0.5), _rnd(7, Wd, scale=0.1),
                                                _rnd(8, C, Wd, scale=(2.0 / Wd) ** 0.5), _rnd(9, C, scale=0.1)))
    bufs = (_rnd(10, S * C), 0.5 + _rnd(11, S * C).abs(), torch.tensor(0))
    gA, gB = _rnd(12, N, C), _rnd(13, N, C)
    leaves = dict(s=s, q=q, gamma=gamma, beta=beta, w1=se[0], b1=se[1], w2=se[2], b2=se[3])
    run = lambda **kw: bnfold_ref64(s, q, gamma, beta, bufs, True, N, C, S, count, 1e-5, 0.1, se=se, pool_count=2 * count, **kw)
    ref = run()
    g = bnfold_grads(ref, gA, gB, leaves)
    lo = run(gate_dtype=torch.float32)
    assert torch.equal(lo.mean, ref.mean) and torch.equal(lo.rstd, ref.rstd) and torch.equal(lo.run_var, ref.run_var)
    assert torch.equal(lo.A0, ref.A0.float().double()) and lo.A.dtype == torch.float64
    assert 0.0 < float((lo.A - ref.A).abs().max()) <= 1e-6 * float(ref.A.abs().max())
    feeds = {'direct': ('s',), 'gate_grad': ('s', 'q', 'gamma', 'beta'), 'mean_gvar': ('s',), 'unbiased': (), 'pool_count': tuple(leaves)}
    for term in TERMS:
        d = run(drop=term)
        gd = bnfold_grads(d, gA, gB, leaves)
        assert torch.equal(d.run_var, ref.run_var) == (term != 'unbiased'), term
        assert torch.equal(d.A, ref.A) == (term != 'pool_count'), term
        for k in leaves:
            assert torch.equal(gd[k], g[k]) == (k not in feeds[term]), (term, k)
