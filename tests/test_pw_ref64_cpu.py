"""tests/pw_ref64.py (the fp64 reference the one-pass pointwise backward kernels are checked against) pinned to fp64 autograd: the forward
y = conv1x1(act(A x + B), W) and the scalar

    L = sum gsc*gy*y + sum_{n,c} gs * sum_q y + sum_{n,c} gq * sum_q y^2 + sum acc * a[..., ::s, ::s]

whose gradients w.r.t. (x, W, A, B) are exactly (gx, gw, gA, gB) of the helper.  CPU only."""

import pytest
import torch

from pw_ref64 import pw_ref64


def _rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _act(z, act):
    if act == 1:
        return torch.relu(z)
    if act == 2:
        return z * torch.sigmoid(z)
    return z


@pytest.mark.parametrize('terms', ['all', 'none', 'gs', 'gsc'])
@pytest.mark.parametrize('acc_s', [None, 2, 3])
@pytest.mark.parametrize('act', [None, 0, 1, 2])
def test_pw_ref64_matches_autograd(act, acc_s, terms):
    N, Cin, Cout, T, H, W = 2, 5, 7, 3, 7, 8
    x = _rnd(1, N, Cin, T, H, W).requires_grad_(True)
    w = _rnd(2, Cout, Cin, scale=0.3).requires_grad_(True)
    A = B = None
    if act is not None:
        A = (1.0 + _rnd(3, N, Cin, scale=0.2)).requires_grad_(True)
        B = _rnd(4, N, Cin, scale=0.2).requires_grad_(True)
    gy = _rnd(5, N, Cout, T, H, W)
    gs = _rnd(6, N, Cout, scale=0.05) if terms in ('all', 'gs') else None
    gq = _rnd(7, N, Cout, scale=0.01) if terms == 'all' else None
    gsc = 1.0 + _rnd(8, N, Cout, scale=0.3) if terms in ('all', 'gsc') else None
    acc = _rnd(9, N, Cin, T, (H - 1) // acc_s + 1, (W - 1) // acc_s + 1) if acc_s else None

    sp = lambda v: v.view(N, -1, 1, 1, 1)
    a = x if A is None else _act(x * sp(A) + sp(B), act)
    y = torch.einsum('nmthw,km->nkthw', a, w)
    L = ((gy * sp(gsc)) if gsc is not None else gy).mul(y).sum()
    if gs is not None:
        L = L + (gs * y.sum((2, 3, 4))).sum()
    if gq is not None:
        L = L + (gq * (y * y).sum((2, 3, 4))).sum()
    if acc is not None:
        L = L + (acc * a[:, :, :, ::acc_s, ::acc_s]).sum()
    leaves = [v for v in (x, w, A, B) if v is not None]
    grads = torch.autograd.grad(L, leaves)

    gx, gA, gB, gw = pw_ref64(gy, y.detach(), gs, gq, gsc, w.detach(), x.detach(), None if A is None else A.detach(),
                              None if B is None else B.detach(), act or 0, acc, acc_s or 1)
    got = [gx, gw] + ([gA, gB] if A is not None else [])
    assert (gA is None) == (A is None) and (gB is None) == (A is None)
    for name, g, r in zip(('gx', 'gw', 'gA', 'gB'), got, grads):
        assert g.dtype == torch.float64 and g.shape == r.shape, name
        assert float((g - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), (name, float((g - r).abs().max()))
    if acc is None:
        return
    # one sample at a time (the full-size GPU cases' mode): the same numbers
    one = pw_ref64(gy, y.detach(), gs, gq, gsc, w.detach(), x.detach(), None if A is None else A.detach(),
                   None if B is None else B.detach(), act or 0, acc, acc_s, per_sample=True)
    for g, r in zip((gx, gA, gB, gw), one):
        assert (g is None) == (r is None)
        if g is not None:
            assert float((g - r).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max()))
