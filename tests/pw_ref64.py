"""fp64 reference of the backward of a stride-1 pointwise (1x1x1) conv behind an optional per-(n, c) prologue (test infrastructure):
the data gradient and the weight gradient that cfn_pwconv_bwd_fused computes in one pass, and cfn_pwconv_bwd_data_acc +
cfn_pwconv_bwd_weight in two.  Same arguments as the C ABI; every optional argument may be None:

    G'  = gsc*gy + gs + 2*gq*y                     (gsc = 1, gs = 0, gq = 0 when absent)
    da  = W^T G' ; da[:, :, :, ::s, ::s] += acc    (acc: gradient w.r.t. the post-prologue activation)
    a   = act(A x + B)                             (a = x without a prologue)
    gx  = A * act'(A x + B) * da                   (gx = da without a prologue)
    gA  = sum_q x * act'(.) * da ,  gB = sum_q act'(.) * da ,  gw = sum_{n,q} G' a^T

Everything is computed in float64 on the inputs' device.  tests/test_pw_ref64_cpu.py pins this to fp64 autograd."""
import torch


def _act(z, act):
    """a = act(z) and act'(z); act 0 = none (affine prologue only), 1 = ReLU (act'(0) = 0), 2 = swish"""
    if act == 1:
        return z.clamp_min(0.0), (z > 0).double()
    if act == 2:
        s = torch.sigmoid(z)
        return z * s, s * (1.0 + z * (1.0 - s))
    assert act == 0, act
    return z, torch.ones_like(z)


def _one(gy, y, gs, gq, gsc, w, x, A, B, act, acc, acc_stride):
    N, Cout = gy.shape[:2]
    Cin = x.shape[1]
    sp = lambda v: v.double().reshape(v.shape[0], v.shape[1], *(1,) * (gy.dim() - 2))
    G = gy.double()
    if gsc is not None:
        G = G * sp(gsc)
    if gs is not None:
        G = G + sp(gs)
    if gq is not None:
        G = G + 2.0 * sp(gq) * y.double()
    Gf = G.reshape(N, Cout, -1)
    da = torch.matmul(w.double().t(), Gf).reshape(x.shape)
    if acc is not None:
        s = acc_stride
        da[:, :, :, ::s, ::s] += acc.double()
    xd = x.double()
    gA = gB = None
    if A is None:
        a, gx = xd, da
    else:
        a, d = _act(xd * sp(A) + sp(B), act)
        t = d * da
        gx = sp(A) * t
        gA, gB = (xd * t).sum((2, 3, 4)), t.sum((2, 3, 4))
    gw = torch.matmul(Gf, a.reshape(N, Cin, -1).transpose(1, 2)).sum(0)
    return gx, gA, gB, gw


def pw_ref64(gy, y, gs, gq, gsc, w, x, A, B, act, acc=None, acc_stride=1, per_sample=False):
    """(gx, gA, gB, gw) in float64; gA = gB = None without a prologue.  gy, y: (N, Cout, T, H, W); x: (N, Cin, T, H, W); w: (Cout, Cin);
    gs, gq, gsc, A, B: (N, C); acc: (N, Cin, T, ceil(H/s), ceil(W/s)).  per_sample: one sample at a time (the fp64 temporaries of the
    full-size shapes do not fit at once)."""
    if not per_sample:
        return _one(gy, y, gs, gq, gsc, w, x, A, B, act, acc, acc_stride)
    sl = lambda v, n: None if v is None else v[n:n + 1]
    outs = [_one(*(sl(v, n) for v in (gy, y, gs, gq, gsc)), w, *(sl(v, n) for v in (x, A, B)), act, sl(acc, n), acc_stride)
            for n in range(gy.shape[0])]
    gx = torch.cat([o[0] for o in outs])
    gA = None if A is None else torch.cat([o[1] for o in outs])
    gB = None if A is None else torch.cat([o[2] for o in outs])
    gw = sum(o[3] for o in outs)
    return gx, gA, gB, gw
