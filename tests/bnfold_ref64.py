"""fp64 reference of bn_fold (csrc/bnfold.hip: SubBatchNorm3d statistics -> per-(n, c) prologue coefficients, running-statistics update,
optional squeeze-excite gate), written as one differentiable torch expression (test infrastructure).  Same arguments as cfn_hip.ops.bn_fold;
CPU or GPU tensors; gradients come from autograd on the expression:

    training:  ss[g,c] = sum_i s[i*S+g, c], qq likewise          (G = N/S samples per split group, sample n is in group n % S)
               cnt = count*G ; mean = ss/cnt ; var = max(qq/cnt - mean^2, 0) ; unb = var*cnt/max(cnt-1, 1)
               run_mean' = (1-m)*run_mean + m*mean ; run_var' = (1-m)*run_var + m*unb   (S*C entries, entry g*C + c) ; nbt' = nbt + 1
    eval:      mean = run_mean, var = run_var (C entries) ; buffers and nbt untouched
    rstd = (var+eps)^-1/2 ; A0 = gamma*rstd ; B0 = beta - mean*gamma*rstd             (gamma = 1, beta = 0 when absent)
    gate:      pooled = (s/pool_count)*A0 + B0 ; pre = fc1(pooled) ; h = relu(pre) ; gate = sigmoid(fc2(h))
               A = A0*gate ; B = B0*gate                                              (A = A0, B = B0 without a gate)

The clamp of the variance passes the gradient straight through: it guards against rounding and is not part of the function (the kernel does
the same; torch's batch_norm has no clamp).  tests/test_bnfold_ref64_cpu.py pins this file to F.batch_norm + the module-level SE branch.

gate_dtype=torch.float32 evaluates the SAME expression the way a plain fp32 implementation would: statistics in fp64, A0 / B0 rounded to fp32,
everything after them in fp32.  Its distance from the fp64 result is the fp32 error of the operation itself -- the yardstick the kernel's
gate arithmetic is judged by.

drop names ONE term to leave out (term-visibility checks: a kernel without the term must be told apart from a correct one):
    'direct'      the direct s -> pooled contribution to the gradient of s
    'gate_grad'   the gate's contribution to the gradients of A0 / B0 (pooled depends on them)
    'mean_gvar'   the -2*mean*g_var term of the gradient of the mean
    'unbiased'    the cnt/(cnt-1) factor of running_var
    'pool_count'  pool_count replaced by count"""
import collections

import torch

TERMS = ('direct', 'gate_grad', 'mean_gvar', 'unbiased', 'pool_count')
GRADS = ('s', 'q', 'gamma', 'beta', 'w1', 'b1', 'w2', 'b2')

BnFoldRef = collections.namedtuple('BnFoldRef', 'A B mean rstd run_mean run_var A0 B0 pooled pre h gate nbt')


def bnfold_ref64(s, q, gamma, beta, bufs, training, N, C, S, count, eps, momentum, se=None, pool_count=1.0, gate_dtype=torch.float64, drop=None):
    """-> BnFoldRef(A, B, mean, rstd, run_mean', run_var', A0, B0, pooled, pre, h, gate, nbt').  A, B, A0, B0, pooled, gate: (N, C); mean, rstd:
    (S, C) in training, (1, C) in eval; run_mean', run_var': like the buffers passed in; pre, h: (N, width).  Everything is float64 (values of
    gate_dtype after A0 / B0); pooled, pre, h, gate are None without a gate.  bufs = (running_mean, running_var, num_batches_tracked) is
    read, never written."""
    assert drop is None or drop in TERMS, drop
    run_mean, run_var, nbt = bufs
    rm, rv = run_mean.detach().double(), run_var.detach().double()
    if training:
        assert N % S == 0, (N, S)
        G = N // S
        ss, qq = s.double().view(G, S, C).sum(0), q.double().view(G, S, C).sum(0)
        cnt = float(count) * G
        mean = ss / cnt
        v = qq / cnt - (mean.detach() if drop == 'mean_gvar' else mean) * mean
        var = v + (v.clamp_min(0.0) - v).detach()
        unb = var if drop == 'unbiased' else var * (cnt / max(cnt - 1.0, 1.0))
        new_mean = ((1.0 - momentum) * rm + momentum * mean.detach().reshape(-1)).view_as(rm)
        new_var = ((1.0 - momentum) * rv + momentum * unb.detach().reshape(-1)).view_as(rv)
        new_nbt = nbt + 1
    else:
        mean, var = rm.view(1, C), rv.view(1, C)
        new_mean, new_var, new_nbt = rm, rv, nbt
    rstd = (var + eps) ** -0.5
    ga = torch.ones_like(rstd[0]) if gamma is None else gamma.double()
    be = torch.zeros_like(rstd[0]) if beta is None else beta.double()
    group = torch.arange(N, device=rstd.device) % mean.shape[0]
    A0, B0 = (ga * rstd)[group], (be - mean * ga * rstd)[group]
    if se is None:
        return BnFoldRef(A0, B0, mean, rstd, new_mean, new_var, A0, B0, None, None, None, None, new_nbt)
    dt = gate_dtype
    w1, b1, w2, b2 = se
    Wd = w1.shape[0]
    A0, B0 = A0.to(dt), B0.to(dt)
    pc = float(count) if drop == 'pool_count' else float(pool_count)
    sm = ((s.detach() if drop == 'direct' else s).double() / pc).to(dt)
    pooled = sm * (A0.detach() if drop == 'gate_grad' else A0) + (B0.detach() if drop == 'gate_grad' else B0)
    pre = pooled @ w1.reshape(Wd, C).to(dt).t() + b1.to(dt)
    h = torch.relu(pre)
    gate = torch.sigmoid(h @ w2.reshape(C, Wd).to(dt).t() + b2.to(dt))
    f64 = lambda v: v.double()
    return BnFoldRef(f64(A0 * gate), f64(B0 * gate), mean, rstd, new_mean, new_var, f64(A0), f64(B0), f64(pooled), f64(pre), f64(h), f64(gate),
                     new_nbt)


def bnfold_grads(out, gA, gB, leaves):
    """gradients of sum(gA*A + gB*B) with respect to `leaves` ({name: tensor that requires grad}) -> {name: float64 gradient or None}"""
    names = [k for k, v in leaves.items() if v is not None and v.requires_grad]
    if not (out.A.requires_grad or out.B.requires_grad):
        return {k: None for k in names}
    g = torch.autograd.grad((out.A * gA.double() + out.B * gB.double()).sum(), [leaves[k] for k in names], allow_unused=True)
    return {k: (None if v is None else v.double()) for k, v in zip(names, g)}
