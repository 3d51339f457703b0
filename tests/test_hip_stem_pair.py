"""The stem pair conv1_s -> conv1_t as one kernel each way (csrc/stempair.hip: cfn_stem_pair_fwd / cfn_stem_pair_bwd, ops.stem_pair).

The kernels are specialised to a 224 x 224 clip, so the small axes are N and T.  With run_frames in {0, 4, 1} the shapes cover clips shorter than
the 5-frame window (T = 1, 2, 3), a window exactly full (T = 5), runs of 4 / 2 and 4 / 4 / 3 frames (T = 6, 11: a ragged last run, and halo
frames that are real frames of the neighbouring run), two samples, and every row band including the top one (whose clip halo row lies above the
image) and the bottom one.  run_frames = 1 is there for the backward kernel's walk: its persistent workgroups take ceil(runs / CUs) consecutive
runs each, run = ((sample, chunk), band) with 56 bands, and with one-frame runs (2, 11) has 1232 runs and (2, 6) 672, so that on a 256-CU device
a workgroup walks 5 (3) runs and the walks cross chunk boundaries (another ta / tb, every 56 runs) and, at T = 11, the sample boundary at run 616
(another descriptor base, gs / gq reloaded) in the middle of a walk, with the prefetch one step ahead of the multiply across it.  With
run_frames in {0, 4} no test shape does that: a walk is one run, or two neighbouring bands of one chunk.

Bounds are those of the tests of the two separate ops (tests/test_hip_ops.py): y within 2e-5 of the fp64 composition and statistics within 1e-5
(check_conv), gw_s within 1e-4 (test_stem_conv), gw_t within 2e-4 (check_conv's tol_g); the forward is bit-identical to the two separate kernels.
One fp64 CPU reference per shape is computed once and shared by all tests of the shape."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import relerr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(1, 1), (1, 2), (2, 3), (1, 5), (2, 6), (2, 11)]
RUNS = [0, 4, 1]


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def reference(N, T, H=224):
    """inputs, the cotangents that check_conv builds, and the fp64 CPU results: y, sum, sumsq, and both weight gradients with and without the
    statistics' cotangents"""
    x, ws, wt = rnd(1, N, 3, T, H, H), rnd(2, 24, 3, 1, 3, 3, scale=0.3), rnd(3, 24, 1, 5, 1, 1, scale=0.4)
    out = {'x': x, 'ws': ws, 'wt': wt}
    for bn in (True, False):
        wsd, wtd = ws.double().requires_grad_(True), wt.double().requires_grad_(True)
        xs = F.conv3d(x.double(), wsd, stride=(1, 2, 2), padding=(0, 1, 1))
        y = F.conv3d(xs, wtd, padding=(2, 0, 0), groups=24)
        s, q = y.sum((2, 3, 4)), (y * y).sum((2, 3, 4))
        r, rs, rq = rnd(7, *y.shape), rnd(8, *s.shape).double(), rnd(9, *q.shape).double() * 0.1
        loss = (y * r).sum()
        if bn:
            loss = loss + (s * rs).sum() + (q * rq).sum()
        loss.backward()
        out['gws', bn], out['gwt', bn] = wsd.grad.reshape(24, 27), wtd.grad.reshape(24, 5)
    out.update(y=y.detach(), s=s.detach(), q=q.detach(), r=r, rs=rs, rq=rq)
    return out


def _dev(ref, *names):
    return [ref[k].to(DEV).contiguous() for k in names]


def pair_forward(x, ws2, wt2):
    """the two separate entry points"""
    import cfn_hip
    N, _, T, H, W = x.shape
    xs = torch.empty(N, 24, T, H // 2, W // 2, device=DEV)
    y = torch.empty_like(xs)
    s, q = torch.zeros(N, 24, dtype=torch.float64, device=DEV), torch.zeros(N, 24, dtype=torch.float64, device=DEV)
    cfn_hip.call('cfn_stem_conv_fwd', x, ws2, xs, N, 3, 24, T, H, W)
    cfn_hip.call('cfn_dwconv_t5_fwd', xs, wt2, y, s, q, N, 24, T, (H // 2) * (W // 2))
    return xs, y, s, q


def fused_forward(x, ws2, wt2, run_frames):
    import cfn_hip
    N, _, T, H, W = x.shape
    xs = torch.full((N, 24, T, H // 2, W // 2), float('nan'), device=DEV)
    y = torch.full_like(xs, float('nan'))
    s, q = torch.zeros(N, 24, dtype=torch.float64, device=DEV), torch.zeros(N, 24, dtype=torch.float64, device=DEV)
    assert cfn_hip.call_try('cfn_stem_pair_fwd', x, ws2, wt2, xs, y, s, q, N, 3, 24, T, H, W, run_frames)
    return xs, y, s, q


def pair_backward(gy, y, gs, gq, wt2, xs, x):
    import cfn_hip
    N, _, T, H, W = x.shape
    gxs = torch.empty_like(xs)
    gwt, gws = torch.zeros(24, 5, dtype=torch.float64, device=DEV), torch.zeros(24, 27, dtype=torch.float64, device=DEV)
    assert cfn_hip.call_try('cfn_dwconv_t5_bwd_fused', gy, y, gs, gq, wt2, xs, gxs, gwt, N, 24, T, (H // 2) * (W // 2))
    cfn_hip.call('cfn_stem_conv_bwd_weight', gxs, x, gws, N, 3, 24, T, H, W)
    return gwt, gws


def fused_backward(gy, y, gs, gq, wt2, xs, x, run_frames):
    import cfn_hip
    N, _, T, H, W = x.shape
    gwt, gws = torch.zeros(24, 5, dtype=torch.float64, device=DEV), torch.zeros(24, 27, dtype=torch.float64, device=DEV)
    assert cfn_hip.call_try('cfn_stem_pair_bwd', gy, y, gs, gq, wt2, xs, x, gwt, gws, N, 3, 24, T, H, W, run_frames)
    return gwt, gws


@pytest.mark.parametrize('run_frames', RUNS)
@pytest.mark.parametrize('N,T', SHAPES)
def test_forward(N, T, run_frames):
    """xs and y bit-identical to cfn_stem_conv_fwd + cfn_dwconv_t5_fwd; y and the statistics against the fp64 CPU composition"""
    ref = reference(N, T)
    x, ws, wt = _dev(ref, 'x', 'ws', 'wt')
    ws2, wt2 = ws.reshape(24, 27), wt.reshape(24, 5)
    xs0, y0, s0, q0 = pair_forward(x, ws2, wt2)
    xs1, y1, s1, q1 = fused_forward(x, ws2, wt2, run_frames)
    assert torch.equal(xs1, xs0)
    assert torch.equal(y1, y0)
    e = dict(y=relerr(y1, ref['y']), s=relerr(s1, ref['s']), q=relerr(q1, ref['q']), s_pair=relerr(s1, s0), q_pair=relerr(q1, q0))
    print('stem_pair_fwd N=%d T=%d run_frames=%d: %s' % (N, T, run_frames, e))
    assert e['y'] <= 2e-5
    assert e['s'] <= 1e-5 and e['q'] <= 1e-5 and e['s_pair'] <= 1e-5 and e['q_pair'] <= 1e-5


@pytest.mark.parametrize('bn', [True, False])
@pytest.mark.parametrize('run_frames', RUNS)
@pytest.mark.parametrize('N,T', SHAPES)
def test_backward(N, T, run_frames, bn):
    """gw_s and gw_t against fp64 CPU autograd of conv3d o conv3d with a random cotangent on y, sum and sumsq (bn) or on y alone (y / gsumsq
    null: the kernel without the batch-norm terms), and against the two separate kernels on the same inputs"""
    ref = reference(N, T)
    x, ws, wt, gy = _dev(ref, 'x', 'ws', 'wt', 'r')
    ws2, wt2 = ws.reshape(24, 27), wt.reshape(24, 5)
    xs, y, _, _ = pair_forward(x, ws2, wt2)
    gs, gq = (_dev(ref, 'rs', 'rq')) if bn else (None, None)
    gwt1, gws1 = fused_backward(gy, y if bn else None, gs, gq, wt2, xs, x, run_frames)
    gwt0, gws0 = pair_backward(gy, y if bn else None, gs, gq, wt2, xs, x)
    e = dict(gws=relerr(gws1, ref['gws', bn]), gwt=relerr(gwt1, ref['gwt', bn]), gws_pair=relerr(gws1, gws0), gwt_pair=relerr(gwt1, gwt0))
    print('stem_pair_bwd N=%d T=%d run_frames=%d bn=%s: %s' % (N, T, run_frames, bn, e))
    assert e['gws'] <= 1e-4 and e['gws_pair'] <= 1e-4
    assert e['gwt'] <= 2e-4 and e['gwt_pair'] <= 2e-4


@pytest.mark.parametrize('run_frames', RUNS)
def test_repeats_bit_for_bit_in_deterministic_mode(run_frames):
    import cfn_hip
    ref = reference(2, 11)
    x, ws, wt, gy, gs, gq = _dev(ref, 'x', 'ws', 'wt', 'r', 'rs', 'rq')
    ws2, wt2 = ws.reshape(24, 27), wt.reshape(24, 5)
    prev = cfn_hip.deterministic(True)
    try:
        a = fused_forward(x, ws2, wt2, run_frames)
        b = fused_forward(x, ws2, wt2, run_frames)
        ga = fused_backward(gy, a[1], gs, gq, wt2, a[0], x, run_frames)
        gb = fused_backward(gy, a[1], gs, gq, wt2, a[0], x, run_frames)
    finally:
        cfn_hip.deterministic(prev)
    for u, v in zip(a + ga, b + gb):
        assert torch.equal(u, v)


def _op_grads(fn, x, ws, wt, r, rs, rq):
    wsl, wtl = ws.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    y, s, q = fn(x, wsl, wtl)
    ((y * r).sum() + (s * rs).sum() + (q * rq).sum()).backward()
    return y.detach(), s.detach(), q.detach(), wsl.grad, wtl.grad


def _separate_ops(x, ws, wt):
    from cfn_hip import ops
    return ops.dwconv_t5(ops.stem_conv(x, ws), wt, stats=True)


def _assert_same_as_separate(x, ws, wt, exact_grads):
    from cfn_hip import ops
    N = x.shape[0]
    r, rs, rq = rnd(7, N, 24, x.shape[2], x.shape[3] // 2, x.shape[4] // 2).to(DEV), rnd(8, N, 24).double().to(DEV), (rnd(9, N, 24).double() * 0.1).to(DEV)
    a = _op_grads(lambda *v: ops.stem_pair(*v, stats=True), x, ws, wt, r, rs, rq)
    b = _op_grads(_separate_ops, x, ws, wt, r, rs, rq)
    assert torch.equal(a[0], b[0])
    if exact_grads:                                      # the same kernels on the same tensors: only the arrival order of the fp64 atomics differs
        for u, v in zip(a[1:], b[1:]):
            assert relerr(u, v) <= 1e-6
    else:
        assert relerr(a[1], b[1]) <= 1e-5 and relerr(a[2], b[2]) <= 1e-5
        assert relerr(a[3], b[3]) <= 1e-4 and relerr(a[4], b[4]) <= 2e-4


def test_declines_other_geometry_and_op_still_gives_the_pair():
    """a 112 x 112 clip: both entry points return -1 without launching, ops.stem_pair runs the separate kernels"""
    import cfn_hip
    N, T, H = 1, 3, 112
    x, ws, wt = rnd(1, N, 3, T, H, H).to(DEV), rnd(2, 24, 3, 1, 3, 3, scale=0.3).to(DEV), rnd(3, 24, 1, 5, 1, 1, scale=0.4).to(DEV)
    ws2, wt2 = ws.reshape(24, 27), wt.reshape(24, 5)
    xs = torch.zeros(N, 24, T, H // 2, H // 2, device=DEV)
    y, gy = torch.zeros_like(xs), torch.ones_like(xs)
    s, q = torch.zeros(N, 24, dtype=torch.float64, device=DEV), torch.zeros(N, 24, dtype=torch.float64, device=DEV)
    gwt, gws = torch.zeros(24, 5, dtype=torch.float64, device=DEV), torch.zeros(24, 27, dtype=torch.float64, device=DEV)
    assert not cfn_hip.call_try('cfn_stem_pair_fwd', x, ws2, wt2, xs, y, s, q, N, 3, 24, T, H, H, 0)
    assert not cfn_hip.call_try('cfn_stem_pair_bwd', gy, y, s, q, wt2, xs, x, gwt, gws, N, 3, 24, T, H, H, 0)
    torch.cuda.synchronize()
    assert float(xs.abs().max()) == 0 and float(y.abs().max()) == 0 and float(gwt.abs().max()) == 0 and float(gws.abs().max()) == 0
    _assert_same_as_separate(x, ws, wt, exact_grads=True)


def test_declines_misaligned_clip_and_op_still_gives_the_pair():
    """a contiguous view that starts 4 bytes into an allocation is not 16-byte aligned"""
    import cfn_hip
    N, T, H = 1, 2, 224
    ws, wt = rnd(2, 24, 3, 1, 3, 3, scale=0.3).to(DEV), rnd(3, 24, 1, 5, 1, 1, scale=0.4).to(DEV)
    flat = torch.zeros(N * 3 * T * H * H + 1, device=DEV)
    x = flat[1:].view(N, 3, T, H, H)
    x.copy_(rnd(1, N, 3, T, H, H))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    xs = torch.zeros(N, 24, T, H // 2, H // 2, device=DEV)
    y, gy = torch.zeros_like(xs), torch.ones_like(xs)
    s, q = torch.zeros(N, 24, dtype=torch.float64, device=DEV), torch.zeros(N, 24, dtype=torch.float64, device=DEV)
    gwt, gws = torch.zeros(24, 5, dtype=torch.float64, device=DEV), torch.zeros(24, 27, dtype=torch.float64, device=DEV)
    assert not cfn_hip.call_try('cfn_stem_pair_fwd', x, ws.reshape(24, 27), wt.reshape(24, 5), xs, y, s, q, N, 3, 24, T, H, H, 0)
    assert not cfn_hip.call_try('cfn_stem_pair_bwd', gy, y, s, q, wt.reshape(24, 5), xs, x, gwt, gws, N, 3, 24, T, H, H, 0)
    _assert_same_as_separate(x, ws, wt, exact_grads=True)


@pytest.mark.parametrize('switch', ['0', '1', '2', '3'])
def test_switch_is_read_per_call(switch, monkeypatch):
    """CFN_STEM_PAIR: bit 0 = fused forward, bit 1 = fused backward; every setting gives the pair's forward bits and its gradients to the bounds above
    (to fp32 rounding with 0: the same four kernels)"""
    ref = reference(2, 6)
    x, ws, wt = _dev(ref, 'x', 'ws', 'wt')
    monkeypatch.setenv('CFN_STEM_PAIR', switch)
    _assert_same_as_separate(x, ws, wt, exact_grads=(switch == '0'))
