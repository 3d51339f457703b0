"""GPU: the fused detection loss (csrc/detloss.hip; cfn_hip.ops.detection_loss, torch.ops.cfn.detection_loss, train_fine.detection_loss(fused=True))
against the committed goldens and against an fp64 CPU evaluation of the reference's expressions (F.interpolate / sigmoid / BCE on .double()
inputs).  Where the fused path is compared with the fp64 reference, the composed device path (fused=False) is measured against the same
reference and the requirement is  err_fused <= 2 * err_composed + 1e-7 * |ref|  (max-abs for probs, Frobenius for the logit gradient): the factor
2 allows for different exp / log implementations, the floor is one fp32 rounding.

Tied maxima.  The gradient of cls goes to ONE frame of a row, so the inputs must not leave that choice open.  A literal "no two unmasked frames
share the row maximum" cannot hold at align_corners=False: the half-pixel resize clamps the first and last TL/(2T) frames onto the first / last
logit, so those frames carry the same value by construction (and every frame does at T = 1).  Such frames read ONE logit with weight 1, the
gradient is the same whichever of them is chosen, and they count as one frame here; the precondition asserted on the CPU reference is that the
row maximum among unmasked frames, taken over these groups, beats every other group by more than 4 fp32 ulps of a probability (2^-22; more
than a tie asks for): both device paths are within an ulp or two of the fp64 probabilities, so all three order such a pair the same way."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, t, maxdiff

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _ops():
    from cfn_hip import ops
    return ops


def ref64(logits, labels, masks, ac, crops=1, norm=None, world=1.0, grad=True):
    """the reference's expressions (train_fine.py:199-213) in fp64 on the CPU -> cls, loc, probs, d((cls + loc) / 2) / d logits"""
    x = logits.detach().cpu().double().requires_grad_(grad)
    y, m = labels.detach().cpu().double(), masks.detach().cpu().double()
    B, C, TL = y.shape
    z = F.interpolate(x, TL, mode='linear', align_corners=bool(ac))
    s = torch.sigmoid(z)
    if crops > 1:
        s = s.view(B, crops, C, TL).max(dim=1)[0]
    p = s * m.unsqueeze(1)
    cls = F.binary_cross_entropy(p.max(dim=2)[0], y.max(dim=2)[0])
    nrm = m.sum() * C if norm is None else float(norm)
    loc = F.binary_cross_entropy(p, y, reduction='sum') / nrm * world
    g = torch.autograd.grad((cls + loc) / 2, x)[0] if grad else None
    return float(cls), float(loc), p.detach(), g


def bce64(p, y):
    """ATen's BCE terms (logs clamped at -100) in fp64 on given probabilities"""
    p, y = p.detach().cpu().double(), y.detach().cpu().double()
    return -(y * torch.log(p).clamp(min=-100.0) + (1 - y) * torch.log1p(-p).clamp(min=-100.0))


def assert_no_tied_maximum(p64, masks, T, ac):
    """see the module docstring; p64 (B, C, TL) from ref64 at crops = 1"""
    B, C, TL = p64.shape
    W = F.interpolate(torch.eye(T, dtype=torch.float64).unsqueeze(0), TL, mode='linear', align_corners=bool(ac))[0]      # (T, TL): d z_j / d x_k
    single = (W != 0).sum(0) == 1                       # frames that read one logit only
    group = torch.where(single, W.abs().argmax(0), T + torch.arange(TL))      # one id per logit for those, one id per frame otherwise
    for b in range(B):
        on = masks[b].cpu() > 0
        if not bool(on.any()):
            continue
        pb, gb = p64[b][:, on], group[on]
        top, arg = pb.max(dim=1)
        other = pb.masked_fill(gb.unsqueeze(0) == gb[arg].unsqueeze(1), -1.0).max(dim=1)[0]
        assert bool((top - other > 2.0 ** -22).all()), 'the test inputs leave a row maximum tied (video %d)' % b


def fused_and_composed(logits, labels, masks, ac, crops=1):
    """-> ((cls, loc, probs, grad) of the fused path, the same of the composed device path), gradients of (cls + loc) / 2"""
    import train_fine
    out = []
    for fused in (True, False):
        x = logits.to(DEV).requires_grad_(True)
        cls, loc, probs = train_fine.detection_loss(x, labels.to(DEV), masks.to(DEV), bool(ac), crops=crops, local_norm=True, fused=fused)
        g = torch.autograd.grad((cls + loc) / 2, x)[0]
        out.append((float(cls), float(loc), probs.detach().cpu(), g.cpu()))
    return out


def propagated_loss_bounds(rp, fp, labels, masks):
    """How far the fp32 probabilities `fp` can move the two losses away from their fp64 values at `rp`: both losses are functions of the
    probabilities alone, so to first order  |d loss| <= sum_j |d loss / d p_j| |fp_j - rp_j|  with the derivative of the BCE at the reference,
    (p - y) / (p (1 - p)) over the normaliser.  The derivative itself moves by less than a factor 2 while |fp - rp| stays below half of
    min(p, 1 - p), which is asserted: the bounds returned are twice the first-order term.  (A probability of 1 - 1e-5 under a zero label carries
    a derivative of 1e5: one fp32 rounding of p moves its term by 6e-3.  That is the fp32 format, not the kernel, and why these shapes cannot
    share the fixed 1e-6 of the masked shape.)  -> (cls bound, loc bound)"""
    y, m = labels.double(), masks.double()
    B, C, TL = y.shape
    dp = (fp.double() - rp).abs()
    room = torch.minimum(rp, 1 - rp)
    assert bool((dp[dp > 0] <= 0.5 * room[dp > 0]).all()), 'a probability sits within two fp32 roundings of 0 or 1: first-order bound not valid'
    slope = (rp - y).abs() / (rp * (1 - rp)).clamp(min=1e-300)
    loc = float(torch.where(dp > 0, slope * dp, torch.zeros_like(dp)).sum() / (m.sum() * C))
    top, arg = rp.max(dim=2)
    ytop = y.max(dim=2)[0]
    dtop = torch.maximum(dp.max(dim=2)[0], (fp.double().max(dim=2)[0] - top).abs())
    cls = float(torch.where(dtop > 0, (top - ytop).abs() / (top * (1 - top)).clamp(min=1e-300) * dtop, torch.zeros_like(dtop)).sum() / (B * C))
    return 2 * cls, 2 * loc


def check_against_ref64(logits, labels, masks, ac, crops=1, tag='', fixed_loss_bound=True):
    """fixed_loss_bound: losses within 1e-6 max(1, |ref|) of the fp64 reference (the bound set for the masked shape and the goldens); otherwise
    within that plus what the measured difference of the probabilities accounts for (propagated_loss_bounds).  Either way the losses must equal,
    to 1e-6 max(1, |ref|), the fp64 BCE of the probabilities the fused path itself returned: the loss arithmetic by itself."""
    rc, rl, rp, rg = ref64(logits, labels, masks, ac, crops)
    (fc, fl, fp, fg), (cc, cl, cp, cg) = fused_and_composed(logits, labels, masks, ac, crops)
    ep_f, ep_c = maxdiff(fp, rp), maxdiff(cp, rp)
    eg_f, eg_c, gn = float((fg.double() - rg).norm()), float((cg.double() - rg).norm()), float(rg.norm())
    msg = ('%s ac=%d: cls fused %.9g composed %.9g ref %.9g | loc fused %.9g composed %.9g ref %.9g | probs max-abs err fused %.3e composed %.3e '
           '| grad Frobenius err / |ref| fused %.3e composed %.3e' % (tag, ac, fc, cc, rc, fl, cl, rl, ep_f, ep_c, eg_f / gn, eg_c / gn))
    print(msg)
    tol_c, tol_l = 1e-6 * max(1.0, abs(rc)), 1e-6 * max(1.0, abs(rl))
    own_l = float(bce64(fp, labels).sum() / (masks.double().sum() * labels.shape[1]))
    own_c = float(bce64(fp.max(dim=2)[0], labels.max(dim=2)[0]).mean())
    assert abs(fc - own_c) <= tol_c and abs(fl - own_l) <= tol_l, msg + ' | BCE of the returned probs: cls %.9g loc %.9g' % (own_c, own_l)
    if not fixed_loss_bound:
        bc, bl = propagated_loss_bounds(rp, fp, labels, masks)
        msg += ' | loss bounds: cls %.3e loc %.3e' % (tol_c + bc, tol_l + bl)
        tol_c, tol_l = tol_c + bc, tol_l + bl
    assert abs(fc - rc) <= tol_c and abs(fl - rl) <= tol_l, msg
    assert ep_f <= 2 * ep_c + 1e-7 * float(rp.abs().max()), msg
    assert eg_f <= 2 * eg_c + 1e-7 * gn, msg
    assert bool(torch.isfinite(fg).all()) and bool(torch.isfinite(fp).all()), msg
    return fg


# ---- 1. goldens: both conventions, both crop counts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['loss_ap', 'loss_multicrop'])
@pytest.mark.parametrize('ac', [1, 0])
def test_goldens(name, ac):
    z = load_golden(name)
    n = int(z['crops']) if 'crops' in z else 1
    lg, labels, masks = (t(z[k]).to(DEV) for k in ('logits', 'labels', 'masks'))
    if name == 'loss_ap':       # the -100 clamp is live: positive labels under masked frames
        assert int(((labels > 0) & (masks.unsqueeze(1) == 0)).sum()) > 0
    cls, loc, probs = _ops().detection_loss(lg, labels, masks, bool(ac), crops=n)
    assert abs(float(cls) - float(z['cls_%d' % ac])) <= 1e-6, (float(cls), float(z['cls_%d' % ac]))
    assert abs(float(loc) - float(z['loc_%d' % ac])) <= 1e-6, (float(loc), float(z['loc_%d' % ac]))
    assert probs.shape == labels.shape
    if 'probs_%d' % ac in z:
        assert maxdiff(probs[:, ::13], z['probs_%d' % ac]) <= 1e-6
    else:
        assert maxdiff(probs, ref64(lg, labels, masks, ac, n, grad=False)[2]) <= 1e-6
    # the train_fine entry takes the same route, and want_probs=False changes no loss bit
    import train_fine
    c2, l2, p2 = train_fine.detection_loss(lg, labels, masks, bool(ac), crops=n, local_norm=True, fused=True)
    c3, l3, p3 = _ops().detection_loss(lg, labels, masks, bool(ac), crops=n, want_probs=False)
    assert torch.equal(c2, cls) and torch.equal(l2, loc) and torch.equal(p2, probs) and torch.equal(c3, cls) and torch.equal(l3, loc) and p3 is None


# ---- 2. shapes where the kernel can go wrong -----------------------------------------------------------------------------------------------
SHAPES = {            # name: (B, C, T, TL)
    'masked': (3, 157, 7, 70),       # masks [all, first 41, none]
    'two_passes': (2, 5, 33, 330),   # TL beyond one 256-thread pass
    'lds_tiles': (1, 3, 300, 3000),  # more than one LDS tile of the backward
    't1': (2, 3, 1, 4),
    'down': (2, 3, 9, 4),
    'identity': (2, 4, 5, 5),
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    B, C, T, TL = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    logits = torch.randn(B, C, T, generator=g) * 3
    labels = (torch.rand(B, C, TL, generator=g) < 0.1).float()
    masks = torch.ones(B, TL)
    if name == 'masked':
        masks[1, 41:] = 0
        masks[2] = 0
    elif name == 't1':              # every frame reads the one logit: distinct mask values / a single unmasked frame keep the rows' maxima apart
        masks[0] = torch.tensor([0.25, 1.0, 0.5, 0.75])
        masks[1] = torch.tensor([0.0, 0.0, 1.0, 0.0])
    else:
        masks[B - 1, TL - max(TL // 4, 1):] = 0
    return logits, labels, masks


@pytest.mark.parametrize('ac', [1, 0])
@pytest.mark.parametrize('name', list(SHAPES))
def test_shapes_against_fp64(name, ac):
    logits, labels, masks = shape_case(name)
    if name != 't1':
        assert_no_tied_maximum(ref64(logits, labels, masks, ac, grad=False)[2], masks, logits.shape[2], ac)
    else:           # T = 1: one group per row by construction; the masks above make its maximum a single frame
        p = ref64(logits, labels, masks, ac, grad=False)[2]
        top2 = p.topk(2, dim=2)[0]
        assert bool((top2[..., 0] - top2[..., 1] > 2.0 ** -22).all())
    fg = check_against_ref64(logits, labels, masks, ac, tag=name, fixed_loss_bound=(name == 'masked'))
    if name == 'masked':
        assert bool((fg[2] == 0).all()), 'the fully masked video must get an exactly zero gradient'


# ---- 3. tie rule -----------------------------------------------------------------------------------------------------------------------------
def test_tie_goes_to_the_lowest_index():
    rows = torch.tensor([[[0.5, 2.0, -1.0, 2.0, 0.0], [2.0, 2.0, 2.0, 0.0, 0.0]]])       # (B, C, T) = (1, 2, 5), T = TL
    labels, masks = torch.zeros(1, 2, 5), torch.ones(1, 5)
    xc = rows.clone().requires_grad_(True)
    import train_fine
    gc = torch.autograd.grad(train_fine.detection_loss(xc, labels, masks, True, fused=False)[0], xc)[0]      # CPU autograd
    x = rows.to(DEV).requires_grad_(True)
    cls, _loc, _p = _ops().detection_loss(x, labels.to(DEV), masks.to(DEV), True)
    g = torch.autograd.grad(cls, x)[0].cpu()
    want = torch.zeros(1, 2, 5)
    want[0, 0, 1] = want[0, 1, 0] = float(torch.sigmoid(torch.tensor(2.0))) / 2
    assert torch.equal(g != 0, want != 0), g
    # sigmoid(2) / 2 = 0.44 through exp, two divisions and three products in fp32: 8 roundings of half an ulp (2^-25 below 0.5) at the most
    assert maxdiff(g, want) <= 8 * 2.0 ** -25 and maxdiff(g, gc) <= 8 * 2.0 ** -25, (g, gc)


# ---- 4. saturation ---------------------------------------------------------------------------------------------------------------------------
def test_saturated_logits():
    logits = torch.tensor([[[30.0, -30.0, 120.0, -120.0, 17.0, 16.0]]])
    labels = torch.tensor([[[0.0, 1.0, 0.0, 1.0, 0.0, 0.0]]])
    masks = torch.ones(1, 6)
    x = logits.to(DEV).requires_grad_(True)
    cls, loc, probs = _ops().detection_loss(x, labels.to(DEV), masks.to(DEV), True)
    g = torch.autograd.grad((cls + loc) / 2, x)[0].cpu()
    assert maxdiff(probs, ref64(logits, labels, masks, 1, grad=False)[2]) <= 1e-6
    # the loss arithmetic, separated from a last-bit difference in sigmoid (which at p -> 1 moves a term between 16.6 and 100): fp64 BCE on the
    # probabilities the op returned
    terms = bce64(probs, labels)
    loc_ref = float(terms.sum() / (masks.sum().double() * 1))
    cls_ref = float(bce64(probs.max(dim=2)[0], labels.max(dim=2)[0]).mean())
    assert abs(float(loc) - loc_ref) <= 1e-6 * max(1.0, abs(loc_ref)), (float(loc), loc_ref)
    assert abs(float(cls) - cls_ref) <= 1e-6 * max(1.0, abs(cls_ref)), (float(cls), cls_ref)
    assert loc_ref > 40.0                  # the clamp is what is being summed here
    assert bool(torch.isfinite(g).all()), g
    p = probs.cpu()
    sat = (p == 0) | (p == 1)
    assert int(sat.sum()) >= 3 and bool((g[sat] == 0).all()), (p, g)


# ---- 5. multi-crop backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ac', [1, 0])
def test_multicrop_backward(ac):
    z = load_golden('loss_multicrop')
    fg = check_against_ref64(t(z['logits']), t(z['labels']), t(z['masks']), ac, crops=int(z['crops']), tag='loss_multicrop')
    assert int((fg != 0).sum()) > 0


# ---- 6. norm and world -----------------------------------------------------------------------------------------------------------------------
def test_norm_and_world():
    import train_fine
    logits, labels, masks = (v.to(DEV) for v in shape_case('two_passes'))
    C = labels.shape[1]
    assert not torch.distributed.is_initialized() or torch.distributed.get_world_size() == 1      # the composed path below runs at world 1
    mask_total = masks.sum() * 3                             # as if three ranks held such a shard
    xa, xb = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    ca, la, _ = _ops().detection_loss(xa, labels, masks, True, 1, norm=mask_total * C, world=2.0)
    cb, lb, _ = train_fine.detection_loss(xb, labels, masks, True, mask_total=mask_total, fused=False)
    assert abs(float(la) - 2 * float(lb)) <= 1e-6 * max(1.0, abs(2 * float(lb))) and abs(float(ca) - float(cb)) <= 1e-6
    ga, gb = torch.autograd.grad(la, xa)[0].double(), 2 * torch.autograd.grad(lb, xb)[0].double()
    assert float((ga - gb).norm()) <= 1e-5 * float(gb.norm())        # two fp32 evaluations of one gradient
    # the train_fine entry hands mask_total * C on as the normaliser
    cf, lf, _ = train_fine.detection_loss(logits, labels, masks, True, mask_total=mask_total, fused=True)
    assert abs(float(lf) - float(lb)) <= 1e-6 * max(1.0, abs(float(lb)))
    # norm=None is C * sum(masks)
    l_none = _ops().detection_loss(logits, labels, masks, True)[1]
    l_expl = _ops().detection_loss(logits, labels, masks, True, 1, norm=masks.sum() * C)[1]
    assert torch.equal(l_none, l_expl)


# ---- 7. determinism --------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits():
    logits, labels, masks = (v.to(DEV) for v in shape_case('masked'))
    runs = []
    for _ in range(2):
        x = logits.clone().requires_grad_(True)
        cls, loc, probs = _ops().detection_loss(x, labels, masks, False)
        runs.append((cls, loc, probs, torch.autograd.grad((cls + loc) / 2, x)[0]))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 8. operator route -----------------------------------------------------------------------------------------------------------------------
def test_operator_equals_ops_and_passes_opcheck():
    import cfn_hip.torchlib  # noqa: F401
    z = load_golden('loss_multicrop')
    n = int(z['crops'])
    lg, labels, masks = (t(z[k]).to(DEV) for k in ('logits', 'labels', 'masks'))
    xa, xb = lg.clone().requires_grad_(True), lg.clone().requires_grad_(True)
    oa = torch.ops.cfn.detection_loss(xa, labels, masks, False, n)
    ob = _ops().detection_loss(xb, labels, masks, False, n)
    for a, b in zip(oa[:3], ob):
        assert torch.equal(a, b)
    ga = torch.autograd.grad((oa[0] + oa[1]) / 2, xa)[0]
    gb = torch.autograd.grad((ob[0] + ob[1]) / 2, xb)[0]
    assert torch.equal(ga, gb) and int((ga != 0).sum()) > 0
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    small = (lg[:, :5].clone().requires_grad_(True), labels[:, :5].contiguous(), masks, True, n)
    torch.library.opcheck(torch.ops.cfn.detection_loss.default, small, test_utils=utils)
    torch.library.opcheck(torch.ops.cfn.detection_loss.default, small[:3] + (False, n, masks.sum() * 5, 2.0, False), test_utils=utils)
    o = torch.ops.cfn.detection_loss(*small)
    one = torch.ones((), device=DEV)
    torch.library.opcheck(torch.ops.cfn.detection_loss_backward.default, (one, one, small[0].detach(), small[1], masks, o[3], o[4], o[5], True, n, 1.0),
                          test_utils=('test_schema', 'test_faketensor'))
    with pytest.raises(RuntimeError):
        torch.ops.cfn.detection_loss(lg.double(), labels, masks, True, n)


# ---- 9. capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.capture
def test_forward_and_backward_replay_from_a_graph():
    logits, labels, masks = (v.to(DEV) for v in shape_case('two_passes'))
    other = (torch.randn(logits.shape, generator=torch.Generator().manual_seed(99)) * 3).to(DEV)

    def step(x):
        cls, loc, probs = _ops().detection_loss(x, labels, masks, True)
        return cls, loc, probs, torch.autograd.grad((cls + loc) / 2, x)[0]

    static = logits.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)                                     # warm-up: code objects, allocator pools
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(static)
    with torch.no_grad():
        static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = step(other.clone().requires_grad_(True))
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)


# ---- 10. end to end --------------------------------------------------------------------------------------------------------------------------
def test_train_step_fused_against_composed():
    import train_fine
    from cfn_hip import dist as cdist
    x = torch.randn(1, 3, 8, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    labels = (torch.rand(1, 157, 80, generator=torch.Generator().manual_seed(2)) < 0.1).float().to(DEV)
    masks = torch.ones(1, 80, device=DEV)
    torch.manual_seed(0)
    net = train_fine.build_model(DEV, pretrained=None)
    net.train(False)            # running-statistics BN: well conditioned gradients, so the two routes can be compared tightly
    state = {k: v.clone() for k, v in net.state_dict().items()}
    res = []
    for fused in (True, False):
        net.load_state_dict(state)
        opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
        grads = []
        torch.manual_seed(7)
        cls, loc, probs = train_fine.train_step(net, cdist.GradReducer(net.parameters()), opt, x, labels, masks,
                                                pre_step=lambda: grads.extend(p.grad.detach().clone().flatten() for p in net.parameters() if p.grad is not None),
                                                fused=fused)
        res.append((float(cls), float(loc), probs, torch.cat(grads)))
    (fc, fl, fp, fg), (cc, cl, cp, cg) = res
    assert abs(fc - cc) <= 1e-6 and abs(fl - cl) <= 1e-6, (fc, cc, fl, cl)
    assert maxdiff(fp, cp) <= 1e-6
    assert fg.numel() == cg.numel() > 1000 and bool(torch.isfinite(fg).all())
    assert float((fg - cg).norm() / cg.norm()) <= 1e-4
