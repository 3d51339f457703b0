"""The streaming kernels of csrc/elementwise.hip and of its 16-bit twin csrc/streambf16.hip (bf16, and fp16 through streamf16.hip) -- the
block tail bn_add_relu (forward, one-tensor backward bwd_g, two-tensor backward), affine_act, channel_stats, pool_hw (general kernel and the
global-mean wave kernel) and film -- against the fp64 references of tests/elementwise_ref64.py (pinned to stock torch, and their bounds shown
to discriminate, by tests/test_elementwise_ref64_cpu.py).  The cases and what each one reaches are listed next to their inputs there.

Bounds.  Elementwise |kernel - ref| <= (n + 8) 2^-24 mag (n, mag per output: elementwise_ref64's docstring); an element without a summand is
an exact zero; g of a single gradient is bit-equal to gout or an exact 0; 16-bit g is bit-equal to the reference rounded once; mask words
are compared exactly, against the reference and against the stored `out`.  Every output is prefilled with NaN (masks with a sentinel word)
and sits inside a larger allocation whose sentinel guards on both sides are checked afterwards: the flat kernels issue out-of-range buffer
accesses on purpose.  The worst err / bound of every case goes to the junit report (elementwise_fp64).

Not reachable here: bn_add_relu_fwd_kernel<4> and bn_add_relu_bwd_g_kernel<4> (the non-flat grid kernels) run only for a channel of more
than 2 GB, which no test of a few seconds can allocate and check; there is no hook to force them.

Largest err / bound seen on an MI355X, per op and output (1.0 is the bound):
    bn_add_relu fp32     out 0.20, g 0.10 with two gradients (bit-equal with one), gA 0.03, gB 0.03, gAr 0.04; two-tensor backward gy 0.21,
                         gres 0.22, gA 0.02, gB 0.02, gAr 0.02; through ops with split=True the same figures
    bn_add_relu 16-bit   out 1.00 (the storage rounding reaches its half ulp; the fp32 part is invisible next to it), g bit-equal, gA, gB,
                         gAr exact (multiples of 2^-12 that fp32 sums without rounding), bf16 and fp16 alike
    affine_act           none / ReLU: out 0.16, gx 0.36, gA 0.02, gB 0.02; Swish: out 0.15, gx 0.28, gA 0.11, gB 0.10; sigmoid: out 0.13,
                         gx 0.39, gA 0.20, gB 0.15
    channel_stats        sum 0.01, sumsq 0.04
    pool_hw fp32         out 0.20 / 0.18 / 0.09 (none / ReLU / Swish), gx 0.17 / 0.17 / 0.21, gA 0.07, gB 0.07
    pool_hw 16-bit       out 0.21, gx 1.00 (half a storage ulp), gA 0.06, gB 0.07
    pool_hw1             out 0.02 / 0.18 / 0.12 / 0.08 (none / ReLU / Swish / sigmoid), gx 0.15 / 0.23 / 0.21 / 0.38, gA 0.06, gB 0.08
    film                 out 0.10, gx 0.11, gm 0.21, gc 0.18
Swish and sigmoid: the term (|z| + 8) 2^-23 |val| assumes one ulp each for the hardware exp and rcp.  Measured against the fp64 reference with
z over [-12, 12]: worst err / bound 0.15 (Swish) and 0.13 (sigmoid) through affine_act, 0.12 and 0.08 through pool_hw: the assumption holds
with a margin of 6, elementwise_ref64.ACT_SCALE stays 1.

fp16 finding.  Before this suite the fp16 forward took the mask bit from the fp32 pre-activation: z = 2^-26 and 2^-25 store as +0 but set the
bit, and the mask route returned g = gout where the `out` route returned 0 (test_bn_add_relu_f16_rounding_to_zero failed with g = 1.5 on all
three channels).  The stored value is now authoritative: the bit is taken from the packed word.

The checks were also run once against a scratch build of elementwise.hip with each of the twelve errors of elementwise_ref64.MUTANTS in the
kernels themselves (the same build with no error switched on passes): every one was caught.  Factor over the bound: relu_ge 1.7e6 and up
(inf at the planted zeros), drop_gout2 1.4e6 .. 6e9, drop_br 9e4 and up, gar_from_y 1e4 .. 1.2e6, mask_nibble_reversed 1.7e6 (g) besides
the mask words, mask_tail_bits_set through the mask words alone (no value moves: the backward never uses a bit past vol), last_chunk_dropped
1.5e6 and inf (the NaN prefill stays), film_swap_hw 1.5e7 .. 1.3e8, film_block_f_minus_1 inf (gx of the skipped row and column stays
unwritten), pool_end_floor 6e5 .. 2.9e6 (inf where a window comes out empty: 3 x 5 -> 7 x 7), pool_swap_hw 1.8e4 .. 3.6e6 and inf,
pool1_first_sweep_only inf (the frames from 512 on keep their NaN prefill)."""
import pytest
import torch

import elementwise_ref64 as E

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
SENT = -7777.0
GUARD = 64                               # elements on each side: a multiple of 16 bytes for every element type used
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
SFX = {'f32': '', 'bf16': '_bf16', 'f16': '_f16'}
KINDS = ('f32', 'bf16', 'f16')


def lib():
    import cfn_hip
    from cfn_hip import ops  # noqa: F401  (cfn_hip.ops)
    return cfn_hip


class Guarded(object):
    """n elements inside a larger allocation: GUARD + off sentinel elements before, GUARD after.  src: the values (any shape; cast to
    dtype); else every element = fill.  off = 1 makes the view start one element past a 16-byte boundary"""

    def __init__(self, n, dtype, fill=NAN, src=None, off=0):
        sent = 0x5A5A5A5A if dtype == torch.int32 else SENT
        self.buf = torch.full((2 * GUARD + off + n,), sent, dtype=dtype, device=DEV)
        self.lo, self.n = GUARD + off, n
        self.t = self.buf[self.lo:self.lo + n]
        if src is not None:
            self.t.copy_(src.reshape(-1).to(dtype))
        else:
            self.t.fill_(sent if dtype == torch.int32 else fill)
        self.sent = self.buf.new_full((), sent)
        assert self.t.is_contiguous() and (self.t.data_ptr() % 16 == 0) == (off == 0)

    def intact(self):
        return bool((self.buf[:self.lo] == self.sent).all()) and bool((self.buf[self.lo + self.n:] == self.sent).all())


def put(v, dtype=None, off=0):
    """an input on the device (misaligned by one element with off = 1); None stays None"""
    return None if v is None else Guarded(v.numel(), dtype or v.dtype, src=v, off=off).t


def report(record, tag, worst):
    if record is not None:
        record('elementwise_fp64', repr(dict(case=tag, worst=worst)))
    for k, w in worst.items():
        assert w <= 1.0, (tag, k, w)


def guards_ok(tag, outs):
    for k, gd in outs.items():
        if gd is not None:
            assert gd.intact(), (tag, k, 'a guard element next to the output was overwritten')


# ---- bn_add_relu ----------------------------------------------------------------------------------------------------------------------------
def tail_words(kind, NC, vol):
    per = 4 if kind == 'f32' else 8
    return NC * -(-vol // E.WG) * 256 if vol % per == 0 else 0


def tail_run(kind, name, route, c=None, v=None):
    """forward + one-tensor backward through the C ABI; route 'mask' or 'out' -> dict of device results (+ 'mask' int64 words on the CPU)"""
    c = c or E.TAIL_CASES[kind][name]
    v = v or E.tail_inputs(kind, name)
    NC, vol, dt, sfx, off = c.NC, c.vol, DT[kind], SFX[kind], int(c.misaligned)
    y, res, gout, gout2 = (put(v[k], dt, off) for k in ('y', 'res', 'gout', 'gout2'))
    A, B, Ar, Br = (put(v[k]) for k in ('A', 'B', 'Ar', 'Br'))
    words = lib().query('cfn_bn_add_relu_mask_words' + sfx, NC, vol)
    assert words == tail_words(kind, NC, vol)
    outs = {'out': Guarded(NC * vol, dt, off=off), 'g': Guarded(NC * vol, dt, off=off), 'gA': Guarded(NC, torch.float64, 0.0),
            'gB': Guarded(NC, torch.float64, 0.0), 'gAr': Guarded(NC, torch.float64, 0.0) if Ar is not None else None,
            'mask': Guarded(words, torch.int32) if route == 'mask' else None}
    t = lambda k: None if outs[k] is None else outs[k].t
    lib().call('cfn_bn_add_relu_fwd' + sfx, y, A, B, res, Ar, Br, t('out'), t('mask'), NC, vol)
    lib().call('cfn_bn_add_relu_bwd_g' + sfx, gout, gout2, None if route == 'mask' else t('out'), t('mask'), y,
               res if Ar is not None else None, t('g'), t('gA'), t('gB'), t('gAr'), NC, vol)
    torch.cuda.synchronize()
    guards_ok((kind, name, route), outs)
    got = {k: (None if outs[k] is None else outs[k].t.clone()) for k in outs}
    for k in ('out', 'g'):
        got[k] = got[k].view(NC, vol)
    if got['mask'] is not None:
        got['mask'] = got['mask'].cpu().long() & 0xffffffff
    return got


def tail_check(record, kind, name, route, got, ref):
    c = E.TAIL_CASES[kind][name]
    worst = {'out': E.ratio_x(got['out'].float(), ref['out'], ref['out_extra'])}
    for k in ('g', 'gA', 'gB') + (('gAr',) if c.ar else ()):
        worst[k] = E.ratio(got[k].float() if k == 'g' else got[k], ref[k])
    report(record, (kind, name, route), worst)
    out, g = got['out'].float().cpu(), got['g'].float().cpu()
    assert got['out'].dtype == DT[kind] and got['g'].dtype == DT[kind]
    assert torch.equal(out > 0, ref['pos'])
    p = c.NC - 1
    for i in E.PLANT:                                       # the planted exact zeros: out = 0, g = 0 although gout != 0
        assert float(out[p, i]) == 0.0 and float(g[p, i]) == 0.0, (kind, name, route, i)
    if not c.two or kind != 'f32':                          # one gradient / 16-bit storage: bit-equal
        assert torch.equal(g, ref['g'].val.float()), (kind, name, route, 'g is not bit-equal')
    if route == 'mask':
        per = 4 if kind == 'f32' else 8
        assert torch.equal(got['mask'], ref['mask']), (kind, name, 'mask words differ from the reference')
        assert torch.equal(got['mask'], E.mask_words(out > 0, per)), (kind, name, 'mask bits differ from out > 0')
    return worst


@pytest.mark.parametrize('kind,name', [(k, n) for k in KINDS for n in E.TAIL_CASES[k]])
def test_bn_add_relu_fp64(kind, name, record_property):
    """cfn_bn_add_relu_fwd and cfn_bn_add_relu_bwd_g of every case of elementwise_ref64.TAIL_CASES, with the bit mask and with `out`
    (vector routes) or with `out` alone (scalar routes, where cfn_bn_add_relu_mask_words is 0 or the tensors are misaligned): out, g, gA,
    gB, gAr within their bounds, every mask word written, each bit equal to out > 0 at its documented position and 0 past vol, the planted
    exact zeros, the sentinel guards.  A misaligned view refuses a mask (and launches nothing) and then matches on the scalar route.  In
    deterministic mode g, gA, gB, gAr of the mask route are bit-equal to those of the out route"""
    c = E.TAIL_CASES[kind][name]
    ref = E.tail_reference(kind, name)
    vec = E.tail_route(kind, name)[0]
    assert (lib().query('cfn_bn_add_relu_mask_words' + SFX[kind], c.NC, c.vol) > 0) == (vec or c.misaligned)
    if c.misaligned:
        with pytest.raises(RuntimeError, match='bit mask'):
            tail_run(kind, name, 'mask')
    was = lib().deterministic(True)
    try:
        by_route = {r: tail_run(kind, name, r) for r in (('mask', 'out') if vec else ('out',))}
    finally:
        lib().deterministic(was)
    for r, got in by_route.items():
        tail_check(record_property, kind, name, r, got, ref)
    if vec:
        for k in ('out', 'g', 'gA', 'gB') + (('gAr',) if c.ar else ()):
            assert torch.equal(by_route['mask'][k], by_route['out'][k]), (kind, name, k, 'mask route and out route differ')


@pytest.mark.parametrize('name', ['v1020', 'v8196-00', 'v8196-11', 's5-10', 's2049', 'm1024'])
def test_bn_add_relu_two_tensor_backward_fp64(name, record_property):
    """cfn_bn_add_relu_bwd (the tail without a link) on the float4 and the scalar routes: gy = g A and gres = g Ar within one more
    rounding, gA, gB, and gAr only with Ar"""
    c = E.TAIL_F32[name]
    v, ref = E.tail_inputs('f32', name), E.tail_reference('f32', name)
    NC, vol, off = c.NC, c.vol, int(c.misaligned)
    y, res, gout, gout2 = (put(v[k], off=off) for k in ('y', 'res', 'gout', 'gout2'))
    A, B, Ar, Br = (put(v[k]) for k in ('A', 'B', 'Ar', 'Br'))
    out = Guarded(NC * vol, torch.float32, off=off)
    lib().call('cfn_bn_add_relu_fwd', y, A, B, res, Ar, Br, out.t, None, NC, vol)
    outs = {'gy': Guarded(NC * vol, torch.float32, off=off), 'gres': Guarded(NC * vol, torch.float32, off=off),
            'gA': Guarded(NC, torch.float64, 0.0), 'gB': Guarded(NC, torch.float64, 0.0),
            'gAr': Guarded(NC, torch.float64, 0.0) if c.ar else None, 'out': out}
    lib().call('cfn_bn_add_relu_bwd', gout, gout2, out.t, y, A, res, Ar, outs['gy'].t, outs['gres'].t, outs['gA'].t, outs['gB'].t,
               outs['gAr'].t if c.ar else None, NC, vol)
    torch.cuda.synchronize()
    guards_ok(name, outs)
    keys = ('gy', 'gres', 'gA', 'gB') + (('gAr',) if c.ar else ())
    report(record_property, ('bwd', name), {k: E.ratio(outs[k].t.view(ref[k].val.shape), ref[k]) for k in keys})
    if not c.ar and not c.two:                              # gres = g * 1 = gout or 0, bit-equal
        assert torch.equal(outs['gres'].t.view(NC, vol).cpu(), ref['g'].val.float())


def _as5d(v, NC, vol):
    return v.view(1, NC, 1, 1, vol)


def test_bn_add_relu_split_through_ops(record_property):
    """ops.bn_add_relu(..., split=True, link=None): both returned tensors receive a cotangent (gout and gout2 of the case), and the
    gradients of y, res, A, B, Ar, Br match the reference of case v8196-11"""
    name = 'v8196-11'
    c, v, ref = E.TAIL_F32[name], E.tail_inputs('f32', name), E.tail_reference('f32', name)
    leaf = {k: _as5d(v[k], c.NC, c.vol).clone().to(DEV).requires_grad_(True) for k in ('y', 'res')}
    leaf.update({k: v[k].view(1, c.NC).clone().to(DEV).requires_grad_(True) for k in ('A', 'B', 'Ar', 'Br')})
    o1, o2 = lib().ops.bn_add_relu(leaf['y'], leaf['A'], leaf['B'], leaf['res'], leaf['Ar'], leaf['Br'], split=True, link=None)
    assert o1.data_ptr() == o2.data_ptr() and o1 is not o2
    torch.autograd.backward([o1, o2], [_as5d(v['gout'], c.NC, c.vol).to(DEV), _as5d(v['gout2'], c.NC, c.vol).to(DEV)])
    torch.cuda.synchronize()
    got = {'out': o1.detach(), 'gy': leaf['y'].grad, 'gres': leaf['res'].grad, 'gA': leaf['A'].grad, 'gB': leaf['B'].grad,
           'gAr': leaf['Ar'].grad, 'gBr': leaf['Br'].grad}
    ref = dict(ref, gBr=ref['gB'])
    report(record_property, ('split', name), {k: E.ratio(got[k].reshape(ref[k].val.shape), ref[k]) for k in got})


@pytest.mark.parametrize('kind', KINDS)
def test_bn_add_relu_link_on_a_misaligned_view(kind, record_property):
    """ops.bn_add_relu(..., link=TailLink()) on contiguous y / res that start one element past a 16-byte boundary: the op asks for no mask
    (the entry point would refuse it), takes the `out` route and matches"""
    name = 'm1024' if kind == 'f32' else 'm2048'
    c = E.TAIL_CASES[kind][name]
    v = dict(E.tail_inputs(kind, name), gout2=None)
    ref = E.tail_ref64(v['y'], v['res'], v['A'], v['B'], v['Ar'], v['Br'], v['gout'], None, 8, store=E.STORE[kind])
    y = _as5d(put(v['y'], DT[kind], off=1), c.NC, c.vol).detach().requires_grad_(True)
    res = _as5d(put(v['res'], DT[kind], off=1), c.NC, c.vol).detach().requires_grad_(True)
    assert y.data_ptr() % 16 and res.data_ptr() % 16 and y.is_contiguous()
    A, B, Ar, Br = (v[k].view(1, c.NC).clone().to(DEV).requires_grad_(True) for k in ('A', 'B', 'Ar', 'Br'))
    link = lib().ops.TailLink()
    out = lib().ops.bn_add_relu(y, A, B, res, Ar, Br, link=link)
    out.backward(_as5d(v['gout'], c.NC, c.vol).to(DT[kind]).to(DEV))
    torch.cuda.synchronize()
    assert link.done and torch.equal(link.y_scale, A.detach().double())
    got = {'out': out.detach().float(), 'g': y.grad.float(), 'gA': A.grad, 'gB': B.grad, 'gAr': Ar.grad}
    worst = {k: (E.ratio_x(got[k].reshape(ref[k].val.shape), ref[k], ref['out_extra']) if k == 'out' else
                 E.ratio(got[k].reshape(ref[k].val.shape), ref[k])) for k in got}
    report(record_property, ('link-misaligned', kind), worst)
    assert torch.equal(res.grad, y.grad)


def test_bn_add_relu_f16_rounding_to_zero():
    """fp16: a positive fp32 pre-activation of 2^-26 or 2^-25 stores as +0, 1.5 2^-25 as 2^-24.  The stored out, the mask bit and the g of
    both backward routes agree with each other and with `stored out > 0`"""
    y, res, A, B, gout, stored_pos = E.f16_tiny_inputs()
    NC, vol = y.shape
    v = dict(y=y, res=res, A=A, B=B, Ar=None, Br=None, gout=gout, gout2=None)
    by_route = {r: tail_run('f16', 'tiny', r, E.Tail(NC, vol, False, False, False), v) for r in ('mask', 'out')}
    want = stored_pos.view(NC, 1).expand(NC, vol)
    for r, got in by_route.items():
        assert torch.equal(got['out'].float().cpu() > 0, want), (r, 'stored out')
        assert torch.equal(got['g'].float().cpu() != 0, want), (r, 'g disagrees with the stored out', got['g'][:, 0].tolist())
    assert torch.equal(by_route['mask']['mask'], E.mask_words(want, 8)), 'mask bits disagree with the stored out'
    assert torch.equal(by_route['mask']['gB'], by_route['out']['gB'])


# ---- affine_act, channel_stats ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('vol', E.AFF_VOLS)
def test_affine_act_and_channel_stats_fp64(vol, act, record_property):
    """volumes 4 and 5, one workgroup exactly (8192), one more float4 (8196), and 2049 (two scalar workgroups); z over [-12, 12].  ReLU and
    none: (n + 8) 2^-24 mag; Swish and sigmoid: the one-ulp-exp-and-rcp bound of elementwise_ref64.act_ref"""
    x, A, B, g = E.aff_inputs(vol, act)
    ref = E.aff_reference(vol, act)
    NC = E.AFF_NC
    xd, gd, Ad, Bd = put(x), put(g), put(A), put(B)
    outs = {'out': Guarded(NC * vol, torch.float32), 'gx': Guarded(NC * vol, torch.float32)}
    outs.update({k: Guarded(NC, torch.float64, 0.0) for k in ('gA', 'gB', 'sum', 'sumsq')})
    lib().call('cfn_affine_act_fwd', xd, Ad, Bd, act, outs['out'].t, NC, vol)
    lib().call('cfn_affine_act_bwd', gd, xd, Ad, Bd, act, outs['gx'].t, outs['gA'].t, outs['gB'].t, NC, vol)
    lib().call('cfn_channel_stats', xd, outs['sum'].t, outs['sumsq'].t, NC, vol)
    torch.cuda.synchronize()
    guards_ok(('affine', vol, act), outs)
    report(record_property, ('affine_act', vol, act), {k: E.ratio(outs[k].t.view(ref[k].val.shape), ref[k]) for k in outs})


# ---- pool_hw ----------------------------------------------------------------------------------------------------------------------------------
def pool_run(kind, T, H, W, OH, OW, pro, act):
    x, A, B, g = E.pool_inputs(kind, T, H, W, OH, OW, pro, act)
    ref = E.pool_reference(kind, T, H, W, OH, OW, pro, act)
    NC, dt, sfx = E.POOL_NC, DT[kind], SFX[kind]
    xd, gd, Ad, Bd = put(x, dt), put(g), put(A), put(B)
    outs = {'out': Guarded(NC * T * OH * OW, torch.float32), 'gx': Guarded(NC * T * H * W, dt),
            'gA': Guarded(NC, torch.float64, 0.0) if pro else None, 'gB': Guarded(NC, torch.float64, 0.0) if pro else None}
    t = lambda k: None if outs[k] is None else outs[k].t
    lib().call('cfn_pool_hw_fwd' + sfx, xd, Ad, Bd, act, t('out'), NC, T, H, W, OH, OW)
    lib().call('cfn_pool_hw_bwd' + sfx, gd, xd, Ad, Bd, act, t('gx'), t('gA'), t('gB'), NC, T, H, W, OH, OW)
    torch.cuda.synchronize()
    guards_ok(('pool', kind, T, H, W, OH, OW, pro, act), outs)
    worst = {'out': E.ratio(t('out').view(ref['out'].val.shape), ref['out']),
             'gx': E.ratio_x(t('gx').float().view(ref['gx'].val.shape), ref['gx'], ref['gx_extra'])}
    if pro:
        worst.update({k: E.ratio(t(k), ref[k]) for k in ('gA', 'gB')})
    return worst


def _merge(into, w):
    for k, v in w.items():
        into[k] = max(into.get(k, 0.0), v)


@pytest.mark.parametrize('T', E.POOL_T)
@pytest.mark.parametrize('H,W,OH,OW', E.POOL_GENERAL)
@pytest.mark.parametrize('kind', KINDS)
def test_pool_hw_fp64(kind, H, W, OH, OW, T, record_property):
    """non-square planes and outputs, OH > H (windows of one pixel that repeat), overlapping windows (16 -> 7, 8 -> 7), the global mean of
    planes too large for the wave kernel (5 x 13 = 65, 14 x 14) and, for the 16-bit kinds (which have the general kernel only), the global
    mean of every plane; T = 6 with a 7 x 7 output: two workgroups, the second ragged.  With and without the A / B prologue, act none,
    ReLU, Swish.  out: n = the window; gx: n = the windows containing the pixel (16-bit: plus half a storage ulp); gA, gB"""
    worst = {}
    for pro in (True, False):
        for act in (0, 1, 2):
            w = pool_run(kind, T, H, W, OH, OW, pro, act)
            for k, val in w.items():
                assert val <= 1.0, ('%.3g x the bound' % val, k, kind, T, H, W, OH, OW, pro, act)
            _merge(worst, {'%s-act%d' % (k, act): val for k, val in w.items()})
    report(record_property, ('pool_hw', kind, T, H, W, OH, OW), worst)


@pytest.mark.parametrize('T', E.POOL1_T)
@pytest.mark.parametrize('H,W', E.POOL1_PLANES)
def test_pool_hw_global_mean_wave_kernel_fp64(H, W, T, record_property):
    """pool_hw1 (fp32, OH = OW = 1, H W <= 64): planes of 1, 49, 63 and 64 (a full wave) elements; T = 1, 8 (one frame group), 9, 33 (a
    second workgroup), 520 and 1030 (the grid is capped at 16 workgroups x 32 frames: the grid-stride loop repeats, once and twice, the last
    sweep ragged).  The backward walks a whole (n, c) row with one workgroup: n = ceil(T H W / 256) + 8 for gA, gB"""
    worst = {}
    for pro, act in ((True, 2), (False, 0), (True, 1), (False, 3)):
        w = pool_run('f32', T, H, W, 1, 1, pro, act)
        for k, val in w.items():
            assert val <= 1.0, ('%.3g x the bound' % val, k, T, H, W, pro, act)
        _merge(worst, {'%s-act%d' % (k, act): val for k, val in w.items()})
    report(record_property, ('pool_hw1', T, H, W), worst)


# ---- film -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', E.FILM_T)
@pytest.mark.parametrize('H,W,f', E.FILM_CASES)
def test_film_fp64(H, W, f, T, record_property):
    """f = 1, 2, 4, 8, non-square planes both ways, one ragged and several workgroups of pixels and of cells (294 and 588 cells at T = 6)"""
    x, m, c, g = E.film_inputs(T, H, W, f)
    ref = E.film_reference(T, H, W, f)
    NC = E.FILM_NC
    xd, md, cd, gd = put(x), put(m), put(c), put(g)
    outs = {'out': Guarded(x.numel(), torch.float32), 'gx': Guarded(x.numel(), torch.float32), 'gm': Guarded(m.numel(), torch.float32),
            'gc': Guarded(m.numel(), torch.float32)}
    lib().call('cfn_film_fwd', xd, md, cd, outs['out'].t, NC, T, H, W, f)
    lib().call('cfn_film_bwd', gd, xd, md, outs['gx'].t, outs['gm'].t, outs['gc'].t, NC, T, H, W, f)
    torch.cuda.synchronize()
    guards_ok(('film', T, H, W, f), outs)
    report(record_property, ('film', T, H, W, f), {k: E.ratio(outs[k].t.view(ref[k].val.shape), ref[k]) for k in outs})
