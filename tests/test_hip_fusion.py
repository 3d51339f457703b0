"""The Multi-stage Fusion kernels of csrc/fusion.hip -- gauss_align (fwd, bwd) and fusion_gather (fwd tiled <4,13|9|8> and one-output, bwd_x,
bwd_w tiled <8,8> and one-output, bwd_reduce) -- against the fp64 references of tests/fusion_ref64.py (pinned to autograd of the oracle's
expressions, and their bounds shown to discriminate, by tests/test_fusion_ref64_cpu.py), through cfn_hip.ops and, for den and the scratch
tensor dw, through the C ABI.  The shapes and what each one reaches are listed next to their inputs in fusion_ref64.py.

Bounds.  fusion_gather: elementwise, derived by counting the kernels' roundings (the docstring of fusion_ref64.py); an element whose bound
is zero (a masked frame, a fully masked video) must be an exact zero.  gauss_align GX: elementwise (expf argument, rounding of mu, an
underflow allowance).  gauss_align ggx and the chained case: measured, kernel error <= 4 x the error of the same expression in plain fp32
torch on the CPU + 2^-23, both relative to the tensor's max.  The worst err / bound of every case goes to the junit report (fusion_fp64).

Largest err / bound seen on an MI355X, per kernel and output (1.0 is the bound): fusion_gather z 0.39, den 0.32, dw 0.24, gx 0.30, gat 0.22,
gGX 0.07, gb 0.002; gauss_align GX 0.65 (the 260-thread case; 0.07 .. 0.45 elsewhere).  Measured rules, kernel error / fp32 CPU
expression's error, max-normalised: gauss_align ggx 6.6e-7 / 6.4e-7 (ratio 256 / 12), 2.7e-7 / 1.9e-7 (ratio 0.5), 2.8e-7 / 2.3e-7
(crops = 3), 2.6e-7 / 4.2e-7 (ratio 1.6), 4.9e-7 / 7.6e-7 (mu outside the window), 8.9e-8 / 1.2e-7 (ties), 1.1e-7 / 1.4e-7 (a fully
masked video), 0 / 0 (every f underflows); the chain z 3.3e-7 / 3.3e-7, gcdf 5.9e-7 / 1.0e-6, gx 1.4e-7 / 1.5e-7, gat 3.0e-7 / 2.3e-7.

The three bit-equalities.  Knot slices and crop rows held as found.  Position slices did not: z and den of the one-output forward kernel
(P > 256) differed from the tiled kernel's in the last bit, because the compiler folded its `d += w` into fma(a, GX * mask, d) while the
tiled kernel adds the rounded w; the one-output kernel now forbids the contraction and the claim holds (both sides were inside the fp64
bound before and after).

The checks were also run once against a kernel build with four deliberate errors: the ragged last k tile of the tiled dw kernel skipped
(dw unwritten, gat at 5e24 x the bound), crop 0's GX for every crop in the tiled forward kernel (z at 3e22 x the bound or not finite in
the crops = 2 cases), z added instead of subtracted in the one-output dw kernel (dw at 1e6 x the bound at P = 260, the position slices no
longer bit-equal), the gauss_align gradient to the last maximal frame (the tie case: 1.3 of the tensor's max against an allowance of
6e-7).  Every one was caught."""
import pytest
import torch

import fusion_ref64 as Fr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U23 = 2.0 ** -23
NAN = float('nan')


def ops():
    from cfn_hip import ops as o
    return o


def dv(v, grad=False):
    return None if v is None else v.clone().to(DEV).requires_grad_(grad)


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def check(record, tag, got, ref, keys):
    """every output in keys within its elementwise bound; the worst err / bound per output goes to the junit report"""
    worst = {k: Fr.worst(got[k], ref[k]) for k in keys}
    if record is not None:
        record('fusion_fp64', repr(dict(case=tag, worst=worst)))
    for k in keys:
        assert got[k].dtype == torch.float32, (tag, k, got[k].dtype)
        assert worst[k] <= 1.0, (tag, k, worst[k])
    return worst


# ---- fusion_gather ------------------------------------------------------------------------------------------------------------------------
GRAD_KEYS = {'x': 'gx', 'at': 'gat', 'b': 'gb', 'GX': 'gGX'}


def fg_run(inp, need=('x', 'at', 'b', 'GX')):
    """through cfn_hip.ops, asking for the gradients in `need` -> {'z', and the gradients asked for}"""
    need = tuple(n for n in need if not (n == 'b' and inp['bias'] is None))
    leaves = {'x': dv(inp['x'], 'x' in need), 'at': dv(inp['at_raw'], 'at' in need), 'b': dv(inp['bias'], 'b' in need),
              'GX': dv(inp['GX'], 'GX' in need)}
    z = ops().fusion_gather(leaves['x'], leaves['at'], leaves['b'], leaves['GX'], dv(inp['mask']), inp['crops'])
    grads = torch.autograd.grad(z, [leaves[n] for n in need], dv(inp['gz']))
    got = {'z': z.detach()}
    got.update({GRAD_KEYS[n]: g for n, g in zip(need, grads)})
    torch.cuda.synchronize()
    return got


def fg_abi(inp, want=('gx', 'gat', 'gGX')):
    """cfn_fusion_gather_fwd and _bwd through the C ABI, every output prefilled with NaN -> {'z', 'den', 'dw', and the outputs in want}"""
    import cfn_hip
    x, at_raw, bias, GX, mask, gz = (dv(inp[k]) for k in ('x', 'at_raw', 'bias', 'GX', 'mask', 'gz'))
    crops = inp['crops']
    B, C, Tf, P = x.shape
    R, K = GX.shape[0], GX.shape[2]
    z, den, dw = nans(R, C, K, P), nans(R, K, P), nans(R, Tf, K, P)
    out = {'gx': nans(*x.shape) if 'gx' in want else None, 'gat': nans(*at_raw.shape) if 'gat' in want else None,
           'gGX': nans(*GX.shape) if 'gGX' in want else None}
    cfn_hip.call('cfn_fusion_gather_fwd', x, at_raw, bias, GX, mask, z, den, B, crops, C, Tf, K, P)
    cfn_hip.call('cfn_fusion_gather_bwd', gz, z, den, x, at_raw, bias, GX, mask, out['gx'], out['gat'], out['gGX'], dw, B, crops, C, Tf, K, P)
    torch.cuda.synchronize()
    got = {'z': z, 'den': den, 'dw': dw}
    got.update({k: v for k, v in out.items() if v is not None})
    return got


@pytest.mark.parametrize('shape,regime', Fr.FG_CASES)
def test_fusion_gather_fp64(shape, regime, record_property):
    """every shape of fusion_ref64.FG_SHAPES with mixed-sign x, logits of scale 3 and the oracle's GX (knots far outside the window: den ~
    1e-6, gz / den = 1e6 gz), the 49-position shapes also behind a fully masked video, with a tenth of the logits at +-100, with
    at_bias = None and with another bias.  z and the four gradients through cfn_hip.ops, den and dw through the C ABI, each element
    within its bound; a masked frame and everything of a fully masked video is an exact zero (their bound is 0), its den exactly
    fp32(1e-6); a saturated logit's gat is an exact zero"""
    inp, ref = Fr.fg_inputs(shape, regime), Fr.fg_reference(shape, regime)
    crops = inp['crops']
    got = fg_run(inp)
    abi = fg_abi(inp, want=('gat',))
    got.update(den=abi['den'], dw=abi['dw'])
    keys = [k for k in Fr.FG_KEYS if ref[k] is not None]
    assert set(keys) == set(got)
    check(record_property, (shape, regime), got, ref, keys)
    assert torch.equal(abi['z'], got['z']) and torch.equal(abi['gat'], got['gat'])          # the C ABI run is the run ops made
    if regime == 'masked':
        assert bool((got['z'][:crops] == 0).all()) and bool((got['den'][:crops] == torch.tensor(1e-6, dtype=torch.float32)).all())
        assert bool((got['gx'][0] == 0).all()) and bool((got['gat'][0] == 0).all()) and bool((got['gGX'][:crops] == 0).all())
    if regime == 'sat':
        sat = inp['at_raw'].abs() == 100
        assert bool((got['gat'].cpu()[sat] == 0).all())


SUBSETS = [('x',), ('at',), ('b',), ('GX',), ('x', 'GX'), ('at', 'b')]


@pytest.mark.parametrize('shape', [(2, 1, 5, 7, 5, 49), (1, 2, 3, 5, 4, 260)])
def test_fusion_gather_gradient_subsets(shape, record_property):
    """x only, at_raw only, the bias only (gat is computed but not returned), GX only and two pairs (gx / gat / gGX null in
    cfn_fusion_gather_bwd as needs_input_grad says): the same bounds, and bit-equal to the run that asks for all four (no atomics)"""
    inp, ref = Fr.fg_inputs(shape, 'oracle'), Fr.fg_reference(shape, 'oracle')
    every = fg_run(inp)
    for need in SUBSETS:
        got = fg_run(inp, need)
        assert set(got) == {'z'} | {GRAD_KEYS[n] for n in need}, need
        check(record_property, (shape, need), got, ref, tuple(got))
        for k in got:
            assert torch.equal(got[k], every[k]), (need, k)


@pytest.mark.parametrize('shape,regime', [((2, 1, 5, 7, 5, 49), 'masked'), ((1, 2, 24, 9, 17, 49), 'oracle'), ((1, 2, 3, 5, 4, 260), 'oracle'),
                                          ((3, 2, 9, 4, 3, 1), 'oracle')])
def test_fusion_gather_abi_writes_every_element(shape, regime, record_property):
    """cfn_fusion_gather_fwd / _bwd through the C ABI with z, den, gx, gat, gGX and dw prefilled with NaN (ops hands them torch.empty):
    nothing is left unwritten, masked frames come back as exact zeros, dw is within its own bound; then with each output null in turn"""
    inp, ref = Fr.fg_inputs(shape, regime), Fr.fg_reference(shape, regime)
    every = fg_abi(inp)
    check(record_property, (shape, regime, 'abi'), every, ref, ('z', 'den', 'dw', 'gx', 'gat', 'gGX'))
    for drop in ('gx', 'gat', 'gGX'):
        want = tuple(k for k in ('gx', 'gat', 'gGX') if k != drop)
        got = fg_abi(inp, want)
        assert set(got) == {'z', 'den', 'dw'} | set(want)
        check(None, (shape, regime, 'abi without ' + drop), got, ref, tuple(got))
        for k in got:
            assert torch.equal(got[k], every[k]), (drop, k)


def test_fusion_gather_position_slices_are_bit_equal(record_property):
    """each output element but gGX depends on ONE position p: the first 49 positions of the P = 260 case (the one-output kernels) run
    alone at P = 49 (the tiled kernels) give the same bits in z, den, gx, gat and dw -- the kernel comments' `bit-identical` claim"""
    big = Fr.fg_inputs((1, 2, 3, 5, 4, 260), 'oracle')
    a, b = fg_abi(big), fg_abi(Fr.fg_slice(big, P=49))
    for k in ('z', 'den', 'dw', 'gx', 'gat'):
        assert torch.equal(a[k][..., :49], b[k]), (k, float((a[k][..., :49] - b[k]).abs().max()))


def test_fusion_gather_knot_slices_are_bit_equal():
    """z, den and dw of a knot depend on that knot's GX column alone: the first 5 knots of the K = 65 case (<4,13>) run alone at K = 5
    (<4,8>) give the same bits"""
    big = Fr.fg_inputs((1, 1, 4, 3, 65, 49), 'oracle')
    a, b = fg_abi(big), fg_abi(Fr.fg_slice(big, K=5))
    assert torch.equal(a['z'][:, :, :5], b['z']) and torch.equal(a['den'][:, :5], b['den']) and torch.equal(a['dw'][:, :, :5], b['dw'])


def test_fusion_gather_crop_rows_are_bit_equal():
    """row r = b * crops + j reads video b and GX row r: the crops = 2 run equals two crops = 1 runs with the respective GX rows in z, den,
    dw and gGX (gx and gat sum over the crops)"""
    big = Fr.fg_inputs((1, 2, 24, 9, 17, 49), 'oracle')
    a = fg_abi(big)
    for j in range(2):
        b = fg_abi(Fr.fg_slice(big, crop=j))
        for k in ('z', 'den', 'dw', 'gGX'):
            assert torch.equal(a[k][j::2], b[k]), (j, k)


# ---- gauss_align --------------------------------------------------------------------------------------------------------------------------
def ga_run(inp):
    gx = dv(inp['gx'], True)
    out = ops().gauss_align(dv(inp['meta']), dv(inp['mask']), gx, inp['tx'], inp['ratio'], inp['crops'], inp['K'])
    got = {'GX': out.detach(), 'ggx': None}
    if gx is not None:
        (got['ggx'],) = torch.autograd.grad(out, [gx], dv(inp['gGX']))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize('name', sorted(Fr.GA_CASES))
def test_gauss_align_fp64(name, record_property):
    """the cases of fusion_ref64.GA_CASES: ratio = 256 / 12, 1.6, 0.5, 16 / 7, 3.2; a second, ragged workgroup; a fully masked video
    (std = 0); gx = None at ratio 1 and 2; exact half-integer mu (two bit-equal ones per column, the gradient to the first); mu outside
    the window on both sides; every f underflowing (GX and ggx exact zeros); crops = 3 with a step of 2 and 3.  GX elementwise within
    its bound; ggx within 4 x the fp32 CPU expression's error + 2^-23 of the fp64 reference, relative to the max, and exactly zero for
    the knots whose gGX column is zero"""
    inp, ref, base = Fr.ga_inputs(name), Fr.ga_reference(name), Fr.ga_baseline(name)
    got = ga_run(inp)
    assert got['GX'].dtype == torch.float32 and bool(torch.isfinite(got['GX']).all())
    w = Fr.worst(got['GX'], ref['GX'])
    errs = None
    if ref['ggx'] is not None:
        assert got['ggx'].dtype == torch.float32 and tuple(got['ggx'].shape) == tuple(ref['ggx'].shape) and bool(torch.isfinite(got['ggx']).all())
        errs = (Fr.maxrel(got['ggx'], ref['ggx']), Fr.maxrel(base['ggx'], ref['ggx']))
    record_property('fusion_fp64', repr(dict(case=('gauss_align', name), worst={'GX': w}, ggx_kernel_vs_cpu=errs)))
    assert w <= 1.0, w
    if name == 'tie':
        fr = ref['mu'] - torch.floor(ref['mu'])
        assert torch.equal((got['GX'].cpu() == 1.0).sum(1) == 2, fr == 0.5)
    if name == 'underflow':
        assert bool((got['GX'] == 0).all()) and bool((got['ggx'] == 0).all())
    if errs is not None:
        assert bool((got['ggx'][:, ::4] == 0).all())
        assert errs[0] <= 4.0 * errs[1] + U23, errs
    else:
        assert inp['gx'] is None


def test_gauss_align_without_a_cdf_gradient(monkeypatch):
    """gx does not require a gradient (the mask does, so that backward runs): None comes back and cfn_gauss_align_bwd is not launched"""
    o = ops()
    launched = []
    real = o.call
    monkeypatch.setattr(o, 'call', lambda name, *a: (launched.append(name), real(name, *a))[1])
    inp = Fr.ga_inputs('t64')
    mask = dv(inp['mask'], True)
    out = o.gauss_align(dv(inp['meta']), mask, dv(inp['gx']), inp['tx'], inp['ratio'], inp['crops'], inp['K'])
    assert out.requires_grad
    (gm,) = torch.autograd.grad(out, [mask], dv(inp['gGX']), allow_unused=True)
    torch.cuda.synchronize()
    assert gm is None and launched == ['cfn_gauss_align_fwd']
    assert Fr.worst(out.detach(), Fr.ga_reference('t64')['GX']) <= 1.0


def test_gauss_align_into_fusion_gather(record_property):
    """gauss_align into fusion_gather at (B, crops, C, Tf, K, P) = (2, 2, 6, 10, 9, 49), the gradient flowing back to the CDF: z, gcdf, gx
    and gat against the chained fp64 reference, each within 4 x the fp32 CPU chain's error + 2^-23, relative to the max (the kernel's GX
    carries its own rounding into the gather, so the elementwise bounds of the two kernels do not apply to the chain)"""
    c = Fr.chain_inputs()
    ref, base = Fr.chain_reference(), Fr.chain_reference(torch.float32)
    cdf, x, at_raw = dv(c['gx'], True), dv(c['x'], True), dv(c['at_raw'], True)
    mask = dv(c['mask'])
    GX = ops().gauss_align(dv(c['meta']), mask, cdf, c['tx'], c['ratio'], c['crops'], c['K'])
    z = ops().fusion_gather(x, at_raw, dv(c['bias']), GX, mask, c['crops'])
    grads = torch.autograd.grad(z, [cdf, x, at_raw], dv(c['gz']))
    torch.cuda.synchronize()
    got = dict(zip(Fr.CHAIN_KEYS, (z.detach(),) + tuple(grads)))
    errs = {k: (Fr.maxrel(got[k], ref[k]), Fr.maxrel(base[k], ref[k])) for k in Fr.CHAIN_KEYS}
    record_property('fusion_fp64', repr(dict(case='chain', kernel_vs_cpu=errs)))
    for k, (e, b) in errs.items():
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == tuple(ref[k].shape) and bool(torch.isfinite(got[k]).all()), k
        assert e <= 4.0 * b + U23, (k, e, b)
