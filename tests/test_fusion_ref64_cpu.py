"""tests/fusion_ref64.py (the fp64 references csrc/fusion.hip is checked against by tests/test_hip_fusion.py) pinned to autograd of the
oracle's expressions in float64, and its bounds shown to discriminate.  CPU only.

Pinning.  Both sides are fp64 and differ in summation order only: 1e-12 relative to each tensor's max.
    fusion_gather   autograd of the einsum form of x3d_coarse.py:209-223 (fusion_ref64.gather_expr, the expression of
                    tests/test_hip_fullsize_coarse.py) in float64; dw is its gradient with respect to the weights at * GX * mask
    gauss_align     autograd of oracle.x3d_ref.gaussian in float64.  The oracle hard-codes float32 for its start offsets and frame indices, so
                    it is restated with the dtype as a parameter (fusion_ref64.gaussian_expr) and shown bit-equal to the oracle on fp32
                    inputs; torch.max(dim) routes the gradient of a tie to the first maximal frame, which the tie case pins

Bounds are not too tight: the same expression in plain fp32 torch lies within the bound of every GPU case (for the measured ggx rule it is
its own yardstick).  Bounds are not too loose: every mutant of fusion_ref64.MUTANTS, applied to the fp64 reference, leaves the bound of every
case that names it.  The conditions the inputs are built for are asserted per case."""
import pytest
import torch

import fusion_ref64 as Fr
from oracle import x3d_ref as R

TOL = 1e-12
U23 = 2.0 ** -23


def _close(name, got, ref):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    err, top = float((got - ref).detach().abs().max()), float(ref.detach().abs().max())
    assert err <= TOL * top, (name, err, top)


# ---- pinning ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,regime', [((2, 1, 5, 7, 5, 49), 'oracle'), ((1, 2, 24, 9, 17, 49), 'bias'), ((1, 2, 24, 9, 17, 49), 'nobias'),
                                          ((3, 2, 9, 4, 3, 1), 'oracle'), ((1, 2, 3, 5, 4, 260), 'oracle'), ((2, 1, 5, 7, 5, 49), 'masked')])
def test_fusion_gather_ref64_matches_autograd(shape, regime):
    inp = Fr.fg_inputs(shape, regime)
    ref = Fr.fg_reference(shape, regime)
    leaf = lambda v: v.double().requires_grad_(True)
    x, at_raw, GX = leaf(inp['x']), leaf(inp['at_raw']), leaf(inp['GX'])
    bias = None if inp['bias'] is None else leaf(inp['bias'])
    z, wgt = Fr.gather_expr(x, at_raw, bias, GX, inp['mask'].double(), inp['crops'])
    wgt.retain_grad()
    (z * inp['gz'].double()).sum().backward()
    _close('z', ref['z'].val, z.detach())
    _close('den', ref['den'].val, (wgt.sum(1) + 1e-6).detach())
    _close('dw', ref['dw'].val, wgt.grad)
    _close('gx', ref['gx'].val, x.grad)
    _close('gat', ref['gat'].val, at_raw.grad)
    _close('gGX', ref['gGX'].val, GX.grad)
    if bias is None:
        assert ref['gb'] is None
    else:
        # gb nearly cancels: pinned against sum |gat|, as its bound is
        assert float((ref['gb'].val - bias.grad).abs()) <= TOL * float(at_raw.grad.abs().sum())


@pytest.mark.parametrize('name', sorted(Fr.GA_CASES))
def test_gauss_align_ref64_matches_oracle_expression(name):
    inp = Fr.ga_inputs(name)
    ref = Fr.ga_reference(name)
    meta, mask, gx, tx, rt, crops, K = (inp[k] for k in ('meta', 'mask', 'gx', 'tx', 'ratio', 'crops', 'K'))
    Rr = mask.shape[0] * crops
    if gx is None:
        dummy = torch.zeros(Rr, 1, K)
        assert torch.equal(Fr.gaussian_expr(meta, mask, dummy, None, rt), R.gaussian(meta, mask, dummy, None, rt)), 'not the oracle'
        _close('GX', ref['GX'].val, Fr.gaussian_expr(meta, mask.double(), dummy.double(), None, rt, dtype=torch.float64))
        assert ref['ggx'] is None
        return
    assert torch.equal(Fr.gaussian_expr(meta, mask, gx, tx, rt), R.gaussian(meta, mask, gx, tx, rt)), 'the restated expression is not the oracle'
    cdf = gx.double().requires_grad_(True)
    GX = Fr.gaussian_expr(meta, mask.double(), cdf, tx, rt, dtype=torch.float64)
    (ggx,) = torch.autograd.grad((GX * inp['gGX'].double()).sum(), [cdf])
    _close('GX', ref['GX'].val, GX.detach())
    if float(ggx.abs().max()) > 0:
        _close('ggx', ref['ggx'], ggx)
    else:
        assert bool((ref['ggx'] == 0).all())


def test_chain_reference_is_the_composition_of_the_two_references():
    """the chained fp64 reference (autograd through both restated expressions) against the two closed forms applied one after the other"""
    c = Fr.chain_inputs()
    ch = Fr.chain_reference()
    g = Fr.ga_ref_of(dict(c, gGX=None))
    GX64 = g['GX'].val
    leafless = Fr.fusion_gather_ref64(c['x'], c['at_raw'], c['bias'], GX64, c['mask'], c['gz'], c['crops'])
    _close('z', leafless['z'].val, ch['z'])
    _close('gx', leafless['gx'].val, ch['gx'])
    _close('gat', leafless['gat'].val, ch['gat'])
    back = Fr.gauss_align_ref64(c['meta'], c['mask'], c['gx'], c['tx'], c['ratio'], c['crops'], c['K'], leafless['gGX'].val)
    _close('gcdf', back['ggx'], ch['gcdf'])


# ---- the bounds: plain fp32 inside, every mutant outside; the conditions the inputs were built for -------------------------------------------
@pytest.mark.parametrize('shape,regime', Fr.FG_CASES)
def test_fusion_gather_bounds(shape, regime):
    B, crops, C, Tf, K, P = shape
    inp = Fr.fg_inputs(shape, regime)
    ref = Fr.fg_reference(shape, regime)
    assert Fr.fwd_ktile(K) == Fr.FG_KTILE[K]
    keys = [k for k in Fr.FG_KEYS if ref[k] is not None]
    assert ('gb' in keys) == (regime != 'nobias')
    for k in keys:
        assert bool(torch.isfinite(ref[k].val).all()) and bool(torch.isfinite(ref[k].bnd).all()) and bool((ref[k].bnd >= 0).all()), k
    # an outside knot: the whole GX column underflows against the normalisation's 1e-16 and den is the 1e-6 of the formula
    assert float(ref['den'].val.min()) < 2e-6, float(ref['den'].val.min())
    # cancellation is present: A / den = sum |x| w / den >= 4 |z| on a tenth of the elements (measured: 0.12 .. 0.67)
    live = inp['mask'].sum(1).repeat_interleave(crops) > 0
    Aq = ref['z'].bnd[live] / ((2 * Tf + Fr.SLACK) * Fr.U24)            # the FL term of the bound is ~1e-38 of it
    frac = float((Aq >= 4 * ref['z'].val[live].abs()).double().mean())
    assert frac >= 0.10, frac
    if regime == 'masked':
        dead = inp['mask'].sum(1) == 0
        assert bool(dead[0]) and not bool(dead[1:].any())
        assert bool((ref['z'].val[:crops] == 0).all()) and bool((ref['z'].bnd[:crops] == 0).all())
        assert bool((ref['den'].val[:crops] == 1e-6).all())
        for k in ('gx', 'gat', 'gGX'):
            zero = (ref[k].val == 0) & (ref[k].bnd == 0)
            assert float(zero.double().mean()) >= 0.25, (k, float(zero.double().mean()))
            assert bool(zero[:crops if k == 'gGX' else 1].all()), k
    if regime == 'sat':
        assert bool((inp['at_raw'] == 100).any()) and bool((inp['at_raw'] == -100).any())
    f32 = Fr.fg_ref_of(inp, dtype=torch.float32)
    for k in keys:
        r = Fr.worst(f32[k].val, ref[k])
        assert r <= 1.0, ('plain fp32 torch is outside the bound', k, r)
    for m in Fr.fg_mutants(shape, regime):
        mut = Fr.fg_ref_of(inp, mutant=m)
        w = max(Fr.worst(mut[k].val, ref[k]) for k in keys)
        assert w > 1.0, ('mutant within the bound: the inputs of this case do not discriminate', m, w)


def test_fusion_gather_every_mutant_is_named():
    assert set(m for s, r in Fr.FG_CASES for m in Fr.fg_mutants(s, r)) == set(Fr.MUTANTS['fusion_gather'])
    assert set(s for s, _ in Fr.FG_CASES) == set(Fr.FG_SHAPES)


def _ggx_errs(name, got):
    ref = Fr.ga_reference(name)
    return Fr.maxrel(got, ref['ggx'])


@pytest.mark.parametrize('name', sorted(Fr.GA_CASES))
def test_gauss_align_bounds(name):
    inp = Fr.ga_inputs(name)
    ref, base = Fr.ga_reference(name), Fr.ga_baseline(name)
    B, crops, Tf, K, tx, rt = Fr.GA_CASES[name]
    assert Fr.ga_margin_ok(ref['mu']), 'an argmax frame of this case depends on the precision'
    assert torch.equal(ref['tm'], base['tm'])
    assert bool(torch.isfinite(ref['GX'].val).all()) and bool(torch.isfinite(ref['GX'].bnd).all())
    fr = ref['mu'] - torch.floor(ref['mu'])
    if name == 'tie':
        assert ref['tm'].tolist() == Fr.GA_TIE_TM and float((fr == 0.5).double().mean()) >= 0.5
        two = (ref['GX'].val == ref['GX'].val.max(1, keepdim=True)[0]).sum(1)          # bit-equal maxima per column: two at a tie
        assert torch.equal(two == 2, fr == 0.5) and torch.equal((base['GX'].val == 1.0).sum(1) == 2, fr == 0.5)
    if name == 'knots2':
        assert bool((fr == 0.5).any())
    if name == 'edges':
        assert ref['tm'].tolist() == Fr.GA_EDGES_TM
    if name == 'underflow':
        assert bool((ref['GX'].val == 0).all()) and bool((ref['ggx'] == 0).all()) and bool((base['GX'].val == 0).all())
    if name == 'masked':
        assert float(inp['mask'][1].sum()) == 0 and bool(torch.isfinite(ref['ggx']).all())
    if name == 'wg2':
        assert B * crops * K > 256
    if name == 'step':
        assert inp['meta'][:, 3].tolist() == [2, 3]
    r = Fr.worst(base['GX'].val, ref['GX'])
    assert r <= 1.0, ('plain fp32 torch is outside the GX bound', r)
    if ref['ggx'] is not None:
        assert bool((ref['ggx'][:, ::4] == 0).all()), 'a knot whose gGX column is zero has a gradient'
        e_base = Fr.maxrel(base['ggx'], ref['ggx'])
        assert e_base < 1e-4, e_base                      # the yardstick itself is an fp32 error, not a disagreement
    for m in Fr.GA_MUTANTS.get(name, ()):
        mut = Fr.ga_ref_of(inp, mutant=m)
        w = Fr.worst(mut['GX'].val, ref['GX'])
        if ref['ggx'] is not None:
            e = Fr.maxrel(mut['ggx'], ref['ggx'])
            w = max(w, e / (4.0 * e_base + U23))
        assert w > 1.0, ('mutant within the bound: the inputs of this case do not discriminate', m, w)


def test_gauss_align_every_mutant_is_named():
    assert set(m for v in Fr.GA_MUTANTS.values() for m in v) == set(Fr.MUTANTS['gauss_align'])
    assert set(Fr.GA_MUTANTS) <= set(Fr.GA_CASES)


def test_chain_baseline_is_an_fp32_error():
    """the fp32 CPU chain (the yardstick of the chained GPU case) is close to the fp64 chain, and a chain whose Gaussian ignores the crop
    offset is not"""
    ref, base = Fr.chain_reference(), Fr.chain_reference(torch.float32)
    for k in Fr.CHAIN_KEYS:
        e = Fr.maxrel(base[k], ref[k])
        assert e < 1e-4, (k, e)
    c = Fr.chain_inputs()
    g = Fr.ga_ref_of(dict(c, gGX=None), mutant='crop0_start')
    mut = Fr.fusion_gather_ref64(c['x'], c['at_raw'], c['bias'], g['GX'].val, c['mask'], c['gz'], c['crops'])
    for k in ('z', 'gx', 'gat'):
        assert Fr.maxrel(mut[k].val, ref[k]) > 4.0 * Fr.maxrel(base[k], ref[k]) + U23, k
