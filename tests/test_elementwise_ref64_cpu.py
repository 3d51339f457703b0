"""tests/elementwise_ref64.py (the fp64 references csrc/elementwise.hip and csrc/streambf16.hip are checked against by
tests/test_hip_elementwise.py) pinned to stock torch in float64, and its elementwise bounds shown to discriminate.  CPU only.

Pinning: fp64 autograd of the plain expression -- F.relu(A y + B + Ar res + Br), act(A x + B) with z sigmoid(z) for Swish,
F.adaptive_avg_pool3d of it, x repeat_interleave(m) + repeat_interleave(c) -- agrees with every reference to 1e-12 of the tensor's max.
Bounds are not too tight: the same expression in plain fp32 torch lies within the bound of every GPU case.
Bounds are not too loose: each mutant of elementwise_ref64.MUTANTS, applied to the fp64 reference, leaves the bound of every case that
names it.  No case holds an ambiguous ReLU decision (0 < |z| <= bound), and the planted exact zeros are zeros of the reference."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref64 as E

TOL = 1e-12
KINDS = ('f32', 'bf16', 'f16')
TAIL_ALL = [(k, n) for k in KINDS for n in E.TAIL_CASES[k]]
POOL_ALL = [(k, T, c) for k in KINDS for T in E.POOL_T for c in E.POOL_GENERAL]
POOL_OPTS = [(pro, act) for pro in (True, False) for act in (0, 1, 2)]
POOL1_OPTS = [(True, 2), (False, 0), (True, 1), (False, 3)]


def _close(name, got, ref):
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    err, top = float((got - ref).detach().abs().max()), float(ref.detach().abs().max())
    assert err <= TOL * top, (name, err, top)


def _act(z, act):
    return (z, F.relu(z), z * torch.sigmoid(z), torch.sigmoid(z))[act]


# ---- pinning --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,name', [(k, n) for k, n in TAIL_ALL if k != 'f16'])
def test_tail_ref64_matches_autograd(kind, name):
    y, res, A, B, Ar, Br, gout, gout2 = E.tail_args(kind, name)
    ref = E.tail_ref64(y, res, A, B, Ar, Br, gout, gout2, 8)
    lv = {k: v.double().clone().requires_grad_(True) for k, v in dict(y=y, res=res, A=A, B=B, Ar=Ar, Br=Br).items() if v is not None}
    col = lambda k: lv[k].view(-1, 1)
    r = lv['res'] * col('Ar') + col('Br') if Ar is not None else lv['res']
    out = F.relu(lv['y'] * col('A') + col('B') + r)
    gt = gout.double() + (gout2.double() if gout2 is not None else 0.0)
    out.backward(gt)
    _close('out', ref['out'].val, out.detach())
    for k, leaf in (('gy', 'y'), ('gres', 'res'), ('gA', 'A'), ('gB', 'B'), ('gAr', 'Ar')):
        if leaf in lv:
            _close(k, ref[k].val, lv[leaf].grad)
    if Ar is not None:
        _close('gBr', ref['gB'].val, lv['Br'].grad)
    _close('g', ref['g'].val, gt * (out.detach() > 0))


@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('vol', E.AFF_VOLS)
def test_affine_ref64_matches_autograd(vol, act):
    x, A, B, g = E.aff_inputs(vol, act)
    ref = E.aff_reference(vol, act)
    xl, Al, Bl = (v.double().clone().requires_grad_(True) for v in (x, A, B))
    out = _act(xl * Al.view(-1, 1) + Bl.view(-1, 1), act)
    out.backward(g.double())
    for k, v in (('out', out.detach()), ('gx', xl.grad), ('gA', Al.grad), ('gB', Bl.grad), ('sum', x.double().sum(1)),
                 ('sumsq', (x.double() ** 2).sum(1))):
        _close(k, ref[k].val, v)
    assert float(ref['out'].val.abs().max()) > 8 or act == 3        # z reaches the range where the |z| term of the bound matters


def _pool_autograd(x, A, B, act, OH, OW, g):
    NC, T = x.shape[:2]
    xl = x.double().requires_grad_(True)
    Al = (A if A is not None else torch.ones(NC, dtype=torch.float64)).clone().requires_grad_(True)
    Bl = (B if B is not None else torch.zeros(NC, dtype=torch.float64)).clone().requires_grad_(True)
    v = _act(xl * Al.view(NC, 1, 1, 1) + Bl.view(NC, 1, 1, 1), act)
    out = F.adaptive_avg_pool3d(v.unsqueeze(0), (T, OH, OW))[0]
    out.backward(g.double())
    return out.detach(), xl.grad, Al.grad, Bl.grad


@pytest.mark.parametrize('T,case', [(T, c) for T in E.POOL_T for c in E.POOL_GENERAL])
def test_pool_ref64_matches_adaptive_avg_pool3d(T, case):
    for pro, act in POOL_OPTS + [(True, 3)]:
        x, A, B, g = E.pool_inputs('f32', T, *case, pro, act)
        ref = E.pool_ref64(x, A, B, act, case[2], case[3], g, 1)
        out, gx, gA, gB = _pool_autograd(x, A, B, act, case[2], case[3], g)
        _close('out', ref['out'].val, out)
        _close('gx', ref['gx'].val, gx)
        if pro:
            _close('gA', ref['gA'].val, gA)
            _close('gB', ref['gB'].val, gB)


@pytest.mark.parametrize('T', E.FILM_T)
@pytest.mark.parametrize('H,W,f', E.FILM_CASES)
def test_film_ref64_matches_autograd(H, W, f, T):
    x, m, c, g = E.film_inputs(T, H, W, f)
    ref = E.film_reference(T, H, W, f)
    xl, ml, cl = (v.double().requires_grad_(True) for v in (x, m, c))
    up = lambda t: t.repeat_interleave(f, 2).repeat_interleave(f, 3)
    out = xl * up(ml) + up(cl)
    out.backward(g.double())
    for k, v in zip(E.FILM_KEYS, (out.detach(), xl.grad, ml.grad, cl.grad)):
        _close(k, ref[k].val, v)


# ---- the mask layout, the planted zeros, the fp16 rounding case ---------------------------------------------------------------------------------
@pytest.mark.parametrize('per,vol', [(4, 1028), (4, 16388), (8, 2056), (8, 8200)])
def test_mask_words_layout(per, vol):
    """bit per*k + e of word (nc nchunks + chunk) 256 + tid, restated element by element"""
    NC = 2
    pos = torch.rand(NC, vol, generator=torch.Generator().manual_seed(vol)) > 0.5
    words = E.mask_words(pos, per)
    nch = -(-vol // E.WG)
    assert words.numel() == NC * nch * 256
    want = [0] * (NC * nch * 256)
    for nc in range(NC):
        for i in torch.nonzero(pos[nc]).view(-1).tolist():
            chunk, rem = divmod(i, E.WG)
            k, rem = divmod(rem, 256 * per)
            tid, e = divmod(rem, per)
            want[(nc * nch + chunk) * 256 + tid] |= 1 << (per * k + e)
    assert words.tolist() == want


@pytest.mark.parametrize('kind,name', TAIL_ALL)
def test_tail_planted_zeros_and_scales(kind, name):
    v, ref = E.tail_inputs(kind, name), E.tail_reference(kind, name)
    p = v['y'].shape[0] - 1
    for i in E.PLANT:
        assert float(ref['z'][p, i]) == 0.0 and float(ref['out'].val[p, i]) == 0.0 and float(ref['g'].val[p, i]) == 0.0
        assert not bool(ref['pos'][p, i]) and float(v['gout'][p, i]) != 0.0
        z32 = v['y'][p, i] * v['A'][p].float() + (v['res'][p, i] * 1.0 + 0.0)
        assert float(z32) == 0.0                                       # an exact zero in fp32 as well
    if v['y'].shape[0] >= 3:
        assert float(v['A'][0]) == 0.0 and float(v['A'][1]) < 0.0
    if kind != 'f32':
        for k in ('y', 'res', 'gout', 'gout2'):
            if v[k] is not None:
                assert torch.equal(v[k], v[k].to(E.STORE[kind]).float()) and torch.equal(v[k] * 64, torch.round(v[k] * 64))
    frac = float(ref['pos'].double().mean())
    assert 0.2 < frac < 0.8 or v['y'].numel() < 64


def test_f16_tiny_case_stores_as_documented():
    y, res, A, B, gout, stored_pos = E.f16_tiny_inputs()
    assert stored_pos.tolist() == [False, False, True]
    assert A.float().half().tolist() == [0.0, 0.0, 2.0 ** -24] and bool((A.float() > 0).all())


def test_flat_grid_totals():
    """the flat grid sizes cfn_xcd_remap is seen at: q = 0 (fewer than 8 workgroups), r != 0 and q > 0"""
    totals = {c.NC * -(-c.vol // E.WG) for n, c in E.TAIL_F32.items() if E.tail_route('f32', n)[0]}
    assert {1, 7, 8, 9, 15, 26} <= totals


# ---- the bounds: no ambiguity, the fp32 expression inside, every mutant outside ---------------------------------------------------------------
@pytest.mark.parametrize('kind,name', TAIL_ALL)
def test_tail_bounds(kind, name):
    args, ref = E.tail_args(kind, name), E.tail_reference(kind, name)
    vec, share, per = E.tail_route(kind, name)
    assert ref['amb'] == 0
    assert (ref['mask'] is not None) == vec
    f32 = E.tail_ref64(*args, share, per=per, store=E.STORE[kind], dtype=torch.float32)
    assert f32['amb'] == 0 and torch.equal(f32['pos'], ref['pos'])
    w = E.tail_worst(f32, ref)
    assert w <= 1.0, ('plain fp32 torch is outside the bound', kind, name, w)
    if kind != 'f32' or args[7] is None:                               # one gradient, or 16-bit storage: g is exact
        assert torch.equal(f32['g'].val, ref['g'].val)
    for m in E.tail_mutants(kind, name):
        w = E.tail_worst(E.tail_ref64(*args, share, per=per, store=E.STORE[kind], mutant=m), ref)
        assert w > 1.0, ('mutant within the bound: the inputs of this case do not discriminate', kind, name, m, w)


def test_tail_every_mutant_is_named():
    named = {m for k in KINDS for n in E.TAIL_CASES[k] for m in E.tail_mutants(k, n)}
    assert named == set(E.MUTANTS[:7])
    for k in KINDS:
        for m in E.MUTANTS[:7]:
            assert sum(m in E.tail_mutants(k, n) for n in E.TAIL_CASES[k]) >= 2, (k, m)


@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('vol', E.AFF_VOLS)
def test_affine_bounds(vol, act):
    x, A, B, g = E.aff_inputs(vol, act)
    ref = E.aff_reference(vol, act)
    assert ref['amb'] == 0
    f32 = E.affine_ref64(x, A, B, act, g, E.aff_share(vol), dtype=torch.float32)
    for k in ('out', 'gx', 'gA', 'gB', 'sum', 'sumsq'):
        w = E.ratio(f32[k].val, ref[k])
        assert w <= 1.0, ('plain fp32 torch is outside the bound', vol, act, k, w)


def _pool_check(kind, T, H, W, OH, OW, pro, act, named):
    x, A, B, g = E.pool_inputs(kind, T, H, W, OH, OW, pro, act)
    ref = E.pool_reference(kind, T, H, W, OH, OW, pro, act)
    share, store = E.pool_share(T, H, W, OH, OW, kind), E.STORE[kind]
    assert ref['amb'] == 0
    f32 = E.pool_ref64(x, A, B, act, OH, OW, g, share, store=store, dtype=torch.float32)
    tag = (kind, T, H, W, OH, OW, pro, act)
    for k in ('out', 'gA', 'gB'):
        if ref[k] is not None:
            assert E.ratio(f32[k].val, ref[k]) <= 1.0, ('plain fp32 torch is outside the bound', tag, k)
    gx32 = f32['gx'].val.float()
    assert E.ratio_x(gx32 if store is None else gx32.to(store).float(), ref['gx'], ref['gx_extra']) <= 1.0, (tag, 'gx')
    for m in E.pool_mutants(T, H, W, OH, OW, kind):
        named.add(m)
        mut = E.pool_ref64(x, A, B, act, OH, OW, g, share, store=store, mutant=m)
        w = max(E.ratio(mut[k].val, ref[k]) for k in ('out', 'gx'))
        assert w > 1.0, ('mutant within the bound: the inputs of this case do not discriminate', tag, m, w)


@pytest.mark.parametrize('kind,T,case', POOL_ALL)
def test_pool_bounds(kind, T, case):
    named = set()
    for pro, act in POOL_OPTS:
        _pool_check(kind, T, *case, pro, act, named)
    H, W, OH, OW = case
    if kind == 'f32' and OH == 1 and OW == 1 and H * W <= 64:
        assert not named
    else:
        assert named == {m for m, on in (('pool_end_floor', H % OH or W % OW), ('pool_swap_hw', H != W)) if on}


@pytest.mark.parametrize('T', E.POOL1_T)
@pytest.mark.parametrize('H,W', E.POOL1_PLANES)
def test_pool1_bounds(H, W, T):
    named = set()
    for pro, act in POOL1_OPTS:
        _pool_check('f32', T, H, W, 1, 1, pro, act, named)
    assert named == ({'pool1_first_sweep_only'} if T > 512 else set())


@pytest.mark.parametrize('T', E.FILM_T)
@pytest.mark.parametrize('H,W,f', E.FILM_CASES)
def test_film_bounds(H, W, f, T):
    x, m, c, g = E.film_inputs(T, H, W, f)
    ref = E.film_reference(T, H, W, f)
    f32 = E.film_ref64(x, m, c, f, g, dtype=torch.float32)
    for k in E.FILM_KEYS:
        assert E.ratio(f32[k].val, ref[k]) <= 1.0, ('plain fp32 torch is outside the bound', (H, W, f, T), k)
    for mu in E.film_mutants(H, W, f):
        mut = E.film_ref64(x, m, c, f, g, mutant=mu)
        w = max(E.ratio(mut[k].val, ref[k]) for k in E.FILM_KEYS)
        assert w > 1.0, ('mutant within the bound: the inputs of this case do not discriminate', (H, W, f, T), mu, w)


def test_pool_and_film_every_mutant_is_named():
    named = {m for T in E.POOL_T for c in E.POOL_GENERAL for m in E.pool_mutants(T, *c)}
    named |= {m for T in E.POOL1_T for (H, W) in E.POOL1_PLANES for m in E.pool_mutants(T, H, W, 1, 1)}
    named |= {m for c in E.FILM_CASES for m in E.film_mutants(*c)}
    assert named == set(E.MUTANTS[7:])
