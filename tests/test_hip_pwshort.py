"""cfn_pwconv_short_bwd (csrc/pwshort.hip): the backward of the stride-2 shortcut conv of a stage-first block in one pass -- the compact
data gradient da = W^T G' and the weight gradient gw += G' act(A x + B)^T on the stride lattice -- against the fp64 expressions of
tests/pw_ref64.py.  The bounds are the ones the two separate kernels are held to in tests/test_hip_ops.py: relerr <= 2e-6 for the data
gradient (test_pwconv_data_gradient_with_compact_shortcut_gradient, PW_CEIL['gx']) and <= 3e-6 for the weight gradient (PW_CEIL['gw'])."""
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr
from pw_ref64 import pw_ref64

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CEIL_DA, CEIL_GW = 2e-6, 3e-6

# (N, Cin, Cout, T, Hi, Wi, prologue act or None)
SHAPES = {
    'l1_24x24_wo8_relu': (2, 24, 24, 3, 16, 16, 1),      # layer-1 widths behind the BN + ReLU prologue, 16-byte loads
    'l2_24x48_wo6': (2, 24, 48, 2, 12, 12, None),        # Wo = 6: not a multiple of 4
    'l3_48x96_wo14': (1, 48, 96, 2, 28, 28, None),       # channel tiles split over 3 x 2 waves, two strips per sample
    'l4_96x192_wo7': (2, 96, 192, 3, 14, 14, None),      # 6 x 1 waves, Wo = 7 and T*Ho*Wo = 147: every element a dword load
    'odd_24x48_15x13': (1, 24, 48, 2, 15, 13, None),     # odd planes: Ho = 8, Wo = 7 (16-byte loads of gy / y, dword loads of x)
    'l4_96x192_wo7_t4': (1, 96, 192, 4, 14, 14, None),   # the 6 x 1 kernel with T*Ho*Wo % 4 == 0: 16-byte loads of gy / y, as at full size
}
TERMS = {'all': ('gs', 'gq', 'gsc'), 'no_gs': ('gq', 'gsc'), 'no_gq': ('gs', 'gsc'), 'no_gsc': ('gs', 'gq')}


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def prefill(*shape):
    """the known non-zero pattern gw starts from: the kernel must ADD into it"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.float64, device=DEV) % 7 - 3) * 0.25 + 0.125).view(shape)


_cache = {}


def case(name, terms):
    """inputs and fp64 references of one case, built once and shared (nothing writes to them)"""
    key = (name, terms)
    if key in _cache:
        return _cache[key]
    N, Cin, Cout, T, Hi, Wi, act = SHAPES[name]
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    f64 = lambda seed, *shape, scale=1.0: (rnd(seed, *shape) * scale).double().to(DEV)
    on = TERMS[terms]
    c = dict(N=N, Cin=Cin, Cout=Cout, T=T, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, act=act or 0)
    c['gy'], c['y'], c['x'] = rnd(1, N, Cout, T, Ho, Wo).to(DEV), rnd(2, N, Cout, T, Ho, Wo).to(DEV), rnd(3, N, Cin, T, Hi, Wi).to(DEV)
    c['w'] = ((2.0 / Cout) ** 0.5 * rnd(4, Cout, Cin)).to(DEV)
    c['gs'] = f64(5, N, Cout, scale=0.05) if 'gs' in on else None
    c['gq'] = f64(6, N, Cout, scale=0.01) if 'gq' in on else None
    c['gsc'] = 1.0 + f64(7, N, Cout, scale=0.3) if 'gsc' in on else None
    c['A'] = c['B'] = None
    if act is not None:
        c['A'], c['B'] = 1.0 + f64(8, N, Cin, scale=0.2), f64(9, N, Cin, scale=0.2)
    xl = c['x'][:, :, :, ::2, ::2].contiguous()
    # da: the data gradient on the output grid without a prologue; gw: the weight gradient behind the prologue on the lattice
    c['da_ref'] = pw_ref64(c['gy'], c['y'], c['gs'], c['gq'], c['gsc'], c['w'], xl, None, None, 0)[0]
    c['gw_ref'] = pw_ref64(c['gy'], c['y'], c['gs'], c['gq'], c['gsc'], c['w'], xl, c['A'], c['B'], c['act'])[3]
    _cache[key] = c
    return c


def run(c, stride=2, fill=True):
    import cfn_hip
    da = torch.full((c['N'], c['Cin'], c['T'], c['Ho'], c['Wo']), float('nan'), device=DEV)
    gw = prefill(c['Cout'], c['Cin']) if fill else torch.zeros(c['Cout'], c['Cin'], dtype=torch.float64, device=DEV)
    ok = cfn_hip.call_try('cfn_pwconv_short_bwd', c['gy'], c['y'], c['gs'], c['gq'], c['gsc'], c['w'], c['x'], c['A'], c['B'], c['act'], da, gw,
                          c['N'], c['Cin'], c['Cout'], c['T'], c['Hi'], c['Wi'], stride)
    return ok, da, gw


@pytest.mark.parametrize('terms', list(TERMS))
@pytest.mark.parametrize('name', list(SHAPES))
def test_short_bwd_against_fp64(name, terms):
    c = case(name, terms)
    ok, da, gw = run(c)
    assert ok is True, 'declined'
    gw = gw - prefill(c['Cout'], c['Cin'])            # what the kernel added to the pattern
    e_da, e_gw = relerr(da, c['da_ref']), relerr(gw, c['gw_ref'])
    print('%s %s: relerr da %.3e  gw %.3e' % (name, terms, e_da, e_gw))
    assert torch.isfinite(da).all()                   # every element of the compact gradient is written
    assert e_da <= CEIL_DA, ('da', e_da)
    assert e_gw <= CEIL_GW, ('gw', e_gw)


def test_terms_are_visible():
    """each of gsum, gsumsq, gscale and the prologue, left out of the reference, moves the outputs far beyond their ceilings: a kernel that
    dropped one cannot pass the cases above"""
    c = case('l1_24x24_wo8_relu', 'all')
    xl = c['x'][:, :, :, ::2, ::2].contiguous()
    for drop in ('gs', 'gq', 'gsc'):
        v = dict(c, **{drop: None})
        da, _, _, gw = pw_ref64(v['gy'], v['y'], v['gs'], v['gq'], v['gsc'], v['w'], xl, v['A'], v['B'], v['act'])
        assert relerr(gw, c['gw_ref']) >= 20 * CEIL_GW, drop
        da = pw_ref64(v['gy'], v['y'], v['gs'], v['gq'], v['gsc'], v['w'], xl, None, None, 0)[0]
        assert relerr(da, c['da_ref']) >= 20 * CEIL_DA, drop
    gw = pw_ref64(c['gy'], c['y'], c['gs'], c['gq'], c['gsc'], c['w'], xl, None, None, 0)[3]
    assert relerr(gw, c['gw_ref']) >= 20 * CEIL_GW, 'prologue'


@pytest.mark.parametrize('name', list(SHAPES))
def test_short_bwd_repeats_bit_for_bit_in_deterministic_mode(name):
    import cfn_hip
    c = case(name, 'all')
    prev = cfn_hip.deterministic(True)
    try:
        outs = [run(c) for _ in range(3)]
    finally:
        cfn_hip.deterministic(prev)
    assert all(o[0] is True for o in outs)
    for o in outs[1:]:
        assert torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])
    assert relerr(outs[0][1], c['da_ref']) <= CEIL_DA
    assert relerr(outs[0][2] - prefill(c['Cout'], c['Cin']), c['gw_ref']) <= CEIL_GW


def test_stride_3_is_declined_and_nothing_is_written():
    c = case('l2_24x48_wo6', 'all')
    ok, da, gw = run(c, stride=3)
    assert ok is False
    assert torch.isnan(da).all() and torch.equal(gw, prefill(c['Cout'], c['Cin']))


def test_switch_declines_per_call(monkeypatch):
    """CFN_PW_SHORT=0 is read per call: the entry point declines (callers take the two separate kernels) and takes the call again without it"""
    c = case('l2_24x48_wo6', 'all')
    monkeypatch.setenv('CFN_PW_SHORT', '0')
    assert run(c)[0] is False
    monkeypatch.setenv('CFN_PW_SHORT', '1')
    assert run(c)[0] is True
    monkeypatch.delenv('CFN_PW_SHORT')
    assert run(c)[0] is True


def test_stage_first_block_gradients_agree_with_the_two_kernel_path(monkeypatch):
    """a stage-first Bottleneck (24 -> (108, 48), stride 2, train mode): every parameter gradient and the input gradient with the one-pass
    shortcut backward (CFN_PW_SHORT=1) against today's two kernels (CFN_PW_SHORT=0), to the tighter of the two bounds"""
    import x3d_fine
    from oracle import spec
    cin, planes = 24, (108, 48)
    ds = torch.nn.Sequential(x3d_fine.conv1x1x1(cin, planes[1], 2), x3d_fine.SubBatchNorm3d(num_splits=1, num_features=planes[1], affine=True))
    m = x3d_fine.Bottleneck(cin, planes, 2, ds, index=0, base_bn_splits=1)
    spec.fill_module_(m)
    m.to(DEV).train(True)
    x0 = F.relu(spec.rand_input(91, (2, cin, 4, 28, 28))).to(DEV)
    r = None
    grads = {}
    for sw in ('1', '0'):
        monkeypatch.setenv('CFN_PW_SHORT', sw)
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        if r is None:
            r = spec.rand_input(92, tuple(y.shape)).to(DEV)
        (y * r).sum().backward()
        torch.cuda.synchronize()
        grads[sw] = dict({k: p.grad.detach().clone() for k, p in m.named_parameters()}, x=x.grad.detach().clone())
    assert set(grads['1']) == set(grads['0']) and 'downsample.0.weight' in grads['1']
    for k in grads['0']:
        e = relerr(grads['1'][k], grads['0'][k])
        print('%s: relerr %.3e' % (k, e))
        assert e <= min(CEIL_DA, CEIL_GW), (k, e)
