"""The fused detection loss (csrc/detloss.hip, opt-in) as far as it can be checked without a GPU: the C-ABI boundary, the `fused` switch of
train_fine.detection_loss on CPU tensors (it must fall through to the composed path, bit for bit), and the operator registration."""
import ctypes

import pytest
import torch

from conftest import load_golden, t, maxdiff


def _lib():
    import os
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def test_detloss_symbols_are_exported_and_check_their_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    assert 'cfn_detloss_fwd' in protos and 'cfn_detloss_bwd' in protos
    raw = ctypes.CDLL(cfn_hip.LIB_PATH)
    assert hasattr(raw, 'cfn_detloss_fwd') and hasattr(raw, 'cfn_detloss_bwd')
    lib = cfn_hip.load()
    # argument validation happens before any launch: a null tensor is reported, not crashed on
    rc = lib.cfn_detloss_fwd(None, None, None, None, 1.0, None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, None)
    assert rc == 1 and 'null' in cfn_hip.last_error()
    rc = lib.cfn_detloss_bwd(None, None, None, None, None, None, None, None, 1.0, None, 1, 1, 1, 1, 1, 1, None)
    assert rc == 1 and 'null' in cfn_hip.last_error()


def _golden(name):
    z = load_golden(name)
    return z, t(z['logits']), t(z['labels']), t(z['masks']), int(z['crops']) if 'crops' in z else 1


@pytest.mark.parametrize('name', ['loss_ap', 'loss_multicrop'])
@pytest.mark.parametrize('ac', [1, 0])
def test_fused_switch_on_cpu_tensors_is_the_composed_path(name, ac, monkeypatch):
    """CPU tensors never reach the kernel: fused=True and CFN_FUSED_LOSS=1 return exactly what fused=False returns, which is the
    reference's loss (the goldens of tests/test_product_cpu.py, same 1e-6)"""
    import train_fine
    import train_coarse_fineFEAT as tc
    z, lg, labels, masks, n = _golden(name)

    def loss(**kw):
        if ac:
            return train_fine.detection_loss(lg, labels, masks, True, crops=n, local_norm=True, **kw)
        return tc.detection_loss(lg, labels, masks, crops=n, local_norm=True, **kw)

    monkeypatch.delenv('CFN_FUSED_LOSS', raising=False)
    assert not train_fine.fused_loss_enabled() and train_fine.fused_loss_enabled(True)
    ref = loss(fused=False)
    on = loss(fused=True)
    monkeypatch.setenv('CFN_FUSED_LOSS', '1')
    assert train_fine.fused_loss_enabled() and not train_fine.fused_loss_enabled(False)      # read at call time, no cached value
    env = loss()
    monkeypatch.setenv('CFN_FUSED_LOSS', '0')
    assert not train_fine.fused_loss_enabled()
    for got in (on, env):
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
    cls, loc, probs = on
    assert abs(float(cls) - float(z['cls_%d' % ac])) <= 1e-6 and abs(float(loc) - float(z['loc_%d' % ac])) <= 1e-6
    if 'probs_%d' % ac in z:
        assert maxdiff(probs[:, ::13], z['probs_%d' % ac]) <= 1e-6


def test_ops_detection_loss_has_no_cpu_fallback():
    _lib()
    from cfn_hip import ops
    _z, lg, labels, masks, _n = _golden('loss_ap')
    with pytest.raises(RuntimeError):
        ops.detection_loss(lg, labels, masks, True)
    with pytest.raises(RuntimeError):
        ops.detection_loss(lg.double(), labels, masks, False, want_probs=False)


def test_detection_loss_operator_is_registered_with_a_fake():
    import cfn_hip.torchlib as tl
    assert 'detection_loss' in tl.OPERATORS
    assert hasattr(torch.ops.cfn, 'detection_loss') and hasattr(torch.ops.cfn, 'detection_loss_backward')
    assert str(torch.ops.cfn.detection_loss.default._schema) == (
        'cfn::detection_loss(Tensor logits, Tensor labels, Tensor masks, bool align_corners, SymInt crops=1, Tensor? norm=None, '
        'float world=1., bool want_probs=True) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)')
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    B, C, T, TL, n = 2, 5, 7, 70, 3
    out = torch.ops.cfn.detection_loss(m(B * n, C, T), m(B, C, TL), m(B, TL), True, n)
    cls, loc, probs = out[:3]
    assert cls.shape == () and loc.shape == () and probs.shape == (B, C, TL) and probs.dtype == torch.float32
    # what the backward operator takes beside the inputs: the first maximal frame and the label maximum of every row, the normaliser
    assert out[3].shape == (B * C,) and out[3].dtype == torch.int32 and out[4].shape == (B * C,) and out[5].dtype == torch.float64
    gx = torch.ops.cfn.detection_loss_backward(m(()), m(()), m(B * n, C, T), m(B, C, TL), m(B, TL), out[3], out[4], out[5], True, n, 1.0)
    assert gx.shape == (B * n, C, T)
    assert torch.ops.cfn.detection_loss(m(B, C, T), m(B, C, TL), m(B, TL), False, 1, None, 1.0, False)[2].shape == (1,)


def test_scripts_pass_the_switch_through():
    """the keyword reaches every step function and run(); each script has the flag"""
    import inspect
    import train_fine
    import train_coarse_fineFEAT as tc
    import train_joint
    for fn in (train_fine.detection_loss, tc.detection_loss, train_fine.forward_backward, train_fine.train_step, tc.train_step,
               train_joint.train_step):
        assert inspect.signature(fn).parameters['fused'].default is None, fn
    for mod in (train_fine, tc, train_joint):
        assert inspect.signature(mod.run).parameters['fused_loss'].default is False, mod
        src = inspect.getsource(mod)
        assert "'--fused-loss'" in src and "['--fused-loss'] if args.fused_loss" in src, mod
