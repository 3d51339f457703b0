"""CPU: the host side of the device-resident AP meter (csrc/apmeter.hip, apmeter.DeviceAPMeter, cfn_hip/metrics.py) -- the fp64
reference the GPU tests use against the host meter and the reference's own AP vector, the C ABI's prototypes and argument checks,
the operator registration, and the opt-in switches of the training loops."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden

import ap_ref64 as R


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1023, 1025, 4097, 20000])
def test_ref64_against_host_meter(n):
    """APMeter accumulates tp and divides in fp32: measured worst case over these inputs 6.2e-8 per class; the bound is three times that"""
    from apmeter import APMeter
    for i, kind in enumerate(('normal', 'sigmoid', 'quant8', 'equal')):
        s, tg = R.make_scores(kind, n, 4, 1000 * i + n)
        m = APMeter()
        m.add(s, tg)
        d = np.abs(m.value().numpy().astype(np.float64) - R.ap_ref64(s, tg)).max()
        print('n %d %s: max |APMeter - ref64| = %.2e' % (n, kind, d))
        assert d <= 2e-7, (n, kind, d)


def test_ref64_against_reference_ap_vector():
    z = load_golden('loss_ap')
    assert np.abs(R.ap_ref64(z['ap_scores'], z['ap_targets']) - z['ap']).max() <= 1e-6      # as the APMeter-versus-golden test


def test_ref64_sorted_rows_order_on_special_values():
    s = np.array([np.nan, -0.0, 0.0, -np.inf, 1e-40, np.inf, -1e-40, np.nan, 0.0], dtype=np.float32)
    tg = np.arange(9) % 2
    ss, st = R.sorted_rows(s, tg)
    assert np.isinf(ss[0, 0]) and ss[0, 0] > 0 and ss[1, 0] == np.float32(1e-40) and ss[1, 0] != 0           # denormals are values
    assert list(st[2:5, 0]) == [1, 0, 0] and not ss[2:5, 0].any()                                            # +-0 tie: insertion order
    assert ss[5, 0] == np.float32(-1e-40) and np.isinf(ss[6, 0]) and np.isnan(ss[7:, 0]).all() and list(st[7:, 0]) == [0, 1]


def test_abi_prototypes_and_argument_checks():
    import cfn_hip
    from cfn_hip import ops
    protos = cfn_hip.header_prototypes()
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    want = {'cfn_ap_append': ([f32, f32, i32, f32, u8, i32, i32], 12), 'cfn_ap_sort': ([f32, u8, i32, f32, u8, i32, u8], 10),
            'cfn_ap_reduce': ([u8, i32, f32], 6)}
    for name, (dts, nargs) in want.items():
        assert name in protos, name
        ret, at, dt = protos[name]
        assert ret is ctypes.c_int and len(at) == nargs and dt[:len(dts)] == dts and at[-1] is ctypes.c_void_p, name
    assert protos['cfn_ap_append'][1][-2] is ctypes.c_long and protos['cfn_ap_sort'][1][-2] is ctypes.c_long          # cap: 64-bit
    lib = cfn_hip.load()                                          # raises if a declared symbol is not exported
    assert lib.cfn_ap_sort_tile() == ops.AP_SORT_TILE
    p = torch.zeros(4, dtype=torch.int32).data_ptr()              # (argument checks run before any launch: never dereferenced)
    ok_append = [p, p, None, p, p, p, p]
    for i in (0, 1, 3, 4, 5, 6):
        a = list(ok_append)
        a[i] = None
        assert lib.cfn_ap_append(*a, 1, 1, 1, 16, None) == 1 and 'null' in cfn_hip.last_error(), i
    for bad in ((0, 1, 1, 16), (1, 0, 1, 16), (1, 1, 0, 16), (1, 1, 1, 0), (1, 1, 1, -5), (1, 1, 1, 2 ** 31)):
        assert lib.cfn_ap_append(*ok_append, *bad, None) == 1 and 'shape' in cfn_hip.last_error(), bad
    for i in range(7):
        a = [p] * 7
        a[i] = None
        assert lib.cfn_ap_sort(*a, 1, 16, None) == 1 and 'null' in cfn_hip.last_error(), i
    for bad in ((0, 16), (1, 0), (-1, 16), (1, 2 ** 31)):
        assert lib.cfn_ap_sort(*([p] * 7), *bad, None) == 1 and 'shape' in cfn_hip.last_error(), bad
    for i in range(3):
        a = [p] * 3
        a[i] = None
        assert lib.cfn_ap_reduce(*a, 1, 16, None) == 1 and 'null' in cfn_hip.last_error(), i
    for bad in ((0, 16), (1, 0)):
        assert lib.cfn_ap_reduce(p, p, p, *bad, None) == 1 and 'shape' in cfn_hip.last_error(), bad


def test_metric_operators_registered_with_meta_shapes():
    import cfn_hip.torchlib as tl
    assert tl.METRIC_OPERATORS == ('ap_append', 'ap_sort', 'average_precision')
    assert not set(tl.METRIC_OPERATORS) & (set(tl.OPERATORS) | set(tl.INPUT_OPERATORS) | set(tl.AUGMENT_OPERATORS))
    for name in tl.METRIC_OPERATORS:
        assert hasattr(torch.ops.cfn, name), name
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    sc, tg, cnt = m(157, 4096), m(157, 4096, dt=torch.uint8), m(1, dt=torch.int32)
    ss, st = torch.ops.cfn.ap_sort(sc, tg, cnt)
    assert ss.shape == (157, 4096) and ss.dtype == torch.float32 and st.shape == (157, 4096) and st.dtype == torch.uint8
    ap = torch.ops.cfn.average_precision(sc, tg, cnt)
    assert ap.shape == (157,) and ap.dtype == torch.float32
    assert torch.ops.cfn.ap_append(m(8, 157, 640), m(8, 157, 640), m(8, dt=torch.int32), sc, tg, cnt, m(1, dt=torch.int32)) is None
    assert torch.ops.cfn.ap_append(m(8, 157, 640), m(8, 157, 640), None, sc, tg, cnt, m(1, dt=torch.int32)) is None
    schema = torch.ops.cfn.ap_append.default._schema
    assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ['scores', 'targets', 'count', 'flags']


def test_cpu_tensors_raise():
    from cfn_hip import ops
    import apmeter
    sc, tg, cnt = torch.zeros(3, 32), torch.zeros(3, 32, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.ap_sort(sc, tg, cnt)
    with pytest.raises(RuntimeError):
        ops.average_precision(sc, tg, cnt)
    with pytest.raises(RuntimeError):
        ops.ap_append(torch.zeros(1, 3, 8), torch.zeros(1, 3, 8), None, sc, tg, cnt, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        apmeter.DeviceAPMeter('cpu')
    meter = apmeter.DeviceAPMeter.__new__(apmeter.DeviceAPMeter)          # (the constructor refuses a CPU device; add_batch refuses CPU tensors)
    with pytest.raises(RuntimeError):
        meter.add_batch(torch.zeros(1, 3, 8), torch.zeros(1, 3, 8))


def test_run_signatures_carry_device_ap_off():
    import train_fine
    import train_coarse_fineFEAT
    import train_joint
    for mod in (train_fine, train_coarse_fineFEAT, train_joint):
        assert inspect.signature(mod.run).parameters['device_ap'].default is False, mod.__name__


def test_step_metrics_host_path_is_the_loops_bookkeeping():
    """StepMetrics(False) on CPU tensors: the host APMeter over _ap_rows and Python-float loss totals, as the loops did inline"""
    import train_fine
    from apmeter import APMeter
    from cfn_hip.metrics import StepMetrics
    g = torch.Generator().manual_seed(5)
    sm, apm = StepMetrics(False), APMeter()
    tot_cls = tot_loc = 0.0
    sm.start_phase()
    for _ in range(3):
        probs, labels = torch.rand(2, 5, 12, generator=g), (torch.rand(2, 5, 12, generator=g) < 0.3).float()
        valid = torch.tensor([12, 7], dtype=torch.int32)
        cls, loc = torch.rand((), generator=g), torch.rand((), generator=g)
        sm.update(cls, loc, probs, labels, valid)
        for sc, tg in train_fine._ap_rows(probs, labels, valid):
            apm.add(sc, tg)
        tot_cls += float(cls)
        tot_loc += float(loc)
    m_loc, m_cls, m_ap = sm.report()
    assert (m_loc, m_cls) == (tot_loc / 3, tot_cls / 3) and m_ap == float(apm.value().mean())
    sm.reset_ap()
    assert sm.mean_ap() == 0.0
