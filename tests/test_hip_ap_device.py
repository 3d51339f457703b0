"""GPU: the device-resident AP meter (csrc/apmeter.hip: cfn_ap_append / cfn_ap_sort / cfn_ap_reduce; apmeter.DeviceAPMeter;
cfn_hip.metrics.StepMetrics) against the fp64 reference of tests/ap_ref64.py and the host meter.

Bounds.  The sort is exact (bytes and bit patterns up to the documented canonicalisation of -0.0 and NaN).  AP against ap_ref64:
the kernel sums tp / r in fp64 (at most ~1e5 terms here: error far below fp32 rounding) and rounds ONCE to fp32; AP <= 1, so the
error is at most 2^-25; the bound is 2^-24.  Device meter against host meter: the host meter is within 2e-7 of ap_ref64
(tests/test_ap_device_cpu.py), the device meter within 6e-8: 2^-22 covers the sum."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import ap_ref64 as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
AP_TOL = 2.0 ** -24
METER_TOL = 2.0 ** -22


def _tile():
    from cfn_hip import ops
    return ops.AP_SORT_TILE


def _stores(scores, targets, cap=None):
    """(n, K) host rows -> class-major device stores (K, cap) whose rows behind n hold NaN / 1, and the device count"""
    n, K = scores.shape
    cap = n if cap is None else cap
    sc = torch.full((K, cap), float('nan'), dtype=torch.float32)
    tg = torch.ones((K, cap), dtype=torch.uint8)
    sc[:, :n] = torch.from_numpy(np.ascontiguousarray(scores.T))
    tg[:, :n] = torch.from_numpy(np.ascontiguousarray((targets != 0).astype(np.uint8).T))
    return sc.to(DEV), tg.to(DEV), torch.tensor([n], dtype=torch.int32, device=DEV)


def _check_sort_and_ap(scores, targets, cap=None, what=''):
    """sort: exact; AP: within one fp32 rounding of the fp64 reference; rows behind count: neither read nor written"""
    from cfn_hip import ops
    n, K = scores.shape
    sc, tg, cnt = _stores(scores, targets, cap)
    cap = sc.shape[1]
    out = (torch.full((K, cap), 7.0, device=DEV), torch.full((K, cap), 9, dtype=torch.uint8, device=DEV),
           torch.empty(K, cap, dtype=torch.int32, device=DEV), torch.empty(K, cap, dtype=torch.uint8, device=DEV))
    ss, st = ops.ap_sort(sc, tg, cnt, out=out)
    want_s, want_t = R.sorted_rows(scores, targets)
    got_s, got_t = ss[:, :n].t().cpu(), st[:, :n].t().cpu()
    assert torch.equal(got_t, torch.from_numpy(want_t)), what
    ws = torch.from_numpy(want_s)
    assert bool(((got_s == ws) | (got_s.isnan() & ws.isnan())).all()), what
    if cap > n:
        assert bool((ss[:, n:] == 7.0).all()) and bool((st[:, n:] == 9).all()), what
    ap = ops.average_precision(sc, tg, cnt).cpu().double().numpy()
    d = np.abs(ap - R.ap_ref64(scores, targets)).max()
    print('%s n %d K %d: max |AP - ref64| = %.2e' % (what, n, K, d))
    assert d <= AP_TOL, (what, d)


def _size(name):
    T = _tile()
    return {'1': 1, '63': 63, '64': 64, '65': 65, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '3T+1': 3 * T + 1}[name]


@pytest.mark.parametrize('size', ['1', '63', '64', '65', 'T-1', 'T', 'T+1', '3T+1'])
def test_sort_exact_and_ap_sizes(size):
    n = _size(size)
    for K in (1, 3):
        for i, kind in enumerate(('normal', 'quant8', 'equal')):
            s, tg = R.make_scores(kind, n, K, 7 * n + 10 * K + i)
            _check_sort_and_ap(s, tg, what=kind)
    s, tg = R.make_scores('normal', n, 3, n + 3)
    _check_sort_and_ap(s, tg, cap=n + 37, what='count < cap')              # (an odd capacity: classes start at any alignment)


def test_sort_exact_157_classes():
    n = _tile() + 1
    for i, kind in enumerate(('sigmoid', 'quant8')):
        s, tg = R.make_scores(kind, n, 157, 50 + i)
        _check_sort_and_ap(s, tg, cap=n + 16, what=kind + ' 157')


@pytest.mark.parametrize('byte', [0, 1, 2, 3])
def test_sort_every_digit_value_of_every_pass(byte):
    """bit patterns that differ ONLY in one byte, all 256 values of it, each 5 times with differing targets: one radix pass decides
    the whole order, the other three must keep it"""
    rs = np.random.RandomState(20 + byte)
    v = np.repeat(np.arange(256, dtype=np.uint32), 5)
    rs.shuffle(v)
    bits = (v << 24) | np.uint32(0x00400000) if byte == 3 else np.uint32(0x3f000000) | (v << (8 * byte))      # (byte 3: finite for every v)
    s = bits.astype(np.uint32).view(np.float32).reshape(-1, 1)
    assert np.isfinite(s).all()
    tg = (rs.uniform(size=s.shape) < 0.5).astype(np.float32)
    _check_sort_and_ap(s, tg, what='byte %d' % byte)
    _check_sort_and_ap(np.concatenate([s, s[::-1]], 1), np.concatenate([tg, 1 - tg], 1), cap=s.shape[0] + 5, what='byte %d x2' % byte)


def test_sort_special_values():
    """+-0 tie, denormals are distinct values, every NaN (any payload, either sign) behind -inf in insertion order"""
    den = int(np.float32(1e-40).view(np.uint32))
    bits = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, den, den | 0x80000000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fc12345,
            0x3f800000, 0xbf800000]                                        # +-0, +-inf, +-1e-40, five NaNs, +-1
    b = np.array(bits * 9, dtype=np.uint32)
    np.random.RandomState(3).shuffle(b)
    s = b.view(np.float32).reshape(-1, 1)
    assert int(np.isnan(s).sum()) == 45 and int((s == 0).sum()) == 18
    tg = (np.arange(s.shape[0]) % 2).astype(np.float32).reshape(-1, 1)
    _check_sort_and_ap(s, tg, what='specials')
    _check_sort_and_ap(np.concatenate([s, s[::-1]], 1), np.concatenate([tg, tg], 1), cap=s.shape[0] + 3, what='specials x2')


def test_sort_one_bin_holds_more_than_16_bits():
    s, tg = R.make_scores('equal', 70000, 1, 70)
    _check_sort_and_ap(s, tg, what='70000 equal')


def test_ap_degenerate_classes_repeatable_and_golden():
    import cfn_hip.torchlib  # noqa: F401  (registers torch.ops.cfn.*)
    from cfn_hip import ops
    n = 1000
    s, tg = R.make_scores('normal', n, 3, 90)
    tg[:, 0], tg[:, 1] = 0.0, 1.0                                          # no positive: 0; only positives: exactly 1
    sc, t8, cnt = _stores(s, tg, cap=n + 8)
    aps = [ops.average_precision(sc, t8, cnt) for _ in range(3)]
    assert float(aps[0][0]) == 0.0 and float(aps[0][1]) == 1.0
    assert np.abs(aps[0].cpu().double().numpy() - R.ap_ref64(s, tg)).max() <= AP_TOL
    assert torch.equal(aps[0], aps[1]) and torch.equal(aps[0], aps[2])                     # bit-identical from run to run
    assert torch.equal(torch.ops.cfn.average_precision(sc, t8, cnt), aps[0])               # the registered operator: the same kernels
    ss, st = torch.ops.cfn.ap_sort(sc, t8, cnt)
    ss2, st2 = ops.ap_sort(sc, t8, cnt)
    assert torch.equal(st[:, :n], st2[:, :n]) and torch.equal(ss[:, :n], ss2[:, :n])
    z = load_golden('loss_ap')                                                             # the reference meter's own AP vector
    sc, t8, cnt = _stores(z['ap_scores'], z['ap_targets'])
    assert np.abs(ops.average_precision(sc, t8, cnt).cpu().numpy() - z['ap']).max() <= 1e-6


# ---- append ---------------------------------------------------------------------------------------------------------------------------
def _batch(seed, B, K, TL, p=0.3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, K, TL, generator=g), (torch.rand(B, K, TL, generator=g) < p).float()


def _host_rows(batches):
    """what the loops feed the host meter: train_fine._ap_rows per batch, concatenated -> (n, K) scores, targets"""
    import train_fine
    sc, tg = [], []
    for probs, labels, valid in batches:
        v = torch.full((probs.shape[0],), probs.shape[2], dtype=torch.int32) if valid is None else valid.clamp(max=probs.shape[2])
        for s, t in train_fine._ap_rows(probs, labels, v):
            sc.append(s)
            tg.append(t)
    return np.concatenate(sc), np.concatenate(tg)


def _dev(batch):
    return tuple(None if x is None else x.to(DEV) for x in batch)


def test_append_matches_host_rows():
    import apmeter
    B, K, TL = 3, 5, 40
    valid = torch.tensor([40, 0, 17], dtype=torch.int32)
    batches = [_batch(1, B, K, TL) + (valid,), _batch(2, B, K, TL) + (torch.tensor([1, 40, 39], dtype=torch.int32),),
               _batch(3, 2, K, TL) + (None,),                                               # valid=None: every frame
               _batch(4, 2, K, TL) + (torch.tensor([1000, 3], dtype=torch.int32),)]         # valid > TL is clamped
    for fixed in (None, 1024):
        m = apmeter.DeviceAPMeter(DEV, capacity=fixed)
        for i, b in enumerate(batches):
            m.add_batch(*_dev(b))
            want_s, want_t = _host_rows(batches[:i + 1])
            n = want_s.shape[0]
            assert int(m.count) == n
            sc, tg = m.stores
            assert torch.equal(sc[:, :n].cpu(), torch.from_numpy(want_s).t())
            assert torch.equal(tg[:, :n].cpu(), torch.from_numpy(want_t).t().to(torch.uint8))
        assert int(m.flags) == 0


def test_append_operator_mutates_its_stores():
    import cfn_hip.torchlib  # noqa: F401  (registers torch.ops.cfn.*)
    K, cap = 5, 64
    sc, tg = torch.zeros(K, cap, device=DEV), torch.zeros(K, cap, dtype=torch.uint8, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    probs, labels = _batch(6, 2, K, 10)
    torch.ops.cfn.ap_append(probs.to(DEV), labels.to(DEV), torch.tensor([10, 4], dtype=torch.int32, device=DEV), sc, tg, state[0:1], state[1:2])
    want_s, want_t = _host_rows([(probs, labels, torch.tensor([10, 4], dtype=torch.int32))])
    assert state.tolist() == [14, 0]
    assert torch.equal(sc[:, :14].cpu(), torch.from_numpy(want_s).t()) and torch.equal(tg[:, :14].cpu(), torch.from_numpy(want_t).t().to(torch.uint8))


def test_append_non_binary_label_raises_at_value():
    import apmeter
    m = apmeter.DeviceAPMeter(DEV)
    probs, labels = _batch(7, 2, 5, 16)
    m.add_batch(probs.to(DEV), labels.to(DEV))
    assert torch.is_tensor(m.value())
    labels[1, 3, 9] = 0.5
    m.add_batch(probs.to(DEV), labels.to(DEV), torch.tensor([16, 9], dtype=torch.int32, device=DEV))       # frame 9 of video 1 is not valid
    assert torch.is_tensor(m.value())
    m.add_batch(probs.to(DEV), labels.to(DEV))
    with pytest.raises(AssertionError, match='targets should be binary'):
        m.value()
    m.reset()
    assert m.value() == 0


def test_append_past_fixed_capacity_flags_and_writes_nothing():
    from cfn_hip import ops
    import apmeter
    K, cap, G = 5, 64, 4096
    sbuf = torch.full((K * cap + G,), -3.0, device=DEV)                       # the stores with a guard region behind them
    tbuf = torch.full((K * cap + G,), 77, dtype=torch.uint8, device=DEV)
    sc, tg = sbuf[:K * cap].view(K, cap), tbuf[:K * cap].view(K, cap)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    probs, labels = _batch(8, 1, K, 40)
    ops.ap_append(probs.to(DEV), labels.to(DEV), None, sc, tg, state[0:1], state[1:2])
    assert state.tolist() == [40, 0]
    ops.ap_append(probs.to(DEV), labels.to(DEV), None, sc, tg, state[0:1], state[1:2])                     # 80 rows do not fit into 64
    assert state.tolist() == [40, ops.AP_FLAG_OVERFLOW]
    assert bool((sc[:, 40:] == -3.0).all()) and bool((tg[:, 40:] == 77).all())
    assert bool((sbuf[K * cap:] == -3.0).all()) and bool((tbuf[K * cap:] == 77).all())
    assert torch.equal(sc[:, :40].cpu(), probs[0])
    ops.ap_append(probs.to(DEV), labels.to(DEV), torch.tensor([24], dtype=torch.int32, device=DEV), sc, tg, state[0:1], state[1:2])   # fits exactly
    assert state.tolist() == [64, ops.AP_FLAG_OVERFLOW] and bool((sbuf[K * cap:] == -3.0).all()) and bool((tbuf[K * cap:] == 77).all())
    m = apmeter.DeviceAPMeter(DEV, capacity=cap)
    m.add_batch(probs.to(DEV), labels.to(DEV))
    assert torch.is_tensor(m.value())
    m.add_batch(probs.to(DEV), labels.to(DEV))
    with pytest.raises(RuntimeError, match='capacity'):
        m.value()


def test_offsets_past_2_31_elements():
    """K * cap above 2^31 elements: class 2 of a (3, 2^30) store starts at element 2^31 (the stores are allocated, never filled)"""
    from cfn_hip import ops
    K, cap = 3, 2 ** 30
    sc, tg = torch.empty(K, cap, dtype=torch.float32, device=DEV), torch.empty(K, cap, dtype=torch.uint8, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    probs = torch.arange(K * 8, dtype=torch.float32).view(1, K, 8)
    labels = torch.tensor([[[0.] * 8, [1.] * 8, [0., 1.] * 4]])
    ops.ap_append(probs.to(DEV), labels.to(DEV), None, sc, tg, state[0:1], state[1:2])
    assert state.tolist() == [8, 0]
    assert torch.equal(sc[:, :8].cpu(), probs[0]) and torch.equal(tg[:, :8].cpu(), labels[0].to(torch.uint8))
    ap = ops.ap_reduce(tg, state[0:1]).cpu().double().numpy()                # (the rows as they lie: already "sorted")
    assert np.abs(ap - R.ap_ref64(-np.arange(8, dtype=np.float32).reshape(8, 1).repeat(3, 1), labels[0].t().numpy())).max() <= AP_TOL


# ---- the meter --------------------------------------------------------------------------------------------------------------------------
def _three_batches(K=7, TL=48):
    return [_batch(11, 3, K, TL) + (torch.tensor([48, 5, 30], dtype=torch.int32),), _batch(12, 3, K, TL) + (torch.tensor([0, 48, 47], dtype=torch.int32),),
            _batch(13, 3, K, TL) + (torch.tensor([17, 18, 19], dtype=torch.int32),)]


def _host_value(batches):
    import apmeter
    import train_fine
    m = apmeter.APMeter()
    for probs, labels, valid in batches:
        for s, t in train_fine._ap_rows(probs, labels, valid):
            m.add(s, t)
    return m.value()


def test_meter_against_host_meter_reset_growth_and_add():
    import apmeter
    import train_fine
    batches = _three_batches()
    want = _host_value(batches)
    assert apmeter.DeviceAPMeter(DEV).value() == 0                           # nothing added: 0, as the reference
    m = apmeter.DeviceAPMeter(DEV)
    m.MIN_CAPACITY = 16                                                      # the second and third batch each cross a capacity boundary
    caps = []
    for b in batches:
        m.add_batch(*_dev(b))
        caps.append(m.stores[0].shape[1])
    assert caps[0] < caps[1] < caps[2]
    got = m.value()
    assert got.dtype == torch.float32 and got.device.type == 'cpu' and got.shape == want.shape
    d = float((got.double() - want.double()).abs().max())
    print('device meter vs host meter: max |dAP| = %.2e' % d)
    assert d <= METER_TOL
    s, t = _host_rows(batches)
    assert np.abs(got.double().numpy() - R.ap_ref64(s, t)).max() <= AP_TOL                # growth kept the earlier rows
    assert torch.equal(m.value_device().cpu(), got)
    m.reset()                                                                # reset keeps the buffers; reuse
    assert m.value() == 0 and m.stores[0].shape[1] == caps[2]
    m.add_batch(*_dev(batches[1]))
    assert float((m.value().double() - _host_value(batches[1:2]).double()).abs().max()) <= METER_TOL
    a = apmeter.DeviceAPMeter(DEV)                                           # add(rows x K) is add_batch of the transposed rows
    for probs, labels, valid in batches:
        for sc, tg in train_fine._ap_rows(probs, labels, valid):
            a.add(torch.from_numpy(sc).to(DEV), torch.from_numpy(tg).to(DEV))
    assert torch.equal(a.value(), got)
    with pytest.raises(NotImplementedError):
        a.add(torch.zeros(4, 7, device=DEV), torch.zeros(4, 7, device=DEV), weight=torch.ones(4, device=DEV))


def _losses(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((), generator=g), torch.rand((), generator=g)) for _ in range(n)]


def _run_step_metrics(device_ap, batches, losses, guard=False):
    from cfn_hip.metrics import StepMetrics
    sm = StepMetrics(device_ap, DEV)
    if device_ap:
        sm.apm.MIN_CAPACITY = 16
    dev_batches = [_dev(b) for b in batches]
    dev_losses = [(c.to(DEV), l.to(DEV)) for c, l in losses]
    sm.start_phase()
    torch.cuda.synchronize()
    if guard:
        torch.cuda.set_sync_debug_mode('error')
    try:
        for (probs, labels, valid), (cls, loc) in zip(dev_batches, dev_losses):
            sm.update(cls, loc, probs, labels, valid)
    finally:
        if guard:
            torch.cuda.set_sync_debug_mode('default')
    return sm.report()


def test_no_host_synchronisation_in_the_hot_path():
    import apmeter
    batches = _three_batches()
    plain = apmeter.DeviceAPMeter(DEV)
    plain.MIN_CAPACITY = 16
    for b in batches:
        plain.add_batch(*_dev(b))
    want = plain.value()
    m = apmeter.DeviceAPMeter(DEV)
    m.MIN_CAPACITY = 16
    dev_batches = [_dev(b) for b in batches]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for b in dev_batches:                                                # three appends, the stores grow on the way
            m.add_batch(*b)
        ap_dev = m.value_device()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert m.stores[0].shape[1] > 16 * 3
    assert torch.equal(m.value(), want) and torch.equal(ap_dev.cpu(), want)
    losses = _losses(21, 3)
    assert _run_step_metrics(True, batches, losses, guard=True) == _run_step_metrics(True, batches, losses)


def test_step_metrics_device_equals_host():
    batches, losses = _three_batches(), _losses(22, 3)
    d_loc, d_cls, d_map = _run_step_metrics(True, batches, losses)
    h_loc, h_cls, h_map = _run_step_metrics(False, batches, losses)
    assert (d_loc, d_cls) == (h_loc, h_cls)                                  # the same fp64 additions in the same order
    assert h_map > 0.1 and abs(d_map - h_map) <= METER_TOL


@pytest.mark.capture
def test_add_batch_in_a_captured_graph():
    import apmeter
    batches = _three_batches()
    eager = apmeter.DeviceAPMeter(DEV, capacity=512)
    for b in batches:
        eager.add_batch(*_dev(b))
    m = apmeter.DeviceAPMeter(DEV, capacity=512)
    static = [x.clone() for x in _dev(batches[0])]
    m.add_batch(*static)                                                     # warm-up outside the capture: the stores exist from here on
    m.reset()
    ptrs = [x.data_ptr() for x in m.stores]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.add_batch(*static)
    for b in batches:
        for dst, src in zip(static, _dev(b)):
            dst.copy_(src)
        g.replay()
    torch.cuda.synchronize()
    assert [x.data_ptr() for x in m.stores] == ptrs
    assert int(m.count) == int(eager.count)
    n = int(m.count)
    assert torch.equal(m.stores[0][:, :n], eager.stores[0][:, :n]) and torch.equal(m.stores[1][:, :n], eager.stores[1][:, :n])
    assert torch.equal(m.value(), eager.value())


# ---- the loops ----------------------------------------------------------------------------------------------------------------------------
def test_train_fine_two_steps_device_ap(tmp_path):
    import train_fine
    loaders = {'train': train_fine.SyntheticCharades(2, 3, frames=8, crop=64),
               'val': train_fine.SyntheticCharades(1, 1, frames=8, crop=64)}
    net = train_fine.run(batch_size=2, dataloaders=loaders, max_steps=2, pretrained=None, log=lambda *_: None,
                         save_model=str(tmp_path / 'fine_'), device_ap=True)
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert int(net.bn1.split_bn.num_batches_tracked) == 2


def test_train_coarse_two_steps_device_ap(tmp_path):
    import train_coarse_fineFEAT as tc
    loaders = {'train': tc.SyntheticCoarse(1, 1, frames=8, fine_len=12), 'val': tc.SyntheticCoarse(1, 1, frames=8, fine_len=12)}
    net = tc.run(batch_size=1, dataloaders=loaders, max_steps=2, pretrained=None, csv_path=None, log=lambda *_: None,
                 save_model=str(tmp_path / 'coarse_'), device_ap=True)
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_train_joint_two_steps_device_ap(tmp_path):
    import train_joint
    loader = train_joint.SyntheticJoint(1, 2, fine_frames=16, coarse_frames=8)
    logs = []
    fine, coarse = train_joint.run(batch_size=1, dataloader=loader, max_steps=2, log=logs.append, save_model=str(tmp_path / 'j_'), device_ap=True)
    assert len(logs) == 2 and all(' mAP: ' in line for line in logs)
    assert all(torch.isfinite(p).all() for m in (fine, coarse) for p in m.parameters())
