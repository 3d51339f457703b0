"""cfn_ap_calibrate on the GPU (csrc/apcal.hip) against cfn_hip.calibrate.thresholds_reference: thr (bit patterns), cut, tp, ok and stat
BIT-EQUAL, in canary-filled buffers, at every row count and class-row alignment at which the kernel takes another path; the loop closed on
the device (meter -> thresholds -> decode gives back the cut); value_and_thresholds; a captured graph replayed on other rows; and the two
training entry points decoding their validation phase with the thresholds their training phases calibrated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY_F, CANARY_I, CANARY_B = 777.25, -77777, 0xAB
F1 = ('f1', None)
K1 = [F1]
K3 = [('recall', 0.6), F1, ('precision', 0.7)]
K16 = [('recall', q) for q in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)] + [F1, ('precision', 0.3), ('precision', 0.5), ('precision', 0.9), ('precision', 1.0), F1]


def _tile():
    import cfn_hip
    return int(cfn_hip.query('cfn_ap_calibrate_tile'))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _padded(C, w, dtype, fill, pad_rows=2, pad_tail=5):
    """a (C, w) contiguous output at the head of a canary-filled buffer with room for pad_rows more rows and a tail"""
    buf = torch.full(((C + pad_rows) * w + pad_tail,), fill, dtype=dtype, device=DEV)
    return buf, buf[:C * w].view(C, w)


def _numpy_sorted(scores, targets, n):
    """the class rows as cfn_ap_sort leaves them: a stable descending sort, -0.0 as +0.0, NaN last"""
    s = np.where(scores[:, :n] == 0, np.float32(0.0), scores[:, :n])
    with np.errstate(invalid='ignore'):
        order = np.argsort(-s, axis=1, kind='stable')
    return np.take_along_axis(s, order, 1), np.take_along_axis(targets[:, :n], order, 1)


def _checked(scores, targets, n, criteria):
    """scores (C, cap) fp32 / targets (C, cap) uint8 numpy, UNSORTED, the first n rows of every class valid -> sorts with ops.ap_sort, runs
    ops.ap_calibrate twice into canary-filled buffers and compares everything with thresholds_reference over the sort's own stores;
    returns the reference's (thr, cut, tp, ok, stat)"""
    from cfn_hip import ops
    from cfn_hip.calibrate import criteria_tensors, thresholds_reference
    C, cap = scores.shape
    K = len(criteria)
    count = torch.tensor([n], dtype=torch.int32, device=DEV)
    sort_out = (torch.full((C, cap), CANARY_F, dtype=torch.float32, device=DEV), torch.full((C, cap), CANARY_B, dtype=torch.uint8, device=DEV),
                torch.empty(C, cap, dtype=torch.int32, device=DEV), torch.empty(C, cap, dtype=torch.uint8, device=DEV))
    ss, st = ops.ap_sort(torch.from_numpy(scores).to(DEV), torch.from_numpy(targets).to(DEV), count, out=sort_out)
    hs, ht = ss.cpu().numpy(), st.cpu().numpy()
    want_s, want_t = _numpy_sorted(scores, targets, n)                                    # the stores, once against numpy's stable sort
    assert np.array_equal(hs[:, :n], want_s, equal_nan=True) and np.array_equal(ht[:, :n], want_t)
    assert (hs[:, n:] == np.float32(CANARY_F)).all() and (ht[:, n:] == CANARY_B).all()
    kinds, values = criteria_tensors(criteria, DEV)
    fills = ((K, torch.float32, CANARY_F), (K, torch.int32, CANARY_I), (K, torch.int32, CANARY_I), (K, torch.uint8, CANARY_B), (2, torch.int32, CANARY_I))
    bufs, outs = zip(*[_padded(C, w, dt, fill) for w, dt, fill in fills])
    got = ops.ap_calibrate(ss, st, count, kinds, values, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    first = [_bits(g).clone() for g in got]
    ref = thresholds_reference(hs, ht, n, criteria)
    for name, g, r in zip(('thr', 'cut', 'tp', 'ok', 'stat'), first, ref):
        assert torch.equal(g, _bits(r)), (name, n, C, K, g.tolist()[:4], _bits(r).tolist()[:4])
    for buf, (w, dt, fill) in zip(bufs, fills):                                           # the padding rows and the tail keep their canary
        assert bool((buf[C * w:] == fill).all())
    ops.ap_calibrate(ss, st, count, kinds, values, out=outs)                              # a second call: the same bits
    assert all(torch.equal(_bits(g), f) for g, f in zip(got, first))
    assert torch.equal(_bits(ss), _bits(torch.from_numpy(hs))) and torch.equal(st.cpu(), torch.from_numpy(ht))      # the stores are only read
    return ref


def _quantised(r, C, n, levels):
    return (r.randint(0, levels, size=(C, n)).astype(np.float32) / np.float32(levels)).astype(np.float32)


def _mixed_stores(seed, C, n, cap):
    """class 0: all distinct; class 1: 4 values (long runs across thread, wave and tile edges); class 2: 256 values with a NaN / -inf / zero tail"""
    r = np.random.RandomState(seed)
    scores = np.full((C, cap), CANARY_F, np.float32)
    targets = np.full((C, cap), CANARY_B, np.uint8)
    for c in range(C):
        kind = c % 3
        if kind == 0:
            s = (r.permutation(n).astype(np.float32) + 1.0) / np.float32(n + 1)
        elif kind == 1:
            s = _quantised(r, 1, n, 4)[0]
        else:
            s = _quantised(r, 1, n, 256)[0]
            special = r.rand(n)
            s = np.where(special < 0.02, np.float32(np.nan), np.where(special < 0.04, np.float32(-np.inf), np.where(special < 0.06, np.float32(-0.0), s)))
        scores[c, :n] = s
        targets[c, :n] = (r.rand(n) < (0.3, 0.05, 0.5)[kind]) * r.randint(1, 256, n)       # a positive is any nonzero byte
    return scores, targets


def _row_counts():
    return ['0', '1', '63', '64', '65', 'T-1', 'T', 'T+1', '2T+3']


@pytest.mark.parametrize('config', ['C1_K1', 'C3_K3_odd_cap', 'C3_K16_count_below_cap'])
@pytest.mark.parametrize('rows', _row_counts())
def test_bit_equal_at_every_row_count_and_alignment(rows, config):
    T = _tile()
    n = {'0': 0, '1': 1, '63': 63, '64': 64, '65': 65, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+3': 2 * T + 3}[rows]
    if config == 'C1_K1':
        C, crit, cap = 1, K1, max((n + 15) // 16 * 16, 16)
    elif config == 'C3_K3_odd_cap':                                                       # classes 1 and 2 start off any 16-byte boundary: scalar loads
        C, crit, cap = 3, K3, (n + 1) | 1
    else:
        C, crit, cap = 3, K16, (n + 15) // 16 * 16 + 48
    scores, targets = _mixed_stores(1000 + n, C, n, cap)
    thr, cut, tp, ok, stat = _checked(scores, targets, n, crit)
    if n >= 63 and config != 'C1_K1':
        assert int(ok.sum()) > 0 and len(set(cut.reshape(-1).tolist())) > 2               # (the criteria found different cuts)


def _runs_at(T, lo, hi, n):
    """descending scores, all distinct but for one run of equal values over rows lo .. hi - 1"""
    s = 1.0 - np.arange(n, dtype=np.float64) / (2.0 * n)
    s[lo:hi] = s[lo]
    return s.astype(np.float32)


@pytest.mark.parametrize('scores_kind', ['distinct', 'q4', 'q256', 'equal', 'tail', 'p0_pn', 'run_ends_at_T', 'run_spans_T'])
def test_score_sets(scores_kind):
    T = _tile()
    C, n = 3, 2 * T + 3
    cap = n + 14                                                                          # odd: classes 1 and 2 take the scalar loads
    r = np.random.RandomState(len(scores_kind) * 131 + 5)
    scores, targets = np.full((C, cap), CANARY_F, np.float32), np.full((C, cap), CANARY_B, np.uint8)
    targets[:, :n] = r.rand(C, n) < 0.2
    if scores_kind == 'distinct':
        scores[:, :n] = np.stack([(r.permutation(n).astype(np.float32) + 1.0) / np.float32(n + 1) for _ in range(C)])
    elif scores_kind in ('q4', 'q256'):
        scores[:, :n] = _quantised(r, C, n, 4 if scores_kind == 'q4' else 256)
        targets[:, :n] = r.rand(C, n) < 0.5 * scores[:, :n]                               # (scores that say something)
    elif scores_kind == 'equal':
        scores[:, :n] = np.float32(0.25)
    elif scores_kind == 'tail':                                                          # most positives sit behind m
        scores[:, :n] = r.rand(C, n).astype(np.float32)
        tail = r.rand(C, n) < 0.4
        scores[:, :n] = np.where(tail, np.where(r.rand(C, n) < 0.5, np.float32(np.nan), np.float32(-np.inf)), scores[:, :n])
        targets[:, :n] = np.where(tail, r.rand(C, n) < 0.9, r.rand(C, n) < 0.05)
    elif scores_kind == 'p0_pn':
        scores[:, :n] = _quantised(r, C, n, 256)
        targets[0, :n], targets[1, :n] = 0, 1
    else:
        lo, hi = (T - 100, T) if scores_kind == 'run_ends_at_T' else (T - 50, T + 50)
        for c in range(C):
            order = r.permutation(n)                                                      # the sort puts the run back in place
            scores[c, :n] = _runs_at(T, lo + c, hi, n)[order]                              # (class c: the run starts c rows later)
            targets[c, :n] = (r.rand(n) < 0.6 * _runs_at(T, lo + c, hi, n))[order]
    thr, cut, tp, ok, stat = _checked(scores, targets, n, K16)
    if scores_kind == 'equal':
        assert set(cut.reshape(-1).tolist()) <= {0, n} and stat[:, 1].tolist() == [n] * C
    if scores_kind == 'tail':
        assert int(stat[:, 1].max()) < n and int((ok[:, :10] == 0).sum()) > 0             # some recall level cannot be reached
    if scores_kind == 'p0_pn':
        assert stat[:2, 0].tolist() == [0, n] and int(ok[0].sum()) == 0 and cut[0].tolist() == [0] * 16 and bool(torch.isinf(thr[0]).all())
    if scores_kind.startswith('run_'):
        lo, hi = (T - 100, T) if scores_kind == 'run_ends_at_T' else (T - 50, T + 50)
        cuts = set(cut.reshape(-1).tolist())
        assert not any(lo + 2 < c < hi for c in cuts)                                    # no cut inside the run


def test_all_classes_of_the_task():
    r = np.random.RandomState(11)
    C, n, cap = 157, 200, 208
    scores, targets = np.full((C, cap), CANARY_F, np.float32), np.full((C, cap), CANARY_B, np.uint8)
    scores[:, :n] = _quantised(r, C, n, 64)
    targets[:, :n] = r.rand(C, n) < np.linspace(0.0, 0.6, C)[:, None]
    thr, cut, tp, ok, stat = _checked(scores, targets, n, [F1, ('recall', 0.2), ('recall', 0.5), ('recall', 0.8), ('precision', 0.5)])
    assert int((stat[:, 0] == 0).sum()) >= 1 and int(ok[:, 0].sum()) > 100
    assert bool((thr[:, 1] >= thr[:, 2]).all() and (thr[:, 2] >= thr[:, 3]).all())       # ascending recall: thresholds high to low


def _batch(seed, B=2, C=3, TL=65):
    r = np.random.RandomState(seed)
    probs = torch.from_numpy(_quantised(r, B * C, TL, 16).reshape(B, C, TL))
    labels = torch.from_numpy((r.rand(B, C, TL) < 0.15 + 0.6 * probs.numpy()).astype(np.float32))
    return probs, labels, torch.tensor([TL, TL - 25][:B], dtype=torch.int32)


def test_the_loop_closes_on_the_device():
    """meter -> thresholds -> decode: per class the frames decode activates are the cut, the positives among them the tp; no reference"""
    from apmeter import DeviceAPMeter
    from cfn_hip.calibrate import Calibration
    from cfn_hip.detections import decode
    probs, labels, valid = (t.to(DEV) for t in _batch(3))
    for spec in ('f1', 'recall:0.5', 'precision:0.6'):
        meter = DeviceAPMeter(DEV)
        meter.add_batch(probs, labels, valid)
        cal = Calibration(spec, 3, DEV, 0.5)
        assert cal.update(meter) is cal and cal.updates == 1
        det = decode(probs, valid, thr=cal.thr_vector)
        total = det.check()
        cls, active = det.seg[:total, 0].long(), det.frames[:total, 2].long()
        per_class = torch.zeros(3, dtype=torch.int64, device=DEV).index_add_(0, cls, active)
        on = (probs > cal.thr_vector[None, :, None]) & (torch.arange(probs.shape[2], device=DEV)[None, None, :] < valid[:, None, None])
        assert per_class.tolist() == cal.cut[:, 0].tolist() == on.sum((0, 2)).tolist(), spec
        assert (on & (labels != 0)).sum((0, 2)).tolist() == cal.tp[:, 0].tolist(), spec
        assert cal.stat[:, 0].tolist() == sum(labels[b, :, :int(valid[b])].sum(1) for b in range(2)).long().tolist()
        s = cal.summary()
        assert s['classes'] == 3 and s['criteria'][0]['ok'] == int(cal.ok.sum())
        if not spec.startswith('precision'):                                              # (every class has positives in front of m: both can be met)
            assert int(cal.ok.sum()) == 3 and int(cal.cut.min()) > 0 and 0.0 < s['criteria'][0]['f1'] <= 1.0, spec


def test_value_and_thresholds_is_value_device_and_calibrate():
    from apmeter import DeviceAPMeter
    from cfn_hip.calibrate import Calibration
    meter = DeviceAPMeter(DEV)
    for seed in (5, 6, 7):
        meter.add_batch(*(t.to(DEV) for t in _batch(seed, 2, 5, 200)))
    a, b = Calibration('recall:0.3,0.6,0.9', 5, DEV, (0.7, 0.5, 0.3)), Calibration('recall:0.3,0.6,0.9', 5, DEV, (0.7, 0.5, 0.3))
    ap = meter.value_and_thresholds(a)
    assert torch.equal(_bits(ap), _bits(meter.value_device())) and torch.equal(_bits(meter.value(b)), _bits(ap))
    c = Calibration('recall:0.3,0.6,0.9', 5, DEV, (0.7, 0.5, 0.3))
    meter.calibrate(c)
    for x in (a, b):
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(x.outputs, c.outputs))
    assert not torch.equal(c.thr.cpu(), torch.tensor([[0.7, 0.5, 0.3]] * 5)) and bool((c.thr[:, :-1] >= c.thr[:, 1:]).all())
    empty = DeviceAPMeter(DEV)
    with pytest.raises(RuntimeError, match='nothing was added'):
        empty.calibrate(c)
    assert empty.value(c) == 0 and c.updates == 1                                         # nothing added: the calibration is left alone


def test_step_metrics_report_calibrates_from_the_sort_behind_its_map():
    from cfn_hip.calibrate import Calibration
    from cfn_hip.metrics import StepMetrics
    tr = StepMetrics(device_ap=True, device=DEV)
    for seed in (8, 9):
        probs, labels, valid = (t.to(DEV) for t in _batch(seed, 2, 4, 120))
        tr.update(torch.tensor(0.5, device=DEV), torch.tensor(0.25, device=DEV), probs, labels, valid)
    a, b = Calibration('f1', 4, DEV, 0.5), Calibration('f1', 4, DEV, 0.5)
    assert tr.report(a) == tr.report() and a.updates == 1                                # the same losses and mAP, one more kernel
    assert tr.calibrate(b) is True and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a.outputs, b.outputs))
    assert not bool((a.thr == 0.5).all())
    tr.reset_ap()
    assert tr.calibrate(b) is False and tr.mean_ap(b) == 0.0 and b.updates == 1           # no rows since: the thresholds stay


@pytest.mark.capture
def test_sort_and_calibrate_replay_in_a_graph_on_other_rows():
    from apmeter import DeviceAPMeter
    from cfn_hip.calibrate import Calibration, thresholds_reference
    C, TL, cap = 4, 300, 1280
    meter = DeviceAPMeter(DEV, capacity=cap)
    cal = Calibration(K3, C, DEV, 0.5)
    cases = [[tuple(t.to(DEV) for t in _batch(20 + 10 * i + j, 2, C, TL)) for j in range(1 + i)] for i in range(2)]      # 1 batch, then 2: another count
    for batch in cases[0]:
        meter.add_batch(*batch)
    scores, targets = meter.stores
    bufs = (torch.empty_like(scores), torch.empty_like(targets), torch.empty(C, cap, dtype=torch.int32, device=DEV), torch.empty_like(targets))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meter.calibrate(cal, out=bufs)                                                    # warm-up outside the capture
    side.synchronize()
    before, held = torch.cuda.memory_stats()['allocation.all.allocated'], torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode('error')
    try:
        meter.calibrate(cal, out=bufs)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before and torch.cuda.memory_allocated() == held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        meter.calibrate(cal, out=bufs)
    seen = []
    for i, case in enumerate(cases):
        meter.reset()
        for batch in case:
            meter.add_batch(*batch)                                                       # the same stores, other rows, another count
        assert meter.stores[0].data_ptr() == scores.data_ptr()
        for o, v in zip(cal.outputs, (CANARY_F, CANARY_I, CANARY_I, CANARY_B, CANARY_I)):
            o.fill_(v)
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        graph.replay()
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
        torch.cuda.synchronize()
        n = int(meter.count)
        ref = thresholds_reference(bufs[0].cpu(), bufs[1].cpu(), n, K3)
        assert all(torch.equal(_bits(g), _bits(r)) for g, r in zip(cal.outputs, ref))
        seen.append((n, _bits(cal.thr).tolist()))
    assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]


# ---- end to end: the training scripts decode their validation phase with the thresholds their training phases calibrated ------------------
def _existing(lines):
    return [ln for ln in lines if 'calibrated' not in ln and 'seg-mAP' not in ln]


def test_train_fine_validates_with_the_calibrated_thresholds(tmp_path, monkeypatch):
    """run(calibration=..., device_ap=True) with a writer and a meter made with the calibration's thr_vector: the thresholds have left the
    typed value when the validation phase starts, the file equals decode_reference of the validation probs at the saved thresholds, and the
    losses and the existing lines are BIT-EQUAL to a run without any of it"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _run, _same_file
    from test_hip_segap import _spy_meter
    from cfn_hip.calibrate import Calibration
    from cfn_hip.detections import DetectionWriter, decode_reference, epoch_path
    from cfn_hip.seglabels import collate_seg
    crop, gap, mlen = 64, 2, 2
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.fine_collate_u8)
    cal = Calibration('f1', 157, DEV, 0.5)
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), cal.thr_vector, gap, mlen)
    meter = _spy_meter((0.1, 0.5), thr=cal.thr_vector, max_gap=gap, min_len=mlen)
    losses, lines, val = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, writer, max_epochs=4, save_model=str(tmp_path / 'm_'),
                              segment_ap=meter, calibration=cal, device_ap=True)
    assert cal.updates == 1 and [i for i, ln in enumerate(lines) if 'calibrated' in ln] == [0] and lines[0].startswith(' Epoch:4 calibrated ')
    thr = cal.thr_vector.cpu()
    summary = cal.summary()
    print('train_fine: %s; %d thresholds left 0.5' % (lines[0].strip(), int((thr != 0.5).sum())))
    assert bool((thr != 0.5).all()) and 0 < summary['classes'] < 157 and int((thr == float('inf')).sum()) == 157 - summary['classes']
    rows = []
    for i, (probs, valid) in enumerate(val):
        lab = collate_seg([_SegVideos(3, crop, False)[i][1]])
        det = decode_reference(probs, valid, lab.fps, lab.window[:, 0].contiguous(), thr, gap, mlen)
        rows.append({'video': 'vid%d' % i, 'unit': 's', 'segments': det.tolist()[0]})
    n = _same_file(epoch_path(writer.path, 4), rows)
    print('train_fine: %d segments in 3 validation videos at the calibrated thresholds' % n)
    losses0, lines0, _ = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / 'n_'))
    assert losses0 == losses and lines0 == _existing(lines) and len(lines) == len(lines0) + 2


def test_train_coarse_validates_with_the_calibrated_levels(tmp_path, monkeypatch):
    """the same through train_coarse_fineFEAT.run with K = 2 recall levels: the writer proposes at the calibrated (C, K) levels"""
    import torch.utils.data as tud
    import collate
    import train_coarse_fineFEAT as tc
    from test_hip_detections import _SegVideos, _run, _same_file
    from test_hip_segap import _spy_meter
    from cfn_hip.calibrate import Calibration
    from cfn_hip.detections import DetectionWriter, epoch_path, propose
    from cfn_hip.seglabels import collate_seg
    gap, mlen = 2, 2
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, 224, False, coarse=True), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.coarse_collate_u8)
    cal = Calibration('recall:0.4,0.8', 157, DEV, (0.6, 0.4))
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), 0.5, gap, mlen, levels=cal.levels, nms=0.5)
    meter = _spy_meter((0.1, 0.5), thr=0.5, max_gap=gap, min_len=mlen, levels=cal.levels, nms=0.5)
    losses, lines, val = _run(tc, monkeypatch, {'train': mk(2, 2), 'val': mk(2, 1)}, writer, max_epochs=2, save_model=str(tmp_path / 'm_'),
                              csv_path=str(tmp_path / 'a.csv'), segment_ap=meter, calibration=cal, device_ap=True)
    assert cal.updates == 1 and [i for i, ln in enumerate(lines) if 'calibrated' in ln] == [0] and lines[0].startswith(' Epoch:2 calibrated ')
    levels = cal.levels.cpu()
    assert not bool((levels == torch.tensor([0.6, 0.4])).any()) and bool((levels[:, 0] >= levels[:, 1]).all())
    rows = []
    for i, (probs, valid) in enumerate(val):
        lab = collate_seg([_SegVideos(2, 224, False, coarse=True)[i][1]])
        det = propose(probs, valid, lab.fps, lab.window[:, 0].contiguous(), levels, 0.5, 'max', gap, mlen, reference=True)
        rows.append({'video': 'vid%d' % i, 'unit': 's', 'segments': det.tolist()[0]})
    n = _same_file(epoch_path(writer.path, 2), rows)
    print('train_coarse_fineFEAT: %s; %d proposals in 2 validation videos at the calibrated levels' % (lines[0].strip(), n))
    losses0, lines0, _ = _run(tc, monkeypatch, {'train': mk(2, 2), 'val': mk(2, 1)}, None, max_epochs=2, save_model=str(tmp_path / 'n_'),
                              csv_path=str(tmp_path / 'b.csv'))
    assert losses0 == losses and lines0 == _existing(lines) and len(lines) == len(lines0) + 2


def test_train_fine_calibrates_where_it_logs_the_training_map(tmp_path, monkeypatch):
    """an epoch of two steps, so every step logs its mAP: each mAP line is followed by a calibrated line, the validation phase starts with an
    empty meter and decodes with the thresholds of the LAST interval, and the other lines and the losses equal a run without a calibration"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _run, _same_file
    from cfn_hip.calibrate import Calibration
    from cfn_hip.detections import DetectionWriter, decode_reference, epoch_path
    from cfn_hip.seglabels import collate_seg
    crop, gap, mlen = 64, 1, 1
    monkeypatch.setattr(train_fine, 'CHARADES_TR_SIZE', 4)                                # iters = 2: a line after every step
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.fine_collate_u8)
    cal = Calibration('recall:0.5', 157, DEV, 0.5)
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), cal.thr_vector, gap, mlen)
    losses, lines, val = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, writer, max_epochs=4, save_model=str(tmp_path / 'm_'),
                              calibration=cal, device_ap=True)
    assert cal.updates == 4 and len(lines) == 9
    assert all(' mAP: ' in lines[2 * i] and ' train ' in lines[2 * i] and lines[2 * i + 1].startswith(' Epoch:%d calibrated ' % (i + 1)) for i in range(4))
    thr = cal.thr_vector.cpu()
    assert bool((thr != 0.5).all())
    rows = []
    for i, (probs, valid) in enumerate(val):
        lab = collate_seg([_SegVideos(3, crop, False)[i][1]])
        det = decode_reference(probs, valid, lab.fps, lab.window[:, 0].contiguous(), thr, gap, mlen)
        rows.append({'video': 'vid%d' % i, 'unit': 's', 'segments': det.tolist()[0]})
    n = _same_file(epoch_path(writer.path, 4), rows)
    print('train_fine: %s; %d segments at the thresholds of the last interval' % (lines[7].strip(), n))
    losses0, lines0, _ = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / 'n_'), device_ap=True)
    assert losses0 == losses and lines0 == _existing(lines) and len(lines0) == 5


def test_a_leftover_does_not_replace_the_thresholds_of_a_whole_interval(tmp_path, monkeypatch):
    """an epoch of six steps: the mAP line behind step 3 calibrates; step 4 leaves one batch in the meter when the validation phase starts,
    and that leftover is NOT calibrated from, because the thresholds were updated since the last validation phase"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _run
    from cfn_hip.calibrate import Calibration
    from cfn_hip.detections import DetectionWriter
    monkeypatch.setattr(train_fine, 'CHARADES_TR_SIZE', 12)                               # iters = 6: a line after every third step
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, 64, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.fine_collate_u8)
    cal = Calibration('f1', 157, DEV, 0.5)
    kept = []
    real = cal.summary_line
    monkeypatch.setattr(cal, 'summary_line', lambda: (kept.append(cal.thr.clone()), real())[1])
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), cal.thr_vector, 1, 1)
    losses, lines, val = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, writer, max_epochs=4, save_model=str(tmp_path / 'm_'),
                              calibration=cal, device_ap=True)
    assert cal.updates == 1 and len(kept) == 1 and torch.equal(_bits(kept[0]), _bits(cal.thr))
    assert len(lines) == 3 and ' steps: 3 ' in lines[0] and lines[1].startswith(' Epoch:3 calibrated ') and ' val ' in lines[2]
