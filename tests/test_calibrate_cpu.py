"""Per-class decode thresholds from sorted AP rows, host side (cfn_hip/calibrate.py): thresholds_reference on hand-written cases with the
expected (cut, tp, thr, ok) typed out, its properties on random small inputs (the thresholds reproduce the cuts under decode's strict
compare, the f1 cut against a brute force in exact fractions, the order of recall levels, the precision cut), parse_criteria, the
Calibration's JSON round trip, the C ABI of cfn_ap_calibrate, the refusals of the op, and the scripts' new flag.  Every comparison is exact:
the rule holds integers, fp32 copies and one fp64 product.  No GPU."""
import argparse
import ctypes
import fractions
import os
import re

import numpy as np
import pytest
import torch

INF = float('inf')
NAN = float('nan')


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _one(scores, targets, criteria, count=None):
    """thresholds_reference of ONE class -> ([(cut, tp, thr, ok) per criterion], [P, m])"""
    from cfn_hip.calibrate import thresholds_reference
    s, g = np.asarray([scores], np.float32), np.asarray([targets], np.uint8)
    thr, cut, tp, ok, stat = thresholds_reference(s, g, len(scores) if count is None else count, criteria)
    return [(int(cut[0, k]), int(tp[0, k]), float(thr[0, k]), int(ok[0, k])) for k in range(len(criteria))], stat[0].tolist()


F1, f32 = ('f1', None), lambda x: float(np.float32(x))


def test_a_clean_separation():
    got, stat = _one([0.9, 0.8, 0.7, 0.3, 0.2, 0.1], [1, 1, 1, 0, 0, 0], [F1, ('precision', 1.0), ('recall', 1.0), ('precision', 0.5), ('recall', 0.5)])
    assert stat == [3, 6]
    assert got == [(3, 3, f32(0.3), 1), (3, 3, f32(0.3), 1), (3, 3, f32(0.3), 1), (6, 3, -INF, 1), (2, 2, f32(0.7), 1)]


def test_ties_move_the_cut_to_the_edge_of_the_run():
    # the unconstrained best cut is r = 3 (F1 = 1), inside the run of 0.5: the admissible cuts are 1, 4 and 5
    got, _ = _one([0.9, 0.5, 0.5, 0.5, 0.1], [1, 1, 1, 0, 0], [F1, ('recall', 0.5), ('precision', 0.9)])
    assert got == [(4, 3, f32(0.1), 1), (4, 3, f32(0.1), 1), (1, 1, f32(0.5), 1)]
    # r = 1 and r = 4 tie exactly (2/3 = 4/6): the smaller r
    got, _ = _one([0.9, 0.5, 0.5, 0.5, 0.1], [1, 1, 0, 0, 0], [F1])
    assert got == [(1, 1, f32(0.5), 1)]


def test_all_scores_equal_only_the_whole_row_is_admissible():
    got, stat = _one([0.4] * 4, [1, 0, 1, 0], [F1, ('precision', 0.6), ('precision', 0.5), ('recall', 0.5)])
    assert stat == [2, 4]
    assert got == [(4, 2, -INF, 1), (0, 0, INF, 0), (4, 2, -INF, 1), (4, 2, -INF, 1)]


def test_no_positive_and_only_positives():
    got, stat = _one([0.9, 0.5], [0, 0], [F1, ('precision', 0.5), ('recall', 0.5)])
    assert stat == [0, 2] and got == [(0, 0, INF, 0)] * 3
    got, stat = _one([0.9, 0.5, 0.2], [1, 1, 1], [F1, ('precision', 1.0), ('recall', 0.5)])
    assert stat == [3, 3] and got == [(3, 3, -INF, 1), (3, 3, -INF, 1), (2, 2, f32(0.2), 1)]
    got, stat = _one([], [], [F1, ('recall', 1.0)])
    assert stat == [0, 0] and got == [(0, 0, INF, 0)] * 2


def test_positives_behind_m_count_in_p_and_can_make_recall_unreachable():
    got, stat = _one([0.8, 0.6, -INF, NAN], [1, 0, 1, 1], [('recall', 0.9), ('recall', 0.3), F1, ('precision', 0.5)])
    assert stat == [3, 2]
    assert got == [(2, 1, -INF, 0), (1, 1, f32(0.6), 1), (1, 1, f32(0.6), 1), (2, 1, -INF, 1)]
    got, stat = _one([-INF, NAN], [1, 1], [('recall', 0.5), F1])            # m == 0: nothing can be active
    assert stat == [2, 0] and got == [(0, 0, INF, 0)] * 2
    got, stat = _one([0.9, 0.5, 0.1], [1, 0, 1], [('recall', 1.0)], count=2)      # the rows behind count do not exist
    assert stat == [1, 2] and got == [(1, 1, f32(0.5), 1)]


def test_the_two_zeros_are_one_score():
    got, _ = _one([0.5, 0.0, -0.0, -1.0], [1, 1, 0, 0], [F1, ('recall', 1.0), ('precision', 1.0)])
    assert got == [(3, 2, -1.0, 1), (3, 2, -1.0, 1), (1, 1, 0.0, 1)]
    got, _ = _one([0.5, -0.0, 0.0, -1.0], [1, 1, 0, 0], [('recall', 1.0)])
    assert got == [(3, 2, -1.0, 1)]


def test_a_precision_that_is_never_reached():
    got, _ = _one([0.9, 0.8, 0.7], [0, 0, 1], [('precision', 0.9), ('precision', 1.0 / 3.0)])
    assert got[0] == (0, 0, INF, 0)
    assert got[1] == (3, 1, -INF, 1)                                        # (double)1 >= (1/3 as a double) * 3.0


# ---- properties on random small inputs -------------------------------------------------------------------------------------------------
def _random_class(r):
    """one sorted class of n <= 40 rows with heavy ties and special values, as ap_sort leaves it: descending, -0.0 as +0.0, NaN last"""
    n = int(r.randint(0, 41))
    pool = np.asarray([0.9, 0.75, 0.5, 0.5, 0.25, 0.0, -0.0, 1e-40, -1.5, INF, -INF, NAN, 0.3], np.float32)[:int(r.randint(2, 14))]
    s = pool[r.randint(0, len(pool), n)] if r.rand() < 0.7 else r.rand(n).astype(np.float32)
    g = (r.rand(n) < r.choice([0.0, 0.1, 0.5, 1.0])).astype(np.uint8)
    s = np.where(s == 0, np.float32(0.0), s)
    with np.errstate(invalid='ignore'):
        order = np.argsort(-s, kind='stable')
    return s[order], g[order]


def _distinct_thresholds(s):
    """every threshold that gives a different active set under the strict compare: +inf, every score value (NaN excepted), -inf"""
    return [np.float32(INF)] + [np.float32(v) for v in sorted({float(x) for x in s if not np.isnan(x)}, reverse=True)] + [np.float32(-INF)]


def _active(s, g, thr):
    with np.errstate(invalid='ignore'):
        on = s > np.float32(thr)
    return int(on.sum()), int((g[on] != 0).sum())


def test_properties_on_random_small_inputs():
    r = np.random.RandomState(7)
    crit = [F1, ('precision', 0.5), ('precision', 0.8), ('recall', 0.2), ('recall', 0.5), ('recall', 0.8), ('recall', 1.0)]
    seen_special = 0
    for _ in range(1500):
        s, g = _random_class(r)
        got, (P, m) = _one(s, g, crit)
        assert P == int((g != 0).sum())
        seen_special += m < len(s)
        for cut, tp, thr, ok in got:                                        # decode's strict compare reproduces the cut and its positives
            assert _active(s, g, thr) == (cut, tp)
        points = [_active(s, g, t) for t in _distinct_thresholds(s)]        # (rows active, positives among them) of every distinct threshold
        f = lambda p: fractions.Fraction(2 * p[1], p[0] + P) if p[0] + P else fractions.Fraction(0)
        best = max(f(p) for p in points)
        assert got[0][0] == min(p[0] for p in points if f(p) == best) and got[0][3] == (1 if best > 0 else 0)
        for k in (1, 2):                                                    # precision: the largest row count among ALL distinct thresholds
            fits = [p[0] for p in points if p[0] > 0 and float(p[1]) >= crit[k][1] * float(p[0])]
            assert got[k][0] == (max(fits) if fits else 0) and got[k][3] == (1 if fits else 0)
        for k in (3, 4, 5, 6):                                              # recall: the smallest, or everything when it cannot be reached
            fits = [p[0] for p in points if P > 0 and p[0] > 0 and float(p[1]) >= crit[k][1] * float(P)]
            assert got[k][0] == (min(fits) if fits else (m if P > 0 else 0)) and got[k][3] == (1 if fits else 0)
        thrs = [got[k][2] for k in (3, 4, 5, 6)]                            # ascending recall: thresholds high to low (rule N2's level order)
        assert all(a >= b for a, b in zip(thrs, thrs[1:]))
    assert seen_special > 100


def test_reference_over_several_classes_and_its_refusals():
    from cfn_hip.calibrate import thresholds_reference
    r = np.random.RandomState(3)
    rows = [_random_class(r) for _ in range(40)]
    rows = [(s, g) for s, g in rows if len(s) >= 12][:5]
    s, g = np.stack([a[:12] for a, _ in rows]), np.stack([b[:12] for _, b in rows])
    crit = [F1, ('recall', 0.5)]
    thr, cut, tp, ok, stat = thresholds_reference(torch.from_numpy(s), torch.from_numpy(g), torch.tensor([12], dtype=torch.int32), crit)
    assert tuple(thr.shape) == (5, 2) and thr.dtype == torch.float32 and cut.dtype == tp.dtype == stat.dtype == torch.int32 and ok.dtype == torch.uint8
    for c in range(5):
        one, st = _one(s[c], g[c], crit)
        assert [(int(cut[c, k]), int(tp[c, k]), int(ok[c, k])) for k in range(2)] == [(o[0], o[1], o[3]) for o in one] and stat[c].tolist() == st
        assert thr[c].numpy().view(np.int32).tolist() == np.asarray([o[2] for o in one], np.float32).view(np.int32).tolist()
    with pytest.raises(ValueError, match='float32'):
        thresholds_reference(s.astype(np.float64), g, 12, crit)
    with pytest.raises(ValueError, match='unknown kind'):
        thresholds_reference(s, g, 12, [('fbeta', 0.5)])


def test_parse_criteria_and_its_refusals():
    from cfn_hip.calibrate import parse_criteria, check_criteria, criteria_tensors
    assert parse_criteria('f1') == [('f1', None)]
    assert parse_criteria('precision:0.5') == [('precision', 0.5)]
    assert parse_criteria(' recall:0.2, 0.4,0.6,0.8 ') == [('recall', 0.2), ('recall', 0.4), ('recall', 0.6), ('recall', 0.8)]
    assert len(parse_criteria('recall:' + ','.join(['0.5'] * 16))) == 16
    for spec, word in (('recall:' + ','.join(['0.5'] * 17), '1 to 16'), ('recall:0', r'\(0, 1\]'), ('recall:1.5', r'\(0, 1\]'), ('precision:-0.1', r'\(0, 1\]'),
                       ('precision:nan', r'\(0, 1\]'), ('fbeta:2', 'unknown kind'), ('', 'expected'), ('f1:0.5', 'no value'), ('recall', 'needs'),
                       ('recall:', 'needs'), ('recall:0.5,,0.6', 'needs'), ('precision:high', 'numbers'), (None, 'expected')):
        with pytest.raises(ValueError, match=word):
            parse_criteria(spec)
    with pytest.raises(ValueError, match='pairs'):
        check_criteria(['f1'])
    with pytest.raises(ValueError, match='1 to 16'):
        check_criteria([])
    kinds, values = criteria_tensors([('f1', None), ('precision', 0.5), ('recall', 1)])
    assert kinds.dtype == torch.int32 and kinds.tolist() == [0, 1, 2] and values.dtype == torch.float64 and values.tolist() == [0.0, 0.5, 1.0]


def test_calibration_holds_the_typed_values_first_and_round_trips_its_bits(tmp_path):
    from cfn_hip.calibrate import Calibration
    cal = Calibration('f1', 5, 'cpu', 0.35)
    assert tuple(cal.thr.shape) == (5, 1) and cal.thr_vector.tolist() == [f32(0.35)] * 5 and cal.thr_vector.is_contiguous()
    assert cal.thr_vector.data_ptr() == cal.thr.data_ptr() == cal.levels.data_ptr() and cal.n_criteria == 1 and cal.updates == 0
    lv = Calibration('recall:0.2,0.5,0.8', 4, 'cpu', (0.8, 0.5, 0.2))
    assert lv.levels.tolist() == [[f32(0.8), f32(0.5), f32(0.2)]] * 4 and lv.kinds.tolist() == [2, 2, 2] and lv.values.tolist() == [0.2, 0.5, 0.8]
    with pytest.raises(ValueError, match='thr_vector'):
        lv.thr_vector
    with pytest.raises(ValueError, match='initial'):
        Calibration('recall:0.2,0.5', 4, 'cpu', (0.8, 0.5, 0.2))
    with pytest.raises(ValueError, match='n_classes'):
        Calibration('f1', 0, 'cpu')
    bits = np.asarray([[0x7f800000, 0xff800000 - (1 << 32), 1], [0x3eb33333, 0x00000001, 0x3f7fffff], [0, 0x00800000, 0x7f7fffff], [5, 6, 7]], np.int32)
    lv.thr.copy_(torch.from_numpy(bits).view(torch.float32))                  # +inf, -inf, denormals: what an update can leave
    path = lv.save(str(tmp_path / 'cal.json'))
    back = Calibration.load(path, 'cpu')
    assert back.criteria == lv.criteria and back.n_classes == 4 and back.initial == lv.initial
    assert back.thr.view(torch.int32).tolist() == bits.tolist()
    s = lv.summary()                                                          # nothing was updated: no class, no row
    assert s['classes'] == 0 and s['n_classes'] == 4 and [r['kind'] for r in s['criteria']] == ['recall'] * 3 and all(r['ok'] == 0 and r['f1'] == 0.0 for r in s['criteria'])
    lv.stat.copy_(torch.tensor([[4, 9], [0, 9], [2, 9], [2, 9]], dtype=torch.int32))
    lv.cut[:, 0] = torch.tensor([2, 0, 1, 1], dtype=torch.int32)
    lv.tp[:, 0] = torch.tensor([2, 0, 1, 0], dtype=torch.int32)
    lv.ok[:, 0] = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    s = lv.summary()
    assert s['classes'] == 3 and s['criteria'][0] == {'kind': 'recall', 'value': 0.2, 'ok': 2, 'precision': 3 / 4, 'recall': 3 / 8, 'f1': 6 / 12}
    assert lv.summary_line().startswith('calibrated 3/4 classes: recall:0.2 ok 2 P 0.7500 R 0.3750 F1 0.5000 recall:0.5 ok 0 ')


def test_entry_points_are_declared_exported_and_check_their_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    ret, at, dts = protos['cfn_ap_calibrate']
    assert ret is ctypes.c_int and len(at) == 14 and at[10:12] == [ctypes.c_int] * 2 and at[12] is ctypes.c_long and at[13] is ctypes.c_void_p
    assert dts[:10] == [torch.float32, torch.uint8, torch.int32, torch.int32, torch.float64, torch.float32, torch.int32, torch.int32, torch.uint8, torch.int32]
    assert protos['cfn_ap_calibrate_tile'][:2] == (ctypes.c_int, [])
    raw = ctypes.CDLL(cfn_hip.LIB_PATH)
    assert hasattr(raw, 'cfn_ap_calibrate') and hasattr(raw, 'cfn_ap_calibrate_tile')
    lib = cfn_hip.load()
    from cfn_hip import ops
    assert lib.cfn_ap_calibrate_tile() == ops.AP_CALIBRATE_TILE == 8192
    buf = (ctypes.c_double * 8)()
    p = [ctypes.addressof(buf)] * 10
    assert lib.cfn_ap_calibrate(*([None] * 10), 157, 1, 1024, None) == 1 and 'null' in cfn_hip.last_error()
    for hole in range(10):                                                   # every pointer is checked
        assert lib.cfn_ap_calibrate(*[None if i == hole else p[i] for i in range(10)], 157, 1, 1024, None) == 1 and 'null' in cfn_hip.last_error()
    for C, K, cap, word in ((0, 1, 8, 'C in'), (-1, 1, 8, 'C in'), (65536, 1, 8, 'C in'), (157, 0, 8, 'K in'), (157, 17, 8, 'K in'), (157, 1, 0, 'cap'),
                            (157, 1, -5, 'cap'), (157, 1, 1 << 31, 'cap')):
        assert lib.cfn_ap_calibrate(*p, C, K, cap, None) == 1, (C, K, cap)   # refused before any launch
        assert 'cfn_ap_calibrate' in cfn_hip.last_error() and word in cfn_hip.last_error(), cfn_hip.last_error()
    src = open(os.path.join(os.path.dirname(cfn_hip.LIB_PATH), '..', 'csrc', 'apcal.hip')).read()
    assert 'getenv' not in src and re.search(r'atomic[A-Z_]|__hip_atomic', src) is None and 'hipMalloc' not in src and 'Synchronize' not in src


def test_the_op_and_the_meters_refuse_what_they_cannot_do():
    _lib()
    from cfn_hip import ops, torchlib as tl
    from cfn_hip.calibrate import Calibration, criteria_tensors
    from cfn_hip.metrics import StepMetrics
    kinds, values = criteria_tensors([('f1', None)])
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.ap_calibrate(torch.zeros(3, 8), torch.zeros(3, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), kinds, values)
    assert not any('calibrate' in n for tup in (tl.OPERATORS, tl.INPUT_OPERATORS, tl.AUGMENT_OPERATORS, tl.METRIC_OPERATORS, tl.FEATURE_OPERATORS,
                                                tl.DECODE_OPERATORS, tl.LABEL_OPERATORS) for n in tup)      # C ABI only
    cal = Calibration('f1', 3, 'cpu')
    host = StepMetrics(device_ap=False)
    for call in (host.report, host.mean_ap, host.calibrate):
        with pytest.raises(RuntimeError, match='device_ap=True'):
            call(cal)
    assert host.report()[2] == 0.0                                           # without one: as before


def test_scripts_take_and_forward_the_calibrate_flag():
    import train_coarse_fineFEAT as tc
    import train_fine
    import inspect
    from cfn_hip.detections import DetectionWriter

    def parser():
        p = argparse.ArgumentParser()
        p.add_argument('--device-ap', action='store_true')
        train_fine.add_detect_args(p)
        train_fine.seg_ap_arguments(p)
        return p
    off = parser().parse_args(['--detect', 'd.jsonl'])
    assert off.detect_calibrate is None and train_fine.calibration_from_args(off) is None and '--detect-calibrate' not in train_fine.detect_argv(off)
    on = parser().parse_args(['--device-ap', '--detect', 'd.jsonl', '--detect-thr', '0.4', '--detect-calibrate', 'f1'])
    again = parser().parse_args(['--device-ap'] + train_fine.detect_argv(on))      # what a spawned worker parses
    assert vars(again) == vars(on) and again.detect_calibrate == 'f1'
    cal = train_fine.calibration_from_args(on, n_classes=6, device='cpu')
    assert cal.criteria == [('f1', None)] and cal.thr_vector.tolist() == [f32(0.4)] * 6
    assert train_fine.calibration_from_args(on) is cal                             # ONE per args: the writer, the meter and run() share the tensor
    w = train_fine.detect_writer(on)
    assert isinstance(w, DetectionWriter) and w.thr.data_ptr() == cal.thr.data_ptr() and w.levels is None and w.n_levels == 1
    lv = parser().parse_args(['--device-ap', '--detect', 'd.jsonl', '--detect-levels', '0.8,0.5,0.2', '--detect-nms', '0.4', '--detect-calibrate', 'recall:0.2,0.5,0.8'])
    assert vars(parser().parse_args(['--device-ap'] + train_fine.detect_argv(lv))) == vars(lv)
    cal = train_fine.calibration_from_args(lv, n_classes=6, device='cpu')
    assert cal.n_criteria == 3 and cal.levels.tolist() == [[f32(0.8), f32(0.5), f32(0.2)]] * 6
    w = train_fine.detect_writer(lv)
    assert w.levels is cal.levels and w.n_levels == 3 and w.nms == 0.4             # K > 1 goes through propose: --detect-nms applies as before
    other = train_fine.detect_writer(lv, train_fine.calibration_from_args(parser().parse_args(['--device-ap'] + train_fine.detect_argv(lv)), 6, 'cpu'))
    assert other.levels is not cal.levels and other.levels.tolist() == cal.levels.tolist()      # an explicit calibration is taken as given
    for argv, word in ((['--detect', 'd.jsonl', '--detect-calibrate', 'f1'], '--device-ap'),
                       (['--device-ap', '--detect-calibrate', 'recall:0.2,0.5'], '--detect-levels'),
                       (['--device-ap', '--detect-levels', '0.8,0.5,0.2', '--detect-calibrate', 'recall:0.2,0.5'], '--detect-levels'),
                       (['--device-ap', '--detect-levels', '0.8,0.5', '--detect-calibrate', 'f1'], '--detect-levels'),
                       (['--device-ap', '--detect-calibrate', 'fbeta:2'], 'unknown kind')):
        with pytest.raises(ValueError, match=word):
            train_fine.calibration_from_args(parser().parse_args(argv), device='cpu')
    with pytest.raises(RuntimeError, match='--device-ap'):                          # run() itself, before anything is built
        train_fine.run(calibration=cal, device_ap=False)
    with pytest.raises(RuntimeError, match='--device-ap'):
        tc.run(calibration=cal, device_ap=False)
    assert tc.detect_writer is train_fine.detect_writer and tc.calibration_from_args is train_fine.calibration_from_args
    for mod in (train_fine, tc):
        src = inspect.getsource(mod.run)
        assert 'tr.mean_ap(calibration)' in src and 'tr.calibrate(calibration)' in src and inspect.signature(mod.run).parameters['calibration'].default is None


def test_the_calibration_is_made_on_the_ranks_own_device(monkeypatch):
    """a worker builds its Calibration in front of run(), where the current device is still cuda:0 on every rank: the device comes from
    LOCAL_RANK as cfn_hip.dist.init_from_env takes it (CFN_SHARE_GPU: modulo the device count)"""
    import train_fine
    import cfn_hip.calibrate
    from cfn_hip import dist as cdist
    assert cdist.local_device() == torch.device('cpu') or torch.cuda.is_available()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 4)
    monkeypatch.delenv('CFN_SHARE_GPU', raising=False)
    monkeypatch.delenv('LOCAL_RANK', raising=False)
    assert cdist.local_device() == torch.device('cuda', 0)
    monkeypatch.setenv('LOCAL_RANK', '2')
    assert cdist.local_device() == torch.device('cuda', 2)
    made = []

    class Spy(object):
        def __init__(self, criteria, n_classes, device, initial):
            made.append((criteria, n_classes, device, initial))
    monkeypatch.setattr(cfn_hip.calibrate, 'Calibration', Spy)
    p = argparse.ArgumentParser()
    p.add_argument('--device-ap', action='store_true')
    train_fine.add_detect_args(p)
    args = p.parse_args(['--device-ap', '--detect', 'd.jsonl', '--detect-calibrate', 'f1'])
    cal = train_fine.calibration_from_args(args)
    assert isinstance(cal, Spy) and made == [([('f1', None)], 157, torch.device('cuda', 2), 0.5)]
    monkeypatch.setenv('LOCAL_RANK', '5')
    monkeypatch.setenv('CFN_SHARE_GPU', '1')
    assert cdist.local_device() == torch.device('cuda', 1)
    import inspect
    assert 'local % torch.cuda.device_count()' in inspect.getsource(cdist.init_from_env)      # the rule local_device repeats
    for mod in (train_fine, __import__('train_coarse_fineFEAT')):
        assert 'check_calibration(calibration, device_ap, dev)' in inspect.getsource(mod.run), mod.__name__


def test_a_calibration_on_another_device_or_beside_typed_levels_is_refused():
    import train_fine
    from cfn_hip.calibrate import Calibration
    cal = Calibration('f1', 4, 'cpu')
    train_fine.check_calibration(cal, True, torch.device('cpu'))
    with pytest.raises(RuntimeError, match='local_device'):
        train_fine.check_calibration(cal, True, torch.device('cuda', 1))
    assert train_fine._calibrated(0.5, {}, None) == (0.5, {})
    thr, more = train_fine._calibrated(0.5, {}, cal)
    assert thr.data_ptr() == cal.thr.data_ptr() and more == {}
    with pytest.raises(ValueError, match='--detect-levels'):
        train_fine._calibrated(0.5, {'levels': [0.6, 0.4], 'nms': None, 'nms_score': 'max'}, cal)
    p = argparse.ArgumentParser()
    p.add_argument('--device-ap', action='store_true')
    train_fine.add_detect_args(p)
    with pytest.raises(ValueError, match='--detect-levels'):                              # an explicit calibration is checked like the flag's own
        train_fine.detect_writer(p.parse_args(['--detect', 'd.jsonl', '--detect-levels', '0.6,0.4']), cal)


def test_initial_takes_any_real_scalar_and_says_what_it_wants():
    from cfn_hip.calibrate import Calibration
    for x in (np.float32(0.25), np.float64(0.25), torch.tensor(0.25), 0.25, fractions.Fraction(1, 4)):
        assert Calibration('recall:0.2,0.5', 3, 'cpu', x).thr.tolist() == [[0.25, 0.25]] * 3
    assert Calibration('recall:0.2,0.5', 3, 'cpu', np.asarray([0.5, 0.25], np.float32)).thr.tolist() == [[0.5, 0.25]] * 3
    assert Calibration('recall:0.2,0.5', 3, 'cpu', torch.tensor([0.5, 0.25])).thr.tolist() == [[0.5, 0.25]] * 3
    for bad in (None, 'half', True, (0.5,), object()):
        with pytest.raises(ValueError, match='initial'):
            Calibration('recall:0.2,0.5', 3, 'cpu', bad)
