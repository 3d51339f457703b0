"""Segment-level AP at temporal-IoU thresholds, on the host: the rules of cfn_hip/segap.py as match_reference / ap_reference spell them (hand
cases worked out in the docstrings, edge inputs, the identity, the golden annotation records), the C ABI of the cfn_segap_* entry points,
the refusals of the ops and the scripts' signatures.  No GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import segap_fixture as fx

W100 = [[0, 100]]


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _one(dets, gts, tiou=(0.5,), score_col=0, C=1, fps=1.0, window=(0, 100)):
    """ONE video -> the reference's dict"""
    from cfn_hip.segap import ap_reference
    det, gt = fx.make_det([dets], C), fx.make_gt([gts], [fps], [list(window)], C)
    return ap_reference([(det, gt)], C, tiou, score_col)


def test_true_false_true_gives_the_worked_out_ap():
    """one class, rows (0, 10) and (20, 30); detections by score: (0, 10) 0.9 TP at rank 1, (50, 60) 0.8 FP at rank 2, (20, 30) 0.7 TP at
    rank 3: AP = (1/1 + 2/3) / 2"""
    r = _one([(0, 0, 10, 0.9, 0), (0, 20, 30, 0.7, 0), (0, 50, 60, 0.8, 0)], [(0, 0, 10), (0, 20, 30)])
    tp, match, n_gt = r['batches'][0]
    assert tp.tolist() == [1, 1, 0] and match.tolist() == [[0, 1, -1]] and n_gt.tolist() == [2]
    assert r['ap'].dtype == np.float32 and r['ap'].shape == (1, 1)
    assert r['ap'][0, 0] == np.float32((1.0 / 1.0 + 2.0 / 3.0) / 2.0) and r['map'][0] == r['ap'][0, 0]
    assert r['scores'][0].tolist() == [np.float32(0.9), np.float32(0.7), np.float32(0.8)] and r['tps'][0].tolist() == [1, 1, 0]


def test_best_tiou_first_differs_from_first_found_first():
    """rows g0 (0, 10), g1 (2, 12) at 0.5.  (2, 12) 0.9 comes first: tIoU 8/12 with g0, 1 with g1 -> it takes g1 (first-found would take g0).
    (-4, 8) 0.8 then takes g0 at 8/14; with g0 gone it would be a false positive, as g1 gives 6/16.  AP 1 instead of 1/2."""
    r = _one([(0, 2, 12, 0.9, 0), (0, -4, 8, 0.8, 0)], [(0, 0, 10), (0, 2, 12)])
    tp, match, _ = r['batches'][0]
    assert tp.tolist() == [1, 1] and match.tolist() == [[0, 1]]              # rows by start: (-4, 8) is row 0 and takes g0
    assert r['ap'][0, 0] == np.float32(1.0)


def test_a_tiou_tie_goes_to_the_lowest_row():
    r = _one([(0, 0, 10, 0.9, 0)], [(0, 0, 10), (0, 0, 10)])
    assert r['batches'][0][1].tolist() == [[0]] and r['ap'][0, 0] == np.float32(0.5)          # one of two rows found
    r = _one([(0, 0, 10, 0.9, 0), (0, 0, 10, 0.6, 0)], [(0, 5, 6), (0, 0, 10), (0, 0, 10)], C=1)
    assert r['batches'][0][1].tolist() == [[1, 2]]


def test_a_score_tie_goes_to_the_lowest_detection_row():
    """(0, 10) and (1, 10), both 0.5, one row (0, 10): the lower row is taken first and takes the row; the other, which alone would match at
    9/10, is a false positive.  With the mean column (0.1 < 0.2) the order turns round."""
    dets = [(0, 0, 10, 0.5, 0.1), (0, 1, 10, 0.5, 0.2)]
    r = _one(dets, [(0, 0, 10)])
    assert r['batches'][0][0].tolist() == [1, 0] and r['ap'][0, 0] == np.float32(1.0)
    r = _one(dets, [(0, 0, 10)], score_col=1)
    assert r['batches'][0][0].tolist() == [0, 1] and r['ap'][0, 0] == np.float32(1.0) and r['scores'][0].tolist() == [np.float32(0.1), np.float32(0.2)]


def test_bit_k_is_threshold_k_and_thresholds_are_independent():
    """row (0, 10); (0, 8) 0.9 has tIoU 0.8, (0, 10) 0.8 has 1: at 0.5 and 0.8 the first takes the row; at 0.9 it cannot, and the second does"""
    r = _one([(0, 0, 8, 0.9, 0)], [(0, 0, 10)], tiou=(0.5, 0.8, 0.9))
    assert r['batches'][0][0].tolist() == [0b011]
    r = _one([(0, 0, 8, 0.9, 0), (0, 0, 10, 0.8, 0)], [(0, 0, 10)], tiou=(0.5, 0.8, 0.9))
    tp, match, _ = r['batches'][0]
    assert sorted(tp.tolist()) == [0b011, 0b100]
    assert r['ap'][:, 0].tolist() == [1.0, 1.0, 0.5]


def test_window_clip_and_rows_that_do_not_participate():
    from cfn_hip.segap import clip_reference, match_reference
    gt = fx.make_gt([[(0, 200, 300), (0, 90, 150), (0, 70, 70), (0, 80, 75), (7, 0, 10), (0.5, 0, 10), (-1, 0, 10), (float('nan'), 0, 10), (0, -5, 3)]],
                    [1.0], W100, 2)
    part, sp, ep, vid = clip_reference(gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, 2)
    assert part.tolist() == [False, True, False, False, False, False, False, False, True]
    assert (sp[1], ep[1]) == (90.0, 99.5) and (sp[8], ep[8]) == (-0.5, 3.0) and vid.tolist() == [0] * 9
    det = fx.make_det([[(0, 90, 99.5, 0.9, 0), (0, 200, 300, 0.8, 0)]], 2)
    tp, match, n_gt = match_reference(det, gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, (0.5, 1.0))
    assert n_gt.tolist() == [2, 0] and tp.tolist() == [3, 0] and match.tolist() == [[1, -1], [1, -1]]       # the clipped row is matched at tIoU 1
    empty = fx.make_gt([[(0, 0, 10)]], [1.0], [[0, 0]], 2, t_max=100)                              # a window without a frame: n = 0
    assert clip_reference(empty.seg, empty.offsets, empty.fps, empty.window, 100, 2)[0].tolist() == [False]
    short = fx.make_gt([[(0, 0, 10), (0, 8, 20)]], [1.0], [[0, 100]], 2, t_max=8)                  # t_max clamps the window's length
    part, sp, ep, _ = clip_reference(short.seg, short.offsets, short.fps, short.window, 8, 2)
    assert part.tolist() == [True, False] and ep[0] == 7.5


def test_videos_without_ground_truth_and_ground_truth_without_detections():
    from cfn_hip.segap import ap_reference
    det = fx.make_det([[(0, 0, 10, 0.9, 0)], [(0, 0, 10, 0.95, 0), (1, 0, 10, 0.5, 0)]], 3)
    gt = fx.make_gt([[(0, 0, 10), (2, 5, 9)], []], [1.0, 1.0], W100 * 2, 3)
    r = ap_reference([(det, gt)], 3)
    assert r['n_gt'].tolist() == [1, 0, 1] and r['counts'].tolist() == [2, 1, 0]
    assert [t.tolist() for t in r['tps']] == [[31, 0], [0], []]
    assert r['ap'][:, 0].tolist() == [0.5] * 5                     # the false positive of video 1 ranks first
    assert r['ap'][:, 1].tolist() == [0.0] * 5                     # no ground truth: 0, and not in the mean
    assert r['ap'][:, 2].tolist() == [0.0] * 5                     # ground truth that nothing found: 0, in the mean
    assert r['map'].tolist() == [0.25] * 5
    none = ap_reference([(fx.make_det([[], []], 3), gt)], 3)
    assert none['counts'].tolist() == [0, 0, 0] and none['n_gt'].tolist() == [1, 0, 1] and none['map'].tolist() == [0.0] * 5


def test_the_hand_batch():
    from cfn_hip.segap import ap_reference
    det, gt = fx.hand_batch()
    r = ap_reference([(det, gt)], 5, fx.HAND_TIOU)
    tp, match, n_gt = r['batches'][0]
    assert n_gt.tolist() == [3, 2, 2, 1, 1] and r['counts'].tolist() == [6, 2, 2, 2, 0]
    assert tp.tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0]
    assert match.tolist() == [[1, 5, -1, 2, 6, 15, -1, 11, 13, 12, -1, -1]]
    want0 = np.float32((1.0 / 2.0 + 2.0 / 4.0 + 3.0 / 5.0) / 3.0)
    assert r['ap'][0].tolist() == [want0, 1.0, 1.0, 1.0, 0.0]
    assert r['map'][0] == np.float32((np.float64(want0) + 1.0 + 1.0 + 1.0 + 0.0) / 5.0)


@pytest.mark.parametrize('score_col', [0, 1])
def test_detections_that_are_the_clipped_rows_give_exactly_one(score_col):
    """(a + a) - a == a and r / r == 1 are exact: every detection finds a row at tIoU 1 at every threshold, whatever the scores"""
    from cfn_hip.segap import ap_reference, clip_reference
    _, gt = fx.random_batch(5, 6, 7, 0, 12, half=False)
    part, sp, ep, vid = clip_reference(gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, 7)
    assert part.sum() > 20 and not part.all()
    rng = np.random.RandomState(1)
    rows = [[] for _ in range(6)]
    for g in np.flatnonzero(part):
        rows[vid[g]].append((int(gt.seg[g, 0]), sp[g], ep[g], float(rng.randint(0, 4)) / 4.0, float(rng.rand())))
    det = fx.make_det(rows, 7)
    r = ap_reference([(det, gt)], 7, (0.1, 0.5, 0.9, 1.0), score_col)
    have = r['n_gt'] > 0
    assert have.sum() >= 5 and (r['ap'][:, have] == np.float32(1.0)).all() and (r['ap'][:, ~have] == 0).all() and (r['map'] == np.float32(1.0)).all()
    assert all(int(t) == 15 for c in range(7) for t in r['tps'][c])


@pytest.mark.parametrize('split', ['training', 'testing'])
def test_golden_records_match_their_own_decoded_labels(split):
    """decode_reference of SegLabels.dense_reference() of the 42 annotation records against their annotations: structure only (greedy
    matching guarantees neither a number nor monotonicity in the threshold)"""
    from cfn_hip.detections import decode_reference
    from cfn_hip.segap import DEFAULT_TIOU, clip_reference, match_reference
    lab = fx.golden_labels(split)
    dense, _, valid = lab.dense_reference()
    det = decode_reference(dense, valid, lab.fps, lab.window[:, 0].contiguous(), 0.5)
    n = det.check()
    assert n > 100
    tp, match, n_gt = match_reference(det, lab.seg, lab.offsets, lab.fps, lab.window, lab.t_max, DEFAULT_TIOU)
    assert tp.shape == (n,) and match.shape == (5, n)
    part, _, _, vid = clip_reference(lab.seg, lab.offsets, lab.fps, lab.window, lab.t_max, 157)
    gcls = lab.seg[:, 0].numpy()
    assert n_gt.tolist() == np.bincount(gcls[part].astype(np.int64), minlength=157).tolist() and n_gt.sum() > 100
    dvid = np.searchsorted(det.offsets.numpy(), np.arange(n), side='right') - 1
    dcls = det.seg[:n, 0].numpy()
    for k in range(5):
        hit = np.flatnonzero((tp >> k) & 1)
        assert (match[k, hit] >= 0).all() and (np.delete(match[k], hit) == -1).all()
        g = match[k, hit]
        assert part[g].all() and (gcls[g] == dcls[hit]).all() and (vid[g] == dvid[hit]).all()
        assert len(set(g.tolist())) == len(g)                                  # no row is matched twice at one threshold
    assert ((tp & 1) != 0).sum() > 100                                         # (an empty matching cannot pass)


def test_entry_points_are_declared_exported_and_check_their_arguments():
    cfn_hip = _lib()
    from cfn_hip import ops
    protos = cfn_hip.header_prototypes()
    names = ('cfn_segap_workspace_bytes', 'cfn_segap_gt_tile', 'cfn_segap_det_tile', 'cfn_segap_match', 'cfn_segap_append', 'cfn_ap_sort_counts',
             'cfn_segap_reduce')
    lib = cfn_hip.load()
    for name in names:
        assert name in protos and hasattr(lib, name), name
    f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8
    ret, at, dts = protos['cfn_segap_match']
    assert ret is ctypes.c_int and len(at) == 19 and dts[:11] == [f64, f32, i32, f64, i32, f64, i32, f64, u8, i32, None]
    assert at[16] is ctypes.c_long and at[17] is ctypes.c_long
    assert protos['cfn_segap_append'][2][:8] == [f32, u8, None, f32, u8, i32, i32, i32] and len(protos['cfn_segap_append'][1]) == 14
    assert protos['cfn_ap_sort_counts'][1] == protos['cfn_ap_sort'][1] and protos['cfn_ap_sort_counts'][2] == protos['cfn_ap_sort'][2]
    assert protos['cfn_segap_reduce'][2][:5] == [u8, i32, i32, f32, f32]
    assert protos['cfn_segap_workspace_bytes'][0] is ctypes.c_long
    assert lib.cfn_segap_gt_tile() == ops.SEGAP_GT_TILE == 64 and lib.cfn_segap_det_tile() == ops.SEGAP_DET_TILE
    assert cfn_hip.query('cfn_segap_workspace_bytes', 2, 157, 1000, 9) == (4 * 2 * 157 + 2 + 1000) * 4 + 16
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (65536, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 0, 1), (1, 1, 1 << 31, 1), (1, 1, 1, 0), (1, 1, 1, 1 << 31)):
        assert cfn_hip.query('cfn_segap_workspace_bytes', *bad) == -1, bad
    p = ctypes.c_void_p(8)                                                       # never dereferenced: EVERY call below is refused before a launch
    ok = [p] * 11
    for i in range(11):
        a = list(ok)
        a[i] = None
        if i == 9:                                   # match may be NULL: with valid sizes that call would launch, so only a refused shape is
            assert lib.cfn_segap_match(*a, 0, 1, 1, 1, 0, 1, 1, None) == 1 and 'shape' in cfn_hip.last_error()      # sent (the GPU file passes None)
            continue
        assert lib.cfn_segap_match(*a, 1, 1, 1, 1, 0, 1, 1, None) == 1 and 'null' in cfn_hip.last_error(), i
    for bad, word in (((0, 1, 1, 1, 0, 1, 1), 'shape'), ((1, 65536, 1, 1, 0, 1, 1), 'shape'), ((1, 1, 0, 1, 0, 1, 1), 't_max'),
                      ((1, 1, 1, 0, 0, 1, 1), 'n_thr'), ((1, 1, 1, 9, 0, 1, 1), 'n_thr'), ((1, 1, 1, 1, 2, 1, 1), 'score_col'),
                      ((1, 1, 1, 1, 0, 0, 1), 'shape'), ((1, 1, 1, 1, 0, 1, 0), 'shape')):
        assert lib.cfn_segap_match(*ok, *bad, None) == 1 and word in cfn_hip.last_error(), (bad, cfn_hip.last_error())
    assert lib.cfn_segap_match(*([p] * 10), ctypes.c_void_p(12), 1, 1, 1, 1, 0, 1, 1, None) == 1 and 'boundary' in cfn_hip.last_error()
    for i in range(8):
        a = [p] * 8
        a[i] = None
        assert lib.cfn_segap_append(*a, 1, 1, 0, 1, 1, None) == 1 and 'null' in cfn_hip.last_error(), i
    for bad in ((0, 1, 0, 1, 1), (1, 0, 0, 1, 1), (1, 1, 0, 0, 1), (1, 1, 0, 1, 0), (1, 1, 0, 1, 1 << 31)):
        assert lib.cfn_segap_append(*([p] * 8), *bad, None) == 1 and 'shape' in cfn_hip.last_error(), bad
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert lib.cfn_segap_reduce(*a, 1, 1, 1, None) == 1 and 'null' in cfn_hip.last_error(), i
    for bad, word in (((0, 1, 1), 'shape'), ((1, 0, 1), 'n_thr'), ((1, 9, 1), 'n_thr'), ((1, 1, 0), 'shape')):
        assert lib.cfn_segap_reduce(*([p] * 5), *bad, None) == 1 and word in cfn_hip.last_error(), bad
    for i in range(7):
        a = [p] * 7
        a[i] = None
        assert lib.cfn_ap_sort_counts(*a, 1, 16, None) == 1 and 'null' in cfn_hip.last_error(), i
    assert lib.cfn_ap_sort_counts(*([p] * 7), 0, 16, None) == 1 and 'shape' in cfn_hip.last_error()


def test_ops_and_meter_refuse_host_tensors_and_bad_arguments():
    _lib()
    from cfn_hip import ops
    from cfn_hip.segap import SegmentAPMeter
    det, gt = fx.hand_batch()
    tiou = torch.tensor([0.5], dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.segap_match(det.seg, det.score, det.offsets, gt.seg, gt.offsets, gt.fps, gt.window, tiou, 5, gt.t_max)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.segap_value(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match='on a GPU'):
        SegmentAPMeter('cpu', 5)
    for kw in ({'tiou': ()}, {'tiou': (0.0,)}, {'tiou': (1.5,)}, {'tiou': (0.5,) * 9}, {'score': 'median'}, {'capacity': 0}):
        with pytest.raises(ValueError):                                          # (refused before anything is allocated)
            SegmentAPMeter('cuda', 5, **kw)


def test_scripts_take_a_segment_ap_meter():
    import train_coarse_fineFEAT
    import train_fine
    for mod in (train_fine, train_coarse_fineFEAT):
        sig = inspect.signature(mod.run)
        assert 'segment_ap' in sig.parameters and sig.parameters['segment_ap'].default is None, mod.__name__
        assert all(callable(getattr(mod, n, None)) for n in ('seg_ap_arguments', 'seg_ap_argv', 'seg_ap_from_args', 'segment_ap_add')), mod.__name__
    p = train_fine.seg_ap_arguments(__import__('argparse').ArgumentParser())
    a = p.parse_args(['--seg-ap', '--seg-ap-tiou', '0.3,0.5', '--seg-ap-score', 'mean', '--seg-ap-capacity', '4096'])
    assert a.seg_ap and a.seg_ap_tiou == '0.3,0.5' and a.seg_ap_score == 'mean' and a.seg_ap_capacity == 4096
    assert not p.parse_args([]).seg_ap
    assert train_fine.seg_ap_argv(a) == ['--seg-ap', '--seg-ap-tiou', '0.3,0.5', '--seg-ap-score', 'mean', '--seg-ap-capacity', '4096']
    assert train_fine.seg_ap_argv(p.parse_args([])) == []
