"""GPU: segment-level AP at temporal-IoU thresholds (csrc/segap.hip, cfn_hip/segap.py).

Against match_reference / ap_reference (the seven rules in numpy, checked by hand in test_segap_cpu.py) the device result is BIT-EQUAL in tp,
match, n_gt, counts and the stores' scores and bytes: a tIoU is fp64 subtractions, additions and ONE correctly rounded division, which give
the same double on the device as on the host, and everything else is integer work.  ap and map are within 1 fp32 ulp and bit-equal between
two calls: fewer than 2^24 terms of at most 1 summed in fp64 err by less than 2^-29 relative in any order, so the kernel's fixed order and
numpy's can differ only in the final rounding to fp32.  Every output is handed over filled with a canary.

The kernels' boundaries (sizes from cfn_hip.ops): lanes hold the ground-truth rows of a video SEGAP_GT_TILE = 64 at a time (more: the general
path through the workspace); the score order of a (video, class) group lives in LDS up to SEGAP_DET_TILE = 1024 detections (more: the general
path); the sort walks a class in tiles of AP_SORT_TILE rows with one count per class."""
import numpy as np
import pytest
import torch

import segap_fixture as fx

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY_F, CANARY_B, CANARY_I = -777.25, 0xAA, -7


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32 if x.dtype == np.float32 else np.int64)


def _match_checked(det, gt, tiou, score_col=0):
    """ops.segap_match over canary-filled outputs against match_reference; returns the reference's (tp, match, n_gt)"""
    from cfn_hip import ops
    from cfn_hip.segap import match_reference
    want_tp, want_match, n_gt = match_reference(det, gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, tiou, score_col)
    d, g = det.to(DEV), gt.to(DEV)
    cap, n, n_thr = int(d.seg.shape[0]), len(want_tp), len(tiou)
    out = (torch.full((cap,), CANARY_B, dtype=torch.uint8, device=DEV), torch.full((n_thr, cap), CANARY_I, dtype=torch.int32, device=DEV),
           torch.empty(ops.segap_workspace_bytes(d.batch, d.n_classes, cap, g.seg.shape[0]), dtype=torch.uint8, device=DEV))
    tp, match, _ = ops.segap_match(d.seg, d.score, d.offsets, g.seg, g.offsets, g.fps, g.window, torch.tensor(tiou, dtype=torch.float64, device=DEV),
                                   d.n_classes, g.t_max, score_col, out=out)
    assert tp is out[0] and match is out[1]
    tp, match = tp.cpu().numpy(), match.cpu().numpy()
    assert (tp[:n] == want_tp).all(), 'tp differs at rows %s' % np.flatnonzero(tp[:n] != want_tp)[:8]
    assert (match[:, :n] == want_match).all(), 'match differs'
    assert (tp[n:] == CANARY_B).all() and (match[:, n:] == CANARY_I).all()                          # rows of no detection are not touched
    return want_tp, want_match, n_gt


def _canary_meter(C, tiou, score='max', capacity=64):
    from cfn_hip.segap import SegmentAPMeter
    m = SegmentAPMeter(DEV, C, tiou, score, capacity)
    m.stores[0].fill_(CANARY_F)
    m.stores[1].fill_(CANARY_B)
    return m


def _stores_checked(meter, ref):
    """counts, n_gt and the stores bit-equal to ap_reference's; the rows behind counts untouched"""
    counts, n_gt = meter.counts.cpu().numpy(), meter.n_gt.cpu().numpy()
    assert counts.tolist() == ref['counts'].tolist() and n_gt.tolist() == ref['n_gt'].tolist()
    scores, tps = meter.stores[0].cpu().numpy(), meter.stores[1].cpu().numpy()
    for c in range(meter.n_classes):
        k = int(counts[c])
        assert (_bits(scores[c, :k]) == _bits(ref['scores'][c])).all() and (tps[c, :k] == ref['tps'][c]).all(), 'store of class %d' % c
        assert (scores[c, k:] == CANARY_F).all() and (tps[c, k:] == CANARY_B).all(), 'rows behind the count of class %d were written' % c


def _value_checked(meter, ref):
    ap, mp = meter.value_device()
    ap2, mp2 = meter.value_device()
    assert torch.equal(ap.view(torch.int32), ap2.view(torch.int32)) and torch.equal(mp.view(torch.int32), mp2.view(torch.int32)), 'two calls differ'
    hap, hmp = meter.value()
    assert torch.equal(hap, ap.cpu()) and torch.equal(hmp, mp.cpu()) and tuple(hap.shape) == ref['ap'].shape
    worst = int(max(_ulps(hap.numpy(), ref['ap']).max(), _ulps(hmp.numpy(), ref['map']).max()))
    print('ap / map: at most %d fp32 ulp from the reference' % worst)
    assert worst <= 1, 'ap: %d fp32 ulps from the reference' % worst
    return hap.numpy(), hmp.numpy()


def _meter_checked(batches, C, tiou, score='max', capacity=64):
    """every batch through add() of a fixed-capacity meter with canary stores against ONE ap_reference run over all of them"""
    from cfn_hip.segap import SCORE_COLUMNS, ap_reference
    ref = ap_reference(batches, C, tiou, SCORE_COLUMNS[score])
    meter = _canary_meter(C, tiou, score, capacity)
    for (det, gt), (want_tp, want_match, _) in zip(batches, ref['batches']):
        tp, match = meter.add(det.to(DEV), gt.to(DEV), want_match=True)
        n = len(want_tp)
        assert (tp.cpu().numpy()[:n] == want_tp).all() and (match.cpu().numpy()[:, :n] == want_match).all()
    _stores_checked(meter, ref)
    assert int(meter.flags.item()) == 0
    return meter, ref, _value_checked(meter, ref)


def test_hand_cases_and_edge_inputs():
    """B = 3, C = 5 (segap_fixture.hand_batch): the worked-out AP, rows the window clips, e <= s, classes outside [0, C), a video without
    ground truth, ground truth without a detection"""
    det, gt = fx.hand_batch()
    tp, match, n_gt = _match_checked(det, gt, fx.HAND_TIOU)
    assert tp.tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0] and n_gt.tolist() == [3, 2, 2, 1, 1]
    _, _, (ap, mp) = _meter_checked([(det, gt)], 5, fx.HAND_TIOU)
    want0 = np.float32((1.0 / 2.0 + 2.0 / 4.0 + 3.0 / 5.0) / 3.0)
    assert _ulps(ap[0], np.array([want0, 1.0, 1.0, 1.0, 0.0], np.float32)).max() <= 1 and ap[0, 1:].tolist() == [1.0, 1.0, 1.0, 0.0]
    _match_checked(det, gt, (0.1, 0.3, 0.5, 0.7, 0.9), 1)


@pytest.mark.parametrize('n_thr,score', [(1, 'max'), (1, 'mean'), (8, 'max'), (8, 'mean')])
def test_random_batches_with_one_and_eight_thresholds_and_both_scores(n_thr, score):
    tiou = (0.5,) if n_thr == 1 else (0.05, 0.2, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0)
    batches = [fx.random_batch(10 + i, B, 6, 40, 30) for i, B in enumerate((4, 1, 3))]
    assert sum(int(d.total) for d, _ in batches) > 100
    _, ref, _ = _meter_checked(batches, 6, tiou, score, capacity=128)
    assert all(len(set(t.tolist())) > 1 for t in ref['tps'][:3])                          # true and false positives in the stores


def test_one_video():
    det, gt = fx.random_batch(3, 1, 4, 30, 20)
    assert det.batch == 1 and int(det.total) > 5
    _match_checked(det, gt, (0.3, 0.7))
    _meter_checked([(det, gt)], 4, (0.3, 0.7))


def test_a_batch_without_detections_and_a_batch_without_ground_truth():
    """no detection: Detections.seg is never empty (one row no offset range covers), nothing is appended but n_gt advances; no ground truth:
    the padding row of SegLabels.seg, which no offset range covers either, so every detection is a false positive"""
    det, gt = fx.random_batch(4, 3, 4, 20, 10)
    none = fx.make_det([[], [], []], 4)
    assert tuple(none.seg.shape) == (1, 3) and int(none.total) == 0
    tp, _, n_gt = _match_checked(none, gt, (0.5,))
    assert len(tp) == 0 and n_gt.sum() > 0
    empty = fx.make_gt([[], [], []], [24.0, 25.0, 30.0], gt.window.tolist(), 4)
    assert tuple(empty.seg.shape) == (1, 3) and empty.offsets.tolist() == [0, 0, 0, 0]
    tp, match, n_gt = _match_checked(det, empty, (0.5, 0.9))
    assert len(tp) > 5 and not tp.any() and (match == -1).all() and n_gt.sum() == 0
    meter, ref, (ap, mp) = _meter_checked([(none, gt), (det, empty), (det, gt)], 4, (0.5, 0.9))
    assert ref['counts'].sum() == 2 * int(det.total)


def _alternating(nd, seed):
    """probs (2, 3, TL) with TL = 2 * nd - 1, just large enough for nd runs of one frame in row (0, 1); a few runs elsewhere; ground truth
    in frame units: rows of class 1 over 1 to 3 frames at random places (tIoU 1, 1/2, 1/3 with the one-frame detections) and some of class 0"""
    rng = np.random.RandomState(seed)
    TL = 2 * nd - 1
    probs = torch.zeros(2, 3, TL)
    probs[0, 1, ::2] = torch.from_numpy(0.5 + rng.randint(1, 32, nd) / 64.0).float()            # (scores tie)
    probs[0, 0, 3:9] = 0.9
    probs[1, 2, 1::5] = 0.8
    probs[1, 1, 0:4] = 0.7
    rows = [[], []]
    for t in rng.choice(nd, 40, replace=False):
        rows[0].append((1, 2 * t - 0.5, 2 * t + 0.5 + 2 * rng.randint(0, 3)))
    rows[0] += [(0, 2.5, 8.5), (0, 0.5, 3.5)]
    rows[1] += [(1, -0.5, 3.5), (2, 0.5, 1.5), (2, 5.5, 7.5)]
    gt = fx.make_gt(rows, [1.0, 1.0], [[0, TL], [0, TL]], 3)
    return probs, torch.tensor([TL, TL], dtype=torch.int32), gt


@pytest.mark.parametrize('edge', [-1, 0, 1])
def test_detections_per_group_around_the_lds_tile(edge):
    """a (video, class) group of SEGAP_DET_TILE - 1, SEGAP_DET_TILE and SEGAP_DET_TILE + 1 detections (the last takes the general path: its
    order goes through the workspace), decoded on the device from alternating frames"""
    from cfn_hip import ops
    from cfn_hip.detections import decode
    nd = ops.SEGAP_DET_TILE + edge
    probs, valid, gt = _alternating(nd, 20 + edge)
    det = decode(probs.to(DEV), valid.to(DEV)).to('cpu')
    assert det.offsets.tolist()[1] == nd + 1 and det.check() > nd
    tp, _, _ = _match_checked(det, gt, (0.3, 0.5, 1.0))
    assert 10 < int((tp & 1).astype(bool).sum()) <= 42                                         # (40 rows of class 1, 2 of class 0)
    _meter_checked([(det, gt)], 3, (0.3, 0.5, 1.0), capacity=nd + 8)


def test_both_general_paths_in_one_group():
    """a group of SEGAP_DET_TILE + 1 detections (its order goes through the workspace) inside a video of more than SEGAP_GT_TILE ground-truth
    rows (its tiles are walked per detection): 110 rows of the group's class and 2 of another"""
    from cfn_hip import ops
    from cfn_hip.detections import decode
    nd = ops.SEGAP_DET_TILE + 1
    probs, valid, gt = _alternating(nd, 21)
    rng = np.random.RandomState(5)
    rows = [[tuple(r) for r in gt.seg[:42].tolist()] + [(1, 2 * t - 0.5, 2 * t + 0.5 + 2 * rng.randint(0, 3)) for t in rng.choice(nd, 70, replace=False)],
            [tuple(r) for r in gt.seg[42:].tolist()]]
    gt = fx.make_gt(rows, [1.0, 1.0], gt.window.tolist(), 3)
    assert gt.offsets.tolist() == [0, 112, 115] and 112 > ops.SEGAP_GT_TILE
    det = decode(probs.to(DEV), valid.to(DEV)).to('cpu')
    assert det.offsets.tolist()[1] == nd + 1
    tp, match, _ = _match_checked(det, gt, (0.3, 0.5, 1.0))
    assert 40 < int((tp & 1).astype(bool).sum()) <= 112 and match.max() > ops.SEGAP_GT_TILE
    _meter_checked([(det, gt)], 3, (0.3, 0.5, 1.0), capacity=nd + 8)


def _crowded(n_rows, n_classes, seed, n_det=90):
    """video 0: n_rows ground-truth rows over n_classes classes (class = row % n_classes), four seconds apart with jittered bounds, and n_det
    detections that are jittered copies of random rows; video 1: a few of each"""
    rng = np.random.RandomState(seed)
    gts = [(i % n_classes, 4.0 * i + 0.5 * rng.randint(0, 3), 4.0 * i + 3.0 + 0.5 * rng.randint(0, 3)) for i in range(n_rows)]
    dets, seen = [], set()
    for i in rng.randint(0, n_rows, n_det):
        c, s, e = gts[i]
        s, e = s + 0.5 * rng.randint(-2, 3), e + 0.5 * rng.randint(-2, 3)
        if (c, s) not in seen:
            seen.add((c, s))
            dets.append((c, s, e, rng.randint(1, 9) / 8.0, rng.rand()))
    C = max(n_classes, 2)
    det = fx.make_det([dets, [(0, 1, 5, 0.5, 0.5), (1, 2, 8, 0.25, 0.5)]], C)
    gt = fx.make_gt([gts, [(0, 1, 4), (1, 2, 8), (0, 1, 6)]], [1.0, 1.0], [[0, 4 * n_rows + 8], [0, 4 * n_rows + 8]], C)
    return det, gt


@pytest.mark.parametrize('edge', [-1, 0, 1])
def test_ground_truth_rows_per_group_around_the_tile_of_lanes(edge):
    """one class with SEGAP_GT_TILE - 1, SEGAP_GT_TILE and SEGAP_GT_TILE + 1 rows in a video; the last takes the general path"""
    from cfn_hip import ops
    det, gt = _crowded(ops.SEGAP_GT_TILE + edge, 1, 30 + edge)
    tp, _, n_gt = _match_checked(det, gt, (0.25, 0.5, 0.75))
    assert n_gt[0] == ops.SEGAP_GT_TILE + edge + 2 and 20 < int((tp & 2).astype(bool).sum()) < len(tp)
    _meter_checked([(det, gt)], 2, (0.25, 0.5, 0.75), capacity=128)


def test_the_general_path_over_several_tiles_of_ground_truth():
    """a video of 3 * SEGAP_GT_TILE + 7 rows over 3 classes: every group walks four tiles, the best row per threshold is carried across them"""
    from cfn_hip import ops
    det, gt = _crowded(3 * ops.SEGAP_GT_TILE + 7, 3, 41, n_det=200)
    tp, match, _ = _match_checked(det, gt, (0.25, 0.5, 0.75, 1.0), 1)
    assert match.max() > 2 * ops.SEGAP_GT_TILE and 50 < int((tp & 1).astype(bool).sum()) < len(tp)
    _meter_checked([(det, gt)], 3, (0.25, 0.5, 0.75, 1.0), 'mean', capacity=256)


def test_sort_tile_edges_with_one_count_per_class():
    """counts of 0, 1, AP_SORT_TILE - 1 and AP_SORT_TILE + 1 in the four classes of one meter, built up by nine small batches"""
    from cfn_hip import ops
    tile = ops.AP_SORT_TILE
    rng = np.random.RandomState(7)
    gt_rows = [(c, 10.0 * i, 10.0 * i + 0.5) for c in (1, 2, 3) for i in range(5)]
    batches, left = [], {1: 1, 2: tile - 1, 3: tile + 1}
    while any(left.values()):
        rows = []
        for c in (1, 2, 3):
            k = min(left[c], 1024)
            left[c] -= k
            rows += [(c, float(i), i + 0.5, rng.randint(0, 64) / 64.0, rng.rand()) for i in rng.choice(2048, k, replace=False)]
        batches.append((fx.make_det([rows], 4), fx.make_gt([gt_rows], [1.0], [[0, 4096]], 4)))
    assert len(batches) == 9
    meter, ref, (ap, _) = _meter_checked(batches, 4, (0.5, 1.0), capacity=tile + 16)
    assert ref['counts'].tolist() == [0, 1, tile - 1, tile + 1] and ref['n_gt'].tolist() == [0, 45, 45, 45]
    assert ap[0, 0] == 0 and (ap[0, 2:] > 0).all()


@pytest.mark.parametrize('split', ['training', 'testing'])
def test_golden_records_through_decode_and_the_meter(split):
    """the 42 annotation records: SegLabels.dense() -> decode -> SegmentAPMeter on the device is bit-equal to dense_reference ->
    decode_reference -> ap_reference on the host"""
    from cfn_hip.detections import decode, decode_reference
    from cfn_hip.segap import DEFAULT_TIOU, ap_reference
    lab = fx.golden_labels(split)
    dense, _, valid = lab.dense_reference()
    want = decode_reference(dense, valid, lab.fps, lab.window[:, 0].contiguous(), 0.5)
    ref = ap_reference([(want, lab)], 157, DEFAULT_TIOU)
    dlab = lab.to(DEV)
    ddense, _, dvalid = dlab.dense()
    det = decode(ddense, dvalid, dlab.fps, dlab.window[:, 0].contiguous(), 0.5, cap=4096)
    meter = _canary_meter(157, DEFAULT_TIOU, capacity=32)
    tp, match = meter.add(det, dlab, want_match=True)
    n = want.check()
    assert int(det.total.item()) == n and torch.equal(det.seg[:n].cpu().view(torch.int64), want.seg[:n].view(torch.int64))
    want_tp, want_match, _ = ref['batches'][0]
    assert (tp.cpu().numpy()[:n] == want_tp).all() and (match.cpu().numpy()[:, :n] == want_match).all()
    _stores_checked(meter, ref)
    _value_checked(meter, ref)
    print('%s windows: %d detections, %d of %d rows participate, true positives %s' % (
        split, n, int(ref['n_gt'].sum()), int(lab.offsets[-1]), [int(((want_tp >> k) & 1).sum()) for k in range(5)]))


@pytest.mark.parametrize('score', ['max', 'mean'])
def test_detections_that_are_the_clipped_rows_give_exactly_one(score):
    from cfn_hip.segap import clip_reference
    _, gt = fx.random_batch(5, 6, 7, 0, 12, half=False)
    part, sp, ep, vid = clip_reference(gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, 7)
    rng = np.random.RandomState(1)
    rows = [[] for _ in range(6)]
    for g in np.flatnonzero(part):
        rows[vid[g]].append((int(gt.seg[g, 0]), sp[g], ep[g], float(rng.randint(0, 4)) / 4.0, float(rng.rand())))
    tiou = (0.1, 0.5, 0.9, 1.0)
    meter, ref, (ap, mp) = _meter_checked([(fx.make_det(rows, 7), gt)], 7, tiou, score)
    have = ref['n_gt'] > 0
    assert have.sum() >= 5 and (ap[:, have] == np.float32(1.0)).all() and (ap[:, ~have] == 0).all() and (mp == np.float32(1.0)).all()


def test_a_dense_label_pair_is_decoded_into_frame_unit_ground_truth():
    from cfn_hip.detections import decode, decode_reference
    from cfn_hip.segap import ap_reference
    rng = np.random.RandomState(3)
    B, C, TL = 3, 5, 37
    labels = torch.from_numpy((rng.rand(B, C, TL) < 0.4).astype(np.float32))
    valid = torch.tensor([37, 20, 0], dtype=torch.int32)
    labels = labels * (torch.arange(TL)[None, None] < valid[:, None, None])
    probs = torch.from_numpy((labels.numpy() * 0.5 + rng.rand(B, C, TL) * 0.6).astype(np.float32))
    det = decode(probs.to(DEV), valid.to(DEV), max_gap=1)
    g = decode_reference(labels, valid, thr=0.5)
    gt = (g.seg, g.offsets, torch.ones(B, dtype=torch.float64), torch.stack([torch.zeros_like(valid), valid], 1), TL)
    ref = ap_reference([(det.to('cpu'),) + gt], C)
    meter = _canary_meter(C, (0.1, 0.3, 0.5, 0.7, 0.9), capacity=128)
    meter.add(det, (labels.to(DEV), valid.to(DEV)))
    _stores_checked(meter, ref)
    _value_checked(meter, ref)
    assert ref['n_gt'].sum() > 20 and sum(int(t.any()) for t in ref['tps']) >= 3


def test_fixed_capacity_drops_the_batch_that_does_not_fit():
    """class 0 of the hand batch has 6 detections: with 5 rows per class nothing of the batch is written, no count changes, the flag is set and
    value() raises; a batch that fits before it stays as it was"""
    from cfn_hip import ops
    from cfn_hip.segap import ap_reference
    det, gt = fx.hand_batch()
    small = (fx.make_det([[(0, 0, 10, 0.5, 0.5)]], 5), fx.make_gt([[(0, 0, 10)]], [1.0], [[0, 100]], 5))
    meter = _canary_meter(5, fx.HAND_TIOU, capacity=5)
    meter.add(small[0].to(DEV), small[1].to(DEV))
    ref = ap_reference([small], 5, fx.HAND_TIOU)
    _stores_checked(meter, ref)
    tp, _ = meter.add(det.to(DEV), gt.to(DEV))
    assert tp.cpu().numpy()[:12].tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0]                # the match itself is a per-batch output
    _stores_checked(meter, ref)                                                                # counts, n_gt, stores and canaries unchanged
    assert int(meter.flags.item()) == ops.SEGAP_FLAG_OVERFLOW
    meter.value_device()
    with pytest.raises(RuntimeError, match='did not fit the fixed capacity of 5'):
        meter.value()
    meter.reset()
    assert int(meter.flags.item()) == 0 and not meter.counts.any() and not meter.n_gt.any()
    meter.add(small[0].to(DEV), small[1].to(DEV))
    assert meter.value()[0][0, 0] == 1.0


def test_growing_stores_give_what_a_large_fixed_capacity_gives():
    from cfn_hip.segap import SegmentAPMeter, ap_reference

    class Small(SegmentAPMeter):
        MIN_CAPACITY = 4
    batches = [fx.random_batch(60 + i, 3, 4, 40, 20) for i in range(5)]
    grow, fixed = Small(DEV, 4), SegmentAPMeter(DEV, 4, capacity=1024)
    assert grow.stores[0].shape[1] == 4
    for det, gt in batches:
        grow.add(det.to(DEV), gt.to(DEV))
        fixed.add(det.to(DEV), gt.to(DEV))
    counts = fixed.counts.cpu()
    assert torch.equal(grow.counts.cpu(), counts) and torch.equal(grow.n_gt.cpu(), fixed.n_gt.cpu()) and int(counts.max()) > 16
    assert 16 < grow.stores[0].shape[1] < 1024                                                 # grown by the true counts, not by the loose bound
    for c in range(4):
        k = int(counts[c])
        assert torch.equal(grow.stores[0][c, :k], fixed.stores[0][c, :k]) and torch.equal(grow.stores[1][c, :k], fixed.stores[1][c, :k])
    (a, m), (a2, m2) = grow.value(), fixed.value()
    assert torch.equal(a, a2) and torch.equal(m, m2)
    ref = ap_reference(batches, 4)
    assert _ulps(a.numpy(), ref['ap']).max() <= 1 and counts.tolist() == ref['counts'].tolist()
    # the bound is B * ((TL + 1) // 2) with TL = the labels' t_max unless tl= says what the detections were decoded over
    det = fx.make_det([[(0, float(i), i + 0.5, 0.5, 0.5) for i in range(30)]], 4).to(DEV)
    short = fx.make_gt([[(0, 0, 1)]], [1.0], [[0, 4]], 4).to(DEV)
    late, told = Small(DEV, 4), Small(DEV, 4)
    late.add(det, short)
    with pytest.raises(RuntimeError, match=r'add\(tl=TL\)'):
        late.value()
    told.add(det, short, tl=60)
    assert told.counts.tolist() == [30, 0, 0, 0] and told.value()[0][0, 0] == 1.0


def test_add_with_out_buffers_is_capturable():
    """fixed capacity and out=: add() allocates nothing and waits for nothing, so a graph holds it; two replays equal two eager calls"""
    from cfn_hip import ops
    from cfn_hip.segap import SegmentAPMeter
    det, gt = fx.random_batch(70, 3, 4, 40, 20)
    det, gt = det.to(DEV), gt.to(DEV)
    cap = int(det.seg.shape[0])
    eager, graphed = SegmentAPMeter(DEV, 4, capacity=256), SegmentAPMeter(DEV, 4, capacity=256)
    out = (torch.empty(cap, dtype=torch.uint8, device=DEV), None,
           torch.empty(ops.segap_workspace_bytes(3, 4, cap, gt.seg.shape[0]), dtype=torch.uint8, device=DEV))
    for _ in range(2):
        eager.add(det, gt)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.add(det, gt, out=out)
    graphed.reset()                                                                            # (whatever the capture's warm-up may have run)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.counts, eager.counts) and torch.equal(graphed.n_gt, eager.n_gt) and int(eager.counts.sum()) == 2 * int(det.total)
    for c in range(4):
        k = int(eager.counts[c])
        assert torch.equal(graphed.stores[0][c, :k], eager.stores[0][c, :k]) and torch.equal(graphed.stores[1][c, :k], eager.stores[1][c, :k])
    assert all(torch.equal(x, y) for x, y in zip(graphed.value(), eager.value()))


class _Spy(object):
    """mixed into SegmentAPMeter: keeps what value() gave run() before run() resets the meter"""

    def value(self):
        self.last = super().value()
        return self.last


def _spy_meter(tiou, **kw):
    from cfn_hip.segap import SegmentAPMeter
    return type('SpyMeter', (_Spy, SegmentAPMeter), {})(DEV, 157, tiou, **kw)


def _run_reference(val, datasets, seconds, tiou, thr, max_gap, min_len):
    """ap_reference over decode_reference of the spied validation probs (one video per batch) against the videos' own labels: SegLabel
    samples in seconds, dense arrays decoded into frame units"""
    from cfn_hip.detections import decode_reference
    from cfn_hip.seglabels import collate_seg
    from cfn_hip.segap import ap_reference
    batches = []
    for i, (probs, valid) in enumerate(val):
        label = datasets[i][1]
        if seconds:
            lab = collate_seg([label])
            batches.append((decode_reference(probs, valid, lab.fps, lab.window[:, 0].contiguous(), thr, max_gap, min_len), lab))
        else:
            dense = torch.from_numpy(np.ascontiguousarray(label))[None]
            g = decode_reference(dense, valid, thr=0.5)
            batches.append((decode_reference(probs, valid, None, None, thr, max_gap, min_len), g.seg, g.offsets, torch.ones(1, dtype=torch.float64),
                            torch.stack([torch.zeros_like(valid), valid], 1), int(dense.shape[2])))
    return ap_reference(batches, 157, tiou)


def _line(epoch, tiou, mp):
    return ' Epoch:%d val ' % epoch + ' '.join('seg-mAP@%g: %.4f' % (t, float(m)) for t, m in zip(tiou, mp))


def test_train_fine_feeds_the_meter_from_its_validation_phase(tmp_path, monkeypatch):
    """run(..., segment_ap=meter) on the tiny SegLabel loader of test_hip_detections.py: the meter's value() at the end of the validation
    phase equals ap_reference over decode_reference of the spied validation probs, the line is logged behind the existing one, and the
    losses and the existing line are bit-equal to a run without the meter"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _run
    crop, tiou = 64, (0.1, 0.5)

    def go(tag, meter):
        mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                          collate_fn=collate.fine_collate_u8)
        return _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / (tag + '_')),
                    segment_ap=meter)
    meter = _spy_meter(tiou, thr=0.5, max_gap=2, min_len=2)
    losses, lines, val = go('seg', meter)
    assert len(lines) == 2 and 'mAP' in lines[0] and lines[1].startswith(' Epoch:4 val seg-mAP@0.1: ') and ' seg-mAP@0.5: ' in lines[1]
    ref = _run_reference(val, _SegVideos(3, crop, False), True, tiou, 0.5, 2, 2)
    assert len(val) == 3 and ref['counts'].sum() > 0 and ref['n_gt'].sum() > 0
    ap, mp = meter.last
    assert _ulps(ap.numpy(), ref['ap']).max() <= 1 and _ulps(mp.numpy(), ref['map']).max() <= 1
    assert lines[1] == _line(4, tiou, mp)
    assert not meter.counts.any()                                                              # empty again for the next phase
    losses0, lines0, _ = go('none', None)
    assert losses0 == losses and lines0 == lines[:1]
    monkeypatch.setattr(train_fine.cdist, 'init_from_env', lambda: (0, 2, torch.device(DEV)))
    with pytest.raises(RuntimeError, match='ONE process'):
        train_fine.run(dataloaders={}, segment_ap=meter)


def test_train_fine_hands_the_writers_decode_to_the_meter_with_dense_labels(tmp_path, monkeypatch):
    """a DetectionWriter AND a meter on the dense loader: the meter is fed the writer's decode (the writer's thr / gap / min_len, not its
    own, which would find other segments) in frame units, against decode(labels, valid_t, thr=0.5) as the ground truth; the file is what
    the writer alone writes"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _expected_rows, _run, _same_file
    from cfn_hip.detections import DetectionWriter, epoch_path
    crop, tiou = 64, (0.3, 0.7)
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, True), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.fine_collate_u8)
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), 0.5, 2, 2)
    meter = _spy_meter(tiou, thr=0.9, max_gap=0, min_len=7)
    _, lines, val = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, writer, max_epochs=4, save_model=str(tmp_path / 'm_'),
                         segment_ap=meter)
    assert _same_file(epoch_path(writer.path, 4), _expected_rows(val, 3, False, 0.5, 2, 2)) > 0
    ref = _run_reference(val, _SegVideos(3, crop, True), False, tiou, 0.5, 2, 2)
    assert ref['counts'].sum() > 0 and ref['n_gt'].sum() > 0
    ap, mp = meter.last
    assert _ulps(ap.numpy(), ref['ap']).max() <= 1 and _ulps(mp.numpy(), ref['map']).max() <= 1
    assert len(lines) == 2 and lines[1] == _line(4, tiou, mp)


def test_train_coarse_feeds_the_meter_from_its_validation_phase(tmp_path, monkeypatch):
    """the same once through train_coarse_fineFEAT.run: two training phases, one validation phase of two videos, SegLabel samples"""
    import torch.utils.data as tud
    import collate
    import train_coarse_fineFEAT as tc
    from test_hip_detections import _SegVideos, _run
    tiou = (0.1, 0.5)
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, 224, False, coarse=True), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.coarse_collate_u8)
    meter = _spy_meter(tiou, thr=0.5, max_gap=2, min_len=2)
    _, lines, val = _run(tc, monkeypatch, {'train': mk(2, 2), 'val': mk(2, 1)}, None, max_epochs=2, save_model=str(tmp_path / 'm_'),
                         csv_path=str(tmp_path / 'c.csv'), segment_ap=meter)
    ref = _run_reference(val, _SegVideos(2, 224, False, coarse=True), True, tiou, 0.5, 2, 2)
    assert len(val) == 2 and ref['counts'].sum() > 0 and ref['n_gt'].sum() > 0
    ap, mp = meter.last
    assert _ulps(ap.numpy(), ref['ap']).max() <= 1 and _ulps(mp.numpy(), ref['map']).max() <= 1
    assert len(lines) == 2 and lines[1] == _line(2, tiou, mp) and not meter.counts.any()
