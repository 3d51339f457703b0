"""GPU: activity proposals -- candidates at K levels (csrc/detections.hip, cfn_decode_segments_levels) and temporal NMS (csrc/segnms.hip),
cfn_hip/detections.py decode_levels / nms / propose.

Against decode_levels_reference and nms_reference (the rules in numpy, checked by hand in test_proposals_cpu.py) the device result is
BIT-EQUAL, everywhere, over canary-filled buffers, and bit-equal between two calls.  That holds for score[:, 1] too, where
test_hip_detections.py allows 1 ulp, because of the inputs chosen here: every level is >= 0.1 > 2^-4 and scores are <= 1, so an active
value is a multiple of 2^-27, a row has at most 2^11 frames, and every partial sum of active values is a multiple of 2^-27 below 2^11 --
38 bits, exact in fp64 in ANY order; the one division and the rounding to fp32 then see the same double on both sides.  NMS copies.

The kernels' boundaries: the level decode's are those of decode (a 64-frame mask word, a 1024-frame pass, 16-byte loads when TL % 4 == 0)
with rows (b, c, k); NMS suppresses a (video, class) group of up to NMS_DET_TILE = 1024 candidates in LDS with 16 flag bits per lane, a
larger one through the workspace (the general path)."""
import numpy as np
import pytest
import torch

import seg_fixture as sf
import segap_fixture as fx
from proposals_fixture import LEVELS5, candidates, random_probs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY_F, CANARY_I, CANARY_B = -777.25, -12345, 0xAB


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _levels_out(B, C, K, TL, rows=None):
    from cfn_hip import ops
    rows = ops.decode_segments_levels_cap(B, C, K, TL) if rows is None else rows
    return (torch.full((rows, 3), CANARY_F, dtype=torch.float64, device=DEV), torch.full((rows, 3), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((rows, 2), CANARY_F, dtype=torch.float32, device=DEV), torch.full((rows,), CANARY_B, dtype=torch.uint8, device=DEV),
            torch.full((B + 1,), CANARY_I, dtype=torch.int32, device=DEV), torch.full((1,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.empty(ops.decode_segments_levels_workspace_bytes(B, C, K, TL), dtype=torch.uint8, device=DEV))


def _nms_out(B, C, cap_in, rows=None):
    from cfn_hip import ops
    rows = cap_in if rows is None else rows
    return (torch.full((rows, 3), CANARY_F, dtype=torch.float64, device=DEV), torch.full((rows, 3), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((rows, 2), CANARY_F, dtype=torch.float32, device=DEV), torch.full((B + 1,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((1,), CANARY_I, dtype=torch.int32, device=DEV), torch.full((cap_in,), CANARY_B, dtype=torch.uint8, device=DEV),
            torch.full((rows,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.empty(ops.nms_segments_workspace_bytes(B, C, cap_in), dtype=torch.uint8, device=DEV))


def _same_records(got, ref, k):
    """the first k rows of a device Detections bit-equal to the reference's, offsets and total equal, the rows behind k untouched"""
    assert got.total.cpu().tolist() == ref.total.tolist() and got.offsets.cpu().tolist() == ref.offsets.tolist()
    seg, frames, score = got.seg.cpu(), got.frames.cpu(), got.score.cpu()
    assert torch.equal(seg[:k].view(torch.int64), ref.seg[:k].view(torch.int64)), 'seg differs in its bits'
    assert torch.equal(frames[:k], ref.frames[:k])
    assert torch.equal(_bits(score[:k]), _bits(ref.score[:k])), 'score differs in its bits'
    assert bool((seg[k:] == CANARY_F).all()) and bool((frames[k:] == CANARY_I).all()) and bool((score[k:] == CANARY_F).all())


def _levels_checked(probs, valid, fps, start, levels, max_gap=0, min_len=1, cap=None):
    """decode_levels(out=canaries) against decode_levels_reference, twice: the second call gives the same bits.  -> (total, device result, level)"""
    from cfn_hip.detections import decode_levels, decode_levels_reference
    B, C, TL = probs.shape
    K = int(levels.shape[1]) if torch.is_tensor(levels) else len(levels)
    ref, ref_level = decode_levels_reference(probs, valid, fps, start, levels, max_gap, min_len)
    total = int(ref.total)
    dl = levels.to(DEV) if torch.is_tensor(levels) else levels
    args = (probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), dl, max_gap, min_len)
    out = _levels_out(B, C, K, TL, rows=None if cap is None else total + 5)
    got, level = decode_levels(*args, cap=cap, out=out)
    assert all(g is o for g, o in zip(got[:5], (out[0], out[1], out[2], out[4], out[5]))) and level is out[3] and got.n_classes == C
    k = total if cap is None else min(total, cap)
    assert got.cap == (out[0].shape[0] if cap is None else cap)
    _same_records(got, ref, k)
    level = level.cpu()
    assert torch.equal(level[:k], ref_level[:k]) and bool((level[k:] == CANARY_B).all())
    again, level2 = decode_levels(*args, cap=cap, out=_levels_out(B, C, K, TL, rows=None if cap is None else total + 5))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[:5], got[:5])) and torch.equal(level2.cpu(), level), 'two calls differ'
    return total, got, level


def _meta(B, TL):
    """valid_t < TL for the second video; non-trivial fps and start"""
    valid = [TL, max(TL - TL // 3, 0), TL]
    return (torch.tensor(valid[:B], dtype=torch.int32), torch.tensor([24.0, 29.97, 12.5][:B], dtype=torch.float64),
            torch.tensor([0, 17, 12345][:B], dtype=torch.int32))


# 1 frame; 63 / 64 / 65 (one mask word, a second one; 64: 16-byte loads); 1023 / 1025 (a pass, and one frame of a second: dword loads);
# 1028 (16-byte loads, one lane over a pass)
@pytest.mark.parametrize('K', [1, 3, 16])
@pytest.mark.parametrize('TL', [1, 63, 64, 65, 1023, 1025, 1028])
def test_level_decode_at_every_boundary(TL, K):
    """per-class, unsorted levels; valid_t < TL; with and without gap closing and min_len"""
    B, C = 2, 3
    probs = random_probs(100 * TL + K, B, C, TL, noise=0.25)
    g = torch.Generator().manual_seed(K)
    levels = 0.1 + 0.8 * torch.rand(C, K, generator=g)
    valid, fps, start = _meta(B, TL)
    found = 0
    for max_gap, min_len in ((0, 1), (3, 4)):
        n, got, level = _levels_checked(probs, valid, fps, start, levels, max_gap, min_len)
        found += n
    assert found > 0 or TL == 1
    if K == 1:                                                     # L4: decode's result bit for bit
        from cfn_hip.detections import decode
        one = decode(probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), levels[:, 0].contiguous().to(DEV), 3, 4)
        assert int(one.total) == n and all(torch.equal(_bits(a[:n]), _bits(b[:n])) for a, b in zip(one[:3], got[:3]))
        assert torch.equal(one.offsets, got.offsets) and not level[:n].any()


def test_level_decode_fills_the_default_cap_and_keeps_the_prefix_under_a_small_cap():
    from cfn_hip import ops
    B, C, TL = 2, 3, 129
    probs = torch.zeros(B, C, TL)
    probs[:, :, ::2] = 0.75
    valid, fps, start = torch.full((B,), TL, dtype=torch.int32), torch.tensor([24.0, 29.97], dtype=torch.float64), torch.tensor([0, 9], dtype=torch.int32)
    n, got, level = _levels_checked(probs, valid, fps, start, (0.5, 0.25, 0.7))          # the alternating worst case at every level
    assert n == ops.decode_segments_levels_cap(B, C, 3, TL) == B * C * 3 * 65 == got.seg.shape[0] and got.check() == n
    assert level[:3 * 65].tolist() == [0] * 65 + [1] * 65 + [2] * 65
    n, cut, _ = _levels_checked(probs, valid, fps, start, (0.5, 0.25, 0.7), cap=100)     # rows >= cap are not written, the counts are true
    assert n == B * C * 3 * 65 and cut.cap == 100
    with pytest.raises(RuntimeError, match=r'%d segments.*cap = 100' % n):
        cut.check()
    from cfn_hip.detections import decode_levels
    with pytest.raises(RuntimeError, match='out'):
        decode_levels(probs.to(DEV), valid.to(DEV), levels=(0.5, 0.25), out=_levels_out(B, C, 3, TL)[:6])


def _nms_checked(det, thr, score='max', cap=None):
    """nms(out=canaries) of a host Detections on the GPU against nms_reference, twice.  -> (kept, reference result, keep)"""
    from cfn_hip.detections import nms, nms_reference
    ref, ref_keep, ref_src = nms_reference(det, thr, score)
    total, n_in = int(ref.total), int(ref_keep.numel())
    d = det.to(DEV)
    B, cap_in = d.batch, int(d.cap)
    out = _nms_out(B, d.n_classes, cap_in, rows=None if cap is None else total + 5)
    got, keep, src = nms(d, thr, score, cap=cap, out=out)
    assert all(g is o for g, o in zip(got[:5], out[:5])) and keep is out[5] and src is out[6] and got.n_classes == det.n_classes
    k = total if cap is None else min(total, cap)
    assert got.cap == (cap_in if cap is None else cap)
    _same_records(got, ref, k)
    keep, src = keep.cpu(), src.cpu()
    assert torch.equal(keep[:n_in], ref_keep), 'keep differs at rows %s' % torch.nonzero(keep[:n_in] != ref_keep).flatten()[:8].tolist()
    assert bool((keep[n_in:] == CANARY_B).all())                                         # rows of no group are not touched
    assert torch.equal(src[:k], ref_src[:k]) and bool((src[k:] == CANARY_I).all())
    again, keep2, src2 = nms(d, thr, score, cap=cap, out=_nms_out(B, d.n_classes, cap_in, rows=None if cap is None else total + 5))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[:5], got[:5])) and torch.equal(keep2.cpu(), keep) and torch.equal(src2.cpu(), src)
    return total, ref, ref_keep


# candidates per group: 1; 63 / 64 / 65 (a tile of lanes); 1023 / 1024 (the LDS tile, its last flag bit) / 1025 (the general path)
@pytest.mark.parametrize('nd', [1, 63, 64, 65, 1023, 1024, 1025])
def test_nms_at_the_group_sizes_that_change_the_path(nd):
    """B = 2, C = 3: video 0 holds nd candidates of class 0 and 5 of class 2 (class 1 is empty), video 1 nd of class 1 and one of class 2"""
    det = candidates(nd, [{0: nd, 2: 5}, {1: nd, 2: 1}], 3, span=max(20.0, nd / 8.0))
    assert int(det.total) == 2 * nd + 6
    kept, _, keep = _nms_checked(det, 0.5, 'max')
    assert nd < 63 or 0 < kept < int(det.total)
    kept_mean, _, keep_mean = _nms_checked(det, 0.3, 'mean')
    assert nd < 63 or (kept_mean < kept and not torch.equal(keep, keep_mean))


@pytest.mark.parametrize('score', ['max', 'mean'])
@pytest.mark.parametrize('thr', [0.0, 0.5, 1.0])
def test_nms_thresholds_and_score_columns(thr, score):
    det = candidates(7, [{0: 65, 1: 200}, {}, {1: 130, 3: 2}], 4, span=40.0)
    kept, _, _ = _nms_checked(det, thr, score)
    assert (kept == int(det.total)) == (thr == 1.0)


def test_nms_empty_batch_overflown_input_and_small_cap_out():
    from cfn_hip.detections import Detections
    none = fx.make_det([[], [], []], 4)
    assert _nms_checked(none, 0.5)[0] == 0
    det = candidates(8, [{0: 70, 2: 40}, {1: 90}], 3, span=30.0)
    total, ref, _ = _nms_checked(det, 0.5, cap=11)                                       # rows >= cap_out are not written, the counts are true
    assert total > 11 and ref.offsets.tolist()[-1] == total
    # an input whose decode overflowed its cap: offsets count 200 rows, 150 were written; the rows behind cap are no candidates
    over = Detections(det.seg[:150].contiguous(), det.frames[:150].contiguous(), det.score[:150].contiguous(), det.offsets, det.total, 3, 150)
    kept, ref, keep = _nms_checked(over, 0.5)
    assert int(over.total) == 200 and keep.numel() == 150 and ref.offsets.tolist()[1] == int(keep[:110].sum()) and kept == int(keep.sum())
    # buffers longer than cap (out= of a decode): only the first cap rows are candidates
    longer = Detections(det.seg, det.frames, det.score, det.offsets, det.total, 3, 150)
    assert _nms_checked(longer, 0.5)[0] == kept


def test_nms_chain_and_level_order_ties():
    """the hand cases of test_proposals_cpu.py on the device: the chain (a suppressed candidate suppresses nothing) and the nested pair
    whose shared maximum leaves the choice to the level order"""
    from cfn_hip.detections import propose
    chain = fx.make_det([[(0, 0, 10, 0.9, 0.1), (0, 4, 14, 0.8, 0.2), (0, 8, 18, 0.7, 0.3)]], 1)
    assert _nms_checked(chain, 0.4)[2].tolist() == [1, 0, 1] and _nms_checked(chain, 0.45)[2].tolist() == [1, 1, 1]
    assert _nms_checked(chain, 0.1)[2].tolist() == [1, 0, 0] and _nms_checked(chain, float(np.float64(6) / np.float64(14)))[2].tolist() == [1, 1, 1]
    p = torch.zeros(1, 1, 12)
    p[0, 0, 2:10] = 0.4
    p[0, 0, 4:7] = 0.9
    valid = torch.tensor([12], dtype=torch.int32)
    for levels, want in (((0.8, 0.3), [4, 6, 3]), ((0.3, 0.8), [2, 9, 8])):
        n, cand, level = _levels_checked(p, valid, torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), levels)
        assert n == 2 and cand.score[:n, 0].cpu().tolist() == [float(np.float32(0.9))] * 2
        out = propose(p.to(DEV), valid.to(DEV), levels=levels, nms_thr=0.3)
        assert out.check() == 1 and out.frames[0].cpu().tolist() == want
        assert propose(p.to(DEV), valid.to(DEV), levels=levels, nms_thr=0.4).check() == 2
    assert propose(p.to(DEV), valid.to(DEV), levels=(0.3, 0.8), nms_thr=0.3, score='mean').frames[0].cpu().tolist() == [4, 6, 3]


def test_nms_ranks_nan_scores_as_minus_infinity_on_both_paths():
    """rule N2 with NaN scores, which no decode gives: a NaN ranks as -inf, behind every finite score and in row order among its like, so
    the ranks stay a permutation.  A group of 65 (the lane-tile edge, LDS path) and one of 1025 (the workspace path) with NaN at rows 0, 63,
    64 and the last row.  Row 0 lies apart from everything: kept.  The last row repeats the segment of row 1, finite and apart from the
    rest: suppressed.  nms_reference spells the NaN rule and is the oracle"""
    det = candidates(11, [{0: 65, 1: 1025}], 2, span=130.0)
    seg, score = det.seg.clone(), det.score.clone()
    nan_rows = []
    for d0, nd in ((0, 65), (65, 1025)):
        seg[d0, 1:] = torch.tensor([1000.0, 1010.0], dtype=torch.float64)
        seg[d0 + 1, 1:] = seg[d0 + nd - 1, 1:] = torch.tensor([2000.0, 2010.0], dtype=torch.float64)
        nan_rows += sorted({d0, d0 + 63, d0 + 64, d0 + nd - 1})
    score[nan_rows] = float('nan')
    det = det._replace(seg=seg, score=score)
    kept, ref, keep = _nms_checked(det, 0.5)
    assert 0 < kept < int(det.total)
    of_nan = keep[nan_rows]
    assert int(of_nan.sum()) >= 2 and int((of_nan == 0).sum()) >= 2                      # per group: at least one NaN row kept, one suppressed
    assert keep[[0, 65]].tolist() == [1, 1] and keep[[1, 66]].tolist() == [1, 1] and keep[[64, 1089]].tolist() == [0, 0]


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_golden_labels_round_trip_through_both_kernels(name):
    """ops.seg_labels(batch) decoded at levels (0.75, 0.5, 0.25): three identical copies; NMS at 0.5 leaves decode(thr=0.5) row for row, and
    its rows rasterise back to the labels, which are the reference's arrays"""
    from cfn_hip.detections import decode, decode_levels, nms
    from cfn_hip.seglabels import collate_seg
    split, idx, labels, masks = sf.batch(name)
    sl = collate_seg([sf.seglabel(i, split) for i in idx]).to(DEV)
    lab, mask, valid = sl.dense()
    start = sl.window[:, 0].contiguous()
    one = decode(lab, valid, sl.fps, start, 0.5)
    n = one.check()
    cand, level = decode_levels(lab, valid, sl.fps, start, (0.75, 0.5, 0.25))
    assert cand.check() == 3 * n > 0 and torch.bincount(level[:3 * n].long(), minlength=3).tolist() == [n, n, n]
    out, keep, src = nms(cand, 0.5)
    assert out.check() == n and torch.equal(out.offsets, one.offsets) and not level[src[:n].long()].any()
    assert all(torch.equal(_bits(a[:n]), _bits(b[:n])) for a, b in zip(out[:3], one[:3]))
    lab2, mask2, valid2 = out.as_seg_labels(sl.fps, sl.window, sl.t_max).dense()
    assert torch.equal(lab2, lab) and torch.equal(mask2, mask) and torch.equal(valid2, valid)
    assert int((lab2.cpu().numpy() != labels).sum()) == 0


def _propose_out(B, C, K, TL):
    from cfn_hip import ops
    return _levels_out(B, C, K, TL), _nms_out(B, C, ops.decode_segments_levels_cap(B, C, K, TL))


@pytest.mark.capture
def test_propose_with_out_allocates_nothing_and_replays_on_new_data():
    from cfn_hip.detections import levels_tensor, propose
    B, C, TL = 3, 7, 200
    cases = [(random_probs(31 + i, B, C, TL),) + _meta(B, TL) for i in range(2)]
    levels = levels_tensor(LEVELS5, C, DEV)
    static = [t.to(DEV).clone() for t in cases[0]]
    out = _propose_out(B, C, 5, TL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        propose(*static, levels, 0.5, 'max', 1, 2, out=out)      # warm-up outside the capture
    side.synchronize()
    before, held = torch.cuda.memory_stats()['allocation.all.allocated'], torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode('error')
    try:
        propose(*static, levels, 0.5, 'max', 1, 2, out=out)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before and torch.cuda.memory_allocated() == held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = propose(*static, levels, 0.5, 'max', 1, 2, out=out)
    assert all(g is o for g, o in zip(got[:5], out[1][:5]))
    totals = []
    for case in cases:
        for dst, src in zip(static, case):
            dst.copy_(src.to(DEV))
        for o, v in zip(out[1][:5], (CANARY_F, CANARY_I, CANARY_F, CANARY_I, CANARY_I)):
            o.fill_(v)
        graph.replay()
        torch.cuda.synchronize()
        ref = propose(*case, LEVELS5, 0.5, 'max', 1, 2, reference=True)
        _same_records(got, ref, int(ref.total))
        totals.append(int(ref.total))
    assert totals[0] != totals[1] and min(totals) > 0


def test_meter_on_a_post_nms_batch():
    """SegmentAPMeter.add of propose()'s result against ap_reference over the reference's proposals: tp, match and the stores bit-equal,
    ap within 1 fp32 ulp (the criterion of test_hip_segap.py); a growing meter told levels=K reserves K times the rows and agrees"""
    from test_hip_segap import _meter_checked
    from cfn_hip.detections import propose
    from cfn_hip.segap import SegmentAPMeter
    B, C, TL = 3, 6, 160
    probs = random_probs(41, B, C, TL)
    valid, fps, start = _meta(B, TL)
    det = propose(probs, valid, fps, start, LEVELS5, 0.6, reference=True)
    dev = propose(probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), LEVELS5, 0.6)
    n = det.check()
    assert dev.check() == n > 20 and all(torch.equal(_bits(a[:n].cpu()), _bits(b[:n])) for a, b in zip(dev[:3], det[:3]))
    # ground truth: the segments a single decode at 0.4 finds, moved by a frame, so that levels and thresholds tell true from false
    from cfn_hip.detections import decode_reference
    g = decode_reference(probs, valid, fps, start, 0.4)
    gt = fx.make_gt([[(int(c), s + 1.0 / 24.0, e) for c, s, e in g.seg[int(g.offsets[b]):int(g.offsets[b + 1])].tolist()] for b in range(B)],
                    fps.tolist(), [[int(s), int(v)] for s, v in zip(start, valid)], C, TL)
    tiou = (0.3, 0.5, 0.7, 0.9)
    per_class = int(torch.bincount(det.seg[:n, 0].long(), minlength=C).max())
    assert per_class > (TL + 1) // 2 // 8                                                # (post-NMS groups of several rows)
    fixed, ref, (ap, mp) = _meter_checked([(det, gt)], C, tiou, capacity=per_class + 3)
    assert 0.0 < float(mp[0]) and len(set(ref['batches'][0][0].tolist())) > 2

    class Small(SegmentAPMeter):
        MIN_CAPACITY = 4
    grow = Small(DEV, C, tiou)
    grow.add(dev, gt.to(DEV), levels=5)
    assert grow._bound == min(B * 5 * ((TL + 1) // 2), dev.cap)
    a2, m2 = grow.value()
    assert torch.equal(a2, torch.from_numpy(ap)) and torch.equal(m2, torch.from_numpy(mp)) and torch.equal(grow.counts, fixed.counts)
    with pytest.raises(ValueError, match='levels'):
        grow.add(dev, gt.to(DEV), levels=0)


def test_train_fine_with_levels_feeds_the_writers_proposals_to_the_meter(tmp_path, monkeypatch):
    """run() with a writer AND a meter, the writer with levels: the file holds propose() of the validation probs, and the meter is handed
    that very batch with levels=K (its own, different options are not used).  The same run without any of the options gives the same
    losses and the same existing log line, bit for bit"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _run, _same_file
    from test_hip_segap import _line, _spy_meter, _ulps
    from cfn_hip.detections import DetectionWriter, epoch_path, propose
    from cfn_hip.seglabels import collate_seg
    from cfn_hip.segap import ap_reference
    crop, tiou, levels = 64, (0.1, 0.5), (0.6, 0.5, 0.4)
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.fine_collate_u8)
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), 0.9, 2, 2, levels=levels, nms=0.5)
    meter = _spy_meter(tiou, thr=0.9, max_gap=0, min_len=7, levels=(0.9,), nms=0.1)
    fed = []
    real_add = meter.add
    monkeypatch.setattr(meter, 'add', lambda det, labels, **kw: (fed.append((det, kw)), real_add(det, labels, **kw))[1])
    kept = []
    real_wadd = writer.add
    monkeypatch.setattr(writer, 'add', lambda *a, **k: (lambda d: (kept.append(d), d)[1])(real_wadd(*a, **k)))
    losses, lines, val = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, writer, max_epochs=4, save_model=str(tmp_path / 'm_'),
                              segment_ap=meter)
    assert len(fed) == len(kept) == 3 and all(f[0] is k and f[1] == {'levels': 3} for f, k in zip(fed, kept))
    rows, batches = [], []
    for i, (probs, valid) in enumerate(val):
        fps, start, _ = _SegVideos.meta(i)
        lab = collate_seg([_SegVideos(3, crop, False)[i][1]])
        det = propose(probs, valid, lab.fps, lab.window[:, 0].contiguous(), levels, 0.5, 'max', 2, 2, reference=True)
        rows.append({'video': 'vid%d' % i, 'unit': 's', 'segments': det.tolist()[0]})
        batches.append((det, lab))
    n = _same_file(epoch_path(writer.path, 4), rows)
    print('train_fine: %d proposals in 3 validation videos' % n)
    assert n > 0
    ref = ap_reference(batches, 157, tiou)
    ap, mp = meter.last
    assert _ulps(ap.numpy(), ref['ap']).max() <= 1 and _ulps(mp.numpy(), ref['map']).max() <= 1
    assert len(lines) == 2 and lines[1] == _line(4, tiou, mp)
    losses0, lines0, _ = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / 'n_'))
    assert losses0 == losses and lines0 == lines[:1]
