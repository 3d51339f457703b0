"""Activity proposals, host side (cfn_hip/detections.py): decode_levels_reference and nms_reference on hand-written cases with the expected
result typed out, the level decode against K single decodes, the properties of the kept set, the round trip through the reference's own
label arrays (tests/golden/seg_labels.npz), the C ABI of cfn_decode_segments_levels / cfn_nms_segments, the refusals of the ops, and the
writer's, the meter's and the scripts' new options.  Every comparison is exact: the rules hold integers, fp32 copies and fp64 with one
division.  No GPU."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import seg_fixture as sf
import segap_fixture as fx
from proposals_fixture import LEVELS5, random_probs as _random_probs


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _same_det(a, b, rows=None):
    """two Detections equal bit for bit over their first `rows` rows (default: total), and in offsets / total"""
    n = int(a.total.item()) if rows is None else rows
    assert a.offsets.tolist() == b.offsets.tolist() and a.total.tolist() == b.total.tolist()
    assert torch.equal(a.seg[:n].view(torch.int64), b.seg[:n].view(torch.int64)) and torch.equal(a.frames[:n], b.frames[:n])
    assert torch.equal(a.score[:n].contiguous().view(torch.int32), b.score[:n].contiguous().view(torch.int32))
    return n


def _nms(rows, thr, score='max', C=1, **kw):
    """nms_reference of ONE video's (class, start, end, max, mean) rows (given in (class, start) order) -> (kept [(start, end)], keep list)"""
    from cfn_hip.detections import nms_reference
    det = fx.make_det([rows], C)
    out, keep, src = nms_reference(det, thr, score, **kw)
    n = out.check()
    assert keep.dtype == torch.uint8 and src.dtype == torch.int32 and out.offsets.tolist() == [0, n] and int(keep.sum()) == n
    assert src[:n].tolist() == torch.nonzero(keep).flatten().tolist()                  # N5 / N6: input order
    assert torch.equal(out.seg[:n], det.seg[src[:n].long()]) and torch.equal(out.score[:n], det.score[src[:n].long()])
    return [(float(s), float(e)) for _, s, e in out.seg[:n].tolist()], keep.tolist()


def test_a_nan_score_ranks_as_minus_infinity_and_ties_go_to_the_lower_row():
    """One group, nms_thr 0.5, neighbours shifted by one second overlap with tIoU 9/11.  N2 orders the rows 1, 2 (0.5 twice: the lower row
    first), then the keys of -inf in row order: 0, 3, 4, 5, 6 (NaN and a true -inf are one key).  N4: 1 is kept and suppresses 2 and 0;
    3 is kept -- a NaN row can be kept -- and suppresses 4; 5 (-inf) is kept and suppresses 6, the NaN row behind it"""
    nan, ninf = float('nan'), float('-inf')
    rows = [(0, 0, 10, nan, nan), (0, 1, 11, 0.5, 0.5), (0, 2, 12, 0.5, 0.5), (0, 20, 30, nan, nan), (0, 21, 31, nan, nan),
            (0, 39, 49, ninf, ninf), (0, 40, 50, nan, nan)]
    from cfn_hip.detections import nms_reference
    det = fx.make_det([rows], 1)
    for col in ('max', 'mean'):
        out, keep, src = nms_reference(det, 0.5, col)
        assert keep.tolist() == [0, 1, 0, 1, 0, 1, 0] and out.check() == 3 and src.tolist() == [1, 3, 5]
        assert out.seg[:, 1:].tolist() == [[1.0, 11.0], [20.0, 30.0], [39.0, 49.0]]
        assert torch.equal(out.score.view(torch.int32), det.score[[1, 3, 5]].view(torch.int32))      # (a NaN is copied bit for bit too)
    assert nms_reference(det, 0.9)[1].tolist() == [1] * 7                               # 9/11 = 0.82 is not above 0.9: nothing falls
    # as +inf, or compared raw (never above, never equal), row 0 would be walked before row 1 and kept
    assert nms_reference(fx.make_det([rows[:2]], 1), 0.5)[1].tolist() == [0, 1]


def test_the_chain_separates_greedy_from_suppressed_by_any_higher_ranked():
    """A (0, 10) 0.9, B (4, 14) 0.8, C (8, 18) 0.7: tIoU AB = BC = 6/14, AC = 2/18.  At 0.4 B falls to A, and C, which only B could have
    suppressed, is kept (N4: a suppressed candidate suppresses nothing)"""
    from cfn_hip.segap import tiou_reference
    f = np.float64
    assert tiou_reference(f(0), f(10), f(4), f(14)) == f(6) / f(14) == tiou_reference(f(4), f(14), f(8), f(18))
    assert tiou_reference(f(0), f(10), f(8), f(18)) == f(2) / f(18)
    chain = [(0, 0, 10, 0.9, 0.1), (0, 4, 14, 0.8, 0.2), (0, 8, 18, 0.7, 0.3)]
    assert _nms(chain, 0.4) == ([(0.0, 10.0), (8.0, 18.0)], [1, 0, 1])
    assert _nms(chain, 0.45) == ([(0.0, 10.0), (4.0, 14.0), (8.0, 18.0)], [1, 1, 1])    # 6/14 = 0.4286 is not above 0.45
    assert _nms(chain, 0.1) == ([(0.0, 10.0)], [1, 0, 0])                               # 2/18 = 0.11 is above 0.1
    # the other score column reverses the walk: C first, B falls to C, A is kept
    assert _nms(chain, 0.4, 'mean') == ([(0.0, 10.0), (8.0, 18.0)], [1, 0, 1])
    # the threshold is strict: a tIoU equal to nms_thr does not suppress
    assert _nms(chain, float(np.float64(6) / np.float64(14)))[1] == [1, 1, 1]
    assert _nms(chain, float(np.nextafter(np.float64(6) / np.float64(14), 0.0)))[1] == [1, 0, 1]


def test_thresholds_0_and_1_and_groups():
    rows = [(0, 0, 10, 0.9, 0.5), (0, 0, 10, 0.8, 0.6), (0, 9, 20, 0.7, 0.7), (0, 10, 20, 0.6, 0.8), (1, 0, 10, 0.5, 0.9)]
    assert _nms(rows, 1.0, C=2)[1] == [1, 1, 1, 1, 1]                                   # N7: an exact duplicate has tIoU 1.0, not above 1
    # 0: anything that overlaps a kept candidate goes; touching segments (inter = 0) and another class do not overlap
    assert _nms(rows, 0.0, C=2)[1] == [1, 0, 0, 1, 1]
    assert _nms(rows, 0.999, C=2)[1] == [1, 0, 1, 1, 1]                                 # the duplicate collapses to the first in the order
    assert _nms(rows, 0.999, 'mean', C=2)[1] == [0, 1, 1, 1, 1]
    with pytest.raises(ValueError):
        _nms(rows, 1.5, C=2)
    with pytest.raises(ValueError):
        _nms(rows, 0.5, 'median', C=2)
    # two videos: groups never cross a video, offsets are recomputed
    from cfn_hip.detections import nms_reference
    det = fx.make_det([rows[:2], rows[:2] + rows[4:]], 2)
    out, keep, src = nms_reference(det, 0.5)
    assert keep.tolist() == [1, 0, 1, 0, 1] and out.offsets.tolist() == [0, 1, 3] and out.total.tolist() == [3] and src.tolist() == [0, 2, 4]
    cut, keep2, src2 = nms_reference(det, 0.5, cap=2)                                   # a cap keeps the prefix and the true counts
    assert cut.cap == 2 and cut.offsets.tolist() == [0, 1, 3] and keep2.tolist() == keep.tolist() and src2.tolist() == [0, 2]
    assert torch.equal(cut.seg, out.seg[:2])
    with pytest.raises(RuntimeError, match='cap = 2'):
        cut.check()
    empty = fx.make_det([[], []], 2)
    out, keep, src = nms_reference(empty, 0.5)
    assert out.check() == 0 and out.offsets.tolist() == [0, 0, 0] and keep.numel() == 0


def _bump():
    """one class, 12 frames, a bump whose top is the tight segment 4..6 and whose foot is 2..9"""
    p = torch.zeros(1, 1, 12)
    p[0, 0, 2:10] = 0.4
    p[0, 0, 4:7] = 0.9
    return p, torch.tensor([12], dtype=torch.int32)


def test_score_ties_are_resolved_by_the_level_order_both_ways():
    """nested candidates share their maximum (N2): tIoU of 4..6 and 2..9 is 3/8, so at nms_thr 0.3 one of the two goes -- the one whose
    level the caller listed later"""
    from cfn_hip.detections import decode_levels_reference, nms_reference, propose
    p, valid = _bump()
    for levels, want_frames, want_level in (((0.8, 0.3), [4, 6, 3], 0), ((0.3, 0.8), [2, 9, 8], 0)):
        cand, level = decode_levels_reference(p, valid, levels=levels)
        assert cand.check() == 2 and level.tolist() == [0, 1] and cand.score[:, 0].tolist() == [float(np.float32(0.9))] * 2
        out, keep, src = nms_reference(cand, 0.3)
        assert out.check() == 1 and out.frames[0].tolist() == want_frames and int(level[src[0]]) == want_level and keep.tolist() == [1, 0]
        assert nms_reference(cand, 0.4)[0].check() == 2                                # 3/8 is not above 0.4
        _same_det(propose(p, valid, levels=levels, nms_thr=0.3, reference=True), out)
    # under score='mean' the tight segment (mean 0.9) wins whatever the level order
    cand, level = decode_levels_reference(p, valid, levels=(0.3, 0.8))
    assert nms_reference(cand, 0.3, 'mean')[0].frames[0].tolist() == [4, 6, 3]


def test_level_decode_is_k_single_decodes_merged():
    """3 x 5 x 130 at 5 levels: every candidate row is the row of the single decode at its level, in (b, c, k, t0) order"""
    from cfn_hip.detections import decode_levels_reference, decode_reference
    B, C, TL = 3, 5, 130
    p = _random_probs(11, B, C, TL)
    valid = torch.tensor([TL, TL - 30, 77], dtype=torch.int32)
    fps, start = torch.tensor([24.0, 29.97, 12.5], dtype=torch.float64), torch.tensor([0, 17, 12345], dtype=torch.int32)
    for max_gap, min_len in ((0, 1), (2, 3)):
        cand, level = decode_levels_reference(p, valid, fps, start, LEVELS5, max_gap, min_len)
        singles = [decode_reference(p, valid, fps, start, thr, max_gap, min_len) for thr in LEVELS5]
        n = cand.check()
        assert n == sum(s.check() for s in singles) > 40 and cand.cap == n and level.dtype == torch.uint8
        keys = [(b, int(cand.seg[i, 0]), int(level[i]), int(cand.frames[i, 0])) for b in range(B) for i in range(int(cand.offsets[b]), int(cand.offsets[b + 1]))]
        assert keys == sorted(keys) and len(set(keys)) == n                             # L3
        for k, s in enumerate(singles):
            mine = torch.nonzero(level[:n] == k).flatten()
            assert mine.numel() == s.check()
            _same_det(type(cand)(cand.seg[mine], cand.frames[mine], cand.score[mine], s.offsets, s.total, C, n), s)      # L1, L2
    # per-class levels, unsorted; K = 1 is decode_reference bit for bit (L4)
    lv = torch.tensor([[0.5, 0.2, 0.7]] * 2 + [[0.9, 0.1, 0.3]] * 3)
    cand, level = decode_levels_reference(p, valid, fps, start, lv)
    for c in range(C):
        for k in range(3):
            rows = torch.nonzero((cand.seg[:, 0] == c) & (level == k)).flatten()
            one = decode_reference(p[:, c:c + 1].contiguous(), valid, fps, start, float(lv[c, k]))
            assert torch.equal(cand.frames[rows], one.frames[:one.check()])
    one, level = decode_levels_reference(p, valid, fps, start, (0.35,), 1, 2)
    ref = decode_reference(p, valid, fps, start, 0.35, 1, 2)
    assert _same_det(one, ref) == ref.check() and one.cap == ref.cap and not level.any()
    cut, lcut = decode_levels_reference(p, valid, fps, start, LEVELS5, cap=7)
    full, lfull = decode_levels_reference(p, valid, fps, start, LEVELS5)
    assert cut.cap == 7 and tuple(cut.seg.shape) == (7, 3) and _same_det(cut, full, rows=7) == 7 and torch.equal(lcut, lfull[:7])
    for bad in ((), (0.5,) * 17, torch.zeros(4, 2), torch.zeros(5)):
        with pytest.raises(ValueError, match='levels'):
            decode_levels_reference(p, valid, levels=bad)


@pytest.mark.parametrize('score', ['max', 'mean'])
@pytest.mark.parametrize('thr', [0.0, 0.3, 0.5, 0.7, 1.0])
def test_the_kept_set_is_what_greedy_nms_promises(thr, score):
    """kept rows are pairwise at or below nms_thr; every dropped row has a kept, earlier-ranked row above it; groups are independent"""
    from cfn_hip.detections import SCORE_COLUMNS, decode_levels_reference, nms_reference
    from cfn_hip.segap import tiou_reference
    B, C, TL = 3, 5, 130
    p = _random_probs(12, B, C, TL)
    cand, _ = decode_levels_reference(p, torch.tensor([TL, TL, 99], dtype=torch.int32), levels=LEVELS5)
    out, keep, src = nms_reference(cand, thr, score)
    n, col = cand.check(), SCORE_COLUMNS[score]
    seg, sc, keep = cand.seg.numpy(), cand.score.numpy(), keep.numpy().astype(bool)
    vid = np.searchsorted(cand.offsets.numpy()[1:], np.arange(n), side='right')
    dropped = 0
    for i in range(n):
        same = [j for j in range(n) if j != i and vid[j] == vid[i] and seg[j, 0] == seg[i, 0]]
        v = {j: tiou_reference(seg[j, 1], seg[j, 2], seg[i, 1], seg[i, 2]) for j in same}
        if keep[i]:
            assert all(v[j] <= thr for j in same if keep[j])
        else:
            dropped += 1
            assert any(keep[j] and v[j] > thr and (sc[j, col] > sc[i, col] or (sc[j, col] == sc[i, col] and j < i)) for j in same)
    assert out.check() == n - dropped and (dropped > 0) == (thr < 1.0)
    assert out.offsets.tolist() == [int(keep[:o].sum()) for o in cand.offsets.tolist()]


def test_golden_arrays_round_trip_through_levels_and_nms():
    """the 126 label arrays decoded at levels (0.75, 0.5, 0.25): three identical copies with tIoU exactly 1; after NMS at 0.5 they are
    decode_reference(thr=0.5) row for row (761 segments), and rasterise back to the arrays"""
    from cfn_hip.detections import decode_levels_reference, decode_reference, nms_reference
    from cfn_hip.seglabels import SegLabel
    recs = sf.records()
    arrays = segments = 0
    for i in range(len(recs)):
        for kind in ('full',) + sf.SPLITS:
            want, sl = sf.expected(i, kind), sf.seglabel(i, kind)
            arrays += 1
            if sl.length == 0:
                continue
            args = (torch.from_numpy(want.copy())[None], torch.tensor([sl.length], dtype=torch.int32), torch.tensor([sl.fps], dtype=torch.float64),
                    torch.tensor([sl.start], dtype=torch.int32))
            cand, level = decode_levels_reference(*args, levels=(0.75, 0.5, 0.25))
            one = decode_reference(*args, 0.5)
            n = one.check()
            assert cand.check() == 3 * n and np.bincount(level[:3 * n].numpy(), minlength=3).tolist() == [n, n, n]
            out, keep, src = nms_reference(cand, 0.5)
            assert _same_det(out, one) == n and (n == 0 or not level[src.long()].any())  # the first copy of each: level 0
            got = SegLabel(out.seg[:n].numpy(), sl.fps, sl.start, sl.length).dense_reference()
            assert int((got != want).sum()) == 0, (recs[i]['vid'], kind)
            segments += n
    assert (arrays, segments) == (126, 761)


def test_entry_points_are_declared_exported_and_check_their_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    ret, at, dts = protos['cfn_decode_segments_levels']
    assert ret is ctypes.c_int and len(at) == 20 and at[-1] is ctypes.c_void_p and at[-2] is ctypes.c_long and at[12:18] == [ctypes.c_int] * 6
    assert dts[:12] == [torch.float32, torch.int32, torch.float64, torch.int32, torch.float32, torch.float64, torch.int32, torch.float32, torch.uint8,
                        torch.int32, torch.int32, None]
    ret, at, dts = protos['cfn_nms_segments']
    assert ret is ctypes.c_int and len(at) == 19 and at[12:15] == [ctypes.c_int] * 3 and at[15] is ctypes.c_double and at[16:18] == [ctypes.c_long] * 2
    assert dts[:12] == [torch.float64, torch.int32, torch.float32, torch.int32, torch.float64, torch.int32, torch.float32, torch.int32, torch.int32,
                        torch.uint8, torch.int32, None]
    assert protos['cfn_decode_segments_levels_workspace_bytes'][:2] == (ctypes.c_long, [ctypes.c_int] * 4)
    assert protos['cfn_nms_segments_workspace_bytes'][:2] == (ctypes.c_long, [ctypes.c_int, ctypes.c_int, ctypes.c_long])
    assert protos['cfn_nms_det_tile'][:2] == (ctypes.c_int, [])
    raw = ctypes.CDLL(cfn_hip.LIB_PATH)
    assert all(hasattr(raw, n) for n in ('cfn_decode_segments_levels', 'cfn_decode_segments_levels_workspace_bytes', 'cfn_nms_segments',
                                         'cfn_nms_segments_workspace_bytes', 'cfn_nms_det_tile'))
    lib = cfn_hip.load()
    from cfn_hip import ops
    assert lib.cfn_nms_det_tile() == ops.NMS_DET_TILE == 1024
    q = cfn_hip.query
    # the rows' bit masks (8 bytes per 64 frames) and B * C * K + 1 counts; K = 1 is cfn_decode_segments' workspace
    assert q('cfn_decode_segments_levels_workspace_bytes', 2, 157, 5, 640) == 2 * 157 * 5 * 10 * 8 + (2 * 157 * 5 + 1) * 4
    assert q('cfn_decode_segments_levels_workspace_bytes', 2, 157, 1, 640) == q('cfn_decode_segments_workspace_bytes', 2, 157, 640)
    for shape in ((0, 157, 1, 8), (1, 0, 1, 8), (1, 157, 0, 8), (1, 157, 17, 8), (1, 157, 1, 0), (65536, 1, 1, 8), (1, 157, 1, 65537), (4096, 157, 16, 640)):
        assert q('cfn_decode_segments_levels_workspace_bytes', *shape) == -1, shape
    # B * C + 1 counts, cap_in ranks, cap_in flag bytes rounded up to 8
    assert q('cfn_nms_segments_workspace_bytes', 2, 157, 1001) == (2 * 157 + 1 + 1001) * 4 + 1008
    for shape in ((0, 157, 8), (1, 0, 8), (65536, 1, 8), (1, 65536, 8), (1, 157, 0), (1, 157, 1 << 31)):
        assert q('cfn_nms_segments_workspace_bytes', *shape) == -1, shape
    buf = (ctypes.c_double * 8)()
    p = [ctypes.addressof(buf)] * 12
    assert lib.cfn_decode_segments_levels(*([None] * 12), 1, 157, 3, 8, 0, 1, 628, None) == 1 and 'null' in cfn_hip.last_error()
    for B, C, K, TL, gap, mlen, cap, word in ((0, 157, 1, 8, 0, 1, 1, 'shape'), (1, 157, 0, 8, 0, 1, 1, 'levels'), (1, 157, 17, 8, 0, 1, 1, 'levels'),
                                              (4096, 157, 16, 640, 0, 1, 1, 'large'), (1, 157, 3, 8, -1, 1, 1, 'max_gap'), (1, 157, 3, 8, 0, 0, 1, 'min_len'),
                                              (1, 157, 3, 8, 0, 1, 0, 'cap'), (1, 157, 3, 8, 0, 1, 1 << 31, 'cap')):
        assert lib.cfn_decode_segments_levels(*p, B, C, K, TL, gap, mlen, cap, None) == 1, (B, C, K, TL, gap, mlen, cap)      # refused before any launch
        assert 'cfn_decode_segments_levels' in cfn_hip.last_error() and word in cfn_hip.last_error(), cfn_hip.last_error()
    assert lib.cfn_nms_segments(*([None] * 12), 1, 157, 0, 0.5, 8, 8, None) == 1 and 'null' in cfn_hip.last_error()
    for B, C, col, thr, cap_in, cap_out, word in ((0, 157, 0, 0.5, 8, 8, 'shape'), (1, 65536, 0, 0.5, 8, 8, 'shape'), (1, 157, 0, 0.5, 0, 8, 'shape'),
                                                  (1, 157, 0, 0.5, 8, 0, 'cap_out'), (1, 157, 2, 0.5, 8, 8, 'score_col'), (1, 157, 0, -0.1, 8, 8, 'nms_thr'),
                                                  (1, 157, 0, 1.5, 8, 8, 'nms_thr'), (1, 157, 0, float('nan'), 8, 8, 'nms_thr'),
                                                  (1, 157, 0, 0.5, 8, 8, 'outputs must not be the inputs')):
        assert lib.cfn_nms_segments(*p, B, C, col, thr, cap_in, cap_out, None) == 1, (B, C, col, thr, cap_in, cap_out)
        assert 'cfn_nms_segments' in cfn_hip.last_error() and word in cfn_hip.last_error(), cfn_hip.last_error()
    csrc = os.path.join(os.path.dirname(cfn_hip.LIB_PATH), '..', 'csrc')
    src = open(os.path.join(csrc, 'segnms.hip')).read()
    assert 'getenv' not in src and 'atomicAdd' not in src and 'hipMalloc' not in src


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    _lib()
    from cfn_hip import ops
    from cfn_hip.detections import decode_levels, nms, propose
    ok = dict(probs=torch.zeros(2, 5, 16), valid_t=torch.full((2,), 16, dtype=torch.int32), fps=torch.ones(2, dtype=torch.float64),
              start=torch.zeros(2, dtype=torch.int32), levels=torch.full((5, 3), 0.5))
    with pytest.raises(RuntimeError, match='probs is on cpu'):           # everything well formed: what is left is the device
        ops.decode_segments_levels(**ok)
    with pytest.raises(RuntimeError, match='no CPU path'):
        decode_levels(ok['probs'], ok['valid_t'], levels=(0.5, 0.3))
    with pytest.raises(RuntimeError, match='no CPU path'):
        propose(ok['probs'], ok['valid_t'])
    bad = [('probs', dict(probs=ok['probs'].double())), ('probs', dict(probs=ok['probs'][:, :, ::2])), ('levels', dict(levels=0.5)),
           ('levels', dict(levels=torch.zeros(5))), ('levels', dict(levels=torch.zeros(4, 3))), ('levels', dict(levels=torch.zeros(5, 17))),
           ('levels', dict(levels=torch.zeros(5, 3, dtype=torch.float64))), ('valid_t', dict(valid_t=ok['valid_t'].long())),
           ('fps', dict(fps=ok['fps'].float())), ('start', dict(start=ok['start'][:1])), ('max_gap', dict(max_gap=-1)), ('min_len', dict(min_len=0)),
           ('cap', dict(cap=0)), ('cap', dict(cap=1 << 31))]
    for word, change in bad:
        with pytest.raises(RuntimeError, match='decode_segments_levels: .*' + word):
            ops.decode_segments_levels(**dict(ok, **change))
    assert ops.decode_segments_levels_cap(2, 5, 3, 16) == 240 == 3 * ops.decode_segments_cap(2, 5, 16)
    with pytest.raises(RuntimeError, match='decode_segments_levels'):
        ops.decode_segments_levels_workspace_bytes(1, 1, 17, 8)
    det, _ = fx.hand_batch()
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.nms_segments(det.seg, det.frames, det.score, det.offsets, 5, 0.5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        nms(det, 0.5)
    with pytest.raises(TypeError):
        nms(det[:5], 0.5)
    with pytest.raises(ValueError, match='score'):
        nms(det, 0.5, 'median')
    with pytest.raises(RuntimeError, match='nms_segments'):
        ops.nms_segments_workspace_bytes(1, 65536, 8)
    from cfn_hip import torchlib as tl
    assert not any('nms' in n or 'levels' in n for tup in (tl.OPERATORS, tl.INPUT_OPERATORS, tl.AUGMENT_OPERATORS, tl.METRIC_OPERATORS,
                                                            tl.FEATURE_OPERATORS, tl.DECODE_OPERATORS, tl.LABEL_OPERATORS) for n in tup)


def test_writer_with_levels_keeps_the_post_nms_batch(tmp_path):
    from cfn_hip.detections import DetectionWriter, decode_reference, propose, read_detections
    p = _random_probs(13, 2, 4, 60)
    valid = torch.tensor([60, 41], dtype=torch.int32)
    w = DetectionWriter(str(tmp_path / 'det.jsonl'), 0.5, 1, 2, levels=LEVELS5, nms=0.4, nms_score='mean')
    assert w.n_levels == 5 and DetectionWriter('x').n_levels == 1 and DetectionWriter('x', levels=torch.zeros(4, 3)).n_levels == 3
    got = w.add(p, valid, None, ['v0', 'v1'], decoder=decode_reference)
    want = propose(p, valid, None, None, LEVELS5, 0.4, 'mean', 1, 2, reference=True)
    assert _same_det(got, want) > 0 and len(w._pending) == 1 and w._pending[0][0] is got            # only the post-NMS batch is kept
    assert w.flush() == 2
    rows = read_detections(w.path)
    assert [r['segments'] for r in rows] == want.tolist() and all(set(r) == {'video', 'unit', 'segments'} for r in rows)      # the format is the same
    assert DetectionWriter('x', levels=LEVELS5).nms == 0.5
    with pytest.raises(ValueError, match='nms'):
        DetectionWriter('x', nms=0.5)
    with pytest.raises(ValueError, match='score'):
        DetectionWriter('x', levels=LEVELS5, nms_score='median')


def test_scripts_forward_the_proposal_flags():
    import train_coarse_fineFEAT as tc
    import train_fine
    parser = argparse.ArgumentParser()
    train_fine.add_detect_args(parser)
    train_fine.seg_ap_arguments(parser)
    off = parser.parse_args(['--detect', 'd.jsonl'])
    assert off.detect_levels is None and off.detect_nms is None and off.detect_nms_score == 'max' and train_fine.detect_levels(off) == {}
    w = train_fine.detect_writer(off)
    assert w.levels is None and w.n_levels == 1 and '--detect-levels' not in train_fine.detect_argv(off)
    on = parser.parse_args(['--detect', 'd.jsonl', '--detect-gap', '1', '--detect-levels', '0.8,0.65,0.5,0.35,0.2', '--detect-nms', '0.45',
                            '--detect-nms-score', 'mean'])
    again = parser.parse_args(train_fine.detect_argv(on))                                 # what a spawned worker parses
    assert vars(again) == vars(on)
    w = train_fine.detect_writer(again)
    assert (w.levels, w.nms, w.nms_score, w.max_gap, w.n_levels) == ([0.8, 0.65, 0.5, 0.35, 0.2], 0.45, 'mean', 1, 5)
    assert train_fine.detect_levels(parser.parse_args(['--detect-levels', '0.6,0.3'])) == {'levels': [0.6, 0.3], 'nms': None, 'nms_score': 'max'}
    with pytest.raises(ValueError, match='--detect-levels'):
        train_fine.detect_levels(parser.parse_args(['--detect-nms', '0.5']))
    assert tc.detect_writer is train_fine.detect_writer and tc.seg_ap_from_args is train_fine.seg_ap_from_args
    import inspect
    assert 'detect_levels(args)' in inspect.getsource(train_fine.seg_ap_from_args)
    for mod in (train_fine, tc):
        assert 'writer=detections' in inspect.getsource(mod.run), mod.__name__


def test_meter_takes_the_proposal_options():
    from cfn_hip.segap import SegmentAPMeter
    import inspect
    p = inspect.signature(SegmentAPMeter.__init__).parameters
    assert (p['levels'].default, p['nms'].default, p['nms_score'].default) == (None, None, 'max')
    assert inspect.signature(SegmentAPMeter.add).parameters['levels'].default == 1
    for kw in ({'nms': 0.5}, {'levels': (0.5, 0.3), 'nms_score': 'median'}):
        with pytest.raises((ValueError, RuntimeError)):
            SegmentAPMeter('cuda', 5, **kw)
