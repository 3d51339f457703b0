"""Activity segments from per-frame scores, host side (cfn_hip/detections.py): decode_reference on hand-written rows with the expected
records typed out, the round trip through the reference's own label arrays (tests/golden/seg_labels.npz: decoding an array and rasterising
the segments again gives the array back, bit for bit), the C ABI of cfn_decode_segments, the refusals of ops.decode_segments, the
Detections batch type, the JSON-lines writer and the scripts' signatures.  No GPU."""
import argparse
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import seg_fixture as sf

NAN, INF = float('nan'), float('inf')


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _f32(*v):
    return [float(np.float32(x)) for x in v]


def _mean(*v):
    """rule 5: the fp64 sum of the fp32 values, divided in fp64, rounded to fp32"""
    return float(np.float32(sum(np.float64(np.float32(x)) for x in v) / np.float64(len(v))))


def _records(rows, valid, thr=0.5, fps=None, start=None, **kw):
    """decode_reference of ONE video whose class rows are `rows` -> [(class, t0, t1, n_active, max, mean, start, end)]"""
    from cfn_hip.detections import decode_reference
    probs = torch.tensor([rows], dtype=torch.float32)
    det = decode_reference(probs, torch.tensor([valid], dtype=torch.int32), None if fps is None else torch.tensor([fps], dtype=torch.float64),
                           None if start is None else torch.tensor([start], dtype=torch.int32), thr, **kw)
    n = det.check()
    assert det.offsets.tolist() == [0, n] and det.n_classes == len(rows)
    assert det.seg.dtype == torch.float64 and det.frames.dtype == torch.int32 and det.score.dtype == torch.float32
    assert det.offsets.dtype == torch.int32 and det.total.dtype == torch.int32 and tuple(det.total.shape) == (1,)
    return [(int(det.seg[i, 0]), int(det.frames[i, 0]), int(det.frames[i, 1]), int(det.frames[i, 2]), float(det.score[i, 0]), float(det.score[i, 1]),
             float(det.seg[i, 1]), float(det.seg[i, 2])) for i in range(n)]


def _same(got, want):
    """records equal; NaN never appears in one, inf compares equal to itself"""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g == tuple(w), (g, w)


def test_runs_at_the_window_edges_and_valid_t():
    a, b = _f32(0.9, 0.8)
    # a run at t = 0; times in frames (fps = 1, start = 0) with the half frame outward
    _same(_records([[0.9, 0.8, 0, 0, 0, 0]], 6), [(0, 0, 1, 2, a, _mean(0.9, 0.8), -0.5, 1.5)])
    # a run ending at valid_t - 1, and the same frames with a longer valid_t
    _same(_records([[0, 0, 0, 0.9, 0.8, 0.9]], 5), [(0, 3, 4, 2, a, _mean(0.9, 0.8), 2.5, 4.5)])
    _same(_records([[0, 0, 0, 0.9, 0.8, 0.9]], 6), [(0, 3, 5, 3, a, _mean(0.9, 0.8, 0.9), 2.5, 5.5)])
    # a run cut by valid_t (frames 2..5 are above the threshold, 4 and 5 are masked), valid_t past the row, valid_t = 0 and below
    _same(_records([[0, 0, 0.9, 0.8, 0.9, 0.9]], 4), [(0, 2, 3, 2, a, _mean(0.9, 0.8), 1.5, 3.5)])
    _same(_records([[0, 0, 0.9, 0.8, 0.9, 0.9]], 99), [(0, 2, 5, 4, a, _mean(0.9, 0.8, 0.9, 0.9), 1.5, 5.5)])
    _same(_records([[0.9] * 6], 0), [])
    _same(_records([[0.9] * 6], -3), [])
    # all active; alternating (every second frame a run of its own: the worst case (TL + 1) // 2)
    _same(_records([[0.8] * 7], 7), [(0, 0, 6, 7, b, _mean(*[0.8] * 7), -0.5, 6.5)])
    _same(_records([[0.9, 0, 0.8, 0, 0.9, 0, 0.8]], 7),
          [(0, 0, 0, 1, a, a, -0.5, 0.5), (0, 2, 2, 1, b, b, 1.5, 2.5), (0, 4, 4, 1, a, a, 3.5, 4.5), (0, 6, 6, 1, b, b, 5.5, 6.5)])
    # seconds: ((start + t0) - 0.5) / fps and ((start + t1) + 0.5) / fps in fp64
    _same(_records([[0, 0.9, 0.8, 0]], 4, fps=29.97, start=100), [(0, 1, 2, 2, a, _mean(0.9, 0.8), (101.0 - 0.5) / 29.97, (102.0 + 0.5) / 29.97)])


def test_comparison_is_strict_fp32_and_per_class():
    h, s = _f32(0.5, 0.6)
    _same(_records([[0.5, 0.6, 0.5]], 3), [(0, 1, 1, 1, s, s, 0.5, 1.5)])                     # a value equal to thr is inactive
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    _same(_records([[0.5, above, 0.5]], 3), [(0, 1, 1, 1, above, above, 0.5, 1.5)])           # one fp32 step above it is active
    # NaN is never active, +inf is; a NaN threshold switches its class off
    _same(_records([[NAN, INF, INF, NAN, 0.6]], 5), [(0, 1, 2, 2, INF, INF, 0.5, 2.5), (0, 4, 4, 1, s, s, 3.5, 4.5)])
    # per-class thresholds: (C,) fp32; order is (class, t0)
    rows = [[0.5, 0.5, 0.0, 0.9], [0.5, 0.5, 0.0, 0.9], [0.5, 0.5, 0.0, 0.9]]
    _same(_records(rows, 4, thr=torch.tensor([0.3, 0.8, NAN])),
          [(0, 0, 1, 2, h, h, -0.5, 1.5), (0, 3, 3, 1, _f32(0.9)[0], _f32(0.9)[0], 2.5, 3.5), (1, 3, 3, 1, _f32(0.9)[0], _f32(0.9)[0], 2.5, 3.5)])


@pytest.mark.parametrize('max_gap', [0, 1, 3])
def test_gap_closing_joins_a_gap_of_exactly_max_gap(max_gap):
    a, b = _f32(0.9, 0.7)
    joined = [0.9] + [0.0] * max_gap + [0.7, 0.0]                                             # a gap of exactly max_gap frames
    t1 = max_gap + 1
    _same(_records([joined], len(joined), max_gap=max_gap), [(0, 0, t1, 2, a, _mean(0.9, 0.7), -0.5, t1 + 0.5)])
    apart = [0.9] + [0.0] * (max_gap + 1) + [0.7, 0.0]                                        # one frame more
    _same(_records([apart], len(apart), max_gap=max_gap), [(0, 0, 0, 1, a, a, -0.5, 0.5), (0, t1 + 1, t1 + 1, 1, b, b, t1 + 0.5, t1 + 1.5)])
    # leading and trailing inactive frames are never part of a run, however short
    _same(_records([[0.0, 0.9, 0.0]], 3, max_gap=max_gap), [(0, 1, 1, 1, a, a, 0.5, 1.5)])


def test_min_len_is_applied_after_closing():
    a, b = _f32(0.9, 0.7)
    row = [0.9, 0.0, 0.7, 0.0, 0.0, 0.0, 0.9, 0.9, 0.9, 0.9, 0.9, 0.0, 0.7]
    both = [(0, 0, 0, 1, a, a, -0.5, 0.5), (0, 2, 2, 1, b, b, 1.5, 2.5), (0, 6, 10, 5, a, a, 5.5, 10.5), (0, 12, 12, 1, b, b, 11.5, 12.5)]
    _same(_records([row], 13, min_len=1), both)
    _same(_records([row], 13, min_len=2), [both[2]])
    _same(_records([row], 13, min_len=5), [both[2]])
    _same(_records([row], 13, min_len=6), [])
    # with max_gap = 1 frames 0..2 are ONE run of 3 frames (2 of them active), and 6..12 one of 7 (6 active)
    closed = [(0, 0, 2, 2, a, _mean(0.9, 0.7), -0.5, 2.5), (0, 6, 12, 6, a, _mean(0.9, 0.9, 0.9, 0.9, 0.9, 0.7), 5.5, 12.5)]
    _same(_records([row], 13, max_gap=1, min_len=1), closed)
    _same(_records([row], 13, max_gap=1, min_len=2), closed)
    _same(_records([row], 13, max_gap=1, min_len=3), closed)
    _same(_records([row], 13, max_gap=1, min_len=5), [closed[1]])
    _same(_records([row], 13, max_gap=1, min_len=8), [])


def test_a_closed_gap_contributes_nothing_to_the_scores():
    a = _f32(0.9)[0]
    clean = _records([[0.9, 0.0, 0.7]], 3, max_gap=1)
    _same(clean, [(0, 0, 2, 2, a, _mean(0.9, 0.7), -0.5, 2.5)])
    _same(_records([[0.9, NAN, 0.7]], 3, max_gap=1), clean)                                   # a NaN inside the gap
    _same(_records([[0.9, -INF, 0.7]], 3, max_gap=1), clean)
    _same(_records([[0.9, 0.5, 0.7]], 3, max_gap=1), clean)


def test_decode_then_rasterise_gives_the_reference_arrays_back():
    """every fixture video, whole and in its training and testing window: decode_reference(the reference's array) -> SegLabel ->
    dense_reference() is the array, 0 differing elements; 761 segments over the 126 arrays, so an empty decode cannot pass"""
    from cfn_hip.detections import decode_reference
    from cfn_hip.seglabels import SegLabel
    recs = sf.records()
    arrays = segments = most = 0
    for i in range(len(recs)):
        for kind in ('full',) + sf.SPLITS:
            want, sl = sf.expected(i, kind), sf.seglabel(i, kind)
            assert want.shape == (157, sl.length)
            if sl.length == 0:
                arrays += 1
                continue
            det = decode_reference(torch.from_numpy(want.copy())[None], torch.tensor([sl.length], dtype=torch.int32),
                                   torch.tensor([sl.fps], dtype=torch.float64), torch.tensor([sl.start], dtype=torch.int32), 0.5)
            n = det.check()
            got = SegLabel(det.seg[:n].numpy(), sl.fps, sl.start, sl.length).dense_reference()
            assert int((got != want).sum()) == 0, (recs[i]['vid'], kind)
            assert int(det.frames[:n, 2].sum()) == int(want.sum())                             # every active frame is in exactly one segment
            arrays, segments = arrays + 1, segments + n
            if n:
                most = max(most, int(np.bincount(det.seg[:n, 0].numpy().astype(np.int64)).max()))
    assert (arrays, segments, most) == (126, 761, 3)


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_collated_batches_round_trip_through_as_seg_labels(name):
    from cfn_hip.detections import Detections, decode_reference
    from cfn_hip.seglabels import SegLabels, collate_seg
    split, idx, labels, masks = sf.batch(name)
    sl = collate_seg([sf.seglabel(i, split) for i in idx])
    valid = torch.from_numpy(masks.sum(1)).to(torch.int32)
    det = decode_reference(torch.from_numpy(labels.copy()), valid, sl.fps, sl.window[:, 0].contiguous(), 0.5)
    assert isinstance(det, Detections) and det.check() > 0 and det.batch == len(idx)
    back = det.as_seg_labels(sl.fps, sl.window, sl.t_max)
    assert isinstance(back, SegLabels) and back.seg is det.seg and back.offsets is det.offsets          # no copy
    lab, mask, got_valid = back.dense_reference()
    assert int((lab.numpy() != labels).sum()) == 0 and int((mask.numpy() != masks).sum()) == 0 and torch.equal(got_valid, valid)


def test_cap_keeps_the_prefix_and_the_true_counts():
    from cfn_hip.detections import decode_reference
    probs = torch.tensor([[[0.9, 0, 0.9, 0, 0.9]], [[0.9, 0.9, 0, 0, 0.9]]])
    valid = torch.tensor([5, 5], dtype=torch.int32)
    full = decode_reference(probs, valid)
    assert full.check() == 5 and full.cap == 5 and full.offsets.tolist() == [0, 3, 5]
    cut = decode_reference(probs, valid, cap=2)
    assert cut.cap == 2 and cut.offsets.tolist() == [0, 3, 5] and cut.total.tolist() == [5] and tuple(cut.seg.shape) == (2, 3)
    assert torch.equal(cut.seg, full.seg[:2]) and torch.equal(cut.frames, full.frames[:2]) and torch.equal(cut.score, full.score[:2])
    with pytest.raises(RuntimeError, match=r'5 segments.*cap = 2'):
        cut.check()
    with pytest.raises(RuntimeError, match='cap = 2'):
        cut.tolist()
    none = decode_reference(torch.zeros(2, 3, 4), torch.tensor([4, 4], dtype=torch.int32))
    assert none.check() == 0 and none.offsets.tolist() == [0, 0, 0] and tuple(none.seg.shape) == (1, 3) and none.tolist() == [[], []]


def test_entry_point_is_declared_exported_and_checks_its_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    assert 'cfn_decode_segments' in protos and 'cfn_decode_segments_workspace_bytes' in protos
    ret, at, dts = protos['cfn_decode_segments']
    assert ret is ctypes.c_int and len(at) == 18 and at[-1] is ctypes.c_void_p and at[-2] is ctypes.c_long
    assert dts[:11] == [torch.float32, torch.int32, torch.float64, torch.int32, torch.float32, torch.float64, torch.int32, torch.float32, torch.int32,
                        torch.int32, None]
    assert at[11:16] == [ctypes.c_int] * 5
    ret, at, _ = protos['cfn_decode_segments_workspace_bytes']
    assert ret is ctypes.c_long and at == [ctypes.c_int] * 3
    raw = ctypes.CDLL(cfn_hip.LIB_PATH)
    assert hasattr(raw, 'cfn_decode_segments') and hasattr(raw, 'cfn_decode_segments_workspace_bytes')
    lib = cfn_hip.load()                                         # the binding: the header's prototypes attached to the exported symbols
    assert list(lib.cfn_decode_segments.argtypes) == protos['cfn_decode_segments'][1] and lib.cfn_decode_segments.restype is ctypes.c_int
    assert lib.cfn_decode_segments_workspace_bytes.restype is ctypes.c_long
    # the rows' bit masks (8 bytes per 64 frames) and B * C + 1 counts
    assert cfn_hip.query('cfn_decode_segments_workspace_bytes', 2, 157, 640) == 2 * 157 * 10 * 8 + (2 * 157 + 1) * 4
    assert cfn_hip.query('cfn_decode_segments_workspace_bytes', 1, 1, 65) == 2 * 8 + 2 * 4
    for B, C, TL in ((0, 157, 8), (1, 0, 8), (1, 157, 0), (65536, 1, 8), (1, 1 << 19, 8), (1, 157, 65537), (65535, 157, 640)):
        assert cfn_hip.query('cfn_decode_segments_workspace_bytes', B, C, TL) == -1, (B, C, TL)
    none = [None] * 11
    assert lib.cfn_decode_segments(*none, 1, 157, 8, 0, 1, 628, None) == 1 and 'null' in cfn_hip.last_error()
    buf = (ctypes.c_double * 8)()
    p = [ctypes.addressof(buf)] * 11
    for B, C, TL, gap, mlen, cap, word in ((0, 157, 8, 0, 1, 1, 'shape'), (1, 0, 8, 0, 1, 1, 'shape'), (1, 157, 0, 0, 1, 1, 'shape'),
                                           (65536, 1, 8, 0, 1, 1, 'large'), (1, 1 << 19, 8, 0, 1, 1, 'large'), (1, 157, 65537, 0, 1, 1, 'large'),
                                           (65535, 157, 640, 0, 1, 1, 'large'), (1, 157, 8, -1, 1, 1, 'max_gap'), (1, 157, 8, 0, 0, 1, 'min_len'),
                                           (1, 157, 8, 0, 1, 0, 'cap'), (1, 157, 8, 0, 1, 1 << 31, 'cap')):
        assert lib.cfn_decode_segments(*p, B, C, TL, gap, mlen, cap, None) == 1, (B, C, TL, gap, mlen, cap)        # refused before any launch
        assert 'cfn_decode_segments' in cfn_hip.last_error() and word in cfn_hip.last_error(), cfn_hip.last_error()
    src = open(os.path.join(os.path.dirname(cfn_hip.LIB_PATH), '..', 'csrc', 'detections.hip')).read()
    assert 'getenv' not in src and 'atomic' not in src and 'train_fine.py:199-206' in src
    hdr = open(cfn_hip.HEADER).read()
    assert 'train_fine.py:199-206' in hdr


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    _lib()
    from cfn_hip import ops
    from cfn_hip.detections import decode
    ok = dict(probs=torch.zeros(2, 5, 16), valid_t=torch.full((2,), 16, dtype=torch.int32), fps=torch.ones(2, dtype=torch.float64),
              start=torch.zeros(2, dtype=torch.int32), thr=0.5)
    with pytest.raises(RuntimeError, match='probs is on cpu'):           # everything well formed: what is left is the device
        ops.decode_segments(**ok)
    with pytest.raises(RuntimeError, match='no CPU path'):
        decode(ok['probs'], ok['valid_t'])
    bad = [('probs', dict(probs=ok['probs'].double())), ('probs', dict(probs=ok['probs'][0])), ('probs', dict(probs=ok['probs'][:, :, ::2])),
           ('probs', dict(probs=torch.zeros(1, 1, 65537))), ('TL <= 65536', dict(probs=torch.zeros(1, 1, 65537))),
           ('valid_t', dict(valid_t=ok['valid_t'].long())), ('valid_t', dict(valid_t=ok['valid_t'][:1])),
           ('fps', dict(fps=ok['fps'].float())), ('fps', dict(fps=torch.ones(3, dtype=torch.float64))),
           ('start', dict(start=ok['start'].long())), ('start', dict(start=torch.zeros(2, 1, dtype=torch.int32))),
           ('thr', dict(thr=torch.zeros(4))), ('thr', dict(thr=torch.zeros(5, dtype=torch.float64))), ('thr', dict(thr='0.5')),
           ('max_gap', dict(max_gap=-1)), ('min_len', dict(min_len=0)), ('cap', dict(cap=0)), ('cap', dict(cap=1 << 31))]
    for word, change in bad:
        with pytest.raises(RuntimeError, match='decode_segments: .*' + word):
            ops.decode_segments(**dict(ok, **change))
    assert ops.decode_segments_cap(2, 5, 16) == 80 and ops.decode_segments_cap(3, 157, 7) == 3 * 157 * 4
    with pytest.raises(RuntimeError, match='decode_segments'):
        ops.decode_segments_workspace_bytes(1, 1, 65537)
    # not an operator of the native library: the cfn:: namespace stays the 47 of cfn_hip.torchlib's tuples
    from cfn_hip import torchlib as tl
    assert not any('decode_segments' in n for tup in (tl.OPERATORS, tl.INPUT_OPERATORS, tl.AUGMENT_OPERATORS, tl.METRIC_OPERATORS,
                                                      tl.FEATURE_OPERATORS, tl.DECODE_OPERATORS, tl.LABEL_OPERATORS) for n in tup)


def _two_videos():
    from cfn_hip.detections import decode_reference
    probs = torch.zeros(2, 4, 12)
    probs[0, 1, 2:5] = torch.tensor([0.9, 0.6, 0.8])
    probs[0, 3, 0] = 0.7
    probs[1, 0, 9:12] = 0.75
    valid = torch.tensor([12, 11], dtype=torch.int32)
    return probs, valid, decode_reference(probs, valid)


def test_detections_to_check_and_tolist():
    from cfn_hip.detections import Detections
    probs, valid, det = _two_videos()
    assert det.check() == 3 and det.batch == 2 and det.device.type == 'cpu' and type(det.cap) is int and type(det.n_classes) is int
    moved = det.to('cpu')
    assert isinstance(moved, Detections) and (moved.n_classes, moved.cap) == (4, 3) and all(torch.equal(a, b) for a, b in zip(moved[:5], det[:5]))
    with pytest.raises(TypeError):
        det.to(torch.float32)
    with pytest.raises(TypeError):
        det.to(None)
    a, b, c, d = (float(np.float32(v)) for v in (0.9, 0.7, 0.75, 0.6))
    want = [[{'class': 1, 'start': 1.5, 'end': 4.5, 't0': 2, 't1': 4, 'score_max': a, 'score_mean': _mean(0.9, 0.6, 0.8)},
             {'class': 3, 'start': -0.5, 'end': 0.5, 't0': 0, 't1': 0, 'score_max': b, 'score_mean': b}],
            [{'class': 0, 'start': 8.5, 'end': 10.5, 't0': 9, 't1': 10, 'score_max': c, 'score_mean': c}]]
    assert det.tolist() == want
    named = det.tolist(names=['walk', 'sit', 'run', 'eat'])
    assert [r['class'] for v in named for r in v] == ['sit', 'eat', 'walk'] and named[0][0]['t1'] == 4
    json.dumps(named)                                            # plain Python values


def test_writer_writes_one_json_object_per_video(tmp_path):
    from cfn_hip.detections import DetectionWriter, decode_reference, epoch_path, read_detections
    from cfn_hip.seglabels import SegLabel, collate_seg
    probs, valid, det = _two_videos()
    w = DetectionWriter(str(tmp_path / 'out' / 'det.jsonl'), 0.5, 0, 1)
    got = w.add(probs, valid, None, ['v0', 'v1'], decoder=decode_reference)                  # dense labels: frame units
    assert all(torch.equal(a, b) for a, b in zip(got[:5], det[:5]))
    sl = collate_seg([SegLabel([[1, 0.0, 1.0]], 24.0, 48, 12, n_classes=4), SegLabel([], 29.97, 7, 11, n_classes=4)])
    w.add(probs, valid, sl, ['v2', 'v3'], decoder=decode_reference)                          # a SegLabels batch: its fps and window, seconds
    with pytest.raises(ValueError, match='names'):
        w.add(probs, valid, None, ['only one'], decoder=decode_reference)
    assert w.flush() == 4
    rows = read_detections(w.path)
    assert [r['video'] for r in rows] == ['v0', 'v1', 'v2', 'v3'] and [r['unit'] for r in rows] == ['frame', 'frame', 's', 's']
    assert all(set(r) == {'video', 'unit', 'segments'} for r in rows)
    assert rows[0]['segments'] == det.tolist()[0] and rows[1]['segments'] == det.tolist()[1]
    secs = decode_reference(probs, valid, sl.fps, sl.window[:, 0].contiguous()).tolist()
    assert rows[2]['segments'] == secs[0] and rows[3]['segments'] == secs[1]
    assert rows[2]['segments'][0]['start'] == (48 + 2 - 0.5) / 24.0 and rows[3]['segments'][0]['end'] == (7 + 10 + 0.5) / 29.97
    assert rows[2]['segments'][0]['t0'] == 2                     # frames stay window relative
    assert w.take() == [] and w.flush(str(tmp_path / 'empty.jsonl')) == 0 and read_detections(str(tmp_path / 'empty.jsonl')) == []
    # gap closing and min_len reach the decode; rows handed in (the ranks' gathered lists) go to the path given
    w2 = DetectionWriter(str(tmp_path / 'det2.jsonl'), thr=0.65, max_gap=1, min_len=3)
    w2.add(probs, valid, None, ['v0', 'v1'], decoder=decode_reference)
    mine = w2.take()
    assert [(s['t0'], s['t1']) for s in mine[0]['segments']] == [(2, 4)] and mine[0]['segments'][0]['score_mean'] == _mean(0.9, 0.8)
    assert mine[1]['segments'] == []                             # frames 9, 10 of video 1: two frames, shorter than min_len
    path = epoch_path(w2.path, 4)
    assert os.path.basename(path) == 'det2.ep004.jsonl'
    assert w2.flush(path, mine + mine) == 4 and len(read_detections(path)) == 4 and not os.path.exists(w2.path)
    # a small budget reads the kept batches back early; the file is the same
    w3 = DetectionWriter(str(tmp_path / 'det3.jsonl'), 0.5, 0, 1, max_pending_bytes=1)
    w3.add(probs, valid, None, ['v0', 'v1'], decoder=decode_reference)
    assert w3._pending == [] and w3.flush() == 2 and read_detections(w3.path) == rows[:2]


def test_scripts_take_a_writer_and_default_to_none():
    import train_coarse_fineFEAT as tc
    import train_fine
    import train_joint
    for mod in (train_fine, tc):
        p = inspect.signature(mod.run).parameters
        assert 'detections' in p and p['detections'].default is None, mod.__name__
    assert 'detections' not in inspect.signature(train_joint.run).parameters            # no validation phase there
    parser = argparse.ArgumentParser()
    train_fine.add_detect_args(parser)
    off = parser.parse_args([])
    assert off.detect is None and train_fine.detect_argv(off) == [] and train_fine.detect_writer(off) is None
    on = parser.parse_args(['--detect', 'out/det.jsonl', '--detect-thr', '0.3', '--detect-gap', '2', '--detect-min-len', '4'])
    again = parser.parse_args(train_fine.detect_argv(on))                                 # what a spawned worker parses
    assert vars(again) == vars(on)
    w = train_fine.detect_writer(again)
    assert (w.path, w.thr, w.max_gap, w.min_len) == ('out/det.jsonl', 0.3, 2, 4)
    for mod in (train_fine, tc):
        src = inspect.getsource(mod)
        assert 'add_detect_args(parser)' in src and 'detect_argv(args)' in src and 'detections=detect_writer(args)' in src, mod.__name__
