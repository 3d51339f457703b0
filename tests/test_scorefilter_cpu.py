"""Temporal score filter without a GPU (cfn_hip/scorefilter.py): filter_reference against a naive per-frame spelling of rules F1-F6 and against
cases worked out by hand, the premise that makes bit-equality a demanding check, the weight tables, the ScoreFilter type, the command-line
option and its refusals, the entry point's argument checks, and that filter=None / radius 0 leave the decode exactly as it was."""
import argparse
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import scorefilter_fixture as fx
import seg_fixture as sf

NAN, INF = float('nan'), float('inf')


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _ref(rows, valid, flt):
    """rows: one video's (C, TL) nested lists -> filter_reference's (C, TL) float32 array"""
    from cfn_hip.scorefilter import filter_reference
    p = torch.tensor([rows], dtype=torch.float32)
    return filter_reference(p, torch.tensor([valid], dtype=torch.int32), flt)[0].numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).tolist()


@pytest.mark.parametrize('kind', ['random', 'quantised', 'wide'])
@pytest.mark.parametrize('method', ['box', 'gaussian', 'median'])
def test_reference_equals_the_naive_per_frame_spelling(kind, method):
    """every rule once more, frame by frame in Python: per-class radii with 0 and 32 among them, valid_t below 0, 0, inside, TL and above"""
    from cfn_hip.scorefilter import ScoreFilter, filter_reference
    B, C, TL = 5, 5, 41
    p = fx.scores(kind, B, C, TL).copy()
    p[2, 1, 7], p[2, 3, 0], p[4, 4, 40], p[4, 2, 20] = NAN, INF, -INF, NAN
    valid = np.array([-1, 0, 17, TL, TL + 5], np.int32)
    flt = ScoreFilter(method, [0, 1, 3, 32, 7], [0.5, 1.0, 2.0, 11.0, 2.5] if method == 'gaussian' else None)
    radius, weights, code = flt.arrays(C)
    got = filter_reference(torch.from_numpy(p), torch.from_numpy(valid), flt).numpy()
    fx.same_bits(got, fx.naive(p, valid, radius, weights, code))
    fx.same_bits(got[:2], p[:2])                                                      # valid_t <= 0: a copy
    fx.same_bits(got[:, 0], p[:, 0])                                                  # radius 0: a copy
    fx.same_bits(got[2, :, 17:], p[2, :, 17:])                                        # behind valid_t: a copy
    assert (got != p)[2:, 1:].sum() > 0


def test_box_and_gaussian_by_hand():
    from cfn_hip.scorefilter import ScoreFilter
    got = _ref([[1, 2, 4]], 3, ScoreFilter('box', 1))
    assert _bits(got[0]) == _bits([np.float32(1.5), np.float32(np.float64(7.0) / np.float64(3.0)), np.float32(3.0)])      # truncated, not padded
    got = _ref([[1, 2, 4, 100]], 3, ScoreFilter('box', 1))                             # frame 3 is behind valid_t: never read, copied
    assert _bits(got[0]) == _bits([1.5, np.float32(7.0 / 3.0), 3.0, 100.0])
    w = np.exp(-1.0 / (2.0 * 0.75 * 0.75))
    got = _ref([[1, 2, 4]], 3, ScoreFilter('gaussian', 1, 0.75))
    want = [np.float32((1.0 + w * 2.0) / (1.0 + w)), np.float32(((w * 1.0 + 2.0) + w * 4.0) / ((w + 1.0) + w)), np.float32((w * 2.0 + 4.0) / (w + 1.0))]
    assert _bits(got[0]) == _bits(want)


def test_median_even_count_at_an_edge_and_zero_ties():
    from cfn_hip.scorefilter import ScoreFilter
    got = _ref([[3, 1, 2]], 3, ScoreFilter('median', 1))
    assert got[0].tolist() == [2.0, 2.0, 1.5]                                          # two frames at each edge: the mean of both
    got = _ref([[3, 1, 2, 9]], 2, ScoreFilter('median', 1))
    assert got[0].tolist() == [2.0, 2.0, 2.0, 9.0]                                     # the window ends at valid_t - 1
    # +0 and -0 compare equal: the earlier frame ranks first, so the middle of three is the LATER zero
    assert _bits(_ref([[0.0, -0.0, 1.0]], 3, ScoreFilter('median', 1))[0][1:2]) == _bits([-0.0])
    assert _bits(_ref([[-0.0, 0.0, 1.0]], 3, ScoreFilter('median', 1))[0][1:2]) == _bits([0.0])
    assert _bits(_ref([[-1.0, 0.0, -0.0]], 3, ScoreFilter('median', 1))[0][1:2]) == _bits([0.0])      # ranks: -1, then +0 (earlier), then -0


@pytest.mark.parametrize('method', ['box', 'median'])
def test_non_finite_windows_give_the_canonical_nan(method):
    from cfn_hip.scorefilter import ScoreFilter
    payload = np.array([0xffc12345], np.uint32).view(np.float32)[0]                    # a negative NaN with a payload
    rows = [[0.5, 0.25, payload, 0.5, 0.5, 0.75, INF, 0.5, 0.25, 0.5], [0.5, 0.25, payload, 0.5, 0.5, 0.75, -INF, 0.5, 0.25, 0.5]]
    got = _ref(rows, 9, ScoreFilter(method, [1, 0]))
    b = _bits(got[0])
    assert b[1:4] == [fx.QNAN] * 3 and b[5:8] == [fx.QNAN] * 3                         # every window that reaches the NaN or the infinity
    assert np.isfinite(got[0][[0, 4, 8]]).all() and got[0][9] == 0.5
    assert _bits(got[1]) == _bits(rows[1])                                             # radius 0: the input bits, payload and all


def test_valid_t_and_radius_are_clamped():
    from cfn_hip.scorefilter import ScoreFilter, filter_reference
    p = torch.from_numpy(fx.scores('random', 3, 2, 9).copy())
    flt = ScoreFilter('box', 2)
    got = filter_reference(p, torch.tensor([0, 9, 14], dtype=torch.int32), flt)
    fx.same_bits(got[0], p[0])
    fx.same_bits(filter_reference(p[1:2], torch.tensor([14], dtype=torch.int32), flt), got[1:2])          # valid_t above TL is TL
    fx.same_bits(filter_reference(p, torch.tensor([-3, -3, -3], dtype=torch.int32), flt), p)
    # a radius beyond R = weights.shape[1] - 1 is R; a negative one is 0
    raw = (np.array([40, -2], np.int32), np.ones((2, 3)), 0)
    want = filter_reference(p, torch.tensor([9, 9, 9], dtype=torch.int32), ScoreFilter('box', [2, 0]))
    fx.same_bits(filter_reference(p, torch.tensor([9, 9, 9], dtype=torch.int32), raw), want)
    raw = (torch.tensor([40, -2], dtype=torch.int32), torch.ones(2, 3, dtype=torch.float64), 1)
    want = filter_reference(p, torch.tensor([9, 9, 9], dtype=torch.int32), ScoreFilter('median', [2, 0]))
    fx.same_bits(filter_reference(p, torch.tensor([9, 9, 9], dtype=torch.int32), raw), want)


def test_fixture_premise_the_order_of_the_sum_shows_in_the_bits():
    """bit-equality has teeth: on the wide-range fixture the same windows summed from their last frame to their first round differently in a
    nonzero number of outputs, so a kernel that sums in another order cannot pass (the box filter: its products are exact, so the fixture's
    planted pairs cancel exactly and the small terms around them survive in one order only)"""
    from cfn_hip.scorefilter import ScoreFilter, filter_reference
    p = fx.scores('wide', 2, 3, 96)
    assert float(np.abs(p).max()) <= 1.0 and 0 < float(np.abs(p)[p != 0].min()) < 2.0 ** -126 and float(np.abs(p).max()) > 2.0 ** -4
    valid = np.array([96, 60], np.int32)
    flt = ScoreFilter('box', [8, 32, 3])
    radius, weights, code = flt.arrays(3)
    ref = filter_reference(torch.from_numpy(p.copy()), torch.from_numpy(valid), flt).numpy()
    fx.same_bits(ref, fx.naive(p, valid, radius, weights, code))
    other = fx.naive(p, valid, radius, weights, code, descending=True)
    changed = int((ref.view(np.uint32) != other.view(np.uint32)).sum())
    assert changed > 0
    assert float(np.abs(other.astype(np.float64) - ref).max()) < 1e-13                 # (the other order is the same filter up to fp64 rounding)


def test_filter_weights_properties():
    from cfn_hip.scorefilter import filter_weights
    w = filter_weights('box', [0, 3, 32])
    assert w.dtype == np.float64 and w.shape == (3, 33) and (w == 1.0).all()
    assert filter_weights('median', 4).shape == (1, 5)
    g = filter_weights('gaussian', [2, 32, 5], [0.5, 11.0, 1.0 / 64.0])
    assert g.dtype == np.float64 and g.shape == (3, 33) and g.flags['C_CONTIGUOUS']
    assert (g[:, 0] == 1.0).all() and (g >= 0).all() and (g <= 1.0).all() and (np.diff(g, axis=1) <= 0).all()
    assert g[1, 1] == np.exp(-1.0 / (2.0 * 11.0 * 11.0)) and g[0, 2] == np.exp(-4.0 / (2.0 * 0.5 * 0.5)) and g[2, 1] == 0.0      # (underflow is a weight of 0)
    assert np.array_equal(filter_weights('gaussian', [4, 4], 2.0)[0], filter_weights('gaussian', 4, [2.0])[0])
    for bad in (('box', [33]), ('box', [-1]), ('mean', [1]), ('box', [1], 1.0), ('gaussian', [1]), ('gaussian', [1], 0.0), ('gaussian', [1], NAN),
                ('gaussian', [1, 2], [1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            filter_weights(*bad)


def test_score_filter_type():
    from cfn_hip.scorefilter import ScoreFilter, parse_spec
    f = ScoreFilter('gaussian', sigma=2.5)
    assert f.radius == (8,) and f.code == 0 and f.spec == 'gaussian:2.5:8' and parse_spec(f.spec) == f                 # ceil(3 sigma)
    assert ScoreFilter('gaussian', sigma=100.0).radius == (32,)                                                      # capped
    assert ScoreFilter('gaussian', sigma=[0.5, 4.0]).radius == (2, 12)
    assert ScoreFilter('median', 3).code == 1 and ScoreFilter('box', 3) == ScoreFilter('box', 3) != ScoreFilter('median', 3)
    radius, weights, code = ScoreFilter('box', [0, 5, 2]).arrays(3)
    assert radius.dtype == np.int32 and radius.tolist() == [0, 5, 2] and weights.shape == (3, 6) and code == 0
    radius, weights, _ = ScoreFilter('gaussian', 2, 1.0).arrays(4)
    assert radius.tolist() == [2] * 4 and weights.shape == (4, 3) and (weights == weights[0]).all()
    f = ScoreFilter('box', 2)
    r1, w1, c1 = f.tensors(7, 'cpu')
    assert r1.dtype == torch.int32 and tuple(r1.shape) == (7,) and w1.dtype == torch.float64 and tuple(w1.shape) == (7, 3) and c1 == 0
    assert f.tensors(7, 'cpu')[0] is r1 and f.tensors(8, 'cpu')[0] is not r1                                          # built once per class count
    for bad in (('box', 33), ('box', -1), ('box', 1.5), ('box', True), ('box', None), ('box', 2, 1.0), ('median', [1, 40]), ('gaussian', 2),
                ('gaussian', 2, 0.0), ('gaussian', 2, NAN), ('gaussian', 2, INF), ('gaussian', [1, 2], [1.0, 2.0, 3.0]), ('mean', 2), ('box', [])):
        with pytest.raises(ValueError):
            ScoreFilter(*bad)
    with pytest.raises(ValueError, match='3 radii for 5 classes'):
        ScoreFilter('box', [1, 2, 3]).arrays(5)
    with pytest.raises(ValueError, match='command-line'):
        ScoreFilter('box', [1, 2, 3]).spec


def test_apply_and_the_operator_have_no_cpu_path():
    _lib()
    from cfn_hip import ops
    from cfn_hip.scorefilter import ScoreFilter, apply
    p, v = torch.rand(2, 3, 8), torch.tensor([8, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU path'):
        apply(p, v, ScoreFilter('box', 1))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.score_filter(p, v, torch.ones(3, dtype=torch.int32), torch.ones(3, 2, dtype=torch.float64), 0)
    with pytest.raises(TypeError):
        apply(p, v, 'box:1')


def test_entry_point_is_declared_exported_and_checks_its_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    assert 'cfn_score_filter' in protos and 'cfn_score_filter_tile' in protos
    ret, at, dts = protos['cfn_score_filter']
    assert ret is ctypes.c_int and len(at) == 11 and at[-1] is ctypes.c_void_p
    assert dts[:5] == [torch.float32, torch.int32, torch.int32, torch.float64, torch.float32]
    lib = cfn_hip.load()
    from cfn_hip import ops
    assert lib.cfn_score_filter_tile() == ops.SCORE_FILTER_TILE
    # refused before any launch (the pointers are never dereferenced on the host): 1 and a reason
    a, b, c, d, e = (ctypes.c_void_p(4096 * k) for k in range(1, 6))
    for args, word in (((None, b, c, d, e, 1, 1, 8, 1, 0), 'null'), ((a, b, c, d, None, 1, 1, 8, 1, 0), 'null'), ((a, b, c, d, e, 0, 1, 8, 1, 0), 'B and C'),
                       ((a, b, c, d, e, 1, 65536, 8, 1, 0), 'B and C'), ((a, b, c, d, e, 1, 1, 0, 1, 0), 'TL'), ((a, b, c, d, e, 1, 1, 65537, 1, 0), 'TL'),
                       ((a, b, c, d, e, 1, 1, 8, 33, 0), 'R in'), ((a, b, c, d, e, 1, 1, 8, -1, 0), 'R in'), ((a, b, c, d, e, 1, 1, 8, 1, 2), 'method'),
                       ((a, b, c, d, a, 1, 1, 8, 1, 0), 'must not be probs')):
        assert lib.cfn_score_filter(*args, None) == 1 and word in cfn_hip.last_error(), (args[5:], cfn_hip.last_error())
    # it is not one of the registered torch operators, and the kernel source reads no environment variable
    src = open(os.path.join(os.path.dirname(os.path.dirname(cfn_hip.LIB_PATH)), 'csrc', 'scorefilter.hip')).read()
    assert 'getenv' not in src and 'atomic' not in src.split('#include')[1]


def _parser():
    import train_fine
    p = argparse.ArgumentParser()
    train_fine.add_detect_args(p)
    train_fine.seg_ap_arguments(p)
    p.add_argument('--device-ap', action='store_true')
    return p


def test_command_line_option_round_trip_and_refusals():
    import train_coarse_fineFEAT as tc
    import train_fine
    from cfn_hip.scorefilter import ScoreFilter, parse_spec
    assert parse_spec('box:3') == ScoreFilter('box', 3) and parse_spec('median:0') == ScoreFilter('median', 0)
    assert parse_spec('gaussian:1.5') == ScoreFilter('gaussian', 5, 1.5) and parse_spec('gaussian:1.5:9') == ScoreFilter('gaussian', 9, 1.5)
    for bad in ('box', 'box:', 'box:33', 'box:-1', 'box:1.5', 'box:1:2', 'median:x', 'gaussian', 'gaussian:0', 'gaussian:nan', 'gaussian:1:40',
                'gaussian:1:2:3', 'mean:3', ''):
        with pytest.raises(ValueError, match='box:R'):
            parse_spec(bad)
    p = _parser()
    assert p.parse_args([]).detect_smooth is None and train_fine.detect_smooth(p.parse_args([])) is None
    for mod in (train_fine, tc):
        assert mod.add_detect_args is train_fine.add_detect_args and mod.detect_argv is train_fine.detect_argv
    a = p.parse_args(['--detect', 'out/det.jsonl', '--detect-smooth', 'gaussian:1.5:6', '--detect-gap', '2'])
    argv = train_fine.detect_argv(a)
    assert argv[argv.index('--detect-smooth') + 1] == 'gaussian:1.5:6'
    again = p.parse_args(argv)
    assert again.detect_smooth == a.detect_smooth and train_fine.detect_argv(again) == argv
    assert '--detect-smooth' not in train_fine.detect_argv(p.parse_args(['--detect', 'x.jsonl']))
    w = train_fine.detect_writer(a)
    assert w.filter == ScoreFilter('gaussian', 6, 1.5) and w.max_gap == 2
    assert train_fine.detect_writer(p.parse_args(['--detect', 'x.jsonl'])).filter is None
    w = train_fine.detect_writer(p.parse_args(['--detect', 'x.jsonl', '--detect-levels', '0.7,0.4', '--detect-smooth', 'median:2']))
    assert w.filter == ScoreFilter('median', 2) and w.n_levels == 2
    with pytest.raises(ValueError, match='box:R'):
        train_fine.detect_writer(p.parse_args(['--detect', 'x.jsonl', '--detect-smooth', 'box:99']))
    both = p.parse_args(['--detect', 'x.jsonl', '--seg-ap', '--device-ap', '--detect-calibrate', 'f1', '--detect-smooth', 'box:2'])
    for make in (train_fine.detect_smooth, train_fine.detect_writer, train_fine.seg_ap_from_args):
        with pytest.raises(ValueError, match='RAW frame scores'):
            make(both)
    assert 'filter=smooth' in inspect.getsource(train_fine.seg_ap_from_args)
    assert 'filter=' in inspect.getsource(train_fine.segment_ap_add)


def test_writer_and_meter_take_a_filter():
    from cfn_hip.detections import DetectionWriter, decode, decode_levels, decode_levels_reference, decode_reference, propose
    from cfn_hip.scorefilter import ScoreFilter
    from cfn_hip.segap import SegmentAPMeter
    for fn in (decode, decode_reference, decode_levels, decode_levels_reference, propose, DetectionWriter.__init__, SegmentAPMeter.__init__):
        assert inspect.signature(fn).parameters['filter'].default is None, fn
    with pytest.raises(TypeError, match='ScoreFilter'):
        DetectionWriter('x', filter='box:2')
    with pytest.raises(TypeError, match='ScoreFilter'):
        SegmentAPMeter('cuda', 5, filter='box:2')
    # the writer hands its filter to the decoder it is given: the numpy references here
    probs = torch.tensor([[[0.9, 0.1, 0.9, 0.9, 0.1, 0.1, 0.9]]])
    valid = torch.tensor([7], dtype=torch.int32)
    flt = ScoreFilter('median', 1)
    raw = DetectionWriter('x').add(probs, valid, None, ['v'], decoder=decode_reference)
    smooth = DetectionWriter('x', filter=flt).add(probs, valid, None, ['v'], decoder=decode_reference)
    assert raw.frames[:3, :2].tolist() == [[0, 0], [2, 3], [6, 6]]
    assert smooth.frames[:1].tolist() == [[1, 3, 3]] and smooth.check() == 1                    # 0.5 0.9 0.9 0.9 0.1 0.1 0.5: one run, not three
    assert smooth.score[0].tolist() == [np.float32(0.9), np.float32(0.9)]                      # the score columns come from the filtered tensor
    lev = DetectionWriter('x', levels=(0.8, 0.3), nms=1.0, filter=flt).add(probs, valid, None, ['v'], decoder=decode_reference)
    want = propose(probs, valid, levels=(0.8, 0.3), nms_thr=1.0, reference=True, filter=flt)
    assert lev.check() == want.check() == 3 and torch.equal(lev.frames, want.frames) and torch.equal(lev.score, want.score)
    cand, level = decode_levels_reference(probs, valid, levels=(0.8, 0.3), filter=flt)
    assert cand.frames[:3, :2].tolist() == [[1, 3], [0, 3], [6, 6]] and level[:3].tolist() == [0, 1, 1]


def test_no_filter_and_radius_zero_leave_the_decode_as_it_was():
    """the 126 label arrays of tests/golden/seg_labels.npz: decode_reference with filter=None and with a radius-0 filter of either method gives
    the rows of the call without the argument, bit for bit"""
    from cfn_hip.detections import decode_reference
    from cfn_hip.scorefilter import ScoreFilter
    recs = sf.records()
    arrays = segments = 0
    for i in range(len(recs)):
        for k, kind in enumerate(('full',) + sf.SPLITS):
            want, sl = sf.expected(i, kind), sf.seglabel(i, kind)
            arrays += 1
            if sl.length == 0:
                continue
            args = (torch.from_numpy(want.copy())[None], torch.tensor([sl.length], dtype=torch.int32), torch.tensor([sl.fps], dtype=torch.float64),
                    torch.tensor([sl.start], dtype=torch.int32), 0.5)
            base = decode_reference(*args)
            for flt in (None, ScoreFilter(('box', 'median', 'box')[k], 0)):
                got = decode_reference(*args, filter=flt)
                assert all(torch.equal(g.view(torch.uint8), b.view(torch.uint8)) for g, b in zip(got[:5], base[:5])) and got.cap == base.cap
            segments += base.check()
    assert (arrays, segments) == (126, 761)
