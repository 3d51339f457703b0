"""Segment labels, host side (cfn_hip/seglabels.py, collate.py): the definition against the reference's own arrays
(tests/golden/seg_labels.npz, made by make_golden_seg.py from charades_fine.make_dataset / Charades.__getitem__ / mt_collate_fn), the window
constructors, every collate builder with SegLabel label members, collate_seg's refusals, the namedtuple through pinning and staging, and the
C ABI / operator registration of cfn_seg_labels.  No GPU."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import seg_fixture as sf

KEYS = ('layer1', 'layer2', 'layer3', 'layer4', 'conv5')
CH = (8, 16, 8, 24, 8)


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def test_dense_reference_equals_the_reference_arrays():
    """every fixture video, whole and in its training and testing window: 0 differing elements"""
    recs = sf.records()
    assert len(recs) >= 40 and sum(r['crafted'] for r in recs) >= 16
    for i in range(len(recs)):
        for kind in ('full',) + sf.SPLITS:
            got, want = sf.seglabel(i, kind).dense_reference(), sf.expected(i, kind)
            assert got.shape == want.shape and got.dtype == np.float32, (i, kind, got.shape, want.shape)
            assert int((got != want).sum()) == 0, (recs[i]['vid'], kind)
    # the boundary case the fixture is built around: 10.0 s at 240 frames, [2.0, 5.0] -- frame 48 is ON the bound (0), frame 49 inside
    i = [r['vid'] for r in recs].index('CRAFT_INT00')
    full = sf.seglabel(i, 'full').dense_reference()
    assert full[3, 48] == 0 and full[3, 49] == 1 and full[3, 119] == 1 and full[3, 120] == 0


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_collated_batches_equal_mt_collate_fn(name):
    from cfn_hip.seglabels import SegLabels, collate_seg
    split, idx, labels, masks = sf.batch(name)
    sl = collate_seg([sf.seglabel(i, split) for i in idx])
    assert isinstance(sl, SegLabels) and sl.n_classes == 157 and sl.t_max == labels.shape[2] and sl.batch == len(idx)
    assert sl.seg.dtype == torch.float64 and sl.offsets.dtype == torch.int32 and sl.fps.dtype == torch.float64 and sl.window.dtype == torch.int32
    got_l, got_m, got_v = sl.dense_reference()
    assert got_l.dtype == torch.float32 and got_m.dtype == torch.float32 and got_v.dtype == torch.int32
    assert int((got_l.numpy() != labels).sum()) == 0 and int((got_m.numpy() != masks).sum()) == 0
    assert got_v.tolist() == [int(m.sum()) for m in masks]


def test_window_constructors_reproduce_the_fixture_windows():
    recs = sf.records()
    cut = 0
    for i, r in enumerate(recs):
        tr, te = sf.seglabel(i, 'training'), sf.seglabel(i, 'testing')
        assert tr.start == r['start_f'] - 1 and tr.length == sf.expected(i, 'training').shape[1]
        assert te.start == 0 and te.length == sf.expected(i, 'testing').shape[1] == (r['num_frames'] // r['gamma_tau']) * r['gamma_tau']
        assert tr.fps == te.fps == r['num_frames'] / r['duration']
        cut += tr.length < min(r['frames'], r['num_frames'])
    assert cut >= 1                                         # a window that the end of the video cuts short
    a = pickle.loads(pickle.dumps(sf.seglabel(1, 'training')))
    assert np.array_equal(a.actions, sf.seglabel(1, 'training').actions) and (a.fps, a.start, a.length, a.n_classes) == (
        recs[1]['num_frames'] / recs[1]['duration'], recs[1]['start_f'] - 1, 640, 157)
    assert len(pickle.dumps(a)) < 2048


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _builders(tmp_path):
    """{builder name: (clip members of 2 samples, coarse?, packed?)}"""
    from cfn_hip import featpack
    r = np.random.RandomState(0)
    f32 = [r.randn(1, 3, t, 4, 4).astype(np.float32) for t in (5, 3)]
    u8 = [r.randint(0, 256, (1, t, 4, 4, 3)).astype(np.uint8) for t in (5, 3)]
    raw, jpeg = jc.raw_samples(jc.MIXED, jc.MIXED_BOX), jc.jpeg_samples(jc.MIXED, jc.MIXED_BOX)
    feats = [{k: np.abs(r.randn(c, t, 7, 7)).astype(np.float32) for k, c in zip(KEYS, CH)} for t in (6, 9)]
    records = []
    for i, f in enumerate(feats):
        payload, frames, channels = featpack.pack_reference({k: torch.from_numpy(v) for k, v in f.items()}, 'fp16')
        records.append(featpack.open_record(featpack.write_record(featpack.record_path(str(tmp_path), 'v%d' % i), payload, 'fp16', frames, channels)))
    clips = {'': f32, '_u8': u8, '_raw_u8': raw, '_jpeg': jpeg}
    out = {}
    for sfx, c in clips.items():
        out['fine_collate' + sfx] = (c, None)
        out['coarse_collate' + sfx] = (c, feats)
        out['coarse_collate_packed' + sfx] = (c, records)
    return out


def test_every_collate_builder_takes_segment_labels(tmp_path):
    """SegLabel label members -> SegLabels + None, the other members identical to the dense call; dense members -> today's batches"""
    import collate
    from cfn_hip.seglabels import SegLabels
    segs = [sf.seglabel(4, 'training'), sf.seglabel(0, 'training')]
    dense = [s.dense_reference() for s in segs]
    tl = max(d.shape[1] for d in dense)
    want_l, want_m = torch.zeros(2, 157, tl), torch.zeros(2, tl)
    for b, d in enumerate(dense):
        want_l[b, :, :d.shape[1]] = torch.from_numpy(d)
        want_m[b, :d.shape[1]] = 1.0
    builders = _builders(tmp_path)
    assert len(builders) == 12 and all(hasattr(collate, n) for n in builders)
    assert not [n for n in dir(collate) if 'collate' in n and 'seg' in n and n != 'collate_seg']          # no second family of builders
    for name, (clips, feats) in builders.items():
        fn = getattr(collate, name)

        def samples(labels):
            if feats is None:
                return [(c, lb, 'vid%d' % i) for i, (c, lb) in enumerate(zip(clips, labels))]
            return [(c, lb, f, np.array([i, 2, 3, 1], dtype=np.int64), 'vid%d' % i, 30.0 + i) for i, (c, lb, f) in enumerate(zip(clips, labels, feats))]
        db, sb = fn(samples(dense)), fn(samples(segs))
        assert len(db) == len(sb) == (4 if feats is None else 8), name
        assert torch.equal(db[1], want_l) and torch.equal(db[2], want_m) and db[1].dtype == db[2].dtype == torch.float32, name
        assert isinstance(sb[1], SegLabels) and sb[2] is None, name
        assert _same(db[0], sb[0]) and _same(list(db[3:]), list(sb[3:])), name
        got = sb[1].dense_reference()
        assert torch.equal(got[0], want_l) and torch.equal(got[1], want_m), name
        with pytest.raises(ValueError, match='SegLabel'):            # one kind of label per batch
            fn(samples([segs[0], dense[1]]))


def test_collate_seg_refuses_malformed_samples():
    from cfn_hip.seglabels import SegLabel, collate_seg
    ok = SegLabel([[3, 1.0, 2.0]], 24.0, 0, 100)
    assert collate_seg([ok]).t_max == 100
    with pytest.raises(ValueError, match='class count'):
        collate_seg([ok, SegLabel([[3, 1.0, 2.0]], 24.0, 0, 100, n_classes=10)])
    for bad in ([[157, 1.0, 2.0]], [[-1, 1.0, 2.0]], [[2.5, 1.0, 2.0]], [[float('nan'), 1.0, 2.0]]):
        with pytest.raises(ValueError, match='classes'):
            collate_seg([ok, SegLabel(bad, 24.0, 0, 100)])
    with pytest.raises(ValueError, match='classes'):
        collate_seg([SegLabel([[33, 1.0, 2.0]], 24.0, 0, 100, n_classes=33)])
    with pytest.raises(ValueError, match='start'):
        collate_seg([ok, SegLabel([], 24.0, -1, 100)])
    for fps in (0.0, -24.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='fps'):
            collate_seg([ok, SegLabel([], fps, 0, 100)])
    with pytest.raises(ValueError):
        collate_seg([])
    with pytest.raises(ValueError):
        collate_seg([ok, np.zeros((157, 5), np.float32)])
    with pytest.raises(ValueError):
        SegLabel([[1, 2.0]], 24.0, 0, 10)
    # a sample without a frame is fine beside one that has some; a batch without any segment keeps one row that no offset range covers
    sl = collate_seg([SegLabel([], 24.0, 5, 0), SegLabel([], 30.0, 0, 7)])
    assert sl.t_max == 7 and tuple(sl.seg.shape) == (1, 3) and sl.offsets.tolist() == [0, 0, 0] and sl.window.tolist() == [[5, 0], [0, 7]]
    lab, mask, valid = sl.dense_reference()
    assert float(lab.sum()) == 0 and mask.sum(1).tolist() == [0.0, 7.0] and valid.tolist() == [0, 7]


def test_seglabels_is_rebuilt_by_pinning_and_staging(monkeypatch):
    """DataLoader pinning and HostStager rebuild the namedtuple around the moved tensors; the host ints stay host ints"""
    from torch.utils.data._utils import pin_memory as pm
    from cfn_hip import staging
    from cfn_hip.seglabels import SegLabel, SegLabels, collate_seg
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, *a, **k: self.clone())      # (no device here: what pinning does to the structure)
    for sl in (collate_seg([sf.seglabel(i, 'training') for i in (1, 0)]), collate_seg([SegLabel([], 24.0, 0, 9)])):
        batch = [torch.zeros(2, 3), sl, None, ['a', 'b']]
        for moved in (pm.pin_memory(batch), staging._map_tensors(batch, lambda t: t.clone())):
            m = moved[1]
            assert isinstance(m, SegLabels) and moved[2] is None and moved[3] == ['a', 'b']
            assert type(m.n_classes) is int and type(m.t_max) is int and (m.n_classes, m.t_max) == (sl.n_classes, sl.t_max)
            for a, b in zip(m[:4], sl[:4]):
                assert a is not b and a.dtype == b.dtype and torch.equal(a, b)
        plan, total = staging.HostStager._plan(batch)
        assert len(plan) == 5 and total < 4096                   # all four tensors travel (none is empty), a few hundred bytes
    with pytest.raises(TypeError):
        sl.to(torch.float32)
    with pytest.raises(TypeError):
        sl.to(None)
    with pytest.raises(TypeError):
        sl.cuda(torch.float32)
    same = sl.to('cpu')
    assert isinstance(same, SegLabels) and same.t_max == sl.t_max and same.device.type == 'cpu'


def test_entry_point_is_declared_exported_and_checks_its_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    assert 'cfn_seg_labels' in protos
    ret, at, dts = protos['cfn_seg_labels']
    assert ret is ctypes.c_int and len(at) == 12
    assert dts[:7] == [torch.float64, torch.int32, torch.float64, torch.int32, torch.float32, torch.float32, torch.int32]
    lib = cfn_hip.load()
    assert lib.cfn_seg_labels(None, None, None, None, None, None, None, 1, 157, 8, 1, None) == 1 and 'null' in cfn_hip.last_error()
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    for B, C, T, S in ((0, 157, 8, 1), (1, 0, 8, 1), (1, 157, 0, 1), (1, 157, 8, -1), (65536, 157, 8, 1), (1, 1 << 19, 8, 1), (1, 157, 1 << 24, 1)):
        assert lib.cfn_seg_labels(p, p, p, p, p, p, p, B, C, T, S, None) == 1, (B, C, T, S)        # refused before any launch
        assert 'cfn_seg_labels' in cfn_hip.last_error()
    src = open(os.path.join(os.path.dirname(cfn_hip.LIB_PATH), '..', 'csrc', 'seglabels.hip')).read()
    assert 'getenv' not in src and 'charades_fine.py:110-117' in src


def test_ops_and_operator_have_no_cpu_path():
    _lib()
    from cfn_hip import ops, torchlib as tl
    from cfn_hip.seglabels import collate_seg, materialize
    sl = collate_seg([sf.seglabel(0, 'training')])
    with pytest.raises(RuntimeError):
        ops.seg_labels(sl.seg, sl.offsets, sl.fps, sl.window, sl.n_classes, sl.t_max)
    with pytest.raises(RuntimeError):
        sl.dense()
    with pytest.raises(RuntimeError):
        materialize(sl, None, 'cpu')
    a, b = torch.zeros(1, 157, 4), torch.ones(1, 4)
    la, mb = materialize(a, b, 'cpu')                           # dense members pass through
    assert la is a and mb is b
    for bad in (dict(seg=sl.seg.float()), dict(offsets=sl.offsets.long()), dict(fps=sl.fps.float()), dict(window=sl.window[:, :1]), dict(t_max=0),
                dict(n_classes=0), dict(seg=sl.seg[:0])):
        with pytest.raises(RuntimeError, match='seg_labels'):
            ops.seg_labels(*sl._replace(**bad))
    assert tl.LABEL_OPERATORS == ('seg_labels',)
    for tup in (tl.OPERATORS, tl.INPUT_OPERATORS, tl.AUGMENT_OPERATORS, tl.METRIC_OPERATORS, tl.FEATURE_OPERATORS, tl.DECODE_OPERATORS):
        assert not set(tl.LABEL_OPERATORS) & set(tup)
    assert hasattr(torch.ops.cfn, 'seg_labels') and not hasattr(torch.ops.cfn, 'seg_labels_backward')
    m = lambda *s, dt: torch.empty(*s, device='meta', dtype=dt)
    lab, mask, valid = torch.ops.cfn.seg_labels(m(9, 3, dt=torch.float64), m(4, dt=torch.int32), m(3, dt=torch.float64), m(3, 2, dt=torch.int32), 33, 17)
    assert (tuple(lab.shape), lab.dtype, tuple(mask.shape), mask.dtype, tuple(valid.shape), valid.dtype) == (
        (3, 33, 17), torch.float32, (3, 17), torch.float32, (3,), torch.int32)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.seg_labels(sl.seg, sl.offsets, sl.fps, sl.window, 157, sl.t_max)
