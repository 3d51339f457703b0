"""GPU: frame labels rasterised from annotation segments (csrc/seglabels.hip, cfn_hip/seglabels.py).

Every comparison is exact -- 0 differing elements in labels, mask and valid_t: the kernel evaluates the reference's own expression
(fr / fps in fp64, strict inequalities), and correctly rounded fp64 division gives the same double on the device as in Python.  The
expected values are the reference's arrays (tests/golden/seg_labels.npz) and SegLabels.dense_reference(), which test_seglabels_cpu.py
ties to the same arrays.  Outputs are handed over filled with NaN, so an element the kernel does not write shows.

The two training-script tests compare a run fed SegLabel samples with the same run fed the dense labels of the same windows.  The tensors
that reach the loss are bit-equal, so the losses must be; for that to be observable the two runs themselves have to repeat bit for bit,
which is what the library's deterministic mode provides (test_hip_determinism.py), so they run under it."""
import numpy as np
import pytest
import torch

import seg_fixture as sf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]


def _nan_out(sl):
    B, C, T = sl.batch, sl.n_classes, sl.t_max
    return (torch.full((B, C, T), float('nan'), device=DEV), torch.full((B, T), float('nan'), device=DEV),
            torch.full((B,), -12345, dtype=torch.int32, device=DEV))


def _dense_checked(sl):
    """dense() of the host batch `sl` into NaN-filled outputs, compared with dense_reference() on the host: (labels, mask, valid_t) on the CPU"""
    out = _nan_out(sl)
    got = sl.to(DEV).dense(out=out)
    assert all(g is o for g, o in zip(got, out))
    got = [g.cpu() for g in got]
    want = sl.dense_reference()
    for name, g, w in zip(('labels', 'mask', 'valid_t'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = int((g != w).sum()) + int(torch.isnan(g.float()).sum())
        assert bad == 0, '%s: %d elements differ from dense_reference()' % (name, bad)
    return got


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_fixture_batches_equal_mt_collate_fn(name):
    """'a': 5 ragged real videos, C = 157, TLmax = 532 (no multiple of 64); 'b': crafted boundary cases, TLmax = 900; 'c': crafted, odd TLmax"""
    from cfn_hip.seglabels import collate_seg
    split, idx, labels, masks = sf.batch(name)
    lab, mask, valid = _dense_checked(collate_seg([sf.seglabel(i, split) for i in idx]))
    assert int((lab.numpy() != labels).sum()) == 0 and int((mask.numpy() != masks).sum()) == 0
    assert valid.tolist() == [int(m.sum()) for m in masks]


@pytest.mark.parametrize('kind', sf.SPLITS)
def test_every_fixture_video_equals_the_reference(kind):
    """all 42 videos in one batch (the 28-action video, the one without actions, windows past 1000 frames): each sample's rows against the
    array the reference's Dataset returned"""
    from cfn_hip.seglabels import collate_seg
    n = len(sf.records())
    lab, mask, valid = _dense_checked(collate_seg([sf.seglabel(i, kind) for i in range(n)]))
    for i in range(n):
        want = sf.expected(i, kind)
        L = want.shape[1]
        assert int(valid[i]) == L and int((lab[i, :, :L].numpy() != want).sum()) == 0 and float(lab[i, :, L:].abs().sum()) == 0, sf.records()[i]['vid']


def _random_batch(seed, B, C, lengths, n_seg, fps=(12.0, 29.97, 24.0, 23.976)):
    """random windows whose segment bounds sit on exact frame times (f / fps) half of the time"""
    from cfn_hip.seglabels import SegLabel, collate_seg
    r = np.random.RandomState(seed)
    samples = []
    for b in range(B):
        f = fps[b % len(fps)]
        start = int(r.randint(0, 50))
        segs = []
        for _ in range(n_seg[b % len(n_seg)]):
            f0 = int(r.randint(0, start + max(lengths[b], 1) + 20))
            f1 = f0 + int(r.randint(1, 40))
            on = r.rand() < 0.5
            segs.append([int(r.randint(0, C)), f0 / f if on else f0 / f + 0.013, f1 / f if on else f1 / f - 0.007])
        samples.append(SegLabel(segs, f, start, lengths[b], n_classes=C))
    return collate_seg(samples)


# B, C, lengths, segments per sample: one element; C = 1 / 33 / 64 / 65 and 15 / 16 (the mask row shares the last 16-row workgroup or opens a
# new one); t_max 256 / 257 (the frame tile), a multiple of 4 or not (16-byte or dword stores); a sample with length 0; more than 128
# segments in one sample (a second LDS chunk)
SHAPES = [(1, 1, [1], [1]), (1, 157, [1], [3]), (2, 1, [5, 3], [2]), (3, 33, [64, 7, 61], [4]), (2, 64, [300, 256], [5]), (2, 65, [257, 13], [5]),
          (3, 15, [40, 0, 33], [6]), (2, 16, [36, 35], [6]), (2, 157, [1027, 640], [300, 7]), (4, 5, [9, 9, 9, 9], [0, 1, 0, 130])]


@pytest.mark.parametrize('B,C,lengths,n_seg', SHAPES)
def test_smallest_shapes(B, C, lengths, n_seg):
    sl = _random_batch(B * 1000 + C, B, C, lengths, n_seg)
    lab, mask, valid = _dense_checked(sl)
    assert valid.tolist() == lengths and lab.shape == (B, C, max(lengths))
    if sum(n_seg) and max(lengths) > 8:
        assert float(lab.sum()) > 0


def test_no_segments_zero_length_and_start_past_the_last_segment():
    from cfn_hip.seglabels import SegLabel, collate_seg
    none = collate_seg([SegLabel([], 24.0, 0, 37), SegLabel([], 30.0, 11, 5)])
    assert tuple(none.seg.shape) == (1, 3)                  # the padding row no offset range covers
    lab, mask, valid = _dense_checked(none)
    assert float(lab.sum()) == 0 and mask.sum(1).tolist() == [37.0, 5.0] and valid.tolist() == [37, 5]
    lab, mask, valid = _dense_checked(collate_seg([SegLabel([[2, 0.0, 1.0]], 24.0, 0, 0, n_classes=7), SegLabel([[2, 0.0, 1.0]], 24.0, 0, 30, n_classes=7)]))
    assert float(lab[0].sum()) == 0 and float(mask[0].sum()) == 0 and float(lab[1, 2].sum()) == 23 and valid.tolist() == [0, 30]
    lab, mask, valid = _dense_checked(collate_seg([SegLabel([[1, 0.5, 2.0], [3, 1.0, 4.0]], 24.0, 96, 50, n_classes=4)]))      # frame 96 = 4.0 s
    assert float(lab.sum()) == 0 and float(mask.sum()) == 50
    # a segment that starts at 0.0 (frame 0 is ON the bound) and one that ends beyond the window
    lab, _, _ = _dense_checked(collate_seg([SegLabel([[0, 0.0, 0.5], [1, 1.0, 99.0]], 24.0, 0, 48, n_classes=2)]))
    assert lab[0, 0].tolist()[:13] == [0.0] + [1.0] * 11 + [0.0] and lab[0, 1].tolist()[24:26] == [0.0, 1.0] and float(lab[0, 1, 25:].sum()) == 23


def test_operator_equals_ops_and_passes_opcheck():
    import cfn_hip.torchlib  # noqa: F401
    from cfn_hip import ops
    for shape in (SHAPES[3], SHAPES[5]):
        sl = _random_batch(7, *shape).to(DEV)
        ys = torch.ops.cfn.seg_labels(sl.seg, sl.offsets, sl.fps, sl.window, sl.n_classes, sl.t_max)
        ref = ops.seg_labels(sl.seg, sl.offsets, sl.fps, sl.window, sl.n_classes, sl.t_max)
        assert len(ys) == 3 and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(ys, ref))
        torch.library.opcheck(torch.ops.cfn.seg_labels.default, (sl.seg, sl.offsets, sl.fps, sl.window, sl.n_classes, sl.t_max),
                              test_utils=('test_schema', 'test_faketensor'))            # (no gradient is registered: labels are targets)
    for bad in (dict(seg=sl.seg.float()), dict(offsets=sl.offsets.long()), dict(fps=sl.fps[:1]), dict(window=sl.window.long()), dict(n_classes=0), dict(t_max=0),
                dict(fps=sl.fps.cpu())):
        with pytest.raises(RuntimeError):
            torch.ops.cfn.seg_labels(*sl._replace(**bad))


def test_out_is_written_in_place_without_allocation_or_synchronisation():
    sl = _random_batch(11, *SHAPES[4]).to(DEV)
    out = _nan_out(sl)
    want = sl.dense()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = sl.dense(out=out)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
    assert all(g is o and g.data_ptr() == o.data_ptr() and torch.equal(g, w) for g, o, w in zip(got, out, want))
    with pytest.raises(RuntimeError, match='out'):
        sl.dense(out=(out[0][:, :, :-1], out[1], out[2]))
    with pytest.raises(RuntimeError, match='out'):
        sl.dense(out=(out[0], out[1], out[2].long()))


@pytest.mark.capture
def test_capture_and_replay_on_new_data():
    from cfn_hip.seglabels import SegLabels
    shape = (3, 33, [64, 7, 61], [4])
    a, b = _random_batch(21, *shape), _random_batch(22, *shape, fps=(30.0, 12.5, 25.0))
    assert a.seg.shape == b.seg.shape and a.t_max == b.t_max and not torch.equal(a.dense_reference()[0], b.dense_reference()[0])
    st = a.to(DEV)                                                    # the static buffers of the graph
    out = _nan_out(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.dense(out=out)                                             # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st.dense(out=out)
    for src in (a, b):
        for dst, s in zip(st[:4], src[:4]):
            dst.copy_(s.to(DEV))
        out[0].fill_(float('nan'))
        out[1].fill_(float('nan'))
        out[2].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want = src.dense_reference()
        assert all(torch.equal(o.cpu(), w) for o, w in zip(out, want))
    assert isinstance(st, SegLabels)


class _Deterministic(object):
    def __enter__(self):
        import cfn_hip
        self.prev = cfn_hip.deterministic(True)

    def __exit__(self, *exc):
        import cfn_hip
        cfn_hip.deterministic(self.prev)


class _SegVideos(torch.utils.data.Dataset):
    """ragged uint8 videos (test_hip_u8_input._U8Videos) whose label member is a SegLabel -- or, dense=True, the dense array of the same
    window; videos 2 and 3 carry no action, so the second batch of two has no segment at all"""

    def __init__(self, n, crop, dense, coarse=False):
        self.n, self.crop, self.dense, self.coarse = n, crop, dense, coarse

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from cfn_hip.seglabels import SegLabel
        r = np.random.RandomState(50 + i)
        T = 8 - 2 * (i % 2)
        clip = r.randint(0, 256, size=(1, T, self.crop, self.crop, 3)).astype(np.uint8)
        fps, start = (24.0, 29.97)[i % 2], 7 * i
        segs = [] if i in (2, 3) else [[int(r.randint(0, 157)), (start + f0) / fps, (start + f0 + 4 + 9 * k) / fps] for k, f0 in enumerate(r.randint(0, T * 10 - 8, 6))]
        label = SegLabel(segs, fps, start, T * 10)
        if self.dense:
            label = label.dense_reference()
        if not self.coarse:
            return clip, label, 'vid%d' % i
        import train_coarse_fineFEAT as tc
        tf = 20 + 4 * (i % 3)
        feat = {k: np.abs(r.randn(c, tf, 7, 7)).astype(np.float32) for k, c in tc.FEAT_DEPTH.items()}
        return clip, label, feat, np.array([2 * (i % 3), T, tf, 1], dtype=np.int64), 'vid%d' % i, 30.0 + i


def _run(mod, monkeypatch, loaders, **kw):
    from test_hip_u8_input import _spy
    seen, stagers = [], []
    with monkeypatch.context() as mp, _Deterministic():
        _spy(mp, mod, seen, stagers)
        torch.manual_seed(0)
        mod.run(batch_size=2, dataloaders=loaders, pretrained=None, log=lambda *_: None, input_norm=(MEAN, STD), **kw)
    assert len(stagers) == 1
    return seen, stagers[0]


def test_segment_labels_feed_train_fine(tmp_path, monkeypatch):
    """Dataset of SegLabel samples -> DataLoader(collate.fine_collate_u8, pin_memory=True) -> HostStager -> train_fine.run, two steps (the
    second batch has no action at all): the losses are BIT-EQUAL to the run fed the dense labels of the same windows, and the labels
    travel as a few hundred bytes"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from cfn_hip.seglabels import SegLabels
    crop = 64

    def go(dense):
        mk = lambda: tud.DataLoader(_SegVideos(6, crop, dense), batch_size=2, shuffle=False, num_workers=0, pin_memory=True, collate_fn=collate.fine_collate_u8)
        if not dense:
            first = next(iter(mk()))
            assert isinstance(first[1], SegLabels) and first[2] is None and first[1].seg.is_pinned()
        return _run(train_fine, monkeypatch, {'train': mk(), 'val': mk()}, max_steps=2, save_model=str(tmp_path / 'f_'))
    sd, std = go(True)
    ss, sts = go(False)
    assert [s[0] for s in sd] == ['train', 'train'] == [s[0] for s in ss]
    for i, (a, b) in enumerate(zip(sd, ss)):
        print('fine run step %d: dense labels cls %r loc %r | segment labels cls %r loc %r' % (i + 1, a[1], a[2], b[1], b[2]))
    assert sd == ss
    assert all(np.isfinite(s[1]) and np.isfinite(s[2]) for s in ss)
    # (the stager runs a batch ahead, so the two runs may have staged 2 or 3 batches: compare per batch) the dense labels are what is saved
    assert std.bytes_staged / std.batches - sts.bytes_staged / sts.batches > 2 * 157 * 60 * 4


def test_segment_labels_feed_train_coarse(tmp_path, monkeypatch):
    """one coarse batch through train_coarse_fineFEAT.run (coarse_collate_u8) in the same way"""
    import torch.utils.data as tud
    import collate
    import train_coarse_fineFEAT as tc

    def go(dense):
        tag = 'dense' if dense else 'seg'
        mk = lambda n: tud.DataLoader(_SegVideos(n, 224, dense, coarse=True), batch_size=2, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.coarse_collate_u8)
        return _run(tc, monkeypatch, {'train': mk(2), 'val': mk(2)}, max_steps=1, save_model=str(tmp_path / ('m_' + tag)),
                    csv_path=str(tmp_path / (tag + '.csv')))
    sd, _ = go(True)
    ss, _ = go(False)
    assert [s[0] for s in sd] == ['train'] == [s[0] for s in ss]
    print('coarse run: dense labels cls %r loc %r | segment labels cls %r loc %r' % (sd[0][1], sd[0][2], ss[0][1], ss[0][2]))
    assert sd == ss and np.isfinite(ss[0][1]) and np.isfinite(ss[0][2])
