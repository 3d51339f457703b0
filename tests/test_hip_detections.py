"""GPU: activity segments decoded from per-frame scores (csrc/detections.hip, cfn_hip/detections.py).

Against decode_reference (the six rules in numpy, tied to the reference's label arrays by test_detections_cpu.py) the device result is
BIT-EQUAL in seg (compared as int64 bit patterns: one fp64 add and one correctly rounded fp64 division give the same double on the device
as on the host), frames, offsets, total and score[:, 0] (a maximum is exact).  score[:, 1] is within 1 fp32 ulp: it is an fp64 sum of at
most 65536 fp32 values, whose relative error stays below 65536 * 2^-53 = 2^-37 in any order, so the kernel's fixed order and numpy's can
differ only in the final rounding to fp32; between two calls it is bit-equal.  Every output is handed over filled with a canary, so a row
the kernel should not touch (behind min(total, cap)) or does not write shows.

The kernel's boundaries: a lane holds 4 frames and a wave 256 (four 64-bit mask words), a workgroup pass covers 1024 frames (PASS below), rows
whose length is a multiple of 4 are loaded 16 bytes per lane and the others by dwords, a thread owns ceil(words / 256) mask words."""
import json

import numpy as np
import pytest
import torch

import seg_fixture as sf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]
PASS = 1024                                        # frames per workgroup pass (DS_PASS in csrc/detections.hip)
CANARY_F, CANARY_I = -777.25, -12345


def _golden_fps():
    r = sf.records()[1]
    return r['num_frames'] / r['duration']


def _canary_out(B, C, TL, rows=None):
    from cfn_hip import ops
    rows = ops.decode_segments_cap(B, C, TL) if rows is None else rows
    return (torch.full((rows, 3), CANARY_F, dtype=torch.float64, device=DEV), torch.full((rows, 3), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((rows, 2), CANARY_F, dtype=torch.float32, device=DEV), torch.full((B + 1,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((1,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.empty(ops.decode_segments_workspace_bytes(B, C, TL), dtype=torch.uint8, device=DEV))


def _ulps(a, b):
    """distance in fp32 steps of two float32 arrays without NaN (equal infinities: 0)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _check(got, ref, rows_written=None):
    """got: Detections on the GPU over canary-filled buffers; ref: decode_reference (exactly its rows).  -> number of segments"""
    total = int(ref.total.item())
    k = total if rows_written is None else rows_written
    assert got.total.cpu().tolist() == [total] and got.offsets.cpu().tolist() == ref.offsets.tolist()
    seg, frames, score = got.seg.cpu(), got.frames.cpu(), got.score.cpu()
    assert torch.equal(seg[:k].view(torch.int64), ref.seg[:k].view(torch.int64)), 'seg differs in its bits'
    assert torch.equal(frames[:k], ref.frames[:k])
    assert torch.equal(score[:k, 0].contiguous().view(torch.int32), ref.score[:k, 0].contiguous().view(torch.int32)), 'score max'
    if k:
        assert not bool(torch.isnan(score[:k]).any())
        worst = int(_ulps(score[:k, 1].contiguous().numpy(), ref.score[:k, 1].contiguous().numpy()).max())
        assert worst <= 1, 'score mean: %d fp32 ulps from the reference' % worst
    # rows behind min(total, cap) are not touched
    assert bool((seg[k:] == CANARY_F).all()) and bool((frames[k:] == CANARY_I).all()) and bool((score[k:] == CANARY_F).all())
    return total


def _decode_checked(probs, valid, fps, start, thr, max_gap=0, min_len=1):
    """decode(out=canaries) of host tensors on the GPU against decode_reference, twice: the second call gives the same bits"""
    from cfn_hip.detections import decode, decode_reference
    B, C, TL = probs.shape
    ref = decode_reference(probs, valid, fps, start, thr, max_gap, min_len)
    dthr = thr.to(DEV) if torch.is_tensor(thr) else thr
    args = (probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), dthr, max_gap, min_len)
    out = _canary_out(B, C, TL)
    got = decode(*args, out=out)
    assert all(g is o for g, o in zip(got[:5], out[:5])) and got.n_classes == C and got.cap == out[0].shape[0]
    n = _check(got, ref)
    again = decode(*args, out=_canary_out(B, C, TL))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(again[:5], got[:5])), 'two calls differ'
    return n, got, ref


def _batch_meta(B, TL, seed):
    """a different valid_t per sample, 0 and TL among them; non-trivial fps and start"""
    valid = [TL, 0, TL // 2 + 1, max(TL - 3, 0)]
    fps = [24.0, 29.97, _golden_fps(), 12.5]
    start = [0, 17, 12345, 3]
    pick = lambda v: [v[(b + seed) % 4] if B > 1 else v[0] for b in range(B)]
    return (torch.tensor(pick(valid), dtype=torch.int32), torch.tensor([fps[(b + seed) % 4] for b in range(B)], dtype=torch.float64),
            torch.tensor([start[(b + seed + 1) % 4] for b in range(B)], dtype=torch.int32))


# 1 frame; 63 / 64 / 65 (one mask word, a second one); 127 / 129, 255 / 257 (a wave's 256 frames); 1000 and 1028 (16-byte loads, 1028 is one
# lane over a pass); PASS + 1 (dword loads, a second pass for one frame)
@pytest.mark.parametrize('TL', [1, 63, 64, 65, 127, 129, 255, 257, 1000, PASS + 1, PASS + 4])
@pytest.mark.parametrize('B,C', [(1, 1), (3, 5), (2, 157)])
def test_random_rows_at_every_boundary(B, C, TL):
    """uniform probs against thresholds that leave 2 %, 50 % and 98 % of the frames active, with and without gap closing and min_len"""
    g = torch.Generator().manual_seed(1000 * TL + 10 * B + C)
    probs = torch.rand(B, C, TL, generator=g)
    found = 0
    for i, (density, max_gap, min_len) in enumerate(((0.02, 0, 1), (0.5, 0, 1), (0.98, 0, 1), (0.02, 70, 2), (0.5, 1, 3), (0.98, 3, 70))):
        valid, fps, start = _batch_meta(B, TL, i)
        thr = torch.full((C,), 1.0 - density) if i % 2 else 1.0 - density          # a float, or a (C,) tensor
        n, _, _ = _decode_checked(probs, valid, fps, start, thr, max_gap, min_len)
        found += n
    assert found > 0 or TL == 1


def _crafted(TL):
    """rows whose runs and gaps sit on the 64-lane and the pass boundary: [(active frames, note)]"""
    P = PASS
    return [list(range(60, 71)),                                   # a run over a 64-lane boundary
            list(range(P - 4, P + 7)),                             # ... over the pass boundary
            [62, 66],                                              # a gap of 3 over the lane boundary
            [P - 2, P + 2],                                        # ... over the pass boundary
            [63, 64],                                              # the last and the first bit of two words
            [0, TL - 1],                                           # the ends of the row
            [5] + list(range(100, 400)) + [P + 3],                 # a run over several words
            list(range(0, TL)),                                    # everything
            []]


@pytest.mark.parametrize('TL', [PASS + 76, PASS + 77])            # 16-byte and dword loads
def test_runs_and_gaps_across_the_lane_and_pass_boundaries(TL):
    rows = _crafted(TL)
    C = len(rows)
    probs = torch.full((1, C, TL), 0.25)
    for c, on in enumerate(rows):
        probs[0, c, on] = torch.linspace(0.6, 0.95, len(on)) if on else torch.zeros(0)
    probs[0, 2, 63:66] = float('nan')                              # the closed gap holds NaNs: never active, never in a score
    valid, fps, start = torch.tensor([TL], dtype=torch.int32), torch.tensor([29.97], dtype=torch.float64), torch.tensor([250], dtype=torch.int32)
    n, got, ref = _decode_checked(probs, valid, fps, start, 0.5, 0, 1)
    fr = got.frames.cpu()[:n, :2].tolist()
    off = [0] + np.cumsum([len(f) for f in ([[60, 70]], [[PASS - 4, PASS + 6]], [[62, 62], [66, 66]], [[PASS - 2, PASS - 2], [PASS + 2, PASS + 2]], [[63, 64]],
                                            [[0, 0], [TL - 1, TL - 1]], [[5, 5], [100, 399], [PASS + 3, PASS + 3]], [[0, TL - 1]], [])]).tolist()
    assert fr[off[0]:off[1]] == [[60, 70]] and fr[off[1]:off[2]] == [[PASS - 4, PASS + 6]] and fr[off[4]:off[5]] == [[63, 64]]
    assert fr[off[7]:off[8]] == [[0, TL - 1]] and n == off[-1]
    # a gap of exactly 3 closes with max_gap = 3 across either boundary, not with 2; the long gaps stay open
    n3, got3, _ = _decode_checked(probs, valid, fps, start, 0.5, 3, 1)
    fr3 = got3.frames.cpu()[:n3].tolist()
    assert [62, 66, 2] in fr3 and [PASS - 2, PASS + 2, 2] in fr3 and [0, 0, 1] in fr3 and [100, 399, 300] in fr3
    n2, got2, _ = _decode_checked(probs, valid, fps, start, 0.5, 2, 1)
    assert n2 == n
    # a gap longer than a word, and min_len over the closed run
    nb, gotb, _ = _decode_checked(probs, valid, fps, start, 0.5, TL, 1)
    assert nb == C - 1 and [0, TL - 1, 2] in gotb.frames.cpu()[:nb].tolist() and [5, PASS + 3, 302] in gotb.frames.cpu()[:nb].tolist()
    nm, gotm, _ = _decode_checked(probs, valid, fps, start, 0.5, 3, 5)
    assert sorted(f[1] - f[0] + 1 for f in gotm.frames.cpu()[:nm].tolist())[0] >= 5 and [62, 66, 2] in gotm.frames.cpu()[:nm].tolist()


def test_alternating_frames_fill_the_default_cap_exactly():
    from cfn_hip import ops
    B, C, TL = 2, 3, 129
    probs = torch.zeros(B, C, TL)
    probs[:, :, ::2] = 0.75
    valid, fps, start = torch.full((B,), TL, dtype=torch.int32), torch.tensor([24.0, 29.97], dtype=torch.float64), torch.tensor([0, 9], dtype=torch.int32)
    n, got, _ = _decode_checked(probs, valid, fps, start, 0.5)
    assert n == ops.decode_segments_cap(B, C, TL) == B * C * 65 == got.seg.shape[0] and got.check() == n
    assert bool((got.frames[:, 2] == 1).all()) and got.offsets.cpu().tolist() == [0, C * 65, n]


def test_overflow_keeps_the_prefix_and_the_true_counts():
    from cfn_hip.detections import decode, decode_reference
    B, C, TL = 3, 5, 257
    probs = torch.rand(B, C, TL, generator=torch.Generator().manual_seed(5))
    valid, fps, start = _batch_meta(B, TL, 2)
    ref = decode_reference(probs, valid, fps, start, 0.5)
    total = ref.check()
    cap = total // 2
    assert cap > 10
    out = _canary_out(B, C, TL, rows=total + 7)                    # larger buffers: the rows behind cap must stay as they are
    got = decode(probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), 0.5, cap=cap, out=out)
    assert got.cap == cap
    assert _check(got, ref, rows_written=cap) == total             # total and offsets are the true values, rows < cap the reference prefix
    with pytest.raises(RuntimeError, match=r'%d segments.*cap = %d' % (total, cap)):
        got.check()
    with pytest.raises(RuntimeError, match='cap'):
        got.tolist()
    fits = decode(probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), 0.5, cap=total)
    assert fits.check() == total and fits.cap == total and _ulps_only(fits.tolist(), ref.tolist())


def _ulps_only(a, b):
    """two tolist() results equal but for score_mean within 1 fp32 ulp"""
    assert len(a) == len(b)
    for va, vb in zip(a, b):
        assert len(va) == len(vb)
        for ra, rb in zip(va, vb):
            assert {k: v for k, v in ra.items() if k != 'score_mean'} == {k: v for k, v in rb.items() if k != 'score_mean'}
            assert int(_ulps(np.array([ra['score_mean']], np.float32), np.array([rb['score_mean']], np.float32))[0]) <= 1
    return True


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_device_round_trip_gives_the_labels_back(name):
    """ops.seg_labels(batch) -> ops.decode_segments -> as_seg_labels(...).dense() equals the first labels exactly, and those are the
    reference's (mt_collate_fn's) arrays"""
    from cfn_hip.detections import decode
    from cfn_hip.seglabels import collate_seg
    split, idx, labels, masks = sf.batch(name)
    sl = collate_seg([sf.seglabel(i, split) for i in idx]).to(DEV)
    lab, mask, valid = sl.dense()
    det = decode(lab, valid, sl.fps, sl.window[:, 0].contiguous(), 0.5)
    assert 0 < det.check() <= det.cap
    lab2, mask2, valid2 = det.as_seg_labels(sl.fps, sl.window, sl.t_max).dense()
    assert torch.equal(lab2, lab) and torch.equal(mask2, mask) and torch.equal(valid2, valid)
    assert int((lab2.cpu().numpy() != labels).sum()) == 0


def _fixed_case(seed, B=3, C=33, TL=200):
    probs = torch.rand(B, C, TL, generator=torch.Generator().manual_seed(seed))
    valid, fps, start = _batch_meta(B, TL, seed)
    return probs, valid, fps, start


def test_out_is_written_in_place_without_allocation_or_synchronisation():
    from cfn_hip.detections import decode, decode_reference
    probs, valid, fps, start = _fixed_case(3)
    ref = decode_reference(probs, valid, fps, start, 0.7, 2, 2)
    args = (probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), torch.full((33,), 0.7, device=DEV), 2, 2)
    out = _canary_out(3, 33, 200)
    decode(*args)                                                  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    held = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = decode(*args, out=out)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before and torch.cuda.memory_allocated() == held
    assert all(g is o and g.data_ptr() == o.data_ptr() for g, o in zip(got[:5], out[:5]))
    _check(got, ref)
    for bad in ((out[0][:-1],) + out[1:], out[:3] + (out[3].long(),) + out[4:], out[:5] + (out[5][:16],), out[:5]):
        with pytest.raises(RuntimeError, match='out'):
            decode(*args, out=bad)


@pytest.mark.capture
def test_capture_and_replay_on_new_data():
    from cfn_hip.detections import decode, decode_reference
    cases = [_fixed_case(21), _fixed_case(22)]
    thr = torch.linspace(0.3, 0.9, 33)
    static = [t.to(DEV).clone() for t in cases[0]] + [thr.to(DEV)]
    out = _canary_out(3, 33, 200)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        decode(*static, 1, 2, out=out)                             # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = decode(*static, 1, 2, out=out)
    totals = []
    for case in cases:
        for dst, src in zip(static[:4], case):
            dst.copy_(src.to(DEV))
        for o, v in zip(out[:5], (CANARY_F, CANARY_I, CANARY_F, CANARY_I, CANARY_I)):
            o.fill_(v)
        graph.replay()
        torch.cuda.synchronize()
        totals.append(_check(got, decode_reference(*case, thr, 1, 2)))
    assert totals[0] != totals[1] and min(totals) > 0


class _Deterministic(object):
    def __enter__(self):
        import cfn_hip
        self.prev = cfn_hip.deterministic(True)

    def __exit__(self, *exc):
        import cfn_hip
        cfn_hip.deterministic(self.prev)


def test_deterministic_mode_gives_the_same_bits():
    from cfn_hip.detections import decode, decode_reference
    probs, valid, fps, start = _fixed_case(8)
    args = (probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), 0.6, 1, 2)
    plain = decode(*args, out=_canary_out(3, 33, 200))
    with _Deterministic():
        det = decode(*args, out=_canary_out(3, 33, 200))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(det[:5], plain[:5]))
    _check(det, decode_reference(probs, valid, fps, start, 0.6, 1, 2))


# ---- end to end: the training scripts write what decode_reference gives for the validation probs ---------------------------------------
class _SegVideos(torch.utils.data.Dataset):
    """ragged uint8 videos whose label member is a SegLabel -- or, dense=True, the dense array of the same window (the tiny loaders of
    test_hip_seglabels.py); video 2 carries no action"""

    def __init__(self, n, crop, dense, coarse=False):
        self.n, self.crop, self.dense, self.coarse = n, crop, dense, coarse

    def __len__(self):
        return self.n

    @staticmethod
    def meta(i):
        return (24.0, 29.97)[i % 2], 7 * i, 8 - 2 * (i % 2)       # fps, first frame, clip frames (10 label frames each)

    def __getitem__(self, i):
        from cfn_hip.seglabels import SegLabel
        r = np.random.RandomState(50 + i)
        fps, start, T = self.meta(i)
        clip = r.randint(0, 256, size=(1, T, self.crop, self.crop, 3)).astype(np.uint8)
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


def _run(mod, monkeypatch, loaders, detections, **kw):
    """mod.run under the deterministic mode -> (losses of every step and validation batch, logged lines, validation (probs, valid_t) per batch)"""
    real_step, real_loss = mod.train_step, mod.detection_loss
    losses, lines, val = [], [], []

    def step(*a, **k):
        out = real_step(*a, **k)
        losses.append(('train', float(out[0]), float(out[1])))
        return out

    def loss(*a, **k):
        out = real_loss(*a, **k)
        if not torch.is_grad_enabled():                            # the validation branch of run()
            losses.append(('val', float(out[0]), float(out[1])))
            val.append((out[2].detach().cpu().clone(), a[2].sum(1).int().cpu()))
        return out
    with monkeypatch.context() as mp, _Deterministic():
        mp.setattr(mod, 'train_step', step)
        mp.setattr(mod, 'detection_loss', loss)
        torch.manual_seed(0)
        mod.run(batch_size=2, dataloaders=loaders, pretrained=None, log=lines.append, input_norm=(MEAN, STD), detections=detections, **kw)
    return losses, lines, val


def _expected_rows(val, n_val, seconds, thr, max_gap, min_len):
    """the file's objects from decode_reference of the spied validation probs (one video per batch)"""
    from cfn_hip.detections import decode_reference
    rows = []
    assert len(val) == n_val
    for i, (probs, valid) in enumerate(val):
        fps, start, _ = _SegVideos.meta(i)
        det = decode_reference(probs, valid, torch.tensor([fps], dtype=torch.float64) if seconds else None,
                               torch.tensor([start], dtype=torch.int32) if seconds else None, thr, max_gap, min_len)
        rows.append({'video': 'vid%d' % i, 'unit': 's' if seconds else 'frame', 'segments': det.tolist()[0]})
    return rows


def _same_file(path, want):
    from cfn_hip.detections import read_detections
    got = read_detections(path)
    assert [(r['video'], r['unit']) for r in got] == [(r['video'], r['unit']) for r in want]
    assert _ulps_only([r['segments'] for r in got], [r['segments'] for r in want])
    return sum(len(r['segments']) for r in got)


def test_train_fine_writes_the_detections_of_its_validation_phase(tmp_path, monkeypatch):
    """four one-batch training phases and one validation phase of three videos: the file of epoch 4 equals decode_reference of the
    validation probs -- in seconds for a SegLabel loader, in frames for a dense one -- and the losses and the logged lines are BIT-EQUAL
    to the same run without a writer"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from cfn_hip.detections import DetectionWriter, epoch_path
    crop, thr, gap, mlen = 64, 0.5, 2, 2

    def go(dense, tag, detect=True):
        mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, dense), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                          collate_fn=collate.fine_collate_u8)
        w = DetectionWriter(str(tmp_path / tag / 'det.jsonl'), thr, gap, mlen) if detect else None
        return (w,) + _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, w, max_epochs=4, save_model=str(tmp_path / (tag + '_')))
    w, losses, lines, val = go(False, 'seg')
    assert [k for k, _, _ in losses] == 4 * ['train'] + 3 * ['val'] and len(lines) == 1 and 'val' in lines[0]
    n = _same_file(epoch_path(w.path, 4), _expected_rows(val, 3, True, thr, gap, mlen))
    print('train_fine: %d segments in 3 validation videos (seconds)' % n)
    assert n > 0 and w.take() == []
    _, losses0, lines0, _ = go(False, 'none', detect=False)
    assert losses0 == losses and lines0 == lines
    w, _, _, val = go(True, 'dense')
    assert _same_file(epoch_path(w.path, 4), _expected_rows(val, 3, False, thr, gap, mlen)) > 0


def test_train_coarse_writes_the_detections_of_its_validation_phase(tmp_path, monkeypatch):
    """the same once through train_coarse_fineFEAT.run: two training phases, one validation phase of two videos"""
    import torch.utils.data as tud
    import collate
    import train_coarse_fineFEAT as tc
    from cfn_hip.detections import DetectionWriter, epoch_path
    thr, gap, mlen = 0.5, 2, 2

    def go(tag, detect=True):
        mk = lambda n, bs: tud.DataLoader(_SegVideos(n, 224, False, coarse=True), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                          collate_fn=collate.coarse_collate_u8)
        w = DetectionWriter(str(tmp_path / tag / 'det.jsonl'), thr, gap, mlen) if detect else None
        return (w,) + _run(tc, monkeypatch, {'train': mk(2, 2), 'val': mk(2, 1)}, w, max_epochs=2, save_model=str(tmp_path / ('m_' + tag)),
                           csv_path=str(tmp_path / (tag + '.csv')))
    w, losses, lines, val = go('seg')
    assert [k for k, _, _ in losses] == 2 * ['train'] + 2 * ['val'] and len(lines) == 1
    n = _same_file(epoch_path(w.path, 2), _expected_rows(val, 2, True, thr, gap, mlen))
    print('train_coarse_fineFEAT: %d segments in 2 validation videos (seconds)' % n)
    assert n > 0
    _, losses0, lines0, _ = go('none', detect=False)
    assert losses0 == losses and lines0 == lines
    assert json.loads(open(epoch_path(w.path, 2)).readline())['video'] == 'vid0'
