"""GPU: soft-NMS of activity proposals (csrc/segnms.hip soft_select / soft_write, cfn_soft_nms_segments), cfn_hip/detections.py soft_nms /
propose(soft=).

Against soft_nms_reference (rules S1-S7 in numpy, checked by hand and against a row-by-row spelling in test_softnms_cpu.py) the device result
is BIT-EQUAL, everywhere, over canary-filled buffers, and bit-equal between two calls.  That can be asked because the rule fixes every fp64
operation and its order: one IEEE division per tIoU (rule N3), one subtraction or one E (rule S5: a polynomial and ten squarings without
fused multiply-add, so neither side's exp is involved) and one product per decay, applied in selection order, and one rounding to fp32.

The kernel's boundaries: candidate j of a group belongs to lane j & 63 (63 / 64 / 65); a group of up to NMS_DET_TILE = 1024 candidates keeps
start, end and the working scores in LDS (1023 / 1024), a larger one keeps the working scores in the workspace (1025)."""
import numpy as np
import pytest
import torch

import seg_fixture as sf
import segap_fixture as fx
from proposals_fixture import LEVELS5, candidates, random_probs
from softnms_fixture import FLOOR, SIZES, SUBNORMAL_KEEP, boundary_batch, first_rows, subnormal_batch
from test_hip_proposals import CANARY_B, CANARY_F, CANARY_I, DEV, _bits, _levels_out, _meta, _same_records

pytestmark = pytest.mark.gpu


def _soft_out(B, C, cap_in, rows=None):
    from cfn_hip import ops
    rows = cap_in if rows is None else rows
    return (torch.full((rows, 3), CANARY_F, dtype=torch.float64, device=DEV), torch.full((rows, 3), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((rows, 2), CANARY_F, dtype=torch.float32, device=DEV), torch.full((B + 1,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.full((1,), CANARY_I, dtype=torch.int32, device=DEV), torch.full((cap_in,), CANARY_B, dtype=torch.uint8, device=DEV),
            torch.full((rows,), CANARY_I, dtype=torch.int32, device=DEV),
            torch.empty(ops.soft_nms_segments_workspace_bytes(B, C, cap_in), dtype=torch.uint8, device=DEV))


def _soft_checked(det, soft, thr=0.5, score='max', cap=None, twice=True, d=None):
    """soft_nms(out=canaries) of a host Detections on the GPU against soft_nms_reference, twice.  -> (selected, reference result, keep, src)"""
    from cfn_hip.detections import SoftNMS, soft_nms, soft_nms_reference
    soft = SoftNMS(*soft)
    ref, ref_keep, ref_src = soft_nms_reference(det, soft, thr, score)
    total, n_in = int(ref.total), int(ref_keep.numel())
    d = det.to(DEV) if d is None else d
    B, cap_in = d.batch, int(d.cap)
    out = _soft_out(B, d.n_classes, cap_in, rows=None if cap is None else total + 5)
    got, keep, src = soft_nms(d, soft, thr, score, cap=cap, out=out)
    assert all(g is o for g, o in zip(got[:5], out[:5])) and keep is out[5] and src is out[6] and got.n_classes == det.n_classes
    k = total if cap is None else min(total, cap)
    assert got.cap == (cap_in if cap is None else cap)
    _same_records(got, ref, k)
    keep, src = keep.cpu(), src.cpu()
    assert torch.equal(keep[:n_in], ref_keep), 'keep differs at rows %s' % torch.nonzero(keep[:n_in] != ref_keep).flatten()[:8].tolist()
    assert bool((keep[n_in:] == CANARY_B).all())                                         # rows of no group are not touched
    assert torch.equal(src[:k], ref_src[:k]) and bool((src[k:] == CANARY_I).all())
    if twice:
        again, keep2, src2 = soft_nms(d, soft, thr, score, cap=cap, out=_soft_out(B, d.n_classes, cap_in, rows=None if cap is None else total + 5))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again[:5], got[:5])) and torch.equal(keep2.cpu(), keep) and torch.equal(src2.cpu(), src)
    return total, ref, ref_keep, ref_src


def _changed(det, ref, src, col=0):
    n = int(ref.total)
    return int((ref.score[:n, col] != det.score[src[:n].long(), col]).sum())


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('nd', SIZES)
def test_soft_nms_at_the_group_sizes_that_change_the_path(nd, method):
    """B = 2, C = 3: two groups of nd candidates beside groups of 5, 1 and 0.  The reference selects a decayed row at every size and drops a
    row from 63 candidates on (test_softnms_cpu.py checks the same premises without a GPU)"""
    det = boundary_batch(nd)
    assert int(det.total) == 2 * nd + 6
    kept, ref, keep, src = _soft_checked(det, (method, 0.5, FLOOR, 0), 0.5, 'max')
    assert _changed(det, ref, src) > 0 and (nd < 63 or 0 < kept < int(det.total))
    kept_mean, ref, keep_mean, src = _soft_checked(det, (method, 0.5, FLOOR, 0), 0.5, 'mean')
    assert _changed(det, ref, src, 1) > 0 and (nd < 63 or (0 < kept_mean < int(det.total) and not torch.equal(keep, keep_mean)))


CUTS = ((0.0, 0), (0.001, 0), (0.3, 0), (0.001, 1), (0.001, 10), (0.0, 10), (0.3, 1))       # (min_score, max_keep)


@pytest.mark.parametrize('score', ['max', 'mean'])
@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('nd', [65, 1025])
def test_parameter_corners(nd, method, score):
    """sigma 1/64, 0.5, 4 (gaussian; linear does not read it) or nms_thr 0, 0.5, 1 (linear; gaussian does not read it), each with min_score
    0, 0.001, 0.3 and max_keep 0, 1, 10, on both score columns"""
    det = boundary_batch(nd)
    d = det.to(DEV)
    seen = set()
    for v in (1.0 / 64.0, 0.5, 4.0) if method == 'gaussian' else (0.0, 0.5, 1.0):
        for floor, count in CUTS:
            sigma, thr = (v, 0.5) if method == 'gaussian' else (0.5, v)
            kept = _soft_checked(det, (method, sigma, floor, count), thr, score, twice=False, d=d)[0]
            assert 0 < kept <= int(det.total) and (count == 0 or kept <= 4 * count)       # (four groups are not empty)
            seen.add(kept)
    assert len(seen) > 6
    if method == 'linear':                                                               # S7: nothing decays at 1, nothing is cut at 0
        assert _soft_checked(det, ('linear', 0.5, 0.0, 0), 1.0, score, twice=False, d=d)[0] == int(det.total)


def test_subnormal_working_scores_follow_ieee():
    """16 identical segments at sigma = 1/64: the working scores pass through the fp64 subnormal range (softnms_fixture.subnormal_batch).  The
    finals are 0 in fp32 there, so it is the ORDER that shows a flush: the count of 12 cuts between the subnormal row and the zeros"""
    sub = subnormal_batch()
    kept, ref, keep, _ = _soft_checked(sub, ('gaussian', 1.0 / 64.0, 0.0, 0))
    assert kept == 16 and ref.score[:, 0].tolist()[:13] == [0.0] * 13
    kept, ref, keep, _ = _soft_checked(sub, ('gaussian', 1.0 / 64.0, 0.0, SUBNORMAL_KEEP))
    assert kept == SUBNORMAL_KEEP and keep.tolist() == [0] * 4 + [1] * 12


def test_identities_on_the_device():
    """S7: linear at nms_thr = 1 returns its input; a real single-level decode passes through both methods; max_keep = 1 leaves hard NMS's
    first row of every group, which is also the first row selected without a count, undecayed"""
    from cfn_hip.detections import SCORE_COLUMNS, SoftNMS, decode, nms, soft_nms
    det = candidates(9, [{0: 65, 1: 1200}, {}, {1: 130, 3: 2}], 4, span=60.0)
    n = int(det.total)
    d = det.to(DEV)
    for score in ('max', 'mean'):
        out, keep, src = soft_nms(d, SoftNMS('linear', 0.5, 0.0, 0), 1.0, score)
        assert out.check() == n and all(torch.equal(_bits(a[:n]), _bits(b[:n])) for a, b in zip(out[:3], d[:3])) and torch.equal(out.offsets, d.offsets)
        assert bool(keep[:n].all()) and src[:n].cpu().tolist() == list(range(n))
    B, C, TL = 3, 6, 200
    valid, fps, start = _meta(B, TL)
    one = decode(random_probs(21, B, C, TL).to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), 0.35, 1, 2)
    m = one.check()
    assert m > 10
    for soft in (SoftNMS(), SoftNMS('linear'), SoftNMS('gaussian', 1.0 / 64.0, 0.35, 0)):
        for score in ('max', 'mean'):
            out = soft_nms(one, soft, 0.0, score)[0]
            assert out.check() == m and all(torch.equal(_bits(a[:m]), _bits(b[:m])) for a, b in zip(out[:3], one[:3])) and torch.equal(out.offsets, one.offsets)
    for method in ('linear', 'gaussian'):
        for score in ('max', 'mean'):
            first, col = first_rows(det, score), SCORE_COLUMNS[score]
            out, keep, src = soft_nms(d, SoftNMS(method, 0.5, 0.001, 1), 0.5, score)
            assert out.check() == len(first) and src[:len(first)].cpu().tolist() == first
            assert all(torch.equal(_bits(a[:len(first)].cpu()), _bits(b[first])) for a, b in zip(out[:3], det[:3]))
            hard = nms(d, 0.5, score)[1].cpu()
            assert all(int(hard[i]) == 1 for i in first)
            full, keep, src = soft_nms(d, SoftNMS(method, 0.5, 0.001, 0), 0.5, score)
            pos = {int(r): i for i, r in enumerate(src[:full.check()].cpu().tolist())}
            fs = full.score.cpu()
            assert all(fs[pos[i], col] == det.score[i, col] for i in first)


def test_empty_batch_overflown_input_and_small_cap_out():
    from cfn_hip.detections import Detections
    none = fx.make_det([[], [], []], 4)
    assert _soft_checked(none, ('gaussian', 0.5, 0.001, 0))[0] == 0
    det = candidates(8, [{0: 70, 2: 40}, {1: 90}], 3, span=30.0)
    for soft in (('gaussian', 0.5, 0.05, 0), ('linear', 0.5, 0.05, 0)):
        total, ref, _, _ = _soft_checked(det, soft, 0.5, cap=11)                         # rows >= cap_out are not written, the counts are true
        assert total > 11 and ref.offsets.tolist()[-1] == total
        # an input whose decode overflowed its cap: offsets count 200 rows, 150 were written; the rows behind cap are no candidates
        over = Detections(det.seg[:150].contiguous(), det.frames[:150].contiguous(), det.score[:150].contiguous(), det.offsets, det.total, 3, 150)
        kept, ref, keep, _ = _soft_checked(over, soft, 0.5)
        assert int(over.total) == 200 and keep.numel() == 150 and ref.offsets.tolist()[1] == int(keep[:110].sum()) and kept == int(keep.sum())
        # buffers longer than cap (out= of a decode): only the first cap rows are candidates
        longer = Detections(det.seg, det.frames, det.score, det.offsets, det.total, 3, 150)
        assert _soft_checked(longer, soft, 0.5)[0] == kept


def test_hand_cases_on_the_device():
    """the chain, the tie the decay makes, strictness and the rows that are out (test_softnms_cpu.py types the expected doubles out)"""
    chain = [(0, 0, 10, 0.9, 0.1), (0, 4, 14, 0.8, 0.2), (0, 8, 18, 0.7, 0.3)]
    det = fx.make_det([chain], 1)
    thr = float(np.float64(6) / np.float64(14))
    for soft, t in ((('linear', 0.5, 0.0, 0), 0.4), (('linear', 0.5, 0.3, 0), 0.4), (('linear', 0.5, 0.0, 2), 0.4), (('linear', 0.5, 0.0, 0), thr),
                    (('linear', 0.5, 0.0, 0), float(np.nextafter(thr, 0.0))), (('gaussian', 0.5, 0.0, 0), 0.5), (('gaussian', 1.0 / 64.0, 0.001, 0), 0.5)):
        for score in ('max', 'mean'):
            _soft_checked(det, soft, t, score)
    tie = fx.make_det([[(0, 0, 10, 1.0, 0.5), (0, 5, 10, 1.0, 0.5), (0, 40, 50, 0.5, 0.5)]], 1)
    assert _soft_checked(tie, ('linear', 0.5, 0.0, 2), 0.4)[2].tolist() == [1, 1, 0]
    for bad in (float('nan'), float('inf'), float('-inf')):
        rows = [(0, 0, 10, 0.9, 0.1), (0, 1, 10, bad, 0.2), (0, 4, 14, 0.8, 0.2), (0, 8, 18, 0.7, 0.3)]
        for method in ('linear', 'gaussian'):
            assert _soft_checked(fx.make_det([rows], 1), (method, 0.5, 0.0, 0), 0.4)[2].tolist() == [1, 0, 1, 1]


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_golden_labels_through_propose_with_soft_nms(name):
    """ops.seg_labels(batch) decoded at levels (0.75, 0.5, 0.25) gives three identical copies of every segment: propose(soft=) equals the
    reference pipeline row for row.  Under linear an exact copy (tIoU 1) decays to w * (1 - 1) = 0, so above a floor exactly
    decode(thr=0.5)'s rows are left, bit for bit"""
    from cfn_hip.detections import SoftNMS, decode, propose
    from cfn_hip.seglabels import collate_seg
    split, idx, labels, masks = sf.batch(name)
    sl = collate_seg([sf.seglabel(i, split) for i in idx])
    dev = sl.to(DEV)
    lab, mask, valid = dev.dense()
    start = dev.window[:, 0].contiguous()
    one = decode(lab, valid, dev.fps, start, 0.5)
    n = one.check()
    for soft in (SoftNMS('linear', 0.5, 0.001, 0), SoftNMS('gaussian', 0.5, 0.001, 0), SoftNMS('gaussian', 1.0 / 64.0, 0.0, 0), SoftNMS('linear', 0.5, 0.0, 2)):
        got = propose(lab, valid, dev.fps, start, (0.75, 0.5, 0.25), 0.5, soft=soft)
        ref = propose(lab.cpu(), valid.cpu(), sl.fps, sl.window[:, 0].contiguous(), (0.75, 0.5, 0.25), 0.5, soft=soft, reference=True)
        k = ref.check()
        assert got.check() == k > 0 and torch.equal(got.offsets.cpu(), ref.offsets)
        assert all(torch.equal(_bits(a[:k].cpu()), _bits(b[:k])) for a, b in zip(got[:3], ref[:3]))
        if soft.method == 'linear' and soft.max_keep == 0:                               # 1 - tIoU = 0 for an exact copy
            assert k == n and all(torch.equal(_bits(a[:n]), _bits(b[:n])) for a, b in zip(got[:3], one[:3]))


@pytest.mark.capture
@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_propose_soft_with_out_allocates_nothing_and_replays_on_new_data(method):
    from cfn_hip import ops
    from cfn_hip.detections import SoftNMS, levels_tensor, propose
    B, C, TL = 3, 7, 200
    soft = SoftNMS(method, 0.5, 0.05, 0)
    cases = [(random_probs(31 + i, B, C, TL),) + _meta(B, TL) for i in range(2)]
    levels = levels_tensor(LEVELS5, C, DEV)
    static = [t.to(DEV).clone() for t in cases[0]]
    out = _levels_out(B, C, 5, TL), _soft_out(B, C, ops.decode_segments_levels_cap(B, C, 5, TL))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        propose(*static, levels, 0.5, 'max', 1, 2, out=out, soft=soft)      # warm-up outside the capture
    side.synchronize()
    before, held = torch.cuda.memory_stats()['allocation.all.allocated'], torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode('error')
    try:
        propose(*static, levels, 0.5, 'max', 1, 2, out=out, soft=soft)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.cuda.memory_stats()['allocation.all.allocated'] == before and torch.cuda.memory_allocated() == held
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = propose(*static, levels, 0.5, 'max', 1, 2, out=out, soft=soft)
    assert all(g is o for g, o in zip(got[:5], out[1][:5]))
    totals = []
    for case in cases:
        for dst, src in zip(static, case):
            dst.copy_(src.to(DEV))
        for o, v in zip(out[1][:5], (CANARY_F, CANARY_I, CANARY_F, CANARY_I, CANARY_I)):
            o.fill_(v)
        graph.replay()
        torch.cuda.synchronize()
        ref = propose(*case, LEVELS5, 0.5, 'max', 1, 2, reference=True, soft=soft)
        hard = propose(*case, LEVELS5, 0.5, 'max', 1, 2, reference=True)
        _same_records(got, ref, int(ref.total))
        assert int(ref.total) != int(hard.total)
        totals.append(int(ref.total))
    assert totals[0] != totals[1] and min(totals) > 0


def test_meter_on_a_post_soft_nms_batch():
    """SegmentAPMeter.add of propose(soft=)'s result against ap_reference over the reference's proposals: tp, match and the stores bit-equal,
    ap within 1 fp32 ulp (the criterion of test_hip_proposals.py and test_hip_segap.py)"""
    from test_hip_segap import _meter_checked
    from cfn_hip.detections import SoftNMS, decode_reference, propose
    B, C, TL = 3, 6, 160
    probs = random_probs(41, B, C, TL)
    valid, fps, start = _meta(B, TL)
    g = decode_reference(probs, valid, fps, start, 0.4)
    gt = fx.make_gt([[(int(c), s + 1.0 / 24.0, e) for c, s, e in g.seg[int(g.offsets[b]):int(g.offsets[b + 1])].tolist()] for b in range(B)],
                    fps.tolist(), [[int(s), int(v)] for s, v in zip(start, valid)], C, TL)
    tiou = (0.3, 0.5, 0.7, 0.9)
    hard = propose(probs, valid, fps, start, LEVELS5, 0.6, reference=True).check()
    for soft in (SoftNMS('gaussian', 0.5, 0.05, 0), SoftNMS('linear', 0.5, 0.05, 0)):
        det = propose(probs, valid, fps, start, LEVELS5, 0.6, reference=True, soft=soft)
        dev = propose(probs.to(DEV), valid.to(DEV), fps.to(DEV), start.to(DEV), LEVELS5, 0.6, soft=soft)
        n = det.check()
        assert dev.check() == n > 20 and n != hard and all(torch.equal(_bits(a[:n].cpu()), _bits(b[:n])) for a, b in zip(dev[:3], det[:3]))
        per_class = int(torch.bincount(det.seg[:n, 0].long(), minlength=C).max())
        fixed, ref, (ap, mp) = _meter_checked([(det, gt)], C, tiou, capacity=per_class + 3)
        assert 0.0 < float(mp[0]) and len(set(ref['batches'][0][0].tolist())) > 2


def test_train_fine_with_soft_nms_in_the_writer_and_the_meter(tmp_path, monkeypatch):
    """run() with a writer AND a meter that take soft=: the file holds propose(soft=) of the validation probs, the meter is handed that very
    batch and agrees with ap_reference over it.  The same run without any of the options gives the same losses and the same existing log
    line, bit for bit"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from test_hip_detections import _SegVideos, _run, _same_file
    from test_hip_segap import _line, _spy_meter, _ulps
    from cfn_hip.detections import DetectionWriter, SoftNMS, epoch_path, propose
    from cfn_hip.seglabels import collate_seg
    from cfn_hip.segap import ap_reference
    crop, tiou, levels, soft = 64, (0.1, 0.5), (0.6, 0.5, 0.4), SoftNMS('gaussian', 0.5, 0.01, 0)
    mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                      collate_fn=collate.fine_collate_u8)
    writer = DetectionWriter(str(tmp_path / 'det.jsonl'), 0.9, 2, 2, levels=levels, nms=0.5, soft=soft)
    meter = _spy_meter(tiou, thr=0.9, max_gap=0, min_len=7, levels=(0.9,), soft=SoftNMS('linear'))
    fed = []
    real_add = meter.add
    monkeypatch.setattr(meter, 'add', lambda det, labels, **kw: (fed.append((det, kw)), real_add(det, labels, **kw))[1])
    kept = []
    real_wadd = writer.add
    monkeypatch.setattr(writer, 'add', lambda *a, **k: (lambda d: (kept.append(d), d)[1])(real_wadd(*a, **k)))
    losses, lines, val = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, writer, max_epochs=4, save_model=str(tmp_path / 'm_'),
                              segment_ap=meter)
    assert len(fed) == len(kept) == 3 and all(f[0] is k and f[1] == {'levels': 3} for f, k in zip(fed, kept))
    rows, batches, hard = [], [], 0
    for i, (probs, valid) in enumerate(val):
        lab = collate_seg([_SegVideos(3, crop, False)[i][1]])
        det = propose(probs, valid, lab.fps, lab.window[:, 0].contiguous(), levels, 0.5, 'max', 2, 2, reference=True, soft=soft)
        hard += propose(probs, valid, lab.fps, lab.window[:, 0].contiguous(), levels, 0.5, 'max', 2, 2, reference=True).check()
        rows.append({'video': 'vid%d' % i, 'unit': 's', 'segments': det.tolist()[0]})
        batches.append((det, lab))
    n = _same_file(epoch_path(writer.path, 4), rows)
    print('train_fine: %d soft-NMS proposals in 3 validation videos (hard NMS: %d)' % (n, hard))
    assert n > 0
    ref = ap_reference(batches, 157, tiou)
    ap, mp = meter.last
    assert _ulps(ap.numpy(), ref['ap']).max() <= 1 and _ulps(mp.numpy(), ref['map']).max() <= 1
    assert len(lines) == 2 and lines[1] == _line(4, tiou, mp)
    losses0, lines0, _ = _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / 'n_'))
    assert losses0 == losses and lines0 == lines[:1]
