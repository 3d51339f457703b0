"""GPU: proposal recall at N per video, AR@N (csrc/segrecall.hip, cfn_hip/recall.py).

Against the numpy reference of cfn_hip/recall.py (checked by hand in test_recall_cpu.py) the device result is BIT-EQUAL in hit, state, recall,
ar and auc: a tIoU is fp64 subtractions, additions and ONE correctly rounded division, the ranks and the state are integers, and the value is
int64 sums, correctly rounded divisions and fp64 additions in a stated order, without a product that could contract.  hit is handed over
filled with a canary: the kernel writes every entry.

The kernels' boundaries: the rank kernel walks a video's scores through LDS tiles of ops.SEG_RECALL_RANK_TILE rows, one workgroup per tile of
rows; the first-hit kernel strides 64 lanes over the candidates of a (video, class) group."""
import os

import numpy as np
import pytest
import torch

import segap_fixture as fx
from test_recall_cpu import HAND_HIT, HAND_N, HAND_TIOU, _clipped_rows_as_detections, hand_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = -7


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def _meter(C, tiou, n_max, score='max'):
    from cfn_hip.recall import ProposalRecallMeter
    return ProposalRecallMeter(DEV, C, tiou, n_max, score)


def _add_checked(meter, det, gt, want_hit):
    """add() over a canary-filled hit table against the reference's"""
    from cfn_hip import ops
    d = det.to(DEV)
    g = gt.to(DEV) if hasattr(gt, 'to') else gt
    S = int(want_hit.shape[1])
    out = (torch.full((len(meter.tiou), S), CANARY, dtype=torch.int32, device=DEV),
           torch.empty(ops.seg_recall_workspace_bytes(d.batch, d.n_classes, d.cap, S, len(meter.tiou)), dtype=torch.uint8, device=DEV))
    hit = meter.add(d, g, out=out)
    assert hit is out[0]
    hit = hit.cpu().numpy()
    assert (hit == want_hit).all(), 'hit differs at %s' % (np.argwhere(hit != want_hit)[:8].tolist(),)


def _value_checked(meter, ref):
    """state, recall, ar, auc and avg_props bit-equal to the reference's dict; two calls give the same bits"""
    assert meter.state.cpu().numpy().tolist() == ref['state'].tolist(), 'state differs'
    v, v2, dv = meter.value(), meter.value(), meter.value_device()
    for k in ('recall', 'ar', 'auc', 'avg_props'):
        assert (_bits(v[k]) == _bits(ref[k])).all(), k
        assert (_bits(v[k]) == _bits(v2[k])).all() and (_bits(dv[k].cpu().numpy()) == _bits(v[k])).all(), k
    assert v['recall'].shape == ref['recall'].shape and v['ar'].shape == ref['ar'].shape and v['n_gt'] == ref['n_gt']
    return v


def _meter_checked(batches, C, tiou, n_max, score='max'):
    from cfn_hip.detections import SCORE_COLUMNS
    from cfn_hip.recall import recall_reference
    ref = recall_reference(batches, C, tiou, n_max, SCORE_COLUMNS[score])
    meter = _meter(C, tiou, n_max, score)
    for (det, gt), hit in zip(batches, ref['hits']):
        _add_checked(meter, det, gt, hit)
    return meter, ref, _value_checked(meter, ref)


def test_the_hand_batch():
    det, gt = hand_batch()
    meter, ref, v = _meter_checked([(det, gt)], 3, HAND_TIOU, HAND_N)
    assert ref['hits'][0].tolist() == HAND_HIT and v['n_gt'] == 7 and v['avg_props'] == 4.0
    assert v['recall'][0, 3] == np.float64(5) / np.float64(7)
    _meter_checked([(det, gt)], 3, HAND_TIOU, HAND_N, 'mean')
    meter.reset()
    assert not meter.state.any()


TIOU16 = tuple(np.linspace(0.2, 0.95, 16).tolist())


@pytest.mark.parametrize('B,C,n_thr,n_max,score', [(1, 1, 1, 1, 'max'), (3, 5, 10, 7, 'max'), (3, 5, 16, 1024, 'mean'), (8, 157, 16, 100, 'max'),
                                                   (8, 157, 10, 7, 'mean'), (1, 1, 16, 100, 'max')])
def test_random_batches(B, C, n_thr, n_max, score):
    """n_b up to 40 candidates per video: n_max 1 and 7 lie below, 100 and 1024 above.  The last batch's detections are its own clipped
    ground-truth rows, so that every threshold has hits with 157 classes too"""
    from cfn_hip.recall import DEFAULT_TIOU
    tiou = {1: (0.5,), 10: DEFAULT_TIOU, 16: TIOU16}[n_thr]
    batches = [fx.random_batch(400 + 10 * B + i, B, C, 40, 20) for i in range(3)]
    gt = fx.random_batch(450 + B, B, C, 0, 20)[1]
    batches.append((_clipped_rows_as_detections(gt, B, C, 7)[0], gt))
    meter, ref, v = _meter_checked(batches, C, tiou, n_max, score)
    assert ref['n_gt'] > 0 and ref['n_props'] > 0
    assert ref['state'][:-3].sum() > 0


def _rand_rows(rng, C, nd, ng, ties=4):
    """one video: nd distinct detections and ng ground-truth rows on a half-second grid (as wide as the detections need, at most 200 s), scores
    on a grid of `ties` values"""
    span = max(60, 2 * nd // C + 20)
    dets, seen = [], set()
    while len(dets) < nd:
        c, s = int(rng.randint(0, C)), 0.5 * rng.randint(0, span)
        if (c, s) not in seen:
            seen.add((c, s))
            dets.append((c, s, s + 0.5 * rng.randint(1, 8), float(rng.randint(0, ties)) / ties, float(rng.randint(0, ties)) / ties))
    gts = []
    for _ in range(ng):
        s = 0.5 * rng.randint(0, span)
        gts.append((int(rng.randint(0, C)), s, s + 0.5 * rng.randint(1, 8)))
    return dets, gts


def _videos(seed, C, sizes, ties=4):
    """sizes: (nd, ng) per video -> (Detections, SegLabels) on the host; fps 1, window [0, 250)"""
    rng = np.random.RandomState(seed)
    rows = [_rand_rows(rng, C, nd, ng, ties) for nd, ng in sizes]
    B = len(sizes)
    return fx.make_det([r[0] for r in rows], C), fx.make_gt([r[1] for r in rows], [1.0] * B, [[0, 250]] * B, C, t_max=250)


def test_a_video_without_candidates_one_without_ground_truth_and_an_overflowed_decode():
    from cfn_hip.detections import Detections
    det, gt = _videos(1, 4, [(0, 9), (25, 0), (30, 12), (0, 0), (20, 15)])
    assert det.offsets.tolist() == [0, 0, 25, 55, 55, 75]
    _, ref, _ = _meter_checked([(det, gt)], 4, (0.3, 0.5, 0.7), 10)
    assert ref['n_props'] == 75 and ref['n_videos'] == 5 and (ref['hits'][0][:, :9] == 10).all()
    # offsets[B] above cap, as an overflowed decode leaves it: the rows beyond cap are ignored (the last video loses 15 of its 20)
    cut = Detections(det.seg[:60].contiguous(), det.frames[:60].contiguous(), det.score[:60].contiguous(), det.offsets, det.total, 4, 60)
    _, ref_cut, _ = _meter_checked([(cut, gt)], 4, (0.3, 0.5, 0.7), 10)
    assert ref_cut['n_props'] == 60 and ref_cut['state'][:-3].sum() < ref['state'][:-3].sum()
    # no ground truth at all (the labels' one placeholder row) and no detection at all
    none_det, none_gt = _videos(2, 4, [(0, 0), (0, 0)])
    _, ref0, v0 = _meter_checked([(none_det, none_gt)], 4, (0.5,), 10)
    assert ref0['n_gt'] == 0 and not v0['recall'].any() and v0['avg_props'] == 0.0


@pytest.mark.parametrize('nd', [63, 64, 65])
def test_candidates_of_one_group_around_the_wave(nd):
    """one video, one class: the 64 lanes of a ground-truth row's wave stride over nd candidates"""
    det, gt = _videos(10 + nd, 1, [(nd, 30)], ties=8)
    _, ref, _ = _meter_checked([(det, gt)], 1, (0.1, 0.5, 0.9), 80)
    assert ref['n_props'] == nd and ref['state'][:-3].sum() > 10


def test_candidates_per_video_around_the_rank_kernels_tile():
    """n_b = tile - 1, tile, tile + 1 and 2 * tile + 3 in one batch, scores on a grid of 3 values: most ties cross a tile, and the row
    tie-break has to order them"""
    from cfn_hip import ops
    from cfn_hip.recall import video_rank_reference
    T = ops.SEG_RECALL_RANK_TILE
    det, gt = _videos(20, 3, [(T - 1, 12), (T, 12), (T + 1, 12), (2 * T + 3, 12)], ties=3)
    assert np.diff(det.offsets.numpy()).tolist() == [T - 1, T, T + 1, 2 * T + 3]
    rank = video_rank_reference(det)
    assert rank.max() == 2 * T + 2
    _, ref, _ = _meter_checked([(det, gt)], 3, (0.3, 0.6), 1024)
    hits = ref['hits'][0]
    assert (hits[(hits >= 0) & (hits < 1024)] > T).any()                                # ranks from behind the first tile are used


@pytest.mark.parametrize('value', [0.5, float('nan')])
def test_all_scores_equal_or_all_nan(value):
    """the video rank is then the row's index in its video"""
    det, gt = _videos(30, 3, [(70, 15), (40, 15)])
    det.score.fill_(value)
    _, ref, _ = _meter_checked([(det, gt)], 3, (0.25, 0.5), 64)
    hits = ref['hits'][0]
    assert (hits == 64).any() and ((hits >= 0) & (hits < 64)).any()


def _graded(dense, seed):
    """label arrays -> probabilities in blocks of 8 frames: 0 outside the labels, 0.25 .. 0.95 inside, so three levels cut different candidates"""
    rng = np.random.RandomState(seed)
    B, C, T = dense.shape
    noise = np.repeat(rng.rand(B, C, (T + 7) // 8).astype(np.float32), 8, axis=2)[:, :, :T]
    return (dense * torch.from_numpy(np.float32(0.25) + np.float32(0.7) * noise)).contiguous()


@pytest.mark.parametrize('split', ['full', 'training', 'testing'])
def test_golden_records_through_propose_and_the_meter(split):
    """the 42 annotation records in their three windows (126 label arrays): dense -> propose at three levels -> meter on the device is
    bit-equal to decode_levels_reference -> nms_reference -> recall_reference on the host.  And the labels themselves decoded at 0.5 against
    the dense pair recall everything at every threshold from N = the candidates of the fullest video on (the host reference says from which N:
    full 28, training 26, testing 28)."""
    from cfn_hip.detections import decode, decode_reference, propose
    from cfn_hip.recall import DEFAULT_TIOU, recall_reference
    lab = fx.golden_labels(split)
    dense, _, valid = lab.dense_reference()
    probs = _graded(dense, 3)
    start = lab.window[:, 0].contiguous()
    levels = (0.8, 0.5, 0.2)
    want = propose(probs, valid, lab.fps, start, levels, 0.5, reference=True)
    ref = recall_reference([(want, lab)], 157, DEFAULT_TIOU, 100)
    dlab = lab.to(DEV)
    det = propose(probs.to(DEV), valid.to(DEV), dlab.fps, dlab.window[:, 0].contiguous(), levels, 0.5)
    n = want.check()
    assert int(det.total.item()) == n and torch.equal(det.seg[:n].cpu().view(torch.int64), want.seg[:n].view(torch.int64))
    meter = _meter(157, DEFAULT_TIOU, 100)
    _add_checked(meter, det, dlab, ref['hits'][0])
    v = _value_checked(meter, ref)
    assert ref['n_gt'] > 50 and 0.0 <= v['ar'][0] < v['ar'][-1] <= 1.0
    # the labels themselves
    own = decode_reference(dense, valid, thr=0.5)
    g = decode_reference(dense, valid, thr=0.5)
    B = int(dense.shape[0])
    gt = (g.seg, g.offsets, torch.ones(B, dtype=torch.float64), torch.stack([torch.zeros_like(valid), valid], 1), int(dense.shape[2]))
    ref_own = recall_reference([(own,) + gt], 157, DEFAULT_TIOU, 100)
    first = int(np.flatnonzero((ref_own['recall'] == 1.0).all(0))[0]) + 1
    assert first == {'full': 28, 'training': 26, 'testing': 28}[split] == int(np.diff(own.offsets.numpy()).max())
    meter.reset()
    meter.add(decode(dense.to(DEV), valid.to(DEV), thr=0.5), (dense.to(DEV), valid.to(DEV)))
    v = _value_checked(meter, ref_own)
    assert (v['recall'][:, first - 1:] == 1.0).all() and (v['ar'][first - 1:] == 1.0).all() and not (v['recall'][:, first - 2] == 1.0).any()
    print('%s windows: %d proposals, %d rows participate, AR@1 %.4f AR@100 %.4f; own decode: recall 1 from N = %d' % (
        split, n, ref['n_gt'], ref['ar'][0], ref['ar'][-1], first))


def test_two_meters_merged_equal_one_and_a_process_group_of_one_changes_nothing():
    import torch.distributed as dist
    from cfn_hip.recall import recall_reference
    batches = [fx.random_batch(500 + i, 3, 5, 40, 20) for i in range(4)]
    one, a, b = (_meter(5, (0.5, 0.75), 50) for _ in range(3))
    for i, (det, gt) in enumerate(batches):
        one.add(det.to(DEV), gt.to(DEV))
        (a if i < 2 else b).add(det.to(DEV), gt.to(DEV))
    assert not torch.equal(a.state, one.state)
    a.merge(b)
    assert torch.equal(a.state, one.state)
    ref = recall_reference(batches, 5, (0.5, 0.75), 50)
    v = _value_checked(one, ref)
    with pytest.raises(ValueError, match='same tiou, n_max, score'):
        a.merge(_meter(5, (0.5, 0.75), 51))
    created = False
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29534')
        dist.init_process_group('nccl', rank=0, world_size=1)
        created = True
    try:
        total = one.all_reduce()
        assert total is not one.state and torch.equal(total, one.state)               # a copy, summed over one rank
        vg = one.value(group=dist.group.WORLD)
        for k in ('recall', 'ar', 'auc', 'avg_props'):
            assert (_bits(vg[k]) == _bits(v[k])).all(), k
        assert vg['n_gt'] == v['n_gt'] and torch.equal(one.state.cpu(), torch.from_numpy(ref['state']))
    finally:
        if created:
            dist.destroy_process_group()


def test_add_with_out_buffers_is_capturable():
    """out=: add() allocates nothing and waits for nothing, so a graph holds it.  Three different batches are copied into static inputs and
    the graph is replayed for each: the state equals the eager meter's; the whole run twice gives identical bits"""
    from cfn_hip import ops
    from cfn_hip.detections import Detections
    from cfn_hip.seglabels import SegLabels
    C, tiou, n_max, cap, S = 4, (0.3, 0.5, 0.7), 30, 160, 64
    batches = [fx.random_batch(600 + i, 3, C, 40, 20) for i in range(3)]
    eager = _meter(C, tiou, n_max)
    for det, gt in batches:
        eager.add(det.to(DEV), gt.to(DEV))
    sdet = Detections(torch.zeros(cap, 3, dtype=torch.float64, device=DEV), torch.zeros(cap, 3, dtype=torch.int32, device=DEV),
                      torch.zeros(cap, 2, dtype=torch.float32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV),
                      torch.zeros(1, dtype=torch.int32, device=DEV), C, cap)
    sgt = SegLabels(torch.zeros(S, 3, dtype=torch.float64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV),
                    torch.ones(3, dtype=torch.float64, device=DEV), torch.zeros(3, 2, dtype=torch.int32, device=DEV), C, 200)
    out = (torch.empty(len(tiou), S, dtype=torch.int32, device=DEV),
           torch.empty(ops.seg_recall_workspace_bytes(3, C, cap, S, len(tiou)), dtype=torch.uint8, device=DEV))

    def run():
        graphed = _meter(C, tiou, n_max)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.add(sdet, sgt, out=out)
        graphed.reset()                                                                # (whatever the capture's warm-up may have run)
        for det, gt in batches:
            n, s = int(det.seg.shape[0]), int(gt.seg.shape[0])
            assert n <= cap and s <= S and gt.t_max == 200
            sdet.seg[:n].copy_(det.seg)
            sdet.score[:n].copy_(det.score)
            sdet.offsets.copy_(det.offsets)
            sgt.seg.fill_(-1.0)                                                        # (rows behind the batch's: no class, and no video covers them)
            sgt.seg[:s].copy_(gt.seg)
            sgt.offsets.copy_(gt.offsets)
            sgt.fps.copy_(gt.fps)
            sgt.window.copy_(gt.window)
            g.replay()
        torch.cuda.synchronize()
        return graphed.state.clone(), graphed.value()
    s1, v1 = run()
    s2, v2 = run()
    assert torch.equal(s1, eager.state) and torch.equal(s2, s1) and int(s1[:-3].sum()) > 0
    ve = eager.value()
    for k in ('recall', 'ar', 'auc', 'avg_props'):
        assert (_bits(v1[k]) == _bits(ve[k])).all() and (_bits(v2[k]) == _bits(v1[k])).all(), k


class _Spy(object):
    """mixed into ProposalRecallMeter: keeps the Detections and labels add() was given and what value() gave run() before the reset"""

    def add(self, det, labels, out=None):
        self.fed.append((det.to('cpu'), labels.to('cpu')))
        return super().add(det, labels, out)

    def value(self, group=None):
        self.last = (self.state.cpu().numpy().copy(), super().value(group))
        return self.last[1]


def test_train_fine_feeds_the_meter_from_its_validation_phase(tmp_path, monkeypatch):
    """run(..., segment_ap=, proposal_recall=) on the tiny SegLabel loader of test_hip_segap.py's
    test_train_fine_feeds_the_meter_from_its_validation_phase: the recall meter is fed the segment-AP meter's proposals (no second decode: the
    spied Detections are what propose gives for the spied validation probs), its state at the end of the phase equals recall_reference over
    them, its line is logged behind the others, and the losses and the other lines are bit-equal to a run without it"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from cfn_hip.detections import propose
    from cfn_hip.recall import ProposalRecallMeter, recall_reference
    from cfn_hip.seglabels import collate_seg
    from cfn_hip.segap import SegmentAPMeter
    from test_hip_detections import _SegVideos, _run
    crop, tiou, levels = 64, (0.3, 0.5), (0.6, 0.5, 0.4)

    def go(tag, recall):
        mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                          collate_fn=collate.fine_collate_u8)
        ap = SegmentAPMeter(DEV, 157, (0.1, 0.5), max_gap=2, min_len=2, levels=levels, nms=0.6)
        return _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / (tag + '_')),
                    segment_ap=ap, proposal_recall=recall)
    meter = type('SpyRecall', (_Spy, ProposalRecallMeter), {})(DEV, 157, tiou, 20)
    meter.fed = []
    losses, lines, val = go('rec', meter)
    assert len(lines) == 3 and 'mAP' in lines[0] and ' seg-mAP@0.1: ' in lines[1]
    state, v = meter.last
    assert lines[2] == ' Epoch:4 val AR@1: %.4f AR@10: %.4f AR@20: %.4f AUC: %.4f props/video: %.1f' % (
        v['ar'][0], v['ar'][9], v['ar'][19], v['auc'], v['avg_props'])
    assert len(val) == 3 and len(meter.fed) == 3 and not meter.state.any()               # empty again for the next phase
    datasets = _SegVideos(3, crop, False)
    batches = []
    for i, ((probs, valid), (det, lab)) in enumerate(zip(val, meter.fed)):
        want_lab = collate_seg([datasets[i][1]])
        want = propose(probs, valid, want_lab.fps, want_lab.window[:, 0].contiguous(), levels, 0.6, max_gap=2, min_len=2, reference=True)
        n = want.check()
        assert int(det.total) == n and torch.equal(det.seg[:n].view(torch.int64), want.seg[:n].view(torch.int64))
        assert torch.equal(lab.seg, want_lab.seg)
        batches.append((want, want_lab))
    ref = recall_reference(batches, 157, tiou, 20)
    assert ref['n_props'] > 0 and ref['n_gt'] > 0 and state.tolist() == ref['state'].tolist()
    for k in ('recall', 'ar', 'auc', 'avg_props'):
        assert (_bits(v[k]) == _bits(ref[k])).all(), k
    losses0, lines0, _ = go('none', None)
    assert losses0 == losses and lines0 == lines[:2]
    with pytest.raises(RuntimeError, match='a decode'):
        train_fine.run(dataloaders={}, proposal_recall=meter)
