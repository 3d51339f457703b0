"""Proposal recall at N per video (AR@N), on the host: the rules of cfn_hip/recall.py as video_rank_reference / first_hit_reference /
recall_from_state / recall_reference spell them (a hand batch worked out in the docstring, the threshold edge, identities, the cross-check
against segment AP's matching, additivity), merging and reducing states, the C ABI of the cfn_seg_recall_* entry points and the refusals.
No GPU; every comparison is exact."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

import segap_fixture as fx
from conftest import PKG

HAND_TIOU, HAND_N = (0.5, 0.9), 4
NAN = float('nan')


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def hand_batch():
    """B = 2, C = 3, tiou (0.5, 0.9), n_max 4.

    video 0 (fps 1, window [0, 100): w0 = -0.5, w1 = 99.5).  Detections in row order (class, start), max score -> video rank:
      row 0 (0:  0, 10) 0.9 -> 0      row 1 (0: 20, 30) 0.5 -> 2 (a tie ACROSS classes with row 4: the lower row)      row 2 (0: 40, 50) NaN -> 4 (as -inf)
      row 3 (1:  0, 10) 0.8 -> 1      row 4 (1: 20, 32) 0.5 -> 3
      (class 1's rows have in-class ranks 0 and 1 but video ranks 1 and 3: the two classes' scores interleave)
    ground truth:
      g0 (0: 0, 10)      row 0 at tIoU 1: rank 0 at both thresholds
      g1 (1: 20, 30)     row 4 at 10 / 12: rank 3 at 0.5, nothing at 0.9 -> 4
      g2 (0: 40, 50)     row 2 at tIoU 1, rank 4 >= n_max -> 4 at both
      g3 (0: 200, 300)   outside the window -> -1
      g4 (1.5: 0, 10)    a fractional class -> -1
      g5 (1: NaN, 10)    the NaN start gives way to w0: (-0.5, 10); row 3 at 10 / 10.5 = 0.952: rank 1 at both
    video 1 (fps 2, window [10, 50): w0 = 4.75, w1 = 29.75):
      row 5 (0: 25, 29.75) 0.7 -> 0 (a tie across classes with row 7: the lower row)      row 6 (2: 5, 10) 0.3 -> 2      row 7 (2: 6, 10) 0.7 -> 1
      g6 (2: 5, 10)      row 7 at 4 / 5 (rank 1) and row 6 at 1 (rank 2): 1 at 0.5, 2 at 0.9
      g7 (0: 25, 40)     clipped to (25, 29.75): row 5 at 1: rank 0 at both
      g8 (1: 12, 20)     class 1 has candidates in video 0 only -> 4 at both
    mean scores rank the rows of a video in reverse row order."""
    det = fx.make_det([
        [(0, 0, 10, 0.9, 0.1), (0, 20, 30, 0.5, 0.2), (0, 40, 50, NAN, 0.3), (1, 0, 10, 0.8, 0.4), (1, 20, 32, 0.5, 0.5)],
        [(0, 25, 29.75, 0.7, 0.1), (2, 5, 10, 0.3, 0.2), (2, 6, 10, 0.7, 0.3)],
    ], 3)
    gt = fx.make_gt([
        [(0, 0, 10), (1, 20, 30), (0, 40, 50), (0, 200, 300), (1.5, 0, 10), (1, NAN, 10)],
        [(2, 5, 10), (0, 25, 40), (1, 12, 20)],
    ], [1.0, 2.0], [[0, 100], [10, 50]], 3, t_max=100)
    return det, gt


HAND_RANK = [0, 2, 4, 1, 3, 0, 2, 1]
HAND_HIT = [[0, 3, 4, -1, -1, 1, 1, 0, 4],
            [0, 4, 4, -1, -1, 1, 2, 0, 4]]
HAND_HIST = [[2, 2, 0, 1],
             [2, 1, 1, 0]]
HAND_TAIL = [7, 2, 8]                                                                  # n_gt, n_videos, n_props


def test_the_hand_batch():
    from cfn_hip.recall import first_hit_reference, recall_reference, video_rank_reference
    det, gt = hand_batch()
    assert video_rank_reference(det).tolist() == HAND_RANK
    assert video_rank_reference(det, 1).tolist() == [4, 3, 2, 1, 0, 2, 1, 0]
    hit, part, n_props = first_hit_reference(det, gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, HAND_TIOU, HAND_N)
    assert hit.dtype == np.int32 and hit.tolist() == HAND_HIT and n_props == 8
    assert part.tolist() == [True, True, True, False, False, True, True, True, True]
    r = recall_reference([(det, gt)], 3, HAND_TIOU, HAND_N)
    assert r['state'].dtype == np.int64 and r['state'].tolist() == HAND_HIST[0] + HAND_HIST[1] + HAND_TAIL
    seven = np.float64(7)
    want = np.array([[2 / seven, 4 / seven, 4 / seven, 5 / seven], [2 / seven, 3 / seven, 4 / seven, 4 / seven]])
    assert r['recall'].dtype == np.float64 and (r['recall'] == want).all()
    ar = (want[0] + want[1]) / np.float64(2)
    assert (r['ar'] == ar).all() and r['auc'] == (((ar[0] + ar[1]) + ar[2]) + ar[3]) / np.float64(4)
    assert r['avg_props'] == 4.0 and r['n_gt'] == 7 and r['n_videos'] == 2 and r['n_props'] == 8
    # a larger n_max shows the NaN-scored candidate at its rank 4
    assert recall_reference([(det, gt)], 3, HAND_TIOU, 5)['hits'][0][:, 2].tolist() == [4, 4]


def test_a_tiou_exactly_on_the_threshold_hits_and_the_next_double_misses():
    from cfn_hip.recall import recall_reference
    det, gt = fx.make_det([[(0, 0, 2, 0.5, 0.5)]], 1), fx.make_gt([[(0, 1, 3)]], [1.0], [[0, 100]], 1)
    third = np.float64(1) / 3
    assert recall_reference([(det, gt)], 1, [third], 3)['hits'][0].tolist() == [[0]]
    assert recall_reference([(det, gt)], 1, [np.nextafter(third, 1.0)], 3)['hits'][0].tolist() == [[3]]


def _clipped_rows_as_detections(gt, B, C, seed):
    from cfn_hip.segap import clip_reference
    part, sp, ep, vid = clip_reference(gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, C)
    rng = np.random.RandomState(seed)
    rows = [[] for _ in range(B)]
    for g in np.flatnonzero(part):
        rows[vid[g]].append((int(gt.seg[g, 0]), sp[g], ep[g], float(rng.randint(0, 4)) / 4.0, float(rng.rand())))
    return fx.make_det(rows, C), part, vid


def test_detections_equal_to_the_ground_truth_recall_everything_from_the_fullest_video_on():
    from cfn_hip.recall import recall_reference
    B, C = 6, 7
    _, gt = fx.random_batch(5, B, C, 0, 12, half=False)
    det, part, vid = _clipped_rows_as_detections(gt, B, C, 1)
    fullest = int(np.diff(det.offsets.numpy()).max())
    assert part.sum() >= 20 and fullest >= 5
    r = recall_reference([(det, gt)], C, (0.1, 0.5, 0.9, 1.0), 20)
    assert (r['recall'][:, fullest - 1:] == 1.0).all() and (r['ar'][fullest - 1:] == 1.0).all()
    assert (r['recall'][:, 0] < 1.0).all()


def test_recall_grows_with_n_and_falls_with_the_threshold():
    from cfn_hip.recall import recall_reference
    tiou = (0.9, 0.3, 0.5, 0.7)                                                        # any order
    batches = [fx.random_batch(100 + i, 4, 3, 30, 20) for i in range(4)]
    r = recall_reference(batches, 3, tiou, 25)
    assert r['n_gt'] > 40 and 0.0 < r['recall'][1, -1] <= 1.0
    assert (np.diff(r['recall'], axis=1) >= 0).all()
    order = np.argsort(tiou)
    assert (np.diff(r['recall'][order], axis=0) <= 0).all() and (r['recall'][1] > r['recall'][0]).any()
    assert 0.0 <= r['auc'] <= r['ar'][-1] <= 1.0


def _pairs(det, gt, C, t):
    """per (video, class) group: the boolean table [detection, participating row] of tIoU > 0 and >= t"""
    from cfn_hip.segap import clip_reference, tiou_reference
    part, sp, ep, vid = clip_reference(gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, C)
    dseg, doff, gcls = det.seg.numpy(), det.offsets.numpy(), gt.seg.numpy()[:, 0]
    out = []
    for b in range(len(doff) - 1):
        for c in range(C):
            ds = [d for d in range(doff[b], doff[b + 1]) if dseg[d, 0] == c]
            gs = [g for g in np.flatnonzero(part & (vid == b)) if gcls[g] == c]
            tab = np.zeros((len(ds), len(gs)), bool)
            for i, d in enumerate(ds):
                for j, g in enumerate(gs):
                    v = tiou_reference(dseg[d, 1], dseg[d, 2], sp[g], ep[g])
                    tab[i, j] = v > 0.0 and v >= t
            out.append((ds, gs, tab))
    return out


def test_recalled_rows_against_the_true_positives_of_segment_ap():
    """with n_max >= every n_b a row is recalled at k iff some detection of its group reaches tiou[k] with it.  A true positive of segment AP
    uses up one such row for itself, so the rows recalled are at least the true positives.  They are equal in every group where no row is
    reached by two detections and no detection reaches two rows: the pairs are then a one-to-one relation, and the greedy matching of rule 4
    of segment AP takes exactly them.  (Distinct best rows alone do not suffice: one detection that reaches two rows recalls both and matches
    one.)"""
    from cfn_hip.recall import recall_reference
    from cfn_hip.segap import match_reference
    tiou = (0.3, 0.5, 0.7)
    C = 3
    equal_groups = strict_groups = 0
    for seed in range(200):
        det, gt = fx.random_batch(seed, 2, C, 12, 12)
        n_b = int(np.diff(det.offsets.numpy()).max()) if det.offsets[-1] else 0
        hit = recall_reference([(det, gt)], C, tiou, max(n_b, 1))['hits'][0]
        tp, match, _ = match_reference(det, gt.seg, gt.offsets, gt.fps, gt.window, gt.t_max, tiou)
        for k, t in enumerate(tiou):
            recalled = (hit[k] >= 0) & (hit[k] < max(n_b, 1))
            assert recalled.sum() >= ((tp >> k) & 1).sum()
            for ds, gs, tab in _pairs(det, gt, C, np.float64(t)):
                n_rec, n_tp = int(recalled[gs].sum()) if gs else 0, int(((tp[ds] >> k) & 1).sum()) if ds else 0
                assert n_rec == int(tab.any(0).sum()) and n_rec >= n_tp
                if tab.any() and (tab.sum(0) <= 1).all() and (tab.sum(1) <= 1).all():
                    assert n_rec == n_tp
                    equal_groups += 1
                strict_groups += n_rec > n_tp
    assert equal_groups > 100 and strict_groups > 10                                   # both cases occur


def test_the_state_is_additive():
    from cfn_hip.recall import recall_reference
    a = [fx.random_batch(300 + i, 3, 5, 40, 20) for i in range(2)]
    b = [fx.random_batch(310 + i, 2, 5, 40, 20) for i in range(3)]
    sa, sb, sab = (recall_reference(x, 5, n_max=17)['state'] for x in (a, b, a + b))
    assert sa[-3] > 0 and sb[-3] > 0 and (sab == sa + sb).all()


def _host_meter(tiou=(0.5, 0.9), n_max=4, score='max', n_classes=3, fill=0):
    """a ProposalRecallMeter whose state is a CPU tensor: the constructor refuses a CPU device, merging and reducing need none"""
    from cfn_hip.detections import SCORE_COLUMNS
    from cfn_hip.recall import ProposalRecallMeter, state_size
    m = ProposalRecallMeter.__new__(ProposalRecallMeter)
    m.device, m.tiou, m.n_max, m.score, m.score_col, m.n_classes = torch.device('cpu'), tuple(tiou), n_max, score, SCORE_COLUMNS[score], n_classes
    m.state = torch.full((state_size(len(tiou), n_max),), fill, dtype=torch.int64)
    return m


def test_merge_adds_states_and_refuses_unequal_settings():
    a, b = _host_meter(fill=2), _host_meter(fill=3)
    assert a.merge(b) is a and (a.state == 5).all() and (b.state == 3).all()
    for other in (_host_meter(tiou=(0.5, 0.8)), _host_meter(n_max=5), _host_meter(score='mean'), _host_meter(n_classes=4), object()):
        with pytest.raises(ValueError, match='same tiou, n_max, score'):
            a.merge(other)
    assert (a.state == 5).all()


def test_all_reduce_without_a_process_group_does_nothing():
    import torch.distributed as dist
    from cfn_hip.recall import all_reduce_state
    assert not dist.is_initialized()
    m = _host_meter(fill=7)
    assert m.all_reduce() is m.state and all_reduce_state(m.state) is m.state and (m.state == 7).all()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, port, out):
    import torch.distributed as dist
    sys.path.insert(0, PKG)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK=str(rank))
    torch.cuda.is_available = lambda: False
    from cfn_hip.recall import all_reduce_state
    dist.init_process_group('gloo', rank=rank, world_size=2)
    state = torch.arange(11, dtype=torch.int64) * (rank + 1) + (1 << 40) * rank      # (past 2^32: the sum is an int64 sum)
    total = all_reduce_state(state)
    out[rank] = (state.clone(), total, total is state)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_sums_the_states_of_two_gloo_ranks_in_a_copy():
    import torch.multiprocessing as mp
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_reduce_worker, args=(port, out), nprocs=2, join=True)
    want = torch.arange(11, dtype=torch.int64) * 3 + (1 << 40)
    for rank in range(2):
        state, total, same = out[rank]
        assert not same and torch.equal(total, want)
        assert torch.equal(state, torch.arange(11, dtype=torch.int64) * (rank + 1) + (1 << 40) * rank)      # the rank's own state is untouched


def test_recall_from_state_without_ground_truth_or_videos_is_zero():
    from cfn_hip.recall import recall_from_state, state_size
    r = recall_from_state(np.zeros(state_size(2, 3), np.int64), 2, 3)
    assert not r['recall'].any() and not r['ar'].any() and r['auc'] == 0.0 and r['avg_props'] == 0.0 and r['n_gt'] == 0
    with pytest.raises(ValueError, match='state'):
        recall_from_state(np.zeros(5, np.int64), 2, 3)


def test_the_reference_refuses_bad_settings():
    from cfn_hip.recall import DEFAULT_TIOU, recall_reference
    det, gt = hand_batch()
    assert len(DEFAULT_TIOU) == 10 and DEFAULT_TIOU[0] == 0.5 and DEFAULT_TIOU[-1] == 0.95
    assert recall_reference([(det, gt)], 3, [0.5] * 16, 1)['recall'].shape == (16, 1)
    for tiou in ([], [0.5] * 17, [0.0], [1.5], [NAN]):
        with pytest.raises(ValueError, match='tiou'):
            recall_reference([(det, gt)], 3, tiou, 4)
    for n_max in (0, 1025, 2.5):
        with pytest.raises(ValueError, match='n_max'):
            recall_reference([(det, gt)], 3, (0.5,), n_max)
    with pytest.raises(ValueError, match='classes'):
        recall_reference([(det, gt)], 4)


def test_c_abi_prototypes_workspace_and_refusals():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    for name in ('cfn_seg_recall_workspace_bytes', 'cfn_seg_recall_rank_tile', 'cfn_seg_recall_add', 'cfn_seg_recall_value'):
        assert name in protos, name
    assert protos['cfn_seg_recall_workspace_bytes'][0] is ctypes.c_long
    dts = protos['cfn_seg_recall_add'][2]
    assert dts[8] == torch.int32 and dts[9] == torch.int64 and dts[0] == torch.float64 and dts[1] == torch.float32
    lib = cfn_hip.load()
    from cfn_hip import ops
    assert lib.cfn_seg_recall_rank_tile() == ops.SEG_RECALL_RANK_TILE
    ws = lib.cfn_seg_recall_workspace_bytes
    assert ws(8, 157, 1000, 50, 10) >= 4000 and ws(8, 157, 1000, 50, 10) % 8 == 0 and ws(1, 1, 1, 1, 1) >= 4
    for bad in ((0, 1, 1, 1, 1), (65536, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 65536, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1 << 31, 1, 1), (1, 1, 1, 0, 1),
                (1, 1, 1, 1 << 31, 1), (1, 1, 1, 1, 0), (1, 1, 1, 1, 17)):
        assert ws(*bad) == -1, bad
    with pytest.raises(RuntimeError, match='seg_recall'):
        ops.seg_recall_workspace_bytes(1, 1, 1, 1, 17)
    p = 4096                                                                           # (never dereferenced: every refusal comes before a launch)
    good = dict(B=2, C=3, t_max=10, n_thr=2, n_max=4, score_col=0, det_cap=8, n_seg=9)

    def add(ptrs=(p,) * 11, **kw):
        a = dict(good, **kw)
        return lib.cfn_seg_recall_add(*ptrs, a['B'], a['C'], a['t_max'], a['n_thr'], a['n_max'], a['score_col'], a['det_cap'], a['n_seg'], None)
    for i in range(11):
        assert add(tuple(None if j == i else p for j in range(11))) == 1 and 'null' in cfn_hip.last_error()
    for kw in (dict(B=0), dict(B=65536), dict(C=0), dict(C=65536), dict(t_max=0), dict(n_thr=0), dict(n_thr=17), dict(n_max=0), dict(n_max=1025),
               dict(score_col=2), dict(score_col=-1), dict(det_cap=0), dict(det_cap=1 << 31), dict(n_seg=0), dict(n_seg=1 << 31)):
        assert add(**kw) == 1, kw
    assert add((p,) * 10 + (p + 4,)) == 1 and 'boundary' in cfn_hip.last_error()
    val = lib.cfn_seg_recall_value
    assert val(None, p, 2, 4, None) == 1 and val(p, None, 2, 4, None) == 1
    for n_thr, n_max in ((0, 4), (17, 4), (2, 0), (2, 1025)):
        assert val(p, p, n_thr, n_max, None) == 1


def test_the_ops_and_the_meter_have_no_cpu_path():
    _lib()
    from cfn_hip import ops
    from cfn_hip.recall import ProposalRecallMeter, state_size
    with pytest.raises(RuntimeError, match='keeps its state on a GPU'):
        ProposalRecallMeter('cpu', 3)
    det, gt = hand_batch()
    state = torch.zeros(state_size(2, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.seg_recall_add(det.seg, det.score, det.offsets, gt.seg, gt.offsets, gt.fps, gt.window, torch.tensor(HAND_TIOU, dtype=torch.float64), state, 3,
                           gt.t_max, 4)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.seg_recall_value(state, 2, 4)


def test_the_scripts_take_the_meter():
    import inspect
    import train_coarse_fineFEAT as tc
    import train_fine
    for mod in (train_fine, tc):
        assert inspect.signature(mod.run).parameters['proposal_recall'].default is None
    import argparse
    parser = argparse.ArgumentParser()
    train_fine.add_detect_args(parser)
    train_fine.seg_ap_arguments(parser)
    args = parser.parse_args([])
    assert args.prop_recall is False and args.prop_recall_n == 100 and args.prop_recall_score == 'max'
    assert train_fine.prop_recall_from_args(args) is None and train_fine.prop_recall_argv(args) == []
    args = parser.parse_args(['--prop-recall', '--prop-recall-n', '50', '--prop-recall-tiou', '0.5,0.75', '--prop-recall-score', 'mean'])
    with pytest.raises(ValueError, match='--detect'):                                  # no decode exists
        train_fine.prop_recall_from_args(args)
    args = parser.parse_args(['--prop-recall', '--seg-ap', '--detect-levels', '0.8,0.5'])
    assert train_fine.prop_recall_argv(args) == ['--prop-recall', '--prop-recall-n', '100', '--prop-recall-tiou', args.prop_recall_tiou,
                                                 '--prop-recall-score', 'max']
    with pytest.raises(RuntimeError, match='a decode'):
        train_fine.check_proposal_recall(object(), None, None)
