"""Proposal recall at N per video (AR@N): how many ground-truth segments at least one of the N best candidates of their video covers at a
temporal-IoU threshold, accumulated on the device (cfn_hip.ops.seg_recall_add / seg_recall_value, csrc/segrecall.hip).

Multi-threshold proposals, NMS and soft-NMS (cfn_hip/detections.py) produce ranked candidate lists.  Segment mAP (cfn_hip/segap.py) mixes
whether the candidates cover the ground truth with whether their scores rank well, and its greedy one-to-one matching punishes the redundancy
a proposal stage is meant to have.  Recall is the figure proposals are judged by; this is the rule, stated once.  Inputs: a ``Detections``
(seg, score, offsets, cap); the ground truth as ``cfn_hip.segap.ground_truth`` yields it: ``seg (S, 3)`` fp64 rows [class, start_s, end_s],
``offsets (B + 1)`` int32, ``fps (B)`` fp64, ``window (B, 2)`` int32 and the host int ``t_max``; ``tiou (n_thr)`` fp64, 1 <= n_thr <= 16, each
in (0, 1], any order (default 0.5, 0.55, ..., 0.95); host ints ``n_max`` in [1, 1024] (default 100) and ``score_col`` (0 = max, 1 = mean):

    R1. participation and window clip: rule 1 of cfn_hip/segap.py to the bit (clip_reference): a row PARTICIPATES iff its window has frames,
        its class is an integer of [0, C) and its clipped end is behind its clipped start.  Row g belongs to video b iff offsets[b] <= g <
        offsets[b + 1] (offsets clamped to [0, S] and expected not to decrease: offsets are data, malformed ones give wrong values, never an
        access outside the buffers).
    R2. tIoU: tiou_reference of cfn_hip/segap.py, unchanged.
    R3. video rank: the candidates of video b are the rows offsets[b] .. offsets[b + 1] of the detections, clamped to [0, cap], ALL classes
        together, ranked by score[:, score_col] descending in fp32.  A NaN is taken as -inf (NMS's convention), so the ranks of a video are a
        permutation of 0 .. n_b - 1; ties go to the lower row index.
    R4. first hit: for a participating row g (video b, class c) and threshold k, hit[k, g] is the smallest video rank among the candidates of
        the SAME video and class whose tIoU with g is > 0 and >= tiou[k]; n_max when there is none or the smallest is >= n_max.  A row that
        does not participate has hit[k, g] = -1.  There is no one-to-one matching: a candidate may recall several rows and a row is recalled
        by any candidate -- what separates the metric from rule 4 of segment AP.
    R5. state: one int64 tensor: hist (n_thr, n_max), then n_gt, n_videos, n_props.  A batch adds 1 to hist[k, hit[k, g]] for every
        participating g with hit < n_max, the participating rows to n_gt, B to n_videos and the sum of the clamped n_b to n_props.  Integer
        arithmetic only: the same in every run whatever order the kernel adds in, and ADDITIVE: the state of two batches, or of two
        data-parallel ranks, is the sum of their states.
    R6. value, fp64: recall[k, n] = float64(hist[k, 0] + .. + hist[k, n]) / float64(n_gt) for n = 0 .. n_max - 1, that is N = n + 1: ONE IEEE
        division, 0 everywhere when n_gt == 0.  ar[n] = (recall[0, n] + .. + recall[n_thr - 1, n]) / n_thr, added in k order.  auc = (ar[0] +
        .. + ar[n_max - 1]) / n_max, added in n order.  avg_props = n_props / n_videos (0 without videos).  There is no product, so nothing
        contracts: the device result is BIT-EQUAL to this module's numpy.

``video_rank_reference``, ``first_hit_reference``, ``recall_from_state`` and ``recall_reference`` spell the rules in numpy on any device and are
the tests' reference; ``ProposalRecallMeter`` is the device-resident meter.  Limits: B and C <= 65535, at most 16 thresholds, n_max <= 1024;
the video rank is by counting, O(n_b^2) in the candidates of a video.  Matching is per class (class-agnostic matching, per-class tables and
the variant that rescales N by a data set's average proposal count are out of scope).  No accuracy gain is claimed for any proposal setting:
this is the instrument that lets one be claimed or refuted.

This module is host only (numpy + torch) apart from the calls into cfn_hip.ops.
"""
import numpy as np
import torch

from .detections import SCORE_COLUMNS, Detections
from .segap import _np, _tiou_list, clip_reference, ground_truth, tiou_reference

DEFAULT_TIOU = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)
MAX_THR, MAX_N = 16, 1024


def _tiou(tiou):
    return _tiou_list(tiou, MAX_THR)


def _n_max(n_max):
    if isinstance(n_max, bool) or int(n_max) != n_max or not 1 <= int(n_max) <= MAX_N:
        raise ValueError('n_max: an int in [1, %d] expected, got %r' % (MAX_N, n_max))
    return int(n_max)


def _ranges(det):
    """the clamped row range of every video of a Detections -> (lo (B,), hi (B,)) int64"""
    doff = _np(det.offsets, np.int64)
    cap = min(int(det.cap), int(det.seg.shape[0]))
    lo = np.clip(doff[:-1], 0, cap)
    return lo, np.clip(doff[1:], lo, cap)


def video_rank_reference(det, score_col=0):
    """R3 in numpy -> rank (rows,) int64: the rank of every row among the candidates of its video, -1 for a row of no video"""
    score = _np(det.score, np.float32)[:, score_col]
    rank = np.full(score.shape[0], -1, np.int64)
    for lo, hi in zip(*_ranges(det)):
        s = score[lo:hi].copy()
        s[np.isnan(s)] = -np.inf
        rank[lo + np.argsort(-s, kind='stable')] = np.arange(hi - lo)                 # (stable: ties keep the row order)
    return rank


def first_hit_reference(det, seg, offsets, fps, window, t_max, tiou=DEFAULT_TIOU, n_max=100, score_col=0):
    """R1-R4 in numpy -> (hit (n_thr, S) int32, part (S,) bool, n_props: the sum of the clamped n_b)"""
    th = [np.float64(x) for x in _tiou(tiou)]
    n_max = _n_max(n_max)
    C = int(det.n_classes)
    dseg = _np(det.seg, np.float64)
    rank = video_rank_reference(det, score_col)
    lo, hi = _ranges(det)
    part, sp, ep, vid = clip_reference(seg, offsets, fps, window, t_max, C)
    gcls = _np(seg, np.float64)[:, 0]
    hit = np.full((len(th), len(part)), -1, np.int32)
    for g in np.flatnonzero(part):
        b = int(vid[g])
        rows = lo[b] + np.flatnonzero(dseg[lo[b]:hi[b], 0] == gcls[g])
        best = [n_max] * len(th)
        for d in rows:
            v = tiou_reference(dseg[d, 1], dseg[d, 2], sp[g], ep[g])
            if v > 0.0:
                for k, t in enumerate(th):
                    if v >= t and rank[d] < best[k]:
                        best[k] = int(rank[d])
        hit[:, g] = best
    return hit, part, int((hi - lo).sum())


def state_size(n_thr, n_max):
    return int(n_thr) * int(n_max) + 3


def state_from_hit(hit, n_props, n_videos, n_max):
    """R5 in numpy: one batch's hit table -> its state (n_thr * n_max + 3,) int64"""
    n_thr = hit.shape[0]
    state = np.zeros(state_size(n_thr, n_max), np.int64)
    hist = state[:n_thr * n_max].reshape(n_thr, n_max)
    for k in range(n_thr):
        h = hit[k]
        np.add.at(hist[k], h[(h >= 0) & (h < n_max)], 1)
    state[-3:] = [int((hit[0] >= 0).sum()), int(n_videos), int(n_props)]
    return state


def recall_from_state(state, n_thr, n_max):
    """R6 in numpy: a state -> a dict: recall (n_thr, n_max), ar (n_max,), auc and avg_props (float64), n_gt, n_videos, n_props (ints)"""
    state = _np(state, np.int64)
    n_thr, n_max = int(n_thr), int(n_max)
    if state.shape != (state_size(n_thr, n_max),):
        raise ValueError('state: (%d,) int64 expected, got %s' % (state_size(n_thr, n_max), state.shape))
    hist = state[:n_thr * n_max].reshape(n_thr, n_max)
    n_gt, n_videos, n_props = (int(x) for x in state[-3:])
    recall = np.zeros((n_thr, n_max), np.float64)
    if n_gt > 0:
        recall = np.cumsum(hist, axis=1, dtype=np.int64).astype(np.float64) / np.float64(n_gt)
    ar = np.zeros(n_max, np.float64)
    for k in range(n_thr):                                                            # k order
        ar = ar + recall[k]
    ar = ar / np.float64(n_thr)
    auc = np.float64(0.0)
    for n in range(n_max):                                                            # n order
        auc = auc + ar[n]
    auc = auc / np.float64(n_max)
    avg = np.float64(n_props) / np.float64(n_videos) if n_videos > 0 else np.float64(0.0)
    return {'recall': recall, 'ar': ar, 'auc': auc, 'avg_props': avg, 'n_gt': n_gt, 'n_videos': n_videos, 'n_props': n_props}


def _batch_gt(batch):
    if len(batch) == 2:
        lab = batch[1]
        return lab.seg, lab.offsets, lab.fps, lab.window, lab.t_max
    return tuple(batch[1:])


def recall_reference(batches, n_classes, tiou=DEFAULT_TIOU, n_max=100, score_col=0):
    """R1-R6 in numpy over a list of batches, each (det, seg, offsets, fps, window, t_max) or (det, SegLabels) -> recall_from_state's dict plus
    state (int64) and hits (per batch)"""
    th, n_max = _tiou(tiou), _n_max(n_max)
    state = np.zeros(state_size(len(th), n_max), np.int64)
    hits = []
    for batch in batches:
        det = batch[0]
        if int(det.n_classes) != int(n_classes):
            raise ValueError('recall_reference: detections over %d classes, %d expected' % (det.n_classes, n_classes))
        hit, _, n_props = first_hit_reference(det, *_batch_gt(batch), th, n_max, score_col)
        state += state_from_hit(hit, n_props, int(det.offsets.numel()) - 1, n_max)
        hits.append(hit)
    out = recall_from_state(state, len(th), n_max)
    out.update(state=state, hits=hits)
    return out


def all_reduce_state(state, group=None):
    """the sum of `state` over the process group, in a COPY (the state itself keeps this rank's counts); without an initialised process group:
    the state itself, untouched"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return state
    total = state.clone()
    dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
    return total


class ProposalRecallMeter(object):
    """Proposal recall over a validation phase, resident on the GPU: ``state`` is one int64 tensor (hist (n_thr, n_max), n_gt, n_videos,
    n_props; rule R5).

    ``add(det, labels)`` takes a batch's ``Detections`` and its ``SegLabels`` -- or the dense pair ``(labels (B, C, TL), valid_t (B,))``, decoded
    into frame-unit ground truth as SegmentAPMeter does -- and advances the state without a read-back (three launches); it returns ``hit
    (n_thr, S)`` on the device.  With ``out=`` (ops.seg_recall_add's tuple) it allocates nothing and is safe inside a graph capture.
    ``value_device()`` -> a dict of device tensors; ``value()`` -> the same as numpy with ONE read-back, plus n_gt.  The state is additive:
    ``merge(other)`` adds another meter's, ``all_reduce(group)`` gives the sum over the data-parallel ranks in a copy, and ``value(group=)``
    evaluates that sum -- so, unlike SegmentAPMeter, it works under a world size above 1."""

    def __init__(self, device, n_classes, tiou=DEFAULT_TIOU, n_max=100, score='max'):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('ProposalRecallMeter keeps its state on a GPU (got device %s); cfn_hip.recall.recall_reference is the host spelling' % self.device)
        if score not in SCORE_COLUMNS:
            raise ValueError("score: 'max' or 'mean' expected, got %r" % (score,))
        if int(n_classes) < 1:
            raise ValueError('n_classes >= 1 expected, got %r' % (n_classes,))
        self.tiou, self.n_max = tuple(_tiou(tiou)), _n_max(n_max)
        self.n_classes, self.score, self.score_col = int(n_classes), score, SCORE_COLUMNS[score]
        self._tiou = torch.tensor(self.tiou, dtype=torch.float64, device=self.device)
        self.state = torch.zeros(state_size(len(self.tiou), self.n_max), dtype=torch.int64, device=self.device)

    @property
    def settings(self):
        return self.tiou, self.n_max, self.score, self.n_classes

    def reset(self):
        self.state.zero_()               # on the current stream

    def add(self, det, labels, out=None):
        from . import ops
        if not isinstance(det, Detections):
            raise TypeError('ProposalRecallMeter.add: a cfn_hip.detections.Detections expected, got %s' % type(det).__name__)
        if int(det.n_classes) != self.n_classes:
            raise RuntimeError('ProposalRecallMeter.add: detections over %d classes, the meter holds %d' % (det.n_classes, self.n_classes))
        seg, offsets, fps, window, t_max = ground_truth(labels, self.device)
        if int(offsets.numel()) != det.batch + 1:
            raise RuntimeError('ProposalRecallMeter.add: detections of %d videos against labels of %d' % (det.batch, int(offsets.numel()) - 1))
        dseg, dscore = det.seg, det.score
        if int(dseg.shape[0]) != int(det.cap):                                        # (out= buffers may be longer than the decode's cap)
            dseg, dscore = dseg[:det.cap], dscore[:det.cap]
        return ops.seg_recall_add(dseg, dscore, det.offsets, seg, offsets, fps, window, self._tiou, self.state, self.n_classes, t_max, self.n_max,
                                  self.score_col, out)

    def merge(self, other):
        """add another meter's state (same tiou, n_max, score and classes) to this one's"""
        if not isinstance(other, ProposalRecallMeter) or other.settings != self.settings:
            raise ValueError('ProposalRecallMeter.merge: a meter of the same tiou, n_max, score and classes expected, got %r against %r'
                             % (getattr(other, 'settings', type(other).__name__), self.settings))
        self.state += other.state.to(self.device)
        return self

    def all_reduce(self, group=None):
        """the state summed over the process group, in a copy; without an initialised group the state itself (nothing is done)"""
        return all_reduce_state(self.state, group)

    def _split(self, flat):
        n_thr, n = len(self.tiou), self.n_max
        return {'recall': flat[:n_thr * n].view(n_thr, n), 'ar': flat[n_thr * n:n_thr * n + n], 'auc': flat[n_thr * n + n], 'avg_props': flat[n_thr * n + n + 1]}

    def value_device(self, state=None):
        """{'recall' (n_thr, n_max), 'ar' (n_max,), 'auc', 'avg_props'} fp64 on the device (rule R6); reads nothing back"""
        from . import ops
        return self._split(ops.seg_recall_value(self.state if state is None else state, len(self.tiou), self.n_max))

    def value(self, group=None):
        """value_device() of the state summed over the ranks of `group` (this rank's alone without a process group) as numpy float64, plus
        the int n_gt, with ONE read-back"""
        from . import ops
        state = self.all_reduce(group)
        flat = ops.seg_recall_value(state, len(self.tiou), self.n_max)
        host = torch.cat([flat.view(torch.int64), state[-3:-2]]).cpu()
        out = {k: v.numpy().copy() for k, v in self._split(host[:-1].view(torch.float64)).items()}
        out['auc'], out['avg_props'] = np.float64(out['auc']), np.float64(out['avg_props'])
        out['n_gt'] = int(host[-1])
        return out
