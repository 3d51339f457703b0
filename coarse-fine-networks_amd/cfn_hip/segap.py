"""Segment-level average precision at temporal-IoU (tIoU) thresholds: ``Detections`` against ``SegLabels``, matched and accumulated on the
device (cfn_hip.ops.segap_match / segap_append / segap_value, csrc/segap.hip).

The project could report only the reference's per-frame mAP (apmeter.APMeter / DeviceAPMeter).  Temporal activity *detection* is judged per
segment: a detection counts when its tIoU with an unmatched ground-truth segment of the same class and video reaches a threshold, and AP is
taken over the ranked detections.  The reference stops at ``probs`` (train_fine.py:199-222), so there is nothing to copy; this is the rule,
stated once.  Inputs: ``Detections`` (seg, score, offsets); ground truth ``seg (S, 3)`` fp64 rows [class, start_s, end_s], ``offsets (B + 1)``
int32, ``fps (B)`` fp64, ``window (B, 2)`` int32 (the tensors of ``SegLabels``) and its host int ``t_max``; ``tiou (n_thr)`` fp64,
1 <= n_thr <= 8, each in (0, 1]; a host int ``score_col`` (0 = max, 1 = mean):

    1. window clip of the ground truth: n = clamp(window[b,1], 0, t_max), w0 = (float64(window[b,0]) - 0.5) / fps[b],
       w1 = (float64(window[b,0] + n) - 0.5) / fps[b] -- the half-frame-outward extent ``decode`` gives a detection that covers the whole
       window.  s' = max(s, w0), e' = min(e, w1) (spelled ``s if s > w0 else w0``: a NaN bound gives way to the window's).  The row
       PARTICIPATES iff n > 0, its class is an integer of [0, C) and e' > s'.  One rule for training windows and for annotations that run
       past the end of the video.  n_gt[c] counts participating rows.
    2. tIoU of a detection (sd, ed) and a clipped row (s', e'): inter = min(ed, e') - max(sd, s'); the tIoU is 0 unless inter > 0, otherwise
       inter / ((ed - sd) + (e' - s') - inter).  Plain IEEE fp64; there is no product, so nothing can contract into an FMA, and the
       division is the only rounding step that matters: device and numpy give the same double.
    3. order: within one (video, class) group the detections are taken by score[:, score_col] descending (fp32), ties by row index
       ascending (= t0 ascending).  Scores of decoded segments are never NaN.
    4. greedy matching, independently per threshold k: a detection takes the participating, not-yet-matched-at-k ground-truth row of its
       video and class with the largest tIoU among those with tIoU >= tiou[k]; ties go to the lowest ground-truth row index.  If it takes
       one it is a true positive at k and the row is used up at k; otherwise it is a false positive.
    5. per detection: one byte ``tp`` (bit k = true positive at k) and optionally ``match (n_thr, cap)`` int32 = the row index or -1.
    6. accumulation: class c's store receives this batch's detections of class c in (video, row) order behind the rows it holds; counts[c]
       and n_gt[c] advance.  A batch that would push ANY class past the capacity writes nothing, changes no count and sets a flag bit (the
       semantics of cfn_ap_append).
    7. AP: per class and threshold a stable descending sort by score in insertion order, with cfn_ap_sort's ordering of special values;
       the tp byte travels as the payload.  ap[k, c] = (sum over the ranks r whose bit k is set of tp_cum_r / r) / n_gt[c], summed in fp64
       in a fixed order, rounded to fp32; 0 where n_gt[c] == 0.  This is the project's non-interpolated AP (apmeter.py) divided by the
       ground-truth count, so a missed segment costs.  map[k] = the mean over the classes with n_gt > 0 (fp64 in class order, rounded to
       fp32).

``match_reference`` and ``ap_reference`` spell the rules in numpy on any device and are the tests' reference; ``SegmentAPMeter`` is the
device-resident meter.  Limits: B and C <= 65535; at most 8 thresholds; the order inside a (video, class) group is rank by counting,
O(nd^2) in its detections.  AP is not additive, so a plain meter is ONE process's (the training entry points refuse it under a world size
above 1); a meter made with ``across_ranks=True`` evaluates the stores of all data-parallel ranks appended in rank order
(cfn_hip/apmerge.py: rules M1-M4), and ``merge`` / ``merged`` do the same for meters of one process.

This module is host only (numpy + torch) apart from the calls into cfn_hip.ops.
"""
import numpy as np
import torch

from .detections import SCORE_COLUMNS, Detections, _soft, decode
from .seglabels import SegLabels

DEFAULT_TIOU = (0.1, 0.3, 0.5, 0.7, 0.9)


def _np(t, dtype):
    return np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dtype, copy=False))


def _tiou_list(tiou, most=8):
    th = [float(x) for x in (tiou.tolist() if torch.is_tensor(tiou) or isinstance(tiou, np.ndarray) else tiou)]
    if not 1 <= len(th) <= most or not all(0.0 < x <= 1.0 for x in th):
        raise ValueError('tiou: 1 to %d thresholds in (0, 1] expected, got %r' % (most, th))
    return th


def clip_reference(seg, offsets, fps, window, t_max, n_classes):
    """rule 1 in numpy -> (part (S,) bool, s' (S,), e' (S,), video (S,) int64 or -1 for rows no offset range covers)"""
    seg, offs = _np(seg, np.float64), _np(offsets, np.int64)
    f, win = _np(fps, np.float64), _np(window, np.int64)
    S = seg.shape[0]
    part, sp, ep, vid = np.zeros(S, bool), np.zeros(S), np.zeros(S), np.full(S, -1, np.int64)
    for b in range(len(offs) - 1):
        n = min(max(int(win[b, 1]), 0), int(t_max))
        with np.errstate(all='ignore'):
            w0 = (np.float64(int(win[b, 0])) - 0.5) / f[b]
            w1 = (np.float64(int(win[b, 0]) + n) - 0.5) / f[b]
        lo = min(max(int(offs[b]), 0), S)
        hi = min(max(int(offs[b + 1]), lo), S)
        for g in range(lo, hi):
            c, s, e = seg[g]
            sp[g] = s if s > w0 else w0
            ep[g] = e if e < w1 else w1
            vid[g] = b
            part[g] = n > 0 and 0 <= c < n_classes and c == np.floor(c) and ep[g] > sp[g]
    return part, sp, ep, vid


def tiou_reference(sd, ed, sp, ep):
    """rule 2 on numpy float64 scalars"""
    inter = (ed if ed < ep else ep) - (sd if sd > sp else sp)
    if not inter > 0.0:
        return np.float64(0.0)
    with np.errstate(all='ignore'):
        return inter / ((ed - sd) + (ep - sp) - inter)


def match_reference(det, seg, offsets, fps, window, t_max, tiou, score_col=0):
    """rules 1-5 in numpy: det (a Detections, any device) against the ground truth tensors -> (tp (n,) uint8, match (n_thr, n) int32,
    n_gt (C,) int64) over the n = min(total, cap) detection rows"""
    th = [np.float64(x) for x in _tiou_list(tiou)]
    C = int(det.n_classes)
    dseg, dscore, doff = _np(det.seg, np.float64), _np(det.score, np.float32), _np(det.offsets, np.int64)
    cap = min(int(det.cap), dseg.shape[0])
    n = min(int(doff[-1]), cap)
    part, sp, ep, vid = clip_reference(seg, offsets, fps, window, t_max, C)
    gcls = _np(seg, np.float64)[:, 0]
    n_gt = np.zeros(C, np.int64)
    for g in np.flatnonzero(part):
        n_gt[int(gcls[g])] += 1
    tp, match = np.zeros(n, np.uint8), np.full((len(th), n), -1, np.int32)
    for b in range(len(doff) - 1):
        lo, hi = min(int(doff[b]), cap), min(int(doff[b + 1]), cap)
        rows_b = np.flatnonzero(part & (vid == b))
        for c in np.unique(dseg[lo:hi, 0]):
            rows = lo + np.flatnonzero(dseg[lo:hi, 0] == c)
            gts = [int(g) for g in rows_b if gcls[g] == c]                            # ascending row index
            order = rows[np.argsort(-dscore[rows, score_col], kind='stable')]         # rule 3
            used = {g: 0 for g in gts}
            for d in order:
                v = {g: tiou_reference(dseg[d, 1], dseg[d, 2], sp[g], ep[g]) for g in gts}
                for k, t in enumerate(th):                                            # rule 4
                    best = -1
                    for g in gts:
                        if v[g] > 0.0 and v[g] >= t and not (used[g] >> k) & 1 and (best < 0 or v[g] > v[best]):
                            best = g
                    if best >= 0:
                        used[best] |= 1 << k
                        tp[d] |= 1 << k
                        match[k, d] = best
    return tp, match, n_gt


def ap_from_stores(scores, tps, n_gt, n_thr):
    """rule 7 in numpy: per class c the arrays scores[c] (fp32) and tps[c] (uint8) in insertion order -> (ap (n_thr, C) fp32, map (n_thr,) fp32)"""
    C = len(scores)
    ap = np.zeros((n_thr, C), np.float32)
    for c in range(C):
        if n_gt[c] <= 0 or len(scores[c]) == 0:
            continue
        order = np.argsort(-np.asarray(scores[c], np.float32), kind='stable')
        bits = np.asarray(tps[c], np.uint8)[order]
        ranks = np.arange(1, len(bits) + 1, dtype=np.float64)
        for k in range(n_thr):
            hit = ((bits >> k) & 1).astype(bool)
            if hit.any():
                terms = np.cumsum(hit)[hit].astype(np.float64) / ranks[hit]
                ap[k, c] = np.float32(np.cumsum(terms)[-1] / np.float64(n_gt[c]))     # (cumsum: one addend after the other)
    have = np.flatnonzero(np.asarray(n_gt) > 0)
    mp = np.zeros(n_thr, np.float32)
    for k in range(n_thr):
        if have.size:
            mp[k] = np.float32(np.cumsum(ap[k, have].astype(np.float64))[-1] / np.float64(have.size))
    return ap, mp


def ap_reference(batches, n_classes, tiou=DEFAULT_TIOU, score_col=0):
    """rules 1-7 in numpy over a list of batches, each (det, seg, offsets, fps, window, t_max) or (det, SegLabels) -> a dict: ap (n_thr, C)
    fp32, map (n_thr,) fp32, counts (C,), n_gt (C,), scores / tps (per class, insertion order), tp / match (per batch)"""
    th = _tiou_list(tiou)
    C = int(n_classes)
    scores, tps = [[] for _ in range(C)], [[] for _ in range(C)]
    n_gt = np.zeros(C, np.int64)
    per_batch = []
    for batch in batches:
        det = batch[0]
        if len(batch) == 2:
            lab = batch[1]
            gt = (lab.seg, lab.offsets, lab.fps, lab.window, lab.t_max)
        else:
            gt = tuple(batch[1:])
        tp, match, g = match_reference(det, *gt, th, score_col)
        per_batch.append((tp, match, g))
        n_gt += g
        dseg, dscore = _np(det.seg, np.float64), _np(det.score, np.float32)
        for i in range(len(tp)):                                                      # rule 6: (video, row) order is row order
            c = int(dseg[i, 0])
            scores[c].append(dscore[i, score_col])
            tps[c].append(tp[i])
    ap, mp = ap_from_stores(scores, tps, n_gt, len(th))
    return {'ap': ap, 'map': mp, 'counts': np.array([len(s) for s in scores], np.int64), 'n_gt': n_gt,
            'scores': [np.asarray(s, np.float32) for s in scores], 'tps': [np.asarray(t, np.uint8) for t in tps], 'batches': per_batch}


def ground_truth(labels, device):
    """labels (a SegLabels, or the dense pair (labels (B, C, TL) fp32, valid_t (B,))) -> (seg, offsets, fps, window, t_max) on `device`: what
    SegmentAPMeter and cfn_hip.recall.ProposalRecallMeter match against"""
    if isinstance(labels, SegLabels):
        labels = labels.to(device)
        return labels.seg, labels.offsets, labels.fps, labels.window, int(labels.t_max)
    dense, valid_t = labels
    dense, valid_t = dense.to(device), valid_t.to(device, torch.int32)
    gt = decode(dense.detach().float().contiguous(), valid_t, thr=0.5)             # frame units: fps = 1, start = 0
    B, TL = int(dense.shape[0]), int(dense.shape[2])
    window = torch.stack([torch.zeros_like(valid_t), valid_t], 1).contiguous()
    return gt.seg, gt.offsets, torch.ones(B, dtype=torch.float64, device=device), window, TL


class SegmentAPMeter(object):
    """Segment-level AP over a validation phase, resident on the GPU: class-major stores scores (C, cap) fp32 and tps (C, cap) uint8,
    counts (C,), n_gt (C,) and a flag word on the device.

    ``add(det, labels)`` matches a batch's ``Detections`` against its ``SegLabels`` and appends without a read-back (three launches).  For
    dense loaders ``labels`` may be the dense pair ``(labels (B, C, TL), valid_t (B,))``, which is decoded with ``decode(labels, valid_t,
    thr=0.5)`` into frame-unit ground truth.  ``value_device()`` -> (ap (n_thr, C), map (n_thr,)) on the device; ``value()`` checks the
    flags with ONE read-back and returns the two as CPU tensors.

    capacity=None: the stores grow geometrically.  The host keeps only an upper bound of the fullest class, B * ((TL + 1) // 2) per batch,
    TL = the frames the detections were decoded over: ``add(tl=)``, by default the labels' t_max (the same number wherever probs and labels
    come from one batch, as in the training entry points; detections decoded over MORE frames than that need tl=, or the bound is too
    small and the batch is dropped and flagged).  The bound is loose for segments, so where it passes the capacity the meter reads the
    true maximum count once (a single int) and resets the bound before it grows.  An explicit capacity (rows per class) never reads back: ``add`` with ``out=`` is then safe inside a
    graph capture, and a batch that does not fit is dropped, flagged on the device and reported by ``value()``.

    thr, max_gap, min_len: the decode parameters the training entry points use when they are given the meter without a DetectionWriter.
    levels, nms (default 0.5), nms_score: with `levels` set those entry points run cfn_hip.detections.propose (candidates at K levels, then
    temporal NMS) in place of decode; the meter only keeps the three for them.  A batch of proposals can hold K times the rows of a decode:
    ``add(levels=K)`` multiplies growing mode's bound (post-NMS groups can still exceed (TL + 1) // 2 rows).  soft (a
    cfn_hip.detections.SoftNMS, with `levels`): propose's second stage is soft_nms; kept for the entry points like the three.  filter (a
    cfn_hip.scorefilter.ScoreFilter): the entry points smooth the probs with it in front of their decode; kept for them like the rest.
    A meter made without the next two arguments is one process's, exactly as before.  across_ranks=True (group: the process group, None =
    the default one): under a world size above 1 ``value_device()`` and ``value()`` evaluate the stores of ALL ranks, appended in rank order
    into a fresh store (cfn_hip.apmerge.gather_stores): every rank gets the same bits, those of one process fed the ranks' batches one rank
    after another.  The call is then a collective that every rank must make; the rank's own stores are untouched, so ``reset()`` and further
    ``add``s behave as before.  Without a process group, or with a world size of 1, nothing is gathered or copied.  ``merge(*others)`` and
    ``SegmentAPMeter.merged(parts)`` append other meters' rows within one process (ONE ops.ap_merge)."""

    MIN_CAPACITY = 1024

    def __init__(self, device, n_classes, tiou=DEFAULT_TIOU, score='max', capacity=None, thr=0.5, max_gap=0, min_len=1, levels=None, nms=None,
                 nms_score='max', soft=None, across_ranks=False, group=None, filter=None):
        self.device = torch.device(device)
        if filter is not None:
            from .scorefilter import ScoreFilter
            if not isinstance(filter, ScoreFilter):
                raise TypeError('SegmentAPMeter: filter: a cfn_hip.scorefilter.ScoreFilter expected, got %s' % type(filter).__name__)
        self.filter = filter
        self.across_ranks, self.group = bool(across_ranks), group
        if self.device.type != 'cuda':
            raise RuntimeError('SegmentAPMeter keeps its rows on a GPU (got device %s); cfn_hip.segap.ap_reference is the host spelling' % self.device)
        if score not in SCORE_COLUMNS:
            raise ValueError("score: 'max' or 'mean' expected, got %r" % (score,))
        if int(n_classes) < 1:
            raise ValueError('n_classes >= 1 expected, got %r' % (n_classes,))
        if capacity is not None and int(capacity) < 1:
            raise ValueError('capacity: a positive number of rows per class expected, got %r' % (capacity,))
        self.tiou = tuple(_tiou_list(tiou))
        self.n_classes, self.score, self.score_col = int(n_classes), score, SCORE_COLUMNS[score]
        self.capacity = None if capacity is None else int(capacity)
        self.thr, self.max_gap, self.min_len = thr, int(max_gap), int(min_len)
        if levels is None and nms is not None:
            raise ValueError('SegmentAPMeter: nms without levels: a single-level decode does not overlap itself')
        if nms_score not in SCORE_COLUMNS:
            raise ValueError("nms_score: 'max' or 'mean' expected, got %r" % (nms_score,))
        self.levels, self.nms, self.nms_score = levels, (0.5 if nms is None else float(nms)), nms_score
        if levels is None and soft is not None:
            raise ValueError('SegmentAPMeter: soft without levels: a single-level decode does not overlap itself')
        self.soft = None if soft is None else _soft(soft, self.nms)[0]
        self._tiou = torch.tensor(self.tiou, dtype=torch.float64, device=self.device)
        self._state = torch.zeros(2 * self.n_classes + 1, dtype=torch.int32, device=self.device)      # counts, n_gt, flags
        cap = self.capacity if self.capacity is not None else self.MIN_CAPACITY
        self._scores, self._tps = self._alloc(cap)
        self._bound = 0
        self._sort_bufs = None

    @property
    def counts(self):
        return self._state[:self.n_classes]

    @property
    def n_gt(self):
        return self._state[self.n_classes:2 * self.n_classes]

    @property
    def flags(self):
        return self._state[2 * self.n_classes:]

    @property
    def stores(self):
        """(scores (C, cap) fp32, tps (C, cap) uint8)"""
        return self._scores, self._tps

    def reset(self):
        self._state.zero_()              # on the current stream; the buffers stay
        self._bound = 0

    def _alloc(self, cap):
        return (torch.empty(self.n_classes, cap, dtype=torch.float32, device=self.device),
                torch.empty(self.n_classes, cap, dtype=torch.uint8, device=self.device))

    def _reserve(self, rows):
        """growing mode: room for `rows` more rows in the fullest class"""
        cap = int(self._scores.shape[1])
        if self._bound + rows > cap:
            self._bound = int(self.counts.max().item())                               # the one read-back: the bound is loose for segments
            if self._bound + rows > cap:
                scores, tps = self._alloc(max(2 * cap, self._bound + rows))
                if self._bound:
                    scores[:, :self._bound].copy_(self._scores[:, :self._bound])
                    tps[:, :self._bound].copy_(self._tps[:, :self._bound])
                self._scores, self._tps, self._sort_bufs = scores, tps, None
        self._bound += rows

    def ground_truth(self, labels):
        """labels (a SegLabels, or the dense pair (labels (B, C, TL) fp32, valid_t (B,))) -> (seg, offsets, fps, window, t_max) on the device"""
        return ground_truth(labels, self.device)

    @property
    def n_levels(self):
        """K of `levels` (1 without)"""
        if self.levels is None:
            return 1
        return int(self.levels.shape[1]) if torch.is_tensor(self.levels) else len(self.levels)

    def add(self, det, labels, want_match=False, out=None, tl=None, levels=1):
        """det: the Detections of a batch on the meter's device; labels: see ground_truth().  Returns (tp, match or None) of the batch on
        the device.  out: (tp (cap,) uint8, match (n_thr, cap) int32 or None, workspace) as ops.segap_match takes them.  tl: the frames
        the detections were decoded over (growing mode's bound; default: the labels' t_max).  levels: K when det are proposals decoded at K
        levels (growing mode's bound times K)."""
        from . import ops
        if not isinstance(det, Detections):
            raise TypeError('SegmentAPMeter.add: a cfn_hip.detections.Detections expected, got %s' % type(det).__name__)
        if int(det.n_classes) != self.n_classes:
            raise RuntimeError('SegmentAPMeter.add: detections over %d classes, the meter holds %d' % (det.n_classes, self.n_classes))
        seg, offsets, fps, window, t_max = self.ground_truth(labels)
        B = det.batch
        if int(offsets.numel()) != B + 1:
            raise RuntimeError('SegmentAPMeter.add: detections of %d videos against labels of %d' % (B, int(offsets.numel()) - 1))
        dseg, dscore = det.seg, det.score
        if int(dseg.shape[0]) != int(det.cap):                                        # (out= buffers may be longer than the decode's cap)
            dseg, dscore = dseg[:det.cap], dscore[:det.cap]
        if int(levels) < 1:
            raise ValueError('SegmentAPMeter.add: levels >= 1 expected, got %r' % (levels,))
        if self.capacity is None:
            self._reserve(min(B * int(levels) * ((max(int(t_max if tl is None else tl), 1) + 1) // 2), int(det.cap)))
        tp, match, ws = ops.segap_match(dseg, dscore, det.offsets, seg, offsets, fps, window, self._tiou, self.n_classes, t_max, self.score_col,
                                        want_match, out)
        ops.segap_append(dscore, tp, ws, self._scores, self._tps, self.counts, self.n_gt, self.flags, B, self.score_col)
        return tp, match

    @property
    def settings(self):
        """what two meters must share for their rows to be one metric's"""
        return self.n_classes, self.tiou, self.score

    def _part(self):
        """this meter's store as apmerge.stack_parts takes it, and the host's upper bound of its fullest class"""
        cap = int(self._scores.shape[1])
        return (self._scores, self._tps, self.counts, self.n_gt, self.flags), (min(self._bound, cap) if self.capacity is None else cap)

    def merge(self, *others):
        """append the rows of `others` (SegmentAPMeters of the same classes, tiou and score, on any GPU) behind this meter's, in the order
        given, in place: ONE ops.ap_merge with R = len(others) (rules M1-M4 of cfn_hip/apmerge.py).  The meter is then, bit for bit, what
        it would be had it been fed its own batches and then the others', one after another.  The others stay untouched.  Growing mode
        reserves from the host's bounds, which stay upper bounds (the one read-back of add()'s reserve where they pass the capacity); a
        fixed capacity never reads back: a merge that does not fit changes nothing, is flagged on the device and reported by value()."""
        from . import apmerge, ops
        for o in others:
            if not isinstance(o, SegmentAPMeter) or o.settings != self.settings:
                raise ValueError('SegmentAPMeter.merge: a SegmentAPMeter of the same classes, tiou and score expected, got %r against %r'
                                 % (getattr(o, 'settings', type(o).__name__), self.settings))
            if o is self:
                raise ValueError('SegmentAPMeter.merge: a meter cannot be merged into itself (sources and destination must not overlap)')
        if not others:
            return self
        parts, bounds = zip(*(o._part() for o in others))
        parts = [tuple(t.to(self.device) for t in p) for p in parts]
        if self.capacity is None:
            self._reserve(sum(bounds))
        # (one part goes as its own stores, whole: no copy, and the tiles behind its counts exit; several are stacked at the largest host bound)
        src = apmerge.stack_parts(parts, m=int(parts[0][0].shape[1]) if len(parts) == 1 else max(bounds))
        ops.ap_merge(self._scores, self._tps, self.counts, self.n_gt, self.flags, *src)
        return self

    @classmethod
    def merged(cls, parts, capacity=None):
        """a NEW meter (parts[0]'s settings and device; growing, or of the fixed `capacity`) that holds the parts' rows in list order, through
        ONE ops.ap_merge with R = len(parts): the code path the gather over ranks takes behind its collectives"""
        parts = list(parts)
        if not parts:
            raise ValueError('SegmentAPMeter.merged: at least one meter expected')
        p = parts[0]
        new = cls(p.device, p.n_classes, p.tiou, p.score, capacity, p.thr, p.max_gap, p.min_len, p.levels, p.nms if p.levels is not None else None,
                  p.nms_score, p.soft, filter=p.filter)
        return new.merge(*parts)

    def _across(self):
        from . import apmerge
        return self.across_ranks and apmerge.world_size(self.group) > 1

    def _evaluate(self):
        """(ap, map, flags) on the device: of this meter's rows, or -- across_ranks under a world size above 1 -- of all ranks' rows in rank
        order (apmerge.gather_stores: a collective; this rank's stores stay untouched)"""
        from . import apmerge, ops
        C, n_thr = self.n_classes, len(self.tiou)
        if self._across():
            scores, tps, state = apmerge.gather_stores(self._scores, self._tps, self._state, C, self.group)
            ap, mp = ops.segap_value(scores, tps, state[:C], state[C:2 * C], n_thr)
            return ap, mp, state[2 * C:]
        if self._sort_bufs is None:
            C, cap = self._scores.shape
            self._sort_bufs = (torch.empty_like(self._scores), torch.empty_like(self._tps), torch.empty(C, cap, dtype=torch.int32, device=self.device),
                               torch.empty_like(self._tps))
        out = self._sort_bufs + (torch.empty(len(self.tiou), self.n_classes, dtype=torch.float32, device=self.device),
                                 torch.empty(len(self.tiou), dtype=torch.float32, device=self.device))
        ap, mp = ops.segap_value(self._scores, self._tps, self.counts, self.n_gt, len(self.tiou), out=out)
        return ap, mp, self.flags

    def value_device(self):
        """(ap (n_thr, C) fp32, map (n_thr,) fp32) on the device; reads nothing back (the flags are not looked at: value() does).  With
        across_ranks under a world size above 1: of all ranks' rows in rank order, the same bits on every rank -- a COLLECTIVE that every
        rank must make (and the one read-back of two ints that sizes the gather)."""
        return self._evaluate()[:2]

    def value(self):
        """(ap (n_thr, C), map (n_thr,)) as float32 CPU tensors, with ONE read-back; raises if a batch did not fit a fixed capacity (on any
        rank, with across_ranks) or a merge met a malformed source"""
        from . import ops
        ap, mp, flags = self._evaluate()
        host = torch.cat([ap.reshape(-1).view(torch.int32), mp.view(torch.int32), flags]).cpu()
        if int(host[-1]) & ops.AP_FLAG_BAD_SOURCE:
            raise RuntimeError('SegmentAPMeter: a merge met a source store whose count was outside [0, capacity] (a malformed source) and was '
                               'refused: the value would miss those rows')
        if int(host[-1]) & ops.SEGAP_FLAG_OVERFLOW:
            if self.capacity is None:
                raise RuntimeError('SegmentAPMeter: a batch held more detections of one class than the growing stores had reserved (%d rows per '
                                   'class now) and was dropped: its detections were decoded over more frames than its labels\' t_max; pass '
                                   'add(tl=TL) with the TL of the decoded probs' % self._scores.shape[1])
            raise RuntimeError('SegmentAPMeter: a batch did not fit the fixed capacity of %d rows per class and was dropped' % self._scores.shape[1])
        n = ap.numel()
        return host[:n].view(torch.float32).reshape(ap.shape).clone(), host[n:-1].view(torch.float32).clone()
