"""Activity segments from per-frame scores: ``probs (B, C, TL)`` -> a compact, canonical, device-resident list of detections
[class, start second, end second, score] per video, in the record layout of ``SegLabels`` (cfn_hip.ops.decode_segments,
csrc/detections.hip).

The reference stops at the per-frame probabilities (train_fine.py:199-206); every caller who wants detections writes a threshold and a
run-finding loop in Python, each with its own rule for where a segment begins and ends.  This is the one rule, the inverse of
cfn_hip/seglabels.py.  Inputs ``probs (B, C, TL)`` fp32, ``valid_t (B,)`` int32, ``fps (B,)`` fp64, ``start (B,)`` int32 (the first frame of
each window, ``SegLabels.window[:, 0]``), ``thr (C,)`` fp32, host ints ``max_gap >= 0`` and ``min_len >= 1``:

    1. frame t of row (b, c) is ACTIVE iff  t < min(valid_t[b], TL)  and  probs[b, c, t] > thr[c]  -- an fp32 comparison, strict, so a NaN
       is never active
    2. gap closing: two active frames t < u are joined when every frame between them is inactive and  u - t - 1 <= max_gap;  the frames
       between them then belong to the run
    3. a SEGMENT is a maximal run [t0, t1] (inclusive, window relative) after 2; both ends are active frames; runs with
       t1 - t0 + 1 < min_len  are dropped
    4. start_s = (float64(start[b] + t0) - 0.5) / fps[b],   end_s = (float64(start[b] + t1) + 0.5) / fps[b]:  one fp64 add and one IEEE
       fp64 division each.  The half frame outward is what makes seg_labels, whose inequalities are strict, accept exactly t0..t1 again
    5. scores over the ACTIVE frames of the run only (a closed gap contributes nothing, so a NaN or a masked frame never reaches a score):
       score_max = the fp32 maximum;  score_mean = the fp64 sum of the active fp32 values in a fixed order, divided in fp64 by their
       count, rounded to fp32;  n_active = that count
    6. the output order is lexicographic in (b, c, t0), from counts and prefix sums: bit-identical from run to run

Outputs (``Detections``): ``seg (cap, 3)`` fp64 rows [class, start_s, end_s] (the layout of ``SegLabels.seg``), ``frames (cap, 3)`` int32
[t0, t1, n_active], ``score (cap, 2)`` fp32 [max, mean], ``offsets (B + 1,)`` int32 (sample b owns rows offsets[b]:offsets[b + 1]; true
counts, not clamped by cap), ``total (1,)`` int32 = offsets[B].  Rows >= cap are not written; the default cap
B * C * ((TL + 1) // 2) is the worst case.

``decode_reference`` spells the six rules in numpy on any device and is the tests' reference; ``decode`` is the one call that needs the GPU
library.  Limits: B <= 65535, C < 2^19, TL <= 65536, B * C * TL < 2^31; the 'loc' task only; no CPU path for the operator.

PROPOSALS (``decode_levels`` -> ``nms``, or ``propose`` for both; cfn_hip.ops.decode_segments_levels / nms_segments, csrc/detections.hip and
csrc/segnms.hip).  ``decode`` thresholds a class at ONE value, so a (video, class) group never overlaps itself and every activity gets one
candidate whose boundaries that value fixes.  The usual way from per-frame scores to ranked segments groups the frames at several thresholds
("levels": tight segments from high levels, long ones from low levels) and removes near-duplicates by non-maximum suppression over temporal IoU.
The rules, stated once (the kernels, the numpy references and include/cfn_hip.h spell the same):

  Level decode.  The inputs of ``decode``, but ``levels (C, K)`` fp32, 1 <= K <= 16, in place of ``thr``: row c holds class c's K thresholds in
  the order the caller gives them, which need not be sorted.

    L1. candidate row (b, c, k) is rules 1-5 above applied to probs[b, c, :] with the threshold levels[c, k]: the same valid_t, max_gap,
        min_len, half-frame-outward fp64 times, scores over active frames only
    L2. the class column of ``seg`` holds c; a separate ``level (cap,)`` uint8 holds k
    L3. the output order is lexicographic in (b, c, k, t0), from counts and prefix sums; offsets and total are true counts, rows >= cap are
        not written
    L4. the worst-case cap is B * C * K * ((TL + 1) // 2); K = 1 gives ``decode``'s result bit for bit

  So the candidates of a (video, class) group are contiguous and the class column does not decrease inside a video: all segap_match needs, and
  a candidate list is a valid ``Detections`` for the meter.

  NMS.  A ``Detections`` whose rows are grouped like that, a host float ``nms_thr`` of [0, 1] and ``score_col`` (0 = max, 1 = mean).

    N1. groups are (video, class) row ranges, found as segap_match finds them
    N2. the order inside a group: score[:, score_col] descending (fp32), ties by row index ascending (cfn_hip/segap.py rule 3; a NaN score,
        which a decode never gives, ranks as -inf).  NESTED CANDIDATES SHARE THEIR MAXIMUM, so under score='max' the caller's LEVEL ORDER
        decides those ties: levels listed high to low put the tight segment first, low to high the long one
    N3. tIoU is cfn_hip/segap.py rule 2 (``tiou_reference``) on the seg columns: plain fp64, one division, no product, 0 unless inter > 0
    N4. greedy: walk the group in the order of N2; a candidate is KEPT iff no candidate KEPT BEFORE IT has tIoU with it strictly above
        nms_thr.  A suppressed candidate suppresses nothing
    N5. the output is a stable compaction: kept rows in their input order, seg / frames / score copied bit for bit; offsets and total are
        recomputed as true counts; rows >= cap_out are not written
    N6. two further outputs: ``keep (cap_in,)`` uint8 (written for the rows of the batch's groups) and ``src (cap_out,)`` int32 = the input
        row of each output row; ``level`` can be gathered through src
    N7. nms_thr = 1 keeps everything; with nms_thr < 1 exact duplicates across levels have tIoU exactly 1.0 and collapse to the first copy; a
        single-level decode passes through unchanged for any nms_thr, because its candidates do not overlap

  SOFT-NMS (``soft_nms``, or ``propose(soft=SoftNMS(...))``; cfn_hip.ops.soft_nms_segments, csrc/segnms.hip).  Hard NMS deletes a candidate
  whose tIoU with a kept one is above ``nms_thr``, so the ranked list is cut at a threshold the user has to guess.  Soft-NMS deletes nothing
  by overlap: a candidate's score is decayed by its overlap with every candidate ranked in front of it, and the list is cut by a score floor
  or a count.  The same ``Detections`` in and out, and the host parameters ``score_col``; ``method`` (0 = linear, 1 = gaussian); ``nms_thr``,
  a double of [0, 1], linear only; ``sigma``, a double of [1/64, 2^20], gaussian only; ``min_score``, a double of [0, 1]; ``max_keep``, an
  int >= 0 (0 = no limit):

    S1. groups are rule N1's (video, class) row ranges
    S2. row i gets the working score w_i = float64(score[i, score_col]); a row whose score is NaN or infinite is out of the group from the
        start: never selected, never decayed, keep 0
    S3. rounds: among the rows not yet selected take the largest w, on a tie the lowest row: m.  Stop when no row is left, when
        not (w_m >= min_score), or when max_keep > 0 and max_keep rows are selected; otherwise m is selected and final_m = w_m.  Selected
        finals never increase, so the selected set is exactly the rows whose final score is at least min_score, cut at max_keep
    S4. decay of every row j not yet selected, iou = tIoU(m, j) by rule N3 unchanged.  linear: if iou > nms_thr (strict),
        w_j = w_j * (1.0 - iou).  gaussian: if iou > 0, w_j = w_j * E((iou * iou) / sigma).  One fp64 subtraction or one E, then one fp64
        product; the decays are applied in selection order
    S5. E(t) = exp(-t) for t in [0, 64], written out so that both sides compute the same double (the device's exp and libm's differ in the
        last bits): y = -(t * 2^-10); p = c8, then p = p * y + c_k for k = 7 .. 0 with c_k = 1.0 / k! as one IEEE fp64 division; then
        p = p * p ten times.  Every product and sum is rounded separately, no fused multiply-add; fp64 subnormals follow IEEE
        (``decay_exp_reference``: within 1.6e-13 relative of exp(-t), E(0) == 1.0 exactly)
    S6. the output is a stable compaction of the selected rows in input order: seg, frames and the other score column copied bit for bit,
        score[:, score_col] = float32(final), round to nearest; offsets and total are true counts; rows >= cap_out are not written; keep
        and src as in N6
    S7. linear with nms_thr = 1, min_score = 0, max_keep = 0 returns its input bit for bit; a single-level decode passes through either
        method unchanged when min_score is not above its scores; max_keep = 1 leaves each group's first row in the order of N2; the first
        selected row of every group is hard NMS's first kept row

SMOOTHING (``filter=``; cfn_hip/scorefilter.py states the rule, F1-F6).  ``decode``, ``decode_levels``, ``propose`` and ``DetectionWriter``
take ``filter=`` -- a ``cfn_hip.scorefilter.ScoreFilter`` (box, Gaussian or median over a per-class window) -- and so do ``decode_reference``
and ``decode_levels_reference``: probs goes through the filter ONCE (one more launch; the references through ``filter_reference``), and
everything behind it, the score columns included, reads the filtered tensor.  With None nothing changes, bit for bit.

``decode_levels_reference``, ``nms_reference`` and ``soft_nms_reference`` spell these in numpy on any device and are the tests' reference.
Limits: K <= 16, B * C * K * TL < 2^31; NMS: B and C <= 65535, ranking is O(nd^2) and suppression O(kept * nd) per group of nd candidates;
soft-NMS is O(selected * nd) per group, which max_keep bounds.  No accuracy gain is claimed: which levels, which nms_thr, and whether hard or
soft NMS help a trained model is for the user to find with the meter.  Out of scope: NMS across classes.

This module is host only (numpy + torch) apart from those calls.
"""
import collections
import json
import os

import numpy as np
import torch

from .seglabels import SegLabels


class Detections(collections.namedtuple('Detections', ['seg', 'frames', 'score', 'offsets', 'total', 'n_classes', 'cap'])):
    """The decoded segments of a batch (see the module text): five tensors on one device and the HOST ints ``n_classes`` and ``cap`` (rows of
    the three record buffers the decode was allowed to write).  A namedtuple, like SegLabels."""
    __slots__ = ()

    @property
    def device(self):
        return self.seg.device

    @property
    def batch(self):
        return int(self.offsets.shape[0]) - 1

    def to(self, device, non_blocking=False):
        """move the five tensors to `device`; the element types are part of the format, so a dtype is refused"""
        if isinstance(device, torch.dtype) or not isinstance(device, (str, int, torch.device)):
            raise TypeError('Detections.to() takes a device: seg stays float64, frames, offsets and total int32, score float32')
        return Detections(*[t.to(device, non_blocking=non_blocking) for t in self[:5]], self.n_classes, self.cap)

    def check(self):
        """ONE read of `total`: the number of segments; raises if the decode found more than `cap` rows could hold"""
        total = int(self.total.item())
        if total > self.cap:
            raise RuntimeError('Detections: the decode found %d segments but cap = %d rows were allowed: rows behind cap were not written '
                               '(decode again with a larger cap; the default cannot overflow)' % (total, self.cap))
        return total

    def _read(self):
        """ONE read-back: (offsets list, seg, frames, score as numpy over the first min(total, cap) rows); raises like check()"""
        n = min(self.cap, int(self.seg.shape[0]))
        parts = [t[:n].contiguous().view(torch.uint8).reshape(-1) for t in self[:3]] + [self.offsets.contiguous().view(torch.uint8).reshape(-1)]
        host = torch.cat(parts).cpu().numpy()                                     # (the fp64 rows first: every part starts aligned)
        cuts = np.cumsum([0, 24 * n, 12 * n, 8 * n, 4 * (self.batch + 1)])
        offs = host[cuts[3]:cuts[4]].view(np.int32)
        k = int(offs[-1])
        if k > self.cap:
            raise RuntimeError('Detections: the decode found %d segments but cap = %d rows were allowed: rows behind cap were not written '
                               '(decode again with a larger cap; the default cannot overflow)' % (k, self.cap))
        return (offs.tolist(), host[cuts[0]:cuts[1]].view(np.float64).reshape(n, 3)[:k], host[cuts[1]:cuts[2]].view(np.int32).reshape(n, 3)[:k],
                host[cuts[2]:cuts[3]].view(np.float32).reshape(n, 2)[:k])

    def tolist(self, names=None):
        """ONE read-back -> per video a list of dicts  class, start, end, t0, t1, score_max, score_mean  in the decode's order (class, then
        t0).  names: class names by index; the class is its integer otherwise.  Raises if the decode overflowed `cap`."""
        offs, seg, frames, score = self._read()
        out = []
        for b in range(self.batch):
            rows = []
            for i in range(offs[b], offs[b + 1]):
                c = int(seg[i, 0])
                rows.append({'class': names[c] if names is not None else c, 'start': float(seg[i, 1]), 'end': float(seg[i, 2]),
                             't0': int(frames[i, 0]), 't1': int(frames[i, 1]), 'score_max': float(score[i, 0]), 'score_mean': float(score[i, 1])})
            out.append(rows)
        return out

    def as_seg_labels(self, fps, window, t_max):
        """a SegLabels batch over the SAME seg / offsets tensors (no copy): its dense() rasterises the detections, and gives back exactly
        the frames t0..t1 of every segment when fps and window[:, 0] are the decode's fps and start.  Needs total <= cap (check())."""
        return SegLabels(self.seg, self.offsets, fps, window, self.n_classes, int(t_max))


def _defaults(probs, fps, start):
    B = int(probs.shape[0])
    if fps is None:
        fps = torch.ones(B, dtype=torch.float64, device=probs.device)
    if start is None:
        start = torch.zeros(B, dtype=torch.int32, device=probs.device)
    return fps, start


def _filtered(probs, valid_t, filter, reference=False):
    """probs through `filter` (a cfn_hip.scorefilter.ScoreFilter; None: probs itself): one launch, or filter_reference on the host"""
    if filter is None:
        return probs
    from . import scorefilter
    return scorefilter.filter_reference(probs, valid_t, filter) if reference else scorefilter.apply(probs, valid_t, filter)


def decode(probs, valid_t, fps=None, start=None, thr=0.5, max_gap=0, min_len=1, cap=None, out=None, filter=None):
    """probs (B, C, TL) fp32 and valid_t (B,) int32 on the GPU -> Detections there (ops.decode_segments: three launches, nothing is read
    back).  fps=None: fps = 1 (and start=None: start = 0), so times are in frames, still with the half frame outward.  thr: a float or a
    (C,) fp32 device tensor.  cap, out: see ops.decode_segments.  filter: a ScoreFilter -- probs is smoothed first (one more launch, into a
    new tensor; for a call that allocates nothing, hand decode the result of cfn_hip.scorefilter.apply(out=) instead)."""
    from . import ops
    probs = _filtered(probs, valid_t, filter)
    fps, start = _defaults(probs, fps, start)
    C = int(probs.shape[1]) if probs.dim() == 3 else 0
    if cap is None and probs.dim() == 3:
        cap = ops.decode_segments_cap(*probs.shape)
    seg, frames, score, offsets, total = ops.decode_segments(probs, valid_t, fps, start, thr, max_gap, min_len, cap, out)
    return Detections(seg, frames, score, offsets, total, C, int(cap))


def decode_reference(probs, valid_t, fps=None, start=None, thr=0.5, max_gap=0, min_len=1, cap=None, filter=None):
    """decode() from the definition, rule by rule, in numpy; tensors on any device, the result on probs' device: the tests' reference and
    the CPU spelling.  cap=None: exactly the rows found (at least one, as SegLabels.seg is never empty); a cap keeps the first `cap` rows and
    the true offsets / total, as the kernel does.  filter: probs goes through cfn_hip.scorefilter.filter_reference first."""
    dev = probs.device
    probs = _filtered(probs, valid_t, filter, reference=True)
    fps, start = _defaults(probs, fps, start)
    p = probs.detach().cpu().numpy()
    if p.dtype != np.float32 or p.ndim != 3:
        raise ValueError('probs: a (B, C, TL) float32 tensor expected, got %s %s' % (p.dtype, p.shape))
    B, C, TL = p.shape
    max_gap, min_len = int(max_gap), int(min_len)
    if max_gap < 0 or min_len < 1:
        raise ValueError('max_gap >= 0 and min_len >= 1 expected, got %d and %d' % (max_gap, min_len))
    th = np.full(C, thr, np.float32) if not torch.is_tensor(thr) else thr.detach().cpu().numpy().astype(np.float32).reshape(C)
    valid = valid_t.detach().cpu().numpy().astype(np.int64)
    f64, first = fps.detach().cpu().numpy().astype(np.float64), start.detach().cpu().numpy().astype(np.int64)
    seg, frames, score, offsets = [], [], [], [0]
    for b in range(B):
        n = min(max(int(valid[b]), 0), TL)
        with np.errstate(invalid='ignore'):
            active = p[b, :, :n] > th[:, None]                                        # rule 1 (fp32, strict; NaN > x is False)
        for c in np.flatnonzero(active.any(1)):
            on = np.flatnonzero(active[c])
            cut = np.flatnonzero(np.diff(on) - 1 > max_gap)                           # rule 2: a run ends where the gap is too long
            lo, hi = np.concatenate([[0], cut + 1]), np.concatenate([cut + 1, [on.size]])
            for i, j in zip(lo, hi):                                                  # rule 3: on[i:j] are the run's active frames
                t0, t1 = int(on[i]), int(on[j - 1])
                if t1 - t0 + 1 < min_len:
                    continue
                vals = p[b, c, on[i:j]]                                               # rule 5: active frames only
                with np.errstate(all='ignore'):
                    mean = np.float32(np.sum(vals.astype(np.float64)) / np.float64(j - i))
                seg.append([float(c), (np.float64(first[b] + t0) - 0.5) / f64[b], (np.float64(first[b] + t1) + 0.5) / f64[b]])      # rule 4
                frames.append([t0, t1, int(j - i)])
                score.append([vals.max(), mean])
        offsets.append(len(seg))                                                      # rule 6: appended in (b, c, t0) order
    total = len(seg)
    keep = max(total, 1) if cap is None else int(cap)
    if keep < 1:
        raise ValueError('cap >= 1 expected, got %d' % keep)
    out_seg, out_frames, out_score = np.zeros((keep, 3), np.float64), np.zeros((keep, 3), np.int32), np.zeros((keep, 2), np.float32)
    k = min(total, keep)
    if k:
        out_seg[:k], out_frames[:k], out_score[:k] = np.asarray(seg, np.float64)[:k], np.asarray(frames, np.int32)[:k], np.asarray(score, np.float32)[:k]
    return Detections(torch.from_numpy(out_seg).to(dev), torch.from_numpy(out_frames).to(dev), torch.from_numpy(out_score).to(dev),
                      torch.tensor(offsets, dtype=torch.int32, device=dev), torch.tensor([total], dtype=torch.int32, device=dev), int(C), keep)


SCORE_COLUMNS = {'max': 0, 'mean': 1}


def _score_col(score):
    if score not in SCORE_COLUMNS:
        raise ValueError("score: 'max' or 'mean' expected, got %r" % (score,))
    return SCORE_COLUMNS[score]


def levels_tensor(levels, n_classes, device=None):
    """levels: a sequence of 1 to 16 floats (every class the same, in that order) or a (C, K) tensor -> a contiguous (C, K) fp32 tensor"""
    C = int(n_classes)
    if torch.is_tensor(levels):
        t = levels.detach().to(torch.float32)
        if t.dim() != 2 or int(t.shape[0]) != C or not 1 <= int(t.shape[1]) <= 16:
            raise ValueError('levels: 1 to 16 floats or a (%d, K) tensor with K <= 16 expected, got %s' % (C, tuple(levels.shape)))
    else:
        vals = [float(x) for x in levels]
        if not 1 <= len(vals) <= 16:
            raise ValueError('levels: 1 to 16 floats or a (%d, K) tensor with K <= 16 expected, got %r' % (C, levels))
        t = torch.tensor(vals, dtype=torch.float32).repeat(C, 1)
    return (t if device is None else t.to(device)).contiguous()


def decode_levels(probs, valid_t, fps=None, start=None, levels=(0.5,), max_gap=0, min_len=1, cap=None, out=None, filter=None):
    """probs (B, C, TL) fp32 and valid_t (B,) int32 on the GPU -> (Detections of the candidates at every level, level (cap,) uint8) there (rules
    L1-L4; ops.decode_segments_levels: three launches, nothing is read back).  levels: floats (every class) or a (C, K) fp32 tensor; fps, start
    as decode().  cap, out: see ops.decode_segments_levels (with out=, hand a (C, K) device tensor for nothing to be allocated).  filter:
    as decode()."""
    from . import ops
    probs = _filtered(probs, valid_t, filter)
    fps, start = _defaults(probs, fps, start)
    C = int(probs.shape[1]) if probs.dim() == 3 else 0
    if not (torch.is_tensor(levels) and levels.dtype == torch.float32 and levels.dim() == 2 and levels.device == probs.device and levels.is_contiguous()):
        levels = levels_tensor(levels, C, probs.device)
    if cap is None and probs.dim() == 3:
        cap = ops.decode_segments_levels_cap(probs.shape[0], C, levels.shape[1], probs.shape[2])
    seg, frames, score, level, offsets, total = ops.decode_segments_levels(probs, valid_t, fps, start, levels, max_gap, min_len, cap, out)
    return Detections(seg, frames, score, offsets, total, C, int(cap)), level


def decode_levels_reference(probs, valid_t, fps=None, start=None, levels=(0.5,), max_gap=0, min_len=1, cap=None, filter=None):
    """decode_levels() from rules L1-L4 in numpy: K decode_reference calls (one per level column), merged in (b, c, k, t0) order; tensors on
    any device, the result on probs' device.  cap as in decode_reference.  filter: as decode_reference, applied once in front of the K calls."""
    dev = probs.device
    probs = _filtered(probs, valid_t, filter, reference=True)
    B, C = int(probs.shape[0]), int(probs.shape[1])
    lv = levels_tensor(levels, C).cpu()
    K = int(lv.shape[1])
    parts = [decode_reference(probs.detach().cpu(), valid_t.cpu(), None if fps is None else fps.cpu(), None if start is None else start.cpu(),
                              lv[:, k].contiguous(), max_gap, min_len) for k in range(K)]
    rows = []                                                                         # (b, c, k, t0) -> (k, row of part k)
    for k, d in enumerate(parts):
        offs = d.offsets.tolist()
        for b in range(B):
            for i in range(offs[b], offs[b + 1]):
                rows.append((b, int(d.seg[i, 0]), k, int(d.frames[i, 0]), i))
    rows.sort()
    total = len(rows)
    keep = max(total, 1) if cap is None else int(cap)
    if keep < 1:
        raise ValueError('cap >= 1 expected, got %d' % keep)
    seg, frames, score = torch.zeros(keep, 3, dtype=torch.float64), torch.zeros(keep, 3, dtype=torch.int32), torch.zeros(keep, 2, dtype=torch.float32)
    level = torch.zeros(keep, dtype=torch.uint8)
    n = min(total, keep)
    if n:
        first = np.cumsum([0] + [int(d.seg.shape[0]) for d in parts])                 # the parts' rows behind one another
        pick = torch.tensor([first[k] + i for _, _, k, _, i in rows[:n]], dtype=torch.int64)
        seg[:n], frames[:n], score[:n] = (torch.cat([d[j] for d in parts])[pick] for j in range(3))
        level[:n] = torch.tensor([k for _, _, k, _, _ in rows[:n]], dtype=torch.uint8)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(np.asarray([r[0] for r in rows], np.int64), minlength=B))]).astype(np.int64).tolist()
    return (Detections(seg.to(dev), frames.to(dev), score.to(dev), torch.tensor(offsets, dtype=torch.int32, device=dev),
                       torch.tensor([total], dtype=torch.int32, device=dev), C, keep), level.to(dev))


def _rows(det):
    """a Detections' three record buffers cut to its cap (out= buffers may be longer than the decode's cap)"""
    if int(det.seg.shape[0]) == int(det.cap):
        return det.seg, det.frames, det.score
    return det.seg[:det.cap], det.frames[:det.cap], det.score[:det.cap]


def nms(det, nms_thr, score='max', cap=None, out=None):
    """Temporal NMS of a Detections on the GPU -> (the kept Detections, keep (cap_in,) uint8, src (cap,) int32) there (rules N1-N7;
    ops.nms_segments: three launches, nothing is read back).  cap (default: det.cap, which cannot overflow) and out: see ops.nms_segments."""
    from . import ops
    if not isinstance(det, Detections):
        raise TypeError('nms: a cfn_hip.detections.Detections expected, got %s' % type(det).__name__)
    seg, frames, score_t = _rows(det)
    cap = int(det.cap) if cap is None else int(cap)
    seg_o, frames_o, score_o, offsets, total, keep, src = ops.nms_segments(seg, frames, score_t, det.offsets, det.n_classes, nms_thr, _score_col(score),
                                                                            cap, out)
    return Detections(seg_o, frames_o, score_o, offsets, total, det.n_classes, cap), keep, src


def _ranges(det):
    """a Detections' offsets clamped to the rows it holds, as the kernels clamp them -> (rows covered by offsets[-1], [(lo, hi) per video])"""
    offs = det.offsets.detach().cpu().numpy().astype(np.int64)
    cap_in = min(int(det.cap), int(det.seg.shape[0]))
    offs = [min(max(int(o), 0), cap_in) for o in offs]
    return offs[-1], list(zip(offs[:-1], offs[1:]))


def _groups(det, seg):
    """rule N1 on the host: the row indices of every (video, class) group of `det` (seg: its seg as numpy), videos in order, classes ascending"""
    for lo, hi in _ranges(det)[1]:
        for c in np.unique(seg[lo:hi, 0]):
            yield lo + np.flatnonzero(seg[lo:hi, 0] == c)


def _compacted(det, keep, sc, cap):
    """rules N5 / N6 (S6) on the host: keep over det's input rows and the score rows to copy -> (the stable compaction as a Detections,
    keep, src) on det's device.  cap=None: exactly the kept rows (at least one)."""
    dev = det.seg.device
    seg, frames = (t.detach().cpu().numpy() for t in det[:2])
    new_offs = [0] + [int(keep[:hi].sum()) for _, hi in _ranges(det)[1]]
    src = np.flatnonzero(keep).astype(np.int32)                                       # input order
    total = int(src.size)
    rows_out = max(total, 1) if cap is None else int(cap)
    if rows_out < 1:
        raise ValueError('cap >= 1 expected, got %d' % rows_out)
    k = min(total, rows_out)
    o_seg, o_frames, o_score = np.zeros((rows_out, 3), np.float64), np.zeros((rows_out, 3), np.int32), np.zeros((rows_out, 2), np.float32)
    o_src = np.zeros(rows_out, np.int32)
    o_seg[:k], o_frames[:k], o_score[:k], o_src[:k] = seg[src[:k]], frames[src[:k]], sc[src[:k]], src[:k]
    out = Detections(torch.from_numpy(o_seg).to(dev), torch.from_numpy(o_frames).to(dev), torch.from_numpy(o_score).to(dev),
                     torch.tensor(new_offs, dtype=torch.int32, device=dev), torch.tensor([total], dtype=torch.int32, device=dev), det.n_classes, rows_out)
    return out, torch.from_numpy(keep).to(dev), torch.from_numpy(o_src).to(dev)


def nms_reference(det, nms_thr, score='max', cap=None):
    """nms() from rules N1-N7 in numpy; a Detections on any device, the results on its device.  cap=None: exactly the kept rows (at least
    one); a cap keeps the first `cap` kept rows and the true offsets / total, as the kernel does.  keep covers the min(total, cap_in) input
    rows; src the rows written."""
    from .segap import tiou_reference
    col = _score_col(score)
    nms_thr = float(nms_thr)
    if not 0.0 <= nms_thr <= 1.0:
        raise ValueError('nms_thr in [0, 1] expected, got %r' % (nms_thr,))
    seg, sc = det.seg.detach().cpu().numpy(), det.score.detach().cpu().numpy()
    keep = np.zeros(_ranges(det)[0], np.uint8)
    for rows in _groups(det, seg):                                                    # N1
        key = sc[rows, col].astype(np.float32)
        key = np.where(np.isnan(key), np.float32(-np.inf), key)
        order = rows[np.argsort(-key, kind='stable')]                                 # N2
        kept = []
        for d in order:                                                               # N4
            if not any(tiou_reference(seg[k, 1], seg[k, 2], seg[d, 1], seg[d, 2]) > nms_thr for k in kept):         # N3
                kept.append(d)
                keep[d] = 1
    return _compacted(det, keep, sc, cap)


SOFT_METHODS = {'linear': 0, 'gaussian': 1}
SoftNMS = collections.namedtuple('SoftNMS', 'method sigma min_score max_keep', defaults=('gaussian', 0.5, 0.001, 0))
SoftNMS.__doc__ = """The options of soft_nms (rules S1-S7): method 'linear' | 'gaussian', sigma in [1/64, 2^20] (gaussian), min_score in [0, 1] (the
score floor that cuts the list), max_keep >= 0 rows per (video, class) group (0: no limit).  linear's threshold is the nms_thr of the call."""


def _soft(soft, nms_thr, error=ValueError):
    """a SoftNMS (or a plain tuple of its four fields) and nms_thr, checked -> (SoftNMS with host numbers, nms_thr)"""
    if not isinstance(soft, tuple) or len(soft) != 4:
        raise TypeError('soft: a cfn_hip.detections.SoftNMS expected, got %s' % type(soft).__name__)
    method, sigma, min_score, max_keep = soft
    if method not in SOFT_METHODS:
        raise error("soft.method: 'linear' or 'gaussian' expected, got %r" % (method,))
    for name, v, lo, hi, text in (('soft.sigma', sigma, 1.0 / 64.0, float(1 << 20), '[1/64, 2^20]'), ('soft.min_score', min_score, 0.0, 1.0, '[0, 1]'),
                                  ('nms_thr', nms_thr, 0.0, 1.0, '[0, 1]')):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) <= hi:
            raise error('%s in %s expected, got %r' % (name, text, v))
    if isinstance(max_keep, bool) or not isinstance(max_keep, int) or not 0 <= max_keep < (1 << 31):
        raise error('soft.max_keep: an int >= 0 expected (0: no limit), got %r' % (max_keep,))
    return SoftNMS(method, float(sigma), float(min_score), max_keep), float(nms_thr)


def decay_exp_reference(t):
    """rule S5: E(t) = exp(-t) on [0, 64] in numpy float64 (a scalar or an array), every product and sum rounded separately -- the double the
    kernel computes.  Neither numpy's nor the device's exp is used: they differ in their last bits."""
    t = np.asarray(t, np.float64)
    with np.errstate(all='ignore'):
        y = -(t * np.float64(2.0 ** -10))
        fact = [np.float64(1.0)]
        for k in range(1, 9):
            fact.append(fact[-1] * np.float64(k))                                     # k! is exact in fp64
        p = np.float64(1.0) / fact[8] + np.zeros_like(y)
        for k in range(7, -1, -1):
            p = p * y + np.float64(1.0) / fact[k]
        for _ in range(10):
            p = p * p
    return p


def soft_nms(det, soft=SoftNMS(), nms_thr=0.5, score='max', cap=None, out=None):
    """Soft-NMS of a Detections on the GPU -> (the selected Detections, keep (cap_in,) uint8, src (cap,) int32) there (rules S1-S7;
    ops.soft_nms_segments: three launches, nothing is read back).  soft: a SoftNMS; nms_thr: linear's threshold (gaussian does not use it).
    The score column `score` of the result holds the final, decayed scores.  cap (default: det.cap, which cannot overflow) and out: see
    ops.soft_nms_segments."""
    from . import ops
    if not isinstance(det, Detections):
        raise TypeError('soft_nms: a cfn_hip.detections.Detections expected, got %s' % type(det).__name__)
    soft, nms_thr = _soft(soft, nms_thr)
    seg, frames, score_t = _rows(det)
    cap = int(det.cap) if cap is None else int(cap)
    seg_o, frames_o, score_o, offsets, total, keep, src = ops.soft_nms_segments(seg, frames, score_t, det.offsets, det.n_classes, SOFT_METHODS[soft.method],
                                                                                 soft.sigma, soft.min_score, soft.max_keep, nms_thr, _score_col(score),
                                                                                 cap, out)
    return Detections(seg_o, frames_o, score_o, offsets, total, det.n_classes, cap), keep, src


def soft_nms_reference(det, soft=SoftNMS(), nms_thr=0.5, score='max', cap=None):
    """soft_nms() from rules S1-S7 in numpy (a round is vectorised over the group: the elementwise fp64 operations give the same bits); a
    Detections on any device, the results on its device.  cap, keep and src as nms_reference gives them."""
    col = _score_col(score)
    soft, nms_thr = _soft(soft, nms_thr)
    gaussian, sigma, floor = soft.method == 'gaussian', np.float64(soft.sigma), np.float64(soft.min_score)
    seg, sc = det.seg.detach().cpu().numpy(), det.score.detach().cpu().numpy()
    n = _ranges(det)[0]
    keep = np.zeros(n, np.uint8)
    final = sc[:n].copy()
    for rows in _groups(det, seg):                                                    # S1
        s, e = seg[rows, 1], seg[rows, 2]
        w = sc[rows, col].astype(np.float64)                                          # S2: -inf marks a row that is out, or selected
        w = np.where(np.isfinite(w), w, -np.inf)
        selected = 0
        with np.errstate(all='ignore'):
            while True:                                                               # S3
                m = int(np.argmax(w))                                                 # (the first of equal maxima: the lowest row)
                wm = w[m]
                if wm == -np.inf or not wm >= floor or (soft.max_keep > 0 and selected >= soft.max_keep):
                    break
                keep[rows[m]], final[rows[m], col] = 1, np.float32(wm)
                selected += 1
                w[m] = -np.inf
                inter = np.where(e[m] < e, e[m], e) - np.where(s[m] > s, s[m], s)      # S4: tiou_reference's expression, elementwise
                iou = np.where(inter > 0.0, inter / ((e[m] - s[m]) + (e - s) - inter), 0.0)
                if gaussian:
                    hit = (iou > 0.0) & (w > -np.inf)
                    w[hit] = w[hit] * decay_exp_reference((iou[hit] * iou[hit]) / sigma)
                else:
                    hit = (iou > nms_thr) & (w > -np.inf)
                    w[hit] = w[hit] * (1.0 - iou[hit])
    return _compacted(det, keep, final, cap)                                          # S6


def propose(probs, valid_t, fps=None, start=None, levels=(0.8, 0.65, 0.5, 0.35, 0.2), nms_thr=0.5, score='max', max_gap=0, min_len=1, out=None,
            reference=False, soft=None, filter=None):
    """probs -> candidates at K levels -> NMS -> the post-NMS Detections, all on the device (six launches, nothing is read back).  Levels
    listed high to low prefer the tight segment among nested candidates under score='max' (rule N2).  out: (the out of decode_levels, the out
    of nms), both for the worst-case cap, for a call that allocates nothing (capturable).  reference=True: the numpy references instead.
    soft: a SoftNMS -- the second stage is soft_nms in place of nms (nms_thr is then linear's threshold; out[1] is the out of soft_nms).
    filter: a ScoreFilter -- probs is smoothed once in front of the level decode (one more launch; filter_reference with reference=True)."""
    probs = _filtered(probs, valid_t, filter, reference)
    if reference:
        cand, _ = decode_levels_reference(probs, valid_t, fps, start, levels, max_gap, min_len)
        return (nms_reference(cand, nms_thr, score) if soft is None else soft_nms_reference(cand, soft, nms_thr, score))[0]
    cand, _ = decode_levels(probs, valid_t, fps, start, levels, max_gap, min_len, out=None if out is None else out[0])
    if soft is not None:
        return soft_nms(cand, soft, nms_thr, score, out=None if out is None else out[1])[0]
    return nms(cand, nms_thr, score, out=None if out is None else out[1])[0]


def epoch_path(path, epoch):
    """'val/det.jsonl', 4 -> 'val/det.ep004.jsonl': the file of one validation phase"""
    root, ext = os.path.splitext(path)
    return '%s.ep%03d%s' % (root, int(epoch), ext)


class DetectionWriter(object):
    """Collects the detections of a validation phase and writes them as JSON lines, one object per video:

        {"video": name, "unit": "s" | "frame", "segments": [{"class", "start", "end", "t0", "t1", "score_max", "score_mean"}, ...]}

    add() decodes on the device and keeps the device tensors (nothing is read back, the host does not wait); take() / flush() read every
    kept batch back once.  ``unit`` is "s" when the batch's labels were a SegLabels (its fps and window give seconds) and "frame"
    otherwise (fps = 1, start = 0).  Every add() decodes with the worst-case cap, which cannot overflow, so a batch keeps
    B * C * ((TL + 1) // 2) * 44 bytes on the device: the kept tensors are read back early once they exceed `max_pending_bytes`.

    levels (floats or a (C, K) tensor), nms (a float of [0, 1], default 0.5), nms_score: with `levels` set add() runs propose() in place of
    decode() -- candidates at the K levels, then temporal NMS -- and keeps only the post-NMS batch (K times the rows); `thr` is then not
    used.  The JSON format is the same.  soft (a SoftNMS, with `levels`): the second stage of propose() is soft_nms -- `nms` is then linear's
    threshold and the score column `nms_score` of the file holds the final, decayed scores.  filter (a cfn_hip.scorefilter.ScoreFilter): every
    add() smooths its probs first (one more launch) and decodes the filtered scores; None changes nothing."""

    def __init__(self, path, thr=0.5, max_gap=0, min_len=1, max_pending_bytes=1 << 30, levels=None, nms=None, nms_score='max', soft=None, filter=None):
        self.path, self.thr, self.max_gap, self.min_len = path, thr, int(max_gap), int(min_len)
        if filter is not None:
            from .scorefilter import ScoreFilter
            if not isinstance(filter, ScoreFilter):
                raise TypeError('DetectionWriter: filter: a cfn_hip.scorefilter.ScoreFilter expected, got %s' % type(filter).__name__)
        self.filter = filter
        self.levels, self.nms, self.nms_score = levels, (0.5 if nms is None else float(nms)), nms_score
        if levels is None and nms is not None:
            raise ValueError('DetectionWriter: nms without levels: a single-level decode does not overlap itself (rule N7)')
        if levels is None and soft is not None:
            raise ValueError('DetectionWriter: soft without levels: a single-level decode does not overlap itself (rule S7)')
        _score_col(nms_score)
        self.soft = None if soft is None else _soft(soft, self.nms)[0]
        self._levels_dev = {}
        self.max_pending_bytes = int(max_pending_bytes)
        self._pending, self._pending_bytes, self._rows = [], 0, []
        self._thr_dev = {}

    def _thr(self, probs):
        """the threshold as a (C,) device tensor, made once per device and class count"""
        thr = self.thr
        if torch.is_tensor(thr) and not thr.is_cuda and probs.is_cuda:
            key = (probs.device, int(probs.shape[1]))
            if key not in self._thr_dev:
                self._thr_dev[key] = thr.to(probs.device, torch.float32).contiguous()
            thr = self._thr_dev[key]
        return thr

    @property
    def n_levels(self):
        """K, the candidates' levels per class (1 without `levels`): what SegmentAPMeter.add(levels=) takes"""
        if self.levels is None:
            return 1
        return int(self.levels.shape[1]) if torch.is_tensor(self.levels) else len(self.levels)

    def _levels(self, probs):
        """the levels as a (C, K) device tensor, made once per device and class count"""
        key = (probs.device, int(probs.shape[1]))
        if key not in self._levels_dev:
            self._levels_dev[key] = levels_tensor(self.levels, key[1], probs.device)
        return self._levels_dev[key]

    def add(self, probs, valid_t, labels, names, decoder=None):
        """probs (B, C, TL) fp32 and valid_t (B,) of one batch, its label member BEFORE it was made dense (a SegLabels batch gives fps and
        window; anything else, or None, gives frame units) and the B video names.  decoder: decode (the device, default) or
        decode_reference."""
        names = list(names)
        if len(names) != int(probs.shape[0]):
            raise ValueError('DetectionWriter.add: %d video names for a batch of %d' % (len(names), int(probs.shape[0])))
        fps = start = None
        unit = 'frame'
        if isinstance(labels, SegLabels):
            labels = labels.to(probs.device)
            fps, start, unit = labels.fps, labels.window[:, 0].contiguous(), 's'
        more = {} if self.filter is None else {'filter': self.filter}
        if self.levels is not None:             # decoder: propose's `reference` switch (decode_reference: the numpy references)
            det = propose(probs.detach(), valid_t.to(torch.int32), fps, start, self._levels(probs), self.nms, self.nms_score, self.max_gap, self.min_len,
                          reference=decoder is decode_reference, soft=self.soft, **more)
        else:
            det = (decoder or decode)(probs.detach(), valid_t.to(torch.int32), fps, start, self._thr(probs), self.max_gap, self.min_len, **more)
        self._pending.append((det, names, unit))
        self._pending_bytes += sum(t.numel() * t.element_size() for t in det[:5])
        if self._pending_bytes > self.max_pending_bytes:
            self._drain()
        return det

    def _drain(self):
        for det, names, unit in self._pending:
            for name, segs in zip(names, det.tolist()):
                self._rows.append({'video': name, 'unit': unit, 'segments': segs})
        self._pending, self._pending_bytes = [], 0

    def take(self):
        """the objects of every video added so far (one read-back per kept batch), in the order added; the writer is empty afterwards"""
        self._drain()
        rows, self._rows = self._rows, []
        return rows

    def flush(self, path=None, rows=None):
        """write `rows` (default: take()) to `path` (default: the writer's) as JSON lines; returns the number of videos"""
        rows = self.take() if rows is None else rows
        path = self.path if path is None else path
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as fh:
            for r in rows:
                fh.write(json.dumps(r) + '\n')
        return len(rows)


def read_detections(path):
    """the list of per-video objects of a file DetectionWriter wrote"""
    with open(path) as fh:
        return [json.loads(line) for line in fh if line.strip()]
