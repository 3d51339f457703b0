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

This module is host only (numpy + torch) apart from that call.
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


def decode(probs, valid_t, fps=None, start=None, thr=0.5, max_gap=0, min_len=1, cap=None, out=None):
    """probs (B, C, TL) fp32 and valid_t (B,) int32 on the GPU -> Detections there (ops.decode_segments: three launches, nothing is read
    back).  fps=None: fps = 1 (and start=None: start = 0), so times are in frames, still with the half frame outward.  thr: a float or a
    (C,) fp32 device tensor.  cap, out: see ops.decode_segments."""
    from . import ops
    fps, start = _defaults(probs, fps, start)
    C = int(probs.shape[1]) if probs.dim() == 3 else 0
    if cap is None and probs.dim() == 3:
        cap = ops.decode_segments_cap(*probs.shape)
    seg, frames, score, offsets, total = ops.decode_segments(probs, valid_t, fps, start, thr, max_gap, min_len, cap, out)
    return Detections(seg, frames, score, offsets, total, C, int(cap))


def decode_reference(probs, valid_t, fps=None, start=None, thr=0.5, max_gap=0, min_len=1, cap=None):
    """decode() from the definition, rule by rule, in numpy; tensors on any device, the result on probs' device: the tests' reference and
    the CPU spelling.  cap=None: exactly the rows found (at least one, as SegLabels.seg is never empty); a cap keeps the first `cap` rows and
    the true offsets / total, as the kernel does."""
    dev = probs.device
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
    B * C * ((TL + 1) // 2) * 44 bytes on the device: the kept tensors are read back early once they exceed `max_pending_bytes`."""

    def __init__(self, path, thr=0.5, max_gap=0, min_len=1, max_pending_bytes=1 << 30):
        self.path, self.thr, self.max_gap, self.min_len = path, thr, int(max_gap), int(min_len)
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
        det = (decoder or decode)(probs.detach(), valid_t.to(torch.int32), fps, start, self._thr(probs), self.max_gap, self.min_len)
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
