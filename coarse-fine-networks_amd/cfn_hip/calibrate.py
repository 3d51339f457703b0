"""Per-class decode thresholds calibrated from the training AP rows, on the GPU (cfn_hip.ops.ap_calibrate, csrc/apcal.hip).

``decode`` / ``propose`` (cfn_hip/detections.py) compare every class against thresholds somebody typed; the scores are sigmoids of classes
whose frame prevalence differs by orders of magnitude, so one constant suits none of them.  With ``device_ap`` the training phases already
keep every valid frame's score and label, class major, in ``apmeter.DeviceAPMeter``, and ``ap_sort`` ranks each class for the AP.  A
per-class operating point is one more walk over those sorted rows, and its result is exactly the ``(C,)`` / ``(C, K)`` fp32 device tensor
``decode`` / ``decode_levels`` take: a ``Calibration`` owns that tensor, ``update`` rewrites it in place without reading anything back, and
every later decode that was handed the tensor sees the new values (a captured graph need not be captured again).

The rule, stated once (the kernel, ``thresholds_reference`` and include/cfn_hip.h spell the same).  Per class c: the first
``n = clamp(count, 0, cap)`` rows of ``sorted_scores[c]`` (fp32, descending, canonical as ap_sort leaves them: NaN last, -inf just in
front) and ``sorted_targets[c]`` (uint8, positive iff != 0); K criteria, 1 <= K <= 16, each a ``(kind, value)`` pair:

    1. P = positives among all n rows.  m = rows with score > -inf (fp32 compare; a NaN fails): a prefix.  Rows behind m can never be
       active under decode's strict ``probs > thr``; their positives still count in P
    2. tp(r) = positives among rows 0 .. r - 1, tp(0) = 0
    3. a cut r of 1 .. m is ADMISSIBLE iff r == m or score[r - 1] > score[r] (strict): a threshold cannot separate equal scores
    4. ``f1``: over r = 0 and the admissible cuts, maximise 2 tp(r) / (r + P), compared EXACTLY in unsigned 64-bit integers: a beats b iff
       tp(a) * (b + P) > tp(b) * (a + P) (both factors are below 2^32); start from r = 0 and replace only on strict improvement, so ties go
       to the smallest r; P == 0 gives r = 0 with no special case
       ``precision p``, 0 < p <= 1: the LARGEST admissible r with (double)tp(r) >= p * (double)r -- one fp64 multiply and one compare,
       nothing to contract; none: r = 0
       ``recall q``, 0 < q <= 1: P == 0 gives r = 0; otherwise the SMALLEST admissible r with (double)tp(r) >= q * (double)P; none (positives
       behind m): r = m
       ok[c, k] = 1 iff the criterion was met: f1: tp > 0; precision and recall: the inequality holds at the returned r > 0
    5. the threshold of a cut: r == 0 gives +inf; 0 < r < m gives score[r], the largest score NOT taken, so decode's strict rule activates
       exactly rows 0 .. r - 1 of the calibration data; r == m > 0 gives -inf
    6. outputs: ``thr (C, K)`` fp32 (the layout of ``levels_tensor``; column 0 of a K = 1 result is a contiguous ``(C,)`` thr), ``cut (C, K)``
       int32, ``tp (C, K)`` int32, ``ok (C, K)`` uint8, ``stat (C, 2)`` int32 [P, m].  Precision tp / cut, recall tp / P and F1
       2 tp / (cut + P) at the operating point follow from these integers on the host
    7. a consequence: recall criteria listed with ascending q give non-increasing thresholds -- the high-to-low level order that rule N2 of
       cfn_hip/detections.py wants under score='max'

Limits: K <= 16, C <= 65535, cap < 2^31; frame-level rows only (the training meter's); rank 0's rows calibrate rank 0; no CPU path for the
operator.  No accuracy gain is claimed.  This module is host only (numpy + torch) apart from ``ops.ap_calibrate``.
"""
import json
import numbers

import numpy as np
import torch

KINDS = {'f1': 0, 'precision': 1, 'recall': 2}
MAX_CRITERIA = 16


def check_criteria(criteria):
    """a sequence of (kind, value) -> the list of (kind, float or None); raises ValueError with the reason"""
    out = []
    for item in criteria:
        if isinstance(item, str) or not hasattr(item, '__len__') or len(item) != 2:
            raise ValueError('criteria: (kind, value) pairs expected, got %r' % (item,))
        kind, value = item
        if kind not in KINDS:
            raise ValueError("criteria: unknown kind %r ('f1', 'precision' or 'recall' expected)" % (kind,))
        if kind == 'f1':
            if value is not None:
                raise ValueError('criteria: f1 takes no value, got %r' % (value,))
            out.append((kind, None))
            continue
        if isinstance(value, bool) or not isinstance(value, (int, float)):
            raise ValueError('criteria: %s needs a value in (0, 1], got %r' % (kind, value))
        value = float(value)
        if not 0.0 < value <= 1.0:                                                    # (a NaN fails too)
            raise ValueError('criteria: %s value in (0, 1] expected, got %r' % (kind, value))
        out.append((kind, value))
    if not 1 <= len(out) <= MAX_CRITERIA:
        raise ValueError('criteria: 1 to %d criteria expected, got %d' % (MAX_CRITERIA, len(out)))
    return out


def parse_criteria(spec):
    """'f1' | 'precision:0.5' | 'recall:0.2,0.4,0.6,0.8' -> [(kind, value), ...] (f1: value None).  Several values are the levels form: one
    criterion each, in the order given.  More than 16 values, a value outside (0, 1] or an unknown kind raises ValueError with the reason."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("criteria: 'f1', 'precision:P' or 'recall:Q1,Q2,...' expected, got %r" % (spec,))
    kind, sep, rest = spec.strip().partition(':')
    kind = kind.strip()
    if kind not in KINDS:
        raise ValueError("criteria: unknown kind %r in %r ('f1', 'precision:P' or 'recall:Q1,Q2,...' expected)" % (kind, spec))
    if kind == 'f1':
        if sep:
            raise ValueError('criteria: f1 takes no value, got %r' % (spec,))
        return [('f1', None)]
    parts = [p.strip() for p in rest.split(',')] if sep else []
    if not parts or any(not p for p in parts):
        raise ValueError('criteria: %s needs 1 to %d values in (0, 1], e.g. %s:0.5; got %r' % (kind, MAX_CRITERIA, kind, spec))
    try:
        vals = [float(p) for p in parts]
    except ValueError:
        raise ValueError('criteria: %s values must be numbers in (0, 1], got %r' % (kind, spec))
    return check_criteria([(kind, v) for v in vals])


def criteria_tensors(criteria, device=None):
    """(kinds (K,) int32, values (K,) fp64) of checked criteria, as ops.ap_calibrate takes them (f1: value 0)"""
    crit = check_criteria(criteria)
    kinds = torch.tensor([KINDS[k] for k, _ in crit], dtype=torch.int32)
    values = torch.tensor([0.0 if v is None else v for _, v in crit], dtype=torch.float64)
    return (kinds, values) if device is None else (kinds.to(device), values.to(device))


def _best_f1(cuts, tp, P):
    """rule 4, f1: cuts ascending (r = 0 first), tp their tp(r) -> the index of the winner.  The exact comparison runs in Python integers
    over the cuts whose fp64 quotient tp / (r + P) is the largest one: a correctly rounded quotient is monotonic in the exact value, so
    every exact maximiser is among them"""
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(cuts + P > 0, tp.astype(np.float64) / np.maximum(cuts + P, 1).astype(np.float64), 0.0)
    best = 0
    for i in np.flatnonzero(q == q.max()):
        a, b = int(cuts[i]), int(cuts[best])
        if int(tp[i]) * (b + P) > int(tp[best]) * (a + P):                              # strict: ties stay with the smaller r
            best = int(i)
    return best


def thresholds_reference(sorted_scores, sorted_targets, count, criteria):
    """ops.ap_calibrate from rules 1-6 in numpy; tensors (or arrays) on any device -> (thr (C, K) fp32, cut, tp (C, K) int32, ok (C, K)
    uint8, stat (C, 2) int32) as CPU tensors: the tests' reference.  count: an int or a one-element tensor."""
    crit = check_criteria(criteria)
    s = sorted_scores.detach().cpu().numpy() if torch.is_tensor(sorted_scores) else np.asarray(sorted_scores)
    g = sorted_targets.detach().cpu().numpy() if torch.is_tensor(sorted_targets) else np.asarray(sorted_targets)
    if s.dtype != np.float32 or s.ndim != 2 or g.dtype != np.uint8 or g.shape != s.shape:
        raise ValueError('sorted stores expected: scores (C, cap) float32 and targets (C, cap) uint8, got %s %s and %s %s' % (s.dtype, s.shape, g.dtype, g.shape))
    C, cap = s.shape
    n = min(max(int(count.item()) if torch.is_tensor(count) else int(count), 0), cap)
    K = len(crit)
    thr, cut, tps = np.zeros((C, K), np.float32), np.zeros((C, K), np.int32), np.zeros((C, K), np.int32)
    ok, stat = np.zeros((C, K), np.uint8), np.zeros((C, 2), np.int32)
    for c in range(C):
        sc, pos = s[c, :n], g[c, :n] != 0
        P = int(pos.sum())                                                            # rule 1
        with np.errstate(invalid='ignore'):
            m = int(np.count_nonzero(sc > np.float32(-np.inf)))
        tp = np.concatenate([[0], np.cumsum(pos[:m], dtype=np.int64)])                # rule 2: tp[r], r = 0 .. m
        adm = np.zeros(m + 1, bool)                                                   # rule 3
        if m > 0:
            adm[m] = True
            with np.errstate(invalid='ignore'):
                adm[1:m] = sc[:m - 1] > sc[1:m]
        cuts = np.flatnonzero(adm).astype(np.int64)                                   # ascending, r >= 1
        stat[c] = P, m
        for k, (kind, value) in enumerate(crit):                                      # rule 4
            r, met = 0, False
            if kind == 'f1':
                cand = np.concatenate([[0], cuts])
                r = int(cand[_best_f1(cand, tp[cand], P)])
                met = tp[r] > 0
            elif kind == 'precision':
                hit = np.flatnonzero(tp[cuts].astype(np.float64) >= np.float64(value) * cuts.astype(np.float64))
                if hit.size:
                    r, met = int(cuts[hit[-1]]), True
            elif P > 0:
                hit = np.flatnonzero(tp[cuts].astype(np.float64) >= np.float64(value) * np.float64(P))
                r, met = (int(cuts[hit[0]]), True) if hit.size else (m, False)
            cut[c, k], tps[c, k], ok[c, k] = r, int(tp[r]), 1 if met else 0
            thr[c, k] = np.float32(np.inf) if r == 0 else (sc[r] if r < m else np.float32(-np.inf))      # rule 5
    return torch.from_numpy(thr), torch.from_numpy(cut), torch.from_numpy(tps), torch.from_numpy(ok), torch.from_numpy(stat)


class Calibration(object):
    """The thresholds of ``n_classes`` classes under K criteria, with everything the kernel writes beside them, on one device:

        thr (C, K) fp32    filled with ``initial`` -- a float, or K floats: the typed --detect-thr / --detect-levels -- so that decodes in
                           front of the first update behave as without a calibration
        cut, tp (C, K) int32, ok (C, K) uint8, stat (C, 2) int32 [P, m]    zero until the first update
        kinds (K,) int32, values (K,) fp64    the criteria as the kernel reads them

    ``thr_vector`` (K = 1 only) is the (C,) view ``decode`` / ``DetectionWriter(thr=)`` / ``SegmentAPMeter(thr=)`` take, ``levels`` the (C, K)
    tensor ``decode_levels`` / ``propose`` / ``levels=`` take: views of ONE tensor that ``update`` rewrites in place.  ``update`` reads
    nothing back; ``summary`` is the one read-back, of the small integer tensors."""

    def __init__(self, criteria, n_classes, device, initial=0.5):
        self.criteria = check_criteria(parse_criteria(criteria) if isinstance(criteria, str) else criteria)
        self.n_classes, self.device = int(n_classes), torch.device(device)
        if not 1 <= self.n_classes <= 65535:
            raise ValueError('n_classes in [1, 65535] expected, got %r' % (n_classes,))
        C, K = self.n_classes, len(self.criteria)
        if torch.is_tensor(initial):
            initial = initial.detach().cpu().tolist()                                     # (a 0-d tensor gives a float)
        if isinstance(initial, numbers.Real) and not isinstance(initial, bool):          # (numpy scalars included)
            init = [float(initial)] * K
        else:
            try:
                init = [float(x) for x in initial]
            except (TypeError, ValueError):
                init = None
            if init is None or len(init) != K:
                raise ValueError('initial: a float or %d floats (one per criterion) expected, got %r' % (K, initial))
        self.initial = init
        self.thr = torch.tensor(init, dtype=torch.float32).repeat(C, 1).to(self.device).contiguous()
        self.cut = torch.zeros(C, K, dtype=torch.int32, device=self.device)
        self.tp = torch.zeros(C, K, dtype=torch.int32, device=self.device)
        self.ok = torch.zeros(C, K, dtype=torch.uint8, device=self.device)
        self.stat = torch.zeros(C, 2, dtype=torch.int32, device=self.device)
        self.kinds, self.values = criteria_tensors(self.criteria, self.device)
        self.updates = 0

    @property
    def n_criteria(self):
        return len(self.criteria)

    @property
    def outputs(self):
        """(thr, cut, tp, ok, stat): the out= of ops.ap_calibrate"""
        return self.thr, self.cut, self.tp, self.ok, self.stat

    @property
    def thr_vector(self):
        """the (C,) view of thr (K = 1 only): what decode / DetectionWriter / SegmentAPMeter take as thr"""
        if self.n_criteria != 1:
            raise ValueError('Calibration.thr_vector: one criterion expected, this calibration has %d: its (C, K) `levels` go through propose' % self.n_criteria)
        return self.thr[:, 0]

    @property
    def levels(self):
        """thr as the (C, K) levels of decode_levels / propose"""
        return self.thr

    def update(self, meter):
        """thresholds from the rows a DeviceAPMeter holds: one sort, one calibrate, in place, NO read-back"""
        meter.calibrate(self)
        return self

    def summary(self):
        """ONE read-back of the integer tensors -> {'classes': classes with P > 0, 'n_classes': C, 'criteria': [{'kind', 'value', 'ok': classes
        that met it, 'precision', 'recall', 'f1': micro figures over all classes at their operating points}, ...]}"""
        C, K = self.n_classes, self.n_criteria
        host = torch.cat([self.stat.reshape(-1), self.cut.reshape(-1), self.tp.reshape(-1), self.ok.to(torch.int32).reshape(-1)]).cpu().numpy().astype(np.int64)
        stat, cut, tp, ok = host[:2 * C].reshape(C, 2), host[2 * C:2 * C + C * K].reshape(C, K), host[2 * C + C * K:2 * C + 2 * C * K].reshape(C, K), \
            host[2 * C + 2 * C * K:].reshape(C, K)
        P = int(stat[:, 0].sum())
        rows = []
        for k, (kind, value) in enumerate(self.criteria):
            t, r = int(tp[:, k].sum()), int(cut[:, k].sum())
            rows.append({'kind': kind, 'value': value, 'ok': int(ok[:, k].sum()), 'precision': t / r if r else 0.0, 'recall': t / P if P else 0.0,
                         'f1': 2.0 * t / (r + P) if r + P else 0.0})
        return {'classes': int((stat[:, 0] > 0).sum()), 'n_classes': C, 'criteria': rows}

    def summary_line(self):
        """summary() as the text the training scripts log behind their mAP line"""
        s = self.summary()
        return 'calibrated {}/{} classes: '.format(s['classes'], s['n_classes']) + ' '.join(
            '{}{} ok {} P {:.4f} R {:.4f} F1 {:.4f}'.format(r['kind'], '' if r['value'] is None else ':%g' % r['value'], r['ok'], r['precision'], r['recall'], r['f1'])
            for r in s['criteria'])

    def save(self, path):
        """JSON: the criteria and the thresholds as fp32 bit patterns (one read-back)"""
        bits = self.thr.detach().cpu().contiguous().view(torch.int32).tolist()
        with open(path, 'w') as fh:
            json.dump({'criteria': [[k, v] for k, v in self.criteria], 'n_classes': self.n_classes, 'initial': self.initial, 'thr_bits': bits}, fh)
        return path

    @classmethod
    def load(cls, path, device):
        """the calibration save() wrote, on `device`: the same criteria and the same threshold bits (cut, tp, ok, stat are not kept)"""
        with open(path) as fh:
            d = json.load(fh)
        cal = cls([(k, v) for k, v in d['criteria']], d['n_classes'], device, d.get('initial', 0.5))
        bits = torch.tensor(d['thr_bits'], dtype=torch.int32)
        if tuple(bits.shape) != tuple(cal.thr.shape):
            raise ValueError('%s: thr_bits of shape %s expected, got %s' % (path, tuple(cal.thr.shape), tuple(bits.shape)))
        cal.thr.copy_(bits.view(torch.float32))
        return cal
