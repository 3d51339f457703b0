"""Per-class average precision accumulator with the reference's ``APMeter`` surface
(apmeter.py:22-136: ``reset`` / ``add(output, target, weight=None)`` / ``value``).

Host-side metric: scores are ranked per class with a stable descending sort and AP is the
mean of precision@rank over the positive ranks -- the same number the reference's torch loop produces
(pinned in tests/golden/loss_ap.npz).  Storage is a list of numpy blocks concatenated lazily instead of a
manually grown torch storage.

``DeviceAPMeter`` is the same metric with the rows kept in HBM (csrc/apmeter.hip): appending a batch reads nothing back, the per-class
ranking and the AP sums run as kernels, and the host is involved only when ``value()`` is called."""
import numpy as np
import torch


class APMeter(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self._scores, self._targets, self._weights = [], [], []

    def add(self, output, target, weight=None):
        output = output.detach().cpu().numpy() if torch.is_tensor(output) else np.asarray(output)
        target = target.detach().cpu().numpy() if torch.is_tensor(target) else np.asarray(target)
        if output.ndim == 1:
            output = output.reshape(-1, 1)
        if target.ndim == 1:
            target = target.reshape(-1, 1)
        assert output.ndim == 2 and target.ndim == 2, 'wrong size (should be 1D or 2D with one column per class)'
        assert np.array_equal(target * target, target), 'targets should be binary (0 or 1)'
        if self._scores:
            assert target.shape[1] == self._targets[0].shape[1], \
                'dimensions for output should match previously added examples.'
        if weight is not None:
            weight = (weight.detach().cpu().numpy() if torch.is_tensor(weight) else np.asarray(weight)).reshape(-1)
            assert weight.shape[0] == target.shape[0], 'Weight dimension 1 should be the same as that of target'
            assert weight.min() >= 0, 'Weight should be non-negative only'
            self._weights.append(weight.astype(np.float32))
        self._scores.append(output.astype(np.float32))
        self._targets.append(target.astype(np.int64))

    def value(self):
        """(K,) float32 tensor of per-class AP; 0 when nothing was added (as the reference)."""
        if not self._scores:
            return 0
        scores, targets = np.concatenate(self._scores), np.concatenate(self._targets)
        weights = np.concatenate(self._weights) if self._weights else None
        n, k = scores.shape
        ap = np.zeros(k, dtype=np.float32)
        ranks = np.arange(1, n + 1, dtype=np.float32)
        for j in range(k):
            order = np.argsort(-scores[:, j], kind='stable')
            truth = targets[order, j].astype(np.float32)
            if weights is not None:
                w = weights[order]
                tp, rg = np.cumsum(truth * w, dtype=np.float32), np.cumsum(w, dtype=np.float32)
            else:
                tp, rg = np.cumsum(truth, dtype=np.float32), ranks
            prec = tp / rg
            ap[j] = prec[truth > 0].sum() / max(truth.sum(), 1)
        return torch.from_numpy(ap)


class DeviceAPMeter(object):
    """``APMeter`` with scores and targets resident on the GPU, class major: scores (K, cap) fp32, targets (K, cap) uint8, the row count
    and a flag word on the device (``cfn_hip.ops.ap_append / ap_sort / average_precision``).

    ``add_batch`` is the hot path and makes no host synchronisation: the host keeps only an UPPER BOUND of the rows held (B * TL per
    batch; the kernels take the exact count from the device).  capacity=None: the stores grow geometrically when that bound passes the
    capacity (a new allocation and a stream-ordered copy).  An explicit capacity (rows) fixes the buffers for good: ``add_batch`` is then
    safe inside a graph capture, and a batch that does not fit is dropped, flagged on the device and reported by ``value()``.
    Unweighted AP only.  ``calibrate`` / ``value_and_thresholds`` turn the same sorted rows into per-class decode thresholds
    (cfn_hip.calibrate.Calibration), in place and without a read-back.

    A meter made without the next three arguments behaves exactly as before.  across_ranks=True (group: the process group, None = the
    default one; n_classes: the class count, needed then, so that a rank without a batch still owns stores of the right shape): under a
    world size above 1 ``value_device``, ``value``, ``calibrate`` and ``value_and_thresholds`` evaluate the rows of ALL ranks, appended in
    rank order into a fresh store (cfn_hip.apmerge.gather_stores, rules M1-M4): every rank gets the same bits, those of one process fed
    the ranks' batches one rank after another.  Each such call is a collective that every rank must make; the rank's own stores are
    untouched.  Without a process group, or with a world size of 1, nothing is gathered or copied.  ``merge(*others)`` and
    ``DeviceAPMeter.merged(parts)`` append other meters' rows within one process (ONE cfn_hip.ops.ap_merge)."""

    MIN_CAPACITY = 16384

    def __init__(self, device, capacity=None, across_ranks=False, group=None, n_classes=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('DeviceAPMeter keeps its rows on a GPU (got device %s); apmeter.APMeter is the host meter' % self.device)
        if capacity is not None and int(capacity) < 1:
            raise ValueError('capacity: a positive number of rows expected, got %r' % (capacity,))
        if n_classes is not None and int(n_classes) < 1:
            raise ValueError('n_classes >= 1 expected, got %r' % (n_classes,))
        if across_ranks and n_classes is None:
            raise ValueError('DeviceAPMeter: across_ranks=True needs n_classes: the gather is a collective, and a rank that has seen no batch '
                             'yet must still know the shape of the stores')
        self.capacity = None if capacity is None else int(capacity)
        self.across_ranks, self.group = bool(across_ranks), group
        self._state = torch.zeros(2, dtype=torch.int32, device=self.device)      # [rows held, flags]
        self._scores = self._targets = None
        self._bound = 0
        self._added = False
        if n_classes is not None:          # the stores from the start (a meter made without n_classes allocates with its first batch, as before)
            self._reserve(int(n_classes), 0)

    @property
    def count(self):
        """the device row count (one int32)"""
        return self._state[0:1]

    @property
    def flags(self):
        return self._state[1:2]

    @property
    def stores(self):
        """(scores (K, cap), targets (K, cap)) or (None, None) before the first batch"""
        return self._scores, self._targets

    def reset(self):
        self._state.zero_()          # on the current stream; the buffers stay
        self._bound = 0
        self._added = False

    def _alloc(self, K, cap):
        if self.capacity is None:
            cap = (cap + 15) // 16 * 16       # rows of a class start on 16-byte boundaries of the target store
        return (torch.empty(K, cap, dtype=torch.float32, device=self.device), torch.empty(K, cap, dtype=torch.uint8, device=self.device))

    def _reserve(self, K, rows):
        if self._scores is None:
            cap = self.capacity if self.capacity is not None else max(self.MIN_CAPACITY, rows)
            self._scores, self._targets = self._alloc(K, cap)
        elif self._scores.shape[0] != K:
            raise AssertionError('dimensions for output should match previously added examples.')
        held, cap = self._bound, self._scores.shape[1]
        self._bound = min(held + rows, 2 ** 31) if self.capacity is not None else held + rows
        if self.capacity is None and self._bound > cap:
            scores, targets = self._alloc(K, max(2 * cap, self._bound))
            if held:
                scores[:, :held].copy_(self._scores[:, :held])
                targets[:, :held].copy_(self._targets[:, :held])
            self._scores, self._targets = scores, targets

    def add_batch(self, probs, labels, valid=None):
        """probs, labels (B, K, TL) on the device, valid (B,) on the device or None: video b adds its first min(valid[b], TL) frames"""
        from cfn_hip import ops
        if not (torch.is_tensor(probs) and torch.is_tensor(labels) and probs.is_cuda and labels.is_cuda) or (valid is not None and not valid.is_cuda):
            raise RuntimeError('DeviceAPMeter.add_batch takes device tensors (there is no CPU path); apmeter.APMeter is the host meter')
        if probs.dim() != 3 or tuple(labels.shape) != tuple(probs.shape):
            raise RuntimeError('probs and labels of one shape (B, K, TL) expected, got %s and %s' % (tuple(probs.shape), tuple(labels.shape)))
        B, K, TL = probs.shape
        self._reserve(K, B * TL)
        ops.ap_append(probs.detach(), labels.detach(), valid, self._scores, self._targets, self.count, self.flags)
        self._added = True

    def add(self, output, target, weight=None):
        """the reference surface: (rows, K) device tensors (1-D: one class)"""
        if weight is not None:
            raise NotImplementedError('DeviceAPMeter computes unweighted AP; apmeter.APMeter takes weights')
        if not (torch.is_tensor(output) and torch.is_tensor(target) and output.is_cuda and target.is_cuda):
            raise RuntimeError('DeviceAPMeter.add takes device tensors (there is no CPU path); apmeter.APMeter is the host meter')
        output, target = output.detach(), target.detach()
        if output.dim() == 1:
            output = output.view(-1, 1)
        if target.dim() == 1:
            target = target.view(-1, 1)
        assert output.dim() == 2 and target.dim() == 2, 'wrong size (should be 1D or 2D with one column per class)'
        if output.shape[0] == 0:
            return
        self.add_batch(output.float().t().contiguous().unsqueeze(0), target.float().t().contiguous().unsqueeze(0))

    def _part(self):
        """this meter's store as cfn_hip.apmerge.stack_parts takes it, and the host's upper bound of the rows it holds"""
        return (self._scores, self._targets, self.count, None, self.flags), min(self._bound, int(self._scores.shape[1]))

    def merge(self, *others):
        """append the rows of `others` (DeviceAPMeters of the same class count, on any GPU) behind this meter's, in the order given, in
        place: ONE cfn_hip.ops.ap_merge with R = the others that hold stores (rules M1-M4 of cfn_hip/apmerge.py).  The meter is then, bit
        for bit, what it would be had it been fed its own batches and then the others'.  The others stay untouched; one that has no stores
        yet adds nothing, and a meter without stores takes its class count from the first that has them.  Growing mode reserves from the
        host's bounds, which stay upper bounds; a fixed capacity never reads back: a merge that does not fit changes nothing, is flagged
        on the device and reported by value()."""
        from cfn_hip import apmerge, ops
        for o in others:
            if not isinstance(o, DeviceAPMeter):
                raise ValueError('DeviceAPMeter.merge: a DeviceAPMeter expected, got %s' % type(o).__name__)
            if o is self:
                raise ValueError('DeviceAPMeter.merge: a meter cannot be merged into itself (sources and destination must not overlap)')
        held = [o for o in others if o._scores is not None]
        K = int(self._scores.shape[0]) if self._scores is not None else (int(held[0]._scores.shape[0]) if held else None)
        for o in held:
            if int(o._scores.shape[0]) != K:
                raise ValueError('DeviceAPMeter.merge: meters of one class count expected, got %d against %d' % (int(o._scores.shape[0]), K))
        if not held:
            return self
        parts, bounds = zip(*(o._part() for o in held))
        parts = [tuple(None if t is None else t.to(self.device) for t in p) for p in parts]
        self._reserve(K, sum(bounds))
        # (one part goes as its own stores, whole: no copy, and the tiles behind its count exit; several are stacked at the largest host bound)
        src = apmerge.stack_parts(parts, m=int(parts[0][0].shape[1]) if len(parts) == 1 else max(bounds))
        ops.ap_merge(self._scores, self._targets, self.count, None, self.flags, *src)
        self._added = self._added or any(o._added for o in held)
        return self

    @classmethod
    def merged(cls, parts, capacity=None):
        """a NEW meter on parts[0]'s device (growing, or of the fixed `capacity`) that holds the parts' rows in list order, through ONE
        cfn_hip.ops.ap_merge with R = len(parts): the code path the gather over ranks takes behind its collectives"""
        parts = list(parts)
        if not parts:
            raise ValueError('DeviceAPMeter.merged: at least one meter expected')
        return cls(parts[0].device, capacity).merge(*parts)

    def _across(self):
        from cfn_hip import apmerge
        return self.across_ranks and apmerge.world_size(self.group) > 1

    def _stores(self, what):
        """(scores, targets, count, flags) to evaluate: this meter's, or -- across_ranks under a world size above 1 -- all ranks' rows
        appended in rank order into a fresh store (cfn_hip.apmerge.gather_stores: a collective; this rank's stores stay untouched)"""
        if self._scores is None:
            raise RuntimeError('DeviceAPMeter.%s: nothing was added yet' % what)
        if self._across():
            from cfn_hip import apmerge
            scores, targets, state = apmerge.gather_stores(self._scores, self._targets, self._state, 1, self.group)
            return scores, targets, state[0:1], state[1:2]
        return self._scores, self._targets, self.count, self.flags

    def value_device(self):
        """(K,) fp32 AP on the device; reads nothing back (flags are not looked at: value() does).  With across_ranks under a world size
        above 1: of all ranks' rows in rank order, the same bits on every rank -- a COLLECTIVE that every rank must make (and the one
        read-back of two ints that sizes the gather); calibrate and value_and_thresholds likewise."""
        from cfn_hip import ops
        scores, targets, count, _ = self._stores('value_device')
        return ops.average_precision(scores, targets, count)

    def _sorted(self, what, out):
        """-> (sorted scores, sorted targets, the count they were sorted under)"""
        from cfn_hip import ops
        scores, targets, count, _ = self._stores(what)
        if scores is not self._scores:     # (the gathered store has its own size: the caller's buffers fit this rank's)
            out = None
        return ops.ap_sort(scores, targets, count, out=out) + (count,)

    def calibrate(self, calibration, out=None):
        """per-class thresholds of the rows held into a cfn_hip.calibrate.Calibration, in place: ONE ap_sort and ap_calibrate on the sorted
        stores; reads nothing back (flags are not looked at).  out: ap_sort's buffers to reuse (with a fixed capacity nothing is allocated
        then: capturable).  Returns the calibration."""
        from cfn_hip import ops
        ss, st, count = self._sorted('calibrate', out)
        ops.ap_calibrate(ss, st, count, calibration.kinds, calibration.values, out=calibration.outputs)
        calibration.updates += 1
        return calibration

    def value_and_thresholds(self, calibration, out=None):
        """(K,) fp32 AP on the device AND the calibration's thresholds from the same rows: ONE ap_sort, then ap_reduce and ap_calibrate on
        the same sorted stores; reads nothing back.  The AP is value_device()'s, the thresholds are calibrate()'s, bit for bit."""
        from cfn_hip import ops
        ss, st, count = self._sorted('value_and_thresholds', out)
        ap = ops.ap_reduce(st, count)
        ops.ap_calibrate(ss, st, count, calibration.kinds, calibration.values, out=calibration.outputs)
        calibration.updates += 1
        return ap

    def value(self, calibration=None):
        """(K,) float32 CPU tensor of per-class AP; 0 when nothing was added (as the reference).  calibration: a
        cfn_hip.calibrate.Calibration to update from the same sorted rows (value_and_thresholds); untouched when nothing was added"""
        if self._across():
            return self._value_across(calibration)
        if not self._added:
            return 0
        flags = int(self._state[1])
        self._check_flags(flags)
        return (self.value_device() if calibration is None else self.value_and_thresholds(calibration)).cpu()

    def _check_flags(self, flags):
        from cfn_hip import ops
        assert not flags & ops.AP_FLAG_NONBINARY, 'targets should be binary (0 or 1)'
        if flags & ops.AP_FLAG_BAD_SOURCE:
            raise RuntimeError('DeviceAPMeter: a merge met a source store whose count was outside [0, capacity] (a malformed source) and was '
                               'refused: the value would miss those rows')
        if flags & ops.AP_FLAG_OVERFLOW:
            raise RuntimeError('DeviceAPMeter: more rows were added than the fixed capacity of %d holds' % self._scores.shape[1])

    def _value_across(self, calibration):
        """value() over all ranks' rows: ONE gather (every rank makes it, whether it added a batch or not), one read-back of the merged
        count and flags; 0 when no rank added a row"""
        from cfn_hip import ops
        scores, targets, count, flags = self._stores('value')
        rows, fl = (int(x) for x in torch.cat([count, flags]).cpu())
        self._check_flags(fl)
        if rows == 0:
            return 0
        ss, st = ops.ap_sort(scores, targets, count)
        if calibration is not None:
            ops.ap_calibrate(ss, st, count, calibration.kinds, calibration.values, out=calibration.outputs)
            calibration.updates += 1
        return ops.ap_reduce(st, count).cpu()
