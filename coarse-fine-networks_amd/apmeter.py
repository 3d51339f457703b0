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
    (cfn_hip.calibrate.Calibration), in place and without a read-back."""

    MIN_CAPACITY = 16384

    def __init__(self, device, capacity=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('DeviceAPMeter keeps its rows on a GPU (got device %s); apmeter.APMeter is the host meter' % self.device)
        if capacity is not None and int(capacity) < 1:
            raise ValueError('capacity: a positive number of rows expected, got %r' % (capacity,))
        self.capacity = None if capacity is None else int(capacity)
        self._state = torch.zeros(2, dtype=torch.int32, device=self.device)      # [rows held, flags]
        self._scores = self._targets = None
        self._bound = 0
        self._added = False

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

    def value_device(self):
        """(K,) fp32 AP on the device; reads nothing back (flags are not looked at: value() does)"""
        from cfn_hip import ops
        if self._scores is None:
            raise RuntimeError('DeviceAPMeter.value_device: nothing was added yet')
        return ops.average_precision(self._scores, self._targets, self.count)

    def _sorted(self, what, out):
        from cfn_hip import ops
        if self._scores is None:
            raise RuntimeError('DeviceAPMeter.%s: nothing was added yet' % what)
        return ops.ap_sort(self._scores, self._targets, self.count, out=out)

    def calibrate(self, calibration, out=None):
        """per-class thresholds of the rows held into a cfn_hip.calibrate.Calibration, in place: ONE ap_sort and ap_calibrate on the sorted
        stores; reads nothing back (flags are not looked at).  out: ap_sort's buffers to reuse (with a fixed capacity nothing is allocated
        then: capturable).  Returns the calibration."""
        from cfn_hip import ops
        ss, st = self._sorted('calibrate', out)
        ops.ap_calibrate(ss, st, self.count, calibration.kinds, calibration.values, out=calibration.outputs)
        calibration.updates += 1
        return calibration

    def value_and_thresholds(self, calibration, out=None):
        """(K,) fp32 AP on the device AND the calibration's thresholds from the same rows: ONE ap_sort, then ap_reduce and ap_calibrate on
        the same sorted stores; reads nothing back.  The AP is value_device()'s, the thresholds are calibrate()'s, bit for bit."""
        from cfn_hip import ops
        ss, st = self._sorted('value_and_thresholds', out)
        ap = ops.ap_reduce(st, self.count)
        ops.ap_calibrate(ss, st, self.count, calibration.kinds, calibration.values, out=calibration.outputs)
        calibration.updates += 1
        return ap

    def value(self, calibration=None):
        """(K,) float32 CPU tensor of per-class AP; 0 when nothing was added (as the reference).  calibration: a
        cfn_hip.calibrate.Calibration to update from the same sorted rows (value_and_thresholds); untouched when nothing was added"""
        if not self._added:
            return 0
        from cfn_hip import ops
        flags = int(self._state[1])
        assert not flags & ops.AP_FLAG_NONBINARY, 'targets should be binary (0 or 1)'
        if flags & ops.AP_FLAG_OVERFLOW:
            raise RuntimeError('DeviceAPMeter: more rows were added than the fixed capacity of %d holds' % self._scores.shape[1])
        return (self.value_device() if calibration is None else self.value_and_thresholds(calibration)).cpu()
