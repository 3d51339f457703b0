"""Bookkeeping of a training phase: the running loss totals and the training mAP of the three loops (train_fine.run,
train_coarse_fineFEAT.run, train_joint.run).

``StepMetrics(device_ap=False)`` is what the loops did inline: both losses are read back with ``float()`` after every step, and the
valid frames of every video go to the host ``apmeter.APMeter`` (one ``int(valid_t[i])`` and two copies per video).

``StepMetrics(device_ap=True)`` leaves everything on the GPU: the rows go to ``apmeter.DeviceAPMeter.add_batch`` with ``valid_t`` as it
is, the loss totals are fp64 device scalars to which the fp32 losses are added in step order (the same additions the host path makes in
Python floats, so the totals are equal bit for bit), and the host waits for the device only in ``report()``."""
import torch

from apmeter import APMeter, DeviceAPMeter


def ap_rows(probs, labels, valid_t):
    """per video: (scores (v, K), targets (v, K)) numpy over the valid frames -- what APMeter.add takes"""
    rows = []
    for i in range(labels.shape[0]):
        v = int(valid_t[i])
        rows.append((probs[i][:, :v].transpose(0, 1).cpu().numpy(), labels[i][:, :v].transpose(0, 1).cpu().numpy()))
    return rows


class StepMetrics(object):
    def __init__(self, device_ap=False, device=None, capacity=None):
        self.device_ap = bool(device_ap)
        self.steps = 0
        if self.device_ap:
            self.device = torch.device('cuda' if device is None else device)
            self.apm = DeviceAPMeter(self.device, capacity=capacity)
            self._tot = torch.zeros(2, dtype=torch.float64, device=self.device)       # [cls, loc]
        else:
            self.apm = APMeter()
            self.tot_cls = self.tot_loc = 0.0

    def start_phase(self):
        """a new training phase: the loss totals start again, the AP rows stay (the loops reset those when they log)"""
        self.steps = 0
        if self.device_ap:
            self._tot.zero_()
        else:
            self.tot_cls = self.tot_loc = 0.0

    def update(self, cls_loss, loc_loss, probs, labels, valid_t):
        """one training step: the two losses (0-d tensors), probs / labels (B, K, TL), valid_t (B,) valid frames per video"""
        self.steps += 1
        if self.device_ap:
            self.apm.add_batch(probs, labels, valid_t)
            self._tot += torch.stack((cls_loss.detach(), loc_loss.detach())).to(torch.float64)
        else:
            for sc, tg in ap_rows(probs.detach(), labels, valid_t):
                self.apm.add(sc, tg)
            self.tot_cls += float(cls_loss)
            self.tot_loc += float(loc_loss)

    def totals(self):
        """(tot_loc, tot_cls) as Python floats (device path: one read-back)"""
        if self.device_ap:
            cls, loc = self._tot.tolist()
            return loc, cls
        return self.tot_loc, self.tot_cls

    def _need_device(self, calibration):
        if calibration is not None and not self.device_ap:
            raise RuntimeError('StepMetrics: a calibration takes its rows from the device meter: calibration needs device_ap=True (the host APMeter '
                               'keeps its rows in numpy)')

    def mean_ap(self, calibration=None):
        """calibration: a cfn_hip.calibrate.Calibration updated from the same sorted rows (DeviceAPMeter.value_and_thresholds; device_ap only)"""
        self._need_device(calibration)
        v = self.apm.value() if calibration is None else self.apm.value(calibration)
        return float(v.mean()) if torch.is_tensor(v) else float(v)

    def calibrate(self, calibration):
        """thresholds from the AP rows held since reset_ap(), without the AP (DeviceAPMeter.calibrate; nothing is read back) -> True, or
        False when no row was added since"""
        self._need_device(calibration)
        if not self.apm._added:
            return False
        self.apm.calibrate(calibration)
        return True

    def report(self, calibration=None):
        """-> (mean loc loss, mean cls loss, mAP) over the steps since start_phase() / the AP rows since reset_ap(); calibration: see mean_ap"""
        self._need_device(calibration)
        loc, cls = self.totals()
        n = max(self.steps, 1)
        return loc / n, cls / n, self.mean_ap(calibration)

    def reset_ap(self):
        self.apm.reset()
