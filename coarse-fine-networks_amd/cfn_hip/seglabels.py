"""Frame labels from annotation segments: a sample carries its video's action segments and its label window instead of the dense
(157, TL) fp32 array; the batch carries a few hundred bytes, and one kernel writes the dense ``labels (B, C, TLmax)``, ``mask (B, TLmax)``
and ``valid_t (B,)`` on the GPU (cfn_hip.ops.seg_labels, csrc/seglabels.hip).

The reference builds the dense array once per video from the annotation file with a Python loop over every frame and every action
(charades_fine.py:110-117, the same lines in charades_coarse_fineFEAT.py:115-122), slices the sample's window out of it
(charades_fine.py:149-165, :188) and zero-pads the batch (mt_collate_fn, charades_fine.py:214-220).  What those three steps give is

    fps = num_frames / duration                        on the host, in Python (fp64); it travels as a double
    fr  = start + t,   start = start_f - 1             window element t of a sample
    labels[c, t] = 1.0  iff  t < length and some segment (c, s, e) has  fr / fps > s  and  fr / fps < e       else 0.0
    mask[t]      = 1.0  iff  t < length

``fr / fps`` is that one fp64 division and both inequalities are strict: ``fr * (1 / fps)`` or ``fr * duration / num_frames`` round
differently where a frame time meets a segment bound.  The kernel, ``SegLabel.dense_reference`` and ``SegLabels.dense_reference`` all spell
exactly this, so they agree with the reference bit for bit (tests/golden/seg_labels.npz).

Limits: the 'loc' task only (the 'class' task reduces the window over time on the host); one class count per batch; ``SegLabels.dense()``
has no CPU path (``dense_reference()`` is the statement of the result on any device).

This module is host only (numpy + torch); ``SegLabels.dense`` is the one call that needs the GPU library.
"""
import collections
import math

import numpy as np
import torch

N_CLASSES = 157


class SegLabel(object):
    """The label member of ONE sample: ``actions`` (S, 3) float64 rows [class, start_s, end_s] (the annotation record's 'actions'),
    ``fps`` = num_frames / duration, ``start`` = first frame of the window (start_f - 1), ``length`` = frames of the window,
    ``n_classes``.  Plain Python and numpy: cheap to pickle between DataLoader workers."""
    __slots__ = ('actions', 'fps', 'start', 'length', 'n_classes')

    def __init__(self, actions, fps, start, length, n_classes=N_CLASSES):
        a = np.asarray(actions if len(actions) else np.zeros((0, 3)), dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError('actions: rows [class, start_s, end_s] expected, got an array of shape %s' % (a.shape,))
        self.actions = np.ascontiguousarray(a)
        self.fps, self.start, self.length, self.n_classes = float(fps), int(start), int(length), int(n_classes)

    @classmethod
    def training(cls, actions, num_frames, duration, start_f, frames, n_classes=N_CLASSES):
        """the training window of Charades.__getitem__ (charades_fine.py:155-165): `frames` labels from frame start_f - 1, cut by the end
        of the video.  start_f is the 1-based first frame the Dataset drew (random.randint(1, max(gamma_tau, num_frames - frames)))."""
        start = int(start_f) - 1
        return cls(actions, num_frames / duration, start, max(min(int(frames), int(num_frames) - start), 0), n_classes)

    @classmethod
    def testing(cls, actions, num_frames, duration, gamma_tau, n_classes=N_CLASSES):
        """the testing window of the 'loc' task (charades_fine.py:152-153, :188): the whole video from frame 0, cut to a multiple of the
        Dataset's frame stride `gamma_tau` (the reference's self.gamma_tau, twice its constructor argument)"""
        return cls(actions, num_frames / duration, 0, (int(num_frames) // int(gamma_tau)) * int(gamma_tau), n_classes)

    def dense_reference(self):
        """the (n_classes, length) float32 array the reference's Dataset returns for this window, from the definition (numpy)"""
        lab = np.zeros((self.n_classes, self.length), np.float32)
        x = np.arange(self.start, self.start + self.length).astype(np.float64) / np.float64(self.fps)
        for c, s, e in self.actions:
            lab[int(c), (x > s) & (x < e)] = 1.0
        return lab

    def __getstate__(self):
        return (self.actions, self.fps, self.start, self.length, self.n_classes)

    def __setstate__(self, st):
        self.actions, self.fps, self.start, self.length, self.n_classes = st

    def __repr__(self):
        return 'SegLabel(%d segments, fps=%r, start=%d, length=%d, n_classes=%d)' % (len(self.actions), self.fps, self.start, self.length,
                                                                                      self.n_classes)


class SegLabels(collections.namedtuple('SegLabels', ['seg', 'offsets', 'fps', 'window', 'n_classes', 't_max'])):
    """A batch of segment labels: ``seg`` (S, 3) float64, every sample's rows [class, start_s, end_s] back to back (never empty: a batch
    without any segment holds one padding row that no offset range covers); ``offsets`` (B + 1,) int32: sample b owns rows
    offsets[b]:offsets[b + 1]; ``fps`` (B,) float64; ``window`` (B, 2) int32 = start, length; ``n_classes`` and ``t_max`` = max(length) as
    HOST ints (dense() never reads the device for them).

    Stands for the pair labels (B, n_classes, t_max) fp32, mask (B, t_max) fp32 of the dense collate.  A namedtuple, like PackedFeats: staging
    and DataLoader pinning rebuild it around the moved tensors."""
    __slots__ = ()

    @property
    def device(self):
        return self.seg.device

    @property
    def batch(self):
        return int(self.fps.shape[0])

    def to(self, device, non_blocking=False):
        """move the four tensors to `device`; the element types are part of the format, so a dtype is refused"""
        if isinstance(device, torch.dtype) or not isinstance(device, (str, int, torch.device)):
            raise TypeError('SegLabels.to() takes a device: seg and fps stay float64, offsets and window int32 (dense() makes the fp32 labels)')
        return SegLabels(self.seg.to(device, non_blocking=non_blocking), self.offsets.to(device, non_blocking=non_blocking),
                         self.fps.to(device, non_blocking=non_blocking), self.window.to(device, non_blocking=non_blocking), self.n_classes,
                         self.t_max)

    def cuda(self, device=None, non_blocking=False):
        if isinstance(device, torch.dtype):
            raise TypeError('SegLabels.cuda() takes a device, not a dtype')
        return SegLabels(self.seg.cuda(device, non_blocking=non_blocking), self.offsets.cuda(device, non_blocking=non_blocking),
                         self.fps.cuda(device, non_blocking=non_blocking), self.window.cuda(device, non_blocking=non_blocking), self.n_classes,
                         self.t_max)

    def dense(self, out=None):
        """(labels (B, n_classes, t_max) fp32, mask (B, t_max) fp32, valid_t (B,) int32) on the data's device and current stream: one kernel
        launch (ops.seg_labels), nothing is read back.  out: the three preallocated tensors -- every element is written and nothing is
        allocated, so the call can be captured in a graph.  No CPU path."""
        from . import ops
        return ops.seg_labels(self.seg, self.offsets, self.fps, self.window, self.n_classes, self.t_max, out=out)

    def dense_reference(self):
        """dense() from the definition in plain torch, on any device: the tests' reference and the CPU spelling"""
        B, C, T, dev = self.batch, int(self.n_classes), int(self.t_max), self.seg.device
        offs, win = self.offsets.tolist(), self.window.tolist()
        labels = torch.zeros(B, C, T, dtype=torch.float32, device=dev)
        mask = torch.zeros(B, T, dtype=torch.float32, device=dev)
        valid = torch.zeros(B, dtype=torch.int32, device=dev)
        for b in range(B):
            start, n = win[b][0], min(max(win[b][1], 0), T)
            x = torch.arange(start, start + n, dtype=torch.float64, device=dev) / self.fps[b]
            for c, s, e in self.seg[offs[b]:offs[b + 1]].tolist():
                if 0 <= c < C and c == int(c):
                    labels[b, int(c), :n][(x > s) & (x < e)] = 1.0
            mask[b, :n] = 1.0
            valid[b] = n
        return labels, mask, valid


def collate_seg(samples):
    """[SegLabel] -> SegLabels on the host.  Raises on mixed class counts, a class that is not an integer of [0, n_classes), a negative
    start or length, or an fps that is not a positive finite number."""
    if not samples:
        raise ValueError('an empty batch')
    for s in samples:
        if not isinstance(s, SegLabel):
            raise ValueError('the label members of a batch are either all dense arrays or all cfn_hip.seglabels.SegLabel, got %s' % type(s).__name__)
    C = samples[0].n_classes
    if C < 1 or any(s.n_classes != C for s in samples):
        raise ValueError('one positive class count per batch expected, got %s' % [s.n_classes for s in samples])
    for s in samples:
        cls = s.actions[:, 0]
        if not np.all((cls >= 0) & (cls < C) & (cls == np.floor(cls))):      # (a NaN fails every comparison)
            raise ValueError('segment classes must be integers of [0, %d), got %s' % (C, cls.tolist()))
        if s.start < 0 or s.length < 0:
            raise ValueError('a window starts at frame >= 0 and has a length >= 0, got start %d, length %d' % (s.start, s.length))
        if not (s.fps > 0 and math.isfinite(s.fps)):
            raise ValueError('fps = num_frames / duration must be positive and finite, got %r' % (s.fps,))
    t_max = max(s.length for s in samples)
    if t_max < 1:
        raise ValueError('no sample of the batch has a frame in its window')
    counts = [len(s.actions) for s in samples]
    if sum(counts):
        seg = torch.from_numpy(np.concatenate([s.actions for s in samples], 0))
    else:                                                                      # (staging leaves zero-element tensors on the host)
        seg = torch.tensor([[-1.0, 0.0, 0.0]], dtype=torch.float64)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    fps = torch.tensor([s.fps for s in samples], dtype=torch.float64)
    window = torch.tensor([[s.start, s.length] for s in samples], dtype=torch.int32)
    return SegLabels(seg, offsets, fps, window, C, t_max)


def materialize(labels, masks, device):
    """the label and mask members of a batch -> dense (labels (B, C, TL) fp32, mask (B, TL) fp32) on `device`: a SegLabels batch is moved
    there (a no-op on a staged batch) and expanded by the kernel; dense tensors pass through untouched except for .to(device)"""
    if isinstance(labels, SegLabels):
        lab, mask, _ = labels.to(device).dense()
        return lab, mask
    return labels.to(device), masks.to(device)
