"""Crop, antialiased bilinear resize and horizontal flip of uint8 frames: the host side (tables, crop parameters, a slow reference).

The reference transforms every frame through PIL on the CPU: ``MultiScaleRandomCropMultigrid`` + ``RandomHorizontalFlip`` for
training (train_fine.py:74-77, train_coarse_fineFEAT.py:79-82; transforms/spatial_transforms.py:480-510, :339-357) and
``CenterCropScaled`` for validation and extraction (train_fine.py:78, extract_fineFEAT.py:76; spatial_transforms.py:201-230).
Here the frames travel to the GPU as decoded and ``ops.crop_resize_flip_u8`` (csrc/aug_u8.hip) does that work there.

PIL's 8-bit ``Image.resize(size, BILINEAR)`` is integer arithmetic, restated here:

* per axis, for input extent c and output extent S, output index xx reads the taps ``xmin .. xmin + n - 1`` with
  ``scale = c / S``, ``fs = max(scale, 1)``, ``center = (xx + 0.5) * scale``, ``xmin = max(int(center - fs + 0.5), 0)``,
  ``n = min(int(center + fs + 0.5), c) - xmin`` and the triangle weights ``max(0, 1 - |(x + xmin - center + 0.5) / fs|)``,
  normalised by their sum (added in index order) and rounded to 22 fractional bits: ``k = int(w * 2^22 + 0.5)``;
* ``out = clip8((2^21 + sum_x in[xmin + x] * k_x) >> 22)`` with an int32 accumulator;
* the horizontal pass runs first and ROUNDS to uint8, the vertical pass runs on those bytes;
* the crop is taken first, so the tables depend on (c, S) alone; c == S gives the table [2^22, 0]: the identity.

All of it is double precision on the host (Python floats): the tables are data for the kernel, which only multiplies and shifts.
"""
import math

import numpy as np
import torch

PRECISION_BITS = 22
MAX_TAPS = 9                     # csrc/aug_u8.hip takes tables up to this width: c <= 4 * S
_tables = {}


def table_width(c, S):
    """K = 2 * ceil(max(c / S, 1)) + 1: the widest tap run of the (c, S) table"""
    return 2 * int(math.ceil(max(c / S, 1.0))) + 1


def resample_table(c, S):
    """(bounds (S, 2) int32 = xmin, n;  coef (S, K) int32, zero behind n) of the c -> S resize; cached per (c, S)"""
    c, S = int(c), int(S)
    if c <= 0 or S <= 0:
        raise ValueError('resample_table: positive extents expected, got c = %d, S = %d' % (c, S))
    hit = _tables.get((c, S))
    if hit is not None:
        return hit
    scale = c / S
    fs = max(scale, 1.0)
    support = fs
    K = table_width(c, S)
    bounds = np.zeros((S, 2), dtype=np.int32)
    coef = np.zeros((S, K), dtype=np.int32)
    for xx in range(S):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), c) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        coef[xx, :n] = [int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
    bounds.setflags(write=False)
    coef.setflags(write=False)
    _tables[(c, S)] = (bounds, coef)
    return bounds, coef


def batch_tables(cs, S):
    """the tables of a batch of clips with crop extents `cs`, padded with zero taps to the batch's widest K:
    (bounds (N, S, 2) int32, coef (N, S, K) int32) torch tensors on the host"""
    tabs = [resample_table(c, S) for c in cs]
    K = max(t[1].shape[1] for t in tabs)
    bounds = np.stack([t[0] for t in tabs])
    coef = np.zeros((len(tabs), int(S), K), dtype=np.int32)
    for i, t in enumerate(tabs):
        coef[i, :, :t[1].shape[1]] = t[1]
    return torch.from_numpy(bounds), torch.from_numpy(coef)


def train_crop_params(rng, hw, scales, size=None):
    """(x1, y1, c, flip) of one training clip of h x w frames, drawn from `rng` (a random.Random or the random module) in the
    reference's order -- randint for the scale, random() for x, random() for y (MultiScaleRandomCropMultigrid.randomize_parameters),
    then random() for the flip (RandomHorizontalFlip) -- so a loader seeded like the reference's augments identically.
    `size` (the output extent) does not enter the box; when given, a crop the kernel cannot take (c > 4 * size) is refused here."""
    h, w = int(hw[0]), int(hw[1])
    scale = scales[rng.randint(0, len(scales) - 1)]
    tl_x = rng.random()
    tl_y = rng.random()
    p = rng.random()
    c = int(min(h, w) * scale)
    x1 = int(tl_x * (w - c))
    y1 = int(tl_y * (h - c))
    if size is not None and c > 4 * int(size):
        raise ValueError('train_crop_params: a %d pixel crop into %d is more than the 4x reduction crop_resize_flip_u8 takes' % (c, size))
    return x1, y1, c, int(p < 0.5)


def center_crop_params(hw):
    """(x1, y1, c, 0) of CenterCropScaled on h x w frames (its rounding: int(round((w - c) / 2.)))"""
    h, w = int(hw[0]), int(hw[1])
    c = min(w, h)
    return int(round((w - c) / 2.)), int(round((h - c) / 2.)), c, 0


def _resample_axis(a, bounds, coef, axis):
    """one pass along `axis` of an int64 array of bytes"""
    S, K = coef.shape
    c = a.shape[axis]
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(K)[None, :], c - 1)            # (S, K); taps behind n have zero weight
    g = np.take(a, idx.reshape(-1), axis=axis)
    g = g.reshape(a.shape[:axis] + (S, K) + a.shape[axis + 1:])
    wshape = [1] * g.ndim
    wshape[axis], wshape[axis + 1] = S, K
    acc = (g * coef.astype(np.int64).reshape(wshape)).sum(axis=axis + 1) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255)


def resize_u8_reference(frames, box, S, lengths=None):
    """Slow CPU emulation of ops.crop_resize_flip_u8, and the statement of its arithmetic: frames (N, T, Hs, Ws, 3) uint8,
    box (N, 4) = x1, y1, c, flip -> (N, T, S, S, 3) uint8 (torch); frames t >= lengths[n] are zero bytes."""
    f = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    b = box.cpu().numpy() if torch.is_tensor(box) else np.asarray(box)
    if f.dtype != np.uint8 or f.ndim != 5 or f.shape[4] != 3:
        raise ValueError('resize_u8_reference: uint8 frames (N, T, Hs, Ws, 3) expected')
    N, T = f.shape[:2]
    b = b.reshape(N, 4)
    S = int(S)
    out = np.zeros((N, T, S, S, 3), dtype=np.uint8)
    for n in range(N):
        x1, y1, c, flip = (int(v) for v in b[n])
        if c <= 0 or x1 < 0 or y1 < 0 or x1 + c > f.shape[3] or y1 + c > f.shape[2]:
            raise ValueError('resize_u8_reference: box %s outside the %d x %d frames' % ((x1, y1, c), f.shape[2], f.shape[3]))
        live = T if lengths is None else int(lengths[n])
        win = f[n, :live, y1:y1 + c, x1:x1 + c].astype(np.int64)
        if c != S:                                       # an axis whose extent does not change is the identity
            bounds, coef = resample_table(c, S)
            win = _resample_axis(win, bounds, coef, 2)   # horizontal first, rounded to bytes
            win = _resample_axis(win, bounds, coef, 1)
        if flip:
            win = win[:, :, ::-1]
        out[n, :live] = win.astype(np.uint8)
    return torch.from_numpy(out)
