"""Temporal filtering of per-frame scores in front of the decode: ``probs (B, C, TL)`` -> ``out (B, C, TL)``, a box, Gaussian or median filter
over a per-class window (cfn_hip.ops.score_filter, csrc/scorefilter.hip).

Raw sigmoid scores flicker from frame to frame, and rule 1 of ``cfn_hip.detections.decode`` then breaks one activity into many runs.  The
repairs ``decode`` offers, ``max_gap`` and ``min_len``, are morphological, act behind the threshold and take one setting for all classes;
the ordinary lever, smoothing the scores BEFORE they are thresholded, every caller had to write in torch with an edge rule of their own.
This is the one rule.  The kernel, ``filter_reference`` below and include/cfn_hip.h spell the same.  Inputs ``probs (B, C, TL)`` fp32,
``valid_t (B,)`` int32, ``radius (C,)`` int32, ``weights (C, R + 1)`` fp64, host ints ``R`` with 0 <= R <= 32 (windows of at most 65
frames) and ``method`` (0 = weighted mean, 1 = median); output ``out (B, C, TL)`` fp32, which must not alias ``probs``:

    F1. n = min(max(valid_t[b], 0), TL) and r = min(max(radius[c], 0), R).  Frames t >= n are copied from probs bit for bit; r = 0 copies
        every frame bit for bit, under either method
    F2. the window of frame t < n is u in [max(0, t - r), min(n - 1, t + r)]: truncated at the valid range; no padding, no reflection
    F3. a window that holds a non-finite value gives the canonical quiet NaN 0x7fc00000, which ``decode`` never activates (rule 1 there is a
        strict comparison); so does a weighted mean whose quotient is a NaN, which the tables of ``filter_weights`` cannot give
    F4. weighted mean, u ascending throughout: num = the sum of weights[c, |u - t|] * float64(probs[b, c, u]), den = the sum of
        weights[c, |u - t|], both from 0.0; every product and every sum is rounded separately (no fused multiply-add); then ONE IEEE fp64
        division and ONE rounding to fp32.  The box filter is the table of ones, so one code path serves both; the Gaussian table is made on
        the HOST by ``filter_weights``, exp(-d * d / (2 * sigma * sigma)) in numpy with weights[c, 0] == 1.0: neither side's device exp is
        involved
    F5. median: the window ordered by (value, u): the rank of u is #{v : p[v] < p[u] or (p[v] == p[u] and v < u)} -- numpy's stable
        argsort, so +0 / -0 ties are decided.  For m window frames, m odd gives the element of rank (m - 1) / 2; m even gives
        float32((float64(a) + float64(b)) * 0.5) with a and b the elements of ranks m / 2 - 1 and m / 2
    F6. no atomics and no read-back: the bits are the same in every run

``ScoreFilter(method, radius, sigma)`` is the host description ('box' | 'gaussian' | 'median', a radius and a sigma per class or one for
all); ``.tensors(n_classes, device)`` builds the device tensors once.  ``apply`` is the one call that needs the GPU library (one launch,
one thread per frame, the median by rank counting over the window in LDS: O(window^2) per frame); ``filter_reference`` spells F1-F6 in numpy
on any device and is the tests' reference.  ``decode``, ``decode_levels``, ``propose``, ``DetectionWriter`` and ``SegmentAPMeter`` take the
filter as ``filter=``, and so do their references.  Limits: B and C <= 65535, TL <= 65536, R <= 32; no CPU path for the operator.  No accuracy
gain is claimed: whether a filter, which one, and which window help a trained model is for the user to find with the meters.  Out of scope:
hysteresis thresholds, composing two filters in one call.

This module is host only (numpy + torch) apart from ``apply``.
"""
import math

import numpy as np
import torch

MAX_RADIUS = 32
METHODS = {'box': 0, 'gaussian': 0, 'median': 1}                                      # -> the kernel's method: 0 weighted mean, 1 median
SIGMA_RANGE = (1.0 / 64.0, float(1 << 20))
QNAN_BITS = 0x7fc00000


def _per_class(name, v, kind):
    """a scalar or a sequence -> (tuple of host numbers, True if it was a scalar)"""
    if torch.is_tensor(v):
        v = v.detach().cpu().tolist()
    elif isinstance(v, np.ndarray):
        v = v.tolist()
    scalar = not isinstance(v, (list, tuple))
    vals = [v] if scalar else list(v)
    if not vals:
        raise ValueError('%s: a number or a non-empty per-class sequence expected, got %r' % (name, v))
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, (int,) if kind is int else (int, float)):
            raise ValueError('%s: %s expected, got %r' % (name, 'ints' if kind is int else 'numbers', x))
    return tuple(kind(x) for x in vals), scalar


def filter_weights(method, radius, sigma=None):
    """the weight table of rule F4 on the host: radius (C,) ints (or one int), sigma (C,) floats (or one; 'gaussian' only) -> (C, R + 1) fp64
    with R = max(radius): ones for 'box' (and for 'median', which does not read it), exp(-d * d / (2 * sigma * sigma)) for 'gaussian' -- numpy
    float64, so weights[:, 0] == 1.0 exactly, 0 <= weights <= 1, not increasing in d.  Entries behind a class's own radius are never read."""
    if method not in METHODS:
        raise ValueError("method: 'box', 'gaussian' or 'median' expected, got %r" % (method,))
    r = np.atleast_1d(np.asarray(radius, np.int64))
    if r.ndim != 1 or r.size < 1 or r.min() < 0 or r.max() > MAX_RADIUS:
        raise ValueError('radius: ints of [0, %d] expected, got %r' % (MAX_RADIUS, radius))
    R = int(r.max())
    if method != 'gaussian':
        if sigma is not None:
            raise ValueError("sigma belongs to 'gaussian', not to %r" % (method,))
        return np.ones((r.size, R + 1), np.float64)
    s = np.atleast_1d(np.asarray(sigma, np.float64)) if sigma is not None else None
    if s is None or s.ndim != 1 or s.size not in (1, r.size) or not np.all((s >= SIGMA_RANGE[0]) & (s <= SIGMA_RANGE[1])):
        raise ValueError("sigma: %s floats of [1/64, 2^20] expected for 'gaussian', got %r" % ('one or %d' % r.size, sigma))
    s = np.broadcast_to(s, (r.size,))[:, None]
    d = np.arange(R + 1, dtype=np.float64)[None, :]
    with np.errstate(under='ignore'):
        return np.ascontiguousarray(np.exp(-(d * d) / (2.0 * s * s)))


class ScoreFilter(object):
    """The host description of a temporal filter (see the module text).  method: 'box' | 'gaussian' | 'median'.  radius: frames on each side,
    an int of [0, 32] or a per-class sequence of them (0: the class passes through); with 'gaussian' None means ceil(3 * sigma), capped at 32.
    sigma ('gaussian' only): a float of [1/64, 2^20] or a per-class sequence.  Out-of-range values raise ValueError.  Two filters are equal
    when the three are."""

    def __init__(self, method, radius=None, sigma=None):
        if method not in METHODS:
            raise ValueError("ScoreFilter: method 'box', 'gaussian' or 'median' expected, got %r" % (method,))
        self.method = method
        self.sigma = self._sigma_scalar = None
        if method == 'gaussian':
            if sigma is None:
                raise ValueError("ScoreFilter: 'gaussian' needs sigma")
            self.sigma, self._sigma_scalar = _per_class('ScoreFilter: sigma', sigma, float)
            if any(not SIGMA_RANGE[0] <= s <= SIGMA_RANGE[1] for s in self.sigma):            # (a NaN fails both comparisons)
                raise ValueError('ScoreFilter: sigma in [1/64, 2^20] expected, got %r' % (sigma,))
            if radius is None:
                radius = [min(int(math.ceil(3.0 * s)), MAX_RADIUS) for s in self.sigma]
                radius = radius[0] if self._sigma_scalar else radius
        elif sigma is not None:
            raise ValueError("ScoreFilter: sigma belongs to 'gaussian', not to %r" % (method,))
        if radius is None:
            raise ValueError('ScoreFilter: %r needs a radius' % (method,))
        self.radius, self._radius_scalar = _per_class('ScoreFilter: radius', radius, int)
        if any(not 0 <= r <= MAX_RADIUS for r in self.radius):
            raise ValueError('ScoreFilter: radius in [0, %d] expected (windows of at most %d frames), got %r' % (MAX_RADIUS, 2 * MAX_RADIUS + 1, radius))
        if self.sigma is not None and not self._sigma_scalar and not self._radius_scalar and len(self.sigma) != len(self.radius):
            raise ValueError('ScoreFilter: %d radii but %d sigmas' % (len(self.radius), len(self.sigma)))
        self._cache = {}

    @property
    def code(self):
        """the kernel's method: 0 = weighted mean ('box', 'gaussian'), 1 = median"""
        return METHODS[self.method]

    def _key(self):
        return self.method, self.radius, self._radius_scalar, self.sigma, self._sigma_scalar

    def __eq__(self, other):
        return isinstance(other, ScoreFilter) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'ScoreFilter(%r, radius=%r%s)' % (self.method, self.radius[0] if self._radius_scalar else list(self.radius),
                                                 '' if self.sigma is None else ', sigma=%r' % (self.sigma[0] if self._sigma_scalar else list(self.sigma),))

    @property
    def spec(self):
        """the filter as --detect-smooth spells it (one radius and one sigma for all classes only): parse_spec(flt.spec) == flt"""
        if not self._radius_scalar or (self.sigma is not None and not self._sigma_scalar):
            raise ValueError('%r: per-class values have no command-line spelling' % (self,))
        if self.method == 'gaussian':
            return 'gaussian:%r:%d' % (self.sigma[0], self.radius[0])
        return '%s:%d' % (self.method, self.radius[0])

    def arrays(self, n_classes):
        """(radius (C,) int32, weights (C, R + 1) fp64, the kernel's method) as numpy: what filter_reference and tensors() are made from"""
        C = int(n_classes)
        if C < 1:
            raise ValueError('ScoreFilter: n_classes >= 1 expected, got %r' % (n_classes,))
        for name, vals, scalar in (('radii', self.radius, self._radius_scalar), ('sigmas', self.sigma, self._sigma_scalar)):
            if vals is not None and not scalar and len(vals) != C:
                raise ValueError('ScoreFilter: %d %s for %d classes' % (len(vals), name, C))
        radius = np.full(C, self.radius[0], np.int32) if self._radius_scalar else np.asarray(self.radius, np.int32)
        sigma = None if self.sigma is None else (np.full(C, self.sigma[0], np.float64) if self._sigma_scalar else np.asarray(self.sigma, np.float64))
        return radius, filter_weights(self.method, radius, sigma), self.code

    def tensors(self, n_classes, device):
        """(radius (C,) int32, weights (C, R + 1) fp64) on `device` and the kernel's method, built once per class count and device"""
        key = (int(n_classes), torch.device(device))
        if key not in self._cache:
            radius, weights, code = self.arrays(n_classes)
            self._cache[key] = (torch.from_numpy(radius).to(key[1]), torch.from_numpy(weights).to(key[1]), code)
        return self._cache[key]


def parse_spec(spec):
    """'box:R' | 'gaussian:SIGMA[:R]' | 'median:R' (the --detect-smooth option) -> a ScoreFilter; anything else raises ValueError"""
    form = "box:R | gaussian:SIGMA[:R] | median:R expected (R an int of [0, %d], SIGMA a float of [1/64, 2^20])" % MAX_RADIUS
    parts = str(spec).split(':')
    method = parts[0]
    try:
        if method in ('box', 'median') and len(parts) == 2:
            return ScoreFilter(method, int(parts[1]))
        if method == 'gaussian' and len(parts) in (2, 3):
            return ScoreFilter(method, int(parts[2]) if len(parts) == 3 else None, float(parts[1]))
    except ValueError as e:
        raise ValueError('%r: %s (%s)' % (spec, form, e))
    raise ValueError('%r: %s' % (spec, form))


def _filter_arrays(flt, n_classes):
    """a ScoreFilter, or the raw triple (radius (C,), weights (C, R + 1), method 0 | 1) of tensors or arrays -> the triple as numpy"""
    if isinstance(flt, ScoreFilter):
        return flt.arrays(n_classes)
    if not isinstance(flt, (tuple, list)) or len(flt) != 3:
        raise TypeError('a cfn_hip.scorefilter.ScoreFilter (or the triple radius, weights, method) expected, got %s' % type(flt).__name__)
    radius, weights, method = flt
    radius = np.asarray(radius.detach().cpu().numpy() if torch.is_tensor(radius) else radius).astype(np.int64)
    weights = np.asarray(weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights).astype(np.float64)
    if radius.shape != (n_classes,) or weights.ndim != 2 or weights.shape[0] != n_classes or not 1 <= weights.shape[1] <= MAX_RADIUS + 1:
        raise ValueError('radius (%d,) and weights (%d, R + 1) with 0 <= R <= %d expected, got %s and %s'
                         % (n_classes, n_classes, MAX_RADIUS, radius.shape, weights.shape))
    if method not in (0, 1):
        raise ValueError('method 0 (weighted mean) or 1 (median) expected, got %r' % (method,))
    return radius, weights, int(method)


def apply(probs, valid_t, flt, out=None):
    """probs (B, C, TL) fp32 and valid_t (B,) on the GPU, flt a ScoreFilter -> the filtered (B, C, TL) fp32 tensor there (ops.score_filter:
    one launch, nothing is read back).  out: a preallocated contiguous (B, C, TL) fp32 tensor that does not overlap probs, for a call that
    allocates nothing (capturable once flt.tensors() has been built for the device)."""
    from . import ops
    if not isinstance(flt, ScoreFilter):
        raise TypeError('apply: a cfn_hip.scorefilter.ScoreFilter expected, got %s' % type(flt).__name__)
    if not torch.is_tensor(probs) or probs.dim() != 3:
        raise RuntimeError('apply: probs: a (B, C, TL) float32 tensor expected, got %s' % (tuple(getattr(probs, 'shape', ())),))
    if not probs.is_cuda:
        raise RuntimeError('apply: probs is on %s: there is no CPU path (filter_reference is the host spelling)' % probs.device)
    radius, weights, code = flt.tensors(int(probs.shape[1]), probs.device)
    return ops.score_filter(probs.detach(), valid_t.to(torch.int32), radius, weights, code, out)


def filter_reference(probs, valid_t, flt):
    """apply() from rules F1-F6 in numpy; tensors on any device, the result on probs' device: the tests' reference and the CPU spelling.
    flt: a ScoreFilter, or the raw triple (radius (C,), weights (C, R + 1), method 0 | 1).  F4 loops over the offset d = -R .. R with fp64
    accumulators over whole arrays (d ascending is u ascending for every frame; np.sum's pairwise order would not be F4's)."""
    dev = probs.device
    p = probs.detach().cpu().numpy()
    if p.dtype != np.float32 or p.ndim != 3:
        raise ValueError('probs: a (B, C, TL) float32 tensor expected, got %s %s' % (p.dtype, p.shape))
    B, C, TL = p.shape
    radius, weights, method = _filter_arrays(flt, C)
    R = int(weights.shape[1]) - 1
    r = np.clip(radius.astype(np.int64), 0, R)                                        # F1
    valid = valid_t.detach().cpu().numpy().astype(np.int64).reshape(B)
    out = np.ascontiguousarray(p).copy()
    bits = out.view(np.uint32)                                                        # (results go in as bits: a copy never touches a NaN's payload)
    for b in range(B):
        n = min(max(int(valid[b]), 0), TL)                                            # F1
        if n == 0 or not r.any():
            continue
        x = p[b, :, :n]
        t = np.arange(n)
        finite = np.isfinite(x)
        bad = np.zeros((C, n), bool)
        num, den = np.zeros((C, n), np.float64), np.zeros((C, n), np.float64)
        win = np.full((C, n, 2 * R + 1), np.inf, np.float32) if method == 1 else None # the median's windows, u ascending; +inf where F2 cuts
        for d in range(-R, R + 1):                                                    # F2: u = t + d inside [0, n) and |d| <= r
            u = t + d
            ok = ((u >= 0) & (u < n))[None, :] & (abs(d) <= r)[:, None]
            uc = np.clip(u, 0, n - 1)
            xu = x[:, uc]
            bad |= ok & ~finite[:, uc]                                                # F3
            if method == 0:                                                           # F4: one product, one sum each, separately rounded
                w = weights[:, abs(d)][:, None]
                with np.errstate(all='ignore'):
                    term = w * xu.astype(np.float64)
                    num = np.where(ok, num + term, num)
                    den = np.where(ok, den + w, den)
            else:
                win[:, :, d + R] = np.where(ok, xu, np.float32(np.inf))
        if method == 0:
            with np.errstate(all='ignore'):
                q = (num / den).astype(np.float32)
        else:                                                                         # F5: a stable sort orders by (value, u)
            m = np.isfinite(win).sum(2)                                               # (only windows without a non-finite value are used)
            order = np.argsort(win, axis=2, kind='stable')
            srt = np.take_along_axis(win, order, 2)
            lo = np.take_along_axis(srt, np.maximum((m - 1) // 2, 0)[:, :, None], 2)[:, :, 0]
            hi = np.take_along_axis(srt, (m // 2)[:, :, None], 2)[:, :, 0]
            with np.errstate(all='ignore'):
                mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(np.float32)
            q = np.where(m % 2 == 1, lo, mid)
        qb = np.ascontiguousarray(q).view(np.uint32)
        qb = np.where(bad | np.isnan(q), np.uint32(QNAN_BITS), qb)                    # F3
        bits[b, :, :n] = np.where((r > 0)[:, None], qb, bits[b, :, :n])               # F1: r = 0 keeps the input bits
    return torch.from_numpy(out).to(dev)
