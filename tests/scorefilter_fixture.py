"""What the score-filter tests share (cfn_hip/scorefilter.py, rules F1-F6): the three score fixtures, made once and left unchanged, the naive
per-frame spelling of the rule that filter_reference is checked against, and the comparison by bits."""
import functools

import numpy as np
import torch

QNAN = 0x7fc00000


@functools.lru_cache(maxsize=None)
def scores(kind, B, C, TL, seed=0):
    """(B, C, TL) float32, read-only.  'random': uniform [0, 1).  'quantised': multiples of 1/8 in [0, 1] with both zeros, so a median window is
    full of ties (and every median, a value or the midpoint of two, is a multiple of 1/16).  'wide': |values| spanning 2^-120 .. 1 with a
    sprinkle of fp32 subnormals, both signs, and one frame in ten followed by its own negative.  An fp64 sum of fp32 values carries 29 spare
    bits, so its order alone reaches the fp32 result about once in 2^23 outputs; it shows through CANCELLATION: 1 - 1 + 2^-60 keeps the small
    term, 2^-60 - 1 + 1 loses it.  The planted pairs make that common, and a kernel that sums a window in another order cannot pass."""
    rng = np.random.RandomState(1000 * seed + 7 * B + 13 * C + TL + {'random': 0, 'quantised': 1, 'wide': 2}[kind])
    if kind == 'random':
        a = rng.random_sample((B, C, TL)).astype(np.float32)
    elif kind == 'quantised':
        a = (rng.randint(0, 9, (B, C, TL)) / 8.0).astype(np.float32)
        a[(a == 0) & (rng.random_sample(a.shape) < 0.5)] = np.float32(-0.0)
    else:
        mant = 1.0 + rng.random_sample((B, C, TL))
        a = (mant * np.exp2(-rng.randint(1, 121, (B, C, TL)).astype(np.float64))).astype(np.float32)
        sub = rng.random_sample(a.shape) < 0.05
        a[sub] = (rng.randint(1, 1 << 22, int(sub.sum())).astype(np.uint32)).view(np.float32)      # fp32 subnormals
        a[rng.random_sample(a.shape) < 0.3] *= np.float32(-1.0)
        if TL > 1:
            pair = np.flatnonzero(rng.random_sample(a.shape[:2] + (TL - 1,)).reshape(-1) < 0.1)
            b_, c_, t_ = np.unravel_index(pair, a.shape[:2] + (TL - 1,))
            big = ((1.0 + rng.random_sample(pair.size)) * np.exp2(-rng.randint(1, 4, pair.size).astype(np.float64))).astype(np.float32)
            a[b_, c_, t_] = big
            a[b_, c_, t_ + 1] = -a[b_, c_, t_]
    a.setflags(write=False)
    return a


def naive(p, valid_t, radius, weights, method, descending=False):
    """rules F1-F6 frame by frame in plain Python floats (IEEE fp64) -> (B, C, TL) float32.  p (B, C, TL) float32; radius (C,) ints, weights
    (C, R + 1) fp64, method 0 | 1.  descending=True sums F4's window from its last frame to its first: NOT the rule, the fixture-premise test's
    other order."""
    B, C, TL = p.shape
    R = weights.shape[1] - 1
    out = p.copy()
    bits = out.view(np.uint32)
    for b in range(B):
        n = min(max(int(valid_t[b]), 0), TL)
        for c in range(C):
            r = min(max(int(radius[c]), 0), R)
            if r == 0:
                continue
            for t in range(n):
                us = list(range(max(0, t - r), min(n - 1, t + r) + 1))
                vals = [p[b, c, u] for u in us]
                if not all(np.isfinite(v) for v in vals):
                    bits[b, c, t] = QNAN
                    continue
                if method == 0:
                    num = den = 0.0
                    for u in (reversed(us) if descending else us):
                        w = float(weights[c, abs(u - t)])
                        num = num + w * float(p[b, c, u])
                        den = den + w
                    q = np.float32(np.float64(num) / np.float64(den))
                else:
                    rank = [sum(1 for j, pv in enumerate(vals) if pv < pu or (pv == pu and j < i)) for i, pu in enumerate(vals)]
                    by_rank = {k: v for k, v in zip(rank, vals)}
                    m = len(vals)
                    q = by_rank[(m - 1) // 2] if m % 2 else np.float32((np.float64(by_rank[m // 2 - 1]) + np.float64(by_rank[m // 2])) * 0.5)
                out[b, c, t] = q
    return out


def same_bits(got, want):
    """two float32 arrays / tensors, equal as BITS (so NaNs by position and payload, and the sign of a zero)"""
    g = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    w = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert g.dtype == np.float32 and w.dtype == np.float32 and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    diff = np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
    assert not diff.any(), '%d of %d elements differ in their bits, first at %s' % (int(diff.sum()), diff.size, tuple(np.argwhere(diff)[0]))
