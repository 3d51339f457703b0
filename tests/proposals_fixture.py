"""Inputs for the proposal tests (test_proposals_cpu.py, test_hip_proposals.py): per-frame scores whose levels cut segments of different
widths, and candidate lists built on the host with a chosen number of rows per (video, class) group.  Nothing here needs a GPU."""
import numpy as np
import torch

import segap_fixture as fx

LEVELS5 = (0.8, 0.65, 0.5, 0.35, 0.2)


def random_probs(seed, B, C, TL, noise=0.15):
    """smooth bumps plus noise in [0, 1]: a level cuts a bump at its own width, the noise splits the runs near a level"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(TL, dtype=torch.float32)
    p = noise * torch.rand(B, C, TL, generator=g)
    for b in range(B):
        for c in range(C):
            for _ in range(int(torch.randint(0, 4, (1,), generator=g))):
                mid, wid = float(torch.rand(1, generator=g)) * TL, 2.0 + float(torch.rand(1, generator=g)) * TL / 6
                p[b, c] += float(0.3 + 0.6 * torch.rand(1, generator=g)) * torch.exp(-((t - mid) / wid) ** 2)
    return p.clamp_(0.0, 1.0)


def candidates(seed, groups, n_classes, span=100.0):
    """groups: per video a dict {class: rows} -> a Detections on the host with that many candidates per (video, class) group: starts and
    lengths on a grid of quarter seconds (equal segments and tIoU ties occur), both scores on a grid of eighths (score ties occur), rows in
    (class, start) order as a decode leaves them"""
    rng = np.random.RandomState(seed)
    videos = []
    for per_class in groups:
        rows = []
        for c, n in sorted(per_class.items()):
            start = np.sort(0.25 * rng.randint(0, int(span * 4), n))
            length = 0.25 * rng.randint(1, 60, n)
            rows += [(c, float(s), float(s + w), float(rng.randint(1, 8)) / 8.0, float(rng.randint(1, 8)) / 8.0) for s, w in zip(start, length)]
        videos.append(rows)
    det = fx.make_det(videos, n_classes)
    return det._replace(frames=torch.arange(3 * det.seg.shape[0], dtype=torch.int32).reshape(-1, 3))       # (something to copy)
