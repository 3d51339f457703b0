"""Batches for the segment-AP tests (test_segap_cpu.py, test_hip_segap.py): Detections and SegLabels built on the host from typed-out rows,
the hand batch both files share, random batches and the golden annotation records.  Nothing here needs a GPU."""
import numpy as np
import torch

import seg_fixture as sf


def make_det(videos, n_classes):
    """videos: per video a list of (class, start, end, score_max, score_mean) -> a Detections on the host, rows ordered by (video, class,
    start) as decode leaves them (the sort is stable: equal starts keep the order given)"""
    from cfn_hip.detections import Detections
    seg, score, offsets = [], [], [0]
    for rows in videos:
        for c, s, e, mx, mean in sorted(rows, key=lambda r: (r[0], r[1])):
            seg.append([float(c), float(s), float(e)])
            score.append([mx, mean])
        offsets.append(len(seg))
    total = len(seg)
    n = max(total, 1)
    seg_t, score_t = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 2, dtype=torch.float32)
    if total:
        seg_t[:total] = torch.tensor(seg, dtype=torch.float64)
        score_t[:total] = torch.tensor(score, dtype=torch.float32)
    return Detections(seg_t, torch.zeros(n, 3, dtype=torch.int32), score_t, torch.tensor(offsets, dtype=torch.int32),
                      torch.tensor([total], dtype=torch.int32), int(n_classes), n)


def make_gt(videos, fps, windows, n_classes, t_max=None):
    """videos: per video a list of (class, start_s, end_s) in annotation order -> a SegLabels on the host (classes are NOT checked: the tests
    hand over rows collate_seg would refuse)"""
    from cfn_hip.seglabels import SegLabels
    rows = [list(map(float, r)) for v in videos for r in v]
    seg = torch.tensor(rows, dtype=torch.float64) if rows else torch.tensor([[-1.0, 0.0, 0.0]], dtype=torch.float64)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(v) for v in videos])]), dtype=torch.int32)
    window = torch.tensor(windows, dtype=torch.int32).reshape(len(videos), 2)
    t_max = int(window[:, 1].max()) if t_max is None else int(t_max)
    return SegLabels(seg, offsets, torch.tensor(fps, dtype=torch.float64), window, int(n_classes), t_max)


HAND_TIOU = (0.5,)


def hand_batch():
    """B = 3, C = 5: the hand cases of test_segap_cpu.py and the edge inputs in one batch.

    video 0 (fps 1, window [0, 100): w0 = -0.5, w1 = 99.5)
      class 0: rows (0, 10), (20, 30); detections (0, 10) 0.9 TP, (20, 30) 0.7 TP, (50, 60) 0.8 FP; also rows with e <= s: (70, 70), (80, 75)
               and a row (200, 300) the window clips away
      class 1: rows g0 (0, 10), g1 (2, 12); detections (2, 12) 0.9 -> best tIoU g1 (1.0; first found would be g0 at 8/12), then (-4, 8) 0.8
               -> g0 at 8/14 (g1 at 6/16 is below 0.5): best-first gives two true positives, first-found one
      class 4: row (40, 50) and no detection: AP 0, counted in map
      rows of classes 7, 2.5 and -1: outside [0, C)
    video 1 (fps 2, window [10, 60): w0 = 4.75, w1 = 29.75)
      class 2: rows (5, 10) twice; detections (5, 10) 0.9 -> the lower row, (5, 10) 0.6 -> the other (a tIoU tie)
      class 3: row (25, 40) clipped to (25, 29.75), detection (25, 29.75) 0.8: tIoU 1; rows (0, 4.75) and (0, 4) clipped away
      class 0: row (12, 22); detections (12, 22) 0.5 and (13, 22) 0.5: the score tie goes to the lower row, which takes the row
    video 2 (fps 1, window [0, 100)): no ground truth; detections of classes 0 (0.99) and 3 (0.3): false positives

    n_gt = [3, 2, 2, 1, 1].  At 0.5, class 0 sorted: 0.99 FP, 0.9 TP, 0.8 FP, 0.7 TP, 0.5 TP, 0.5 FP -> (1/2 + 2/4 + 3/5) / 3; classes 1, 2, 3:
    1; class 4: 0."""
    C = 5
    det = make_det([
        [(0, 0, 10, 0.9, 0.1), (0, 20, 30, 0.7, 0.2), (0, 50, 60, 0.8, 0.3), (1, 2, 12, 0.9, 0.4), (1, -4, 8, 0.8, 0.5)],
        [(2, 5, 10, 0.9, 0.6), (2, 5, 10, 0.6, 0.7), (3, 25, 29.75, 0.8, 0.8), (0, 12, 22, 0.5, 0.9), (0, 13, 22, 0.5, 0.95)],
        [(0, 1, 5, 0.99, 0.05), (3, 2, 6, 0.3, 0.15)],
    ], C)
    gt = make_gt([
        [(7, 0, 10), (0, 0, 10), (1, 0, 10), (0, 70, 70), (2.5, 0, 10), (0, 20, 30), (1, 2, 12), (0, 80, 75), (4, 40, 50), (-1, 0, 10), (0, 200, 300)],
        [(2, 5, 10), (3, 25, 40), (2, 5, 10), (3, 0, 4.75), (0, 12, 22), (3, 0, 4)],
        [],
    ], [1.0, 2.0, 1.0], [[0, 100], [10, 50], [0, 100]], C)
    return det, gt


def random_batch(seed, B, C, n_det, n_gt, t_max=200, half=True):
    """a random batch: per video up to n_det detections and n_gt ground-truth rows over C classes, times on a grid of half seconds so that
    tIoU ties and exact bounds occur; some rows reach past the window, some are empty, some scores tie"""
    rng = np.random.RandomState(seed)
    fps = (rng.randint(2, 6, B) * 6.0).tolist()
    windows = [[int(rng.randint(0, 50)), int(rng.randint(t_max // 2, t_max + 1))] for _ in range(B)]
    dets, gts = [], []
    for b in range(B):
        lo, hi = windows[b][0] / fps[b], (windows[b][0] + windows[b][1]) / fps[b]
        step = 0.5 if half else 0.125

        def span():
            s = lo - 1.0 + step * rng.randint(0, int((hi - lo + 2.0) / step))
            return s, s + step * rng.randint(0 if rng.rand() < 0.1 else 1, 8)
        gts.append([(int(rng.randint(0, C)),) + span() for _ in range(rng.randint(0, n_gt + 1))])
        rows, seen = [], set()
        for _ in range(rng.randint(0, n_det + 1)):
            c, (s, e) = int(rng.randint(0, C)), span()
            if e > s and (c, s) not in seen:                                          # (decode gives one segment per (class, t0))
                seen.add((c, s))
                rows.append((c, s, e, float(rng.randint(1, 6)) / 8.0, float(rng.rand())))
        dets.append(rows)
    return make_det(dets, C), make_gt(gts, fps, windows, C, t_max)


def golden_labels(split):
    """the 42 annotation records of tests/golden/seg_labels.npz in their `split` windows as ONE SegLabels batch (videos whose window is
    empty stay in the batch: they have no frame and their rows do not participate)"""
    from cfn_hip.seglabels import collate_seg
    return collate_seg([sf.seglabel(i, split) for i in range(len(sf.records()))])
