"""Inputs and a second spelling of the rule for the soft-NMS tests (test_softnms_cpu.py, test_hip_softnms.py).  Nothing here needs a GPU.

``soft_loop`` is rules S1-S7 of cfn_hip/detections.py written row by row with scalar fp64 arithmetic and ``tiou_reference``: slow, obvious, and
independent of the vectorised rounds of ``soft_nms_reference``; it also returns the selection order, which the result does not hold."""
import numpy as np
import torch

import segap_fixture as fx
from proposals_fixture import candidates

SIZES = (1, 63, 64, 65, 1023, 1024, 1025)          # a tile of lanes and its neighbours; the LDS tile, its last entry, the workspace path
FLOOR = 0.05                                        # the boundary cases' min_score: both methods drop rows at every size from 63 on


def boundary_batch(nd):
    """B = 2, C = 3 (the batch of test_hip_proposals.py's boundary test): video 0 holds nd candidates of class 0 and 5 of class 2 (class 1
    is empty), video 1 nd of class 1 and one of class 2.  nd = 1 takes a seed whose group of 5 overlaps itself above 0.5"""
    return candidates(3 if nd == 1 else nd, [{0: nd, 2: 5}, {1: nd, 2: 1}], 3, span=max(20.0, nd / 8.0))


SUBNORMAL_KEEP = 12


def subnormal_batch():
    """one group of 16 identical segments, row i with the score 10^-(15 - i): under gaussian, sigma = 1/64, every selected row multiplies the
    rest by E(64) = 1.6e-28, so the row of rank r (row 15 - r) is selected with w = 10^(-28.8 r): 1.5e-317 at rank 11, which is SUBNORMAL
    (below 2.2e-308), and exactly 0 from rank 12 on.  The finals round to 0 in fp32 from rank 2 on, so the subnormal shows in the ORDER alone:
    rank 11 is row 4, the zeros behind it tie and go by row (0, 1, 2, 3).  max_keep = SUBNORMAL_KEEP = 12 therefore keeps rows 4 .. 15; a
    device that flushed the subnormal to 0 would let row 0 win the tie and keep rows 0 and 5 .. 15"""
    return fx.make_det([[(0, 2.0, 9.5, 10.0 ** -(15 - i), 0.5) for i in range(16)]], 1)


def soft_loop(det, soft, nms_thr=0.5, score='max'):
    """-> (keep (n,) uint8, final (n,) float32 of the selected rows (the input score elsewhere), order: the selected rows in selection order,
    group after group)"""
    from cfn_hip.detections import SCORE_COLUMNS, decay_exp_reference
    from cfn_hip.segap import tiou_reference
    method, sigma, floor, max_keep = soft
    col = SCORE_COLUMNS[score]
    seg, sc = det.seg.numpy(), det.score.numpy()
    offs = det.offsets.tolist()
    n = min(offs[-1], det.cap)
    keep, final, order = np.zeros(n, np.uint8), sc[:n, col].copy(), []
    for b in range(len(offs) - 1):
        for c in sorted(set(seg[offs[b]:min(offs[b + 1], n), 0].tolist())):
            rows = [i for i in range(offs[b], min(offs[b + 1], n)) if seg[i, 0] == c]
            w = {i: np.float64(sc[i, col]) for i in rows if np.isfinite(sc[i, col])}
            picked = 0
            while w and not (max_keep > 0 and picked >= max_keep):
                m = min(w, key=lambda i: (-w[i], i))
                if not w[m] >= np.float64(floor):
                    break
                keep[m], final[m] = 1, np.float32(w.pop(m))
                order.append(m)
                picked += 1
                for j in w:
                    iou = tiou_reference(seg[m, 1], seg[m, 2], seg[j, 1], seg[j, 2])
                    with np.errstate(all='ignore'):
                        if method == 'linear':
                            if iou > np.float64(nms_thr):
                                w[j] = w[j] * (np.float64(1.0) - iou)
                        elif iou > 0.0:
                            w[j] = w[j] * np.float64(decay_exp_reference((iou * iou) / np.float64(sigma)))
    return keep, final, order


def first_rows(det, score='max'):
    """the first row of every (video, class) group in hard NMS's order (rule N2: the score descending, ties to the lower row)"""
    from cfn_hip.detections import SCORE_COLUMNS
    col = SCORE_COLUMNS[score]
    seg, sc = det.seg.numpy(), det.score.numpy()
    offs = det.offsets.tolist()
    out = []
    for b in range(len(offs) - 1):
        for c in sorted(set(seg[offs[b]:offs[b + 1], 0].tolist())):
            rows = [i for i in range(offs[b], offs[b + 1]) if seg[i, 0] == c]
            out.append(min(rows, key=lambda i: (-sc[i, col], i)))
    return out


def same_det(a, b, rows=None):
    """two host Detections equal bit for bit over their first `rows` rows (default: total), and in offsets / total"""
    n = int(a.total.item()) if rows is None else rows
    assert a.offsets.tolist() == b.offsets.tolist() and a.total.tolist() == b.total.tolist()
    assert torch.equal(a.seg[:n].view(torch.int64), b.seg[:n].view(torch.int64)) and torch.equal(a.frames[:n], b.frames[:n])
    assert torch.equal(a.score[:n].contiguous().view(torch.int32), b.score[:n].contiguous().view(torch.int32)), 'score differs in its bits'
    return n
