"""fp64 reference of per-class average precision as apmeter.APMeter defines it (apmeter.py value(): per class a STABLE descending
sort of the scores in insertion order, AP = (sum over the positive ranks r of tp_r / r) / max(npos, 1)), and the sorted rows that
definition implies.  tp and r are integers; the only floating-point operations are the fp64 divisions and their fp64 sum."""
import numpy as np


def sorted_rows(scores, targets):
    """scores (n, K) float32, targets (n, K) -> (scores, targets != 0 as uint8) with every column in np.argsort(-s, kind='stable') order"""
    scores, targets = np.asarray(scores, dtype=np.float32), np.asarray(targets)
    if scores.ndim == 1:
        scores, targets = scores.reshape(-1, 1), targets.reshape(-1, 1)
    ss, st = np.empty_like(scores), np.empty(scores.shape, dtype=np.uint8)
    for j in range(scores.shape[1]):
        order = np.argsort(-scores[:, j], kind='stable')
        ss[:, j] = scores[order, j]
        st[:, j] = targets[order, j] != 0
    return ss, st


def ap_ref64(scores, targets):
    """(K,) float64"""
    _, st = sorted_rows(scores, targets)
    n, k = st.shape
    ranks = np.arange(1, n + 1, dtype=np.float64)
    ap = np.zeros(k, dtype=np.float64)
    for j in range(k):
        truth = st[:, j].astype(np.int64)
        tp = np.cumsum(truth)                                      # integers
        prec = tp.astype(np.float64) / ranks
        ap[j] = prec[truth > 0].sum() / max(int(truth.sum()), 1)
    return ap


def make_scores(kind, n, k, seed):
    """seeded (n, k) float32 scores of one of the kinds the AP tests use, and Bernoulli(0.3) targets"""
    rs = np.random.RandomState(seed)
    if kind == 'normal':
        s = rs.standard_normal((n, k))
    elif kind == 'sigmoid':
        s = 1.0 / (1.0 + np.exp(-2.0 * rs.standard_normal((n, k)) + 2.0))
    elif kind == 'quant8':
        s = rs.randint(0, 8, size=(n, k)) / 8.0
    elif kind == 'equal':
        s = np.full((n, k), 0.25)
    else:
        raise ValueError(kind)
    return s.astype(np.float32), (rs.uniform(size=(n, k)) < 0.3).astype(np.float32)
