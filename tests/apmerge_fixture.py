"""Stores for the AP-merge tests (test_apmerge_cpu.py, test_hip_apmerge.py): class-major segment-AP stores built on the host with
cfn_hip.segap.match_reference from the segap_fixture batches, the tied-score shards whose order decides the AP, and bit patterns for the
kernel tests.  Nothing here needs a GPU."""
import numpy as np

import segap_fixture as sx

C = 5
TIOU = (0.3, 0.5, 0.7)
SENTINEL_SCORE = np.int32(0x7fc0dead)          # a NaN with a payload: a row nobody wrote
SENTINEL_BYTE = np.uint8(0xa5)


def batches():
    """four batches over C = 5 classes: the hand batch and three random ones (scores on a grid of eighths: ties inside and across batches)"""
    return [sx.hand_batch(), sx.random_batch(11, 3, C, 9, 5), sx.random_batch(12, 2, C, 12, 4), sx.random_batch(13, 4, C, 6, 6)]


def tied_shards():
    """two one-batch shards with ONE tied score in class 0: A holds a true positive at 0.5, B a false positive at 0.5.  A then B ranks the true
    positive first (AP 1), B then A the false positive (AP 1/2): the order of a merge is visible in the value"""
    a = (sx.make_det([[(0, 0, 10, 0.5, 0.5)]], C), sx.make_gt([[(0, 0, 10)]], [1.0], [[0, 100]], C))
    b = (sx.make_det([[(0, 20, 30, 0.5, 0.5)]], C), sx.make_gt([[]], [1.0], [[0, 100]], C))
    return a, b


def _gt(batch):
    lab = batch[1]
    return lab.seg, lab.offsets, lab.fps, lab.window, lab.t_max


def store_from(batch_list, cap, tiou=TIOU, n_classes=C, flags=0):
    """rule 6 of cfn_hip/segap.py on the host: the batches into a fresh store -> (scores (C, cap) int32 BITS of the fp32 scores, tps (C, cap)
    uint8, state [counts (C), n_gt (C), flags] int32); rows behind the counts hold the sentinels"""
    from cfn_hip.segap import match_reference
    scores = np.full((n_classes, cap), SENTINEL_SCORE, np.int32)
    tps = np.full((n_classes, cap), SENTINEL_BYTE, np.uint8)
    state = np.zeros(2 * n_classes + 1, np.int32)
    state[-1] = flags
    for batch in batch_list:
        det = batch[0]
        tp, _, g = match_reference(det, *_gt(batch), tiou, 0)
        state[n_classes:2 * n_classes] += g.astype(np.int32)
        dseg, dscore = det.seg.numpy(), det.score.numpy()
        for i in range(len(tp)):
            c = int(dseg[i, 0])
            scores[c, state[c]] = dscore[i, 0:1].view(np.int32)[0]
            tps[c, state[c]] = tp[i]
            state[c] += 1
    return scores, tps, state


def split_state(state, n_classes=C):
    """state -> (counts, n_gt, flags) views"""
    return state[:n_classes], state[n_classes:2 * n_classes], state[2 * n_classes:]


def ap_of_store(scores, tps, state, tiou=TIOU, n_classes=C):
    """rule 7 on a store -> (ap, map) fp32"""
    from cfn_hip.segap import ap_from_stores
    counts, n_gt, _ = split_state(state, n_classes)
    return ap_from_stores([scores[c, :counts[c]].view(np.float32) for c in range(n_classes)], [tps[c, :counts[c]] for c in range(n_classes)],
                          n_gt, len(tiou))


def prefixes(scores, payload, counts):
    """the rows in front of the counts, per class (counts of one entry: one count for all classes)"""
    n = [int(counts[0 if len(counts) == 1 else c]) for c in range(scores.shape[0])]
    return [scores[c, :n[c]].copy() for c in range(scores.shape[0])], [payload[c, :n[c]].copy() for c in range(scores.shape[0])]


def same_rows(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def score_bits(rng, shape):
    """random 32-bit patterns with the special values of fp32 sprinkled in: NaNs with payloads (quiet and signalling), -0.0, +-inf, denormals"""
    bits = rng.randint(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
    special = np.array([0x7fc00001, 0x7fa12345, -0x003fffff, -0x80000000, 0x7f800000, -0x00800000, 0x00000001, -0x7fffffff, 0x007fffff, 0],
                       np.int64).astype(np.int32)        # (-0x003fffff = 0xffc00001: a negative NaN; -0x00800000 = 0xff800000: -inf)
    pick = rng.rand(*shape) < 0.25
    bits[pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
    return bits
