#!/usr/bin/env python
"""Activity proposals on the GPU (cfn_hip.detections.decode_levels / nms / propose; csrc/detections.hip, csrc/segnms.hip) at 8 x 157 x 640
(the training window) and 4 x 157 x 2,200 (whole validation videos) with K = 5 levels (0.8, 0.65, 0.5, 0.35, 0.2) and nms_thr 0.5, for two
kinds of probabilities:

  sparse      5 % of the class rows carry about 3 bumps of activity each (a level cuts a bump at its own width), the rest stays under
              every level: what a trained detector gives
  alternating every second frame is a run of its own at every level: the worst case.  Every (video, class) group then holds
              K * ((TL + 1) // 2) candidates (1,600 and 5,500: the general path of the select kernel), five exact copies of each segment, all
              with one score; NMS keeps nd / K of them and each kept one walks the ranks behind it, so a group costs nd^2 / 64 rank steps
              and kept * nd / 64 = nd^2 / (64 K) suppression steps of a wave -- quadratic in TL, stated here, not hidden

Per shape and kind, alternating in the same run, device time per call with the calls captured in one graph:

  levels      ONE decode_levels call (3 graph nodes)
  5 decodes   five decode calls, one per level (15 nodes): how the parent commit produces the same candidates
  nms         nms on those candidates (3 nodes);  propose = levels + nms (6 nodes)
  copy        a device-to-device copy of the candidates' records (seg, frames, score): the yardstick
  baseline    sparse only: the parent commit's way to the same result -- five decode calls, tolist() of each (the read-back), the merge
              and nms_reference's greedy loop on the host; wall clock.  NOT measured for the alternating case: it needs
              B * C * nd^2 / (2 K) tIoU evaluations in Python (about 3e8 and 2e9)

No time is a pass criterion.  The sparse result of the timed calls is compared with the numpy references; the alternating one by its
counts.  One JSON document on stdout and in --out.

    python tools/proposals_bench.py --out profiles/proposals.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cfn_hip import ops  # noqa: E402
from cfn_hip.detections import Detections, decode, decode_levels, decode_levels_reference, levels_tensor, nms, nms_reference  # noqa: E402

C = 157
LEVELS = (0.8, 0.65, 0.5, 0.35, 0.2)
NMS_THR = 0.5


def make_probs(B, TL, kind, seed):
    r = np.random.RandomState(seed)
    if kind == 'alternating':
        p = np.zeros((B, C, TL), np.float32)
        p[:, :, ::2] = 0.9
        return torch.from_numpy(p)
    p = (r.rand(B, C, TL) * 0.15).astype(np.float32)                 # background under every level
    t = np.arange(TL, dtype=np.float32)
    for b in range(B):
        for c in np.flatnonzero(r.rand(C) < 0.05):
            for _ in range(3):
                mid, wid = r.rand() * TL, 8.0 + 50.0 * r.rand()
                p[b, c] += (0.5 + 0.45 * r.rand()) * np.exp(-((t - mid) / wid) ** 2)
    return torch.from_numpy(np.clip(p, 0.0, 1.0))


def event_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def graph_ms(fn, budget_ms=60.0):
    """device time per call with several calls captured in one graph; how many: what fits `budget_ms` per replay (at most 50), from one
    timed eager call"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        once = event_ms(fn, 1, warmup=1)
    side.synchronize()
    launches = int(min(50, max(1, budget_ms / max(once, 1e-3))))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(launches):
            fn()
    return event_ms(graph.replay, 5 if launches > 1 else 2, warmup=1) / launches


def parent_way(d, names=None):
    """five decode calls, their read-backs, the merge in (b, c, k, t0) order and the greedy loop on the host -> the kept Detections"""
    probs, valid, fps, start = d
    B = int(probs.shape[0])
    lists = [decode(probs, valid, fps, start, thr).tolist() for thr in LEVELS]
    seg, score, frames, offsets = [], [], [], [0]
    for b in range(B):
        rows = sorted((s['class'], k, s['t0'], s) for k, per_video in enumerate(lists) for s in per_video[b])
        for c, k, t0, s in rows:
            seg.append([float(c), s['start'], s['end']])
            frames.append([s['t0'], s['t1'], 0])
            score.append([s['score_max'], s['score_mean']])
        offsets.append(len(seg))
    n = max(len(seg), 1)
    cand = Detections(torch.tensor(seg, dtype=torch.float64).reshape(-1, 3) if seg else torch.zeros(1, 3, dtype=torch.float64),
                      torch.tensor(frames, dtype=torch.int32).reshape(-1, 3) if seg else torch.zeros(1, 3, dtype=torch.int32),
                      torch.tensor(score, dtype=torch.float32).reshape(-1, 2) if seg else torch.zeros(1, 2),
                      torch.tensor(offsets, dtype=torch.int32), torch.tensor([len(seg)], dtype=torch.int32), C, n)
    return nms_reference(cand, NMS_THR)[0]


def measure(B, TL, kind, dev, repeats):
    K = len(LEVELS)
    probs = make_probs(B, TL, kind, 7 * B + TL)
    valid = torch.full((B,), TL, dtype=torch.int32)
    fps, start = torch.full((B,), 24.0, dtype=torch.float64), torch.arange(B, dtype=torch.int32) * 100
    d = [t.to(dev) for t in (probs, valid, fps, start)]
    levels = levels_tensor(LEVELS, C, dev)
    thr = [torch.full((C,), x, device=dev) for x in LEVELS]
    cap1, capk = ops.decode_segments_cap(B, C, TL), ops.decode_segments_levels_cap(B, C, K, TL)

    def records(rows):
        return (torch.empty(rows, 3, dtype=torch.float64, device=dev), torch.empty(rows, 3, dtype=torch.int32, device=dev), torch.empty(rows, 2, device=dev))
    tail = lambda: (torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    out_one = records(cap1) + tail() + (torch.empty(ops.decode_segments_workspace_bytes(B, C, TL), dtype=torch.uint8, device=dev),)
    out_lev = records(capk) + (torch.empty(capk, dtype=torch.uint8, device=dev),) + tail() + \
        (torch.empty(ops.decode_segments_levels_workspace_bytes(B, C, K, TL), dtype=torch.uint8, device=dev),)
    out_nms = records(capk) + tail() + (torch.empty(capk, dtype=torch.uint8, device=dev), torch.empty(capk, dtype=torch.int32, device=dev),
                                        torch.empty(ops.nms_segments_workspace_bytes(B, C, capk), dtype=torch.uint8, device=dev))
    cand, level = decode_levels(*d, levels, out=out_lev)
    total = cand.check()
    src = [t[:max(total, 1)] for t in cand[:3]]
    dst = [torch.empty_like(t) for t in src]

    def five():
        for t in thr:
            decode(*d, t, out=out_one)

    def copy():
        for a, b in zip(dst, src):
            a.copy_(b)
    runs = {'levels': lambda: decode_levels(*d, levels, out=out_lev), 'five_decodes': five, 'nms': lambda: nms(cand, NMS_THR, out=out_nms),
            'propose': lambda: nms(decode_levels(*d, levels, out=out_lev)[0], NMS_THR, out=out_nms), 'copy': copy}
    raw = {k: [] for k in runs}
    for _ in range(repeats):                                         # alternating
        for k, fn in runs.items():
            raw[k].append(graph_ms(fn))
    med = {k: statistics.median(v) for k, v in raw.items()}
    kept, _, _ = runs['propose']()
    n_kept = kept.check()
    groups = torch.bincount((cand.seg[:total, 0].long() + C * (torch.bucketize(torch.arange(total, device=dev), cand.offsets[1:].long(), right=True))),
                            minlength=B * C) if total else torch.zeros(1, dtype=torch.long)
    res = {'candidates': total, 'kept': n_kept, 'largest_group': int(groups.max()), 'groups_with_candidates': int((groups > 0).sum()),
           'record_bytes': total * 45, 'levels_graph_ms': round(med['levels'], 5), 'levels_min': round(min(raw['levels']), 5),
           'levels_max': round(max(raw['levels']), 5), 'five_decodes_graph_ms': round(med['five_decodes'], 5),
           'five_decodes_over_levels': round(med['five_decodes'] / med['levels'], 3), 'nms_graph_ms': round(med['nms'], 5),
           'nms_min': round(min(raw['nms']), 5), 'nms_max': round(max(raw['nms']), 5), 'propose_graph_ms': round(med['propose'], 5),
           'copy_of_records_graph_ms': round(med['copy'], 5), 'propose_multiple_of_copy': round(med['propose'] / med['copy'], 2)}
    if kind == 'sparse':
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            base = parent_way(d)
            wall.append((time.perf_counter() - t0) * 1e3)
        ref_c, ref_l = decode_levels_reference(probs, valid, fps, start, LEVELS)
        ref_k = nms_reference(ref_c, NMS_THR)[0]
        same = total == ref_c.check() and n_kept == ref_k.check() == base.check() and bool(torch.equal(level[:total].cpu(), ref_l[:total])) \
            and all(bool(torch.equal(a[:total].cpu(), b[:total])) for a, b in zip(cand[:2], ref_c[:2])) \
            and all(bool(torch.equal(a[:n_kept].cpu(), b[:n_kept])) for a, b in zip(kept[:2], ref_k[:2])) \
            and bool(torch.equal(kept.seg[:n_kept].cpu(), base.seg[:n_kept])) and bool(torch.equal(kept.offsets.cpu(), ref_k.offsets))
        res.update({'parent_way_wall_ms': round(statistics.median(wall), 3), 'parent_way_over_propose': round(statistics.median(wall) / med['propose'], 1),
                    'equals_the_references_and_the_parent_way': bool(same)})
    else:
        res.update({'parent_way_wall_ms': 'NOT measured', 'equals_the_references_and_the_parent_way': 'NOT checked (counts only)',
                    'counts_as_expected': total == capk and n_kept * K == total})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x640,4x2200', help='B x TL, comma separated')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    out = {'classes': C, 'levels': list(LEVELS), 'nms_thr': NMS_THR, 'repeats': a.repeats, 'device': cfn_hip.device_info(), 'shapes': {}}
    for shape in a.shapes.split(','):
        B, TL = (int(v) for v in shape.split('x'))
        out['shapes']['%dx%dx%d' % (B, C, TL)] = {kind: measure(B, TL, kind, torch.device('cuda:0'), a.repeats) for kind in ('sparse', 'alternating')}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
