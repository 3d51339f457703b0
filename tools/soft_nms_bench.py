#!/usr/bin/env python
"""Soft-NMS of activity proposals on the GPU (cfn_hip.detections.soft_nms / propose(soft=); csrc/segnms.hip) on the four inputs of
tools/proposals_bench.py: 8 x 157 x 640 (the training window) and 4 x 157 x 2,200 (whole validation videos), K = 5 levels, sparse (what a
trained detector gives) and alternating (every second frame a run of its own at every level: groups of 1,600 and 5,500 candidates, five exact
copies of each segment, the workspace path of soft_select).

soft_select costs selected * nd / 64 passes of a wave per group, and unlike hard NMS nothing is deleted: a group is walked until the largest
working score falls under min_score (0.001 here).  In the alternating case linear (nms_thr 0.5) zeroes the four copies of a selected segment
(tIoU 1), so nd / K rows are selected; gaussian (sigma 0.5) decays a copy by E(2) = 0.135 per selected copy, so all K copies but the last
stay above the floor and about 4 nd / K rows are selected -- quadratic in the group size, stated here, not hidden.

Per shape and kind, alternating in the same run, device time per call with the calls captured in one graph:

  soft_nms    soft_nms on the candidates of ONE decode_levels call (3 graph nodes), linear and gaussian
  nms         hard nms at 0.5 on the SAME candidates in the same run: the baseline
  propose     decode_levels + the second stage (6 nodes), hard and both soft methods
  copy        a device-to-device copy of the candidates' records (seg, frames, score): the yardstick
  baseline    sparse only: the way without this stage -- tolist() of the candidates (the read-back) and soft_nms_reference's rounds on the
              host; wall clock.  NOT measured for the alternating case (about 1e9 tIoU evaluations in numpy)

No time is a pass criterion.  The sparse result of the timed calls is compared with soft_nms_reference; the alternating one by its counts.
One JSON document on stdout and in --out.

    python tools/soft_nms_bench.py --out profiles/soft_nms.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from cfn_hip import ops  # noqa: E402
from cfn_hip.detections import Detections, SoftNMS, decode_levels, levels_tensor, nms, soft_nms, soft_nms_reference  # noqa: E402
from proposals_bench import C, LEVELS, NMS_THR, graph_ms, make_probs  # noqa: E402

SOFT = {'linear': SoftNMS('linear', 0.5, 0.001, 0), 'gaussian': SoftNMS('gaussian', 0.5, 0.001, 0)}


def parent_way(cand, soft):
    """the read-back of the candidates and the rounds on the host -> the selected Detections"""
    rows = cand.tolist()
    seg, frames, score, offsets = [], [], [], [0]
    for per_video in rows:
        for s in per_video:
            seg.append([float(s['class']), s['start'], s['end']])
            frames.append([s['t0'], s['t1'], 0])
            score.append([s['score_max'], s['score_mean']])
        offsets.append(len(seg))
    n = max(len(seg), 1)
    host = Detections(torch.tensor(seg, dtype=torch.float64).reshape(-1, 3) if seg else torch.zeros(1, 3, dtype=torch.float64),
                      torch.tensor(frames, dtype=torch.int32).reshape(-1, 3) if seg else torch.zeros(1, 3, dtype=torch.int32),
                      torch.tensor(score, dtype=torch.float32).reshape(-1, 2) if seg else torch.zeros(1, 2),
                      torch.tensor(offsets, dtype=torch.int32), torch.tensor([len(seg)], dtype=torch.int32), C, n)
    return soft_nms_reference(host, soft, NMS_THR)[0]


def measure(B, TL, kind, dev, repeats):
    K = len(LEVELS)
    probs = make_probs(B, TL, kind, 7 * B + TL)
    valid = torch.full((B,), TL, dtype=torch.int32)
    fps, start = torch.full((B,), 24.0, dtype=torch.float64), torch.arange(B, dtype=torch.int32) * 100
    d = [t.to(dev) for t in (probs, valid, fps, start)]
    levels = levels_tensor(LEVELS, C, dev)
    capk = ops.decode_segments_levels_cap(B, C, K, TL)

    def records(rows):
        return (torch.empty(rows, 3, dtype=torch.float64, device=dev), torch.empty(rows, 3, dtype=torch.int32, device=dev), torch.empty(rows, 2, device=dev))
    tail = lambda: (torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    out_lev = records(capk) + (torch.empty(capk, dtype=torch.uint8, device=dev),) + tail() + \
        (torch.empty(ops.decode_segments_levels_workspace_bytes(B, C, K, TL), dtype=torch.uint8, device=dev),)
    second = lambda ws: records(capk) + tail() + (torch.empty(capk, dtype=torch.uint8, device=dev), torch.empty(capk, dtype=torch.int32, device=dev),
                                                  torch.empty(ws, dtype=torch.uint8, device=dev))
    out_nms = second(ops.nms_segments_workspace_bytes(B, C, capk))
    out_soft = second(ops.soft_nms_segments_workspace_bytes(B, C, capk))
    cand, _ = decode_levels(*d, levels, out=out_lev)
    total = cand.check()
    src = [t[:max(total, 1)] for t in cand[:3]]
    dst = [torch.empty_like(t) for t in src]

    def copy():
        for a, b in zip(dst, src):
            a.copy_(b)
    runs = {'nms': lambda: nms(cand, NMS_THR, out=out_nms), 'copy': copy,
            'propose_nms': lambda: nms(decode_levels(*d, levels, out=out_lev)[0], NMS_THR, out=out_nms)}
    for name, soft in SOFT.items():
        runs['soft_' + name] = lambda soft=soft: soft_nms(cand, soft, NMS_THR, out=out_soft)
        runs['propose_soft_' + name] = lambda soft=soft: soft_nms(decode_levels(*d, levels, out=out_lev)[0], soft, NMS_THR, out=out_soft)
    raw = {k: [] for k in runs}
    for _ in range(repeats):                                         # alternating
        for k, fn in runs.items():
            raw[k].append(graph_ms(fn))
    med = {k: statistics.median(v) for k, v in raw.items()}
    groups = torch.bincount((cand.seg[:total, 0].long() + C * (torch.bucketize(torch.arange(total, device=dev), cand.offsets[1:].long(), right=True))),
                            minlength=B * C) if total else torch.zeros(1, dtype=torch.long)
    res = {'candidates': total, 'largest_group': int(groups.max()), 'groups_with_candidates': int((groups > 0).sum()), 'record_bytes': total * 44,
           'kept_by_nms': runs['nms']()[0].check(), 'copy_of_records_graph_ms': round(med['copy'], 5)}
    for k in runs:
        if k != 'copy':
            res[k + '_graph_ms'] = round(med[k], 5)
            res[k + '_min_max'] = [round(min(raw[k]), 5), round(max(raw[k]), 5)]
    for name, soft in SOFT.items():
        got = runs['soft_' + name]()[0]
        n = got.check()
        res['selected_' + name] = n
        res['soft_%s_over_nms' % name] = round(med['soft_' + name] / med['nms'], 2)
        if kind == 'sparse':
            wall = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                base = parent_way(cand, soft)
                wall.append((time.perf_counter() - t0) * 1e3)
            same = n == base.check() and bool(torch.equal(got.offsets.cpu(), base.offsets)) \
                and bool(torch.equal(got.seg[:n].cpu(), base.seg[:n])) and bool(torch.equal(got.score[:n].cpu(), base.score[:n]))
            res.update({'host_way_%s_wall_ms' % name: round(statistics.median(wall), 3),
                        'host_way_%s_over_soft_nms' % name: round(statistics.median(wall) / med['soft_' + name], 1),
                        '%s_equals_the_reference' % name: bool(same)})
        else:
            want = total // K if name == 'linear' else 4 * total // K
            res.update({'host_way_%s_wall_ms' % name: 'NOT measured', '%s_counts_as_expected' % name: total == capk and n == want})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x640,4x2200', help='B x TL, comma separated')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    out = {'classes': C, 'levels': list(LEVELS), 'nms_thr': NMS_THR, 'soft': {k: v._asdict() for k, v in SOFT.items()}, 'repeats': a.repeats,
           'device': cfn_hip.device_info(), 'shapes': {}}
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
