#!/usr/bin/env python
"""Proposal recall at N per video on the GPU (cfn_hip.recall.ProposalRecallMeter, csrc/segrecall.hip), at 8 x 157 x 640 (the training window)
and 4 x 157 x 2,200 (whole validation videos), on the inputs of tools/proposals_bench.py:

  sparse      5 % of the class rows carry about 3 bumps of activity each; the candidates are propose() at K = 5 levels (0.8, 0.65, 0.5,
              0.35, 0.2) with nms_thr 0.5; the ground truth is the decode at 0.5 of the same probabilities three frames later
  alternating decode's worst case: every second frame is a detection, (TL + 1) // 2 in every (video, class) group and C times as many in a
              video.  The rank kernel is O(n_b^2) in the candidates of a video: reported as measured, with n_b.  32 of each video's
              detections are its ground truth

Per shape and kind, alternating in the same run:

  add         ProposalRecallMeter.add (rank + first hit + accumulate) per call, device time with the calls captured in one graph
  (a) seg-AP  SegmentAPMeter.add (match + plan + copy) on the same inputs, the same way: the closest sibling
  (b) host    what it replaces: Detections.tolist() plus recall_reference in numpy, read-back included (wall clock; sparse only)

and once value_device() and value() (with its read-back).  No time is a pass criterion.  The timed add's hit table and state are compared with
recall_reference (sparse).  One JSON document on stdout and in --out.

    python tools/proposal_recall_bench.py --out profiles/proposal_recall.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cfn_hip import ops  # noqa: E402
from cfn_hip.detections import decode, propose  # noqa: E402
from cfn_hip.recall import DEFAULT_TIOU, ProposalRecallMeter, recall_reference  # noqa: E402
from cfn_hip.seglabels import SegLabels  # noqa: E402
from cfn_hip.segap import SegmentAPMeter  # noqa: E402
from detections_bench import event_ms, wall_ms  # noqa: E402
from proposals_bench import LEVELS, NMS_THR, make_probs  # noqa: E402
from segment_ap_bench import graph_ms  # noqa: E402

C = 157
N_MAX = 100


def make_batch(B, TL, kind, dev):
    probs = make_probs(B, TL, kind, 7 * B + TL).to(dev)
    valid = torch.full((B,), TL, dtype=torch.int32, device=dev)
    fps, start = torch.full((B,), 24.0, dtype=torch.float64, device=dev), (torch.arange(B, dtype=torch.int32) * 100).to(dev)
    window = torch.stack([start, valid], 1).contiguous()
    if kind == 'sparse':
        det = propose(probs, valid, fps, start, LEVELS, NMS_THR)
        g = decode(torch.roll(probs, 3, 2), valid, fps, start, 0.5)
        n = g.check()
        lab = SegLabels(g.seg[:max(n, 1)].contiguous(), g.offsets, fps, window, C, TL)
    else:
        det = decode(probs, valid, fps, start, 0.5)
        offs = det.offsets.tolist()
        r = np.random.RandomState(B + TL)
        pick = np.concatenate([np.sort(r.choice(np.arange(offs[b], offs[b + 1]), 32, replace=False)) for b in range(B)])
        lab = SegLabels(det.seg[torch.from_numpy(pick).to(dev)].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev) * 32, fps, window, C, TL)
    return det, det.check(), lab


def measure(B, TL, kind, dev, launches, replays, host_iters):
    det, total, lab = make_batch(B, TL, kind, dev)
    cap, S = int(det.cap), int(lab.seg.shape[0])
    offs = det.offsets.tolist()
    per_class = int(torch.bincount(det.seg[:total, 0].long(), minlength=C).max()) if total else 1
    meter = ProposalRecallMeter(dev, C, DEFAULT_TIOU, N_MAX)
    out = (torch.empty(len(DEFAULT_TIOU), S, dtype=torch.int32, device=dev),
           torch.empty(ops.seg_recall_workspace_bytes(B, C, cap, S, len(DEFAULT_TIOU)), dtype=torch.uint8, device=dev))
    add = lambda: meter.add(det, lab, out=out)
    ap_meter = SegmentAPMeter(dev, C, capacity=per_class * (launches + 1))
    ap_out = (torch.empty(cap, dtype=torch.uint8, device=dev), None,
              torch.empty(ops.segap_workspace_bytes(B, C, cap, S), dtype=torch.uint8, device=dev))
    ap_add = lambda: ap_meter.add(det, lab, out=ap_out)
    raw = {'add': [], 'segap': [], 'host': []}
    for i in range(5):                                               # alternating
        raw['add'].append(graph_ms(meter.reset, add, launches, replays))
        raw['segap'].append(graph_ms(ap_meter.reset, ap_add, launches, replays))
        if kind == 'sparse' and i % 2 == 0:
            raw['host'].append(wall_ms(lambda: (det.tolist(), recall_reference([(det, lab)], C, DEFAULT_TIOU, N_MAX)), host_iters))
    assert not int(ap_meter.flags.item()), 'the timed batches did not fit the segment-AP stores'
    med = {k: statistics.median(v) for k, v in raw.items() if v}
    meter.reset()
    hit = add()
    v = meter.value()
    res = {'candidates': total, 'candidates_per_video': [offs[b + 1] - offs[b] for b in range(B)], 'fullest_class_of_the_batch': per_class,
           'ground_truth_rows': int(lab.offsets[-1].item()), 'n_gt': v['n_gt'], 'graph_calls_per_replay': launches,
           'graph_ms_per_add': round(med['add'], 5), 'min': round(min(raw['add']), 5), 'max': round(max(raw['add']), 5),
           'segment_ap_graph_ms_per_add': round(med['segap'], 5), 'multiple_of_segment_ap_add': round(med['add'] / med['segap'], 3),
           'ar_at_1': round(float(v['ar'][0]), 4), 'ar_at_10': round(float(v['ar'][9]), 4), 'ar_at_100': round(float(v['ar'][-1]), 4),
           'auc': round(float(v['auc']), 4), 'avg_props': round(float(v['avg_props']), 1)}
    if kind == 'sparse':
        ref = recall_reference([(det, lab)], C, DEFAULT_TIOU, N_MAX)
        res.update({'host_tolist_and_recall_reference_ms': round(med['host'], 3), 'host_over_graph_add': round(med['host'] / med['add'], 1),
                    'equals_recall_reference': bool((hit.cpu().numpy() == ref['hits'][0]).all() and meter.state.cpu().numpy().tolist() == ref['state'].tolist()
                                                    and (v['recall'] == ref['recall']).all() and v['auc'] == ref['auc'])})
    else:
        res['host_tolist_and_recall_reference_ms'] = None            # (minutes of Python per batch: not run)
    return res, meter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x640,4x2200', help='B x TL, comma separated')
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    dev = torch.device('cuda:0')
    out = {'classes': C, 'tiou': list(DEFAULT_TIOU), 'n_max': N_MAX, 'levels': list(LEVELS), 'nms_thr': NMS_THR, 'device': cfn_hip.device_info(),
           'rank_tile': ops.SEG_RECALL_RANK_TILE, 'shapes': {}}
    meter = None
    for shape in a.shapes.split(','):
        B, TL = (int(v) for v in shape.split('x'))
        sparse, meter = measure(B, TL, 'sparse', dev, 50, 20, a.host_iters)
        worst, _ = measure(B, TL, 'alternating', dev, 3, 3, a.host_iters)
        out['shapes']['%dx%dx%d' % (B, C, TL)] = {'sparse': sparse, 'alternating': worst}
    dev_ms = [event_ms(meter.value_device, 20) for _ in range(5)]
    host_ms = [wall_ms(meter.value, 20) for _ in range(5)]
    out['value'] = {'value_device_ms': round(statistics.median(dev_ms), 4), 'value_with_read_back_ms': round(statistics.median(host_ms), 4)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
