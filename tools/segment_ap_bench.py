#!/usr/bin/env python
"""Segment-level AP on the GPU (cfn_hip.segap.SegmentAPMeter, csrc/segap.hip), at 8 x 157 x 640 (the training window) and 4 x 157 x 2,200
(whole validation videos), for the two kinds of probabilities of tools/detections_bench.py:

  sparse      5 % of the class rows carry about 3 runs each (what a trained detector gives); the ground truth is the decode of the same
              probabilities three frames later, so most detections find a row at a tIoU below 1
  alternating every second frame is a detection: decode's worst case, (TL + 1) // 2 detections in every (video, class) group, ordered by
              counting in O(nd^2) per group; 32 of each video's detections are its ground truth

Per shape and kind, alternating in the same run:

  add         SegmentAPMeter.add (match + plan + copy) per call, device time with the calls captured in one graph behind one reset(), and eagerly
  (a) copy    a device-to-device copy of the bytes of the batch's Detections records (44 per segment), the same way: the yardstick
  (b) host    the composition it replaces: Detections.tolist() plus ap_reference in numpy, read-back included (wall clock; sparse only --
              the worst case is minutes of Python per batch)

and once: value_device() and value() (with its read-back) at one validation phase's volume, 1,850 videos of the sparse kind.  No time is a
pass criterion.  The timed add's tp bytes are compared with match_reference (sparse).  One JSON document on stdout and in --out.

    python tools/segment_ap_bench.py --out profiles/segment_ap.json
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
from cfn_hip.detections import decode  # noqa: E402
from cfn_hip.seglabels import SegLabels  # noqa: E402
from cfn_hip.segap import DEFAULT_TIOU, SegmentAPMeter, ap_reference, match_reference  # noqa: E402
from detections_bench import event_ms, make_probs, wall_ms  # noqa: E402

C = 157


def graph_ms(pre, fn, launches, replays):
    """device time per call of fn: one graph of pre() and `launches` calls of fn (the gap between two nodes stays in the figure)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pre()
        fn()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pre()
        for _ in range(launches):
            fn()
    return event_ms(graph.replay, replays, warmup=2) / launches


def make_batch(B, TL, kind, dev):
    probs = make_probs(B, TL, kind, 7 * B + TL).to(dev)
    valid = torch.full((B,), TL, dtype=torch.int32, device=dev)
    fps, start = torch.full((B,), 24.0, dtype=torch.float64, device=dev), (torch.arange(B, dtype=torch.int32) * 100).to(dev)
    det = decode(probs, valid, fps, start, 0.5)
    total = det.check()
    window = torch.stack([start, valid], 1).contiguous()
    if kind == 'sparse':
        g = decode(torch.roll(probs, 3, 2), valid, fps, start, 0.5)
        n = g.check()
        lab = SegLabels(g.seg[:max(n, 1)].contiguous(), g.offsets, fps, window, C, TL)
    else:
        offs = det.offsets.tolist()
        r = np.random.RandomState(B + TL)
        pick = np.concatenate([np.sort(r.choice(np.arange(offs[b], offs[b + 1]), 32, replace=False)) for b in range(B)])
        lab = SegLabels(det.seg[torch.from_numpy(pick).to(dev)].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev) * 32, fps, window, C, TL)
    return det, total, lab


def measure(B, TL, kind, dev, iters, launches, replays, host_iters):
    det, total, lab = make_batch(B, TL, kind, dev)
    per_class = B * ((TL + 1) // 2) if kind == 'alternating' else 64
    meter = SegmentAPMeter(dev, C, capacity=per_class * (launches + 1))
    cap = int(det.seg.shape[0])
    out = (torch.empty(cap, dtype=torch.uint8, device=dev), None,
           torch.empty(ops.segap_workspace_bytes(B, C, cap, int(lab.seg.shape[0])), dtype=torch.uint8, device=dev))
    add = lambda: meter.add(det, lab, out=out)
    one = lambda: (meter.reset(), add())
    src = torch.empty(max(total, 1) * 44, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)
    raw = {'add_graph': [], 'copy_graph': [], 'add_eager': [], 'copy_eager': [], 'host': []}
    for i in range(5):                                               # alternating
        raw['add_graph'].append(graph_ms(meter.reset, add, launches, replays))
        raw['copy_graph'].append(graph_ms(lambda: None, copy, launches, replays))
        raw['add_eager'].append(event_ms(one, iters))
        raw['copy_eager'].append(event_ms(copy, iters))
        if kind == 'sparse' and i % 2 == 0:
            raw['host'].append(wall_ms(lambda: (det.tolist(), ap_reference([(det, lab)], C)), host_iters))
    assert not int(meter.flags.item()), 'the timed batches did not fit the stores'
    med = {k: statistics.median(v) for k, v in raw.items() if v}
    res = {'segments': total, 'ground_truth_rows': int(lab.offsets[-1].item()), 'record_bytes': total * 44, 'graph_calls_per_replay': launches,
           'graph_ms_per_add': round(med['add_graph'], 5), 'min': round(min(raw['add_graph']), 5), 'max': round(max(raw['add_graph']), 5),
           'graph_copy_of_records_ms': round(med['copy_graph'], 5), 'graph_multiple_of_copy': round(med['add_graph'] / med['copy_graph'], 2),
           'eager_ms_per_reset_and_add': round(med['add_eager'], 5), 'eager_copy_of_records_ms': round(med['copy_eager'], 5)}
    if kind == 'sparse':
        meter.reset()
        tp, _ = add()
        want, _, n_gt = match_reference(det, lab.seg, lab.offsets, lab.fps, lab.window, lab.t_max, DEFAULT_TIOU)
        res.update({'host_tolist_and_ap_reference_ms': round(med['host'], 3), 'host_over_graph_add': round(med['host'] / med['add_graph'], 1),
                    'true_positives_at_0.5': int(((want >> 2) & 1).sum()), 'equals_match_reference': bool((tp.cpu().numpy()[:total] == want).all()
                                                                                                          and meter.n_gt.cpu().tolist() == n_gt.tolist())})
    else:
        res['host_tolist_and_ap_reference_ms'] = None                # (minutes of Python per batch: not run)
    return res


def measure_value(dev, videos, iters):
    """value_device() and value() with one validation phase in the stores: `videos` videos of the sparse kind, 4 per add"""
    det, total, lab = make_batch(4, 2200, 'sparse', dev)
    meter = SegmentAPMeter(dev, C)
    adds = (videos + 3) // 4
    for _ in range(adds):
        meter.add(det, lab)
    counts = meter.counts.cpu()
    dev_ms = [event_ms(meter.value_device, iters) for _ in range(5)]
    host_ms = [wall_ms(meter.value, iters) for _ in range(5)]
    ap, mp = meter.value()
    return {'videos': adds * 4, 'detections': int(counts.sum()), 'fullest_class': int(counts.max()), 'capacity': int(meter.stores[0].shape[1]),
            'value_device_ms': round(statistics.median(dev_ms), 4), 'min': round(min(dev_ms), 4), 'max': round(max(dev_ms), 4),
            'value_with_read_back_ms': round(statistics.median(host_ms), 4), 'map': [round(float(m), 4) for m in mp]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x640,4x2200', help='B x TL, comma separated')
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--videos', type=int, default=1850)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    dev = torch.device('cuda:0')
    out = {'classes': C, 'tiou': list(DEFAULT_TIOU), 'iters': a.iters, 'device': cfn_hip.device_info(), 'gt_tile': ops.SEGAP_GT_TILE,
           'det_tile': ops.SEGAP_DET_TILE, 'shapes': {}}
    for shape in a.shapes.split(','):
        B, TL = (int(v) for v in shape.split('x'))
        out['shapes']['%dx%dx%d' % (B, C, TL)] = {
            'sparse': measure(B, TL, 'sparse', dev, a.iters, 50, 20, a.host_iters),
            'alternating': measure(B, TL, 'alternating', dev, max(a.iters // 10, 3), 5, 3, a.host_iters)}
    out['value'] = measure_value(dev, a.videos, 20)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
