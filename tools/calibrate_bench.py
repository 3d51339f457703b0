#!/usr/bin/env python
"""Per-class thresholds from sorted AP rows on the GPU (cfn_hip.ops.ap_calibrate; csrc/apcal.hip) on 157 classes x 2^18 and x 2^21 rows
(a logging interval of the training meter, and well beyond one), with K = 1 (f1) and K = 5 criteria (f1, precision 0.5, recall 0.3 / 0.6 /
0.9), for two kinds of scores:

  uniform     fp32 uniform in [0, 1): nearly every row is a cut of its own
  q256        the same quantised to 256 values: tie runs of thousands of rows, 255 admissible cuts per class

The stores are sorted once with ops.ap_sort; per shape and kind, alternating in the same run, device time per call with the calls captured
in one graph:

  calibrate_k1, calibrate_k5   ONE ap_calibrate call each (1 graph node)
  reduce                       ap_reduce on the same sorted targets (1 node): the AP the same rows already pay for
  copy                         a device-to-device copy of the classes' sorted scores + targets (5 bytes per row): the yardstick
  reference                    thresholds_reference for the K = 5 criteria WITH its read-back of the sorted stores: what a user without the
                               kernel does; wall clock, once

ap_calibrate reads every row twice (P and m; then scores and targets together), 10 bytes per row against ap_reduce's 1, and like ap_reduce
it runs one workgroup per class: 157 workgroups on 256 CUs, so neither can reach the HBM rate.  The expectation, written down and NOT
enforced: a small multiple of ap_reduce.  No time is a pass criterion; the K = 5 result of the timed call is compared with the reference.
One JSON document on stdout and in --out.

    python tools/calibrate_bench.py --out profiles/calibrate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import torch  # noqa: E402

from cfn_hip import ops  # noqa: E402
from cfn_hip.calibrate import criteria_tensors, thresholds_reference  # noqa: E402

C = 157
K1 = [('f1', None)]
K5 = [('f1', None), ('precision', 0.5), ('recall', 0.3), ('recall', 0.6), ('recall', 0.9)]


def make_sorted(rows, kind, dev, seed):
    """sorted class-major stores of `rows` rows per class and their device count; labels that follow the scores loosely"""
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.rand(C, rows, device=dev, generator=g)
    if kind == 'q256':
        s = torch.floor(s * 256.0) / 256.0
    t = (torch.rand(C, rows, device=dev, generator=g) < 0.05 + 0.5 * s).to(torch.uint8)
    count = torch.tensor([rows], dtype=torch.int32, device=dev)
    ss, st = ops.ap_sort(s, t, count)
    return ss, st, count


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
    timed eager call (tools/proposals_bench.py)"""
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


def outputs(K, dev):
    return (torch.empty(C, K, device=dev), torch.empty(C, K, dtype=torch.int32, device=dev), torch.empty(C, K, dtype=torch.int32, device=dev),
            torch.empty(C, K, dtype=torch.uint8, device=dev), torch.empty(C, 2, dtype=torch.int32, device=dev))


def measure(rows, kind, dev, repeats, reference):
    ss, st, count = make_sorted(rows, kind, dev, rows % 1000 + len(kind))
    torch.cuda.empty_cache()
    c1, c5 = criteria_tensors(K1, dev), criteria_tensors(K5, dev)
    o1, o5 = outputs(1, dev), outputs(5, dev)
    ds, dt = torch.empty_like(ss), torch.empty_like(st)

    def copy():
        ds.copy_(ss)
        dt.copy_(st)
    runs = {'calibrate_k1': lambda: ops.ap_calibrate(ss, st, count, c1[0], c1[1], out=o1), 'calibrate_k5': lambda: ops.ap_calibrate(ss, st, count, c5[0], c5[1], out=o5),
            'reduce': lambda: ops.ap_reduce(st, count), 'copy': copy}
    raw = {k: [] for k in runs}
    for _ in range(repeats):                                         # alternating
        for k, fn in runs.items():
            raw[k].append(graph_ms(fn))
    med = {k: statistics.median(v) for k, v in raw.items()}
    del ds, dt
    runs['calibrate_k5']()
    torch.cuda.synchronize()
    res = {'rows_per_class': rows, 'bytes_read_by_calibrate': C * rows * 10,
           'classes_ok_k5': [int(x) for x in o5[3].sum(0).tolist()]}
    for k in runs:
        res[k + '_graph_ms'] = round(med[k], 5)
        res[k + '_min_max'] = [round(min(raw[k]), 5), round(max(raw[k]), 5)]
    res['calibrate_k1_over_reduce'] = round(med['calibrate_k1'] / med['reduce'], 2)
    res['calibrate_k5_over_reduce'] = round(med['calibrate_k5'] / med['reduce'], 2)
    res['calibrate_k5_over_copy'] = round(med['calibrate_k5'] / med['copy'], 2)
    res['calibrate_k5_GBps'] = round(C * rows * 10 / med['calibrate_k5'] / 1e6, 1)
    if reference:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = thresholds_reference(ss, st, count, K5)                # (its .cpu() of the sorted stores is the read-back)
        wall = (time.perf_counter() - t0) * 1e3
        same = all(bool(torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8))) for a, b in zip(o5, ref))
        res.update({'reference_with_read_back_wall_ms': round(wall, 1), 'reference_over_calibrate_k5': round(wall / med['calibrate_k5'], 1),
                    'equals_the_reference': bool(same)})
    else:
        res.update({'reference_with_read_back_wall_ms': 'NOT measured', 'equals_the_reference': 'NOT checked'})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', default='262144,2097152', help='rows per class, comma separated')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-reference', action='store_true', help='skip the numpy reference and its read-back')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    out = {'classes': C, 'criteria_k1': K1, 'criteria_k5': K5, 'repeats': a.repeats, 'device': cfn_hip.device_info(), 'shapes': {}}
    for rows in (int(v) for v in a.rows.split(',')):
        out['shapes']['%dx%d' % (C, rows)] = {kind: measure(rows, kind, torch.device('cuda:0'), a.repeats, not a.no_reference) for kind in ('uniform', 'q256')}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
