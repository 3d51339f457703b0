#!/usr/bin/env python
"""Activity segments decoded from per-frame scores on the GPU (cfn_hip.detections.decode, csrc/detections.hip), at 8 x 157 x 640 (the
training window) and 4 x 157 x 2,200 (whole validation videos), for two kinds of probabilities:

  sparse      5 % of the class rows carry about 3 runs of activity each, the rest stays under the threshold (what a trained detector gives)
  alternating every second frame is a run of its own: the worst case, B * C * ((TL + 1) // 2) records, the default cap filled exactly

Per shape and kind, alternating in the same run:

  decode      device time per call with 50 calls captured in one graph (no host enqueue between the launches), and launched eagerly
  (a) copy    a device-to-device copy of probs, the same way: the decode reads probs once, so this is the floor of its count launch
  (b) torch   decode_reference on the GPU tensors: the composition a caller writes today, with its read-backs (wall clock, a few calls)

No time is a pass criterion: the ratios to (a) and (b) are the record.  The result of the timed call is compared with decode_reference.
One JSON document on stdout and in --out.

    python tools/detections_bench.py --out profiles/detections.json
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
from cfn_hip.detections import decode, decode_reference  # noqa: E402

C = 157


def make_probs(B, TL, kind, seed):
    r = np.random.RandomState(seed)
    if kind == 'alternating':
        p = np.zeros((B, C, TL), np.float32)
        p[:, :, ::2] = 0.75
        return torch.from_numpy(p)
    p = (r.rand(B, C, TL) * 0.4).astype(np.float32)                  # background under the threshold
    for b in range(B):
        for c in np.flatnonzero(r.rand(C) < 0.05):
            for _ in range(3):
                t0 = int(r.randint(0, TL))
                p[b, c, t0:t0 + int(r.randint(8, 120))] = 0.55 + 0.4 * r.rand()
    return torch.from_numpy(p)


def event_ms(fn, iters, warmup=5):
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


def graph_ms(fn, launches=50, replays=20):
    """device time per call with `launches` of them captured in one graph (the gap between two nodes of a graph stays in the figure)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(launches):
            fn()
    return event_ms(graph.replay, replays, warmup=2) / launches


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def measure(B, TL, kind, dev, iters, ref_iters):
    probs = make_probs(B, TL, kind, 7 * B + TL)
    valid = torch.full((B,), TL, dtype=torch.int32)
    fps, start = torch.full((B,), 24.0, dtype=torch.float64), torch.arange(B, dtype=torch.int32) * 100
    d = [t.to(dev) for t in (probs, valid, fps, start)] + [torch.full((C,), 0.5, device=dev)]
    cap = ops.decode_segments_cap(B, C, TL)
    out = (torch.empty(cap, 3, dtype=torch.float64, device=dev), torch.empty(cap, 3, dtype=torch.int32, device=dev),
           torch.empty(cap, 2, device=dev), torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
           torch.empty(ops.decode_segments_workspace_bytes(B, C, TL), dtype=torch.uint8, device=dev))
    dst = torch.empty_like(d[0])
    run = lambda: decode(*d, out=out)
    copy = lambda: dst.copy_(d[0])
    raw = {'decode_graph': [], 'copy_graph': [], 'decode_eager': [], 'copy_eager': [], 'torch': []}
    for i in range(5):                                               # alternating
        raw['decode_graph'].append(graph_ms(run))
        raw['copy_graph'].append(graph_ms(copy))
        raw['decode_eager'].append(event_ms(run, iters))
        raw['copy_eager'].append(event_ms(copy, iters))
        if i % 2 == 0:                                               # (seconds per call in the worst case: three visits)
            raw['torch'].append(wall_ms(lambda: decode_reference(*d[:4], 0.5), ref_iters))
    got, ref = run(), decode_reference(probs, valid, fps, start, 0.5)
    total = got.check()
    same = total == ref.check() and all(bool(torch.equal(a[:total].cpu(), b[:total])) for a, b in zip(got[:2], ref[:2])) \
        and bool(torch.equal(got.offsets.cpu(), ref.offsets)) and bool(torch.equal(got.score[:total, 0].cpu(), ref.score[:total, 0]))
    med = {k: statistics.median(v) for k, v in raw.items()}
    return {'segments': total, 'probs_bytes': probs.numel() * 4, 'record_bytes': total * 44,
            'graph_ms_per_call': round(med['decode_graph'], 5), 'min': round(min(raw['decode_graph']), 5), 'max': round(max(raw['decode_graph']), 5),
            'graph_copy_of_probs_ms': round(med['copy_graph'], 5), 'graph_multiple_of_copy': round(med['decode_graph'] / med['copy_graph'], 3),
            'eager_ms_per_call': round(med['decode_eager'], 5), 'eager_copy_of_probs_ms': round(med['copy_eager'], 5),
            'torch_composition_ms': round(med['torch'], 3), 'torch_composition_over_graph_decode': round(med['torch'] / med['decode_graph'], 1),
            'equals_decode_reference': bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x640,4x2200', help='B x TL, comma separated')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--ref-iters', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    out = {'classes': C, 'iters': a.iters, 'graph_calls_per_replay': 50, 'device': cfn_hip.device_info(), 'shapes': {}}
    for shape in a.shapes.split(','):
        B, TL = (int(v) for v in shape.split('x'))
        out['shapes']['%dx%dx%d' % (B, C, TL)] = {kind: measure(B, TL, kind, torch.device('cuda:0'), a.iters, a.ref_iters)
                                                  for kind in ('sparse', 'alternating')}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
