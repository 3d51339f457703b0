#!/usr/bin/env python
"""Frame labels rasterised from annotation segments on the GPU against the dense label path, at 8 x 157 x 640 (the training window) and
4 x 157 x 2,200 (whole validation videos):

  1. kernel        SegLabels.dense(out=) (device events), beside a device-to-device copy of the SAME OUTPUT BYTES (labels + mask) and as a
                   multiple of it; achieved bytes/s from the algorithmic bytes (the outputs; the inputs are a few hundred bytes).  Twice:
                   launched eagerly from Python (a few microseconds of kernel behind a longer enqueue: the host's rate), and 100 launches
                   captured in one graph (device time per launch)
  2. host collate  collate.fine_collate of samples with dense (157, TL) labels against the same samples with SegLabel members, seconds per
                   batch; the clips are 1 x 3 x 1 x 8 x 8, so that the leg times the labels, which is what differs.  --host-only runs this
                   leg alone, on any CPU: the JSON labels it with the machine it ran on
  3. bytes staged  what HostStager lays out per batch for the label and mask members of either kind (from its own plan: every tensor on a
                   256-byte boundary)

No pass bar: the dense path is the comparison, the JSON is the record.  One JSON document on stdout and in --out.

    python tools/seg_labels_bench.py --out profiles/seg_labels.json
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import collate  # noqa: E402
from cfn_hip import staging  # noqa: E402
from cfn_hip.seglabels import SegLabel  # noqa: E402

C = 157


def make_samples(B, TL, seed):
    """per-video samples as a Dataset would return them: about 7 actions per video (the mean of the Charades annotations), 24 frames per
    second, a window of TL frames; the dense twin is the array of the same window"""
    r = np.random.RandomState(seed)
    seg, dense = [], []
    for i in range(B):
        fps, start = 24.0, int(r.randint(0, 200))
        acts = []
        for _ in range(int(r.randint(3, 12))):
            s = float(r.uniform(0, (start + TL) / fps))
            acts.append([int(r.randint(0, C)), round(s, 2), round(s + float(r.uniform(1, 15)), 2)])
        lb = SegLabel(acts, fps, start, TL)
        clip = torch.zeros(1, 3, 1, 8, 8)
        seg.append((clip, lb, 'v%d' % i))
        dense.append((clip, lb.dense_reference(), 'v%d' % i))
    return dense, seg


def host_collate(dense, seg, repeats):
    legs = {'dense': dense, 'segments': seg}
    secs = {k: [] for k in legs}
    by = {}
    for _ in range(repeats + 1):                       # alternating; the first visit warms the allocator
        for name, smp in legs.items():
            t0 = time.perf_counter()
            batch = collate.fine_collate(smp)
            secs[name].append(time.perf_counter() - t0)
            by[name] = staging.HostStager._plan([batch[1], batch[2]])[1]
    return {name: {'s_per_batch': round(statistics.median(v[1:]), 6), 'min': round(min(v[1:]), 6), 'max': round(max(v[1:]), 6),
                   'label_and_mask_bytes_staged_per_batch': by[name]} for name, v in secs.items()}


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


def graph_ms(fn, launches=100, replays=20):
    """device time per launch with `launches` of them captured in one graph: no host enqueue between the kernels (the gap between two
    nodes of a graph stays in the figure)"""
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


def kernel(seg, dev, iters):
    sl = collate.fine_collate(seg)[1].to(dev)
    out = (torch.empty(sl.batch, C, sl.t_max, device=dev), torch.empty(sl.batch, sl.t_max, device=dev),
           torch.empty(sl.batch, dtype=torch.int32, device=dev))
    n_out = out[0].numel() + out[1].numel()
    src, dst = torch.empty(n_out, device=dev), torch.empty(n_out, device=dev)
    raw = {'dense': [], 'copy': [], 'dense_graph': [], 'copy_graph': []}
    for _ in range(5):                                 # alternating
        raw['dense'].append(event_ms(lambda: sl.dense(out=out), iters))
        raw['copy'].append(event_ms(lambda: dst.copy_(src), iters))
        raw['dense_graph'].append(graph_ms(lambda: sl.dense(out=out)))
        raw['copy_graph'].append(graph_ms(lambda: dst.copy_(src)))
    ref = sl.dense_reference()
    exact = all(bool(torch.equal(o, w)) for o, w in zip(out, ref))
    med = {k: statistics.median(v) for k, v in raw.items()}
    return {'ms': round(med['dense'], 5), 'min': round(min(raw['dense']), 5), 'max': round(max(raw['dense']), 5), 'output_bytes': n_out * 4,
            'segments': int(sl.seg.shape[0]), 'GB_per_s': round(n_out * 4 / med['dense'] / 1e6, 1), 'copy_of_output_ms': round(med['copy'], 5),
            'multiple_of_copy': round(med['dense'] / med['copy'], 3),
            # the two figures above are eager launches from Python: at these sizes they measure the host's enqueue rate as much as the kernel.
            # Below: 100 launches per graph replay
            'graph_ms_per_launch': round(med['dense_graph'], 5), 'graph_copy_ms_per_launch': round(med['copy_graph'], 5),
            'graph_multiple_of_copy': round(med['dense_graph'] / med['copy_graph'], 3),
            'graph_GB_per_s': round(n_out * 4 / med['dense_graph'] / 1e6, 1), 'equals_dense_reference': exact}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x640,4x2200', help='B x TL, comma separated')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--kernel-iters', type=int, default=500)
    ap.add_argument('--host-only', action='store_true', help='the host-collate and bytes legs alone (runs without a GPU)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    gpu = torch.cuda.is_available()
    if not a.host_only:
        assert gpu, 'the kernel leg measures the HIP path: it needs a GPU (--host-only: the collate leg alone)'
    out = {'classes': C, 'repeats': a.repeats, 'kernel_iters': a.kernel_iters,
           'host': {'machine': platform.machine(), 'cpus': os.cpu_count(), 'torch_threads': torch.get_num_threads(),
                    'kind': 'GPU host' if gpu else 'build machine (no GPU): host-collate times only, not the training host'},
           'shapes': {}}
    if gpu and not a.host_only:
        import cfn_hip
        out['device'] = cfn_hip.device_info()
    for shape in a.shapes.split(','):
        B, TL = (int(v) for v in shape.split('x'))
        dense, seg = make_samples(B, TL, 1234 + B)
        res = {'host_collate': host_collate(dense, seg, a.repeats)}
        if not a.host_only:
            res['kernel'] = kernel(seg, torch.device('cuda:0'), a.kernel_iters)
        out['shapes']['%dx%dx%d' % (B, C, TL)] = res
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
