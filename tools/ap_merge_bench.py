#!/usr/bin/env python
"""Merging class-major AP stores on the GPU (cfn_hip.ops.ap_merge; csrc/apmerge.hip): R = 2, 4, 8 parts appended behind a destination that
holds 3 rows, at the two shapes the meters have:

  segment     157 classes x 4096 rows per class and part, one count per class plus n_gt (SegmentAPMeter)
  frame       157 classes x 2^17 rows per part, ONE count for all classes (DeviceAPMeter: a logging interval of the training meter)

Part r holds cap_s - (r % 4) rows, so the parts' bases in the destination take every byte alignment.  Per shape and R, alternating in the
same run, device time per call with the calls captured in one graph (each call is preceded by the reset of the destination's small state
vector, in both runs):

  merge       ONE ap_merge call (2 kernel nodes)
  copy        torch's copy_ of the same rows, part by part: scores and payload, 2 R strided device-to-device copies -- the yardstick; it needs
              the counts on the HOST, which a meter does not have without a read-back

The result of the timed merge is compared with the copies' bit for bit.  No time is a pass criterion and none is promised: the merge runs
once per validation phase, off the step's critical path.  One JSON document on stdout and in --out.

    python tools/ap_merge_bench.py --out profiles/ap_merge.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import torch  # noqa: E402

from cfn_hip import ops  # noqa: E402

C = 157
SHAPES = {'segment': (4096, True), 'frame': (1 << 17, False)}        # rows per class and part, one count per class?
HELD = 3                                                              # rows the destination holds in front


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


def measure(name, R, dev, repeats):
    cap_s, per_class = SHAPES[name]
    n_cnt, n_extra = (C, C) if per_class else (1, 0)
    g = torch.Generator(device=dev).manual_seed(R + cap_s)
    src_s = torch.rand(R, C, cap_s, device=dev, generator=g)
    src_p = torch.randint(0, 256, (R, C, cap_s), device=dev, generator=g, dtype=torch.uint8)
    rows = [cap_s - (r % 4) for r in range(R)]
    cap_d = HELD + sum(rows)
    src_state = torch.zeros(R, n_cnt + n_extra + 1, dtype=torch.int32)
    for r in range(R):
        src_state[r, :n_cnt] = rows[r]
        src_state[r, n_cnt:n_cnt + n_extra] = r + 1
    src_state = src_state.to(dev)
    src_counts, src_extra, src_flags = src_state[:, :n_cnt].contiguous(), src_state[:, n_cnt:n_cnt + n_extra].contiguous(), src_state[:, -1].contiguous()
    state0 = torch.zeros(n_cnt + n_extra + 1, dtype=torch.int32)
    state0[:n_cnt] = HELD
    state0 = state0.to(dev)
    ws = torch.empty(ops.ap_merge_workspace_bytes(R, C), dtype=torch.uint8, device=dev)

    def store():
        return (torch.zeros(C, cap_d, device=dev), torch.zeros(C, cap_d, dtype=torch.uint8, device=dev), state0.clone())
    m_s, m_p, m_state = store()
    c_s, c_p, c_state = store()

    def merge():
        m_state.copy_(state0)
        ops.ap_merge(m_s, m_p, m_state[:n_cnt], m_state[n_cnt:n_cnt + n_extra] if n_extra else None, m_state[-1:], src_s, src_p, src_counts,
                     src_extra if n_extra else None, src_flags, out=ws)

    def copy():
        c_state.copy_(state0)
        at = HELD
        for r in range(R):
            c_s[:, at:at + rows[r]].copy_(src_s[r, :, :rows[r]])
            c_p[:, at:at + rows[r]].copy_(src_p[r, :, :rows[r]])
            at += rows[r]
    runs = {'merge': merge, 'copy': copy}
    raw = {k: [] for k in runs}
    for _ in range(repeats):                                         # alternating
        for k, fn in runs.items():
            raw[k].append(graph_ms(fn))
    med = {k: statistics.median(v) for k, v in raw.items()}
    merge()
    copy()
    torch.cuda.synchronize()
    moved = C * sum(rows) * 5
    same = bool(torch.equal(m_s.view(torch.int32), c_s.view(torch.int32)) and torch.equal(m_p, c_p))
    committed = bool((m_state[:n_cnt] == cap_d).all()) and int(m_state[-1]) == 0
    res = {'parts': R, 'rows_per_class_and_part': cap_s, 'rows_per_class_merged': sum(rows), 'bytes_moved': moved,
           'equals_the_copies': same, 'committed_without_a_flag': committed}
    for k in runs:
        res[k + '_graph_ms'] = round(med[k], 5)
        res[k + '_min_max'] = [round(min(raw[k]), 5), round(max(raw[k]), 5)]
    res['merge_over_copy'] = round(med['merge'] / med['copy'], 3)
    res['merge_GBps_read_plus_write'] = round(2 * moved / med['merge'] / 1e6, 1)
    res['copy_GBps_read_plus_write'] = round(2 * moved / med['copy'] / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='2,4,8', help='R, comma separated')
    ap.add_argument('--shapes', default='segment,frame')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measures the HIP path: it needs a GPU'
    import cfn_hip
    dev = torch.device('cuda:0')
    out = {'classes': C, 'held_rows': HELD, 'repeats': a.repeats, 'device': cfn_hip.device_info(), 'shapes': {}}
    for name in a.shapes.split(','):
        out['shapes'][name] = {}
        for R in (int(v) for v in a.parts.split(',')):
            out['shapes'][name]['R%d' % R] = measure(name, R, dev, a.repeats)
            torch.cuda.empty_cache()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
