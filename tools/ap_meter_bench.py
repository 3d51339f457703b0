#!/usr/bin/env python
"""The device-resident AP meter (csrc/apmeter.hip, apmeter.DeviceAPMeter, cfn_hip.metrics.StepMetrics), measured:

  1. value(): the host `APMeter.value()` and `DeviceAPMeter.value()` on the SAME rows, K = 157 classes, n = 8 x 640 x {40, 490} rows (40
     steps' worth, and the half epoch after which the loops log).  Beside the wall times: the sort and the reduce kernels by themselves
     (HIP events) with the bytes each moves -- histogram: 4 n K read; each of the 4 radix passes: 5 n K read + 5 n K written; reduce: n K.
     The host meter is timed once per n (it takes seconds to minutes); the device legs run around it, alternating.
  2. the fine train step at the default training shape (8 clips x 64 frames x 224 x 224, labels 8 x 157 x 640), three ways in one
     process, legs alternating: bare; followed by StepMetrics(False).update (host meter, a read-back per video and per loss); followed by
     StepMetrics(True).update (device meter, nothing read back).  Wall time per step over `--steps` steps with ONE synchronisation at
     the end, so a leg whose host runs ahead of the device is credited for it.  The append kernel by itself: HIP events.

Per figure: median over the repeats with min / max.  One JSON document on stdout and in --out.

    python tools/ap_meter_bench.py --out profiles/ap_meter.json
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
import torch.optim as optim  # noqa: E402

import apmeter  # noqa: E402
import cfn_hip  # noqa: E402
import train_fine  # noqa: E402
from cfn_hip import dist as cdist  # noqa: E402
from cfn_hip import ops  # noqa: E402
from cfn_hip.metrics import StepMetrics  # noqa: E402

K = 157


def events_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v, nd=4):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


def batch(dev, seed, B, TL):
    g = torch.Generator(device=dev).manual_seed(seed)
    probs = torch.sigmoid(2.0 * torch.randn(B, K, TL, generator=g, device=dev) - 2.0)
    labels = (torch.rand(B, K, TL, generator=g, device=dev) < 0.05).float()
    return probs, labels


def value_leg(dev, B, TL, steps, repeats, host):
    n = B * TL * steps
    meter = apmeter.DeviceAPMeter(dev)
    host_meter = apmeter.APMeter() if host else None
    for s in range(steps):
        probs, labels = batch(dev, 100 + s, B, TL)
        meter.add_batch(probs, labels)
        if host:
            for b in range(B):
                host_meter.add(probs[b].t().cpu().numpy(), labels[b].t().cpu().numpy())
    scores, targets = meter.stores
    cap = scores.shape[1]
    bufs = (torch.empty_like(scores), torch.empty_like(targets), torch.empty(K, cap, dtype=torch.int32, device=dev), torch.empty_like(targets))
    sort = lambda: ops.ap_sort(scores, targets, meter.count, out=bufs)
    reduce_ = lambda: ops.ap_reduce(bufs[1], meter.count)
    sort()
    reduce_()
    torch.cuda.synchronize()
    sm, rm, vm = [], [], []

    def device_round():
        sm.append(events_ms(sort))
        rm.append(events_ms(reduce_))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = meter.value()
        vm.append((time.perf_counter() - t0) * 1e3)
        return v
    for _ in range(repeats):
        dv = device_round()
    res = {'rows': n, 'classes': K, 'capacity': cap, 'sort_kernel_ms': None, 'reduce_kernel_ms': None, 'device_value_ms': None}
    if host:
        t0 = time.perf_counter()
        hv = host_meter.value()
        res['host_value_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        res['max_abs_diff_device_vs_host'] = float((dv.double() - hv.double()).abs().max())
        for _ in range(repeats):
            device_round()
    nk = n * K
    res.update({'sort_kernel_ms': stats(sm), 'reduce_kernel_ms': stats(rm), 'device_value_ms': stats(vm),
                'bytes': {'histogram_read': 4 * nk, 'per_radix_pass_read': 5 * nk, 'per_radix_pass_written': 5 * nk, 'radix_passes': 4,
                          'sort_total': 44 * nk, 'reduce_read': nk},
                'sort_GBps': round(44 * nk / statistics.median(sm) / 1e6, 1), 'reduce_GBps': round(nk / statistics.median(rm) / 1e6, 1)})
    if host:
        res['host_over_device'] = round(res['host_value_ms'] / statistics.median(vm), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--label-frames', type=int, default=640)
    ap.add_argument('--crop', type=int, default=224)
    ap.add_argument('--value-steps', type=int, nargs='*', default=[40, 490], help="steps' worth of rows per value() leg")
    ap.add_argument('--no-host-value', action='store_true', help='skip the host meter in the value() legs (minutes at 490 steps)')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='skip the train-step legs')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures the HIP path; it needs a GPU'
    dev = torch.device('cuda:0')
    B, T, TL, S = a.batch, a.frames, a.label_frames, a.crop
    out = {'shape': {'clips': B, 'frames': T, 'label_frames': TL, 'size': S, 'classes': K}, 'repeats': a.repeats, 'device': cfn_hip.device_info(),
           'sort_tile': ops.AP_SORT_TILE, 'value': {}}

    for steps in a.value_steps:
        out['value']['%d_steps' % steps] = r = value_leg(dev, B, TL, steps, a.repeats, not a.no_host_value)
        print('value() over %d rows: device %.2f ms (sort %.2f, reduce %.3f), host %s ms'
              % (r['rows'], r['device_value_ms']['median'], r['sort_kernel_ms']['median'], r['reduce_kernel_ms']['median'], r.get('host_value_ms')),
              file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    if not a.no_step:
        torch.manual_seed(0)
        net = train_fine.build_model(dev, pretrained=None)
        net.train(True)
        optimizer = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
        reducer = cdist.GradReducer(net.parameters())
        g = torch.Generator().manual_seed(3)
        x = torch.randn(B, 3, T, S, S, generator=g).to(dev)
        labels = (torch.rand(B, K, TL, generator=g) < 0.05).float().to(dev)
        masks = torch.zeros(B, TL)
        for b in range(B):
            masks[b, :TL - 40 * b] = 1
        masks = masks.to(dev)
        valid_t = masks.sum(1).int()
        labels = labels * masks.unsqueeze(1)
        meters = {'bare': None, 'host_metrics': StepMetrics(False), 'device_metrics': StepMetrics(True, dev)}

        def leg(kind):
            sm = meters[kind]
            if sm is not None:
                sm.start_phase()
                sm.reset_ap()

            def one():
                cls, loc, probs = train_fine.train_step(net, reducer, optimizer, x, labels, masks)
                if sm is not None:
                    sm.update(cls, loc, probs, labels, valid_t)
            for _ in range(a.warmup):
                one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                one()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3
        res = {k: [] for k in meters}
        for _ in range(a.repeats):
            for k in meters:
                res[k].append(leg(k))
            print('step: ' + ', '.join('%s %.3f ms' % (k, res[k][-1]) for k in meters), file=sys.stderr, flush=True)
        probs, _ = batch(dev, 5, B, TL)
        m = apmeter.DeviceAPMeter(dev, capacity=B * TL * 64)
        m.add_batch(probs, labels, valid_t)
        torch.cuda.synchronize()
        am = []
        for _ in range(a.repeats):
            m.reset()
            am.append(events_ms(lambda: m.add_batch(probs, labels, valid_t), 20))
        med = {k: statistics.median(v) for k, v in res.items()}
        out['fine_train_step'] = {'steps': a.steps, 'warmup': a.warmup, 'bare_ms': stats(res['bare'], 3), 'host_metrics_ms': stats(res['host_metrics'], 3),
                                  'device_metrics_ms': stats(res['device_metrics'], 3), 'append_kernel_ms': stats(am),
                                  'bare_spread_ms': round(max(res['bare']) - min(res['bare']), 3),
                                  'device_minus_bare_ms': round(med['device_metrics'] - med['bare'], 3),
                                  'host_minus_bare_ms': round(med['host_metrics'] - med['bare'], 3)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
