#!/usr/bin/env python
"""The fused detection loss (csrc/detloss.hip, cfn_hip.ops.detection_loss) against the composed operator chain of train_fine.detection_loss,
in ONE process, legs alternating:

  1. the loss by itself at three shapes -- (8, 157, 256 -> 2560, align_corners) forward + backward: the fine benchmark's; (8, 157, 128 -> 640,
     half-pixel) forward + backward: the coarse stream's; (4 x 3 crops, 157, 256 -> 2560) forward under no_grad: validation.  HIP events around
     `--calls` calls per sample, `--repeats` samples per leg; median with min / max.  Kernel launches of one call: the device-side kernel
     records of torch.profiler (memcpy / memset records left out).  Beside the times: the bytes the fused kernels have to move (labels and
     masks read forward and backward, probs written once, logits and their gradient) and the rate that makes of the median.
  2. kernel launches of one fine train step (1 clip x 64 frames x 224 x 224; the count does not depend on the batch), both settings.
  3. outputs of both paths at the timed shapes: max |difference| of the losses, probs and the logit gradient.

The step-level A/B is taken with bench.py itself under CFN_FUSED_LOSS=0 / 1; `--merge-bench NAME=FILE ...` copies such result lines into the
same document.  One JSON document on stdout and in --out.

    python tools/loss_bench.py --out profiles/fused_loss.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import torch  # noqa: E402
import torch.optim as optim  # noqa: E402
from torch.profiler import profile, ProfilerActivity  # noqa: E402

import cfn_hip  # noqa: E402
import train_fine  # noqa: E402
from cfn_hip import dist as cdist  # noqa: E402

K = 157
SHAPES = [      # name, videos, crops, T, TL, align_corners, backward
    ('fine_train', 8, 1, 256, 2560, True, True),
    ('coarse_train', 8, 1, 128, 640, False, True),
    ('fine_val_3crops', 4, 3, 256, 2560, True, False),
]


def stats(v, nd=4):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def kernel_launches(fn):
    """device-side kernel records of one call (None when the profiler yields no device records on this build)"""
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kern = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and not any(s in e.name.lower() for s in ('memcpy', 'memset'))]
    return len(kern) or None


def loss_case(dev, B, n, T, TL, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B * n, K, T, generator=g) * 3).to(dev)
    labels = (torch.rand(B, K, TL, generator=g) < 0.05).float().to(dev)
    masks = torch.zeros(B, TL)
    for b in range(B):
        masks[b, :TL - (TL // 64) * b] = 1
    return logits, labels, masks.to(dev)


def isolated(dev, name, B, n, T, TL, ac, backward, a):
    logits, labels, masks = loss_case(dev, B, n, T, TL, 11)
    x = logits.clone().requires_grad_(backward)

    def call(fused):
        if backward:
            x.grad = None
            cls, loc, probs = train_fine.detection_loss(x, labels, masks, ac, crops=n, local_norm=True, fused=fused)
            ((cls + loc) / 2).backward()
            return cls, loc, probs, x.grad
        with torch.no_grad():
            return train_fine.detection_loss(x, labels, masks, ac, crops=n, local_norm=True, fused=fused) + (None,)

    legs = {'composed': lambda: call(False), 'fused': lambda: call(True)}
    outs = {k: [None if v is None else v.detach().clone() for v in f()] for k, f in legs.items()}
    for f in legs.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, f in legs.items():
            ms[k].append(events_ms(f, a.calls))
    bc = B * K
    by = 4 * (bc * TL * 2 + B * TL + bc * n * T) + (4 * (bc * TL + B * TL + 2 * bc * n * T) if backward else 0)
    res = {'shape': {'videos': B, 'crops': n, 'classes': K, 'T': T, 'TL': TL, 'align_corners': ac, 'backward': backward},
           'calls_per_sample': a.calls, 'samples': a.repeats,
           'composed_ms': stats(ms['composed']), 'fused_ms': stats(ms['fused']),
           'composed_over_fused': round(statistics.median(ms['composed']) / statistics.median(ms['fused']), 2),
           'launches': {k: kernel_launches(f) for k, f in legs.items()},
           'fused_algorithmic_bytes': by, 'fused_GBps_of_median': round(by / statistics.median(ms['fused']) / 1e6, 1),
           'max_abs_diff_fused_vs_composed': {nm: (None if u is None else float((u.double() - v.double()).abs().max()))
                                              for nm, u, v in zip(('cls', 'loc', 'probs', 'grad'), outs['fused'], outs['composed'])}}
    print('%s: composed %.4f ms, fused %.4f ms, launches %s' % (name, res['composed_ms']['median'], res['fused_ms']['median'], res['launches']),
          file=sys.stderr, flush=True)
    return res


def step_launches(dev):
    torch.manual_seed(0)
    net = train_fine.build_model(dev, pretrained=None)
    net.train(True)
    optimizer = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    reducer = cdist.GradReducer(net.parameters())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, 64, 224, 224, generator=g).to(dev)
    labels = (torch.rand(1, K, 640, generator=g) < 0.05).float().to(dev)
    masks = torch.ones(1, 640, device=dev)
    res = {'shape': {'clips': 1, 'frames': 64, 'size': 224, 'label_frames': 640}}
    for name, fused in (('composed', False), ('fused', True)):
        one = lambda: train_fine.train_step(net, reducer, optimizer, x, labels, masks, fused=fused)
        for _ in range(2):
            one()
        res[name] = kernel_launches(one)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200, help='calls between the two HIP events of one sample')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7, help='samples per leg (legs alternate)')
    ap.add_argument('--no-step', action='store_true', help='skip the launch count of the train step')
    ap.add_argument('--merge-bench', nargs='*', default=[], metavar='NAME=FILE', help='result lines of bench.py to copy into the document')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures the HIP path; it needs a GPU'
    dev = torch.device('cuda:0')
    cfn_hip.load()
    out = {'device': cfn_hip.device_info(), 'isolated': {}}
    for name, B, n, T, TL, ac, backward in SHAPES:
        out['isolated'][name] = isolated(dev, name, B, n, T, TL, ac, backward, a)
    if not a.no_step:
        out['fine_train_step_launches'] = step_launches(dev)
    if a.merge_bench:
        out['bench'] = {}
        for item in a.merge_bench:
            name, path = item.split('=', 1)
            with open(path) as fh:
                lines = [ln for ln in fh.read().splitlines() if ln.startswith('{')]
            out['bench'][name] = json.loads(lines[-1])
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
