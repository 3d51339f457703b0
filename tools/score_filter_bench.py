#!/usr/bin/env python
"""Temporal filtering of per-frame scores on the GPU (cfn_hip.scorefilter.apply, csrc/scorefilter.hip), at 8 x 157 x 640 (the training window)
and 4 x 157 x 2,200 (whole validation videos), on the sparse probabilities of tools/detections_bench.py; radii 2, 8 and 32 under both
methods (0 = weighted mean with the box table, 1 = median).  Per shape, radius and method, the legs alternating in the same run:

  filter      apply(out=) per call, device time with the calls captured in one graph
  copy        a device copy of probs (dst.copy_(probs)) the same way: the floor, one read and one write of the tensor
  torch       what a caller would write instead, timed EAGERLY with events (a chain of torch operators with temporaries of their own, so
              launch gaps are part of the figure -- as they would be for that caller):
                mean     conv1d of probs * mask with the box kernel, divided by the conv1d of the mask (renormalised edges)
                median   pad with NaN, unfold(2r + 1), nanmedian over the window (the LOWER median where a truncated window is even: not rule
                         F5's mean of the two middle values, so it is a timing leg only)

The timed output is compared with filter_reference once per configuration (bit-equal).  No time is a pass criterion.  One JSON document on
stdout and in --out.

    python tools/score_filter_bench.py --out profiles/score_filter.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import cfn_hip  # noqa: E402
from cfn_hip.scorefilter import ScoreFilter, apply, filter_reference  # noqa: E402
from detections_bench import event_ms, graph_ms, make_probs  # noqa: E402

C = 157


def torch_mean(probs, mask, r):
    k = torch.ones(1, 1, 2 * r + 1, device=probs.device)
    B, Cc, TL = probs.shape
    num = F.conv1d((probs * mask[:, None, :]).reshape(B * Cc, 1, TL), k, padding=r)
    den = F.conv1d(mask[:, None, :], k, padding=r).clamp_(min=1.0)
    return torch.where(mask[:, None, :] > 0, num.view(B, Cc, TL) / den, probs)


def torch_median(probs, mask, r):
    p = torch.where(mask[:, None, :] > 0, probs, torch.full_like(probs, float('nan')))
    win = F.pad(p, (r, r), value=float('nan')).unfold(2, 2 * r + 1, 1)
    return torch.where(mask[:, None, :] > 0, win.nanmedian(dim=3).values, probs)


def measure(B, TL, r, method, dev, launches, replays, torch_iters):
    probs = make_probs(B, TL, 'sparse', 7 * B + TL).to(dev)
    valid_host = torch.tensor([TL - 37 * b for b in range(B)], dtype=torch.int32)
    valid = valid_host.to(dev)
    mask = (torch.arange(TL, device=dev)[None, :] < valid[:, None]).float()
    flt = ScoreFilter('box' if method == 0 else 'median', r)
    out, dst = torch.empty_like(probs), torch.empty_like(probs)
    run = lambda: apply(probs, valid, flt, out=out)
    copy = lambda: dst.copy_(probs)
    other = (lambda: torch_mean(probs, mask, r)) if method == 0 else (lambda: torch_median(probs, mask, r))
    raw = {'filter': [], 'copy': [], 'torch': []}
    for _ in range(5):                                               # alternating
        raw['filter'].append(graph_ms(run, launches, replays))
        raw['copy'].append(graph_ms(copy, launches, replays))
        raw['torch'].append(event_ms(other, torch_iters, warmup=1))
    med = {k: statistics.median(v) for k, v in raw.items()}
    run()
    ref = filter_reference(probs.cpu(), valid_host, flt)
    same = bool(torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32)))
    nbytes = 2.0 * probs.numel() * 4
    return {'graph_calls_per_replay': launches, 'filter_graph_ms': round(med['filter'], 5), 'filter_min': round(min(raw['filter']), 5),
            'filter_max': round(max(raw['filter']), 5), 'copy_graph_ms': round(med['copy'], 5), 'multiple_of_the_copy': round(med['filter'] / med['copy'], 2),
            'filter_gb_per_s': round(nbytes / med['filter'] / 1e6, 1), 'torch_eager_ms': round(med['torch'], 5),
            'torch_over_filter': round(med['torch'] / med['filter'], 1), 'equals_filter_reference': same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--replays', type=int, default=10)
    ap.add_argument('--torch-iters', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'classes': C, 'device': cfn_hip.device_info(), 'tile': int(cfn_hip.query('cfn_score_filter_tile')), 'shapes': {}}
    for B, TL in ((8, 640), (4, 2200)):
        shape = res['shapes']['%dx%dx%d' % (B, C, TL)] = {}
        for method, name in ((0, 'mean'), (1, 'median')):
            for r in (2, 8, 32):
                shape['%s_r%d' % (name, r)] = measure(B, TL, r, method, dev, args.launches, args.replays, args.torch_iters)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
