#!/usr/bin/env python3
"""Kernel-level A/B of the fused stem pair (csrc/stempair.hip) against the kernels it replaces, at 8 x 3 x 256 x 224 x 224, in one process
with HIP events, the candidates interleaved round by round:
    python tools/stem_pair_bench.py [--json out.json] [--runs 0,32,64,128] [--only fwd|bwd]
forward:  cfn_stem_conv_fwd + cfn_dwconv_t5_fwd             against cfn_stem_pair_fwd   (should move 6.17 GB)
backward: cfn_dwconv_t5_bwd_fused + cfn_stem_conv_bwd_weight against cfn_stem_pair_bwd   (should move 8.63 GB)
--once fwd|bwd|both launches the fused kernel(s) twice each and nothing else after the set-up (for a counter run under a profiler)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))
import torch  # noqa: E402
import cfn_hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--json')
ap.add_argument('--runs', default='0,32,64,128')
ap.add_argument('--only', choices=['fwd', 'bwd'])
ap.add_argument('--once', choices=['fwd', 'bwd', 'both'])
ap.add_argument('--rounds', type=int, default=12)
args = ap.parse_args()
cfn_hip.load()
B, T = int(os.environ.get('B', 8)), int(os.environ.get('T', 256))
dev = 'cuda'
x = torch.randn(B, 3, T, 224, 224, device=dev)
ws, wt = torch.randn(24, 27, device=dev) * 0.3, torch.randn(24, 5, device=dev) * 0.4
xs = torch.empty(B, 24, T, 112, 112, device=dev)
y, gy, gxs = torch.empty_like(xs), torch.randn(B, 24, T, 112, 112, device=dev), torch.empty_like(xs)
s, q = torch.zeros(B, 24, dtype=torch.float64, device=dev), torch.zeros(B, 24, dtype=torch.float64, device=dev)
gs, gq = torch.randn(B, 24, dtype=torch.float64, device=dev), torch.randn(B, 24, dtype=torch.float64, device=dev) * 0.1
gwt, gws = torch.zeros(24, 5, dtype=torch.float64, device=dev), torch.zeros(24, 27, dtype=torch.float64, device=dev)
P = 112 * 112
GB_F = 4.0 * B * T * (3 * 224 * 224 + 2 * 24 * P) / 1e9
GB_B = 4.0 * B * T * (3 * 224 * 224 + 3 * 24 * P) / 1e9


def fwd_pair():
    cfn_hip.call('cfn_stem_conv_fwd', x, ws, xs, B, 3, 24, T, 224, 224)
    cfn_hip.call('cfn_dwconv_t5_fwd', xs, wt, y, s, q, B, 24, T, P)


def bwd_pair():
    cfn_hip.call('cfn_dwconv_t5_bwd_fused', gy, y, gs, gq, wt, xs, gxs, gwt, B, 24, T, P)
    cfn_hip.call('cfn_stem_conv_bwd_weight', gxs, x, gws, B, 3, 24, T, 224, 224)


def fwd_fused(r):
    return lambda: cfn_hip.call('cfn_stem_pair_fwd', x, ws, wt, xs, y, s, q, B, 3, 24, T, 224, 224, r)


def bwd_fused(r):
    return lambda: cfn_hip.call('cfn_stem_pair_bwd', gy, y, gs, gq, wt, xs, x, gwt, gws, B, 3, 24, T, 224, 224, r)


fwd_pair()
torch.cuda.synchronize()
if args.once:
    for fn in ([fwd_fused(0)] if args.once != 'bwd' else []) + ([bwd_fused(0)] if args.once != 'fwd' else []):
        fn()
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
    sys.exit(0)

runs = [int(v) for v in args.runs.split(',')]
cands = []
if args.only != 'bwd':
    cands += [('fwd pair', fwd_pair, GB_F)] + [('fwd fused run_frames=%d' % r, fwd_fused(r), GB_F) for r in runs]
if args.only != 'fwd':
    cands += [('bwd pair', bwd_pair, GB_B)] + [('bwd fused run_frames=%d' % r, bwd_fused(r), GB_B) for r in runs]
for _, fn, _ in cands:
    fn()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ms = {name: [] for name, _, _ in cands}
for _ in range(args.rounds):
    for name, fn, _ in cands:
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / 5)
out = {}
for name, _, gb in cands:
    v = sorted(ms[name])
    med = v[len(v) // 2]
    out[name] = {'min_ms': v[0], 'median_ms': med, 'max_ms': v[-1], 'gb': gb, 'tbps_at_median': gb / med}
    print('%-28s min %.3f  median %.3f  max %.3f ms   %.2f GB -> %.2f TB/s' % (name, v[0], med, v[-1], gb, gb / med))
if args.json:
    with open(args.json, 'w') as fh:
        json.dump({'shape': [B, 3, T, 224, 224], 'rounds': args.rounds, 'launches_per_round': 5, 'results': out}, fh, indent=1)
