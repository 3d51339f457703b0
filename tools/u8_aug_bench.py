#!/usr/bin/env python
"""Crop + resize + flip of uint8 frames on the GPU (csrc/aug_u8.hip), measured (default 8 clips x 256 frames into 224 x 224):

  1. the kernel by itself, HIP events around `--reps` launches, for 180 x 320, 240 x 320 and 360 x 480 source frames with the boxes the
     reference's training transform draws (scales 0.875 / 0.7); beside it, IN THE SAME RUN, a device-to-device copy that moves the same
     number of bytes (the whole source read once + the output written once, half of it read and half written by the copy): the copy is
     the yardstick, not the spec peak.  Ratio = kernel time / copy time.
  2. the fine train step fed RawU8Clips resident in HBM (transform on the step's stream, then the step) against the same step on the
     U8Clips that transform produces, resident too; legs alternating.

Per figure: median over the repeats with min / max.  One JSON document on stdout and in --out.

    python tools/u8_aug_bench.py --out profiles/u8_aug.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import torch  # noqa: E402
import torch.optim as optim  # noqa: E402

import cfn_hip  # noqa: E402
import train_fine  # noqa: E402
from cfn_hip import dist as cdist  # noqa: E402
from cfn_hip import ops, u8aug  # noqa: E402
from cfn_hip.u8clips import RawU8Clips, CHARADES_MEAN, CHARADES_STD  # noqa: E402

SCALES = [0.875, 0.7]
# PIL on ONE core of the build machine (not the GPU host): crop().resize((224, 224), BILINEAR).transpose(FLIP_LEFT_RIGHT), per frame
HOST_PIL_MS_PER_FRAME = {'180x320': 0.98, '240x320': 0.77, '360x480': 1.28}


def raw_batch(B, T, h, w, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rng = random.Random(seed)
    frames = torch.randint(0, 256, (B, T, h, w, 3), generator=g, dtype=torch.uint8, device=dev)
    box = torch.tensor([u8aug.train_crop_params(rng, (h, w), SCALES, 224) for _ in range(B)], dtype=torch.int32)
    return RawU8Clips(frames, torch.full((B,), T, dtype=torch.int32, device=dev), box.to(dev)), box


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v, nd=4):
    return {'median': round(statistics.median(v), nd), 'min': round(min(v), nd), 'max': round(max(v), nd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--crop', type=int, default=224)
    ap.add_argument('--reps', type=int, default=20, help='launches per timed window of the kernel / copy legs')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='skip the train-step legs')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures the HIP path; it needs a GPU'
    dev = torch.device('cuda:0')
    B, T, S = a.batch, a.frames, a.crop
    out = {'shape': {'clips': B, 'frames': T, 'size': S}, 'reps': a.reps, 'repeats': a.repeats, 'device': cfn_hip.device_info(), 'kernel': {},
           'host_pil_one_core_build_machine': {k: {'ms_per_frame': v, 'core_seconds_per_step': round(v * B * T / 1e3, 2)} for k, v in HOST_PIL_MS_PER_FRAME.items()}}

    for h, w in ((180, 320), (240, 320), (360, 480)):
        raw, box = raw_batch(B, T, h, w, dev, 7)
        tabs = ops.aug_tables(box, S, dev)
        dst = torch.empty(B, T, S, S, 3, dtype=torch.uint8, device=dev)
        nbytes = raw.frames.numel() + dst.numel()
        window = int(sum(int(c) * int(c) * 3 * T for c in box[:, 2])) + dst.numel()
        half = nbytes // 2
        ca, cb = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        kern = lambda: ops.crop_resize_flip_u8(raw.frames, raw.lengths, raw.box, S, out=dst, tables=tabs)
        copy = lambda: cb.copy_(ca)
        for _ in range(5):                                 # warm-up of both
            kern()
            copy()
        torch.cuda.synchronize()
        km, cm = [], []
        for _ in range(a.repeats):                         # alternating
            km.append(events_ms(kern, a.reps))
            cm.append(events_ms(copy, a.reps))
        k, c = statistics.median(km), statistics.median(cm)
        out['kernel']['%dx%d' % (h, w)] = {
            'crop_extents': sorted(set(int(v) for v in box[:, 2])), 'taps': int(tabs[1].shape[2]),
            'bytes_source_plus_output': nbytes, 'bytes_windows_plus_output': window,
            'kernel_ms': stats(km), 'copy_same_bytes_ms': stats(cm), 'kernel_over_copy': round(k / c, 3),
            'kernel_GBps_source_plus_output': round(nbytes / k / 1e6, 1), 'copy_GBps': round(nbytes / c / 1e6, 1)}
        print('%dx%d: kernel %.4f ms, copy of the same bytes %.4f ms' % (h, w, k, c), file=sys.stderr, flush=True)
        del raw, dst, ca, cb
        torch.cuda.empty_cache()

    if not a.no_step:
        torch.manual_seed(0)
        net = train_fine.build_model(dev, pretrained=None, input_norm=(CHARADES_MEAN, CHARADES_STD))
        net.train(True)
        optimizer = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
        reducer = cdist.GradReducer(net.parameters())
        raw, box = raw_batch(B, T, 240, 320, dev, 11)
        g = torch.Generator().manual_seed(3)
        labels = (torch.rand(B, 157, T * 10, generator=g) < 0.05).float().to(dev)
        masks = torch.ones(B, T * 10, device=dev)
        u8 = raw.transform(S)

        def leg(kind):
            def one():
                x = raw.transform(S) if kind == 'raw' else u8
                return train_fine.train_step(net, reducer, optimizer, x, labels, masks)
            for _ in range(a.warmup):
                one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                one()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3
        res = {'resident_u8': [], 'resident_raw_u8': []}
        for _ in range(a.repeats):
            res['resident_u8'].append(leg('u8'))
            res['resident_raw_u8'].append(leg('raw'))
            print('step: U8Clips %.3f ms, RawU8Clips %.3f ms' % (res['resident_u8'][-1], res['resident_raw_u8'][-1]), file=sys.stderr, flush=True)
        out['fine_train_step'] = {'source': '240x320', 'steps': a.steps, 'warmup': a.warmup,
                                  'resident_u8_ms': stats(res['resident_u8'], 3), 'resident_raw_u8_ms': stats(res['resident_raw_u8'], 3),
                                  'difference_ms': round(statistics.median(res['resident_raw_u8']) - statistics.median(res['resident_u8']), 3)}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
