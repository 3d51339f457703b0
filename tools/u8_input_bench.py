#!/usr/bin/env python
"""uint8 video input against the fp32 input path, fine stream, same process, legs alternating (default 8 x 256 x 224 x 224):

  1. resident fp32    the normalised clip lives in HBM (what bench.py times)
  2. resident uint8   the frames live in HBM as bytes, conv1_s normalises them while it loads them
  3. staged fp32      a loader COLLATES every step (collate.fine_collate of per-video fp32 samples) -> HostStager -> step
  4. staged uint8     the same with collate.fine_collate_u8 of per-video uint8 samples

(The A/B against convert + the fp32 kernels that made the fused forward and weight gradient the default: "routes" in profiles/u8_input.json.)

Per leg: ms/step (median over the repeats, with min / max), host bytes per step; collate seconds per batch for the staged legs; the
stem family's device time per step (cfn_prof_enable(6)) beside its algorithmic bytes for the resident legs.  One JSON document on
stdout and in --out.

    python tools/u8_input_bench.py --out u8_input.json
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

import cfn_hip  # noqa: E402
import collate  # noqa: E402
import train_fine  # noqa: E402
from cfn_hip import dist as cdist  # noqa: E402
from cfn_hip import ops, staging  # noqa: E402
from cfn_hip.u8clips import U8Clips, CHARADES_MEAN, CHARADES_STD  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--crop', type=int, default=224)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--resident-only', action='store_true', help='skip the staged legs')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures the HIP path; it needs a GPU'
    dev = torch.device('cuda:0')
    B, T, S = a.batch, a.frames, a.crop
    torch.manual_seed(0)
    net = train_fine.build_model(dev, pretrained=None, input_norm=(CHARADES_MEAN, CHARADES_STD))
    net.train(True)
    optimizer = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    reducer = cdist.GradReducer(net.parameters())

    # per-video host samples, as a Dataset would return them: uint8 (1, T, H, W, 3) and the reference's normalised fp32 (1, 3, T, H, W)
    g = torch.Generator().manual_seed(1234)
    tl = T * 10
    vids_u8, vids_f32 = [], []
    for i in range(B):
        f = torch.randint(0, 256, (1, T, S, S, 3), generator=g, dtype=torch.uint8)
        label = (torch.rand(157, tl, generator=g) < 0.05).float()
        vids_u8.append((f, label, 'v%d' % i))
        x = ops.clip_u8_to_f32(f.to(dev), net.input_lut).cpu()              # (the conversion itself is not what is timed here)
        vids_f32.append((x, label, 'v%d' % i))
    collators = {'f32': (collate.fine_collate, vids_f32), 'u8': (collate.fine_collate_u8, vids_u8)}

    def flat(batch):
        x, labels, masks, _ = batch
        return train_fine.flatten_clips(x, dev), labels.to(dev), masks.to(dev)
    resident = {k: flat(fn(v)) for k, (fn, v) in collators.items()}

    def step(inp):
        return train_fine.train_step(net, reducer, optimizer, *inp)

    def timed_resident(kind):
        for _ in range(a.warmup):
            step(resident[kind])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step(resident[kind])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, 0, 0.0

    stagers = {k: staging.HostStager(dev) for k in collators}

    def timed_staged(kind):
        fn, vids = collators[kind]
        secs = []

        def loader():
            for _ in range(a.warmup + a.steps):
                c0 = time.perf_counter()
                batch = fn(vids)
                secs.append(time.perf_counter() - c0)
                yield batch
        st = stagers[kind]
        b0, n0 = st.bytes_staged, st.batches
        t0 = None
        for i, batch in enumerate(st.stage(loader())):
            if i == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            step(flat(batch))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps * 1e3
        return dt, (st.bytes_staged - b0) // max(st.batches - n0, 1), statistics.median(secs)

    legs = [('resident_f32', timed_resident, 'f32'), ('resident_u8', timed_resident, 'u8'),
            ('staged_f32', timed_staged, 'f32'), ('staged_u8', timed_staged, 'u8')]
    if a.resident_only:
        legs = legs[:2]
    raw = {name: [] for name, _, _ in legs}
    for _ in range(a.repeats):                     # alternating: every repeat visits every leg
        for name, fn, kind in legs:
            raw[name].append(fn(kind))
            print('%s: %.3f ms/step' % (name, raw[name][-1][0]), file=sys.stderr, flush=True)

    def stem_profile(kind):
        cfn_hip.prof_enable('stem', True)
        cfn_hip.prof_collect('stem')
        for _ in range(3):
            step(resident[kind])
        torch.cuda.synchronize()
        cfn_hip.prof_enable('stem', False)
        ms, n, by = cfn_hip.prof_collect('stem')
        return {'ms_per_step': round(ms / 3, 4), 'launches_per_step': n // 3, 'algorithmic_GB_per_step': round(by / 3 / 1e9, 4)}

    out = {'shape': [B, T, S, S], 'steps': a.steps, 'warmup': a.warmup, 'repeats': a.repeats,
           'device': cfn_hip.device_info(), 'legs': {}}
    for name, _, _ in legs:
        ms = [r[0] for r in raw[name]]
        out['legs'][name] = {'ms_per_step': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3),
                             'host_bytes_per_step': int(raw[name][-1][1]), 'collate_s_per_batch': round(raw[name][-1][2], 4)}
    out['stem_family'] = {'f32': stem_profile('f32'), 'u8': stem_profile('u8')}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
