#!/usr/bin/env python
"""Packed 16-bit fine features against the fp32 dict path, coarse stream (default B = 6 and 8 at T' = 128, 64-frame clips):

  1. kernels       ops.feat_unpack of the batch and ops.feat_pack of one video (device events), each beside a device-to-device copy of the
                   SAME OUTPUT BYTES and as a multiple of it; achieved bytes/s from the algorithmic bytes (2 B in + 4 B out per element)
  2. host collate  collate.coarse_collate of per-video fp32 dict samples against collate.coarse_collate_packed of the same videos' records
                   (memory-mapped, page cache warm), seconds per batch; the clips of this leg are cut to 8 x 8 pixels, so that it times
                   the features (and labels), which is what differs.  --host-only runs this leg alone, on any CPU: the JSON labels it
                   with the machine it ran on -- a CPU without a GPU is the build machine, not the training host
  3. train step    a loader COLLATES every step -> HostStager -> train_coarse_fineFEAT.train_step, fp32 dict against packed, the two legs
                   alternating in one process; ms/step (median over the repeats, min / max), host bytes staged per step

No pass bar: the fp32 dict path is the comparison, the JSON is the record.  One JSON document on stdout and in --out.

    python tools/feat_pack_bench.py --out profiles/feat_pack.json
"""
import argparse
import json
import os
import platform
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))

import torch  # noqa: E402

import collate  # noqa: E402
from cfn_hip import featpack  # noqa: E402

DEPTH = {'layer1': 24, 'layer2': 48, 'layer3': 96, 'layer4': 192, 'conv5': 432}


def make_videos(n, tf, clip_frames, crop, dt, tmp):
    """per-video samples as a Dataset would return them: fp32 dict features and the record of the same (rounded) features"""
    g = torch.Generator().manual_seed(1234)
    plain, packed = [], []
    for i in range(n):
        feat = {k: torch.relu(torch.randn(c, tf, 7, 7, generator=g)) for k, c in DEPTH.items()}
        payload, frames, channels = featpack.pack_reference(feat, dt)
        rec = featpack.open_record(featpack.write_record(featpack.record_path(tmp, 'v%d' % i), payload, dt, frames, channels))
        clip = torch.randn(1, 3, clip_frames, crop, crop, generator=g)
        label = (torch.rand(157, clip_frames * 10, generator=g) < 0.05).float()
        meta = torch.tensor([0, clip_frames, tf, 1])
        plain.append((clip, label, rec.to_dict(), meta, 'v%d' % i, 30.0))
        packed.append((clip, label, rec, meta, 'v%d' % i, 30.0))
    return plain, packed


def feature_bytes(batch):
    f = batch[3]
    if isinstance(f, featpack.PackedFeats):
        return f.data.numel() * 2 + f.offsets.numel() * 8 + f.lengths.numel() * 4
    return sum(v.numel() * 4 for v in f.values())


def host_collate(plain, packed, repeats):
    legs = {'coarse_collate': (collate.coarse_collate, plain), 'coarse_collate_packed': (collate.coarse_collate_packed, packed)}
    secs = {k: [] for k in legs}
    by = {}
    for _ in range(repeats + 1):                       # alternating; the first visit warms the page cache and the allocator
        for name, (fn, smp) in legs.items():
            t0 = time.perf_counter()
            batch = fn(smp)
            secs[name].append(time.perf_counter() - t0)
            by[name] = feature_bytes(batch)
    return {name: {'s_per_batch': round(statistics.median(v[1:]), 5), 'min': round(min(v[1:]), 5), 'max': round(max(v[1:]), 5),
                   'feature_bytes_per_batch': by[name]} for name, v in secs.items()}


def event_ms(fn, iters, warmup=3):
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


def kernels(packed, dt, dev, iters):
    from cfn_hip import ops
    pf = collate.coarse_collate_packed(packed)[3].to(dev)
    out = [torch.empty(pf.batch, c, pf.t_max, 7, 7, device=dev) for c in pf.channels]
    n_out = sum(o.numel() for o in out)
    src32, dst32 = torch.empty(n_out, device=dev), torch.empty(n_out, device=dev)
    maps = [o[0].contiguous() for o in ops.feat_unpack(pf.data, pf.offsets, pf.lengths, pf.channels, pf.t_max)]
    n_pack = sum(m.numel() for m in maps)
    payload = torch.empty(n_pack, dtype=dt, device=dev)
    src16, dst16 = torch.empty(n_pack, dtype=dt, device=dev), torch.empty(n_pack, dtype=dt, device=dev)
    res = {}
    raw = {k: [] for k in ('unpack', 'copy_unpack_out', 'pack', 'copy_pack_out')}
    for _ in range(3):                                 # alternating
        raw['unpack'].append(event_ms(lambda: ops.feat_unpack(pf.data, pf.offsets, pf.lengths, pf.channels, pf.t_max, out=out), iters))
        raw['copy_unpack_out'].append(event_ms(lambda: dst32.copy_(src32), iters))
        raw['pack'].append(event_ms(lambda: ops.feat_pack(maps, dt, out=payload), iters))
        raw['copy_pack_out'].append(event_ms(lambda: dst16.copy_(src16), iters))
    med = {k: statistics.median(v) for k, v in raw.items()}
    res['unpack'] = {'ms': round(med['unpack'], 5), 'output_bytes': n_out * 4, 'algorithmic_bytes': int(pf.data.numel()) * 2 + n_out * 4,
                     'GB_per_s': round((int(pf.data.numel()) * 2 + n_out * 4) / med['unpack'] / 1e6, 1),
                     'copy_of_output_ms': round(med['copy_unpack_out'], 5), 'multiple_of_copy': round(med['unpack'] / med['copy_unpack_out'], 3)}
    res['pack_one_video'] = {'ms': round(med['pack'], 5), 'output_bytes': n_pack * 2, 'algorithmic_bytes': n_pack * 6,
                             'GB_per_s': round(n_pack * 6 / med['pack'] / 1e6, 1),
                             'copy_of_output_ms': round(med['copy_pack_out'], 5), 'multiple_of_copy': round(med['pack'] / med['copy_pack_out'], 3)}
    return res


def train_steps(plain, packed, dev, a):
    import torch.optim as optim
    import train_coarse_fineFEAT as tc
    from cfn_hip import dist as cdist
    from cfn_hip import staging
    from train_fine import flatten_clips
    torch.manual_seed(0)
    net = tc.build_model(dev, pretrained=None)
    net.train(True)
    optimizer = optim.SGD(tc.param_groups(net, 0.01), lr=0.01, momentum=0.9, weight_decay=1e-5)
    reducer = cdist.GradReducer(net.parameters())
    legs = {'staged_f32_dict': (collate.coarse_collate, plain), 'staged_packed': (collate.coarse_collate_packed, packed)}
    stagers = {k: staging.HostStager(dev) for k in legs}

    def timed(name):
        fn, smp = legs[name]
        secs = []

        def loader():
            for _ in range(a.warmup + a.steps):
                c0 = time.perf_counter()
                batch = fn(smp)
                secs.append(time.perf_counter() - c0)
                yield batch
        st = stagers[name]
        b0, n0 = st.bytes_staged, st.batches
        t0 = None
        for i, (x, labels, masks, feat, fm, meta, _names, _dur) in enumerate(st.stage(loader())):
            if i == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            tc.train_step(net, reducer, optimizer, flatten_clips(x, dev, tc.CROP), labels, masks, tc.unpack_feat(feat, dev), fm, meta, i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3, (st.bytes_staged - b0) // max(st.batches - n0, 1), statistics.median(secs)
    raw = {k: [] for k in legs}
    for _ in range(a.repeats):                         # alternating: every repeat visits both legs
        for name in legs:
            raw[name].append(timed(name))
            print('%s: %.3f ms/step' % (name, raw[name][-1][0]), file=sys.stderr, flush=True)
    out = {}
    for name, v in raw.items():
        ms = [r[0] for r in v]
        out[name] = {'ms_per_step': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3),
                     'host_bytes_per_step': int(v[-1][1]), 'collate_s_per_batch': round(v[-1][2], 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='6,8')
    ap.add_argument('--feat-frames', type=int, default=128)
    ap.add_argument('--clip-frames', type=int, default=64)
    ap.add_argument('--crop', type=int, default=224)
    ap.add_argument('--dtype', default='fp16', choices=['fp16', 'bf16'])
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernel-iters', type=int, default=200)
    ap.add_argument('--host-only', action='store_true', help='the host-collate leg alone (runs without a GPU)')
    ap.add_argument('--no-step', action='store_true', help='skip the train-step leg')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dt = featpack.feat_dtype(a.dtype)
    gpu = torch.cuda.is_available()
    if not a.host_only:
        assert gpu, 'the kernel and train-step legs measure the HIP path: they need a GPU (--host-only: the collate leg alone)'
    out = {'feat_frames': a.feat_frames, 'clip_frames': a.clip_frames, 'dtype': a.dtype, 'steps': a.steps, 'warmup': a.warmup, 'repeats': a.repeats,
           'host': {'machine': platform.machine(), 'cpus': os.cpu_count(), 'torch_threads': torch.get_num_threads(),
                    'kind': 'GPU host' if gpu else 'build machine (no GPU): host-collate times only, not the training host'},
           'batches': {}}
    if gpu and not a.host_only:
        import cfn_hip
        out['device'] = cfn_hip.device_info()
    with tempfile.TemporaryDirectory() as tmp:
        for B in [int(v) for v in a.batches.split(',')]:
            plain, packed = make_videos(B, a.feat_frames, a.clip_frames, a.crop if not a.host_only else 8, dt, os.path.join(tmp, 'b%d' % B))
            small = lambda smp: [(s[0][..., :8, :8].contiguous(),) + s[1:] for s in smp]      # 8 x 8 clips: the leg times features + labels, not the video
            res = {'host_collate': host_collate(small(plain), small(packed), max(a.repeats, 5))}
            if not a.host_only:
                dev = torch.device('cuda:0')
                res['kernels'] = kernels(packed, dt, dev, a.kernel_iters)
                if not a.no_step:
                    res['train_step'] = train_steps(plain, packed, dev, a)
            out['batches'][str(B)] = res
            print('B = %d done' % B, file=sys.stderr, flush=True)
            del plain, packed
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
