#!/usr/bin/env python
"""Baseline JPEG decode on the GPU (csrc/jpegdec.hip) at the fine stream's benchmarked batch, 8 clips x 256 frames, 4:2:0, for the three
frame sizes stored in tests/golden/jpeg_bench.npz (180 x 320, 240 x 320, 360 x 480; photo-like synthetic frames, so the tool needs no
PIL on the GPU host).  Every frame of a batch is the SAME picture, replicated into distinct addresses of `data`: the lanes of a wave
then walk their bit streams in step, which real frames would not -- the JSON says so.

  1. decode        JpegClips.decode() as a whole (device events) and per kernel (torch.profiler's device times), beside a device-to-device
                   copy of the output bytes and as a multiple of it; the stored frames carry no restart markers: one decoder lane per frame
  2. bytes         host bytes staged per step: the JpegClips batch against the RawU8Clips batch it decodes to
  3. train step    train_fine.train_step fed the resident JpegClips batch (decode + crop/resize/flip + step) against the resident
                   RawU8Clips batch (crop/resize/flip + step), alternating in one process; 180 x 320 only
  4. host          (--host-only, needs PIL) PIL's Image.open().convert('RGB') per frame on one core of the machine it runs on

  5. entropy modes (--entropy sync --sub-bytes 64,128,256) legs 1 and 3 with the sync entropy mode (one workgroup per frame, one lane per
                   subsequence) beside the lane-per-interval mode, alternating in the same run: decode and per-kernel times per
                   subsequence size, the rounds decode_coefficients_sync needs for the stored frame, and the train step fed the
                   resident JpegClips batch in both modes (the sync leg at jpegdec.SYNC_SUB_BYTES) against the RawU8Clips batch

No pass bar; the JSON is the record.  One JSON document on stdout and in --out.

    python tools/jpeg_decode_bench.py --host-only --out profiles/jpeg_decode_host.json        # any machine with PIL
    python tools/jpeg_decode_bench.py --host-leg profiles/jpeg_decode_host.json --out profiles/jpeg_decode.json
    python tools/jpeg_decode_bench.py --entropy sync --sub-bytes 64,128,256 --out profiles/jpeg_decode_sync.json
"""
import argparse
import io
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

from cfn_hip import jpegdec  # noqa: E402
from cfn_hip.u8clips import RawU8Clips  # noqa: E402

SIZES = ['180x320', '240x320', '360x480']


def frames_npz():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'jpeg_bench.npz'), allow_pickle=False)
    return {k: z[k + '.jpg'].tobytes() for k in SIZES}


def replicated(jpg, B, T):
    """B clips x T frames of one encoded frame: collate one frame, then replicate its record and its segment (distinct addresses)"""
    one = jpegdec.collate_jpeg([([[jpg]], torch.tensor([[0, 0, min(jpegdec.parse(jpg)[:2]), 0]]))])
    seg = one.data.numpy()
    rows = one.frames[0].tolist()
    stride, lanes1 = seg.size, rows[jpegdec.F_LANES]
    data = np.tile(seg, B * T)
    fr = np.zeros((B * T, jpegdec.F_COLS), dtype=np.int32)
    i = np.arange(B * T)
    fr[:, jpegdec.F_CLIP], fr[:, jpegdec.F_T] = i // T, i % T
    fr[:, jpegdec.F_OFFSET], fr[:, jpegdec.F_BYTES] = i * stride, rows[jpegdec.F_BYTES]
    fr[:, jpegdec.F_RESTART], fr[:, jpegdec.F_LANE], fr[:, jpegdec.F_LANES] = rows[jpegdec.F_RESTART], i * lanes1, lanes1
    h, w = int(one.geom[0, 0, 0]), int(one.geom[0, 0, 1])
    c = min(h, w)
    box = torch.tensor([[(w - c) // 2, (h - c) // 2, c, 0]], dtype=torch.int32).repeat(B, 1).view(B, 1, 4)
    return jpegdec.JpegClips(torch.from_numpy(data), torch.from_numpy(fr), one.tables, one.geom.repeat(B, 1, 1),
                             torch.full((B, 1), T, dtype=torch.int32), box, (T, h, w, B * T * lanes1, one.dims[4]))


def nbytes(batch):
    return sum(m.numel() * m.element_size() for m in batch if torch.is_tensor(m))


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


def per_kernel_ms(fn, iters):
    """device time per launch of every jpeg_* kernel, from torch.profiler; {} when the profiler yields no device times"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            if 'jpeg_' in ev.key:
                us = getattr(ev, 'device_time_total', None)
                if us is None:
                    us = getattr(ev, 'cuda_time_total', 0.0)
                name = ev.key.split('jpeg_')[1].split('_kernel')[0]
                out[name] = round(us / max(ev.count, 1) / 1e3, 4)
        return out
    except Exception as exc:                           # the record then says why there are no stage times
        return {'unavailable': repr(exc)[:200]}


def decode_leg(jc, dev, iters):
    from cfn_hip import ops
    d = jc.to(dev)
    N, T, H, W = d.lengths.numel(), d.dims[0], d.dims[1], d.dims[2]
    out = torch.empty(N, T, H, W, 3, dtype=torch.uint8, device=dev)
    status = torch.empty(d.frames.shape[0], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.jpeg_workspace_bytes(d.frames.shape[0], N * T, d.dims[3], d.dims[4]), dtype=torch.uint8, device=dev)
    src = torch.empty_like(out)
    run = lambda: ops.jpeg_decode_u8(d, out=out, status=status, workspace=ws)
    run()
    assert not status.cpu().any(), 'the bench frames did not decode'
    raw = {'decode': [], 'copy': []}
    for _ in range(3):                                 # alternating
        raw['decode'].append(event_ms(run, iters))
        raw['copy'].append(event_ms(lambda: out.copy_(src), iters))
    ms, cp = statistics.median(raw['decode']), statistics.median(raw['copy'])
    frames = d.frames.shape[0]
    return {'frames': frames, 'decoder_lanes': d.dims[3], 'encoded_bytes': int(jc.data.numel()), 'output_bytes': out.numel(),
            'workspace_bytes': ws.numel(), 'decode_ms': round(ms, 4), 'decode_ms_min_max': [round(min(raw['decode']), 4), round(max(raw['decode']), 4)],
            'frames_per_s': round(frames / ms * 1e3), 'copy_of_output_ms': round(cp, 4), 'multiple_of_copy': round(ms / cp, 1),
            'kernel_ms': per_kernel_ms(run, 3)}


def modes_leg(jc, jpg, dev, iters, subs, max_subs=None):
    """leg 1 for the lane-per-interval mode and the sync mode at every size of `subs`, alternating; the outputs are compared byte for byte"""
    from cfn_hip import ops
    d = jc.to(dev)
    N, T, H, W = d.lengths.numel(), d.dims[0], d.dims[1], d.dims[2]
    out = torch.empty(N, T, H, W, 3, dtype=torch.uint8, device=dev)
    status = torch.empty(d.frames.shape[0], dtype=torch.int32, device=dev)
    ws = torch.empty(ops.jpeg_workspace_bytes(d.frames.shape[0], N * T, d.dims[3], d.dims[4]), dtype=torch.uint8, device=dev)
    runs = {'interval': lambda: ops.jpeg_decode_u8(d, out=out, status=status, workspace=ws)}
    for sb in subs:
        runs['sync_%d' % sb] = (lambda sb=sb: ops.jpeg_decode_u8(d, out=out, status=status, workspace=ws, entropy='sync', sub_bytes=sb, max_subs=max_subs))
    want = None
    for name, run in runs.items():
        out.fill_(0xA5)
        run()
        assert not status.cpu().any(), 'the bench frames did not decode (%s)' % name
        want = out.clone() if want is None else want
        assert torch.equal(out, want), 'the %s mode decodes other bytes than the interval mode' % name
    del want
    raw = {k: [] for k in runs}
    for _ in range(3):                                 # alternating: every repeat visits every mode
        for name, run in runs.items():
            raw[name].append(event_ms(run, iters))
    res = {'frames': d.frames.shape[0], 'encoded_bytes_per_frame_segment': int(d.frames[0, jpegdec.F_BYTES]),
           'max_subs': max_subs or jpegdec.SYNC_DEFAULT_MAX_SUBS, 'modes': {}}
    for name, run in runs.items():
        ms = statistics.median(raw[name])
        m = {'decode_ms': round(ms, 4), 'decode_ms_min_max': [round(min(raw[name]), 4), round(max(raw[name]), 4)], 'kernel_ms': per_kernel_ms(run, 3)}
        if name != 'interval':
            st = {}
            jpegdec.decode_coefficients_sync(jpg, int(name.split('_')[1]), stats=st)
            m['subsequences'], m['rounds'] = st['subsequences'], st['rounds']
            m['taken_by_sync'] = st['subsequences'] <= (max_subs or jpegdec.SYNC_DEFAULT_MAX_SUBS)          # otherwise: one lane per frame, as 'interval'
        res['modes'][name] = m
    return res


def train_leg(jc, dev, a):
    import torch.optim as optim
    import train_fine
    from cfn_hip import dist as cdist
    torch.manual_seed(0)
    net = train_fine.build_model(dev, pretrained=None, input_norm=(train_fine.CHARADES_MEAN, train_fine.CHARADES_STD))
    net.train(True)
    optimizer = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    reducer = cdist.GradReducer(net.parameters())
    B, T = jc.lengths.shape[0], jc.dims[0]
    g = torch.Generator().manual_seed(1)
    labels = (torch.rand(B, 157, T * 10, generator=g) < 0.05).float().to(dev)
    masks = torch.ones(B, T * 10, device=dev)
    dj = jc.to(dev)
    legs = {'resident_jpeg': dj, 'resident_raw_u8': dj.decode()}
    modes = {'resident_jpeg': 'interval', 'resident_raw_u8': None}
    if a.entropy == 'sync':
        legs = {'resident_jpeg': dj, 'resident_jpeg_sync': dj, 'resident_raw_u8': legs['resident_raw_u8']}
        modes['resident_jpeg_sync'] = 'sync'
    torch.cuda.synchronize()

    def timed(batch, mode):
        t0 = None
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            x = train_fine.flatten_clips(batch, dev, 224, jpeg_entropy=mode)          # a JpegClips batch: decode (+ one status read-back), then as RawU8Clips
            train_fine.train_step(net, reducer, optimizer, x, labels, masks)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3
    raw = {k: [] for k in legs}
    for _ in range(a.repeats):                         # alternating: every repeat visits both legs
        for name, batch in legs.items():
            raw[name].append(timed(batch, modes[name]))
            print('%s: %.3f ms/step' % (name, raw[name][-1]), file=sys.stderr, flush=True)
    return {k: {'ms_per_step': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)} for k, v in raw.items()}


def host_leg(frames, repeats):
    from PIL import Image, features
    import PIL
    out = {'machine': platform.node() or platform.machine(), 'arch': platform.machine(), 'cpus': os.cpu_count(),
           'pillow': PIL.__version__, 'libjpeg': str(features.version('jpg')), 'one_core': True, 'ms_per_frame': {}}
    for k, jpg in frames.items():
        secs = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(50):
                np.asarray(Image.open(io.BytesIO(jpg)).convert('RGB'))
            secs.append((time.perf_counter() - t0) / 50)
        out['ms_per_frame'][k] = round(statistics.median(secs) * 1e3, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=8)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--host-only', action='store_true', help="PIL's decode time alone (needs PIL, no GPU)")
    ap.add_argument('--host-leg', default=None, help='a JSON written with --host-only, embedded as measured on that machine')
    ap.add_argument('--entropy', default='interval', choices=('interval', 'sync'), help='sync: leg 5, both entropy modes side by side')
    ap.add_argument('--sub-bytes', default='64,128,256', help='the subsequence sizes of the sync legs')
    ap.add_argument('--max-subs', type=int, default=None, help='most subsequences of a frame in the sync legs (default: the library\'s)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    frames = frames_npz()
    if a.host_only:
        out = {'pil_decode': host_leg(frames, 5)}
    else:
        assert torch.cuda.is_available(), 'the decode and train-step legs measure the HIP path: they need a GPU'
        import cfn_hip
        dev = torch.device('cuda:0')
        out = {'clips': a.clips, 'frames_per_clip': a.frames, 'sampling': '4:2:0', 'restart_interval': 0,
               'content': 'all frames of a batch have EQUAL content (one stored frame replicated into distinct addresses): the lanes of a wave '
                          'decode in step, which distinct frames would not',
               'device': cfn_hip.device_info(), 'sizes': {}}
        for k in SIZES:
            jc = replicated(frames[k], a.clips, a.frames)
            if a.entropy == 'sync':
                res = {'encoded_bytes_per_frame': len(frames[k]), 'decode': modes_leg(jc, frames[k], dev, a.iters, [int(v) for v in a.sub_bytes.split(',')], a.max_subs)}
                if k == SIZES[0] and not a.no_step:
                    res['train_step'] = train_leg(jc, dev, a)
                    res['train_step_sync_sub_bytes'] = jpegdec.SYNC_SUB_BYTES
                out['sizes'][k] = res
                print('%s done' % k, file=sys.stderr, flush=True)
                del jc
                torch.cuda.empty_cache()
                continue
            res = {'encoded_bytes_per_frame': len(frames[k]), 'decode': decode_leg(jc, dev, a.iters)}
            raw_bytes = a.clips * a.frames * jc.dims[1] * jc.dims[2] * 3 + a.clips * 4 + a.clips * 16
            res['host_bytes_per_step'] = {'jpeg_clips': nbytes(jc), 'raw_u8_clips': raw_bytes, 'ratio': round(raw_bytes / nbytes(jc), 1)}
            if k == SIZES[0] and not a.no_step:
                res['train_step'] = train_leg(jc, dev, a)
            out['sizes'][k] = res
            print('%s done' % k, file=sys.stderr, flush=True)
            del jc
            torch.cuda.empty_cache()
        if a.host_leg and os.path.exists(a.host_leg):
            with open(a.host_leg) as fh:
                out['pil_decode'] = json.load(fh)['pil_decode']
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(txt + '\n')


if __name__ == '__main__':
    main()
