"""GPU: crop + antialiased bilinear resize + flip of uint8 frames (csrc/aug_u8.hip) against the bytes the reference's PIL transforms
produced (tests/golden/aug_u8*.npz) and against the integer emulation cfn_hip.u8aug.resize_u8_reference; the batch type, the models,
the training scripts fed by a DataLoader of untransformed frames, the long-video chunking and the feature extractor.

Bounds.  The operator is integer arithmetic: every comparison of its bytes is torch.equal.  A net fed the transformed bytes runs the
same stem kernel on the same bytes as one fed the host-transformed U8Clips: its eval-mode forward is compared with torch.equal too;
training steps and whole-script runs use the bounds tests/test_hip_u8_input.py uses for two input routes (LOGIT_TOL, GRAD_TOL)."""
import os

import numpy as np
import pytest
import torch

from conftest import t
from test_u8_aug_cpu import golden_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]
LOGIT_TOL, GRAD_TOL = 1e-3, 5e-2                       # tests/test_hip_u8_input.py


def _torch_op(frames, lengths, box, S):
    import cfn_hip.torchlib  # noqa: F401
    from cfn_hip import ops
    bounds, coef = ops.aug_tables(box, S, frames.device)
    return torch.ops.cfn.crop_resize_flip_u8(frames, lengths, box.to(frames.device), bounds, coef, S)


def test_kernel_reproduces_every_golden_case():
    """the reference's own transform outputs, bit for bit, through the C ABI (ops) and through torch.ops.cfn; the one fixture whose
    crop is more than 4x the output (140 pixels into 32) is refused by both, as the ABI says"""
    from cfn_hip import ops
    refused = 0
    for name, src, box, S, want in golden_cases():
        frames, b = t(src).unsqueeze(0).to(DEV), t(box).view(1, 4)
        if int(box[2]) > 4 * S:
            with pytest.raises(RuntimeError):
                ops.crop_resize_flip_u8(frames, None, b, S)
            refused += 1
            continue
        got = ops.crop_resize_flip_u8(frames, None, b, S)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + want.shape
        assert torch.equal(got[0].cpu(), t(want)), name
        assert torch.equal(_torch_op(frames, None, b, S), got), name
    assert refused == 1
    import cfn_hip.torchlib  # noqa: F401
    with pytest.raises(RuntimeError):                      # 11 taps: the operator has no other route
        z = torch.zeros
        torch.ops.cfn.crop_resize_flip_u8(z(1, 1, 150, 150, 3, dtype=torch.uint8, device=DEV), None, torch.tensor([[0, 0, 140, 0]], dtype=torch.int32, device=DEV),
                                          z(1, 32, 2, dtype=torch.int32, device=DEV), z(1, 32, 11, dtype=torch.int32, device=DEV), 32)


def _sweep_batch(S, variant, T=3):
    """three clips in one Hs x Ws buffer with odd Ws: an upscale, an identity (c == S) and a reduction (> 3x where that stays small),
    so the batch mixes table widths; x1 = 3 * variant + (0, 1, 2): x1 * 3 mod 4 takes all four residues over the two variants.
    Everything outside a clip's crop window is 255: a read outside the window shows."""
    cs = {30: (19, 30, 100), 32: (21, 32, 120), 160: (100, 160, 250), 224: (157, 224, 300), 312: (200, 312, 400)}[S]
    x1 = [3 * variant + i for i in range(3)]
    y1 = [2, 0, 5]
    flip = [0, 1, 0] if variant == 0 else [1, 0, 1]
    Hs, Ws = max(cs) + 9, (max(cs) + 11) | 1
    assert Ws % 2 == 1
    g = torch.Generator().manual_seed(S * 10 + variant)
    frames = torch.full((3, T, Hs, Ws, 3), 255, dtype=torch.uint8)
    for n in range(3):
        frames[n, :, y1[n]:y1[n] + cs[n], x1[n]:x1[n] + cs[n]] = torch.randint(0, 256, (T, cs[n], cs[n], 3), generator=g, dtype=torch.uint8)
    box = torch.tensor([[x1[n], y1[n], cs[n], flip[n]] for n in range(3)], dtype=torch.int32)
    lengths = [0, T, 1] if variant == 0 else None
    return frames, box, lengths


@pytest.mark.parametrize('variant', [0, 1])
@pytest.mark.parametrize('S', [30, 32, 160, 224, 312])
def test_sweep_equals_integer_emulation(S, variant):
    from cfn_hip import ops, u8aug
    frames, box, lengths = _sweep_batch(S, variant)
    assert len({u8aug.table_width(int(c), S) for c in box[:, 2]}) >= 2             # K differs within the batch
    assert {(int(x) * 3) % 4 for v in (0, 1) for x in _sweep_batch(S, v, 1)[1][:, 0]} == {0, 1, 2, 3}      # every alignment of a row's first byte
    want = u8aug.resize_u8_reference(frames, box, S, lengths)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    got = ops.crop_resize_flip_u8(frames.to(DEV), ln, box.to(DEV), S)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(_torch_op(frames.to(DEV), ln, box, S), got)
    # c == S: the cropped source itself (mirrored when flipped)
    x1, y1, c, flip = (int(v) for v in box[1])
    src = frames[1, :, y1:y1 + c, x1:x1 + c]
    live = 3 if lengths is None else lengths[1]
    assert c == S and torch.equal(got[1, :live].cpu(), (src.flip(2) if flip else src)[:live])
    if lengths is not None:                                # padding frames are zero bytes
        for n, k in enumerate(lengths):
            assert not bool(got[n, k:].any())


def test_unaligned_buffers_and_out_argument():
    """src and dst at odd byte offsets inside larger buffers (heads and tails of the 16-byte units on both sides); `out=` receives the
    result in place, allocates nothing, and the bytes around it stay as they were"""
    from cfn_hip import ops, u8aug
    T = 2
    ln = torch.tensor([2, 1, 2], dtype=torch.int32, device=DEV)
    # S = 30: rows of 90 bytes, the byte-wise vertical pass; S = 32: the dword-wise one, which needs dst on a dword boundary (do = 4) and
    # falls back otherwise (do = 5, 3)
    for S, so, do in ((30, 1, 5), (30, 7, 3), (30, 16, 0), (32, 1, 4), (32, 7, 5), (32, 3, 3)):
        frames, box, _ = _sweep_batch(S, 1, T)
        want = u8aug.resize_u8_reference(frames, box, S, [2, 1, 2])
        nsrc, ndst = frames.numel(), want.numel()
        sbuf = torch.full((nsrc + 64,), 255, dtype=torch.uint8, device=DEV)
        sbuf[so:so + nsrc] = frames.to(DEV).view(-1)
        dbuf = torch.full((ndst + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        out = dbuf[do:do + ndst].view(want.shape)
        dbox = box.to(DEV)
        tabs = ops.aug_tables(box, S, DEV)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()['allocation.all.allocated']       # allocations made so far (a count: frees do not move it)
        res = ops.crop_resize_flip_u8(sbuf[so:so + nsrc].view(frames.shape), ln, dbox, S, out=out, tables=tabs)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == before      # nothing allocated on the device
        assert res is out and torch.equal(out.cpu(), want)
        assert bool((dbuf[:do] == 0xA5).all()) and bool((dbuf[do + ndst:] == 0xA5).all())
    with pytest.raises(RuntimeError):
        ops.crop_resize_flip_u8(frames.to(DEV), ln, box, S, out=torch.empty(3, T, S, S + 1, 3, dtype=torch.uint8, device=DEV))


@pytest.mark.capture
def test_capture_in_one_stream_and_replay_on_new_data():
    from cfn_hip import ops, u8aug
    S, T = 32, 2
    frames, box, _ = _sweep_batch(S, 0, T)
    frames2, box2, _ = _sweep_batch(S, 1, T)
    assert torch.equal(box[:, 2], box2[:, 2])               # the same crop extents: the same tables
    src, dbox = frames.to(DEV), box.to(DEV)
    ln = torch.tensor([2, 1, 2], dtype=torch.int32, device=DEV)
    tabs = ops.aug_tables(box, S, DEV)
    out = torch.zeros(3, T, S, S, 3, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.crop_resize_flip_u8(src, ln, dbox, S, out=out, tables=tabs)        # warm-up outside the capture
    side.synchronize()
    assert torch.equal(out.cpu(), u8aug.resize_u8_reference(frames, box, S, [2, 1, 2]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.crop_resize_flip_u8(src, ln, dbox, S, out=out, tables=tabs)
    src.copy_(frames2.to(DEV))
    dbox.copy_(box2.to(DEV))
    ln.copy_(torch.tensor([1, 2, 0], dtype=torch.int32, device=DEV))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.crop_resize_flip_u8(src, ln, dbox, S, tables=tabs)
    assert torch.equal(out, eager) and torch.equal(out.cpu(), u8aug.resize_u8_reference(frames2, box2, S, [1, 2, 0]))


def _raw_batch(seed, sizes, T, train=True):
    """RawU8Clips (N, T, Hmax, Wmax, 3) of clips with the given (h, w), boxes drawn as the reference draws them, and the list of lengths"""
    import random
    from cfn_hip import u8aug
    from cfn_hip.u8clips import RawU8Clips
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = max(s[0] for s in sizes), max(s[1] for s in sizes)
    frames = torch.zeros(len(sizes), T, Hs, Ws, 3, dtype=torch.uint8)
    boxes = []
    for n, (h, w) in enumerate(sizes):
        frames[n, :, :h, :w] = torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8)
        boxes.append(u8aug.train_crop_params(rng, (h, w), [0.875, 0.7], 224) if train else u8aug.center_crop_params((h, w)))
    lengths = [T - (n % 2) * 2 for n in range(len(sizes))]
    return RawU8Clips(frames, torch.tensor(lengths, dtype=torch.int32), torch.tensor(boxes, dtype=torch.int32))


def _host_transform(raw, S):
    from cfn_hip import u8aug
    from cfn_hip.u8clips import U8Clips
    fl = raw.flatten_crops()
    y = u8aug.resize_u8_reference(fl.frames, fl.box, S, fl.lengths.tolist())
    return U8Clips(y.view(tuple(raw.frames.shape[:-4]) + tuple(y.shape[1:])), raw.lengths)


def test_raw_u8_clips_transform_and_x3d_fine_forward():
    """RawU8Clips.transform on the GPU = the host emulation's U8Clips, and x3d_fine's forward on either is the same bits"""
    import x3d_fine
    from cfn_hip.u8clips import RawU8Clips, U8Clips
    raw = _raw_batch(5, [(120, 160), (135, 101)], 4)
    want = _host_transform(raw, 224)
    got = raw.to(DEV).transform(224)
    assert isinstance(got, U8Clips) and got.frames.is_cuda and torch.equal(got.frames.cpu(), want.frames) and torch.equal(got.lengths.cpu(), want.lengths)
    nested = RawU8Clips(raw.frames.unsqueeze(1), raw.lengths.unsqueeze(1), raw.box.unsqueeze(1)).cuda().transform(224)      # (B, n, ...) as collated
    assert tuple(nested.frames.shape) == (2, 1, 4, 224, 224, 3) and torch.equal(nested.flatten_crops().frames, got.frames)
    torch.manual_seed(0)
    net = x3d_fine.generate_model('M', n_classes=157, n_input_channels=3, task='loc', dropout=0.0, base_bn_splits=1)
    net.set_input_norm(MEAN, STD).to(DEV).eval()
    with torch.no_grad():
        a = net([got, None])
        b = net([want.to(DEV), None])
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


class _RawVideos(torch.utils.data.Dataset):
    """ragged uint8 videos of differing frame sizes, as decoded, with the crop box the reference's training transform would draw; or
    (host=True) the same videos already cropped / resized / flipped on the CPU by the integer emulation"""
    SIZES = [(120, 160), (135, 180), (144, 108), (120, 160)]

    def __init__(self, n, seed, host, S=224, coarse=False, train=True):
        self.n, self.seed, self.host, self.S, self.coarse, self.train = n, seed, host, S, coarse, train

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        import random
        from cfn_hip import u8aug
        r = np.random.RandomState(self.seed + i)
        T = 8 - 2 * (i % 2)
        h, w = self.SIZES[i % len(self.SIZES)]
        frames = torch.from_numpy(r.randint(0, 256, size=(1, T, h, w, 3)).astype(np.uint8))
        label = (r.rand(157, T * 10) < 0.05).astype(np.float32)
        box = u8aug.train_crop_params(random.Random(self.seed + i), (h, w), [0.875, 0.7], self.S) if self.train else u8aug.center_crop_params((h, w))
        box = torch.tensor([box], dtype=torch.int32)
        clip = u8aug.resize_u8_reference(frames, box, self.S) if self.host else (frames, box)
        if not self.coarse:
            return clip, label, 'vid%d' % i
        import train_coarse_fineFEAT as tc
        tf = 20 + 4 * (i % 3)
        feat = {k: np.abs(r.randn(c, tf, 7, 7)).astype(np.float32) for k, c in tc.FEAT_DEPTH.items()}
        return clip, label, feat, np.array([2 * (i % 3), T, tf, 1], dtype=np.int64), 'vid%d' % i, 30.0 + i


def test_raw_dataloader_feeds_train_fine(tmp_path, monkeypatch):
    """Dataset of untransformed videos -> DataLoader(collate.fine_collate_raw_u8, pin_memory=True) -> staging -> train_fine.run, one step,
    against the same videos transformed on the host and collated by fine_collate_u8: loss, probabilities and the step's parameter
    update (= the gradients) within the bounds of the two input routes"""
    import torch.utils.data as tud
    import collate
    import train_fine
    from cfn_hip import staging
    from cfn_hip.u8clips import RawU8Clips, U8Clips

    def go(rawmode):
        ds = _RawVideos(2, 0, host=not rawmode)
        mk = lambda: tud.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, pin_memory=True,
                                    collate_fn=collate.fine_collate_raw_u8 if rawmode else collate.fine_collate_u8)
        seen, kinds, stagers = [], [], []
        real_step, real_flat, real_stager = train_fine.train_step, train_fine.flatten_clips, staging.HostStager

        def step(net, reducer, optimizer, inputs, *a, **k):
            assert isinstance(inputs, U8Clips) and inputs.frames.is_cuda and tuple(inputs.frames.shape[2:]) == (224, 224, 3)
            out = real_step(net, reducer, optimizer, inputs, *a, **k)
            seen.append((float(out[0]), float(out[1]), out[2].detach().clone()))
            return out

        def flat(inputs, *a, **k):
            kinds.append((type(inputs), inputs.frames.is_cuda))
            return real_flat(inputs, *a, **k)

        def stager(*a, **k):
            st = real_stager(*a, **k)
            stagers.append(st)
            return st
        with monkeypatch.context() as mp:
            mp.setattr(train_fine, 'train_step', step)
            mp.setattr(train_fine, 'flatten_clips', flat)
            mp.setattr(staging, 'HostStager', stager)
            torch.manual_seed(0)
            init = {k: v.detach().clone() for k, v in train_fine.build_model(DEV, pretrained=None, input_norm=(MEAN, STD)).named_parameters()}
            torch.manual_seed(0)
            net = train_fine.run(batch_size=2, dataloaders={'train': mk(), 'val': mk()}, max_steps=1, pretrained=None, log=lambda *_: None,
                                 save_model=str(tmp_path / 'f_'), input_norm=(MEAN, STD))
        assert len(stagers) == 1 and stagers[0].batches >= 1
        assert kinds[0] == (RawU8Clips if rawmode else U8Clips, True)                # the staged batch arrives on the device as the type it left as
        return seen, {k: v.detach() - init[k] for k, v in net.named_parameters()}
    s_host, d_host = go(False)
    s_raw, d_raw = go(True)
    assert len(s_host) == len(s_raw) == 1
    (c0, l0, p0), (c1, l1, p1) = s_host[0], s_raw[0]
    print('fine run: host-transformed cls %.6f loc %.6f | GPU-transformed cls %.6f loc %.6f' % (c0, l0, c1, l1))
    assert abs(c0 - c1) <= LOGIT_TOL * abs(c0) and abs(l0 - l1) <= LOGIT_TOL * abs(l0)
    assert float((p0 - p1).abs().max()) <= LOGIT_TOL * float(p0.abs().max())
    worst = max(float((d_host[k] - d_raw[k]).norm() / (d_host[k].norm() + 1e-30)) for k in d_host)
    print('fine run: worst parameter-update norm-rel difference %.2e' % worst)
    assert worst <= GRAD_TOL


def test_forward_video_chunks_raw_clips():
    """the coarse net's long-video chunking on untransformed frames: every chunk is transformed when its turn comes; logits equal those of
    the host-transformed U8Clips chunked the same way"""
    import train_coarse_fineFEAT as tc
    from oracle import spec
    net = tc.build_model(DEV, pretrained=None, dropout=0.0, input_norm=(MEAN, STD))
    spec.fill_module_(net)
    net.eval()
    Tv, Tf, lim = 40, 24, 16
    raw = _raw_batch(9, [(126, 168)], Tv, train=False)
    raw = type(raw)(raw.frames, torch.tensor([36], dtype=torch.int32), raw.box)       # the last 4 frames are padding
    host = _host_transform(raw, 224)
    g = torch.Generator().manual_seed(5)
    feat = {k: torch.relu(torch.randn(1, c, Tf, 7, 7, generator=g)).to(DEV) for k, c in tc.FEAT_DEPTH.items()}
    fm = torch.ones(1, Tf, device=DEV)
    meta = torch.tensor([[2, Tv, 60, 1]], dtype=torch.int64, device=DEV)
    pieces = [raw.to(DEV).time_slice(s, min(s + lim, Tv)).transform(224) for s in range(0, Tv, lim)]
    assert [int(p.lengths[0]) for p in pieces] == [16, 16, 4] and torch.equal(torch.cat([p.frames for p in pieces], 1).cpu(), host.frames)
    with torch.no_grad():
        got = tc.forward_video(net, raw.to(DEV), feat, fm, 0, meta, t_lim=lim)
        want = tc.forward_video(net, host.to(DEV), feat, fm, 0, meta, t_lim=lim)
        whole = tc.forward_video(net, raw.to(DEV), feat, fm, 0, meta)             # < 1005 frames: one piece
        whole_u8 = tc.forward_video(net, host.to(DEV), feat, fm, 0, meta)
    assert got.shape == want.shape and whole.shape == whole_u8.shape
    assert float((got - want).abs().max() / want.abs().max()) <= LOGIT_TOL
    assert float((whole - whole_u8).abs().max() / whole_u8.abs().max()) <= LOGIT_TOL
    assert int(meta[0, 0]) == 2


def test_extract_fine_features_from_raw_clips(tmp_path):
    import extract_fineFEAT as ex
    torch.manual_seed(0)
    net = ex.build_tower(DEV, ckpt=None, input_norm=(MEAN, STD))
    raw = _raw_batch(11, [(130, 174)], 8, train=False)
    raw = type(raw)(raw.frames, torch.tensor([8], dtype=torch.int32), raw.box)
    host = _host_transform(raw, 224)
    assert ex.extract(net, [('vidA', raw)], str(tmp_path / 'raw')) == 1
    assert ex.extract(net, [('vidA', host)], str(tmp_path / 'u8')) == 1
    for k, c in (('layer1', 24), ('layer2', 48), ('layer3', 96), ('layer4', 192), ('conv5', 432)):
        f = torch.load(os.path.join(str(tmp_path / 'raw'), k, 'vidA'))
        f8 = torch.load(os.path.join(str(tmp_path / 'u8'), k, 'vidA'))
        assert f.shape == (1, c, 8, 7, 7) and f.dtype == torch.float32
        assert float((f - f8).abs().max()) <= LOGIT_TOL * float(f8.abs().max())
