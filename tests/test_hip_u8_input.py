"""GPU: uint8 video frames normalised inside the stem conv (csrc/stem_u8.hip) -- the converter and the fused stem kernels against the
table gather and the fp32 kernels, the models, the long-video chunking, the training scripts fed by a DataLoader of uint8 batches,
the feature extractor and the graphed step.

Bounds.  Exact (torch.equal) wherever the uint8 path only re-stages the same fp32 values: the converter, and the fused forward, which
builds the same LDS image as the fp32 kernel and leaves its MFMA loop alone.  Whole nets: the bounds the suite uses for the SAME input
run twice (test_hip_train.test_run_to_run_reproducibility: logits 1e-3 of max |logit|, per-parameter gradient norm 5e-2) -- the two
paths differ in the order of fp64 commits only, which is what those bounds allow for.  Weight gradient of the stem: the fp32 kernel's
own error against an fp64 reference is the yardstick (at most 2x)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, t

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]
LOGIT_TOL, GRAD_TOL = 1e-3, 5e-2                       # test_run_to_run_reproducibility

# (N, T, H, W, lengths, the fused forward takes it): the three X3D crops (S 160, M 224, XL 312: a 936-byte row pitch), W % 4 != 0 with an
# odd plane, a plane that is a multiple of 4 but not of 16 pixels, odd H; lengths ragged, including 0 and T; 16 x 312: bands of 8 output
# rows, whose image fits the 64 KiB of LDS without the table (the fp32 kernel takes it) and not with it
SHAPES = [(3, 3, 224, 224, [3, 0, 1], True), (2, 3, 160, 160, [2, 3], True), (2, 2, 312, 312, [2, 1], True), (3, 3, 30, 35, [0, 3, 2], False),
          (2, 4, 6, 10, [4, 1], False), (2, 2, 33, 36, [1, 2], False), (1, 2, 224, 224, None, True), (1, 2, 16, 312, None, False)]
# (the ids pytest gives (N, T, H, W, lengths) rows)
SHAPE_IDS = ['%d-%d-%d-%d-%s' % (s[:4] + ('None' if s[4] is None else 'lengths%d' % i,)) for i, s in enumerate(SHAPES)]


def _lut():
    from cfn_hip import ops
    return ops.clip_lut(MEAN, STD)


def _frames(seed, N, T, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, T, H, W, 3), generator=g, dtype=torch.uint8)


def _cpu_clip(frames, lengths, lut):
    from cfn_hip.u8clips import U8Clips
    N, T = frames.shape[:2]
    ln = torch.full((N,), T, dtype=torch.int32) if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    return U8Clips(frames, ln).to_f32(lut)


def _len(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)


def test_clip_u8_to_f32_golden_fixture():
    """the reference's own ToTensor + Normalize + stack + permute output, reproduced bit for bit on the GPU"""
    from cfn_hip import ops
    z = load_golden('clip_u8')
    lut = ops.clip_lut([float(v) for v in z['mean']], [float(v) for v in z['std']], int(z['norm_value']))
    x = ops.clip_u8_to_f32(t(z['frames']).unsqueeze(0).to(DEV), lut.to(DEV))
    assert torch.equal(x[0].cpu(), t(z['clip']))
    import cfn_hip.torchlib  # noqa: F401
    x2 = torch.ops.cfn.clip_u8_to_f32(t(z['frames']).unsqueeze(0).to(DEV), lut.to(DEV))
    assert torch.equal(x2, x)


@pytest.mark.parametrize('N,T,H,W,lengths', [s[:5] for s in SHAPES], ids=SHAPE_IDS)
def test_clip_u8_to_f32_equals_cpu_gather(N, T, H, W, lengths):
    from cfn_hip import ops
    lut = _lut()
    frames = _frames(H + W, N, T, H, W)
    want = _cpu_clip(frames, lengths, lut)
    got = ops.clip_u8_to_f32(frames.to(DEV), lut.to(DEV), _len(lengths))
    assert got.shape == (N, 3, T, H, W) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want)
    if lengths is not None:
        for n, ln in enumerate(lengths):
            assert bool((got[n, :, ln:] == 0).all()) and bool((got[n, :, :ln] != 0).all())


@pytest.mark.parametrize('N,T,H,W,lengths,fused', SHAPES, ids=SHAPE_IDS)
def test_stem_conv_u8_forward_is_bit_identical(N, T, H, W, lengths, fused):
    """fused (W % 4 == 0, even H, image and table within 64 KiB of LDS) and fallback routes: the same bits as the fp32 stem conv of the converted clip; padded frames give
    exact zeros"""
    from cfn_hip import ops
    lut = _lut().to(DEV)
    frames = _frames(7 + H, N, T, H, W).to(DEV)
    w = (torch.randn(24, 3, 1, 3, 3, generator=torch.Generator().manual_seed(1)) * 0.2).to(DEV)
    ln = _len(lengths)
    want = ops.stem_conv(ops.clip_u8_to_f32(frames, lut, ln), w)
    got = ops.stem_conv_u8(frames, ln, lut, w)
    assert got.shape == want.shape and torch.equal(got, want)
    import cfn_hip.torchlib  # noqa: F401
    assert torch.equal(torch.ops.cfn.stem_conv_u8(frames, ln, lut, w), want)
    if lengths is not None:
        for n, k in enumerate(lengths):
            assert bool((got[n, :, k:] == 0).all())
    from cfn_hip import call_try
    y = torch.empty_like(want)
    took = call_try('cfn_stem_conv_u8_fwd', frames, lut, ln, w.reshape(24, 27).contiguous(), y, N, 3, 24, T, H, W)
    assert took == fused            # a shape the fused kernel does not take is REPORTED (and nothing is launched)
    assert ops.conv3d_dense_route(5, N, 3, 24, T, H, W).startswith('convert') == (not fused)
    if took:
        assert torch.equal(y, want)


@pytest.mark.parametrize('N,T,H,W,lengths', [(2, 3, 224, 224, [3, 1]), (2, 2, 224, 224, None), (2, 3, 160, 160, [2, 3]), (3, 3, 30, 35, [0, 3, 2]),
                                             (2, 2, 312, 312, [2, 1])])
def test_stem_conv_u8_weight_gradient(N, T, H, W, lengths):
    """against the fp64 conv3d weight gradient of the converted clip (CPU): the uint8 path's error is at most 2x the fp32 path's on the
    same input (224 x 224: the LDS-staged kernel's body on the uint8 source; other shapes: convert + the fp32 entry point)"""
    from cfn_hip import ops
    lut = _lut()
    frames = _frames(11 + H, N, T, H, W)
    g = torch.Generator().manual_seed(2)
    w = torch.randn(24, 3, 1, 3, 3, generator=g) * 0.2
    x = _cpu_clip(frames, lengths, lut)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, 24, T, Ho, Wo, generator=g)
    ref = torch.nn.grad.conv3d_weight(x.double(), w.shape, gy.double(), stride=(1, 2, 2), padding=(0, 1, 1))

    def grad_of(fn):
        wd = w.to(DEV).requires_grad_(True)
        fn(wd).backward(gy.to(DEV))
        return wd.grad.detach().cpu().double()
    ln = _len(lengths)
    g32 = grad_of(lambda wd: ops.stem_conv(x.to(DEV), wd))
    gu8 = grad_of(lambda wd: ops.stem_conv_u8(frames.to(DEV), ln, lut.to(DEV), wd))
    scale = float(ref.abs().max())
    e32, eu8 = float((g32 - ref).abs().max()) / scale, float((gu8 - ref).abs().max()) / scale
    print('stem wgrad %dx%d: fp32 path rel err %.3e, uint8 path rel err %.3e' % (H, W, e32, eu8))
    assert eu8 <= 2 * e32, (eu8, e32)
    from cfn_hip import call_try
    g64 = torch.zeros(24, 27, dtype=torch.float64, device=DEV)
    took = call_try('cfn_stem_conv_u8_bwd_weight', gy.to(DEV), frames.to(DEV), lut.to(DEV), ln, g64, N, 3, 24, T, H, W)
    assert took == (H == 224 and W == 224)
    assert ops.conv3d_dense_route(6, N, 3, 24, T, H, W).startswith('convert') == (not took)
    import cfn_hip.torchlib  # noqa: F401
    gop = torch.ops.cfn.stem_conv_u8_backward(gy.to(DEV), frames.to(DEV), ln, lut.to(DEV), w.to(DEV)).cpu().double()
    assert float((gop - ref).abs().max()) / scale <= 2 * e32


def test_stem_u8_weight_gradient_equals_fp32_bits_deterministic():
    """deterministic mode, 224 x 224: cfn_stem_conv_u8_bwd_weight and cfn_stem_conv_bwd_weight on the converted clip fill the fp64 tile with
    the same bits.  Both run one kernel body over the same partition of items over workgroups (one plan); a padded frame adds gy * 0.0 in the
    fp32 source's run and is not multiplied in the uint8 source's, and the accumulators start at +0, so neither can produce a -0."""
    import cfn_hip
    from cfn_hip import call, call_try, ops
    N, T, H, W, lengths = 2, 3, 224, 224, [3, 1]
    lut = _lut().to(DEV)
    frames = _frames(11 + H, N, T, H, W).to(DEV)
    ln = _len(lengths)
    gy = torch.randn(N, 24, T, H // 2, W // 2, generator=torch.Generator().manual_seed(2)).to(DEV)
    x = ops.clip_u8_to_f32(frames, lut, ln)
    prev = cfn_hip.deterministic(True)
    try:
        g8 = torch.zeros(24, 27, dtype=torch.float64, device=DEV)
        g32 = torch.zeros(24, 27, dtype=torch.float64, device=DEV)
        assert call_try('cfn_stem_conv_u8_bwd_weight', gy, frames, lut, ln, g8, N, 3, 24, T, H, W)
        call('cfn_stem_conv_bwd_weight', gy, x, g32, N, 3, 24, T, H, W)
        torch.cuda.synchronize()
    finally:
        cfn_hip.deterministic(prev)
    assert bool((g32 != 0).all())
    print('stem wgrad, deterministic: max |u8 - fp32| = %.3e' % float((g8 - g32).abs().max()))
    assert torch.equal(g8.view(torch.int64), g32.view(torch.int64))


def _compare_nets(run_f32, run_u8, net):
    """eval and train, forward and all gradients, uint8 frames against the converted fp32 clip"""
    for train in (False, True):
        net.train(train)
        res = []
        for run in (run_f32, run_u8):
            state = [b.clone() for b in net.buffers()]
            net.zero_grad(set_to_none=True)
            out = run()
            (out * out).mean().backward()
            res.append((out.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}))
            for b, s in zip(net.buffers(), state):
                b.copy_(s)
        (o1, g1), (o2, g2) = res
        assert o1.shape == o2.shape and g1.keys() == g2.keys() and 'conv1_s.weight' in g1
        d_out = float((o1 - o2).abs().max() / o1.abs().max())
        worst = max(float((g1[k] - g2[k]).norm() / (g1[k].norm() + 1e-30)) for k in g1)
        print('%s train=%s: logits rel %.2e, worst gradient norm-rel %.2e' % (type(net).__module__, train, d_out, worst))
        assert d_out <= LOGIT_TOL and worst <= GRAD_TOL, (train, d_out, worst)


def test_x3d_fine_u8_equals_converted_clip():
    import x3d_fine
    from cfn_hip import ops
    from cfn_hip.u8clips import U8Clips
    torch.manual_seed(0)
    net = x3d_fine.generate_model('M', n_classes=157, n_input_channels=3, task='loc', dropout=0.0, base_bn_splits=1)
    net.set_input_norm(MEAN, STD).to(DEV)
    assert net.input_lut.is_cuda                        # the table follows .to()
    frames = _frames(21, 2, 8, 224, 224).to(DEV)
    ln = torch.tensor([8, 6], dtype=torch.int32, device=DEV)
    x = ops.clip_u8_to_f32(frames, net.input_lut, ln)
    _compare_nets(lambda: net([x, None]), lambda: net([U8Clips(frames, ln), None]), net)
    bare = x3d_fine.generate_model('M', n_classes=157, task='loc', base_bn_splits=1).to(DEV)
    with pytest.raises(RuntimeError, match='set_input_norm'):
        bare([U8Clips(frames, ln), None])


def _coarse_batch(T, Tf=12, seed=0):
    import train_coarse_fineFEAT as tc
    x, l, m, feat, fm, meta, _, _ = next(iter(tc.SyntheticCoarse(2, 1, frames=T, fine_len=Tf, seed=seed)))
    return l.to(DEV), m.to(DEV), {k: v.to(DEV) for k, v in feat.items()}, fm.to(DEV), meta.to(DEV)


def test_x3d_coarse_u8_equals_converted_clip():
    import train_coarse_fineFEAT as tc
    from cfn_hip import ops
    from cfn_hip.u8clips import U8Clips
    torch.manual_seed(0)
    net = tc.build_model(DEV, pretrained=None, dropout=0.0, input_norm=(MEAN, STD))
    net.rw6.dropout.p = 0.0
    _, _, feat, fm, meta = _coarse_batch(8)
    frames = _frames(22, 2, 8, 224, 224).to(DEV)
    ln = torch.tensor([6, 8], dtype=torch.int32, device=DEV)
    x = ops.clip_u8_to_f32(frames, net.input_lut, ln)
    _compare_nets(lambda: net([x, feat, fm, 0, meta]), lambda: net([U8Clips(frames, ln), feat, fm, 0, meta]), net)


def test_forward_video_chunks_u8_clips():
    """long-video chunking (train_coarse_fineFEAT.py:215-224) on uint8 frames: the chunks are time slices with clamped lengths, and the
    logits equal those of the converted fp32 clip chunked the same way; the slices together are the unchunked call's frames"""
    import train_coarse_fineFEAT as tc
    from cfn_hip import ops
    from cfn_hip.u8clips import U8Clips
    from oracle import spec
    net = tc.build_model(DEV, pretrained=None, dropout=0.0, input_norm=(MEAN, STD))
    spec.fill_module_(net)
    net.eval()
    Tv, Tf, lim = 40, 24, 16
    frames = _frames(23, 1, Tv, 224, 224).to(DEV)
    ln = torch.tensor([36], dtype=torch.int32, device=DEV)           # the last 4 frames are padding: the last chunk holds 4 of 8
    u = U8Clips(frames, ln)
    g = torch.Generator().manual_seed(5)
    feat = {k: torch.relu(torch.randn(1, c, Tf, 7, 7, generator=g)).to(DEV) for k, c in tc.FEAT_DEPTH.items()}
    fm = torch.ones(1, Tf, device=DEV)
    meta = torch.tensor([[2, Tv, 60, 1]], dtype=torch.int64, device=DEV)
    x = ops.clip_u8_to_f32(frames, net.input_lut, ln)
    pieces = [u.time_slice(s, min(s + lim, Tv)) for s in range(0, Tv, lim)]
    assert [int(p.lengths[0]) for p in pieces] == [16, 16, 4] and torch.equal(torch.cat([p.frames for p in pieces], 1), frames)
    assert torch.equal(torch.cat([ops.clip_u8_to_f32(p.frames, net.input_lut, p.lengths) for p in pieces], 2), x)
    with torch.no_grad():
        got = tc.forward_video(net, u, feat, fm, 0, meta, t_lim=lim)
        want = tc.forward_video(net, x, feat, fm, 0, meta, t_lim=lim)
        whole = tc.forward_video(net, u, feat, fm, 0, meta)           # < 1005 frames: one piece
        whole32 = net([x, feat, fm, 0, meta])
    assert got.shape == want.shape and whole.shape == whole32.shape
    assert float((got - want).abs().max() / want.abs().max()) <= LOGIT_TOL
    assert float((whole - whole32).abs().max() / whole32.abs().max()) <= LOGIT_TOL
    assert int(meta[0, 0]) == 2


class _U8Videos(torch.utils.data.Dataset):
    """ragged uint8 videos shaped like charades_fine's samples before ToTensor / Normalize: (clips (1,T,H,W,3) uint8, label, vid)"""

    def __init__(self, n, seed, crop, normalise=None, coarse=False):
        self.n, self.seed, self.crop, self.normalise, self.coarse = n, seed, crop, normalise, coarse

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        from cfn_hip.u8clips import U8Clips
        r = np.random.RandomState(self.seed + i)
        T = 8 - 2 * (i % 2)                                      # ragged clips: 8, 6, 8, 6 frames
        clip = r.randint(0, 256, size=(1, T, self.crop, self.crop, 3)).astype(np.uint8)
        label = (r.rand(157, T * 10) < 0.05).astype(np.float32)
        if self.normalise is not None:                          # what the reference's loader does on the CPU
            clip = U8Clips(torch.from_numpy(clip), torch.tensor([T], dtype=torch.int32)).to_f32(self.normalise)
        if not self.coarse:
            return clip, label, 'vid%d' % i
        import train_coarse_fineFEAT as tc
        tf = 20 + 4 * (i % 3)
        feat = {k: np.abs(r.randn(c, tf, 7, 7)).astype(np.float32) for k, c in tc.FEAT_DEPTH.items()}
        return clip, label, feat, np.array([2 * (i % 3), T, tf, 1], dtype=np.int64), 'vid%d' % i, 30.0 + i


def _align(nbytes, a=256):
    return (nbytes + a - 1) // a * a


def _spy(monkeypatch, mod, seen, stagers):
    """record (phase, cls_loss, loc_loss) of every batch run() feeds to train_step / detection_loss, and the HostStager it builds"""
    from cfn_hip import staging
    real_step, real_loss, real_stager = mod.train_step, mod.detection_loss, staging.HostStager

    def step(*a, **k):
        out = real_step(*a, **k)
        seen.append(('train', float(out[0]), float(out[1])))
        return out

    def loss(*a, **k):
        out = real_loss(*a, **k)
        if not torch.is_grad_enabled():                  # the validation branch of run() (train_step calls it with grad enabled)
            seen.append(('val', float(out[0]), float(out[1])))
        return out

    def stager(*a, **k):
        st = real_stager(*a, **k)
        stagers.append(st)
        return st
    monkeypatch.setattr(mod, 'train_step', step)
    monkeypatch.setattr(mod, 'detection_loss', loss)
    monkeypatch.setattr(staging, 'HostStager', stager)


def test_u8_dataloader_feeds_train_fine(tmp_path, monkeypatch):
    """Dataset of ragged uint8 videos -> DataLoader(collate.fine_collate_u8, pin_memory=True) -> train_fine.run, two steps: the losses
    equal the fp32-loader run on the same frames, and what travels to the GPU per batch is the uint8 byte count"""
    import torch.utils.data as tud
    import collate
    import train_fine
    lut = _lut()
    crop, B, Tmax = 64, 2, 8

    def go(u8):
        ds = _U8Videos(6, 0, crop, None if u8 else lut)
        mk = lambda: tud.DataLoader(ds, batch_size=B, shuffle=False, num_workers=0, pin_memory=True,
                                    collate_fn=collate.fine_collate_u8 if u8 else collate.fine_collate)
        seen, stagers = [], []
        with monkeypatch.context() as mp:
            _spy(mp, train_fine, seen, stagers)
            torch.manual_seed(0)
            net = train_fine.run(batch_size=B, dataloaders={'train': mk(), 'val': mk()}, max_steps=2, pretrained=None, log=lambda *_: None,
                                 save_model=str(tmp_path / 'f_'), input_norm=(MEAN, STD) if u8 else None)
        assert len(stagers) == 1
        return net, seen, stagers[0]
    net32, s32, st32 = go(False)
    net8, s8, st8 = go(True)
    assert [s[0] for s in s8] == ['train', 'train'] == [s[0] for s in s32]
    for i, (a, b) in enumerate(zip(s32, s8)):
        print('fine run step %d: fp32 loader cls %.6f loc %.6f | uint8 loader cls %.6f loc %.6f' % (i + 1, a[1], a[2], b[1], b[2]))
        assert abs(a[1] - b[1]) <= LOGIT_TOL * abs(a[1]) and abs(a[2] - b[2]) <= LOGIT_TOL * abs(a[2])
    assert all(bool(torch.isfinite(p).all()) for p in net8.parameters())
    # bytes per batch from shapes (every tensor of a batch starts on a 256-byte boundary of the slab): frames at ONE byte per element
    rest = _align(B * 157 * Tmax * 10 * 4) + _align(B * Tmax * 10 * 4)
    per_u8 = _align(B * 1 * Tmax * crop * crop * 3) + _align(B * 1 * 4) + rest
    per_f32 = _align(B * 1 * 3 * Tmax * crop * crop * 4) + rest
    assert st8.batches >= 2 and st8.bytes_staged == st8.batches * per_u8
    assert st32.bytes_staged == st32.batches * per_f32


def test_u8_dataloader_feeds_train_coarse(tmp_path, monkeypatch):
    """the same through train_coarse_fineFEAT.run (coarse_collate_u8), two steps and one validation video"""
    import torch.utils.data as tud
    import collate
    import train_coarse_fineFEAT as tc
    lut = _lut()

    def go(u8):
        col = collate.coarse_collate_u8 if u8 else collate.coarse_collate
        norm = None if u8 else lut
        loaders = {'train': tud.DataLoader(_U8Videos(4, 0, 224, norm, coarse=True), batch_size=2, shuffle=False, num_workers=0, pin_memory=True, collate_fn=col),
                   'val': tud.DataLoader(_U8Videos(1, 100, 224, norm, coarse=True), batch_size=1, shuffle=False, num_workers=0, pin_memory=True, collate_fn=col)}
        seen, logs = [], []
        tag = 'u8' if u8 else 'f32'
        with monkeypatch.context() as mp:
            _spy(mp, tc, seen, [])
            torch.manual_seed(0)
            net = tc.run(max_epochs=2, batch_size=2, dataloaders=loaders, pretrained=None, save_model=str(tmp_path / ('m_' + tag)),
                         csv_path=str(tmp_path / (tag + '.csv')), log=logs.append, input_norm=(MEAN, STD) if u8 else None)
        return net, seen, logs
    net32, s32, _ = go(False)
    net8, s8, logs = go(True)
    assert [s[0] for s in s8] == [s[0] for s in s32] and [s[0] for s in s8].count('val') == 1 and [s[0] for s in s8].count('train') == 4
    for i, (a, b) in enumerate(zip(s32[:2], s8[:2])):        # the first two optimisation steps (later ones compound the weights' run-to-run differences)
        print('coarse run step %d: fp32 loader cls %.6f loc %.6f | uint8 loader cls %.6f loc %.6f' % (i + 1, a[1], a[2], b[1], b[2]))
        assert abs(a[1] - b[1]) <= LOGIT_TOL * abs(a[1]) and abs(a[2] - b[2]) <= LOGIT_TOL * abs(a[2])
    assert all(bool(torch.isfinite(p).all()) for p in net8.parameters())
    assert any('val Loc Loss' in l for l in logs) and all('nan' not in l.lower() for l in logs), logs
    assert os.path.getsize(str(tmp_path / 'u8.csv')) > 0


def test_extract_fine_features_from_u8(tmp_path):
    import extract_fineFEAT as ex
    from cfn_hip import ops
    from cfn_hip.u8clips import U8Clips
    torch.manual_seed(0)
    net = ex.build_tower(DEV, ckpt=None, input_norm=(MEAN, STD))
    frames = _frames(31, 1, 8, 224, 224)
    u = U8Clips(frames, torch.tensor([8], dtype=torch.int32))
    x = u.to_f32(_lut())
    assert ex.extract(net, [('vidA', u)], str(tmp_path / 'u8')) == 1
    assert ex.extract(net, [('vidA', x)], str(tmp_path / 'f32')) == 1
    for k, c in (('layer1', 24), ('layer2', 48), ('layer3', 96), ('layer4', 192), ('conv5', 432)):
        f = torch.load(os.path.join(str(tmp_path / 'u8'), k, 'vidA'))
        f32 = torch.load(os.path.join(str(tmp_path / 'f32'), k, 'vidA'))
        assert f.shape == (1, c, 8, 7, 7) and f.dtype == torch.float32 and bool((f >= 0).all())
        assert float((f - f32).abs().max()) <= LOGIT_TOL * float(f32.abs().max())


@pytest.mark.capture
def test_graphed_step_takes_u8_clips():
    """hipGraph capture of the train step with a U8Clips argument (cfn_hip/graph.py copies both members into the graph's static
    inputs): replayed steps equal eager steps from the same start (the bounds of test_graphed_step_equals_eager_step)"""
    import copy
    import torch.optim as optim
    import train_fine
    from cfn_hip import dist as cdist
    from cfn_hip.graph import GraphedStep
    from cfn_hip.u8clips import U8Clips
    torch.manual_seed(0)
    net = train_fine.build_model(DEV, pretrained=None, dropout=0.0, input_norm=(MEAN, STD))
    batches = []
    for i, (_, l, m, _) in enumerate(train_fine.SyntheticCharades(2, 3, frames=8, crop=64)):
        u = U8Clips(_frames(40 + i, 2, 8, 64, 64).to(DEV), torch.tensor([8, 8 - 2 * i], dtype=torch.int32, device=DEV))
        batches.append((u, l.to(DEV), m.to(DEV)))
    mk = lambda n, o: (lambda x, l, m: train_fine.train_step(n, cdist.GradReducer(n.parameters()), o, x, l, m)[:2])
    net.train(True)
    net2 = copy.deepcopy(net)
    o1 = optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    o2 = optim.SGD(net2.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
    eager, graphed = mk(net, o1), GraphedStep(mk(net2, o2), optimizer=o2)     # call 1 eager, call 2 captures, call 3 replays
    for b in batches:
        le = [float(v) for v in eager(*b)]
        lg = [float(v) for v in graphed(*b)]
        assert all(abs(a - c) <= 1e-5 * max(abs(a), 1.0) for a, c in zip(le, lg)), (le, lg)
    assert len(graphed._graphs) == 1                   # one capture serves every batch of the same shapes: lengths are data
    for (n1, p1), (_, p2) in zip(net.state_dict().items(), net2.state_dict().items()):
        d = float((p1.double() - p2.double()).abs().max())
        assert d <= 3e-5 * (float(p1.double().abs().max()) + 1e-3), (n1, d)
