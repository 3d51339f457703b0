"""GPU: baseline JPEG frames decoded by csrc/jpegdec.hip against the pixels PIL decoded (tests/golden/jpeg_u8.npz).

Bounds.  The decoder is integer arithmetic from the bit stream to the RGB bytes, and cfn_hip.jpegdec.decode_reference, the same arithmetic
in numpy, reproduces PIL's pixels with 0 differing bytes on every fixture (tests/test_jpeg_cpu.py).  Every comparison here is therefore
torch.equal.  A net fed the decoded batch reads the same bytes as one fed the RawU8Clips batch built from PIL's pixels: with the library's
deterministic mode on, the losses of a training step are compared with == as well."""
import copy

import numpy as np
import pytest
import torch

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]


def _one(name):
    from cfn_hip import jpegdec
    return jpegdec.collate_jpeg([([[jc.jpg(name)]], torch.tensor([jc.full_box(name)]))])


@pytest.fixture(scope='module')
def mixed():
    """(the JpegClips batch on the host, the RawU8Clips batch collate.fine_collate_raw_u8 builds from PIL's pixels)"""
    import collate
    labels = [torch.zeros(157, 4), torch.zeros(157, 6)]
    jb = collate.fine_collate_jpeg([(s, lb, 'v%d' % i) for i, (s, lb) in enumerate(zip(jc.jpeg_samples(jc.MIXED, jc.MIXED_BOX), labels))])
    rb = collate.fine_collate_raw_u8([(s, lb, 'v%d' % i) for i, (s, lb) in enumerate(zip(jc.raw_samples(jc.MIXED, jc.MIXED_BOX), labels))])
    return jb[0], rb[0]


def test_every_fixture_alone():
    """one launch sequence per fixture: all sizes, contents, sampling types, table kinds, restart intervals and the gray image"""
    from cfn_hip import jpegdec
    bad = []
    for name in jc.names():
        clips = _one(name).to(DEV)
        status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
        raw = clips.decode(status=status)
        want = torch.from_numpy(np.array(jc.pixels(name)))
        assert tuple(raw.frames.shape) == (1, 1, 1) + tuple(want.shape) and raw.frames.dtype == torch.uint8
        diff = int((raw.frames[0, 0, 0].cpu() != want).sum())
        if diff or int(status[0]):
            bad.append((name, diff, int(status[0])))
    assert not bad, bad
    assert jpegdec.STATUS_OUT_OF_DATA == 2


def test_mixed_batch_equals_collated_pixels(mixed):
    from cfn_hip import jpegdec
    from cfn_hip.u8clips import RawU8Clips
    clips, want = mixed
    assert len(set(clips.frames[:, jpegdec.F_SET].tolist())) >= 3 and int(clips.frames[:, jpegdec.F_LANES].max()) > 1
    dclips = clips.to(DEV)
    status = torch.full((clips.frames.shape[0],), -1, dtype=torch.int32, device=DEV)
    got = dclips.decode(status=status)
    assert isinstance(got, RawU8Clips) and got.frames.is_cuda
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b)
    assert not status.cpu().any()
    # a preallocated, dirty output buffer: every byte is written
    out = torch.full(tuple(want.frames.shape), 0xA5, dtype=torch.uint8, device=DEV)
    again = dclips.decode(out=out, status=status)
    assert again.frames.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), want.frames) and not status.cpu().any()
    # two runs are bit-identical
    assert torch.equal(dclips.decode().frames, got.frames)
    with pytest.raises(RuntimeError):
        dclips.decode(out=torch.empty(tuple(want.frames.shape[:-1]) + (4,), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        dclips.decode(status=torch.zeros(1, dtype=torch.int32, device=DEV))


def test_ragged_batch():
    """3, 0, 2 and 1 frames per clip, each clip its own size, a gray clip, a clip with restart intervals: the pictures in the top-left
    corners, zero bytes everywhere else"""
    from cfn_hip import jpegdec
    clips = jpegdec.collate_jpeg(jc.jpeg_samples(jc.RAGGED, jc.RAGGED_BOX)).to(DEV)
    status = torch.empty(clips.frames.shape[0], dtype=torch.int32, device=DEV)
    got = clips.decode(status=status)
    assert torch.equal(got.frames.cpu(), jc.padded(jc.RAGGED)) and not status.cpu().any()
    assert got.lengths.cpu().tolist() == [[3, 0], [2, 1]] and got.box.cpu().tolist() == jc.RAGGED_BOX
    jpegdec.check_status(status, clips.frames.cpu(), ['a', 'b'], crops=2)


def test_cut_segment_sets_only_its_status(mixed):
    """a frame whose segment is cut in half reports it in its own status word; every other frame of the batch stays exact.  Row 1 has no
    restart interval (it runs out of data), the last row has (its later intervals lose their markers)"""
    from cfn_hip import jpegdec
    clips, want = mixed
    rows = clips.frames.shape[0]
    for row in (1, rows - 1):
        fr = clips.frames.clone()
        fr[row, jpegdec.F_BYTES] //= 2
        cut = clips._replace(frames=fr).to(DEV)
        status = torch.empty(rows, dtype=torch.int32, device=DEV)
        got = cut.decode(status=status).frames.cpu()
        st = status.cpu().tolist()
        assert st[row] != 0 and not any(s for i, s in enumerate(st) if i != row), st
        clip, t = int(fr[row, jpegdec.F_CLIP]), int(fr[row, jpegdec.F_T])
        keep = torch.ones(got.shape[:3], dtype=torch.bool)
        keep[clip // 2, clip % 2, t] = False
        assert torch.equal(got[keep], want.frames[keep])
        with pytest.raises(RuntimeError, match='v%d' % (clip // 2)):
            jpegdec.check_status(status, fr, ['v0', 'v1'], crops=2)
    # records that disagree with the batch are refused by the kernels, not followed
    fr = clips.frames.clone()
    fr[0, jpegdec.F_OFFSET] = clips.data.numel()
    fr[2, jpegdec.F_SET] = 99
    fr[3, jpegdec.F_LANE] = 10 ** 6
    status = torch.empty(rows, dtype=torch.int32, device=DEV)
    clips._replace(frames=fr).to(DEV).decode(status=status)
    st = status.cpu().tolist()
    assert [bool(s & jpegdec.STATUS_BAD_ROW) for s in st] == [i in (0, 2, 3) for i in range(rows)], st


def test_native_operator_equals_ctypes(mixed):
    from cfn_hip import ops, torchlib  # noqa: F401
    clips, want = mixed
    d = clips.to(DEV)
    frames, status = torch.ops.cfn.jpeg_decode_u8(d.data, d.frames, d.tables, d.geom, d.lengths, list(d.dims))
    assert torch.equal(frames, ops.jpeg_decode_u8(d)) and not status.cpu().any()
    assert torch.equal(frames.view(tuple(want.frames.shape)).cpu(), want.frames)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.jpeg_decode_u8(d.data, d.frames[:, :6], d.tables, d.geom, d.lengths, list(d.dims))
    with pytest.raises(RuntimeError):
        ops.jpeg_decode_u8(clips)                      # host tensors


def test_flatten_clips_decodes(mixed):
    import train_fine
    clips, want = mixed
    for crop in (None, 32):
        a = train_fine.flatten_clips(clips, torch.device(DEV), crop, names=['v0', 'v1'])
        b = train_fine.flatten_clips(want, torch.device(DEV), crop)
        assert type(a) is type(b) and a.frames.is_cuda
        for x, y in zip(a, b):
            assert tuple(x.shape) == tuple(y.shape) and torch.equal(x, y)
    fr = clips.frames.clone()
    fr[0, 3] //= 2
    with pytest.raises(RuntimeError, match='v0'):
        train_fine.flatten_clips(clips._replace(frames=fr), torch.device(DEV), 32, names=['v0', 'v1'])


def test_train_step_loss_bits():
    """one train_fine.train_step fed the decoded JpegClips batch returns the loss bits of the same step fed the RawU8Clips batch of PIL's
    pixels (8 frames, crop 64: the smallest the model tests use)"""
    import cfn_hip
    import collate
    import torch.optim as optim
    import train_fine
    from cfn_hip import dist as cdist
    a = ['48x64_smooth_420q75', '48x64_smooth_420q95', '48x64_smooth_420q50opt', '48x64_smooth_420q10', '48x64_smooth_420q100',
         '48x64_smooth_420q75rst3', '48x64_noise_420q100', '48x64_smooth_420q75']
    b = ['37x50_smooth_420q75', '37x50_smooth_420q95', '37x50_noise_420q100', '37x50_smooth_420q75rst3', '37x50_smooth_420q10',
         '37x50_smooth_420q50opt']
    clips, boxes = [[a], [b]], [[[8, 0, 48, 1]], [[5, 0, 37, 0]]]
    (_, labels, masks, _), = list(train_fine.SyntheticCharades(2, 1, frames=8, crop=64))
    jclips = collate.fine_collate_jpeg([(s, labels[i], 'v%d' % i) for i, s in enumerate(jc.jpeg_samples(clips, boxes))])[0]
    rclips = collate.fine_collate_raw_u8([(s, labels[i], 'v%d' % i) for i, s in enumerate(jc.raw_samples([[a], [b + b[:2]]], boxes))])[0]
    rclips = type(rclips)(rclips.frames, torch.tensor([[8], [6]], dtype=torch.int32), rclips.box)     # the second video: 6 frames of its own
    rclips.frames[1, 0, 6:] = 0
    torch.manual_seed(0)
    net = train_fine.build_model(DEV, pretrained=None, dropout=0.0, input_norm=(MEAN, STD))
    net.train(True)
    net2 = copy.deepcopy(net)
    prev = cfn_hip.deterministic(True)
    try:
        losses = []
        for n, batch in ((net, jclips), (net2, rclips)):
            opt = optim.SGD(n.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
            x = train_fine.flatten_clips(batch, torch.device(DEV), 64)
            out = train_fine.train_step(n, cdist.GradReducer(n.parameters()), opt, x, labels.to(DEV), masks.to(DEV))
            losses.append((float(out[0]), float(out[1])))
    finally:
        cfn_hip.deterministic(prev)
    print('train step: JPEG-fed cls %.9g loc %.9g | pixel-fed cls %.9g loc %.9g' % (losses[0] + losses[1]))
    assert losses[0] == losses[1] and all(np.isfinite(v) for v in losses[0])
