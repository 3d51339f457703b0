"""GPU: the 'sync' entropy mode of csrc/jpegdec.hip (jpeg_entropy_sync_kernel: one workgroup per frame without restart markers, one lane per
subsequence) against the pixels PIL decoded and against the lane-per-interval mode.

Bounds.  Integer arithmetic from the bit stream to the RGB bytes, and the rounds are exact by construction (cfn_hip.jpegdec
decode_coefficients_sync, tests/test_jpeg_sync_cpu.py): every comparison is torch.equal, losses are compared with ==.  Shapes: the fixtures
are at most 48 x 64; 16 bytes per subsequence is the smallest size the entry point takes and gives the most subsequences and rounds per
frame; the 360 x 480 bench frame at 16 bytes has more subsequences (970) than the workgroup has lanes (128), 48x64_noise_420q100 at 16 needs
as many rounds as it has subsequences (380)."""
import copy
import os

import numpy as np
import pytest
import torch

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]


def _plain():
    from cfn_hip import jpegdec
    return [n for n in jc.names() if jpegdec.parse(jc.jpg(n)).restart_interval == 0]


def _batch(clips, boxes):
    from cfn_hip import jpegdec
    return jpegdec.collate_jpeg(jc.jpeg_samples(clips, boxes))


def _decode(clips, **kw):
    """(frames on the host, status words); the sync mode with the most subsequences per frame the kernel takes, so that no frame that is
    meant to go through it falls back"""
    from cfn_hip import jpegdec, ops
    status = torch.full((clips.frames.shape[0],), 77, dtype=torch.int32, device=DEV)
    if kw.get('entropy') == 'sync':
        kw.setdefault('max_subs', jpegdec.SYNC_MAX_SUBS)
    frames = ops.jpeg_decode_u8(clips, status=status, **kw)
    return frames.view(tuple(clips.lengths.shape) + tuple(frames.shape[-4:])).cpu(), status.cpu()


@pytest.mark.parametrize('sub_bytes', (16, 64))
def test_every_plain_fixture_alone(sub_bytes):
    from cfn_hip import jpegdec
    bad = []
    for name in _plain():
        clips = jpegdec.collate_jpeg([([[jc.jpg(name)]], torch.tensor([jc.full_box(name)]))]).to(DEV)
        got, st = _decode(clips, entropy='sync', sub_bytes=sub_bytes)
        ref, st0 = _decode(clips)
        want = torch.from_numpy(np.array(jc.pixels(name)))
        diff = int((got[0, 0, 0] != want).sum())
        if diff or st.any() or st0.any() or not torch.equal(got, ref):
            bad.append((name, diff, st.tolist()))
    assert not bad, bad


@pytest.mark.parametrize('which,sub_bytes', (('mixed', 16), ('ragged', 16), ('mixed', 128), ('ragged', 128)))
def test_mixed_and_ragged_batches(which, sub_bytes):
    """restart frames, a gray clip, an empty clip and (at 128 bytes) frames shorter than a subsequence in one call with frames the sync
    mode takes"""
    from cfn_hip import jpegdec
    cl, bx = (jc.MIXED, jc.MIXED_BOX) if which == 'mixed' else (jc.RAGGED, jc.RAGGED_BOX)
    clips = _batch(cl, bx)
    by = clips.frames[:, jpegdec.F_BYTES]
    plain = clips.frames[:, jpegdec.F_RESTART] == 0
    assert bool((plain & (by > sub_bytes)).any()) and bool((~plain).any()) and (sub_bytes == 16 or bool((plain & (by <= sub_bytes)).any()))
    got, st = _decode(clips.to(DEV), entropy='sync', sub_bytes=sub_bytes)
    assert torch.equal(got, jc.padded(cl)) and not st.any()
    # a dirty, preallocated output: every byte is written in this mode too
    out = torch.full(tuple(got.shape), 0xA5, dtype=torch.uint8, device=DEV)
    clips.to(DEV).decode(out=out, entropy='sync', sub_bytes=sub_bytes)
    assert torch.equal(out.cpu(), jc.padded(cl))


def test_max_subs_falls_back():
    """frames with more than max_subs subsequences keep the lane-per-interval decode; the output does not change"""
    from cfn_hip import jpegdec, ops
    clips = _batch(jc.MIXED, jc.MIXED_BOX)
    n = -(-clips.frames[:, jpegdec.F_BYTES] // 16)
    assert bool((n > 4).all()) and bool((n > 8).any()) and bool((n <= 8).any())       # 4: every frame falls back; 8: some do
    d = clips.to(DEV)
    for most in (4, 8):
        status = torch.empty(clips.frames.shape[0], dtype=torch.int32, device=DEV)
        got = ops.jpeg_decode_u8(d, status=status, entropy='sync', sub_bytes=16, max_subs=most)
        assert torch.equal(got.cpu().view(tuple(jc.padded(jc.MIXED).shape)), jc.padded(jc.MIXED)) and not status.cpu().any()


def test_more_subsequences_than_lanes_and_many_rounds():
    from cfn_hip import jpegdec
    z = np.load(os.path.join(jc.GOLDEN, 'jpeg_bench.npz'), allow_pickle=False)
    big = z['360x480.jpg'].tobytes()
    info = jpegdec.parse(big)
    assert -(-(info.scan_end - info.scan_start) // 16) == 970
    clips = jpegdec.collate_jpeg([([[big, big]], torch.tensor([[0, 0, 360, 0]]))]).to(DEV)
    got, st = _decode(clips, entropy='sync', sub_bytes=16)
    ref, st0 = _decode(clips)
    assert torch.equal(got, ref) and not st.any() and not st0.any() and int(ref.max()) > 0
    name = '48x64_noise_420q100'                                   # 380 rounds for 380 subsequences (tests/test_jpeg_sync_cpu.py)
    clips = jpegdec.collate_jpeg([([[jc.jpg(name)]], torch.tensor([jc.full_box(name)]))]).to(DEV)
    got, st = _decode(clips, entropy='sync', sub_bytes=16)
    assert torch.equal(got, _decode(clips)[0]) and not st.any()
    assert torch.equal(got[0, 0, 0], torch.from_numpy(np.array(jc.pixels(name))))


CUT = [[['48x64_noise_420q100', '48x64_smooth_420q100', '48x64_smooth_420q75']], [['48x64_smooth_420q95', '48x64_smooth_420q75rst3']]]
CUT_BOX = [[[0, 0, 48, 0]], [[0, 0, 48, 0]]]


def test_cut_segments_are_flagged_like_the_default_path():
    """frames whose segment is cut in half, among whole ones: the same rows flagged as by the lane-per-interval mode, every other frame
    exact, decode_checked names the video.  (The cut frames are long enough to stay with the sync mode at 16 and at 128 bytes.)"""
    from cfn_hip import jpegdec
    clips = _batch(CUT, CUT_BOX)
    want = jc.padded(CUT)
    rows = clips.frames.shape[0]
    for cut_rows in ((0,), (1, 3), (4,)):
        fr = clips.frames.clone()
        for row in cut_rows:
            fr[row, jpegdec.F_BYTES] //= 2
        cut = clips._replace(frames=fr)
        assert all(int(fr[r, jpegdec.F_BYTES]) > 128 for r in cut_rows if int(fr[r, jpegdec.F_RESTART]) == 0)
        ref, st0 = _decode(cut.to(DEV))
        for sub in (16, 128):
            got, st = _decode(cut.to(DEV), entropy='sync', sub_bytes=sub)
            assert [bool(s) for s in st.tolist()] == [bool(s) for s in st0.tolist()] == [r in cut_rows for r in range(rows)], (st, st0)
            for r in range(rows):
                if r not in cut_rows:
                    c, t = int(fr[r, jpegdec.F_CLIP]), int(fr[r, jpegdec.F_T])
                    assert torch.equal(got[c, 0, t], want[c, 0, t])
        video = 'v%d' % int(fr[cut_rows[0], jpegdec.F_CLIP])
        with pytest.raises(RuntimeError, match=video):
            jpegdec.decode_checked(cut, torch.device(DEV), ['v0', 'v1'], entropy='sync')
    raw = jpegdec.decode_checked(clips, torch.device(DEV), ['v0', 'v1'], entropy='sync')
    assert torch.equal(raw.frames.cpu(), want)


def test_two_decodes_give_equal_bytes(monkeypatch):
    clips = _batch(jc.RAGGED, jc.RAGGED_BOX).to(DEV)
    a, _ = _decode(clips, entropy='sync', sub_bytes=16)
    b, _ = _decode(clips, entropy='sync', sub_bytes=16)
    assert torch.equal(a, b)
    monkeypatch.setenv('CFN_JPEG_ENTROPY', 'sync')                 # the default of decode(), read at call time
    status = torch.full((clips.frames.shape[0],), 77, dtype=torch.int32, device=DEV)
    c = clips.decode(status=status)
    assert torch.equal(a, c.frames.cpu()) and not status.cpu().any()
    assert torch.equal(a, clips.decode(entropy='sync', sub_bytes=32).frames.cpu())


def test_native_operator_equals_ctypes():
    from cfn_hip import ops, torchlib  # noqa: F401
    d = _batch(jc.MIXED, jc.MIXED_BOX).to(DEV)
    frames, status = torch.ops.cfn.jpeg_decode_sync_u8(d.data, d.frames, d.tables, d.geom, d.lengths, list(d.dims), 16, 64)
    assert torch.equal(frames, ops.jpeg_decode_u8(d, entropy='sync', sub_bytes=16, max_subs=64)) and not status.cpu().any()
    assert torch.equal(frames.cpu().view(tuple(jc.padded(jc.MIXED).shape)), jc.padded(jc.MIXED))
    with pytest.raises(RuntimeError, match='sub_bytes'):
        torch.ops.cfn.jpeg_decode_sync_u8(d.data, d.frames, d.tables, d.geom, d.lengths, list(d.dims), 18, 64)
    with pytest.raises(RuntimeError, match='max_subs'):
        torch.ops.cfn.jpeg_decode_sync_u8(d.data, d.frames, d.tables, d.geom, d.lengths, list(d.dims), 16, 0)


def test_train_step_loss_bits():
    """one train_fine.train_step fed a JpegClips batch decoded with jpeg_entropy='sync' returns the loss bits of the same step with the
    default decode (8 frames, crop 64: the smallest the model tests use; five of the frames are longer than the default subsequence)"""
    import cfn_hip
    import collate
    import torch.optim as optim
    import train_fine
    from cfn_hip import dist as cdist
    from cfn_hip import jpegdec
    a = ['48x64_smooth_420q75', '48x64_smooth_420q95', '48x64_smooth_420q50opt', '48x64_smooth_420q10', '48x64_smooth_420q100',
         '48x64_smooth_420q75rst3', '48x64_noise_420q100', '48x64_smooth_420q75']
    b = ['37x50_smooth_420q75', '37x50_smooth_420q95', '37x50_noise_420q100', '37x50_smooth_420q75rst3', '37x50_smooth_420q10',
         '37x50_smooth_420q50opt']
    clips, boxes = [[a], [b]], [[[8, 0, 48, 1]], [[5, 0, 37, 0]]]
    (_, labels, masks, _), = list(train_fine.SyntheticCharades(2, 1, frames=8, crop=64))
    jclips = collate.fine_collate_jpeg([(s, labels[i], 'v%d' % i) for i, s in enumerate(jc.jpeg_samples(clips, boxes))])[0]
    taken = (jclips.frames[:, jpegdec.F_RESTART] == 0) & (jclips.frames[:, jpegdec.F_BYTES] > jpegdec.SYNC_SUB_BYTES)
    assert int(taken.sum()) >= 3
    torch.manual_seed(0)
    net = train_fine.build_model(DEV, pretrained=None, dropout=0.0, input_norm=(MEAN, STD))
    net.train(True)
    net2 = copy.deepcopy(net)
    prev = cfn_hip.deterministic(True)
    try:
        losses = []
        for n, mode in ((net, 'sync'), (net2, None)):
            opt = optim.SGD(n.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-5)
            x = train_fine.flatten_clips(jclips, torch.device(DEV), 64, names=['v0', 'v1'], jpeg_entropy=mode)
            out = train_fine.train_step(n, cdist.GradReducer(n.parameters()), opt, x, labels.to(DEV), masks.to(DEV))
            losses.append((float(out[0]), float(out[1])))
    finally:
        cfn_hip.deterministic(prev)
    print('train step: sync-decoded cls %.9g loc %.9g | default cls %.9g loc %.9g' % (losses[0] + losses[1]))
    assert losses[0] == losses[1] and all(np.isfinite(v) for v in losses[0])
