"""Batch builders of the two training scripts: ragged per-video samples -> the padded, masked batch
structure the models and losses consume.

* ``fine_collate``  = ``mt_collate_fn`` of charades_fine.py:201-224
  sample  = (clips (n,3,T,H,W), label (157,TL), vid)
  batch   = [clips (B,n,3,Tmax,H,W), label (B,157,TLmax), mask (B,TLmax), [vid...]]
* ``coarse_collate`` = ``mt_collate_fn`` of charades_coarse_fineFEAT.py:208-252
  sample  = (clips, label, feat{k: (C_k,T',7,7)}, meta (4,), vid, dur)
  batch   = [clips, label, mask, feat{k: (B,C_k,T'max<=cap,7,7)}, feat_mask (B,T'max), meta (B,4), [vid...], dur (B,)]

Zero padding on the right along time, ``mask`` = 1 over each sample's own label length, fine features and their mask
truncated to ``cap`` = 128 frames (the Gaussian-alignment tables of the fusion layers are sized for that).  Inputs may
be numpy arrays or tensors; outputs are fp32 tensors (pin them and copy with non_blocking=True in the loader).

``fine_collate_u8`` / ``coarse_collate_u8``: the same batches from samples whose clips are still uint8 frames
(n, T, H, W, 3), channels last, as the decoder and the crop / flip transforms leave them.  The clip member becomes a
``U8Clips(frames (B,n,Tmax,H,W,3) uint8, lengths (B,n) int32)``: a quarter of the bytes to pad, pin and copy, and no CPU
normalisation (the reference's ToTensor + Normalize, spatial_transforms.py:46-85, :108-118) -- the stem conv normalises on the
GPU (``model.set_input_norm``).  Labels, masks, features and meta are what the fp32 builders produce.

``fine_collate_raw_u8`` / ``coarse_collate_raw_u8``: the clips are the frames AS DECODED, before any spatial transform -- the clip
member of a sample is a pair ``(frames (n, T, h, w, 3) uint8, box (n, 4) int = x1, y1, c, flip)`` with h, w differing from sample
to sample (cfn_hip.u8aug.train_crop_params / center_crop_params draw the boxes as the reference's transforms do).  The clip
member of the batch becomes a ``RawU8Clips(frames (B,n,Tmax,Hmax,Wmax,3), lengths (B,n), box (B,n,4))``, every picture in the
top-left corner of its zero-padded frame; crop, resize and flip run on the GPU (``RawU8Clips.transform``, which the training and
extraction scripts call).

``coarse_collate_packed`` / ``_packed_u8`` / ``_packed_raw_u8``: the feature member of a sample is a ``cfn_hip.featpack.Record`` -- the
memory-mapped 16-bit record of the video (one file instead of five fp32 ones).  Member 3 of the batch becomes a ``PackedFeats``: the first
min(T', cap) frames of every block copied, unpadded and still 16-bit, into one flat buffer (five contiguous copies per sample, no zero
fill); ``PackedFeats.unpack()`` widens and pads on the GPU.  The other seven members are what ``coarse_collate*`` builds.

``fine_collate_jpeg`` / ``coarse_collate_jpeg`` / ``coarse_collate_packed_jpeg``: the samples of ``*_collate_raw_u8`` with the frames still ENCODED --
the clip member of a sample is a pair ``(n lists of T_i baseline JPEG frames (bytes), box (n, 4) int)``.  The clip member of the batch becomes a
``cfn_hip.jpegdec.JpegClips``: the entropy-coded segments in one flat buffer plus the decoder tables; ``JpegClips.decode()`` makes the RawU8Clips
batch on the GPU, bit for bit what PIL decodes (the training and extraction scripts call it).  All frames of a clip share size and sampling.

Segment labels: with EVERY builder above the label member of a sample may be a ``cfn_hip.seglabels.SegLabel`` -- the video's action segments
[class, start_s, end_s] plus the label window (``SegLabel.training(...)`` / ``SegLabel.testing(...)``) -- instead of the dense (157, TL) array.  The
label member of the batch is then a ``cfn_hip.seglabels.SegLabels`` (a few hundred bytes) and the mask member is ``None``; the batch keeps its 4 / 8
members.  ``SegLabels.dense()`` writes labels (B, 157, TLmax), mask (B, TLmax) and the valid lengths on the GPU, bit for bit what the dense collate
gives (``cfn_hip.seglabels.materialize``, which the training scripts call).  All samples of a batch carry the same kind of label; 'loc' task only.
"""
import numpy as np
import torch

from cfn_hip.u8clips import RawU8Clips, U8Clips, CHARADES_MEAN, CHARADES_STD  # noqa: F401
from cfn_hip.featpack import PackedFeats, Record, collate_records  # noqa: F401
from cfn_hip.jpegdec import JpegClips, collate_jpeg  # noqa: F401
from cfn_hip.seglabels import SegLabel, SegLabels, collate_seg  # noqa: F401


def _t(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))


def _pad_time(items, dim, length):
    """stack `items` after zero-padding dimension `dim` on the right to `length`"""
    first = _t(items[0])
    shape = list(first.shape)
    shape[dim] = length
    out = torch.zeros([len(items)] + shape, dtype=torch.float32)
    for i, it in enumerate(items):
        it = _t(it).to(torch.float32)
        n = min(it.shape[dim], length)
        idx = [i] + [slice(None)] * it.dim()
        idx[dim + 1] = slice(0, n)
        out[tuple(idx)] = it.narrow(dim, 0, n)
    return out


def _label_mask(labels, tl):
    mask = torch.zeros(len(labels), tl, dtype=torch.float32)
    for i, lb in enumerate(labels):
        mask[i, :_t(lb).shape[1]] = 1.0
    return mask


def _labels(labels):
    """the label and mask members of a batch: dense (B, C, TLmax) + (B, TLmax), or SegLabels + None when the samples carry SegLabel records"""
    if any(isinstance(lb, SegLabel) for lb in labels):
        return collate_seg(labels), None
    tl_max = max(_t(lb).shape[1] for lb in labels)
    return _pad_time(labels, 1, tl_max), _label_mask(labels, tl_max)


def _pad_time_u8(clips):
    """uint8 clips (n, T_i, H, W, 3) -> U8Clips((B, n, Tmax, H, W, 3), lengths (B, n)); zero bytes behind each clip's own length"""
    clips = [_t(c) for c in clips]
    for c in clips:
        if c.dtype != torch.uint8 or c.dim() != 5 or c.shape[4] != 3:
            raise ValueError('uint8 clips of shape (n, T, H, W, 3) expected, got %s %s' % (c.dtype, tuple(c.shape)))
    t_max = max(c.shape[1] for c in clips)
    n, _, H, W, _ = clips[0].shape
    frames = torch.zeros((len(clips), n, t_max, H, W, 3), dtype=torch.uint8)
    lengths = torch.zeros((len(clips), n), dtype=torch.int32)
    for i, c in enumerate(clips):
        frames[i, :, :c.shape[1]] = c
        lengths[i] = c.shape[1]
    return U8Clips(frames, lengths)


def _pad_raw_u8(samples):
    """[(frames (n, T_i, h_i, w_i, 3) uint8, box (n, 4) int)] -> RawU8Clips((B, n, Tmax, Hmax, Wmax, 3), lengths (B, n), box (B, n, 4)):
    zero bytes right of and below each picture and behind each clip's own length"""
    clips, boxes = [], []
    for smp in samples:
        if not isinstance(smp, (tuple, list)) or len(smp) != 2:
            raise ValueError('a raw clip is a pair (frames (n, T, h, w, 3) uint8, box (n, 4) int)')
        c, b = _t(smp[0]), _t(smp[1])
        if c.dtype != torch.uint8 or c.dim() != 5 or c.shape[4] != 3:
            raise ValueError('uint8 frames of shape (n, T, h, w, 3) expected, got %s %s' % (c.dtype, tuple(c.shape)))
        if b.is_floating_point() or b.dtype == torch.bool or tuple(b.shape) != (c.shape[0], 4):
            raise ValueError('integer boxes of shape (n, 4) = x1, y1, c, flip expected for %d clips, got %s %s' % (c.shape[0], b.dtype, tuple(b.shape)))
        b = b.to(torch.int32)
        h, w = c.shape[2], c.shape[3]
        for x1, y1, cs, flip in b.tolist():
            if cs <= 0 or x1 < 0 or y1 < 0 or x1 + cs > w or y1 + cs > h or flip not in (0, 1):
                raise ValueError('box (x1, y1, c, flip) = %s does not lie inside the %d x %d frames' % ((x1, y1, cs, flip), h, w))
        clips.append(c)
        boxes.append(b)
    n = clips[0].shape[0]
    if any(c.shape[0] != n for c in clips):
        raise ValueError('the same number of clips per sample expected, got %s' % [c.shape[0] for c in clips])
    t_max, h_max, w_max = (max(c.shape[d] for c in clips) for d in (1, 2, 3))
    frames = torch.zeros((len(clips), n, t_max, h_max, w_max, 3), dtype=torch.uint8)
    lengths = torch.zeros((len(clips), n), dtype=torch.int32)
    for i, c in enumerate(clips):
        frames[i, :, :c.shape[1], :c.shape[2], :c.shape[3]] = c
        lengths[i] = c.shape[1]
    return RawU8Clips(frames, lengths, torch.stack(boxes))


def fine_collate(batch):
    clips = [b[0] for b in batch]
    t_max = max(_t(c).shape[2] for c in clips)
    return [_pad_time(clips, 2, t_max), *_labels([b[1] for b in batch]), [b[2] for b in batch]]


def fine_collate_u8(batch):
    """fine_collate for samples (uint8 clips (n,T,H,W,3), label (157,TL), vid)"""
    return [_pad_time_u8([b[0] for b in batch]), *_labels([b[1] for b in batch]), [b[2] for b in batch]]


def fine_collate_raw_u8(batch):
    """fine_collate for samples ((frames (n,T,h,w,3) uint8, box (n,4)), label (157,TL), vid): untransformed frames + crop boxes"""
    return [_pad_raw_u8([b[0] for b in batch]), *_labels([b[1] for b in batch]), [b[2] for b in batch]]


def _coarse_rest(batch, cap):
    """everything of a coarse batch but the clip: [label, mask, feat, feat_mask, meta, [vid...], dur]"""
    feats = [b[2] for b in batch]
    keys = list(feats[0].keys())
    tf_max = min(max(_t(f[keys[0]]).shape[1] for f in feats), cap)
    feat = {k: _pad_time([f[k] for f in feats], 1, tf_max) for k in keys}
    feat_mask = torch.zeros(len(batch), tf_max, dtype=torch.float32)
    for i, f in enumerate(feats):
        feat_mask[i, :min(cap, _t(f[keys[0]]).shape[1])] = 1.0
    meta = torch.stack([_t(b[3]) for b in batch])
    dur = torch.as_tensor([float(b[5]) for b in batch], dtype=torch.float64)
    return [*_labels([b[1] for b in batch]), feat, feat_mask, meta, [b[4] for b in batch], dur]


def coarse_collate(batch, cap=128):
    clips = [b[0] for b in batch]
    t_max = max(_t(c).shape[2] for c in clips)
    return [_pad_time(clips, 2, t_max)] + _coarse_rest(batch, cap)


def coarse_collate_u8(batch, cap=128):
    """coarse_collate for samples whose clips are uint8 (n,T,H,W,3)"""
    return [_pad_time_u8([b[0] for b in batch])] + _coarse_rest(batch, cap)


def coarse_collate_raw_u8(batch, cap=128):
    """coarse_collate for samples whose clips are (frames (n,T,h,w,3) uint8, box (n,4)) pairs: untransformed frames + crop boxes"""
    return [_pad_raw_u8([b[0] for b in batch])] + _coarse_rest(batch, cap)


def _coarse_rest_packed(batch, cap):
    """_coarse_rest for samples whose feature member is a Record: [label, mask, PackedFeats, feat_mask, meta, [vid...], dur]"""
    feat, feat_mask = collate_records([b[2] for b in batch], cap)
    meta = torch.stack([_t(b[3]) for b in batch])
    dur = torch.as_tensor([float(b[5]) for b in batch], dtype=torch.float64)
    return [*_labels([b[1] for b in batch]), feat, feat_mask, meta, [b[4] for b in batch], dur]


def coarse_collate_packed(batch, cap=128):
    """coarse_collate for samples (clips, label, Record, meta, vid, dur): the features stay 16-bit and unpadded (PackedFeats)"""
    clips = [b[0] for b in batch]
    t_max = max(_t(c).shape[2] for c in clips)
    return [_pad_time(clips, 2, t_max)] + _coarse_rest_packed(batch, cap)


def coarse_collate_packed_u8(batch, cap=128):
    """coarse_collate_packed for samples whose clips are uint8 (n,T,H,W,3)"""
    return [_pad_time_u8([b[0] for b in batch])] + _coarse_rest_packed(batch, cap)


def coarse_collate_packed_raw_u8(batch, cap=128):
    """coarse_collate_packed for samples whose clips are (frames (n,T,h,w,3) uint8, box (n,4)) pairs"""
    return [_pad_raw_u8([b[0] for b in batch])] + _coarse_rest_packed(batch, cap)


def fine_collate_jpeg(batch):
    """fine_collate_raw_u8 for samples ((n lists of encoded frames, box (n,4)), label (157,TL), vid): the frames stay JPEG (JpegClips)"""
    return [collate_jpeg([b[0] for b in batch]), *_labels([b[1] for b in batch]), [b[2] for b in batch]]


def coarse_collate_jpeg(batch, cap=128):
    """coarse_collate_raw_u8 for samples whose clips are (n lists of encoded frames, box (n,4)) pairs"""
    return [collate_jpeg([b[0] for b in batch])] + _coarse_rest(batch, cap)


def coarse_collate_packed_jpeg(batch, cap=128):
    """coarse_collate_packed_raw_u8 for samples whose clips are (n lists of encoded frames, box (n,4)) pairs"""
    return [collate_jpeg([b[0] for b in batch])] + _coarse_rest_packed(batch, cap)
