"""uint8 video batches: frames stay bytes on the host, over PCIe and in HBM; the stem conv normalises them where it loads
them (cfn_hip.ops.stem_conv_u8, csrc/stem_u8.hip).

The reference normalises on the CPU -- ToTensor(255) + Normalize(mean, std) per frame (spatial_transforms.py:46-85, :108-118),
stack + permute per clip (charades_fine.py:170-173) -- and collates padded fp32 batches.  Crop, resize and flip commute with the
conversion and run on the GPU as well, on the bytes: a loader may hand over the frames as decoded, with one crop box per clip
(RawU8Clips below; ops.crop_resize_flip_u8, csrc/aug_u8.hip, bit-exact to the reference's PIL transforms), or do that work itself
and hand over U8Clips.  Only the decode stays on the host.
"""
import collections

import torch

# per-channel statistics of the Charades training set, frame-wise means (train_fine.py:48-49)
CHARADES_MEAN = [0.413, 0.368, 0.338]
CHARADES_STD = [0.131, 0.125, 0.132]


def clip_lut(mean, std, norm_value=255):
    """(3, 256) fp32 table: the normalised value of every byte per channel, computed with the reference's operations in the
    reference's order -- ``img.float().div(norm_value)`` (ToTensor), then ``t.sub_(m).div_(s)`` per channel (Normalize) -- so that
    a gather through it is bit-identical to the reference's clip (a multiply-add form is off by up to 4.8e-7)."""
    if len(mean) != 3 or len(std) != 3:
        raise ValueError('clip_lut: mean and std of the 3 image channels expected')
    lut = torch.arange(256, dtype=torch.uint8).view(1, 256).repeat(3, 1).float().div(norm_value)
    for t, m, s in zip(lut, mean, std):
        t.sub_(m).div_(s)
    return lut


class U8Clips(collections.namedtuple('U8Clips', ['frames', 'lengths'])):
    """A batch of uint8 clips: ``frames`` (..., T, H, W, 3) uint8, channels last, zero padded on the right along time;
    ``lengths`` (...) int32 = every clip's own frame count.  Frame t >= length is padding and reads as 0.0 after
    normalisation (collate pads AFTER normalising, and no byte normalises to 0.0).

    A namedtuple, so the staging code and DataLoader pinning rebuild it around the moved tensors.  ``shape`` is the LOGICAL
    shape of the fp32 clip it stands for: (B, n, 3, T, H, W) as collated, (N, 3, T, H, W) after flatten_crops()."""
    __slots__ = ()

    @property
    def shape(self):
        s = tuple(self.frames.shape)
        return torch.Size(s[:-4] + (3,) + s[-4:-1])

    @property
    def device(self):
        return self.frames.device

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return len(self.shape)

    def to(self, device, non_blocking=False):
        """move both members to `device`; the element types are part of the format, so a dtype is refused"""
        if isinstance(device, torch.dtype) or not isinstance(device, (str, int, torch.device)):
            raise TypeError('U8Clips.to() takes a device: frames stay uint8 and lengths int32 (ops.clip_u8_to_f32 makes the fp32 clip)')
        return U8Clips(self.frames.to(device, non_blocking=non_blocking), self.lengths.to(device, non_blocking=non_blocking))

    def cuda(self, device=None, non_blocking=False):
        return U8Clips(self.frames.cuda(device, non_blocking=non_blocking), self.lengths.cuda(device, non_blocking=non_blocking))

    def flatten_crops(self):
        """(B, n, T, H, W, 3) -> (B * n, T, H, W, 3); lengths follow"""
        f = self.frames
        return U8Clips(f.reshape((-1,) + tuple(f.shape[-4:])), self.lengths.reshape(-1))

    def time_slice(self, t0, t1):
        """frames [t0, t1) of every clip; lengths are clamped to what is left of each clip inside the slice"""
        T = self.frames.shape[-4]
        t0, t1 = max(0, min(int(t0), T)), max(0, min(int(t1), T))
        t1 = max(t0, t1)
        return U8Clips(self.frames.narrow(-4, t0, t1 - t0), (self.lengths - t0).clamp(min=0, max=t1 - t0))

    def to_f32(self, lut):
        """the fp32 clip this batch stands for, (..., 3, T, H, W), by gathering the table with torch indexing (any device; the
        tests' reference -- the product path is ops.clip_u8_to_f32 / ops.stem_conv_u8)"""
        f = self.frames
        idx = f.long()
        x = torch.stack([lut[c].to(f.device)[idx[..., c]] for c in range(3)], dim=-1)      # (..., T, H, W, 3)
        T = f.shape[-4]
        live = torch.arange(T, device=f.device).view((1,) * self.lengths.dim() + (T,)) < self.lengths.unsqueeze(-1).to(f.device)
        x = torch.where(live.view(tuple(live.shape) + (1, 1, 1)), x, torch.zeros((), dtype=x.dtype, device=x.device))
        nd = x.dim()
        return x.permute(tuple(range(nd - 4)) + (nd - 1, nd - 4, nd - 3, nd - 2)).contiguous()


class RawU8Clips(collections.namedtuple('RawU8Clips', ['frames', 'lengths', 'box'])):
    """A batch of uint8 clips as DECODED, before the spatial transform: ``frames`` (..., T, Hs, Ws, 3) uint8, every clip's h x w picture
    in the top-left corner of a common Hs x Ws and zero padded along time; ``lengths`` (...) int32; ``box`` (..., 4) int32 =
    x1, y1, c, flip: the square crop window and whether the result is mirrored (cfn_hip.u8aug.train_crop_params / center_crop_params
    draw them as the reference's MultiScaleRandomCropMultigrid + RandomHorizontalFlip / CenterCropScaled do).

    ``transform(size)`` crops, resizes and flips on the frames' device and returns the U8Clips the models take.  A namedtuple, like
    U8Clips: staging and pinning rebuild it around the moved tensors.  ``shape`` is the logical shape BEFORE the transform."""
    __slots__ = ()

    @property
    def shape(self):
        s = tuple(self.frames.shape)
        return torch.Size(s[:-4] + (3,) + s[-4:-1])

    @property
    def device(self):
        return self.frames.device

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return len(self.shape)

    def to(self, device, non_blocking=False):
        """move all three members to `device`; the element types are part of the format, so a dtype is refused"""
        if isinstance(device, torch.dtype) or not isinstance(device, (str, int, torch.device)):
            raise TypeError('RawU8Clips.to() takes a device: frames stay uint8, lengths and box int32')
        return RawU8Clips(*[m.to(device, non_blocking=non_blocking) for m in self])

    def cuda(self, device=None, non_blocking=False):
        return RawU8Clips(*[m.cuda(device, non_blocking=non_blocking) for m in self])

    def flatten_crops(self):
        """(B, n, T, Hs, Ws, 3) -> (B * n, T, Hs, Ws, 3); lengths and boxes follow"""
        f = self.frames
        return RawU8Clips(f.reshape((-1,) + tuple(f.shape[-4:])), self.lengths.reshape(-1), self.box.reshape(-1, 4))

    def time_slice(self, t0, t1):
        """frames [t0, t1) of every clip, as U8Clips.time_slice; the boxes stay"""
        u = U8Clips(self.frames, self.lengths).time_slice(t0, t1)
        return RawU8Clips(u.frames, u.lengths, self.box)

    def transform(self, size, out=None):
        """crop + antialiased bilinear resize to size x size + flip on the GPU, on the current stream of the frames' device
        (ops.crop_resize_flip_u8): the U8Clips batch (..., T, size, size, 3) on the same device.  The crop extents box[..., 2] select
        the tap tables on the host: a box that already lives on the device is copied back for that (16 bytes per clip)."""
        from . import ops
        f = self.frames
        lead = tuple(f.shape[:-4])
        flat = self.flatten_crops()
        y = ops.crop_resize_flip_u8(flat.frames, flat.lengths, flat.box, size, out=out)
        return U8Clips(y.view(lead + tuple(y.shape[1:])), self.lengths)
