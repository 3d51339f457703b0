"""Packed 16-bit fine features: the five multi-level feature maps of the Fine stream stay fp16 or bf16 on disk, on the host and over PCIe,
unpadded, one record per video; a kernel widens and pads them into the fp32 maps the fusion layers take (cfn_hip.ops.feat_unpack,
csrc/featpack.hip).

The reference stores five fp32 files per video (extract_fineFEAT.py:153-173), reads them back in the dataset
(charades_coarse_fineFEAT.py:84-87) and collates zero-padded fp32 batches (:208-252): 792 channels x 128 frames x 49 positions x 4 bytes =
19.9 MB per clip at the collate cap.  The features are post-ReLU spatial means; fp16 rounds them by at most 2^-11 relative, bf16 by 2^-8.

Record ``<save_dir>/packed/<vid>.cff``, little-endian:

    0   magic  b'CFNFEAT1'
    8   u32    dtype: 1 = fp16, 2 = bf16
    12  u32    frames T'
    16  u32    positions (49)
    20  u32    number of keys (5)
    24  5 x u32 channel counts, in FEAT_KEYS order
    44  zero up to byte 64
    64  payload: per key one TIME-MAJOR block (T', C_k, 49) of 16-bit values

Time-major makes the first `cap` frames of every key a contiguous prefix of its block: truncation at the collate cap is a slice.  Channel
counts are multiples of 8, so every frame (C_k x 98 bytes) and every block starts on a 16-byte boundary.

This module is host only (numpy + torch); ``PackedFeats.unpack`` is the one call that needs the GPU library.
"""
import collections
import os
import struct
import warnings

import numpy as np
import torch

FEAT_KEYS = ('layer1', 'layer2', 'layer3', 'layer4', 'conv5')
MAGIC = b'CFNFEAT1'
HEADER_BYTES = 64
POSITIONS = 49
DTYPE_CODES = {1: torch.float16, 2: torch.bfloat16}
DTYPE_NAMES = {'fp16': torch.float16, 'f16': torch.float16, 'half': torch.float16, 'bf16': torch.bfloat16, 'bfloat16': torch.bfloat16}
PACKED_DIR = 'packed'
SUFFIX = '.cff'


def feat_dtype(dtype):
    """'fp16' / 'bf16' / torch.float16 / torch.bfloat16 -> the torch dtype; anything else is refused"""
    dt = DTYPE_NAMES.get(dtype, dtype) if isinstance(dtype, str) else dtype
    if dt not in (torch.float16, torch.bfloat16):
        raise ValueError("feature dtype must be 'fp16' or 'bf16', got %r" % (dtype,))
    return dt


def _code(dt):
    return 1 if dt == torch.float16 else 2


def _check_channels(channels):
    channels = tuple(int(c) for c in channels)
    if len(channels) != len(FEAT_KEYS) or any(c <= 0 or c % 8 for c in channels):
        raise ValueError('%d channel counts that are positive multiples of 8 expected (every frame and block then starts on a 16-byte '
                         'boundary), got %s' % (len(FEAT_KEYS), channels))
    return channels


def record_path(save_dir, vid):
    return os.path.join(save_dir, PACKED_DIR, vid + SUFFIX)


def payload_elements(frames, channels):
    return int(frames) * sum(channels) * POSITIONS


def _as_bits(t):
    """a 16-bit float tensor as its int16 bit patterns (numpy has no bfloat16)"""
    return t.contiguous().view(torch.int16)


def pack_reference(feat, dtype):
    """{k: (C_k, T', 7, 7)} (or (1, C_k, T', 7, 7)) fp32 -> (payload 1-D `dtype` tensor, T', channels) on the CPU with tensor.to(dtype):
    the statement of what ops.feat_pack computes"""
    dt = feat_dtype(dtype)
    blocks, channels, frames = [], [], None
    for k in FEAT_KEYS:
        x = feat[k]
        x = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
        if x.dim() == 5 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 4 or x.shape[2] * x.shape[3] != POSITIONS:
            raise ValueError('feature map %s: (C, T, 7, 7) expected, got %s' % (k, tuple(x.shape)))
        if frames is None:
            frames = int(x.shape[1])
        elif int(x.shape[1]) != frames:
            raise ValueError('feature map %s has %d frames, %s has %d' % (k, x.shape[1], FEAT_KEYS[0], frames))
        channels.append(int(x.shape[0]))
        blocks.append(x.detach().cpu().to(torch.float32).to(dt).reshape(x.shape[0], frames, POSITIONS).permute(1, 0, 2).reshape(-1))
    return torch.cat(blocks), frames, _check_channels(channels)


def write_record(path, payload, dtype, frames, channels):
    """payload: 1-D 16-bit tensor (or its raw bytes) of frames * sum(channels) * 49 elements, the five time-major blocks back to back"""
    dt = feat_dtype(dtype)
    channels = _check_channels(channels)
    frames = int(frames)
    if frames < 1:
        raise ValueError('a record holds at least one frame, got %d' % frames)
    n = payload_elements(frames, channels)
    if torch.is_tensor(payload):
        if payload.dtype != dt or payload.numel() != n:
            raise ValueError('payload of %d %s elements expected, got %d %s' % (n, dt, payload.numel(), payload.dtype))
        raw = _as_bits(payload.detach().cpu().reshape(-1)).numpy().tobytes()
    else:
        raw = bytes(payload)
        if len(raw) != 2 * n:
            raise ValueError('payload of %d bytes expected, got %d' % (2 * n, len(raw)))
    head = MAGIC + struct.pack('<4I', _code(dt), frames, POSITIONS, len(FEAT_KEYS)) + struct.pack('<5I', *channels)
    head += b'\0' * (HEADER_BYTES - len(head))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as fh:
        fh.write(head)
        fh.write(raw)
    return path


class Record(object):
    """an opened record: ``dtype``, ``frames``, ``channels`` and memory-mapped views of the blocks"""

    def __init__(self, path):
        self.path = path
        try:
            size = os.path.getsize(path)
            with open(path, 'rb') as fh:
                head = fh.read(HEADER_BYTES)
        except OSError as exc:
            raise ValueError('%s: cannot read the record (%s)' % (path, exc))
        if len(head) < HEADER_BYTES or head[:8] != MAGIC:
            raise ValueError('%s: not a packed feature record (magic %r)' % (path, head[:8]))
        code, frames, pos, nkeys = struct.unpack('<4I', head[8:24])
        if code not in DTYPE_CODES:
            raise ValueError('%s: unknown dtype code %d (1 = fp16, 2 = bf16)' % (path, code))
        if pos != POSITIONS or nkeys != len(FEAT_KEYS) or frames < 1:
            raise ValueError('%s: %d positions, %d keys, %d frames (49 positions, 5 keys, >= 1 frame expected)' % (path, pos, nkeys, frames))
        channels = struct.unpack('<5I', head[24:44])
        try:
            channels = _check_channels(channels)
        except ValueError as exc:
            raise ValueError('%s: %s' % (path, exc))
        want = HEADER_BYTES + 2 * payload_elements(frames, channels)
        if size != want:
            raise ValueError('%s: %d bytes, but %d frames of %s channels take %d' % (path, size, frames, channels, want))
        self.dtype, self.frames, self.channels = DTYPE_CODES[code], int(frames), channels
        self._map = np.memmap(path, dtype='<i2', mode='r', offset=HEADER_BYTES, shape=(payload_elements(frames, channels),))
        self._start = [0]
        for c in channels:
            self._start.append(self._start[-1] + self.frames * c * POSITIONS)

    def _bits(self, k, t_max=None):
        """key k's first min(T', t_max) frames as a flat int16 numpy view of the map: a contiguous prefix of the block"""
        k = FEAT_KEYS.index(k) if isinstance(k, str) else int(k)
        t = self.frames if t_max is None else max(0, min(self.frames, int(t_max)))
        return self._map[self._start[k]:self._start[k] + t * self.channels[k] * POSITIONS], t, self.channels[k]

    def block(self, k, t_max=None):
        """the memory-mapped (t, C_k, 49) view of key k (index or name), t = min(T', t_max); read-only"""
        bits, t, c = self._bits(k, t_max)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')            # (torch warns about tensors over read-only memory: nothing here writes)
            return torch.from_numpy(bits).view(self.dtype).view(t, c, POSITIONS)

    def to_dict(self):
        """the reference's sample member {k: (C_k, T', 7, 7)} in fp32"""
        return {k: self.block(i).to(torch.float32).permute(1, 0, 2).reshape(self.channels[i], self.frames, 7, 7).contiguous()
                for i, k in enumerate(FEAT_KEYS)}

    def __repr__(self):
        return 'Record(%r, %s, frames=%d, channels=%s)' % (self.path, self.dtype, self.frames, self.channels)

    def __getstate__(self):            # (DataLoader workers: the map is reopened on the other side)
        return self.path

    def __setstate__(self, path):
        self.__init__(path)


def open_record(path):
    return Record(path)


def convert_dir(src, dst, dtype):
    """an fp32 five-file store ``src/<key>/<vid>`` (extract_fineFEAT.extract) -> records ``dst/packed/<vid>.cff``, on the CPU with
    tensor.to(dtype); returns the number of videos"""
    dt = feat_dtype(dtype)
    vids = sorted(os.listdir(os.path.join(src, FEAT_KEYS[0])))
    for vid in vids:
        feat = {k: torch.load(os.path.join(src, k, vid), map_location='cpu') for k in FEAT_KEYS}
        payload, frames, channels = pack_reference(feat, dt)
        write_record(record_path(dst, vid), payload, dt, frames, channels)
    return len(vids)


class PackedFeats(collections.namedtuple('PackedFeats', ['data', 'offsets', 'lengths', 'channels', 't_max'])):
    """A batch of packed fine features: ``data`` 1-D fp16 / bf16, every video's five time-major blocks (length, C_k, 49) somewhere inside
    it; ``offsets`` (B, 5) int64 = first element of each block, multiples of 8; ``lengths`` (B,) int32 = each video's min(T', cap);
    ``channels`` the five channel counts; ``t_max`` = max(lengths) as a HOST int (unpack() never reads the device for it).

    Stands for the dict {k: (B, C_k, t_max, 7, 7) fp32}, zero behind each video's own length.  A namedtuple, like U8Clips: staging and
    DataLoader pinning rebuild it around the moved tensors."""
    __slots__ = ()

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def batch(self):
        return int(self.lengths.shape[0])

    def keys(self):
        return FEAT_KEYS

    def to(self, device, non_blocking=False):
        """move the three tensors to `device`; the element types are part of the format, so a dtype is refused"""
        if isinstance(device, torch.dtype) or not isinstance(device, (str, int, torch.device)):
            raise TypeError('PackedFeats.to() takes a device: data stays %s, offsets int64 and lengths int32 (unpack() makes the fp32 maps)'
                            % (self.data.dtype,))
        return PackedFeats(self.data.to(device, non_blocking=non_blocking), self.offsets.to(device, non_blocking=non_blocking),
                           self.lengths.to(device, non_blocking=non_blocking), self.channels, self.t_max)

    def cuda(self, device=None, non_blocking=False):
        return PackedFeats(self.data.cuda(device, non_blocking=non_blocking), self.offsets.cuda(device, non_blocking=non_blocking),
                           self.lengths.cuda(device, non_blocking=non_blocking), self.channels, self.t_max)

    def unpack(self, out=None):
        """{k: (B, C_k, t_max, 7, 7) fp32} on the data's device and current stream, one kernel launch for the five maps
        (ops.feat_unpack); nothing is read back.  out: a dict of preallocated maps to write into."""
        from . import ops
        outs = None if out is None else [out[k] for k in FEAT_KEYS]
        ys = ops.feat_unpack(self.data, self.offsets, self.lengths, self.channels, self.t_max, out=outs)
        return dict(zip(FEAT_KEYS, ys))

    def unpack_reference(self):
        """unpack() with torch indexing, on any device: the tests' reference"""
        B, dev = self.batch, self.data.device
        t_max = int(self.t_max)
        lengths = self.lengths.to(torch.int64).clamp(0, t_max).tolist()
        offs = self.offsets.tolist()
        res = {}
        for i, k in enumerate(FEAT_KEYS):
            c = self.channels[i]
            y = torch.zeros(B, c, t_max, 7, 7, dtype=torch.float32, device=dev)
            for b in range(B):
                n = lengths[b]
                blk = self.data[offs[b][i]:offs[b][i] + n * c * POSITIONS].view(n, c, POSITIONS)
                y[b, :, :n] = blk.to(torch.float32).permute(1, 0, 2).reshape(c, n, 7, 7)
            res[k] = y
        return res


def collate_records(records, cap=128):
    """[Record] -> (PackedFeats on the host, feat_mask (B, t_max) fp32): five contiguous prefix copies per sample into one flat buffer,
    nothing zero-filled"""
    if not records:
        raise ValueError('an empty batch')
    for r in records:
        if not isinstance(r, Record):
            raise ValueError('the feature member of a packed sample is a cfn_hip.featpack.Record, got %s' % type(r).__name__)
    dt, channels = records[0].dtype, records[0].channels
    if any(r.dtype != dt or r.channels != channels for r in records):
        raise ValueError('records of one dtype and one set of channel counts expected in a batch, got %s'
                         % [(r.dtype, r.channels) for r in records])
    lengths = [min(r.frames, int(cap)) for r in records]
    per_frame = sum(channels) * POSITIONS
    data = torch.empty(sum(lengths) * per_frame, dtype=dt)
    bits = data.view(torch.int16)
    offsets, pos = [], 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                # (tensors over the read-only maps: they are only read)
        for b, r in enumerate(records):
            offsets.append([])
            for k in range(len(FEAT_KEYS)):
                src = torch.from_numpy(r._bits(k, lengths[b])[0])
                bits[pos:pos + src.numel()].copy_(src)         # one contiguous copy: a prefix of the block
                offsets[b].append(pos)
                pos += src.numel()
    offsets = torch.tensor(offsets, dtype=torch.int64)
    t_max = max(lengths)
    mask = torch.zeros(len(records), t_max, dtype=torch.float32)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1.0
    return PackedFeats(data, offsets, torch.tensor(lengths, dtype=torch.int32), channels, t_max), mask
