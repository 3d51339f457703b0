"""Baseline JPEG frames decoded on the GPU, bit for bit like PIL (cfn_hip.ops.jpeg_decode_u8, csrc/jpegdec.hip).

The reference decodes every frame on the host: ``Image.open(f).convert('RGB')`` in ``pil_loader`` (charades_fine.py,
charades_coarse_fineFEAT.py).  Here a loader may hand over the frames as the ENCODED bytes it read from disk: the host only walks the
markers (``parse``), copies every frame's entropy-coded segment into one flat buffer and builds the decoder tables (``collate_jpeg`` ->
``JpegClips``); Huffman decode, dequantisation, libjpeg's "islow" inverse DCT, "fancy" chroma upsampling and the fixed-point YCbCr -> RGB
conversion run on the GPU and leave a ``RawU8Clips`` batch, byte for byte what ``collate._pad_raw_u8`` builds from PIL's pixels.

Accepted: baseline sequential DCT (SOF0), 8 bit, Huffman, ONE interleaved scan, 1 component (gray, replicated to R = G = B) or 3
components YCbCr with luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1, Cb and Cr sharing their tables.  Anything
else is refused by ``parse`` with the reason.  All frames of one clip share size and sampling.  ``decode_reference`` states the same
arithmetic in numpy and plain Python: it serves the CPU tests and debugging and is NOT a fallback of ``JpegClips.decode()``, which has
no CPU path.

The entropy stage has two modes with the same output: 'interval' (the default), one lane per (frame, restart interval), and 'sync'
(``decode(entropy='sync')``, ``CFN_JPEG_ENTROPY=sync``), which decodes a frame WITHOUT restart markers with one lane per subsequence of
``sub_bytes`` raw bytes; ``decode_coefficients_sync`` states its rounds in plain Python.
"""
import collections

import numpy as np
import torch

from .u8clips import RawU8Clips

# zigzag position -> natural (row-major) index of the 8 x 8 block
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                   12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                   58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

# sampling codes of geom[..., 2]: luma (h << 4) | v
SAMP_444, SAMP_422, SAMP_420 = 0x11, 0x21, 0x22
_SAMPLINGS = {(1, 1): SAMP_444, (2, 1): SAMP_422, (2, 2): SAMP_420}

# one table set on the device, int32 words: 2 quantisation tables (natural order; slot 0 = component 0, slot 1 = components 1 and 2),
# then 4 Huffman tables DC0, DC1, AC0, AC1 (slot 0 / 1 as above), each
#   look[512]    9-bit lookahead: (code length << 8) | symbol, 0 where the code is longer than 9 bits
#   maxcode[32]  index = code length 1..16: the largest code of that length, -1 where there is none
#   valoff[32]   index = code length: (index of the length's first symbol in huffval) - (its first code)
#   huffval[256]
LOOK_BITS = 9
HT_LOOK, HT_MAXCODE, HT_VALOFF, HT_VAL, HT_WORDS = 0, 512, 544, 576, 832
SET_QUANT, SET_HUFF, SET_WORDS = 0, 128, 128 + 4 * 832

# columns of JpegClips.frames
F_CLIP, F_T, F_OFFSET, F_BYTES, F_SET, F_RESTART, F_LANE, F_LANES, F_COLS = 0, 1, 2, 3, 4, 5, 6, 7, 8
# bits of a frame's status word
STATUS_BAD_ROW, STATUS_OUT_OF_DATA, STATUS_BAD_CODE = 1, 2, 4

FrameInfo = collections.namedtuple('FrameInfo', ['height', 'width', 'components', 'qtables', 'htables', 'restart_interval', 'scan_start',
                                                 'scan_end'])
FrameInfo.__doc__ = """what parse() reads from the headers: components = [(id, h, v, tq, td, ta)]; qtables = {tq: (64,) int32, natural order};
htables = {(0 = DC / 1 = AC, id): (BITS (16,) int32, HUFFVAL (n,) uint8)}; buf[scan_start:scan_end] = the entropy-coded segment."""

_SOF_REASON = {0xC1: 'extended sequential DCT (SOF1)', 0xC2: 'progressive DCT (SOF2)', 0xC3: 'lossless (SOF3)',
               0xC5: 'differential sequential DCT (SOF5)', 0xC6: 'differential progressive DCT (SOF6)', 0xC7: 'differential lossless (SOF7)',
               0xC9: 'arithmetic coding (SOF9)', 0xCA: 'arithmetic coding (SOF10)', 0xCB: 'arithmetic coding (SOF11)',
               0xCD: 'arithmetic coding (SOF13)', 0xCE: 'arithmetic coding (SOF14)', 0xCF: 'arithmetic coding (SOF15)'}


def _bytes(buf):
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(buf, dtype=np.uint8)
    a = buf.numpy() if torch.is_tensor(buf) else np.asarray(buf)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError('a JPEG file as bytes or a flat uint8 array expected, got %s %s' % (a.dtype, a.shape))
    return a


def parse(buf):
    """the headers of one JPEG file (bytes or a flat uint8 array) up to the start of scan -> FrameInfo; ValueError with the reason for
    everything the decoder does not take"""
    a = _bytes(buf)
    n = a.size
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        raise ValueError('not a JPEG file: no SOI marker')
    pos = 2
    h = w = None
    comps, qt, ht, ri = None, {}, {}, 0

    def need(p, k):
        if p + k > n:
            raise ValueError('truncated header')

    while True:
        need(pos, 2)
        if a[pos] != 0xFF:
            raise ValueError('a marker expected at byte %d' % pos)
        while pos < n and a[pos] == 0xFF:          # fill bytes
            pos += 1
        need(pos, 1)
        m = int(a[pos])
        pos += 1
        if m == 0xD9:
            raise ValueError('end of image before a scan')
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        need(pos, 2)
        ln = (int(a[pos]) << 8) | int(a[pos + 1])
        if ln < 2:
            raise ValueError('bad segment length at byte %d' % pos)
        need(pos, ln)
        seg = a[pos + 2:pos + ln]
        if m in _SOF_REASON:
            raise ValueError('%s is not supported: baseline sequential DCT (SOF0) only' % _SOF_REASON[m])
        if m == 0xEE and seg.size >= 5 and bytes(seg[:5]) == b'Adobe':
            raise ValueError('an Adobe APP14 marker (CMYK / YCCK / RGB colour transforms) is not supported')
        if m == 0xC0:
            if comps is not None:
                raise ValueError('more than one frame header')
            if seg.size < 6:
                raise ValueError('truncated header')
            if seg[0] != 8:
                raise ValueError('%d-bit samples are not supported: 8 bit only' % int(seg[0]))
            h, w, nc = (int(seg[1]) << 8) | int(seg[2]), (int(seg[3]) << 8) | int(seg[4]), int(seg[5])
            if nc not in (1, 3):
                raise ValueError('%d components are not supported: 1 (gray) or 3 (YCbCr)' % nc)
            if h < 1 or w < 1:
                raise ValueError('an empty picture (%d x %d)' % (h, w))
            if seg.size < 6 + 3 * nc:
                raise ValueError('truncated header')
            comps = [[int(seg[6 + 3 * i]), int(seg[7 + 3 * i]) >> 4, int(seg[7 + 3 * i]) & 15, int(seg[8 + 3 * i]), None, None] for i in range(nc)]
        elif m == 0xDB:
            p = 0
            while p < seg.size:
                pq, tq = int(seg[p]) >> 4, int(seg[p]) & 15
                p += 1
                if pq > 1 or tq > 3 or p + 64 * (pq + 1) > seg.size:
                    raise ValueError('bad quantisation table segment')
                v = seg[p:p + 64 * (pq + 1)].astype(np.int32)
                if pq:
                    v = (v[0::2] << 8) | v[1::2]
                p += 64 * (pq + 1)
                t = np.zeros(64, dtype=np.int32)
                t[ZIGZAG] = v
                qt[tq] = t
        elif m == 0xC4:
            p = 0
            while p < seg.size:
                if p + 17 > seg.size:
                    raise ValueError('bad Huffman table segment')
                tc, th = int(seg[p]) >> 4, int(seg[p]) & 15
                bits = seg[p + 1:p + 17].astype(np.int32)
                cnt = int(bits.sum())
                if tc > 1 or th > 3 or cnt > 256 or p + 17 + cnt > seg.size:
                    raise ValueError('bad Huffman table segment')
                code = 0
                for l in range(16):                    # the code lengths must describe a prefix code
                    code = (code + int(bits[l])) << 1
                    if code > (2 << (l + 1)):
                        raise ValueError('bad Huffman table: too many codes of length %d' % (l + 1))
                ht[(tc, th)] = (bits, seg[p + 17:p + 17 + cnt].copy())
                p += 17 + cnt
        elif m == 0xDD:
            if seg.size < 2:
                raise ValueError('truncated header')
            ri = (int(seg[0]) << 8) | int(seg[1])
        elif m == 0xDA:
            if comps is None:
                raise ValueError('a scan before the frame header')
            ns = int(seg[0]) if seg.size else 0
            if ns != len(comps):
                raise ValueError('several scans (%d of %d components in the first) are not supported: one interleaved scan only' % (ns, len(comps)))
            if seg.size < 1 + 2 * ns + 3:
                raise ValueError('truncated header')
            for i in range(ns):
                cid, sel = int(seg[1 + 2 * i]), int(seg[2 + 2 * i])
                if cid != comps[i][0]:
                    raise ValueError('scan components out of frame order')
                comps[i][4], comps[i][5] = sel >> 4, sel & 15
            ss, se, ahl = int(seg[1 + 2 * ns]), int(seg[2 + 2 * ns]), int(seg[3 + 2 * ns])
            if ss != 0 or se != 63 or ahl != 0:
                raise ValueError('a spectral selection / successive approximation scan (progressive) is not supported')
            pos += ln
            break
        pos += ln
    if len(comps) == 3:
        if [c[0] for c in comps] == [82, 71, 66]:
            raise ValueError('an RGB JPEG (component ids R, G, B) is not supported: YCbCr only')
        if (comps[0][1], comps[0][2]) not in _SAMPLINGS or (comps[1][1], comps[1][2], comps[2][1], comps[2][2]) != (1, 1, 1, 1):
            raise ValueError('sampling factors %s are not supported: luma 1x1, 2x1 or 2x2 with chroma 1x1'
                             % ['%dx%d' % (c[1], c[2]) for c in comps])
        if comps[1][3:] != comps[2][3:]:
            raise ValueError('Cb and Cr with different tables are not supported')
    for c in comps:
        if c[3] not in qt:
            raise ValueError('missing quantisation table %d' % c[3])
        if (0, c[4]) not in ht or (1, c[5]) not in ht:
            raise ValueError('missing Huffman table (DC %d / AC %d)' % (c[4], c[5]))
    # the entropy-coded segment ends at the first marker that is neither a stuffed zero nor RSTn
    body = a[pos:]
    ff = np.flatnonzero(body[:-1] == 0xFF) if body.size > 1 else np.zeros(0, dtype=np.int64)
    nxt = body[ff + 1]
    stop = ff[(nxt != 0) & ((nxt & 0xF8) != 0xD0) & (nxt != 0xFF)]
    if stop.size == 0:
        raise ValueError('truncated file: no marker behind the scan')
    end = pos + int(stop[0])
    if a[end + 1] != 0xD9:
        raise ValueError('several scans are not supported: marker 0x%02X behind the first scan' % int(a[end + 1]))
    return FrameInfo(h, w, [tuple(c) for c in comps], qt, ht, ri, pos, end)


def sampling_code(info):
    return SAMP_444 if len(info.components) == 1 else _SAMPLINGS[(info.components[0][1], info.components[0][2])]


def block_grid(h, w, ncomp, samp):
    """(hs, vs, MCUs per row, MCU rows, blocks of the frame) as the kernels derive them from geom"""
    hs, vs = (1, 1) if ncomp == 1 else (samp >> 4, samp & 15)
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    return hs, vs, mx, my, mx * my * (hs * vs + (2 if ncomp == 3 else 0))


def _huff_lookup(bits, vals):
    """{(length, code): symbol} of a canonical Huffman table"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(int(bits[l - 1])):
            out[(l, code)] = int(vals[k])
            code += 1
            k += 1
        code <<= 1
    return out


class _BitReader(object):
    def __init__(self, a, pos, end):
        self.a, self.pos, self.end, self.acc, self.cnt = a, pos, end, 0, 0
        self.longest = self.zrl = 0            # the longest Huffman code and the ZRL symbols met (the fixtures' coverage flags)

    def bit(self):
        if self.cnt == 0:
            if self.pos >= self.end:
                raise ValueError('the entropy-coded segment ran out of data')
            b = int(self.a[self.pos])
            self.pos += 1
            if b == 0xFF:
                if self.pos < self.end and self.a[self.pos] == 0:
                    self.pos += 1
                else:
                    raise ValueError('a marker inside an interval of the entropy-coded segment')
            self.acc, self.cnt = b, 8
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((l, code))
            if s is not None:
                self.longest = max(self.longest, l)
                return s
        raise ValueError('an invalid Huffman code')

    def restart(self):
        self.cnt = 0
        if self.pos + 2 > self.end or self.a[self.pos] != 0xFF or (int(self.a[self.pos + 1]) & 0xF8) != 0xD0:
            raise ValueError('a restart marker expected at byte %d' % self.pos)
        self.pos += 2


def _extend(v, n):
    return v if n == 0 or v >= (1 << (n - 1)) else v - (1 << n) + 1


def decode_coefficients(buf, info=None, stats=None):
    """the quantised coefficients of every component, natural order: [(block rows, block columns, 64) int32]; stats: a dict that
    receives the longest Huffman code and the number of ZRL symbols of the scan"""
    a = _bytes(buf)
    info = info or parse(a)
    nc = len(info.components)
    hs, vs, mx, my, _ = block_grid(info.height, info.width, nc, sampling_code(info))
    fac = [(hs, vs)] + [(1, 1)] * (nc - 1)
    planes = [np.zeros((my * v, mx * h, 64), dtype=np.int32) for h, v in fac]
    dc = [_huff_lookup(*info.htables[(0, c[4])]) for c in info.components]
    ac = [_huff_lookup(*info.htables[(1, c[5])]) for c in info.components]
    rd = _BitReader(a, info.scan_start, info.scan_end)
    pred = [0] * nc
    for k in range(mx * my):
        if info.restart_interval and k and k % info.restart_interval == 0:
            rd.restart()
            pred = [0] * nc
        r, c = divmod(k, mx)
        for ci, (h, v) in enumerate(fac):
            for by in range(v):
                for bx in range(h):
                    blk = planes[ci][r * v + by, c * h + bx]
                    s = rd.symbol(dc[ci])
                    pred[ci] += _extend(rd.receive(s & 15), s & 15)
                    blk[0] = pred[ci]
                    i = 1
                    while i < 64:
                        rs = rd.symbol(ac[ci])
                        run, s = rs >> 4, rs & 15
                        if s == 0:
                            if run != 15:
                                break
                            i += 16
                            rd.zrl += 1
                            continue
                        i += run
                        if i > 63:
                            raise ValueError('a coefficient index beyond 63')
                        blk[ZIGZAG[i]] = _extend(rd.receive(s), s)
                        i += 1
    if stats is not None:
        stats.update(longest_code=rd.longest, zrl=rd.zrl)
    return planes


# ---- the 'sync' entropy mode, stated on the CPU (csrc/jpegdec.hip: jpeg_sub_decode, jpeg_entropy_sync_kernel) --------------------------------
# Huffman-coded data self-synchronises: a decoder started at an arbitrary byte falls into step with the true decode after a few symbols
# (Weissenberger & Schmidt, "Accelerating JPEG Decompression on GPUs").  A frame WITHOUT restart markers is cut into subsequences of
# `sub_bytes` raw bytes (stuffed FF 00 included), one decoder lane each.  A decoder state at a symbol boundary is (p, b, u, zz): the raw
# byte index and bit (0 = the most significant) of the next symbol's first bit -- a stuffed 00 never holds a bit --, the unit index inside
# the MCU and the zigzag index (0 = a DC symbol is due).  The byte behind a data byte FF is skipped whatever it is, bytes behind the
# segment's end read as 0: that makes a lane's decode a pure function of its entry state, which is all the rounds need to be exact.
SYNC_SUB_BYTES = 128                                   # the default subsequence size
SYNC_SUB_BYTES_RANGE = (16, 1024)                      # a multiple of 4: a symbol and its value (<= 31 bits, stuffing included) end inside the next subsequence
SYNC_MAX_SUBS = 1536                                   # the kernel's ceiling: 32 bytes of LDS per subsequence
SYNC_DEFAULT_MAX_SUBS = 192                            # 13,328 + 32 * 192 bytes of LDS: eight workgroups on a CU's 160 KiB
ENTROPY_MODES = ('interval', 'sync')


def entropy_mode(entropy=None):
    """None -> CFN_JPEG_ENTROPY (read at call time; unset = 'interval', today's lane per restart interval); anything but the two modes raises"""
    import os
    if entropy is None:
        entropy = os.environ.get('CFN_JPEG_ENTROPY') or 'interval'
    if entropy not in ENTROPY_MODES:
        raise ValueError("entropy: 'interval' or 'sync' expected, got %r" % (entropy,))
    return entropy


def check_sync_sizes(sub_bytes=None, max_subs=None):
    """(sub_bytes, max_subs) with the defaults filled in; ValueError naming the argument that is out of range"""
    sub_bytes = SYNC_SUB_BYTES if sub_bytes is None else sub_bytes
    max_subs = SYNC_DEFAULT_MAX_SUBS if max_subs is None else max_subs
    if not isinstance(sub_bytes, int) or isinstance(sub_bytes, bool) or sub_bytes % 4 or not SYNC_SUB_BYTES_RANGE[0] <= sub_bytes <= SYNC_SUB_BYTES_RANGE[1]:
        raise ValueError('sub_bytes: a multiple of 4 in [%d, %d] expected, got %r' % (SYNC_SUB_BYTES_RANGE + (sub_bytes,)))
    if not isinstance(max_subs, int) or isinstance(max_subs, bool) or not 1 <= max_subs <= SYNC_MAX_SUBS:
        raise ValueError('max_subs: an integer in [1, %d] expected, got %r' % (SYNC_MAX_SUBS, max_subs))
    return sub_bytes, max_subs


def _sync_sub(seg, end, dc, ac, comp, entry, limit, sink=None):
    """decode from `entry` = (p, b, u, zz) up to the first symbol whose first bit lies at or behind raw byte `limit` (or the segment's
    `end`) -> (exit state or None = invalid, blocks completed, [sum of DC differences per component]).  sink = [planes locator, next
    block, blocks of the frame, predictors]: the write pass, which also stops behind the frame's last block and raises on bad data."""
    p, b, u, zz = entry
    bpm = len(comp)
    blocks, dcsum = 0, [0, 0, 0]

    def bit():
        nonlocal p, b
        v = (int(seg[p]) >> (7 - b)) & 1 if p < end else 0
        b += 1
        if b == 8:
            b = 0
            p += 2 if p < end and seg[p] == 0xFF else 1
        return v

    def symbol(table):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | bit()
            s = table.get((l, code))
            if s is not None:
                return s
        return -1

    def receive(n):
        v = 0
        for _ in range(n):
            v = (v << 1) | bit()
        return _extend(v, n)

    def bad(why):
        if sink is not None:
            raise ValueError(why)
        return None, blocks, dcsum

    while p < limit and (sink is None or sink[1] < sink[2]):
        c = comp[u]
        if zz == 0:
            s = symbol(dc[c])
            if s < 0:
                return bad('an invalid Huffman code')
            d = receive(s & 15)
            dcsum[c] += d
            if sink is not None:
                sink[3][c] += d
                sink[0](sink[1])[0] = sink[3][c]
            zz = 1
            continue
        rs = symbol(ac[c])
        if rs < 0:
            return bad('an invalid Huffman code')
        run, s = rs >> 4, rs & 15
        if s == 0:
            zz = zz + 16 if run == 15 else 64          # ZRL, EOB
        else:
            zz += run
            if zz > 63:
                return bad('a coefficient index beyond 63')
            v = receive(s)
            if sink is not None:
                sink[0](sink[1])[ZIGZAG[zz]] = v
            zz += 1
        if zz >= 64:
            zz, u, blocks = 0, (u + 1) % bpm, blocks + 1
            if sink is not None:
                sink[1] += 1
    if sink is not None and (p > end or (p == end and b > 0)):
        raise ValueError('the entropy-coded segment ran out of data')
    return (p, b, u, zz), blocks, dcsum


def decode_coefficients_sync(buf, sub_bytes, max_rounds=None, stats=None):
    """decode_coefficients by the rounds of the 'sync' entropy mode, in plain Python over raw byte positions (frames without restart
    markers).  Round 0: every subsequence j is decoded, storing nothing, from its speculative start (byte j * sub_bytes, one on when the
    byte in front is FF; u = zz = 0), subsequence 0 from the true state.  Round k: j is decoded again from the exit state j - 1 had after
    round k - 1 (from its speculative start when that exit is invalid), unless that is the entry it last used.  After round k the first
    k + 1 exits are the true ones, so at most n rounds are needed; the rounds stop as soon as one changes no exit.  A scan of the block
    counts and DC sums gives every subsequence its first block and entry predictors, and a last pass from the true entries writes.
    stats receives subsequences, rounds (those in which something was decoded, round 0 included), entries [(p, b, u, zz)],
    first_blocks, predictors [[3]], invalid_exits (speculative decodes that ended in an invalid code) and stuffed_starts (subsequences
    whose first byte is a stuffed 00).  The reference of the CPU tests and of the kernel's intermediate values, NOT a fallback."""
    a = _bytes(buf)
    info = parse(a)
    if info.restart_interval:
        raise ValueError('the sync entropy mode takes frames without restart markers (restart interval %d)' % info.restart_interval)
    S, _ = check_sync_sizes(sub_bytes)
    nc = len(info.components)
    hs, vs, mx, my, nblocks = block_grid(info.height, info.width, nc, sampling_code(info))
    fac = [(hs, vs)] + [(1, 1)] * (nc - 1)
    planes = [np.zeros((my * v, mx * h, 64), dtype=np.int32) for h, v in fac]
    dc = [_huff_lookup(*info.htables[(0, c[4])]) for c in info.components]
    ac = [_huff_lookup(*info.htables[(1, c[5])]) for c in info.components]
    comp = [0] * (hs * vs) + list(range(1, nc))        # unit of the MCU -> component
    bpm = len(comp)
    seg = a[info.scan_start:info.scan_end]
    end = int(seg.size)
    n = max(1, -(-end // S))
    spec = [(0, 0, 0, 0)] + [(j * S + (1 if seg[j * S - 1] == 0xFF else 0), 0, 0, 0) for j in range(1, n)]
    limit = [min((j + 1) * S, end) for j in range(n)]

    def locate(k):
        m, u = divmod(k, bpm)
        r, c = divmod(m, mx)
        if u < hs * vs:
            return planes[0][r * vs + u // hs, c * hs + u % hs]
        return planes[comp[u]][r, c]

    rec = [_sync_sub(seg, end, dc, ac, comp, spec[j], limit[j]) for j in range(n)]                  # round 0
    used = list(spec)
    invalid = sum(1 for r in rec if r[0] is None)
    rounds = 1
    cap = n if max_rounds is None else min(n, max_rounds)
    while rounds < cap:
        prev = [r[0] for r in rec]
        todo = [j for j in range(1, n) if (prev[j - 1] or spec[j]) != used[j]]
        if not todo:
            break
        rounds += 1
        changed = False
        for j in todo:
            used[j] = prev[j - 1] or spec[j]
            new = _sync_sub(seg, end, dc, ac, comp, used[j], limit[j])
            invalid += 1 if new[0] is None else 0
            changed = changed or new[0] != rec[j][0]
            rec[j] = new
        if not changed:
            break
    first, preds, k, pr = [], [], 0, [0, 0, 0]
    for j in range(n):                                 # the exclusive scan
        first.append(k)
        preds.append(list(pr))
        k += rec[j][1]
        pr = [x + y for x, y in zip(pr, rec[j][2])]
    entries = [spec[0]] + [rec[j - 1][0] for j in range(1, n)]
    done = 0
    for j in range(n):                                 # the write pass
        if entries[j] is None or first[j] >= nblocks:
            continue
        sink = [locate, first[j], nblocks, list(preds[j])]
        _sync_sub(seg, end, dc, ac, comp, entries[j], limit[j], sink)
        done = max(done, sink[1])
    if done < nblocks:
        raise ValueError('the entropy-coded segment ran out of data')
    if stats is not None:
        stats.update(subsequences=n, rounds=rounds, entries=entries, first_blocks=first, predictors=preds, invalid_exits=invalid,
                     stuffed_starts=sum(1 for j in range(1, n) if spec[j][0] != j * S))
    return planes


def _idct_pass(i, shift):
    """one 1-D pass of libjpeg's jidctint over axis 0 of i (8, ...) int64"""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    rnd = 1 << (shift - 1)
    return np.stack([(x + rnd) >> shift for x in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)])


def idct_reference(coef, quant):
    """(..., 64) quantised coefficients, (64,) table -> (..., 8, 8) uint8 samples"""
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    x = np.moveaxis(_idct_pass(np.moveaxis(x, -2, 0), 11), 0, -2)          # down the columns
    x = np.moveaxis(_idct_pass(np.moveaxis(x, -1, 0), 18), 0, -1)          # along the rows
    return np.clip(x + 128, 0, 255).astype(np.uint8)


def _plane(blocks):
    br, bc = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(br * 8, bc * 8)


def _up_h(cs, lo, hi, shift):
    """horizontal triangle filter over (rows, dw) int64 -> (rows, 2 dw)"""
    left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
    right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    out = np.empty((cs.shape[0], 2 * cs.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * cs + left + lo) >> shift
    out[:, 1::2] = (3 * cs + right + hi) >> shift
    return out


def upsample_reference(p, H, W, samp):
    """libjpeg's "fancy" upsampling of one chroma plane (padded samples allowed behind the real ones) to H x W int64"""
    if samp == SAMP_444:
        return p[:H, :W].astype(np.int64)
    dw = (W + 1) // 2
    if samp == SAMP_422:
        return _up_h(p[:H, :dw].astype(np.int64), 1, 2, 2)[:, :W]
    dh = (H + 1) // 2
    q = p[:dh, :dw].astype(np.int64)
    up = np.concatenate([q[:1], q[:-1]])
    dn = np.concatenate([q[1:], q[-1:]])
    out = np.empty((2 * dh, 2 * dw), dtype=np.int64)
    out[0::2] = _up_h(3 * q + up, 8, 7, 4)
    out[1::2] = _up_h(3 * q + dn, 8, 7, 4)
    return out[:H, :W]


def decode_reference(buf):
    """(h, w, 3) uint8: what Image.open(buf).convert('RGB') gives, restated in numpy and plain Python (the tests' reference)"""
    a = _bytes(buf)
    info = parse(a)
    H, W, samp = info.height, info.width, sampling_code(info)
    planes = [_plane(idct_reference(c, info.qtables[comp[3]])) for c, comp in zip(decode_coefficients(a, info), info.components)]
    y = planes[0][:H, :W].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, axis=2)
    cb = upsample_reference(planes[1], H, W, samp) - 128
    cr = upsample_reference(planes[2], H, W, samp) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def _huff_words(bits, vals):
    t = np.zeros(HT_WORDS, dtype=np.int32)
    t[HT_MAXCODE:HT_MAXCODE + 32] = -1
    code, k = 0, 0
    for l in range(1, 17):
        t[HT_VALOFF + l] = k - code
        for _ in range(int(bits[l - 1])):
            if l <= LOOK_BITS:
                first = code << (LOOK_BITS - l)
                t[HT_LOOK + first:HT_LOOK + first + (1 << (LOOK_BITS - l))] = (l << 8) | int(vals[k])
            code += 1
            k += 1
        if bits[l - 1]:
            t[HT_MAXCODE + l] = code - 1
        code <<= 1
    t[HT_VAL:HT_VAL + len(vals)] = vals
    return t


def device_tables(info):
    """one table set (SET_WORDS int32) for the kernels, see the layout at the top of this file"""
    t = np.zeros(SET_WORDS, dtype=np.int32)
    slots = [info.components[0], info.components[-1]]          # a gray frame fills slot 1 with its only tables
    for s, c in enumerate(slots):
        t[SET_QUANT + 64 * s:SET_QUANT + 64 * (s + 1)] = info.qtables[c[3]]
        for cls in (0, 1):
            o = SET_HUFF + (2 * cls + s) * HT_WORDS
            t[o:o + HT_WORDS] = _huff_words(*info.htables[(cls, c[4 + cls])])
    return t


class JpegClips(collections.namedtuple('JpegClips', ['data', 'frames', 'tables', 'geom', 'lengths', 'box', 'dims'])):
    """A batch of clips whose frames are still baseline JPEG:

    * ``data``  flat uint8: every frame's entropy-coded segment (stuffed FF 00 bytes and RSTn markers kept), each 4-byte aligned and
      followed by at least 8 zero bytes;
    * ``frames`` (R, 8) int32, one row per frame, clip-major: clip index, t, data offset, byte length, table-set index, restart
      interval, first decoder lane, decoder lanes (= restart intervals of the frame: the entropy kernel runs one lane per interval);
    * ``tables`` (S, SET_WORDS) int32: the de-duplicated table sets of the batch (device_tables);
    * ``geom`` (B, n, 4) int32: h, w, sampling code, component count of every clip (one size and sampling per clip);
    * ``lengths`` (B, n) int32, ``box`` (B, n, 4) int32 = x1, y1, c, flip: as RawU8Clips has them;
    * ``dims`` HOST ints (Tmax, Hmax, Wmax, decoder lanes of the batch, most 8 x 8 blocks of a frame): what sizes the output, the
      workspace and the grids, so that decode() never reads the device for them.

    Stands for the RawU8Clips batch ``decode()`` makes; ``shape`` is that batch's logical shape (B, n, 3, Tmax, Hmax, Wmax).  A
    namedtuple, like RawU8Clips: staging and pinning rebuild it around the moved tensors."""
    __slots__ = ()

    @property
    def shape(self):
        return torch.Size(tuple(self.lengths.shape) + (3,) + tuple(int(d) for d in self.dims[:3]))

    @property
    def device(self):
        return self.data.device

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return len(self.shape)

    def _moved(self, fn):
        return JpegClips(*([fn(m) for m in self[:6]] + [self.dims]))

    def to(self, device, non_blocking=False):
        """move the six tensors to `device`; the element types are part of the format, so a dtype is refused"""
        if isinstance(device, torch.dtype) or not isinstance(device, (str, int, torch.device)):
            raise TypeError('JpegClips.to() takes a device: data stays uint8, the other members int32 (decode() makes the frames)')
        return self._moved(lambda m: m.to(device, non_blocking=non_blocking))

    def cuda(self, device=None, non_blocking=False):
        return self._moved(lambda m: m.cuda(device, non_blocking=non_blocking))

    def flatten_crops(self):
        """(B, n) clips -> (B * n); the rows of `frames` already count clips that way"""
        return JpegClips(self.data, self.frames, self.tables, self.geom.reshape(-1, 4), self.lengths.reshape(-1), self.box.reshape(-1, 4),
                         self.dims)

    def decode(self, out=None, status=None, entropy=None, sub_bytes=None):
        """the RawU8Clips batch these frames decode to, on the data's device and current stream (ops.jpeg_decode_u8; there is no CPU
        path).  out: preallocated frames (..., Tmax, Hmax, Wmax, 3), every byte of which is written; status: (R,) int32, one word per
        row of `frames`, 0 = decoded (check_status raises on anything else).  entropy: 'interval' or 'sync' (ops.jpeg_decode_u8; the
        same bytes), None = CFN_JPEG_ENTROPY, read at call time (unset: 'interval'); sub_bytes: the sync mode's subsequence size."""
        from . import ops
        mode = entropy_mode(entropy)
        if mode == 'sync':
            frames = ops.jpeg_decode_u8(self, out=out, status=status, entropy='sync', sub_bytes=sub_bytes)
        else:
            if sub_bytes is not None:
                raise ValueError("sub_bytes belongs to entropy='sync', got entropy=%r" % (mode,))
            frames = ops.jpeg_decode_u8(self, out=out, status=status)
        return RawU8Clips(frames.view(tuple(self.lengths.shape) + tuple(frames.shape[-4:])), self.lengths, self.box)


def check_status(status, frames, names=None, crops=1):
    """raise for the first frame whose status word is not 0 (ONE read-back of `status`); names: one per video of `crops` clips each, for
    the message"""
    st = status.cpu()
    bad = torch.nonzero(st).flatten()
    if bad.numel():
        row = frames[int(bad[0])].tolist()
        clip, t = row[F_CLIP], row[F_T]
        who = ''
        if names is not None and 0 <= clip // max(crops, 1) < len(names):
            who = ' of video %s' % (names[clip // max(crops, 1)],)
        bits = int(st[int(bad[0])])
        why = ', '.join(w for b, w in ((STATUS_BAD_ROW, 'inconsistent frame record'), (STATUS_OUT_OF_DATA, 'ran out of data or a restart marker is missing'),
                                       (STATUS_BAD_CODE, 'invalid Huffman code')) if bits & b)
        raise RuntimeError('JPEG decode failed for %d frame(s); first: frame %d of clip %d%s: %s' % (bad.numel(), t, clip, who, why))


def decode_checked(jpeg_clips, device, names=None, entropy=None):
    """JpegClips (on any device) -> the RawU8Clips batch on `device`, decoded there on the current stream; the status words are read back
    once and a frame that did not decode raises, naming its video (names: one per video of the batch).  entropy: as JpegClips.decode"""
    mode = entropy_mode(entropy)
    jc = jpeg_clips.to(device, non_blocking=True)
    status = torch.empty(jc.frames.shape[0], dtype=torch.int32, device=jc.device)
    raw = jc.decode(status=status, entropy=mode)
    check_status(status, jpeg_clips.frames, names, crops=jpeg_clips.lengths.shape[1] if jpeg_clips.lengths.dim() > 1 else 1)
    return raw


def collate_jpeg(samples):
    """[(clips, box)] -> JpegClips on the host.  clips: n lists of encoded frames (bytes), one list per clip of the sample, each of its
    own length; box (n, 4) int = x1, y1, c, flip.  A clip whose frames differ in size, sampling or component count raises."""
    if not samples:
        raise ValueError('an empty batch')
    segs, rows, geom, lengths, boxes, sets, set_rows = [], [], [], [], [], {}, []
    pos = lanes = blocks_max = 0
    n = None
    for smp in samples:
        if not isinstance(smp, (tuple, list)) or len(smp) != 2:
            raise ValueError('a JPEG clip member is a pair (n lists of encoded frames, box (n, 4) int)')
        clips, b = smp
        b = b if torch.is_tensor(b) else torch.from_numpy(np.asarray(b))
        if n is None:
            n = len(clips)
        if len(clips) != n:
            raise ValueError('the same number of clips per sample expected, got %d and %d' % (n, len(clips)))
        if b.is_floating_point() or b.dtype == torch.bool or tuple(b.shape) != (n, 4):
            raise ValueError('integer boxes of shape (n, 4) = x1, y1, c, flip expected for %d clips, got %s %s' % (n, b.dtype, tuple(b.shape)))
        b = b.to(torch.int32)
        geom.append([])
        lengths.append([])
        for ci, clip in enumerate(clips):
            g = None
            for t, f in enumerate(clip):
                a = _bytes(f)
                info = parse(a)
                gi = (info.height, info.width, sampling_code(info), len(info.components))
                if g is None:
                    g = gi
                elif gi != g:
                    raise ValueError('the frames of one clip must share size and sampling: frame %d is %s, frame 0 %s' % (t, gi, g))
                words = device_tables(info)
                key = words.tobytes()
                if key not in sets:
                    sets[key] = len(set_rows)
                    set_rows.append(words)
                _, _, mx, my, nblk = block_grid(gi[0], gi[1], gi[3], gi[2])
                ri = info.restart_interval
                ni = -(-(mx * my) // ri) if ri else 1
                seg = a[info.scan_start:info.scan_end]
                rows.append([len(lengths) * n - n + ci, t, pos, seg.size, sets[key], ri, lanes, ni])
                segs.append((pos, seg))
                pos += (seg.size + 8 + 3) & ~3
                lanes += ni
                blocks_max = max(blocks_max, nblk)
            if g is not None:
                x1, y1, cs, flip = b[ci].tolist()
                if cs <= 0 or x1 < 0 or y1 < 0 or x1 + cs > g[1] or y1 + cs > g[0] or flip not in (0, 1):
                    raise ValueError('box (x1, y1, c, flip) = %s does not lie inside the %d x %d frames' % ((x1, y1, cs, flip), g[0], g[1]))
            geom[-1].append(list(g) if g is not None else [0, 0, 0, 0])
            lengths[-1].append(len(clip))
        boxes.append(b)
    if not rows:
        raise ValueError('a batch without a single frame')
    data = np.zeros(pos, dtype=np.uint8)
    for p, seg in segs:
        data[p:p + seg.size] = seg
    geom = torch.tensor(geom, dtype=torch.int32)
    lengths = torch.tensor(lengths, dtype=torch.int32)
    dims = (int(lengths.max()), int(geom[..., 0].max()), int(geom[..., 1].max()), lanes, blocks_max)
    return JpegClips(torch.from_numpy(data), torch.tensor(rows, dtype=torch.int32), torch.from_numpy(np.stack(set_rows)), geom, lengths,
                     torch.stack(boxes), dims)
