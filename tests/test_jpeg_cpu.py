"""CPU: the host side of the GPU JPEG decoder (cfn_hip/jpegdec.py) -- the header parser and its refusals, the numpy statement of the
decoder's arithmetic against the pixels PIL decoded (0 differing bytes: the acceptance level of the GPU kernels as well), the structure
of the collated batch, and the ABI / operator registration of the entry points (csrc/jpegdec.hip, csrc/capi.hip)."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected_fields(name):
    """(h, w, components, sampling, restart interval in MCUs) from the case's name"""
    from cfn_hip import jpegdec
    size, kind, tag = name.split('_')
    h, w = (int(v) for v in size.split('x'))
    if kind == 'gray':
        return h, w, 1, jpegdec.SAMP_444, 0
    samp = {'420': jpegdec.SAMP_420, '422': jpegdec.SAMP_422, '444': jpegdec.SAMP_444}[tag[:3]]
    ri = 0
    if tag.endswith('rst3'):                     # restart_marker_blocks=3: three MCU rows' worth is not it -- PIL counts MCUs
        ri = 3
    return h, w, 3, samp, ri


def test_fixture_coverage():
    cov = jc.coverage()
    assert cov['zrl'] >= 1 and cov['coef63'] >= 1 and cov['stuffed'] >= 1 and cov['longest_code'] >= 10 and cov['restart'] >= 1, cov
    assert len(jc.names()) >= 60


@pytest.mark.parametrize('name', jc.names())
def test_parse_fields(name):
    from cfn_hip import jpegdec
    buf = jc.jpg(name)
    info = jpegdec.parse(buf)
    h, w, nc, samp, ri = _expected_fields(name)
    assert (info.height, info.width, len(info.components)) == (h, w, nc)
    assert jpegdec.sampling_code(info) == samp
    assert info.restart_interval == ri
    assert (h, w) == jc.pixels(name).shape[:2]
    for cid, hs, vs, tq, td, ta in info.components:
        q = info.qtables[tq]
        assert q.shape == (64,) and q.dtype == np.int32 and int(q.min()) >= 1 and int(q.max()) <= 255
        for cls, sel in ((0, td), (1, ta)):
            bits, vals = info.htables[(cls, sel)]
            assert bits.shape == (16,) and int(bits.sum()) == len(vals) >= 1
    if nc == 3:
        assert [c[1:3] for c in info.components[1:]] == [(1, 1), (1, 1)]
        # a quantisation table in natural order: the libjpeg tables grow towards high frequencies along the first row as well as the first column
        q = info.qtables[info.components[0][3]].reshape(8, 8)
        assert int(q[0, 7]) >= int(q[0, 0]) and int(q[7, 0]) >= int(q[0, 0])
    raw = np.frombuffer(buf, dtype=np.uint8)
    assert bytes(raw[info.scan_end:info.scan_end + 2]) == b'\xff\xd9' and info.scan_end + 2 == len(buf)          # the segment ends at EOI
    assert raw[info.scan_start - 3] == 0 and raw[info.scan_start - 2] == 63 and raw[info.scan_start - 1] == 0    # ... and starts behind Ss, Se, Ah/Al
    assert jpegdec.parse(raw).scan_end == info.scan_end                                                          # bytes or a uint8 array


@pytest.mark.parametrize('name', jc.names())
def test_decode_reference_equals_pil(name):
    from cfn_hip import jpegdec
    got = jpegdec.decode_reference(jc.jpg(name))
    want = jc.pixels(name)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert int((got != want).sum()) == 0


def test_refusals():
    from cfn_hip import jpegdec
    with pytest.raises(ValueError, match='progressive'):
        jpegdec.parse(jc.refused('progressive'))
    with pytest.raises(ValueError, match='Adobe|4 components'):
        jpegdec.parse(jc.refused('cmyk'))
    good = bytearray(jc.jpg('16x16_smooth_420q75'))
    info = jpegdec.parse(bytes(good))
    with pytest.raises(ValueError, match='truncated'):
        jpegdec.parse(bytes(good[:info.scan_start - 20]))
    with pytest.raises(ValueError, match='SOI'):
        jpegdec.parse(b'\x89PNG' + bytes(good))
    sof = bytes(good).index(b'\xff\xc0')

    def patched(off, val, marker=None):
        b = bytearray(good)
        if marker is not None:
            b[sof + 1] = marker
        b[sof + off] = val
        return bytes(b)
    with pytest.raises(ValueError, match='12-bit'):
        jpegdec.parse(patched(4, 12))
    with pytest.raises(ValueError, match='arithmetic'):
        jpegdec.parse(patched(4, 8, marker=0xC9))
    with pytest.raises(ValueError, match='sampling'):
        jpegdec.parse(patched(11, 0x41))                       # luma 4x1
    with pytest.raises(ValueError, match='4 components'):
        jpegdec.parse(patched(9, 4))
    dht = bytes(good).index(b'\xff\xc4')
    b = bytearray(good)
    b[dht + 1] = 0xFE                                          # the first Huffman table segment becomes a comment: a table is missing
    with pytest.raises(ValueError, match='missing Huffman'):
        jpegdec.parse(bytes(b))
    sos = bytes(good).index(b'\xff\xda')
    b = bytearray(good)
    b[sos + 4] = 1                                             # the scan names one component of three
    with pytest.raises(ValueError, match='several scans'):
        jpegdec.parse(bytes(b))


def test_collate_structure():
    import collate
    from cfn_hip import jpegdec
    from cfn_hip.jpegdec import JpegClips
    label = [torch.zeros(157, 5), torch.ones(157, 3)]
    batch = [(s, lb, 'vid%d' % i) for i, (s, lb) in enumerate(zip(jc.jpeg_samples(jc.RAGGED, jc.RAGGED_BOX), label))]
    clips, labels, masks, vids = collate.fine_collate_jpeg(batch)
    assert isinstance(clips, JpegClips) and vids == ['vid0', 'vid1'] and tuple(labels.shape) == (2, 157, 5) and tuple(masks.shape) == (2, 5)
    assert tuple(clips.shape) == (2, 2, 3, 3, 48, 64) and clips.dim() == 6 and clips.size(4) == 48 and clips.device.type == 'cpu'
    assert clips.lengths.tolist() == [[3, 0], [2, 1]] and clips.lengths.dtype == torch.int32
    assert clips.box.tolist() == jc.RAGGED_BOX and clips.box.dtype == torch.int32
    assert clips.geom.tolist() == [[[48, 64, jpegdec.SAMP_420, 3], [0, 0, 0, 0]], [[33, 31, jpegdec.SAMP_444, 1], [9, 17, jpegdec.SAMP_422, 3]]]
    fr = clips.frames
    assert fr.dtype == torch.int32 and tuple(fr.shape) == (6, jpegdec.F_COLS)
    assert fr[:, jpegdec.F_CLIP].tolist() == [0, 0, 0, 2, 2, 3] and fr[:, jpegdec.F_T].tolist() == [0, 1, 2, 0, 1, 0]
    data = clips.data.numpy()
    flat = [n for video in jc.RAGGED for clip in video for n in clip]
    end_prev = 0
    for row, name in zip(fr.tolist(), flat):
        off, nb = row[jpegdec.F_OFFSET], row[jpegdec.F_BYTES]
        info = jpegdec.parse(jc.jpg(name))
        assert off % 4 == 0 and off >= end_prev
        assert bytes(data[off:off + nb]) == jc.jpg(name)[info.scan_start:info.scan_end]
        assert not data[off + nb:off + nb + 8].any() and off + nb + 8 <= data.size           # >= 8 zero bytes behind the segment
        assert not data[end_prev:off].any()
        assert row[jpegdec.F_RESTART] == info.restart_interval
        end_prev = off + nb
    # the two gray frames are the same file: one table set; the restart-marker frame shares the default tables of no other frame here
    assert fr[3, jpegdec.F_SET] == fr[4, jpegdec.F_SET] and tuple(clips.tables.shape) == (int(fr[:, jpegdec.F_SET].max()) + 1, jpegdec.SET_WORDS)
    assert len(set(fr[:3, jpegdec.F_SET].tolist())) == 3                                       # quality 75, 100 and 10: three sets
    # decoder lanes: one per restart interval (48 x 64 at 4:2:0 = 12 MCUs, 3 per interval), contiguous
    assert fr[:, jpegdec.F_LANES].tolist() == [4, 1, 1, 1, 1, 1]
    assert fr[:, jpegdec.F_LANE].tolist() == [0, 4, 5, 6, 7, 8]
    assert clips.dims == (3, 48, 64, 9, 12 * 6)                   # 12 MCUs of 4 luma + 2 chroma blocks
    # two frames written by one encoder run share their set
    two = jpegdec.collate_jpeg([([[jc.jpg('37x50_smooth_420q75'), jc.jpg('37x50_smooth_420q75rst3')]], torch.tensor([[0, 0, 37, 0]]))])
    assert two.frames[:, jpegdec.F_SET].tolist() == [0, 0] and two.tables.shape[0] == 1
    # flatten_crops
    fl = clips.flatten_crops()
    assert tuple(fl.shape) == (4, 3, 3, 48, 64) and fl.lengths.tolist() == [3, 0, 2, 1] and tuple(fl.box.shape) == (4, 4) and tuple(fl.geom.shape) == (4, 4)
    # a clip that mixes sizes, or sampling types, raises
    with pytest.raises(ValueError, match='share size'):
        jpegdec.collate_jpeg([([[jc.jpg('33x31_smooth_420q75'), jc.jpg('37x50_smooth_420q75')]], torch.tensor([[0, 0, 31, 0]]))])
    with pytest.raises(ValueError, match='share size'):
        jpegdec.collate_jpeg([([[jc.jpg('33x31_smooth_420q75'), jc.jpg('33x31_smooth_444q90')]], torch.tensor([[0, 0, 31, 0]]))])
    with pytest.raises(ValueError, match='box'):
        jpegdec.collate_jpeg([([[jc.jpg('33x31_smooth_420q75')]], torch.tensor([[0, 0, 32, 0]]))])
    with pytest.raises(ValueError):
        jpegdec.collate_jpeg([([[jc.refused('progressive')]], torch.tensor([[0, 0, 31, 0]]))])


def test_coarse_collate_jpeg_members(tmp_path):
    """the coarse builders: member 0 is the JpegClips batch, the rest is what coarse_collate_raw_u8 builds from the decoded samples"""
    import collate
    from cfn_hip.jpegdec import JpegClips
    g = torch.Generator().manual_seed(3)
    feats = [{k: torch.randn(c, t, 7, 7, generator=g) for k, c in (('a', 8), ('b', 16))} for t in (5, 9)]
    rest = [(torch.rand(157, 4 + i, generator=g), feats[i], torch.tensor([0, 8, 30, 1]), 'v%d' % i, 12.5 + i) for i in range(2)]
    jb = collate.coarse_collate_jpeg([(s,) + r for s, r in zip(jc.jpeg_samples(jc.MIXED, jc.MIXED_BOX), rest)])
    rb = collate.coarse_collate_raw_u8([(s,) + r for s, r in zip(jc.raw_samples(jc.MIXED, jc.MIXED_BOX), rest)])
    assert isinstance(jb[0], JpegClips) and len(jb) == len(rb) == 8
    assert tuple(jb[0].shape) == tuple(rb[0].shape) and torch.equal(jb[0].lengths, rb[0].lengths) and torch.equal(jb[0].box, rb[0].box)
    for a, b in zip(jb[1:], rb[1:]):
        if isinstance(a, dict):
            assert all(torch.equal(a[k], b[k]) for k in b)
        elif torch.is_tensor(a):
            assert torch.equal(a, b)
        else:
            assert a == b
    assert callable(collate.coarse_collate_packed_jpeg)


def test_jpegclips_to_and_rebuild():
    from cfn_hip import jpegdec, staging
    clips = jpegdec.collate_jpeg(jc.jpeg_samples(jc.MIXED, jc.MIXED_BOX))
    with pytest.raises(TypeError):
        clips.to(torch.float32)
    with pytest.raises(TypeError):
        clips.to(None)
    same = clips.to('cpu')
    assert isinstance(same, jpegdec.JpegClips) and same.dims == clips.dims and all(torch.equal(a, b) for a, b in zip(same[:6], clips[:6]))
    moved = staging._map_tensors(clips, lambda t: t.clone())          # what the stager and pinning do with a namedtuple
    assert isinstance(moved, jpegdec.JpegClips) and moved.dims == clips.dims and torch.equal(moved.data, clips.data)
    from torch.utils.data._utils.collate import default_collate  # noqa: F401  (DataLoader's pinning walks namedtuples the same way)
    with pytest.raises(RuntimeError):
        clips.decode()                                               # host tensors: there is no CPU path


def test_device_tables_decode_every_code():
    """the lookahead / maxcode / valoff form of a Huffman table returns the symbol of every code of the table"""
    from cfn_hip import jpegdec
    for name in ('48x64_smooth_420q50opt', '48x64_noise_420q100', '33x31_gray_q85'):
        info = jpegdec.parse(jc.jpg(name))
        words = jpegdec.device_tables(info)
        assert words.shape == (jpegdec.SET_WORDS,) and words.dtype == np.int32
        slots = [info.components[0], info.components[-1]]
        for s, comp in enumerate(slots):
            assert np.array_equal(words[64 * s:64 * s + 64], info.qtables[comp[3]])
            for cls in (0, 1):
                ht = words[jpegdec.SET_HUFF + (2 * cls + s) * jpegdec.HT_WORDS:][:jpegdec.HT_WORDS]
                for (length, code), sym in jpegdec._huff_lookup(*info.htables[(cls, comp[4 + cls])]).items():
                    peek = code << (16 - length)                  # the code followed by zero bits
                    e = int(ht[jpegdec.HT_LOOK + (peek >> (16 - jpegdec.LOOK_BITS))])
                    if length <= jpegdec.LOOK_BITS:
                        assert e == (length << 8) | sym
                    else:
                        assert e == 0
                        hit = [l for l in range(jpegdec.LOOK_BITS + 1, 17) if (peek >> (16 - l)) <= ht[jpegdec.HT_MAXCODE + l]]
                        assert hit and hit[0] == length
                        assert int(ht[jpegdec.HT_VAL + ((int(ht[jpegdec.HT_VALOFF + length]) + code) & 255)]) == sym


def test_operator_tuples_and_header():
    import cfn_hip
    from cfn_hip import torchlib
    assert torchlib.DECODE_OPERATORS == ('jpeg_decode_u8',)
    others = (torchlib.OPERATORS, torchlib.INPUT_OPERATORS, torchlib.AUGMENT_OPERATORS, torchlib.METRIC_OPERATORS, torchlib.FEATURE_OPERATORS)
    for tup in others:
        assert not set(torchlib.DECODE_OPERATORS) & set(tup)
    assert hasattr(torch.ops.cfn, 'jpeg_decode_u8')
    protos = cfn_hip.header_prototypes()
    assert 'cfn_jpeg_workspace_bytes' in protos and 'cfn_jpeg_decode_u8' in protos
    ret, at, dt = protos['cfn_jpeg_decode_u8']
    assert len(at) == 19 and dt[0] == torch.uint8 and dt[1] == torch.int32 and dt[5] == torch.uint8 and dt[6] == torch.int32
    assert len(protos['cfn_jpeg_workspace_bytes'][1]) == 4
    with open(os.path.join(ROOT, 'include', 'cfn_hip.h')) as fh:
        assert 'pil_loader' in fh.read()
    lib = cfn_hip.load()
    assert lib.cfn_jpeg_workspace_bytes(0, 1, 1, 1) == -1
    n = lib.cfn_jpeg_workspace_bytes(6, 12, 9, 36)
    assert n >= 6 * 36 * (128 + 64) + 2 * 9 * 4 + 12 * 4 and n % 256 == 0
