"""CPU: the packed 16-bit fine-feature format (cfn_hip/featpack.py) -- the record file, the conversion of an fp32 five-file store, the
packed collate builders against coarse_collate on the same samples, the batch type through pinning and staging, and the ABI / operator
registration of the two kernels' entry points (csrc/featpack.hip).  Everything here is exact: comparisons are torch.equal."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

CH = (8, 16, 24, 8, 40)                  # small channel counts (multiples of 8)
REAL = (24, 48, 96, 192, 432)
DTYPES = [torch.float16, torch.bfloat16]


def _feat(seed, frames, channels=CH):
    """post-ReLU-like maps {k: (C_k, T', 7, 7)} fp32 with values no 16-bit format holds exactly"""
    from cfn_hip import featpack
    g = torch.Generator().manual_seed(seed)
    return {k: torch.relu(torch.randn(c, frames, 7, 7, generator=g)) * 3.0 for k, c in zip(featpack.FEAT_KEYS, channels)}


def _rounded(feat, dt):
    return {k: v.to(dt).float() for k, v in feat.items()}


def _record(tmp_path, name, feat, dt):
    from cfn_hip import featpack
    payload, frames, channels = featpack.pack_reference(feat, dt)
    return featpack.open_record(featpack.write_record(featpack.record_path(str(tmp_path), name), payload, dt, frames, channels))


@pytest.mark.parametrize('dt', DTYPES)
def test_record_round_trip(tmp_path, dt):
    from cfn_hip import featpack
    feat = _feat(1, 13)
    rec = _record(tmp_path, 'vidA', feat, dt)
    assert rec.path.endswith(os.path.join('packed', 'vidA.cff'))
    assert rec.dtype == dt and rec.frames == 13 and rec.channels == CH
    assert os.path.getsize(rec.path) == 64 + 2 * 13 * sum(CH) * 49
    want = _rounded(feat, dt)
    got = rec.to_dict()
    assert list(got) == list(featpack.FEAT_KEYS)
    for k in want:
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    # block(k, t_max): the time-major (t, C_k, 49) view, a prefix of the block; by index or by name
    for i, k in enumerate(featpack.FEAT_KEYS):
        blk = rec.block(i, 5)
        assert blk.dtype == dt and tuple(blk.shape) == (5, CH[i], 49)
        assert torch.equal(blk.float(), want[k][:, :5].reshape(CH[i], 5, 49).permute(1, 0, 2))
        assert tuple(rec.block(k).shape) == (13, CH[i], 49) and tuple(rec.block(k, 200).shape) == (13, CH[i], 49)
    # the header, byte for byte
    head = open(rec.path, 'rb').read(64)
    assert head[:8] == b'CFNFEAT1' and struct.unpack('<4I', head[8:24]) == (1 if dt == torch.float16 else 2, 13, 49, 5)
    assert struct.unpack('<5I', head[24:44]) == CH and head[44:] == b'\0' * 20
    # a payload handed over as bytes gives the same file
    payload, frames, channels = featpack.pack_reference(feat, dt)
    other = featpack.write_record(str(tmp_path / 'raw.cff'), payload.view(torch.int16).numpy().tobytes(), dt, frames, channels)
    assert open(other, 'rb').read() == open(rec.path, 'rb').read()


def test_bad_records_raise_value_error_naming_the_file(tmp_path):
    from cfn_hip import featpack
    rec = _record(tmp_path, 'good', _feat(2, 4), torch.float16)
    raw = open(rec.path, 'rb').read()
    cases = {'magic': b'CFNFEAT0' + raw[8:], 'dtype': raw[:8] + struct.pack('<I', 3) + raw[12:], 'short': raw[:-2], 'long': raw + b'\0\0',
             'header': raw[:40], 'channels': raw[:24] + struct.pack('<I', 12) + raw[28:]}
    for name, data in cases.items():
        p = str(tmp_path / (name + '.cff'))
        with open(p, 'wb') as fh:
            fh.write(data)
        with pytest.raises(ValueError, match=name + '.cff'):
            featpack.open_record(p)
    with pytest.raises(ValueError, match='nothing.cff'):
        featpack.open_record(str(tmp_path / 'nothing.cff'))
    payload, frames, channels = featpack.pack_reference(_feat(2, 4), torch.float16)
    with pytest.raises(ValueError):                       # channel counts must be multiples of 8
        featpack.write_record(str(tmp_path / 'x.cff'), payload, torch.float16, frames, (8, 16, 24, 12, 36))
    with pytest.raises(ValueError):                       # the payload is not of the stated size
        featpack.write_record(str(tmp_path / 'x.cff'), payload[:-1], torch.float16, frames, channels)
    with pytest.raises(ValueError):                       # ... or type
        featpack.write_record(str(tmp_path / 'x.cff'), payload, torch.bfloat16, frames, channels)
    with pytest.raises(ValueError):
        featpack.write_record(str(tmp_path / 'x.cff'), payload, torch.float32, frames, channels)


@pytest.mark.parametrize('dt', ['fp16', 'bf16'])
def test_convert_dir_of_a_five_file_store(tmp_path, dt):
    """the layout extract_fineFEAT.extract writes: <dir>/<key>/<vid> = one torch.save'd fp32 tensor (1, C_k, T', 7, 7)"""
    from cfn_hip import featpack
    src, dst = str(tmp_path / 'f32'), str(tmp_path / 'p16')
    feats = {'vid_a': _feat(3, 6, REAL), 'vid_b': _feat(4, 1, REAL)}
    for vid, feat in feats.items():
        for k, v in feat.items():
            os.makedirs(os.path.join(src, k), exist_ok=True)
            torch.save(v.unsqueeze(0), os.path.join(src, k, vid))
    assert featpack.convert_dir(src, dst, dt) == 2
    tdt = featpack.feat_dtype(dt)
    for vid, feat in feats.items():
        rec = featpack.open_record(featpack.record_path(dst, vid))
        assert rec.dtype == tdt and rec.channels == REAL and rec.frames == feat['layer1'].shape[1]
        got, want = rec.to_dict(), _rounded(feat, tdt)
        assert all(torch.equal(got[k], want[k]) for k in want)


LENGTHS = (1, 5, 13, 128, 150)             # the last one is truncated at the cap


@pytest.fixture(scope='module')
def packed_samples(tmp_path_factory):
    """five coarse samples whose feature member is a Record, and the same samples with the record's to_dict()"""
    d = tmp_path_factory.mktemp('packed_samples')
    g = torch.Generator().manual_seed(7)
    out = {}
    for dt in DTYPES:
        packed, plain = [], []
        for i, n in enumerate(LENGTHS):
            rec = _record(d / str(dt), 'v%d' % i, _feat(10 + i, n), dt)
            T = 4 + i
            rest = (torch.randn(1, 3, T, 8, 8, generator=g), (torch.rand(157, T * 10, generator=g) < 0.1).float())
            tail = (torch.tensor([i, T, n, 1]), 'v%d' % i, 10.0 + i)
            packed.append(rest + (rec,) + tail)
            plain.append(rest + (rec.to_dict(),) + tail)
        out[dt] = (packed, plain)
    return out


@pytest.mark.parametrize('dt', DTYPES)
def test_packed_collate_equals_coarse_collate(packed_samples, dt):
    import collate
    from cfn_hip.featpack import PackedFeats
    from cfn_hip.u8clips import U8Clips, RawU8Clips
    packed, plain = packed_samples[dt]
    got, ref = collate.coarse_collate_packed(packed), collate.coarse_collate(plain)
    assert len(got) == len(ref) == 8
    pf = got[3]
    assert isinstance(pf, PackedFeats) and pf.data.dtype == dt and pf.data.dim() == 1 and pf.channels == CH
    assert pf.offsets.dtype == torch.int64 and tuple(pf.offsets.shape) == (5, 5) and not bool((pf.offsets % 8).any())
    assert pf.lengths.dtype == torch.int32 and pf.lengths.tolist() == [1, 5, 13, 128, 128]
    assert isinstance(pf.t_max, int) and pf.t_max == 128
    assert pf.data.numel() == sum(pf.lengths.tolist()) * sum(CH) * 49                   # unpadded: nothing but the live frames
    un = pf.unpack_reference()
    assert list(un) == list(ref[3])
    for k in ref[3]:
        assert un[k].dtype == torch.float32 and un[k].shape == ref[3][k].shape and torch.equal(un[k], ref[3][k]), k
    for i in (0, 1, 2, 4, 5, 7):
        assert torch.equal(got[i], ref[i]), i
    assert got[6] == ref[6]
    # a smaller cap; a batch whose longest video is shorter than the cap
    got, ref = collate.coarse_collate_packed(packed, cap=7), collate.coarse_collate(plain, cap=7)
    assert got[3].t_max == 7 and got[3].lengths.tolist() == [1, 5, 7, 7, 7] and torch.equal(got[4], ref[4])
    assert all(torch.equal(got[3].unpack_reference()[k], ref[3][k]) for k in ref[3])
    got, ref = collate.coarse_collate_packed(packed[:3]), collate.coarse_collate(plain[:3])
    assert got[3].t_max == 13 and torch.equal(got[4], ref[4]) and all(torch.equal(got[3].unpack_reference()[k], ref[3][k]) for k in ref[3])
    # the uint8 spellings: the clip member changes, the rest is the same
    u8 = lambda smp: [(torch.zeros(1, s[0].shape[2], 8, 8, 3, dtype=torch.uint8),) + s[1:] for s in smp]
    g8, r8 = collate.coarse_collate_packed_u8(u8(packed)), collate.coarse_collate_u8(u8(plain))
    assert isinstance(g8[0], U8Clips) and torch.equal(g8[0].frames, r8[0].frames) and torch.equal(g8[4], r8[4])
    assert isinstance(g8[3], PackedFeats) and torch.equal(g8[3].data.view(torch.int16), pf.data.view(torch.int16))
    raw = lambda smp: [((torch.zeros(1, s[0].shape[2], 8, 8, 3, dtype=torch.uint8), torch.tensor([[0, 0, 8, 0]])),) + s[1:] for s in smp]
    gr = collate.coarse_collate_packed_raw_u8(raw(packed))
    assert isinstance(gr[0], RawU8Clips) and isinstance(gr[3], PackedFeats) and torch.equal(gr[3].offsets, pf.offsets)
    with pytest.raises(ValueError):                       # a dict where a Record belongs
        collate.coarse_collate_packed(plain)
    other = packed_samples[DTYPES[1] if dt == DTYPES[0] else DTYPES[0]][0]
    with pytest.raises(ValueError):                       # fp16 and bf16 records in one batch
        collate.coarse_collate_packed([packed[0], other[1]])


def test_packed_feats_batch_type(packed_samples):
    import collate
    from cfn_hip import staging
    from cfn_hip.featpack import PackedFeats
    pf = collate.coarse_collate_packed(packed_samples[torch.float16][0][:3])[3]
    assert PackedFeats._fields == ('data', 'offsets', 'lengths', 'channels', 't_max')
    assert pf.device.type == 'cpu' and pf.dtype == torch.float16 and pf.batch == 3
    with pytest.raises(TypeError):
        pf.to(torch.float32)
    with pytest.raises(TypeError):
        pf.to(None)
    moved = pf.to('cpu')
    assert isinstance(moved, PackedFeats) and torch.equal(moved.data, pf.data) and moved.channels == pf.channels and moved.t_max == pf.t_max
    # staging rebuilds it around the mapped tensors; ints and the channel tuple pass through
    seen = []

    def fn(t):
        seen.append(t)
        return t.clone()
    mapped = staging._map_tensors([pf, {'x': pf.lengths}], fn)
    assert isinstance(mapped[0], PackedFeats) and len(seen) == 4 and mapped[0].data is not pf.data
    assert torch.equal(mapped[0].data, pf.data) and torch.equal(mapped[0].offsets, pf.offsets) and torch.equal(mapped[0].lengths, pf.lengths)
    assert tuple(mapped[0].channels) == CH and mapped[0].t_max == 13
    assert all(torch.equal(a, b) for a, b in zip(mapped[0].unpack_reference().values(), pf.unpack_reference().values()))
    # DataLoader pinning walks namedtuples the same way
    from torch.utils.data._utils.pin_memory import pin_memory
    try:
        pinned = pin_memory(pf)
    except RuntimeError:                                   # no accelerator runtime to pin with: the walk itself is what is checked below
        pinned = None
    if pinned is not None:
        assert isinstance(pinned, PackedFeats) and torch.equal(pinned.data, pf.data) and tuple(pinned.channels) == CH and pinned.t_max == 13
    with pytest.raises(RuntimeError):
        pf.unpack()                                        # host tensors: the kernel runs on the GPU only


def test_abi_prototypes_and_argument_checks():
    import cfn_hip
    protos = cfn_hip.header_prototypes()
    for sfx, dt in (('_f16', torch.float16), ('_bf16', torch.bfloat16)):
        ret, at, dts = protos['cfn_feat_unpack' + sfx]
        assert ret is ctypes.c_int and len(at) == 17 and at[-1] is ctypes.c_void_p and at[-2] is ctypes.c_long
        assert dts[:8] == [dt, torch.int64, torch.int32] + [torch.float32] * 5
        ret, at, dts = protos['cfn_feat_pack' + sfx]
        assert ret is ctypes.c_int and len(at) == 13 and dts[:6] == [torch.float32] * 5 + [dt]
    lib = cfn_hip.load()
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr() + (-buf.data_ptr()) % 16          # (argument checks run before any launch: host pointers are never dereferenced)
    ch = (8, 16, 24, 8, 40)
    for f in (lib.cfn_feat_unpack_f16, lib.cfn_feat_unpack_bf16):
        for i in range(8):
            a = [p] * 8
            a[i] = None
            assert f(*a, 1, 1, *ch, 64, None) == 1 and 'null' in cfn_hip.last_error(), i
        assert f(*[p] * 8, 0, 1, *ch, 64, None) == 1 and 'shape' in cfn_hip.last_error()
        assert f(*[p] * 8, 1, 0, *ch, 64, None) == 1 and 'shape' in cfn_hip.last_error()
        for bad in ((8, 16, 24, 12, 40), (0, 16, 24, 8, 40), (8, 16, 24, 8, -8)):
            assert f(*[p] * 8, 1, 1, *bad, 64, None) == 1 and 'multiples of 8' in cfn_hip.last_error(), bad
        assert f(p + 2, *[p] * 7, 1, 1, *ch, 64, None) == 1 and '16-byte' in cfn_hip.last_error()
    for f in (lib.cfn_feat_pack_f16, lib.cfn_feat_pack_bf16):
        for i in range(6):
            a = [p] * 6
            a[i] = None
            assert f(*a, 1, *ch, None) == 1 and 'null' in cfn_hip.last_error(), i
        assert f(*[p] * 6, 0, *ch, None) == 1 and 'shape' in cfn_hip.last_error()
        assert f(*[p] * 6, 1, 8, 16, 24, 8, 41, None) == 1 and 'multiples of 8' in cfn_hip.last_error()
        assert f(*[p] * 5, p + 8, 1, *ch, None) == 1 and '16-byte' in cfn_hip.last_error()
    from cfn_hip import ops
    with pytest.raises(RuntimeError):
        ops.feat_unpack(torch.zeros(8 * 49, dtype=torch.float16), torch.zeros(1, 5, dtype=torch.int64), torch.ones(1, dtype=torch.int32), ch, 1)
    with pytest.raises(RuntimeError):
        ops.feat_unpack(torch.zeros(8 * 49), torch.zeros(1, 5, dtype=torch.int64), torch.ones(1, dtype=torch.int32), ch, 1)      # fp32 data
    with pytest.raises(RuntimeError):
        ops.feat_pack([torch.zeros(c, 2, 7, 7) for c in ch], torch.float16)                 # host tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        ops.feat_pack([torch.zeros(c, 2, 7, 7) for c in ch], torch.float32)


def test_operator_registration_and_meta_shapes():
    import cfn_hip.torchlib as tl
    assert tl.FEATURE_OPERATORS == ('feat_unpack', 'feat_pack')
    assert not set(tl.FEATURE_OPERATORS) & (set(tl.OPERATORS) | set(tl.INPUT_OPERATORS) | set(tl.AUGMENT_OPERATORS) | set(tl.METRIC_OPERATORS))
    for name in tl.FEATURE_OPERATORS:
        assert hasattr(torch.ops.cfn, name), name
    m = lambda *s, dt=torch.int32: torch.empty(*s, device='meta', dtype=dt)
    ys = torch.ops.cfn.feat_unpack(m(1000, dt=torch.bfloat16), m(3, 5, dt=torch.int64), m(3), list(REAL), 17)
    assert [tuple(y.shape) for y in ys] == [(3, c, 17, 7, 7) for c in REAL] and all(y.dtype == torch.float32 for y in ys)
    y = torch.ops.cfn.feat_pack([m(c, 9, 7, 7, dt=torch.float32) for c in CH], torch.float16)
    assert y.dtype == torch.float16 and tuple(y.shape) == (9 * sum(CH) * 49,)
    y = torch.ops.cfn.feat_pack([m(1, c, 9, 7, 7, dt=torch.float32) for c in CH], torch.bfloat16)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (9 * sum(CH) * 49,)


def test_rounding_claims_of_the_formats():
    """what the docs state about the two formats on post-ReLU unit-normal values: fp16 within 2^-11 relative, bf16 within 2^-8"""
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(1 << 16, generator=g))
    x = x[x > 6.2e-5]                                      # above fp16's smallest normal
    assert float(((x.half().float() - x).abs() / x).max()) <= 2.0 ** -11
    assert float(((x.bfloat16().float() - x).abs() / x).max()) <= 2.0 ** -8
