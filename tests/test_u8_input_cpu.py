"""uint8 video input, host side (no GPU): the normalisation table against the reference's own pipeline, the uint8 batch
builders against the fp32 ones, the U8Clips batch type, the ABI mapping and the models' state_dict keys."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, t

MEAN, STD = [0.413, 0.368, 0.338], [0.131, 0.125, 0.132]


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _u8_clip(g, n, T, H=8, W=12):
    return torch.randint(0, 256, (n, T, H, W, 3), generator=g, dtype=torch.uint8)


def _normalised(clip_u8, lut):
    """what the reference's loader hands to its collate: (n, 3, T, H, W) fp32"""
    from cfn_hip.u8clips import U8Clips
    return U8Clips(clip_u8, torch.full((clip_u8.shape[0],), clip_u8.shape[1], dtype=torch.int32)).to_f32(lut)


def test_clip_lut_reproduces_the_reference_pipeline():
    """tests/golden/clip_u8.npz: frames with every byte value in every channel through the reference's ToTensor + Normalize +
    stack + permute; a gather through the table is bit-identical"""
    from cfn_hip import ops
    from cfn_hip.u8clips import CHARADES_MEAN, CHARADES_STD
    z = load_golden('clip_u8')
    frames, clip = t(z['frames']), t(z['clip'])
    for c in range(3):
        assert len(torch.unique(frames[..., c])) == 256
    assert [float(v) for v in z['mean']] == CHARADES_MEAN and [float(v) for v in z['std']] == CHARADES_STD
    lut = ops.clip_lut([float(v) for v in z['mean']], [float(v) for v in z['std']], int(z['norm_value']))
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    got = torch.stack([lut[c][frames[..., c].long()] for c in range(3)], 0)            # (3, T, H, W)
    assert torch.equal(got, clip)
    assert not bool((lut == 0).any())               # no byte normalises to 0.0: padding needs the per-clip lengths
    import cfn_hip.torchlib  # noqa: F401  (the registered operator builds the same table)
    assert torch.equal(torch.ops.cfn.clip_lut(CHARADES_MEAN, CHARADES_STD), lut)


def test_u8clips_shape_slice_flatten():
    from cfn_hip.u8clips import U8Clips
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (2, 3, 10, 8, 12, 3), generator=g, dtype=torch.uint8)
    lengths = torch.tensor([[10, 10, 10], [4, 4, 4]], dtype=torch.int32)
    u = U8Clips(frames, lengths)
    assert tuple(u.shape) == (2, 3, 3, 10, 8, 12) and tuple(u.shape[:2]) == (2, 3)
    f = u.flatten_crops()
    assert isinstance(f, U8Clips) and tuple(f.frames.shape) == (6, 10, 8, 12, 3) and tuple(f.shape) == (6, 3, 10, 8, 12) and f.shape[2] == 10
    assert f.lengths.tolist() == [10, 10, 10, 4, 4, 4] and torch.equal(f.frames[4], frames[1, 1])
    s = f.time_slice(3, 8)
    assert tuple(s.frames.shape) == (6, 5, 8, 12, 3) and s.lengths.tolist() == [5, 5, 5, 1, 1, 1] and s.lengths.dtype == torch.int32
    assert torch.equal(s.frames, f.frames[:, 3:8])
    assert f.time_slice(6, 10).lengths.tolist() == [4, 4, 4, 0, 0, 0]
    assert f.time_slice(8, 99).frames.shape[1] == 2
    # the fp32 clip it stands for: slicing commutes with the conversion, padding is exact zeros
    from cfn_hip import ops
    lut = ops.clip_lut(MEAN, STD)
    x = f.to_f32(lut)
    assert tuple(x.shape) == (6, 3, 10, 8, 12) and bool((x[3:, :, 4:] == 0).all()) and bool((x[3:, :, :4] != 0).all())
    assert torch.equal(s.to_f32(lut), x[:, :, 3:8])


def test_u8clips_survives_map_tensors_and_pinning(monkeypatch):
    from cfn_hip.u8clips import U8Clips
    from cfn_hip import staging
    u = U8Clips(torch.zeros(2, 1, 4, 4, 4, 3, dtype=torch.uint8), torch.tensor([[4], [2]], dtype=torch.int32))
    seen = []
    m = staging._map_tensors([u, torch.zeros(2), ['a', 'b']], lambda x: (seen.append(x.dtype), x.clone())[1])
    assert isinstance(m[0], U8Clips) and torch.equal(m[0].lengths, u.lengths) and m[0].frames is not u.frames
    assert seen == [torch.uint8, torch.int32, torch.float32]
    plan, total = staging.HostStager._plan([u, torch.zeros(2)])
    assert [p[2] for p in plan] == [2 * 4 * 4 * 4 * 3, 8, 8]
    # DataLoader(pin_memory=True) walks the batch with this function and rebuilds namedtuples around the pinned members.  A host without
    # an accelerator runtime cannot pin, so Tensor.pin_memory is replaced by a copy: the walk and the rebuild are what is checked here.
    from torch.utils.data._utils.pin_memory import pin_memory
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self, *a, **k: self.clone())
    p = pin_memory([u, torch.zeros(2)])
    assert isinstance(p[0], U8Clips) and torch.equal(p[0].frames, u.frames) and p[0].frames is not u.frames and torch.equal(p[0].lengths, u.lengths)
    with pytest.raises(TypeError):
        u.to(torch.float32)                      # the element types are part of the format
    assert isinstance(u.to('cpu'), U8Clips)


def test_fine_collate_u8_matches_fine_collate():
    import collate
    from cfn_hip import ops
    from cfn_hip.u8clips import U8Clips
    g = torch.Generator().manual_seed(1)
    lut = ops.clip_lut(MEAN, STD)
    lens, tls = [5, 9, 7], [50, 90, 70]
    raw = [(_u8_clip(g, 2, T), (torch.rand(157, tl, generator=g) < 0.1).float(), 'v%d' % i) for i, (T, tl) in enumerate(zip(lens, tls))]
    ref = collate.fine_collate([(_normalised(c, lut), lb, v) for c, lb, v in raw])
    got = collate.fine_collate_u8([(c.numpy() if i == 1 else c, lb, v) for i, (c, lb, v) in enumerate(raw)])      # numpy or tensors
    assert isinstance(got[0], U8Clips) and got[0].frames.dtype == torch.uint8 and got[0].lengths.dtype == torch.int32
    assert tuple(got[0].frames.shape) == (3, 2, 9, 8, 12, 3) and got[0].lengths.tolist() == [[5, 5], [9, 9], [7, 7]]
    assert tuple(got[0].shape) == tuple(ref[0].shape)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and got[3] == ref[3]
    assert torch.equal(got[0].to_f32(lut), ref[0])          # table gather + zeroed padding + permute = the fp32 batch
    assert got[0].frames.numel() * got[0].frames.element_size() * 4 == ref[0].numel() * ref[0].element_size()      # a quarter of the bytes


def test_coarse_collate_u8_matches_coarse_collate():
    import collate
    from cfn_hip import ops
    g = torch.Generator().manual_seed(2)
    lut = ops.clip_lut(MEAN, STD)
    raw = []
    for i, (T, tl, tf) in enumerate(((6, 60, 150), (4, 40, 20))):
        feat = {k: torch.randn(c, tf, 7, 7, generator=g) for k, c in (('layer1', 4), ('conv5', 6))}
        raw.append((_u8_clip(g, 1, T), (torch.rand(157, tl, generator=g) < 0.1).float(), feat, torch.tensor([0, T, T, 1]), 'v%d' % i, 10.0 + i))
    ref = collate.coarse_collate([(_normalised(b[0], lut),) + b[1:] for b in raw])
    got = collate.coarse_collate_u8(raw)
    assert got[0].lengths.tolist() == [[6], [4]] and tuple(got[0].shape) == tuple(ref[0].shape)
    assert torch.equal(got[0].to_f32(lut), ref[0])
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and torch.equal(got[4], ref[4]) and torch.equal(got[5], ref[5])
    assert got[3].keys() == ref[3].keys() and all(torch.equal(got[3][k], ref[3][k]) for k in ref[3])
    assert got[6] == ref[6] and torch.equal(got[7], ref[7])
    with pytest.raises(ValueError):
        collate.fine_collate_u8([(torch.zeros(1, 3, 4, 8, 8), torch.zeros(157, 4), 'v')])      # an fp32 clip is not uint8 frames


def test_header_maps_unsigned_char_and_ops_refuse_cpu_tensors():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    for name in ('cfn_clip_u8_to_f32', 'cfn_stem_conv_u8_fwd', 'cfn_stem_conv_u8_bwd_weight'):
        assert name in protos, name
    assert protos['cfn_clip_u8_to_f32'][2][:4] == [torch.uint8, torch.float32, torch.int32, torch.float32]
    assert protos['cfn_stem_conv_u8_fwd'][2][0] == torch.uint8 and protos['cfn_stem_conv_u8_bwd_weight'][2][1] == torch.uint8
    lib = cfn_hip.load()
    assert lib.cfn_clip_u8_to_f32(None, None, None, None, 1, 1, 4, 4, None) == 1 and 'null' in cfn_hip.last_error()
    assert lib.cfn_stem_conv_u8_fwd(None, None, None, None, None, 1, 3, 24, 1, 4, 4, None) == 1
    one = torch.zeros(1)
    p = one.data_ptr()        # (argument checks run before any launch: host pointers are never dereferenced)
    assert lib.cfn_stem_conv_u8_fwd(p, p, None, p, p, 1, 4, 24, 1, 4, 4, None) == 1 and 'Cimg' in cfn_hip.last_error()
    assert lib.cfn_stem_conv_u8_bwd_weight(p, p, p, None, p, 1, 1, 24, 1, 224, 224, None) == 1 and 'Cimg' in cfn_hip.last_error()
    from cfn_hip import ops
    lut = ops.clip_lut(MEAN, STD)
    frames = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.clip_u8_to_f32(frames, lut)
    with pytest.raises(RuntimeError):
        ops.stem_conv_u8(frames, None, lut, torch.zeros(24, 3, 1, 3, 3))
    with pytest.raises(RuntimeError):
        ops.clip_u8_to_f32(frames.float(), lut)           # not uint8
    import cfn_hip.torchlib as tl
    assert 'stem_conv_u8' in tl.OPERATORS and set(tl.INPUT_OPERATORS) == {'clip_lut', 'clip_u8_to_f32'}
    for name in tl.INPUT_OPERATORS + ('stem_conv_u8', 'stem_conv_u8_backward'):
        assert hasattr(torch.ops.cfn, name), name
    m = lambda *s, dt=torch.float32: torch.empty(*s, device='meta', dtype=dt)
    assert torch.ops.cfn.stem_conv_u8(m(2, 4, 32, 32, 3, dt=torch.uint8), m(2, dt=torch.int32), m(3, 256), m(24, 3, 1, 3, 3)).shape == (2, 24, 4, 16, 16)
    assert torch.ops.cfn.clip_u8_to_f32(m(2, 4, 30, 34, 3, dt=torch.uint8), m(3, 256)).shape == (2, 3, 4, 30, 34)


def test_set_input_norm_keeps_state_dict_keys():
    import x3d_fine
    import x3d_coarse
    from cfn_hip import ops
    from cfn_hip.u8clips import U8Clips, CHARADES_MEAN, CHARADES_STD
    for net in (x3d_fine.generate_model('M', n_classes=157, task='loc', base_bn_splits=1),
                x3d_coarse.generate_model('M', n_classes=157, task='loc', base_bn_splits=1, learnedMixing=True, isMixing=True, t_pool='grid',
                                          feat_depth={'layer1': 24, 'layer2': 48, 'layer3': 96, 'layer4': 192, 'conv5': 432})):
        keys = list(net.state_dict().keys())
        assert net.set_input_norm(CHARADES_MEAN, CHARADES_STD) is net
        assert list(net.state_dict().keys()) == keys
        assert torch.equal(net.input_lut, ops.clip_lut(CHARADES_MEAN, CHARADES_STD)) and 'input_lut' in dict(net.named_buffers())
        net.load_state_dict(net.state_dict())             # strict: the table is not a checkpoint key
    bare = x3d_fine.generate_model('M', n_classes=157, task='loc', base_bn_splits=1)
    with pytest.raises(RuntimeError, match='set_input_norm'):
        bare([U8Clips(torch.zeros(1, 4, 32, 32, 3, dtype=torch.uint8), torch.tensor([4], dtype=torch.int32)), None])
