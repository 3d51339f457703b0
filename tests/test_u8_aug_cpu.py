"""CPU: the host side of the GPU crop / resize / flip of uint8 frames (cfn_hip/u8aug.py, csrc/aug_u8.hip) -- the integer emulation
against the bytes the reference's PIL transforms produced (tests/golden/aug_u8*.npz, make_golden_aug.py), the crop parameters against
what the reference's randomize_parameters drew, the tap tables' invariants, the C ABI's argument checks, the operator registration, the
batch type and the collate builders.  Everything here is exact: the arithmetic is integer."""
import random

import numpy as np
import pytest
import torch

from conftest import load_golden, t


def golden_cases():
    """[(name, src (T, h, w, 3), box (4,), S, want (T, S, S, 3))]: every transform output of the fixtures; loaded once"""
    global _CASES
    if _CASES is None:
        _CASES = []
        z = load_golden('aug_u8')
        for c in z['cases']:
            for i, kind in enumerate(('train', 'train_flip', 'center')):
                _CASES.append(('%s_%s' % (c, kind), z[c + '_src'], z[c + '_box'][i], int(z['size']), z[c + '_out'][i]))
        for tag in ('224a', '224b'):
            z, zt = load_golden('aug_u8_' + tag), load_golden('aug_u8_' + tag + '_train')
            outs = [zt['out_train'][0], zt['out_train'][1], z['out_center']]
            for i, kind in enumerate(('train', 'train_flip', 'center')):
                _CASES.append(('%s_%s' % (tag, kind), z['src'], z['box'][i], int(z['size']), outs[i]))
    return _CASES


_CASES = None


def test_reference_emulation_reproduces_every_golden_case():
    from cfn_hip import u8aug
    cases = golden_cases()
    assert len(cases) == 15
    flips = set()
    for name, src, box, S, want in cases:
        got = u8aug.resize_u8_reference(t(src).unsqueeze(0), t(box).view(1, 4), S)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + want.shape
        assert np.array_equal(got[0].numpy(), want), name
        flips.add(int(box[3]))
    assert flips == {0, 1}
    # the fixtures cover an upscale (3 taps), a near-identity, a > 3x reduction (9 taps) and the model's crop size
    widths = {u8aug.table_width(int(b[2]), S) for _, _, b, S, _ in cases}
    assert {3, 5, 9} <= widths


def test_reference_emulation_pads_time_and_refuses_bad_input():
    from cfn_hip import u8aug
    g = torch.Generator().manual_seed(0)
    f = torch.randint(0, 256, (2, 3, 20, 26, 3), generator=g, dtype=torch.uint8)
    box = torch.tensor([[3, 1, 17, 1], [0, 0, 20, 0]], dtype=torch.int32)
    full = u8aug.resize_u8_reference(f, box, 12)
    cut = u8aug.resize_u8_reference(f, box, 12, lengths=[1, 0])
    assert torch.equal(cut[0, :1], full[0, :1]) and not bool(cut[0, 1:].any()) and not bool(cut[1].any())
    with pytest.raises(ValueError):
        u8aug.resize_u8_reference(f, torch.tensor([[10, 0, 17, 0], [0, 0, 20, 0]]), 12)       # x1 + c > Ws
    with pytest.raises(ValueError):
        u8aug.resize_u8_reference(f.float(), box, 12)


def test_crop_params_reproduce_the_reference_draws():
    from cfn_hip import u8aug
    z = load_golden('aug_params')
    scales = [float(s) for s in z['scales']]
    assert scales == [0.875, 0.7]
    assert len(z['seeds']) >= 20
    for seed, hw, draw, box, center in zip(z['seeds'], z['hw'], z['draws'], z['boxes'], z['centers']):
        rng = random.Random(int(seed))
        got = u8aug.train_crop_params(rng, hw, scales, 224)
        assert got == tuple(int(v) for v in box), (seed, hw)
        assert u8aug.center_crop_params(hw) == tuple(int(v) for v in center), hw
        # the draw order: randint for the scale, then x, y and the flip
        r2 = random.Random(int(seed))
        assert scales[r2.randint(0, 1)] == draw[0] and r2.random() == draw[1] and r2.random() == draw[2] and r2.random() == draw[3]
        assert got[3] == int(draw[3] < 0.5)
    random.seed(7)                                         # the random MODULE is an rng too (the reference's loader uses it)
    a = u8aug.train_crop_params(random, (240, 320), scales)
    assert a == u8aug.train_crop_params(random.Random(7), (240, 320), scales)
    with pytest.raises(ValueError):
        u8aug.train_crop_params(random.Random(0), (600, 800), scales, 64)       # 420 or 525 pixels into 64: more than 4x


def test_resample_table_invariants():
    from cfn_hip import u8aug
    for c, S in [(21, 32), (39, 32), (45, 32), (98, 32), (128, 32), (157, 224), (180, 224), (256, 224), (315, 224), (50, 16), (37, 30),
                 (600, 160), (1248, 312), (1, 8), (7, 7)]:
        bounds, coef = u8aug.resample_table(c, S)
        K = u8aug.table_width(c, S)
        assert bounds.shape == (S, 2) and coef.shape == (S, K) and bounds.dtype == np.int32 and coef.dtype == np.int32
        assert K == 2 * int(np.ceil(max(c / S, 1.0))) + 1 and (K <= u8aug.MAX_TAPS) == (c <= 4 * S)
        xmin, n = bounds[:, 0], bounds[:, 1]
        assert (n >= 1).all() and (n <= K).all() and (xmin >= 0).all() and (xmin + n <= c).all()
        assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= 2).all()
        assert (coef >= 0).all()
        for xx in range(S):
            assert not coef[xx, n[xx]:].any()              # zero taps behind n
        assert (np.diff(xmin) >= 0).all()
        # the rows of the crop a band of 8 output rows reads: what csrc/aug_u8.hip sizes its LDS image for
        half = max(K // 2, 1)
        for rb in (8, 16):                                  # (16 rows per band for tables of up to 5 taps)
            for r0 in range(0, S, rb):
                r1 = min(r0 + rb, S)
                assert (xmin[r0:r1] + n[r0:r1]).max() - xmin[r0] <= (rb + 1) * half + 2
        assert u8aug.resample_table(c, S)[1] is coef        # cached per (c, S)
    for S in (7, 32, 224):                                  # c == S: the identity
        bounds, coef = u8aug.resample_table(S, S)
        assert (bounds[:, 0] == np.arange(S)).all() and (coef[:, 0] == 1 << 22).all() and not coef[:, 1:].any()
    bounds, coef = u8aug.batch_tables([21, 32, 98], 32)      # a batch mixes widths: padded with zero taps to the widest
    assert tuple(bounds.shape) == (3, 32, 2) and tuple(coef.shape) == (3, 32, 9) and coef.dtype == torch.int32
    assert torch.equal(coef[0, :, :3], t(np.array(u8aug.resample_table(21, 32)[1]))) and not bool(coef[0, :, 3:].any())
    with pytest.raises(ValueError):
        u8aug.resample_table(0, 32)


def test_identity_crop_is_the_cropped_source():
    from cfn_hip import u8aug
    g = torch.Generator().manual_seed(1)
    f = torch.randint(0, 256, (1, 2, 40, 50, 3), generator=g, dtype=torch.uint8)
    got = u8aug.resize_u8_reference(f, torch.tensor([[7, 5, 32, 0]]), 32)
    assert torch.equal(got[0], f[0, :, 5:37, 7:39])
    got = u8aug.resize_u8_reference(f, torch.tensor([[7, 5, 32, 1]]), 32)
    assert torch.equal(got[0], f[0, :, 5:37, 7:39].flip(2))
    # and through the tables (what the kernel does: it has no identity branch)
    bounds, coef = u8aug.resample_table(32, 32)
    win = f[0, 0, 5:37, 7:39].numpy().astype(np.int64)
    assert np.array_equal(u8aug._resample_axis(u8aug._resample_axis(win, bounds, coef, 1), bounds, coef, 0), win)


def test_abi_prototype_and_argument_checks():
    import ctypes
    import cfn_hip
    protos = cfn_hip.header_prototypes()
    assert 'cfn_crop_resize_flip_u8' in protos
    ret, at, dt = protos['cfn_crop_resize_flip_u8']
    assert ret is ctypes.c_int and len(at) == 13
    assert dt[:6] == [torch.uint8, torch.int32, torch.int32, torch.int32, torch.int32, torch.uint8] and at[-1] is ctypes.c_void_p
    lib = cfn_hip.load()
    f = lib.cfn_crop_resize_flip_u8
    one = torch.zeros(4, dtype=torch.int32)
    p = one.data_ptr()        # (argument checks run before any launch: host pointers are never dereferenced)
    assert f(None, None, p, p, p, p, 1, 1, 8, 8, 4, 3, None) == 1 and 'null' in cfn_hip.last_error()
    assert f(p, None, None, p, p, p, 1, 1, 8, 8, 4, 3, None) == 1
    assert f(p, None, p, None, p, p, 1, 1, 8, 8, 4, 3, None) == 1
    assert f(p, None, p, p, None, p, 1, 1, 8, 8, 4, 3, None) == 1
    assert f(p, None, p, p, p, None, 1, 1, 8, 8, 4, 3, None) == 1 and 'null' in cfn_hip.last_error()
    for bad in ((0, 1, 8, 8, 4, 3), (1, 0, 8, 8, 4, 3), (1, 1, 0, 8, 4, 3), (1, 1, 8, -1, 4, 3), (1, 1, 8, 8, 0, 3), (1, 1, 8, 8, 4, 0)):
        assert f(p, None, p, p, p, p, *bad, None) == 1 and 'shape' in cfn_hip.last_error(), bad
    # declined geometries: -1, nothing launched (lengths may be NULL: it is optional)
    assert f(p, None, p, p, p, p, 1, 1, 8, 8, 4, 11, None) == -1            # 11 taps: c > 4 * S
    assert f(p, None, p, p, p, p, 1, 1, 8, 8, 4096, 3, None) == -1          # an output row too wide for the LDS image
    from cfn_hip import ops
    frames = torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8)
    box = torch.tensor([[0, 0, 8, 0]], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.crop_resize_flip_u8(frames, None, box, 4)                       # host tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        ops.crop_resize_flip_u8(frames.float(), None, box, 4)
    with pytest.raises(RuntimeError, match='4 \\* size'):
        ops.crop_resize_flip_u8(frames, None, torch.tensor([[0, 0, 8, 0]], dtype=torch.int32), 1)      # 8 pixels into 1
    with pytest.raises(RuntimeError):
        ops.crop_resize_flip_u8(frames, None, torch.zeros(2, 4, dtype=torch.int32), 4)                 # two boxes for one clip


def test_operator_registration_and_meta_shape():
    import cfn_hip.torchlib as tl
    assert tl.AUGMENT_OPERATORS == ('crop_resize_flip_u8',)
    assert not set(tl.AUGMENT_OPERATORS) & (set(tl.OPERATORS) | set(tl.INPUT_OPERATORS))
    for name in tl.AUGMENT_OPERATORS:
        assert hasattr(torch.ops.cfn, name), name
    m = lambda *s, dt=torch.int32: torch.empty(*s, device='meta', dtype=dt)
    y = torch.ops.cfn.crop_resize_flip_u8(m(2, 4, 30, 34, 3, dt=torch.uint8), m(2), m(2, 4), m(2, 16, 2), m(2, 16, 5), 16)
    assert y.shape == (2, 4, 16, 16, 3) and y.dtype == torch.uint8
    y = torch.ops.cfn.crop_resize_flip_u8(m(1, 1, 240, 320, 3, dt=torch.uint8), None, m(1, 4), m(1, 224, 2), m(1, 224, 3), 224)
    assert y.shape == (1, 1, 224, 224, 3)


def _raw_clip(g, n, T, h, w):
    return torch.randint(0, 256, (n, T, h, w, 3), generator=g, dtype=torch.uint8)


def test_raw_u8_clips_batch_type():
    from cfn_hip.u8clips import RawU8Clips
    g = torch.Generator().manual_seed(3)
    r = RawU8Clips(_raw_clip(g, 2, 5, 20, 30).view(1, 2, 5, 20, 30, 3), torch.tensor([[5, 3]], dtype=torch.int32),
                   torch.tensor([[[1, 2, 14, 0], [0, 0, 20, 1]]], dtype=torch.int32))
    assert tuple(r.shape) == (1, 2, 3, 5, 20, 30) and r.dim() == 6 and r.size(0) == 1 and r.device.type == 'cpu'
    fl = r.flatten_crops()
    assert isinstance(fl, RawU8Clips) and tuple(fl.frames.shape) == (2, 5, 20, 30, 3) and tuple(fl.lengths.shape) == (2,) and tuple(fl.box.shape) == (2, 4)
    moved = r.to('cpu')
    assert isinstance(moved, RawU8Clips) and all(torch.equal(a, b) for a, b in zip(moved, r))
    with pytest.raises(TypeError):
        r.to(torch.float32)
    sl = fl.time_slice(2, 5)
    assert isinstance(sl, RawU8Clips) and sl.frames.shape[1] == 3 and sl.lengths.tolist() == [3, 1] and torch.equal(sl.box, fl.box)
    assert all(a is b for a, b in zip(type(r)(*[m for m in r]), r))       # a namedtuple: rebuilt from its members (staging, pinning)
    assert RawU8Clips._fields == ('frames', 'lengths', 'box')
    with pytest.raises(RuntimeError):
        fl.transform(16)                                    # host tensors: the transform runs on the GPU only


def test_raw_collate_builders_pad_space_and_time():
    import collate
    from cfn_hip.u8clips import RawU8Clips
    g = torch.Generator().manual_seed(4)
    shapes = [(5, 20, 30), (9, 24, 18), (7, 12, 12)]
    boxes = [[[2, 1, 17, 1]], [[0, 3, 18, 0]], [[0, 0, 12, 0]]]
    smp = []
    for i, ((T, h, w), b) in enumerate(zip(shapes, boxes)):
        smp.append(((_raw_clip(g, 1, T, h, w), np.asarray(b) if i == 1 else torch.tensor(b)), (torch.rand(157, T * 10, generator=g) < 0.1).float(), 'v%d' % i))
    got = collate.fine_collate_raw_u8(smp)
    raw = got[0]
    assert isinstance(raw, RawU8Clips) and raw.frames.dtype == torch.uint8 and raw.lengths.dtype == torch.int32 and raw.box.dtype == torch.int32
    assert tuple(raw.frames.shape) == (3, 1, 9, 24, 30, 3) and raw.lengths.tolist() == [[5], [9], [7]] and raw.box.tolist() == boxes
    for i, (T, h, w) in enumerate(shapes):
        assert torch.equal(raw.frames[i, :, :T, :h, :w], smp[i][0][0])
        pad = raw.frames[i].clone()
        pad[:, :T, :h, :w] = 0
        assert not bool(pad.any())                          # zero right of, below and behind every clip
    ref = collate.fine_collate_u8([(c[0][:, :, :8, :8].contiguous(), lb, v) for c, lb, v in smp])
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and got[3] == ref[3]

    feat = lambda tf: {k: torch.randn(c, tf, 7, 7, generator=g) for k, c in (('layer1', 4), ('conv5', 6))}
    csmp = [(s[0], s[1], feat(20 + 5 * i), torch.tensor([0, shapes[i][0], 20, 1]), s[2], 10.0 + i) for i, s in enumerate(smp)]
    cgot = collate.coarse_collate_raw_u8(csmp)
    cref = collate.coarse_collate_u8([(s[0][0][:, :, :8, :8].contiguous(),) + s[1:] for s in csmp])
    assert isinstance(cgot[0], RawU8Clips) and all(torch.equal(a, b) for a, b in zip(cgot[0], raw))
    assert torch.equal(cgot[1], cref[1]) and torch.equal(cgot[4], cref[4]) and torch.equal(cgot[5], cref[5]) and cgot[6] == cref[6]
    assert all(torch.equal(cgot[3][k], cref[3][k]) for k in cref[3])

    lb = torch.zeros(157, 40)
    for clip in ((torch.zeros(1, 4, 8, 8, 3), torch.tensor([[0, 0, 8, 0]])),                            # fp32 frames
                 (torch.zeros(1, 4, 8, 8, dtype=torch.uint8), torch.tensor([[0, 0, 8, 0]])),             # no channel dimension
                 (torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([[0., 0., 8., 0.]])),      # float boxes
                 (torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([0, 0, 8, 0])),            # (4,) for n = 1 clips
                 (torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([[1, 0, 8, 0]])),          # the window leaves the picture
                 (torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([[0, 0, 0, 0]])),          # empty window
                 (torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([[0, 0, 8, 2]])),          # flip is 0 or 1
                 torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8)):                                         # no box at all
        with pytest.raises(ValueError):
            collate.fine_collate_raw_u8([(clip, lb, 'v')])
    with pytest.raises(ValueError):                          # one clip per sample here, two there
        collate.fine_collate_raw_u8([((torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([[0, 0, 8, 0]])), lb, 'a'),
                                     ((torch.zeros(2, 4, 8, 8, 3, dtype=torch.uint8), torch.tensor([[0, 0, 8, 0], [0, 0, 8, 0]])), lb, 'b')])
