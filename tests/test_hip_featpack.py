"""GPU: packed 16-bit fine features (csrc/featpack.hip, cfn_hip/featpack.py) -- the unpack kernel against PackedFeats.unpack_reference, the
pack kernel against the CPU's tensor.to(dtype), no host synchronisation and graph capture, the two native operators, the coarse net on
unpacked features, and the extraction / training scripts fed by records.

Bounds.  Widening a 16-bit float to fp32 is exact and rounding to nearest even is defined bit for bit, so every comparison of the kernels'
outputs is torch.equal (on bit patterns where -0.0 matters).  A net fed PackedFeats.unpack() reads the same fp32 values as one fed the dict
built on the host from the rounded features: with the library's deterministic mode on (cross-workgroup accumulations commit in a fixed
order) its logits and the training losses are compared with == as well."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CH = (8, 16, 24, 8, 40)
REAL = (24, 48, 96, 192, 432)
DTYPES = [torch.float16, torch.bfloat16]


def _finite_bits(n, dt, seed):
    """n random 16-bit patterns of `dt` as int16, every finite value class included (subnormals, both zeros); NaNs become infinities"""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32)
    exp, man = (0x7c00, 0x03ff) if dt == torch.float16 else (0x7f80, 0x007f)
    bits = torch.where((bits & exp) == exp, bits & ~man, bits)
    return bits.to(torch.int16)


def _special_bits(dt):
    """smallest / largest subnormal, -0.0, +0.0, 65504 (fp16's largest; bf16: its neighbour 65280), +inf, -inf"""
    if dt == torch.float16:
        pats = [0x0001, 0x03ff, 0x8001, 0x8000, 0x0000, 0x7bff, 0x7c00, 0xfc00]
    else:
        pats = [0x0001, 0x007f, 0x8001, 0x8000, 0x0000, 0x477f, 0x7f80, 0xff80]
    return torch.tensor(pats, dtype=torch.int32).to(torch.int16)


def _packed(dt, channels, lengths, seed, order=None, gap=0, t_max=None, numel=None):
    """a PackedFeats batch on the host over random finite bit patterns (the specials at the start of every block); `order`: the order
    in which the B * 5 blocks lie in the buffer; `gap`: multiples of 8 unused elements (a recognisable value) in front of each block"""
    from cfn_hip.featpack import PackedFeats
    B = len(lengths)
    ids = [(b, k) for b in range(B) for k in range(5)]
    if order is not None:
        ids = [ids[i] for i in order]
    sizes = {(b, k): lengths[b] * channels[k] * 49 for b, k in ids}
    total = sum(sizes.values()) + 8 * gap * (len(ids) + 1)
    data = torch.full((max(total, numel or 0),), 0x5a5a, dtype=torch.int16)
    offsets = torch.zeros(B, 5, dtype=torch.int64)
    pos = 0
    sp = _special_bits(dt)
    for j, (b, k) in enumerate(ids):
        pos += 8 * gap
        blk = _finite_bits(sizes[(b, k)], dt, seed * 1000 + j)
        blk[:min(len(sp), len(blk))] = sp[:len(blk)]
        data[pos:pos + sizes[(b, k)]] = blk
        offsets[b, k] = pos
        pos += sizes[(b, k)]
    assert not bool((offsets % 8).any())
    return PackedFeats(data.view(dt), offsets, torch.tensor(lengths, dtype=torch.int32), tuple(channels), int(t_max or max(lengths)))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check_unpack(pf):
    want = pf.unpack_reference()
    dpf = pf.to(DEV)
    out = {k: torch.full((pf.batch, c, pf.t_max, 7, 7), float('nan'), device=DEV) for k, c in zip(pf.keys(), pf.channels)}
    got = dpf.unpack(out=out)
    assert list(got) == list(want)
    for k in want:
        assert got[k] is out[k] and torch.equal(_bits(got[k].cpu()), _bits(want[k])), k        # bit patterns: -0.0 stays -0.0
        assert not bool(torch.isnan(got[k]).any()), k                                           # every element was written
    fresh = dpf.unpack()                                                                        # outputs from torch.empty
    assert all(torch.equal(_bits(fresh[k]), _bits(got[k])) for k in want)
    return got


@pytest.mark.parametrize('dt', DTYPES)
def test_unpack_equals_reference(dt):
    """small channels with lengths (1, 5, 13): one partial tile of frames, padding behind every shorter video; the real channel counts with
    lengths (128, 127): 8 full tiles of 16 frames, the last one with a single padding frame; lengths (17, 33) with t_max 40: tiles that
    are whole padding and a t_max that is no multiple of the tile"""
    got = _check_unpack(_packed(dt, CH, (1, 5, 13), 1))
    assert not bool(got['layer1'][0, :, 1:].any()) and not bool(got['conv5'][1, :, 5:].any())
    sp = _special_bits(dt).view(dt).float()
    assert torch.equal(_bits(got['layer2'][2, 0, 0].reshape(-1)[:8].cpu()), _bits(sp))          # the specials, through the whole path
    _check_unpack(_packed(dt, REAL, (128, 127), 2))
    _check_unpack(_packed(dt, CH, (17, 33), 3, t_max=40))


@pytest.mark.parametrize('dt', DTYPES)
def test_unpack_blocks_out_of_order_with_gaps(dt):
    order = [7, 2, 14, 0, 9, 4, 11, 1, 13, 6, 3, 12, 8, 5, 10]
    pf = _packed(dt, CH, (1, 5, 13), 4, order=order, gap=3)
    assert pf.offsets.view(-1).tolist() != sorted(pf.offsets.view(-1).tolist())
    _check_unpack(pf)
    # lengths are data too: a length beyond t_max is clamped, a negative one reads as 0 (the reference clamps the same way)
    from cfn_hip.featpack import PackedFeats
    big = _packed(dt, CH, (13, 13, 13), 5)
    odd = PackedFeats(big.data, big.offsets, torch.tensor([40, -3, 6], dtype=torch.int32), big.channels, 13)
    got = _check_unpack(odd)
    assert not bool(got['layer3'][1].any()) and not bool(got['layer3'][2, :, 6:].any())


def _pack_inputs(T, channels, dt, seed):
    g = torch.Generator().manual_seed(seed)
    maps = [torch.randn(c, T, 7, 7, generator=g) * 10.0 ** float(torch.randint(-6, 5, (1,), generator=g)) for c in channels]
    if dt == torch.float16:                    # exact ties of fp16 (11 significant bits), its overflow threshold, its subnormal range
        sp = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 65519.9, 65520.0, -0.0, -65520.0, 65504.0, 2.0 ** -24, 3 * 2.0 ** -25, 1e-40, 1e38,
              -(1 + 2.0 ** -11), 6.1e-5]
    else:                                      # the same values (none is a tie of bf16's 8 bits) and bf16's own ties; fp32 subnormals stay subnormal
        sp = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 65519.9, 65520.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1e-40, -1e-40, 3.3e38, 3.4e38,
              2.0 ** -133 * 1.5, 2.0 ** -134]
    for m in maps:
        m.view(-1)[:len(sp)] = torch.tensor(sp, dtype=torch.float64).to(torch.float32)[:m.numel()]
    return maps


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('T,channels', [(1, CH), (7, CH), (7, REAL), (128, CH)])
def test_pack_equals_cpu_rounding(T, channels, dt):
    import cfn_hip.torchlib  # noqa: F401
    from cfn_hip import featpack, ops
    maps = _pack_inputs(T, channels, dt, T)
    maps[1].view(-1)[-1] = float('nan')
    maps[4].view(-1)[20] = -float('nan')
    want, frames, ch = featpack.pack_reference(dict(zip(featpack.FEAT_KEYS, maps)), dt)
    assert frames == T and ch == tuple(channels)
    got = ops.feat_pack([m.to(DEV) for m in maps], dt)
    assert got.dtype == dt and got.shape == want.shape
    nan = torch.isnan(want)
    assert int(nan.sum()) == 2 and torch.equal(torch.isnan(got).cpu(), nan)                     # a NaN stays a NaN
    gb, wb = got.cpu().view(torch.int16), want.view(torch.int16)
    bad = (gb != wb) & ~nan
    assert not bool(bad.any()), (int(bad.sum()), got.cpu()[bad][:8], want[bad][:8])
    if dt == torch.float16:
        head = got[:8].float().cpu().tolist()          # (t = 0, c = 0, p = 0..7 of the first block: the first specials)
        assert head[0] == 1.0 and head[1] == 1 + 2.0 ** -9 and head[2] == 0.0 and head[3] == 65504.0 and head[4] == float('inf')
    assert torch.equal(torch.ops.cfn.feat_pack([m.unsqueeze(0).to(DEV) for m in maps], dt).view(torch.int16)[~nan.to(DEV)], got.view(torch.int16)[~nan.to(DEV)])
    # pack -> unpack: the maps, rounded
    from cfn_hip.featpack import PackedFeats
    clean = [torch.nan_to_num(m, nan=0.0) for m in maps]
    data = ops.feat_pack([m.to(DEV) for m in clean], dt)
    starts = np.cumsum([0] + [T * c * 49 for c in channels[:-1]]).tolist()
    pf = PackedFeats(data, torch.tensor([starts], dtype=torch.int64, device=DEV), torch.tensor([T], dtype=torch.int32, device=DEV), tuple(channels), T)
    un = pf.unpack()
    for k, m in zip(pf.keys(), clean):
        assert torch.equal(_bits(un[k][0].cpu()), _bits(m.to(dt).float())), k


@pytest.mark.parametrize('dt', DTYPES)
def test_unpack_does_not_synchronise(dt):
    pf = _packed(dt, CH, (1, 5, 13), 6).to(DEV)
    want = pf.unpack()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = pf.unpack()
        again = pf.unpack(out=got)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert all(again[k] is got[k] and torch.equal(_bits(got[k]), _bits(want[k])) for k in want)


@pytest.mark.capture
@pytest.mark.parametrize('dt', DTYPES)
def test_capture_and_replay_on_new_data(dt):
    from cfn_hip.featpack import PackedFeats
    a = _packed(dt, CH, (13, 5, 1), 7, numel=110000)
    b = _packed(dt, CH, (2, 13, 7), 8, order=list(range(14, -1, -1)), gap=2, numel=110000)
    assert a.data.numel() == b.data.numel() == 110000 and a.t_max == b.t_max == 13
    st = a.to(DEV)                                                    # the static buffers of the graph
    out = {k: torch.zeros(3, c, 13, 7, 7, device=DEV) for k, c in zip(a.keys(), CH)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.unpack(out=out)                                            # warm-up outside the capture
    side.synchronize()
    assert all(torch.equal(_bits(out[k].cpu()), _bits(v)) for k, v in a.unpack_reference().items())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st.unpack(out=out)
    st.data.copy_(b.data.to(DEV))
    st.offsets.copy_(b.offsets.to(DEV))
    st.lengths.copy_(b.lengths.to(DEV))
    for v in out.values():
        v.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    eager = PackedFeats(st.data, st.offsets, st.lengths, CH, 13).unpack()
    want = b.unpack_reference()
    assert all(torch.equal(_bits(out[k]), _bits(eager[k])) and torch.equal(_bits(out[k].cpu()), _bits(want[k])) for k in want)


def test_operators_equal_ops_and_pass_opcheck():
    import cfn_hip.torchlib  # noqa: F401
    from cfn_hip import ops
    utils = ('test_schema', 'test_faketensor')             # (no gradient is registered: features from disk carry none)
    for dt in DTYPES:
        pf = _packed(dt, CH, (1, 5, 13), 9).to(DEV)
        ys = torch.ops.cfn.feat_unpack(pf.data, pf.offsets, pf.lengths, list(pf.channels), pf.t_max)
        ref = ops.feat_unpack(pf.data, pf.offsets, pf.lengths, pf.channels, pf.t_max)
        assert len(ys) == 5 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ys, ref))
        torch.library.opcheck(torch.ops.cfn.feat_unpack.default, (pf.data, pf.offsets, pf.lengths, list(pf.channels), pf.t_max), test_utils=utils)
        maps = [m.to(DEV) for m in _pack_inputs(3, CH, dt, 10)]
        torch.library.opcheck(torch.ops.cfn.feat_pack.default, (maps, dt), test_utils=utils)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.feat_unpack(pf.data.float(), pf.offsets, pf.lengths, list(CH), 13)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.feat_unpack(pf.data, pf.offsets, pf.lengths, [8, 16, 24, 12, 36], 13)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.feat_unpack(pf.data, pf.offsets.int(), pf.lengths, list(CH), 13)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.feat_pack(maps, torch.float32)
    with pytest.raises(RuntimeError):
        torch.ops.cfn.feat_pack(maps[:4], torch.float16)


class _Deterministic(object):
    def __enter__(self):
        import cfn_hip
        self.prev = cfn_hip.deterministic(True)

    def __exit__(self, *exc):
        import cfn_hip
        cfn_hip.deterministic(self.prev)


@pytest.fixture(scope='module')
def coarse_net():
    import train_coarse_fineFEAT as tc
    from oracle import spec
    net = tc.build_model(DEV, pretrained=None, dropout=0.0)
    spec.fill_module_(net)
    return net.eval()


@pytest.mark.parametrize('dt', DTYPES)
def test_coarse_forward_on_unpacked_features(coarse_net, dt, tmp_path):
    """x3d_coarse, eval mode, 2 x 3 x 16 x 224 x 224 with T' = (24, 17): PackedFeats.unpack() against the dict {k: rounded.float()} built on
    the host -- single crop (two videos) and multi-crop (n = 2: the two clips are crops of the first video)"""
    import collate
    import train_coarse_fineFEAT as tc
    from cfn_hip import featpack
    from oracle import spec
    x = spec.rand_input(300, (2, 3, 16, 224, 224)).to(DEV)
    recs, plain = [], []
    for b, n in enumerate((24, 17)):
        feat = {k: spec.rand_input(310 + 5 * b + i, (c, n, 7, 7), nonneg=True) for i, (k, c) in enumerate(tc.FEAT_DEPTH.items())}
        payload, frames, channels = featpack.pack_reference(feat, dt)
        recs.append(featpack.open_record(featpack.write_record(featpack.record_path(str(tmp_path), 'v%d' % b), payload, dt, frames, channels)))
        plain.append({k: v.to(dt).float() for k, v in feat.items()})
    lb = torch.zeros(157, 160)
    smp = lambda feats: [(torch.zeros(1, 3, 1, 1, 1), lb, f, torch.tensor([2 * b, 16, n, 1]), 'v%d' % b, 1.0) for b, (f, n) in enumerate(zip(feats, (24, 17)))]
    with _Deterministic(), torch.no_grad():
        for nb in (2, 1):                                                       # nb = 1: multi-crop, n = 2
            bp, bd = collate.coarse_collate_packed(smp(recs)[:nb]), collate.coarse_collate(smp(plain)[:nb])
            pf = bp[3].to(DEV)
            assert pf.t_max == 24 and pf.data.dtype == dt
            fm, meta = bp[4].to(DEV), bp[5].to(DEV)
            assert torch.equal(bp[4], bd[4]) and torch.equal(bp[5], bd[5])
            want = coarse_net([x, {k: v.to(DEV) for k, v in bd[3].items()}, fm, 0, meta])
            got = coarse_net([x, pf.unpack(), fm, 0, meta])
            via = tc.forward_video(coarse_net, x, pf, fm, 0, meta)               # the script's entry takes the PackedFeats itself
            assert tuple(got.shape) == (2, 157, 16) and bool(torch.isfinite(got).all())
            assert torch.equal(got, want) and torch.equal(via, want), (nb, float((got - want).abs().max()))


@pytest.fixture(scope='module')
def extracted(tmp_path_factory):
    """two synthetic videos through the fine tower: the fp32 five-file store and the fp16 records of the SAME net"""
    import extract_fineFEAT as ex
    d = tmp_path_factory.mktemp('extracted')
    torch.manual_seed(0)
    net = ex.build_tower(DEV, ckpt=None)
    g = torch.Generator().manual_seed(1)
    vids = [('vid_a', torch.randn(1, 3, 24, 224, 224, generator=g)), ('vid_b', torch.randn(1, 3, 17, 224, 224, generator=g))]
    with _Deterministic():
        assert ex.extract(net, vids, str(d / 'f32')) == 2
        assert ex.extract(net, vids, str(d / 'p16'), feat_dtype='fp16') == 2
        assert ex.extract(net, vids[:1], str(d / 'pb16'), feat_dtype='bf16') == 1
    return d


def test_extract_writes_records_equal_to_the_rounded_fp32_files(extracted):
    from cfn_hip import featpack
    d = extracted
    assert sorted(os.listdir(str(d / 'p16'))) == ['packed'] and sorted(os.listdir(str(d / 'p16' / 'packed'))) == ['vid_a.cff', 'vid_b.cff']
    for sub, dt, vids in (('p16', torch.float16, (('vid_a', 24), ('vid_b', 17))), ('pb16', torch.bfloat16, (('vid_a', 24),))):
        for vid, frames in vids:
            rec = featpack.open_record(featpack.record_path(str(d / sub), vid))
            assert rec.dtype == dt and rec.frames == frames and rec.channels == REAL
            got = rec.to_dict()
            for k in featpack.FEAT_KEYS:
                f32 = torch.load(os.path.join(str(d / 'f32'), k, vid))
                assert f32.dtype == torch.float32 and tuple(f32.shape) == (1,) + tuple(got[k].shape)
                assert torch.equal(got[k], f32[0].to(dt).float()), (vid, k)
                assert float(f32.abs().max()) > 0


def test_records_feed_the_coarse_training_script(extracted, tmp_path, monkeypatch):
    """Dataset of samples whose feature member is a Record -> DataLoader(collate.coarse_collate_packed, pin_memory=True) -> staging ->
    train_coarse_fineFEAT.run(max_steps=2), against the same run fed dict batches of the same rounded features: the same losses"""
    import torch.utils.data as tud
    import collate
    import train_coarse_fineFEAT as tc
    from cfn_hip import featpack, staging
    from cfn_hip.featpack import PackedFeats
    recs = [featpack.open_record(featpack.record_path(str(extracted / 'p16'), v)) for v in ('vid_a', 'vid_b')]

    class Videos(tud.Dataset):
        def __init__(self, packed):
            self.packed = packed

        def __len__(self):
            return 4

        def __getitem__(self, i):
            r = np.random.RandomState(50 + i)
            rec = recs[(i + i // 2) % 2]
            feat = rec if self.packed else rec.to_dict()
            return (r.randn(1, 3, 16, 224, 224).astype(np.float32), (r.rand(157, 160 - 10 * (i % 2)) < 0.05).astype(np.float32), feat,
                    np.array([i % 2, 16, rec.frames, 1], dtype=np.int64), 'vid%d' % i, 30.0 + i)

    def go(packed):
        seen, kinds, stagers = [], [], []
        real_step, real_stager = tc.train_step, staging.HostStager

        def step(net, reducer, optimizer, inputs, labels, masks, feat, *a, **k):
            kinds.append(type(feat))
            out = real_step(net, reducer, optimizer, inputs, labels, masks, feat, *a, **k)
            seen.append((float(out[0]), float(out[1])))
            return out

        def stager(*a, **k):
            st = real_stager(*a, **k)
            real_stage = st.stage

            def stage(it):
                for batch in real_stage(it):
                    kinds.append(type(batch[3]))
                    yield batch
            st.stage = stage
            stagers.append(st)
            return st
        mk = lambda: tud.DataLoader(Videos(packed), batch_size=2, shuffle=False, num_workers=0, pin_memory=True,
                                    collate_fn=collate.coarse_collate_packed if packed else collate.coarse_collate)
        with monkeypatch.context() as mp, _Deterministic():
            mp.setattr(tc, 'train_step', step)
            mp.setattr(staging, 'HostStager', stager)
            torch.manual_seed(0)
            tc.run(batch_size=2, dataloaders={'train': mk(), 'val': mk()}, max_steps=2, pretrained=None, log=lambda *_: None,
                   save_model=str(tmp_path / 'm_'), csv_path=None)
        assert len(stagers) == 1 and stagers[0].batches >= 2
        return seen, kinds
    s_dict, k_dict = go(False)
    s_pack, k_pack = go(True)
    assert k_pack[0] is PackedFeats and k_pack[1] is dict                # staged as PackedFeats, unpacked before the step
    assert k_dict[0] is dict and k_dict[1] is dict
    print('coarse run: dict batches %s | packed batches %s' % (s_dict, s_pack))
    assert len(s_dict) == len(s_pack) == 2 and all(np.isfinite(v) for s in s_dict for v in s)
    assert s_dict == s_pack
