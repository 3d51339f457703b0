"""GPU: cfn_ap_merge (csrc/apmerge.hip) against merge_reference of cfn_hip/apmerge.py, the meters' merge / merged / across_ranks, capture and
the training entry points.  Everything is compared as bits (int32 / uint8); no test uses a tolerance."""
import os

import numpy as np
import pytest
import torch

import apmerge_fixture as fx

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C, TIOU = fx.C, fx.TIOU
CANARY_I, CANARY_B = np.int32(0x5ca1ab1e), np.uint8(0xc3)


def _tile():
    from cfn_hip import load, ops
    assert load().cfn_ap_merge_tile() == ops.AP_MERGE_TILE
    return ops.AP_MERGE_TILE


class _Case(object):
    """a destination inside larger buffers (canaries in front and behind, sentinels behind the counts) and R parts, on the host; run() does
    the merge on the device and with merge_reference and compares EVERY byte of the buffers, counts, extras and flags"""

    def __init__(self, seed, n_classes, cap_d, cap_s, dst_counts, part_counts, n_extra=None, front_s=4, front_p=8, src_front_p=0, flags_d=0,
                 flags_s=None, extra_d=None, extra_s=None):
        rng = np.random.RandomState(seed)
        K, R = n_classes, len(part_counts)
        self.K, self.R, self.cap_d, self.cap_s = K, R, cap_d, cap_s
        self.front_s, self.front_p, self.src_front_p = front_s, front_p, src_front_p
        self.dc = np.array(dst_counts, np.int32).reshape(-1)
        self.sc = np.array(part_counts, np.int32).reshape(R, -1)
        n_cnt = self.dc.shape[0]
        assert n_cnt in (1, K) and self.sc.shape[1] == n_cnt
        n_extra = (K if n_cnt == K else 0) if n_extra is None else n_extra
        self.de = None if n_extra == 0 else (rng.randint(0, 1000, n_extra).astype(np.int32) if extra_d is None else np.array(extra_d, np.int32))
        self.se = None if n_extra == 0 else (rng.randint(0, 1000, (R, n_extra)).astype(np.int32) if extra_s is None else np.array(extra_s, np.int32))
        self.df = np.array([flags_d], np.int32)
        self.sf = np.array(flags_s if flags_s is not None else [0] * R, np.int32)
        self.big_s = np.full(front_s + K * cap_d + 5, CANARY_I, np.int32)
        self.big_p = np.full(front_p + K * cap_d + 7, CANARY_B, np.uint8)
        ds, dp = self.dst_views(self.big_s, self.big_p)
        ds[:], dp[:] = fx.SENTINEL_SCORE, fx.SENTINEL_BYTE
        for c in range(K):
            n = int(np.clip(self.dc[0 if n_cnt == 1 else c], 0, cap_d))
            ds[c, :n], dp[c, :n] = fx.score_bits(rng, (n,)), rng.randint(0, 256, n)
        self.src_s = fx.score_bits(rng, (R, K, cap_s))
        self.src_p = np.full(src_front_p + R * K * cap_s, CANARY_B, np.uint8)
        self.src_p[src_front_p:] = rng.randint(0, 256, R * K * cap_s)

    def dst_views(self, big_s, big_p):
        n = self.K * self.cap_d
        return big_s[self.front_s:self.front_s + n].reshape(self.K, self.cap_d), big_p[self.front_p:self.front_p + n].reshape(self.K, self.cap_d)

    def src_payload(self, flat):
        return flat[self.src_front_p:].reshape(self.R, self.K, self.cap_s)

    def alignments(self, dst_ptr, src_ptr):
        """the (source, destination) byte alignment of every (part, class) copy that has a body, from the device pointers and the rule's rows"""
        pairs = set()
        n_cnt = self.dc.shape[0]
        for c in range(self.K):
            at = int(self.dc[0 if n_cnt == 1 else c])
            for r in range(self.R):
                n = int(self.sc[r, 0 if n_cnt == 1 else c])
                if n >= 8:
                    pairs.add(((src_ptr + (r * self.K + c) * self.cap_s) & 3, (dst_ptr + c * self.cap_d + at) & 3))
                at += n
        return pairs

    def run(self, out=None):
        from cfn_hip import ops
        from cfn_hip.apmerge import merge_reference
        want_s, want_p = self.big_s.copy(), self.big_p.copy()
        w_dc, w_df = self.dc.copy(), self.df.copy()
        w_de = None if self.de is None else self.de.copy()
        ws, wp = self.dst_views(want_s, want_p)
        ok = merge_reference(ws, wp, w_dc, w_de, w_df, self.src_s, self.src_payload(self.src_p), self.sc, self.se, self.sf)
        dev = lambda a: None if a is None else torch.from_numpy(a.copy()).to(DEV)
        big_s, big_p, src_p_flat = dev(self.big_s), dev(self.big_p), dev(self.src_p)
        ds, dp = self.dst_views(big_s, big_p)
        dc, de, df = dev(self.dc), dev(self.de), dev(self.df)
        src_p = self.src_payload(src_p_flat)
        ops.ap_merge(ds.view(torch.float32), dp, dc, de, df, dev(self.src_s).view(torch.float32), src_p, dev(self.sc), dev(self.se), dev(self.sf), out=out)
        got_s, got_p = big_s.cpu().numpy(), big_p.cpu().numpy()
        assert np.array_equal(got_s, want_s), 'scores, canaries or sentinels differ'
        assert np.array_equal(got_p, want_p), 'payload, canaries or sentinels differ'
        assert np.array_equal(dc.cpu().numpy(), w_dc) and np.array_equal(df.cpu().numpy(), w_df)
        assert de is None or np.array_equal(de.cpu().numpy(), w_de)
        assert (got_s[:self.front_s] == CANARY_I).all() and (got_s[-5:] == CANARY_I).all()
        assert (got_p[:self.front_p] == CANARY_B).all() and (got_p[-7:] == CANARY_B).all()
        assert np.array_equal(src_p_flat.cpu().numpy(), self.src_p)                    # the sources are untouched
        self.pairs = self.alignments(dp.data_ptr(), src_p.data_ptr())
        self.after = (got_s, got_p, w_dc, w_de, w_df)
        return ok


def _cycled_counts(R, n_cnt, cap_s, shift):
    T = _tile()
    cand = [n for n in (0, 1, 2, 3, 4, 5, T - 1, T, T + 1, cap_s) if n <= cap_s]
    return [[cand[(r * n_cnt + j + shift) % len(cand)] for j in range(n_cnt)] for r in range(R)]


@pytest.mark.parametrize('per_class', [False, True])
@pytest.mark.parametrize('R', [1, 2, 3])
@pytest.mark.parametrize('cap_s', [1, 7, 64, 257, 'two_tiles_and_3'])
def test_kernel_against_the_reference(cap_s, R, per_class):
    cap_s = 2 * _tile() + 3 if cap_s == 'two_tiles_and_3' else cap_s
    n_cnt = C if per_class else 1
    parts = _cycled_counts(R, n_cnt, cap_s, shift=R + cap_s)
    dst = [(3 * j + R + cap_s) % 7 for j in range(n_cnt)]
    cap_d = max(d + sum(p[j] for p in parts) for j, d in enumerate(dst)) + 3
    cap_d += 1 - cap_d % 2                                                            # odd: the rows of the classes start at every alignment
    case = _Case(1000 * R + cap_s, C, cap_d, cap_s, dst, parts, front_s=4 + R, front_p=8 + R, src_front_p=cap_s % 4, flags_d=8, flags_s=[16] + [0] * (R - 1))
    assert case.run() is True


def test_one_hundred_and_fifty_seven_classes():
    rng = np.random.RandomState(3)
    parts = rng.randint(0, 258, (2, 157)).tolist()
    dst = rng.randint(0, 40, 157).tolist()
    assert _Case(157, 157, 40 + 2 * 257 + 1, 257, dst, parts).run() is True


@pytest.mark.parametrize('per_class', [False, True])
def test_every_source_and_destination_byte_alignment(per_class):
    """capacities that are multiples of 4 and 16-byte aligned allocations: the source alignment is the source buffer's offset, the
    destination's is the offset plus the destination count -- all 4 x 4 pairs, checked from the device pointers"""
    seen = set()
    for sa in range(4):
        for da in range(4):
            dst = [da + 4 * ((c + sa) % 3) for c in range(C)] if per_class else [da + 4 * sa]
            parts = [[37 + 4 * (c % 2) for c in range(C)], [22] * C] if per_class else [[37], [22]]
            case = _Case(10 * sa + da, C, 200, 64, dst, parts, front_p=16, src_front_p=sa)
            assert case.run() is True
            assert (sa, da) in case.pairs, (sa, da, case.pairs)
            seen |= case.pairs
    assert seen == {(s, d) for s in range(4) for d in range(4)}


def test_part_counts_on_the_tile_edges():
    T = _tile()
    cap_s = 2 * T + 3
    edges = [0, 1, 2, 3, 4, 5, T - 1, T, T + 1, cap_s]
    parts = [edges[:5], edges[5:]]
    assert _Case(1, C, 5 + 2 * cap_s, cap_s, [1, 2, 3, 0, 5], parts, src_front_p=1).run() is True
    for n in (T - 1, T, T + 1, cap_s):                                               # one count for all classes
        assert _Case(n, C, 2 + n + 3 + 1, cap_s, [2], [[n], [3]], src_front_p=2).run() is True


def test_refusals_on_the_device():
    from cfn_hip import ops
    assert (ops.AP_FLAG_OVERFLOW, ops.AP_FLAG_BAD_SOURCE) == (2, 4)
    # one row too many in class 3 of part 1: the whole buffer, counts and extras are bit-equal to before (run() compares them with the
    # reference, which changed nothing), and the flag is set -- the other part's flag all the same
    case = _Case(1, C, 30, 12, [5, 6, 7, 9, 9], [[10, 10, 10, 10, 10], [1, 2, 3, 12, 4]], flags_s=[0, 1])      # class 3: 9 + 10 + 12 = 31 > 30
    before = (case.big_s.copy(), case.big_p.copy())
    assert case.run() is False
    assert np.array_equal(case.after[0], before[0]) and np.array_equal(case.after[1], before[1])
    assert np.array_equal(case.after[2], case.dc) and np.array_equal(case.after[3], case.de) and int(case.after[4][0]) == 1 | ops.AP_FLAG_OVERFLOW
    # the exact fit succeeds
    case = _Case(2, C, 30, 12, [5, 6, 7, 8, 9], [[10, 10, 10, 10, 10], [1, 2, 3, 12, 4]], flags_s=[0, 1])
    assert case.run() is True and case.after[2].tolist() == [16, 18, 20, 30, 23] and int(case.after[4][0]) == 1
    # a source count of cap_s + 1, and one of -1: refused with bit 4, nothing changes, flags propagate
    for bad in (13, -1):
        case = _Case(3, C, 30, 12, [0, 0, 0, 0, 0], [[1, 1, 1, 1, 1], [1, 1, bad, 1, 1]], flags_d=1, flags_s=[2, 0])
        before = (case.big_s.copy(), case.big_p.copy())
        assert case.run() is False
        assert np.array_equal(case.after[0], before[0]) and np.array_equal(case.after[1], before[1])
        assert np.array_equal(case.after[2], case.dc) and np.array_equal(case.after[3], case.de) and int(case.after[4][0]) == 1 | 2 | ops.AP_FLAG_BAD_SOURCE
    # a summed extra that leaves int32 (one count for all classes, three extras)
    case = _Case(4, C, 30, 12, [5], [[3], [4]], n_extra=3, extra_d=[1, 2 ** 31 - 10, 3], extra_s=[[1, 5, 1], [1, 5, 1]])
    assert case.run() is False and int(case.after[4][0]) == ops.AP_FLAG_OVERFLOW
    case = _Case(4, C, 30, 12, [5], [[3], [4]], n_extra=3, extra_d=[1, 2 ** 31 - 11, 3], extra_s=[[1, 5, 1], [1, 5, 1]])
    assert case.run() is True and case.after[3].tolist() == [3, 2 ** 31 - 1, 5]


def test_arguments_are_checked():
    from cfn_hip import ops
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
    ds, dp, ss, sp = z(C, 8, dt=torch.float32), z(C, 8, dt=torch.uint8), z(2, C, 4, dt=torch.float32), z(2, C, 4, dt=torch.uint8)
    good = [ds, dp, z(C), z(C), z(1), ss, sp, z(2, C), z(2, C), z(2)]
    ops.ap_merge(*good)
    with pytest.raises(RuntimeError, match='n_cnt|dst_counts'):
        ops.ap_merge(*(good[:2] + [z(2)] + good[3:7] + [z(2, 2)] + good[8:]))
    with pytest.raises(RuntimeError, match='overlap'):
        both = z(3, C, 4, dt=torch.float32)
        ops.ap_merge(both[0], dp[:, :4].contiguous(), *good[2:5], both[:2], *good[6:])
    with pytest.raises(RuntimeError, match='workspace'):
        ops.ap_merge(*good, out=torch.empty(ops.ap_merge_workspace_bytes(2, C) + 8, dtype=torch.uint8, device=DEV)[1:])
    with pytest.raises(RuntimeError, match='CPU|device'):
        ops.ap_merge(*([ds.cpu()] + good[1:]))
    assert ops.ap_merge_workspace_bytes(2, C) >= 8 + 8 * 2 * C
    with pytest.raises(RuntimeError):
        ops.ap_merge_workspace_bytes(0, C)


# ---- the meters -------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(xs, ys):
    """tensors equal as BITS (a store's rows behind its count are whatever the allocation held: NaNs among them)"""
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(xs, ys))


def _seg_meter(**kw):
    from cfn_hip.segap import SegmentAPMeter
    return SegmentAPMeter(DEV, C, TIOU, **kw)


def _fed(meter, batch_list):
    for det, gt in batch_list:
        meter.add(det.to(DEV), gt.to(DEV))
    return meter


def _same_segment_meter(got, want):
    assert torch.equal(got.counts, want.counts) and torch.equal(got.n_gt, want.n_gt) and torch.equal(got.flags, want.flags)
    for c in range(C):
        k = int(want.counts[c])
        assert torch.equal(_bits(got.stores[0][c, :k]), _bits(want.stores[0][c, :k])) and torch.equal(got.stores[1][c, :k], want.stores[1][c, :k])
    v, w = got.value(), want.value()
    assert torch.equal(_bits(v[0]), _bits(w[0])) and torch.equal(_bits(v[1]), _bits(w[1]))
    return w


def test_segment_meters_merge_like_one_meter(monkeypatch):
    from cfn_hip import ops
    from cfn_hip.segap import SegmentAPMeter, ap_reference
    b = fx.batches()
    one, a, bb = _fed(_seg_meter(), b), _fed(_seg_meter(), b[:2]), _fed(_seg_meter(), b[2:])
    b_stores = [x.clone() for x in bb.stores] + [bb._state.clone()]
    assert a.merge(bb) is a
    w = _same_segment_meter(a, one)
    ref = ap_reference(b, C, TIOU)
    assert np.array_equal(_bits(w[0]).numpy(), ref['ap'].view(np.int32)) and ref['map'].max() > 0
    assert _same(b_stores, list(bb.stores) + [bb._state])                             # the source meter is untouched
    # list order: [b, a] is a meter fed 2, 3, 0, 1
    a2 = _fed(_seg_meter(), b[:2])
    _same_segment_meter(SegmentAPMeter.merged([bb, a2]), _fed(_seg_meter(), b[2:] + b[:2]))
    # three parts, ONE call with R = 3
    calls = []
    real = ops.ap_merge
    monkeypatch.setattr(ops, 'ap_merge', lambda *args, **kw: calls.append(int(args[5].shape[0])) or real(*args, **kw))
    parts = [_fed(_seg_meter(), b[:1]), _fed(_seg_meter(capacity=80), b[1:3]), _fed(_seg_meter(), b[3:])]
    _same_segment_meter(SegmentAPMeter.merged(parts), one)
    assert calls == [3]
    # the tied shards: the order is visible in the value, as the reference says it must be
    ta, tb = fx.tied_shards()
    one_t, ma, mb = _fed(_seg_meter(), [ta, tb]), _fed(_seg_meter(), [ta]), _fed(_seg_meter(), [tb])
    ba, ab = SegmentAPMeter.merged([mb, ma]).value(), one_t.value()
    assert not torch.equal(_bits(ba[0]), _bits(ab[0]))
    assert np.array_equal(_bits(ba[0]).numpy(), ap_reference([tb, ta], C, TIOU)['ap'].view(np.int32))
    assert np.array_equal(_bits(ab[0]).numpy(), ap_reference([ta, tb], C, TIOU)['ap'].view(np.int32))
    _same_segment_meter(SegmentAPMeter.merged([ma, mb]), one_t)


def test_segment_meter_merge_refuses_other_settings_and_reports_an_overflow():
    from cfn_hip.segap import SegmentAPMeter
    b = fx.batches()
    a = _fed(_seg_meter(), b[:1])
    for other in (SegmentAPMeter(DEV, C + 1, TIOU), SegmentAPMeter(DEV, C, (0.3, 0.5)), SegmentAPMeter(DEV, C, TIOU, score='mean')):
        with pytest.raises(ValueError, match='same classes, tiou and score'):
            a.merge(other)
    with pytest.raises(ValueError, match='itself'):
        a.merge(a)
    fullest = int(a.counts.max())
    small = _fed(_seg_meter(capacity=2 * fullest - 1), b[:1])
    before = [x.clone() for x in small.stores] + [small._state.clone()]
    small.merge(a)                                                                    # fixed capacity: no read-back, all or nothing
    assert _same(before[:2], small.stores) and torch.equal(small._state[:-1], before[2][:-1])
    with pytest.raises(RuntimeError, match='did not fit the fixed capacity'):
        small.value()
    exact = _fed(_seg_meter(capacity=2 * fullest), b[:1]).merge(a)
    _same_segment_meter(exact, _fed(_seg_meter(), b[:1] + b[:1]))


def _frame_batches():
    """four batches (B, K = 3, TL) of probs on a grid of sixteenths (ties inside and across batches) and binary labels, with valid lengths"""
    rng = np.random.RandomState(21)
    out = []
    for B, TL in ((2, 50), (3, 17), (1, 64), (2, 33)):
        probs = torch.from_numpy(rng.randint(0, 17, (B, 3, TL)).astype(np.float32) / 16.0)
        labels = torch.from_numpy((rng.rand(B, 3, TL) < 0.3).astype(np.float32))
        valid = torch.from_numpy(rng.randint(TL // 2, TL + 1, B).astype(np.int32))
        out.append((probs, labels, valid))
    return out


def _frame_fed(meter, batch_list):
    for probs, labels, valid in batch_list:
        meter.add_batch(probs.to(DEV), labels.to(DEV), valid.to(DEV))
    return meter


def _same_frame_meter(got, want):
    assert torch.equal(got._state, want._state)
    k = int(want.count)
    assert torch.equal(_bits(got.stores[0][:, :k]), _bits(want.stores[0][:, :k])) and torch.equal(got.stores[1][:, :k], want.stores[1][:, :k])
    v, w = got.value(), want.value()
    assert torch.equal(_bits(v), _bits(w)) and float(w.max()) > 0
    return w


def test_frame_meters_merge_like_one_meter(monkeypatch):
    from apmeter import DeviceAPMeter
    from cfn_hip import ops
    b = _frame_batches()
    one, a, bb = _frame_fed(DeviceAPMeter(DEV), b), _frame_fed(DeviceAPMeter(DEV), b[:2]), _frame_fed(DeviceAPMeter(DEV), b[2:])
    assert a.merge(bb) is a
    _same_frame_meter(a, one)
    _same_frame_meter(DeviceAPMeter.merged([bb, _frame_fed(DeviceAPMeter(DEV), b[:2])]), _frame_fed(DeviceAPMeter(DEV), b[2:] + b[:2]))
    calls = []
    real = ops.ap_merge
    monkeypatch.setattr(ops, 'ap_merge', lambda *args, **kw: calls.append(int(args[5].shape[0])) or real(*args, **kw))
    parts = [_frame_fed(DeviceAPMeter(DEV), b[:1]), _frame_fed(DeviceAPMeter(DEV, capacity=300), b[1:3]), _frame_fed(DeviceAPMeter(DEV), b[3:])]
    _same_frame_meter(DeviceAPMeter.merged(parts), one)
    assert calls == [3]
    with pytest.raises(ValueError, match='one class count'):
        a.merge(_frame_fed(DeviceAPMeter(DEV), [(torch.rand(1, 4, 8), torch.zeros(1, 4, 8), torch.tensor([8], dtype=torch.int32))]))


def test_frame_meter_growing_merge_reallocates_and_a_fixed_capacity_overflows():
    from apmeter import DeviceAPMeter
    rng = np.random.RandomState(4)
    rows = DeviceAPMeter.MIN_CAPACITY // 2 + 100
    big = [(torch.from_numpy(rng.randint(0, 9, (1, 3, rows)).astype(np.float32) / 8.0), torch.from_numpy((rng.rand(1, 3, rows) < 0.5).astype(np.float32)),
            torch.tensor([rows - i], dtype=torch.int32)) for i in range(2)]
    a, bb = _frame_fed(DeviceAPMeter(DEV), big[:1]), _frame_fed(DeviceAPMeter(DEV), big[1:])
    assert a.stores[0].shape[1] == DeviceAPMeter.MIN_CAPACITY
    a.merge(bb)
    assert a.stores[0].shape[1] >= 2 * rows > DeviceAPMeter.MIN_CAPACITY              # a new allocation, the rows held copied over
    _same_frame_meter(a, _frame_fed(DeviceAPMeter(DEV), big))
    b = _frame_batches()
    n0, n1 = int(b[0][2].sum()), int(b[1][2].sum())
    fixed = _frame_fed(DeviceAPMeter(DEV, capacity=n0 + n1 - 1), b[:1])
    before = [x.clone() for x in fixed.stores]
    fixed.merge(_frame_fed(DeviceAPMeter(DEV), b[1:2]))
    assert int(fixed.count) == n0 and _same(before, fixed.stores)
    with pytest.raises(RuntimeError, match='fixed capacity'):
        fixed.value()
    exact = _frame_fed(DeviceAPMeter(DEV, capacity=n0 + n1), b[:1]).merge(_frame_fed(DeviceAPMeter(DEV), b[1:2]))
    _same_frame_meter(exact, _frame_fed(DeviceAPMeter(DEV), b[:2]))


def test_frame_meter_without_a_batch_merges_both_ways():
    from apmeter import DeviceAPMeter
    b = _frame_batches()
    a = _frame_fed(DeviceAPMeter(DEV), b[:2])
    into = DeviceAPMeter(DEV).merge(a)                                                # into a meter that has no stores yet
    _same_frame_meter(into, a)
    state = a._state.clone()
    a.merge(DeviceAPMeter(DEV))                                                       # of a meter that has none: nothing changes
    assert torch.equal(a._state, state)
    nothing = DeviceAPMeter(DEV).merge(DeviceAPMeter(DEV), DeviceAPMeter(DEV))
    assert nothing.value() == 0 and nothing.stores == (None, None)
    _same_frame_meter(DeviceAPMeter.merged([DeviceAPMeter(DEV), a, DeviceAPMeter(DEV)]), a)


def test_across_ranks_under_a_process_group_of_one_rank_changes_nothing(monkeypatch):
    import torch.distributed as dist
    from apmeter import DeviceAPMeter
    from cfn_hip import apmerge
    with pytest.raises(ValueError, match='n_classes'):
        DeviceAPMeter(DEV, across_ranks=True)
    sb, fb = fx.batches(), _frame_batches()
    plain_s, across_s = _fed(_seg_meter(), sb[:3]), _fed(_seg_meter(across_ranks=True), sb[:3])
    plain_f, across_f = _frame_fed(DeviceAPMeter(DEV), fb[:3]), _frame_fed(DeviceAPMeter(DEV, across_ranks=True, n_classes=3), fb[:3])
    without_group = across_s.value()
    gathers = []
    real = apmerge.gather_stores
    monkeypatch.setattr(apmerge, 'gather_stores', lambda *a, **k: gathers.append(1) or real(*a, **k))
    created = False
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29541')
        dist.init_process_group('nccl', rank=0, world_size=1)
        created = True
    try:
        ptrs = [t.data_ptr() for t in across_s.stores + across_f.stores]
        held = [t.clone() for t in across_s.stores + across_f.stores] + [across_s._state.clone(), across_f._state.clone()]
        vs, ws = across_s.value(), plain_s.value()
        assert torch.equal(_bits(vs[0]), _bits(ws[0])) and torch.equal(_bits(vs[1]), _bits(ws[1])) and torch.equal(_bits(vs[0]), _bits(without_group[0]))
        assert torch.equal(_bits(across_f.value()), _bits(plain_f.value()))
        assert torch.equal(_bits(across_f.value_device()), _bits(plain_f.value_device()))
        assert not gathers                                                            # a world size of 1: nothing is gathered or copied
        assert ptrs == [t.data_ptr() for t in across_s.stores + across_f.stores]
        assert _same(held, list(across_s.stores + across_f.stores) + [across_s._state, across_f._state])
        # usable afterwards: one more batch each, and a reset
        _same_segment_meter(_fed(across_s, sb[3:]), _fed(plain_s, sb[3:]))
        _same_frame_meter(_frame_fed(across_f, fb[3:]), _frame_fed(plain_f, fb[3:]))
        across_f.reset()
        assert across_f.value() == 0
        # the gather itself, one rank: the stores of "all ranks" are this rank's
        gs, gp, gstate = real(across_s.stores[0], across_s.stores[1], across_s._state, C, dist.group.WORLD)
        assert torch.equal(gstate, across_s._state) and gs.shape[1] == int(across_s.counts.max())
        for c in range(C):
            k = int(across_s.counts[c])
            assert torch.equal(_bits(gs[c, :k]), _bits(across_s.stores[0][c, :k])) and torch.equal(gp[c, :k], across_s.stores[1][c, :k])
    finally:
        if created:
            dist.destroy_process_group()


def _captured_graph_shape(fn):
    """capture fn() on a stream of its own through the HIP runtime this process already holds -> (nodes, [(from, to), ...]) of the graph"""
    import ctypes
    path = next(line.split()[-1] for line in open('/proc/self/maps') if 'libamdhip64' in line)
    hip = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphDestroy.argtypes = [vp]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = vp()
    with torch.cuda.stream(stream):
        assert hip.hipStreamBeginCapture(stream.cuda_stream, 1) == 0                   # (1: thread-local capture mode)
        try:
            fn()
        finally:
            rc = hip.hipStreamEndCapture(stream.cuda_stream, ctypes.byref(graph))
    assert rc == 0 and graph.value
    try:
        n_nodes, n_edges = sz(0), sz(0)
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n_nodes)) == 0
        assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n_edges)) == 0
        src, dst = (vp * max(n_edges.value, 1))(), (vp * max(n_edges.value, 1))()
        if n_edges.value:
            assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(n_edges)) == 0
        return n_nodes.value, [(src[i], dst[i]) for i in range(n_edges.value)]
    finally:
        hip.hipGraphDestroy(graph)


@pytest.mark.capture
def test_merge_with_a_workspace_is_capturable_as_one_linear_chain():
    """out= and fixed capacities: nothing is allocated and nothing waits, so a graph holds the merge.  Replayed for two source contents (and a
    destination reset in front of each replay), each replay equals the eager result; the captured graph is one chain: no node has two
    successors or two predecessors"""
    from cfn_hip import ops
    from cfn_hip.apmerge import merge_reference
    rng = np.random.RandomState(9)
    R, cap_s, cap_d = 2, 300, 700
    z = lambda a: torch.from_numpy(a).to(DEV)
    dst0 = (fx.score_bits(rng, (C, cap_d)), rng.randint(0, 256, (C, cap_d)).astype(np.uint8), np.array([3, 0, 50, 7, 99], np.int32),
            np.array([1, 2, 3, 4, 5], np.int32), np.array([0], np.int32))
    contents = [(fx.score_bits(rng, (R, C, cap_s)), rng.randint(0, 256, (R, C, cap_s)).astype(np.uint8), rng.randint(0, cap_s + 1, (R, C)).astype(np.int32),
                 rng.randint(0, 9, (R, C)).astype(np.int32), np.array([0, i], np.int32)) for i in range(2)]
    dst = [z(x.copy()) for x in dst0]
    src = [z(x.copy()) for x in contents[0]]
    ws = torch.empty(ops.ap_merge_workspace_bytes(R, C), dtype=torch.uint8, device=DEV)
    args = lambda d, s: (d[0].view(torch.float32), d[1], d[2], d[3], d[4], s[0].view(torch.float32), s[1], s[2], s[3], s[4])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.ap_merge(*args(dst, src), out=ws)
    for content in contents:
        for t, x in zip(dst, dst0):
            t.copy_(z(x.copy()))
        for t, x in zip(src, content):
            t.copy_(z(x.copy()))
        g.replay()
        torch.cuda.synchronize()
        eager_d, eager_s = [z(x.copy()) for x in dst0], [z(x.copy()) for x in content]
        ops.ap_merge(*args(eager_d, eager_s))
        want = [x.copy() for x in dst0]
        assert merge_reference(*want, *content) is True
        for got, eager, w in zip(dst, eager_d, want):
            assert torch.equal(got, eager) and np.array_equal(got.cpu().numpy(), w)
    # the structure: two kernel nodes, one edge -- plan, then copy; no node has two successors or two predecessors
    for t, x in zip(dst, dst0):
        t.copy_(z(x.copy()))
    nodes, edges = _captured_graph_shape(lambda: ops.ap_merge(*args(dst, src), out=ws))
    assert nodes == 2 and len(edges) == 1 and edges[0][0] != edges[0][1]
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges)


# ---- the training entry points ----------------------------------------------------------------------------------------------------------------
def test_train_fine_logs_the_same_line_with_an_across_ranks_meter(tmp_path, monkeypatch):
    import argparse
    import torch.utils.data as tud
    import collate
    import train_fine
    from cfn_hip.segap import SegmentAPMeter
    from test_hip_detections import _SegVideos, _run
    crop, tiou = 64, (0.1, 0.5)

    def go(tag, meter):
        mk = lambda n, bs: tud.DataLoader(_SegVideos(n, crop, False), batch_size=bs, shuffle=False, num_workers=0, pin_memory=True,
                                          collate_fn=collate.fine_collate_u8)
        return _run(train_fine, monkeypatch, {'train': mk(2, 2), 'val': mk(3, 1)}, None, max_epochs=4, save_model=str(tmp_path / (tag + '_')),
                    segment_ap=meter)
    plain = SegmentAPMeter(DEV, 157, tiou, thr=0.5, max_gap=2, min_len=2)
    across = SegmentAPMeter(DEV, 157, tiou, thr=0.5, max_gap=2, min_len=2, across_ranks=True)
    losses, lines, _ = go('across', across)
    losses0, lines0, _ = go('plain', plain)
    assert len(lines) == 2 and lines[1].startswith(' Epoch:4 val seg-mAP@0.1: ') and lines == lines0 and losses == losses0
    train_fine.check_segment_ap(across, 2)
    train_fine.check_segment_ap(None, 2)
    with pytest.raises(RuntimeError, match='ONE process.*--seg-ap-all-ranks'):
        train_fine.check_segment_ap(plain, 2)
    # the flag: --seg-ap-all-ranks makes the meter across_ranks, travels to the workers' command line, and is off by default
    parser = argparse.ArgumentParser()
    train_fine.add_detect_args(parser)
    train_fine.seg_ap_arguments(parser)
    on, off = parser.parse_args(['--seg-ap', '--seg-ap-all-ranks']), parser.parse_args(['--seg-ap'])
    assert train_fine.seg_ap_from_args(on).across_ranks is True and train_fine.seg_ap_from_args(off).across_ranks is False
    assert '--seg-ap-all-ranks' in train_fine.seg_ap_argv(on) and '--seg-ap-all-ranks' not in train_fine.seg_ap_argv(off)
