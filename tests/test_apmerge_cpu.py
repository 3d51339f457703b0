"""The merge rule M1-M4 of cfn_hip/apmerge.py on the host: merge_reference against plain concatenation, refusals on crafted states, the order
of a merge in the value, and gather_stores over two gloo ranks on CPU tensors.  Everything is bit-exact; nothing needs a GPU."""
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG

import apmerge_fixture as fx

C, TIOU = fx.C, fx.TIOU
WORLD = 2


def _fresh(cap, state_len=2 * C + 1, n_classes=C):
    return (np.full((n_classes, cap), fx.SENTINEL_SCORE, np.int32), np.full((n_classes, cap), fx.SENTINEL_BYTE, np.uint8), np.zeros(state_len, np.int32))


def _stack(stores, m=None):
    """numpy stores -> the (R, C, m) sources of one merge (apmerge.stack_parts on CPU tensors)"""
    from cfn_hip.apmerge import stack_parts
    parts = []
    for scores, tps, state in stores:
        counts, n_gt, flags = (torch.from_numpy(x) for x in fx.split_state(state))
        parts.append((torch.from_numpy(scores), torch.from_numpy(tps), counts, n_gt, flags))
    return stack_parts(parts, m)


def _merge(dst, stores, m=None):
    from cfn_hip.apmerge import merge_reference
    scores, tps, state = dst
    counts, n_gt, flags = fx.split_state(state)
    return merge_reference(scores, tps, counts, n_gt, flags, *_stack(stores, m))


def _assert_store_equals(got, want):
    (gs, gp, gst), (ws, wp, wst) = got, want
    assert np.array_equal(gst, wst)
    assert fx.same_rows(fx.prefixes(gs, gp, gst[:C])[0], fx.prefixes(ws, wp, wst[:C])[0])
    assert fx.same_rows(fx.prefixes(gs, gp, gst[:C])[1], fx.prefixes(ws, wp, wst[:C])[1])


def test_merge_reference_is_concatenation_in_part_order():
    from cfn_hip.segap import ap_reference
    b = fx.batches()
    whole = fx.store_from(b, 96)
    shards = [fx.store_from(b[0:1], 40), fx.store_from(b[1:3], 64), fx.store_from(b[3:4], 33)]
    assert len({tuple(s[2][:C]) for s in shards}) == 3 and min(int(s[2][:C].max()) for s in shards) > 0
    # into an empty destination, R = 3 (stack_parts reads the largest count itself), and behind the rows of shard 0, R = 2
    for dst, rest in ((_fresh(96), shards), (fx.store_from(b[0:1], 96), shards[1:])):
        assert _merge(dst, rest) is True
        _assert_store_equals(dst, whole)
        counts = dst[2][:C]
        for c in range(C):                                                            # rows behind the new counts are untouched
            assert (dst[0][c, counts[c]:] == fx.SENTINEL_SCORE).all() and (dst[1][c, counts[c]:] == fx.SENTINEL_BYTE).all()
        ref = ap_reference(b, C, TIOU)
        ap, mp_ = fx.ap_of_store(*dst)
        assert np.array_equal(ap.view(np.int32), ref['ap'].view(np.int32)) and np.array_equal(mp_.view(np.int32), ref['map'].view(np.int32))
        assert np.array_equal(dst[2][:C], ref['counts']) and np.array_equal(dst[2][C:2 * C], ref['n_gt'])
        assert ref['map'].max() > 0
    # the sources are untouched
    for s, again in zip(shards, (fx.store_from(b[0:1], 40), fx.store_from(b[1:3], 64), fx.store_from(b[3:4], 33))):
        assert all(np.array_equal(x, y) for x, y in zip(s, again))


def test_one_count_for_all_classes():
    """n_cnt == 1 (the frame meter): every class advances by the same count; no extras"""
    from cfn_hip.apmerge import merge_reference
    rng = np.random.RandomState(5)
    K, cap_s, cap_d = 3, 9, 20
    ds, dp = fx.score_bits(rng, (K, cap_d)), rng.randint(0, 256, (K, cap_d)).astype(np.uint8)
    ss, sp = fx.score_bits(rng, (2, K, cap_s)), rng.randint(0, 256, (2, K, cap_s)).astype(np.uint8)
    ds0, dp0 = ds.copy(), dp.copy()
    dc, df = np.array([4], np.int32), np.array([0], np.int32)
    assert merge_reference(ds, dp, dc, None, df, ss, sp, np.array([[9], [2]], np.int32), None, np.array([0, 1], np.int32)) is True
    assert dc[0] == 15 and df[0] == 1
    for k in range(K):
        assert np.array_equal(ds[k], np.concatenate([ds0[k, :4], ss[0, k, :9], ss[1, k, :2], ds0[k, 15:]]))
        assert np.array_equal(dp[k], np.concatenate([dp0[k, :4], sp[0, k, :9], sp[1, k, :2], dp0[k, 15:]]))


def _crafted(counts_d, counts_s, cap_d=10, cap_s=6, flags_d=0, flags_s=None, extra_d=None, extra_s=None):
    """a destination and R parts over 2 classes with the given counts -> the arguments of merge_reference, and a copy of the destination"""
    rng = np.random.RandomState(17)
    R = len(counts_s)
    ds, dp = fx.score_bits(rng, (2, cap_d)), rng.randint(0, 256, (2, cap_d)).astype(np.uint8)
    ss, sp = fx.score_bits(rng, (R, 2, cap_s)), rng.randint(0, 256, (R, 2, cap_s)).astype(np.uint8)
    de = np.array(extra_d if extra_d is not None else [1, 2], np.int32)
    se = np.array(extra_s if extra_s is not None else [[3, 4]] * R, np.int32)
    args = [ds, dp, np.array(counts_d, np.int32), de, np.array([flags_d], np.int32), ss, sp, np.array(counts_s, np.int32), se,
            np.array(flags_s if flags_s is not None else [0] * R, np.int32)]
    return args, [a.copy() for a in args[:5]]


def _unchanged_but_flags(args, before, flags):
    return all(np.array_equal(a, b) for a, b in zip(args[:4], before[:4])) and int(args[4][0]) == flags


def test_refusals_and_flags_on_crafted_states():
    from cfn_hip.apmerge import AP_FLAG_BAD_SOURCE, AP_FLAG_OVERFLOW, merge_reference
    assert (AP_FLAG_OVERFLOW, AP_FLAG_BAD_SOURCE) == (2, 4)
    # M2: class 1's total is cap_d + 1 -> nothing changes but the overflow bit; the other part's flag 1 is OR-ed in all the same (M4)
    args, before = _crafted([3, 4], [[2, 3], [1, 4]], flags_s=[0, 1])
    assert merge_reference(*args) is False and _unchanged_but_flags(args, before, 1 | AP_FLAG_OVERFLOW)
    # ... and a total that fits exactly succeeds
    args, before = _crafted([3, 4], [[2, 3], [1, 3]], flags_d=8, flags_s=[16, 1])
    assert merge_reference(*args) is True
    assert args[2].tolist() == [6, 10] and args[3].tolist() == [7, 10] and int(args[4][0]) == 8 | 16 | 1
    assert np.array_equal(args[0][1], np.concatenate([before[0][1, :4], args[5][0, 1, :3], args[5][1, 1, :3]]))
    assert np.array_equal(args[1][0], np.concatenate([before[1][0, :3], args[6][0, 0, :2], args[6][1, 0, :1], before[1][0, 6:]]))
    # M1: a count of cap_s + 1, and a count of -1 (whose total would even fit): refused with bit 4, flags OR-ed in
    for bad in ([[7, 0], [0, 0]], [[0, 0], [1, -1]]):
        args, before = _crafted([3, 4], bad, flags_s=[2, 0])
        assert merge_reference(*args) is False and _unchanged_but_flags(args, before, 2 | AP_FLAG_BAD_SOURCE)
    # M2: an extra that leaves int32
    args, before = _crafted([0, 0], [[1, 1]], extra_d=[2 ** 31 - 2, 0], extra_s=[[2, 0]])
    assert merge_reference(*args) is False and _unchanged_but_flags(args, before, AP_FLAG_OVERFLOW)
    args, before = _crafted([0, 0], [[1, 1]], extra_d=[2 ** 31 - 2, 0], extra_s=[[1, 0]])
    assert merge_reference(*args) is True and args[3].tolist() == [2 ** 31 - 1, 0]


def test_the_order_of_a_merge_decides_the_value():
    """two shards with a tied score across them: the references of the two orders differ (a condition on the inputs, checked here), and
    merge_reference reproduces each"""
    from cfn_hip.segap import ap_reference
    a, b = fx.tied_shards()
    ref_ab, ref_ba = ap_reference([a, b], C, TIOU), ap_reference([b, a], C, TIOU)
    assert not np.array_equal(ref_ab['ap'].view(np.int32), ref_ba['ap'].view(np.int32))
    assert ref_ab['ap'][1, 0] == 1.0 and ref_ba['ap'][1, 0] == 0.5
    sa, sb = fx.store_from([a], 4), fx.store_from([b], 4)
    for order, ref in (((sa, sb), ref_ab), ((sb, sa), ref_ba)):
        dst = _fresh(8)
        assert _merge(dst, order) is True
        ap, mp_ = fx.ap_of_store(*dst)
        assert np.array_equal(ap.view(np.int32), ref['ap'].view(np.int32)) and np.array_equal(mp_.view(np.int32), ref['map'].view(np.int32))


def test_the_all_ranks_flag_and_the_world_size_check():
    """--seg-ap-all-ranks: off by default, travels to the workers' command line; check_segment_ap lets an across_ranks meter pass a world
    size above 1 and keeps refusing any other"""
    import argparse
    import types
    sys.path.insert(0, PKG)
    import train_fine
    parser = argparse.ArgumentParser()
    train_fine.seg_ap_arguments(parser)
    on, off = parser.parse_args(['--seg-ap', '--seg-ap-all-ranks']), parser.parse_args(['--seg-ap'])
    assert on.seg_ap_all_ranks is True and off.seg_ap_all_ranks is False
    assert train_fine.seg_ap_argv(on)[-1] == '--seg-ap-all-ranks' and '--seg-ap-all-ranks' not in train_fine.seg_ap_argv(off)
    assert train_fine.seg_ap_argv(parser.parse_args(['--seg-ap-all-ranks'])) == []
    train_fine.check_segment_ap(types.SimpleNamespace(across_ranks=True), 2)
    train_fine.check_segment_ap(types.SimpleNamespace(across_ranks=False), 1)
    for plain in (types.SimpleNamespace(across_ranks=False), object()):
        with pytest.raises(RuntimeError, match='ONE process.*--seg-ap-all-ranks'):
            train_fine.check_segment_ap(plain, 2)


# ---- gather_stores over gloo: two spawned CPU ranks -----------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_batches(case):
    """what each of the two ranks was fed, (batches, capacity of its stores, its flags)"""
    b = fx.batches()
    only_class_0 = fx.tied_shards()[1]
    if case == 'uneven':                 # different counts; rank 1 holds rows of class 0 only, in stores shorter than rank 0's fullest class
        return [(b[0:3], 64, 0), ([only_class_0], 2, 1)]
    if case == 'one_empty':              # rank 0 holds nothing at all
        return [([], 7, 2), (b[1:4], 50, 0)]
    return [([], 3, 0), ([], 5, 0)]      # 'both_empty'


def _gather_worker(rank, port, case, out):
    sys.path.insert(0, PKG)
    torch.cuda.is_available = lambda: False                # (this worker never opens the GPU)
    import torch.distributed as dist
    from cfn_hip.apmerge import gather_stores, merge_reference
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=WORLD)
    try:
        batches, cap, flags = _rank_batches(case)[rank]
        scores, tps, state = fx.store_from(batches, cap, flags=flags)
        mine = [x.copy() for x in (scores, tps, state)]
        got = gather_stores(torch.from_numpy(scores).view(torch.float32), torch.from_numpy(tps), torch.from_numpy(state), C, None, merge=merge_reference)
        assert all(np.array_equal(x, y) for x, y in zip((scores, tps, state), mine))       # this rank's stores are untouched
        out[rank] = (got[0].view(torch.int32).numpy().copy(), got[1].numpy().copy(), got[2].numpy().copy())
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('case', ['uneven', 'one_empty', 'both_empty'])
def test_gather_stores_over_two_gloo_ranks(case):
    out = mp.Manager().dict()
    mp.spawn(_gather_worker, args=(_free_port(), case, out), nprocs=WORLD, join=True)
    per_rank = _rank_batches(case)
    counts = [fx.store_from(bt, cap)[2][:C] for bt, cap, _ in per_rank]
    if case == 'uneven':
        assert counts[0].tolist() != counts[1].tolist() and counts[1][1:].max() == 0 and counts[1][0] > 0 and counts[0][1:].min() > 0
    elif case == 'one_empty':
        assert counts[0].max() == 0 and counts[1].max() > 0
    else:
        assert counts[0].max() == 0 and counts[1].max() == 0
    total = int((counts[0].astype(np.int64) + counts[1]).max())
    want = fx.store_from(per_rank[0][0] + per_rank[1][0], max(total, 1), flags=per_rank[0][2] | per_rank[1][2])
    for rank in range(WORLD):
        got = out[rank]
        assert got[0].shape == (C, max(total, 1))                                     # a fresh store sized by the largest per-class total
        _assert_store_equals(got, want)
    _assert_store_equals(out[0], out[1])                                              # every rank holds the same bits
