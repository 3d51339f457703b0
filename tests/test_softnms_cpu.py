"""Soft-NMS, host side (cfn_hip/detections.py): decay_exp_reference against exp, soft_nms_reference on hand-worked cases with the expected
doubles typed out operation by operation, against a second, row-by-row spelling of the rule (softnms_fixture.soft_loop), the identities of
rule S7, the C ABI of cfn_soft_nms_segments, the refusals of the op, and the writer's, the meter's and the scripts' new option.  Every
comparison of results is exact: the rule is fp64 products in a stated order.  No GPU."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

import segap_fixture as fx
from proposals_fixture import LEVELS5, candidates, random_probs
from softnms_fixture import FLOOR, SIZES, SUBNORMAL_KEEP, boundary_batch, first_rows, same_det, soft_loop, subnormal_batch

F = np.float64
CHAIN = [(0, 0, 10, 0.9, 0.1), (0, 4, 14, 0.8, 0.2), (0, 8, 18, 0.7, 0.3)]      # tIoU AB = BC = 6/14, AC = 2/18


def _lib():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return cfn_hip


def _soft(rows, soft, nms_thr=0.5, score='max', C=1, **kw):
    """soft_nms_reference of ONE video's rows -> (keep list, the score column of the result as float32 numpy, the result)"""
    from cfn_hip.detections import SCORE_COLUMNS, SoftNMS, soft_nms_reference
    det = fx.make_det([rows], C)
    out, keep, src = soft_nms_reference(det, SoftNMS(*soft), nms_thr, score, **kw)
    n = out.check()
    assert keep.dtype == torch.uint8 and src.dtype == torch.int32 and out.offsets.tolist() == [0, n] and int(keep.sum()) == n
    assert src[:n].tolist() == torch.nonzero(keep).flatten().tolist()                  # S6: input order
    other = 1 - SCORE_COLUMNS[score]
    assert torch.equal(out.seg[:n], det.seg[src[:n].long()]) and torch.equal(out.score[:n, other], det.score[src[:n].long(), other])
    return keep.tolist(), out.score[:n, SCORE_COLUMNS[score]].numpy(), out


def test_decay_exp_is_exp_to_1e_12_and_exact_at_0():
    from cfn_hip.detections import decay_exp_reference as E
    assert E(0.0) == 1.0 and E(np.zeros(3)).tolist() == [1.0] * 3
    t = np.concatenate([np.linspace(0.0, 64.0, 20001), np.float64(2.0) ** -np.arange(1, 40), [64.0, 63.999999, 1.0 / 3.0]])
    got = E(t)
    assert got.dtype == np.float64 and np.abs(got / np.exp(-t) - 1.0).max() < 1e-12
    s = np.sort(t)
    assert bool(np.all(np.diff(E(s)) <= 0.0))                                          # monotone on the sample
    # the spelling, operation by operation, at one point
    y = -(F(0.734375) * F(2.0) ** -10)
    p = F(1.0) / F(40320.0)
    for k in (5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0):
        p = p * y + F(1.0) / F(k)
    for _ in range(10):
        p = p * p
    assert E(0.734375) == p


def test_the_chain_under_linear_decay():
    """A 0.9, B 0.8, C 0.7 at nms_thr 0.4: A is selected; B (6/14 > 0.4) decays to 0.8 * (1 - 6/14) = 0.457, C (2/18) does not; C is selected
    with 0.7 and decays B once more; B is selected last with 0.8 * (8/14)^2 = 0.261.  Nothing is deleted by overlap"""
    a, b, c = (F(np.float32(x)) for x in (0.9, 0.8, 0.7))
    ab = F(6) / F(14)
    keep, sc, _ = _soft(CHAIN, ('linear', 0.5, 0.0, 0), 0.4)
    want_b = (b * (F(1.0) - ab)) * (F(1.0) - ab)
    assert keep == [1, 1, 1] and sc.tolist() == [np.float32(a), np.float32(want_b), np.float32(c)]
    assert abs(float(sc[1]) - 0.8 * (8.0 / 14.0) ** 2) < 1e-7
    # the floor cuts the list: B's 0.261 is below 0.3
    keep, sc, _ = _soft(CHAIN, ('linear', 0.5, 0.3, 0), 0.4)
    assert keep == [1, 0, 1] and sc.tolist() == [np.float32(a), np.float32(c)]
    # a count cuts it in selection order: A, then C
    assert _soft(CHAIN, ('linear', 0.5, 0.0, 1), 0.4)[0] == [1, 0, 0] and _soft(CHAIN, ('linear', 0.5, 0.0, 2), 0.4)[0] == [1, 0, 1]
    # at 0.1 the weak overlap AC decays too: C = 0.7 * (1 - 2/18) = 0.622 is still in front of B = 0.457
    keep, sc, _ = _soft(CHAIN, ('linear', 0.5, 0.0, 0), 0.1)
    ac = F(2) / F(18)
    assert sc.tolist() == [np.float32(a), np.float32((b * (F(1.0) - ab)) * (F(1.0) - ab)), np.float32(c * (F(1.0) - ac))]
    # the other score column reverses the walk: C 0.3 first; B decays to 0.2 * 8/14 = 0.114, still in front of A 0.1, which it then decays
    keep, sc, out = _soft(CHAIN, ('linear', 0.5, 0.0, 0), 0.4, 'mean')
    assert sc.tolist() == [np.float32(F(np.float32(0.1)) * (F(1.0) - ab)), np.float32(F(np.float32(0.2)) * (F(1.0) - ab)), np.float32(0.3)]
    assert out.score[:, 0].tolist() == [float(np.float32(x)) for x in (0.9, 0.8, 0.7)]  # the max column is copied


def test_the_chain_under_gaussian_decay():
    """sigma 0.5: every overlap decays.  A; then B = 0.8 * E((6/14)^2 / 0.5) = 0.554 and C = 0.7 * E((2/18)^2 / 0.5) = 0.683; C is selected and
    decays B to 0.384"""
    from cfn_hip.detections import decay_exp_reference as E
    a, b, c = (F(np.float32(x)) for x in (0.9, 0.8, 0.7))
    ab, ac, sigma = F(6) / F(14), F(2) / F(18), F(0.5)
    eb, ec = F(E((ab * ab) / sigma)), F(E((ac * ac) / sigma))
    keep, sc, _ = _soft(CHAIN, ('gaussian', 0.5, 0.0, 0))
    assert keep == [1, 1, 1] and sc.tolist() == [np.float32(a), np.float32((b * eb) * eb), np.float32(c * ec)]
    assert abs(float(sc[1]) - 0.8 * np.exp(-2 * (6 / 14) ** 2 / 0.5)) < 1e-7 and abs(float(sc[2]) - 0.7 * np.exp(-(2 / 18) ** 2 / 0.5)) < 1e-7
    # gaussian does not look at nms_thr
    assert all(np.array_equal(_soft(CHAIN, ('gaussian', 0.5, 0.0, 0), thr)[1], sc) for thr in (0.0, 1.0))
    assert _soft(CHAIN, ('gaussian', 0.5, 0.4, 0))[0] == [1, 0, 1]                      # the floor: B's 0.384 is below 0.4
    # a small sigma is hard NMS at 0 in effect: 1/64 gives E(11.8) = 8e-6 for AB, E(0.79) = 0.45 for AC
    keep, sc, _ = _soft(CHAIN, ('gaussian', 1.0 / 64.0, 0.001, 0))
    assert keep == [1, 0, 1] and sc.tolist() == [np.float32(a), np.float32(c * F(E((ac * ac) / F(1.0 / 64.0))))]
    # touching segments (inter = 0) do not decay
    keep, sc, _ = _soft([(0, 0, 10, 0.9, 0.1), (0, 10, 20, 0.8, 0.2)], ('gaussian', 1.0 / 64.0, 0.0, 0))
    assert sc.tolist() == [np.float32(0.9), np.float32(0.8)]


def test_a_score_tie_goes_to_the_lower_row():
    rows = [(0, 0, 10, 0.5, 0.5), (0, 20, 30, 0.5, 0.5), (0, 40, 50, 0.5, 0.5)]
    assert _soft(rows, ('linear', 0.5, 0.0, 1))[0] == [1, 0, 0] and _soft(rows, ('gaussian', 0.5, 0.0, 2))[0] == [1, 1, 0]
    # a tie that the decay makes: X 1.0 halves Y (tIoU 1/2 > 0.4) to 0.5 exactly, which ties with Z 0.5; Y is the lower row
    rows = [(0, 0, 10, 1.0, 0.5), (0, 5, 10, 1.0, 0.5), (0, 40, 50, 0.5, 0.5)]
    keep, sc, _ = _soft(rows, ('linear', 0.5, 0.0, 2), 0.4)
    assert keep == [1, 1, 0] and sc.tolist() == [1.0, 0.5]
    rows = [(0, 0, 10, 1.0, 0.5), (0, 5, 10, 1.0, 0.5), (0, -50, -40, 0.5, 0.5)]       # ... and here Z is
    assert _soft(rows, ('linear', 0.5, 0.0, 2), 0.4)[0] == [1, 1, 0]                   # (rows are ordered by start: Z, X, Y)


def test_linear_is_strict_at_the_threshold():
    thr = float(F(6) / F(14))
    keep, sc, _ = _soft(CHAIN, ('linear', 0.5, 0.0, 0), thr)
    assert sc.tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.7)]           # a tIoU equal to nms_thr does not decay
    keep, sc, _ = _soft(CHAIN, ('linear', 0.5, 0.0, 0), float(np.nextafter(F(6) / F(14), 0.0)))
    assert sc[1] < np.float32(0.3) and sc[0] == np.float32(0.9) and sc[2] == np.float32(0.7)


def test_a_nan_or_infinite_score_is_out_of_the_group():
    """S2: such a row is never selected and decays nothing, wherever it would have ranked"""
    for bad in (float('nan'), float('inf'), float('-inf')):
        rows = [(0, 0, 10, 0.9, 0.1), (0, 1, 10, bad, 0.2), (0, 4, 14, 0.8, 0.2), (0, 8, 18, 0.7, 0.3)]
        for soft in (('linear', 0.5, 0.0, 0), ('gaussian', 0.5, 0.0, 0)):
            keep, sc, _ = _soft(rows, soft, 0.4)
            assert keep == [1, 0, 1, 1] and np.array_equal(sc, _soft(CHAIN, soft, 0.4)[1])
    keep, sc, out = _soft([(0, 0, 10, float('nan'), 0.1)], ('gaussian', 0.5, 0.0, 0))
    assert keep == [0] and out.check() == 0


@pytest.mark.parametrize('score', ['max', 'mean'])
@pytest.mark.parametrize('soft', [('linear', 0.5, 0.001, 0), ('gaussian', 0.5, 0.001, 0), ('gaussian', 4.0, 0.3, 0), ('linear', 0.5, 0.0, 10),
                                  ('gaussian', 1.0 / 64.0, 0.0, 0)])
def test_the_reference_is_the_rule_row_by_row_and_finals_never_increase(soft, score):
    """the vectorised rounds against the scalar spelling, bit for bit; in selection order the finals of a group do not increase, so the floor
    and the count cut a ranked list"""
    from cfn_hip.detections import SCORE_COLUMNS, SoftNMS, soft_nms_reference
    det = candidates(7, [{0: 65, 1: 200}, {}, {1: 130, 3: 2}], 4, span=40.0)
    out, keep, src = soft_nms_reference(det, SoftNMS(*soft), 0.3, score)
    k2, final, order = soft_loop(det, soft, 0.3, score)
    n, col = out.check(), SCORE_COLUMNS[score]
    assert np.array_equal(keep.numpy(), k2) and 0 < n == len(order) and (n < int(det.total) or soft[2] == 0.0 and soft[3] == 0)
    assert np.array_equal(out.score[:n, col].numpy().view(np.int32), final[src[:n].numpy()].view(np.int32))
    if not soft[3]:                                                                      # (a count of 10 is reached before a decayed row)
        assert int((out.score[:n, col] != det.score[src[:n].long(), col]).sum()) > 0    # something was decayed and selected
    seg, offs = det.seg.numpy(), det.offsets.numpy()
    vid = np.searchsorted(offs[1:], order, side='right')
    for a, b in zip(range(len(order) - 1), range(1, len(order))):
        if vid[a] == vid[b] and seg[order[a], 0] == seg[order[b], 0]:
            assert final[order[a]] >= final[order[b]]
    if soft[3]:
        assert np.bincount(np.unique(np.stack([vid, seg[order, 0]]), axis=1, return_inverse=True)[1].ravel()).max() == soft[3]


def test_the_premises_of_the_boundary_and_subnormal_cases():
    """what test_hip_softnms.py assumes of its inputs, checked where no GPU is needed: at every size both methods select a decayed row and,
    from 63 candidates on, drop one; the issue's counts; the subnormal case's order"""
    from cfn_hip.detections import SoftNMS, decay_exp_reference, soft_nms_reference
    for nd in SIZES:
        det = boundary_batch(nd)
        assert int(det.total) == 2 * nd + 6
        for method in ('linear', 'gaussian'):
            out, keep, src = soft_nms_reference(det, SoftNMS(method, 0.5, FLOOR, 0), 0.5)
            n = out.check()
            assert int((out.score[:n, 0] != det.score[src[:n].long(), 0]).sum()) > 0, (nd, method)
            assert nd < 63 or n < int(det.total), (nd, method)
    counts = {(nd, ms, m): soft_nms_reference(candidates(7, [{0: nd}], 1), SoftNMS(m, 0.5, ms, 0), 0.5)[0].check()
              for nd, ms in ((65, 0.05), (65, 0.001), (1025, 0.001)) for m in ('linear', 'gaussian')}
    assert counts[(65, 0.05, 'gaussian')] == 49 and (counts[(65, 0.001, 'linear')], counts[(65, 0.001, 'gaussian')]) == (64, 65)
    assert (counts[(1025, 0.001, 'linear')], counts[(1025, 0.001, 'gaussian')]) == (426, 351)
    sub = subnormal_batch()
    e64 = F(decay_exp_reference(64.0))
    w = F(np.float32(1e-11))
    for _ in range(11):
        w = w * e64
    assert 0.0 < w < np.finfo(np.float64).tiny and w * e64 == 0.0                        # rank 11 is subnormal, rank 12 is 0
    soft = ('gaussian', 1.0 / 64.0, 0.0, 0)
    out, keep, _ = soft_nms_reference(sub, SoftNMS(*soft))
    assert keep.tolist() == [1] * 16 and soft_loop(sub, soft)[2] == [15 - r for r in range(12)] + [0, 1, 2, 3]
    assert out.score[:, 0].tolist()[:13] == [0.0] * 13 and out.score[15, 0] == 1.0 and 0.0 < float(out.score[14, 0]) < 1e-28
    assert soft_nms_reference(sub, SoftNMS('gaussian', 1.0 / 64.0, 0.0, SUBNORMAL_KEEP))[1].tolist() == [0] * 4 + [1] * 12


def test_identity_linear_at_1_returns_its_input():
    from cfn_hip.detections import SoftNMS, soft_nms_reference
    det = candidates(9, [{0: 65, 1: 200}, {}, {1: 130, 3: 2}], 4, span=40.0)
    for score in ('max', 'mean'):
        out, keep, src = soft_nms_reference(det, SoftNMS('linear', 0.5, 0.0, 0), 1.0, score)
        assert same_det(out, det) == int(det.total) and keep.all() and src.tolist() == list(range(int(det.total)))


def test_identity_a_single_level_decode_passes_through():
    from cfn_hip.detections import SoftNMS, decode_reference, soft_nms_reference
    p = random_probs(11, 3, 5, 130)
    one = decode_reference(p, torch.tensor([130, 100, 77], dtype=torch.int32), thr=0.35, max_gap=1, min_len=2)
    assert one.check() > 10
    for soft in (SoftNMS(), SoftNMS('linear'), SoftNMS('gaussian', 1.0 / 64.0, 0.35, 0)):
        for score in ('max', 'mean'):
            assert same_det(soft_nms_reference(one, soft, 0.0, score)[0], one) == one.check()
    assert soft_nms_reference(one, SoftNMS('gaussian', 0.5, 0.9, 0))[0].check() < one.check()      # a floor above some scores does cut


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
def test_identity_the_first_selected_row_is_hard_nms_first_kept_row(method):
    """max_keep = 1 leaves each group's first row in hard NMS's order, with its score; and without a count that row is selected undecayed"""
    from cfn_hip.detections import SCORE_COLUMNS, SoftNMS, nms_reference, soft_nms_reference
    det = candidates(5, [{0: 65, 1: 200}, {2: 7}, {1: 130, 3: 2}], 4, span=40.0)
    for score in ('max', 'mean'):
        first, col = first_rows(det, score), SCORE_COLUMNS[score]
        out, keep, src = soft_nms_reference(det, SoftNMS(method, 0.5, 0.001, 1), 0.5, score)
        assert src.tolist() == first and same_det(out, type(det)(det.seg[first], det.frames[first], det.score[first], out.offsets, out.total, 4, len(first)))
        for thr in (0.0, 0.5):
            hard = nms_reference(det, thr, score)[1].numpy()
            assert all(hard[i] for i in first)
        full, keep, src = soft_nms_reference(det, SoftNMS(method, 0.5, 0.001, 0), 0.5, score)
        pos = {int(r): i for i, r in enumerate(src.tolist())}
        assert all(full.score[pos[i], col] == det.score[i, col] for i in first)


def test_caps_groups_and_an_empty_batch():
    from cfn_hip.detections import SoftNMS, soft_nms_reference
    det = candidates(8, [{0: 70, 2: 40}, {1: 90}], 3, span=30.0)
    full, keep, src = soft_nms_reference(det, SoftNMS('gaussian', 0.5, 0.05, 0))
    n = full.check()
    assert 11 < n < 200 and full.offsets.tolist() == [0, int(keep[:110].sum()), n]
    cut, keep2, src2 = soft_nms_reference(det, SoftNMS('gaussian', 0.5, 0.05, 0), cap=11)    # a cap keeps the prefix and the true counts
    assert cut.cap == 11 and cut.offsets.tolist() == full.offsets.tolist() and torch.equal(keep2, keep) and torch.equal(src2, src[:11])
    assert same_det(cut, full, rows=11) == 11
    with pytest.raises(RuntimeError, match='cap = 11'):
        cut.check()
    out, keep, src = soft_nms_reference(fx.make_det([[], []], 2), SoftNMS())
    assert out.check() == 0 and out.offsets.tolist() == [0, 0, 0] and keep.numel() == 0


def test_the_options_are_checked():
    from cfn_hip.detections import SoftNMS, soft_nms, soft_nms_reference
    assert SoftNMS() == ('gaussian', 0.5, 0.001, 0) and SoftNMS._fields == ('method', 'sigma', 'min_score', 'max_keep')
    det = fx.make_det([CHAIN], 1)
    for bad in (SoftNMS('exp'), SoftNMS(sigma=1.0 / 128.0), SoftNMS(sigma=float(1 << 21)), SoftNMS(sigma=float('nan')), SoftNMS(min_score=-0.1),
                SoftNMS(min_score=1.5), SoftNMS(min_score=float('nan')), SoftNMS(max_keep=-1), SoftNMS(max_keep=1.5)):
        with pytest.raises(ValueError, match='soft'):
            soft_nms_reference(det, bad)
        with pytest.raises(ValueError, match='soft'):
            soft_nms(det, bad)
    for thr in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='nms_thr'):
            soft_nms_reference(det, SoftNMS('linear'), thr)
    with pytest.raises(ValueError, match='score'):
        soft_nms_reference(det, SoftNMS(), score='median')
    with pytest.raises(TypeError):
        soft_nms_reference(det, 'gaussian')
    with pytest.raises(TypeError):
        soft_nms(det[:5], SoftNMS())
    assert soft_nms_reference(det, ('linear', 0.5, 0.0, 0), 0.4)[0].check() == 3          # a plain tuple of the four is taken


def test_entry_point_is_declared_exported_and_checks_its_arguments():
    cfn_hip = _lib()
    protos = cfn_hip.header_prototypes()
    ret, at, dts = protos['cfn_soft_nms_segments']
    i, d, l, p = ctypes.c_int, ctypes.c_double, ctypes.c_long, ctypes.c_void_p
    assert ret is i and at == [p] * 12 + [i, i, i, d, i, d, d, i, l, l, p]
    assert dts[:12] == protos['cfn_nms_segments'][2][:12]
    assert protos['cfn_soft_nms_segments_workspace_bytes'][:2] == (l, [i, i, l])
    raw = ctypes.CDLL(cfn_hip.LIB_PATH)
    assert hasattr(raw, 'cfn_soft_nms_segments') and hasattr(raw, 'cfn_soft_nms_segments_workspace_bytes')
    lib = cfn_hip.load()
    q = cfn_hip.query
    # 8 bytes of working score and 4 of final score per input row, B * C + 1 counts, rounded up to 8
    assert q('cfn_soft_nms_segments_workspace_bytes', 2, 157, 1001) == 1001 * 8 + ((1001 * 4 + (2 * 157 + 1) * 4 + 7) // 8) * 8
    assert q('cfn_soft_nms_segments_workspace_bytes', 1, 1, 1) == 8 + 16
    for shape in ((0, 157, 8), (1, 0, 8), (65536, 1, 8), (1, 65536, 8), (1, 157, 0), (1, 157, 1 << 31)):
        assert q('cfn_soft_nms_segments_workspace_bytes', *shape) == -1, shape
    buf = (ctypes.c_double * 8)()
    ptr = [ctypes.addressof(buf)] * 12
    ok = dict(B=1, C=157, col=0, thr=0.5, method=1, sigma=0.5, floor=0.001, keep=0, cap_in=8, cap_out=8)
    call = lambda a, **kw: lib.cfn_soft_nms_segments(*a, *[dict(ok, **kw)[k] for k in ok], None)
    assert call([None] * 12) == 1 and 'null' in cfn_hip.last_error()
    nan = float('nan')
    for kw, word in ((dict(B=0), 'shape'), (dict(C=65536), 'shape'), (dict(cap_in=0), 'shape'), (dict(cap_out=0), 'cap_out'), (dict(col=2), 'score_col'),
                     (dict(thr=-0.1), 'nms_thr'), (dict(thr=1.5), 'nms_thr'), (dict(thr=nan), 'nms_thr'), (dict(method=2), 'method'),
                     (dict(method=-1), 'method'), (dict(sigma=1.0 / 128.0), 'sigma'), (dict(sigma=float(1 << 21)), 'sigma'), (dict(sigma=nan), 'sigma'),
                     (dict(sigma=0.0), 'sigma'), (dict(floor=-0.001), 'min_score'), (dict(floor=1.001), 'min_score'), (dict(floor=nan), 'min_score'),
                     (dict(keep=-1), 'max_keep'), ({}, 'outputs must not be the inputs')):
        assert call(ptr, **kw) == 1, kw                                                # refused before any launch
        assert 'cfn_soft_nms_segments' in cfn_hip.last_error() and word in cfn_hip.last_error(), cfn_hip.last_error()
    csrc = os.path.join(os.path.dirname(cfn_hip.LIB_PATH), '..', 'csrc')
    src = open(os.path.join(csrc, 'segnms.hip')).read()
    assert 'getenv' not in src and 'atomicAdd' not in src and 'hipMalloc' not in src and 'fp contract(off)' in src
    from cfn_hip import torchlib as tl
    assert not any('nms' in n for tup in (tl.OPERATORS, tl.INPUT_OPERATORS, tl.AUGMENT_OPERATORS, tl.METRIC_OPERATORS, tl.FEATURE_OPERATORS,
                                          tl.DECODE_OPERATORS, tl.LABEL_OPERATORS) for n in tup)


def test_op_refuses_cpu_tensors_and_malformed_arguments():
    _lib()
    from cfn_hip import ops
    from cfn_hip.detections import SoftNMS, propose, soft_nms
    det, _ = fx.hand_batch()
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.soft_nms_segments(det.seg, det.frames, det.score, det.offsets, 5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        soft_nms(det, SoftNMS())
    with pytest.raises(RuntimeError, match='no CPU path'):
        propose(torch.zeros(2, 5, 16), torch.full((2,), 16, dtype=torch.int32), soft=SoftNMS())
    with pytest.raises(RuntimeError, match='soft_nms_segments'):
        ops.soft_nms_segments_workspace_bytes(1, 65536, 8)


def test_writer_with_soft_keeps_the_soft_nms_batch(tmp_path):
    from cfn_hip.detections import DetectionWriter, SoftNMS, decode_reference, propose, read_detections
    p = random_probs(13, 2, 4, 60)
    valid = torch.tensor([60, 41], dtype=torch.int32)
    soft = SoftNMS('linear', 0.5, 0.05, 3)
    w = DetectionWriter(str(tmp_path / 'det.jsonl'), 0.5, 1, 2, levels=LEVELS5, nms=0.4, nms_score='mean', soft=soft)
    assert w.soft == soft and DetectionWriter('x', levels=LEVELS5).soft is None
    got = w.add(p, valid, None, ['v0', 'v1'], decoder=decode_reference)
    want = propose(p, valid, None, None, LEVELS5, 0.4, 'mean', 1, 2, reference=True, soft=soft)
    hard = propose(p, valid, None, None, LEVELS5, 0.4, 'mean', 1, 2, reference=True)
    assert same_det(got, want) > 0 and got.check() != hard.check() and len(w._pending) == 1
    assert w.flush() == 2
    rows = read_detections(w.path)
    assert [r['segments'] for r in rows] == want.tolist() and all(set(r) == {'video', 'unit', 'segments'} for r in rows)
    with pytest.raises(ValueError, match='soft'):
        DetectionWriter('x', soft=soft)
    with pytest.raises(ValueError, match='soft'):
        DetectionWriter('x', levels=LEVELS5, soft=SoftNMS('exp'))


def test_meter_takes_the_soft_option():
    from cfn_hip.detections import SoftNMS
    from cfn_hip.segap import SegmentAPMeter
    import inspect
    assert inspect.signature(SegmentAPMeter.__init__).parameters['soft'].default is None
    for kw in ({'soft': SoftNMS()}, {'levels': (0.5, 0.3), 'soft': SoftNMS(sigma=0.0)}):
        with pytest.raises(ValueError, match='soft'):
            SegmentAPMeter('cuda', 5, **kw)
    import train_fine
    assert 'soft=meter.soft' in inspect.getsource(train_fine.segment_ap_add)


def test_scripts_forward_the_soft_nms_flags():
    import train_coarse_fineFEAT as tc
    import train_fine
    from cfn_hip.detections import SoftNMS
    parser = argparse.ArgumentParser()
    train_fine.add_detect_args(parser)
    train_fine.seg_ap_arguments(parser)
    # without the options nothing changes: the dict of an `args` that does not know them, and of one that does
    old = argparse.Namespace(detect='d.jsonl', detect_thr=0.5, detect_gap=0, detect_min_len=1, detect_levels='0.6,0.3', detect_nms=None, detect_nms_score='max')
    today = {'levels': [0.6, 0.3], 'nms': None, 'nms_score': 'max'}
    assert train_fine.detect_levels(old) == today == train_fine.detect_levels(parser.parse_args(['--detect-levels', '0.6,0.3']))
    assert train_fine.detect_levels(parser.parse_args(['--detect', 'd.jsonl'])) == {}
    assert not any('soft' in a or 'min-score' in a or 'max-keep' in a for a in train_fine.detect_argv(parser.parse_args(['--detect', 'd', '--detect-levels', '0.6'])))
    on = parser.parse_args(['--detect', 'd.jsonl', '--detect-levels', '0.8,0.5,0.2', '--detect-soft-nms', 'gaussian', '--detect-soft-sigma', '0.3',
                            '--detect-min-score', '0.01', '--detect-max-keep', '20'])
    again = parser.parse_args(train_fine.detect_argv(on))                                 # what a spawned worker parses
    assert vars(again) == vars(on)
    assert train_fine.detect_levels(again) == dict(levels=[0.8, 0.5, 0.2], nms=None, nms_score='max', soft=SoftNMS('gaussian', 0.3, 0.01, 20))
    w = train_fine.detect_writer(again)
    assert (w.soft, w.nms, w.n_levels) == (SoftNMS('gaussian', 0.3, 0.01, 20), 0.5, 3)
    lin = parser.parse_args(['--detect', 'd', '--detect-levels', '0.6,0.3', '--detect-soft-nms', 'linear', '--detect-nms', '0.45'])
    assert train_fine.detect_levels(lin)['soft'] == SoftNMS('linear') and train_fine.detect_writer(lin).nms == 0.45
    assert vars(parser.parse_args(train_fine.detect_argv(lin))) == vars(lin)
    for argv, word in ((['--detect-soft-nms', 'gaussian'], '--detect-levels'), (['--detect-levels', '0.5', '--detect-min-score', '0.1'], '--detect-soft-nms'),
                       (['--detect-levels', '0.5', '--detect-max-keep', '3'], '--detect-soft-nms'),
                       (['--detect-levels', '0.5', '--detect-soft-sigma', '0.3'], '--detect-soft-nms'),
                       (['--detect-levels', '0.5', '--detect-soft-nms', 'gaussian', '--detect-nms', '0.5'], 'gaussian'),
                       (['--detect-levels', '0.5', '--detect-soft-nms', 'gaussian', '--detect-soft-sigma', '0.001'], 'sigma')):
        with pytest.raises(ValueError, match=word):
            train_fine.detect_writer(parser.parse_args(['--detect', 'd'] + argv))
    with pytest.raises(SystemExit):
        parser.parse_args(['--detect-soft-nms', 'exp'])
    assert tc.add_detect_args is train_fine.add_detect_args and tc.detect_argv is train_fine.detect_argv
