"""Temporal score filter on the GPU (cfn_hip.ops.score_filter, csrc/scorefilter.hip) against filter_reference: bit-equal (NaNs by position and
by the bits of rule F3) and equal between two calls, at every tile boundary and every valid_t that changes a window; out= inside canaries;
refusals; filter + decode in one graph; and the filter in front of the writer's and the meter's decode on the golden label arrays."""
import numpy as np
import pytest
import torch

import scorefilter_fixture as fx
import seg_fixture as sf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = -777.25
PAD = 1024                                         # canary floats on each side of out
RADII = (0, 1, 3, 32, 7)


def _tile():
    import cfn_hip
    return int(cfn_hip.query('cfn_score_filter_tile'))


def _filters():
    from cfn_hip.scorefilter import ScoreFilter
    return {'box': ScoreFilter('box', RADII), 'gaussian': ScoreFilter('gaussian', RADII, [0.5, 0.6, 1.25, 11.0, 2.5]), 'median': ScoreFilter('median', RADII)}


def _apply_checked(p, valid, flt):
    """apply(out = a view inside a canary-filled buffer) of host arrays on the GPU, twice -> the result on the host; the canaries on both
    sides are intact and the second call gives the same bits"""
    from cfn_hip.scorefilter import apply
    B, C, TL = p.shape
    n = B * C * TL
    dp, dv = torch.from_numpy(p.copy()).to(DEV), torch.from_numpy(np.asarray(valid, np.int32)).to(DEV)
    results = []
    for _ in range(2):
        buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
        out = buf[PAD:PAD + n].view(B, C, TL)
        got = apply(dp, dv, flt, out=out)
        assert got is out
        host = buf.cpu()
        assert bool((host[:PAD] == CANARY).all()) and bool((host[PAD + n:] == CANARY).all()), 'a store outside out'
        results.append(host[PAD:PAD + n].view(B, C, TL).clone())
    fx.same_bits(results[1], results[0])
    fx.same_bits(dp, p)                                                               # the input is not written
    return results[0]


def _valid_triples(TL, r=32):
    """the issue's valid_t values {-1, 0, 1, r, r + 1, TL - 1, TL, TL + 5}, three videos at a time (the ninth slot: half the row)"""
    v = [-1, 0, 1, r, r + 1, TL - 1, TL, TL + 5, TL // 2]
    return [v[0:3], v[3:6], v[6:9]]


@pytest.mark.parametrize('method', ['box', 'gaussian', 'median'])
@pytest.mark.parametrize('TL', ['1', '2', 'T-1', 'T', 'T+1', 'T+32', '2T+1'])
def test_bit_equal_to_the_reference_at_every_boundary(TL, method):
    """B = 3, C = 5, radii (0, 1, 3, 32, 7) in one call; TL around the tile of cfn_score_filter_tile() frames and its 32-frame halo; every
    valid_t that cuts a window; the random, quantised (median ties) and wide-range (order of the sum) fixtures"""
    from cfn_hip.scorefilter import filter_reference
    T = _tile()
    TL = {'1': 1, '2': 2, 'T-1': T - 1, 'T': T, 'T+1': T + 1, 'T+32': T + 32, '2T+1': 2 * T + 1}[TL]
    flt = _filters()[method]
    changed = 0
    for kind in ('random', 'quantised', 'wide'):
        p = fx.scores(kind, 3, 5, TL)
        for valid in _valid_triples(TL):
            ref = filter_reference(torch.from_numpy(p.copy()), torch.tensor(valid, dtype=torch.int32), flt)
            got = _apply_checked(p, valid, flt)
            fx.same_bits(got, ref)
            fx.same_bits(got[:, 0], p[:, 0])                                          # radius 0
            changed += int((got.numpy().view(np.uint32) != p.view(np.uint32)).sum())
    assert changed > 0 or TL == 1                                                     # (a one-frame row is its own window)


@pytest.mark.parametrize('method', ['box', 'median'])
def test_non_finite_values_give_the_canonical_nan_by_position(method):
    from cfn_hip.scorefilter import filter_reference
    T = _tile()
    TL = T + 40
    p = fx.scores('random', 3, 5, TL).copy()
    payload = np.array([0xffc12345], np.uint32).view(np.float32)[0]
    for b, c, t, v in ((0, 1, 0, np.nan), (0, 3, T - 1, np.inf), (1, 3, T, -np.inf), (1, 4, TL - 1, payload), (2, 2, T + 3, payload), (2, 0, 5, payload),
                       (0, 4, T + 20, np.inf), (2, 3, 100, np.nan)):
        p[b, c, t] = v
    flt = _filters()[method]
    valid = [TL, TL - 1, T + 2]
    ref = filter_reference(torch.from_numpy(p.copy()), torch.tensor(valid, dtype=torch.int32), flt)
    got = _apply_checked(p, valid, flt)
    fx.same_bits(got, ref)
    bits = got.numpy().view(np.uint32)
    assert bits[0, 3, T - 33:T + 32].tolist() == [fx.QNAN] * 65 and bits[0, 1, :2].tolist() == [fx.QNAN] * 2            # the halo on both sides of a tile edge
    assert bits[2, 0, 5] == 0xffc12345 and bits[1, 4, TL - 1] == 0xffc12345          # radius 0, and behind valid_t: the input bits
    assert bits[2, 2, T + 3] == 0xffc12345 and np.isfinite(got.numpy()[2, 2, :T + 2]).all()        # a NaN behind valid_t reaches no window


@pytest.mark.parametrize('method', ['box', 'median'])
def test_radius_zero_returns_the_input_bits(method):
    from cfn_hip.scorefilter import ScoreFilter
    T = _tile()
    p = fx.scores('wide', 2, 3, T + 7).copy()
    p.view(np.uint32)[0, 1, 3], p.view(np.uint32)[1, 2, T] = 0xffc12345, 0x7f800001   # a quiet NaN with a payload, a signalling one
    p[1, 0, 9] = np.inf
    fx.same_bits(_apply_checked(p, [T + 7, 40], ScoreFilter(method, 0)), p)


def test_refusals():
    from cfn_hip import ops
    from cfn_hip.scorefilter import ScoreFilter, apply
    flt = ScoreFilter('box', 2)
    p = torch.rand(2, 3, 16, device=DEV)
    v = torch.tensor([16, 9], dtype=torch.int32, device=DEV)
    radius, weights, code = flt.tensors(3, p.device)
    ops.score_filter(p, v, radius, weights, code)
    with pytest.raises(RuntimeError, match='must not be'):                            # aliasing
        apply(p, v, flt, out=p)
    big = torch.rand(2 * 3 * 16 + 8, device=DEV)
    with pytest.raises(RuntimeError, match='must not be'):                            # partial overlap
        ops.score_filter(big[:96].view(2, 3, 16), v, radius, weights, code, out=big[8:104].view(2, 3, 16))
    with pytest.raises(RuntimeError, match='no CPU path'):                            # CPU tensors
        apply(p.cpu(), v.cpu(), flt)
    for bad in ((p.cpu(), v, radius, weights), (p, v.cpu(), radius, weights), (p, v, radius.cpu(), weights), (p, v, radius, weights.cpu())):
        with pytest.raises(RuntimeError, match='no CPU path'):
            ops.score_filter(*bad, code)
    with pytest.raises(RuntimeError, match='out'):
        ops.score_filter(p, v, radius, weights, code, out=torch.empty(2, 3, 16))
    for bad in ((p.double(), v, radius, weights), (p.half(), v, radius, weights), (p, v.long(), radius, weights), (p, v, radius.long(), weights),
                (p, v, radius, weights.float()), (p[0], v, radius, weights), (p, v[:1], radius, weights), (p, v, radius[:2], weights),
                (p, v, radius, weights[:2])):                                         # wrong dtypes and shapes
        with pytest.raises(RuntimeError, match='expected'):
            ops.score_filter(*bad, code)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.score_filter(p.transpose(1, 2).contiguous().transpose(1, 2), v, radius, weights, code)
    with pytest.raises(RuntimeError, match='R <= 32'):                                # R = 33
        ops.score_filter(p, v, radius, torch.ones(3, 34, dtype=torch.float64, device=DEV), code)
    with pytest.raises(RuntimeError, match='out'):
        ops.score_filter(p, v, radius, weights, code, out=torch.empty(2, 3, 16, dtype=torch.float64, device=DEV))
    for bad in (2, -1, True, 0.0, 'median'):
        with pytest.raises(RuntimeError, match='method'):
            ops.score_filter(p, v, radius, weights, bad)
    import cfn_hip
    with pytest.raises(RuntimeError, match='R in'):                                   # the entry point itself refuses R = 33 too
        cfn_hip.call('cfn_score_filter', p, v, radius, torch.ones(3, 34, dtype=torch.float64, device=DEV), torch.empty_like(p), 2, 3, 16, 33, 0)


def _same_detections(got, ref):
    """a Detections on the GPU and decode_reference's: the same counts, and the rows found equal bit for bit in every column"""
    k = ref.check()
    assert got.total.cpu().tolist() == [k] and got.offsets.cpu().tolist() == ref.offsets.tolist()
    for g, r in zip(got[:3], ref[:3]):
        assert torch.equal(g[:k].cpu().contiguous().view(torch.uint8), r[:k].contiguous().view(torch.uint8))
    return k


@pytest.mark.capture
def test_filter_and_decode_in_one_graph_replayed_on_new_scores():
    """apply(out=) and decode(out=) captured together.  Quantised scores under the median: every filtered value is a multiple of 1/16, so the
    decode's fp64 mean is exact in any order and the whole result can be asked to EQUAL the reference, mean column included"""
    from cfn_hip import ops
    from cfn_hip.detections import decode, decode_reference
    from cfn_hip.scorefilter import ScoreFilter, apply, filter_reference
    T = _tile()
    B, C, TL = 3, 5, T + 9
    flt = ScoreFilter('median', [0, 1, 3, 32, 7])
    cases = [(fx.scores('quantised', B, C, TL, seed), torch.tensor(valid, dtype=torch.int32)) for seed, valid in ((1, [TL, T, 40]), (2, [T + 1, TL, 0]))]
    probs, valid = torch.from_numpy(cases[0][0].copy()).to(DEV), cases[0][1].to(DEV)
    fps, start = torch.tensor([24.0, 29.97, 12.5], dtype=torch.float64, device=DEV), torch.tensor([0, 17, 3], dtype=torch.int32, device=DEV)
    thr = torch.full((C,), 0.5, dtype=torch.float32, device=DEV)
    smooth = torch.empty_like(probs)
    cap = ops.decode_segments_cap(B, C, TL)
    out = (torch.empty(cap, 3, dtype=torch.float64, device=DEV), torch.empty(cap, 3, dtype=torch.int32, device=DEV),
           torch.empty(cap, 2, dtype=torch.float32, device=DEV), torch.empty(B + 1, dtype=torch.int32, device=DEV),
           torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(ops.decode_segments_workspace_bytes(B, C, TL), dtype=torch.uint8, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                     # warm-up outside the capture (builds flt's tensors)
        decode(apply(probs, valid, flt, out=smooth), valid, fps, start, thr, 1, 2, out=out)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = decode(apply(probs, valid, flt, out=smooth), valid, fps, start, thr, 1, 2, out=out)
    totals = []
    for p, v in cases:
        probs.copy_(torch.from_numpy(p.copy()))
        valid.copy_(v)
        smooth.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        ref = decode_reference(torch.from_numpy(p.copy()), v, fps.cpu(), start.cpu(), 0.5, 1, 2, filter=flt)
        fx.same_bits(smooth, filter_reference(torch.from_numpy(p.copy()), v, flt))
        totals.append(_same_detections(got, ref))
    assert totals[0] != totals[1] and min(totals) > 0


def _golden_batch(name):
    """batch `name` of the golden label arrays as scores: (labels (B, 157, TL) on the GPU, valid_t, the collated SegLabels, video names)"""
    from cfn_hip.seglabels import collate_seg
    split, idx, labels, masks = sf.batch(name)
    sl = collate_seg([sf.seglabel(i, split) for i in idx])
    valid = torch.from_numpy(masks.sum(1)).to(torch.int32)
    return torch.from_numpy(labels.copy()), valid, sl, ['%s%d' % (name, i) for i in idx]


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_median_in_front_of_the_writer_and_the_meter_on_the_golden_labels(name):
    """median:2, then decode(thr = 0.5), equals decode_reference(filter=) row for row -- through DetectionWriter(filter=) and through
    SegmentAPMeter(filter=) fed by train_fine.segment_ap_add.  (Labels are 0 / 1, so medians are 0, 0.5 or 1 and every column is exact.)"""
    import train_fine
    from cfn_hip.detections import DetectionWriter, decode_reference
    from cfn_hip.scorefilter import parse_spec
    from cfn_hip.segap import SegmentAPMeter
    flt = parse_spec('median:2')
    probs, valid, sl, names = _golden_batch(name)
    ref = decode_reference(probs, valid, sl.fps, sl.window[:, 0].contiguous(), 0.5, filter=flt)
    raw = decode_reference(probs, valid, sl.fps, sl.window[:, 0].contiguous(), 0.5)
    # the filter removes short runs of batches b and c (25 -> 20 and 32 -> 29 segments); batch a's runs are all longer than the window
    assert (ref.check(), raw.check()) == {'a': (24, 24), 'b': (20, 25), 'c': (29, 32)}[name]
    writer = DetectionWriter('unused.jsonl', 0.5, filter=flt)
    det = writer.add(probs.to(DEV), valid.to(DEV), sl, names)
    _same_detections(det, ref)
    host = DetectionWriter('unused.jsonl', 0.5, filter=flt)
    host.add(probs, valid, sl, names, decoder=decode_reference)
    assert writer.take() == host.take()
    meter, fed = SegmentAPMeter(DEV, 157, filter=flt), SegmentAPMeter(DEV, 157)
    det2 = train_fine.segment_ap_add(meter, None, probs.to(DEV), valid.to(DEV), sl, None)
    _same_detections(det2, ref)
    fed.add(ref.to(DEV), sl)
    (ap, mp), (ap2, mp2) = meter.value(), fed.value()
    assert torch.equal(ap, ap2) and torch.equal(mp, mp2) and float(mp.max()) > 0
    both = train_fine.segment_ap_add(meter, det, probs.to(DEV), valid.to(DEV), sl, None, writer=writer)      # the writer's batch is not decoded again
    assert both is det
