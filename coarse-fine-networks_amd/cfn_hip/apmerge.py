"""Merge class-major AP stores: several meters' rows into one store, in a defined order, on the device (cfn_hip.ops.ap_merge,
csrc/apmerge.hip) -- what lets frame AP (apmeter.DeviceAPMeter) and segment AP (cfn_hip.segap.SegmentAPMeter) be evaluated over the
data-parallel ranks of a validation phase.

AP is not additive, so the ranks' values cannot be summed the way cfn_hip.recall's state can.  But both meters keep one layout -- ``scores
(C, cap)`` fp32 plus a payload byte ``(C, cap)`` (the target bit, the tp byte), with ONE count for all classes (frame AP) or one count per
class plus n_gt (segment AP) -- and the sort behind AP is stable and breaks ties in insertion order.  Appending the ranks' stores in a fixed
order therefore gives every rank the same bits, and they are the bits ONE process would have produced had it been fed the ranks' batches one
rank after another.  This is the rule, stated once:

    destination  scores (C, cap_d) fp32, payload (C, cap_d) uint8, counts (n_cnt,) int32 with n_cnt == 1 (one count for all classes) or C,
                 extra (n_extra,) int32 (additive integers carried along: n_gt of segment AP; none for the frame meter), ONE flags word.
    sources      R >= 1 parts in one call: scores (R, C, cap_s), payload (R, C, cap_s), counts (R, n_cnt), extra (R, n_extra), flags (R,).
                 Sources and destination do not overlap.
    M1. a source count outside [0, cap_s] makes the call a refusal: nothing is written, no count or extra changes, and flag bit 2 (value 4,
        AP_FLAG_BAD_SOURCE, "malformed source") is set.
    M2. totals in 64-bit integers: tot[c] = counts_d[c] + sum_r counts_s[r][c].  Any tot[c] > cap_d (or a destination count below 0) is a
        refusal: nothing is written, nothing changes, and the overflow bit (value 2, cfn_ap_append's) is set.  Any summed extra that leaves
        int32 is a refusal in the same way.  All or nothing: cfn_ap_append's semantics.
    M3. otherwise row i of part r, class c goes to destination row counts_d[c] + sum_{q<r} counts_s[q][c] + i.  Scores and payload are copied
        as BITS (NaN payloads, -0.0 and denormals stay as they are); counts and extras advance by the sums; rows behind the new counts are
        untouched.
    M4. in every case, refusals included, flags |= OR_r flags_s[r]: a batch dropped on any rank taints the merged value.

``merge_reference`` spells the rule in numpy (in place, on numpy arrays or CPU tensors) and is the tests' reference; ``stack_parts`` builds the
(R, C, m) sources from several stores; ``gather_stores`` is the collective: every rank ends with the concatenation of all ranks' stores in
rank order.  Limits: C and R <= 65535, capacities < 2^31; the merged store is materialised whole on every rank (the sum of the ranks' rows:
5 bytes per row and class).  This module is host only (numpy + torch) apart from the call into cfn_hip.ops.
"""
import numpy as np
import torch

AP_FLAG_OVERFLOW, AP_FLAG_BAD_SOURCE = 2, 4


def _arr(x, dtype):
    """a numpy VIEW of a CPU tensor or array (written in place), bits kept: fp32 stores are handled as their int32 patterns"""
    if x is None:
        return None
    a = x.detach().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.dtype == np.float32 and dtype == np.int32:
        a = a.view(np.int32)
    if a.dtype != dtype:
        raise TypeError('merge_reference: %s expected, got %s' % (np.dtype(dtype), a.dtype))
    return a


def merge_reference(dst_scores, dst_payload, dst_counts, dst_extra, dst_flags, src_scores, src_payload, src_counts, src_extra, src_flags, out=None):
    """M1-M4 in numpy, in place on the destination (numpy arrays or CPU tensors; ops.ap_merge's arguments, `out` is ignored).  Returns True
    when the rows were appended, False for a refusal."""
    ds, dp = _arr(dst_scores, np.int32), _arr(dst_payload, np.uint8)
    dc, de, df = _arr(dst_counts, np.int32), _arr(dst_extra, np.int32), _arr(dst_flags, np.int32).reshape(-1)
    ss, sp = _arr(src_scores, np.int32), _arr(src_payload, np.uint8)
    sc, se, sf = _arr(src_counts, np.int32), _arr(src_extra, np.int32), _arr(src_flags, np.int32).reshape(-1)
    C, cap_d = ds.shape
    R, _, cap_s = ss.shape
    n_cnt = dc.shape[0]
    if ss.shape[1] != C or dp.shape != ds.shape or sp.shape != ss.shape or n_cnt not in (1, C) or sc.shape != (R, n_cnt) or sf.shape != (R,) \
            or df.shape != (1,) or (de is None) != (se is None) or (de is not None and se.shape != (R, de.shape[0])):
        raise ValueError('merge_reference: inconsistent shapes')
    for r in range(R):                                                                # M4, refusals included
        df[0] |= sf[r]
    if ((sc < 0) | (sc > cap_s)).any():                                               # M1
        df[0] |= AP_FLAG_BAD_SOURCE
        return False
    tot = dc.astype(np.int64) + sc.astype(np.int64).sum(0)                            # M2
    ext = None if de is None else de.astype(np.int64) + se.astype(np.int64).sum(0)
    if (dc < 0).any() or (tot > cap_d).any() or (ext is not None and ((ext < -2 ** 31) | (ext > 2 ** 31 - 1)).any()):
        df[0] |= AP_FLAG_OVERFLOW
        return False
    for c in range(C):                                                                # M3
        j = 0 if n_cnt == 1 else c
        at = int(dc[j])
        for r in range(R):
            n = int(sc[r, j])
            ds[c, at:at + n] = ss[r, c, :n]
            dp[c, at:at + n] = sp[r, c, :n]
            at += n
    dc[:] = tot.astype(np.int32)
    if de is not None:
        de[:] = ext.astype(np.int32)
    return True


def stack_parts(meter_states, m=None):
    """several stores -> the sources of ONE merge: meter_states is a list of (scores (C, cap_i), payload (C, cap_i), counts (n_cnt,), extra
    (n_extra,) or None, flags (1,)) on one device -> (scores (R, C, m), payload (R, C, m), counts (R, n_cnt), extra (R, n_extra) or None, flags
    (R,)).  m: the rows per class to carry, an upper bound of every part's largest count (a host bound avoids the read-back); None: the
    largest count among them, with ONE read-back.  A part shorter than m is padded (the rows behind its count are never looked at)."""
    if not meter_states:
        raise ValueError('stack_parts: at least one store expected')
    counts = torch.stack([s[2].reshape(-1) for s in meter_states])
    if m is None:
        m = int(counts.max())
    m = max(int(m), 1)
    sc0, pl0 = meter_states[0][0], meter_states[0][1]
    if len(meter_states) == 1 and int(sc0.shape[1]) == m and sc0.is_contiguous() and pl0.is_contiguous():
        scores, payload = sc0.unsqueeze(0), pl0.unsqueeze(0)                          # (one part of the right width: its own stores, no copy)
    else:
        C = int(sc0.shape[0])
        scores = sc0.new_empty(len(meter_states), C, m)
        payload = pl0.new_empty(len(meter_states), C, m)
        for r, s in enumerate(meter_states):
            k = min(m, int(s[0].shape[1]))
            scores[r, :, :k].copy_(s[0][:, :k])
            payload[r, :, :k].copy_(s[1][:, :k])
    extra = None if meter_states[0][3] is None else torch.stack([s[3].reshape(-1) for s in meter_states])
    flags = torch.cat([s[4].reshape(-1) for s in meter_states])
    return scores, payload, counts, extra, flags


def world_size(group=None):
    """the ranks of `group`; 1 without an initialised process group"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return int(dist.get_world_size(group))


def gather_stores(scores, payload, state, n_cnt, group=None, merge=None):
    """The stores of ALL ranks of `group`, appended in rank order into a fresh store sized by the total -> (scores (C, cap), payload (C, cap),
    state) with cap = the largest per-class total (at least 1); the same bits on every rank.  scores (C, cap_i) fp32, payload (C, cap_i)
    uint8 and state = [counts (n_cnt), extra (...), flags (1)] int32 are this rank's and stay untouched.  A COLLECTIVE: every rank calls it.
    One all_gather_into_tensor of the states; ONE read-back of two ints taken from the gathered tensor (the largest count m and the largest
    per-class total: the same tensor on every rank, so nothing further is needed to agree); one all_gather_into_tensor each of scores[:, :m]
    and payload[:, :m] (skipped when m == 0: nobody holds a row); one merge (M1-M4).  Only torch.distributed on whatever device the tensors
    live on: over gloo with CPU tensors, `merge` = merge_reference -- for tests only; product code passes nothing (ops.ap_merge)."""
    import torch.distributed as dist
    if merge is None:
        from . import ops
        merge = ops.ap_merge
    W = dist.get_world_size(group)
    n_cnt, L = int(n_cnt), int(state.numel())
    C = int(scores.shape[0])
    n_extra = L - n_cnt - 1
    if state.dtype != torch.int32 or state.dim() != 1 or n_cnt not in (1, C) or n_extra < 0:
        raise ValueError('gather_stores: state: (n_cnt + n_extra + 1,) int32 with n_cnt 1 or %d expected, got %s %s' % (C, state.dtype, tuple(state.shape)))
    dev = scores.device
    gathered = torch.empty(W * L, dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(gathered, state.contiguous(), group=group)
    g = gathered.view(W, L)
    cnt = g[:, :n_cnt].to(torch.int64)
    m, total = (int(x) for x in torch.stack([cnt.max(), cnt.sum(0).max()]).cpu())     # the ONE read-back
    if m > 0:
        mine_s, mine_p = scores.new_empty(C, m), payload.new_empty(C, m)
        k = min(m, int(scores.shape[1]))                                              # (this rank's stores may be shorter than the fullest rank's count)
        mine_s[:, :k].copy_(scores[:, :k])
        mine_p[:, :k].copy_(payload[:, :k])
        src_s, src_p = scores.new_empty(W, C, m), payload.new_empty(W, C, m)
        dist.all_gather_into_tensor(src_s.view(-1), mine_s.view(-1), group=group)      # (flat: the one layout every backend takes)
        dist.all_gather_into_tensor(src_p.view(-1), mine_p.view(-1), group=group)
    else:                                                                             # nobody holds a row: extras and flags still merge
        src_s, src_p = scores.new_zeros(W, C, 1), payload.new_zeros(W, C, 1)
    cap = max(total, 1)
    out_s, out_p = scores.new_empty(C, cap), payload.new_empty(C, cap)
    out_state = torch.zeros(L, dtype=torch.int32, device=dev)
    merge(out_s, out_p, out_state[:n_cnt], out_state[n_cnt:L - 1] if n_extra else None, out_state[L - 1:],
          src_s, src_p, g[:, :n_cnt].contiguous(), g[:, n_cnt:L - 1].contiguous() if n_extra else None, g[:, L - 1].contiguous())
    return out_s, out_p, out_state
