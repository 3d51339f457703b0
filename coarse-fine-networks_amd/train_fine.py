"""train_fine -- entry point #1 of the reference (train_fine.py) on the MI355X engine.

    python train_fine.py -gpu 0,1,...            one process per listed GPU is spawned (RCCL all-reduce)
    torchrun --nproc-per-node N train_fine.py    same thing under an external launcher

Same ``run()`` keyword arguments, loss, optimiser, LR schedule, phase pattern and checkpoint dict as the
reference (train_fine.py:56-263).  The Charades JPEG pipeline is out of scope: batches come
from ``SyntheticCharades`` which yields the same structures and shapes ``mt_collate_fn`` produces
(charades_fine.py:201-224); plug a real loader in through ``run(dataloaders=...)``.

DataParallel -> one-process-per-GPU differences that are handled explicitly:
  * the loc-loss normaliser sum(masks) is taken over the GLOBAL batch (all-reduced scalar);
  * BN statistics stay per replica; rank 0's running stats are broadcast before eval / checkpoints;
  * short last batches are skipped as in the reference (train_fine.py:180-181).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import x3d_fine                                   # noqa: E402
from cfn_hip import dist as cdist                 # noqa: E402
from cfn_hip import staging                       # noqa: E402
from cfn_hip.u8clips import RawU8Clips, U8Clips, CHARADES_MEAN, CHARADES_STD   # noqa: E402,F401
from cfn_hip.jpegdec import JpegClips, decode_checked        # noqa: E402
from apmeter import APMeter                       # noqa: E402
from cfn_hip import metrics                       # noqa: E402
from cfn_hip.seglabels import materialize         # noqa: E402
from cfn_hip.detections import DetectionWriter, epoch_path   # noqa: E402
from cfn_hip.seglabels import SegLabels           # noqa: E402

BS = 8
BS_UPSCALE = 1
INIT_LR = 0.01 * BS_UPSCALE
X3D_VERSION = 'M'
CHARADES_TR_SIZE = 7900
CHARADES_VAL_SIZE = 1850
NUM_CLASSES = 157


class SyntheticCharades(object):
    """Iterable of collated batches shaped like the reference loader's output for task='loc':
    inputs (B,1,3,T,H,W) fp32, labels (B,157,TL) in {0,1}, masks (B,TL), names."""

    def __init__(self, batch_size, iters, frames=64, crop=224, stride=10, seed=0, device='cpu', label_p=0.05):
        self.bs, self.iters, self.T, self.crop, self.stride = batch_size, iters, frames, crop, stride
        self.seed, self.device, self.p = seed, device, label_p

    def __len__(self):
        return self.iters

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        tl = self.T * self.stride
        for i in range(self.iters):
            x = torch.randn(self.bs, 1, 3, self.T, self.crop, self.crop, generator=g)
            labels = (torch.rand(self.bs, NUM_CLASSES, tl, generator=g) < self.p).float()
            masks = torch.ones(self.bs, tl)
            yield x, labels, masks, ['synthetic_%d' % i] * self.bs


def fused_loss_enabled(fused=None):
    """the opt-in switch of the fused detection loss (cfn_hip.ops.detection_loss): an explicit True / False, or None = the environment
    variable CFN_FUSED_LOSS, read at every call (default off)"""
    if fused is None:
        return os.environ.get('CFN_FUSED_LOSS', '0') not in ('', '0')
    return bool(fused)


def detection_loss(per_frame_logits, labels, masks, align_corners=True, group=None, crops=1, local_norm=False, mask_total=None, fused=None):
    """cls + loc loss of train_fine.py:199-213 for one rank's shard.

    ``loc_loss`` is normalised by the GLOBAL sum(masks) and multiplied by the world size, so that the
    average of the ranks' gradients equals the gradient of the reference's gathered-batch loss.
    crops = n > 1: validation-time multi-crop, logits are (b*n, C, T) against (b, ...) labels / masks; the per-frame
    probability is the max over the n crops of a video (train_fine.py:204-207).  local_norm=True (evaluation): this
    rank's own sum(masks) and no world factor -- no collective, ranks may hold different numbers of videos.
    mask_total: the global sum(masks) computed beforehand (cfn_hip.graph.GraphedDPStep takes the collective out of the captured part).
    fused (see fused_loss_enabled): device fp32 logits go through ONE forward and ONE backward kernel (cfn_hip.ops.detection_loss)
    instead of the operator chain below; anything else (CPU tensors, other dtypes) takes the chain as before."""
    if fused_loss_enabled(fused) and per_frame_logits.is_cuda and per_frame_logits.dtype == torch.float32:
        from cfn_hip import ops
        world = 1
        if not local_norm and torch.distributed.is_initialized():
            world = torch.distributed.get_world_size(group)
        if mask_total is not None:
            norm = mask_total * labels.shape[1]
        elif world > 1:                              # the normaliser is global: one collective, as below
            norm = cdist.global_mask_count(masks, group) * labels.shape[1]
        else:
            norm = None                              # the kernel sums this shard's masks itself
        return ops.detection_loss(per_frame_logits, labels, masks, align_corners, crops, norm, float(world), True)
    tl = labels.size(2)
    if per_frame_logits.is_cuda:
        from cfn_hip import ops
        logits = ops.time_resize(per_frame_logits, tl, align_corners)   # = F.interpolate(mode='linear', align_corners=...)
    else:
        logits = F.interpolate(per_frame_logits, tl, mode='linear', align_corners=align_corners)
    if crops > 1:
        logits = logits.view(labels.shape[0], crops, logits.shape[1], tl)
        probs = torch.max(torch.sigmoid(logits), dim=1)[0] * masks.unsqueeze(1)
    else:
        probs = torch.sigmoid(logits) * masks.unsqueeze(1)
    cls_loss = F.binary_cross_entropy(torch.max(probs, dim=2)[0], torch.max(labels, dim=2)[0])
    world = 1
    if not local_norm and torch.distributed.is_initialized():
        world = torch.distributed.get_world_size(group)
    norm = (cdist.global_mask_count(masks, group, local=local_norm) if mask_total is None else mask_total) * labels.shape[1]
    loc_loss = F.binary_cross_entropy(probs, labels, reduction='sum') / norm * world
    return cls_loss, loc_loss, probs


def _mean_ap(apm):
    v = apm.value()
    return float(v.mean()) if torch.is_tensor(v) else float(v)


def lr_warmup(init_lr, cur_steps, warmup_steps, opt):
    start_after = 1
    if cur_steps < warmup_steps and cur_steps > start_after:
        lr_scale = min(1., float(cur_steps + 1) / warmup_steps)
        for pg in opt.param_groups:
            pg['lr'] = lr_scale * init_lr


def build_model(device, n_classes=NUM_CLASSES, pretrained=None, dropout=0.5, act_dtype=None, input_norm=None):
    """input_norm = (mean, std[, norm_value]): the net also takes uint8 frames (collate.fine_collate_u8) and normalises them in the stem
    conv, e.g. (CHARADES_MEAN, CHARADES_STD) -- the reference's Normalize(CHARADES_MEAN, CHARADES_STD), train_fine.py:77-80"""
    net = x3d_fine.generate_model(x3d_version=X3D_VERSION, n_classes=400, n_input_channels=3, task='loc',
                                  dropout=dropout, base_bn_splits=1, t_downsample=False, extract_feat=False,
                                  act_dtype=act_dtype)
    if pretrained:      # partial state.update as train_fine.py:104-107; a missing file raises, as in the reference
        ckpt = torch.load(pretrained, map_location='cpu')
        state = net.state_dict()
        state.update(ckpt['model_state_dict'])
        net.load_state_dict(state)
    net.replace_logits(n_classes)
    if input_norm is not None:
        net.set_input_norm(*input_norm)
    return net.to(device)


def flatten_clips(inputs, dev, crop=None, names=None, jpeg_entropy=None):
    """(b, n crops, ...) -> (b * n, ...) on `dev`: an fp32 clip tensor (b, n, 3, T, H, W), a U8Clips batch, or a RawU8Clips batch
    (frames as decoded + crop boxes, collate.fine_collate_raw_u8), which is cropped, resized to `crop` x `crop` and flipped on `dev`, on
    the current stream, into the U8Clips batch the net takes (crop=None: handed on as it is).  A JpegClips batch (frames still JPEG,
    collate.fine_collate_jpeg) is first decoded on `dev`, on the current stream, into that RawU8Clips batch; its status words are read
    back once, and a frame that did not decode raises, naming the video (names: one per video of the batch).  jpeg_entropy: the entropy
    mode of that decode, 'interval' or 'sync' (cfn_hip.jpegdec.decode_checked; None leaves the choice to CFN_JPEG_ENTROPY)."""
    if isinstance(inputs, JpegClips):
        inputs = decode_checked(inputs, dev, names, entropy=jpeg_entropy)
    if isinstance(inputs, RawU8Clips):
        raw = inputs.flatten_crops().to(dev, non_blocking=True)
        return raw if crop is None else raw.transform(crop)
    if isinstance(inputs, U8Clips):
        return inputs.flatten_crops().to(dev, non_blocking=True)
    b, n = inputs.shape[:2]
    return inputs.view((b * n,) + tuple(inputs.shape[2:])).to(dev, non_blocking=True)


def forward_backward(net, inputs, labels, masks, gamma_tau=5, mask_total=None, fused=None):
    """forward + loss + backward of one shard (no collective when mask_total is given, no optimizer): the capturable part of a
    data-parallel step (cfn_hip.graph.GraphedDPStep).  With fp16 activations the loss is multiplied by the net's loss scale:
    EVERY caller runs `post_reduce(net)` between the gradient reduction and the optimizer (train_step below does; GraphedDPStep takes it
    as its `post_reduce` hook and captures it in front of the optimizer graph).  fused: see detection_loss."""
    masks_clip = masks[:, ::gamma_tau * 2]
    logits = net([inputs, masks_clip])
    cls_loss, loc_loss, probs = detection_loss(logits, labels, masks, True, mask_total=mask_total, fused=fused)
    loss = (cls_loss + loc_loss) / 2
    scaler = loss_scaler(net)
    (loss if scaler is None else scaler.scale_loss(loss)).backward()
    return cls_loss.detach(), loc_loss.detach(), probs.detach()


# fp16 activation path (x3d_fine act_dtype='fp16', BASELINE configs[4]): activation gradients are stored as IEEE half (5 exponent bits), so the
# backward pass runs on a scaled loss; weight gradients accumulate in fp64 / fp32 and are divided by the scale before the optimizer step.
# Initial scale (gradients of this loss at the logits are ~1 / (B x 157 x T)); it is halved on the device whenever a gradient overflowed.
LOSS_SCALE_FP16 = 4096.0


class LossScaler(object):
    """Loss scale of the fp16 path, kept ON THE DEVICE: no host synchronisation, so the whole sequence survives hipGraph capture.

    `scale_loss` multiplies by the current scale; `unscale_` divides the gradients by it, and if ANY gradient is inf / nan (a half-stored
    activation gradient saturated) it zeroes ALL of them -- the optimizer step that follows then applies momentum and weight decay only,
    instead of poisoning the weights -- and halves the scale; after `interval` clean steps the scale doubles (torch's GradScaler rule,
    `torch._amp_update_scale_`, without its `.item()`)."""

    def __init__(self, device, init=LOSS_SCALE_FP16, backoff=0.5, growth=2.0, interval=2000):
        self.scale = torch.full((1,), float(init), dtype=torch.float32, device=device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=device)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=device)
        self.backoff, self.growth, self.interval = backoff, growth, interval

    def scale_loss(self, loss):
        return loss * self.scale.to(loss.dtype).squeeze(0)

    def unscale_(self, params):
        grads = [p.grad for p in params if p.grad is not None]
        if not grads:
            return
        self.found_inf.zero_()
        by_kind = {}
        for g in grads:
            by_kind.setdefault((g.device, g.dtype), []).append(g)
        inv = self.scale.double().reciprocal().float()
        for gs in by_kind.values():
            torch._amp_foreach_non_finite_check_and_unscale_(gs, self.found_inf, inv)
        # all-or-nothing without a host decision and without ever multiplying an inf / nan (inf * 0 = nan): the gradients' BIT PATTERNS are
        # multiplied by an int32 0 / 1 -- two multi-tensor launches for the whole parameter set (a per-tensor nan_to_num_ was ~300 launches)
        keep = (1.0 - self.found_inf).to(torch.int32).squeeze(0)          # 1 = clean step, 0 = an overflow somewhere
        torch._foreach_mul_([g.view(torch.int32) for g in grads if g.dtype == torch.float32], keep)
        rest = [g for g in grads if g.dtype != torch.float32]
        if rest:                                                          # (no such gradient on this path; kept correct)
            for g in rest:
                g.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
            torch._foreach_mul_(rest, (1.0 - self.found_inf).squeeze(0))
        torch._amp_update_scale_(self.scale, self.tracker, self.found_inf, self.growth, self.backoff, self.interval)


def loss_scale(*nets):
    """the INITIAL loss scale of a set of nets (1 unless one of them stores fp16 activations)"""
    return LOSS_SCALE_FP16 if any(getattr(n, 'act_dtype', None) == torch.float16 for n in nets) else 1.0


def loss_scaler(*nets):
    """the LossScaler shared by `nets` (created on first use, kept on the first fp16 net); None when no net stores fp16 activations"""
    for n in nets:
        if getattr(n, 'act_dtype', None) == torch.float16:
            sc = getattr(n, '_cfn_loss_scaler', None)
            if sc is None:
                sc = LossScaler(next(n.parameters()).device)
                object.__setattr__(n, '_cfn_loss_scaler', sc)
            return sc
    return None


def unscale_grads(params, scale):
    """scale: a LossScaler (overflow-checked, see there), None / 1.0 (nothing to do) or a plain factor"""
    if isinstance(scale, LossScaler):
        scale.unscale_(list(params))
    elif scale is not None and scale != 1.0:
        grads = [p.grad for p in params if p.grad is not None]
        if grads:
            torch._foreach_mul_(grads, 1.0 / scale)


def post_reduce(net):
    """what has to run between the gradient reduction and optimizer.step() -- the other half of forward_backward's loss scale"""
    unscale_grads(net.parameters(), loss_scaler(net))


def train_step(net, reducer, optimizer, inputs, labels, masks, gamma_tau=5, pre_step=None, fused=None):
    """one optimisation step on this rank's shard; returns (cls_loss, loc_loss, probs).  pre_step() runs between the
    gradient reduction and optimizer.step() -- where the reference adjusts the warm-up learning rate
    (train_fine.py:241-244).  fused: see detection_loss."""
    reducer.begin_pass()
    cls_loss, loc_loss, probs = forward_backward(net, inputs, labels, masks, gamma_tau, fused=fused)
    reducer.finish()
    post_reduce(net)
    if pre_step is not None:
        pre_step()
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    return cls_loss, loc_loss, probs


_ap_rows = metrics.ap_rows      # per video: (scores (v,157), targets (v,157)) numpy over the valid frames -- what APMeter.add takes


def run(init_lr=INIT_LR, warmup_steps=0, max_epochs=200, mode='rgb', root=None, train_split=None,
        batch_size=BS * BS_UPSCALE, frames=80 * 4, dataloaders=None, max_steps=None, save_model='models/fine_charades_',
        pretrained='models/x3d_multigrid_kinetics_fb_pretrained.pt', log=print, phase_hook=None, input_norm=None,
        device_ap=False, fused_loss=False, jpeg_entropy=None, detections=None, segment_ap=None, calibration=None, proposal_recall=None):
    """detections: a cfn_hip.detections.DetectionWriter -- every validation phase decodes its probs into activity segments on the GPU
    (cfn_hip.ops.decode_segments) and rank 0 writes them, all ranks' videos, as JSON lines to the writer's path with the epoch inserted
    (cfn_hip.detections.epoch_path); seconds when the loaders collate SegLabel samples, frames otherwise.  None: nothing changes.
    segment_ap: a cfn_hip.segap.SegmentAPMeter -- every validation phase matches the same decoded segments (the writer's decode; the meter's
    own thr / max_gap / min_len without a writer) against the batch's segment labels on the GPU and logs ' Epoch:E val seg-mAP@t: ...' behind the
    existing line.  AP is not additive, so a plain meter is one process's and a world size above 1 raises; a meter made with across_ranks=True
    (--seg-ap-all-ranks) evaluates the stores of all ranks appended in rank order on the GPU (cfn_hip/apmerge.py): every rank builds the line
    (a collective), rank 0 logs it.  None: nothing changes.  A writer or a meter made with levels= decodes with cfn_hip.detections.propose instead (candidates at K
    levels, then temporal NMS -- soft-NMS when it was also made with soft=); the meter is still fed the writer's batch when both are given.
    A writer or a meter made with filter= (a cfn_hip.scorefilter.ScoreFilter, --detect-smooth) smooths the probs on the GPU in front of that decode
    (DESIGN 4.23); the frame-mAP line and the loss stay on the raw probs.
    calibration: a cfn_hip.calibrate.Calibration whose thr_vector / levels the writer and the meter were made with -- wherever a
    proposal_recall: a cfn_hip.recall.ProposalRecallMeter -- every validation phase feeds it the very Detections the writer or the segment-AP
    meter made (no second decode, so one of the two must be given) and logs ' Epoch:E val AR@1: ... AR@10: ... AR@N: ... AUC: ... props/video:
    ...' behind the other lines.  Its state is additive, so unlike segment_ap a world size above 1 is allowed: the line's value is all-reduced
    and rank 0 logs it.  None: nothing changes.
    training mAP is taken the same sorted rows give the per-class thresholds (StepMetrics.mean_ap(calibration): no read-back of its own), and
    a validation phase that starts with rows the meter still holds calibrates from those first (StepMetrics.calibrate); each is followed by one
    ' Epoch:E calibrated ...' line (Calibration.summary_line, one read-back of a few integers).  The validation decode then reads the updated
    tensor.  The calibration in front of a validation phase is skipped when an mAP line has updated the thresholds since the last validation
    phase: the leftover of an interval (possibly a step or two) never replaces the thresholds of a whole one.  Every rank calibrates from
    its own rows, so the calibration lives on the rank's device.  Needs device_ap=True.  None: nothing changes.
    input_norm: see build_model -- needed when the loaders collate uint8 frames (collate.fine_collate_u8, or fine_collate_raw_u8:
    untransformed frames + crop boxes, cropped / resized to the model's crop size / flipped on the GPU in front of the step).
    device_ap: the training phases keep their AP rows and loss totals on the GPU (cfn_hip.metrics.StepMetrics, apmeter.DeviceAPMeter):
    no read-back per step, the host waits for the device only where a line is logged.
    fused_loss: the loss of every step and of validation runs as one forward and one backward kernel (detection_loss(fused=True)); False leaves
    the choice to CFN_FUSED_LOSS.
    jpeg_entropy: how JpegClips batches are entropy-decoded, 'interval' or 'sync' (flatten_clips); None leaves the choice to CFN_JPEG_ENTROPY."""
    check_calibration(calibration, device_ap)
    fused = True if fused_loss else None
    rank, world, dev = cdist.init_from_env()
    check_segment_ap(segment_ap, world)
    check_proposal_recall(proposal_recall, detections, segment_ap)
    check_calibration(calibration, device_ap, dev)
    gamma_tau = {'S': 6, 'M': 5, 'XL': 5}[X3D_VERSION]
    crop = {'S': 160, 'M': 224, 'XL': 312}[X3D_VERSION]
    clip_frames = frames * 2 // (gamma_tau * 2)          # 640-frame window at stride 10 -> 64 frames
    local_bs = max(batch_size // world, 1)
    iters = CHARADES_TR_SIZE // batch_size
    val_bs = max(batch_size // 2 // world, 1)
    val_iters = CHARADES_VAL_SIZE // max(batch_size // 2, 1)
    if dataloaders is None:
        dataloaders = {'train': SyntheticCharades(local_bs, iters, clip_frames, crop, gamma_tau * 2, seed=rank),
                       'val': SyntheticCharades(val_bs, val_iters, clip_frames, crop, gamma_tau * 2, seed=1000 + rank)}
    net = build_model(dev, pretrained=pretrained, input_norm=input_norm)
    cdist.sync_module(net)        # one model on every rank (DataParallel replicates rank 0's; fc2 was just re-drawn)
    optimizer = optim.SGD(net.parameters(), lr=init_lr, momentum=0.9, weight_decay=1e-5)
    lr_sched = optim.lr_scheduler.MultiStepLR(optimizer, [15, 20, 25])
    reducer = cdist.GradReducer(net.parameters())
    tr, val_apm = metrics.StepMetrics(device_ap, dev), APMeter()
    # batches reach HBM through a pinned slab on a copy stream, one batch ahead of the step (the reference: a synchronous `.cuda()` per tensor
    # in front of every step, train_fine.py:184-197); the `.to(dev)` calls below are no-ops on staged batches
    stager = staging.HostStager(dev) if dev.type == 'cuda' else None
    steps, epochs = 0, 0
    cal_seen = 0          # calibration.updates at the end of the last validation phase
    while epochs < max_epochs:
        for phase in 4 * ['train'] + ['val']:
            train = phase == 'train'
            net.train(train)
            if train:
                epochs += 1
            else:
                cdist.broadcast_buffers(net)
                net.aggregate_sub_bn_stats()
            tot_loc = tot_cls = 0.0
            n_it = 0
            val_rows = []
            # no mAP line calibrated since the last validation phase: take the rows the meter holds (a leftover never replaces a whole interval)
            if not train and calibration is not None and calibration.updates == cal_seen and tr.calibrate(calibration) and rank == 0:
                log(calibration_line(calibration, epochs))
            tr.start_phase()
            for inputs, labels, masks, _name in (stager.stage(dataloaders[phase]) if stager else dataloaders[phase]):
                want = local_bs if train else val_bs
                ok = inputs.shape[0] == want
                if train:      # the skip is a collective decision: no rank may leave the others alone in an all-reduce
                    ok = cdist.all_agree(ok, dev) if world > 1 else ok
                if not ok:
                    continue
                b, n = inputs.shape[:2]          # n crops per video (1 in training, train_fine.py:176-185)
                inputs = flatten_clips(inputs, dev, crop, names=_name, jpeg_entropy=jpeg_entropy)
                seg_batch = labels if detections is not None or segment_ap is not None else None      # (its fps / window, before materialize drops the SegLabels)
                labels, masks = materialize(labels, masks, dev)      # dense tensors: .to(dev); a SegLabels batch (segment labels): one kernel
                valid_t = masks.sum(1).int()
                n_it += 1
                if train:
                    warm = (lambda: lr_warmup(init_lr, steps, warmup_steps, optimizer))
                    cls_loss, loc_loss, probs = train_step(net, reducer, optimizer, inputs, labels, masks, gamma_tau, pre_step=warm, fused=fused)
                    steps += 1
                    tr.update(cls_loss, loc_loss, probs, labels, valid_t)
                else:
                    with torch.no_grad():
                        logits = net([inputs, masks[:, ::gamma_tau * 2]])
                        cls_loss, loc_loss, probs = detection_loss(logits, labels, masks, True, crops=n, local_norm=True, fused=fused)
                    val_rows.extend(_ap_rows(probs, labels, valid_t))
                    det = None
                    if detections is not None:      # decoded on the device; the segments stay there until the end of the phase
                        det = detections.add(probs, valid_t, seg_batch, _name)
                    if segment_ap is not None:      # matched and appended on the device; nothing is read back before the end of the phase
                        det = segment_ap_add(segment_ap, det, probs, valid_t, seg_batch, labels, writer=detections)
                    if proposal_recall is not None:      # the same Detections once more; its counts stay on the device
                        proposal_recall_add(proposal_recall, det, valid_t, seg_batch, labels)
                    tot_cls += float(cls_loss)
                    tot_loc += float(loc_loss)
                if train and steps % max(iters // 2, 1) == 0:
                    t_loc, t_cls = tr.totals()
                    m_loc, m_cls = cdist.mean_over_ranks([t_loc / n_it, t_cls / n_it], dev)
                    if rank == 0 or calibration is not None:      # (a rank's thresholds come from the sort behind its own mAP)
                        m_ap = tr.mean_ap(calibration)
                    if rank == 0:
                        log(' Epoch:{} {} steps: {} Loc Loss: {:.4f} Cls Loss: {:.4f} mAP: {:.4f}'.format(
                            epochs, phase, steps, m_loc, m_cls, m_ap))
                        if calibration is not None:
                            log(calibration_line(calibration, epochs))
                    tr.reset_ap()
                if train and steps % 1000 == 0 and rank == 0:
                    os.makedirs(os.path.dirname(save_model) or '.', exist_ok=True)
                    torch.save({'model_state_dict': net.state_dict(), 'optimizer_state_dict': optimizer.state_dict(),
                                'scheduler_state_dict': lr_sched.state_dict()}, save_model + str(steps).zfill(6) + '.pt')
                if max_steps is not None and steps >= max_steps:
                    return net
            if not train:
                # every rank validated its own shard: the reported mAP / losses cover the WHOLE validation set
                gathered = cdist.gather_objects((val_rows, tot_loc, tot_cls, n_it))
                if rank == 0:
                    g_loc = g_cls = 0.0
                    g_it = 0
                    for rows, r_loc, r_cls, r_it in gathered:
                        for sc, tg in rows:
                            val_apm.add(sc, tg)
                        g_loc, g_cls, g_it = g_loc + r_loc, g_cls + r_cls, g_it + r_it
                    log(' Epoch:{} val Loc Loss: {:.4f} Cls Loss: {:.4f} mAP: {:.4f}'.format(
                        epochs, g_loc / max(g_it, 1), g_cls / max(g_it, 1), _mean_ap(val_apm)))
                if detections is not None:      # every rank's videos, one file per validation phase
                    det_rows = cdist.gather_objects(detections.take())
                    if rank == 0:
                        detections.flush(epoch_path(detections.path, epochs), [r for part in det_rows for r in part])
                if segment_ap is not None:
                    line = segment_ap_line(segment_ap, epochs)      # (a collective with an across_ranks meter under a world size above 1: every rank)
                    if rank == 0:
                        log(line)
                if proposal_recall is not None:
                    line = proposal_recall_line(proposal_recall, epochs)      # (a collective under a world size above 1: every rank)
                    if rank == 0:
                        log(line)
                val_apm.reset()
                cal_seen = calibration.updates if calibration is not None else 0
                lr_sched.step()            # once per val phase, as the reference (not per epoch, not per step)
            if phase_hook is not None:         # test / logging hook: end of a phase (not in the reference's signature)
                phase_hook(phase, epochs, optimizer)
    return net


def check_segment_ap(meter, world):
    """a plain SegmentAPMeter works in ONE process: AP is not additive.  One made with across_ranks=True (--seg-ap-all-ranks) evaluates the
    stores of all ranks appended in rank order (cfn_hip/apmerge.py) and passes"""
    if meter is not None and world > 1 and not getattr(meter, 'across_ranks', False):
        raise RuntimeError('segment_ap: a SegmentAPMeter holds the detections of ONE process; AP is not additive over ranks and this meter does '
                           'not merge their stores (world size %d): validate on one GPU, leave segment_ap=None, or make the meter with '
                           'across_ranks=True (--seg-ap-all-ranks)' % world)


def check_calibration(calibration, device_ap, dev=None):
    """a Calibration takes its rows from the device meter of the training phases, so it lives on this rank's device `dev`"""
    if calibration is not None and not device_ap:
        raise RuntimeError('calibration: the thresholds are calibrated from the AP rows the training phases keep on the GPU: '
                           '--detect-calibrate needs --device-ap (run(device_ap=True))')
    if calibration is not None and dev is not None and calibration.thr.device != dev:
        raise RuntimeError('calibration: its tensors are on %s but this rank trains on %s: make the Calibration on the rank\'s own device '
                           '(cfn_hip.dist.local_device())' % (calibration.thr.device, dev))


def calibration_line(calibration, epochs):
    """the line behind a training mAP line (ONE read-back of the calibration's integers)"""
    return ' Epoch:{} {}'.format(epochs, calibration.summary_line())


def segment_ap_add(meter, det, probs, valid_t, seg_batch, labels, writer=None):
    """one validation batch into the meter: `det` = what the DetectionWriter `writer` decoded (None: decode here with the meter's
    parameters and its filter -- propose() when it has levels); ground truth = the batch's SegLabels (seconds), or the dense labels decoded into frame units"""
    from cfn_hip.detections import decode, propose
    valid_t = valid_t.to(torch.int32)
    fps = start = None
    if isinstance(seg_batch, SegLabels):
        seg_batch = seg_batch.to(probs.device)
        fps, start = seg_batch.fps, seg_batch.window[:, 0].contiguous()
    levels = writer.n_levels if det is not None and writer is not None else meter.n_levels
    if det is None and meter.levels is not None:
        det = propose(probs.detach(), valid_t, fps, start, meter.levels, meter.nms, meter.nms_score, meter.max_gap, meter.min_len, soft=meter.soft,
                      filter=getattr(meter, 'filter', None))
    elif det is None:
        det = decode(probs.detach(), valid_t, fps, start, meter.thr, meter.max_gap, meter.min_len, filter=getattr(meter, 'filter', None))
    meter.add(det, seg_batch if fps is not None else (labels, valid_t), levels=levels)
    return det


def check_proposal_recall(meter, detections, segment_ap):
    """a ProposalRecallMeter is fed the Detections of the writer or of the segment-AP meter: without either no decode exists"""
    if meter is not None and detections is None and segment_ap is None:
        raise RuntimeError('proposal_recall: the meter is fed the segments a DetectionWriter (detections=) or a SegmentAPMeter (segment_ap=) decodes '
                           'in the validation phase, and neither was given: a decode does not exist')


def proposal_recall_add(meter, det, valid_t, seg_batch, labels):
    """one validation batch into the recall meter: `det` = what the writer or the segment-AP meter decoded; the ground truth as segment_ap_add
    takes it"""
    meter.add(det, seg_batch.to(det.seg.device) if isinstance(seg_batch, SegLabels) else (labels, valid_t.to(torch.int32)))


def proposal_recall_line(meter, epochs):
    """the phase's line (ONE read-back; summed over the ranks of a process group), and the meter is empty again"""
    v = meter.value(group=None)
    meter.reset()
    ar = v['ar']
    at = sorted({1, min(10, meter.n_max), meter.n_max})
    return ' Epoch:{} val {} AUC: {:.4f} props/video: {:.1f}'.format(epochs, ' '.join('AR@{}: {:.4f}'.format(n, float(ar[n - 1])) for n in at),
                                                                    float(v['auc']), float(v['avg_props']))


def segment_ap_line(meter, epochs):
    """the phase's line (ONE read-back), and the meter is empty again"""
    _, mp = meter.value()
    meter.reset()
    return ' Epoch:{} val {}'.format(epochs, ' '.join('seg-mAP@{:g}: {:.4f}'.format(t, float(m)) for t, m in zip(meter.tiou, mp)))


def seg_ap_arguments(parser):
    """the --seg-ap group: segment-level AP at tIoU thresholds of every validation phase (cfn_hip.segap.SegmentAPMeter)"""
    g = parser.add_argument_group('segment AP')
    g.add_argument('--seg-ap', action='store_true', help='log seg-mAP@tIoU of every validation phase (one process; several ranks with --seg-ap-all-ranks)')
    g.add_argument('--seg-ap-tiou', default='0.1,0.3,0.5,0.7,0.9', help='1 to 8 tIoU thresholds in (0, 1], comma separated')
    g.add_argument('--seg-ap-score', choices=('max', 'mean'), default='max', help='the score column detections are ranked by')
    g.add_argument('--seg-ap-capacity', type=int, default=None, help='rows per class, fixed (default: the stores grow)')
    g.add_argument('--seg-ap-all-ranks', action='store_true',
                   help='with --seg-ap under several ranks: evaluate the detections of ALL ranks, their stores appended in rank order on the GPU '
                        '(every rank gets the same value; rank 0 logs it)')
    return parser


def seg_ap_argv(args):
    """the --seg-ap group of `args` as a worker's command line"""
    if not args.seg_ap:
        return []
    return ['--seg-ap', '--seg-ap-tiou', args.seg_ap_tiou, '--seg-ap-score', args.seg_ap_score] + \
        (['--seg-ap-capacity', str(args.seg_ap_capacity)] if args.seg_ap_capacity is not None else []) + \
        (['--seg-ap-all-ranks'] if getattr(args, 'seg_ap_all_ranks', False) else [])


def seg_ap_from_args(args, n_classes=157, calibration=None):
    """the meter of the --seg-ap group on this process's GPU (decode parameters: the --detect group's; calibration: see detect_writer), or None"""
    if not args.seg_ap:
        return None
    from cfn_hip.segap import SegmentAPMeter
    smooth = detect_smooth(args)                # (refuses --detect-calibrate before a calibration is made)
    thr, more = _calibrated(args.detect_thr, detect_levels(args), calibration_from_args(args, n_classes) if calibration is None else calibration)
    return SegmentAPMeter(torch.device('cuda', torch.cuda.current_device()), n_classes, [float(x) for x in args.seg_ap_tiou.split(',')], args.seg_ap_score,
                          args.seg_ap_capacity, thr, args.detect_gap, args.detect_min_len, across_ranks=bool(getattr(args, 'seg_ap_all_ranks', False)),
                          filter=smooth, **more)


def add_detect_args(parser):
    """the --detect group: activity segments of every validation phase as JSON lines (cfn_hip.detections.DetectionWriter)"""
    g = parser.add_argument_group('detections')
    g.add_argument('--detect', metavar='PATH', default=None, help='write the decoded segments of every validation phase to PATH (epoch number inserted)')
    g.add_argument('--detect-thr', type=float, default=0.5, help='a frame is active when its probability is above this')
    g.add_argument('--detect-gap', type=int, default=0, help='close gaps of at most N inactive frames')
    g.add_argument('--detect-min-len', type=int, default=1, help='drop segments shorter than N frames')
    g.add_argument('--detect-levels', metavar='T1,T2,...', default=None,
                   help='proposals: candidates at these 1 to 16 thresholds in place of --detect-thr, e.g. 0.8,0.65,0.5,0.35,0.2 (high to low: '
                        'the tight segment wins a tie of nested candidates), then temporal NMS')
    g.add_argument('--detect-nms', type=float, default=None, help='with --detect-levels: suppress a candidate whose temporal IoU with a kept one is above this (default 0.5)')
    g.add_argument('--detect-nms-score', choices=('max', 'mean'), default='max', help='with --detect-levels: the score column NMS ranks by')
    g.add_argument('--detect-soft-nms', choices=('linear', 'gaussian'), default=None,
                   help='with --detect-levels: soft-NMS in place of NMS -- nothing is deleted by overlap, a score is decayed by the overlap with every '
                        'candidate ranked in front (linear: times 1 - tIoU where tIoU is above --detect-nms; gaussian: times exp(-tIoU^2 / sigma)), and '
                        'the list is cut by --detect-min-score or --detect-max-keep')
    g.add_argument('--detect-soft-sigma', type=float, default=None, help='with --detect-soft-nms gaussian: sigma, in [1/64, 2^20] (default 0.5)')
    g.add_argument('--detect-min-score', type=float, default=None, help='with --detect-soft-nms: stop at the first decayed score below this (default 0.001)')
    g.add_argument('--detect-max-keep', type=int, default=None, help='with --detect-soft-nms: at most N segments per video and class (default 0: no limit)')
    g.add_argument('--detect-smooth', metavar='SPEC', default=None,
                   help='smooth the per-frame scores on the GPU before they are thresholded: box:R | gaussian:SIGMA[:R] | median:R, R frames on each '
                        'side (at most 32; gaussian default: ceil(3 SIGMA)), the window truncated at the ends of the video.  The frame-mAP line and '
                        'the loss stay on the raw scores')
    g.add_argument('--prop-recall', action='store_true',
                   help='log the proposal recall AR@N of every validation phase (needs --detect or --seg-ap, whose decode it is fed: with '
                        '--detect-levels the proposals; any number of processes)')
    g.add_argument('--prop-recall-n', type=int, default=100, help='with --prop-recall: the largest N, 1 to 1024')
    g.add_argument('--prop-recall-tiou', default='0.5,0.55,0.6,0.65,0.7,0.75,0.8,0.85,0.9,0.95', help='with --prop-recall: 1 to 16 tIoU thresholds in (0, 1]')
    g.add_argument('--prop-recall-score', choices=('max', 'mean'), default='max', help='with --prop-recall: the score column the candidates of a video are ranked by')
    g.add_argument('--detect-calibrate', metavar='SPEC', default=None,
                   help="per-class thresholds calibrated on the GPU from the training AP rows (needs --device-ap): f1 | precision:P | recall:Q replaces "
                        "--detect-thr once the first training mAP is taken; recall:Q1,Q2,... (ascending: thresholds high to low) replaces the same "
                        "number of --detect-levels")


def detect_levels(args):
    """the proposal options of the --detect group as the keywords of DetectionWriter / SegmentAPMeter ({} without --detect-levels)"""
    method = getattr(args, 'detect_soft_nms', None)
    given = {k: getattr(args, 'detect_' + k, None) for k in ('soft_sigma', 'min_score', 'max_keep')}
    if method is None and any(v is not None for v in given.values()):
        raise ValueError('--detect-soft-sigma, --detect-min-score and --detect-max-keep need --detect-soft-nms linear|gaussian')
    if getattr(args, 'detect_levels', None) is None:
        if getattr(args, 'detect_nms', None) is not None:
            raise ValueError('--detect-nms needs --detect-levels: a single-level decode does not overlap itself')
        if method is not None:
            raise ValueError('--detect-soft-nms needs --detect-levels: a single-level decode does not overlap itself')
        return {}
    more = {'levels': [float(x) for x in args.detect_levels.split(',')], 'nms': args.detect_nms, 'nms_score': args.detect_nms_score}
    if method is not None:                                        # (the key only with the option: every caller without it sees the same dict)
        from cfn_hip.detections import SoftNMS
        if method == 'gaussian' and args.detect_nms is not None:
            raise ValueError('--detect-nms is the threshold of NMS and of --detect-soft-nms linear; gaussian does not use it')
        more['soft'] = SoftNMS(method)._replace(**{k: v for k, v in (('sigma', given['soft_sigma']), ('min_score', given['min_score']),
                                                                      ('max_keep', given['max_keep'])) if v is not None})
    return more


def detect_smooth(args):
    """the ScoreFilter of --detect-smooth (cfn_hip.scorefilter.parse_spec), or None without the option"""
    spec = getattr(args, 'detect_smooth', None)
    if spec is None:
        return None
    if getattr(args, 'detect_calibrate', None) is not None:
        raise ValueError('--detect-smooth with --detect-calibrate: the calibration rows are RAW frame scores (the training phases\' AP rows), so a '
                         'threshold calibrated on them says nothing about the smoothed scores it would be applied to: drop one of the two')
    from cfn_hip.scorefilter import parse_spec
    return parse_spec(spec)


def detect_argv(args):
    """the --detect group of `args` as a worker's command line"""
    if not args.detect:
        return []
    more = (['--detect-levels', args.detect_levels, '--detect-nms-score', args.detect_nms_score] if args.detect_levels is not None else []) + \
        (['--detect-nms', repr(args.detect_nms)] if args.detect_nms is not None else []) + \
        [x for flag, k, f in (('--detect-soft-nms', 'detect_soft_nms', str), ('--detect-soft-sigma', 'detect_soft_sigma', repr),
                              ('--detect-min-score', 'detect_min_score', repr), ('--detect-max-keep', 'detect_max_keep', str))
         if getattr(args, k, None) is not None for x in (flag, f(getattr(args, k)))] + \
        (['--detect-calibrate', args.detect_calibrate] if getattr(args, 'detect_calibrate', None) is not None else []) + \
        (['--detect-smooth', args.detect_smooth] if getattr(args, 'detect_smooth', None) is not None else [])
    return ['--detect', args.detect, '--detect-thr', repr(args.detect_thr), '--detect-gap', str(args.detect_gap), '--detect-min-len', str(args.detect_min_len)] + more


def prop_recall_argv(args):
    """the --prop-recall options of `args` as a worker's command line"""
    if not getattr(args, 'prop_recall', False):
        return []
    return ['--prop-recall', '--prop-recall-n', str(args.prop_recall_n), '--prop-recall-tiou', args.prop_recall_tiou, '--prop-recall-score',
            args.prop_recall_score]


def prop_recall_from_args(args, n_classes=157, device=None):
    """the meter of --prop-recall on this rank's GPU, or None.  It is fed the decode of --detect or --seg-ap (the proposals with --detect-levels):
    without either no decode exists and the option is refused"""
    if not getattr(args, 'prop_recall', False):
        return None
    if not getattr(args, 'detect', None) and not getattr(args, 'seg_ap', False):
        raise ValueError('--prop-recall measures the segments that --detect PATH or --seg-ap decode in the validation phase (with --detect-levels: the '
                         'proposals), and neither is given: there is no decode to measure')
    from cfn_hip.recall import ProposalRecallMeter
    return ProposalRecallMeter(cdist.local_device() if device is None else device, n_classes, [float(x) for x in args.prop_recall_tiou.split(',')],
                               args.prop_recall_n, args.prop_recall_score)


def calibration_from_args(args, n_classes=157, device=None):
    """the Calibration of --detect-calibrate on this RANK's GPU (cfn_hip.dist.local_device: the device run() will make current, where the
    rank's meter lives -- not the current device, which is cuda:0 on every worker in front of run()), or None.  One criterion calibrates the (C,) thr and starts from
    --detect-thr; K > 1 criteria (recall:Q1,Q2,...) calibrate the (C, K) levels, which go through propose like typed levels (so --detect-nms
    applies as it does without), and start from the K values of --detect-levels.  It is made once per `args` and kept there: the writer, the
    meter and run() must share ONE tensor"""
    spec = getattr(args, 'detect_calibrate', None)
    if spec is None:
        return None
    if getattr(args, 'calibration', None) is not None:
        return args.calibration
    from cfn_hip.calibrate import Calibration, parse_criteria
    criteria = parse_criteria(spec)
    if not getattr(args, 'device_ap', False):
        raise ValueError('--detect-calibrate needs --device-ap: the thresholds are calibrated from the AP rows the training phases keep on the GPU')
    levels = detect_levels(args).get('levels')
    if len(criteria) == 1:
        if levels is not None:
            raise ValueError('--detect-calibrate %s gives ONE threshold per class and replaces --detect-thr; --detect-levels asks for proposals at '
                             'several: calibrate them with recall:Q1,Q2,... or drop one of the two' % spec)
        initial = args.detect_thr
    else:
        if levels is None or len(levels) != len(criteria):
            raise ValueError('--detect-calibrate %s gives %d levels per class, which go through the proposals (candidates at every level, then NMS): '
                             'type the %d --detect-levels they start from' % (spec, len(criteria), len(criteria)))
        initial = levels
    args.calibration = Calibration(criteria, n_classes, cdist.local_device() if device is None else device, initial)
    return args.calibration


def _calibrated(thr, more, calibration):
    """(thr, the proposal keywords) of a writer / meter: the typed ones, or the calibration's device tensors in their place"""
    if calibration is None:
        return thr, more
    if calibration.n_criteria == 1:
        if more.get('levels') is not None:
            raise ValueError('a calibration of ONE criterion replaces --detect-thr, but --detect-levels asks for proposals at several levels: '
                             'calibrate those with recall:Q1,Q2,... or drop one of the two')
        return calibration.thr_vector, more
    return thr, dict(more, levels=calibration.levels)


def detect_writer(args, calibration=None):
    """the writer of the --detect group, or None.  calibration (default: calibration_from_args(args), None without --detect-calibrate): its
    thr_vector (one criterion) or levels take the place of the typed thresholds -- device tensors the writer passes through untouched, so an
    update in place reaches every later decode"""
    if not args.detect:
        return None
    smooth = detect_smooth(args)                # (refuses --detect-calibrate before a calibration is made)
    thr, more = _calibrated(args.detect_thr, detect_levels(args), calibration_from_args(args) if calibration is None else calibration)
    return DetectionWriter(args.detect, thr, args.detect_gap, args.detect_min_len, filter=smooth, **more)


def _spawn(gpus, argv):
    """`-gpu 0,1,2` -> one worker process per GPU (what nn.DataParallel did with threads)."""
    import subprocess
    env = dict(os.environ, CUDA_VISIBLE_DEVICES=gpus, HSA_ENABLE_IPC_MODE_LEGACY='0')
    n = len(gpus.split(','))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', os.environ.get('MASTER_PORT', '29511'),
           os.path.abspath(__file__)] + argv
    return subprocess.call(cmd, env=env)


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('-gpu', default='0', type=str)
    parser.add_argument('--max-steps', type=int, default=None)
    parser.add_argument('--batch-size', type=int, default=BS * BS_UPSCALE)
    parser.add_argument('--device-ap', action='store_true', help='training AP rows and loss totals stay on the GPU')
    parser.add_argument('--fused-loss', action='store_true', help='the detection loss as one forward and one backward HIP kernel')
    parser.add_argument('--jpeg-entropy', choices=('interval', 'sync'), default=None,
                        help='entropy mode of the GPU JPEG decode: sync = parallel inside a frame without restart markers')
    add_detect_args(parser)
    seg_ap_arguments(parser)
    args = parser.parse_args()
    if 'RANK' not in os.environ and len(args.gpu.split(',')) > 1:
        sys.exit(_spawn(args.gpu, ['--batch-size', str(args.batch_size)] +
                        (['--max-steps', str(args.max_steps)] if args.max_steps else []) + (['--device-ap'] if args.device_ap else []) +
                        (['--fused-loss'] if args.fused_loss else []) + (['--jpeg-entropy', args.jpeg_entropy] if args.jpeg_entropy else []) +
                        detect_argv(args) + seg_ap_argv(args) + prop_recall_argv(args)))
    if 'RANK' not in os.environ:
        os.environ['CUDA_VISIBLE_DEVICES'] = args.gpu
    run(batch_size=args.batch_size, max_steps=args.max_steps, device_ap=args.device_ap, fused_loss=args.fused_loss, jpeg_entropy=args.jpeg_entropy,
        detections=detect_writer(args), segment_ap=seg_ap_from_args(args), calibration=calibration_from_args(args),
        proposal_recall=prop_recall_from_args(args))
