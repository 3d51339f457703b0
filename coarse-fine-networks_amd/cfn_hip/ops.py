"""torch.autograd glue over the C ABI: each Function allocates outputs with torch (device memory,
caching allocator, current stream) and hands raw pointers to libcfn_hip.so.  No op here has a CPU
or eager fallback.

Convention shared by the conv ops: the input is read through the per-(n,c) *prologue*
``a = act(A*x + B)`` (A, B: fp32 (N,C) or None) and the op returns the raw conv output ``y``
together with fp64 per-(n,c) ``sum(y)`` / ``sum(y*y)``.  Batch-norm statistics, the SE squeeze and
their gradients are then tiny (N,C) tensor expressions handled by ordinary autograd, while every
full-size tensor is touched only inside the HIP kernels.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import ctypes
import os
import threading

from . import call, call_try, check, query, last_error, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_SIGMOID  # noqa: F401


_scratch_epoch = [0]


class _ZeroArena(object):
    """fp64 zero-filled scratch handed out in slices: the statistics / gradient accumulators of ~400 kernel
    launches per step come out of a few large memsets instead of one tiny fill kernel each.  A chunk stays alive
    as long as any slice of it does (autograd may save them)."""
    CHUNK = 1 << 20

    def __init__(self):
        self.buf, self.off, self.epoch = {}, {}, _scratch_epoch[0]

    def take(self, numel, dev):
        if self.epoch != _scratch_epoch[0]:      # reset_scratch() was called (from any thread): drop the old chunks
            self.buf, self.off, self.epoch = {}, {}, _scratch_epoch[0]
        numel_al = (numel + 1) & ~1
        key = (dev.type, dev.index)
        if key not in self.buf or self.off[key] + numel_al > self.buf[key].numel():
            self.buf[key] = torch.zeros(max(self.CHUNK, numel_al), dtype=torch.float64, device=dev)
            self.off[key] = 0
        o = self.off[key]
        self.off[key] = o + numel_al
        return self.buf[key][o:o + numel]


class _GradCast(object):
    """fp64 weight-gradient accumulators -> fp32 gradients with ONE cast kernel per backward pass.

    The wgrad kernels accumulate into fp64 (zero-filled) buffers.  Casting each of the ~110 buffers on its own costs a
    ~6 us kernel apiece, so the accumulators of one backward pass are carved out of one fp64 chunk that is mirrored
    by an fp32 chunk of the same layout; backward returns views of the fp32 chunk and a callback queued on the
    autograd engine fills it with a single copy when the pass ends.

    A view is only handed out when nobody can read the gradient before that copy (`_gw_buffers`): leaf parameter
    without an existing .grad, no create_graph, no tensor hooks, no post-accumulate hooks other than GradReducer's (which
    flushes before it packs a bucket), and the FIRST gradient of that parameter in the running pass (a parameter used
    twice in one graph would have its two unfilled views summed by autograd mid-pass).  State is per (thread, backward
    pass): a pass that died with an exception cannot leave `scheduled` set, because the next pass is recognised by its
    graph-task id and starts from scratch."""

    def __init__(self):
        self._reset()
        self.last_total = 0

    def _reset(self):
        self.cur, self.live, self.scheduled, self.seen, self.task = {}, [], False, set(), None

    def begin(self):
        """called before every hand-out: a new autograd graph task means a new pass"""
        tid = torch._C._current_graph_task_id()
        if tid != self.task:
            if self.live:      # the previous pass never reached its end-of-backward callback (exception): make what it
                self.flush()   # handed out valid, then forget it
            self._reset()
            self.task = tid

    def first_use(self, w):
        if id(w) in self.seen:
            return False
        self.seen.add(id(w))
        return True

    def take(self, numel, shape, dev):
        al = (numel + 3) & ~3
        key = (dev.type, dev.index)
        ch = self.cur.get(key)
        if ch is None or ch['off'] + al > ch['f64'].numel():
            size = max(int(self.last_total * 1.05) + 1024, al, 1 << 16)
            ch = {'f64': torch.zeros(size, dtype=torch.float64, device=dev),
                  'f32': torch.empty(size, dtype=torch.float32, device=dev), 'off': 0, 'done': 0}
            self.cur[key] = ch
            self.live.append(ch)
        o = ch['off']
        ch['off'] = o + al
        if not self.scheduled:
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)
            self.scheduled = True
        return ch['f64'][o:o + numel], ch['f32'][o:o + numel].view(shape)

    def flush(self):
        for ch in self.live:
            if ch['off'] > ch['done']:
                ch['f32'][ch['done']:ch['off']].copy_(ch['f64'][ch['done']:ch['off']])
                ch['done'] = ch['off']

    def _end_of_backward(self):
        self.flush()
        self.last_total = max(sum(ch['off'] for ch in self.live), 1)
        # the fp32 chunk now belongs to the gradients that view it; the next pass gets fresh chunks
        self._reset()


class _PerThread(threading.local):
    """scratch state is per calling thread (the reference's DataParallel drives one thread per device; the autograd
    engine runs backward on per-device worker threads) and, inside it, per device"""

    def __init__(self):
        self.arena = _ZeroArena()
        self.gradcast = _GradCast()


_tls = _PerThread()
LAZY_GRAD_CAST = True     # set False to cast every weight gradient immediately (one small kernel each)


def _f64(n, c, dev):
    return _tls.arena.take(n * c, dev).view(n, c)


def _f64pair(n, c, dev):
    """two adjacent (n,c) accumulators, returned together so one cast converts both"""
    t = _tls.arena.take(2 * n * c, dev).view(2, n, c)
    return t, t[0], t[1]


def reset_scratch():
    """forget the zero-filled scratch chunks of EVERY thread (forward runs on the caller's thread, backward on the autograd
    engine's per-device threads): the next accumulator allocates a fresh, zeroed chunk.  hipGraph capture brackets itself
    with this: a chunk zeroed before the capture would not be re-zeroed at replay, and a chunk that lives in the graph's
    memory pool must not serve eager calls afterwards."""
    _scratch_epoch[0] += 1


def flush_grad_casts():
    """make every weight gradient handed out so far in the running backward pass valid (see _GradCast)"""
    _tls.gradcast.flush()


def allow_lazy_grad_cast(params, ok=True):
    """Opt parameters in to the lazily cast weight gradients (_GradCast): their gradient may be handed to autograd as a view
    that is filled at the end of the backward pass.  ONLY for parameters whose every reader inside the pass calls
    flush_grad_casts() first -- cfn_hip.dist.GradReducer does and opts its parameters in.  Anything else (torch DDP / FSDP
    reducers and other hooks on the AccumulateGrad node, which cannot be detected from here) keeps the default: an immediate
    cast, one small kernel per weight gradient."""
    for p in params:
        p._cfn_lazy_grad_ok = bool(ok)


def _lazy_ok(w):
    if not LAZY_GRAD_CAST or w is None or not w.is_leaf or w.grad is not None or torch.is_grad_enabled():
        return False
    if not getattr(w, '_cfn_lazy_grad_ok', False):
        return False      # not opted in (allow_lazy_grad_cast): somebody unseen (DDP / FSDP node hooks) might read it early
    if w._backward_hooks:
        return False
    hooks = getattr(w, '_post_accumulate_grad_hooks', None)
    if hooks:
        from .dist import _BucketHook
        if not all(isinstance(h, _BucketHook) for h in hooks.values()):
            return False  # a foreign post-accumulate hook (optimizer-in-backward ...) would read the gradient before the flush
    return True


def _lazy_ok_probe(w):
    """_lazy_ok as the backward pass would see it (grad mode off); for tests"""
    with torch.no_grad():
        return _lazy_ok(w)


def _grad_owner(w):
    """the leaf parameter whose .grad receives w's gradient without a kernel in between: w itself, or -- for a pure reshape of a whole
    parameter, `conv1d.weight.view(O, I, 1, 1, 1)` of the fusion modules (x3d_coarse._w5), `fc2.weight.view(...)` of the head -- the
    parameter behind the view (ViewBackward only reshapes the gradient).  The lazy-cast rules are the owner's."""
    if w is not None and not w.is_leaf and w._is_view():
        base = w._base
        if base is not None and base.is_leaf and base.numel() == w.numel() and w.is_contiguous() and base.is_contiguous():
            return base
    return w


def _gw_buffers(w, rows, cols, dev):
    """(fp64 accumulator (rows, cols), finish() -> fp32 gradient shaped like w)"""
    gc = _tls.gradcast
    owner = _grad_owner(w)
    if _lazy_ok(owner):
        gc.begin()
        if gc.first_use(owner):
            g64, g32 = gc.take(rows * cols, tuple(w.shape), dev)
            return g64.view(rows, cols), (lambda: g32)
        # second gradient of the same parameter in this pass: autograd is about to ADD it to the view handed out for the
        # first one -- fill that view now (its accumulation was enqueued before this call), and cast this one eagerly
        gc.flush()
    g64 = _f64(rows, cols, dev)
    return g64, (lambda: g64.float().view(tuple(w.shape)))


def _opt(t):
    return None if t is None else t.contiguous()


def _coef(t, rows=None, cols=None):
    """prologue coefficients (N,C): the ABI takes fp64 (bn_fold emits fp64; hand-made fp32 ones are widened here).  rows / cols: the (N, C)
    the kernel will index -- the C ABI sees a pointer only, so a coefficient tensor of another size is refused here instead of being read
    out of bounds on the device"""
    if t is None:
        return None
    if rows is not None and t.numel() != rows * cols:
        raise RuntimeError('per-sample coefficients of %d x %d channels expected, got a tensor of shape %s' % (rows, cols, tuple(t.shape)))
    return t.to(torch.float64).contiguous()


class ShortcutToken(object):
    """Couples the two pointwise convs that read a stage-first block's input (conv1, stride 1, and the spatially
    strided shortcut conv, x3d_fine.py:284-287) in the backward pass: the shortcut conv, whose backward runs first, leaves
    its data gradient as a COMPACT tensor at output resolution here instead of a zero-filled sparse one, and conv1's
    data-gradient kernel adds it on the stride lattice before its act' epilogue (the dense add between the two
    gradients and the memset disappear).  If conv1's backward happens to run first the plain path is used."""

    def __init__(self):
        self.acc, self.acc_stride, self.main_done = None, 1, False


class TailLink(object):
    """Couples a block tail (bn_add_relu) with the pointwise conv(s) whose raw outputs it consumes (conv3 as `y`, the
    strided shortcut conv as `res`).  With a link the tail's backward writes ONE tensor g = (gout [+ gout2]) * relu' and
    hands it out as the gradient of both inputs; the per-(n,c) factors A (for y) and Ar (for res) that turn it into the
    true gradients are left here and applied by the convs' backward kernels when they load it (`gscale`).  The gradient
    tensors of y / res are therefore only meaningful to those convs -- which is why the link must be given to both
    sides."""

    def __init__(self):
        self.y_scale = self.res_scale = None
        self.done = False


def _bf(t):
    """2-byte activation tensor (bf16 or fp16: the *_bf16 / *_f16 entry points)"""
    return t is not None and t.dtype in (torch.bfloat16, torch.float16)


def subsample_hw(x, s):
    """x[..., ::s, ::s] of a bf16 (N,C,T,H,W) tensor (cfn_subsample_hw_bf16); no autograd (used inside the conv ops)"""
    N, C, T, H, W = x.shape
    out = torch.empty(N, C, T, (H - 1) // s + 1, (W - 1) // s + 1, dtype=x.dtype, device=x.device)
    call('cfn_subsample_hw' + _sfx(x), x, out, N * C * T, H, W, s)
    return out


class _PwConv(Function):
    """1x1x1 conv (optionally spatial stride 2); fp32 MFMA for fp32 tensors (cfn_pwconv_*), bf16 MFMA with fp32 accumulation
    for bf16 tensors (cfn_pwconv_*_bf16: a strided conv is a gather + the stride-1 contraction on the compact tensor)."""

    @staticmethod
    def forward(ctx, x, A, B, w, act, stride, want_stats, token, role, tail=None, tail_role=None):
        x = check(x).contiguous()
        N, Cin, T, H, W = x.shape
        Cout = w.shape[0]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        y = torch.empty(N, Cout, T, Ho, Wo, dtype=x.dtype, device=x.device)
        s = q = None
        if want_stats:
            s, q = _f64(N, Cout, x.device), _f64(N, Cout, x.device)
        w2 = w.reshape(Cout, Cin).contiguous()
        A, B = _coef(A, N, Cin), _coef(B, N, Cin)
        xs = None
        if _bf(x):
            xs = subsample_hw(x, stride) if stride > 1 else x
            call('cfn_pwconv_fwd' + _sfx(x), xs, A, B, act, w2, y, s, q, N, Cin, Cout, T * Ho * Wo)
        else:
            call('cfn_pwconv_fwd', x, A, B, act, w2, y, s, q, N, Cin, Cout, T, H, W, stride)
        ctx.save_for_backward(x, A, B, w2, y, xs if stride > 1 else None)
        ctx.meta = (act, stride, tuple(w.shape))
        ctx.wparam = w
        ctx.token, ctx.role = token, role
        ctx.tail, ctx.tail_role = tail, tail_role
        if not want_stats:
            return y, None, None
        return y, s, q

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs, gq):
        x, A, B, w2, y, xs = ctx.saved_tensors
        act, stride, wshape = ctx.meta
        token, role = ctx.token, ctx.role
        N, Cin, T, H, W = x.shape
        Cout = w2.shape[0]
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        gs, gq = _opt(gs), _opt(gq)
        gsc = None   # gy of a linked block tail is unscaled: the kernels apply the tail's per-(n,c) factor on load
        if ctx.tail is not None and ctx.tail.done:
            gsc = ctx.tail.y_scale if ctx.tail_role == 'y' else ctx.tail.res_scale
        if _bf(x):
            return _PwConv._backward_bf16(ctx, gy, gs, gq, gsc)
        gx = gA = gB = gw = None
        g64 = fin = None
        fused = False
        if ctx.needs_input_grad[0] or (A is not None and ctx.needs_input_grad[1]):
            if token is not None and role == 'short' and stride > 1 and not token.main_done:
                # compact W^T g' at output resolution (a stride-1 data gradient over the strided grid, no epilogue);
                # conv1's data gradient consumes it
                Ho, Wo = y.shape[3], y.shape[4]
                da = torch.empty(N, Cin, T, Ho, Wo, dtype=torch.float32, device=x.device)
                # stride 2 and a weight gradient wanted: both products in one pass over gy, y and the lattice of x
                # (csrc/pwshort.hip; CFN_PW_SHORT=0, read per call, declines it)
                if ctx.needs_input_grad[3]:
                    g64, fin = _gw_buffers(ctx.wparam, Cout, Cin, x.device)
                    fused = call_try('cfn_pwconv_short_bwd', gy, y, gs, gq, gsc, w2, x, A, B, act, da, g64, N, Cin, Cout, T, H, W,
                                     stride)
                if not fused:
                    call('cfn_pwconv_bwd_data_acc', gy, y, gs, gq, w2, None, None, None, ACT_NONE, da, None, None, N, Cin, Cout, T,
                         Ho, Wo, 1, None, 1, gsc)
                token.acc, token.acc_stride = da, stride
            else:
                gx = torch.zeros_like(x) if stride != 1 else torch.empty_like(x)
                ab = a64 = b64 = None
                if A is not None:
                    ab, a64, b64 = _f64pair(N, Cin, x.device)
                acc, acc_stride = None, 1
                if token is not None and role == 'main':
                    if token.acc is not None:
                        acc, acc_stride, token.acc = token.acc, token.acc_stride, None
                    else:
                        token.main_done = True
                # few channels (layer 1: HBM bound): data and weight gradient in one pass over gy, y, x
                if stride == 1 and ctx.needs_input_grad[3]:
                    g64, fin = _gw_buffers(ctx.wparam, Cout, Cin, x.device)
                    fused = call_try('cfn_pwconv_bwd_fused', gy, y, gs, gq, w2, x, A, B, act, gx, a64, b64, g64, N, Cin, Cout,
                                     T, H, W, acc, acc_stride, gsc)
                if not fused:
                    call('cfn_pwconv_bwd_data_acc', gy, y, gs, gq, w2, x, A, B, act, gx, a64, b64, N, Cin, Cout, T, H, W, stride,
                         acc, acc_stride, gsc)
                if A is not None:
                    gA, gB = ab[0], ab[1]
        if ctx.needs_input_grad[3]:
            if g64 is None:
                g64, fin = _gw_buffers(ctx.wparam, Cout, Cin, x.device)
            if not fused:
                call('cfn_pwconv_bwd_weight', gy, y, gs, gq, x, A, B, act, g64, N, Cin, Cout, T, H, W, stride, gsc)
            gw = fin()
        return gx, gA, gB, gw, None, None, None, None, None, None, None

    @staticmethod
    def _backward_bf16(ctx, gy, gs, gq, gsc):
        """bf16 tensors: data gradient and weight gradient as two bf16-MFMA kernels; a strided conv works on the compact
        (subsampled) input saved by the forward"""
        x, A, B, w2, y, xs = ctx.saved_tensors
        act, stride, wshape = ctx.meta
        token, role = ctx.token, ctx.role
        N, Cin, T, H, W = x.shape
        Cout = w2.shape[0]
        Ho, Wo = y.shape[3], y.shape[4]
        xin = xs if stride > 1 else x
        gx = gA = gB = gw = None
        if ctx.needs_input_grad[0] or (A is not None and ctx.needs_input_grad[1]):
            if token is not None and role == 'short' and stride > 1 and not token.main_done:
                da = torch.empty(N, Cin, T, Ho, Wo, dtype=x.dtype, device=x.device)      # compact, no epilogue
                call('cfn_pwconv_bwd_data' + _sfx(gy), gy, y, gs, gq, w2, None, None, None, ACT_NONE, da, None, None, N, Cin, Cout, T,
                     Ho, Wo, None, 1, gsc)
                token.acc, token.acc_stride = da, stride
            else:
                ab = a64 = b64 = None
                if A is not None:
                    ab, a64, b64 = _f64pair(N, Cin, x.device)
                acc, acc_stride = None, 1
                if token is not None and role == 'main':
                    if token.acc is not None:
                        acc, acc_stride, token.acc = token.acc, token.acc_stride, None
                    else:
                        token.main_done = True
                gxc = torch.empty_like(xin)
                call('cfn_pwconv_bwd_data' + _sfx(gy), gy, y, gs, gq, w2, xin, A, B, act, gxc, a64, b64, N, Cin, Cout, T, Ho, Wo,
                     acc, acc_stride, gsc)
                if stride > 1:      # only reached when conv1's backward ran before the shortcut's: scatter onto the lattice
                    gx = torch.zeros_like(x)
                    gx[:, :, :, ::stride, ::stride] = gxc
                else:
                    gx = gxc
                if A is not None:
                    gA, gB = ab[0], ab[1]
        if ctx.needs_input_grad[3]:
            g64, fin = _gw_buffers(ctx.wparam, Cout, Cin, x.device)
            call('cfn_pwconv_bwd_weight' + _sfx(gy), gy, y, gs, gq, xin, A, B, act, g64, N, Cin, Cout, T * Ho * Wo, gsc)
            gw = fin()
        return gx, gA, gB, gw, None, None, None, None, None, None, None


def pwconv(x, w, A=None, B=None, act=ACT_NONE, stride=1, stats=True, token=None, role=None, tail=None, tail_role=None):
    """returns (y, sum, sumsq); sum/sumsq are None when stats=False.  token / role ('main' | 'short'): see ShortcutToken;
    tail / tail_role ('y' | 'res'): see TailLink.

    The kernels address one sample's (channels x positions) block through a 32-bit buffer descriptor (2 GiB fp32, 1 GiB
    bf16).  Whole-video validation exceeds that (x3d_coarse layer 1 on a 1000-frame chunk, train_coarse_fineFEAT.py:215-224:
    54 x 1000 x 112 x 112 x 4 B = 2.7 GB): without autograd the conv then runs over frame ranges -- a 1x1x1 conv is
    per-frame -- and the statistics add up.  With autograd the kernel's refusal stands."""
    N, Cin, T, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    es = x.element_size()
    lim = (1 << 31) if es == 4 else (1 << 30)
    span = max(Cin * H * W, w.shape[0] * H * W, w.shape[0] * Ho * Wo, Cin * Ho * Wo) * es     # pw_plan range-checks M * Pin too
    needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w, A, B))
    if span * T < lim or needs_grad or T == 1:
        return _PwConv.apply(x, A, B, w, act, stride, stats, token, role, tail, tail_role)
    step = max((lim - 1) // span, 1)
    odd_plane = es == 2 and (Ho * Wo) % 2 == 1       # bf16 kernels need an even position count: even frame counts then
    if odd_plane:
        if 2 * span >= lim:
            raise RuntimeError('pwconv: two frames of %d x %d x %d bf16 elements exceed the 1 GiB buffer range the frame-range '
                               'chunking has to respect (odd plane: frames travel in pairs)' % (max(Cin, w.shape[0]), H, W))
        step = max(step & ~1, 2)
    y = torch.empty(N, w.shape[0], T, Ho, Wo, dtype=x.dtype, device=x.device)
    s = q = None
    t0 = 0
    while t0 < T:
        t1 = min(t0 + step, T)
        if odd_plane and (t1 - t0) % 2 and t1 - t0 > 1:
            t1 -= 1                               # keep the chunk even; a single odd frame is left for the end
        pad = odd_plane and (t1 - t0) % 2 == 1     # T itself odd: the last frame travels with a pad frame (its output, act(B), is sliced off below and the statistics are recomputed)
        xc = x[:, :, t0:t1].contiguous()
        if pad:
            xc = torch.cat([xc, torch.zeros_like(xc)], 2)
        yc, sc, qc = _PwConv.apply(xc, A, B, w, act, stride, False if pad else stats, None, None)
        if pad:
            yc = yc[:, :, :1]
            if stats:
                sc, qc = yc.double().sum((2, 3, 4)), (yc.double() ** 2).sum((2, 3, 4))
        y[:, :, t0:t1] = yc
        if stats:
            s, q = (sc, qc) if s is None else (s + sc, q + qc)
        t0 = t1
    return y, s, q


def pwconv_route(op, N, Cin, Cout, T, H, W, stride=1, act=ACT_NONE, flags=0):
    """the kernel a pointwise conv of this shape runs on (cfn_pwconv_route, include/cfn_hip.h): host only, no GPU needed"""
    out = ctypes.create_string_buffer(256)
    if query('cfn_pwconv_route', op, N, Cin, Cout, T, H, W, stride, act, flags, out, 256):
        raise RuntimeError(last_error())
    return out.value.decode()


def dwconv3d_route(op, dtype, N, C, T, H, W, stride=1, act=ACT_NONE, flags=0):
    """the kernel a depthwise 3x3x3 conv of this shape runs on (cfn_dwconv3d_route, include/cfn_hip.h): host only, no GPU needed.
    op 0 forward, 1 data gradient, 2 weight gradient, 3 one-pass backward; dtype 0 fp32, 1 bf16, 2 fp16; H, W: the input plane"""
    out = ctypes.create_string_buffer(256)
    if query('cfn_dwconv3d_route', op, dtype, N, C, T, H, W, stride, act, flags, out, 256):
        raise RuntimeError(last_error())
    return out.value.decode()


def _sfx(t):
    """entry-point suffix for the element type of an activation tensor"""
    return '_bf16' if t.dtype == torch.bfloat16 else ('_f16' if t.dtype == torch.float16 else '')


class _DwConv3d(Function):
    """depthwise 3x3x3, pad 1, stride (1,s,s); see cfn_dwconv3d_*."""

    @staticmethod
    def forward(ctx, x, A, B, w, act, stride, want_stats):
        x = check(x).contiguous()
        N, C, T, H, W = x.shape
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        y = torch.empty(N, C, T, Ho, Wo, dtype=x.dtype, device=x.device)
        s = q = None
        if want_stats:
            s, q = _f64(N, C, x.device), _f64(N, C, x.device)
        w2 = w.reshape(C, 27).contiguous()
        A, B = _coef(A, N, C), _coef(B, N, C)
        call('cfn_dwconv3d_fwd' + _sfx(x), x, A, B, act, w2, y, s, q, N, C, T, H, W, stride)
        ctx.save_for_backward(x, A, B, w2, y)
        ctx.meta = (act, stride, tuple(w.shape))
        ctx.wparam = w
        if not want_stats:
            return y, None, None
        return y, s, q

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs, gq):
        x, A, B, w2, y = ctx.saved_tensors
        act, stride, wshape = ctx.meta
        N, C, T, H, W = x.shape
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        gs, gq = _opt(gs), _opt(gq)
        gx = gA = gB = gw = None
        want_x = ctx.needs_input_grad[0] or (A is not None and ctx.needs_input_grad[1])
        want_w = ctx.needs_input_grad[3]
        ab = a64 = b64 = g64 = fin = None
        if want_x:
            gx = torch.empty_like(x)
            if A is not None:
                ab, a64, b64 = _f64pair(N, C, x.device)
        if want_w:
            g64, fin = _gw_buffers(ctx.wparam, C, 27, x.device)
        # stride 1, big planes: data and weight gradient in ONE pass over gy, y, x (declines small planes)
        sfx = _sfx(x)
        fused = want_x and want_w and stride == 1 and call_try('cfn_dwconv3d_bwd_fused' + sfx, gy, y, gs, gq, w2, x, A, B, act,
                                                             gx, a64, b64, g64, N, C, T, H, W)
        # stride 2 (first block of a stage): x read once instead of twice (declines other geometries)
        if not fused and want_x and want_w and stride == 2:
            fused = call_try('cfn_dwconv3d_bwd_fused_s2' + sfx, gy, y, gs, gq, w2, x, A, B, act, gx, a64, b64, g64, N, C, T, H, W)
        if not fused:
            if want_x:
                call('cfn_dwconv3d_bwd_data' + sfx, gy, y, gs, gq, w2, x, A, B, act, gx, a64, b64, N, C, T, H, W, stride)
            if want_w:
                call('cfn_dwconv3d_bwd_weight' + sfx, gy, y, gs, gq, x, A, B, act, g64, N, C, T, H, W, stride)
        if want_x and A is not None:
            gA, gB = ab[0], ab[1]
        if want_w:
            gw = fin()
        return gx, gA, gB, gw, None, None, None


def dwconv3d(x, w, A=None, B=None, act=ACT_NONE, stride=1, stats=True):
    return _DwConv3d.apply(x, A, B, w, act, stride, stats)


class _DwConvT5(Function):
    """depthwise 5x1x1 temporal conv of the stem; see cfn_dwconv_t5_*."""

    @staticmethod
    def forward(ctx, x, w, want_stats, out_dtype=None):
        x = check(x, torch.float32).contiguous()       # the stem conv's output stays fp32 in both precisions
        N, C, T, H, W = x.shape
        y = torch.empty_like(x, dtype=out_dtype or x.dtype)
        s = q = None
        if want_stats:
            s, q = _f64(N, C, x.device), _f64(N, C, x.device)
        w2 = w.reshape(C, 5).contiguous()
        call('cfn_dwconv_t5_fwd' + _sfx(y), x, w2, y, s, q, N, C, T, H * W)
        ctx.save_for_backward(x, w2, y)
        ctx.wshape = tuple(w.shape)
        ctx.wparam = w
        if not want_stats:
            return y, None, None
        return y, s, q

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs, gq):
        x, w2, y = ctx.saved_tensors
        N, C, T, H, W = x.shape
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        gs, gq = _opt(gs), _opt(gq)
        gx = gw = None
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if want_x:
            gx = torch.empty_like(x)
        if want_w:
            g64, fin = _gw_buffers(ctx.wparam, C, 5, x.device)
        # both gradients in one march over gy, y, x (declines planes that are not whole float4s)
        fused = want_x and want_w and call_try('cfn_dwconv_t5_bwd_fused' + _sfx(y), gy, y, gs, gq, w2, x, gx, g64, N, C, T, H * W)
        if not fused:
            if want_x:
                call('cfn_dwconv_t5_bwd_data' + _sfx(y), gy, y, gs, gq, w2, gx, N, C, T, H * W)
            if want_w:
                call('cfn_dwconv_t5_bwd_weight' + _sfx(y), gy, y, gs, gq, x, g64, N, C, T, H * W)
        if want_w:
            gw = fin()
        return gx, gw, None, None


def dwconv_t5(x, w, stats=True, out_dtype=None):
    """out_dtype=torch.bfloat16: the bf16 activation path starts here (fp32 in, bf16 out)"""
    return _DwConvT5.apply(x, w, stats, out_dtype)


class _StemConv(Function):
    """conv1_s: dense 1x3x3 stride (1,2,2) pad (0,1,1); the clip gets no gradient."""

    @staticmethod
    def forward(ctx, x, w):
        x = check(x).contiguous()
        N, Ci, T, H, W = x.shape
        Co = w.shape[0]
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        y = torch.empty(N, Co, T, Ho, Wo, dtype=torch.float32, device=x.device)
        w2 = w.reshape(Co, Ci * 9).contiguous()
        call('cfn_stem_conv_fwd', x, w2, y, N, Ci, Co, T, H, W)
        ctx.save_for_backward(x)
        ctx.wshape = tuple(w.shape)
        ctx.wparam = w
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        N, Ci, T, H, W = x.shape
        Co = ctx.wshape[0]
        gw = None
        if ctx.needs_input_grad[1]:
            g64, fin = _gw_buffers(ctx.wparam, Co, Ci * 9, x.device)
            call('cfn_stem_conv_bwd_weight', gy.contiguous(), x, g64, N, Ci, Co, T, H, W)
            gw = fin()
        return None, gw


def stem_conv(x, w):
    return _StemConv.apply(x, w)


def _stem_pair_switch():
    """CFN_STEM_PAIR, read per call: bit 0 = fused forward, bit 1 = fused backward (default 3; 0 = the four separate kernels)"""
    try:
        return int(os.environ.get('CFN_STEM_PAIR', '3'))
    except ValueError:
        raise RuntimeError('CFN_STEM_PAIR must be an integer (bit 0: forward, bit 1: backward), got %r' % os.environ['CFN_STEM_PAIR'])


class _StemPair(Function):
    """conv1_s -> conv1_t of an fp32 clip with fp32 activations, one kernel each way (csrc/stempair.hip): the forward writes conv1_s's output xs
    and does not read it back, the backward never writes its gradient.  Where an entry point declines (or CFN_STEM_PAIR switches it off)
    the two separate ops' kernels run on the same tensors."""

    @staticmethod
    def forward(ctx, x, w_s, w_t, want_stats, run_frames):
        x = check(x).contiguous()
        if x.dtype != torch.float32:                   # (check() lets 16-bit activations through; the clip of the pair is fp32)
            raise RuntimeError('stem_pair: fp32 clip expected, got %s' % x.dtype)
        N, Ci, T, H, W = x.shape
        Co = w_s.shape[0]
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        xs = torch.empty(N, Co, T, Ho, Wo, dtype=torch.float32, device=x.device)
        y = torch.empty_like(xs)
        s = q = None
        if want_stats:
            s, q = _f64(N, Co, x.device), _f64(N, Co, x.device)
        ws2 = w_s.reshape(Co, Ci * 9).contiguous()
        wt2 = w_t.reshape(Co, 5).contiguous()
        if not (_stem_pair_switch() & 1 and call_try('cfn_stem_pair_fwd', x, ws2, wt2, xs, y, s, q, N, Ci, Co, T, H, W, run_frames)):
            call('cfn_stem_conv_fwd', x, ws2, xs, N, Ci, Co, T, H, W)
            call('cfn_dwconv_t5_fwd', xs, wt2, y, s, q, N, Co, T, Ho * Wo)
        ctx.save_for_backward(x, xs, y, wt2)
        ctx.params = (w_s, w_t)
        ctx.run_frames = run_frames
        if not want_stats:
            return y, None, None
        return y, s, q

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs, gq):
        x, xs, y, wt2 = ctx.saved_tensors
        w_s, w_t = ctx.params
        N, Ci, T, H, W = x.shape
        _, Co, _, Ho, Wo = xs.shape
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        gs, gq = _opt(gs), _opt(gq)
        want_s, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gws = gwt = None
        if want_s and want_t:
            gs64, fin_s = _gw_buffers(w_s, Co, Ci * 9, x.device)
            gt64, fin_t = _gw_buffers(w_t, Co, 5, x.device)
            if not (_stem_pair_switch() & 2 and
                    call_try('cfn_stem_pair_bwd', gy, y, gs, gq, wt2, xs, x, gt64, gs64, N, Ci, Co, T, H, W, ctx.run_frames)):
                gxs = torch.empty_like(xs)
                if not call_try('cfn_dwconv_t5_bwd_fused', gy, y, gs, gq, wt2, xs, gxs, gt64, N, Co, T, Ho * Wo):
                    call('cfn_dwconv_t5_bwd_data', gy, y, gs, gq, wt2, gxs, N, Co, T, Ho * Wo)
                    call('cfn_dwconv_t5_bwd_weight', gy, y, gs, gq, xs, gt64, N, Co, T, Ho * Wo)
                call('cfn_stem_conv_bwd_weight', gxs, x, gs64, N, Ci, Co, T, H, W)
            gws, gwt = fin_s(), fin_t()
        elif want_t:
            gt64, fin_t = _gw_buffers(w_t, Co, 5, x.device)
            call('cfn_dwconv_t5_bwd_weight', gy, y, gs, gq, xs, gt64, N, Co, T, Ho * Wo)
            gwt = fin_t()
        elif want_s:
            gs64, fin_s = _gw_buffers(w_s, Co, Ci * 9, x.device)
            gxs = torch.empty_like(xs)
            call('cfn_dwconv_t5_bwd_data', gy, y, gs, gq, wt2, gxs, N, Co, T, Ho * Wo)
            call('cfn_stem_conv_bwd_weight', gxs, x, gs64, N, Ci, Co, T, H, W)
            gws = fin_s()
        return None, gws, gwt, None, None


def stem_pair(x, w_s, w_t, stats=True, run_frames=0):
    """dwconv_t5(stem_conv(x, w_s), w_t, stats) for an fp32 clip and fp32 activations; run_frames: see cfn_stem_pair_fwd (0 = planned)"""
    return _StemPair.apply(x, w_s, w_t, stats, run_frames)


# ---- uint8 frames: normalised on the GPU (csrc/stem_u8.hip) -------------------------------------------------------------------
from .u8clips import clip_lut  # noqa: E402,F401  (host-built (3, 256) table, the reference's op order)


def _u8_args(frames, lengths, lut):
    """frames (N, T, H, W, 3) uint8, lengths (N) int32 or None, lut (3, 256) fp32: checked here, the C ABI sees pointers only"""
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[4] != 3:
        raise RuntimeError('uint8 frames of shape (N, T, H, W, 3) expected, got %s %s' % (frames.dtype, tuple(frames.shape)))
    if lut.dtype != torch.float32 or lut.numel() != 3 * 256:
        raise RuntimeError('a (3, 256) fp32 table expected (ops.clip_lut), got %s %s' % (lut.dtype, tuple(lut.shape)))
    if lengths is not None:
        if lengths.numel() != frames.shape[0]:
            raise RuntimeError('one length per clip expected: %d clips, lengths %s' % (frames.shape[0], tuple(lengths.shape)))
        lengths = lengths.to(torch.int32).contiguous()
    return frames.contiguous(), lengths, lut.contiguous()


def clip_u8_to_f32(frames, lut, lengths=None):
    """(N, T, H, W, 3) uint8 -> the normalised fp32 clip (N, 3, T, H, W); frames t >= lengths[n] are zero"""
    frames, lengths, lut = _u8_args(frames, lengths, lut)
    N, T, H, W, _ = frames.shape
    x = torch.empty(N, 3, T, H, W, dtype=torch.float32, device=frames.device)
    call('cfn_clip_u8_to_f32', frames, lut, lengths, x, N, T, H, W)
    return x


class _StemConvU8(Function):
    """conv1_s on uint8 frames.  Shapes the fused kernels decline run as convert + the fp32 entry point."""

    @staticmethod
    def forward(ctx, frames, lengths, lut, w):
        frames, lengths, lut = _u8_args(frames, lengths, lut)
        N, T, H, W, Ci = frames.shape
        Co = w.shape[0]
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        y = torch.empty(N, Co, T, Ho, Wo, dtype=torch.float32, device=frames.device)
        w2 = w.reshape(Co, Ci * 9).contiguous()
        if not call_try('cfn_stem_conv_u8_fwd', frames, lut, lengths, w2, y, N, Ci, Co, T, H, W):
            call('cfn_stem_conv_fwd', clip_u8_to_f32(frames, lut, lengths), w2, y, N, Ci, Co, T, H, W)
        ctx.save_for_backward(frames, lengths, lut)
        ctx.wshape = tuple(w.shape)
        ctx.wparam = w
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        frames, lengths, lut = ctx.saved_tensors
        N, T, H, W, Ci = frames.shape
        Co = ctx.wshape[0]
        gw = None
        if ctx.needs_input_grad[3]:
            g64, fin = _gw_buffers(ctx.wparam, Co, Ci * 9, frames.device)
            gy = gy.contiguous()
            if not call_try('cfn_stem_conv_u8_bwd_weight', gy, frames, lut, lengths, g64, N, Ci, Co, T, H, W):
                call('cfn_stem_conv_bwd_weight', gy, clip_u8_to_f32(frames, lut, lengths), g64, N, Ci, Co, T, H, W)
            gw = fin()
        return None, None, None, gw


def stem_conv_u8(frames, lengths, lut, w):
    """stem_conv(clip_u8_to_f32(frames, lut, lengths), w) without the fp32 clip (bit-identical forward)"""
    return _StemConvU8.apply(frames, lengths, lut, w)


# ---- uint8 frames: crop, antialiased bilinear resize and flip on the GPU (csrc/aug_u8.hip; tables: cfn_hip/u8aug.py) -------------
from . import u8aug  # noqa: E402

_AUG_TABLES = {}                 # (crop extents of the batch, S, device) -> (bounds, coef) on the device
_AUG_TABLES_MAX = 256


def aug_tables(box, size, device):
    """device tables (bounds (N, S, 2), coef (N, S, K) int32) of a batch whose crop extents are box[:, 2]; `box` is read on the host
    (a device tensor costs one small copy back and a wait for it).  Cached per (extents, size, device): a dataset has a handful of
    distinct crop extents."""
    cs = tuple(int(v) for v in box.detach().reshape(-1, 4)[:, 2].cpu().tolist())
    device = torch.device(device)
    key = (cs, int(size), device.type, device.index)
    hit = _AUG_TABLES.get(key)
    if hit is None:
        if any(c <= 0 or c > 4 * int(size) for c in cs):
            raise RuntimeError('crop_resize_flip_u8: crop extents %s into %d: 1 <= c <= 4 * size expected (the kernel takes tables of up '
                               'to %d taps; there is no CPU fallback)' % (sorted(set(cs)), size, u8aug.MAX_TAPS))
        bounds, coef = u8aug.batch_tables(cs, size)
        hit = (bounds.to(device), coef.to(device))
        if len(_AUG_TABLES) >= _AUG_TABLES_MAX:
            _AUG_TABLES.clear()
        _AUG_TABLES[key] = hit
    return hit


def crop_resize_flip_u8(frames, lengths, box, size, out=None, tables=None):
    """frames (N, T, Hs, Ws, 3) uint8 on the GPU, box (N, 4) int32 = x1, y1, c, flip per clip -> (N, T, size, size, 3) uint8: the
    reference's PIL crop + resize(BILINEAR) + FLIP_LEFT_RIGHT, bit for bit; frames t >= lengths[n] are zero bytes.
    tables = aug_tables(box, size, device) may be handed in (then `box` is not read on the host: no wait, capturable); with `out`,
    a device `box` and cached or given tables nothing is allocated on the device."""
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[4] != 3:
        raise RuntimeError('uint8 frames of shape (N, T, Hs, Ws, 3) expected, got %s %s' % (frames.dtype, tuple(frames.shape)))
    N, T, Hs, Ws, _ = frames.shape
    S = int(size)
    if box.numel() != 4 * N:
        raise RuntimeError('one box (x1, y1, c, flip) per clip expected: %d clips, box %s' % (N, tuple(box.shape)))
    if lengths is not None:
        if lengths.numel() != N:
            raise RuntimeError('one length per clip expected: %d clips, lengths %s' % (N, tuple(lengths.shape)))
        lengths = lengths.to(torch.int32).contiguous()
    bounds, coef = tables if tables is not None else aug_tables(box, S, frames.device)
    if tuple(bounds.shape) != (N, S, 2) or coef.dim() != 3 or tuple(coef.shape[:2]) != (N, S):
        raise RuntimeError('tables of %d clips into %d expected, got bounds %s coef %s' % (N, S, tuple(bounds.shape), tuple(coef.shape)))
    box = box.reshape(N, 4).to(device=frames.device, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty(N, T, S, S, 3, dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, T, S, S, 3) or not out.is_contiguous():
        raise RuntimeError('out: a contiguous uint8 tensor of shape %s expected, got %s %s' % ((N, T, S, S, 3), out.dtype, tuple(out.shape)))
    if not call_try('cfn_crop_resize_flip_u8', frames.contiguous(), lengths, box, bounds.contiguous(), coef.contiguous(), out, N, T, Hs, Ws,
                    S, int(coef.shape[2])):
        raise RuntimeError('crop_resize_flip_u8: %d taps into size %d is beyond what the kernel was built for (c <= 4 * size, size <= 312 '
                           'at 9 taps); there is no CPU fallback' % (int(coef.shape[2]), S))
    return out


# ---- per-class average precision on the GPU (csrc/apmeter.hip; the meter: apmeter.DeviceAPMeter) -----------------------------------
AP_SORT_TILE = 8192              # rows per tile of cfn_ap_sort (cfn_ap_sort_tile(); tests place sizes on its edges)
AP_FLAG_NONBINARY, AP_FLAG_OVERFLOW = 1, 2


def _ap_stores(scores, targets, count, what):
    for name, x in (('scores', scores), ('targets', targets), ('count', count)):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError('%s: %s must be a device tensor; there is no CPU path' % (what, name))
    if scores.dtype != torch.float32 or scores.dim() != 2 or targets.dtype != torch.uint8 or tuple(targets.shape) != tuple(scores.shape):
        raise RuntimeError('%s: class-major stores expected, scores (K, cap) fp32 and targets (K, cap) uint8; got %s %s, %s %s'
                           % (what, scores.dtype, tuple(scores.shape), targets.dtype, tuple(targets.shape)))
    if count.dtype != torch.int32 or count.numel() != 1:
        raise RuntimeError('%s: count must be one int32 on the device, got %s %s' % (what, count.dtype, tuple(count.shape)))
    if scores.shape[0] < 1 or scores.shape[1] < 1:
        raise RuntimeError('%s: empty stores %s' % (what, tuple(scores.shape)))
    return int(scores.shape[0]), int(scores.shape[1])


def ap_append(probs, labels, valid, scores, targets, count, flags):
    """Append a batch to class-major AP stores, in place, without reading anything back: probs / labels (B, K, TL) fp32 on the device,
    valid (B,) int32 on the device or None (every frame); video b contributes its first min(valid[b], TL) frames, videos in batch
    order (train_fine._ap_rows).  scores (K, cap) fp32, targets (K, cap) uint8, count and flags one int32 each, all on the device.
    A batch that does not fit sets AP_FLAG_OVERFLOW in flags and writes nothing; a label other than 0 / 1 sets AP_FLAG_NONBINARY."""
    K, cap = _ap_stores(scores, targets, count, 'ap_append')
    for name, x in (('probs', probs), ('labels', labels), ('flags', flags)):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError('ap_append: %s must be a device tensor; there is no CPU path' % name)
    if probs.dim() != 3 or probs.shape[1] != K or tuple(labels.shape) != tuple(probs.shape):
        raise RuntimeError('ap_append: probs and labels (B, %d, TL) expected, got %s and %s' % (K, tuple(probs.shape), tuple(labels.shape)))
    if flags.dtype != torch.int32 or flags.numel() != 1:
        raise RuntimeError('ap_append: flags must be one int32 on the device')
    B, _, TL = probs.shape
    if valid is not None:
        if valid.numel() != B:
            raise RuntimeError('ap_append: one valid length per video expected: %d videos, valid %s' % (B, tuple(valid.shape)))
        valid = valid.to(torch.int32).contiguous()
    call('cfn_ap_append', probs.float().contiguous(), labels.float().contiguous(), valid, scores, targets, count, flags, B, K, TL, cap)


def ap_sort(scores, targets, count, out=None):
    """Stable descending sort of rows 0 .. count - 1 of every class: scores (K, cap) fp32, targets (K, cap) uint8, count one int32
    on the device -> (sorted_scores, sorted_targets) of the same shapes; rows behind count are not written.  The sorted scores are
    canonical (+0.0 for -0.0, one NaN pattern for every NaN).  out = (sorted_scores, sorted_targets, tmp_keys int32, tmp_targets):
    buffers to reuse; allocated with torch otherwise."""
    K, cap = _ap_stores(scores, targets, count, 'ap_sort')
    if out is None:
        out = (torch.empty_like(scores), torch.empty_like(targets), torch.empty(K, cap, dtype=torch.int32, device=scores.device),
               torch.empty_like(targets))
    ss, st, tk, tt = out
    for x, ref, dt in ((ss, scores, torch.float32), (st, targets, torch.uint8), (tk, scores, torch.int32), (tt, targets, torch.uint8)):
        if tuple(x.shape) != tuple(ref.shape) or x.dtype != dt or x.device != ref.device:
            raise RuntimeError('ap_sort: out buffers of shape %s (fp32, uint8, int32, uint8) on %s expected' % (tuple(ref.shape), ref.device))
    call('cfn_ap_sort', scores, targets, count, ss, st, tk, tt, K, cap)
    return ss, st


def ap_reduce(sorted_targets, count):
    """(K, cap) uint8 sorted target bytes -> (K,) fp32 AP over the first count rows (a class without a positive: 0)"""
    if not sorted_targets.is_cuda or not count.is_cuda:
        raise RuntimeError('ap_reduce: device tensors only; there is no CPU path')
    if sorted_targets.dtype != torch.uint8 or sorted_targets.dim() != 2 or count.dtype != torch.int32 or count.numel() != 1:
        raise RuntimeError('ap_reduce: sorted targets (K, cap) uint8 and one int32 count expected')
    K, cap = sorted_targets.shape
    ap = torch.empty(K, dtype=torch.float32, device=sorted_targets.device)
    call('cfn_ap_reduce', sorted_targets, count, ap, K, cap)
    return ap


def average_precision(scores, targets, count, out=None):
    """(K,) fp32 per-class AP of the first count rows of class-major stores, on the device: ap_sort + ap_reduce (nothing is read back)"""
    _, st = ap_sort(scores, targets, count, out=out)
    return ap_reduce(st, count)


# ---- merge class-major AP stores (csrc/apmerge.hip; the rule M1-M4, the numpy reference and the gather over ranks: cfn_hip/apmerge.py) ------
AP_FLAG_BAD_SOURCE = 4
AP_MERGE_TILE = 2048             # rows per workgroup of cfn_ap_merge's copy (cfn_ap_merge_tile(); tests place sizes on its edges)


def ap_merge_workspace_bytes(R, C):
    n = int(query('cfn_ap_merge_workspace_bytes', int(R), int(C)))
    if n < 0:
        raise RuntimeError('ap_merge: R and C in [1, 65535] expected, got (%d, %d)' % (R, C))
    return n


def ap_merge(dst_scores, dst_payload, dst_counts, dst_extra, dst_flags, src_scores, src_payload, src_counts, src_extra, src_flags, out=None):
    """Append R source stores behind the rows a destination store holds, in part order, in place (rules M1-M4 of cfn_hip/apmerge.py):
    dst_scores (C, cap_d) fp32, dst_payload (C, cap_d) uint8, dst_counts (n_cnt,) int32 with n_cnt 1 (one count for all classes: the frame
    meter) or C (segment AP), dst_extra (n_extra,) int32 or None (additive integers carried along: n_gt), dst_flags one int32; src_scores
    (R, C, cap_s), src_payload (R, C, cap_s), src_counts (R, n_cnt), src_extra (R, n_extra) or None, src_flags (R,); all contiguous on one
    GPU, sources and destination apart.  All or nothing: a total past cap_d sets AP_FLAG_OVERFLOW, a source count outside [0, cap_s]
    AP_FLAG_BAD_SOURCE, and nothing else changes; the sources' flags are OR-ed in either way.  Two launches, nothing is read back (no
    wait).  out: a uint8 workspace of ap_merge_workspace_bytes(R, C) bytes on an 8-byte boundary (capturable with it).  Returns the
    workspace.  No CPU path (apmerge.merge_reference is the host spelling)."""
    what = 'ap_merge'
    tensors = dict(dst_scores=dst_scores, dst_payload=dst_payload, dst_counts=dst_counts, dst_flags=dst_flags, src_scores=src_scores,
                   src_payload=src_payload, src_counts=src_counts, src_flags=src_flags)
    if (dst_extra is None) != (src_extra is None):
        raise RuntimeError('%s: dst_extra and src_extra: both or neither expected' % what)
    if dst_extra is not None:
        tensors.update(dst_extra=dst_extra, src_extra=src_extra)
    dev = _one_gpu(what, 'cfn_hip.apmerge.merge_reference', **tensors)
    if dst_scores.dtype != torch.float32 or dst_scores.dim() != 2 or min(dst_scores.shape) < 1 or dst_payload.dtype != torch.uint8 \
            or tuple(dst_payload.shape) != tuple(dst_scores.shape):
        raise RuntimeError('%s: destination: class-major stores expected, scores (C, cap_d) fp32 and payload (C, cap_d) uint8; got %s %s, %s %s'
                           % (what, dst_scores.dtype, tuple(dst_scores.shape), dst_payload.dtype, tuple(dst_payload.shape)))
    C, cap_d = int(dst_scores.shape[0]), int(dst_scores.shape[1])
    if src_scores.dtype != torch.float32 or src_scores.dim() != 3 or int(src_scores.shape[1]) != C or min(src_scores.shape) < 1 \
            or src_payload.dtype != torch.uint8 or tuple(src_payload.shape) != tuple(src_scores.shape):
        raise RuntimeError('%s: sources: scores (R, %d, cap_s) fp32 and payload (R, %d, cap_s) uint8 expected; got %s %s, %s %s'
                           % (what, C, C, src_scores.dtype, tuple(src_scores.shape), src_payload.dtype, tuple(src_payload.shape)))
    R, cap_s = int(src_scores.shape[0]), int(src_scores.shape[2])
    n_cnt = int(dst_counts.numel())
    if dst_counts.dtype != torch.int32 or dst_counts.dim() != 1 or n_cnt not in (1, C) or src_counts.dtype != torch.int32 \
            or tuple(src_counts.shape) != (R, n_cnt):
        raise RuntimeError('%s: dst_counts (1,) or (%d,) int32 and src_counts (%d, n_cnt) int32 expected, got %s %s and %s %s'
                           % (what, C, R, dst_counts.dtype, tuple(dst_counts.shape), src_counts.dtype, tuple(src_counts.shape)))
    n_extra = 0
    if dst_extra is not None:
        n_extra = int(dst_extra.numel())
        if dst_extra.dtype != torch.int32 or dst_extra.dim() != 1 or src_extra.dtype != torch.int32 or tuple(src_extra.shape) != (R, n_extra):
            raise RuntimeError('%s: dst_extra (n_extra,) int32 and src_extra (%d, n_extra) int32 expected, got %s %s and %s %s'
                               % (what, R, dst_extra.dtype, tuple(dst_extra.shape), src_extra.dtype, tuple(src_extra.shape)))
        if n_extra == 0:
            dst_extra = src_extra = None
    if dst_flags.dtype != torch.int32 or dst_flags.numel() != 1 or src_flags.dtype != torch.int32 or tuple(src_flags.shape) != (R,):
        raise RuntimeError('%s: dst_flags one int32 and src_flags (%d,) int32 expected, got %s %s and %s %s'
                           % (what, R, dst_flags.dtype, tuple(dst_flags.shape), src_flags.dtype, tuple(src_flags.shape)))
    if not (1 <= R <= 65535 and C <= 65535 and cap_s < (1 << 31) and cap_d < (1 << 31)):
        raise RuntimeError('%s: R and C <= 65535 and capacities < 2^31 expected, got R %d, C %d, cap_s %d, cap_d %d' % (what, R, C, cap_s, cap_d))
    lo, hi = dst_scores.data_ptr(), dst_scores.data_ptr() + 4 * C * cap_d
    plo, phi = dst_payload.data_ptr(), dst_payload.data_ptr() + C * cap_d
    if (src_scores.data_ptr() < hi and lo < src_scores.data_ptr() + 4 * R * C * cap_s) \
            or (src_payload.data_ptr() < phi and plo < src_payload.data_ptr() + R * C * cap_s):
        raise RuntimeError('%s: sources and destination overlap' % what)
    ws_bytes = ap_merge_workspace_bytes(R, C)
    if out is None:
        out = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < ws_bytes or out.data_ptr() % 8 \
            or not out.is_contiguous() or out.device != dev:
        raise RuntimeError('%s: out: an 8-byte aligned uint8 workspace of >= %d bytes on %s expected' % (what, ws_bytes, dev))
    call('cfn_ap_merge', dst_scores, dst_payload, dst_counts, dst_extra, dst_flags, src_scores, src_payload, src_counts, src_extra, src_flags, out,
         R, C, n_cnt, n_extra, cap_s, cap_d)
    return out


# ---- per-class decode thresholds from the sorted AP rows (csrc/apcal.hip; the rule and the Calibration: cfn_hip/calibrate.py) -------------
AP_CALIBRATE_TILE = 8192         # rows per tile of cfn_ap_calibrate's second walk (cfn_ap_calibrate_tile(); tests place sizes on its edges)
AP_CALIBRATE_MAX_K = 16
AP_KIND_F1, AP_KIND_PRECISION, AP_KIND_RECALL = 0, 1, 2


def ap_calibrate(sorted_scores, sorted_targets, count, kinds, values, out=None):
    """Per-class operating points of K criteria over the first count rows of SORTED class-major stores (ap_sort's outputs): sorted_scores
    (C, cap) fp32, sorted_targets (C, cap) uint8, count one int32, kinds (K,) int32 (AP_KIND_*) and values (K,) fp64, 1 <= K <= 16, all on
    the device -> (thr (C, K) fp32, cut (C, K) int32, tp (C, K) int32, ok (C, K) uint8, stat (C, 2) int32 [P, m]); the rule is in
    cfn_hip/calibrate.py (thresholds_reference spells it on the host).  One launch, nothing is read back (no wait, capturable with out=):
    kinds and values are NOT looked at here -- calibrate.criteria_tensors refuses what the rule does not know; on the device an unknown
    kind or a value outside (0, 1] gives cut 0 and ok 0.  out: the five tensors to reuse, contiguous and exactly of these shapes
    (the kernel writes dense (C, K) blocks).  No gradient, no CPU path."""
    C, cap = _ap_stores(sorted_scores, sorted_targets, count, 'ap_calibrate')
    for name, x, dt in (('kinds', kinds, torch.int32), ('values', values, torch.float64)):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError('ap_calibrate: %s must be a device tensor; there is no CPU path' % name)
        if x.dtype != dt or x.dim() != 1 or not x.is_contiguous():
            raise RuntimeError('ap_calibrate: %s: a contiguous (K,) %s tensor expected, got %s %s' % (name, dt, x.dtype, tuple(x.shape)))
    K = int(kinds.shape[0])
    if not 1 <= K <= AP_CALIBRATE_MAX_K or int(values.shape[0]) != K:
        raise RuntimeError('ap_calibrate: kinds and values of one length K in [1, %d] expected, got %d and %d' % (AP_CALIBRATE_MAX_K, K, int(values.shape[0])))
    if C > 65535 or cap >= (1 << 31):
        raise RuntimeError('ap_calibrate: C <= 65535 and cap < 2^31 expected, got stores %s' % ((C, cap),))
    if not (sorted_scores.is_contiguous() and sorted_targets.is_contiguous()):
        raise RuntimeError('ap_calibrate: contiguous class-major stores expected')
    dev = sorted_scores.device
    want = ((K, torch.float32), (K, torch.int32), (K, torch.int32), (K, torch.uint8), (2, torch.int32))
    if out is None:
        out = tuple(torch.empty(C, w, dtype=dt, device=dev) for w, dt in want)
    else:
        out = tuple(out)
        if len(out) != 5 or any(not torch.is_tensor(y) or tuple(y.shape) != (C, w) or y.dtype != dt or y.device != dev or not y.is_contiguous()
                                for y, (w, dt) in zip(out, want)):
            raise RuntimeError('ap_calibrate: out: contiguous thr (%d, %d) fp32, cut and tp (%d, %d) int32, ok (%d, %d) uint8 and stat (%d, 2) int32 on %s '
                               'expected' % (C, K, C, K, C, K, C, dev))
    for name, x in (('count', count), ('kinds', kinds), ('values', values)):
        if x.device != dev:
            raise RuntimeError('ap_calibrate: %s is on %s, the stores on %s' % (name, x.device, dev))
    call('cfn_ap_calibrate', sorted_scores, sorted_targets, count, kinds, values, out[0], out[1], out[2], out[3], out[4], C, K, cap)
    return out


class _BnFold(Function):
    """(sum, sumsq) of a conv output -> per-(n,c) prologue (A, B); optional fused SE gate.  cfn_bn_fold_*."""

    @staticmethod
    def forward(ctx, s, q, gamma, beta, w1, b1, w2, b2, bufs, cfg):
        training, N, C, S, count, eps, momentum, pool_count = cfg
        run_mean, run_var, nbt = bufs
        dev = run_mean.device
        Wd = w1.shape[0] if w1 is not None else 0
        Se = S if training else 1
        A = torch.empty(N, C, dtype=torch.float64, device=dev)   # prologue coefficients travel as fp64 (fp32 values):
        B = torch.empty_like(A)                                    # their gradients are the kernels' fp64 accumulators, uncast
        mean = torch.empty(Se, C, dtype=torch.float64, device=dev)
        rstd = torch.empty_like(mean)
        A0 = B0 = gate = hbuf = pooled = None
        w1c = w2c = None
        if Wd:
            A0, B0, gate, pooled = (torch.empty(N, C, dtype=torch.float32, device=dev) for _ in range(4))
            hbuf = torch.empty(N, Wd, dtype=torch.float32, device=dev)
            w1c, w2c = w1.reshape(Wd, C).contiguous(), w2.reshape(C, Wd).contiguous()
        s, q = _opt(s), _opt(q)
        call('cfn_bn_fold_fwd', s, q, gamma, beta, run_mean, run_var, nbt if training else None, int(training), N, C, S,
             float(count), float(eps), float(momentum), w1c, b1, w2c, b2, Wd, float(pool_count), A, B, mean, rstd,
             A0, B0, gate, hbuf, pooled)
        ctx.save_for_backward(s, gamma, mean, rstd, A0, B0, gate, hbuf, pooled, w1c, w2c)
        ctx.cfg = (training, N, C, S, Wd, count, pool_count, None if w1 is None else tuple(w1.shape),
                   None if w2 is None else tuple(w2.shape))
        return A, B

    @staticmethod
    @once_differentiable
    def backward(ctx, gA, gB):
        s, gamma, mean, rstd, A0, B0, gate, hbuf, pooled, w1c, w2c = ctx.saved_tensors
        training, N, C, S, Wd, count, pool_count, w1s, w2s = ctx.cfg
        dev = mean.device
        gA = torch.zeros(N, C, dtype=torch.float64, device=dev) if gA is None else gA.contiguous()
        gB = torch.zeros(N, C, dtype=torch.float64, device=dev) if gB is None else gB.contiguous()
        gs = gq = None
        if training:
            gs = torch.empty(N, C, dtype=torch.float64, device=dev)
            gq = torch.empty_like(gs)
        elif Wd:     # eval mode: the statistics are constants, but the SE gate still depends on sum(y) (x3d_fine.py:158)
            gs = torch.empty(N, C, dtype=torch.float64, device=dev)
        gg = gbt = None
        if gamma is not None:
            gg, gbt = torch.empty(C, device=dev), torch.empty(C, device=dev)
        gw1 = gb1 = gw2 = gb2 = tA = tB = None
        if Wd:
            gw1, gb1 = torch.empty(Wd, C, device=dev), torch.empty(Wd, device=dev)
            gw2, gb2 = torch.empty(C, Wd, device=dev), torch.empty(C, device=dev)
            tA, tB = (torch.empty(N, C, dtype=torch.float64, device=dev) for _ in range(2))
        call('cfn_bn_fold_bwd', gA, gB, s, gamma, mean, rstd, A0, B0, gate, hbuf, pooled, w1c, w2c, int(training), N, C, S,
             Wd, float(count), float(pool_count), gs, gq, gg, gbt, gw1, gb1, gw2, gb2, tA, tB)
        if Wd:
            gw1, gw2 = gw1.view(w1s), gw2.view(w2s)
        return gs, gq, gg, gbt, gw1, gb1, gw2, gb2, None, None


def bn_fold(s, q, gamma, beta, bufs, training, N, C, S, count, eps, momentum, se=None, pool_count=1.0):
    """bufs = (running_mean, running_var, num_batches_tracked) of split_bn (training) or bn (eval);
    se = (fc1.weight, fc1.bias, fc2.weight, fc2.bias) or None."""
    w1, b1, w2, b2 = se if se is not None else (None, None, None, None)
    return _BnFold.apply(s, q, gamma, beta, w1, b1, w2, b2, bufs, (training, N, C, S, count, eps, momentum, pool_count))


class _BnAddRelu(Function):
    """out = relu(A*y + B + (Ar*res + Br)); Ar/Br None = plain residual.

    split=True returns the output twice (two tensor objects over one storage): the caller hands one to the next
    block's conv1 and the other to its residual input, so autograd delivers their gradients separately and the backward
    kernel sums them on the fly instead of a 3-pass add kernel in between.  Nothing may write to either in place."""

    @staticmethod
    def forward(ctx, y, A, B, res, Ar, Br, split, link):
        y, res = check(y).contiguous(), check(res).contiguous()
        N, C = y.shape[:2]
        vol = y[0, 0].numel()
        if tuple(res.shape) != tuple(y.shape):
            raise RuntimeError('bn_add_relu: residual %s does not match y %s' % (tuple(res.shape), tuple(y.shape)))
        out = torch.empty_like(y)
        A, B, Ar, Br = _coef(A, N, C), _coef(B, N, C), _coef(Ar, N, C), _coef(Br, N, C)
        mask = None
        sfx = _sfx(y)
        if link is not None:   # ReLU bit mask for the one-tensor backward (1/32 of a tensor instead of re-reading out)
            words = query('cfn_bn_add_relu_mask_words' + sfx, N * C, vol)
            # (the mask comes from the vector kernels only: a contiguous view that does not start on a 16-byte boundary takes the scalar route,
            # whose entry point refuses a mask -- the backward then reads `out`)
            if words > 0 and all(t.data_ptr() % 16 == 0 for t in (y, res, out)):
                mask = torch.empty(words, dtype=torch.int32, device=y.device)
        call('cfn_bn_add_relu_fwd' + sfx, y, A, B, res, Ar, Br, out, mask, N * C, vol)
        ctx.link, ctx.has_mask = link, mask is not None
        ctx.save_for_backward(y, A, res, Ar, mask if mask is not None else out)
        if not split:
            return out
        alias = torch.empty(0, dtype=out.dtype, device=out.device).set_(out.untyped_storage(), out.storage_offset(),
                                                                         out.shape, out.stride())
        return out, alias

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, gout2=None):
        y, A, res, Ar, out = ctx.saved_tensors
        N, C = y.shape[:2]
        vol = y[0, 0].numel()
        if gout is None:
            gout, gout2 = gout2, None
        if gout is None:
            gout = torch.zeros_like(y)
        gout2 = None if gout2 is None else gout2.contiguous()
        t3 = _tls.arena.take(3 * N * C, y.device).view(3, N, C)
        gA, gB = t3[0], t3[1]
        gAr = t3[2] if Ar is not None else None
        gBr = gB if Ar is not None else None
        link = ctx.link
        if link is not None:
            g = torch.empty_like(y)
            mask = out if ctx.has_mask else None
            call('cfn_bn_add_relu_bwd_g' + _sfx(y), gout.contiguous(), gout2, None if ctx.has_mask else out, mask, y,
                 res if Ar is not None else None, g, gA, gB, gAr, N * C, vol)
            # DETACHED: A / Ar come back from saved_tensors with their grad_fn, and that graph contains the conv whose ctx holds this link -- a
            # reference cycle through C++ autograd nodes that Python's collector cannot break (it leaked the ctx objects, the link and the (N, C)
            # factors of every block: ~190 KB per step at 8 clips)
            link.y_scale, link.res_scale, link.done = A.detach(), (None if Ar is None else Ar.detach()), True
            # one tensor, two consumers: a second tensor object over the same storage keeps autograd from accumulating
            # into it in place
            g2 = torch.empty(0, dtype=g.dtype, device=g.device).set_(g.untyped_storage(), g.storage_offset(), g.shape, g.stride())
            return g, gA, gB, g2, gAr, gBr, None, None
        if _bf(y):   # no link (a tail used on its own): one-tensor kernel, then the two per-(n,c) scalings as tensor ops
            g = torch.empty_like(y)
            call('cfn_bn_add_relu_bwd_g' + _sfx(y), gout.contiguous(), gout2, out, None, y, res if Ar is not None else None, g, gA, gB,
                 gAr, N * C, vol)
            shp = (N, C) + (1,) * (y.dim() - 2)
            gres = g if Ar is None else (g.float() * Ar.float().view(shp)).to(y.dtype)
            return (g.float() * A.float().view(shp)).to(y.dtype), gA, gB, gres, gAr, gBr, None, None
        gy, gres = torch.empty_like(y), torch.empty_like(res)
        call('cfn_bn_add_relu_bwd', gout.contiguous(), gout2, out, y, A, res, Ar, gy, gres, gA, gB, gAr, N * C, vol)
        return gy, gA, gB, gres, gAr, gBr, None, None


def bn_add_relu(y, A, B, res, Ar=None, Br=None, split=False, link=None):
    """link (TailLink): one-tensor backward, see TailLink -- the producers of y (and of res when Ar is given) MUST be pwconv
    calls carrying the same link"""
    return _BnAddRelu.apply(y, A, B, res, Ar, Br, split, link)


class _AffineAct(Function):
    @staticmethod
    def forward(ctx, x, A, B, act):
        x = check(x).contiguous()
        N, C = x.shape[:2]
        out = torch.empty_like(x)
        A, B = _coef(A, N, C), _coef(B, N, C)
        call('cfn_affine_act_fwd', x, A, B, act, out, N * C, x[0, 0].numel())
        ctx.save_for_backward(x, A, B)
        ctx.act = act
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, A, B = ctx.saved_tensors
        N, C = x.shape[:2]
        gx = torch.empty_like(x)
        a64, b64 = _f64(N, C, x.device), _f64(N, C, x.device)
        call('cfn_affine_act_bwd', gout.contiguous(), x, A, B, ctx.act, gx, a64, b64, N * C, x[0, 0].numel())
        return gx, a64, b64, None


def affine_act(x, A, B, act=ACT_NONE):
    return _AffineAct.apply(x, A, B, act)


class _ChannelStats(Function):
    """per-(n,c) sum / sumsq (fp64) of a tensor; backward = broadcast (gs + 2 x gq)."""

    @staticmethod
    def forward(ctx, x):
        x = check(x).contiguous()
        N, C = x.shape[:2]
        s, q = _f64(N, C, x.device), _f64(N, C, x.device)
        call('cfn_channel_stats', x, s, q, N * C, x[0, 0].numel())
        ctx.save_for_backward(x)
        return s, q

    @staticmethod
    @once_differentiable
    def backward(ctx, gs, gq):
        (x,) = ctx.saved_tensors
        N, C = x.shape[:2]
        gx = torch.zeros_like(x)
        shp = (N, C) + (1,) * (x.dim() - 2)
        if gs is not None:
            gx = gx + gs.float().view(shp)
        if gq is not None:
            gx = gx + 2.0 * gq.float().view(shp) * x
        return gx


def channel_stats(x):
    return _ChannelStats.apply(x)


class _PoolHW(Function):
    """adaptive (OH,OW) spatial mean of act(A*x+B); see cfn_pool_hw_*."""

    @staticmethod
    def forward(ctx, x, A, B, act, OH, OW):
        x = check(x).contiguous()
        N, C, T, H, W = x.shape
        out = torch.empty(N, C, T, OH, OW, dtype=torch.float32, device=x.device)     # pooled tensors are fp32 in both precisions
        A, B = _coef(A, N, C), _coef(B, N, C)
        call('cfn_pool_hw_fwd' + _sfx(x), x, A, B, act, out, N * C, T, H, W, OH, OW)
        ctx.save_for_backward(x, A, B)
        ctx.meta = (act, OH, OW)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, A, B = ctx.saved_tensors
        act, OH, OW = ctx.meta
        N, C, T, H, W = x.shape
        gx = torch.empty_like(x)
        a64 = b64 = None
        if A is not None:
            a64, b64 = _f64(N, C, x.device), _f64(N, C, x.device)
        call('cfn_pool_hw_bwd' + _sfx(x), gout.contiguous(), x, A, B, act, gx, a64, b64, N * C, T, H, W, OH, OW)
        if A is None:
            return gx, None, None, None, None, None
        return gx, a64, b64, None, None, None


def pool_hw(x, OH, OW, A=None, B=None, act=ACT_NONE):
    return _PoolHW.apply(x, A, B, act, OH, OW)


class _Film(Function):
    """out = x * m + c with m, c constant over f x f spatial blocks ((N,C,T,H/f,W/f))."""

    @staticmethod
    def forward(ctx, x, m, c, f):
        x, m, c = check(x).contiguous(), check(m).contiguous(), check(c).contiguous()
        N, C, T, H, W = x.shape
        want = (N, C, T, H // f if f > 0 else -1, W // f if f > 0 else -1)
        if f <= 0 or H % f or W % f or tuple(m.shape) != want or tuple(c.shape) != want:
            # (the C ABI sees pointers only: block-constant coefficients of another plane size would be read out of bounds -- 96 x 96 clips
            # against 7 x 7 fine features faulted the device before this check)
            raise RuntimeError('film: coefficients %s / %s do not tile x %s with %d x %d blocks (expected %s)'
                               % (tuple(m.shape), tuple(c.shape), tuple(x.shape), f, f, want))
        out = torch.empty_like(x)
        call('cfn_film_fwd', x, m, c, out, N * C, T, H, W, f)
        ctx.save_for_backward(x, m)
        ctx.f = f
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, m = ctx.saved_tensors
        N, C, T, H, W = x.shape
        gx, gm, gc = torch.empty_like(x), torch.empty_like(m), torch.empty_like(m)
        call('cfn_film_bwd', g.contiguous(), x, m, gx, gm, gc, N * C, T, H, W, ctx.f)
        return gx, gm, gc, None


def film(x, m, c, f):
    return _Film.apply(x, m, c, f)


class _TimeSample(Function):
    """Grid Pool / Unpool resampler: x (B,C,Tin,*) , cdf (B,K) -> (B,C,K,*) ; see cfn_time_sample_*."""

    @staticmethod
    def forward(ctx, x, cdf):
        x, cdf = check(x).contiguous(), check(cdf).contiguous()
        B, C, Tin = x.shape[:3]
        K = cdf.shape[1]
        P = x[0, 0, 0].numel()
        out = torch.empty((B, C, K) + tuple(x.shape[3:]), dtype=torch.float32, device=x.device)
        call('cfn_time_sample_fwd', x, cdf, out, B, C, Tin, K, P)
        ctx.save_for_backward(x, cdf)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, cdf = ctx.saved_tensors
        B, C, Tin = x.shape[:3]
        K = cdf.shape[1]
        P = x[0, 0, 0].numel()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g64 = torch.zeros(B, K, dtype=torch.float64, device=x.device) if ctx.needs_input_grad[1] else None
        call('cfn_time_sample_bwd', g.contiguous(), x, cdf, gx, g64, B, C, Tin, K, P)
        return gx, (g64.float() if g64 is not None else None)


def time_sample(x, cdf):
    return _TimeSample.apply(x, cdf)


class _TimePool(Function):
    """t_pool 'avg' / 'max': (B,C,T,H,W) -> (B,C,T//R,H,W)   (cfn_time_pool_*)"""

    @staticmethod
    def forward(ctx, x, mode, R):
        x = check(x, torch.float32).contiguous()
        B, C, T = x.shape[:3]
        P = x[0, 0, 0].numel()
        out = torch.empty((B, C, T // R) + tuple(x.shape[3:]), dtype=torch.float32, device=x.device)
        call('cfn_time_pool_fwd', x, out, mode, B * C, T, R, P)
        ctx.save_for_backward(x)
        ctx.meta = (mode, R)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        mode, R = ctx.meta
        B, C, T = x.shape[:3]
        gx = torch.empty_like(x)
        call('cfn_time_pool_bwd', g.contiguous(), x, gx, mode, B * C, T, R, x[0, 0, 0].numel())
        return gx, None, None


def time_pool(x, mode, R=4):
    """mode 'avg' | 'max'"""
    return _TimePool.apply(x, {'avg': 0, 'max': 1}[mode], R)


def grid_time_index(cdf, Tin):
    """(i0 int32, w1 fp32) the resampler derives from a CDF (bit-exact ATen index arithmetic)."""
    cdf = check(cdf).contiguous()
    i0 = torch.empty(cdf.shape, dtype=torch.int32, device=cdf.device)
    w1 = torch.empty(cdf.shape, dtype=torch.float32, device=cdf.device)
    call('cfn_grid_time_index', cdf, cdf.numel(), Tin, i0, w1)
    return i0, w1


class _Interp1d(Function):
    @staticmethod
    def forward(ctx, x, y, xnew):
        x, y, xnew = check(x).contiguous(), check(y).contiguous(), check(xnew).contiguous()
        B = max(x.shape[0], y.shape[0], xnew.shape[0])
        N, Pq = x.shape[1], xnew.shape[1]
        rows = (int(x.shape[0] > 1), int(y.shape[0] > 1), int(xnew.shape[0] > 1))
        ynew = torch.empty(B, Pq, dtype=torch.float32, device=x.device)
        ind = torch.empty(B, Pq, dtype=torch.int64, device=x.device)
        call('cfn_interp1d_fwd', x, y, xnew, ynew, ind, B, N, Pq, *rows)
        ctx.save_for_backward(x, y, xnew, ind)
        ctx.rows = rows
        ctx.mark_non_differentiable(ind)
        return ynew, ind

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gind):
        x, y, xnew, ind = ctx.saved_tensors
        B, Pq = ind.shape
        N = x.shape[1]
        gx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.zeros_like(y) if ctx.needs_input_grad[1] else None
        gq = torch.zeros_like(xnew) if ctx.needs_input_grad[2] else None
        call('cfn_interp1d_bwd', g.contiguous(), x, y, xnew, ind, gx, gy, gq, B, N, Pq, *ctx.rows)
        return gx, gy, gq


def interp1d(x, y, xnew):
    """2-D inputs (rows broadcast when a tensor has a single row) -> (ynew, ind)."""
    return _Interp1d.apply(x, y, xnew)


class _TimeResize(Function):
    """linear resize along dim 2 (F.interpolate mode='linear', either align_corners convention)."""

    @staticmethod
    def forward(ctx, x, L, align_corners):
        x = check(x).contiguous()
        BC = x.shape[0] * x.shape[1]
        Kin = x.shape[2]
        P = x[0, 0, 0].numel()
        out = torch.empty(tuple(x.shape[:2]) + (L,) + tuple(x.shape[3:]), dtype=torch.float32, device=x.device)
        call('cfn_time_resize_fwd', x, out, BC, Kin, L, P, int(bool(align_corners)))
        ctx.meta = (tuple(x.shape), L, int(bool(align_corners)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        shape, L, ac = ctx.meta
        gx = torch.empty(shape, dtype=torch.float32, device=g.device)
        P = 1
        for d in shape[3:]:
            P *= d
        call('cfn_time_resize_bwd', g.contiguous(), gx, shape[0] * shape[1], shape[2], L, P, ac)
        return gx, None, None


def time_resize(x, L, align_corners=True):
    return _TimeResize.apply(x, L, align_corners)


def _detloss_args(logits, labels, masks, crops):
    """device fp32 tensors of matching shapes, contiguous -> (logits, labels, masks, B, C, T, TL)"""
    for name, v in (('logits', logits), ('labels', labels), ('masks', masks)):
        if not v.is_cuda or v.dtype != torch.float32:
            raise RuntimeError('detection_loss: %s must be a device fp32 tensor, got %s on %s (there is no CPU path)' % (name, v.dtype, v.device))
        if v.device != logits.device:
            raise RuntimeError('detection_loss: %s lives on %s, the logits on %s' % (name, v.device, logits.device))
    crops = int(crops)
    if logits.dim() != 3 or labels.dim() != 3 or masks.dim() != 2 or crops < 1:
        raise RuntimeError('detection_loss: logits (B*crops, C, T), labels (B, C, TL), masks (B, TL), crops >= 1')
    B, C, TL = labels.shape
    if logits.shape[0] != B * crops or logits.shape[1] != C or tuple(masks.shape) != (B, TL) or 0 in logits.shape or 0 in labels.shape:
        raise RuntimeError('detection_loss: logits %s, labels %s, masks %s do not belong together at %d crop(s)'
                           % (tuple(logits.shape), tuple(labels.shape), tuple(masks.shape), crops))
    return logits.contiguous(), labels.contiguous(), masks.contiguous(), B, C, logits.shape[2], TL


def detection_loss_fwd(logits, labels, masks, align_corners=True, crops=1, norm=None, world=1.0, want_probs=True):
    """cfn_detloss_fwd -> (cls (), loc (), probs (B, C, TL) or None, jstar (B*C) int32, ymax (B*C), norm_used (1) fp64); the last three are
    what cfn_detloss_bwd needs beside the inputs"""
    logits, labels, masks, B, C, T, TL = _detloss_args(logits, labels, masks, crops)
    dev = logits.device
    if norm is not None:
        if not norm.is_cuda or norm.device != dev or norm.numel() != 1:
            raise RuntimeError('detection_loss: norm must be a one-element tensor on the device of the logits')
        norm = norm.detach().to(torch.float32).reshape(1)
    cls = torch.empty((), dtype=torch.float32, device=dev)
    loc = torch.empty((), dtype=torch.float32, device=dev)
    probs = torch.empty(B, C, TL, dtype=torch.float32, device=dev) if want_probs else None
    jstar = torch.empty(B * C, dtype=torch.int32, device=dev)
    ymax = torch.empty(B * C, dtype=torch.float32, device=dev)
    rows = torch.empty(2 * B * C, dtype=torch.float64, device=dev)
    norm_used = torch.empty(1, dtype=torch.float64, device=dev)
    call('cfn_detloss_fwd', logits, labels, masks, norm, float(world), probs, cls, loc, jstar, ymax, rows, norm_used, B, C, T, TL, int(crops),
         int(bool(align_corners)))
    return cls, loc, probs, jstar, ymax, norm_used


def detection_loss_bwd(g_cls, g_loc, logits, labels, masks, jstar, ymax, norm_used, align_corners=True, crops=1, world=1.0):
    """cfn_detloss_bwd -> the gradient of g_cls * cls + g_loc * loc at the logits; g_cls / g_loc are device scalars"""
    logits, labels, masks, B, C, T, TL = _detloss_args(logits, labels, masks, crops)
    if jstar.numel() != B * C or ymax.numel() != B * C or norm_used.numel() != 1:
        raise RuntimeError('detection_loss_bwd: jstar / ymax / norm_used are not the ones the forward returned for these shapes')
    g_cls, g_loc = (g.detach().to(torch.float32).reshape(1) for g in (g_cls, g_loc))
    gx = torch.empty_like(logits)
    call('cfn_detloss_bwd', g_cls, g_loc, logits, labels, masks, jstar.contiguous(), ymax.contiguous(), norm_used, float(world), gx, B, C, T, TL,
         int(crops), int(bool(align_corners)))
    return gx


class _DetectionLoss(Function):
    """the detection loss of both training scripts in one forward and one backward kernel (csrc/detloss.hip)"""

    @staticmethod
    def forward(ctx, logits, labels, masks, align_corners, crops, norm, world, want_probs):
        cls, loc, probs, jstar, ymax, norm_used = detection_loss_fwd(logits, labels, masks, align_corners, crops, norm, world, want_probs)
        ctx.save_for_backward(logits, labels, masks, jstar, ymax, norm_used)
        ctx.meta = (bool(align_corners), int(crops), float(world))
        if probs is not None:
            ctx.mark_non_differentiable(probs)
        return cls, loc, probs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_loc, _g_probs):
        gx = detection_loss_bwd(g_cls, g_loc, *ctx.saved_tensors, *ctx.meta) if ctx.needs_input_grad[0] else None
        return gx, None, None, None, None, None, None, None


def detection_loss(logits, labels, masks, align_corners, crops=1, norm=None, world=1.0, want_probs=True):
    """cls + loc loss of train_fine.py:199-213 / train_coarse_fineFEAT.py:226-240 -> (cls, loc, probs).  logits (B*crops, C, T), labels
    (B, C, TL), masks (B, TL): device fp32.  norm: the loc normaliser as a device scalar (None: C * sum(masks) of this call); world: the
    factor on loc.  probs carries no gradient (the training loops log it); want_probs=False skips its store and returns None."""
    return _DetectionLoss.apply(logits, labels, masks, align_corners, crops, norm, world, want_probs)


def _geom(kernel, stride, padding):
    return (ctypes.c_int * 9)(*(tuple(kernel) + tuple(stride) + tuple(padding)))


class _ConvDense(Function):
    """dense conv3d (no bias) as implicit GEMM; prologue / stats convention of the other convs.  cfn_conv3d_dense_*."""

    @staticmethod
    def forward(ctx, x, A, B, w, act, kernel, stride, padding, want_stats):
        x = check(x).contiguous()
        N, Ci, T, H, W = x.shape
        Co = w.shape[0]
        g = _geom(kernel, stride, padding)
        To = (T + 2 * padding[0] - kernel[0]) // stride[0] + 1
        Ho = (H + 2 * padding[1] - kernel[1]) // stride[1] + 1
        Wo = (W + 2 * padding[2] - kernel[2]) // stride[2] + 1
        y = torch.empty(N, Co, To, Ho, Wo, dtype=torch.float32, device=x.device)
        s = q = None
        if want_stats:
            s, q = _f64(N, Co, x.device), _f64(N, Co, x.device)
        w2 = w.reshape(Co, -1).contiguous()
        A, B = _coef(A, N, Ci), _coef(B, N, Ci)
        call('cfn_conv3d_dense_fwd', x, A, B, act, w2, y, s, q, N, Ci, Co, T, H, W, g)
        ctx.save_for_backward(x, A, B, w2, y)
        ctx.meta = (act, tuple(kernel), tuple(stride), tuple(padding), tuple(w.shape))
        ctx.wparam = w
        if not want_stats:
            return y, None, None
        return y, s, q

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gs, gq):
        x, A, B, w2, y = ctx.saved_tensors
        act, kernel, stride, padding, wshape = ctx.meta
        N, Ci, T, H, W = x.shape
        Co = w2.shape[0]
        g = _geom(kernel, stride, padding)
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        gs, gq = _opt(gs), _opt(gq)
        gx = gA = gB = gw = None
        if ctx.needs_input_grad[0] or (A is not None and ctx.needs_input_grad[1]):
            gx = torch.empty_like(x)
            ab = a64 = b64 = None
            if A is not None:
                ab, a64, b64 = _f64pair(N, Ci, x.device)
            call('cfn_conv3d_dense_bwd_data', gy, y, gs, gq, w2, x, A, B, act, gx, a64, b64, N, Ci, Co, T, H, W, g)
            if A is not None:
                gA, gB = ab[0], ab[1]
        if ctx.needs_input_grad[3]:
            g64, fin = _gw_buffers(ctx.wparam, Co, w2.shape[1], x.device)
            call('cfn_conv3d_dense_bwd_weight', gy, y, gs, gq, x, A, B, act, g64, N, Ci, Co, T, H, W, g)
            gw = fin()
        return gx, gA, gB, gw, None, None, None, None, None


def conv3d_dense(x, w, kernel, stride, padding, A=None, B=None, act=ACT_NONE, stats=True):
    return _ConvDense.apply(x, A, B, w, act, kernel, stride, padding, stats)


def conv3d_dense_route(op, N, Cin, Cout, T, H, W, geom=None, flags=0, cus=0):
    """the kernel a dense conv of this shape runs on (cfn_conv3d_dense_route, include/cfn_hip.h): host only.  op 0 forward, 1 data gradient,
    2 weight gradient, 3 stem forward, 4 stem weight gradient, 5 / 6 the stem on uint8 frames, forward / weight gradient ('convert ' + the line of
    op 3 / 4 where stem_conv_u8 converts the frames first); geom = (kernel, stride, padding) flattened to 9 ints (ops 0-2);
    cus = 0: the current device's CUs (256 without a device)"""
    out = ctypes.create_string_buffer(256)
    g = (ctypes.c_int * 9)(*geom) if geom is not None else None
    if query('cfn_conv3d_dense_route', op, N, Cin, Cout, T, H, W, g, flags, cus, out, 256):
        raise RuntimeError(last_error())
    return out.value.decode()


class _FusionGather(Function):
    """z[r,c,k,p] = sum_t x[b] at[b] GX[r] mask[b] / (sum_t at GX mask + 1e-6), at = sigmoid(at_raw + at_bias), r = b*crops + j
    (cfn_fusion_gather_*)"""

    @staticmethod
    def forward(ctx, x, at_raw, at_bias, GX, mask, crops):
        x, at_raw, GX, mask = check(x).contiguous(), check(at_raw).contiguous(), check(GX).contiguous(), check(mask).contiguous()
        B, C, Tf, P = x.shape
        K = GX.shape[2]
        if GX.shape[0] != B * crops or GX.shape[1] != Tf or tuple(mask.shape) != (B, Tf) or tuple(at_raw.shape) != (B, Tf, P):
            raise RuntimeError('fusion_gather: inconsistent shapes x %s at %s GX %s mask %s crops %d'
                               % (tuple(x.shape), tuple(at_raw.shape), tuple(GX.shape), tuple(mask.shape), crops))
        z = torch.empty(B * crops, C, K, P, dtype=torch.float32, device=x.device)
        den = torch.empty(B * crops, K, P, dtype=torch.float32, device=x.device)
        call('cfn_fusion_gather_fwd', x, at_raw, at_bias, GX, mask, z, den, B, crops, C, Tf, K, P)
        ctx.save_for_backward(x, at_raw, at_bias, GX, mask, z, den)
        ctx.crops = crops
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        x, at_raw, at_bias, GX, mask, z, den = ctx.saved_tensors
        B, C, Tf, P = x.shape
        K, crops = GX.shape[2], ctx.crops
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[0] else None
        want_at = need[1] or (at_bias is not None and need[2])
        gat = torch.empty_like(at_raw) if want_at else None
        gGX = torch.empty_like(GX) if need[3] else None
        dw = torch.empty(B * crops, Tf, K, P, dtype=torch.float32, device=x.device)
        call('cfn_fusion_gather_bwd', gz.contiguous(), z, den, x, at_raw, at_bias, GX, mask, gx, gat, gGX, dw, B, crops, C, Tf, K, P)
        gb = gat.sum().view(at_bias.shape) if (at_bias is not None and need[2]) else None
        return gx, (gat if need[1] else None), gb, gGX, None, None


def fusion_gather(x, at_raw, at_bias, GX, mask, crops=1):
    """x (B,C,Tf,P), at_raw (B,Tf,P), at_bias (1,) or None, GX (B*crops,Tf,K), mask (B,Tf) -> (B*crops,C,K,P)"""
    return _FusionGather.apply(x, at_raw, at_bias, GX, mask, crops)


class _GaussAlign(Function):
    """Gaussian.forward (x3d_coarse.py:256-286) as one kernel; gradient w.r.t. the CDF knots only."""

    @staticmethod
    def forward(ctx, meta, mask, gx, tx, ratio, crops, K):
        # the C ABI takes pointers and sizes: refuse shapes that do not fit BEFORE any launch (the wording of cfn::gauss_align)
        if mask.dim() != 2 or meta.dim() != 2 or tuple(meta.shape) != (mask.shape[0], 4) or meta.device != mask.device or crops < 1 or K < 1:
            raise RuntimeError('gauss_align: meta (B, 4), mask (B, Tf) on one device, crops >= 1, K >= 1 (got meta %s mask %s crops %d K %d)'
                               % (tuple(meta.shape), tuple(mask.shape), crops, K))
        meta, mask = meta.contiguous(), check(mask).contiguous()
        if meta.dtype != torch.int64:
            meta = meta.to(torch.int64)
        B, Tf = mask.shape
        if gx is not None:
            if tuple(gx.shape) != (B * crops, K) or gx.device != mask.device:
                raise RuntimeError('gauss_align: gx must be the (B * crops, K) CDF (got %s for B %d crops %d K %d)'
                                   % (tuple(gx.shape), B, crops, K))
            gx = check(gx).contiguous()
        GX = torch.empty(B * crops, Tf, K, dtype=torch.float32, device=mask.device)
        call('cfn_gauss_align_fwd', meta, mask, gx, float(tx), float(ratio), GX, B, crops, Tf, K)
        ctx.save_for_backward(meta, mask, gx)
        ctx.cfg = (float(tx), float(ratio), crops, K)
        return GX

    @staticmethod
    @once_differentiable
    def backward(ctx, gGX):
        meta, mask, gx = ctx.saved_tensors
        tx, ratio, crops, K = ctx.cfg
        ggx = None
        if gx is not None and ctx.needs_input_grad[2]:
            B, Tf = mask.shape
            ggx = torch.empty_like(gx)
            call('cfn_gauss_align_bwd', gGX.contiguous(), meta, mask, gx, tx, ratio, ggx, B, crops, Tf, K)
        return None, None, ggx, None, None, None, None


def gauss_align(meta, mask, gx, tx, ratio, crops, K):
    """meta (B,4) int64, mask (B,Tf), gx (B*crops,K) or None (then tl = arange(K)) -> GX (B*crops,Tf,K)"""
    return _GaussAlign.apply(meta, mask, gx, 1.0 if tx is None else tx, ratio, crops, K)


class _GridCdf(Function):
    """saliency logits (B,Kin) (+ scalar bias) -> CDF knots (B,Kin+1)   (cfn_grid_cdf_*)"""

    @staticmethod
    def forward(ctx, g, bias):
        g = check(g).contiguous()
        B, Kin = g.shape
        cdf = torch.empty(B, Kin + 1, dtype=torch.float32, device=g.device)
        call('cfn_grid_cdf_fwd', g, bias, cdf, B, Kin)
        ctx.save_for_backward(g, bias)
        return cdf

    @staticmethod
    @once_differentiable
    def backward(ctx, gcdf):
        g, bias = ctx.saved_tensors
        B, Kin = g.shape
        gg = torch.empty_like(g)
        call('cfn_grid_cdf_bwd', gcdf.contiguous(), g, bias, gg, B, Kin)
        gb = gg.sum().view(bias.shape) if (bias is not None and ctx.needs_input_grad[1]) else None
        return gg, gb


def grid_cdf(g, bias=None):
    return _GridCdf.apply(g, bias)


# ---- packed 16-bit fine features (csrc/featpack.hip; the record format and the batch type: cfn_hip/featpack.py) ---------------------------
FEAT_POSITIONS = 49


def _feat_channels(channels, what):
    channels = tuple(int(c) for c in channels)
    if len(channels) != 5 or any(c <= 0 or c % 8 for c in channels):
        raise RuntimeError('%s: five channel counts that are positive multiples of 8 expected, got %s' % (what, channels))
    return channels


def _feat_sfx(dtype, what):
    if dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError('%s: fp16 or bf16 data expected, got %s' % (what, dtype))
    return '_f16' if dtype == torch.float16 else '_bf16'


def feat_unpack(data, offsets, lengths, channels, t_max, out=None):
    """data: 1-D fp16 / bf16 on the GPU; offsets (B, 5) int64 = first element of every video's five time-major blocks (length, C_k, 49),
    multiples of 8; lengths (B,) int32 -> the five fp32 maps (B, C_k, t_max, 7, 7), zero behind each video's own length.  One launch;
    offsets and lengths are read on the device only (no wait, capturable); `t_max` is a host int.  out: five preallocated maps."""
    channels = _feat_channels(channels, 'feat_unpack')
    sfx = _feat_sfx(data.dtype, 'feat_unpack')
    t_max = int(t_max)
    if data.dim() != 1 or not data.is_contiguous():
        raise RuntimeError('feat_unpack: a flat contiguous buffer expected, got %s' % (tuple(data.shape),))
    if offsets.dtype != torch.int64 or offsets.dim() != 2 or offsets.shape[1] != 5 or offsets.shape[0] < 1:
        raise RuntimeError('feat_unpack: offsets (B, 5) int64 expected, got %s %s' % (offsets.dtype, tuple(offsets.shape)))
    B = int(offsets.shape[0])
    if lengths.dtype != torch.int32 or lengths.numel() != B:
        raise RuntimeError('feat_unpack: lengths (%d,) int32 expected, got %s %s' % (B, lengths.dtype, tuple(lengths.shape)))
    if t_max < 1:
        raise RuntimeError('feat_unpack: t_max >= 1 expected, got %d' % t_max)
    if out is None:
        out = [torch.empty(B, c, t_max, 7, 7, dtype=torch.float32, device=data.device) for c in channels]
    else:
        out = list(out)
        if len(out) != 5:
            raise RuntimeError('feat_unpack: out: five maps expected, got %d' % len(out))
        for y, c in zip(out, channels):
            if y.dtype != torch.float32 or tuple(y.shape) != (B, c, t_max, 7, 7) or not y.is_contiguous():
                raise RuntimeError('feat_unpack: out: five contiguous fp32 maps (%d, C_k, %d, 7, 7) with C_k = %s expected, got %s %s'
                                   % (B, t_max, channels, y.dtype, tuple(y.shape)))
    call('cfn_feat_unpack' + sfx, data, offsets.contiguous(), lengths.contiguous(), *out, B, t_max, *channels, int(data.numel()))
    return out


def feat_pack(feat, dtype, out=None):
    """feat: the five fp32 maps (C_k, T', 7, 7) (or (1, C_k, T', 7, 7)) of ONE video on the GPU, in key order -> its record payload: a
    1-D fp16 / bf16 tensor, the five time-major blocks (T', C_k, 49) back to back; round to nearest even, as tensor.to(dtype) on the CPU"""
    sfx = _feat_sfx(dtype, 'feat_pack')
    xs = []
    for x in feat:
        if x.dim() == 5 and x.shape[0] == 1:
            x = x[0]
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[2] * x.shape[3] != FEAT_POSITIONS:
            raise RuntimeError('feat_pack: fp32 maps (C, T, 7, 7) expected, got %s %s' % (x.dtype, tuple(x.shape)))
        xs.append(x.contiguous())
    if len(xs) != 5 or any(x.shape[1] != xs[0].shape[1] for x in xs):
        raise RuntimeError('feat_pack: five maps of one frame count expected, got %s' % [tuple(x.shape) for x in xs])
    channels = _feat_channels([x.shape[0] for x in xs], 'feat_pack')
    T = int(xs[0].shape[1])
    n = T * sum(channels) * FEAT_POSITIONS
    if out is None:
        out = torch.empty(n, dtype=dtype, device=xs[0].device)
    elif out.dtype != dtype or out.dim() != 1 or out.numel() != n or not out.is_contiguous():
        raise RuntimeError('feat_pack: out: a flat %s tensor of %d elements expected, got %s %s' % (dtype, n, out.dtype, tuple(out.shape)))
    call('cfn_feat_pack' + sfx, *xs, out, T, *channels)
    return out


# ---- frame labels from annotation segments (csrc/seglabels.hip; the sample record and the batch type: cfn_hip/seglabels.py) ----------------
def seg_labels(seg, offsets, fps, window, n_classes, t_max, out=None):
    """seg (S, 3) fp64 rows [class, start_s, end_s] on the GPU; offsets (B + 1,) int32: sample b owns rows offsets[b]:offsets[b + 1];
    fps (B,) fp64; window (B, 2) int32 = first frame, length -> (labels (B, n_classes, t_max) fp32, mask (B, t_max) fp32, valid_t (B,) int32):
    labels[b, c, t] = 1 iff t < length and some segment (c, s, e) of sample b has (start + t) / fps > s and (start + t) / fps < e, in fp64
    (charades_fine.py:110-117, :165, :214-220).  One launch that writes every element; the tensors are read on the device only (no wait,
    capturable); `n_classes` and `t_max` are host ints.  out: the three preallocated tensors.  No gradient, no CPU path."""
    n_classes, t_max = int(n_classes), int(t_max)
    if seg.dtype != torch.float64 or seg.dim() != 2 or seg.shape[1] != 3 or seg.shape[0] < 1 or not seg.is_contiguous():
        raise RuntimeError('seg_labels: seg: a contiguous (S, 3) float64 tensor with S >= 1 expected, got %s %s' % (seg.dtype, tuple(seg.shape)))
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
        raise RuntimeError('seg_labels: offsets (B + 1,) int32 expected, got %s %s' % (offsets.dtype, tuple(offsets.shape)))
    B = int(offsets.numel()) - 1
    if fps.dtype != torch.float64 or tuple(fps.shape) != (B,):
        raise RuntimeError('seg_labels: fps (%d,) float64 expected, got %s %s' % (B, fps.dtype, tuple(fps.shape)))
    if window.dtype != torch.int32 or tuple(window.shape) != (B, 2):
        raise RuntimeError('seg_labels: window (%d, 2) int32 = start, length expected, got %s %s' % (B, window.dtype, tuple(window.shape)))
    if n_classes < 1 or t_max < 1:
        raise RuntimeError('seg_labels: n_classes >= 1 and t_max >= 1 expected, got %d and %d' % (n_classes, t_max))
    dev = seg.device
    if out is None:
        out = (torch.empty(B, n_classes, t_max, dtype=torch.float32, device=dev), torch.empty(B, t_max, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))
    else:
        out = tuple(out)
        want = ((torch.float32, (B, n_classes, t_max)), (torch.float32, (B, t_max)), (torch.int32, (B,)))
        if len(out) != 3 or any(y.dtype != dt or tuple(y.shape) != shp or not y.is_contiguous() for y, (dt, shp) in zip(out, want)):
            raise RuntimeError('seg_labels: out: contiguous labels %s fp32, mask %s fp32 and valid_t %s int32 expected, got %s'
                               % (want[0][1], want[1][1], want[2][1], [(y.dtype, tuple(y.shape)) for y in out]))
    call('cfn_seg_labels', seg, offsets.contiguous(), fps.contiguous(), window.contiguous(), out[0], out[1], out[2], B, n_classes, t_max,
         int(seg.shape[0]))
    return out


# ---- argument checks shared by the segment operators below (decode, levels, NMS, soft-NMS, segment AP) ---------------------------------------
def _one_gpu(what, host, **tensors):
    """every argument a contiguous device tensor, all on one GPU -> that device.  host: the host spelling that the refusal names"""
    dev = None
    for name, t in tensors.items():
        if not torch.is_tensor(t) or t.device.type != 'cuda' or (dev is not None and t.device != dev):
            raise RuntimeError('%s: %s is on %s: device tensors on one GPU expected (there is no CPU path; %s is the host spelling)'
                               % (what, name, getattr(t, 'device', 'the host (a %s)' % type(t).__name__), host))
        if not t.is_contiguous():
            raise RuntimeError('%s: %s must be contiguous' % (what, name))
        dev = t.device
    return dev


def _out_tuple(what, out, dev, slots, ws_bytes):
    """slots: (name, dtype, trailing shape, rows, exact) per output, exact: rows == or >=.  out=None: new tensors for the slots and a uint8
    workspace of ws_bytes behind them; otherwise the caller's tuple, checked against the same list (the workspace: 8-byte aligned, >= ws_bytes)"""
    if out is None:
        return tuple(torch.empty(rows, *trail, dtype=dt, device=dev) for _, dt, trail, rows, _ in slots) \
            + (torch.empty(ws_bytes, dtype=torch.uint8, device=dev),)
    out = tuple(out)
    if len(out) != len(slots) + 1 or any(y.dtype != dt or tuple(y.shape[1:]) != tuple(trail) or y.dim() != 1 + len(trail) or not y.is_contiguous()
                                         or (y.shape[0] != rows if exact else y.shape[0] < rows) for y, (_, dt, trail, rows, exact) in zip(out, slots)) \
            or out[-1].dtype != torch.uint8 or out[-1].dim() != 1 or out[-1].numel() < ws_bytes or out[-1].data_ptr() % 8 or not out[-1].is_contiguous():
        want = ', '.join('%s (%s%d%s) %s' % (name, '' if exact else '>= ', rows, ''.join(', %d' % w for w in trail) or ',', str(dt)[6:])
                         for name, dt, trail, rows, exact in slots)
        raise RuntimeError('%s: out: contiguous %s and an 8-byte aligned uint8 workspace of >= %d bytes expected, got %s'
                           % (what, want, ws_bytes, [(y.dtype, tuple(y.shape)) for y in out]))
    return out


def _record_slots(cap):
    """the three record buffers of a Detections"""
    return [('seg', torch.float64, (3,), cap, False), ('frames', torch.int32, (3,), cap, False), ('score', torch.float32, (2,), cap, False)]


# ---- activity segments from per-frame scores (csrc/detections.hip; the batch type, the host reference and the writer: cfn_hip/detections.py) --
DECODE_MAX_TL = 65536


def decode_segments_cap(B, C, TL):
    """the worst case of decode_segments: every second frame of every row a run of its own"""
    return int(B) * int(C) * ((int(TL) + 1) // 2)


def decode_segments_workspace_bytes(B, C, TL):
    n = int(query('cfn_decode_segments_workspace_bytes', int(B), int(C), int(TL)))
    if n < 0:
        raise RuntimeError('decode_segments: probs: B <= 65535, C < 2^19, TL <= %d and B * C * TL < 2^31 expected, got (%d, %d, %d)'
                           % (DECODE_MAX_TL, B, C, TL))
    return n


def _decode_arguments(what, probs, valid_t, fps, start, name, levels, max_gap, min_len, cap):
    """the checks decode_segments and decode_segments_levels share.  name 'levels': levels (C, K); name 'thr': the K = 1 case, `levels` is
    decode_segments' thr, a float or a (C,) tensor -> (B, C, K, TL, valid_t, fps, start and the thresholds as contiguous device tensors,
    max_gap, min_len, cap, the device)"""
    if not torch.is_tensor(probs) or probs.dtype != torch.float32 or probs.dim() != 3 or min(probs.shape) < 1 or not probs.is_contiguous():
        raise RuntimeError('%s: probs: a contiguous (B, C, TL) float32 tensor expected, got %s %s'
                           % (what, getattr(probs, 'dtype', type(probs).__name__), tuple(getattr(probs, 'shape', ()))))
    B, C, TL = (int(s) for s in probs.shape)
    got = '%s %s' % (getattr(levels, 'dtype', type(levels).__name__), tuple(getattr(levels, 'shape', ())))
    if name == 'thr':
        K = 1
        if isinstance(levels, bool) or not isinstance(levels, (int, float, torch.Tensor)) \
                or (torch.is_tensor(levels) and (levels.dtype != torch.float32 or tuple(levels.shape) != (C,))):
            raise RuntimeError('%s: thr: a float or a (%d,) float32 tensor expected, got %s' % (what, C, got))
    else:
        if not torch.is_tensor(levels) or levels.dtype != torch.float32 or levels.dim() != 2 or int(levels.shape[0]) != C \
                or not 1 <= int(levels.shape[1]) <= DECODE_MAX_LEVELS or not levels.is_contiguous():
            raise RuntimeError('%s: levels: a contiguous (%d, K) float32 tensor with 1 <= K <= %d expected, got %s' % (what, C, DECODE_MAX_LEVELS, got))
        K = int(levels.shape[1])
    if TL > DECODE_MAX_TL or B > 65535 or C >= (1 << 19) or B * C * K * TL >= (1 << 31):
        raise RuntimeError('%s: probs: B <= 65535, C < 2^19, TL <= %d and B * C * K * TL < 2^31 expected, got (%d, %d, %d) and K = %d'
                           % (what, DECODE_MAX_TL, B, C, TL, K))
    for arg, t, dt in (('valid_t', valid_t, torch.int32), ('fps', fps, torch.float64), ('start', start, torch.int32)):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (B,):
            raise RuntimeError('%s: %s (%d,) %s expected, got %s %s' % (what, arg, B, dt, getattr(t, 'dtype', type(t).__name__), tuple(getattr(t, 'shape', ()))))
    max_gap, min_len = int(max_gap), int(min_len)
    if max_gap < 0:
        raise RuntimeError('%s: max_gap >= 0 expected, got %d' % (what, max_gap))
    if min_len < 1:
        raise RuntimeError('%s: min_len >= 1 expected, got %d' % (what, min_len))
    cap = decode_segments_levels_cap(B, C, K, TL) if cap is None else int(cap)
    if cap < 1 or cap >= (1 << 31):
        raise RuntimeError('%s: cap in [1, 2^31) expected, got %d' % (what, cap))
    valid_t, fps, start = valid_t.contiguous(), fps.contiguous(), start.contiguous()
    tensors = dict(probs=probs, valid_t=valid_t, fps=fps, start=start)
    if torch.is_tensor(levels):
        levels = tensors[name] = levels.contiguous()
    dev = _one_gpu(what, 'cfn_hip.detections.' + ('decode_reference' if name == 'thr' else 'decode_levels_reference'), **tensors)
    if not torch.is_tensor(levels):
        levels = torch.full((C,), float(levels), dtype=torch.float32, device=dev)
    return B, C, K, TL, valid_t, fps, start, levels, max_gap, min_len, cap, dev


def decode_segments(probs, valid_t, fps, start, thr, max_gap=0, min_len=1, cap=None, out=None):
    """probs (B, C, TL) fp32 on the GPU; valid_t (B,) int32; fps (B,) fp64; start (B,) int32 = first frame of each window
    (SegLabels.window[:, 0]); thr: a float or a (C,) fp32 device tensor -> (seg (cap, 3) fp64 rows [class, start_s, end_s], frames (cap, 3)
    int32 [t0, t1, n_active], score (cap, 2) fp32 [max, mean], offsets (B + 1,) int32, total (1,) int32): the runs of frames with
    probs > thr[c] in front of valid_t, gaps of at most `max_gap` inactive frames closed, runs shorter than `min_len` dropped, ordered by
    (b, c, t0) -- the definition is in cfn_hip/detections.py (decode_reference spells it on the host).  offsets and total are true counts;
    rows >= cap are not written (cap=None: B * C * ((TL + 1) // 2), which cannot overflow).  Three launches, no atomics, nothing is read
    back (no wait, capturable with out=); `max_gap`, `min_len` and `cap` are host ints.  out: the five preallocated tensors and a uint8
    workspace of decode_segments_workspace_bytes(B, C, TL) bytes (then thr must be a tensor for nothing to be allocated).  No gradient, no CPU path."""
    what = 'decode_segments'
    B, C, _, TL, valid_t, fps, start, thr, max_gap, min_len, cap, dev = _decode_arguments(what, probs, valid_t, fps, start, 'thr', thr, max_gap, min_len, cap)
    out = _out_tuple(what, out, dev, _record_slots(cap) + [('offsets', torch.int32, (), B + 1, True), ('total', torch.int32, (), 1, True)],
                     decode_segments_workspace_bytes(B, C, TL))
    call('cfn_decode_segments', probs, valid_t, fps, start, thr, out[0], out[1], out[2], out[3],
         out[4], out[5], B, C, TL, max_gap, min_len, cap)
    return out[:5]


# ---- activity proposals: candidates at K levels, then temporal NMS (csrc/detections.hip, csrc/segnms.hip; the rules: cfn_hip/detections.py) ---
DECODE_MAX_LEVELS = 16
NMS_DET_TILE = 1024              # candidates of a (video, class) group suppressed in LDS (cfn_nms_det_tile(); more take the general path)


def decode_segments_levels_cap(B, C, K, TL):
    """the worst case of decode_segments_levels: every second frame of every row a run of its own, at every level"""
    return int(B) * int(C) * int(K) * ((int(TL) + 1) // 2)


def decode_segments_levels_workspace_bytes(B, C, K, TL):
    n = int(query('cfn_decode_segments_levels_workspace_bytes', int(B), int(C), int(K), int(TL)))
    if n < 0:
        raise RuntimeError('decode_segments_levels: probs: B <= 65535, C < 2^19, TL <= %d, K in [1, %d] and B * C * K * TL < 2^31 expected, got '
                           '(%d, %d, %d) and K = %d' % (DECODE_MAX_TL, DECODE_MAX_LEVELS, B, C, TL, K))
    return n


def decode_segments_levels(probs, valid_t, fps, start, levels, max_gap=0, min_len=1, cap=None, out=None):
    """decode_segments at K threshold levels in one call: levels (C, K) fp32 on the device, 1 <= K <= 16, row c = class c's thresholds in the
    caller's order -> (seg, frames, score, level (cap,) uint8, offsets, total): candidate row (b, c, k) is decode_segments' rules applied to
    probs[b, c, :] with levels[c, k]; seg's class column holds c, `level` holds k; the order is (b, c, k, t0) (rules L1-L4 of
    cfn_hip/detections.py; decode_levels_reference spells them on the host).  cap=None: B * C * K * ((TL + 1) // 2), which cannot overflow.
    Three launches, nothing is read back (capturable with out=).  out: the six tensors and a uint8 workspace of
    decode_segments_levels_workspace_bytes(B, C, K, TL) bytes.  No gradient, no CPU path."""
    what = 'decode_segments_levels'
    B, C, K, TL, valid_t, fps, start, levels, max_gap, min_len, cap, dev = _decode_arguments(what, probs, valid_t, fps, start, 'levels', levels, max_gap,
                                                                                             min_len, cap)
    out = _out_tuple(what, out, dev, _record_slots(cap) + [('level', torch.uint8, (), cap, False), ('offsets', torch.int32, (), B + 1, True),
                                                           ('total', torch.int32, (), 1, True)], decode_segments_levels_workspace_bytes(B, C, K, TL))
    call('cfn_decode_segments_levels', probs, valid_t, fps, start, levels, out[0], out[1], out[2], out[3],
         out[4], out[5], out[6], B, C, K, TL, max_gap, min_len, cap)
    return out[:6]


def nms_segments_workspace_bytes(B, C, cap_in):
    n = int(query('cfn_nms_segments_workspace_bytes', int(B), int(C), int(cap_in)))
    if n < 0:
        raise RuntimeError('nms_segments: B and C in [1, 65535] and cap_in in [1, 2^31) expected, got (%d, %d, %d)' % (B, C, cap_in))
    return n


def _nms_arguments(what, seg, frames, score, offsets, n_classes, score_col, cap_out, out, workspace_bytes):
    """the checks nms_segments and soft_nms_segments share -> (B, n_classes, score_col, cap_in, cap_out, out: the seven tensors and the workspace)"""
    dev = _one_gpu(what, 'cfn_hip.detections.' + what.replace('_segments', '_reference'), seg=seg, frames=frames, score=score, offsets=offsets)
    if seg.dtype != torch.float64 or seg.dim() != 2 or seg.shape[1] != 3 or seg.shape[0] < 1:
        raise RuntimeError('%s: seg: a (cap_in, 3) float64 tensor with cap_in >= 1 expected, got %s %s' % (what, seg.dtype, tuple(seg.shape)))
    cap_in = int(seg.shape[0])
    if frames.dtype != torch.int32 or tuple(frames.shape) != (cap_in, 3) or score.dtype != torch.float32 or tuple(score.shape) != (cap_in, 2):
        raise RuntimeError('%s: frames (%d, 3) int32 and score (%d, 2) float32 expected, got %s %s and %s %s'
                           % (what, cap_in, cap_in, frames.dtype, tuple(frames.shape), score.dtype, tuple(score.shape)))
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
        raise RuntimeError('%s: offsets (B + 1,) int32 expected, got %s %s' % (what, offsets.dtype, tuple(offsets.shape)))
    B, n_classes, score_col = int(offsets.numel()) - 1, int(n_classes), int(score_col)
    if n_classes < 1 or score_col not in (0, 1):
        raise RuntimeError('%s: n_classes >= 1 and score_col 0 (max) or 1 (mean) expected, got %d, %d' % (what, n_classes, score_col))
    cap_out = cap_in if cap_out is None else int(cap_out)
    if cap_out < 1 or cap_out >= (1 << 31):
        raise RuntimeError('%s: cap_out in [1, 2^31) expected, got %d' % (what, cap_out))
    out = _out_tuple(what, out, dev, _record_slots(cap_out) + [('offsets', torch.int32, (), B + 1, True), ('total', torch.int32, (), 1, True),
                                                               ('keep', torch.uint8, (), cap_in, False), ('src', torch.int32, (), cap_out, False)],
                     workspace_bytes(B, n_classes, cap_in))
    if any(y.data_ptr() == x.data_ptr() for y, x in zip(out[:3], (seg, frames, score))):
        raise RuntimeError('%s: out: seg, frames and score must not be the inputs' % what)
    return B, n_classes, score_col, cap_in, cap_out, out


def _host_float(what, name, v, lo, hi, text):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) <= hi:
        raise RuntimeError('%s: %s: a host float of %s expected, got %r' % (what, name, text, v))
    return float(v)


def nms_segments(seg, frames, score, offsets, n_classes, nms_thr, score_col=0, cap_out=None, out=None):
    """Temporal non-maximum suppression of a batch's detections (seg (cap_in, 3) fp64, frames (cap_in, 3) int32, score (cap_in, 2) fp32,
    offsets (B + 1,) int32: a Detections whose (video, class) groups are contiguous) -> (seg, frames, score, offsets, total, keep (cap_in,)
    uint8, src (cap_out,) int32): inside every group, in the order of score[:, score_col] descending (ties: the lower row), a candidate is
    kept iff no candidate kept before it has a temporal IoU with it above `nms_thr`; the kept rows in their input order, copied bit for bit
    (rules N1-N7 of cfn_hip/detections.py; nms_reference spells them on the host).  offsets and total are true counts; rows >= cap_out
    (default: cap_in, which cannot overflow) are not written; keep is written for the rows of the batch's groups only; src holds the input
    row of each output row.  `n_classes`, `nms_thr` (a float of [0, 1]), `score_col` (0 = max, 1 = mean) and `cap_out` are host values.
    Three launches, nothing is read back (capturable with out=).  out: the seven tensors and a uint8 workspace of
    nms_segments_workspace_bytes(B, C, cap_in) bytes.  No gradient, no CPU path."""
    what = 'nms_segments'
    B, n_classes, score_col, cap_in, cap_out, out = _nms_arguments(what, seg, frames, score, offsets, n_classes, score_col, cap_out, out,
                                                                   nms_segments_workspace_bytes)
    nms_thr = _host_float(what, 'nms_thr', nms_thr, 0.0, 1.0, '[0, 1]')
    call('cfn_nms_segments', seg, frames, score, offsets, out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], B, n_classes, score_col,
         nms_thr, cap_in, cap_out)
    return out[:7]


def soft_nms_segments_workspace_bytes(B, C, cap_in):
    n = int(query('cfn_soft_nms_segments_workspace_bytes', int(B), int(C), int(cap_in)))
    if n < 0:
        raise RuntimeError('soft_nms_segments: B and C in [1, 65535] and cap_in in [1, 2^31) expected, got (%d, %d, %d)' % (B, C, cap_in))
    return n


def soft_nms_segments(seg, frames, score, offsets, n_classes, method=1, sigma=0.5, min_score=0.001, max_keep=0, nms_thr=0.5, score_col=0,
                      cap_out=None, out=None):
    """Soft-NMS of a batch's detections (the inputs and outputs of nms_segments): inside every (video, class) group the candidate with the
    largest working score among those not yet selected is selected (ties: the lower row) and the working score of every other one is decayed
    by its temporal IoU with it -- `method` 0 (linear): times 1 - iou where iou > nms_thr; 1 (gaussian): times E(iou^2 / sigma) where iou > 0
    -- until the largest is below `min_score` or `max_keep` > 0 rows are selected.  The selected rows in their input order;
    score[:, score_col] holds the final score, everything else is copied bit for bit; keep and src as nms_segments gives them (rules S1-S7 of
    cfn_hip/detections.py; soft_nms_reference spells them on the host).  sigma in [1/64, 2^20], min_score and nms_thr in [0, 1], max_keep >= 0
    (0: no limit) are host values.  Three launches, nothing is read back (capturable with out=).  out: the seven tensors and a uint8 workspace
    of soft_nms_segments_workspace_bytes(B, C, cap_in) bytes.  No gradient, no CPU path."""
    what = 'soft_nms_segments'
    B, n_classes, score_col, cap_in, cap_out, out = _nms_arguments(what, seg, frames, score, offsets, n_classes, score_col, cap_out, out,
                                                                   soft_nms_segments_workspace_bytes)
    if isinstance(method, bool) or not isinstance(method, int) or method not in (0, 1):
        raise RuntimeError('%s: method 0 (linear) or 1 (gaussian) expected, got %r' % (what, method))
    nms_thr = _host_float(what, 'nms_thr', nms_thr, 0.0, 1.0, '[0, 1]')
    sigma = _host_float(what, 'sigma', sigma, 1.0 / 64.0, float(1 << 20), '[1/64, 2^20]')
    min_score = _host_float(what, 'min_score', min_score, 0.0, 1.0, '[0, 1]')
    if isinstance(max_keep, bool) or not isinstance(max_keep, int) or not 0 <= max_keep < (1 << 31):
        raise RuntimeError('%s: max_keep: a host int >= 0 expected (0: no limit), got %r' % (what, max_keep))
    call('cfn_soft_nms_segments', seg, frames, score, offsets, out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], B, n_classes, score_col,
         nms_thr, method, sigma, min_score, max_keep, cap_in, cap_out)
    return out[:7]


# ---- temporal filtering of per-frame scores in front of the decode (csrc/scorefilter.hip; the rule, the host reference and the ScoreFilter type:
# cfn_hip/scorefilter.py) ------------------------------------------------------------------------------------------------------------------------
SCORE_FILTER_MAX_R = 32
SCORE_FILTER_TILE = 256          # frames of a row per workgroup (cfn_score_filter_tile())
SCORE_FILTER_MAX_TL = 65536


def score_filter(probs, valid_t, radius, weights, method, out=None):
    """probs (B, C, TL) fp32 on the GPU; valid_t (B,) int32; radius (C,) int32; weights (C, R + 1) fp64 with 0 <= R <= 32; method 0 (weighted
    mean) or 1 (median), a host int -> out (B, C, TL) fp32: every frame in front of valid_t replaced by the weighted mean or the median of
    its window of radius[c] frames on each side, truncated at the valid range; frames behind valid_t and classes of radius 0 copied bit for
    bit; a window with a non-finite value gives the canonical NaN (rules F1-F6 of cfn_hip/scorefilter.py; filter_reference spells them on
    the host).  One launch, no atomics, nothing is read back (no wait, capturable with out=).  out: a preallocated contiguous (B, C, TL)
    fp32 tensor (a view inside a larger buffer will do) that does not overlap probs.  No gradient, no CPU path."""
    what = 'score_filter'
    if not torch.is_tensor(probs) or probs.dtype != torch.float32 or probs.dim() != 3 or min(probs.shape) < 1:
        raise RuntimeError('%s: probs: a contiguous (B, C, TL) float32 tensor expected, got %s %s'
                           % (what, getattr(probs, 'dtype', type(probs).__name__), tuple(getattr(probs, 'shape', ()))))
    B, C, TL = (int(s) for s in probs.shape)
    if B > 65535 or C > 65535 or TL > SCORE_FILTER_MAX_TL:
        raise RuntimeError('%s: probs: B and C <= 65535 and TL <= %d expected, got (%d, %d, %d)' % (what, SCORE_FILTER_MAX_TL, B, C, TL))
    for arg, t, dt, shape in (('valid_t', valid_t, torch.int32, (B,)), ('radius', radius, torch.int32, (C,))):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape:
            raise RuntimeError('%s: %s %s %s expected, got %s %s' % (what, arg, shape, dt, getattr(t, 'dtype', type(t).__name__), tuple(getattr(t, 'shape', ()))))
    if not torch.is_tensor(weights) or weights.dtype != torch.float64 or weights.dim() != 2 or int(weights.shape[0]) != C \
            or not 1 <= int(weights.shape[1]) <= SCORE_FILTER_MAX_R + 1:
        raise RuntimeError('%s: weights: a (%d, R + 1) float64 tensor with 0 <= R <= %d expected, got %s %s'
                           % (what, C, SCORE_FILTER_MAX_R, getattr(weights, 'dtype', type(weights).__name__), tuple(getattr(weights, 'shape', ()))))
    R = int(weights.shape[1]) - 1
    if isinstance(method, bool) or not isinstance(method, int) or method not in (0, 1):
        raise RuntimeError('%s: method 0 (weighted mean) or 1 (median) expected, got %r' % (what, method))
    dev = _one_gpu(what, 'cfn_hip.scorefilter.filter_reference', probs=probs, valid_t=valid_t, radius=radius, weights=weights)
    if out is None:
        out = torch.empty(B, C, TL, dtype=torch.float32, device=dev)
    else:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (B, C, TL) or out.device != dev or not out.is_contiguous():
            raise RuntimeError('%s: out: a contiguous (%d, %d, %d) float32 tensor on %s expected, got %s %s on %s'
                               % (what, B, C, TL, dev, getattr(out, 'dtype', type(out).__name__), tuple(getattr(out, 'shape', ())), getattr(out, 'device', 'the host')))
        nbytes = B * C * TL * 4
        if out.data_ptr() < probs.data_ptr() + nbytes and probs.data_ptr() < out.data_ptr() + nbytes:
            raise RuntimeError('%s: out must not be (or overlap) probs: a window reads frames that another thread has already written' % what)
    call('cfn_score_filter', probs, valid_t, radius, weights, out, B, C, TL, R, method)
    return out


# ---- segment-level AP at temporal-IoU thresholds (csrc/segap.hip; the rule, the host reference and the meter: cfn_hip/segap.py) -------------
SEGAP_GT_TILE = 64               # ground-truth rows of a video per tile of lanes (cfn_segap_gt_tile(); more take the general path)
SEGAP_DET_TILE = 1024            # detections of a (video, class) group ordered in LDS (cfn_segap_det_tile(); more take the general path)
SEGAP_MAX_THR = 8
SEGAP_FLAG_OVERFLOW = 2


def segap_workspace_bytes(B, C, det_cap, n_seg):
    n = int(query('cfn_segap_workspace_bytes', int(B), int(C), int(det_cap), int(n_seg)))
    if n < 0:
        raise RuntimeError('segap: B and C in [1, 65535], det_cap and n_seg in [1, 2^31) expected, got (%d, %d, %d, %d)' % (B, C, det_cap, n_seg))
    return n


def _segap_dev(what, **tensors):
    return _one_gpu(what, 'cfn_hip.segap.match_reference / ap_reference', **tensors)


def segap_match(det_seg, det_score, det_offsets, seg, offsets, fps, window, tiou, n_classes, t_max, score_col=0, want_match=True, out=None):
    """Match the detections of a batch (det_seg (cap, 3) fp64, det_score (cap, 2) fp32, det_offsets (B + 1,) int32: Detections) against its
    ground truth (seg (S, 3) fp64, offsets (B + 1,) int32, fps (B,) fp64, window (B, 2) int32: SegLabels) at the thresholds tiou (n_thr,)
    fp64 on the device -> (tp (cap,) uint8: bit k = true positive at tiou[k], match (n_thr, cap) int32 = ground-truth row or -1 (None with
    want_match=False), workspace).  Rules 1-5 of cfn_hip/segap.py; one launch, nothing is read back (no wait; capturable with out=).  Only
    the rows of the batch's detections are written.  `n_classes`, `t_max` and `score_col` (0 = max, 1 = mean) are host ints.  out:
    (tp, match or None, a uint8 workspace of segap_workspace_bytes(B, C, cap, S) bytes); the workspace goes to segap_append.  No CPU path."""
    what = 'segap_match'
    dev = _segap_dev(what, det_seg=det_seg, det_score=det_score, det_offsets=det_offsets, seg=seg, offsets=offsets, fps=fps, window=window, tiou=tiou)
    if det_seg.dtype != torch.float64 or det_seg.dim() != 2 or det_seg.shape[1] != 3 or det_seg.shape[0] < 1:
        raise RuntimeError('%s: det_seg: a (cap, 3) float64 tensor with cap >= 1 expected, got %s %s' % (what, det_seg.dtype, tuple(det_seg.shape)))
    cap = int(det_seg.shape[0])
    if det_score.dtype != torch.float32 or tuple(det_score.shape) != (cap, 2):
        raise RuntimeError('%s: det_score (%d, 2) float32 expected, got %s %s' % (what, cap, det_score.dtype, tuple(det_score.shape)))
    if seg.dtype != torch.float64 or seg.dim() != 2 or seg.shape[1] != 3 or seg.shape[0] < 1:
        raise RuntimeError('%s: seg: a (S, 3) float64 tensor with S >= 1 expected, got %s %s' % (what, seg.dtype, tuple(seg.shape)))
    S = int(seg.shape[0])
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
        raise RuntimeError('%s: offsets (B + 1,) int32 expected, got %s %s' % (what, offsets.dtype, tuple(offsets.shape)))
    B = int(offsets.numel()) - 1
    if det_offsets.dtype != torch.int32 or tuple(det_offsets.shape) != (B + 1,):
        raise RuntimeError('%s: det_offsets (%d,) int32 expected (one batch size for detections and ground truth), got %s %s'
                           % (what, B + 1, det_offsets.dtype, tuple(det_offsets.shape)))
    if fps.dtype != torch.float64 or tuple(fps.shape) != (B,) or window.dtype != torch.int32 or tuple(window.shape) != (B, 2):
        raise RuntimeError('%s: fps (%d,) float64 and window (%d, 2) int32 expected, got %s %s and %s %s'
                           % (what, B, B, fps.dtype, tuple(fps.shape), window.dtype, tuple(window.shape)))
    if tiou.dtype != torch.float64 or tiou.dim() != 1 or not 1 <= tiou.numel() <= SEGAP_MAX_THR:
        raise RuntimeError('%s: tiou: 1 to %d float64 thresholds expected, got %s %s' % (what, SEGAP_MAX_THR, tiou.dtype, tuple(tiou.shape)))
    n_thr, n_classes, t_max, score_col = int(tiou.numel()), int(n_classes), int(t_max), int(score_col)
    if n_classes < 1 or t_max < 1 or score_col not in (0, 1):
        raise RuntimeError('%s: n_classes >= 1, t_max >= 1 and score_col 0 (max) or 1 (mean) expected, got %d, %d, %d' % (what, n_classes, t_max, score_col))
    ws_bytes = segap_workspace_bytes(B, n_classes, cap, S)
    if out is None:
        out = (torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(n_thr, cap, dtype=torch.int32, device=dev) if want_match else None,
               torch.empty(ws_bytes, dtype=torch.uint8, device=dev))
    else:
        out = tuple(out)
        if len(out) != 3 or out[0].dtype != torch.uint8 or tuple(out[0].shape) != (cap,) or not out[0].is_contiguous() \
                or (out[1] is not None and (out[1].dtype != torch.int32 or tuple(out[1].shape) != (n_thr, cap) or not out[1].is_contiguous())) \
                or out[2].dtype != torch.uint8 or out[2].dim() != 1 or out[2].numel() < ws_bytes or out[2].data_ptr() % 8 or not out[2].is_contiguous():
            raise RuntimeError('%s: out: tp (%d,) uint8, match (%d, %d) int32 or None and an 8-byte aligned uint8 workspace of >= %d bytes expected'
                               % (what, cap, n_thr, cap, ws_bytes))
    call('cfn_segap_match', det_seg, det_score, det_offsets, seg, offsets, fps, window, tiou, out[0], out[1], out[2], B, n_classes, t_max, n_thr,
         score_col, cap, S)
    return out


def _segap_stores(what, scores, tps, counts, n_gt):
    _segap_dev(what, scores=scores, tps=tps, counts=counts, n_gt=n_gt)
    if scores.dtype != torch.float32 or scores.dim() != 2 or min(scores.shape) < 1 or tps.dtype != torch.uint8 or tuple(tps.shape) != tuple(scores.shape):
        raise RuntimeError('%s: class-major stores expected, scores (C, cap) fp32 and tps (C, cap) uint8; got %s %s, %s %s'
                           % (what, scores.dtype, tuple(scores.shape), tps.dtype, tuple(tps.shape)))
    C, cap = int(scores.shape[0]), int(scores.shape[1])
    for name, t in (('counts', counts), ('n_gt', n_gt)):
        if t.dtype != torch.int32 or tuple(t.shape) != (C,):
            raise RuntimeError('%s: %s (%d,) int32 expected, got %s %s' % (what, name, C, t.dtype, tuple(t.shape)))
    return C, cap


def segap_append(det_score, tp, workspace, scores, tps, counts, n_gt, flags, batch, score_col=0):
    """Rule 6 of cfn_hip/segap.py behind segap_match of the same batch (its tp and workspace): class c's rows of scores (C, cap) fp32 / tps
    (C, cap) uint8 receive the batch's detections of class c in (video, row) order; counts (C,) and n_gt (C,) int32 advance.  A batch that
    would push any class past cap writes nothing, changes no count and sets SEGAP_FLAG_OVERFLOW in flags (one int32).  In place, two
    launches, nothing is read back (capturable).  `batch` = B of the match."""
    what = 'segap_append'
    C, cap = _segap_stores(what, scores, tps, counts, n_gt)
    _segap_dev(what, det_score=det_score, tp=tp, workspace=workspace, flags=flags, scores=scores)
    dcap = int(tp.numel())
    if tp.dtype != torch.uint8 or tp.dim() != 1 or det_score.dtype != torch.float32 or tuple(det_score.shape) != (dcap, 2):
        raise RuntimeError('%s: tp (cap,) uint8 and det_score (cap, 2) float32 expected, got %s %s and %s %s'
                           % (what, tp.dtype, tuple(tp.shape), det_score.dtype, tuple(det_score.shape)))
    if flags.dtype != torch.int32 or flags.numel() != 1:
        raise RuntimeError('%s: flags must be one int32 on the device' % what)
    need = segap_workspace_bytes(int(batch), C, dcap, 1)
    if workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.numel() < need or workspace.data_ptr() % 8:
        raise RuntimeError('%s: workspace: the 8-byte aligned uint8 tensor segap_match filled (>= %d bytes) expected' % (what, need))
    call('cfn_segap_append', det_score, tp, workspace, scores, tps, counts, n_gt, flags, int(batch), C, int(score_col), dcap, cap)


def segap_value(scores, tps, counts, n_gt, n_thr, out=None):
    """Rule 7 of cfn_hip/segap.py: class-major stores -> (ap (n_thr, C) fp32, map (n_thr,) fp32) on the device: the stable descending sort of
    ap_sort with one count per class and the tp byte as the payload, then the reduction.  Nothing is read back.  out = (sorted_scores,
    sorted_tps, tmp_keys int32, tmp_tps, ap, map): buffers to reuse."""
    what = 'segap_value'
    C, cap = _segap_stores(what, scores, tps, counts, n_gt)
    n_thr = int(n_thr)
    if not 1 <= n_thr <= SEGAP_MAX_THR:
        raise RuntimeError('%s: n_thr in [1, %d] expected, got %d' % (what, SEGAP_MAX_THR, n_thr))
    dev = scores.device
    if out is None:
        out = (torch.empty_like(scores), torch.empty_like(tps), torch.empty(C, cap, dtype=torch.int32, device=dev), torch.empty_like(tps),
               torch.empty(n_thr, C, dtype=torch.float32, device=dev), torch.empty(n_thr, dtype=torch.float32, device=dev))
    ss, st, tk, tt, ap, mp = out
    for x, shp, dt in ((ss, (C, cap), torch.float32), (st, (C, cap), torch.uint8), (tk, (C, cap), torch.int32), (tt, (C, cap), torch.uint8),
                       (ap, (n_thr, C), torch.float32), (mp, (n_thr,), torch.float32)):
        if tuple(x.shape) != shp or x.dtype != dt or x.device != dev or not x.is_contiguous():
            raise RuntimeError('%s: out: sorted scores, sorted tps, tmp keys (int32), tmp tps of shape %s, ap %s and map %s fp32 on %s expected'
                               % (what, (C, cap), (n_thr, C), (n_thr,), dev))
    call('cfn_ap_sort_counts', scores, tps, counts, ss, st, tk, tt, C, cap)
    call('cfn_segap_reduce', st, counts, n_gt, ap, mp, C, n_thr, cap)
    return ap, mp


# ---- proposal recall at N per video, AR@N (csrc/segrecall.hip; the rule, the host reference and the meter: cfn_hip/recall.py) ----------------
SEG_RECALL_MAX_THR = 16
SEG_RECALL_MAX_N = 1024
SEG_RECALL_RANK_TILE = 256       # scores of a video per LDS tile of the rank kernel (cfn_seg_recall_rank_tile())


def seg_recall_workspace_bytes(B, C, det_cap, n_seg, n_thr):
    n = int(query('cfn_seg_recall_workspace_bytes', int(B), int(C), int(det_cap), int(n_seg), int(n_thr)))
    if n < 0:
        raise RuntimeError('seg_recall: B and C in [1, 65535], det_cap and n_seg in [1, 2^31) and n_thr in [1, %d] expected, got (%d, %d, %d, %d, %d)'
                           % (SEG_RECALL_MAX_THR, B, C, det_cap, n_seg, n_thr))
    return n


def seg_recall_state_size(n_thr, n_max):
    """int64 values of a recall state: hist (n_thr, n_max), n_gt, n_videos, n_props"""
    return int(n_thr) * int(n_max) + 3


def _seg_recall_state(what, state, n_thr, n_max):
    if not 1 <= n_thr <= SEG_RECALL_MAX_THR or not 1 <= n_max <= SEG_RECALL_MAX_N:
        raise RuntimeError('%s: n_thr in [1, %d] and n_max in [1, %d] expected, got %d and %d' % (what, SEG_RECALL_MAX_THR, SEG_RECALL_MAX_N, n_thr, n_max))
    if state.dtype != torch.int64 or tuple(state.shape) != (seg_recall_state_size(n_thr, n_max),):
        raise RuntimeError('%s: state: (%d,) int64 expected (hist (%d, %d), n_gt, n_videos, n_props), got %s %s'
                           % (what, seg_recall_state_size(n_thr, n_max), n_thr, n_max, state.dtype, tuple(state.shape)))


def seg_recall_add(det_seg, det_score, det_offsets, seg, offsets, fps, window, tiou, state, n_classes, t_max, n_max, score_col=0, out=None):
    """One batch into a proposal-recall state (rules R1-R5 of cfn_hip/recall.py): detections (det_seg (cap, 3) fp64, det_score (cap, 2) fp32,
    det_offsets (B + 1,) int32) against the ground truth (seg (S, 3) fp64, offsets (B + 1,) int32, fps (B,) fp64, window (B, 2) int32) at
    tiou (n_thr,) fp64 on the device, 1 <= n_thr <= 16 -> hit (n_thr, S) int32: the video rank of the first candidate of the row's video and
    class that reaches tiou[k], n_max when none of the n_max best does, -1 for a row that does not participate.  state (n_thr * n_max + 3,)
    int64 advances in place.  Three launches, nothing is read back (capturable with out=).  `n_classes`, `t_max`, `n_max` (1 .. 1024) and
    `score_col` (0 = max, 1 = mean) are host ints.  out: (hit, a uint8 workspace of seg_recall_workspace_bytes(B, C, cap, S, n_thr) bytes).
    No CPU path."""
    what = 'seg_recall_add'
    dev = _one_gpu(what, 'cfn_hip.recall.recall_reference', det_seg=det_seg, det_score=det_score, det_offsets=det_offsets, seg=seg, offsets=offsets,
                   fps=fps, window=window, tiou=tiou, state=state)
    if det_seg.dtype != torch.float64 or det_seg.dim() != 2 or det_seg.shape[1] != 3 or det_seg.shape[0] < 1:
        raise RuntimeError('%s: det_seg: a (cap, 3) float64 tensor with cap >= 1 expected, got %s %s' % (what, det_seg.dtype, tuple(det_seg.shape)))
    cap = int(det_seg.shape[0])
    if det_score.dtype != torch.float32 or tuple(det_score.shape) != (cap, 2):
        raise RuntimeError('%s: det_score (%d, 2) float32 expected, got %s %s' % (what, cap, det_score.dtype, tuple(det_score.shape)))
    if seg.dtype != torch.float64 or seg.dim() != 2 or seg.shape[1] != 3 or seg.shape[0] < 1:
        raise RuntimeError('%s: seg: a (S, 3) float64 tensor with S >= 1 expected, got %s %s' % (what, seg.dtype, tuple(seg.shape)))
    S = int(seg.shape[0])
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
        raise RuntimeError('%s: offsets (B + 1,) int32 expected, got %s %s' % (what, offsets.dtype, tuple(offsets.shape)))
    B = int(offsets.numel()) - 1
    if det_offsets.dtype != torch.int32 or tuple(det_offsets.shape) != (B + 1,):
        raise RuntimeError('%s: det_offsets (%d,) int32 expected (one batch size for detections and ground truth), got %s %s'
                           % (what, B + 1, det_offsets.dtype, tuple(det_offsets.shape)))
    if fps.dtype != torch.float64 or tuple(fps.shape) != (B,) or window.dtype != torch.int32 or tuple(window.shape) != (B, 2):
        raise RuntimeError('%s: fps (%d,) float64 and window (%d, 2) int32 expected, got %s %s and %s %s'
                           % (what, B, B, fps.dtype, tuple(fps.shape), window.dtype, tuple(window.shape)))
    if tiou.dtype != torch.float64 or tiou.dim() != 1 or not 1 <= tiou.numel() <= SEG_RECALL_MAX_THR:
        raise RuntimeError('%s: tiou: 1 to %d float64 thresholds expected, got %s %s' % (what, SEG_RECALL_MAX_THR, tiou.dtype, tuple(tiou.shape)))
    n_thr, n_classes, t_max, n_max, score_col = int(tiou.numel()), int(n_classes), int(t_max), int(n_max), int(score_col)
    if n_classes < 1 or t_max < 1 or score_col not in (0, 1):
        raise RuntimeError('%s: n_classes >= 1, t_max >= 1 and score_col 0 (max) or 1 (mean) expected, got %d, %d, %d' % (what, n_classes, t_max, score_col))
    _seg_recall_state(what, state, n_thr, n_max)
    ws_bytes = seg_recall_workspace_bytes(B, n_classes, cap, S, n_thr)
    if out is None:
        out = (torch.empty(n_thr, S, dtype=torch.int32, device=dev), torch.empty(ws_bytes, dtype=torch.uint8, device=dev))
    else:
        out = tuple(out)
        if len(out) != 2 or out[0].dtype != torch.int32 or tuple(out[0].shape) != (n_thr, S) or not out[0].is_contiguous() or out[0].device != dev \
                or out[1].dtype != torch.uint8 or out[1].dim() != 1 or out[1].numel() < ws_bytes or out[1].data_ptr() % 8 or not out[1].is_contiguous() \
                or out[1].device != dev:
            raise RuntimeError('%s: out: hit (%d, %d) int32 and an 8-byte aligned uint8 workspace of >= %d bytes on %s expected' % (what, n_thr, S, ws_bytes, dev))
    call('cfn_seg_recall_add', det_seg, det_score, det_offsets, seg, offsets, fps, window, tiou, out[0], state, out[1], B, n_classes, t_max, n_thr,
         n_max, score_col, cap, S)
    return out[0]


def seg_recall_value(state, n_thr, n_max, out=None):
    """Rule R6 of cfn_hip/recall.py: a recall state -> (n_thr * n_max + n_max + 2,) fp64 on the device: recall (n_thr, n_max), ar (n_max,), auc,
    avg_props.  One launch, nothing is read back.  out: the tensor to fill."""
    what = 'seg_recall_value'
    n_thr, n_max = int(n_thr), int(n_max)
    dev = _one_gpu(what, 'cfn_hip.recall.recall_from_state', state=state)
    _seg_recall_state(what, state, n_thr, n_max)
    n = n_thr * n_max + n_max + 2
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (n,) or out.device != dev or not out.is_contiguous():
        raise RuntimeError('%s: out: (%d,) float64 on %s expected' % (what, n, dev))
    call('cfn_seg_recall_value', state, out, n_thr, n_max)
    return out


# ---- baseline JPEG frames decoded on the GPU (csrc/jpegdec.hip; the host side and the batch type: cfn_hip/jpegdec.py) ------------------------
def jpeg_workspace_bytes(rows, slots, lanes, blocks_max, entropy=None, sub_bytes=None, max_subs=None):
    """bytes of workspace cfn_jpeg_decode_u8 needs for `rows` frames into `slots` = clips x Tmax frame slots.  entropy, sub_bytes,
    max_subs: as jpeg_decode_u8 takes them; they are checked, and the sync mode needs no more (its records live in LDS)"""
    from . import jpegdec
    if jpegdec.entropy_mode(entropy) == 'sync' or sub_bytes is not None or max_subs is not None:
        jpegdec.check_sync_sizes(sub_bytes, max_subs)
    n = int(query('cfn_jpeg_workspace_bytes', int(rows), int(slots), int(lanes), int(blocks_max)))
    if n < 0:
        raise RuntimeError('jpeg_decode_u8: bad sizes (%d frames, %d slots, %d lanes, %d blocks)' % (rows, slots, lanes, blocks_max))
    return n


def jpeg_decode_u8(jpeg_clips, out=None, status=None, workspace=None, entropy=None, sub_bytes=None, max_subs=None):
    """a cfn_hip.jpegdec.JpegClips batch on the GPU -> its frames (N, Tmax, Hmax, Wmax, 3) uint8, N = all clips of the batch: what PIL
    decodes, bit for bit, each picture in the top-left corner, zero bytes elsewhere (RawU8Clips.frames as collate._pad_raw_u8 builds
    them).  On the current stream; nothing is read back: sizes come from the batch's host-side `dims`.
    out: preallocated frames, every byte is written.  status: (R,) int32, one word per row of `frames`, zeroed and set by the kernels
    (0 = decoded; jpegdec.check_status raises on anything else); with status=None the words are dropped -- pass one to learn of a bad
    frame.  workspace: a uint8 device buffer of at least jpeg_workspace_bytes(...) (allocated per call otherwise).  No CPU path.
    entropy: None / 'interval' = one lane per (frame, restart interval), cfn_jpeg_decode_u8; 'sync' = cfn_jpeg_decode_u8_sync: a frame
    without restart markers that is longer than `sub_bytes` (a multiple of 4 in [16, 1024], default jpegdec.SYNC_SUB_BYTES) and has at
    most `max_subs` (<= jpegdec.SYNC_MAX_SUBS, default jpegdec.SYNC_DEFAULT_MAX_SUBS) subsequences of that size is decoded by one workgroup, a lane per
    subsequence; every other frame as before.  The same bytes either way.  The environment is NOT read here (JpegClips.decode does)."""
    from . import jpegdec
    if entropy not in (None,) + jpegdec.ENTROPY_MODES:
        raise ValueError("jpeg_decode_u8: entropy: None, 'interval' or 'sync' expected, got %r" % (entropy,))
    sync = entropy == 'sync'
    if sync or sub_bytes is not None or max_subs is not None:
        sub_bytes, max_subs = jpegdec.check_sync_sizes(sub_bytes, max_subs)
        if not sync:
            raise ValueError("jpeg_decode_u8: sub_bytes / max_subs belong to entropy='sync', got entropy=%r" % (entropy,))
    jc = jpeg_clips
    if not (hasattr(jc, '_fields') and jc._fields[:6] == ('data', 'frames', 'tables', 'geom', 'lengths', 'box')):
        raise RuntimeError('jpeg_decode_u8: a JpegClips batch expected, got %s' % type(jc).__name__)
    data, frames, tables = jc.data, jc.frames, jc.tables
    geom, lengths = jc.geom.reshape(-1, 4), jc.lengths.reshape(-1)
    T, H, W, lanes, blocks_max = (int(d) for d in jc.dims)
    if data.dtype != torch.uint8 or data.dim() != 1 or data.numel() < 1:
        raise RuntimeError('jpeg_decode_u8: data: a flat uint8 buffer expected, got %s %s' % (data.dtype, tuple(data.shape)))
    if frames.dim() != 2 or frames.shape[1] != 8 or frames.shape[0] < 1:
        raise RuntimeError('jpeg_decode_u8: frames (R, 8) int32 expected, got %s %s' % (frames.dtype, tuple(frames.shape)))
    if tables.dim() != 2 or tables.shape[1] != 3456 or tables.shape[0] < 1:
        raise RuntimeError('jpeg_decode_u8: tables (S, 3456) int32 expected, got %s %s' % (tables.dtype, tuple(tables.shape)))
    N, R = int(lengths.numel()), int(frames.shape[0])
    if geom.shape[0] != N:
        raise RuntimeError('jpeg_decode_u8: one geometry per clip expected: %d clips, geom %s' % (N, tuple(jc.geom.shape)))
    dev = data.device
    if out is None:
        out = torch.empty(N, T, H, W, 3, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.numel() != N * T * H * W * 3 or tuple(out.shape[-4:]) != (T, H, W, 3) or not out.is_contiguous():
        raise RuntimeError('jpeg_decode_u8: out: a contiguous uint8 tensor (..., %d, %d, %d, 3) of %d clips expected, got %s %s'
                           % (T, H, W, N, out.dtype, tuple(out.shape)))
    if status is None:
        status = torch.empty(R, dtype=torch.int32, device=dev)
    elif status.dtype != torch.int32 or status.numel() != R or not status.is_contiguous():
        raise RuntimeError('jpeg_decode_u8: status: %d contiguous int32 words expected, got %s %s' % (R, status.dtype, tuple(status.shape)))
    need = jpeg_workspace_bytes(R, N * T, lanes, blocks_max)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise RuntimeError('jpeg_decode_u8: workspace: a contiguous uint8 buffer of at least %d bytes expected, got %s %s'
                           % (need, workspace.dtype, tuple(workspace.shape)))
    args = (data.contiguous(), frames.contiguous(), tables.contiguous(), geom.contiguous(), lengths.contiguous(), out, status, workspace,
            int(workspace.numel()), int(data.numel()), R, int(tables.shape[0]), N, T, H, W, lanes, blocks_max)
    if sync:
        call('cfn_jpeg_decode_u8_sync', *(args + (sub_bytes, max_subs)))
    else:
        call('cfn_jpeg_decode_u8', *args)
    return out.view(N, T, H, W, 3)
