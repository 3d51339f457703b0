"""The kernels as registered torch operators (namespace ``cfn``): ``torch.ops.cfn.dwconv3d``, ``torch.ops.cfn.pwconv``,
``torch.ops.cfn.time_sample`` and the rest of the operator tuples below, so that ``torch.compile`` / ``torch.export`` see them as
opaque nodes instead of graph-breaking on ctypes calls.

    import cfn_hip.torchlib            # loads the operator library and completes the registrations
    y, s, q = torch.ops.cfn.dwconv3d(x, w, A, B, act, stride)

Every operator is defined and implemented once, in C++: csrc/torch/cfn_torch.cpp -> cfn_hip/libcfn_torch.so (``TORCH_LIBRARY``, built by
``__graft_entry__.build()``) holds the schemas and the CUDA (= HIP) kernels, which call the C-ABI entry points of include/cfn_hip.h.  This
module loads that library and attaches what has to be Python: the fake (meta) implementations and the autograd formulas.  It also holds the
operator-name tuples and ``TorchOps``, the ``cfn_hip.ops``-shaped facade over the operators.  There is no Python implementation of any
operator: without the library the import raises.

The drop-in modules (x3d_fine / x3d_coarse) keep calling ``cfn_hip.ops`` directly: its autograd Functions carry the cross-op
fusions (shortcut tokens, tail links, batched gradient casts) that a functional op signature cannot express, and skip the
dispatcher's per-call cost (~1100 launches per step).  The operators here are the same C-ABI entry points with plain semantics:

* ``cfn::dwconv3d(x, w, A?, B?, act, stride) -> (y, sum, sumsq)``   depthwise 3x3x3, pad 1, stride (1,s,s), input read through
  the prologue act(A x + B); per-(n,c) fp64 statistics of y              (x3d_fine.py:89-97 conv3x3x3 + the BN that follows)
* ``cfn::pwconv(x, w, A?, B?, act, stride) -> (y, sum, sumsq)``     1x1x1 conv, same conventions      (x3d_fine.py:100-105)
* ``cfn::time_sample(x, cdf) -> out``                                Grid Pool / Unpool resampler      (x3d_coarse.py:394-416)

No CPU implementation is registered: calling them with CPU tensors fails in the dispatcher.
"""
import os

import torch

from . import load, ACT_NONE

_HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE_LIB = os.path.join(_HERE, 'libcfn_torch.so')      # (C++ consumers load the same file: INTEGRATION.md 3b)


def _require_default_kernels(default=os.path.join(_HERE, 'libcfn_hip.so')):
    """libcfn_torch.so is linked against the in-tree libcfn_hip.so (rpath $ORIGIN).  With a variant selected, cfn_hip.ops would run the variant
    and torch.ops.cfn.* the default build, each with its own workspaces, profiler tables and deterministic-mode state: refuse."""
    variant = os.environ.get('CFN_HIP_LIB')
    if variant and os.path.realpath(variant) != os.path.realpath(default):
        raise RuntimeError('CFN_HIP_LIB=%s selects a variant build of the kernels, but the operator library is linked against the default '
                           'build (%s): variant builds serve the cfn_hip.ops route only, not cfn_hip.torchlib / torch.ops.cfn.*' % (variant, default))


def _require_library(path):
    if not os.path.exists(path):
        raise RuntimeError('libcfn_torch.so not found at %s -- run `python __graft_entry__.py` (hipcc, gfx950) first; '
                           'there is no Python fallback for the torch.ops.cfn operators' % path)


_require_default_kernels()
_require_library(NATIVE_LIB)
load()                                   # libcfn_hip.so first: the operator library is linked against it
torch.ops.load_library(NATIVE_LIB)


class _NativeOp(object):
    """module-level handle of an operator that the TORCH_LIBRARY block defines: callable, and the place to attach the Python registrations"""

    def __init__(self, qualname):
        self.qualname = qualname
        ns, name = qualname.split('::')
        self._op = getattr(getattr(torch.ops, ns), name)

    def __call__(self, *a, **k):
        return self._op(*a, **k)

    def register_fake(self, fn):
        torch.library.register_fake(self.qualname)(fn)
        return fn

    def register_autograd(self, backward, setup_context=None):
        torch.library.register_autograd(self.qualname, backward, setup_context=setup_context)


def _op(name):
    return _NativeOp('cfn::' + name)


def _z(ref, dtype=torch.float32):
    """placeholder for "no tensor" in an operator result (results may not be None)"""
    return ref.new_zeros(1, dtype=dtype)


def _gz(g, like, dtype=None):
    """incoming gradient or zeros (autograd passes None for unused outputs)"""
    return torch.zeros_like(like, dtype=dtype or like.dtype) if g is None else g


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise 3x3x3
# ---------------------------------------------------------------------------------------------------------------------------
dwconv3d = _op('dwconv3d')


@dwconv3d.register_fake
def _(x, w, A=None, B=None, act=0, stride=1):
    N, C, T, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (x.new_empty(N, C, T, Ho, Wo), x.new_empty(N, C, dtype=torch.float64), x.new_empty(N, C, dtype=torch.float64))


dwconv3d_backward = _op('dwconv3d_backward')      # -> (gx, gw, gA, gB); gA / gB are zeros (1 element) when there is no prologue


@dwconv3d_backward.register_fake
def _(gy, gs, gq, x, w, y, A=None, B=None, act=0, stride=1):
    n = (x.shape[0], x.shape[1]) if A is not None else (1,)
    return (torch.empty_like(x), torch.empty_like(w, dtype=torch.float32), x.new_empty(n, dtype=torch.float32),
            x.new_empty(n, dtype=torch.float32))


def _dw_setup(ctx, inputs, output):
    x, w, A, B, act, stride = inputs
    y, _, _ = output
    ctx.save_for_backward(x, w, y, A, B)
    ctx.act, ctx.stride = act, stride


def _dw_backward(ctx, gy, gs, gq):
    x, w, y, A, B = ctx.saved_tensors
    gy = torch.zeros_like(y) if gy is None else gy
    gs = torch.zeros(y.shape[:2], dtype=torch.float64, device=y.device) if gs is None else gs
    gq = torch.zeros(y.shape[:2], dtype=torch.float64, device=y.device) if gq is None else gq
    gx, gw, gA, gB = torch.ops.cfn.dwconv3d_backward(gy, gs, gq, x, w, y, A, B, ctx.act, ctx.stride)
    return gx, gw, (gA if A is not None else None), (gB if B is not None else None), None, None


dwconv3d.register_autograd(_dw_backward, setup_context=_dw_setup)


# ---------------------------------------------------------------------------------------------------------------------------
# pointwise 1x1x1 (fp32 tensors; the bf16 pointwise path is reached through cfn_hip.ops)
# ---------------------------------------------------------------------------------------------------------------------------
pwconv = _op('pwconv')


@pwconv.register_fake
def _(x, w, A=None, B=None, act=0, stride=1):
    N, Cin, T, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (x.new_empty(N, w.shape[0], T, Ho, Wo), x.new_empty(N, w.shape[0], dtype=torch.float64),
            x.new_empty(N, w.shape[0], dtype=torch.float64))


pwconv_backward = _op('pwconv_backward')


@pwconv_backward.register_fake
def _(gy, gs, gq, x, w, y, A=None, B=None, act=0, stride=1):
    n = (x.shape[0], x.shape[1]) if A is not None else (1,)
    return (torch.empty_like(x), torch.empty_like(w, dtype=torch.float32), x.new_empty(n, dtype=torch.float32),
            x.new_empty(n, dtype=torch.float32))


def _pw_backward(ctx, gy, gs, gq):
    x, w, y, A, B = ctx.saved_tensors
    gy = torch.zeros_like(y) if gy is None else gy
    gs = torch.zeros(y.shape[:2], dtype=torch.float64, device=y.device) if gs is None else gs
    gq = torch.zeros(y.shape[:2], dtype=torch.float64, device=y.device) if gq is None else gq
    gx, gw, gA, gB = torch.ops.cfn.pwconv_backward(gy, gs, gq, x, w, y, A, B, ctx.act, ctx.stride)
    return gx, gw, (gA if A is not None else None), (gB if B is not None else None), None, None


pwconv.register_autograd(_pw_backward, setup_context=_dw_setup)


# ---------------------------------------------------------------------------------------------------------------------------
# Grid Pool / Grid Unpool resampler
# ---------------------------------------------------------------------------------------------------------------------------
time_sample = _op('time_sample')


@time_sample.register_fake
def _(x, cdf):
    return x.new_empty((x.shape[0], x.shape[1], cdf.shape[1]) + tuple(x.shape[3:]))


time_sample_backward = _op('time_sample_backward')


@time_sample_backward.register_fake
def _(g, x, cdf):
    return torch.empty_like(x), torch.empty_like(cdf)


def _ts_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _ts_backward(ctx, g):
    x, cdf = ctx.saved_tensors
    return torch.ops.cfn.time_sample_backward(g, x, cdf)


time_sample.register_autograd(_ts_backward, setup_context=_ts_setup)


# ---------------------------------------------------------------------------------------------------------------------------
# The rest of the operator set.  Each operator runs the same C-ABI entry points as the autograd Function of cfn_hip.ops, behind a
# dispatcher schema + fake (meta) implementation + registered autograd formula.  Plain semantics: no ShortcutToken / TailLink /
# lazily cast gradients.  Coefficients (A, B) may be fp32 or fp64 (the C ABI takes fp64); their gradients come back in the dtype
# of the input.
# ---------------------------------------------------------------------------------------------------------------------------

# ---- conv1_t: depthwise 5x1x1 ------------------------------------------------------------------------------------------------
dwconv_t5 = _op('dwconv_t5')


@dwconv_t5.register_fake
def _(x, w):
    return torch.empty_like(x), x.new_empty(x.shape[:2], dtype=torch.float64), x.new_empty(x.shape[:2], dtype=torch.float64)


dwconv_t5_backward = _op('dwconv_t5_backward')


@dwconv_t5_backward.register_fake
def _(gy, gs, gq, x, w, y):
    return torch.empty_like(x), torch.empty_like(w, dtype=torch.float32)


def _t5_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[0])


def _t5_backward(ctx, gy, gs, gq):
    x, w, y = ctx.saved_tensors
    f64 = lambda g: torch.zeros(y.shape[:2], dtype=torch.float64, device=y.device) if g is None else g
    return torch.ops.cfn.dwconv_t5_backward(_gz(gy, y), f64(gs), f64(gq), x, w, y)


dwconv_t5.register_autograd(_t5_backward, setup_context=_t5_setup)


# ---- conv1_s: dense 1x3x3 stem conv (the clip gets no gradient) ----------------------------------------------------------------
stem_conv = _op('stem_conv')


@stem_conv.register_fake
def _(x, w):
    N, _, T, H, W = x.shape
    return x.new_empty(N, w.shape[0], T, (H - 1) // 2 + 1, (W - 1) // 2 + 1)


stem_conv_backward = _op('stem_conv_backward')


@stem_conv_backward.register_fake
def _(gy, x, w):
    return torch.empty_like(w, dtype=torch.float32)


stem_conv.register_autograd(lambda ctx, gy: (None, torch.ops.cfn.stem_conv_backward(gy, *ctx.saved_tensors)),
                            setup_context=lambda ctx, inputs, output: ctx.save_for_backward(*inputs))


# ---- uint8 frames, normalised on the GPU: the table (host), the converter, conv1_s on the bytes (no clip gradient) ----------------
clip_lut = _op('clip_lut')      # (no tensor argument: one composite kernel for every dispatch key, no fake implementation needed)
clip_u8_to_f32 = _op('clip_u8_to_f32')


@clip_u8_to_f32.register_fake
def _(frames, lut, lengths=None):
    N, T, H, W, _ = frames.shape
    return frames.new_empty((N, 3, T, H, W), dtype=torch.float32)


stem_conv_u8 = _op('stem_conv_u8')


@stem_conv_u8.register_fake
def _(frames, lengths, lut, w):
    N, T, H, W, _ = frames.shape
    return w.new_empty((N, w.shape[0], T, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32)


stem_conv_u8_backward = _op('stem_conv_u8_backward')


@stem_conv_u8_backward.register_fake
def _(gy, frames, lengths, lut, w):
    return torch.empty_like(w, dtype=torch.float32)


def _su8_setup(ctx, inputs, output):
    frames, lengths, lut, w = inputs
    ctx.has_len = lengths is not None
    ctx.save_for_backward(*([frames, lut, w] + ([lengths] if ctx.has_len else [])))


def _su8_backward(ctx, gy):
    frames, lut, w = ctx.saved_tensors[:3]
    lengths = ctx.saved_tensors[3] if ctx.has_len else None
    return None, None, None, torch.ops.cfn.stem_conv_u8_backward(gy, frames, lengths, lut, w)


stem_conv_u8.register_autograd(_su8_backward, setup_context=_su8_setup)


# ---- dense conv3d (Grid Pool saliency convs) -------------------------------------------------------------------------------------
conv3d_dense = _op('conv3d_dense')


@conv3d_dense.register_fake
def _(x, w, kernel, stride, padding, A=None, B=None, act=0):
    N, _, T, H, W = x.shape
    o = [(d + 2 * p - k) // s + 1 for d, k, s, p in zip((T, H, W), kernel, stride, padding)]
    return (x.new_empty(N, w.shape[0], *o), x.new_empty(N, w.shape[0], dtype=torch.float64), x.new_empty(N, w.shape[0], dtype=torch.float64))


conv3d_dense_backward = _op('conv3d_dense_backward')


@conv3d_dense_backward.register_fake
def _(gy, gs, gq, x, w, y, kernel, stride, padding, A=None, B=None, act=0):
    ab = (lambda t: torch.empty_like(t)) if A is not None else (lambda t: x.new_empty(1))
    return torch.empty_like(x), torch.empty_like(w, dtype=torch.float32), ab(A), ab(B)


def _cd_setup(ctx, inputs, output):
    x, w, kernel, stride, padding, A, B, act = inputs
    ctx.save_for_backward(x, w, output[0], A, B)
    ctx.geom = (kernel, stride, padding, act)


def _cd_backward(ctx, gy, gs, gq):
    x, w, y, A, B = ctx.saved_tensors
    kernel, stride, padding, act = ctx.geom
    f64 = lambda g: torch.zeros(y.shape[:2], dtype=torch.float64, device=y.device) if g is None else g
    gx, gw, gA, gB = torch.ops.cfn.conv3d_dense_backward(_gz(gy, y), f64(gs), f64(gq), x, w, y, kernel, stride, padding, A, B, act)
    return gx, gw, None, None, None, (gA if A is not None else None), (gB if B is not None else None), None


conv3d_dense.register_autograd(_cd_backward, setup_context=_cd_setup)


# ---- SubBatchNorm3d statistics -> prologue coefficients (+ SE gate) ---------------------------------------------------------------
# bn_fold -> [A, B, mean, rstd, A0, B0, gate, hbuf, pooled, new_run_mean, new_run_var, new_nbt].  FUNCTIONAL: the running statistics
# are returned, not updated in place (a dispatcher operator with an autograd formula may not mutate its arguments); the caller
# copies them into its buffers (x3d_fine.SubBatchNorm3d.fold does).  A0 .. pooled are 1-element placeholders without an SE branch.
bn_fold = _op('bn_fold')


@bn_fold.register_fake
def _(s, q, gamma, beta, run_mean, run_var, nbt, training, N, C, S, count, eps, momentum, w1=None, b1=None, w2=None, b2=None,
      pool_count=1.0):
    dev = run_mean.device
    f64 = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
    f32 = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    Se = S if training else 1
    new = [torch.empty_like(run_mean), torch.empty_like(run_var), torch.empty_like(nbt)]
    if w1 is None:
        return [f64(N, C), f64(N, C), f64(Se, C), f64(Se, C)] + [f32(1) for _ in range(5)] + new
    return [f64(N, C), f64(N, C), f64(Se, C), f64(Se, C), f32(N, C), f32(N, C), f32(N, C), f32(N, w1.shape[0]), f32(N, C)] + new


# -> [gs, gq, ggamma, gbeta, gw1, gb1, gw2, gb2] (1-element placeholders where there is nothing)
bn_fold_backward = _op('bn_fold_backward')


@bn_fold_backward.register_fake
def _(gA, gB, s, gamma, saved, training, N, C, S, count, pool_count, w1=None, w2=None):
    dev = gA.device
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=dev)
    has_s = training or w1 is not None
    out = [e(N, C, dt=torch.float64) if has_s else e(1), e(N, C, dt=torch.float64) if training else e(1)]
    out += [e(C), e(C)] if gamma is not None else [e(1), e(1)]
    if w1 is not None:
        out += [torch.empty_like(w1, dtype=torch.float32), e(w1.shape[0]), torch.empty_like(w2, dtype=torch.float32), e(C)]
    else:
        out += [e(1) for _ in range(4)]
    return out


def _bf_setup(ctx, inputs, output):
    (s, q, gamma, beta, run_mean, run_var, nbt, training, N, C, S, count, eps, momentum, w1, b1, w2, b2, pool_count) = inputs
    ctx.save_for_backward(s, gamma, w1, w2, *output[2:9])
    ctx.cfg = (training, N, C, S, count, pool_count, q is not None, beta is not None, b1 is not None, b2 is not None)


def _bf_backward(ctx, grads):
    s, gamma, w1, w2 = ctx.saved_tensors[:4]
    saved = list(ctx.saved_tensors[4:])
    training, N, C, S, count, pool_count, has_q, has_beta, has_b1, has_b2 = ctx.cfg
    z = lambda: torch.zeros(N, C, dtype=torch.float64, device=saved[0].device)
    gA = z() if grads[0] is None else grads[0]
    gB = z() if grads[1] is None else grads[1]
    gs, gq, gg, gbt, gw1, gb1, gw2, gb2 = torch.ops.cfn.bn_fold_backward(gA, gB, s, gamma, saved, training, N, C, S, count, pool_count, w1, w2)
    has_s = s is not None and (training or w1 is not None)
    return (gs if has_s else None, gq if (training and has_q) else None, gg if gamma is not None else None,
            gbt if has_beta else None, None, None, None, None, None, None, None, None, None, None,
            gw1 if w1 is not None else None, gb1 if has_b1 else None, gw2 if w2 is not None else None, gb2 if has_b2 else None, None)


bn_fold.register_autograd(_bf_backward, setup_context=_bf_setup)


# ---- block tail: relu(A y + B + (Ar res + Br)) -------------------------------------------------------------------------------------
bn_add_relu = _op('bn_add_relu')


@bn_add_relu.register_fake
def _(y, A, B, res, Ar=None, Br=None):
    return torch.empty_like(y)


bn_add_relu_backward = _op('bn_add_relu_backward')      # -> [gy, gA, gB, gres, gAr, gBr]


@bn_add_relu_backward.register_fake
def _(gout, y, A, res, out, Ar=None):
    r = (lambda: torch.empty_like(Ar)) if Ar is not None else (lambda: y.new_empty(1))
    return [torch.empty_like(y), torch.empty_like(A), torch.empty_like(A), torch.empty_like(res), r(), r()]


def _bar_setup(ctx, inputs, output):
    y, A, B, res, Ar, Br = inputs
    ctx.save_for_backward(y, A, res, Ar, output)
    ctx.has_br = Br is not None


def _bar_backward(ctx, gout):
    y, A, res, Ar, out = ctx.saved_tensors
    gy, gA, gB, gres, gAr, gBr = torch.ops.cfn.bn_add_relu_backward(gout, y, A, res, out, Ar)
    return gy, gA, gB, gres, (gAr if Ar is not None else None), (gBr if ctx.has_br else None)


bn_add_relu.register_autograd(_bar_backward, setup_context=_bar_setup)


# ---- act(A x + B) materialised ---------------------------------------------------------------------------------------------------
affine_act = _op('affine_act')


@affine_act.register_fake
def _(x, A, B, act=0):
    return torch.empty_like(x)


affine_act_backward = _op('affine_act_backward')


@affine_act_backward.register_fake
def _(gout, x, A, B, act):
    return torch.empty_like(x), torch.empty_like(A), torch.empty_like(B)


def _aa_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:3])
    ctx.act = inputs[3]


affine_act.register_autograd(lambda ctx, g: (*torch.ops.cfn.affine_act_backward(g, *ctx.saved_tensors, ctx.act), None), setup_context=_aa_setup)


# ---- adaptive (OH, OW) spatial mean of act(A x + B) ------------------------------------------------------------------------------
pool_hw = _op('pool_hw')


@pool_hw.register_fake
def _(x, OH, OW, A=None, B=None, act=0):
    return x.new_empty(tuple(x.shape[:3]) + (OH, OW), dtype=torch.float32)


pool_hw_backward = _op('pool_hw_backward')


@pool_hw_backward.register_fake
def _(gout, x, OH, OW, A=None, B=None, act=0):
    ab = (lambda t: torch.empty_like(t)) if A is not None else (lambda t: x.new_empty(1, dtype=torch.float32))
    return torch.empty_like(x), ab(A), ab(B)


def _ph_setup(ctx, inputs, output):
    x, OH, OW, A, B, act = inputs
    ctx.save_for_backward(x, A, B)
    ctx.meta = (OH, OW, act)


def _ph_backward(ctx, g):
    x, A, B = ctx.saved_tensors
    OH, OW, act = ctx.meta
    gx, gA, gB = torch.ops.cfn.pool_hw_backward(g, x, OH, OW, A, B, act)
    return gx, None, None, (gA if A is not None else None), (gB if B is not None else None), None


pool_hw.register_autograd(_ph_backward, setup_context=_ph_setup)


# ---- Interp1d (interp1d.py:8-147) ---------------------------------------------------------------------------------------------------
interp1d = _op('interp1d')


@interp1d.register_fake
def _(x, y, xnew):
    B = max(x.shape[0], y.shape[0], xnew.shape[0])
    return x.new_empty(B, xnew.shape[1], dtype=torch.float32), x.new_empty(B, xnew.shape[1], dtype=torch.int64)


interp1d_backward = _op('interp1d_backward')


@interp1d_backward.register_fake
def _(g, x, y, xnew, ind):
    return torch.empty_like(x), torch.empty_like(y), torch.empty_like(xnew)


interp1d.register_autograd(lambda ctx, g, _gi: torch.ops.cfn.interp1d_backward(_gz(g, ctx.saved_tensors[3], torch.float32), *ctx.saved_tensors),
                           setup_context=lambda ctx, inputs, output: ctx.save_for_backward(*inputs, output[1]))


# ---- Grid Pool CDF (x3d_coarse.py:384-392) ---------------------------------------------------------------------------------------------
grid_cdf = _op('grid_cdf')


@grid_cdf.register_fake
def _(g, bias=None):
    return g.new_empty(g.shape[0], g.shape[1] + 1)


grid_cdf_backward = _op('grid_cdf_backward')


@grid_cdf_backward.register_fake
def _(gcdf, g, bias=None):
    return torch.empty_like(g), (torch.empty_like(bias) if bias is not None else g.new_empty(1))


def _gc_backward(ctx, gcdf):
    g, bias = ctx.saved_tensors
    gg, gb = torch.ops.cfn.grid_cdf_backward(gcdf, g, bias)
    return gg, (gb if bias is not None else None)


grid_cdf.register_autograd(_gc_backward, setup_context=lambda ctx, inputs, output: ctx.save_for_backward(*inputs))


# ---- Gaussian temporal alignment (x3d_coarse.py:251-286) ----------------------------------------------------------------------------
gauss_align = _op('gauss_align')


@gauss_align.register_fake
def _(meta, mask, gx, tx, ratio, crops, K):
    return mask.new_empty(mask.shape[0] * crops, mask.shape[1], K, dtype=torch.float32)


gauss_align_backward = _op('gauss_align_backward')


@gauss_align_backward.register_fake
def _(gGX, meta, mask, gx, tx, ratio, crops, K):
    return torch.empty_like(gx)


def _ga_setup(ctx, inputs, output):
    meta, mask, gx, tx, ratio, crops, K = inputs
    ctx.save_for_backward(meta, mask, gx)
    ctx.cfg = (tx, ratio, crops, K)


def _ga_backward(ctx, gGX):
    meta, mask, gx = ctx.saved_tensors
    ggx = torch.ops.cfn.gauss_align_backward(gGX, meta, mask, gx, *ctx.cfg) if gx is not None else None
    return None, None, ggx, None, None, None, None


gauss_align.register_autograd(_ga_backward, setup_context=_ga_setup)


# ---- Multi-stage-Fusion gather (x3d_coarse.py:199-247) --------------------------------------------------------------------------------
fusion_gather = _op('fusion_gather')      # -> (z, den): den is what the backward operator takes


@fusion_gather.register_fake
def _(x, at_raw, at_bias, GX, mask, crops=1):
    B, C, Tf, P = x.shape
    return x.new_empty(B * crops, C, GX.shape[2], P), x.new_empty(B * crops, GX.shape[2], P)


fusion_gather_backward = _op('fusion_gather_backward')


@fusion_gather_backward.register_fake
def _(gz, z, den, x, at_raw, at_bias, GX, mask, crops):
    return torch.empty_like(x), torch.empty_like(at_raw), (torch.empty_like(at_bias) if at_bias is not None else x.new_empty(1)), torch.empty_like(GX)


def _fg_setup(ctx, inputs, output):
    x, at_raw, at_bias, GX, mask, crops = inputs
    ctx.save_for_backward(x, at_raw, at_bias, GX, mask, output[0], output[1])
    ctx.crops = crops


def _fg_backward(ctx, gz, _gden):
    x, at_raw, at_bias, GX, mask, z, den = ctx.saved_tensors
    gx, gat, gb, gGX = torch.ops.cfn.fusion_gather_backward(_gz(gz, z), z, den, x, at_raw, at_bias, GX, mask, ctx.crops)
    return gx, gat, (gb if at_bias is not None else None), gGX, None, None


fusion_gather.register_autograd(_fg_backward, setup_context=_fg_setup)


# ---- block-broadcast FiLM: x * m + c with m, c constant over f x f blocks -----------------------------------------------------------------
film = _op('film')


@film.register_fake
def _(x, m, c, f):
    return torch.empty_like(x)


film_backward = _op('film_backward')


@film_backward.register_fake
def _(g, x, m, f):
    return torch.empty_like(x), torch.empty_like(m), torch.empty_like(m)


def _film_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.f = inputs[3]


film.register_autograd(lambda ctx, g: (*torch.ops.cfn.film_backward(g, *ctx.saved_tensors, ctx.f), None), setup_context=_film_setup)


# ---- linear resize along t (F.interpolate mode='linear', both align_corners conventions) -------------------------------------------------
time_resize = _op('time_resize')


@time_resize.register_fake
def _(x, L, align_corners=True):
    return x.new_empty(tuple(x.shape[:2]) + (L,) + tuple(x.shape[3:]), dtype=torch.float32)


time_resize_backward = _op('time_resize_backward')


@time_resize_backward.register_fake
def _(g, shape, L, align_corners):
    return g.new_empty(shape, dtype=torch.float32)


def _tr_setup(ctx, inputs, output):
    ctx.meta = (list(inputs[0].shape), inputs[1], inputs[2])


time_resize.register_autograd(lambda ctx, g: (torch.ops.cfn.time_resize_backward(g, *ctx.meta), None, None), setup_context=_tr_setup)


# ---- detection loss of both training scripts, one forward + one backward kernel (csrc/detloss.hip; opt-in: CFN_FUSED_LOSS / --fused-loss) ------
# -> (cls, loc, probs, jstar, ymax, norm_used): the last three are what the backward operator takes; probs is a 1-element placeholder
# when it is not wanted
detection_loss = _op('detection_loss')


@detection_loss.register_fake
def _(logits, labels, masks, align_corners, crops=1, norm=None, world=1.0, want_probs=True):
    B, C, TL = labels.shape
    return (logits.new_empty((), dtype=torch.float32), logits.new_empty((), dtype=torch.float32),
            logits.new_empty((B, C, TL) if want_probs else (1,), dtype=torch.float32), logits.new_empty((B * C,), dtype=torch.int32),
            logits.new_empty((B * C,), dtype=torch.float32), logits.new_empty((1,), dtype=torch.float64))


detection_loss_backward = _op('detection_loss_backward')


@detection_loss_backward.register_fake
def _(g_cls, g_loc, logits, labels, masks, jstar, ymax, norm_used, align_corners, crops, world):
    return logits.new_empty(logits.shape, dtype=torch.float32)


def _dl_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2], output[3], output[4], output[5])
    ctx.meta = (inputs[3], inputs[4], inputs[6])


def _dl_backward(ctx, g_cls, g_loc, *_rest):      # (probs and the saved statistics carry no gradient)
    return (torch.ops.cfn.detection_loss_backward(g_cls, g_loc, *ctx.saved_tensors, *ctx.meta),) + (None,) * 7


detection_loss.register_autograd(_dl_backward, setup_context=_dl_setup)


# ---- uint8 frames: crop + antialiased bilinear resize + flip on the GPU (csrc/aug_u8.hip; the tap tables: cfn_hip/u8aug.py) -------
crop_resize_flip_u8 = _op('crop_resize_flip_u8')


@crop_resize_flip_u8.register_fake
def _(frames, lengths, box, bounds, coef, size):
    N, T = frames.shape[:2]
    return frames.new_empty((N, T, size, size, 3), dtype=torch.uint8)


# ---- per-class average precision on the GPU (csrc/apmeter.hip): class-major stores on the device, no gradient ------------------------------
ap_append = _op('ap_append')      # (mutates scores, targets, count, flags)


@ap_append.register_fake
def _(probs, labels, valid, scores, targets, count, flags):
    return None


ap_sort = _op('ap_sort')


@ap_sort.register_fake
def _(scores, targets, count):
    return torch.empty_like(scores), torch.empty_like(targets)


average_precision = _op('average_precision')


@average_precision.register_fake
def _(scores, targets, count):
    return scores.new_empty((scores.shape[0],), dtype=torch.float32)


# ---- packed 16-bit fine features (csrc/featpack.hip; the record format and the batch type: cfn_hip/featpack.py), no gradient ------------------
feat_unpack = _op('feat_unpack')


@feat_unpack.register_fake
def _(data, offsets, lengths, channels, t_max):
    return [data.new_empty((offsets.shape[0], c, t_max, 7, 7), dtype=torch.float32) for c in channels]


feat_pack = _op('feat_pack')


@feat_pack.register_fake
def _(feat, dtype):
    n = 0
    for f in feat:
        n = n + f.shape[-4] * f.shape[-3] * 49
    return feat[0].new_empty((n,), dtype=dtype)


# ---- baseline JPEG frames decoded on the GPU (csrc/jpegdec.hip; the batch type: cfn_hip/jpegdec.py), no gradient ----------------------------
# the members of a JpegClips batch -> (frames (N, Tmax, Hmax, Wmax, 3) uint8, status (R,) int32)
jpeg_decode_u8 = _op('jpeg_decode_u8')


@jpeg_decode_u8.register_fake
def _(data, frames, tables, geom, lengths, dims):
    return (data.new_empty((lengths.numel(), dims[0], dims[1], dims[2], 3), dtype=torch.uint8),
            data.new_empty((frames.shape[0],), dtype=torch.int32))


# jpeg_decode_u8 with the sync entropy mode (ops.jpeg_decode_u8(..., entropy='sync', sub_bytes, max_subs)): the same outputs
jpeg_decode_sync_u8 = _op('jpeg_decode_sync_u8')


@jpeg_decode_sync_u8.register_fake
def _(data, frames, tables, geom, lengths, dims, sub_bytes, max_subs):
    return (data.new_empty((lengths.numel(), dims[0], dims[1], dims[2], 3), dtype=torch.uint8),
            data.new_empty((frames.shape[0],), dtype=torch.int32))


# ---- frame labels from annotation segments (csrc/seglabels.hip; the sample record and the batch type: cfn_hip/seglabels.py), no gradient ------
seg_labels = _op('seg_labels')


@seg_labels.register_fake
def _(seg, offsets, fps, window, n_classes, t_max):
    B = offsets.shape[0] - 1
    return (seg.new_empty((B, n_classes, t_max), dtype=torch.float32), seg.new_empty((B, t_max), dtype=torch.float32),
            seg.new_empty((B,), dtype=torch.int32))


OPERATORS = ('dwconv3d', 'pwconv', 'time_sample', 'dwconv_t5', 'stem_conv', 'conv3d_dense', 'bn_fold', 'bn_add_relu', 'affine_act',
             'pool_hw', 'interp1d', 'grid_cdf', 'gauss_align', 'fusion_gather', 'film', 'time_resize', 'stem_conv_u8', 'detection_loss')
# the uint8 input path's operators without a gradient (the host-built table, the frames -> fp32 clip converter)
INPUT_OPERATORS = ('clip_lut', 'clip_u8_to_f32')
# spatial augmentation of uint8 frames on the GPU (no gradient)
AUGMENT_OPERATORS = ('crop_resize_flip_u8',)
# device-resident average precision (no gradient; ap_append mutates its stores)
METRIC_OPERATORS = ('ap_append', 'ap_sort', 'average_precision')
# packed 16-bit fine features: widen + pad a batch, round + transpose one video's maps (no gradient)
FEATURE_OPERATORS = ('feat_unpack', 'feat_pack')
# baseline JPEG frames -> uint8 frames on the GPU (no gradient)
DECODE_OPERATORS = ('jpeg_decode_u8',)
# the same decode with the sync entropy mode: parallel inside a frame without restart markers (no gradient)
DECODE_SYNC_OPERATORS = ('jpeg_decode_sync_u8',)
# annotation segments -> dense frame labels, mask and lengths on the GPU (no gradient)
LABEL_OPERATORS = ('seg_labels',)


# ---------------------------------------------------------------------------------------------------------------------------
# cfn_hip.ops-shaped facade over the registered operators: the CFN_USE_TORCH_OPS route of the x3d_coarse modules (GridPoolLayer,
# GridUnpool, Gaussian, RewightLayer, MixingLayer; reference x3d_coarse.py:175-451) calls the SAME function names with the same
# arguments, and every call goes through the dispatcher (torch.ops.cfn.*) instead of the autograd Functions of cfn_hip.ops.
# Prologue coefficients arrive as fp64 tensors holding fp32 values (cfn_hip.ops convention); the operators' gradient formulas return
# fp32, so they are narrowed here (lossless, differentiable).
# ---------------------------------------------------------------------------------------------------------------------------
def _f32(t):
    return t if t is None or t.dtype == torch.float32 else t.float()


class TorchOps(object):
    @staticmethod
    def pwconv(x, w, A=None, B=None, act=ACT_NONE, stride=1, stats=True, **_unused):
        y, s, q = torch.ops.cfn.pwconv(x, w, _f32(A), _f32(B), act, stride)
        return (y, s, q) if stats else (y, None, None)

    @staticmethod
    def conv3d_dense(x, w, kernel, stride, padding, A=None, B=None, act=ACT_NONE, stats=True):
        y, s, q = torch.ops.cfn.conv3d_dense(x, w, list(kernel), list(stride), list(padding), _f32(A), _f32(B), act)
        return (y, s, q) if stats else (y, None, None)

    @staticmethod
    def affine_act(x, A, B, act=ACT_NONE):
        return torch.ops.cfn.affine_act(x, _f32(A), _f32(B), act)

    @staticmethod
    def pool_hw(x, OH, OW, A=None, B=None, act=ACT_NONE):
        return torch.ops.cfn.pool_hw(x, OH, OW, _f32(A), _f32(B), act)

    @staticmethod
    def fusion_gather(x, at_raw, at_bias, GX, mask, crops=1):
        return torch.ops.cfn.fusion_gather(x, at_raw, at_bias, GX, mask, crops)[0]

    @staticmethod
    def gauss_align(meta, mask, gx, tx, ratio, crops, K):
        return torch.ops.cfn.gauss_align(meta, mask, gx, 1.0 if tx is None else float(tx), float(ratio), crops, K)

    @staticmethod
    def grid_cdf(g, bias=None):
        return torch.ops.cfn.grid_cdf(g, bias)

    @staticmethod
    def time_sample(x, cdf):
        return torch.ops.cfn.time_sample(x, cdf)

    @staticmethod
    def time_resize(x, L, align_corners=True):
        return torch.ops.cfn.time_resize(x, L, align_corners)

    @staticmethod
    def film(x, m, c, f):
        return torch.ops.cfn.film(x, m, c, f)

    @staticmethod
    def detection_loss(logits, labels, masks, align_corners, crops=1, norm=None, world=1.0, want_probs=True):
        cls, loc, probs = torch.ops.cfn.detection_loss(logits, labels, masks, align_corners, crops, norm, world, want_probs)[:3]
        return cls, loc, (probs if want_probs else None)

    @staticmethod
    def interp1d(x, y, xnew):
        return torch.ops.cfn.interp1d(x, y, xnew)
