"""fp64 reference of the dense conv entry points (cfn_conv3d_dense_fwd / _bwd_data / _bwd_weight, cfn_stem_conv_*), with the C ABI's
arguments (every optional one may be None), in plain tensor operations -- slices and einsum, one temporal / spatial tap at a time, no
conv3d call -- so it runs on either device without MIOpen.

    a  = relu(A x + B)            (a = x without a prologue; the zero padding comes AFTER the prologue)
    y  = W * a,   s = sum_pos y,   q = sum_pos y^2
    G' = gy + gs + 2 gq y
    gx = act'(A x + B) A  W^T * G',   gA = sum_pos dz x,   gB = sum_pos dz        (dz = act'() W^T * G')
    gw = sum_{n, pos} G' (x) im2col(a)

Next to every output the reference returns the magnitude sums an error bound needs (sum |w||a|, sum |w||G'|, ...).

BOUNDS (u = 2^-24).  An output element that is a sum of products is bounded by  gamma(n) * mag + (input roundings),  gamma(n) = n u / (1 - n u),
mag = the fp64 sum of the absolute values of its summands, n = the number of fp32 roundings on the longest path to it.  The kernels' summation
orders inside a wave are the matrix pipe's; n is therefore the WORST order, the whole share of one wave in a row, plus the cross-wave sums:

  y    fp32 kernels (sal_fwd, pw_gemm, stem_fwd):  n = K + 4  (K = Cin kT kH kW products and adds; 3 cross-wave adds; 1 to spare).
       salconvb: six bf16 x bf16 products per element pair (exact in fp32), 168 k per wave -> n = 6 * 168 + 4 summands of total magnitude
       <= (1 + 2^-7) mag; the three dropped products a2 b3 + a3 b2 + a3 b3: round-to-nearest-even bf16 terms have |a2| <= 2^-8 |a|,
       |a3| <= 2^-16 |a| and a1 + a2 + a3 = a exactly (24 = 3 x 8 bits), so they are <= (2 * 2^-24 + 2^-32) |a b| = 2.01 u mag.
       The prologue rounds A, B to fp32 and then one fma:  |da| <= 3 u (|A||x| + |B|); through the conv: 3 u sum |w| (|A||x| + |B|).
  s, q fp64 atomics fed by fp32 partial sums of n_s values (sal kernels: a lane's frames of one chunk + 5 shuffles + 1; pw_gemm: taken as
       all Q positions): sum of the y bounds + gamma(n_s) sum |y|;  q: 2 |y| * (y bound) + gamma(n_s + 1) sum y^2.
  G'   (float)gs, 2 (float)gq, one add, one fma:  <= 3 u (|gy| + |gs| + 2 |gq||y|) =: 3 u gmag.
  gx   n = Cout kT kH kW + 4 (all taps of all output channels in a row; (float)A and the product with it), mag = |A| sum |w||G'|,
       + 3 u |A| sum |w| gmag.  A position under a dead ReLU, or one that no tap reaches, has no summand: exactly 0.
  gA, gB  sum of the dz bounds (times |x|) + gamma(n_acc) sum |dz| (|x|),  n_acc = 520: a lane of sal_dgrad adds <= 64 steps x 4 classes x 2
       values before the shuffles; the generic kernels add 6 + 3.
  gw   fp32 over the positions ONE workgroup multiplies (sal_wgrad: all items of the persistent loop, ceil(items / grid) * chunk * 56 positions;
       stem_wgrad: chunk * 448; the generic kernels: taken as all N Q positions), then fp64 atomics:  gamma(n_w) sum |G'||a|
       + 3 u sum (gmag |a| + |G'| (|A||x| + |B|)).
"""
import torch

U = 2.0 ** -24
NONE, RELU = 0, 1
SAL = (3, 3, 3, 2, 2, 2, 1, 1, 1)
STEM = (1, 3, 3, 1, 2, 2, 0, 1, 1)
PRO, STATS, Y, MISALIGNED, SWISH = 1, 2, 4, 16, 32
MIS_X, MIS_G, MIS_OUT = 64, 128, 256      # one tensor alone off the boundary: x; gy and y; the output (y / gx)
FWD, DGRAD, WGRAD, STEM_FWD, STEM_WGRAD = 0, 1, 2, 3, 4
STEM_U8_FWD, STEM_U8_WGRAD = 5, 6      # uint8 frames (N, T, H, W, 3): MIS_X puts them off a 4-byte boundary; a declined call is 'convert ' + the line of op 3 / 4


def gamma(n):
    return n * U / (1.0 - n * U)


def out_shape(T, H, W, g):
    return ((T + 2 * g[6] - g[0]) // g[3] + 1, (H + 2 * g[7] - g[1]) // g[4] + 1, (W + 2 * g[8] - g[2]) // g[5] + 1)


def _pad(a, g, value=None):
    """zero padding; value (N, C): the padding holds value[n, c] instead (a planted error)"""
    N, C, T, H, W = a.shape
    ap = a.new_zeros(N, C, T + 2 * g[6], H + 2 * g[7], W + 2 * g[8])
    if value is not None:
        ap += value.view(N, C, 1, 1, 1)
    ap[:, :, g[6]:g[6] + T, g[7]:g[7] + H, g[8]:g[8] + W] = a
    return ap


def _tap(ap, kt, kh, kw, g, osz):
    """the padded input at tap (kt, kh, kw) of every output position: (N, C, To, Ho, Wo), a view"""
    To, Ho, Wo = osz
    return ap[:, :, kt:kt + g[3] * (To - 1) + 1:g[3], kh:kh + g[4] * (Ho - 1) + 1:g[4], kw:kw + g[5] * (Wo - 1) + 1:g[5]]


def _bc(v):
    return v.double().view(v.shape[0], v.shape[1], 1, 1, 1)


def prologue(x, A, B, act, ge=False):
    """a, the pre-activation z (None without a prologue) and the magnitude |A||x| + |B| of the roundings that reach a (0 where a = 0)"""
    x = x.double()
    if A is None:
        return x, None, torch.zeros_like(x)
    z = _bc(A) * x + _bc(B)
    if act == NONE:
        return z, z, _bc(A).abs() * x.abs() + _bc(B).abs()
    assert act == RELU, 'the reference knows the prologues the forward accepts: none, ReLU'
    on = (z >= 0) if ge else (z > 0)
    return z * (z > 0), z, (_bc(A).abs() * x.abs() + _bc(B).abs()) * on


def ambiguous(x, A, B):
    """positions whose pre-activation is so close to 0 that fp32 may decide the ReLU the other way: 0 < |z| <= 3 u (|A||x| + |B|) (an exact
    zero -- A x = B = 0 -- is decided the same way in both arithmetics)"""
    x = x.double()
    z = _bc(A) * x + _bc(B)
    bz = 3 * U * (_bc(A).abs() * x.abs() + _bc(B).abs())
    return (z.abs() <= bz) & (bz > 0)


def forward(x, A, B, act, w, geom, mutant=None, plan=None):
    """{'y', 's', 'q'} and the magnitudes {'wa': sum |w||a|, 'wam': sum |w| (|A||x| + |B|)} per output element.  mutant: a planted error
    (MUTANTS); plan: what the seam mutants need of the kernel's plan (chunk = TO, rb = output rows per band)"""
    g = geom
    kT, kH, kW = g[0], g[1], g[2]
    a, z, am = prologue(x, A, B, act)
    N, C, T, H, W = a.shape
    Co = w.shape[0]
    w5 = w.double().view(Co, C, kT, kH, kW)
    osz = out_shape(T, H, W, g)
    halo = None
    if mutant == 'halo_no_prologue' and A is not None:
        halo = B.double().clamp(min=0)
    ap, amp = _pad(a, g, halo), _pad(am, g)
    y = a.new_zeros((N, Co) + osz)
    wa, wam = torch.zeros_like(y), torch.zeros_like(y)
    if mutant == 'five_terms':      # a1 b2 dropped: a1 = bf16(a), w2 = bf16(w - bf16(w))
        a1p = _pad(a.float().bfloat16().double(), g)
        w1 = w5.float().bfloat16().double()
        w2 = (w5 - w1).float().bfloat16().double()
    to = torch.arange(osz[0], device=a.device).view(1, 1, -1, 1, 1)
    oh = torch.arange(osz[1], device=a.device).view(1, 1, 1, -1, 1)
    for kt in range(kT):
        for kh in range(kH):
            for kw in range(kW):
                sl = _tap(ap, kt, kh, kw, g, osz)
                if mutant == 'tap2_wrong_frame' and kt == 2:
                    sl = _tap(ap, 1, kh, kw, g, osz)
                c = torch.einsum('nctuv,oc->notuv', sl, w5[:, :, kt, kh, kw])
                if mutant == 'tap0_chunk_seam' and kt == 0:
                    c = c * ~((to % plan['chunk'] == 0) & (to > 0))
                if mutant == 'halo_row_band_seam' and kh == 0:
                    c = c * ~((oh % plan['rb'] == 0) & (oh > 0))
                if mutant == 'five_terms':
                    c = c - torch.einsum('nctuv,oc->notuv', _tap(a1p, kt, kh, kw, g, osz), w2[:, :, kt, kh, kw])
                y += c
                wabs = w5[:, :, kt, kh, kw].abs()
                wa += torch.einsum('nctuv,oc->notuv', _tap(ap, kt, kh, kw, g, osz).abs(), wabs)
                wam += torch.einsum('nctuv,oc->notuv', _tap(amp, kt, kh, kw, g, osz), wabs)
    return {'y': y, 's': y.sum((2, 3, 4)), 'q': (y * y).sum((2, 3, 4)), 'wa': wa, 'wam': wam}


def forward_bounds(r, n_y, n_s, split=False):
    """per-element bounds of y, s, q from forward()'s magnitudes"""
    by = (gamma(n_y) * (1 + 2.0 ** -7) + 2.01 * U) * r['wa'] if split else gamma(n_y) * r['wa']
    by = by + 3 * U * r['wam']
    y = r['y']
    bs = by.sum((2, 3, 4)) + gamma(n_s) * y.abs().sum((2, 3, 4))
    bq = (2 * y.abs() * by + by * by).sum((2, 3, 4)) + gamma(n_s + 1) * (y * y).sum((2, 3, 4))
    return {'y': by, 's': bs, 'q': bq}


def backward(gy, y, gs, gq, w, x, A, B, act, geom, mutant=None, plan=None, want=('gx', 'gw')):
    """{'gx', 'gA', 'gB', 'gw'} and their magnitudes: 'wg' = sum |w||G'| and 'wgm' = sum |w| gmag per input position (before A and act'),
    'ga' = sum |G'||a| and 'gam' = sum (gmag |a| + |G'| am) per weight"""
    g = geom
    kT, kH, kW = g[0], g[1], g[2]
    a, z, am = prologue(x, A, B, act)
    N, C, T, H, W = a.shape
    Co = w.shape[0]
    w5 = w.double().view(Co, C, kT, kH, kW)
    osz = out_shape(T, H, W, g)
    G = gy.double()
    gm = G.abs()
    if gs is not None and mutant != 'no_gs':
        G = G + _bc(gs)
    if gs is not None:
        gm = gm + _bc(gs).abs()
    if gq is not None and mutant != 'no_gq':
        G = G + 2 * _bc(gq) * y.double()
    if gq is not None:
        gm = gm + 2 * _bc(gq).abs() * y.double().abs()
    out = {}
    to = torch.arange(osz[0], device=a.device).view(1, 1, -1, 1, 1)
    oh = torch.arange(osz[1], device=a.device).view(1, 1, 1, -1, 1)
    if 'gx' in want:
        dap = _pad(torch.zeros_like(a), g)
        wgp, wgmp = torch.zeros_like(dap), torch.zeros_like(dap)
        Ga = G.abs()
        for kt in range(kT):
            for kh in range(kH):
                for kw in range(kW):
                    wt = w5[:, :, kt, kh, kw]
                    _tap(dap, kt, kh, kw, g, osz).add_(torch.einsum('notuv,oc->nctuv', G, wt))
                    _tap(wgp, kt, kh, kw, g, osz).add_(torch.einsum('notuv,oc->nctuv', Ga, wt.abs()))
                    _tap(wgmp, kt, kh, kw, g, osz).add_(torch.einsum('notuv,oc->nctuv', gm, wt.abs()))
        crop = lambda t: t[:, :, g[6]:g[6] + T, g[7]:g[7] + H, g[8]:g[8] + W]
        da, wg, wgm = crop(dap), crop(wgp), crop(wgmp)
        if A is None:
            out.update(gx=da, wg=wg, wgm=wgm)
        else:
            on = ((z >= 0) if mutant == 'relu_ge' else (z > 0)) if act == RELU else torch.ones_like(z, dtype=torch.bool)
            dz = da * on
            wg, wgm = wg * on, wgm * on
            xd = x.double()
            out.update(gx=dz * _bc(A), wg=wg, wgm=wgm, gB=dz.sum((2, 3, 4)),
                       gA=(dz if mutant == 'gA_no_x' else dz * xd).sum((2, 3, 4)), dz=dz)
    if 'gw' in want:
        ap, amp = _pad(a, g), _pad(am, g)
        Gw = G
        if mutant == 'skip_last_chunk':
            Gw = G * (to < (plan['nchunks'] - 1) * plan['chunk'])
        if mutant == 'skip_second_item':      # item `grid`: the second trip of workgroup 0's persistent loop
            it = plan['grid']
            band, chunk, n = it % plan['bands'], (it // plan['bands']) % plan['nchunks'], it // (plan['bands'] * plan['nchunks'])
            keep = torch.ones_like(G, dtype=torch.bool)
            keep[n, :, chunk * plan['chunk']:(chunk + 1) * plan['chunk'], band * plan['rb']:(band + 1) * plan['rb']] = False
            Gw = G * keep
        gw = a.new_zeros(Co, C, kT, kH, kW)
        ga, gam = torch.zeros_like(gw), torch.zeros_like(gw)
        for kt in range(kT):
            for kh in range(kH):
                for kw in range(kW):
                    sl = _tap(ap, kt, kh, kw, g, osz)
                    gw[:, :, kt, kh, kw] = torch.einsum('notuv,nctuv->oc', Gw, sl)
                    ga[:, :, kt, kh, kw] = torch.einsum('notuv,nctuv->oc', G.abs(), sl.abs())
                    gam[:, :, kt, kh, kw] = (torch.einsum('notuv,nctuv->oc', gm, sl.abs())
                                             + torch.einsum('notuv,nctuv->oc', G.abs(), _tap(amp, kt, kh, kw, g, osz)))
        if mutant == 'swap_khkw':
            gw = gw.transpose(3, 4).contiguous()
        out.update(gw=gw.reshape(Co, -1), ga=ga.reshape(Co, -1), gam=gam.reshape(Co, -1))
    return out


def backward_bounds(r, x, A, n_d, n_w, n_acc=520):
    b = {}
    if 'gx' in r:
        bd = gamma(n_d) * r['wg'] + 3 * U * r['wgm']
        if A is None:
            b['gx'] = bd
        else:
            b['gx'] = bd * _bc(A).abs()
            xa = x.double().abs()
            b['gB'] = bd.sum((2, 3, 4)) + gamma(n_acc) * r['dz'].abs().sum((2, 3, 4))
            b['gA'] = (bd * xa).sum((2, 3, 4)) + gamma(n_acc + 1) * (r['dz'].abs() * xa).sum((2, 3, 4))
    if 'gw' in r:
        b['gw'] = gamma(n_w) * r['ga'] + 3 * U * r['gam']
    return b


def worst(got, ref, bound):
    """max err / bound over the elements (an element whose bound is 0 has to be exact: inf otherwise)"""
    err = (got.double() - ref).abs()
    ok0 = (bound > 0) | (err == 0)
    if not bool(ok0.all()):
        return float('inf')
    return float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0


# ---- the kernel's plan, from a line of cfn_conv3d_dense_route ---------------------------------------------------------------------------
def fields(line):
    f = {'family': line.split()[0], 'kernel': line.split(' ', 1)[1].split(' grid=')[0] if ' grid=' in line else line}
    for kv in line.split():
        if '=' in kv:
            k, v = kv.split('=')
            f[k] = v if 'x' in v else int(v)
    return f


def roundings(op, line, N, Cin, Cout, T, H, W, geom):
    """n of the module docstring for the kernel named by the route line"""
    f = fields(line)
    K = Cin * geom[0] * geom[1] * geom[2]
    To, Ho, Wo = out_shape(T, H, W, geom)
    Q = To * Ho * Wo
    fam = f['family']
    if op in (FWD, STEM_FWD):
        return {'n_y': 6 * 168 + 4 if fam == 'salb' else K + 4, 'n_s': f['chunk'] + 6 if fam in ('salb', 'sal') else Q, 'split': fam == 'salb'}
    if op == DGRAD:
        return {'n_d': Cout * geom[0] * geom[1] * geom[2] + 4}
    if fam == 'sal':
        return {'n_w': -(-f['items'] // f['grid']) * f['chunk'] * 56 + 2}
    if fam == 'stem':
        return {'n_w': f['chunk'] * 448 + 8}
    return {'n_w': N * Q}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def seed_of(name):
    """the seed of a committed case: from its name, the same in the CPU and the GPU test"""
    return sum((k + 1) * ord(c) for k, c in enumerate(name)) % 100003


def make_inputs(seed, N, Cin, Cout, T, H, W, geom, pro, exact_zero=False):
    """deterministic fp32 inputs (CPU generator).  With a prologue, x is moved by 1/4 wherever the pre-activation would land within 1e-3 of 0:
    no committed case holds an ambiguous ReLU decision.  exact_zero: channel 0 has B = 0 and some x = 0, pre-activations that are exactly 0"""
    g = torch.Generator().manual_seed(seed)
    K = Cin * geom[0] * geom[1] * geom[2]
    x = torch.randn(N, Cin, T, H, W, generator=g)
    w = torch.randn(Cout, K, generator=g) * (2.0 / K) ** 0.5
    A = B = None
    if pro:
        A = (1 + 0.2 * torch.randn(N, Cin, generator=g)).double()
        B = (0.3 * torch.randn(N, Cin, generator=g)).double()
        if exact_zero:
            B[:, 0] = 0
        z = _bc(A) * x.double() + _bc(B)
        x = torch.where(z.abs() < 1e-3, x + 0.25, x)
        if exact_zero:
            x[:, 0, :, ::3, ::5] = 0
    osz = out_shape(T, H, W, geom)
    gy = torch.randn((N, Cout) + osz, generator=g)
    gs = (0.01 * torch.randn(N, Cout, generator=g)).double()
    gq = (0.001 * torch.randn(N, Cout, generator=g)).double()
    return {'x': x, 'w': w, 'A': A, 'B': B, 'gy': gy, 'gs': gs, 'gq': gq}


# ---- mutants: name -> (pass, output that must leave its bound) -------------------------------------------------------------------------
MUTANTS = {
    'tap0_chunk_seam': ('fwd', 'y'),          # temporal tap 0 lost at the first output frame of a chunk (the halo frame 2 to0 - 1)
    'halo_row_band_seam': ('fwd', 'y'),       # the halo row above a band lost
    'tap2_wrong_frame': ('fwd', 'y'),         # tap 2 taken from frame 2 to instead of 2 to + 1
    'halo_no_prologue': ('fwd', 'y'),         # relu(B) instead of 0 in the padding
    'five_terms': ('fwd', 'y'),               # one first-order cross term of the bf16 split (a1 b2) lost
    'no_gq': ('bwd', 'gx'),                   # G' without 2 gq y
    'no_gs': ('bwd', 'gx'),                   # G' without gs
    'relu_ge': ('bwd', 'gx'),                 # ReLU' taken at z >= 0
    'gA_no_x': ('bwd', 'gA'),                 # gA without its x factor
    'skip_last_chunk': ('bwd', 'gw'),         # the last, shorter chunk of output frames not multiplied
    'skip_second_item': ('bwd', 'gw'),        # a persistent workgroup stops after its first item
    'swap_khkw': ('bwd', 'gw'),               # kh and kw exchanged in gw
}


# ---- the GPU cases (tests/test_hip_dense.py); tests/test_dense_route_cpu.py confirms every claimed branch at 256 CUs -----------------------
# (name, geom, N, Cin, Cout, T, H, W, flags, claims): flags as in cfn_conv3d_dense_route; claims: op -> (kernel, predicate on the route fields)
def _c(kernel, pred=None):
    return (kernel, pred)


SAL_CASES = [
    # 56 wide, no prologue, T odd: salb / sal_fwd<56, 1, false>, bands of 1 / 1 row; dgrad bands of 4 (Ho = 10: ragged), wgrad bands of 2;
    # T = 5 -> To = 3, chunk 2: a short last chunk in all three
    ('w56_T5', SAL, 2, 24, 24, 5, 20, 56, STATS | Y,
     {FWD: _c('sal_fwdb_kernel<56, false>', lambda f: f['last'] != f['chunk']), DGRAD: _c('sal_dgrad_kernel<56, false, true>', lambda f: f['bands'] == 3),
      WGRAD: _c('sal_wgrad_kernel<56, false, true>', lambda f: f['last'] == 1)}),
    # 28 wide, ReLU prologue, T even; Ho = 10 is ragged for all three band heights at 28 wide (2, 8, 4 rows)
    ('w28_pro_T4', SAL, 2, 24, 24, 4, 20, 28, PRO | STATS | Y,
     {FWD: _c('sal_fwdb_kernel<28, true>', lambda f: f['bands'] == 5), DGRAD: _c('sal_dgrad_kernel<28, true, true>', lambda f: f['bands'] == 2),
      WGRAD: _c('sal_wgrad_kernel<28, true, true>', lambda f: f['bands'] == 3)}),
    # T = 1: one output frame, no odd frame at all; 56 wide with the prologue; only gs in the backward (YV = false, two-term G')
    ('w56_pro_T1_gs', SAL, 1, 24, 24, 1, 8, 56, PRO | STATS,
     {FWD: _c('sal_fwdb_kernel<56, true>', lambda f: f['nchunks'] == 1 and f['last'] == 1), DGRAD: _c('sal_dgrad_kernel<56, true, false>'),
      WGRAD: _c('sal_wgrad_kernel<56, true, false>')}),
    # T = 2, the shortest plane (Hi = 2), 28 wide, neither gs nor gq (YV = false, G' = gy); one group: an idle half-workgroup in dgrad
    ('w28_T2_H2_plain', SAL, 1, 24, 24, 2, 2, 28, 0,
     {FWD: _c('sal_fwdb_kernel<28, false>', lambda f: f['bands'] == 1), DGRAD: _c('sal_dgrad_kernel<28, false, false>', lambda f: f['items'] % 2 == 1),
      WGRAD: _c('sal_wgrad_kernel<28, false, false>')}),
    # pre-activations that are EXACTLY 0 (a name ending in _z0: B = 0 in channel 0 and zeros in x): ReLU' must be 0 there, in gx and in gA / gB
    ('w28_pro_z0', SAL, 1, 24, 24, 3, 8, 28, PRO | STATS | Y,
     {DGRAD: _c('sal_dgrad_kernel<28, true, true>'), WGRAD: _c('sal_wgrad_kernel<28, true, true>')}),
    # forward only: Cout 20 and 32 (the channel guards of the epilogue)
    ('w28_co20', SAL, 1, 24, 20, 3, 6, 28, PRO | STATS, {FWD: _c('sal_fwdb_kernel<28, true>')}),
    ('w56_co32', SAL, 1, 24, 32, 3, 4, 56, STATS, {FWD: _c('sal_fwdb_kernel<56, false>')}),
    # every tensor one element past a 16-byte boundary: all three sal kernels decline (16-byte loads of x, 8-byte loads / stores of g', y, x, gx)
    ('w28_misaligned', SAL, 1, 24, 24, 3, 8, 28, PRO | STATS | Y | MISALIGNED,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 1, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    # ONE tensor off the boundary at a time, each clause of the gates on its own.  x alone: the forward and the weight gradient read it 16 bytes at a
    # time and decline, the data gradient reads it for the prologue (8 bytes at a time) and declines ...
    ('w28_mis_x', SAL, 1, 24, 24, 3, 8, 28, PRO | STATS | Y | MIS_X,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 1, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    # ... but without a prologue the data gradient never reads x and stays on the sal kernel
    ('w28_mis_x_plain', SAL, 1, 24, 24, 3, 8, 28, STATS | Y | MIS_X,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 0, true>'), DGRAD: _c('sal_dgrad_kernel<28, false, true>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    # gy and y alone: both backward kernels read them 8 bytes at a time and decline; the forward has neither
    ('w28_mis_g', SAL, 1, 24, 24, 3, 8, 28, PRO | STATS | Y | MIS_G,
     {FWD: _c('sal_fwdb_kernel<28, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    # the output alone: the forwards store y one element at a time and stay (sal_fwdb and sal_fwd), the data gradient stores gx 8 bytes at a time and
    # declines, the weight gradient's output is the fp64 gw
    ('w28_mis_out', SAL, 1, 24, 24, 3, 8, 28, PRO | STATS | Y | MIS_OUT,
     {FWD: _c('sal_fwdb_kernel<28, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('sal_wgrad_kernel<28, true, true>')}),
]

# long chunks: the smallest inputs the query gives for each branch (256 CUs; found by scanning N, T, Hi with the query)
LONG_CASES = [
    # forward TO = 3 with a full and with a short last chunk (two accumulator sets across the chunk seam, odd chunk length)
    ('fwd_TO3_full', SAL, 4, 24, 24, 17, 52, 56, STATS, {FWD: _c('sal_fwdb_kernel<56, false>', lambda f: f['chunk'] == 3 and f['last'] == 3)}),
    ('fwd_TO3_short', SAL, 4, 24, 24, 21, 44, 56, PRO | STATS, {FWD: _c('sal_fwdb_kernel<56, true>', lambda f: f['chunk'] == 3 and f['last'] == 2)}),
    # weight gradient CH = 4 (28 wide)
    ('wg_CH4', SAL, 4, 24, 24, 129, 10, 28, PRO | STATS | Y, {WGRAD: _c('sal_wgrad_kernel<28, true, true>', lambda f: f['chunk'] == 4 and f['last'] != 4)}),
    # weight gradient: the persistent loop makes a second trip in some workgroups only (468 items on 256 workgroups)
    ('wg_persistent', SAL, 4, 24, 24, 33, 50, 56, STATS | Y, {WGRAD: _c('sal_wgrad_kernel<56, false, true>', lambda f: f['grid'] < f['items'] < 2 * f['grid'])}),
    # data gradient CH = 4: the two-slot g' ring goes round twice
    ('dg_CH4', SAL, 4, 24, 24, 129, 26, 56, STATS | Y, {DGRAD: _c('sal_dgrad_kernel<56, false, true>', lambda f: f['chunk'] == 4 and f['last'] != 4)}),
    # the forward at the benchmark's plan, TO = 8 at 8 x 56 x 56: T = 29 is the shortest clip that gives it (last chunk 7)
    ('fwd_bench_TO8', SAL, 8, 24, 24, 29, 56, 56, STATS, {FWD: _c('sal_fwdb_kernel<56, false>', lambda f: f['chunk'] == 8 and f['bands'] == 28)}),
    # data gradient, odd group count with CH = 4: the last workgroup's second half idles through the long loop
    ('dg_odd', SAL, 3, 24, 24, 97, 50, 56, PRO | STATS | Y, {DGRAD: _c('sal_dgrad_kernel<56, true, true>', lambda f: f['chunk'] == 4 and f['items'] % 2 == 1)}),
]

G3 = (3, 3, 3, 2, 2, 2, 1, 1, 1)
G1 = STEM
GENERIC_CASES = [
    # (1,3,3)/(1,2,2)/(0,1,1), T = 1, odd plane 9 x 7, Cin 3 -> all-channel CI = 8; Wo = 4 and Q = 20: the direct weight gradient, one tile
    ('g1_ci3_9x7', G1, 2, 3, 5, 1, 9, 7, PRO | STATS | Y,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 1, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<8>'), WGRAD: _c('pw_wgrad_direct_kernel<1, 2, 1, 1>')}),
    # Cin 8 / 9 across the CI = 8 | 24 limit; 3x3x3; Wo = 5: the LDS-staged weight gradient <1, 2> / <1, 2>
    ('g3_ci8', G3, 1, 8, 7, 3, 9, 9, STATS | Y, {FWD: _c('pw_gemm_kernel<1, 0, true, 0, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<8>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    ('g3_ci9', G3, 1, 9, 7, 3, 9, 9, STATS | Y, {DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    # Cin 24 / 25 across CI = 24 | 32, Cin 32 / 33: the per-channel kernel; Cout 40: staged <2, 2>
    ('g1_ci25', G1, 1, 25, 40, 2, 8, 8, PRO | STATS | Y, {FWD: _c('pw_gemm_kernel<2, 0, true, 1, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<32>'), WGRAD: _c('pw_wgrad_direct_kernel<1, 2, 3, 3>')}),
    ('g1_ci32', G1, 1, 32, 40, 2, 7, 6, STATS | Y, {DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<32>'), WGRAD: _c('pw_wgrad_kernel<2, 2>')}),
    ('g1_ci33', G1, 1, 33, 24, 2, 7, 7, PRO | STATS | Y, {FWD: _c('pw_gemm_kernel<1, 0, true, 1, true>'), DGRAD: _c('conv3d_dense_bwd_data_kernel'), WGRAD: _c('pw_wgrad_direct_kernel<1, 2, 3, 3>')}),
    # the all-channel weight image between 48 and 64 KiB (hipFuncSetAttribute) and past 64 KiB (per-channel kernel): 3x3x3, Cin 24 -> 2592 B per Cout
    ('g3_lds48', G3, 1, 24, 20, 3, 9, 7, STATS | Y, {DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>', lambda f: 48 * 1024 < f['lds'] <= 64 * 1024), WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 3, 3>')}),
    ('g3_lds64', G3, 1, 24, 26, 3, 9, 7, STATS | Y, {DGRAD: _c('conv3d_dense_bwd_data_kernel'), WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 3, 3>')}),
    # the direct weight gradient asks for Wo % 4 == 0 and Q % 4 == 0; Q = To Ho Wo is a multiple of 4 whenever Wo is, so a case that holds the first
    # and fails the second cannot exist.  Wo = 4 (Q = 12): direct, one tile; Wo = 3: the narrow staged tiles <1, 1> (K = 27) and <2, 1> (Cout 40)
    ('g1_wo4', G1, 1, 3, 24, 1, 5, 8, STATS | Y, {WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 1, 1>', lambda f: f['grid'] == 1)}),
    ('g1_wg11', G1, 1, 3, 24, 1, 5, 6, STATS | Y, {WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
    ('g1_wg21', G1, 1, 3, 40, 1, 5, 6, STATS | Y, {WGRAD: _c('pw_wgrad_kernel<2, 1>')}),
    # every tensor one element past a 16-byte boundary: the direct weight gradient (aligned: <0, 2, 3, 3>) gives way to the staged one
    ('g3_ci9_misaligned', G3, 1, 9, 7, 3, 9, 8, STATS | Y | MISALIGNED,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 0, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    # one tensor off the boundary at a time (aligned: pw_gemm, allci<24>, direct <0, 2, 3, 3>): only gy / y matter, to the direct weight gradient,
    # which loads them 16 bytes at a time; it reads x one element at a time and takes it misaligned
    ('g3_ci9_mis_x', G3, 1, 9, 7, 3, 9, 8, STATS | Y | MIS_X,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 0, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 3, 3>')}),
    ('g3_ci9_mis_g', G3, 1, 9, 7, 3, 9, 8, STATS | Y | MIS_G,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 0, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_kernel<1, 2>')}),
    ('g3_ci9_mis_out', G3, 1, 9, 7, 3, 9, 8, STATS | Y | MIS_OUT,
     {FWD: _c('pw_gemm_kernel<1, 0, true, 0, true>'), DGRAD: _c('conv3d_dense_bwd_data_allci_kernel<24>'), WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 3, 3>')}),
]

STEM_CASES = [
    # (name, N, Cout, T, H, W, misaligned, claims)
    ('rb8', 2, 24, 2, 16, 12, 0, {STEM_FWD: _c('stem_fwd_kernel<3>', lambda f: f['chunk'] == 8), STEM_WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
    ('rb4_ragged', 1, 32, 3, 20, 12, 0, {STEM_FWD: _c('stem_fwd_kernel<3>', lambda f: f['chunk'] == 4 and f['bands'] == 3)}),
    ('co33', 1, 33, 1, 8, 8, 0, {STEM_FWD: _c('pw_gemm_kernel<2, 0, false, 0, true>'), STEM_WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 1, 1>')}),
    ('w_odd4', 1, 24, 2, 8, 10, 0, {STEM_FWD: _c('pw_gemm_kernel<1, 0, false, 0, true>'), STEM_WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
    ('h_odd', 1, 24, 2, 9, 8, 0, {STEM_FWD: _c('pw_gemm_kernel<1, 0, false, 0, true>')}),
    ('misaligned', 1, 24, 2, 8, 8, MISALIGNED, {STEM_FWD: _c('pw_gemm_kernel<1, 0, false, 0, true>'), STEM_WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
    ('wg224_T1', 1, 24, 1, 224, 224, 0, {STEM_FWD: _c('stem_fwd_kernel<3>', lambda f: f['chunk'] == 8), STEM_WGRAD: _c('stem_wgrad_kernel')}),
    ('wg224_T3_misaligned', 1, 24, 3, 224, 224, MISALIGNED, {STEM_WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
    # one tensor off the boundary at a time: x alone (16-byte loads in both stem kernels), the output alone (stem_fwd stores one element at a time
    # and stays), gy alone (stem_wgrad and the direct kernel load it 16 bytes at a time)
    ('mis_x', 1, 24, 2, 8, 8, MIS_X, {STEM_FWD: _c('pw_gemm_kernel<1, 0, false, 0, true>'), STEM_WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 1, 1>')}),
    ('mis_out', 1, 24, 2, 8, 8, MIS_OUT, {STEM_FWD: _c('stem_fwd_kernel<3>'), STEM_WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 1, 1>')}),
    ('mis_g', 1, 24, 2, 8, 8, MIS_G, {STEM_FWD: _c('stem_fwd_kernel<3>'), STEM_WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
    ('wg224_T1_mis_x', 1, 24, 1, 224, 224, MIS_X, {STEM_WGRAD: _c('pw_wgrad_direct_kernel<0, 2, 1, 1>')}),
    ('wg224_T1_mis_g', 1, 24, 1, 224, 224, MIS_G, {STEM_FWD: _c('stem_fwd_kernel<3>'), STEM_WGRAD: _c('pw_wgrad_kernel<1, 1>')}),
]
