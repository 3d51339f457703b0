"""Which kernel serves a dense conv call (saliency convs, stem on fp32 clips and on uint8 frames, generic shapes), asked on the host:
cfn_conv3d_dense_route, the plan functions the launchers call.  The lines of the benchmark's saliency and stem shapes at 256 CUs are literals and are looked up in
profiles/dense_route_parent_coarse.csv / _coarse_t256.csv, the kernel traces of the commit BEFORE the plans were split from the launchers
(bench.py --stream coarse [--frames 256] --steps 2 --warmup 1 under a kernel trace).  The traces record static LDS only (68096 bytes for
stem_wgrad_kernel, 0 elsewhere); lds= is the DYNAMIC LDS a launcher asks for (0 for stem_wgrad_kernel), pinned from the plans' own
arithmetic and not comparable with that column.  Every case of tests/test_hip_dense.py is asked here
at 256 CUs for the kernel and the branch its comment in tests/dense_ref64.py claims."""
import csv
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'coarse-fine-networks_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import dense_ref64 as R      # noqa: E402
from dense_ref64 import (DGRAD, FWD, MIS_G, MIS_OUT, MIS_X, MISALIGNED, PRO, SAL, STATS, STEM, STEM_FWD, STEM_U8_FWD, STEM_U8_WGRAD,      # noqa: E402
                         STEM_WGRAD, SWISH, WGRAD, Y)


@pytest.fixture(scope='module')
def route():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    from cfn_hip import ops
    prev = cfn_hip.query('cfn_pw_split_terms', -1)
    cfn_hip.query('cfn_pw_split_terms', 6)
    yield lambda op, N, Ci, Co, T, H, W, g=None, flags=0, cus=256: ops.conv3d_dense_route(op, N, Ci, Co, T, H, W, g, flags, cus)
    cfn_hip.query('cfn_pw_split_terms', prev)


# the dense convs of the coarse stream's step, 8 clips: Grid Pool conv1 (layer-1 output, 56 x 56), conv2 (28 x 28, bn1 + ReLU as prologue),
# conv3 (1x3x3 to one channel, 14 x 14), the stem: (op, N, Cin, Cout, T, H, W, geom, flags) -> line at 256 CUs
def bench_routes(T):
    T2, T3 = (T - 1) // 2 + 1, ((T - 1) // 2 + 1 - 1) // 2 + 1
    return [(FWD, 8, 24, 24, T, 56, 56, SAL, STATS), (DGRAD, 8, 24, 24, T, 56, 56, SAL, STATS | Y), (WGRAD, 8, 24, 24, T, 56, 56, SAL, STATS | Y),
            (FWD, 8, 24, 24, T2, 28, 28, SAL, PRO | STATS), (DGRAD, 8, 24, 24, T2, 28, 28, SAL, PRO | STATS | Y), (WGRAD, 8, 24, 24, T2, 28, 28, SAL, PRO | STATS | Y),
            (FWD, 8, 24, 1, T3, 14, 14, STEM, PRO), (DGRAD, 8, 24, 1, T3, 14, 14, STEM, PRO), (WGRAD, 8, 24, 1, T3, 14, 14, STEM, PRO),
            (STEM_FWD, 8, 3, 24, T, 224, 224, None, 0), (STEM_WGRAD, 8, 3, 24, T, 224, 224, None, 0)]


BENCH_LINES = {
    64: ['salb sal_fwdb_kernel<56, false> grid=3584 wg=256 lds=65632 bands=28 chunk=2 nchunks=16 last=2 items=3584',
         'sal sal_dgrad_kernel<56, false, true> grid=224 wg=512 lds=124032 bands=7 chunk=4 nchunks=8 last=4 items=448',
         'sal sal_wgrad_kernel<56, false, true> grid=224 wg=512 lds=92256 bands=14 chunk=16 nchunks=2 last=16 items=224',
         'salb sal_fwdb_kernel<28, true> grid=448 wg=256 lds=58144 bands=7 chunk=2 nchunks=8 last=2 items=448',
         'sal sal_dgrad_kernel<28, true, true> grid=64 wg=512 lds=117888 bands=2 chunk=2 nchunks=8 last=2 items=128',
         'sal sal_wgrad_kernel<28, true, true> grid=256 wg=512 lds=88800 bands=4 chunk=2 nchunks=8 last=2 items=256',
         'pw_gemm pw_gemm_kernel<1, 0, false, 1, true> grid=56 wg=256 lds=50432',
         'allci conv3d_dense_bwd_data_allci_kernel<24> grid=4x8x4 wg=256 lds=1640',
         'wg pw_wgrad_kernel<1, 2> grid=128 wg=256 lds=50816',
         'stem stem_fwd_kernel<3> grid=7168 wg=256 lds=47328 bands=14 chunk=8 items=7168',
         'stem stem_wgrad_kernel grid=512 wg=512 lds=0 bands=28 chunk=28 items=14336'],
    # 256 frames: the production chunk lengths -- forward TO = 8, data gradient CH = 16, weight gradient CH = 8 with 7 items per workgroup
    256: ['salb sal_fwdb_kernel<56, false> grid=3584 wg=256 lds=65632 bands=28 chunk=8 nchunks=16 last=8 items=3584',
          'sal sal_dgrad_kernel<56, false, true> grid=224 wg=512 lds=124032 bands=7 chunk=16 nchunks=8 last=16 items=448',
          'sal sal_wgrad_kernel<56, false, true> grid=256 wg=512 lds=92256 bands=14 chunk=8 nchunks=16 last=8 items=1792',
          'salb sal_fwdb_kernel<28, true> grid=448 wg=256 lds=58144 bands=7 chunk=8 nchunks=8 last=8 items=448',
          'sal sal_dgrad_kernel<28, true, true> grid=256 wg=512 lds=117888 bands=2 chunk=2 nchunks=32 last=2 items=512',
          'sal sal_wgrad_kernel<28, true, true> grid=256 wg=512 lds=88800 bands=4 chunk=8 nchunks=8 last=8 items=256',
          'pw_gemm pw_gemm_kernel<1, 0, false, 1, true> grid=200 wg=256 lds=50432',
          'allci conv3d_dense_bwd_data_allci_kernel<24> grid=13x8x4 wg=256 lds=1640',
          'wg pw_wgrad_kernel<1, 2> grid=416 wg=256 lds=50816',
          'stem stem_fwd_kernel<3> grid=28672 wg=256 lds=47328 bands=14 chunk=8 items=28672',
          'stem stem_wgrad_kernel grid=512 wg=512 lds=0 bands=28 chunk=112 items=57344'],
}

ARGS = {'sal_fwdb_kernel': 'SalBArgs', 'sal_fwd_kernel': 'SalArgs', 'sal_dgrad_kernel': 'SalBwdArgs', 'sal_wgrad_kernel': 'SalBwdArgs',
        'conv3d_dense_bwd_data_allci_kernel': 'DenseBwdArgs', 'conv3d_dense_bwd_data_kernel': 'DenseBwdArgs', 'pw_gemm_kernel': 'PwArgs',
        'pw_wgrad_kernel': 'WgArgs', 'pw_wgrad_direct_kernel': 'WdArgs', 'stem_fwd_kernel': 'StemArgs', 'stem_wgrad_kernel': 'StemWgArgs',
        'stem_u8_fwd_kernel': 'StemU8Args', 'stem_u8_wgrad_kernel': 'StemWgU8Args'}

# the stem on uint8 frames (8 x T x 224 x 224 x 3), forward and weight gradient: grid, bands and chunk of the fp32 lines above (one plan serves both
# sources); the forward's LDS holds the (3, 256) table behind the image: 47328 + 3072
BENCH_U8_LINES = {
    64: ['stem stem_u8_fwd_kernel grid=7168 wg=256 lds=50400 bands=14 chunk=8 items=7168',
         'stem stem_u8_wgrad_kernel grid=512 wg=512 lds=0 bands=28 chunk=28 items=14336'],
    256: ['stem stem_u8_fwd_kernel grid=28672 wg=256 lds=50400 bands=14 chunk=8 items=28672',
          'stem stem_u8_wgrad_kernel grid=512 wg=512 lds=0 bands=28 chunk=112 items=57344'],
}


def as_trace_row(line):
    """(Kernel_Name, Grid_Size, Workgroup_Size) as a kernel trace prints the launch: templates carry 'void', the grid counts work-items"""
    f = R.fields(line)
    k = f['kernel']
    name = '%s%s(%s)' % ('void ' if '<' in k else '', k, ARGS[k.split('<')[0]])
    g = [int(v) for v in str(f['grid']).split('x')] + [1, 1]
    return (name, '%dx%dx%d' % (g[0] * f['wg'], g[1], g[2]), '%dx1x1' % f['wg'])


@pytest.mark.parametrize('T,trace', [(64, 'dense_route_parent_coarse.csv'), (256, 'dense_route_parent_coarse_t256.csv')])
def test_benchmark_routes_match_parent_trace(route, T, trace):
    with open(os.path.join(ROOT, 'profiles', trace)) as fh:
        rows = {(r['Kernel_Name'], r['Grid_Size'], r['Workgroup_Size']) for r in csv.DictReader(fh)}
    for call, want in zip(bench_routes(T), BENCH_LINES[T]):
        line = route(*call)
        assert line == want, call
        assert as_trace_row(line) in rows, (call, as_trace_row(line))
    # the other way round: every saliency / stem / dense data-gradient launch of the trace is the route of one of the calls
    mine = {r for r in rows if r[0].split('(')[0].replace('void ', '').split('<')[0] in
            ('sal_fwdb_kernel', 'sal_fwd_kernel', 'sal_dgrad_kernel', 'sal_wgrad_kernel', 'conv3d_dense_bwd_data_allci_kernel',
             'conv3d_dense_bwd_data_kernel', 'stem_fwd_kernel', 'stem_wgrad_kernel')}
    assert len(mine) == 9 and mine <= {as_trace_row(w) for w in BENCH_LINES[T]}


@pytest.mark.parametrize('T', [64, 256])
def test_benchmark_u8_routes_share_the_fp32_plan(route, T):
    for op, want, f32 in zip((STEM_U8_FWD, STEM_U8_WGRAD), BENCH_U8_LINES[T], BENCH_LINES[T][-2:]):
        line = route(op, 8, 3, 24, T, 224, 224)
        assert line == want
        f, g = R.fields(line), R.fields(f32)
        assert all(f[k] == g[k] for k in ('family', 'grid', 'wg', 'bands', 'chunk', 'items'))
        assert f['lds'] - g['lds'] == (3 * 256 * 4 if op == STEM_U8_FWD else 0)
        assert as_trace_row(line)[0] == '%s(%s)' % (f['kernel'], ARGS[f['kernel']]) and as_trace_row(line)[1:] == as_trace_row(f32)[1:]


def _claims():
    out = []
    for name, g, N, Ci, Co, T, H, W, flags, claims in R.SAL_CASES + R.LONG_CASES + R.GENERIC_CASES:
        for op, (kernel, pred) in claims.items():
            out.append(pytest.param(op, (N, Ci, Co, T, H, W, g, flags if op else flags & ~Y), kernel, pred, id='%s-op%d' % (name, op)))
    for name, N, Co, T, H, W, mis, claims in R.STEM_CASES:
        for op, (kernel, pred) in claims.items():
            out.append(pytest.param(op, (N, 3, Co, T, H, W, None, mis), kernel, pred, id='stem_%s-op%d' % (name, op)))
    return out


@pytest.mark.parametrize('op,args,kernel,pred', _claims())
def test_gpu_case_reaches_its_branch(route, op, args, kernel, pred):
    line = route(op, *args)
    f = R.fields(line)
    assert f['kernel'] == kernel, line
    assert pred is None or pred(f), line


def test_long_case_inputs_stay_under_the_ceiling():
    for name, g, N, Ci, Co, T, H, W, flags, claims in R.LONG_CASES:
        assert N * Ci * T * H * W * 4 < 100e6, name


def test_no_benchmark_data_gradient_plan_under_the_ceiling(route):
    """CH = 16 of the data gradient at 8 x 56 x 56 (the benchmark's plan) needs more than 100 MB of input: tests/test_hip_dense.py lists it
    as not reached"""
    for T in range(1, 42):      # 8 x 24 x 41 x 56 x 56 x 4 B = 99 MB
        assert R.fields(route(DGRAD, 8, 24, 24, T, 56, 56, SAL, STATS | Y))['chunk'] < 16, T
    assert R.fields(route(FWD, 8, 24, 24, 28, 56, 56, SAL, STATS))['chunk'] < 8      # ... and T = 29 is the forward's shortest


DECLINES = [
    # (op, args, family that runs instead) -- the sal kernels decline ...
    (DGRAD, (1, 24, 25, 3, 8, 28, SAL, STATS | Y), 'perch'), (DGRAD, (1, 24, 32, 3, 8, 28, SAL, STATS | Y), 'perch'),      # Cout 25 .. 32 (forward only)
    (DGRAD, (1, 24, 23, 3, 8, 28, SAL, STATS | Y), 'allci'), (WGRAD, (1, 24, 23, 3, 8, 28, SAL, STATS | Y), 'wg'),
    (WGRAD, (1, 24, 25, 3, 8, 28, SAL, STATS | Y), 'wg'), (WGRAD, (1, 24, 32, 3, 8, 28, SAL, STATS | Y), 'wg'),
    (FWD, (1, 24, 32, 3, 8, 28, SAL, STATS), 'salb'), (FWD, (1, 24, 33, 3, 8, 28, SAL, STATS), 'pw_gemm'),
    (FWD, (1, 24, 24, 3, 8, 32, SAL, STATS), 'pw_gemm'), (DGRAD, (1, 24, 24, 3, 8, 32, SAL, STATS | Y), 'allci'), (WGRAD, (1, 24, 24, 3, 8, 32, SAL, STATS | Y), 'wd'),      # Wi
    (FWD, (1, 24, 24, 3, 9, 28, SAL, STATS), 'pw_gemm'), (DGRAD, (1, 24, 24, 3, 9, 28, SAL, STATS | Y), 'allci'), (WGRAD, (1, 24, 24, 3, 9, 28, SAL, STATS | Y), 'wg'),       # odd Hi
    (FWD, (1, 23, 24, 3, 8, 28, SAL, STATS), 'pw_gemm'), (FWD, (1, 24, 24, 3, 8, 28, STEM, STATS), 'pw_gemm'),             # Cin, geometry
    (DGRAD, (1, 24, 24, 3, 8, 28, SAL, PRO | SWISH | STATS | Y), 'allci'), (WGRAD, (1, 24, 24, 3, 8, 28, SAL, PRO | SWISH | STATS | Y), 'wg'),      # Swish prologue
    (FWD, (1, 24, 24, 3, 8, 28, SAL, PRO | SWISH | STATS), 'declined'),                                                      # the forward refuses it
    (FWD, (1, 24, 24, 3, 8, 28, SAL, STATS | MISALIGNED), 'pw_gemm'), (WGRAD, (1, 24, 24, 3, 8, 28, SAL, STATS | Y | MISALIGNED), 'wg'),      # misaligned
    (DGRAD, (1, 24, 24, 3, 8, 28, SAL, STATS | Y | MISALIGNED), 'allci'),      # ... the data gradient too: it moves 8 bytes at a time
    # the stem kernels
    (STEM_FWD, (1, 3, 33, 2, 8, 8, None, 0), 'pw_gemm'), (STEM_FWD, (1, 3, 32, 2, 8, 8, None, 0), 'stem'), (STEM_FWD, (1, 4, 24, 2, 8, 8, None, 0), 'pw_gemm'),
    (STEM_FWD, (1, 3, 24, 2, 8, 10, None, 0), 'pw_gemm'), (STEM_FWD, (1, 3, 24, 2, 9, 8, None, 0), 'pw_gemm'), (STEM_FWD, (1, 3, 24, 2, 8, 8, None, MISALIGNED), 'pw_gemm'),
    (STEM_WGRAD, (1, 3, 24, 2, 224, 224, None, 0), 'stem'), (STEM_WGRAD, (1, 3, 24, 2, 224, 216, None, 0), 'wd'), (STEM_WGRAD, (1, 3, 25, 2, 224, 224, None, 0), 'wd'),
    (STEM_WGRAD, (1, 3, 24, 2, 224, 224, None, MISALIGNED), 'wg'),
    # the direct weight gradient: Wo % 4 and Q % 4
    (WGRAD, (1, 3, 24, 1, 5, 8, STEM, 0), 'wd'), (WGRAD, (1, 3, 24, 1, 5, 6, STEM, 0), 'wg'), (WGRAD, (1, 3, 24, 1, 5, 8, STEM, MISALIGNED), 'wg'),
]


# every clause of the alignment gates on its own: ONE tensor 4 bytes off a 16-byte boundary (x; gy and y; the output) -> family
B = STATS | Y
ALIGNMENT = [
    # forward: x (16-byte loads) declines, y (stored one element at a time) does not; there is no gy
    (FWD, (1, 24, 24, 3, 8, 28, SAL, STATS | MIS_X), 'pw_gemm'), (FWD, (1, 24, 24, 3, 8, 28, SAL, STATS | MIS_OUT), 'salb'),
    (FWD, (1, 24, 24, 3, 8, 28, SAL, STATS | MIS_G), 'salb'),
    # data gradient: gy / y and gx (8-byte units) decline; x only where the prologue reads it
    (DGRAD, (1, 24, 24, 3, 8, 28, SAL, B | MIS_G), 'allci'), (DGRAD, (1, 24, 24, 3, 8, 28, SAL, B | MIS_OUT), 'allci'),
    (DGRAD, (1, 24, 24, 3, 8, 28, SAL, B | MIS_X), 'sal'), (DGRAD, (1, 24, 24, 3, 8, 28, SAL, B | PRO | MIS_X), 'allci'),
    (DGRAD, (1, 24, 24, 3, 8, 28, SAL, B | PRO), 'sal'),
    # weight gradient: x (16-byte loads) and gy / y (8-byte loads) decline; the output is the fp64 gw
    (WGRAD, (1, 24, 24, 3, 8, 28, SAL, B | MIS_X), 'wg'), (WGRAD, (1, 24, 24, 3, 8, 28, SAL, B | MIS_G), 'wg'), (WGRAD, (1, 24, 24, 3, 8, 28, SAL, B | MIS_OUT), 'sal'),
    # the direct weight gradient: gy / y alone
    (WGRAD, (1, 9, 7, 3, 9, 8, SAL, B | MIS_X), 'wd'), (WGRAD, (1, 9, 7, 3, 9, 8, SAL, B | MIS_G), 'wg'), (WGRAD, (1, 9, 7, 3, 9, 8, SAL, B | MIS_OUT), 'wd'),
    # stem: x declines in both kernels, gy in the weight gradient, the forward's y nowhere
    (STEM_FWD, (1, 3, 24, 2, 8, 8, None, MIS_X), 'pw_gemm'), (STEM_FWD, (1, 3, 24, 2, 8, 8, None, MIS_OUT), 'stem'), (STEM_FWD, (1, 3, 24, 2, 8, 8, None, MIS_G), 'stem'),
    (STEM_WGRAD, (1, 3, 24, 2, 224, 224, None, MIS_X), 'wd'), (STEM_WGRAD, (1, 3, 24, 2, 224, 224, None, MIS_G), 'wg'), (STEM_WGRAD, (1, 3, 24, 2, 224, 224, None, MIS_OUT), 'stem'),
]


@pytest.mark.parametrize('op,args,fam', ALIGNMENT)
def test_alignment_gates_one_tensor_at_a_time(route, op, args, fam):
    assert R.fields(route(op, *args))['family'] == fam, route(op, *args)


def test_data_gradient_refuses_what_the_entry_point_refuses(route):
    """N * Cin beyond grid.y: cfn_conv3d_dense_bwd_data fails whatever the kernel"""
    assert route(DGRAD, 2731, 24, 24, 1, 2, 28, SAL, B) == 'declined' and route(DGRAD, 2730, 24, 24, 1, 2, 28, SAL, B) != 'declined'


@pytest.mark.parametrize('op,args,fam', DECLINES)
def test_declines(route, op, args, fam):
    assert R.fields(route(op, *args))['family'] == fam, route(op, *args)


# uint8 frames (ops 5, 6): (op, args, the uint8 kernel takes the call, family that runs -- behind 'convert ' where it does not)
U8_ROUTES = [
    (STEM_U8_FWD, (3, 3, 24, 3, 30, 35, None, 0), False, 'pw_gemm'),                  # W % 4 != 0
    (STEM_U8_FWD, (2, 3, 24, 2, 33, 36, None, 0), False, 'pw_gemm'),                  # odd H
    (STEM_U8_FWD, (1, 3, 33, 2, 8, 8, None, 0), False, 'pw_gemm'), (STEM_U8_FWD, (1, 3, 32, 2, 8, 8, None, 0), True, 'stem'),      # Cout
    # frames off a 4-byte boundary: converted into a new, aligned clip, which the fp32 kernel takes
    (STEM_U8_FWD, (1, 3, 24, 2, 8, 8, None, MIS_X), False, 'stem'), (STEM_U8_FWD, (1, 3, 24, 2, 8, 8, None, MISALIGNED), False, 'stem'),
    (STEM_U8_FWD, (1, 3, 24, 2, 8, 8, None, MIS_OUT | MIS_G), True, 'stem'),
    # 8-row bands at Wi = 312: the image alone fits 64 KiB (65280 B), image + table (68352 B) does not; 4-row bands: both fit
    (STEM_FWD, (1, 3, 24, 1, 16, 312, None, 0), True, 'stem'), (STEM_U8_FWD, (1, 3, 24, 1, 16, 312, None, 0), False, 'stem'),
    (STEM_FWD, (1, 3, 24, 1, 24, 312, None, 0), True, 'stem'), (STEM_U8_FWD, (1, 3, 24, 1, 24, 312, None, 0), True, 'stem'),
    (STEM_U8_WGRAD, (1, 3, 24, 2, 224, 224, None, 0), True, 'stem'), (STEM_U8_WGRAD, (1, 3, 24, 2, 224, 224, None, MIS_OUT), True, 'stem'),
    (STEM_U8_WGRAD, (2, 3, 24, 3, 160, 160, None, 0), False, 'wd'),                   # anything but 224 x 224
    (STEM_U8_WGRAD, (1, 3, 25, 2, 224, 224, None, 0), False, 'wd'),                   # Cout
    (STEM_U8_WGRAD, (1, 3, 24, 2, 224, 224, None, MIS_G), False, 'wg'),               # gy: misaligned for the fp32 kernels too
    (STEM_U8_WGRAD, (1, 3, 24, 2, 224, 224, None, MIS_X), False, 'stem'),             # frames: the converted clip is aligned
    (STEM_U8_WGRAD, (1, 3, 24, 2, 224, 224, None, MISALIGNED), False, 'wg'),
]


def _behind_conversion(flags):
    """the flags of the fp32 call that follows a conversion: the clip is a new allocation and aligned, the other tensors are the caller's"""
    return (flags & ~(MIS_X | MISALIGNED)) | ((MIS_G | MIS_OUT) if flags & MISALIGNED else 0)


@pytest.mark.parametrize('op,args,takes,fam', U8_ROUTES)
def test_u8_stem_routes(route, op, args, takes, fam):
    line = route(op, *args)
    if op in (STEM_FWD, STEM_WGRAD):
        assert takes and R.fields(line)['family'] == fam, line
        return
    f32 = route(op - 2, *args[:-1], _behind_conversion(args[-1]))
    assert line.startswith('convert ') == (not takes), line
    if takes:
        assert R.fields(line)['family'] == fam and R.fields(line)['kernel'] == ('stem_u8_fwd_kernel' if op == STEM_U8_FWD else 'stem_u8_wgrad_kernel'), line
        assert all(R.fields(line)[k] == R.fields(f32)[k] for k in ('family', 'grid', 'wg', 'bands', 'chunk', 'items')), (line, f32)
    else:
        assert line == 'convert ' + f32 and R.fields(f32)['family'] == fam, (line, f32)


def test_u8_stem_route_parts_from_fp32_at_the_lds_ceiling(route):
    a, b = route(STEM_FWD, 1, 3, 24, 1, 16, 312), route(STEM_U8_FWD, 1, 3, 24, 1, 16, 312)
    assert R.fields(a)['lds'] == 65280 and R.fields(a)['chunk'] == 8 and b == 'convert ' + a
    a, b = R.fields(route(STEM_FWD, 1, 3, 24, 1, 24, 312)), R.fields(route(STEM_U8_FWD, 1, 3, 24, 1, 24, 312))
    assert a['chunk'] == b['chunk'] == 4 and b['lds'] == a['lds'] + 3072 and b['kernel'] == 'stem_u8_fwd_kernel'


def test_u8_stem_route_refuses_what_the_entry_point_refuses(route):
    """uint8 frames have 3 interleaved channels: cfn_stem_conv_u8_fwd / _bwd_weight fail for any other Cimg"""
    assert route(STEM_U8_FWD, 1, 4, 24, 2, 8, 8) == 'declined' and route(STEM_U8_WGRAD, 1, 1, 24, 1, 224, 224) == 'declined'
    with pytest.raises(RuntimeError, match='0 .. 6'):
        route(7, 1, 3, 24, 1, 8, 8)


def test_exact_forward_runs_when_the_split_is_off(route):
    import cfn_hip
    prev = cfn_hip.query('cfn_pw_split_terms', 0)
    try:
        line = route(FWD, 2, 24, 24, 5, 20, 56, SAL, STATS)
        assert line.startswith('sal sal_fwd_kernel<56, 1, false> grid=40 wg=256'), line
        assert R.fields(line)['chunk'] == 2 and R.fields(line)['last'] == 1
        cfn_hip.query('cfn_pw_split_terms', 3)
        assert R.fields(route(FWD, 2, 24, 24, 5, 20, 56, SAL, STATS))['kernel'] == 'sal_fwd_kernel<56, 1, false>'
    finally:
        cfn_hip.query('cfn_pw_split_terms', prev)


def test_cus_changes_the_chunk_not_the_kernel(route):
    a, b = R.fields(route(FWD, 8, 24, 24, 29, 56, 56, SAL, STATS, 256)), R.fields(route(FWD, 8, 24, 24, 29, 56, 56, SAL, STATS, 64))
    assert a['kernel'] == b['kernel'] and a['chunk'] == 8 and b['chunk'] != 8
