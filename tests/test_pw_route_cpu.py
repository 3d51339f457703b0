"""Which kernel serves a pointwise conv call -- forward, data gradient, weight gradient, one-pass backward, strided-shortcut
backward -- asked on the host (cfn_pwconv_route: the routing functions the entry points call, no GPU).  The expected lines of
the X3D-M shapes are literals.  Kernel, template arguments, grid and workgroup of every line that runs in the default
configuration are also looked up in profiles/pw_route_parent_fine.csv / _coarse.csv, the tables of kernel traces of the commit
BEFORE the router existed (bench.py --steps 2 --warmup 1 [--stream coarse --eager] under a kernel trace): those four are the
old chains' choices, not the router's.  The traces record static LDS only, so the lds= and ws= figures are pinned from the
router's own arithmetic (unchanged formulas) and guard against later drift, no more."""
import csv
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'coarse-fine-networks_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

NONE, RELU, SWISH = 0, 1, 2
PRO, STATS, Y, ACC, MISALIGNED = 1, 2, 4, 8, 16
FWD, DGRAD = 0, 1


@pytest.fixture(scope='module')
def route():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    from cfn_hip import ops
    prev = cfn_hip.query('cfn_pw_split_terms', -1)
    cfn_hip.query('cfn_pw_split_terms', 6)
    yield ops.pwconv_route
    cfn_hip.query('cfn_pw_split_terms', prev)


def family(line):
    return line.split()[0]


def kernel(line):
    """'pws_kernel<3, 2, 0, true, 2, false, 3, 0>' out of a route line"""
    return line.split(' ', 1)[1].split(' grid=')[0]


WGRAD, FUSED, SHORT = 2, 3, 4


def model_calls(N=8, T=256, size=224, T_deep=None):
    """(name, op, (N, Cin, Cout, T, H, W, stride, act, flags)) of the pointwise convs of one X3D-M training step, from the model's
    own width and depth tables: per block conv1, conv3 and, for a stage's first block, the stride-2 shortcut; conv5 and fc1.
    The stem halves the plane, every stage halves it again (the stride sits on the depthwise conv2 and on the shortcut).
    T_deep: the frame count behind the coarse stream's Grid Pool (layers 2-4, head: T / 4 + 1).
    Per conv: the forward (op 0), then every backward entry point ops._PwConv.backward may call for it -- the one-pass backward
    (op 3; stride 1) or the strided-shortcut backward (op 4; stride 2) first, and the data gradient (op 1; for a shortcut the
    compact one on the output grid) and weight gradient (op 2) it falls back to when that one declines."""
    import x3d_fine
    planes, blocks = x3d_fine.get_inplanes('M'), x3d_fine.get_blocks('M')
    calls = []

    def conv(nm, cin, cout, t, r, stride, act, pro, acc=0, stats=STATS):
        calls.append((nm, FWD, (N, cin, cout, t, r, r, stride, act, pro | stats)))
        back = pro | Y | stats      # gsum / gsumsq arrive only where the forward returned statistics
        if stride == 1:
            calls.append((nm, FUSED, (N, cin, cout, t, r, r, 1, act, back | acc)))
            calls.append((nm, DGRAD, (N, cin, cout, t, r, r, 1, act, back | acc)))
        else:
            calls.append((nm, SHORT, (N, cin, cout, t, r, r, stride, act, back)))
            calls.append((nm, DGRAD, (N, cin, cout, t, r // stride, r // stride, 1, NONE, Y | stats)))      # compact, no epilogue
        calls.append((nm, WGRAD, (N, cin, cout, t, r, r, stride, act, back)))

    cin, res = planes[0][1], size // 2
    for li, ((mid, out), nb) in enumerate(zip(planes, blocks), 1):
        if li == 2 and T_deep:
            T = T_deep
        for b in range(nb):
            first = b == 0
            r_in, r_out = (res, res // 2) if first else (res // 2, res // 2)
            # layer1.0 reads the stem's output with bn1 + ReLU still deferred: a prologue; every other block reads a materialised tensor
            pro, act = (PRO, RELU) if (li == 1 and first) else (0, NONE)
            nm = 'layer%d.%d.' % (li, b)
            conv(nm + 'conv1', cin, mid, T, r_in, 1, act, pro, ACC if first else 0)      # stage-first: the shortcut's compact gradient rides along
            conv(nm + 'conv3', mid, out, T, r_out, 1, SWISH, PRO)
            if first:
                conv(nm + 'downsample', cin, out, T, r_in, 2, act, pro)
            cin = out
        res //= 2
    conv('conv5', cin, planes[3][0], T, res, 1, NONE, 0)
    conv('fc1', planes[3][0], 2048, T, 1, 1, NONE, 0, stats=0)
    conv('fc2', 2048, 157, T, 1, 1, NONE, 0, stats=0)
    return calls


def reached(calls, lines):
    """the calls of `calls` that run in the default configuration: a data / weight gradient only where the one-pass entry point declined"""
    out, declined = [], {}
    for (nm, op, args), line in zip(calls, lines):
        if op in (FUSED, SHORT):
            declined[nm] = line == 'declined'
            if not declined[nm]:
                out.append(line)
        elif op == FWD or declined[nm]:
            out.append(line)
    return out


# distinct (call -> route line) of the fine stream, 8 clips x 256 frames x 224 x 224
MODEL_ROUTES = {
    (0, 8, 24, 54, 256, 112, 112, 1, 1, 3):
        'pw_gemm pw_gemm_kernel<2, 0, true, 1, false> grid=1024 wg=256 lds=24576 ws=0',   # layer1.0.conv1
    (3, 8, 24, 54, 256, 112, 112, 1, 1, 15):
        'pf pw_bwd_fused_kernel<2, 1, 1> grid=1024 wg=256 lds=51968 ws=0',   # layer1.0.conv1
    (1, 8, 24, 54, 256, 112, 112, 1, 1, 15):
        'pw_gemm pw_gemm_kernel<1, 1, true, 1, false> grid=1024 wg=256 lds=25600 ws=0',   # layer1.0.conv1
    (2, 8, 24, 54, 256, 112, 112, 1, 1, 7):
        'wg pw_wgrad_kernel<2, 1> grid=640 wg=256 lds=50944 ws=0',   # layer1.0.conv1
    (0, 8, 54, 24, 256, 56, 56, 1, 2, 3):
        'pw_gemm pw_gemm_kernel<1, 0, true, 2, false> grid=1024 wg=256 lds=25600 ws=0',   # layer1.0.conv3
    (3, 8, 54, 24, 256, 56, 56, 1, 2, 7):
        'pf pw_bwd_fused_kernel<1, 2, 2> grid=1024 wg=256 lds=52864 ws=0',   # layer1.0.conv3
    (1, 8, 54, 24, 256, 56, 56, 1, 2, 7):
        'pw_gemm pw_gemm_kernel<2, 1, true, 2, false> grid=1024 wg=256 lds=24576 ws=0',   # layer1.0.conv3
    (2, 8, 54, 24, 256, 56, 56, 1, 2, 7):
        'wg pw_wgrad_kernel<1, 2> grid=640 wg=256 lds=50816 ws=0',   # layer1.0.conv3
    (0, 8, 24, 24, 256, 112, 112, 2, 1, 3):
        'pw_gemm pw_gemm_kernel<1, 0, true, 1, false> grid=1024 wg=256 lds=20992 ws=0',   # layer1.0.downsample
    (4, 8, 24, 24, 256, 112, 112, 2, 1, 7):
        'psh pw_short_bwd_kernel<1, 1, 2, 6, 1, 4, 64, 2, 1, 3> grid=1528 wg=256 lds=33664 ws=0',   # layer1.0.downsample
    (1, 8, 24, 24, 256, 56, 56, 1, 0, 6):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=1024 wg=256 lds=20992 ws=0',   # layer1.0.downsample
    (2, 8, 24, 24, 256, 112, 112, 2, 1, 7):
        'wd pw_wgrad_direct_kernel<1, 1, 3, 3> grid=256 wg=512 lds=0 ws=0',   # layer1.0.downsample
    (0, 8, 24, 54, 256, 56, 56, 1, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=1024 wg=256 lds=24576 ws=0',   # layer1.1.conv1
    (3, 8, 24, 54, 256, 56, 56, 1, 0, 6):
        'pf pw_bwd_fused_kernel<2, 1, -1> grid=1528 wg=256 lds=51968 ws=0',   # layer1.1.conv1
    (1, 8, 24, 54, 256, 56, 56, 1, 0, 6):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=1024 wg=256 lds=25600 ws=0',   # layer1.1.conv1
    (2, 8, 24, 54, 256, 56, 56, 1, 0, 6):
        'wg pw_wgrad_kernel<2, 1> grid=640 wg=256 lds=50944 ws=0',   # layer1.1.conv1
    (0, 8, 24, 108, 256, 56, 56, 1, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=1024 wg=256 lds=24576 ws=0',   # layer2.0.conv1
    (3, 8, 24, 108, 256, 56, 56, 1, 0, 14):
        'pfs pw_bwd_fused_split_kernel<4, 1, -1> grid=512 wg=512 lds=112128 ws=0',   # layer2.0.conv1
    (1, 8, 24, 108, 256, 56, 56, 1, 0, 14):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=1024 wg=256 lds=33664 ws=0',   # layer2.0.conv1
    (2, 8, 24, 108, 256, 56, 56, 1, 0, 6):
        'wg pw_wgrad_kernel<2, 1> grid=640 wg=256 lds=50944 ws=0',   # layer2.0.conv1
    (0, 8, 108, 48, 256, 28, 28, 1, 2, 3):
        'pws pws_kernel<2, 2, 0, true, 2, false, 3, 0> grid=256 wg=512 lds=81664 ws=0',   # layer2.0.conv3
    (3, 8, 108, 48, 256, 28, 28, 1, 2, 7):
        'declined',   # layer2.0.conv3
    (1, 8, 108, 48, 256, 28, 28, 1, 2, 7):
        'pws pws_kernel<4, 1, 1, true, 2, true, 3, 0> grid=256 wg=512 lds=65280 ws=0',   # layer2.0.conv3
    (2, 8, 108, 48, 256, 28, 28, 1, 2, 7):
        'pss pws_wgrad_staged_kernel<2, 1, 2, true, 3, 4, 0, 0, false> grid=256 wg=512 lds=94208 ws=8388608',   # layer2.0.conv3
    (0, 8, 24, 48, 256, 56, 56, 2, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=968 wg=256 lds=24576 ws=0',   # layer2.0.downsample
    (4, 8, 24, 48, 256, 56, 56, 2, 0, 6):
        'psh pw_short_bwd_kernel<2, 1, 2, 12, 1, 4, 64, 2, 0, 2> grid=1008 wg=256 lds=50688 ws=0',   # layer2.0.downsample
    (1, 8, 24, 48, 256, 28, 28, 1, 0, 6):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=968 wg=256 lds=24448 ws=0',   # layer2.0.downsample
    (2, 8, 24, 48, 256, 56, 56, 2, 0, 6):
        'wd pw_wgrad_direct_kernel<0, 1, 3, 3> grid=256 wg=512 lds=0 ws=0',   # layer2.0.downsample
    (0, 8, 48, 108, 256, 28, 28, 1, 0, 2):
        'pws pws_kernel<4, 1, 0, true, 0, false, 3, 0> grid=256 wg=512 lds=65280 ws=0',   # layer2.1.conv1
    (3, 8, 48, 108, 256, 28, 28, 1, 0, 6):
        'pfs pw_bwd_fused_split_kernel<4, 2, -1> grid=512 wg=512 lds=156160 ws=0',   # layer2.1.conv1
    (1, 8, 48, 108, 256, 28, 28, 1, 0, 6):
        'pws pws_kernel<2, 2, 1, false, 0, true, 3, 0> grid=256 wg=512 lds=81664 ws=0',   # layer2.1.conv1
    (2, 8, 48, 108, 256, 28, 28, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<2, 1, 0, true, 3, 4, 0, 0, false> grid=256 wg=512 lds=94720 ws=8388608',   # layer2.1.conv1
    (0, 8, 48, 216, 256, 28, 28, 1, 0, 2):
        'pwk pwk_kernel<3, 1, 0, 0, true, false> grid=256 wg=512 lds=86784 ws=0',   # layer3.0.conv1
    (3, 8, 48, 216, 256, 28, 28, 1, 0, 14):
        'pf3 pw_bwd_fused_split3_kernel<7, 2> grid=512 wg=512 lds=89856 ws=89088',   # layer3.0.conv1
    (1, 8, 48, 216, 256, 28, 28, 1, 0, 14):
        'pwk pwk_kernel<14, 2, 1, 0, false, true> grid=256 wg=512 lds=129536 ws=0 +lattice_add',   # layer3.0.conv1
    (2, 8, 48, 216, 256, 28, 28, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=256 wg=512 lds=142336 ws=14680064',   # layer3.0.conv1
    (0, 8, 216, 96, 256, 14, 14, 1, 2, 3):
        'pwk pwk_kernel<14, 2, 0, 2, true, false> grid=256 wg=512 lds=147968 ws=0',   # layer3.0.conv3
    (3, 8, 216, 96, 256, 14, 14, 1, 2, 7):
        'declined',   # layer3.0.conv3
    (1, 8, 216, 96, 256, 14, 14, 1, 2, 7):
        'pwk pwk_kernel<6, 1, 1, 2, true, true> grid=256 wg=512 lds=110592 ws=0',   # layer3.0.conv3
    (2, 8, 216, 96, 256, 14, 14, 1, 2, 7):
        'pss pws_wgrad_staged_kernel<4, 3, 2, true, 3, 4, 3, 1, true> grid=256 wg=512 lds=156928 ws=22020096',   # layer3.0.conv3
    (0, 8, 48, 96, 256, 28, 28, 2, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=896 wg=256 lds=31104 ws=0',   # layer3.0.downsample
    (4, 8, 48, 96, 256, 28, 28, 2, 0, 6):
        'psh pw_short_bwd_kernel<3, 2, 3, 24, 3, 2, 64, 2, 0, 1> grid=256 wg=384 lds=84352 ws=0',   # layer3.0.downsample
    (1, 8, 48, 96, 256, 14, 14, 1, 0, 6):
        'pws pws_kernel<2, 2, 1, false, 0, true, 3, 0> grid=256 wg=512 lds=62464 ws=0',   # layer3.0.downsample
    (2, 8, 48, 96, 256, 28, 28, 2, 0, 6):
        'wg pw_wgrad_kernel<2, 2> grid=640 wg=256 lds=67840 ws=0',   # layer3.0.downsample
    (0, 8, 96, 216, 256, 14, 14, 1, 0, 2):
        'pwk pwk_kernel<6, 1, 0, 0, true, false> grid=256 wg=512 lds=105984 ws=0',   # layer3.1.conv1
    (3, 8, 96, 216, 256, 14, 14, 1, 0, 6):
        'pf3 pw_bwd_fused_split3_kernel<7, 3> grid=256 wg=512 lds=98304 ws=133632',   # layer3.1.conv1
    (1, 8, 96, 216, 256, 14, 14, 1, 0, 6):
        'pwk pwk_kernel<14, 2, 1, 0, false, true> grid=256 wg=512 lds=147968 ws=0',   # layer3.1.conv1
    (2, 8, 96, 216, 256, 14, 14, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=256 wg=512 lds=157952 ws=22020096',   # layer3.1.conv1
    (0, 8, 96, 432, 256, 14, 14, 1, 0, 2):
        'pwk pwk_kernel<6, 1, 0, 0, true, false> grid=256 wg=512 lds=105984 ws=0',   # layer4.0.conv1
    (3, 8, 96, 432, 256, 14, 14, 1, 0, 14):
        'declined',   # layer4.0.conv1
    (1, 8, 96, 432, 256, 14, 14, 1, 0, 14):
        'pwt pws_kernel<3, 1, 1, false, 0, true, 3, 3> grid=256 wg=512 lds=92672 ws=290304 +lattice_add',   # layer4.0.conv1
    (2, 8, 96, 432, 256, 14, 14, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=256 wg=512 lds=157952 ws=22020096',   # layer4.0.conv1
    (0, 8, 432, 192, 256, 7, 7, 1, 2, 3):
        'pwt pws_kernel<6, 1, 0, true, 2, false, 3, 3> grid=256 wg=512 lds=157952 ws=580608',   # layer4.0.conv3
    (3, 8, 432, 192, 256, 7, 7, 1, 2, 7):
        'declined',   # layer4.0.conv3
    (1, 8, 432, 192, 256, 7, 7, 1, 2, 7):
        'pwt pws_kernel<5, 1, 1, true, 2, true, 3, 3> grid=240 wg=512 lds=132352 ws=645120',   # layer4.0.conv3
    (2, 8, 432, 192, 256, 7, 7, 1, 2, 7):
        'pss pws_wgrad_staged_kernel<4, 3, 2, true, 3, 4, 3, 1, true> grid=256 wg=512 lds=156928 ws=22020096',   # layer4.0.conv3
    (0, 8, 96, 192, 256, 14, 14, 2, 0, 2):
        'pw_gemm pw_gemm_kernel<1, 0, true, 0, false> grid=960 wg=256 lds=31360 ws=0',   # layer4.0.downsample
    (4, 8, 96, 192, 256, 14, 14, 2, 0, 6):
        'psh pw_short_bwd_kernel<6, 3, 6, 48, 6, 1, 32, 1, 0, 1> grid=248 wg=384 lds=78336 ws=0',   # layer4.0.downsample
    (1, 8, 96, 192, 256, 7, 7, 1, 0, 6):
        'pwk pwk_kernel<12, 2, 1, 0, false, true> grid=256 wg=512 lds=135168 ws=0',   # layer4.0.downsample
    (2, 8, 96, 192, 256, 14, 14, 2, 0, 6):
        'wg pw_wgrad_kernel<2, 2> grid=624 wg=256 lds=67840 ws=0',   # layer4.0.downsample
    (0, 8, 192, 432, 256, 7, 7, 1, 0, 2):
        'pwk pwk_kernel<12, 1, 0, 0, true, false> grid=256 wg=512 lds=144384 ws=0',   # layer4.1.conv1
    (3, 8, 192, 432, 256, 7, 7, 1, 0, 6):
        'declined',   # layer4.1.conv1
    (1, 8, 192, 432, 256, 7, 7, 1, 0, 6):
        'pwt pws_kernel<6, 1, 1, false, 0, true, 3, 3> grid=256 wg=512 lds=157952 ws=580608',   # layer4.1.conv1
    (2, 8, 192, 432, 256, 7, 7, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=256 wg=512 lds=157184 ws=25165824',   # layer4.1.conv1
    (0, 8, 432, 2048, 256, 1, 1, 1, 0, 0):
        'pwt pws_kernel<6, 1, 0, false, 0, false, 3, 3> grid=88 wg=512 lds=157952 ws=6386688',   # fc1
    (3, 8, 432, 2048, 256, 1, 1, 1, 0, 4):
        'declined',   # fc1
    (1, 8, 432, 2048, 256, 1, 1, 1, 0, 4):
        'pwt pws_kernel<5, 1, 1, false, 0, false, 3, 3> grid=24 wg=512 lds=162304 ws=6935040',   # fc1
    (2, 8, 432, 2048, 256, 1, 1, 1, 0, 4):
        'pss pws_wgrad_staged_kernel<4, 6, 0, false, 3, 4, 0, 0, false> grid=312 wg=512 lds=157440 ws=31948800',   # fc1
    (0, 8, 2048, 157, 256, 1, 1, 1, 0, 0):
        'pwt pws_kernel<5, 1, 0, false, 0, false, 3, 3> grid=8 wg=512 lds=162304 ws=2311680',   # fc2
    (3, 8, 2048, 157, 256, 1, 1, 1, 0, 4):
        'declined',   # fc2
    (1, 8, 2048, 157, 256, 1, 1, 1, 0, 4):
        'pwd pw_deep_kernel<6, 1, false, 0, 8> grid=88 wg=512 lds=160896 ws=0',   # fc2
    (2, 8, 2048, 157, 256, 1, 1, 1, 0, 4):
        'pss pws_wgrad_staged_kernel<4, 6, 0, false, 3, 4, 0, 0, false> grid=208 wg=512 lds=157440 ws=21299200',   # fc2
}

# the coarse stream, 8 clips x 64 frames: stem and layer 1 at 64 frames, layers 2-4 at 17 (layer 4: 17 x 7 x 7 = 833 positions, no multiple of 4)
COARSE_ROUTES = {
    (0, 8, 24, 54, 64, 112, 112, 1, 1, 3):
        'pw_gemm pw_gemm_kernel<2, 0, true, 1, false> grid=1024 wg=256 lds=24576 ws=0',   # layer1.0.conv1
    (3, 8, 24, 54, 64, 112, 112, 1, 1, 15):
        'pf pw_bwd_fused_kernel<2, 1, 1> grid=1024 wg=256 lds=51968 ws=0',   # layer1.0.conv1
    (1, 8, 24, 54, 64, 112, 112, 1, 1, 15):
        'pw_gemm pw_gemm_kernel<1, 1, true, 1, false> grid=1024 wg=256 lds=25600 ws=0',   # layer1.0.conv1
    (2, 8, 24, 54, 64, 112, 112, 1, 1, 7):
        'wg pw_wgrad_kernel<2, 1> grid=640 wg=256 lds=50944 ws=0',   # layer1.0.conv1
    (0, 8, 54, 24, 64, 56, 56, 1, 2, 3):
        'pw_gemm pw_gemm_kernel<1, 0, true, 2, false> grid=968 wg=256 lds=25600 ws=0',   # layer1.0.conv3
    (3, 8, 54, 24, 64, 56, 56, 1, 2, 7):
        'pf pw_bwd_fused_kernel<1, 2, 2> grid=1008 wg=256 lds=52864 ws=0',   # layer1.0.conv3
    (1, 8, 54, 24, 64, 56, 56, 1, 2, 7):
        'pw_gemm pw_gemm_kernel<2, 1, true, 2, false> grid=968 wg=256 lds=24576 ws=0',   # layer1.0.conv3
    (2, 8, 54, 24, 64, 56, 56, 1, 2, 7):
        'wg pw_wgrad_kernel<1, 2> grid=632 wg=256 lds=50816 ws=0',   # layer1.0.conv3
    (0, 8, 24, 24, 64, 112, 112, 2, 1, 3):
        'pw_gemm pw_gemm_kernel<1, 0, true, 1, false> grid=968 wg=256 lds=20992 ws=0',   # layer1.0.downsample
    (4, 8, 24, 24, 64, 112, 112, 2, 1, 7):
        'psh pw_short_bwd_kernel<1, 1, 2, 6, 1, 4, 64, 2, 1, 3> grid=1480 wg=256 lds=33664 ws=0',   # layer1.0.downsample
    (1, 8, 24, 24, 64, 56, 56, 1, 0, 6):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=968 wg=256 lds=20992 ws=0',   # layer1.0.downsample
    (2, 8, 24, 24, 64, 112, 112, 2, 1, 7):
        'wd pw_wgrad_direct_kernel<1, 1, 3, 3> grid=256 wg=512 lds=0 ws=0',   # layer1.0.downsample
    (0, 8, 24, 54, 64, 56, 56, 1, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=968 wg=256 lds=24576 ws=0',   # layer1.1.conv1
    (3, 8, 24, 54, 64, 56, 56, 1, 0, 6):
        'pf pw_bwd_fused_kernel<2, 1, -1> grid=1480 wg=256 lds=51968 ws=0',   # layer1.1.conv1
    (1, 8, 24, 54, 64, 56, 56, 1, 0, 6):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=968 wg=256 lds=25600 ws=0',   # layer1.1.conv1
    (2, 8, 24, 54, 64, 56, 56, 1, 0, 6):
        'wg pw_wgrad_kernel<2, 1> grid=632 wg=256 lds=50944 ws=0',   # layer1.1.conv1
    (0, 8, 24, 108, 17, 56, 56, 1, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=960 wg=256 lds=24576 ws=0',   # layer2.0.conv1
    (3, 8, 24, 108, 17, 56, 56, 1, 0, 14):
        'pfs pw_bwd_fused_split_kernel<4, 1, -1> grid=480 wg=512 lds=112128 ws=0',   # layer2.0.conv1
    (1, 8, 24, 108, 17, 56, 56, 1, 0, 14):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=840 wg=256 lds=33664 ws=0',   # layer2.0.conv1
    (2, 8, 24, 108, 17, 56, 56, 1, 0, 6):
        'wg pw_wgrad_kernel<2, 1> grid=640 wg=256 lds=50944 ws=0',   # layer2.0.conv1
    (0, 8, 108, 48, 17, 28, 28, 1, 2, 3):
        'pws pws_kernel<2, 2, 0, true, 2, false, 3, 0> grid=216 wg=512 lds=81664 ws=0',   # layer2.0.conv3
    (3, 8, 108, 48, 17, 28, 28, 1, 2, 7):
        'declined',   # layer2.0.conv3
    (1, 8, 108, 48, 17, 28, 28, 1, 2, 7):
        'pws pws_kernel<4, 1, 1, true, 2, true, 3, 0> grid=256 wg=512 lds=65280 ws=0',   # layer2.0.conv3
    (2, 8, 108, 48, 17, 28, 28, 1, 2, 7):
        'pss pws_wgrad_staged_kernel<2, 1, 2, true, 3, 4, 0, 0, false> grid=240 wg=512 lds=94208 ws=7864320',   # layer2.0.conv3
    (0, 8, 24, 48, 17, 56, 56, 2, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=840 wg=256 lds=24576 ws=0',   # layer2.0.downsample
    (4, 8, 24, 48, 17, 56, 56, 2, 0, 6):
        'psh pw_short_bwd_kernel<2, 1, 2, 12, 1, 4, 64, 2, 0, 2> grid=424 wg=256 lds=50688 ws=0',   # layer2.0.downsample
    (1, 8, 24, 48, 17, 28, 28, 1, 0, 6):
        'pw_gemm pw_gemm_kernel<1, 1, false, 0, false> grid=840 wg=256 lds=24448 ws=0',   # layer2.0.downsample
    (2, 8, 24, 48, 17, 56, 56, 2, 0, 6):
        'wd pw_wgrad_direct_kernel<0, 1, 3, 3> grid=256 wg=512 lds=0 ws=0',   # layer2.0.downsample
    (0, 8, 48, 108, 17, 28, 28, 1, 0, 2):
        'pws pws_kernel<4, 1, 0, true, 0, false, 3, 0> grid=256 wg=512 lds=65280 ws=0',   # layer2.1.conv1
    (3, 8, 48, 108, 17, 28, 28, 1, 0, 6):
        'pfs pw_bwd_fused_split_kernel<4, 2, -1> grid=424 wg=512 lds=156160 ws=0',   # layer2.1.conv1
    (1, 8, 48, 108, 17, 28, 28, 1, 0, 6):
        'pws pws_kernel<2, 2, 1, false, 0, true, 3, 0> grid=216 wg=512 lds=81664 ws=0',   # layer2.1.conv1
    (2, 8, 48, 108, 17, 28, 28, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<2, 1, 0, true, 3, 4, 0, 0, false> grid=240 wg=512 lds=94720 ws=7864320',   # layer2.1.conv1
    (0, 8, 48, 216, 17, 28, 28, 1, 0, 2):
        'pwk pwk_kernel<3, 1, 0, 0, true, false> grid=256 wg=512 lds=86784 ws=0',   # layer3.0.conv1
    (3, 8, 48, 216, 17, 28, 28, 1, 0, 14):
        'pf3 pw_bwd_fused_split3_kernel<7, 2> grid=240 wg=512 lds=89856 ws=89088',   # layer3.0.conv1
    (1, 8, 48, 216, 17, 28, 28, 1, 0, 14):
        'pwk pwk_kernel<14, 2, 1, 0, false, true> grid=256 wg=512 lds=129536 ws=0 +lattice_add',   # layer3.0.conv1
    (2, 8, 48, 216, 17, 28, 28, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=240 wg=512 lds=142336 ws=13762560',   # layer3.0.conv1
    (0, 8, 216, 96, 17, 14, 14, 1, 2, 3):
        'pwk pwk_kernel<14, 2, 0, 2, true, false> grid=256 wg=512 lds=147968 ws=0',   # layer3.0.conv3
    (3, 8, 216, 96, 17, 14, 14, 1, 2, 7):
        'declined',   # layer3.0.conv3
    (1, 8, 216, 96, 17, 14, 14, 1, 2, 7):
        'pwk pwk_kernel<6, 1, 1, 2, true, true> grid=256 wg=512 lds=110592 ws=0',   # layer3.0.conv3
    (2, 8, 216, 96, 17, 14, 14, 1, 2, 7):
        'pss pws_wgrad_staged_kernel<4, 3, 2, true, 3, 4, 3, 1, true> grid=216 wg=512 lds=156928 ws=18579456',   # layer3.0.conv3
    (0, 8, 48, 96, 17, 28, 28, 2, 0, 2):
        'pw_gemm pw_gemm_kernel<2, 0, true, 0, false> grid=432 wg=256 lds=31104 ws=0',   # layer3.0.downsample
    (4, 8, 48, 96, 17, 28, 28, 2, 0, 6):
        'psh pw_short_bwd_kernel<3, 2, 3, 24, 3, 2, 64, 2, 0, 1> grid=112 wg=384 lds=84352 ws=0',   # layer3.0.downsample
    (1, 8, 48, 96, 17, 14, 14, 1, 0, 6):
        'pws pws_kernel<2, 2, 1, false, 0, true, 3, 0> grid=56 wg=512 lds=62464 ws=0',   # layer3.0.downsample
    (2, 8, 48, 96, 17, 28, 28, 2, 0, 6):
        'wg pw_wgrad_kernel<2, 2> grid=224 wg=256 lds=67840 ws=0',   # layer3.0.downsample
    (0, 8, 96, 216, 17, 14, 14, 1, 0, 2):
        'pwk pwk_kernel<6, 1, 0, 0, true, false> grid=256 wg=512 lds=105984 ws=0',   # layer3.1.conv1
    (3, 8, 96, 216, 17, 14, 14, 1, 0, 6):
        'pf3 pw_bwd_fused_split3_kernel<7, 3> grid=216 wg=512 lds=98304 ws=133632',   # layer3.1.conv1
    (1, 8, 96, 216, 17, 14, 14, 1, 0, 6):
        'pwk pwk_kernel<14, 2, 1, 0, false, true> grid=256 wg=512 lds=147968 ws=0',   # layer3.1.conv1
    (2, 8, 96, 216, 17, 14, 14, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=216 wg=512 lds=157952 ws=18579456',   # layer3.1.conv1
    (0, 8, 96, 432, 17, 14, 14, 1, 0, 2):
        'pwk pwk_kernel<6, 1, 0, 0, true, false> grid=256 wg=512 lds=105984 ws=0',   # layer4.0.conv1
    (3, 8, 96, 432, 17, 14, 14, 1, 0, 14):
        'declined',   # layer4.0.conv1
    (1, 8, 96, 432, 17, 14, 14, 1, 0, 14):
        'pwt pws_kernel<3, 1, 1, false, 0, true, 3, 3> grid=112 wg=512 lds=92672 ws=290304 +lattice_add',   # layer4.0.conv1
    (2, 8, 96, 432, 17, 14, 14, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=240 wg=512 lds=157952 ws=20643840',   # layer4.0.conv1
    (0, 8, 432, 192, 17, 7, 7, 1, 2, 3):
        'pwd pw_deep_kernel<2, 0, true, 2, 8> grid=96 wg=512 lds=151936 ws=0',   # layer4.0.conv3
    (3, 8, 432, 192, 17, 7, 7, 1, 2, 7):
        'declined',   # layer4.0.conv3
    (1, 8, 432, 192, 17, 7, 7, 1, 2, 7):
        'pwt pws_kernel<5, 1, 1, true, 2, true, 3, 3> grid=96 wg=512 lds=132352 ws=645120',   # layer4.0.conv3
    (2, 8, 432, 192, 17, 7, 7, 1, 2, 7):
        'pss pws_wgrad_staged_kernel<4, 3, 2, true, 3, 4, 3, 1, true> grid=224 wg=512 lds=156928 ws=19267584',   # layer4.0.conv3
    (0, 8, 96, 192, 17, 14, 14, 2, 0, 2):
        'pw_gemm pw_gemm_kernel<1, 0, true, 0, false> grid=336 wg=256 lds=31360 ws=0',   # layer4.0.downsample
    (4, 8, 96, 192, 17, 14, 14, 2, 0, 6):
        'psh pw_short_bwd_kernel<6, 3, 6, 48, 6, 1, 32, 0, 0, 1> grid=56 wg=384 lds=78336 ws=0',   # layer4.0.downsample
    (1, 8, 96, 192, 17, 7, 7, 1, 0, 6):
        'pwd pw_deep_kernel<3, 1, false, 0, 8> grid=32 wg=512 lds=111488 ws=0',   # layer4.0.downsample
    (2, 8, 96, 192, 17, 14, 14, 2, 0, 6):
        'wg pw_wgrad_kernel<2, 2> grid=192 wg=256 lds=67840 ws=0',   # layer4.0.downsample
    (0, 8, 192, 432, 17, 7, 7, 1, 0, 2):
        'pwd pw_deep_kernel<5, 0, true, 0, 8> grid=96 wg=512 lds=161152 ws=0',   # layer4.1.conv1
    (3, 8, 192, 432, 17, 7, 7, 1, 0, 6):
        'declined',   # layer4.1.conv1
    (1, 8, 192, 432, 17, 7, 7, 1, 0, 6):
        'pwt pws_kernel<6, 1, 1, false, 0, true, 3, 3> grid=32 wg=512 lds=157952 ws=580608',   # layer4.1.conv1
    (2, 8, 192, 432, 17, 7, 7, 1, 0, 6):
        'pss pws_wgrad_staged_kernel<4, 3, 0, true, 3, 4, 1, 3, true> grid=224 wg=512 lds=157184 ws=22020096',   # layer4.1.conv1
    (0, 8, 432, 2048, 17, 1, 1, 1, 0, 0):
        'pwd pw_deep_kernel<2, 0, false, 0, 8> grid=256 wg=512 lds=151936 ws=0',   # fc1
    (3, 8, 432, 2048, 17, 1, 1, 1, 0, 4):
        'declined',   # fc1
    (1, 8, 432, 2048, 17, 1, 1, 1, 0, 4):
        'pwt pws_kernel<5, 1, 1, false, 0, false, 3, 3> grid=24 wg=512 lds=162304 ws=6935040',   # fc1
    (2, 8, 432, 2048, 17, 1, 1, 1, 0, 4):
        'pss pws_wgrad_staged_kernel<4, 6, 0, false, 3, 4, 0, 0, false> grid=312 wg=512 lds=157440 ws=31948800',   # fc1
    (0, 8, 2048, 157, 17, 1, 1, 1, 0, 0):
        'pw_gemm pw_gemm_kernel<1, 0, false, 0, false> grid=40 wg=256 lds=115840 ws=0',   # fc2
    (3, 8, 2048, 157, 17, 1, 1, 1, 0, 4):
        'declined',   # fc2
    (1, 8, 2048, 157, 17, 1, 1, 1, 0, 4):
        'pwd pw_deep_kernel<6, 1, false, 0, 8> grid=88 wg=512 lds=160896 ws=0',   # fc2
    (2, 8, 2048, 157, 17, 1, 1, 1, 0, 4):
        'pss pws_wgrad_staged_kernel<4, 6, 0, false, 3, 4, 0, 0, false> grid=104 wg=512 lds=157440 ws=10649600',   # fc2
}

# the coarse stream at 256 frames has 65 x 7 x 7 = 3,185 positions per row in layer 4 (not a multiple of 4 either)
COARSE_T256_L4_ROUTES = {
    # forward: no whole 16-byte groups, so the split-bf16 kernels decline and pw_deep_kernel runs
    (0, 8, 192, 432, 65, 7, 7, 1, 0, 2): 'pwd pw_deep_kernel<5, 0, true, 0, 8> grid=240 wg=512 lds=161152 ws=0',
    (0, 8, 432, 192, 65, 7, 7, 1, 2, 3): 'pwd pw_deep_kernel<2, 0, true, 2, 8> grid=240 wg=512 lds=151936 ws=0',
    # data gradient: pwt moves 4-byte elements both ways and takes them
    (1, 8, 432, 192, 65, 7, 7, 1, 2, 7): 'pwt pws_kernel<5, 1, 1, true, 2, true, 3, 3> grid=240 wg=512 lds=132352 ws=645120',
    (1, 8, 192, 432, 65, 7, 7, 1, 0, 6): 'pwt pws_kernel<6, 1, 1, false, 0, true, 3, 3> grid=104 wg=512 lds=157952 ws=580608',
}


def _trace(name):
    rows = set()
    with open(os.path.join(ROOT, 'profiles', name)) as fh:
        for r in csv.DictReader(fh):
            rows.add((r['Kernel_Name'], r['Grid_Size'], r['Workgroup_Size']))
    return rows


def _as_trace_row(line):
    f = dict(kv.split('=') for kv in line.split() if '=' in kv)
    grid, wg = int(f['grid']), int(f['wg'])
    return ('void %s(%s)' % (kernel(line), ARGS[family(line)]), '%dx1x1' % (grid * wg), '%dx1x1' % wg)      # a trace counts the grid in work-items


ARGS = {'pwk': 'PwArgs', 'pwt': 'PwArgs', 'pws': 'PwArgs', 'pwd': 'PwArgs', 'pw_gemm': 'PwArgs', 'pss': 'WssArgs', 'wd': 'WdArgs', 'wg': 'WgArgs',
        'pf': 'PfArgs', 'pfs': 'PfsArgs', 'pf3': 'Pf3Args', 'pf3e': 'Pf3eArgs', 'psh': 'PshArgs'}


@pytest.mark.parametrize('pinned,trace,kw', [(MODEL_ROUTES, 'pw_route_parent_fine.csv', {}),
                                             (COARSE_ROUTES, 'pw_route_parent_coarse.csv', dict(T=64, T_deep=17))], ids=['fine', 'coarse'])
def test_model_table_routes(route, pinned, trace, kw):
    """every pointwise call of the X3D-M step (shapes derived from x3d_fine's own tables), all five entry points, routes to the pinned line;
    of the lines that run in the default configuration, (kernel, grid, workgroup) is a row of the parent commit's kernel trace, and every
    pointwise contraction kernel of the fine trace is the route of some call of the table"""
    calls = model_calls(**kw)
    lines = []
    for name, op, args in calls:
        key = (op,) + args
        assert key in pinned, (name, key)
        lines.append(route(op, *args))
        assert lines[-1] == pinned[key], (name, key)
    assert {(op,) + args for _, op, args in calls} == set(pinned)
    rows = _trace(trace)
    run = {_as_trace_row(line) for line in reached(calls, lines)}
    assert not run - rows, sorted(run - rows)
    if not kw:
        # the fine trace the other way round (helpers aside: pre-split, reduce, lattice add); the coarse stream has pointwise convs of its own
        # (Grid Pool, fusion) that the table does not list
        mine = [r for r in rows if r[0].startswith('void p') and r[0].endswith(tuple('(%s)' % a for a in set(ARGS.values())))]
        assert len(mine) >= 30 and not set(mine) - run, sorted(set(mine) - run)
        # ... and every kernel with its template arguments is a row ("Name" column) of the kernel statistics committed with the strided-shortcut
        # kernel, profiles/pwshort_kernel_stats.csv, e.g. "void pwk_kernel<14, 2, 0, 2, true, false>(PwArgs)" for layer 3's conv3 forward
        with open(os.path.join(ROOT, 'profiles', 'pwshort_kernel_stats.csv')) as fh:
            names = {r['Name'] for r in csv.DictReader(fh)}
        assert not {r[0] for r in run} - names, sorted({r[0] for r in run} - names)


def test_coarse_t256_layer4_routes(route):
    for key, line in COARSE_T256_L4_ROUTES.items():
        assert route(*key) == line, key


# One shape on each side of every bound of the routing tables (csrc/pwroute.hip): (op, N, Cin, Cout, T, H, W, stride, act, flags) -> family.
# T x H x W = 2 x 4 x 4 = 32 positions unless the bound is about positions.  Forward: K = Cin, M = Cout; data gradient: K = Cout, M = Cin.
BOUNDARIES = [
    # pwk, two k slices: 128 < K <= 224 with an even number of 16-blocks, 32 < M <= 128
    ((0, 1, 128, 64, 2, 4, 4, 1, 0, 2), 'pws'), ((0, 1, 144, 64, 2, 4, 4, 1, 0, 2), 'pwd'),       # K 128 | above; 144 = 9 blocks is odd: not pwk's
    ((0, 1, 160, 64, 2, 4, 4, 1, 0, 2), 'pwk'), ((0, 1, 224, 64, 2, 4, 4, 1, 0, 2), 'pwk'), ((0, 1, 225, 64, 2, 4, 4, 1, 0, 2), 'pwd'),
    ((0, 1, 160, 32, 2, 4, 4, 1, 0, 2), 'pw_gemm'), ((0, 1, 160, 33, 2, 4, 4, 1, 0, 2), 'pwk'),
    ((0, 1, 160, 128, 2, 4, 4, 1, 0, 2), 'pwk'), ((0, 1, 160, 129, 2, 4, 4, 1, 0, 2), 'pwd'),
    # pwk, one slice: 48 <= K <= 112 (192 when M > 256), 128 < M <= 512, forward or act' epilogue (M <= 256)
    ((0, 1, 47, 160, 2, 4, 4, 1, 0, 2), 'pw_gemm'), ((0, 1, 48, 160, 2, 4, 4, 1, 0, 2), 'pwk'),
    ((0, 1, 112, 160, 2, 4, 4, 1, 0, 2), 'pwk'), ((0, 1, 113, 160, 2, 4, 4, 1, 0, 2), 'pws'),
    ((0, 1, 192, 300, 2, 4, 4, 1, 0, 2), 'pwk'), ((0, 1, 193, 300, 2, 4, 4, 1, 0, 2), 'pwd'), ((0, 1, 192, 256, 2, 4, 4, 1, 0, 2), 'pwd'),
    ((0, 1, 96, 512, 2, 4, 4, 1, 0, 2), 'pwk'), ((0, 1, 96, 513, 2, 4, 4, 1, 0, 2), 'pwd'),
    ((1, 1, 256, 96, 2, 4, 4, 1, 2, 7), 'pwk'), ((1, 1, 257, 96, 2, 4, 4, 1, 2, 7), 'pws'),       # act' epilogue: M <= 256 (K = 96 is within pws's range)
    ((1, 1, 160, 96, 2, 4, 4, 1, 0, 6), 'pws'),                                                    # no epilogue: not the one-slice kernel
    # pws: 48 <= K <= 128, M > 32, at most two slabs
    ((0, 1, 128, 33, 2, 4, 4, 1, 0, 2), 'pws'), ((0, 1, 128, 32, 2, 4, 4, 1, 0, 2), 'pw_gemm'), ((0, 1, 129, 33, 2, 4, 4, 1, 0, 2), 'pwd'),
    ((0, 1, 48, 64, 2, 4, 4, 1, 0, 2), 'pws'), ((0, 1, 47, 64, 2, 4, 4, 1, 0, 2), 'pw_gemm'),
    # pwt: M > 32 and (K >= 400, or act' epilogue with K >= 160 and M > 256)
    ((0, 1, 400, 64, 2, 4, 4, 1, 0, 2), 'pwt'), ((0, 1, 399, 64, 2, 4, 4, 1, 0, 2), 'pwd'), ((0, 1, 400, 32, 2, 4, 4, 1, 0, 2), 'pw_gemm'),
    ((1, 1, 257, 160, 2, 4, 4, 1, 2, 7), 'pwt'), ((1, 1, 257, 159, 2, 4, 4, 1, 2, 7), 'pwd'), ((1, 1, 256, 160, 2, 4, 4, 1, 2, 7), 'pwd'),
    # pwd: K >= 48 (below: pw_gemm); stride 2 is pw_gemm's
    ((0, 1, 300, 64, 2, 4, 4, 1, 0, 2), 'pwd'), ((0, 1, 300, 64, 2, 8, 8, 2, 0, 2), 'pw_gemm'),
    # Q % 4: 2 x 3 x 5 = 30 positions; the data gradient of pwt does not need whole 16-byte groups
    ((0, 1, 96, 64, 2, 3, 5, 1, 0, 2), 'pwd'), ((0, 1, 160, 64, 2, 3, 5, 1, 0, 2), 'pwd'), ((0, 1, 432, 64, 2, 3, 5, 1, 0, 2), 'pwd'),
    ((1, 1, 64, 432, 2, 3, 5, 1, 0, 6), 'pwt'),
    # tensors misaligned by 4 bytes: no 16-byte loads; pwt's data gradient only needs 4
    ((0, 1, 96, 64, 2, 4, 4, 1, 0, 2 | 16), 'pwd'), ((0, 1, 160, 64, 2, 4, 4, 1, 0, 2 | 16), 'pwd'), ((0, 1, 432, 64, 2, 4, 4, 1, 0, 2 | 16), 'pwd'),
    ((1, 1, 64, 432, 2, 4, 4, 1, 0, 6 | 16), 'pwt'),
    # the compact shortcut gradient: without an epilogue pwk / pwt run without it and the lattice add follows; with one pw_deep_kernel adds it
    ((1, 1, 96, 216, 2, 4, 4, 1, 0, 6 | 8), 'pwk'), ((1, 1, 96, 432, 2, 4, 4, 1, 0, 6 | 8), 'pwt'), ((1, 1, 96, 216, 2, 4, 4, 1, 1, 7 | 8), 'pwd'),
    ((1, 1, 96, 108, 2, 4, 4, 1, 0, 6 | 8), 'pwd'),
    # ---- one-pass backward (op 3) ----
    # pf (fp32): Cin, Cout <= 64, not both above 32
    ((3, 1, 24, 64, 2, 4, 4, 1, 0, 6), 'pf'), ((3, 1, 33, 33, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 32, 64, 2, 4, 4, 1, 0, 6), 'pf'),
    ((3, 1, 64, 32, 2, 4, 4, 1, 0, 6), 'pf'), ((3, 1, 65, 32, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 15, 65, 2, 4, 4, 1, 0, 6), 'declined'),
    ((3, 1, 24, 54, 2, 3, 5, 1, 0, 6), 'declined'), ((3, 1, 24, 54, 2, 4, 4, 1, 0, 6 | 16), 'declined'),
    # pfs (split bf16, no prologue by default): 64 < Cout <= 128 with 16 <= Cin <= 64; with a prologue (CFN_PWF_SPLIT=2) also 64 < Cin <= 128, 32 < Cout <= 64
    ((3, 1, 16, 65, 2, 4, 4, 1, 0, 6), 'pfs'), ((3, 1, 15, 100, 2, 4, 4, 1, 0, 6), 'declined'),
    ((3, 1, 32, 100, 2, 4, 4, 1, 0, 6), 'pfs'), ((3, 1, 33, 100, 2, 4, 4, 1, 0, 6), 'pfs'), ((3, 1, 64, 128, 2, 4, 4, 1, 0, 6), 'pfs'),
    ((3, 1, 65, 128, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 64, 129, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 48, 64, 2, 4, 4, 1, 0, 6), 'declined'),
    ((3, 1, 48, 108, 2, 4, 4, 1, 1, 7), 'declined'),                                               # a prologue needs CFN_PWF_SPLIT=2
    # pf3 (layer 3's conv1, no prologue): 192 < Cout <= 224, 32 < Cin <= 96
    ((3, 1, 96, 192, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 96, 193, 2, 4, 4, 1, 0, 6), 'pf3'), ((3, 1, 96, 224, 2, 4, 4, 1, 0, 6), 'pf3'),
    ((3, 1, 96, 225, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 32, 216, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 33, 216, 2, 4, 4, 1, 0, 6), 'pf3'),
    ((3, 1, 97, 216, 2, 4, 4, 1, 0, 6), 'declined'), ((3, 1, 96, 216, 2, 4, 4, 1, 1, 7), 'declined'), ((3, 1, 216, 96, 2, 4, 4, 1, 2, 7), 'declined'),
    # ---- strided-shortcut backward (op 4): Cout <= 192, Cin <= 96; variants by (Cout 24 / 48 / 96, Cin 32 / 48) ----
    ((4, 1, 32, 24, 2, 8, 8, 2, 0, 6), 'psh'), ((4, 1, 96, 192, 2, 8, 8, 2, 0, 6), 'psh'), ((4, 1, 96, 193, 2, 8, 8, 2, 0, 6), 'declined'),
    ((4, 1, 97, 192, 2, 8, 8, 2, 0, 6), 'declined'), ((4, 1, 24, 24, 2, 8, 8, 1, 0, 6), 'declined'), ((4, 1, 24, 24, 2, 8, 8, 2, 2, 7), 'declined'),
    ((4, 1, 24, 24, 2, 8, 8, 2, 0, 6 | 16), 'psh'),                                                # 4-byte alignment is enough (dword loads)
    # ---- weight gradient (op 2): pss from 48 x 48 at stride 1; stride 2: direct operands where Wo % 4 == 0, else LDS-staged ----
    ((2, 1, 48, 48, 2, 4, 4, 1, 0, 6), 'pss'), ((2, 1, 47, 48, 2, 4, 4, 1, 0, 6), 'wg'), ((2, 1, 48, 47, 2, 4, 4, 1, 0, 6), 'wg'),
    ((2, 1, 48, 96, 2, 4, 4, 1, 0, 6 | 16), 'wg'), ((2, 1, 48, 96, 2, 8, 8, 2, 0, 6), 'wd'), ((2, 1, 48, 96, 2, 6, 6, 2, 0, 6), 'wg'),
]

# the variant of the strided-shortcut kernel on each side of its width bounds: (Cin, Cout) -> leading template arguments MT, NT
PSH_VARIANTS = [((32, 24), '<1, 1,'), ((33, 24), '<3, 2,'), ((32, 25), '<2, 1,'), ((32, 48), '<2, 1,'), ((32, 49), '<3, 2,'), ((48, 96), '<3, 2,'),
                ((49, 96), '<6, 3,'), ((48, 97), '<6, 3,'), ((96, 192), '<6, 3,')]


@pytest.mark.parametrize('args,fam', BOUNDARIES)
def test_boundaries(route, args, fam):
    line = route(*args)
    assert family(line) == fam, line
    assert ('+lattice_add' in line) == (args[0] == DGRAD and bool(args[-1] & ACC) and fam in ('pwk', 'pwt')), line


@pytest.mark.parametrize('widths,targs', PSH_VARIANTS)
def test_short_variants(route, widths, targs):
    line = route(SHORT, 1, widths[0], widths[1], 2, 8, 8, 2, 0, 6)
    assert line.startswith('psh pw_short_bwd_kernel' + targs), line


def test_fused_variants_under_switches(route, monkeypatch):
    """the one-pass backward's remaining bounds need a switch: pfs with a prologue (CFN_PWF_SPLIT=2: 64 < Cin <= 128, 32 < Cout <= 64) and pf3e
    (CFN_PWF_L3E=1: 192 < Cin <= 224, 64 < Cout <= 96)"""
    monkeypatch.setenv('CFN_PWF_SPLIT', '2')
    for cin, cout, fam in [(65, 33, 'pfs'), (64, 33, 'declined'), (128, 64, 'pfs'), (129, 64, 'declined'), (65, 32, 'declined'), (128, 65, 'declined'),
                           (48, 108, 'pfs')]:
        assert family(route(FUSED, 1, cin, cout, 2, 4, 4, 1, 2, 7)) == fam, (cin, cout)
    monkeypatch.setenv('CFN_PWF_SPLIT', '1')
    monkeypatch.setenv('CFN_PWF_L3E', '1')
    for cin, cout, fam in [(193, 96, 'pf3e'), (192, 96, 'declined'), (224, 96, 'pf3e'), (225, 96, 'declined'), (216, 64, 'declined'), (216, 65, 'pf3e'),
                           (216, 97, 'declined')]:
        assert family(route(FUSED, 1, cin, cout, 2, 4, 4, 1, 2, 7)) == fam, (cin, cout)
    assert route(FUSED, 1, 216, 96, 2, 4, 4, 1, 2, 7 | ACC) == 'declined'


def test_one_pass_backward_declines(route, monkeypatch):
    """every case of test_hip_ops.PW_DECLINES (checked there on the GPU through NaN-prefilled outputs) answers `declined` on the host, under the
    same switch settings"""
    import test_hip_ops
    assert len(test_hip_ops.PW_DECLINES) >= 39
    for name, env, N, Cin, Cout, T, H, W, act, acc_s, mis in test_hip_ops.PW_DECLINES:
        with monkeypatch.context() as m:
            for k in ('CFN_PWF_SPLIT', 'CFN_PWF_L3E'):
                m.delenv(k, raising=False)
            for k, v in env.items():
                m.setenv(k, v)
            flags = STATS | Y | (PRO if act is not None else 0) | (ACC if acc_s else 0) | (MISALIGNED if mis else 0)
            assert route(FUSED, N, Cin, Cout, T, H, W, 1, act or 0, flags) == 'declined', name


def _all_routes(route):
    return {key: route(*key) for key in MODEL_ROUTES}


def test_split_terms_switch_moves_only_the_split_routes(route):
    """cfn_pw_split_terms(0): no split-bf16 family is left, the fp32 routes stay; 3: of the forward / data-gradient families pws alone stays, with two
    weight images, and the staged weight gradient runs with two terms; the one-pass split kernels need 6"""
    import cfn_hip
    fp32 = ('pwd', 'pw_gemm', 'wd', 'wg', 'pf', 'psh', 'declined')
    try:
        cfn_hip.query('cfn_pw_split_terms', 0)
        for key, got in _all_routes(route).items():
            assert family(got) in fp32, (key, got)
            if family(MODEL_ROUTES[key]) in fp32 and not (key[0] == WGRAD and family(MODEL_ROUTES[key]) == 'wg'):
                assert got == MODEL_ROUTES[key], key
        cfn_hip.query('cfn_pw_split_terms', 3)
        for key, got in _all_routes(route).items():
            line = MODEL_ROUTES[key]
            assert family(got) in fp32 + ('pws', 'pss'), (key, got)
            if family(line) == 'pws':
                assert kernel(got) == kernel(line).replace(', 3, 0>', ', 2, 0>'), (key, got)
            if family(line) == 'pss':
                assert family(got) == 'pss' and ', 2, 4, ' in kernel(got), (key, got)
            if family(line) in ('pwd', 'pw_gemm', 'wd', 'wg', 'pf', 'psh'):
                assert got == line, key
    finally:
        cfn_hip.query('cfn_pw_split_terms', 6)


# what each backward switch moves in the model table (INTEGRATION.md's table), as (op, family before) -> family after; every other route stays
SWITCH_MOVES = [
    ('CFN_PW_SHORT', '0', {(SHORT, 'psh'): 'declined'}),                                            # the two separate kernels
    ('CFN_PWF_SPLIT', '0', {(FUSED, 'pfs'): 'declined', (FUSED, 'pf3'): 'declined'}),               # the one-pass split kernels off; the fp32 one stays
    ('CFN_PWF_SPLIT', '1', {}),                                                                     # the default
    ('CFN_PWF_SPLIT', '2', {(FUSED, 'declined', 108, 48): 'pfs'}),                                  # also layer 2's conv3 (prologue)
    ('CFN_PWF_L3E', '1', {(FUSED, 'declined', 216, 96): 'pf3e'}),                                   # also layer 3's conv3
]


@pytest.mark.parametrize('name,value,moves', SWITCH_MOVES, ids=['%s=%s' % m[:2] for m in SWITCH_MOVES])
def test_backward_switches_move_exactly_their_routes(route, monkeypatch, name, value, moves):
    for k in ('CFN_PW_SHORT', 'CFN_PWF_SPLIT', 'CFN_PWF_L3E'):
        monkeypatch.delenv(k, raising=False)
    assert _all_routes(route) == MODEL_ROUTES                # unset = the defaults
    monkeypatch.setenv(name, value)
    moved = 0
    for key, got in _all_routes(route).items():
        line = MODEL_ROUTES[key]
        want = moves.get((key[0], family(line)), moves.get((key[0], family(line), key[2], key[3])))
        if want is None:
            assert got == line, (key, got)
        else:
            assert family(got) == want, (key, got)
            moved += 1
    assert (moved > 0) == bool(moves)


def _gpu_case_kernels(route):
    """the forward / data-gradient kernels the existing GPU lists reach at their own small sizes, with the options their tests pass:
    PW_CASES (test_pwconv: forward with statistics, backward through ops.pwconv with gs / gq / y; the listed act and prologue),
    SPLIT_CASES (test_pwconv_split: the same), PWK_CASES and PWT_CASES (forward with prologue + statistics, act 0 / 2; data gradient
    without epilogue, with and without the y operand), PWK1_CASES (forward only), PWK_ACT_DGRAD (data gradient with act' epilogue)"""
    import test_hip_ops
    import test_hip_split
    out = set()

    def both(N, Cin, Cout, T, H, W, stride, act, pro):
        p = PRO if pro else 0
        out.add(kernel(route(FWD, N, Cin, Cout, T, H, W, stride, act, p | STATS)))
        if route(FUSED, N, Cin, Cout, T, H, W, 1, act, p | STATS | Y) == 'declined' or stride != 1:
            out.add(kernel(route(DGRAD, N, Cin, Cout, T, H, W, stride, act, p | STATS | Y)))

    for c in test_hip_ops.PW_CASES:
        both(*c)
    for N, Cin, Cout, T, H, W, act, pro in test_hip_split.SPLIT_CASES:
        both(N, Cin, Cout, T, H, W, 1, act, pro)
    for lst in (test_hip_split.PWK_CASES, test_hip_split.PWT_CASES, test_hip_split.PWK1_CASES):
        for N, K, M, T, H, W in lst:
            for act in (NONE, SWISH):
                out.add(kernel(route(FWD, N, K, M, T, H, W, 1, act, PRO | STATS)))
            if lst is test_hip_split.PWT_CASES:      # test_pwt_forward_vs_fp64 repeats the forward without statistics
                for act in (NONE, SWISH):
                    out.add(kernel(route(FWD, N, K, M, T, H, W, 1, act, PRO)))
            if lst is not test_hip_split.PWK1_CASES:
                for flags in (STATS, STATS | Y):
                    out.add(kernel(route(DGRAD, N, M, K, T, H, W, 1, NONE, flags)))
    for case in test_hip_split.PWK_ACT_DGRAD:
        N, Ci, Co, T, H, W, act = case
        out.add(kernel(route(DGRAD, N, Ci, Co, T, H, W, 1, act, PRO | STATS | Y)))
    return out


def test_every_model_kernel_is_reached_by_a_small_gpu_case(route):
    """forward / data-gradient kernels of the model tables that run in the default configuration"""
    reached_small = _gpu_case_kernels(route)
    want = set()
    for pinned, kw in ((MODEL_ROUTES, {}), (COARSE_ROUTES, dict(T=64, T_deep=17))):
        calls = model_calls(**kw)
        for line in reached(calls, [pinned[(op,) + a] for _, op, a in calls]):
            if family(line) in ('pwk', 'pwt', 'pws', 'pwd', 'pw_gemm'):
                want.add(kernel(line))
    # The head convs run WITHOUT statistics, and in the coarse stream on 17 positions per row, so on the fp32 kernels' STATS = false forward
    # instances.  No GPU list's test passes stats=False to a conv outside the streamed-weight range (test_pwconv always asks for statistics), so
    # no list can reach these two at any size; the whole-model tests and smoke() run them.
    NO_SMALL_CASE = {'pw_deep_kernel<2, 0, false, 0, 8>', 'pw_gemm_kernel<1, 0, false, 0, false>'}
    assert want - reached_small == NO_SMALL_CASE, sorted(want - reached_small)
