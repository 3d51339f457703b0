"""Which kernel serves a depthwise 3x3x3 conv call -- forward, data gradient, weight gradient, one-pass backward, for fp32, bf16 and fp16
tensors -- asked on the host (cfn_dwconv3d_route: the routing function the entry points call, no GPU).  The expected lines of the X3D-M
shapes are literals.  Kernel, template arguments, grid and workgroup of every line that runs in the default configuration are also looked
up in profiles/dw_route_parent_{fine,coarse,bf16,fp16}.csv, the tables of kernel traces of the commit BEFORE the router existed (bench.py
--steps 2 --warmup 1 [--stream coarse --eager | --dtype bf16 | --dtype fp16] under a kernel trace): those are the old chains' choices,
not the router's.  The wave kernels' LDS images are static, which the router does not know, and the traces do not record the band
kernels' dynamic LDS, so the lds= figures are pinned from the plans' own arithmetic (unchanged formulas) and guard against later drift,
no more."""
import csv
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'coarse-fine-networks_amd')
for p in (ROOT, PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

NONE, RELU, SWISH = 0, 1, 2
PRO, STATS, Y, MISALIGNED = 1, 2, 4, 16
FWD, DGRAD, WGRAD, FUSED = 0, 1, 2, 3
F32, BF16, F16 = 0, 1, 2
# the router's full family list (csrc/dw_plan.h)
FAMILIES = {'flat', 'flat_s2', 'flat14to7', 'cp', 'small', 'band', 'dgrad_s2', 'flatb', 'cpbx', 'bandf', 'flatb_s2', 'cpb2x'}


@pytest.fixture(scope='module')
def route():
    import cfn_hip
    if not os.path.exists(cfn_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    from cfn_hip import ops
    return ops.dwconv3d_route


def family(line):
    return line.split()[0]


def kernel(line):
    """'dw3d_cpx_bwd_kernel<14, 2, 7, 2, 3, true>' out of a route line"""
    return line.split(' ', 1)[1].split(' grid=')[0]


def model_calls(N=8, T=256, size=224, T_deep=None):
    """(name, op, (N, C, T, H, W, stride, act, flags)) of conv2 of every block of one X3D-M training step, from the model's own width and
    depth tables.  The stem halves the plane; the first block of a stage has the stride.  conv2 reads conv1's output with bn1 + ReLU as
    its prologue and returns statistics, so gsum, gsumsq and y arrive in the backward.  T_deep: the frame count behind the coarse stream's
    Grid Pool (layers 2-4).  Per conv: the forward (op 0), the one-pass backward (op 3), and the data (op 1) and weight gradient (op 2)
    ops._DwConv3d.backward falls back to when that one declines."""
    import x3d_fine
    planes, blocks = x3d_fine.get_inplanes('M'), x3d_fine.get_blocks('M')
    calls, res = [], size // 2
    for li, ((mid, _), nb) in enumerate(zip(planes, blocks), 1):
        if li == 2 and T_deep:
            T = T_deep
        for b in range(nb):
            stride, r = (2, res) if b == 0 else (1, res // 2)
            nm = 'layer%d.%d.conv2' % (li, b)
            calls.append((nm, FWD, (N, mid, T, r, r, stride, RELU, PRO | STATS)))
            for op in (FUSED, DGRAD, WGRAD):
                calls.append((nm, op, (N, mid, T, r, r, stride, RELU, PRO | STATS | Y)))
        res //= 2
    return calls


def reached(calls, lines):
    """the calls that run in the default configuration: a data / weight gradient only where the one-pass entry point declined"""
    out, declined = [], {}
    for (nm, op, args), line in zip(calls, lines):
        if op == FUSED:
            declined[nm] = line == 'declined'
        if op == FWD or (op == FUSED and not declined[nm]) or (op in (DGRAD, WGRAD) and declined[nm]):
            out.append(line)
    return out


# distinct (op, N, C, T, H, W, stride, act, flags) -> route line of the fine stream, 8 clips x 256 frames x 224 x 224, fp32
FINE_ROUTES = {
    (0, 8, 54, 256, 112, 112, 2, 1, 3):
        'flat_s2 dw3d_flat_s2_fwd_kernel<56, 4, 8> grid=193536 wg=256 lds=0',   # layer1.0.conv2
    (3, 8, 54, 256, 112, 112, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<56, 2, 3, true> grid=33264 wg=256 lds=0',   # layer1.0.conv2
    (1, 8, 54, 256, 112, 112, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=52x432x1 wg=256 lds=0',   # layer1.0.conv2
    (2, 8, 54, 256, 112, 112, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, true> grid=6048 wg=256 lds=9080',   # layer1.0.conv2
    (0, 8, 54, 256, 56, 56, 1, 1, 3):
        'flat dw3d_flat_fwd_kernel<56, 14, 8> grid=55296 wg=256 lds=0',   # layer1.1.conv2
    (3, 8, 54, 256, 56, 56, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<56, 2, 2, 1, 3, true> grid=6048 wg=256 lds=0',   # layer1.1.conv2
    (1, 8, 54, 256, 56, 56, 1, 1, 7):
        'band dw3d_kernel<1, 1, 7, 4, 2, true> grid=6048 wg=256 lds=15400',   # layer1.1.conv2
    (2, 8, 54, 256, 56, 56, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 4, 2, true> grid=6048 wg=256 lds=15800',   # layer1.1.conv2
    (0, 8, 108, 256, 56, 56, 2, 1, 3):
        'flat_s2 dw3d_flat_s2_fwd_kernel<28, 7, 8> grid=110592 wg=256 lds=0',   # layer2.0.conv2
    (3, 8, 108, 256, 56, 56, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<28, 4, 3, true> grid=16632 wg=256 lds=0',   # layer2.0.conv2
    (1, 8, 108, 256, 56, 56, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=16x864x1 wg=256 lds=0',   # layer2.0.conv2
    (2, 8, 108, 256, 56, 56, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, false> grid=3456 wg=256 lds=8120',   # layer2.0.conv2
    (0, 8, 108, 256, 28, 28, 1, 1, 3):
        'flat dw3d_flat_fwd_kernel<28, 28, 8> grid=27648 wg=256 lds=0',   # layer2.1.conv2
    (3, 8, 108, 256, 28, 28, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<28, 1, 4, 1, 4, true> grid=6048 wg=256 lds=0',   # layer2.1.conv2
    (1, 8, 108, 256, 28, 28, 1, 1, 7):
        'band dw3d_kernel<1, 1, 7, 4, 2, true> grid=3024 wg=256 lds=17360',   # layer2.1.conv2
    (2, 8, 108, 256, 28, 28, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 4, 2, true> grid=3024 wg=256 lds=18160',   # layer2.1.conv2
    (0, 8, 216, 256, 28, 28, 2, 1, 3):
        'flat_s2 dw3d_flat_s2_fwd_kernel<14, 14, 8> grid=55296 wg=256 lds=0',   # layer3.0.conv2
    (3, 8, 216, 256, 28, 28, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<14, 7, 3, true> grid=9504 wg=256 lds=0',   # layer3.0.conv2
    (1, 8, 216, 256, 28, 28, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=4x1728x1 wg=256 lds=0',   # layer3.0.conv2
    (2, 8, 216, 256, 28, 28, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, false> grid=3456 wg=256 lds=8792',   # layer3.0.conv2
    (0, 8, 216, 256, 14, 14, 1, 1, 3):
        'flat dw3d_flat14_fwd_kernel<8> grid=13824 wg=256 lds=0',   # layer3.1.conv2
    (3, 8, 216, 256, 14, 14, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<14, 2, 7, 2, 3, true> grid=1728 wg=256 lds=0',   # layer3.1.conv2
    (1, 8, 216, 256, 14, 14, 1, 1, 7):
        'band dw3d_kernel<1, 1, 2, 2, 2, false> grid=6048 wg=256 lds=4688',   # layer3.1.conv2
    (2, 8, 216, 256, 14, 14, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 2, 2, false> grid=1536 wg=256 lds=24696',   # layer3.1.conv2
    (0, 8, 432, 256, 14, 14, 2, 1, 3):
        'flat14to7 dw3d_flat14to7_fwd_kernel<8> grid=27648 wg=256 lds=0',   # layer4.0.conv2
    (3, 8, 432, 256, 14, 14, 2, 1, 7):
        'flatb_s2 dw3d_flat14to7_bwd_kernel<8, true> grid=3456 wg=256 lds=0',   # layer4.0.conv2
    (1, 8, 432, 256, 14, 14, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<true> grid=4x692x1 wg=256 lds=0',   # layer4.0.conv2
    (2, 8, 432, 256, 14, 14, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 2, 2, false> grid=3480 wg=256 lds=13000',   # layer4.0.conv2
    (0, 8, 432, 256, 7, 7, 1, 1, 3):
        'small dw3d_small_fwd_kernel<7, 1> grid=3456 wg=256 lds=0',   # layer4.1.conv2
    (3, 8, 432, 256, 7, 7, 1, 1, 7):
        'flatb dw3d_flat7_bwd_kernel<8, true> grid=3456 wg=256 lds=0',   # layer4.1.conv2
    (1, 8, 432, 256, 7, 7, 1, 1, 7):
        'band dw3d_kernel<1, 1, 1, 1, 4, false> grid=4872 wg=256 lds=3440',   # layer4.1.conv2
    (2, 8, 432, 256, 7, 7, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 1, 8, false> grid=1008 wg=256 lds=34816',   # layer4.1.conv2
}

# the coarse stream: 64 frames in layer 1, 17 behind the Grid Pool
COARSE_ROUTES = {
    (0, 8, 54, 64, 112, 112, 2, 1, 3):
        'flat_s2 dw3d_flat_s2_fwd_kernel<56, 4, 8> grid=48384 wg=256 lds=0',   # layer1.0.conv2
    (3, 8, 54, 64, 112, 112, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<56, 2, 3, true> grid=9072 wg=256 lds=0',   # layer1.0.conv2
    (1, 8, 54, 64, 112, 112, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=13x432x1 wg=256 lds=0',   # layer1.0.conv2
    (2, 8, 54, 64, 112, 112, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, true> grid=6048 wg=256 lds=9080',   # layer1.0.conv2
    (0, 8, 54, 64, 56, 56, 1, 1, 3):
        'flat dw3d_flat_fwd_kernel<56, 14, 8> grid=13824 wg=256 lds=0',   # layer1.1.conv2
    (3, 8, 54, 64, 56, 56, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<56, 2, 2, 1, 3, true> grid=3024 wg=256 lds=0',   # layer1.1.conv2
    (1, 8, 54, 64, 56, 56, 1, 1, 7):
        'band dw3d_kernel<1, 1, 7, 4, 2, true> grid=1728 wg=256 lds=15400',   # layer1.1.conv2
    (2, 8, 54, 64, 56, 56, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 4, 2, true> grid=1728 wg=256 lds=15800',   # layer1.1.conv2
    (0, 8, 108, 17, 56, 56, 2, 1, 3):
        'flat_s2 dw3d_flat_s2_fwd_kernel<28, 7, 8> grid=10368 wg=256 lds=0',   # layer2.0.conv2
    (3, 8, 108, 17, 56, 56, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<28, 4, 3, true> grid=1512 wg=256 lds=0',   # layer2.0.conv2
    (1, 8, 108, 17, 56, 56, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=4x864x1 wg=256 lds=0',   # layer2.0.conv2
    (2, 8, 108, 17, 56, 56, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, false> grid=3456 wg=256 lds=8120',   # layer2.0.conv2
    (0, 8, 108, 17, 28, 28, 1, 1, 3):
        'flat dw3d_flat_fwd_kernel<28, 28, 8> grid=2592 wg=256 lds=0',   # layer2.1.conv2
    (3, 8, 108, 17, 28, 28, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<28, 1, 4, 1, 4, true> grid=1512 wg=256 lds=0',   # layer2.1.conv2
    (1, 8, 108, 17, 28, 28, 1, 1, 7):
        'band dw3d_kernel<1, 1, 7, 4, 2, true> grid=432 wg=256 lds=17360',   # layer2.1.conv2
    (2, 8, 108, 17, 28, 28, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 4, 2, true> grid=432 wg=256 lds=18160',   # layer2.1.conv2
    (0, 8, 216, 17, 28, 28, 2, 1, 3):
        'flat_s2 dw3d_flat_s2_fwd_kernel<14, 14, 8> grid=5184 wg=256 lds=0',   # layer3.0.conv2
    (3, 8, 216, 17, 28, 28, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<14, 7, 3, true> grid=864 wg=256 lds=0',   # layer3.0.conv2
    (1, 8, 216, 17, 28, 28, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=2x1728x1 wg=256 lds=0',   # layer3.0.conv2
    (2, 8, 216, 17, 28, 28, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, false> grid=1728 wg=256 lds=8792',   # layer3.0.conv2
    (0, 8, 216, 17, 14, 14, 1, 1, 3):
        'flat dw3d_flat14_fwd_kernel<8> grid=1296 wg=256 lds=0',   # layer3.1.conv2
    (3, 8, 216, 17, 14, 14, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<14, 2, 7, 2, 3, true> grid=432 wg=256 lds=0',   # layer3.1.conv2
    (1, 8, 216, 17, 14, 14, 1, 1, 7):
        'band dw3d_kernel<1, 1, 2, 2, 2, false> grid=864 wg=256 lds=4688',   # layer3.1.conv2
    (2, 8, 216, 17, 14, 14, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 2, 2, false> grid=384 wg=256 lds=24696',   # layer3.1.conv2
    (0, 8, 432, 17, 14, 14, 2, 1, 3):
        'flat14to7 dw3d_flat14to7_fwd_kernel<8> grid=2592 wg=256 lds=0',   # layer4.0.conv2
    (3, 8, 432, 17, 14, 14, 2, 1, 7):
        'flatb_s2 dw3d_flat14to7_bwd_kernel<8, true> grid=864 wg=256 lds=0',   # layer4.0.conv2
    (1, 8, 432, 17, 14, 14, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<true> grid=3x692x1 wg=256 lds=0',   # layer4.0.conv2
    (2, 8, 432, 17, 14, 14, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 2, 2, false> grid=696 wg=256 lds=13000',   # layer4.0.conv2
    (0, 8, 432, 17, 7, 7, 1, 1, 3):
        'small dw3d_small_fwd_kernel<7, 1> grid=2592 wg=256 lds=0',   # layer4.1.conv2
    (3, 8, 432, 17, 7, 7, 1, 1, 7):
        'flatb dw3d_flat7_bwd_kernel<8, true> grid=864 wg=256 lds=0',   # layer4.1.conv2
    (1, 8, 432, 17, 7, 7, 1, 1, 7):
        'band dw3d_kernel<1, 1, 1, 1, 4, false> grid=696 wg=256 lds=3440',   # layer4.1.conv2
    (2, 8, 432, 17, 7, 7, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 1, 8, false> grid=336 wg=256 lds=34816',   # layer4.1.conv2
}

# bf16 and fp16 tensors route alike (the gates see the element size only): the fine stream again
H16_ROUTES = {
    (0, 8, 54, 256, 112, 112, 2, 1, 3):
        'cp dw3d_cp_fwd_kernel<56, 2, 2, 2, 2, 4> grid=24192 wg=256 lds=0',   # layer1.0.conv2
    (3, 8, 54, 256, 112, 112, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<56, 2, 3, true> grid=33264 wg=256 lds=0',   # layer1.0.conv2
    (1, 8, 54, 256, 112, 112, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=52x432x1 wg=256 lds=0',   # layer1.0.conv2
    (2, 8, 54, 256, 112, 112, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, true> grid=6048 wg=256 lds=9080',   # layer1.0.conv2
    (0, 8, 54, 256, 56, 56, 1, 1, 3):
        'cp dw3d_cp_fwd_kernel<56, 1, 2, 2, 2, 4> grid=7560 wg=256 lds=0',   # layer1.1.conv2
    (3, 8, 54, 256, 56, 56, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<56, 2, 2, 1, 3, true> grid=6048 wg=256 lds=0',   # layer1.1.conv2
    (1, 8, 54, 256, 56, 56, 1, 1, 7):
        'band dw3d_kernel<1, 1, 7, 4, 2, true> grid=6048 wg=256 lds=15400',   # layer1.1.conv2
    (2, 8, 54, 256, 56, 56, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 4, 2, true> grid=6048 wg=256 lds=15800',   # layer1.1.conv2
    (0, 8, 108, 256, 56, 56, 2, 1, 3):
        'cp dw3d_cp_fwd_kernel<28, 2, 1, 4, 2, 4> grid=24192 wg=256 lds=0',   # layer2.0.conv2
    (3, 8, 108, 256, 56, 56, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<28, 4, 3, true> grid=16632 wg=256 lds=0',   # layer2.0.conv2
    (1, 8, 108, 256, 56, 56, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=16x864x1 wg=256 lds=0',   # layer2.0.conv2
    (2, 8, 108, 256, 56, 56, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, false> grid=3456 wg=256 lds=8120',   # layer2.0.conv2
    (0, 8, 108, 256, 28, 28, 1, 1, 3):
        'cp dw3d_cp_fwd_kernel<28, 1, 1, 4, 2, 4> grid=7560 wg=256 lds=0',   # layer2.1.conv2
    (3, 8, 108, 256, 28, 28, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<28, 1, 4, 1, 4, true> grid=6048 wg=256 lds=0',   # layer2.1.conv2
    (1, 8, 108, 256, 28, 28, 1, 1, 7):
        'band dw3d_kernel<1, 1, 7, 4, 2, true> grid=3024 wg=256 lds=17360',   # layer2.1.conv2
    (2, 8, 108, 256, 28, 28, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 4, 2, true> grid=3024 wg=256 lds=18160',   # layer2.1.conv2
    (0, 8, 216, 256, 28, 28, 2, 1, 3):
        'cp dw3d_cp_fwd_kernel<14, 2, 1, 7, 2, 4> grid=13824 wg=256 lds=0',   # layer3.0.conv2
    (3, 8, 216, 256, 28, 28, 2, 1, 7):
        'cpb2x dw3d_cpx_bwd_s2_kernel<14, 7, 3, true> grid=9504 wg=256 lds=0',   # layer3.0.conv2
    (1, 8, 216, 256, 28, 28, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<false> grid=4x1728x1 wg=256 lds=0',   # layer3.0.conv2
    (2, 8, 216, 256, 28, 28, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 4, 2, false> grid=3456 wg=256 lds=8792',   # layer3.0.conv2
    (0, 8, 216, 256, 14, 14, 1, 1, 3):
        'cp dw3d_cp_fwd_kernel<14, 1, 2, 7, 4, 4> grid=5184 wg=256 lds=0',   # layer3.1.conv2
    (3, 8, 216, 256, 14, 14, 1, 1, 7):
        'cpbx dw3d_cpx_bwd_kernel<14, 2, 7, 2, 3, true> grid=1728 wg=256 lds=0',   # layer3.1.conv2
    (1, 8, 216, 256, 14, 14, 1, 1, 7):
        'band dw3d_kernel<1, 1, 2, 2, 2, false> grid=6048 wg=256 lds=4688',   # layer3.1.conv2
    (2, 8, 216, 256, 14, 14, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 2, 2, false> grid=1536 wg=256 lds=24696',   # layer3.1.conv2
    (0, 8, 432, 256, 14, 14, 2, 1, 3):
        'band dw3d_kernel<0, 2, 1, 2, 2, false> grid=3480 wg=256 lds=11000',   # layer4.0.conv2
    (3, 8, 432, 256, 14, 14, 2, 1, 7):
        'flatb_s2 dw3d_flat14to7_bwd_kernel<8, true> grid=3456 wg=256 lds=0',   # layer4.0.conv2
    (1, 8, 432, 256, 14, 14, 2, 1, 7):
        'dgrad_s2 dw3d_dgrad_s2_fast_kernel<true> grid=4x692x1 wg=256 lds=0',   # layer4.0.conv2
    (2, 8, 432, 256, 14, 14, 2, 1, 7):
        'band dw3d_kernel<2, 2, 1, 2, 2, false> grid=3480 wg=256 lds=13000',   # layer4.0.conv2
    (0, 8, 432, 256, 7, 7, 1, 1, 3):
        'small dw3d_small_fwd_kernel<7, 1> grid=3456 wg=256 lds=0',   # layer4.1.conv2
    (3, 8, 432, 256, 7, 7, 1, 1, 7):
        'flatb dw3d_flat7_bwd_kernel<8, true> grid=3456 wg=256 lds=0',   # layer4.1.conv2
    (1, 8, 432, 256, 7, 7, 1, 1, 7):
        'band dw3d_kernel<1, 1, 1, 1, 4, false> grid=4872 wg=256 lds=3440',   # layer4.1.conv2
    (2, 8, 432, 256, 7, 7, 1, 1, 7):
        'band dw3d_kernel<2, 1, 7, 1, 8, false> grid=1008 wg=256 lds=34816',   # layer4.1.conv2
}

ARGS = {'flat': 'DwFlatArgs', 'flat_s2': 'DwFlatArgs', 'flat14to7': 'DwFlatArgs', 'cp': 'DwCpArgs', 'small': 'DwSmallArgs', 'flatb': 'DwFlatBArgs',
        'flatb_s2': 'DwFlatBArgs', 'cpbx': 'DwCpbxArgs', 'cpb2x': 'DwCpb2xArgs', 'band': 'DwArgs', 'bandf': 'DwFusedArgs', 'dgrad_s2': 'DwS2Args'}
BAND_FAMILIES = ('band', 'bandf', 'dgrad_s2')       # dwconv3d.hip names its argument structs DwArgsBf16 / DwArgsF16, the wave kernels DwCpArgs_bf16 / _f16


def _trace(name):
    rows = set()
    with open(os.path.join(ROOT, 'profiles', name)) as fh:
        for r in csv.DictReader(fh):
            rows.add((r['Kernel_Name'], r['Grid_Size'], r['Workgroup_Size']))
    return rows


def _as_trace_row(line, dtype):
    f = dict(kv.split('=') for kv in line.split() if '=' in kv)
    grid, wg = [int(g) for g in (f['grid'] + 'x1x1').split('x')[:3]], int(f['wg'])
    sfx = '' if dtype == F32 else (('Bf16', 'F16') if family(line) in BAND_FAMILIES else ('_bf16', '_f16'))[dtype - 1]
    return ('void %s(%s)' % (kernel(line), ARGS[family(line)] + sfx), '%dx%dx%d' % (grid[0] * wg, grid[1], grid[2]), '%dx1x1' % wg)      # a trace counts the grid in work-items


@pytest.mark.parametrize('pinned,dtype,trace,kw', [(FINE_ROUTES, F32, 'dw_route_parent_fine.csv', {}),
                                                   (COARSE_ROUTES, F32, 'dw_route_parent_coarse.csv', dict(T=64, T_deep=17)),
                                                   (H16_ROUTES, BF16, 'dw_route_parent_bf16.csv', {}),
                                                   (H16_ROUTES, F16, 'dw_route_parent_fp16.csv', {})], ids=['fine', 'coarse', 'bf16', 'fp16'])
def test_model_table_routes(route, pinned, dtype, trace, kw):
    """every conv2 of the X3D-M step (shapes derived from x3d_fine's own tables), all four ops, routes to the pinned line; of the lines that run in
    the default configuration, (kernel, grid, workgroup) is a row of the parent commit's kernel trace, and every dw3d_* row of that trace is the
    route of some call of the table"""
    calls = model_calls(**kw)
    lines = []
    for name, op, args in calls:
        key = (op,) + args
        assert key in pinned, (name, key)
        lines.append(route(op, dtype, *args))
        assert lines[-1] == pinned[key], (name, key)
    assert {(op,) + args for _, op, args in calls} == set(pinned)
    rows = _trace(trace)
    run = {_as_trace_row(line, dtype) for line in reached(calls, lines)}
    assert not run - rows, sorted(run - rows)
    mine = {r for r in rows if r[0].startswith('void dw3d_')}
    assert len(mine) == 16 and mine == run, sorted(mine ^ run)


def test_new_parent_tables_repeat_the_recorded_depthwise_rows():
    """profiles/pw_route_parent_*.csv were traced from the same three configurations before any depthwise source changed again: the 16 dw3d_*
    rows of each, dispatch counts included, are rows of the new tables"""
    for n in ('fine', 'coarse', 'bf16'):
        def rows(name):
            with open(os.path.join(ROOT, 'profiles', name)) as fh:
                return {tuple(r.values()) for r in csv.DictReader(fh) if r['Kernel_Name'].startswith('void dw3d_')}
        old, new = rows('pw_route_parent_%s.csv' % n), rows('dw_route_parent_%s.csv' % n)
        assert len(old) == 16 and old == new, (n, sorted(old ^ new))


# ---- the GPU case lists of tests/test_hip_ops.py: DW_CASES (N, C, T, H, W, stride, act, prologue) and WAVE_CASES (N, C, T, H, stride, act, prologue), asked as
# their tests call the conv: forward with statistics, backward with gsum, gsumsq and y; WAVE_CASES also without statistics (the last key element; the
# kernels' HASY = false).  Per case: "forward | one-pass backward | data gradient | weight gradient" for fp32 tensors, then for bf16 and fp16 (alike).
# A token is the family and the template arguments (band: MODE, S, HS, VEC, MAXLD, UNIW; bandf: HS, VEC, MAXLD, UNIW; dgrad_s2 / dgrad_s2_fast: PACKED).
DW_CASE_ROUTES = {
    (2, 6, 5, 7, 7, 1, 1, True):
        ('small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>',
         'small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>'),
    (1, 75, 6, 7, 7, 1, 1, True):   # 'more channels than one workgroup takes at 7x7': of the band kernel, which has the two gradients after flatb
        ('small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>',
         'small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>'),
    (1, 20, 9, 14, 14, 1, 1, True):
        ('flat<4> | cpbx<14, 2, 7, 2, 3, true> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>',
         'cp<14, 1, 2, 7, 4, 4> | cpbx<14, 2, 7, 2, 3, true> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>'),
    (1, 8, 5, 14, 14, 2, 1, True):
        ('flat14to7<4> | flatb_s2<4, true> | dgrad_s2_fast<true> | band<2, 2, 1, 2, 2, false>',
         'band<0, 2, 1, 2, 2, false> | flatb_s2<4, true> | dgrad_s2_fast<true> | band<2, 2, 1, 2, 2, false>'),
    (2, 5, 6, 28, 28, 1, 1, True):
        ('flat<28, 28, 4> | cpbx<28, 1, 4, 1, 4, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<28, 1, 1, 4, 2, 4> | cpbx<28, 1, 4, 1, 4, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 4, 4, 28, 28, 2, 0, False):
        ('flat_s2<14, 14, 4> | cpb2x<14, 7, 3, true> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>',
         'cp<14, 2, 1, 7, 2, 4> | cpb2x<14, 7, 3, true> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 3, 37, 56, 56, 1, 1, True):   # 'several t-chunks': flat items of 8 frames
        ('flat<56, 14, 8> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 2, 3, 112, 112, 2, 1, True):
        ('flat_s2<56, 4, 4> | cpb2x<56, 2, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, true>',
         'cp<56, 2, 2, 2, 2, 4> | cpb2x<56, 2, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, true>'),
    (2, 5, 7, 56, 56, 2, 1, True):   # 'fused stride-2 backward, several bands': cpb2x
        ('flat_s2<28, 7, 4> | cpb2x<28, 4, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>',
         'cp<28, 2, 1, 4, 2, 4> | cpb2x<28, 4, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 3, 20, 28, 28, 2, 1, True):
        ('flat_s2<14, 14, 8> | cpb2x<14, 7, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>',
         'cp<14, 2, 1, 7, 2, 4> | cpb2x<14, 7, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 3, 4, 40, 40, 1, 1, True):   # 'HS=4 path': the band kernel's third template argument; 4 x 40 thread slots are not wave uniform: no one-pass backward
        ('band<0, 1, 4, 4, 2, false> | declined | band<1, 1, 4, 4, 2, false> | band<2, 1, 4, 4, 2, false>',
         'band<0, 1, 4, 4, 2, false> | declined | band<1, 1, 4, 4, 2, false> | band<2, 1, 4, 4, 2, false>'),
    (1, 2, 3, 80, 80, 2, 1, True):
        ('band<0, 2, 1, 4, 2, false> | declined | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>',
         'band<0, 2, 1, 4, 2, false> | declined | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 3, 3, 10, 10, 1, 2, True):   # 'HS=2 path'
        ('band<0, 1, 2, 2, 2, false> | declined | band<1, 1, 2, 2, 2, false> | band<2, 1, 2, 2, 2, false>',
         'band<0, 1, 2, 2, 2, false> | declined | band<1, 1, 2, 2, 2, false> | band<2, 1, 2, 2, 2, false>'),
    (2, 3, 2, 5, 5, 2, 1, True):   # 'HS=1 path'; odd width: the plain stride-2 data gradient, packed
        ('band<0, 2, 1, 1, 4, false> | declined | dgrad_s2<true> | band<2, 2, 1, 1, 4, false>',
         'band<0, 2, 1, 1, 4, false> | declined | dgrad_s2<true> | band<2, 2, 1, 1, 4, false>'),
    (1, 2, 1, 7, 7, 1, 1, True):
        ('small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (1, 3, 4, 16, 16, 1, 1, True):   # the one-pass band kernel, 4-row strips
        ('band<0, 1, 4, 4, 2, true> | bandf<4, 4, 2, true> | band<1, 1, 4, 4, 2, true> | band<2, 1, 4, 4, 2, true>',
         'band<0, 1, 4, 4, 2, true> | bandf<4, 4, 2, true> | band<1, 1, 4, 4, 2, true> | band<2, 1, 4, 4, 2, true>'),
    (1, 3, 4, 28, 28, 1, 2, True):   # the one-pass band kernel, 7-row strips; the Swish prologue leaves flat / cp / cpbx for the band kernels
        ('band<0, 1, 7, 4, 2, true> | bandf<7, 4, 2, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'band<0, 1, 7, 4, 2, true> | bandf<7, 4, 2, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
}

WAVE_CASE_ROUTES = {
    (2, 3, 1, 56, 1, 1, True, True):
        ('flat<56, 14, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (2, 3, 1, 56, 1, 1, True, False):
        ('flat<56, 14, 4> | cpbx<56, 2, 2, 1, 3, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 2, 2, 56, 1, 0, False, True):
        ('flat<56, 14, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 2, 2, 56, 1, 0, False, False):
        ('flat<56, 14, 4> | cpbx<56, 2, 2, 1, 3, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 3, 61, 28, 1, 1, True, True):
        ('flat<28, 28, 8> | cpbx<28, 1, 4, 1, 4, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<28, 1, 1, 4, 2, 4> | cpbx<28, 1, 4, 1, 4, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 3, 61, 28, 1, 1, True, False):
        ('flat<28, 28, 8> | cpbx<28, 1, 4, 1, 4, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<28, 1, 1, 4, 2, 4> | cpbx<28, 1, 4, 1, 4, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (2, 2, 7, 14, 1, 0, True, True):
        ('flat<4> | cpbx<14, 2, 7, 2, 3, true> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>',
         'cp<14, 1, 2, 7, 4, 4> | cpbx<14, 2, 7, 2, 3, true> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>'),
    (2, 2, 7, 14, 1, 0, True, False):
        ('flat<4> | cpbx<14, 2, 7, 2, 3, false> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>',
         'cp<14, 1, 2, 7, 4, 4> | cpbx<14, 2, 7, 2, 3, false> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>'),
    (1, 5, 4, 7, 1, 1, True, True):
        ('small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>',
         'small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>'),
    (1, 5, 4, 7, 1, 1, True, False):
        ('small<7, 1> | flatb<4, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>',
         'small<7, 1> | flatb<4, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 8, false>'),
    (1, 3, 3, 7, 1, 0, False, True):
        ('small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<4, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (1, 3, 3, 7, 1, 0, False, False):
        ('small<7, 1> | flatb<4, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<4, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (1, 2, 1, 112, 2, 1, True, True):
        ('flat_s2<56, 4, 4> | cpb2x<56, 2, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, true>',
         'cp<56, 2, 2, 2, 2, 4> | cpb2x<56, 2, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, true>'),
    (1, 2, 1, 112, 2, 1, True, False):
        ('flat_s2<56, 4, 4> | cpb2x<56, 2, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, true>',
         'cp<56, 2, 2, 2, 2, 4> | cpb2x<56, 2, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, true>'),
    (2, 3, 5, 56, 2, 0, False, True):
        ('flat_s2<28, 7, 4> | cpb2x<28, 4, 3, true> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>',
         'cp<28, 2, 1, 4, 2, 4> | cpb2x<28, 4, 3, true> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>'),
    (2, 3, 5, 56, 2, 0, False, False):
        ('flat_s2<28, 7, 4> | cpb2x<28, 4, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>',
         'cp<28, 2, 1, 4, 2, 4> | cpb2x<28, 4, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 4, 58, 28, 2, 1, True, True):
        ('flat_s2<14, 14, 8> | cpb2x<14, 7, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>',
         'cp<14, 2, 1, 7, 2, 4> | cpb2x<14, 7, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 4, 58, 28, 2, 1, True, False):
        ('flat_s2<14, 14, 8> | cpb2x<14, 7, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>',
         'cp<14, 2, 1, 7, 2, 4> | cpb2x<14, 7, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 2, 13, 14, 1, 1, True, True):
        ('flat<8> | cpbx<14, 2, 7, 2, 3, true> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>',
         'cp<14, 1, 2, 7, 4, 4> | cpbx<14, 2, 7, 2, 3, true> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>'),
    (1, 2, 13, 14, 1, 1, True, False):
        ('flat<8> | cpbx<14, 2, 7, 2, 3, false> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>',
         'cp<14, 1, 2, 7, 4, 4> | cpbx<14, 2, 7, 2, 3, false> | band<1, 1, 2, 2, 2, false> | band<2, 1, 7, 2, 2, false>'),
    (2, 2, 8, 56, 1, 1, True, True):
        ('flat<56, 14, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (2, 2, 8, 56, 1, 1, True, False):
        ('flat<56, 14, 4> | cpbx<56, 2, 2, 1, 3, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<56, 1, 2, 2, 2, 4> | cpbx<56, 2, 2, 1, 3, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 2, 11, 28, 1, 0, True, True):
        ('flat<28, 28, 4> | cpbx<28, 1, 4, 1, 4, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<28, 1, 1, 4, 2, 4> | cpbx<28, 1, 4, 1, 4, true> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 2, 11, 28, 1, 0, True, False):
        ('flat<28, 28, 4> | cpbx<28, 1, 4, 1, 4, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>',
         'cp<28, 1, 1, 4, 2, 4> | cpbx<28, 1, 4, 1, 4, false> | band<1, 1, 7, 4, 2, true> | band<2, 1, 7, 4, 2, true>'),
    (1, 2, 12, 112, 2, 1, True, True):
        ('flat_s2<56, 4, 8> | cpb2x<56, 2, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, true>',
         'cp<56, 2, 2, 2, 2, 4> | cpb2x<56, 2, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, true>'),
    (1, 2, 12, 112, 2, 1, True, False):
        ('flat_s2<56, 4, 8> | cpb2x<56, 2, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, true>',
         'cp<56, 2, 2, 2, 2, 4> | cpb2x<56, 2, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, true>'),
    (2, 2, 19, 28, 2, 1, True, True):
        ('flat_s2<14, 14, 8> | cpb2x<14, 7, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>',
         'cp<14, 2, 1, 7, 2, 4> | cpb2x<14, 7, 3, true> | dgrad_s2_fast<false> | band<2, 2, 1, 4, 2, false>'),
    (2, 2, 19, 28, 2, 1, True, False):
        ('flat_s2<14, 14, 8> | cpb2x<14, 7, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>',
         'cp<14, 2, 1, 7, 2, 4> | cpb2x<14, 7, 3, false> | dgrad_s2<false> | band<2, 2, 1, 4, 2, false>'),
    (1, 4, 21, 7, 1, 1, True, True):
        ('small<7, 1> | flatb<8, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<8, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (1, 4, 21, 7, 1, 1, True, False):
        ('small<7, 1> | flatb<8, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<8, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (2, 3, 16, 7, 1, 0, True, True):
        ('small<7, 1> | flatb<8, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<8, true> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (2, 3, 16, 7, 1, 0, True, False):
        ('small<7, 1> | flatb<8, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>',
         'small<7, 1> | flatb<8, false> | band<1, 1, 1, 1, 4, false> | band<2, 1, 7, 1, 4, false>'),
    (1, 3, 13, 14, 2, 1, True, True):
        ('flat14to7<8> | flatb_s2<8, true> | dgrad_s2_fast<true> | band<2, 2, 1, 2, 2, false>',
         'band<0, 2, 1, 2, 2, false> | flatb_s2<8, true> | dgrad_s2_fast<true> | band<2, 2, 1, 2, 2, false>'),
    (1, 3, 13, 14, 2, 1, True, False):
        ('flat14to7<8> | flatb_s2<8, false> | dgrad_s2<true> | band<2, 2, 1, 2, 2, false>',
         'band<0, 2, 1, 2, 2, false> | flatb_s2<8, false> | dgrad_s2<true> | band<2, 2, 1, 2, 2, false>'),
}


def _token(line):
    if line == 'declined':
        return line
    k = kernel(line)
    return family(line) + ('_fast' if '_fast_' in k else '') + k[k.index('<'):]


def _four(route, dtype, N, C, T, H, W, stride, act, pro, stats):
    fwd = (PRO if pro else 0) | (STATS if stats else 0)
    back = fwd | (Y if stats else 0)
    return [route(FWD, dtype, N, C, T, H, W, stride, act, fwd)] + [route(op, dtype, N, C, T, H, W, stride, act, back) for op in (FUSED, DGRAD, WGRAD)]


def _gpu_case_lines(route):
    """{(list, case key, dtype): the four route lines} over both lists and the three element types"""
    import test_hip_ops
    out = {}
    for c in test_hip_ops.DW_CASES:
        for dtype in (F32, BF16, F16):
            out['dw', c, dtype] = _four(route, dtype, *c, True)
    for c in test_hip_ops.WAVE_CASES:
        N, C, T, H, stride, act, pro = c
        for stats in (True, False):
            for dtype in (F32, BF16, F16):
                out['wave', c + (stats,), dtype] = _four(route, dtype, N, C, T, H, H, stride, act, pro, stats)
    return out


def test_gpu_cases_route_as_pinned(route):
    import test_hip_ops
    assert set(DW_CASE_ROUTES) == set(test_hip_ops.DW_CASES) and len(test_hip_ops.DW_CASES) >= 17
    assert set(WAVE_CASE_ROUTES) == {c + (s,) for c in test_hip_ops.WAVE_CASES for s in (True, False)} and len(test_hip_ops.WAVE_CASES) >= 17
    for (lst, key, dtype), lines in _gpu_case_lines(route).items():
        want = (DW_CASE_ROUTES if lst == 'dw' else WAVE_CASE_ROUTES)[key][0 if dtype == F32 else 1]
        assert ' | '.join(_token(l) for l in lines) == want, (lst, key, dtype)


def test_gpu_cases_reach_every_family_and_branch(route):
    """conditions, not measurements: the union of the families the two lists reach is the router's full list, the one-pass band kernel at both
    strip heights included, and the stride-2 data gradient is reached with each of fast / plain x packed / one channel per workgroup"""
    tokens = {_token(l) for lines in _gpu_case_lines(route).values() for l in lines}
    assert {t.split('<')[0].replace('dgrad_s2_fast', 'dgrad_s2') for t in tokens} - {'declined'} == FAMILIES
    assert 'declined' in tokens
    assert {t.split(',')[0] for t in tokens if t.startswith('bandf<')} == {'bandf<4', 'bandf<7'}
    assert {t for t in tokens if t.startswith('dgrad_s2')} == {'dgrad_s2<false>', 'dgrad_s2<true>', 'dgrad_s2_fast<false>', 'dgrad_s2_fast<true>'}
    # the band kernel's strip heights, the third template argument: 7, 4, 2 and 1 rows
    assert {t.split(', ')[2] for t in tokens if t.startswith('band<')} == {'7', '4', '2', '1'}


def test_what_leaves_the_wave_kernels(route):
    """a Swish prologue, tensors aligned to their element only (where the gates look at alignment) and a non-square plane go to the band kernels;
    Swish WITHOUT a prologue is no prologue at all and stays"""
    for dtype, fwd56 in ((F32, 'flat'), (BF16, 'cp'), (F16, 'cp')):
        shapes = [((2, 4, 8, 56, 56, 1), fwd56, 'cpbx'), ((2, 4, 8, 28, 28, 1), fwd56, 'cpbx'), ((2, 4, 8, 14, 14, 1), fwd56, 'cpbx'),
                  ((2, 4, 8, 112, 112, 2), 'flat_s2' if dtype == F32 else 'cp', 'cpb2x'), ((2, 4, 8, 7, 7, 1), 'small', 'flatb'),
                  ((2, 4, 8, 14, 14, 2), 'flat14to7' if dtype == F32 else 'band', 'flatb_s2')]
        for dims, fwd, one in shapes:
            assert family(route(FWD, dtype, *dims, RELU, PRO | STATS)) == fwd, (dtype, dims)
            assert family(route(FUSED, dtype, *dims, RELU, PRO | STATS | Y)) == one, (dtype, dims)
            assert family(route(FWD, dtype, *dims, SWISH, STATS)) == fwd, (dtype, dims)
            # Swish prologue: every wave kernel declines
            assert family(route(FWD, dtype, *dims, SWISH, PRO | STATS)) == 'band', (dtype, dims)
            assert family(route(FUSED, dtype, *dims, SWISH, PRO | STATS | Y)) in ('bandf', 'declined'), (dtype, dims)
            # element alignment only: flat / cp (16 / 8-byte loads) and the column-pair backward kernels decline; the 7x7 kernels load single
            # elements and stay; the 14 -> 7 backward wants element PAIRS
            mis_f = family(route(FWD, dtype, *dims, RELU, PRO | STATS | MISALIGNED))
            mis_b = family(route(FUSED, dtype, *dims, RELU, PRO | STATS | Y | MISALIGNED))
            assert mis_f == ('small' if fwd == 'small' else 'band'), (dtype, dims, mis_f)
            assert mis_b == ('flatb' if one == 'flatb' else ('bandf' if dims[3] in (56, 28) and dims[5] == 1 else 'declined')), (dtype, dims, mis_b)
    for dtype in (F32, BF16, F16):
        # non-square planes: the band kernels; no one-pass backward at these sizes
        assert family(route(FWD, dtype, 1, 4, 8, 56, 28, 1, RELU, PRO | STATS)) == 'band'
        assert family(route(FWD, dtype, 1, 4, 8, 7, 14, 1, RELU, PRO | STATS)) == 'band'
        assert family(route(FUSED, dtype, 1, 4, 8, 7, 14, 1, RELU, PRO | STATS | Y)) == 'declined'
        assert family(route(FUSED, dtype, 1, 4, 8, 56, 28, 2, RELU, PRO | STATS | Y)) == 'declined'
        # a 10 x 10 plane has no one-pass backward
        assert route(FUSED, dtype, 1, 3, 3, 10, 10, 1, SWISH, PRO | STATS | Y) == 'declined'
        assert route(FUSED, dtype, 1, 3, 3, 10, 10, 2, RELU, PRO | STATS | Y) == 'declined'


def test_unsupported_shapes_return_the_entry_points_error(route):
    """an output wider than 512 columns: cfn_dwconv3d_fwd / _bwd_data / _bwd_weight fail with CFN_ERR_UNSUPPORTED, and so does the query; the one-pass
    backward declines it like any other plane it does not take; the stride-2 data gradient has no width limit"""
    import cfn_hip
    for dtype in (F32, BF16, F16):
        for op, stride in ((FWD, 1), (FWD, 2), (DGRAD, 1), (WGRAD, 1), (WGRAD, 2)):
            W = 516 * stride
            with pytest.raises(RuntimeError, match='output width %d > 512' % 516):
                route(op, dtype, 1, 2, 2, 8, W, stride, RELU, PRO | STATS | (Y if op else 0))
            out = ctypes.create_string_buffer(256)
            assert cfn_hip.query('cfn_dwconv3d_route', op, dtype, 1, 2, 2, 8, W, stride, RELU, PRO | STATS, out, 256) == 3      # CFN_ERR_UNSUPPORTED
        assert route(FUSED, dtype, 1, 2, 2, 8, 516, 1, RELU, PRO | STATS | Y) == 'declined'
        assert family(route(DGRAD, dtype, 1, 2, 2, 8, 1032, 2, RELU, PRO | STATS | Y)) == 'dgrad_s2'
        assert family(route(FWD, dtype, 1, 2, 2, 8, 512, 1, RELU, PRO | STATS)) == 'band'
    with pytest.raises(RuntimeError):
        route(4, F32, 1, 2, 2, 8, 8, 1, RELU, 0)
    with pytest.raises(RuntimeError):
        route(FWD, 3, 1, 2, 2, 8, 8, 1, RELU, 0)
