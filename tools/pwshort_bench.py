#!/usr/bin/env python3
"""Backward of the strided shortcut convs of the four stage-first blocks at the benchmark's shapes (8 clips x 256 frames): the one-pass
kernel (csrc/pwshort.hip, cfn_pwconv_short_bwd) against the two separate kernels (compact data gradient + strided weight gradient), through
the C ABI.  GPU box only.  ONLY=new runs the one-pass kernel alone (for a counter pass); LAYERS=1,2 picks the stages."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'coarse-fine-networks_amd'))
import torch                      # noqa: E402
import cfn_hip                    # noqa: E402

DEV = 'cuda'
N, T = int(os.environ.get('NB', '8')), int(os.environ.get('FRAMES', '256'))
CASES = {1: ('L1.0 ds 24->24 112->56 (BN+ReLU prologue)', 24, 24, 112, 1), 2: ('L2.0 ds 24->48 56->28', 24, 48, 56, None),
         3: ('L3.0 ds 48->96 28->14', 48, 96, 28, None), 4: ('L4.0 ds 96->192 14->7', 96, 192, 14, None)}
ONLY = os.environ.get('ONLY', '')
ITERS = int(os.environ.get('ITERS', '10'))


def timeit(fn, iters=ITERS, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for layer in [int(v) for v in os.environ.get('LAYERS', '1,2,3,4').split(',')]:
    name, Cin, Cout, H, act = CASES[layer]
    Ho = H // 2
    g = torch.Generator(device=DEV).manual_seed(layer)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    gy, y, x = rn(N, Cout, T, Ho, Ho), rn(N, Cout, T, Ho, Ho), rn(N, Cin, T, H, H)
    w = 0.3 * rn(Cout, Cin)
    gs, gq, gsc = (0.05 * rn(N, Cout)).double(), (0.01 * rn(N, Cout)).double(), (1.0 + 0.3 * rn(N, Cout)).double()
    A = B = None
    if act is not None:
        A, B = (1.0 + 0.2 * rn(N, Cin)).double(), (0.2 * rn(N, Cin)).double()
    a_ = 0 if act is None else act
    da = torch.empty(N, Cin, T, Ho, Ho, device=DEV)
    gw = torch.zeros(Cout, Cin, dtype=torch.float64, device=DEV)

    def separate():
        cfn_hip.call('cfn_pwconv_bwd_data_acc', gy, y, gs, gq, w, None, None, None, 0, da, None, None, N, Cin, Cout, T, Ho, Ho, 1, None, 1, gsc)
        cfn_hip.call('cfn_pwconv_bwd_weight', gy, y, gs, gq, x, A, B, a_, gw, N, Cin, Cout, T, H, H, 2, gsc)

    def onepass():
        assert cfn_hip.call_try('cfn_pwconv_short_bwd', gy, y, gs, gq, gsc, w, x, A, B, a_, da, gw, N, Cin, Cout, T, H, H, 2)

    Q = N * T * Ho * Ho
    traffic = 4.0 * Q * (2 * Cout + 2 * Cin + Cin) / 1e9          # gy, y once; the even rows of x (2 Q per channel); da written
    tn = timeit(onepass)
    if ONLY == 'new':
        print('%-44s one pass %.3f ms   traffic %.2f GB = %.2f TB/s' % (name, tn, traffic, traffic / tn))
        continue
    ts = timeit(separate)
    print('%-44s separate %.3f ms   one pass %.3f ms   traffic %.2f GB = %.2f TB/s one pass' % (name, ts, tn, traffic, traffic / tn))
