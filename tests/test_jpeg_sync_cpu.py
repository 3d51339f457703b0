"""CPU: the 'sync' entropy mode of the JPEG decoder (parallel inside a frame without restart markers), as cfn_hip.jpegdec states it in plain
Python (decode_coefficients_sync), and the boundary the GPU path adds: header prototypes, operator tuple, fake kernel, argument checks.

Bounds.  Everything is integer arithmetic on the bit stream: every comparison is equality.  Rounds are counted as decode_coefficients_sync
counts them: rounds in which at least one subsequence was decoded, round 0 included.  The last of them is the round that re-decodes the
subsequences whose entry moved in the round before and finds no exit changed; a count of the rounds needed to REACH the true states is
therefore one lower (4 / 3 / 3 for the bench frames at 128 bytes, 3 for 48x64_smooth_444q90 at 16), except where the cap of n rounds
ends the loop (48x64_noise_420q100 at 16: 380 of 380) or there is one subsequence only."""
import functools
import os

import numpy as np
import pytest
import torch

import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (16, 32, 64)


@functools.lru_cache(maxsize=None)
def plain_names():
    """the fixtures without restart markers"""
    from cfn_hip import jpegdec
    return tuple(n for n in jc.names() if jpegdec.parse(jc.jpg(n)).restart_interval == 0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """decode_coefficients of a fixture, computed once and shared"""
    from cfn_hip import jpegdec
    planes = jpegdec.decode_coefficients(jc.jpg(name))
    for p in planes:
        p.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def stuffed_boundary():
    """(fixture, sub_bytes, boundaries): the first fixture and size for which some j * sub_bytes falls on the 00 of an FF 00 pair"""
    from cfn_hip import jpegdec
    for name in plain_names():
        a = np.frombuffer(jc.jpg(name), dtype=np.uint8)
        info = jpegdec.parse(a)
        seg = a[info.scan_start:info.scan_end]
        for S in SIZES:
            hits = [j for j in range(1, -(-seg.size // S)) if seg[j * S - 1] == 0xFF and seg[j * S] == 0]
            if hits:
                return name, S, len(hits)
    return None


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def test_fixture_inventory():
    assert len(plain_names()) == 63 and jc.coverage()['stuffed'] > 0


@pytest.mark.parametrize('sub_bytes', SIZES)
def test_sync_equals_sequential_on_every_fixture(sub_bytes):
    from cfn_hip import jpegdec
    bad = []
    for name in plain_names():
        stats = {}
        got = jpegdec.decode_coefficients_sync(jc.jpg(name), sub_bytes, stats=stats)
        info = jpegdec.parse(jc.jpg(name))
        hs, vs, _, _, nblocks = jpegdec.block_grid(info.height, info.width, len(info.components), jpegdec.sampling_code(info))
        bpm = hs * vs + len(info.components) - 1
        n = stats['subsequences']
        ok = _same(got, reference(name)) and 1 <= stats['rounds'] <= n and n == max(1, -(-(info.scan_end - info.scan_start) // sub_bytes))
        ok = ok and len(stats['entries']) == len(stats['first_blocks']) == len(stats['predictors']) == n and stats['entries'][0] == (0, 0, 0, 0)
        for e, first in zip(stats['entries'], stats['first_blocks']):
            # (an entry behind the frame's last block is whatever the padding bits decode to: it takes no part)
            ok = ok and (first >= nblocks or (e is not None and e[2] == first % bpm and 0 <= e[3] < 64 and 0 <= e[1] < 8))
        if not ok:
            bad.append((name, stats['rounds'], n))
    assert not bad, bad


def test_rounds_at_both_ends():
    """the cap of n rounds, quick synchronisation, and a frame of one subsequence"""
    from cfn_hip import jpegdec
    seen = {}
    for name in ('48x64_noise_420q100', '48x64_smooth_444q90', '16x16_smooth_420q10'):
        stats = {}
        assert _same(jpegdec.decode_coefficients_sync(jc.jpg(name), 16, stats=stats), reference(name))
        seen[name] = (stats['rounds'], stats['subsequences'])
    print('rounds / subsequences at 16 bytes:', seen)
    assert seen == {'48x64_noise_420q100': (380, 380), '48x64_smooth_444q90': (4, 47), '16x16_smooth_420q10': (1, 1)}
    info = jpegdec.parse(jc.jpg('16x16_smooth_420q10'))
    assert info.scan_end - info.scan_start == 12               # shorter than a subsequence: the kernels leave it to the lane-per-interval path
    # fewer rounds than needed: the statement does not hide it
    try:
        short = jpegdec.decode_coefficients_sync(jc.jpg('48x64_noise_420q100'), 16, max_rounds=3)
    except ValueError:
        short = None
    assert short is None or not _same(short, reference('48x64_noise_420q100'))


def test_bench_frames_at_128():
    from cfn_hip import jpegdec
    z = np.load(os.path.join(jc.GOLDEN, 'jpeg_bench.npz'), allow_pickle=False)
    rounds = []
    for key in ('180x320.jpg', '240x320.jpg', '360x480.jpg'):
        buf = z[key].tobytes()
        stats = {}
        assert _same(jpegdec.decode_coefficients_sync(buf, 128, stats=stats), jpegdec.decode_coefficients(buf))
        rounds.append((stats['rounds'], stats['subsequences']))
    print('bench frames, 128 bytes: rounds / subsequences', rounds)
    # one more than the 4 / 3 / 3 rounds after which every exit is the true one: the confirming round is counted (see the module docstring)
    assert rounds == [(5, 49), (4, 56), (4, 122)]


def test_boundary_on_a_stuffed_zero():
    from cfn_hip import jpegdec
    found = stuffed_boundary()
    assert found is not None, 'no fixture with a subsequence boundary on a stuffed 00'
    name, S, hits = found
    stats = {}
    assert _same(jpegdec.decode_coefficients_sync(jc.jpg(name), S, stats=stats), reference(name))
    assert stats['stuffed_starts'] == hits >= 1


def test_invalid_predecessor_does_not_travel():
    """optimised tables leave codes unused: speculative decodes end in them, and the successor then starts from its own speculative start
    instead of passing the invalid state down the frame"""
    from cfn_hip import jpegdec
    stats = {}
    name = '48x64_smooth_420q50opt'
    assert _same(jpegdec.decode_coefficients_sync(jc.jpg(name), 16, stats=stats), reference(name))
    assert stats['invalid_exits'] >= 1 and stats['rounds'] < stats['subsequences'], stats
    with pytest.raises(ValueError, match='restart'):
        jpegdec.decode_coefficients_sync(jc.jpg('48x64_smooth_420q75rst3'), 16)


def test_header_and_operator_tuples():
    import cfn_hip
    from cfn_hip import torchlib
    protos = cfn_hip.header_prototypes()
    ret, at, dt = protos['cfn_jpeg_decode_u8_sync']
    assert len(at) == 21 and dt[0] == torch.uint8 and dt[1] == torch.int32 and dt[5] == torch.uint8 and dt[6] == torch.int32
    assert len(protos['cfn_jpeg_decode_u8'][1]) == 19 and len(protos['cfn_jpeg_workspace_bytes'][1]) == 4
    assert protos['cfn_jpeg_decode_u8_sync'][1][:18] == protos['cfn_jpeg_decode_u8'][1][:18]
    with open(os.path.join(ROOT, 'include', 'cfn_hip.h')) as fh:
        txt = fh.read()
    assert txt.count('pil_loader') >= 2
    assert torchlib.DECODE_OPERATORS == ('jpeg_decode_u8',) and torchlib.DECODE_SYNC_OPERATORS == ('jpeg_decode_sync_u8',)
    for tup in (torchlib.OPERATORS, torchlib.INPUT_OPERATORS, torchlib.AUGMENT_OPERATORS, torchlib.METRIC_OPERATORS, torchlib.FEATURE_OPERATORS,
                torchlib.DECODE_OPERATORS, torchlib.LABEL_OPERATORS):
        assert not set(torchlib.DECODE_SYNC_OPERATORS) & set(tup)
    assert hasattr(torch.ops.cfn, 'jpeg_decode_sync_u8')


def test_fake_kernel_shapes():
    from cfn_hip import torchlib  # noqa: F401
    m = dict(device='meta')
    frames, status = torch.ops.cfn.jpeg_decode_sync_u8(torch.empty(1000, dtype=torch.uint8, **m), torch.empty(7, 8, dtype=torch.int32, **m),
                                                       torch.empty(2, 3456, dtype=torch.int32, **m), torch.empty(4, 4, dtype=torch.int32, **m),
                                                       torch.empty(4, dtype=torch.int32, **m), [3, 48, 64, 9, 36], 128, 512)
    assert tuple(frames.shape) == (4, 3, 48, 64, 3) and frames.dtype == torch.uint8 and frames.device.type == 'meta'
    assert tuple(status.shape) == (7,) and status.dtype == torch.int32


def test_bad_arguments_name_the_argument(monkeypatch):
    import cfn_hip
    from cfn_hip import jpegdec, ops
    clips = jpegdec.collate_jpeg(jc.jpeg_samples(jc.MIXED, jc.MIXED_BOX))
    for kw, word in ((dict(entropy='bogus'), 'entropy'), (dict(entropy='sync', sub_bytes=18), 'sub_bytes'),
                     (dict(entropy='sync', sub_bytes=12), 'sub_bytes'), (dict(entropy='sync', sub_bytes=2048), 'sub_bytes'),
                     (dict(entropy='sync', max_subs=0), 'max_subs'), (dict(entropy='sync', max_subs=jpegdec.SYNC_MAX_SUBS + 1), 'max_subs'),
                     (dict(sub_bytes=64), 'sub_bytes'), (dict(entropy='interval', max_subs=8), 'max_subs')):
        with pytest.raises(ValueError, match=word):
            ops.jpeg_decode_u8(clips, **kw)
    with pytest.raises(ValueError, match='sub_bytes'):
        ops.jpeg_workspace_bytes(6, 12, 9, 36, entropy='sync', sub_bytes=30)
    with pytest.raises(ValueError, match='entropy'):
        clips.decode(entropy='fast')
    with pytest.raises(ValueError, match='entropy'):
        jpegdec.decode_checked(clips, 'cpu', entropy='fast')
    with pytest.raises(ValueError, match='sub_bytes'):
        clips.decode(entropy='interval', sub_bytes=64)
    # the default comes from the environment, at call time
    monkeypatch.delenv('CFN_JPEG_ENTROPY', raising=False)
    assert jpegdec.entropy_mode() == 'interval'
    monkeypatch.setenv('CFN_JPEG_ENTROPY', 'sync')
    assert jpegdec.entropy_mode() == 'sync' and jpegdec.entropy_mode('interval') == 'interval'
    monkeypatch.setenv('CFN_JPEG_ENTROPY', 'quick')
    with pytest.raises(ValueError, match='entropy'):
        clips.decode()
    monkeypatch.delenv('CFN_JPEG_ENTROPY')
    for mode in ('interval', 'sync'):
        with pytest.raises(RuntimeError):
            clips.decode(entropy=mode)                          # host tensors: there is no CPU path in either mode
    # the C boundary
    lib = cfn_hip.load()
    null = [None] * 8
    assert lib.cfn_jpeg_decode_u8_sync(*(null + [0, 16, 1, 1, 1, 1, 8, 8, 1, 1, 128, 64, None])) == 1
    assert 'null tensor' in cfn_hip.last_error() and 'cfn_jpeg_decode_u8_sync' in cfn_hip.last_error()
    assert lib.cfn_jpeg_decode_u8_sync(*(null + [0, 16, 1, 1, 1, 1, 8, 8, 1, 1, 18, 64, None])) == 1
    assert 'sub_bytes' in cfn_hip.last_error()
    assert lib.cfn_jpeg_decode_u8_sync(*(null + [0, 16, 1, 1, 1, 1, 8, 8, 1, 1, 128, 0, None])) == 1
    assert 'max_subs' in cfn_hip.last_error()


def test_scripts_take_jpeg_entropy():
    import inspect
    import extract_fineFEAT
    import train_coarse_fineFEAT
    import train_fine
    import train_joint
    for fn in (train_fine.run, train_coarse_fineFEAT.run, train_joint.run, extract_fineFEAT.extract, train_fine.flatten_clips):
        assert inspect.signature(fn).parameters['jpeg_entropy'].default is None
