"""The JPEG fixtures of tests/golden/jpeg_u8.npz (written by tests/golden/make_golden_jpeg.py) for the decoder's CPU and GPU tests: per case the
encoded bytes and the pixels PIL decoded from them, loaded once and shared."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@functools.lru_cache(maxsize=None)
def _npz():
    z = np.load(os.path.join(GOLDEN, 'jpeg_u8.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in _npz()['names']]


def jpg(name):
    """the file's bytes"""
    return _npz()[name + '.jpg'].tobytes()


@functools.lru_cache(maxsize=None)
def pixels(name):
    """(h, w, 3) uint8 as PIL decoded them (stored as horizontal differences modulo 256)"""
    p = np.cumsum(_npz()[name + '.rgb'], axis=1, dtype=np.uint8)
    p.setflags(write=False)
    return p


def coverage():
    return dict(zip(('zrl', 'coef63', 'stuffed', 'longest_code', 'restart'), (int(v) for v in _npz()['coverage'])))


def refused(kind):
    return _npz()['refuse_%s.jpg' % kind].tobytes()


def full_box(name):
    h, w = pixels(name).shape[:2]
    return [0, 0, min(h, w), 0]


# one batch of B = 2 videos x n = 2 clips that mixes sizes, sampling types, table sets (default, quality 95, optimised) and restart intervals;
# both clips of a video share frame count and size, as collate.fine_collate_raw_u8 needs them
MIXED = [[['33x31_smooth_420q75', '33x31_noise_420q95', '33x31_smooth_420q50opt'],
          ['33x31_smooth_444q90', '33x31_noise_444q90', '33x31_smooth_444q90']],
         [['37x50_noise_422q75'], ['37x50_smooth_420q75rst3']]]
MIXED_BOX = [[[0, 0, 31, 0], [1, 2, 20, 1]], [[3, 0, 37, 1], [0, 0, 30, 0]]]
# ragged: 3, 0, 2 and 1 frames, one size per clip, a gray clip among them
RAGGED = [[['48x64_smooth_420q75rst3', '48x64_noise_420q100', '48x64_smooth_420q10'], []],
          [['33x31_gray_q85', '33x31_gray_q85'], ['9x17_noise_422q75']]]
RAGGED_BOX = [[[0, 0, 48, 0], [0, 0, 1, 0]], [[0, 0, 31, 1], [2, 0, 9, 0]]]


def jpeg_samples(clips, boxes):
    """the clip members of the samples collate.*_collate_jpeg takes"""
    return [([[jpg(n) for n in clip] for clip in video], torch.tensor(box, dtype=torch.int32)) for video, box in zip(clips, boxes)]


def raw_samples(clips, boxes):
    """the same videos decoded by PIL: the clip members collate.*_collate_raw_u8 takes (equal frame counts and sizes inside a video)"""
    return [(torch.from_numpy(np.stack([np.stack([pixels(n) for n in clip]) for clip in video])), torch.tensor(box, dtype=torch.int32))
            for video, box in zip(clips, boxes)]


def padded(clips):
    """(B, n, Tmax, Hmax, Wmax, 3) uint8: every picture in the top-left corner of its frame, zero elsewhere (what collate._pad_raw_u8 builds,
    also for ragged clips)"""
    flat = [clip for video in clips for clip in video]
    T = max(len(c) for c in flat)
    H = max(pixels(n).shape[0] for c in flat for n in c)
    W = max(pixels(n).shape[1] for c in flat for n in c)
    out = np.zeros((len(clips), len(clips[0]), T, H, W, 3), dtype=np.uint8)
    for b, video in enumerate(clips):
        for i, clip in enumerate(video):
            for t, n in enumerate(clip):
                p = pixels(n)
                out[b, i, t, :p.shape[0], :p.shape[1]] = p
    return torch.from_numpy(out)
