#!/usr/bin/env python
"""Generate tests/golden/aug_u8*.npz and aug_params.npz by running the REFERENCE's own spatial transforms (build container only).

    python tests/golden/make_golden_aug.py         # needs the reference checkout (CFN_REFERENCE, default /root/reference) and PIL

Random uint8 frames go, frame by frame as PIL images, through the reference's training transform
``Compose([MultiScaleRandomCropMultigrid([S/256, S/320] = [0.875, 0.7], S), RandomHorizontalFlip()])`` (train_fine.py:74-75) --
once with a draw that flips and once with one that does not -- and through its validation transform ``CenterCropScaled(S)``
(train_fine.py:78).  Stored: the source frames, the (x1, y1, c, flip) each transform used, and the bytes it produced.

  aug_u8.npz               S = 32 from 45 x 80 (near identity), 24 x 32 (upscale) and 140 x 190 (about 4x down); T = 3
  aug_u8_224a.npz          S = 224 from 180 x 320, T = 1: source, boxes, CenterCropScaled output;  aug_u8_224a_train.npz: the two training outputs
  aug_u8_224b.npz / _train the same from 256 x 340
  aug_params.npz           for a few seeds and frame sizes: what randomize_parameters drew (scale, tl_x, tl_y, p) and the boxes

Nothing of the reference's source is copied.
"""
import os
import random
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('CFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from transforms.spatial_transforms import CenterCropScaled, Compose, MultiScaleRandomCropMultigrid, RandomHorizontalFlip  # noqa: E402  (reference)

RESIZE = [256, 320]                   # train_fine.py: scales = crop_size / 256, crop_size / 320 = 0.875, 0.7 at 224


def scales_of(S):
    return [224 / r for r in RESIZE]                                      # 0.875 and 0.7, whatever the output extent


def run_train(frames, S, want_flip, seed0):
    """the first seed from seed0 on whose draw flips / does not flip; returns (box, out)"""
    h, w = frames.shape[1:3]
    for seed in range(seed0, seed0 + 64):
        tf = Compose([MultiScaleRandomCropMultigrid(scales_of(S), S), RandomHorizontalFlip()])
        random.seed(seed)
        tf.randomize_parameters(S)
        crop, flip = tf.transforms
        if (flip.p < 0.5) != want_flip:
            continue
        c = int(min(h, w) * crop.scale)
        box = (int(crop.tl_x * (w - c)), int(crop.tl_y * (h - c)), c, int(flip.p < 0.5))
        out = np.stack([np.asarray(tf(Image.fromarray(f))) for f in frames])
        return box, out
    raise RuntimeError('no seed with flip = %s' % want_flip)


def run_center(frames, S):
    h, w = frames.shape[1:3]
    tf = Compose([CenterCropScaled(S)])
    tf.randomize_parameters(S)
    c = min(h, w)
    box = (int(round((w - c) / 2.)), int(round((h - c) / 2.)), c, 0)
    return box, np.stack([np.asarray(tf(Image.fromarray(f))) for f in frames])


def case(seed, T, h, w, S):
    frames = np.random.RandomState(seed).randint(0, 256, size=(T, h, w, 3)).astype(np.uint8)
    b0, o0 = run_train(frames, S, False, 100 * seed)
    b1, o1 = run_train(frames, S, True, 100 * seed)
    b2, o2 = run_center(frames, S)
    for o in (o0, o1, o2):
        assert o.shape == (T, S, S, 3) and o.dtype == np.uint8
    return frames, np.asarray([b0, b1, b2], dtype=np.int32), np.stack([o0, o1, o2])


def save(name, **arrays):
    out = os.path.join(HERE, name + '.npz')
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print('wrote', out, size, 'bytes')
    assert size < 512 * 1024, name


def main():
    small = {}
    for tag, seed, (h, w) in (('near', 1, (45, 80)), ('up', 2, (24, 32)), ('down', 3, (140, 190))):
        src, box, out = case(seed, 3, h, w, 32)
        small.update({tag + '_src': src, tag + '_box': box, tag + '_out': out})
        print(tag, (h, w), 'boxes', box.tolist())
    save('aug_u8', size=np.asarray(32), cases=np.asarray(['near', 'up', 'down']), **small)
    for tag, seed, (h, w) in (('224a', 4, (180, 320)), ('224b', 5, (256, 340))):
        src, box, out = case(seed, 1, h, w, 224)
        print(tag, (h, w), 'boxes', box.tolist())
        save('aug_u8_' + tag, size=np.asarray(224), src=src, box=box, out_center=out[2])
        save('aug_u8_' + tag + '_train', out_train=out[:2])

    # what randomize_parameters draws, and the boxes that follow from it
    seeds, hws, draws, boxes, centers = [], [], [], [], []
    for seed in (0, 1, 7, 123, 2024):
        for h, w in ((180, 320), (240, 320), (360, 480), (256, 340), (320, 240), (45, 80)):
            tf = Compose([MultiScaleRandomCropMultigrid(scales_of(224), 224), RandomHorizontalFlip()])
            random.seed(seed)
            tf.randomize_parameters(224)
            crop, flip = tf.transforms
            c = int(min(h, w) * crop.scale)
            seeds.append(seed)
            hws.append((h, w))
            draws.append((crop.scale, crop.tl_x, crop.tl_y, flip.p))
            boxes.append((int(crop.tl_x * (w - c)), int(crop.tl_y * (h - c)), c, int(flip.p < 0.5)))
            # the box CenterCropScaled uses, read off its output: the crop of an index image at full size
            cc = min(h, w)
            idx = np.arange(h * w, dtype=np.int32).reshape(h, w)
            o = np.asarray(CenterCropScaled(cc)(Image.fromarray(idx, mode='I')))
            assert o.shape == (cc, cc)
            centers.append((int(o[0, 0]) % w, int(o[0, 0]) // w, cc, 0))
    save('aug_params', seeds=np.asarray(seeds), hw=np.asarray(hws, dtype=np.int32), scales=np.asarray(scales_of(224)),
         draws=np.asarray(draws, dtype=np.float64), boxes=np.asarray(boxes, dtype=np.int32), centers=np.asarray(centers, dtype=np.int32))


if __name__ == '__main__':
    main()
