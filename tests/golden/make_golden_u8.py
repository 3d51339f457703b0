#!/usr/bin/env python
"""Generate tests/golden/clip_u8.npz by running the REFERENCE's own input pipeline (build container only).

    python tests/golden/make_golden_u8.py          # needs the reference checkout (CFN_REFERENCE, default /root/reference)

A few small uint8 frames that contain every byte value in every channel go through the reference's ToTensor(255) and
Normalize(CHARADES_MEAN, CHARADES_STD) per frame (transforms/spatial_transforms.py:37-118) and its stack + permute per clip
(charades_fine.py:170-173).  Stored: the frames (T, H, W, 3) uint8, the fp32 clip (3, T, H, W) the reference produced, and the
mean / std / norm_value it was given.  Nothing of the reference's source is copied.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('CFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from transforms.spatial_transforms import Compose, Normalize, ToTensor  # noqa: E402  (reference)

MEAN = [0.413, 0.368, 0.338]          # CHARADES_MEAN / CHARADES_STD of the reference's train_fine.py:48-49
STD = [0.131, 0.125, 0.132]
T, H, W = 4, 16, 16


def main():
    i = np.arange(T * H * W, dtype=np.int64).reshape(T, H, W, 1)
    c = np.arange(3, dtype=np.int64).reshape(1, 1, 1, 3)
    frames = ((i * 37 + c * 101 + (i // 256) * 11) % 256).astype(np.uint8)          # every byte value 4 times per channel
    for ch in range(3):
        assert len(np.unique(frames[..., ch])) == 256
    tf = Compose([ToTensor(255), Normalize(MEAN, STD)])
    tf.randomize_parameters(224)
    imgs_l = [tf(img) for img in frames]                                   # charades_fine.py:172 (numpy frames)
    clip = torch.stack(imgs_l, 0).permute(1, 0, 2, 3)                      # charades_fine.py:173: T C H W --> C T H W
    try:                                                                   # the PIL route of ToTensor gives the same values
        from PIL import Image
        pil = torch.stack([tf(Image.fromarray(img)) for img in frames], 0).permute(1, 0, 2, 3)
        assert torch.equal(pil, clip)
    except ImportError:
        pass
    out = os.path.join(HERE, 'clip_u8.npz')
    np.savez_compressed(out, frames=frames, clip=clip.contiguous().numpy(), mean=np.asarray(MEAN), std=np.asarray(STD),
                        norm_value=np.asarray(255))
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
