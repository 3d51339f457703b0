"""extract_fineFEAT -- runs the trained Fine stream as a feature tower over whole videos and stores the five
multi-level feature maps per video, in the reference's on-disk format (extract_fineFEAT.py:153-173; read back by
charades_coarse_fineFEAT.py:84-87):

    <save_dir>/<key>/<vid>     one ``torch.save``d fp32 CPU tensor of shape (1, C_key, T', 7, 7)
    keys = layer1 (24), layer2 (48), layer3 (96), layer4 (192), conv5 (432)

``x3d_fine.generate_model(..., global_tower=True)`` produces them with the HIP path (adaptive (None,7,7)
average pooling of every stage output, x3d_fine.py:339-363).  ``extract(videos)`` takes any iterable of
(vid, clip (1,3,T,224,224)); the Charades frame reader itself is out of scope.  A clip may also be uint8 frames:
U8Clips (1,T,224,224,3), or RawU8Clips -- the frames as decoded plus a crop box (cfn_hip.u8aug.center_crop_params), cropped and
resized on the GPU as the reference's CenterCropScaled does on the CPU (extract_fineFEAT.py:76).

``extract(..., feat_dtype='fp16' | 'bf16')`` writes ONE packed 16-bit record per video instead, ``<save_dir>/packed/<vid>.cff``
(cfn_hip/featpack.py): the five maps are rounded and laid out time-major on the GPU (ops.feat_pack) and read back in one copy."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3d_fine                                   # noqa: E402
from cfn_hip.u8clips import RawU8Clips            # noqa: E402
from cfn_hip.jpegdec import JpegClips, decode_checked   # noqa: E402
from cfn_hip import featpack                      # noqa: E402

FEAT_KEYS = ('layer1', 'layer2', 'layer3', 'layer4', 'conv5')


def build_tower(device, ckpt=None, n_classes=157, input_norm=None):
    """input_norm = (mean, std[, norm_value]): extract() then also takes videos as uint8 frames (cfn_hip.u8clips.U8Clips, frames
    (1, T, H, W, 3)), normalised in the stem conv -- the reference's Normalize(CHARADES_MEAN, CHARADES_STD), extract_fineFEAT.py:78"""
    net = x3d_fine.generate_model('M', n_classes=n_classes, n_input_channels=3, task='loc', dropout=0.5,
                                  base_bn_splits=1, global_tower=True)
    if ckpt and os.path.exists(ckpt):
        net.load_state_dict(torch.load(ckpt, map_location='cpu')['model_state_dict'])
    if input_norm is not None:
        net.set_input_norm(*input_norm)
    net.to(device).train(False)
    net.aggregate_sub_bn_stats()          # extract_fineFEAT.py:136-139
    return net


@torch.no_grad()
def extract(net, videos, save_dir, device='cuda', crop=224, feat_dtype=None, jpeg_entropy=None):
    """feat_dtype None: the reference's five fp32 files per video; 'fp16' / 'bf16': one packed record per video.  jpeg_entropy: how JpegClips
    videos are entropy-decoded, 'interval' or 'sync' (cfn_hip.jpegdec.decode_checked); None leaves the choice to CFN_JPEG_ENTROPY"""
    dt = None if feat_dtype is None else featpack.feat_dtype(feat_dtype)
    if dt is None:
        for k in FEAT_KEYS:
            os.makedirs(os.path.join(save_dir, k), exist_ok=True)
    else:
        from cfn_hip import ops
    n = 0
    for vid, clip in videos:
        if isinstance(clip, JpegClips):            # frames still JPEG: decoded on the device into the RawU8Clips batch (one status read-back)
            clip = decode_checked(clip, device, [vid], entropy=jpeg_entropy).flatten_crops()
        clip = clip.to(device)
        if isinstance(clip, RawU8Clips):
            clip = clip.transform(crop)
        feat, _ = net([clip, None])
        if dt is None:
            for k in FEAT_KEYS:
                torch.save(feat[k].data.cpu(), os.path.join(save_dir, k, vid))
        else:
            maps = [feat[k].data for k in FEAT_KEYS]
            payload = ops.feat_pack(maps, dt).cpu()            # one read-back per video
            featpack.write_record(featpack.record_path(save_dir, vid), payload, dt, maps[0].shape[-3], [m.shape[-4] for m in maps])
        n += 1
    return n


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('-gpu', default='0')
    ap.add_argument('--save-dir', default='fine_feat')
    ap.add_argument('--ckpt', default='models/fine_charades_039000_SAVE.pt')
    ap.add_argument('--synthetic', type=int, default=2, help='number of synthetic videos to run')
    ap.add_argument('--feat-dtype', default=None, choices=['fp16', 'bf16'],
                    help='write one packed 16-bit record per video (<save-dir>/packed/<vid>.cff) instead of five fp32 files')
    ap.add_argument('--jpeg-entropy', choices=('interval', 'sync'), default=None,
                    help='entropy mode of the GPU JPEG decode: sync = parallel inside a frame without restart markers')
    a = ap.parse_args()
    os.environ.setdefault('CUDA_VISIBLE_DEVICES', a.gpu)
    g = torch.Generator().manual_seed(0)
    vids = (('synthetic_%03d' % i, torch.randn(1, 3, 64, 224, 224, generator=g)) for i in range(a.synthetic))
    print('wrote', extract(build_tower('cuda', a.ckpt), vids, a.save_dir, feat_dtype=a.feat_dtype, jpeg_entropy=a.jpeg_entropy), 'videos to', a.save_dir)
