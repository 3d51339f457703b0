"""Writes tests/golden/jpeg_u8.npz (the decoder's fixtures) and tests/golden/jpeg_bench.npz (the frames of tools/jpeg_decode_bench.py).
Needs PIL and numpy; the coverage flags are computed with cfn_hip.jpegdec's reference decoder.

    python tests/golden/make_golden_jpeg.py

Per case the npz holds the JPEG bytes (`<name>.jpg`) and the pixels PIL decodes from them (`<name>.rgb`, Image.open().convert('RGB'), stored as
horizontal differences: see delta()).
The cases are the shapes at which a decoder can still go wrong: one MCU, partial MCUs on both axes with odd chroma extents, exact
multiples; smooth and white-noise content; every sampling type; default and optimised Huffman tables; quality 10 and 100 (clamping, full
63-coefficient blocks); restart markers; one gray image; one progressive and one CMYK file (bytes only) for the refusals."""
import io
import os
import sys

import numpy as np
from PIL import Image, features
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'coarse-fine-networks_amd'))
from cfn_hip import jpegdec  # noqa: E402

SIZES = [(16, 16), (9, 17), (33, 31), (37, 50), (48, 64)]           # h, w
SETTINGS = [('420q75', dict(quality=75, subsampling='4:2:0')),
            ('420q95', dict(quality=95, subsampling='4:2:0')),
            ('444q90', dict(quality=90, subsampling='4:4:4')),
            ('422q75', dict(quality=75, subsampling='4:2:2')),
            ('420q50opt', dict(quality=50, subsampling='4:2:0', optimize=True)),
            ('420q10', dict(quality=10, subsampling='4:2:0')),
            ('420q100', dict(quality=100, subsampling='4:2:0')),
            ('420q75rst3', dict(quality=75, subsampling='4:2:0', restart_marker_blocks=3))]
# white noise does not compress, and the file has a size cap: the two largest sizes carry their noise image in these settings only (every
# sampling type, the full 63-coefficient blocks of quality 100); every other combination of size, content and setting is present
NOISE_LARGE = ('420q100', '444q90', '422q75')


def smooth(h, w, rng):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 255.0 * (x + y) / max(h + w - 2, 1)], axis=2)
    return np.clip(img + rng.normal(0.0, 2.0, img.shape), 0, 255).astype(np.uint8)


def noise(h, w, rng):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def photo(h, w, rng):
    """photo-like: soft shapes over a gradient, some texture"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([120 + 80 * np.sin(x / 37.0 + y / 91.0), 110 + 70 * np.cos(x / 53.0 - y / 29.0), 90 + 60 * np.sin((x + y) / 61.0)], axis=2)
    for _ in range(12):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(8, min(h, w) / 3)
        m = ((y - cy) ** 2 + (x - cx) ** 2) < r * r
        img[m] = 0.5 * img[m] + 0.5 * rng.uniform(0, 255, 3)
    return np.clip(img + rng.normal(0.0, 4.0, img.shape), 0, 255).astype(np.uint8)


def delta(rgb):
    """the pixels as differences to the left neighbour, modulo 256 (gradients then compress; np.cumsum(..., axis=1, dtype=np.uint8) undoes it)"""
    d = rgb.copy()
    d[:, 1:] = rgb[:, 1:] - rgb[:, :-1]
    return d


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', **kw)
    return buf.getvalue()


def main():
    rng = np.random.default_rng(20261018)
    out, names = {}, []
    cover = dict(zrl=0, coef63=0, stuffed=0, longest_code=0, restart=0)
    for h, w in SIZES:
        for kind, make in (('smooth', smooth), ('noise', noise)):
            img = make(h, w, rng)
            for tag, kw in SETTINGS:
                if kind == 'noise' and h * w > 33 * 31 and tag not in NOISE_LARGE:
                    continue
                name = '%dx%d_%s_%s' % (h, w, kind, tag)
                out[name + '.jpg'] = np.frombuffer(encode(img, **kw), dtype=np.uint8)
                names.append(name)
    gray = smooth(33, 31, rng)[:, :, 0]
    buf = io.BytesIO()
    Image.fromarray(gray, mode='L').save(buf, format='JPEG', quality=85)
    out['33x31_gray_q85.jpg'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    names.append('33x31_gray_q85')
    for name in names:
        jpg = out[name + '.jpg']
        rgb = np.asarray(Image.open(io.BytesIO(jpg.tobytes())).convert('RGB'))
        out[name + '.rgb'] = delta(rgb)
        info = jpegdec.parse(jpg)
        stats = {}
        planes = jpegdec.decode_coefficients(jpg, info, stats)
        seg = jpg[info.scan_start:info.scan_end]
        ff = np.flatnonzero(seg[:-1] == 0xFF)
        cover['zrl'] += stats['zrl']
        cover['longest_code'] = max(cover['longest_code'], stats['longest_code'])
        cover['coef63'] += int(sum((p[..., 63] != 0).sum() for p in planes))
        cover['stuffed'] += int((seg[ff + 1] == 0).sum())
        cover['restart'] += int(((seg[ff + 1] & 0xF8) == 0xD0).sum())
    assert cover['zrl'] >= 1, cover
    assert cover['coef63'] >= 1, cover
    assert cover['stuffed'] >= 1, cover
    assert cover['longest_code'] >= 10, cover
    assert cover['restart'] >= 1, cover
    base = smooth(33, 31, rng)
    out['refuse_progressive.jpg'] = np.frombuffer(encode(base, quality=75, progressive=True), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(base).convert('CMYK').save(buf, format='JPEG', quality=75)
    out['refuse_cmyk.jpg'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    out['names'] = np.array(names)
    out['coverage'] = np.array([cover[k] for k in ('zrl', 'coef63', 'stuffed', 'longest_code', 'restart')], dtype=np.int64)
    out['versions'] = np.array(['Pillow ' + PIL.__version__, 'libjpeg ' + str(features.version('jpg'))])
    path = os.path.join(HERE, 'jpeg_u8.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', len(names), 'cases; coverage', cover)
    assert os.path.getsize(path) < 256 * 1024

    bench = {}
    for h, w in ((180, 320), (240, 320), (360, 480)):
        bench['%dx%d.jpg' % (h, w)] = np.frombuffer(encode(photo(h, w, rng), quality=75, subsampling='4:2:0'), dtype=np.uint8)
    bench['versions'] = out['versions']
    path = os.path.join(HERE, 'jpeg_bench.npz')
    np.savez_compressed(path, **bench)
    print(path, os.path.getsize(path), 'bytes;', {k: v.size for k, v in bench.items() if k.endswith('.jpg')})
    assert os.path.getsize(path) < 256 * 1024


if __name__ == '__main__':
    main()
