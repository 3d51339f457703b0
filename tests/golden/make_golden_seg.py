#!/usr/bin/env python
"""Generate tests/golden/seg_labels.npz by running the REFERENCE's own label code (build container only, CPU).

    python tests/golden/make_golden_seg.py         # needs the reference checkout (CFN_REFERENCE, default /root/reference) and PIL

The reference's ``charades_fine`` is imported as it is (stub modules stand in for its unused imports h5py, cv2 and torchvision), pointed at
a temporary annotation file and temporary frame directories of 1 x 1 JPEGs, and asked for

  * ``make_dataset``: the dense (157, num_frames) label array of every video (charades_fine.py:110-117),
  * ``Charades.__getitem__`` for 'training' and for 'testing' with task='loc' (frames=80*4, gamma_tau=5 as train_fine.py:57-88 passes
    them): the label window (charades_fine.py:149-165, :188).  ``random`` is re-seeded before each training item and the
    ``randint(1, max(gamma_tau, nf - frames))`` draw is repeated afterwards to learn start_f,
  * ``mt_collate_fn`` of three ragged batches (charades_fine.py:201-224).

Videos: 24 real records of the reference's data/charades.json (one without an action, the one with 28 actions, overlapping same-class
segments, a segment from 0.0, a segment ending past the duration; num_frames = duration x 12, 24, 30 or 23.976, at least 162) and 18
crafted ones whose segment bounds sit exactly ON frame times: integral fps with bounds on whole frame times (10.0 s at 240 frames,
[2.0, 5.0]: frame 48 is 0, frame 49 is 1), and bounds set to the exact doubles f0 / fps and f1 / fps (frames f0 and f1 are 0).  The script
ASSERTS that each of fr * (1 / fps), fr * duration / num_frames and fp32 arithmetic mislabels at least one element of the crafted set, so
the fixture cannot silently lose its teeth.

Stored per video: the annotation record, num_frames, the seed and start_f of the training item, and the three label arrays bit-packed;
per batch: the member indices and mt_collate_fn's labels and masks bit-packed.  Nothing of the reference's source is copied.
(numpy.save is a no-op while the Dataset is built: make_dataset caches a ragged list that current numpy refuses to save.)
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('CFN_REFERENCE', '/root/reference')

for name in ('h5py', 'cv2', 'torchvision'):               # imported by the reference, unused on this path
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
tv = sys.modules['torchvision']
if not hasattr(tv, '__file__'):                           # the stub: get_default_image_loader() asks for these two
    tv.set_image_backend = lambda backend: None
    tv.get_image_backend = lambda: 'PIL'
sys.path.insert(0, REF)
import charades_fine as cf  # noqa: E402  (reference)

FRAMES, GAMMA_TAU, C = 80 * 4, 5, 157                     # train_fine.py:57-88
RATES = (12.0, 24.0, 30.0, 23.976)


class StubTransform(object):
    def randomize_parameters(self, size):
        pass

    def __call__(self, img):
        return torch.zeros(1, 1, 1)


def real_records():
    with open(os.path.join(REF, 'data', 'charades.json')) as fh:
        data = json.load(fh)
    vids = sorted(data)

    def overlaps(r):
        A = r['actions']
        return any(a is not b and a[0] == b[0] and a[1] < b[2] and b[1] < a[2] for a in A for b in A)
    picked = []

    def first(pred, short=True):
        picked.append(next(v for v in vids if v not in picked and (not short or 8.0 < data[v]['duration'] < 40.0) and pred(data[v])))

    first(lambda r: not r['actions'])
    first(lambda r: len(r['actions']) == 28, short=False)
    first(overlaps)
    first(lambda r: any(a[1] == 0.0 for a in r['actions']))
    first(lambda r: any(a[2] > r['duration'] for a in r['actions']))
    pool = [v for v in vids if 8.0 < data[v]['duration'] < 40.0 and data[v]['actions'] and v not in picked]
    picked += pool[::len(pool) // 19][:19]
    out = []
    for i, v in enumerate(picked):
        r = data[v]
        out.append((v, {'subset': r['subset'], 'duration': r['duration'], 'actions': r['actions']},
                    max(162, int(round(r['duration'] * RATES[i % len(RATES)])))))
    return out


def crafted_records():
    out = []
    # integral fps, bounds on whole frame times
    for i, (nf, dur, segs) in enumerate([(240, 10.0, [[3, 2.0, 5.0]]),
                                         (250, 10.0, [[0, 1.0, 4.0], [156, 4.0, 10.0]]),
                                         (300, 10.0, [[7, 0.0, 3.0], [7, 3.0, 10.0], [8, 9.9, 12.0]]),
                                         (180, 15.0, [[1, 0.25, 0.5], [2, 7.0, 7.5], [2, 7.25, 14.0]]),
                                         (720, 30.0, [[5, 1.0, 29.0], [6, 29.0, 31.0]]),
                                         (900, 30.0, [[9, 0.1, 0.2], [10, 10.0, 20.0], [11, 20.0, 30.0]])]):
        out.append(('CRAFT_INT%02d' % i, {'subset': 'training', 'duration': dur, 'actions': segs}, nf))
    # bounds that ARE the frame times, as the exact doubles f0 / fps and f1 / fps
    rng = random.Random(1234)
    for i, (nf, dur) in enumerate([(287, 11.37), (162, 6.71), (333, 13.9), (701, 29.23), (455, 18.98), (199, 8.3), (1013, 33.79),
                                   (650, 21.7), (649, 27.07), (271, 9.04), (815, 34.0), (400, 16.69)]):
        fps = nf / dur
        segs = []
        for c in rng.sample(range(C), 6):
            f0 = rng.randrange(0, nf - 2)
            f1 = rng.randrange(f0 + 1, nf)
            segs.append([c, f0 / fps, f1 / fps])
        out.append(('CRAFT_EXA%02d' % i, {'subset': 'training', 'duration': dur, 'actions': segs}, nf))
    return out


def wrong_formulas(rec, nf):
    """the three restatements that are NOT the reference's expression: {name: (157, nf) array}"""
    dur = rec['duration']
    fps = nf / dur
    fr = np.arange(nf, dtype=np.float64)
    xs = {'fr * (1 / fps)': fr * (1.0 / fps), 'fr * duration / num_frames': fr * dur / nf}
    res = {}
    for k, x in xs.items():
        lab = np.zeros((C, nf), np.float32)
        for c, s, e in rec['actions']:
            lab[c, (x > s) & (x < e)] = 1
        res[k] = lab
    x32 = fr.astype(np.float32) / np.float32(fps)
    lab = np.zeros((C, nf), np.float32)
    for c, s, e in rec['actions']:
        lab[c, (x32 > np.float32(s)) & (x32 < np.float32(e))] = 1
    res['fp32'] = lab
    return res


def pack(a):
    a = np.asarray(a)
    assert set(np.unique(a)) <= {0.0, 1.0}
    return np.packbits(a.astype(np.uint8).reshape(-1)), np.asarray(a.shape, np.int64)


def build(split_file, split, root):
    np_save, np.save = np.save, (lambda *a, **k: None)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return cf.Charades(split_file, split, root, StubTransform(), task='loc', frames=FRAMES, gamma_tau=GAMMA_TAU, crops=1)
    finally:
        np.save = np_save


def main():
    records = real_records() + crafted_records()
    n_real = len(records) - len(crafted_records())
    buf = io.BytesIO()
    Image.new('RGB', (1, 1)).save(buf, format='JPEG')
    jpeg = buf.getvalue()
    out, meta = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'frames')
        for vid, _rec, nf in records:
            os.makedirs(os.path.join(root, vid))
            for i in range(1, nf + 1):
                with open(os.path.join(root, vid, vid + '-' + str(i).zfill(6) + '.jpg'), 'wb') as fh:
                    fh.write(jpeg)
        sets = {}
        for split in ('training', 'testing'):
            path = os.path.join(tmp, split + '.json')
            with open(path, 'w') as fh:
                json.dump({vid: dict(rec, subset=split) for vid, rec, _nf in records}, fh)
            sets[split] = build(path, split, root)
        tr, te = sets['training'], sets['testing']
        assert [d[0] for d in tr.data] == [r[0] for r in records] == [d[0] for d in te.data]
        items = {'training': [], 'testing': []}
        wrong = {}
        for i, (vid, rec, nf) in enumerate(records):
            _vid, full, dur, nf_ref = tr.data[i]
            assert nf_ref == nf and full.shape == (C, nf) and np.array_equal(full, te.data[i][1])
            seed = 1000 + i
            random.seed(seed)
            clips, lab_tr, _ = tr[i]
            random.seed(seed)
            frames = min(tr.frames, nf)
            start_f = random.randint(1, max(tr.gamma_tau, nf - frames))
            lab_tr = lab_tr.numpy()
            assert np.array_equal(lab_tr, full[:, start_f - 1:start_f - 1 + frames])
            clips_te, lab_te, _ = te[i]
            lab_te = lab_te.numpy()
            assert lab_te.shape[1] == (nf // te.gamma_tau) * te.gamma_tau
            items['training'].append((clips, torch.from_numpy(lab_tr), vid))
            items['testing'].append((clips_te, torch.from_numpy(lab_te), vid))
            meta.append({'vid': vid, 'duration': rec['duration'], 'actions': rec['actions'], 'num_frames': nf, 'seed': seed, 'start_f': start_f,
                         'frames': tr.frames, 'gamma_tau': tr.gamma_tau, 'crafted': i >= n_real})
            for key, a in (('full', full), ('train', lab_tr), ('test', lab_te)):
                out['%s_%d' % (key, i)], out['%s_shape_%d' % (key, i)] = pack(a)
            if i >= n_real:
                for k, lab in wrong_formulas(rec, nf).items():
                    wrong[k] = wrong.get(k, 0) + int((lab != full).sum())
        # the crafted set must tell the reference's expression from each restatement
        print('elements of the crafted set each restatement mislabels:', wrong)
        assert all(n > 0 for n in wrong.values()), wrong
        lens = [m['num_frames'] for m in meta]
        assert any(nf - min(tr.frames, nf) < tr.gamma_tau for nf in lens[:n_real]) and any(nf > tr.frames + tr.gamma_tau for nf in lens[:n_real])
        assert items['training'][n_real][1][3, 47].item() == 0 and items['testing'][n_real][1][3, 48].item() == 0 \
            and items['testing'][n_real][1][3, 49].item() == 1          # CRAFT_INT00: 10.0 s at 240 frames, [2.0, 5.0]
        # three ragged batches through the reference's collate: 5 real training windows cut by the end of the video (TLmax no multiple of
        # 64), 8 crafted testing windows, 6 crafted training windows with an odd TLmax
        cut = [i for i in range(n_real) if items['training'][i][1].shape[1] % 64 and items['training'][i][1].shape[1] < tr.frames]
        odd = [i for i in range(n_real, len(records)) if items['training'][i][1].shape[1] % 2]
        batches = {'a': ('training', cut[:5]), 'b': ('testing', list(range(n_real, n_real + 8))), 'c': ('training', odd[:6])}
        assert 0 in batches['a'][1] and len(odd) >= 6
        for name, (split, idx) in batches.items():
            _clips, labels, masks, vids = cf.mt_collate_fn([items[split][i] for i in idx])
            assert list(vids) == [records[i][0] for i in idx]
            assert len(set(items[split][i][1].shape[1] for i in idx)) > 1, 'a ragged batch expected'
            out['batch_%s_labels' % name], out['batch_%s_labels_shape' % name] = pack(labels.numpy())
            out['batch_%s_masks' % name], out['batch_%s_masks_shape' % name] = pack(masks.numpy())
            out['batch_%s_index' % name] = np.asarray(idx, np.int64)
            out['batch_%s_split' % name] = np.asarray(split)
    out['records'] = np.asarray(json.dumps(meta))
    path = os.path.join(HERE, 'seg_labels.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d videos (%d real, %d crafted), %d bytes' % (path, len(meta), n_real, len(meta) - n_real, os.path.getsize(path)))


if __name__ == '__main__':
    main()
