"""tests/golden/seg_labels.npz (make_golden_seg.py: the reference's make_dataset, Charades.__getitem__ and mt_collate_fn run on 24 real and 18
crafted annotation records) as the segment-label tests read it; loaded once and left unchanged."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SPLITS = ('training', 'testing')


@functools.lru_cache(maxsize=None)
def _npz():
    z = np.load(os.path.join(GOLDEN, 'seg_labels.npz'), allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def records():
    """per video: vid, duration, actions, num_frames, seed, start_f, frames (the Dataset's window, 640), gamma_tau (its stride, 10), crafted"""
    return json.loads(str(_npz()['records']))


def _unpack(key, shape_key):
    z = _npz()
    shape = tuple(int(s) for s in z[shape_key])
    return np.unpackbits(z[key])[:int(np.prod(shape))].reshape(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def expected(i, kind):
    """the reference's array of video i: 'full' = make_dataset's (157, num_frames); 'training' / 'testing' = what __getitem__ returned"""
    name = {'full': 'full', 'training': 'train', 'testing': 'test'}[kind]
    a = _unpack('%s_%d' % (name, i), '%s_shape_%d' % (name, i))
    a.setflags(write=False)
    return a


def seglabel(i, kind):
    """video i's SegLabel for the same window, through the constructors a Dataset would call"""
    from cfn_hip.seglabels import SegLabel
    r = records()[i]
    if kind == 'training':
        return SegLabel.training(r['actions'], r['num_frames'], r['duration'], r['start_f'], r['frames'])
    if kind == 'testing':
        return SegLabel.testing(r['actions'], r['num_frames'], r['duration'], r['gamma_tau'])
    return SegLabel(r['actions'], r['num_frames'] / r['duration'], 0, r['num_frames'])


@functools.lru_cache(maxsize=None)
def batch(name):
    """mt_collate_fn's output for batch 'a' (5 real training windows cut by the end of the video), 'b' (8 crafted testing windows) or
    'c' (6 crafted training windows, odd TLmax):
    (split, video indices, labels (B, 157, TLmax), masks (B, TLmax))"""
    z = _npz()
    labels, masks = (_unpack('batch_%s_%s' % (name, k), 'batch_%s_%s_shape' % (name, k)) for k in ('labels', 'masks'))
    labels.setflags(write=False)
    masks.setflags(write=False)
    return str(z['batch_%s_split' % name]), [int(i) for i in z['batch_%s_index' % name]], labels, masks
