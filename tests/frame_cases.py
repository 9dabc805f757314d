"""Shared by test_frame_cache_cpu.py / test_frame_cache_gpu.py: frame trees for the HBM frame cache (no test in here)."""
import pickle

import numpy as np
from PIL import Image

CAPTIONS = {'vid0': ['digit 3 is left and right.', 'a Digit moves'], 'vid1': ['digit 7 is top and bottom.'],
            'vid2': ['digit 1 is right and left.', 'digit 9 is left.'], 'vid3': ['digit 4 is top.'], 'gone': ['never read']}
# captions of EQUAL length (8, 8, 8 tokens; 6, 6) so that collate_fn's stable sort decides the order inside a batch


def make_tree(tmp_path, sizes=((72, 80), (44, 50), (90, 100), (30, 30)), frames=(40, 33, 40, 20)):
    """Four videos of noise frames (seeded): vid0 RGB .png, vid1 grey .png, vid2 RGB .jpg (quality 90), vid3 grey .jpg of 30x30
    (smaller than most crops: zero fill); vid0 and vid2 have two captions; the pickle names a missing video. -> (root, anno)."""
    rng = np.random.RandomState(11)
    root = tmp_path / 'videos'
    for v in range(4):
        d = root / ('vid%d' % v)
        d.mkdir(parents=True)
        h, w = sizes[v]
        grey, jpg = v in (1, 3), v in (2, 3)
        for n in range(frames[v]):
            a = rng.randint(0, 256, size=(h, w) if grey else (h, w, 3)).astype(np.uint8)
            a[:4, :4] = n                                    # (frame number in a corner: a wrong frame cannot pass)
            Image.fromarray(a).save(d / ('%d.%s' % (n, 'jpg' if jpg else 'png')), **({'quality': 90} if jpg else {}))
        (d / 'notes.txt').write_text('ignored')
    anno = tmp_path / 'sent.pickle'
    with open(anno, 'wb') as f:
        pickle.dump(CAPTIONS, f)
    return str(root), str(anno)


def make_golden_tree(g, tmp_path):
    """The two JPEG frame folders + captions of tests/golden/data_contract.npz, byte for byte. -> (root, anno, (h, w))."""
    for key in g.files:
        if key.startswith('jpeg_'):
            _, vid, idx = key.split('_')
            (tmp_path / vid).mkdir(exist_ok=True)
            (tmp_path / vid / ('%s.jpg' % idx)).write_bytes(g[key].tobytes())
    cap_path = tmp_path / 'captions.pkl'
    cap_path.write_bytes(pickle.dumps(pickle.loads(g['captions_pickle'].tobytes())))
    return str(tmp_path), str(cap_path), tuple(g['ds_frames_0'].shape[-2:])
