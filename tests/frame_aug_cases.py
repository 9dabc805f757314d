"""Shared by test_frame_aug_cpu.py / test_frame_aug_gpu.py: the augmented clips of a frame-folder `Dataset` (hflip, crop_jitter,
window) constructed INDEPENDENTLY of `default_transform` — plain numpy slicing of the zero-padded, converted source image — and the
documented draw order replayed by hand (no test in here)."""
import os

import numpy as np
from PIL import Image

from txt2vid_amd import data as D

# (h, w) of the four videos of frame_cases.make_tree: (w - 64) and (h - 64) are ODD for vid0, (w - 30) odd for vid1 — with an odd
# margin that is where rounding an enlarged crop's offset (half to even) would differ from the plain crop's offset minus the
# margin; vid3 stays 30x30 so that the zero fill meets the margin
ODD = ((73, 81), (44, 51), (90, 100), (30, 30))
BIG_ODD = ((151, 161), (131, 141), (160, 171), (30, 30))      # around a 128x128 crop


def frame_names(root, vid):
    names = [n for n in os.listdir(os.path.join(root, vid)) if n.split('.')[0].isdigit()]
    return sorted(names, key=lambda n: int(n.split('.')[0]))


def source_window(path, crop, channels, dy=0, dx=0, flip=0, margin=0):
    """uint8 [C, h + 2 margin, w + 2 margin]: the converted image, zero-padded far beyond any offset, sliced where the crop box
    displaced by (dy, dx) lies; mirrored left to right when `flip`."""
    ch, cw = crop
    with Image.open(path) as img:
        a = np.asarray(img.convert('RGB' if channels == 3 else 'L'), dtype=np.uint8)
    a = a[None] if a.ndim == 2 else a.transpose(2, 0, 1)
    h, w = a.shape[1:]
    P = 400
    pad = np.zeros((a.shape[0], h + 2 * P, w + 2 * P), dtype=np.uint8)
    pad[:, P:P + h, P:P + w] = a
    top, left = int(np.rint((h - ch) / 2.0)), int(np.rint((w - cw) / 2.0))       # the plain centre crop's corner (half to even)
    y, x = P + top + dy - margin, P + left + dx - margin
    out = pad[:, y:y + ch + 2 * margin, x:x + cw + 2 * margin]
    return out[:, :, ::-1] if flip else out


def replay_draws(count, num_frames, window, jitter, hflip):
    """The documented per-item draws from global np.random: start, (dy, dx), flip; a key that is off draws nothing."""
    start = dy = dx = flip = 0
    if window:
        start = int(np.random.randint(0, count - ((num_frames - 1) * window + 1) + 1))
    if jitter:
        dy, dx = [int(v) for v in np.random.randint(-jitter, jitter + 1, size=2)]
    if hflip:
        flip = int(np.random.randint(0, 2))
    return start, dy, dx, flip


def expected_clip(root, vid, crop, channels, num_frames, window, start, dy, dx, flip):
    """float32 [T, C, h, w]: what `ds[i][0]` must be for these draws (without `window`: the strided pick)."""
    names = frame_names(root, vid)
    if window:
        picked = [names[start + window * t] for t in range(num_frames)]
    else:
        picked = [names[(len(names) // num_frames) * t] for t in range(num_frames)]
    return np.stack([D.unit_range(source_window(os.path.join(root, vid, n), crop, channels, dy, dx, flip)) for n in picked])


def aug_dataset(tree, crop, channels, on_device=False, **keys):
    """Through `my_dataset(**args)` with the spec's own key names, as a JSON `--data` spec reaches it."""
    root, anno = tree
    args = dict({'data': root, 'on_device': on_device}, **keys)
    return D.my_dataset(vocab=D.Vocab(), anno=anno, transform=D.default_transform([crop], channels), **args)
