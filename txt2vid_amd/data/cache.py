"""Write the frame cache of a frame-folder dataset ahead of a run (what the reference's create_cache.py was for): later runs
name the file as `cache_file` in their `--data` spec and skip the decode.

    python -m txt2vid_amd.data.cache --data DIR --anno P --vocab V --frame_size S --num_channels C [--random_frames N] [--crop_jitter J] [--window S] --out FILE
"""
import argparse

from . import Vocab, default_transform, my_dataset
from .frames import FrameCache


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--data', required=True, help='folder of <video id>/<n>.jpg|png frame folders')
    p.add_argument('--anno', required=True, help='captions pickle {video id -> [sentence, ...]}')
    p.add_argument('--vocab', default=None, help='vocabulary pickle (default: the synthetic captions\' words)')
    p.add_argument('--frame_size', type=int, nargs='+', default=[64], help='crop: S, or H W')
    p.add_argument('--num_channels', type=int, default=3)
    p.add_argument('--num_frames', type=int, default=16)
    p.add_argument('--random_frames', type=int, default=0, help='> 0: keep EVERY frame (any random pick is then a set of rows)')
    p.add_argument('--crop_jitter', type=int, default=0, help='J > 0: store the crop with a margin of J pixels (serves crop_jitter <= J)')
    p.add_argument('--window', type=int, default=0, help='S > 0: keep EVERY frame, for a data set that reads windows of stride S')
    p.add_argument('--out', required=True, help='cache file (.npy; the sidecar is <out>.json)')
    args = p.parse_args(argv)
    if args.vocab:
        from ..util.pick import load
        vocab = load(args.vocab)
    else:
        vocab = Vocab()
    dset = my_dataset(data=args.data, vocab=vocab, anno=args.anno, transform=default_transform(args.frame_size, args.num_channels),
                      random_frames=args.random_frames, num_frames=args.num_frames, crop_jitter=args.crop_jitter, window=args.window)
    cache = FrameCache.build(dset)
    path = cache.save(args.out)
    print('%s: %d frames of %dx%dx%d uint8 (%d videos, %d items), %.1f MB, decoded in %.2f s'
          % (path, cache.block.shape[0], cache.channels, cache.stored[0], cache.stored[1], len(cache.table), len(dset), cache.nbytes / 1e6,
             cache.seconds))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
