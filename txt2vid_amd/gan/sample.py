"""Sampling tool: a finished run turns captions into clips (not in the reference, whose only sampling path is `test()`:
the loader's first batch, its captions, one plain randn draw, one min/max-normalised grid).

    python -m txt2vid_amd.gan.sample --weights CKPT --data SPEC [the model flags of train.gan] [--sample_n N] [--sample_seed S]
        [--captions FILE] [--truncation TAU] [--interp S] [--standing_stats NB] [--export PATH] [--gif] [--nearest K]

The models are built as `train.gan` builds them. If the checkpoint holds `gen_ema`, the averaged generator is sampled (`--no_ema`:
the live weights). `--standing_stats NB` first recomputes the BatchNorm buffers with the weights, latents and captions that are
sampled (Brock et al. 2019): the running buffers of a checkpoint belong to the live weights. `--export PATH` writes the clips as
the frame cache's bytes, `[N*T, C*H*W]` uint8 (`t2v_clip_export`: float clips never reach the host on that path); `--nearest K`
shows each sample next to its K nearest training clips in pixel space (`t2v_clip_nn`): a figure against memorisation, not a metric.

Isolation: z and the conditioning-augmentation eps come from a device generator of the tool, truncation redraws from a host generator
of the tool, the latents of `--standing_stats` from a third pair: no global generator moves, and the recomputed buffers live for the
process only."""
import contextlib
import json
import math
import os

import numpy as np
import torch

from .. import functional as TF
from ..util.log import status

STANDING_SEED = 0x5374                 # added to --sample_seed for the latents of --standing_stats: the samples' draws stay put
SAMPLES_FILE = 'samples.json'
CAPTIONS_FILE = 'captions.txt'
NEAREST_MAX_N = 64                     # functional_sample.NN_MAX_ROWS
NEAREST_MAX_K = 8


def add_flags(parser):
    parser.add_argument('--sample_n', type=int, default=16, metavar='N', help='(new) number of latents (clips; with --interp, N/2 pairs)')
    parser.add_argument('--sample_seed', type=int, default=0, metavar='S', help="(new) seed of the tool's own generators")
    parser.add_argument('--captions', type=str, default=None, metavar='FILE',
                        help='(new) one caption per line, cycled to N (default: the captions of dataset items 0..N-1)')
    parser.add_argument('--truncation', type=float, default=None, metavar='TAU',
                        help='(new) redraw every component of z with |z| > TAU until it is inside (BigGAN); TAU > 0')
    parser.add_argument('--interp', type=int, default=None, metavar='S',
                        help="(new) S >= 2 clips on the spherical interpolation of each pair of latents, under the first one's caption")
    parser.add_argument('--standing_stats', type=int, default=0, metavar='NB',
                        help='(new) recompute the BatchNorm buffers from NB batches of the sampled weights and latents first; 0 = off')
    parser.add_argument('--gif', action='store_true', default=False, help='(new) one animated GIF per clip, from the exported bytes')
    parser.add_argument('--export', type=str, default=None, metavar='PATH',
                        help='(new) write the clips as bytes to PATH.npy ([N*T, C*H*W] uint8, the frame cache layout) and PATH.json')
    parser.add_argument('--nearest', type=int, default=0, metavar='K',
                        help='(new) show each sample with its K (1..8) nearest dataset clips in pixel space; at most 64 samples')
    parser.add_argument('--nearest_clips', type=int, default=None, metavar='M', help='(new) look at the first M dataset items only')
    parser.add_argument('--no_ema', action='store_true', default=False,
                        help='(new) sample the live weights even if the checkpoint holds an averaged generator')
    return parser


def build_parser():
    from ..train import gan as train_gan
    return add_flags(train_gan.build_parser())


def n_clips(args):
    return args.sample_n if args.interp is None else args.sample_n // 2 * args.interp


def check_args(args):
    """The flags' rules, before anything is built."""
    if getattr(args, 'weights', None) is None:
        raise SystemExit('txt2vid_amd.gan.sample samples a checkpoint: pass --weights')
    if args.captions is not None and getattr(args, 'dont_use_sent', False):
        raise SystemExit('--captions needs a text-conditioned model: it cannot run with --dont_use_sent')
    if args.sample_n < 1:
        raise ValueError('--sample_n takes a number of clips >= 1, got %d' % args.sample_n)
    if args.truncation is not None and not args.truncation > 0:
        raise ValueError('--truncation takes TAU > 0, got %r' % args.truncation)
    if args.interp is not None:
        if args.interp < 2:
            raise ValueError('--interp takes S >= 2 steps, got %d' % args.interp)
        if args.sample_n % 2:
            raise ValueError('--interp takes the latents in pairs: --sample_n must be even, got %d' % args.sample_n)
    if args.standing_stats < 0:
        raise ValueError('--standing_stats takes a number of batches >= 0 (0 = off), got %d' % args.standing_stats)
    if args.nearest:
        if not 1 <= args.nearest <= NEAREST_MAX_K:
            raise ValueError('--nearest takes 1 to %d neighbours (0 = off), got %d' % (NEAREST_MAX_K, args.nearest))
        if n_clips(args) > NEAREST_MAX_N:
            raise ValueError('--nearest is a figure, not a metric: at most %d samples, got %d' % (NEAREST_MAX_N, n_clips(args)))
        if args.nearest_clips is not None and args.nearest_clips < 1:
            raise ValueError('--nearest_clips takes a number of dataset items >= 1, got %d' % args.nearest_clips)


# ---- latents ---------------------------------------------------------------------------------------------------------------------
def generators(seed, device):
    """(device generator for z and eps, host generator for truncation redraws), both under `seed`."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    h = torch.Generator()
    h.manual_seed(int(seed))
    return g, h


def draw_latents(n, dim, gen, host_gen, tau=None, device='cpu'):
    """[n, dim] normal draws of `gen`; with `tau`, every component outside [-tau, tau] is redrawn from `host_gen` until it is
    inside. tau = inf returns the plain draw bit for bit."""
    z = torch.randn(n, dim, generator=gen, device=device)
    if tau is None:
        return z
    if not tau > 0:
        raise ValueError('truncation takes TAU > 0, got %r' % tau)
    zh = z.cpu()
    bad = zh.abs() > tau
    while bool(bad.any()):
        zh[bad] = torch.randn(int(bad.sum()), generator=host_gen)
        bad = zh.abs() > tau
    return zh.to(device)


def slerp(a, b, steps):
    """[steps, dim]: sin((1-t)w)/sin(w) a + sin(tw)/sin(w) b, t = i/(steps-1), w the angle between a and b (White 2016); computed
    in float64 on the host. Steps 0 and steps-1 are a and b bit for bit; parallel endpoints fall back to the straight line."""
    if steps < 2:
        raise ValueError('slerp takes at least 2 steps, got %d' % steps)
    a64, b64 = a.detach().cpu().double(), b.detach().cpu().double()
    na, nb = float(a64.norm()), float(b64.norm())
    cos = float((a64 * b64).sum()) / (na * nb) if na > 0 and nb > 0 else 1.0
    w = math.acos(max(-1.0, min(1.0, cos)))
    out = []
    for i in range(steps):
        t = i / float(steps - 1)
        if i == 0:
            out.append(a64)
        elif i == steps - 1:
            out.append(b64)
        elif math.sin(w) < 1e-9:
            out.append((1.0 - t) * a64 + t * b64)
        else:
            out.append(math.sin((1.0 - t) * w) / math.sin(w) * a64 + math.sin(t * w) / math.sin(w) * b64)
    return torch.stack(out).to(torch.float32)


# ---- captions --------------------------------------------------------------------------------------------------------------------
def read_captions(path):
    with open(path) as f:
        lines = [l.strip() for l in f]
    lines = [l for l in lines if l]
    if not lines:
        raise SystemExit('--captions %s holds no caption' % path)
    return lines


def tokens_of(vocab, sentence):
    """Token ids of a typed caption: <start> ... <end>, as `data.Dataset.tokens`."""
    toks = [vocab(t) for t in vocab.tokenize(sentence)]
    if toks[-1] != vocab(vocab.END):
        toks.append(vocab(vocab.END))
    return toks


def resolve_captions(args, conditional, dset, vocab, n):
    """n token lists (None for an unconditional model): --captions cycled, else the captions of dataset items 0..n-1 by index."""
    if not conditional:
        if args.captions is not None:
            raise SystemExit('--captions needs a text-conditioned model')
        return None
    if args.captions is not None:
        lines = read_captions(args.captions)
        return [tokens_of(vocab, lines[i % len(lines)]) for i in range(n)]
    if dset is None or len(dset) == 0:
        raise SystemExit('a text-conditioned model needs captions: pass --captions FILE or a dataset (--data) that holds some')
    out = []
    for i in range(n):
        k = i % len(dset)
        toks = dset.tokens(k) if hasattr(dset, 'tokens') else dset[k][1]
        out.append([int(t) for t in (toks.tolist() if hasattr(toks, 'tolist') else toks)])
    return out


def sorted_batch(token_lists):
    """(order, tokens [b, L] int64 zero-padded, lengths desc): the packed encoder's contract, as `collate_fn` sorts. `order[k]` is the
    position in `token_lists` of sorted row k."""
    order = sorted(range(len(token_lists)), key=lambda i: -len(token_lists[i]))
    lengths = [len(token_lists[i]) for i in order]
    toks = torch.zeros(len(order), lengths[0], dtype=torch.long)
    for k, i in enumerate(order):
        toks[k, :lengths[k]] = torch.tensor(token_lists[i], dtype=torch.long)
    return order, toks, lengths


def take_rows(x, rows):
    """x[rows] for a dense 2-D device tensor, any number of rows, on the copy kernel (off the hot path: one launch per row)."""
    out = torch.empty((len(rows), x.shape[1]), device=x.device, dtype=torch.float32)
    for k, i in enumerate(rows):
        TF.copy_into(x[int(i):int(i) + 1], out[k:k + 1])
    return out


def encode_captions(encoder, token_lists, device, batch=32):
    """[n, cond_dim] sentence codes in the order of `token_lists`: batches sorted by length for the encoder, then un-sorted."""
    out = []
    with torch.no_grad():
        for o in range(0, len(token_lists), batch):
            order, toks, lengths = sorted_batch(token_lists[o:o + batch])
            _, _, cond = encoder.encode(toks.to(device), lengths)
            inv = [0] * len(order)
            for k, i in enumerate(order):
                inv[i] = k
            out.append(take_rows(cond.detach(), inv))                         # row i <- sorted row inv[i]
    if len(out) == 1:
        return out[0]
    bank = torch.empty((len(token_lists), out[0].shape[1]), device=device, dtype=torch.float32)
    o = 0
    for c in out:
        TF.copy_into(c, bank[o:o + c.shape[0]])
        o += c.shape[0]
    return bank


# ---- the forward -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def sampling(gan, use_ema=True):
    """Inside: the generator in eval mode, the averaged weights swapped in (or every packed copy refreshed), no autograd; the
    recipe of `KidEvaluator._render`. On exit mode, weights, draws object and the host generator are as before."""
    gen = gan.gen
    ema = getattr(gan, 'gen_ema', None) if use_ema else None
    was_training, old_draws, host = gen.training, TF.draws, torch.get_rng_state()
    gen.eval()
    try:
        with torch.no_grad(), (ema.swapped() if ema is not None else contextlib.nullcontext()):
            if ema is None:
                TF.repack_params([p for p in gen.parameters()][::-1])
            yield gen
    finally:
        TF.set_draws(old_draws)
        gen.train(was_training)
        torch.set_rng_state(host)


def forward(gan, z, cond=None, eps=None, output_blocks=None):
    """The levels the eval-mode generator renders for these latents; `eps`: this batch's conditioning-augmentation draws."""
    from .kid import _EvalDraws
    TF.set_draws(_EvalDraws(eps))
    return gan(z, cond=cond, output_blocks=output_blocks)


def batchnorm_sites(gen):
    from ..models.layers import BatchNorm2d
    return [m for m in gen.modules() if isinstance(m, BatchNorm2d)]


def standing_stats(gan, batches):
    """Recompute running_mean / running_var of every BatchNorm2d of the generator as the plain average of the batches' statistics:
    the sites run in training mode with momentum 1/(k+1) at batch k, inside an eval-mode generator (full clips, every level
    rendered so that every site is reached). `batches`: (z, cond, eps) triples. Called inside `sampling()`. Modes and momenta are
    restored; returns the number of batches."""
    gen = gan.gen
    sites = batchnorm_sites(gen)
    saved = [(m.momentum, m.training) for m in sites]
    k = 0
    try:
        for z, cond, eps in batches:
            for m in sites:
                m.training = True
                m.momentum = 1.0 / (k + 1)                    # (torch's momentum=None; BatchNorm2d.forward takes the float)
            forward(gan, z, cond, eps, output_blocks=range(len(gen.render_blocks)))
            k += 1
    finally:
        for m, (mom, tr) in zip(sites, saved):
            m.momentum, m.training = mom, tr
    return k


# ---- nearest real clips ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def forked_host():
    """The three host generators are read back on exit: a `random_frames` dataset draws its frames from numpy's."""
    import random
    state = (random.getstate(), np.random.get_state())
    try:
        with torch.random.fork_rng(devices=[]):
            yield
    finally:
        random.setstate(state[0])
        np.random.set_state(state[1])


def _real_batch(dset, lo, hi, device):
    """Items lo..hi-1 by index, stacked and uploaded: [b, C, T, H, W] dense. Of a data set that augments its clips, the plain items
    (`Dataset.plain`: no flip, no jitter, the centred window, no draw): the search compares against the clips as they are."""
    item = dset.plain if getattr(dset, 'augmented', False) else dset.__getitem__
    x = torch.stack([item(i)[0] for i in range(lo, hi)]).to(device)
    return TF.video_to_channel_first(x)


def nearest_pass(samples, dset, K, device, limit=None, batch=32):
    """(d2 [N, K] list, idx [N, K] list): the K nearest items of dset[0 .. limit) to each sample [N, C, T, H, W], reading the
    dataset by index, in order, under forked host generators (a `random_frames` dataset draws its frames from numpy's)."""
    from .. import functional_sample as FS
    N = int(samples.shape[0])
    D = int(samples[0].numel())
    total = len(dset) if limit is None else min(int(limit), len(dset))
    batch = min(batch, FS.NN_MAX_ROWS)
    FS.check_nn_sizes(N, min(batch, max(total, 1)), D, K)
    g = samples.reshape(N, D)
    bd, bi = FS.nn_init(N, K, device)
    ws = torch.empty((int(TF.lib().t2v_clip_nn_ws_bytes(N, batch, D)),), device=device, dtype=torch.uint8)
    with forked_host():
        for lo in range(0, total, batch):
            hi = min(lo + batch, total)
            r = _real_batch(dset, lo, hi, device)
            if int(r[0].numel()) != D:
                raise ValueError('--nearest: dataset clips hold %d values, samples %d' % (int(r[0].numel()), D))
            FS.clip_nn(g, r.reshape(hi - lo, D), lo, bd, bi, ws=ws)
    return bd.tolist(), bi.tolist(), total


# ---- output ----------------------------------------------------------------------------------------------------------------------
def write_gif(path, rows, C, H, W):
    """rows: uint8 [T, C*H*W] (exported bytes of one clip) -> animated GIF."""
    from PIL import Image
    frames = []
    for row in np.asarray(rows):
        a = row.reshape(C, H, W)
        frames.append(Image.fromarray(a[0], 'L') if C == 1 else Image.fromarray(np.ascontiguousarray(a[:3].transpose(1, 2, 0)), 'RGB'))
    frames[0].save(path, save_all=True, append_images=frames[1:], duration=100, loop=0)


def write_json(path, rec):
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')


def export_record(args, shape, n, captions, iteration):
    """What PATH.json holds next to PATH.npy."""
    from ..functional_sample import BYTE_MAP
    C, T, H, W = shape
    return {'N': int(n), 'T': int(T), 'C': int(C), 'H': int(H), 'W': int(W), 'captions': captions, 'seed': int(args.sample_seed),
            'truncation': args.truncation, 'iteration': int(iteration), 'byte_map': BYTE_MAP,
            'layout': '[N*T, C*H*W] uint8: one channel-planar row per frame, clip b at rows b*T .. b*T+T-1'}


def main(argv=None):
    from ..train import gan as train_gan
    from ..util.dir import ensure_exists
    from .samples import save_frames
    from .. import functional_sample as FS
    args = build_parser().parse_args(argv)
    check_args(args)
    held = torch.load(args.weights, map_location='cpu', weights_only=False)
    has_ema = isinstance(held, dict) and 'gen_ema' in held
    del held
    use_ema = has_ema and not args.no_ema
    # the key is loaded only into a run that has an average: any decay will do, no update ever runs here
    args.G_ema = (args.G_ema or 0.999) if use_ema else 0.0
    args.sample_batch_size = args.sample_batch_size or 32
    built = train_gan.construct(args, continue_draws=False)
    gan, device, vocab, ck = built['gan'], built['device'], built['vocab'], built['ck']
    gen = gan.gen
    dset = getattr(built['dataset'], 'dataset', None)
    iteration = int(ck.get('iteration', 0))
    if use_ema:
        which = 'averaged generator (%d updates)' % gan.gen_ema.updates
    else:
        which = 'live weights' + (' (--no_ema)' if has_ema else '')
    status('sampling from the %s' % which)
    N, total, sb = args.sample_n, n_clips(args), int(args.sample_batch_size)
    ensure_exists(args.out_samples)

    # captions and sentence codes, one per latent
    token_lists = resolve_captions(args, gan.cond_encoder is not None, dset, vocab, N)
    captions = None if token_lists is None else [vocab.to_words(t) for t in token_lists]
    codes = None if token_lists is None else encode_captions(gan.cond_encoder, token_lists, device, batch=sb)

    # latents: the tool's generators; the third pair serves --standing_stats alone
    ca = int(getattr(gen, 'ca_dim', 0) or 0)
    g_dev, g_host = generators(args.sample_seed, device)
    z = draw_latents(N, gen.latent_size, g_dev, g_host, args.truncation, device)
    eps = torch.randn(N, ca, generator=g_dev, device=device) if ca else None
    if args.interp is not None:
        S = args.interp
        zh = z.cpu()
        z = torch.cat([slerp(zh[2 * p], zh[2 * p + 1], S) for p in range(N // 2)]).to(device)
        first = [2 * p for p in range(N // 2) for _ in range(S)]           # clip -> its pair's first latent
        if codes is not None:
            codes = take_rows(codes, first)
            captions = [captions[i] for i in first]
        if eps is not None:
            eps = take_rows(eps, first)
    per_file = args.interp if args.interp is not None else sb
    files, gifs = [], []
    mm = pinned = dev_bytes = shape = samples = None
    want_bytes = args.export is not None or args.gif
    with sampling(gan, use_ema):
        if args.standing_stats:
            s_dev, s_host = generators(args.sample_seed + STANDING_SEED, device)

            def batches():
                for k in range(args.standing_stats):
                    zs = draw_latents(sb, gen.latent_size, s_dev, s_host, args.truncation, device)
                    es = torch.randn(sb, ca, generator=s_dev, device=device) if ca else None
                    cs = None
                    if codes is not None:
                        cs = take_rows(codes, [(k * sb + i) % int(codes.shape[0]) for i in range(sb)])
                    yield zs, cs, es
            nb = standing_stats(gan, batches())
            status('standing statistics: %d BatchNorm sites recomputed from %d batches of %d' % (len(batchnorm_sites(gen)), nb, sb))
        for o in range(0, total, per_file):
            k = min(per_file, total - o)
            fake = forward(gan, z[o:o + k], None if codes is None else codes[o:o + k], None if eps is None else eps[o:o + k])[-1]
            if shape is None:
                shape = tuple(int(v) for v in fake.shape[1:])                # (C, T, H, W)
            name = 'sample_%d.png' % len(files)
            save_frames(fake, os.path.join(args.out_samples, name), is_images=getattr(args, 'img_model', False))
            files.append(name)
            if args.nearest:
                if samples is None:
                    samples = torch.empty((total,) + shape, device=device, dtype=torch.float32)
                TF.copy_into(fake, samples[o:o + k])
            if want_bytes:
                C, T, H, W = shape
                if dev_bytes is None:
                    dev_bytes = torch.empty((per_file * T, C * H * W), device=device, dtype=torch.uint8)
                    pinned = torch.empty((per_file * T, C * H * W), dtype=torch.uint8).pin_memory()
                    if args.export is not None:
                        mm = np.lib.format.open_memmap(args.export + '.npy', mode='w+', dtype=np.uint8, shape=(total * T, C * H * W))
                FS.clip_export(fake, out=dev_bytes[:k * T])
                pinned[:k * T].copy_(dev_bytes[:k * T])
                host = pinned[:k * T].numpy()
                if mm is not None:
                    mm[o * T:(o + k) * T] = host
                if args.gif:
                    for i in range(k):
                        gname = 'sample_%d.gif' % (o + i)
                        write_gif(os.path.join(args.out_samples, gname), host[i * T:(i + 1) * T], C, H, W)
                        gifs.append(gname)
    if mm is not None:
        mm.flush()
        del mm
        write_json(args.export + '.json', export_record(args, shape, total, captions, iteration))
        status('exported %d clips to %s.npy' % (total, args.export))

    nearest = None
    if args.nearest:
        if dset is None or len(dset) == 0:
            raise SystemExit('--nearest needs a dataset (--data)')
        d2, idx, seen = nearest_pass(samples, dset, args.nearest, device, limit=args.nearest_clips, batch=min(sb, 32))
        D = int(samples[0].numel())
        nearest = []
        for i in range(total):
            found = [(d, j) for d, j in zip(d2[i], idx[i]) if j >= 0]
            nearest.append([{'index': int(j), 'd2': float(d), 'rms': math.sqrt(float(d) / D)} for d, j in found])
            rows = torch.empty((1 + len(found),) + shape, device=device, dtype=torch.float32)
            TF.copy_into(samples[i:i + 1], rows[0:1])
            with forked_host():
                for k, (_, j) in enumerate(found):
                    TF.copy_into(_real_batch(dset, j, j + 1, device), rows[k + 1:k + 2])
            name = 'nearest_%d.png' % i
            save_frames(rows, os.path.join(args.out_samples, name))
            files.append(name)
        status('nearest real clips: %d neighbours of %d samples among %d dataset items' % (args.nearest, total, seen))

    if captions is not None:
        with open(os.path.join(args.out_samples, CAPTIONS_FILE), 'w') as f:
            f.write(''.join(c + '\n' for c in captions))
    rec = {'iteration': iteration, 'weights': 'gen_ema' if use_ema else 'gen', 'seed': int(args.sample_seed),
           'truncation': args.truncation, 'standing_stats': int(args.standing_stats), 'interp': args.interp, 'clips': int(total),
           'captions': captions, 'files': files + gifs, 'nearest': nearest,
           'export': None if args.export is None else os.path.basename(args.export) + '.npy'}
    write_json(os.path.join(args.out_samples, SAMPLES_FILE), rec)
    return rec


if __name__ == '__main__':
    main()
