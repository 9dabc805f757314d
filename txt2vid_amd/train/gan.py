"""CLI entry of the TGANv2 hot path — flag-for-flag txt2vid/train/gan.py:28-221 (+ trainer.py:15-42), so
`scripts/run_tganv2*.sh` / `config/*.json` drive this build. One process per GPU: launched under
`torch.distributed.run` it trains data-parallel over RCCL (the reference's `--ngpu` was never read).
The opt-in features are built in `main()` in a load-bearing order, from the flags and the checkpoint's extra keys.

    python -m txt2vid_amd.train.gan --data config/synth.json --G txt2vid.models.tganv2.gen.MultiScaleGen ...
"""
import argparse
import os

import torch

from .. import data
from ..gan.cond_gan import CondGan
from ..gan.losses import MixedGanLoss
from ..gan.trainer import add_params_to_parser, train, test
from ..optim import Adam, SGD
from ..util.log import status
from ..util.pick import load
from ..util.reflection import create_object
from ..util.torch.init import init
from .setup import setup, set_rng_state


def _model(spec, args, kind='D', **kw):
    """`create_object(spec, cond_dim=...)` like the reference; convenience: a bare class name also gets
    `num_channels=--num_channels`, and a bare generator class `width = height = --frame_sizes[-1]` (the reference needs a
    JSON spec for anything but its 3-channel / 128x128 defaults)."""
    if isinstance(spec, str) and not os.path.exists(spec):
        kw.setdefault('num_channels', args.num_channels)
        if kind == 'G':                       # the reference's default generator is 128x128 whatever --frame_sizes says
            kw.setdefault('width', args.frame_sizes[-1])
            kw.setdefault('height', args.frame_sizes[-1])
    return create_object(spec, **kw)


def _dataset(args, vocab, rank):
    transform = data.default_transform(frame_size=[args.frame_sizes[-1]], num_channels=args.num_channels)
    return create_object(args.data, vocab=vocab, anno=args.anno, transform=transform, size=args.frame_sizes[-1],
                         channels=args.num_channels, seed=(args.seed or 0) + rank)


def _epoch_clips(args, world):
    """Clips the writer rank sees in one epoch (whole batches), from a dataset object built for the count alone; the host
    generators are left as they were."""
    import random
    import numpy as np
    state = (random.getstate(), np.random.get_state())
    try:
        with torch.random.fork_rng(devices=[]):
            dset = _dataset(args, load(args.vocab) if args.vocab else data.Vocab(), 0)
    finally:
        random.setstate(state[0])
        np.random.set_state(state[1])
    per_rank = len(dset) if isinstance(dset, data.SyntheticMovingDigits) else len(dset) // world
    return per_rank // args.batch_size * args.batch_size


def construct(args, continue_draws=True):
    """Everything `main` builds in front of the loop, as a dict (gan, optD, optG, losses, dataset, device, vocab, grad_sync, ck):
    the stand-alone evaluation (gan/kid.py) builds its models through here too — with `continue_draws=False`, which leaves the
    host generators where a fresh run under --seed has them instead of continuing the checkpoint's draw sequence, so that its
    loader yields the clips the run's first iterations saw."""
    from ..gan import ada, grad_guard, kid, lecam, lr_sched, match
    from ..gan.ema import GenAverage
    from ..gan.spectral import check_flags, check_checkpoint, SpectralNorm, attach
    # the flags' rules are checked before a process group forms (a data-parallel start with --D_ada is refused here)
    check_flags(args)
    ada.check_args(args, world=int(os.environ.get('WORLD_SIZE', '1')))
    lecam.check_args(args, world=int(os.environ.get('WORLD_SIZE', '1')))
    match.check_args(args, world=int(os.environ.get('WORLD_SIZE', '1')))
    lr_sched.check_args(args)
    grad_guard.check_args(args)
    kid.check_args(args, world=int(os.environ.get('WORLD_SIZE', '1')),
                   epoch_clips=lambda: _epoch_clips(args, int(os.environ.get('WORLD_SIZE', '1'))))
    from .. import dist as tdist
    rank, world = tdist.init_from_env('nccl')
    from ..util.misc import limit_host_threads
    limit_host_threads()                 # an oversubscribed CPU thread pool starves the HIP runtime's submission thread
    if world > 1 and args.seed is None:
        import random
        args.seed = tdist.broadcast_seed(random.randint(1, 100000))      # one seed for all ranks: identical replicas
    seed, device = setup(args)
    status('%d cuda devices available; rank %d of %d' % (torch.cuda.device_count(), rank, world))
    vocab = load(args.vocab) if args.vocab else data.Vocab()
    txt_encoder = None
    if not args.dont_use_sent:
        if args.sent_weights:
            from ..util.reflection import alias_reference_modules
            alias_reference_modules()            # the reference pickles the whole Seq2Seq object under its own module path
            txt_encoder = torch.load(args.sent_weights, weights_only=False, map_location='cpu')
            if isinstance(txt_encoder, dict) and 'txt' in txt_encoder:
                txt_encoder = txt_encoder['txt']
            txt_encoder = txt_encoder.to(device)
            if hasattr(txt_encoder, 'differentiable'):
                txt_encoder.differentiable(False)      # a pre-training checkpoint may carry the autograd-path flag: the GAN loop
                #                                        detaches the sentence code (trainer.py:211-215), forward-only kernels
        else:
            txt_encoder = create_object(args.sent, vocab_size=len(vocab)).to(device)
            init(txt_encoder, init_method=args.sent_init_method or args.init_method)
    cond_dim = txt_encoder.encoder.encoding_size if txt_encoder is not None else 0
    gen = _model(args.G, args, kind='G', cond_dim=cond_dim)
    discrims = [_model(d, args, cond_dim=cond_dim) for d in args.D]
    # (the flags need the matching head of the --D spec; a training run refuses a head without flags in main())
    match.check_discrims(args, discrims, training=False)
    init(gen, init_method=args.init_method)
    for d in discrims:
        init(d, init_method=args.init_method)
    gen.to(device)
    discrims = [d.to(device) for d in discrims]
    if args.M:
        raise NotImplementedError('--M sample mappings (TCWYT baseline) are outside the hot path')
    D_params = [{'params': d.parameters()} for d in discrims]
    G_params = [{'params': gen.parameters()}]
    if args.end2end and txt_encoder is not None:
        # train/gan.py:82-85: the text encoder trains with the GAN — its parameters join BOTH optimisers, the sentence code keeps
        # its graph (trainer.py:213-214), the D backward retains it (trainer.py:240) and the G backward runs through it again after
        # optD.step() has moved the encoder. That sequence only runs where the optimiser's in-place update does not bump autograd's
        # version counters: the reference's pinned torch 0.4.1 (updates through `.data`) — and here, where Adam is a kernel
        # writing through raw pointers. Stock torch >= 1.x raises "modified by an inplace operation" on the G backward.
        # Eager launches (the encoder graph spans the D and the G step: no graph replay), no gradient sink.
        D_params.append({'params': txt_encoder.parameters()})
        G_params.append({'params': txt_encoder.parameters()})
        txt_encoder.differentiable(True)
    if args.sgd:                                   # train/gan.py:86-89: momentum = beta1
        status('Using SGD')
        optD = SGD(D_params, lr=args.D_lr, momentum=args.D_beta1)
        optG = SGD(G_params, lr=args.G_lr, momentum=args.G_beta1)
    else:
        optD = Adam(D_params, lr=args.D_lr, betas=(args.D_beta1, args.D_beta2))
        optG = Adam(G_params, lr=args.G_lr, betas=(args.G_beta1, args.G_beta2))
    ck = {}      # the checkpoint's entries outside the reference's layout, for the opt-in features below (their order: DESIGN §22)
    gan = CondGan(gen=gen, discrims=discrims, cond_encoder=txt_encoder, discrim_names=args.D_names,
                  discrim_lambdas=args.D_lambdas, gp_scale=float(world))
    if args.D_ada is not None:
        # (in front of load_from_dict, which loads its state: a file without the key 'ada' starts from --D_aug_p)
        gan.ada = ada.AdaState(args.D_ada, args.D_ada_interval, args.D_ada_kclips, args.D_aug_p, device)
        status('Adaptive augmentation strength: target %g, update every %d D steps, %g kclips, initial p %g (defaults are the '
               "paper's values for images, untuned for video)" % (args.D_ada, args.D_ada_interval, args.D_ada_kclips, args.D_aug_p))
    if args.D_lecam is not None:
        # (likewise in front of load_from_dict: a file without the key 'lecam' starts with no anchors)
        gan.lecam = lecam.LeCamState(args.D_lecam, args.D_lecam_decay, args.D_lecam_start, device)
        status('LeCam regularisation of the discriminator: weight %g, anchor decay %g, from D step %d (0.3 is the paper\'s value for '
               'images, untuned for video)' % (args.D_lecam, args.D_lecam_decay, args.D_lecam_start))
    if match.enabled(args):
        # (no state beyond the head's W, which is a parameter of the discriminator)
        gan.match = match.MatchState(args.D_match, args.G_match, args.match_tau, device)
        status('Clip-caption matching term: D weight %s, G weight %s, temperature %g (XMC-GAN\'s values for images, untuned for '
               'video)' % (args.D_match, args.G_match, args.match_tau))
    if args.weights is not None:
        to_load = torch.load(args.weights, map_location=device, weights_only=False)
        check_checkpoint(to_load, args.D_sn, args.weights)
        gan.load_from_dict(to_load)
        if 'optD' in to_load:
            optD.load_state_dict(to_load['optD'])
        if 'optG' in to_load:
            optG.load_state_dict(to_load['optG'])
        ck = {k: v for k, v in to_load.items() if k in ('rng_state', 'iteration', 'gen_ema_updates', 'discrim_sn', 'lr_sched',
                                                         'grad_guard') or (k == 'gen_ema' and args.G_ema > 0)}
        del to_load
    if gan.ada is not None:
        st = gan.ada.ada.tolist()
        status('Augmentation probability p = %r; window: sign sum %g over %g pairs in %g D steps' % (st[0], st[1], st[2], st[3]))
    if gan.lecam is not None:
        st = gan.lecam.lecam.tolist()
        n_lv = int(st[3])
        status('LeCam state: %d D steps seen, last R %r (gate %d); anchors real %r, fake %r' % (
            int(st[0]), st[1], int(st[2]), st[lecam.A_R:lecam.A_R + n_lv], st[lecam.A_F:lecam.A_F + n_lv]))
    if args.lr_decay != 'none':
        # (behind the optimisers' own state. Every rank ticks identical state: no exchange)
        sched = lr_sched.LrSchedule(args.lr_decay, args.lr_decay_iters, args.lr_decay_start, args.lr_final, args.discrim_steps,
                                    args.gen_steps, device).attach(optD, optG)
        for note in sched.load_state_dict(ck.get('lr_sched'), int(ck.get('iteration', 0))):
            status('Learning-rate schedule: ' + note)
        k = sched.counters()
        status('Learning-rate schedule: %s from iteration %d to %d, final fraction %g; D at update %d, G at update %d' % (
            args.lr_decay, args.lr_decay_start, args.lr_decay_iters, args.lr_final, k['D'], k['G']))
    elif 'lr_sched' in ck:
        status('the checkpoint holds a learning-rate schedule state (%s); without --lr_decay it is ignored' % (ck['lr_sched'],))
    if grad_guard.enabled(args):
        # (likewise. Every rank sees the same gradients and takes the same decision: no exchange)
        guard = grad_guard.GradGuard(args.D_clip, args.G_clip, device).attach(optD, optG)
        if args.weights is not None:
            for note in guard.load_state_dict(ck.get('grad_guard')):
                status('Gradient guard: ' + note)
        k = guard.counters()
        status('Gradient guard: D clip %s, G clip %s, non-finite steps are skipped; D %d steps (%d skipped, %d clipped), '
               'G %d steps (%d skipped, %d clipped) so far' % (
                   'off' if args.D_clip is None else '%g' % args.D_clip, 'off' if args.G_clip is None else '%g' % args.G_clip,
                   k['D']['steps'], k['D']['skipped'], k['D']['clipped'], k['G']['steps'], k['G']['skipped'], k['G']['clipped']))
    elif 'grad_guard' in ck:
        status('the checkpoint holds gradient-guard counts (%s); without --grad_guard / --D_clip / --G_clip the key is ignored'
               % (ck['grad_guard'],))
    if world > 1:
        # replicas bit-identical before the first step, then per-rank generators for everything drawn per iteration
        from .. import functional as TF
        tdist.sync_replicas([gen] + list(discrims) + [txt_encoder])
        TF.bump_weight_epoch()
        import random
        import numpy as np
        for seeder in (random.seed, np.random.seed, torch.manual_seed):
            seeder(seed + rank + 1000003 * int(ck.get('iteration', 0)))     # (a resumed run does not replay the first run's draws)
    if args.G_ema > 0:
        # (from the loaded / initialised and synchronised weights, identical on every rank: no exchange)
        gan.gen_ema = GenAverage(gen, args.G_ema, start=args.G_ema_start)
        if 'gen_ema' in ck:
            gan.gen_ema.load_state_dict(ck['gen_ema'], ck.get('gen_ema_updates', 0))
        status('Averaged generator: decay %g after %d updates (%d updates so far)' % (args.G_ema, args.G_ema_start,
                                                                                     gan.gen_ema.updates))
    if args.D_sn:
        # (likewise. A checkpoint with its state continues bit for bit; u comes from a generator of its own)
        attach(gan, optD, SpectralNorm(discrims, seed=seed, state=ck.get('discrim_sn')))
        status('Spectral normalisation of %d discriminator weights (%s)' % (
            len(gan.discrim_sn.params), 'state from the checkpoint' if 'discrim_sn' in ck else '%d initial power iterations'
            % gan.discrim_sn.n_init))
    if getattr(args, 'eval_period', 0) > 0 and rank == 0:
        # (the writer alone. Its feature network is initialised under a seed of its own with the host generators
        # forked, its latents come from a device generator of its own: no draw of the training loop moves)
        gan.kid = kid.from_args(gan, args, device)
    if ck.get('rng_state') is not None and rank == 0 and continue_draws:
        # the writer's (rank 0's) generator states: the run continues the saved draw sequence (reference files have no such key)
        set_rng_state(ck['rng_state'])
    dset = _dataset(args, vocab, rank)
    dataset = data.get_loader(dset=dset, batch_size=args.batch_size, val=False, num_workers=args.workers, rank=rank,
                              world=world, seed=seed, device=device)
    status('GAN has %d parameters' % gan.count_params())
    if args.G_loss is None:
        args.G_loss = args.D_loss
    losses = MixedGanLoss(g_loss=create_object(args.G_loss), d_loss=create_object(args.D_loss))
    grad_sync = None
    if world > 1:
        from .. import functional as TF
        # --end2end: the text encoder sits in BOTH optimisers (train/gan.py:82-85), so its gradients travel with both exchanges
        shared = [txt_encoder] if (args.end2end and txt_encoder is not None) else []
        arenas = {'D': tdist.model_arena(list(discrims) + shared, TF.copy_into), 'G': tdist.model_arena([gen] + shared, TF.copy_into)}
        grad_sync = tdist.make_grad_sync(arenas, {'D': optD, 'G': optG}, world)
    return {'gan': gan, 'optD': optD, 'optG': optG, 'losses': losses, 'dataset': dataset, 'device': device, 'vocab': vocab,
            'grad_sync': grad_sync, 'ck': ck}


def main(args):
    c = construct(args)
    gan, optD, optG, losses, dataset, device, vocab, grad_sync = (c[k] for k in ('gan', 'optD', 'optG', 'losses', 'dataset', 'device',
                                                                                 'vocab', 'grad_sync'))
    if not args.test:
        from ..gan import match
        match.check_discrims(args, gan.discrims)          # a matching head that no flag trains is refused before the loop
    if args.test:
        test(gan=gan, num_samples=args.num_samples, dataset=dataset, device=device, params=args,
             channel_first=not args.sequence_first, vocab=vocab)
    else:
        train(gan=gan, num_epoch=args.epochs, dataset=dataset, device=device, optD=optD, optG=optG, params=args,
              losses=losses, vocab=vocab, channel_first=not args.sequence_first, end2end=args.end2end,
              grad_sync=grad_sync, max_iters=args.max_iters)


# txt2vid/train/gan.py:163-221 — same flags, types and defaults; `max_iters` is new (stop after that many iterations)
FLAGS = """
test flag
num_samples int 1
seed int -
cuda flag
workers int 2
ngpu int 1
frame_sizes ints 64
num_channels int 1
random_frames int 0
opt_level str O2
epochs int 5
batch_size int 64
init_method str xavier
G_loss str -
G_lr float 0.0001
G_beta1 float 0.5
G_beta2 float 0.9
D_loss str txt2vid.gan.losses.VanillaGanLoss
D_lr float 0.0001
D_beta1 float 0.5
D_beta2 float 0.9
weights str -
sent_weights str -
data str - !
anno str -
vocab str -
M str -
G str - !
D strs - !
D_names strs -
D_lambdas floats -
sent str -
sent_init_method str -
dont_use_sent flag
end2end flag
sgd flag
sequence_first flag
debug flag
max_iters int -
"""


def build_parser():
    from ..util.cli import add_flags
    p = argparse.ArgumentParser()
    add_params_to_parser(p)
    return add_flags(p, FLAGS)


if __name__ == '__main__':
    main(build_parser().parse_args())
