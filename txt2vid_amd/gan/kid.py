"""Kernel Inception Distance of the generator during training (opt-in: `--eval_period N`; Bińkowski et al. 2018; not in
the reference, whose evaluation is by eye).

The estimator is the unbiased MMD² with the cubic polynomial kernel k(u, v) = (alpha·uᵀv + 1)³ between features of M real and M
generated clips, in blocks of S clips (functional_kid.py; fp64 on the matrix pipe): `kid` is the mean over the M / S blocks,
`stderr` the standard error of that mean (None for one block). Features are the spatially summed activations [b, 1024] of a
`Resnet3D` trunk that is NOT the trained discriminator: by default a randomly initialised one — the project's own `init()` under
a seed that is a constant of this file, so numbers compare across runs — or, with `--eval_net PATH`, the discriminator trunk of a
checkpoint. Numbers compare only under the same feature network.

`--eval_prdc K` adds improved precision/recall (Kynkäänniemi et al. 2019) and density/coverage (Naeem et al. 2020) on
the same two banks with K nearest neighbours (functional_prdc.py; the whole bank, no blocks): fidelity and diversity apart, where
KID is one number. They compare only under the same feature network, K and M.

Isolation: the evaluator owns its network (frozen, eval mode, in no optimiser and no checkpoint), its latents and its draws (a
device generator and a draws object of its own), restores the generator's mode and weights, and reads the host generators'
state back, so a run with the flag computes bit for bit what it computes without it.

    python -m txt2vid_amd.gan.kid --weights CKPT --data SPEC [the model flags of train.gan]

evaluates a finished run: the models are built as `train.gan` builds them, the real bank is filled from the loader — under the
run's --seed and flags with the clips the run's first iterations saw — and one JSON line is printed (with `--eval_prdc K`, the
extended record)."""
import contextlib
import json
import math
import os

import torch

from .. import functional as TF
from ..draws import HostDraws
from ..functional_kid import kid_sums_raw, estimate
from .. import functional_prdc as FP
from ..util.log import status

FEATURE_SEED = 20181                  # the random feature network's seed: a constant of the code, never the run's --seed
LATENT_SEED = 20182                   # the M latents (and conditioning-augmentation eps) of every evaluation
FEATURE_INIT = 'xavier'
HEAD_KEYS = ('fc_uncond.', 'fc.', 'proj.', 'mbstd.', 'match.')
METRICS_FILE = 'metrics.jsonl'


def add_flags(parser):
    parser.add_argument('--eval_period', type=int, default=0, metavar='N',
                        help='(new) every N iterations, the Kernel Inception Distance between --eval_clips real and generated '
                             'clips on features of a fixed Resnet3D trunk, logged and appended to <out>/metrics.jsonl; 0 = off')
    parser.add_argument('--eval_clips', type=int, default=2048, metavar='M',
                        help='(new) clips per side of --eval_period: the first M real clips of the run, M fixed latents')
    parser.add_argument('--eval_block', type=int, default=None, metavar='S',
                        help='(new) block size of the estimate (default min(M, 1024)); M / S blocks give the standard error')
    parser.add_argument('--eval_net', type=str, default=None, metavar='PATH',
                        help="(new) take the feature network of --eval_period from this checkpoint's discriminator trunk instead "
                             'of the fixed random initialisation')
    parser.add_argument('--eval_prdc', type=int, default=0, metavar='K',
                        help='(new) with --eval_period, also precision/recall and density/coverage of the same features with K '
                             'nearest neighbours, 1..16 (5: Naeem et al. 2020; 3: Kynkäänniemi et al. 2019); 0 = off')
    return parser


def check_args(args, world=1, epoch_clips=None):
    """The flags' rules, before a process group forms. `epoch_clips`: a callable that returns the clips the writer rank sees in
    one epoch (called only with the feature on)."""
    period = getattr(args, 'eval_period', 0) or 0
    if period < 0:
        raise ValueError('--eval_period takes a number of iterations >= 0 (0 = off), got %d' % period)
    K = getattr(args, 'eval_prdc', 0) or 0
    if K < 0 or K > FP.MAX_K:
        raise ValueError('--eval_prdc takes a number of neighbours from 1 to %d (0 = off), got %d' % (FP.MAX_K, K))
    if K > 0 and period == 0:
        raise ValueError('--eval_prdc %d needs --eval_period: the metrics are computed on the banks of that evaluation' % K)
    if period == 0:
        return
    M = args.eval_clips
    S = args.eval_block if args.eval_block is not None else min(M, 1024)
    if M < 2 or S < 2:
        raise ValueError('--eval_clips and --eval_block take at least 2 clips, got %d and %d' % (M, S))
    if M % S:
        raise ValueError('--eval_clips must be a multiple of --eval_block (whole blocks), got %d and %d' % (M, S))
    if getattr(args, 'end2end', False):
        raise ValueError('--eval_period cannot run with --end2end: the sentence codes of the real bank would come from a text '
                         'encoder that has moved on since')
    if args.eval_net is not None and not os.path.exists(args.eval_net):
        raise ValueError('--eval_net %s: no such file' % args.eval_net)
    if K >= M:
        raise ValueError('--eval_prdc %d needs more than %d clips (--eval_clips): a clip has M - 1 neighbours' % (K, M))
    args.eval_block = S
    if epoch_clips is not None:
        have = int(epoch_clips())
        if M > have:
            raise ValueError('--eval_clips %d exceeds the %d clips of an epoch: the real bank would hold duplicates, which bias '
                             'the estimate' % (M, have))


def _trunk_state(path):
    """The trunk's tensors of the first discriminator entry of a checkpoint (project or reference layout; `single_discrim.*`,
    `single_discrim.module.*` and `sub_discrims.N.*` key styles), head keys dropped."""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    for name, sd in ck.items():
        if not isinstance(sd, dict) or name in ('gen', 'gen_ema', 'cond', 'optD', 'optG'):
            continue
        keys = [k for k in sd if isinstance(k, str)]
        for pre in ('single_discrim.module.', 'single_discrim.', 'sub_discrims.%d.module.' % 0, 'sub_discrims.%d.' % 0):
            if any(k.startswith(pre) for k in keys):
                out = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
                return name, {k: v for k, v in out.items() if not k.startswith(HEAD_KEYS)}
    raise ValueError('--eval_net %s holds no discriminator entry (single_discrim.* or sub_discrims.* keys)' % path)


def feature_network(num_channels, device, path=None):
    """(network, name): a plain Resnet3D in eval mode with frozen parameters. No draw of the caller's generators moves."""
    from ..models.resnet3d import Resnet3D
    from ..util.torch.init import init
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(FEATURE_SEED)
        net = Resnet3D(num_channels=num_channels)
        init(net, init_method=FEATURE_INIT)
    name = 'random-init Resnet3D (%s, seed %d)' % (FEATURE_INIT, FEATURE_SEED)
    if path is not None:
        entry, sd = _trunk_state(path)
        own = net.state_dict()
        want = [k for k in own if not k.startswith(HEAD_KEYS)]
        missing = [k for k in want if k not in sd]
        wrong = [k for k in want if k in sd and tuple(sd[k].shape) != tuple(own[k].shape)]
        if missing or wrong:
            raise ValueError('--eval_net %s (entry %r) does not fit Resnet3D(num_channels=%d): missing %s, other shapes %s'
                             % (path, entry, num_channels, missing[:3], wrong[:3]))
        own.update({k: sd[k].detach().to(torch.float32) for k in want})
        net.load_state_dict(own)
        name = "trunk of %r in %s" % (entry, os.path.basename(path))
    net.to(device).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net, name


class _EvalDraws(HostDraws):
    """The draws of an evaluation forward: the conditioning augmentation's eps comes from the evaluator's fixed bank; an
    eval-mode generator asks for nothing else."""

    def __init__(self, eps):
        self.eps, self.at = eps, 0

    def ca_eps(self, b, d, device):
        out = self.eps[self.at:self.at + b]
        self.at += b
        if out.shape != (b, d):
            raise RuntimeError('the evaluation drew %s conditioning-augmentation eps where %s were banked' % ((b, d), tuple(out.shape)))
        return out

    def _refuse(self, *a, **k):
        raise RuntimeError('an evaluation forward asked for a training draw')
    multiscale_t0 = phase = z = alpha = aug = perm = _refuse


class KidEvaluator(object):
    """gan.kid (None by default). `observe(x, cond)` banks the features of the first M real clips; `evaluate(iteration)` renders
    M clips from fixed latents and returns the record; `due(iteration)` says when."""

    def __init__(self, gan, device, clips=2048, block=None, num_channels=1, seed=LATENT_SEED, period=1, sample_batch=None,
                 net=None, out_dir=None, prdc=0):
        block = min(clips, 1024) if block is None else block
        if clips < 2 or block < 2 or clips % block:
            raise ValueError('KID takes M >= 2 clips in whole blocks of S >= 2, got M = %d, S = %d' % (clips, block))
        self.gan, self.device, self.M, self.S, self.period = gan, torch.device(device), int(clips), int(block), int(period)
        self.sample_batch, self.out_dir = sample_batch, out_dir
        self.net, self.net_name = feature_network(num_channels, device, net)
        self.dim = self.net.fc_uncond.weight.shape[1]
        self.real_bank = torch.zeros(self.M, self.dim, device=device)
        self.fake_bank = torch.zeros(self.M, self.dim, device=device)
        self.cond_bank = None                                   # [M, cond_dim] once the first text-conditioned batch arrives
        self.filled, self.alpha = 0, None
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed))
        gen = gan.gen
        self.z = torch.randn(self.M, gen.latent_size, generator=g, device=self.device)
        ca = int(getattr(gen, 'ca_dim', 0) or 0)
        self.eps = torch.randn(self.M, ca, generator=g, device=self.device) if ca else None
        self.sums = torch.zeros(self.M // self.S, 3, device=device, dtype=torch.float64)
        need = int(TF.lib().t2v_kid_sums_ws_bytes(self.M, self.dim, self.S))
        self.ws = torch.zeros(need // 8 + 1, device=device, dtype=torch.float64).view(torch.uint8)
        self.prdc = int(prdc or 0)                              # --eval_prdc K: neighbours of precision/recall/density/coverage, 0 = off
        if self.prdc:
            FP.check_sizes(self.M, self.dim, self.prdc)
            L = TF.lib()
            need = max(int(L.t2v_knn_radii_ws_bytes(self.M, self.dim, self.prdc)), int(L.t2v_prdc_counts_ws_bytes(self.M, self.dim, self.prdc)))
            if need < 1:
                raise ValueError('PRDC: no launch plan for M = %d, k = %d' % (self.M, self.prdc))
            self.prdc_ws = torch.zeros(need // 8 + 1, device=device, dtype=torch.float64).view(torch.uint8)
            self.rX = torch.zeros(self.M, device=device, dtype=torch.float64)       # squared radii of the real bank: once, when it fills
            self.rY = torch.zeros(self.M, device=device, dtype=torch.float64)
            self.counts = torch.zeros(4, device=device, dtype=torch.int64)
        self.last = None
        self._waiting_logged = False

    # ---- features ------------------------------------------------------------------------------------------------------------
    def features(self, x):
        """[b, C, T, S, S] -> [b, 1024]: the trunk's spatially summed activations, a group of one through the existing kernels."""
        with torch.no_grad():
            return self.net(x.detach())[2]

    @property
    def full(self):
        return self.filled >= self.M

    def observe(self, x, cond=None):
        """Bank the features (and sentence codes) of this iteration's real clips until M are held. x: the full-resolution batch
        the loop already has on the device, before any augmentation."""
        if self.full:
            return
        k = min(int(x.shape[0]), self.M - self.filled)
        x = x[:k]
        f = self.features(x if x.is_contiguous() else x.contiguous())
        TF.copy_into(f, self.real_bank[self.filled:self.filled + k])
        if cond is not None:
            if self.cond_bank is None:
                self.cond_bank = torch.zeros(self.M, cond.shape[1], device=self.device)
            TF.copy_into(cond.detach()[:k].contiguous(), self.cond_bank[self.filled:self.filled + k])
        self.filled += k
        if self.full:
            with torch.no_grad():
                sq = TF.row_sqnorm(self.real_bank)                                    # t2v_row_sqnorm
            mean = sum(float(v) for v in sq.tolist()) / self.M
            if not mean > 0 or not math.isfinite(mean):
                raise RuntimeError('KID: the real features have mean squared norm %r' % mean)
            self.alpha = 1.0 / mean
            if self.prdc:
                FP.knn_radii_raw(self.real_bank, self.prdc, out=self.rX, ws=self.prdc_ws)

    def due(self, iteration):
        return self.period > 0 and iteration % self.period == 0

    # ---- evaluation ----------------------------------------------------------------------------------------------------------
    def _render(self):
        gan, gen = self.gan, self.gan.gen
        ema = getattr(gan, 'gen_ema', None)
        sb = int(self.sample_batch or 32)
        was_training = gen.training
        old_draws = TF.draws
        host = torch.get_rng_state()
        gen.eval()
        draws = _EvalDraws(self.eps)
        TF.set_draws(draws)
        try:
            with torch.no_grad(), (ema.swapped() if ema is not None else contextlib.nullcontext()):
                if ema is None:
                    # the packed copies of the weights are refreshed inside the replayed graph for the variants the training step
                    # uses; an eval-mode forward may read others: refresh them all (a table of its own, like the average's swap)
                    TF.repack_params([p for p in gen.parameters()][::-1])
                for o in range(0, self.M, sb):
                    k = min(sb, self.M - o)
                    c = None if self.cond_bank is None else self.cond_bank[o:o + k]
                    fake = gan(self.z[o:o + k], cond=c)[-1]
                    TF.copy_into(self.features(fake), self.fake_bank[o:o + k])
        finally:
            TF.set_draws(old_draws)
            gen.train(was_training)
            torch.set_rng_state(host)

    def evaluate(self, iteration):
        """One evaluation from the fixed latents; returns the record that goes to the log and to metrics.jsonl."""
        if not self.full:
            raise RuntimeError('KID: the real bank holds %d of %d clips' % (self.filled, self.M))
        self._render()
        kid_sums_raw(self.real_bank, self.fake_bank, self.S, self.alpha, out=self.sums, ws=self.ws)
        if self.prdc:
            FP.knn_radii_raw(self.fake_bank, self.prdc, out=self.rY, ws=self.prdc_ws)
            FP.prdc_counts_raw(self.real_bank, self.fake_bank, self.prdc, self.rX, self.rY, out=self.counts, ws=self.prdc_ws)
        kid, stderr, _ = estimate(self.sums.tolist(), self.S)
        self.last = {'iteration': int(iteration), 'kid': kid, 'stderr': stderr, 'clips': self.M, 'block': self.S,
                     'alpha': self.alpha, 'net': self.net_name}
        if self.prdc:
            p, r, d, c = FP.estimate(self.counts.tolist(), self.M, self.prdc)
            self.last.update({'precision': p, 'recall': r, 'density': d, 'coverage': c, 'prdc_k': self.prdc})
        return self.last

    def log_line(self, rec):
        pm = '' if rec['stderr'] is None else ' ± %.5f' % rec['stderr']
        return 'Iter %d, KID: %.5f%s (%d clips in blocks of %d; features: %s)' % (rec['iteration'], rec['kid'], pm, rec['clips'],
                                                                                   rec['block'], rec['net'])

    def prdc_line(self, rec):
        return 'Iter %d, PRDC (k=%d): precision %.3f, recall %.3f, density %.3f, coverage %.3f' % (
            rec['iteration'], rec['prdc_k'], rec['precision'], rec['recall'], rec['density'], rec['coverage'])

    def step(self, iteration):
        """What train() calls behind an iteration: evaluate, log and append to <out>/metrics.jsonl when one is due."""
        if not self.due(iteration):
            return None
        if not self.full:
            if not self._waiting_logged:
                status('Iter %d, KID: waiting for the real bank (%d of %d clips)' % (iteration, self.filled, self.M))
                self._waiting_logged = True
            return None
        rec = self.evaluate(iteration)
        status(self.log_line(rec))
        if self.prdc:
            status(self.prdc_line(rec))
        if self.out_dir is not None:
            with open(os.path.join(self.out_dir, METRICS_FILE), 'a') as f:
                f.write(json.dumps(rec) + '\n')
        return rec


def from_args(gan, args, device):
    """The evaluator of a run (main(): behind sync_replicas, in front of set_rng_state), announced in the log."""
    ev = KidEvaluator(gan, device, clips=args.eval_clips, block=args.eval_block, num_channels=args.num_channels,
                      period=args.eval_period, sample_batch=args.sample_batch_size or args.batch_size, net=args.eval_net,
                      out_dir=args.out, prdc=getattr(args, 'eval_prdc', 0))
    status('KID evaluation every %d iterations: %d clips in blocks of %d; features: %s. Numbers compare only under the same '
           'feature network' % (ev.period, ev.M, ev.S, ev.net_name))
    if ev.prdc:
        status('with precision/recall and density/coverage on the same features, k = %d nearest neighbours among all %d clips'
               % (ev.prdc, ev.M))
    return ev


def main(argv=None):
    """Stand-alone evaluation of a checkpoint: `train.gan`'s construction, the real bank from the loader, one JSON line."""
    from ..data import DevicePrefetcher
    from ..train import gan as train_gan
    args = train_gan.build_parser().parse_args(argv)
    if args.weights is None:
        raise SystemExit('txt2vid_amd.gan.kid evaluates a checkpoint: pass --weights')
    args.eval_period = args.eval_period or 1
    # the real bank of a run is its first M clips: the loader has to start where the run's did, not where the checkpoint's draw
    # sequence goes on. Under the run's --seed and flags the record of a checkpoint is then the one the run logged at that iteration
    built = train_gan.construct(args, continue_draws=False)
    gan, device, ev = built['gan'], built['device'], built['gan'].kid
    pre = DevicePrefetcher(built['dataset'], device)
    x, y = pre.next()
    while x is not None and not ev.full:
        x = TF.video_to_channel_first(x)
        cond = None
        if gan.cond_encoder is not None and len(y) >= 2:
            with torch.no_grad():
                _, _, cond = gan.cond_encoder.encode(y[0], y[1])
        ev.observe(x, cond)
        x, y = pre.next()
    rec = ev.evaluate(int(built['ck'].get('iteration', 0)))
    status(ev.log_line(rec))
    if ev.prdc:
        status(ev.prdc_line(rec))
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == '__main__':
    main()
