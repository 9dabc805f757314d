"""GPU: every opt-in training feature at once through the command line — the order of their log lines, the checkpoint's key set
and a resumed run that continues every count (each feature's own round trip lives in its test_*_gpu.py)."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_KEYS = {'gen_ema', 'gen_ema_updates', 'discrim_sn', 'ada', 'lr_sched', 'grad_guard', 'iteration', 'rng_state', 'optD', 'optG'}


def test_all_extras_cli(tmp_path):
    cfg = str(tmp_path / 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    base = ['--data', cfg, '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
            '--G_lr', '0.0002', '--D_lr', '0.0004', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
            '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1', '--save_example_period', '0',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--epochs', '1',
            '--G_ema', '0.9', '--D_aug', 'color,translation', '--D_ada', '0.6', '--D_sn', '--lr_decay', 'linear',
            '--lr_decay_iters', '100', '--D_clip', '1e-3']

    def run(args):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + base + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert p.returncode == 0, out[-3000:]
        return out

    def block(log, i):
        """The positions of iteration i's lines: Loss_D, p, learning rates, gradient guard (None where a line is missing)."""
        marks = ('Iter %d, Loss_D' % i, 'Iter %d, augmentation probability p (--D_ada, target 0.6)' % i,
                 'Iter %d, learning rates (--lr_decay linear' % i, 'Iter %d, gradient guard: norm D' % i)
        assert all(log.count(m) <= 1 for m in marks), log[-3000:]
        return [log.find(m) if m in log else None for m in marks]
    out1 = str(tmp_path / 'out1')
    log = run(['--out', out1, '--out_samples', str(tmp_path / 's1'), '--max_iters', '4', '--save_model_period', '4'])
    # under replay p and the guard's state travel with the losses, one iteration late: iteration 1 has neither line yet
    first = block(log, 1)
    assert first[0] is not None and first[1] is None and first[2] is not None and first[3] is None, log[-3000:]
    for i in (2, 3, 4):
        at = block(log, i)
        assert None not in at and at == sorted(at), (i, at, log[-3000:])
    assert block(log, 4)[0] > block(log, 3)[3] > block(log, 3)[0] > block(log, 2)[3]
    ck = glob.glob(os.path.join(out1, 'iter_4_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    reference = set(torch.load(os.path.join(GOLDEN, 'ref_checkpoint_uncond.pt'), weights_only=False, map_location='cpu'))
    assert reference == {'optG', 'optD', 'gen', 'video'} and set(sd) == reference | EXTRA_KEYS, sorted(sd)
    assert sd['iteration'] == 4 and sd['gen_ema_updates'] == 4 and sd['grad_guard']['D']['steps'] == 4
    assert (sd['lr_sched']['D'], sd['lr_sched']['G']) == (4, 4)
    # resumed: every count continues, nothing starts over
    out2 = str(tmp_path / 'out2')
    log = run(['--out', out2, '--out_samples', str(tmp_path / 's2'), '--weights', ck[0], '--max_iters', '2', '--save_model_period', '2'])
    assert 'D 4 steps (0 skipped, 4 clipped), G 4 steps (0 skipped, 0 clipped) so far' in log, log[-3000:]
    assert 'D at update 4, G at update 4' in log and '(4 updates so far)' in log and 'state from the checkpoint' in log
    p = float(re.search(r'Augmentation probability p = ([-0-9.e]+);', log).group(1))
    assert p == sd['ada']['ada'][0].item()
    assert not re.search(r'has no \w+ key', log) and 'initial power iterations' not in log and 'is ignored' not in log
    at = block(log, 2)
    assert None not in at and at == sorted(at)
    assert re.search(r'Iter 2, learning rates \(--lr_decay linear, iteration 6 of the schedule', log)
    assert re.search(r'Iter 2, gradient guard: .* clipped D 5 G 0', log)          # (iteration 1's state: one late)
    ck2 = glob.glob(os.path.join(out2, 'iter_2_lossG_*'))
    assert len(ck2) == 1
    sd2 = torch.load(ck2[0], map_location='cpu', weights_only=False)
    assert set(sd2) == set(sd) and sd2['iteration'] == 2 and sd2['gen_ema_updates'] == 6
    assert sd2['grad_guard']['D'] == {'steps': 6, 'skipped': 0, 'clipped': 6} and sd2['grad_guard']['G']['steps'] == 6
    assert (sd2['lr_sched']['D'], sd2['lr_sched']['G']) == (6, 6)
