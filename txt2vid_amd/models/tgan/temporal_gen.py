"""TGAN-v1 frame-seed generator — same parameters / state_dict as txt2vid/models/tgan/temporal_gen.py:10-34; the five
layers run as one launch each forward and backward (`functional_temporal`, csrc/temporal.hip)."""
import torch.nn as nn

from ... import functional_temporal as TT


class ConvTranspose1d(nn.ConvTranspose1d):
    """Parameters only (creation, init, state_dict): the generator drives its layers through fused kernels."""

    def forward(self, x):
        raise NotImplementedError('ConvTranspose1d runs inside FrameSeedGenerator')


class BatchNorm1d(nn.BatchNorm1d):
    def forward(self, x):
        raise NotImplementedError('BatchNorm1d runs inside FrameSeedGenerator')


class FrameSeedGenerator(nn.Module):
    """z_slow [B, z_slow_dim] -> z_fast [B, z_fast_dim, 16]: 16 frame seeds from one latent (the reference hard-codes 16)."""

    def __init__(self, z_slow_dim, z_fast_dim):
        super().__init__()
        self.z_slow_dim = z_slow_dim
        self.z_fast_dim = z_fast_dim
        # registration order = the reference's (its default-init draws and state_dict order)
        self.dc0 = ConvTranspose1d(z_slow_dim, 512, 1, 1, 0)
        self.dc1 = ConvTranspose1d(512, 256, 4, 2, 1)
        self.dc2 = ConvTranspose1d(256, 128, 4, 2, 1)
        self.dc3 = ConvTranspose1d(128, 128, 4, 2, 1)
        self.dc4 = ConvTranspose1d(128, z_fast_dim, 4, 2, 1)
        self.bn0 = BatchNorm1d(512)
        self.bn1 = BatchNorm1d(256)
        self.bn2 = BatchNorm1d(128)
        self.bn3 = BatchNorm1d(128)

    def forward(self, z_slow):
        B = z_slow.size(0)
        if self.training and B == 1:
            # what the reference's bn0 raises: training-mode statistics over ONE value per channel
            raise ValueError('Expected more than 1 value per channel when training, got input size [1, 512, 1]')
        h, st, bn_in = z_slow.reshape(B, -1, 1), None, None
        for i in range(4):
            bn = getattr(self, 'bn%d' % i)
            h, st = TT.tseed_bn(h, st, getattr(self, 'dc%d' % i), bn_in, bn, self.training)
            bn_in = bn
        return TT.tseed_tanh(h, st, self.dc4, bn_in)
