"""StackGAN++-style conditioning augmentation (CA) in front of the text-conditioned generator's fc. The reference has no such
module (SURVEY headline fact 4): it is an opt-in block, off by default (`MultiScaleGen(ca_dim=0)`), see DESIGN "Conditioning
augmentation". Parameters `fc.weight` [4D, cond_dim] and `fc.bias` [4D], initialised by `init()` like every other Linear."""
import torch.nn as nn

from .layers import Linear


class CondAugmentation(nn.Module):
    def __init__(self, cond_dim, ca_dim):
        super().__init__()
        if cond_dim < 1 or ca_dim < 1:
            raise ValueError('conditioning augmentation needs cond_dim >= 1 and ca_dim >= 1 (got %d, %d)' % (cond_dim, ca_dim))
        self.cond_dim, self.ca_dim = cond_dim, ca_dim
        self.fc = Linear(cond_dim, 4 * ca_dim)

    def forward(self, z, cond):
        """([z | c] [B, latent + ca_dim], KL 0-d). eps ~ N(0, 1) [B, ca_dim] comes from `TF.draws` (host generator, like z) —
        one draw per call, in train and in eval mode."""
        from .. import functional as TF
        from ..functional_ca import cond_aug
        h = self.fc(cond)
        eps = TF.draws.ca_eps(cond.size(0), self.ca_dim, cond.device)
        return cond_aug(h, z, eps)
