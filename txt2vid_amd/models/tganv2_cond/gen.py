"""Text-conditioned TGANv2 generator: `cat(z, cond)` into fc, 2-D non-local block after the third
abstract block — txt2vid/models/tganv2_cond/gen.py:22-124. `ca_dim > 0` (not in the reference): `cat(z, c)` with c the
conditioning augmentation of the sentence code (models/ca.py). `cond_bn=True` (not in the reference): every BatchNorm2d is
modulated by a projection of that condition vector (functional_cbn.py)."""
from ..tganv2.gen import MultiScaleGen as _Base, BaseFrameGen  # noqa: F401


class MultiScaleGen(_Base):
    _cond_variant = True

    def __init__(self, latent_size=256, width=64, height=64, num_channels=3, additional_blocks=[64, 32, 32],
                 fm_channels=1024, num_frames=16, cond_dim=256, no_lstm=False, ca_dim=0,
                 ca_kl_coeff=2.0, cond_bn=False):
        super().__init__(latent_size=latent_size, width=width, height=height, num_channels=num_channels,
                         additional_blocks=additional_blocks, fm_channels=fm_channels, num_frames=num_frames,
                         cond_dim=cond_dim, no_lstm=no_lstm, ca_dim=ca_dim, ca_kl_coeff=ca_kl_coeff, cond_bn=cond_bn)
