"""Parameter layout of GANimation's generator (third_part/ganimation_replicate/model/model_utils.py:
209-248, 419-482): SplitGenerator(3, 17, 64, InstanceNorm2d(affine=False), n_blocks=6, padding 'zero'), the
network GANimationModel.initialize builds (ganimation.py:16).

``model`` is the reference's nn.Sequential by index: a 7x7 stem (0), two 4x4 stride-2 stages (3, 6), six
ResnetBlocks (9..14, two 3x3 convs each under ``conv_block.0`` / ``conv_block.3``), two 4x4 stride-2
transposed stages (15, 18); the instance norms and ReLUs between them hold no parameters or buffers.
``color_top.0`` / ``au_top.0`` are the two 7x7 heads without bias.  The class only declares the parameters
under the reference attribute paths, so ``30_net_gen.pth`` loads with strict=True: 36 entries.
"""
from __future__ import annotations

from torch import nn

IMG_NC, AUS_NC, NGF, N_BLOCKS = 3, 17, 64, 6
IN_EPS = 1e-5                              # nn.InstanceNorm2d's default; biased variance
DOWN = ((3, NGF, 2 * NGF), (6, 2 * NGF, 4 * NGF))                  # (index in ``model``, cin, cout)
BLOCKS = tuple(range(9, 9 + N_BLOCKS))
UP = ((15, 4 * NGF, 2 * NGF), (18, 2 * NGF, NGF))


class _Block(nn.Module):
    """ResnetBlock with padding 'zero': conv_block = [conv, IN, ReLU, conv, IN]."""

    def __init__(self, dim):
        super().__init__()
        self.conv_block = nn.Sequential(nn.Conv2d(dim, dim, 3, padding=1), nn.Identity(), nn.Identity(),
                                        nn.Conv2d(dim, dim, 3, padding=1), nn.Identity())


class SplitGeneratorParams(nn.Module):
    def __init__(self, img_nc=IMG_NC, aus_nc=AUS_NC, ngf=NGF, n_blocks=N_BLOCKS):
        super().__init__()
        if (img_nc, aus_nc, ngf, n_blocks) != (IMG_NC, AUS_NC, NGF, N_BLOCKS):
            raise NotImplementedError("SplitGenerator: only the (3, 17, 64, n_blocks=6) network of "
                                      "GANimationModel.initialize is built")
        layers = [nn.Identity() for _ in range(21)]
        layers[0] = nn.Conv2d(img_nc + aus_nc, ngf, 7, 1, 3)
        for i, cin, cout in DOWN:
            layers[i] = nn.Conv2d(cin, cout, 4, 2, 1)
        for i in BLOCKS:
            layers[i] = _Block(4 * ngf)
        for i, cin, cout in UP:
            layers[i] = nn.ConvTranspose2d(cin, cout, 4, 2, 1)
        self.model = nn.Sequential(*layers)
        self.color_top = nn.Sequential(nn.Conv2d(ngf, img_nc, 7, 1, 3, bias=False), nn.Identity())
        self.au_top = nn.Sequential(nn.Conv2d(ngf, 1, 7, 1, 3, bias=False), nn.Identity())


def check_input(h: int, w: int):
    """Two stride-2 stages down and two up: the output has the input's size only when both divide by 4."""
    if h <= 0 or w <= 0 or h % 4 or w % 4:
        raise ValueError(f"GANimation: a {h}x{w} input; both sides must be positive multiples of 4")
