"""h_s (reference modelling/blocks/prior_synthesis.py:40-72): transposed convs
with the hyper-prior kernels/strides reversed, ReLU between, then
sigma = clamp(exp(.), 1e-10, 1e10)."""
import math

import torch.nn as nn

from ...functional import ExpClampFn, hs_layer, hs_supported
from ..layers import ConvTranspose2d, ReLU


class HyperpriorSynthesisTransform(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        hp = cfg.MODEL.HYPER_PRIOR
        n = len(hp.STRIDES)
        mods = []
        for i, (s, k) in enumerate(zip(reversed(list(hp.STRIDES)), reversed(list(hp.KERNELS)))):
            cout = cfg.MODEL.INTER_CHANNELS if i < n - 1 else cfg.MODEL.LATENT_CHANNELS
            conv = ConvTranspose2d(cfg.MODEL.INTER_CHANNELS, cout, k, stride=s, padding=k // 2,
                                   bias=True, output_padding=s - 1)
            nn.init.xavier_normal_(conv.weight.data, math.sqrt(2))
            nn.init.constant_(conv.bias.data, 0.01)
            mods.append(conv)
            if i < n - 1:
                mods.append(ReLU())
        self._layers = nn.Sequential(*mods)
        # how the inference paths compute h_s (MODEL.HYPER_SYNTHESIS.KERNEL); no parameter or state-dict key depends on it
        self.kernel = cfg.MODEL.get("HYPER_SYNTHESIS", {}).get("KERNEL", "conv")
        if self.kernel not in ("conv", "invariant"):
            raise ValueError(f'MODEL.HYPER_SYNTHESIS.KERNEL {self.kernel!r}: expected "conv" or "invariant"')
        if self.kernel == "invariant":
            for conv in self.convs():
                k, s = conv.kernel_size[0], conv.stride[0]
                if not hs_supported(conv.in_channels, conv.out_channels, k, s):
                    raise ValueError(f'MODEL.HYPER_SYNTHESIS.KERNEL "invariant": no kernel for the h_s layer k {k}, stride '
                                     f"{s}, channels {conv.in_channels} -> {conv.out_channels} (k odd and at most 5, "
                                     "stride 1 or 2, 1 .. 4096 channels)")

    def convs(self):
        """The transposed convs of h_s, in order."""
        return [m for m in self._layers if isinstance(m, ConvTranspose2d)]

    def invariant(self, z_hat, second=None):
        """forward(z_hat) by the batch-invariant kernel (functional.hs_layer): one launch per layer, the ReLUs and the
        exp-clamp in the epilogues.  `second` = (weight, bias) of a second head shaped like the last layer, on the
        trunk activation and in the last launch: the result is then (sigma, that head's plain output).  Inference
        only; image n's bits do not depend on the batch."""
        convs = self.convs()
        t = z_hat
        for conv in convs[:-1]:
            t = hs_layer(t, conv.weight, conv.bias, conv.stride[0], "relu")
        last = convs[-1]
        return hs_layer(t, last.weight, last.bias, last.stride[0], "exp_clamp",
                        second=None if second is None else (*second, "none"), clamp=(1e-10, 1e10))

    def forward(self, x):
        return ExpClampFn.apply(self._layers(x), 1e-10, 1e10)

    # forward(x) in two steps, for a model with a second head on the same trunk
    # (MeanScaleCompressor2018): finish(trunk(x)) runs the modules forward(x) runs, in its order.
    def trunk(self, x):
        """The activation that feeds the last layer (every layer but the last, ReLU included)."""
        return self._layers[:-1](x)

    def finish(self, t):
        """sigma from the trunk activation: the last layer, then the exp-clamp."""
        return ExpClampFn.apply(self._layers[-1](t), 1e-10, 1e10)
