"""MeanScaleCompressor2018 -- the mean-scale hyperprior of Minnen et al. 2018 without the context
model, on the transforms, entropy models and coder of Compressor2018.

h_s predicts a mean mu beside the scale sigma, and y is coded about it: the symbols are the residual
rint(y - mu), the reconstruction is r + mu.  Nothing is autoregressive, so the chunked wave64 coder
serves it as it serves the scale-only model.  Differences from Compressor2018:
  * h_a reads the signed latent y, not |y| (a mean cannot be predicted from magnitudes);
  * h_s has two heads on one trunk: `prior_synthesis` (unchanged, state-dict keys included) gives sigma,
    `prior_mean`, one transposed conv shaped like prior_synthesis's last layer, gives mu with no
    activation -- one conv with 2 x LATENT outputs split in two, written as two convs so that each has
    the shape the existing conv plans serve;
  * the hyperprior runs serially in both modes: in eval mode y_hat = rint(y - mu) + mu depends on mu, so
    g_s cannot run beside it, and the training step takes the same route (side-stream concurrency for it
    is not built).
A scale-only checkpoint's shared modules load with strict=False (missing: prior_mean.weight / .bias);
h_a then sees signed inputs it was not trained on, so this is a starting point, not a converted model."""
import math

import torch
import torch.nn as nn

from ... import codec as _codec
from ..blocks.entropy_model import center_round
from ..layers import ConvTranspose2d
from .bmshl2018 import Compressor2018
from .build import META_ARCH_REGISTRY


@META_ARCH_REGISTRY.register()
class MeanScaleCompressor2018(Compressor2018):
    def __init__(self, cfg):
        super().__init__(cfg)
        # after every shared module: their initial values are Compressor2018's from the same seed
        hp = cfg.MODEL.HYPER_PRIOR
        k, s = list(hp.KERNELS)[0], list(hp.STRIDES)[0]   # h_s reverses the lists: its last layer has the first pair
        self.prior_mean = ConvTranspose2d(cfg.MODEL.INTER_CHANNELS, cfg.MODEL.LATENT_CHANNELS, k, stride=s,
                                          padding=k // 2, bias=True, output_padding=s - 1)
        nn.init.xavier_normal_(self.prior_mean.weight.data, math.sqrt(2))
        nn.init.constant_(self.prior_mean.bias.data, 0.01)
        self.concurrent_hyperprior = False

    def hyperprior_modules(self):
        """No module runs on the hyperprior side stream: the hyperprior is serial in both modes."""
        return []

    def gradient_streams(self, device):
        """No parameter's gradient is produced on a side stream."""
        return []

    def _hyper_input(self, y):
        return y

    def _prior(self, z_hat):
        """(sigma, mu): both heads on the one trunk activation."""
        if self._hs_invariant():   # the mean head shares the last layer's launch
            with torch.no_grad():
                return self.prior_synthesis.invariant(z_hat, second=(self.prior_mean.weight, self.prior_mean.bias))
        t = self.prior_synthesis.trunk(z_hat)
        return self.prior_synthesis.finish(t), self.prior_mean(t)

    def _stream_kind(self):
        return self.conditional_model.KIND | _codec.KIND_MEAN

    def forward(self, x):
        """Training: (x_tilde.detach(), losses) as Compressor2018, with y~ = y + u and
        p_y = conditional(y, sigma, mu); the Philox draws in the same order (z, then y).
        Eval: inference only -- y_hat = rint(y - mu) + mu, p_y the pmf of the residual at mean 0 (what the
        coder's tables are built from), the whole forward under no_grad: its outputs carry no grad."""
        if self.concurrent_hyperprior:   # Compressor2018's side-stream branch is the scale-only step
            raise NotImplementedError("the mean-scale hyperprior runs serially: concurrent_hyperprior must stay False")
        if self.training:
            return super().forward(x)
        cm = self.conditional_model
        if float(cm.bin) != 1.0:   # in front of any launch
            raise NotImplementedError(f"the eval forward rounds the residual to integers: BIN must be 1, got {cm.bin}")
        with torch.no_grad():
            return super().forward(x)

    def _check_call(self, N, H, W, who):
        cm = self.conditional_model
        if float(cm.bin) != 1.0:
            raise NotImplementedError(f"{who} rounds the residual to integers, as the eval forward does: BIN must be 1, "
                                      f"got {cm.bin}")

    def _forward_y(self, y, sigma, mu):
        cm = self.conditional_model
        if self.training:
            return cm(y, sigma, mu)
        r, y_tilde = center_round(y, mu.expand_as(y))
        return y_tilde, cm.likelihood(r, sigma)
