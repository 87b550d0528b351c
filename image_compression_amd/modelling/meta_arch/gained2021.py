"""GainedMeanScaleCompressor2018 -- the mean-scale hyperprior with the gain units of Cui et al. 2021 ("Asymmetric
Gained Deep Image Compression With Continuous Rate Adaptation"): one network for a ladder of rates.

The model carries S learnt per-channel gain vectors for y and for z, and their inverses, as four level tables of
logarithms (`gain`: log_y, log_inv_y (S, LATENT_CHANNELS), log_z, log_inv_z (S, INTER_CHANNELS)); level s is trained
against MODEL.GAIN.LOSS_WEIGHTS[s].  A quality q in [0, S-1] picks the vectors by the gain-vector rule of codec.py
(csrc/gain.hip): exp(t[q]) at an integer q, the geometric interpolation of the neighbouring levels between them.  With
(g_y, g_y', g_z, g_z') the four vectors at the call's quality, every product one fp32 multiplication per element:
    y = g_a(x);  z = h_a(y)
    z_g = z * g_z            -> factorized model (noise / rint); the symbols of z are rint(z_g)
    z_hat = z_g~ * g_z'      -> (sigma, mu) = both heads of h_s(z_hat)
    y_g = y * g_y            -> conditional model about mu (train), rint(y_g - mu) + mu (eval, coder)
    y_hat = y_g~ * g_y'      -> g_s, clamp
All of it through the hooks of Compressor2018's skeleton: the forward and the four bitstream calls are the
skeleton's.  The tables start at zero, where every gain is exactly 1.0: a fresh model computes what
MeanScaleCompressor2018 computes from the same seed, and a mean-scale checkpoint loaded with strict=False (missing:
the four tables) is a converted model.

Quality.  `set_quality(q)` / `quality`: the quality of the eval forward and of `compress` (default S-1);
`set_quality([q_0, ..., q_{N-1}])`: one quality per image, for `compress_each` alone.  The decoders take the quality
from the stream, never from the model.  In training mode with `sample_quality` (the default) every forward draws
an integer level uniformly from a CPU generator seeded with cfg.SEED (`last_quality`; no device draw, the Philox
order z, then y is unchanged); with `sample_quality = False` it uses `quality`.  The distortion weight of a step is
LOSS_WEIGHTS at its level, between levels exp of the interpolated logarithms: it and the level change on the host
every step, which is why TrainStep(graph=True) refuses this model (`graph_refusal`)."""
import math
from numbers import Real

import numpy as np
import torch
import torch.nn as nn

from ... import codec as _codec
from ...functional import channel_scale, gain_vector
from .build import META_ARCH_REGISTRY
from .mshp2018 import MeanScaleCompressor2018


class GainUnit(nn.Module):
    """The four level tables, logarithms of the gains: y and z, forward and inverse.  Zero: every gain is 1."""

    def __init__(self, levels, latent_channels, hyper_channels):
        super().__init__()
        self.log_y = nn.Parameter(torch.zeros(levels, latent_channels))
        self.log_inv_y = nn.Parameter(torch.zeros(levels, latent_channels))
        self.log_z = nn.Parameter(torch.zeros(levels, hyper_channels))
        self.log_inv_z = nn.Parameter(torch.zeros(levels, hyper_channels))

    def forward(self, qualities):
        """(g_y, g_y', g_z, g_z'), each (len(qualities), C): the gain vectors at every quality."""
        return tuple(gain_vector(t, qualities) for t in (self.log_y, self.log_inv_y, self.log_z, self.log_inv_z))


def _as_quality(q, levels):
    """q as the float32 value the container stores; ValueError outside [0, levels - 1] (NaN included)."""
    if isinstance(q, bool) or not isinstance(q, Real):
        raise ValueError(f"a quality is a number in [0, {levels - 1}], got {q!r}")
    v = float(np.float32(q))
    if not 0.0 <= v <= levels - 1:
        raise ValueError(f"quality {q!r} is outside [0, {levels - 1}]")
    return v


@META_ARCH_REGISTRY.register()
class GainedMeanScaleCompressor2018(MeanScaleCompressor2018):
    graph_refusal = ("GainedMeanScaleCompressor2018 draws its gain level and its distortion weight on the host every "
                     "step: a captured graph would replay one level for ever; use TrainStep(graph=False)")

    def __init__(self, cfg):
        super().__init__(cfg)
        weights = [float(w) for w in cfg.MODEL.GAIN.LOSS_WEIGHTS]
        if len(weights) < 2 or not all(math.isfinite(w) and w > 0.0 for w in weights):
            raise ValueError(f"MODEL.GAIN.LOSS_WEIGHTS must hold at least 2 positive weights, got {weights}")
        self.loss_weights = weights
        self.levels = len(weights)
        # after every inherited module: their initial values are MeanScaleCompressor2018's from the same seed
        self.gain = GainUnit(self.levels, cfg.MODEL.LATENT_CHANNELS, cfg.MODEL.INTER_CHANNELS)
        self.sample_quality = True
        self.last_quality = None
        self._quality = float(self.levels - 1)
        self._sampler = torch.Generator().manual_seed(int(cfg.SEED))
        self._gains = self._qualities = None
        self.distortion_loss_weight = self.loss_weight(self._quality)

    # ---- quality
    @property
    def quality(self):
        return self._quality

    def set_quality(self, q):
        """A float in [0, S-1], or a sequence of them: one per image of the next `compress_each` calls."""
        if isinstance(q, (str, bytes)):
            raise ValueError(f"a quality is a number in [0, {self.levels - 1}], got {q!r}")
        if isinstance(q, (list, tuple, np.ndarray, torch.Tensor)) and getattr(q, "ndim", 1) > 0:
            q = [_as_quality(v.item() if hasattr(v, "item") else v, self.levels) for v in q]
            if not q:
                raise ValueError("an empty sequence of qualities")
            self._quality = q
        else:
            self._quality = _as_quality(q.item() if hasattr(q, "item") else q, self.levels)

    def _one_quality(self, who):
        if isinstance(self._quality, list):
            raise ValueError(f"{who} takes one quality for the batch: a sequence of qualities serves compress_each only")
        return self._quality

    def sample_level(self):
        """The next integer level of the training sampler, uniform over the S levels (CPU generator, cfg.SEED)."""
        return int(torch.randint(0, self.levels, (1,), generator=self._sampler))

    def loss_weight(self, q):
        """LOSS_WEIGHTS at an integer level; between levels exp of the linear interpolation of the log-weights."""
        s = min(int(math.floor(q)), self.levels - 2)
        f = q - s
        if f == 0.0 or f == 1.0:
            return self.loss_weights[s + int(f)]
        a, b = math.log(self.loss_weights[s]), math.log(self.loss_weights[s + 1])
        return math.exp(a + f * (b - a))

    def _use(self, qualities):
        """The gain vectors of the call: one row for the batch, or one per image."""
        self._qualities = tuple(qualities)
        self._gains = self.gain(self._qualities)

    # ---- the forward
    def forward(self, x):
        self._one_quality("forward")   # in front of any launch
        return super().forward(x)

    def _forward(self, x):
        q = self._one_quality("forward")
        if self.training and self.sample_quality:
            q = float(self.sample_level())
        self.last_quality = q
        self.distortion_loss_weight = self.loss_weight(q)
        try:
            self._use((q,))
            return super()._forward(x)
        finally:
            self._gains = self._qualities = None   # no graph kept alive by module state

    def _check_call(self, N, H, W, who):
        super()._check_call(N, H, W, who)
        self._one_quality(who)

    def _begin_call(self, N, H, W, device, who):
        self._use((self._one_quality(who),))

    def _end_call(self):
        self._gains = self._qualities = None

    def _hyper_gain(self, z):
        return channel_scale(z, self._gains[2])

    def _hyper_ungain(self, z_hat):
        return channel_scale(z_hat, self._gains[3])

    def _latent_gain(self, y):
        return channel_scale(y, self._gains[0])

    def _latent_ungain(self, y_hat):
        return channel_scale(y_hat, self._gains[1])

    # ---- bitstreams: containers "ICRG" and "ICRQ" (codec.py)
    _pack, _parse = staticmethod(_codec.pack_gained), staticmethod(_codec.parse_gained)
    _pack_image, _parse_image = staticmethod(_codec.pack_gained_image), staticmethod(_codec.parse_gained_image)

    def _codable(self):
        super()._codable()
        self._gains = self._qualities = None

    def _analyse(self, x, each=False):
        if each and isinstance(self._quality, list):
            if len(self._quality) != x.shape[0]:
                raise ValueError(f"compress_each: {len(self._quality)} qualities for {x.shape[0]} images")
            self._use(self._quality)
        else:
            self._use((self._one_quality("compress"),))
        return super()._analyse(x, each)

    def _header(self, N, H, W, y, z, steps_per_chunk, kz, ky, size=None, image=0):
        h = super()._header(N, H, W, y, z, steps_per_chunk, kz, ky, size)
        quality = self._qualities[image if len(self._qualities) > 1 else 0]
        return (_codec.GainedHeader if size is None else _codec.GainedImageHeader)(**vars(h), levels=self.levels,
                                                                                  quality=quality)

    def _check_stream(self, h, who, stream="the stream"):
        super()._check_stream(h, who, stream)
        if h.levels != self.levels:
            raise ValueError(f"{who}: {stream} was coded by a different model ({h.levels} gain levels, this model has "
                             f"{self.levels})")

    def _begin_decode(self, headers):
        self._use([h.quality for h in headers])
