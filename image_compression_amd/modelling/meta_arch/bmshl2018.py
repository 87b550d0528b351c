"""Compressor2018 — Balle et al. 2018 scale hyperprior (reference
modelling/meta_arch/bmshl2018.py:49-110), every tensor op on HIP kernels.

forward(x) -> (x_tilde.detach(), losses) with losses =
{z_entropy, y_entropy, bpp, total_loss, <distortion names>}; only
total_loss carries grad."""
import math
import os
from numbers import Real
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ... import codec as _codec
from ... import noise as _noise
from ...functional import (AbsFn, CELossFn, NonNegFn, NonNegMultiFn, RoundThroughFn, _match, _to_last, block_bits,
                           block_sse, conditional_likelihood, factorized, refine_dist_grad, refine_keep, refine_kmax,
                           refine_objective, refine_update, route_weight_gradients)
from ..blocks.entropy_model import (_decode_seg, _encode_seg, symbolize, symbolize_mean, symbolize_mean_seg,
                                    symbolize_seg, symbols_as_tensor, table_pool)
from ..blocks import (ENTROPY_MODEL_REGISTRY, AnalysisTransform, HyperpriorAnalysisTransform,
                      HyperpriorSynthesisTransform, SynthesisTransform)
from ..layers import LowerBound, UpperBound
from ..loss import get_loss_dict
from .build import META_ARCH_REGISTRY


class RDMap(NamedTuple):
    """What `Compressor2018.rate_distortion_map` returns.  A block is 64 x 64 pixels (codec.MAP_BLOCK); the maps are
    fp32 (N, Hb, Wb) over the padded size, Hb = ceil(h / 64), Wb = ceil(w / 64)."""
    bits_y: torch.Tensor    # estimated bits of y's 4 x 4 positions of every block
    bits_z: torch.Tensor    # estimated bits of z's position of every block
    bits: torch.Tensor      # bits_y + bits_z, one fp32 addition
    sse: torch.Tensor       # squared error of x against x_hat over the block's real pixels and 3 channels
    pixels: np.ndarray      # (Hb, Wb) int64: the real pixels of every block
    x_hat: torch.Tensor     # (N, 3, h, w), the eval forward's reconstruction (cropped when the image was padded)
    p_y: Optional[torch.Tensor] = None   # with likelihoods=True: (N, M, H / 16, W / 16), what bits_y sums
    p_z: Optional[torch.Tensor] = None   # (N, C_z, H / 64, W / 64), what bits_z sums


class RefineReport(NamedTuple):
    """What `Compressor2018.compress_each_refined` returns beside the streams: per-image lists.  J = B + w D in bits
    (codec.py: the refinement rule), B the estimated bits of y and D the squared error over the padded image."""
    before: list        # J of the unrefined latent (evaluation 0)
    after: list         # J of the symbols that were coded
    bits_before: list
    bits_after: list
    sse_before: list
    sse_after: list
    step: list          # the evaluation that won; 0: the unrefined latent


def block_pixels(h, w):
    """(ceil(h / 64), ceil(w / 64)) int64: how many pixels of an h x w image every 64 x 64 block holds."""
    b = _codec.MAP_BLOCK
    rows = np.minimum(b, h - b * np.arange(-(-h // b), dtype=np.int64))
    cols = np.minimum(b, w - b * np.arange(-(-w // b), dtype=np.int64))
    return rows[:, None] * cols[None, :]


_SIDE = {}
_WGRAD = {}


class _StreamEdge(torch.autograd.Function):
    """Identity at a stream crossing.  Forward runs on the consumer stream of the value;
    backward (on that same stream) records the incoming gradient on `other`, the stream
    that consumes the gradient next, before handing it over."""

    @staticmethod
    def forward(ctx, t, other):
        ctx.other = other
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        if g is not None:
            g.record_stream(ctx.other)
        return g, None


def side_stream(device):
    """One side stream per device for the hyperprior branch, and beside it a stream for the
    hyperprior convs' weight gradients (functional: convs run on the side stream compute them there,
    off the chain of input gradients g_a's backward waits for).  Both at normal priority: a
    high-priority side stream dispatched its blocks ahead of the main stream's critical kernels
    whenever a CU freed up (C3 6.44 -> 6.35 ms per step at normal priority, C2 equal; r05s,
    profiles/r05s_side_priority_ab.txt)."""
    k = device.index if device.index is not None else torch.cuda.current_device()
    if k not in _SIDE:
        # IMGCOMP_SIDE_PRIORITY: stream priority of the two (0 normal, -1 high); diagnostic A/B knob
        prio = int(os.environ.get("IMGCOMP_SIDE_PRIORITY", "0"))
        _SIDE[k] = torch.cuda.Stream(device=device, priority=prio)
        _WGRAD[k] = torch.cuda.Stream(device=device, priority=prio)
        route_weight_gradients(_SIDE[k], _WGRAD[k])
    return _SIDE[k]


def wgrad_stream(device):
    """The stream the hyperprior convs' weight gradients run on (see side_stream)."""
    side_stream(device)
    return _WGRAD[device.index if device.index is not None else torch.cuda.current_device()]


@META_ARCH_REGISTRY.register()
class Compressor2018(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.analysis_transform = AnalysisTransform(cfg)
        self.prior_analysis = HyperpriorAnalysisTransform(cfg)
        self.prior_synthesis = HyperpriorSynthesisTransform(cfg)
        self.synthesis_transform = SynthesisTransform(cfg)
        # The reference sizes the factorized model with LATENT_CHANNELS while z
        # carries INTER_CHANNELS (crash when they differ); z's
        # channel count is used here, identical whenever the reference runs.
        self.entropy_model = ENTROPY_MODEL_REGISTRY.get("EntropyModel")(cfg.MODEL.INTER_CHANNELS, cfg)
        self.conditional_model = ENTROPY_MODEL_REGISTRY.get(cfg.MODEL.ENTROPY_MODEL.CONDITIONAL_MODEL)(cfg)
        self.distortion_loss_fns = get_loss_dict(cfg, cfg.MODEL.LOSS.DISTORTION_LOSS_NAMES)
        self.distortion_loss_weight = cfg.MODEL.LOSS.DISTORTION_LOSS_WEIGHT
        self.loss_names = ["y_entropy", "z_entropy", "bpp"] + list(self.distortion_loss_fns.keys())
        # g_s's taps and strides: what a pixel of the output depends on (decompress_window)
        self._synthesis_geometry = (int(cfg.MODEL.CONV_KERNEL), tuple(int(s) for s in cfg.MODEL.STRIDES))
        # y's channels: what the layers of a layered stream divide (compress_each_layered)
        self._latent_channels = int(cfg.MODEL.LATENT_CHANNELS)
        # the hyperprior branch (h_a, factorized model, h_s, the y likelihood) on a second
        # stream, concurrent with the synthesis transform (see forward)
        self.concurrent_hyperprior = True
        # how the inference paths compute h_s: "conv" (the conv plans) or "invariant" (functional.hs_layer); validated
        # by HyperpriorSynthesisTransform.  It is the streams' format version (`_format_version`)
        self.hs_kernel = self.prior_synthesis.kernel

    def _hs_invariant(self):
        """Whether h_s runs through the batch-invariant kernel: MODEL.HYPER_SYNTHESIS.KERNEL "invariant", outside
        training mode."""
        return self.hs_kernel == "invariant" and not self.training

    def hyperprior_modules(self):
        """The modules whose forward, and so whose backward, run on the hyperprior side stream
        when concurrent_hyperprior is on (h_a, the factorized model, h_s, the conditional
        model): their parameters' gradients are produced on that stream (distributed.wrap)."""
        return [self.prior_analysis, self.entropy_model, self.prior_synthesis, self.conditional_model]

    def gradient_streams(self, device):
        """[(stream, parameters)]: the stream each hyperprior parameter's gradient is produced and
        accumulated on when concurrent_hyperprior is on -- the convs' weights and biases on the
        weight-gradient stream, the entropy models' parameters on the side stream (main-stream
        parameters are not listed).  distributed.wrap makes their AccumulateGrad nodes there."""
        convs = [p for blk in (self.prior_analysis, self.prior_synthesis) for m in blk.modules()
                 if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) for p in m.parameters(recurse=False)]
        ids = {id(p) for p in convs}
        rest = [p for m in self.hyperprior_modules() for p in m.parameters() if id(p) not in ids]
        return [(wgrad_stream(device), convs), (side_stream(device), rest)]

    def _reparameterise_gdn(self, x):
        """Each main transform's GDN gamma / beta (NonNegativeParam) formed by one launch, their
        gradients by one more (functional.NonNegMultiFn), instead of two launches per parameter;
        every NonNegativeParam returns the value formed here at its next call.  Only with autograd
        on a device tensor (the eval weight cache keeps its own values)."""
        from ..layers.gdn import NonNegativeParam
        for blk in (self.analysis_transform, self.synthesis_transform):
            mods = [m for m in blk.modules() if isinstance(m, NonNegativeParam)]
            for m in mods:
                m.__dict__.pop("_pre", None)
            if mods and x.is_cuda and torch.is_grad_enabled():
                vals = NonNegMultiFn.apply([float(m.bound) for m in mods], [float(m.pedestal) for m in mods],
                                           *[m.param for m in mods])
                for m, v in zip(mods, vals):
                    m.__dict__["_pre"] = v

    def _clear_reparameterised(self):
        from ..layers.gdn import NonNegativeParam
        for blk in (self.analysis_transform, self.synthesis_transform):
            for m in blk.modules():
                if isinstance(m, NonNegativeParam):
                    m.__dict__.pop("_pre", None)

    def forward(self, x):
        # every GDN consumes its pre-formed value during the step; if the step raises first, none
        # may stay behind in the module (a stale value, and a graph kept alive by module state)
        try:
            return self._forward(x)
        finally:
            self._clear_reparameterised()

    def _forward(self, x):
        if self.training:
            _noise.begin_step(x.device)  # fresh Philox counters for this step
        self._reparameterise_gdn(x)
        N, _, H, W = x.shape
        num_pixels = N * H * W
        y = self.analysis_transform(x)
        cm = self.conditional_model
        # the split path calls cm.quantize / cm.likelihood instead of cm(y, sigma): with a
        # forward hook on cm (a caller observing its (q, p)) the call stays whole (serial)
        hooked = bool(cm._forward_hooks or cm._forward_pre_hooks or nn.modules.module._global_forward_hooks
                      or nn.modules.module._global_forward_pre_hooks)
        # under "invariant" the eval forward is the serial step: its sigma comes from `_prior`, as the coder's does
        if (self.concurrent_hyperprior and x.is_cuda and hasattr(cm, "quantize") and not hooked
                and not self._hs_invariant()):
            # every tensor that crosses streams passes a _StreamEdge: its gradient, computed on
            # one stream and consumed on the other, is recorded on the consumer's stream, so the
            # caching allocator does not hand its memory to the producer stream's next
            # allocation while the consumer still reads it
            # y~ = y + noise (train) / round(y) (eval) does not depend on sigma, so the synthesis
            # transform need not wait for the hyperprior: the hyperprior branch and the y
            # likelihood run on a side stream while g_s runs here, and autograd runs their
            # backward on the same streams (the small hyperprior kernels hide under g_s's).
            # Same kernels, same draws in the same order (z, then y): bitwise the serial result.
            main = torch.cuda.current_stream(x.device)
            side = side_stream(x.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                y.record_stream(side)
                y_s = _StreamEdge.apply(y, main)
                z = self.prior_analysis(AbsFn.apply(y_s))
                z_tilde, _z_probs, z_ce = self.entropy_model(z)
                sigma = self.prior_synthesis(z_tilde)
            y_tilde = self.conditional_model.quantize(y)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                y_tilde.record_stream(side)
                y_probs = self.conditional_model.likelihood(_StreamEdge.apply(y_tilde, main), sigma)
                y_ce = self.conditional_model._ce_loss(y_probs)
            x_tilde = self.synthesis_transform(y_tilde)
            x_tilde = LowerBound.apply(UpperBound.apply(x_tilde, 1.), 0.)
            dist = self.distortion_loss(x, x_tilde)
            main.wait_stream(side)
            z_ce.record_stream(main)
            y_ce.record_stream(main)
            z_ce = _StreamEdge.apply(z_ce, side)
            y_ce = _StreamEdge.apply(y_ce, side)
        else:
            # the serial step of every model, its differences in _hyper_input, _prior and _forward_y
            z = self._hyper_gain(self.prior_analysis(self._hyper_input(y)))
            z_tilde, _z_probs, z_ce = self.entropy_model(z)
            y_tilde, y_probs = self._forward_y(self._latent_gain(y), *self._prior(self._hyper_ungain(z_tilde)))
            y_ce = self.conditional_model._ce_loss(y_probs)
            x_tilde = self._reconstruct(self._latent_ungain(y_tilde))
            dist = self.distortion_loss(x, x_tilde)
        return x_tilde.detach(), self._losses(z_ce, y_ce, dist, num_pixels)

    def _forward_y(self, y, sigma, mean):
        """(y_tilde, p_y) of the forward from y and `_prior`'s (sigma, mean): how y is quantised and scored."""
        return self.conditional_model(y, sigma)

    def _reconstruct(self, y_hat, sizes=None):
        """g_s and the clamp to [0, 1].  With `sizes`, the (h, w) of every image of the batch: a list of the images
        (1, 3, h, w), each the top-left corner of its reconstruction (the per-image streams' crop, inference only)."""
        x = self.synthesis_transform(y_hat)
        if sizes is None:
            return LowerBound.apply(UpperBound.apply(x, 1.), 0.)
        if len(set(sizes)) == 1:
            x = _lib.stream_ops().crop_clamp(x, *sizes[0])
            return [x[k:k + 1] for k in range(len(sizes))]
        return [_lib.stream_ops().crop_clamp(x[k:k + 1], h, w) for k, (h, w) in enumerate(sizes)]

    def _losses(self, z_ce, y_ce, dist, num_pixels):
        total_dist = sum(dist.values())
        entropy = (z_ce + y_ce) / num_pixels
        total = self.distortion_loss_weight * total_dist + entropy
        losses = {
            "z_entropy": z_ce.detach() / num_pixels,
            "y_entropy": y_ce.detach() / num_pixels,
            "bpp": entropy.detach(),
            "total_loss": total,
        }
        losses.update({k: v.detach() for k, v in dist.items()})
        return losses

    def distortion_loss(self, img1, img2):
        return {name: fn(img1, img2) for name, fn in self.distortion_loss_fns.items()}

    # ---- real bitstreams (beyond the reference, whose compress / decompress are stubs:
    # bmshl2018.py:106-110).  Format and contract: image_compression_amd/codec.py, INTEGRATION.md.
    def _codable(self):
        if self.training:
            raise RuntimeError("compress / decompress run in eval mode only: call model.eval() first")
        self._clear_reparameterised()

    # Where a model with another hyperprior or another way of coding y differs (MeanScaleCompressor2018,
    # CheckerboardCompressor2018): what h_a reads (_hyper_input), what h_s gives (_prior), the conditional-kind byte that
    # says so in the container (_stream_kind), how the forward quantises and scores y (_forward_y, above), how y becomes
    # streams and comes back (_encode_y / _decode_y), and the containers with the checks in front of them
    # (_pack / _parse, _pack_image / _parse_image, _codable_batch).  A model that rescales its latents around the
    # quantisers (GainedMeanScaleCompressor2018) overrides the four gain hooks, identities here, and learns what the
    # streams it is about to decode say about that in _begin_decode.
    def _hyper_input(self, y):
        return AbsFn.apply(y)

    def _hyper_gain(self, z):
        """z = h_a(.) as the factorized model quantises and codes it."""
        return z

    def _hyper_ungain(self, z_hat):
        """What h_s reads, from the hyper-latent as quantised (every image of the batch by its own rule)."""
        return z_hat

    def _latent_gain(self, y):
        """y as the conditional model quantises and codes it."""
        return y

    def _latent_ungain(self, y_hat):
        """What g_s reads, from the latent as quantised."""
        return y_hat

    def _begin_decode(self, headers):
        """The parsed, checked headers of the streams the next launches decode (one of a batch, or one per image),
        in front of `_prior`."""

    def _prior(self, z_hat):
        """(sigma, mean) from the hyper-latent's integers; mean None: y is coded about 0."""
        if self._hs_invariant():   # inference only: the eval forward's sigma carries no graph
            with torch.no_grad():
                return self.prior_synthesis.invariant(z_hat), None
        return self.prior_synthesis(z_hat), None

    def _stream_kind(self):
        return self.conditional_model.KIND

    def _encode_y(self, y, prior, steps_per_chunk):
        """(kmax_y, the streams [(payload, chunk lengths)] of y) under `_prior`'s (sigma, mean)."""
        sigma, mean = prior
        y_sym, ky = self._symbols(y, mean)
        return ky, [self.conditional_model.encode_symbols(y_sym, ky, sigma.expand_as(y), steps_per_chunk, mean=mean)]

    def _decode_y(self, h, streams, prior):
        """y_hat from the parsed header, the streams [(payload, chunk lengths)] of y and `_prior`'s (sigma, mean)."""
        (py, ly), = streams
        sigma, mean = prior
        return self.conditional_model.decompress(py, sigma, ly, h.kmax_y, h.R, mean=mean)

    # the model's containers (pack, parse, per-image pack, per-image parse) and the format version it writes and
    # reads in them: the route that computed h_s, so a stream is only ever decoded by the arithmetic that coded it
    _containers = (_codec.pack, _codec.parse, _codec.pack_image, _codec.parse_image)

    def _format_version(self):
        return _codec.INVARIANT_FORMAT_VERSION if self.hs_kernel == "invariant" else _codec.FORMAT_VERSION

    def _image_format_version(self):
        return self._format_version()

    def _pack(self, *parts):
        return self._containers[0](*parts, version=self._format_version())

    def _parse(self, data, abi, compute_dtype):
        return self._containers[1](data, abi, compute_dtype, version=self._format_version())

    def _pack_image(self, *parts):
        return self._containers[2](*parts, version=self._image_format_version())

    def _parse_image(self, data, abi, compute_dtype):
        return self._containers[3](data, abi, compute_dtype, version=self._image_format_version())

    def _codable_batch(self):
        self._codable()

    # ---- what compress, decompress and their per-image forms share
    def _build_id(self):
        """(ic_version(), COMPUTE_DTYPE): what a stream must have been coded by, as the parsers take them."""
        return int(_lib.load().ic_version()), getattr(self, "compute_dtype", "fp32")

    @staticmethod
    def _symbols(t, mean=None, each=False):
        """(int32 symbols, kmax) of t, about `mean` if there is one; `each`: image by image ([kmax of image n])."""
        if not each:
            return symbolize(t) if mean is None else symbolize_mean(t, mean)
        try:
            return symbolize_seg(t) if mean is None else symbolize_mean_seg(t, mean)
        except ValueError as e:
            raise ValueError(f"compress_each: {e}") from None

    def _analyse(self, x, each=False):
        """(y, z, symbols of z, kmax_z, `_prior`): g_a, h_a, and sigma (and the mean) from the integers the decoder
        will hold, in the layout it will hold them in; `each`: one image at a time, as that decoder computes them."""
        y = self.analysis_transform(x)
        z = self._hyper_gain(self.prior_analysis(self._hyper_input(y)))
        z_sym, kz = self._symbols(z, each=each)
        z_hat = self._hyper_ungain(symbols_as_tensor(z_sym.to(torch.float32), tuple(z.shape)))
        return y, z, z_sym, kz, (self._prior_each if each else self._prior)(z_hat)

    def _header(self, N, H, W, y, z, steps_per_chunk, kz, ky, size=None, image=0):
        """The Header of a batch's stream, or with `size` = (h, w) the ImageHeader of the stream of image `image` of
        the call."""
        cm = self.conditional_model
        abi, dtype = self._build_id()
        h = (_codec.Header if size is None else _codec.ImageHeader)(
            N, H, W, y.shape[1], z.shape[1], self._stream_kind(), dtype, abi, cm.num_scales, cm.scale_min, cm.scale_max,
            int(steps_per_chunk), kz, ky, *(size or ()))
        if tuple(z.shape[1:]) != h.z_shape[1:] or tuple(y.shape[1:]) != h.y_shape[1:]:
            who, what = ("compress", "image") if size is None else ("compress_each", "padded image")
            raise ValueError(f"{who}: latents {tuple(y.shape)} / {tuple(z.shape)} are not the {what} size over "
                             f"{_codec.Y_DOWN} / {_codec.Z_DOWN}")
        return h

    def _check_stream(self, h, who, stream="the stream"):
        em, cm = self.entropy_model, self.conditional_model
        if h.kind != self._stream_kind() or h.hyper_channels != em.channels:
            raise ValueError(f"{who}: {stream} was coded by a different model (conditional kind / channels)")
        if (h.L, h.scale_min, h.scale_max) != (cm.num_scales, cm.scale_min, cm.scale_max):
            raise ValueError(f"{who}: {stream} was coded with a different scale table")

    @torch.no_grad()
    def compress(self, x, steps_per_chunk=1024):
        """x (N, 3, H, W) in [0, 1], H and W multiples of 64 -> one bytes object for the batch."""
        self._codable_batch()
        if x.dim() != 4 or x.shape[2] % _codec.Z_DOWN or x.shape[3] % _codec.Z_DOWN:
            raise ValueError(f"compress: image size {tuple(x.shape)} must be (N, C, H, W) with H and W "
                             f"multiples of {_codec.Z_DOWN}")
        N, _, H, W = x.shape
        y, z, z_sym, kz, prior = self._analyse(x)
        pz, lz = self.entropy_model.encode_symbols(z_sym, kz, steps_per_chunk)
        ky, streams = self._encode_y(self._latent_gain(y), prior, steps_per_chunk)
        h = self._header(N, H, W, y, z, steps_per_chunk, kz, ky)
        return self._pack(h, lz, *(l for _, l in streams), pz, *(p for p, _ in streams))

    @torch.no_grad()
    def decompress(self, data):
        """bytes from `compress` (same weights, build, COMPUTE_DTYPE, device type and batch shape) ->
        x_hat (N, 3, H, W), the eval forward's reconstruction."""
        self._codable_batch()
        h, *rest = self._parse(data, *self._build_id())
        lens, payloads = rest[:len(rest) // 2], rest[len(rest) // 2:]
        self._check_stream(h, "decompress")
        self._begin_decode([h])
        z_hat = self.entropy_model.decompress(payloads[0], h.z_shape, lens[0], h.kmax_z, h.R)
        prior = self._prior(self._hyper_ungain(z_hat))
        if any(t is not None and tuple(t.shape) != h.y_shape for t in prior):
            raise ValueError(f"decompress: the model's sigma {tuple(prior[0].shape)} is not the stream's latent shape "
                             f"{h.y_shape}")
        return self._reconstruct(self._latent_ungain(self._decode_y(h, list(zip(payloads[1:], lens[1:])), prior)))

    # ---- per-image streams: any image size, every image its own self-contained stream (container
    # "ICRP", codec.py).  The one rule that makes stream n decodable alone: h_s runs one image at a
    # time on both sides, so the sigma bits that select the table rows do not depend on the batch.
    def _codable_each(self):
        self._codable()
        self.entropy_model._codable()       # BIN == 1, before anything is computed
        self.conditional_model._codable()

    def _prior_each(self, z_hat):
        """`_prior` of every image of z_hat on its own (batch shape 1), concatenated.  Under "invariant" image n's
        bits do not depend on the batch: one call for all of them."""
        if self._hs_invariant():
            return self._prior(z_hat)
        parts = [self._prior(z_hat[n:n + 1]) for n in range(z_hat.shape[0])]
        if len(parts) == 1:
            return parts[0]
        sigma, mean = zip(*parts)
        return torch.cat(sigma), (None if mean[0] is None else torch.cat(mean))

    @staticmethod
    def _pad_each(x):
        """(x padded at the bottom and the right to multiples of 64 by replicating its edge, (N, h, w, H, W))."""
        if x.dim() != 4 or min(x.shape) < 1:
            raise ValueError(f"compress_each: image batch {tuple(x.shape)} must be (N, C, h, w) with h, w >= 1")
        N, _, h, w = x.shape
        H, W = _codec.padded_size(h, w)
        if (H, W) != (h, w):
            _lib.require_device(x)
            x = _lib.stream_ops().pad_edge(x.contiguous(), H, W)
        return x, (N, h, w, H, W)

    @torch.no_grad()
    def compress_each(self, x, steps_per_chunk=1024):
        """x (N, 3, h, w) in [0, 1], any h, w >= 1 -> a list of N bytes objects, one stream per image."""
        self._codable_each()
        em, cm = self.entropy_model, self.conditional_model
        x, (N, h, w, H, W) = self._pad_each(x)
        y, z, z_sym, kz, (sigma, mean) = self._analyse(x, each=True)
        y_sym, ky = self._symbols(self._latent_gain(y), mean, each=True)
        sz = em.encode_symbols_seg(z_sym, kz, steps_per_chunk)
        sy = cm.encode_symbols_seg(y_sym, ky, sigma.expand_as(y), steps_per_chunk, mean=mean)
        return [self._pack_image(self._header(1, H, W, y, z, steps_per_chunk, kz[n], ky[n], (h, w), n),
                                 sz[n][1], sy[n][1], sz[n][0], sy[n][0]) for n in range(N)]

    @torch.no_grad()
    def decompress_each(self, streams):
        """A list of M bytes objects from `compress_each` (any sizes, coded in any calls; same weights, build,
        COMPUTE_DTYPE and device type) -> a list of M tensors (1, 3, h_m, w_m).  Streams that share a padded
        size and chunk size are decoded by the same launches and pass g_s as one batch."""
        self._codable_each()
        em, cm = self.entropy_model, self.conditional_model
        parsed = [self._parse_image(d, *self._build_id()) for d in streams]   # everything is validated before any launch
        groups = {}
        for m, (h, *_rest) in enumerate(parsed):
            self._check_stream(h, "decompress_each", f"stream {m}")
            groups.setdefault((h.H, h.W, h.latent_channels, h.R), []).append(m)
        out = [None] * len(parsed)
        for (H, W, _cy, R), idx in groups.items():
            hs = [parsed[m][0] for m in idx]
            self._begin_decode(hs)
            z_hat = em.decompress_seg([parsed[m][3] for m in idx], hs[0].z_shape, [parsed[m][1] for m in idx],
                                      [h.kmax_z for h in hs], R)
            sigma, mean = self._prior_each(self._hyper_ungain(z_hat))
            if tuple(sigma.shape[1:]) != hs[0].y_shape[1:]:
                raise ValueError(f"decompress_each: the model's sigma {tuple(sigma.shape)} is not the streams' latent "
                                 f"shape {hs[0].y_shape}")
            y_hat = self._latent_ungain(cm.decompress_seg([parsed[m][4] for m in idx], sigma, [parsed[m][2] for m in idx],
                                                          [h.kmax_y for h in hs], R, mean=mean))
            for m, img in zip(idx, self._reconstruct_each(y_hat, hs)):
                out[m] = img
        return out

    # ---- layered per-image streams: y coded in channel layers, any prefix that holds the tables decodes (containers
    # "ICRL" / "ICRH"; codec.py states the rule).  A layer is a segment of the segmented coder; a layer that has not
    # arrived reconstructs as mu, the hyperprior's own prediction.
    layered_refusal = None    # a model whose y is not one bitstream under (sigma, mu) = h_s(z_hat) says why here
    _layered_containers = (_codec.pack_layered_image, _codec.parse_layered_image, _codec.LayeredImageHeader)

    def _check_layered(self, who):
        if self.layered_refusal:
            raise ValueError(f"{who}: {self.layered_refusal}")
        self._codable_each()

    @torch.no_grad()
    def compress_each_layered(self, x, layers=8, order="energy", steps_per_chunk=1024):
        """x (N, 3, h, w) in [0, 1], any h, w >= 1 -> a list of N bytes objects, one layered stream per image: the
        symbols of `compress_each`, y's channels in `layers` layers, each a bitstream of its own behind all tables, so
        that `decompress_each_layered` reads any prefix that holds the tables (codec.py: "Layered per-image
        containers").  order: "energy" (the channels by descending sum of symbol^2, per image: a steering heuristic
        that the decoder reads from the stream, never recomputes), "identity", or an integer array (C,) or (N, C)."""
        who = "compress_each_layered"
        self._check_layered(who)
        em, cm = self.entropy_model, self.conditional_model
        C, G = self._latent_channels, layers
        if isinstance(G, bool) or not isinstance(G, (int, np.integer)) or not 1 <= G <= C or C % G:
            raise ValueError(f"{who}: layers is an integer in [1, {C}] that divides the {C} latent channels, got {G!r}")
        G = int(G)
        if x.dim() == 4 and x.shape[0] * G > 65535:
            raise ValueError(f"{who}: {x.shape[0]} images in {G} layers are more than 65535 segments")
        energy = isinstance(order, str) and order == "energy"
        if not energy and x.dim() == 4:
            try:
                orders = _codec.layer_orders(order, x.shape[0], C)     # in front of any launch
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
        pack, _parse, header = self._layered_containers
        x, (N, h, w, H, W) = self._pad_each(x)
        y, z, z_sym, kz, (sigma, mean) = self._analyse(x, each=True)
        y_sym, ky = self._symbols(self._latent_gain(y), mean, each=True)
        if y.shape[1] != C:
            raise ValueError(f"{who}: the latent has {y.shape[1]} channels, the model's configuration says {C}")
        P = y.shape[2] * y.shape[3]
        sym = y_sym.view(N, P, C)
        ops = _lib.layer_ops()
        if energy:
            orders = _codec.layer_order(ops.energy(sym).cpu().numpy())    # the one small copy: (N, C) integers
        flat_order = orders.reshape(-1).tolist()
        seg = [v for n in range(N) for g in range(G) for v in (n, g)]
        rows = cm.scale_rows(sigma.expand_as(y)).view(N, P, C)
        sz = em.encode_symbols_seg(z_sym, kz, steps_per_chunk)
        sy = _encode_seg(ops.gather(sym, G, flat_order, seg), N * G, ops.gather(rows, G, flat_order, seg), 0,
                         lambda K: cm.tables(K, y.device), [k for k in ky for _ in range(G)], steps_per_chunk)
        out = []
        for n in range(N):
            hd = header(**vars(self._header(1, H, W, y, z, steps_per_chunk, kz[n], ky[n], (h, w), n)), layers=G,
                        order=orders[n].copy())
            mine = sy[n * G:(n + 1) * G]
            out.append(pack(hd, sz[n][1], [l for _, l in mine], sz[n][0], [p for p, _ in mine],
                            version=self._image_format_version()))
        return out

    def _layered_latents(self, streams, layers, who):
        """Parses and checks everything, then for every group of streams that share (H, W, C, R, G) yields
        ([m], their headers, the coded-domain latent (len([m]), C, Hy, Wy) in front of `_latent_ungain`), with
        `_begin_decode` done for the group: the caller finishes a group before it asks for the next."""
        self._check_layered(who)
        em, cm = self.entropy_model, self.conditional_model
        if isinstance(streams, (bytes, bytearray, memoryview, str)):
            raise ValueError(f"{who}: `streams` is a list of layered streams, not one {type(streams).__name__}")
        streams = list(streams)
        caps = list(layers) if isinstance(layers, (list, tuple, np.ndarray)) else [layers] * len(streams)
        if len(caps) != len(streams):
            raise ValueError(f"{who}: {len(caps)} layer counts for {len(streams)} streams")
        for cap in caps:
            if cap is not None and (isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0):
                raise ValueError(f"{who}: layers is None or an integer >= 0 (one for all streams or one each), got {cap!r}")
        parse = self._layered_containers[1]
        parsed, held, groups = [], [], {}
        for m, d in enumerate(streams):     # everything is validated before any launch
            parsed.append(parse(d, *self._build_id(), version=self._image_format_version(), prefix=True))
            h = parsed[-1][0]
            self._check_stream(h, who, f"stream {m}")
            held.append(len(parsed[-1][4]) if caps[m] is None else min(len(parsed[-1][4]), int(caps[m])))
            groups.setdefault((h.H, h.W, h.latent_channels, h.R, h.layers), []).append(m)
        for idx in groups.values():
            if sum(held[m] for m in idx) > 65535:
                raise ValueError(f"{who}: {sum(held[m] for m in idx)} layers of one shape are more than 65535 segments")
        ops = _lib.layer_ops()
        for (_H, _W, C, R, G), idx in groups.items():
            hs = [parsed[m][0] for m in idx]
            self._begin_decode(hs)
            z_hat = em.decompress_seg([parsed[m][3] for m in idx], hs[0].z_shape, [parsed[m][1] for m in idx],
                                      [h.kmax_z for h in hs], R)
            sigma, mean = self._prior_each(self._hyper_ungain(z_hat))
            if tuple(sigma.shape[1:]) != hs[0].y_shape[1:]:
                raise ValueError(f"{who}: the model's sigma {tuple(sigma.shape)} is not the streams' latent shape "
                                 f"{hs[0].y_shape}")
            n, (_, _, Hy, Wy) = len(idx), hs[0].y_shape
            P, Cg = Hy * Wy, C // G
            flat_order = np.concatenate([h.order for h in hs]).tolist()
            nl = [held[m] for m in idx]
            seg = [v for k in range(n) for g in range(nl[k]) for v in (k, g)]
            if seg:
                rows = ops.gather(cm.scale_rows(sigma).view(n, P, C), G, flat_order, seg)
                q = _decode_seg([parsed[m][4][g] for k, m in enumerate(idx) for g in range(nl[k])],
                                [parsed[m][2][g] for k, m in enumerate(idx) for g in range(nl[k])], P * Cg, rows, 0,
                                lambda K: cm.tables(K, sigma.device), [h.kmax_y for k, h in enumerate(hs) for _ in range(nl[k])],
                                R, sigma.device)
            else:
                q = torch.empty(0, dtype=torch.float32, device=sigma.device)
            mu = None if mean is None else _to_last(mean).view(n, P, C)
            flat = ops.scatter(q, mu, n, P, C, G, flat_order, nl)
            yield idx, hs, symbols_as_tensor(flat.view(-1), (n, C, Hy, Wy))

    @torch.no_grad()
    def decompress_each_layered(self, streams, layers=None):
        """A list of M layered streams from `compress_each_layered`, each whole or any prefix that holds its tables
        (`codec.layer_ends(data)[0]` bytes at least) -> a list of M tensors (1, 3, h_m, w_m).  A stream decodes from
        the whole layers its bytes hold, at most `layers` of them (None: all; an int, or one per stream); the channels
        of every other layer reconstruct as mu, the hyperprior's prediction (+0.0 on the scale hyperprior), and
        `layers=0` is the hyperprior's own picture of the image.  Everything is parsed and checked before any launch;
        streams that share a padded size, a chunk size and a layer count pass the same launches, whatever each
        holds.  The quality of the prefixes comes from the layer order, a heuristic measured on untrained weights."""
        out = {}
        for idx, hs, y_hat in self._layered_latents(streams, layers, "decompress_each_layered"):
            for m, img in zip(idx, self._reconstruct_each(self._latent_ungain(y_hat), hs)):
                out[m] = img
        return [out[m] for m in range(len(out))]

    # ---- a pixel window of a per-image stream: only the chunks that hold its latent rows are decoded and g_s runs on the
    # latent window alone (codec.py states the plan).  The streams are `compress_each`'s, unchanged.
    window_refusal = None    # a model whose streams do not map a band of latent rows to a chunk range says why here

    def _begin_window_decode(self, hs, plans):
        """`_begin_decode` for a group of latent windows, one header and one plan per window: what `_latent_ungain`
        needs to act on the windows."""
        self._begin_decode(hs)

    @torch.no_grad()
    def _window_latents(self, streams, boxes):
        """(plans, groups): the WindowPlan of every box and, per group of windows that share a latent shape and a
        chunk size, ([m], what g_s reads for them, (len([m]), C, rh, rw)).  Everything is parsed and planned
        before any launch; a bytes object given more than once is parsed, z-decoded and passed through h_s once."""
        who = "decompress_window"
        if self.window_refusal:
            raise ValueError(f"{who}: {self.window_refusal}")
        self._codable_each()
        em, cm = self.entropy_model, self.conditional_model
        streams, boxes = list(streams), list(boxes)
        if len(streams) != len(boxes):
            raise ValueError(f"{who}: {len(streams)} streams for {len(boxes)} boxes")
        kernel, strides = self._synthesis_geometry
        parsed, owner, seen = [], [], {}
        for m, d in enumerate(streams):
            if id(d) not in seen:     # the same object, not an equal one: `streams` keeps every object alive
                seen[id(d)] = len(parsed)
                parsed.append(self._parse_image(d, *self._build_id()))
                self._check_stream(parsed[-1][0], who, f"stream {m}")
            owner.append(seen[id(d)])
        plans = []
        for m, s in enumerate(owner):
            h, lz, ly = parsed[s][:3]
            try:
                plans.append(_codec.window_plan(h, boxes[m], kernel, strides, lengths=(lz, ly)))
            except ValueError as e:
                raise ValueError(f"{who}: box {m}: {e}") from None
        # per distinct stream: z whole, h_s on the whole z at batch shape 1 (its sigma bits select the table rows)
        prior = []
        for h, lz, _ly, pz, _py in parsed:
            self._begin_decode([h])
            z_hat = em.decompress_seg([pz], h.z_shape, [lz], [h.kmax_z], h.R)
            sigma, mean = self._prior_each(self._hyper_ungain(z_hat))
            if tuple(sigma.shape) != h.y_shape:
                raise ValueError(f"{who}: the model's sigma {tuple(sigma.shape)} is not the stream's latent shape "
                                 f"{h.y_shape}")
            prior.append((cm.scale_rows(sigma), None if mean is None else _to_last(mean).reshape(-1)))
        groups = {}
        for m, s in enumerate(owner):
            groups.setdefault((*plans[m].shape, parsed[s][0].latent_channels, parsed[s][0].R), []).append(m)
        out = []
        for (rh, rw, C, R), idx in groups.items():
            hs = [parsed[owner[m]][0] for m in idx]
            used = sorted({owner[m] for m in idx})
            base, at = {}, 0
            for s in used:     # the rows (and the means) of the group's streams back to back
                base[s] = at
                at += prior[s][0].numel()
            rows = prior[used[0]][0] if len(used) == 1 else torch.cat([prior[s][0] for s in used])
            mu = None
            if prior[used[0]][1] is not None:
                mu = prior[used[0]][1] if len(used) == 1 else torch.cat([prior[s][1] for s in used])
            pool, nrows, ks, offs = table_pool(lambda K: cm.tables(K, rows.device), [h.kmax_y for h in hs])
            # the payload of the spanned chunks alone, a chunk range that several windows share once
            parts, where, words, windows, spans = [], {}, 0, [], []
            ends_of = {s: np.concatenate(([0], np.cumsum(parsed[s][2], dtype=np.int64))) for s in used}
            for m, h, K, off in zip(idx, hs, ks, offs):
                s, (k0, k1) = owner[m], plans[m].chunks
                ends = ends_of[s]
                if (s, k0, k1) not in where:
                    where[s, k0, k1] = words
                    parts.append(parsed[s][4][int(ends[k0]):int(ends[k1])])
                    words += len(parts[-1]) // 2
                first = where[s, k0, k1] - int(ends[k0]) // 2
                spans += [first + int(e) // 2 for k in range(k0, k1) for e in (ends[k], ends[k + 1])]
                _, _, Hy, Wy = h.y_shape
                windows += [base[s], off, Hy, Wy, K, plans[m].rows[0], plans[m].cols[0], k0, k1]
            buf = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to(rows.device)
            flat = _lib.window_ops().decode(buf, windows, rh, rw, spans, rows, mu, C, pool, nrows, R)
            self._begin_window_decode(hs, [plans[m] for m in idx])
            out.append((idx, self._latent_ungain(symbols_as_tensor(flat, (len(idx), C, rh, rw)))))
        return plans, out

    @torch.no_grad()
    def decompress_window(self, streams, boxes):
        """streams[m]: bytes from `compress_each`, `compress_each_to` or `compress_each_refined`, unchanged;
        boxes[m] = (top, left, height, width) in pixels of that image -> a list of tensors (1, 3, height_m, width_m):
        the box of what `decompress_each` returns for the stream, up to the arithmetic's rounding (g_s runs on another
        shape), from the chunks of y that hold the box's latent rows and g_s on the latent window alone.  z and h_s are
        decoded and run whole, once per bytes object: give the tiles of one image the same object.  Windows that
        share a latent shape and a chunk size are decoded by one launch and pass g_s as one batch."""
        plans, groups = self._window_latents(streams, boxes)
        out = [None] * len(plans)
        for idx, y_hat in groups:
            x = self.synthesis_transform(y_hat)
            for k, m in enumerate(idx):
                _, _, height, width = plans[m].box
                out[m] = _lib.window_ops().crop_clamp_at(x[k:k + 1], *plans[m].crop, height, width)
        return out

    # ---- transcoding in the latent domain: a stream to another stream of this model without g_a or g_s (codec.py states
    # the rules).  Re-chunking here; the gained model adds requantization to another quality and to a byte budget.
    transcode_refusal = None    # a model whose streams are not one bitstream of z and one of y says why here

    def _transcode_qualities(self, qualities, M, who):
        """The float32 target quality of every one of M streams; here a refusal: this model codes at one rate."""
        raise ValueError(f"{who}: {type(self).__name__} codes at one rate: `qualities` needs the gain units of "
                         "GainedMeanScaleCompressor2018; leave it None to re-chunk")

    def _transcode_parse(self, streams, steps_per_chunk, who, qualities=None):
        """(streams as a list, [(header, lens_z, lens_y, payload_z, payload_y)], the target qualities or None): every
        refusal and every check of the arguments and the streams, in front of any launch."""
        if self.transcode_refusal:
            raise ValueError(f"{who}: {self.transcode_refusal}")
        self._codable_each()
        if isinstance(streams, (bytes, bytearray, memoryview, str)):
            raise ValueError(f"{who}: `streams` is a list of per-image streams, not one {type(streams).__name__}")
        streams = list(streams)
        R = steps_per_chunk
        if R is not None and (isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= _codec.MAX_STEPS):
            raise ValueError(f"{who}: steps_per_chunk is None or an integer in [1, {_codec.MAX_STEPS}], got {R!r}")
        targets = None if qualities is None else self._transcode_qualities(qualities, len(streams), who)
        parsed = []
        for m, d in enumerate(streams):
            parsed.append(self._parse_image(d, *self._build_id()))
            self._check_stream(parsed[-1][0], who, f"stream {m}")
        return streams, parsed, targets

    def _transcode_decode_z(self, parsed, idx):
        """(the decoded integers of z, what h_s reads, its `_prior_each`) for the streams `idx`, which share a padded
        size and a chunk size; `_begin_decode` has run for them."""
        hs = [parsed[m][0] for m in idx]
        k_z = self.entropy_model.decompress_seg([parsed[m][3] for m in idx], hs[0].z_shape, [parsed[m][1] for m in idx],
                                                [h.kmax_z for h in hs], hs[0].R)
        z_hat = self._hyper_ungain(k_z)
        sigma, mean = self._prior_each(z_hat)
        if tuple(sigma.shape[1:]) != hs[0].y_shape[1:]:
            raise ValueError(f"transcode_each: the model's sigma {tuple(sigma.shape)} is not the streams' latent shape "
                             f"{hs[0].y_shape}")
        return k_z, z_hat, sigma, mean

    def _transcode_decode_y(self, parsed, idx, rows):
        """The decoded integers of y of the streams `idx`, flat floats in (n, *, c) order: the residual where the
        model codes y about a mean, which is not added."""
        hs = [parsed[m][0] for m in idx]
        cm = self.conditional_model
        return _decode_seg([parsed[m][4] for m in idx], [parsed[m][2] for m in idx], hs[0].nsym_y, rows, 0,
                           lambda K: cm.tables(K, rows.device), [h.kmax_y for h in hs], hs[0].R, rows.device)

    def _rechunk_group(self, parsed, idx, R):
        """The streams `idx` (one padded size, one chunk size) coded again at R steps per chunk: their symbols, the
        rows of their sigma computed once, and their headers with R replaced."""
        em, cm = self.entropy_model, self.conditional_model
        hs = [parsed[m][0] for m in idx]
        self._begin_decode(hs)
        k_z, _z_hat, sigma, _mean = self._transcode_decode_z(parsed, idx)
        rows = cm.scale_rows(sigma)
        k_y = self._transcode_decode_y(parsed, idx, rows)
        sz = em.encode_symbols_seg(_to_last(k_z).reshape(-1).to(torch.int32), [h.kmax_z for h in hs], R)
        sy = _encode_seg(k_y.to(torch.int32), len(idx), rows, 0, lambda K: cm.tables(K, rows.device),
                         [h.kmax_y for h in hs], R)
        return [self._pack_image(_codec.transcoded_header(h, R=int(R)), sz[k][1], sy[k][1], sz[k][0], sy[k][0])
                for k, h in enumerate(hs)]

    def _transcode_groups(self, parsed, todo):
        """{(H, W, latent channels, R): [m]} of the streams `todo`, as `decompress_each` groups them."""
        groups = {}
        for m in todo:
            h = parsed[m][0]
            groups.setdefault((h.H, h.W, h.latent_channels, h.R), []).append(m)
        return groups

    @torch.no_grad()
    def transcode_each(self, streams, qualities=None, steps_per_chunk=None):
        """A list of M per-image streams of this model (any sizes, coded in any calls) -> a list of M streams, without
        g_a, g_s or a pixel: the rules are codec.py's.  Eval mode only.

        steps_per_chunk: None keeps every stream's own R; an int in [1, codec.MAX_STEPS] writes every output at that R.
        qualities None is re-chunking only: the symbols of z and of y are decoded and coded again, the header is the
        parsed one with R replaced, and the result is byte for byte what `compress_each` writes at that R.  A stream
        that already has the target R is returned as the same object, with no launch for it.
        qualities given (one float, or M of them) requantizes every stream to that quality: on
        GainedMeanScaleCompressor2018 only (ValueError here).  `decompress_each` and `decompress_window` read the
        results as they read any stream.  Everything is parsed, checked and planned before any launch; streams that
        share a padded size and a chunk size go through the same launches."""
        who = "transcode_each"
        streams, parsed, targets = self._transcode_parse(streams, steps_per_chunk, who, qualities)
        out = list(streams)
        requant = [] if targets is None else [m for m, p in enumerate(parsed) if targets[m] != p[0].quality]
        moved = set(requant)
        rechunk = [m for m, p in enumerate(parsed)
                   if steps_per_chunk is not None and p[0].R != steps_per_chunk and m not in moved]
        try:
            for idx in self._transcode_groups(parsed, rechunk).values():
                for m, s in zip(idx, self._rechunk_group(parsed, idx, steps_per_chunk)):
                    out[m] = s
            for (_H, _W, _C, R), idx in self._transcode_groups(parsed, requant).items():
                res = self._requant_group(parsed, idx, [targets[m] for m in idx], steps_per_chunk or R, who)
                for m, s in zip(idx, res):
                    out[m] = s
        finally:
            self._end_call()
        return out

    # ---- encode-time latent refinement: lower R + lambda D for this image, same decoder (codec.py states the rule)
    refine_refusal = None    # a model whose streams the rule does not cover says why here

    def _refine_weights(self, N):
        """[lambda_n]: the distortion weight of every image of a `compress_each_refined` call (after `_analyse`)."""
        return [float(self.distortion_loss_weight)] * N

    def _check_refine(self, steps, lr):
        """The refusals of `compress_each_refined`, in front of any launch."""
        who = "compress_each_refined"
        if self.refine_refusal:
            raise ValueError(f"{who}: {self.refine_refusal}")
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
            raise ValueError(f"{who}: steps is an integer >= 0, got {steps!r}")
        if isinstance(lr, bool) or not isinstance(lr, Real) or not math.isfinite(lr) or not lr > 0:
            raise ValueError(f"{who}: lr is a finite positive number, got {lr!r}")
        if list(self.distortion_loss_fns) != ["MSE"]:
            raise ValueError(f"{who}: the objective is R + lambda MSE; this model's distortion is "
                             f"{list(self.distortion_loss_fns)}")

    def compress_each_refined(self, x, steps=8, lr=0.1, steps_per_chunk=1024):
        """x (N, 3, h, w) in [0, 1], any h, w >= 1 -> (a list of N streams as `compress_each` writes them, a
        RefineReport): every image coded with the integers of y that gave it the lowest J = R + lambda D among the
        unrefined latent and `steps` Adam steps (learning rate `lr`) on the image's own objective.  The decoder's
        inputs (the weights, the hyper-latent and so sigma and mu) are untouched: `decompress_each` reads the streams
        as any other, and steps = 0 gives `compress_each`'s bytes.  J_after <= J_before for every image.  The defaults
        come from an experiment on untrained weights; they are not validated on trained ones.

        The rule (codec.py has the whole of it).  In the coded domain v0 = `_latent_gain(y)`:
          Evaluate(v): s = symbol_of(v - mu), y_hat = float(s) + mu, x_hat = `_reconstruct(_latent_ungain(y_hat))`,
            D_n the squared error over the padded image, B_n the rate terms of the conditional likelihood of y_hat
            under (sigma, mu), J_n = B_n + w_n D_n with w_n = lambda_n / x.shape[1];
          Gradient: d(sum w_n D_n) / d y_hat, straight through the rounding, plus d(rate at the unrounded v) / dv;
          Update: Adam on v (beta 0.9 / 0.999, eps 1e-8, bias corrections from the host; csrc/refine.hip);
          Keep-best: evaluation t replaces image n's kept symbols iff J_n(t) < best_n (strict, a NaN never wins).

        The loop runs g_s forward and its input-gradient backward and no weight-gradient kernel: every parameter has
        requires_grad off for the duration, and it and every .grad are afterwards what they were.  The whole loop is
        enqueued without a copy to the host or a wait; the one copy, after the last evaluation, brings the N maxima
        of the kept symbols and the report."""
        from ..layers.gdn import NonNegativeParam
        who = "compress_each_refined"
        self._check_refine(steps, lr)
        self._codable_each()
        em, cm, T, R = self.entropy_model, self.conditional_model, int(steps), steps_per_chunk
        params = list(self.parameters())
        flags = [p.requires_grad for p in params]
        try:
            for p in params:
                p.requires_grad_(False)
            with torch.no_grad():
                x, (N, h, w, H, W) = self._pad_each(x)
                x = x.contiguous()
                y, z, z_sym, kz, (sigma, mean) = self._analyse(x, each=True)
                v0 = self._latent_gain(y)
                shape = tuple(v0.shape)
                v = _to_last(v0)
                if v.data_ptr() == v0.data_ptr():
                    v = v.clone()                    # stepped in place: never the model's own tensor
                logical = symbols_as_tensor(v, shape)
                sigma = _match(sigma.expand_as(logical), logical)
                mean = None if mean is None else _match(mean.expand_as(logical), logical)
                mu = None if mean is None else _to_last(mean)
                m, u = torch.zeros_like(v), torch.zeros_like(v)
                wts = torch.tensor([lam / x.shape[1] for lam in self._refine_weights(N)], dtype=torch.float64).to(x.device)
                best = torch.full((3, N), float("inf"), dtype=torch.float64, device=x.device)
                best_step = torch.zeros(N, dtype=torch.int32, device=x.device)
                one = torch.ones((), device=x.device)
                gdns = [mod for mod in self.synthesis_transform.modules() if isinstance(mod, NonNegativeParam)]
                pre = [NonNegFn.apply(mod.param, float(mod.bound), float(mod.pedestal)) for mod in gdns]
            y_shift = (_codec.MAP_BLOCK // _codec.Y_DOWN).bit_length() - 1
            first = best_sym = g = None
            for t in range(T + 1):
                with torch.no_grad():
                    if t == 0:
                        sym, y_hat = refine_update(v, None, None, None, mu)
                    else:
                        sym, y_hat = refine_update(v, m, u, _to_last(g), mu, lr, 1.0 / (1.0 - 0.9 ** t),
                                                   1.0 / (1.0 - 0.999 ** t))
                    y_hat = symbols_as_tensor(y_hat, shape)
                for mod, val in zip(gdns, pre):       # g_s's GDN parameters, re-parameterised once for the call
                    mod.__dict__["_pre"] = val
                with torch.set_grad_enabled(t < T):
                    if t < T:
                        leaf = symbols_as_tensor(v, shape).detach().requires_grad_(True)
                        y_hat = RoundThroughFn.apply(leaf, y_hat)
                    x_hat = self._reconstruct(self._latent_ungain(y_hat))
                    if t < T:
                        rate = CELossFn.apply(conditional_likelihood(leaf, sigma, mean, cm.KIND, cm.bin))
                with torch.no_grad():
                    p = conditional_likelihood(y_hat.detach(), sigma, mean, cm.KIND, cm.bin)
                    xd = x_hat.detach().contiguous()
                    obj = refine_objective(block_bits(p, y_shift), block_sse(x, xd, _codec.MAP_BLOCK.bit_length() - 1), wts)
                    if t == 0:
                        # the unrefined latent, `compress_each`'s symbols: kept even where its J is a NaN
                        first, best_sym = obj, sym.clone()
                    refine_keep(sym, best_sym, obj, best, best_step, t)
                    if t < T:
                        gx = refine_dist_grad(x, xd, wts)
                if t < T:
                    g, = torch.autograd.grad([x_hat, rate], [leaf], [gx, one])
                    del leaf, rate
                del x_hat
            with torch.no_grad():
                kd = refine_kmax(best_sym, N)
                # the one copy to the host: the report and the N maxima
                out = torch.cat([first.reshape(-1), best.reshape(-1), best_step.double(), kd.double()]).cpu().numpy()
                ky = [int(k) for k in out[7 * N:]]
                for n, k in enumerate(ky):
                    if k > _codec.KMAX_LIMIT:
                        raise ValueError(f"{who}: image {n} has a symbol of magnitude {k}, which exceeds the coder's "
                                         f"limit of {_codec.KMAX_LIMIT}")
                sz = em.encode_symbols_seg(z_sym, kz, R)
                sy = cm.encode_symbols_seg(best_sym, ky, sigma, R, mean=mean)
                streams = [self._pack_image(self._header(1, H, W, y, z, R, kz[n], ky[n], (h, w), n),
                                            sz[n][1], sy[n][1], sz[n][0], sy[n][0]) for n in range(N)]
        finally:
            for p, f in zip(params, flags):
                p.requires_grad_(f)
            self._clear_reparameterised()
            self._end_call()
        rows = [[float(a) for a in out[k * N:(k + 1) * N]] for k in range(6)]
        return streams, RefineReport(before=rows[2], after=rows[5], bits_before=rows[0], bits_after=rows[3],
                                     sse_before=rows[1], sse_after=rows[4], step=[int(a) for a in out[6 * N:7 * N]])

    # ---- rate and distortion maps: where the bits go and where the error is, block by block, from one eval pass
    def _check_call(self, N, H, W, who):
        """What a call on N images of padded size H x W needs of the model's settings (its arithmetic, its quality or
        quality map), checked in front of any launch."""

    def _begin_call(self, N, H, W, device, who):
        """The state the gain hooks read during a call outside `forward`; `_end_call` drops it."""

    def _end_call(self):
        pass

    def rate_distortion_map(self, x, likelihoods=False):
        """The estimated bits and the squared error of every 64 x 64 pixel block (codec.MAP_BLOCK: one position of z,
        4 x 4 of y -- the shape of a quality map) of x (N, 3, h, w), any h, w >= 1, from one eval pass with no coder
        in the loop -> RDMap.

        Eval mode only, under no_grad, on the current stream, always the serial route of the forward.  An image whose
        size is no multiple of 64 is padded by the per-image streams' rule (edge replication) and its reconstruction
        cropped and clamped as theirs is; at a multiple of 64 neither kernel runs and `x_hat` is `model(x)[0]` bit
        for bit.  The quality is the forward's: `set_quality`, or the map of `set_quality_map` (checked against the
        padded size in front of any launch).

        This is an estimate of the eval forward, not of a stream: the bits are -log2 of the likelihoods the forward
        scores (clamped as its loss clamps them), not a coder's output, and sigma (and the mean) come from the batch
        as the forward computes them, not image by image as `compress_each` does."""
        who = "rate_distortion_map"
        if self.training:
            raise RuntimeError(f"{who} runs in eval mode only: call model.eval() first")
        if x.dim() != 4 or min(x.shape) < 1:
            raise ValueError(f"{who}: image batch {tuple(x.shape)} must be (N, C, h, w) with h, w >= 1")
        N, _, h, w = x.shape
        H, W = _codec.padded_size(h, w)
        self._check_call(N, H, W, who)
        self._clear_reparameterised()
        with torch.no_grad():
            xp = x
            if (H, W) != (h, w):
                _lib.require_device(x)
                xp = _lib.stream_ops().pad_edge(x.contiguous(), H, W)
            try:
                self._begin_call(N, H, W, x.device, who)
                y = self.analysis_transform(xp)
                return self._rate_distortion_from(x, y, self.prior_analysis(self._hyper_input(y)), likelihoods)
            finally:
                self._end_call()

    def _rate_distortion_from(self, x, y, z, likelihoods=False):
        """The RDMap of `rate_distortion_map` from y = g_a(padded x) and z = h_a(y) as they come out of the transforms,
        neither of which depends on the quality: the rest of the eval pass and the four map kernels, under the gain
        state the caller has set up (`_begin_call`).  x is the unpadded batch."""
        h, w = x.shape[2:]
        H, W = _codec.padded_size(h, w)
        y_shift, z_shift = ((_codec.MAP_BLOCK // d).bit_length() - 1 for d in (_codec.Y_DOWN, _codec.Z_DOWN))
        em = self.entropy_model
        z = self._hyper_gain(z)
        # the factorized model's (rint(z), p_z) without its loss: p_z in z's own logical shape
        z_hat, p_z = factorized(z, em._cdf_estimator.flat_params(), False, None, em._cdf_estimator.dims, em.bin)
        y_hat, p_y = self._forward_y(self._latent_gain(y), *self._prior(self._hyper_ungain(z_hat)))
        if (H, W) == (h, w):
            x_hat = self._reconstruct(self._latent_ungain(y_hat))
        else:
            x_hat = _lib.stream_ops().crop_clamp(self.synthesis_transform(self._latent_ungain(y_hat)), h, w)
        bits_y = block_bits(p_y, y_shift)
        bits_z = block_bits(p_z, z_shift)
        bits = block_bits(p_z, z_shift, add=bits_y)
        sse = block_sse(x, x_hat, (_codec.MAP_BLOCK).bit_length() - 1)
        return RDMap(bits_y, bits_z, bits, sse, block_pixels(h, w), x_hat, *((p_y, p_z) if likelihoods else ()))

    def _reconstruct_each(self, y_hat, hs):
        """[x_hat of image k, (1, 3, h_k, w_k)] from the latents of a group of streams that share one padded size, and
        their headers: g_s on the group as one batch, then each image cropped to its own size and clamped."""
        sizes = [(h.height, h.width) for h in hs]
        if set(sizes) == {(hs[0].H, hs[0].W)}:
            x_hat = self._reconstruct(y_hat).contiguous()
            return [x_hat[k:k + 1] for k in range(len(hs))]
        return self._reconstruct(y_hat, sizes)
