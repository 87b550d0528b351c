"""CheckerboardCompressor2018 -- MeanScaleCompressor2018 with the checkerboard context model of He et al. 2021
("Checkerboard Context Model for Efficient Learned Image Compression"): the context model of Minnen et al. 2018 in
a form that decodes in two parallel passes instead of one serial scan.

Position (i, j) of the latent map is an anchor when i + j is even.  The anchors are coded from the hyperprior
alone, (sigma_h, mu_h) = h_s(z_hat); every non-anchor is coded with parameters that also depend on the decoded
anchors in the 5 x 5 window around it (`_context`):
    u, v = anchors of y_hat, anchors of |y_hat - mu_h|          (+0.0 at the non-anchors)
    mu    = mu_h + context_mean(u)                              at the non-anchors, mu_h at the anchors
    sigma = sigma_h * exp(clamp(context_scale(v), -4, 4))       at the non-anchors, sigma_h at the anchors
Both heads are single linear 5 x 5 convs: the mean is predicted from the neighbours' values, the log-scale from
the magnitudes of their residuals.  Their weights and biases start at zero, so a freshly built model is exactly the
mean-scale model (and a mean-scale checkpoint, loaded with strict=False, is a converted model: the four missing
tensors are the zero context, which changes nothing) and the context is learnt from there.

No weight mask.  The usual checkerboard convolution masks the 13 of 25 taps (di, dj) with di + dj even, which read
a non-anchor from a non-anchor.  Here those taps contribute exactly 0 to every value that is used, because u and v
are zero at the non-anchors and the convs' outputs at the anchors are discarded; and they receive a gradient of
exactly 0, because in every product of their weight gradient either the output gradient (an anchor output) or the
input (a non-anchor input) is zero.  So they stay at their initial zero without being masked.  (They still cost
their multiply-adds)

Decodability: the contract of Compressor2018.decompress (same weights, build, COMPUTE_DTYPE, device type and batch
shape) and nothing more.  The two sides agree bit for bit on the non-anchors' (sigma, mu) because the decoder's
`add_mean` is `center_round`'s addition, so u and v are identical at the anchors and +0.0 elsewhere on both sides,
and the convs are deterministic for a given shape, arithmetic and build.

MODEL.CONTEXT.KERNEL.  "conv" (the default) is everything above.  "fused" changes how the inference paths -- the eval
forward, `compress`, `decompress` -- compute `_context`: one kernel (functional.ckbd_context, csrc/ckbd_context.hip)
that evaluates the 12 live taps at the non-anchors only, in exact fp32 whatever COMPUTE_DTYPE is, and gives image n
the same bits whatever the batch around it.  The training forward keeps the convs (autograd lives there), the
parameters and the state dict are the same, so one checkpoint loads under either value.  Because the two routes round
differently, their batch streams are told apart by the "ICRC" format version (1: convs, 2: fused kernel), and each
model refuses the other's.  Because the fused context does not depend on the batch, a "fused" model also has
per-image streams (`compress_each` / `decompress_each`, container "ICRK"): h_s runs image by image as in every
model, the context once for the whole call."""
import torch
import torch.nn as nn

from ... import codec as _codec
from ...functional import conditional_likelihood
from ...functional import ckbd_context
from ..blocks.entropy_model import (_decode, _decode_seg, _encode, _encode_seg, add_mean, center_round, ckbd_gather,
                                    ckbd_input, ckbd_params, ckbd_scatter, symbolize_mean)
from ..layers import Conv2d
from .build import META_ARCH_REGISTRY
from .mshp2018 import MeanScaleCompressor2018


@META_ARCH_REGISTRY.register()
class CheckerboardCompressor2018(MeanScaleCompressor2018):
    """The mean-scale hyperprior plus two 5 x 5 context convs over the anchors (see the module docstring).  The
    convs carry no weight mask and need none: their inputs are zero at the non-anchors and their outputs at the
    anchors are discarded, so the 13 taps (di, dj) with di + dj even contribute exactly 0 to every value that is
    used and receive a gradient of exactly 0.  State dict: MeanScaleCompressor2018's plus
    context_mean.{weight,bias} and context_scale.{weight,bias}, all zero in a fresh model."""

    refine_refusal = ("CheckerboardCompressor2018 is not covered: the non-anchors' (sigma, mu) depend on y, so moving y "
                      "moves the decoder's inputs")
    layered_refusal = ("CheckerboardCompressor2018 is not covered: the non-anchors' (sigma, mu) come from the decoded "
                       "anchors of every channel, so a channel layer cannot be decoded, or left out, on its own")
    window_refusal = ("CheckerboardCompressor2018 is not covered: y is coded as two gathered halves, anchors and "
                      "non-anchors, so a band of latent rows is not a range of chunks, and the non-anchors' (sigma, mu) "
                      "need the anchors around them")
    transcode_refusal = ("CheckerboardCompressor2018 is not covered: its streams hold y as two bitstreams, anchors and "
                         "non-anchors, and the non-anchors' (sigma, mu) depend on the anchors as decoded")

    def __init__(self, cfg):
        super().__init__(cfg)
        # after every inherited module: their initial values are MeanScaleCompressor2018's from the same seed
        M = cfg.MODEL.LATENT_CHANNELS
        self.context_mean = Conv2d(M, M, 5, stride=1, padding=2)
        self.context_scale = Conv2d(M, M, 5, stride=1, padding=2)
        for conv in (self.context_mean, self.context_scale):
            nn.init.zeros_(conv.weight.data)
            nn.init.zeros_(conv.bias.data)
        # how the inference paths compute `_context`; no parameter or state-dict key depends on it
        self.context_kernel = cfg.MODEL.get("CONTEXT", {}).get("KERNEL", "conv")
        if self.context_kernel not in ("conv", "fused"):
            raise ValueError(f'MODEL.CONTEXT.KERNEL {self.context_kernel!r}: expected "conv" or "fused"')

    def _context(self, y_in, sigma_h, mu_h):
        """(sigma, mu) of every position from the hyperprior's (sigma_h, mu_h) and the anchors of y_in; the whole
        dependence on neighbours is here.  y_in's non-anchors are not read."""
        if self.context_kernel == "fused" and not self.training:
            cm, cs = self.context_mean, self.context_scale
            mu, sigma = ckbd_context(y_in, mu_h, sigma_h, cm.weight, cm.bias, cs.weight, cs.bias)
            return sigma, mu
        u, v = ckbd_input(y_in, mu_h)
        mu, sigma = ckbd_params(mu_h, sigma_h, self.context_mean(u), self.context_scale(v))
        return sigma, mu

    def _eval_params(self, y, sigma_h, mu_h):
        """(sigma, mu) as the decoder will hold them: the context of the anchors as decoded, rint(y - mu_h) + mu_h."""
        _, y_anchor = center_round(y, mu_h.expand_as(y))
        return self._context(y_anchor, sigma_h.expand_as(y), mu_h.expand_as(y))

    def _forward_y(self, y, sigma_h, mu_h):
        cm = self.conditional_model
        if self.training:
            y_tilde = cm.quantize(y)
            sigma, mu = self._context(y_tilde, sigma_h.expand_as(y), mu_h.expand_as(y))
            return y_tilde, conditional_likelihood(y_tilde, sigma, mu, cm.KIND, cm.bin)
        sigma, mu = self._eval_params(y, sigma_h, mu_h)
        r, y_tilde = center_round(y, mu)   # at the anchors mu is mu_h bit for bit: one call serves both halves
        return y_tilde, cm.likelihood(r, sigma)

    # ---- bitstreams: container "ICRC" (codec.py), y as two streams -- the anchors, then the non-anchors.  The format
    # version says which route computed the context, so a stream is only ever decoded by the arithmetic that coded it
    def _route(self):
        """What `pack_checkerboard` / `parse_checkerboard` take: the context's route (1 or 2) and whether h_s ran
        through the batch-invariant kernel."""
        fused = self.context_kernel == "fused"
        return dict(version=_codec.CKBD_FUSED_FORMAT_VERSION if fused else _codec.CKBD_FORMAT_VERSION,
                    invariant=self.hs_kernel == "invariant")

    def _format_version(self):
        """The number "ICRC" carries: 1 or 2 by the context's route; with h_s by the batch-invariant kernel, 3 or 4."""
        return _codec.checkerboard_version(**self._route())

    def _image_format_version(self):   # "ICRK" is "fused" only: its version says how h_s ran
        return (_codec.INVARIANT_FORMAT_VERSION if self.hs_kernel == "invariant"
                else _codec.CKBD_IMAGE_FORMAT_VERSION)

    def _pack(self, *parts):
        return _codec.pack_checkerboard(*parts, **self._route())

    def _parse(self, data, abi, compute_dtype):
        return _codec.parse_checkerboard(data, abi, compute_dtype, **self._route())

    def _codable_batch(self):
        self._codable_each()    # BIN == 1, before anything is computed

    def _encode_y(self, y, prior, steps_per_chunk):
        """The context of the anchors as the decoder will decode them, then each half of y as a stream of its own."""
        cm, shape = self.conditional_model, tuple(y.shape)
        sigma, mu = self._eval_params(y, *prior)
        y_sym, ky = symbolize_mean(y, mu)       # one K and one table set for both halves
        rows, tables = cm.scale_rows(sigma), cm.tables(ky, y.device)
        return ky, [_encode(ckbd_gather(y_sym, shape, p), ckbd_gather(rows, shape, p), 0, tables, steps_per_chunk)
                    for p in (0, 1)]

    def _decode_y(self, h, streams, prior):
        """Two passes: the anchors from the hyperprior, then the non-anchors from the hyperprior and the decoded
        anchors."""
        cm = self.conditional_model
        (pa, la), (pn, ln) = streams
        sigma_h, mu_h = prior
        dev, half = sigma_h.device, h.nsym_y // 2
        tables = cm.tables(h.kmax_y, dev)
        flat = torch.zeros(h.nsym_y, dtype=torch.float32, device=dev)
        # pass one: the anchors, coded under the hyperprior's own parameters
        rows = ckbd_gather(cm.scale_rows(sigma_h), h.y_shape, 0)
        ckbd_scatter(_decode(pa, la, half, rows, 0, tables, h.R, dev), flat, h.y_shape, 0)
        sigma, mu = self._context(add_mean(flat, mu_h), sigma_h, mu_h)
        # pass two: the non-anchors, under the parameters the decoded anchors give them
        rows = ckbd_gather(cm.scale_rows(sigma), h.y_shape, 1)
        ckbd_scatter(_decode(pn, ln, half, rows, 0, tables, h.R, dev), flat, h.y_shape, 1)
        return add_mean(flat, mu)

    # ---- per-image streams: container "ICRK" (codec.py), "fused" only.  With the convs, a non-anchor's (sigma, mu)
    # bits depend on the batch shape (the conv plans' kernel instance and split-K do), so a lone decoder could not
    # reproduce them; the fused context gives image n the same bits in any call, and h_s runs image by image as in
    # every model (`_prior_each`).
    def _codable_fused(self, what):
        if self.context_kernel != "fused":
            self._codable()
            raise NotImplementedError(f"CheckerboardCompressor2018 has no per-image streams ({what}): use "
                                      f"{what[:-len('_each')]} (or build the model with MODEL.CONTEXT.KERNEL \"fused\")")
        self._codable_each()

    @torch.no_grad()
    def compress_each(self, x, steps_per_chunk=1024):
        """x (N, 3, h, w) in [0, 1], any h, w >= 1 -> a list of N bytes objects, one "ICRK" stream per image."""
        self._codable_fused("compress_each")
        em, cm = self.entropy_model, self.conditional_model
        x, (N, h, w, H, W) = self._pad_each(x)
        y, z, z_sym, kz, (sigma_h, mu_h) = self._analyse(x, each=True)
        sigma, mu = self._eval_params(y, sigma_h, mu_h)      # one launch for the whole call
        y_sym, ky = self._symbols(y, mu, each=True)          # one K per image, serving both of its halves
        sz = em.encode_symbols_seg(z_sym, kz, steps_per_chunk)
        shape, rows, tables_of = tuple(y.shape), cm.scale_rows(sigma), self._tables_of(y.device)
        # image n's half is contiguous in the gathered buffers: the segments of the segmented coder are the images
        (sa, sn) = (_encode_seg(ckbd_gather(y_sym, shape, p), N, ckbd_gather(rows, shape, p), 0, tables_of, ky,
                                steps_per_chunk) for p in (0, 1))
        return [_codec.pack_checkerboard_image(self._header(1, H, W, y, z, steps_per_chunk, kz[n], ky[n], (h, w), n),
                                               sz[n][1], sa[n][1], sn[n][1], sz[n][0], sa[n][0], sn[n][0],
                                               version=self._image_format_version())
                for n in range(N)]

    def _tables_of(self, device):
        """K -> the conditional model's tables, each K built once for the two halves."""
        built = {}

        def tables_of(K):
            if K not in built:
                built[K] = self.conditional_model.tables(K, device)
            return built[K]
        return tables_of

    @torch.no_grad()
    def decompress_each(self, streams):
        """A list of M bytes objects from `compress_each` (any sizes, coded in any calls; same weights, build,
        COMPUTE_DTYPE and device type) -> a list of M tensors (1, 3, h_m, w_m).  Streams that share a padded size and
        chunk size are decoded by the same launches: all their anchors, one context, all their non-anchors, one g_s."""
        self._codable_fused("decompress_each")
        em, cm = self.entropy_model, self.conditional_model
        parsed = [_codec.parse_checkerboard_image(d, *self._build_id(), version=self._image_format_version())
                  for d in streams]   # all validated before any launch
        groups = {}
        for m, (h, *_rest) in enumerate(parsed):
            self._check_stream(h, "decompress_each", f"stream {m}")
            groups.setdefault((h.H, h.W, h.latent_channels, h.R), []).append(m)
        out = [None] * len(parsed)
        for (_H, _W, _cy, R), idx in groups.items():
            hs = [parsed[m][0] for m in idx]
            lz, la, ln, pz, pa, pn = ([parsed[m][k] for m in idx] for k in range(1, 7))
            z_hat = em.decompress_seg(pz, hs[0].z_shape, lz, [h.kmax_z for h in hs], R)
            sigma_h, mu_h = self._prior_each(z_hat)
            shape = (len(idx), *hs[0].y_shape[1:])
            if tuple(sigma_h.shape) != shape:
                raise ValueError(f"decompress_each: the model's sigma {tuple(sigma_h.shape)} is not the streams' latent "
                                 f"shape {shape}")
            dev, half, kys = sigma_h.device, hs[0].nsym_y // 2, [h.kmax_y for h in hs]
            tables_of = self._tables_of(dev)
            flat = torch.zeros(len(idx) * hs[0].nsym_y, dtype=torch.float32, device=dev)
            # pass one: every image's anchors, under the hyperprior's own parameters
            rows = ckbd_gather(cm.scale_rows(sigma_h), shape, 0)
            ckbd_scatter(_decode_seg(pa, la, half, rows, 0, tables_of, kys, R, dev), flat, shape, 0)
            sigma, mu = self._context(add_mean(flat, mu_h), sigma_h, mu_h)
            # pass two: every image's non-anchors, under the parameters its decoded anchors give them
            rows = ckbd_gather(cm.scale_rows(sigma), shape, 1)
            ckbd_scatter(_decode_seg(pn, ln, half, rows, 0, tables_of, kys, R, dev), flat, shape, 1)
            for m, img in zip(idx, self._reconstruct_each(add_mean(flat, mu), hs)):
                out[m] = img
        return out
