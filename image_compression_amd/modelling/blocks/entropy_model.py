"""Entropy bottleneck (reference modelling/blocks/entropy_model.py).

EntropyModel (factorized prior on z, :188-269) and the symmetric conditional
models on y (:272-378).  Noise/round + likelihood run in fused HIP kernels
(csrc/entropy.hip): the factorized CDF MLP (1->3->3->3->1 per channel, softplus
weights, tanh gates) is evaluated twice per element in registers, and the
per-channel parameter gradients are deterministic block reductions.  Other
cfg.MODEL.ENTROPY_MODEL.DIMS and any BIN run the generic kernels
(ic_factorized_*_net, ic_conditional_*_bin): up to 5 hidden layers of width <= 8
with the activations in registers, larger nets (up to 31 hidden layers of width
<= 256) with them in a workspace.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib
from ... import codec as _codec
from ... import noise as _noise
from ...functional import CELossFn, _to_last, conditional, conditional_likelihood, factorized, quantize
from ...functional import ckbd_input as _ckbd_input, ckbd_params as _ckbd_params
from .build import ENTROPY_MODEL_REGISTRY

LOG2 = math.log(2.0)


class CDFLayer(nn.Module):
    """One per-channel affine(+gate) layer (entropy_model.py:47-78).
    Parameter shapes and init order match the reference (weight constant
    ln(expm1(1/scale/out)), bias U(-1/2, 1/2), factor 0)."""

    def __init__(self, channels, in_dim, out_dim, init_scale, act=True):
        super().__init__()
        self.act = act
        w0 = math.log(math.expm1(1.0 / init_scale / out_dim))
        self.weight = nn.Parameter(nn.init.constant_(torch.empty(1, channels, out_dim, in_dim), w0))
        self.bias = nn.Parameter(nn.init.uniform_(torch.empty(1, channels, out_dim, 1), -0.5, 0.5))
        if act:
            self.factor = nn.Parameter(nn.init.zeros_(torch.empty(1, channels, out_dim, 1)))

    def forward(self, x):
        # auxiliary API (the hot path evaluates the whole MLP in one kernel)
        x = torch.matmul(F.softplus(self.weight), x) + self.bias
        return x + torch.tanh(x) * torch.tanh(self.factor) if self.act else x


class CDFEstimator(nn.Module):
    """Per-channel monotone CDF logits (entropy_model.py:81-114)."""

    def __init__(self, channels, dims=(3, 3, 3), init_scale=10.):
        super().__init__()
        dims = [1] + list(dims) + [1]  # the reference inserts into the cfg list in place
        n = len(dims) - 1
        scale = init_scale ** (1 / n)
        self.layers = nn.Sequential(*[CDFLayer(channels, dims[i], dims[i + 1], scale, i < n - 1)
                                      for i in range(n)])
        self.dims = dims

    def forward(self, x):
        # auxiliary API; returns the reference's layout (see EntropyModel._ref_layout)
        N, C = x.shape[:2]
        order = [0] + list(range(2, x.dim())) + [1]
        h = x.permute(*order).reshape(-1, C, 1, 1)
        h = self.layers(h)
        return h.view(N, *x.shape[2:], C).permute(*order)

    def flat_params(self):
        out = []
        for i, layer in enumerate(self.layers):
            out += [layer.weight, layer.bias]
            if layer.act:
                out.append(layer.factor)
        return out


class BaseEntropyModel(nn.Module):
    """entropy_model.py:117-185."""

    def _prob_mass(self, x):
        raise NotImplementedError("to be inherited")

    def _quantize(self, x, mode):
        raise NotImplementedError()

    def _dequantize(self, x):
        raise NotImplementedError()

    def compress(self, x):
        raise NotImplementedError()

    def decompress(self, x):
        raise NotImplementedError()

    def _codable(self):
        if self.training:
            raise RuntimeError("compress / decompress run in eval mode only (rounding, not noise)")
        if float(self.bin) != 1.0:
            raise NotImplementedError(f"the entropy coder codes integer symbols: BIN must be 1, got {self.bin}")

    def _ce_loss(self, probs):
        """sum clamp(-log2(p + 1e-10), 0, 50) — deterministic HIP reduction."""
        return CELossFn.apply(probs)


def symbolize(x):
    """x (N, C, *) -> (int32 symbols flattened in (n, *, c) order, kmax = max |symbol|): the
    eval-mode rounding of `quantize` / `factorized`.  ValueError beyond the coder's limit."""
    _lib.require_device(x)
    sym, kmax = _lib.codec_ops().symbolize(_to_last(x))
    return sym, int(kmax)


def _mean_last(x, mean):
    """(x, mean) as dense channels-last storage; the mean must have x's shape (its elements pair with x's)."""
    _lib.require_device(x, mean)
    if tuple(mean.shape) != tuple(x.shape):
        raise ValueError(f"the mean {tuple(mean.shape)} must have the shape of the tensor it centres {tuple(x.shape)}")
    return _to_last(x), _to_last(mean)


def symbolize_mean(y, mean):
    """`symbolize` of the residual: int32 rint(y - mean), one fp32 subtraction per element, and its kmax."""
    sym, kmax = _lib.mean_ops().symbolize(*_mean_last(y, mean))
    return sym, int(kmax)


def symbolize_mean_seg(y, mean):
    """`symbolize_seg` of the residual rint(y - mean): [kmax of image n]; ValueError naming the image."""
    sym, kmax = _lib.mean_ops().symbolize_seg(*_mean_last(y, mean), int(y.shape[0]))
    return sym, [int(k) for k in kmax]


def center_round(y, mean):
    """(r, y_hat) = (rint(y - mean), r + mean) as (N, C, *) tensors over channels-last storage: the eval-mode
    quantiser about a mean.  Inference only (no autograd node)."""
    yl, ml = _mean_last(y, mean)
    r, y_hat = _lib.mean_ops().center_round(yl, ml)
    return symbols_as_tensor(r, tuple(y.shape)), symbols_as_tensor(y_hat, tuple(y.shape))


def add_mean(flat, mean):
    """The decoder's y_hat = r + mean (the addition of `center_round`, bit for bit) from the flat float
    integers r in (n, *, c) order, as the (N, C, *) tensor over that storage."""
    _lib.require_device(flat, mean)
    return symbols_as_tensor(_lib.mean_ops().add_mean(flat, _to_last(mean)), tuple(mean.shape))


# ---- checkerboard context model: position (i, j) of a latent map is an anchor when i + j is even (parity 0)
def ckbd_input(y, mean):
    """(u, v): y and |y - mean| (one fp32 subtraction) at the anchors, +0.0 elsewhere -- what the context convs
    read.  Differentiable in y and mean."""
    return _ckbd_input(y, mean.expand_as(y))


def ckbd_params(mean_h, sigma_h, a, b):
    """(mean, sigma): (mean_h + a, sigma_h * exp(clamp(b, -4, 4))) at the non-anchors, the hyperprior's own
    (mean_h, sigma_h) bit for bit at the anchors.  Differentiable in all four."""
    return _ckbd_params(mean_h, sigma_h.expand_as(mean_h), a, b)


def _ckbd_view(flat, shape):
    N, C, H, W = shape
    if flat.numel() != N * C * H * W:
        raise ValueError(f"{flat.numel()} values are not a latent of shape {tuple(shape)}")
    return flat.contiguous().view(N, H, W, C)


def ckbd_gather(flat, shape, parity):
    """The values of `flat` (a latent of logical `shape` (N, C, H, W) flattened in (n, i, j, c) order: float
    values, int32 symbols or uint8 table rows) at the positions of `parity`, packed in that same order."""
    if not flat.is_cuda:
        raise RuntimeError(f"imgcomp: HIP kernels need tensors on a ROCm (cuda) device; got a tensor on {flat.device}")
    return _lib.ckbd_ops().gather(_ckbd_view(flat, shape), int(parity))


def ckbd_scatter(half, flat, shape, parity):
    """Writes the packed float values `half` of `parity` to their positions of `flat` (in place; the other parity
    keeps its values) and returns `flat`."""
    _lib.require_device(half, flat)
    if not flat.is_contiguous():
        raise ValueError("ckbd_scatter writes in place: the full tensor must be contiguous")
    _lib.ckbd_ops().scatter(half.contiguous(), _ckbd_view(flat, shape), int(parity))
    return flat


def symbols_as_tensor(flat, shape):
    """Float symbols flattened in (n, *, c) order -> the logical (N, C, *) tensor over that
    channels-last storage: the layout the eval forward's quantized tensors have."""
    return flat.view(shape[0], *shape[2:], shape[1]).movedim(-1, 1)


def _encode(sym, rows, channels, tables, steps):
    packed = _lib.codec_ops().encode(sym, rows, int(channels), tables, int(steps))
    lens, payload = _codec.split_packed(packed.cpu().numpy(), sym.numel(), steps)  # the one D2H copy
    return payload, lens


def _decode(payload, lengths, n, rows, channels, tables, steps, device):
    buf = torch.from_numpy(_codec.join_packed(lengths, payload).copy()).to(device)
    return _lib.codec_ops().decode(buf, int(n), rows, int(channels), tables, int(steps))


# ---- segmented pieces (per-image streams): the images of a call lie back to back in one symbol buffer,
# each with its own K and table, and one launch serves them all
def symbolize_seg(x):
    """x (N, C, *) -> (int32 symbols of the N images back to back, each in (*, c) order, [kmax of image n]).
    ValueError naming the image whose symbols exceed the coder's limit."""
    _lib.require_device(x)
    sym, kmax = _lib.stream_ops().symbolize_seg(_to_last(x), int(x.shape[0]))
    return sym, [int(k) for k in kmax]


def table_pool(tables_of, kmaxes):
    """(pool, rows, K per segment, table word offset per segment): one table per distinct K, built by
    `tables_of(K)`, back to back in one device buffer; segments with the same K share theirs."""
    offs, parts, at = {}, [], 0
    for K in sorted(set(kmaxes)):
        t = tables_of(K)
        offs[K], rows = at, t.shape[0]
        parts.append(t.reshape(-1))
        at += t.numel()
    pool = parts[0] if len(parts) == 1 else torch.cat(parts)
    return pool, rows, [int(k) for k in kmaxes], [offs[k] for k in kmaxes]


def _encode_seg(sym, nseg, rows, channels, tables_of, kmaxes, steps):
    pool, nrows, ks, offs = table_pool(tables_of, kmaxes)
    packed = _lib.stream_ops().encode_seg(sym, int(nseg), rows, int(channels), pool, nrows, ks, offs, int(steps))
    parts = _codec.split_packed_seg(packed.cpu().numpy(), nseg, sym.numel() // nseg, steps)  # the one D2H copy
    return [(payload, lens) for lens, payload in parts]


def _decode_seg(payloads, lengths, seg_len, rows, channels, tables_of, kmaxes, steps, device):
    pool, nrows, ks, offs = table_pool(tables_of, kmaxes)
    buf = torch.from_numpy(_codec.join_packed_seg(list(zip(lengths, payloads))).copy()).to(device)
    return _lib.stream_ops().decode_seg(buf, len(payloads), int(seg_len), rows, int(channels), pool, nrows, ks, offs,
                                        int(steps))


def _ref_layout(p):
    """The reference re-permutes the CDF output with the forward permutation
    instead of its inverse (entropy_model.py:108-113): for (N, C, H, W) the
    probabilities come back as (N, W, C, H), p_ref[n, w, c, h] = p[n, c, h, w].
    Reproduced as a zero-copy view so parity holds on the returned tensor."""
    order = [0] + list(range(2, p.dim())) + [1]
    return p.movedim(1, -1).permute(*order)


@ENTROPY_MODEL_REGISTRY.register()
class EntropyModel(BaseEntropyModel):
    def __init__(self, in_channels, cfg):
        super().__init__()
        em = cfg.MODEL.ENTROPY_MODEL
        self._cdf_estimator = CDFEstimator(in_channels, em.DIMS, em.INIT_SCALE)
        self.bin = em.BIN

    def forward(self, x):
        u = _noise.pop_injected() if self.training else None
        q, p = factorized(x, self._cdf_estimator.flat_params(), self.training, u, self._cdf_estimator.dims, self.bin)
        probs = _ref_layout(p)
        return q, probs, self._ce_loss(probs)

    def _logit_cumulative(self, x):
        return self._cdf_estimator(x)

    # ---- entropy coding (eval only): one table row per channel, rebuilt per call from the weights
    @property
    def channels(self):
        return self._cdf_estimator.layers[0].weight.shape[1]

    def tables(self, kmax):
        """Quantized CDFs [C][2K+2] of the integers -K..K under the current weights: the eval-mode
        likelihood kernel on the grid (1, C, 2K+1, 1), then the table kernel."""
        self._codable()
        dev = self._cdf_estimator.layers[0].weight.device
        K = int(kmax)
        grid = torch.arange(-K, K + 1, device=dev, dtype=torch.float32).view(1, 1, -1, 1).expand(1, self.channels, -1, 1)
        with torch.no_grad():
            _, p = factorized(grid, self._cdf_estimator.flat_params(), False, None, self._cdf_estimator.dims, self.bin)
            return _lib.codec_ops().build_tables(p[0, :, :, 0].contiguous())

    def encode_symbols(self, sym, kmax, steps_per_chunk=1024):
        return _encode(sym, None, self.channels, self.tables(kmax), steps_per_chunk)

    @torch.no_grad()
    def compress(self, z, steps_per_chunk=1024):
        """z (N, C, *) -> (payload bytes, chunk lengths uint32[chunks], kmax)."""
        self._codable()
        sym, kmax = symbolize(z)
        payload, lens = self.encode_symbols(sym, kmax, steps_per_chunk)
        return payload, lens, kmax

    @torch.no_grad()
    def decompress(self, payload, shape, lengths, kmax, steps_per_chunk=1024):
        """The float tensor of integers (N, C, *) = `shape` that `compress` coded."""
        self._codable()
        tables = self.tables(kmax)
        n = math.prod(shape)
        flat = _decode(payload, lengths, n, None, self.channels, tables, steps_per_chunk, tables.device)
        return symbols_as_tensor(flat, tuple(shape))

    def encode_symbols_seg(self, sym, kmaxes, steps_per_chunk=1024):
        """Symbols of len(kmaxes) images back to back -> [(payload bytes, chunk lengths)] per image."""
        return _encode_seg(sym, len(kmaxes), None, self.channels, self.tables, kmaxes, steps_per_chunk)

    @torch.no_grad()
    def decompress_seg(self, payloads, shape, lengths, kmaxes, steps_per_chunk=1024):
        """M streams of images of one `shape` (1, C, *) -> the float tensor of integers (M, C, *)."""
        self._codable()
        dev = self._cdf_estimator.layers[0].weight.device
        flat = _decode_seg(payloads, lengths, math.prod(shape), None, self.channels, self.tables, kmaxes,
                           steps_per_chunk, dev)
        return symbols_as_tensor(flat, (len(payloads), *shape[1:]))


class SymmetricConditionalModel(BaseEntropyModel):
    """entropy_model.py:272-352; subclasses pick the standardized CDF."""
    KIND = None

    def __init__(self, cfg, scale_min=0.11, scale_max=256., num_scales=64):
        super().__init__()
        self.bin = cfg.MODEL.ENTROPY_MODEL.BIN
        # the entropy coder's scale table: num_scales log-spaced scales (compress / decompress only)
        self.scale_min, self.scale_max, self.num_scales = float(scale_min), float(scale_max), int(num_scales)

    # ---- entropy coding (eval only): one table row per table scale, rebuilt per call
    def tables(self, kmax, device):
        """Quantized CDFs [L][2K+2] of the integers -K..K at each table scale: the likelihood
        kernel (mode 4) on the grid, then the table kernel."""
        self._codable()
        K = int(kmax)
        scales, _ = _codec.scale_table(self.num_scales, self.scale_min, self.scale_max)
        grid = torch.arange(-K, K + 1, device=device, dtype=torch.float32).expand(self.num_scales, -1).contiguous()
        scale = torch.from_numpy(scales).to(device).view(-1, 1).expand_as(grid).contiguous()
        with torch.no_grad():
            return _lib.codec_ops().build_tables(conditional_likelihood(grid, scale, None, self.KIND, self.bin))

    def scale_rows(self, sigma):
        """uint8 table row of every sigma (N, C, *), flattened in (n, *, c) order."""
        _lib.require_device(sigma)
        _, mids = _codec.scale_table(self.num_scales, self.scale_min, self.scale_max)
        return _lib.codec_ops().scale_index(_to_last(sigma), [float(m) for m in mids])

    # With `mean` (N, C, *) the symbols are those of the residual y - mean (mean-scale hyperprior): the tables,
    # rows and chunks are the same, K is the largest |residual|, and the decoders return r + mean.
    @staticmethod
    def _check_mean(mean, sigma):
        if mean is not None and tuple(mean.shape) != tuple(sigma.shape):
            raise ValueError(f"the mean {tuple(mean.shape)} must have sigma's shape {tuple(sigma.shape)}")

    def encode_symbols(self, sym, kmax, sigma, steps_per_chunk=1024, mean=None):
        """`sym`: rint(y), or with `mean` rint(y - mean) (`symbolize_mean`); the mean itself is not coded."""
        self._check_mean(mean, sigma)
        return _encode(sym, self.scale_rows(sigma), 0, self.tables(kmax, sigma.device), steps_per_chunk)

    @torch.no_grad()
    def compress(self, y, sigma, steps_per_chunk=1024, mean=None):
        """y, sigma (N, C, *) -> (payload bytes, chunk lengths uint32[chunks], kmax)."""
        self._codable()
        sigma = sigma.expand_as(y)
        sym, kmax = symbolize(y) if mean is None else symbolize_mean(y, mean.expand_as(y))
        payload, lens = self.encode_symbols(sym, kmax, sigma, steps_per_chunk)
        return payload, lens, kmax

    @torch.no_grad()
    def decompress(self, payload, sigma, lengths, kmax, steps_per_chunk=1024, mean=None):
        """The float tensor of integers, shaped like sigma, that `compress` coded with this sigma; with `mean`,
        those integers plus the mean."""
        self._codable()
        self._check_mean(mean, sigma)
        tables = self.tables(kmax, sigma.device)
        flat = _decode(payload, lengths, sigma.numel(), self.scale_rows(sigma), 0, tables, steps_per_chunk,
                       sigma.device)
        return symbols_as_tensor(flat, tuple(sigma.shape)) if mean is None else add_mean(flat, mean)

    def encode_symbols_seg(self, sym, kmaxes, sigma, steps_per_chunk=1024, mean=None):
        """Symbols of the N = len(kmaxes) images of sigma (N, C, *) back to back -> [(payload, lengths)];
        `mean` as in `encode_symbols` (`symbolize_mean_seg`)."""
        self._check_mean(mean, sigma)
        return _encode_seg(sym, len(kmaxes), self.scale_rows(sigma), 0, lambda K: self.tables(K, sigma.device), kmaxes,
                           steps_per_chunk)

    @torch.no_grad()
    def decompress_seg(self, payloads, sigma, lengths, kmaxes, steps_per_chunk=1024, mean=None):
        """M streams coded with the M images of sigma (M, C, *) -> the float tensor of integers like sigma; with
        `mean`, those integers plus the mean."""
        self._codable()
        self._check_mean(mean, sigma)
        flat = _decode_seg(payloads, lengths, sigma[0].numel(), self.scale_rows(sigma), 0,
                           lambda K: self.tables(K, sigma.device), kmaxes, steps_per_chunk, sigma.device)
        return symbols_as_tensor(flat, tuple(sigma.shape)) if mean is None else add_mean(flat, mean)

    def quantize(self, x):
        """_quantize on its own (train: noise, eval: round): with likelihood() the two halves of
        forward(), which Compressor2018 runs apart so the hyperprior can run meanwhile."""
        u = _noise.pop_injected() if self.training else None
        return quantize(x, self.training, u, self.bin)

    def likelihood(self, q, scale):
        """_prob_mass of already-quantized q (mean 0)."""
        return conditional_likelihood(q, scale.expand_as(q), None, self.KIND, self.bin)

    def forward(self, x, scale, mean=0):
        if isinstance(mean, torch.Tensor):
            mean_t = mean.expand_as(x)
        elif mean == 0:
            mean_t = None
        else:
            mean_t = torch.full_like(x, float(mean))
        u = _noise.pop_injected() if self.training else None
        return conditional(x, scale.expand_as(x), mean_t, self.KIND, self.training, u, self.bin)


@ENTROPY_MODEL_REGISTRY.register()
class GaussianConditionalModel(SymmetricConditionalModel):
    """Normal(0,1) CDF (entropy_model.py:355-365)."""
    KIND = 1


@ENTROPY_MODEL_REGISTRY.register()
class LaplacianConditionalModel(SymmetricConditionalModel):
    """Laplace(0,1) CDF (entropy_model.py:368-378) — the default (config.py:70)."""
    KIND = 0
