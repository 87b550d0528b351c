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
every step, which is why TrainStep(graph=True) refuses this model (`graph_refusal`).

Budget.  `compress_each_to(x, budgets)` chooses the quality of every image so that its stream holds at most its
budget of bytes: the grid search of codec.py on sizes the coder itself reports, every candidate of every image
measured from one pass of g_a and h_a.  It neither reads nor changes `quality`."""
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
    _containers = (_codec.pack_gained, _codec.parse_gained, _codec.pack_gained_image, _codec.parse_gained_image)
    _layered_containers = (_codec.pack_layered_gained_image, _codec.parse_layered_gained_image,
                           _codec.LayeredGainedImageHeader)

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

    def _refine_weights(self, N):
        """`loss_weight` of every image's quality: the call's qualities give both the gains and lambda_n."""
        qs = self._qualities if len(self._qualities) == N else self._qualities * N
        return [float(self.loss_weight(q)) for q in qs]

    # ---- coding to a byte budget: the search rule of codec.py on sizes the coder itself reports
    def _check_budget_call(self, x, budgets, steps_per_chunk, candidates, rounds):
        """The budgets of a `compress_each_to` call, one int per image; every check in front of any launch."""
        who = "compress_each_to"
        if x.dim() != 4 or min(x.shape) < 1:
            raise ValueError(f"{who}: image batch {tuple(x.shape)} must be (N, C, h, w) with h, w >= 1")
        return self._check_budget_args(who, x.shape[0], "images", budgets, steps_per_chunk, candidates, rounds)

    @staticmethod
    def _check_budget_args(who, N, what, budgets, steps_per_chunk, candidates, rounds):
        """The budgets of a call on N images or streams (`what`), one int each, and the checks of the search's
        arguments."""
        def integer(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

        if integer(budgets):
            budgets = [budgets] * N
        elif isinstance(budgets, (list, tuple, np.ndarray)) and getattr(budgets, "ndim", 1) == 1:
            budgets = list(budgets)
        else:
            raise ValueError(f"{who}: budgets are one positive int or a sequence of them, got {budgets!r}")
        if len(budgets) != N:
            raise ValueError(f"{who}: {len(budgets)} budgets for {N} {what}")
        if not all(integer(b) and b > 0 for b in budgets):
            raise ValueError(f"{who}: a budget is a positive int, a number of bytes, got {budgets!r}")
        for name, v, lo, hi in (("candidates", candidates, 2, 64), ("rounds", rounds, 1, 4),
                                ("steps_per_chunk", steps_per_chunk, 1, _codec.MAX_STEPS)):
            if not integer(v) or not lo <= v <= hi:
                raise ValueError(f"{who}: {name} is an integer in [{lo}, {hi}], got {v!r}")
        if N * candidates > 65535:
            raise ValueError(f"{who}: {N} {what} x {candidates} candidates exceed the 65535 segments of one launch")
        return [int(b) for b in budgets]

    def _budget_rounds(self, budgets, todo, measured, candidates, rounds, strict, measure):
        """The round loop of codec.py's search rule, shared by `compress_each_to` and `transcode_each_to`.
        budgets {n: bytes}; todo {n: the qualities of round 1}, consumed; measured {n: {quality: bytes}}, extended by
        everything the rounds measure; measure([(n, q)]) -> ([bytes of candidate m], keep) measures one round's
        candidates in one set of launches, keep(m) being what the final coding needs of candidate m.  Returns
        ({n: the chosen quality}, {n: keep(its candidate)}); a miss in round 1 is a BudgetError (strict) or the
        round's first quality."""
        chosen, kept = {}, {}
        for rnd in range(rounds):
            cands = [(n, q) for n in sorted(todo) for q in todo[n]]
            if not cands:
                break
            img, qs = [n for n, _ in cands], [q for _, q in cands]
            size, keep = measure(cands)
            for n in sorted(todo):
                ms = [m for m in range(len(cands)) if img[m] == n]
                measured[n].update((qs[m], size[m]) for m in ms)
                pick = _codec.budget_choice([qs[m] for m in ms], [size[m] for m in ms], budgets[n])
                if pick is None and rnd == 0:
                    smallest = min(size[m] for m in ms)
                    if strict:
                        raise _codec.BudgetError(n, budgets[n], smallest)
                    pick = qs[ms[0]]     # quality 0, the grid's first: the one stream that may exceed its budget
                    del todo[n]
                if pick is not None:
                    chosen[n] = pick
                    kept[n] = keep(ms[[qs[k] for k in ms].index(pick)])
            for n in list(todo):
                nxt = _codec.budget_next(measured[n], chosen[n])
                todo[n] = [] if nxt is None else _codec.budget_refine(chosen[n], nxt, candidates)
                if not todo[n]:
                    del todo[n]     # chosen is S-1, or no float32 lies between it and the next one measured
        return chosen, kept

    @torch.no_grad()
    def compress_each_to(self, x, budgets, steps_per_chunk=1024, candidates=8, rounds=2, strict=True):
        """x (N, 3, h, w) in [0, 1], any h, w >= 1, and `budgets` (one positive int, or N of them: bytes of the whole
        stream, header included) -> (a list of N "ICRQ" streams as `compress_each` writes them, their float32
        qualities): every image at the quality the search rule of codec.py chooses for its budget among `rounds`
        rounds of `candidates` qualities, so that len(stream) <= budget.  `model.quality` is not looked at and not
        changed.

        All candidates of all images are measured by one set of launches per round, from one pass of g_a and h_a:
        the gains, the symbols of z and of y, h_s (image by image, as `compress_each` and the decoder run it, which
        is what makes the measured size the size of the stream), the table rows and the coder's own chunk lengths
        (`measure_seg`: the coder without its output); one small copy of the lengths comes back per round.  Only the
        N chosen candidates are coded.

        An image that fits at no quality of round 1: codec.BudgetError (a ValueError with .image, .budget,
        .smallest) in front of any packing; with strict=False it is coded at quality 0 and is the one stream that may
        exceed its budget."""
        from ...functional import gain_symbolize_seg, measure_seg
        from ..blocks.entropy_model import symbolize_seg, symbols_as_tensor, table_pool
        who = "compress_each_to"
        budgets = self._check_budget_call(x, budgets, steps_per_chunk, candidates, rounds)
        self._codable_each()
        em, cm, R = self.entropy_model, self.conditional_model, int(steps_per_chunk)
        x, (N, h, w, H, W) = self._pad_each(x)
        y = self.analysis_transform(x)
        z = self.prior_analysis(self._hyper_input(y))
        z_tables, y_tables = {}, {}     # one table per K and tensor kind for the whole call

        def tables_z(K):
            if K not in z_tables:
                z_tables[K] = em.tables(K)
            return z_tables[K]

        def tables_y(K):
            if K not in y_tables:
                y_tables[K] = cm.tables(K, y.device)
            return y_tables[K]

        def measure(cands):
            img, qs = [n for n, _ in cands], [q for _, q in cands]
            M = len(cands)
            self._use(qs)
            g_y, _, g_z, g_inv_z = self._gains
            try:
                z_sym, kz = symbolize_seg(channel_scale(z[torch.as_tensor(img, device=z.device)], g_z))
                z_hat = channel_scale(symbols_as_tensor(z_sym.to(torch.float32), (M, *z.shape[1:])), g_inv_z)
                sigma, mean = self._prior_each(z_hat)
                y_sym, ky = gain_symbolize_seg(y, g_y, mean, img)
            except ValueError as e:
                raise ValueError(f"{who}: among the candidates {cands}: {e}") from None
            rows = cm.scale_rows(sigma.expand_as(mean))
            lz = measure_seg(z_sym, M, None, em.channels, *table_pool(tables_z, kz), R)
            ly = measure_seg(y_sym, M, rows, 0, *table_pool(tables_y, ky), R)
            lens = torch.cat([lz, ly]).cpu().numpy().astype(np.int64)    # the one D2H copy of the round
            lz, ly = lens[:lz.numel()].reshape(M, -1), lens[lz.numel():].reshape(M, -1)
            fixed = _codec.gained_image_fixed_bytes(self._header(1, H, W, y, z, R, 0, 0, (h, w)))
            size = [_codec.image_stream_bytes(fixed, lz[m], ly[m]) for m in range(M)]
            nz, ny = z_sym.numel() // M, y_sym.numel() // M

            def keep(m):
                return (z_sym[m * nz:(m + 1) * nz].clone(), kz[m], y_sym[m * ny:(m + 1) * ny].clone(), ky[m],
                        sigma[m:m + 1].clone(), mean[m:m + 1].clone(), size[m])
            return size, keep

        measured = {n: {} for n in range(N)}   # quality -> bytes, everything measured for the image so far
        todo = {n: _codec.budget_grid(self.levels, candidates) for n in range(N)}
        try:
            chosen, kept = self._budget_rounds(dict(enumerate(budgets)), todo, measured, candidates, rounds, strict, measure)
            chosen, kept = [chosen[n] for n in range(N)], [kept[n] for n in range(N)]
            self._use(chosen)
            z_sym, y_sym = (torch.cat([k[i] for k in kept]) for i in (0, 2))
            sigma, mean = (torch.cat([k[i] for k in kept]) for i in (4, 5))
            kz, ky = ([k[i] for k in kept] for i in (1, 3))
            sz = em.encode_symbols_seg(z_sym, kz, R)
            sy = cm.encode_symbols_seg(y_sym, ky, sigma.expand_as(y), R, mean=mean)
            streams = [self._pack_image(self._header(1, H, W, y, z, R, kz[n], ky[n], (h, w), n),
                                        sz[n][1], sy[n][1], sz[n][0], sy[n][0]) for n in range(N)]
        finally:
            self._end_call()
        for n, s in enumerate(streams):
            if len(s) != kept[n][6]:
                raise RuntimeError(f"{who}: the stream of image {n} at quality {chosen[n]} holds {len(s)} bytes, "
                                   f"{kept[n][6]} were measured")
        return streams, chosen

    # ---- transcoding in the latent domain: a stream at quality q1 to quality q2, or to a byte budget, from its integers
    # alone (codec.py states the requantization rule and the search's two differences)
    def _transcode_qualities(self, qualities, M, who):
        if isinstance(qualities, (str, bytes)):
            raise ValueError(f"{who}: a quality is a number in [0, {self.levels - 1}], got {qualities!r}")
        if isinstance(qualities, (list, tuple, np.ndarray, torch.Tensor)) and getattr(qualities, "ndim", 1) > 0:
            qs = [_as_quality(v.item() if hasattr(v, "item") else v, self.levels) for v in qualities]
            if len(qs) != M:
                raise ValueError(f"{who}: {len(qs)} qualities for {M} streams")
            return qs
        return [_as_quality(qualities.item() if hasattr(qualities, "item") else qualities, self.levels)] * M

    def _requant_decode(self, parsed, idx):
        """What the requantizer reads of the streams `idx` (one padded size, one chunk size), decoded once however many
        targets follow: (z_hat1, r1 (N, C, *), mu1, g_y'(q1) (N, C))."""
        from ..blocks.entropy_model import symbols_as_tensor
        hs = [parsed[m][0] for m in idx]
        self._begin_decode(hs)
        g_inv_y = self._gains[1]
        _k_z, z_hat, sigma, mean = self._transcode_decode_z(parsed, idx)
        r = self._transcode_decode_y(parsed, idx, self.conditional_model.scale_rows(sigma))
        return z_hat, symbols_as_tensor(r, tuple(mean.shape)), mean, g_inv_y

    def _requant_targets(self, decoded, img, qs):
        """(symbols of z, kmax_z, symbols of y, kmax_y, sigma2, mu2) of the targets (source img[m], quality qs[m]) of
        one `_requant_decode`, by the requantization rule: one set of launches for all of them."""
        from ...functional import requant_seg
        from ..blocks.entropy_model import symbolize_seg, symbols_as_tensor
        z_hat1, r, mu1, g_inv_y1 = decoded
        M = len(img)
        self._use(qs)
        g_y, _, g_z, g_inv_z = self._gains
        src = z_hat1 if list(img) == list(range(z_hat1.shape[0])) else z_hat1[torch.as_tensor(img, device=z_hat1.device)]
        z_sym, kz = symbolize_seg(channel_scale(src, g_z))
        z_hat2 = channel_scale(symbols_as_tensor(z_sym.to(torch.float32), (M, *z_hat1.shape[1:])), g_inv_z)
        sigma, mean = self._prior_each(z_hat2)
        y_sym, ky = requant_seg(r, mu1, g_inv_y1, g_y, mean, img)
        return z_sym, kz, y_sym, ky, sigma, mean

    def _requant_group(self, parsed, idx, targets, R, who):
        """The streams `idx` requantized to `targets`, one quality each, at R steps per chunk."""
        from ..blocks.entropy_model import _encode_seg
        em, cm = self.entropy_model, self.conditional_model
        hs = [parsed[m][0] for m in idx]
        decoded = self._requant_decode(parsed, idx)
        try:
            z_sym, kz, y_sym, ky, sigma, mean = self._requant_targets(decoded, range(len(idx)), targets)
        except ValueError as e:
            raise ValueError(f"{who}: among the streams {list(idx)} at the qualities {list(targets)}: {e}") from None
        rows = cm.scale_rows(sigma.expand_as(mean))
        sz = em.encode_symbols_seg(z_sym, kz, R)
        sy = _encode_seg(y_sym, len(idx), rows, 0, lambda K: cm.tables(K, rows.device), ky, R)
        return [self._pack_image(_codec.transcoded_header(h, R=int(R), quality=targets[k], kmax_z=kz[k], kmax_y=ky[k]),
                                 sz[k][1], sy[k][1], sz[k][0], sy[k][0]) for k, h in enumerate(hs)]

    @torch.no_grad()
    def transcode_each_to(self, streams, budgets, steps_per_chunk=None, candidates=8, rounds=2, strict=True):
        """`compress_each_to` for someone who holds only the streams: a list of M "ICRQ" streams of this model and
        `budgets` (one positive int, or M of them: bytes of the whole stream, header included) -> (a list of M
        streams, their float32 qualities), every stream with len(stream) <= budget, without g_a, g_s or a pixel.
        `model.quality` is not looked at and not changed.

        A stream is first re-chunked where `steps_per_chunk` asks for another R (no loss); one that then fits its
        budget is the result at its own quality -- with no re-chunk asked the same object: no generation is lost
        where none is needed.  Otherwise the search rule of codec.py runs on the sizes the coder reports for the
        requantized candidates (`measure_seg`), round 1 being the grid below the stream's quality and the stream's
        own size the upper end of every refinement.  The streams of a group are decoded once; all candidates of all
        of them are requantized and measured by one set of launches per round, and only chunk lengths come back.

        A stream that fits at no quality of round 1 (or is already at quality 0): codec.BudgetError (.image the
        stream's index) in front of any packing of a requantized stream -- for a stream at quality 0 that already has
        the target R in front of any launch; one that must be re-chunked is judged at its re-chunked length.  With
        strict=False it is returned at quality 0 and is the one result
        that may exceed its budget."""
        from ...functional import measure_seg
        from ..blocks.entropy_model import _encode_seg, table_pool
        who = "transcode_each_to"
        streams, parsed, _ = self._transcode_parse(streams, steps_per_chunk, who)
        budgets = self._check_budget_args(who, len(streams), "streams", budgets,
                                          1 if steps_per_chunk is None else steps_per_chunk, candidates, rounds)
        em, cm = self.entropy_model, self.conditional_model
        if strict:      # what the headers alone show, in front of any launch: quality 0, its final R, too large
            for m, (h, *_rest) in enumerate(parsed):
                if h.quality == 0.0 and h.R == (steps_per_chunk or h.R) and len(streams[m]) > budgets[m]:
                    raise _codec.BudgetError(m, budgets[m], len(streams[m]))
        if steps_per_chunk is not None and any(p[0].R != steps_per_chunk for p in parsed):
            streams = self.transcode_each(streams, steps_per_chunk=steps_per_chunk)
            parsed = [self._parse_image(d, *self._build_id()) for d in streams]
        out, qualities = list(streams), [p[0].quality for p in parsed]
        search = [m for m, d in enumerate(streams) if len(d) > budgets[m]]
        grids = {m: _codec.transcode_grid(self.levels, candidates, parsed[m][0].quality) for m in search}
        for m in search:
            if not grids[m]:      # at quality 0, nothing below it, and too large even as re-chunked
                if strict:
                    raise _codec.BudgetError(m, budgets[m], len(streams[m]))
        search = [m for m in search if grids[m]]
        z_tables, y_tables = {}, {}     # one table per K and tensor kind for the whole call

        def tables_z(K):
            if K not in z_tables:
                z_tables[K] = em.tables(K)
            return z_tables[K]

        def tables_y(K):
            if K not in y_tables:
                y_tables[K] = cm.tables(K, next(self.parameters()).device)
            return y_tables[K]

        found = []     # per group: (its streams, R, {m: chosen quality}, {m: what the final coding needs})
        try:
            for (_H, _W, _C, R), idx in self._transcode_groups(parsed, search).items():
                local = {m: k for k, m in enumerate(idx)}
                decoded = self._requant_decode(parsed, idx)
                fixed = _codec.gained_image_fixed_bytes(parsed[idx[0]][0])

                def measure(cands):
                    img, qs = [local[m] for m, _ in cands], [q for _, q in cands]
                    M = len(cands)
                    try:
                        z_sym, kz, y_sym, ky, sigma, mean = self._requant_targets(decoded, img, qs)
                    except ValueError as e:
                        raise ValueError(f"{who}: among the candidates (stream, quality) {cands}: {e}") from None
                    rows = cm.scale_rows(sigma.expand_as(mean))
                    lz = measure_seg(z_sym, M, None, em.channels, *table_pool(tables_z, kz), R)
                    ly = measure_seg(y_sym, M, rows, 0, *table_pool(tables_y, ky), R)
                    lens = torch.cat([lz, ly]).cpu().numpy().astype(np.int64)    # the one D2H copy of the round
                    lz, ly = lens[:lz.numel()].reshape(M, -1), lens[lz.numel():].reshape(M, -1)
                    size = [_codec.image_stream_bytes(fixed, lz[m], ly[m]) for m in range(M)]
                    nz, ny = z_sym.numel() // M, y_sym.numel() // M

                    def keep(m):
                        return (z_sym[m * nz:(m + 1) * nz].clone(), kz[m], y_sym[m * ny:(m + 1) * ny].clone(), ky[m],
                                rows[m * ny:(m + 1) * ny].clone(), size[m])
                    return size, keep

                measured = {m: _codec.transcode_measured(parsed[m][0].quality, len(streams[m])) for m in idx}
                chosen, kept = self._budget_rounds({m: budgets[m] for m in idx}, {m: grids[m] for m in idx}, measured,
                                                   candidates, rounds, strict, measure)
                found.append((idx, R, chosen, kept))
            for idx, R, chosen, kept in found:      # every stream has its quality: nothing was packed before this
                z_sym, y_sym, rows = (torch.cat([kept[m][i] for m in idx]) for i in (0, 2, 4))
                kz, ky = ([kept[m][i] for m in idx] for i in (1, 3))
                sz = em.encode_symbols_seg(z_sym, kz, R)
                sy = _encode_seg(y_sym, len(idx), rows, 0, tables_y, ky, R)
                for k, m in enumerate(idx):
                    h = _codec.transcoded_header(parsed[m][0], quality=chosen[m], kmax_z=kz[k], kmax_y=ky[k])
                    out[m], qualities[m] = self._pack_image(h, sz[k][1], sy[k][1], sz[k][0], sy[k][0]), chosen[m]
                    if len(out[m]) != kept[m][5]:
                        raise RuntimeError(f"{who}: stream {m} at quality {chosen[m]} holds {len(out[m])} bytes, "
                                           f"{kept[m][5]} were measured")
        finally:
            self._end_call()
        return out, qualities
