"""RegionGainedMeanScaleCompressor2018 -- region-of-interest coding on the gained mean-scale hyperprior: a quality
per 64 x 64 pixel block instead of one per image, so that a face or a line of text is coded at quality 5 while the sky
around it is coded at quality 1.

The parameters and the state-dict keys are GainedMeanScaleCompressor2018's (a gained checkpoint loads with
strict=True; a fresh model has the gained model's values from the same seed).  What changes is where the gain
vectors come from.  A quality map is uint8 codes k[n, bi, bj] (codec.py: q(k) = k (S - 1) / 255 in float32); one
block is one position of z and 4 x 4 positions of y.  Per call, on both sides of the codec:
    U = the distinct codes, ascending;  rows = gain_vector(table, [q(u) for u in U]) for each of the four tables;
    every position is scaled by the row whose index is the rank of its block's code (functional.block_scale, shift 0
    on z and 2 on y).
A uniform map of code k therefore holds bit for bit the gains of the gained model at quality q(k), and a two-region
map costs the same four gain_vector launches as a scalar quality.

Quality.  `set_quality_map(codes)`: uint8 codes (Hb, Wb) for every image of the batch or (N, Hb, Wb), numpy or torch,
None to clear; (Hb, Wb) must be the call's padded size over 64 or the call raises ValueError before any launch.
`set_quality(q)` is the uniform map of quality_code(q, S) sized to the call (a sequence: one uniform map per image of
`compress_each`), and clears a map.  The decoders take the map from the stream ("ICRM" / "ICRR"), never from the model.

Training.  Only the MSE with REDUCTION "mean": total_loss = block_mse(x, x~; w) + bpp with w[r] = loss_weight(q(U[r])),
losses["MSE"] the plain mean (the kernel's second output).  With `sample_quality` (the default) every training
forward draws one integer level per block, independent and uniform, from the CPU generator seeded with cfg.SEED
(`last_quality`: the code map; no device draw, the Philox order z, then y is unchanged); otherwise it uses the map
that was set, or the uniform map of `quality`.  H and W must be multiples of 64 in training mode.  The map changes on
the host every step, which is why TrainStep(graph=True) refuses this model (`graph_refusal`).

Budget.  `compress_each_map_to(x, budgets)` chooses the map of every image so that its stream holds at most its budget
of bytes: per block the level that minimises bits + w sse on the tables of `rate_distortion_tables` (the allocation
rule of codec.py: an estimate that steers), at the slope the search rule of codec.py finds on sizes the coder itself
reports (exact), every candidate map of every image allocated, symbolised and measured on the device from one pass of
g_a and h_a.  It neither reads nor changes `quality` and `quality_map`."""
import numpy as np
import torch

from ... import codec as _codec
from ...functional import block_mse, block_scale
from .build import META_ARCH_REGISTRY
from .gained2021 import GainedMeanScaleCompressor2018


def _as_codes(codes):
    """A quality map as a contiguous uint8 numpy array (Hb, Wb) or (N, Hb, Wb); ValueError for anything else."""
    if isinstance(codes, torch.Tensor):
        if codes.dtype != torch.uint8:
            raise ValueError(f"a quality map holds uint8 codes, got {codes.dtype}")
        codes = codes.detach().cpu().numpy()
    codes = np.asarray(codes)
    if codes.dtype != np.uint8 or codes.ndim not in (2, 3) or codes.size == 0:
        raise ValueError(f"a quality map holds uint8 codes of shape (Hb, Wb) or (N, Hb, Wb), got {codes.dtype} "
                         f"{codes.shape}")
    return np.ascontiguousarray(codes).copy()


@META_ARCH_REGISTRY.register()
class RegionGainedMeanScaleCompressor2018(GainedMeanScaleCompressor2018):
    graph_refusal = ("RegionGainedMeanScaleCompressor2018 draws its quality map and its block weights on the host every "
                     "step: a captured graph would replay one map for ever; use TrainStep(graph=False)")
    refine_refusal = ("RegionGainedMeanScaleCompressor2018 is not covered: its distortion is weighed by a quality map, "
                      "which the objective R + lambda MSE does not know; use GainedMeanScaleCompressor2018")
    layered_refusal = ("RegionGainedMeanScaleCompressor2018 is not covered: the layered containers carry one quality "
                       "per image, not a quality map; use GainedMeanScaleCompressor2018")

    def __init__(self, cfg):
        names, reduction = list(cfg.MODEL.LOSS.DISTORTION_LOSS_NAMES), cfg.MODEL.LOSS.REDUCTION
        if names != ["MSE"] or reduction != "mean":
            raise ValueError("RegionGainedMeanScaleCompressor2018 trains with the block-weighted MSE only: "
                             f"DISTORTION_LOSS_NAMES [\"MSE\"] with REDUCTION \"mean\", got {names} with {reduction!r}")
        super().__init__(cfg)
        self._map = None
        self._codes = self._idx = self._weights = None

    # ---- quality
    @property
    def quality_map(self):
        """The map that was set (a copy), or None."""
        return None if self._map is None else self._map.copy()

    def set_quality_map(self, codes):
        """uint8 codes (Hb, Wb), shared by the batch, or (N, Hb, Wb); None: back to the uniform map of `quality`."""
        self._map = None if codes is None else _as_codes(codes)

    def set_quality(self, q):
        super().set_quality(q)
        self._map = None

    def _one_quality(self, who):
        return None if self._map is not None else super()._one_quality(who)

    def _call_map(self, N, H, W, who, each=False):
        """The codes (N, Hb, Wb) of a call on N images of padded size H x W; ValueError for a map of another shape."""
        hb, wb = -(-H // _codec.MAP_BLOCK), -(-W // _codec.MAP_BLOCK)
        if self._map is not None:
            m = self._map
            if m.shape[-2:] != (hb, wb) or (m.ndim == 3 and m.shape[0] != N):
                raise ValueError(f"{who}: the quality map {m.shape} is not the call's: {N} images of {hb} x {wb} blocks "
                                 f"(padded size {H} x {W} over {_codec.MAP_BLOCK})")
            return np.ascontiguousarray(np.broadcast_to(m, (N, hb, wb)))
        if each and isinstance(self._quality, list):
            if len(self._quality) != N:
                raise ValueError(f"compress_each: {len(self._quality)} qualities for {N} images")
            ks = [_codec.quality_code(q, self.levels) for q in self._quality]
        else:
            ks = [_codec.quality_code(self._one_quality(who), self.levels)] * N
        return np.ascontiguousarray(np.broadcast_to(np.asarray(ks, dtype=np.uint8)[:, None, None], (N, hb, wb)))

    def sample_map(self, N, hb, wb):
        """The next code map of the training sampler: one integer level per block, independent and uniform over the S
        levels (CPU generator, cfg.SEED)."""
        levels = torch.randint(0, self.levels, (N, hb, wb), generator=self._sampler).numpy()
        lut = np.asarray([_codec.quality_code(s, self.levels) for s in range(self.levels)], dtype=np.uint8)
        return lut[levels]

    def _use_map(self, codes, device, loss=False):
        """The rows and the rank indices of a call: U = the distinct codes ascending, one gain row per code, and for
        every block the rank of its code; `loss`: one distortion weight per code too (the forward)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        U, ranks = np.unique(codes, return_inverse=True)
        ranks = ranks.reshape(codes.shape).astype(np.uint8)
        self._codes = codes
        self._use([_codec.code_quality(int(u), self.levels) for u in U])
        self._idx = torch.from_numpy(ranks).to(device)
        if loss:
            w = np.asarray([self.loss_weight(q) for q in self._qualities], dtype=np.float64)
            self.distortion_loss_weight = float(w[ranks].mean())
            self._weights = torch.from_numpy(w.astype(np.float32)).to(device)

    def _clear(self):
        self._gains = self._qualities = self._codes = self._idx = self._weights = None

    # ---- the forward
    def forward(self, x):
        if x.dim() != 4:
            raise ValueError(f"forward: image batch {tuple(x.shape)} must be (N, C, H, W)")
        N, _, H, W = x.shape
        if self.training and (H % _codec.MAP_BLOCK or W % _codec.MAP_BLOCK):
            raise ValueError(f"forward: in training mode H and W must be multiples of {_codec.MAP_BLOCK} (whole blocks), "
                             f"got {H} x {W}")
        if not (self.training and self.sample_quality):
            self._call_map(N, H, W, "forward")   # in front of any launch
        return super().forward(x)

    def _forward(self, x):
        N, _, H, W = x.shape
        if self.training and self.sample_quality:
            codes = self.sample_map(N, H // _codec.MAP_BLOCK, W // _codec.MAP_BLOCK)
        else:
            codes = self._call_map(N, H, W, "forward")
        self.last_quality = codes
        try:
            self._use_map(codes, x.device, loss=True)
            return super(GainedMeanScaleCompressor2018, self)._forward(x)
        finally:
            self._clear()   # no graph kept alive by module state

    def _check_call(self, N, H, W, who):
        super()._check_call(N, H, W, who)   # one quality, or a map
        self._call_map(N, H, W, who)

    def _begin_call(self, N, H, W, device, who):
        self._use_map(self._call_map(N, H, W, who), device)

    def _end_call(self):
        self._clear()

    def _hyper_gain(self, z):
        return block_scale(z, self._gains[2], self._idx, 0)

    def _hyper_ungain(self, z_hat):
        return block_scale(z_hat, self._gains[3], self._idx, 0)

    def _latent_gain(self, y):
        return block_scale(y, self._gains[0], self._idx, 2)

    def _latent_ungain(self, y_hat):
        return block_scale(y_hat, self._gains[1], self._idx, 2)

    def distortion_loss(self, img1, img2):
        """{"MSE": (the block-weighted mean, the plain mean)} of one pass over the two images."""
        return {"MSE": block_mse(img1, img2, self._weights, self._idx)}

    def _losses(self, z_ce, y_ce, dist, num_pixels):
        weighted, plain = dist["MSE"]
        entropy = (z_ce + y_ce) / num_pixels
        return {
            "z_entropy": z_ce.detach() / num_pixels,
            "y_entropy": y_ce.detach() / num_pixels,
            "bpp": entropy.detach(),
            "total_loss": weighted + entropy,
            "MSE": plain.detach(),
        }

    # ---- bitstreams: containers "ICRM" and "ICRR" (codec.py)
    _containers = (_codec.pack_region, _codec.parse_region, _codec.pack_region_image, _codec.parse_region_image)

    def _codable(self):
        super()._codable()
        self._clear()

    def compress_each(self, x, steps_per_chunk=1024):
        if x.dim() == 4 and min(x.shape) >= 1:   # the map against the padded size, in front of any launch
            self._call_map(x.shape[0], *_codec.padded_size(*x.shape[2:]), "compress_each", each=True)
        return super().compress_each(x, steps_per_chunk)

    def compress_each_to(self, x, budgets, steps_per_chunk=1024, candidates=8, rounds=2, strict=True):
        raise ValueError("compress_each_to searches one quality per image, not a quality map: use compress_each_map_to, "
                         "which chooses the map for the budget, or GainedMeanScaleCompressor2018 for one quality")

    # ---- a quality map under a byte budget: the allocation rule of codec.py, the search rule on the coder's own sizes
    def _check_map_budget_call(self, x, budgets, steps_per_chunk, candidates, rounds, who):
        if x.dim() != 4 or min(x.shape) < 1:
            raise ValueError(f"{who}: image batch {tuple(x.shape)} must be (N, C, h, w) with h, w >= 1")
        if self.levels > _codec.MAP_MAX_LEVELS:
            raise ValueError(f"{who}: the allocation chooses among at most {_codec.MAP_MAX_LEVELS} levels, this model "
                             f"has {self.levels}")
        return self._check_budget_args(who, x.shape[0], "images", budgets, steps_per_chunk, candidates, rounds)

    def _level_tables(self, x, y, z):
        """(bits, sse), each float32 (N, S, Hb Wb): `rate_distortion_map`'s `bits` and `sse` of the batch at every
        integer level, from y = g_a(padded x) and z = h_a(y) computed once; x is the unpadded batch."""
        N = x.shape[0]
        H, W = _codec.padded_size(*x.shape[2:])
        hb, wb = H // _codec.MAP_BLOCK, W // _codec.MAP_BLOCK
        bits, sse = [], []
        try:
            for code in _codec.map_level_codes(self.levels):
                self._use_map(np.full((N, hb, wb), code, dtype=np.uint8), x.device)
                rd = self._rate_distortion_from(x, y, z)
                bits.append(rd.bits.reshape(N, hb * wb))
                sse.append(rd.sse.reshape(N, hb * wb))
        finally:
            self._clear()
        return torch.stack(bits, dim=1), torch.stack(sse, dim=1)

    @torch.no_grad()
    def rate_distortion_tables(self, x):
        """x (N, 3, h, w), any h, w >= 1 -> (bits, sse), each float32 (N, S, Hb Wb) on the device: the tables the
        allocation rule of codec.py reads, bit for bit the `bits` and `sse` of `rate_distortion_map(x)` after
        `set_quality(l)` for l = 0 .. S-1, from one pass of g_a and h_a.  Eval mode; `quality` and `quality_map` are
        neither read nor changed."""
        who = "rate_distortion_tables"
        if self.training:
            raise RuntimeError(f"{who} runs in eval mode only: call model.eval() first")
        if x.dim() != 4 or min(x.shape) < 1:
            raise ValueError(f"{who}: image batch {tuple(x.shape)} must be (N, C, h, w) with h, w >= 1")
        self._codable_each()
        xp, _ = self._pad_each(x)
        y = self.analysis_transform(xp)
        return self._level_tables(x, y, self.prior_analysis(self._hyper_input(y)))

    @torch.no_grad()
    def compress_each_map_to(self, x, budgets, steps_per_chunk=1024, candidates=8, rounds=2, strict=True):
        """x (N, 3, h, w) in [0, 1], any h, w >= 1, and `budgets` (one positive int, or N of them: bytes of the whole
        stream, header and map included) -> (a list of N "ICRR" streams, their quality maps: uint8 (Hb, Wb) arrays, the
        float32 slopes the maps were allocated at): for every image the map the allocation rule of codec.py gives at
        the slope its search rule chooses for the budget among `rounds` rounds of `candidates` slopes, so that
        len(stream) <= budget.  A stream is byte for byte what `set_quality_map(map)` and `compress_each` write for
        the image.  `quality` and `quality_map` are neither read nor changed.

        What is exact and what is an estimate: the per-block tables (`rate_distortion_tables`: the estimated bits and
        the squared error of every block at every integer level) only steer where the bits go, and a map is the exact
        minimiser of their tabulated sum and nothing more; the budget is enforced on the sizes the coder itself
        reports for every candidate map (`measure_seg`), h_s run image by image as the decoder runs it.

        g_a and h_a run once; the S passes of h_s and g_s for the tables run at batch N.  All candidates of all images
        of a round are allocated, symbolised and measured by one set of launches, the maps staying on the device; one
        small copy of the chunk lengths comes back per round.  Only the N chosen candidates are coded, and their maps
        copied to the host once.

        An image that fits at no slope of round 1: codec.BudgetError (a ValueError with .image, .budget, .smallest) in
        front of any packing; with strict=False it is coded with the map of slope 0 and is the one stream that may
        exceed its budget."""
        from ...functional import block_allocate, block_gain_symbolize_seg, measure_seg
        from ..blocks.entropy_model import symbolize_seg, symbols_as_tensor, table_pool
        who = "compress_each_map_to"
        budgets = self._check_map_budget_call(x, budgets, steps_per_chunk, candidates, rounds, who)
        self._codable_each()
        em, cm, R, S = self.entropy_model, self.conditional_model, int(steps_per_chunk), self.levels
        channels = x.shape[1]
        xp, (N, h, w, H, W) = self._pad_each(x)
        hb, wb = H // _codec.MAP_BLOCK, W // _codec.MAP_BLOCK
        y = self.analysis_transform(xp)
        z = self.prior_analysis(self._hyper_input(y))
        bits, sse = self._level_tables(x, y, z)
        level_codes = _codec.map_level_codes(S)
        z_tables, y_tables = {}, {}     # one table per K and tensor kind for the whole call

        def tables_z(K):
            if K not in z_tables:
                z_tables[K] = em.tables(K)
            return z_tables[K]

        def tables_y(K):
            if K not in y_tables:
                y_tables[K] = cm.tables(K, y.device)
            return y_tables[K]

        try:
            # one gain row per level: a row is a function of its code alone, so level indices serve as ranks
            self._use([_codec.code_quality(k, S) for k in level_codes])
            g_y, _, g_z, g_inv_z = self._gains
            self._codes = np.zeros((1, hb, wb), dtype=np.uint8)     # the fixed part does not depend on the map
            fixed = _codec.region_image_fixed_bytes(self._header(1, H, W, y, z, R, 0, 0, (h, w)))

            def measure(cands):
                img, ts = [n for n, _ in cands], [t for _, t in cands]
                M = len(cands)
                ws = [_codec.map_weight(self.loss_weight(t), channels) for t in ts]
                ranks, codes, _sums = block_allocate(bits, sse, img, ws, level_codes)
                ranks = ranks.view(M, hb, wb)
                try:
                    zc = z[torch.as_tensor(img, device=z.device)]
                    z_sym, kz = symbolize_seg(block_scale(zc, g_z, ranks, 0))
                    z_hat = block_scale(symbols_as_tensor(z_sym.to(torch.float32), (M, *z.shape[1:])), g_inv_z, ranks, 0)
                    sigma, mean = self._prior_each(z_hat)
                    y_sym, ky = block_gain_symbolize_seg(y, g_y, ranks, mean, img, 2)
                except ValueError as e:
                    raise ValueError(f"{who}: among the candidates (image, slope) {cands}: {e}") from None
                rows = cm.scale_rows(sigma.expand_as(mean))
                lz = measure_seg(z_sym, M, None, em.channels, *table_pool(tables_z, kz), R)
                ly = measure_seg(y_sym, M, rows, 0, *table_pool(tables_y, ky), R)
                lens = torch.cat([lz, ly]).cpu().numpy().astype(np.int64)    # the one D2H copy of the round
                lz, ly = lens[:lz.numel()].reshape(M, -1), lens[lz.numel():].reshape(M, -1)
                size = [_codec.image_stream_bytes(fixed, lz[m], ly[m]) for m in range(M)]
                nz, ny = z_sym.numel() // M, y_sym.numel() // M

                def keep(m):
                    return (z_sym[m * nz:(m + 1) * nz].clone(), kz[m], y_sym[m * ny:(m + 1) * ny].clone(), ky[m],
                            sigma[m:m + 1].clone(), mean[m:m + 1].clone(), size[m], codes[m].clone())
                return size, keep

            measured = {n: {} for n in range(N)}   # slope -> bytes, everything measured for the image so far
            todo = {n: _codec.budget_grid(S, candidates) for n in range(N)}
            chosen, kept = self._budget_rounds(dict(enumerate(budgets)), todo, measured, candidates, rounds, strict, measure)
            chosen, kept = [chosen[n] for n in range(N)], [kept[n] for n in range(N)]
            self._codes = torch.stack([k[7] for k in kept]).cpu().numpy().reshape(N, hb, wb)    # the maps, once
            z_sym, y_sym = (torch.cat([k[i] for k in kept]) for i in (0, 2))
            sigma, mean = (torch.cat([k[i] for k in kept]) for i in (4, 5))
            kz, ky = ([k[i] for k in kept] for i in (1, 3))
            sz = em.encode_symbols_seg(z_sym, kz, R)
            sy = cm.encode_symbols_seg(y_sym, ky, sigma.expand_as(y), R, mean=mean)
            streams = [self._pack_image(self._header(1, H, W, y, z, R, kz[n], ky[n], (h, w), n),
                                        sz[n][1], sy[n][1], sz[n][0], sy[n][0]) for n in range(N)]
            maps = [self._codes[n].copy() for n in range(N)]
        finally:
            self._clear()
        for n, s in enumerate(streams):
            if len(s) != kept[n][6]:
                raise RuntimeError(f"{who}: the stream of image {n} at slope {chosen[n]} holds {len(s)} bytes, "
                                   f"{kept[n][6]} were measured")
        return streams, maps, chosen

    def _transcode_qualities(self, qualities, M, who):
        raise ValueError(f"{who}: the streams of RegionGainedMeanScaleCompressor2018 carry a quality map: requantizing a "
                         "map to another map is not built; leave `qualities` None to re-chunk")

    def transcode_each_to(self, streams, budgets, steps_per_chunk=None, candidates=8, rounds=2, strict=True):
        raise ValueError("transcode_each_to searches one quality per stream: a byte budget for a quality map is not "
                         "built; use GainedMeanScaleCompressor2018 for budgets")

    def _analyse(self, x, each=False):
        N, _, H, W = x.shape
        self._use_map(self._call_map(N, H, W, "compress_each" if each else "compress", each), x.device)
        return super(GainedMeanScaleCompressor2018, self)._analyse(x, each)

    def _header(self, N, H, W, y, z, steps_per_chunk, kz, ky, size=None, image=0):
        h = super(GainedMeanScaleCompressor2018, self)._header(N, H, W, y, z, steps_per_chunk, kz, ky, size)
        codes = self._codes if size is None else self._codes[image]
        return (_codec.RegionHeader if size is None else _codec.RegionImageHeader)(
            **vars(h), levels=self.levels, map_h=codes.shape[-2], map_w=codes.shape[-1], codes=np.ascontiguousarray(codes))

    def _begin_decode(self, headers):
        codes = headers[0].codes if len(headers) == 1 and headers[0].codes.ndim == 3 else np.stack([h.codes for h in headers])
        self._use_map(codes, next(self.parameters()).device)

    def _begin_window_decode(self, hs, plans):
        """Every window's own blocks of its stream's map: a latent window is whole blocks (codec.LATENT_SNAP), and a
        gain row is a function of its code alone, so the cropped map gives the window the gains of the whole one."""
        n = _codec.LATENT_SNAP
        codes = np.stack([h.codes[p.rows[0] // n:p.rows[1] // n, p.cols[0] // n:p.cols[1] // n] for h, p in zip(hs, plans)])
        self._use_map(codes, next(self.parameters()).device)
