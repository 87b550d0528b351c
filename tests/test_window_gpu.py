"""Decoding a pixel window of a per-image stream on the GPU: the window decoder against the segmented decoder
(bitwise, with and without a mean and per-symbol rows), `crop_clamp_at` against the bound pair and the slice, and
`decompress_window` of the scale, mean-scale, gained and region models against `decompress_each`: the latent windows
bitwise, the pixels by the project's bar for streams decoded in another grouping; only the planned bytes are read;
a bytes object given several times is parsed, z-decoded and passed through h_s once."""
import functools

import numpy as np
import pytest
import torch

from test_codec import draw, random_tables
from test_codec_gpu import _model as _scale_model
from test_gained_gpu import _model as _gained_model, _tables as _gain_tables
from test_mean_scale_gpu import _changed, _model as _mean_model
from test_region_gpu import _region_of
from test_stream_gpu import SEG_KS, _scaled

pytestmark = pytest.mark.gpu

DEV = "cuda"
HY, WY, C = 8, 11, 192                  # the latent of every segment of the op test: 16,896 symbols
SEG_LEN = HY * WY * C
KIND = "LaplacianConditionalModel"


def _wops():
    from image_compression_amd import _lib
    return _lib.window_ops()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. the op against the existing decoder
@functools.lru_cache(maxsize=None)
def _coded(R, mode):
    """Three segments, K = 1, 37 and 2047, random symbols coded by encode_seg at R; "rows": a random row of 64 per
    symbol (K = 1 and 37 staged in LDS, 2047 read from the pool), "channel": the z rule g % C on 192 rows (K = 1
    staged, 37 and 2047 from the pool).  -> what the decoders take, and decode_seg's output (3, HY, WY, C)."""
    from image_compression_amd import _lib, codec
    nrows = 64 if mode == "rows" else C
    rng = np.random.default_rng(R + nrows)
    tables = {K: random_tables(np.random.default_rng(K + nrows), nrows, K) for K in SEG_KS}
    offs, at = {}, 0
    for K in SEG_KS:
        offs[K], at = at, at + tables[K].size
    pool = torch.from_numpy(np.concatenate([tables[K].ravel() for K in SEG_KS]).astype(np.int32)).to(DEV)
    rows_np = [rng.integers(0, nrows, SEG_LEN) if mode == "rows" else (s * SEG_LEN + np.arange(SEG_LEN)) % C
               for s in range(3)]
    sym = np.concatenate([draw(rng, tables[K], r) - K for K, r in zip(SEG_KS, rows_np)]).astype(np.int32)
    rows = torch.from_numpy(np.concatenate(rows_np).astype(np.uint8)).to(DEV) if mode == "rows" else None
    ks, to = list(SEG_KS), [offs[K] for K in SEG_KS]
    ops = _lib.stream_ops()
    packed = ops.encode_seg(torch.from_numpy(sym).to(DEV), 3, rows, C, pool, nrows, ks, to, R)
    parts = codec.split_packed_seg(packed.cpu().numpy(), 3, SEG_LEN, R)      # [(lengths, payload)] per segment
    joined = torch.from_numpy(codec.join_packed_seg(parts).copy()).to(DEV)
    flat = ops.decode_seg(joined, 3, SEG_LEN, rows, C, pool, nrows, ks, to, R)
    assert np.array_equal(flat.cpu().numpy(), sym.astype(np.float32)), "decode_seg does not return the symbols"
    mu = torch.randn(3 * SEG_LEN, generator=torch.Generator().manual_seed(R)).mul_(3.0).to(DEV)
    mu[::7] = -0.0
    with_mu = _lib.mean_ops().add_mean(flat, mu)
    return dict(parts=parts, rows=rows, pool=pool, nrows=nrows, ks=ks, offs=to, R=R, mu=mu,
                ref=flat.view(3, HY, WY, C), ref_mu=with_mu.view(3, HY, WY, C))


def _decode_windows(coded, wins, rh, rw, mu):
    """One launch for `wins` = [(segment, r0, c0)], all of shape rh x rw: the payload of the spanned chunks alone."""
    per = 64 * coded["R"]
    parts, windows, spans, words = [], [], [], 0
    for s, r0, c0 in wins:
        lens, payload = coded["parts"][s]
        ends = np.concatenate(([0], np.cumsum(lens.astype(np.int64))))
        k0, k1 = r0 * WY * C // per, -(-(r0 + rh) * WY * C // per)
        parts.append(payload[int(ends[k0]):int(ends[k1])])
        spans += [words + int(e - ends[k0]) // 2 for k in range(k0, k1) for e in (ends[k], ends[k + 1])]
        words += len(parts[-1]) // 2
        windows += [s * SEG_LEN, coded["offs"][s], HY, WY, coded["ks"][s], r0, c0, k0, k1]
    buf = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to(DEV)
    return _wops().decode(buf, windows, rh, rw, spans, coded["rows"], mu, C, coded["pool"], coded["nrows"], coded["R"])


# (rh, rw, [(segment, r0, c0)]): one position, the last row, a column strip, an interior 4 x 4, the whole latent --
# each in all three segments, which mixes staged and pooled tables in a launch -- and two windows of one segment
WINDOW_CASES = [
    (1, 1, [(0, 3, 5), (1, 0, 0), (2, 7, 10)]),
    (1, WY, [(0, 7, 0), (1, 7, 0), (2, 7, 0)]),
    (HY, 2, [(0, 0, 4), (1, 0, 9), (2, 0, 0)]),
    (4, 4, [(0, 2, 3), (1, 2, 3), (2, 1, 6)]),
    (HY, WY, [(0, 0, 0), (1, 0, 0), (2, 0, 0)]),
    (4, 4, [(1, 0, 0), (1, 4, 7), (2, 4, 0), (1, 3, 3)]),
]


@pytest.mark.parametrize("mode", ["rows", "channel"])
@pytest.mark.parametrize("R", [5, 1024])
def test_window_decoder_is_the_segmented_decoder_cropped(R, mode):
    """R = 5: 320-symbol chunks cut rows and channel vectors and leave a short last chunk; R = 1024: one chunk."""
    coded = _coded(R, mode)
    assert len(coded["parts"][0][0]) == -(-SEG_LEN // (64 * R)) and (R == 1024 or SEG_LEN % (64 * R))
    for rh, rw, wins in WINDOW_CASES:
        for mu, ref in ((None, coded["ref"]), (coded["mu"], coded["ref_mu"])):
            got = _decode_windows(coded, wins, rh, rw, mu)
            assert got.shape == (len(wins), rh, rw, C) and got.dtype == torch.float32 and got.is_contiguous()
            for k, (s, r0, c0) in enumerate(wins):
                want = ref[s, r0:r0 + rh, c0:c0 + rw]
                assert torch.equal(_bits(got[k]), _bits(want)), (rh, rw, s, r0, c0, mu is not None)


def test_window_decoder_keeps_every_read_inside_its_span():
    """Any payload bytes under valid descriptors: wrong symbols of the segment's own alphabet, nothing else."""
    coded = dict(_coded(5, "rows"))
    rng = np.random.default_rng(2)
    coded["parts"] = [(lens, rng.integers(0, 256, len(p), dtype=np.uint8).tobytes()) for lens, p in coded["parts"]]
    got = _decode_windows(coded, [(0, 2, 3), (1, 2, 3), (2, 1, 6)], 4, 4, None).cpu().numpy()
    assert np.array_equal(got, np.round(got))
    for k, K in enumerate(SEG_KS):
        assert np.abs(got[k]).max() <= K


def test_window_op_refuses_bad_descriptors():
    coded = _coded(5, "rows")
    ops, buf = _wops(), torch.zeros(4096, dtype=torch.uint8, device=DEV)
    good = [0, coded["offs"][0], HY, WY, 1, 0, 0, 0, 7]            # rows [0, 1): 2112 symbols, chunks [0, 7)
    spans = [v for k in range(7) for v in (128 * k, 128 * k + 128)]
    args = (coded["rows"], None, C, coded["pool"], coded["nrows"], 5)
    assert ops.decode(buf, good, 1, WY, spans, *args).shape == (1, 1, WY, C)
    for field, value in ((5, 8), (6, 1), (4, 2048), (1, coded["pool"].numel()), (0, 2 * SEG_LEN + 1), (7, 1), (8, 6)):
        bad = list(good)
        bad[field] = value
        with pytest.raises(RuntimeError, match="1001"):      # the spans are those of the range that is named
            ops.decode(buf, bad, 1, WY, spans[:2 * (bad[8] - bad[7])], *args)
    with pytest.raises(RuntimeError, match="1001"):
        ops.decode(buf, good, 1, WY, spans[:-1] + [2049], *args)      # a span past the buffer
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. crop_clamp_at
def test_crop_clamp_at_is_the_bound_pair_then_the_slice():
    from image_compression_amd.modelling.layers import LowerBound, UpperBound
    x = torch.rand(2, 3, 40, 96, generator=torch.Generator().manual_seed(3)) * 3.0 - 1.0
    x[0, 0, 0, 0], x[1, 2, 5, 7], x[0, 1, 3, 3], x[1, 0, 1, 1] = float("nan"), float("inf"), -float("inf"), -0.0
    x = x.to(DEV)
    want = LowerBound.apply(UpperBound.apply(x, 1.), 0.)
    srcs = (x, x.contiguous(memory_format=torch.channels_last), x[1:2])
    for width in range(1, 68):
        top, left = (0, 5, 1, 17)[width % 4], (0, 3, 29, 8)[(width // 4) % 4]      # 0 and odd offsets; 29 + 67 = 96
        height = 1 + (7 * width) % (40 - top)
        for src in srcs:
            got = _wops().crop_clamp_at(src, top, left, height, width)
            ref = (want if src.shape[0] == 2 else want[1:2])[:, :, top:top + height, left:left + width]
            assert got.is_contiguous() and got.shape == ref.shape
            assert torch.equal(_bits(got), _bits(ref)), (top, left, height, width)      # bitwise, NaN and -0 too
    got = _wops().crop_clamp_at(x, 0, 0, 40, 96)                                        # the whole tensor
    assert torch.equal(_bits(got), _bits(want))
    got = _wops().crop_clamp_at(x, 39, 95, 1, 1)
    assert torch.equal(_bits(got), _bits(want[:, :, 39:, 95:]))


# ------------------------------------------------------------------ 3. the models
H_IMG, W_IMG = 200, 328                 # padded to 256 x 384: y is 16 x 24
BOXES = [(0, 0, H_IMG, W_IMG), (0, 0, 1, 1), (H_IMG - 1, W_IMG - 1, 1, 1), (37, 51, 90, 101),
         (150, 250, 50, 78)]            # the last touches the bottom-right corner, which lies in the padded block
MODELS = ["scale", "mean", "gained", "region"]


def _images():
    return torch.rand(2, 3, H_IMG, W_IMG, generator=torch.Generator().manual_seed(11)).to(DEV)


class _setup:
    """The model of `name` with its weights changed as the existing tests change them ("x32": the last analysis conv
    times 32; the mean-scale model's prior_mean.bias = 0.37; the gain tables at fixed random values; two images at
    different qualities; a map with three distinct codes); everything is put back on exit."""

    def __init__(self, name, scaled):
        self.name = name
        if name == "scale":
            self.model = _scale_model(KIND, "fp32_split")
            self.ctx = [_scaled(self.model, scaled)]
        elif name == "mean":
            self.model = _mean_model(KIND, "fp32_split")
            self.ctx = [_changed(self.model, scaled, bias=0.37)]
        else:
            self.model = _gained_model(KIND, "fp32_split") if name == "gained" else _region_of(KIND, "fp32_split")
            self.ctx = [_changed(self.model, scaled), _gain_tables(self.model)]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()
        m = self.model
        if self.name == "gained":
            self.saved = m._quality
            m.set_quality([1.0, 3.5])
        elif self.name == "region":
            self.saved = (m._quality, m._map)
            codes = np.zeros((2, 4, 6), dtype=np.uint8)
            codes[0, 1:3, 2:5], codes[0, 3, :], codes[1, :, ::2], codes[1, 2, 1] = 255, 102, 102, 255
            assert len(np.unique(codes[0])) == 3 and len(np.unique(codes[1])) == 3
            m.set_quality_map(codes)
        return m

    def __exit__(self, *exc):
        if self.name == "gained":
            self.model._quality = self.saved
        elif self.name == "region":
            self.model._quality, self.model._map = self.saved
        for c in reversed(self.ctx):
            c.__exit__(*exc)


def _full_decode(model, streams):
    """(decompress_each's images, what it handed g_s: the latents of the streams in order)."""
    seen = []
    orig = model._reconstruct_each
    model._reconstruct_each = lambda y_hat, hs: (seen.append(y_hat), orig(y_hat, hs))[1]
    try:
        full = model.decompress_each(streams)
    finally:
        del model._reconstruct_each
    assert len(seen) == 1 and seen[0].shape[0] == len(streams)
    return full, seen[0]


def _close(got, want, whole, name):
    """The bar of test_model_round_trip_each (conftest.assert_close at 1e-4) on the pixels of a box: |got - want| <=
    1e-4 max|reconstruction the box is cropped from| + 1e-4 |want|.  Prints the largest difference first."""
    d = (got.double() - want.double()).abs()
    bound = 1e-4 * float(whole.abs().max()) + 1e-4 * want.double().abs()
    print(f"{name}: max |window - crop| = {float(d.max()):.3e}")
    assert bool((d <= bound).all()), (name, float(d.max()))


@pytest.mark.parametrize("R", [16, 1024])
@pytest.mark.parametrize("scaled", [False, True], ids=["seed", "x32"])
@pytest.mark.parametrize("name", MODELS)
def test_model_windows(name, scaled, R):
    x = _images()
    with _setup(name, scaled) as model:
        streams = model.compress_each(x, steps_per_chunk=R)
        full, y_full = _full_decode(model, streams)
        wstreams = [streams[n] for n in range(2) for _ in BOXES]
        wboxes = [b for _ in range(2) for b in BOXES]
        plans, groups = model._window_latents(wstreams, wboxes)
        assert sorted(m for idx, _ in groups for m in idx) == list(range(len(wboxes)))
        for idx, lat in groups:
            for k, m in enumerate(idx):
                (r0, r1), (c0, c1) = plans[m].rows, plans[m].cols
                assert lat.shape[1:] == (192, r1 - r0, c1 - c0)
                want = y_full[m // len(BOXES), :, r0:r1, c0:c1]
                assert torch.equal(_bits(lat[k]), _bits(want)), (name, wboxes[m], "the latent window")
        nchunks = -(-16 * 24 * 192 // (64 * R))      # 72 chunks of y at R = 16, 2 at 1024
        assert all(0 <= k0 < k1 <= nchunks for k0, k1 in (p.chunks for p in plans))
        assert R != 16 or min(k1 - k0 for k0, k1 in (p.chunks for p in plans)) < nchunks // 2
        got = model.decompress_window(wstreams, wboxes)
        assert len(got) == len(wboxes)
        for m, (img, (top, left, height, width)) in enumerate(zip(got, wboxes)):
            n = m // len(BOXES)
            assert img.shape == (1, 3, height, width) and img.is_contiguous() and img.dtype == torch.float32
            assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
            _close(img, full[n][:, :, top:top + height, left:left + width], full[n],
                   f"{name} {'x32' if scaled else 'seed'} R={R} image {n} box {(top, left, height, width)}")


# ------------------------------------------------------------------ 4. only the planned bytes are read
@pytest.mark.parametrize("name", ["mean", "region"])
def test_only_the_planned_bytes_are_read(name):
    from image_compression_amd import codec
    box = (37, 51, 90, 101)
    with _setup(name, True) as model:
        stream = model.compress_each(_images(), steps_per_chunk=16)[0]
        header, lz, ly, _pz, _py = model._parse_image(stream, *model._build_id())
        kernel, strides = model._synthesis_geometry
        plan = codec.window_plan(header, box, kernel, strides, lengths=(lz, ly))
        k0, k1 = plan.chunks
        assert len(ly) == 72 and k1 - k0 < len(ly), "the box must leave at least one chunk of y unspanned"
        keep = np.zeros(len(stream), dtype=bool)
        for a, b in plan.byte_ranges:
            keep[a:b] = True
        assert 0 < int((~keep).sum()) == int(ly.sum()) - int(ly[k0:k1].sum())
        spoilt = np.frombuffer(stream, dtype=np.uint8).copy()
        spoilt[~keep] = 0xFF
        spoilt = spoilt.tobytes()
        assert spoilt != stream
        want = model.decompress_window([stream], [box])[0]
        got = model.decompress_window([spoilt], [box])[0]
        assert torch.equal(_bits(got), _bits(want))
        # and the bytes that are planned do matter: the same treatment of a spanned chunk changes the window
        # (a chunk in the middle of the range: latent row 6, columns 0 .. 5, which the box's pixels depend on)
        y_at, mid = len(stream) - int(ly.sum()), (k0 + k1) // 2
        a = y_at + int(ly[:mid].sum())
        hit = np.frombuffer(stream, dtype=np.uint8).copy()
        hit[a:a + int(ly[mid])] = 0xFF
        assert not torch.equal(model.decompress_window([hit.tobytes()], [box])[0], want)


# ------------------------------------------------------------------ 5. sharing
def test_tiles_of_one_stream_share_z_and_h_s():
    tiles = [(0, 0, 60, 100), (0, 100, 60, 228), (60, 0, 140, 100), (60, 100, 140, 228)]      # latent windows 8 x 12 .. 16 x 20
    with _setup("mean", True) as model:
        stream = model.compress_each(_images()[:1], steps_per_chunk=16)[0]
        calls = []
        orig = model._prior
        model._prior = lambda z_hat: (calls.append(tuple(z_hat.shape)), orig(z_hat))[1]
        try:
            plans, _ = model._window_latents([stream] * 4, tiles)
            assert len({p.shape for p in plans}) == 4, "four latent shapes: every tile passes g_s alone in both calls"
            calls.clear()
            together = model.decompress_window([stream] * 4, tiles)
            assert calls == [(1, 192, 4, 6)], calls                 # z whole, h_s once, at batch shape 1
            calls.clear()
            alone = [model.decompress_window([stream], [t])[0] for t in tiles]
            assert len(calls) == 4
            calls.clear()
            model.decompress_window([stream, bytes(bytearray(stream))], tiles[:2])
            assert len(calls) == 2, "an equal copy is another object: it is parsed and decoded on its own"
        finally:
            del model._prior
        for t, a, b in zip(tiles, together, alone):
            assert a.shape == (1, 3, t[2], t[3]) and torch.equal(_bits(a), _bits(b)), t
        # the tiles put together are the image, by the bar of the model test
        full = model.decompress_each([stream])[0]
        whole = torch.cat([torch.cat(together[:2], dim=3), torch.cat(together[2:], dim=3)], dim=2)
        _close(whole, full, full, "four tiles")
