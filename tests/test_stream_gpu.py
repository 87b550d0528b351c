"""Per-image streams on the GPU: the segmented rANS kernels against the numpy reference coder of
tests/test_codec.py (stream s = the reference encoding of segment s alone), symbolize_seg, the pad / crop
kernels, and the model's compress_each / decompress_each: round trip against the eval forward, every stream
decodable alone and in any company, the tie to compress(), and the rate."""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from test_codec import draw, random_tables, ref_decode, ref_encode
from test_codec_gpu import _model

pytestmark = pytest.mark.gpu

DEV = "cuda"
NROWS = 64
SEG_KS = (1, 37, 2047)          # 64 rows: K = 1 and 37 are staged in LDS (19 KiB at 37), K = 2047 (1 MiB) is not
# (segment length, steps per chunk): one symbol, a partial step, one past a chunk, exactly two chunks, and the
# default chunk size with a second, short chunk
SEG_CASES = [(1, 4), (63, 4), (64 * 4 + 1, 4), (2 * 64 * 4, 4), (65536 + 5, 1024)]


def _ops():
    from image_compression_amd import _lib
    return _lib.stream_ops()


@functools.lru_cache(maxsize=None)
def _tables(K):
    return random_tables(np.random.default_rng(K), NROWS, K)


@functools.lru_cache(maxsize=None)
def _pool():
    """The tables of SEG_KS back to back on the device, and each one's word offset."""
    offs, at = {}, 0
    for K in SEG_KS:
        offs[K] = at
        at += _tables(K).size
    flat = np.concatenate([_tables(K).ravel() for K in SEG_KS]).astype(np.int32)
    return torch.from_numpy(flat).to(DEV), offs


@functools.lru_cache(maxsize=None)
def _segments(seg_len, R, nseg, mode):
    """Per segment (K, rows, symbol indices drawn from its own table, reference payload, reference lengths);
    C = the channel count of the "channel" mode: segment starts must be multiples of it."""
    ks = (37,) if nseg == 1 else SEG_KS
    C = max(c for c in range(1, 8) if seg_len % c == 0)
    rng = np.random.default_rng(seg_len + 7 * nseg)
    segs = []
    for s, K in enumerate(ks):
        rows = rng.integers(0, NROWS, seg_len) if mode == "rows" else (s * seg_len + np.arange(seg_len)) % C
        idx = draw(rng, _tables(K), rows)
        if seg_len > 2:
            idx[0], idx[-1] = 0, 2 * K            # the ends of the alphabet are coded too
        payload, lens = ref_encode(idx, rows, _tables(K), R)
        segs.append((K, rows, idx, payload, lens))
    return segs, C


def _device_args(segs, mode):
    pool, offs = _pool()
    sym = torch.from_numpy(np.concatenate([idx - K for K, _, idx, _, _ in segs]).astype(np.int32)).to(DEV)
    rows = torch.from_numpy(np.concatenate([r for _, r, _, _, _ in segs]).astype(np.uint8)).to(DEV) if mode == "rows" \
        else None
    return sym, rows, pool, [K for K, *_ in segs], [offs[K] for K, *_ in segs]


def _packed(segs, order):
    from image_compression_amd import codec
    return torch.from_numpy(codec.join_packed_seg([(segs[s][4], segs[s][3]) for s in order]).copy()).to(DEV)


@pytest.mark.parametrize("mode", ["rows", "channel"])
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("seg_len,R", SEG_CASES)
def test_segmented_coder_matches_the_reference_coder(seg_len, R, nseg, mode):
    from image_compression_amd import codec
    ops = _ops()
    segs, C = _segments(seg_len, R, nseg, mode)
    sym, rows, pool, ks, offs = _device_args(segs, mode)
    packed = ops.encode_seg(sym, nseg, rows, C, pool, NROWS, ks, offs, R)
    cps = -(-seg_len // (64 * R))
    assert packed.numel() == nseg * cps * (4 + 2 * 64 * R + 256)
    got = codec.split_packed_seg(packed.cpu().numpy(), nseg, seg_len, R)
    for s, (K, r, idx, payload, lens) in enumerate(segs):
        assert np.array_equal(got[s][0], lens), f"chunk lengths of segment {s} (K = {K})"
        assert got[s][1] == payload, f"payload of segment {s} (K = {K}) differs from the reference encoder's"
        assert np.array_equal(ref_decode(got[s][1], got[s][0], seg_len, r, _tables(K), R), idx)
    want = np.concatenate([idx - K for K, _, idx, _, _ in segs]).astype(np.float32)
    out = ops.decode_seg(_packed(segs, range(nseg)), nseg, seg_len, rows, C, pool, NROWS, ks, offs, R)
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), want), "decode_seg"
    if nseg > 1:
        # the streams in another order (with their rows, K and tables) give the symbols in that order; in
        # the channel mode the row is the global index % C, the same in every order as seg_len % C == 0
        order = [2, 0, 1]
        rows_p = None if rows is None else torch.cat([rows[s * seg_len:(s + 1) * seg_len] for s in order])
        out = ops.decode_seg(_packed(segs, order), nseg, seg_len, rows_p, C, pool, NROWS, [ks[s] for s in order],
                             [offs[s] for s in order], R)
        assert np.array_equal(out.cpu().numpy(), want.reshape(nseg, seg_len)[order].ravel()), "permuted decode_seg"


@pytest.mark.parametrize("mode", ["rows", "channel"])
def test_segmented_decoder_maps_any_payload_into_each_segments_alphabet(mode):
    """The length tables are kept and only payload bytes replaced: every read stays inside its chunk's
    [begin, end) and every search inside its row by the decoder's guards, so wrong bytes give wrong symbols of
    the segment's own alphabet and nothing else."""
    seg_len, R, nseg = 64 * 4 + 1, 4, 3
    segs, C = _segments(seg_len, R, nseg, mode)
    _, rows, pool, ks, offs = _device_args(segs, mode)
    buf = _packed(segs, range(nseg)).cpu().numpy().copy()
    head = 4 * nseg * 2
    buf[head:] = np.random.default_rng(1).integers(0, 256, buf.size - head, dtype=np.uint8)
    out = _ops().decode_seg(torch.from_numpy(buf).to(DEV), nseg, seg_len, rows, C, pool, NROWS, ks, offs, R)
    out = out.cpu().numpy().reshape(nseg, seg_len)
    assert np.array_equal(out, np.round(out))
    for s, K in enumerate(ks):
        assert np.abs(out[s]).max() <= K, (s, K)


def test_symbolize_seg_is_torch_round_with_the_exact_maximum_of_every_image():
    from image_compression_amd.modelling.blocks.entropy_model import symbolize_seg
    v = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -0.3, 0.3, 7.49, -6.5, 0.0, -0.0, 4.5])
    x = v.repeat(60)[:3 * 4 * 7 * 9].view(3, 4, 7, 9).clone()          # (N, C, H, W): 252 values per image
    x[1, 2, 3, 4], x[2, 0, 6, 8] = -2046.5, 2047.49
    x = x.to(DEV)
    sym, kmax = symbolize_seg(x)
    assert sym.dtype == torch.int32 and kmax == [7, 2046, 2047]
    assert torch.equal(sym.cpu(), torch.round(x.cpu()).movedim(1, -1).reshape(-1).to(torch.int32))
    assert symbolize_seg(x[:1])[1] == [7]
    for bad in (2047.5, -2048.0, 1e20, float("inf"), float("nan")):
        x[1, 0, 0, 0] = bad                                             # |q| = 2048 and beyond, in image 1
        with pytest.raises(ValueError, match="image 1 .*2047"):
            symbolize_seg(x)


@pytest.mark.parametrize("h,w", [(72, 100), (65, 1), (1, 1)])
def test_pad_edge_is_replicate_padding(h, w):
    from image_compression_amd import codec
    x = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h + w))
    Hp, Wp = codec.padded_size(h, w)
    got = _ops().pad_edge(x.to(DEV), Hp, Wp)
    assert got.is_contiguous() and torch.equal(got.cpu(), F.pad(x, (0, Wp - w, 0, Hp - h), mode="replicate"))


@pytest.mark.parametrize("h,w", [(72, 100), (65, 1), (1, 1), (128, 128)])
def test_crop_clamp_is_the_bound_pair_then_the_slice(h, w):
    from image_compression_amd.modelling.layers import LowerBound, UpperBound
    x = (torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(3)) * 3.0 - 1.0)
    x[0, 0, 0, 0], x[1, 2, 0, 0], x[0, 1, 0, 0], x[1, 0, 0, 0] = float("nan"), float("inf"), -float("inf"), -0.0
    x = x.to(DEV)
    want = LowerBound.apply(UpperBound.apply(x, 1.), 0.)[:, :, :h, :w]
    for src in (x, x.contiguous(memory_format=torch.channels_last), x[1:2]):
        got = _ops().crop_clamp(src, h, w)
        ref = want if src.shape[0] == 2 else want[1:2]
        assert got.is_contiguous() and got.shape == ref.shape
        assert torch.equal(got.view(torch.int32), ref.contiguous().view(torch.int32))     # bitwise, NaN and -0 too


# ------------------------------------------------------------------ the model
SHAPES = [(3, 3, 72, 100), (2, 3, 64, 192), (1, 3, 65, 1)]
R_MODEL = 16            # every image has several chunks (y of a 64 x 64 padded image: 3072 symbols = 3 chunks)


def _batch(shape):
    """Images that differ: uniform noise, a constant 0.5, noise x 0.25 (then again from the start)."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand(*shape, generator=g)
    if shape[0] > 1:
        x[1] = 0.5
    if shape[0] > 2:
        x[2] *= 0.25
    return x.to(DEV)


def _last_analysis_conv(model):
    return [m for m in model.analysis_transform.modules() if hasattr(m, "weight") and m.weight.dim() == 4][-1]


class _scaled:
    """The existing "x32" scaling of the last analysis conv (symbols up to a few dozen), undone on exit."""

    def __init__(self, model, on):
        self.w, self.on = _last_analysis_conv(model).weight, on

    def __enter__(self):
        if self.on:
            with torch.no_grad():
                self.w.mul_(32.0)

    def __exit__(self, *exc):
        if self.on:
            with torch.no_grad():
                self.w.div_(32.0)


def _pad(x):
    from image_compression_amd import codec
    Hp, Wp = codec.padded_size(*x.shape[2:])
    return F.pad(x, (0, Wp - x.shape[3], 0, Hp - x.shape[2]), mode="replicate")


@pytest.mark.parametrize("scaled", [False, True], ids=["seed", "x32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["3x72x100", "2x64x192", "1x65x1"])
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", ["LaplacianConditionalModel", "GaussianConditionalModel"])
def test_model_round_trip_each(kind, dtype, shape, scaled):
    from image_compression_amd import codec
    model = _model(kind, dtype)
    x = _batch(shape)
    N, _, h, w = shape
    with _scaled(model, scaled):
        with torch.no_grad():
            want = model(_pad(x))[0][:, :, :h, :w]
        streams = model.compress_each(x, steps_per_chunk=R_MODEL)
        assert len(streams) == N and all(isinstance(s, bytes) for s in streams)
        assert model.compress_each(x, steps_per_chunk=R_MODEL) == streams, "compressing twice gives different bytes"
        heads = [codec.parse_image(s, 4, dtype)[0] for s in streams]
        print(f"each {kind[:5]} {dtype} {shape} {'x32' if scaled else 'seed'}: kmax_z {[hd.kmax_z for hd in heads]} "
              f"kmax_y {[hd.kmax_y for hd in heads]} bytes {[len(s) for s in streams]}")
        for hd in heads:
            assert (hd.N, hd.height, hd.width, hd.R) == (1, h, w, R_MODEL)
            assert (hd.H, hd.W) == codec.padded_size(h, w)
            assert codec.num_chunks(hd.nsym_y, hd.R) >= 3
        if scaled and N == 3:
            assert len({hd.kmax_y for hd in heads}) >= 2, "the images of the batch share one kmax_y"
        # decoded together, in order: the same batch through the same kernels -> the eval forward, bitwise
        got = model.decompress_each(streams)
        assert len(got) == N
        for n in range(N):
            assert got[n].shape == (1, 3, h, w) and got[n].is_contiguous()
            assert torch.equal(got[n][0], want[n]), f"image {n} is not the eval forward's reconstruction"
        # every stream alone, the list reversed, and in the company of streams of another size: g_s runs on
        # another batch (its low bits may follow the grouping), sigma and so the symbols may not change
        ref = want.cpu().numpy()
        for n in range(N):
            assert_close(model.decompress_each([streams[n]])[0][0].cpu().numpy(), ref[n], 1e-4, f"image {n} alone")
        for n, img in zip(reversed(range(N)), model.decompress_each(streams[::-1])):
            assert_close(img[0].cpu().numpy(), ref[n], 1e-4, f"image {n} reversed")
        x2 = torch.rand(1, 3, 40, 130, generator=torch.Generator().manual_seed(9)).to(DEV)
        with torch.no_grad():
            want2 = model(_pad(x2))[0][:, :, :40, :130].cpu().numpy()
        other = model.compress_each(x2, steps_per_chunk=R_MODEL)
        mixed = model.decompress_each([streams[0], other[0]] + streams[1:])
        assert [tuple(t.shape) for t in mixed] == [(1, 3, h, w), (1, 3, 40, 130)] + [(1, 3, h, w)] * (N - 1)
        assert_close(mixed[1].cpu().numpy(), want2, 1e-4, "the other size")
        for n, img in zip(range(N), [mixed[0]] + mixed[2:]):
            assert_close(img[0].cpu().numpy(), ref[n], 1e-4, f"image {n} mixed")


def _same_but_for_the_image_size(image_header, header):
    a = dataclasses.asdict(image_header)
    return (a.pop("height"), a.pop("width")) == (header.H, header.W) and a == dataclasses.asdict(header)


@pytest.mark.parametrize("scaled", [False, True], ids=["seed", "x32"])
def test_single_image_stream_carries_the_bitstreams_of_compress(scaled):
    from image_compression_amd import codec
    model = _model("LaplacianConditionalModel", "fp32_split")
    x = _batch((1, 3, 64, 128))
    with _scaled(model, scaled):
        each = codec.parse_image(model.compress_each(x)[0], 4, "fp32_split")
        batch = codec.parse(model.compress(x), 4, "fp32_split")
    assert _same_but_for_the_image_size(each[0], batch[0]), "only the container differs"
    assert np.array_equal(each[1], batch[1]) and np.array_equal(each[2], batch[2]), "chunk lengths"
    assert each[3] == batch[3] and each[4] == batch[4], "payloads"


@pytest.mark.parametrize("scaled", [False, True], ids=["seed", "x32"])
@pytest.mark.parametrize("shape", [(3, 3, 72, 100), (2, 3, 64, 192)], ids=["3x72x100", "2x64x192"])
def test_rate_of_every_stream(shape, scaled):
    """Each stream's coded bits against the ideal code length of its symbols under the tables it was coded
    with, by the bounds tests/test_codec_gpu.py holds compress() to."""
    from image_compression_amd import codec
    from image_compression_amd.functional import AbsFn
    from image_compression_amd.modelling.blocks.entropy_model import symbolize_seg, symbols_as_tensor
    model = _model("LaplacianConditionalModel", "fp32_split")
    em, cm = model.entropy_model, model.conditional_model
    x = _batch(shape)
    N = shape[0]
    with _scaled(model, scaled):
        streams = model.compress_each(x, steps_per_chunk=R_MODEL)
        with torch.no_grad():
            y = model.analysis_transform(_pad(x))
            z = model.prior_analysis(AbsFn.apply(y))
            z_sym, kz = symbolize_seg(z)
            y_sym, ky = symbolize_seg(y)
            z_hat = symbols_as_tensor(z_sym.float(), tuple(z.shape))
            sigma = torch.cat([model.prior_synthesis(z_hat[n:n + 1]) for n in range(N)])
            rows = cm.scale_rows(sigma.expand_as(y)).cpu().numpy().astype(np.int64).reshape(N, -1)
            tz = {K: np.diff(em.tables(K).cpu().numpy().astype(np.int64), axis=1) for K in set(kz)}
            ty = {K: np.diff(cm.tables(K, x.device).cpu().numpy().astype(np.int64), axis=1) for K in set(ky)}
        if shape[2] % 64 == 0 and shape[3] % 64 == 0:
            whole = model.compress(x, steps_per_chunk=R_MODEL)
            print(f"rate each {shape} {'x32' if scaled else 'seed'}: {N} streams {sum(map(len, streams))} bytes, the "
                  f"batch container {len(whole)} bytes")
    zs = z_sym.cpu().numpy().astype(np.int64).reshape(N, -1)
    ys = y_sym.cpu().numpy().astype(np.int64).reshape(N, -1)
    for n, s in enumerate(streams):
        hd = codec.parse_image(s, 4, "fp32_split")[0]
        assert (hd.kmax_z, hd.kmax_y) == (kz[n], ky[n])
        ideal = float(np.sum(16.0 - np.log2(tz[kz[n]][np.arange(zs.shape[1]) % em.channels, zs[n] + kz[n]]))
                      + np.sum(16.0 - np.log2(ty[ky[n]][rows[n], ys[n] + ky[n]])))
        chunks = codec.num_chunks(hd.nsym_z, hd.R) + codec.num_chunks(hd.nsym_y, hd.R)
        coded = 8 * len(s) - 8 * codec.image_fixed_bytes(hd)
        print(f"rate each {shape} {'x32' if scaled else 'seed'} image {n}: kmax_z {kz[n]} kmax_y {ky[n]} bytes {len(s)} "
              f"ideal bits {ideal:.1f} coded - ideal {coded - ideal:+.1f} over {chunks} chunks")
        assert ideal - 16 * 64 * chunks - 1 <= coded <= ideal * 1.001 + 8 * chunks, (n, coded, ideal, chunks)
