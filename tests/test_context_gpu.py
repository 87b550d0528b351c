"""The fused checkerboard context on the GPU: the kernel (torch.ops.imgcomp_ctx.context_fwd) against an fp64 numpy
restatement of its formulas, its exact properties (anchors copied, dead taps and non-anchor inputs never read, a zero
context), its batch invariance bit for bit, its agreement with the conv route and its weight cache; then
CheckerboardCompressor2018 under MODEL.CONTEXT.KERNEL "fused": the batch streams ("ICRC" version 2) and the per-image
streams ("ICRK") against the eval forward and against a reference composed from the model's own pieces, the zero
context against MeanScaleCompressor2018, and the rate of every stream."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_checkerboard_gpu import _anchors, _ckbd_model, _set_context
from test_mean_scale_gpu import DEV, KINDS, _cfg, _changed, _ideal_bits, _model

pytestmark = pytest.mark.gpu

ARCH = "CheckerboardCompressor2018"
LIMIT = 4.0
# a single position (no non-anchor), a row of two, one full 2 x 2, odd sizes both ways, 4 x 4, and 8 x 12 (two tiles of
# 32 non-anchors, the second half full); C = 5 (scalar loads, one padded channel group), 8 (one whole group), 192
MAPS = [(1, 1), (1, 2), (2, 2), (3, 5), (4, 4), (8, 12)]
CASES = [(H, W, C) for (H, W) in MAPS for C in (5, 8, 192)] + [(32, 48, 192)]     # the last: 24 tiles per image
IDS = [f"{H}x{W}x{C}" for H, W, C in CASES]
LIVE = [(ky, kx) for ky in range(5) for kx in range(5) if (ky + kx) % 2 == 1]    # (ky-2) + (kx-2) odd


def _op():
    from image_compression_amd import _lib
    return _lib.ctx_ops().context_fwd


def _batch(H, W, C):
    return 2 if (H, W) == (32, 48) else 3


@functools.lru_cache(maxsize=None)
def _inputs(H, W, C):
    """fp32 numpy (y, mu_h, sigma_h, w_mean, b_mean, w_scale, b_scale): every one of the 25 taps nonzero, nonzero
    biases, the log-scale b of std about 2.5 where the window is whole, and two scale biases at +-6 so that the clamp
    is hit on both sides at every shape that has a non-anchor."""
    N = _batch(H, W, C)
    rng = np.random.default_rng(1000 * H + 10 * W + C)
    full = (N, H, W, C)
    y = (rng.standard_normal(full) * 3).astype(np.float32)
    mu_h = rng.standard_normal(full).astype(np.float32)
    sigma_h = np.exp(rng.standard_normal(full)).astype(np.float32)
    s = 1.0 / np.sqrt(12.0 * C)
    wm = (rng.standard_normal((C, C, 5, 5)) * s).astype(np.float32)
    ws = (rng.standard_normal((C, C, 5, 5)) * s * 0.8).astype(np.float32)
    bm = rng.standard_normal(C).astype(np.float32)
    bs = (rng.standard_normal(C) * 0.5).astype(np.float32)
    bs[0], bs[1] = 6.0, -6.0
    assert (wm != 0).all() and (ws != 0).all() and (bm != 0).all() and (bs != 0).all()
    return y, mu_h, sigma_h, wm, bm, ws, bs


@functools.lru_cache(maxsize=None)
def _reference(H, W, C):
    """(mu, sigma, b) in fp64 from the fp32 inputs: the formulas of the kernel's header, restated."""
    y, mu_h, sigma_h, wm, bm, ws, bs = _inputs(H, W, C)
    N = y.shape[0]
    d = np.abs(y - mu_h)                                    # one fp32 subtraction
    assert d.dtype == np.float32
    yp, vp = (np.zeros((N, H + 4, W + 4, C)) for _ in range(2))       # a neighbour outside the map contributes 0
    yp[:, 2:-2, 2:-2], vp[:, 2:-2, 2:-2] = y, d
    a = np.broadcast_to(bm.astype(np.float64), (N, H, W, C)).copy()
    b = np.broadcast_to(bs.astype(np.float64), (N, H, W, C)).copy()
    for ky, kx in LIVE:
        a += np.einsum("nijc,oc->nijo", yp[:, ky:ky + H, kx:kx + W], wm[:, :, ky, kx].astype(np.float64))
        b += np.einsum("nijc,oc->nijo", vp[:, ky:ky + H, kx:kx + W], ws[:, :, ky, kx].astype(np.float64))
    A = _anchors(H, W)[None, :, :, None]
    mu = np.where(A, mu_h, mu_h.astype(np.float64) + a)
    sigma = np.where(A, sigma_h, sigma_h.astype(np.float64) * np.exp(np.clip(b, -LIMIT, LIMIT)))
    return mu, sigma, b


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@functools.lru_cache(maxsize=None)
def _run(H, W, C):
    """The kernel's (mu, sigma) on the device for `_inputs`, computed once and left unchanged."""
    return _op()(*_dev(*_inputs(H, W, C)))


def _same(a, b):
    """Bit for bit, NaN payloads and zero signs included."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_is_the_fp64_restatement_of_its_formulas(case):
    H, W, C = case
    y, mu_h, sigma_h, *_ = _inputs(*case)
    mu, sigma = _run(*case)
    want_mu, want_sigma, b = _reference(*case)
    A = np.broadcast_to(_anchors(H, W)[None, :, :, None], y.shape)
    assert tuple(mu.shape) == tuple(sigma.shape) == y.shape and mu.is_contiguous() and sigma.is_contiguous()
    if (~A).any():
        nb = b[~A]
        assert (nb > LIMIT).any() and (nb < -LIMIT).any(), "the clamp is not hit on both sides"
        assert C < 8 or H * W < 4 or (np.abs(nb) < LIMIT).any(), "every b is clamped"
    got_mu, got_sigma = mu.cpu().numpy(), sigma.cpu().numpy()
    for name, got, want in (("mu", got_mu, want_mu), ("sigma", got_sigma, want_sigma)):
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"context_fwd {case} {name}: max |d| / max |ref| = {err:.2e}")
        assert_close(got, want, 1e-4, name)
    # the anchors: the hyperprior's own parameters, bit for bit
    dm, ds = _dev(mu_h, sigma_h)
    At = torch.from_numpy(A.copy()).to(DEV)
    assert _same(mu[At], dm[At]) and _same(sigma[At], ds[At])


@pytest.mark.parametrize("case", CASES[:-1], ids=IDS[:-1])
def test_kernel_never_reads_the_dead_taps_or_the_non_anchors_of_y(case):
    H, W, C = case
    y, mu_h, sigma_h, wm, bm, ws, bs = _inputs(*case)
    mu, sigma = _run(*case)
    dead = np.ones((5, 5), dtype=bool)
    for ky, kx in LIVE:
        dead[ky, kx] = False
    assert dead.sum() == 13 and dead[2, 2]
    rng = np.random.default_rng(5)
    for fill in ("other", "nan"):
        wm2, ws2 = wm.copy(), ws.copy()
        for w in (wm2, ws2):
            w[:, :, dead] = np.nan if fill == "nan" else rng.standard_normal((C, C, 13)).astype(np.float32) * 50
        mu2, sigma2 = _op()(*_dev(y, mu_h, sigma_h, wm2, bm, ws2, bs))
        assert _same(mu2, mu) and _same(sigma2, sigma), f"the 13 same-parity taps ({fill}) changed an output"
    y2 = np.where(_anchors(H, W)[None, :, :, None], y, np.float32(np.nan))
    assert H * W == 1 or np.isnan(y2).any()
    mu3, sigma3 = _op()(*_dev(y2, mu_h, sigma_h, wm, bm, ws, bs))
    assert _same(mu3, mu) and _same(sigma3, sigma), "the non-anchors of y_in changed an output"
    assert not torch.isnan(mu3).any() and not torch.isnan(sigma3).any()


@pytest.mark.parametrize("case", CASES[:-1], ids=IDS[:-1])
def test_zero_context_returns_the_hyperprior_parameters(case):
    y, mu_h, sigma_h, wm, bm, ws, bs = _inputs(*case)
    dy, dm, ds = _dev(y, mu_h, sigma_h)
    zw, zb = torch.zeros(wm.shape, device=DEV), torch.zeros(bm.shape, device=DEV)
    mu, sigma = _op()(dy, dm, ds, zw, zb, zw.clone(), zb.clone())
    assert _same(sigma, ds), "sigma_h * expf(0) is not sigma_h"
    assert _same(mu, dm + 0.0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_image_n_has_the_same_bits_in_any_batch_and_at_any_index(case):
    H, W, C = case
    arrays = _inputs(*case)
    N = arrays[0].shape[0]
    mu, sigma = _run(*case)
    weights = _dev(*arrays[3:])
    acts = _dev(*arrays[:3])
    for n in range(N):                                  # alone: N = 1
        m1, s1 = _op()(*(t[n:n + 1].contiguous() for t in acts), *weights)
        assert _same(m1[0], mu[n]) and _same(s1[0], sigma[n]), f"image {n} alone differs from image {n} of {N}"
    # at another index, among other neighbours: the batch rotated by one, image 0 repeated behind it
    order = [*range(1, N), 0, 0]
    m2, s2 = _op()(*(t[order].contiguous() for t in acts), *weights)
    for k, n in enumerate(order):
        assert _same(m2[k], mu[n]) and _same(s2[k], sigma[n]), f"image {n} at index {k} of {len(order)}"


def test_more_images_than_grid_rows_keep_the_bits():
    """Past 65535 images the grid's rows loop over the batch: the last image of 65537 against itself alone."""
    y, mu_h, sigma_h, *w = _inputs(1, 2, 5)
    N = 65537
    rng = np.random.default_rng(9)
    acts = _dev(*(np.concatenate([rng.standard_normal((N - 1, 1, 2, 5)).astype(np.float32) + 2.0, t[:1]]) for t in
                  (y, mu_h, np.log(sigma_h))))
    acts[2] = acts[2].exp()
    weights = _dev(*w)
    mu, sigma = _op()(*acts, *weights)
    for n in (0, 65534, 65535, 65536):
        m1, s1 = _op()(*(t[n:n + 1].contiguous() for t in acts), *weights)
        assert _same(m1[0], mu[n]) and _same(s1[0], sigma[n]), n
    assert _same(mu[N - 1], _run(1, 2, 5)[0][0])        # and image 0 of the three-image call: the same y_in and mu_h


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
def test_kernel_agrees_with_the_conv_route(dtype):
    from image_compression_amd import functional as F
    from image_compression_amd.modelling.blocks.entropy_model import ckbd_input, ckbd_params
    model = _ckbd_model(KINDS[0], dtype)
    N, C, H, W = 2, 192, 8, 12
    g = torch.Generator().manual_seed(4)
    y_in = (torch.randn(N, C, H, W, generator=g) * 3).to(DEV)
    mu_h = torch.randn(N, C, H, W, generator=g).to(DEV)
    sigma_h = torch.randn(N, C, H, W, generator=g).exp().to(DEV)
    cm, cs = model.context_mean, model.context_scale
    with torch.no_grad():
        u, v = ckbd_input(y_in, mu_h)
        want_mu, want_sigma = ckbd_params(mu_h, sigma_h, cm(u), cs(v))
        mu, sigma = F.ckbd_context(y_in, mu_h, sigma_h, cm.weight, cm.bias, cs.weight, cs.bias)
    assert tuple(mu.shape) == (N, C, H, W) and mu.is_contiguous(memory_format=torch.channels_last)
    for name, got, want in (("mu", mu, want_mu), ("sigma", sigma, want_sigma)):
        print(f"fused against convs [{dtype}] {name}: max |d| = {float((got - want).abs().max()):.3e}")
        assert not torch.equal(got, mu_h if name == "mu" else sigma_h)
        assert_close(got.cpu().numpy(), want.cpu().numpy(), 1e-4, name)


def test_weight_cache_keeps_the_packed_taps_until_a_weight_changes():
    from image_compression_amd import functional as F
    y, mu_h, sigma_h, *w = _inputs(8, 12, 8)
    to_logical = lambda t: t.movedim(-1, 1)          # noqa: E731  (N, H, W, C) storage -> logical (N, C, H, W)
    acts = [to_logical(t) for t in _dev(y, mu_h, sigma_h)]
    wm, bm, ws, bs = _dev(*w)
    want = [to_logical(t) for t in _run(8, 12, 8)]
    tiny = [t[:1, :, :1, :1] for t in acts]          # a 1 x 1 map packs nothing: it must not mark the entry packed
    with torch.no_grad(), F.weight_cache():
        F.ckbd_context(*tiny, wm, bm, ws, bs)
        for _ in range(3):                           # packs once, then reads the kept pack
            mu, sigma = F.ckbd_context(*acts, wm, bm, ws, bs)
            assert _same(mu.contiguous(), want[0].contiguous()) and _same(sigma.contiguous(), want[1].contiguous())
        for changed in (wm, ws):                     # an in-place update of either weight is seen
            changed.mul_(1.5)
            mu, sigma = F.ckbd_context(*acts, wm, bm, ws, bs)
            fresh = _op()(*(t.movedim(1, -1).contiguous() for t in acts), wm, bm, ws, bs)
            assert _same(mu.movedim(1, -1).contiguous(), fresh[0]) and _same(sigma.movedim(1, -1).contiguous(), fresh[1])
            assert not _same(mu.contiguous(), want[0].contiguous()) or changed is ws
            assert not _same(sigma.contiguous(), want[1].contiguous()) or changed is wm
            want = [mu, sigma]


# ------------------------------------------------------------------ the model
R_MODEL = 16
DTYPES = ["fp32_split", "fp32"]


def _fused_cfg(kind, dtype, arch=ARCH):
    cfg = _cfg(kind, dtype, arch)
    cfg.MODEL.CONTEXT.KERNEL = "fused"
    return cfg


@functools.lru_cache(maxsize=None)
def _fused_model(kind, dtype):
    """The weights of test_checkerboard_gpu's `_ckbd_model` (seed 0, seeded nonzero context), with the fused context."""
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return _set_context(modelling.build_model(_fused_cfg(kind, dtype))).to(DEV).eval()


def _pad(x):
    from image_compression_amd import _lib, codec
    H, W = codec.padded_size(*x.shape[2:])
    return x if (H, W) == tuple(x.shape[2:]) else _lib.stream_ops().pad_edge(x.contiguous(), H, W)


def _pieces(model, x):
    """What the issue's reference is composed of, on the padded batch: g_a / h_a, h_s image by image, the context of
    the anchors as decoded, the quantised latent, the reconstruction -- and the integers and rows that were coded."""
    from image_compression_amd.modelling.blocks.entropy_model import center_round, symbolize, symbols_as_tensor
    cm = model.conditional_model
    with torch.no_grad():
        y = model.analysis_transform(_pad(x))
        z = model.prior_analysis(y)
        z_hat = symbols_as_tensor(symbolize(z)[0].float(), tuple(z.shape))
        sigma_h, mu_h = model._prior_each(z_hat)
        _, y_anchor = center_round(y, mu_h)
        sigma, mu = model._context(y_anchor, sigma_h, mu_h)
        res, y_hat = center_round(y, mu)
        x_hat = model._reconstruct(y_hat)[:, :, :x.shape[2], :x.shape[3]]
        rows = cm.scale_rows(sigma).view(x.shape[0], -1)
    return dict(y=y, z_hat=z_hat, sigma_h=sigma_h, mu_h=mu_h, sigma=sigma, mu=mu, res=res, y_hat=y_hat, x_hat=x_hat, rows=rows)


def _flat_int(t, n):
    """Image n of a logical (N, C, *) tensor of float integers, in the coder's (*, c) order, as int64 numpy."""
    return t[n].movedim(0, -1).reshape(-1).cpu().numpy().astype(np.int64)


def _check_rate(model, data, h, lens, fixed, z_sym, res, rows, what):
    """The coded bits of one stream within the existing bound per chunk, under the stream's own tables."""
    ideal = _ideal_bits(model, z_sym, h.kmax_z, res, h.kmax_y, rows)
    chunks = sum(len(l) for l in lens)
    coded = 8 * len(data) - 8 * fixed
    print(f"{what}: kmax_z {h.kmax_z} kmax_y {h.kmax_y} bytes {len(data)} ideal bits {ideal:.1f} coded - ideal "
          f"{coded - ideal:+.1f} over {chunks} chunks")
    assert ideal - 16 * 64 * chunks <= coded <= ideal * 1.001 + 8 * chunks, (what, coded, ideal, chunks)


class _spy_reconstruct:
    """Records the y_hat `_reconstruct` is handed, in call order."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __enter__(self):
        orig = self.model._reconstruct

        def spy(y_hat, *args):
            self.seen.append(y_hat.clone())
            return orig(y_hat, *args)
        self.model._reconstruct = spy
        return self.seen

    def __exit__(self, *exc):
        del self.model._reconstruct


@pytest.mark.parametrize("shape", [(2, 3, 128, 128), (1, 3, 64, 192)], ids=["2x128x128", "1x64x192"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_batch_round_trip_is_the_eval_forward_bitwise_in_icrc_version_2(kind, dtype, shape):
    from image_compression_amd import codec
    model, conv = _fused_model(kind, dtype), _ckbd_model(kind, dtype)
    assert (model.context_kernel, conv.context_kernel) == ("fused", "conv")
    for p, q in zip(model.parameters(), conv.parameters()):
        assert torch.equal(p, q)
    assert all(torch.count_nonzero(p) for c in (model.context_mean, model.context_scale) for p in c.parameters())
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    with _changed(model, True), _changed(conv, True):
        x_fwd, _ = model(x)
        data = model.compress(x, steps_per_chunk=R_MODEL)
        assert data[:4] == b"ICRC" and int.from_bytes(data[4:6], "little") == 2
        assert model.compress(x, steps_per_chunk=R_MODEL) == data, "compressing twice gives different bytes"
        x_hat = model.decompress(data)
        old = conv.compress(x, steps_per_chunk=R_MODEL)
        assert old[:4] == b"ICRC" and int.from_bytes(old[4:6], "little") == 1
        with pytest.raises(ValueError, match="format version 2"):
            conv.decompress(data)
        with pytest.raises(ValueError, match="format version 1"):
            model.decompress(old)
        assert torch.equal(conv.decompress(old), conv(x)[0])
        h, lz, la, ln, *_ = codec.parse_checkerboard(data, 4, dtype, version=2)
        # the rate: the batch's symbols under the batch's own (sigma, mu) -- h_s on the whole batch here
        with torch.no_grad():
            y = model.analysis_transform(x)
            z_hat = torch.round(model.prior_analysis(y))
            sigma_h, mu_h = model._prior(z_hat)
            sigma, mu = model._eval_params(y, sigma_h, mu_h)
            rows = model.conditional_model.scale_rows(sigma).cpu().numpy().astype(np.int64)
        res = torch.round(y - mu)
        flat = lambda t: t.movedim(1, -1).reshape(-1).cpu().numpy().astype(np.int64)     # noqa: E731
        assert h.kmax_y == int(res.abs().max()) > 16 and h.R == R_MODEL and len(la) == len(ln) >= 2
        _check_rate(model, data, h, (lz, la, ln), codec.checkerboard_fixed_bytes(h), flat(z_hat), flat(res), rows,
                    f"ICRC v2 {kind[:5]} {dtype} {shape}")
    assert torch.equal(x_hat, x_fwd), "decompress(compress(x)) is not the eval forward's reconstruction"


@pytest.mark.parametrize("size", [(64, 128), (40, 130)], ids=["64x128", "40x130"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_image_round_trip_is_the_eval_forward_of_the_padded_image(kind, dtype, size):
    model = _fused_model(kind, dtype)
    x = torch.rand(1, 3, *size, generator=torch.Generator().manual_seed(8)).to(DEV)
    with _changed(model, True):
        streams = model.compress_each(x, steps_per_chunk=R_MODEL)
        assert len(streams) == 1 and streams[0][:4] == b"ICRK"
        out = model.decompress_each(streams)
        want = model(_pad(x))[0][:, :, :size[0], :size[1]]
    assert len(out) == 1 and tuple(out[0].shape) == (1, 3, *size)
    assert torch.equal(out[0], want), "decompress_each(compress_each(x)) is not the padded image's eval forward, cropped"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_three_images_decode_alone_together_reversed_and_mixed(kind, dtype):
    from image_compression_amd import codec
    model = _fused_model(kind, dtype)
    g = torch.Generator().manual_seed(9)
    noise = torch.rand(3, 3, 72, 100, generator=g)
    x = torch.stack([noise[0], torch.full((3, 72, 100), 0.5), noise[2] * 0.25]).to(DEV)
    other = torch.rand(1, 3, 40, 130, generator=g).to(DEV)
    with _changed(model, True):
        streams = model.compress_each(x, steps_per_chunk=R_MODEL)
        assert model.compress_each(x, steps_per_chunk=R_MODEL) == streams, "compressing twice gives different bytes"
        extra = model.compress_each(other, steps_per_chunk=R_MODEL)
        ref = _pieces(model, x)
        with _spy_reconstruct(model) as seen:
            together = model.decompress_each(streams)
            alone = [model.decompress_each([s])[0] for s in streams]
            backwards = model.decompress_each(streams[::-1])[::-1]
            mixed = model.decompress_each([streams[1], extra[0], streams[2], streams[0]])
        parsed = [codec.parse_checkerboard_image(s, 4, dtype) for s in streams]
        # the rate of every stream under its own tables
        for n, (h, lz, la, ln, *_) in enumerate(parsed):
            assert (h.N, h.H, h.W, h.height, h.width, h.R) == (1, 128, 128, 72, 100, R_MODEL)
            assert len(la) == len(ln) == codec.num_chunks(h.nsym_y // 2, h.R) >= 3
            res = _flat_int(ref["res"], n)
            assert h.kmax_y == int(np.abs(res).max()) and h.kmax_z == int(ref["z_hat"][n].abs().max())
            _check_rate(model, streams[n], h, (lz, la, ln), codec.checkerboard_image_fixed_bytes(h),
                        _flat_int(ref["z_hat"], n), res, ref["rows"][n].cpu().numpy().astype(np.int64),
                        f"ICRK {kind[:5]} {dtype} image {n}")
    assert len({p[0].kmax_y for p in parsed}) > 1, "the three images take one K: the test does not separate them"
    # together: the reference composed from the model's own pieces, bit for bit
    assert len(together) == 3
    for n in range(3):
        assert tuple(together[n].shape) == (1, 3, 72, 100)
        assert torch.equal(together[n][0], ref["x_hat"][n]), f"image {n} decoded together is not the composed reference"
    # the latent of image n: the same bits however its stream is grouped
    y_together, y_alone, y_back, y_mixed = seen[0], seen[1:4], seen[4], seen[5:]
    assert len(seen) == 7 and tuple(y_together.shape) == (3, 192, 8, 8)
    assert torch.equal(y_together, ref["y_hat"])
    shapes = sorted(tuple(t.shape) for t in y_mixed)
    assert shapes == [(1, 192, 4, 12), (3, 192, 8, 8)]
    y_mix = next(t for t in y_mixed if t.shape[0] == 3)                     # in the order streams 1, 2, 0
    for n in range(3):
        assert torch.equal(y_alone[n][0], y_together[n]), f"image {n} alone"
        assert torch.equal(y_back[2 - n], y_together[n]), f"image {n} reversed"
        assert torch.equal(y_mix[[2, 0, 1][n]], y_together[n]), f"image {n} mixed"
    # the images: g_s's low bits follow the grouping
    for name, imgs in (("alone", alone), ("reversed", backwards), ("mixed", [mixed[3], mixed[0], mixed[2]])):
        for n in range(3):
            assert_close(imgs[n].cpu().numpy(), together[n].cpu().numpy(), 1e-4, f"image {n} {name}")
    assert tuple(mixed[1].shape) == (1, 3, 40, 130)
    assert_close(mixed[1].cpu().numpy(), model.decompress_each(extra)[0].cpu().numpy(), 1e-4, "the other image")


@pytest.mark.parametrize("kind", KINDS)
def test_fresh_fused_model_is_the_mean_scale_model(kind):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    fresh = modelling.build_model(_fused_cfg(kind, "fp32_split")).to(DEV).eval()
    base = _model(kind, "fp32_split")
    assert all(torch.count_nonzero(p) == 0 for c in (fresh.context_mean, fresh.context_scale) for p in c.parameters())
    g = torch.Generator().manual_seed(10)
    x = torch.rand(2, 3, 72, 100, generator=g).to(DEV)
    xb = torch.rand(2, 3, 128, 128, generator=g).to(DEV)
    with _changed(fresh, True), _changed(base, True):
        a = fresh.decompress_each(fresh.compress_each(x, steps_per_chunk=R_MODEL))
        b = base.decompress_each(base.compress_each(x, steps_per_chunk=R_MODEL))
        (xa, la), (xm, lm) = fresh(xb), base(xb)
    for n in range(2):
        assert torch.equal(a[n], b[n]), f"image {n}: the zero context is not the mean-scale model"
    assert torch.equal(xa, xm) and set(la) == set(lm)
    for k in lm:
        assert torch.equal(la[k], lm[k]), k
