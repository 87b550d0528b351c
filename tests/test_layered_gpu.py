"""Layered per-image streams on the GPU: the three ops against torch indexing (bitwise, both routes of every kernel),
the bytes of a gathered layer against the segmented coder on that layer alone, `compress_each_layered` /
`decompress_each_layered` of the scale, mean-scale and gained models against `compress_each` / `decompress_each` --
whole streams and every kind of prefix, latents bitwise and pixels by the bar of streams decoded in another call --
and `evaluation.progressive_sweep`."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_codec import draw, random_tables
from test_stream_gpu import _scaled

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 3
# (C, G): one channel per layer (direct kernels), whole 16-byte groups (tiles), C3's latent in layers of 5 (direct)
# and of 64 (tiles, rows too)
OP_CASES = [(192, 192), (192, 8), (320, 64), (320, 5)]
# positions: 15 = 5 x 3 (one short tile per image), 40 (two whole tiles and a short one)
POSITIONS = [15, 40]


def _ops():
    from image_compression_amd import _lib
    return _lib.layer_ops()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _orders(C, kind, seed=0):
    if kind == "identity":
        return np.tile(np.arange(C), (N, 1))
    rng = np.random.default_rng(seed + C)
    return np.stack([rng.permutation(C) for _ in range(N)])


# ------------------------------------------------------------------ 1. the ops against torch indexing
@pytest.mark.parametrize("kind", ["random", "identity"])
@pytest.mark.parametrize("P", POSITIONS)
@pytest.mark.parametrize("C,G", OP_CASES)
def test_gather_is_torch_indexing(C, G, P, kind):
    Cg = C // G
    order = _orders(C, kind)
    rng = np.random.default_rng(C + G + P)
    pairs = [(n, g) for n in range(N) for g in range(G)]
    seg = [pairs[i] for i in rng.permutation(len(pairs))[:max(2, (2 * len(pairs)) // 3)]]
    seg.append(seg[0])                                   # a pair may be asked for twice
    if G > 1:
        seg = [p for p in seg if p[0] != 1] or seg       # an image without segments
    ord_t = torch.from_numpy(order).to(DEV)
    for dtype, hi in ((torch.int32, 2 ** 31 - 1), (torch.uint8, 256)):
        src = torch.randint(-hi if dtype == torch.int32 else 0, hi, (N, P, C), dtype=dtype, device=DEV)
        got = _ops().gather(src, G, order.reshape(-1).tolist(), [v for p in seg for v in p])
        want = torch.cat([src[n][:, ord_t[n, g * Cg:(g + 1) * Cg]].reshape(-1) for n, g in seg])
        assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got, want), (C, G, P, kind, dtype)


def _scatter_reference(q, mu, order, nl, P, C, G):
    Cg = C // G
    y = torch.zeros(N, P, C, device=DEV) if mu is None else mu.clone()
    base = 0
    for n in range(N):
        k = nl[n]
        if k:
            chans = torch.from_numpy(order[n][:k * Cg]).to(DEV)
            qn = q[base:base + k * P * Cg].view(k, P, Cg).permute(1, 0, 2).reshape(P, k * Cg)
            y[n][:, chans] = qn if mu is None else qn + mu[n][:, chans]      # one fp32 addition
            base += k * P * Cg
    return y


@pytest.mark.parametrize("kind", ["random", "identity"])
@pytest.mark.parametrize("P", POSITIONS)
@pytest.mark.parametrize("C,G", OP_CASES)
def test_scatter_is_torch_indexing(C, G, P, kind):
    Cg = C // G
    order = _orders(C, kind, seed=1)
    g = torch.Generator().manual_seed(C + G + P)
    mu = torch.randn(N, P, C, generator=g).mul_(3.0)
    mu.view(-1)[::7] = -0.0
    mu = mu.to(DEV)
    for nl in ([0, G // 2, G], [G, 0, 1], [0, 0, 0]):
        q = torch.randint(-2047, 2048, (sum(nl) * P * Cg,), generator=g).float().to(DEV)
        for m in (mu, None):
            got = _ops().scatter(q, m, N, P, C, G, order.reshape(-1).tolist(), nl)
            want = _scatter_reference(q, m, order, nl, P, C, G)
            assert got.shape == (N, P, C) and got.dtype == torch.float32 and got.is_contiguous()
            assert torch.equal(_bits(got), _bits(want)), (C, G, P, kind, nl, m is not None)
            absent = torch.from_numpy(order[0][nl[0] * Cg:]).to(DEV)
            if len(absent):       # an absent channel: mu bit for bit, its -0.0 included, or +0.0
                held = _bits(got[0][:, absent])
                assert torch.equal(held, _bits(mu[0][:, absent])) if m is not None else not held.any()
    assert (_bits(mu) == -2 ** 31).any()


@pytest.mark.parametrize("P", POSITIONS + [300])
@pytest.mark.parametrize("C", [192, 320, 5])
def test_energy_is_the_exact_sum_of_squares(C, P):
    g = torch.Generator().manual_seed(C + P)
    sym = torch.randint(-60, 61, (N, P, C), generator=g, dtype=torch.int32)
    sym[0, :, 0], sym[1, ::2, C - 1], sym[2, P - 1, C // 2] = 2047, -2047, -2047
    sym[2, :, 1] = 0
    sym = sym.to(DEV)
    got = _ops().energy(sym)
    assert got.dtype == torch.int64 and got.shape == (N, C)
    assert torch.equal(got, sym.long().pow(2).sum(1))
    assert int(got[0, 0]) == P * 2047 * 2047 and int(got[2, 1]) == 0


# ------------------------------------------------------------------ 2. the bytes of a layer
HY, WY, CL, GL, K, NROWS = 8, 11, 192, 8, 37, 64


@functools.lru_cache(maxsize=None)
def _layer_source():
    """Two images of 8 x 11 x 192 symbols drawn from random tables of 64 rows at K = 37, a random row per symbol."""
    rng = np.random.default_rng(3)
    table = random_tables(np.random.default_rng(K + NROWS), NROWS, K)
    rows = rng.integers(0, NROWS, 2 * HY * WY * CL)
    sym = (draw(rng, table, rows) - K).astype(np.int32)
    order = np.stack([rng.permutation(CL) for _ in range(2)])
    return (torch.from_numpy(sym).to(DEV).view(2, HY * WY, CL), torch.from_numpy(rows.astype(np.uint8)).to(DEV).view(2, HY * WY, CL),
            torch.from_numpy(table.ravel().astype(np.int32)).to(DEV), order)


@pytest.mark.parametrize("R", [5, 1024])
def test_a_gathered_layer_codes_to_the_bytes_of_the_layer_alone(R):
    """R = 5: a layer's 2,112 symbols are six whole chunks and a short one; R = 1024: one chunk."""
    from image_compression_amd import _lib, codec
    sym, rows, pool, order = _layer_source()
    P, Cg = HY * WY, CL // GL
    seg_len = P * Cg
    assert codec.num_chunks(seg_len, R) == (7 if R == 5 else 1) and (R == 1024 or seg_len % (64 * R))
    pairs = [(n, g) for n in range(2) for g in range(GL)]
    flat = [v for p in pairs for v in p]
    gs = _ops().gather(sym, GL, order.reshape(-1).tolist(), flat)
    gr = _ops().gather(rows, GL, order.reshape(-1).tolist(), flat)
    enc = _lib.stream_ops().encode_seg
    packed = enc(gs, len(pairs), gr, 0, pool, NROWS, [K] * len(pairs), [0] * len(pairs), R)
    parts = codec.split_packed_seg(packed.cpu().numpy(), len(pairs), seg_len, R)
    ord_t = torch.from_numpy(order).to(DEV)
    for s, (n, g) in enumerate(pairs):
        chans = ord_t[n, g * Cg:(g + 1) * Cg]
        alone = enc(sym[n][:, chans].reshape(-1).contiguous(), 1, rows[n][:, chans].reshape(-1).contiguous(), 0, pool,
                    NROWS, [K], [0], R)
        lens, payload = codec.split_packed_seg(alone.cpu().numpy(), 1, seg_len, R)[0]
        assert np.array_equal(parts[s][0], lens) and parts[s][1] == payload, (R, n, g)


# ------------------------------------------------------------------ 3. the models
ARCHS = {"scale": "Compressor2018", "mean": "MeanScaleCompressor2018", "gained": "GainedMeanScaleCompressor2018"}
LAYERS, R_MODEL = 8, 5
QUALITIES = [1.0, 4.0]


@functools.lru_cache(maxsize=None)
def _model(name, kernel="conv"):
    from image_compression_amd import get_cfg_defaults, modelling
    cfg = get_cfg_defaults()
    cfg.MODEL.META_ARCHITECTURE = ARCHS.get(name, name)
    cfg.MODEL.LOSS.REDUCTION = "mean"
    cfg.MODEL.HYPER_SYNTHESIS.KERNEL = kernel
    torch.manual_seed(0)
    model = modelling.build_model(cfg).to(DEV).eval()
    if name == "gained":
        g = torch.Generator().manual_seed(42)
        with torch.no_grad():
            for p in model.gain.parameters():
                p.copy_((torch.rand(p.shape, generator=g) - 0.5).to(DEV))
        model.set_quality(QUALITIES)
    return model


def _images():
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, 3, 70, 100, generator=g)
    x[1] *= 0.25
    return x.to(DEV)


@contextlib.contextmanager
def _spy(model):
    """Records what `_latent_ungain` reads (the coded-domain latent) and what `_prior_each` returns."""
    seen = {"latent": [], "prior": []}
    ungain, prior = model._latent_ungain, model._prior_each

    def spy_ungain(y_hat):
        seen["latent"].append(y_hat.clone())
        return ungain(y_hat)

    def spy_prior(z_hat):
        out = prior(z_hat)
        seen["prior"].append(out)
        return out
    model._latent_ungain, model._prior_each = spy_ungain, spy_prior
    try:
        yield seen
    finally:
        del model._latent_ungain, model._prior_each


def _parser(model):
    return functools.partial(model._layered_containers[1], abi=4, compute_dtype="fp32_split",
                             version=model._image_format_version())


@pytest.mark.parametrize("name,kernel", [("scale", "conv"), ("mean", "conv"), ("gained", "conv"), ("mean", "invariant")])
def test_layered_streams_of_the_models(name, kernel):
    from image_compression_amd import codec
    model = _model(name, kernel)
    x = _images()
    C, Cg = 192, 192 // LAYERS
    with _scaled(model, True):
        plain = model.compress_each(x, steps_per_chunk=R_MODEL)
        with _spy(model) as seen:
            want = model.decompress_each(plain)
        (latent,), ((_, mean),) = seen["latent"], seen["prior"]
        assert latent.shape == (2, C, 8, 8) and (mean is None) == (name == "scale")

        # G = 1 in identity order: the layer is compress_each's y, byte for byte
        one = model.compress_each_layered(x, layers=1, order="identity", steps_per_chunk=R_MODEL)
        for n in range(2):
            h1, lz1, (ly1,), pz1, (py1,) = _parser(model)(one[n])
            h0, lz0, ly0, pz0, py0 = model._parse_image(plain[n], 4, "fp32_split")
            assert np.array_equal(ly1, ly0) and py1 == py0 and np.array_equal(lz1, lz0) and pz1 == pz0
            assert (h1.kmax_y, h1.kmax_z, h1.height, h1.width, h1.layers) == (h0.kmax_y, h0.kmax_z, 70, 100, 1)
            assert len(one[n]) == len(plain[n]) + 4 + 2 * C

        streams = model.compress_each_layered(x, layers=LAYERS, steps_per_chunk=R_MODEL)
        assert model.compress_each_layered(x, layers=LAYERS, steps_per_chunk=R_MODEL) == streams
        heads = [_parser(model)(s)[0] for s in streams]
        ends = [codec.layer_ends(s) for s in streams]
        print(f"layered {name} {kernel}: bytes {[len(s) for s in streams]} plain {[len(s) for s in plain]} "
              f"kmax_y {[h.kmax_y for h in heads]} ends {ends}")
        for n, h in enumerate(heads):
            assert h.layers == LAYERS and sorted(h.order.tolist()) == list(range(C)) and ends[n][-1] == len(streams[n])
            assert codec.num_chunks(h.nsym_y // LAYERS, R_MODEL) == 5          # 1,536 symbols: four whole chunks, a short one
            assert h.kmax_y > 0
            if name == "gained":
                assert h.quality == QUALITIES[n]
            # the default order: descending energy of the symbols the plain stream holds
            sym = (latent[n] - (0 if mean is None else mean[n])).round().long()
            assert h.order.tolist() == codec.layer_order(sym.pow(2).sum((1, 2)).cpu().numpy()).tolist()

        # whole streams: the latent of decompress_each, bitwise; the pixels by the bar of another call
        with _spy(model) as seen:
            full = model.decompress_each_layered(streams)
        assert torch.equal(_bits(seen["latent"][0]), _bits(latent))
        for n in range(2):
            assert full[n].shape == (1, 3, 70, 100)
            assert_close(full[n].cpu().numpy(), want[n].cpu().numpy(), 1e-4, f"image {n}")

        # prefixes at every ends[L], one byte behind it and one byte in front of the next: all in one call
        cuts = []
        for n in range(2):
            for L in range(LAYERS + 1):
                cuts.append((n, L, ends[n][L]))
                if L < LAYERS:
                    cuts += [(n, L, ends[n][L] + 1), (n, L, ends[n][L + 1] - 1)]
        with _spy(model) as seen:
            imgs = model.decompress_each_layered([streams[n][:e] for n, _, e in cuts])
        (got,) = seen["latent"]
        assert got.shape[0] == len(cuts) == len(imgs)

        def expected(n, L):
            out = latent[n].clone()
            absent = torch.from_numpy(heads[n].order[L * Cg:].astype(np.int64)).to(DEV)
            out[absent] = 0.0 if mean is None else mean[n][absent]
            return out
        for k, (n, L, e) in enumerate(cuts):
            assert torch.equal(_bits(got[k]), _bits(expected(n, L))), (n, L, e)
            assert imgs[k].shape == (1, 3, 70, 100) and bool(torch.isfinite(imgs[k]).all())

        # streams with different L in one call give what each gives alone; `layers=` caps like a cut
        for k in (0, 4, 13, len(cuts) - 1):
            n, L, e = cuts[k]
            with _spy(model) as seen:
                alone = model.decompress_each_layered([streams[n][:e]])[0]
            assert torch.equal(_bits(seen["latent"][0][0]), _bits(got[k]))
            assert_close(alone.cpu().numpy(), imgs[k].cpu().numpy(), 1e-4, f"cut {k} alone")
        with _spy(model) as seen:
            model.decompress_each_layered(streams, layers=[3, 0])
        assert torch.equal(_bits(seen["latent"][0][0]), _bits(expected(0, 3)))
        assert torch.equal(_bits(seen["latent"][0][1]), _bits(expected(1, 0)))

        # an explicit order is honoured and stored
        order = np.stack([np.arange(C)[::-1], np.roll(np.arange(C), 5)])
        explicit = model.compress_each_layered(x, layers=LAYERS, order=order, steps_per_chunk=R_MODEL)
        assert [_parser(model)(s)[0].order.tolist() for s in explicit] == order.tolist()
        with _spy(model) as seen:
            model.decompress_each_layered([s[:codec.layer_ends(s)[2]] for s in explicit])
        for n in range(2):
            out = latent[n].clone()
            absent = torch.from_numpy(order[n][2 * Cg:].copy()).to(DEV)
            out[absent] = 0.0 if mean is None else mean[n][absent]
            assert torch.equal(_bits(seen["latent"][0][n]), _bits(out))


def test_the_route_versions_refuse_each_other():
    conv, inv = _model("mean", "conv"), _model("mean", "invariant")
    x = _images()[:1]
    a = conv.compress_each_layered(x, layers=LAYERS, steps_per_chunk=R_MODEL)
    b = inv.compress_each_layered(x, layers=LAYERS, steps_per_chunk=R_MODEL)
    assert a[0][4:6] == b"\x01\x00" and b[0][4:6] == b"\x02\x00"
    for model, data in ((conv, b), (inv, a)):
        with pytest.raises(ValueError, match="format version"):
            model.decompress_each_layered(data)


@pytest.mark.parametrize("arch", ["CheckerboardCompressor2018", "RegionGainedMeanScaleCompressor2018"])
def test_uncovered_models_refuse(arch):
    model = _model(arch)
    for call in (lambda: model.compress_each_layered(_images()), lambda: model.decompress_each_layered([b"ICRL"])):
        with pytest.raises(ValueError) as e:
            call()
        assert model.layered_refusal in str(e.value)


# ------------------------------------------------------------------ 4. the sweep
def test_progressive_sweep():
    from image_compression_amd import evaluation
    model = _model("mean")
    x = _images()
    with _scaled(model, True):
        rows = evaluation.progressive_sweep(model, [x], layers=LAYERS, steps_per_chunk=R_MODEL)
        whole = torch.cat(model.decompress_each(model.compress_each(x, steps_per_chunk=R_MODEL)))
        want = float(evaluation.psnr(whole, x).double().mean())
    print("progressive sweep:", [(r["layers"], round(r["bpp"], 4), round(r["psnr"], 3)) for r in rows])
    assert [r["layers"] for r in rows] == list(range(LAYERS + 1))
    assert all(a["bpp"] < b["bpp"] for a, b in zip(rows, rows[1:]))
    assert rows[-1]["psnr"] == pytest.approx(want, rel=1e-6)
