"""The entropy coder on the GPU: the rANS kernels against the numpy reference coder of
tests/test_codec.py (same bytes, same symbols), the table, scale-index and symbolize kernels, and the
model's compress / decompress round trip with its rate against the estimated bpp."""
import functools

import numpy as np
import pytest
import torch

from test_codec import CASES, draw, ref_decode, ref_encode

pytestmark = pytest.mark.gpu

DEV = "cuda"
NROWS = 64
# the default chunk size with more than one chunk and a partial last step
GPU_CASES = CASES + [(2 * 65536 + 5, 1024)]


def _ops():
    from image_compression_amd import _lib
    return _lib.codec_ops()


def _check_tables(cdf):
    cdf = cdf.cpu().numpy().astype(np.int64)
    assert (cdf[:, 0] == 0).all(), "a row does not start at 0"
    assert (np.diff(cdf, axis=1) >= 1).all(), "a row is not strictly increasing"
    assert (cdf[:, -1] == 65536).all(), "a row does not end at 65536"
    return cdf


@functools.lru_cache(maxsize=None)
def _random_tables(K):
    """64 rows from the table kernel on random pmfs: peaked and flat rows, exact zeros, a one-hot row."""
    rng = np.random.default_rng(K)
    k = np.arange(-K, K + 1)
    pmf = np.stack([np.exp(-np.abs(k) / (0.05 + 30.0 * rng.random() ** 3)) * rng.random(2 * K + 1)
                    for _ in range(NROWS)])
    pmf[rng.random(pmf.shape) < 0.1] = 0.0
    pmf[:, K] += 1e-3                      # no all-zero row among the random ones
    pmf[0] = (k == 0)
    pmf = (pmf / pmf.sum(1, keepdims=True)).astype(np.float32)
    cdf = _check_tables(_ops().build_tables(torch.from_numpy(pmf).to(DEV)))
    # the counts follow the pmf: a symbol's share is its probability within the floor's reach (DESIGN.md:
    # c = 1 + floor(p (65536 - M)), the remainder to the largest count)
    M = 2 * K + 1
    c = np.diff(cdf, axis=1)
    base = 1 + np.floor(pmf.astype(np.float64) / pmf.astype(np.float64).sum(1, keepdims=True) * (65536 - M))
    # (the kernel sums the row in another order: a count may sit one off where p (65536 - M) is an integer)
    off = np.abs(c - base) > 1
    assert (off.sum(1) <= 1).all(), "more than one count repaired"
    assert (np.abs(c - base).max(1) <= M + 2).all()
    return cdf


@pytest.mark.parametrize("mode", ["rows", "channel"])
@pytest.mark.parametrize("K", [1, 37, 2047])
@pytest.mark.parametrize("n,R", GPU_CASES)
def test_coder_matches_the_reference_coder(n, R, K, mode):
    ops = _ops()
    cdf = _random_tables(K)
    rng = np.random.default_rng(n + K)
    C = 5
    rows = rng.integers(0, NROWS, n) if mode == "rows" else np.arange(n) % C
    idx = draw(rng, cdf, rows)
    if n > 2:
        idx[0], idx[-1] = 0, 2 * K            # the ends of the alphabet are coded too
    payload, lens = ref_encode(idx, rows, cdf, R)

    tab = torch.from_numpy(cdf.astype(np.int32)).to(DEV)
    sym = torch.from_numpy((idx - K).astype(np.int32)).to(DEV)
    rows_t = torch.from_numpy(rows.astype(np.uint8)).to(DEV) if mode == "rows" else None
    packed = ops.encode(sym, rows_t, C, tab, R)
    nchunks = len(lens)
    assert packed.numel() == 4 * nchunks + nchunks * (2 * 64 * R + 256)
    host = packed.cpu().numpy()
    got_lens = host[:4 * nchunks].view("<u4")
    assert np.array_equal(got_lens, lens), "chunk lengths differ from the reference encoder's"
    got = host[4 * nchunks:4 * nchunks + int(lens.sum())].tobytes()
    assert got == payload, "payload differs from the reference encoder's"

    out = ops.decode(packed[:4 * nchunks + len(payload)].clone(), n, rows_t, C, tab, R)
    assert out.dtype == torch.float32
    assert np.array_equal(out.cpu().numpy(), (idx - K).astype(np.float32)), "GPU decode"
    assert np.array_equal(ref_decode(got, got_lens, n, rows, cdf, R), idx), "reference decode of the GPU bytes"


def _cfg(kind="LaplacianConditionalModel", dtype="fp32_split", dims=None):
    from image_compression_amd import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.LOSS.REDUCTION = "mean"
    cfg.MODEL.ENTROPY_MODEL.CONDITIONAL_MODEL = kind
    cfg.MODEL.COMPUTE_DTYPE = dtype
    if dims is not None:
        cfg.MODEL.ENTROPY_MODEL.DIMS = list(dims)
    return cfg


@pytest.mark.parametrize("K", [1, 37, 2047])
@pytest.mark.parametrize("kind", ["LaplacianConditionalModel", "GaussianConditionalModel"])
def test_tables_of_the_conditional_models(kind, K):
    """All 64 scales; at K = 2047 the 0.11 row's pmf is all mass around 0 and the tail counts are the floor 1."""
    from image_compression_amd.modelling.blocks import ENTROPY_MODEL_REGISTRY
    cm = ENTROPY_MODEL_REGISTRY.get(kind)(_cfg(kind)).eval()
    cdf = _check_tables(cm.tables(K, torch.device(DEV)))
    assert cdf.shape == (64, 2 * K + 2)
    c = np.diff(cdf, axis=1)
    M = 2 * K + 1
    assert (c[:, K] + M >= c.max(1)).all()            # zero-mean unimodal models peak at 0 (up to the repair)
    if K == 2047:
        # the 0.11 row: beyond a few symbols from 0 the pmf underflows and every count is the floor
        assert c[0, K] > 60000 and (c[0, :K - 100] == 1).all() and (c[0, K + 101:] == 1).all()


@pytest.mark.parametrize("dims", [(3, 3, 3), (2, 4)])
def test_tables_of_the_factorized_model(dims):
    from image_compression_amd.modelling.blocks import ENTROPY_MODEL_REGISTRY
    torch.manual_seed(3)
    em = ENTROPY_MODEL_REGISTRY.get("EntropyModel")(6, _cfg(dims=dims)).to(DEV).eval()
    for K in (1, 37, 2047):
        cdf = _check_tables(em.tables(K))
        assert cdf.shape == (6, 2 * K + 2)


def test_scale_index_is_the_float32_comparison_rule():
    from image_compression_amd import codec
    scales, mids = codec.scale_table(64, 0.11, 256.0)
    below, above = np.nextafter(mids, np.float32(0)), np.nextafter(mids, np.float32(np.inf))
    sigma = np.concatenate([np.float32([1e-10, 1e10]), scales, mids, below, above]).astype(np.float32)
    want = (sigma[:, None] > mids[None, :]).sum(1)                   # the rule, in float32
    t = torch.from_numpy(sigma).to(DEV).view(1, 1, -1, 1)
    got = _ops().scale_index(t, [float(m) for m in mids]).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got[0] == 0 and got[1] == 63                               # the exp-clamp's ends clamp to the end rows
    assert np.array_equal(got[2:66], np.arange(64))                   # every table scale is its own row
    # identical sigma bits give identical rows, wherever they stand in the tensor
    again = _ops().scale_index(torch.from_numpy(sigma[::-1].copy()).to(DEV), [float(m) for m in mids]).cpu().numpy()
    assert np.array_equal(again[::-1], got)


def test_symbolize_is_torch_round_with_the_exact_kmax():
    from image_compression_amd.modelling.blocks.entropy_model import symbolize
    v = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -0.3, 0.3, 7.49, -2046.5, 2046.49, 0.0, -0.0, 100.5])
    x = v.repeat(40)[:512].view(2, 4, 8, 8).to(DEV)                    # (N, C, H, W): symbols come in (n, h, w, c) order
    sym, kmax = symbolize(x)
    assert sym.dtype == torch.int32
    assert torch.equal(sym.cpu(), torch.round(x.cpu()).movedim(1, -1).reshape(-1).to(torch.int32))
    assert kmax == 2046
    x[1, 2, 3, 4] = -2047.4
    assert symbolize(x)[1] == 2047
    for bad in (2047.5, -2048.0, 1e20, float("inf")):
        x[0, 0, 0, 0] = bad                                            # |q| = 2048 and beyond
        with pytest.raises(ValueError, match="2047"):
            symbolize(x)


# ------------------------------------------------------------------ the model
# Relative excess of the coded payload (everything the format does not fix) over the estimated rate of the
# same forward.  The two differ by the scale table (64 rows for a continuum of sigma) and the 16-bit frequency
# floor, which cost bits, and by the tables' support: a table covers only [-kmax, kmax] of its tensor and is
# renormalised there, which saves the mass the model spends beyond kmax.  Measured on the GPU over the cases of
# test_model_round_trip_and_rate (DESIGN.md section 11 lists all sixteen), the excess lies between -43.3 % and
# -15.9 %: with these untrained weights the support term dominates, and the largest measured excess is negative.
# The margin is defined as twice the largest measured excess rounded up to the next 0.5 %, as headroom above it;
# doubling a negative excess would turn the headroom into a bound the measured cases themselves miss, so the
# excess counts as 0 and the margin is 0: the coded payload may not exceed the estimate at all.
RATE_MARGIN = 0.0

SHAPES = [(2, 3, 128, 128), (1, 3, 64, 192)]


@functools.lru_cache(maxsize=None)
def _model(kind, dtype):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return modelling.build_model(_cfg(kind, dtype)).to(DEV).eval()


@pytest.mark.parametrize("scaled", [False, True], ids=["seed", "x32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["2x128x128", "1x64x192"])
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", ["LaplacianConditionalModel", "GaussianConditionalModel"])
def test_model_round_trip_and_rate(kind, dtype, shape, scaled):
    from image_compression_amd import codec
    model = _model(kind, dtype)
    last = [m for m in model.analysis_transform.modules() if hasattr(m, "weight") and m.weight.dim() == 4][-1]
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    if scaled:
        with torch.no_grad():
            last.weight.mul_(32.0)
    try:
        with torch.no_grad():
            y = model.analysis_transform(x)
            x_fwd, losses = model(x)
        data = model.compress(x)
        assert isinstance(data, bytes)
        assert model.compress(x) == data, "compressing twice gives different bytes"
        seen = []
        hook = model.synthesis_transform.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0]))
        try:
            x_hat = model.decompress(data)
        finally:
            hook.remove()
        h = codec.parse(data, 4, dtype)[0]
        if scaled:
            assert h.kmax_y > 16, h.kmax_y
        assert len(seen) == 1 and torch.equal(seen[0], torch.round(y)), "decoded y symbols"
        assert h.kmax_y == int(torch.round(y).abs().max())
        assert torch.equal(x_hat, x_fwd), "decompress(compress(x)) is not the eval forward's reconstruction"
        # rate: what is not fixed by the format against the estimated cross-entropy of the same forward
        N, _, H, W = shape
        estimated = float(losses["bpp"]) * N * H * W
        coded = 8 * len(data) - 8 * codec.fixed_bytes(h)
        excess = coded / estimated - 1.0
        print(f"rate {kind[:5]} {dtype} {shape} {'x32' if scaled else 'seed'}: kmax_z {h.kmax_z} kmax_y {h.kmax_y} "
              f"bytes {len(data)} fixed {codec.fixed_bytes(h)} estimated bits {estimated:.1f} coded bits {coded} "
              f"excess {100 * excess:+.3f} %")
        assert coded <= estimated * (1.0 + RATE_MARGIN), (coded, estimated, excess)
        # ... and against the ideal code length of the same symbols under the very tables the coder used, which
        # the support does not blur: a lane's state ends below 2^32, holding up to 16 message bits beyond the
        # 16 it started with (they are part of the fixed 32 * 64 bits per chunk), and a 32-bit rANS state loses
        # under 0.1 % to its integer divisions (the bound tests/test_codec.py holds the reference coder to)
        from image_compression_amd.functional import AbsFn
        from image_compression_amd.modelling.blocks.entropy_model import symbolize, symbols_as_tensor
        em, cm = model.entropy_model, model.conditional_model
        with torch.no_grad():
            z = model.prior_analysis(AbsFn.apply(y))
            z_sym, kz = symbolize(z)
            y_sym, ky = symbolize(y)
            sigma = model.prior_synthesis(symbols_as_tensor(z_sym.float(), tuple(z.shape)))
            rows = cm.scale_rows(sigma.expand_as(y)).cpu().numpy().astype(np.int64)
            tz = np.diff(em.tables(kz).cpu().numpy().astype(np.int64), axis=1)
            ty = np.diff(cm.tables(ky, x.device).cpu().numpy().astype(np.int64), axis=1)
        assert (kz, ky) == (h.kmax_z, h.kmax_y)
        zs, ys = z_sym.cpu().numpy().astype(np.int64), y_sym.cpu().numpy().astype(np.int64)
        ideal = float(np.sum(16.0 - np.log2(tz[np.arange(zs.size) % em.channels, zs + kz]))
                      + np.sum(16.0 - np.log2(ty[rows, ys + ky])))
        chunks = codec.num_chunks(zs.size, h.R) + codec.num_chunks(ys.size, h.R)
        print(f"     ideal bits under the tables {ideal:.1f}, coded - ideal {coded - ideal:+.1f} over {chunks} chunks")
        assert ideal - 16 * 64 * chunks - 1 <= coded <= ideal * 1.001 + 8 * chunks, (coded, ideal, chunks)
    finally:
        if scaled:
            with torch.no_grad():
                last.weight.div_(32.0)


def test_evaluator_reports_the_coded_rate():
    from image_compression_amd.evaluation import Evaluator
    model = _model("LaplacianConditionalModel", "fp32_split")
    g = torch.Generator().manual_seed(11)
    batches = [torch.rand(1, 3, 256, 256, generator=g).to(DEV), torch.rand(1, 3, 256, 256, generator=g).to(DEV)]
    plain = Evaluator(model).run_eval(batches)
    assert set(plain) == {"psnr", "ms_ssim", "y_entropy", "z_entropy", "bpp", "MSE"}
    coded = Evaluator(model, coded=True).run_eval(batches)
    assert set(coded) == set(plain) | {"coded_bpp"}
    for k in plain:
        assert coded[k] == plain[k], k
    want = np.mean([8.0 * len(model.compress(b)) / (256 * 256) for b in batches])
    assert coded["coded_bpp"] == pytest.approx(want, rel=1e-12)
    with pytest.raises(ValueError):
        Evaluator(model, graph=True, coded=True)
