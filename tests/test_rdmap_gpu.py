"""Rate and distortion maps on the GPU: ic_block_bits and ic_block_sse against numpy in fp64 on the same fp32 inputs
(partial blocks, one block, one position, C of 4 / 5 / 192 / 320, both storage layouts, a misaligned pointer, N > 1) and
their bitwise guarantees (run to run, alignment, batch invariance, the `add` operand); then
`Compressor2018.rate_distortion_map` of every architecture against its own eval forward, the region model against the
gained model, and `Evaluator.run_eval_each`."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_checkerboard_gpu import _set_context
from test_gained import cfg_of
from test_gained_gpu import S, _bits, _dev, _tables
from test_mean_scale_gpu import _batch, _last_analysis_conv

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYOUTS = ("last", "nchw")


def _ops():
    from image_compression_amd import _lib
    return _lib.map_ops()


def _store(a, layout, offset):
    """The logical (N, C, H, W) array on the device in channels-last or NCHW storage, aligned or one element past."""
    if layout == "last":
        return _dev(np.ascontiguousarray(a.transpose(0, 2, 3, 1)), offset).permute(0, 3, 1, 2)
    return _dev(a, offset)


def _block_sums(t, shift):
    """(N, C, H, W) float64 -> (N, ceil(H / 2^shift), ceil(W / 2^shift)): the sum over the channels and every block."""
    s = t.sum(axis=1)
    i, j = np.arange(0, s.shape[1], 1 << shift), np.arange(0, s.shape[2], 1 << shift)
    return np.add.reduceat(np.add.reduceat(s, i, axis=1), j, axis=2)


def _terms(p):
    """clamp(-log2(p + 1e-10), 0, 50) in fp64 on the fp32 values."""
    return np.clip(-np.log2(p.astype(np.float64) + 1e-10), 0.0, 50.0)


SPECIAL = (0.0, 1.0, 1e-30, 1.5)    # 1e-10's bits, 0 bits, 1e-10's bits again, a negative term clamped to 0 bits


def _likelihoods(rng, shape):
    """Log-uniform in [1e-12, 1], with a few entries at the special values."""
    p = np.exp(rng.uniform(np.log(1e-12), 0.0, shape)).astype(np.float32)
    flat = p.reshape(-1)
    at = rng.choice(flat.size, size=min(flat.size // 2, 8), replace=False)
    flat[at] = np.asarray(SPECIAL, np.float32)[np.arange(at.size) % 4]
    return p


def test_the_terms_of_the_special_values():
    p = np.asarray(SPECIAL, np.float32).reshape(1, 1, 1, 4)      # one channel, four positions: at shift 0 the map is the terms
    got = _ops().block_bits(_dev(p, 0), 0)
    assert got.shape == (1, 1, 4)
    assert_close(got.cpu().numpy(), _terms(p)[:, 0], 1e-4, "the special values")
    assert got[0, 0, 1] == 0.0 and got[0, 0, 3] == 0.0 and abs(float(got[0, 0, 0]) - 33.2193) < 1e-3


@pytest.mark.parametrize("C", [192, 320, 5, 4])
@pytest.mark.parametrize("Hm,Wm,shift", [(1, 1, 2), (4, 4, 2), (5, 7, 2), (8, 12, 2), (3, 2, 0), (1, 1, 0), (9, 5, 3)])
def test_block_bits(Hm, Wm, shift, C):
    ops = _ops()
    rng = np.random.default_rng(1000 * Hm + 10 * Wm + C + shift)
    nb = (-(-Hm >> shift), -(-Wm >> shift))
    for N in (1, 3):
        p = _likelihoods(rng, (N, C, Hm, Wm))
        want = _block_sums(_terms(p), shift)
        add = rng.uniform(0.0, 100.0, (N, *nb)).astype(np.float32)
        for layout in LAYOUTS:
            first = None
            for offset in (0, 1):
                tag = f"{Hm}x{Wm} shift {shift} C {C} N {N} {layout} offset {offset}"
                pd = _store(p, layout, offset)
                assert pd.shape == (N, C, Hm, Wm)
                out = ops.block_bits(pd, shift)
                assert out.shape == (N, *nb) and out.dtype == torch.float32 and out.is_contiguous()
                got = out.cpu().numpy()
                print(f"block_bits {tag}: max rel err {np.abs(got - want).max() / np.abs(want).max():.3e}")
                assert_close(got, want, 1e-4, f"block_bits {tag}")
                assert np.array_equal(_bits(ops.block_bits(pd, shift)), _bits(out)), f"two runs differ: {tag}"
                if first is None:
                    first = _bits(out)
                assert np.array_equal(_bits(out), first), f"the bits depend on the alignment: {tag}"
                for n in range(N):
                    alone = ops.block_bits(pd[n:n + 1], shift)
                    assert np.array_equal(_bits(alone), _bits(out[n:n + 1])), f"image {n} depends on its batch: {tag}"
                summed = ops.block_bits(pd, shift, _dev(add, offset))
                assert summed.dtype == torch.float32
                assert np.array_equal(_bits(summed), _bits(add + got)), f"add is not one fp32 addition: {tag}"


@pytest.mark.parametrize("h,w,shift", [(1, 1, 6), (64, 64, 6), (65, 130, 6), (100, 70, 6), (128, 192, 6), (100, 70, 3)])
def test_block_sse(h, w, shift):
    ops = _ops()
    rng = np.random.default_rng(1000 * h + w + shift)
    nb = (-(-h >> shift), -(-w >> shift))
    for N in (1, 3):
        a = rng.uniform(0.0, 1.0, (N, 3, h, w)).astype(np.float32)
        b = np.clip(a + rng.standard_normal(a.shape).astype(np.float32) * 0.05, 0.0, 1.0).astype(np.float32)
        want = _block_sums((a.astype(np.float64) - b.astype(np.float64)) ** 2, shift)
        for la in LAYOUTS:                  # the order of a sum is that of a's storage: one set of bits per layout of a
            first = None
            for lb in LAYOUTS:
                for offset in (0, 1):
                    tag = f"{h}x{w} shift {shift} N {N} a {la} b {lb} offset {offset}"
                    ad, bd = _store(a, la, offset), _store(b, lb, offset)
                    out = ops.block_sse(ad, bd, shift)
                    assert out.shape == (N, *nb) and out.dtype == torch.float32 and out.is_contiguous()
                    got = out.cpu().numpy()
                    print(f"block_sse {tag}: max rel err {np.abs(got - want).max() / np.abs(want).max():.3e}")
                    assert_close(got, want, 1e-4, f"block_sse {tag}")
                    assert np.array_equal(_bits(ops.block_sse(ad, bd, shift)), _bits(out)), f"two runs differ: {tag}"
                    if first is None:
                        first = _bits(out)
                    assert np.array_equal(_bits(out), first), f"the bits depend on the alignment or on b's layout: {tag}"
                    for n in range(N):
                        alone = ops.block_sse(ad[n:n + 1], bd[n:n + 1], shift)
                        assert np.array_equal(_bits(alone), _bits(out[n:n + 1])), f"image {n} depends on its batch: {tag}"
    assert float(ops.block_sse(ad, ad, shift).abs().max()) == 0.0


def test_functional_copies_only_what_the_kernels_cannot_walk():
    from image_compression_amd import functional as F
    rng = np.random.default_rng(5)
    p = _likelihoods(rng, (2, 192, 8, 12))
    want = _bits(_ops().block_bits(_store(p, "nchw", 0), 2))
    pd = _store(p, "last", 0)
    with pytest.raises(RuntimeError, match="dense"):
        _ops().block_bits(pd[:, :, ::2], 2)
    half = F.block_bits(pd[:, :, ::2], 1)                       # a strided view: copied dense, NCHW
    assert np.array_equal(_bits(half), _bits(_ops().block_bits(_store(p[:, :, ::2], "nchw", 0), 1)))
    assert np.array_equal(_bits(F.block_bits(_store(p, "nchw", 0).requires_grad_(True).detach(), 2)), want)
    with pytest.raises(RuntimeError, match="inference only"):
        F.block_bits(_store(p, "nchw", 0).requires_grad_(True), 2)
    with torch.no_grad():
        assert np.array_equal(_bits(F.block_bits(_store(p, "nchw", 0).requires_grad_(True), 2)), want)
    with pytest.raises(ValueError, match="add"):
        F.block_bits(pd, 2, add=torch.zeros(2, 2, 2, device=DEV))
    a = torch.rand(2, 3, 70, 100, device=DEV)
    assert F.block_sse(a, a * 0.5).shape == (2, 2, 2)            # shift 6 by default


def test_one_block_sums_to_the_cross_entropy_loss():
    from image_compression_amd import _lib
    rng = np.random.default_rng(6)
    for shape in ((2, 192, 8, 12), (1, 5, 9, 7)):
        p = _likelihoods(rng, shape)
        for layout in LAYOUTS:
            pd = _store(p, layout, 0)
            one = _ops().block_bits(pd, 6)
            assert one.shape == (shape[0], 1, 1)
            ce = float(_lib.ops().ce_loss_fwd(pd if layout == "nchw" else pd.permute(0, 2, 3, 1)))
            assert_close(np.asarray([float(one.double().sum())]), np.asarray([ce]), 1e-4, f"one block against ce_loss_fwd {shape}")
            assert_close(np.asarray([ce]), np.asarray([_terms(p).sum()]), 1e-4, f"ce_loss_fwd against numpy {shape}")


# torch.ops.imgcomp.ce_loss_fwd on `_fixed_p()`, recorded on an MI355X from the commit before the term moved into
# csrc/bits_term.h: its fp32 bit pattern.  The device code of elementwise.hip is instruction for instruction what it
# was, so the sum must be too.
CE_LOSS_BITS_BEFORE = 0x45ba24a0    # 5956.578125


def _fixed_p():
    """4099 likelihoods (k + 1) / 2^24, k a fixed permutation-like sequence: exact in fp32 on every host."""
    k = (np.arange(4099, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 24)
    return ((k + np.uint64(1)).astype(np.float64) / float(1 << 24)).astype(np.float32)


def test_ce_loss_fwd_keeps_its_bits():
    from image_compression_amd import _lib
    p = _fixed_p()
    assert p.min() > 0.0 and p.max() <= 1.0 and np.array_equal(p.astype(np.float64) * (1 << 24) % 1, np.zeros(4099))
    out = _lib.ops().ce_loss_fwd(torch.from_numpy(p).to(DEV))
    bits = int(_bits(out.reshape(1))[0])
    print(f"ce_loss_fwd on the fixed p: {float(out)!r}, bits 0x{bits:08x}")
    assert bits == CE_LOSS_BITS_BEFORE


# ------------------------------------------------------------------ the model
ARCHS = [("Compressor2018", "conv"), ("MeanScaleCompressor2018", "conv"), ("CheckerboardCompressor2018", "conv"),
         ("CheckerboardCompressor2018", "fused"), ("GainedMeanScaleCompressor2018", "conv"),
         ("RegionGainedMeanScaleCompressor2018", "conv")]
ARCH_IDS = [a.replace("Compressor2018", "") + ("-fused" if k == "fused" else "") for a, k in ARCHS]
DTYPES = ["fp32_split", "fp32"]
BIG, ODD = (2, 3, 128, 192), (2, 3, 100, 70)


@functools.lru_cache(maxsize=None)
def _rd_model(arch, kernel, dtype):
    from image_compression_amd import modelling
    cfg = cfg_of(arch, dtype=dtype)
    cfg.MODEL.CONTEXT.KERNEL = kernel
    torch.manual_seed(0)
    model = modelling.build_model(cfg)
    if hasattr(model, "context_mean"):
        _set_context(model)
    return model.to(DEV).eval()


class _x32:
    """The last analysis conv scaled by 32 (the existing tests' "x32": symbols up to a few dozen), and the gain
    tables of a model that has them set to test_gained_gpu's values; undone on exit."""

    def __init__(self, model):
        self.w = _last_analysis_conv(model).weight
        self.tables = _tables(model) if hasattr(model, "gain") else None

    def __enter__(self):
        with torch.no_grad():
            self.w.mul_(32.0)
        if self.tables is not None:
            self.tables.__enter__()

    def __exit__(self, *exc):
        with torch.no_grad():
            self.w.div_(32.0)
        if self.tables is not None:
            self.tables.__exit__(*exc)


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _clean(model):
    return getattr(model, "_gains", None) is None and getattr(model, "_idx", None) is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("arch,kernel", ARCHS, ids=ARCH_IDS)
def test_map_of_whole_blocks_is_the_eval_forward(arch, kernel, dtype):
    from image_compression_amd import functional as F
    model = _rd_model(arch, kernel, dtype)
    x = _batch(BIG)
    N, _, H, W = BIG
    with _x32(model), torch.no_grad():
        before = model.compress(x)
        x_fwd, losses = model(x)
        rd = model.rate_distortion_map(x, likelihoods=True)
        assert _clean(model)
        assert model.compress(x) == before, "compress after rate_distortion_map gives other bytes"
        plain = model.rate_distortion_map(x)
    assert plain.p_y is None and plain.p_z is None
    assert torch.equal(rd.x_hat, x_fwd), "x_hat is not the eval forward's reconstruction"
    assert rd.pixels.tolist() == [[4096] * 3] * 2
    for name in ("bits_y", "bits_z", "bits", "sse"):
        t = getattr(rd, name)
        assert t.shape == (N, H // 64, W // 64) and t.dtype == torch.float32 and bool(torch.isfinite(t).all()), name
        assert torch.equal(t, getattr(plain, name)), name
    assert torch.equal(plain.x_hat, rd.x_hat)
    assert rd.p_y.shape == (N, 192, H // 16, W // 16) and rd.p_z.shape == (N, 192, H // 64, W // 64)
    npix = N * H * W
    for name, loss in (("bits_y", "y_entropy"), ("bits_z", "z_entropy"), ("bits", "bpp")):
        got, want = float(getattr(rd, name).double().sum()), float(losses[loss]) * npix
        print(f"{arch} {kernel} {dtype} {name}: {got:.6f} against {want:.6f}, rel {_rel(got, want):.3e}")
        assert want > 0.0 and _rel(got, want) <= 1e-4, (name, got, want)
    got, want = float(rd.sse.double().sum()) / (3 * npix), float(losses["MSE"])
    print(f"{arch} {kernel} {dtype} mse: {got:.8f} against {want:.8f}, rel {_rel(got, want):.3e}")
    assert _rel(got, want) <= 1e-4, (got, want)
    assert np.array_equal(_bits(rd.bits_y), _bits(F.block_bits(rd.p_y, 2)))
    assert np.array_equal(_bits(rd.bits_z), _bits(F.block_bits(rd.p_z, 0)))
    assert np.array_equal(_bits(rd.bits), _bits(rd.bits_y.cpu().numpy() + rd.bits_z.cpu().numpy()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("arch,kernel", ARCHS, ids=ARCH_IDS)
def test_map_of_a_padded_image(arch, kernel, dtype):
    from image_compression_amd import _lib
    model = _rd_model(arch, kernel, dtype)
    x = _batch(ODD)
    N, _, h, w = ODD
    with _x32(model), torch.no_grad():
        rd = model.rate_distortion_map(x)
        assert _clean(model)
        x_pad = model(_lib.stream_ops().pad_edge(x, 128, 128))[0]
    assert rd.x_hat.shape == ODD and torch.equal(rd.x_hat, x_pad[:, :, :h, :w]), "x_hat is not the padded forward's, cropped"
    for name in ("bits_y", "bits_z", "bits", "sse"):
        t = getattr(rd, name)
        assert t.shape == (N, 2, 2) and bool(torch.isfinite(t).all()), name
    assert rd.pixels.tolist() == [[4096, 384], [2304, 216]] and rd.pixels.sum() == 7000
    d = (x.double() - rd.x_hat.double()).cpu().numpy() ** 2
    want = _block_sums(d, 6)
    assert_close(rd.sse.cpu().numpy(), want, 1e-4, "sse over the real pixels")


@pytest.mark.parametrize("dtype", DTYPES)
def test_region_model_with_a_uniform_map_is_the_gained_model(dtype):
    from image_compression_amd import codec
    region = _rd_model("RegionGainedMeanScaleCompressor2018", "conv", dtype)
    gained = _rd_model("GainedMeanScaleCompressor2018", "conv", dtype)
    before = gained.quality
    try:
        with _x32(region), _x32(gained), torch.no_grad():
            for shape, k in ((BIG, 0), (BIG, 77), (ODD, 255), (ODD, 130)):
                x = _batch(shape)
                hb, wb = -(-shape[2] // 64), -(-shape[3] // 64)
                region.set_quality_map(np.full((hb, wb), k, np.uint8))
                gained.set_quality(codec.code_quality(k, S))
                a, b = region.rate_distortion_map(x, likelihoods=True), gained.rate_distortion_map(x, likelihoods=True)
                assert _clean(region) and _clean(gained)
                for name in a._fields:
                    u, v = getattr(a, name), getattr(b, name)
                    same = np.array_equal(u, v) if name == "pixels" else torch.equal(u, v)
                    assert same, f"{name} differs from the gained model's at code {k}, {shape}"
            # two codes: the map runs, and is not the uniform one
            x = _batch(BIG)
            codes = np.asarray([[10, 10, 250], [10, 250, 250]], np.uint8)
            region.set_quality_map(codes)
            two = region.rate_distortion_map(x)
            region.set_quality_map(np.full((2, 3), 10, np.uint8))
            low = region.rate_distortion_map(x)
            for name in ("bits_y", "bits_z", "bits", "sse"):
                t = getattr(two, name)
                assert t.shape == (2, 2, 3) and bool(torch.isfinite(t).all()), name
            assert not torch.equal(two.bits, low.bits)
            # a map of another shape is refused against the padded size, in front of any launch
            region.set_quality_map(np.zeros((2, 3), np.uint8))
            with pytest.raises(ValueError, match="padded size 128 x 128"):
                region.rate_distortion_map(_batch(ODD))
            assert _clean(region)
    finally:
        region.set_quality_map(None)
        region.set_quality(before)
        gained.set_quality(before)


@pytest.mark.parametrize("arch", ["MeanScaleCompressor2018", "GainedMeanScaleCompressor2018"])
def test_run_eval_each(arch):
    from image_compression_amd import evaluation
    model = _rd_model(arch, "conv", "fp32_split")
    g = torch.Generator().manual_seed(11)
    batches = [_batch(BIG), torch.rand(*BIG, generator=g).to(DEV)]
    N, _, H, W = BIG
    ev = evaluation.Evaluator(model)
    ev.monitor = evaluation.Monitor(model.loss_names, {"psnr": evaluation.psnr})   # MS-SSIM's 5 levels need a larger image
    with _x32(model):
        each = ev.run_eval_each(batches)
        mean = ev.run_eval(batches)
        with torch.no_grad():
            rds = [model.rate_distortion_map(b) for b in batches]
            psnrs = [evaluation.psnr(rd.x_hat, b).cpu().numpy() for rd, b in zip(rds, batches)]
    assert not model.training and len(each) == 2 * N
    want_keys = {"bpp", "y_bpp", "z_bpp", "mse", "psnr", "worst_block"} | ({"quality"} if hasattr(model, "quality") else set())
    for i, res in enumerate(each):
        rd, n = rds[i // N], i % N
        assert set(res) == want_keys
        assert _rel(res["bpp"], float(rd.bits[n].double().sum()) / (H * W)) <= 1e-12, "the dicts are not in the images' order"
        assert _rel(res["y_bpp"] + res["z_bpp"], res["bpp"]) <= 1e-6
        assert _rel(res["psnr"], psnrs[i // N][n]) <= 1e-4, (res["psnr"], psnrs[i // N][n])
        per = (rd.sse[n].double().cpu().numpy() / rd.pixels)
        assert res["worst_block"] == tuple(int(v) for v in np.unravel_index(np.argmax(per), per.shape))
        if "quality" in res:
            assert res["quality"] == model.quality
    got, want = float(np.mean([r["bpp"] for r in each])), mean["bpp"]
    print(f"run_eval_each {arch}: mean bpp {got:.6f} against run_eval's {want:.6f}, rel {_rel(got, want):.3e}")
    assert _rel(got, want) <= 1e-4
