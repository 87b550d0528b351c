"""The distortion kernels (csrc/msssim.hip, csrc/elementwise.hip MSE / squared difference,
csrc/metrics.hip PSNR) against the fp64 CPU oracle at tile edges, every filter size class, both
inputs' gradients, the LowerBound gate, the trained regime, the metric mode and the refusals.
GPU only.

Shape arithmetic (msssim.hip): the fused 11-tap forward tiles 64 x 16 valid outputs (FTW, FTH), the
fused backward 32 x 22 pixels (BTW, BTH); a level of H x W has (H - 10) x (W - 10) valid outputs; a
pyramid level halves H and W rounding up (reflect pad).  Every filter size but 11 runs the generic
chain hfilt_k -> vstats_k and hfilt_k -> dmaps_k -> vadj_k -> hadj_k."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close, rel_err
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

DEV = "cuda"
DEFAULT_W = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
EPS = 1e-5  # the losses' default LowerBound

# (N, C, H, W), filter size, sigma, level weights (None: single-scale SSIMLoss)
FUSED_SINGLE = [
    ((1, 1, 11, 11), 11, 1.5, None),    # 1 x 1 valid map
    ((1, 1, 11, 74), 11, 1.5, None),    # Wv = 64: exactly one forward tile
    ((2, 1, 26, 75), 11, 1.5, None),    # Hv = 16, Wv = 65
    ((1, 2, 27, 138), 11, 1.5, None),   # Hv = 17, Wv = 128
    ((1, 1, 22, 32), 11, 1.5, None),    # exactly one backward tile
    ((1, 1, 23, 33), 11, 1.5, None),    # one backward tile plus one, both directions
    ((3, 2, 45, 65), 11, 1.5, None),    # C = 2, N = 3: n = p / C
]
FUSED_MULTI = [
    ((2, 3, 44, 64), 11, 1.5, (0.5, 0.5)),
    ((1, 3, 45, 43), 11, 1.5, (0.25, 0.35, 0.4)),    # odd/odd -> odd/even -> 12 x 11
    ((1, 1, 24, 45), 11, 1.5, (0.3, 0.7)),           # even H, odd W pooling
    ((1, 1, 176, 161), 11, 1.5, DEFAULT_W),          # last level 11 x 11: one valid output
]
GENERIC = [
    ((1, 1, 384, 385), 3, 1.5, (0.125,) * 8),        # MAXLEV; last level 3 x 4
    ((2, 3, 40, 56), 7, 0.8, (0.25, 0.35, 0.4)),
    ((1, 2, 61, 33), 15, 1.5, (0.3, 0.7)),           # MAXF
    ((1, 1, 17, 19), 8, 3.0, (0.3, 0.7)),            # even window
    ((1, 3, 5, 4), 1, 2.0, None),                    # one-tap window
]
GEOMETRY = FUSED_SINGLE + FUSED_MULTI + GENERIC


def _id(case):
    (n, c, h, w), fs, _, wts = case
    return f"{n}x{c}x{h}x{w}-f{fs}-" + ("ssim" if wts is None else f"L{len(wts)}")


# ------------------------------------------------------------------ inputs (CPU fp32, made once)
@functools.lru_cache(maxsize=None)
def _noisy(shape, seed=0):
    """a uniform, b = a + 0.1 randn clamped: every level term near 0.95."""
    a = torch.rand(*shape, generator=torch.Generator().manual_seed(100 + seed))
    b = (a + 0.1 * torch.randn(*shape, generator=torch.Generator().manual_seed(200 + seed))).clamp(0, 1)
    return a, b


@functools.lru_cache(maxsize=None)
def _anti(shape):
    """b = 1 - a + 0.05 randn clamped: anti-correlated, structure terms negative (below eps)."""
    a = torch.rand(*shape, generator=torch.Generator().manual_seed(300))
    b = (1.0 - a + 0.05 * torch.randn(*shape, generator=torch.Generator().manual_seed(301))).clamp(0, 1)
    return a, b


@functools.lru_cache(maxsize=None)
def _smooth(shape, noise):
    """The regime the model is trained into: a smooth image and a reconstruction close to it."""
    N, C, H, W = shape
    y = torch.arange(H, dtype=torch.float64)[:, None] / (H - 1)
    x = torch.arange(W, dtype=torch.float64)[None, :] / (W - 1)
    s = torch.linspace(0.6, 1.0, N * C, dtype=torch.float64).reshape(N, C, 1, 1)
    base = ((0.5 + 0.35 * torch.sin(3 * y + 1) * torch.cos(2 * x)) * s).float()
    b = (base + noise * torch.randn(*shape, generator=torch.Generator().manual_seed(400))).clamp(0, 1)
    return base, b


# ------------------------------------------------------------------ the two sides
def _backprop(loss, case, log_scale, up):
    """The upstream gradient: per-image weights linspace(-1, 2, N) for the per-image output of the
    single-scale log form (a swapped gout[n] cannot pass), else the scalar `up`."""
    if case[3] is None and log_scale:
        wt = torch.linspace(-1, 2, case[0][0]).to(device=loss.device, dtype=loss.dtype)
        (loss * wt).sum().backward()
    else:
        (loss * up).backward()


@contextlib.contextmanager
def _oracle_terms():
    """Records what the oracle hands to its LowerBound: per level the per-image (ssim, cs) means."""
    rec, orig = [], ref_cpu.lower_bound

    def spy(x, b):
        rec.append(x.detach().clone())
        return orig(x, b)

    ref_cpu.lower_bound = spy
    try:
        yield rec
    finally:
        ref_cpu.lower_bound = orig


def _used_terms(rec, nlev):
    """The level terms a loss is made of: cs of every level but the last, ssim of the last."""
    assert len(rec) == 2 * nlev, (len(rec), nlev)
    return torch.stack([rec[2 * l + 1] if l < nlev - 1 else rec[2 * l] for l in range(nlev)])


def _oracle_run(a, b, case, log_scale, up, dtype):
    _, fs, sigma, wts = case
    ar, br = (t.detach().clone().to(dtype).requires_grad_(True) for t in (a, b))  # the shared inputs stay as made
    with _oracle_terms() as rec:
        if wts is None:
            loss = ref_cpu.ssim_loss(ar, br, size=fs, sigma=sigma, log_scale=log_scale, eps=EPS)
        else:
            loss = ref_cpu.ms_ssim_loss(ar, br, size=fs, sigma=sigma, log_scale=log_scale, eps=EPS, weights=wts)
    _backprop(loss, case, log_scale, up)
    terms = _used_terms(rec, 1 if wts is None else len(wts))
    return loss.detach().numpy(), ar.grad.numpy(), br.grad.numpy(), terms.numpy()


@functools.lru_cache(maxsize=None)
def _oracle(kind, case, log_scale, up=0.37, dtype=torch.float64):
    a, b = _inputs(kind, case)
    return _oracle_run(a, b, case, log_scale, up, dtype)


def _inputs(kind, case):
    if kind == "noisy":
        return _noisy(case[0])
    if kind == "anti":
        return _anti(case[0])
    return _smooth(case[0], kind)  # kind: the noise level


def _hip(a, b, case, log_scale, up=0.37, need=(True, True)):
    from image_compression_amd.modelling.loss import MS_SSIMLoss, SSIMLoss
    _, fs, sigma, wts = case
    kw = dict(filter_size=fs, filter_sigma=sigma, log_scale=log_scale, eps=EPS)
    mod = SSIMLoss(**kw) if wts is None else MS_SSIMLoss(weights=wts, **kw)
    ad = a.to(DEV).requires_grad_(need[0])
    bd = b.to(DEV).requires_grad_(need[1])
    loss = mod(ad, bd)
    _backprop(loss, case, log_scale, up)
    return (loss.detach().cpu().numpy(), None if ad.grad is None else ad.grad.cpu().numpy(),
            None if bd.grad is None else bd.grad.cpu().numpy())


def _check_reference(ref, far_from_eps=True):
    """The input conditions, on the oracle's own fp64 values."""
    lr, gar, gbr, terms = ref
    assert np.isfinite(lr).all() and np.isfinite(gar).all() and np.isfinite(gbr).all(), "reference not finite"
    assert np.isfinite(terms).all()
    if far_from_eps:  # the fp32 clamp decision cannot differ from the fp64 one
        assert np.abs(terms - EPS).min() >= 1e-3, terms


def _compare(got, ref, rtol=1e-4, name=""):
    assert_close(got[0], ref[0], rtol, name + " loss")
    assert_close(got[1], ref[1], rtol, name + " d/d img1")
    assert_close(got[2], ref[2], rtol, name + " d/d img2")


# ------------------------------------------------------------------ 1. the geometry matrix
@pytest.mark.parametrize("log_scale", [True, False], ids=["log", "lin"])
@pytest.mark.parametrize("case", GEOMETRY, ids=_id)
def test_ssim_geometry(case, log_scale):
    ref = _oracle("noisy", case, log_scale)
    _check_reference(ref)
    assert ref[3].min() > 0.9 and ref[3].max() <= 1.0 + 1e-12, ref[3]  # images that agree: no level clamped
    a, b = _noisy(case[0])
    _compare(_hip(a, b, case, log_scale), ref, 1e-4, _id(case))


@pytest.mark.parametrize("case", GENERIC, ids=_id)
def test_generic_cases_take_the_generic_path(case):
    """Only the generic chain keeps the five horizontal moment planes (th), the derivative maps (D)
    and their vertical adjoint (E) in the workspace; the fused tile kernels hold them in LDS.  A
    workspace with room for all three says the library plans the generic kernels for this size."""
    from image_compression_amd import _lib
    (N, C, H, W), fs, _, wts = case
    nlev = 1 if wts is None else len(wts)
    Hv, Wv = H - fs + 1, W - fs + 1
    planes = 5 * N * C * 4 * (2 * H * Wv + Hv * Wv)
    assert _lib.load().ic_msssim_ws(N, C, H, W, nlev, fs) >= planes
    if H >= 11 and W >= 11:  # the same image through the 11-tap fused kernels plans none of them
        assert _lib.load().ic_msssim_ws(N, C, H, W, 1, 11) < _lib.load().ic_msssim_ws(N, C, H, W, 1, 10)


@pytest.mark.parametrize("log_scale", [True, False], ids=["log", "lin"])
def test_ssim_batch_limit(log_scale):
    """N = 1024: the whole of combine_k's vals[1024], four rounds of its and coef_k's image loop."""
    case = ((1024, 1, 11, 11), 11, 1.5, None)
    ref = _oracle("noisy", case, log_scale)
    _check_reference(ref)
    a, b = _noisy(case[0])
    _compare(_hip(a, b, case, log_scale), ref, 1e-4, "N=1024")


DETERMINISM = [FUSED_MULTI[0], GENERIC[1]]


@pytest.mark.parametrize("case", DETERMINISM, ids=_id)
def test_ssim_bitwise_repeatable(case):
    """Fixed-order reductions (msssim.hip header): two runs agree bit for bit."""
    a, b = _noisy(case[0])
    for log_scale in (True, False):
        r1, r2 = _hip(a, b, case, log_scale), _hip(a, b, case, log_scale)
        for x, y in zip(r1, r2):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("case", DETERMINISM, ids=_id)
def test_ssim_single_gradient_requested(case):
    """need_a alone and need_b alone (a null ga / gb in scale_out_k) give the tensors of both."""
    a, b = _noisy(case[0])
    both = _hip(a, b, case, True)
    only_a = _hip(a, b, case, True, need=(True, False))
    only_b = _hip(a, b, case, True, need=(False, True))
    assert only_a[2] is None and only_b[1] is None
    assert np.array_equal(only_a[1], both[1]) and np.array_equal(only_b[2], both[2])
    assert np.array_equal(only_a[0], both[0]) and np.array_equal(only_b[0], both[0])


# ------------------------------------------------------------------ 2. the LowerBound gate
# log form only: the product form's reference gradient is 0 * inf = NaN on these inputs
@pytest.mark.parametrize("case", [FUSED_SINGLE[2], FUSED_SINGLE[6]], ids=_id)
def test_lower_bound_gate_per_image(case):
    """Anti-correlated images, upstream linspace(-1, 2, N): every image's ssim mean is below eps;
    image 0 (negative upstream: dLoss/dt > 0) is gated to exactly zero, the others pass with
    gradients of order 1/eps."""
    ref = _oracle("anti", case, True)
    _check_reference(ref)
    assert (ref[3] < EPS).all(), ref[3]
    assert not ref[1][0].any() and not ref[2][0].any() and np.abs(ref[1][1:]).max() > 1.0
    a, b = _anti(case[0])
    got = _hip(a, b, case, True)
    assert not got[1][0].any() and not got[2][0].any(), "gated image has a gradient"
    _compare(got, ref, 1e-4, _id(case) + " gate")


GATE_MULTI = [
    # case, levels below eps in the fp64 oracle
    (FUSED_MULTI[3], (0, 1, 2, 3)),      # level 4 (ssim) is not clamped
    (GENERIC[0], None),                  # four clamped, four not (asserted below)
    (GENERIC[1], (0, 1, 2)),             # all clamped, generic path
]


@pytest.mark.parametrize("up", [1.0, -1.0], ids=["up+1", "up-1"])
@pytest.mark.parametrize("case,clamped", GATE_MULTI, ids=[_id(c) for c, _ in GATE_MULTI])
def test_lower_bound_gate_per_level(case, clamped, up):
    """Upstream +1: dLoss/dt_l = -w_l / t_l < 0, every level passes (the clamped ones with 1/eps).
    Upstream -1: the clamped levels are gated and only the others' gradient is left: exactly zero
    where all are clamped."""
    ref = _oracle("anti", case, True, up)
    _check_reference(ref)
    below = tuple(int(l) for l in np.nonzero((ref[3] < EPS).all(axis=1))[0])
    assert ((ref[3] < EPS).all(axis=1) | (ref[3] > EPS).all(axis=1)).all()
    if clamped is None:
        assert len(below) == 4 and len(case[3]) == 8, below
    else:
        assert below == clamped, below
    a, b = _anti(case[0])
    got = _hip(a, b, case, True, up)
    if up < 0 and len(below) == len(case[3]):
        assert not ref[1].any() and not ref[2].any()
        assert not got[1].any() and not got[2].any(), "every level is gated, yet a gradient"
    else:
        assert np.abs(ref[1]).max() > 0
    _compare(got, ref, 1e-4, _id(case) + f" gate up={up}")


# ------------------------------------------------------------------ 3. the trained regime
def _err(x, ref):
    """The smallest rtol at which assert_close(x, ref, rtol) passes."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(x - ref) / (max(np.abs(ref).max(), 1e-30) + np.abs(ref))).max())


TRAINED = [((2, 3, 45, 65), 11, 1.5, None), FUSED_MULTI[0], ((1, 3, 176, 161), 11, 1.5, DEFAULT_W)]


@pytest.mark.parametrize("log_scale", [True, False], ids=["log", "lin"])
@pytest.mark.parametrize("noise", [0.02, 0.002])
@pytest.mark.parametrize("case", TRAINED, ids=_id)
def test_ssim_trained_regime(case, noise, log_scale):
    """Smooth, nearly equal images: E[a^2] - E[a]^2 cancels and 1 - ssim is a small difference,
    so the reference's own formulas lose digits in fp32.  The bar is max(1e-4, 2 e_ref), e_ref the
    fp32 oracle's error against the fp64 one in assert_close's norm (the factor 2: another
    summation order and the 1-ulp reciprocal).  Measured on an MI355X: the
    kernels stay below e_ref's bar in every case."""
    ref = _oracle(noise, case, log_scale)
    ref32 = _oracle(noise, case, log_scale, dtype=torch.float32)
    _check_reference(ref)
    a, b = _smooth(case[0], noise)
    got = _hip(a, b, case, log_scale)
    rows = []
    for k, nm in enumerate(("loss", "d/d img1", "d/d img2")):
        e_ref, e_hip = _err(ref32[k], ref[k]), _err(got[k], ref[k])
        bar = max(1e-4, 2 * e_ref)
        rows.append((nm, e_ref, e_hip, bar))
        print(f"trained {_id(case)} noise={noise} {'log' if log_scale else 'lin'} {nm:9s} "
              f"e_ref={e_ref:.2e} e_hip={e_hip:.2e} bar={bar:.2e} normwise={rel_err(got[k], ref[k]):.2e}")
    for k, (nm, e_ref, e_hip, bar) in enumerate(rows):
        assert_close(got[k], ref[k], bar, f"{_id(case)} noise={noise} {nm} (e_ref {e_ref:.2e})")


# ------------------------------------------------------------------ 4. metric mode (single = 2)
METRIC = [FUSED_MULTI[0], FUSED_MULTI[1], GENERIC[1], FUSED_MULTI[3]]


def _metric_db(a, b, case):
    from image_compression_amd import evaluation
    _, fs, sigma, wts = case
    return evaluation.ms_ssim_db(a.to(DEV), b.to(DEV), filter_size=fs, filter_sigma=sigma, weights=wts).cpu().numpy()


@pytest.mark.parametrize("case", METRIC, ids=_id)
def test_ms_ssim_db(case):
    _, fs, sigma, wts = case
    a, b = _noisy(case[0])
    ref = ref_cpu.ms_ssim_metric_db(a.double() * 255, b.double() * 255, size=fs, sigma=sigma, weights=wts).numpy()
    assert np.isfinite(ref).all() and (ref > 0).all()
    got = _metric_db(a, b, case)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-4, (got, ref)


def test_ms_ssim_db_anticorrelated_is_zero():
    """Negative structure means clamp to 0 (non_negative): the product is 0 and the metric 0 dB."""
    case = FUSED_MULTI[3]
    a, b = _anti(case[0])
    ref = ref_cpu.ms_ssim_metric_db(a.double() * 255, b.double() * 255, weights=case[3]).numpy()
    assert (np.abs(ref) == 0).all()
    assert (np.abs(_metric_db(a, b, case)) == 0).all()


# ------------------------------------------------------------------ 5. refusals
def _valid_call_passes():
    case = FUSED_SINGLE[4]
    a, b = _noisy(case[0])
    _compare(_hip(a, b, case, True), _oracle("noisy", case, True), 1e-4, "after a refusal")


def _refused(mod, shape):
    a = torch.rand(*shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    with pytest.raises(RuntimeError):
        mod(a, a.clone().requires_grad_(True))
    torch.cuda.synchronize()
    _valid_call_passes()


def test_refuses_image_too_small_for_the_levels():
    from image_compression_amd.modelling.loss import MS_SSIMLoss
    _refused(MS_SSIMLoss(), (2, 3, 64, 64))  # level 3 is 8 x 8 < 11


def test_refuses_filter_size_16():
    from image_compression_amd.modelling.loss import MS_SSIMLoss
    _refused(MS_SSIMLoss(filter_size=16, weights=(0.5, 0.5)), (1, 1, 64, 64))


def test_refuses_nine_levels():
    from image_compression_amd.modelling.loss import MS_SSIMLoss
    _refused(MS_SSIMLoss(filter_size=1, weights=(1.0 / 9,) * 9), (1, 1, 64, 64))


def test_refuses_more_than_1024_images():
    from image_compression_amd.modelling.loss import SSIMLoss
    _refused(SSIMLoss(), (1025, 1, 11, 11))
    _refused(SSIMLoss(log_scale=True), (1025, 1, 11, 11))


# ------------------------------------------------------------------ 6. the MSE family
MSE_SHAPES = [
    (1, 1, 1, 1),         # numel 1
    (1, 3, 5, 17),        # 255
    (1, 1, 257, 1),       # 257
    (2, 3, 9, 7),
    (1, 5, 13, 4033),     # 256 * 1024 + 1: the second grid-stride pass of reduce_partial_k
]
LAYOUTS = [(False, False), (True, False), (False, True)]  # (input, target) channels-last


def _leaf(t, cl):
    d = t.to(DEV)
    if cl:
        d = d.contiguous(memory_format=torch.channels_last)
    return d.detach().requires_grad_(True)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["nchw-nchw", "nhwc-nchw", "nchw-nhwc"])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("shape", MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mse_family(shape, reduction, layout):
    from image_compression_amd.modelling.loss import MSELoss
    assert int(np.prod(shape)) in (1, 255, 257, 378, 256 * 1024 + 1)
    gen = torch.Generator().manual_seed(61)
    a = torch.rand(*shape, generator=gen)
    b = (a + 0.1 * torch.randn(*shape, generator=gen)).clamp(0, 1)
    g = torch.randn(*shape, generator=gen) if reduction == "none" else torch.tensor(-1.7)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    lr = torch.nn.functional.mse_loss(ar, br, reduction=reduction)
    lr.backward(g.double())
    ad, bd = _leaf(a, layout[0]), _leaf(b, layout[1])
    l = MSELoss(reduction=reduction)(ad, bd)
    assert l.shape == lr.shape
    l.backward(g.to(DEV))
    assert_close(l.detach().cpu().numpy(), lr.detach().numpy(), 1e-5, f"mse {reduction}")
    assert_close(ad.grad.cpu().numpy(), ar.grad.numpy(), 1e-5, f"mse {reduction} d/d input")
    assert_close(bd.grad.cpu().numpy(), br.grad.numpy(), 1e-5, f"mse {reduction} d/d target")


# ------------------------------------------------------------------ 7. PSNR
PSNR_SHAPES = [
    (3, 1, 1, 7),      # fewer elements than PSNR_NB chunks; per % 4 != 0: scalar path
    (2, 3, 4, 4),      # vector path, 12 live blocks of 128
    (1, 3, 5, 7),      # scalar path
    (2, 3, 64, 64),
]


def _psnr_ref(a, b):
    return ref_cpu.psnr_metric(a.double() * 255, b.double() * 255).numpy()


@pytest.mark.parametrize("shape", PSNR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_psnr(shape):
    from image_compression_amd import evaluation
    a, b = _noisy(shape, seed=7)
    ref = _psnr_ref(a, b)
    assert np.isfinite(ref).all()
    got = evaluation.psnr(a.to(DEV), b.to(DEV)).cpu().numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-4, (got, ref)


@pytest.mark.parametrize("off", [(1, 0), (0, 1), (1, 1)], ids=["a+1", "b+1", "both+1"])
def test_psnr_misaligned_base(off):
    """per % 4 == 0 but an image starts one float into its buffer: not 16-byte aligned, scalar path."""
    from image_compression_amd import evaluation
    shape = (2, 3, 8, 8)
    a, b = _noisy(shape, seed=8)
    n = a.numel()
    views = []
    for t, o in zip((a, b), off):
        buf = torch.zeros(n + 8, device=DEV)
        v = buf[o:o + n].view(shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * o
        views.append(v)
    got = evaluation.psnr(*views).cpu().numpy()
    assert np.abs(got - _psnr_ref(a, b)).max() <= 1e-4


@pytest.mark.parametrize("shape", [(3, 1, 1, 7), (2, 3, 4, 4)], ids=["scalar", "vector"])
def test_psnr_identical_images_is_inf(shape):
    from image_compression_amd import evaluation
    a, _ = _noisy(shape, seed=7)
    assert np.isposinf(_psnr_ref(a, a)).all()
    assert torch.isposinf(evaluation.psnr(a.to(DEV), a.to(DEV).clone())).all()
