"""Encode-time latent refinement without a GPU: the exported symbols and the shape kernels of torch.ops.imgcomp_refine,
the host-side argument checks of the entry points, the refusals of `compress_each_refined` in front of any launch, the
update rule restated in numpy float32 (`adam_evaluate`, which tests/test_refine_gpu.py holds the kernel to bit for bit)
against a float64 evaluation, and the whole loop restated in torch fp64 on oracle.ref_cpu (`oracle_refine`, the
reference of the GPU test's gains).

The oracle's figures on the inputs below (Compressor2018, seed-0 weights, 8 Adam steps, lr 0.1; J per pixel, image 0 /
image 1), as `test_oracle_loop_lowers_j` prints them:
    lambda 256:   J 77.5734 / 59.0449 -> 61.8319 / 44.6658   (-20.29 % / -24.35 %), falling at every step
    lambda 1:     J 1.38458 / 1.29095 -> 1.33739 / 1.26198   (-3.41 % / -2.24 %), flat after seven steps
    lambda 0.01:  J 1.08878 / 1.06672 -> 1.02099 / 1.02023   (-6.23 % / -4.36 %), flat after seven steps"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from test_gained import cfg_of

F32 = np.float32
LIMIT = 2 ** 30
STEPS, LR = 8, 0.1
LAMBDAS = (256.0, 1.0, 0.01)


# ------------------------------------------------------------------ the update rule, restated
def bias_corrections(t):
    """(c1, c2) = 1 / (1 - beta^t) of Adam step t >= 1, in double: the caller's part of the rule."""
    return 1.0 / (1.0 - 0.9 ** t), 1.0 / (1.0 - 0.999 ** t)


def evaluate(v, mu):
    """(sym int32, y_hat float32) of the Evaluate rule on float32 arrays: symbol_of(v - mu), float(sym) + mu; the rule
    of codec_sym.h: rint, clamped to +-2^30 by fmax / fmin (which drop a NaN), then 2^30 where a NaN is left."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = v if mu is None else v - mu
        q = np.fmin(np.fmax(np.rint(d), F32(-LIMIT)), F32(LIMIT))
        sym = np.where(q == q, q, F32(LIMIT)).astype(np.int32)
        y_hat = sym.astype(F32)
        return sym, (y_hat if mu is None else y_hat + mu)


def adam_evaluate(v, m, u, g, mu, lr, t):
    """ic_refine_update in numpy float32, one rounding per operation in the kernel's order -> (v, m, u, sym, y_hat);
    g None: no step."""
    assert all(a is None or a.dtype == F32 for a in (v, m, u, g, mu))
    if g is not None:
        c1, c2 = (F32(c) for c in bias_corrections(t))
        with np.errstate(invalid="ignore", over="ignore"):
            m = F32(0.9) * m + F32(0.1) * g
            u = F32(0.999) * u + F32(0.001) * (g * g)
            v = v - (F32(lr) * (m * c1)) / (np.sqrt(u * c2) + F32(1e-8))
        assert v.dtype == m.dtype == u.dtype == F32
    return (v, m, u, *evaluate(v, mu))


def _adam64(v, m, u, g, lr, t):
    c1, c2 = bias_corrections(t)
    v, m, u, g = (a.astype(np.float64) for a in (v, m, u, g))
    m = 0.9 * m + 0.1 * g
    u = 0.999 * u + 0.001 * g * g
    return v - lr * m * c1 / (np.sqrt(u * c2) + 1e-8), m, u


def update_case(shape, seed, nan=False):
    """(v, m, u, g, mu) float32 of one update test: a latent-like v, moments as a few steps leave them."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(shape) * 4).astype(F32)
    g = (rng.standard_normal(shape) * np.exp(rng.uniform(-6, 2, shape))).astype(F32)
    m = (rng.standard_normal(shape) * 0.1).astype(F32)
    u = (rng.uniform(0, 1, shape) ** 4).astype(F32)
    mu = rng.standard_normal(shape).astype(F32)
    g.reshape(-1)[::7] = 0.0            # exact zeros: sqrt(0) + eps
    u.reshape(-1)[::14] = 0.0
    if nan:
        v.reshape(-1)[3] = np.nan
        v.reshape(-1)[5] = 3.0e9        # beyond 2^30
        v.reshape(-1)[6] = -3.0e9
    return v, m, u, g, mu


@pytest.mark.parametrize("t", [1, 5])
def test_float32_restatement_agrees_with_float64(t):
    v, m, u, g, mu = update_case((3, 5, 6), 11)
    got = adam_evaluate(v, m, u, g, mu, LR, t)
    want = _adam64(v, m, u, g, LR, t)
    for name, a, b in zip("vmu", got, want):
        assert_close(a, b, 1e-4, f"{name} at step {t}")
    sym, y_hat = got[3], got[4]
    assert sym.dtype == np.int32 and np.array_equal(sym, np.rint(got[0] - mu).astype(np.int32))
    assert np.array_equal(y_hat, sym.astype(F32) + mu)
    # no step, no mean
    v2, m2, u2, sym2, y2 = adam_evaluate(v, m, u, None, None, LR, t)
    assert v2 is v and m2 is m and u2 is u and np.array_equal(y2, np.rint(v)) and np.array_equal(sym2, y2.astype(np.int32))


def test_symbol_rule_at_its_edges():
    v = np.asarray([0.5, 1.5, -0.5, 2.5, np.nan, 3.0e9, -3.0e9, np.inf, 2047.49], F32)
    sym, y_hat = evaluate(v, None)
    assert sym.tolist() == [0, 2, 0, 2, -LIMIT, LIMIT, -LIMIT, LIMIT, 2047]     # half to even; fmax drops the NaN
    assert np.array_equal(y_hat, sym.astype(F32))


# ------------------------------------------------------------------ the ops and the entry points
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_library_exports_the_new_symbols():
    from image_compression_amd import _lib
    L = _lib.load()
    assert {"ic_refine_update", "ic_refine_dist_grad", "ic_refine_objective", "ic_refine_keep",
            "ic_refine_kmax"} <= _lib.exported_symbols()
    assert L.ic_version() == 4


def test_refine_ops_have_shape_kernels():
    from image_compression_amd import _lib
    ops = _lib.refine_ops()
    registered = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("imgcomp_refine::")}
    assert registered == {"update", "dist_grad", "objective", "keep", "kmax"}
    f64, i32 = torch.float64, torch.int32
    for shape in ((3, 5, 6), (2, 4, 4, 192)):
        v = _meta(*shape)
        for g, mu in ((None, None), (_meta(*shape), _meta(*shape))):
            sym, y_hat = ops.update(v, _meta(*shape), _meta(*shape), g, mu, 0.1, 10.0, 1000.0)
            assert sym.device.type == "meta" and sym.dtype == i32 and sym.shape == (v.numel(),)
            assert y_hat.dtype == torch.float32 and y_hat.shape == v.shape
    sym, _ = ops.update(_meta(2, 3, 4), None, None, None, None, 0.0, 1.0, 1.0)    # an evaluation needs no moments
    assert sym.shape == (24,)
    with pytest.raises(RuntimeError, match="moments"):
        ops.update(_meta(2, 3, 4), None, None, _meta(2, 3, 4), None, 0.1, 10.0, 1000.0)
    with pytest.raises(RuntimeError, match="shape"):
        ops.update(_meta(2, 3, 4), _meta(2, 3, 4), _meta(2, 3, 4), _meta(2, 3, 5), None, 0.1, 10.0, 1000.0)
    for bad in (dict(lr=0.0), dict(lr=-0.1), dict(lr=float("nan")), dict(lr=float("inf")), dict(c1=0.5), dict(c2=float("nan"))):
        kw = {**dict(lr=0.1, c1=10.0, c2=1000.0), **bad}
        with pytest.raises(ValueError):
            ops.update(_meta(2, 3, 4), _meta(2, 3, 4), _meta(2, 3, 4), _meta(2, 3, 4), None, kw["lr"], kw["c1"], kw["c2"])
    out = ops.objective(_meta(3, 2, 3), _meta(3, 2, 3), _meta(3, dtype=f64))
    assert out.dtype == f64 and out.shape == (3, 3)
    with pytest.raises(RuntimeError):
        ops.objective(_meta(3, 2, 3), _meta(3, 2, 2), _meta(3, dtype=f64))
    with pytest.raises(RuntimeError, match="float64"):
        ops.objective(_meta(3, 2, 3), _meta(3, 2, 3), _meta(3))
    gx = ops.dist_grad(_meta(2, 3, 8, 8), _meta(2, 3, 8, 8), _meta(2, dtype=f64))
    assert gx.dtype == torch.float32 and gx.shape == (2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        ops.dist_grad(_meta(2, 3, 8, 8), _meta(2, 3, 8, 7), _meta(2, dtype=f64))
    assert ops.keep(_meta(40, dtype=i32), _meta(40, dtype=i32), _meta(3, 4, dtype=f64), _meta(3, 4, dtype=f64),
                    _meta(4, dtype=i32), 3) is None
    with pytest.raises(RuntimeError):
        ops.keep(_meta(41, dtype=i32), _meta(41, dtype=i32), _meta(3, 4, dtype=f64), _meta(3, 4, dtype=f64),
                 _meta(4, dtype=i32), 3)
    with pytest.raises(ValueError):
        ops.keep(_meta(40, dtype=i32), _meta(40, dtype=i32), _meta(3, 4, dtype=f64), _meta(3, 4, dtype=f64),
                 _meta(4, dtype=i32), -1)
    k = ops.kmax(_meta(40, dtype=i32), 4)
    assert k.dtype == i32 and k.shape == (4,)
    with pytest.raises(RuntimeError):
        ops.kmax(_meta(40, dtype=i32), 3)


def test_pinned_namespaces_are_untouched():
    from test_abi import OP_NAMESPACES
    from image_compression_amd import _lib
    _lib.ops()
    assert "imgcomp_refine" not in OP_NAMESPACES and len(OP_NAMESPACES) == 5
    names = [n for n in torch._C._dispatch_get_all_op_names() if n.split("::")[0] in OP_NAMESPACES]
    assert len(names) == 69


def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal below returns before anything is launched: the pointers are null or never dereferenced."""
    from image_compression_amd import _lib
    L = _lib.load()
    ERR, p, q = 1001, 256, 512     # non-null addresses nothing reads: each call fails an earlier check
    nan, inf = float("nan"), float("inf")

    def update(v=p, m=p, u=p, g=p, mu=p, N=2, P=16, C=192, lr=0.1, c1=10.0, c2=1000.0, sym=p, y_hat=p):
        return L.ic_refine_update(v, m, u, g, mu, N, P, C, lr, c1, c2, sym, y_hat, None)

    for name in ("v", "sym", "y_hat", "m", "u"):
        assert update(**{name: None}) == ERR, name
    for bad in (dict(N=0), dict(N=65536), dict(P=0), dict(C=0), dict(P=2 ** 62), dict(lr=0.0), dict(lr=-1.0), dict(lr=nan),
                dict(lr=inf), dict(c1=0.5), dict(c1=nan), dict(c2=inf), dict(c2=0.0)):
        assert update(**bad) == ERR, bad

    def grad(x=p, x_hat=p, w=p, N=2, n=100, gx=p):
        return L.ic_refine_dist_grad(x, x_hat, w, N, n, gx, None)

    def objective(bits=p, sse=p, w=p, N=3, nb=6, out=p):
        return L.ic_refine_objective(bits, sse, w, N, nb, out, None)

    def keep(sym=p, best_sym=q, obj=p, best=p, best_step=p, step=1, N=4, n=10, mode=0):
        return L.ic_refine_keep(sym, best_sym, obj, best, best_step, step, N, n, mode, None)

    def kmax(sym=p, N=4, n=10, out=p):
        return L.ic_refine_kmax(sym, N, n, out, None)

    for fn, names in ((grad, ("x", "x_hat", "w", "gx")), (objective, ("bits", "sse", "w", "out")),
                      (keep, ("sym", "best_sym", "obj", "best")), (kmax, ("sym", "out"))):
        for name in names:
            assert fn(**{name: None}) == ERR, (fn.__name__, name)
        for bad in (dict(N=0), dict(N=65536), dict(N=-1)):
            assert fn(**bad) == ERR, (fn.__name__, bad)
    assert grad(n=0) == ERR and objective(nb=0) == ERR and keep(n=0) == ERR and kmax(n=0) == ERR
    assert keep(best_sym=p) == ERR                             # one buffer for both
    assert keep(mode=2) == ERR and keep(mode=-1) == ERR
    assert keep(mode=1, best_step=None) == ERR and keep(mode=1, step=-1) == ERR


def test_wrappers_refuse_host_tensors():
    from image_compression_amd import functional as IF
    z = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.refine_update(z, None, None, None, None)
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.refine_objective(torch.zeros(2, 1, 1), torch.zeros(2, 1, 1), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.refine_dist_grad(z, z, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.refine_kmax(torch.zeros(8, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.refine_keep(torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.float64),
                       torch.zeros(3, 2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 1)


# ------------------------------------------------------------------ compress_each_refined in front of any launch
def _cpu_model(arch, names=None):
    from image_compression_amd import modelling
    cfg = cfg_of(arch)
    if names is not None:
        cfg.MODEL.LOSS.DISTORTION_LOSS_NAMES = names
    torch.manual_seed(0)
    return modelling.build_model(cfg).eval()


def _state(model):
    return [(p.requires_grad, p.grad) for p in model.parameters()]


def test_report_fields():
    from image_compression_amd.modelling.meta_arch.bmshl2018 import RefineReport
    assert RefineReport._fields == ("before", "after", "bits_before", "bits_after", "sse_before", "sse_after", "step")


@pytest.mark.parametrize("arch", ["Compressor2018", "MeanScaleCompressor2018", "GainedMeanScaleCompressor2018"])
def test_refusals_come_before_any_launch(arch):
    """A host model and host images: any launch would raise RuntimeError naming the device; every refusal comes first."""
    model = _cpu_model(arch)
    x = torch.rand(2, 3, 72, 100)
    next(model.parameters()).requires_grad_(False)      # a mixed pattern to restore
    before = _state(model)
    for bad in (-1, 1.0, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="steps"):
            model.compress_each_refined(x, steps=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="lr"):
            model.compress_each_refined(x, lr=bad)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.compress_each_refined(x)
    model.eval()
    with pytest.raises(RuntimeError, match="ROCm"):     # everything passes: the first launch refuses the host tensor
        model.compress_each_refined(x, steps=2)
    after = _state(model)
    assert [a[0] for a in after] == [b[0] for b in before] and all(a[1] is b[1] for a, b in zip(after, before))
    if arch.startswith("Gained"):
        assert model._gains is None and model._qualities is None


def test_other_distortions_and_models_are_refused():
    x = torch.rand(1, 3, 64, 64)
    for names in (["MS_SSIMLoss"], ["MSE", "MS_SSIMLoss"], ["SSIMLoss"]):
        with pytest.raises(ValueError, match="distortion"):
            _cpu_model("Compressor2018", names).compress_each_refined(x)
    with pytest.raises(ValueError, match="Checkerboard"):
        _cpu_model("CheckerboardCompressor2018").compress_each_refined(x)
    with pytest.raises(ValueError, match="quality map"):
        _cpu_model("RegionGainedMeanScaleCompressor2018").compress_each_refined(x)


# ------------------------------------------------------------------ the loop in fp64 on oracle.ref_cpu
def pair():
    """The 2 x 3 x 64 x 64 input: rand under seed 1, image 1 squeezed to a quarter of its contrast about 0.5."""
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    x[1] = 0.5 + (x[1] - 0.5) * 0.25
    return x


def seed0_params(arch="Compressor2018"):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return {k: v.clone() for k, v in modelling.build_model(cfg_of(arch, dtype="fp32")).state_dict().items()}


def _bits64(p):
    return torch.clamp(-torch.log2(p + 1e-10), 0.0, 50.0).sum(dim=(1, 2, 3))


def oracle_refine(params, x, lam, steps=STEPS, lr=LR):
    """The rule of codec.py for Compressor2018 (no mean, no gains) in torch fp64 on oracle.ref_cpu -> (J of every
    evaluation (steps + 1, N), J before (N), J after (N)), J in bits."""
    from oracle import ref_cpu as R
    P = {k: v.double() for k, v in params.items()}
    x = x.double()
    w = lam / x.shape[1]
    with torch.no_grad():
        y = R.analysis(P, x)
        z_hat = torch.round(R.hyper_analysis(P, y.abs()))
        sigma = R.hyper_synthesis(P, z_hat)
    v, m, u = y.clone(), torch.zeros_like(y), torch.zeros_like(y)
    best, trace = None, []
    for t in range(steps + 1):
        y_hat = torch.round(v).requires_grad_(True)
        x_hat = R.lower_bound(R.upper_bound(R.synthesis(P, y_hat), 1.0), 0.0)
        D = ((x - x_hat) ** 2).sum(dim=(1, 2, 3))
        with torch.no_grad():
            _, p = R.conditional(y_hat, sigma, train=False, sym=y_hat)
            J = _bits64(p) + w * D
        trace.append(J.clone())
        best = J.clone() if best is None else torch.where(J < best, J, best)
        if t == steps:
            break
        g_d, = torch.autograd.grad((w * D).sum(), y_hat)
        vv = v.clone().requires_grad_(True)
        _, p = R.conditional(vv, sigma, u=torch.full_like(vv, 0.5), train=True)     # q = v: the likelihood at v itself
        g_r, = torch.autograd.grad(R.ce_loss(p), vv)
        g = g_d + g_r
        c1, c2 = bias_corrections(t + 1)
        m = 0.9 * m + 0.1 * g
        u = 0.999 * u + 0.001 * g * g
        v = v - lr * (m * c1) / (torch.sqrt(u * c2) + 1e-8)
    return torch.stack(trace).numpy(), trace[0].numpy(), best.numpy()


@functools.lru_cache(maxsize=None)
def oracle_gains(lam):
    """(J before, J after, the relative gain (before - after) / before) per image of `pair` at this lambda."""
    _, before, after = oracle_refine(seed0_params(), pair(), lam)
    return before, after, (before - after) / before


@pytest.mark.parametrize("lam", LAMBDAS)
def test_oracle_loop_lowers_j(lam):
    trace, before, after = oracle_refine(seed0_params(), pair(), lam)
    pixels = 64 * 64
    print(f"lambda {lam}: J per pixel {before / pixels} -> {after / pixels}, change {(after - before) / before * 100} %; "
          f"per evaluation {trace / pixels}")
    assert np.all(after < before), "the method bites on untrained weights in both regimes"
    assert np.all(after <= trace.min(axis=0)) and np.array_equal(before, trace[0])
    if lam == 256.0:
        assert np.all(np.diff(trace, axis=0) < 0), "distortion-dominated: J falls at every step"
