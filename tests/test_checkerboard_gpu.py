"""The checkerboard context model on the GPU: the gather / scatter, input and parameter kernels against numpy on
the same fp32 inputs, their backward against torch autograd on an fp64 restatement, CheckerboardCompressor2018's
training step against an fp64 oracle composed from oracle.ref_cpu's layers, the fresh model against
MeanScaleCompressor2018, the causality of `_context`, the eval forward against the model's own three bitstreams with
their rate, and the refusals between the models."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import HipReluMasks, assert_close, check_relu_ties, rel_err
from test_mean_scale_gpu import (DEV, EVAL_SHAPES, KINDS, TRAIN_SHAPES, _cfg, _changed, _dev, _ideal_bits, _latents, _model,
                                 _train_inputs)

pytestmark = pytest.mark.gpu

ARCH = "CheckerboardCompressor2018"
LIMIT = 4.0
# (N, C, H, W): a single position, a row of two, odd sizes both ways (the halves differ in length and the number of
# positions per row alternates), C = 4 (the 16-byte path of floats), several blocks with C % 16 == 0 (that of bytes)
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (2, 3, 3, 5), (1, 4, 4, 4), (3, 5, 5, 3), (2, 192, 8, 8)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _ops():
    from image_compression_amd import _lib
    return _lib.ckbd_ops()


def _anchors(H, W):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (i + j) % 2 == 0


def _dev_any(a, offset):
    """`_dev` for any dtype: the flat array 16-byte aligned, or one element past an aligned address."""
    t = torch.from_numpy(a.reshape(-1))
    if not offset:
        return t.to(DEV)
    buf = torch.empty(a.size + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.to(DEV)
    view = buf[1:]
    assert view.data_ptr() % 16 == a.itemsize and view.is_contiguous()
    return view


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.int32)


# ------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_and_scatter_are_numpy_mask_indexing_bitwise(shape, offset):
    ops = _ops()
    N, C, H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    A = _anchors(H, W)
    full = (N, H, W, C)
    for dtype in (np.uint8, np.int32, np.float32):
        a = rng.integers(0, 256, size=full).astype(dtype) if dtype != np.float32 else \
            rng.standard_normal(full).astype(np.float32)
        src = (_dev(a.reshape(-1), offset) if dtype == np.float32 else _dev_any(a, offset)).view(full)
        for parity, mask in ((0, A), (1, ~A)):
            want = a[:, mask, :].reshape(-1)                     # ascending (n, i, j, c)
            got = ops.gather(src, parity)
            assert got.dtype == src.dtype and got.dim() == 1 and got.numel() == want.size, (dtype, parity)
            assert np.array_equal(got.cpu().numpy(), want), (dtype.__name__, parity)
    a = rng.standard_normal(full).astype(np.float32)
    halves = [_dev(a[:, m, :].reshape(-1), offset) if m.any() else torch.empty(0, device=DEV) for m in (A, ~A)]
    nan = np.full(a.size, np.nan, dtype=np.float32)
    # both halves into a NaN-filled tensor: the original, bit for bit
    both = _dev(nan, offset).view(full)
    ops.scatter(halves[0], both, 0)
    ops.scatter(halves[1], both, 1)
    assert np.array_equal(_bits(both), a.reshape(-1).view(np.int32)) and not torch.isnan(both).any()
    # one half: exactly the other parity stays NaN
    for parity, mask in ((0, A), (1, ~A)):
        one = _dev(nan, offset).view(full)
        ops.scatter(halves[parity], one, parity)
        got = one.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.broadcast_to(~mask[None, :, :, None], full)), parity
        assert np.array_equal(got[:, mask, :], a[:, mask, :]), parity


def test_gather_indexes_in_64_bits_past_two_to_the_31_elements():
    """The only size at which the 64-bit index path runs: table rows (1 byte each) of a 4 x (2^29 + 2) map, each half
    against strided slicing of the rows on the device."""
    H, W = 4, 2 ** 29 + 2
    n = H * W
    src = torch.arange(251, device=DEV, dtype=torch.uint8).repeat(n // 251 + 1)[:n].view(1, H, W, 1)   # period 251, a prime
    assert src.numel() > 2 ** 31 and src.is_contiguous()
    for parity in (0, 1):
        want = torch.cat([src[0, i, (i + parity) % 2::2, 0] for i in range(H)])
        got = _ops().gather(src, parity)
        assert got.numel() == H * W // 2 and torch.equal(got, want), parity
        del got, want


# ------------------------------------------------------------------ the input and parameter kernels
def _operands(shape, seed):
    """fp32 (y, mu_h, sigma_h, a, b) laid out (N, H, W, C): one anchor with y == mu, b beyond +-4 planted where the
    tensor has room, and every other b at least 1e-3 from +-4."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    full = (N, H, W, C)
    y = (rng.standard_normal(full) * 5).astype(np.float32)
    mu = rng.standard_normal(full).astype(np.float32)
    y[0, 0, 0, 0] = mu[0, 0, 0, 0]                                 # (0, 0) is an anchor
    sigma = np.exp(rng.standard_normal(full)).astype(np.float32)
    a = rng.standard_normal(full).astype(np.float32)
    b = (rng.standard_normal(full) * 2).astype(np.float32)
    flat = b.reshape(-1)
    flat[1::7], flat[2::7], flat[3::11] = 5.5, -4.5, -7.0
    near = np.abs(np.abs(b) - LIMIT) < 1e-3
    b[near] = 3.0
    return y, mu, sigma, a, b


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_input_and_params_forward_are_numpy_on_the_same_fp32_inputs(shape, offset):
    ops = _ops()
    N, C, H, W = shape
    full = (N, H, W, C)
    y, mu_h, sigma_h, a, b = _operands(shape, 7 + H)
    A = np.broadcast_to(_anchors(H, W)[None, :, :, None], full)
    dev = lambda t: _dev(t.reshape(-1), offset).view(full)     # noqa: E731
    u, v = ops.input_fwd(dev(y), dev(mu_h))
    zero = np.float32(0.0)
    want_u, want_v = np.where(A, y, zero), np.where(A, np.abs(y - mu_h), zero)
    assert want_v.dtype == np.float32 and want_v[0, 0, 0, 0] == 0.0
    assert np.array_equal(_bits(u), want_u.reshape(-1).view(np.int32)), "u"
    assert np.array_equal(_bits(v), want_v.reshape(-1).view(np.int32)), "v"
    for t in (u, v):                                                # the masked zeros are +0.0
        assert not np.signbit(t.cpu().numpy()[~A]).any()
    mu, sigma = ops.params_fwd(dev(mu_h), dev(sigma_h), dev(a), dev(b))
    want_mu = np.where(A, mu_h, mu_h + a)
    assert want_mu.dtype == np.float32
    assert np.array_equal(_bits(mu), want_mu.reshape(-1).view(np.int32)), "mu"
    got = sigma.cpu().numpy()
    assert np.array_equal(got[A].view(np.int32), sigma_h[A].view(np.int32)), "sigma at the anchors"
    if (~A).any():
        assert (np.abs(b[~A]) > LIMIT).any() or b.size < 4, "no saturated b among the non-anchors"
        want = sigma_h.astype(np.float64) * np.exp(np.clip(b.astype(np.float64), -LIMIT, LIMIT))
        err = np.abs(got[~A] - want[~A]) / want[~A]
        print(f"params_fwd {shape} offset {offset}: sigma at the non-anchors, worst relative error {err.max():.2e}")
        assert err.max() <= 1e-6
    from image_compression_amd import functional
    assert functional.CKBD_LOG_SCALE_LIMIT == LIMIT


def _fp64_backward(shape, y, mu_h, sigma_h, a, b, du, dv, dmu, dsigma):
    """torch autograd on the fp64 restatement with torch.where masks -> the six gradients as numpy (N, H, W, C)."""
    N, C, H, W = shape
    A = torch.from_numpy(np.array(np.broadcast_to(_anchors(H, W)[None, :, :, None], (N, H, W, C))))     # a writable copy
    t = lambda x: torch.from_numpy(x).double().requires_grad_(True)     # noqa: E731
    y, mu_h2, sigma_h, a, b = t(y), t(mu_h), t(sigma_h), t(a), t(b)
    mu_in = t(mu_h)
    zero = torch.zeros((), dtype=torch.float64)
    u, v = torch.where(A, y, zero), torch.where(A, (y - mu_in).abs(), zero)
    (u * torch.from_numpy(du).double() + v * torch.from_numpy(dv).double()).sum().backward()
    mu = torch.where(A, mu_h2, mu_h2 + a)
    sigma = torch.where(A, sigma_h, sigma_h * torch.clamp(b, -LIMIT, LIMIT).exp())
    (mu * torch.from_numpy(dmu).double() + sigma * torch.from_numpy(dsigma).double()).sum().backward()
    return [g.grad.numpy() for g in (y, mu_in, mu_h2, sigma_h, a, b)]


def _close(got, want, name):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, name
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (name, float(np.abs(got - want).max()))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_ops_are_autograd_on_the_fp64_restatement(shape, offset):
    ops = _ops()
    N, C, H, W = shape
    full = (N, H, W, C)
    y, mu_h, sigma_h, a, b = _operands(shape, 11 + W)
    A = np.broadcast_to(_anchors(H, W)[None, :, :, None], full)
    assert np.all((np.abs(np.abs(b) - LIMIT) >= 1e-3)), "a b within 1e-3 of the clamp"
    rng = np.random.default_rng(5)
    du, dv, dmu, dsigma = (rng.standard_normal(full).astype(np.float32) for _ in range(4))
    want = _fp64_backward(shape, y, mu_h, sigma_h, a, b, du, dv, dmu, dsigma)
    dev = lambda t: _dev(t.reshape(-1), offset).view(full)     # noqa: E731
    dy, dmu_in = ops.input_bwd(dev(y), dev(mu_h), dev(du), dev(dv))
    dmu_h, dsigma_h, da, db = ops.params_bwd(dev(sigma_h), dev(b), dev(dmu), dev(dsigma))
    for got, ref, name in zip((dy, dmu_in, dmu_h, dsigma_h, da, db), want, ("dy", "dmu", "dmu_h", "dsigma_h", "da", "db")):
        _close(got, ref, name)
    # the y == mu anchor: no dv contribution; saturated b: db exactly 0; every masked gradient exactly 0
    assert float(dy[0, 0, 0, 0]) == du[0, 0, 0, 0] and float(dmu_in[0, 0, 0, 0]) == 0.0
    sat = (np.abs(b) > LIMIT) & ~A
    assert np.all(db.cpu().numpy()[sat] == 0.0) and np.all(db.cpu().numpy()[A] == 0.0) and np.all(da.cpu().numpy()[A] == 0.0)
    assert np.all(dy.cpu().numpy()[~A] == 0.0) and np.all(dmu_in.cpu().numpy()[~A] == 0.0)
    if sat.any():
        assert np.all(dsigma_h.cpu().numpy()[sat] != 0.0)


def test_autograd_functions_take_logical_tensors_of_either_layout():
    """ckbd_input / ckbd_params on (N, C, H, W) tensors, contiguous and channels-last: the same fp64 gradients."""
    from image_compression_amd.modelling.blocks.entropy_model import ckbd_input, ckbd_params
    shape = (2, 4, 5, 3)
    ops_in = _operands(shape, 3)
    rng = np.random.default_rng(6)
    grads = [rng.standard_normal(ops_in[0].shape).astype(np.float32) for _ in range(4)]
    want = _fp64_backward(shape, *ops_in, *grads)
    for fmt in (torch.contiguous_format, torch.channels_last):
        def lay(t, g=False):
            return torch.from_numpy(t).to(DEV).permute(0, 3, 1, 2).contiguous(memory_format=fmt).requires_grad_(g)

        y, mu_h, sigma_h, a, b = (lay(t, True) for t in ops_in)
        mu_in = lay(ops_in[1], True)
        du, dv, dmu, dsigma = (lay(t) for t in grads)
        u, v = ckbd_input(y, mu_in)
        mu, sigma = ckbd_params(mu_h, sigma_h, a, b)
        assert u.shape == v.shape == mu.shape == sigma.shape == y.shape
        (u * du + v * dv).sum().backward()
        (mu * dmu + sigma * dsigma).sum().backward()
        for t, ref, name in zip((y, mu_in, mu_h, sigma_h, a, b), want, ("dy", "dmu", "dmu_h", "dsigma_h", "da", "db")):
            _close(t.grad.permute(0, 2, 3, 1), ref, name)


# ------------------------------------------------------------------ the model
def _set_context(model, std_mean=0.02, std_scale=0.005):
    """Seeded normal context weights on all 25 taps (and small biases)."""
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for conv, std in ((model.context_mean, std_mean), (model.context_scale, std_scale)):
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * std)
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * std)
    return model


@functools.lru_cache(maxsize=None)
def _ckbd_model(kind, dtype):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return _set_context(modelling.build_model(_cfg(kind, dtype, ARCH))).to(DEV).eval()


class _zero_context:
    """The context weights and biases at zero; undone on exit."""

    def __init__(self, model):
        self.ps = [p for c in (model.context_mean, model.context_scale) for p in c.parameters()]

    def __enter__(self):
        self.saved = [p.detach().clone() for p in self.ps]
        with torch.no_grad():
            for p in self.ps:
                p.zero_()

    def __exit__(self, *exc):
        with torch.no_grad():
            for p, s in zip(self.ps, self.saved):
                p.copy_(s)


class _spy_context:
    """Records the (sigma, mu) `_context` returns, in call order."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __enter__(self):
        orig = self.model._context

        def spy(*args):
            out = orig(*args)
            self.seen.append(out)
            return out
        self.model._context = spy
        return self.seen

    def __exit__(self, *exc):
        del self.model._context


def _taps():
    di, dj = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    return (di + dj) % 2 == 0        # (2, 2) is the centre: di + dj even are the taps between positions of one parity


# ---- the training step against the fp64 oracle
def _oracle(params, x, uz, uy, kind, masks=None):
    """CheckerboardCompressor2018's training forward and backward in fp64 from oracle.ref_cpu's layers: the mean-scale
    oracle of tests/test_mean_scale_gpu.py with y~ quantised first, the two context convs (F.conv2d, padding 2) on
    the masked inputs, and the masked corrections."""
    from oracle import ref_cpu as R
    P = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    x, uz, uy = x.double(), uz.double(), uy.double()
    ctl = {"masks": masks} if masks else {}
    y = R.analysis(P, x)
    z = R.hyper_analysis(P, y, relu_ctl=ctl)
    z_tilde, _, ce_z = R.factorized(P, z, uz, True)
    t = z_tilde
    pre = "prior_synthesis._layers."
    for i, (s, k) in enumerate(((2, 5), (2, 5))):                       # the trunk: h_s but for its last layer
        t = R._relu(F.conv_transpose2d(t, P[f"{pre}{2 * i}.weight"], P[f"{pre}{2 * i}.bias"], stride=s, padding=k // 2,
                                       output_padding=s - 1), ctl)
    sigma_h = torch.clamp(F.conv_transpose2d(t, P[pre + "4.weight"], P[pre + "4.bias"], stride=1, padding=1).exp(),
                          1e-10, 1e10)
    mu_h = F.conv_transpose2d(t, P["prior_mean.weight"], P["prior_mean.bias"], stride=1, padding=1)
    y_tilde = y + (uy - 0.5)
    A = torch.from_numpy(_anchors(*y.shape[2:]))[None, None]
    zero = torch.zeros((), dtype=torch.float64)
    u, v = torch.where(A, y_tilde, zero), torch.where(A, (y_tilde - mu_h).abs(), zero)
    a = F.conv2d(u, P["context_mean.weight"], P["context_mean.bias"], padding=2)
    b = F.conv2d(v, P["context_scale.weight"], P["context_scale.bias"], padding=2)
    mu = torch.where(A, mu_h, mu_h + a)
    sigma = torch.where(A, sigma_h, sigma_h * torch.clamp(b, -LIMIT, LIMIT).exp())
    q, p_y = R.conditional(y, sigma, uy, True, "laplace" if kind.startswith("Laplacian") else "gauss", mean=mu)
    assert torch.equal(q.detach(), y_tilde.detach())
    ce_y = R.ce_loss(p_y)
    x_tilde = R.lower_bound(R.upper_bound(R.synthesis(P, y_tilde), 1.0), 0.0)
    npx = x.shape[0] * x.shape[2] * x.shape[3]
    mse = R.mse(x, x_tilde)
    bpp = (ce_z + ce_y) / npx
    total = 256.0 * mse + bpp
    total.backward()
    losses = {"MSE": mse, "bpp": bpp, "total_loss": total, "z_entropy": ce_z / npx, "y_entropy": ce_y / npx}
    return ({"x_tilde": x_tilde.detach(), "mu": mu.detach(), "sigma": sigma.detach()},
            {k: float(v.detach()) for k, v in losses.items()}, {k: p.grad for k, p in P.items()}, ctl,
            float(b.detach()[(~A).expand_as(b)].abs().max()))


@functools.lru_cache(maxsize=None)
def _oracle_of(shape, kind):
    """The oracle with its own ReLU masks, once per (input, kind): shared by the arithmetics."""
    from image_compression_amd import modelling
    torch.manual_seed(0)
    model = _set_context(modelling.build_model(_cfg(kind, "fp32", ARCH)))
    params = {k: v.clone() for k, v in model.state_dict().items()}
    return params, _oracle(params, *_train_inputs(shape), kind)


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("shape", TRAIN_SHAPES, ids=["2x128x128", "1x64x192"])
@pytest.mark.parametrize("kind", KINDS)
def test_training_step_matches_the_fp64_oracle(kind, shape, dtype):
    from image_compression_amd import injected_noise, modelling
    params, (o_out, o_loss, o_grad, ctl, b_max) = _oracle_of(shape, kind)
    assert 0.0 < b_max < 3.9, f"the oracle's largest |b| {b_max}: the clamp is in play"
    torch.manual_seed(0)
    model = _set_context(modelling.build_model(_cfg(kind, dtype, ARCH)))
    for k, v in model.state_dict().items():
        assert torch.equal(v, params[k]), k
    for conv in (model.context_mean, model.context_scale):
        assert torch.count_nonzero(conv.weight) == conv.weight.numel(), "a context tap is zero"
    model = model.to(DEV).train()
    x, uz, uy = _train_inputs(shape)
    rec = HipReluMasks(model)
    with _spy_context(model) as seen, injected_noise([uz.to(DEV), uy.to(DEV)]):
        x_tilde, losses = model(x.to(DEV))
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    rec.remove()
    if check_relu_ties(rec.masks, ctl):
        # a pre-activation on a tie took the other side: the oracle under the HIP path's masks (conftest)
        o_out, o_loss, o_grad, _, _ = _oracle(params, x, uz, uy, kind, masks=rec.masks)
    (sigma, mu), = seen
    got = {"x_tilde": x_tilde, "mu": mu, "sigma": sigma}
    for k in ("MSE", "bpp", "total_loss", "z_entropy", "y_entropy"):
        a, b = float(losses[k].detach()), o_loss[k]
        print(f"train {kind[:5]} {dtype} {shape} {k}: {a:.8g} oracle {b:.8g} rel {abs(a - b) / abs(b):.2e}")
        assert abs(a - b) < 1e-4 * abs(b), (k, a, b)
    for k, v in got.items():
        v = v.detach().cpu().numpy()
        print(f"train {kind[:5]} {dtype} {shape} {k}: rel_err {rel_err(v, o_out[k].numpy()):.2e}")
        assert rel_err(v, o_out[k].numpy()) < 1e-4, k
        assert_close(v, o_out[k].numpy(), 1e-4, k)
    worst = ("", 0.0)
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        e = rel_err(p.grad.cpu().numpy(), o_grad[k].numpy())
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < 1e-4, (k, e)
    print(f"train {kind[:5]} {dtype} {shape}: worst gradient {worst[0]} rel_err {worst[1]:.2e}; oracle max |b| {b_max:.3f}")
    same = _taps()
    for name in ("context_mean.weight", "context_scale.weight"):
        for g in (dict(model.named_parameters())[name].grad.cpu().numpy(), o_grad[name].numpy()):
            assert np.abs(g).max() > 0.0, name
            assert np.all(g[:, :, same] == 0), f"{name}: a tap between positions of one parity has a gradient"
            assert np.all(np.abs(g[:, :, ~same]).reshape(-1, 12).max(axis=0) > 0), f"{name}: a context tap has none"


# ---- a fresh model is the mean-scale model
@pytest.mark.parametrize("kind", KINDS)
def test_fresh_model_is_the_mean_scale_model(kind):
    from image_compression_amd import injected_noise, modelling
    torch.manual_seed(0)
    fresh = modelling.build_model(_cfg(kind, "fp32_split", ARCH)).to(DEV)
    torch.manual_seed(0)
    base = modelling.build_model(_cfg(kind, "fp32_split")).to(DEV)
    assert all(torch.count_nonzero(p) == 0 for c in (fresh.context_mean, fresh.context_scale) for p in c.parameters())
    shape = (2, 3, 128, 128)
    x, uz, uy = (t.to(DEV) for t in _train_inputs(shape))
    fresh.eval(), base.eval()
    (xa, la), (xb, lb) = fresh(x), base(x)
    assert set(la) == set(lb) and torch.equal(xa, xb)
    for k in lb:
        assert torch.equal(la[k], lb[k]), k
    fresh.train(), base.train()
    with injected_noise([uz, uy]):
        _, la = fresh(x)
    with injected_noise([uz, uy]):
        _, lb = base(x)
    for k in lb:
        a, b = float(la[k].detach()), float(lb[k].detach())
        print(f"fresh {kind[:5]} train {k}: {a:.9g} mean-scale {b:.9g} rel {abs(a - b) / abs(b):.2e}")
        assert abs(a - b) <= 1e-6 * abs(b), (k, a, b)


# ---- causality
@pytest.mark.parametrize("dtype", ["fp32_split", "bf16"])
def test_context_reads_the_anchors_only_and_within_its_window(dtype):
    model = _ckbd_model(KINDS[0], dtype)
    N, C, H, W = 2, 192, 12, 10
    g = torch.Generator().manual_seed(4)
    y_in = (torch.randn(N, C, H, W, generator=g) * 3).to(DEV)
    mu_h = torch.randn(N, C, H, W, generator=g).to(DEV)
    sigma_h = torch.randn(N, C, H, W, generator=g).exp().to(DEV)
    A = torch.from_numpy(_anchors(H, W)).to(DEV)
    with torch.no_grad():
        sigma, mu = model._context(y_in, sigma_h, mu_h)
        # every non-anchor replaced by unrelated values: nothing changes
        other = torch.where(A, y_in, (torch.randn(N, C, H, W, generator=g) * 100).to(DEV))
        assert not torch.equal(other, y_in)
        sigma2, mu2 = model._context(other, sigma_h, mu_h)
        assert torch.equal(sigma2, sigma) and torch.equal(mu2, mu)
        # at the anchors the hyperprior's own parameters, bit for bit
        assert torch.equal(mu[:, :, A], mu_h[:, :, A]) and torch.equal(sigma[:, :, A], sigma_h[:, :, A])
        assert not torch.equal(mu[:, :, ~A], mu_h[:, :, ~A]) and not torch.equal(sigma[:, :, ~A], sigma_h[:, :, ~A])
        # one anchor value changed: only non-anchors within its 5 x 5 window move
        n0, c0, i0, j0 = 1, 17, 6, 4
        assert bool(A[i0, j0])
        moved = y_in.clone()
        moved[n0, c0, i0, j0] += 8.0
        sigma3, mu3 = model._context(moved, sigma_h, mu_h)
    window = torch.zeros(N, H, W, dtype=torch.bool, device=DEV)
    window[n0, i0 - 2:i0 + 3, j0 - 2:j0 + 3] = True
    window &= ~A
    for name, new, old in (("mu", mu3, mu), ("sigma", sigma3, sigma)):
        changed = (new != old).any(dim=1)
        assert changed.any(), name
        assert not (changed & ~window).any(), f"{name} changed outside the window of the anchor"
    assert ((mu3 != mu).any(dim=1) == window).all(), "a non-anchor of the window did not see the anchor"


# ---- eval: the forward against the model's own bitstreams
R_MODEL = 16


@pytest.mark.parametrize("scaled", [False, True], ids=["seed", "x32"])
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=["2x128x128", "1x64x192"])
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_is_the_eval_forward_bitwise(kind, dtype, shape, scaled):
    from image_compression_amd import codec
    from image_compression_amd.modelling.blocks.entropy_model import _decode, ckbd_gather
    model = _ckbd_model(kind, dtype)
    cm = model.conditional_model
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    with _changed(model, scaled):
        x_fwd, losses = model(x)                       # no torch.no_grad(): the eval forward is inference only
        assert not x_fwd.requires_grad and not any(v.requires_grad for v in losses.values())
        data = model.compress(x, steps_per_chunk=R_MODEL)
        assert isinstance(data, bytes) and data[:4] == b"ICRC"
        assert model.compress(x, steps_per_chunk=R_MODEL) == data, "compressing twice gives different bytes"
        x_hat = model.decompress(data)
        h, lz, la, ln, pz, pa, pn = codec.parse_checkerboard(data, 4, dtype)
        y, z, z_hat, sigma_h, mu_h = _latents(model, x)
        with torch.no_grad():
            sigma, mu = model._eval_params(y, sigma_h, mu_h)
            rows = cm.scale_rows(sigma)
            tables = cm.tables(h.kmax_y, torch.device(DEV))
            half = h.nsym_y // 2
            sym_a = _decode(pa, la, half, ckbd_gather(cm.scale_rows(sigma_h), h.y_shape, 0), 0, tables, h.R, DEV)
            sym_n = _decode(pn, ln, half, ckbd_gather(rows, h.y_shape, 1), 0, tables, h.R, DEV)
        with _zero_context(model):
            x_zero = model.decompress(data)            # other rows for the non-anchors: other symbols, no error
    res = torch.round(y - mu)
    res_h = torch.round(y - mu_h)
    ideal = _ideal_bits(model, z_hat.movedim(1, -1).reshape(-1).cpu().numpy().astype(np.int64), h.kmax_z,
                        res.movedim(1, -1).reshape(-1).cpu().numpy().astype(np.int64), h.kmax_y,
                        rows.cpu().numpy().astype(np.int64).reshape(-1))
    assert h.kind == cm.KIND | 2 and h.kind in (2, 3) and h.R == R_MODEL
    assert (h.kmax_z, h.kmax_y) == (int(z_hat.abs().max()), int(res.abs().max()))
    if scaled:
        assert h.kmax_y > 16, h.kmax_y
    assert torch.equal(x_hat, x_fwd), "decompress(compress(x)) is not the eval forward's reconstruction"
    # the context is in the stream
    A = torch.from_numpy(_anchors(*y.shape[2:])).to(DEV)
    last = lambda t, m: t.movedim(1, -1)[:, m, :].reshape(-1)     # noqa: E731
    assert torch.equal(mu[:, :, A], mu_h[:, :, A])
    assert torch.equal(sym_a, last(res_h, A)), "the anchor half is not rint(y - mu_h) at the anchors"
    assert torch.equal(sym_n, last(res, ~A)), "the non-anchor half is not rint(y - mu) at the non-anchors"
    differ = int((sym_n != last(res_h, ~A)).sum())
    assert differ > 0, "the non-anchors are coded as the mean-scale model would code them"
    assert x_zero.shape == x_hat.shape and not torch.equal(x_zero, x_hat)
    # the rate, by the existing bounds (tests/test_codec_gpu.py), over the three streams
    assert len(la) == len(ln) == codec.num_chunks(half, h.R) >= 2
    chunks = len(lz) + len(la) + len(ln)
    coded = 8 * len(data) - 8 * codec.checkerboard_fixed_bytes(h)
    print(f"round trip {kind[:5]} {dtype} {shape} {'x32' if scaled else 'seed'}: kmax_z {h.kmax_z} kmax_y {h.kmax_y} "
          f"bytes {len(data)} ideal bits {ideal:.1f} coded - ideal {coded - ideal:+.1f} over {chunks} chunks; "
          f"{differ} of {half} non-anchor symbols differ from the mean-scale model's")
    assert ideal - 16 * 64 * chunks - 1 <= coded <= ideal * 1.001 + 8 * chunks, (coded, ideal, chunks)


def test_evaluator_codes_through_compress():
    from image_compression_amd.evaluation import Evaluator
    model = _ckbd_model(KINDS[0], "fp32_split")
    batches = [torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(11)).to(DEV)]
    plain = Evaluator(model).run_eval(batches)
    coded = Evaluator(model, coded=True).run_eval(batches)
    assert set(coded) == set(plain) | {"coded_bpp"}
    for k in plain:
        assert coded[k] == plain[k], k
    assert coded["coded_bpp"] == pytest.approx(8.0 * len(model.compress(batches[0])) / (256 * 256), rel=1e-12)


# ---- refusals
def test_the_models_refuse_each_others_streams_before_any_launch():
    ckbd, mean = _ckbd_model(KINDS[0], "fp32_split"), _model(KINDS[0], "fp32_split")
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    icrc, icra = ckbd.compress(x), mean.compress(x)
    assert (icrc[:4], icra[:4], icra[7]) == (b"ICRC", b"ICRA", 2)

    def no_prior(z_hat):
        raise AssertionError("_prior was called: something was launched before the stream was refused")

    for model, data in ((mean, icrc), (ckbd, icra)):
        model._prior = no_prior
        try:
            with pytest.raises(ValueError, match="magic"):
                model.decompress(data)
        finally:
            del model._prior
    # Laplace / Gauss still tell each other apart
    with pytest.raises(ValueError, match="different model"):
        _ckbd_model(KINDS[1], "fp32_split").decompress(icrc)
    with pytest.raises(NotImplementedError, match="CheckerboardCompressor2018"):
        ckbd.compress_each(x)
    with pytest.raises(NotImplementedError, match="CheckerboardCompressor2018"):
        ckbd.decompress_each([icrc])
    assert torch.equal(ckbd.decompress(icrc), ckbd(x)[0])
