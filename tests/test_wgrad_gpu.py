"""The weight-gradient kernels (csrc/wgrad.hip, the edge and column-buffer detours of csrc/conv_api.hip) one
op at a time: torch.ops.imgcomp.conv2d_wgrad / conv_transpose2d_wgrad with bias, on every case of
wgrad_cases.CASES (test_wgrad_plans.py holds, without a GPU, which kernel each launches), against torch's own
convolution autograd in float64.

Per case and math mode: dw and db at the fp32 bar; split arithmetic within 1.5x of the native
fp32 kernel's own error and bitwise different from it where a split kernel runs; bf16 operands by the two-sided
rule of test_bf16_gpu.test_wgrad_bf16 (fp32-class against fp64 of the rounded operands, bf16-class against exact
fp64); a mode that cannot take bf16 bitwise the mode it falls to; the same call twice bitwise equal (fixed-order
reduction); a NaN-filled block of the workspace's size allocated and freed before every call, so that a slab
element nobody wrote most likely reads NaN; and the operands once more as interiors of NaN-filled tensors,
bitwise the compact result and free of NaN.  The measured errors are printed (DESIGN.md 1b holds them)."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as W
from conftest import assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [c.name for c in W.CASES]


def _nan_block(nbytes):
    """Allocate and free a block of NaN (all bits set) of the workspace's size: the op's own workspace, allocated
    next, most likely lands on it.  Nothing here depends on that."""
    t = torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    del t


def _wgrad(c, x, dy, math, copies=None):
    from image_compression_amd import _lib
    L, ops = _lib.load(), _lib.ops()
    query = L.ic_conv_transpose2d_wgrad_ws_ex if c.tr else L.ic_conv2d_wgrad_ws_ex
    _nan_block(query(_lib.act(x), _lib.act(dy), c.k, c.s, c.p, math))
    w = torch.empty(W.weight_shape(c), device=DEV)   # read for its shape only
    if copies is not None:
        op = ops.conv_transpose2d_wgrad_xb if c.tr else ops.conv2d_wgrad_xb
        dw, db = op(x, copies[0], dy, copies[1], w, c.s, c.p, True, math)
    else:
        op = ops.conv_transpose2d_wgrad if c.tr else ops.conv2d_wgrad
        dw, db = op(x, dy, w, c.s, c.p, True, math)
    assert dw.shape == w.shape and db.shape == (c.cout,)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), (c.name, math, "NaN / inf in the result")
    return dw, db


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _split_rule(c, math, got, native, ref, ran):
    """test_split_gpu._check on dw: the fp32 bar, and no worse than 1.5x the native fp32 kernel; db at the fp32 bar."""
    assert_close(got[0].cpu(), ref[0], 1e-4, f"{c.name} math {math} dw")
    assert_close(got[1].cpu(), ref[1], 1e-4, f"{c.name} math {math} db")
    es, en = rel_err(got[0].cpu(), ref[0]), rel_err(native[0].cpu(), ref[0])
    print(f"WGRAD {c.name} math {math} {c.kern[math]} dw: split {es:.2e} native fp32 {en:.2e}; "
          f"db {rel_err(got[1].cpu(), ref[1]):.2e}")
    assert es <= 1.5 * en + 1e-8, (c.name, math, es, en)
    if ran:
        assert not torch.equal(got[0], native[0]), (c.name, math, "the split kernel did not run")


def _bf16_rule(c, math, got, x, dy, ref):
    """test_bf16_gpu.test_wgrad_bf16's two sides.  e_ref: the native fp32 kernel on the same pre-rounded operands,
    against the same fp64 result; db is summed from the unrounded dy: the fp32 bar."""
    xr, dyr = W.round_bf16(x), W.round_bf16(dy)
    assert xr.stride() == x.stride() and dyr.stride() == dy.stride()
    ref_r = [t.cpu() for t in W.reference(c, xr, dyr)]
    e_ref = rel_err(_wgrad(c, xr, dyr, 0)[0].cpu(), ref_r[0])
    e_em, e = rel_err(got[0].cpu(), ref_r[0]), rel_err(got[0].cpu(), ref[0])
    print(f"WGRAD {c.name} math {math} {c.kern[math]} dw: vs fp64 of the bf16 operands {e_em:.2e} "
          f"(fp32 kernel on them {e_ref:.2e}), vs fp64 {e:.2e}")
    assert e_em <= max(1e-5, 2 * e_ref), (c.name, math, e_em, e_ref)
    assert 1e-5 < e < 1e-2, (c.name, math, e)
    assert_close(got[1].cpu(), ref[1], 1e-4, f"{c.name} math {math} db")


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_wgrad_parity(case):
    c = case
    x, dy = W.make_operands(c, "compact", DEV)
    ref = [t.cpu() for t in W.reference(c, x, dy)]
    out = {}
    for m in W.MATHS:
        assert W.plan_of(c, x, dy, m) == W.expected_plan(c, m), (c.name, m)
        out[m] = _wgrad(c, x, dy, m)
        assert _same(_wgrad(c, x, dy, m), out[m]), (c.name, m, "two runs differ")
    # fp32
    for name, g, r in (("dw", out[0][0], ref[0]), ("db", out[0][1], ref[1])):
        assert_close(g.cpu(), r, 1e-4, f"{c.name} math 0 {name}")
        print(f"WGRAD {c.name} math 0 {c.kern[0]} {name}: native fp32 {rel_err(g.cpu(), r):.2e}")
    # split arithmetic: a split kernel (the edge kernel's split form too), else the fp32 launch itself
    split_ran = c.kern[2] == W.SP or W.is_edge(c)
    _split_rule(c, 2, out[2], out[0], ref, split_ran)
    if not split_ran:
        assert _same(out[2], out[0]), (c.name, "math 2 is not the fp32 launch")
    # bf16 operands, or the launch of the mode without them
    for m, base in ((1, 0), (3, 2)):
        if c.kern[m] in (W.BF, W.EB):
            _bf16_rule(c, m, out[m], x, dy, ref)
        else:
            assert _same(out[m], out[base]), (c.name, f"math {m} is not the math {base} launch")
    # the operands as interiors of NaN-filled tensors: the same plan (test_wgrad_plans.py), the same values in the
    # same order.  db is summed by the kernel that takes dy's layout, so it is bitwise only where dy stays compact.
    for view in c.views:
        xv, dyv = W.make_operands(c, view, DEV)
        assert torch.equal(xv, x) and torch.equal(dyv, dy)
        for m in W.MATHS:
            assert W.plan_of(c, xv, dyv, m) == W.expected_plan(c, m), (c.name, view, m)
            dw, db = _wgrad(c, xv, dyv, m)
            assert torch.equal(dw, out[m][0]), (c.name, view, m, "dw differs from the compact run")
            if view == "x":
                assert torch.equal(db, out[m][1]), (c.name, view, m, "db differs from the compact run")
            else:
                assert_close(db.cpu(), ref[1], 1e-4, f"{c.name} {view} math {m} db")


def test_wgrad_bf16_copies_bitwise():
    """conv2d_wgrad_xb on the tap-group kernel reads the operands' bf16 copies: the same round-to-nearest values
    the kernel forms itself, so the result is bitwise the math-1 result without them."""
    c = W.BY_NAME["x3p_32x32"]
    x, dy = W.make_operands(c, "compact", DEV)
    plain = _wgrad(c, x, dy, 1)
    xb, dyb = x.to(torch.bfloat16), dy.to(torch.bfloat16)
    assert xb.stride() == x.stride() and dyb.stride() == dy.stride()
    assert _same(_wgrad(c, x, dy, 1, copies=(xb, dyb)), plain)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("C,n,h,w,fmt", W.GDN_CASES)
def test_gdn_gemm_dgamma_dbeta(C, n, h, w, fmt, inverse):
    """The GDN backward off the fused kernels' layouts: dgamma = q^T x^2 on the weight-gradient kernels with x
    squared in the operand load (AOP_SQUARE), dbeta the column sums of q, against oracle.ref_cpu.gdn in fp64.
    The oracle differentiates the raw parameters p (gamma = p^2 - pedestal above the bound), so the op's
    gradients of gamma and beta are taken to p's by the exact factor 2 p."""
    from image_compression_amd import _lib
    from oracle import ref_cpu
    g = torch.Generator().manual_seed(7 * C + h)
    x, dy = torch.randn(n, C, h, w, generator=g), torch.randn(n, C, h, w, generator=g)
    gamma = (torch.eye(C) * 0.1 + torch.rand(C, C, generator=g) * 0.05).view(C, C, 1, 1)
    beta = 1.0 + torch.rand(C, generator=g) * 0.1
    ped = float(2.0 ** -18) ** 2
    gp = torch.sqrt(gamma.double() + ped).requires_grad_(True)
    bp = torch.sqrt(beta.double() + ped).requires_grad_(True)
    ref_cpu.gdn(x.double(), gp, bp, inverse=inverse).backward(dy.double())
    norm = F.conv2d(x.double() ** 2, gamma.double(), beta.double()).float()

    def put(t):
        t = t.to(DEV)
        return t.contiguous(memory_format=torch.channels_last) if fmt == "cl" else t.contiguous()

    xd, dyd, nd = put(x), put(dy), put(norm)
    assert _lib.plan("gdn_bwd", xd)["kernel"] == "gdn_gemm"
    runs = []
    for _ in range(2):
        _nan_block(_lib.load().ic_gdn_bwd_ws(_lib.act(xd)))
        _, dg, db = _lib.ops().gdn_bwd(xd, nd, dyd, gamma.to(DEV), inverse, 0)
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())
        runs.append((dg, db))
    assert _same(runs[0], runs[1]), "two runs differ"
    dgp = runs[0][0].cpu().double() * 2 * gp.detach()
    dbp = runs[0][1].cpu().double() * 2 * bp.detach()
    print(f"WGRAD gdn C={C} {n}x{h}x{w} {fmt} inverse={inverse} nsplit {W.gdn_nsplit(C, n, h, w, fmt)}: "
          f"dgamma {rel_err(dgp, gp.grad):.2e} dbeta {rel_err(dbp, bp.grad):.2e}")
    assert_close(dgp, gp.grad, 1e-4, "dgamma")
    assert_close(dbp, bp.grad, 1e-4, "dbeta")
