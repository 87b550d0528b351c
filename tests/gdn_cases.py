"""The GDN / IGDN case table shared by test_gdn_plans.py (CPU: which kernel each case launches, from the
library's plan query) and test_gdn_gpu.py (parity of y, norm, dx, dgamma, dbeta and dx's column sums against
float64).

csrc/gdn.hip sends a GDN to the fused kernels of csrc/gdn_fused.hip when C is 64, 128 or 192 and x is NHWC-dense
(channel stride 1, pixel stride C over every dimension above size 1) on a 16-byte aligned base, and to the
implicit GEMM otherwise; the math mode (1: bf16 operands, 2: split arithmetic, 3: both) picks among the fused
kernels.  The plan query names a kernel family; which template instantiation a call launches, how many tiles a
block of the persistent kernels runs and where the GEMM path takes split arithmetic are restated here once
(expected_plan, instantiation, tiling, split_gemm), and the plan test holds the first against the library and the
others against the numbers the table's comments quote.

A case is (name, C, (n, h, w), layout): `cl` channels-last; `nchw`; `cl_off4` NHWC in a flat buffer whose base is
advanced by one float (dense, not 16-byte aligned)."""
import collections
import functools

import torch

CL = torch.channels_last
MATHS = (0, 1, 2, 3)
BF16, SPLIT = 1, 2          # IC_MATH_BF16, IC_MATH_SPLIT
DIRS = ("fwd", "bwd")
FUSED, FSPLIT, FBF16, GEMM = "gdn_fused", "gdn_fused_split", "gdn_fused_bf16", "gdn_gemm"
KERNEL_NAMES = {FUSED, FSPLIT, FBF16, GEMM}

Case = collections.namedtuple("Case", "name C shape layout note")

# pixel sets of the fused kernels.  Tile rows: fused forward 16 (grid <= 512), x3s forward 32 (grid <= 256), both
# backwards 16 (grid <= 256)
PIXELS = [
    ((1, 1, 1), "one row of one tile; every stride belongs to a dimension of size 1"),
    ((1, 3, 5), "15: a 16-row tile one row short"),
    ((1, 4, 4), "16: one whole 16-row tile"),
    ((1, 1, 17), "17: one row into the second tile"),
    ((1, 1, 31), "31: a 32-row tile one row short"),
    ((1, 3, 11), "33: one row into the second 32-row tile"),
    ((3, 7, 5), "105: the ragged case of the older tests"),
    ((1, 65, 65), "4225: backward 265 tiles on 256 blocks (blocks 0-8 run two, the last tile has one row)"),
    ((3, 75, 73), "16425: fp32 forward 1027 tiles (2-3 per block), backward 4-5, x3s 514 (2-3); last tile 9 rows"),
    ((4, 79, 78), "24648: x3s forward 771 tiles, 3-4 per block: the three x buffers and both plane sets wrap"),
]


def pixels(shape):
    return shape[0] * shape[1] * shape[2]


def _fused_cases():
    out = []
    for C in (192, 64, 128):
        for shape, note in PIXELS:
            if pixels(shape) == 24648 and C != 192:
                continue
            out.append(Case(f"c{C}_p{pixels(shape)}", C, shape, "cl", note))
    # a batch of 1 x 1 maps: strides (C, 1, 1, 1) as channels-last; planned gdn_gemm before the stride of a
    # dimension of size 1 stopped counting (csrc/gdn_fused.hip gdn_fused_ok)
    out.append(Case("c192_n2_1x1", 192, (2, 1, 1), "cl", "two pixels in the batch dimension alone"))
    out.append(Case("c64_n2_1x1", 64, (2, 1, 1), "cl", "two pixels in the batch dimension alone"))
    return out


CASES = _fused_cases() + [
    Case("c3_nchw", 3, (2, 9, 7), "nchw", "GEMM path, gather form through the channel stride"),
    Case("c10_cl", 10, (2, 9, 7), "cl", "GEMM path, gather form, C % 4 != 0"),
    Case("c48_cl", 48, (2, 9, 7), "cl", "C % 32 != 0, padded K"),
    Case("c96_cl", 96, (2, 33, 33), "cl", "fast form; math 2 takes the split GEMM forward"),
    Case("c320_cl", 320, (2, 8, 8), "cl", "second column tile partial"),
    Case("c192_nchw", 192, (1, 9, 16), "nchw", "C = 192 off the fused kernels' layout"),
    Case("c192_off4", 192, (3, 7, 5), "cl_off4", "the fused kernels' aligned base"),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------ the dispatch, restated
def fused_ok(c):
    return c.C in (64, 128, 192) and c.layout == "cl"


def _fsplit(c, math):
    """gdn_fwd_impl's `split`: split arithmetic is asked for and the forward has a form of it"""
    return bool(math & SPLIT) and c.C % 32 == 0 and c.layout != "nchw" and c.C >= 64


def expected_plan(c, direction, math):
    """gdn_plan (csrc/gdn.hip) as a kernel name."""
    if direction == "fwd":
        fs = _fsplit(c, math)
        if (not fs or c.C == 192) and fused_ok(c):
            return FBF16 if fs and math & BF16 else FSPLIT if fs else FUSED
        return GEMM
    if fused_ok(c):
        return FBF16 if math & BF16 and c.C == 192 else FSPLIT if math & SPLIT and c.C == 192 else FUSED
    return GEMM


def split_gemm(c, math):
    """The GEMM forward in split arithmetic (ig_kernel_x3s with the squared load): the fast form only, so a
    channels-last x on an aligned base with strides that are multiples of 4; the backward's GEMMs take no math."""
    s = make(c, torch.empty(c.shape[0], c.C, *c.shape[1:])).stride()
    return expected_plan(c, "fwd", math) == GEMM and _fsplit(c, math) and c.layout == "cl" and \
        s[0] % 4 == 0 and s[2] % 4 == 0 and s[3] % 4 == 0


def falls_to(c, direction, math):
    """The math mode whose launch `math` repeats bit for bit, or None where `math` is a launch of its own."""
    if math == 0:
        return None
    k = expected_plan(c, direction, math)
    if direction == "fwd":
        if math == 1:
            return 0                                   # the forward takes bf16 operands only with split set
        if math == 2:
            # (the GEMM forward in fp32, where x is off the fast form: a launch of its own, not a split one)
            return None if k == FSPLIT or split_gemm(c, 2) or k != expected_plan(c, direction, 0) else 0
        return None if k == FBF16 else 2               # math 3 off the bf16 kernel: math 2's launch
    if k == FBF16:
        return None if math == 1 else 1                # one kernel; the test gives math 3 the bf16 forward's norm
    if k == FSPLIT:
        return None
    return 0


# launched instantiations (gdn_fwd_fused / gdn_bwd_fused, csrc/gdn_fused.hip).  gdn_bwd_x3w_kernel<192, INV, 1> and
# <192, INV, 1, true> (the bf16 and XB forms of the pipelined split backward) and gdn_bwd_fused_kernel<192, true>
# (split dgamma on the two-group kernel) are compiled but never launched by the dispatcher: outside the table.
INSTANTIATIONS = (
    "gdn_fwd_fused_kernel<64>", "gdn_fwd_fused_kernel<128>", "gdn_fwd_fused_kernel<192>",
    "gdn_fwd_x3s_kernel<192, 3>", "gdn_fwd_x3s_kernel<192, 1>", "gdn_fwd_x3s_kernel<192, 1, true>",
    "gdn_fwd_x3s_kernel<192, 1, false, false>", "gdn_fwd_x3s_kernel<192, 1, true, false>",
    "gdn_bwd_fused_kernel<64>", "gdn_bwd_fused_kernel<128>", "gdn_bwd_fused_kernel<192>",
    "gdn_bwd_fused_kernel<192, true, true>", "gdn_bwd_fused_kernel<192, true, true, true>",
    "gdn_bwd_fused_kernel<192, true, true, false, true>", "gdn_bwd_fused_kernel<192, true, true, true, true>",
    "gdn_bwd_x3w_kernel<192, false>", "gdn_bwd_x3w_kernel<192, true>",
    "gdn_slab_reduce_kernel",
)
# the variants of test_gdn_gpu.py: (op, copy): the plain ops, the ops with a bf16 copy, the norm-free pair
VARIANTS = (("plain", False), ("xb", True), ("rn", False), ("rn", True))


def instantiation(c, direction, math, inverse=False, variant=("plain", False)):
    """The fused kernel a call launches (None on the GEMM path; the copy of an `xb` op off the bf16 kernel is
    ig_cvt_bf16's, after the plain kernel)."""
    k = expected_plan(c, direction, math)
    op, copy = variant
    if k == GEMM or (op == "rn" and k != FBF16):
        return None
    if direction == "fwd":
        if k == FUSED:
            return f"gdn_fwd_fused_kernel<{c.C}>"
        if k == FSPLIT:
            return "gdn_fwd_x3s_kernel<192, 3>"
        yb = "true" if copy else "false"
        if op == "rn":
            return f"gdn_fwd_x3s_kernel<192, 1, {yb}, false>"
        return "gdn_fwd_x3s_kernel<192, 1, true>" if copy else "gdn_fwd_x3s_kernel<192, 1>"
    if k == FUSED:
        return f"gdn_bwd_fused_kernel<{c.C}>"
    if k == FSPLIT:
        return "gdn_bwd_x3w_kernel<192, %s>" % ("true" if inverse else "false")
    if op == "rn":
        return "gdn_bwd_fused_kernel<192, true, true, %s, true>" % ("true" if copy else "false")
    return "gdn_bwd_fused_kernel<192, true, true, true>" if copy else "gdn_bwd_fused_kernel<192, true, true>"


Tiling = collections.namedtuple("Tiling", "rows grid tiles per_block last_rows")


def tiling(c, direction, math):
    """Tile rows, grid, tile count, (fewest, most) tiles a block runs and the last tile's rows of the persistent
    fused kernel; None on the GEMM path."""
    k = expected_plan(c, direction, math)
    if k == GEMM:
        return None
    rows, cap = (32, 256) if direction == "fwd" and k != FUSED else (16, 512 if direction == "fwd" else 256)
    P = pixels(c.shape)
    tiles = -(-P // rows)
    grid = min(tiles, cap)
    return Tiling(rows, grid, tiles, (tiles // grid, -(-tiles // grid)), P - (tiles - 1) * rows)


# ------------------------------------------------------------------ operands
def make(c, t, device=None):
    """t (logical N, C, H, W, contiguous) in the case's layout."""
    t = t if device is None else t.to(device)
    if c.layout == "nchw":
        return t.contiguous()
    if c.layout == "cl":
        return t.contiguous(memory_format=CL)
    n, ch, h, w = t.shape
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(n, h, w, ch)
    v.copy_(t.permute(0, 2, 3, 1))
    return v.permute(0, 3, 1, 2)


def plan_of(direction, x, math):
    from image_compression_amd import _lib
    return _lib.plan("gdn_" + direction, x, math=math)["kernel"]


@functools.lru_cache(maxsize=None)
def values(name):
    """x, dy ~ N(0, 1); gamma = 0.1 I + 0.05 U(0, 1); beta = 1 + 0.1 U(0, 1), so norm >= 1; a seed per case."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + IDS.index(name))
    n, h, w = c.shape
    x = torch.randn(n, c.C, h, w, generator=g)
    dy = torch.randn(n, c.C, h, w, generator=g)
    gamma = 0.1 * torch.eye(c.C) + 0.05 * torch.rand(c.C, c.C, generator=g)
    beta = 1.0 + 0.1 * torch.rand(c.C, generator=g)
    return {"x": x, "dy": dy, "gamma": gamma.reshape(c.C, c.C, 1, 1), "beta": beta}


# ------------------------------------------------------------------ references (float64, CPU)
def _rows(t):
    """(N, C, H, W) -> [pixel][C]: the 1 x 1 convolution is a matrix product over the rows"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _maps(m, like):
    n, ch, h, w = like.shape
    return m.reshape(n, h, w, ch).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=4)
def reference(name, inverse):
    """norm = conv2d(x^2, gamma, beta), y = x norm^-1/2 (IGDN: x norm^1/2), and dx, dgamma, dbeta by autograd of
    sum(y dy), all in float64 from the re-parameterised gamma and beta the op takes; dxsum = dx.sum((0, 2, 3))."""
    v = values(name)
    x = _rows(v["x"]).double().requires_grad_(True)
    g = v["gamma"].reshape(v["beta"].numel(), -1).double().requires_grad_(True)
    b = v["beta"].double().requires_grad_(True)
    norm = (x * x) @ g.t() + b
    y = x * norm.sqrt() if inverse else x / norm.sqrt()
    y.backward(_rows(v["dy"]).double())
    like = v["x"]
    dx = _maps(x.grad, like)
    return {"y": _maps(y.detach(), like), "norm": _maps(norm.detach(), like), "dx": dx, "dgamma": g.grad.reshape(v["gamma"].shape),
            "dbeta": b.grad, "dxsum": dx.sum((0, 2, 3))}


def rnd(t):
    """to bf16 (round to nearest even) and back to float64: what a bf16-operand MFMA sees of t"""
    return t.to(torch.bfloat16).double()


def emulate(name, inverse, fwd_bf16, bwd_bf16, fp32_q=False):
    """The fused bf16 kernels' arithmetic in float64, GDN and IGDN: the forward (gdn_fwd_x3s_kernel<192, 1>)
    contracts bf16(gamma) with bf16 of the fp32 square of x; the backward (gdn_bwd_phase_a<..., BF>, group A)
    contracts bf16(q) with bf16(x^2) for dgamma and bf16(q) with bf16(gamma) for dx; dbeta sums the unrounded q.
    fp32_q: q, the direct term and the norm they come from formed in fp32 as the kernel forms them (rsq, then
    products) instead of float64: the emulation's own spread (q rounds to a neighbouring bf16 on either side)."""
    v = values(name)
    x32, dy32 = _rows(v["x"]), _rows(v["dy"])
    g32 = v["gamma"].reshape(v["beta"].numel(), -1)
    x, dy, g, b = x32.double(), dy32.double(), g32.double(), v["beta"].double()
    x2r = rnd(x32 * x32)                                            # the fp32 square, rounded
    norm = x2r @ rnd(g32).t() + b if fwd_bf16 else (x * x) @ g.t() + b
    y = x * norm.sqrt() if inverse else x / norm.sqrt()
    if fp32_q:
        n32 = norm.float()
        rs = n32.rsqrt()
        q = (0.5 * dy32 * x32 * rs) if inverse else (-0.5 * dy32 * x32 * (rs * rs * rs))
        direct = dy32 * (n32 * rs) if inverse else dy32 * rs
        qr = rnd(q) if bwd_bf16 else q.double()
        q, direct = q.double(), direct.double()
    else:
        q = 0.5 * dy * x / norm.sqrt() if inverse else -0.5 * dy * x * norm.pow(-1.5)
        direct = dy * norm.sqrt() if inverse else dy / norm.sqrt()
        qr = rnd(q) if bwd_bf16 else q
    dx = direct + 2.0 * x * (qr @ (rnd(g32) if bwd_bf16 else g))     # sum_n q[m][n] gamma[n][k]
    dgamma = qr.t() @ (x2r if bwd_bf16 else x * x)
    like = v["x"]
    dx = _maps(dx, like)
    return {"y": _maps(y, like), "norm": _maps(norm, like), "dx": dx, "dgamma": dgamma.reshape(v["gamma"].shape),
            "dbeta": q.sum(0), "dxsum": dx.sum((0, 2, 3))}


# The emulation side of the bf16 rule.  1e-4 is the bound the project measured for the forward GDN
# (tests/test_bf16_gpu.py).  For both GDN and IGDN the emulation's own spread between q formed in float64 and in
# fp32 (emulate(fp32_q=True); q lands on the other side of a bf16 rounding boundary for a few elements in 1e5),
# measured on the CPU at the 105- and 16425-pixel cases of C = 192, is below 4e-5 for dx and dgamma
# in both directions: 1e-4 sits above it, so it is the bound for IGDN too.
EMUL_BOUND = 1e-4
