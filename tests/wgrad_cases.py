"""The weight-gradient case table shared by test_wgrad_plans.py (CPU: which kernel each case
launches, from the library's plan query) and test_wgrad_gpu.py (parity of dw / db against fp64).

csrc/wgrad.hip chooses among its kernels by channel counts, the width of the gradient map, the
pixel count P, the pixel split pps that wg_plan derives from P, pointer alignment and layout;
csrc/conv_api.hip adds the image-edge kernels (csrc/edge.hip) and the column-buffer detour for an
X of a few channels.  The plan query names a kernel family only, so the two rules that pick the
kernel inside a family are restated here once (restate_nsplit, split_sub): the plan test holds
them against the library's own nsplit for every case, and so keeps the kernel a case names in
its comment the one that runs.

In the GEMM, G is the operand whose channels are the rows of dw and whose pixel grid is summed
over: dy for a convolution, x for a transposed one; X is the other."""
import collections

import torch
import torch.nn.functional as F

CL = torch.channels_last

LD, SP, BF, FP, GA, ED, EB = ("wg_ldsdma", "wg_split", "wg_bf16", "wg_fp32", "wg_fp32_gather", "edge_wgrad",
                              "edge_wgrad_bf16")
# the kernel at math 0 (fp32), 1 (bf16 operands), 2 (split arithmetic), 3 (bf16, else split)
WIDE_BF = (LD, BF, SP, BF)    # a split kernel that has a bf16 form: x3p, x3d, x3d16
WIDE_SP = (LD, LD, SP, SP)    # a split kernel without one: x3rf, x3g
NARROW = (LD, LD, LD, LD)     # fewer than 128 channels on a side, or the column buffer: fp32 in every mode
EDGE = (ED, EB, ED, EB)

MATHS = (0, 1, 2, 3)
SUBS = ("x3p", "x3d", "x3d16", "x3rf", "x3g")   # wg_x3p_kernel, wg_x3d_kernel<SEG16 = false / true>,
BF16_SUBS = ("x3p", "x3d", "x3d16")             # wg_x3_kernel<ROWFAST = true / false>

Case = collections.namedtuple(
    "Case", "name tr n cin h w cout k s p op kern bn sub im2col ns xfmt dyfmt views chan")


def _case(name, tr, n, cin, h, w, cout, k, s, p, op=0, *, kern, bn, ns, sub=None, im2col=0, xfmt=None, dyfmt=None,
          views=("x", "both"), chan=False):
    """kern: the planned kernel at math 0..3; bn: the column tile (edge kernels: restated, None); ns: nsplit of the
    fp32 plan and of the math-2 plan; sub: the split kernel behind wg_split (math 2), also the bf16 form where
    kern[1] is wg_bf16; views: which operands the NaN-haloed runs take as interiors of larger tensors; chan: x is
    channels [1 : C + 1] of a channels-last tensor of C + 8 channels (rows 16-byte aligned, base pointer off by 4)."""
    xfmt = xfmt or ("nchw" if cin <= 8 else "cl")
    dyfmt = dyfmt or ("nchw" if cout <= 4 else "cl")
    return Case(name, tr, n, cin, h, w, cout, k, s, p, op, kern, bn, sub, im2col, ns, xfmt, dyfmt, views, chan)


def _conv(name, *a, **kw):
    return _case(name, False, *a, **kw)


def _tconv(name, *a, **kw):
    return _case(name, True, *a, **kw)


# n, cin, h, w, cout, k, stride, pad[, output padding]
CASES = [
    # ---- the split kernels (math 2) and their bf16 forms (math 1): >= 128 channels on both sides
    _conv("x3p_32x32", 2, 192, 64, 64, 192, 5, 2, 2, kern=WIDE_BF, bn=192, sub="x3p", ns=(16, 10)),   # last split: 32 pixels
    _conv("x3p_17x32", 3, 192, 34, 64, 192, 5, 2, 2, kern=WIDE_BF, bn=192, sub="x3p", ns=(17, 9)),    # odd rows, splits cross images
    _conv("x3p_odd_input", 1, 192, 31, 63, 192, 5, 2, 2, kern=WIDE_BF, bn=192, sub="x3p", ns=(8, 8)),  # bottom / right taps out of range
    _conv("x3d_cg320", 2, 192, 16, 32, 320, 3, 1, 1, kern=WIDE_BF, bn=192, sub="x3d", ns=(16, 11)),   # second row tile: 128 of 192
    _conv("x3d_cx320", 2, 320, 16, 32, 192, 3, 1, 1, kern=WIDE_BF, bn=192, sub="x3d", ns=(16, 11)),   # second column tile partial
    _conv("x3d_two_level", 4, 192, 32, 32, 192, 3, 1, 1, kern=WIDE_BF, bn=192, sub="x3d", ns=(43, 26)),  # fp32: G = 2, row-fast
    _conv("x3d_w64_midrow", 2, 192, 16, 64, 192, 3, 1, 1, kern=WIDE_BF, bn=192, sub="x3d", ns=(32, 22)),  # pps 96: mid-row splits
    _conv("x3d16_s2", 2, 192, 30, 32, 192, 5, 2, 2, kern=WIDE_BF, bn=192, sub="x3d16", ns=(8, 8)),    # a step spans two images
    _conv("x3d16_s1", 2, 192, 15, 16, 192, 3, 1, 1, kern=WIDE_BF, bn=192, sub="x3d16", ns=(8, 8)),
    _conv("x3d16_w48", 1, 128, 6, 48, 320, 3, 1, 1, kern=WIDE_BF, bn=192, sub="x3d16", ns=(5, 5)),    # Cx 128, Cg 320
    _conv("x3rf_half_step", 1, 192, 30, 32, 192, 5, 2, 2, kern=WIDE_SP, bn=192, sub="x3rf", ns=(4, 4)),  # P % 32 == 16
    _conv("x3rf_w48", 1, 192, 10, 96, 192, 5, 2, 2, kern=WIDE_SP, bn=192, sub="x3rf", ns=(4, 4)),
    _conv("x3g_4x17", 1, 192, 7, 33, 192, 5, 2, 2, kern=WIDE_SP, bn=192, sub="x3g", ns=(2, 2)),       # last split: 4 pixels
    _conv("x3g_two_level", 4, 192, 30, 30, 192, 3, 1, 1, kern=WIDE_SP, bn=192, sub="x3g", ns=(38, 23)),  # fp32: G = 2, gather
    _conv("x3g_200_136", 2, 200, 8, 8, 136, 3, 1, 1, kern=WIDE_SP, bn=192, sub="x3g", ns=(2, 2)),     # no channel count % 64 == 0
    _conv("k1_two_groups", 1, 192, 64, 64, 192, 1, 1, 0, kern=WIDE_BF, bn=192, sub="x3d", ns=(64, 64)),  # G = 2, two full groups
    _conv("k1_ragged_group", 1, 192, 47, 45, 192, 1, 1, 0, kern=WIDE_SP, bn=192, sub="x3g", ns=(34, 34)),  # second group: 2 splits
    # ---- the LDS-DMA kernel's 192 x 64 tile (Cx < 128): fp32 in every mode
    _conv("ld64_rowfast", 2, 64, 9, 16, 192, 3, 1, 1, kern=NARROW, bn=64, ns=(5, 5)),
    _conv("ld64_cg64", 2, 96, 18, 10, 64, 5, 2, 2, kern=NARROW, bn=64, ns=(2, 2)),                    # last split: 26 pixels
    # ---- operands the LDS-DMA kernel cannot take
    _conv("gather_cx10", 1, 10, 9, 7, 64, 3, 1, 1, kern=(GA,) * 4, bn=64, ns=(1, 1)),                 # Cx % 4 != 0
    _conv("gather_nchw16", 2, 16, 9, 11, 64, 3, 1, 1, kern=(GA,) * 4, bn=64, ns=(4, 4), xfmt="nchw"),  # xs_c != 1
    _conv("fp32_cout6", 1, 64, 9, 16, 6, 3, 1, 1, kern=(FP,) * 4, bn=64, ns=(3, 3)),                  # scalar G loads
    _conv("fp32_chan192", 2, 192, 9, 16, 192, 3, 1, 1, kern=(FP,) * 4, bn=192, ns=(5, 5), chan=True, views=("dy",)),
    _conv("fp32_chan64", 1, 64, 7, 9, 136, 3, 1, 1, kern=(FP,) * 4, bn=64, ns=(1, 1), chan=True, views=("dy",)),
    # ---- a few X channels: the image-edge kernels, else the column buffer
    _conv("edge_image", 2, 3, 20, 24, 192, 5, 2, 2, kern=EDGE, bn=None, ns=(0, 0), views=("x",)),     # ragged edge unit
    _conv("edge_c4_k3", 1, 4, 9, 7, 64, 3, 1, 1, kern=EDGE, bn=None, ns=(0, 0), views=("x",)),
    _conv("col_cout96", 2, 3, 20, 24, 96, 5, 2, 2, kern=NARROW, bn=64, im2col=1, ns=(4, 4)),          # Cout outside {64, 128, 192}
    _conv("col_kp128", 2, 5, 12, 12, 64, 5, 2, 2, kern=NARROW, bn=192, im2col=1, ns=(2, 2)),
    _conv("col_k3", 2, 8, 12, 12, 64, 3, 2, 1, kern=NARROW, bn=64, im2col=1, ns=(2, 2)),
    # ---- the bias gradient's row kernel at each channel count, rows % blocks != 0 (323 rows, 2 blocks); C = 6: the
    # strided kernel
    _conv("bias_c64", 1, 8, 17, 19, 64, 1, 1, 0, kern=NARROW, bn=64, im2col=1, ns=(6, 6)),
    _conv("bias_c136", 1, 8, 17, 19, 136, 1, 1, 0, kern=NARROW, bn=64, im2col=1, ns=(6, 6)),
    _conv("bias_c192", 1, 8, 17, 19, 192, 1, 1, 0, kern=NARROW, bn=64, im2col=1, ns=(6, 6)),
    _conv("bias_c320", 1, 8, 17, 19, 320, 1, 1, 0, kern=NARROW, bn=64, im2col=1, ns=(6, 6)),
    _conv("bias_c6", 1, 8, 17, 19, 6, 1, 1, 0, kern=(FP,) * 4, bn=64, im2col=1, ns=(6, 6)),
    # ---- transposed convolutions: G = x on the input grid, X = dy
    _tconv("t_x3d16_16x16", 2, 192, 16, 16, 192, 5, 2, 2, 1, kern=WIDE_BF, bn=192, sub="x3d16", ns=(8, 8)),
    _tconv("t_x3d16_8x16", 2, 192, 8, 16, 192, 5, 2, 2, 1, kern=WIDE_BF, bn=192, sub="x3d16", ns=(4, 4)),
    _tconv("t_x3rf_cg320", 1, 320, 15, 16, 192, 5, 2, 2, 1, kern=WIDE_SP, bn=192, sub="x3rf", ns=(4, 4)),  # P = 240
    _tconv("t_x3g", 2, 192, 6, 6, 192, 3, 1, 1, 0, kern=WIDE_SP, bn=192, sub="x3g", ns=(2, 2)),
    _tconv("t_edge", 2, 192, 20, 24, 3, 5, 2, 2, 1, kern=EDGE, bn=None, ns=(0, 0), views=("dy",)),   # db: planes, 2 chunks
    _tconv("t_edge_ragged", 1, 192, 20, 23, 3, 5, 2, 2, 1, kern=EDGE, bn=None, ns=(0, 0), views=("dy",)),  # 1,840-pixel planes
    _tconv("t_edge_one_chunk", 2, 64, 16, 16, 3, 5, 2, 2, 1, kern=EDGE, bn=None, ns=(0, 0), views=("dy",)),  # 2 x 3 x 32 x 32
    _tconv("t_col_cin96", 2, 96, 20, 24, 3, 5, 2, 2, 1, kern=NARROW, bn=64, im2col=1, ns=(15, 15)),
    _tconv("t_col_cin80", 1, 80, 9, 7, 3, 5, 2, 2, 1, kern=NARROW, bn=64, im2col=1, ns=(1, 1)),       # db: 18 x 14 planes
    # 25 taps x 6 channels = 150 columns, wider than the column buffer's 128: the gather form on dy itself
    _tconv("t_gather_kp160", 1, 64, 9, 7, 6, 5, 2, 2, 1, kern=(GA,) * 4, bn=64, ns=(1, 1), dyfmt="nchw"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

VIEWS = ("compact", "x", "dy", "both")


def out_hw(c):
    if c.tr:
        return ((c.h - 1) * c.s - 2 * c.p + c.k + c.op, (c.w - 1) * c.s - 2 * c.p + c.k + c.op)
    return ((c.h + 2 * c.p - c.k) // c.s + 1, (c.w + 2 * c.p - c.k) // c.s + 1)


def weight_shape(c):
    return (c.cin, c.cout, c.k, c.k) if c.tr else (c.cout, c.cin, c.k, c.k)


def op_name(c):
    return "conv_transpose2d_wgrad" if c.tr else "conv2d_wgrad"


def gemm(c):
    """The GEMM's geometry: G's channels, height, width; X's channels and layout."""
    ho, wo = out_hw(c)
    if c.tr:
        return dict(Cg=c.cin, Hg=c.h, Wg=c.w, Cx=c.cout, xfmt=c.dyfmt, gfmt=c.xfmt)
    return dict(Cg=c.cout, Hg=ho, Wg=wo, Cx=c.cin, xfmt=c.xfmt, gfmt=c.dyfmt)


def is_edge(c):
    return c.kern[0] == ED


def wide(c):
    """wg_plan's condition for the split kernel family: both operands channel-contiguous with 16-byte aligned
    rows of >= 128 channels."""
    g = gemm(c)
    return (not c.im2col and not c.chan and g["xfmt"] == "cl" and g["gfmt"] == "cl" and g["Cx"] >= 128 and
            g["Cg"] >= 128 and g["Cx"] % 4 == 0 and g["Cg"] % 4 == 0)


def runs_split_family(c, math):
    """Whether the launch is one of the split family's (wg_split or wg_bf16) in this math mode."""
    g = gemm(c)
    P = c.n * g["Hg"] * g["Wg"]
    bf16_ok = g["Wg"] % 16 == 0 and (g["Wg"] % 32 == 0 or P % 32 == 0)
    return wide(c) and bool((math & 2) or ((math & 1) and bf16_ok))


def restate_nsplit(c, math):
    """wg_plan, restated: (nsplit, pps).  One block of a split-family kernel is resident per CU (256 slots), two
    of any other (512); never fewer than 64 pixels per split; splits of whole 32-pixel steps."""
    if is_edge(c):
        return 0, 0
    g = gemm(c)
    P = c.n * g["Hg"] * g["Wg"]
    T, Cx = c.k * c.k, g["Cx"]
    if c.im2col:
        T, Cx = 1, (T * Cx + 31) // 32 * 32     # one tap over the column buffer's Kp columns
    generic = Cx % 4 != 0 or g["xfmt"] != "cl"
    if generic:
        tiles = -(-g["Cg"] // 192) * -(-(T * Cx) // 64)
    else:
        tiles = -(-g["Cg"] // 192) * -(-Cx // (192 if Cx >= 128 else 64)) * T
    slots = 256 if runs_split_family(c, math) else 512
    ns = max(1, min(slots // tiles if tiles < slots else 1, -(-P // 64)))
    pps = -(-(-(-P // ns)) // 32) * 32
    return -(-P // pps), pps


def split_sub(c):
    """wg_x3_launch, restated: the kernel behind wg_split (math 2), None outside the split family."""
    if not wide(c):
        return None
    g = gemm(c)
    Wg, P = g["Wg"], c.n * g["Hg"] * g["Wg"]
    pps = restate_nsplit(c, 2)[1]
    rowfast = Wg % 16 == 0 and pps % 16 == 0
    if (c.s == 2 and c.k == 5 and g["Cg"] == 192 and g["Cx"] == 192 and rowfast and Wg % 32 == 0 and pps % 32 == 0 and
            P % 32 == 0):
        return "x3p"
    if rowfast and Wg % 32 == 0:
        return "x3d"
    if rowfast and P % 32 == 0:
        return "x3d16"
    return "x3rf" if rowfast else "x3g"


def expected_plan(c, math):
    """The table's plan of the case in one math mode, in the fields of _lib.plan."""
    g = gemm(c)
    if is_edge(c):
        bf = bool(math & 1)
        # the bias gradient rides in G's all-ones column when the bias is G's (a convolution's) and G is not rounded
        kc = c.k * c.k * g["Cx"] + (0 if (c.tr or bf) else 1)
        return dict(kernel=c.kern[math], bm=g["Cg"], bn=kc, nsplit=0, im2col=0, variant=1 if math else 0)
    return dict(kernel=c.kern[math], bm=192, bn=c.bn, nsplit=c.ns[1 if runs_split_family(c, math) else 0],
                im2col=c.im2col, variant=int(g["Wg"] % 16 == 0))


def colsum_kernel(c):
    """csrc/wgrad.hip colsum, restated: which kernel sums dy into db ("ones": the edge kernel's all-ones column,
    fp32 and split arithmetic of a convolution)."""
    ho, wo = out_hw(c)
    rows, hw = c.n * ho * wo, ho * wo
    nb = max(1, min(512, -(-rows // 256)))
    if c.dyfmt == "cl" and c.cout % 4 == 0:
        return "rows"
    if c.dyfmt == "nchw" and hw >= 1024 and c.n * c.cout <= nb:
        nchunk = max(1, nb // (c.n * c.cout))
        chunk = -(-(-(-hw // nchunk)) // 1024) * 1024
        return "planes:%d" % -(-hw // chunk)
    return "partial"


def paths(c):
    """The launch paths the case reaches, over its math modes."""
    out = set()
    g = gemm(c)
    for m in MATHS:
        k = c.kern[m]
        if k == SP:
            out.add("split:" + c.sub)
        elif k == BF:
            out.add("bf16:" + c.sub)
        elif k in (LD, FP):
            out.add("%s:%d" % (k, c.bn))
        else:
            out.add(k)
        if c.im2col:
            out.add("im2col")
        if not is_edge(c):
            ns = c.ns[1 if runs_split_family(c, m) else 0]
            out.add("reduce:G%d:%s" % (-(-ns // 32), "rowfast" if g["Wg"] % 16 == 0 else "gather"))
    out.add("colsum:" + colsum_kernel(c))
    return out


REQUIRED_PATHS = (
    {"split:" + s for s in SUBS} | {"bf16:" + s for s in BF16_SUBS} |
    {"wg_ldsdma:192", "wg_ldsdma:64", "wg_fp32:192", "wg_fp32:64", GA, ED, EB, "im2col",
     "reduce:G1:rowfast", "reduce:G2:rowfast", "reduce:G1:gather", "reduce:G2:gather",
     "colsum:rows", "colsum:partial", "colsum:planes:1", "colsum:planes:2"})


# ---------------------------------------------------------------- operands
def _values(c):
    """x and dy as compact NCHW fp32 tensors from a generator seeded by the case's place in the table."""
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    ho, wo = out_hw(c)
    return (torch.randn(c.n, c.cin, c.h, c.w, generator=g), torch.randn(c.n, c.cout, ho, wo, generator=g))


def _place(v, shape, fmt, halo, chan, device):
    """The tensor of `shape` in layout `fmt` holding v (None: uninitialised), compact, or as the interior of a
    NaN-filled tensor one pixel larger on every side (halo), or as channels [1 : C + 1] of a NaN-filled
    channels-last tensor of C + 8 channels (chan)."""
    n, ch, h, w = shape
    big = (n, ch + 8 if chan else ch, h + 2 * halo, w + 2 * halo)
    mf = CL if fmt == "cl" else torch.contiguous_format
    if v is None:
        t = torch.empty(big, device=device).contiguous(memory_format=mf)
    else:
        t = torch.full(big, float("nan")).contiguous(memory_format=mf)
    view = t[:, 1:ch + 1] if chan else t
    if halo:
        view = view[:, :, 1:-1, 1:-1]
    if v is not None:
        view.copy_(v)
        if t.device != torch.device(device):
            t = t.to(device)        # the whole buffer moves, then the same view of it is taken
            view = t[:, 1:ch + 1] if chan else t
            view = view[:, :, 1:-1, 1:-1] if halo else view
    assert tuple(view.shape) == tuple(shape)
    return view


def make_operands(c, view="compact", device="cpu", values=True):
    """(x, dy) of the case on `device`.  view: "compact", or which operands are interiors of NaN-haloed tensors
    ("x", "dy", "both").  A `chan` case's x is the channel slice in every view.  values=False: uninitialised
    memory of the same layout (for a plan query)."""
    assert view in VIEWS, view
    ho, wo = out_hw(c)
    vx, vdy = _values(c) if values else (None, None)
    x = _place(vx, (c.n, c.cin, c.h, c.w), c.xfmt, int(view in ("x", "both")), c.chan, device)
    dy = _place(vdy, (c.n, c.cout, ho, wo), c.dyfmt, int(view in ("dy", "both")), False, device)
    return x, dy


def round_bf16(t):
    """Round-to-nearest-even to bf16, kept in t's dtype: what a bf16-operand kernel multiplies."""
    return t.to(torch.bfloat16).to(t.dtype)


def reference(c, x, dy):
    """(dw, db) in float64 from torch's own convolution autograd on the same values, on their device."""
    x64 = x.detach().double().contiguous()
    dy64 = dy.detach().double().contiguous()
    w = torch.zeros(weight_shape(c), dtype=torch.float64, device=x.device, requires_grad=True)
    b = torch.zeros(c.cout, dtype=torch.float64, device=x.device, requires_grad=True)
    if c.tr:
        y = F.conv_transpose2d(x64, w, b, stride=c.s, padding=c.p, output_padding=c.op)
    else:
        y = F.conv2d(x64, w, b, stride=c.s, padding=c.p)
    assert y.shape == dy64.shape, (c.name, y.shape, dy64.shape)
    y.backward(dy64)
    return w.grad, b.grad


def plan_of(c, x, dy, math):
    from image_compression_amd import _lib
    p = _lib.plan(op_name(c), x, dy, c.k, c.s, c.p, math)
    return {k: p[k] for k in ("kernel", "bm", "bn", "nsplit", "im2col", "variant")}


# ---------------------------------------------------------------- GDN backward on the GEMM path
# (C, N, H, W, layout): dgamma = q^T x^2 on the weight-gradient kernels with x squared in the load, dbeta the
# column sums of q
GDN_CASES = [
    (96, 2, 33, 33, "cl"),      # 2,178 pixels: 35 splits, two-level reduce, gather map
    (96, 2, 32, 48, "cl"),      # row-fast map, two-level reduce
    (320, 2, 8, 8, "cl"),       # second row / column tile partial
    (10, 2, 9, 7, "cl"),        # C % 4 != 0: gather form
    (3, 2, 9, 7, "nchw"),       # gather form through the channel stride
    (192, 1, 9, 16, "nchw"),
]


def gdn_nsplit(C, n, h, w, fmt):
    """wg_plan for the GDN backward's dgamma GEMM (one tap, G = q and X = x on the same grid), restated."""
    P = n * h * w
    generic = C % 4 != 0 or fmt != "cl"
    tiles = -(-C // 192) * -(-C // (64 if generic or C < 128 else 192))
    ns = max(1, min(512 // tiles if tiles < 512 else 1, -(-P // 64)))
    pps = -(-(-(-P // ns)) // 32) * 32
    return -(-P // pps)

