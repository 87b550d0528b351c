"""GDN / IGDN one op at a time on every launch path (csrc/gdn_fused.hip, the implicit-GEMM detour of csrc/gdn.hip):
torch.ops.imgcomp.gdn_fwd / gdn_bwd / gdn_bwd_sum / gdn_fwd_xb / gdn_bwd_sum_xb / gdn_fwd_rn / gdn_bwd_sum_rn on
every case of gdn_cases.CASES (test_gdn_plans.py holds, without a GPU, which kernel each launches and how many
tiles a block runs), both directions, GDN and IGDN, against float64 on the CPU (gdn_cases.reference).

Per case, direction and math mode the plan is asserted before the launch.
  fp32 (math 0): y, norm, dx, dgamma, dbeta, dxsum at the project's bar (conftest.assert_close, 1e-4).
  split (math 2): the same bar; where a split kernel or the split GEMM runs, y, norm, dx and dgamma within 1.5x of
    the math-0 launch's own error (+ 1e-8) and not its bits (dbeta and dxsum are plain sums, in another order on
    the pipelined split backward: the fp32 bar); bitwise the math-0 result where the plan is math 0's.
  bf16 (math 3; math 1 in the backward at C = 192): against gdn_cases.emulate, float64 of the kernels' bf16
    operands, below gdn_cases.EMUL_BOUND; against exact float64 between 1e-5 and 1e-2, so bf16 operands really
    ran; dbeta, a plain sum of the unrounded q, at the fp32 bar against the sum of the q that follows from the norm
    the kernel was given (the emulation's).
  A mode that repeats another mode's launch (gdn_cases.falls_to) is bitwise that mode's result.
The backward takes the fp32 forward's norm; at math 3 on the bf16 kernel the bf16 forward's, as the layer does.
dxsum is also held to the column sums of the kernel's own dx.  Every call runs twice, bitwise equal, after a
NaN-filled block of the workspace's size was freed; every output is finite; gdn_bwd is gdn_bwd_sum bit for bit.

The bf16 copies are the fp32 results rounded to nearest even, bit for bit, from the fused bf16 kernel and from the
ig_cvt_bf16 pass after every other path; the norm-free pair is the storing pair bit for bit on every C = 192 pixel
set; the C ABI writes y, norm, dx and the copies into interiors of NaN-filled buffers and leaves every guard
element NaN, with x, norm and dy read out of NaN surrounds; functional.gdn runs a batch of 1 x 1 maps.  The
measured errors are printed (DESIGN.md 1d holds them)."""

import pytest
import torch

import gdn_cases as G
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
INV = pytest.mark.parametrize("inverse", (False, True), ids=("gdn", "igdn"))
FWD_OUT = ("y", "norm")
BWD_OUT = ("dx", "dgamma", "dbeta", "dxsum")


def _nan_block(nbytes):
    """Allocate and free a block of NaN (all bits set) of the workspace's size: the op's own workspace, allocated
    next, most likely lands on it.  Nothing here depends on that."""
    t = torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)
    del t


def _rel(a, ref):
    """conftest.rel_err, on the device: ||a - ref|| / ||ref|| in float64."""
    nb = float(ref.norm())
    return float((a.double() - ref).norm()) / (nb if nb > 0 else 1.0)


def _close(a, ref, name):
    """conftest.assert_close at 1e-4, the same criterion evaluated on the device; on a miss conftest's own check runs
    for its message."""
    assert a.shape == ref.shape, (name, a.shape, ref.shape)
    atol = 1e-4 * max(float(ref.abs().max()), 1e-30)
    if bool(((a.double() - ref).abs() > atol + 1e-4 * ref.abs()).any()):
        assert_close(a.cpu(), ref.cpu(), 1e-4, name)
        raise AssertionError(name)


def _dev(d):
    return {k: t.to(DEV) for k, t in d.items()}


def _layout_of(t, x):
    """t has x's layout: equal strides in every dimension above size 1"""
    return t.shape == x.shape and all(a == b for a, b, n in zip(t.stride(), x.stride(), x.shape) if n > 1)


def _ws(direction, x, math):
    from image_compression_amd import _lib
    L = _lib.load()
    return L.ic_gdn_fwd_ws_ex(_lib.act(x), math) if direction == "fwd" else L.ic_gdn_bwd_ws(_lib.act(x))


class Run:
    """One case's operands on the device and its launches."""

    def __init__(self, c):
        v = G.values(c.name)
        self.c = c
        self.x, self.dy = G.make(c, v["x"], DEV), G.make(c, v["dy"], DEV)
        self.gamma, self.beta = v["gamma"].to(DEV), v["beta"].to(DEV)
        assert self.x.stride() == self.dy.stride()

    def check_plan(self, direction, math):
        got, want = G.plan_of(direction, self.x, math), G.expected_plan(self.c, direction, math)
        assert got == want, (self.c.name, direction, math, got, want)
        return want

    def _finite(self, out, what):
        for t in out:
            assert bool(torch.isfinite(t.float()).all()), (self.c.name, what, "NaN / inf in a result")
        return out

    def fwd(self, math, inverse, op="gdn_fwd", *extra):
        from image_compression_amd import _lib
        _nan_block(_ws("fwd", self.x, math))
        return self._finite(getattr(_lib.ops(), op)(self.x, self.gamma, self.beta, inverse, math, *extra), (op, math))

    def bwd(self, nob, math, inverse, op="gdn_bwd_sum", *extra):
        """nob: norm, or beta for the norm-free op."""
        from image_compression_amd import _lib
        _nan_block(_ws("bwd", self.x, math))
        return self._finite(getattr(_lib.ops(), op)(self.x, nob, self.dy, self.gamma, inverse, math, *extra), (op, math))


def _same(a, b, what):
    for i, (s, t) in enumerate(zip(a, b)):
        assert s.shape == t.shape and torch.equal(s, t), (what, i, float((s.float() - t.float()).abs().max()))


def _tag(c, inverse, direction, math, kernel):
    return f"GDN {c.name} {'igdn' if inverse else 'gdn'} {direction} math {math} {kernel}"


def _fp32_bar(tag, names, got, ref):
    errs = []
    for nm, t in zip(names, got):
        _close(t, ref[nm], f"{tag} {nm}")
        errs.append(f"{nm} {_rel(t, ref[nm]):.2e}")
    return " ".join(errs)


def _split_rule(tag, names, got, native, ref):
    """test_split_gpu._check on the outputs split arithmetic forms: the fp32 bar, no worse than 1.5x the fp32 kernel
    on the same inputs, and not its bits."""
    msg = _fp32_bar(tag, names, got, ref)
    for nm, t, t0 in zip(names, got, native):
        if nm in ("dbeta", "dxsum"):
            continue
        es, en = _rel(t, ref[nm]), _rel(t0, ref[nm])
        assert es <= 1.5 * en + 1e-8, (tag, nm, es, en)
        assert not torch.equal(t, t0), (tag, nm, "the split kernel did not run")
        msg += f" ({nm} fp32 {en:.2e})"
    print(f"{tag}: split {msg}")


def _bf16_rule(tag, names, got, emul, exact):
    """test_bf16_gpu's two sides; dbeta and dxsum apart (plain sums)."""
    msg = []
    for nm, t in zip(names, got):
        if nm == "dbeta":
            _close(t, emul[nm], f"{tag} dbeta")
            msg.append(f"dbeta {_rel(t, emul[nm]):.2e}")
            continue
        if nm == "dxsum":
            continue
        e_em, e = _rel(t, emul[nm]), _rel(t, exact[nm])
        msg.append(f"{nm} {e_em:.2e} / {e:.2e}")
        assert e_em < G.EMUL_BOUND, (tag, nm, "against float64 of the bf16 operands", e_em)
        assert 1e-5 < e < 1e-2, (tag, nm, "against exact float64", e)
    print(f"{tag}: vs fp64 of the bf16 operands / vs fp64: " + " ".join(msg))


def _column_sums(tag, dx, dxsum):
    """test_ops_gpu.test_gdn_bwd_dx_column_sums: dxsum[c] = sum over pixels of the kernel's own dx."""
    ref = dx.double().sum(dim=(0, 2, 3))
    assert float((dxsum.double() - ref).abs().max() / ref.abs().max()) < 1e-5, tag


@INV
@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_gdn_parity(case, inverse):
    c, r = case, Run(case)
    ref = _dev(G.reference(c.name, inverse))
    # ---- forward
    fo, kern = {}, {}
    for m in G.MATHS:
        kern[m] = r.check_plan("fwd", m)
        fo[m] = r.fwd(m, inverse)
        _same(r.fwd(m, inverse), fo[m], (c.name, "fwd", m, "two runs differ"))
        assert all(_layout_of(t, r.x) for t in fo[m])
    print(f"{_tag(c, inverse, 'fwd', 0, kern[0])}: fp32 {_fp32_bar(_tag(c, inverse, 'fwd', 0, kern[0]), FWD_OUT, fo[0], ref)}")
    for m in (1, 2, 3):
        tag, base = _tag(c, inverse, "fwd", m, kern[m]), G.falls_to(c, "fwd", m)
        if base is not None:
            _same(fo[m], fo[base], (tag, f"not the math {base} launch"))
            print(f"{tag}: = math {base}, bit for bit")
        elif kern[m] == G.FBF16:
            _bf16_rule(tag, FWD_OUT, fo[m], _dev(G.emulate(c.name, inverse, True, False)), ref)
        elif kern[m] == G.FSPLIT or G.split_gemm(c, m):
            _split_rule(tag, FWD_OUT, fo[m], fo[0], ref)
        else:   # the GEMM in fp32 where math 0 runs the fused kernel
            print(f"{tag}: fp32 {_fp32_bar(tag, FWD_OUT, fo[m], ref)}")
    # ---- backward
    bo = {}
    for m in G.MATHS:
        kern[m] = r.check_plan("bwd", m)
        norm = fo[3][1] if m == 3 and kern[m] == G.FBF16 else fo[0][1]
        bo[m] = r.bwd(norm, m, inverse)
        _same(r.bwd(norm, m, inverse), bo[m], (c.name, "bwd", m, "two runs differ"))
        _same(r.bwd(norm, m, inverse, "gdn_bwd"), bo[m][:3], (c.name, "bwd", m, "gdn_bwd is not gdn_bwd_sum"))
        assert _layout_of(bo[m][0], r.x) and bo[m][1].shape == r.gamma.shape
        _column_sums(_tag(c, inverse, "bwd", m, kern[m]), bo[m][0], bo[m][3])
    print(f"{_tag(c, inverse, 'bwd', 0, kern[0])}: fp32 {_fp32_bar(_tag(c, inverse, 'bwd', 0, kern[0]), BWD_OUT, bo[0], ref)}")
    for m in (1, 2, 3):
        tag, base = _tag(c, inverse, "bwd", m, kern[m]), G.falls_to(c, "bwd", m)
        if kern[m] == G.FBF16:      # math 1 and 3: one kernel, the fp32 and the bf16 forward's norm
            _bf16_rule(tag, BWD_OUT, bo[m], _dev(G.emulate(c.name, inverse, m == 3, True)), ref)
        elif base is not None:
            _same(bo[m], bo[base], (tag, f"not the math {base} launch"))
            print(f"{tag}: = math {base}, bit for bit")
        else:
            assert kern[m] == G.FSPLIT
            _split_rule(tag, BWD_OUT, bo[m], bo[0], ref)


COPY_CASES = [n for n in G.IDS if G.BY_NAME[n].C == 192 and G.BY_NAME[n].layout == "cl"] + \
    ["c64_p17", "c64_p4225", "c192_off4", "c48_cl"]


@INV
@pytest.mark.parametrize("name", COPY_CASES)
def test_gdn_copies_and_norm_recompute(name, inverse):
    """yb is y.to(bfloat16) and dxb dx.to(bfloat16), bit for bit, beside results that are bitwise the plain ops': from
    the fused bf16 kernel's epilogue (math 3, C = 192) and from the ig_cvt_bf16 pass after the fp32 and split
    kernels and the GEMM path.  The norm-free pair (gdn_fwd_rn / gdn_bwd_sum_rn) is the storing pair bit for bit,
    with and without the copies; any arithmetic but the fused bf16 kernels' refuses it."""
    c, r = G.BY_NAME[name], Run(G.BY_NAME[name])
    fused192 = c.C == 192 and G.fused_ok(c)
    for m in ((0, 2, 3) if c.C == 192 else (0,)):
        r.check_plan("fwd", m), r.check_plan("bwd", m)
        y, norm = r.fwd(m, inverse)
        y1, norm1, yb = r.fwd(m, inverse, "gdn_fwd_xb")
        _same((y1, norm1), (y, norm), (name, m, "gdn_fwd_xb is not gdn_fwd"))
        assert yb.dtype == torch.bfloat16 and yb.stride() == y.stride()
        assert torch.equal(yb, y.to(torch.bfloat16)), (name, m, "yb is not y rounded to nearest even")
        res = r.bwd(norm, m, inverse)
        rxb = r.bwd(norm, m, inverse, "gdn_bwd_sum_xb")
        _same(rxb[:4], res, (name, m, "gdn_bwd_sum_xb is not gdn_bwd_sum"))
        assert rxb[4].dtype == torch.bfloat16 and rxb[4].stride() == res[0].stride()
        assert torch.equal(rxb[4], res[0].to(torch.bfloat16)), (name, m, "dxb is not dx rounded to nearest even")
        if m == 3 and fused192:
            for xb in (True, False):
                y2, yb2 = r.fwd(3, inverse, "gdn_fwd_rn", xb)
                assert torch.equal(y2, y) and (torch.equal(yb2, yb) if xb else yb2.numel() == 0), (name, xb)
                r2 = r.bwd(r.beta, 3, inverse, "gdn_bwd_sum_rn", xb)
                _same(r2[:4], rxb[:4], (name, xb, "the norm-free backward is not the storing one"))
                assert torch.equal(r2[4], rxb[4]) if xb else r2[4].numel() == 0, (name, xb)
    # refused before any launch: the norm-free pair off the fused bf16 kernels
    from image_compression_amd import _lib
    ops = _lib.ops()
    for m in G.MATHS:
        if not (m == 3 and fused192):
            with pytest.raises(RuntimeError):
                ops.gdn_fwd_rn(r.x, r.gamma, r.beta, inverse, m, False)
        if G.expected_plan(c, "bwd", m) != G.FBF16:
            with pytest.raises(RuntimeError):
                ops.gdn_bwd_sum_rn(r.x, r.beta, r.dy, r.gamma, inverse, m, False)


def test_gdn_copies_refuse_nchw():
    """The bf16 copies are compact NHWC: an NCHW y / dx is refused (compact_nhwc), not given a mis-strided copy; the
    plain ops run the same operands."""
    from image_compression_amd import _lib
    ops, r = _lib.ops(), Run(G.BY_NAME["c192_nchw"])
    assert r.x.is_contiguous() and r.x.stride(1) != 1
    for m in (0, 3):
        y, norm = r.fwd(m, False)
        with pytest.raises(RuntimeError):
            ops.gdn_fwd_xb(r.x, r.gamma, r.beta, False, m)
        with pytest.raises(RuntimeError):
            ops.gdn_bwd_sum_xb(r.x, norm, r.dy, r.gamma, False, m)
        _same(r.fwd(m, False), (y, norm), "the forward after a refusal")


# ------------------------------------------------------------------ guard bands through the C ABI
GUARD = 12288   # elements on each side: two 32 x 192 tiles, a multiple of 4 (the interior stays 16-byte aligned)
GUARD_CASES = [(192, p, m) for p in (1, 17, 33, 4225, 16425) for m in (0, 2, 3)] + \
    [(C, p, 0) for C in (64, 128) for p in (17, 4225)]


class Guarded:
    """A tensor of x's shape as the interior of a NaN-filled flat buffer, NHWC-dense."""

    def __init__(self, like, dtype=torch.float32, values=None):
        n, ch, h, w = like.shape
        self.numel = like.numel()
        self.buf = torch.full((self.numel + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.numel].view(n, h, w, ch).permute(0, 3, 1, 2)
        assert self.t.data_ptr() % 16 == 0
        if values is not None:
            self.t.copy_(values)

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.numel:]).all())


@INV
@pytest.mark.parametrize("C,p,math", GUARD_CASES, ids=[f"c{C}_p{p}_m{m}" for C, p, m in GUARD_CASES])
def test_gdn_guard_bands(C, p, math, inverse):
    """The fused kernels keep rows past P out of memory three ways (m0 + row < P, a clamp to row P - 1, a dump
    slot).  Every output the C ABI writes is the interior of a NaN-filled buffer with 12288 elements of guard on each
    side, every input the interior of one too: the guards stay NaN, the results are finite and bitwise the op's own.
    Each guard is looked at right after the call that could have written it, before anything else runs."""
    from image_compression_amd import _lib
    L, c = _lib.load(), G.BY_NAME[f"c{C}_p{p}"]
    r = Run(c)
    x, dy = Guarded(r.x, values=r.x), Guarded(r.x, values=r.dy)
    assert G.plan_of("fwd", x.t, math) == G.expected_plan(c, "fwd", math)
    assert G.plan_of("bwd", x.t, math) == G.expected_plan(c, "bwd", math)
    ax, g, b, inv = _lib.act(x.t), _lib.ptr(r.gamma), _lib.ptr(r.beta), int(inverse)
    st = _lib.stream_of(r.x)
    bf = lambda: Guarded(r.x, torch.bfloat16)

    def call(fn, what, outs, *args):
        nb = _ws("fwd" if "fwd" in what else "bwd", x.t, math)
        _nan_block(nb)
        ws = _lib.workspace(nb, DEV)
        _lib.check(getattr(L, fn)(*args, _lib.ptr(ws), nb, st), what)
        torch.cuda.synchronize()
        for o in outs:
            assert o.intact(), (what, math, "a store outside the tensor")
            assert bool(torch.isfinite(o.t.float()).all()), (what, math, "NaN / inf in a result")
        assert x.intact() and dy.intact()

    y, norm, y1, norm1, yb = Guarded(r.x), Guarded(r.x), Guarded(r.x), Guarded(r.x), bf()
    call("ic_gdn_fwd_ex", "gdn_fwd", (y, norm), ax, g, b, inv, _lib.act(y.t), _lib.ptr(norm.t), math)
    call("ic_gdn_fwd_xb", "gdn_fwd_xb", (y1, norm1, yb), ax, g, b, inv, _lib.act(y1.t), _lib.ptr(norm1.t),
         _lib.ptr(yb.t), math)
    par = lambda: [torch.full_like(t, float("nan")) for t in (r.gamma, r.beta, r.beta)]   # dgamma, dbeta, dxsum
    dx, dx1, dxb, p0, p1 = Guarded(r.x), Guarded(r.x), bf(), par(), par()
    call("ic_gdn_bwd_sum_ex", "gdn_bwd_sum", (dx,), ax, _lib.ptr(norm.t), _lib.ptr(dy.t), g, inv, _lib.act(dx.t),
         *map(_lib.ptr, p0), math)
    call("ic_gdn_bwd_sum_xb", "gdn_bwd_sum_xb", (dx1, dxb), ax, _lib.ptr(norm.t), _lib.ptr(dy.t), g, inv,
         _lib.act(dx1.t), *map(_lib.ptr, p1), _lib.ptr(dxb.t), math)
    assert norm.intact()
    rn = None
    if math == 3:   # the norm-free pair
        y2, yb2, dx2, dxb2, p2 = Guarded(r.x), bf(), Guarded(r.x), bf(), par()
        call("ic_gdn_fwd_rn", "gdn_fwd_rn", (y2, yb2), ax, g, b, inv, _lib.act(y2.t), _lib.ptr(yb2.t), math)
        call("ic_gdn_bwd_sum_rn", "gdn_bwd_sum_rn", (dx2, dxb2), ax, b, _lib.ptr(dy.t), g, inv, _lib.act(dx2.t),
             *map(_lib.ptr, p2), _lib.ptr(dxb2.t), math)
        rn = (y2.t, yb2.t, dx2.t, *p2, dxb2.t)
    # the op's own results on compact operands
    oy, onorm, oyb = r.fwd(math, inverse, "gdn_fwd_xb")
    ores = r.bwd(onorm, math, inverse, "gdn_bwd_sum_xb")
    _same((y.t, norm.t, y1.t, norm1.t, yb.t), (oy, onorm, oy, onorm, oyb), (c.name, math, "forward"))
    _same((dx.t, *p0, dx1.t, *p1, dxb.t), (*ores[:4], *ores), (c.name, math, "backward"))
    if rn is not None:
        _same(rn, (oy, oyb, *ores), (c.name, "the norm-free pair"))


# ------------------------------------------------------------------ the layer path on a batch of 1 x 1 maps
@INV
@pytest.mark.parametrize("xb", (0, 3))
@pytest.mark.parametrize("math", (0, 2, 3))
@pytest.mark.parametrize("C", (192, 64))
def test_gdn_layer_on_1x1_maps(C, math, xb, inverse):
    """functional.gdn with math = math_fwd on (2, C, 1, 1): contiguous, so channels-last with strides (C, 1, 1, 1).
    The strides of the dimensions of size 1 kept such a tensor off the fused kernels, and with bf16 operands in both
    directions at C = 192 the layer asks for the norm-free forward, which the GEMM path refuses: it raised."""
    from image_compression_amd import functional as IF
    c = G.BY_NAME[f"c{C}_n2_1x1"]
    v, ref = G.values(c.name), _dev(G.reference(c.name, inverse))
    x, gamma, beta = (v[k].to(DEV).requires_grad_(True) for k in ("x", "gamma", "beta"))
    assert x.stride() == (C, 1, 1, 1)
    with IF.record_plans() as log:
        y = IF.gdn(x, gamma, beta, inverse, math, math, xb)
        y.backward(v["dy"].to(DEV))
    want = [G.expected_plan(c, "fwd", math), G.expected_plan(c, "bwd", math)]
    assert [p["kernel"] for p in log] == want, (log, want)
    names, got = ("y", "dx", "dgamma", "dbeta"), (y.detach(), x.grad, gamma.grad, beta.grad)
    tag = f"GDN layer {c.name} {'igdn' if inverse else 'gdn'} math {math} xb {xb} {want[0]} / {want[1]}"
    if want[1] == G.FBF16:
        _bf16_rule(tag, names, got, _dev(G.emulate(c.name, inverse, True, True)), ref)
    else:
        print(f"{tag}: fp32 {_fp32_bar(tag, names, got, ref)}")
