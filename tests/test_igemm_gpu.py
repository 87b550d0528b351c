"""The forward and input-gradient kernels (csrc/igemm.hip, the edge, tconv_few, im2col and col2im paths of
csrc/conv_api.hip) one op at a time: torch.ops.imgcomp.conv2d_fwd / conv2d_dgrad / conv_transpose2d_fwd /
conv_transpose2d_dgrad on every case of igemm_cases.CASES (test_igemm_plans.py holds, without a GPU, which kernel
each launches), against torch's own float64 convolution of the same values on the device.

Per case, op and math mode the plan is asserted before the launch.  fp32 at the project's bar; split
arithmetic within 1.5x of the native fp32 kernel's own error and bitwise different from it where a split kernel is
planned, bitwise equal where the plan is the fp32 kernel's; bf16 operands by the two-sided rule of
test_wgrad_gpu._bf16_rule (fp32-class against fp64 of the rounded operands, bf16-class against exact fp64); a
mode that cannot take bf16 bitwise the mode it falls to; the same call twice bitwise equal; a NaN-filled block of
the workspace's size allocated and freed before every call, so that a partial sum nobody wrote most likely reads
NaN.  The input once more as the interior of a NaN-filled tensor: bitwise the compact result where the plan is the
same, the bars above where the kernel wants a compact input; the output as the interior of a NaN-filled tensor
through the C ABI: bitwise, and the halo still NaN.  The measured errors are printed (DESIGN.md 1c holds them)."""
import pytest
import torch

import igemm_cases as G
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [c.name for c in G.CASES]
IC_MATH_WPACKED = 4


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
    """conftest.assert_close at 1e-4, the same criterion evaluated on the device (the largest maps have 25 million
    elements); on a miss conftest's own check runs for its message."""
    assert a.shape == ref.shape, (name, a.shape, ref.shape)
    atol = 1e-4 * max(float(ref.abs().max()), 1e-30)
    if bool(((a.double() - ref).abs() > atol + 1e-4 * ref.abs()).any()):
        assert_close(a.cpu(), ref.cpu(), 1e-4, name)
        raise AssertionError(name)


def _ws_query(c, op, inp, out, math):
    from image_compression_amd import _lib
    L = _lib.load()
    q = getattr(L, "ic_%s_ws_ex" % G.op_name(c, op))
    return q(_lib.act(inp), c.k, c.s, c.p, _lib.act(out), math)


class Run:
    """One case's operands on the device and its launches."""

    def __init__(self, c):
        self.c = c
        self.vals = G.values(c)
        self.v = {k: t.to(DEV) for k, t in self.vals.items()}

    def inp(self, op, view="compact"):
        return G.make_input(self.c, op, view, DEV, self.vals)

    def check_plan(self, op, inp, math, want, out=None):
        out = G.make_output(self.c, op, DEV)[1] if out is None else out
        got = G.plan_of(self.c, op, inp, out, math)
        assert got == want, (self.c.name, op, math, got, want)
        return out

    def launch(self, op, inp, math, w=None, copy=None):
        """The torch op on the case's weight (w: another one) after a freed NaN block of its workspace's size."""
        from image_compression_amd import _lib
        c, ops = self.c, _lib.ops()
        w = self.v["w"] if w is None else w
        like = G.make_output(c, op, DEV)[1]
        _nan_block(_ws_query(c, op, inp, like, math))
        tail = "" if copy is None else "_xb"
        fn = getattr(ops, G.op_name(c, op) + tail)
        a = (inp,) if copy is None else (inp, copy)
        if op == "fwd":
            y = fn(*a, w, self.v["b"], c.s, c.p, *((c.op,) if c.tr else ()), int(c.relu), math)
        else:
            y = fn(*a, w, like, c.s, c.p, math)
        if copy is None:    # the *_xb input gradients give dx the layout of its channel count
            assert y.shape == like.shape and y.stride() == like.stride(), (c.name, op, y.stride(), like.stride())
        assert bool(torch.isfinite(y).all()), (c.name, op, math, "NaN / inf in the result")
        return y

    def abi(self, op, inp, out, math):
        """The same op through the C ABI into `out` (a view)."""
        from image_compression_amd import _lib
        c, L = self.c, _lib.load()
        nb = _ws_query(c, op, inp, out, math)
        _nan_block(nb)
        ws = _lib.workspace(nb, DEV)
        fn = getattr(L, "ic_%s_ex" % G.op_name(c, op))
        if op == "fwd":
            rc = fn(_lib.act(inp), _lib.ptr(self.v["w"]), _lib.ptr(self.v["b"]), c.k, c.s, c.p, _lib.act(out),
                    int(c.relu), math, _lib.ptr(ws), nb, _lib.stream_of(inp))
        else:
            rc = fn(_lib.act(inp), _lib.ptr(self.v["w"]), c.k, c.s, c.p, _lib.act(out), math, _lib.ptr(ws), nb,
                    _lib.stream_of(inp))
        _lib.check(rc, G.op_name(c, op))
        torch.cuda.synchronize()

    def ref(self, op, inp, w=None):
        c = self.c
        return G.reference(c, op, inp, self.v["w"] if w is None else w, self.v["b"], c.relu)


def _tag(c, op, math, p):
    return f"IGEMM {c.name} {op} math {math} {p['kernel']} {p['bm']}x{p['bn']} ks{p['ksplit']}"


def _split_planned(p):
    return p["kernel"] in ("ig_split", "ig_split_dma") or (p["variant"] == 1 and p["kernel"] not in G.BF16_KERNELS)


def _split_rule(tag, got, native, ref):
    """test_split_gpu._check: the fp32 bar, no worse than 1.5x the native fp32 kernel, and not its bits."""
    _close(got, ref, tag)
    es, en = _rel(got, ref), _rel(native, ref)
    print(f"{tag}: split {es:.2e} native fp32 {en:.2e}")
    assert es <= 1.5 * en + 1e-8, (tag, es, en)
    assert not torch.equal(got, native), (tag, "the split kernel did not run")


class Bf16Rule:
    """test_wgrad_gpu._bf16_rule's two sides.  e_ref: the native fp32 kernel (math 0) on the same pre-rounded
    input and weight, against fp64 of them; measured once per op."""

    def __init__(self, run, op, inp, ref):
        self.run, self.op, self.inp, self.exact = run, op, inp, ref
        self.ref_r = None

    def __call__(self, tag, got):
        r = self.run
        if self.ref_r is None:
            ir, wr = G.round_bf16(self.inp), G.round_bf16(r.v["w"])
            assert ir.stride() == self.inp.stride()
            self.ref_r = r.ref(self.op, ir, wr)
            self.e_ref = _rel(r.launch(self.op, ir, 0, w=wr), self.ref_r)
        e_em, e = _rel(got, self.ref_r), _rel(got, self.exact)
        print(f"{tag}: vs fp64 of the bf16 operands {e_em:.2e} (fp32 kernel on them {self.e_ref:.2e}), vs fp64 {e:.2e}")
        assert e_em <= max(1e-5, 2 * self.e_ref), (tag, e_em, self.e_ref)
        assert 1e-5 < e < 1e-2, (tag, e)


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_igemm_parity(case):
    c, r = case, Run(case)
    for op in G.OPS:
        plans, inp = c.plans[op], r.inp(op)
        ref = r.ref(op, inp)
        bf16 = Bf16Rule(r, op, inp, ref)
        out = {}
        for m in G.MATHS:
            r.check_plan(op, inp, m, plans[m])
            out[m] = r.launch(op, inp, m)
            assert torch.equal(r.launch(op, inp, m), out[m]), (c.name, op, m, "two runs differ")
        # fp32
        _close(out[0], ref, _tag(c, op, 0, plans[0]))
        print(f"{_tag(c, op, 0, plans[0])}: native fp32 {_rel(out[0], ref):.2e}")
        # split arithmetic: a split kernel, else the fp32 launch itself
        assert _split_planned(plans[2]) == (plans[2] != plans[0]), (c.name, op)
        if _split_planned(plans[2]):
            _split_rule(_tag(c, op, 2, plans[2]), out[2], out[0], ref)
        else:
            assert torch.equal(out[2], out[0]), (c.name, op, "math 2 is not the fp32 launch")
        # bf16 operands, or the launch of the mode without them
        for m, base in ((1, 0), (3, 2)):
            if plans[m]["kernel"] in G.BF16_KERNELS:
                bf16(_tag(c, op, m, plans[m]), out[m])
            else:
                assert plans[m] == plans[base]
                assert torch.equal(out[m], out[base]), (c.name, op, f"math {m} is not the math {base} launch")
        # the input as the interior of a NaN-filled tensor: the same values in the same order where the plan is the
        # same; the kernels that want a compact input give way to others, held to the bars above
        iv = r.inp(op, "halo")
        assert torch.equal(iv, inp) and not iv.is_contiguous(memory_format=G.CL) and not iv.is_contiguous()
        hout = {}
        for m in G.MATHS:
            hp = c.halo[op][m]
            r.check_plan(op, iv, m, hp)
            hout[m] = r.launch(op, iv, m)
            tag = _tag(c, op, m, hp) + " (halo)"
            if hp == plans[m]:
                assert torch.equal(hout[m], out[m]), (tag, "differs from the compact run")
            elif hp["kernel"] in G.BF16_KERNELS:
                bf16(tag, hout[m])
            elif _split_planned(hp):
                _split_rule(tag, hout[m], hout[0], ref)
            else:
                _close(hout[m], ref, tag)
                print(f"{tag}: native fp32 {_rel(hout[m], ref):.2e}")
                assert torch.equal(hout[m], hout[0]), (tag, "not the halo view's fp32 launch")
        # the output as the interior of a NaN-filled tensor, through the C ABI: no store outside the map
        if c.yview:
            for m in G.MATHS:
                big, yv = G.make_output(c, op, DEV, haloed=True)
                r.check_plan(op, inp, m, plans[m], out=yv)
                r.abi(op, inp, yv, m)
                assert torch.equal(yv, out[m]), (c.name, op, m, "the view's interior differs from the op's result")
                assert int(torch.isnan(big).sum()) == big.numel() - yv.numel(), (c.name, op, m, "halo written")


@pytest.mark.parametrize("op", G.OPS)
@pytest.mark.parametrize("name", G.MISALIGNED)
def test_misaligned_channel_slice(name, op):
    """An input off 16-byte alignment (a channel slice of a wider channels-last tensor) runs the gather form,
    asserted from the plan query before each launch, and meets the fp32 bar in every math mode."""
    c = G.BY_NAME[name]
    r = Run(c)
    ref = r.ref(op, r.inp(op))
    for view in G.CHAN_VIEWS:
        iv = r.inp(op, view)
        assert iv.data_ptr() % 16 == (4 if view == "chan8" else 0) and (view == "chan8" or iv.stride(3) % 4 == 1)
        outs = []
        for m in G.MATHS:
            like = G.make_output(c, op, DEV)[1]
            p = G.plan_of(c, op, iv, like, m)
            assert p["kernel"] == "ig_fp32_gather", (name, op, view, m, p)   # never a 16-byte load of this input
            outs.append(r.launch(op, iv, m))
        _close(outs[0], ref, f"{name} {op} {view}")
        print(f"{_tag(c, op, 0, p)} ({view}): native fp32 {_rel(outs[0], ref):.2e}")
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), (name, op, view, "the math modes differ")


@pytest.mark.parametrize("name", ["dma_k3", "dma_tconv_op0"])
def test_bf16_copy_bitwise(name):
    """The *_xb ops read the input's bf16 copy where the bf16 DMA tiles run (the same round-to-nearest values the
    op forms itself) and ignore it elsewhere: bitwise the math-1 result without the copy."""
    c = G.BY_NAME[name]
    r = Run(c)
    for op in G.OPS:
        inp = r.inp(op)
        r.check_plan(op, inp, 1, c.plans[op][1])
        plain = r.launch(op, inp, 1)
        cp = inp.to(torch.bfloat16)
        assert cp.stride() == inp.stride()
        got = r.launch(op, inp, 1, copy=cp)
        assert got.shape == plain.shape and torch.equal(got, plain), (name, op)


@pytest.mark.parametrize("math", [0, 1, 2])
@pytest.mark.parametrize("name", ["body_s2", "tconv_body", "edge_image", "dma_k3"])
def test_cached_pack_bitwise(name, math):
    """conv2d_fwd_ws / conv_transpose2d_fwd_ws on a caller's workspace: the packing call and the call that finds
    the pack there (IC_MATH_WPACKED) are bitwise the plain forward."""
    from image_compression_amd import _lib
    c = G.BY_NAME[name]
    r = Run(c)
    x = r.inp("fwd")
    r.check_plan("fwd", x, math, c.plans["fwd"][math])
    plain = r.launch("fwd", x, math)
    ws = torch.empty(16, dtype=torch.uint8, device=DEV)
    fn = getattr(_lib.ops(), G.op_name(c, "fwd") + "_ws")
    for m in (math, math | IC_MATH_WPACKED):
        y = fn(x, r.v["w"], r.v["b"], c.s, c.p, *((c.op,) if c.tr else ()), int(c.relu), m, ws)
        assert torch.equal(y, plain), (name, math, m)
