"""Which forward / input-gradient kernel each case of igemm_cases.CASES launches, from the library's plan query
(ic_conv_plan launches nothing, so this runs without a GPU): every case, compact and in each view the GPU test
runs, in the four math modes and both ops, must plan what the table says; the table must reach every launch path
of csrc/igemm.hip and the detours of csrc/conv_api.hip; a mode that cannot take bf16 operands must plan the
launch of the mode it falls to; and an input off 16-byte alignment must never plan a kernel that reads 16 bytes
at a time."""
import pytest
import torch

import igemm_cases as G

IDS = [c.name for c in G.CASES]
# the kernels whose A operand is read by float4 loads or LDS-DMA (csrc/igemm.hip); gemm_col2im runs them on x
VEC16 = ("ig_fp32", "ig_bf16", "ig_split", "ig_split_bf16", "ig_split_dma", "ig_bf16_dma", "gemm_col2im")


def _plans(c, op, view, haloed_out=False):
    inp = G.make_input(c, op, view)
    out = G.make_output(c, op, haloed=haloed_out)[1]
    return [G.plan_of(c, op, inp, out, m) for m in G.MATHS]


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_plan_is_the_tables(case):
    for op in G.OPS:
        assert _plans(case, op, "compact") == list(case.plans[op]), op
        assert _plans(case, op, "halo") == list(case.halo[op]), (op, "halo")
        if case.yview:      # the output view of the GPU test keeps the compact plan
            assert _plans(case, op, "compact", haloed_out=True) == list(case.plans[op]), (op, "y view")


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_fallback_takes_the_fallen_to_launch(case):
    """Where math 1 or 3 cannot take bf16 operands (Cin % 64 != 0, the gather form, a kernel without a bf16 form)
    the launch is the one of math 0 or 2, K split included (the GPU test asserts the results bitwise equal)."""
    for op in G.OPS:
        for plans in (_plans(case, op, "compact"), _plans(case, op, "halo")):
            cin = G.io(case, op)[0][1]
            for m, base in ((1, 0), (3, 2)):
                if plans[m]["kernel"] not in G.BF16_KERNELS:
                    assert plans[m] == plans[base], (op, m)
            if plans[0]["kernel"] in G.IG_KERNELS and (cin % 64 or plans[0]["kernel"] == "ig_fp32_gather"):
                assert plans[1] == plans[0] and plans[3] == plans[2], op
            # math 3 is math 1 wherever bf16 operands run
            if plans[1]["kernel"] in G.BF16_KERNELS:
                assert plans[3] == plans[1], op


def test_table_reaches_every_path():
    reached = set().union(*(G.paths(c) for c in G.CASES))
    assert not (G.REQUIRED_PATHS - reached), sorted(G.REQUIRED_PATHS - reached)


def test_named_edge_cases_hold():
    """The geometry that gates the cases named for an edge."""
    B = G.BY_NAME
    # odd output sizes: a direct gather whose bottom / right taps leave the image, sub-pixel phases of unequal size
    assert G.out_hw(B["dma_s2_odd"]) == (90, 91) and G.out_hw(B["dma_tconv_op0"]) == (255, 255)
    assert G.out_hw(B["tconv_k3s2_op0"]) == (13, 9) and G.io(B["dma_dgrad4_odd"], "dgrad")[2][2:] == (255, 255)
    assert [p[2] for p in G.phases(B["tconv_k3s2_op0"], "fwd")] == [1, 2, 2, 4]
    assert len({p[:2] for p in G.phases(B["tconv_k3s2_op0"], "fwd")}) == 4
    # four phases of 9 / 6 / 6 / 4 taps on 27 splits of 2 chunks: the 4-tap phase has chunks for 12 of them
    c = B["body_s2"]
    assert [p[2] for p in G.phases(c, "dgrad")] == [9, 6, 6, 4]
    assert G.last_split_chunks(c, "dgrad", c.plans["dgrad"][0]) == (2, 2) and 4 * (192 // 32) // 2 == 12 < 27
    # a phase with no pixels: the odd output rows of a one-row input
    ph = G.phases(B["tconv_h1"], "fwd")
    assert [p[0] for p in ph] == [1, 1, 0, 0] and all(p[1] > 0 for p in ph)
    # a last K split shorter than the others
    c = B["k5_c32"]
    assert G.chunks(c, "fwd", c.plans["fwd"][0]) == 25 and G.last_split_chunks(c, "fwd", c.plans["fwd"][0]) == (3, 1)
    # a last 256-row tile that is partial, on 32 tiles (the fewest that take the DMA kernels)
    ho, wo = G.out_hw(B["dma_k3"])
    assert -(-ho * wo // 256) == 32 and ho * wo % 256 == 164
    # four phases of 64 tiles each, none of them whole
    assert [-(-h * w // 256) for h, w, t in G.phases(B["dma_tconv_op0"], "fwd")] == [64, 64, 64, 64]
    assert all(h * w % 256 for h, w, t in G.phases(B["dma_tconv_op0"], "fwd")[1:])
    # the 128-row tiles start at 65,536 pixels; a partial 64-row tile that crosses images
    assert all(B[n].h * B[n].w == 65536 for n in ("tile128_cout384", "gather_tile128"))
    c = B["body_n3_ragged"]
    assert c.n * G.out_hw(c)[0] * G.out_hw(c)[1] == 180 and (G.out_hw(c)[0] * G.out_hw(c)[1]) % 64
    # column tiles with padding: 136 -> 192 columns (8 of the last 64 valid), 10 -> 32, 40 -> 64
    assert -(-136 // 64) * 64 - 136 == 56
    # the tconv_few kernels: three column segments of 128 with a ragged last one; pad 6 past the 5-pixel halo
    assert B["t_few_w300"].w == 300 > 2 * 128 and 300 % 128 and B["t_few_pad6"].p == 6
    # ig_reduce_kernel on both detours' sides: 10 channels, 75 columns
    c = B["t_col2im_c224"]
    assert G.gemm_cout(c, "fwd", c.plans["fwd"][0]) == 75
    assert G.reduce_kernel(c, "fwd", c.plans["fwd"][0]) == "ig_reduce"
    assert G.reduce_kernel(B["cout10"], "fwd", B["cout10"].plans["fwd"][0]) == "ig_reduce"
    for name, ks in (("k1_c128", 2), ("k1_c192", 3), ("k1_c256", 4), ("k2_c128", 8)):
        assert G.reduce_kernel(B[name], "fwd", B[name].plans["fwd"][0]) == "ig_reduce4<%d>" % ks


def test_bf16_runs_at_one_split_where_fp32_takes_three():
    for name in ("k1_c32", "k1_c128", "k1_c256"):
        p = G.BY_NAME[name].plans["dgrad"]
        assert (p[0]["ksplit"], p[1]["kernel"], p[1]["ksplit"]) == (3, "ig_bf16", 1)


@pytest.mark.parametrize("op", G.OPS)
@pytest.mark.parametrize("name", G.MISALIGNED)
def test_misaligned_input_plans_no_16_byte_loads(name, op):
    """The fast kernels read their input 16 bytes at a time (float4 loads, global_load_lds_dwordx4).  An input
    whose base or whose pixel strides are not 16-byte aligned must plan the gather form, which loads element by
    element: channels [1 : C + 1] of C + 8 (base off by 4 bytes) and channels [: C] of C + 1 (pixel stride odd).
    Compact, the same operands plan the vector-load and DMA kernels."""
    c = G.BY_NAME[name]
    out = G.make_output(c, op)[1]
    assert any(p["kernel"] in ("ig_split_dma", "ig_bf16_dma", "ig_split", "ig_bf16") for p in c.plans[op])
    assert all(p["kernel"] in VEC16 for p in c.plans[op])
    for view in G.CHAN_VIEWS:
        inp = G.make_input(c, op, view)
        assert inp.stride(1) == 1
        if view == "chan8":
            assert inp.data_ptr() % 16 == 4 and all(s % 4 == 0 for s in inp.stride()[2:] + inp.stride()[:1])
        else:
            assert inp.data_ptr() % 16 == 0 and inp.stride(3) % 4 == 1
        for m in G.MATHS:
            p = G.plan_of(c, op, inp, out, m)
            assert p["kernel"] == "ig_fp32_gather", (view, m, p)
            assert p == G.plan_of(c, op, inp, out, 0), (view, m)


def test_misaligned_input_of_the_detours():
    """The few-channel outputs of a transposed gather: the col2im detour runs the fast GEMM kernels on x and the
    tconv_few kernels read x by 16 bytes, so a misaligned x takes neither; the few-channel inputs of a direct
    gather are read element by element (edge_conv, im2col), whatever their alignment."""
    from image_compression_amd import _lib
    for name, op in (("t_col2im_c6", "fwd"), ("t_few_rows", "fwd"), ("edge_image", "dgrad")):
        c = G.BY_NAME[name]
        inp, out = G.make_input(c, op, "chan8"), G.make_output(c, op)[1]
        for m in G.MATHS:
            assert G.plan_of(c, op, inp, out, m)["kernel"] == "ig_fp32_gather", (name, m)
    # a compact dy at a base off by 4 bytes: tconv_few_run refuses it, so it is not planned
    c = G.BY_NAME["edge_image"]
    dy, dx = G.make_input(c, "dgrad"), G.make_output(c, "dgrad")[1]
    off = torch.empty(dy.numel() + 1)[1:].view(dy.permute(0, 2, 3, 1).shape).permute(0, 3, 1, 2)
    assert off.stride() == dy.stride() and off.data_ptr() % 16 == 4
    assert G.plan_of(c, "dgrad", dy, dx, 0)["kernel"] == "tconv_few_rows"
    assert G.plan_of(c, "dgrad", off, dx, 0)["kernel"] == "ig_fp32_gather"
    # an NCHW image off alignment keeps the edge kernel and the im2col detour
    for name in ("edge_image", "col_cout96"):
        c = G.BY_NAME[name]
        x, y = G.make_input(c, "fwd"), G.make_output(c, "fwd")[1]
        xo = torch.empty(x.numel() + 1)[1:].view(x.shape)
        assert xo.data_ptr() % 16 == 4
        for m in G.MATHS:
            assert G.plan_of(c, "fwd", xo, y, m) == c.plans["fwd"][m], (name, m)
    # the same through a raw descriptor with a null base (a workspace query without the tensor): aligned
    c = G.BY_NAME["dma_k3"]
    x, y = G.make_input(c, "fwd"), G.make_output(c, "fwd")[1]
    ax, ay = _lib.act(x), _lib.act(y)
    ax.data = None
    assert _lib.plan("conv2d_fwd", ax, ay, c.k, c.s, c.p, 2)["kernel"] == "ig_split_dma"


def test_wide_column_rows_take_the_gather_form():
    """The im2col buffer has rows of at most 128 columns (csrc/im2col.hip).  At most 8 input channels with more
    (tap, channel) pairs than that (5 x 5 taps of 6 to 8 channels) were planned as im2col_gemm and refused by the
    run; they plan, and run, the gather form on the input itself."""
    from image_compression_amd import _lib
    c = G.BY_NAME["t_col2im_c6"]
    assert c.k * c.k * c.cout == 150 > 128 and c.plans["dgrad"][0]["kernel"] == "ig_fp32_gather"
    c = G.BY_NAME["col_c8"]
    assert c.k * c.k * c.cin == 72 and c.plans["fwd"][0]["kernel"] == "im2col_gemm"
    for ch, want in ((5, "im2col_gemm"), (6, "ig_fp32_gather"), (8, "ig_fp32_gather")):
        x, y = torch.empty(1, ch, 12, 12), torch.empty(1, 64, 6, 6).contiguous(memory_format=G.CL)
        assert _lib.plan("conv2d_fwd", x, y, 5, 2, 2, 0)["kernel"] == want, ch
        # the weight gradient's column buffer has the same rows
        assert _lib.plan("conv2d_wgrad", x, y, 5, 2, 2, 0)["im2col"] == int(want == "im2col_gemm"), ch


def test_plan_query_sees_the_tensors_own_pointer():
    """_lib.plan passes the tensor's data pointer, so the query plans what the run, given the same tensor, runs."""
    from image_compression_amd import _lib
    t = torch.empty(2, 8, 3, 3)[:, 1:5]
    assert _lib.act(t).data == t.data_ptr() and t.data_ptr() != t.untyped_storage().data_ptr()
