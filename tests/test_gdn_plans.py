"""Which GDN / IGDN kernel each case of gdn_cases.CASES launches, from the library's plan query (ic_conv_plan
launches nothing, so this runs without a GPU): every case, both directions, in the four math modes must plan what
gdn_cases.expected_plan says; the table must reach every kernel name and every template instantiation the
dispatcher of csrc/gdn_fused.hip launches; and the tiles per block the table's comments quote are computed."""
import pytest
import torch

import gdn_cases as G


def _x(c):
    n, h, w = c.shape
    return G.make(c, torch.empty(n, c.C, h, w))


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_plan_is_the_tables(case):
    x = _x(case)
    for d in G.DIRS:
        for m in G.MATHS:
            assert G.plan_of(d, x, m) == G.expected_plan(case, d, m), (case.name, d, m)


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_layouts_are_what_the_names_say(case):
    x = _x(case)
    n, h, w = case.shape
    assert x.shape == (n, case.C, h, w)
    if case.layout == "cl_off4":
        assert x.data_ptr() % 16 == 4 and x.stride() == (h * w * case.C, 1, w * case.C, case.C)
    elif case.layout == "cl":
        assert x.data_ptr() % 16 == 0 and x.is_contiguous(memory_format=G.CL) and x.stride(1) == 1
    else:
        assert x.is_contiguous() and (x.stride(1) != 1 or h * w == 1)


def test_fallen_to_modes_plan_the_same_kernel():
    """A math mode that repeats another's launch (the GPU test asserts the results bitwise equal) plans its kernel;
    math 1 is the asymmetric one: an fp32 forward, and at C = 192 a bf16 backward."""
    for c in G.CASES:
        for d in G.DIRS:
            for m in G.MATHS:
                b = G.falls_to(c, d, m)
                if b is not None:
                    assert G.expected_plan(c, d, m) == G.expected_plan(c, d, b), (c.name, d, m, b)
        assert G.expected_plan(c, "fwd", 1) == G.expected_plan(c, "fwd", 0)
    c = G.BY_NAME["c192_p105"]
    assert [G.expected_plan(c, "fwd", m) for m in G.MATHS] == [G.FUSED, G.FUSED, G.FSPLIT, G.FBF16]
    assert [G.expected_plan(c, "bwd", m) for m in G.MATHS] == [G.FUSED, G.FBF16, G.FSPLIT, G.FBF16]
    for name in ("c64_p105", "c128_p105"):   # the split forward off C = 192 is the GEMM's; the backward stays fused
        c = G.BY_NAME[name]
        assert [G.expected_plan(c, "fwd", m) for m in G.MATHS] == [G.FUSED, G.FUSED, G.GEMM, G.GEMM]
        assert [G.expected_plan(c, "bwd", m) for m in G.MATHS] == [G.FUSED] * 4
        assert G.split_gemm(c, 2) and G.split_gemm(c, 3) and not G.split_gemm(c, 1)
    # the split GEMM forward: the fast form only
    assert [n for n in G.IDS if G.split_gemm(G.BY_NAME[n], 2) and G.BY_NAME[n].C not in (64, 128)] == ["c96_cl", "c320_cl"]
    assert not G.split_gemm(G.BY_NAME["c192_off4"], 2) and not G.split_gemm(G.BY_NAME["c64_n2_1x1"], 2)


def test_table_reaches_every_kernel_and_instantiation():
    names, inst = set(), set()
    for c in G.CASES:
        for d in G.DIRS:
            for m in G.MATHS:
                names.add(G.expected_plan(c, d, m))
                for inv in (False, True):
                    for v in G.VARIANTS:
                        inst.add(G.instantiation(c, d, m, inv, v))
                if d == "bwd" and G.expected_plan(c, d, m) != G.GEMM:
                    inst.add("gdn_slab_reduce_kernel")      # every fused backward ends in it
    assert names == G.KERNEL_NAMES
    inst.discard(None)
    assert inst == set(G.INSTANTIATIONS), (sorted(set(G.INSTANTIATIONS) - inst), sorted(inst - set(G.INSTANTIATIONS)))
    # DMA_B (group B issues the next tile's DMA) is on for C < 192 and the bf16 kernels, off for fp32 at C = 192: each
    # side has a case whose blocks run more than one tile
    for name, m in (("c64_p4225", 0), ("c128_p4225", 0), ("c192_p4225", 0), ("c192_p4225", 1), ("c192_p4225", 2)):
        assert G.tiling(G.BY_NAME[name], "bwd", m).per_block == (1, 2), name


def test_tiles_per_block_are_what_the_table_says():
    B = G.BY_NAME
    T = G.Tiling
    # one row, a tile short, exact, one over (16-row tiles: the fp32 forward and every backward)
    for p, tiles, last in ((1, 1, 1), (15, 1, 15), (16, 1, 16), (17, 2, 1), (31, 2, 15), (33, 3, 1)):
        for C in (64, 128, 192):
            c = B[f"c{C}_p{p}"]
            assert G.tiling(c, "fwd", 0) == T(16, tiles, tiles, (1, 1), last)
            assert G.tiling(c, "bwd", 0) == T(16, tiles, tiles, (1, 1), last)
    # the 32-row tiles of gdn_fwd_x3s_kernel
    for p, tiles, last in ((1, 1, 1), (31, 1, 31), (33, 2, 1), (105, 4, 9)):
        for m in (2, 3):
            assert G.tiling(B[f"c192_p{p}"], "fwd", m) == T(32, tiles, tiles, (1, 1), last)
    # 4225: the backward's 265 tiles on 256 blocks, the last of one row; the forwards one tile per block
    for C in (64, 128, 192):
        c = B[f"c{C}_p4225"]
        assert G.tiling(c, "bwd", 0) == T(16, 256, 265, (1, 2), 1) and 265 - 256 == 9
        assert G.tiling(c, "fwd", 0) == T(16, 265, 265, (1, 1), 1)
    assert G.tiling(B["c192_p4225"], "bwd", 3) == T(16, 256, 265, (1, 2), 1)
    assert G.tiling(B["c192_p4225"], "fwd", 3) == T(32, 133, 133, (1, 1), 1)
    # 16425: both buffers of every persistent loop are reused
    for C in (64, 128, 192):
        c = B[f"c{C}_p16425"]
        assert G.tiling(c, "fwd", 0) == T(16, 512, 1027, (2, 3), 9)
        assert G.tiling(c, "bwd", 0) == T(16, 256, 1027, (4, 5), 9)
    for m in (2, 3):
        assert G.tiling(B["c192_p16425"], "fwd", m) == T(32, 256, 514, (2, 3), 9)
        assert G.tiling(B["c192_p16425"], "bwd", m) == T(16, 256, 1027, (4, 5), 9)
    # 24648: the three x buffers and the two plane sets of gdn_fwd_x3s_kernel wrap (more than three tiles)
    for m in (2, 3):
        assert G.tiling(B["c192_p24648"], "fwd", m) == T(32, 256, 771, (3, 4), 8)
    # off the fused kernels
    for name in ("c3_nchw", "c10_cl", "c48_cl", "c96_cl", "c320_cl", "c192_nchw", "c192_off4"):
        assert all(G.tiling(B[name], d, m) is None for d in G.DIRS for m in G.MATHS)
    assert G.tiling(B["c64_p105"], "fwd", 2) is None and G.tiling(B["c64_p105"], "bwd", 2) is not None


def test_size_one_strides_do_not_count():
    """A contiguous (n, C, 1, 1) tensor keeps strides (C, 1, 1, 1) as channels-last (what functional._cl hands the
    op); the stride of a dimension of size 1 multiplies no index, so such a tensor is NHWC-dense and takes the fused
    kernels (it planned gdn_gemm, whose forward refuses to leave norm out: the C3 layer raised)."""
    for C, n in ((192, 2), (64, 2), (192, 1)):
        x = torch.empty(n, C, 1, 1).contiguous(memory_format=G.CL)
        assert x.stride()[1:] == (1, 1, 1)
        assert [G.plan_of("fwd", x, m) for m in G.MATHS] == \
            [G.FUSED, G.FUSED, G.FSPLIT if C == 192 else G.GEMM, G.FBF16 if C == 192 else G.GEMM]
        assert G.plan_of("bwd", x, 3) == (G.FBF16 if C == 192 else G.FUSED)
    # the dimensions above size 1 still have to be dense: a row stride with a gap, a channel slice
    x = torch.empty(2, 4, 6, 192).permute(0, 3, 1, 2)[:, :, :, :5]
    assert G.plan_of("fwd", x, 0) == G.GEMM and G.plan_of("bwd", x, 0) == G.GEMM
    x = torch.empty(2, 1, 1, 256).permute(0, 3, 1, 2)[:, :192]
    assert x.stride(0) == 256 and G.plan_of("fwd", x, 0) == G.GEMM
    x = torch.empty(1, 1, 5, 256).permute(0, 3, 1, 2)[:, :192]
    assert G.plan_of("bwd", x, 0) == G.GEMM
