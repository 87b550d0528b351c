"""Which weight-gradient kernel each case of wgrad_cases.CASES launches, from the library's plan query
(ic_conv_plan launches nothing, so this runs without a GPU): every case, compact and in each view the GPU
test runs, in the four math modes, must plan what the table says; the restated pixel split must be the
library's and the restated sub-kernel the one the case names; and the table must reach every launch path of
csrc/wgrad.hip and the detours of csrc/conv_api.hip."""
import pytest
import torch

import wgrad_cases as W

IDS = [c.name for c in W.CASES]


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_plan_is_the_tables(case):
    for view in ("compact",) + tuple(case.views):
        x, dy = W.make_operands(case, view, values=False)
        for math in W.MATHS:
            got = W.plan_of(case, x, dy, math)
            assert got == W.expected_plan(case, math), (view, math, got)
            assert W.restate_nsplit(case, math)[0] == got["nsplit"], (view, math, got)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_sub_kernel_is_the_cases(case):
    """The kernel behind wg_split / wg_bf16 by the restated wg_x3_launch (its pps cross-checked above)."""
    assert W.split_sub(case) == case.sub
    assert (case.sub is not None) == (case.kern[2] == W.SP)
    assert (case.kern[1] == W.BF) == (case.sub in W.BF16_SUBS)
    if not W.is_edge(case):
        assert case.kern[3] == (W.BF if case.kern[1] == W.BF else case.kern[2])
    for math in W.MATHS:
        assert W.runs_split_family(case, math) == (case.kern[math] in (W.SP, W.BF))


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_fallback_takes_the_fallen_to_launch(case):
    """Where math 1 or 3 cannot take bf16 operands the launch is the one of math 0 or 2, pixel split included
    (the GPU test asserts the results bitwise equal)."""
    x, dy = W.make_operands(case, "compact", values=False)
    plans = [W.plan_of(case, x, dy, m) for m in W.MATHS]
    if case.kern[1] not in (W.BF, W.EB):
        assert plans[1] == plans[0]
        assert plans[3] == plans[2]


def test_table_reaches_every_path():
    reached = set().union(*(W.paths(c) for c in W.CASES))
    assert not (W.REQUIRED_PATHS - reached), sorted(W.REQUIRED_PATHS - reached)
    # the cases the two-level reduce was written for
    assert max(c.ns[0] for c in W.CASES) > 32 and W.BY_NAME["k1_two_groups"].ns == (64, 64)
    # a row-fast map 64 wide with splits that start in mid row
    c = W.BY_NAME["x3d_w64_midrow"]
    assert W.gemm(c)["Wg"] == 64 and W.restate_nsplit(c, 2)[1] % 64 != 0
    # a 32-pixel step of the SEG16 form that spans two images: 16-wide rows, an odd row count per image
    c = W.BY_NAME["x3d16_s2"]
    assert W.gemm(c)["Wg"] == 16 and W.gemm(c)["Hg"] % 2 == 1 and c.n > 1


def test_column_buffer_plan_ignores_x_alignment():
    """The few-channel detour runs the GEMM on the column buffer in the workspace, so the plan is the same
    whatever X's own pointer: a 3-channel image view with a base 4 bytes off a 16-byte boundary plans
    wg_ldsdma, as it runs, and not wg_fp32."""
    from image_compression_amd import _lib
    case = W.BY_NAME["col_cout96"]
    x, dy = W.make_operands(case, "compact", values=False)
    big = torch.empty(x.numel() + 1)
    xv = big[1:].view(x.shape)
    assert xv.data_ptr() % 16 == 4 and xv.stride() == x.stride()
    for math in W.MATHS:
        assert W.plan_of(case, xv, dy, math) == W.plan_of(case, x, dy, math) == W.expected_plan(case, math)
    # the same through a raw descriptor, as tests/test_abi.py queries
    ho, wo = W.out_hw(case)
    g = _lib.ICAct(256, case.n, case.cout, ho, wo, case.cout * ho * wo, 1, wo * case.cout, case.cout)
    for base in (256, 260):
        a = _lib.ICAct(base, case.n, 3, case.h, case.w, 3 * case.h * case.w, case.h * case.w, case.w, 1)
        assert _lib.plan("conv2d_wgrad", a, g, case.k, case.s, case.p, 0)["kernel"] == "wg_ldsdma"


def test_channel_slice_is_the_route_to_wg_fp32():
    """The channel-sliced x (rows 16-byte aligned, base off by 4 bytes) plans wg_fp32 at both tiles; the same
    values compact plan the LDS-DMA kernel (fewer than 128 channels) or the split family."""
    for name, bn in (("fp32_chan192", 192), ("fp32_chan64", 64)):
        c = W.BY_NAME[name]
        x, dy = W.make_operands(c, "compact", values=False)
        assert x.data_ptr() % 16 == 4 and x.stride(1) == 1 and all(s % 4 == 0 for s in x.stride()[2:])
        assert W.plan_of(c, x, dy, 0)["kernel"] == "wg_fp32" and W.plan_of(c, x, dy, 0)["bn"] == bn
        xc = torch.empty(x.shape).contiguous(memory_format=torch.channels_last)
        assert W.plan_of(c, xc, dy, 0)["kernel"] == "wg_ldsdma"
        assert W.plan_of(c, xc, dy, 2)["kernel"] == ("wg_split" if bn == 192 else "wg_ldsdma")


@pytest.mark.parametrize("C,n,h,w,fmt", W.GDN_CASES)
def test_gdn_cases_plan_the_gemm_path(C, n, h, w, fmt):
    from image_compression_amd import _lib
    x = torch.empty(n, C, h, w)
    x = x.contiguous(memory_format=torch.channels_last) if fmt == "cl" else x
    assert _lib.plan("gdn_bwd", x)["kernel"] == "gdn_gemm"


def test_gdn_cases_reach_the_two_level_reduce():
    ns = {c[:4]: W.gdn_nsplit(*c) for c in W.GDN_CASES}
    assert ns[(96, 2, 33, 33)] == 35 and ns[(96, 2, 32, 48)] > 32      # gather map / row-fast map, G = 2
    assert 33 % 16 != 0 and 48 % 16 == 0
