"""ig_kernel_x3d's chunk loop at its edges: the split A fragments of chunk c + 1 may be prepared during
chunk c (IG_X3D_PRESPLIT), so the first chunk, the last chunk and the shortest chunk ranges each take a
path of their own.  Every case asserts through the plan that the DMA tiles run (ig_split_dma), holds the
result to the rule of tests/test_dma_gpu.py (fp64 torch at 1e-4, error <= 1.5 x the native fp32 kernel's)
and asserts that a second identical launch is bitwise equal.

Shapes are the smallest the planner still gives the DMA tiles (found with _lib.plan):
  * split K: the 5 x 5 stride-2 192 -> 192 conv at 8 x 64^2 (ksplit 8: ranges of 19 chunks, the last 17),
    8 x 128^2 (ksplit 2: 75 + 75) and 13 x 50^2 (ragged rows, ksplit 8).  Its input gradient is a four-phase
    map, which the planner never splits in K on these tiles: it takes them at 8 x 128^2 only (512 tiles); at
    the two smaller shapes it runs ig_split, is still checked, and the split-K gradient on DMA tiles is the
    transposed conv's (a one-phase stride-2 conv) at 2, 3 and 4 images of 128^2 (ksplit 8, 6, 4).
  * the shortest ranges: a 3 x 3 stride-1 192 -> 192 conv has 54 chunks; its largest ksplit is 8 (32 tiles,
    8 x 32^2), ranges of 7 chunks and a last one of 5.  No reachable shape leaves a split empty: ig_plan
    sets ksplit = ceil(chunks / ceil(chunks / ksplit)), so (ksplit - 1) * kcps < chunks always, and maps
    with several phases are not split.  Shorter ranges come from fewer input channels: 1 x 1 convs from
    32 / 64 / 96 channels run ranges of 1 / 2 / 3 chunks (no loop trip, one, two), 3 x 3 convs from them
    ranges of 3 chunks under ksplit 3 / 6 / 7.
  * the four phases (9 / 6 / 6 / 4 taps): the transposed conv at 4 x 64^2, the smallest batch with 256 tiles,
    with and without bias + ReLU in the kernel's own epilogue.
  * a partial last tile without split K: 18 x 122^2 (261 full tiles and one of 162 rows).
GPU only."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
SPLIT, NATIVE = 2, 0  # IC_MATH_*


def _r(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _act(*shape, seed):
    return _r(*shape, seed=seed).contiguous(memory_format=CL)


def _plan(op, a, b, k, s, p):
    from image_compression_amd import _lib
    q = _lib.plan(op, a, b, k, s, p, SPLIT)
    return q["kernel"], q["bm"], q["ksplit"]


def _check(run, ref, name):
    """run(math) -> tensor: the split kernel against fp64 and the native kernel, and twice bitwise."""
    got = run(SPLIT)
    again = run(SPLIT)
    assert torch.equal(got, again), f"{name}: two identical launches differ"
    del again
    got, native, ref = got.double().cpu(), run(NATIVE).double().cpu(), ref.cpu()
    assert_close(got, ref, 1e-4, name)
    es, en = rel_err(got, ref), rel_err(native, ref)
    print(f"{name}: DMA split {es:.2e} native fp32 {en:.2e}")
    assert es <= 1.5 * en + 1e-8, (name, es, en)


def _conv(n, cin, h, k, s, p, ksplit, relu=False, dgrad=None, seed=0):
    """Forward (bias, optional ReLU) on DMA tiles with this ksplit; dgrad: None, or whether the input
    gradient takes the DMA tiles too (it is checked either way)."""
    from image_compression_amd import _lib
    ops = _lib.ops()
    x = _act(n, cin, h, h, seed=seed + 1)
    w = _r(192, cin, k, k, seed=seed + 2, scale=0.03)
    b = _r(192, seed=seed + 3, scale=0.1)
    ho = (h + 2 * p - k) // s + 1
    y = torch.empty(n, 192, ho, ho, device=DEV).contiguous(memory_format=CL)
    assert _plan("conv2d_fwd", x, y, k, s, p) == ("ig_split_dma", 256, ksplit)
    yr = F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p)
    _check(lambda m: ops.conv2d_fwd(x, w, b, s, p, int(relu), m), yr.relu() if relu else yr, "y")
    del yr
    if dgrad is None:
        return
    gy = _act(n, 192, ho, ho, seed=seed + 4)
    assert (_plan("conv2d_dgrad", gy, x, k, s, p)[0] == "ig_split_dma") == dgrad
    dxr = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), stride=s, padding=p)
    _check(lambda m: ops.conv2d_dgrad(gy, w, x, s, p, m), dxr, "dx")


@pytest.mark.parametrize("n,h,ksplit,dgrad_dma", [(8, 64, 8, False), (8, 128, 2, True), (13, 50, 8, False)])
def test_split_k_ranges(n, h, ksplit, dgrad_dma):
    _conv(n, 192, h, 5, 2, 2, ksplit, dgrad=dgrad_dma, seed=10)


def test_shortest_split_ranges():
    # 54 chunks under the largest ksplit the planner gives them: 7 x 7 chunks and a last range of 5
    _conv(8, 192, 32, 3, 1, 1, 8, dgrad=True, seed=20)


@pytest.mark.parametrize("cin,ksplit3", [(32, 3), (64, 6), (96, 7)])
def test_one_two_three_chunk_ranges(cin, ksplit3):
    _conv(8, cin, 32, 1, 1, 0, 1, seed=30)              # cin / 32 chunks, unsplit
    _conv(8, cin, 32, 3, 1, 1, ksplit3, relu=True, seed=40)  # ranges of 3 chunks, split


@pytest.mark.parametrize("epilogue", [False, True])
def test_four_phases(epilogue):
    from image_compression_amd import _lib
    ops = _lib.ops()
    n, h = 4, 64
    x = _act(n, 192, h, h, seed=51)
    w = _r(192, 192, 5, 5, seed=52, scale=0.03)
    b = _r(192, seed=53, scale=0.1) if epilogue else None
    y = torch.empty(n, 192, 2 * h, 2 * h, device=DEV).contiguous(memory_format=CL)
    assert _plan("conv_transpose2d_fwd", x, y, 5, 2, 2) == ("ig_split_dma", 256, 1)
    yr = F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=2,
                            output_padding=1)
    _check(lambda m: ops.conv_transpose2d_fwd(x, w, b, 2, 2, 1, int(epilogue), m), yr.relu() if epilogue else yr, "y")


# the transposed conv's input gradient: a one-phase stride-2 conv onto 64^2, K split 8 / 6 / 4 ways
@pytest.mark.parametrize("n,ksplit", [(2, 8), (3, 6), (4, 4)])
def test_tconv_dgrad_split_k(n, ksplit):
    from image_compression_amd import _lib
    ops = _lib.ops()
    x = _act(n, 192, 64, 64, seed=61)
    w = _r(192, 192, 5, 5, seed=62, scale=0.03)
    gy = _act(n, 192, 128, 128, seed=63)
    assert _plan("conv_transpose2d_dgrad", gy, x, 5, 2, 2) == ("ig_split_dma", 256, ksplit)
    dxr = F.conv2d(gy.double(), w.double(), None, stride=2, padding=2)
    _check(lambda m: ops.conv_transpose2d_dgrad(gy, w, x, 2, 2, m), dxr, "dx")


def test_partial_last_tile():
    _conv(18, 192, 122, 5, 2, 2, 1, seed=70)
