"""The forward / input-gradient case table shared by test_igemm_plans.py (CPU: which kernel each case launches,
from the library's plan query) and test_igemm_gpu.py (parity of y / dx against fp64).

Each case is one geometry and stands for two ops: the forward (conv2d_fwd or conv_transpose2d_fwd) and the
input gradient of the same layer (conv2d_dgrad or conv_transpose2d_dgrad), which is the other gather: a
convolution's forward and a transposed convolution's input gradient are the direct gather (one phase, stride s),
a transposed convolution's forward and a convolution's input gradient the transposed one (s * s sub-pixel phases
of stride 1).  csrc/igemm.hip chooses among its kernels by the GEMM's Cout, the pixel count, Cin, the layout,
alignment and compactness of the input and the number of phases; csrc/conv_api.hip adds the image-edge kernels,
the two tconv_few kernels and the im2col / col2im detours.  The plan fields kernel, bm, bn, ksplit, im2col and
variant name the instantiation completely, but for the split-K reduce kernel, which goes by ksplit and the
GEMM's Cout % 4: that rule is restated here once (reduce_kernel).

A plan is written "kernel[@BMxBN] ksplit [col] [v1]" under the tile of the line; four of them, " / "-separated,
are math 0 (fp32) / 1 (bf16 operands) / 2 (split arithmetic) / 3 (bf16, else split); one stands for all four."""
import collections

import torch
import torch.nn.functional as F

CL = torch.channels_last
MATHS = (0, 1, 2, 3)
OPS = ("fwd", "dgrad")
PLAN_FIELDS = ("kernel", "bm", "bn", "ksplit", "im2col", "variant")

IG_KERNELS = ("ig_fp32", "ig_fp32_gather", "ig_bf16", "ig_split", "ig_split_bf16", "ig_split_dma", "ig_bf16_dma")
GEMM_KERNELS = IG_KERNELS + ("im2col_gemm", "gemm_col2im")     # ig_plan's tile and K split; ig_run's reduce
BF16_KERNELS = ("ig_bf16", "ig_split_bf16", "ig_bf16_dma", "edge_conv_bf16", "tconv_few_rows_bf16")
DMA_KERNELS = ("ig_split_dma", "ig_bf16_dma")

Case = collections.namedtuple("Case", "name tr n cin h w cout k s p op xfmt plans halo yview relu")

# the image-edge kernels' four modes (csrc/edge.hip): variant 1 is split arithmetic or bf16 operands
EDGE = "edge_conv 1 / edge_conv_bf16 1 v1 / edge_conv 1 v1 / edge_conv_bf16 1 v1"
FEW_ROWS = "tconv_few_rows 1 / tconv_few_rows_bf16 1 v1 / tconv_few_rows 1 v1 / tconv_few_rows_bf16 1 v1"


def _plans(spec):
    tile, text = spec
    ents = [e.strip() for e in text.split("/")]
    ents = ents * 4 if len(ents) == 1 else ents
    assert len(ents) == 4, spec
    out = []
    for e in ents:
        tok = e.split()
        kern, _, t = tok[0].partition("@")
        bm, bn = (int(v) for v in (t or tile).split("x"))
        assert set(tok[2:]) <= {"col", "v1"}, e
        out.append(dict(kernel=kern, bm=bm, bn=bn, ksplit=int(tok[1]), im2col=int("col" in tok[2:]),
                        variant=int("v1" in tok[2:])))
    return tuple(out)


def _case(name, tr, n, cin, h, w, cout, k, s, p, op=0, *, fwd, dgrad, fwd_halo=None, dgrad_halo=None, xfmt=None,
          yview=False, relu=False):
    """fwd / dgrad: the plans of the two ops on compact operands; *_halo: the plans with the op's input as the
    interior of a larger tensor, where they differ (the kernels that want a compact input); xfmt: x's layout where
    it is not the one of its channel count; yview: the case also runs into an output view through the C ABI;
    relu: the forward runs with the ReLU epilogue."""
    plans = {"fwd": _plans(fwd), "dgrad": _plans(dgrad)}
    halo = {"fwd": _plans(fwd_halo) if fwd_halo else plans["fwd"],
            "dgrad": _plans(dgrad_halo) if dgrad_halo else plans["dgrad"]}
    return Case(name, bool(tr), n, cin, h, w, cout, k, s, p, op, xfmt or act_format(cin), plans, halo, yview, relu)


def _conv(name, *a, **kw):
    return _case(name, False, *a, **kw)


def _tconv(name, *a, **kw):
    return _case(name, True, *a, **kw)


def act_format(c):
    """csrc/torch_ops.cpp act_format: the layout the ops give an output of c channels."""
    return "cl" if c >= 32 else "nchw"


# n, cin, h, w, cout, k, stride, pad[, output padding]
CASES = [
    # ---- the 64 x 192 tile (Cout % 192 == 0, fewer than 65,536 pixels): ig_kernel, ig_kernel_x3s with three
    # products (ig_split) and with one (ig_split_bf16)
    # dgrad: four phases of 9 / 6 / 6 / 4 taps; the splits past a phase's chunks add zeros
    _conv("body_s2", 2, 192, 16, 16, 192, 5, 2, 2, yview=True, relu=True,
          fwd=("64x192", "ig_fp32 30 / ig_split_bf16 30 / ig_split 30 / ig_split_bf16 30"),
          dgrad=("64x192", "ig_fp32 27 / ig_split_bf16 27 / ig_split 27 / ig_split_bf16 27")),
    # 180 rows: the last tile partial, tiles cross images
    _conv("body_n3_ragged", 3, 192, 20, 12, 192, 5, 2, 2,
          fwd=("64x192", "ig_fp32 30 / ig_split_bf16 30 / ig_split 30 / ig_split_bf16 30"),
          dgrad=("64x192", "ig_fp32 27 / ig_split_bf16 27 / ig_split 27 / ig_split_bf16 27")),
    # ---- K splits of 1, 2, 3, 4 and 8: no reduce, ig_reduce4_kernel<2 / 3 / 4 / 8>; the input gradients on the
    # 256 x 32 and 128 x 64 tiles, ig_kernel_bf16 at one split where fp32 takes three
    _conv("k1_c32", 1, 32, 9, 7, 192, 1, 1, 0,
          fwd=("64x192", "ig_fp32 1 / ig_fp32 1 / ig_split 1 / ig_split 1"),
          dgrad=("256x32", "ig_fp32 3 / ig_bf16 1 / ig_fp32 3 / ig_bf16 1")),
    _conv("k1_c128", 1, 128, 9, 7, 192, 1, 1, 0, relu=True,
          fwd=("64x192", "ig_fp32 2 / ig_split_bf16 2 / ig_split 2 / ig_split_bf16 2"),
          dgrad=("128x64", "ig_fp32 3 / ig_bf16 1 / ig_split 3 / ig_bf16 1")),
    _conv("k1_c192", 1, 192, 9, 7, 192, 1, 1, 0,
          fwd=("64x192", "ig_fp32 3 / ig_split_bf16 3 / ig_split 3 / ig_split_bf16 3"),
          dgrad=("64x192", "ig_fp32 3 / ig_split_bf16 3 / ig_split 3 / ig_split_bf16 3")),
    _conv("k1_c256", 1, 256, 9, 7, 192, 1, 1, 0,
          fwd=("64x192", "ig_fp32 4 / ig_split_bf16 4 / ig_split 4 / ig_split_bf16 4"),
          dgrad=("128x64", "ig_fp32 3 / ig_bf16 1 / ig_split 3 / ig_bf16 1")),
    _conv("k2_c128", 1, 128, 9, 7, 192, 2, 1, 0, relu=True,
          fwd=("64x192", "ig_fp32 8 / ig_split_bf16 8 / ig_split 8 / ig_split_bf16 8"),
          dgrad=("128x64", "ig_fp32 12 / ig_bf16 6 / ig_split 12 / ig_bf16 6")),
    # 9 splits of 25 chunks: the last split one chunk, ig_reduce4_kernel<0>; Cin % 64 != 0: no bf16 forward
    _conv("k5_c32", 1, 32, 9, 7, 192, 5, 2, 2,
          fwd=("64x192", "ig_fp32 9 / ig_fp32 9 / ig_split 9 / ig_split 9"),
          dgrad=("256x32", "ig_fp32 27 / ig_bf16 9 / ig_fp32 27 / ig_bf16 9")),
    # ---- the 128 x 64 tile (Cout >= 64, Cout % 192 != 0)
    _conv("cout64", 2, 96, 18, 10, 64, 5, 2, 2,                      # Cin % 64 != 0
          fwd=("128x64", "ig_fp32 25 / ig_fp32 25 / ig_split 25 / ig_split 25"),
          dgrad=("128x64", "ig_fp32 9 / ig_bf16 3 / ig_split 9 / ig_bf16 3")),
    # Npad 192: the last column tile has 8 of 64 valid; dgrad: 136 % 32 != 0, the gather form
    _conv("cout136", 1, 64, 9, 11, 136, 3, 1, 1, relu=True,
          fwd=("128x64", "ig_fp32 9 / ig_bf16 3 / ig_split 9 / ig_bf16 3"),
          dgrad=("128x64", "ig_fp32_gather 13")),
    _conv("cout320", 2, 192, 8, 8, 320, 5, 2, 2,
          fwd=("128x64", "ig_fp32 30 / ig_bf16 25 / ig_split 30 / ig_bf16 25"),
          dgrad=("64x192", "ig_fp32 30 / ig_split_bf16 30 / ig_split 30 / ig_split_bf16 30")),
    _conv("cout384_small", 1, 64, 9, 7, 384, 3, 1, 1,                # two column tiles of 192
          fwd=("64x192", "ig_fp32 9 / ig_split_bf16 9 / ig_split 9 / ig_split_bf16 9"),
          dgrad=("128x64", "ig_fp32 27 / ig_bf16 27 / ig_split 27 / ig_bf16 27")),
    # ---- the 128 x 192 tile: 65,536 pixels.  Cout 384: at Cout 192 the split and bf16 modes take the DMA tiles
    _conv("tile128_cout384", 1, 64, 256, 256, 384, 1, 1, 0, relu=True,
          fwd=("128x192", "ig_fp32 1 / ig_bf16 1 / ig_split 1 / ig_bf16 1"),
          dgrad=("128x64", "ig_fp32 1 / ig_bf16 1 / ig_split 1 / ig_bf16 1")),
    # ---- the 256 x 32 tile (Cout < 64): no split kernel; Cout % 4 != 0: ig_reduce_kernel, y NCHW
    _conv("cout10", 1, 64, 9, 11, 10, 3, 1, 1, yview=True,
          fwd=("256x32", "ig_fp32 9 / ig_bf16 3 / ig_fp32 9 / ig_bf16 3"),
          dgrad=("128x64", "ig_fp32_gather 1")),
    _conv("cout40", 1, 64, 9, 11, 40, 3, 1, 1,                       # two column tiles of 32
          fwd=("256x32", "ig_fp32 9 / ig_bf16 3 / ig_fp32 9 / ig_bf16 3"),
          dgrad=("128x64", "ig_fp32_gather 6")),
    # ---- the gather form: Cin % 32 != 0, x not channels-last; at each tile
    _conv("gather_c10", 1, 10, 9, 7, 64, 3, 1, 1, xfmt="cl", relu=True,
          fwd=("128x64", "ig_fp32_gather 1"),
          dgrad=("256x32", "ig_fp32 9 / ig_bf16 3 / ig_fp32 9 / ig_bf16 3")),
    _conv("gather_nchw64", 2, 64, 9, 11, 192, 3, 1, 1, xfmt="nchw",
          fwd=("64x192", "ig_fp32_gather 9"),
          dgrad=("128x64", "ig_fp32 27 / ig_bf16 9 / ig_split 27 / ig_bf16 9")),
    _conv("gather_tile128", 1, 12, 256, 256, 192, 1, 1, 0, xfmt="cl",
          fwd=("128x192", "ig_fp32_gather 1"),
          dgrad=("256x32", "ig_fp32 3 / ig_bf16 1 / ig_fp32 3 / ig_bf16 1")),
    # ---- the all-DMA kernels (Cout 192, at least 32 tiles of 256 rows; 256 tiles with several phases):
    # ig_kernel_x3d (ig_split_dma) and, on a compact x only, ig_kernel_b16d (ig_bf16_dma)
    # 8,100 rows: 32 tiles, the last of 164 rows
    _conv("dma_k3", 1, 64, 90, 90, 192, 3, 1, 1, relu=True,
          fwd=("256x192", "ig_fp32@64x192 9 / ig_bf16_dma 3 / ig_split_dma 6 / ig_bf16_dma 3"),
          dgrad=("128x64", "ig_fp32 14 / ig_bf16 9 / ig_split 14 / ig_bf16 9"),
          fwd_halo=("64x192", "ig_fp32 9 / ig_split_bf16 9 / ig_split_dma@256x192 6 / ig_split_bf16 9")),
    _conv("dma_k1", 1, 64, 90, 90, 192, 1, 1, 0,                     # one split, one chunk per split in bf16
          fwd=("256x192", "ig_fp32@64x192 1 / ig_bf16_dma 1 / ig_split_dma 1 / ig_bf16_dma 1"),
          dgrad=("128x64", "ig_fp32 3 / ig_bf16 1 / ig_split 3 / ig_bf16 1"),
          fwd_halo=("64x192", "ig_fp32 1 / ig_split_bf16 1 / ig_split_dma@256x192 1 / ig_split_bf16 1")),
    # out 90 x 91; the bottom and right taps out of range
    _conv("dma_s2_odd", 1, 64, 179, 181, 192, 5, 2, 2,
          fwd=("256x192", "ig_fp32@64x192 8 / ig_bf16_dma 7 / ig_split_dma 8 / ig_bf16_dma 7"),
          dgrad=("128x64", "ig_fp32 5 / ig_bf16 5 / ig_split 5 / ig_bf16 5"),
          fwd_halo=("64x192", "ig_fp32 8 / ig_split_bf16 8 / ig_split_dma@256x192 8 / ig_split_bf16 8")),
    # out 255 x 255: four phases of 128 / 127 rows and columns, 64 tiles each (the last ones partial), tile remap
    _tconv("dma_tconv_op0", 1, 64, 128, 128, 192, 5, 2, 2, 0, yview=True, relu=True,
           fwd=("256x192", "ig_fp32@64x192 1 / ig_bf16_dma 1 / ig_split_dma 1 / ig_bf16_dma 1"),
           dgrad=("128x64", "ig_fp32 8 / ig_bf16 8 / ig_split 8 / ig_bf16 8"),
           fwd_halo=("64x192", "ig_fp32 1 / ig_split_bf16 1 / ig_split_dma@256x192 1 / ig_split_bf16 1")),
    # dgrad: the four-phase DMA kernels into an odd-sized dx
    _conv("dma_dgrad4_odd", 1, 192, 255, 255, 64, 3, 2, 1,
          fwd=("128x64", "ig_fp32 8 / ig_bf16 7 / ig_split 8 / ig_bf16 7"),
          dgrad=("256x192", "ig_fp32@64x192 1 / ig_bf16_dma 1 / ig_split_dma 1 / ig_bf16_dma 1"),
          dgrad_halo=("64x192", "ig_fp32 1 / ig_split_bf16 1 / ig_split_dma@256x192 1 / ig_split_bf16 1")),
    # ---- transposed convolutions on the GEMM kernels
    _tconv("tconv_body", 2, 192, 8, 8, 192, 5, 2, 2, 1,
           fwd=("64x192", "ig_fp32 27 / ig_split_bf16 27 / ig_split 27 / ig_split_bf16 27"),
           dgrad=("64x192", "ig_fp32 30 / ig_split_bf16 30 / ig_split 30 / ig_split_bf16 30")),
    _tconv("tconv_k3s1", 2, 192, 6, 6, 192, 3, 1, 1, 0, relu=True,
           fwd=("64x192", "ig_fp32 27 / ig_split_bf16 27 / ig_split 27 / ig_split_bf16 27"),
           dgrad=("64x192", "ig_fp32 27 / ig_split_bf16 27 / ig_split 27 / ig_split_bf16 27")),
    # out 13 x 9: phases of 1 / 2 / 2 / 4 taps and of unequal size; the blocks past a phase's tiles return
    _tconv("tconv_k3s2_op0", 2, 64, 7, 5, 192, 3, 2, 1, 0, yview=True,
           fwd=("64x192", "ig_fp32 4 / ig_split_bf16 4 / ig_split 4 / ig_split_bf16 4"),
           dgrad=("128x64", "ig_fp32 27 / ig_bf16 9 / ig_split 27 / ig_bf16 9")),
    _tconv("tconv_k4s2", 2, 64, 7, 5, 64, 4, 2, 1, 0,
           fwd=("128x64", "ig_fp32 4 / ig_bf16 2 / ig_split 4 / ig_bf16 2"),
           dgrad=("128x64", "ig_fp32 16 / ig_bf16 8 / ig_split 16 / ig_bf16 8")),
    # out 1 x 9: the odd-row phases have no pixels
    _tconv("tconv_h1", 2, 64, 1, 5, 192, 3, 2, 1, 0, yview=True, relu=True,
           fwd=("64x192", "ig_fp32 2 / ig_split_bf16 2 / ig_split 2 / ig_split_bf16 2"),
           dgrad=("128x64", "ig_fp32 27 / ig_bf16 9 / ig_split 27 / ig_bf16 9")),
    # the gather form over four phases: one weight pack per phase
    _tconv("tconv_gather_c80", 1, 80, 9, 7, 64, 5, 2, 2, 1,
           fwd=("128x64", "ig_fp32_gather 8"),
           dgrad=("128x64", "ig_fp32 25 / ig_bf16 9 / ig_split 25 / ig_bf16 9")),
    # ---- at most 8 input channels: the image-edge kernel, else im2col and one 1 x 1 GEMM; their input
    # gradients: at most 4 channels the tconv_few kernels (a compact dy), else the GEMM and col2im
    _conv("edge_image", 2, 3, 20, 24, 192, 5, 2, 2, yview=True,
          fwd=("64x192", EDGE), dgrad=("0x3", FEW_ROWS), dgrad_halo=("128x64", "gemm_col2im 3 col")),
    _conv("edge_c1_k5", 1, 1, 9, 7, 128, 5, 2, 2, relu=True,
          fwd=("64x128", EDGE), dgrad=("0x1", FEW_ROWS), dgrad_halo=("256x32", "gemm_col2im 2 col")),
    _conv("edge_c4_k3", 1, 4, 9, 7, 64, 3, 1, 1,                     # stride 1: no tconv_few
          fwd=("64x64", EDGE), dgrad=("256x32", "gemm_col2im 1 col")),
    _conv("edge_c4_k5", 1, 4, 12, 12, 192, 5, 2, 2,                  # 25 taps x 4 channels > 96: no split edge kernel
          fwd=("64x192", "edge_conv 1"), dgrad=("128x64", "gemm_col2im 3 col")),
    _conv("col_cout96", 2, 3, 20, 24, 96, 5, 2, 2, relu=True,        # Cout outside {64, 128, 192}
          fwd=("128x64", "im2col_gemm 1 col"), dgrad=("0x3", FEW_ROWS), dgrad_halo=("128x64", "gemm_col2im 1 col")),
    _conv("col_c8", 2, 8, 12, 12, 64, 3, 2, 1,                       # more than 4 channels
          fwd=("128x64", "im2col_gemm 1 col"), dgrad=("128x64", "gemm_col2im 1 col")),
    # ---- transposed convolutions to at most 4 channels: the input-row kernel (tconv_few_rows; split and bf16
    # forms where Cin % 32 == 0), the output-row kernel (tconv_few) past its halo; their input gradients
    _tconv("t_few_rows", 2, 192, 20, 24, 3, 5, 2, 2, 1,
           fwd=("0x3", FEW_ROWS), dgrad=("64x192", EDGE), fwd_halo=("128x64", "gemm_col2im 3 col")),
    _tconv("t_few_c80", 1, 80, 9, 7, 3, 5, 2, 2, 1, relu=True,
           fwd=("0x3", "tconv_few_rows 1"), dgrad=("128x64", "im2col_gemm 1 col"),
           fwd_halo=("256x32", "ig_fp32_gather 8")),
    _tconv("t_few_c4", 1, 48, 6, 5, 4, 3, 2, 1, 1,
           fwd=("0x4", "tconv_few_rows 1"), dgrad=("256x32", "im2col_gemm 1 col"),
           fwd_halo=("256x32", "ig_fp32_gather 3")),
    _tconv("t_few_k3", 1, 16, 2, 130, 3, 3, 2, 1, 1, xfmt="cl",      # 130 columns: two segments
           fwd=("0x3", "tconv_few_rows 1"), dgrad=("256x32", "im2col_gemm 1 col"),
           fwd_halo=("256x32", "ig_fp32_gather 1")),
    _tconv("t_few_w300", 1, 32, 4, 300, 3, 5, 2, 2, 1, yview=True, relu=True,   # three segments, the last ragged
           fwd=("0x3", FEW_ROWS), dgrad=("256x32", "im2col_gemm 1 col"), fwd_halo=("128x64", "gemm_col2im 1 col")),
    # pad 6 > 5 (out 24 x 24): the only operands that reach tconv_few, the output-row kernel
    _tconv("t_few_pad6", 1, 32, 16, 16, 3, 5, 2, 6, 1,
           fwd=("0x3", "tconv_few 1"), dgrad=("256x32", "im2col_gemm 1 col"), fwd_halo=("128x64", "gemm_col2im 1 col")),
    # the same at input widths past 64 and past 128: tconv_few_kernel<8, 1> and <8, 2> (16 pixels per wave and step)
    _tconv("t_few_pad6_w70", 1, 16, 5, 70, 3, 5, 2, 6, 1, xfmt="cl",
           fwd=("0x3", "tconv_few 1"), dgrad=("256x32", "im2col_gemm 1 col"), fwd_halo=("256x32", "ig_fp32_gather 2")),
    _tconv("t_few_pad6_w130", 1, 16, 5, 130, 3, 5, 2, 6, 1, xfmt="cl", relu=True,
           fwd=("0x3", "tconv_few 1"), dgrad=("256x32", "im2col_gemm 1 col"), fwd_halo=("256x32", "ig_fp32_gather 2")),
    # ---- at most 8 output channels off the tconv_few kernels: one GEMM with N = k * k * Cout, then col2im
    # dgrad: 25 taps x 6 channels = 150 columns, wider than the im2col buffer's 128: the gather form on dy itself
    _tconv("t_col2im_c6", 1, 64, 9, 7, 6, 5, 2, 2, 1,
           fwd=("128x64", "gemm_col2im 1 col"), dgrad=("128x64", "ig_fp32_gather 2")),
    _tconv("t_col2im_c224", 1, 224, 9, 7, 3, 5, 2, 2, 1, yview=True, relu=True,   # 75 columns: ig_reduce_kernel
           fwd=("128x64", "gemm_col2im 3 col"), dgrad=("128x64", "im2col_gemm 1 col")),
    _tconv("t_col2im_s1", 1, 64, 9, 7, 3, 3, 1, 1, 0,
           fwd=("256x32", "gemm_col2im 1 col"), dgrad=("64x64", EDGE)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the cases whose input also runs as a channel slice off 16-byte alignment (test_igemm_plans.py: the alignment rule)
MISALIGNED = ("dma_k3", "tile128_cout384", "body_s2")
CHAN_VIEWS = ("chan8", "chan1")
VIEWS = ("compact", "halo") + CHAN_VIEWS


# ---------------------------------------------------------------- geometry
def out_hw(c):
    if c.tr:
        return ((c.h - 1) * c.s - 2 * c.p + c.k + c.op, (c.w - 1) * c.s - 2 * c.p + c.k + c.op)
    return ((c.h + 2 * c.p - c.k) // c.s + 1, (c.w + 2 * c.p - c.k) // c.s + 1)


def weight_shape(c):
    return (c.cin, c.cout, c.k, c.k) if c.tr else (c.cout, c.cin, c.k, c.k)


def op_name(c, op):
    return ("conv_transpose2d_" if c.tr else "conv2d_") + op


def io(c, op):
    """(input shape, input layout, output shape, output layout) of the op: the forward reads x and writes y, the
    input gradient reads dy and writes dx.  The outputs' layouts are the ones the torch ops allocate: by channel
    count, but conv2d_dgrad gives dx x's own."""
    ho, wo = out_hw(c)
    xs, ys = (c.n, c.cin, c.h, c.w), (c.n, c.cout, ho, wo)
    if op == "fwd":
        return xs, c.xfmt, ys, act_format(c.cout)
    return ys, act_format(c.cout), xs, (act_format(c.cin) if c.tr else c.xfmt)


def transposed_gather(c, op):
    """Whether the op is the transposed gather (sub-pixel phases): a transposed convolution's forward, a
    convolution's input gradient."""
    return c.tr == (op == "fwd")


def phases(c, op):
    """transposed_impl, restated: (rows, columns, taps) of each sub-pixel phase of the op's output grid, the empty
    ones included (the library skips them).  The direct gather is one phase of k * k taps."""
    _, _, (_, _, ho, wo), _ = io(c, op)
    if not transposed_gather(c, op):
        return [(ho, wo, c.k * c.k)]
    out = []
    for py in range(c.s):
        for px in range(c.s):
            ty = sum((py + c.p - a) % c.s == 0 for a in range(c.k))
            tx = sum((px + c.p - b) % c.s == 0 for b in range(c.k))
            out.append(((ho - py + c.s - 1) // c.s, (wo - px + c.s - 1) // c.s, ty * tx))
    return out


def gemm_cout(c, op, plan):
    """The GEMM's Cout: the op's output channels; k * k times them on the col2im detour."""
    ch = io(c, op)[2][1]
    return c.k * c.k * ch if plan["kernel"] == "gemm_col2im" else ch


def chunks(c, op, plan):
    """ig_plan, restated: the K chunks of the longest phase (32 channels of a tap; 64 on ig_kernel_bf16 and the
    bf16 DMA kernel; 32 columns of the (tap, channel) rows in the gather form and of the im2col buffer)."""
    cin = io(c, op)[0][1]
    taps = max(t for h, w, t in phases(c, op) if h > 0 and w > 0)
    kern = plan["kernel"]
    if kern == "ig_fp32_gather" or kern == "im2col_gemm":
        return -(-taps * cin // 32)
    if kern == "gemm_col2im":
        return cin // 32
    return taps * cin // (64 if kern in ("ig_bf16", "ig_bf16_dma") else 32)


def last_split_chunks(c, op, plan):
    """(chunks per split, chunks of the last split) of the longest phase."""
    n = chunks(c, op, plan)
    kcps = -(-n // plan["ksplit"])
    assert -(-n // kcps) == plan["ksplit"], (c.name, op, plan, n)
    return kcps, n - (plan["ksplit"] - 1) * kcps


def reduce_kernel(c, op, plan):
    """ig_run, restated: the kernel that sums the K splits (None: one split, the GEMM kernel stores y itself)."""
    if plan["kernel"] not in GEMM_KERNELS or plan["ksplit"] == 1:
        return None
    if gemm_cout(c, op, plan) % 4:
        return "ig_reduce"
    return "ig_reduce4<%d>" % (plan["ksplit"] if plan["ksplit"] in (2, 3, 4, 8) else 0)


def paths(c):
    """The launch paths the case reaches, over its ops, math modes and views."""
    out = set()
    for op in OPS:
        nph = sum(1 for h, w, t in phases(c, op) if h > 0 and w > 0)
        for plans in (c.plans[op], c.halo[op]):
            for p in plans:
                k = p["kernel"]
                if k in DMA_KERNELS:
                    out.add("%s:phases%d" % (k, nph))
                elif k in IG_KERNELS:
                    out.add("%s:%dx%d" % (k, p["bm"], p["bn"]))
                    if k == "ig_fp32_gather" and nph > 1:
                        out.add("ig_fp32_gather:phase_packs")
                elif k in ("edge_conv", "tconv_few_rows"):
                    out.add("%s:v%d" % (k, p["variant"]))
                else:
                    out.add(k)
                if k == "tconv_few":     # tconv_few_run: the instantiation goes by the input width
                    out.add("tconv_few:w%d" % (64 if io(c, op)[0][3] <= 64 else 128 if io(c, op)[0][3] <= 128 else 256))
                if k.startswith("tconv_few_rows") and io(c, op)[0][3] > 128:
                    out.add("tconv_few_rows:segments")
                r = reduce_kernel(c, op, p)
                if k in GEMM_KERNELS:
                    out.add(r or "no_reduce")
                if r and k in DMA_KERNELS:
                    out.add("dma:" + r.split("<")[0])
    return out


REQUIRED_PATHS = (
    {"ig_fp32:" + t for t in ("64x192", "128x192", "128x64", "256x32")} |
    {"ig_fp32_gather:" + t for t in ("64x192", "128x192", "128x64", "256x32")} | {"ig_fp32_gather:phase_packs"} |
    {"ig_bf16:" + t for t in ("128x192", "128x64", "256x32")} |
    {"ig_split:" + t for t in ("64x192", "128x192", "128x64")} | {"ig_split_bf16:64x192"} |
    {"ig_split_dma:phases1", "ig_split_dma:phases4", "ig_bf16_dma:phases1", "ig_bf16_dma:phases4", "dma:ig_reduce4"} |
    {"no_reduce", "ig_reduce", "ig_reduce4<0>", "ig_reduce4<2>", "ig_reduce4<3>", "ig_reduce4<4>", "ig_reduce4<8>"} |
    {"edge_conv:v0", "edge_conv:v1", "edge_conv_bf16", "im2col_gemm", "gemm_col2im", "tconv_few",
     "tconv_few:w64", "tconv_few:w128", "tconv_few:w256",
     "tconv_few_rows:v0", "tconv_few_rows:v1", "tconv_few_rows_bf16", "tconv_few_rows:segments"})


# ---------------------------------------------------------------- operands
def values(c):
    """x, dy (compact NCHW fp32), the weight and the bias from a generator seeded by the case's place in the table."""
    g = torch.Generator().manual_seed(2000 + CASES.index(c))
    ho, wo = out_hw(c)
    ws = weight_shape(c)
    w = torch.randn(ws, generator=g) * (ws[1 if not c.tr else 0] * c.k * c.k / (c.s * c.s if c.tr else 1)) ** -0.5
    return dict(x=torch.randn(c.n, c.cin, c.h, c.w, generator=g), dy=torch.randn(c.n, c.cout, ho, wo, generator=g),
                w=w, b=torch.randn(c.cout, generator=g) * 0.5)


def place(v, shape, fmt, view="compact", device="cpu"):
    """The tensor of `shape` in layout `fmt` holding v (None: uninitialised memory, for a plan query): compact; the
    interior of a NaN-filled tensor one pixel larger on every side (halo); channels [1 : C + 1] of a NaN-filled
    channels-last tensor of C + 8 channels (chan8: pixel strides 16-byte aligned, the base off by 4 bytes); or
    channels [: C] of one of C + 1 channels (chan1: the base aligned, the pixel stride odd)."""
    assert view in VIEWS and (view not in CHAN_VIEWS or fmt == "cl"), (view, fmt)
    n, ch, h, w = shape
    halo = int(view == "halo")
    big = (n, ch + {"chan8": 8, "chan1": 1}.get(view, 0), h + 2 * halo, w + 2 * halo)
    mf = CL if fmt == "cl" else torch.contiguous_format
    if v is None:
        t = torch.empty(big, device=device).contiguous(memory_format=mf)
    else:
        t = torch.full(big, float("nan")).contiguous(memory_format=mf)

    def cut(t):
        t = t[:, 1:ch + 1] if view == "chan8" else t[:, :ch]
        return t[:, :, 1:-1, 1:-1] if halo else t

    if v is not None:
        cut(t).copy_(v)
        t = t.to(device)        # the whole buffer moves, then the same view of it is taken
    out = cut(t)
    assert tuple(out.shape) == tuple(shape)
    return out


def make_input(c, op, view="compact", device="cpu", vals=None):
    """The op's input (x of the forward, dy of the input gradient) in a view; vals: values(c), None: uninitialised."""
    shape, fmt, _, _ = io(c, op)
    return place(None if vals is None else vals["x" if op == "fwd" else "dy"], shape, fmt, view, device)


def make_output(c, op, device="cpu", haloed=False):
    """An output of the op's shape and layout: compact, uninitialised; or (haloed) the interior of a NaN-filled
    tensor whose halo keeps the interior's base and pixel strides 16-byte aligned: a pixel on every side of a
    channels-last map (C % 4 == 0), a row above and below and 4 columns left, at least 4 right of an NCHW one.
    Returns (the whole tensor, the view)."""
    _, _, (n, ch, h, w), fmt = io(c, op)
    if not haloed:
        t = torch.empty((n, ch, h, w), device=device).contiguous(memory_format=CL if fmt == "cl" else
                                                                  torch.contiguous_format)
        return t, t
    if fmt == "cl":
        assert ch % 4 == 0
        t = torch.full((n, ch, h + 2, w + 2), float("nan"), device=device).contiguous(memory_format=CL)
        v = t[:, :, 1:-1, 1:-1]
    else:
        t = torch.full((n, ch, h + 2, -(-(w + 8) // 4) * 4), float("nan"), device=device)
        v = t[:, :, 1:-1, 4:4 + w]
    assert v.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in (v.stride(0), v.stride(2))), (c.name, op)
    return t, v


def round_bf16(t):
    """Round-to-nearest-even to bf16, kept in t's dtype: what a bf16-operand kernel multiplies."""
    return t.to(torch.bfloat16).to(t.dtype)


def reference(c, op, inp, w, b=None, relu=False):
    """The op in float64 by torch's own convolution of the same values, on their device."""
    i64, w64 = inp.detach().double().contiguous(), w.detach().double()
    if op == "fwd":
        b64 = None if b is None else b.double()
        if c.tr:
            y = F.conv_transpose2d(i64, w64, b64, stride=c.s, padding=c.p, output_padding=c.op)
        else:
            y = F.conv2d(i64, w64, b64, stride=c.s, padding=c.p)
        return torch.relu(y) if relu else y
    if c.tr:    # the input gradient of a transposed convolution is the convolution
        return F.conv2d(i64, w64, None, stride=c.s, padding=c.p)
    ho, wo = out_hw(c)
    opad = (c.h - ((ho - 1) * c.s - 2 * c.p + c.k), c.w - ((wo - 1) * c.s - 2 * c.p + c.k))
    return F.conv_transpose2d(i64, w64, None, stride=c.s, padding=c.p, output_padding=opad)


def plan_of(c, op, inp, out, math):
    from image_compression_amd import _lib
    p = _lib.plan(op_name(c, op), inp, out, c.k, c.s, c.p, math)
    return {k: p[k] for k in PLAN_FIELDS}
