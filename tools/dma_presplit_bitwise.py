#!/usr/bin/env python3
"""Outputs of the DMA-tile split convolutions (ig_kernel_x3d) on fixed inputs: save them (--out F) or
compare bitwise with a saved run (--ref F) -- run once per library build (IMGCOMP_LIB) to check that two
builds of the kernel agree bitwise (the A pre-split against the in-loop split, IG_X3D_PRESPLIT=0).
Covers the shapes of tests/test_dma_presplit_gpu.py -- split K with even, odd and short chunk ranges, one-,
two- and three-chunk ranges, the four phases of a transposed conv, a partial last tile, bias / ReLU -- and
g_a.2 / g_s.4 forward at the bench shape (32 x 192 x 128^2 -> 64^2, 32 x 192 x 64^2 -> 128^2).  Every case must
plan ig_split_dma, or the tool stops.  GPU only."""
import argparse, os, sys, torch
sys.path.insert(0, os.getcwd())
from image_compression_amd import _lib
ap = argparse.ArgumentParser(); ap.add_argument("--out"); ap.add_argument("--ref"); a = ap.parse_args()
ops = _lib.ops(); dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(29)
CL = torch.channels_last
M = 2  # IC_MATH fp32_split
res = {}


def act(*s):
    return (torch.randn(*s, device=dev, generator=g)).contiguous(memory_format=CL)


def dma(op, p, q, k, s, pad):
    pl = _lib.plan(op, p, q, k, s, pad, M)
    if pl["kernel"] != "ig_split_dma":
        sys.exit(f"{op} {tuple(p.shape)} k{k}s{s}: plans {pl['kernel']}, not ig_split_dma")
    return pl["ksplit"]


def conv(tag, n, cin, h, k, s, pad, bias=True, relu=0, dgrad=False):
    x = act(n, cin, h, h)
    w = torch.randn(192, cin, k, k, device=dev, generator=g) * 0.03
    b = torch.randn(192, device=dev, generator=g) * 0.1 if bias else None
    ho = (h + 2 * pad - k) // s + 1
    y = torch.empty(n, 192, ho, ho, device=dev).contiguous(memory_format=CL)
    ks = dma("conv2d_fwd", x, y, k, s, pad)
    res[f"{tag}_fwd_ks{ks}"] = ops.conv2d_fwd(x, w, b, s, pad, relu, M).clone()
    if dgrad:
        gy = act(n, 192, ho, ho)
        ks = dma("conv2d_dgrad", gy, x, k, s, pad)
        res[f"{tag}_dgrad_ks{ks}"] = ops.conv2d_dgrad(gy, w, x, s, pad, M).clone()


def tconv(tag, n, h, bias=False, relu=0, fwd=True, dgrad=True):
    x = act(n, 192, h, h)
    w = torch.randn(192, 192, 5, 5, device=dev, generator=g) * 0.03
    b = torch.randn(192, device=dev, generator=g) * 0.1 if bias else None
    y = torch.empty(n, 192, 2 * h, 2 * h, device=dev).contiguous(memory_format=CL)
    if fwd:
        ks = dma("conv_transpose2d_fwd", x, y, 5, 2, 2)
        res[f"{tag}_tfwd_ks{ks}"] = ops.conv_transpose2d_fwd(x, w, b, 2, 2, 1, relu, M).clone()
    if dgrad:
        gy = act(n, 192, 2 * h, 2 * h)
        ks = dma("conv_transpose2d_dgrad", gy, x, 5, 2, 2)
        res[f"{tag}_tdgrad_ks{ks}"] = ops.conv_transpose2d_dgrad(gy, w, x, 2, 2, M).clone()


conv("5x5_8x64", 8, 192, 64, 5, 2, 2)
conv("5x5_8x128", 8, 192, 128, 5, 2, 2, dgrad=True)
conv("5x5_13x50", 13, 192, 50, 5, 2, 2)
conv("3x3_8x32", 8, 192, 32, 3, 1, 1, dgrad=True)
for cin in (32, 64, 96):
    conv(f"1x1_cin{cin}", 8, cin, 32, 1, 1, 0)
    conv(f"3x3_cin{cin}", 8, cin, 32, 3, 1, 1)
tconv("t_4x64", 4, 64)
tconv("t_2x64", 2, 64, fwd=False)
tconv("t_3x64", 3, 64, fwd=False)
tconv("t_4x64_bias_relu", 4, 64, bias=True, relu=1, dgrad=False)
conv("5x5_18x122_relu", 18, 192, 122, 5, 2, 2, relu=1)
conv("g_a.2", 32, 192, 128, 5, 2, 2)
tconv("g_s.4", 32, 64, bias=True, dgrad=False)
torch.cuda.synchronize()
print("cases:", " ".join(res))
if a.out:
    torch.save({k: v.cpu() for k, v in res.items()}, a.out); print("saved", len(res))
if a.ref:
    ref = torch.load(a.ref, weights_only=True)
    bad = [k for k in ref if k not in res or not torch.equal(ref[k], res[k].cpu())]
    for k in bad:
        print("DIFF", k, (ref[k] - res[k].cpu()).abs().max().item() if k in res else "missing")
    print("bitwise equal" if not bad else f"{len(bad)} of {len(ref)} differ", len(ref), "tensors")
    sys.exit(1 if bad else 0)
