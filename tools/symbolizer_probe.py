#!/usr/bin/env python3
"""The seven symbolizer entry points at the budget bench's size, for a kernel trace (rocprofv3 --kernel-trace --stats
-- python tools/symbolizer_probe.py) or device-event times: N = 8 images of 32 x 48 x 192 latents, M = 64 candidates
or segments.  Prints the best and the median of REPS (default 10) event times per entry point.

    python tools/symbolizer_probe.py [REPS]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from image_compression_amd import _lib  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
DEV = "cuda"
g0 = torch.Generator(device=DEV).manual_seed(3)
N, M, Hm, Wm, C = 8, 64, 32, 48, 192
P = Hm * Wm
y = torch.randn(N, Hm, Wm, C, device=DEV, generator=g0) * 20
r = torch.round(y)
mu1 = torch.randn(N, Hm, Wm, C, device=DEV, generator=g0)
mu = torch.randn(M, Hm, Wm, C, device=DEV, generator=g0)
yM = torch.randn(M, Hm, Wm, C, device=DEV, generator=g0) * 20
g = torch.rand(M, C, device=DEV, generator=g0) + 0.5
a = torch.rand(N, C, device=DEV, generator=g0) + 0.5
gr = torch.rand(6, C, device=DEV, generator=g0) + 0.5
shift = 6
rank = torch.randint(0, 6, (M, (Hm + 63) // 64, (Wm + 63) // 64), device=DEV, generator=g0, dtype=torch.uint8)
img = [m % N for m in range(M)]

cases = {
    "codec_symbolize": lambda: _lib.codec_ops().symbolize(yM),
    "codec_symbolize_seg": lambda: _lib.stream_ops().symbolize_seg(yM, M),
    "codec_symbolize_mean": lambda: _lib.mean_ops().symbolize(yM, mu),
    "codec_symbolize_mean_seg": lambda: _lib.mean_ops().symbolize_seg(yM, mu, M),
    "gain_symbolize_seg": lambda: _lib.rate_ops().gain_symbolize_seg(y, g, mu, img),
    "requant_seg": lambda: _lib.transcode_ops().requant_seg(r, mu1, a, g, mu, img),
    "block_gain_symbolize_seg": lambda: _lib.alloc_ops().block_gain_symbolize_seg(y, gr, rank, mu, img, shift),
}
out = {}
for name, fn in cases.items():
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    out[name] = (min(times), sorted(times)[len(times) // 2])
for k, (b, m) in out.items():
    print(f"{k:28s} best {b:.4f} ms  median {m:.4f} ms  ({M * P * C} symbols)")
