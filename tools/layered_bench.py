#!/usr/bin/env python3
"""Cost of the layered per-image streams beside the plain ones, on the same build, alternated in one process:
`compress_each_layered` against `compress_each`, `decompress_each_layered` at L = G and at L = G / 2 against
`decompress_each`, the bytes a layered stream adds, and the three layer kernels alone by device events with the
bytes they move computed from the shapes.  --batch x 3 x --height x --width synthetic images (default 8 x 3 x 512 x
768), random-init weights with the last analysis conv times --scale (32: symbols up to a few dozen), the model's
default arithmetic, inside functional.weight_cache.  Wall times are the best of --reps alternating repetitions with a
device synchronise inside the timed region (the convention of tools/codec_bench.py).  One JSON line; --out also writes
it to a file.

    python tools/layered_bench.py [--arch MeanScaleCompressor2018] [--layers 8] [--reps 10] [--out profiles/layered_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _alternate(fns, reps):
    """Best wall time of every function, one repetition of each at a time."""
    best = [None] * len(fns)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t = _wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
    return [round(t, 3) for t in best]


def _events(fn, reps, inner=20):
    """Best mean device time of `inner` back-to-back calls, in microseconds."""
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        t = 1e3 * a.elapsed_time(b) / inner
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="MeanScaleCompressor2018")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=32.0)
    ap.add_argument("--steps", type=int, default=1024, help="steps_per_chunk of the streams")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from image_compression_amd import _lib, codec, evaluation, get_cfg_defaults, modelling
    from image_compression_amd import functional as F
    cfg = get_cfg_defaults()
    cfg.MODEL.LOSS.REDUCTION = "mean"
    cfg.MODEL.META_ARCHITECTURE = args.arch
    torch.manual_seed(0)
    model = modelling.build_model(cfg).cuda().eval()
    last = [m for m in model.analysis_transform.modules() if hasattr(m, "weight") and m.weight.dim() == 4][-1]
    with torch.no_grad():
        last.weight.mul_(args.scale)
    N, G, R, reps = args.batch, args.layers, args.steps, args.reps
    x = torch.rand(N, 3, args.height, args.width, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out = {"metric": f"layered per-image streams beside the plain ones, {N} x 3 x {args.height} x {args.width}, {G} layers, "
                     f"weight cache, best of {reps} alternating reps", "unit": "ms", "arch": args.arch,
           "compute_dtype": cfg.MODEL.COMPUTE_DTYPE, "weight_scale": args.scale, "steps_per_chunk": R, "reps": reps,
           "weights": "random init: the prefix-quality curve is not that of a trained model",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad(), F.weight_cache():
        plain = model.compress_each(x, steps_per_chunk=R)                    # the warm-up of every shape, too
        layered = model.compress_each_layered(x, layers=G, steps_per_chunk=R)
        ends = [codec.layer_ends(s) for s in layered]
        half = [s[:e[G // 2]] for s, e in zip(layered, ends)]
        a = torch.cat(model.decompress_each(plain))
        b = torch.cat(model.decompress_each_layered(layered))
        model.decompress_each_layered(half)
        out["max_abs_layered_minus_plain"] = float((a - b).abs().max())
        t = _alternate([lambda: model.compress_each(x, steps_per_chunk=R),
                        lambda: model.compress_each_layered(x, layers=G, steps_per_chunk=R)], reps)
        out["compress_ms"] = {"compress_each": t[0], "compress_each_layered": t[1], "ratio": round(t[1] / t[0], 3)}
        t = _alternate([lambda: model.decompress_each(plain), lambda: model.decompress_each_layered(layered),
                        lambda: model.decompress_each_layered(half)], reps)
        out["decompress_ms"] = {"decompress_each": t[0], "layered_all_layers": t[1], "layered_half_the_layers": t[2],
                                "all_over_plain": round(t[1] / t[0], 3), "half_over_all": round(t[2] / t[1], 3)}
        h = model._layered_containers[1](layered[0], *model._build_id(), version=model._image_format_version())[0]
        C = h.latent_channels
        extra = [len(l) - len(p) for l, p in zip(layered, plain)]
        out["bytes"] = {"plain": [len(s) for s in plain], "layered": [len(s) for s in layered], "extra": extra,
                        "header_and_order": 2 * C + 4,
                        "extra_chunks": G * codec.num_chunks(h.nsym_y // G, R) - codec.num_chunks(h.nsym_y, R),
                        "bits_per_pixel_of_the_prefixes": [round(float(np.mean([8.0 * e[L] / (args.height * args.width)
                                                                                for e in ends])), 4) for L in range(G + 1)]}
        out["progressive_sweep"] = evaluation.progressive_sweep(model, [x], layers=G, steps_per_chunk=R)
        # the kernels alone: bytes from the shapes over device time
        ops = _lib.layer_ops()
        P = h.nsym_y // C
        n = N * P * C
        sym = torch.randint(-40, 41, (N, P, C), dtype=torch.int32, device="cuda")
        rows = torch.randint(0, 64, (N, P, C), dtype=torch.uint8, device="cuda")
        mu = torch.randn(N, P, C, device="cuda")
        order = np.stack([np.random.default_rng(k).permutation(C) for k in range(N)]).reshape(-1).tolist()
        seg = [v for k in range(N) for g in range(G) for v in (k, g)]
        q = ops.gather(sym, G, order, seg).float()
        kernels = {"energy": (lambda: ops.energy(sym), 4 * n),
                   "gather_symbols": (lambda: ops.gather(sym, G, order, seg), 8 * n),
                   "gather_rows": (lambda: ops.gather(rows, G, order, seg), 2 * n),
                   "scatter_with_mean": (lambda: ops.scatter(q, mu, N, P, C, G, order, [G] * N), 12 * n),
                   "scatter_half_with_mean": (lambda: ops.scatter(q[:n // 2], mu, N, P, C, G, order, [G // 2] * N), 10 * n)}
        out["kernels"] = {"symbols": n, "note": "op calls: the host's check and copy of the order included"}
        for name, (fn, nbytes) in kernels.items():
            fn()
            us = _events(fn, reps)
            out["kernels"][name] = {"us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
