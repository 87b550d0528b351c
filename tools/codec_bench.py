#!/usr/bin/env python3
"""Cost of real bitstreams: Compressor2018.compress / decompress at the Kodak evaluator's shape
(batch 1, 512x768) inside functional.weight_cache, on synthetic images with random-init weights,
beside the eval forward measured the way tools/eval_bench.py measures it (eager, weight cache), and
the coder's own ops (symbolize, scale index, tables, encode + compact, decode) timed by events on the
symbols of the same image.  One JSON line; --out also writes it to a file.

    python tools/codec_bench.py [--reps 10] [--height 512] [--width 768] [--scale 1] [--out FILE]
    python tools/codec_bench.py --each 8 [--reps 10] [--scale 32] [--out profiles/codec_each_bench.json]
    python tools/codec_bench.py --compare 8 [--reps 10] [--scale 32] [--out FILE]

--arch NAME (default Compressor2018) runs the two modes above on another registered model, e.g.
MeanScaleCompressor2018; the output then carries an "arch" key.  For CheckerboardCompressor2018 (another container,
no per-image streams) the first mode reports the forward, compress and decompress times and the bytes only.

--compare N times Compressor2018 and MeanScaleCompressor2018 alternately in one process: compress / decompress
and compress_each / decompress_each at 1 and N images of --height x --width (ms per image, best of --reps), the
mean-scale model's elementwise ops beside their scale-only counterparts by device events, and the coded bytes of both.

--arch GainedMeanScaleCompressor2018 [--quality q] codes at quality q (default: the model's, its top level).

--gained N times MeanScaleCompressor2018 and GainedMeanScaleCompressor2018 alternately in one process: the eval
forward, compress and decompress at 1 x --height x --width (seed weights and zero tables: both code the same
symbols), the gain kernels beside ic_center_round by device events on the y of N images, one eager training step
of both at 32 x 256 x 256, and the coded bytes at every integer level of a ladder of gains on --scale'd weights.

--region N times GainedMeanScaleCompressor2018 (scalar quality 3) and RegionGainedMeanScaleCompressor2018 (a centre
rectangle at level 5 over a background at level 1) alternately in one process, both on --scale'd weights with ladder
tables: the eval forward, compress and decompress at 1 x --height x --width; ic_block_scale / _bwd beside
ic_channel_scale / _bwd with a row per image and ic_block_mse beside ic_mse by device events on N images; one eager
training step of both at 32 x 256 x 256; and the coded bytes of three maps.

--rdmap N times the rate and distortion maps: ic_block_bits beside ic_ce_loss_fwd on the p_y and the p_z of N images
and ic_block_sse beside ic_mse_fwd on the images and their reconstructions, by device events over 20 back-to-back
calls; `rate_distortion_map` beside the eval forward at 1 x --height x --width on the gained and the region model;
and per image the estimated bytes (bits.sum() / 8) beside the bytes of its `compress_each` stream.

--budget BYTES [--candidates 8] [--rounds 2] codes 8 x 3 x 512 x 768 images ("x32" weights, ladder tables) to BYTES
each, (a) by the naive search from public calls (compress_each at every grid quality, then at every refinement; the
images of a call each at their own candidate) and (b) by compress_each_to, alternately in one process; then
measure_seg beside encode_seg + compact_seg and the fused symbolizer beside gather + channel_scale +
symbolize_mean_seg on one round's candidates, by device events.  --out profiles/codec_budget_bench.json.

--map-budget BYTES [--candidates 8] [--rounds 2] codes 8 x 3 x 512 x 768 images whose blocks differ in activity ("x32"
weights, ladder tables, level weights 10 .. 1e6) to BYTES each with a quality map per image, (a) by the naive search
from public calls (S rate_distortion_map calls, the allocation rule in numpy, set_quality_map + compress_each per
candidate slope) and (b) by compress_each_map_to, alternately in one process; and, for the record only, every image's
measured squared error under its map beside compress_each_to's one quality on the gained model at the same budget.
--out profiles/codec_mapbudget_bench.json.

--refine T [--arch NAME] [--scale 32] times compress_each and compress_each_refined with T steps on 8 x 3 x 512 x 768
images (ms per image, best of --reps wall times), the cost of one refinement step by device events ((T steps - 0
steps) / T) and, beside it, one g_s forward with its input-gradient backward.  --out profiles/codec_refine_bench.json.

--transcode Q2 [--rechunk R] [--transcode-budget BYTES] takes 8 x 3 x 512 x 768 "ICRQ" streams ("x32" weights, ladder
tables) from quality S - 1 to Q2, (a) through pixels (decompress_each, set_quality, compress_each) and (b) by
transcode_each, alternately in one process; with a budget, transcode_each_to beside the search rule run on (a)-style
calls; requant_seg beside add_mean + channel_scale x 2 + symbolize_mean_seg on the same operands, by device events; and
the PSNR and the sizes of both routes beside direct coding at Q2.  --out profiles/codec_transcode_bench.json.

--hs-compare [--budget 450000] runs MODEL.HYPER_SYNTHESIS.KERNEL "conv" and "invariant" alternately on the gained model
("x32" weights, ladder tables): h_s alone at 1, 8 and 64 maps of z 8 x 12 x 192 by device events (batch-1 conv passes,
one batched conv pass, one invariant pass), compress_each / decompress_each / compress_each_to at 8 x 3 x 512 x 768 and
the batch-1 eval forward, compress and decompress; every repetition is kept.  --out profiles/codec_hs_invariant.json.

--context fused|conv builds CheckerboardCompressor2018 with that MODEL.CONTEXT.KERNEL (default conv); with fused,
--each works on it too (its loop arm is then the fused model's own compress / decompress).

--context-compare N times the "conv" and the "fused" checkerboard model (same weights, a nonzero context)
alternately in one process: the eval forward, compress and decompress of one --height x --width image; the context
alone by device events on that image's latent (two convs and two elementwise ops against the one kernel); the loop
of the conv model's compress(x[n:n+1]) / decompress against the fused model's compress_each / decompress_each on N
images, and the latter on N images of 500 x 750; and the bytes of the "ICRK" streams beside "ICRC" version 2 and
the mean-scale model's "ICRP" streams of the same images.

--each N measures per-image streams instead: N images of --height x --width coded (a) by the loop of
compress(x[n:n+1]) / decompress and (b) by compress_each / decompress_each, timed alternately in one process
(best of --reps wall times, device synchronised inside the timed region), then (b) alone on N images of
500 x 750 (the padded case, which (a) cannot code), the coder ops of both by device events, and N
single-image h_s passes beside one batched pass.

--scale multiplies the last analysis conv's weight (random-init latents round to 0 almost everywhere;
32 gives symbols up to a few dozen, the alphabet of a trained model).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _wall(fn, reps):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return 1e3 * best


def _events(fn, reps):
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    return best


def each_bench(args, model, cfg):
    """--each N: the loop over single-image batches against compress_each / decompress_each."""
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    from image_compression_amd.modelling.blocks.entropy_model import table_pool
    N, H, W, reps = args.each, args.height, args.width, args.reps
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(N, 3, H, W, device="cuda", generator=g)
    x_odd = torch.rand(N, 3, 500, 750, device="cuda", generator=g)
    ops, sops = _lib.codec_ops(), _lib.stream_ops()
    em, cm = model.entropy_model, model.conditional_model
    R = 1024
    with torch.no_grad(), F.weight_cache():
        loop_c = lambda: [model.compress(x[n:n + 1]) for n in range(N)]
        loop_d = lambda: [model.decompress(d) for d in datas]
        each_c = lambda: model.compress_each(x)
        each_d = lambda: model.decompress_each(streams)
        for _ in range(2):                                   # warm-up of every candidate
            datas, streams, odd = loop_c(), each_c(), model.compress_each(x_odd)
            loop_d(), each_d(), model.decompress_each(odd)
        want = model(x)[0]
        same = all(bool(torch.equal(t[0], want[n])) for n, t in enumerate(each_d()))
        t = {"loop_compress": [], "each_compress": [], "loop_decompress": [], "each_decompress": []}
        for _ in range(reps):                                # alternately, one repetition of each at a time
            t["loop_compress"].append(_wall(loop_c, 1))
            t["each_compress"].append(_wall(each_c, 1))
            t["loop_decompress"].append(_wall(loop_d, 1))
            t["each_decompress"].append(_wall(each_d, 1))
        best = {k: min(v) for k, v in t.items()}
        t_odd_c = _wall(lambda: model.compress_each(x_odd), reps)
        t_odd_d = _wall(lambda: model.decompress_each(odd), reps)
        # the coder ops alone, on the latents of these images: N launches of the whole-tensor kernels against
        # one launch of the segmented ones
        y, z, z_sym, kz, (sigma, mean) = model._analyse(x, each=True)
        z_hat = z_sym.float().view(N, *z.shape[2:], z.shape[1]).movedim(-1, 1)
        sigma = sigma.expand_as(y)
        y_sym, ky = model._symbols(y, mean, each=True)
        rows = cm.scale_rows(sigma)
        ny, nz = y_sym.numel() // N, z_sym.numel() // N
        y_l = y.movedim(1, -1).contiguous()
        if mean is None:
            sym_loop = lambda: [ops.symbolize(y_l[n]) for n in range(N)]
            sym_seg = lambda: sops.symbolize_seg(y_l, N)
        else:
            m_l, mops = mean.movedim(1, -1).contiguous(), _lib.mean_ops()
            sym_loop = lambda: [mops.symbolize(y_l[n], m_l[n]) for n in range(N)]
            sym_seg = lambda: mops.symbolize_seg(y_l, m_l, N)
        ty = {K: cm.tables(K, x.device) for K in set(ky)}
        tz = {K: em.tables(K) for K in set(kz)}
        pool_y, nrows_y, ks_y, offs_y = table_pool(lambda K: ty[K], ky)
        pool_z, nrows_z, ks_z, offs_z = table_pool(lambda K: tz[K], kz)
        py = sops.encode_seg(y_sym, N, rows, 0, pool_y, nrows_y, ks_y, offs_y, R)
        parts = codec.split_packed_seg(py.cpu().numpy(), N, ny, R)
        buf_y = torch.from_numpy(codec.join_packed_seg(parts).copy()).cuda()
        one_y = [torch.from_numpy(codec.join_packed(l, p).copy()).cuda() for l, p in parts]
        kern = {
            "symbolize_y_loop": _events(sym_loop, reps),
            "symbolize_y_seg": _events(sym_seg, reps),
            "encode_y_loop": _events(lambda: [ops.encode(y_sym[n * ny:(n + 1) * ny], rows[n * ny:(n + 1) * ny], 0,
                                                         ty[ky[n]], R) for n in range(N)], reps),
            "encode_y_seg": _events(lambda: sops.encode_seg(y_sym, N, rows, 0, pool_y, nrows_y, ks_y, offs_y, R), reps),
            "encode_z_loop": _events(lambda: [ops.encode(z_sym[n * nz:(n + 1) * nz], None, em.channels, tz[kz[n]], R)
                                              for n in range(N)], reps),
            "encode_z_seg": _events(lambda: sops.encode_seg(z_sym, N, None, em.channels, pool_z, nrows_z, ks_z, offs_z,
                                                            R), reps),
            "decode_y_loop": _events(lambda: [ops.decode(one_y[n], ny, rows[n * ny:(n + 1) * ny], 0, ty[ky[n]], R)
                                              for n in range(N)], reps),
            "decode_y_seg": _events(lambda: sops.decode_seg(buf_y, N, ny, rows, 0, pool_y, nrows_y, ks_y, offs_y, R),
                                    reps),
            "tables_y_loop": _events(lambda: [cm.tables(K, x.device) for K in ky], reps),
            "tables_y_seg": _events(lambda: table_pool(lambda K: cm.tables(K, x.device), ky), reps),
            "h_s_single_x_n": _events(lambda: model._prior_each(z_hat), reps),
            "h_s_batched": _events(lambda: model._prior(z_hat), reps),
            "pad_edge_500x750": _events(lambda: sops.pad_edge(x_odd, 512, 768), reps),
            "crop_clamp_500x750": _events(lambda: sops.crop_clamp(want, 500, 750), reps),
        }
    out = {
        "metric": f"per-image streams: ms per image, {N} x 3 x {H} x {W}, weight cache, best of {reps} alternating reps",
        "unit": "ms per image",
        "loop_compress_ms": round(best["loop_compress"] / N, 4), "each_compress_ms": round(best["each_compress"] / N, 4),
        "compress_ratio_each_over_loop": round(best["each_compress"] / best["loop_compress"], 4),
        "loop_decompress_ms": round(best["loop_decompress"] / N, 4),
        "each_decompress_ms": round(best["each_decompress"] / N, 4),
        "decompress_ratio_each_over_loop": round(best["each_decompress"] / best["loop_decompress"], 4),
        "each_no_slower_than_loop": bool(best["each_compress"] <= best["loop_compress"]
                                         and best["each_decompress"] <= best["loop_decompress"]),
        "padded_500x750_each_compress_ms": round(t_odd_c / N, 4),
        "padded_500x750_each_decompress_ms": round(t_odd_d / N, 4),
        "all_reps_ms_per_batch": {k: [round(v, 3) for v in vs] for k, vs in t.items()},
        "coder_ops_ms_per_batch": {k: round(v, 4) for k, v in kern.items()},
        "bytes_loop": sum(map(len, datas)), "bytes_each": sum(map(len, streams)), "bytes_each_500x750": sum(map(len, odd)),
        "kmax_y": ky, "kmax_z": kz, "steps_per_chunk": R, "images": N,
        "decompress_each_equals_batched_forward": same, "weight_scale": args.scale, "reps": reps,
        "compute_dtype": cfg.MODEL.COMPUTE_DTYPE,
        "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0)",
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--each", type=int, default=0, metavar="N",
                    help="per-image streams: the loop of compress(x[n:n+1]) against compress_each over N images")
    ap.add_argument("--arch", default="Compressor2018", help="the registered model to measure (META_ARCHITECTURE)")
    ap.add_argument("--compare", type=int, default=0, metavar="N",
                    help="Compressor2018 and MeanScaleCompressor2018 alternately, at 1 and N images")
    ap.add_argument("--quality", type=float, default=None, help="the quality a model with gain units codes at")
    ap.add_argument("--gained", type=int, default=0, metavar="N",
                    help="MeanScaleCompressor2018 and GainedMeanScaleCompressor2018 alternately; kernels on the y of N images")
    ap.add_argument("--context", choices=("conv", "fused"), default="conv",
                    help="MODEL.CONTEXT.KERNEL of CheckerboardCompressor2018")
    ap.add_argument("--context-compare", type=int, default=0, metavar="N", dest="context_compare",
                    help='the "conv" and the "fused" checkerboard model alternately; per-image streams at N images')
    ap.add_argument("--region", type=int, default=0, metavar="N",
                    help="GainedMeanScaleCompressor2018 and RegionGainedMeanScaleCompressor2018 alternately; kernels on "
                         "the y of N images")
    ap.add_argument("--rdmap", type=int, default=0, metavar="N",
                    help="the rate / distortion map kernels beside ic_ce_loss_fwd / ic_mse_fwd on N images; "
                         "rate_distortion_map beside the eval forward")
    ap.add_argument("--budget", type=int, default=0, metavar="BYTES",
                    help="8 x 3 x 512 x 768 images coded to BYTES each: the naive search from compress_each against "
                         "compress_each_to (--candidates, --rounds)")
    ap.add_argument("--map-budget", type=int, default=0, metavar="BYTES", dest="map_budget",
                    help="8 x 3 x 512 x 768 images coded to BYTES each with a quality map per image: the naive search from "
                         "rate_distortion_map, set_quality_map and compress_each against compress_each_map_to "
                         "(--candidates, --rounds)")
    ap.add_argument("--refine", type=int, default=None, metavar="T",
                    help="compress_each beside compress_each_refined with T steps at 8 x 3 x 512 x 768; ms per step")
    ap.add_argument("--candidates", type=int, default=8,
                    help="candidate qualities per round of --budget / --transcode-budget")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of --budget / --transcode-budget")
    ap.add_argument("--transcode", type=float, default=None, metavar="Q2",
                    help="8 x 3 x 512 x 768 streams at quality S - 1 taken to Q2: decompress_each + set_quality + "
                         "compress_each against transcode_each; requant_seg beside the four ops it replaces")
    ap.add_argument("--rechunk", type=int, default=0, metavar="R", help="steps per chunk of --transcode's outputs")
    ap.add_argument("--transcode-budget", type=int, default=0, metavar="BYTES", dest="transcode_budget",
                    help="with --transcode: transcode_each_to BYTES per stream against the search through pixels")
    ap.add_argument("--hs-compare", action="store_true", dest="hs_compare",
                    help='MODEL.HYPER_SYNTHESIS.KERNEL "conv" and "invariant" alternately on the gained model: h_s alone at '
                         "1, 8 and 64 maps, the per-image calls at 8 x 3 x 512 x 768 (compress_each_to at --budget), the "
                         "batch-1 calls")
    args = ap.parse_args()
    from image_compression_amd import _lib, codec, get_cfg_defaults, modelling
    from image_compression_amd import functional as F
    if args.hs_compare:
        _emit(hs_bench(args), args.out)
        return
    if args.transcode is not None:
        _emit(transcode_bench(args), args.out)
        return
    if args.transcode_budget or args.rechunk:
        ap.error("--transcode-budget and --rechunk go with --transcode Q2")
    if args.refine is not None:
        if args.refine < 0:
            ap.error("--refine: a number of steps >= 0")
        _emit(refine_bench(args), args.out)
        return
    if args.budget:
        _emit(budget_bench(args), args.out)
        return
    if args.map_budget:
        _emit(map_budget_bench(args), args.out)
        return
    if args.rdmap:
        _emit(rdmap_bench(args), args.out)
        return
    if args.region:
        _emit(region_bench(args), args.out)
        return
    if args.context_compare:
        _emit(context_bench(args), args.out)
        return
    if args.compare:
        _emit(compare_bench(args), args.out)
        return
    if args.gained:
        _emit(gained_bench(args), args.out)
        return
    model, cfg = _build(args.arch, args.scale, args.context)
    if args.quality is not None:
        if not hasattr(model, "set_quality"):
            ap.error(f"--quality: {args.arch} has no gain units")
        model.set_quality(args.quality)
    tag = lambda out: out if args.arch == "Compressor2018" else dict(out, arch=args.arch)
    if args.each:
        _emit(tag(each_bench(args, model, cfg)), args.out)
        return
    x = torch.rand(1, 3, args.height, args.width, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    ops = _lib.codec_ops()
    em, cm = model.entropy_model, model.conditional_model

    wall = lambda fn: _wall(fn, args.reps)
    events = lambda fn: _events(fn, args.reps)

    with torch.no_grad(), F.weight_cache():
        for _ in range(2):
            model(x)
            data = model.compress(x)
            x_hat = model.decompress(data)
        same = bool(torch.equal(x_hat, model(x)[0]))
        t_fwd = wall(lambda: model(x))
        t_c = wall(lambda: model.compress(x))
        t_d = wall(lambda: model.decompress(data))
        if data[:4] != codec.MAGIC:
            # another container (CheckerboardCompressor2018's "ICRC", y in two streams): the three calls only
            _emit(tag({"metric": f"compress / decompress ms per image ({args.height}x{args.width}, batch 1, weight cache)",
                       "unit": "ms", "forward_ms": round(t_fwd, 3), "compress_ms": round(t_c, 3),
                       "decompress_ms": round(t_d, 3), "bytes": len(data),
                       "coded_bpp": round(8 * len(data) / (args.height * args.width), 5),
                       "container": data[:4].decode(), "decompress_equals_forward": same, "weight_scale": args.scale,
                       **({"quality": model.quality} if hasattr(model, "set_quality") else {}),
                       "reps": args.reps, "compute_dtype": cfg.MODEL.COMPUTE_DTYPE}), args.out)
            return
        # the coder's ops alone, on this image's latents
        h = codec.parse(data, int(_lib.load().ic_version()), cfg.MODEL.COMPUTE_DTYPE)[0]
        y, z, z_sym, kz, (sigma, mean) = model._analyse(x)
        sigma = sigma.expand_as(y)
        y_sym, ky = model._symbols(y, mean)
        sig_l = sigma.movedim(1, -1).contiguous()
        if mean is None:
            sym_y = lambda: ops.symbolize(y.movedim(1, -1).contiguous())
        else:
            sym_y = lambda: _lib.mean_ops().symbolize(y.movedim(1, -1).contiguous(), mean.movedim(1, -1).contiguous())
        mids = [float(m) for m in codec.scale_table(cm.num_scales, cm.scale_min, cm.scale_max)[1]]
        tz, ty = em.tables(kz), cm.tables(ky, x.device)
        rows = ops.scale_index(sig_l, mids)
        pz, py = ops.encode(z_sym, None, em.channels, tz, h.R), ops.encode(y_sym, rows, 0, ty, h.R)
        nz, ny = codec.num_chunks(z_sym.numel(), h.R), codec.num_chunks(y_sym.numel(), h.R)
        kern = {
            "symbolize_y": events(sym_y),
            "scale_index_y": events(lambda: ops.scale_index(sig_l, mids)),
            "tables_z": events(lambda: em.tables(kz)),
            "tables_y": events(lambda: cm.tables(ky, x.device)),
            "encode_z": events(lambda: ops.encode(z_sym, None, em.channels, tz, h.R)),
            "encode_y": events(lambda: ops.encode(y_sym, rows, 0, ty, h.R)),
            "decode_z": events(lambda: ops.decode(pz, z_sym.numel(), None, em.channels, tz, h.R)),
            "decode_y": events(lambda: ops.decode(py, y_sym.numel(), rows, 0, ty, h.R)),
        }
    n_pix = args.height * args.width
    out = {
        "metric": f"compress / decompress ms per image ({args.height}x{args.width}, batch 1, weight cache)",
        "unit": "ms",
        "forward_ms": round(t_fwd, 3), "compress_ms": round(t_c, 3), "decompress_ms": round(t_d, 3),
        "coder_ops_ms": {k: round(v, 4) for k, v in kern.items()},
        "coder_ops_total_ms": {"compress": round(sum(kern[k] for k in ("symbolize_y", "scale_index_y", "tables_z",
                                                                        "tables_y", "encode_z", "encode_y")), 3),
                               "decompress": round(sum(kern[k] for k in ("scale_index_y", "tables_z", "tables_y",
                                                                          "decode_z", "decode_y")), 3)},
        "bytes": len(data), "coded_bpp": round(8 * len(data) / n_pix, 5), "fixed_bytes": codec.fixed_bytes(h),
        "kmax_z": h.kmax_z, "kmax_y": h.kmax_y, "chunks_z": nz, "chunks_y": ny, "steps_per_chunk": h.R,
        "symbols_y": y_sym.numel(), "symbols_z": z_sym.numel(),
        "decompress_equals_forward": same, "weight_scale": args.scale, "reps": args.reps,
        "compute_dtype": cfg.MODEL.COMPUTE_DTYPE,
        "data": "synthetic uniform [0,1) image resident in HBM; random-init weights (reference init, seed 0)",
    }
    _emit(tag(out), args.out)


def _build(arch, scale, context="conv", hs="conv"):
    from image_compression_amd import get_cfg_defaults, modelling
    cfg = get_cfg_defaults()
    cfg.MODEL.LOSS.REDUCTION = "mean"
    cfg.MODEL.META_ARCHITECTURE = arch
    cfg.MODEL.CONTEXT.KERNEL = context
    cfg.MODEL.HYPER_SYNTHESIS.KERNEL = hs
    torch.manual_seed(0)
    model = modelling.build_model(cfg).cuda().eval()
    if scale != 1.0:
        last = [m for m in model.analysis_transform.modules() if hasattr(m, "weight") and m.weight.dim() == 4][-1]
        with torch.no_grad():
            last.weight.mul_(scale)
    return model, cfg


def compare_bench(args):
    """--compare N: the scale-only and the mean-scale model, one repetition of each at a time."""
    from image_compression_amd import _lib
    from image_compression_amd import functional as F
    archs = ("Compressor2018", "MeanScaleCompressor2018")
    models = {a: _build(a, args.scale)[0] for a in archs}
    H, W, reps = args.height, args.width, args.reps
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {"metric": f"scale-only and mean-scale codec, ms per image at 3 x {H} x {W}, weight cache, best of {reps} "
                     "alternating reps", "unit": "ms per image", "weight_scale": args.scale, "reps": reps,
           "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0)"}
    with torch.no_grad(), F.weight_cache():
        for N in sorted({1, args.compare}):
            x = torch.rand(N, 3, H, W, device="cuda", generator=g)
            data, streams = {}, {}
            for a, m in models.items():
                for _ in range(2):                           # warm-up of every candidate
                    data[a], streams[a] = m.compress(x), m.compress_each(x)
                    same = bool(torch.equal(m.decompress(data[a]), m(x)[0]))
                    m.decompress_each(streams[a])
                out[f"{a}_decompress_equals_forward_n{N}"] = same
            fns = {"compress": lambda m, a: m.compress(x), "decompress": lambda m, a: m.decompress(data[a]),
                   "compress_each": lambda m, a: m.compress_each(x),
                   "decompress_each": lambda m, a: m.decompress_each(streams[a])}
            t = {(k, a): [] for k in fns for a in archs}
            for _ in range(reps):
                for k, fn in fns.items():
                    for a, m in models.items():
                        t[k, a].append(_wall(lambda: fn(m, a), 1))
            for (k, a), v in t.items():
                out[f"{a}_{k}_ms_n{N}"] = round(min(v) / N, 4)
            for a in archs:
                out[f"{a}_bytes_n{N}"] = len(data[a])
                out[f"{a}_bytes_each_n{N}"] = sum(map(len, streams[a]))
        # the mean-scale model's elementwise ops beside their scale-only counterparts, on its latents of the last x
        m = models["MeanScaleCompressor2018"]
        ops, sops, mops = _lib.codec_ops(), _lib.stream_ops(), _lib.mean_ops()
        y = m.analysis_transform(x)
        z_hat = torch.round(m.prior_analysis(y))
        sigma, mu = m._prior(z_hat)
        y_l, m_l = y.movedim(1, -1).contiguous(), mu.movedim(1, -1).contiguous()
        r = mops.center_round(y_l, m_l)[0]
        out["elementwise_ops_ms"] = {k: round(v, 4) for k, v in {
            "symbolize_y": _events(lambda: ops.symbolize(y_l), reps),
            "symbolize_mean_y": _events(lambda: mops.symbolize(y_l, m_l), reps),
            "symbolize_seg_y": _events(lambda: sops.symbolize_seg(y_l, N), reps),
            "symbolize_mean_seg_y": _events(lambda: mops.symbolize_seg(y_l, m_l, N), reps),
            "quantize_y": _events(lambda: F.quantize(y_l, False), reps),
            "center_round_y": _events(lambda: mops.center_round(y_l, m_l), reps),
            "add_mean_y": _events(lambda: mops.add_mean(r, m_l), reps),
            "h_s_sigma_only": _events(lambda: m.prior_synthesis(z_hat), reps),
            "h_s_both_heads": _events(lambda: m._prior(z_hat), reps),
        }.items()}
        out["elementwise_ops_values"] = y_l.numel()
        out["elementwise_ops_images"] = N
    return out


def context_bench(args):
    """--context-compare N: the checkerboard model with the context convs and with the fused context kernel."""
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    from image_compression_amd.modelling.blocks.entropy_model import ckbd_input, ckbd_params
    CK = "CheckerboardCompressor2018"
    models = {k: _build(CK, args.scale, k)[0] for k in ("conv", "fused")}
    mean = _build("MeanScaleCompressor2018", args.scale)[0]
    gw = torch.Generator().manual_seed(1)
    with torch.no_grad():                                    # one nonzero context, all 25 taps, in both models
        for name, std in (("context_mean", 0.02), ("context_scale", 0.005)):
            w = torch.randn(getattr(models["conv"], name).weight.shape, generator=gw) * std
            b = torch.randn(getattr(models["conv"], name).bias.shape, generator=gw) * std
            for m in models.values():
                getattr(m, name).weight.copy_(w)
                getattr(m, name).bias.copy_(b)
    H, W, reps, N = args.height, args.width, args.reps, args.context_compare
    g = torch.Generator(device="cuda").manual_seed(5)
    x1 = torch.rand(1, 3, H, W, device="cuda", generator=g)
    xn = torch.rand(N, 3, H, W, device="cuda", generator=g)
    x_odd = torch.rand(N, 3, 500, 750, device="cuda", generator=g)
    out = {"metric": f"checkerboard context, convs against the fused kernel, 3 x {H} x {W}, weight cache, best of {reps} "
                     "alternating reps", "unit": "ms", "reps": reps, "weight_scale": args.scale, "images": N,
           "compute_dtype": "fp32_split",
           "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0), "
                   "seeded normal context weights"}
    with torch.no_grad(), F.weight_cache():
        # (a) one image: forward, compress, decompress
        data = {}
        for k, m in models.items():
            for _ in range(2):
                data[k] = m.compress(x1)
                same = bool(torch.equal(m.decompress(data[k]), m(x1)[0]))
            out[f"{k}_decompress_equals_forward"] = same
            out[f"{k}_bytes_n1"] = len(data[k])
        fns = {"forward": lambda m, k: m(x1), "compress": lambda m, k: m.compress(x1),
               "decompress": lambda m, k: m.decompress(data[k])}
        t = {(f, k): [] for f in fns for k in models}
        for _ in range(reps):
            for f, fn in fns.items():
                for k, m in models.items():
                    t[f, k].append(_wall(lambda: fn(m, k), 1))
        for (f, k), v in t.items():
            out[f"{k}_{f}_ms_n1"] = round(min(v), 4)
        # the context alone, by device events, on that image's latent and on the N images'; 10 calls between the events
        calls = 10
        for tag_, x in (("n1", x1), (f"n{N}", xn)):
            m = models["fused"]
            y = m.analysis_transform(x)
            sigma_h, mu_h = m._prior(torch.round(m.prior_analysis(y)))
            y_in = torch.round(y - mu_h) + mu_h
            for k, mk in models.items():
                mk._context(y_in, sigma_h, mu_h)
                ms = _events(lambda: [mk._context(y_in, sigma_h, mu_h) for _ in range(calls)], reps) / calls
                out[f"{k}_context_alone_ms_{tag_}"] = round(ms, 5)
            (sc, mc), (sf, mf) = (mk._context(y_in, sigma_h, mu_h) for mk in models.values())
            out[f"context_max_diff_over_max_mu_sigma_{tag_}"] = [float((mc - mf).abs().max() / mc.abs().max()),
                                                                float((sc - sf).abs().max() / sc.abs().max())]
            out[f"context_latent_{tag_}"] = list(y.shape)
        # (b) N images: the conv model's loop of single-image batches against the fused model's per-image streams
        conv, fused = models["conv"], models["fused"]
        loop_c = lambda: [conv.compress(xn[n:n + 1]) for n in range(N)]
        loop_d = lambda: [conv.decompress(d) for d in datas]
        each_c = lambda: fused.compress_each(xn)
        each_d = lambda: fused.decompress_each(streams)
        for _ in range(2):
            datas, streams, odd = loop_c(), each_c(), fused.compress_each(x_odd)
            loop_d(), each_d(), fused.decompress_each(odd)
        # the streams decoded one at a time against all together: the latents are the same bits (tests/test_context_gpu.py),
        # the images follow g_s, whose low bits depend on the batch it runs in
        together = each_d()
        out["decompress_each_alone_max_diff_to_together"] = max(
            float((fused.decompress_each([s])[0] - t).abs().max()) for s, t in zip(streams, together))
        t = {"loop_compress": [], "each_compress": [], "loop_decompress": [], "each_decompress": []}
        for _ in range(reps):
            t["loop_compress"].append(_wall(loop_c, 1))
            t["each_compress"].append(_wall(each_c, 1))
            t["loop_decompress"].append(_wall(loop_d, 1))
            t["each_decompress"].append(_wall(each_d, 1))
        best = {k: min(v) for k, v in t.items()}
        for k, v in best.items():
            out[f"{k}_ms_per_image"] = round(v / N, 4)
        out["each_no_slower_than_loop"] = bool(best["each_compress"] <= best["loop_compress"]
                                               and best["each_decompress"] <= best["loop_decompress"])
        out["all_reps_ms_per_batch"] = {k: [round(u, 3) for u in v] for k, v in t.items()}
        out["padded_500x750_each_compress_ms_per_image"] = round(_wall(lambda: fused.compress_each(x_odd), reps) / N, 4)
        out["padded_500x750_each_decompress_ms_per_image"] = round(_wall(lambda: fused.decompress_each(odd), reps) / N, 4)
        # (c) bytes: "ICRK" per image against "ICRC" version 2 of single-image batches and the mean-scale "ICRP"
        abi = int(_lib.load().ic_version())
        batch1 = [fused.compress(xn[n:n + 1]) for n in range(N)]
        icrp = mean.compress_each(xn)
        hk = [codec.parse_checkerboard_image(d, abi, "fp32_split")[0] for d in streams]
        out["bytes_icrk"], out["bytes_icrc_v2_single_image_batches"] = sum(map(len, streams)), sum(map(len, batch1))
        out["bytes_icrc_v1_single_image_batches"], out["bytes_mean_scale_icrp"] = sum(map(len, datas)), sum(map(len, icrp))
        out["bytes_icrk_500x750"] = sum(map(len, odd))
        # with a zero context the symbols are the mean-scale model's: what is left is the container
        zero = _build(CK, args.scale, "fused")[0].compress_each(xn)
        out["bytes_icrk_zero_context"] = sum(map(len, zero))
        out["icrk_zero_context_minus_icrp_per_image"] = [len(a) - len(b) for a, b in zip(zero, icrp)]
        out["icrk_minus_icrc_v2_per_image"] = [len(a) - len(b) for a, b in zip(streams, batch1)]
        out["header_bytes"] = {"ICRK": codec._CKBD_IMAGE_HEAD.size, "ICRC": codec._CKBD_HEAD.size, "ICRP": codec._IMAGE_HEAD.size}
        out["fixed_bytes_icrk"] = [codec.checkerboard_image_fixed_bytes(h) for h in hk]
        out["fixed_bytes_mean_scale_icrp"] = [codec.image_fixed_bytes(codec.parse_image(d, abi, "fp32_split")[0]) for d in icrp]
        out["kmax_y_icrk"] = [h.kmax_y for h in hk]
    return out


def gained_bench(args):
    """--gained N: the mean-scale model and the model with gain units, one repetition of each at a time."""
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    from image_compression_amd.step import TrainStep
    archs = ("MeanScaleCompressor2018", "GainedMeanScaleCompressor2018")
    GAINED = archs[1]
    models = {a: _build(a, 1.0)[0] for a in archs}      # seed weights, zero tables: the same symbols
    H, W, reps, N = args.height, args.width, args.reps, args.gained
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {"metric": f"mean-scale codec with and without gain units at 3 x {H} x {W}, weight cache, best of {reps} "
                     "alternating reps", "unit": "ms", "reps": reps,
           "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0)"}
    x = torch.rand(1, 3, H, W, device="cuda", generator=g)
    with torch.no_grad(), F.weight_cache():
        data = {}
        for a, m in models.items():
            for _ in range(2):                               # warm-up of every candidate
                data[a] = m.compress(x)
                same = bool(torch.equal(m.decompress(data[a]), m(x)[0]))
            out[f"{a}_decompress_equals_forward"] = same
            out[f"{a}_bytes"] = len(data[a])
        out["same_payload"] = data[archs[0]][codec._HEAD.size:] == data[GAINED][codec._GAINED_HEAD.size:]
        fns = {"forward": lambda m, a: m(x), "compress": lambda m, a: m.compress(x),
               "decompress": lambda m, a: m.decompress(data[a])}
        t = {(k, a): [] for k in fns for a in archs}
        for _ in range(reps):
            for k, fn in fns.items():
                for a, m in models.items():
                    t[k, a].append(_wall(lambda: fn(m, a), 1))
        for (k, a), v in t.items():
            out[f"{a}_{k}_ms"] = round(min(v), 4)
            out[f"{a}_{k}_all_ms"] = [round(u, 3) for u in v]
        # the gain kernels beside ic_center_round, by device events on the y of N images; 20 calls between the events
        m = models[GAINED]
        gops, mops = _lib.gain_ops(), _lib.mean_ops()
        xn = torch.rand(N, 3, H, W, device="cuda", generator=g)
        y = m.analysis_transform(xn)
        _, mu = m._prior(torch.round(m.prior_analysis(y)))
        y_l, m_l = y.movedim(1, -1).contiguous(), mu.movedim(1, -1).contiguous()
        dy = torch.rand_like(y_l)
        gv = gops.gain_vector(m.gain.log_y, [2.5])
        gn = gops.gain_vector(m.gain.log_y, [2.5] * N)
        calls = 20
        per = lambda fn: _events(lambda: [fn() for _ in range(calls)], reps) / calls
        n = y_l.numel()
        kern = {   # name: (ms per call, bytes the kernel must move)
            "center_round": (per(lambda: mops.center_round(y_l, m_l)), 16 * n),
            "channel_scale": (per(lambda: gops.channel_scale(y_l, gv)), 8 * n),
            "channel_scale_per_image": (per(lambda: gops.channel_scale(y_l, gn)), 8 * n),
            "channel_scale_bwd": (per(lambda: gops.channel_scale_bwd(y_l, gv, dy)), 12 * n),
            "channel_scale_bwd_per_image": (per(lambda: gops.channel_scale_bwd(y_l, gn, dy)), 12 * n),
            "gain_vector": (per(lambda: gops.gain_vector(m.gain.log_y, [2.5])), 4 * 3 * y_l.shape[-1]),
            "gain_vector_bwd": (per(lambda: gops.gain_vector_bwd(gv, gv, m.levels, [2.5])),
                                4 * (2 + m.levels) * y_l.shape[-1]),
        }
        out["kernels_ms_per_call"] = {k: round(v, 5) for k, (v, _) in kern.items()}
        out["kernels_bytes"] = {k: b for k, (_, b) in kern.items()}
        out["kernels_gb_per_s"] = {k: round(b / v / 1e6, 1) for k, (v, b) in kern.items()}
        out["kernels_values"], out["kernels_images"], out["kernels_calls_between_events"] = n, N, calls
        # coded bytes at every integer level of a ladder of gains, on scaled weights (a table, not a rate result)
        ms = _build(GAINED, args.scale)[0]
        for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
            getattr(ms.gain, name).copy_(sign * 0.3 * torch.arange(ms.levels, device="cuda").view(-1, 1))
        ladder = []
        for s in range(ms.levels):
            ms.set_quality(s)
            d = ms.compress(x)
            h = codec.parse_gained(d, int(_lib.load().ic_version()), "fp32_split")[0]
            x_hat = ms.decompress(d)
            ladder.append({"quality": s, "bytes": len(d), "coded_bpp": round(8 * len(d) / (H * W), 5), "kmax_z": h.kmax_z,
                           "kmax_y": h.kmax_y, "decompress_equals_forward": bool(torch.equal(x_hat, ms(x)[0])),
                           "mse": float(((x_hat - x) ** 2).mean())})
        out["ladder_0.3_per_level"], out["ladder_weight_scale"] = ladder, args.scale
    # one eager training step of both at 32 x 256 x 256
    xt = torch.rand(32, 3, 256, 256, device="cuda", generator=g)
    steps = {a: TrainStep(_build(a, 1.0)[0].train(), xt, graph=False) for a in archs}
    for _ in range(3):
        for st in steps.values():
            st()
    t = {a: [] for a in archs}
    for _ in range(reps):
        for a, st in steps.items():
            t[a].append(_wall(st, 1))
    for a, v in t.items():
        out[f"{a}_train_step_32x256x256_ms"] = round(min(v), 3)
        out[f"{a}_train_step_32x256x256_all_ms"] = [round(u, 3) for u in v]
    return out


def region_bench(args):
    """--region N: the gained model at a scalar quality and the region model at a two-code map, one repetition of
    each at a time."""
    import numpy as np
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    from image_compression_amd.step import TrainStep
    archs = ("GainedMeanScaleCompressor2018", "RegionGainedMeanScaleCompressor2018")
    GAINED, REGION = archs
    H, W, reps, N = args.height, args.width, args.reps, args.region
    hb, wb = H // 64, W // 64
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {"metric": f"gained codec with a scalar quality and with a quality map at 3 x {H} x {W}, weight cache, best of "
                     f"{reps} alternating reps", "unit": "ms", "reps": reps, "weight_scale": args.scale,
           "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0), "
                   "ladder tables +-0.3 per level"}

    def ladder(m):
        for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
            getattr(m.gain, name).copy_(sign * 0.3 * torch.arange(m.levels, device="cuda").view(-1, 1))
        return m

    def centre(lo, hi):
        """A centre rectangle of a quarter of the blocks at level `hi` over a background at level `lo`."""
        return codec.block_map(H, W, 6, lo, [(64 * (hb // 4), 64 * (wb // 4), 64 * (hb // 2), 64 * (wb // 2), hi)])

    x = torch.rand(1, 3, H, W, device="cuda", generator=g)
    with torch.no_grad(), F.weight_cache():
        models = {a: ladder(_build(a, args.scale)[0]) for a in archs}
        models[GAINED].set_quality(3.0)
        two = centre(1, 5)
        models[REGION].set_quality_map(two)
        out["map_codes"], out["map_blocks"] = sorted(set(two.reshape(-1).tolist())), [hb, wb]
        data = {}
        for a, m in models.items():
            for _ in range(2):                               # warm-up of every candidate
                data[a] = m.compress(x)
                same = bool(torch.equal(m.decompress(data[a]), m(x)[0]))
            out[f"{a}_decompress_equals_forward"] = same
            out[f"{a}_bytes"] = len(data[a])
        fns = {"forward": lambda m, a: m(x), "compress": lambda m, a: m.compress(x),
               "decompress": lambda m, a: m.decompress(data[a])}
        t = {(k, a): [] for k in fns for a in archs}
        for _ in range(reps):
            for k, fn in fns.items():
                for a, m in models.items():
                    t[k, a].append(_wall(lambda: fn(m, a), 1))
        for (k, a), v in t.items():
            out[f"{a}_{k}_ms"] = round(min(v), 4)
            out[f"{a}_{k}_all_ms"] = [round(u, 3) for u in v]
        for k in fns:
            out[f"region_minus_gained_{k}_ms"] = round(min(t[k, REGION]) - min(t[k, GAINED]), 4)
            out[f"gained_{k}_scatter_ms"] = round(max(t[k, GAINED]) - min(t[k, GAINED]), 4)
        # the kernels by device events on the y of N images; the candidates alternate inside every repetition
        m = models[REGION]
        gops, rops, ops = _lib.gain_ops(), _lib.region_ops(), _lib.ops()
        xn = torch.rand(N, 3, H, W, device="cuda", generator=g)
        y_l = m.analysis_transform(xn).movedim(1, -1).contiguous()
        dy = torch.rand_like(y_l)
        Cy = y_l.shape[-1]
        gn = gops.gain_vector(m.gain.log_y, [float(n % 6) for n in range(N)])
        g3 = gops.gain_vector(m.gain.log_y, [1.0, 2.686, 5.0])
        idx = torch.randint(0, 3, (N, hb, wb), device="cuda", generator=g).to(torch.uint8)
        w3 = torch.tensor([512.0, 1647.0, 8192.0], device="cuda")
        xt = torch.rand(N, 3, H, W, device="cuda", generator=g)
        one = torch.ones((), device="cuda")
        calls = 20
        kern = {   # name: (the call, bytes the kernel must move)
            "channel_scale_per_image": (lambda: gops.channel_scale(y_l, gn), 8 * y_l.numel()),
            "block_scale": (lambda: rops.block_scale(y_l, g3, idx, 2), 8 * y_l.numel()),
            "channel_scale_bwd_per_image": (lambda: gops.channel_scale_bwd(y_l, gn, dy), 12 * y_l.numel()),
            "block_scale_bwd": (lambda: rops.block_scale_bwd(y_l, g3, idx, dy, 2), 12 * y_l.numel()),
            "mse_fwd": (lambda: ops.mse_fwd(xn, xt), 8 * xn.numel()),
            "block_mse_fwd": (lambda: rops.block_mse_fwd(xn, xt, w3, idx), 8 * xn.numel()),
            "mse_bwd": (lambda: ops.mse_bwd(xn, xt, one, False, True), 12 * xn.numel()),
            "block_mse_bwd": (lambda: rops.block_mse_bwd(xn, xt, w3, idx, one, False, True), 12 * xn.numel()),
        }
        for fn, _ in kern.values():
            fn()
        tk = {k: [] for k in kern}
        for _ in range(reps):
            for k, (fn, _) in kern.items():
                tk[k].append(_events(lambda: [fn() for _ in range(calls)], 1) / calls)
        out["kernels_ms_per_call"] = {k: round(min(v), 5) for k, v in tk.items()}
        out["kernels_all_ms_per_call"] = {k: [round(u, 5) for u in v] for k, v in tk.items()}
        out["kernels_bytes"] = {k: b for k, (_, b) in kern.items()}
        out["kernels_gb_per_s"] = {k: round(kern[k][1] / min(v) / 1e6, 1) for k, v in tk.items()}
        out["kernels_latent_shape"], out["kernels_calls_between_events"] = list(y_l.shape), calls
        ratio = min(tk["block_scale"]) / min(tk["channel_scale_per_image"])
        out["block_scale_over_channel_scale"], out["block_scale_within_1.25x"] = round(ratio, 3), bool(ratio <= 1.25)
        assert Cy == g3.shape[1]
        # bytes following the map, on the ladder tables (a table, not a rate-distortion claim: no trained weights)
        m = models[REGION]
        rate = []
        for name, codes in (("level 1 everywhere", centre(1, 1)), ("level 5 everywhere", centre(5, 5)),
                            ("centre quarter at 5 over 1", two)):
            m.set_quality_map(codes)
            d = m.compress(x)
            h = codec.parse_region(d, int(_lib.load().ic_version()), "fp32_split")[0]
            rate.append({"map": name, "bytes": len(d), "coded_bpp": round(8 * len(d) / (H * W), 5), "kmax_z": h.kmax_z,
                         "kmax_y": h.kmax_y, "blocks_at_5": int(np.sum(codes == 255)),
                         "decompress_equals_forward": bool(torch.equal(m.decompress(d), m(x)[0]))})
        out["rate_table"] = rate
    # one eager training step of both at 32 x 256 x 256
    xt = torch.rand(32, 3, 256, 256, device="cuda", generator=g)
    steps = {a: TrainStep(_build(a, 1.0)[0].train(), xt, graph=False) for a in archs}
    for _ in range(3):
        for st in steps.values():
            st()
    t = {a: [] for a in archs}
    for _ in range(reps):
        for a, st in steps.items():
            t[a].append(_wall(st, 1))
    for a, v in t.items():
        out[f"{a}_train_step_32x256x256_ms"] = round(min(v), 3)
        out[f"{a}_train_step_32x256x256_all_ms"] = [round(u, 3) for u in v]
    return out


def rdmap_bench(args):
    """--rdmap N: the map kernels beside the reductions that read the same bytes, by device events on the likelihoods
    and images of N images; rate_distortion_map beside the eval forward at one image on the gained and the region
    model; and per image the estimated bytes beside the bytes of its stream.  Candidates alternate inside every
    repetition."""
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    archs = ("GainedMeanScaleCompressor2018", "RegionGainedMeanScaleCompressor2018")
    GAINED, REGION = archs
    H, W, reps, N = args.height, args.width, args.reps, args.rdmap
    hb, wb = -(-H // 64), -(-W // 64)
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {"metric": f"rate / distortion maps at {N} x 3 x {H} x {W} (kernels) and 1 x 3 x {H} x {W} (model), weight "
                     f"cache, best of {reps} alternating reps", "unit": "ms", "reps": reps, "weight_scale": args.scale,
           "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0), "
                   "ladder tables +-0.3 per level"}
    x = torch.rand(1, 3, H, W, device="cuda", generator=g)
    xn = torch.rand(N, 3, H, W, device="cuda", generator=g)
    with torch.no_grad(), F.weight_cache():
        models = {a: _build(a, args.scale)[0] for a in archs}
        for m in models.values():
            for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
                getattr(m.gain, name).copy_(sign * 0.3 * torch.arange(m.levels, device="cuda").view(-1, 1))
        models[GAINED].set_quality(3.0)
        models[REGION].set_quality_map(codec.block_map(64 * hb, 64 * wb, 6, 1, [(64 * (hb // 4), 64 * (wb // 4),
                                                                                 64 * (hb // 2), 64 * (wb // 2), 5)]))
        # the model: rate_distortion_map beside the eval forward
        fns = {"forward": lambda m: m(x), "rate_distortion_map": lambda m: m.rate_distortion_map(x)}
        for m in models.values():
            for fn in fns.values():
                for _ in range(2):
                    fn(m)
        t = {(k, a): [] for k in fns for a in archs}
        for _ in range(reps):
            for k, fn in fns.items():
                for a, m in models.items():
                    t[k, a].append(_wall(lambda: fn(m), 1))
        for (k, a), v in t.items():
            out[f"{a}_{k}_ms"] = round(min(v), 4)
            out[f"{a}_{k}_all_ms"] = [round(u, 3) for u in v]
        for a in archs:
            out[f"{a}_map_minus_forward_ms"] = round(min(t["rate_distortion_map", a]) - min(t["forward", a]), 4)
        # the kernels by device events
        m = models[GAINED]
        rd = m.rate_distortion_map(xn, likelihoods=True)
        mops, ops = _lib.map_ops(), _lib.ops()
        p_y, p_z, xh = rd.p_y, rd.p_z, rd.x_hat.contiguous()
        calls = 20
        kern = {   # name: (the call, bytes the kernel must move)
            "ce_loss_fwd_y": (lambda: ops.ce_loss_fwd(p_y), 4 * p_y.numel()),
            "block_bits_y": (lambda: mops.block_bits(p_y, 2), 4 * p_y.numel()),
            "ce_loss_fwd_z": (lambda: ops.ce_loss_fwd(p_z), 4 * p_z.numel()),
            "block_bits_z": (lambda: mops.block_bits(p_z, 0), 4 * p_z.numel()),
            "block_bits_z_add": (lambda: mops.block_bits(p_z, 0, rd.bits_y), 4 * p_z.numel()),
            "mse_fwd": (lambda: ops.mse_fwd(xn, xh), 8 * xn.numel()),
            "block_sse": (lambda: mops.block_sse(xn, xh, 6), 8 * xn.numel()),
            "block_sse_as_the_model_calls_it": (lambda: mops.block_sse(xn, rd.x_hat, 6), 8 * xn.numel()),
        }
        for fn, _ in kern.values():
            fn()
        tk = {k: [] for k in kern}
        for _ in range(reps):
            for k, (fn, _) in kern.items():
                tk[k].append(_events(lambda: [fn() for _ in range(calls)], 1) / calls)
        out["kernels_ms_per_call"] = {k: round(min(v), 5) for k, v in tk.items()}
        out["kernels_all_ms_per_call"] = {k: [round(u, 5) for u in v] for k, v in tk.items()}
        out["kernels_bytes"] = {k: b for k, (_, b) in kern.items()}
        out["kernels_gb_per_s"] = {k: round(kern[k][1] / min(v) / 1e6, 1) for k, v in tk.items()}
        out["kernels_shapes"] = {"p_y": list(p_y.shape), "p_y_strides": list(p_y.stride()), "p_z": list(p_z.shape),
                                 "p_z_strides": list(p_z.stride()), "x_hat_strides": list(rd.x_hat.stride())}
        out["kernels_calls_between_events"] = calls
        for new, old in (("block_bits_y", "ce_loss_fwd_y"), ("block_bits_z", "ce_loss_fwd_z"), ("block_sse", "mse_fwd")):
            ratio = min(tk[new]) / min(tk[old])
            out[f"{new}_over_{old}"], out[f"{new}_within_1.25x"] = round(ratio, 3), bool(ratio <= 1.25)
        # per image: the estimate beside the stream (a table, not a claim: no trained weights)
        table = []
        for a, m in models.items():
            rd, streams = m.rate_distortion_map(xn), m.compress_each(xn)
            bits = rd.bits.double().sum(dim=(1, 2)).cpu().tolist()
            table += [{"arch": a, "image": n, "estimated_bytes": round(bits[n] / 8, 1), "stream_bytes": len(streams[n]),
                       "stream_minus_estimate": round(len(streams[n]) - bits[n] / 8, 1)} for n in range(N)]
        out["bytes_table"] = table
    return out


def budget_bench(args):
    """--budget N: coding 8 images to a budget of N bytes each, (a) by the naive search from public calls --
    compress_each at every grid quality, then at every refinement, the choice rule of codec.py on len() -- and (b) by
    compress_each_to with the same candidates and rounds; alternately in one process, device synchronised inside
    the timed region.  Then measure_seg beside encode_seg (encode + compact) on the y symbols of one round's
    candidates, by device events."""
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    from image_compression_amd.modelling.blocks.entropy_model import table_pool
    N, H, W, reps, budget = 8, 512, 768, args.reps, args.budget
    Q, rounds, R = args.candidates, args.rounds, 1024
    scale = 32.0
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(N, 3, H, W, device="cuda", generator=g)
    x *= torch.linspace(0.25, 1.0, N, device="cuda").view(N, 1, 1, 1)    # images that differ in their rate
    out = {"metric": f"coding {N} x 3 x {H} x {W} to {budget} bytes per image: naive search from compress_each against "
                     f"compress_each_to, {Q} candidates, {rounds} rounds, weight cache, best of {reps} alternating reps",
           "unit": "ms per call", "reps": reps, "weight_scale": scale, "budget": budget, "candidates": Q, "rounds": rounds,
           "data": "synthetic uniform [0,1) images scaled by 0.25 .. 1, resident in HBM; random-init weights (reference "
                   "init, seed 0), ladder tables +-0.3 per level"}
    with torch.no_grad(), F.weight_cache():
        model = _build("GainedMeanScaleCompressor2018", scale)[0]
        for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
            getattr(model.gain, name).copy_(sign * 0.3 * torch.arange(model.levels, device="cuda").view(-1, 1))
        S = model.levels
        calls = {"naive": 0}

        def naive():
            """Every image searches in every round: one compress_each per distinct candidate quality of the round,
            each image at its own candidate (images that have stopped ride along at their choice)."""
            seen = [{} for _ in range(N)]
            best = [None] * N
            todo = {n: codec.budget_grid(S, Q) for n in range(N)}
            for rnd in range(rounds):
                if not todo:
                    break
                width = max(len(v) for v in todo.values())
                new = [{} for _ in range(N)]
                for k in range(width):
                    qs = [todo[n][k] if n in todo and k < len(todo[n]) else (best[n][0] if best[n] else 0.0) for n in range(N)]
                    model.set_quality(qs)
                    streams = model.compress_each(x, steps_per_chunk=R)
                    calls["naive"] += 1
                    for n in todo:
                        if k < len(todo[n]):
                            new[n][qs[n]] = streams[n]
                for n in list(todo):
                    seen[n].update((q, len(s)) for q, s in new[n].items())
                    qs = sorted(new[n])
                    pick = codec.budget_choice(qs, [len(new[n][q]) for q in qs], budget)
                    if pick is None and rnd == 0:
                        pick = qs[0]
                        best[n] = (pick, new[n][pick])
                        del todo[n]
                        continue
                    if pick is not None:
                        best[n] = (pick, new[n][pick])
                    nxt = codec.budget_next(seen[n], best[n][0])
                    todo[n] = [] if nxt is None else codec.budget_refine(best[n][0], nxt, Q)
                    if not todo[n]:
                        del todo[n]
            return [b[1] for b in best], [b[0] for b in best]

        def fused():
            return model.compress_each_to(x, budget, steps_per_chunk=R, candidates=Q, rounds=rounds, strict=False)

        quality = model.quality
        for _ in range(2):
            a, b = naive(), fused()
        calls["naive"] = 0
        a, b = naive(), fused()
        out["naive_compress_each_calls"] = calls["naive"]
        out["same_streams"] = bool(a[0] == b[0] and a[1] == b[1])
        out["qualities"], out["stream_bytes"] = b[1], [len(s) for s in b[0]]
        out["within_budget"] = [len(s) <= budget for s in b[0]]
        t = {"naive": [], "compress_each_to": []}
        for _ in range(reps):
            t["naive"].append(_wall(naive, 1))
            t["compress_each_to"].append(_wall(fused, 1))
        model.set_quality(quality)
        for k, v in t.items():
            out[f"{k}_ms"], out[f"{k}_all_ms"] = round(min(v), 3), [round(u, 3) for u in v]
        out["compress_each_to_over_naive"] = round(min(t["compress_each_to"]) / min(t["naive"]), 4)
        out["compress_each_to_no_slower"] = bool(min(t["compress_each_to"]) <= min(t["naive"]))

        # the kernels by device events: the y symbols of one round's candidates (every image at every grid quality)
        cm = model.conditional_model
        cands = [(n, q) for n in range(N) for q in codec.budget_grid(S, Q)]
        img, qs = [n for n, _ in cands], [q for _, q in cands]
        M = len(cands)
        y = model.analysis_transform(x)
        z = model.prior_analysis(y)
        g_y, _, g_z, g_inv_z = model.gain(qs)
        from image_compression_amd.modelling.blocks.entropy_model import symbolize_seg, symbols_as_tensor
        z_sym, _ = symbolize_seg(F.channel_scale(z[torch.as_tensor(img, device="cuda")], g_z))
        z_hat = F.channel_scale(symbols_as_tensor(z_sym.float(), (M, *z.shape[1:])), g_inv_z)
        sigma, mean = model._prior_each(z_hat)
        y_sym, ky = F.gain_symbolize_seg(y, g_y, mean, img)
        rows = cm.scale_rows(sigma.expand_as(mean))
        pool, nrows, ks, offs = table_pool(lambda K: cm.tables(K, "cuda"), ky)
        kern = {
            "measure_seg": lambda: F.measure_seg(y_sym, M, rows, 0, pool, nrows, ks, offs, R),
            "encode_seg_and_compact_seg": lambda: _lib.stream_ops().encode_seg(y_sym, M, rows, 0, pool, nrows, ks, offs, R),
            "gain_symbolize_seg": lambda: F.gain_symbolize_seg(y, g_y, mean, img),
            "gather_channel_scale_symbolize_mean_seg": lambda: _lib.mean_ops().symbolize_seg(
                F._to_last(F.channel_scale(y[torch.as_tensor(img, device="cuda")], g_y)), F._to_last(mean), M),
        }
        for fn in kern.values():
            fn()
        tk = {k: [] for k in kern}
        for _ in range(reps):
            for k, fn in kern.items():
                tk[k].append(_events(fn, 1))
        out["kernels_ms"] = {k: round(min(v), 4) for k, v in tk.items()}
        out["kernels_all_ms"] = {k: [round(u, 4) for u in v] for k, v in tk.items()}
        out["kernels_segments"], out["kernels_symbols_per_segment"] = M, y_sym.numel() // M
        out["kernels_chunks"] = M * codec.num_chunks(y_sym.numel() // M, R)
        out["kernels_kmax_y"] = [min(ky), max(ky)]
        out["kernels_note"] = ("device events around one call; the two symbolizers include their copy of the maxima and "
                               "their stream wait, encode_seg_and_compact_seg allocates its worst-case buffers")
    return out


def map_budget_bench(args):
    """--map-budget N: coding 8 images to a budget of N bytes each with a quality map per image, (a) by the naive search
    from public calls -- S rate_distortion_map calls for the tables, the allocation rule in numpy, set_quality_map +
    compress_each per candidate slope, the choice rule of codec.py on len() -- and (b) by compress_each_map_to with the
    same candidates and rounds; alternately in one process, device synchronised inside the timed region.  Then, for the
    record, the measured squared error of every image under its chosen map beside the gained model's compress_each_to
    (one quality per image) at the same budget, same state dict."""
    import numpy as np
    from image_compression_amd import codec
    from image_compression_amd import functional as F
    N, H, W, reps, budget = 8, 512, 768, args.reps, args.map_budget
    Q, rounds, R = args.candidates, args.rounds, 1024
    scale = 32.0
    hb, wb = H // codec.MAP_BLOCK, W // codec.MAP_BLOCK
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(N, 3, H, W, device="cuda", generator=g) - 0.5
    amp = 0.05 + 0.95 * torch.rand(N, 1, hb, wb, device="cuda", generator=g)     # blocks that differ in activity
    x = 0.5 + x * amp.repeat_interleave(codec.MAP_BLOCK, 2).repeat_interleave(codec.MAP_BLOCK, 3)
    # untrained weights: the squared error hardly depends on the level, so the weights of the levels are spread until the
    # slopes of the grid lie on both sides of the crossing of rate and distortion (tests/test_mapbudget_gpu.py, WIDE)
    weights = [10.0 ** (1 + l) for l in range(6)]
    out = {"metric": f"coding {N} x 3 x {H} x {W} to {budget} bytes per image with a quality map: naive search from "
                     f"rate_distortion_map, set_quality_map and compress_each against compress_each_map_to, {Q} candidates, "
                     f"{rounds} rounds, weight cache, best of {reps} alternating reps",
           "unit": "ms per call", "reps": reps, "weight_scale": scale, "budget": budget, "candidates": Q, "rounds": rounds,
           "loss_weights": weights,
           "data": "synthetic uniform noise about 0.5 with an amplitude of 0.05 .. 1 per 64 x 64 block, resident in HBM; "
                   "random-init weights (reference init, seed 0), ladder tables +-0.3 per level"}
    with torch.no_grad(), F.weight_cache():
        model = _build("RegionGainedMeanScaleCompressor2018", scale)[0]
        for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
            getattr(model.gain, name).copy_(sign * 0.3 * torch.arange(model.levels, device="cuda").view(-1, 1))
        model.loss_weights = list(weights)
        S = model.levels
        lut = np.asarray(codec.map_level_codes(S), dtype=np.uint8)
        calls = {"compress_each": 0, "rate_distortion_map": 0}

        def naive():
            """The tables from S rate_distortion_map calls; every image searches in every round: one compress_each per
            candidate index of the round, each image under the map of its own candidate slope (images that have stopped
            ride along under their choice)."""
            bits, sse = [], []
            for l in range(S):
                model.set_quality(l)
                rd = model.rate_distortion_map(x)
                calls["rate_distortion_map"] += 1
                bits.append(rd.bits.reshape(N, -1))
                sse.append(rd.sse.reshape(N, -1))
            tb = torch.stack([torch.stack(bits, 1), torch.stack(sse, 1)]).cpu().numpy()      # (2, N, S, nb), one copy

            def map_of(n, t):
                w = codec.map_weight(model.loss_weight(t), x.shape[1])
                return lut[codec.map_allocate(tb[0, n], tb[1, n], w)].reshape(hb, wb)

            seen = [{} for _ in range(N)]
            best = [None] * N
            todo = {n: codec.budget_grid(S, Q) for n in range(N)}
            for rnd in range(rounds):
                if not todo:
                    break
                width = max(len(v) for v in todo.values())
                new = [{} for _ in range(N)]
                for k in range(width):
                    ts = [todo[n][k] if n in todo and k < len(todo[n]) else (best[n][0] if best[n] else 0.0) for n in range(N)]
                    maps = np.stack([map_of(n, t) for n, t in enumerate(ts)])
                    model.set_quality_map(maps)
                    streams = model.compress_each(x, steps_per_chunk=R)
                    calls["compress_each"] += 1
                    for n in todo:
                        if k < len(todo[n]):
                            new[n][ts[n]] = (streams[n], maps[n])
                for n in list(todo):
                    seen[n].update((t, len(s)) for t, (s, _) in new[n].items())
                    ts = sorted(new[n])
                    pick = codec.budget_choice(ts, [len(new[n][t][0]) for t in ts], budget)
                    if pick is None and rnd == 0:
                        best[n] = (ts[0], *new[n][ts[0]])
                        del todo[n]
                        continue
                    if pick is not None:
                        best[n] = (pick, *new[n][pick])
                    nxt = codec.budget_next(seen[n], best[n][0])
                    todo[n] = [] if nxt is None else codec.budget_refine(best[n][0], nxt, Q)
                    if not todo[n]:
                        del todo[n]
            return [b[1] for b in best], [b[2] for b in best], [b[0] for b in best]

        def fused():
            return model.compress_each_map_to(x, budget, steps_per_chunk=R, candidates=Q, rounds=rounds, strict=False)

        for _ in range(2):
            a, b = naive(), fused()
        calls = {k: 0 for k in calls}
        a, b = naive(), fused()
        out["naive_calls"] = dict(calls)
        out["same_streams"] = bool(a[0] == b[0] and a[2] == b[2] and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])))
        out["slopes"], out["stream_bytes"] = b[2], [len(s) for s in b[0]]
        out["within_budget"] = [len(s) <= budget for s in b[0]]
        out["map_levels"] = [sorted({int(k) for k in m.reshape(-1)}) for m in b[1]]
        t = {"naive": [], "compress_each_map_to": []}
        for _ in range(reps):
            t["naive"].append(_wall(naive, 1))
            t["compress_each_map_to"].append(_wall(fused, 1))
        model.set_quality(S - 1)
        for k, v in t.items():
            out[f"{k}_ms"], out[f"{k}_all_ms"] = round(min(v), 3), [round(u, 3) for u in v]
        out["compress_each_map_to_over_naive"] = round(min(t["compress_each_map_to"]) / min(t["naive"]), 4)
        out["compress_each_map_to_no_slower"] = bool(min(t["compress_each_map_to"]) <= min(t["naive"]))

        # for the record only (no trained weights, no rate-distortion claim): the measured squared error per image under
        # the chosen map beside one quality per image from the gained model's compress_each_to, same budget and weights
        gained = _build("GainedMeanScaleCompressor2018", scale)[0]
        gained.load_state_dict(model.state_dict())
        gained.loss_weights = list(weights)
        uniform, qualities = gained.compress_each_to(x, budget, steps_per_chunk=R, candidates=Q, rounds=rounds, strict=False)

        def sse_of(m, streams):
            return [round(float(((x[n:n + 1] - xh) ** 2).sum()), 3) for n, xh in enumerate(m.decompress_each(streams))]

        out["record_only"] = {"note": "measured squared error of the decoded image, per image; untrained weights: no "
                                      "rate-distortion claim",
                              "map_sse": sse_of(model, b[0]), "map_bytes": [len(s) for s in b[0]],
                              "uniform_sse": sse_of(gained, uniform), "uniform_bytes": [len(s) for s in uniform],
                              "uniform_qualities": qualities}
    return out


def refine_bench(args):
    """--refine T: compress_each beside compress_each_refined with T steps on 8 x 3 x 512 x 768 images, alternately in
    one process (wall time, device synchronised inside the timed region); the cost of one refinement step by device
    events, as (the call with T steps - the call with 0 steps) / T; and beside it one g_s forward with its
    input-gradient backward on the same latent, also by device events: the structure says a step costs about that."""
    from image_compression_amd import functional as F
    N, H, W, reps, T = 8, 512, 768, args.reps, args.refine
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(N, 3, H, W, device="cuda", generator=g)
    model, cfg = _build(args.arch, args.scale)
    out = {"metric": f"compress_each and compress_each_refined({T} steps, lr 0.1) at {N} x 3 x {H} x {W}, "
                     f"{cfg.MODEL.COMPUTE_DTYPE}, best of {reps} alternating reps", "unit": "ms", "reps": reps, "steps": T,
           "arch": args.arch, "weight_scale": args.scale,
           "data": "synthetic uniform [0,1) images resident in HBM; random-init weights (reference init, seed 0)"}
    calls = {"compress_each": lambda: model.compress_each(x),
             "compress_each_refined_0": lambda: model.compress_each_refined(x, steps=0),
             "compress_each_refined": lambda: model.compress_each_refined(x, steps=T)}
    for fn in calls.values():
        for _ in range(2):
            fn()
    wall, dev = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            wall[k].append(_wall(fn, 1))
        for k, fn in calls.items():
            dev[k].append(_events(fn, 1))
    for k in calls:
        out[f"{k}_ms_per_image"] = round(min(wall[k]) / N, 4)
        out[f"{k}_all_ms"] = [round(u, 3) for u in wall[k]]
        out[f"{k}_events_ms"] = round(min(dev[k]), 3)
    out["refined_over_plain"] = round(min(wall["compress_each_refined"]) / min(wall["compress_each"]), 3)
    if T:
        out["step_ms_by_events"] = round((min(dev["compress_each_refined"]) - min(dev["compress_each_refined_0"])) / T, 4)
    # one g_s forward and its input-gradient backward on the call's own latent shape, no weight gradient
    streams, report = model.compress_each_refined(x, steps=T)
    out["stream_bytes"] = [len(s) for s in streams]
    out["plain_stream_bytes"] = [len(s) for s in model.compress_each(x)]
    out["j_before"], out["j_after"], out["winning_evaluation"] = report.before, report.after, report.step
    params = list(model.parameters())
    flags = [p.requires_grad for p in params]
    try:
        for p in params:
            p.requires_grad_(False)
        with torch.no_grad():
            y = model.analysis_transform(x)
            gx = torch.ones(N, 3, H, W, device="cuda")

        def gs_pair():
            leaf = y.detach().requires_grad_(True)
            torch.autograd.grad([model._reconstruct(leaf)], [leaf], [gx])

        with F.record_plans() as log:
            gs_pair()
        out["g_s_pair_ops"] = sorted({p["op"] for p in log})
        gs_pair()
        out["g_s_forward_and_dgrad_ms_by_events"] = round(min(_events(gs_pair, 1) for _ in range(reps)), 4)
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)
        model._clear_reparameterised()
    if T:
        out["step_over_g_s_pair"] = round(out["step_ms_by_events"] / out["g_s_forward_and_dgrad_ms_by_events"], 3)
    return out


def transcode_bench(args):
    """--transcode Q2 [--rechunk R] [--transcode-budget BYTES]: 8 x 3 x 512 x 768 images coded at quality S - 1 and taken to
    Q2 (a) through pixels -- decompress_each, set_quality, compress_each -- and (b) by transcode_each, alternately in
    one process, device synchronised inside the timed region; with a budget, transcode_each_to beside the (a)-style
    search (one decompress_each + compress_each per candidate of every round); requant_seg beside the four ops it
    replaces on the same operands, by device events; and the PSNR and the sizes of both routes beside direct coding."""
    from image_compression_amd import _lib, codec
    from image_compression_amd import functional as F
    N, H, W, reps, q2 = 8, 512, 768, args.reps, float(args.transcode)
    Q, rounds, R1 = args.candidates, args.rounds, 1024
    R2 = args.rechunk or None
    scale = 32.0
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(N, 3, H, W, device="cuda", generator=g)
    x *= torch.linspace(0.25, 1.0, N, device="cuda").view(N, 1, 1, 1)    # images that differ in their rate
    out = {"metric": f"{N} x 3 x {H} x {W} streams from quality S - 1 to {q2}"
                     f"{'' if R2 is None else f' and {R2} steps per chunk'}: decompress_each + set_quality + compress_each "
                     f"against transcode_each, weight cache, best of {reps} alternating reps",
           "unit": "ms per call", "reps": reps, "weight_scale": scale, "target_quality": q2, "rechunk": R2,
           "data": "synthetic uniform [0,1) images scaled by 0.25 .. 1, resident in HBM; random-init weights (reference "
                   "init, seed 0), ladder tables +-0.3 per level"}

    def psnr(a, b):
        return round(float(-10.0 * torch.log10(((a - b) ** 2).mean())), 3)

    def timed(routes):
        t = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():
                t[k].append(_wall(fn, 1))
        for k, v in t.items():
            out[f"{k}_ms"], out[f"{k}_all_ms"] = round(min(v), 3), [round(u, 3) for u in v]
        return {k: min(v) for k, v in t.items()}

    with torch.no_grad(), F.weight_cache():
        model = _build("GainedMeanScaleCompressor2018", scale)[0]
        for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
            getattr(model.gain, name).copy_(sign * 0.3 * torch.arange(model.levels, device="cuda").view(-1, 1))
        S = model.levels
        q1 = float(S - 1)
        model.set_quality(q1)
        src = model.compress_each(x, steps_per_chunk=R1)
        out["source_quality"], out["source_bytes"] = q1, [len(s) for s in src]

        def pixels(q=q2, streams=src):
            x_hat = torch.cat(model.decompress_each(streams))
            model.set_quality(q if isinstance(q, float) else list(q))
            return model.compress_each(x_hat, steps_per_chunk=R2 or R1)

        def latent():
            return model.transcode_each(src, qualities=q2, steps_per_chunk=R2)

        for _ in range(2):
            a, b = pixels(), latent()
        best = timed({"through_pixels": pixels, "transcode_each": latent})
        out["transcode_each_over_through_pixels"] = round(best["transcode_each"] / best["through_pixels"], 4)
        out["transcode_each_no_slower"] = bool(best["transcode_each"] <= best["through_pixels"])
        model.set_quality(q2)
        direct = model.compress_each(x, steps_per_chunk=R2 or R1)
        out["bytes"] = {"through_pixels": [len(s) for s in a], "transcode_each": [len(s) for s in b],
                        "direct_at_target": [len(s) for s in direct]}
        out["psnr_db"] = {k: psnr(torch.cat(model.decompress_each(v)), x)
                          for k, v in (("source", src), ("through_pixels", a), ("transcode_each", b),
                                       ("direct_at_target", direct))}
        out["psnr_note"] = "random-init weights: recorded, nothing is claimed about rate-distortion"

        if args.transcode_budget:
            budget = args.transcode_budget
            calls = {"naive": 0}

            def naive():
                """The search rule from (a)-style calls: every candidate of every round is one decompress_each +
                set_quality + compress_each of all streams, each at its own candidate."""
                seen = [codec.transcode_measured(q1, len(s)) for s in src]
                best_ = [(q1, s) if len(s) <= budget else None for s in src]
                todo = {n: codec.transcode_grid(S, Q, q1) for n in range(N) if best_[n] is None}
                for rnd in range(rounds):
                    if not todo:
                        break
                    new = [{} for _ in range(N)]
                    for k in range(max(len(v) for v in todo.values())):
                        qs = [todo[n][k] if n in todo and k < len(todo[n]) else 0.0 for n in range(N)]
                        streams = pixels(qs)
                        calls["naive"] += 1
                        for n in todo:
                            if k < len(todo[n]):
                                new[n][qs[n]] = streams[n]
                    for n in list(todo):
                        seen[n].update((q, len(s)) for q, s in new[n].items())
                        qs = sorted(new[n])
                        pick = codec.budget_choice(qs, [len(new[n][q]) for q in qs], budget)
                        if pick is None and rnd == 0:
                            best_[n] = (qs[0], new[n][qs[0]])
                            del todo[n]
                            continue
                        if pick is not None:
                            best_[n] = (pick, new[n][pick])
                        nxt = codec.budget_next(seen[n], best_[n][0])
                        todo[n] = [] if nxt is None else codec.budget_refine(best_[n][0], nxt, Q)
                        if not todo[n]:
                            del todo[n]
                return [v[1] for v in best_], [v[0] for v in best_]

            def searched():
                return model.transcode_each_to(src, budget, steps_per_chunk=R2, candidates=Q, rounds=rounds, strict=False)

            for _ in range(2):
                na, se = naive(), searched()
            calls["naive"] = 0
            na, se = naive(), searched()
            rounds_through_pixels = calls["naive"]
            best = timed({"naive_search_through_pixels": naive, "transcode_each_to": searched})
            out["budget"] = {"bytes": budget, "candidates": Q, "rounds": rounds, "naive_rounds_through_pixels": rounds_through_pixels,
                             "qualities": {"naive": na[1], "transcode_each_to": se[1]},
                             "stream_bytes": {"naive": [len(s) for s in na[0]], "transcode_each_to": [len(s) for s in se[0]]},
                             "within_budget": [len(s) <= budget for s in se[0]],
                             "psnr_db": {"naive": psnr(torch.cat(model.decompress_each(na[0])), x),
                                         "transcode_each_to": psnr(torch.cat(model.decompress_each(se[0])), x)}}
            out["transcode_each_to_over_naive"] = round(best["transcode_each_to"] / best["naive_search_through_pixels"], 4)
            out["transcode_each_to_no_slower"] = bool(best["transcode_each_to"] <= best["naive_search_through_pixels"])

        # the kernel by device events, on the operands of the two calls: every stream to one target (transcode_each),
        # and every stream to every quality of the grid below q1 (one round of transcode_each_to)
        model._codable_each()
        parsed = [model._parse_image(s, int(_lib.load().ic_version()), "fp32_split") for s in src]
        z_hat1, r, mu1, a_inv = model._requant_decode(parsed, list(range(N)))
        rl, m1l = F._to_last(r), F._to_last(mu1)
        out["kernels_ms"], out["kernels_all_ms"] = {}, {}
        for tag, cands in (("each", [(n, q2) for n in range(N)]),
                           ("search", [(n, q) for n in range(N) for q in codec.transcode_grid(S, Q, q1)])):
            img, qs = [n for n, _ in cands], [q for _, q in cands]
            M = len(cands)
            _, _, _, _, _, mu2 = model._requant_targets((z_hat1, r, mu1, a_inv), img, qs)
            g_y = model.gain(qs)[0]
            m2l = F._to_last(mu2)
            idx = torch.as_tensor(img, device="cuda")
            gather = img != list(range(N))

            def four_ops():
                rr, mm, aa = (rl[idx], m1l[idx], a_inv[idx]) if gather else (rl, m1l, a_inv)
                y_hat = _lib.mean_ops().add_mean(rr.reshape(-1), mm).view(mm.shape)
                scaled = _lib.gain_ops().channel_scale(_lib.gain_ops().channel_scale(y_hat, aa), g_y)
                return _lib.mean_ops().symbolize_seg(scaled, m2l, M)

            kern = {"requant_seg": lambda: F.requant_seg(r, mu1, a_inv, g_y, mu2, img),
                    ("gather_" if gather else "") + "add_mean_channel_scale_x2_symbolize_mean_seg": four_ops}
            same = bool(torch.equal(kern["requant_seg"]()[0], four_ops()[0]))
            tk = {k: [] for k in kern}
            for _ in range(reps):
                for k, fn in kern.items():
                    tk[k].append(_events(fn, 1))
            out["kernels_ms"][tag] = {k: round(min(v), 4) for k, v in tk.items()}
            out["kernels_all_ms"][tag] = {k: [round(u, 4) for u in v] for k, v in tk.items()}
            out["kernels_ms"][tag].update(targets=M, symbols_per_target=int(mu2[0].numel()), same_symbols=same)
            times = [min(v) for v in tk.values()]
            out["kernels_ms"][tag]["requant_seg_no_slower"] = bool(times[0] <= times[1])
        model._end_call()
        out["kernels_note"] = ("device events around one call; both symbolizers include their copy of the maxima and their "
                               "stream wait; cache rates, comparable with one another only")
        out["requant_share_of_transcode_each"] = round(out["kernels_ms"]["each"]["requant_seg"] / out["transcode_each_ms"], 4)
    return out


def hs_bench(args):
    """--hs-compare [--budget BYTES]: the two values of MODEL.HYPER_SYNTHESIS.KERNEL on GainedMeanScaleCompressor2018
    ("x32" weights, ladder tables, one state dict), alternately rep by rep in one process, inside weight_cache, device
    synchronised inside the timed region; every repetition is kept.  "conv" is the path of the tree before the switch
    existed, launch for launch: the yardstick.  h_s alone by device events: M maps of z 8 x 12 x 192 (the latent of
    512 x 768) as M batch-1 conv passes (what `_prior_each` ran), one batched conv pass, and one invariant pass."""
    from image_compression_amd import functional as F
    N, H, W, reps = 8, 512, 768, args.reps
    budget, Q, rounds, R = args.budget or 450000, args.candidates, args.rounds, 1024
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(N, 3, H, W, device="cuda", generator=g)
    x *= torch.linspace(0.25, 1.0, N, device="cuda").view(N, 1, 1, 1)
    out = {"metric": f"MODEL.HYPER_SYNTHESIS.KERNEL conv | invariant, GainedMeanScaleCompressor2018, {N} x 3 x {H} x {W}, "
                     f"weight cache, {reps} alternating reps (all kept, best reported)",
           "unit": "ms", "reps": reps, "weight_scale": 32.0, "budget": budget, "candidates": Q, "rounds": rounds,
           "data": "synthetic uniform [0,1) images scaled by 0.25 .. 1, resident in HBM; random-init weights (reference "
                   "init, seed 0), ladder tables +-0.3 per level"}

    def every(fns, timer):
        """{name: [ms of every rep]} of the functions, alternately."""
        got = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                got[k].append(timer(fn, 1))
        return got

    def report(got):
        return {k: {"best": min(v), "worst": max(v), "all": v} for k, v in got.items()}

    with torch.no_grad(), F.weight_cache():
        models = {}
        for hs in ("conv", "invariant"):
            m = _build("GainedMeanScaleCompressor2018", 32.0, hs=hs)[0]
            for name, sign in (("log_y", 1.0), ("log_inv_y", -1.0), ("log_z", 1.0), ("log_inv_z", -1.0)):
                getattr(m.gain, name).copy_(sign * 0.3 * torch.arange(m.levels, device="cuda").view(-1, 1))
            m.set_quality(m.levels - 1)
            models[hs] = m
        for p, q in zip(models["conv"].parameters(), models["invariant"].parameters()):
            assert torch.equal(p, q)
        conv, inv = models["conv"], models["invariant"]
        out["h_s"] = {}
        for M in (1, 8, 64):
            z = torch.round(torch.randn(M, 192, 8, 12, device="cuda", generator=g) * 3)
            fns = {"conv_each": lambda: conv._prior_each(z), "conv_batched": lambda: conv._prior(z),
                   "invariant": lambda: inv._prior_each(z)}
            for fn in fns.values():
                fn()
            out["h_s"][str(M)] = report(every(fns, _events))
        x1 = x[:1].contiguous()
        streams = {k: m.compress_each(x, steps_per_chunk=R) for k, m in models.items()}
        batch1 = {k: m.compress(x1, steps_per_chunk=R) for k, m in models.items()}
        calls = {
            "compress_each": lambda k, m: m.compress_each(x, steps_per_chunk=R),
            "decompress_each": lambda k, m: m.decompress_each(streams[k]),
            "compress_each_to": lambda k, m: m.compress_each_to(x, budget, steps_per_chunk=R, candidates=Q, rounds=rounds,
                                                                strict=False),
            "eval_forward_1": lambda k, m: m(x1),
            "compress_1": lambda k, m: m.compress(x1, steps_per_chunk=R),
            "decompress_1": lambda k, m: m.decompress(batch1[k]),
        }
        out["calls"] = {}
        for name, call in calls.items():
            fns = {k: (lambda k=k, m=m: call(k, m)) for k, m in models.items()}
            for fn in fns.values():
                fn()
            out["calls"][name] = report(every(fns, _wall))
        out["stream_bytes"] = {k: [len(s) for s in v] for k, v in streams.items()}
        to = {k: m.compress_each_to(x, budget, steps_per_chunk=R, candidates=Q, rounds=rounds, strict=False)
              for k, m in models.items()}
        out["compress_each_to_qualities"] = {k: [float(q) for q in v[1]] for k, v in to.items()}
    return out


def _emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
