"""Transcoding in the latent domain without a GPU: the two search-rule functions of codec.py as pure functions and against
an independently written search (`tsearch`, which tests/test_transcode_gpu.py runs on brute-force sizes), header
replacement with pack / parse round trips for "ICRP", "ICRQ" and "ICRR", every refusal of `transcode_each` and
`transcode_each_to` on a host model in front of any launch, the shape kernel of torch.ops.imgcomp_transcode and the
host-side argument checks of ic_requant_seg."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from test_budget import _bumpy, _monotone, grid, refine
from test_gained import _lens, cfg_of

S = 6
ABI = 4


# ------------------------------------------------------------------ the rule, stated on its own
def tsearch(size_of, S_, q1, size1, budget, candidates, rounds):
    """(chosen quality or None, the smallest size of round 1 or None, the qualities measured) for one stream of size1
    bytes at quality q1 whose requantization to q is size_of(q) bytes long: the rule of the issue, written without
    codec.py's functions.  The caller has already found size1 > budget."""
    first = [q for q in grid(S_, candidates) if q < q1]
    seen = {q1: size1}
    if not first:
        return None, None, sorted(seen)
    new = {q: size_of(q) for q in first}
    seen.update(new)
    fit = [q for q, n in new.items() if n <= budget]
    if not fit:
        return None, min(new.values()), sorted(seen)
    chosen = max(fit)
    for _ in range(rounds - 1):
        hi = min(q for q in seen if q > chosen)      # q1 at the latest
        new = {q: size_of(q) for q in refine(chosen, hi, candidates)}
        if not new:
            break
        seen.update(new)
        fit = [q for q, n in new.items() if n <= budget]
        if fit:
            chosen = max(fit)
    return chosen, min(size_of(q) for q in first), sorted(seen)


def _by_codec(size_of, S_, q1, size1, budget, candidates, rounds):
    """The search as `transcode_each_to` runs it, from codec.py's functions alone."""
    from image_compression_amd import codec
    qs = codec.transcode_grid(S_, candidates, q1)
    seen = codec.transcode_measured(q1, size1)
    if not qs:
        return None, None, sorted(seen)
    first = {q: size_of(q) for q in qs}
    seen.update(first)
    chosen = codec.budget_choice(qs, [seen[q] for q in qs], budget)
    if chosen is None:
        return None, min(first.values()), sorted(seen)
    for _ in range(rounds - 1):
        nxt = codec.budget_next(seen, chosen)
        qs = [] if nxt is None else codec.budget_refine(chosen, nxt, candidates)
        if not qs:
            break
        seen.update((q, size_of(q)) for q in qs)
        pick = codec.budget_choice(qs, [seen[q] for q in qs], budget)
        chosen = chosen if pick is None else pick
    return chosen, min(first.values()), sorted(seen)


@pytest.mark.parametrize("Q", [2, 4, 8])
def test_grid_is_the_budget_grid_clipped_strictly_below_the_streams_quality(Q):
    from image_compression_amd import codec
    full = codec.budget_grid(S, Q)
    assert codec.transcode_grid(S, Q, 0.0) == [], "nothing lies below quality 0"
    assert codec.transcode_grid(S, Q, float(S - 1)) == full[:-1]
    for q1 in (0.5, 1.0, float(np.float32(5 / 3)), 2.5, 4.999, 5.0):
        g = codec.transcode_grid(S, Q, q1)
        assert g == [q for q in grid(S, Q) if q < q1] and all(q < q1 for q in g)
        assert g == full[:len(g)] and 0.0 in g
    # a quality that is itself a grid point is not a candidate: transcoding to an equal quality never runs
    for q1 in full[1:]:
        assert q1 not in codec.transcode_grid(S, Q, q1)
    for bad in (-0.5, S - 0.5, float("nan")):
        with pytest.raises(ValueError):
            codec.transcode_grid(S, Q, bad)
    with pytest.raises(ValueError):
        codec.transcode_grid(S, 1, 2.0)


def test_measured_starts_as_the_stream_itself_and_refinement_stays_strictly_inside():
    from image_compression_amd import codec
    q1 = 3.25
    seen = codec.transcode_measured(q1, 4321)
    assert seen == {q1: 4321} and all(isinstance(k, float) for k in seen)
    for bad in (0, -1, 10.0, True, None):
        with pytest.raises(ValueError):
            codec.transcode_measured(q1, bad)
    g = codec.transcode_grid(S, 6, q1)                       # 0 1 2 3
    assert g == [0.0, 1.0, 2.0, 3.0]
    seen.update((q, 100) for q in g)
    assert codec.budget_next(seen, 3.0) == q1, "the top grid point below q1 refines towards q1"
    r = codec.budget_refine(3.0, codec.budget_next(seen, 3.0), 6)
    assert r == refine(3.0, q1, 6) and all(3.0 < q < q1 for q in r) and len(r) == 6
    assert codec.budget_next(seen, 1.0) == 2.0


@pytest.mark.parametrize("size_of", [_monotone, _bumpy], ids=["monotone", "bumpy"])
def test_search_against_the_independent_one(size_of):
    for q1 in (5.0, 3.25, 1.0, 0.5, 0.0):
        size1 = size_of(q1)
        for budget in (999, 1000, 1001, 1299, 1300, 1500, 1900, 2300, 2399, 2400, size1 - 1):
            if budget >= size1 or budget < 1:
                continue
            for rounds in (1, 2, 3):
                got = tsearch(size_of, S, q1, size1, budget, 6, rounds)
                assert got == _by_codec(size_of, S, q1, size1, budget, 6, rounds), (q1, budget, rounds)
                q = got[0]
                if q is not None:
                    assert q < q1 and size_of(q) <= budget
                    assert max(got[2]) == q1, "nothing above the stream's own quality is measured"
    assert tsearch(_monotone, S, 0.0, 1000, 500, 6, 2) == (None, None, [0.0])
    assert tsearch(_monotone, S, 3.25, _monotone(3.25), 999, 6, 2)[:2] == (None, 1000)
    one = tsearch(_monotone, S, 3.25, _monotone(3.25), 3200, 6, 1)[0]
    two = tsearch(_monotone, S, 3.25, _monotone(3.25), 3200, 6, 2)[0]
    assert one == 3.0 and 3.0 < two < 3.25, "round 2 refines between the top grid point and the stream's quality"
    # the hump of the bumpy table: quality 2 fails, 3 and 4 fit
    assert tsearch(_bumpy, S, 5.0, _bumpy(5.0), 2300, 6, 1)[0] == 4.0


# ------------------------------------------------------------------ headers
def _headers(R=16, quality=2.5):
    from image_compression_amd import codec
    common = dict(N=1, H=128, W=192, latent_channels=8, hyper_channels=4, kind=2, compute_dtype="fp32", abi=ABI, L=64,
                  scale_min=0.11, scale_max=256.0, R=R, kmax_z=3, kmax_y=40, height=100, width=136)
    codes = np.arange(6, dtype=np.uint8).reshape(2, 3) * 51
    return {
        "ICRP": (codec.ImageHeader(**common), codec.pack_image, codec.parse_image),
        "ICRQ": (codec.GainedImageHeader(**common, levels=S, quality=quality), codec.pack_gained_image,
                 codec.parse_gained_image),
        "ICRR": (codec.RegionImageHeader(**common, levels=S, map_h=2, map_w=3, codes=codes), codec.pack_region_image,
                 codec.parse_region_image),
    }


@pytest.mark.parametrize("magic", ["ICRP", "ICRQ", "ICRR"])
def test_header_replacement_round_trips_through_the_container(magic):
    from image_compression_amd import codec
    h, pack, parse = _headers()[magic]
    rng = np.random.default_rng(3)
    for R2 in (1, 16, 64, 1024):
        h2 = codec.transcoded_header(h, R=R2)
        assert type(h2) is type(h) and h2 is not h and h.R == 16
        assert dataclasses.replace(h2, R=16) == h, "only R moved"
        lz, ly = _lens(h2.nsym_z, R2, rng), _lens(h2.nsym_y, R2, rng)
        pz, py = bytes(int(lz.sum())), bytes(int(ly.sum()))
        data = pack(h2, lz, ly, pz, py)
        assert data[:4] == magic.encode()
        g, glz, gly, gpz, gpy = parse(data, ABI, "fp32")
        assert g == h2 and g.R == R2 and (g.kmax_z, g.kmax_y) == (3, 40)
        assert np.array_equal(glz, lz) and np.array_equal(gly, ly) and (gpz, gpy) == (pz, py)
        if magic == "ICRR":
            assert np.array_equal(g.codes, h.codes)
    if magic == "ICRQ":
        h2 = codec.transcoded_header(h, R=64, quality=1.25, kmax_z=1, kmax_y=17)
        assert (h2.R, h2.quality, h2.kmax_z, h2.kmax_y, h2.levels) == (64, 1.25, 1, 17, S)
        lz, ly = _lens(h2.nsym_z, 64, rng), _lens(h2.nsym_y, 64, rng)
        g = parse(pack(h2, lz, ly, bytes(int(lz.sum())), bytes(int(ly.sum()))), ABI, "fp32")[0]
        assert g == h2
        assert len(pack(h2, lz, ly, bytes(int(lz.sum())), bytes(int(ly.sum())))) == \
            codec.image_stream_bytes(codec.gained_image_fixed_bytes(h2), lz, ly)
    else:
        with pytest.raises(ValueError, match="quality"):
            codec.transcoded_header(h, quality=1.0)
    for bad in (dict(H=64), dict(levels=5), dict(height=1), dict(codes=None)):
        with pytest.raises(ValueError):
            codec.transcoded_header(h, **bad)
    with pytest.raises(ValueError, match="per-image"):
        codec.transcoded_header(codec.Header(1, 64, 64, 8, 4, 2, "fp32", ABI, 64, 0.11, 256.0, 16, 0, 0), R=4)


# ------------------------------------------------------------------ the refusals, on host models
def _cpu_model(arch="GainedMeanScaleCompressor2018", **kw):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return modelling.build_model(cfg_of(arch, **kw)).eval()


def _stream(model, R=16, size=(60, 50), **changes):
    """A well-formed stream of `model` with made-up chunk lengths and zero payloads: every parser and check takes it."""
    from image_compression_amd import codec
    cm = model.conditional_model
    h, w = size
    H, W = codec.padded_size(h, w)
    common = dict(N=1, H=H, W=W, latent_channels=192, hyper_channels=192, kind=model._stream_kind(),
                  compute_dtype="fp32_split", abi=ABI, L=cm.num_scales, scale_min=cm.scale_min, scale_max=cm.scale_max, R=R,
                  kmax_z=2, kmax_y=9, height=h, width=w)
    name = type(model).__name__
    if name.startswith("Region"):
        codes = np.zeros((H // 64, W // 64), np.uint8)
        hd = codec.RegionImageHeader(**common, levels=model.levels, map_h=H // 64, map_w=W // 64, codes=codes)
    elif name.startswith("Gained"):
        hd = codec.GainedImageHeader(**common, levels=model.levels, quality=2.5)
    else:
        hd = codec.ImageHeader(**common)
    hd = dataclasses.replace(hd, **changes)
    rng = np.random.default_rng(0)
    lz, ly = _lens(hd.nsym_z, hd.R, rng), _lens(hd.nsym_y, hd.R, rng)
    return model._pack_image(hd, lz, ly, bytes(int(lz.sum())), bytes(int(ly.sum())))


def test_transcode_each_validates_before_any_launch():
    """A host model: any launch would raise RuntimeError (no device); every refusal here comes first."""
    model = _cpu_model()
    streams = [_stream(model), _stream(model, size=(100, 136))]
    for bad in (0, -1, 65537, 16.0, True, "16"):
        with pytest.raises(ValueError, match="steps_per_chunk"):
            model.transcode_each(streams, steps_per_chunk=bad)
    for bad in ([1.0], [1.0, 2.0, 3.0], []):
        with pytest.raises(ValueError, match="qualities for 2 streams"):
            model.transcode_each(streams, qualities=bad)
    for bad in (-0.5, S - 0.5, float("nan"), "2", True, None.__class__, [1.0, "x"]):
        with pytest.raises(ValueError, match="quality"):
            model.transcode_each(streams, qualities=bad)
    with pytest.raises(ValueError, match="list of per-image streams"):
        model.transcode_each(streams[0])
    # wrong model, wrong levels, wrong build
    mean = _cpu_model("MeanScaleCompressor2018")
    with pytest.raises(ValueError, match="magic"):
        model.transcode_each([streams[0], _stream(mean)], steps_per_chunk=4)
    with pytest.raises(ValueError, match="magic"):
        mean.transcode_each(streams, steps_per_chunk=4)
    with pytest.raises(ValueError, match="stream 1 .*gain levels"):
        model.transcode_each([streams[0], _stream(model, levels=5)], steps_per_chunk=4)
    with pytest.raises(ValueError, match="ABI"):
        model.transcode_each([_stream(model, abi=5)], steps_per_chunk=4)
    with pytest.raises(ValueError, match="COMPUTE_DTYPE"):
        model.transcode_each([_stream(model, compute_dtype="fp32")], steps_per_chunk=4)
    with pytest.raises(ValueError, match="conditional kind"):
        model.transcode_each([_stream(model, kind=3)], steps_per_chunk=4)
    with pytest.raises(ValueError):
        model.transcode_each([streams[0][:-1]], steps_per_chunk=4)
    q = model.quality
    model.train()
    for call in (lambda: model.transcode_each(streams, steps_per_chunk=4), lambda: model.transcode_each_to(streams, 100)):
        with pytest.raises(RuntimeError, match="eval"):
            call()
    model.eval()
    # nothing to do is done without a launch: the same objects come back
    out = model.transcode_each(streams)
    assert all(a is b for a, b in zip(out, streams))
    out = model.transcode_each(streams, steps_per_chunk=16)
    assert all(a is b for a, b in zip(out, streams))
    out = model.transcode_each(streams, qualities=2.5, steps_per_chunk=16)
    assert all(a is b for a, b in zip(out, streams)), "an equal quality is never requantized"
    # everything passes: the first launch refuses the host model
    for kw in (dict(steps_per_chunk=4), dict(qualities=1.0), dict(qualities=[2.5, 1.0])):
        with pytest.raises(RuntimeError, match="ROCm"):
            model.transcode_each(streams, **kw)
    assert model.quality == q and model._gains is None and model._qualities is None


def test_transcode_each_to_validates_before_any_launch():
    from image_compression_amd import codec
    model = _cpu_model()
    streams = [_stream(model), _stream(model, size=(100, 136)), _stream(model)]
    sizes = [len(s) for s in streams]
    ok = dict(budgets=[n - 1 for n in sizes], candidates=4, rounds=2)

    def call(ss=streams, **kw):
        return model.transcode_each_to(ss, **{**ok, **kw})

    for bad in ([5000, 6000], [5000] * 4, [], [5000, 0, 7000], [5000, -1, 7000], [5000, 6000.0, 7000], 0, -5, 5000.0,
                "5000", None, [True, 6000, 7000], True, np.zeros((3, 1), dtype=np.int64)):
        with pytest.raises(ValueError, match="budget"):
            call(budgets=bad)
    for bad in (1, 65, 0, 4.0, None, True):
        with pytest.raises(ValueError, match="candidates"):
            call(candidates=bad)
    for bad in (0, 5, 2.0, None, False):
        with pytest.raises(ValueError, match="rounds"):
            call(rounds=bad)
    for bad in (0, 65537, 16.0, False):
        with pytest.raises(ValueError, match="steps_per_chunk"):
            call(steps_per_chunk=bad)
    with pytest.raises(ValueError, match="gain levels"):
        call([streams[0], _stream(model, levels=5), streams[2]])
    # streams that fit come back as the same objects with their own qualities, without a launch
    q = model.quality
    out, qs = call(budgets=[sizes[0], sizes[1] + 1, 10 ** 9])
    assert all(a is b for a, b in zip(out, streams)) and qs == [2.5, 2.5, 2.5]
    out, qs = call(budgets=10 ** 9, steps_per_chunk=16)
    assert all(a is b for a, b in zip(out, streams)) and qs == [2.5, 2.5, 2.5]
    # a stream at quality 0 has nothing below it: a miss in front of any launch
    zero = [_stream(model, quality=0.0)]
    with pytest.raises(codec.BudgetError) as err:
        model.transcode_each_to(zero, len(zero[0]) - 1)
    assert (err.value.image, err.value.budget, err.value.smallest) == (0, len(zero[0]) - 1, len(zero[0]))
    out, qs = model.transcode_each_to(zero, len(zero[0]) - 1, strict=False)
    assert out[0] is zero[0] and qs == [0.0]
    for kw in ({}, dict(steps_per_chunk=4)):
        with pytest.raises(RuntimeError, match="ROCm"):   # everything passes: the first launch refuses the host model
            call(**kw)
    assert model.quality == q and model._gains is None and model._qualities is None


def test_one_rate_region_and_checkerboard_models():
    for arch in ("Compressor2018", "MeanScaleCompressor2018"):
        model = _cpu_model(arch)
        streams = [_stream(model)]
        with pytest.raises(ValueError, match="one rate"):
            model.transcode_each(streams, qualities=1.0)
        assert not hasattr(model, "transcode_each_to")
        assert model.transcode_each(streams, steps_per_chunk=16)[0] is streams[0]
        with pytest.raises(RuntimeError, match="ROCm"):
            model.transcode_each(streams, steps_per_chunk=8)
    region = _cpu_model("RegionGainedMeanScaleCompressor2018")
    streams = [_stream(region)]
    with pytest.raises(ValueError, match="quality map"):
        region.transcode_each(streams, qualities=1.0)
    with pytest.raises(ValueError, match="quality map"):
        region.transcode_each_to(streams, 10 ** 6)
    assert region.transcode_each(streams, steps_per_chunk=16)[0] is streams[0]
    with pytest.raises(RuntimeError, match="ROCm"):
        region.transcode_each(streams, steps_per_chunk=8)
    ckbd = _cpu_model("CheckerboardCompressor2018")
    assert ckbd.transcode_refusal and _cpu_model("MeanScaleCompressor2018").transcode_refusal is None
    for kw in (dict(steps_per_chunk=8), dict(qualities=1.0), {}):
        with pytest.raises(ValueError, match="CheckerboardCompressor2018 is not covered"):
            ckbd.transcode_each([b"anything"], **kw)


# ------------------------------------------------------------------ the op and the entry point
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_transcode_op_has_a_shape_kernel():
    from image_compression_amd import _lib
    ops = _lib.transcode_ops()
    registered = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("imgcomp_transcode::")}
    assert registered == {"requant_seg"}
    img = [0, 1, 1, 0, 1]
    for shape in ((2, 7, 192), (2, 3, 4, 5)):
        r = _meta(*shape)
        C = shape[-1]
        sym, kmax = ops.requant_seg(r, _meta(*shape), _meta(2, C), _meta(5, C), _meta(5, *shape[1:]), img)
        assert sym.device.type == "meta" and sym.dtype == torch.int32 and sym.shape == (5 * r[0].numel(),)
        assert list(kmax) == [0] * 5
    r = _meta(2, 7, 192)
    for bad in (dict(mu1=_meta(2, 6, 192)), dict(a=_meta(1, 192)), dict(a=_meta(2, 191)), dict(b=_meta(4, 192)),
                dict(mu2=_meta(4, 7, 192))):
        kw = {**dict(mu1=r, a=_meta(2, 192), b=_meta(5, 192), mu2=_meta(5, 7, 192)), **bad}
        with pytest.raises(RuntimeError):
            ops.requant_seg(r, kw["mu1"], kw["a"], kw["b"], kw["mu2"], img)


def test_library_exports_the_entry_point():
    from image_compression_amd import _lib
    L = _lib.load()
    assert "ic_requant_seg" in _lib.exported_symbols()
    assert L.ic_version() == 4


def test_entry_point_checks_its_arguments_on_the_host():
    """Every refusal below returns before anything is launched: the pointers are null or never dereferenced."""
    from image_compression_amd import _lib
    L = _lib.load()
    ERR = 1001
    p = 256   # a non-null address nothing reads: each call fails an earlier check

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    img = ints(0, 1, 1, 0, 1)

    def requant(r=p, mu1=p, N=2, P=48, C=192, a=p, b=p, mu2=p, nseg=5, im=img, dev=p, sym=p, kd=p, kh=ints(0, 0, 0, 0, 0)):
        return L.ic_requant_seg(r, mu1, N, P, C, a, b, mu2, nseg, im, dev, sym, kd, kh, None)

    for name in ("r", "mu1", "a", "b", "mu2", "im", "dev", "sym", "kd", "kh"):
        assert requant(**{name: None}) == ERR, name
    for bad in (dict(N=0), dict(N=-1), dict(N=65536), dict(P=0), dict(C=0), dict(C=-4), dict(nseg=0), dict(nseg=-2),
                dict(nseg=65536), dict(P=2 ** 62)):
        assert requant(**bad) == ERR, bad
    assert requant(im=ints(0, 1, 2, 0, 1)) == ERR             # img[m] outside [0, N)
    assert requant(im=ints(0, 1, 1, 0, -1)) == ERR


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    from image_compression_amd import functional as IF
    r, a, b, mu2 = torch.zeros(2, 4, 3, 3), torch.ones(2, 4), torch.ones(5, 4), torch.zeros(5, 4, 3, 3)
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.requant_seg(r, r, a, b, mu2, [0, 1, 1, 0, 1])
