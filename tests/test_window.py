"""Decoding a pixel window of a per-image stream, the host side (no GPU): the latent window of `codec.latent_window` /
`codec.window_plan` against transposed convs run in fp64 on the CPU, the chunk range against brute force, the byte
ranges against streams packed from synthetic lengths, the refusals in front of any launch, the op namespace's shape
kernels and the C entry points' descriptor checks."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ABI = 4
GEOMETRIES = [(5, (2, 2, 2, 2)), (3, (2, 2))]


def _header(h, w, C=192, R=1024, cls=None, **extra):
    from image_compression_amd import codec
    H, W = codec.padded_size(h, w)
    return (cls or codec.ImageHeader)(N=1, H=H, W=W, latent_channels=C, hyper_channels=5, kind=2, compute_dtype="fp32_split",
                                      abi=ABI, L=64, scale_min=0.11, scale_max=256.0, R=R, kmax_z=3, kmax_y=9, height=h,
                                      width=w, **extra)


# ------------------------------------------------------------------ the receptive field
@functools.lru_cache(maxsize=None)
def _synthesis(kernel, strides):
    """g_s's shape in fp64 on 2 channels: transposed convs (k x k, stride s, padding k // 2, output padding s - 1)
    with a bias each and a pointwise map between them, as GDN is pointwise in space."""
    g = torch.Generator().manual_seed(kernel + len(strides))
    weights = [(torch.randn(2, 2, kernel, kernel, generator=g, dtype=torch.float64),
                torch.randn(2, generator=g, dtype=torch.float64)) for _ in strides]

    def run(y):
        for i, ((w, b), s) in enumerate(zip(weights, strides)):
            y = F.conv_transpose2d(y, w, b, stride=s, padding=kernel // 2, output_padding=s - 1)
            if i < len(strides) - 1:
                y = y / torch.sqrt(1.0 + y * y)
        return y
    return run


def _walk(a, b, extent, kernel, strides):
    """The issue's walk, restated: the closed latent interval behind the output interval [a, b]."""
    D = int(np.prod(strides))
    for s in reversed(strides):
        D //= s
        a = -((-(a + kernel // 2 - (kernel - 1))) // s)      # ceil
        b = (b + kernel // 2) // s                            # floor
        a, b = max(a, 0), min(b, extent * D - 1)
    return a, b


def _boxes(h, w, rng, count=24):
    """1 x 1 boxes at the corners and inside, a box on each edge, the full image, and random ones."""
    boxes = [(0, 0, 1, 1), (h - 1, w - 1, 1, 1), (h // 2, w // 3, 1, 1), (0, 5, 7, 9), (3, 0, 11, 6), (h - 9, 4, 9, 13),
             (6, w - 17, 8, 17), (0, 0, h, w), (0, 0, h, 1), (h - 1, 0, 1, w)]
    while len(boxes) < count:
        top, left = int(rng.integers(0, h)), int(rng.integers(0, w))
        boxes.append((top, left, int(rng.integers(1, h - top + 1)), int(rng.integers(1, w - left + 1))))
    return boxes


@pytest.mark.parametrize("kernel,strides", GEOMETRIES, ids=["k5s2222", "k3s22"])
def test_latent_window_holds_what_the_box_depends_on(kernel, strides):
    """g_s on the plan's latent window, cropped at `crop`, is the crop of g_s on the whole latent, to 1e-12 in fp64;
    and the window is the walked interval snapped outward to 4, never more."""
    from image_compression_amd import codec
    D = int(np.prod(strides))
    Hy, Wy = 16, 24
    h, w = D * Hy - 56 * D // 16, D * Wy - 56 * D // 16        # (200, 328) of a 256 x 384 padded image at D = 16
    rng = np.random.default_rng(kernel)
    run = _synthesis(kernel, strides)
    y = torch.randn(1, 2, Hy, Wy, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    full = run(y)
    assert full.shape == (1, 2, D * Hy, D * Wy)
    header = _header(h, w) if D == codec.Y_DOWN else None
    for box in _boxes(h, w, rng):
        top, left, height, width = box
        r0, r1, c0, c1, crop = codec.latent_window(box, (Hy, Wy), kernel, strides)
        if header is not None:      # the plan of a stream with this latent is that window
            plan = codec.window_plan(header, box, kernel, strides)
            assert (plan.rows, plan.cols, plan.crop, plan.box) == ((r0, r1), (c0, c1), crop, box)
            assert plan.shape == (r1 - r0, c1 - c0) and plan.byte_ranges is None
        assert crop == (top - D * r0, left - D * c0)
        part = run(y[:, :, r0:r1, c0:c1])[:, :, crop[0]:crop[0] + height, crop[1]:crop[1] + width]
        want = full[:, :, top:top + height, left:left + width]
        assert part.shape == want.shape, box
        assert float((part - want).abs().max()) <= 1e-12, (box, (r0, r1, c0, c1))
        for (lo, hi), (a, n, extent) in zip(((r0, r1), (c0, c1)), ((top, height, Hy), (left, width, Wy))):
            wa, wb = _walk(a, a + n - 1, extent, kernel, strides)
            assert (lo, hi) == (wa // 4 * 4, min(-(-(wb + 1) // 4) * 4, extent)), (box, lo, hi, wa, wb)
            assert lo % 4 == 0 and (hi % 4 == 0 or hi == extent) and 0 <= lo < hi <= extent


def test_default_geometry_reaches_two_positions_beyond_the_box():
    from image_compression_amd import codec, get_cfg_defaults
    cfg = get_cfg_defaults()
    kernel, strides = int(cfg.MODEL.CONV_KERNEL), [int(s) for s in cfg.MODEL.STRIDES]
    assert (kernel, strides) == (5, [2, 2, 2, 2])
    worst = 0
    for a in range(64, 192):
        for n in (1, 2, 15, 16, 17, 33):
            lo, hi = codec._walk_back(a, a + n - 1, 64, kernel, strides)
            worst = max(worst, a // 16 - lo, hi - (a + n - 1) // 16)
    assert worst == 2


# ------------------------------------------------------------------ the chunk range
@pytest.mark.parametrize("R", [1, 5, 1024])
@pytest.mark.parametrize("h,w,C", [(200, 328, 3), (64, 130, 7), (640, 100, 191)])
def test_chunk_range_is_the_chunks_that_hold_the_rows(h, w, C, R):
    from image_compression_amd import codec
    header = _header(h, w, C=C, R=R)
    _, _, Hy, Wy = header.y_shape
    assert (Wy * C) % (64 * R), "rows must not end on chunk boundaries"
    chunk_of = np.arange(Hy * Wy * C) // (64 * R)
    rng = np.random.default_rng(R + C)
    for box in _boxes(h, w, rng, count=16):
        plan = codec.window_plan(header, box, 5, (2, 2, 2, 2))
        (r0, r1), (k0, k1) = plan.rows, plan.chunks
        assert plan.symbols == (r0 * Wy * C, r1 * Wy * C)
        held = np.unique(chunk_of[plan.symbols[0]:plan.symbols[1]])
        assert np.array_equal(held, np.arange(k0, k1)), (box, held, k0, k1)
        assert 0 <= k0 < k1 <= codec.num_chunks(header.nsym_y, R)


# ------------------------------------------------------------------ the byte ranges
def _lens(nsym, R, rng):
    from image_compression_amd import codec
    per = 64 * R
    words = [int(rng.integers(0, min(per, nsym - c * per) + 1)) for c in range(codec.num_chunks(nsym, R))]
    return np.asarray([codec.CHUNK_HEAD + 2 * v for v in words], dtype="<u4")


def _stream(container, h, w, R, rng, C=6):
    """(bytes, parser) of a stream of `container` packed from synthetic chunk lengths and random payload bytes."""
    from image_compression_amd import codec
    if container == "ICRP":
        header, pack, parse = _header(h, w, C=C, R=R), codec.pack_image, codec.parse_image
    elif container == "ICRQ":
        header = _header(h, w, C=C, R=R, cls=codec.GainedImageHeader, levels=6, quality=2.5)
        pack, parse = codec.pack_gained_image, codec.parse_gained_image
    else:
        H, W = codec.padded_size(h, w)
        codes = rng.integers(0, 256, (H // 64, W // 64), dtype=np.uint8)
        header = _header(h, w, C=C, R=R, cls=codec.RegionImageHeader, levels=6, map_h=H // 64, map_w=W // 64, codes=codes)
        pack, parse = codec.pack_region_image, codec.parse_region_image
    lz, ly = _lens(header.nsym_z, R, rng), _lens(header.nsym_y, R, rng)
    pz, py = (rng.integers(0, 256, int(l.sum()), dtype=np.uint8).tobytes() for l in (lz, ly))
    return pack(header, lz, ly, pz, py), parse


@pytest.mark.parametrize("container", ["ICRP", "ICRQ", "ICRR"])
@pytest.mark.parametrize("R", [1, 5, 1024])
def test_byte_ranges_cover_exactly_what_a_window_decode_reads(container, R):
    from image_compression_amd import codec
    rng = np.random.default_rng(R)
    h, w = 200, 328
    data, parse = _stream(container, h, w, R, rng)
    header, lz, ly, pz, py = parse(data, ABI, "fp32_split")
    y_at = len(data) - len(py)
    assert data[y_at - len(pz):y_at] == pz
    ends = np.concatenate(([0], np.cumsum(ly.astype(np.int64))))
    spanned = set()
    for box in _boxes(h, w, rng, count=16):
        plan = codec.window_plan(header, box, 5, (2, 2, 2, 2), lengths=(lz, ly))
        ranges = plan.byte_ranges
        assert all(0 <= a < b <= len(data) for a, b in ranges), ranges
        assert all(b <= a2 for (_, b), (a2, _) in zip(ranges, ranges[1:])), ranges      # ascending and disjoint
        got = np.zeros(len(data), dtype=bool)
        for a, b in ranges:
            got[a:b] = True
        want = np.zeros(len(data), dtype=bool)
        want[:y_at] = True                         # the header, both length tables and all of z's payload
        k0, k1 = plan.chunks
        want[y_at + ends[k0]:y_at + ends[k1]] = True
        assert np.array_equal(got, want), box
        spanned.add((k0, k1))
    if R < 1024:
        assert len(spanned) > 2, "the boxes span different chunk ranges"
    with pytest.raises(ValueError, match="length tables"):
        codec.window_plan(header, (0, 0, 1, 1), 5, (2, 2, 2, 2), lengths=(lz, np.concatenate([ly, ly])))


# ------------------------------------------------------------------ the refusals
BAD_BOXES = [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (-1, 0, 5, 5), (0, -1, 5, 5), (196, 0, 5, 5), (0, 324, 5, 5),
             (200, 0, 1, 1), (0, 328, 1, 1), (0, 0, 201, 1), (0, 0, 1, 329)]


def test_every_box_refusal_is_raised_in_front_of_everything_else():
    from image_compression_amd import codec
    header = _header(200, 328)
    for box in BAD_BOXES:
        with pytest.raises(ValueError, match="empty or leaves"):
            codec.window_plan(header, box, 5, (2, 2, 2, 2))
        with pytest.raises(ValueError, match="empty or leaves"):      # before the geometry and the lengths are looked at
            codec.window_plan(header, box, 5, (2, 2), lengths=(None, None))
    for bad in (None, (0, 0, 1), "abcd", (0, 0, 1, None)):
        with pytest.raises(ValueError, match="box"):
            codec.window_plan(header, bad, 5, (2, 2, 2, 2))
    # the last pixel reaches latent rows 11 .. 14: two blocks, the second the one that holds the padding
    assert codec.window_plan(header, (199, 327, 1, 1), 5, (2, 2, 2, 2)).rows == (8, 16)
    with pytest.raises(ValueError, match="strides"):
        codec.window_plan(header, (0, 0, 1, 1), 5, (2, 2, 2))
    plain = codec.Header(**{k: v for k, v in vars(header).items() if k not in ("height", "width")})
    with pytest.raises(ValueError, match="per-image"):
        codec.window_plan(plain, (0, 0, 1, 1), 5, (2, 2, 2, 2))
    for bad in ((0, 0, 0, 1), (0, 0, 1, 65), (60, 0, 5, 1)):
        with pytest.raises(ValueError, match="empty or leaves"):
            codec.latent_window(bad, (4, 4), 5, (2, 2, 2, 2))


@functools.lru_cache(maxsize=None)
def _cpu_model(arch):
    from image_compression_amd import get_cfg_defaults, modelling
    cfg = get_cfg_defaults()
    cfg.MODEL.META_ARCHITECTURE = arch
    cfg.MODEL.LOSS.REDUCTION = "mean"
    torch.manual_seed(0)
    return modelling.build_model(cfg).eval()


def test_checkerboard_models_refuse_with_a_reason():
    from image_compression_amd.modelling.meta_arch.bmshl2018 import Compressor2018
    assert Compressor2018.window_refusal is None
    model = _cpu_model("CheckerboardCompressor2018")
    assert "halves" in model.window_refusal
    with pytest.raises(ValueError, match="decompress_window: CheckerboardCompressor2018 is not covered"):
        model.decompress_window([b""], [(0, 0, 1, 1)])
    model.train()
    try:
        with pytest.raises(ValueError, match="not covered"):      # the refusal is in front of the eval-mode check too
            model.decompress_window([b""], [(0, 0, 1, 1)])
    finally:
        model.eval()


def test_model_refusals_come_before_any_launch():
    """A host model: any launch would raise RuntimeError naming the device.  Every stream is parsed and every box
    planned first, so a bad second box is refused although the first is fine."""
    from image_compression_amd import codec
    model = _cpu_model("Compressor2018")
    cm, rng = model.conditional_model, np.random.default_rng(0)
    header = codec.ImageHeader(N=1, H=64, W=128, latent_channels=192, hyper_channels=192, kind=cm.KIND,
                               compute_dtype=model._build_id()[1], abi=model._build_id()[0], L=cm.num_scales,
                               scale_min=cm.scale_min, scale_max=cm.scale_max, R=16, kmax_z=1, kmax_y=2, height=40, width=100)
    lz, ly = _lens(header.nsym_z, 16, rng), _lens(header.nsym_y, 16, rng)
    data = codec.pack_image(header, lz, ly, bytes(int(lz.sum())), bytes(int(ly.sum())))
    with pytest.raises(ValueError, match="1 streams for 2 boxes"):
        model.decompress_window([data], [(0, 0, 1, 1), (0, 0, 1, 1)])
    with pytest.raises(ValueError, match="box 1.*empty or leaves"):
        model.decompress_window([data, data], [(0, 0, 1, 1), (0, 0, 41, 1)])
    with pytest.raises(ValueError, match="magic"):
        model.decompress_window([data, b"ICRQ" + data[4:]], [(0, 0, 1, 1), (0, 0, 1, 1)])
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.decompress_window([data], [(0, 0, 1, 1)])
    model.eval()
    with pytest.raises(RuntimeError, match="ROCm"):      # everything passes: the first launch refuses the host tensors
        model.decompress_window([data], [(0, 0, 1, 1)])


# ------------------------------------------------------------------ the ops and the C entry points
def test_window_ops_have_shape_kernels():
    from image_compression_amd import _lib
    ops = _lib.window_ops()
    registered = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("imgcomp_window::")}
    assert registered == {"imgcomp_window::decode", "imgcomp_window::crop_clamp_at"}
    packed = torch.empty(4096, dtype=torch.uint8, device="meta")
    pool = torch.empty(64 * 8, dtype=torch.int32, device="meta")
    rows = torch.empty(2 * 8 * 11 * 3, dtype=torch.uint8, device="meta")
    mu = torch.empty(2 * 8 * 11 * 3, device="meta")
    windows = [0, 0, 8, 11, 3, 4, 7, 2, 5, 264, 0, 8, 11, 3, 0, 0, 0, 3]
    out = ops.decode(packed, windows, 4, 4, list(range(12)), rows, mu, 3, pool, 64, 1)
    assert out.device.type == "meta" and out.shape == (2, 4, 4, 3) and out.dtype == torch.float32
    assert ops.decode(packed, windows[:9], 4, 4, [0, 1], None, None, 3, pool, 64, 1).shape == (1, 4, 4, 3)
    for bad in (windows[:8], []):
        with pytest.raises(RuntimeError, match="windows"):
            ops.decode(packed, bad, 4, 4, [0, 1], rows, mu, 3, pool, 64, 1)
    with pytest.raises(RuntimeError, match="spans"):
        ops.decode(packed, windows, 4, 4, [0, 1, 2], rows, mu, 3, pool, 64, 1)
    x = torch.empty(2, 3, 64, 96, device="meta")
    y = ops.crop_clamp_at(x, 5, 7, 11, 67)
    assert y.device.type == "meta" and y.shape == (2, 3, 11, 67)
    for top, left, hh, ww in ((-1, 0, 1, 1), (0, 0, 0, 1), (60, 0, 5, 1), (0, 90, 1, 7)):
        with pytest.raises(RuntimeError, match="rectangle"):
            ops.crop_clamp_at(x, top, left, hh, ww)


def test_entry_points_refuse_bad_descriptors_before_touching_a_device():
    """Host buffers of the sizes the arguments name: every call is refused, so none of them is read by a device
    (tools/window_hostcheck.cpp runs the full list under the sanitizers)."""
    from image_compression_amd import _lib
    L = _lib.load()
    C, seg = 3, 8 * 11 * 3
    buf = np.zeros(1024, dtype=np.uint16)
    rows, mu = np.zeros(2 * seg, dtype=np.uint8), np.zeros(2 * seg, dtype=np.float32)
    pool, ws, out = np.zeros(4 * 6, dtype=np.uint32), np.zeros(64, dtype=np.int64), np.full(2 * 4 * 4 * C, -1.0, np.float32)
    spans = (ctypes.c_longlong * 12)(*[v for b in range(6) for v in (128 * b, 128 * b + 128)])

    def call(edit=None, nblocks=6, in_bytes=2048, ws_bytes=512):
        win = (_lib.ICWindow * 2)(_lib.ICWindow(0, 0, 8, 11, 2, 4, 7, 2, 5), _lib.ICWindow(seg, 0, 8, 11, 2, 0, 0, 0, 3))
        if edit:
            edit(win)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        return L.ic_codec_decode_window(p(buf), in_bytes, win, 2, 4, 4, spans, nblocks, p(rows), p(mu), 2 * seg, C, p(pool),
                                        pool.size, 4, 1, p(ws), ws_bytes, p(out), None)

    def field(k, name, value):
        return lambda win: setattr(win[k], name, value)

    edits = [field(0, "r0", 5), field(0, "c0", 8), field(1, "base", seg + 1), field(0, "K", 3), field(1, "table", 1),
             field(0, "k1", 6), field(0, "k0", 3), field(1, "k1", 2), field(0, "hy", 0), field(1, "wy", -11)]
    for e in edits:
        assert call(e) == 1001
    assert call(nblocks=5) == 1001 and call(nblocks=7) == 1001 and call(in_bytes=1534) == 1001
    assert call(ws_bytes=L.ic_codec_window_ws(2, 6) - 1) == 1002
    assert 0 < L.ic_codec_window_ws(2, 6) <= 512 and L.ic_codec_window_ws(0, 6) == 0 and L.ic_codec_window_ws(2, 0) == 0
    assert bool((out == -1.0).all())
    x = np.zeros(2 * 3 * 8 * 8, dtype=np.float32)
    a = _lib.ICAct(x.ctypes.data, 2, 3, 8, 8, 192, 64, 8, 1)
    for top, left, hh, ww in ((-1, 0, 4, 4), (5, 0, 4, 4), (0, 5, 4, 4), (0, 0, 0, 4), (0, 0, 4, 9)):
        assert L.ic_crop_clamp_at(ctypes.byref(a), top, left, hh, ww, ctypes.c_void_p(out.ctypes.data), None) == 1001
