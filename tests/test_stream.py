"""Per-image streams on the CPU: the "ICRP" container's pack_image / parse_image with its validation,
the registration of the segmented coder's ops and symbols, their host-side queries and argument checks,
and the model's refusals.  No GPU: the kernels are held to the numpy coder in tests/test_stream_gpu.py."""
import ctypes
import dataclasses
import struct

import numpy as np
import pytest
import torch

from test_codec import draw, random_tables, ref_encode


def _image(R=4, height=72, width=100):
    from image_compression_amd import codec
    H, W = codec.padded_size(height, width)
    h = codec.ImageHeader(N=1, H=H, W=W, latent_channels=6, hyper_channels=5, kind=1, compute_dtype="fp32_split", abi=4,
                          L=64, scale_min=0.11, scale_max=256.0, R=R, kmax_z=3, kmax_y=40, height=height, width=width)
    rng = np.random.default_rng(0)
    out = []
    for nsym, K in ((h.nsym_z, h.kmax_z), (h.nsym_y, h.kmax_y)):
        cdf = random_tables(rng, 5, K)
        rows = np.arange(nsym) % 5
        payload, lens = ref_encode(draw(rng, cdf, rows), rows, cdf, R)
        out.append((lens, payload))
    return codec, h, out[0], out[1]


OK = dict(abi=4, compute_dtype="fp32_split")


def test_padded_size_rounds_up_to_64():
    from image_compression_amd import codec
    assert [codec.padded_size(*s) for s in ((1, 1), (64, 65), (72, 100), (500, 750), (512, 768))] == \
        [(64, 64), (64, 128), (128, 128), (512, 768), (512, 768)]


def test_image_container_round_trips():
    codec, h, (lz, pz), (ly, py) = _image()
    assert (h.H, h.W) == (128, 128) and (h.z_shape, h.y_shape) == ((1, 5, 2, 2), (1, 6, 8, 8))
    data = codec.pack_image(h, lz, ly, pz, py)
    assert isinstance(data, bytes) and data[:4] == b"ICRP"
    h2, lz2, ly2, pz2, py2 = codec.parse_image(data, **OK)
    assert h2 == h and np.array_equal(lz2, lz) and np.array_equal(ly2, ly) and pz2 == pz and py2 == py
    # the ICRA header's fields at the ICRA header's offsets, then height and width
    assert codec._IMAGE_HEAD.size == codec._HEAD.size + 8
    assert struct.unpack_from("<II", data, codec._HEAD.size) == (72, 100)
    assert codec.image_fixed_bytes(h) == len(data) - (len(pz) + len(py)) + 256 * (len(lz) + len(ly))
    # the two containers do not read each other
    with pytest.raises(ValueError, match="magic"):
        codec.parse(data, **OK)
    batch = codec.pack(codec.Header(*dataclasses.astuple(h)[:14]), lz, ly, pz, py)
    with pytest.raises(ValueError, match="magic"):
        codec.parse_image(batch, **OK)
    with pytest.raises(ValueError, match="magic"):
        codec.parse_image(batch + b"\0" * 8, **OK)


def test_parse_image_rejects_inconsistent_buffers():
    codec, h, (lz, pz), (ly, py) = _image()
    data = codec.pack_image(h, lz, ly, pz, py)
    head = codec._IMAGE_HEAD.size
    for cut in (0, 3, 40, codec._HEAD.size, head - 1, head + 2, len(data) - len(py) - len(pz) - 2, len(data) - 1):
        with pytest.raises(ValueError):
            codec.parse_image(data[:cut], **OK)                                     # truncated anywhere
    with pytest.raises(ValueError):
        codec.parse_image(data + b"\0\0", **OK)                                     # trailing bytes
    with pytest.raises(ValueError, match="format version"):
        codec.parse_image(data[:4] + struct.pack("<H", 2) + data[6:], **OK)
    with pytest.raises(ValueError, match="ABI"):
        codec.parse_image(data, abi=5, compute_dtype="fp32_split")
    with pytest.raises(ValueError, match="COMPUTE_DTYPE"):
        codec.parse_image(data, abi=4, compute_dtype="fp32")

    def with_size(height, width):
        raw = bytearray(data)
        raw[codec._HEAD.size:head] = struct.pack("<II", height, width)
        return bytes(raw)

    assert codec.parse_image(with_size(65, 128), **OK)[0].height == 65             # the ends of the valid range
    for height, width in ((129, 100), (72, 129), (64, 100), (72, 64), (0, 100), (72, 0)):
        with pytest.raises(ValueError, match="pad"):
            codec.parse_image(with_size(height, width), **OK)
        with pytest.raises(ValueError, match="pad"):
            codec.pack_image(dataclasses.replace(h, height=height, width=width), lz, ly, pz, py)
    # N != 1: at pack, and in a buffer (N is the first u32 after the ABI version, offset 12)
    with pytest.raises(ValueError, match="one image"):
        codec.pack_image(dataclasses.replace(h, N=2), lz, ly, pz, py)
    raw = bytearray(data)
    assert raw[12:16] == struct.pack("<I", 1)
    raw[12:16] = struct.pack("<I", 2)
    with pytest.raises(ValueError, match="one image"):
        codec.parse_image(bytes(raw), **OK)
    # the checks shared with parse: a chunk length that disagrees with the buffer, with and without the buffer grown
    bad = bytearray(data)
    bad[head:head + 4] = struct.pack("<I", int(lz[0]) + 2)
    with pytest.raises(ValueError):
        codec.parse_image(bytes(bad), **OK)
    worst = 256 + 2 * min(64 * h.R, h.nsym_z)
    bad[head:head + 4] = struct.pack("<I", worst + 2)
    with pytest.raises(ValueError):
        codec.parse_image(bytes(bad) + b"\0" * (worst + 2 - int(lz[0])), **OK)
    for field, at in (("kmax_z", 56), ("kmax_y", 60)):
        with pytest.raises(ValueError, match="2047"):
            codec.pack_image(dataclasses.replace(h, **{field: 2048}), lz, ly, pz, py)
        raw = bytearray(data)
        raw[at:at + 4] = struct.pack("<I", 2048)
        with pytest.raises(ValueError, match="2047"):
            codec.parse_image(bytes(raw), **OK)
    with pytest.raises(ValueError):
        codec.pack_image(dataclasses.replace(h, H=192, height=136), lz, ly, pz, py)  # counts do not follow the shape
    with pytest.raises(ValueError, match="multiple"):
        codec.pack_image(dataclasses.replace(h, W=96, width=90), lz, ly, pz, py)


def test_split_and_join_of_the_segmented_buffer():
    from image_compression_amd import codec
    rng = np.random.default_rng(3)
    cdf = random_tables(rng, 5, 9)
    seg_len, R, nseg = 64 * 4 + 1, 4, 3
    parts = []
    for _ in range(nseg):
        rows = np.arange(seg_len) % 5
        payload, lens = ref_encode(draw(rng, cdf, rows), rows, cdf, R)
        parts.append((lens, payload))
    buf = codec.join_packed_seg(parts)
    assert buf.dtype == np.uint8 and buf.size == 4 * 6 + sum(len(p) for _, p in parts)
    back = codec.split_packed_seg(np.concatenate([buf, np.zeros(100, np.uint8)]), nseg, seg_len, R)
    for (l0, p0), (l1, p1) in zip(parts, back):
        assert np.array_equal(l0, l1) and p0 == p1
    with pytest.raises(RuntimeError):
        codec.split_packed_seg(buf[:-2], nseg, seg_len, R)


# ------------------------------------------------------------------ registration
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_every_stream_op_has_a_meta_kernel():
    from image_compression_amd import _lib
    ops = _lib.stream_ops()
    seg_len, R, nseg = 64 * 4 + 1, 4, 3
    pool = _meta(5 * (2 * 37 + 2), dtype=torch.int32)
    ks, offs = [37] * nseg, [0] * nseg
    chunks = 6
    cases = {
        "symbolize_seg": (lambda: ops.symbolize_seg(_meta(3, 4, 4, 6), 3)[0], (288,), torch.int32),
        "encode_seg": (lambda: ops.encode_seg(_meta(nseg * seg_len, dtype=torch.int32), nseg, None, 5, pool, 5, ks, offs, R),
                       (chunks * 4 + chunks * (2 * 64 * R + 256),), torch.uint8),
        "decode_seg": (lambda: ops.decode_seg(_meta(1000, dtype=torch.uint8), nseg, seg_len,
                                              _meta(nseg * seg_len, dtype=torch.uint8), 0, pool, 5, ks, offs, R),
                       (nseg * seg_len,), torch.float32),
        "pad_edge": (lambda: ops.pad_edge(_meta(2, 3, 72, 100), 128, 128), (2, 3, 128, 128), torch.float32),
        "crop_clamp": (lambda: ops.crop_clamp(_meta(2, 3, 128, 128), 72, 100), (2, 3, 72, 100), torch.float32),
    }
    registered = {nm.split("::")[1] for nm in torch._C._dispatch_get_all_op_names() if nm.startswith("imgcomp_stream::")}
    assert registered == set(cases), sorted(registered ^ set(cases))
    for name, (call, shape, dtype) in cases.items():
        out = call()
        assert out.device.type == "meta" and tuple(out.shape) == shape and out.dtype == dtype, name
        assert out.is_contiguous(), name
    assert list(ops.symbolize_seg(_meta(6), 3)[1]) == [0, 0, 0]


def test_library_carries_the_segmented_symbols():
    from image_compression_amd import _lib
    names = {"ic_codec_seg_chunks", "ic_codec_encode_seg_ws", "ic_codec_compact_seg_bytes", "ic_codec_symbolize_seg",
             "ic_codec_encode_seg", "ic_codec_compact_seg", "ic_codec_decode_seg", "ic_pad_edge", "ic_crop_clamp"}
    assert names <= set(_lib.SIGNATURES) and names <= _lib.exported_symbols()
    L = _lib.load()
    assert L.ic_version() == 4                      # purely additive
    # nseg * ceil(seg_len / (64 R)) chunks: a chunk never straddles a segment
    assert L.ic_codec_seg_chunks(3, 64 * 4 + 1, 4) == 6 and L.ic_codec_seg_chunks(1, 64 * 4 + 1, 4) == 2
    assert L.ic_codec_seg_chunks(8, 1, 1024) == 8 and L.ic_codec_seg_chunks(2, 2 * 64 * 4, 4) == 4
    assert L.ic_codec_encode_seg_ws(3, 64 * 4 + 1, 4) == 6 * (2 * 64 * 4 + 256)
    assert L.ic_codec_compact_seg_bytes(3, 64 * 4 + 1, 4) == 6 * 4 + 6 * (2 * 64 * 4 + 256)
    for bad in ((0, 10, 4), (3, 0, 4), (3, 10, 0), (3, 10, 65537), (2, 2 ** 62, 4)):
        assert L.ic_codec_seg_chunks(*bad) == 0 and L.ic_codec_encode_seg_ws(*bad) == 0
        assert L.ic_codec_compact_seg_bytes(*bad) == 0


def test_segmented_argument_checks_come_before_any_launch():
    """Every call below must return 1001 from the host checks: the pointers are not device memory."""
    from image_compression_amd import _lib
    L = _lib.load()
    fake = ctypes.c_void_p(4096)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    lls = lambda *v: (ctypes.c_longlong * len(v))(*v)
    M1 = 2 * 3 + 2

    def enc(nseg=2, seg_len=10, rows=fake, C=0, pool_words=5 * M1, nrows=5, ks=(3, 3), offs=(0, 0), R=4, sym=fake):
        return L.ic_codec_encode_seg(sym, nseg, seg_len, rows, C, fake, pool_words, nrows, ints(*ks), lls(*offs), fake, R,
                                     fake, 1 << 30, fake, None)

    def dec(nseg=2, seg_len=10, rows=fake, C=0, pool_words=5 * M1, nrows=5, ks=(3, 3), offs=(0, 0), R=4, in_bytes=1 << 20):
        return L.ic_codec_decode_seg(fake, in_bytes, nseg, seg_len, rows, C, fake, pool_words, nrows, ints(*ks),
                                     lls(*offs), fake, R, fake, None)

    for f in (enc, dec):
        assert f(nseg=0) == 1001 and f(seg_len=0) == 1001 and f(R=0) == 1001 and f(R=65537) == 1001
        assert f(nrows=0) == 1001
        assert f(ks=(3, 2048)) == 1001 and f(ks=(-1, 3)) == 1001           # K outside [0, 2047]
        assert f(offs=(0, 1)) == 1001 and f(offs=(0, -8)) == 1001          # a table that leaves the pool
        assert f(pool_words=5 * M1 - 1) == 1001
        assert f(rows=None, C=0) == 1001 and f(rows=None, C=6) == 1001     # channel rows: 1 <= C <= nrows ...
        assert f(rows=None, C=3) == 1001                                   # ... and segment starts multiples of C
    assert enc(sym=None) == 1001
    assert dec(in_bytes=7) == 1001                                         # the length tables must be inside the buffer
    assert L.ic_codec_symbolize_seg(None, 2, 10, fake, fake, ints(0, 0), None) == 1001
    assert L.ic_codec_symbolize_seg(fake, 0, 10, fake, fake, ints(0, 0), None) == 1001
    assert L.ic_codec_symbolize_seg(fake, 65536, 10, fake, fake, ints(0, 0), None) == 1001
    assert L.ic_codec_compact_seg(fake, fake, 0, 4, fake, 1 << 30, None) == 1001
    assert L.ic_codec_compact_seg(fake, fake, 6, 4, fake, 6 * 4 + 6 * (2 * 64 * 4 + 256) - 1, None) == 1002
    assert L.ic_pad_edge(fake, 1, 3, 72, 100, 64, 128, fake, None) == 1001  # padded size below the image's
    assert L.ic_pad_edge(fake, 1, 3, 0, 100, 64, 128, fake, None) == 1001
    a = _lib.ICAct(fake, 1, 3, 64, 128, 3 * 64 * 128, 64 * 128, 128, 1)
    assert L.ic_crop_clamp(a, 65, 100, fake, None) == 1001 and L.ic_crop_clamp(a, 0, 100, fake, None) == 1001
    assert L.ic_crop_clamp(a, 64, 100, None, None) == 1001


def test_model_refuses_per_image_coding_outside_eval_or_bin_one():
    from image_compression_amd import get_cfg_defaults, modelling
    cfg = get_cfg_defaults()
    model = modelling.build_model(cfg)
    with pytest.raises(RuntimeError, match="eval"):
        model.compress_each(torch.rand(1, 3, 50, 70))
    with pytest.raises(RuntimeError, match="eval"):
        model.decompress_each([b""])
    model.eval()
    with pytest.raises(ValueError):
        model.compress_each(torch.rand(3, 50, 70))
    with pytest.raises(ValueError):
        model.compress_each(torch.rand(1, 3, 0, 70))
    with pytest.raises(ValueError):
        model.decompress_each([b"ICRP"])
    assert model.decompress_each([]) == []
    cfg.MODEL.ENTROPY_MODEL.BIN = 2.0
    m2 = modelling.build_model(cfg).eval()
    with pytest.raises(NotImplementedError, match="BIN"):
        m2.compress_each(torch.rand(1, 3, 50, 70))
    with pytest.raises(NotImplementedError, match="BIN"):
        m2.decompress_each([b""])
