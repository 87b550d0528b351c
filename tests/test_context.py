"""The fused checkerboard context on the CPU: the per-image container "ICRK", the two format versions of "ICRC", the
MODEL.CONTEXT.KERNEL switch on CheckerboardCompressor2018 (state dict, refusals, parse errors without a device), and
the registration of torch.ops.imgcomp_ctx and of the library's symbols with their host-side argument checks.  No GPU:
the kernel and the model's streams are held to numpy and to the model's own pieces in tests/test_context_gpu.py."""
import dataclasses
import os
import re
import struct

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_checkerboard import _cfg, _ckbd_container, _packed
from test_gained import ABI, _five, _lens

OK = dict(abi=4, compute_dtype="fp32_split")
HEAD = "<4sHBBIIIIIIIddIIIQQ" + "III" + "II"   # the ICRC header, then image height and width
KIND_AT = 7
ARCH = "CheckerboardCompressor2018"


# ------------------------------------------------------------------ "ICRK"
def _image_stream(rng, **over):
    """(ImageHeader, pack arguments) of a random valid per-image checkerboard stream."""
    from image_compression_amd import codec
    H, W = (int(64 * rng.integers(1, 4)) for _ in range(2))
    fields = dict(N=1, H=H, W=W, latent_channels=int(rng.integers(1, 9)), hyper_channels=int(rng.integers(1, 9)),
                  kind=int(rng.integers(2, 4)), compute_dtype=codec.COMPUTE_DTYPES[int(rng.integers(0, 3))], abi=ABI,
                  L=int(rng.integers(1, 65)), scale_min=0.11, scale_max=256.0, R=int(rng.integers(1, 40)),
                  kmax_z=int(rng.integers(0, 2048)), kmax_y=int(rng.integers(0, 2048)),
                  height=H - int(rng.integers(0, 64)), width=W - int(rng.integers(0, 64)))
    fields.update(over)
    h = codec.ImageHeader(**fields)
    lens = [_lens(n, h.R, rng) for n in (h.nsym_z, *codec._half_symbols(h))]
    pays = [rng.integers(0, 256, int(l.sum()), dtype=np.uint8).tobytes() for l in lens]
    return h, (*lens, *pays)


def test_icrk_round_trips_over_random_headers():
    from image_compression_amd import codec
    rng = np.random.default_rng(21)
    assert codec._CKBD_IMAGE_HEAD.size == struct.calcsize(HEAD) == codec._CKBD_HEAD.size + 8
    for _ in range(50):
        h, args = _image_stream(rng)
        data = codec.pack_checkerboard_image(h, *args)
        assert isinstance(data, bytes) and data[:4] == b"ICRK" and struct.unpack_from("<H", data, 4)[0] == 1
        assert struct.unpack_from("<II", data, struct.calcsize(HEAD) - 8) == (h.height, h.width)
        g, *rest = codec.parse_checkerboard_image(data, ABI, h.compute_dtype)
        assert g == h and type(g) is codec.ImageHeader
        for got, want in zip(rest, args):
            assert np.array_equal(got, want) if isinstance(want, np.ndarray) else got == want
        lz, la, ln = args[:3]
        # each half is chunked from its own first symbol, and holds half of y
        assert len(la) == len(ln) == codec.num_chunks(h.nsym_y // 2, h.R) and len(lz) == codec.num_chunks(h.nsym_z, h.R)
        nc = len(lz) + len(la) + len(ln)
        assert codec.checkerboard_image_fixed_bytes(h) == struct.calcsize(HEAD) + 4 * nc + 256 * nc
        words = sum(int(l.sum()) for l in (lz, la, ln)) - 256 * nc
        assert len(data) == codec.checkerboard_image_fixed_bytes(h) + words


def _offset(name):
    names = ["magic", "ver", "dt", "kind", "abi", "N", "H", "W", "cy", "cz", "L", "smin", "smax", "R", "kz", "ky", "nz", "ny",
             "ncz", "nca", "ncn", "height", "width"]
    fields, off, out = ["4s"] + list(HEAD[3:]), 0, {}
    assert len(fields) == len(names)
    for nm, f in zip(names, fields):
        out[nm] = off
        off += struct.calcsize("<" + f)
    assert off == struct.calcsize(HEAD)
    return out[name]


def test_icrk_parse_and_pack_refuse_what_is_inconsistent():
    from image_compression_amd import codec
    rng = np.random.default_rng(22)
    h, args = _image_stream(rng, compute_dtype="fp32_split", H=128, W=192, height=100, width=130, R=2, latent_channels=6)
    data = codec.pack_checkerboard_image(h, *args)
    parse = lambda d: codec.parse_checkerboard_image(d, **OK)     # noqa: E731
    assert parse(data)[0] == h and _offset("kind") == KIND_AT
    # truncation anywhere, and a byte too many
    for cut in (0, 3, 50, _offset("ncn"), _offset("height"), _offset("width") + 3, struct.calcsize(HEAD) + 5, len(data) - 1):
        with pytest.raises(ValueError):
            parse(data[:cut])
    with pytest.raises(ValueError):
        parse(data + b"\0")

    def patched(name, fmt, value):
        raw = bytearray(data)
        struct.pack_into("<" + fmt, raw, _offset(name), value)
        return bytes(raw)

    # wrong chunk counts, in each of the three places (the count of the whole of y among them)
    for name, n in (("ncz", 2), ("nca", len(args[1]) + 1), ("ncn", 0), ("nca", codec.num_chunks(h.nsym_y, h.R))):
        assert n != {"ncz": len(args[0]), "nca": len(args[1]), "ncn": len(args[2])}[name]
        with pytest.raises(ValueError, match="chunk counts"):
            parse(patched(name, "I", n))
    for ny in (h.nsym_y - 1, h.nsym_y + 2, h.nsym_y // 2):
        with pytest.raises(ValueError, match="symbol counts"):
            parse(patched("ny", "Q", ny))
    # kinds without a mean
    for kind in (0, 1, 4):
        with pytest.raises(ValueError, match="conditional kind"):
            parse(patched("kind", "B", kind))
        with pytest.raises(ValueError, match="conditional kind"):
            codec.pack_checkerboard_image(dataclasses.replace(h, kind=kind), *args)
    # one image, whose size pads to H x W
    with pytest.raises(ValueError, match="one image"):
        parse(patched("N", "I", 2))
    for name, v in (("height", 0), ("height", 129), ("height", 64), ("width", 0), ("width", 193), ("width", 128)):
        with pytest.raises(ValueError, match="does not pad"):
            parse(patched(name, "I", v))
        with pytest.raises(ValueError, match="does not pad"):
            codec.pack_checkerboard_image(dataclasses.replace(h, **{name: v}), *args)
    with pytest.raises(ValueError, match="format version"):
        parse(patched("ver", "H", 2))
    with pytest.raises(ValueError, match="ABI"):
        codec.parse_checkerboard_image(data, abi=5, compute_dtype="fp32_split")
    with pytest.raises(ValueError, match="COMPUTE_DTYPE"):
        codec.parse_checkerboard_image(data, abi=4, compute_dtype="fp32")
    # lengths that do not add up: a table entry moved by two bytes, and a payload that is not its lengths' sum
    raw = bytearray(data)
    first = struct.calcsize(HEAD)
    struct.pack_into("<I", raw, first, struct.unpack_from("<I", raw, first)[0] + 2)
    with pytest.raises(ValueError):
        parse(bytes(raw))
    lz, la, ln, pz, pa, pn = args
    with pytest.raises(ValueError, match="add up"):
        codec.pack_checkerboard_image(h, lz, la, ln, pz, pa, pn + b"\0\0")
    with pytest.raises(ValueError, match="chunk"):
        codec.pack_checkerboard_image(h, lz, np.concatenate([la, la]), ln, pz, pa + pa, pn)


def test_all_six_containers_refuse_one_anothers_magic():
    from image_compression_amd import codec
    six = dict(_five())
    h, args = _image_stream(np.random.default_rng(23))
    six["ICRK"] = (codec.parse_checkerboard_image, codec.pack_checkerboard_image(h, *args), h.compute_dtype)
    assert sorted(six) == ["ICRA", "ICRC", "ICRG", "ICRK", "ICRP", "ICRQ"]
    for name, (parse, data, dt) in six.items():
        assert data[:4] == name.encode() and parse(data, ABI, dt)[0] is not None
        for other, (_, theirs, odt) in six.items():
            if other != name:
                with pytest.raises(ValueError, match="magic"):
                    parse(theirs, ABI, odt)
                with pytest.raises(ValueError, match="magic"):       # and its own body under another's magic
                    parse(other.encode() + data[4:], ABI, dt)


# ------------------------------------------------------------------ "ICRC" versions
def test_icrc_versions_refuse_each_other_by_the_version_message():
    codec, h, streams = _ckbd_container()
    (lz, pz), (la, pa), (ln, pn) = streams
    v1 = _packed(codec, h, streams)
    assert v1 == codec.pack_checkerboard(h, lz, la, ln, pz, pa, pn, version=1)     # 1 is the default, as before
    v2 = codec.pack_checkerboard(h, lz, la, ln, pz, pa, pn, version=2)
    assert (codec.CKBD_FORMAT_VERSION, codec.CKBD_FUSED_FORMAT_VERSION) == (1, 2)
    assert [struct.unpack_from("<H", d, 4)[0] for d in (v1, v2)] == [1, 2]
    assert v1[:4] == v2[:4] == b"ICRC" and v1[6:] == v2[6:], "the two versions share one layout"
    assert codec.parse_checkerboard(v1, **OK)[0] == codec.parse_checkerboard(v1, version=1, **OK)[0] == h
    got = codec.parse_checkerboard(v2, version=2, **OK)
    assert got[0] == h and got[4:] == (pz, pa, pn) and all(np.array_equal(a, b) for a, b in zip(got[1:4], (lz, la, ln)))
    with pytest.raises(ValueError, match="format version 2, this build reads 1"):
        codec.parse_checkerboard(v2, **OK)
    with pytest.raises(ValueError, match="format version 1, this build reads 2"):
        codec.parse_checkerboard(v1, version=2, **OK)
    for bad in (0, 3):
        with pytest.raises(ValueError, match="format version"):
            codec.pack_checkerboard(h, lz, la, ln, pz, pa, pn, version=bad)
        with pytest.raises(ValueError, match="format version"):
            codec.parse_checkerboard(v1, version=bad, **OK)


# ------------------------------------------------------------------ the model
def _fused_cfg(kernel="fused"):
    cfg = _cfg(ARCH)
    cfg.MODEL.CONTEXT.KERNEL = kernel
    return cfg


def test_default_kernel_is_conv_and_the_key_changes_no_parameter():
    from image_compression_amd import get_cfg_defaults, modelling
    assert get_cfg_defaults().MODEL.CONTEXT.KERNEL == "conv"
    torch.manual_seed(0)
    conv = modelling.build_model(_cfg(ARCH))
    torch.manual_seed(0)
    fused = modelling.build_model(_fused_cfg())
    assert (conv.context_kernel, fused.context_kernel) == ("conv", "fused")
    sc, sf = conv.state_dict(), fused.state_dict()
    assert list(sc) == list(sf)
    for k in sc:
        assert torch.equal(sc[k], sf[k]), k
    assert fused.load_state_dict(sc, strict=True).missing_keys == []      # one checkpoint loads under either value
    assert conv.context_mean.math == fused.context_mean.math               # the training convs keep their arithmetic
    assert (conv._format_version(), fused._format_version()) == (1, 2)
    with pytest.raises(ValueError, match="MODEL.CONTEXT.KERNEL"):
        modelling.build_model(_fused_cfg("triton"))


def test_fused_model_refuses_training_mode_and_bad_streams_without_a_device():
    from image_compression_amd import codec, modelling
    model = modelling.build_model(_fused_cfg())
    x = torch.rand(1, 3, 64, 64)
    for call in (lambda: model.compress(x), lambda: model.decompress(b""), lambda: model.compress_each(x),
                 lambda: model.decompress_each([b""])):
        with pytest.raises(RuntimeError, match="eval"):
            call()
    model.eval()
    # everything is parsed before anything is launched: no device is needed to refuse these
    with pytest.raises(ValueError, match="multiples of 64"):
        model.compress(torch.rand(1, 3, 64, 72))
    with pytest.raises(ValueError, match="h, w >= 1"):
        model.compress_each(torch.rand(3, 64, 64))
    with pytest.raises(ValueError, match="shorter"):
        model.decompress(b"ICRC")
    with pytest.raises(ValueError, match="shorter"):
        model.decompress_each([b"ICRK"])
    cdc, hc, streams = _ckbd_container()
    (lz, pz), (la, pa), (ln, pn) = streams
    v1, v2 = _packed(cdc, hc, streams), cdc.pack_checkerboard(hc, lz, la, ln, pz, pa, pn, version=2)
    with pytest.raises(ValueError, match="format version 1"):
        model.decompress(v1)
    with pytest.raises(ValueError, match="different model"):       # the right version; 5 hyper channels, not 192
        model.decompress(v2)
    conv = modelling.build_model(_cfg(ARCH)).eval()
    with pytest.raises(ValueError, match="format version 2"):
        conv.decompress(v2)
    with pytest.raises(ValueError, match="magic"):
        model.decompress_each([v2])
    h, args = _image_stream(np.random.default_rng(24), compute_dtype="fp32_split")
    icrk = codec.pack_checkerboard_image(h, *args)
    with pytest.raises(ValueError, match="magic"):
        model.decompress(icrk)
    with pytest.raises(ValueError, match="different model|scale table"):
        model.decompress_each([icrk])
    with pytest.raises(ValueError, match="magic"):
        modelling.build_model(_cfg("MeanScaleCompressor2018")).eval().decompress_each([icrk])
    # the conv model keeps refusing per-image streams
    with pytest.raises(NotImplementedError, match=ARCH):
        conv.compress_each(x)
    with pytest.raises(NotImplementedError, match=ARCH):
        conv.decompress_each([icrk])


def test_fused_context_refuses_cpu_tensors_and_autograd():
    from image_compression_amd import functional as F
    from image_compression_amd import modelling
    model = modelling.build_model(_fused_cfg()).eval()
    y = torch.zeros(1, 192, 2, 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm"):
        model._context(y, y + 1, y)
    w, b = torch.zeros(4, 4, 5, 5, requires_grad=True), torch.zeros(4)
    t = torch.zeros(1, 4, 2, 2)
    with pytest.raises(RuntimeError, match="no backward"):
        F.ckbd_context(t, t, t, w, b, w, b)


# ------------------------------------------------------------------ the op and the library
def _meta(*shape):
    return torch.empty(*shape, device="meta")


def test_ctx_namespace_holds_the_context_op_with_a_meta_kernel():
    from image_compression_amd import _lib
    ops = _lib.ctx_ops()
    registered = {nm.split("::")[1] for nm in torch._C._dispatch_get_all_op_names() if nm.startswith("imgcomp_ctx::")}
    assert registered == {"context_fwd", "context_fwd_ws"}
    assert str(ops.context_fwd.default._schema) == (
        "imgcomp_ctx::context_fwd(Tensor y_in, Tensor mu_h, Tensor sigma_h, Tensor w_mean, Tensor b_mean, "
        "Tensor w_scale, Tensor b_scale) -> (Tensor, Tensor)")
    for N, H, W, C in ((2, 8, 12, 192), (1, 1, 1, 5), (3, 3, 5, 8)):
        t, w, b = _meta(N, H, W, C), _meta(C, C, 5, 5), _meta(C)
        for out in (ops.context_fwd(t, t, t, w, b, w, b),
                    ops.context_fwd_ws(t, t, t, w, b, w, b, torch.empty(16, dtype=torch.uint8, device="meta"), False)):
            assert len(out) == 2
            for o in out:       # the dense channels-last storage (N, H, W, C) of a logical (N, C, H, W) latent
                assert o.device.type == "meta" and tuple(o.shape) == (N, H, W, C) and o.is_contiguous()
                assert o.dtype == torch.float32 and not o.requires_grad
                v = o.movedim(-1, 1)
                assert tuple(v.shape) == (N, C, H, W) and (C == 1 or H * W == 1 or
                                                           v.is_contiguous(memory_format=torch.channels_last))
    t, w, b = _meta(2, 4, 4, 8), _meta(8, 8, 5, 5), _meta(8)
    with pytest.raises(RuntimeError, match="same shape"):
        ops.context_fwd(t, _meta(2, 4, 4, 7), t, w, b, w, b)
    with pytest.raises(RuntimeError, match="weight"):
        ops.context_fwd(t, t, t, _meta(8, 8, 3, 3), b, w, b)
    with pytest.raises(RuntimeError, match="bias"):
        ops.context_fwd(t, t, t, w, b, w, _meta(7))
    # CPU tensors: no kernel is registered for them, and nothing falls back to eager arithmetic
    c, cw, cb = torch.zeros(1, 2, 2, 8), torch.zeros(8, 8, 5, 5), torch.zeros(8)
    with pytest.raises((RuntimeError, NotImplementedError)):
        ops.context_fwd(c, c, c, cw, cb, cw, cb)


NAMES = {"ic_context_fwd", "ic_context_ws"}


def test_library_carries_the_context_symbols_and_checks_arguments_before_any_launch():
    from image_compression_amd import _lib
    txt = open(os.path.join(ROOT, "include", "imgcomp.h")).read()
    declared = set(re.findall(r"\b(ic_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert NAMES <= declared and NAMES <= set(_lib.SIGNATURES) and NAMES <= _lib.exported_symbols()
    L = _lib.load()
    assert L.ic_version() == 4          # additive: streams are still parsed with ABI version 4
    # the packed live taps: 2 heads x 12 taps x ceil(C / 8) groups x (C padded to 32) outputs x 8 channels, fp32
    for C, want in ((192, 2 * 12 * 24 * 192 * 8 * 4), (5, 2 * 12 * 1 * 32 * 8 * 4), (8, 2 * 12 * 1 * 32 * 8 * 4),
                    (33, 2 * 12 * 5 * 64 * 8 * 4), (0, 0), (-1, 0), (4097, 0)):
        assert L.ic_context_ws(C) == want, C
    p = [256 * (k + 1) for k in range(9)]    # distinct non-null pointers, never dereferenced: every call fails its checks
    ws, nb = 65536, L.ic_context_ws(6)

    def call(ptrs=p, dims=(2, 3, 5, 6), ws=ws, nb=nb, packed=0):
        return L.ic_context_fwd(*ptrs[:7], *dims, *ptrs[7:], ws, nb, packed, None)

    for k in range(9):                  # a null pointer, each in turn
        assert call([None if i == k else q for i, q in enumerate(p)]) == 1001, k
    assert call(ws=None) == 1001
    for bad in ((0, 3, 5, 6), (2, 0, 5, 6), (2, 3, -1, 6), (2, 3, 5, 0), (2 ** 31 - 1,) * 3 + (6,), (2, 3, 5, 4097)):
        assert call(dims=bad) == 1001, bad
    assert call(p[:7] + [p[7], p[7]]) == 1001                      # mu and sigma share a buffer
    for k in range(3):                                              # an output on top of an input
        assert call(p[:7] + [p[k], p[8]]) == 1001 and call(p[:7] + [p[7], p[k]]) == 1001, k
    assert call(ws=ws + 4) == 1001                                  # a workspace that is not 16-byte aligned
    assert call(nb=nb - 1) == 1002 and call(nb=0, packed=1) == 1002   # a short workspace
