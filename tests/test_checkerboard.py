"""The checkerboard context model on the CPU: the "ICRC" container with its three bitstreams, the packed order of a
half, the registration of CheckerboardCompressor2018 and of its ops and symbols, their host-side argument checks, and
the model's state dict beside MeanScaleCompressor2018's.  No GPU: the kernels and the model are held to numpy and
the fp64 oracle in tests/test_checkerboard_gpu.py."""
import dataclasses
import struct

import numpy as np
import pytest
import torch

from test_codec import _container, draw, random_tables, ref_encode
from test_stream import _image

OK = dict(abi=4, compute_dtype="fp32_split")
KIND_AT = 7        # magic (4), u16 format version, u8 arithmetic tag, u8 conditional kind
NEW_KEYS = {"context_mean.weight", "context_mean.bias", "context_scale.weight", "context_scale.bias"}


# ------------------------------------------------------------------ the container
def _ckbd_container(R=4, kind=2):
    """A header and three reference-coded streams: z, and the two halves of y, each chunked on its own."""
    from image_compression_amd import codec
    h = codec.Header(N=2, H=128, W=64, latent_channels=6, hyper_channels=5, kind=kind, compute_dtype="fp32_split", abi=4,
                     L=64, scale_min=0.11, scale_max=256.0, R=R, kmax_z=3, kmax_y=40)
    rng = np.random.default_rng(0)
    out = []
    for nsym, K in ((h.nsym_z, h.kmax_z), (h.nsym_y // 2, h.kmax_y), (h.nsym_y // 2, h.kmax_y)):
        cdf = random_tables(rng, 5, K)
        rows = np.arange(nsym) % 5
        payload, lens = ref_encode(draw(rng, cdf, rows), rows, cdf, R)
        out.append((lens, payload))
    return codec, h, out


def _packed(codec, h, streams):
    (lz, pz), (la, pa), (ln, pn) = streams
    return codec.pack_checkerboard(h, lz, la, ln, pz, pa, pn)


@pytest.mark.parametrize("kind", [2, 3])
def test_container_round_trips_the_mean_kinds(kind):
    codec, h, streams = _ckbd_container(kind=kind)
    data = _packed(codec, h, streams)
    assert isinstance(data, bytes) and data[:4] == b"ICRC" and data[KIND_AT] == kind
    h2, lz, la, ln, pz, pa, pn = codec.parse_checkerboard(data, **OK)
    assert h2 == h and h2.kind == kind
    for (lens, payload), lens2, payload2 in zip(streams, (lz, la, ln), (pz, pa, pn)):
        assert np.array_equal(lens2, lens) and payload2 == payload
    # each half of y is chunked from its own first symbol
    assert h.nsym_y == 2 * 6 * 8 * 4 and len(la) == len(ln) == codec.num_chunks(h.nsym_y // 2, h.R) == 1
    assert len(lz) == codec.num_chunks(h.nsym_z, h.R)
    nc = len(lz) + len(la) + len(ln)
    head = struct.calcsize("<4sHBBIIIIIIIddIIIQQIII")
    assert codec.checkerboard_fixed_bytes(h) == head + 4 * nc + 256 * nc
    assert len(data) == head + 4 * nc + sum(len(p) for _, p in streams)


def test_container_with_several_chunks_per_half():
    codec, h, streams = _ckbd_container(R=1)
    assert len(streams[1][0]) == len(streams[2][0]) == 3 and codec.num_chunks(h.nsym_y, 1) == 6
    h2, _, la, ln, _, pa, pn = codec.parse_checkerboard(_packed(codec, h, streams), **OK)
    assert h2 == h and np.array_equal(la, streams[1][0]) and pn == streams[2][1]


@pytest.mark.parametrize("kind", [0, 1, 4])
def test_kinds_without_a_mean_are_refused_at_pack_and_in_a_buffer(kind):
    codec, h, streams = _ckbd_container()
    with pytest.raises(ValueError, match="conditional kind"):
        _packed(codec, dataclasses.replace(h, kind=kind), streams)
    raw = bytearray(_packed(codec, h, streams))
    raw[KIND_AT] = kind
    with pytest.raises(ValueError, match="conditional kind"):
        codec.parse_checkerboard(bytes(raw), **OK)


def _field_offset(name):
    """Byte offset of one field of the "ICRC" header."""
    names = ["magic", "ver", "dt", "kind", "abi", "N", "H", "W", "cy", "cz", "L", "smin", "smax", "R", "kz", "ky", "nz", "ny",
             "ncz", "nca", "ncn"]
    fmt = "4sHBBIIIIIIIddIIIQQIII"
    # walk the format one field at a time (no padding with "<")
    fields, off, out = ["4s"] + list(fmt[2:]), 0, {}
    for nm, f in zip(names, fields):
        out[nm] = off
        off += struct.calcsize("<" + f)
    return out[name]


def test_parse_refuses_inconsistent_buffers():
    codec, h, streams = _ckbd_container()
    data = _packed(codec, h, streams)
    assert _field_offset("ncn") + 4 == struct.calcsize("<4sHBBIIIIIIIddIIIQQIII") and _field_offset("kind") == KIND_AT
    for cut in (0, 3, 50, _field_offset("ncn"), len(data) - 1):
        with pytest.raises(ValueError):
            codec.parse_checkerboard(data[:cut], **OK)
    with pytest.raises(ValueError):
        codec.parse_checkerboard(data + b"\0", **OK)

    def patched(name, fmt, value):
        raw = bytearray(data)
        struct.pack_into("<" + fmt, raw, _field_offset(name), value)
        return bytes(raw)

    # the symbols of y no longer make two halves of the batch shape
    for ny in (h.nsym_y - 1, h.nsym_y + 2, h.nsym_y // 2):
        with pytest.raises(ValueError, match="symbol counts"):
            codec.parse_checkerboard(patched("ny", "Q", ny), **OK)
    with pytest.raises(ValueError, match="symbol counts"):
        codec.parse_checkerboard(patched("nz", "Q", h.nsym_z + 1), **OK)
    # a wrong chunk count, in each of the three places (the ICRA count of all of y among them)
    for name, n in (("ncz", 2), ("nca", 2), ("ncn", 0), ("nca", codec.num_chunks(h.nsym_y, h.R) + 1)):
        with pytest.raises(ValueError, match="chunk counts"):
            codec.parse_checkerboard(patched(name, "I", n), **OK)
    with pytest.raises(ValueError, match="ABI"):
        codec.parse_checkerboard(data, abi=5, compute_dtype="fp32_split")
    with pytest.raises(ValueError, match="COMPUTE_DTYPE"):
        codec.parse_checkerboard(data, abi=4, compute_dtype="bf16")
    with pytest.raises(ValueError, match="format version"):
        codec.parse_checkerboard(patched("ver", "H", 2), **OK)
    # pack checks the same: a half with the chunks of the whole of y, a payload that is not its lengths' sum
    (lz, pz), (la, pa), (ln, pn) = streams
    with pytest.raises(ValueError, match="chunk"):
        codec.pack_checkerboard(h, lz, np.concatenate([la, la]), ln, pz, pa + pa, pn)
    with pytest.raises(ValueError, match="add up"):
        codec.pack_checkerboard(h, lz, la, ln, pz, pa, pn + b"\0\0")


def test_the_three_parsers_refuse_one_anothers_buffers():
    codec, h, (lz, pz), (ly, py) = _container()
    batch = codec.pack(dataclasses.replace(h, kind=2), lz, ly, pz, py)
    codec, hi, (lz, pz), (ly, py) = _image()
    image = codec.pack_image(dataclasses.replace(hi, kind=2), lz, ly, pz, py)
    codec, hc, streams = _ckbd_container()
    ckbd = _packed(codec, hc, streams)
    assert (batch[:4], image[:4], ckbd[:4]) == (b"ICRA", b"ICRP", b"ICRC")
    for parser, others in ((codec.parse, (image, ckbd)), (codec.parse_image, (batch, ckbd)),
                           (codec.parse_checkerboard, (batch, image))):
        for other in others:
            with pytest.raises(ValueError, match="magic"):
                parser(other, **OK)


@pytest.mark.parametrize("hw", [(1, 1), (1, 4), (3, 5), (4, 4), (5, 3)])
def test_packed_order_of_a_half_is_the_ascending_positions_of_its_parity(hw):
    from image_compression_amd import _lib, codec
    h, w = hw
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for parity in (0, 1):
        want = np.flatnonzero(((i + j) % 2 == parity).reshape(-1))        # ascending (i, j): numpy's own statement
        assert codec.checkerboard_count(h, w, parity) == want.size == _lib.load().ic_ckbd_count(h, w, parity)
        assert np.array_equal(codec.checkerboard_order(h, w, parity), want)
    assert codec.checkerboard_count(h, w, 0) + codec.checkerboard_count(h, w, 1) == h * w
    with pytest.raises(ValueError):
        codec.checkerboard_count(h, w, 2)
    with pytest.raises(ValueError):
        codec.checkerboard_count(0, w, 0)


# ------------------------------------------------------------------ the model
def _cfg(arch, kind="LaplacianConditionalModel"):
    from image_compression_amd import get_cfg_defaults
    cfg = get_cfg_defaults()
    cfg.MODEL.META_ARCHITECTURE = arch
    cfg.MODEL.ENTROPY_MODEL.CONDITIONAL_MODEL = kind
    return cfg


def test_model_is_registered_and_a_fresh_one_is_the_mean_scale_model_plus_a_zero_context():
    from image_compression_amd import modelling
    from image_compression_amd.modelling.layers import Conv2d
    from image_compression_amd.modelling.meta_arch import (META_ARCH_REGISTRY, CheckerboardCompressor2018,
                                                           MeanScaleCompressor2018)
    assert "CheckerboardCompressor2018" in META_ARCH_REGISTRY
    assert META_ARCH_REGISTRY.get("CheckerboardCompressor2018") is CheckerboardCompressor2018
    torch.manual_seed(0)
    base = modelling.build_model(_cfg("MeanScaleCompressor2018"))
    torch.manual_seed(0)
    model = modelling.build_model(_cfg("CheckerboardCompressor2018"))
    assert type(base) is MeanScaleCompressor2018 and type(model) is CheckerboardCompressor2018
    assert isinstance(model, MeanScaleCompressor2018)
    sd, bd = model.state_dict(), base.state_dict()
    assert set(sd) == set(bd) | NEW_KEYS and not NEW_KEYS & set(bd)
    for k, v in bd.items():
        assert torch.equal(sd[k], v), k
    for k in NEW_KEYS:
        assert tuple(sd[k].shape) == ((192, 192, 5, 5) if k.endswith("weight") else (192,)), k
        assert torch.count_nonzero(sd[k]) == 0, k
    for conv in (model.context_mean, model.context_scale):
        assert type(conv) is Conv2d and (conv.stride, conv.padding, conv.kernel_size) == ((1, 1), (2, 2), (5, 5))
        assert conv.math == model.prior_mean.math != 0
    modelling.meta_arch.build.set_compute_dtype(model, "fp32")
    assert model.context_mean.math == model.context_scale.math == model.prior_mean.math == 0
    modelling.meta_arch.build.set_compute_dtype(model, "bf16")
    assert model.context_mean.math == model.context_scale.math == model.prior_mean.math != 0
    # serial hyperprior, as inherited; the same stream kinds as the mean-scale model (no new kind value)
    assert model.concurrent_hyperprior is False and model.hyperprior_modules() == []
    assert model._stream_kind() == 2
    assert modelling.build_model(_cfg("CheckerboardCompressor2018", "GaussianConditionalModel"))._stream_kind() == 3


def test_mean_scale_checkpoint_loads_non_strictly_missing_the_context():
    from image_compression_amd import modelling
    torch.manual_seed(1)
    base = modelling.build_model(_cfg("MeanScaleCompressor2018"))
    torch.manual_seed(2)
    model = modelling.build_model(_cfg("CheckerboardCompressor2018"))
    res = model.load_state_dict(base.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(NEW_KEYS) and res.unexpected_keys == []
    for k, v in base.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    with pytest.raises(RuntimeError, match="context_mean"):
        model.load_state_dict(base.state_dict(), strict=True)


def test_model_refuses_to_code_in_training_mode_and_has_no_per_image_streams():
    from image_compression_amd import modelling
    model = modelling.build_model(_cfg("CheckerboardCompressor2018"))
    x = torch.rand(1, 3, 64, 64)
    for call in (lambda: model.compress(x), lambda: model.decompress(b""), lambda: model.compress_each(x),
                 lambda: model.decompress_each([b""])):
        with pytest.raises(RuntimeError, match="eval"):
            call()
    model.eval()
    with pytest.raises(NotImplementedError, match="CheckerboardCompressor2018"):
        model.compress_each(x)
    with pytest.raises(NotImplementedError, match="CheckerboardCompressor2018"):
        model.decompress_each([b""])
    # everything is parsed before anything is launched: no device is needed to refuse these
    with pytest.raises(ValueError, match="multiples of 64"):
        model.compress(torch.rand(1, 3, 64, 72))
    with pytest.raises(ValueError, match="shorter"):
        model.decompress(b"ICRC")
    codec, h, (lz, pz), (ly, py) = _container()
    with pytest.raises(ValueError, match="magic"):
        model.decompress(codec.pack(dataclasses.replace(h, kind=2), lz, ly, pz, py))
    codec, hc, streams = _ckbd_container()
    with pytest.raises(ValueError, match="magic"):
        modelling.build_model(_cfg("MeanScaleCompressor2018")).eval().decompress(_packed(codec, hc, streams))
    with pytest.raises(ValueError, match="different model"):       # 5 hyper channels, not the model's 192
        model.decompress(_packed(codec, hc, streams))


# ------------------------------------------------------------------ the library and the ops
NAMES = {"ic_ckbd_input_fwd", "ic_ckbd_input_bwd", "ic_ckbd_params_fwd", "ic_ckbd_params_bwd", "ic_ckbd_count",
         "ic_ckbd_gather", "ic_ckbd_scatter"}


def test_library_carries_the_checkerboard_symbols_and_checks_arguments_before_any_launch():
    from image_compression_amd import _lib
    assert NAMES <= set(_lib.SIGNATURES) and NAMES <= _lib.exported_symbols()
    assert {n for n in _lib.SIGNATURES if n.startswith("ic_ckbd_")} == NAMES
    L = _lib.load()
    assert L.ic_version() == 4
    p, q, r, s = 256, 512, 768, 1024    # non-null pointers that are never dereferenced: every call below fails its checks first
    dims = (2, 3, 5, 4)
    big = (2 ** 31 - 1,) * 4            # N H W C overflows 63 bits
    for bad in ((0, 3, 5, 4), (2, 0, 5, 4), (2, 3, -1, 4), (2, 3, 5, 0), big):
        assert L.ic_ckbd_input_fwd(p, p, *bad, q, r, None) == 1001
        assert L.ic_ckbd_input_bwd(p, p, p, p, *bad, q, r, None) == 1001
        assert L.ic_ckbd_params_fwd(p, p, p, p, *bad, q, r, None) == 1001
        assert L.ic_ckbd_params_bwd(p, p, p, p, *bad, p + 64, q, r, s, None) == 1001
        assert L.ic_ckbd_gather(p, 4, *bad, 0, q, None) == 1001
        assert L.ic_ckbd_scatter(p, *bad, 1, q, None) == 1001
    # a null pointer in every place
    for k in range(4):
        a = [p, p, q, r]
        a[k] = None
        assert L.ic_ckbd_input_fwd(a[0], a[1], *dims, a[2], a[3], None) == 1001
    for k in range(6):
        a = [p, p, p, p, q, r]
        a[k] = None
        assert L.ic_ckbd_input_bwd(*a[:4], *dims, *a[4:], None) == 1001
        assert L.ic_ckbd_params_fwd(*a[:4], *dims, *a[4:], None) == 1001
    for k in range(8):
        a = [p, p, p, p, p + 64, q, r, s]
        a[k] = None
        assert L.ic_ckbd_params_bwd(*a[:4], *dims, *a[4:], None) == 1001
    assert L.ic_ckbd_gather(None, 4, *dims, 0, q, None) == 1001
    assert L.ic_ckbd_gather(p, 4, *dims, 0, None, None) == 1001
    assert L.ic_ckbd_scatter(None, *dims, 0, q, None) == 1001
    assert L.ic_ckbd_scatter(p, *dims, 0, None, None) == 1001
    # outputs that share a buffer
    assert L.ic_ckbd_input_fwd(p, p, *dims, q, q, None) == 1001
    assert L.ic_ckbd_input_bwd(p, p, p, p, *dims, q, q, None) == 1001
    assert L.ic_ckbd_params_fwd(p, p, p, p, *dims, q, q, None) == 1001
    outs = [p + 64, q, r, s]
    for i in range(4):
        for j in range(i + 1, 4):
            o = list(outs)
            o[j] = o[i]
            assert L.ic_ckbd_params_bwd(p, p, p, p, *dims, *o, None) == 1001, (i, j)
    assert L.ic_ckbd_gather(p, 4, *dims, 0, p, None) == 1001
    assert L.ic_ckbd_scatter(p, *dims, 0, p, None) == 1001
    # parity and element size
    for parity in (-1, 2):
        assert L.ic_ckbd_gather(p, 4, *dims, parity, q, None) == 1001
        assert L.ic_ckbd_scatter(p, *dims, parity, q, None) == 1001
        assert L.ic_ckbd_count(3, 5, parity) == -1
    for eb in (0, 2, 3, 8):
        assert L.ic_ckbd_gather(p, eb, *dims, 0, q, None) == 1001
    assert L.ic_ckbd_count(0, 5, 0) == -1 and L.ic_ckbd_count(3, 0, 1) == -1


def test_count_is_brute_force_for_every_small_map():
    from image_compression_amd import _lib, codec
    L = _lib.load()
    for h in range(1, 10):
        for w in range(1, 10):
            for parity in (0, 1):
                want = sum((i + j) % 2 == parity for i in range(h) for j in range(w))
                assert L.ic_ckbd_count(h, w, parity) == want == codec.checkerboard_count(h, w, parity), (h, w, parity)
    assert L.ic_ckbd_count(2 ** 31 - 1, 2 ** 31 - 1, 0) == ((2 ** 31 - 1) ** 2 + 1) // 2


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_every_checkerboard_op_has_a_meta_kernel_and_checks_the_shapes():
    from image_compression_amd import _lib
    ops = _lib.ckbd_ops()
    t = _meta(2, 3, 5, 4)                         # (N, H, W, C): 8 anchors and 7 non-anchors per map
    full = (2, 3, 5, 4)
    cases = {
        "input_fwd": (lambda: ops.input_fwd(t, t), [full, full], torch.float32),
        "input_bwd": (lambda: ops.input_bwd(t, t, t, t), [full, full], torch.float32),
        "params_fwd": (lambda: ops.params_fwd(t, t, t, t), [full, full], torch.float32),
        "params_bwd": (lambda: ops.params_bwd(t, t, t, t), [full] * 4, torch.float32),
        "gather": (lambda: ops.gather(_meta(*full, dtype=torch.uint8), 1), [(2 * 7 * 4,)], torch.uint8),
        "scatter": (lambda: (ops.scatter(_meta(2 * 8 * 4), t, 0), ())[1], [], torch.float32),
    }
    registered = {nm.split("::")[1] for nm in torch._C._dispatch_get_all_op_names() if nm.startswith("imgcomp_ckbd::")}
    assert registered == set(cases), sorted(registered ^ set(cases))
    for name, (call, shapes, dtype) in cases.items():
        out = call()
        out = out if isinstance(out, tuple) else (out,)
        assert [tuple(o.shape) for o in out] == [tuple(s) for s in shapes], name
        assert all(o.device.type == "meta" and o.dtype == dtype for o in out), name
    assert tuple(ops.gather(_meta(*full, dtype=torch.int32), 0).shape) == (2 * 8 * 4,)
    assert ops.gather(_meta(*full, dtype=torch.int32), 0).dtype == torch.int32
    assert tuple(ops.gather(_meta(1, 1, 1, 6), 1).shape) == (0,)               # a 1 x 1 map has no non-anchor
    with pytest.raises(RuntimeError, match="same shape"):
        ops.input_fwd(t, _meta(2, 3, 5, 3))
    with pytest.raises(RuntimeError, match="same shape"):
        ops.params_bwd(t, t, _meta(2, 3, 4, 4), t)
    with pytest.raises(RuntimeError, match="parity"):
        ops.gather(t, 2)
    with pytest.raises(RuntimeError, match="values of parity"):
        ops.scatter(_meta(2 * 8 * 4), t, 1)
    with pytest.raises(RuntimeError, match=r"\(N, H, W, C\)"):
        ops.input_fwd(_meta(120), _meta(120))
