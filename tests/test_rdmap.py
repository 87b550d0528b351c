"""Rate and distortion maps without a GPU: the two ops of torch.ops.imgcomp_map and their shape kernels, the host-side
argument checks of ic_block_bits / ic_block_sse, the pixel counts of the blocks, and everything
`rate_distortion_map`, `functional.block_bits` and `functional.block_sse` refuse in front of any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gained import cfg_of

IC_ERR_ARG = 1001


@functools.lru_cache(maxsize=None)
def _model(arch):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return modelling.build_model(cfg_of(arch)).eval()


def _meta(*shape, cl=False):
    t = torch.empty(*shape, device="meta")
    return t.contiguous(memory_format=torch.channels_last) if cl else t


def test_ops_are_registered_with_shape_kernels():
    from image_compression_amd import _lib
    ops = _lib.map_ops()
    assert ops is torch.ops.imgcomp_map
    names = {n for n in torch._C._dispatch_get_all_op_names() if n.startswith("imgcomp_map::")}
    assert names == {"imgcomp_map::block_bits", "imgcomp_map::block_sse"}
    assert str(ops.block_bits.default._schema) == "imgcomp_map::block_bits(Tensor p, int shift, Tensor? add=None) -> Tensor"
    assert str(ops.block_sse.default._schema) == "imgcomp_map::block_sse(Tensor a, Tensor b, int shift) -> Tensor"
    for cl in (False, True):
        p = _meta(2, 192, 5, 7, cl=cl)
        out = ops.block_bits(p, 2)
        assert out.device.type == "meta" and out.dtype == torch.float32 and tuple(out.shape) == (2, 2, 2)
        assert out.is_contiguous()
        assert tuple(ops.block_bits(p, 0).shape) == (2, 5, 7)
        assert tuple(ops.block_bits(p, 2, out).shape) == (2, 2, 2)
        assert tuple(ops.block_bits(p, 6).shape) == (2, 1, 1)
    a = _meta(2, 3, 100, 70)
    assert tuple(ops.block_sse(a, _meta(2, 3, 100, 70, cl=True), 6).shape) == (2, 2, 2)
    for shift in (-1, 7):
        with pytest.raises(ValueError, match="shift"):
            ops.block_bits(_meta(1, 4, 4, 4), shift)
    with pytest.raises(RuntimeError, match="add"):
        ops.block_bits(_meta(2, 192, 5, 7), 2, _meta(2, 2, 3))
    with pytest.raises(RuntimeError, match="share a shape"):
        ops.block_sse(a, _meta(2, 3, 100, 71), 6)
    with pytest.raises(RuntimeError):
        ops.block_bits(_meta(192, 5, 7), 2)


def test_abi_version_is_unchanged():
    from image_compression_amd import _lib
    assert _lib.load().ic_version() == 4
    assert {"ic_block_bits", "ic_block_sse"} <= _lib.exported_symbols()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal returns IC_ERR_ARG from the host checks: nothing is launched, so no device is needed."""
    from image_compression_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    C, H, W = 4, 2, 2
    last, nchw = (1, W * C, C), (H * W, W, 1)

    def bits(p_=p, N=1, C_=C, H_=H, W_=W, sn=16, s=last, shift=2, out=p):
        return L.ic_block_bits(p_, N, C_, H_, W_, sn, *s, shift, None, out, None)

    def sse(a=p, b=p, N=1, C_=C, H_=H, W_=W, an=16, sa=last, bn=16, sb=nchw, shift=6, out=p):
        return L.ic_block_sse(a, b, N, C_, H_, W_, an, *sa, bn, *sb, shift, out, None)

    bad_bits = [dict(p_=None), dict(out=None), dict(N=0), dict(N=65536), dict(C_=0), dict(H_=0), dict(W_=0), dict(shift=-1),
                dict(shift=7), dict(sn=-1), dict(s=(2, W * C, C)), dict(s=(1, W * C + 1, C)), dict(s=(1, W * C, C + 1)),
                dict(s=(H * W, W, 2)), dict(C_=1 << 16, H_=1 << 8, W_=1 << 7, s=(1, 1 << 23, 1 << 16))]
    for kw in bad_bits:
        assert bits(**kw) == IC_ERR_ARG, kw
    bad_sse = [dict(a=None), dict(b=None), dict(out=None), dict(N=0), dict(N=65536), dict(C_=0), dict(H_=0), dict(W_=0),
               dict(shift=-1), dict(shift=7), dict(an=-1), dict(bn=-1), dict(sa=(1, W * C, C + 1)), dict(sb=(H * W, W + 1, 1)),
               dict(C_=1 << 16, H_=1 << 8, W_=1 << 7, sa=(1, 1 << 23, 1 << 16), sb=(1, 1 << 23, 1 << 16))]
    for kw in bad_sse:
        assert sse(**kw) == IC_ERR_ARG, kw


def test_block_pixels():
    from image_compression_amd.modelling.meta_arch.bmshl2018 import block_pixels
    px = block_pixels(100, 70)
    assert px.dtype == np.int64 and px.tolist() == [[4096, 384], [2304, 216]] and px.sum() == 7000
    assert block_pixels(128, 192).tolist() == [[4096] * 3] * 2
    assert block_pixels(1, 1).tolist() == [[1]]
    assert block_pixels(65, 64).tolist() == [[4096], [64]]


def test_result_type():
    from image_compression_amd.modelling.meta_arch.bmshl2018 import RDMap
    assert RDMap._fields == ("bits_y", "bits_z", "bits", "sse", "pixels", "x_hat", "p_y", "p_z")
    r = RDMap(*range(6))
    assert r.p_y is None and r.p_z is None and r.x_hat == 5


ARCHS = ["Compressor2018", "MeanScaleCompressor2018", "CheckerboardCompressor2018", "GainedMeanScaleCompressor2018",
         "RegionGainedMeanScaleCompressor2018"]


@pytest.mark.parametrize("arch", ARCHS)
def test_model_refuses_training_mode_and_a_3d_input(arch):
    model = _model(arch)
    owners = [k.__name__ for k in type(model).__mro__ if "rate_distortion_map" in vars(k)]
    assert owners == ["Compressor2018"], "the skeleton's method is overridden"
    x = torch.rand(1, 3, 64, 64)
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            model.rate_distortion_map(x)
    finally:
        model.eval()
    for bad in (torch.rand(3, 64, 64), torch.rand(1, 1, 3, 64, 64), torch.rand(1, 3, 0, 64)):
        with pytest.raises(ValueError, match="rate_distortion_map"):
            model.rate_distortion_map(bad)


def test_region_model_checks_its_map_against_the_padded_size():
    model = _model("RegionGainedMeanScaleCompressor2018")
    x = torch.rand(1, 3, 100, 200)                       # padded: 128 x 256, 2 x 4 blocks
    try:
        for shape in ((2, 2), (2, 3), (1, 4), (2, 2, 4)):
            model.set_quality_map(np.zeros(shape, np.uint8))
            with pytest.raises(ValueError, match=r"rate_distortion_map: the quality map .*padded size 128 x 256"):
                model.rate_distortion_map(x)
            assert model._gains is None and model._idx is None
    finally:
        model.set_quality_map(None)


@pytest.mark.parametrize("arch", ARCHS[3:])
def test_gained_models_refuse_a_sequence_of_qualities(arch):
    model = _model(arch)
    before = model.quality
    try:
        model.set_quality([1.0, 2.0])
        with pytest.raises(ValueError, match="rate_distortion_map takes one quality for the batch"):
            model.rate_distortion_map(torch.rand(2, 3, 64, 64))
        assert model._gains is None
    finally:
        model.set_quality(before)


def test_functional_is_inference_only():
    from image_compression_amd import functional as F
    p = torch.rand(1, 4, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="block_bits is inference only"):
        F.block_bits(p, 2)
    with pytest.raises(RuntimeError, match="block_bits is inference only"):
        F.block_bits(p.detach(), 2, add=torch.zeros(1, 1, 1, requires_grad=True))
    a = torch.rand(1, 3, 8, 8)
    for pair in ((a.clone().requires_grad_(True), a), (a, a.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="block_sse is inference only"):
            F.block_sse(*pair)
    # nothing runs on the host: a CPU tensor is an error, never a fallback
    with pytest.raises(RuntimeError, match="ROCm"):
        F.block_bits(p.detach(), 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm"):
        F.block_sse(a.requires_grad_(True), a)
