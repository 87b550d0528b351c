"""Transcoding in the latent domain on the GPU: the requantizer against the four ops it replaces on the gathered batch
and against numpy on the same fp32 inputs (bitwise), re-chunking against `compress_each` at the other chunk size (byte
for byte) on the scale, mean-scale, gained and region models, requantization against the composition of existing calls
(byte for byte), and `transcode_each_to` against a brute-force search from `transcode_each` (the rule of
tests/test_transcode.py on the sizes).  No tolerance anywhere: bytes, bits and integers."""
import contextlib
import dataclasses
import functools

import numpy as np
import pytest
import torch

from planted_ties import _fusable
from test_budget_gpu import TABLE_SETS
from test_gained import cfg_of
from test_gained_gpu import S, _dev, _model as _gained, _tables
from test_mean_scale_gpu import KINDS, TIES, _last_analysis_conv, _model as _mean_scale
from test_region_gpu import _region_of
from test_transcode import tsearch

pytestmark = pytest.mark.gpu

DEV = "cuda"
R_MODEL, R_BIG = 16, 1024
IMG = (0, 1, 1, 0, 1)


# ------------------------------------------------------------------ the requantizer
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("P", [1, 7, 48])
@pytest.mark.parametrize("C", [4, 5, 192])
def test_requant_is_the_four_ops_and_numpy_bitwise(C, P, offset):
    from image_compression_amd import _lib
    rng = np.random.default_rng(1000 * C + 10 * P + offset)
    N, M = 2, len(IMG)
    r = np.rint(rng.standard_normal((N, P, C)) * 20).astype(np.float32)
    mu1 = rng.standard_normal((N, P, C)).astype(np.float32)
    a = np.exp(rng.uniform(-1.5, 1.5, (N, C))).astype(np.float32)
    b = np.exp(rng.uniform(-1.5, 1.5, (M, C))).astype(np.float32)
    mu2 = rng.standard_normal((M, P, C)).astype(np.float32)
    # ties at .5: a = 1 in channels 0 and 1, b = 1 in channel 0 and 2 in channel 1; r + mu1 = (k + 0.75) / b exactly (an
    # integer plus 0.75, 0.375 or 0.875), so ((r + mu1) a) b - 0.25 = k + 0.5 for every target
    a[:, :2], b[:, 0], b[:, 1] = 1.0, 1.0, 2.0
    planted = []
    for t, (top, low) in enumerate(TIES[:2 * P]):
        p, c = t // 2, t % 2
        half = top / b[0, c]
        r[:, p, c] = np.floor(half)
        mu1[:, p, c] = half - np.floor(half)
        mu2[:, p, c] = low
        planted.append((p, c))
    # negative zeros: -0 + -0 = -0, times positive gains -0, minus +0 = -0; and +0 - (-0) = +0
    r[:, 0, 2], mu1[:, 0, 2], mu2[:, 0, 2] = -0.0, -0.0, 0.0
    r[:, 0, 3], mu1[:, 0, 3], mu2[:, 0, 3] = -0.0, 0.0, -0.0
    src = list(IMG)
    y_hat = (r[src] + mu1[src]) * a[src][:, None, :]          # every operation one float32 operation per element
    d = y_hat * b[:, None, :] - mu2
    assert y_hat.dtype == d.dtype == np.float32
    for p, c in planted:
        assert (np.abs(d[:, p, c] - np.trunc(d[:, p, c])) == 0.5).all(), "the planted ties are not ties"
    assert np.signbit(d[:, 0, 2]).all() and (d[:, 0, 2] == 0).all() and not np.signbit(d[:, 0, 3]).any()
    want = np.rint(d).astype(np.int32)
    rd, m1d, ad, bd, m2d = (_dev(t, offset) for t in (r, mu1, a, b, mu2))
    sym, kmax = _lib.transcode_ops().requant_seg(rd, m1d, ad, bd, m2d, src)
    assert sym.dtype == torch.int32 and sym.shape == (M * P * C,)
    # the four existing ops on the gathered batch
    idx = torch.tensor(IMG, device=DEV)
    gr, gm, ga = rd[idx].contiguous(), m1d[idx].contiguous(), ad[idx].contiguous()
    summed = _lib.mean_ops().add_mean(gr.reshape(-1), gm).view(M, P, C)
    scaled = _lib.gain_ops().channel_scale(_lib.gain_ops().channel_scale(summed, ga), bd)
    ref_sym, ref_kmax = _lib.mean_ops().symbolize_seg(scaled, m2d, M)
    assert torch.equal(sym, ref_sym), "not add_mean + channel_scale + channel_scale + symbolize_mean_seg"
    assert list(kmax) == list(ref_kmax) == [int(np.abs(w).max()) for w in want.reshape(M, -1)]
    assert np.array_equal(sym.cpu().numpy(), want.reshape(-1)), "not numpy on the same fp32 inputs"
    sym2, kmax2 = _lib.transcode_ops().requant_seg(rd, m1d, ad, bd, m2d, src)
    assert torch.equal(sym2, sym) and list(kmax2) == list(kmax)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_requant_never_fuses_the_second_product_with_the_difference(offset):
    """Every element of target 0 is planted so that a kernel which contracts the second product with the difference
    into one FMA gives another symbol (`_fusable`): gains of 1.3 and 0.7, a = 1 so that r + mu1 is y_hat exactly."""
    from image_compression_amd import _lib
    N, M, P, C = 1, 2, 16, 8
    a = np.ones((N, C), np.float32)
    b = np.empty((M, C), np.float32)
    b[:, 0::2], b[:, 1::2] = 1.3, 0.7
    r, mu1 = np.empty((N, P, C), np.float32), np.empty((N, P, C), np.float32)
    mu2 = np.empty((M, P, C), np.float32)
    for c in range(C):
        y_hat, mu = _fusable(b[0, c], P, 10 * c + offset)
        r[0, :, c], mu1[0, :, c], mu2[0, :, c] = np.floor(y_hat), y_hat - np.floor(y_hat), mu
    assert np.array_equal(r[0] + mu1[0], (r[0].astype(np.float64) + mu1[0]).astype(np.float32)), "r + mu1 is not exact"
    mu2[1] = mu2[0] + np.float32(0.25)
    d = ((r[[0, 0]] + mu1[[0, 0]]) * a[[0, 0]][:, None, :]) * b[:, None, :] - mu2
    assert d.dtype == np.float32 and (np.abs(d[0] - np.trunc(d[0])) == 0.5).all(), "the planted ties are not ties"
    want = np.rint(d).astype(np.int32)
    sym, _ = _lib.transcode_ops().requant_seg(*(_dev(t, offset) for t in (r, mu1, a, b, mu2)), [0, 0])
    got = sym.cpu().numpy().reshape(M, P, C)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} symbols moved: a product was fused"


def test_requant_wrapper_and_the_limit():
    """The functional wrapper on (N, C, H, W) tensors of both layouts, and the symbolizers' ValueError for a target
    past the coder's limit."""
    from image_compression_amd import functional as IF
    from image_compression_amd.modelling.blocks.entropy_model import add_mean, symbolize_mean_seg
    g0 = torch.Generator().manual_seed(5)
    r = torch.round(torch.randn(2, 8, 3, 5, generator=g0) * 10).to(DEV)
    mu1 = torch.randn(2, 8, 3, 5, generator=g0).to(DEV)
    a = (torch.rand(2, 8, generator=g0) + 0.5).to(DEV)
    b = (torch.rand(5, 8, generator=g0) + 0.5).to(DEV)
    mu2 = torch.randn(5, 8, 3, 5, generator=g0).to(DEV)
    idx = torch.tensor(IMG, device=DEV)
    flat = r.movedim(1, -1).contiguous().reshape(-1)
    y_hat = IF.channel_scale(add_mean(flat, mu1), a)
    want, want_k = symbolize_mean_seg(IF.channel_scale(y_hat[idx], b), mu2)
    for cl in (False, True):
        rr, mm, m2 = ((t.contiguous(memory_format=torch.channels_last) if cl else t) for t in (r, mu1, mu2))
        sym, kmax = IF.requant_seg(rr, mm, a, b, m2, IMG)
        assert torch.equal(sym, want) and kmax == want_k
    big = r.clone()
    big[1, 2, 1, 1] = 1e6
    with pytest.raises(ValueError, match="target 1 .*2047"):
        IF.requant_seg(big, mu1, a, b, mu2, IMG)
    with pytest.raises(ValueError, match="names source 2"):
        IF.requant_seg(r, mu1, a, b, mu2, (0, 1, 2, 0, 1))
    with pytest.raises(ValueError, match="target gains"):
        IF.requant_seg(r, mu1, a, b[:4], mu2, IMG)
    with pytest.raises(ValueError, match="source gains"):
        IF.requant_seg(r, mu1, a[:1], b, mu2, IMG)
    with pytest.raises(ValueError, match="mean"):
        IF.requant_seg(r, mu1, a, b, mu2[:4], IMG)
    with pytest.raises(ValueError, match="mean"):
        IF.requant_seg(r, mu1[:1], a, b, mu2, IMG)


# ------------------------------------------------------------------ the models
@functools.lru_cache(maxsize=None)
def _scale(kind, dtype):
    from image_compression_amd import modelling
    torch.manual_seed(0)
    return modelling.build_model(cfg_of("Compressor2018", kind, dtype)).to(DEV).eval()


class _x32:
    """The last analysis conv scaled by 32 (the existing tests' "x32"), for any of the models; undone on exit."""

    def __init__(self, model):
        self.w = _last_analysis_conv(model).weight

    def __enter__(self):
        with torch.no_grad():
            self.w.mul_(32.0)

    def __exit__(self, *exc):
        with torch.no_grad():
            self.w.div_(32.0)


class _count_transforms:
    """Counts the calls of g_a and g_s while it is open."""

    def __init__(self, model):
        self.mods, self.calls = (model.analysis_transform, model.synthesis_transform), 0

    def __enter__(self):
        def counting(orig):
            def forward(*a, **kw):
                self.calls += 1
                return orig(*a, **kw)
            return forward
        for m in self.mods:
            m.forward = counting(m.forward)
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            del m.forward


@functools.lru_cache(maxsize=None)
def _images():
    g = torch.Generator().manual_seed(7)
    return torch.rand(2, 3, 100, 136, generator=g).to(DEV), torch.rand(1, 3, 64, 64, generator=g).to(DEV)


def _arch(arch, kind, dtype):
    """(model, a function that sets what the next compress_each of a batch of padded size H x W codes at)."""
    if arch == "scale":
        return _scale(kind, dtype), lambda H, W: None
    if arch == "mean-scale":
        return _mean_scale(kind, dtype), lambda H, W: None
    if arch == "gained":
        model = _gained(kind, dtype)
        return model, lambda H, W: model.set_quality(2.5)
    model = _region_of(kind, dtype)

    def non_uniform(H, W):
        codes = (np.arange((H // 64) * (W // 64), dtype=np.int64) * 97 % 256).astype(np.uint8).reshape(H // 64, W // 64)
        codes[0, 0] = 255
        model.set_quality_map(codes)
    return model, non_uniform


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arch", ["scale", "mean-scale", "gained", "region"])
def test_rechunking_gives_compress_each_at_the_other_chunk_size(arch, kind, dtype):
    model, prepare = _arch(arch, kind, dtype)
    x, x1 = _images()
    tables = _tables(model) if arch in ("gained", "region") else contextlib.nullcontext()
    with _x32(model), tables:
        coded = {}
        for R in (R_MODEL, R_BIG):
            prepare(128, 192)
            two = model.compress_each(x, steps_per_chunk=R)
            prepare(64, 64)
            coded[R] = two + model.compress_each(x1, steps_per_chunk=R)
        small, big = coded[R_MODEL], coded[R_BIG]
        assert small != big
        if arch == "region":
            model.set_quality_map(None)               # the map comes from the streams
        with _count_transforms(model) as seen:
            out = model.transcode_each(small, steps_per_chunk=R_BIG)          # two sizes in one call
            back = model.transcode_each(out, steps_per_chunk=R_MODEL)
            mixed = model.transcode_each([small[0], big[1], small[2]], steps_per_chunk=R_BIG)
            kept = model.transcode_each(small)
        assert seen.calls == 0, "g_a or g_s ran"
        assert all(isinstance(s, bytes) for s in out) and out == big, "not compress_each at the new chunk size"
        assert back == small, "R1 -> R2 -> R1 is not the original"
        assert mixed == big and mixed[1] is big[1], "a stream already at the target is not the same object"
        assert all(a is b for a, b in zip(kept, small))
        for a, b in zip(model.decompress_each(out), model.decompress_each(small)):
            assert torch.equal(a, b)
        box = (10, 20, 40, 50)
        assert torch.equal(model.decompress_window([out[0]], [box])[0], model.decompress_window([small[0]], [box])[0])
        assert model.transcode_each(small[:1], steps_per_chunk=64) == model.transcode_each(big[:1], steps_per_chunk=64)


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_zero_tables_transcode_to_compress_each_at_the_other_quality(kind, dtype):
    """A fresh gained model: all gains are exactly 1, so only the header's quality differs from the input."""
    from image_compression_amd import codec
    model = _gained(kind, dtype)
    x, _ = _images()
    with _x32(model):
        model.set_quality(float(S - 1))
        src = model.compress_each(x, steps_per_chunk=R_MODEL)
        model.set_quality(2.0)
        want = model.compress_each(x, steps_per_chunk=R_MODEL)
        model.set_quality(float(S - 1))
        got = model.transcode_each(src, qualities=2.0)
        assert got == want and got != src
        head = codec._GAINED_IMAGE_HEAD.size
        assert [g[head:] for g in got] == [s[head:] for s in src] and [g[:head - 4] for g in got] == [s[:head - 4] for s in src]
        assert model.quality == float(S - 1)


def _reference(model, stream, q2, R, dtype):
    """(the stream, x_hat) of `stream` requantized to q2 from existing calls only, one stream at batch shape 1:
    decompress_seg -> add_mean / channel_scale x 2 -> symbolize_mean_seg -> encode_symbols_seg -> _pack_image, z by the
    rule's own line."""
    from image_compression_amd.functional import channel_scale
    from image_compression_amd.modelling.blocks.entropy_model import (add_mean, symbolize_mean_seg, symbolize_seg,
                                                                      symbols_as_tensor)
    em, cm = model.entropy_model, model.conditional_model
    h, lz, ly, pz, py = model._parse_image(stream, 4, dtype)
    try:
        model._use([h.quality])
        _, g_inv_y1, _, g_inv_z1 = model._gains
        k_z1 = em.decompress_seg([pz], h.z_shape, [lz], [h.kmax_z], h.R)
        z_hat1 = channel_scale(k_z1, g_inv_z1)
        sigma1, mu1 = model._prior(z_hat1)
        y_hat1 = channel_scale(cm.decompress_seg([py], sigma1, [ly], [h.kmax_y], h.R, mean=mu1), g_inv_y1)
        model._use([q2])
        g_y2, _, g_z2, g_inv_z2 = model._gains
        z_sym, kz = symbolize_seg(channel_scale(z_hat1, g_z2))
        z_hat2 = channel_scale(symbols_as_tensor(z_sym.to(torch.float32), h.z_shape), g_inv_z2)
        sigma2, mu2 = model._prior(z_hat2)
        y_sym, ky = symbolize_mean_seg(channel_scale(y_hat1, g_y2), mu2)
        sz = em.encode_symbols_seg(z_sym, kz, R)
        sy = cm.encode_symbols_seg(y_sym, ky, sigma2.expand_as(mu2), R, mean=mu2)
        h2 = dataclasses.replace(h, quality=q2, kmax_z=kz[0], kmax_y=ky[0], R=R)
        out = model._pack_image(h2, sz[0][1], sy[0][1], sz[0][0], sy[0][0])
        x_hat = model._reconstruct_each(model._latent_ungain(add_mean(y_sym.to(torch.float32), mu2)), [h2])[0]
    finally:
        model._end_call()
    return out, x_hat


@pytest.mark.parametrize("tables", sorted(TABLE_SETS))
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_requantization_is_the_composition_of_existing_calls(kind, dtype, tables):
    from image_compression_amd import codec
    model = _gained(kind, dtype)
    x, x1 = _images()
    with _x32(model), _tables(model, TABLE_SETS[tables]()):
        model.set_quality([float(S - 1), 3.5])
        streams = model.compress_each(x, steps_per_chunk=R_MODEL)
        model.set_quality(4.0)
        streams += model.compress_each(x1, steps_per_chunk=R_MODEL)
        model.set_quality(1.25)
        targets = [2.0, 1.25, 0.5]
        with _count_transforms(model) as seen:
            out = model.transcode_each(streams, qualities=targets)            # two sizes, a quality per stream
            alone = [model.transcode_each([s], qualities=[q])[0] for s, q in zip(streams, targets)]
            scalar = model.transcode_each(streams[:2], qualities=2.0)
            both = model.transcode_each(streams, qualities=targets, steps_per_chunk=R_BIG)
            same = model.transcode_each(streams, qualities=[float(S - 1), 3.5, 4.0])
        assert seen.calls == 0, "g_a or g_s ran"
        assert model.quality == 1.25 and model._gains is None, "the call changed the model's quality"
        ref = [_reference(model, s, q, R_MODEL, dtype) for s, q in zip(streams, targets)]
        assert out == [r[0] for r in ref], "not the composition of the existing calls"
        assert all(a != b for a, b in zip(out, streams))
        heads = [codec.parse_gained_image(s, 4, dtype)[0] for s in out]
        assert [h.quality for h in heads] == targets and [h.R for h in heads] == [R_MODEL] * 3
        assert alone == out, "streams transcoded together are not the streams one by one"
        assert scalar[0] == out[0] and scalar[1] == _reference(model, streams[1], 2.0, R_MODEL, dtype)[0]
        assert both == model.transcode_each(out, steps_per_chunk=R_BIG)
        assert both == [_reference(model, s, q, R_BIG, dtype)[0] for s, q in zip(streams, targets)]
        assert all(a is b for a, b in zip(same, streams)), "an equal quality was requantized"
        for s, (_, want) in zip(out, ref):      # alone, as the reference runs g_s: at batch shape 1
            assert torch.equal(model.decompress_each([s])[0], want), "not g_s of the requantized latent"
        model.set_quality(float(S - 1))


CANDIDATES, ROUNDS = 4, 2


class _Brute:
    """The size table from `transcode_each`: sizes(q)[m] = len of stream m requantized to q; one call per quality."""

    def __init__(self, model, streams, q1):
        self.model, self.src, self.q1, self.table, self.streams = model, streams, q1, {}, {}

    def sizes(self, q):
        if q not in self.table:
            self.streams[q] = self.model.transcode_each(self.src, qualities=q)
            self.table[q] = [len(s) for s in self.streams[q]]
        return self.table[q]

    def first(self, m):
        from image_compression_amd import codec
        return [q for q in codec.budget_grid(S, CANDIDATES) if q < self.q1[m]]

    def expect(self, m, budget, rounds=ROUNDS):
        """(quality, smallest of round 1) of stream m: its own quality where it fits, else the rule of
        tests/test_transcode.py on this table."""
        if len(self.src[m]) <= budget:
            return self.q1[m], None
        q, smallest, _ = tsearch(lambda v: self.sizes(v)[m], S, self.q1[m], len(self.src[m]), budget, CANDIDATES, rounds)
        return q, smallest


@pytest.mark.parametrize("tables", sorted(TABLE_SETS))
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_transcode_each_to_is_the_brute_force_search(kind, dtype, tables):
    from image_compression_amd import codec
    model = _gained(kind, dtype)
    x, x1 = _images()
    with _x32(model), _tables(model, TABLE_SETS[tables]()):
        q1 = [float(S - 1), 3.25, 4.0, 1.0]
        model.set_quality(q1[:2])
        streams = model.compress_each(x, steps_per_chunk=R_MODEL)
        model.set_quality(q1[2])
        streams += model.compress_each(x1, steps_per_chunk=R_MODEL)
        model.set_quality(q1[3])
        streams += model.compress_each(x[:1], steps_per_chunk=R_MODEL)
        model.set_quality(1.25)
        brute = _Brute(model, streams, q1)
        col = [sorted({brute.sizes(q)[m] for q in brute.first(m)}) for m in range(4)]
        assert all(len(c) >= 2 for c in col[:3]), col
        # midway between two sizes; exactly a size; midway; at least the stream's own size
        budgets = [(col[0][-2] + col[0][-1]) // 2, col[1][-1], (col[2][0] + col[2][1]) // 2, len(streams[3])]
        expected = [brute.expect(m, budgets[m])[0] for m in range(4)]
        print(f"transcode budget {kind[:5]} {dtype} {tables}: sizes {[len(s) for s in streams]} round 1 {col} budgets "
              f"{budgets} expected {expected} over {len(brute.table)} qualities")
        assert None not in expected and expected[3] == q1[3]
        with _count_transforms(model) as seen:
            out, qualities = model.transcode_each_to(streams, budgets, candidates=CANDIDATES, rounds=ROUNDS)
        assert seen.calls == 0, "g_a or g_s ran"
        assert model.quality == 1.25 and model._gains is None, "the call changed the model's quality"
        assert qualities == expected
        assert all(isinstance(q, float) and q == float(np.float32(q)) for q in qualities)
        assert all(isinstance(s, bytes) and len(s) <= b for s, b in zip(out, budgets)), ([len(s) for s in out], budgets)
        assert out[3] is streams[3], "a stream that fits is not the same object"
        assert out[:3] == [streams[m] if qualities[m] == q1[m] else brute.streams[qualities[m]][m] for m in range(3)], \
            "not transcode_each at the returned qualities"
        assert [codec.parse_gained_image(s, 4, dtype)[0].quality for s in out] == qualities
        again, q_again = model.transcode_each_to(streams, budgets, candidates=CANDIDATES, rounds=ROUNDS)
        assert again == out and q_again == qualities, "a second call gives other bytes"

        # one round, and one budget for all
        one = max(c[0] for c in col)
        for rounds in (1, 2):
            expected = [brute.expect(m, one, rounds)[0] for m in range(4)]
            got, qs = model.transcode_each_to(streams, one, candidates=CANDIDATES, rounds=rounds)
            assert qs == expected and None not in expected, rounds
            assert all(len(s) <= one for s in got)
            assert got == [streams[m] if qs[m] == q1[m] else brute.streams[qs[m]][m] for m in range(4)]
            if rounds == 1:
                assert all(q == q1[m] or q in brute.first(m) for m, q in enumerate(qs))

        # a miss: one byte below the smallest size of round 1, for a stream that is itself no smaller than that (on
        # the ladder every stream is; learnt tables need not be monotone)
        low = [col[m][0] for m in range(3)]
        k = next((m for m in (2, 1, 0) if len(streams[m]) >= low[m]), None)
        assert k is not None or tables != "ladder"
        if k is None:
            print(f"transcode budget {kind[:5]} {dtype} {tables}: every stream is smaller than all of its round 1, the "
                  f"miss is not exercised on these tables (sizes {[len(s) for s in streams[:3]]}, smallest {low})")
        if k is not None:
            missed = list(budgets)
            missed[k] = low[k] - 1
            assert brute.expect(k, missed[k]) == (None, low[k])
            with pytest.raises(codec.BudgetError) as err:
                model.transcode_each_to(streams, missed, candidates=CANDIDATES, rounds=ROUNDS)
            assert (err.value.image, err.value.budget, err.value.smallest) == (k, missed[k], low[k])
            assert model.quality == 1.25 and model._gains is None
            loose, q_loose = model.transcode_each_to(streams, missed, candidates=CANDIDATES, rounds=ROUNDS, strict=False)
            assert q_loose == qualities[:k] + [0.0] + qualities[k + 1:] and loose[3] is streams[3]
            assert [s for m, s in enumerate(loose) if m != k] == [s for m, s in enumerate(out) if m != k]
            assert loose[k] == brute.streams[0.0][k] and len(loose[k]) > missed[k]

        # another chunk size: the streams are re-chunked first, then searched at that size
        rechunked = model.transcode_each(streams, steps_per_chunk=R_BIG)
        big = [len(s) for s in rechunked]
        bounds = [big[0], big[1] - 1, big[2], big[3]]
        got, qs = model.transcode_each_to(streams, bounds, steps_per_chunk=R_BIG, candidates=CANDIDATES, rounds=1,
                                          strict=False)
        want, want_q = model.transcode_each_to(rechunked, bounds, candidates=CANDIDATES, rounds=1, strict=False)
        assert got == want and qs == want_q and qs[0] == q1[0] and qs[2:] == q1[2:] and qs[1] < q1[1]
        assert [g for m, g in enumerate(got) if m != 1] == [r for m, r in enumerate(rechunked) if m != 1]
        assert codec.parse_gained_image(got[1], 4, dtype)[0].R == R_BIG
        model.set_quality(float(S - 1))
