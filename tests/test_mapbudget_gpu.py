"""A quality map under a byte budget on the GPU: `block_allocate` against the rule of tests/test_mapbudget.py (bitwise),
the fused block-gain symbolizer against `block_scale` + `symbolize_mean_seg` on the gathered batch and against numpy
(bitwise), and `compress_each_map_to` against a brute force from public calls: `rate_distortion_map` at every level
gives the tables, the numpy allocation the map of every slope the rule visits, `set_quality_map` + `compress_each` its
size, and the search of tests/test_budget.py on the sizes the expected slopes."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from test_budget import search
from test_gained_gpu import R_MODEL, S, TABLES, _dev, _model, _table_values, _tables
from test_mapbudget import allocate, level_codes, weight
from test_mean_scale_gpu import KINDS, TIES, _changed, _pad

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARCH = "RegionGainedMeanScaleCompressor2018"
IMG = (0, 1, 1, 0, 1)


# ------------------------------------------------------------------ block_allocate
ONE_UP = 1.0 + 2.0 ** -12     # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 in float32: an inexact product
WEIGHTS = [float(np.float32(v)) for v in (0.0, ONE_UP, 1.0, 85.333336, 1e4)]


def _alloc_tables(N, L, nb, seed):
    """Finite tables (N, L, nb): rates that rise and errors that fall with the level, blocks of different activity, so
    that the levels' J cross between blocks; block 0 holds an exact tie of two levels at the minimum, block 1 (where
    there is one) a tie that exists only after the float32 rounding of the sum at w = 1."""
    rng = np.random.default_rng(seed)
    lv = np.arange(L, dtype=np.float64)[None, :, None]
    act = rng.uniform(0.2, 5.0, (N, 1, nb))
    bits = (200.0 * act * (1 + lv) * rng.uniform(0.9, 1.1, (N, L, nb))).astype(np.float32)
    sse = (300.0 * act ** 2 / (1 + lv) ** 2 * rng.uniform(0.9, 1.1, (N, L, nb))).astype(np.float32)
    a, b = (0, 1) if L == 2 else (1, L - 1)
    bits[:, :, 0], sse[:, :, 0] = 1000.0, 0.0
    bits[:, a, 0] = bits[:, b, 0] = 10.0
    if nb > 1:
        bits[:, :, 1], sse[:, :, 1] = 16777216.0, 0.0
        sse[:, 0, 1] = 1.0
    if nb > 2:
        # block 2, at w = 1 + 2^-12: level 0 has J = (-0.5 - 2^-11) + fl(w sse) = 0.5 exactly, a tie with level 1 that
        # goes to level 0; a fused multiply-add keeps the product's 2^-24 and would choose level 1
        bits[:, :, 2], sse[:, :, 2] = 1000.0, 0.0
        bits[:, 0, 2], sse[:, 0, 2], bits[:, 1, 2] = -0.5 - 2.0 ** -11, ONE_UP, 0.5
    return bits, sse


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("nb", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("L", [2, 5, 16])
def test_block_allocate_is_the_rule_bitwise(L, nb, offset):
    from image_compression_amd import _lib
    N, M = 2, len(IMG)
    bits, sse = _alloc_tables(N, L, nb, 1000 * L + 10 * nb + offset)
    lut = np.asarray([(37 * l + 5) % 256 for l in range(L)], dtype=np.uint8)
    want = np.stack([allocate(bits[n], sse[n], w) for n, w in zip(IMG, WEIGHTS)])
    a = 0 if L == 2 else 1
    assert (want[:, 0] == a).all(), "the planted tie does not go to the lower of its two levels"
    if nb > 1:
        assert want[2, 1] == 0 and want[3, 1] == 1, "the tie after rounding (w = 1) and its control (w > 1)"
    if nb > 2:
        assert want[1, 2] == 0, "the tie behind an inexact product"
        fused = float(bits[1, 0, 2]) + float(np.float32(ONE_UP)) * float(sse[1, 0, 2])      # exact in float64
        assert np.float32(fused) > np.float32(0.5), "a fused multiply-add would not tell"
    if nb >= 63:
        assert all(len(np.unique(row)) >= 2 for row in want[1:]), "the reference's maps hold one level only"
    bd, sd = _dev(bits, offset), _dev(sse, offset)
    ranks, codes, sums = _lib.alloc_ops().block_allocate(bd, sd, list(IMG), WEIGHTS, lut.tolist())
    assert ranks.dtype == codes.dtype == torch.uint8 and ranks.shape == codes.shape == (M, nb) and ranks.is_cuda
    assert sums.dtype == torch.float64 and sums.shape == (2, M)
    assert np.array_equal(ranks.cpu().numpy(), want), "not the allocation rule"
    assert np.array_equal(codes.cpu().numpy(), lut[want])
    col = np.arange(nb)
    ref = np.asarray([[t[n][want[m], col].astype(np.float64).sum() for m, n in enumerate(IMG)] for t in (bits, sse)])
    got = sums.cpu().numpy()
    print(f"block_allocate L {L} nb {nb}: sums' worst relative error "
          f"{(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max():.3g}")
    assert (np.abs(got - ref) <= 1e-12 * np.abs(ref)).all(), (got, ref)
    again = _lib.alloc_ops().block_allocate(bd, sd, list(IMG), WEIGHTS, lut.tolist())
    assert all(torch.equal(p, q) for p, q in zip(again, (ranks, codes, sums))), "two runs differ"


def test_block_allocate_wrapper_and_its_refusals():
    from image_compression_amd import functional as IF
    bits, sse = _alloc_tables(2, 6, 96, 3)
    bd, sd = torch.from_numpy(bits).to(DEV), torch.from_numpy(sse).to(DEV)
    ranks, codes, sums = IF.block_allocate(bd, sd, IMG, WEIGHTS, level_codes(6))
    want = np.stack([allocate(bits[n], sse[n], w) for n, w in zip(IMG, WEIGHTS)])
    assert np.array_equal(ranks.cpu().numpy(), want)
    assert np.array_equal(codes.cpu().numpy(), np.asarray(level_codes(6), dtype=np.uint8)[want])
    with pytest.raises(ValueError, match="names image 2"):
        IF.block_allocate(bd, sd, (0, 1, 2, 0, 1), WEIGHTS, level_codes(6))
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="weight of candidate 3"):
            IF.block_allocate(bd, sd, IMG, WEIGHTS[:3] + [bad] + WEIGHTS[4:], level_codes(6))
    with pytest.raises(ValueError, match="code of level 5"):
        IF.block_allocate(bd, sd, IMG, WEIGHTS, level_codes(6)[:5] + [256])
    with pytest.raises(RuntimeError, match="codes for 6 levels"):
        IF.block_allocate(bd, sd, IMG, WEIGHTS, level_codes(6)[:5])


# ------------------------------------------------------------------ the fused block-gain symbolizer
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (5, 7), (8, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [4, 5, 192])
def test_block_gain_symbolize_is_block_scale_then_symbolize_bitwise(C, shape, offset):
    from image_compression_amd import _lib
    Hm, Wm = shape
    rng = np.random.default_rng(1000 * C + 100 * Hm + 10 * Wm + offset)
    N, M, R, shift = 2, len(IMG), 3, 2
    hb, wb = -(-Hm // 4), -(-Wm // 4)
    y = (rng.standard_normal((N, Hm, Wm, C)) * 20).astype(np.float32)
    g = np.exp(rng.uniform(-1.5, 1.5, (R, C))).astype(np.float32)
    mu = rng.standard_normal((M, Hm, Wm, C)).astype(np.float32)
    rank = (2 * rng.integers(0, 2, (M, hb, wb))).astype(np.uint8)      # rows 0 and 2: row 1 is never used
    if hb * wb > 1:
        rank[:, 0, 0], rank[:, -1, -1] = 0, 2
    # ties at .5: channel 0 with a gain of 1 and channel 1 with a gain of 2 in every row, y g - mu = k + 0.5 exactly for
    # every candidate (k + 0.75, its half and 0.25 are exact in fp32); negative zeros in channels 2 and 3
    g[:, 0], g[:, 1] = 1.0, 2.0
    planted = []
    for t, (a, b) in enumerate(TIES[:2 * Hm * Wm]):
        (i, j), c = divmod(t // 2, Wm), t % 2
        y[:, i, j, c] = a / g[0, c]
        mu[:, i, j, c] = b
        planted.append((i, j, c))
    y[:, 0, 0, 2], mu[:, 0, 0, 2] = -0.0, 0.0
    y[0, 0, 0, 3], y[1, 0, 0, 3], mu[:, 0, 0, 3] = -0.0, 0.0, -0.0
    if Hm * Wm > 1:
        # a tie behind an inexact product, last position and channel: fl(y g) - mu = 0.5 exactly, symbol 0; a fused
        # multiply-add keeps the product's 2^-24 and gives 1
        g[:, -1], y[:, -1, -1, -1], mu[:, -1, -1, -1] = ONE_UP, ONE_UP, 0.5 + 2.0 ** -11
    up = np.repeat(np.repeat(rank, 4, axis=1), 4, axis=2)[:, :Hm, :Wm]           # the rank of every position
    scaled = y[list(IMG)] * g[up]                                               # one float32 multiplication per element
    d = scaled - mu                                                             # one float32 subtraction per element
    assert scaled.dtype == d.dtype == np.float32
    for i, j, c in planted:
        assert (np.abs(d[:, i, j, c] - np.trunc(d[:, i, j, c])) == 0.5).all(), "the planted ties are not ties"
    assert np.signbit(d[:, 0, 0, 2]).all() and (d[:, 0, 0, 2] == 0).all()
    want = np.rint(d).astype(np.int32)
    if Hm * Wm > 1:
        assert (d[:, -1, -1, -1] == 0.5).all() and (want[:, -1, -1, -1] == 0).all()
        assert np.float32(float(np.float32(ONE_UP)) ** 2 - float(mu[0, -1, -1, -1])) > np.float32(0.5)
    yd, gd, md = _dev(y, offset), _dev(g, offset), _dev(mu, offset)
    rd = torch.from_numpy(rank).to(DEV)
    sym, kmax = _lib.alloc_ops().block_gain_symbolize_seg(yd, gd, rd, md, list(IMG), shift)
    assert sym.dtype == torch.int32 and sym.shape == (M * Hm * Wm * C,)
    # the two existing ops on the gathered batch
    gathered = yd[torch.tensor(IMG, device=DEV)].contiguous()
    ref_sym, ref_kmax = _lib.mean_ops().symbolize_seg(_lib.region_ops().block_scale(gathered, gd, rd, shift), md, M)
    assert torch.equal(sym, ref_sym), "not block_scale + symbolize_mean_seg"
    assert list(kmax) == list(ref_kmax) == [int(np.abs(v).max()) for v in want.reshape(M, -1)]
    assert np.array_equal(sym.cpu().numpy(), want.reshape(-1)), "not numpy on the same fp32 inputs"
    sym2, kmax2 = _lib.alloc_ops().block_gain_symbolize_seg(yd, gd, rd, md, list(IMG), shift)
    assert torch.equal(sym2, sym) and list(kmax2) == list(kmax)


@pytest.mark.parametrize("C,shape,offset", [(192, (80, 84), 0), (5, (231, 229), 0), (4, (263, 257), 1)],
                         ids=["16-byte", "scalar-C5", "scalar-offset1"])
def test_block_gain_symbolize_walks_past_one_grid_stride(C, shape, offset):
    """More elements per image than one stride of the largest grid (1024 blocks of 256 threads, four elements each on the
    16-byte path): a thread's (row, column, channel) advance with their carries, and partial blocks at both edges."""
    from image_compression_amd import _lib
    Hm, Wm = shape
    assert Hm * Wm * C // (4 if C % 4 == 0 and not offset else 1) > 1024 * 256
    rng = np.random.default_rng(C)
    N, M, R, shift = 2, len(IMG), 3, 2
    hb, wb = -(-Hm // 4), -(-Wm // 4)
    y = (rng.standard_normal((N, Hm, Wm, C)) * 20).astype(np.float32)
    g = np.exp(rng.uniform(-1.5, 1.5, (R, C))).astype(np.float32)
    mu = rng.standard_normal((M, Hm, Wm, C)).astype(np.float32)
    rank = rng.integers(0, R, (M, hb, wb)).astype(np.uint8)
    up = np.repeat(np.repeat(rank, 4, axis=1), 4, axis=2)[:, :Hm, :Wm]
    want = np.rint(y[list(IMG)] * g[up] - mu).astype(np.int32)
    yd, gd, md = _dev(y, offset), _dev(g, offset), _dev(mu, offset)
    rd = torch.from_numpy(rank).to(DEV)
    sym, kmax = _lib.alloc_ops().block_gain_symbolize_seg(yd, gd, rd, md, list(IMG), shift)
    gathered = yd[torch.tensor(IMG, device=DEV)].contiguous()
    ref_sym, ref_kmax = _lib.mean_ops().symbolize_seg(_lib.region_ops().block_scale(gathered, gd, rd, shift), md, M)
    assert torch.equal(sym, ref_sym), "not block_scale + symbolize_mean_seg"
    assert list(kmax) == list(ref_kmax) == [int(np.abs(v).max()) for v in want.reshape(M, -1)]
    assert np.array_equal(sym.cpu().numpy(), want.reshape(-1)), "not numpy on the same fp32 inputs"


def test_block_gain_symbolize_wrapper_and_the_limit():
    """The functional wrapper on (N, C, H, W) tensors of both layouts, and the symbolizers' ValueError for a candidate
    past the coder's limit."""
    from image_compression_amd import functional as IF
    from image_compression_amd.modelling.blocks.entropy_model import symbolize_mean_seg
    g0 = torch.Generator().manual_seed(5)
    y = (torch.randn(2, 8, 5, 7, generator=g0) * 10).to(DEV)
    g = (torch.rand(3, 8, generator=g0) + 0.5).to(DEV)
    mean = torch.randn(5, 8, 5, 7, generator=g0).to(DEV)
    rank = torch.randint(0, 3, (5, 2, 2), generator=g0).to(torch.uint8).to(DEV)
    want, want_k = symbolize_mean_seg(IF.block_scale(y[torch.tensor(IMG, device=DEV)], g, rank, 2), mean)
    for cl in (False, True):
        yy = y.contiguous(memory_format=torch.channels_last) if cl else y
        sym, kmax = IF.block_gain_symbolize_seg(yy, g, rank, mean, IMG)
        assert torch.equal(sym, want) and kmax == want_k
    big = y.clone()
    big[1, 2, 1, 1] = 1e6
    with pytest.raises(ValueError, match="candidate 1 .*2047"):
        IF.block_gain_symbolize_seg(big, g, rank, mean, IMG)
    with pytest.raises(ValueError, match="names image 2"):
        IF.block_gain_symbolize_seg(y, g, rank, mean, (0, 1, 2, 0, 1))
    with pytest.raises(ValueError, match="gains"):
        IF.block_gain_symbolize_seg(y, g[:, :7], rank, mean, IMG)
    with pytest.raises(ValueError, match="rank map"):
        IF.block_gain_symbolize_seg(y, g, rank[:4], mean, IMG)
    with pytest.raises(ValueError, match="mean"):
        IF.block_gain_symbolize_seg(y, g, rank, mean[:, :, :4], IMG)


# ------------------------------------------------------------------ the model
CANDIDATES, ROUNDS = 4, 2
# The distortion weights of the test model's levels.  The weights are not trained, so the reconstruction hardly depends
# on the level: on these images a block's sse moves by about 1 between levels while its bits move by about 5000 per level
# of the ladder tables (printed by a run of the tables on the MI355X).  At the default weights (w = 85 .. 2731) every
# map would be level 0 everywhere, whatever the images; with w = 3.3 .. 3.3e5 the slopes of the grid lie on both sides
# of the crossing (w about 5e3 .. 1.5e5 on the ladder, 3 .. 3e3 on the random tables), so maps differ between slopes
# and between blocks.
WIDE = tuple(10.0 ** (1 + l) for l in range(S))


def _region_model(kind, dtype):
    return _model(kind, dtype, ARCH, WIDE)


def _ladder():
    """DESIGN 11f's ladder: log_y = log_z = 0.3 s, the inverses -0.3 s."""
    up = 0.3 * torch.arange(S, dtype=torch.float32).view(-1, 1).expand(S, 192)
    return {name: (-up if "inv" in name else up).clone() for name in TABLES}


TABLE_SETS = {"ladder": _ladder, "random": _table_values}


def _images(N=3, h=72, w=100, seed=7):
    """Images whose 64 x 64 blocks differ in activity: uniform noise about 0.5, its amplitude set per block."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, h, w, generator=g) - 0.5
    amp = torch.tensor([[1.0, 0.05], [0.3, 0.6]])
    for n in range(N):
        a = torch.roll(amp.flatten(), n).view(2, 2) * (1.0, 0.6, 0.25)[n % 3]
        x[n] *= a.repeat_interleave(64, 0).repeat_interleave(64, 1)[:h, :w]
    return (x + 0.5).to(DEV)


class _Brute:
    """Everything from public calls: the tables from `rate_distortion_map` at every level, the map of slope t by the
    numpy allocation, sizes(t)[n] = len of image n's stream from `set_quality_map` + `compress_each`."""

    def __init__(self, model, x):
        from image_compression_amd import codec
        self.model, self.x, self.table, self.streams, self.maps = model, x, {}, {}, {}
        N, _, h, w = x.shape
        self.hb, self.wb = -(-h // codec.MAP_BLOCK), -(-w // codec.MAP_BLOCK)
        bits, sse = [], []
        for l in range(S):
            model.set_quality(l)
            rd = model.rate_distortion_map(x)
            bits.append(rd.bits.reshape(N, -1))
            sse.append(rd.sse.reshape(N, -1))
        self.bits, self.sse = torch.stack(bits, 1), torch.stack(sse, 1)          # (N, S, nb)
        self.lut = np.asarray(level_codes(S), dtype=np.uint8)

    def map_of(self, t):
        if t not in self.maps:
            b, d = self.bits.cpu().numpy(), self.sse.cpu().numpy()
            w = weight(self.model.loss_weight(t), self.x.shape[1])
            self.maps[t] = np.stack([self.lut[allocate(b[n], d[n], w)].reshape(self.hb, self.wb)
                                     for n in range(self.x.shape[0])])
        return self.maps[t]

    def sizes(self, t):
        if t not in self.table:
            self.model.set_quality_map(self.map_of(t))
            self.streams[t] = self.model.compress_each(self.x, steps_per_chunk=R_MODEL)
            self.table[t] = [len(s) for s in self.streams[t]]
        return self.table[t]

    def expect(self, n, budget, candidates=CANDIDATES, rounds=ROUNDS):
        """(slope or None, smallest of round 1) of image n by the rule of tests/test_budget.py on this table."""
        t, smallest, _ = search(lambda v: self.sizes(v)[n], S, budget, candidates, rounds)
        return t, smallest


def _grid():
    from image_compression_amd import codec
    return codec.budget_grid(S, CANDIDATES)


def _budgets(brute):
    """Image 0: midway between two measured sizes; image 1: exactly a measured size; image 2: one byte above its
    largest.  All from round 1's table."""
    col = [sorted({brute.sizes(t)[n] for t in _grid()}) for n in range(3)]
    assert len(col[0]) >= 2, "image 0 codes to one size at every slope of the grid"
    mid = len(col[0]) // 2
    return [(col[0][mid - 1] + col[0][mid]) // 2, col[1][len(col[1]) // 2], col[2][-1] + 1]


SENTINEL = np.full((2, 2), 102, dtype=np.uint8)


def _untouched(model):
    return model.quality == 1.25 and np.array_equal(model.quality_map, SENTINEL) and model._gains is None \
        and model._codes is None and model._idx is None


def _mark(model):
    model.set_quality(1.25)
    model.set_quality_map(SENTINEL)


@pytest.mark.parametrize("tables", sorted(TABLE_SETS))
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_compress_each_map_to_is_the_brute_force_search(kind, dtype, tables):
    from image_compression_amd import codec
    model = _region_model(kind, dtype)
    x = _images()
    N, _, h, w = x.shape
    args = dict(steps_per_chunk=R_MODEL, candidates=CANDIDATES, rounds=ROUNDS)
    with _changed(model, True), _tables(model, TABLE_SETS[tables]()):
        brute = _Brute(model, x)
        _mark(model)
        bits, sse = model.rate_distortion_tables(x)
        assert _untouched(model)
        assert bits.dtype == sse.dtype == torch.float32 and bits.shape == sse.shape == (N, S, brute.hb * brute.wb)
        assert torch.equal(bits, brute.bits) and torch.equal(sse, brute.sse), \
            "the tables from one pass of g_a and h_a are not rate_distortion_map's at every level"
        budgets = _budgets(brute)
        expected = [brute.expect(n, budgets[n])[0] for n in range(N)]
        distinct = max(len(np.unique(m)) for maps in brute.maps.values() for m in maps)
        print(f"map budget {kind[:5]} {dtype} {tables}: round 1 {[brute.table[t] for t in _grid()]} budgets {budgets} "
              f"expected {expected} over {len(brute.table)} slopes; most distinct codes in a map {distinct}; maps at the "
              f"expected slopes {[brute.map_of(t)[n].reshape(-1).tolist() for n, t in enumerate(expected)]}")
        assert None not in expected
        assert distinct >= 2, "every brute-force map is uniform: the images' blocks do not differ enough"
        _mark(model)
        streams, maps, slopes = model.compress_each_map_to(x, budgets, **args)
        assert _untouched(model), "the call changed the model's quality or map"
        assert slopes == expected
        assert all(isinstance(t, float) and t == float(np.float32(t)) for t in slopes)
        assert all(isinstance(m, np.ndarray) and m.dtype == np.uint8 and m.shape == (brute.hb, brute.wb) for m in maps)
        assert all(np.array_equal(m, brute.map_of(t)[n]) for n, (m, t) in enumerate(zip(maps, slopes)))
        assert all(isinstance(s, bytes) and len(s) <= b for s, b in zip(streams, budgets)), \
            ([len(s) for s in streams], budgets)
        assert [len(s) for s in streams] == [brute.sizes(t)[n] for n, t in enumerate(slopes)]
        heads = [codec.parse_region_image(s, 4, dtype)[0] for s in streams]
        assert all(np.array_equal(hd.codes, m) for hd, m in zip(heads, maps))
        again, m_again, t_again = model.compress_each_map_to(x, budgets, **args)
        assert again == streams and t_again == slopes and all(np.array_equal(p, q) for p, q in zip(m_again, maps)), \
            "a second call gives other bytes"
        model.set_quality_map(np.stack(maps))
        assert model.compress_each(x, steps_per_chunk=R_MODEL) == streams, "not compress_each with the returned maps"
        want = model(_pad(x))[0][:, :, :h, :w]
        _mark(model)
        got = model.decompress_each(streams)
        for n in range(N):
            assert torch.equal(got[n][0], want[n]), f"image {n} is not the eval forward's reconstruction under its map"
            assert_close(model.decompress_each([streams[n]])[0][0].cpu().numpy(), want[n].cpu().numpy(), 1e-4,
                         f"image {n} alone")
        box = model.decompress_window([streams[0]], [(8, 16, 40, 60)])[0]
        assert_close(box[0].cpu().numpy(), want[0][:, 8:48, 16:76].cpu().numpy(), 1e-4, "a window of image 0")

        # a miss: image 0 one byte below its smallest size
        smallest = min(brute.sizes(t)[0] for t in _grid())
        missed = [smallest - 1] + budgets[1:]
        assert brute.expect(0, missed[0]) == (None, smallest)
        _mark(model)
        with pytest.raises(codec.BudgetError) as err:
            model.compress_each_map_to(x, missed, **args)
        assert (err.value.image, err.value.budget, err.value.smallest) == (0, missed[0], smallest)
        assert _untouched(model)
        loose, m_loose, t_loose = model.compress_each_map_to(x, missed, strict=False, **args)
        assert t_loose == [0.0] + slopes[1:] and loose[1:] == streams[1:]
        assert loose[0] == brute.streams[0.0][0] and len(loose[0]) > missed[0]
        assert np.array_equal(m_loose[0], brute.map_of(0.0)[0])
        model.set_quality(S - 1)


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_compress_each_map_to_variants(kind, dtype):
    """One budget for all images, a single round, and one 64 x 64 image, on the ladder tables."""
    model = _region_model(kind, dtype)
    x = _images()
    with _changed(model, True), _tables(model, _ladder()):
        brute = _Brute(model, x)
        budget = _budgets(brute)[0]
        small = max(min(brute.sizes(t)[n] for t in _grid()) for n in range(3))
        budget = max(budget, small)              # every image fits somewhere on the grid
        for rounds in (2, 1):
            expected = [brute.expect(n, budget, rounds=rounds)[0] for n in range(3)]
            _mark(model)
            streams, maps, slopes = model.compress_each_map_to(x, budget, steps_per_chunk=R_MODEL, candidates=CANDIDATES,
                                                               rounds=rounds)
            assert slopes == expected and _untouched(model), rounds
            assert all(len(s) <= budget for s in streams)
            assert streams == [brute.streams[t][n] for n, t in enumerate(slopes)]
            assert all(np.array_equal(m, brute.map_of(t)[n]) for n, (m, t) in enumerate(zip(maps, slopes)))
            if rounds == 1:
                assert set(slopes) <= set(_grid())
        x1 = _images(1, 64, 64, seed=9)
        one = _Brute(model, x1)
        col = sorted({one.sizes(t)[0] for t in _grid()})
        b1 = (col[0] + col[-1]) // 2
        expected, _ = one.expect(0, b1)
        streams, maps, slopes = model.compress_each_map_to(x1, [b1], steps_per_chunk=R_MODEL, candidates=CANDIDATES,
                                                           rounds=ROUNDS)
        assert slopes == [expected] and len(streams) == 1 and len(streams[0]) <= b1
        assert streams[0] == one.streams[expected][0] and maps[0].shape == (1, 1)
        assert np.array_equal(maps[0], one.map_of(expected)[0])
        model.set_quality(S - 1)
