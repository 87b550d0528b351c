"""Coding to a byte budget on the GPU: `measure_seg` against the coder's own lengths and the numpy reference coder,
the fused gain-and-symbolize kernel against `channel_scale` + `symbolize_mean_seg` on the gathered batch (bitwise), and
`compress_each_to` against a brute-force search from public calls (`compress_each` at every quality the rule visits,
the rule of tests/test_budget.py on the sizes)."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from planted_ties import _fusable
from test_budget import search
from test_codec import draw, random_tables, ref_encode
from test_gained_gpu import R_MODEL, S, TABLES, _dev, _model, _table_values, _tables
from test_mean_scale_gpu import KINDS, TIES, _batch, _changed, _pad

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------ measure_seg against the coder
def _measure_case(nseg, seg_len, Ks, R, nrows, rows_given, seed):
    """One launch of measure_seg and one of encode_seg on the same operands, and the reference coder's chunk sizes."""
    from image_compression_amd import _lib, codec
    rng = np.random.default_rng(seed)
    C = 4
    n = nseg * seg_len
    rows = rng.integers(0, nrows, n) if rows_given else np.arange(n) % C
    tabs = {K: random_tables(rng, nrows, K) for K in sorted(set(Ks))}
    offs, at = {}, 0
    for K, t in tabs.items():
        offs[K], at = at, at + t.size
    pool = torch.from_numpy(np.concatenate([t.reshape(-1) for t in tabs.values()]).astype(np.int32)).to(DEV)
    idx = [draw(rng, tabs[K], rows[s * seg_len:(s + 1) * seg_len]) for s, K in enumerate(Ks)]
    sym = torch.from_numpy(np.concatenate([i - K for i, K in zip(idx, Ks)]).astype(np.int32)).to(DEV)
    rows_d = torch.from_numpy(rows.astype(np.uint8)).to(DEV) if rows_given else None
    args = (sym, nseg, rows_d, 0 if rows_given else C, pool, nrows, list(Ks), [offs[K] for K in Ks], R)
    lens = _lib.rate_ops().measure_seg(*args)
    cps = codec.num_chunks(seg_len, R)
    assert lens.dtype == torch.int32 and lens.shape == (nseg * cps,) and lens.is_cuda
    got = lens.cpu().numpy().astype(np.int64).reshape(nseg, cps)
    packed = _lib.stream_ops().encode_seg(*args)
    coder = np.stack([l for l, _ in codec.split_packed_seg(packed.cpu().numpy(), nseg, seg_len, R)]).astype(np.int64)
    assert np.array_equal(got, coder), f"measure_seg {got.tolist()} is not encode_seg's lengths {coder.tolist()}"
    for s, K in enumerate(Ks):
        _, want = ref_encode(idx[s], rows[s * seg_len:(s + 1) * seg_len], tabs[K], R)
        assert np.array_equal(got[s], want.astype(np.int64)), f"segment {s} (K {K}) against the reference coder"
    assert torch.equal(_lib.rate_ops().measure_seg(*args), lens), "two runs give different lengths"
    return got


# R = 4: a single partial step, exactly one chunk, two chunks and a short last one; without rows the row is the
# global index % 4, which the entry point takes only for segments of whole positions: 36 stands in for 37 there
@pytest.mark.parametrize("rows_given", [True, False], ids=["rows", "index%4"])
@pytest.mark.parametrize("seg_len", [37, 256, 2 * 256 + 37])
def test_measure_seg_is_the_coders_length(seg_len, rows_given):
    if not rows_given:
        seg_len -= seg_len % 4
    got = _measure_case(1, seg_len, (37,), 4, 7, rows_given, seg_len)
    assert got.shape == (1, -(-seg_len // 256)) and (got >= 256).all() and (got % 2 == 0).all()


@pytest.mark.parametrize("rows_given", [True, False], ids=["rows", "index%4"])
@pytest.mark.parametrize("seg_len", [37, 256, 2 * 256 + 37])
def test_measure_seg_mixes_lds_and_pool_tables(seg_len, rows_given):
    """K = (1, 37, 2047) with 7 rows in one launch: 7 x 4096 x 4 bytes do not fit the 48 KiB the kernel stages, the
    other two tables do."""
    if not rows_given:
        seg_len -= seg_len % 4
    got = _measure_case(3, seg_len, (1, 37, 2047), 4, 7, rows_given, 100 + seg_len)
    assert got.shape == (3, -(-seg_len // 256))


# ------------------------------------------------------------------ the fused symbolizer
IMG = (0, 1, 1, 0, 1)


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("P", [1, 7, 48])
@pytest.mark.parametrize("C", [4, 5, 192])
def test_gain_symbolize_is_scale_then_symbolize_bitwise(C, P, offset):
    from image_compression_amd import _lib
    rng = np.random.default_rng(1000 * C + 10 * P + offset)
    N, M = 2, len(IMG)
    y = (rng.standard_normal((N, P, C)) * 20).astype(np.float32)
    g = np.exp(rng.uniform(-1.5, 1.5, (M, C))).astype(np.float32)
    mu = rng.standard_normal((M, P, C)).astype(np.float32)
    # ties at .5: channel 0 with a gain of 1 and channel 1 with a gain of 2, y g - mu = k + 0.5 exactly for every
    # candidate (k + 0.75, its half and 0.25 are exact in fp32); negative zeros in channels 2 and 3
    g[:, 0], g[:, 1] = 1.0, 2.0
    planted = []
    for t, (a, b) in enumerate(TIES[:2 * P]):
        p, c = t // 2, t % 2
        y[:, p, c] = a / g[0, c]
        mu[:, p, c] = b
        planted.append((p, c))
    y[:, 0, 2], mu[:, 0, 2] = -0.0, 0.0
    y[0, 0, 3], y[1, 0, 3], mu[:, 0, 3] = -0.0, 0.0, -0.0
    scaled = y[list(IMG)] * g[:, None, :]                      # one float32 multiplication per element
    d = scaled - mu                                            # one float32 subtraction per element
    assert scaled.dtype == d.dtype == np.float32
    for p, c in planted:
        assert (np.abs(d[:, p, c] - np.trunc(d[:, p, c])) == 0.5).all(), "the planted ties are not ties"
    assert np.signbit(d[:, 0, 2]).all() and (d[:, 0, 2] == 0).all()
    want = np.rint(d).astype(np.int32)
    yd, gd, md = _dev(y, offset), _dev(g, offset), _dev(mu, offset)
    sym, kmax = _lib.rate_ops().gain_symbolize_seg(yd, gd, md, list(IMG))
    assert sym.dtype == torch.int32 and sym.shape == (M * P * C,)
    # the two existing ops on the gathered batch
    gathered = yd[torch.tensor(IMG, device=DEV)].contiguous()
    ref_sym, ref_kmax = _lib.mean_ops().symbolize_seg(_lib.gain_ops().channel_scale(gathered, gd), md, M)
    assert torch.equal(sym, ref_sym), "not channel_scale + symbolize_mean_seg"
    assert list(kmax) == list(ref_kmax) == [int(np.abs(w).max()) for w in want.reshape(M, -1)]
    assert np.array_equal(sym.cpu().numpy(), want.reshape(-1)), "not numpy on the same fp32 inputs"
    sym2, kmax2 = _lib.rate_ops().gain_symbolize_seg(yd, gd, md, list(IMG))
    assert torch.equal(sym2, sym) and list(kmax2) == list(kmax)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_gain_symbolize_never_fuses_the_product_with_the_difference(offset):
    """Every element of candidate 0 is planted so that a kernel which contracts the product with the difference into
    one FMA gives another symbol (`_fusable`): gains of 1.3 and 0.7, whose products are inexact, where the ties of the
    test above sit behind gains of 1 and 2."""
    from image_compression_amd import _lib
    N, M, P, C = 1, 2, 16, 8
    g = np.empty((M, C), np.float32)
    g[:, 0::2], g[:, 1::2] = 1.3, 0.7
    y, mu = np.empty((N, P, C), np.float32), np.empty((M, P, C), np.float32)
    for c in range(C):
        y[0, :, c], mu[0, :, c] = _fusable(g[0, c], P, 10 * c + offset)
    mu[1] = mu[0] + np.float32(0.25)
    d = y[[0, 0]] * g[:, None, :] - mu
    assert d.dtype == np.float32 and (np.abs(d[0] - np.trunc(d[0])) == 0.5).all(), "the planted ties are not ties"
    want = np.rint(d).astype(np.int32)
    sym, _ = _lib.rate_ops().gain_symbolize_seg(*(_dev(t, offset) for t in (y, g, mu)), [0, 0])
    got = sym.cpu().numpy().reshape(M, P, C)
    print(f"gain_symbolize offset {offset}: {int((got != want).sum())} of {want.size} symbols differ from numpy, "
          f"{int((got[0] != want[0]).sum())} of {want[0].size} planted")
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} symbols moved: the product was fused"


def test_gain_symbolize_wrapper_and_the_limit():
    """The functional wrapper on (N, C, H, W) tensors of both layouts, and the symbolizers' ValueError for a
    candidate past the coder's limit."""
    from image_compression_amd import functional as IF
    from image_compression_amd.modelling.blocks.entropy_model import symbolize_mean_seg
    g0 = torch.Generator().manual_seed(5)
    y = (torch.randn(2, 8, 3, 5, generator=g0) * 10).to(DEV)
    g = (torch.rand(5, 8, generator=g0) + 0.5).to(DEV)
    mean = torch.randn(5, 8, 3, 5, generator=g0).to(DEV)
    want, want_k = symbolize_mean_seg(IF.channel_scale(y[torch.tensor(IMG, device=DEV)], g), mean)
    for cl in (False, True):
        yy = y.contiguous(memory_format=torch.channels_last) if cl else y
        sym, kmax = IF.gain_symbolize_seg(yy, g, mean, IMG)
        assert torch.equal(sym, want) and kmax == want_k
    big = y.clone()
    big[1, 2, 1, 1] = 1e6
    with pytest.raises(ValueError, match="candidate 1 .*2047"):
        IF.gain_symbolize_seg(big, g, mean, IMG)
    with pytest.raises(ValueError, match="names image 2"):
        IF.gain_symbolize_seg(y, g, mean, (0, 1, 2, 0, 1))
    with pytest.raises(ValueError, match="gains"):
        IF.gain_symbolize_seg(y, g[:4], mean, IMG)
    with pytest.raises(ValueError, match="mean"):
        IF.gain_symbolize_seg(y, g, mean[:4], IMG)


# ------------------------------------------------------------------ the model
CANDIDATES, ROUNDS = 4, 2


def _ladder():
    """DESIGN 11f's ladder: log_y = log_z = 0.3 s, the inverses -0.3 s."""
    up = 0.3 * torch.arange(S, dtype=torch.float32).view(-1, 1).expand(S, 192)
    return {name: (-up if "inv" in name else up).clone() for name in TABLES}


TABLE_SETS = {"ladder": _ladder, "random": _table_values}


class _Brute:
    """The size table from public calls: sizes(q)[n] = len of image n's stream from `compress_each` at quality q
    for every image; one call per distinct quality."""

    def __init__(self, model, x):
        self.model, self.x, self.table, self.streams = model, x, {}, {}

    def sizes(self, q):
        if q not in self.table:
            self.model.set_quality([q] * self.x.shape[0])
            self.streams[q] = self.model.compress_each(self.x, steps_per_chunk=R_MODEL)
            self.table[q] = [len(s) for s in self.streams[q]]
        return self.table[q]

    def expect(self, n, budget, candidates=CANDIDATES, rounds=ROUNDS):
        """(quality or None, smallest of round 1) of image n by the rule of tests/test_budget.py on this table."""
        q, smallest, _ = search(lambda v: self.sizes(v)[n], S, budget, candidates, rounds)
        return q, smallest


def _grid():
    from image_compression_amd import codec
    return codec.budget_grid(S, CANDIDATES)


def _budgets(brute):
    """Image 0: midway between two measured sizes; image 1: exactly a measured size; image 2: one byte above its
    largest.  All from round 1's table."""
    col = [sorted({brute.sizes(q)[n] for q in _grid()}) for n in range(3)]
    assert len(col[0]) >= 2, "image 0 codes to one size at every quality of the grid"
    mid = len(col[0]) // 2
    return [(col[0][mid - 1] + col[0][mid]) // 2, col[1][len(col[1]) // 2], col[2][-1] + 1]


@pytest.mark.parametrize("tables", sorted(TABLE_SETS))
@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_compress_each_to_is_the_brute_force_search(kind, dtype, tables):
    from image_compression_amd import codec
    model = _model(kind, dtype)
    shape = (3, 3, 72, 100)
    N, _, h, w = shape
    x = _batch(shape)
    with _changed(model, True), _tables(model, TABLE_SETS[tables]()):
        model.set_quality(1.25)
        brute = _Brute(model, x)
        budgets = _budgets(brute)
        expected = [brute.expect(n, budgets[n])[0] for n in range(N)]
        print(f"budget {kind[:5]} {dtype} {tables}: round 1 {[brute.table[q] for q in _grid()]} budgets {budgets} "
              f"expected {expected} over {len(brute.table)} qualities")
        assert None not in expected
        model.set_quality(1.25)
        streams, qualities = model.compress_each_to(x, budgets, steps_per_chunk=R_MODEL, candidates=CANDIDATES,
                                                    rounds=ROUNDS)
        assert model.quality == 1.25, "the call changed the model's quality"
        assert qualities == expected
        assert all(isinstance(q, float) and q == float(np.float32(q)) for q in qualities)
        assert all(isinstance(s, bytes) and len(s) <= b for s, b in zip(streams, budgets)), \
            ([len(s) for s in streams], budgets)
        assert [len(s) for s in streams] == [brute.sizes(q)[n] for n, q in enumerate(qualities)]
        heads = [codec.parse_gained_image(s, 4, dtype)[0] for s in streams]
        assert [hd.quality for hd in heads] == qualities
        again, q_again = model.compress_each_to(x, budgets, steps_per_chunk=R_MODEL, candidates=CANDIDATES, rounds=ROUNDS)
        assert again == streams and q_again == qualities, "a second call gives other bytes"
        model.set_quality(qualities)
        assert model.compress_each(x, steps_per_chunk=R_MODEL) == streams, "not compress_each at the returned qualities"
        want = []
        for n, q in enumerate(qualities):
            model.set_quality(q)
            want.append(model(_pad(x))[0][n, :, :h, :w])
        model.set_quality(1.25)
        got = model.decompress_each(streams)
        for n in range(N):
            assert torch.equal(got[n][0], want[n]), f"image {n} is not the eval forward's reconstruction at its quality"
            assert_close(model.decompress_each([streams[n]])[0][0].cpu().numpy(), want[n].cpu().numpy(), 1e-4,
                         f"image {n} alone")

        # a miss: image 0 one byte below its smallest size
        smallest = min(brute.sizes(q)[0] for q in _grid())
        missed = [smallest - 1] + budgets[1:]
        assert brute.expect(0, missed[0]) == (None, smallest)
        with pytest.raises(codec.BudgetError) as err:
            model.compress_each_to(x, missed, steps_per_chunk=R_MODEL, candidates=CANDIDATES, rounds=ROUNDS)
        assert (err.value.image, err.value.budget, err.value.smallest) == (0, missed[0], smallest)
        assert model.quality == 1.25 and model._gains is None
        loose, q_loose = model.compress_each_to(x, missed, steps_per_chunk=R_MODEL, candidates=CANDIDATES, rounds=ROUNDS,
                                                strict=False)
        assert q_loose == [0.0] + qualities[1:] and loose[1:] == streams[1:]
        assert loose[0] == brute.streams[0.0][0] and len(loose[0]) > missed[0]
        model.set_quality(S - 1)


@pytest.mark.parametrize("dtype", ["fp32_split", "fp32"])
@pytest.mark.parametrize("kind", KINDS)
def test_compress_each_to_variants(kind, dtype):
    """One budget for all images, a single round, and one 64 x 64 image, on the ladder tables."""
    model = _model(kind, dtype)
    x = _batch((3, 3, 72, 100))
    with _changed(model, True), _tables(model, _ladder()):
        brute = _Brute(model, x)
        budget = _budgets(brute)[0]
        small = max(min(brute.sizes(q)[n] for q in _grid()) for n in range(3))
        budget = max(budget, small)              # every image fits somewhere on the grid
        for rounds in (2, 1):
            expected = [brute.expect(n, budget, rounds=rounds)[0] for n in range(3)]
            model.set_quality(3.0)
            streams, qualities = model.compress_each_to(x, budget, steps_per_chunk=R_MODEL, candidates=CANDIDATES,
                                                        rounds=rounds)
            assert qualities == expected and model.quality == 3.0, rounds
            assert all(len(s) <= budget for s in streams)
            assert [len(s) for s in streams] == [brute.sizes(q)[n] for n, q in enumerate(qualities)]
            assert streams == [brute.streams[q][n] for n, q in enumerate(qualities)]
            if rounds == 1:
                assert set(qualities) <= set(_grid())
        x1 = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
        one = _Brute(model, x1)
        col = sorted({one.sizes(q)[0] for q in _grid()})
        b1 = (col[0] + col[-1]) // 2
        expected, _ = one.expect(0, b1)
        streams, qualities = model.compress_each_to(x1, [b1], steps_per_chunk=R_MODEL, candidates=CANDIDATES, rounds=ROUNDS)
        assert qualities == [expected] and len(streams) == 1 and len(streams[0]) <= b1
        assert streams[0] == one.streams[expected][0]
        model.set_quality(S - 1)
