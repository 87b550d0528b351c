"""Coding to a byte budget without a GPU: the grid and the refinement of codec.py, the choice rule as a pure function on
made-up size tables (`search`, which tests/test_budget_gpu.py runs on brute-force sizes), the shape kernels of
torch.ops.imgcomp_rate, the host-side argument checks of the two C entry points and the refusals of
`compress_each_to` in front of any launch."""
import ctypes

import numpy as np
import pytest
import torch

from test_gained import cfg_of

S = 6


# ------------------------------------------------------------------ the rule, stated on its own
def grid(S_, Q):
    return [float(np.float32(k * (S_ - 1) / (Q - 1))) for k in range(Q)]


def refine(lo, hi, Q):
    out = []
    for j in range(1, Q + 1):
        q = float(np.float32(lo + j * (hi - lo) / (Q + 1)))
        if lo < q < hi and q not in out:
            out.append(q)
    return sorted(out)


def search(size_of, S_, budget, candidates, rounds):
    """(chosen quality or None, the smallest size of round 1, the qualities measured) for one image whose stream at
    quality q is size_of(q) bytes long: the rule of the issue, written without codec.py's functions."""
    seen = {q: size_of(q) for q in grid(S_, candidates)}
    smallest = min(seen.values())
    fit = [q for q, n in seen.items() if n <= budget]
    if not fit:
        return None, smallest, sorted(seen)
    chosen = max(fit)
    for _ in range(rounds - 1):
        above = [q for q in seen if q > chosen]
        if not above:             # chosen is S - 1
            break
        new = {q: size_of(q) for q in refine(chosen, min(above), candidates)}
        seen.update(new)
        fit = [q for q, n in new.items() if n <= budget]
        if fit:
            chosen = max(fit)
    return chosen, smallest, sorted(seen)


# ------------------------------------------------------------------ budget_grid / budget_refine
@pytest.mark.parametrize("levels", [2, 6, 8])
@pytest.mark.parametrize("Q", [2, 3, 4, 8, 64])
def test_grid_has_exact_ends_and_float32_values(levels, Q):
    from image_compression_amd import codec
    g = codec.budget_grid(levels, Q)
    assert g == grid(levels, Q) and len(g) == Q
    assert g[0] == 0.0 and g[-1] == float(levels - 1)
    assert all(isinstance(q, float) and q == float(np.float32(q)) for q in g)
    assert all(a < b for a, b in zip(g, g[1:]))


def test_refine_is_strictly_inside_ascending_and_distinct():
    from image_compression_amd import codec
    for lo, hi, Q in ((0.0, 5.0, 8), (1.25, 2.5, 4), (0.0, float(np.float32(5 / 3)), 4), (4.0, 5.0, 64), (2.0, 2.5, 1)):
        r = codec.budget_refine(lo, hi, Q)
        assert r == refine(lo, hi, Q) and len(r) == Q
        assert all(q == float(np.float32(q)) and lo < q < hi for q in r)
        assert all(a < b for a, b in zip(r, r[1:]))
    # adjacent floats have nothing between them; close ones have fewer values than candidates
    lo = float(np.float32(1.7))
    hi = float(np.nextafter(np.float32(lo), np.float32(9)))
    assert codec.budget_refine(lo, hi, 8) == []
    assert codec.budget_refine(lo, lo, 8) == []
    hi3 = float(np.nextafter(np.nextafter(np.float32(hi), np.float32(9)), np.float32(9)))
    r = codec.budget_refine(lo, hi3, 8)
    assert r == refine(lo, hi3, 8) and 1 <= len(r) <= 2 and all(lo < q < hi3 for q in r)


def test_bad_candidate_counts_are_refused():
    from image_compression_amd import codec
    for Q in (1, 0, -3, 2.0, True, None, "4"):
        with pytest.raises(ValueError):
            codec.budget_grid(S, Q)
    for Q in (0, -1, 1.5, False, None):
        with pytest.raises(ValueError):
            codec.budget_refine(0.0, 1.0, Q)
    for levels in (1, 0, True):
        with pytest.raises(ValueError):
            codec.budget_grid(levels, 4)
    with pytest.raises(ValueError):
        codec.budget_refine(2.0, 1.0, 4)
    with pytest.raises(ValueError):
        codec.budget_refine(float("nan"), 1.0, 4)


# ------------------------------------------------------------------ the choice rule on made-up tables
def _by_codec(size_of, S_, budget, candidates, rounds):
    """The search as `compress_each_to` runs it, from codec.py's functions alone."""
    from image_compression_amd import codec
    qs = codec.budget_grid(S_, candidates)
    seen = {q: size_of(q) for q in qs}
    chosen = codec.budget_choice(qs, [seen[q] for q in qs], budget)
    if chosen is None:
        return None, min(seen.values()), sorted(seen)
    for _ in range(rounds - 1):
        nxt = codec.budget_next(seen, chosen)
        qs = [] if nxt is None else codec.budget_refine(chosen, nxt, candidates)
        if not qs:
            break
        seen.update((q, size_of(q)) for q in qs)
        pick = codec.budget_choice(qs, [seen[q] for q in qs], budget)
        chosen = chosen if pick is None else pick
    return chosen, min(size_of(q) for q in codec.budget_grid(S_, candidates)), sorted(seen)


def _monotone(q):
    return 1000 + int(700 * q)


def _bumpy(q):
    """Not monotone: a hump between 1 and 2.5 that is larger than everything up to 4."""
    return 1000 + int(300 * q) + (2500 if 1.0 < q < 2.5 else 0)


def test_choice_on_a_monotone_table():
    for budget in (1000, 1001, 1500, 2399, 2400, 2401, 4499, 4500, 10 ** 6):
        for rounds in (1, 2, 3):
            got = search(_monotone, S, budget, 6, rounds)
            assert got == _by_codec(_monotone, S, budget, 6, rounds)
            q = got[0]
            assert _monotone(q) <= budget
            # monotone: nothing measured above the choice fits
            assert all(_monotone(v) > budget for v in got[2] if v > q)
    q1 = search(_monotone, S, 2399, 6, 1)[0]
    q2 = search(_monotone, S, 2399, 6, 2)[0]
    q3 = search(_monotone, S, 2399, 6, 3)[0]
    assert q1 == 1.0 and q1 < q2 < q3 < 2.0, "each round refines towards the budget"


def test_choice_takes_the_largest_that_fits_past_one_that_fails():
    from image_compression_amd import codec
    qs = codec.budget_grid(S, 6)                      # 0 .. 5
    sizes = [_bumpy(q) for q in qs]                   # 1000 1300 4100 1900 2200 2500
    assert sizes[2] > sizes[4] > sizes[1]
    assert codec.budget_choice(qs, sizes, 2300) == 4.0, "quality 2 fails, 3 and 4 fit: the largest that fits"
    assert codec.budget_choice(qs, sizes, 1300) == 1.0
    got = search(_bumpy, S, 2300, 6, 2)
    assert got == _by_codec(_bumpy, S, 2300, 6, 2)
    assert 4.0 <= got[0] < 5.0 and _bumpy(got[0]) <= 2300
    # the next larger quality is taken among everything measured, so round 3 refines inside round 2's interval
    three = search(_bumpy, S, 2300, 6, 3)
    assert three == _by_codec(_bumpy, S, 2300, 6, 3) and got[0] <= three[0] < 5.0
    assert codec.budget_next({0.0: 1, 2.0: 1, 5.0: 1}, 2.0) == 5.0 and codec.budget_next({0.0: 1, 5.0: 1}, 5.0) is None


def test_choice_bound_is_inclusive_and_the_ends_behave():
    from image_compression_amd import codec
    qs = codec.budget_grid(S, 6)
    sizes = [_monotone(q) for q in qs]
    assert codec.budget_choice(qs, sizes, sizes[3]) == 3.0        # a budget equal to a size
    assert codec.budget_choice(qs, sizes, sizes[3] - 1) == 2.0
    assert codec.budget_choice(qs, sizes, sizes[0] - 1) is None   # no size fits
    assert codec.budget_choice(qs, sizes, sizes[-1]) == 5.0       # everything fits
    none = search(_monotone, S, 999, 6, 3)
    assert none == (None, 1000, qs) == _by_codec(_monotone, S, 999, 6, 3), "no later round after a miss"
    top = search(_monotone, S, 10 ** 6, 6, 3)
    assert top == (5.0, 1000, qs) == _by_codec(_monotone, S, 10 ** 6, 6, 3), "no later round at S - 1"


def test_budget_error_and_stream_bytes():
    from image_compression_amd import codec
    e = codec.BudgetError(2, 1000, 1234)
    assert isinstance(e, ValueError) and (e.image, e.budget, e.smallest) == (2, 1000, 1234)
    assert "1234" in str(e) and "image 2" in str(e)
    h = codec.GainedImageHeader(1, 128, 192, 192, 192, 2, "fp32", 4, 64, 0.11, 256.0, 16, 3, 40, 100, 150, 6, 2.5)
    nz, ny = codec.num_chunks(h.nsym_z, h.R), codec.num_chunks(h.nsym_y, h.R)
    rng = np.random.default_rng(0)
    lz = (256 + 2 * rng.integers(0, 50, nz)).astype(np.uint32)
    ly = (256 + 2 * rng.integers(0, 500, ny)).astype(np.uint32)
    packed = codec.pack_gained_image(h, lz, ly, bytes(int(lz.sum())), bytes(int(ly.sum())))
    assert codec.image_stream_bytes(codec.gained_image_fixed_bytes(h), lz, ly) == len(packed)


# ------------------------------------------------------------------ the ops and the entry points
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype)


def test_rate_ops_have_shape_kernels():
    from image_compression_amd import _lib
    ops = _lib.rate_ops()
    registered = {n.split("::")[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith("imgcomp_rate::")}
    assert registered == {"measure_seg", "gain_symbolize_seg"}
    for nseg, seg_len, R, chunks in ((3, 2 * 256 + 37, 4, 9), (1, 37, 4, 1), (5, 1024, 16, 5)):
        lens = ops.measure_seg(_meta(nseg * seg_len, dtype=torch.int32), nseg, None, 4, _meta(100, dtype=torch.int32), 4,
                               [1] * nseg, [0] * nseg, R)
        assert lens.device.type == "meta" and lens.dtype == torch.int32 and lens.shape == (chunks,)
    with pytest.raises(RuntimeError):
        ops.measure_seg(_meta(10, dtype=torch.int32), 3, None, 4, _meta(100, dtype=torch.int32), 4, [1] * 3, [0] * 3, 4)
    for shape in ((2, 7, 192), (2, 3, 4, 5)):
        y = _meta(*shape)
        sym, kmax = ops.gain_symbolize_seg(y, _meta(5, shape[-1]), _meta(5, *shape[1:]), [0, 1, 1, 0, 1])
        assert sym.device.type == "meta" and sym.dtype == torch.int32 and sym.shape == (5 * y[0].numel(),)
        assert list(kmax) == [0] * 5
    with pytest.raises(RuntimeError):
        ops.gain_symbolize_seg(_meta(2, 7, 192), _meta(4, 192), _meta(5, 7, 192), [0, 1, 1, 0, 1])
    with pytest.raises(RuntimeError):
        ops.gain_symbolize_seg(_meta(2, 7, 192), _meta(5, 192), _meta(4, 7, 192), [0, 1, 1, 0, 1])


def test_library_exports_the_new_symbols():
    from image_compression_amd import _lib
    L = _lib.load()
    assert {"ic_codec_measure_seg", "ic_gain_symbolize_seg"} <= _lib.exported_symbols()
    assert L.ic_version() == 4


def test_entry_points_check_their_arguments_on_the_host():
    """Every refusal below returns before anything is launched: the pointers are null or never dereferenced."""
    from image_compression_amd import _lib
    L = _lib.load()
    ERR = 1001
    p = 256   # a non-null address nothing reads: each call fails an earlier check

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def lls(*v):
        return (ctypes.c_longlong * len(v))(*v)

    K = ints(1, 37, 2047)
    words = [4 * (2 * k + 2) for k in (1, 37, 2047)]
    off = lls(0, words[0], words[0] + words[1])
    pool = sum(words)

    def measure(sym=p, nseg=3, seg_len=256, rows=p, C=0, tab=p, pool_words=pool, nrows=4, k=K, o=off, dev=p, R=4, lens=p):
        return L.ic_codec_measure_seg(sym, nseg, seg_len, rows, C, tab, pool_words, nrows, k, o, dev, R, lens, None)

    for name in ("sym", "tab", "dev", "lens", "k", "o"):
        assert measure(**{name: None}) == ERR, name
    for nseg in (0, -1):
        assert measure(nseg=nseg) == ERR
    assert measure(seg_len=0) == ERR
    for R in (0, 65537):
        assert measure(R=R) == ERR
    assert measure(nrows=0) == ERR
    assert measure(rows=None, C=3, seg_len=256) == ERR          # seg_len % C != 0 with null rows
    assert measure(rows=None, C=0) == ERR
    assert measure(rows=None, C=5, seg_len=255) == ERR          # C > nrows
    assert measure(k=ints(1, 37, 2048)) == ERR                  # a K above the limit
    assert measure(k=ints(1, -1, 2047)) == ERR
    assert measure(pool_words=pool - 1) == ERR                  # the last table leaves the pool
    assert measure(o=lls(0, words[0], pool)) == ERR
    assert measure(o=lls(0, -4, words[0])) == ERR

    img = ints(0, 1, 1, 0, 1)

    def symbolize(y=p, N=2, P=48, C=192, g=p, mu=p, nseg=5, im=img, dev=p, sym=p, kd=p, kh=ints(0, 0, 0, 0, 0)):
        return L.ic_gain_symbolize_seg(y, N, P, C, g, mu, nseg, im, dev, sym, kd, kh, None)

    for name in ("y", "g", "mu", "im", "dev", "sym", "kd", "kh"):
        assert symbolize(**{name: None}) == ERR, name
    for bad in (dict(N=0), dict(N=65536), dict(P=0), dict(C=0), dict(nseg=0), dict(nseg=-2), dict(nseg=65536),
                dict(P=2 ** 62)):
        assert symbolize(**bad) == ERR, bad
    assert symbolize(im=ints(0, 1, 2, 0, 1)) == ERR             # img[m] outside [0, N)
    assert symbolize(im=ints(0, 1, 1, 0, -1)) == ERR


# ------------------------------------------------------------------ compress_each_to in front of any launch
def _cpu_model(arch="GainedMeanScaleCompressor2018", bin_=None):
    from image_compression_amd import modelling
    cfg = cfg_of(arch)
    if bin_ is not None:
        cfg.MODEL.ENTROPY_MODEL.BIN = bin_
    torch.manual_seed(0)
    return modelling.build_model(cfg).eval()


def test_compress_each_to_validates_before_any_launch():
    """A host model and host images: any launch would raise RuntimeError (no device), every refusal here comes first."""
    model = _cpu_model()
    x = torch.rand(3, 3, 72, 100)
    ok = dict(budgets=[5000, 6000, 7000], steps_per_chunk=16, candidates=4, rounds=2)

    def call(xx=x, **kw):
        return model.compress_each_to(xx, **{**ok, **kw})

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
    for bad in (0, 65537, 16.0, None):
        with pytest.raises(ValueError, match="steps_per_chunk"):
            call(steps_per_chunk=bad)
    for shape in ((3, 72, 100), (3, 3, 0, 100)):
        with pytest.raises(ValueError, match="image batch"):
            call(torch.rand(*shape))
    q = model.quality
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        call()
    model.eval()
    assert model.quality == q
    with pytest.raises(RuntimeError, match="ROCm"):      # everything passes: the first launch refuses the host tensor
        call()
    assert model.quality == q and model._gains is None and model._qualities is None


def test_compress_each_to_refuses_the_region_model_and_other_bins():
    x = torch.rand(1, 3, 64, 64)
    region = _cpu_model("RegionGainedMeanScaleCompressor2018")
    with pytest.raises(ValueError, match="quality map"):
        region.compress_each_to(x, 5000)
    with pytest.raises(NotImplementedError, match="BIN"):
        _cpu_model(bin_=2.0).compress_each_to(x, 5000)


def test_wrappers_refuse_host_tensors():
    from image_compression_amd import functional as IF
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.measure_seg(torch.zeros(256, dtype=torch.int32), 1, None, 4, torch.zeros(16, dtype=torch.int32), 4, [1], [0], 4)
    with pytest.raises(RuntimeError, match="ROCm"):
        IF.gain_symbolize_seg(torch.zeros(2, 4, 3, 3), torch.ones(5, 4), torch.zeros(5, 4, 3, 3), [0, 1, 1, 0, 1])
