"""Operands that tell a product rounded before a difference from the two contracted into one FMA (pure numpy).  The GPU
tests of the symbolizers that scale and then subtract a mean plant them: tests/test_budget_gpu.py and
tests/test_transcode_gpu.py."""
import numpy as np


def _fusable(b, count, seed):
    """(y_hat, mu2) float32[count] for the gain b, no power of two: fl(y_hat b) - mu2 rounds to k + 0.5 while
    fma(y_hat, b, -mu2), the unrounded product minus mu2, rounds to a neighbour of k + 0.5.  With e the product's
    rounding error and u the spacing at k + 0.5, mu2 = fl(y_hat b) - (k + 0.5) - d with d = sign(e) (u - |e|) / 2: then
    |d| < u / 2 and |e + d| > u / 2.  One bounded draw; every pair is verified below."""
    rng = np.random.default_rng(seed)
    b = np.float32(b)
    y = rng.uniform(16.0 / b, 32.0 / b, 200000).astype(np.float32)
    prod = y * b                                               # fp32, in [16, 32): the spacing is 2^-19
    exact = y.astype(np.float64) * np.float64(b)               # 24 x 24 bits: exact in fp64
    e = exact - prod.astype(np.float64)
    tie = np.floor(prod) + np.float32(0.5)
    d = np.sign(e) * (2.0 ** -20 - np.abs(e) / 2)
    mu = (prod.astype(np.float64) - tie.astype(np.float64) - d).astype(np.float32)
    plain = prod - mu
    fused = (exact - mu.astype(np.float64)).astype(np.float32)
    ok = (prod >= 16) & (prod < 32) & (np.abs(prod - tie) < 2.0 ** -6) & (np.abs(e) > 2.0 ** -23)
    ok &= (plain == tie) & (np.rint(fused) != np.rint(plain))
    pick = np.flatnonzero(ok)[:count]
    assert len(pick) == count, f"only {len(pick)} of {count} values planted"
    return y[pick], mu[pick]
