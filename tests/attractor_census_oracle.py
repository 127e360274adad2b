"""ORACLE (test infrastructure only, numpy): the attractor census by brute
force.  Every configuration x in [0, 2^n) -- node v is +1 iff bit v of x is
set -- is run through attractor_oracle.attractor, 2^16 rows at a time, and
binned by (class, p, k):

    class 0 plus   c = 1 and s(p) is all +1      2 fixed  c = 1, neither
          1 minus  c = 1 and s(p) is all -1      3 cycle  c = 2
    hist[class, p, k], unsettled[k] (p > t_max), k = popcount(x)
    lightest_plus = the smallest (k, x) over class plus, as k << 48 | x
    longest       = the largest (p, x) over the settled x, as p << 48 | x (0 when
                    nothing has settled: the key of all -1 in block 0)
"""
import numpy as np

import attractor_oracle as ao
import census_oracle as co

CHUNK = 1 << 16
CLASSES = ("plus", "minus", "fixed", "cycle")
step_ell, step_csr, configs = co.step_ell, co.step_csr, co.configs


def bin_rows(step, S, x, n, t_max, out=None):
    """Bin the rows S (R, n) with configuration indices x (R,) into ``out`` (a
    new result when None) -> out: dict hist, unsettled, lightest_plus, longest."""
    if out is None:
        out = {"hist": np.zeros((4, t_max + 1, n + 1), np.int64), "unsettled": np.zeros(n + 1, np.int64),
               "lightest_plus": None, "longest": 0}
    x = np.asarray(x, dtype=np.int64)
    k = (S == 1).sum(axis=1)
    res = ao.attractor(step, S, t_max=t_max)
    p, c, s0 = res["p"], res["c"], res["sum_att"][:, 0]
    done = p >= 0
    cls = np.where(c == 2, 3, np.where(s0 == n, 0, np.where(s0 == -n, 1, 2)))
    np.add.at(out["hist"], (cls[done], p[done], k[done]), 1)
    out["unsettled"] += np.bincount(k[~done], minlength=n + 1)
    plus = done & (cls == 0)
    if plus.any():
        key = int(((k[plus] << 48) | x[plus]).min())
        out["lightest_plus"] = key if out["lightest_plus"] is None else min(out["lightest_plus"], key)
    if done.any():
        out["longest"] = max(out["longest"], int(((p[done] << 48) | x[done]).max()))
    return out


def attractor_census(step, n, t_max):
    """All 2^n configurations -> dict hist int64 (4, t_max+1, n+1), unsettled
    int64 (n+1,), lightest_plus and longest (ints)."""
    out = None
    for lo in range(0, 1 << n, CHUNK):
        hi = min(1 << n, lo + CHUNK)
        out = bin_rows(step, configs(lo, hi, n), np.arange(lo, hi), n, t_max, out)
    assert out["lightest_plus"] is not None, "all +1 is a fixed point"
    return out


def derived(res, n):
    """The values ``attractor_census`` derives from the oracle's bins and keys."""
    kp, kl = res["lightest_plus"], res["longest"]
    low = (1 << 48) - 1
    return {"reach_plus": np.cumsum(res["hist"][0], axis=0), "min_plus_ever": kp >> 48,
            "witness_plus": co.spins(kp & low, n).astype(np.int8), "p_longest": kl >> 48,
            "witness_longest": co.spins(kl & low, n).astype(np.int8)}
