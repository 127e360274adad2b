"""ORACLE (test infrastructure only, numpy): the consensus census by brute
force.  Every configuration x in [0, 2^n) -- node v is +1 iff bit v of x is
set -- is stepped with oracle.majority's one-step rules, 2^16 rows at a time.

    counts[t, k] = #{x : popcount(x) = k and onestep^t(x) is all +1}, t = 0..T
    min_plus[t]  = the smallest k with counts[t, k] > 0
    witness[t]   = the x with the smallest (popcount(x), x) counted in counts[t]
"""
import numpy as np

from oracle import majority as orc

CHUNK = 1 << 16


def step_ell(adj):
    adj = np.asarray(adj, dtype=np.int64)
    if adj.shape[1] == 0:
        return lambda S: S
    return lambda S: orc.onestep_majority_batch(adj, S)


def step_csr(row_ptr, col):
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    return lambda S: orc.onestep_majority_er(row_ptr, col, S)


def configs(lo, hi, n):
    """Rows x = lo .. hi-1 as +-1 spins (hi - lo, n)."""
    x = np.arange(lo, hi, dtype=np.uint64)
    bits = (x[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)
    return 2 * bits.astype(np.int64) - 1


def spins(x, n):
    """Configuration index -> +-1 spins [n]."""
    return configs(int(x), int(x) + 1, n)[0]


def census(step, n, T):
    """-> dict counts int64 (T+1, n+1), min_plus int64 (T+1,), witness_x int64
    (T+1,) and witness int8 (T+1, n)."""
    counts = np.zeros((T + 1, n + 1), np.int64)
    best = [None] * (T + 1)                                  # (k, x)
    total = 1 << n
    for lo in range(0, total, CHUNK):
        hi = min(total, lo + CHUNK)
        S = configs(lo, hi, n)
        k = (S == 1).sum(axis=1)
        for t in range(T + 1):
            if t:
                S = step(S)
            hit = np.flatnonzero((S == 1).all(axis=1))
            if hit.size == 0:
                continue
            counts[t] += np.bincount(k[hit], minlength=n + 1)
            kmin = int(k[hit].min())
            cand = (kmin, lo + int(hit[k[hit] == kmin][0]))   # hit is ascending in x
            if best[t] is None or cand < best[t]:
                best[t] = cand
    assert all(b is not None for b in best), "all +1 is counted at every level"
    wx = np.array([b[1] for b in best], np.int64)
    return {"counts": counts, "min_plus": np.array([b[0] for b in best], np.int64), "witness_x": wx,
            "witness": np.stack([spins(x, n) for x in wx]).astype(np.int8)}
