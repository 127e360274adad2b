"""ORACLE (test infrastructure only, numpy): the minimal consensus sets by
brute force.  U_t[x] says that configuration x -- node v is +1 iff bit v of x
is set -- is all +1 after t steps (census_oracle's rows and step functions);

    M_t      = U_t & ~OR_i(bit i of x set & U_t[x ^ bit i])
    minima   = M_t counted by popcount(x), int64 (T+1, n+1)
    heaviest = the x of M_t with the largest (popcount(x), x)
"""
import numpy as np

import census_oracle as co


def reach(step, n, T):
    """-> bool (T+1, 2^n): U_t[x]."""
    total = 1 << n
    U = np.zeros((T + 1, total), bool)
    for lo in range(0, total, co.CHUNK):
        hi = min(total, lo + co.CHUNK)
        S = co.configs(lo, hi, n)
        for t in range(T + 1):
            if t:
                S = step(S)
            U[t, lo:hi] = (S == 1).all(axis=1)
    return U


def minimal(U, n):
    """-> bool, the shape of U: the members no single +1 node can be dropped from."""
    x = np.arange(1 << n, dtype=np.int64)
    drop = np.zeros_like(U)
    for i in range(n):
        drop |= ((x >> i) & 1).astype(bool)[None, :] & U[:, x ^ (1 << i)]
    return U & ~drop


def weights(n):
    x = np.arange(1 << n, dtype=np.uint64)
    return sum(((x >> np.uint64(i)) & np.uint64(1)).astype(np.int64) for i in range(n))


def census_of(U, n):
    """The census of the minima of any (L, 2^n) bool array of up-sets -> dict minima int64 (L, n+1),
    max_plus and heaviest_x int64 (L,) (-1 where a level is empty), and M itself."""
    M = minimal(U, n)
    k = weights(n)
    minima = np.stack([np.bincount(k[row], minlength=n + 1) for row in M]).astype(np.int64)
    max_plus, heavy = [], []
    for row in M:
        hit = np.flatnonzero(row)
        if hit.size == 0:
            max_plus.append(-1), heavy.append(-1)
            continue
        kmax = int(k[hit].max())
        max_plus.append(kmax), heavy.append(int(hit[k[hit] == kmax][-1]))      # hit is ascending in x
    return {"minima": minima, "max_plus": np.array(max_plus, np.int64), "heaviest_x": np.array(heavy, np.int64),
            "M": M}


def census_minima(step, n, T):
    """-> census_of(U) with U, and the census of the levels (census_oracle.census's keys) from the same U."""
    U = reach(step, n, T)
    res = census_of(U, n)
    k = weights(n)
    res["U"] = U
    res["counts"] = np.stack([np.bincount(k[row], minlength=n + 1) for row in U]).astype(np.int64)
    res["witness_max"] = np.stack([co.spins(x, n) for x in res["heaviest_x"]]).astype(np.int8)
    return res


def words(U, n):
    """The bitmap of the ABI: bool (L, 2^n) -> uint64 (L, B), bit j of word b is configuration 64 b + j."""
    L = U.shape[0]
    if n < 6:
        U = np.concatenate([U, np.zeros((L, 64 - (1 << n)), bool)], axis=1)
    bits = U.reshape(L, -1, 64).astype(np.uint64)
    return (bits << np.arange(64, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)
