"""ORACLE (test infrastructure only, numpy): the census marginals by brute
force, on top of census_oracle's rows and step functions.  With x running over
all 2^n configurations (node v is +1 iff bit v of x is set):

    node_counts[t, k, v] = #{x : popcount(x) = k, bit v of x set, onestep^t(x) all +1}

-- the configurations census_oracle.census counts in counts[t, k], summed over
their rows -- and the Boltzmann averages of one level by a direct sum over the
configurations, without any log-sum-exp.
"""
import numpy as np

import census_oracle as co


def node_counts(step, n, T):
    """-> int64 (T+1, n+1, n), every level."""
    out = np.zeros((T + 1, n + 1, n), np.int64)
    total = 1 << n
    for lo in range(0, total, co.CHUNK):
        S = co.configs(lo, min(total, lo + co.CHUNK), n)
        up = (S == 1).astype(np.int64)                       # the start rows: S is stepped below
        k = up.sum(axis=1)
        for t in range(T + 1):
            if t:
                S = step(S)
            hit = np.flatnonzero((S == 1).all(axis=1))
            np.add.at(out[t], k[hit], up[hit])
    return out


def census(step, n, T):
    """census_oracle.census's dict and ``node_counts``, ``optimal`` int64 (T+1,), ``backbone_plus`` and
    ``backbone_minus`` bool (T+1, n), every level."""
    res = co.census(step, n, T)
    nc = node_counts(step, n, T)
    t = np.arange(T + 1)
    optimal = res["counts"][t, res["min_plus"]]
    at_best = nc[t, res["min_plus"]]
    res.update(node_counts=nc, optimal=optimal, backbone_plus=at_best == optimal[:, None], backbone_minus=at_best == 0)
    return res


def boltzmann_direct(step, n, t, lam):
    """phi, m_init and p_plus (n,) of level t at one lambda by a sum over all 2^n configurations with the
    weight exp(-lam sum_v s_v(0)); n small, lam moderate (no rescaling)."""
    S0 = co.configs(0, 1 << n, n)
    S = S0
    for _ in range(t):
        S = step(S)
    hit = (S == 1).all(axis=1)
    s0 = S0[hit]
    w = np.exp(-lam * s0.sum(axis=1).astype(np.float64))
    Z = w.sum()
    return {"phi": np.log(Z) / n, "m_init": (w * s0.sum(axis=1)).sum() / Z / n,
            "p_plus": (w[:, None] * (s0 == 1)).sum(axis=0) / Z}


def recursive_tree(n, seed):
    """A random recursive tree: the parent of v = 1..n-1 is drawn from 0..v-1 with default_rng(seed).
    -> (edges (n-1, 2) as (parent, v), row_ptr, col with sorted rows)."""
    rng = np.random.default_rng(seed)
    edges = np.array([(int(rng.integers(0, v)), v) for v in range(1, n)], dtype=np.int64)
    return (edges,) + csr_of(n, edges)


def csr_of(n, edges):
    """-> (row_ptr int64, col int64) of an edge list, both directions, rows sorted."""
    rows = [[] for _ in range(n)]
    for u, v in np.asarray(edges).tolist():
        rows[u].append(v)
        rows[v].append(u)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rp, np.array([u for r in rows for u in sorted(r)], dtype=np.int64)
