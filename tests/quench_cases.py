"""The graphs and starts the GPU quench tests share (tests/test_quench_gpu.py,
tests/test_quench_restarts_gpu.py, tests/test_quench_regions_gpu.py).  Plain
module, imported like tests/quench_oracle.py."""
import functools

import numpy as np

import quench_oracle as qo

R_CASE = 128
# name -> (graph kind, degree / mean degree, n, T, m_init, graph seed, start seed)
CASES = {
    "rrg_d4_n200_T1": ("rrg", 4, 200, 1, 0.9, 1, 11),
    "rrg_d3_n200_T2": ("rrg", 3, 200, 2, 0.8, 2, 12),
    "rrg_d4_n96_T3": ("rrg", 4, 96, 3, 0.45, 3, 13),
    "rrg_d5_n120_T2": ("rrg", 5, 120, 2, 0.5, 4, 14),
    "rrg_d3_n130_T4": ("rrg", 3, 130, 4, 0.6, 5, 15),
    "er_n300_deg3_T2": ("er", 3.0, 300, 2, 0.9, 6, 16),
    "er_n300_deg5_T3": ("er", 5.0, 300, 3, 0.7, 7, 17),
    "rrg_d3_n64_T6": ("rrg", 3, 64, 6, 0.55, 8, 18),
}
TABLE = [k for k in CASES if k != "rrg_d3_n64_T6"]
# graphs much larger than a 2T-ball: several candidates commit per round ("er+iso": isolated nodes kept,
# so there are disconnected components)
PARALLEL = {
    "rrg_d4_n600_T1": ("rrg", 4, 600, 1, 0.9, 21, 31),
    "rrg_d3_n1500_T2": ("rrg", 3, 1500, 2, 0.93, 22, 32),
    "ring_n256_T3": ("ring", 2, 256, 3, 0.9, 0, 33),
    "er_n600_deg3_T2": ("er+iso", 3.0, 600, 2, 0.95, 24, 34),
}
# name -> nodes joined to the hub: "hub80" has a row longer than a wave's 64 lanes
HUBS = {"hub": 60, "hub80": 80}


def hub_graph(seed=9, more=60):
    """ER graph of n = 300 (mean degree 3, isolated nodes kept) with node 0
    joined to ``more`` further nodes, among them every isolated node but the
    last: one long row and one node of degree 0."""
    import mjx
    n = 300
    u, v = mjx.erdos_renyi_edges(n, 3.0 / (n - 1), seed=seed)
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    iso = np.flatnonzero(deg == 0)
    iso = iso[iso != 0]
    assert iso.size >= 1
    lone = int(iso[-1])
    nb0 = set(v[u == 0].tolist()) | set(u[v == 0].tolist()) | {0, lone}
    others = [k for k in range(n) if k not in nb0 and k not in set(iso.tolist())]
    extra = np.array(iso[:-1].tolist() + others[:more - (iso.size - 1)], dtype=np.int64)
    assert extra.size == more
    rp, col = mjx.csr_from_edges(n, np.concatenate([u, np.zeros(more, np.int64)]), np.concatenate([v, extra]))
    d = np.diff(rp)
    assert d[lone] == 0 and (d == 0).sum() == 1 and d[0] >= more
    return rp, col, lone


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (graph as the package takes it, oracle step, S (R_CASE, n), T).  Shared: never written."""
    import mjx
    if name in HUBS:
        rp, col, _ = hub_graph(more=HUBS[name])
        return ("csr", rp, col), qo.step_csr(rp, col), qo.random_starts(R_CASE, 300, 0.9, seed=19), 3
    kind, d, n, T, m_init, gseed, sseed = {**CASES, **PARALLEL}[name]
    if kind == "rrg":
        adj = mjx.random_regular_graph(d, n, seed=gseed)
        return ("ell", adj), qo.step_ell(adj), qo.random_starts(R_CASE, n, m_init, sseed), T
    if kind == "ring":
        adj = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1).astype(np.int32)
        return ("ell", adj), qo.step_ell(adj), qo.random_starts(R_CASE, n, m_init, sseed), T
    if kind == "er+iso":
        u, v = mjx.erdos_renyi_edges(n, d / (n - 1), seed=gseed)
        rp, col = mjx.csr_from_edges(n, u, v)
        assert (np.diff(rp) == 0).sum() >= 2
        return ("csr", rp, col), qo.step_csr(rp, col), qo.random_starts(R_CASE, n, m_init, sseed), T
    rp, col, _ = mjx.erdos_renyi(n, d / (n - 1), seed=gseed, drop_isolated=True)
    return ("csr", rp, col), qo.step_csr(rp, col), qo.random_starts(R_CASE, rp.shape[0] - 1, m_init, sseed), T


@functools.lru_cache(maxsize=None)
def _graph(name):
    import mjx
    spec = _case(name)[0]
    return mjx.Graph.ell(spec[1]) if spec[0] == "ell" else mjx.Graph.csr(spec[1], spec[2])
