"""The built graphs, the LDS-budget formula and the oracle loop that the ER-HPR
edge tests share (tests/test_hpr_er_edges_gpu.py on the device,
tests/test_hpr_er_cases.py for the host side).  Plain module, imported like
tests/quench_cases.py.  Everything here runs without a GPU except ``plan``."""
import functools

import numpy as np
import torch

from oracle import hpr as orc
from oracle import majority as om

K_MAX_LDS = 160 * 1024                   # kMaxLds of csrc/mjx_hpr_er.hip
SIZEOF = {torch.float32: 8, torch.float64: 8}      # of a table entry: double for float messages too

# name -> (core nodes, core mean degree, seed, hub degrees, classes D present)
# A hub of degree g is one extra node joined to g core nodes: its g messages are class D = g - 1.  A leaf is
# joined to core node 0, so class 0 is there by construction.  The class set is recorded, not searched for:
# ``built`` asserts it.
GRAPHS = {
    "slab_t4": (60, 2.5, 1, (11,), (0, 1, 2, 3, 4, 5, 10)),      # D = 10: slab at T = 4
    "slab_t3": (60, 2.5, 2, (22,), (0, 1, 2, 3, 4, 5, 6, 7, 21)),      # D = 21: slab at T = 3
    "edge_t4": (60, 2.5, 3, (7, 8), (0, 1, 2, 3, 4, 5, 6, 7)),         # D = 6 | 7: the LDS boundary at T = 4
    "more_t4": (60, 2.5, 4, (8, 9, 10), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)),
    "edge_t3": (60, 2.5, 5, (17, 18), (0, 1, 2, 3, 4, 5, 7, 16, 17)),  # D = 16 | 17: the boundary at T = 3
    "more_t3": (60, 2.5, 6, (21, 22), (0, 1, 2, 3, 4, 5, 20, 21)),
    "loop_a": (80, 2.5, 7, (), (0, 1, 2, 3, 4, 6)),
    "loop_hub": (80, 2.5, 8, (9,), (0, 1, 2, 3, 4, 5, 8)),      # D = 8: an LDS class at T <= 3
    "star40": (60, 2.5, 9, (40,), (0, 1, 2, 3, 4, 5, 39)),
}


# D = 0 only: a single edge; D = 0 and D = 1: a path of three nodes
SMALL = {"edge2": (2, ((0, 1),)), "path3": (3, ((0, 1), (1, 2)))}


class Built:
    """One built graph on the host: edge list (row order of the messages),
    CSR, the oracle's classes, the hub and leaf nodes."""

    def __init__(self, edges, rp, col, hubs, leaf):
        self.edges, self.rp, self.col, self.hubs, self.leaf = edges, rp, col, hubs, leaf
        self.n, self.E = rp.size - 1, edges.shape[0]
        self.deg = np.diff(rp)
        self.classes, self.src, self.out_rows = orc.er_classes(edges, rp, col)
        self.class_set = tuple(D for D, _, _ in self.classes)

    def rows_of(self, D):
        return next(rows for d, rows, _ in self.classes if d == D)


def _csr(n, pairs):
    u = np.array([a for a, _ in pairs], dtype=np.int64)
    v = np.array([b for _, b in pairs], dtype=np.int64)
    src, dst = np.concatenate([u, v]), np.concatenate([v, u])
    order = np.lexsort((dst, src))
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rp[1:])
    return np.stack([u, v], axis=1), rp, dst[order]


def from_pairs(n, pairs):
    """A graph written out edge by edge (the single edge, the path)."""
    return Built(*_csr(n, sorted(pairs)), (), None)


@functools.lru_cache(maxsize=None)
def built(name):
    """Deterministic: G(n, mean / (n - 1)) from numpy's generator at the
    recorded seed with its isolated nodes dropped, then one leaf on core node
    0, then every hub as a new node joined to core nodes drawn without
    replacement.  Shared: never written."""
    if name in SMALL:
        return from_pairs(*SMALL[name])
    n0, mean, seed, hub_degs, want = GRAPHS[name]
    rng = np.random.default_rng(seed)
    iu, iv = np.triu_indices(n0, k=1)
    keep = rng.random(iu.size) < mean / (n0 - 1)
    iu, iv = iu[keep], iv[keep]
    used = np.zeros(n0, dtype=bool)
    used[iu] = used[iv] = True
    new_id = np.cumsum(used) - 1
    n = int(used.sum())
    pairs = set(zip(new_id[iu].tolist(), new_id[iv].tolist()))
    ncore = n
    leaf = n
    pairs.add((0, leaf))
    n += 1
    hubs = []
    for g in hub_degs:
        for k in rng.choice(ncore, size=g, replace=False).tolist():
            pairs.add((int(k), n))
        hubs.append(n)
        n += 1
    G = Built(*_csr(n, sorted(pairs)), tuple(hubs), leaf)
    assert G.deg[leaf] == 1 and 0 in G.class_set
    for h, g in zip(hubs, hub_degs):
        assert G.deg[h] == g and G.rows_of(g - 1).size >= g
        assert h in G.src[G.rows_of(g - 1)]
    assert G.class_set == want, (name, G.class_set)
    return G


def plan(mjx, G):
    """The device plan of a built graph (a fresh one: tests patch SCRATCH_CAP)."""
    pl = mjx.HPRERPlan(G.edges, G.rp, G.col)
    assert np.array_equal(pl.out_rows_host, G.out_rows)
    for (D, rows, inc), (Dd, rows_d, inc_d, _, m) in zip(G.classes, pl.classes):
        assert D == Dd and m == rows.size
    return pl


# ---- the LDS budget, written out (csrc/mjx_hpr_er.hip: tab_bytes, m_bytes, lds_bytes) ----
def table_bytes(dtype, D, T):
    return (2 ** T // 2) * (D + 1) ** T * SIZEOF[dtype]


def incoming_bytes(dtype, D, T):
    return D * (2 ** T // 2) * 2 ** T * SIZEOF[dtype]


def scratch_bytes(dtype, D, T):
    """What mjx_hpr_er_scratch_bytes must return: 0 for a class whose table and
    incoming messages fit the 160 KiB of LDS, else the bytes of one table."""
    if D > 255 or T > 4 or (D + 1) ** T > 1 << 22 or incoming_bytes(dtype, D, T) > K_MAX_LDS:
        return -1
    return 0 if table_bytes(dtype, D, T) + incoming_bytes(dtype, D, T) <= K_MAX_LDS else table_bytes(dtype, D, T)


# T -> (graph, last LDS class, first slab class), the same for float and double messages since the table
# is double for both; and further slab classes that float runs (their tables would be 4-byte sized
# 209 952 .. 320 000 B at T = 4, 148 176 / 170 368 B at T = 3, were the table float)
BOUNDARY = {4: ("edge_t4", 6, 7), 3: ("edge_t3", 16, 17)}
MORE_SLAB = {4: ("more_t4", (8, 9)), 3: ("more_t3", (20, 21))}
SPLITS = {4: [(1, 3), (2, 2), (3, 1)], 3: [(1, 2), (2, 1)]}


# ---- one oracle step, shared ----
def random_state(G, p, c, seed):
    rng = np.random.default_rng(seed)
    chi = rng.random((2 * G.E, 4 ** (p + c)))
    chi /= chi.sum(1, keepdims=True)
    b = rng.random((G.n, 2))
    b /= b.sum(1, keepdims=True)
    return chi, b


@functools.lru_cache(maxsize=None)
def oracle_step(name, p, c, attr, seed=0):
    """-> (chi0, biases0, chi1, marginals of chi1) of built(name), float64.  Shared: never written."""
    G = built(name)
    chi, b = random_state(G, p, c, seed)
    new = orc.HPr_dp_er(chi, b, G.classes, G.src, G.n, p, c, attr, 25 * G.n, 0.4)
    marg = orc.marginals_comp_csr(new, G.rp, G.out_rows, p, c)
    for a in (chi, b, new, marg):
        a.setflags(write=False)
    return chi, b, new, marg


# ---- the loop of hpr_er_run, from the oracle's parts ----
def initial_state(G, p, c, seed):
    """chi0, biases0 and the generator after them, as hpr_er_run draws."""
    gen = torch.Generator().manual_seed(seed)
    chi0 = torch.rand((2 * G.E, 4 ** (p + c)), dtype=torch.float64, generator=gen)
    chi0 = chi0 / torch.sum(chi0, axis=1, keepdims=True)
    b0 = torch.rand((G.n, 2), dtype=torch.float64, generator=gen)
    b0 = b0 / torch.sum(b0, axis=1, keepdims=True)
    return chi0, b0, gen


@functools.lru_cache(maxsize=None)
def oracle_loop(name, p, c, TT, seed, lmbd_per_n=25, damp=0.4, pie=0.3, gamma=0.1):
    """HPr_dp_er -> marginals_comp_csr -> new_biases_i until the ER majority
    dynamics of s reach consensus or t > TT, on torch's CPU stream.  Records s
    and the smallest relative margin |m+ - m-| / (m+ + m-) of every iteration."""
    G = built(name)
    chi0, b0, gen = initial_state(G, p, c, seed)
    chi, b = chi0.numpy(), b0.numpy()
    s = np.where(b[:, 0] > b[:, 1], 1, -1).astype(np.int32)
    m = np.sum(om.s_endstate_er(G.rp, G.col, s, p, c)) / G.n
    t, S, margins = 0, [], []
    while m < 1:
        chi = orc.HPr_dp_er(chi, b, G.classes, G.src, G.n, p, c, 1, lmbd_per_n * G.n, damp)
        marg = orc.marginals_comp_csr(chi, G.rp, G.out_rows, p, c)
        margins.append(float(np.min(np.abs(marg[:, 0] - marg[:, 1]) / (marg[:, 0] + marg[:, 1]))))
        u = torch.rand(G.n, dtype=torch.float64, generator=gen).numpy()
        b, s = orc.new_biases_i(b, pie, gamma, marg, t, u)
        S.append(s.copy())
        t += 1
        m = 2 if t > TT else np.sum(om.s_endstate_er(G.rp, G.col, s, p, c)) / G.n
    low = [i for i, x in enumerate(margins) if x < 1e-4]
    return {"num_steps": t, "conf": s.astype(np.float64), "mag_reached": float(np.sum(s) / G.n), "s": S,
            "margins": margins, "first_low": low[0] if low else None, "consensus": bool(m == 1),
            "next_rand": torch.rand(4, dtype=torch.float64, generator=gen)}


# (graph, p, c, TT, torch seed, lmbd / n) -> what oracle_loop records: num_steps, stopped by consensus, first
# iteration with a relative margin below 1e-4 (None: never), smallest margin of the run.  The seeds were
# chosen from the oracle alone, so that no float64 decision comes within 1e-9 of a tie and float32 has at
# least 20 iterations above 1e-4.  (At lmbd = 25 n the (2, 1) and (1, 2) runs on these graphs meet an exact
# tie near iteration 59, once the messages saturate; they therefore use a smaller lmbd.)
LOOPS = {
    ("loop_a", 1, 1, 60, 0, 25): (61, False, None, 8.030e-04),       # hpr_er_run's default lmbd: stops at the cap
    ("loop_a", 2, 1, 60, 0, 8): (42, True, None, 4.901e-03),
    ("loop_a", 2, 1, 60, 0, 3): (36, True, 27, 1.071e-06),            # float32 is compared on iterations 0..26
    ("loop_hub", 1, 2, 60, 0, 3): (26, True, None, 4.044e-03),        # a leaf and a hub in class 8 (LDS)
    ("loop_hub", 2, 1, 60, 1, 8): (61, False, None, 1.976e-03),
}


def check_loop(key):
    """-> (the oracle loop of LOOPS[key] with its recorded figures asserted,
    the number of iterations float32 is compared on)."""
    steps, consensus, first_low, min_margin = LOOPS[key]
    ref = oracle_loop(*key)
    assert (ref["num_steps"], ref["consensus"], ref["first_low"]) == (steps, consensus, first_low), key
    assert abs(min(ref["margins"]) - min_margin) <= 1e-3 * min_margin and min_margin >= 1e-9, key
    assert steps == key[3] + 1 or consensus
    upto32 = steps if first_low is None else first_low
    assert upto32 >= 20
    return ref, upto32
