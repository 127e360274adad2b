"""Shared cases of the BDCM edge tests (host only, numpy): forests whose degree
classes are chosen one by one, the spin-flip map on message arrays, a per-entry
error measure, and the oracle's side of the leaf reset and the sweeps that the
CPU and the GPU tests both compare against.

Hub degree lists.  The kernels of csrc/mjx_bdcm.hip choose three things per
degree class D (edge class D = k - 1, node class D = k of a hub of degree k),
with XV = 2^(T-1) valid trajectories and a count table of S = (D+1)^T entries
per trajectory:

  item_threads   64 while XV*S <= 128, 128 while XV*S <= 512, else 256
      T = 1: D+1 <= 128            -> 64 | 128 at D = 127 | 128 (512 lies past the class limit 255)
      T = 2: 2(D+1)^2 <= 128, 512  -> D = 7 | 8 and 15 | 16
      T = 3: 4(D+1)^3 <= 128, 512  -> D = 2 | 3 and 4 | 5
      T = 4: 8(D+1)^4 <= 128, 512  -> D = 1 | 2 for both (16 entries per trajectory, then 81)
  src_tab        on for D > 1 while src_bytes = XV*S*(XV+1)*4 <= kSrcTabMax = 32 KiB
      T = 2: 24(D+1)^2 <= 32768    -> D = 35 | 36
      T = 3: 80(D+1)^3 <= 32768    -> D = 6 | 7
      T = 4: 288(D+1)^4 <= 32768   -> D = 2 | 3
      T = 1: 8(D+1) never reaches it; what moves instead is the number of
             chunks of the top-down convolution: one (partial) chunk of the
             64-wide workgroup up to D = 63, two from D = 64
  LDS or slab    LDS while tab_bytes + m_bytes = 8*XV*S + 8*D*XV^2 <= kMaxLds = 160 KiB
      T = 3: 32(D+1)^3 + 128 D     -> D = 16 | 17   (159264 | 188800)
      T = 4: 64(D+1)^4 + 512 D     -> D = 6 | 7     (156736 | 265728)
      T = 2: 16(D+1)^2 + 32 D      -> D = 99 | 100, left out: the numpy oracle
             needs about 100 s there, and T = 3 and T = 4 run the slab path
  class limit    D <= 255 (T = 1 reaches it: edge class 254, node class 255)

Every list holds k = D and k = D + 1 (node class) and k = D + 1 and D + 2
(edge class) for each boundary "D | D + 1" above, so both kernels run on both
sides of it.  A constant that moves in the source moves the matching entries.
"""
import functools

import numpy as np

from oracle import bdcm as orc

HUB_DEGREES = {
    1: (2, 3, 63, 64, 65, 127, 128, 129, 255),
    2: (2, 3, 7, 8, 9, 15, 16, 17, 35, 36, 37),
    3: (2, 3, 4, 5, 6, 7, 8, 16, 17, 18),
    4: (2, 3, 4, 6, 7, 8),
}
# last D whose count table still lives in LDS (asserted against the library on the GPU)
LDS_LAST_D = {3: 16, 4: 6}
PC_ALL = [(p, T - p) for T in (1, 2, 3, 4) for p in range(T)]      # the ten (p, c) with p + c <= 4


def hub_forest(degrees, seed=None):
    """A path of hubs with the listed degrees (hub i adjacent to hub i + 1),
    every other neighbour of a hub a leaf: edge classes {0} and {k - 1}, node
    classes {1} and {k}, nothing else.  Nodes 0..H-1 are the hubs.  Returns
    (n, edges (E, 2), row_ptr, col); ``seed``: every CSR row is permuted with
    default_rng(seed)."""
    degrees = [int(k) for k in degrees]
    H = len(degrees)
    edges, nbrs = [], [[] for _ in range(H)]
    n = H
    for i, k in enumerate(degrees):
        hubs = (i > 0) + (i < H - 1)
        if k < max(hubs, 1):
            raise ValueError(f"hub {i} of degree {k} has {hubs} hub neighbours")
        if i > 0:
            nbrs[i].append(i - 1)
        if i < H - 1:
            edges.append((i, i + 1))
            nbrs[i].append(i + 1)
        for _ in range(k - hubs):
            edges.append((i, n))
            nbrs[i].append(n)
            nbrs.append([i])
            n += 1
    if seed is not None:
        rng = np.random.default_rng(seed)
        nbrs = [list(rng.permutation(x)) for x in nbrs]
    row_ptr = np.concatenate([[0], np.cumsum([len(x) for x in nbrs])]).astype(np.int64)
    return n, np.array(edges, dtype=np.int64).reshape(-1, 2), row_ptr, np.concatenate(nbrs).astype(np.int64)


def reverse_rows(row_ptr, col):
    """The same CSR with every neighbour list reversed."""
    return np.concatenate([col[row_ptr[i]:row_ptr[i + 1]][::-1] for i in range(row_ptr.size - 1)])


def flip(chi, T):
    """The global spin flip on a message array (rows, 4^T): the index
    complement x -> 2^T - 1 - x on both trajectory axes."""
    X = 2 ** T
    chi = np.asarray(chi)
    return np.ascontiguousarray(chi.reshape(-1, X, X)[:, ::-1, ::-1]).reshape(chi.shape)


def entry_err(got, want):
    """Largest |got - want| / |want| over the non-zero entries; the exact zeros
    must be the same set on both sides, and a NaN anywhere fails."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert not np.isnan(got).any() and not np.isnan(want).any(), "NaN"
    assert np.array_equal(got == 0, want == 0), "the exact zeros differ"
    nz = want != 0
    if not nz.any():
        return 0.0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))


def random_chi(rows, T, seed):
    chi = np.random.default_rng(seed).random((rows, 4 ** T))
    return chi / chi.sum(axis=1, keepdims=True)


def oracle_leaf_and_sweeps(hp, chi0, p, c, attr_value, lmbd, epsilon):
    """What the edge tests run, on the oracle: the leaf reset, one assigning
    sweep (damppar = 1, so the exact-zero sectors show), one damped sweep
    (damppar = 0.3), and one assigning sweep of chi0 as it is -- without the
    leaf reset every message into a hub's table is a different one, where
    after it all leaves send the same.  Returns the four message arrays
    (leaf, sweep, damped sweep, raw sweep)."""
    leaf = np.array(chi0, dtype=np.float64, copy=True)
    if 0 in hp.class_rows:
        leaf[hp.class_rows[0]] = orc.leaf_message(p, c, attr_value, lmbd)[None, :]
    s1 = orc.BDCM_ER(leaf, hp, p, c, attr_value, lmbd, 1.0, epsilon)
    s2 = orc.BDCM_ER(s1, hp, p, c, attr_value, lmbd, 0.3, epsilon)
    raw = orc.BDCM_ER(chi0, hp, p, c, attr_value, lmbd, 1.0, epsilon)
    return leaf, s1, s2, raw


@functools.lru_cache(maxsize=None)
def forest_case(T, n_iso=0):
    """(n_core, edges, row_ptr, col, oracle plan) of the hub forest of
    HUB_DEGREES[T] with ``n_iso`` isolated nodes on top; shared, never written."""
    n, edges, rp, col = hub_forest(HUB_DEGREES[T], seed=T)
    return n, edges, rp, col, orc.Plan.from_csr(edges, rp, col, n + n_iso, n_iso)


# a small forest for the symmetry tests: leaves, three hub classes, isolated nodes
SMALL_DEGREES = (2, 3, 4, 3)
N_ISO = 3


@functools.lru_cache(maxsize=None)
def small_case():
    n, edges, rp, col = hub_forest(SMALL_DEGREES, seed=11)
    return n, edges, rp, col, orc.Plan.from_csr(edges, rp, col, n + N_ISO, N_ISO)
