"""Exact consensus census of a small graph: ground truth by enumeration.

With T = p + c - 1 and x running over all 2^n start configurations (node v is
+1 iff bit v of x is set; definitions: include/mjx.h):

    counts[t, k]  = #{x : popcount(x) = k and onestep^t(x) is all +1}, t = 0..T
    min_plus[t]   = the smallest k with counts[t, k] > 0
    m_min[t]      = (2 min_plus[t] - n) / n, the exact minimal initial magnetisation
    witness[t]    = the configuration with the smallest (popcount(x), x) counted in counts[t]
    entropy[t, k] = ln(counts[t, k]) / n

SA, HPR and the quenches report a magnetisation at which consensus is reached;
this is the optimum they can be measured against, and the count a BDCM entropy
can be checked against, for n <= 48.  The configurations are generated inside
the kernel (csrc/mjx_census.hip: a lane per block of 64 configurations, the
levels in LDS), so the enumeration moves no memory; the host only splits the
blocks over launches of at most ``chunk_blocks`` each.

``census_minima`` keeps the membership bit of every x and counts, from that
bitmap, the minimal elements of every level: the local minima of the quenches.

``attractor_census`` runs every x to its attractor instead of a fixed horizon:
how many starts of each weight end all +1, all -1, in another fixed point or in
a 2-cycle, and after how many steps -- the exact counterpart of
``consensus_curve``.

``census_marginals`` counts the configurations of a level per +1 node as well,
which gives the backbone of the optimum and, through ``census_boltzmann``, the
exact phi, m_init and per-node marginals that BDCM and BP approximate.

Not covered: several devices (the block range makes it a host loop), n > 48,
symmetry reduction.  There is no CPU fallback.
"""
import math

import numpy as np
import torch

from . import _device, _lib
from .dynamics import as_graph
from .graph import Graph
from .quench import _steps

N_MAX = 48
DEG_MAX = 47
# blocks of 64 configurations per launch: 2^26 configurations, a fraction of a millisecond of
# kernel at n = 32 (about 2 ms for the attractor census, which sweeps until every configuration has
# settled), so no single launch holds a shared device for long (census)
CHUNK_BLOCKS = 1 << 20
# attractor_census: the classes in the order of hist's first axis, the kernel's limits (include/mjx.h)
CLASSES = ("plus", "minus", "fixed", "cycle")
T_MAX_CAP = 1024
LDS_MAX = 64 * 1024
LAUNCH_BLOCKS_MAX = 1 << 25            # 32-bit LDS cells: a launch counts at most 2^31 configurations


def _kernel_options(kernel):
    kernel = dict(kernel or {})
    grid = int(kernel.pop("grid", 0) or 0)
    if kernel:
        raise ValueError(f"unknown kernel options {sorted(kernel)}")
    if grid < 0:
        raise ValueError("grid must be >= 0")
    return grid


def _host_rows(graph):
    """The adjacency as host lists, one row of neighbours per node (n is small)."""
    if isinstance(graph, Graph):
        if graph.kind == "ell":
            return [list(r) for r in graph.adj.cpu().numpy().reshape(graph.n, graph.d).tolist()]
        rp, col = graph.row_ptr.cpu().numpy(), graph.col.cpu().numpy()
        return [col[rp[v]:rp[v + 1]].tolist() for v in range(graph.n)]
    a = graph.cpu().numpy() if isinstance(graph, torch.Tensor) else np.asarray(graph)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("graph must be a Graph or an integer (n, d) neighbour array")
    return a.tolist()


def _host_n(graph):
    if isinstance(graph, Graph):
        return graph.n
    shape = tuple(graph.shape) if hasattr(graph, "shape") else np.shape(graph)
    if len(shape) != 2:
        raise ValueError("graph must be a Graph or an integer (n, d) neighbour array")
    return int(shape[0])


def _check_rows(rows, n):
    """Range, row length and symmetry (u in row(v) as often as v in row(u)) on the host."""
    pairs = {}
    for v, row in enumerate(rows):
        if len(row) > DEG_MAX:
            raise ValueError(f"census: node {v} has {len(row)} neighbours, at most {DEG_MAX} are supported")
        for u in row:
            if not 0 <= u < n:
                raise ValueError("adjacency index out of range")
            pairs[(v, u)] = pairs.get((v, u), 0) + 1
    if any(pairs.get((u, v), 0) != k for (v, u), k in pairs.items()):
        raise ValueError("the adjacency is not symmetric (v in row(u) as often as u in row(v)): the census is "
                         "defined for undirected graphs")


def _launch(stem, g, head, block_lo, block_hi, chunk, grid, out, tail, what):
    """mjx_<stem>_{ell,csr}(graph, *head, lo, hi, grid, *out, flag, *tail, stream) on the blocks [block_lo,
    block_hi) in launches of at most ``chunk`` blocks; raises when a kernel raised the flag.  ``out`` and
    ``tail``: device tensors, or None."""
    kind, ga = g.kernel_args()
    flag = torch.zeros(1, dtype=torch.int32, device=g.device)
    ptrs = [None if t is None else _device.ptr(t) for t in (*out, flag, *tail)]
    st = _device.stream_handle()
    for lo in range(block_lo, block_hi, chunk):
        _lib.call(f"mjx_{stem}_{kind}", *ga, *head, lo, min(block_hi, lo + chunk), grid, *ptrs, st)
    if int(flag.item()):
        raise _lib.MjxError(f"{what}: an adjacency entry lies outside 0..n-1 or a row is longer than 47")


def _run(g, p, c, block_lo, block_hi, chunk, grid, mask=None):
    """Blocks [block_lo, block_hi) in launches of at most ``chunk`` blocks -> (counts int64 (T+1, n+1), keys
    int64 (T+1,): the witness keys as signed words), device tensors.  ``mask``: a device int64 (T+1, B)
    tensor that receives the membership words of the blocks (the mask entry points)."""
    n, T = g.n, p + c - 1
    counts = torch.zeros((T + 1, n + 1), dtype=torch.int64, device=g.device)
    keys = torch.full((T + 1,), -1, dtype=torch.int64, device=g.device)      # all ones
    _launch("census" if mask is None else "census_mask", g, (p, c), block_lo, block_hi, chunk, grid,
            (counts, keys), () if mask is None else (mask,), "census")
    return counts, keys


def _checked_enumeration(graph, max_configs, chunk_blocks, kernel, bitmap_levels=0, fits=None):
    """The host refusals every enumeration shares -> (graph, n, blocks, chunk, grid); ``bitmap_levels``:
    the refusal of a large 2^n names the bytes of a bitmap of that many levels; ``fits(n)``: the caller's
    own refusal of a shape, made before the graph goes to the device."""
    grid = _kernel_options(kernel)
    n = _host_n(graph)
    if n < 1:
        raise ValueError("census: the graph has no nodes")
    if n > N_MAX:
        raise ValueError(f"census: n = {n} nodes; the enumeration is limited to n <= {N_MAX}")
    configs = 1 << n
    if configs > int(max_configs):
        raise ValueError(f"census: 2^{n} = {configs} configurations exceed max_configs = {int(max_configs)}"
                         + (f"; the bitmap of the {bitmap_levels} levels would take (T+1) * 2^n / 8 = "
                            f"{bitmap_levels * max(configs, 64) // 8} bytes" if bitmap_levels else ""))
    blocks = 1 << max(n - 6, 0)
    chunk = CHUNK_BLOCKS if chunk_blocks is None else int(chunk_blocks)
    if chunk < 1:
        raise ValueError("chunk_blocks must be >= 1")
    if fits is not None:
        fits(n)
    _check_rows(_host_rows(graph), n)
    return as_graph(graph), n, blocks, chunk, grid


def _checked(graph, p, c, max_configs, chunk_blocks, kernel, mask=False):
    """The host refusals of ``census`` -> (graph, p, c, n, blocks, chunk, grid); ``mask``: the refusal of a
    large 2^n names the bytes of the bitmap."""
    p, c, T = _steps(p, c)
    g, n, blocks, chunk, grid = _checked_enumeration(graph, max_configs, chunk_blocks, kernel, (T + 1) if mask else 0)
    return g, p, c, n, blocks, chunk, grid


def _spins(key, n):
    """The configurations of keys k << 48 | x as +-1 rows, int8 (len(key), n)."""
    x = key & np.uint64((1 << 48) - 1)
    bits = (x[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)
    return np.where(bits == 1, 1, -1).astype(np.int8)


def _levels(cnt, key, n):
    """Counts and witness keys of the levels -> the result dict of ``census``."""
    min_plus = (key >> np.uint64(48)).astype(np.int64)
    with np.errstate(divide="ignore"):
        entropy = np.log(cnt.astype(np.float64)) / n
    return {"counts": cnt, "min_plus": min_plus, "m_min": (2 * min_plus - n) / n, "witness": _spins(key, n),
            "entropy": entropy, "configs": 1 << n}


def census(graph, p, c, *, max_configs=2 ** 36, chunk_blocks=None, kernel=None):
    """Count, for every weight, the start configurations of ``graph`` that are
    all +1 after t = 0..p+c-1 steps of the majority rule, by running all 2^n.

    graph: as for ``quench`` -- an ELL or CSR ``Graph`` with symmetric
    adjacency, or an (n, d) neighbour array; n <= 48, rows of at most 47
    entries.  ``max_configs``: a larger 2^n raises ValueError (an accidental
    n = 44 is an hour).  ``chunk_blocks``: 64-config blocks per launch (default
    2^20); ``kernel``: ``{"grid": g}`` forces the number of workgroups; the
    result depends on neither.

    Returns a dict of numpy arrays: ``counts`` int64 (T+1, n+1), ``min_plus``
    int64 (T+1,), ``m_min`` float64 (T+1,), ``witness`` int8 (T+1, n) of +-1,
    ``entropy`` float64 (T+1, n+1) (-inf where the count is 0) and ``configs``
    = 2^n.  Level 0 counts the all +1 configuration alone, so every level has a
    witness."""
    g, p, c, n, blocks, chunk, grid = _checked(graph, p, c, max_configs, chunk_blocks, kernel)
    counts, keys = _run(g, p, c, 0, blocks, chunk, grid)
    key = keys.cpu().numpy().view(np.uint64)
    if (key == np.uint64(0xFFFFFFFFFFFFFFFF)).any():                        # every level counts all +1 at least
        raise _lib.MjxError("census: a level without a witness")
    return _levels(counts.cpu().numpy(), key, n)


def census_minima(graph, p, c, *, max_configs=2 ** 34, chunk_blocks=None, kernel=None, return_mask=False):
    """``census`` and, for every level t, the census of its minimal consensus
    sets M_t: the configurations that are all +1 after t steps and from which
    no single +1 node can be dropped -- the local minima a greedy quench at
    T = t can end in (``quench``, ``quench_restarts``), all of them, by weight.

    Arguments as for ``census``.  Pass 1 is the census that keeps the bit "x is
    all +1 after t steps" of every x and level in a device bitmap of
    (T+1) * 2^n / 8 bytes (2 GiB at n = 32, T = 3: hence the smaller default of
    ``max_configs``, whose refusal names the bytes); pass 2 counts the minimal
    elements from the bitmap alone (mjx_census_minima, include/mjx.h).  Both
    run on the current stream in launches of at most ``chunk_blocks`` blocks,
    pass 2 in multiples of 64 blocks; ``kernel``: ``{"grid": g}`` forces the
    workgroups of both.

    Returns the dict of ``census`` (same values) and ``minima`` int64
    (T+1, n+1), ``minima_total`` int64 (T+1,), ``max_plus`` int64 (T+1,) with
    ``m_max`` = (2 max_plus - n) / n and ``witness_max`` int8 (T+1, n): the
    minimum with the largest (weight, x); ``mean_plus`` float64 (T+1,) =
    sum k minima / sum minima.  The lightest minimum is ``witness``, and
    ``minima[t, min_plus[t]] == counts[t, min_plus[t]]``.  ``return_mask``:
    also ``mask``, the device bitmap as int64 bit patterns (T+1, B),
    B = 2^max(n-6, 0): bit j of word b of level t is configuration 64 b + j."""
    g, p, c, n, blocks, chunk, grid = _checked(graph, p, c, max_configs, chunk_blocks, kernel, mask=True)
    T, dev = p + c - 1, g.device
    mask = torch.empty((T + 1, blocks), dtype=torch.int64, device=dev)       # pass 1 writes every word
    counts, keys = _run(g, p, c, 0, blocks, chunk, grid, mask=mask)
    minima = torch.zeros((T + 1, n + 1), dtype=torch.int64, device=dev)
    heavy = torch.zeros((T + 1,), dtype=torch.int64, device=dev)
    st = _device.stream_handle()
    rows = -(-chunk // 64) * 64                                              # a wave's 64 blocks go together
    for lo in range(0, blocks, rows):
        _lib.call("mjx_census_minima", _device.ptr(mask), n, T, lo, min(blocks, lo + rows), grid,
                  _device.ptr(minima), _device.ptr(heavy), st)
    key = keys.cpu().numpy().view(np.uint64)
    top = heavy.cpu().numpy().view(np.uint64)
    if (key == np.uint64(0xFFFFFFFFFFFFFFFF)).any() or (top == 0).any():    # all +1 is in every level
        raise _lib.MjxError("census_minima: a level without a minimum")
    res = _levels(counts.cpu().numpy(), key, n)
    mn = minima.cpu().numpy()
    max_plus = (top >> np.uint64(48)).astype(np.int64)
    res.update(minima=mn, minima_total=mn.sum(axis=1), max_plus=max_plus, m_max=(2 * max_plus - n) / n,
               witness_max=_spins(top, n),
               mean_plus=(mn * np.arange(n + 1)[None, :]).sum(axis=1) / mn.sum(axis=1))
    if return_mask:
        res["mask"] = mask
    return res


def census_nodes_lds(n):
    """LDS bytes of a workgroup of the census that also counts per node (mjx_census_nodes_lds without its
    ceiling): two levels, counts and keys, node[n+1][n] as 32-bit cells, level-0 patterns, row offsets,
    neighbour bytes."""
    return (1024 * n + 56 * (n + 2) + 4 * (n + 1) * n + 8 * n + 8 * (-(-(n + 1) // 4))
            + 8 * (-(-(DEG_MAX * n) // 8)))


def _run_nodes(g, p, c, t_node, block_lo, block_hi, chunk, grid):
    """``_run`` through the entry points that also count level ``t_node`` per node -> (counts, keys, node
    counts int64 (n+1, n)), device tensors."""
    n, T = g.n, p + c - 1
    counts = torch.zeros((T + 1, n + 1), dtype=torch.int64, device=g.device)
    keys = torch.full((T + 1,), -1, dtype=torch.int64, device=g.device)      # all ones
    node = torch.zeros((n + 1, n), dtype=torch.int64, device=g.device)
    _launch("census_nodes", g, (p, c, t_node), block_lo, block_hi, min(chunk, LAUNCH_BLOCKS_MAX), grid,
            (counts, keys, node), (), "census_marginals")
    return counts, keys, node


def _marginal_levels(levels, T):
    """``levels`` of ``census_marginals`` -> a list of step counts in 0..T, default [T]."""
    out = [T] if levels is None else list(levels)
    if not out:
        raise ValueError("census_marginals: levels is empty")
    for t in out:
        if int(t) != t or not 0 <= t <= T:
            raise ValueError(f"census_marginals: level {t} is outside 0..T = p + c - 1 = {T}")
    return [int(t) for t in out]


def census_marginals(graph, p, c, *, levels=None, max_configs=2 ** 36, chunk_blocks=None, kernel=None):
    """``census`` and, for each requested level t, where the +1 spins of the
    counted configurations sit:

        node_counts[l, k, v] = #{x : popcount(x) = k, bit v of x set,
                                 onestep^t(x) all +1},  t = levels[l]

    the exact per-node counts that BP marginals and BDCM's m_init approximate
    (``census_boltzmann`` turns them into the Boltzmann averages at any lambda).

    Arguments and refusals as for ``census``.  ``levels``: step counts in 0..T,
    T = p + c - 1, default ``[T]``; each is one enumeration by the census kernel
    with node cells in LDS (mjx_census_nodes_*, include/mjx.h), in launches of
    at most ``chunk_blocks`` blocks (at most 2^25 take effect).  BDCM at (p, c)
    corresponds to level t = p: for c = 2, x(p+1) all +1 and x(p+2) = x(p)
    force x(p) all +1.

    Returns the dict of ``census`` (same values) and ``levels`` (list),
    ``node_counts`` int64 (len(levels), n+1, n), ``optimal`` int64
    (len(levels),) = counts[t, min_plus[t]], and the backbone of the optimum,
    bool (len(levels), n): ``backbone_plus[l, v]`` -- node v is +1 in every
    configuration of weight min_plus[t] counted at level t
    (node_counts[l, min_plus[t], v] == optimal[l]) -- and ``backbone_minus``
    (that node count is 0)."""
    p_, c_, T = _steps(p, c)
    lv = _marginal_levels(levels, T)

    def fits(n):
        lds = census_nodes_lds(n)
        if lds > LDS_MAX:
            raise ValueError(f"census_marginals: n = {n} needs {lds} bytes of LDS per workgroup, more than {LDS_MAX}")

    g, n, blocks, chunk, grid = _checked_enumeration(graph, max_configs, chunk_blocks, kernel, fits=fits)
    runs = [_run_nodes(g, p_, c_, t, 0, blocks, chunk, grid) for t in lv]   # every pass counts the levels anew
    counts, keys = runs[-1][:2]
    node = torch.stack([r[2] for r in runs])
    key = keys.cpu().numpy().view(np.uint64)
    if (key == np.uint64(0xFFFFFFFFFFFFFFFF)).any():                        # every level counts all +1 at least
        raise _lib.MjxError("census_marginals: a level without a witness")
    res = _levels(counts.cpu().numpy(), key, n)
    nc = node.cpu().numpy()
    best = res["min_plus"][lv]
    optimal = res["counts"][lv, best]
    at_best = nc[np.arange(len(lv)), best]                                  # (len(levels), n)
    res.update(levels=lv, node_counts=nc, optimal=optimal, backbone_plus=at_best == optimal[:, None],
               backbone_minus=at_best == 0)
    return res


def census_boltzmann(res, lam, level=-1, attr_value=1):
    """The exact Boltzmann averages that BDCM approximates, from the counts of
    ``census_marginals``; float64 numpy, no device.

    With w_k = exp(-lam (2k - n)), t = res["levels"][level] and
    Z = sum_k counts[t, k] w_k (by log-sum-exp): ``phi`` = ln Z / n, ``m_init``
    = <2k - n> / n, ``ent1`` = phi + lam m_init, ``p_plus`` (n,) =
    sum_k node_counts[level, k, v] w_k / Z = P(s_v(0) = +1) and ``m_node`` =
    2 p_plus - 1.  These are BDCM's definitions (``phi_BP_GENERAL_ER``,
    ``avg_m_init_GENERAL_ER``) at attractor +1, its isolated nodes included: a
    node of degree 0 never moves, so it starts +1 in every counted x.
    ``level`` indexes ``res["levels"]``.  ``lam``: a scalar, or an array -- the
    outputs then gain a leading axis.  ``attr_value`` = -1 is refused: the
    census counts the configurations that end all +1 only."""
    if int(attr_value) != 1:
        raise ValueError(f"census_boltzmann: attr_value = {attr_value}; the census counts all +1 only (attr_value = 1)")
    levels = list(res["levels"])
    if not -len(levels) <= int(level) < len(levels):
        raise ValueError(f"census_boltzmann: level index {level} is outside the {len(levels)} levels of the result")
    t = levels[int(level)]
    counts = np.asarray(res["counts"])[t].astype(np.float64)
    node = np.asarray(res["node_counts"])[int(level)].astype(np.float64)   # (n+1, n)
    n = node.shape[1]
    lam_a = np.asarray(lam, dtype=np.float64)
    lm = lam_a.reshape(-1)
    mag = 2.0 * np.arange(n + 1) - n                                       # 2k - n
    with np.errstate(divide="ignore"):
        a = np.log(counts)[None, :] - lm[:, None] * mag[None, :]           # ln(counts w_k), -inf where 0
    top = a.max(axis=1)                                                    # finite: all +1 is counted
    e = np.exp(a - top[:, None])
    z = e.sum(axis=1)
    phi = (top + np.log(z)) / n
    m_init = (e * mag[None, :]).sum(axis=1) / z / n
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(counts[:, None] > 0, node / counts[:, None], 0.0)  # of the level's weight-k set
    p_plus = ((e / z[:, None])[:, :, None] * share[None, :, :]).sum(axis=1)  # no BLAS: the same for any batch
    out = {"phi": phi, "m_init": m_init, "ent1": phi + lm * m_init, "p_plus": p_plus, "m_node": 2.0 * p_plus - 1.0}
    return {k: v.reshape(lam_a.shape + v.shape[1:]) for k, v in out.items()}


def attractor_census_lds(n, t_max):
    """LDS bytes of a workgroup of the attractor census (mjx_attractor_census_lds without its ceiling): two
    levels, hist[4][t_max+1][n+1] and unsettled[n+1] as 32-bit cells, two keys, level-0 patterns, row offsets,
    neighbour bytes."""
    return (1024 * n + 16 * (t_max + 1) * (n + 1) + 8 * (-(-(n + 1) // 2)) + 16 + 8 * n + 8 * (-(-(n + 1) // 4))
            + 8 * (-(-(DEG_MAX * n) // 8)))


def _run_attractor(g, t_max, block_lo, block_hi, chunk, grid, stats=False):
    """Blocks [block_lo, block_hi) in launches of at most ``chunk`` blocks -> (hist int64 (4, t_max+1, n+1),
    unsettled int64 (n+1,), keys int64 (2,): lightest plus and longest as signed words, stats int64 (2,) or
    None: rows of 64 blocks and sweeps), device tensors."""
    n, dev = g.n, g.device
    hist = torch.zeros((4, t_max + 1, n + 1), dtype=torch.int64, device=dev)
    uns = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    keys = torch.tensor([-1, 0], dtype=torch.int64, device=dev)             # all ones; 0
    st8 = torch.zeros(2, dtype=torch.int64, device=dev) if stats else None
    _launch("attractor_census", g, (t_max,), block_lo, block_hi, min(chunk, LAUNCH_BLOCKS_MAX), grid,
            (hist, uns, keys), (st8,), "attractor_census")
    return hist, uns, keys, st8


def attractor_census(graph, t_max=32, *, max_configs=2 ** 36, chunk_blocks=None, kernel=None):
    """Run all 2^n start configurations of ``graph`` to their attractors and
    count them by class, transient and weight.

    With s(0) = x, s(t+1) = onestep(s(t)), p = min{t : s(t+2) = s(t)} and c = 1
    if s(p+1) = s(p) else 2 (``attractor``'s definitions), x is ``plus`` (c = 1,
    s(p) all +1), ``minus`` (c = 1, all -1), ``fixed`` (c = 1, neither) or
    ``cycle`` (c = 2); p > ``t_max`` is unsettled and in no class.

    graph, ``max_configs``, ``chunk_blocks`` (at most 2^25 take effect) and
    ``kernel`` as for ``census``; 0 <= t_max <= 1024, and the workgroup's LDS,
    1024 n + 16 (t_max+1)(n+1) + ..., must fit 64 KiB (n = 32 or 40 at
    t_max = 32 do, n = 48 up to t_max = 16).

    Returns a dict: ``hist`` int64 (4, t_max+1, n+1) [class, p, k], ``unsettled``
    int64 (n+1,), ``configs`` = 2^n, ``classes`` = ("plus", "minus", "fixed",
    "cycle"), ``reach_plus`` int64 (t_max+1, n+1) = cumsum of hist[0] over p
    (``census``'s ``counts`` for every horizon), ``p_plus`` float64 (n+1,) =
    sum_p hist[0, p, k] / C(n, k), the exact consensus curve, ``min_plus_ever``
    (the smallest weight that ever reaches all +1), ``m_min_ever`` =
    (2 min_plus_ever - n) / n, ``witness_plus`` int8 (n,) of +-1: the plus
    configuration with the smallest (weight, x), ``p_longest`` and
    ``witness_longest`` int8 (n,): the settled configuration with the largest
    (p, x), and ``mean_sweeps``: the sweeps a wave made on average."""
    t_max = int(t_max)
    if t_max < 0 or t_max > T_MAX_CAP:
        raise ValueError(f"attractor_census: t_max = {t_max}; need 0 <= t_max <= {T_MAX_CAP}")

    def fits(n):
        lds = attractor_census_lds(n, t_max)
        if lds > LDS_MAX:
            raise ValueError(f"attractor_census: n = {n}, t_max = {t_max} need {lds} bytes of LDS per workgroup, "
                             f"more than {LDS_MAX}: lower t_max")

    g, n, blocks, chunk, grid = _checked_enumeration(graph, max_configs, chunk_blocks, kernel, fits=fits)
    hist, uns, keys, st8 = _run_attractor(g, t_max, 0, blocks, chunk, grid, stats=True)
    key = keys.cpu().numpy().view(np.uint64)
    if key[0] == np.uint64(0xFFFFFFFFFFFFFFFF):                             # all +1 is a fixed point, p = 0
        raise _lib.MjxError("attractor_census: no configuration reached all +1")
    h = hist.cpu().numpy()
    rows, sweeps = (int(v) for v in st8.cpu().numpy())
    binom = np.array([math.comb(n, k) for k in range(n + 1)], dtype=np.float64)
    min_plus = int(key[0] >> np.uint64(48))
    return {"hist": h, "unsettled": uns.cpu().numpy(), "configs": 1 << n, "classes": CLASSES,
            "reach_plus": np.cumsum(h[0], axis=0), "p_plus": h[0].sum(axis=0) / binom,
            "min_plus_ever": min_plus, "m_min_ever": (2 * min_plus - n) / n, "witness_plus": _spins(key[:1], n)[0],
            "p_longest": int(key[1] >> np.uint64(48)), "witness_longest": _spins(key[1:], n)[0],
            "mean_sweeps": sweeps / rows}
