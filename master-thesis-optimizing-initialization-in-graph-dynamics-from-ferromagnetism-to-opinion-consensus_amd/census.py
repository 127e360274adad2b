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

Not covered: several devices (the block range makes it a host loop), n > 48,
symmetry reduction.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _device, _lib
from .dynamics import as_graph
from .graph import Graph
from .quench import _steps

N_MAX = 48
DEG_MAX = 47
# blocks of 64 configurations per launch: 2^26 configurations, a fraction of a millisecond of
# kernel at n = 32, so no single launch holds a shared device for long (census)
CHUNK_BLOCKS = 1 << 20


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


def _run(g, p, c, block_lo, block_hi, chunk, grid):
    """Blocks [block_lo, block_hi) in launches of at most ``chunk`` blocks -> (counts int64 (T+1, n+1), keys
    int64 (T+1,): the witness keys as signed words), device tensors."""
    n, T = g.n, p + c - 1
    dev = g.adj.device if g.kind == "ell" else g.row_ptr.device
    counts = torch.zeros((T + 1, n + 1), dtype=torch.int64, device=dev)
    keys = torch.full((T + 1,), -1, dtype=torch.int64, device=dev)           # all ones
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if g.kind == "ell":
        name, ga = "mjx_census_ell", (_device.ptr(g.adj) if g.d else None, n, g.d)
    else:
        name, ga = "mjx_census_csr", (_device.ptr(g.row_ptr), _device.ptr(g.col) if g.nnz else None, n)
    st = _device.stream_handle()
    for lo in range(block_lo, block_hi, chunk):
        _lib.call(name, *ga, p, c, lo, min(block_hi, lo + chunk), grid, _device.ptr(counts), _device.ptr(keys),
                  _device.ptr(flag), st)
    if int(flag.item()):
        raise _lib.MjxError("census: an adjacency entry lies outside 0..n-1 or a row is longer than 47")
    return counts, keys


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
    p, c, T = _steps(p, c)
    grid = _kernel_options(kernel)
    n = _host_n(graph)
    if n < 1:
        raise ValueError("census: the graph has no nodes")
    if n > N_MAX:
        raise ValueError(f"census: n = {n} nodes; the enumeration is limited to n <= {N_MAX}")
    configs = 1 << n
    if configs > int(max_configs):
        raise ValueError(f"census: 2^{n} = {configs} configurations exceed max_configs = {int(max_configs)}")
    blocks = 1 << max(n - 6, 0)
    chunk = CHUNK_BLOCKS if chunk_blocks is None else int(chunk_blocks)
    if chunk < 1:
        raise ValueError("chunk_blocks must be >= 1")
    _check_rows(_host_rows(graph), n)
    counts, keys = _run(as_graph(graph), p, c, 0, blocks, chunk, grid)
    cnt = counts.cpu().numpy()
    key = keys.cpu().numpy().view(np.uint64)
    if (key == np.uint64(0xFFFFFFFFFFFFFFFF)).any():                        # every level counts all +1 at least
        raise _lib.MjxError("census: a level without a witness")
    min_plus = (key >> np.uint64(48)).astype(np.int64)
    x = key & np.uint64((1 << 48) - 1)
    bits = (x[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)
    with np.errstate(divide="ignore"):
        entropy = np.log(cnt.astype(np.float64)) / n
    return {"counts": cnt, "min_plus": min_plus, "m_min": (2 * min_plus - n) / n,
            "witness": np.where(bits == 1, 1, -1).astype(np.int8), "entropy": entropy, "configs": configs}
