"""Flip gains and the greedy quench: prune a start to a local minimum.

With T = p + c - 1, s_end = onestep^T(s), F(s) = sum s_end and s^i = s with
spin i flipped (definitions and the monotonicity argument: include/mjx.h):

    gain[r, i]    = F(s^i) - F(s)
    consensus[r]  = (F(s) = n)
    removable     = bit (i, r) set iff s_i = +1, consensus[r] and F(s^i) = n
    quench        = visit the nodes in ``order``; drop every +1 spin whose
                    removal keeps the end state all +1 (per replica)

``flip_gains`` evaluates every (node, 64-replica word column) pair with the
bit-parallel light cone of csrc/mjx_quench.hip on the cached levels
onestep^t(s), t = 0..T (one ``rollout`` step per level); ``quench`` walks, per
word column, the nodes of the initial removable mask in ``order`` order with
the same evaluator and commits the accepted flips into copies of the levels.
SA and HPR stop at the first configuration that reaches consensus; this is the
zero-temperature clean-up after them.  ``quench(..., schedule="regions")`` is
the same pass in rounds: candidates further apart than 2 (p + c - 1) commute,
so those of a window whose balls meet no ball of an earlier pending candidate
commit together, for all word columns at once; the result is identical.

The local minimum depends on the visiting order.  ``quench_restarts`` runs
R starts x K orders as R K independent jobs in one call
(csrc/mjx_quench_lds.hip: a workgroup per job, the job's single replica
node-packed in LDS), with an order per job and, for an (R, n, d) stack, a graph
per start, and returns the best of the K results per start.

Every one of these ends in a single-flip local minimum.  ``quench_exchange``
runs the same jobs and then leaves that minimum downwards by (1, 2) exchanges:
one -1 spin becomes +1, two +1 spins near it are dropped, in passes over the
job's order until a pass commits nothing (k_quench_exchange_jobs in the same
unit; p + c - 1 <= 3).

Not covered: packed input to ``quench_restarts``, a CSR graph per start,
several devices.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _device, _lib
from .dynamics import as_graph, pack, popcount, rollout, unpack
from .graph import Graph, check_ell

T_MAX = 6


def _steps(p, c):
    p, c = int(p), int(c)
    T = p + c - 1
    if p < 0 or c < 0 or not 0 <= T <= T_MAX:
        raise ValueError(f"need p, c >= 0 and 0 <= p + c - 1 <= {T_MAX}, got p = {p}, c = {c}")
    return p, c, T


def _kernel_options(kernel):
    kernel = dict(kernel or {})
    lds_entries = int(kernel.pop("lds_entries", 0) or 0)
    if kernel:
        raise ValueError(f"unknown kernel options {sorted(kernel)}")
    if lds_entries < 0:
        raise ValueError("lds_entries must be >= 0")
    return lds_entries


def _host_n(graph, s, words):
    """Node count without touching the device."""
    if isinstance(graph, Graph):
        return graph.n
    if words is None:
        return int(np.shape(s)[-1])
    return int(np.shape(graph)[0])


def _are_permutations(rows, n):
    """rows: int64 (m, n) -> every row is a permutation of 0..n-1."""
    if not rows.size:
        return True
    slots = rows + n * np.arange(rows.shape[0])[:, None]         # row j counts into its own n bins
    return bool(rows.min() >= 0 and rows.max() < n and np.bincount(slots.ravel(), minlength=rows.size).max() == 1)


def _check_order(order, seed, n):
    """``order`` as an int64 numpy permutation of 0..n-1, or None for the
    identity; host only."""
    if order is not None and seed is not None:
        raise ValueError("give order or seed, not both")
    if seed is not None:
        return np.random.default_rng(seed).permutation(n).astype(np.int64)
    if order is None:
        return None
    o = np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order)
    if o.ndim != 1 or o.shape[0] != n or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f"order must be an integer permutation of 0..{n - 1}")
    o = o.astype(np.int64)
    if not _are_permutations(o[None, :], n):
        raise ValueError(f"order must be a permutation of 0..{n - 1}")
    return o


def _check_symmetric(g):
    if g.kind == "ell":
        if check_ell(g)[2]:
            raise ValueError("the neighbour array is not symmetric: the light cone relies on it")
    else:
        from .sa_er import csr_is_symmetric
        if not csr_is_symmetric(g):
            raise ValueError("the CSR adjacency is not symmetric (v in row(u) as often as u in row(v)): "
                             "the light cone relies on it")


def _spins_2d(s):
    """+-1 spins (n,) or (R, n) -> (contiguous 2-D int8 / int32 / int64 device tensor, "s is a vector")."""
    t = _device.to_device(s)
    vector = t.dim() == 1
    if vector:
        t = t[None, :]
    if t.dtype not in (torch.int8, torch.int32, torch.int64):
        t = t.to(torch.int64)
    return t.contiguous(), vector


def _conf_like(conf, s, vector):
    """conf: device spins (R, n) -> the shape, kind and dtype of the input ``s``."""
    if vector:
        conf = conf[0]
    if isinstance(s, torch.Tensor):
        return conf.to(device=s.device, dtype=s.dtype)
    return conf.cpu().numpy().astype(np.asarray(s).dtype, copy=False)


def _packed_input(g, s, words):
    """-> (bits, R, W, "the +-1 input is a vector" or None for packed input)."""
    if words is not None:
        bits = _device.to_device(s, torch.int64).reshape(-1)
        W = int(words)
        if W < 1 or bits.numel() != g.n * W:
            raise ValueError(f"packed spins hold {bits.numel()} words, n * words = {g.n * W}")
        return bits, 64 * W, W, None
    t, vector = _spins_2d(s)
    if t.dim() != 2 or t.shape[1] != g.n:
        raise ValueError(f"spins must be (n,) or (R, n) with n = {g.n}")
    R = t.shape[0]
    return pack(t), R, _device.words_for(R), vector


def _levels(g, bits, W, T, copy):
    """[onestep^t(s) for t = 0..T]; level 0 is ``bits`` itself unless ``copy``."""
    lv = [bits.clone() if copy else bits]
    for _ in range(T):
        lv.append(rollout(g, lv[-1], 1, words=W))
    return lv


def _caps(g, T):
    out = (_lib.c_i64 * (T + 1))()
    if g.kind == "ell":
        _lib.call("mjx_ell_ball_bound", g.n, g.d, T, out)
    else:
        from .sa_er import SAReplicasER
        out = (_lib.c_i64 * (T + 1))(*SAReplicasER.ball_bound(g, T))
    return out


def _scratch(nbytes, what, T, lds_entries, dev):
    if nbytes < 0 or _lib.load().mjx_quench_lds(T, lds_entries) < 0:
        raise ValueError(f"{what}: lds_entries = {lds_entries} does not fit the workgroup's LDS at p + c - 1 = {T}")
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device=dev)


def _check_overflow(scratch, what):
    if int(scratch[0].item()):
        raise _lib.MjxError(f"{what}: a light-cone list outgrew the ball bound of the graph")


def _cone_call(entry, what, g, levels, R, p, c, T, caps, lds_entries, scratch_bytes):
    """The set-up the level-based entry points share -> (call, consensus uint8 [R]).  ``call(*args)`` runs
    mjx_<entry>_{ell,csr}_rp(graph, R, p, c, levels, caps, lds_entries, scratch, its bytes, *args, stream) on
    one scratch area of ``scratch_bytes`` and raises when the overflow flag is up afterwards."""
    dev = levels[0].device
    scratch = _scratch(scratch_bytes, what, T, lds_entries, dev)
    lv = (ctypes.c_void_p * (T + 1))(*[t.data_ptr() for t in levels])
    kind, ga = g.kernel_args()

    def call(*args):
        _lib.call(f"mjx_{entry}_{kind}_rp", *ga, R, p, c, lv, caps, lds_entries, _device.ptr(scratch),
                  scratch.numel() * 8, *args, _device.stream_handle())
        _check_overflow(scratch, what)

    return call, torch.empty(R, dtype=torch.uint8, device=dev)


def _flip_gains_packed(g, levels, R, W, p, c, T, caps, lds_entries, gain):
    """Device call on cached levels -> (removable, consensus uint8 [R], gain int32 (n, 64 W) or None)."""
    dev = levels[0].device
    call, consensus = _cone_call("flip_gain", "flip_gains", g, levels, R, p, c, T, caps, lds_entries,
                                 _lib.load().mjx_flip_gain_scratch_bytes(g.n, R, T, caps, lds_entries))
    removable = torch.empty(g.n * W, dtype=torch.int64, device=dev)
    gains = torch.empty((g.n, 64 * W), dtype=torch.int32, device=dev) if gain else None
    call(_device.ptr(removable), _device.ptr(consensus), _device.ptr(gains))
    return removable, consensus, gains


def _like(x, like):
    return x.to(like.device) if isinstance(like, torch.Tensor) else x.cpu().numpy()


def flip_gains(graph, s, p, c, words=None, gain=True, kernel=None, validate=True):
    """Per-node flip gains of every replica of ``s`` on ``graph``.

    graph: an ELL or CSR ``Graph`` with symmetric adjacency, or an (n, d)
    neighbour array.  s: +-1 spins (n,) or (R, n); or, with ``words``,
    replica-packed bits (n * words int64, 64 * words replicas).  The input is
    never written.  ``validate`` checks the symmetry once (``check_ell`` /
    ``csr_is_symmetric``).  ``kernel``: ``{"lds_entries": k}`` list entries kept
    in LDS (tests use a small k to force the scratch path); the results never
    depend on it.

    Returns a dict: ``gain`` int32 (R, n) (None with ``gain=False``: the table
    is 4 n R bytes, large runs ask for the masks only), ``removable`` (packed
    device tensor, n * ``words`` int64), ``consensus`` bool [R], ``n_removable``
    int64 [R] and ``words``.  numpy in -> numpy out, tensor in -> tensors on the
    input's device (``removable`` stays a device tensor either way)."""
    p, c, T = _steps(p, c)
    lds_entries = _kernel_options(kernel)
    g = as_graph(graph)
    if validate:
        _check_symmetric(g)
    bits, R, W, _ = _packed_input(g, s, words)
    levels = _levels(g, bits, W, T, copy=False)
    removable, consensus, gains = _flip_gains_packed(g, levels, R, W, p, c, T, _caps(g, T), lds_entries, gain)
    out = {"gain": _like(gains[:, :R].t().contiguous(), s) if gain else None,
           "removable": removable,
           "consensus": _like(consensus.to(torch.bool), s),
           "n_removable": _like(popcount(removable, g.n, words=W)[:R], s),
           "words": W}
    return out


def _candidates(removable, n, W, order):
    """Per word column the nodes with a removable bit, in ``order`` order:
    (cand int32 [K], cand_ptr int64 [W + 1]) on the device."""
    rem = removable.view(n, W) != 0
    if order is not None:
        order_t = torch.from_numpy(order).to(removable.device)
        rem = rem[order_t]
    nz = rem.t().nonzero()                          # sorted by (column, position in order)
    pos = nz[:, 1]
    cand = (pos if order is None else order_t[pos]).to(torch.int32).contiguous()
    cand_ptr = torch.zeros(W + 1, dtype=torch.int64, device=removable.device)
    cand_ptr[1:] = torch.cumsum(rem.sum(dim=0), dim=0)
    return cand, cand_ptr


def _quench_prepare(g, bits, R, W, p, c, T, lds_entries):
    """The parallel part of both schedules: the caps, copies of the levels and
    the initial removable mask -> (levels, caps, removable)."""
    caps = _caps(g, T)
    levels = _levels(g, bits, W, T, copy=True)
    removable, _, _ = _flip_gains_packed(g, levels, R, W, p, c, T, caps, lds_entries, False)
    return levels, caps, removable


def _quench_pass(g, levels, R, W, p, c, T, caps, cand, cand_ptr, lds_entries):
    """The sequential part, one workgroup per word column; ``levels`` are
    updated in place -> (consensus uint8 [R], flipped int64 [R])."""
    call, consensus = _cone_call("quench", "quench", g, levels, R, p, c, T, caps, lds_entries,
                                 _lib.load().mjx_quench_scratch_bytes(R, T, caps, lds_entries))
    flipped = torch.zeros(64 * W, dtype=torch.int64, device=levels[0].device)
    call(_device.ptr(cand) if cand.numel() else None, _device.ptr(cand_ptr), _device.ptr(consensus),
         _device.ptr(flipped))
    return consensus, flipped[:R]


def _quench_packed(g, bits, R, W, p, c, T, order, lds_entries, schedule="sequential", window=None):
    """-> (state = packed result (a new tensor), consensus uint8 [R], flipped int64 [R], candidates visited,
    the regions pass's {"rounds", "window", "max_commits"} or {})."""
    levels, caps, removable = _quench_prepare(g, bits, R, W, p, c, T, lds_entries)
    if schedule == "regions":
        cand, visited = _union_candidates(removable, g.n, W, order)
        consensus, flipped, info = _quench_regions_pass(g, levels, R, W, p, c, T, caps, removable, cand, window,
                                                        lds_entries)
    else:
        cand, cand_ptr = _candidates(removable, g.n, W, order)
        consensus, flipped = _quench_pass(g, levels, R, W, p, c, T, caps, cand, cand_ptr, lds_entries)
        visited, info = int(cand.numel()), {}
    return levels[0], consensus, flipped, visited, info


SCHEDULES = ("sequential", "regions")
WINDOW_BALLS = 16           # default window: this many times n / (estimated 2T-ball), see default_window
WINDOW_MAX = 8192


def _check_schedule(schedule, window):
    """Host only -> window as an int or None."""
    if schedule not in SCHEDULES:
        raise ValueError(f"unknown schedule {schedule!r}: one of {SCHEDULES}")
    if window is None:
        return None
    if schedule != "regions":
        raise ValueError("window belongs to schedule='regions': the sequential pass has none")
    if isinstance(window, bool) or int(window) != window or int(window) < 1:
        raise ValueError(f"window must be an integer >= 1, got {window!r}")
    return int(window)


def default_window(n, ball_T):
    """Slots of the regions pass when none are asked for.  Two candidates can
    commit together when their radius-T balls (at most ``ball_T`` = caps[T]
    nodes) do not meet, so about n / B candidates fit one round, B the 2T-ball,
    estimated from above by min(n, ball_T^2); slots past a few times that only
    wait.  WINDOW_BALLS of them, at least 1, at most WINDOW_MAX (the stored
    balls, 4 ball_T bytes a slot, then stay below 64 MB for every n < 2^31)."""
    n, ball_T = int(n), max(1, int(ball_T))
    return int(max(1, min(WINDOW_BALLS * n // min(n, ball_T * ball_T), WINDOW_MAX)))


def _union_candidates(removable, n, W, order):
    """The nodes with a removable bit in any word column, in ``order`` order
    (int32 on the device), and the (node, column) pairs the pass visits."""
    rem = removable.view(n, W) != 0
    visited = int(rem.sum().item())
    some = rem.any(dim=1)
    if order is None:
        cand = some.nonzero()[:, 0]
    else:
        order_t = torch.from_numpy(order).to(removable.device)
        cand = order_t[some[order_t].nonzero()[:, 0]]
    return cand.to(torch.int32).contiguous(), visited


def _quench_regions_pass(g, levels, R, W, p, c, T, caps, removable, cand, window, lds_entries):
    """The pass in rounds (csrc/mjx_quench.hip, the region-parallel pass):
    ``levels`` are updated in place -> (consensus uint8 [R], flipped int64 [R],
    {"rounds", "window", "max_commits"}).  The host reads the candidates-left
    counter once per chunk of rounds and never enqueues more rounds than there
    are candidates."""
    dev = levels[0].device
    ncand = int(cand.numel())
    K = max(1, min(default_window(g.n, caps[T]) if window is None else window, ncand))
    call, consensus = _cone_call("quench_regions", "quench", g, levels, R, p, c, T, caps, lds_entries,
                                 _lib.load().mjx_quench_regions_scratch_bytes(g.n, R, T, caps, lds_entries, K))
    flipped = torch.empty(64 * W, dtype=torch.int64, device=dev)
    stats = torch.empty(4, dtype=torch.int64, device=dev)

    def enqueue(round0, rounds):
        call(K, _device.ptr(removable), _device.ptr(cand) if ncand else None, ncand, _device.ptr(consensus),
             _device.ptr(flipped), _device.ptr(stats), round0, rounds)
        return [int(x) for x in stats.cpu().tolist()]

    launched = min(ncand, 16)
    left, rounds, most, _ = enqueue(0, launched)
    while left:
        if launched >= ncand:
            raise _lib.MjxError(f"quench: {left} of {ncand} candidates are left after {launched} rounds; every round "
                                "with a pending candidate commits one")
        # as many rounds as the commits per round so far would need, at most 1024 between two reads
        chunk = min(ncand - launched, 1024, max(1, -(-left * rounds // max(1, ncand - left))))
        left, rounds, most, _ = enqueue(launched, chunk)
        launched += chunk
    return consensus, flipped[:R], {"rounds": rounds, "window": K, "max_commits": most}


def quench(graph, s, p, c, order=None, seed=None, words=None, kernel=None, validate=True, schedule="sequential",
           window=None):
    """One greedy pass: every consensus replica of ``s`` visits the nodes in
    ``order`` (a permutation of 0..n-1 shared by all replicas; default the
    identity; ``seed`` is shorthand for ``np.random.default_rng(seed)
    .permutation(n)``) and drops each +1 spin whose removal keeps
    onestep^(p+c-1) all +1.  The result has an empty removable mask; replicas
    without consensus come back unchanged; the input is never written.

    Inputs as ``flip_gains``.  Returns a dict: ``conf`` (+-1 input only: same
    shape and kind as the input), ``state`` and ``words`` (the packed result, a
    device tensor of n * ``words`` int64: all a packed input gets back),
    ``flipped`` int64 [R], ``consensus`` bool [R] (of the input), ``mag``
    float64 [R] = sum(s)/n of the result, ``visited`` = candidates walked.

    ``schedule``: ``"sequential"`` (default) walks every word column's
    candidates one after the other, a workgroup per column.  ``"regions"``
    gives the same result, bit for bit, in rounds: the candidates of all
    columns share one order, and those of a window of ``window`` pending
    candidates whose radius-(p+c-1) balls meet no ball of an earlier pending
    candidate commit together, on as many workgroups as there are (candidate,
    column) pairs (``window=None``: ``default_window``).  It adds ``rounds``,
    ``window`` (the slots used: never more than there are candidates) and
    ``max_commits`` (the most candidates of one round) to the dict.  It pays
    on large graphs (n of 1e5 and more at T = 3, d = 4)."""
    p, c, T = _steps(p, c)
    lds_entries = _kernel_options(kernel)
    window = _check_schedule(schedule, window)
    order = _check_order(order, seed, _host_n(graph, s, words))
    g = as_graph(graph)
    if order is not None and order.shape[0] != g.n:
        raise ValueError(f"order must be a permutation of 0..{g.n - 1}")
    if validate:
        _check_symmetric(g)
    bits, R, W, vector = _packed_input(g, s, words)
    state, consensus, flipped, visited, info = _quench_packed(g, bits, R, W, p, c, T, order, lds_entries, schedule,
                                                              window)
    plus = popcount(state, g.n, words=W)[:R]
    # sum(s) / n as numpy divides two integers (a device division may multiply by 1/n)
    mag = torch.from_numpy((2 * plus.cpu().numpy() - g.n) / g.n)
    out = {"flipped": _like(flipped, s), "consensus": _like(consensus.to(torch.bool), s), "mag": _like(mag, s),
           "visited": visited, "state": state, "words": W, **info}
    if words is None:
        out["conf"] = _conf_like(unpack(state, g.n, R), s, vector)
    return out


# ---------------------------------------------------------------------------
# restarts: a job per (start, order), the state in LDS (csrc/mjx_quench_lds.hip)
# ---------------------------------------------------------------------------
def restart_order(seed, r, k, n):
    """The order of job (start r, restart k) under ``seed``."""
    return np.random.default_rng([int(seed), int(r), int(k)]).permutation(n)


def pick_best(sums):
    """sums: integer (R, K) = sum of the spins of every job's result -> int64
    [R], per start the restart with the smallest sum, the smallest k on ties."""
    return np.argmin(np.asarray(sums), axis=1).astype(np.int64)


def _check_orders(orders, seed, restarts, R, n):
    """-> int32 numpy orders (1 or R, K, n); host only."""
    K = int(restarts)
    if K < 1:
        raise ValueError("restarts must be >= 1")
    if orders is not None and seed is not None:
        raise ValueError("give orders or seed, not both")
    if seed is not None:
        return np.stack([np.stack([restart_order(seed, r, k, n) for k in range(K)])
                         for r in range(R)]).astype(np.int32)
    if orders is None:
        if K != 1:
            raise ValueError("restarts > 1 needs orders or seed: without them every restart would walk the identity")
        return np.arange(n, dtype=np.int32).reshape(1, 1, n)
    o = np.asarray(orders.cpu() if isinstance(orders, torch.Tensor) else orders)
    if o.ndim not in (1, 2, 3) or o.shape[-1] != n or not np.issubdtype(o.dtype, np.integer):
        raise ValueError(f"orders must be integer permutations of 0..{n - 1}: (n,), (K, n) or (R, K, n)")
    o = o.reshape((1,) * (3 - o.ndim) + o.shape).astype(np.int64)
    if o.shape[1] != K:
        raise ValueError(f"restarts = {K} but orders holds {o.shape[1]} per start")
    if o.shape[0] not in (1, R):
        raise ValueError(f"orders of shape (R, K, n) need R = {R} starts, got {o.shape[0]}")
    if not _are_permutations(o.reshape(-1, n), n):
        raise ValueError(f"every row of orders must be a permutation of 0..{n - 1}")
    return np.ascontiguousarray(o, dtype=np.int32)


def _host_shapes(graph, s):
    """(graph per start?, n, R) without touching the device."""
    if isinstance(graph, Graph):
        stack, n = False, graph.n
    elif isinstance(graph, (list, tuple)) and any(isinstance(x, Graph) for x in graph):
        raise ValueError("a graph per start must be an (R, n, d) neighbour stack (ELL); a CSR graph is shared by "
                         "all starts")
    else:
        gs = tuple(graph.shape) if hasattr(graph, "shape") else np.shape(graph)
        if len(gs) not in (2, 3):
            raise ValueError("graph must be a Graph, an (n, d) neighbour array or an (R, n, d) stack of them")
        stack, n = len(gs) == 3, int(gs[-2])
    ss = tuple(s.shape) if hasattr(s, "shape") else np.shape(s)
    if len(ss) not in (1, 2) or ss[-1] != n:
        raise ValueError(f"spins must be (n,) or (R, n) with n = {n}; packed input is not taken here")
    R = 1 if len(ss) == 1 else int(ss[0])
    if R < 1:
        raise ValueError("no starts")
    if stack and int(gs[0]) != R:
        raise ValueError(f"a graph per start: {int(gs[0])} graphs for {R} starts")
    return stack, n, R


def _run_jobs(g, adj_stack, R, K, p, c, caps, s_np, order_t, exchange=None, what="quench_restarts", anneal=None):
    """The device call: R x K jobs -> (out_np int64 (R K, ceil(n/64)), flipped int64 [R K], plus int64 [R K],
    consensus uint8 [R]).  g: the shared graph, or any graph of ``adj_stack`` (device int32 (R, n, d): a graph
    per start); s_np int64 (R, ceil(n/64)); order_t device int32 (1 or R, K, n).  ``exchange`` = (cap2T,
    max_passes, "with stats"): the exchange descent behind the pass (mjx_quench_exchange_jobs_*); a fifth
    entry of the result then holds plus_quench, exchanges, passes int64 [R K], converged uint8 [R K] and
    stats int64 (R K, 4) or None.  ``anneal`` = (thr device int32 tensor holding the uint32 thresholds, seed,
    "with trace"): the Metropolis sweeps behind the pass (mjx_quench_anneal_jobs_*); the fifth entry then holds
    plus_quench, plus_best, best_sweep int64 [R K], moves int64 (R K, 3) and trace int32 (R K, U) or None."""
    n, dev, st = g.n, s_np.device, _device.stream_handle()
    Wn = (n + 63) // 64

    def new(dtype, *shape):
        return torch.empty(shape or (R * K,), dtype=dtype, device=dev)

    out_np, flipped, plus = new(torch.int64, R * K, Wn), new(torch.int64), new(torch.int64)
    consensus, flag = new(torch.uint8, R), new(torch.int32)
    jobs = (R, K, p, c, caps)
    starts = (_device.ptr(s_np), _device.ptr(order_t), K * n if order_t.shape[0] > 1 else 0)
    outs = (_device.ptr(out_np), _device.ptr(flipped), _device.ptr(plus))
    ends = (_device.ptr(consensus), _device.ptr(flag))
    if anneal is not None:
        thr, seed, with_trace = anneal
        U = int(thr.numel())
        more = {"plus_quench": new(torch.int64), "plus_best": new(torch.int64), "best_sweep": new(torch.int64),
                "moves": new(torch.int64, R * K, 3), "trace": new(torch.int32, R * K, U) if with_trace else None}
        entry = "mjx_quench_anneal_jobs"
        tail = (*jobs, U, _device.ptr(thr) if U else None, seed, *starts, *outs, _device.ptr(more["plus_quench"]),
                _device.ptr(more["plus_best"]), _device.ptr(more["best_sweep"]), _device.ptr(more["moves"]),
                _device.ptr(more["trace"]) if with_trace and U else None, *ends, st)
    elif exchange is None:
        entry, tail, more = "mjx_quench_jobs", (*jobs, *starts, *outs, *ends, st), None
    else:
        cap2T, max_passes, with_stats = exchange
        rank = new(torch.int32, R * K * n)
        more = {"plus_quench": new(torch.int64), "exchanges": new(torch.int64), "passes": new(torch.int64),
                "converged": new(torch.uint8), "stats": new(torch.int64, R * K, 4) if with_stats else None}
        entry = "mjx_quench_exchange_jobs"
        tail = (*jobs, cap2T, max_passes, *starts, _device.ptr(rank), *outs, _device.ptr(more["plus_quench"]),
                _device.ptr(more["exchanges"]), _device.ptr(more["passes"]), _device.ptr(more["converged"]), *ends,
                _device.ptr(more["stats"]), st)
    if g.kind == "ell":
        adj = g.adj if adj_stack is None else adj_stack
        _lib.call(entry + "_ell", _device.ptr(adj) if g.d else None, n, g.d, 0 if adj_stack is None else n * g.d, *tail)
    else:
        _lib.call(entry + "_csr", _device.ptr(g.row_ptr), _device.ptr(g.col) if g.nnz else None, n, *tail)
    flags = int(flag.max().item())
    if flags & 1:
        raise _lib.MjxError(f"{what}: a light-cone list outgrew the ball bound of the graph")
    if flags & 2:
        raise _lib.MjxError(f"{what}: an order or adjacency entry lies outside 0..n-1")
    if flags:
        raise _lib.MjxError(f"{what}: " + ("an accepted add" if anneal is not None else "a flip that restores the state")
                            + " did not commit (a bug in the kernel)")
    res = (out_np, flipped, plus, consensus)
    return res if more is None else res + (more,)


EXCHANGE_T_MAX = 3          # the candidates of an add lie in a ball of radius 2T, and the ball bounds serve 6


def _quench_jobs(what, graph, s, p, c, restarts, orders, seed, keep_all, kernel, validate, exchange=False,
                 max_passes=None, anneal=None):
    """``quench_restarts``, ``quench_exchange`` (``exchange``, with its ``max_passes``) and ``quench_anneal``
    (``anneal`` = (uint32 numpy thresholds, seed, "with trace")): the checks, the device call and the result
    dict they share."""
    p, c, T = _steps(p, c)
    if kernel:
        raise ValueError(f"unknown kernel options {sorted(dict(kernel))}")
    if exchange:
        if T > EXCHANGE_T_MAX:
            raise ValueError(f"{what}: need p + c - 1 <= {EXCHANGE_T_MAX} (the candidates of an add fill a ball of "
                             f"radius 2 (p + c - 1)), got p = {p}, c = {c}")
        if not isinstance(max_passes, (int, np.integer)) or isinstance(max_passes, bool) or max_passes < 1:
            raise ValueError(f"max_passes must be an integer >= 1, got {max_passes!r}")
        max_passes = int(max_passes)
    stack, n, R = _host_shapes(graph, s)
    K = int(restarts)
    orders = _check_orders(orders, seed, K, R, n)
    lib = _lib.load()

    def lds_of(caps, caps2):
        """LDS bytes of a job; refuses a shape that does not fit."""
        lds = int(lib.mjx_quench_exchange_jobs_lds(n, T, caps, caps2[2 * T]) if exchange else
                  lib.mjx_quench_anneal_jobs_lds(n, T, caps) if anneal is not None else
                  lib.mjx_quench_jobs_lds(n, T, caps))
        if lds < 0:
            raise ValueError(f"{what}: a job of n = {n}, p + c - 1 = {T} (ball bound {list(caps)}) does not fit "
                             "the workgroup's LDS; quench is the path for this shape")
        return lds

    def ell_caps(d, radius):
        out = (_lib.c_i64 * (radius + 1))()
        _lib.call("mjx_ell_ball_bound", n, d, radius, out)
        return out

    d_host = graph.d if isinstance(graph, Graph) and graph.kind == "ell" else \
        None if isinstance(graph, Graph) else int((graph.shape if hasattr(graph, "shape") else np.shape(graph))[-1])
    if d_host is not None and 0 <= d_host <= 255:
        # a neighbour array: the budget is a function of (n, d), known before anything reaches the device
        lds_of(ell_caps(d_host, T), ell_caps(d_host, 2 * T) if exchange else None)
    if stack:
        adj = graph.cpu().numpy() if isinstance(graph, torch.Tensor) else np.asarray(graph)
        if not np.issubdtype(adj.dtype, np.integer):
            raise ValueError("the (R, n, d) graph stack must be an integer array")
        if adj.size and (adj.min() < 0 or adj.max() >= n):
            raise ValueError("adjacency index out of range")
        d = int(adj.shape[2])
        adj_t = _device.to_device(adj.astype(np.int32, copy=False))
        graphs = [Graph("ell", n, d=d, adj=adj_t[r]) for r in range(R)]
        g = graphs[0]
    else:
        g = as_graph(graph)
        graphs = [g]
    if validate:
        for gr in graphs:
            _check_symmetric(gr)
    caps = _caps(g, T)                      # ELL: a function of (n, d) alone, the same for every graph of a stack
    caps2 = _caps(g, 2 * T) if exchange else None
    lds_of(caps, caps2)
    t, vector = _spins_2d(s)
    dev, st, Wn = t.device, _device.stream_handle(), (n + 63) // 64
    s_np = torch.empty((R, Wn), dtype=torch.int64, device=dev)
    code, step = _device.dtype_code(t), n * t.element_size()
    for r in range(R):
        _lib.call("mjx_pack_np", t.data_ptr() + r * step, code, n, s_np.data_ptr() + r * Wn * 8, st)
    order_t = _device.to_device(orders)
    if anneal is not None:
        # the uint32 thresholds travel as the same bits in an int32 tensor
        anneal = (_device.to_device(anneal[0].view(np.int32)), anneal[1], anneal[2])
    out_np, flipped, plus, consensus, *more = _run_jobs(
        g, adj_t if stack else None, R, K, p, c, caps, s_np, order_t,
        (int(caps2[2 * T]), max_passes, False) if exchange else None, what, anneal)
    sums = 2 * plus.cpu().numpy().reshape(R, K) - n
    best = pick_best(sums)
    # sum(s) / n as numpy divides two integers, as quench does
    mag = sums / n
    mag_best = mag[np.arange(R), best]
    state_best = out_np.view(R, K, Wn)[torch.arange(R, device=dev), torch.from_numpy(best).to(dev)].contiguous()

    def rows(bits, dtype):
        conf = torch.empty((bits.shape[0], n), dtype=dtype, device=dev)
        dc, row = _device.dtype_code(conf), n * conf.element_size()
        for j in range(bits.shape[0]):
            _lib.call("mjx_unpack_np", bits.data_ptr() + j * Wn * 8, n, conf.data_ptr() + j * row, dc, st)
        return conf

    conf_best = _conf_like(rows(state_best, t.dtype), s, vector)
    out = {"mag": _like(torch.from_numpy(mag), s), "flipped": _like(flipped.view(R, K), s),
           "consensus": _like(consensus.to(torch.bool), s), "best": _like(torch.from_numpy(best), s),
           "conf_best": conf_best, "mag_best": _like(torch.from_numpy(mag_best), s), "state_best": state_best}
    if exchange:
        x = more[0]
        mag_quench = (2 * x["plus_quench"].cpu().numpy().reshape(R, K) - n) / n
        out.update({"mag_quench": _like(torch.from_numpy(mag_quench), s),
                    "exchanges": _like(x["exchanges"].view(R, K), s), "passes": _like(x["passes"].view(R, K), s),
                    "converged": _like(x["converged"].view(R, K).to(torch.bool), s)})
    if anneal is not None:
        x = more[0]
        for key, src in (("mag_quench", "plus_quench"), ("mag_best_sweep", "plus_best")):
            out[key] = _like(torch.from_numpy((2 * x[src].cpu().numpy().reshape(R, K) - n) / n), s)
        out["best_sweep"] = _like(x["best_sweep"].view(R, K), s)
        for j, key in enumerate(("adds", "drops", "refused")):
            out[key] = _like(x["moves"][:, j].contiguous().view(R, K), s)
        if anneal[2]:
            out["trace"] = _like(x["trace"].view(R, K, -1), s)
    if keep_all:
        out["conf"] = _like(rows(out_np, torch.int8).view(R, K, n), s)
    return out


def quench_restarts(graph, s, p, c, restarts=1, orders=None, seed=None, keep_all=False, kernel=None, validate=True):
    """Best of ``restarts`` greedy passes per start, every (start r, restart k)
    a job with its own visiting order, all jobs in one device call.

    graph: as for ``quench``, shared by the starts; or an (R, n, d) integer
    array, start r living on graph r (ELL only).  s: +-1 spins (n,) or (R, n).
    orders: (n,), (K, n) shared by the starts, or (R, K, n), every row a
    permutation of 0..n-1 and K = ``restarts``; or ``seed``: job (r, k) walks
    ``np.random.default_rng([seed, r, k]).permutation(n)`` (``restart_order``).
    With neither, ``restarts`` must be 1 and the order is the identity.  A
    job's result is ``quench``'s for that start, graph and order.  A shape whose
    job does not fit the workgroup's LDS raises ValueError: ``quench`` is the
    path for it.

    Returns a dict: ``mag`` float64 (R, K), ``flipped`` int64 (R, K),
    ``consensus`` bool [R] (of the input), ``best`` int64 [R] (the k with the
    smallest sum of spins, the smallest k on ties), ``conf_best`` (shape, kind
    and dtype of the input), ``mag_best`` float64 [R], ``state_best`` (device
    tensor int64 (R, ceil(n/64)): node-packed ``conf_best``, padding bits 0)
    and, with ``keep_all``, ``conf`` int8 (R, K, n).  numpy in -> numpy out,
    tensor in -> tensors on the input's device.  The input is never written;
    starts without consensus come back unchanged in every restart."""
    return _quench_jobs("quench_restarts", graph, s, p, c, restarts, orders, seed, keep_all, kernel, validate)


def quench_exchange(graph, s, p, c, restarts=1, orders=None, seed=None, max_passes=8, keep_all=False, kernel=None,
                    validate=True):
    """``quench_restarts`` with the (1, 2) exchange descent behind every job's
    pass: the move that leaves a single-flip local minimum downwards.

    After its quench pass a job walks its order again, up to ``max_passes``
    times: every -1 node j in turn becomes +1 (consensus is kept), the +1
    nodes are tried for removal in the job's order, and the add stays when two
    or more of them dropped (a net loss of at least one +1 spin); otherwise
    the state is as it was.  The passes end with the first one that commits
    nothing.  The result is again a single-flip local minimum, never heavier
    than the pass's, and equal, bit for bit, to the walk that tries every +1
    node (include/mjx.h has the definition, DESIGN.md why the kernel may try
    only the nodes near the add).

    Inputs, orders / ``seed`` rule, graph forms and refusals as
    ``quench_restarts``; p + c - 1 <= 3 and ``max_passes`` >= 1.  Returns
    ``quench_restarts``'s dict (``mag``, ``flipped`` (of the quench pass),
    ``best``, ``conf_best``, ... describe the results after the descent) plus,
    all (R, K): ``mag_quench`` float64 (sum(s)/n after the quench pass alone),
    ``exchanges`` int64 (adds that stayed), ``passes`` int64 (walked; 0 without
    consensus) and ``converged`` bool (the last pass committed nothing)."""
    return _quench_jobs("quench_exchange", graph, s, p, c, restarts, orders, seed, keep_all, kernel, validate,
                        exchange=True, max_passes=max_passes)


ANNEAL_BETA = (1.5, 6.0)     # quench_anneal's ``beta`` when neither beta nor thresholds is given


def anneal_thresholds(beta):
    """Inverse temperatures -> the uint32 accept thresholds of ``quench_anneal``:
    min(floor(exp(-beta) * 2^32), 2^32 - 1) in float64, so an add whose 32-bit
    word lies below the threshold is accepted with probability e^{-beta} (to
    2^-32).  beta = 0 gives 2^32 - 1, ``inf`` gives 0; a negative or NaN beta
    is refused.  Host only."""
    b = np.atleast_1d(np.asarray(beta, dtype=np.float64))
    if b.ndim != 1 or np.isnan(b).any() or (b < 0).any():
        raise ValueError("beta must be a vector of inverse temperatures >= 0")
    return np.minimum(np.floor(np.exp(-b) * 4294967296.0), 4294967295.0).astype(np.uint32)


def _check_anneal(sweeps, beta, thresholds, anneal_seed):
    """Host only -> (uint32 numpy thresholds [sweeps], seed in 0 .. 2^64 - 1)."""
    if not isinstance(sweeps, (int, np.integer)) or isinstance(sweeps, bool) or not 0 <= sweeps < 2 ** 31:
        raise ValueError(f"sweeps must be an integer in 0 .. 2^31 - 1, got {sweeps!r}")
    U = int(sweeps)
    if thresholds is not None:
        if beta is not None:
            raise ValueError("give beta or thresholds, not both")
        thr = np.asarray(thresholds.cpu() if isinstance(thresholds, torch.Tensor) else thresholds)
        if thr.shape != (U,) or not np.issubdtype(thr.dtype, np.integer) or \
                (U and (int(thr.min()) < 0 or int(thr.max()) > 0xFFFFFFFF)):
            raise ValueError(f"thresholds must be {U} integers in 0 .. 2^32 - 1, one per sweep")
        thr = thr.astype(np.uint32)
    else:
        b = np.asarray(ANNEAL_BETA if beta is None else beta, dtype=np.float64)
        if b.shape == (2,) and U != 2:                      # U = 2: the pair and the array are the same thing
            if not np.isfinite(b).all():
                raise ValueError("beta as a pair (first, last) must be finite: np.linspace(first, last, sweeps)")
            b = np.linspace(b[0], b[1], U)
        elif b.shape != (U,):
            raise ValueError(f"beta must be a pair (first, last) or an array of sweeps = {U} values")
        thr = anneal_thresholds(b) if U else np.zeros(0, np.uint32)
    if not isinstance(anneal_seed, (int, np.integer)) or isinstance(anneal_seed, bool) or \
            not 0 <= int(anneal_seed) < 2 ** 64:
        raise ValueError(f"anneal_seed must be an integer in 0 .. 2^64 - 1, got {anneal_seed!r}")
    return np.ascontiguousarray(thr), int(anneal_seed)


def quench_anneal(graph, s, p, c, sweeps, beta=None, thresholds=None, restarts=1, orders=None, seed=None,
                  anneal_seed=0, trace=False, keep_all=False, validate=True):
    """``quench_restarts`` with a Metropolis walk inside the consensus set behind
    every job's pass: simulated annealing on the weight that never leaves
    consensus.

    After its quench pass a job makes ``sweeps`` sweeps of n proposals.  A
    proposal draws a node (Philox, keyed by ``anneal_seed``, counter (proposal,
    sweep, start r, restart k), so a job's stream does not depend on R or K):
    a +1 node is dropped when consensus survives (always: it lowers the
    weight), a -1 node is added with probability e^{-beta} of the sweep (an add
    cannot leave consensus).  The lightest state seen at a sweep end is kept,
    and the job closes with a quench pass from it, so the result is a consensus
    single-flip local minimum and never heavier than ``quench_restarts``' on
    the same job; ``sweeps = 0`` is exactly ``quench_restarts``.  include/mjx.h
    has the definition; results are integer-exact functions of the inputs.

    ``beta``: a pair (first, last), meaning ``np.linspace(first, last,
    sweeps)``, or an array of ``sweeps`` inverse temperatures >= 0 (``inf``:
    no add; the pair must be finite, ``np.linspace`` has to reach its end);
    default ``None`` = (1.5, 6.0), which comes from CPU runs at n <= 96 and has
    NOT been tuned at n = 1e4.  ``thresholds``: instead of ``beta``, the uint32
    accept thresholds themselves (``anneal_thresholds``); giving both raises
    ValueError.  Inputs, orders / ``seed`` rule (``seed`` is the ORDER seed),
    graph forms and refusals as ``quench_restarts``; p + c - 1 <= 6.

    Returns ``quench_restarts``' dict (``mag``, ``best``, ``conf_best``, ...
    describe the final states; ``flipped`` the first pass) plus, all (R, K):
    ``mag_quench`` float64 (sum(s)/n after the first pass), ``mag_best_sweep``
    float64 (of the lightest sweep end, before the closing pass),
    ``best_sweep`` int64 (0: no sweep end beat the first pass), ``adds``,
    ``drops``, ``refused`` int64, and with ``trace=True`` ``trace`` int32
    (R, K, sweeps), the +1 spins after every sweep."""
    thr, aseed = _check_anneal(sweeps, beta, thresholds, anneal_seed)
    return _quench_jobs("quench_anneal", graph, s, p, c, restarts, orders, seed, keep_all, None, validate,
                        anneal=(thr, aseed, bool(trace)))
