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
zero-temperature clean-up after them.

Not covered: an order per replica, a graph per replica inside one call, the
node-packed layout, several devices.  There is no CPU fallback.
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
    if o.size and (o.min() < 0 or o.max() >= n or np.bincount(o, minlength=n).max() != 1):
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


def _packed_input(g, s, words):
    """-> (bits, R, W, ndim of the +-1 input or None for packed input)."""
    if words is not None:
        bits = _device.to_device(s, torch.int64).reshape(-1)
        W = int(words)
        if W < 1 or bits.numel() != g.n * W:
            raise ValueError(f"packed spins hold {bits.numel()} words, n * words = {g.n * W}")
        return bits, 64 * W, W, None
    t = _device.to_device(s)
    ndim = t.dim()
    if ndim == 1:
        t = t[None, :]
    if t.dim() != 2 or t.shape[1] != g.n:
        raise ValueError(f"spins must be (n,) or (R, n) with n = {g.n}")
    if t.dtype not in (torch.int8, torch.int32, torch.int64):
        t = t.to(torch.int64)
    R = t.shape[0]
    return pack(t.contiguous()), R, _device.words_for(R), ndim


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


def _graph_args(g):
    if g.kind == "ell":
        return "ell", (_device.ptr(g.adj) if g.d else None, g.n, g.d)
    return "csr", (_device.ptr(g.row_ptr), _device.ptr(g.col) if g.nnz else None, g.n)


def _scratch(nbytes, what, T, lds_entries, dev):
    if nbytes < 0 or _lib.load().mjx_quench_lds(T, lds_entries) < 0:
        raise ValueError(f"{what}: lds_entries = {lds_entries} does not fit the workgroup's LDS at p + c - 1 = {T}")
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device=dev)


def _check_overflow(scratch, what):
    if int(scratch[0].item()):
        raise _lib.MjxError(f"{what}: a light-cone list outgrew the ball bound of the graph")


def _flip_gains_packed(g, levels, R, W, p, c, T, caps, lds_entries, gain):
    """Device call on cached levels -> (removable, consensus uint8 [R], gain int32 (n, 64 W) or None)."""
    dev = levels[0].device
    lib = _lib.load()
    scratch = _scratch(lib.mjx_flip_gain_scratch_bytes(g.n, R, T, caps, lds_entries), "flip_gains", T, lds_entries, dev)
    lv = (ctypes.c_void_p * (T + 1))(*[t.data_ptr() for t in levels])
    removable = torch.empty(g.n * W, dtype=torch.int64, device=dev)
    consensus = torch.empty(R, dtype=torch.uint8, device=dev)
    gains = torch.empty((g.n, 64 * W), dtype=torch.int32, device=dev) if gain else None
    kind, ga = _graph_args(g)
    _lib.call(f"mjx_flip_gain_{kind}_rp", *ga, R, p, c, lv, caps, lds_entries, _device.ptr(scratch),
              scratch.numel() * 8, _device.ptr(removable), _device.ptr(consensus), _device.ptr(gains),
              _device.stream_handle())
    _check_overflow(scratch, "flip_gains")
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


def _quench_prepare(g, bits, R, W, p, c, T, order, lds_entries):
    """The parallel part: copies of the levels, the initial removable mask and
    the candidate lists -> (levels, caps, cand, cand_ptr)."""
    caps = _caps(g, T)
    levels = _levels(g, bits, W, T, copy=True)
    removable, _, _ = _flip_gains_packed(g, levels, R, W, p, c, T, caps, lds_entries, False)
    cand, cand_ptr = _candidates(removable, g.n, W, order)
    return levels, caps, cand, cand_ptr


def _quench_pass(g, levels, R, W, p, c, T, caps, cand, cand_ptr, lds_entries):
    """The sequential part, one workgroup per word column; ``levels`` are
    updated in place -> (consensus uint8 [R], flipped int64 [R])."""
    dev = levels[0].device
    lib = _lib.load()
    scratch = _scratch(lib.mjx_quench_scratch_bytes(R, T, caps, lds_entries), "quench", T, lds_entries, dev)
    lv = (ctypes.c_void_p * (T + 1))(*[t.data_ptr() for t in levels])
    consensus = torch.empty(R, dtype=torch.uint8, device=dev)
    flipped = torch.zeros(64 * W, dtype=torch.int64, device=dev)
    kind, ga = _graph_args(g)
    _lib.call(f"mjx_quench_{kind}_rp", *ga, R, p, c, lv, caps, lds_entries, _device.ptr(scratch), scratch.numel() * 8,
              _device.ptr(cand) if cand.numel() else None, _device.ptr(cand_ptr), _device.ptr(consensus),
              _device.ptr(flipped), _device.stream_handle())
    _check_overflow(scratch, "quench")
    return consensus, flipped[:R]


def _quench_packed(g, bits, R, W, p, c, T, order, lds_entries):
    """-> (state = packed result (a new tensor), consensus uint8 [R], flipped int64 [R], candidates visited)."""
    levels, caps, cand, cand_ptr = _quench_prepare(g, bits, R, W, p, c, T, order, lds_entries)
    consensus, flipped = _quench_pass(g, levels, R, W, p, c, T, caps, cand, cand_ptr, lds_entries)
    return levels[0], consensus, flipped, int(cand.numel())


def quench(graph, s, p, c, order=None, seed=None, words=None, kernel=None, validate=True):
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
    float64 [R] = sum(s)/n of the result, ``visited`` = candidates walked."""
    p, c, T = _steps(p, c)
    lds_entries = _kernel_options(kernel)
    order = _check_order(order, seed, _host_n(graph, s, words))
    g = as_graph(graph)
    if order is not None and order.shape[0] != g.n:
        raise ValueError(f"order must be a permutation of 0..{g.n - 1}")
    if validate:
        _check_symmetric(g)
    bits, R, W, ndim = _packed_input(g, s, words)
    state, consensus, flipped, visited = _quench_packed(g, bits, R, W, p, c, T, order, lds_entries)
    plus = popcount(state, g.n, words=W)[:R]
    # sum(s) / n as numpy divides two integers (a device division may multiply by 1/n)
    mag = torch.from_numpy((2 * plus.cpu().numpy() - g.n) / g.n)
    out = {"flipped": _like(flipped, s), "consensus": _like(consensus.to(torch.bool), s), "mag": _like(mag, s),
           "visited": visited, "state": state, "words": W}
    if words is not None:
        return out
    conf = unpack(state, g.n, R)
    if ndim == 1:
        conf = conf[0]
    if isinstance(s, torch.Tensor):
        out["conf"] = conf.to(device=s.device, dtype=s.dtype)
    else:
        out["conf"] = conf.cpu().numpy().astype(np.asarray(s).dtype, copy=False)
    return out
