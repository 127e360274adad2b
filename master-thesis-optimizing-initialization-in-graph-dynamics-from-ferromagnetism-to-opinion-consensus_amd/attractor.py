"""Run the majority dynamics to its attractor, per replica.

Synchronous majority dynamics with always-stay ties on an undirected graph end
in a fixed point or a 2-cycle (Goles & Olivos 1980).  With the trajectory
s(0) = s0, s(t+1) = onestep_majority(s(t)) a replica has

    p = min{t >= 0 : s(t+2) = s(t)}      (transient length)
    c = 1 if s(p+1) = s(p) else 2        (cycle length)
    sum_att = (sum s(p), sum s(p+1))     (both n at +1 consensus)

-- the (p, c) that SA, HPR and BDCM fix in advance, measured.  A replica with
p > t_max reports p = -1, c = 0.

The sweeps are the tracked replica-packed kernels (mjx_sweep_track_ell_rp /
mjx_sweep_track_csr_rp): beside the new state and its fused +1 counts they OR,
per replica, "some node changed against s(t)" and "... against s(t-1)" into two
flag words per 64 replicas; mjx_attractor_record turns them into p, c and
sum_att on the device.  The host reads one counter per chunk of sweeps.

Not covered: the node-packed layout, the degree-class ELL (a CSR graph runs on
its row_ptr/col rows here) and a graph per replica.
"""
import numpy as np
import torch

from . import _device, _lib
from .dynamics import as_graph, pack, popcount


def _sweep_track(g, words, s_in, s_prev, s_out, counts, diff, st):
    if g.kind == "ell":
        _lib.call("mjx_sweep_track_ell_rp", _device.ptr(g.adj), g.n, g.d, int(words), _device.ptr(s_in),
                  _device.ptr(s_prev), _device.ptr(s_out), _device.ptr(counts), _device.ptr(diff), st)
    else:
        _lib.call("mjx_sweep_track_csr_rp", _device.ptr(g.row_ptr), _device.ptr(g.col) if g.nnz else None,
                  _device.ptr(g.order), g.n, int(words), _device.ptr(s_in), _device.ptr(s_prev),
                  _device.ptr(s_out), _device.ptr(counts), _device.ptr(diff), st)


def _attractor_packed(g, bits, R, words, t_max, chunk):
    """Device loop on packed spins: ``bits`` (never written) is s(0).  Returns
    device tensors p, c (int32 [R]), sum_att (int64 [R, 2]), the number of
    sweeps made and the packed s(t_end)."""
    if t_max < 0 or chunk < 1:
        raise ValueError("t_max >= 0 and chunk >= 1")
    n, W, dev = g.n, int(words), bits.device
    if bits.numel() != n * W:
        raise ValueError(f"packed spins hold {bits.numel()} words, n * words = {n * W}")
    if not 0 < R <= 64 * W:
        raise ValueError("0 < R <= 64 * words")
    st = _device.stream_handle()
    p = torch.full((R,), -1, dtype=torch.int32, device=dev)
    c = torch.zeros(R, dtype=torch.int32, device=dev)
    sum_att = torch.zeros((R, 2), dtype=torch.int64, device=dev)
    unsettled = torch.full((1,), R, dtype=torch.int64, device=dev)
    # three state buffers: the caller's s(0) and a ping-pong pair.  Sweep k
    # reads s(k-1), compares with s(k-2) and, from k = 3 on, writes s(k) over it
    pair = (torch.empty_like(bits), torch.empty_like(bits))
    cnt_km2 = None
    cnt_km1 = popcount(bits, n, words=W)                 # +1 counts of s(0)
    diff_prev = None
    src, prev, k, last = bits, None, 0, t_max + 2
    while k < last:
        m = min(chunk, last - k)
        cnts = torch.zeros((m, 64 * W), dtype=torch.int64, device=dev)
        diffs = torch.zeros((m, 2 * W), dtype=torch.int64, device=dev)
        for i in range(m):
            k += 1
            dst = pair[k & 1]
            _sweep_track(g, W, src, prev, dst, cnts[i], diffs[i], st)
            if k >= 2:
                _lib.call("mjx_attractor_record", n, R, k, _device.ptr(diffs[i]), _device.ptr(diff_prev),
                          _device.ptr(cnt_km2), _device.ptr(cnt_km1), _device.ptr(p), _device.ptr(c),
                          _device.ptr(sum_att), _device.ptr(unsettled), st)
            cnt_km2, cnt_km1, diff_prev = cnt_km1, cnts[i], diffs[i]
            prev, src = src, dst
        if int(unsettled.item()) == 0:                   # the one host read per chunk
            break
    return p, c, sum_att, k, src


def attractor(graph, s0, t_max=4096, chunk=16, words=None):
    """Attractor of every replica of ``s0`` on ``graph``.

    graph: an ELL or CSR ``Graph``, or an (n, d) neighbour array.
    s0: +-1 spins (n,) or (R, n); or, with ``words``, replica-packed bits
    (n * words int64, 64 * words replicas, as ``pack`` / ``random_spins``
    return them).  The input is never written.

    Runs chunks of ``chunk`` tracked sweeps and stops at the first chunk
    boundary where every replica has settled, or after t_max + 2 sweeps.
    Returns a dict: ``p``, ``c`` (int64 [R]; R = 1 for an (n,) input),
    ``sum_att`` (int64 [R, 2]), ``t_end`` (sweeps made), ``state`` = the packed
    s(t_end) (device tensor of n * ``words`` int64) and ``words``.  numpy in ->
    numpy out, tensor in -> tensors on the input's device (``state`` stays a
    device tensor either way: ``unpack(state, n, R)`` opens it).
    """
    g = as_graph(graph)
    if words is not None:
        bits = _device.to_device(s0, torch.int64).reshape(-1)
        W, R = int(words), 64 * int(words)
    else:
        s = _device.to_device(s0)
        if s.dim() == 1:
            s = s[None, :]
        if s.dim() != 2 or s.shape[1] != g.n:
            raise ValueError(f"spins must be (n,) or (R, n) with n = {g.n}")
        R = s.shape[0]
        W = _device.words_for(R)
        bits = pack(s)
    p, c, sum_att, t_end, state = _attractor_packed(g, bits, R, W, int(t_max), int(chunk))
    out = {"p": p.to(torch.int64), "c": c.to(torch.int64), "sum_att": sum_att}
    if isinstance(s0, torch.Tensor):
        out = {k: v.to(s0.device) for k, v in out.items()}
    else:
        out = {k: v.cpu().numpy() for k, v in out.items()}
    out["t_end"] = t_end
    out["state"] = state
    out["words"] = W
    return out


def random_spins(n, R, m_init, seed):
    """Replica-packed random starts: replica r's spins are independent, +1 with
    probability (1 + m_init[r]) / 2 (``m_init`` a scalar or of length R).

    Spin (v, r) is a pure function of (seed, v, r) -- Philox-4x32-10 of counter
    (v, r >> 2), key = seed, word r & 3, compared with floor(prob * 2^32) -- so
    a replica gets the same spins whatever R is.  Returns the packed bits
    (device int64, n * ceil(R / 64)); padding replicas are 0."""
    dev = _device.require_gpu()
    n, R = int(n), int(R)
    prob = (1.0 + np.broadcast_to(np.asarray(m_init, dtype=np.float64), (R,))) / 2.0
    if not np.all((prob >= 0.0) & (prob <= 1.0)):
        raise ValueError("m_init must lie in [-1, 1]")
    prob_d = torch.from_numpy(np.ascontiguousarray(prob)).to(dev)
    bits = torch.empty(n * _device.words_for(R), dtype=torch.int64, device=dev)
    _lib.call("mjx_random_spins_rp", n, R, int(seed) & 0xFFFFFFFFFFFFFFFF, _device.ptr(prob_d), _device.ptr(bits),
              _device.stream_handle())
    return bits


def consensus_curve(graph, m_inits, replicas, seed, t_max=4096, chunk=16, batch=None):
    """Random-initialisation baseline: for every m_init, ``replicas`` random
    starts at that magnetisation run to their attractors.

    Layout: replica ``j * replicas + i`` of the batch is start i of
    ``m_inits[j]``, drawn by ``random_spins(n, len(m_inits) * replicas,
    repeat(m_inits, replicas), seed)`` -- all m_inits run as one replica-packed
    batch.  ``batch`` (m_inits per batch; None = all of them) splits a run whose
    three state buffers would not fit in device memory: the batch that starts
    at ``m_inits[j0]`` is laid out the same way and drawn with ``seed + j0``.
    Every array of the result is reshaped to (len(m_inits), replicas).

    Returns a dict: ``m_init`` (float64 [M]); integer counts per m_init
    ``consensus`` (attractor all +1), ``c1``, ``c2``, ``unsettled``; and the
    arrays ``p`` [M, replicas], ``c`` [M, replicas], ``sum_att``
    [M, replicas, 2] and ``init_plus`` [M, replicas] (the realised number of +1
    spins of each start)."""
    g = as_graph(graph)
    m_inits = np.atleast_1d(np.asarray(m_inits, dtype=np.float64))
    M, K, n = m_inits.shape[0], int(replicas), g.n
    if K < 1 or M < 1:
        raise ValueError("replicas >= 1 and at least one m_init")
    group = M if batch is None else max(1, int(batch))
    p = np.empty((M, K), np.int64)
    c = np.empty((M, K), np.int64)
    sum_att = np.empty((M, K, 2), np.int64)
    init_plus = np.empty((M, K), np.int64)
    for j0 in range(0, M, group):
        j1 = min(M, j0 + group)
        R = (j1 - j0) * K
        W = _device.words_for(R)
        bits = random_spins(n, R, np.repeat(m_inits[j0:j1], K), int(seed) + j0)
        init_plus[j0:j1] = popcount(bits, n, words=W)[:R].cpu().numpy().reshape(j1 - j0, K)
        pd, cd, sd, _, _ = _attractor_packed(g, bits, R, W, int(t_max), int(chunk))
        p[j0:j1] = pd.cpu().numpy().reshape(j1 - j0, K)
        c[j0:j1] = cd.cpu().numpy().reshape(j1 - j0, K)
        sum_att[j0:j1] = sd.cpu().numpy().reshape(j1 - j0, K, 2)
    return {"m_init": m_inits,
            "consensus": ((c == 1) & (sum_att[..., 0] == n)).sum(axis=1).astype(np.int64),
            "c1": (c == 1).sum(axis=1).astype(np.int64), "c2": (c == 2).sum(axis=1).astype(np.int64),
            "unsettled": (p < 0).sum(axis=1).astype(np.int64),
            "p": p, "c": c, "sum_att": sum_att, "init_plus": init_plus}
