"""Simulated annealing on irregular graphs (Erdos-Renyi / any CSR adjacency).

``SAReplicasER`` runs R independent replicas of the reference's SA loop
(code/SA_RRG.py:65-85), bit-packed 64 per word as ``SAReplicas`` does, on ONE
graph given as CSR, with ``s_endstate`` replaced by the notebook's ER rule
(code/ER_BDCM_entropy.ipynb nb:113-123: sign(2S+s), a degree-0 node keeps its
spin).  Replica r is bit-identical to

    np.random.seed(seeds[r])
    s = 2*np.random.binomial(n=1, p=0.5, size=[n]) - 1
    ... while(m_final<1): ...            # randint(0, n), rand(), delta_H, schedule

with ``schedule_constants(n)`` of the node count of the graph as passed.  Row
entries count with multiplicity (self-loops, doubled edges).  On the CSR of a
d-regular neighbour array the trajectories equal ``SAReplicas``'.

The adjacency must be SYMMETRIC as a multiset of directed entries (v in row(u)
as often as u in row(v)): the light cone finds the nodes that read a changed
node in that node's own row.  The constructor checks it once on the device
(``validate=False`` skips the check for giant graphs).

Modes, bit-identical to each other:

* ``"lightcone"``: one persistent kernel per call (mjx_sa_csr_lightcone_steps);
  per-level changed / candidate lists in LDS up to ``lds_entries`` per replica
  and level, beyond that in an HBM spill area sized by the graph's ball bound
  (mjx_sa_csr_ball_bound).  Nothing is truncated.
* ``"rollout"``: per step a proposal, a full CSR rollout with the fused +1
  count and the Metropolis test (mjx_sa_csr_steps).
"""
import hashlib
import time

import numpy as np
import torch

from . import _device, _lib
from .dynamics import unpack
from .graph import Graph, erdos_renyi
from .sa import PAR_A, PAR_B, schedule_constants


def _as_csr_graph(graph):
    if isinstance(graph, Graph):
        g = graph
    elif isinstance(graph, (tuple, list)) and len(graph) == 2:
        rp, col = graph
        if isinstance(rp, torch.Tensor) and rp.is_cuda and isinstance(col, torch.Tensor) and col.is_cuda:
            g = Graph.csr_device(rp, col)
        else:
            g = Graph.csr(rp, col)
    else:
        raise ValueError("SAReplicasER needs a CSR Graph or a (row_ptr, col) pair")
    if g.kind != "csr":
        raise ValueError("SAReplicasER runs on CSR graphs (Graph.csr); random regular ELL graphs go to SAReplicas")
    return g


def csr_is_symmetric(g):
    """True when the CSR adjacency is symmetric as a multiset of directed
    entries: the sorted keys of (u, v) equal the sorted keys of (v, u)."""
    n = g.n
    if g.nnz == 0:
        return True
    deg = g.row_ptr[1:] - g.row_ptr[:-1]
    u = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=deg.device), deg)
    v = g.col.to(torch.int64)
    if int(v.min().item()) < 0 or int(v.max().item()) >= n:
        raise ValueError("CSR column index out of range")
    a = torch.sort(u * n + v).values
    b = torch.sort(v * n + u).values
    return bool(torch.equal(a, b))


class SAReplicasER:
    """R bit-packed SA replicas on one CSR graph (device resident); the
    surface of ``SAReplicas``."""

    def __init__(self, graph, p, c, seeds, par_a=PAR_A, par_b=PAR_B, a0=None, b0=None, mode="auto", mt_state=None,
                 kernel=None, scratch_limit=1 << 30, validate=True):
        """``graph``: a CSR ``Graph`` or ``(row_ptr, col)``.  ``mt_state`` =
        (mt uint32 (R, 624), idx int32 (R,)): continue these MT19937 streams
        instead of seeding.  ``mode="auto"``: the light cone when 1 <= p+c-1
        <= 6 and its spill area fits ``scratch_limit`` bytes, else rollout.
        ``kernel``: ``{"lds_entries": k}`` list entries per replica and level
        kept in LDS (tests use a small k to force the spill path) and
        ``{"split": w}`` waves per word column (1, 2, ..., 64; default: enough to
        fill the device); the results never depend on either."""
        seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
        if seeds.size == 0 or seeds.min() < 0 or seeds.max() > 0xFFFFFFFF:
            raise ValueError("seeds must be in [0, 2**32)")  # np.random.seed's range
        dev = _device.require_gpu()
        self.graph = g = _as_csr_graph(graph)
        self.R = R = int(seeds.size)
        self.n = n = g.n
        self.p, self.c = int(p), int(c)
        if n < 2:
            raise ValueError("n must be >= 2")
        if self.p < 0 or self.c < 0 or self.p + self.c < 1:
            raise ValueError("need p, c >= 0 and p + c >= 1")
        if validate and not csr_is_symmetric(g):
            raise ValueError("the CSR adjacency is not symmetric (v in row(u) as often as u in row(v)): "
                             "the light cone relies on it")
        self.W = W = _device.words_for(R)
        a0d, b0d, self.a_cap, self.b_cap, self.t_cap = schedule_constants(n)
        self.a0 = a0d if a0 is None else float(a0)
        self.b0 = b0d if b0 is None else float(b0)
        self.par_a, self.par_b = float(par_a), float(par_b)
        self.t_cap = min(self.t_cap, 2 ** 63 - 1)
        kernel = dict(kernel or {})
        self.lds_entries = int(kernel.pop("lds_entries", 0) or 0)
        split = int(kernel.pop("split", 0) or 0)
        if kernel:
            raise ValueError(f"unknown kernel options {sorted(kernel)}")
        if self.lds_entries < 0 or split < 0 or (split and (split > 64 or 64 % split)):
            raise ValueError("lds_entries must be >= 0 and split a divisor of 64")
        T = self.p + self.c - 1
        lib = _lib.load()
        # mode: the caps of the ball bound size the light cone's spill area
        self.caps = None
        self._caps_c = None
        spill_bytes = -1
        if mode not in ("auto", "lightcone", "rollout"):
            raise ValueError(f"unknown SA mode {mode!r}")
        if mode != "rollout" and 1 <= T <= 6 and lib.mjx_sa_csr_lightcone_lds(T, self.lds_entries) > 0:
            self.caps = self.ball_bound(g, T)
            self._caps_c = (_lib.c_i64 * (T + 1))(*self.caps)
            spill_bytes = int(lib.mjx_sa_csr_lightcone_scratch_bytes(R, T, self._caps_c, self.lds_entries))
        fits = 0 <= spill_bytes <= int(scratch_limit)
        if mode == "auto":
            mode = "lightcone" if fits else "rollout"
        if mode == "lightcone" and not fits:
            raise ValueError(f"light-cone SA does not fit: p+c-1={T} (1..6), lds_entries={self.lds_entries}, spill "
                             f"area {spill_bytes} B against scratch_limit={int(scratch_limit)} B")
        self.mode = mode
        i64 = torch.int64
        self.s = torch.zeros(n * W, dtype=i64, device=dev)
        self.tmp1 = torch.empty_like(self.s)
        self.tmp2 = torch.empty_like(self.s)
        self.seeds = torch.from_numpy(seeds.astype(np.uint32).view(np.int32)).to(dev)
        self.mt = torch.empty(R * 624, dtype=torch.int32, device=dev)
        self.mt_idx = torch.empty(R, dtype=torch.int32, device=dev)
        self.a = torch.empty(R, dtype=torch.float64, device=dev)
        self.b = torch.empty(R, dtype=torch.float64, device=dev)
        self.t = torch.zeros(R, dtype=i64, device=dev)
        self.sum_end = torch.zeros(R, dtype=i64, device=dev)
        self.done = torch.zeros(R, dtype=torch.int32, device=dev)
        self.prop_i = torch.empty(R, dtype=torch.int32, device=dev)
        self.prop_s = torch.empty(R, dtype=torch.int8, device=dev)
        self.prop_u = torch.empty(R, dtype=torch.float64, device=dev)
        self.cnt = torch.zeros(R, dtype=i64, device=dev)
        self.ties = torch.zeros(R, dtype=torch.int32, device=dev)
        self._state = _lib.MjxSaState()
        for f in ("mt", "mt_idx", "a", "b", "t", "sum_end", "done", "prop_i", "prop_s", "prop_u", "cnt"):
            setattr(self._state, f, getattr(self, f).data_ptr())
        self._state.tr_tie = self.ties.data_ptr()
        self._state.opt_split = split
        self._col = _device.ptr(g.col) if g.nnz else None
        tmp2 = _device.ptr(self.tmp2) if T >= 2 else None
        if mt_state is None:
            _lib.call("mjx_sa_csr_init", _device.ptr(g.row_ptr), self._col, n, self.p, self.c, R,
                      _device.ptr(self.seeds), self.a0, self.b0, _device.ptr(self.s), _device.ptr(self.tmp1), tmp2,
                      _lib.ctypes.byref(self._state), _device.stream_handle())
        else:
            mt_in = np.ascontiguousarray(np.asarray(mt_state[0], dtype=np.uint32).reshape(R, 624))
            idx_in = np.ascontiguousarray(np.asarray(mt_state[1], dtype=np.int32).reshape(R))
            if idx_in.min() < 0 or idx_in.max() > 624:
                raise ValueError("MT19937 word index must be in [0, 624]")
            mt_d = torch.from_numpy(mt_in.view(np.int32)).to(dev)
            idx_d = torch.from_numpy(idx_in).to(dev)
            _lib.call("mjx_sa_csr_init_mt", _device.ptr(g.row_ptr), self._col, n, self.p, self.c, R,
                      _device.ptr(mt_d), _device.ptr(idx_d), self.a0, self.b0, _device.ptr(self.s),
                      _device.ptr(self.tmp1), tmp2, _lib.ctypes.byref(self._state), _device.stream_handle())
            torch.cuda.current_stream().synchronize()       # mt_d / idx_d are freed on return
        self._levels = None
        self.spill = None
        self.spill_bytes = 0
        if mode == "lightcone":
            # levels s_1..s_T = onestep^t(s); the rollout ping-pong buffers are reused
            self._levels = [self.tmp1, self.tmp2][:T] + [torch.empty_like(self.s) for _ in range(T - 2)]
            self._lvl = (_lib.ctypes.c_void_p * T)(*[t.data_ptr() for t in self._levels])
            self.spill_bytes = spill_bytes
            if spill_bytes:
                self.spill = torch.empty(spill_bytes // 4, dtype=torch.int32, device=dev)
            self._build_levels()

    @staticmethod
    def ball_bound(graph, T):
        """caps[t] = min(n, max_v B_t(v)), t = 0..T, B_t(v) the number of walks of
        length <= t from v (mjx_sa_csr_ball_bound): the bound of the candidate
        and changed sets of level t of any proposal."""
        g = _as_csr_graph(graph)
        lib = _lib.load()
        work = torch.empty(int(lib.mjx_sa_csr_ball_work_bytes(g.n)), dtype=torch.uint8, device=g.row_ptr.device)
        out = (_lib.c_i64 * (int(T) + 1))()
        _lib.call("mjx_sa_csr_ball_bound", _device.ptr(g.row_ptr), _device.ptr(g.col) if g.nnz else None, g.n, int(T),
                  _device.ptr(work), out, _device.stream_handle())
        return [int(x) for x in out]

    def _build_levels(self):
        _lib.call("mjx_sa_csr_lightcone_prepare", _device.ptr(self.graph.row_ptr), self._col, self.n, self.p, self.c,
                  self.R, _device.ptr(self.s), self._lvl, _device.stream_handle())

    # -- checkpoint / resume ------------------------------------------------
    _CKPT_STATE = ("s", "mt", "mt_idx", "a", "b", "t", "sum_end", "done", "ties")

    def graph_digest(self):
        """SHA-256 of the graph this run reads: n, row_ptr (int64) and col (int32)."""
        h = hashlib.sha256()
        h.update(np.array([self.n, self.graph.nnz], dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(self.graph.row_ptr.cpu().numpy().astype(np.int64)).tobytes())
        h.update(np.ascontiguousarray(self.graph.col.cpu().numpy().astype(np.int32)).tobytes())
        return h.hexdigest()

    def checkpoint(self):
        """Everything a resumed run needs, as host arrays (the configuration,
        every replica's MT19937 stream exactly, a, b, t, sum(s_end), the done
        flags, the parameters and the graph's digest).  ``resume`` continues it
        bit for bit: proposals are always drawn in the step, never ahead."""
        torch.cuda.current_stream().synchronize()
        out = {k: getattr(self, k).cpu().numpy().copy() for k in self._CKPT_STATE}
        out["params"] = np.array([self.n, self.graph.nnz, self.p, self.c, self.R], dtype=np.int64)
        out["schedule"] = np.array([self.par_a, self.par_b, self.a0, self.b0, self.a_cap, self.b_cap],
                                   dtype=np.float64)
        out["t_cap"] = np.array(self.t_cap, dtype=np.int64)
        out["graph_sha256"] = np.array(self.graph_digest())
        return out

    def save_checkpoint(self, path):
        np.savez(path, **self.checkpoint())

    @classmethod
    def resume(cls, graph, ckpt, mode="auto", kernel=None, scratch_limit=1 << 30, validate=True):
        """A run continued from ``checkpoint()`` (a dict, or the path of a
        ``save_checkpoint`` file) on the same graph: the same proposals,
        accepts and final state as the uninterrupted run."""
        if not isinstance(ckpt, dict):
            with np.load(ckpt, allow_pickle=False) as z:
                ckpt = {k: z[k] for k in z.files}
        n, nnz, p, c, R = (int(x) for x in ckpt["params"])
        par_a, par_b, a0, b0 = (float(x) for x in ckpt["schedule"][:4])
        g = _as_csr_graph(graph)
        if (g.n, g.nnz) != (n, nnz):
            raise ValueError(f"checkpoint of n={n}, nnz={nnz} does not fit this graph (n={g.n}, nnz={g.nnz})")
        sa = cls(g, p, c, np.zeros(R, dtype=np.int64), par_a=par_a, par_b=par_b, a0=a0, b0=b0, mode=mode,
                 kernel=kernel, scratch_limit=scratch_limit, validate=validate)
        if str(ckpt["graph_sha256"]) != sa.graph_digest():
            raise ValueError("checkpoint was taken on another graph than this one")
        a_cap, b_cap = (float(x) for x in ckpt["schedule"][4:6])
        if (a_cap, b_cap) != (sa.a_cap, sa.b_cap) or int(ckpt["t_cap"]) != int(sa.t_cap):
            raise ValueError(f"checkpoint caps a={a_cap}, b={b_cap}, t={int(ckpt['t_cap'])} differ from "
                             f"code/SA_RRG.py's for n={n} (a={sa.a_cap}, b={sa.b_cap}, t={sa.t_cap})")
        for k in cls._CKPT_STATE:
            dst = getattr(sa, k)
            src = torch.from_numpy(np.ascontiguousarray(ckpt[k])).to(dst.device)
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError(f"checkpoint field {k}: {tuple(src.shape)} {src.dtype}, expected "
                                 f"{tuple(dst.shape)} {dst.dtype}")
            dst.copy_(src)
        if sa.mode == "lightcone":
            sa._build_levels()
        torch.cuda.current_stream().synchronize()
        return sa

    # -- stepping -----------------------------------------------------------
    def steps(self, k, trace=False):
        """Advance every running replica by k proposals.  With ``trace`` the
        per-step (i, accept, sum_end, delta_H) arrays of shape (k, R) are
        returned (i = -1 / accept = -1 once a replica is done)."""
        k = int(k)
        st = self._state
        tr = None
        if trace:
            dev = self.s.device
            tr = {
                "i": torch.empty((k, self.R), dtype=torch.int32, device=dev),
                "accept": torch.empty((k, self.R), dtype=torch.int8, device=dev),
                "sum_end": torch.empty((k, self.R), dtype=torch.int64, device=dev),
                "dE": torch.empty((k, self.R), dtype=torch.float64, device=dev),
            }
            st.tr_i, st.tr_acc = tr["i"].data_ptr(), tr["accept"].data_ptr()
            st.tr_sum, st.tr_dE = tr["sum_end"].data_ptr(), tr["dE"].data_ptr()
        else:
            st.tr_i = st.tr_acc = st.tr_sum = st.tr_dE = None
        T = self.p + self.c - 1
        rp = _device.ptr(self.graph.row_ptr)
        if self.mode == "lightcone":
            _lib.call("mjx_sa_csr_lightcone_steps", rp, self._col, self.n, self.p, self.c, self.R,
                      _device.ptr(self.s), self._lvl, _lib.ctypes.byref(st), k, self.par_a, self.par_b, self.a_cap,
                      self.b_cap, int(self.t_cap), self._caps_c, self.lds_entries,
                      _device.ptr(self.spill) if self.spill is not None else None, self.spill_bytes,
                      _device.stream_handle())
        else:
            _lib.call("mjx_sa_csr_steps", rp, self._col, self.n, self.p, self.c, self.R, _device.ptr(self.s),
                      _device.ptr(self.tmp1), _device.ptr(self.tmp2) if T >= 2 else None, _lib.ctypes.byref(st), k,
                      self.par_a, self.par_b, self.a_cap, self.b_cap, int(self.t_cap), _device.stream_handle())
        st.tr_i = st.tr_acc = st.tr_sum = st.tr_dE = None
        return tr

    @property
    def levels(self):
        """The cached levels onestep^t(s), t = 1..T, as (n*W,) arrays."""
        if self.mode != "lightcone":
            raise AttributeError("levels exist in the light-cone mode only")
        return self._levels

    def all_done(self):
        return bool((self.done != 0).all().item())

    def mt_state(self):
        """Host copy (mt uint32 (R, 624), idx int32 (R,)) of every replica's
        MT19937 stream: exactly where numpy's stream would be after the same
        draws (proposals are drawn in the step in both modes)."""
        mt = self.mt.cpu().numpy().view(np.uint32).reshape(self.R, 624).copy()
        return mt, self.mt_idx.cpu().numpy().copy()

    def run(self, max_steps=None, chunk=256, max_chunk=16384, max_seconds=None):
        """Step until every replica has reached consensus or the t cap
        (``while(m_final<1)``, code/SA_RRG.py:72), or ``max_steps``, or
        ``max_seconds`` of wall time; the done flags are read once per chunk."""
        t0 = time.perf_counter()
        taken = 0
        while not self.all_done():
            k = chunk if max_steps is None else min(chunk, max_steps - taken)
            if k <= 0 or (max_seconds is not None and time.perf_counter() - t0 >= max_seconds):
                break
            self.steps(k)
            taken += k
            chunk = min(2 * chunk, max_chunk)
        return taken

    # -- results (code/SA_RRG.py:86-88) ---------------------------------------
    def conf(self):
        """(R, n) int64 +-1 current configurations."""
        return unpack(self.s, self.n, self.R)

    def results(self):
        conf = self.conf().cpu().numpy()
        return {
            "mag_reached": np.sum(conf, axis=1) / self.n,
            "num_steps": self.t.cpu().numpy().astype(np.float64),
            "conf": conf,
            "done": self.done.cpu().numpy(),
            "near_ties": self.ties.cpu().numpy(),
        }


def lightcone_stats(reset=False):
    """(proposals evaluated by the CSR light-cone step on this device since the
    last reset, those of them with a list longer than its LDS part)."""
    out = (_lib.ctypes.c_ulonglong * 2)()
    _lib.call("mjx_sa_csr_lightcone_stats", out, int(bool(reset)))
    return int(out[0]), int(out[1])


def sa_er_run(n=None, prob=None, p=1, c=1, par_a=PAR_A, par_b=PAR_B, N_stat=5, seed=0, seeds=None, graph=None,
              graph_seed=None, drop_isolated=True, max_steps=None, max_seconds=None, mode="auto"):
    """The SA experiment (code/SA_RRG.py:44-92) on one Erdos-Renyi graph.

    Graph: ``graph`` (a CSR ``Graph`` or ``(row_ptr, col)``), else G(n, prob)
    from this package's sampler seeded ``graph_seed`` (default ``seed``), with
    the isolated nodes dropped and the rest relabelled as the notebook does
    (nb:283-291) unless ``drop_isolated=False``.  All ``N_stat`` replicas run
    on that graph, replica k on its own stream ``np.random.seed(seeds[k])``
    (default ``seed + k``).

    Returns ``mag_reached, num_steps, conf`` (the reference's keys, row k =
    replica k, over the graph's nodes), ``done, near_ties, wall_s`` and the
    graph: ``row_ptr, col, n_iso`` (isolated nodes dropped by the sampler)."""
    n_iso = 0
    if graph is None:
        if n is None or prob is None:
            raise ValueError("sa_er_run needs a graph or (n, prob)")
        gs = seed if graph_seed is None else graph_seed
        if drop_isolated:
            rp, col, n_iso = erdos_renyi(int(n), float(prob), seed=gs, drop_isolated=True)
        else:
            rp, col = erdos_renyi(int(n), float(prob), seed=gs)
        graph = Graph.csr(rp, col)
    g = _as_csr_graph(graph)
    R = int(N_stat)
    if seeds is None:
        seeds = [seed + k for k in range(R)]
    seeds = list(seeds)
    if len(seeds) != R:
        raise ValueError(f"seeds: one per replica ({R}), got {len(seeds)}")
    sa = SAReplicasER(g, p, c, seeds, par_a=par_a, par_b=par_b, mode=mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sa.run(max_steps=max_steps, max_seconds=max_seconds)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    res = sa.results()
    res["wall_s"] = np.full(R, wall)
    res["row_ptr"] = g.row_ptr.cpu().numpy().astype(np.int64)
    res["col"] = g.col.cpu().numpy().astype(np.int32)
    res["n_iso"] = np.array(int(n_iso), dtype=np.int64)
    return res
