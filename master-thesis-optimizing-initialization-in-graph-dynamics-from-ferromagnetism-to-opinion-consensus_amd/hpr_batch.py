"""HPR (code/HPR_pytorch_RRG.py:224-377) on a batch of graphs in one device loop.

G d-regular graphs on n nodes are one d-regular disjoint-union graph on G n
nodes.  The update, marginals, node-step and rollout kernels of ``hpr`` run on
it unchanged -- every message row and node depends only on its own inputs -- so
the launches of one iteration carry G times the work.  What the union cannot
express by itself is added here:

  * every instance continues its own torch CPU generator on the device
    (mjx_hpr_refresh_masks_jump_batch), as ``hpr_run(seed=seeds[k])`` would;
  * the consensus test and the stop are per instance and on the device
    (mjx_hpr_batch_record): the host reads one counter per batch of iterations;
  * finished instances are retired by compaction: at a batch boundary the union
    is rebuilt from the live instances once they are few enough.

All instances walk the iteration number t in lockstep from 0, so the
reinforcement thresholds 1-(1+t)^-gamma and the decay scales of the "q" layout
are shared.  The lambda weights exp(-+lmbd/n) use the instance's n.

Layout: instance g's nodes are g n + i; its forward message rows (row r < E of
its own (2E, 4^T) matrix) are g E + r and its reverse rows (E + r) are
E_tot + g E + r with E_tot = G E, which keeps "reverse of row r is r + E_tot".

  hpr_batch_layout(edges_list, n, d, nbrs_list)   the union's index arrays (numpy only)
  HPRBatch                                        the union's device loop
  hpr_run_batch(d, n, p, c, edges_list, seeds)    hpr_run for every instance, leading dimension G
"""
import numpy as np
import torch

from . import _device, _lib
from .dynamics import rollout
from .hpr import HPRPlan, HPRState, _code, _weights, hpr_plan_indices

INT32_MAX = 2 ** 31 - 1
INT64_MAX = 2 ** 63 - 1
MAX_INSTANCES = 65535       # blockIdx.y of k_mt_refresh_jump_batch


def _union(per, n, d):
    """Union index arrays of the instances ``per`` (hpr_plan_indices tuples)."""
    G = len(per)
    E = per[0][0].shape[0]
    Et = G * E
    if G * n * d > INT32_MAX:
        # in_row / out_row / nbr are int32 on the device (row products are 64-bit in the kernels)
        raise ValueError(f"the union of {G} graphs has {G * n * d} message rows: row and node ids are int32")
    if G > MAX_INSTANCES:
        raise ValueError(f"{G} graphs in one union: the mask generator's grid holds at most {MAX_INSTANCES} instances")

    def rows(g, r):
        return np.where(r < E, g * E + r, Et + g * E + (r - E))

    return {"G": G, "n": n, "d": d, "E": E, "E_tot": Et,
            "edges": np.concatenate([p[0] + g * n for g, p in enumerate(per)]),
            "nbrs": np.concatenate([p[1] + g * n for g, p in enumerate(per)]),
            "out_row": np.concatenate([rows(g, p[2]) for g, p in enumerate(per)]),
            "in_row": np.concatenate([rows(g, p[3]) for g, p in enumerate(per)]),
            "rows": np.stack([rows(g, np.arange(2 * E, dtype=np.int64)) for g in range(G)]),
            "node_off": np.arange(G + 1, dtype=np.int64) * n}


def _instance_indices(edges_list, n, d, nbrs_list=None):
    n, d = int(n), int(d)
    edges_list = list(edges_list)
    if not edges_list:
        raise ValueError("a batch needs at least one graph")
    if nbrs_list is None:
        nbrs_list = [None] * len(edges_list)
    if len(nbrs_list) != len(edges_list):
        raise ValueError("nbrs_list must name one neighbour array per graph")
    per = []
    for g, (e, nb) in enumerate(zip(edges_list, nbrs_list)):
        e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
        if e.size and (e.min() < 0 or e.max() >= n):
            raise ValueError(f"instance {g} has node ids outside [0, {n})")
        try:
            per.append(hpr_plan_indices(e, n, d, nb))
        except ValueError as err:
            raise ValueError(f"instance {g}: {err}") from None
    return per


def hpr_batch_layout(edges_list, n, d, nbrs_list=None):
    """Index arrays of the disjoint union of G d-regular graphs on n nodes (host
    arrays only).  edges_list: G edge lists (E, 2); nbrs_list (optional): their
    (n, d) neighbour arrays (HPRPlan's ``nbrs``).  A graph that is not
    d-regular on n nodes raises ValueError, as do an empty list and a union
    whose rows do not fit the kernels' int32 index arrays.

    Returns a dict: G, n, d, E, E_tot; ``edges`` (E_tot, 2), ``nbrs`` (G n, d),
    ``out_row`` / ``in_row`` (G n, d) in union ids -- what
    HPRPlan(edges, G n, d, nbrs) computes; ``rows`` (G, 2E): the union row of
    each row of instance g's own (2E, 4^T) matrix; ``node_off`` (G+1)."""
    return _union(_instance_indices(edges_list, n, d, nbrs_list), int(n), int(d))


def _plan_of(lay):
    return HPRPlan(lay["edges"], lay["G"] * lay["n"], lay["d"],
                   indices=(lay["edges"], lay["nbrs"], lay["out_row"], lay["in_row"]))


class HPRBatch:
    """The device loop of G HPR instances on their union graph.

    chi0_list / biases0_list: per instance the (2E, 4^T) messages and (n, 2)
    biases the run starts from (reference layout); generators: per instance the
    torch CPU generator whose stream the per-iteration rand(n) continues.
    ``run`` iterates until every instance has stopped; ``results`` returns
    hpr_run's keys with leading dimension G.  ``compact``: rebuild the union
    from the live instances at a batch boundary once they number at most
    compact x the instances of the current union (0: never)."""

    MASK_WORKGROUPS = 256      # instances x chunks of the mask generator (one workgroup per CU)

    def __init__(self, d, n, p, c, edges_list, chi0_list, biases0_list, generators, dtype=torch.float32,
                 damppar=0.4, attr_value=1, lmbd_in=None, pie=0.3, gamma=0.1, TT=10000, batch=16, graph=True,
                 layout=None, compact=0.5, nbrs_list=None):
        self.n, self.d, self.p, self.c = int(n), int(d), int(p), int(c)
        self.dtype, self.TT = dtype, int(TT)
        self.k = max(2, int(batch) + int(batch) % 2)           # even: the message buffers alternate
        self.use_graph, self.compact = bool(graph), float(compact)
        self.per = _instance_indices(edges_list, n, d, nbrs_list)
        G = self.G = len(self.per)
        if not (len(chi0_list) == len(biases0_list) == len(generators) == G):
            raise ValueError(f"{G} graphs need {G} message arrays, bias arrays and generators")
        lay = _union(self.per, self.n, self.d)
        self.E = lay["E"]
        dev = _device.require_gpu()
        nc = 4 ** (self.p + self.c)
        E, Et = self.E, lay["E_tot"]
        chi0 = torch.empty((2 * Et, nc), dtype=dtype, device=dev)
        b0 = torch.empty((G * self.n, 2), dtype=dtype, device=dev)
        for g in range(G):
            ch = torch.as_tensor(chi0_list[g]).to(dtype)       # the cast hpr_run makes, then the upload
            if ch.shape != (2 * E, nc):
                raise ValueError(f"instance {g}: chi0 must be ({2 * E}, {nc}), got {tuple(ch.shape)}")
            chi0[g * E:(g + 1) * E].copy_(ch[:E])
            chi0[Et + g * E:Et + (g + 1) * E].copy_(ch[E:])
            b0[g * self.n:(g + 1) * self.n].copy_(torch.as_tensor(biases0_list[g]).to(dtype).reshape(self.n, 2))
        lmbd = 25 * self.n if lmbd_in is None else lmbd_in     # of the instance, not of the union
        self._w = _weights(lmbd, self.n)
        self.st = HPRState(_plan_of(lay), p, c, chi0, b0, dtype=dtype, damppar=damppar, attr_value=attr_value,
                           lmbd_in=lmbd, pie=pie, gamma=gamma, layout=layout)
        self.inst = np.arange(G, dtype=np.int64)               # slot of the current union -> instance
        self.done = torch.zeros(G, dtype=torch.int32, device=dev)
        self.t_stop = torch.zeros(G, dtype=torch.int64, device=dev)
        self.conf = torch.zeros((G, self.n), dtype=torch.int32, device=dev)
        self._live = torch.full((1,), G, dtype=torch.int64, device=dev)
        self._live_host = torch.empty(1, dtype=torch.int64).pin_memory()
        self._tbase = torch.zeros(1, dtype=torch.int64, device=dev)
        self._done_ev = torch.cuda.Event()
        self._gen_stream = torch.cuda.Stream(device=dev)
        self._tables = {}
        self.generators = list(generators)
        self._final = np.zeros(G, dtype=bool)                  # generator already left at its stop
        self._drawn = None
        self._attach()
        self._alloc()
        self._record(self._rolled(first=True), 0, INT64_MAX)   # :337-343, the test before the loop
        self.live = self._read_live()
        self._finish_generators(None, 0)

    # -- buffers of the current union ----------------------------------------------
    def _attach(self):
        """The generators' engines (torch's CPU MT19937: get_state() bytes 8, 16
        and 24..5016) as one (G, 624) / (G, 2) pair on the device."""
        self._gen_bytes, words, ln = [], [], []
        for g in self.generators:
            b = g.get_state().numpy()
            if b.size != 5056:
                raise _lib.MjxError(f"unexpected CPU generator state size {b.size}")
            self._gen_bytes.append(b.copy())
            words.append(b[24:24 + 624 * 8].view(np.uint64).astype(np.uint32).view(np.int32))
            ln.append([int(b[8:12].view(np.int32)[0]), int(b[16:24].view(np.uint64)[0])])
        dev = self.done.device
        self._mt = torch.from_numpy(np.stack(words)).to(dev)
        self._ln = torch.tensor(ln, dtype=torch.int32, device=dev)

    def _alloc(self):
        plan, k, dev = self.st.plan, self.k, self.done.device
        N, Gc = plan.n, len(self.inst)
        self._inst_dev = torch.from_numpy(self.inst.astype(np.int32)).to(dev)
        self._mask = torch.empty((k, N), dtype=torch.bool, device=dev)
        self._gmask = [torch.empty((k, N), dtype=torch.bool, device=dev) for _ in range(2)]
        self._gthr = [torch.empty(k, dtype=torch.float64, device=dev) for _ in range(2)]
        self._snap = [(torch.empty_like(self._mt), torch.empty_like(self._ln)) for _ in range(2)]
        self._gen_done = [torch.cuda.Event(), torch.cuda.Event()]
        self._mask_free = [torch.cuda.Event(), torch.cuda.Event()]
        self._slot = 0
        self._scales = torch.ones(k + 1, dtype=self.dtype, device=dev)
        self._pin_scales = [torch.empty(k + 1, dtype=self.dtype).pin_memory() for _ in range(2)]
        self._bits = torch.empty((N + 63) // 64, dtype=torch.int64, device=dev)
        self._rtmp = (torch.empty_like(self._bits), torch.empty_like(self._bits))
        self._counts = torch.zeros(Gc, dtype=torch.int64, device=dev)
        self._graph, self._warm = None, False
        # chunks per instance: instances x chunks near the single-stream path's 256 workgroups
        self._chunks = max(1, self.MASK_WORKGROUPS // Gc)

    def _table(self):
        key = (self.k, self._chunks)
        if key not in self._tables:
            words = _lib.load().mjx_mt_jump_table_words(self.n, self.k, self._chunks)
            if words < 0:
                raise _lib.MjxError(f"no jump-ahead geometry for n={self.n}, k={self.k}")
            if words == 0:
                self._tables[key] = None
            else:
                host = np.empty(words, dtype=np.uint64)
                _lib.call("mjx_mt_jump_table", self.n, self.k, self._chunks, host.ctypes.data)
                self._tables[key] = torch.from_numpy(host.view(np.int64)).to(self.done.device)
        return self._tables[key]

    # -- one iteration's tail: rollout and record ------------------------------------
    def _rolled(self, first=False):
        """The node-packed end state s_endstate(s) of the union (:352)."""
        st, T = self.st, self.p + self.c - 1
        if first:
            st.s_from_biases()
            _lib.call("mjx_pack_np", _device.ptr(st.s), _lib.MJX_I32, st.plan.n, _device.ptr(self._bits),
                      _device.stream_handle())
        if not T:
            return self._bits
        return rollout(st.plan.graph, self._bits, T, out=self._rtmp[0], tmp=self._rtmp[1])

    def _record(self, end, t_add, TT):
        _lib.call("mjx_hpr_batch_record", _device.ptr(end), _device.ptr(self.st.s), self.n, len(self.inst),
                  _device.ptr(self._inst_dev), _device.ptr(self._tbase), int(t_add), int(TT),
                  _device.ptr(self._counts), _device.ptr(self.done), _device.ptr(self.t_stop),
                  _device.ptr(self.conf), _device.ptr(self._live), _device.stream_handle())

    def _launches(self):
        """The launches of k iterations (code/HPR_pytorch_RRG.py:345-356) of the
        union on the current stream, every argument fixed (HPRState.
        _batch_launches with the record in the place of the counts)."""
        st, plan, lib = self.st, self.st.plan, _lib.load()
        N, d, p, c, code, h = plan.n, plan.d, self.p, self.c, _code(self.dtype), _device.stream_handle()
        wp, wm = self._w
        q = st.layout == "q"
        sc, sz = self._scales.data_ptr(), self._scales.element_size()
        nbr, in_row, out_row = _device.ptr(plan.nbr), _device.ptr(plan.in_row), _device.ptr(plan.out_row)
        for j in range(self.k):
            src, dst = (st.chi, st.chi_b) if j % 2 == 0 else (st.chi_b, st.chi)
            mask = _device.ptr(self._mask[j])
            if q:
                _lib.call("mjx_hpr_update_q", code, _device.ptr(src), _device.ptr(dst), _device.ptr(st.biases), nbr,
                          in_row, out_row, N, d, p, c, st.attr_value, wp, wm, st.damppar, sc + j * sz, h)
                _lib.call("mjx_hpr_marginals_q", code, _device.ptr(dst), out_row, N, d, p, c, 1e-15,
                          sc + (j + 1) * sz, _device.ptr(st._ii), _device.ptr(st.zwork), None, h)
                _lib.call("mjx_hpr_node_step", code, _device.ptr(st.zwork), out_row, N, d, _device.ptr(st.marg),
                          _device.ptr(st.biases), mask, st.pie, _device.ptr(st.s), _device.ptr(self._bits), h)
            else:
                rc = lib.mjx_hpr_update(code, _device.ptr(src), _device.ptr(dst), _device.ptr(st.biases), nbr, in_row,
                                        out_row, N, d, p, c, st.attr_value, wp, wm, st.damppar, h)
                if rc == _lib.MJX_ERANGE:
                    raise _lib.MjxError(f"HPR batches run the register update kernels only: d={d}, p={p}, c={c} "
                                        "needs the per-degree-class kernel (use hpr_run)")
                _lib.check(rc, "mjx_hpr_update")
                _lib.call("mjx_hpr_marginals", code, _device.ptr(dst), out_row, N, d, p, c, 1e-15,
                          _device.ptr(st.zwork), _device.ptr(st.marg), h)
                _lib.call("mjx_hpr_new_biases_mask", code, _device.ptr(st.biases), _device.ptr(st.marg), mask, st.pie,
                          N, _device.ptr(st.s), h)
                _lib.call("mjx_pack_np", _device.ptr(st.s), _lib.MJX_I32, N, _device.ptr(self._bits), h)
            self._record(self._rolled(), j + 1, self.TT)

    # -- batches ---------------------------------------------------------------------
    def _draw(self, t0):
        """The refresh masks of the k iterations from t0 on, every instance from
        its own stream, on the generators' side stream; the engines' states at
        the batch start stay in the slot's snapshot."""
        st, k = self.st, self.k
        slot = self._slot
        self._slot ^= 1
        thr = torch.tensor([1 - (1 + (t0 + j)) ** (-st.gamma) for j in range(k)], dtype=torch.float64)
        if st.layout == "q":
            self._pin_scales[slot].copy_(torch.tensor([st.decay(t0 + j) for j in range(k + 1)], dtype=self.dtype))
        gs, table = self._gen_stream, self._table()
        with torch.cuda.stream(gs):
            gs.wait_event(self._mask_free[slot])               # the batch two back has copied its masks out
            self._snap[slot][0].copy_(self._mt)
            self._snap[slot][1].copy_(self._ln)
            self._gthr[slot].copy_(thr)
            _lib.call("mjx_hpr_refresh_masks_jump_batch", _device.ptr(self._snap[slot][0]),
                      _device.ptr(self._snap[slot][1]), _device.ptr(self._mt), _device.ptr(self._ln), self.n, k,
                      self._chunks, len(self.inst), _device.ptr(table) if table is not None else None,
                      _device.ptr(self._gthr[slot]), _device.ptr(self._gmask[slot]), gs.cuda_stream)
            self._gen_done[slot].record(gs)
        return {"t0": t0, "slot": slot}

    def _launch(self, drawn):
        slot = drawn["slot"]
        if drawn["t0"] != self.st.t:
            raise ValueError("batch drawn for another iteration")
        torch.cuda.current_stream().wait_event(self._gen_done[slot])
        self._mask.copy_(self._gmask[slot])
        self._mask_free[slot].record()
        if self.st.layout == "q":
            self._scales.copy_(self._pin_scales[slot], non_blocking=True)
        if self.use_graph and self._graph is not None:
            self._graph.replay()
        elif self.use_graph and self._warm:
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._launches()
            self._graph.replay()
        else:
            try:
                self._launches()
            except _lib.MjxError:
                torch.cuda.synchronize()                       # the masks in flight write buffers about to be freed
                raise
            self._warm = True
        self._tbase.add_(self.k)                               # the record kernels read the batch's first t here
        self.st.t += self.k
        self._live_host.copy_(self._live, non_blocking=True)
        self._done_ev.record()

    def _read_live(self):
        self._live_host.copy_(self._live, non_blocking=True)
        self._done_ev.record()
        return self._collect()

    def _collect(self):
        """The one host read of a batch: the number of instances still running."""
        self._done_ev.synchronize()
        return int(self._live_host[0])

    def _finish_generators(self, slot, t0):
        """Leave the generator of every instance that stopped in the batch drawn
        in ``slot`` (from iteration t0) where the reference's would be: the
        batch-start engine plus one rand(n) per iteration up to its stop."""
        done = self.done.cpu().numpy()
        new = [(i, int(o)) for i, o in enumerate(self.inst) if done[o] and not self._final[o]]
        if not new:
            return done
        if slot is not None:
            t_stop = self.t_stop.cpu().numpy()
            mt = self._snap[slot][0].cpu().numpy()
            ln = self._snap[slot][1].cpu().numpy()
        for i, o in new:
            self._final[o] = True
            if slot is None:
                continue                                       # stopped before the loop: no draw made
            gen = self.generators[o]
            gen.set_state(self._state_bytes(o, mt[i], ln[i]))
            for _ in range(int(t_stop[o]) - t0):
                torch.rand(self.n, dtype=torch.float64, generator=gen)
        return done

    def _state_bytes(self, o, mt, ln):
        """Instance o's CPU generator state with the engine (mt[624], (left, next))."""
        b = self._gen_bytes[o].copy()
        b[24:24 + 624 * 8] = mt.view(np.uint32).astype(np.uint64).view(np.uint8)
        b[8:12] = np.array([ln[0]], dtype=np.int32).view(np.uint8)
        b[16:24] = np.array([ln[1]], dtype=np.uint64).view(np.uint8)
        return torch.from_numpy(b)

    def rng_state_bytes(self, slot, i):
        """The CPU generator state (uint8 tensor for set_state) of the instance
        in slot i of the current union at the start of the batch drawn in ``slot``."""
        self._gen_stream.synchronize()                         # the snapshot is written on the generators' stream
        mt, ln = self._snap[slot]
        return self._state_bytes(int(self.inst[i]), mt[i].cpu().numpy(), ln[i].cpu().numpy())

    def _rebuild(self, done, nxt):
        """Compaction: the union of the live instances, their message rows, II
        sums, biases and engines (at the start of the batch drawn ahead in
        ``nxt``, which is dropped) gathered from the current union."""
        st, n, E, dev = self.st, self.n, self.E, self.done.device
        keep = [i for i, o in enumerate(self.inst) if not done[o]]
        self._gen_stream.synchronize()
        torch.cuda.current_stream().synchronize()              # nothing in flight holds the old buffers
        Et = len(self.inst) * E
        sel = torch.tensor(keep, dtype=torch.int64, device=dev)
        fwd = (sel[:, None] * E + torch.arange(E, device=dev)[None, :]).reshape(-1)
        rows = torch.cat([fwd, Et + fwd])
        nodes = (sel[:, None] * n + torch.arange(n, device=dev)[None, :]).reshape(-1)
        self._mt = self._snap[nxt["slot"]][0].index_select(0, sel)
        self._ln = self._snap[nxt["slot"]][1].index_select(0, sel)
        st.chi, st.chi_b = st.chi.index_select(0, rows), st.chi_b.index_select(0, rows)
        if st.layout == "q":
            st._ii = st._ii.view(Et, 4).index_select(0, fwd).reshape(-1)
        st.biases = st.biases.index_select(0, nodes)
        self.inst = self.inst[keep]
        st.plan = _plan_of(_union([self.per[o] for o in self.inst], n, self.d))
        st.zwork = torch.empty(4 * st.plan.E, dtype=self.dtype, device=dev)
        st.marg = torch.empty((st.plan.n, 2), dtype=self.dtype, device=dev)
        st.s = torch.empty(st.plan.n, dtype=torch.int32, device=dev)
        self._alloc()

    def run(self, max_batches=None, stop=True):
        """Batches of k iterations until every instance has stopped (or
        ``max_batches`` batches; ``stop=False``: exactly that many, whatever has
        stopped, for timing).  Returns the number of instances still running."""
        nb = 0
        if (self.live == 0 and stop) or max_batches == 0:
            return self.live
        drawn = self._drawn if self._drawn is not None else self._draw(self.st.t)
        while True:
            t0 = self.st.t
            self._launch(drawn)
            cur = drawn
            drawn = self._draw(t0 + self.k)                    # one batch ahead, beside the iterations
            live = self._collect()
            nb += 1
            if live < self.live:
                done = self._finish_generators(cur["slot"], t0)
                self.live = live
                Gc = len(self.inst)
                if stop and 0 < live < Gc and live <= self.compact * Gc:
                    self._rebuild(done, drawn)
                    drawn = self._draw(self.st.t)
            if (stop and self.live == 0) or (max_batches is not None and nb >= max_batches):
                break
        self._drawn = drawn                                    # the batch drawn ahead: the next call's first
        if stop and self.live == 0:
            self._gen_stream.synchronize()                     # nothing left to run: it is dropped
        return self.live

    def results(self):
        """hpr_run's keys (:377) with leading dimension G."""
        conf = self.conf.cpu().numpy()
        return {"mag_reached": conf.sum(axis=1) / self.n,
                "num_steps": self.t_stop.cpu().numpy().astype(np.float64),
                "conf": conf.astype(np.float64),
                "graphs": np.stack([p[1] for p in self.per]).astype(np.float64)}


def hpr_run_batch(d, n, p, c, edges_list, seeds=None, damppar=0.4, attr_value=1, lmbd_in=None, pie=0.3, gamma=0.1,
                  TT=10000, nbrs_list=None, dtype=torch.float32, batch=16, graph=True, layout=None, compact=0.5,
                  generators=None):
    """``hpr_run`` for G graphs at once, as one union graph (HPRBatch).

    Instance k runs on edges_list[k] and draws chi0, biases0 and its
    per-iteration rand(n) from its own torch CPU generator -- generators[k], or
    a new one seeded seeds[k] -- exactly as hpr_run(seed=seeds[k]) does; on
    return each generator has made the draws the reference makes up to that
    instance's stop iteration.  ``batch`` iterations per host read (replayed as
    a hipGraph with ``graph``); ``compact``: see HPRBatch (results do not
    depend on it).  Shapes beyond the register update kernels (where hpr_run
    falls back to the per-degree-class kernel) raise MjxError.
    Returns mag_reached (G,), num_steps (G,), conf (G, n), graphs (G, n, d)."""
    edges_list = list(edges_list)
    G = len(edges_list)
    if generators is None:
        if seeds is None or len(seeds) != G:
            raise ValueError("one seed (or generator) per graph")
        generators = [torch.Generator().manual_seed(int(s)) for s in seeds]
    if len(generators) != G:
        raise ValueError("one generator per graph")
    E, nc = int(n) * int(d) // 2, 4 ** (int(p) + int(c))
    chi0s, b0s = [], []
    for gen in generators:
        chi0 = torch.rand((2 * E, nc), dtype=torch.float64, generator=gen)      # mes_init_mat, :101-103
        chi0s.append(chi0 / torch.sum(chi0, axis=1, keepdims=True))
        b0 = torch.rand((int(n), 2), dtype=torch.float64, generator=gen)        # :334-335
        b0s.append(b0 / torch.sum(b0, axis=1, keepdims=True))
    hb = HPRBatch(d, n, p, c, edges_list, chi0s, b0s, generators, dtype=dtype, damppar=damppar,
                  attr_value=attr_value, lmbd_in=lmbd_in, pie=pie, gamma=gamma, TT=TT, batch=batch, graph=graph,
                  layout=layout, compact=compact, nbrs_list=nbrs_list)
    hb.run()
    return hb.results()
