"""BDCM lambda sweeps over a batch of graphs in one device loop.

G graphs are one disjoint-union graph: class D of the union is the union of the
instances' classes D, so "Gauss-Seidel across classes, Jacobi within a class"
(nb:133-198) holds for every instance exactly as when it runs alone, and the
launches of one sweep carry G times the work.  What the single-plan functions
of ``bdcm`` cannot express is per-instance control, which the ``*_batch``
kernels take from a control block per instance (include/mjx.h): each instance
stops its convergence loop at its own sweep and leaves the lambda sweep at its
own lambda, and phi and m_init are per-graph sums.

Layout: instance g owns the rows [row_off[g], row_off[g] + 2 E_g) of one chi
tensor of shape (sum 2 E_g, 4^T) and keeps the notebook's layout inside its
block, so ``chi[row_off[g]:row_off[g+1]]`` is a drop-in per-instance message
array; its core nodes are node_off[g] + i.

  bdcm_batch_layout(graphs, p, c)            the union's index arrays (numpy only)
  BDCMBatch(plans, p, c)                     the same on the device, from BDCMPlans
  bdcm_leaf_reset_batch, BDCM_ER_batch       one union pass, in place, optionally gated
  bdcm_converge_batch                        ``converge`` with a stop flag per instance
  bdcm_partition_batch                       Zi, Zij and the m_init terms of the union
  bdcm_observables_batch                     (phi[G], m_init[G])
  BDCM_entropy_procedure_batch               G lambda sweeps in lockstep
"""
import math

import numpy as np
import torch

from . import _device, _lib
from .bdcm import plan_indices

INT32_MAX = 2 ** 31 - 1


def bdcm_batch_layout(graphs, p=1, c=1, pcs=None):
    """Index arrays of the disjoint union of ``graphs`` (host arrays only).

    graphs: sequence of ``plan_indices`` dicts, or of (edges, row_ptr, col)
    triples.  pcs (optional): the (p, c) each instance was prepared for; one
    that differs from the batch's (p, c) raises ValueError, as do an empty
    list and a union whose rows or nodes do not fit int32.

    Returns a dict: G, p, c, row_off[G+1], node_off[G+1] (= the seg_ptr over
    nodes), edge_seg[G+1] (seg_ptr over union edges), edges (E_total, 2) and
    deg in union node ids, fwd_row[e] / rev_row[e] (rows of u -> v and v -> u
    of union edge e), edge_classes = [(D, rows[m], inc[m, D], inst[m])] and
    node_classes = [(D, nodes[m], inc[m, D], inst[m])] in ascending D, items
    ordered by instance and then in the instance's own order."""
    graphs = [g if isinstance(g, dict) else plan_indices(*g) for g in graphs]
    G = len(graphs)
    if G == 0:
        raise ValueError("a batch needs at least one graph")
    if pcs is not None:
        if len(pcs) != G:
            raise ValueError("pcs must name one (p, c) per graph")
        for g, pc in enumerate(pcs):
            if (int(pc[0]), int(pc[1])) != (int(p), int(c)):
                raise ValueError(f"instance {g} has (p, c) = {tuple(pc)}, the batch ({p}, {c})")
    E = np.array([h["E"] for h in graphs], dtype=np.int64)
    row_off = np.concatenate([[0], np.cumsum(2 * E)])
    node_off = np.concatenate([[0], np.cumsum([h["n_core"] for h in graphs])]).astype(np.int64)
    edge_seg = np.concatenate([[0], np.cumsum(E)])
    if row_off[-1] > INT32_MAX or node_off[-1] > INT32_MAX:
        raise ValueError(f"the union has {row_off[-1]} rows and {node_off[-1]} nodes: row and node ids are int32")

    def union(key, item_off):
        out = []
        for D in sorted({D for h in graphs for D, _, _ in h[key]}):
            items, inc, inst = [], [], []
            for g, h in enumerate(graphs):
                for Dg, it, ic in h[key]:
                    if Dg == D:
                        items.append(it + item_off[g])
                        inc.append(ic.reshape(it.size, D) + row_off[g])
                        inst.append(np.full(it.size, g, dtype=np.int64))
            out.append((int(D), np.concatenate(items), np.concatenate(inc), np.concatenate(inst)))
        return out

    r = [np.arange(e, dtype=np.int64) for e in E]
    return {"G": G, "p": int(p), "c": int(c), "row_off": row_off, "node_off": node_off, "edge_seg": edge_seg,
            "edges": np.concatenate([h["edges"] + node_off[g] for g, h in enumerate(graphs)]),
            "deg": np.concatenate([h["deg"] for h in graphs]),
            "fwd_row": np.concatenate([row_off[g] + r[g] for g in range(G)]),
            "rev_row": np.concatenate([row_off[g] + r[g] + E[g] for g in range(G)]),
            "edge_classes": union("edge_classes", row_off), "node_classes": union("node_classes", node_off)}


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))).to(dev)


class BDCMBatch:
    """The union of G BDCMPlans on the device, for messages of 4^(p+c) columns.

    G, row_off, node_off (host); ``chi_from(arrays)`` packs per-instance message
    arrays into the union's device tensor, ``views(chi)`` gives the G
    per-instance views of it."""

    SCRATCH_CAP = 256 << 20          # bytes of count tables in flight for the high-degree classes

    def __init__(self, plans, p=1, c=1):
        plans = list(plans)
        lay = bdcm_batch_layout([pl.host for pl in plans], p, c)
        dev = _device.require_gpu()
        self.device = dev
        self.plans = plans
        self.p, self.c = int(p), int(c)
        self.nc = 4 ** (self.p + self.c)
        self.G = lay["G"]
        self.row_off, self.node_off, self.edge_seg = lay["row_off"], lay["node_off"], lay["edge_seg"]
        self.rows_total, self.n_core, self.E = int(self.row_off[-1]), int(self.node_off[-1]), int(self.edge_seg[-1])
        self.n = np.array([pl.n for pl in plans], dtype=np.int64)
        self.n_iso = np.array([pl.n_iso for pl in plans], dtype=np.int64)
        self.edge_classes = [(D, _i32(rows, dev), _i32(inc, dev), _i32(inst, dev), int(rows.size))
                             for D, rows, inc, inst in lay["edge_classes"]]
        self.node_classes = [(D, _i32(nodes, dev), _i32(inc, dev), int(nodes.size))
                             for D, nodes, inc, _ in lay["node_classes"]]
        self.edges, self.deg = _i32(lay["edges"], dev), _i32(lay["deg"], dev)
        self.fwd_row, self.rev_row = _i32(lay["fwd_row"], dev), _i32(lay["rev_row"], dev)
        self.edge_seg_dev = torch.from_numpy(self.edge_seg).to(dev)
        self.node_seg_dev = torch.from_numpy(self.node_off).to(dev)
        G = self.G
        self._work = torch.empty(G * 256, dtype=torch.float64, device=dev)
        self._sums = torch.zeros((3, G), dtype=torch.float64, device=dev)
        self._ctl = torch.zeros((G, 4), dtype=torch.int64, device=dev)     # mjx_bdcm_iter_*_batch
        self._w = torch.zeros(2, dtype=torch.float64, device=dev)          # lambda weights of a captured loop
        self._upd = torch.empty(max(max(m for *_, m in self.edge_classes) * self.nc, 1), dtype=torch.float64,
                                device=dev)
        self._scratch = None
        self._graphs = {}

    @property
    def classes(self):
        return [D for D, *_ in self.edge_classes]

    def check_pc(self, p, c):
        if (int(p), int(c)) != (self.p, self.c):
            raise ValueError(f"the batch was built for (p, c) = ({self.p}, {self.c}), got ({p}, {c})")

    def scratch_args(self):
        """(pointer, bytes) of the slab for the count tables of the classes
        beyond the LDS budget, (None, 0) if every class fits; raises MjxError if
        a class is unsupported.  Like BDCMPlan.scratch, for the union's classes."""
        lib = _lib.load()
        need = 0
        for D, m in [(D, m) for D, *_, m in self.edge_classes] + [(D, m) for D, *_, m in self.node_classes]:
            b = lib.mjx_bdcm_scratch_bytes(D, self.p, self.c)
            if b < 0:
                raise _lib.MjxError(f"BDCM class D={D} at p+c={self.p + self.c} is unsupported")
            need = max(need, min(b * m, max(b, self.SCRATCH_CAP)))
        if not need:
            return None, 0
        if self._scratch is None or self._scratch.numel() != need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._graphs.clear()             # a captured loop holds the old slab's address
        return _device.ptr(self._scratch), need

    def chi_from(self, arrays):
        """The packed (sum 2 E_g, 4^T) float64 device tensor of G per-instance
        message arrays (numpy or torch, (2 E_g, 4^T) or (2 E_g,) + (2,)*2T)."""
        arrays = list(arrays)
        if len(arrays) != self.G:
            raise ValueError(f"{self.G} instances, {len(arrays)} message arrays")
        chi = torch.empty((self.rows_total, self.nc), dtype=torch.float64, device=self.device)
        for g, a in enumerate(arrays):
            a = torch.as_tensor(a, dtype=torch.float64)
            lo, hi = int(self.row_off[g]), int(self.row_off[g + 1])
            if a.numel() != (hi - lo) * self.nc:
                raise ValueError(f"instance {g} must hold (2E, 4^T) = ({hi - lo}, {self.nc}) messages, "
                                 f"got {tuple(a.shape)}")
            chi[lo:hi].copy_(a.reshape(hi - lo, self.nc))
        return chi

    def views(self, chi):
        ch = _chi2d(chi, self, self.p, self.c)
        return [ch[int(self.row_off[g]):int(self.row_off[g + 1])] for g in range(self.G)]

    def set_active(self, active=None):
        """Zero the control blocks; the stop flag of every instance not in the
        boolean mask ``active`` is preset, so gated launches leave it untouched."""
        h = np.zeros((self.G, 4), dtype=np.int64)
        if active is not None:
            h[:, 1] = ~np.asarray(active, dtype=bool)
        self._ctl.copy_(torch.from_numpy(h))
        return self._ctl


def _chi2d(chi, batch, p, c):
    batch.check_pc(p, c)
    if not (isinstance(chi, torch.Tensor) and chi.is_cuda and chi.dtype == torch.float64 and chi.is_contiguous()):
        raise _lib.MjxError("chi must be a contiguous float64 device tensor (it is updated in place, nb:196-198)")
    if chi.numel() != batch.rows_total * batch.nc:
        raise ValueError(f"chi must hold ({batch.rows_total}, {batch.nc}) messages, got {tuple(chi.shape)}")
    return chi.view(batch.rows_total, batch.nc)


def _update(ch, batch, D, rows, inc, inst, m, attr_value, lmbd, damp, eps, flags, w_dev=None):
    _lib.call("mjx_bdcm_update_class_batch", _device.ptr(ch), _device.ptr(rows), _device.ptr(inc) if D else None,
              _device.ptr(inst), m, D, batch.p, batch.c, int(attr_value), float(lmbd), float(damp), float(eps),
              _device.ptr(batch._upd), _device.ptr(batch._ctl), int(flags),
              _device.ptr(w_dev) if w_dev is not None else None, *batch.scratch_args(), _device.stream_handle())


def BDCM_ER_batch(chi, batch, p, c, attr_value, lmbd_in, damppar, epsilon=0.0, gated=False, delta=False, w_dev=None):
    """One BDCM sweep of the union (``BDCM_ER`` for every instance), in place.
    ``gated``: instances whose stop flag in the batch's control blocks is set
    are left untouched; ``delta``: every instance's max |chi_new - chi_old|
    goes into its own control block (atomic max of float64 bits)."""
    ch = _chi2d(chi, batch, p, c)
    flags = (_lib.MJX_BDCM_GATE if gated else 0) | (_lib.MJX_BDCM_DELTA if delta else 0)
    for (D, rows, inc, inst, m) in batch.edge_classes:
        if D > 0:
            _update(ch, batch, D, rows, inc, inst, m, attr_value, lmbd_in, damppar, epsilon, flags, w_dev)
    return chi


def bdcm_leaf_reset_batch(chi, batch, p, c, attr_value, lmbd_in, gated=False):
    """``bdcm_leaf_reset`` for every instance (``gated``: every instance whose
    stop flag is not set)."""
    ch = _chi2d(chi, batch, p, c)
    for (D, rows, inc, inst, m) in batch.edge_classes:
        if D == 0:
            _update(ch, batch, 0, rows, inc, inst, m, attr_value, lmbd_in, 1.0, 0.0,
                    _lib.MJX_BDCM_GATE if gated else 0)
    return chi


def _sweep_gated(ch, batch, attr_value, lmbd, damppar, epsilon, eps, T_max, w_dev=None):
    """One iteration of the device loop: begin, the gated sweep, end."""
    st = _device.stream_handle()
    _lib.call("mjx_bdcm_iter_begin_batch", _device.ptr(batch._ctl), batch.G, st)
    BDCM_ER_batch(ch, batch, batch.p, batch.c, attr_value, lmbd, damppar, epsilon, gated=True, delta=True, w_dev=w_dev)
    _lib.call("mjx_bdcm_iter_end_batch", _device.ptr(batch._ctl), batch.G, float(eps), int(T_max), st)


def bdcm_converge_batch(chi, batch, p, c, attr_value, lmbd_in, damppar, eps, T_max, epsilon=0.0, active=None,
                        batch_sweeps=32, graph=True):
    """``converge`` for every instance of the union at once: each instance stops
    at its own sweep (own delta <= eps, own T_max hit) and is untouched from
    then on, the loop ends when every stop flag is set; one host read of the
    control blocks per ``batch_sweeps`` sweeps.  ``active`` (bool mask, optional):
    instances to iterate; the others are held still (t = 0).  ``graph``: the
    sweeps are captured once as one linear hipGraph (kept on the batch, keyed
    on every address and constant it bakes in; lambda is read from device
    memory) and replayed.  Returns (t[G], delta[G] of each instance's last sweep)."""
    ch = _chi2d(chi, batch, p, c)
    sc = batch.scratch_args()                  # every buffer exists before a capture
    ctl = batch.set_active(active)
    g = None
    w_dev = None
    if graph:
        w_dev = batch._w
        w_dev.copy_(torch.tensor([math.exp(-lmbd_in), math.exp(lmbd_in)], dtype=torch.float64))
        key = (ch.data_ptr(), batch._upd.data_ptr(), sc[0], ctl.data_ptr(), w_dev.data_ptr(), batch.p, batch.c,
               int(attr_value), float(damppar), float(eps), int(T_max), float(epsilon), int(batch_sweeps))
        g = batch._graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(batch_sweeps):
                    _sweep_gated(ch, batch, attr_value, lmbd_in, damppar, epsilon, eps, T_max, w_dev)
            batch._graphs.clear()              # one live graph per batch
            batch._graphs[key] = g
    while True:
        if graph:
            g.replay()
        else:
            for _ in range(batch_sweeps):
                _sweep_gated(ch, batch, attr_value, lmbd_in, damppar, epsilon, eps, T_max)
        h = ctl.cpu().numpy()
        if np.all(h[:, 1] != 0):
            return h[:, 2].copy(), np.ascontiguousarray(h[:, 3]).view(np.float64).copy()


def bdcm_partition_batch(chi, batch, p, c, attr_value, lmbd_in, epsilon=0.0):
    """(zi[sum n_core], zij[sum E], m_term[sum E]) of the union: ``Zi_ER``, ``Zij``
    and the per-edge term of m_init; instance g's share is the slice
    node_off[g]:node_off[g+1] resp. edge_seg[g]:edge_seg[g+1]."""
    ch = _chi2d(chi, batch, p, c)
    st = _device.stream_handle()
    zi = torch.empty(batch.n_core, dtype=torch.float64, device=ch.device)
    for (D, nodes, inc, m) in batch.node_classes:
        _lib.call("mjx_bdcm_node_z", _device.ptr(ch), _device.ptr(nodes), _device.ptr(inc), m, D, batch.p, batch.c,
                  int(attr_value), float(lmbd_in), float(epsilon), _device.ptr(zi), *batch.scratch_args(), st)
    zij = torch.empty(batch.E, dtype=torch.float64, device=ch.device)
    mt = torch.empty(batch.E, dtype=torch.float64, device=ch.device)
    _lib.call("mjx_bdcm_edge_obs_batch", _device.ptr(ch), _device.ptr(batch.fwd_row), _device.ptr(batch.rev_row),
              _device.ptr(batch.edges), _device.ptr(batch.deg), batch.E, batch.p, batch.c, int(attr_value),
              float(epsilon), _device.ptr(zij), _device.ptr(mt), st)
    return zi, zij, mt


def bdcm_observables_batch(chi, batch, p, c, attr_value, lmbd_in, epsilon=0.0):
    """(phi[G], m_init[G]) of nb:372-392 per instance, with one device->host read."""
    zi, zij, mt = bdcm_partition_batch(chi, batch, p, c, attr_value, lmbd_in, epsilon)
    st = _device.stream_handle()
    for slot, (x, seg, take_log) in enumerate(((zi, batch.node_seg_dev, 1), (zij, batch.edge_seg_dev, 1),
                                               (mt, batch.edge_seg_dev, 0))):
        _lib.call("mjx_segsum_f64", _device.ptr(x), _device.ptr(seg), batch.G, take_log, _device.ptr(batch._work),
                  _device.ptr(batch._sums[slot]), st)
    s = batch._sums.cpu().numpy()
    # isolated nodes follow the attractor, as in bdcm.observables
    phi = (s[0] - s[1] - int(attr_value) * lmbd_in * batch.n_iso) / batch.n
    m_init = (s[2] + int(attr_value) * batch.n_iso) / batch.n
    return phi, m_init


def BDCM_entropy_procedure_batch(chi, batch, lambdas, T_max=1300, p=1, c=1, attr_value=1, eps=1e-6, damppar=0.1,
                                 epsilon=0.0, stop_ent=-0.05, verbose=False, batch_sweeps=32):
    """``BDCM_entropy_procedure_GENERAL_ER`` for every instance of the union:
    all instances walk the shared lambda grid in lockstep; one that meets
    ent1 < stop_ent or a non-converged lambda (counts > 0) is deactivated from
    the next lambda on -- its messages frozen, its later entries zeros, as in
    the single function.  Returns a list of G dicts(m_init, ent1, ent, counts,
    iters)."""
    ch = _chi2d(chi, batch, p, c)
    batch.scratch_args()
    lambdas = np.asarray(lambdas, dtype=np.float64)
    L, G = lambdas.size, batch.G
    res = [{"m_init": np.zeros(L), "ent1": np.zeros(L), "ent": np.zeros(L), "counts": 0,
            "iters": np.zeros(L, dtype=np.int64)} for _ in range(G)]
    active = np.ones(G, dtype=bool)
    for k, lm in enumerate(lambdas.tolist()):
        if not active.any():
            break
        batch.set_active(active)
        bdcm_leaf_reset_batch(ch, batch, p, c, attr_value, lm, gated=True)
        t, _ = bdcm_converge_batch(ch, batch, p, c, attr_value, lm, damppar, eps, T_max, epsilon, active=active,
                                   batch_sweeps=batch_sweeps)
        phi, m_init = bdcm_observables_batch(ch, batch, p, c, attr_value, lm, epsilon)
        for g in np.flatnonzero(active).tolist():
            r = res[g]
            if t[g] >= T_max:
                r["counts"] = lm
            r["iters"][k] = t[g]
            r["ent"][k], r["m_init"][k] = float(phi[g]), float(m_init[g])
            r["ent1"][k] = r["ent"][k] + lm * r["m_init"][k]
            if verbose:
                print(f"instance {g} lambda= {lm}  t= {t[g]}  m_init: {r['m_init'][k]} ent: {r['ent1'][k]}", flush=True)
            if r["ent1"][k] < stop_ent or r["counts"] > 0:
                active[g] = False
    return res
