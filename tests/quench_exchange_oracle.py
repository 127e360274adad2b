"""ORACLE helper (test infrastructure only) for the (1, 2) exchange descent:
the definition of include/mjx.h restated in numpy on quench_oracle.end_state.

A job is one start with one visiting order.  After the quench pass, every -1
node j of the order is added in turn and every +1 node a != j of the order is
then tried for removal with a full rollout of the whole graph (the tries
between two drops see the same state and run as one batch); the add is kept when at least two
nodes dropped, otherwise the state is as it was.  Nothing here uses a light
cone, a candidate set or the monotonicity fact: every +1 node is tried.

``lemma_set`` restates the set of nodes the kernel may restrict its tries to:
D_t = the nodes whose level-t value differs between x and x + j, and the union
of the balls B(D_t, t + 2), by breadth-first search.
"""
import numpy as np

import quench_oracle as qo


def _consensus(step, x, T):
    return bool((qo.end_state(step, x[None, :], T) == 1).all())


def exchange(step, s, T, order, max_passes=8, on_drop=None):
    """One job.  s: (n,) +-1, order: a permutation of 0..n-1.
    -> dict conf (n,), consensus (of s), flipped, plus_quench, exchanges, passes, converged.
    ``on_drop(x, j, a)``: called for every drop of a committed exchange with the state x before its add."""
    s = np.asarray(s, dtype=np.int64)
    order = np.asarray(order)
    if not _consensus(step, s, T):
        return {"conf": s.copy(), "consensus": False, "flipped": 0, "plus_quench": int((s == 1).sum()),
                "exchanges": 0, "passes": 0, "converged": True}
    w = qo.quench(step, s[None, :], T, order)
    x = w["conf"][0].copy()
    out = {"consensus": True, "flipped": int(w["flipped"][0]), "plus_quench": int((x == 1).sum()),
           "exchanges": 0, "passes": 0, "converged": False}
    for ps in range(1, int(max_passes) + 1):
        moved = False
        for j in order:
            if x[j] != -1:
                continue
            y = x.copy()
            y[j] = 1
            # the inner walk.  Only a drop changes y, so the nodes between two drops are all tried on the
            # same y: one batched rollout per stretch, the first success is the next drop, and the walk goes
            # on behind it.  (A node's own spin changes only by its own drop: +1 now is +1 at its turn.)
            todo = [int(a) for a in order if a != j and y[a] == 1]
            drops = []
            while todo:
                Y = np.repeat(y[None, :], len(todo), axis=0)
                Y[np.arange(len(todo)), todo] = -1
                ok = np.flatnonzero((qo.end_state(step, Y, T) == 1).all(axis=1))
                if ok.size == 0:
                    break
                y[todo[ok[0]]] = -1
                drops.append(todo[ok[0]])
                todo = todo[ok[0] + 1:]
            if len(drops) >= 2:
                if on_drop is not None:
                    for a in drops:
                        on_drop(x, int(j), a)
                x = y
                out["exchanges"] += 1
                moved = True
        out["passes"] = ps
        if not moved:
            out["converged"] = True
            break
    out["conf"] = x
    return out


def exchange_jobs(step, S, T, orders, max_passes=8):
    """S (R, n); orders (K, n) shared or (R, K, n).  One ``exchange`` per job; ``step`` may be a list of R
    steps (a graph per start).  -> dict conf (R, K, n), flipped / plus_quench / exchanges / passes int64
    (R, K), converged bool (R, K), consensus bool [R], sums (R, K)."""
    S = np.asarray(S, dtype=np.int64)
    R, n = S.shape
    orders = np.broadcast_to(orders, (R,) + np.shape(orders)[-2:])
    K = orders.shape[1]
    out = {"conf": np.empty((R, K, n), np.int64), "consensus": np.empty(R, bool),
           "converged": np.empty((R, K), bool)}
    for key in ("flipped", "plus_quench", "exchanges", "passes"):
        out[key] = np.empty((R, K), np.int64)
    for r in range(R):
        st = step[r] if isinstance(step, (list, tuple)) else step
        for k in range(K):
            w = exchange(st, S[r], T, orders[r, k], max_passes)
            out["consensus"][r] = w["consensus"]
            for key in ("conf", "flipped", "plus_quench", "exchanges", "passes", "converged"):
                out[key][r, k] = w[key]
    out["sums"] = out["conf"].sum(axis=2)
    return out


def neighbours_ell(adj):
    adj = np.asarray(adj)
    return [np.unique(adj[v]) for v in range(adj.shape[0])]


def neighbours_csr(row_ptr, col):
    return [np.unique(col[row_ptr[v]:row_ptr[v + 1]]) for v in range(len(row_ptr) - 1)]


def ball(nbrs, seeds, radius):
    """Nodes within ``radius`` hops of any node of ``seeds``."""
    seen = set(int(v) for v in seeds)
    front = set(seen)
    for _ in range(radius):
        front = {int(u) for v in front for u in nbrs[v]} - seen
        seen |= front
    return seen


def lemma_set(step, nbrs, x, j, T):
    """x with x[j] = -1 -> ([D_0, .., D_{T-1}], union of B(D_t, t + 2))."""
    x = np.asarray(x, dtype=np.int64)
    y = x.copy()
    y[j] = 1
    D, allowed = [], set()
    lx, ly = x[None, :], y[None, :]
    for t in range(T):
        D.append(np.flatnonzero(lx[0] != ly[0]))
        allowed |= ball(nbrs, D[t], t + 2)
        lx, ly = step(lx), step(ly)
    return D, allowed
