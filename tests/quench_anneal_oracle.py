"""ORACLE helper (test infrastructure only) for the Metropolis add / drop walk
inside the consensus set: the definition of include/mjx.h restated in numpy on
quench_oracle.end_state / quench and attractor_oracle.philox4x32_10.

A job is (start r, restart k) with its visiting order.  After the quench pass,
sweep u makes n proposals; proposal q draws (w0, w1) = words 0 and 1 of
philox4x32_10((q, u, r, k), (seed_lo, seed_hi)) and the node i = (w0 n) >> 32.
A +1 node is dropped when a full rollout of the whole graph from the state
without it still ends all +1; a -1 node is added when w1 < thr[u].  The
lightest sweep end is kept and quenched once more.  Nothing here uses a light
cone or the monotonicity fact.

Jobs that share a graph advance together: proposal (u, q) of all of them is one
batched rollout.  That is bookkeeping only; no job reads another's state.
"""
import itertools

import numpy as np

import quench_oracle as qo
from attractor_oracle import philox4x32_10


def thresholds(beta):
    """min(floor(e^-beta 2^32), 2^32 - 1) in float64 -> uint32."""
    b = np.asarray(beta, dtype=np.float64)
    return np.minimum(np.floor(np.exp(-b) * 4294967296.0), 4294967295.0).astype(np.uint32)


def proposals(n, u, r, k, seed):
    """The n proposals of sweep u of job (r, k): (nodes int64 [n], accept words uint32 [n])."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((np.arange(n, dtype=np.uint64), u, r, k), (seed & 0xFFFFFFFF, seed >> 32))
    return ((w[0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64), w[1]


def _consensus(step, X, T):
    return (qo.end_state(step, X, T) == 1).all(axis=1)


def _batch(step, S, T, ords, rr, kk, thr, seed):
    """Jobs j = 0..J-1 on one graph: start S[j], order ords[j], stream (rr[j], kk[j])."""
    S = np.asarray(S, dtype=np.int64)
    J, n = S.shape
    U = len(thr)
    cons = _consensus(step, S, T)
    X = S.copy()
    flipped = np.zeros(J, np.int64)
    for j in np.flatnonzero(cons):
        w = qo.quench(step, S[j:j + 1], T, ords[j])
        X[j], flipped[j] = w["conf"][0], w["flipped"][0]
    plus_quench = (X == 1).sum(axis=1)
    best, plus_best, best_sweep = X.copy(), plus_quench.copy(), np.zeros(J, np.int64)
    moves = np.zeros((J, 3), np.int64)
    trace = np.empty((J, U), np.int32)
    add_after_drop_pending = np.zeros(J, bool)          # an add happened; a later drop completes "drop after add"
    drop_after_add = np.zeros(J, bool)
    live = np.flatnonzero(cons)
    for u in range(U):
        if live.size:
            draws = [proposals(n, u, rr[j], kk[j], seed) for j in live]
            nodes = np.stack([d[0] for d in draws])                      # (live, n)
            words = np.stack([d[1] for d in draws])
            for q in range(n):
                i = nodes[:, q]
                up = X[live, i] == 1
                # drops: a full rollout of every proposing job's state without its node
                t = live[up]
                if t.size:
                    Y = X[t].copy()
                    Y[np.arange(t.size), i[up]] = -1
                    ok = _consensus(step, Y, T)
                    X[t[ok]] = Y[ok]
                    moves[t[ok], 1] += 1
                    moves[t[~ok], 2] += 1
                    drop_after_add[t[ok]] |= add_after_drop_pending[t[ok]]
                a = ~up & (words[:, q] < thr[u])
                X[live[a], i[a]] = 1
                moves[live[a], 0] += 1
                add_after_drop_pending[live[a]] = True
        now = (X == 1).sum(axis=1)
        trace[:, u] = now
        better = cons & (now < plus_best)
        best[better], plus_best[better], best_sweep[better] = X[better], now[better], u + 1
    conf = best.copy()
    for j in live:
        conf[j] = qo.quench(step, best[j:j + 1], T, ords[j])["conf"][0]
    return {"conf": conf, "consensus": cons, "flipped": flipped, "plus_quench": plus_quench, "plus_best": plus_best,
            "best_sweep": best_sweep, "moves": moves, "trace": trace, "drop_after_add": drop_after_add}


def anneal_jobs(step, S, T, orders, thr, seed):
    """S (R, n); orders (K, n) shared or (R, K, n); thr: uint32 [U]; ``step`` may be a list of R steps (a graph
    per start).  -> dict conf (R, K, n), flipped / plus_quench / plus_best / best_sweep int64 (R, K), moves
    int64 (R, K, 3) = adds, drops, refused, trace int32 (R, K, U), consensus bool [R], sums (R, K) and
    drop_after_add bool (R, K) (some drop came after some add)."""
    S = np.asarray(S, dtype=np.int64)
    R, n = S.shape
    orders = np.broadcast_to(orders, (R,) + np.shape(orders)[-2:])
    K = orders.shape[1]
    thr = np.asarray(thr, dtype=np.uint32)
    jobs = list(itertools.product(range(R), range(K)))
    groups = [[j for j in jobs if j[0] == r] for r in range(R)] if isinstance(step, (list, tuple)) else [jobs]
    out = None
    for grp in groups:
        rr, kk = [j[0] for j in grp], [j[1] for j in grp]
        st = step[rr[0]] if isinstance(step, (list, tuple)) else step
        w = _batch(st, S[rr], T, [orders[r, k] for r, k in grp], rr, kk, thr, seed)
        if out is None:
            out = {key: np.empty((R, K) + v.shape[1:], v.dtype) for key, v in w.items() if key != "consensus"}
            out["consensus"] = np.empty(R, bool)
        for key, v in w.items():
            if key == "consensus":
                out[key][rr] = v
            else:
                out[key][rr, kk] = v
    out["sums"] = out["conf"].sum(axis=2)
    return out


def anneal(step, s, T, order, thr, seed, r=0, k=0):
    """One job -> the dict of ``anneal_jobs`` without the (R, K) axes."""
    w = _batch(step, np.asarray(s, dtype=np.int64)[None, :], T, [np.asarray(order)], [r], [k],
               np.asarray(thr, dtype=np.uint32), seed)
    return {key: v[0] for key, v in w.items()}


def optimum(step, n, T):
    """Brute force over all 2^n states (n <= 20): the smallest weight of a consensus state."""
    assert n <= 20
    best = n
    for lo in range(0, 1 << n, 1 << 14):
        x = np.arange(lo, min(lo + (1 << 14), 1 << n), dtype=np.int64)
        X = np.where((x[:, None] >> np.arange(n)) & 1, 1, -1).astype(np.int64)
        ok = _consensus(step, X, T)
        if ok.any():
            best = min(best, int((X[ok] == 1).sum(axis=1).min()))
    return best
