"""TEST HELPER (not a test): the reference's SA loop (code/SA_RRG.py:65-85)
restated over a CSR graph with ``np.random.RandomState(seed)`` -- the same
MT19937 stream and draw methods as the script's global ``np.random`` after
``np.random.seed(seed)`` -- and scored with the notebook's ER end state
(oracle.fast.s_endstate_er, nb:113-123).  Returns the per-step trace
(i, accept, sum_end, dE) and the final configuration, as the golden SA
fixtures record them for regular graphs."""
import numpy as np

from oracle import fast as orc


def csr_of_ell(N):
    """CSR (row_ptr int64, col int32) of an (n, d) neighbour array, row order kept."""
    N = np.asarray(N)
    n, d = N.shape
    return np.arange(n + 1, dtype=np.int64) * d, np.ascontiguousarray(N.reshape(-1).astype(np.int32))


def sa_loop_er(row_ptr, col, p, c, seed, par_a=1.0005, par_b=1.0005, max_steps=None, a0=None, b0=None):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int32)
    n = row_ptr.shape[0] - 1
    rs = np.random.RandomState(int(seed))
    s = 2 * rs.binomial(n=1, p=0.5, size=[n]) - 1                 # code/SA_RRG.py:65
    s0 = s.copy()
    a = 0.015 * n if a0 is None else a0                            # :67
    b = 0.01 * n if b0 is None else b0                             # :68
    t = 0
    sum_cur = np.sum(orc.s_endstate_er(row_ptr, col, s, p, c))
    tr = {"i": [], "accept": [], "sum_end": [], "dE": []}
    sum_end0 = int(sum_cur)
    m_final = sum_cur / n                                          # :71
    while m_final < 1 and (max_steps is None or t < max_steps):    # :72
        i = rs.randint(low=0, high=n)                              # :73
        s2 = s.copy()
        s2[i] = -s[i]
        sum_new = np.sum(orc.s_endstate_er(row_ptr, col, s2, p, c))
        delta_H = (-2 * a * s[i] + b * (sum_cur - sum_new)) / n    # :37
        prob_accept = min([1, np.exp(-delta_H)])                   # :75
        acc = rs.rand() < prob_accept                              # :76
        if acc:
            s[i] = -s[i]                                           # :77
            sum_cur = sum_new
        if a < 4.5 * n:                                            # :80
            a = par_a * a
        if b < 5 * n:                                              # :81
            b = par_b * b
        t += 1                                                     # :82
        tr["i"].append(i)
        tr["accept"].append(1 if acc else 0)
        tr["sum_end"].append(int(sum_cur))
        tr["dE"].append(float(delta_H))
        if t > 2 * n ** 3:                                         # :84
            m_final = 2
        else:
            m_final = sum_cur / n                                  # :85
    done = 2 if m_final == 2 else (1 if m_final >= 1 else 0)
    return {"conf": s.astype(np.int64), "s0": s0.astype(np.int64), "sum_end0": sum_end0, "num_steps": t,
            "mag_reached": np.sum(s) / n, "done": done, "a": a, "b": b,
            "trace": {"i": np.asarray(tr["i"], dtype=np.int64), "accept": np.asarray(tr["accept"], dtype=np.int8),
                      "sum_end": np.asarray(tr["sum_end"], dtype=np.int64),
                      "dE": np.asarray(tr["dE"], dtype=np.float64)}}


def delta_E(row_ptr, col, s, a, b, p, c, i):
    """E(s with s_i flipped) - E(s) on a CSR graph (code/SA_RRG.py:32-37)."""
    s = np.asarray(s).astype(np.int64)
    n = s.shape[0]
    s2 = s.copy()
    s2[i] = -s[i]
    sum1 = np.sum(orc.s_endstate_er(row_ptr, col, s, p, c))
    sum2 = np.sum(orc.s_endstate_er(row_ptr, col, s2, p, c))
    return (-2 * a * s[i] + b * (sum1 - sum2)) / n


# the issue's test graphs, built on the host with the package's samplers
def graph_A(mjx):
    rp, col, _ = mjx.erdos_renyi(150, 4 / 149, seed=3, drop_isolated=True)
    return rp, col


def graph_B(mjx):
    return mjx.erdos_renyi(97, 2.5 / 96, seed=3)


def graph_H(mjx):
    u, v = mjx.erdos_renyi_edges(300, 3 / 299, seed=5)
    u = np.concatenate([u, np.zeros(200, dtype=np.int64)])
    v = np.concatenate([v, np.arange(1, 201, dtype=np.int64)])
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    keys = np.unique(lo * 300 + hi)                # de-duplicated
    return mjx.csr_from_edges(300, keys // 300, keys % 300)


def graph_M(mjx):
    """Graph B with three self-loops and three doubled edges appended symmetrically."""
    rp, col = graph_B(mjx)
    n = rp.shape[0] - 1
    rows = [list(col[rp[v]:rp[v + 1]]) for v in range(n)]
    deg = np.diff(rp)
    nodes = [int(v) for v in np.flatnonzero(deg > 0)]
    for v in nodes[:3]:                            # a self-loop: one entry (v, v)
        rows[v].append(v)
    for v in nodes[3:6]:                           # a doubled edge: (v, w) and (w, v) once more
        w = int(rows[v][0])
        rows[v].append(w)
        rows[w].append(v)
    rp2 = np.zeros(n + 1, dtype=np.int64)
    rp2[1:] = np.cumsum([len(r) for r in rows])
    return rp2, np.asarray([x for r in rows for x in r], dtype=np.int32)


GRAPHS = {"A": graph_A, "B": graph_B, "H": graph_H, "M": graph_M}
