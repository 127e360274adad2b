"""Simulated annealing on CSR graphs on the device: every replica of
``SAReplicasER`` equals the CPU restatement of the reference loop
(tests/sa_er_oracle.py, pinned to the reference fixtures by tests/test_sa_er.py)
step by step -- proposals, accept decisions, sum(s_end), delta_H -- in the
light-cone mode with its lists in LDS, with every list spilled to HBM
(``lds_entries=4``) and in the full-rollout mode; on Erdos-Renyi graphs with
and without isolated nodes, a hub graph whose radius-2 bound is the whole
graph, and a multigraph with self-loops and doubled edges."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

import sa_er_oracle as ero

pytestmark = pytest.mark.gpu

R = 70                       # two word columns, the second ragged
CHECK = (0, 1, 63, 64, 69)   # first column's ends, second column's ends
STEPS, CHUNK = 3000, 1000
SEED0 = 7


@functools.lru_cache(maxsize=None)
def _graph(name):
    import mjx
    rp, col = ero.GRAPHS[name](mjx)
    return np.asarray(rp, dtype=np.int64), np.asarray(col, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _oracle(name, p, c, seed, steps):
    rp, col = _graph(name)
    return ero.sa_loop_er(rp, col, p, c, seed, max_steps=steps)


def _make(mjx, name, p, c, mode, seeds=None, **kw):
    rp, col = _graph(name)
    kernel = None
    if mode == "lightcone-spill":
        mode, kernel = "lightcone", {"lds_entries": 4}
    elif mode == "lightcone-wave":
        mode, kernel = "lightcone", {"split": 1}
    seeds = [SEED0 + r for r in range(R)] if seeds is None else seeds
    return mjx.SAReplicasER(mjx.Graph.csr(rp, col), p, c, seeds, mode=mode, kernel=kernel, **kw)


def _trace(sa, steps, chunk):
    parts = [sa.steps(chunk, trace=True) for _ in range(steps // chunk)]
    return {k: torch.cat([q[k] for q in parts]).cpu().numpy() for k in parts[0]}


def _assert_trace(tr, r, o, steps):
    L = len(o["i"])
    for key in ("i", "accept", "sum_end", "dE"):
        assert np.array_equal(tr[key][:L, r], o[key]), (r, key)
    if L < steps:                       # the replica finished: later rows are marked
        assert (tr["i"][L:, r] == -1).all() and (tr["accept"][L:, r] == -1).all()


def test_init_equals_numpy_and_the_oracle(mjx_mod):
    sa = _make(mjx_mod, "B", 2, 1, "lightcone")
    conf = sa.conf().cpu().numpy()
    sums = sa.sum_end.cpu().numpy()
    n = conf.shape[1]
    for r in range(R):
        s0 = 2 * np.random.RandomState(SEED0 + r).binomial(n=1, p=0.5, size=[n]) - 1
        assert np.array_equal(conf[r], s0), r
    for r in CHECK:
        assert sums[r] == _oracle("B", 2, 1, SEED0 + r, STEPS)["sum_end0"], r
    assert (sa.t.cpu().numpy() == 0).all()


CASES = [(g, pc, m) for g in "ABHM" for pc in ((1, 1), (2, 1), (2, 2))
         for m in ("lightcone", "lightcone-spill", "rollout") if m != "rollout" or g in "AH"]
CASES += [("A", (2, 2), "lightcone-wave"), ("M", (2, 1), "lightcone-wave")]   # a whole wave per word column


@pytest.mark.parametrize("gname,pc,mode", CASES, ids=[f"{g}-p{pc[0]}c{pc[1]}-{m}" for g, pc, m in CASES])
def test_trace_parity_with_the_oracle(mjx_mod, gname, pc, mode):
    p, c = pc
    sa = _make(mjx_mod, gname, p, c, mode)
    if mode == "lightcone-spill":
        assert sa.spill_bytes > 0
    if gname == "H" and mode.startswith("lightcone") and p + c - 1 >= 2:
        assert sa.caps[1] == 201 and sa.caps[2] == 300 and sa.spill_bytes > 0    # the hub: spills under any choice
    tr = _trace(sa, STEPS, CHUNK)
    res = sa.results()
    for r in CHECK:
        o = _oracle(gname, p, c, SEED0 + r, STEPS)
        _assert_trace(tr, r, o["trace"], STEPS)
        assert np.array_equal(res["conf"][r], o["conf"]), r
        assert res["num_steps"][r] == o["num_steps"] and res["done"][r] == o["done"], r
    assert int(res["near_ties"].sum()) == 0
    assert int(res["done"].max()) <= 2              # no list ever outgrew its cap


def test_hub_is_proposed_and_reached(mjx_mod):
    """The hub case exercises what it is meant to: the hub itself is proposed
    (a 201-entry candidate list) in the traced window."""
    o = _oracle("H", 2, 1, SEED0, STEPS)
    assert int((o["trace"]["i"] == 0).sum()) == 14


def test_lightcone_equals_rollout(mjx_mod):
    seeds = list(range(130))
    a = _make(mjx_mod, "A", 2, 2, "lightcone", seeds=seeds)
    b = _make(mjx_mod, "A", 2, 2, "rollout", seeds=seeds)
    for _ in range(3):
        a.steps(1000)
        b.steps(1000)
    for f in ("s", "t", "a", "b", "sum_end", "done", "mt", "mt_idx"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    g = a.graph
    cur = a.s
    for lvl in a.levels:
        cur = mjx_mod.rollout(g, cur, 1, words=a.W)
        assert torch.equal(lvl, cur)


@pytest.mark.parametrize("name", ["sa_d3_n300_p2c1.npz", "sa_d4_n200_p1c1.npz"])
def test_regular_graph_as_csr_reproduces_the_reference_fixtures(mjx_mod, name):
    z = load_golden(name)
    p, c = int(z["p"]), int(z["c"])
    seeds = [int(s) for s in z["seeds"]]
    rp, col = ero.csr_of_ell(z["N"])
    sa = mjx_mod.SAReplicasER(mjx_mod.Graph.csr(rp, col), p, c, seeds, mode="lightcone")
    L = max(len(z[f"seed{sd}_i"]) for sd in seeds)
    chunk = 1024
    steps = -(-L // chunk) * chunk
    tr = _trace(sa, steps, chunk)
    for r, sd in enumerate(seeds):
        _assert_trace(tr, r, {k: z[f"seed{sd}_{k}"] for k in ("i", "accept", "sum_end", "dE")}, steps)
    assert int(sa.results()["near_ties"].sum()) == 0


def test_runs_to_consensus(mjx_mod):
    seeds = [0, 1]
    orc = [ero.sa_loop_er(*_graph("A"), 2, 1, sd, max_steps=60000) for sd in seeds]
    assert all(o["done"] == 1 for o in orc)          # both finish within 60000 proposals
    sa = _make(mjx_mod, "A", 2, 1, "lightcone", seeds=seeds)
    chunk, parts = 4096, []
    while not sa.all_done() and len(parts) * chunk < 60000:
        parts.append(sa.steps(chunk, trace=True))
    tr = {k: torch.cat([q[k] for q in parts]).cpu().numpy() for k in parts[0]}
    res = sa.results()
    for r, o in enumerate(orc):
        assert res["done"][r] == 1
        assert res["num_steps"][r] == o["num_steps"]
        assert np.array_equal(res["conf"][r], o["conf"])
        assert res["mag_reached"][r] == o["mag_reached"]
        _assert_trace(tr, r, o["trace"], tr["i"].shape[0])
        assert (tr["i"][o["num_steps"]:, r] == -1).all()


def test_chunking_and_resume(mjx_mod, tmp_path):
    one = _make(mjx_mod, "A", 2, 1, "lightcone")
    one.steps(3000)
    three = _make(mjx_mod, "A", 2, 1, "lightcone")
    half = _make(mjx_mod, "A", 2, 1, "lightcone")
    for _ in range(3):
        three.steps(1000)
    half.steps(1500)
    path = str(tmp_path / "ck.npz")
    half.save_checkpoint(path)
    rp, col = _graph("A")
    back = mjx_mod.SAReplicasER.resume(mjx_mod.Graph.csr(rp, col), path, mode="lightcone")
    back.steps(1500)
    for other in (three, back):
        for f in ("s", "t", "a", "b", "sum_end", "done", "mt", "mt_idx", "ties"):
            assert torch.equal(getattr(one, f), getattr(other, f)), f
        for x, y in zip(one.levels, other.levels):
            assert torch.equal(x, y)
    with pytest.raises(ValueError):
        mjx_mod.SAReplicasER.resume(mjx_mod.Graph.csr(*_graph("B")), path)


def test_refusals(mjx_mod):
    rp, col = _graph("B")
    bad = col.copy()
    bad[0] = (int(col[0]) + 1) % (rp.shape[0] - 1)      # (v, x) -> (v, x+1): (x, v) has lost its partner
    with pytest.raises(ValueError, match="symmetric"):
        mjx_mod.SAReplicasER(mjx_mod.Graph.csr(rp, bad), 2, 1, [0, 1])
    # H: the spill area of 70 replicas at p+c-1 = 2 with the default LDS part
    sa = _make(mjx_mod, "H", 2, 1, "lightcone")
    need = sa.spill_bytes
    assert need > 0
    assert _make(mjx_mod, "H", 2, 1, "auto", scratch_limit=need - 1).mode == "rollout"
    assert _make(mjx_mod, "H", 2, 1, "auto", scratch_limit=need).mode == "lightcone"
    with pytest.raises(ValueError, match="scratch_limit"):
        _make(mjx_mod, "H", 2, 1, "lightcone", scratch_limit=need - 1)
    with pytest.raises(ValueError):
        mjx_mod.SAReplicas(mjx_mod.Graph.csr(*_graph("A")), 2, 1, [0])       # the regular class still refuses CSR
    # direct ABI calls: argument checks that return before any launch
    lib, L = mjx_mod.load_library(), mjx_mod._lib

    def call(state, spill_bytes):
        return lib.mjx_sa_csr_lightcone_steps(sa.graph.row_ptr.data_ptr(), sa.graph.col.data_ptr(), sa.n, 2, 1, R,
                                              sa.s.data_ptr(), sa._lvl, ctypes.byref(state), 1, sa.par_a, sa.par_b,
                                              sa.a_cap, sa.b_cap, int(sa.t_cap), sa._caps_c, 0, sa.spill.data_ptr(),
                                              spill_bytes, None)

    before = sa.t.clone()
    st = L.MjxSaState.from_buffer_copy(sa._state)
    st.rep_graph = sa.prop_i.data_ptr()
    assert call(st, need) == L.MJX_EINVAL
    st = L.MjxSaState.from_buffer_copy(sa._state)
    assert call(st, need - 4) == L.MJX_EINVAL
    st.philox_key = sa.cnt.data_ptr()
    assert call(st, need) == L.MJX_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(sa.t, before)                 # nothing ran


def test_sa_er_run_and_e_delta(mjx_mod):
    res = mjx_mod.sa_er_run(120, 4 / 119, 2, 1, N_stat=3, seed=5, max_steps=2000)
    n = res["row_ptr"].shape[0] - 1
    assert set(res) == {"mag_reached", "num_steps", "conf", "done", "near_ties", "wall_s", "row_ptr", "col", "n_iso"}
    assert n + int(res["n_iso"]) == 120 and res["col"].shape[0] == res["row_ptr"][-1]
    assert res["conf"].shape == (3, n) and set(np.unique(res["conf"])) <= {-1, 1}
    for k in ("mag_reached", "num_steps", "done", "near_ties", "wall_s"):
        assert res[k].shape == (3,), k
    assert ((res["num_steps"] == 2000) | (res["done"] != 0)).all()
    assert np.array_equal(res["mag_reached"], res["conf"].sum(axis=1) / n)
    # same graph given explicitly, same seeds: the same result
    again = mjx_mod.sa_er_run(p=2, c=1, N_stat=3, seed=5, max_steps=2000, graph=(res["row_ptr"], res["col"]),
                              mode="rollout")
    assert np.array_equal(again["conf"], res["conf"]) and np.array_equal(again["num_steps"], res["num_steps"])
    # E_delta on the CSR graph against the oracle's
    g = mjx_mod.Graph.csr(res["row_ptr"], res["col"])
    s0 = 2 * np.random.RandomState(3).binomial(n=1, p=0.5, size=[n]) - 1
    a, b = 0.015 * n, 0.01 * n
    for i in (0, 1, n // 2, n - 2, n - 1):
        assert mjx_mod.E_delta(g, s0, a, b, 2, 1, i) == ero.delta_E(res["row_ptr"], res["col"], s0, a, b, 2, 1, i), i
