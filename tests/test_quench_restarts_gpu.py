"""``quench_restarts`` on the GPU: every (start, order) job against the numpy
restatement of the sequential pass (tests/quench_oracle.py), one oracle call
per job.  Integer exact: every comparison is array_equal."""
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import quench_cases
import quench_oracle as qo
from conftest import ROOT
from quench_cases import _graph, hub_graph

pytestmark = pytest.mark.gpu

K_CASE = 3
# name -> starts R: the first R of the shared table's starts (``random_starts`` fills row by row, so they
# are the starts of seed and R alone); R is the smallest multiple of 16 at which the case is not
# degenerate (_not_degenerate).  "hub80": a row longer than a wave's 64 lanes, and one node of degree 0
STARTS = {"rrg_d3_n200_T2": 32, "rrg_d4_n96_T3": 16, "rrg_d5_n120_T2": 16, "rrg_d3_n130_T4": 16,
          "er_n300_deg3_T2": 16, "er_n300_deg5_T3": 32, "rrg_d3_n64_T6": 16, "hub80": 16}
TABLE = [k for k in STARTS if k not in ("rrg_d3_n64_T6", "hub80")]


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (graph as the package takes it, oracle step, S (STARTS[name], n), T).  Shared: never written."""
    spec, step, S, T = quench_cases._case(name)
    return spec, step, S[:STARTS[name]], T


def _shared_orders(n, K=K_CASE):
    return np.stack([np.random.default_rng([5, k]).permutation(n) for k in range(K)])


def _oracle(step, S, T, orders):
    """One oracle call per job.  orders: (K, n) shared or (R, K, n).
    -> dict conf (R, K, n), flipped (R, K), sums (R, K), consensus [R]."""
    R, n = S.shape
    orders = np.broadcast_to(orders, (R,) + orders.shape[-2:])
    K = orders.shape[1]
    conf = np.empty((R, K, n), np.int64)
    flipped = np.empty((R, K), np.int64)
    consensus = np.empty(R, bool)
    for r in range(R):
        for k in range(K):
            w = qo.quench(step, S[r:r + 1], T, orders[r, k])
            conf[r, k], flipped[r, k], consensus[r] = w["conf"][0], w["flipped"][0], w["consensus"][0]
    return {"conf": conf, "flipped": flipped, "sums": conf.sum(axis=2), "consensus": consensus}


@functools.lru_cache(maxsize=None)
def _want(name):
    _, step, S, T = _case(name)
    return _oracle(step, S, T, _shared_orders(S.shape[1]))


def _not_degenerate(want, name):
    """The conditions a case must meet in the oracle before anything is compared."""
    cons = want["consensus"]
    assert cons.sum() >= 4 and (~cons).sum() >= 4, f"{name}: {cons.sum()} of {cons.size} starts at consensus"
    K = want["conf"].shape[1]
    differ = [all(not np.array_equal(want["conf"][r, a], want["conf"][r, b]) for a in range(K) for b in range(a))
              for r in np.flatnonzero(cons)]
    assert any(differ), f"{name}: no consensus start whose {K} results differ pairwise"


def _assert_jobs(res, want, S):
    R, n = S.shape
    K = want["conf"].shape[1]
    assert res["conf"].dtype == np.int8 and res["conf"].shape == (R, K, n)
    assert np.array_equal(res["conf"], want["conf"])
    assert res["flipped"].dtype == np.int64 and np.array_equal(res["flipped"], want["flipped"])
    assert res["mag"].dtype == np.float64 and np.array_equal(res["mag"], want["sums"] / n)
    assert res["consensus"].dtype == bool and np.array_equal(res["consensus"], want["consensus"])
    cons = want["consensus"]
    assert np.array_equal(res["conf"][~cons], np.repeat(S[~cons][:, None, :], K, axis=1))
    assert not res["flipped"][~cons].any()
    assert res["flipped"][cons].sum() > 0


# ---- 1. the table -------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE)
def test_every_job_equals_the_oracle(mjx_mod, name):
    want = _want(name)
    _not_degenerate(want, name)
    _, _, S, T = _case(name)
    keep = S.copy()
    res = mjx_mod.quench_restarts(_graph(name), S, T, 1, restarts=K_CASE, orders=_shared_orders(S.shape[1]),
                                  keep_all=True)
    assert np.array_equal(S, keep), "the input was written"
    _assert_jobs(res, want, S)


# ---- 2. per-start orders and the seed rule ---------------------------------------
def test_orders_per_start_and_the_seed_rule(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, step, S, T = _case(name)
    R, n = S.shape
    orders = np.stack([np.stack([np.random.default_rng([7, r, k]).permutation(n) for k in range(2)])
                       for r in range(R)])
    want = _oracle(step, S, T, orders)
    _not_degenerate(_want(name), name)
    explicit = mjx_mod.quench_restarts(_graph(name), S, T, 1, restarts=2, orders=orders, keep_all=True)
    _assert_jobs(explicit, want, S)
    # the orders are per start: start r's jobs differ from what start 0's orders would give
    shared = _oracle(step, S, T, orders[0])
    assert not np.array_equal(shared["conf"], want["conf"])
    seeded = mjx_mod.quench_restarts(_graph(name), S, T, 1, restarts=2, seed=7, keep_all=True)
    for key in ("conf", "flipped", "mag", "consensus", "best", "conf_best", "mag_best"):
        assert np.array_equal(seeded[key], explicit[key]), key


# ---- 3. the same answer as quench ---------------------------------------------------
@pytest.mark.parametrize("name", ["rrg_d4_n96_T3", "er_n300_deg5_T3"])
def test_one_order_equals_quench(mjx_mod, name):
    _, _, S, T = _case(name)
    o = np.random.default_rng(3).permutation(S.shape[1])
    old = mjx_mod.quench(_graph(name), S, T, 1, order=o)
    assert old["flipped"].sum() > 0
    new = mjx_mod.quench_restarts(_graph(name), S, T, 1, orders=o)
    assert new["conf_best"].dtype == old["conf"].dtype and np.array_equal(new["conf_best"], old["conf"])
    assert np.array_equal(new["flipped"][:, 0], old["flipped"])
    assert np.array_equal(new["mag_best"], old["mag"]) and np.array_equal(new["consensus"], old["consensus"])
    # neither orders nor seed: the identity, quench's default
    ident = mjx_mod.quench_restarts(_graph(name), S, T, 1)
    assert np.array_equal(ident["conf_best"], mjx_mod.quench(_graph(name), S, T, 1)["conf"])


# ---- 4. a graph per start --------------------------------------------------------------
def test_a_graph_per_start(mjx_mod):
    n, d, T, K = 96, 4, 3, 2
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    assert graphs.shape == (4, 96, 4)
    S = qo.random_starts(4, n, 0.7, seed=41)
    S[3] = 1
    orders = _shared_orders(n, K)
    res = mjx_mod.quench_restarts(graphs, S, T, 1, restarts=K, orders=orders, keep_all=True)
    confs = []
    for r in range(4):
        for k in range(K):
            w = qo.quench(qo.step_ell(graphs[r]), S[r:r + 1], T, orders[k])
            assert np.array_equal(res["conf"][r, k], w["conf"][0]), (r, k)
            assert res["flipped"][r, k] == w["flipped"][0] and res["consensus"][r] == w["consensus"][0]
        # the graph matters: start r on graph 0 ends elsewhere (checked where anything flips)
        confs.append(qo.quench(qo.step_ell(graphs[0]), S[r:r + 1], T, orders[0])["conf"][0])
    assert res["consensus"][3] and res["flipped"][3].min() > 0
    assert any(not np.array_equal(confs[r], res["conf"][r, 0]) for r in range(1, 4))
    with pytest.raises(ValueError, match="4 graphs for 3 starts"):
        mjx_mod.quench_restarts(graphs, S[:3], T, 1, restarts=K, orders=orders)


# ---- 5. word edges and tiny sizes --------------------------------------------------------
@pytest.mark.parametrize("n", [33, 64, 65, 70])
def test_word_edges_one_start_and_padding_bits(mjx_mod, n):
    d = 3 if (n * 3) % 2 == 0 else 4
    T = 2
    adj = mjx_mod.random_regular_graph(d, n, seed=50 + n)
    step = qo.step_ell(adj)
    S = qo.random_starts(8, n, 0.7, seed=60 + n)
    S[0] = 1                                        # a start that is at consensus for sure
    orders = _shared_orders(n)
    want = _oracle(step, S, T, orders)
    assert want["flipped"][0].min() > 0
    res = mjx_mod.quench_restarts(adj, S, T, 1, restarts=K_CASE, orders=orders, keep_all=True)
    assert np.array_equal(res["conf"], want["conf"]) and np.array_equal(res["flipped"], want["flipped"])
    # R = 1 with an (n,) input: the input's shape back
    one = mjx_mod.quench_restarts(adj, S[0], T, 1, restarts=K_CASE, orders=orders, keep_all=True)
    assert one["conf_best"].shape == (n,) and one["conf"].shape == (1, K_CASE, n)
    assert np.array_equal(one["conf"][0], want["conf"][0])
    assert one["mag"].shape == (1, K_CASE) and one["best"].shape == (1,) and one["consensus"].tolist() == [True]
    assert np.array_equal(one["conf_best"], want["conf"][0, one["best"][0]])
    # the packed result: bit v of the words = spin v, the bits past n are 0
    words = res["state_best"].cpu().numpy().view(np.uint64)
    Wn = (n + 63) // 64
    assert words.shape == (8, Wn)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(8, Wn * 64)
    assert not bits[:, n:].any(), "padding bits of the packed output must be 0"
    assert np.array_equal(np.where(bits[:, :n] == 1, 1, -1), res["conf_best"])


def test_padding_bits_through_the_abi(mjx_mod):
    """Dirty padding bits in s_np are ignored and out_np comes back with them 0."""
    n, d, T, R, K = 70, 3, 2, 2, 2
    adj = mjx_mod.random_regular_graph(d, n, seed=120)
    g = mjx_mod.Graph.ell(adj)
    S = np.ones((R, n), np.int64)
    S[1, ::2] = -1
    orders = _shared_orders(n, K)
    want = _oracle(qo.step_ell(adj), S, T, orders)
    assert want["consensus"].tolist() == [True, False]
    lib = mjx_mod.load_library()
    caps = (ctypes.c_int64 * (T + 1))()
    assert lib.mjx_ell_ball_bound(n, d, T, caps) == 0
    Wn = 2
    s_np = torch.stack([mjx_mod.pack(S[r]) for r in range(R)])
    s_np[:, 1] |= ~((1 << (n - 64)) - 1)            # every bit past n set
    dev = s_np.device
    order_t = torch.from_numpy(orders.astype(np.int32)).to(dev)
    out_np = torch.full((R * K, Wn), -1, dtype=torch.int64, device=dev)
    flipped = torch.full((R * K,), -1, dtype=torch.int64, device=dev)
    plus = torch.full((R * K,), -1, dtype=torch.int64, device=dev)
    consensus = torch.full((R,), 7, dtype=torch.uint8, device=dev)
    flag = torch.full((R * K,), 7, dtype=torch.int32, device=dev)
    rc = lib.mjx_quench_jobs_ell(g.adj.data_ptr(), n, d, 0, R, K, T, 1, caps, s_np.data_ptr(), order_t.data_ptr(), 0,
                                 out_np.data_ptr(), flipped.data_ptr(), plus.data_ptr(), consensus.data_ptr(),
                                 flag.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert not flag.any() and consensus.tolist() == [1, 0]
    words = out_np.cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(R * K, 128)
    assert not bits[:, n:].any()
    assert np.array_equal(np.where(bits[:, :n] == 1, 1, -1), want["conf"].reshape(R * K, n))
    assert np.array_equal(flipped.cpu().numpy(), want["flipped"].reshape(-1))
    assert np.array_equal(2 * plus.cpu().numpy() - n, want["sums"].reshape(-1))


def test_wrong_caps_raise_the_jobs_flag_and_a_shape_past_the_lds_is_refused(mjx_mod):
    """Caps below the graph's ball bound: the job stops at the first list that would outgrow its cap and says
    so in its flag; a job without consensus builds no list and keeps flag 0.  A shape whose bitmaps do not
    fit the LDS never reaches the kernel."""
    n, d, T, R, K = 70, 3, 2, 2, 1
    adj = mjx_mod.random_regular_graph(d, n, seed=120)
    g = mjx_mod.Graph.ell(adj)
    S = np.ones((R, n), np.int64)
    S[1, ::2] = -1
    lib = mjx_mod.load_library()
    caps = (ctypes.c_int64 * (T + 1))(1, 1, 1)
    s_np = torch.stack([mjx_mod.pack(S[r]) for r in range(R)])
    dev = s_np.device
    order_t = torch.arange(n, dtype=torch.int32, device=dev)
    out_np = torch.zeros((R * K, 2), dtype=torch.int64, device=dev)
    flipped, plus = torch.zeros(R * K, dtype=torch.int64, device=dev), torch.zeros(R * K, dtype=torch.int64, device=dev)
    consensus, flag = torch.zeros(R, dtype=torch.uint8, device=dev), torch.zeros(R * K, dtype=torch.int32, device=dev)
    rc = lib.mjx_quench_jobs_ell(g.adj.data_ptr(), n, d, 0, R, K, T, 1, caps, s_np.data_ptr(), order_t.data_ptr(), 0,
                                 out_np.data_ptr(), flipped.data_ptr(), plus.data_ptr(), consensus.data_ptr(),
                                 flag.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert flag.tolist() == [1, 0] and consensus.tolist() == [1, 0]
    # 2e5 nodes on a ring: five bitmaps of 25 KB each
    big = 200_000
    ring = np.stack([(np.arange(big) - 1) % big, (np.arange(big) + 1) % big], axis=1)
    with pytest.raises(ValueError, match="quench is the path"):
        mjx_mod.quench_restarts(ring, np.ones(big, np.int64), 3, 1)


# ---- 6. hub and isolated node --------------------------------------------------------------
def test_a_hub_past_64_lanes_and_an_isolated_node(mjx_mod):
    _, step, S, T = _case("hub80")
    rp, col, lone = hub_graph(more=80)
    g = _graph("hub80")
    assert np.diff(rp)[0] >= 70
    caps = mjx_mod.SAReplicasER.ball_bound(g, T)
    assert caps[T] > 64, "the lists must be longer than one wave"
    orders = _shared_orders(300, 2)
    want = _oracle(step, S, T, orders)
    cons = want["consensus"]
    assert cons.sum() >= 4 and want["flipped"][cons].min() > 0
    res = mjx_mod.quench_restarts(g, S, T, 1, restarts=2, orders=orders, keep_all=True)
    _assert_jobs(res, want, S)
    # the isolated node keeps its spin, so where the end state is all +1 it is +1 and stays
    assert (S[cons, lone] == 1).all() and (res["conf"][cons][:, :, lone] == 1).all()
    # the hub itself is tried: some job drops it or keeps it, as the oracle says
    assert np.array_equal(res["conf"][:, :, 0], want["conf"][:, :, 0])


# ---- 7. the ends of the T range ----------------------------------------------------------------
def test_T0_flips_nothing_and_T7_is_refused(mjx_mod):
    name = "rrg_d3_n200_T2"
    _, _, S, _ = _case(name)
    S = S.copy()
    S[5] = 1                                        # T = 0: consensus means all +1 already
    res = mjx_mod.quench_restarts(_graph(name), S, 1, 0, restarts=2, seed=1, keep_all=True)
    assert np.array_equal(res["conf_best"], S) and not res["flipped"].any()
    assert np.array_equal(res["conf"], np.repeat(S[:, None, :], 2, axis=1))
    assert np.array_equal(res["consensus"], (S == 1).all(axis=1)) and res["consensus"][5]
    assert not res["best"].any()
    for p, c in ((7, 1), (6, 2), (4, 4)):
        with pytest.raises(ValueError):
            mjx_mod.quench_restarts(_graph(name), S, p, c)


def test_T6_against_the_oracle(mjx_mod):
    name = "rrg_d3_n64_T6"
    want = _want(name)
    _not_degenerate(want, name)
    _, _, S, T = _case(name)
    assert T == 6
    res = mjx_mod.quench_restarts(_graph(name), S, 5, 2, restarts=K_CASE, orders=_shared_orders(64), keep_all=True)
    _assert_jobs(res, want, S)


# ---- 8. local minimum ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rrg_d4_n96_T3", "er_n300_deg3_T2"])
def test_the_best_result_is_a_local_minimum(mjx_mod, name):
    _, _, S, T = _case(name)
    g = _graph(name)
    res = mjx_mod.quench_restarts(g, S, T, 1, restarts=K_CASE, seed=2)
    after = mjx_mod.flip_gains(g, res["conf_best"], T, 1, gain=False)
    assert not after["n_removable"].any()
    assert np.array_equal(after["consensus"], res["consensus"]) and res["consensus"].any()


# ---- 9. best -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rrg_d4_n96_T3", "rrg_d5_n120_T2"])
def test_best_is_the_first_smallest_sum(mjx_mod, name):
    want = _want(name)
    _, _, S, T = _case(name)
    n = S.shape[1]
    res = mjx_mod.quench_restarts(_graph(name), S, T, 1, restarts=K_CASE, orders=_shared_orders(n))
    assert "conf" not in res
    best = np.argmin(want["sums"], axis=1)
    assert res["best"].dtype == np.int64 and np.array_equal(res["best"], best)
    rows = np.arange(S.shape[0])
    assert np.array_equal(res["mag_best"], res["mag"][rows, res["best"]])
    assert np.array_equal(res["conf_best"], want["conf"][rows, best])
    cons = want["consensus"]
    assert (want["sums"][cons].max(axis=1) > want["sums"][cons].min(axis=1)).any(), "the pick must matter somewhere"
    assert not res["best"][~cons].any(), "all restarts tie without consensus: the first"


# ---- 10. plumbing --------------------------------------------------------------------------------------
def test_tensor_in_tensor_out_and_the_input_buffer_is_untouched(mjx_mod):
    name = "rrg_d4_n96_T3"
    want = _want(name)
    _, _, S, T = _case(name)
    orders = _shared_orders(S.shape[1])
    rows = np.arange(S.shape[0])
    for dtype in (torch.int8, torch.int64):
        s = torch.from_numpy(S).to("cuda", dtype)
        keep = s.clone()
        res = mjx_mod.quench_restarts(_graph(name), s, T, 1, restarts=K_CASE, orders=torch.from_numpy(orders),
                                      keep_all=True)
        assert torch.equal(s, keep)
        for key in ("mag", "flipped", "consensus", "best", "conf_best", "mag_best", "conf"):
            assert isinstance(res[key], torch.Tensor) and res[key].device == s.device, key
        assert res["conf_best"].dtype == dtype and res["conf"].dtype == torch.int8
        assert res["consensus"].dtype == torch.bool and res["mag"].dtype == torch.float64
        assert np.array_equal(res["conf"].cpu().numpy(), want["conf"])
        best = res["best"].cpu().numpy()
        assert np.array_equal(res["conf_best"].cpu().numpy(), want["conf"][rows, best])
        assert np.array_equal(res["flipped"].cpu().numpy(), want["flipped"])


# ---- 11. CLI ---------------------------------------------------------------------------------------------
def test_cli_restarts_in_a_fresh_process(mjx_mod, tmp_path):
    n, d, T = 96, 4, 3
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    conf = qo.random_starts(4, n, 0.7, seed=41).astype(np.float64)
    conf[3] = 1.0
    f1 = tmp_path / "sa.npz"
    np.savez(f1, conf=conf, graphs=graphs.astype(np.float64), mag_reached=conf.mean(axis=1))
    spec, _, S, T2 = _case("er_n300_deg3_T2")
    f2 = tmp_path / "er.npz"
    np.savez(f2, conf=S.astype(np.float64), row_ptr=spec[1], col=spec[2], n_iso=np.int64(0))
    for f, p in ((f1, T), (f2, T2)):
        run = subprocess.run([sys.executable, "-m", "mjx", "quench", "--in", str(f), "--p", str(p), "--c", "1",
                              "--restarts", "3", "--order-seed", "5", "--out", str(f) + ".out.npz"],
                             capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert run.returncode == 0, run.stderr[-2000:]
    with np.load(str(f1) + ".out.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["best", "conf", "conf_quenched", "consensus", "flipped", "graphs", "mag_quenched",
                                   "mag_reached", "mag_restarts"]
        want = mjx_mod.quench_restarts(graphs, conf.astype(np.int64), T, 1, restarts=3, seed=5)
        assert np.array_equal(z["conf"], conf) and z["conf_quenched"].dtype == np.float64
        assert np.array_equal(z["conf_quenched"], want["conf_best"])
        assert np.array_equal(z["mag_quenched"], want["mag_best"]) and np.array_equal(z["best"], want["best"])
        assert z["mag_restarts"].shape == (4, 3) and np.array_equal(z["mag_restarts"], want["mag"])
        assert np.array_equal(z["consensus"], want["consensus"]) and z["consensus"][3]
        assert np.array_equal(z["flipped"], want["flipped"][np.arange(4), want["best"]]) and z["flipped"][3] > 0
    with np.load(str(f2) + ".out.npz", allow_pickle=False) as z:
        want = mjx_mod.quench_restarts(_graph("er_n300_deg3_T2"), S, T2, 1, restarts=3, seed=5)
        assert np.array_equal(z["conf_quenched"], want["conf_best"]) and np.array_equal(z["best"], want["best"])
        assert np.array_equal(z["mag_restarts"], want["mag"]) and np.array_equal(z["mag_quenched"], want["mag_best"])
        assert np.array_equal(z["consensus"], want["consensus"]) and np.array_equal(z["row_ptr"], spec[1])
        assert np.array_equal(z["flipped"], want["flipped"][np.arange(S.shape[0]), want["best"]])
