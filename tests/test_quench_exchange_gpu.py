"""``quench_exchange`` on the GPU: every (start, order) job against the numpy
restatement of the descent (tests/quench_exchange_oracle.py), which tries every
+1 node after every add with a rollout of the whole graph.  Integer exact:
every comparison is array_equal.  The oracle's results are computed once per
case and shared."""
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import quench_cases
import quench_exchange_oracle as xo
import quench_oracle as qo
from conftest import ROOT
from quench_cases import _graph, hub_graph

pytestmark = pytest.mark.gpu

K_CASE = 2
ORDER_SEED = 5
# name -> starts R: the first R of the shared table's starts
STARTS = {"rrg_d4_n96_T3": 16, "rrg_d3_n200_T2": 32, "rrg_d5_n120_T2": 16, "rrg_d4_n200_T1": 8,
          "er_n300_deg3_T2": 4}
KEYS = ("conf", "flipped", "mag_quench", "exchanges", "passes", "converged")


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (graph as the package takes it, oracle step, S (STARTS[name], n), T).  Shared: never written."""
    spec, step, S, T = quench_cases._case(name)
    return spec, step, S[:STARTS[name]], T


def _orders(R, n, K=K_CASE, seed=ORDER_SEED):
    """The seed rule written out: job (r, k) walks default_rng([seed, r, k]).permutation(n)."""
    return np.stack([np.stack([np.random.default_rng([seed, r, k]).permutation(n) for k in range(K)])
                     for r in range(R)])


@functools.lru_cache(maxsize=None)
def _want(name, max_passes=8):
    _, step, S, T = _case(name)
    return xo.exchange_jobs(step, S, T, _orders(*S.shape), max_passes)


def _not_degenerate(want, name):
    """The conditions a case must meet in the oracle before anything is compared."""
    cons = want["consensus"]
    moved = (want["exchanges"][cons] > 0).any(axis=1).sum()
    assert moved >= 2, f"{name}: {moved} consensus starts with an exchange"
    assert (~cons).sum() >= 1, f"{name}: every start is at consensus"
    assert want["passes"].max() >= 3, f"{name}: no job needs three passes"


def _assert_jobs(res, want, S):
    R, n = S.shape
    K = want["conf"].shape[1]
    assert res["conf"].dtype == np.int8 and res["conf"].shape == (R, K, n)
    assert np.array_equal(res["conf"], want["conf"])
    for key in ("flipped", "exchanges", "passes"):
        assert res[key].dtype == np.int64 and res[key].shape == (R, K) and np.array_equal(res[key], want[key]), key
    assert res["converged"].dtype == bool and np.array_equal(res["converged"], want["converged"])
    assert res["mag_quench"].dtype == np.float64
    assert np.array_equal(res["mag_quench"], (2 * want["plus_quench"] - n) / n)
    assert res["mag"].dtype == np.float64 and np.array_equal(res["mag"], want["sums"] / n)
    assert res["consensus"].dtype == bool and np.array_equal(res["consensus"], want["consensus"])
    cons = want["consensus"]
    assert np.array_equal(res["conf"][~cons], np.repeat(S[~cons][:, None, :], K, axis=1))
    assert not res["passes"][~cons].any() and res["converged"][~cons].all()
    best = np.argmin(want["sums"], axis=1)
    assert np.array_equal(res["best"], best)
    assert np.array_equal(res["conf_best"], want["conf"][np.arange(R), best])
    assert np.array_equal(res["mag_best"], res["mag"][np.arange(R), best])


# ---- 1. the table -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STARTS))
def test_every_job_equals_the_oracle(mjx_mod, name):
    want = _want(name)
    _not_degenerate(want, name)
    _, _, S, T = _case(name)
    keep = S.copy()
    res = mjx_mod.quench_exchange(_graph(name), S, T, 1, restarts=K_CASE, orders=_orders(*S.shape), keep_all=True)
    assert np.array_equal(S, keep), "the input was written"
    _assert_jobs(res, want, S)
    print(f"{name}: +1 spins after quench {want['plus_quench'][want['consensus']].mean():.1f}, after the descent "
          f"{(want['conf'][want['consensus']] == 1).sum(axis=2).mean():.1f}")


def test_the_seed_rule(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, _, S, T = _case(name)
    res = mjx_mod.quench_exchange(_graph(name), S, T, 1, restarts=K_CASE, seed=ORDER_SEED, keep_all=True)
    _assert_jobs(res, _want(name), S)


# ---- 2. hub and isolated node ---------------------------------------------------------
def test_a_hub_past_64_lanes_and_an_isolated_node(mjx_mod):
    _, step, S, T = quench_cases._case("hub80")
    rp, col, lone = hub_graph(more=80)
    g = _graph("hub80")
    assert np.diff(rp)[0] >= 70
    cons = np.flatnonzero((qo.end_state(step, S[:8], T) == 1).all(axis=1))[:2]
    assert cons.size == 2
    S = S[cons]
    orders = _orders(2, 300, 1)
    want = xo.exchange_jobs(step, S, T, orders)
    assert want["consensus"].all() and want["exchanges"].min() >= 1
    res = mjx_mod.quench_exchange(g, S, T, 1, orders=orders, keep_all=True)
    for key in KEYS[:2] + KEYS[3:]:
        assert np.array_equal(res[key], want[key]), key
    assert np.array_equal(res["mag_quench"], (2 * want["plus_quench"] - 300) / 300)
    # the isolated node keeps its spin: it is never dropped, and never added since it is +1
    assert (S[:, lone] == 1).all() and (res["conf"][:, :, lone] == 1).all()


# ---- 3. word edges -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 64, 65])
def test_word_edges_and_padding_bits(mjx_mod, n):
    d = 3 if (n * 3) % 2 == 0 else 4
    T = 2
    adj = mjx_mod.random_regular_graph(d, n, seed=50 + n)
    step = qo.step_ell(adj)
    S = qo.random_starts(8, n, 0.7, seed=60 + n)
    S[0] = 1                                        # a start that is at consensus for sure
    orders = _orders(8, n)
    want = xo.exchange_jobs(step, S, T, orders)
    assert want["consensus"][0] and want["exchanges"].sum() > 0
    res = mjx_mod.quench_exchange(adj, S, T, 1, restarts=K_CASE, orders=orders, keep_all=True)
    _assert_jobs(res, want, S)
    one = mjx_mod.quench_exchange(adj, S[0], T, 1, restarts=K_CASE, orders=orders[0], keep_all=True)
    assert one["conf_best"].shape == (n,) and one["conf"].shape == (1, K_CASE, n)
    assert np.array_equal(one["conf"][0], want["conf"][0]) and one["exchanges"].shape == (1, K_CASE)
    words = res["state_best"].cpu().numpy().view(np.uint64)
    Wn = (n + 63) // 64
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(8, Wn * 64)
    assert not bits[:, n:].any(), "padding bits of the packed output must be 0"
    assert np.array_equal(np.where(bits[:, :n] == 1, 1, -1), res["conf_best"])


class _Abi:
    """One call of mjx_quench_exchange_jobs_ell on poisoned outputs with a guard word at both ends."""
    GUARD = 0x5A

    def __init__(self, mjx_mod, adj, S, T, orders, caps, cap2T, max_passes=8, dirty_padding=False):
        self.n, self.d = adj.shape
        n, R, K = self.n, S.shape[0], orders.shape[0]
        g = mjx_mod.Graph.ell(adj)
        lib = mjx_mod.load_library()
        Wn = (n + 63) // 64
        s_np = torch.stack([mjx_mod.pack(S[r]) for r in range(R)]).reshape(R, Wn)
        if dirty_padding and n % 64:
            s_np[:, -1] |= ~((1 << (n % 64)) - 1)   # every bit past n set
        dev = s_np.device
        order_t = torch.from_numpy(orders.astype(np.int32)).to(dev)

        def buf(dtype, count):
            return torch.full((count + 2,), self.GUARD, dtype=dtype, device=dev)

        self.bufs = {"rank": buf(torch.int32, R * K * n), "out_np": buf(torch.int64, R * K * Wn),
                     "flipped": buf(torch.int64, R * K), "plus": buf(torch.int64, R * K),
                     "plus_quench": buf(torch.int64, R * K), "exchanges": buf(torch.int64, R * K),
                     "passes": buf(torch.int64, R * K), "converged": buf(torch.uint8, R * K),
                     "consensus": buf(torch.uint8, R), "flag": buf(torch.int32, R * K),
                     "stats": buf(torch.int64, R * K * 4)}
        b = {k: v[1:].data_ptr() for k, v in self.bufs.items()}
        self.rc = lib.mjx_quench_exchange_jobs_ell(
            g.adj.data_ptr(), n, self.d, 0, R, K, T, 1, caps, cap2T, max_passes, s_np.data_ptr(), order_t.data_ptr(),
            0, b["rank"], b["out_np"], b["flipped"], b["plus"], b["plus_quench"], b["exchanges"], b["passes"],
            b["converged"], b["consensus"], b["flag"], b["stats"], None)
        torch.cuda.synchronize()
        self.R, self.K, self.Wn = R, K, Wn

    def guards_intact(self):
        return all(int(v[0]) == self.GUARD and int(v[-1]) == self.GUARD for v in self.bufs.values())

    def get(self, key):
        return self.bufs[key][1:-1].cpu().numpy()

    def conf(self):
        words = self.get("out_np").view(np.uint64).reshape(self.R * self.K, self.Wn)
        bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1))
        bits = bits.reshape(self.R * self.K, self.Wn * 64)
        return np.where(bits[:, :self.n] == 1, 1, -1), bool(bits[:, self.n:].any())


def _ell_caps(lib, n, d, T):
    caps = (ctypes.c_int64 * (T + 1))()
    assert lib.mjx_ell_ball_bound(n, d, T, caps) == 0
    return caps


@pytest.mark.parametrize("n", [33, 65])
def test_dirty_padding_bits_through_the_abi(mjx_mod, n):
    """Padding bits of s_np are ignored, out_np comes back with them 0, every output array is written
    within its bounds, and the stats count what the oracle's walk implies."""
    d, T, R, K = 4, 2, 2, 2
    adj = mjx_mod.random_regular_graph(d, n, seed=120 + n)
    S = np.ones((R, n), np.int64)
    S[1, ::2] = -1
    orders = _orders(1, n, K)[0]
    want = xo.exchange_jobs(qo.step_ell(adj), S, T, orders)
    assert want["consensus"].tolist() == [True, False] and want["exchanges"][0].max() >= 1
    lib = mjx_mod.load_library()
    run = _Abi(mjx_mod, adj, S, T, orders, _ell_caps(lib, n, d, T), _ell_caps(lib, n, d, 2 * T)[2 * T],
               dirty_padding=True)
    assert run.rc == 0 and run.guards_intact()
    assert not run.get("flag").any() and run.get("consensus").tolist() == [1, 0]
    conf, padding = run.conf()
    assert not padding
    assert np.array_equal(conf, want["conf"].reshape(R * K, n))
    for key in ("flipped", "plus_quench", "exchanges", "passes"):
        assert np.array_equal(run.get(key), want[key].reshape(-1)), key
    assert np.array_equal(run.get("converged"), want["converged"].reshape(-1).astype(np.uint8))
    assert np.array_equal(2 * run.get("plus") - n, want["sums"].reshape(-1))
    stats = run.get("stats").reshape(R * K, 4)
    assert (stats[:K, 0] >= want["exchanges"][0]).all() and (stats[:K, 1] >= 2 * want["exchanges"][0]).all()
    assert not stats[K:, :2].any(), "a start without consensus adds nothing"


def test_wrong_caps_raise_the_jobs_flag_and_write_nothing_out_of_bounds(mjx_mod):
    """A candidate list past cap2T, or a light-cone list past its cap, stops the job with flag bit 0; a
    job without consensus builds no list and keeps flag 0."""
    n, d, T, R = 70, 3, 2, 2
    adj = mjx_mod.random_regular_graph(d, n, seed=120)
    S = np.ones((R, n), np.int64)
    S[1, ::2] = -1
    orders = np.arange(n)[None, :]
    lib = mjx_mod.load_library()
    right = _ell_caps(lib, n, d, T)
    # the right light-cone caps, so the quench pass runs and leaves -1 nodes; a candidate list of 2 entries
    # cannot hold the ball of the first add
    run = _Abi(mjx_mod, adj, S, T, orders, right, 2)
    assert run.rc == 0 and run.guards_intact()
    assert run.get("flag").tolist() == [1, 0] and run.get("consensus").tolist() == [1, 0]
    assert run.get("flipped")[0] > 0
    # light-cone caps of 1: the first try of the quench pass stops the job
    run = _Abi(mjx_mod, adj, S, T, orders, (ctypes.c_int64 * (T + 1))(1, 1, 1), 1000)
    assert run.rc == 0 and run.guards_intact()
    assert run.get("flag").tolist() == [1, 0] and run.get("consensus").tolist() == [1, 0]


# ---- 4. a graph per start ------------------------------------------------------------------
def test_a_graph_per_start(mjx_mod):
    n, d, T, K = 96, 4, 3, 2
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    S = qo.random_starts(4, n, 0.7, seed=41)
    S[3] = 1
    orders = _orders(4, n, K)
    steps = [qo.step_ell(graphs[r]) for r in range(4)]
    want = xo.exchange_jobs(steps, S, T, orders)
    assert want["consensus"][3] and want["exchanges"].sum() > 0
    res = mjx_mod.quench_exchange(graphs, S, T, 1, restarts=K, orders=orders, keep_all=True)
    _assert_jobs(res, want, S)
    # the graph matters: start 3 on graph 0 ends elsewhere
    other = xo.exchange(steps[0], S[3], T, orders[3, 0])
    assert not np.array_equal(other["conf"], want["conf"][3, 0])
    with pytest.raises(ValueError, match="4 graphs for 3 starts"):
        mjx_mod.quench_exchange(graphs, S[:3], T, 1, restarts=K, orders=orders[:3])


# ---- 5. max_passes ---------------------------------------------------------------------------
def test_one_pass_of_a_job_that_commits_in_it_is_not_converged(mjx_mod):
    name = "rrg_d4_n96_T3"
    full, want = _want(name), _want(name, 1)
    _, _, S, T = _case(name)
    busy = full["exchanges"] > 0
    assert busy.any() and (want["exchanges"][busy] > 0).all(), "an exchange of the run is one of its first pass"
    assert not want["converged"][busy].any() and (want["passes"][busy] == 1).all()
    assert (want["sums"] > full["sums"]).any(), "somewhere a later pass has to matter"
    res = mjx_mod.quench_exchange(_graph(name), S, T, 1, restarts=K_CASE, orders=_orders(*S.shape), max_passes=1,
                                  keep_all=True)
    _assert_jobs(res, want, S)


# ---- 6. the ends of the T range ------------------------------------------------------------------
def test_T0_returns_the_start_and_T4_is_refused(mjx_mod):
    name = "rrg_d3_n200_T2"
    _, _, S, _ = _case(name)
    S = S.copy()
    S[5] = 1                                        # T = 0: consensus means all +1 already
    res = mjx_mod.quench_exchange(_graph(name), S, 1, 0, restarts=2, seed=1, keep_all=True)
    assert np.array_equal(res["conf_best"], S) and not res["flipped"].any() and not res["exchanges"].any()
    assert np.array_equal(res["conf"], np.repeat(S[:, None, :], 2, axis=1))
    cons = (S == 1).all(axis=1)
    assert np.array_equal(res["consensus"], cons) and cons[5]
    assert res["converged"].all() and np.array_equal(res["passes"], np.repeat(cons[:, None], 2, axis=1).astype(np.int64))
    assert np.array_equal(res["mag_quench"], res["mag"])
    for p, c in ((4, 1), (3, 2), (7, 1)):
        with pytest.raises(ValueError):
            mjx_mod.quench_exchange(_graph(name), S, p, c)


# ---- 7. against the package itself -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["rrg_d4_n96_T3", "er_n300_deg3_T2"])
def test_the_quench_phase_is_quench_restarts_and_the_result_a_local_minimum(mjx_mod, name):
    _, _, S, T = _case(name)
    g = _graph(name)
    n = S.shape[1]
    orders = _orders(*S.shape)[:, :1]
    new = mjx_mod.quench_exchange(g, S, T, 1, orders=orders)
    old = mjx_mod.quench_restarts(g, S, T, 1, orders=orders)
    assert np.array_equal(new["mag_quench"], old["mag"]) and np.array_equal(new["flipped"], old["flipped"])
    assert np.array_equal(new["consensus"], old["consensus"]) and old["consensus"].any()
    assert (new["mag"] <= old["mag"]).all() and (new["mag"] < old["mag"]).any()
    # rollout says consensus, flip_gains says nothing removable
    cons = new["consensus"]
    end = mjx_mod.unpack(mjx_mod.rollout(g, mjx_mod.pack(new["conf_best"]), T, words=(S.shape[0] + 63) // 64), n,
                         S.shape[0])
    end = end.cpu().numpy() if isinstance(end, torch.Tensor) else np.asarray(end)
    assert np.array_equal((end == 1).all(axis=1), cons)
    after = mjx_mod.flip_gains(g, new["conf_best"], T, 1, gain=False)
    assert np.array_equal(after["consensus"], cons) and not after["n_removable"].any()


def test_no_result_is_lighter_than_the_census_minimum(mjx_mod):
    n, d, p = 24, 4, 3
    adj = mjx_mod.random_regular_graph(d, n, seed=7)
    floor = int(mjx_mod.census(adj, p, 1)["min_plus"][p])
    S = np.ones((1, n), np.int64)
    res = mjx_mod.quench_exchange(adj, S, p, 1, restarts=32, seed=3, keep_all=True)
    plus = (res["conf"] == 1).sum(axis=2)
    plus_q = np.rint((res["mag_quench"] * n + n) / 2).astype(np.int64)
    assert res["consensus"].all() and (plus >= floor).all() and (plus <= plus_q).all()
    print(f"census minimum {floor} of {n}; best of 32 orders: quench {plus_q.min()}, exchange descent {plus.min()}")


# ---- 8. plumbing --------------------------------------------------------------------------------------
def test_tensor_in_tensor_out_and_the_input_buffer_is_untouched(mjx_mod):
    name = "rrg_d4_n96_T3"
    want = _want(name)
    _, _, S, T = _case(name)
    n = S.shape[1]
    orders = _orders(*S.shape)
    for dtype in (torch.int8, torch.int64):
        s = torch.from_numpy(S).to("cuda", dtype)
        keep = s.clone()
        res = mjx_mod.quench_exchange(_graph(name), s, T, 1, restarts=K_CASE, orders=torch.from_numpy(orders),
                                      keep_all=True)
        assert torch.equal(s, keep)
        for key in ("mag", "flipped", "consensus", "best", "conf_best", "mag_best", "conf", "mag_quench", "exchanges",
                    "passes", "converged"):
            assert isinstance(res[key], torch.Tensor) and res[key].device == s.device, key
        assert res["conf_best"].dtype == dtype and res["conf"].dtype == torch.int8
        assert res["converged"].dtype == torch.bool and res["mag_quench"].dtype == torch.float64
        assert res["exchanges"].dtype == torch.int64 and res["passes"].dtype == torch.int64
        assert np.array_equal(res["conf"].cpu().numpy(), want["conf"])
        for key in ("flipped", "exchanges", "passes", "converged"):
            assert np.array_equal(res[key].cpu().numpy(), want[key]), key
        assert np.array_equal(res["mag_quench"].cpu().numpy(), (2 * want["plus_quench"] - n) / n)


# ---- 9. CLI ---------------------------------------------------------------------------------------------
def test_cli_exchange_in_a_fresh_process(mjx_mod, tmp_path):
    n, d, T = 96, 4, 3
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    conf = qo.random_starts(4, n, 0.7, seed=41).astype(np.float64)
    conf[3] = 1.0
    f = tmp_path / "sa.npz"
    np.savez(f, conf=conf, graphs=graphs.astype(np.float64), mag_reached=conf.mean(axis=1))
    run = subprocess.run([sys.executable, "-m", "mjx", "quench", "--in", str(f), "--p", str(T), "--c", "1",
                          "--restarts", "3", "--order-seed", "5", "--exchange", "--max-passes", "6", "--out",
                          str(f) + ".out.npz"], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(str(f) + ".out.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["best", "conf", "conf_quenched", "consensus", "converged", "exchanges", "flipped",
                                   "graphs", "mag_quench", "mag_quenched", "mag_reached", "mag_restarts", "passes"]
        want = mjx_mod.quench_exchange(graphs, conf.astype(np.int64), T, 1, restarts=3, seed=5, max_passes=6)
        assert np.array_equal(z["conf"], conf) and z["conf_quenched"].dtype == np.float64
        assert np.array_equal(z["conf_quenched"], want["conf_best"])
        assert np.array_equal(z["mag_quenched"], want["mag_best"]) and np.array_equal(z["best"], want["best"])
        assert np.array_equal(z["mag_restarts"], want["mag"]) and z["mag_restarts"].shape == (4, 3)
        for key in ("mag_quench", "exchanges", "passes", "converged", "consensus"):
            assert np.array_equal(z[key], want[key]), key
        assert z["consensus"][3] and z["exchanges"][3].sum() > 0 and (z["mag_restarts"] <= z["mag_quench"]).all()
