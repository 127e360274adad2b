"""``quench_anneal`` on the GPU: every (start, order) job against the numpy
restatement of the walk (tests/quench_anneal_oracle.py), which decides every
drop with a rollout of the whole graph.  Integer exact: every comparison is
array_equal.  The oracle's results are computed once per case and shared."""
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import quench_anneal_oracle as ao
import quench_cases
import quench_oracle as qo
from conftest import ROOT
from quench_cases import _graph, hub_graph

pytestmark = pytest.mark.gpu

R_CASE, K_CASE = 16, 2
ORDER_SEED, ANNEAL_SEED = 5, 7
BETA = (1.0, 5.0)
# name -> sweeps
SWEEPS = {"rrg_d4_n96_T3": 16, "rrg_d3_n200_T2": 8, "rrg_d5_n120_T2": 12, "er_n300_deg3_T2": 8}
MOVES = ("adds", "drops", "refused")


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (graph as the package takes it, oracle step, S (R_CASE, n), T).  Shared: never written."""
    spec, step, S, T = quench_cases._case(name)
    return spec, step, S[:R_CASE], T


def _orders(R, n, K=K_CASE, seed=ORDER_SEED):
    """The seed rule written out: job (r, k) walks default_rng([seed, r, k]).permutation(n)."""
    return np.stack([np.stack([np.random.default_rng([seed, r, k]).permutation(n) for k in range(K)])
                     for r in range(R)])


def _thr(U, beta=BETA):
    return ao.thresholds(np.linspace(beta[0], beta[1], U))


@functools.lru_cache(maxsize=None)
def _want(name):
    _, step, S, T = _case(name)
    return ao.anneal_jobs(step, S, T, _orders(*S.shape), _thr(SWEEPS[name]), ANNEAL_SEED)


def _plus(want):
    return (want["conf"] == 1).sum(axis=2)


def _not_degenerate(want, name, U):
    """The conditions a case must meet in the oracle before anything is compared."""
    cons = want["consensus"]
    plus = _plus(want)
    assert (plus[cons] < want["plus_quench"][cons]).sum() >= 2, f"{name}: the walk has to improve two jobs"
    assert (~cons).sum() >= 1, f"{name}: every start is at consensus"
    assert ((want["best_sweep"] > 0) & (want["best_sweep"] < U)).any(), f"{name}: no best sweep inside the run"
    assert ((want["moves"][:, :, 0] > 0) & want["drop_after_add"]).any(), f"{name}: no drop after an add"


def _assert_jobs(res, want, S, trace=True):
    R, n = S.shape
    K = want["conf"].shape[1]
    assert res["conf"].dtype == np.int8 and res["conf"].shape == (R, K, n)
    assert np.array_equal(res["conf"], want["conf"])
    for key in ("flipped", "best_sweep"):
        assert res[key].dtype == np.int64 and res[key].shape == (R, K) and np.array_equal(res[key], want[key]), key
    for j, key in enumerate(MOVES):
        assert res[key].dtype == np.int64 and np.array_equal(res[key], want["moves"][:, :, j]), key
    for key, src in (("mag_quench", "plus_quench"), ("mag_best_sweep", "plus_best")):
        assert res[key].dtype == np.float64 and np.array_equal(res[key], (2 * want[src] - n) / n), key
    if trace:
        assert res["trace"].dtype == np.int32 and np.array_equal(res["trace"], want["trace"])
    else:
        assert "trace" not in res
    assert res["mag"].dtype == np.float64 and np.array_equal(res["mag"], want["sums"] / n)
    assert res["consensus"].dtype == bool and np.array_equal(res["consensus"], want["consensus"])
    cons = want["consensus"]
    assert np.array_equal(res["conf"][~cons], np.repeat(S[~cons][:, None, :], K, axis=1))
    for key in MOVES + ("best_sweep", "flipped"):
        assert not res[key][~cons].any(), key
    assert (res["mag"] <= res["mag_best_sweep"]).all() and (res["mag_best_sweep"] <= res["mag_quench"]).all()
    best = np.argmin(want["sums"], axis=1)
    assert np.array_equal(res["best"], best)
    assert np.array_equal(res["conf_best"], want["conf"][np.arange(R), best])
    assert np.array_equal(res["mag_best"], res["mag"][np.arange(R), best])


# ---- 1. the table -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_every_job_equals_the_oracle(mjx_mod, name):
    U = SWEEPS[name]
    want = _want(name)
    _not_degenerate(want, name, U)
    _, _, S, T = _case(name)
    keep = S.copy()
    res = mjx_mod.quench_anneal(_graph(name), S, T, 1, U, beta=BETA, restarts=K_CASE, orders=_orders(*S.shape),
                                anneal_seed=ANNEAL_SEED, trace=True, keep_all=True)
    assert np.array_equal(S, keep), "the input was written"
    _assert_jobs(res, want, S)
    cons = want["consensus"]
    print(f"{name}: +1 spins after quench {want['plus_quench'][cons].mean():.1f}, after {U} sweeps and the closing "
          f"pass {_plus(want)[cons].mean():.1f}")


def test_the_closing_pass_drops_something(mjx_mod):
    """A lightest sweep end that is no local minimum: the closing pass goes below plus_best.  Five jobs of
    its own, found on the CPU: on the first five starts of rrg_d4_n96_T3, 12 sweeps at beta 1 -> 3 under
    anneal seed 3, the walk of start 4 is lightest at 53 and its closing pass ends at 51."""
    name = "rrg_d4_n96_T3"
    _, step, S, T = _case(name)
    S, U, beta, seed = S[:5], 12, (1.0, 3.0), 3
    orders = _orders(5, S.shape[1], 1)
    want = ao.anneal_jobs(step, S, T, orders, _thr(U, beta), seed)
    closing = _plus(want) < want["plus_best"]
    assert closing.sum() >= 1, "the oracle's closing pass drops nothing in this case"
    res = mjx_mod.quench_anneal(_graph(name), S, T, 1, U, beta=beta, seed=ORDER_SEED, anneal_seed=seed,
                                keep_all=True)                               # the seed rule, no trace
    _assert_jobs(res, want, S, trace=False)
    assert np.array_equal(res["mag"] < res["mag_best_sweep"], closing)


# ---- 2. edges of the schedule ---------------------------------------------------
def test_no_sweeps_is_quench_restarts(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, _, S, T = _case(name)
    orders = _orders(*S.shape)
    new = mjx_mod.quench_anneal(_graph(name), S, T, 1, 0, restarts=K_CASE, orders=orders, trace=True, keep_all=True)
    old = mjx_mod.quench_restarts(_graph(name), S, T, 1, restarts=K_CASE, orders=orders, keep_all=True)
    for key in ("conf", "mag", "flipped", "consensus", "best", "conf_best", "mag_best"):
        assert np.array_equal(new[key], old[key]), key
    assert old["consensus"].any() and np.array_equal(new["mag_quench"], old["mag"])
    assert np.array_equal(new["mag_best_sweep"], old["mag"])
    assert new["trace"].shape == (R_CASE, K_CASE, 0)
    for key in MOVES + ("best_sweep",):
        assert not new[key].any(), key


def test_thresholds_of_zero_never_add_and_of_all_ones_always_add(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, step, S, T = _case(name)
    S, U = S[:8], 6
    orders = _orders(*S.shape)
    for value in (0, 2 ** 32 - 1):
        thr = np.full(U, value, np.uint32)
        want = ao.anneal_jobs(step, S, T, orders, thr, ANNEAL_SEED)
        assert want["consensus"].any()
        res = mjx_mod.quench_anneal(_graph(name), S, T, 1, U, thresholds=thr, restarts=K_CASE, orders=orders,
                                    anneal_seed=ANNEAL_SEED, trace=True, keep_all=True)
        _assert_jobs(res, want, S)
        cons = want["consensus"]
        if value == 0:
            # a quench result has nothing to drop and nothing is ever added: the state never moves
            assert not res["adds"].any() and not res["drops"].any() and res["refused"][cons].all()
            assert np.array_equal(res["mag"], res["mag_quench"])
        else:
            # 2^32 - 1: every -1 proposal but the word 2^32 - 1 itself is added
            assert (res["adds"][cons] > 0).all() and (res["trace"][cons][:, :, 0] > want["plus_quench"][cons]).all()
    with pytest.raises(ValueError, match="not both"):
        mjx_mod.quench_anneal(_graph(name), S, T, 1, U, beta=(1.0, 2.0), thresholds=thr)


def test_same_seed_same_result_other_seed_another(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, _, S, T = _case(name)
    kw = dict(beta=BETA, restarts=K_CASE, seed=ORDER_SEED, trace=True, keep_all=True)
    a = mjx_mod.quench_anneal(_graph(name), S, T, 1, SWEEPS[name], anneal_seed=ANNEAL_SEED, **kw)
    b = mjx_mod.quench_anneal(_graph(name), S, T, 1, SWEEPS[name], anneal_seed=ANNEAL_SEED, **kw)
    c = mjx_mod.quench_anneal(_graph(name), S, T, 1, SWEEPS[name], anneal_seed=ANNEAL_SEED + (1 << 32), **kw)
    _assert_jobs(a, _want(name), S)
    for key in ("conf", "trace", "best_sweep") + MOVES:
        assert np.array_equal(a[key], b[key]), key
    assert not np.array_equal(a["trace"], c["trace"]), "the high word of the seed is part of the key"
    assert np.array_equal(a["mag_quench"], c["mag_quench"])


def test_a_job_keeps_its_stream_whatever_R_and_K_are(mjx_mod):
    name = "rrg_d4_n96_T3"
    want = _want(name)
    _, _, S, T = _case(name)
    n, U = S.shape[1], SWEEPS[name]
    assert want["consensus"][:5].any()
    fewer = mjx_mod.quench_anneal(_graph(name), S[:5], T, 1, U, beta=BETA, orders=_orders(5, n, 1),
                                  anneal_seed=ANNEAL_SEED, trace=True, keep_all=True)
    more = mjx_mod.quench_anneal(_graph(name), S[:9], T, 1, U, beta=BETA, restarts=3, orders=_orders(9, n, 3),
                                 anneal_seed=ANNEAL_SEED, trace=True, keep_all=True)
    for key, src in (("conf", "conf"), ("trace", "trace"), ("best_sweep", "best_sweep"), ("flipped", "flipped")):
        assert np.array_equal(fewer[key], want[src][:5, :1]), key
        assert np.array_equal(more[key][:, :2], want[src][:9]), key
    for j, key in enumerate(MOVES):
        assert np.array_equal(fewer[key], want["moves"][:5, :1, j]) and \
            np.array_equal(more[key][:, :2], want["moves"][:9, :, j]), key


# ---- 3. a graph per start, hub, word edges ----------------------------------------
def test_a_graph_per_start(mjx_mod):
    n, d, T, K, U = 96, 4, 3, 2, 8
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    S = qo.random_starts(4, n, 0.7, seed=41)
    S[3] = 1
    orders = _orders(4, n, K)
    steps = [qo.step_ell(graphs[r]) for r in range(4)]
    want = ao.anneal_jobs(steps, S, T, orders, _thr(U), ANNEAL_SEED)
    assert want["consensus"][3] and want["moves"][:, :, 0].sum() > 0
    res = mjx_mod.quench_anneal(graphs, S, T, 1, U, beta=BETA, restarts=K, orders=orders, anneal_seed=ANNEAL_SEED,
                                trace=True, keep_all=True)
    _assert_jobs(res, want, S)
    # the graph matters: start 3 on graph 0 ends elsewhere
    other = ao.anneal(steps[0], S[3], T, orders[3, 0], _thr(U), ANNEAL_SEED, r=3, k=0)
    assert not np.array_equal(other["conf"], want["conf"][3, 0])
    with pytest.raises(ValueError, match="4 graphs for 3 starts"):
        mjx_mod.quench_anneal(graphs, S[:3], T, 1, U, restarts=K, orders=orders[:3])


def test_a_hub_past_64_lanes_and_an_isolated_node(mjx_mod):
    _, step, S, T = quench_cases._case("hub80")
    rp, col, lone = hub_graph(more=80)
    assert np.diff(rp)[0] >= 70
    cons = np.flatnonzero((qo.end_state(step, S[:8], T) == 1).all(axis=1))[:2]
    assert cons.size == 2
    S, U = S[cons], 4
    orders = _orders(2, 300, 1)
    want = ao.anneal_jobs(step, S, T, orders, _thr(U), ANNEAL_SEED)
    assert want["consensus"].all() and (want["moves"][:, :, :2] > 0).all()
    res = mjx_mod.quench_anneal(_graph("hub80"), S, T, 1, U, beta=BETA, orders=orders, anneal_seed=ANNEAL_SEED,
                                trace=True, keep_all=True)
    _assert_jobs(res, want, S)
    # the isolated node keeps its spin: it is never dropped, and never added since it is +1
    assert (S[:, lone] == 1).all() and (res["conf"][:, :, lone] == 1).all()


@pytest.mark.parametrize("n", [33, 64, 65])
def test_word_edges_and_padding_bits(mjx_mod, n):
    d = 3 if (n * 3) % 2 == 0 else 4
    T, U = 2, 10
    adj = mjx_mod.random_regular_graph(d, n, seed=50 + n)
    S = qo.random_starts(8, n, 0.7, seed=60 + n)
    S[0] = 1                                        # a start that is at consensus for sure
    orders = _orders(8, n)
    want = ao.anneal_jobs(qo.step_ell(adj), S, T, orders, _thr(U), ANNEAL_SEED)
    assert want["consensus"][0] and want["moves"][:, :, :2].sum(axis=(0, 1)).min() > 0
    res = mjx_mod.quench_anneal(adj, S, T, 1, U, beta=BETA, restarts=K_CASE, orders=orders, anneal_seed=ANNEAL_SEED,
                                trace=True, keep_all=True)
    _assert_jobs(res, want, S)
    one = mjx_mod.quench_anneal(adj, S[0], T, 1, U, beta=BETA, restarts=K_CASE, orders=orders[0],
                                anneal_seed=ANNEAL_SEED, keep_all=True)
    assert one["conf_best"].shape == (n,) and one["conf"].shape == (1, K_CASE, n)
    assert np.array_equal(one["conf"][0], want["conf"][0]) and one["adds"].shape == (1, K_CASE)
    words = res["state_best"].cpu().numpy().view(np.uint64)
    Wn = (n + 63) // 64
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(8, Wn * 64)
    assert not bits[:, n:].any(), "padding bits of the packed output must be 0"
    assert np.array_equal(np.where(bits[:, :n] == 1, 1, -1), res["conf_best"])


class _Abi:
    """One call of mjx_quench_anneal_jobs_ell on poisoned outputs with a guard word at both ends."""
    GUARD = 0x5A

    def __init__(self, mjx_mod, adj, S, T, orders, caps, thr, seed, dirty_padding=False):
        self.n, self.d = adj.shape
        n, R, K, U = self.n, S.shape[0], orders.shape[0], len(thr)
        g = mjx_mod.Graph.ell(adj)
        lib = mjx_mod.load_library()
        Wn = (n + 63) // 64
        s_np = torch.stack([mjx_mod.pack(S[r]) for r in range(R)]).reshape(R, Wn)
        if dirty_padding and n % 64:
            s_np[:, -1] |= ~((1 << (n % 64)) - 1)   # every bit past n set
        dev = s_np.device
        order_t = torch.from_numpy(orders.astype(np.int32)).to(dev)
        thr_t = torch.from_numpy(np.asarray(thr, np.uint32).view(np.int32)).to(dev)

        def buf(dtype, count):
            return torch.full((count + 2,), self.GUARD, dtype=dtype, device=dev)

        self.bufs = {"out_np": buf(torch.int64, R * K * Wn), "flipped": buf(torch.int64, R * K),
                     "plus": buf(torch.int64, R * K), "plus_quench": buf(torch.int64, R * K),
                     "plus_best": buf(torch.int64, R * K), "best_sweep": buf(torch.int64, R * K),
                     "moves": buf(torch.int64, R * K * 3), "trace": buf(torch.int32, R * K * U),
                     "consensus": buf(torch.uint8, R), "flag": buf(torch.int32, R * K)}
        b = {k: v[1:].data_ptr() for k, v in self.bufs.items()}
        self.rc = lib.mjx_quench_anneal_jobs_ell(
            g.adj.data_ptr(), n, self.d, 0, R, K, T, 1, caps, U, thr_t.data_ptr(), seed, s_np.data_ptr(),
            order_t.data_ptr(), 0, b["out_np"], b["flipped"], b["plus"], b["plus_quench"], b["plus_best"],
            b["best_sweep"], b["moves"], b["trace"], b["consensus"], b["flag"], None)
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


@pytest.mark.parametrize("n", [33, 64, 65])
def test_dirty_padding_bits_through_the_abi(mjx_mod, n):
    """Padding bits of s_np are ignored, out_np comes back with them 0, and every output array, the trace
    among them, is written within its bounds."""
    d, T, R, K, U = 4, 2, 2, 2, 9
    adj = mjx_mod.random_regular_graph(d, n, seed=120 + n)
    S = np.ones((R, n), np.int64)
    S[1, ::2] = -1
    orders = _orders(1, n, K)[0]
    thr = _thr(U)
    want = ao.anneal_jobs(qo.step_ell(adj), S, T, orders, thr, ANNEAL_SEED)
    assert want["consensus"].tolist() == [True, False] and want["moves"][0, :, :2].min() >= 1
    lib = mjx_mod.load_library()
    run = _Abi(mjx_mod, adj, S, T, orders, _ell_caps(lib, n, d, T), thr, ANNEAL_SEED, dirty_padding=True)
    assert run.rc == 0 and run.guards_intact()
    assert not run.get("flag").any() and run.get("consensus").tolist() == [1, 0]
    conf, padding = run.conf()
    assert not padding
    assert np.array_equal(conf, want["conf"].reshape(R * K, n))
    for key in ("flipped", "plus_quench", "plus_best", "best_sweep", "moves", "trace"):
        assert np.array_equal(run.get(key), want[key].reshape(-1)), key
    assert np.array_equal(2 * run.get("plus") - n, want["sums"].reshape(-1))
    assert (run.get("trace").reshape(R, K, U)[1] == (S[1] == 1).sum()).all(), "no consensus: a flat trace"


def test_wrong_caps_raise_the_jobs_flag_and_write_nothing_out_of_bounds(mjx_mod):
    """A light-cone list past its cap stops the job with flag bit 0; a job without consensus builds no
    list and keeps flag 0."""
    n, d, T, R = 70, 3, 2, 2
    adj = mjx_mod.random_regular_graph(d, n, seed=120)
    S = np.ones((R, n), np.int64)
    S[1, ::2] = -1
    orders = np.arange(n)[None, :]
    run = _Abi(mjx_mod, adj, S, T, orders, (ctypes.c_int64 * (T + 1))(1, 1, 1), _thr(4), ANNEAL_SEED)
    assert run.rc == 0 and run.guards_intact()
    assert run.get("flag").tolist() == [1, 0] and run.get("consensus").tolist() == [1, 0]


# ---- 4. the ends of the T range and of the LDS ------------------------------------------
def test_T0_refuses_every_proposal(mjx_mod):
    name = "rrg_d3_n200_T2"
    _, step, S, _ = _case(name)
    S = S[:6].copy()
    S[5] = 1                                        # T = 0: consensus means all +1 already
    n, U = S.shape[1], 3
    want = ao.anneal_jobs(step, S, 0, _orders(6, n), _thr(U), ANNEAL_SEED)
    res = mjx_mod.quench_anneal(_graph(name), S, 1, 0, U, beta=BETA, restarts=2, seed=ORDER_SEED,
                                anneal_seed=ANNEAL_SEED, trace=True, keep_all=True)
    _assert_jobs(res, want, S)
    cons = (S == 1).all(axis=1)
    assert np.array_equal(res["consensus"], cons) and cons[5]
    assert np.array_equal(res["conf"], np.repeat(S[:, None, :], 2, axis=1))
    assert (res["refused"][5] == U * n).all() and not res["adds"].any() and not res["drops"].any()


def test_T6_runs_and_T7_is_refused(mjx_mod):
    name = "rrg_d3_n64_T6"
    spec, step, S, T = quench_cases._case(name)
    assert T == 6
    S, U = S[:8], 6
    orders = _orders(8, 64, 1)
    want = ao.anneal_jobs(step, S, T, orders, _thr(U), ANNEAL_SEED)
    assert want["consensus"].any() and want["moves"][:, :, :2].sum(axis=(0, 1)).min() > 0
    res = mjx_mod.quench_anneal(_graph(name), S, 6, 1, U, beta=BETA, orders=orders, anneal_seed=ANNEAL_SEED,
                                trace=True, keep_all=True)
    _assert_jobs(res, want, S)
    for p, c in ((7, 1), (4, 4), (0, 0)):
        with pytest.raises(ValueError, match="p \\+ c - 1"):
            mjx_mod.quench_anneal(_graph(name), S, p, c, U)


def test_a_shape_past_the_lds_is_refused(mjx_mod):
    """n = 1e5, d = 4, T = 3: the quench job fits 64 KiB, the snapshot bitmap on top of it does not."""
    big = 100_000
    i = np.arange(big)
    lattice = np.stack([(i - 1) % big, (i + 1) % big, (i - 2) % big, (i + 2) % big], axis=1)
    with pytest.raises(ValueError, match="quench_anneal: .* does not fit"):
        mjx_mod.quench_anneal(lattice, np.ones(big, np.int64), 3, 1, 2)
    lib = mjx_mod.load_library()
    caps = _ell_caps(lib, big, 4, 3)
    a = ctypes.c_void_p(64)
    assert lib.mjx_quench_jobs_lds(big, 3, caps) > 0 and lib.mjx_quench_anneal_jobs_lds(big, 3, caps) == -1
    assert lib.mjx_quench_anneal_jobs_ell(a, big, 4, 0, 1, 1, 3, 1, caps, 2, a, 0, a, a, 0, a, a, a, a, a, a, a, None,
                                          a, a, None) == 1


# ---- 5. against the package itself -----------------------------------------------------------
@pytest.mark.parametrize("name", ["rrg_d4_n96_T3", "er_n300_deg3_T2"])
def test_the_result_is_a_consensus_local_minimum_no_heavier_than_quench_restarts(mjx_mod, name):
    _, _, S, T = _case(name)
    g = _graph(name)
    n = S.shape[1]
    orders = _orders(*S.shape)
    new = mjx_mod.quench_anneal(g, S, T, 1, SWEEPS[name], beta=BETA, restarts=K_CASE, orders=orders,
                                anneal_seed=ANNEAL_SEED, keep_all=True)
    old = mjx_mod.quench_restarts(g, S, T, 1, restarts=K_CASE, orders=orders)
    assert np.array_equal(new["mag_quench"], old["mag"]) and np.array_equal(new["flipped"], old["flipped"])
    assert np.array_equal(new["consensus"], old["consensus"]) and old["consensus"].any()
    assert (new["mag"] <= old["mag"]).all() and (new["mag"] < old["mag"]).any()
    # rollout says consensus, flip_gains says nothing removable: of every job's result
    cons = np.repeat(new["consensus"], K_CASE)
    conf = new["conf"].reshape(-1, n).astype(np.int64)
    J = conf.shape[0]
    end = mjx_mod.unpack(mjx_mod.rollout(g, mjx_mod.pack(conf), T, words=(J + 63) // 64), n, J)
    end = end.cpu().numpy() if isinstance(end, torch.Tensor) else np.asarray(end)
    assert np.array_equal((end == 1).all(axis=1), cons)
    after = mjx_mod.flip_gains(g, conf, T, 1, gain=False)
    assert np.array_equal(after["consensus"], cons) and not after["n_removable"].any()


@pytest.mark.parametrize("d,optimum,jobs,reached", [(3, 10, 7, 5), (4, 9, 13, 6)])
def test_against_the_exact_optimum_of_an_18_node_graph(mjx_mod, d, optimum, jobs, reached):
    """No job falls below the brute-force optimum, and some job reaches it, where every quench stays above."""
    n, T, U = 18, 3, 128
    adj = mjx_mod.random_regular_graph(d, n, seed=1)
    step = qo.step_ell(adj)
    assert ao.optimum(step, n, T) == optimum
    assert int(mjx_mod.census(adj, T, 1)["min_plus"][T]) == optimum
    S = qo.random_starts(16, n, 0.6, 58)
    orders = _orders(16, n, 1)
    want = ao.anneal_jobs(step, S, T, orders, ao.thresholds(np.linspace(1.5, 6.0, U)), ANNEAL_SEED)
    cons = want["consensus"]
    assert cons.sum() == jobs and (_plus(want)[cons] == optimum).sum() == reached
    res = mjx_mod.quench_anneal(adj, S, T, 1, U, orders=orders, anneal_seed=ANNEAL_SEED, trace=True, keep_all=True)
    _assert_jobs(res, want, S)
    plus = (res["conf"] == 1).sum(axis=2)[cons]
    assert (plus >= optimum).all() and (plus == optimum).sum() >= 1
    plus_q = np.rint((res["mag_quench"][cons] * n + n) / 2).astype(np.int64)
    print(f"d = {d}: optimum {optimum}; quench {plus_q.ravel().tolist()}, anneal {plus.ravel().tolist()}")


# ---- 6. plumbing ----------------------------------------------------------------------------------
def test_tensor_in_tensor_out_and_the_input_buffer_is_untouched(mjx_mod):
    name = "rrg_d4_n96_T3"
    want = _want(name)
    _, _, S, T = _case(name)
    n = S.shape[1]
    orders = _orders(*S.shape)
    for dtype in (torch.int8, torch.int64):
        s = torch.from_numpy(S).to("cuda", dtype)
        keep = s.clone()
        res = mjx_mod.quench_anneal(_graph(name), s, T, 1, SWEEPS[name], beta=BETA, restarts=K_CASE,
                                    orders=torch.from_numpy(orders), anneal_seed=ANNEAL_SEED, trace=True,
                                    keep_all=True)
        assert torch.equal(s, keep)
        for key in ("mag", "flipped", "consensus", "best", "conf_best", "mag_best", "conf", "mag_quench",
                    "mag_best_sweep", "best_sweep", "trace") + MOVES:
            assert isinstance(res[key], torch.Tensor) and res[key].device == s.device, key
        assert res["conf_best"].dtype == dtype and res["conf"].dtype == torch.int8
        assert res["trace"].dtype == torch.int32 and res["mag_best_sweep"].dtype == torch.float64
        assert np.array_equal(res["conf"].cpu().numpy(), want["conf"])
        assert np.array_equal(res["trace"].cpu().numpy(), want["trace"])
        for j, key in enumerate(MOVES):
            assert res[key].dtype == torch.int64 and np.array_equal(res[key].cpu().numpy(), want["moves"][:, :, j])
        assert np.array_equal(res["mag_quench"].cpu().numpy(), (2 * want["plus_quench"] - n) / n)


def test_cli_anneal_in_a_fresh_process(mjx_mod, tmp_path):
    n, d, T = 96, 4, 3
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    conf = qo.random_starts(4, n, 0.7, seed=41).astype(np.float64)
    conf[3] = 1.0
    f = tmp_path / "sa.npz"
    np.savez(f, conf=conf, graphs=graphs.astype(np.float64), mag_reached=conf.mean(axis=1))
    run = subprocess.run([sys.executable, "-m", "mjx", "quench", "--in", str(f), "--p", str(T), "--c", "1",
                          "--restarts", "3", "--order-seed", "5", "--anneal", "12", "--beta", "1.0", "5.0",
                          "--anneal-seed", "7", "--out", str(f) + ".out.npz"],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(str(f) + ".out.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["adds", "best", "best_sweep", "conf", "conf_quenched", "consensus", "drops",
                                   "flipped", "graphs", "mag_best_sweep", "mag_quench", "mag_quenched", "mag_reached",
                                   "mag_restarts", "refused"]
        want = mjx_mod.quench_anneal(graphs, conf.astype(np.int64), T, 1, 12, beta=(1.0, 5.0), restarts=3, seed=5,
                                     anneal_seed=7)
        assert np.array_equal(z["conf"], conf) and z["conf_quenched"].dtype == np.float64
        assert np.array_equal(z["conf_quenched"], want["conf_best"])
        assert np.array_equal(z["mag_quenched"], want["mag_best"]) and np.array_equal(z["best"], want["best"])
        assert np.array_equal(z["mag_restarts"], want["mag"]) and z["mag_restarts"].shape == (4, 3)
        for key in ("mag_quench", "mag_best_sweep", "best_sweep", "consensus") + MOVES:
            assert np.array_equal(z[key], want[key]), key
        assert z["consensus"][3] and z["adds"][3].sum() > 0 and (z["mag_restarts"] <= z["mag_quench"]).all()
