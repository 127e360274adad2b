"""``quench(schedule="regions")`` on the GPU: the pass in rounds must return
what the sequential pass returns, bit for bit.  The oracle is the numpy
restatement (tests/quench_oracle.py) up to n = 600 and the sequential
``quench`` at n = 1500.  Integer exact: every comparison is array_equal."""
import functools
import importlib
import subprocess
import sys

import numpy as np
import pytest
import torch

import quench_oracle as qo
from conftest import ROOT
from quench_cases import PARALLEL, R_CASE, TABLE, _case, _graph, hub_graph

pytestmark = pytest.mark.gpu


def _rows(name):
    spec = _case(name)[0]
    if spec[0] == "ell":
        return list(spec[1])
    return [spec[2][spec[1][v]:spec[1][v + 1]] for v in range(spec[1].shape[0] - 1)]


def _order(name, key):
    """None / a seed / "bfs" (from node 0, one component after the other) / "bfs_reversed" / "two_halves"
    (the first and the second half of the BFS order, far apart in the graph, taking turns)."""
    n = _case(name)[2].shape[1]
    if key is None:
        return None
    if isinstance(key, int):
        return np.random.default_rng(key).permutation(n)
    rows, seen, bfs = _rows(name), np.zeros(n, bool), []
    for root in range(n):
        if seen[root]:
            continue
        seen[root] = True
        queue = [root]
        while queue:
            bfs += queue
            nxt = []
            for v in queue:
                for k in rows[v]:
                    if not seen[k]:
                        seen[k] = True
                        nxt.append(int(k))
            queue = nxt
    bfs = np.array(bfs, dtype=np.int64)
    assert np.array_equal(np.sort(bfs), np.arange(n))
    if key == "bfs":
        return bfs
    if key == "bfs_reversed":
        return bfs[::-1].copy()
    assert key == "two_halves" and n % 2 == 0
    return np.stack([bfs[:n // 2], bfs[n // 2:]], axis=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def _want(name, key):
    """The sequential pass: the numpy oracle, with the two counts the device reports
    from the oracle's removable mask.  n = 1500: the device's sequential ``quench``."""
    import mjx
    _, step, S, T = _case(name)
    order = _order(name, key)
    if S.shape[1] > 600:
        q = mjx.quench(_graph(name), S, T, 1, order=order)
        rem, _ = qo.unpack_mask(mjx.flip_gains(_graph(name), S, T, 1, gain=False)["removable"].cpu().numpy(),
                                S.shape[1], S.shape[0])
        w = {k: q[k] for k in ("conf", "flipped", "consensus", "mag")}
        assert q["visited"] == sum(int(rem[b:b + 64].any(axis=0).sum()) for b in range(0, S.shape[0], 64))
    else:
        w = qo.quench(step, S, T, order)
        rem = _removable(name)
    w["visited"] = sum(int(rem[b:b + 64].any(axis=0).sum()) for b in range(0, S.shape[0], 64))
    w["union"] = int(rem.any(axis=0).sum())
    return w


@functools.lru_cache(maxsize=None)
def _removable(name):
    _, step, S, T = _case(name)
    return qo.flip_gains(step, S, T)["removable"]


def _assert_same(res, want, S, R=None):
    sl = slice(0, S.shape[0] if R is None else R)
    assert res["conf"].dtype == S.dtype and np.array_equal(res["conf"], want["conf"][sl])
    assert res["flipped"].dtype == np.int64 and np.array_equal(res["flipped"], want["flipped"][sl])
    assert res["consensus"].dtype == bool and np.array_equal(res["consensus"], want["consensus"][sl])
    assert res["mag"].dtype == np.float64 and np.array_equal(res["mag"], want["conf"][sl].sum(axis=1) / S.shape[1])
    if R is None:
        assert res["visited"] == want["visited"]


def _regions(mjx_mod, name, key, window=None, **kw):
    _, _, S, T = _case(name)
    return mjx_mod.quench(_graph(name), S, T, 1, order=_order(name, key), schedule="regions", window=window, **kw)


# ---- the table of cases ------------------------------------------------------
@pytest.mark.parametrize("key", [None, 3], ids=["identity", "seed3"])
@pytest.mark.parametrize("name", TABLE)
def test_regions_equal_the_sequential_oracle(mjx_mod, name, key):
    _, _, S, T = _case(name)
    want = _want(name, key)
    cons = want["consensus"]
    assert cons.sum() >= 8 and (~cons).sum() >= 8 and want["flipped"].sum() > 0, f"{name}: degenerate"
    keep = S.copy()
    n = S.shape[1]
    for window in (1, 7, None, n, 3 * n):
        res = _regions(mjx_mod, name, key, window)
        _assert_same(res, want, S)
        assert np.array_equal(S, keep), "the input was written"
        assert 1 <= res["max_commits"] <= res["window"] <= want["union"]
        assert res["window"] == min(want["union"], window or res["window"])
        assert -(-want["union"] // res["window"]) <= res["rounds"] <= want["union"]
        if window == 1:
            assert res["rounds"] == want["union"] and res["max_commits"] == 1
    if name == "rrg_d4_n96_T3":
        # the 2T-ball of every node is the whole graph: no two candidates may share a round
        rows = _rows(name)
        reach = {0}
        for _ in range(2 * T):
            reach |= {int(k) for v in reach for k in rows[v]}
        assert len(reach) == n
        assert res["rounds"] == want["union"] and res["max_commits"] == 1


# ---- real parallelism ----------------------------------------------------------
def _schedule(name, key, window):
    """The commits of every round by the rule alone (ranks and distances, no dynamics): of the ``window``
    pending candidates of lowest rank those with no pending candidate of lower rank within 2T."""
    _, _, S, T = _case(name)
    order = _order(name, key)
    some = _removable(name).any(axis=0)
    cand = [int(i) for i in (np.arange(S.shape[1]) if order is None else order) if some[i]]
    rank = {i: k for k, i in enumerate(cand)}
    rows, near = _rows(name), []
    for k, i in enumerate(cand):
        ball = {i}
        for _ in range(2 * T):
            ball |= {int(x) for v in ball for x in rows[v]}
        near.append({rank[v] for v in ball if v in rank and rank[v] < k})
    pending, commits = list(range(len(cand))), []
    while pending:
        win = set(pending[:window])
        ready = {k for k in pending[:window] if not (near[k] & win)}
        pending = [k for k in pending if k not in ready]
        commits.append(len(ready))
    return commits


# the ring in identity order is left out: every node is a candidate of some replica, so each candidate
# has its predecessor next to it and the pass is a chain (the test after this one)
@pytest.mark.parametrize("name,key", [(n, k) for n in PARALLEL for k in (None, 3) if (n, k) != ("ring_n256_T3", None)])
def test_far_apart_candidates_commit_in_the_same_round(mjx_mod, name, key):
    _, _, S, T = _case(name)
    want = _want(name, key)
    cons = want["consensus"]
    assert cons.sum() >= 4 and (~cons).sum() >= 4 and want["flipped"].sum() > 0, f"{name}: degenerate"
    res = _regions(mjx_mod, name, key)
    assert res["max_commits"] >= 2 and res["rounds"] < want["union"], (res["rounds"], res["max_commits"], res["window"])
    one = _regions(mjx_mod, name, key, 1)
    assert one["rounds"] == want["union"] and one["max_commits"] == 1
    wide = _regions(mjx_mod, name, key, S.shape[1])
    assert wide["rounds"] <= res["rounds"]          # a wider window commits no candidate later
    seven = _regions(mjx_mod, name, key, 7)
    for r in (res, one, wide, seven):
        _assert_same(r, want, S)
    if S.shape[1] <= 600:                           # the rounds themselves are the rule's
        for r in (res, wide, seven):
            commits = _schedule(name, key, r["window"])
            assert (r["rounds"], r["max_commits"]) == (len(commits), max(commits)), r["window"]
    after = mjx_mod.flip_gains(_graph(name), res["conf"], T, 1, gain=False)
    assert not after["n_removable"].any() and np.array_equal(after["consensus"], cons)


def test_a_chain_of_neighbours_is_walked_one_by_one(mjx_mod):
    name = "ring_n256_T3"
    _, _, S, _ = _case(name)
    want = _want(name, None)
    cons = want["consensus"]
    assert cons.sum() >= 4 and (~cons).sum() >= 4 and want["flipped"].sum() > 0 and want["union"] == 256
    for window in (None, 7, 256):
        res = _regions(mjx_mod, name, None, window)
        _assert_same(res, want, S)
        assert (res["rounds"], res["max_commits"]) == (256, 1)


@pytest.mark.parametrize("key", ["bfs", "bfs_reversed", "two_halves"])
@pytest.mark.parametrize("name", ["rrg_d4_n600_T1", "ring_n256_T3", "er_n600_deg3_T2"])
def test_orders_that_stress_the_reservations(mjx_mod, name, key):
    _, _, S, _ = _case(name)
    want = _want(name, key)
    assert want["flipped"].sum() > 0
    for window in (None, 7, S.shape[1]):
        _assert_same(_regions(mjx_mod, name, key, window), want, S)


def test_two_calls_give_the_same_result_and_the_same_rounds(mjx_mod):
    name = "rrg_d3_n1500_T2"
    a, b = _regions(mjx_mod, name, 3), _regions(mjx_mod, name, 3)
    assert torch.equal(a["state"], b["state"]) and np.array_equal(a["flipped"], b["flipped"])
    assert (a["rounds"], a["max_commits"], a["window"]) == (b["rounds"], b["max_commits"], b["window"])
    assert a["max_commits"] >= 2


# ---- layout edges --------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 64, 70])
def test_replica_counts_and_padding(mjx_mod, R):
    name = "rrg_d3_n200_T2"
    _, _, S, T = _case(name)
    want = _want(name, 3)
    first = int(np.flatnonzero(want["consensus"])[0]) if R == 1 else 0      # R = 1: a replica that does something
    sl = slice(first, first + R)
    Ssub = np.ascontiguousarray(S[sl])
    n = S.shape[1]
    assert want["flipped"][sl].sum() > 0
    for window in (None, 4):
        res = mjx_mod.quench(_graph(name), Ssub, T, 1, seed=3, schedule="regions", window=window)
        _assert_same(res, {k: (v[sl] if isinstance(v, np.ndarray) else v) for k, v in want.items()}, Ssub, R)
        assert res["words"] == (R + 63) // 64
        conf, pad = qo.unpack_mask(res["state"].cpu().numpy(), n, R)
        assert not pad, "padding replicas of the state must stay 0"
        assert np.array_equal(np.where(conf, 1, -1), want["conf"][sl])
        seq = mjx_mod.quench(_graph(name), Ssub, T, 1, seed=3)
        assert res["visited"] == seq["visited"] and torch.equal(res["state"], seq["state"])


def test_packed_input_equals_the_spin_path(mjx_mod):
    name = "rrg_d3_n200_T2"
    _, _, S, T = _case(name)
    n = S.shape[1]
    Ssub = np.ascontiguousarray(S[:70])
    bits = mjx_mod.pack(Ssub)                       # 2 words per node, replicas 70..127 are -1
    keep = bits.clone()
    qs = mjx_mod.quench(_graph(name), Ssub, T, 1, seed=3, schedule="regions")
    qp = mjx_mod.quench(_graph(name), bits, T, 1, seed=3, words=2, schedule="regions")
    assert torch.equal(bits, keep) and "conf" not in qp and qp["words"] == 2
    assert torch.equal(qp["state"], qs["state"])
    assert (qp["rounds"], qp["window"], qp["visited"]) == (qs["rounds"], qs["window"], qs["visited"])
    assert np.array_equal(mjx_mod.unpack(qp["state"], n, 70).cpu().numpy(), _want(name, 3)["conf"][:70])
    assert np.array_equal(qp["flipped"][:70].cpu().numpy(), qs["flipped"]) and not bool(qp["flipped"][70:].any())


def test_tensor_in_tensor_out_and_the_input_buffer_is_untouched(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, _, S, T = _case(name)
    want = _want(name, None)
    for dtype in (torch.int8, torch.int64):
        s = torch.from_numpy(S).to("cuda", dtype)
        keep = s.clone()
        res = mjx_mod.quench(_graph(name), s, T, 1, schedule="regions")
        assert torch.equal(s, keep)
        assert res["conf"].is_cuda and res["conf"].dtype == dtype
        assert np.array_equal(res["conf"].cpu().numpy(), want["conf"])
        assert res["flipped"].is_cuda and np.array_equal(res["flipped"].cpu().numpy(), want["flipped"])
        assert res["consensus"].is_cuda and res["mag"].is_cuda and isinstance(res["rounds"], int)
    r = int(np.flatnonzero(want["consensus"])[0])
    one = mjx_mod.quench(_graph(name), S[r], T, 1, schedule="regions")
    assert one["conf"].shape == S[r].shape and np.array_equal(one["conf"], want["conf"][r])
    assert one["flipped"].tolist() == [want["flipped"][r]]


# ---- the scratch path ----------------------------------------------------------
def test_hub_lists_beyond_lds_go_to_scratch_and_nothing_changes(mjx_mod):
    _, _, S, T = _case("hub")
    lone = hub_graph()[2]
    g = _graph("hub")
    assert mjx_mod.SAReplicasER.ball_bound(g, T)[T] > 64, "the default LDS part must overflow too"
    want = _want("hub", 3)
    cons = want["consensus"]
    assert cons.sum() >= 8 and (~cons).sum() >= 8 and want["flipped"].sum() > 0
    for kernel in ({"lds_entries": 4}, None, {"lds_entries": 1}):
        for window in (None, 6):
            _assert_same(_regions(mjx_mod, "hub", 3, window, kernel=kernel), want, S)
    assert np.all(want["conf"][cons, lone] == 1)    # the isolated node is load-bearing where it is +1
    with pytest.raises(ValueError, match="unknown kernel options"):
        _regions(mjx_mod, "hub", 3, kernel={"split": 2})


def test_wrong_caps_raise_the_overflow_flag(mjx_mod):
    """Caps that are not the graph's: the balls and the cone's lists stop at
    them, the flag is raised, nothing is written out of bounds."""
    import ctypes
    Q = importlib.import_module("mjx.quench")
    name = "rrg_d3_n200_T2"
    _, _, S, T = _case(name)
    g = _graph(name)
    bits = mjx_mod.pack(S)
    for wrong in ((1, 4, 5), (1, 2, 13)):           # the ball of radius 2 outgrows 5; a level-1 list outgrows 2
        levels, caps, removable = Q._quench_prepare(g, bits, R_CASE, 2, T, 1, T, 0)
        assert list(caps) == [1, 4, 13]
        cand, _ = Q._union_candidates(removable, g.n, 2, None)
        with pytest.raises(mjx_mod.MjxError, match="outgrew"):
            Q._quench_regions_pass(g, levels, R_CASE, 2, T, 1, T, (ctypes.c_int64 * 3)(*wrong), removable, cand, 8, 0)
    # and the same call with the graph's caps is the oracle's result
    levels, caps, removable = Q._quench_prepare(g, bits, R_CASE, 2, T, 1, T, 0)
    cand, _ = Q._union_candidates(removable, g.n, 2, None)
    _, flipped, info = Q._quench_regions_pass(g, levels, R_CASE, 2, T, 1, T, caps, removable, cand, 8, 0)
    assert np.array_equal(flipped.cpu().numpy(), _want(name, None)["flipped"]) and info["window"] == 8
    assert np.array_equal(mjx_mod.unpack(levels[0], g.n, R_CASE).cpu().numpy(), _want(name, None)["conf"])


# ---- the ends of the T range ---------------------------------------------------
def test_T0_flips_nothing_in_no_rounds_and_T7_is_refused(mjx_mod):
    name = "rrg_d4_n200_T1"
    _, _, S, _ = _case(name)
    S = S.copy()
    S[5] = 1                                        # T = 0: consensus means all +1 already
    q = mjx_mod.quench(_graph(name), S, 1, 0, schedule="regions")
    assert np.array_equal(q["conf"], S) and not q["flipped"].any() and q["consensus"][5]
    assert (q["rounds"], q["max_commits"], q["visited"]) == (0, 0, 0) and q["window"] == 1
    for p, c in ((7, 1), (6, 2), (4, 4)):
        with pytest.raises(ValueError):
            mjx_mod.quench(_graph(name), S, p, c, schedule="regions")


def test_T6_against_the_oracle(mjx_mod):
    name = "rrg_d3_n64_T6"
    _, _, S, T = _case(name)
    assert T == 6
    for key in (None, 3):
        want = _want(name, key)
        assert want["consensus"].sum() >= 8 and want["flipped"].sum() > 0
        for window in (None, 5):
            res = mjx_mod.quench(_graph(name), S, 5, 2, order=_order(name, key), schedule="regions", window=window)
            _assert_same(res, want, S)


def test_an_asymmetric_graph_is_refused(mjx_mod):
    adj = mjx_mod.random_regular_graph(3, 20, seed=0).copy()
    a, b = (adj[0, 0], adj[1, 0]) if adj[0, 0] != adj[1, 0] else (adj[0, 0], adj[1, 1])
    adj[0, 0], adj[1, 0] = b, a
    with pytest.raises(ValueError, match="symmetric"):
        mjx_mod.quench(adj, np.ones(20, np.int64), 1, 1, schedule="regions")


# ---- CLI -------------------------------------------------------------------------
def test_cli_runs_the_regions_schedule_in_a_fresh_process(mjx_mod, tmp_path):
    name = "er_n300_deg3_T2"
    _, _, S, T = _case(name)
    spec = _case(name)[0]
    f = tmp_path / "er.npz"
    np.savez(f, conf=S[:40].astype(np.float64), row_ptr=spec[1], col=spec[2], n_iso=np.int64(0))
    run = subprocess.run([sys.executable, "-m", "mjx", "quench", "--in", str(f), "--p", str(T), "--c", "1",
                          "--order-seed", "3", "--schedule", "regions", "--window", "5", "--out", str(f) + ".out.npz"],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    want = _want(name, 3)
    with np.load(str(f) + ".out.npz", allow_pickle=False) as z:
        assert np.array_equal(z["conf_quenched"], want["conf"][:40]) and z["conf_quenched"].dtype == np.float64
        assert np.array_equal(z["flipped"], want["flipped"][:40])
        assert np.array_equal(z["consensus"], want["consensus"][:40])
        assert np.array_equal(z["mag_quenched"], want["conf"][:40].sum(axis=1) / S.shape[1])
