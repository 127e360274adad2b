"""``census`` on the GPU against the brute-force oracle (tests/census_oracle.py):
counts, minimal weights and witnesses of every level.  Integer exact: every
comparison is array_equal."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import census_oracle as co
from conftest import ROOT

pytestmark = pytest.mark.gpu

# the oracle's values on networkx.random_regular_graph(d, n, seed=1), rows sorted: name -> (min_plus, counts[T]
# from the first weight that is not 0); checked only when the graph comes from there
QUOTED = {"rrg_d3_n12": ([12, 8, 8, 7], [8, 101, 132, 58, 12, 1]), "rrg_d4_n16": ([16, 10, 9, 8], None)}
REGULAR = {"rrg_d3_n12": (3, 12, 3), "rrg_d3_n16": (3, 16, 3), "rrg_d4_n16": (4, 16, 3), "rrg_d4_n14": (4, 14, 2)}


def _rrg(d, n):
    """-> (adj (n, d), from networkx?)"""
    try:
        import networkx as nx
    except ImportError:
        import mjx
        return mjx.random_regular_graph(d, n, seed=1), False
    G = nx.random_regular_graph(d, n, seed=1)
    return np.array([sorted(G[v]) for v in range(n)], dtype=np.int64), True


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([u for r in rows for u in r], dtype=np.int32)
    return rp, col


def _path(n):
    return _csr([[u for u in (v - 1, v + 1) if 0 <= u < n] for v in range(n)])


def _ring(n):
    return np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1)


def _complete(n):
    return np.array([[u for u in range(n) if u != v] for v in range(n)], dtype=np.int64)


def _star():
    """Node 0 joined to nodes 1..15, node 16 alone: degrees 15, 1 and 0."""
    return _csr([list(range(1, 16))] + [[0]] * 15 + [[]])


def _er14():
    import mjx
    rp, col = mjx.erdos_renyi(14, 0.25, seed=4)
    assert (np.diff(rp) == 0).sum() >= 1, "the case needs a node of degree 0"
    return rp, col


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (kind, arrays, n, T, oracle census).  Shared: never written."""
    if name in REGULAR:
        d, n, T = REGULAR[name]
        adj, _ = _rrg(d, n)
        spec = ("ell", (adj,))
    elif name == "rrg_d3_n20":
        n, T = 20, 3
        spec = ("ell", (_rrg(3, 20)[0],))
    elif name == "rrg_d4_n13":
        import mjx
        n, T = 13, 3                                         # 13 * 3 is odd: d = 4
        spec = ("ell", (mjx.random_regular_graph(4, 13, seed=2),))
    elif name == "rrg_d3_n12_T6":
        n, T = 12, 6
        spec = ("ell", (_rrg(3, 12)[0],))
    elif name.startswith("path"):
        n, T = int(name[4:]), 3
        spec = ("csr", _path(n))
    elif name.startswith("ring"):
        n, T = int(name[4:]), 3
        spec = ("ell", (_ring(n),))
    elif name == "lone":
        n, T, spec = 1, 2, ("csr", _csr([[]]))
    elif name == "edge":
        n, T, spec = 2, 2, ("ell", (np.array([[1], [0]]),))
    elif name == "star":
        n, T, spec = 17, 2, ("csr", _star())
    elif name in ("K9", "K8"):
        n, T = int(name[1:]), 2
        spec = ("ell", (_complete(n),))
    elif name == "er14":
        n, T, spec = 14, 3, ("csr", _er14())
    else:
        raise KeyError(name)
    step = co.step_ell(spec[1][0]) if spec[0] == "ell" else co.step_csr(*spec[1])
    return spec[0], spec[1], n, T, co.census(step, n, T)


def _graph(mjx_mod, name, kind=None):
    k, arrays, n, _, _ = _case(name)
    if (kind or k) == "ell":
        return mjx_mod.Graph.ell(arrays[0])
    if k == "csr":
        return mjx_mod.Graph.csr(*arrays)
    return mjx_mod.Graph.csr(*_csr([list(r) for r in arrays[0].tolist()]))       # an ELL case as CSR


def _assert_census(res, want, n, T):
    assert res["counts"].dtype == np.int64 and res["counts"].shape == (T + 1, n + 1)
    assert np.array_equal(res["counts"], want["counts"])
    assert res["min_plus"].dtype == np.int64 and np.array_equal(res["min_plus"], want["min_plus"])
    assert res["witness"].dtype == np.int8 and res["witness"].shape == (T + 1, n)
    assert np.array_equal(res["witness"], want["witness"])
    assert np.array_equal(res["m_min"], (2 * want["min_plus"] - n) / n)
    with np.errstate(divide="ignore"):
        assert np.array_equal(res["entropy"], np.log(want["counts"].astype(np.float64)) / n)
    assert res["configs"] == 1 << n


# ---- 1. regular graphs, ELL and CSR ---------------------------------------------
@pytest.mark.parametrize("name", list(REGULAR))
def test_regular_graphs_equal_the_oracle_as_ell_and_as_csr(mjx_mod, name):
    _, arrays, n, T, want = _case(name)
    d = REGULAR[name][0]
    # not degenerate: something below all +1 reaches consensus, and every step adds configurations
    assert want["min_plus"][T] < n
    assert all((want["counts"][t] != want["counts"][t + 1]).any() for t in range(T))
    if name in QUOTED and _rrg(d, n)[1]:
        min_plus, tail = QUOTED[name]
        assert want["min_plus"].tolist() == min_plus
        if tail:
            assert want["counts"][T].tolist() == [0] * (n + 1 - len(tail)) + tail
    ell = mjx_mod.census(_graph(mjx_mod, name), T, 1)
    _assert_census(ell, want, n, T)
    assert np.isneginf(ell["entropy"][T][0]) and ell["entropy"][T][n] == 0.0
    _assert_census(mjx_mod.census(arrays[0], T, 1), want, n, T)           # the (n, d) array itself
    _assert_census(mjx_mod.census(_graph(mjx_mod, name, "csr"), T, 1), want, n, T)


# ---- 2. fewer nodes than pattern bits ---------------------------------------------
@pytest.mark.parametrize("name", ["lone", "edge", "path3", "path5", "path6", "path7", "ring3", "ring5", "ring6",
                                  "ring7"])
def test_fewer_nodes_than_pattern_bits(mjx_mod, name):
    _, _, n, T, want = _case(name)
    res = mjx_mod.census(_graph(mjx_mod, name), T, 1)
    _assert_census(res, want, n, T)
    assert res["counts"].sum(axis=1).max() <= 1 << n
    if name == "lone":                                       # a node of degree 0 keeps its spin
        assert res["counts"].tolist() == [[0, 1]] * (T + 1)
    if name == "ring6":                                      # the tie rule: two +1 neighbours needed, or one and +1
        assert want["counts"][1].sum() > 1


# ---- 3. lane and loop boundaries ------------------------------------------------------
def test_one_block_per_lane_and_two_trips_per_lane(mjx_mod):
    _, _, n, T, want = _case("rrg_d3_n12")
    assert 1 << (n - 6) == 64
    _assert_census(mjx_mod.census(_graph(mjx_mod, "rrg_d3_n12"), T, 1, kernel={"grid": 1}), want, n, T)
    _, _, n, T, want = _case("rrg_d4_n13")
    assert 1 << (n - 6) == 128 and want["min_plus"][T] < n
    g = _graph(mjx_mod, "rrg_d4_n13")
    for grid in (1, 2, 3):
        _assert_census(mjx_mod.census(g, T, 1, kernel={"grid": grid}), want, n, T)


@pytest.mark.parametrize("chunk", [1, 3, 64, None])
def test_the_result_does_not_depend_on_the_split(mjx_mod, chunk):
    _, _, n, T, want = _case("rrg_d3_n12")
    _assert_census(mjx_mod.census(_graph(mjx_mod, "rrg_d3_n12"), T, 1, chunk_blocks=chunk), want, n, T)


def _abi_buffers(T, n, dev, pad=8):
    """counts, keys and flag in the middle of guarded allocations."""
    cells = (T + 1) * (n + 1)
    cbuf = torch.full((cells + 2 * pad,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    kbuf = torch.full((T + 1 + 2 * pad,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    fbuf = torch.full((1 + 2 * pad,), 0x5A5A, dtype=torch.int32, device=dev)
    cbuf[pad:pad + cells] = 0
    kbuf[pad:pad + T + 1] = -1
    fbuf[pad] = 0
    return cbuf, kbuf, fbuf, pad


def _guards_intact(cbuf, kbuf, fbuf, pad):
    return all(bool((b[:pad] == v).all()) and bool((b[-pad:] == v).all())
               for b, v in ((cbuf, 0x5A5A5A5A5A5A), (kbuf, 0x5A5A5A5A5A5A), (fbuf, 0x5A5A)))


def test_two_calls_into_the_same_buffers_equal_one(mjx_mod):
    _, arrays, n, T, want = _case("rrg_d4_n16")
    g = mjx_mod.Graph.ell(arrays[0])
    lib = mjx_mod.load_library()
    B = 1 << (n - 6)
    cells = (T + 1) * (n + 1)
    cbuf, kbuf, fbuf, pad = _abi_buffers(T, n, g.adj.device)
    cp, kp, fp = cbuf.data_ptr() + 8 * pad, kbuf.data_ptr() + 8 * pad, fbuf.data_ptr() + 4 * pad
    for lo, hi in ((0, B // 3), (B // 3, B)):
        assert lib.mjx_census_ell(g.adj.data_ptr(), n, 4, T, 1, lo, hi, 0, cp, kp, fp, None) == 0
    torch.cuda.synchronize()
    assert int(fbuf[pad]) == 0 and _guards_intact(cbuf, kbuf, fbuf, pad)
    assert np.array_equal(cbuf[pad:pad + cells].cpu().numpy().reshape(T + 1, n + 1), want["counts"])
    keys = kbuf[pad:pad + T + 1].cpu().numpy()
    assert np.array_equal(keys, (want["min_plus"] << 48) | want["witness_x"])
    # the first part alone: fewer configurations, and the keys of the levels it does not reach stay all ones
    cbuf2, kbuf2, fbuf2, _ = _abi_buffers(T, n, g.adj.device)
    assert lib.mjx_census_ell(g.adj.data_ptr(), n, 4, T, 1, 0, B // 3, 0, cbuf2.data_ptr() + 8 * pad,
                              kbuf2.data_ptr() + 8 * pad, fbuf2.data_ptr() + 4 * pad, None) == 0
    torch.cuda.synchronize()
    part = cbuf2[pad:pad + cells].cpu().numpy().reshape(T + 1, n + 1)
    assert (part <= want["counts"]).all() and part.sum() < want["counts"].sum()
    assert int(kbuf2[pad]) == -1, "all +1 lies in the last block"


# ---- 4. degrees --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["star", "K9", "K8", "er14"])
def test_degrees(mjx_mod, name):
    _, arrays, n, T, want = _case(name)
    res = mjx_mod.census(_graph(mjx_mod, name), T, 1)
    _assert_census(res, want, n, T)
    if name == "star":
        # the isolated node 16 must start +1; the hub decides the leaves and the leaves the hub
        assert (res["witness"][1:, 16] == 1).all() and want["min_plus"][T] < n
    if name == "K9":
        # even degree 8, ties keep the spin: 5 of 9 up win in one step, 4 of 9 never do
        assert want["min_plus"].tolist() == [9, 5, 5] and want["counts"][1][5] == 126
    if name == "K8":
        # odd degree 7: a node with 4 of 8 up sees 3 or 4 of 7, so 4 of 8 oscillates; 5 of 8 wins
        assert want["min_plus"].tolist() == [8, 5, 5]
    if name == "er14":
        iso = np.flatnonzero(np.diff(arrays[0]) == 0)
        assert (res["witness"][:, iso] == 1).all()


# ---- 5. the ends of the T range ----------------------------------------------------------------
def test_T0_T6_and_T7(mjx_mod):
    _, _, n, T, want = _case("rrg_d3_n12_T6")
    assert T == 6
    g = _graph(mjx_mod, "rrg_d3_n12_T6")
    _assert_census(mjx_mod.census(g, 5, 2), want, n, 6)
    res0 = mjx_mod.census(g, 1, 0)
    assert res0["counts"].tolist() == [[0] * n + [1]] and res0["min_plus"].tolist() == [n]
    assert res0["witness"].tolist() == [[1] * n]
    # one enumeration gives the whole dependence on p: the levels of a shorter run are a prefix
    res3 = mjx_mod.census(g, 3, 1)
    assert np.array_equal(res3["counts"], want["counts"][:4]) and np.array_equal(res3["witness"], want["witness"][:4])
    for p, c in ((7, 1), (6, 2), (4, 4)):
        with pytest.raises(ValueError):
            mjx_mod.census(g, p, c)


# ---- 6. one larger case ---------------------------------------------------------------------------
def test_n20_against_the_largest_oracle(mjx_mod):
    _, _, n, T, want = _case("rrg_d3_n20")
    assert want["min_plus"][T] < n
    _assert_census(mjx_mod.census(_graph(mjx_mod, "rrg_d3_n20"), T, 1), want, n, T)
    _assert_census(mjx_mod.census(_graph(mjx_mod, "rrg_d3_n20"), T, 1, chunk_blocks=1000, kernel={"grid": 7}),
                   want, n, T)


# ---- 7. the witness, by the existing rollout ----------------------------------------------------------
@pytest.mark.parametrize("name", ["rrg_d4_n16", "er14"])
def test_the_witness_reaches_consensus_in_t_steps_and_not_sooner(mjx_mod, name):
    _, _, n, T, want = _case(name)
    g = _graph(mjx_mod, name)
    res = mjx_mod.census(g, T, 1)
    assert np.array_equal(res["witness"], want["witness"])
    for t in range(T + 1):
        w = res["witness"][t].astype(np.int64)
        assert (w == 1).sum() == res["min_plus"][t]
        end = w if t == 0 else mjx_mod.s_endstate(g, w, t, 1)
        assert int(np.asarray(end).sum()) == n
        # a strictly lighter witness than the level before needs the extra step
        if t > 1 and res["min_plus"][t] < res["min_plus"][t - 1]:
            assert int(np.asarray(mjx_mod.s_endstate(g, w, t - 1, 1)).sum()) < n


# ---- 8. a bad adjacency through the ABI -------------------------------------------------------------------
def test_an_adjacency_entry_out_of_range_raises_the_flag_in_bounds(mjx_mod):
    _, arrays, n, T, _ = _case("rrg_d3_n12")
    lib = mjx_mod.load_library()
    for bad in (n, -1, 255, 1 << 20):
        adj = torch.from_numpy(arrays[0].astype(np.int32)).cuda()
        adj[5, 1] = bad
        cbuf, kbuf, fbuf, pad = _abi_buffers(T, n, adj.device)
        rc = lib.mjx_census_ell(adj.data_ptr(), n, 3, T, 1, 0, 64, 0, cbuf.data_ptr() + 8 * pad,
                                kbuf.data_ptr() + 8 * pad, fbuf.data_ptr() + 4 * pad, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(fbuf[pad]) == 2, bad
        assert _guards_intact(cbuf, kbuf, fbuf, pad)
        assert not cbuf[pad:-pad].any() and bool((kbuf[pad:-pad] == -1).all()), "a void run writes nothing"
    # CSR: a column out of range (bit 1), a row longer than 47 entries (bit 2)
    rp, col = _csr([list(r) for r in arrays[0].tolist()])
    for rp2, col2, want in ((rp, np.where(np.arange(col.size) == 7, n, col), 2),
                            (np.concatenate([[0], np.full(n, 48)]), np.zeros(48, np.int64), 4)):
        rpt, colt = torch.from_numpy(rp2.astype(np.int64)).cuda(), torch.from_numpy(col2.astype(np.int32)).cuda()
        cbuf, kbuf, fbuf, pad = _abi_buffers(T, n, rpt.device)
        rc = lib.mjx_census_csr(rpt.data_ptr(), colt.data_ptr(), n, T, 1, 0, 64, 0, cbuf.data_ptr() + 8 * pad,
                                kbuf.data_ptr() + 8 * pad, fbuf.data_ptr() + 4 * pad, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(fbuf[pad]) == want and _guards_intact(cbuf, kbuf, fbuf, pad)
        assert not cbuf[pad:-pad].any() and bool((kbuf[pad:-pad] == -1).all())


# ---- 9. CLI ---------------------------------------------------------------------------------------------------
def test_cli_census_in_a_fresh_process(mjx_mod, tmp_path):
    out = tmp_path / "census.npz"
    run = subprocess.run([sys.executable, "-m", "mjx", "census", "--graph", "rrg", "--n", "14", "--d", "3",
                          "--graph-seed", "3", "--p", "2", "--c", "1", "--out", str(out)],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    adj = mjx_mod.random_regular_graph(3, 14, seed=3)
    want = co.census(co.step_ell(adj), 14, 2)
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == ["configs", "counts", "edges", "entropy", "m_min", "min_plus", "witness"]
        assert np.array_equal(z["counts"], want["counts"]) and np.array_equal(z["min_plus"], want["min_plus"])
        assert np.array_equal(z["witness"], want["witness"]) and int(z["configs"]) == 1 << 14
        edges = {(int(u), int(v)) for u, v in z["edges"]}
        assert edges == {(v, int(u)) for v in range(14) for u in adj[v] if v < u} and len(edges) == 21
