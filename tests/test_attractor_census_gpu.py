"""``attractor_census`` on the GPU against the brute-force oracle
(tests/attractor_census_oracle.py) and, at sizes the oracle does not reach,
against ``census`` and ``attractor``.  Integer exact: every comparison is
array_equal."""
import functools
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import attractor_census_oracle as aco
from conftest import ROOT

pytestmark = pytest.mark.gpu

T_MAX = 16
PLUS, MINUS, FIXED, CYCLE = range(4)


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([u for r in rows for u in r], dtype=np.int32)
    return rp, col


def _path(n):
    return _csr([[u for u in (v - 1, v + 1) if 0 <= u < n] for v in range(n)])


def _ring(n):
    return np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1)


def _spec(name):
    """-> (kind, arrays, n)"""
    import mjx
    if name.startswith("rrg"):                               # rrg_d{d}_n{n}
        d, n = int(name[5]), int(name[8:])
        return "ell", (mjx.random_regular_graph(d, n, seed=1),), n
    if name == "er15":
        rp, col = mjx.erdos_renyi(15, 3.0 / 14, seed=5)[:2]
        assert (np.diff(rp) == 0).any(), "the case needs a node of degree 0"
        return "csr", (rp, col), 15
    if name.startswith("path"):
        return "csr", _path(int(name[4:])), int(name[4:])
    if name.startswith("ring"):
        return "ell", (_ring(int(name[4:])),), int(name[4:])
    if name == "star9":
        return "csr", _csr([list(range(1, 9))] + [[0]] * 8), 9
    if name == "lone":
        return "csr", _csr([[]]), 1
    if name == "edge":
        return "ell", (np.array([[1], [0]]),), 2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name, t_max=T_MAX):
    """-> (kind, arrays, n, oracle result).  Shared: never written."""
    kind, arrays, n = _spec(name)
    step = aco.step_ell(arrays[0]) if kind == "ell" else aco.step_csr(*arrays)
    return kind, arrays, n, aco.attractor_census(step, n, t_max)


def _graph(mjx_mod, name, kind=None):
    k, arrays, _ = _spec(name)
    if (kind or k) == "ell":
        return mjx_mod.Graph.ell(arrays[0])
    if k == "csr":
        return mjx_mod.Graph.csr(*arrays)
    return mjx_mod.Graph.csr(*_csr([list(r) for r in arrays[0].tolist()]))       # an ELL case as CSR


def _assert_equal(res, want, n, t_max):
    d = aco.derived(want, n)
    assert res["hist"].dtype == np.int64 and res["hist"].shape == (4, t_max + 1, n + 1)
    assert np.array_equal(res["hist"], want["hist"])
    assert res["unsettled"].dtype == np.int64 and np.array_equal(res["unsettled"], want["unsettled"])
    assert res["configs"] == 1 << n and tuple(res["classes"]) == ("plus", "minus", "fixed", "cycle")
    assert res["reach_plus"].dtype == np.int64 and np.array_equal(res["reach_plus"], d["reach_plus"])
    binom = np.array([math.comb(n, k) for k in range(n + 1)], dtype=np.float64)
    assert res["p_plus"].dtype == np.float64 and np.array_equal(res["p_plus"], want["hist"][0].sum(axis=0) / binom)
    assert res["min_plus_ever"] == d["min_plus_ever"] and res["m_min_ever"] == (2 * d["min_plus_ever"] - n) / n
    assert res["witness_plus"].dtype == np.int8 and np.array_equal(res["witness_plus"], d["witness_plus"])
    assert res["p_longest"] == d["p_longest"]
    assert res["witness_longest"].dtype == np.int8 and np.array_equal(res["witness_longest"], d["witness_longest"])
    assert 2 <= res["mean_sweeps"] <= t_max + 2


# ---- 1. against the oracle, full enumeration -----------------------------------------------------
FULL = ["rrg_d3_n16", "rrg_d4_n16", "rrg_d5_n12", "er15", "path16", "star9", "lone", "edge", "path5", "ring5", "ring6",
        "path7"]


@pytest.mark.parametrize("name", FULL)
def test_full_enumeration_equals_the_oracle(mjx_mod, name):
    _, _, n, want = _case(name)
    assert not want["unsettled"].any(), "t_max covers every transient of the case"
    _assert_equal(mjx_mod.attractor_census(_graph(mjx_mod, name), T_MAX), want, n, T_MAX)


def test_the_cases_are_not_degenerate():
    full = [_case(name)[3] for name in FULL]
    assert sum(bool((w["hist"].sum(axis=(1, 2)) > 0).all()) for w in full) >= 2, "all four classes on two cases"
    assert max(w["longest"] >> 48 for w in full) >= 8
    assert _case("rrg_d5_n12")[3]["hist"][:, 1:].any() and _case("er15")[3]["hist"][FIXED].any()


def test_the_same_graph_as_ell_csr_and_array(mjx_mod):
    _, arrays, n, want = _case("rrg_d3_n16")
    _assert_equal(mjx_mod.attractor_census(arrays[0], T_MAX), want, n, T_MAX)                 # the (n, d) array
    _assert_equal(mjx_mod.attractor_census(_graph(mjx_mod, "rrg_d3_n16", "csr"), T_MAX), want, n, T_MAX)
    _, arrays, n, want = _case("rrg_d4_n16")
    _assert_equal(mjx_mod.attractor_census(_graph(mjx_mod, "rrg_d4_n16", "csr"), T_MAX), want, n, T_MAX)


# ---- 2. truncation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("t_max", [0, 1, 4])
def test_truncation(mjx_mod, t_max):
    name = "path16"
    _, _, n, full = _case(name)
    assert full["longest"] >> 48 >= 8
    _, _, _, want = _case(name, t_max)
    assert want["unsettled"].any() and want["longest"] >> 48 <= t_max
    assert np.array_equal(want["hist"], full["hist"][:, :t_max + 1])
    res = mjx_mod.attractor_census(_graph(mjx_mod, name), t_max)
    _assert_equal(res, want, n, t_max)
    if t_max == 0:
        assert res["mean_sweeps"] == 2                       # sweeps 1 and 2 decide p = 0


# ---- 3. independence of the split and the grid -------------------------------------------------------
@pytest.mark.parametrize("how", [{"chunk_blocks": 1}, {"chunk_blocks": 3}, {"chunk_blocks": 64}, {"kernel": {"grid": 1}},
                                 {"kernel": {"grid": 7}}, {"chunk_blocks": 100, "kernel": {"grid": 3}}])
def test_the_result_does_not_depend_on_the_split_or_the_grid(mjx_mod, how):
    _, _, n, want = _case("rrg_d3_n14")
    _assert_equal(mjx_mod.attractor_census(_graph(mjx_mod, "rrg_d3_n14"), T_MAX, **how), want, n, T_MAX)


# ---- 4. against the package itself at n = 24 ---------------------------------------------------------
def test_n24_against_census_and_attractor(mjx_mod):
    n, t_max = 24, 32
    g = mjx_mod.Graph.ell(mjx_mod.random_regular_graph(4, n, seed=1))
    res = mjx_mod.attractor_census(g, t_max)
    hist, uns = res["hist"], res["unsettled"]
    for t in range(1, 7):
        assert np.array_equal(res["reach_plus"][t], mjx_mod.census(g, t, 1)["counts"][t]), t
    assert res["min_plus_ever"] <= mjx_mod.census(g, 6, 1)["min_plus"][6]
    binom = np.array([math.comb(n, k) for k in range(n + 1)])
    assert np.array_equal(hist.sum(axis=(0, 1)) + uns, binom)
    assert np.array_equal(hist[PLUS], hist[MINUS][:, ::-1])
    assert np.array_equal(hist[FIXED], hist[FIXED][:, ::-1]) and np.array_equal(hist[CYCLE], hist[CYCLE][:, ::-1])
    assert np.array_equal(uns, uns[::-1])
    w = res["witness_plus"].astype(np.int64)
    assert (w == 1).sum() == res["min_plus_ever"]
    a = mjx_mod.attractor(g, w, t_max)
    assert int(a["c"][0]) == 1 and a["sum_att"][0].tolist() == [n, n]
    a = mjx_mod.attractor(g, res["witness_longest"].astype(np.int64), t_max)
    assert int(a["p"][0]) == res["p_longest"] and res["p_longest"] == np.flatnonzero(hist.sum(axis=(0, 2))).max()


# ---- 5. the raw ABI on a block sub-range ----------------------------------------------------------------
GUARD = 0x5A5A5A5A5A5A


def _abi_buffers(t_max, n, dev, pad=8):
    """hist, unsettled, keys and flag in the middle of guarded allocations -> (buffers, pointers, pad)."""
    sizes = (4 * (t_max + 1) * (n + 1), n + 1, 2)
    bufs = [torch.full((s + 2 * pad,), GUARD, dtype=torch.int64, device=dev) for s in sizes]
    bufs.append(torch.full((1 + 2 * pad,), 0x5A5A, dtype=torch.int32, device=dev))
    for b in bufs:
        b[pad:-pad] = 0
    bufs[2][pad] = -1                                        # lightest plus: all ones; longest: 0
    ptrs = [b.data_ptr() + b.element_size() * pad for b in bufs]
    return bufs, ptrs, pad


def _guards_intact(bufs, pad):
    return all(bool((b[:pad] == v).all()) and bool((b[-pad:] == v).all())
               for b, v in zip(bufs, (GUARD, GUARD, GUARD, 0x5A5A)))


def _untouched(bufs, pad):
    return (not bufs[0][pad:-pad].any() and not bufs[1][pad:-pad].any()
            and bufs[2][pad:-pad].tolist() == [-1, 0])


@pytest.mark.parametrize("b0,t_max", [(5, 24), ((0x2A5 << 24) | 0x81234, 24), ((0x2A5 << 24) | 0x81234, 3),
                                      ((1 << 34) - 64, 3)])
def test_raw_abi_on_a_block_sub_range(mjx_mod, b0, t_max):
    n, d = 40, 3
    adj = mjx_mod.random_regular_graph(d, n, seed=4)
    g = mjx_mod.Graph.ell(adj)
    lib = mjx_mod.load_library()
    # the 4096 configurations of the blocks on the host, through ``attractor``
    x = np.arange(64 * b0, 64 * (b0 + 64), dtype=np.int64)
    S = 2 * ((x[:, None] >> np.arange(n)[None, :]) & 1) - 1
    a = mjx_mod.attractor(g, S, t_max)
    p, c, s0 = a["p"], a["c"], a["sum_att"][:, 0]
    k = (S == 1).sum(axis=1)
    done = p >= 0
    cls = np.where(c == 2, CYCLE, np.where(s0 == n, PLUS, np.where(s0 == -n, MINUS, FIXED)))
    hist = np.zeros((4, t_max + 1, n + 1), np.int64)
    np.add.at(hist, (cls[done], p[done], k[done]), 1)
    uns = np.bincount(k[~done], minlength=n + 1)
    plus = done & (cls == PLUS)
    keys = [int(((k[plus] << 48) | x[plus]).min()) if plus.any() else -1,
            int(((p[done] << 48) | x[done]).max()) if done.any() else 0]
    assert hist.sum() + uns.sum() == 4096 and done.any()
    if t_max < 8:
        assert uns.any(), "the truncated range leaves configurations unsettled"
    bufs, ptrs, pad = _abi_buffers(t_max, n, g.adj.device)
    assert lib.mjx_attractor_census_ell(g.adj.data_ptr(), n, d, t_max, b0, b0 + 64, 0, *ptrs, None, None) == 0
    torch.cuda.synchronize()
    assert int(bufs[3][pad]) == 0 and _guards_intact(bufs, pad)
    assert np.array_equal(bufs[0][pad:-pad].cpu().numpy().reshape(4, t_max + 1, n + 1), hist)
    assert np.array_equal(bufs[1][pad:-pad].cpu().numpy(), uns)
    assert bufs[2][pad:-pad].tolist() == keys
    # the same range in two launches with a forced grid, and the sweep statistics
    bufs, ptrs, pad = _abi_buffers(t_max, n, g.adj.device)
    stats = torch.zeros(2, dtype=torch.int64, device=g.adj.device)
    for lo, hi in ((b0, b0 + 23), (b0 + 23, b0 + 64)):
        assert lib.mjx_attractor_census_ell(g.adj.data_ptr(), n, d, t_max, lo, hi, 2, *ptrs, stats.data_ptr(),
                                            None) == 0
    torch.cuda.synchronize()
    assert int(bufs[3][pad]) == 0 and _guards_intact(bufs, pad)
    assert np.array_equal(bufs[0][pad:-pad].cpu().numpy().reshape(4, t_max + 1, n + 1), hist)
    assert np.array_equal(bufs[1][pad:-pad].cpu().numpy(), uns) and bufs[2][pad:-pad].tolist() == keys
    rows, sweeps = stats.tolist()
    assert rows == 2 and 2 * 2 <= sweeps <= 2 * (t_max + 2)


# ---- 6. flags and refusals through the ABI ------------------------------------------------------------------
def test_a_bad_adjacency_raises_the_flag_and_writes_nothing(mjx_mod):
    _, arrays, n, _ = _case("rrg_d3_n14")
    lib = mjx_mod.load_library()
    for bad in (n, -1):
        adj = torch.from_numpy(arrays[0].astype(np.int32)).cuda()
        adj[5, 1] = bad
        bufs, ptrs, pad = _abi_buffers(T_MAX, n, adj.device)
        assert lib.mjx_attractor_census_ell(adj.data_ptr(), n, 3, T_MAX, 0, 64, 0, *ptrs, None, None) == 0
        torch.cuda.synchronize()
        assert int(bufs[3][pad]) == 2, bad
        assert _guards_intact(bufs, pad) and _untouched(bufs, pad), "a void run writes nothing"
    rp, col = _csr([list(r) for r in arrays[0].tolist()])
    down = rp.copy()
    down[4] = down[3] - 1                                    # a decreasing row_ptr
    for rp2, col2, want in ((rp, np.where(np.arange(col.size) == 7, n, col), 2), (down, col, 4)):
        rpt, colt = torch.from_numpy(rp2.astype(np.int64)).cuda(), torch.from_numpy(col2.astype(np.int32)).cuda()
        bufs, ptrs, pad = _abi_buffers(T_MAX, n, rpt.device)
        assert lib.mjx_attractor_census_csr(rpt.data_ptr(), colt.data_ptr(), n, T_MAX, 0, 64, 0, *ptrs, None,
                                            None) == 0
        torch.cuda.synchronize()
        assert int(bufs[3][pad]) == want and _guards_intact(bufs, pad) and _untouched(bufs, pad)


def test_a_shape_past_the_lds_ceiling_is_refused(mjx_mod):
    n, d = 40, 3
    g = mjx_mod.Graph.ell(mjx_mod.random_regular_graph(d, n, seed=4))
    lib = mjx_mod.load_library()
    assert lib.mjx_attractor_census_lds(n, 33) == -1
    bufs, ptrs, pad = _abi_buffers(33, n, g.adj.device)
    assert lib.mjx_attractor_census_ell(g.adj.data_ptr(), n, d, 33, 0, 64, 0, *ptrs, None, None) == 1   # MJX_EINVAL
    torch.cuda.synchronize()
    assert int(bufs[3][pad]) == 0 and _guards_intact(bufs, pad) and _untouched(bufs, pad)
    with pytest.raises(ValueError, match="n = 40, t_max = 33 need 65736 bytes"):
        mjx_mod.attractor_census(g, 33, max_configs=2 ** 40)


# ---- 7. the CLI ------------------------------------------------------------------------------------------------
def test_cli_attractor_census_in_a_fresh_process(mjx_mod, tmp_path):
    out = tmp_path / "ac.npz"
    run = subprocess.run([sys.executable, "-m", "mjx", "attractor-census", "--graph", "rrg", "--n", "14", "--d", "3",
                          "--graph-seed", "1", "--t-max", str(T_MAX), "--out", str(out)],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    adj = mjx_mod.random_regular_graph(3, 14, seed=1)
    res = mjx_mod.attractor_census(adj, T_MAX)
    _assert_equal(res, _case("rrg_d3_n14")[3], 14, T_MAX)
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(list(res) + ["edges"])
        for key, val in res.items():
            assert np.array_equal(z[key], np.asarray(val)), key
        edges = {(int(u), int(v)) for u, v in z["edges"]}
        assert edges == {(v, int(u)) for v in range(14) for u in adj[v] if v < u} and len(edges) == 21
