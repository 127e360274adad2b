"""Census marginals, CPU side: the invariants of the brute-force oracle
(tests/census_marginals_oracle.py), ``census_boltzmann`` against a direct sum
over the configurations, the premise of the BDCM cross-check on a tree (the
numpy BDCM oracle against the enumeration), the new entry points' ABI and
argument checks, the host-side refusals and the CLI parser.  No GPU."""
import ctypes
import functools
import importlib
import os
import re

import numpy as np
import pytest

import bdcm_cases as bc
import census_marginals_oracle as cmo
import census_oracle as co
from conftest import ROOT
from oracle import bdcm as orc

NEW_SYMBOLS = ("mjx_census_nodes_lds", "mjx_census_nodes_ell", "mjx_census_nodes_csr", "mjx_bdcm_edge_m")
TREE_N, TREE_SEED = 13, 3
TREE_LAMBDAS = (0.0, 0.5, 1.2)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (step, n, T, oracle marginals).  Shared: never written."""
    import mjx
    if name == "rrg":
        n, T = 12, 3
        step = co.step_ell(mjx.random_regular_graph(3, n, seed=1))
    elif name == "er":
        n, T = 11, 2
        rp, col = mjx.erdos_renyi(n, 0.3, seed=3)[:2]
        step = co.step_csr(rp, col)
    else:
        n, T = TREE_N, 3
        _, rp, col = cmo.recursive_tree(TREE_N, TREE_SEED)
        step = co.step_csr(rp, col)
    return step, n, T, cmo.census(step, n, T)


def _as_result(want, levels):
    """The oracle's arrays in the shape of ``census_marginals``'s result for these levels."""
    return {"counts": want["counts"], "levels": list(levels), "node_counts": want["node_counts"][list(levels)]}


@pytest.mark.parametrize("name", ["rrg", "er", "tree"])
def test_oracle_invariants(name):
    step, n, T, res = _case(name)
    counts, nc = res["counts"], res["node_counts"]
    assert nc.shape == (T + 1, n + 1, n) and nc.dtype == np.int64
    # every counted configuration of weight k has k nodes up
    assert np.array_equal(nc.sum(axis=2), counts * np.arange(n + 1)[None, :])
    # level 0 counts all +1 alone
    assert (nc[0, n] == 1).all() and not nc[0, :n].any()
    assert (nc >= 0).all() and (nc <= counts[:, :, None]).all()
    # nested levels, and not degenerate: some node is up in a part of some counted set only
    assert (nc[:-1] <= nc[1:]).all()
    assert ((nc[T] > 0) & (nc[T] < counts[T][:, None])).any()
    # the backbone rule, from the optimal configurations themselves
    S0 = co.configs(0, 1 << n, n)
    S = S0
    for t in range(T + 1):
        if t:
            S = step(S)
        best = S0[(S == 1).all(axis=1) & ((S0 == 1).sum(axis=1) == res["min_plus"][t])]
        assert best.shape[0] == res["optimal"][t] > 0
        assert np.array_equal(res["backbone_plus"][t], (best == 1).all(axis=0))
        assert np.array_equal(res["backbone_minus"][t], (best == -1).all(axis=0))
        assert not (res["backbone_plus"][t] & res["backbone_minus"][t]).any()
    assert res["backbone_plus"][0].all()


@pytest.mark.parametrize("name", ["rrg", "er"])
def test_boltzmann_from_oracle_counts_equals_the_direct_sum(mjx_mod, name):
    step, n, T, want = _case(name)
    assert n <= 12
    res = _as_result(want, range(T + 1))
    for t in range(T + 1):
        for lam in (0.0, 0.5, 3.0):
            got = mjx_mod.census_boltzmann(res, lam, level=t)
            ref = cmo.boltzmann_direct(step, n, t, lam)
            assert abs(got["phi"] - ref["phi"]) <= 1e-13 and abs(got["m_init"] - ref["m_init"]) <= 1e-13
            assert np.abs(got["p_plus"] - ref["p_plus"]).max() <= 1e-13
            assert got["ent1"] == got["phi"] + lam * got["m_init"]
            assert np.array_equal(got["m_node"], 2 * got["p_plus"] - 1)
            # the node marginals average to the magnetisation
            assert abs(got["m_node"].mean() - got["m_init"]) <= 1e-13
    # lambda = 40: the weights span e^(+-480); phi is of the order of lambda, so the bar is relative to it.
    # The optimum dominates: phi -> -lam m_min + ln(optimal) / n, m_init -> m_min, p_plus -> the backbone
    got = mjx_mod.census_boltzmann(res, 40.0, level=T)
    ref = cmo.boltzmann_direct(step, n, T, 40.0)
    assert abs(got["phi"] - ref["phi"]) <= 1e-13 * abs(ref["phi"]) and abs(got["m_init"] - ref["m_init"]) <= 1e-13
    m_min = (2 * want["min_plus"][T] - n) / n
    assert abs(got["phi"] - (-40.0 * m_min + np.log(want["optimal"][T]) / n)) <= 1e-13 * abs(ref["phi"])
    assert abs(got["m_init"] - m_min) <= 1e-13
    assert np.abs(got["p_plus"][want["backbone_plus"][T]] - 1).max() <= 1e-13
    # where the direct sum would overflow, the log-sum-exp does not
    far = mjx_mod.census_boltzmann(res, [-400.0, 400.0], level=T)
    assert all(np.isfinite(v).all() for v in far.values())
    assert far["m_init"][0] == 1.0 and abs(far["m_init"][1] - m_min) <= 1e-13


def test_boltzmann_arguments(mjx_mod):
    _, n, T, want = _case("rrg")
    res = _as_result(want, [1, T])
    one = mjx_mod.census_boltzmann(res, 0.5)
    assert one["phi"].shape == () and one["p_plus"].shape == (n,)
    many = mjx_mod.census_boltzmann(res, [0.0, 0.5, 3.0])
    assert many["phi"].shape == (3,) and many["ent1"].shape == (3,) and many["m_node"].shape == (3, n)
    assert many["phi"][1] == one["phi"] and np.array_equal(many["p_plus"][1], one["p_plus"])
    assert all(v.dtype == np.float64 for v in many.values())
    # the default level is the last one requested; ``level`` indexes ``levels``
    assert mjx_mod.census_boltzmann(res, 0.5, level=1)["phi"] == one["phi"]
    assert mjx_mod.census_boltzmann(res, 0.5, level=0)["phi"] < one["phi"]
    # lambda = 0 counts: phi = ln(number of counted configurations) / n
    assert abs(mjx_mod.census_boltzmann(res, 0.0)["phi"] - np.log(want["counts"][T].sum()) / n) <= 1e-15
    with pytest.raises(ValueError, match="attr_value = -1.*all \\+1 only"):
        mjx_mod.census_boltzmann(res, 0.5, attr_value=-1)
    with pytest.raises(ValueError, match="level index 2"):
        mjx_mod.census_boltzmann(res, 0.5, level=2)


def test_an_isolated_node_starts_plus_as_in_bdcm(mjx_mod):
    """BDCM's isolated-node terms (-attr_value lmbd n_iso in phi, attr_value n_iso in m_init) are what the
    enumeration gives: a node of degree 0 is +1 in every counted configuration."""
    step = co.step_csr(np.array([0, 1, 2, 2]), np.array([1, 0]))        # an edge and a node alone
    want = cmo.census(step, 3, 1)
    assert want["backbone_plus"][1][2] and (want["node_counts"][1][:, 2] == want["counts"][1]).all()
    got = mjx_mod.census_boltzmann(_as_result(want, [1]), 0.7)
    assert got["p_plus"][2] == 1.0
    pair = cmo.census(co.step_ell(np.array([[1], [0]])), 2, 1)
    alone = mjx_mod.census_boltzmann(_as_result(pair, [1]), 0.7)
    assert abs(3 * got["phi"] - (2 * alone["phi"] - 0.7)) <= 1e-14
    assert abs(3 * got["m_init"] - (2 * alone["m_init"] + 1)) <= 1e-14


@pytest.mark.parametrize("p,c", [(1, 1), (2, 1), (3, 1), (1, 2)])
def test_bdcm_on_a_tree_equals_the_enumeration_at_level_p(mjx_mod, p, c):
    """The premise of the device cross-check, on the CPU: the numpy BDCM oracle at its fixed point on the
    13-node random recursive tree against ``census_boltzmann`` of the brute-force counts at level t = p (for
    c = 2, x(p+1) all +1 and x(p+2) = x(p) force x(p) all +1, so the level is p and not p + c - 1).
    Largest distance measured over the four (p, c) and three lambdas: 1.2e-15 in phi, 1.2e-14 in m_init (both at (3, 1))."""
    edges, rp, col = cmo.recursive_tree(TREE_N, TREE_SEED)
    assert np.diff(rp).max() >= 4, "a tree with hubs, not a path"
    _, n, T, want = _case("tree")
    plan = orc.Plan.from_csr(edges, rp, col, n, 0)
    chi0 = bc.random_chi(2 * plan.E, p + c, 100 * p + c)
    m_init, _, phi, counts, iters, _ = orc.entropy_procedure(chi0, plan, p, c, 1, list(TREE_LAMBDAS), 0.5, eps=1e-14,
                                                             T_max=2000, stop_ent=-1e300)
    assert counts == 0 and (iters < 2000).all(), "converged at every lambda"
    exact = mjx_mod.census_boltzmann(_as_result(want, [p]), list(TREE_LAMBDAS))
    d_phi, d_m = np.abs(phi - exact["phi"]).max(), np.abs(m_init - exact["m_init"]).max()
    print(f"(p, c) = ({p}, {c}): max |d phi| = {d_phi:.3g}, max |d m_init| = {d_m:.3g}")
    assert d_phi <= 1e-12 and d_m <= 1e-12
    if c == 2:                                               # and level p + c - 1 is another set
        other = mjx_mod.census_boltzmann(_as_result(want, [p + c - 1]), list(TREE_LAMBDAS))
        assert np.abs(phi - other["phi"]).min() > 1e-3


def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "Node counts:" in src and "Backbone:" in src, "the definitions belong to the contract"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(mjx_mod.lib_path())
    sig = mjx_mod._lib.SIGNATURES
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, f"{name} not declared in include/mjx.h"
        assert name in sig, f"{name} has no ctypes signature"
        assert len(sig[name]) == len(decl.group(1).split(",")), name
        assert hasattr(raw, name)
    assert len(sig["mjx_census_nodes_ell"]) == len(sig["mjx_census_ell"]) + 2       # t_node and node_counts
    assert len(sig["mjx_census_nodes_csr"]) == len(sig["mjx_census_csr"]) + 2
    assert len(sig["mjx_bdcm_edge_m"]) == 8
    assert mjx_mod._lib._RESTYPES["mjx_census_nodes_lds"] is ctypes.c_int64
    for name in ("census_marginals", "census_boltzmann", "bdcm_node_m_init"):
        assert name in mjx_mod.__all__ and callable(getattr(mjx_mod, name))
    mod = importlib.import_module("mjx.census")
    assert mjx_mod.census_marginals is mod.census_marginals and mjx_mod.census_boltzmann is mod.census_boltzmann


def test_lds_formula_and_argument_checks_without_gpu(mjx_mod):
    lib = mjx_mod.load_library()
    mod = importlib.import_module("mjx.census")
    EINVAL, ERANGE = 1, 3
    for n in range(1, 49):
        assert lib.mjx_census_nodes_lds(n) == lib.mjx_census_lds(n) + 4 * (n + 1) * n == mod.census_nodes_lds(n)
    assert lib.mjx_census_nodes_lds(48) == 64104 <= 64 * 1024
    for n in (0, -1, 49, 1 << 40):
        assert lib.mjx_census_nodes_lds(n) == -1
    # compute entry points: validation fails before any pointer is read
    a = ctypes.c_void_p(64)
    #     adj n  d  p  c  t  lo hi   grid counts keys node flag stream
    ok = (a, 16, 3, 3, 1, 3, 0, 1024, 0, a, a, a, a, None)
    ell = lib.mjx_census_nodes_ell
    assert ell(*(ok[:1] + (49,) + ok[2:])) == ERANGE                         # n > 48
    assert ell(*(ok[:3] + (7, 1, 3) + ok[6:])) == ERANGE                     # T = 7
    assert ell(*(ok[:2] + (48,) + ok[3:])) == ERANGE                         # d > 47
    assert ell(*(ok[:1] + (0,) + ok[2:])) == EINVAL                          # n < 1
    assert ell(*(ok[:3] + (0, 0, 0) + ok[6:])) == EINVAL                     # T = -1
    assert ell(*(ok[:5] + (4,) + ok[6:])) == EINVAL                          # t_node > T
    assert ell(*(ok[:5] + (-1,) + ok[6:])) == EINVAL                         # t_node < 0
    assert ell(*(ok[:7] + (1025,) + ok[8:])) == EINVAL                       # block_hi > B
    assert ell(*(ok[:6] + (5, 4) + ok[8:])) == EINVAL                        # lo > hi
    assert ell(*(ok[:8] + (-1,) + ok[9:])) == EINVAL                         # grid < 0
    for k in (9, 10, 11, 12):
        assert ell(*(ok[:k] + (None,) + ok[k + 1:])) == EINVAL               # counts, keys, node counts, flag
    assert ell(*((None,) + ok[1:])) == EINVAL                                # d > 0 without adj
    assert ell(*(ok[:6] + (7, 7) + ok[8:])) == 0                             # an empty range: nothing to do
    big = (a, 40, 3, 3, 1, 3, 0, (1 << 25) + 1, 0, a, a, a, a, None)
    assert ell(*big) == ERANGE                                               # more than 2^25 blocks in a launch
    okc = (a, a, 16, 3, 1, 3, 0, 1024, 0, a, a, a, a, None)
    csr = lib.mjx_census_nodes_csr
    assert csr(*((None,) + okc[1:])) == EINVAL
    assert csr(*(okc[:2] + (49,) + okc[3:])) == ERANGE
    assert csr(*(okc[:3] + (4, 4, 0) + okc[6:])) == ERANGE
    assert csr(*(okc[:5] + (4,) + okc[6:])) == EINVAL
    assert csr(*(okc[:7] + (1025,) + okc[8:])) == EINVAL
    m = lib.mjx_bdcm_edge_m
    assert m(a, -1, 1, 1, 1, 0.0, a, None) == EINVAL                         # E < 0
    assert m(a, 4, 1, 0, 1, 0.0, a, None) == EINVAL                          # c < 1
    assert m(a, 4, 1, 1, 0, 0.0, a, None) == EINVAL                          # attr_value
    assert m(None, 4, 1, 1, 1, 0.0, a, None) == EINVAL and m(a, 4, 1, 1, 1, 0.0, None, None) == EINVAL
    assert m(None, 0, 1, 1, 1, 0.0, None, None) == 0                         # no edges: nothing to do


def test_census_marginals_refuses_on_the_host(mjx_mod):
    """Every refusal comes before any device call: the same ValueError with and without a GPU."""
    adj = mjx_mod.random_regular_graph(3, 20, seed=0)
    for levels in ([4], [-1], [0, 7], [1.5], []):
        with pytest.raises(ValueError, match="level"):
            mjx_mod.census_marginals(adj, 3, 1, levels=levels)
    with pytest.raises(ValueError, match="level 2 is outside 0..T = p \\+ c - 1 = 1"):
        mjx_mod.census_marginals(adj, 1, 1, levels=[0, 2])
    with pytest.raises(ValueError, match="n = 50.*n <= 48"):
        mjx_mod.census_marginals(mjx_mod.random_regular_graph(3, 50, seed=0), 1, 1)
    for p, c in ((7, 1), (4, 4), (0, 0)):
        with pytest.raises(ValueError, match="p \\+ c - 1"):
            mjx_mod.census_marginals(adj, p, c)
    with pytest.raises(ValueError, match="2\\^20 = 1048576 configurations exceed max_configs = 1000"):
        mjx_mod.census_marginals(adj, 1, 1, max_configs=1000)
    with pytest.raises(ValueError, match="unknown kernel options"):
        mjx_mod.census_marginals(adj, 1, 1, kernel={"lds_entries": 4})
    with pytest.raises(ValueError, match="chunk_blocks"):
        mjx_mod.census_marginals(adj, 1, 1, chunk_blocks=0)
    asym = adj.copy()
    u = int(asym[0, 0])
    asym[0, 0] = next(v for v in range(1, 20) if v != u and v not in asym[0])
    with pytest.raises(ValueError, match="not symmetric"):
        mjx_mod.census_marginals(asym, 1, 1)


def test_cli_parser_accepts_marginals():
    cli = importlib.import_module("mjx.cli")
    a = cli.build_parser().parse_args(["census", "--graph", "rrg", "--n", "16", "--p", "3", "--c", "1", "--marginals",
                                       "--levels", "0", "3", "--lam", "0", "0.5", "--out", "x.npz"])
    assert (a.cmd, a.marginals, a.levels, a.lam, a.minima) == ("census", True, [0, 3], [0.0, 0.5], False)
    a = cli.build_parser().parse_args(["census", "--p", "1", "--c", "1"])
    assert (a.marginals, a.levels, a.lam) == (False, None, None)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["census", "--p", "1", "--c", "1", "--levels", "x"])
    for extra in (["--levels", "1"], ["--lam", "0.5"], ["--marginals", "--minima"]):
        with pytest.raises(SystemExit, match="--marginals"):
            cli.run_census(cli.build_parser().parse_args(["census", "--p", "1", "--c", "1"] + extra))
