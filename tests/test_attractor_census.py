"""Attractor census, CPU side: hand cases and invariants of the brute-force
oracle (tests/attractor_census_oracle.py), the new entry points' ABI and
argument checks, the host-side refusals of ``attractor_census`` and the CLI
parser.  No GPU."""
import ctypes
import functools
import importlib
import math
import os
import re

import numpy as np
import pytest

import attractor_census_oracle as aco
import census_oracle as co
from conftest import ROOT

NEW_SYMBOLS = ("mjx_attractor_census_lds", "mjx_attractor_census_ell", "mjx_attractor_census_csr")
PLUS, MINUS, FIXED, CYCLE = range(4)


def _cells(hist):
    """{(class, p, k): count} of the non-zero cells."""
    return {tuple(int(i) for i in idx): int(hist[tuple(idx)]) for idx in np.argwhere(hist)}


# ---- hand cases ---------------------------------------------------------------------------------
def test_one_edge():
    res = aco.attractor_census(aco.step_ell(np.array([[1], [0]])), 2, 4)
    # ++ and -- stay; +- and -+ swap for ever: a 2-cycle entered at once
    assert _cells(res["hist"]) == {(PLUS, 0, 2): 1, (MINUS, 0, 0): 1, (CYCLE, 0, 1): 2}
    assert not res["unsettled"].any()
    assert res["lightest_plus"] == (2 << 48) | 3 and res["longest"] == 3


def test_the_edgeless_graph():
    n = 5
    res = aco.attractor_census(aco.step_csr(np.zeros(n + 1, np.int64), np.zeros(0, np.int64)), n, 3)
    want = {(PLUS, 0, n): 1, (MINUS, 0, 0): 1}
    want.update({(FIXED, 0, k): math.comb(n, k) for k in range(1, n)})
    assert _cells(res["hist"]) == want and not res["unsettled"].any()
    assert res["lightest_plus"] == (n << 48) | 31 and res["longest"] == 31


def test_a_triangle():
    tri = np.array([[1, 2], [0, 2], [0, 1]])
    res = aco.attractor_census(aco.step_ell(tri), 3, 4)
    # even degree 2, ties keep the spin.  One +1: its neighbours see a tie and stay -1, it sees two -1 and
    # flips: all -1 after one step.  Two +1: the mirror image.
    assert _cells(res["hist"]) == {(PLUS, 0, 3): 1, (MINUS, 0, 0): 1, (MINUS, 1, 1): 3, (PLUS, 1, 2): 3}
    assert res["lightest_plus"] == (2 << 48) | 3 and res["longest"] == (1 << 48) | 6
    d = aco.derived(res, 3)
    assert d["min_plus_ever"] == 2 and d["witness_plus"].tolist() == [1, 1, -1]
    assert d["p_longest"] == 1 and d["witness_longest"].tolist() == [-1, 1, 1]
    # truncated at t_max = 0 the six mixed configurations are unsettled, and the longest is all +1
    cut = aco.attractor_census(aco.step_ell(tri), 3, 0)
    assert _cells(cut["hist"]) == {(PLUS, 0, 3): 1, (MINUS, 0, 0): 1} and cut["unsettled"].tolist() == [0, 3, 3, 0]
    assert cut["longest"] == 7


# ---- invariants on one ELL and one CSR graph ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (step, n, t_max, oracle result).  Shared: never written."""
    import mjx
    if name == "rrg":
        n = 12
        step = co.step_ell(mjx.random_regular_graph(3, n, seed=1))
    else:
        n = 13
        step = co.step_csr(*mjx.erdos_renyi(n, 0.3, seed=3))
    return step, n, 16, aco.attractor_census(step, n, 16)


@pytest.mark.parametrize("name", ["rrg", "er"])
def test_oracle_invariants(name):
    step, n, t_max, res = _case(name)
    hist, uns = res["hist"], res["unsettled"]
    binom = np.array([math.comb(n, k) for k in range(n + 1)])
    assert np.array_equal(hist.sum(axis=(0, 1)) + uns, binom)
    assert not uns.any() and hist[:, 1:].any(), "the case settles within t_max and has transients"
    # the rule is odd: flipping every spin maps trajectories onto trajectories
    assert np.array_equal(hist[PLUS], hist[MINUS][:, ::-1])
    assert np.array_equal(hist[FIXED], hist[FIXED][:, ::-1]) and np.array_equal(hist[CYCLE], hist[CYCLE][:, ::-1])
    assert np.array_equal(uns, uns[::-1])
    # all +1 after t steps <=> class plus with p <= t (all +1 is a fixed point)
    reach = aco.derived(res, n)["reach_plus"]
    assert np.array_equal(reach[:7], co.census(step, n, 6)["counts"])
    # truncation moves the long transients to unsettled and nothing else
    cut = aco.attractor_census(step, n, 1)
    assert np.array_equal(cut["hist"], hist[:, :2]) and np.array_equal(cut["unsettled"], hist[:, 2:].sum(axis=(0, 1)))
    assert cut["longest"] >> 48 <= 1 < res["longest"] >> 48


# ---- the package side --------------------------------------------------------------------------------
def test_package_exports_attractor_census(mjx_mod):
    mod = importlib.import_module("mjx.census")
    assert mjx_mod.attractor_census is mod.attractor_census and "attractor_census" in mjx_mod.__all__
    assert mod.CLASSES == aco.CLASSES == ("plus", "minus", "fixed", "cycle")


def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "hist[class][p][k]" in src and "lightest_plus" in src, "the definitions belong to the contract"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    raw = ctypes.CDLL(mjx_mod.lib_path())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(raw, name)
    sig = mjx_mod._lib.SIGNATURES
    assert len(sig["mjx_attractor_census_ell"]) == 13 and len(sig["mjx_attractor_census_csr"]) == 13
    assert len(sig["mjx_attractor_census_lds"]) == 2
    assert mjx_mod._lib._RESTYPES["mjx_attractor_census_lds"] is ctypes.c_int64


def test_lds_formula_ceiling_and_argument_checks_without_gpu(mjx_mod):
    lib = mjx_mod.load_library()
    cs = importlib.import_module("mjx.census")
    EINVAL, ERANGE = 1, 3
    for n in range(1, 49):
        for t_max in (0, 1, 6, 13, 16, 17, 32, 33, 100, 1024):
            # two levels, hist[4][t_max+1][n+1] and unsettled[n+1] of 32-bit cells, two keys, patterns, offsets, bytes
            want = (1024 * n + 16 * (t_max + 1) * (n + 1) + 8 * (-(-(n + 1) // 2)) + 16 + 8 * n
                    + 8 * (-(-(n + 1) // 4)) + 8 * (-(-(47 * n) // 8)))
            assert cs.attractor_census_lds(n, t_max) == want
            assert lib.mjx_attractor_census_lds(n, t_max) == (want if want <= 64 * 1024 else -1), (n, t_max)
    assert lib.mjx_attractor_census_lds(32, 32) == 52176
    assert 0 < lib.mjx_attractor_census_lds(40, 32) <= 64 * 1024 and lib.mjx_attractor_census_lds(40, 33) == -1
    for n, t_max in ((0, 4), (-1, 4), (49, 4), (1 << 40, 4), (8, -1), (2, 1025)):
        assert lib.mjx_attractor_census_lds(n, t_max) == -1
    # compute entry points: validation fails before any pointer is read
    a = ctypes.c_void_p(64)
    ok = (a, 16, 3, 8, 0, 1024, 0, a, a, a, a, None, None)
    ell = lib.mjx_attractor_census_ell
    assert ell(*(ok[:1] + (49,) + ok[2:])) == ERANGE                                   # n > 48
    assert ell(*(ok[:3] + (1025,) + ok[4:])) == ERANGE                                 # t_max past the cap
    assert ell(*(ok[:2] + (48,) + ok[3:])) == ERANGE                                   # d > 47
    assert ell(*(ok[:1] + (32, 3, 8, 0, (1 << 25) + 1) + ok[6:])) == ERANGE            # more than 2^25 blocks a launch
    assert ell(*(ok[:1] + (0,) + ok[2:])) == EINVAL                                    # n < 1
    assert ell(*(ok[:3] + (-1,) + ok[4:])) == EINVAL                                   # t_max < 0
    assert ell(*(ok[:1] + (40, 3, 33, 0, 64) + ok[6:])) == EINVAL                      # 65,736 bytes of LDS
    assert ell(*(ok[:1] + (48, 3, 32, 0, 64) + ok[6:])) == EINVAL
    assert ell(*(ok[:5] + (1025,) + ok[6:])) == EINVAL                                 # block_hi > B
    assert ell(*(ok[:4] + (5, 4) + ok[6:])) == EINVAL                                  # lo > hi
    assert ell(*(ok[:4] + (-1, 4) + ok[6:])) == EINVAL
    assert ell(*(ok[:6] + (-1,) + ok[7:])) == EINVAL                                   # grid < 0
    for k in (7, 8, 9, 10):
        assert ell(*(ok[:k] + (None,) + ok[k + 1:])) == EINVAL                         # hist, unsettled, keys, flag
    assert ell(*((None,) + ok[1:])) == EINVAL                                          # d > 0 without adj
    assert ell(*(ok[:4] + (7, 7) + ok[6:])) == 0                                       # an empty range: nothing to do
    okc = (a, a, 16, 8, 0, 1024, 0, a, a, a, a, None, None)
    csr = lib.mjx_attractor_census_csr
    assert csr(*((None,) + okc[1:])) == EINVAL
    assert csr(*(okc[:2] + (49,) + okc[3:])) == ERANGE
    assert csr(*(okc[:3] + (1025,) + okc[4:])) == ERANGE
    assert csr(*(okc[:5] + (1025,) + okc[6:])) == EINVAL
    assert csr(*(okc[:2] + (5,) + okc[3:5] + (2,) + okc[6:])) == EINVAL                # n < 6: one block
    assert csr(*(okc[:4] + (3, 3) + okc[6:])) == 0


def test_attractor_census_refuses_on_the_host(mjx_mod):
    """Every refusal comes before any device call: the same ValueError with and
    without a GPU."""
    ac = mjx_mod.attractor_census
    adj = mjx_mod.random_regular_graph(3, 20, seed=0)
    with pytest.raises(ValueError, match="n = 50.*n <= 48"):
        ac(mjx_mod.random_regular_graph(3, 50, seed=0))
    for t_max in (-1, 1025):
        with pytest.raises(ValueError, match=f"t_max = {t_max}"):
            ac(adj, t_max)
    with pytest.raises(ValueError, match="2\\^20 = 1048576 configurations exceed max_configs = 1000"):
        ac(adj, max_configs=1000)
    with pytest.raises(ValueError, match="2\\^40"):
        ac(mjx_mod.random_regular_graph(3, 40, seed=0))
    # the LDS ceiling, with the byte count: n = 36 at t_max = 64, and n = 48 at the default t_max
    want = 1024 * 36 + 16 * 65 * 37 + 8 * 19 + 16 + 8 * 36 + 8 * 10 + 8 * 212
    with pytest.raises(ValueError, match=f"n = 36, t_max = 64 need {want} bytes"):
        ac(mjx_mod.random_regular_graph(3, 36, seed=0), 64)
    with pytest.raises(ValueError, match="n = 48, t_max = 32 need 77984 bytes"):
        ac(mjx_mod.random_regular_graph(3, 48, seed=0), max_configs=2 ** 48)
    with pytest.raises(ValueError, match="unknown kernel options \\['lds_entries'\\]"):
        ac(adj, kernel={"lds_entries": 4})
    with pytest.raises(ValueError, match="grid must be >= 0"):
        ac(adj, kernel={"grid": -1})
    with pytest.raises(ValueError, match="chunk_blocks"):
        ac(adj, chunk_blocks=0)
    asym = adj.copy()
    u = int(asym[0, 0])
    asym[0, 0] = next(v for v in range(1, 20) if v != u and v not in asym[0])
    with pytest.raises(ValueError, match="not symmetric"):
        ac(asym)
    out = adj.copy()
    out[3, 1] = 20
    with pytest.raises(ValueError, match="out of range"):
        ac(out)
    with pytest.raises(ValueError, match="at most 47"):
        ac(np.zeros((2, 48), np.int64))
    with pytest.raises(ValueError, match="neighbour array"):
        ac(np.ones(20, np.int64))


def test_compute_fails_loudly_without_gpu(mjx_mod):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(mjx_mod.MjxError):
        mjx_mod.attractor_census(mjx_mod.random_regular_graph(3, 12, seed=0))
    with pytest.raises(mjx_mod.MjxError):
        mjx_mod.attractor_census(mjx_mod.random_regular_graph(3, 12, seed=0), 4, chunk_blocks=8, kernel={"grid": 2})


def test_cli_parser_accepts_attractor_census():
    cli = importlib.import_module("mjx.cli")
    a = cli.build_parser().parse_args(["attractor-census", "--graph", "rrg", "--n", "16", "--d", "4", "--graph-seed",
                                       "5", "--t-max", "12", "--out", "x.npz"])
    assert (a.cmd, a.graph, a.n, a.d, a.graph_seed, a.t_max, a.out) == ("attractor-census", "rrg", 16, 4, 5, 12,
                                                                        "x.npz")
    a = cli.build_parser().parse_args(["attractor-census", "--graph", "er", "--n", "14", "--deg", "2.5"])
    assert (a.graph, a.deg, a.out, a.graph_seed, a.t_max, a.max_configs) == ("er", 2.5, None, 0, 32, None)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["attractor-census", "--graph", "ring"])
