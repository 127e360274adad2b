"""Consensus census, CPU side: the invariants of the brute-force oracle
(tests/census_oracle.py), the new entry points' ABI and argument checks, the
host-side refusals of ``census`` and the CLI parser.  No GPU."""
import ctypes
import functools
import importlib
import math
import os
import re

import numpy as np
import pytest

import census_oracle as co
from conftest import ROOT

NEW_SYMBOLS = ("mjx_census_lds", "mjx_census_ell", "mjx_census_csr")


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (step, n, T, oracle census).  Shared: never written."""
    import mjx
    if name == "rrg":
        n, T = 12, 3
        step = co.step_ell(mjx.random_regular_graph(3, n, seed=1))
    else:
        n, T = 13, 2
        step = co.step_csr(*mjx.erdos_renyi(n, 0.3, seed=3))
    return step, n, T, co.census(step, n, T)


@pytest.mark.parametrize("name", ["rrg", "er"])
def test_oracle_invariants(name):
    step, n, T, res = _case(name)
    counts = res["counts"]
    # level 0 counts the all +1 configuration alone
    assert counts[0].tolist() == [0] * n + [1] and res["min_plus"][0] == n and res["witness_x"][0] == (1 << n) - 1
    # all +1 is a fixed point: the levels are nested, and the case is not degenerate
    assert (counts[:-1] <= counts[1:]).all()
    assert all((counts[t] != counts[t + 1]).any() for t in range(T)) and res["min_plus"][T] < n
    assert (counts <= np.array([math.comb(n, k) for k in range(n + 1)])[None, :]).all()
    # the witness rule: smallest weight, then smallest index, among the counted configurations
    S = co.configs(0, 1 << n, n)
    k = (S == 1).sum(axis=1)
    for t in range(T + 1):
        if t:
            S = step(S)
        hit = np.flatnonzero((S == 1).all(axis=1))
        assert np.array_equal(np.bincount(k[hit], minlength=n + 1), counts[t])
        kmin = k[hit].min()
        assert res["min_plus"][t] == kmin and res["witness_x"][t] == hit[k[hit] == kmin].min()
        assert np.array_equal(res["witness"][t], co.spins(res["witness_x"][t], n))
    # the rule is monotone, so the counted set is an up-set: raising one spin keeps a configuration counted
    counted = set(hit.tolist())
    rng = np.random.default_rng(0)
    for x in rng.choice(hit, size=min(200, hit.size), replace=False).tolist() + [int(res["witness_x"][T])]:
        for v in range(n):
            assert (x | (1 << v)) in counted


def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "64-config block" in src and "Witness" in src, "the definitions belong to the contract"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    raw = ctypes.CDLL(mjx_mod.lib_path())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(raw, name)
    assert len(mjx_mod._lib.SIGNATURES["mjx_census_ell"]) == 12 and len(mjx_mod._lib.SIGNATURES["mjx_census_csr"]) == 12
    assert mjx_mod.load_library().mjx_abi_version() == 2


def test_lds_formula_and_argument_checks_without_gpu(mjx_mod):
    lib = mjx_mod.load_library()
    EINVAL, ERANGE = 1, 3
    for n in range(1, 49):
        # two levels [node][lane], counts and keys, level-0 patterns, row offsets, neighbour bytes
        want = 1024 * n + 56 * (n + 2) + 8 * n + 8 * (-(-(n + 1) // 4)) + 8 * (-(-(47 * n) // 8))
        assert lib.mjx_census_lds(n) == want
    assert lib.mjx_census_lds(48) <= 64 * 1024
    for n in (0, -1, 49, 1 << 40):
        assert lib.mjx_census_lds(n) == -1
    # compute entry points: validation fails before any pointer is read
    a = ctypes.c_void_p(64)
    ok = (a, 16, 3, 3, 1, 0, 1024, 0, a, a, a, None)
    assert lib.mjx_census_ell(*(ok[:1] + (49,) + ok[2:])) == ERANGE                    # n > 48
    assert lib.mjx_census_ell(*(ok[:3] + (7, 1) + ok[5:])) == ERANGE                   # T = 7
    assert lib.mjx_census_ell(*(ok[:2] + (48,) + ok[3:])) == ERANGE                    # d > 47
    assert lib.mjx_census_ell(*(ok[:1] + (0,) + ok[2:])) == EINVAL                     # n < 1
    assert lib.mjx_census_ell(*(ok[:3] + (0, 0) + ok[5:])) == EINVAL                   # T = -1
    assert lib.mjx_census_ell(*(ok[:6] + (1025,) + ok[7:])) == EINVAL                  # block_hi > B
    assert lib.mjx_census_ell(*(ok[:5] + (5, 4) + ok[7:])) == EINVAL                   # lo > hi
    assert lib.mjx_census_ell(*(ok[:5] + (-1, 4) + ok[7:])) == EINVAL
    assert lib.mjx_census_ell(*(ok[:7] + (-1,) + ok[8:])) == EINVAL                    # grid < 0
    for k in (8, 9, 10):
        assert lib.mjx_census_ell(*(ok[:k] + (None,) + ok[k + 1:])) == EINVAL          # counts, keys, flag
    assert lib.mjx_census_ell(*((None,) + ok[1:])) == EINVAL                           # d > 0 without adj
    assert lib.mjx_census_ell(*(ok[:5] + (7, 7) + ok[7:])) == 0                        # an empty range: nothing to do
    okc = (a, a, 16, 3, 1, 0, 1024, 0, a, a, a, None)
    assert lib.mjx_census_csr(*((None,) + okc[1:])) == EINVAL
    assert lib.mjx_census_csr(*(okc[:2] + (49,) + okc[3:])) == ERANGE
    assert lib.mjx_census_csr(*(okc[:3] + (4, 4) + okc[5:])) == ERANGE
    assert lib.mjx_census_csr(*(okc[:6] + (1025,) + okc[7:])) == EINVAL
    assert lib.mjx_census_csr(*(okc[:2] + (5,) + okc[3:6] + (2,) + okc[7:])) == EINVAL  # n < 6: one block


def test_package_exports_census(mjx_mod):
    mod = importlib.import_module("mjx.census")
    assert mjx_mod.census is mod.census and "census" in mjx_mod.__all__


def test_census_refuses_on_the_host(mjx_mod):
    """Every refusal comes before any device call: the same ValueError with and
    without a GPU."""
    adj = mjx_mod.random_regular_graph(3, 20, seed=0)
    big = mjx_mod.random_regular_graph(3, 50, seed=0)
    with pytest.raises(ValueError, match="n = 50.*n <= 48"):
        mjx_mod.census(big, 1, 1)
    for p, c in ((7, 1), (4, 4), (0, 0)):
        with pytest.raises(ValueError, match="p \\+ c - 1"):
            mjx_mod.census(adj, p, c)
    with pytest.raises(ValueError, match="2\\^20 = 1048576 configurations exceed max_configs = 1000"):
        mjx_mod.census(adj, 1, 1, max_configs=1000)
    with pytest.raises(ValueError, match="2\\^40"):
        mjx_mod.census(mjx_mod.random_regular_graph(3, 40, seed=0), 1, 1)
    with pytest.raises(ValueError, match="unknown kernel options \\['lds_entries'\\]"):
        mjx_mod.census(adj, 1, 1, kernel={"lds_entries": 4})
    with pytest.raises(ValueError, match="chunk_blocks"):
        mjx_mod.census(adj, 1, 1, chunk_blocks=0)
    asym = adj.copy()
    u = int(asym[0, 0])
    asym[0, 0] = next(v for v in range(1, 20) if v != u and v not in asym[0])
    with pytest.raises(ValueError, match="not symmetric"):
        mjx_mod.census(asym, 1, 1)
    out = adj.copy()
    out[3, 1] = 20
    with pytest.raises(ValueError, match="out of range"):
        mjx_mod.census(out, 1, 1)
    with pytest.raises(ValueError, match="neighbour array"):
        mjx_mod.census(np.ones(20, np.int64), 1, 1)


def test_cli_parser_accepts_census():
    cli = importlib.import_module("mjx.cli")
    a = cli.build_parser().parse_args(["census", "--graph", "rrg", "--n", "16", "--d", "4", "--graph-seed", "5",
                                       "--p", "3", "--c", "1", "--out", "x.npz"])
    assert (a.cmd, a.graph, a.n, a.d, a.graph_seed, a.p, a.c, a.out) == ("census", "rrg", 16, 4, 5, 3, 1, "x.npz")
    a = cli.build_parser().parse_args(["census", "--graph", "er", "--n", "14", "--deg", "2.5", "--p", "1", "--c", "1"])
    assert (a.graph, a.deg, a.out, a.graph_seed) == ("er", 2.5, None, 0)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["census", "--n", "16"])
