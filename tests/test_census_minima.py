"""Census of the minimal consensus sets, CPU side: the invariants of the
brute-force oracle (tests/census_minima_oracle.py), the new entry points' ABI
and argument checks, the host-side refusals of ``census_minima`` and the CLI
parser.  No GPU."""
import ctypes
import functools
import importlib
import os
import re

import numpy as np
import pytest

import census_minima_oracle as cm
import census_oracle as co
from conftest import ROOT

NEW_SYMBOLS = ("mjx_census_mask_ell", "mjx_census_mask_csr", "mjx_census_minima")
# minima[3] of networkx.random_regular_graph(d, n, seed=1), rows sorted, from the first weight that has one
QUOTED = {(3, 12): (7, [8, 61]), (4, 16): (8, [18, 1547, 448, 2]), (3, 18): (10, [2, 247, 490])}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (n, T, oracle census of the minima).  Shared: never written."""
    import mjx
    if name == "rrg":
        n, T = 12, 3
        step = co.step_ell(mjx.random_regular_graph(3, n, seed=1))
    else:
        n, T = 13, 2
        step = co.step_csr(*mjx.erdos_renyi(n, 0.3, seed=3))
    return n, T, cm.census_minima(step, n, T), co.census(step, n, T)


@pytest.mark.parametrize("name", ["rrg", "er"])
def test_oracle_invariants(name):
    n, T, res, cen = _case(name)
    U, M, k = res["U"], res["M"], cm.weights(n)
    assert np.array_equal(res["counts"], cen["counts"])
    assert not (M & ~U).any()                                # M_t is a part of U_t
    x = np.arange(1 << n, dtype=np.int64)
    for t in range(T + 1):
        members = np.flatnonzero(M[t])
        # an antichain: no minimum lies below another one
        for a in members.tolist():
            assert not ((members & a) == a)[members != a].any()
        # every x of U_t lies above some minimum: drop removable nodes until none is left
        y = x[U[t]].copy()
        for _ in range(n):
            for i in range(n):
                can = ((y >> i) & 1).astype(bool) & U[t][y ^ (1 << i)]
                y = np.where(can, y ^ (1 << i), y)
        assert M[t][y].all() and ((y & x[U[t]]) == y).all()
        # the three invariants of include/mjx.h
        lo = cen["min_plus"][t]
        assert res["minima"][t][lo] == res["counts"][t][lo] and not res["minima"][t][:lo].any()
        assert (res["minima"][t] <= res["counts"][t]).all()
        hit = members[k[members] == res["max_plus"][t]]
        assert res["heaviest_x"][t] == hit.max() and k[members].max() == res["max_plus"][t]
    assert res["minima"][0].tolist() == [0] * n + [1]
    assert np.array_equal(res["minima"].sum(axis=1), M.sum(axis=1))
    # not degenerate: the last level has minima at two weights or more
    assert (res["minima"][T] > 0).sum() >= 2
    # the words of the ABI hold the same bits
    W = cm.words(U, n)
    assert W.shape == (T + 1, 1 << (n - 6))
    assert all(bool((int(W[T, a >> 6]) >> (a & 63)) & 1) == bool(U[T, a]) for a in range(0, 1 << n, 37))


@pytest.mark.parametrize("d,n", list(QUOTED))
def test_the_quoted_tables(d, n):
    nx = pytest.importorskip("networkx")
    G = nx.random_regular_graph(d, n, seed=1)
    adj = np.array([sorted(G[v]) for v in range(n)], dtype=np.int64)
    res = cm.census_minima(co.step_ell(adj), n, 3)
    first, tail = QUOTED[(d, n)]
    want = [0] * first + tail
    assert res["minima"][3].tolist() == want + [0] * (n + 1 - len(want))


def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "Heaviest minimum" in src and "Minimal set" in src, "the definitions belong to the contract"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    raw = ctypes.CDLL(mjx_mod.lib_path())
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(raw, name)
    sig = mjx_mod._lib.SIGNATURES
    assert len(sig["mjx_census_mask_ell"]) == 13 and len(sig["mjx_census_mask_csr"]) == 13
    assert len(sig["mjx_census_minima"]) == 9
    assert len(sig["mjx_census_ell"]) == 12 and len(sig["mjx_census_csr"]) == 12
    assert mjx_mod.load_library().mjx_abi_version() == 2


def test_argument_checks_without_gpu(mjx_mod):
    """Validation fails before any pointer is read or anything is launched."""
    lib = mjx_mod.load_library()
    EINVAL, ERANGE = 1, 3
    a = ctypes.c_void_p(64)
    ok = (a, 16, 3, 3, 1, 0, 1024, 0, a, a, a, a, None)
    ell = lib.mjx_census_mask_ell
    assert ell(*(ok[:1] + (49,) + ok[2:])) == ERANGE                     # n > 48
    assert ell(*(ok[:3] + (7, 1) + ok[5:])) == ERANGE                    # T = 7
    assert ell(*(ok[:2] + (48,) + ok[3:])) == ERANGE                     # d > 47
    assert ell(*(ok[:1] + (0,) + ok[2:])) == EINVAL                      # n < 1
    assert ell(*(ok[:3] + (0, 0) + ok[5:])) == EINVAL                    # T = -1
    assert ell(*(ok[:3] + (-1, 3) + ok[5:])) == EINVAL                   # p < 0
    assert ell(*(ok[:6] + (1025,) + ok[7:])) == EINVAL                   # block_hi > B
    assert ell(*(ok[:5] + (5, 4) + ok[7:])) == EINVAL                    # lo > hi
    assert ell(*(ok[:5] + (-1, 4) + ok[7:])) == EINVAL
    assert ell(*(ok[:7] + (-1,) + ok[8:])) == EINVAL                     # grid < 0
    for k in (8, 9, 10, 11):
        assert ell(*(ok[:k] + (None,) + ok[k + 1:])) == EINVAL           # counts, keys, flag, mask
    assert ell(*((None,) + ok[1:])) == EINVAL                            # d > 0 without adj
    assert ell(*(ok[:2] + (-1,) + ok[3:])) == EINVAL                     # d < 0
    assert ell(*(ok[:5] + (7, 7) + ok[7:])) == 0                         # an empty range: nothing to do
    assert ell(*(ok[:5] + (3, 3) + ok[7:])) == 0                         # pass 1 takes any range
    okc = (a, a, 16, 3, 1, 0, 1024, 0, a, a, a, a, None)
    csr = lib.mjx_census_mask_csr
    assert csr(*((None,) + okc[1:])) == EINVAL
    assert csr(*(okc[:2] + (49,) + okc[3:])) == ERANGE
    assert csr(*(okc[:3] + (4, 4) + okc[5:])) == ERANGE
    assert csr(*(okc[:2] + (0,) + okc[3:])) == EINVAL
    assert csr(*(okc[:6] + (1025,) + okc[7:])) == EINVAL
    assert csr(*(okc[:2] + (5,) + okc[3:6] + (2,) + okc[7:])) == EINVAL   # n < 6: one block
    assert csr(*(okc[:7] + (-1,) + okc[8:])) == EINVAL
    assert csr(*(okc[:11] + (None,) + okc[12:])) == EINVAL               # no mask
    assert csr(*(okc[:5] + (9, 9) + okc[7:])) == 0
    # pass 2: (mask, n, T, block_lo, block_hi, grid, minima, heaviest_key, stream)
    okm = (a, 16, 3, 0, 1024, 0, a, a, None)
    mn = lib.mjx_census_minima
    for k in (0, 6, 7):
        assert mn(*(okm[:k] + (None,) + okm[k + 1:])) == EINVAL          # mask, minima, heaviest_key
    assert mn(*(okm[:1] + (0,) + okm[2:])) == EINVAL                     # n < 1
    assert mn(*(okm[:2] + (-1,) + okm[3:])) == EINVAL                    # T < 0
    assert mn(*(okm[:5] + (-1,) + okm[6:])) == EINVAL                    # grid < 0
    assert mn(*(okm[:1] + (49,) + okm[2:])) == ERANGE                    # n > 48
    assert mn(*(okm[:2] + (7,) + okm[3:])) == ERANGE                     # T > 6
    assert mn(*(okm[:4] + (1025,) + okm[5:])) == EINVAL                  # block_hi > B
    assert mn(*(okm[:3] + (128, 64) + okm[5:])) == EINVAL                # lo > hi
    assert mn(*(okm[:3] + (-64, 64) + okm[5:])) == EINVAL
    assert mn(*(okm[:3] + (1, 64) + okm[5:])) == EINVAL                  # block_lo not a multiple of 64
    assert mn(*(okm[:3] + (32, 1024) + okm[5:])) == EINVAL
    assert mn(*(okm[:3] + (0, 65) + okm[5:])) == EINVAL                  # block_hi neither a multiple of 64 nor B
    assert mn(*(okm[:3] + (64, 1000) + okm[5:])) == EINVAL
    assert mn(*(okm[:3] + (64, 64) + okm[5:])) == 0                      # an empty range: nothing to do
    assert mn(*(okm[:3] + (1024, 1024) + okm[5:])) == 0
    assert mn(*((a, 10, 3, 0, 17) + okm[5:])) == EINVAL                  # n = 10: B = 16 is the only short end
    assert mn(*((a, 10, 3, 16, 16) + okm[5:])) == EINVAL                 # ... and 16 is no multiple of 64 to start at
    assert mn(*((a, 5, 3, 0, 2) + okm[5:])) == EINVAL                    # n < 6: one block


def test_package_exports_census_minima(mjx_mod):
    mod = importlib.import_module("mjx.census")
    assert mjx_mod.census_minima is mod.census_minima and "census_minima" in mjx_mod.__all__
    assert mjx_mod.census is mod.census


def test_census_minima_refuses_on_the_host(mjx_mod):
    """Every refusal comes before any device call: the same ValueError with and
    without a GPU."""
    adj = mjx_mod.random_regular_graph(3, 20, seed=0)
    with pytest.raises(ValueError, match="n = 50.*n <= 48"):
        mjx_mod.census_minima(mjx_mod.random_regular_graph(3, 50, seed=0), 1, 1)
    for p, c in ((7, 1), (4, 4), (0, 0)):
        with pytest.raises(ValueError, match="p \\+ c - 1"):
            mjx_mod.census_minima(adj, p, c)
    # the bitmap: (T+1) * 2^n / 8 bytes
    with pytest.raises(ValueError, match="2\\^20 = 1048576 configurations exceed max_configs = 1000; the bitmap "
                                         "of the 4 levels would take \\(T\\+1\\) \\* 2\\^n / 8 = 524288 bytes"):
        mjx_mod.census_minima(adj, 3, 1, max_configs=1000)
    # the default is 2^34 (census: 2^36)
    with pytest.raises(ValueError, match="2\\^36 = 68719476736 configurations exceed max_configs = 17179869184; "
                                         ".* = 34359738368 bytes"):
        mjx_mod.census_minima(mjx_mod.random_regular_graph(3, 36, seed=0), 3, 1)
    with pytest.raises(ValueError, match="unknown kernel options \\['lds_entries'\\]"):
        mjx_mod.census_minima(adj, 1, 1, kernel={"lds_entries": 4})
    with pytest.raises(ValueError, match="grid"):
        mjx_mod.census_minima(adj, 1, 1, kernel={"grid": -1})
    with pytest.raises(ValueError, match="chunk_blocks"):
        mjx_mod.census_minima(adj, 1, 1, chunk_blocks=0)
    asym = adj.copy()
    u = int(asym[0, 0])
    asym[0, 0] = next(v for v in range(1, 20) if v != u and v not in asym[0])
    with pytest.raises(ValueError, match="not symmetric"):
        mjx_mod.census_minima(asym, 1, 1)
    out = adj.copy()
    out[3, 1] = 20
    with pytest.raises(ValueError, match="out of range"):
        mjx_mod.census_minima(out, 1, 1)
    with pytest.raises(ValueError, match="neighbour array"):
        mjx_mod.census_minima(np.ones(20, np.int64), 1, 1)
    with pytest.raises(TypeError):
        mjx_mod.census_minima(adj, 1, 1, 2 ** 20)                        # the options are keyword-only


def test_cli_parser_accepts_minima():
    cli = importlib.import_module("mjx.cli")
    base = ["census", "--graph", "rrg", "--n", "16", "--d", "4", "--p", "3", "--c", "1"]
    a = cli.build_parser().parse_args(base)
    assert a.minima is False and a.max_configs is None
    a = cli.build_parser().parse_args(base + ["--minima", "--max-configs", "65536"])
    assert a.minima is True and a.max_configs == 65536 and (a.cmd, a.n, a.d, a.p, a.c) == ("census", 16, 4, 3, 1)
