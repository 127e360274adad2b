"""Quench restarts, CPU side: the new entry points' ABI and LDS budget, the
host-side refusals of ``quench_restarts`` (all before any device call), the
seed rule and the best-of-K pick as pure host functions, the CLI parser.
No GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("mjx_quench_jobs_lds", "mjx_quench_jobs_ell", "mjx_quench_jobs_csr")


def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "REFUSED" in src, "the spill-or-refuse decision belongs to the header"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    lib = mjx_mod.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name)
    assert mjx_mod.quench_restarts is importlib.import_module("mjx.quench").quench_restarts
    assert "quench_restarts" in mjx_mod.__all__


def _caps(lib, n, d, T):
    caps = (ctypes.c_int64 * (T + 1))()
    assert lib.mjx_ell_ball_bound(n, d, T, caps) == 0
    return caps


def test_lds_budget_grows_with_n_and_T_and_ends_at_64_kib(mjx_mod):
    lib = mjx_mod.load_library()

    def lds(n, T, d=4):
        return lib.mjx_quench_jobs_lds(n, T, _caps(lib, max(n, 1), d, min(max(T, 0), 6)))

    # the documented formula: T + 2 bitmaps of 2 ceil(n/64) words, lists 1, caps[1..T], caps[T]
    assert lds(10000, 3) == (4 * (5 * 2 * 157 + 1 + 5 + 21 + 85 + 85) + 15) // 16 * 16
    assert lds(96, 3) == (4 * (5 * 2 * 2 + 1 + 5 + 21 + 85 + 85) + 15) // 16 * 16
    assert lds(50, 0) == (4 * (2 * 2 * 1 + 1 + 1) + 15) // 16 * 16
    sizes = [lds(n, 3) for n in (64, 65, 1000, 10000, 100000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and 0 < sizes[0] and sizes[-1] <= 64 * 1024
    by_T = [lds(10000, T) for T in range(7)]
    assert all(a < b for a, b in zip(by_T, by_T[1:])) and by_T[0] > 0
    assert lds(200000, 3) == -1 and lds(100000, 6) == -1           # past the ceiling
    assert lds(10000, 7) == -1 and lds(10000, -1) == -1 and lds(0, 3) == -1
    assert lib.mjx_quench_jobs_lds(10000, 3, None) == -1


def test_compute_entry_points_validate_before_any_pointer_is_read(mjx_mod):
    lib = mjx_mod.load_library()
    EINVAL = 1
    a = ctypes.c_void_p(64)
    n, d, R, K = 1000, 4, 3, 2
    caps = _caps(lib, n, d, 3)
    ok = [a, n, d, 0, R, K, 3, 1, caps, a, a, 0, a, a, a, a, a, None]

    def ell(**kw):
        names = ["adj", "n", "d", "graph_stride", "R", "K", "p", "c", "caps", "s_np", "order", "order_stride_r",
                 "out_np", "flipped", "plus", "consensus", "flag", "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.mjx_quench_jobs_ell(*args)

    assert ell(p=7) == EINVAL and ell(p=0, c=0) == EINVAL and ell(p=4, c=4) == EINVAL
    assert ell(n=1 << 31) == EINVAL and ell(n=0) == EINVAL
    assert ell(R=0) == EINVAL and ell(K=0) == EINVAL
    for name in ("adj", "caps", "s_np", "order", "out_np", "flipped", "plus", "consensus", "flag"):
        assert ell(**{name: None}) == EINVAL, name
    assert ell(graph_stride=n) == EINVAL and ell(order_stride_r=n) == EINVAL
    big = _caps(lib, 200000, d, 3)
    assert ell(n=200000, caps=big) == EINVAL                        # does not fit the LDS
    csr = [a, a, n, R, K, 3, 1, caps, a, a, 0, a, a, a, a, a, None]
    assert lib.mjx_quench_jobs_csr(*([None] + csr[1:])) == EINVAL
    assert lib.mjx_quench_jobs_csr(*(csr[:5] + [7, 1] + csr[7:])) == EINVAL
    assert lib.mjx_quench_jobs_csr(*(csr[:8] + [None] + csr[9:])) == EINVAL


# ---- host-side refusals ---------------------------------------------------------
def test_refusals_happen_on_the_host(mjx_mod):
    """The same ValueError with and without a GPU: nothing here reaches the device."""
    n = 20
    adj = mjx_mod.random_regular_graph(3, n, seed=0)
    s = np.ones((2, n), np.int64)
    qr = mjx_mod.quench_restarts
    ident = np.arange(n)
    for bad in (np.zeros(n, np.int64), np.arange(n - 1), np.arange(1, n + 1), ident * 1.0,
                np.r_[np.arange(n - 1), n - 2], np.stack([ident, np.zeros(n, np.int64)])[None].repeat(2, 0)):
        K = 1 if np.ndim(bad) == 1 else np.shape(bad)[-2]
        with pytest.raises(ValueError, match="permutation"):
            qr(adj, s, 1, 1, restarts=K, orders=bad)
    with pytest.raises(ValueError, match="not both"):
        qr(adj, s, 1, 1, orders=ident, seed=3)
    with pytest.raises(ValueError, match="restarts = 3"):
        qr(adj, s, 1, 1, restarts=3, orders=np.stack([ident, ident[::-1]]))
    with pytest.raises(ValueError, match="restarts = 1"):
        qr(adj, s, 1, 1, orders=np.stack([ident, ident[::-1]]))
    with pytest.raises(ValueError, match="orders or seed"):
        qr(adj, s, 1, 1, restarts=2)
    with pytest.raises(ValueError, match="restarts must be >= 1"):
        qr(adj, s, 1, 1, restarts=0, seed=1)
    with pytest.raises(ValueError, match="R = 2 starts"):
        qr(adj, s, 1, 1, orders=np.tile(ident, (3, 1, 1)))
    with pytest.raises(ValueError, match="p \\+ c - 1"):
        qr(adj, s, 7, 1)
    # packed input: n * words int64 words are no (n,) or (R, n) spins
    with pytest.raises(ValueError, match="packed input"):
        qr(adj, np.zeros(n * 2, np.int64), 1, 1)
    # a graph per start is an ELL stack: CSR graphs, and a stack of another R, are refused
    csr = mjx_mod.Graph("csr", n)
    with pytest.raises(ValueError, match="CSR"):
        qr([csr, csr], s, 1, 1)
    with pytest.raises(ValueError, match="3 graphs for 2 starts"):
        qr(np.stack([adj] * 3), s, 1, 1)
    with pytest.raises(ValueError, match="unknown kernel options"):
        qr(adj, s, 1, 1, kernel={"lds_entries": 4})


# ---- the seed rule and the pick ---------------------------------------------------
def test_the_seed_rule_is_default_rng_of_seed_r_k(mjx_mod):
    mod = importlib.import_module("mjx.quench")
    n = 37
    for seed, r, k in ((7, 0, 0), (7, 3, 1), (0, 5, 2)):
        want = np.random.default_rng([seed, r, k]).permutation(n)
        assert np.array_equal(mod.restart_order(seed, r, k, n), want)
    o = mod._check_orders(None, 7, 3, 4, n)
    assert o.shape == (4, 3, n) and o.dtype == np.int32
    for r in range(4):
        for k in range(3):
            assert np.array_equal(o[r, k], np.random.default_rng([7, r, k]).permutation(n))
    assert len({o[r, k].tobytes() for r in range(4) for k in range(3)}) == 12, "the jobs' orders differ"
    # explicit orders: (n,) and (K, n) are shared by the starts, (R, K, n) is per start
    ident = np.arange(n)
    assert mod._check_orders(ident, None, 1, 4, n).shape == (1, 1, n)
    assert mod._check_orders(np.stack([ident, ident[::-1]]), None, 2, 4, n).shape == (1, 2, n)
    assert mod._check_orders(o, None, 3, 4, n).shape == (4, 3, n)
    assert np.array_equal(mod._check_orders(None, None, 1, 4, n), ident.reshape(1, 1, n))


def test_best_is_the_smallest_sum_with_the_first_index_on_ties(mjx_mod):
    mod = importlib.import_module("mjx.quench")
    sums = np.array([[10, 4, 4], [2, 2, 2], [6, 8, -2], [-4, 0, 0]])
    best = mod.pick_best(sums)
    assert best.dtype == np.int64 and best.tolist() == [1, 0, 2, 0]


# ---- CLI ---------------------------------------------------------------------------
def test_cli_parser_knows_restarts():
    cli = importlib.import_module("mjx.cli")
    base = ["quench", "--in", "x.npz", "--p", "3", "--c", "1"]
    a = cli.build_parser().parse_args(base)
    assert a.restarts == 0 and a.order_seed is None
    a = cli.build_parser().parse_args(base + ["--order-seed", "5"])
    assert a.restarts == 0 and a.order_seed == 5
    a = cli.build_parser().parse_args(base + ["--restarts", "2", "--order-seed", "5"])
    assert (a.restarts, a.order_seed) == (2, 5)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--restarts", "2"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--restarts", "-1", "--order-seed", "5"])
