"""The (1, 2) exchange descent, CPU side: what the numpy oracle
(tests/quench_exchange_oracle.py) delivers, the lemma the kernel's candidate
set rests on, the entry points' ABI and LDS budget, the host-side refusals of
``quench_exchange`` (all before any device call) and the CLI parser.  No GPU."""
import ctypes
import functools
import importlib
import os
import re

import numpy as np
import pytest

import quench_cases
import quench_exchange_oracle as xo
import quench_oracle as qo
from conftest import ROOT

NEW_SYMBOLS = ("mjx_quench_exchange_jobs_lds", "mjx_quench_exchange_jobs_ell", "mjx_quench_exchange_jobs_csr")
# name -> starts taken from the shared table (the first ones, as the GPU files take them)
STARTS = {"rrg_d4_n96_T3": 16, "rrg_d3_n200_T2": 32}


def _order(r, n):
    return np.random.default_rng([5, r, 0]).permutation(n)


@functools.lru_cache(maxsize=None)
def _runs(name):
    """Per consensus start of the case: (start, quench result, exchange result, the drops of its committed
    exchanges as (state before the add, j, a)).  Shared: never written."""
    spec, step, S, T = quench_cases._case(name)
    n = S.shape[1]
    out = []
    for r in range(STARTS[name]):
        drops = []
        w = xo.exchange(step, S[r], T, _order(r, n), on_drop=lambda x, j, a: drops.append((x.copy(), j, a)))
        if w["consensus"]:
            out.append((S[r], qo.quench(step, S[r:r + 1], T, _order(r, n)), w, drops))
    return out


@pytest.mark.parametrize("name", sorted(STARTS))
def test_the_oracles_result_is_a_consensus_local_minimum_no_heavier_than_the_quench(mjx_mod, name):
    _, step, _, T = quench_cases._case(name)
    runs = _runs(name)
    assert len(runs) >= 3
    improved = 0
    for s, q, w, _ in runs:
        conf = w["conf"]
        g = qo.flip_gains(step, conf[None, :], T)
        assert g["consensus"][0] and g["n_removable"][0] == 0
        plus, plus_q = int((conf == 1).sum()), int((q["conf"][0] == 1).sum())
        assert w["plus_quench"] == plus_q and w["flipped"] == q["flipped"][0]
        assert plus <= plus_q - w["exchanges"], "every exchange lowers the weight by at least 1"
        assert (w["exchanges"] == 0) == np.array_equal(conf, q["conf"][0])
        assert w["converged"] and 1 <= w["passes"] <= 8
        improved += plus < plus_q
    assert improved >= 2, f"{name}: the descent has to move somewhere"


@pytest.mark.parametrize("name", sorted(STARTS))
def test_every_committed_drop_lies_in_the_lemmas_set(mjx_mod, name):
    """dist(a, D_t) <= t + 2 for some t < T, D_t = the level-t changes of the add."""
    spec, step, _, T = quench_cases._case(name)
    nbrs = xo.neighbours_ell(spec[1])
    seen = 0
    for _, _, _, drops in _runs(name):
        for x, j, a in drops:
            D, allowed = xo.lemma_set(step, nbrs, x, j, T)
            assert D[0].tolist() == [j] and len(D) == T
            assert allowed <= xo.ball(nbrs, [j], 2 * T)
            assert a in allowed, (j, a)
            seen += 1
    assert seen >= 8, f"{name}: only {seen} drops to check"


def test_the_oracle_without_consensus_and_at_T0(mjx_mod):
    _, step, S, _ = quench_cases._case("rrg_d4_n96_T3")
    s = -np.ones(96, np.int64)
    w = xo.exchange(step, s, 3, np.arange(96))
    assert not w["consensus"] and np.array_equal(w["conf"], s)
    assert (w["flipped"], w["exchanges"], w["passes"], w["converged"]) == (0, 0, 0, True)
    one = np.ones(96, np.int64)
    w = xo.exchange(step, one, 0, np.arange(96))
    assert w["consensus"] and np.array_equal(w["conf"], one) and w["exchanges"] == 0 and w["converged"]


# ---- ABI ------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    lib = mjx_mod.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name)
    assert mjx_mod.quench_exchange is importlib.import_module("mjx.quench").quench_exchange
    assert "quench_exchange" in mjx_mod.__all__


def _caps(lib, n, d, T):
    caps = (ctypes.c_int64 * (T + 1))()
    assert lib.mjx_ell_ball_bound(n, d, T, caps) == 0
    return caps


def test_lds_budget_is_the_jobs_plus_the_candidate_list_and_ends_at_64_kib(mjx_mod):
    lib = mjx_mod.load_library()

    def both(n, T, d=4):
        caps = _caps(lib, n, d, T)
        cap2T = _caps(lib, n, d, 2 * T)[2 * T]
        return lib.mjx_quench_jobs_lds(n, T, caps), lib.mjx_quench_exchange_jobs_lds(n, T, caps, cap2T), cap2T

    for n, T, ball in ((10000, 3, 5461), (96, 3, 96), (10000, 2, 341), (10000, 1, 21), (50, 0, 1)):
        jobs, ex, cap2T = both(n, T)
        assert cap2T == ball
        assert jobs > 0 and ex == (jobs + 4 * ball + 15) // 16 * 16
    assert both(10000, 3)[1] == (4 * (5 * 2 * 157 + 1 + 5 + 21 + 85 + 85) + 15) // 16 * 16 + 4 * 5461 + 12
    # cap2T past n counts as n
    caps = _caps(lib, 96, 4, 3)
    assert lib.mjx_quench_exchange_jobs_lds(96, 3, caps, 10 ** 9) == lib.mjx_quench_exchange_jobs_lds(96, 3, caps, 96)
    # the ceiling: a quench job of n = 1e5 fits, the exchange's list on top of it does not
    jobs, ex, _ = both(100000, 3)
    assert 0 < jobs <= 64 * 1024 and ex == -1
    jobs, ex, _ = both(50000, 3)
    assert 0 < jobs < ex <= 64 * 1024
    # T past 3, caps that are none
    c6 = _caps(lib, 10000, 4, 6)
    assert lib.mjx_quench_jobs_lds(10000, 4, c6) > 0 and lib.mjx_quench_exchange_jobs_lds(10000, 4, c6, 5461) == -1
    c3 = _caps(lib, 10000, 4, 3)
    assert lib.mjx_quench_exchange_jobs_lds(10000, 3, c3, 0) == -1
    assert lib.mjx_quench_exchange_jobs_lds(10000, 3, None, 5461) == -1
    assert lib.mjx_quench_exchange_jobs_lds(0, 3, c3, 5461) == -1
    assert lib.mjx_quench_exchange_jobs_lds(10000, -1, c3, 5461) == -1


def test_compute_entry_points_validate_before_any_pointer_is_read(mjx_mod):
    lib = mjx_mod.load_library()
    EINVAL = 1
    a = ctypes.c_void_p(64)
    n, d, R, K = 1000, 4, 3, 2
    caps = _caps(lib, n, d, 3)
    names = ["adj", "n", "d", "graph_stride", "R", "K", "p", "c", "caps", "cap2T", "max_passes", "s_np", "order",
             "order_stride_r", "rank_work", "out_np", "flipped", "plus", "plus_quench", "exchanges", "passes",
             "converged", "consensus", "flag", "stats", "stream"]
    ok = [a, n, d, 0, R, K, 3, 1, caps, 1000, 8, a, a, 0, a, a, a, a, a, a, a, a, a, a, None, None]
    assert len(names) == len(ok) == len(mjx_mod._lib.SIGNATURES["mjx_quench_exchange_jobs_ell"])

    def ell(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.mjx_quench_exchange_jobs_ell(*args)

    assert ell(p=4) == EINVAL and ell(p=3, c=2) == EINVAL and ell(p=0, c=0) == EINVAL and ell(p=7) == EINVAL
    assert ell(max_passes=0) == EINVAL and ell(max_passes=-1) == EINVAL and ell(cap2T=0) == EINVAL
    assert ell(n=1 << 31) == EINVAL and ell(n=0) == EINVAL and ell(R=0) == EINVAL and ell(K=0) == EINVAL
    for name in ("adj", "caps", "s_np", "order", "rank_work", "out_np", "flipped", "plus", "plus_quench", "exchanges",
                 "passes", "converged", "consensus", "flag"):
        assert ell(**{name: None}) == EINVAL, name
    assert ell(graph_stride=n) == EINVAL and ell(order_stride_r=n) == EINVAL
    big = _caps(lib, 100000, d, 3)
    assert ell(n=100000, caps=big, cap2T=5461) == EINVAL            # does not fit the LDS
    cnames = ["row_ptr", "col"] + [k for k in names[1:] if k not in ("d", "graph_stride")]
    cok = [a, a] + [v for k, v in zip(names[1:], ok[1:]) if k not in ("d", "graph_stride")]
    assert len(cok) == len(mjx_mod._lib.SIGNATURES["mjx_quench_exchange_jobs_csr"])

    def csr(**kw):
        args = list(cok)
        for k, v in kw.items():
            args[cnames.index(k)] = v
        return lib.mjx_quench_exchange_jobs_csr(*args)

    assert csr(row_ptr=None) == EINVAL and csr(p=4) == EINVAL and csr(max_passes=0) == EINVAL
    assert csr(rank_work=None) == EINVAL and csr(converged=None) == EINVAL and csr(caps=None) == EINVAL


# ---- host-side refusals ---------------------------------------------------------
def test_refusals_happen_on_the_host(mjx_mod):
    """The same ValueError with and without a GPU: nothing here reaches the device."""
    n = 20
    adj = mjx_mod.random_regular_graph(3, n, seed=0)
    s = np.ones((2, n), np.int64)
    qx = mjx_mod.quench_exchange
    ident = np.arange(n)
    for p, c in ((4, 1), (3, 2), (1, 4), (6, 1)):
        with pytest.raises(ValueError, match="p \\+ c - 1 <= 3"):
            qx(adj, s, p, c)
    with pytest.raises(ValueError, match="p \\+ c - 1"):
        qx(adj, s, 7, 1)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError), match="max_passes"):
            qx(adj, s, 1, 1, max_passes=bad)
    for bad in (np.zeros(n, np.int64), np.arange(n - 1), np.arange(1, n + 1), ident * 1.0,
                np.r_[np.arange(n - 1), n - 2], np.stack([ident, np.zeros(n, np.int64)])[None].repeat(2, 0)):
        K = 1 if np.ndim(bad) == 1 else np.shape(bad)[-2]
        with pytest.raises(ValueError, match="permutation"):
            qx(adj, s, 1, 1, restarts=K, orders=bad)
    with pytest.raises(ValueError, match="not both"):
        qx(adj, s, 1, 1, orders=ident, seed=3)
    with pytest.raises(ValueError, match="restarts = 3"):
        qx(adj, s, 1, 1, restarts=3, orders=np.stack([ident, ident[::-1]]))
    with pytest.raises(ValueError, match="orders or seed"):
        qx(adj, s, 1, 1, restarts=2)
    with pytest.raises(ValueError, match="restarts must be >= 1"):
        qx(adj, s, 1, 1, restarts=0, seed=1)
    with pytest.raises(ValueError, match="packed input"):
        qx(adj, np.zeros(n * 2, np.int64), 1, 1)
    csr = mjx_mod.Graph("csr", n)
    with pytest.raises(ValueError, match="CSR"):
        qx([csr, csr], s, 1, 1)
    with pytest.raises(ValueError, match="3 graphs for 2 starts"):
        qx(np.stack([adj] * 3), s, 1, 1)
    with pytest.raises(ValueError, match="unknown kernel options"):
        qx(adj, s, 1, 1, kernel={"lds_entries": 4})
    # 1e5 nodes of degree 4 at T = 3: the quench job fits the LDS, the candidate list on top does not
    big = 100_000
    i = np.arange(big)
    lattice = np.stack([(i - 1) % big, (i + 1) % big, (i - 2) % big, (i + 2) % big], axis=1)
    with pytest.raises(ValueError, match="quench_exchange: .* does not fit"):
        qx(lattice, np.ones(big, np.int64), 3, 1)


# ---- CLI ---------------------------------------------------------------------------
def test_cli_parser_knows_exchange():
    cli = importlib.import_module("mjx.cli")
    base = ["quench", "--in", "x.npz", "--p", "3", "--c", "1"]
    a = cli.build_parser().parse_args(base)
    assert a.exchange is False and a.max_passes is None
    a = cli.build_parser().parse_args(base + ["--restarts", "2", "--order-seed", "5", "--exchange"])
    assert a.exchange is True and a.max_passes is None and (a.restarts, a.order_seed) == (2, 5)
    a = cli.build_parser().parse_args(base + ["--restarts", "1", "--order-seed", "5", "--exchange", "--max-passes", "3"])
    assert a.exchange is True and a.max_passes == 3
    for bad in (["--exchange"], ["--exchange", "--order-seed", "5"], ["--exchange", "--restarts", "2"],
                ["--restarts", "2", "--order-seed", "5", "--max-passes", "3"],
                ["--restarts", "2", "--order-seed", "5", "--exchange", "--max-passes", "0"],
                ["--restarts", "2", "--order-seed", "5", "--exchange", "--schedule", "regions"],
                ["--exchange", "--schedule", "regions"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)
