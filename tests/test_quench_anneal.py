"""The Metropolis add / drop walk inside the consensus set, CPU side: what the
numpy oracle (tests/quench_anneal_oracle.py) delivers, ``anneal_thresholds``,
the entry points' ABI and LDS budget, the host-side refusals of
``quench_anneal`` (all before any device call) and the CLI parser.  No GPU."""
import ctypes
import functools
import importlib
import os
import re

import numpy as np
import pytest

import quench_anneal_oracle as ao
import quench_cases
import quench_oracle as qo
from conftest import ROOT

NEW_SYMBOLS = ("mjx_quench_anneal_jobs_lds", "mjx_quench_anneal_jobs_ell", "mjx_quench_anneal_jobs_csr")
# name -> (starts taken from the shared table, sweeps)
RUNS = {"rrg_d4_n96_T3": (16, 16), "rrg_d3_n200_T2": (16, 8)}


def _orders(R, n, K=2):
    return np.stack([np.stack([np.random.default_rng([5, r, k]).permutation(n) for k in range(K)]) for r in range(R)])


@functools.lru_cache(maxsize=None)
def _run(name, sweeps=None):
    _, step, S, T = quench_cases._case(name)
    R, U = RUNS[name]
    U = U if sweeps is None else sweeps
    return ao.anneal_jobs(step, S[:R], T, _orders(R, S.shape[1]), ao.thresholds(np.linspace(1.0, 5.0, U)), 7)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_the_oracles_result_is_a_consensus_local_minimum_between_its_bounds(mjx_mod, name):
    _, step, S, T = quench_cases._case(name)
    R, U = RUNS[name]
    w = _run(name)
    cons = w["consensus"]
    assert cons.sum() >= 2 and (~cons).sum() >= 1
    plus = (w["conf"] == 1).sum(axis=2)
    assert w["trace"].shape == (R, 2, U) and w["trace"].dtype == np.int32
    assert (plus <= w["plus_best"]).all() and (w["plus_best"] <= w["plus_quench"]).all()
    assert (plus[cons] < w["plus_quench"][cons]).any(), f"{name}: the walk has to move somewhere"
    g = qo.flip_gains(step, w["conf"].reshape(-1, S.shape[1]), T)
    assert np.array_equal(g["consensus"], np.repeat(cons, 2)) and not g["n_removable"].any()
    # the trace is the weight after every sweep, plus_best its running minimum with the quench in front
    low = np.minimum(w["plus_quench"], w["trace"].min(axis=2))
    assert np.array_equal(w["plus_best"], low)
    first = np.argmax(w["trace"] == low[:, :, None], axis=2) + 1
    assert np.array_equal(w["best_sweep"], np.where(low < w["plus_quench"], first, 0))
    # every proposal is an add, a drop, a refusal or a -1 node that stays
    assert (w["moves"].sum(axis=2)[cons] <= U * S.shape[1]).all() and (w["moves"][cons][:, :, 2] > 0).all()
    assert np.array_equal(w["trace"][:, :, -1], w["plus_quench"] + w["moves"][:, :, 0] - w["moves"][:, :, 1])
    # without consensus: the start, flat trace, no moves
    assert np.array_equal(w["conf"][~cons], np.repeat(S[:R][~cons][:, None], 2, axis=1))
    assert not w["moves"][~cons].any() and not w["flipped"][~cons].any() and not w["best_sweep"][~cons].any()
    assert (w["trace"][~cons] == (S[:R][~cons] == 1).sum(axis=1)[:, None, None]).all()


def test_the_oracle_without_sweeps_is_the_quench(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, step, S, T = quench_cases._case(name)
    w = _run(name, 0)
    assert w["trace"].shape == (16, 2, 0) and not w["moves"].any() and not w["best_sweep"].any()
    orders = _orders(16, 96)
    for r in range(16):
        for k in range(2):
            q = qo.quench(step, S[r:r + 1], T, orders[r, k])
            assert np.array_equal(w["conf"][r, k], q["conf"][0]) and w["flipped"][r, k] == q["flipped"][0]
            assert w["consensus"][r] == q["consensus"][0]
    assert np.array_equal(w["plus_quench"], (w["conf"] == 1).sum(axis=2))
    assert np.array_equal(w["plus_best"], w["plus_quench"])


def test_the_oracles_stream_belongs_to_the_job(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, step, S, T = quench_cases._case(name)
    w = _run(name)
    r = int(np.flatnonzero(w["consensus"])[0])
    one = ao.anneal(step, S[r], T, _orders(16, 96)[r, 1], ao.thresholds(np.linspace(1.0, 5.0, 16)), 7, r=r, k=1)
    assert np.array_equal(one["conf"], w["conf"][r, 1]) and np.array_equal(one["trace"], w["trace"][r, 1])
    nodes, words = ao.proposals(96, 3, r, 1, 7)
    assert nodes.min() >= 0 and nodes.max() < 96 and words.dtype == np.uint32
    assert not np.array_equal(nodes, ao.proposals(96, 3, r, 0, 7)[0])
    assert not np.array_equal(nodes, ao.proposals(96, 3, r, 1, 7 + (1 << 32))[0])


# ---- thresholds -----------------------------------------------------------------------
def test_anneal_thresholds(mjx_mod):
    at = mjx_mod.anneal_thresholds
    t = at([0.0, 1e-12, 1.0, 2.5, 22.0, 23.0, 800.0, np.inf])
    assert t.dtype == np.uint32 and t[0] == 2 ** 32 - 1 and t[-1] == 0 and t[-2] == 0
    assert t[2] == int(np.floor(np.exp(-1.0) * 2.0 ** 32)) and t[4] > 0 and t[5] == 0
    assert (np.diff(t.astype(np.int64)) <= 0).all(), "monotone in beta"
    beta = np.linspace(0.0, 12.0, 257)
    assert np.array_equal(at(beta), ao.thresholds(beta))
    assert (np.diff(at(beta).astype(np.int64)) < 0).all()
    assert at(2.0).shape == (1,) and at(np.zeros(0)).shape == (0,)
    for bad in ([-1e-9], [1.0, -2.0], [np.nan], [[1.0, 2.0]], [-np.inf]):
        with pytest.raises(ValueError, match="beta"):
            at(bad)


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
    mod = importlib.import_module("mjx.quench")
    assert mjx_mod.quench_anneal is mod.quench_anneal and mjx_mod.anneal_thresholds is mod.anneal_thresholds
    assert "quench_anneal" in mjx_mod.__all__ and "anneal_thresholds" in mjx_mod.__all__
    import mjx as shim
    assert shim.quench_anneal is mod.quench_anneal


def _caps(lib, n, d, T):
    caps = (ctypes.c_int64 * (T + 1))()
    assert lib.mjx_ell_ball_bound(n, d, T, caps) == 0
    return caps


def test_lds_budget_is_the_jobs_plus_one_bitmap_and_ends_at_64_kib(mjx_mod):
    lib = mjx_mod.load_library()

    def both(n, T, d=4):
        caps = _caps(lib, n, d, T)
        return lib.mjx_quench_jobs_lds(n, T, caps), lib.mjx_quench_anneal_jobs_lds(n, T, caps)

    for n, T in ((10000, 3), (96, 3), (10000, 2), (33, 1), (64, 6), (65, 6), (50, 0)):
        jobs, an = both(n, T)
        assert jobs > 0 and an == (jobs + 4 * 2 * ((n + 63) // 64) + 15) // 16 * 16, (n, T)
    assert both(10000, 3)[1] == (4 * (6 * 2 * 157 + 1 + 5 + 21 + 85 + 85) + 15) // 16 * 16
    # the ceiling: a quench job of n = 1e5 fits, the snapshot on top of it does not; 8e4 fits both
    jobs, an = both(100000, 3)
    assert 0 < jobs <= 64 * 1024 and an == -1
    jobs, an = both(80000, 3)
    assert 0 < jobs < an <= 64 * 1024
    # T = 4..6 are served (no 2T ball), 7 and -1 are not; caps that are none
    c6 = _caps(lib, 10000, 4, 6)
    for T in (4, 5, 6):
        assert lib.mjx_quench_anneal_jobs_lds(10000, T, c6) > 0
    assert lib.mjx_quench_anneal_jobs_lds(10000, 7, c6) == -1 and lib.mjx_quench_anneal_jobs_lds(10000, -1, c6) == -1
    assert lib.mjx_quench_anneal_jobs_lds(10000, 3, None) == -1 and lib.mjx_quench_anneal_jobs_lds(0, 3, c6) == -1
    assert lib.mjx_quench_anneal_jobs_lds(1 << 31, 3, c6) == -1
    assert lib.mjx_quench_anneal_jobs_lds(100, 2, (ctypes.c_int64 * 3)(1, 0, 5)) == -1


def test_compute_entry_points_validate_before_any_pointer_is_read(mjx_mod):
    lib = mjx_mod.load_library()
    EINVAL = 1
    a = ctypes.c_void_p(64)
    n, d, R, K = 1000, 4, 3, 2
    caps = _caps(lib, n, d, 6)
    names = ["adj", "n", "d", "graph_stride", "R", "K", "p", "c", "caps", "sweeps", "thr", "seed", "s_np", "order",
             "order_stride_r", "out_np", "flipped", "plus", "plus_quench", "plus_best", "best_sweep", "moves", "trace",
             "consensus", "flag", "stream"]
    ok = [a, n, d, 0, R, K, 3, 1, caps, 5, a, 7, a, a, 0, a, a, a, a, a, a, a, None, a, a, None]
    assert len(names) == len(ok) == len(mjx_mod._lib.SIGNATURES["mjx_quench_anneal_jobs_ell"])

    def ell(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.mjx_quench_anneal_jobs_ell(*args)

    assert ell(p=7) == EINVAL and ell(p=4, c=4) == EINVAL and ell(p=0, c=0) == EINVAL and ell(p=-1) == EINVAL
    assert ell(sweeps=-1) == EINVAL and ell(sweeps=1 << 31) == EINVAL
    assert ell(thr=None) == EINVAL and ell(thr=None, sweeps=1) == EINVAL
    assert ell(n=1 << 31) == EINVAL and ell(n=0) == EINVAL and ell(R=0) == EINVAL and ell(K=0) == EINVAL
    assert ell(R=1 << 20, K=1 << 20) == EINVAL
    for name in ("adj", "caps", "s_np", "order", "out_np", "flipped", "plus", "plus_quench", "plus_best", "best_sweep",
                 "moves", "consensus", "flag"):
        assert ell(**{name: None}) == EINVAL, name
    assert ell(graph_stride=n) == EINVAL and ell(order_stride_r=n) == EINVAL and ell(d=-1) == EINVAL
    big = _caps(lib, 100000, d, 3)
    assert ell(n=100000, caps=big) == EINVAL                        # does not fit the LDS
    cnames = ["row_ptr", "col"] + [k for k in names[1:] if k not in ("d", "graph_stride")]
    cok = [a, a] + [v for k, v in zip(names[1:], ok[1:]) if k not in ("d", "graph_stride")]
    assert len(cok) == len(mjx_mod._lib.SIGNATURES["mjx_quench_anneal_jobs_csr"])

    def csr(**kw):
        args = list(cok)
        for k, v in kw.items():
            args[cnames.index(k)] = v
        return lib.mjx_quench_anneal_jobs_csr(*args)

    assert csr(row_ptr=None) == EINVAL and csr(p=7) == EINVAL and csr(sweeps=-1) == EINVAL
    assert csr(thr=None) == EINVAL and csr(moves=None) == EINVAL and csr(caps=None) == EINVAL
    assert csr(plus_best=None) == EINVAL and csr(order_stride_r=1) == EINVAL


# ---- host-side refusals ---------------------------------------------------------
def test_refusals_happen_on_the_host(mjx_mod):
    """The same ValueError with and without a GPU: nothing here reaches the device."""
    n = 20
    adj = mjx_mod.random_regular_graph(3, n, seed=0)
    s = np.ones((2, n), np.int64)
    qa = mjx_mod.quench_anneal
    ident = np.arange(n)
    for p, c in ((7, 1), (4, 4), (0, 0), (-1, 3)):
        with pytest.raises(ValueError, match="p \\+ c - 1|p, c >= 0"):
            qa(adj, s, p, c, 4)
    for bad in (-1, 1.5, True, None, 2 ** 31, "4"):
        with pytest.raises(ValueError, match="sweeps"):
            qa(adj, s, 1, 1, bad)
    for bad in ((-1.0, 2.0), (1.0, np.inf), (np.nan, 1.0), (1.0, 2.0, 3.0), np.ones(5), [1.0, -1.0, 1.0, 1.0],
                [1.0, np.nan, 1.0, 1.0], np.ones((2, 2)), 3.0):
        with pytest.raises(ValueError, match="beta"):
            qa(adj, s, 1, 1, 4, beta=bad)
    with pytest.raises(ValueError, match="not both"):
        qa(adj, s, 1, 1, 4, beta=(1.0, 2.0), thresholds=np.zeros(4, np.uint32))
    for bad in (np.zeros(3, np.uint32), np.zeros(4), np.array([0, 0, 0, -1]), np.array([0, 0, 0, 2 ** 32]),
                np.zeros((1, 4), np.uint32)):
        with pytest.raises(ValueError, match="thresholds"):
            qa(adj, s, 1, 1, 4, thresholds=bad)
    for bad in (-1, 2 ** 64, 1.5, True, None):
        with pytest.raises(ValueError, match="anneal_seed"):
            qa(adj, s, 1, 1, 4, anneal_seed=bad)
    # quench_restarts' refusals
    for bad in (np.zeros(n, np.int64), np.arange(n - 1), np.arange(1, n + 1), ident * 1.0,
                np.r_[np.arange(n - 1), n - 2], np.stack([ident, np.zeros(n, np.int64)])[None].repeat(2, 0)):
        K = 1 if np.ndim(bad) == 1 else np.shape(bad)[-2]
        with pytest.raises(ValueError, match="permutation"):
            qa(adj, s, 1, 1, 4, restarts=K, orders=bad)
    with pytest.raises(ValueError, match="not both"):
        qa(adj, s, 1, 1, 4, orders=ident, seed=3)
    with pytest.raises(ValueError, match="restarts = 3"):
        qa(adj, s, 1, 1, 4, restarts=3, orders=np.stack([ident, ident[::-1]]))
    with pytest.raises(ValueError, match="orders or seed"):
        qa(adj, s, 1, 1, 4, restarts=2)
    with pytest.raises(ValueError, match="restarts must be >= 1"):
        qa(adj, s, 1, 1, 4, restarts=0, seed=1)
    with pytest.raises(ValueError, match="packed input"):
        qa(adj, np.zeros(n * 2, np.int64), 1, 1, 4)
    csr = mjx_mod.Graph("csr", n)
    with pytest.raises(ValueError, match="CSR"):
        qa([csr, csr], s, 1, 1, 4)
    with pytest.raises(ValueError, match="3 graphs for 2 starts"):
        qa(np.stack([adj] * 3), s, 1, 1, 4)
    # 1e5 nodes of degree 4 at T = 3: the quench job fits the LDS, the snapshot on top does not
    big = 100_000
    i = np.arange(big)
    lattice = np.stack([(i - 1) % big, (i + 1) % big, (i - 2) % big, (i + 2) % big], axis=1)
    with pytest.raises(ValueError, match="quench_anneal: .* does not fit"):
        qa(lattice, np.ones(big, np.int64), 3, 1, 2)


def test_beta_forms_give_the_documented_thresholds(mjx_mod):
    check = importlib.import_module("mjx.quench")._check_anneal
    at = mjx_mod.anneal_thresholds
    assert np.array_equal(check(5, None, None, 0)[0], at(np.linspace(1.5, 6.0, 5)))
    assert np.array_equal(check(5, (1.0, 3.0), None, 0)[0], at(np.linspace(1.0, 3.0, 5)))
    assert np.array_equal(check(5, [1.0, 3.0], None, 0)[0], at(np.linspace(1.0, 3.0, 5)))
    assert np.array_equal(check(2, (1.0, 3.0), None, 0)[0], at([1.0, 3.0]))
    assert np.array_equal(check(1, (1.0, 3.0), None, 0)[0], at([1.0]))
    assert np.array_equal(check(3, [2.0, np.inf, 0.0], None, 0)[0], np.array([at(2.0)[0], 0, 2 ** 32 - 1], np.uint32))
    thr, seed = check(0, None, None, 2 ** 64 - 1)
    assert thr.shape == (0,) and thr.dtype == np.uint32 and seed == 2 ** 64 - 1
    thr, _ = check(3, None, [0, 5, 2 ** 32 - 1], 0)
    assert thr.dtype == np.uint32 and thr.tolist() == [0, 5, 2 ** 32 - 1]


# ---- CLI ---------------------------------------------------------------------------
def test_cli_parser_knows_anneal():
    cli = importlib.import_module("mjx.cli")
    base = ["quench", "--in", "x.npz", "--p", "3", "--c", "1"]
    jobs = ["--restarts", "2", "--order-seed", "5"]
    a = cli.build_parser().parse_args(base)
    assert a.anneal is None and a.beta is None and a.anneal_seed is None
    a = cli.build_parser().parse_args(base + jobs + ["--anneal", "25"])
    assert a.anneal == 25 and a.beta is None and a.anneal_seed is None and (a.restarts, a.order_seed) == (2, 5)
    a = cli.build_parser().parse_args(base + jobs + ["--anneal", "0", "--beta", "1", "5.5", "--anneal-seed", "9"])
    assert a.anneal == 0 and a.beta == [1.0, 5.5] and a.anneal_seed == 9
    for bad in (["--anneal", "5"], ["--anneal", "5", "--order-seed", "5"], ["--anneal", "5", "--restarts", "2"],
                ["--restarts", "0", "--order-seed", "5", "--anneal", "5"],
                jobs + ["--anneal", "-1"], jobs + ["--anneal", "5", "--exchange"],
                jobs + ["--anneal", "5", "--schedule", "regions"], ["--anneal", "5", "--schedule", "regions"],
                jobs + ["--beta", "1", "5"], jobs + ["--anneal-seed", "3"], jobs + ["--exchange", "--beta", "1", "5"],
                jobs + ["--anneal", "5", "--beta", "1"], jobs + ["--anneal", "5", "--beta", "-1", "5"],
                jobs + ["--anneal", "5", "--beta", "1", "inf"], jobs + ["--anneal", "5", "--anneal-seed", "-1"],
                jobs + ["--anneal", "5", "--anneal-seed", str(2 ** 64)]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)
