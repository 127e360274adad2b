"""Region-parallel quench, CPU side: a numpy model of the distance-2T rule
against the sequential oracle (tests/quench_oracle.py), the new entry points'
ABI and argument checks, the host-side refusals of ``quench`` and the CLI
parser.  No GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import quench_oracle as qo
from conftest import ROOT

NEW_SYMBOLS = ("mjx_quench_regions_scratch_bytes", "mjx_quench_regions_ell_rp", "mjx_quench_regions_csr_rp")


# ---- the rule, in numpy --------------------------------------------------------
def within(rows, i, radius):
    """The nodes within graph distance ``radius`` of i; rows[v] = the row of v."""
    seen, front = {int(i)}, [int(i)]
    for _ in range(radius):
        front = [int(k) for v in front for k in rows[v] if int(k) not in seen and not seen.add(int(k))]
    return seen


def regions_model(step, rows, S, T, order, window):
    """The pass in rounds: of the ``window`` pending candidates of lowest rank,
    those with no pending candidate of lower rank within distance 2T try their
    flip against the state at the START of the round, and what they accept is
    applied together.  -> (conf, flipped, commits of every round)."""
    S = np.asarray(S, dtype=np.int64).copy()
    n = S.shape[1]
    consensus = qo.end_state(step, S, T).sum(axis=1) == n
    removable = qo.flip_gains(step, S, T)["removable"]
    cand = [int(i) for i in order if removable[:, i].any()]
    rank = {i: k for k, i in enumerate(cand)}
    near = [{rank[v] for v in within(rows, i, 2 * T) if v in rank and rank[v] < k} for k, i in enumerate(cand)]
    pending, flipped, commits = list(range(len(cand))), np.zeros(S.shape[0], np.int64), []
    while pending:
        win = set(pending[:window])                 # every pending candidate of lower rank is in the window too
        ready = [k for k in pending[:window] if not (near[k] & win)]
        assert ready and ready[0] == pending[0], "the pending candidate of lowest rank always commits"
        start = S.copy()
        for k in ready:
            i = cand[k]
            try_ = np.flatnonzero(consensus & (start[:, i] == 1))
            Si = start[try_].copy()
            Si[:, i] = -1
            keep = try_[qo.end_state(step, Si, T).sum(axis=1) == n]
            S[keep, i] = -1
            flipped[keep] += 1
        pending = [k for k in pending if k not in set(ready)]
        commits.append(len(ready))
    return S, flipped, commits


def _rrg():
    from mjx import random_regular_graph
    adj = random_regular_graph(3, 200, seed=2)
    return qo.step_ell(adj), list(adj), qo.random_starts(16, 200, 0.8, seed=12), 2


def _er():
    from mjx import erdos_renyi
    rp, col, _ = erdos_renyi(300, 3.0 / 299, seed=6, drop_isolated=True)
    n = rp.shape[0] - 1
    return qo.step_csr(rp, col), [col[rp[v]:rp[v + 1]] for v in range(n)], qo.random_starts(16, n, 0.9, seed=16), 2


def _ring():
    n = 128
    adj = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1)
    return qo.step_ell(adj), list(adj), qo.random_starts(16, n, 0.9, seed=5), 3


@pytest.mark.parametrize("case", [_rrg, _er, _ring], ids=["rrg_d3_n200_T2", "er_n300_T2", "ring_n128_T3"])
def test_the_rule_in_numpy_equals_the_sequential_oracle(case):
    step, rows, S, T = case()
    n = S.shape[1]
    most = 0
    for order in (np.arange(n), np.random.default_rng(3).permutation(n)):
        want = qo.quench(step, S, T, order)
        assert want["consensus"].any() and (~want["consensus"]).any() and want["flipped"].sum() > 0, "degenerate case"
        for window in (1, 8, n):
            conf, flipped, commits = regions_model(step, rows, S, T, order, window)
            assert np.array_equal(conf, want["conf"]) and np.array_equal(flipped, want["flipped"]), window
            if window == 1:
                assert max(commits) == 1
            most = max(most, max(commits))
    assert most >= 2, "no round applied two candidates: the case does not test the rule"


def test_within_is_a_ball():
    ring = [((v - 1) % 10, (v + 1) % 10) for v in range(10)]
    assert within(ring, 0, 0) == {0} and within(ring, 0, 2) == {8, 9, 0, 1, 2} and len(within(ring, 3, 7)) == 10


# ---- ABI ---------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "distance > 2T" in src and "distance l+2" in src, "the distance rule belongs to the contract"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(mjx_mod.load_library(), name)


def test_scratch_bytes_and_argument_checks_without_gpu(mjx_mod):
    lib = mjx_mod.load_library()
    EINVAL = 1
    caps = (ctypes.c_int64 * 7)()
    assert lib.mjx_ell_ball_bound(1000, 4, 3, caps) == 0 and list(caps)[:4] == [1, 5, 21, 85]
    size = lib.mjx_quench_regions_scratch_bytes
    head = (1 + 65 * 2) * 8
    # every list in LDS: header, 8 n of claims, 8 of the ready count, 4 (3 + caps[T]) per slot
    assert size(1000, 128, 2, caps, 0, 1) == head + 8000 + 8 + 8 * ((4 * 24 + 7) // 8)
    assert size(1000, 128, 2, caps, 0, 10) == head + 8000 + 8 + 4 * 10 * (3 + 21)
    # lds_entries = 4: a list part per workgroup of the commit grid, min(window * W, 8192)
    per = ((1 + 17 + 81) * 12 + 81 * 4 + 7) // 8 * 8
    slots = lambda k: 8000 + 8 + (4 * k * 88 + 7) // 8 * 8
    assert size(1000, 128, 3, caps, 4, 1) == head + 2 * per + slots(1)
    assert size(1000, 128, 3, caps, 4, 7) == head + 14 * per + slots(7)
    assert size(1000, 128, 3, caps, 4, 5000) == head + 8192 * per + slots(5000)
    assert size(1000, 128, 3, caps, 4, 6000) - size(1000, 128, 3, caps, 4, 5000) == 4 * 1000 * 88
    for bad in ((0, 128, 3, caps, 0, 4), (1000, 0, 3, caps, 0, 4), (1000, 128, 7, caps, 0, 4),
                (1000, 128, -1, caps, 0, 4), (1000, 128, 3, None, 0, 4), (1000, 128, 3, caps, -1, 4),
                (1000, 128, 3, caps, 0, 0), (1000, 128, 3, caps, 0, -3), (1 << 31, 128, 3, caps, 0, 4)):
        assert size(*bad) == -1, bad
    # compute entry points: validation fails before any pointer is read
    a = ctypes.c_void_p(64)
    lv = (ctypes.c_void_p * 8)(*[64] * 8)
    #     adj n     d  R    p  c  lv  caps lds scr  bytes   win rem cand ncand cons flip stats r0 rounds stream
    ok = (a, 1000, 4, 128, 3, 1, lv, caps, 0, a, 1 << 30, 8, a, a, 10, a, a, a, 0, 4, None)
    ell = lib.mjx_quench_regions_ell_rp

    def but(k, v):
        return ok[:k] + (v,) + ok[k + 1:]

    assert ell(*but(4, 7)) == EINVAL                       # T = 7
    assert ell(*(ok[:4] + (4, 4) + ok[6:])) == EINVAL      # T = 7 again
    assert ell(*but(1, 1 << 31)) == EINVAL                 # n >= 2^31
    assert ell(*but(11, 0)) == EINVAL                      # window < 1
    assert ell(*but(10, 8)) == EINVAL                      # scratch too small
    assert ell(*but(10, size(1000, 128, 3, caps, 0, 8) - 8)) == EINVAL
    for k in (0, 6, 7, 9, 12, 13, 15, 16, 17):             # a NULL required pointer
        assert ell(*but(k, None)) == EINVAL, k
    assert ell(*but(14, -1)) == EINVAL and ell(*but(14, 1001)) == EINVAL      # ncand outside 0..n
    assert ell(*but(18, -1)) == EINVAL and ell(*but(19, -1)) == EINVAL        # round0, rounds
    csr = lib.mjx_quench_regions_csr_rp
    okc = (a, a) + ok[1:2] + ok[3:]
    assert csr(*((None,) + okc[1:])) == EINVAL
    assert csr(*(okc[:11] + (0,) + okc[12:])) == EINVAL    # window < 1


# ---- Python surface ------------------------------------------------------------
def test_quench_refuses_schedule_and_window_on_the_host(mjx_mod):
    """Before any device call: the same ValueError with and without a GPU."""
    adj = mjx_mod.random_regular_graph(3, 20, seed=0)
    s = np.ones((2, 20), np.int64)
    with pytest.raises(ValueError, match="unknown schedule"):
        mjx_mod.quench(adj, s, 1, 1, schedule="parallel")
    for bad in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match="window must be"):
            mjx_mod.quench(adj, s, 1, 1, schedule="regions", window=bad)
    with pytest.raises(ValueError, match="window belongs to"):
        mjx_mod.quench(adj, s, 1, 1, window=8)
    with pytest.raises(ValueError, match="window belongs to"):
        mjx_mod.quench(adj, s, 1, 1, schedule="sequential", window=8)
    with pytest.raises(ValueError, match="p \\+ c - 1"):
        mjx_mod.quench(adj, s, 7, 1, schedule="regions")
    with pytest.raises(ValueError, match="permutation"):
        mjx_mod.quench(adj, s, 1, 1, schedule="regions", order=np.zeros(20, np.int64))


def test_default_window_rule(mjx_mod):
    q = importlib.import_module("mjx.quench")
    assert q.default_window(10, 1000) == q.WINDOW_BALLS                # the 2T-ball is the graph
    assert q.default_window(10 ** 6, 85) == q.WINDOW_BALLS * 10 ** 6 // (85 * 85)
    assert q.default_window(10 ** 9, 2) == q.WINDOW_MAX
    assert q.default_window(1, 1) >= 1


def test_cli_parser_accepts_schedule_and_window():
    cli = importlib.import_module("mjx.cli")
    base = ["quench", "--in", "x.npz", "--p", "3", "--c", "1"]
    a = cli.build_parser().parse_args(base)
    assert (a.schedule, a.window) == ("sequential", None)
    a = cli.build_parser().parse_args(base + ["--schedule", "regions"])
    assert (a.schedule, a.window) == ("regions", None)
    a = cli.build_parser().parse_args(base + ["--schedule", "regions", "--window", "64", "--order-seed", "5"])
    assert (a.schedule, a.window, a.order_seed) == ("regions", 64, 5)
    for bad in (["--schedule", "balls"], ["--window", "8"], ["--schedule", "regions", "--window", "0"],
                ["--schedule", "regions", "--restarts", "2", "--order-seed", "1"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)
