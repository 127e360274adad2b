"""Run-to-attractor layer, CPU side: the numpy oracle (tests/attractor_oracle.py)
on hand cases, its Philox against the C checker, the spin rule at the ends of
the probability range, and the new entry points' ABI.  No GPU."""
import os
import re

import numpy as np

import attractor_oracle as ao
from conftest import ROOT
from oracle import fast

NEW_SYMBOLS = ("mjx_sweep_track_ell_rp", "mjx_sweep_track_csr_rp", "mjx_attractor_record", "mjx_random_spins_rp")


# ---- hand cases for the oracle ---------------------------------------------
def test_perfect_matching_with_opposite_spins_is_a_two_cycle():
    n = 10
    adj = (np.arange(n) ^ 1).reshape(n, 1)               # edges (0,1), (2,3), ...
    s0 = np.where(np.arange(n) % 2 == 0, 1, -1)[None, :]
    r = ao.attractor(ao.step_ell(adj), s0, t_max=8)
    assert r["p"].tolist() == [0] and r["c"].tolist() == [2]
    assert r["sum_att"].tolist() == [[0, 0]]


def test_all_plus_is_a_fixed_point():
    from mjx import random_regular_graph
    n = 50
    adj = random_regular_graph(3, n, seed=1)
    r = ao.attractor(ao.step_ell(adj), np.ones((1, n), np.int64), t_max=8)
    assert r["p"].tolist() == [0] and r["c"].tolist() == [1]
    assert r["sum_att"].tolist() == [[n, n]]


def test_one_step_from_a_fixed_point_has_p_one():
    from mjx import random_regular_graph
    n = 50
    adj = random_regular_graph(3, n, seed=1)
    s0 = np.ones((1, n), np.int64)
    s0[0, 7] = -1                                        # its three neighbours are +1: flips back at once
    r = ao.attractor(ao.step_ell(adj), s0, t_max=8)
    assert r["p"].tolist() == [1] and r["c"].tolist() == [1]
    assert r["sum_att"].tolist() == [[n, n]]


def test_budget_truncates_and_chunks_do_not_matter():
    from mjx import random_regular_graph
    n = 400
    adj = random_regular_graph(4, n, seed=3)
    S0 = 2 * np.random.default_rng(0).integers(0, 2, (32, n)) - 1
    full = ao.attractor(ao.step_ell(adj), S0, t_max=256, chunk=16)
    assert np.all(full["p"] >= 0) and full["p"].max() >= 3
    for chunk in (1, 2, 7):
        other = ao.attractor(ao.step_ell(adj), S0, t_max=256, chunk=chunk)
        for key in ("p", "c", "sum_att"):
            assert np.array_equal(full[key], other[key])
    cut = int(full["p"].max()) - 1
    short = ao.attractor(ao.step_ell(adj), S0, t_max=cut, chunk=16)
    late = full["p"] > cut
    assert late.any() and np.all(short["p"][late] == -1) and np.all(short["c"][late] == 0)
    assert np.array_equal(short["p"][~late], full["p"][~late])
    assert np.array_equal(short["sum_att"][~late], full["sum_att"][~late])
    assert short["t_end"] == cut + 2
    # the definition, replica by replica: s(p+2) = s(p) and p is the first such t
    step = ao.step_ell(adj)
    traj = [S0]
    for _ in range(int(full["p"].max()) + 2):
        traj.append(step(traj[-1]))
    for r in range(S0.shape[0]):
        p = int(full["p"][r])
        assert np.array_equal(traj[p + 2][r], traj[p][r])
        assert all(not np.array_equal(traj[t + 2][r], traj[t][r]) for t in range(p))
        assert full["c"][r] == (1 if np.array_equal(traj[p + 1][r], traj[p][r]) else 2)


# ---- Philox and the spin rule ----------------------------------------------
def test_numpy_philox_equals_the_c_checker():
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, size=(4, 200), dtype=np.uint64).astype(np.uint32)
    ctr[:, 0] = 0
    ctr[:, 1] = 0xFFFFFFFF
    for key in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0xA4093822, 0x299F31D0), (12345, 0)):
        got = ao.philox4x32_10(tuple(ctr), key)
        for i in range(ctr.shape[1]):
            want = fast.philox4x32_10(ctr[:, i], key)
            assert [int(g[i]) for g in got] == [int(x) for x in want]


def test_spin_rule_at_the_ends_of_the_range():
    S = ao.random_spins(300, 6, [0.0, 1.0, 0.0, 1.0, 0.5, 0.37], seed=9)
    assert np.all(S[[0, 2]] == -1) and np.all(S[[1, 3]] == 1)
    for r, pr in ((4, 0.5), (5, 0.37)):                  # 300 Bernoulli draws, 6 sigma
        assert abs((S[r] == 1).mean() - pr) < 6 * np.sqrt(pr * (1 - pr) / 300)
    # a pure function of (seed, v, r): the same replica whatever R is
    assert np.array_equal(ao.random_spins(300, 5, [0.0, 1.0, 0.0, 1.0, 0.5], seed=9), S[:5])
    assert not np.array_equal(ao.random_spins(300, 6, [0.0, 1.0, 0.0, 1.0, 0.5, 0.37], seed=10)[4], S[4])


# ---- ABI -------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
    lib = mjx_mod.load_library()
    assert lib.mjx_abi_version() == 2
    EINVAL = 1
    # argument validation only (no device call): aliasing and null pointers
    import ctypes
    a, b = ctypes.c_void_p(64), ctypes.c_void_p(128)
    assert lib.mjx_sweep_track_ell_rp(a, 10, 4, 1, b, None, b, None, a, None) == EINVAL      # s_out == s_in
    assert lib.mjx_sweep_track_ell_rp(a, 10, 4, 1, b, b, a, None, a, None) == EINVAL         # s_prev == s_in
    assert lib.mjx_sweep_track_ell_rp(a, 10, 4, 1, b, None, a, None, None, None) == EINVAL   # no diff
    assert lib.mjx_sweep_track_csr_rp(None, a, None, 10, 1, b, None, a, None, a, None) == EINVAL
    assert lib.mjx_attractor_record(10, 64, 1, a, a, a, a, a, a, a, a, None) == EINVAL       # k < 2
    assert lib.mjx_random_spins_rp(10, 0, 1, a, a, None) == EINVAL
    for name in ("attractor", "random_spins", "consensus_curve"):
        assert callable(getattr(mjx_mod, name))
