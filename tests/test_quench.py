"""Flip-gain / quench layer, CPU side: the monotonicity fact on the numpy
oracle (tests/quench_oracle.py), the new entry points' ABI and argument
checks, the host-side checks of ``quench`` and the CLI parser.  No GPU."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import quench_oracle as qo
from conftest import ROOT

NEW_SYMBOLS = ("mjx_ell_ball_bound", "mjx_quench_lds", "mjx_flip_gain_scratch_bytes", "mjx_quench_scratch_bytes",
               "mjx_flip_gain_ell_rp", "mjx_flip_gain_csr_rp", "mjx_quench_ell_rp", "mjx_quench_csr_rp")


def _rrg():
    from mjx import random_regular_graph
    adj = random_regular_graph(3, 60, seed=4)
    return qo.step_ell(adj), qo.random_starts(24, 60, 0.8, seed=1), 2


def _er():
    from mjx import erdos_renyi
    rp, col, _ = erdos_renyi(70, 3.0 / 69, seed=2, drop_isolated=True)
    return qo.step_csr(rp, col), qo.random_starts(24, rp.shape[0] - 1, 0.9, seed=2), 2


# ---- the monotonicity fact, on the oracle -----------------------------------
@pytest.mark.parametrize("case", [_rrg, _er], ids=["rrg", "er"])
def test_one_pass_ends_in_a_local_minimum(case):
    step, S, T = case()
    n = S.shape[1]
    before = qo.flip_gains(step, S, T)
    cons = before["consensus"]
    assert cons.any() and (~cons).any() and before["removable"].any(), "degenerate case"
    for order in (None, np.random.default_rng(3).permutation(n)):
        q = qo.quench(step, S, T, order)
        after = qo.flip_gains(step, q["conf"], T)
        # consequence 2: nothing is removable any more, consensus is kept
        assert not after["removable"].any()
        assert np.array_equal(after["consensus"], cons)
        # consequence 3: every flipped node was removable at the start
        assert not (q["turned"] & ~before["removable"]).any()
        assert q["flipped"][cons].sum() > 0 and not q["flipped"][~cons].any()
        assert np.array_equal(q["conf"][~cons], S[~cons])
        # a second pass flips nothing
        again = qo.quench(step, q["conf"], T, order)
        assert not again["flipped"].any() and np.array_equal(again["conf"], q["conf"])
        # the rule is monotone: a state below the start never ends above it
        assert np.all(qo.end_state(step, q["conf"], T) <= qo.end_state(step, S, T))


def test_oracle_gain_on_a_hand_case():
    # a 4-cycle, all +1, T = 1: flipping one spin changes nothing at the neighbours
    # (1 of 2 neighbours down: a tie keeps +1) and the flipped node returns to +1
    adj = np.array([[1, 3], [0, 2], [1, 3], [0, 2]])
    fg = qo.flip_gains(qo.step_ell(adj), np.ones((1, 4), np.int64), 1)
    assert fg["gain"].tolist() == [[0, 0, 0, 0]] and fg["removable"].all() and fg["consensus"].all()
    fg0 = qo.flip_gains(qo.step_ell(adj), np.array([[1, -1, 1, 1]]), 0)
    assert fg0["gain"].tolist() == [[-2, 2, -2, -2]] and not fg0["removable"].any()


# ---- ABI ---------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    assert "non-decreasing in every input" in src, "the monotonicity fact belongs to the contract"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes signature"
    assert mjx_mod.load_library().mjx_abi_version() == 2


def test_size_queries_and_argument_checks_without_gpu(mjx_mod):
    lib = mjx_mod.load_library()
    EINVAL = 1
    caps = (ctypes.c_int64 * 7)()
    assert lib.mjx_ell_ball_bound(1000, 4, 3, caps) == 0 and list(caps)[:4] == [1, 5, 21, 85]
    assert lib.mjx_ell_ball_bound(50, 4, 6, caps) == 0 and list(caps) == [1, 5, 21, 50, 50, 50, 50]
    assert lib.mjx_ell_ball_bound(50, 4, 7, caps) == EINVAL
    assert lib.mjx_ell_ball_bound(1000, 4, 3, caps) == 0
    # LDS: 12 bytes per entry of the T + 1 change lists, 4 per candidate
    assert lib.mjx_quench_lds(3, 0) == 64 * (4 * 12 + 4)
    assert lib.mjx_quench_lds(3, 4) == 4 * (4 * 12 + 4)
    assert lib.mjx_quench_lds(7, 0) == -1 and lib.mjx_quench_lds(-1, 0) == -1 and lib.mjx_quench_lds(3, -1) == -1
    assert lib.mjx_quench_lds(6, 100000) == -1
    # scratch: the header alone when every list fits LDS, more when it does not
    head = (1 + 65 * 2) * 8
    assert lib.mjx_flip_gain_scratch_bytes(1000, 128, 3, caps, 0) == head + 2000 * (((85 - 64) * 12 + (85 - 64) * 4 + 7) // 8) * 8
    assert lib.mjx_quench_scratch_bytes(128, 2, caps, 0) == head
    per = ((1 + 17 + 81) * 12 + 81 * 4 + 7) // 8 * 8          # lds_entries = 4: caps 5, 21, 85 lose 4 each
    assert lib.mjx_quench_scratch_bytes(128, 3, caps, 4) == head + 2 * per
    assert lib.mjx_quench_scratch_bytes(128, 7, caps, 0) == -1
    assert lib.mjx_flip_gain_scratch_bytes(0, 128, 3, caps, 0) == -1
    # compute entry points: validation fails before any pointer is read
    a = ctypes.c_void_p(64)
    lv = (ctypes.c_void_p * 8)(*[64] * 8)
    ok = (a, 1000, 4, 128, 3, 1, lv, caps, 0, a, 1 << 30, a, a, None, None)
    bad_T = ok[:4] + (7, 1) + ok[6:]
    assert lib.mjx_flip_gain_ell_rp(*bad_T) == EINVAL
    assert lib.mjx_flip_gain_ell_rp(*(ok[:1] + (1 << 31,) + ok[2:])) == EINVAL          # n >= 2^31
    assert lib.mjx_flip_gain_ell_rp(*(ok[:6] + (None,) + ok[7:])) == EINVAL             # no levels
    assert lib.mjx_flip_gain_ell_rp(*(ok[:11] + (None,) + ok[12:])) == EINVAL           # no removable
    assert lib.mjx_flip_gain_ell_rp(*(ok[:10] + (8,) + ok[11:])) == EINVAL              # scratch too small
    assert lib.mjx_flip_gain_csr_rp(None, a, 1000, 128, 3, 1, lv, caps, 0, a, 1 << 30, a, a, None, None) == EINVAL
    assert lib.mjx_quench_ell_rp(a, 1000, 4, 128, 4, 4, lv, caps, 0, a, 1 << 30, a, a, a, a, None) == EINVAL
    assert lib.mjx_quench_ell_rp(a, 1000, 4, 128, 3, 1, lv, caps, 0, a, 1 << 30, a, None, a, a, None) == EINVAL
    assert lib.mjx_quench_csr_rp(a, a, 1000, 128, 3, 1, lv, None, 0, a, 1 << 30, a, a, a, a, None) == EINVAL


# ---- Python surface ------------------------------------------------------------
def test_package_exports_the_new_functions(mjx_mod):
    mod = importlib.import_module("mjx.quench")
    assert mjx_mod.quench is mod.quench and mjx_mod.flip_gains is mod.flip_gains
    assert "quench" in mjx_mod.__all__ and "flip_gains" in mjx_mod.__all__


def test_quench_checks_order_on_the_host(mjx_mod):
    """A bad order is refused before any device call: the same ValueError with
    and without a GPU."""
    adj = mjx_mod.random_regular_graph(3, 20, seed=0)
    s = np.ones((2, 20), np.int64)
    for bad in (np.zeros(20, np.int64), np.arange(19), np.arange(1, 21), np.arange(20) * 1.0,
                np.r_[np.arange(19), 18], np.arange(40).reshape(2, 20)):
        with pytest.raises(ValueError, match="permutation"):
            mjx_mod.quench(adj, s, 1, 1, order=bad)
    with pytest.raises(ValueError, match="not both"):
        mjx_mod.quench(adj, s, 1, 1, order=np.arange(20), seed=3)
    with pytest.raises(ValueError, match="p \\+ c - 1"):
        mjx_mod.quench(adj, s, 7, 1)
    with pytest.raises(ValueError, match="p \\+ c - 1"):
        mjx_mod.flip_gains(adj, s, 0, 0)
    with pytest.raises(ValueError, match="unknown kernel options"):
        mjx_mod.flip_gains(adj, s, 1, 1, kernel={"split": 2})


def test_cli_parser_accepts_quench():
    cli = importlib.import_module("mjx.cli")
    a = cli.build_parser().parse_args(["quench", "--in", "x.npz", "--p", "3", "--c", "1", "--order-seed", "5"])
    assert (a.cmd, a.inp, a.p, a.c, a.order_seed, a.out) == ("quench", "x.npz", 3, 1, 5, None)
    a = cli.build_parser().parse_args(["quench", "--in", "x.npz", "--p", "1", "--c", "1", "--out", "y.npz"])
    assert a.order_seed is None and a.out == "y.npz"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["quench", "--p", "1", "--c", "1"])
