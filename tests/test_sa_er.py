"""Simulated annealing on CSR graphs, CPU side: the test oracle
(tests/sa_er_oracle.py) is pinned to the reference-generated SA fixtures, the
C ABI and the Python surface declare the new entry points, and the ``sa-er``
front parses its options.  No GPU is touched."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import sa_er_oracle as ero

NEW_ENTRY_POINTS = (
    "mjx_sa_csr_init", "mjx_sa_csr_init_mt", "mjx_sa_csr_steps", "mjx_sa_csr_ball_bound",
    "mjx_sa_csr_lightcone_scratch_bytes", "mjx_sa_csr_lightcone_lds", "mjx_sa_csr_lightcone_prepare",
    "mjx_sa_csr_lightcone_steps",
)


@pytest.mark.parametrize("name", ["sa_d3_n300_p2c1.npz", "sa_d4_n200_p1c1.npz"])
def test_oracle_on_regular_csr_equals_the_reference_fixtures(name):
    """The CSR restatement of the SA loop, run on the CSR of a fixture's own
    neighbour array, reproduces the fixture's reference-generated traces over
    their full length, and its final state where the fixture ran to consensus."""
    z = load_golden(name)
    N, p, c = z["N"], int(z["p"]), int(z["c"])
    rp, col = ero.csr_of_ell(N)
    for sd in (int(s) for s in z["seeds"]):
        L = len(z[f"seed{sd}_i"])
        o = ero.sa_loop_er(rp, col, p, c, sd, max_steps=L)
        assert len(o["trace"]["i"]) == L
        for key in ("i", "accept", "sum_end", "dE"):
            assert np.array_equal(o["trace"][key], z[f"seed{sd}_{key}"]), (sd, key)
        if L == int(z[f"seed{sd}_num_steps"]):
            assert np.array_equal(o["conf"], z[f"seed{sd}_conf"])
            assert o["mag_reached"] == float(z[f"seed{sd}_mag_reached"])


def test_abi_and_python_surface_declare_sa_on_csr(mjx_mod):
    src = open(os.path.join(ROOT, "include", "mjx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mjx_[a-z0-9_]+)\s*\(", src))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, f"{name} not declared in include/mjx.h"
        assert name in mjx_mod._lib.SIGNATURES, f"{name} has no ctypes prototype"
    assert callable(mjx_mod.SAReplicasER) and callable(mjx_mod.sa_er_run)
    # additions only: the ABI version and the state struct are what they were
    assert mjx_mod.load_library().mjx_abi_version() == 2
    # argument checks that return before any launch (no GPU here)
    lib = mjx_mod.load_library()
    assert lib.mjx_sa_csr_lightcone_lds(0, 0) == -1 and lib.mjx_sa_csr_lightcone_lds(7, 0) == -1
    assert lib.mjx_sa_csr_lightcone_lds(2, 4) == 4 * 4 * 64 * 4
    caps = (mjx_mod._lib.c_i64 * 3)(1, 201, 300)
    assert lib.mjx_sa_csr_lightcone_scratch_bytes(70, 2, caps, 4) == 2 * 64 * 4 * ((201 - 4) + 2 * (300 - 4))
    assert lib.mjx_sa_csr_lightcone_scratch_bytes(70, 2, caps, 512) == -1          # 512 entries x 4 lists: no such LDS
    small = (mjx_mod._lib.c_i64 * 3)(1, 9, 32)
    assert lib.mjx_sa_csr_lightcone_scratch_bytes(70, 2, small, 0) == 0             # every list within the LDS part
    assert lib.mjx_sa_csr_steps(None, None, 10, 1, 1, 64, None, None, None, None, 1, 1.0, 1.0, 1.0, 1.0, 1,
                                None) == mjx_mod._lib.MJX_EINVAL


def test_sa_er_front_parses_its_options(mjx_mod):
    import importlib
    cli = importlib.import_module("mjx.cli")
    ap = cli.build_parser()
    a = vars(ap.parse_args(["sa-er"]))
    for k, v in cli.SA_ER_DEFAULTS.items():
        assert a[k] == v, (k, a[k], v)
    assert a["mode"] == "auto" and a["seed"] == 0 and a["replicas"] is None and not a["keep_isolated"]
    a = ap.parse_args(["sa-er", "--n", "500", "--deg", "3.5", "--p", "2", "--c", "2", "--N_stat", "9", "--mode",
                       "rollout", "--max-steps", "100", "--max-seconds", "2.5", "--keep-isolated", "--graph-seed",
                       "4", "--out", "x.npz"])
    assert (a.cmd, a.n, a.deg, a.p, a.c, a.N_stat, a.mode) == ("sa-er", 500, 3.5, 2, 2, 9, "rollout")
    assert (a.max_steps, a.max_seconds, a.keep_isolated, a.graph_seed, a.out) == (100, 2.5, True, 4, "x.npz")
    with pytest.raises(SystemExit):
        ap.parse_args(["sa-er", "--mode", "tape"])


def test_issue_graphs_have_the_stated_shapes(mjx_mod):
    """The four test graphs are what the GPU tests assume: sizes, degrees,
    isolated nodes, symmetry (every (u, v) entry has its (v, u))."""
    def stats(rp, col):
        n = rp.shape[0] - 1
        deg = np.diff(rp)
        u = np.repeat(np.arange(n), deg)
        sym = np.array_equal(np.sort(u * n + col), np.sort(col.astype(np.int64) * n + u))
        return n, int(deg.max()), int((deg == 0).sum()), sym
    assert stats(*ero.graph_A(mjx_mod)) == (148, 8, 0, True)
    assert stats(*ero.graph_B(mjx_mod)) == (97, 6, 5, True)
    n, dmax, iso, sym = stats(*ero.graph_H(mjx_mod))
    assert (n, dmax, sym) == (300, 200, True)
    rpB, colB = ero.graph_B(mjx_mod)
    rpM, colM = ero.graph_M(mjx_mod)
    assert stats(rpM, colM)[3] and colM.shape[0] == colB.shape[0] + 3 + 6
