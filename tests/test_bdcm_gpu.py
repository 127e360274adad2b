"""GPU parity of the BDCM kernels (rows a12-a13 of SURVEY.md 8a).

Bar: one BDCM_ER sweep (and the leaf reset), Zi, Zij, phi and m_init from
identical float64 inputs within 1e-12 of the notebook's own values
(tests/golden/bdcm_er_*.npz, produced by the reference functions); the whole
lambda procedure with the same iteration counts and m_init, ent1, ent within
1e-5 relative (north star), which in float64 it meets by ~1e-10.
"""
import glob
import os

import numpy as np
import pytest
import torch

from bdcm_cases import entry_err
from conftest import GOLDEN, load_golden
from oracle import bdcm as orc

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "bdcm_er_*.npz")))


def plan_of(mjx_mod, z):
    return mjx_mod.BDCMPlan(z["edges"], z["row_ptr"], z["col"], n_total=int(z["n"]), n_iso=int(z["n_iso"]))


def rowrel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.max(np.abs(ref), axis=1, keepdims=True)))


def dev(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", CASES)
def test_bdcm_sweep_and_observables_vs_reference(mjx_mod, name):
    z = load_golden(name)
    p, c, lm, damp = int(z["p"]), int(z["c"]), float(z["sweep_lmbd"]), float(z["damppar"])
    av, epsilon = int(z["attr_value"]), float(z["epsilon"])
    plan = plan_of(mjx_mod, z)
    chi = dev(z["chi0"])
    mjx_mod.bdcm_leaf_reset(chi, plan, p, c, av, lm)
    assert rowrel(chi.cpu().numpy(), z["sweep_leaf"]) < 1e-14
    assert entry_err(chi.cpu().numpy(), z["sweep_leaf"]) <= 1e-12
    chi = dev(z["sweep_leaf"])
    out = mjx_mod.BDCM_ER(chi, plan, p, c, av, lm, damp, epsilon)
    assert out is chi                                   # in place, like nb:196-198
    assert rowrel(chi.cpu().numpy(), z["sweep_chi"]) < 1e-12
    assert entry_err(chi.cpu().numpy(), z["sweep_chi"]) <= 1e-12
    ref = dev(z["sweep_chi"])
    np.testing.assert_allclose(mjx_mod.Zi_ER(ref, plan, p, c, av, lm, epsilon).cpu().numpy(), z["sweep_zi"],
                               rtol=1e-12, atol=0)
    np.testing.assert_allclose(mjx_mod.Zij(ref, plan, p, c, av, epsilon).cpu().numpy(), z["sweep_zij"],
                               rtol=1e-12, atol=0)
    assert abs(mjx_mod.phi_BP_GENERAL_ER(ref, plan, p, c, av, lm, epsilon) - float(z["sweep_phi"])) < 1e-12
    assert abs(mjx_mod.avg_m_init_GENERAL_ER(ref, plan, p, c, av, epsilon) - float(z["sweep_m_init"])) < 1e-12


@pytest.mark.parametrize("name", CASES)
def test_bdcm_entropy_procedure_vs_reference(mjx_mod, name):
    z = load_golden(name)
    p, c = int(z["p"]), int(z["c"])
    plan = plan_of(mjx_mod, z)
    chi = dev(z["chi0"])
    res = mjx_mod.BDCM_entropy_procedure_GENERAL_ER(chi, plan, z["lambdas"], T_max=int(z["T_max"]), p=p, c=c,
                                                    attr_value=int(z["attr_value"]), eps=float(z["eps"]),
                                                    damppar=float(z["damppar"]), epsilon=float(z["epsilon"]))
    L = len(z["iters"])
    assert np.array_equal(res["iters"][:L], z["iters"])
    for k in ("m_init", "ent1", "ent"):
        np.testing.assert_allclose(res[k], z[k], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(res[k], z[k], rtol=1e-9, atol=1e-12)
    assert res["counts"] == z["counts"]
    assert rowrel(chi.cpu().numpy(), z["chi_final"]) < 1e-9
    assert entry_err(chi.cpu().numpy(), z["chi_final"]) <= 1e-9


@pytest.mark.parametrize("p,c,deg", [(1, 1, 5.0), (2, 1, 3.0), (1, 2, 3.0), (2, 2, 2.0), (3, 1, 2.0),
                                     (2, 1, 5.0), (1, 2, 5.0), (2, 2, 5.0)])
def test_bdcm_random_graph_vs_oracle(mjx_mod, p, c, deg):
    """Own ER graphs (hubs up to degree ~14, leaves, all T <= 4) against the
    oracle: one leaf reset + sweep, Zi, Zij, phi, m_init.  No seed re-rolling:
    classes whose count table exceeds the LDS budget (T = 4 beyond 6 incoming
    messages, T = 3 beyond 16, T = 2 beyond 99) run from the global scratch slab."""
    n = 2000 if p + c <= 3 else (500 if deg < 5 else 200)     # the oracle's T = 4 tables grow as (D+1)^4
    plan = mjx_mod.bdcm_er_plan(n, deg / (n - 1), seed=7 * p + c)
    lib = mjx_mod.load_library()
    if deg == 5.0 and p + c == 4:
        assert any(lib.mjx_bdcm_scratch_bytes(D, p, c) > 0 for D in plan.classes), "no class beyond LDS"
    hp = orc.Plan.from_csr(plan.edges_host, plan.row_ptr_host, plan.col_host, plan.n, plan.n_iso)
    rng = np.random.default_rng(p + 10 * c)
    nc = 4 ** (p + c)
    chi0 = rng.random((2 * plan.E, nc))
    chi0 /= chi0.sum(axis=1, keepdims=True)
    lm = 0.7
    want = chi0.copy()
    if 0 in hp.class_rows:
        want[hp.class_rows[0]] = orc.leaf_message(p, c, 1, lm)[None, :]
    want = orc.BDCM_ER(want, hp, p, c, 1, lm, 0.1)
    chi = dev(chi0)
    mjx_mod.bdcm_leaf_reset(chi, plan, p, c, 1, lm)
    mjx_mod.BDCM_ER(chi, plan, p, c, 1, lm, 0.1)
    assert rowrel(chi.cpu().numpy(), want) < 1e-12
    np.testing.assert_allclose(mjx_mod.Zi_ER(chi, plan, p, c, 1, lm).cpu().numpy(),
                               orc.Zi_ER(want, hp, p, c, 1, lm), rtol=1e-11)
    np.testing.assert_allclose(mjx_mod.Zij(chi, plan, p, c, 1).cpu().numpy(), orc.Zij(want, hp, p, c, 1), rtol=1e-12)
    assert abs(mjx_mod.phi_BP_GENERAL_ER(chi, plan, p, c, 1, lm) - orc.phi_BP(want, hp, p, c, 1, lm)) < 1e-10
    assert abs(mjx_mod.avg_m_init_GENERAL_ER(chi, plan, p, c, 1) - orc.avg_m_init(want, hp, p, c, 1)) < 1e-12


def test_bdcm_reproduces_notebook_stdout_statistically(mjx_mod):
    """The notebook's recorded run (ER mean degree 1.0, n=1000, p=c=1, nb:15-37:
    m_init 0.7860 / ent1 0.1721 at lambda=0, 0.7138 / 0.1549 at 0.5) is
    unseeded, so it is a statistical anchor: three own graphs must scatter
    around it as the reference's re-runs did."""
    m0, e0, m5, e5 = [], [], [], []
    for s in range(3):
        plan = mjx_mod.bdcm_er_plan(1000, 1.0 / 999, seed=100 + s)
        rng = np.random.default_rng(s)
        chi = rng.random((2 * plan.E, 16))
        chi = dev(chi / chi.sum(axis=1, keepdims=True))
        r = mjx_mod.BDCM_entropy_procedure_GENERAL_ER(chi, plan, [0.0, 0.5])
        assert r["counts"] == 0 and np.all(r["iters"] < 1300)
        m0.append(r["m_init"][0]); e0.append(r["ent1"][0]); m5.append(r["m_init"][1]); e5.append(r["ent1"][1])
    assert abs(np.mean(m0) - 0.786) < 0.015 and abs(np.mean(e0) - 0.172) < 0.01
    assert abs(np.mean(m5) - 0.714) < 0.015 and abs(np.mean(e5) - 0.155) < 0.01


def test_bdcm_rejects_unsupported_trajectories(mjx_mod):
    z = load_golden(CASES[0])
    plan = plan_of(mjx_mod, z)
    chi = torch.ones((2 * plan.E, 4 ** 5), dtype=torch.float64, device="cuda")
    with pytest.raises(mjx_mod.MjxError):
        mjx_mod.BDCM_entropy_procedure_GENERAL_ER(chi, plan, [0.0], p=4, c=1)


@pytest.mark.parametrize("graph", [True, False])
def test_bdcm_device_loop_equals_host_loop(mjx_mod, graph):
    """The convergence loop with the device stop flag (captured batches, one
    host read per batch) stops at the same sweep as the reference's
    while(delta > eps) (nb:422-431) and leaves chi bit-identical: the sweeps
    of a batch past the stop are no-ops."""
    z = load_golden(CASES[0])
    p, c, damp = int(z["p"]), int(z["c"]), float(z["damppar"])
    plan = plan_of(mjx_mod, z)
    eps = float(z["eps"])
    for lm, batch in ((0.0, 32), (0.5, 7)):
        a = dev(z["chi0"])
        b = dev(z["chi0"])
        mjx_mod.bdcm_leaf_reset(a, plan, p, c, 1, lm)
        mjx_mod.bdcm_leaf_reset(b, plan, p, c, 1, lm)
        t_dev, d_dev = mjx_mod.bdcm_converge(a, plan, p, c, 1, lm, damp, eps, 1300, batch=batch, graph=graph)
        delta, t = 1.0, 0
        dbits = plan._delta
        while delta > eps:
            dbits.zero_()
            mjx_mod.BDCM_ER(b, plan, p, c, 1, lm, damp, delta=dbits)
            delta = float(dbits.view(torch.float64).item())
            t += 1
        assert t_dev == t and d_dev == delta
        assert torch.equal(a, b)


def test_bdcm_device_loop_stops_at_t_max(mjx_mod):
    """eps = 0 never converges: the device loop stops after exactly T_max
    sweeps (the reference's counts = lambda branch) even inside a batch."""
    z = load_golden(CASES[0])
    p, c, damp = int(z["p"]), int(z["c"]), float(z["damppar"])
    plan = plan_of(mjx_mod, z)
    a = dev(z["chi0"])
    b = dev(z["chi0"])
    t, _ = mjx_mod.bdcm_converge(a, plan, p, c, 1, 0.3, damp, 0.0, 11, batch=8)
    for _ in range(11):
        mjx_mod.BDCM_ER(b, plan, p, c, 1, 0.3, damp)
    assert t == 11 and torch.equal(a, b)
    res = mjx_mod.BDCM_entropy_procedure_GENERAL_ER(dev(z["chi0"]), plan, [0.0, 0.5], T_max=5, p=p, c=c, eps=0.0,
                                                    damppar=damp)
    host = mjx_mod.BDCM_entropy_procedure_GENERAL_ER(dev(z["chi0"]), plan, [0.0, 0.5], T_max=5, p=p, c=c, eps=0.0,
                                                     damppar=damp, device_loop=False)
    # lambda = 0 sets counts = 0 (no stop), lambda = 0.5 sets counts = 0.5 and stops (nb:428-452)
    assert res["counts"] == host["counts"] == 0.5 and list(res["iters"]) == list(host["iters"]) == [5, 5]
    for k in ("m_init", "ent1", "ent"):
        assert np.array_equal(res[k], host[k])


def test_captured_loop_survives_buffer_reallocation(mjx_mod):
    """A captured convergence loop bakes in the plan's update buffer and
    scratch slab: converge at p=c=1, a sweep at p+c=3 (the update buffer
    grows, a new scratch slab for the hub's class), converge at p=c=1 again
    -- the second loop must not replay the first capture into freed memory
    (ADVICE r02): it equals the host loop."""
    rng = np.random.default_rng(3)
    n = 120
    u, v = mjx_mod.erdos_renyi_edges(n, 3.0 / (n - 1), seed=4)
    hub_nb = rng.choice(np.arange(1, n), size=14, replace=False)        # degree >= 14: scratch slab at T=3
    pairs = set(zip(u.tolist(), v.tolist())) | {(min(0, int(k)), max(0, int(k))) for k in hub_nb}
    pairs = sorted((a, b) for a, b in pairs if a != b)
    u, v = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    n2, u2, v2, iso = mjx_mod.remove_isolated(n, u, v)
    rp, col = mjx_mod.csr_from_edges(n2, u2, v2)
    plan = mjx_mod.BDCMPlan(np.stack([u2, v2], axis=1), rp, col, n_total=n, n_iso=iso)
    assert max(plan.classes) >= 13
    assert mjx_mod.load_library().mjx_bdcm_scratch_bytes(max(plan.classes), 2, 1) > 0

    def chi0(nc):
        x = rng.random((2 * plan.E, nc))
        return x / x.sum(axis=1, keepdims=True)

    lm, damp, eps = 0.4, 0.1, 1e-9
    x16, x64 = chi0(16), chi0(64)
    a = dev(x16)
    mjx_mod.bdcm_converge(a, plan, 1, 1, 1, lm, damp, eps, 40, batch=8, graph=True)
    b64 = dev(x64)
    mjx_mod.BDCM_ER(b64, plan, 2, 1, 1, lm, damp)
    a2, b2 = dev(x16), dev(x16)
    t_dev, _ = mjx_mod.bdcm_converge(a2, plan, 1, 1, 1, lm, damp, eps, 40, batch=8, graph=True)
    t = 0
    while t < t_dev:
        mjx_mod.BDCM_ER(b2, plan, 1, 1, 1, lm, damp)
        t += 1
    assert torch.equal(a2, b2)
    want = orc.BDCM_ER(x64, orc.Plan.from_csr(plan.edges_host, plan.row_ptr_host, plan.col_host, plan.n,
                                               plan.n_iso), 2, 1, 1, lm, damp)
    assert np.max(np.abs(b64.cpu().numpy() - want)) < 1e-12
