"""GPU tests of the BDCM batch path (a batch of graphs as one disjoint union
with per-instance control).  The bar is bit-for-bit equality with the
single-plan functions on each instance alone -- per-item arithmetic does not
depend on the grid position and a maximum does not depend on the order -- and,
where a reference fixture exists, the existing tests' distance to it.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEG2, DEG5, T3 = "bdcm_er_n300_deg2_p1c1.npz", "bdcm_er_n300_deg5_p1c1.npz", "bdcm_er_n120_deg3_p1c2.npz"


def dev(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def rowrel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.max(np.abs(ref), axis=1, keepdims=True)))


@pytest.fixture(scope="module")
def fx():
    return {name: load_golden(name) for name in (DEG2, DEG5, T3)}


@pytest.fixture(scope="module")
def plans(mjx_mod, fx):
    return {name: mjx_mod.BDCMPlan(z["edges"], z["row_ptr"], z["col"], n_total=int(z["n"]), n_iso=int(z["n_iso"]))
            for name, z in fx.items()}


@pytest.fixture(scope="module")
def pair(mjx_mod, plans):
    """The two p = c = 1 fixtures as one batch."""
    return mjx_mod.BDCMBatch([plans[DEG2], plans[DEG5]], 1, 1)


def run_single(mjx_mod, fx, plans, lambdas, **kw):
    """Single-plan lambda sweeps of the two p = c = 1 fixtures: [(result dict, final chi)]."""
    out = []
    for name in (DEG2, DEG5):
        z = fx[name]
        chi = dev(z["chi0"])
        res = mjx_mod.BDCM_entropy_procedure_GENERAL_ER(chi, plans[name], lambdas, p=1, c=1, damppar=float(z["damppar"]),
                                                        **kw)
        out.append((res, chi))
    return out


def run_batch(mjx_mod, fx, pair, lambdas, **kw):
    chi = pair.chi_from([fx[DEG2]["chi0"], fx[DEG5]["chi0"]])
    res = mjx_mod.BDCM_entropy_procedure_batch(chi, pair, lambdas, p=1, c=1, damppar=float(fx[DEG2]["damppar"]), **kw)
    return res, pair.views(chi)


def assert_same_runs(res, views, single):
    for g, (want, chi) in enumerate(single):
        assert set(res[g]) == set(want)
        assert np.array_equal(res[g]["iters"], want["iters"]), g
        for k in ("m_init", "ent1", "ent"):
            assert np.array_equal(res[g][k], want[k]), (g, k)
        assert res[g]["counts"] == want["counts"], g
        assert torch.equal(views[g], chi), g


def test_batch_equals_separate_runs_and_reference(mjx_mod, fx, plans, pair):
    """Instances that stop at different sweeps inside the same captured batches
    (iterations [193, 233] and [179, 191])."""
    z2 = fx[DEG2]
    kw = dict(T_max=int(z2["T_max"]), eps=float(z2["eps"]))
    lambdas = [0.0, 0.5]
    res, views = run_batch(mjx_mod, fx, pair, lambdas, **kw)
    assert_same_runs(res, views, run_single(mjx_mod, fx, plans, lambdas, **kw))
    for g, name in enumerate((DEG2, DEG5)):
        z = fx[name]
        assert np.array_equal(res[g]["iters"], z["iters"][:2])
        for k in ("m_init", "ent1", "ent"):
            np.testing.assert_allclose(res[g][k], z[k][:2], rtol=1e-9, atol=1e-12)
    assert list(res[0]["iters"]) == [193, 233] and list(res[1]["iters"]) == [179, 191]


def test_instances_leave_the_lambda_sweep_at_different_lambda(mjx_mod, fx, plans, pair):
    """stop_ent = 0.28: the deg-2 instance (ent1 0.2994, 0.2698) stops after
    lambda = 0.5 and stays frozen while the deg-5 one (0.4446, 0.4109) goes on."""
    kw = dict(T_max=1300, eps=float(fx[DEG2]["eps"]), stop_ent=0.28)
    lambdas = [0.0, 0.5, 1.0]
    res, views = run_batch(mjx_mod, fx, pair, lambdas, **kw)
    assert_same_runs(res, views, run_single(mjx_mod, fx, plans, lambdas, **kw))
    assert res[0]["iters"][2] == 0 and res[0]["ent1"][2] == 0.0 and res[0]["ent1"][1] < 0.28
    assert res[1]["iters"][2] > 0 and res[1]["ent1"][2] != 0.0
    frozen = views[0].clone()
    _, short = run_batch(mjx_mod, fx, pair, lambdas[:2], **kw)
    assert torch.equal(frozen, short[0])


def test_t_max_per_instance(mjx_mod, fx, plans, pair):
    """T_max = 200: at lambda = 0.5 the deg-2 instance (233 sweeps needed) stops
    at 200 with counts = 0.5 and leaves; the deg-5 one (191) converges and goes on."""
    kw = dict(T_max=200, eps=float(fx[DEG2]["eps"]))
    lambdas = [0.0, 0.5, 1.0]
    res, views = run_batch(mjx_mod, fx, pair, lambdas, **kw)
    assert_same_runs(res, views, run_single(mjx_mod, fx, plans, lambdas, **kw))
    assert res[0]["counts"] == 0.5 and list(res[0]["iters"]) == [193, 200, 0]
    assert res[1]["iters"][1] == 191 and res[1]["iters"][2] > 0      # went on to lambda = 1.0


def test_t_max_inside_a_captured_batch(mjx_mod, fx, plans, pair):
    """eps = 0 never converges: every instance reports exactly T_max = 11 sweeps
    with 8 sweeps per replay, and chi is 11 eager single-plan sweeps."""
    damp = float(fx[DEG2]["damppar"])
    chi = pair.chi_from([fx[DEG2]["chi0"], fx[DEG5]["chi0"]])
    t, _ = mjx_mod.bdcm_converge_batch(chi, pair, 1, 1, 1, 0.3, damp, 0.0, 11, batch_sweeps=8)
    assert t.tolist() == [11, 11]
    for g, name in enumerate((DEG2, DEG5)):
        b = dev(fx[name]["chi0"])
        for _ in range(11):
            mjx_mod.BDCM_ER(b, plans[name], 1, 1, 1, 0.3, damp)
        assert torch.equal(pair.views(chi)[g], b)


def test_gating_at_the_abi_level(mjx_mod, fx, plans):
    """One gated union sweep with the middle instance's stop flag preset."""
    names = (DEG2, DEG5, DEG2)
    bt = mjx_mod.BDCMBatch([plans[n] for n in names], 1, 1)
    rng = np.random.default_rng(5)
    chi0 = [fx[DEG2]["chi0"], fx[DEG5]["chi0"], rng.permutation(fx[DEG2]["chi0"])]
    damp, lm = 0.1, 0.4
    chi = bt.chi_from(chi0)
    before = chi.clone()
    ctl = bt.set_active([True, False, True])
    sentinel = 0x1234567
    ctl[1, 0] = sentinel
    assert ctl.cpu()[:, 1].tolist() == [0, 1, 0]
    mjx_mod.BDCM_ER_batch(chi, bt, 1, 1, 1, lm, damp, gated=True, delta=True)
    h = ctl.cpu().numpy()
    views, old = bt.views(chi), bt.views(before)
    assert torch.equal(views[1], old[1])
    assert h[1, 0] == sentinel
    for g in (0, 2):
        plan = plans[names[g]]
        b = dev(chi0[g])
        plan._delta.zero_()
        mjx_mod.BDCM_ER(b, plan, 1, 1, 1, lm, damp, delta=plan._delta)
        assert torch.equal(views[g], b)
        assert h[g, 0] == int(plan._delta.item()) and h[g, 0] != 0
    assert h[0, 0] != h[2, 0]                       # each instance its own maximum


def hub_plan(mjx_mod):
    """n = 120, mean degree 3, node 0 raised to degree >= 14: its edge class
    D >= 13 exceeds the LDS budget at T = 3."""
    rng = np.random.default_rng(3)
    n = 120
    u, v = mjx_mod.erdos_renyi_edges(n, 3.0 / (n - 1), seed=4)
    hub_nb = rng.choice(np.arange(1, n), size=14, replace=False)
    pairs = set(zip(u.tolist(), v.tolist())) | {(0, int(k)) for k in hub_nb}
    pairs = sorted((min(a, b), max(a, b)) for a, b in pairs if a != b)
    pairs = sorted(set(pairs))
    u, v = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    n2, u2, v2, iso = mjx_mod.remove_isolated(n, u, v)
    rp, col = mjx_mod.csr_from_edges(n2, u2, v2)
    return mjx_mod.BDCMPlan(np.stack([u2, v2], axis=1), rp, col, n_total=n, n_iso=iso)


def test_three_steps_and_the_scratch_slab(mjx_mod, fx, plans):
    """p = 1, c = 2: the fixture and the hub graph as one batch, the hub's class
    in at least two chunked launches from a small slab."""
    z = fx[T3]
    p, c, lm, damp = 1, 2, float(z["sweep_lmbd"]), float(z["damppar"])
    hub = hub_plan(mjx_mod)
    lib = mjx_mod.load_library()
    Dmax = max(hub.classes)
    tab = lib.mjx_bdcm_scratch_bytes(Dmax, p, c)
    assert Dmax >= 13 and tab > 0
    bt = mjx_mod.BDCMBatch([plans[T3], hub], p, c)
    bt.SCRATCH_CAP = 2 * tab                        # two tables in flight, >= 14 items in the hub's class
    m_hub = [m for D, *_, m in bt.edge_classes if D == Dmax][0]
    assert m_hub >= 14 and bt.scratch_args()[1] // tab == 2
    rng = np.random.default_rng(11)
    x = rng.random((2 * hub.E, 64))
    chi0 = [z["chi0"], x / x.sum(axis=1, keepdims=True)]
    chi = bt.chi_from(chi0)
    mjx_mod.bdcm_leaf_reset_batch(chi, bt, p, c, 1, lm)
    singles = [dev(a) for a in chi0]
    for b, plan in zip(singles, (plans[T3], hub)):
        mjx_mod.bdcm_leaf_reset(b, plan, p, c, 1, lm)
    for g in range(2):
        assert torch.equal(bt.views(chi)[g], singles[g])
    assert rowrel(bt.views(chi)[0].cpu().numpy(), z["sweep_leaf"]) < 1e-14
    mjx_mod.BDCM_ER_batch(chi, bt, p, c, 1, lm, damp)
    phi, m_init = mjx_mod.bdcm_observables_batch(chi, bt, p, c, 1, lm)
    zi, zij, _ = mjx_mod.bdcm_partition_batch(chi, bt, p, c, 1, lm)
    for g, (b, plan) in enumerate(zip(singles, (plans[T3], hub))):
        mjx_mod.BDCM_ER(b, plan, p, c, 1, lm, damp)
        assert torch.equal(bt.views(chi)[g], b)
        assert torch.equal(zi[bt.node_off[g]:bt.node_off[g + 1]], mjx_mod.Zi_ER(b, plan, p, c, 1, lm))
        assert torch.equal(zij[bt.edge_seg[g]:bt.edge_seg[g + 1]], mjx_mod.Zij(b, plan, p, c, 1))
        assert (phi[g], m_init[g]) == mjx_mod.bdcm.observables(b, plan, p, c, 1, lm)
    # the fixture instance against the reference's own values, as the single-plan test
    assert rowrel(bt.views(chi)[0].cpu().numpy(), z["sweep_chi"]) < 1e-12
    ref = bt.chi_from([z["sweep_chi"], singles[1]])
    zi, zij, _ = mjx_mod.bdcm_partition_batch(ref, bt, p, c, 1, lm)
    np.testing.assert_allclose(zi[:bt.node_off[1]].cpu().numpy(), z["sweep_zi"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(zij[:bt.edge_seg[1]].cpu().numpy(), z["sweep_zij"], rtol=1e-12, atol=0)
    phi, m_init = mjx_mod.bdcm_observables_batch(ref, bt, p, c, 1, lm)
    assert abs(phi[0] - float(z["sweep_phi"])) < 1e-12
    assert abs(m_init[0] - float(z["sweep_m_init"])) < 1e-12


@pytest.mark.parametrize("take_log", [0, 1])
def test_segsum_has_the_bits_of_sum_f64(mjx_mod, take_log):
    lib = mjx_mod.load_library()
    lens = [0, 1, 255, 257, 70001]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = dev(np.random.default_rng(2).random(int(seg[-1])) + 0.05)
    G = len(lens)
    segd = torch.from_numpy(seg).cuda()
    work = torch.empty(G * 256, dtype=torch.float64, device="cuda")
    out = torch.full((G,), -1.0, dtype=torch.float64, device="cuda")
    st = mjx_mod._device.stream_handle()
    assert lib.mjx_segsum_f64(x.data_ptr(), segd.data_ptr(), G, take_log, work.data_ptr(), out.data_ptr(), st) == 0
    w1 = torch.empty(256, dtype=torch.float64, device="cuda")
    one = torch.empty(G, dtype=torch.float64, device="cuda")
    for g in range(G):
        assert lib.mjx_sum_f64(x.data_ptr() + 8 * int(seg[g]), lens[g], take_log, w1.data_ptr(),
                               one.data_ptr() + 8 * g, st) == 0
    got, want = out.cpu().numpy(), one.cpu().numpy()
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert got[0] == 0.0
    np.testing.assert_allclose(got[4], (np.log(x[seg[4]:].cpu().numpy()) if take_log else x[seg[4]:].cpu().numpy()).sum(),
                               rtol=1e-12)


def test_graph_replay_equals_eager_launches(mjx_mod, fx, pair):
    damp, eps, lm = float(fx[DEG2]["damppar"]), float(fx[DEG2]["eps"]), 0.5
    chi0 = [fx[DEG2]["chi0"], fx[DEG5]["chi0"]]
    out = []
    keep = []
    for graph in (True, False, True):
        chi = pair.chi_from(chi0)               # a fresh tensor: the third run must not replay the first capture
        keep.append(chi)
        mjx_mod.bdcm_leaf_reset_batch(chi, pair, 1, 1, 1, lm)
        t, d = mjx_mod.bdcm_converge_batch(chi, pair, 1, 1, 1, lm, damp, eps, 1300, batch_sweeps=7, graph=graph)
        out.append((t, d, chi))
    assert len({c.data_ptr() for c in keep}) == 3
    for t, d, chi in out[1:]:
        assert np.array_equal(t, out[0][0]) and np.array_equal(d.view(np.int64), out[0][1].view(np.int64))
        assert torch.equal(chi, out[0][2])
    assert out[0][0][0] != out[0][0][1] and np.all(out[0][1] <= eps) and np.all(out[0][1] > 0)
    # instances held still by the active mask are untouched and report t = 0
    chi = pair.chi_from(chi0)
    before = chi.clone()
    t, _ = mjx_mod.bdcm_converge_batch(chi, pair, 1, 1, 1, lm, damp, eps, 1300, active=[False, True], batch_sweeps=7)
    assert t[0] == 0 and t[1] > 0
    assert torch.equal(pair.views(chi)[0], pair.views(before)[0])
    assert not torch.equal(pair.views(chi)[1], pair.views(before)[1])


@pytest.fixture(scope="module")
def er_run_sequential(mjx_mod):
    return mjx_mod.bdcm_er_run(n=200, deg=(1.0, 3.0), num_rep=2, a=1, dl=0.5, seed=3, batch=0)


@pytest.mark.parametrize("B", [4, 3])
def test_er_run_batched_equals_sequential(mjx_mod, er_run_sequential, B):
    """batch = 3: the last group is partial."""
    got = mjx_mod.bdcm_er_run(n=200, deg=(1.0, 3.0), num_rep=2, a=1, dl=0.5, seed=3, batch=B)
    assert set(got) == set(er_run_sequential)
    for k, want in er_run_sequential.items():
        assert np.array_equal(got[k], want), k
    assert np.any(got["ent1"] != 0)


def test_abi_rejects_missing_instance_arrays(mjx_mod):
    lib = mjx_mod.load_library()
    L = mjx_mod._lib
    fake = ctypes.c_void_p(64)              # never dereferenced: validation fails first
    for flags in (L.MJX_BDCM_GATE, L.MJX_BDCM_DELTA, L.MJX_BDCM_GATE | L.MJX_BDCM_DELTA):
        assert lib.mjx_bdcm_update_class_batch(fake, fake, fake, None, 4, 1, 1, 1, 1, 0.0, 0.1, 0.0, fake, fake,
                                               flags, None, None, 0, None) == L.MJX_EINVAL
        assert lib.mjx_bdcm_update_class_batch(fake, fake, fake, fake, 4, 1, 1, 1, 1, 0.0, 0.1, 0.0, fake, None,
                                               flags, None, None, 0, None) == L.MJX_EINVAL
    assert lib.mjx_bdcm_update_class_batch(fake, fake, fake, fake, 4, 1, 1, 1, 1, 0.0, 0.1, 0.0, fake, fake, 4,
                                           None, None, 0, None) == L.MJX_EINVAL
    assert lib.mjx_abi_version() == 2
