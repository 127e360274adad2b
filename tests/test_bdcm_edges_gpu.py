"""The BDCM kernels at their edges: both attractors, pure cycles (p = 0) and
c >= 3, a binding epsilon, both sides of every kernel-variant boundary, chunked
slab launches, the class limits and a NaN in the convergence loop.

Accuracy is per entry (bdcm_cases.entry_err): the exact zeros of the oracle
must be exact zeros on the device, and every other entry agrees to 1e-12
relative -- the project's float64 bar applied entry by entry.
All arithmetic is sums and products of non-negative numbers, and the oracle's
own dependence on the order of the neighbours is below 1e-13
(test_bdcm_cases.test_oracle_alone_stays_within_the_per_entry_bar), so the bar
is attainable; a miss is a finding in the kernel, not a number to loosen.
"""
import time

import numpy as np
import pytest
import torch

import bdcm_cases as bc
from oracle import bdcm as orc

pytestmark = pytest.mark.gpu

_PLANS = {}


def dev(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def forest_plan(mjx_mod, T):
    """The device plan of the boundary forest of T steps (one per session)."""
    if T not in _PLANS:
        n, edges, rp, col, _ = bc.forest_case(T)
        _PLANS[T] = mjx_mod.BDCMPlan(edges, rp, col, n_total=n, n_iso=0)
    return _PLANS[T]


def small_plan(mjx_mod, n_iso=bc.N_ISO):
    n, edges, rp, col, _ = bc.small_case()
    return mjx_mod.BDCMPlan(edges, rp, col, n_total=n + n_iso, n_iso=n_iso)


def check_observables(mjx_mod, chi_host, plan, hp, p, c, av, lm, epsilon):
    """Zi, Zij, phi and m_init of the device against the oracle on the same input."""
    chi = dev(chi_host)
    zi, zij = orc.Zi_ER(chi_host, hp, p, c, av, lm, epsilon), orc.Zij(chi_host, hp, p, c, av, epsilon)
    np.testing.assert_allclose(mjx_mod.Zi_ER(chi, plan, p, c, av, lm, epsilon).cpu().numpy(), zi, rtol=1e-12, atol=0)
    np.testing.assert_allclose(mjx_mod.Zij(chi, plan, p, c, av, epsilon).cpu().numpy(), zij, rtol=1e-12, atol=0)
    assert abs(mjx_mod.phi_BP_GENERAL_ER(chi, plan, p, c, av, lm, epsilon)
               - orc.phi_BP(chi_host, hp, p, c, av, lm, epsilon)) <= 1e-12
    assert abs(mjx_mod.avg_m_init_GENERAL_ER(chi, plan, p, c, av, epsilon)
               - orc.avg_m_init(chi_host, hp, p, c, av, epsilon)) <= 1e-12
    return zi, zij


@pytest.mark.parametrize("T", [3, 4])
def test_forests_sit_on_both_sides_of_the_lds_limit(mjx_mod, T):
    """The library's own answer: the last D of bdcm_cases.LDS_LAST_D keeps its
    count table in LDS, the next one runs from the slab, and the forest of T
    steps has edge and node classes on both sides."""
    lib = mjx_mod.load_library()
    p, c, D = T - 1, 1, bc.LDS_LAST_D[T]
    assert lib.mjx_bdcm_scratch_bytes(D, p, c) == 0
    assert lib.mjx_bdcm_scratch_bytes(D + 1, p, c) == 8 * 2 ** (T - 1) * (D + 2) ** T
    plan = forest_plan(mjx_mod, T)
    for classes in (plan.classes, [D for D, _, _, _ in plan.node_classes]):
        assert D in classes and D + 1 in classes
    assert plan.scratch(p, c) is not None


@pytest.mark.parametrize("epsilon", [0.0, 1e-3])
@pytest.mark.parametrize("attr_value", [1, -1])
@pytest.mark.parametrize("p,c", bc.PC_ALL)
def test_forest_parity_per_entry(mjx_mod, p, c, attr_value, epsilon):
    """Leaf reset, one assigning sweep (damppar = 1: the exact zeros show) and
    one damped sweep on the boundary forest against the oracle, and one
    assigning sweep of the random messages themselves (every message into a
    hub's table a different one), per entry within 1e-12; Zi, Zij, phi and
    m_init from the oracle's own messages and from the random ones -- with
    epsilon > 0 scaled so that the clamps of Zi and Zij bind on some items and
    not on others.
    Largest per-entry error measured on an MI355X over the forty cases:
    1.7e-15 (the sweep of the random messages at (1, 2), attractor +1,
    epsilon 0; 1.1e-15 after the leaf reset); the leaf reset is exact."""
    T = p + c
    lm = 0.7 * attr_value
    plan = forest_plan(mjx_mod, T)
    hp = bc.forest_case(T)[4]
    chi0 = bc.random_chi(2 * hp.E, T, 7 * p + c)
    t_start = time.perf_counter()
    leaf, s1, s2, raw = bc.oracle_leaf_and_sweeps(hp, chi0, p, c, attr_value, lm, epsilon)
    t_oracle = time.perf_counter() - t_start
    chi = dev(chi0)
    mjx_mod.bdcm_leaf_reset(chi, plan, p, c, attr_value, lm)
    errs = [bc.entry_err(chi.cpu().numpy(), leaf)]
    mjx_mod.BDCM_ER(chi, plan, p, c, attr_value, lm, 1.0, epsilon)
    errs.append(bc.entry_err(chi.cpu().numpy(), s1))
    chi = dev(s1)                                       # both sides read identical input
    mjx_mod.BDCM_ER(chi, plan, p, c, attr_value, lm, 0.3, epsilon)
    errs.append(bc.entry_err(chi.cpu().numpy(), s2))
    chi = dev(chi0)
    mjx_mod.BDCM_ER(chi, plan, p, c, attr_value, lm, 1.0, epsilon)
    errs.append(bc.entry_err(chi.cpu().numpy(), raw))
    print(f"per-entry error (p, c) = ({p}, {c}) attractor {attr_value} epsilon {epsilon}: "
          f"leaf {errs[0]:.3g} sweep {errs[1]:.3g} damped sweep {errs[2]:.3g} raw sweep {errs[3]:.3g}; "
          f"oracle sweeps {t_oracle:.2f} s of {time.perf_counter() - t_start:.2f} s so far")
    if epsilon == 0.0:
        upd = np.concatenate([hp.class_rows[D] for D in hp.classes if D > 0])
        assert np.all((s1[upd] == 0).mean(axis=1) >= 0.25)          # the sectors a row maximum would hide
    assert max(errs) <= 1e-12
    check_observables(mjx_mod, s2, plan, hp, p, c, attr_value, lm, epsilon)
    if epsilon == 0.0:
        check_observables(mjx_mod, chi0, plan, hp, p, c, attr_value, lm, epsilon)
    else:
        # the random messages scaled so that the median Zij lands on epsilon
        z0 = orc.Zij(chi0, hp, p, c, attr_value, 0.0)
        small = chi0 * np.sqrt(epsilon / np.median(z0))
        zi, zij = check_observables(mjx_mod, small, plan, hp, p, c, attr_value, lm, epsilon)
        assert 0 < np.count_nonzero(zij == epsilon) < zij.size
        assert 0 < np.count_nonzero(zi == epsilon) < zi.size


@pytest.mark.parametrize("p,c", [(1, 1), (0, 2), (2, 1), (2, 2)])
def test_flip_symmetry_on_the_device(mjx_mod, p, c):
    """(+1, lmbd, chi) and (-1, -lmbd, flip(chi)) are mirror images on the
    device too, isolated nodes included: messages, Zi, Zij per entry, phi equal
    and m_init opposite -- single plan and batch."""
    T = p + c
    lm, damp = 0.7, 0.3
    plan = small_plan(mjx_mod)
    assert plan.n_iso == 3 and plan.n == plan.n_core + 3
    chi0 = bc.random_chi(2 * plan.E, T, 50 + 10 * p + c)
    a, b = dev(chi0), dev(bc.flip(chi0, T))
    for x, av in ((a, 1), (b, -1)):
        mjx_mod.bdcm_leaf_reset(x, plan, p, c, av, av * lm)
        mjx_mod.BDCM_ER(x, plan, p, c, av, av * lm, damp)
    ah = a.cpu().numpy()
    assert bc.entry_err(bc.flip(b.cpu().numpy(), T), ah) <= 1e-12
    b = dev(bc.flip(ah, T))                             # exact mirror images as input
    assert bc.entry_err(mjx_mod.Zi_ER(b, plan, p, c, -1, -lm).cpu().numpy(),
                        mjx_mod.Zi_ER(a, plan, p, c, 1, lm).cpu().numpy()) <= 1e-12
    assert bc.entry_err(mjx_mod.Zij(b, plan, p, c, -1).cpu().numpy(),
                        mjx_mod.Zij(a, plan, p, c, 1).cpu().numpy()) <= 1e-12
    phi_p, m_p = mjx_mod.bdcm.observables(a, plan, p, c, 1, lm)
    phi_m, m_m = mjx_mod.bdcm.observables(b, plan, p, c, -1, -lm)
    assert abs(phi_p - phi_m) <= 1e-12 and abs(m_p + m_m) <= 1e-12
    assert abs(mjx_mod.phi_BP_GENERAL_ER(b, plan, p, c, -1, -lm) - phi_p) <= 1e-12
    assert abs(mjx_mod.avg_m_init_GENERAL_ER(b, plan, p, c, -1) + m_p) <= 1e-12
    # the batch: two instances that differ in their isolated nodes, both attractors
    other = small_plan(mjx_mod, n_iso=1)
    bt = mjx_mod.BDCMBatch([plan, other], p, c)
    out = {}
    for av in (1, -1):
        start = chi0 if av > 0 else bc.flip(chi0, T)
        chi = bt.chi_from([start, start])
        mjx_mod.bdcm_leaf_reset_batch(chi, bt, p, c, av, av * lm)
        mjx_mod.BDCM_ER_batch(chi, bt, p, c, av, av * lm, damp)
        out[av] = chi
    for v in bt.views(out[1]):
        assert torch.equal(v, a)
    assert bc.entry_err(bc.flip(out[-1].cpu().numpy(), T), out[1].cpu().numpy()) <= 1e-12
    mirror = dev(bc.flip(out[1].cpu().numpy(), T))
    phi_bp, m_bp = mjx_mod.bdcm_observables_batch(out[1], bt, p, c, 1, lm)
    phi_bm, m_bm = mjx_mod.bdcm_observables_batch(mirror, bt, p, c, -1, -lm)
    assert np.max(np.abs(phi_bp - phi_bm)) <= 1e-12 and np.max(np.abs(m_bp + m_bm)) <= 1e-12
    assert (phi_bp[0], m_bp[0]) == (phi_p, m_p) and (phi_bm[0], m_bm[0]) == (phi_m, m_m)
    assert m_bp[0] != m_bp[1]                           # the instances' own n_iso and n


@pytest.mark.parametrize("p,c,degrees", [(2, 1, bc.HUB_DEGREES[3]), (2, 2, bc.HUB_DEGREES[4]),
                                         (2, 1, (18, 18)), (2, 2, (8, 8))])
def test_chunked_slab_launches_of_a_single_plan(mjx_mod, p, c, degrees):
    """A slab of exactly one count table: the top hub's edge class goes out in
    k launches of one item (item offset > 0 into the class, table 0 of the
    slab), and with two hubs of the same degree the node kernel does too.
    Bit-identical to the plan with the default cap."""
    T = p + c
    lib = mjx_mod.load_library()
    n, edges, rp, col = bc.hub_forest(degrees, seed=T)
    Dmax = max(degrees)
    tab = lib.mjx_bdcm_scratch_bytes(Dmax, p, c)
    assert tab == 8 * 2 ** (T - 1) * (Dmax + 1) ** T
    assert 0 < lib.mjx_bdcm_scratch_bytes(Dmax - 1, p, c) and tab // lib.mjx_bdcm_scratch_bytes(Dmax - 1, p, c) == 1
    wide, narrow = (mjx_mod.BDCMPlan(edges, rp, col, n_total=n, n_iso=0) for _ in range(2))
    narrow.SCRATCH_CAP = tab
    assert narrow.scratch(p, c).numel() == tab                      # one table in flight
    assert wide.scratch(p, c).numel() > tab
    m_edge = [m for D, _, _, m in narrow.edge_classes if D == Dmax - 1][0]
    assert m_edge == Dmax * degrees.count(Dmax)
    chi0 = bc.random_chi(2 * wide.E, T, 3)
    a, b = dev(chi0), dev(chi0)
    for x, plan in ((a, wide), (b, narrow)):
        mjx_mod.bdcm_leaf_reset(x, plan, p, c, -1, 0.4)
        mjx_mod.BDCM_ER(x, plan, p, c, -1, 0.4, 0.3, 1e-3)
    assert torch.equal(a, b)
    x = dev(chi0)                                       # distinct messages into the node tables
    assert torch.equal(mjx_mod.Zi_ER(x, wide, p, c, -1, 0.4), mjx_mod.Zi_ER(x, narrow, p, c, -1, 0.4))


def test_class_limits(mjx_mod):
    """Degree 257 (edge class 256) is refused before any launch; the size
    functions at the limits (no launch at D = 44, T = 4: a 262 MB table)."""
    lib = mjx_mod.load_library()
    n, edges, rp, col = bc.hub_forest((257,))
    plan = mjx_mod.BDCMPlan(edges, rp, col, n_total=n, n_iso=0)
    assert max(plan.classes) == 256
    with pytest.raises(mjx_mod.MjxError):
        plan.check_sizes(0, 1)
    chi = dev(bc.random_chi(2 * plan.E, 1, 1))
    before = chi.clone()
    with pytest.raises(mjx_mod.MjxError):
        mjx_mod.Zi_ER(chi, plan, 0, 1, 1, 0.0)
    with pytest.raises(mjx_mod.MjxError):
        mjx_mod.BDCM_ER(chi, plan, 0, 1, 1, 0.0, 0.5)
    assert torch.equal(chi, before)
    assert lib.mjx_bdcm_scratch_bytes(45, 2, 2) == -1               # 46^4 > 2^22
    assert lib.mjx_bdcm_scratch_bytes(44, 2, 2) == 8 * 45 ** 4 * 8
    assert lib.mjx_bdcm_scratch_bytes(256, 0, 1) == -1 and lib.mjx_bdcm_lds_bytes(256, 0, 1) == -1
    for T, D in ((3, 16), (3, 17), (4, 6), (4, 7)):
        XV = 2 ** (T - 1)
        assert lib.mjx_bdcm_lds_bytes(D, T - 1, 1) == 8 * XV * (D + 1) ** T + 8 * D * XV * XV
        assert (lib.mjx_bdcm_lds_bytes(D, T - 1, 1) <= 160 * 1024) == (D == bc.LDS_LAST_D[T])


@pytest.mark.parametrize("graph", [True, False])
def test_nan_ends_the_device_loop_after_one_sweep(mjx_mod, graph):
    """One NaN in a non-leaf message: the reference's ``while delta > eps`` ends
    after that sweep (NaN > eps is false), and so does the device loop -- t = 1,
    a NaN delta, and chi exactly as one host-loop sweep leaves it."""
    p, c, lm, damp = 1, 1, 0.4, 0.3
    plan = small_plan(mjx_mod)
    chi0 = bc.random_chi(2 * plan.E, 2, 9)
    hp = bc.small_case()[4]
    row = int(hp.class_rows[max(hp.classes)][0])
    chi0[row, 5] = np.nan
    a, b = dev(chi0), dev(chi0)
    t, delta = mjx_mod.bdcm_converge(a, plan, p, c, 1, lm, damp, 1e-6, 50, batch=4, graph=graph)
    assert t == 1 and np.isnan(delta)
    mjx_mod.BDCM_ER(b, plan, p, c, 1, lm, damp)
    assert torch.isnan(b).any()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
