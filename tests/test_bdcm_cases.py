"""The BDCM edge cases on the host (numpy only): the forests have the classes
they are built for, the oracle is symmetric under the global spin flip
(which defines the attr_value = -1 attractor), and the oracle alone
stays within the per-entry bar that tests/test_bdcm_edges_gpu.py holds the
kernels to."""
import itertools

import numpy as np
import pytest

import bdcm_cases as bc
from oracle import bdcm as orc


@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_hub_forest_has_exactly_the_intended_classes(mjx_mod, T):
    ks = bc.HUB_DEGREES[T]
    n, edges, rp, col, hp = bc.forest_case(T)
    assert n == sum(ks) - (len(ks) - 1) + 1 and edges.shape == (n - 1, 2)       # a tree
    assert np.array_equal(np.diff(rp)[:len(ks)], ks) and np.all(np.diff(rp)[len(ks):] == 1)
    assert hp.classes == sorted({0} | {k - 1 for k in ks})
    assert hp.node_classes == sorted({1} | set(ks))
    h = mjx_mod.bdcm_plan_indices(edges, rp, col)
    assert [D for D, _, _ in h["edge_classes"]] == hp.classes
    assert [D for D, _, _ in h["node_classes"]] == hp.node_classes
    for (D, rows, inc), Do in zip(h["edge_classes"], hp.classes):
        assert np.array_equal(rows, hp.class_rows[Do]) and np.array_equal(inc, hp.class_inc[Do])
    for (D, nodes, inc), Do in zip(h["node_classes"], hp.node_classes):
        assert np.array_equal(nodes, hp.node_rows[Do]) and np.array_equal(inc, hp.node_inc[Do])
    # the permuted rows are a permutation of the plain ones, and not the identity
    _, e0, rp0, col0 = bc.hub_forest(ks)
    assert np.array_equal(e0, edges) and np.array_equal(rp0, rp) and not np.array_equal(col0, col)
    for i in range(n):
        assert sorted(col0[rp[i]:rp[i + 1]]) == sorted(col[rp[i]:rp[i + 1]])


def test_hub_forest_rejects_a_hub_without_room_for_the_path():
    with pytest.raises(ValueError):
        bc.hub_forest((2, 1, 2))


def test_flip_and_entry_err():
    chi = np.arange(2 * 16, dtype=np.float64).reshape(2, 16)
    f = bc.flip(chi, 2)
    assert f[0, 0] == 15 and f[1, 5] == 16 + 10 and np.array_equal(bc.flip(f, 2), chi)
    want = np.array([[0.0, 1.0, 1e-6]])
    assert bc.entry_err(np.array([[0.0, 1.0, 1.1e-6]]), want) == pytest.approx(0.1)
    with pytest.raises(AssertionError):
        bc.entry_err(np.array([[1e-300, 1.0, 1e-6]]), want)          # a zero that is not exact
    with pytest.raises(AssertionError):
        bc.entry_err(np.array([[0.0, np.nan, 1e-6]]), want)


@pytest.mark.parametrize("epsilon", [0.0, 1e-4])
@pytest.mark.parametrize("p,c", bc.PC_ALL)
def test_oracle_is_symmetric_under_the_global_spin_flip(p, c, epsilon):
    """The majority rule with always-stay ties commutes with flipping every
    spin, so (attr_value, lmbd, chi) and (-attr_value, -lmbd, flip(chi)) are
    mirror images: messages, Zi and Zij equal under the flip, phi equal, m_init
    opposite.  The graph has isolated nodes, which follow the attractor
    (phi and m_init missed by 2 lmbd n_iso / n and 2 n_iso / n before they did)."""
    T = p + c
    n, edges, rp, col, hp = bc.small_case()
    assert hp.n_iso == bc.N_ISO > 0
    lm = 0.7
    chi0 = bc.random_chi(2 * hp.E, T, 100 + 10 * p + c)
    plus = bc.oracle_leaf_and_sweeps(hp, chi0, p, c, 1, lm, epsilon)
    minus = bc.oracle_leaf_and_sweeps(hp, bc.flip(chi0, T), p, c, -1, -lm, epsilon)
    for a, b in zip(plus, minus):
        assert bc.entry_err(bc.flip(b, T), a) <= 1e-13
    a, b = plus[2], bc.flip(plus[2], T)                  # exact mirror images as input
    np.testing.assert_allclose(orc.Zi_ER(b, hp, p, c, -1, -lm, epsilon), orc.Zi_ER(a, hp, p, c, 1, lm, epsilon),
                               rtol=1e-13, atol=0)
    np.testing.assert_allclose(orc.Zij(b, hp, p, c, -1, epsilon), orc.Zij(a, hp, p, c, 1, epsilon), rtol=1e-13, atol=0)
    assert abs(orc.phi_BP(a, hp, p, c, 1, lm, epsilon) - orc.phi_BP(b, hp, p, c, -1, -lm, epsilon)) <= 1e-13
    assert abs(orc.avg_m_init(a, hp, p, c, 1, epsilon) + orc.avg_m_init(b, hp, p, c, -1, epsilon)) <= 1e-13


def test_entropy_procedure_is_symmetric_under_the_flip():
    """The whole lambda procedure inherits the symmetry (it calls phi_BP and
    avg_m_init): same iteration counts and entropies, opposite m_init."""
    n, edges, rp, col, hp = bc.small_case()
    chi0 = bc.random_chi(2 * hp.E, 2, 5)
    lambdas = np.array([0.0, 0.4])
    mp, e1p, ep, _, itp, _ = orc.entropy_procedure(chi0, hp, 1, 1, 1, lambdas, 0.3, eps=1e-8, T_max=200)
    mm, e1m, em, _, itm, _ = orc.entropy_procedure(bc.flip(chi0, 2), hp, 1, 1, -1, -lambdas, 0.3, eps=1e-8, T_max=200)
    assert np.array_equal(itp, itm) and itp.max() < 200
    np.testing.assert_allclose(mm, -mp, rtol=0, atol=1e-13)
    np.testing.assert_allclose(em, ep, rtol=0, atol=1e-13)
    np.testing.assert_allclose(e1m, e1p, rtol=0, atol=1e-13)


@pytest.mark.parametrize("attr_value", [1, -1])
@pytest.mark.parametrize("p,c", bc.PC_ALL)
def test_oracle_alone_stays_within_the_per_entry_bar(p, c, attr_value):
    """The oracle against itself with every neighbour list reversed (another
    order of the convolution's products and sums) on the boundary forests:
    per entry within 1e-13, which licenses the kernels' per-entry bar of 1e-12.
    Measured: 1.7e-15 at most over the twenty cases (at T = 1, with the
    degree-255 hub)."""
    T = p + c
    n, edges, rp, col, hp = bc.forest_case(T)
    hr = orc.Plan.from_csr(edges, rp, bc.reverse_rows(rp, col), n, 0)
    lm = 0.7 * attr_value
    chi0 = bc.random_chi(2 * hp.E, T, 7 * p + c)
    a = bc.oracle_leaf_and_sweeps(hp, chi0, p, c, attr_value, lm, 0.0)
    b = bc.oracle_leaf_and_sweeps(hr, chi0, p, c, attr_value, lm, 0.0)
    worst = max(bc.entry_err(x, y) for x, y in zip(a, b))
    for x in (a[2], chi0):
        za, zb = orc.Zi_ER(x, hp, p, c, attr_value, lm), orc.Zi_ER(x, hr, p, c, attr_value, lm)
        worst = max(worst, bc.entry_err(zb, za))
    print(f"oracle vs reversed oracle (p, c) = ({p}, {c}) attractor {attr_value}: {worst:.3g}")
    assert worst <= 1e-13
    # a quarter or more of every updated row is exactly zero at epsilon = 0, and the test sees it
    upd = np.concatenate([hp.class_rows[D] for D in hp.classes if D > 0])
    assert np.all((a[1][upd] == 0).mean(axis=1) >= 0.25)


@pytest.mark.parametrize("attr_value", [1, -1])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_pure_cycle_factors_by_enumeration(c, attr_value):
    """p = 0: the last step closes the cycle onto t = 0.  leaf_message and
    factor_A / factor_Ai against allowed(), entry by entry."""
    p, T, X = 0, c, 2 ** c
    tr = 2 * orc.traj01(T) - 1
    lm = 0.3
    leaf = orc.leaf_message(p, c, attr_value, lm).reshape(X, X)
    want = np.zeros((X, X))
    for a, b in itertools.product(range(X), repeat=2):
        if tr[a][T - 1] == attr_value:
            want[a, b] = np.exp(-lm * tr[a][0]) * orc.allowed(tr[a], tr[b], np.zeros(T, dtype=np.int64), p, c)
    assert want.sum() > 0
    assert bc.entry_err(leaf, want / want.sum()) <= 1e-15
    if c == 1:
        # one time step, no neighbours: the field is the receiver's spin, which the spin must equal
        k = 1 if attr_value > 0 else 0
        assert np.count_nonzero(leaf) == 1 and leaf[k, k] == 1.0
    D = 2
    rhos = list(itertools.product(range(D + 1), repeat=T))
    A, Ai = orc.factor_A(D, p, c, attr_value), orc.factor_Ai(D, p, c, attr_value)
    assert A.shape == (X, X, len(rhos)) and Ai.shape == (X, len(rhos))
    for a in range(X):
        ends = tr[a][T - 1] == attr_value
        for q, rho in enumerate(rhos):
            f = 2 * np.array(rho) - D
            assert Ai[a, q] == (orc.allowed(tr[a], np.zeros(T, dtype=np.int64), f, p, c) if ends else 0)
            for b in range(X):
                assert A[a, b, q] == (orc.allowed(tr[a], tr[b], f, p, c) if ends else 0)
