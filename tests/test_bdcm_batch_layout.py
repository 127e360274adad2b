"""The union layout of a BDCM batch (host index arrays only, no GPU): every
instance's share of a union class is that instance's own class, shifted by its
row / node offset, in the instance's own order."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import bdcm as orc


def path_graph(n=6):
    """0 - 1 - ... - n-1: leaves (edge class 0) and edge class 1, nothing above."""
    e = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    nbrs = [[k for k in (i - 1, i + 1) if 0 <= k < n] for i in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(x) for x in nbrs])])
    return e, rp, np.concatenate(nbrs)


@pytest.fixture(scope="module")
def graphs():
    out = []
    for name in ("bdcm_er_n300_deg2_p1c1.npz", "bdcm_er_n300_deg5_p1c1.npz"):
        z = load_golden(name)
        out.append((z["edges"], z["row_ptr"], z["col"]))
    out.insert(1, path_graph())             # an instance lacking classes, between two that have them
    return out


@pytest.fixture(scope="module")
def layout(mjx_mod, graphs):
    return mjx_mod.bdcm_batch_layout(graphs, 1, 1)


@pytest.fixture(scope="module")
def oracle_plans(graphs):
    return [orc.Plan.from_csr(e, rp, col, int(len(rp) - 1), 0) for e, rp, col in graphs]


def test_offsets_and_segments(layout, oracle_plans):
    G = layout["G"]
    assert G == len(oracle_plans) == 3
    E = np.array([pl.E for pl in oracle_plans])
    n = np.array([pl.n_core for pl in oracle_plans])
    assert np.array_equal(layout["row_off"], np.concatenate([[0], np.cumsum(2 * E)]))
    assert np.array_equal(layout["node_off"], np.concatenate([[0], np.cumsum(n)]))
    assert np.array_equal(layout["edge_seg"], np.concatenate([[0], np.cumsum(E)]))
    assert layout["edges"].shape == (E.sum(), 2) and layout["deg"].shape == (n.sum(),)
    for g, pl in enumerate(oracle_plans):
        lo, hi = layout["edge_seg"][g], layout["edge_seg"][g + 1]
        assert np.array_equal(layout["edges"][lo:hi] - layout["node_off"][g], pl.edges)
        assert np.array_equal(layout["deg"][layout["node_off"][g]:layout["node_off"][g + 1]], pl.deg)
        r = np.arange(pl.E)
        assert np.array_equal(layout["fwd_row"][lo:hi], layout["row_off"][g] + r)
        assert np.array_equal(layout["rev_row"][lo:hi], layout["row_off"][g] + r + pl.E)


def same_sets(got, want):
    return got.shape == want.shape and np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1))


def test_edge_classes_are_the_instances_classes(layout, oracle_plans):
    Ds = [D for D, *_ in layout["edge_classes"]]
    assert Ds == sorted(set().union(*[pl.classes for pl in oracle_plans]))
    seen = 0
    for D, rows, inc, inst in layout["edge_classes"]:
        assert rows.shape == inst.shape and inc.shape == (rows.size, D)
        assert np.all(np.diff(inst) >= 0)                      # ordered by instance
        for g, pl in enumerate(oracle_plans):
            sel = inst == g
            if D not in pl.class_rows:
                assert not sel.any()
                continue
            assert np.array_equal(rows[sel] - layout["row_off"][g], pl.class_rows[D])
            assert same_sets(inc[sel] - layout["row_off"][g], pl.class_inc[D])
        seen += rows.size
    assert seen == layout["row_off"][-1]                       # every message in exactly one class
    assert set(oracle_plans[1].classes) == {0, 1}              # the path graph: leaves and class 1 only


def test_node_classes_are_the_instances_classes(layout, oracle_plans):
    assert [D for D, *_ in layout["node_classes"]] == sorted(set().union(*[pl.node_classes for pl in oracle_plans]))
    seen = 0
    for D, nodes, inc, inst in layout["node_classes"]:
        assert inc.shape == (nodes.size, D) and np.all(np.diff(inst) >= 0)
        for g, pl in enumerate(oracle_plans):
            sel = inst == g
            if D not in pl.node_rows:
                assert not sel.any()
                continue
            assert np.array_equal(nodes[sel] - layout["node_off"][g], pl.node_rows[D])
            assert same_sets(inc[sel] - layout["row_off"][g], pl.node_inc[D])
        seen += nodes.size
    assert seen == layout["node_off"][-1]


def test_bad_batches_raise(mjx_mod, graphs):
    with pytest.raises(ValueError):
        mjx_mod.bdcm_batch_layout([], 1, 1)
    with pytest.raises(ValueError):
        mjx_mod.bdcm_batch_layout(graphs, 1, 1, pcs=[(1, 1), (2, 1), (1, 1)])
    assert mjx_mod.bdcm_batch_layout(graphs, 1, 1, pcs=[(1, 1)] * 3)["G"] == 3


def test_union_beyond_int32_raises(mjx_mod, monkeypatch):
    """Row and node ids are int32 on the device: a union past 2^31 - 1 rows is
    refused (the limit lowered here, the check is the same comparison)."""
    import mjx.bdcm_batch as bb
    monkeypatch.setattr(bb, "INT32_MAX", 15)
    assert mjx_mod.bdcm_batch_layout([path_graph()], 1, 1)["row_off"][-1] == 10
    with pytest.raises(ValueError):
        mjx_mod.bdcm_batch_layout([path_graph(), path_graph()], 1, 1)
