"""The host side of the ER-HPR edge tests (tests/test_hpr_er_edges_gpu.py),
which needs no GPU: the built graphs hold the classes they are recorded with,
the LDS-budget formula gives the recorded bytes at the classes around the
budget, and the oracle loops give the recorded figures."""
import pytest
import torch

import hpr_er_cases as hc


@pytest.mark.parametrize("name", list(hc.GRAPHS))
def test_built_graphs_hold_their_recorded_classes(name):
    n0, _, _, hub_degs, want = hc.GRAPHS[name]
    G = hc.built(name)                                    # asserts the leaf, the hubs and the class set
    assert G.class_set == want and 0 in want and all(g - 1 in want for g in hub_degs)
    assert G.n <= n0 + 1 + len(hub_degs) and G.deg.min() >= 1
    assert G.col.size == 2 * G.E and G.out_rows.size == 2 * G.E


def test_lds_budget_formula_at_the_boundary_classes():
    """Table plus incoming messages, 8 B an entry for either dtype, against the 160 KiB."""
    want = {4: (6, 159808, 7, 262144), 3: (16, 161312, 17, 186624)}
    for T, (name, d_lds, d_slab) in hc.BOUNDARY.items():
        for dtype in (torch.float32, torch.float64):
            lds_bytes = hc.table_bytes(dtype, d_lds, T) + hc.incoming_bytes(dtype, d_lds, T)
            assert (d_lds, lds_bytes, d_slab, hc.scratch_bytes(dtype, d_slab, T)) == want[T]
            assert hc.scratch_bytes(dtype, d_lds, T) == 0 and lds_bytes <= hc.K_MAX_LDS
        G = hc.built(name)
        assert d_lds in G.class_set and d_slab in G.class_set
        assert all(D in hc.built(hc.MORE_SLAB[T][0]).class_set for D in hc.MORE_SLAB[T][1])


@pytest.mark.parametrize("key", list(hc.LOOPS), ids=lambda k: f"{k[0]}-p{k[1]}c{k[2]}-lm{k[5]}")
def test_oracle_loops_give_their_recorded_figures(key):
    hc.check_loop(key)
