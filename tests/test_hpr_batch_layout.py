"""The union layout of an HPR batch (host index arrays only, no GPU): instance
g's nodes are g n + i, its forward rows g E + r, its reverse rows E_tot + g E + r,
and the union's out_row / in_row are each instance's own, shifted."""
import numpy as np
import pytest

N, D, G = 10, 3, 3


@pytest.fixture(scope="module")
def graphs(mjx_mod):
    return [mjx_mod.random_regular_edges(D, N, seed=100 + k) for k in range(G)]


@pytest.fixture(scope="module")
def layout(mjx_mod, graphs):
    return mjx_mod.hpr_batch_layout(graphs, N, D)


def numpy_rows(edges, n, nbrs):
    """out_row / in_row of one graph by the definition: row r is edges[r] = (u, v)
    as u -> v, row r + E is v -> u."""
    E = len(edges)
    row = {}
    for r, (u, v) in enumerate(np.asarray(edges).tolist()):
        row[(u, v)] = r
        row[(v, u)] = r + E
    out = np.array([[row[(a, k)] for k in nbrs[a]] for a in range(n)])
    inn = np.array([[row[(k, a)] for k in nbrs[a]] for a in range(n)])
    return out, inn


def test_union_edges_nbrs_and_row_maps(layout, graphs):
    E = N * D // 2
    Et = G * E
    assert (layout["G"], layout["n"], layout["d"], layout["E"], layout["E_tot"]) == (G, N, D, E, Et)
    assert layout["edges"].shape == (Et, 2) and layout["nbrs"].shape == (G * N, D)
    assert np.array_equal(layout["node_off"], np.arange(G + 1) * N)
    assert layout["rows"].shape == (G, 2 * E)
    for g, e in enumerate(graphs):
        assert np.array_equal(layout["edges"][g * E:(g + 1) * E], np.asarray(e) + g * N)
        assert np.array_equal(layout["rows"][g, :E], g * E + np.arange(E))
        assert np.array_equal(layout["rows"][g, E:], Et + g * E + np.arange(E))
        nb = layout["nbrs"][g * N:(g + 1) * N] - g * N
        assert nb.min() >= 0 and nb.max() < N                   # no neighbour outside the instance
        for a in range(N):                                      # sorted neighbour lists of the instance's own edges
            want = sorted([v for u, v in np.asarray(e).tolist() if u == a] +
                          [u for u, v in np.asarray(e).tolist() if v == a])
            assert nb[a].tolist() == want
    assert np.array_equal(np.sort(layout["rows"].reshape(-1)), np.arange(2 * Et))      # a bijection onto the rows


def test_per_instance_rows_are_the_unions_minus_offsets(layout, graphs):
    E = N * D // 2
    Et = G * E
    for g, e in enumerate(graphs):
        nb = layout["nbrs"][g * N:(g + 1) * N] - g * N
        out, inn = numpy_rows(e, N, nb)
        for name, own in (("out_row", out), ("in_row", inn)):
            got = layout[name][g * N:(g + 1) * N]
            assert np.array_equal(got, layout["rows"][g][own]), name
            # forward rows shift by g E, reverse rows by E_tot - E + g E
            assert np.array_equal(np.where(got < Et, got - g * E, got - Et - g * E + E), own), name
    # the union is itself a d-regular graph on G n nodes: the same arrays by the definition
    out, inn = numpy_rows(layout["edges"], G * N, layout["nbrs"])
    assert np.array_equal(layout["out_row"], out) and np.array_equal(layout["in_row"], inn)


def test_union_equals_the_plan_indices_of_the_union_graph(mjx_mod, layout):
    e, nbrs, out, inn = mjx_mod.hpr_plan_indices(layout["edges"], G * N, D, layout["nbrs"])
    assert np.array_equal(out, layout["out_row"]) and np.array_equal(inn, layout["in_row"])
    assert np.array_equal(mjx_mod.hpr_plan_indices(layout["edges"], G * N, D)[1], layout["nbrs"])


def test_reverse_of_row_r_is_r_plus_E_tot(layout):
    Et = layout["E_tot"]
    out, inn = layout["out_row"], layout["in_row"]
    # the message a -> k and the message k -> a are each other's reverse
    assert np.array_equal(np.where(out < Et, out + Et, out - Et), inn)
    u, v = layout["edges"][:, 0], layout["edges"][:, 1]
    for r in range(Et):
        a, m = u[r], list(layout["nbrs"][u[r]]).index(v[r])
        assert out[a, m] == r and inn[a, m] == r + Et


def test_explicit_neighbour_arrays_are_kept(mjx_mod, graphs):
    rng = np.random.default_rng(0)
    base = mjx_mod.hpr_batch_layout(graphs, N, D)
    nbrs = [rng.permuted(base["nbrs"][g * N:(g + 1) * N] - g * N, axis=1) for g in range(G)]
    lay = mjx_mod.hpr_batch_layout(graphs, N, D, nbrs)
    for g in range(G):
        assert np.array_equal(lay["nbrs"][g * N:(g + 1) * N] - g * N, nbrs[g])
        out, inn = numpy_rows(graphs[g], N, nbrs[g])
        assert np.array_equal(lay["out_row"][g * N:(g + 1) * N], lay["rows"][g][out])
        assert np.array_equal(lay["in_row"][g * N:(g + 1) * N], lay["rows"][g][inn])


def test_bad_batches_raise(mjx_mod, graphs):
    with pytest.raises(ValueError):
        mjx_mod.hpr_batch_layout([], N, D)
    with pytest.raises(ValueError):                             # another n
        mjx_mod.hpr_batch_layout(graphs[:2] + [mjx_mod.random_regular_edges(D, N + 2, seed=1)], N, D)
    with pytest.raises(ValueError):                             # another d
        mjx_mod.hpr_batch_layout(graphs[:2] + [mjx_mod.random_regular_edges(D + 1, N, seed=1)], N, D)
    with pytest.raises(ValueError):                             # same edge count, other (n, d)
        mjx_mod.hpr_batch_layout(graphs[:1] + [mjx_mod.random_regular_edges(2, 15, seed=1)], N, D)
    with pytest.raises(ValueError):
        mjx_mod.hpr_batch_layout(graphs, N, D, nbrs_list=[None])


def test_union_beyond_int32_raises(mjx_mod, graphs, monkeypatch):
    """in_row / out_row / nbr are int32 on the device: a union past 2^31 - 1 rows
    is refused (the limit lowered here, the check is the same comparison)."""
    import mjx.hpr_batch as hb
    monkeypatch.setattr(hb, "INT32_MAX", 2 * N * D)
    assert mjx_mod.hpr_batch_layout(graphs[:2], N, D)["G"] == 2
    with pytest.raises(ValueError):
        mjx_mod.hpr_batch_layout(graphs, N, D)
    # the mask generator runs one grid row per instance (65 535 at most)
    monkeypatch.setattr(hb, "INT32_MAX", 2 ** 31 - 1)
    monkeypatch.setattr(hb, "MAX_INSTANCES", 2)
    with pytest.raises(ValueError):
        mjx_mod.hpr_batch_layout(graphs, N, D)
