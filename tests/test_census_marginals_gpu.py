"""``census_marginals`` on the GPU against the brute-force oracle
(tests/census_marginals_oracle.py) -- integer exact, every comparison is
array_equal -- and the cross-check it exists for: BDCM's fixed point on a tree
against the enumeration (``census_boltzmann``), phi, m_init and every node's
magnetisation (``bdcm_node_m_init``)."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import bdcm_cases as bc
import census_marginals_oracle as cmo
import census_oracle as co
from conftest import ROOT
from test_census_gpu import _complete, _csr, _er14, _path, _rrg, _star

pytestmark = pytest.mark.gpu

REGULAR = {f"rrg_d{d}_n{n}": (d, n, 3) for d in (3, 4) for n in (12, 14, 16)}
ER_FOREST_SEED = 117                   # erdos_renyi(16, 0.1, seed): a forest without isolated nodes (asserted)
PC = [(1, 1), (2, 1), (1, 2)]
LAMBDAS = (0.0, 0.5, 1.2)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (kind, arrays, n, T, oracle marginals).  Shared: never written."""
    if name in REGULAR:
        d, n, T = REGULAR[name]
        spec = ("ell", (_rrg(d, n)[0],))
    elif name == "rrg_d3_n12_T6":
        n, T, spec = 12, 6, ("ell", (_rrg(3, 12)[0],))
    elif name == "rrg_d3_n20":
        n, T, spec = 20, 2, ("ell", (_rrg(3, 20)[0],))
    elif name == "rrg_d4_n13":
        import mjx
        n, T, spec = 13, 3, ("ell", (mjx.random_regular_graph(4, 13, seed=2),))
    elif name.startswith("path"):
        n, T = int(name[4:]), 3
        spec = ("csr", _path(n))
    elif name == "lone":
        n, T, spec = 1, 2, ("csr", _csr([[]]))
    elif name == "edge":
        n, T, spec = 2, 2, ("ell", (np.array([[1], [0]]),))
    elif name == "star":
        n, T, spec = 17, 2, ("csr", _star())
    elif name in ("K9", "K8"):
        n, T = int(name[1:]), 2
        spec = ("ell", (_complete(n),))
    elif name == "er14":
        n, T, spec = 14, 3, ("csr", _er14())
    elif name == "tree":
        n, T, spec = 13, 2, ("csr", cmo.recursive_tree(13, 3)[1:])
    elif name == "forest":
        n, T, spec = 16, 2, ("csr", _forest()[1:])
    else:
        raise KeyError(name)
    step = co.step_ell(spec[1][0]) if spec[0] == "ell" else co.step_csr(*spec[1])
    return spec[0], spec[1], n, T, cmo.census(step, n, T)


def _forest():
    """-> (edges u < v, row_ptr, col) of the 16-node Erdos-Renyi forest."""
    import mjx
    rp, col = (np.asarray(a, dtype=np.int64) for a in mjx.erdos_renyi(16, 0.1, seed=ER_FOREST_SEED)[:2])
    u = np.repeat(np.arange(16), np.diff(rp))
    edges = np.stack([u[u < col], col[u < col]], axis=1)
    assert np.diff(rp).min() >= 1, "no isolated node"
    comp = np.arange(16)                                     # acyclic: E = n - components
    for _ in range(16):
        for a, b in edges.tolist():
            comp[a] = comp[b] = min(comp[a], comp[b])
    assert edges.shape[0] == 16 - np.unique(comp).size and np.unique(comp).size >= 2
    return edges, rp, col


def _graph(mjx_mod, name, kind=None):
    k, arrays, _, _, _ = _case(name)
    if (kind or k) == "ell":
        return mjx_mod.Graph.ell(arrays[0])
    if k == "csr":
        return mjx_mod.Graph.csr(*arrays)
    return mjx_mod.Graph.csr(*_csr([list(r) for r in arrays[0].tolist()]))       # an ELL case as CSR


def _assert_marginals(res, want, n, T, levels):
    lv = list(levels)
    assert np.array_equal(res["counts"], want["counts"]) and np.array_equal(res["min_plus"], want["min_plus"])
    assert np.array_equal(res["witness"], want["witness"]) and res["configs"] == 1 << n
    assert res["levels"] == lv
    assert res["node_counts"].dtype == np.int64 and res["node_counts"].shape == (len(lv), n + 1, n)
    assert np.array_equal(res["node_counts"], want["node_counts"][lv])
    assert res["optimal"].dtype == np.int64 and np.array_equal(res["optimal"], want["optimal"][lv])
    for key in ("backbone_plus", "backbone_minus"):
        assert res[key].dtype == np.bool_ and np.array_equal(res[key], want[key][lv]), key


# ---- 1. regular graphs: ELL, the bare array and CSR ---------------------------------------------------------
@pytest.mark.parametrize("name", list(REGULAR))
def test_regular_graphs_equal_the_oracle_as_ell_array_and_csr(mjx_mod, name):
    _, arrays, n, T, want = _case(name)
    nc, counts = want["node_counts"], want["counts"]
    assert ((nc[T] > 0) & (nc[T] < counts[T][:, None])).any(), "degenerate: no node count strictly inside"
    assert want["min_plus"][T] < n
    levels = [0, 1, T]
    ell = mjx_mod.census_marginals(_graph(mjx_mod, name), T, 1, levels=levels)
    _assert_marginals(ell, want, n, T, levels)
    _assert_marginals(mjx_mod.census_marginals(arrays[0], T, 1, levels=levels), want, n, T, levels)
    _assert_marginals(mjx_mod.census_marginals(_graph(mjx_mod, name, "csr"), T, 1, levels=levels), want, n, T, levels)
    plain = mjx_mod.census(_graph(mjx_mod, name), T, 1)
    assert sorted(set(ell) - set(plain)) == ["backbone_minus", "backbone_plus", "levels", "node_counts", "optimal"]
    for key, val in plain.items():
        assert np.array_equal(ell[key], val), key
    # the default level is T
    _assert_marginals(mjx_mod.census_marginals(arrays[0], T, 1), want, n, T, [T])


# ---- 2. the three classes of nodes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lone", "edge", "path5", "path7", "path11"])
def test_pattern_bits_and_lane_bits(mjx_mod, name):
    _, _, n, T, want = _case(name)
    levels = list(range(T + 1))
    _assert_marginals(mjx_mod.census_marginals(_graph(mjx_mod, name), T, 1, levels=levels), want, n, T, levels)
    if name == "lone":                                       # a node of degree 0 keeps its spin
        assert want["node_counts"].tolist() == [[[0], [1]]] * (T + 1)


def test_one_wave_uniform_bit_and_two_rows_per_wave(mjx_mod):
    _, _, n, T, want = _case("rrg_d4_n13")
    assert 1 << (n - 6) == 128 and want["min_plus"][T] < n
    g = _graph(mjx_mod, "rrg_d4_n13")
    for grid in (1, 2, 3):
        _assert_marginals(mjx_mod.census_marginals(g, T, 1, levels=[1, T], kernel={"grid": grid}), want, n, T, [1, T])


def test_eight_wave_uniform_bits(mjx_mod):
    _, _, n, T, want = _case("rrg_d3_n20")
    assert want["min_plus"][T] < n
    g = _graph(mjx_mod, "rrg_d3_n20")
    _assert_marginals(mjx_mod.census_marginals(g, T, 1), want, n, T, [T])
    # rows that do not start at a multiple of 64: every lane adds for its own block
    _assert_marginals(mjx_mod.census_marginals(g, T, 1, chunk_blocks=1000, kernel={"grid": 7}), want, n, T, [T])


# ---- 3. irregular graphs and ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["star", "K9", "K8", "er14"])
def test_degrees_and_ties(mjx_mod, name):
    _, arrays, n, T, want = _case(name)
    levels = list(range(T + 1))
    res = mjx_mod.census_marginals(_graph(mjx_mod, name), T, 1, levels=levels)
    _assert_marginals(res, want, n, T, levels)
    if name == "star":                                       # the isolated node 16 starts +1 in every counted x
        assert res["backbone_plus"][:, 16].all()
        assert np.array_equal(res["node_counts"][:, :, 16], res["counts"])
    if name in ("K9", "K8"):                                 # every 5-subset wins: no node is in the backbone
        assert res["optimal"][1] == (126 if name == "K9" else 56)
        assert not res["backbone_plus"][1].any() and not res["backbone_minus"][1].any()
    if name == "er14":
        iso = np.flatnonzero(np.diff(arrays[0]) == 0)
        assert res["backbone_plus"][:, iso].all()


# ---- 4. range splits and levels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 3, 64, None])
def test_the_result_does_not_depend_on_the_split(mjx_mod, chunk):
    _, _, n, T, want = _case("rrg_d3_n14")                   # 256 blocks: nodes 12 and 13 in rows of every alignment
    res = mjx_mod.census_marginals(_graph(mjx_mod, "rrg_d3_n14"), T, 1, levels=[2, T], chunk_blocks=chunk)
    _assert_marginals(res, want, n, T, [2, T])


GUARD = 0x5A5A5A5A5A5A


def _abi_buffers(T, n, dev, pad=8):
    """counts, keys, node counts and flag in the middle of guarded allocations -> (buffers, pointers, pad)."""
    sizes = ((T + 1) * (n + 1), T + 1, (n + 1) * n)
    bufs = [torch.full((s + 2 * pad,), GUARD, dtype=torch.int64, device=dev) for s in sizes]
    bufs.append(torch.full((1 + 2 * pad,), 0x5A5A, dtype=torch.int32, device=dev))
    for b, fill in zip(bufs, (0, -1, 0, 0)):
        b[pad:-pad] = fill
    return bufs, [b.data_ptr() + b.element_size() * pad for b in bufs], pad


def _guards_intact(bufs, pad):
    return all(bool((b[:pad] == v).all()) and bool((b[-pad:] == v).all())
               for b, v in zip(bufs, (GUARD, GUARD, GUARD, 0x5A5A)))


def test_two_calls_into_the_same_buffers_equal_one(mjx_mod):
    _, arrays, n, T, want = _case("rrg_d4_n16")
    g = mjx_mod.Graph.ell(arrays[0])
    lib = mjx_mod.load_library()
    B = 1 << (n - 6)
    bufs, (cp, kp, np_, fp), pad = _abi_buffers(T, n, g.adj.device)
    for lo, hi in ((0, B // 3), (B // 3, B)):
        assert lib.mjx_census_nodes_ell(g.adj.data_ptr(), n, 4, T, 1, 2, lo, hi, 0, cp, kp, np_, fp, None) == 0
    torch.cuda.synchronize()
    assert int(bufs[3][pad]) == 0 and _guards_intact(bufs, pad)
    assert np.array_equal(bufs[0][pad:-pad].cpu().numpy().reshape(T + 1, n + 1), want["counts"])
    assert np.array_equal(bufs[1][pad:-pad].cpu().numpy(), (want["min_plus"] << 48) | want["witness_x"])
    assert np.array_equal(bufs[2][pad:-pad].cpu().numpy().reshape(n + 1, n), want["node_counts"][2])
    # the first part alone counts less
    bufs2, (cp, kp, np_, fp), _ = _abi_buffers(T, n, g.adj.device)
    assert lib.mjx_census_nodes_ell(g.adj.data_ptr(), n, 4, T, 1, 2, 0, B // 3, 0, cp, kp, np_, fp, None) == 0
    torch.cuda.synchronize()
    part = bufs2[2][pad:-pad].cpu().numpy().reshape(n + 1, n)
    assert (part <= want["node_counts"][2]).all() and 0 < part.sum() < want["node_counts"][2].sum()
    assert _guards_intact(bufs2, pad)


def test_T6_at_level_6_and_T7(mjx_mod):
    _, _, n, T, want = _case("rrg_d3_n12_T6")
    assert T == 6
    g = _graph(mjx_mod, "rrg_d3_n12_T6")
    _assert_marginals(mjx_mod.census_marginals(g, 6, 1, levels=[6, 0, 3]), want, n, 6, [6, 0, 3])
    _assert_marginals(mjx_mod.census_marginals(g, 5, 2), want, n, 6, [6])
    for p, c in ((7, 1), (6, 2)):
        with pytest.raises(ValueError):
            mjx_mod.census_marginals(g, p, c)
    with pytest.raises(ValueError, match="level 7"):
        mjx_mod.census_marginals(g, 6, 1, levels=[7])


# ---- 5. a bad adjacency through the ABI -----------------------------------------------------------------------------------
def test_a_bad_adjacency_raises_the_flag_and_counts_nothing(mjx_mod):
    _, arrays, n, T, _ = _case("rrg_d3_n12")
    lib = mjx_mod.load_library()

    def void(bufs, pad, flag):
        torch.cuda.synchronize()
        assert int(bufs[3][pad]) == flag and _guards_intact(bufs, pad)
        assert not bufs[0][pad:-pad].any() and bool((bufs[1][pad:-pad] == -1).all()), "a void run writes nothing"
        assert not bufs[2][pad:-pad].any(), "the node cells stay untouched"

    for bad in (n, -1, 255):
        adj = torch.from_numpy(arrays[0].astype(np.int32)).cuda()
        adj[5, 1] = bad
        bufs, (cp, kp, np_, fp), pad = _abi_buffers(T, n, adj.device)
        assert lib.mjx_census_nodes_ell(adj.data_ptr(), n, 3, T, 1, T, 0, 64, 0, cp, kp, np_, fp, None) == 0
        void(bufs, pad, 2)
    rpt = torch.from_numpy(np.concatenate([[0], np.full(n, 48)]).astype(np.int64)).cuda()      # a row of 48
    colt = torch.zeros(48, dtype=torch.int32, device="cuda")
    bufs, (cp, kp, np_, fp), pad = _abi_buffers(T, n, rpt.device)
    assert lib.mjx_census_nodes_csr(rpt.data_ptr(), colt.data_ptr(), n, T, 1, T, 0, 64, 0, cp, kp, np_, fp, None) == 0
    void(bufs, pad, 4)


# ---- 6. the backbone against the solvers ------------------------------------------------------------------------------------
def test_every_optimal_quench_result_respects_the_backbone(mjx_mod):
    _, arrays, n, T, want = _case("rrg_d3_n16")
    res = mjx_mod.census_marginals(arrays[0], T, 1)
    plus, minus = res["backbone_plus"][0], res["backbone_minus"][0]
    q = mjx_mod.quench_restarts(arrays[0], np.ones(n, np.int8), T, 1, restarts=256, seed=0, keep_all=True)
    conf = np.asarray(q["conf"]).reshape(-1, n)
    optimal = conf[(conf == 1).sum(axis=1) == res["min_plus"][T]]
    assert optimal.shape[0] > 0, "no restart reached the optimum: the test would show nothing"
    assert (np.asarray(mjx_mod.s_endstate(arrays[0], optimal.astype(np.int64), T, 1)).reshape(-1, n) == 1).all()
    assert (optimal[:, plus] == 1).all() and (optimal[:, minus] == -1).all()
    print(f"backbone: {plus.sum()} nodes +1, {minus.sum()} nodes -1 of {n}; {optimal.shape[0]} of {conf.shape[0]} "
          f"restarts optimal, {np.unique(optimal, axis=0).shape[0]} of the {res['optimal'][0]} optima")


# ---- 7. BDCM against the enumeration -----------------------------------------------------------------------------------------
def _dev(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def _bdcm_fixed_point(mjx_mod, plan, p, c, lam, seed, T_max=2000):
    chi = _dev(bc.random_chi(2 * plan.E, p + c, seed))
    mjx_mod.bdcm_leaf_reset(chi, plan, p, c, 1, lam)
    t, delta = mjx_mod.bdcm_converge(chi, plan, p, c, 1, lam, 0.5, 1e-14, T_max)
    return chi, t, delta


@pytest.mark.parametrize("name", ["tree", "forest"])
def test_bdcm_on_a_tree_equals_the_enumeration(mjx_mod, name):
    """The bar is 1e-10: the kernels' per-entry bar of 1e-12 with two decades for the sums and logs over at
    most 2 (n - 1) edge terms.  BDCM at (p, c) is level t = p of the census."""
    _, (rp, col), n, T, want = _case(name)
    edges = cmo.recursive_tree(13, 3)[0] if name == "tree" else _forest()[0]
    plan = mjx_mod.BDCMPlan(edges, rp, col, n_total=n, n_iso=0)
    g = mjx_mod.Graph.csr(rp, col)
    worst = 0.0
    for p, c in PC:
        res = mjx_mod.census_marginals(g, p, c, levels=[p])
        assert np.array_equal(res["node_counts"][0], want["node_counts"][p])
        for lam in LAMBDAS:
            exact = mjx_mod.census_boltzmann(res, lam)
            chi, t, _ = _bdcm_fixed_point(mjx_mod, plan, p, c, lam, 10 * p + c)
            assert t < 2000, "not converged"
            phi = mjx_mod.phi_BP_GENERAL_ER(chi, plan, p, c, 1, lam)
            m_init = mjx_mod.avg_m_init_GENERAL_ER(chi, plan, p, c, 1)
            m_node = mjx_mod.bdcm_node_m_init(chi, plan, p, c, 1)
            assert m_node.dtype == torch.float64 and tuple(m_node.shape) == (n,)
            err = (abs(phi - exact["phi"]), abs(m_init - exact["m_init"]),
                   np.abs(m_node.cpu().numpy() - exact["m_node"]).max())
            print(f"{name} (p, c) = ({p}, {c}) lam = {lam}: {t} sweeps, |d phi| = {err[0]:.2g}, |d m_init| = "
                  f"{err[1]:.2g}, max |d m_node| = {err[2]:.2g}")
            worst = max(worst, *err)
            assert max(err) <= 1e-10
    print(f"{name}: largest distance {worst:.3g}")


def test_bp_error_per_node_on_a_loopy_graph(mjx_mod):
    """What the feature exists to show: how far BDCM's node magnetisations are from the exact ones on a graph
    with loops.  No value is asserted."""
    _, arrays, n, _, _ = _case("rrg_d3_n14")
    adj = arrays[0]
    u = np.repeat(np.arange(n), 3)
    v = adj.reshape(-1)
    edges = np.stack([u[u < v], v[u < v]], axis=1)
    plan = mjx_mod.BDCMPlan(edges, *cmo.csr_of(n, edges), n_total=n, n_iso=0)
    p, c, lam = 1, 1, 0.5
    exact = mjx_mod.census_boltzmann(mjx_mod.census_marginals(adj, p, c, levels=[p]), lam)
    chi, t, delta = _bdcm_fixed_point(mjx_mod, plan, p, c, lam, 5, T_max=500)
    m_node = mjx_mod.bdcm_node_m_init(chi, plan, p, c, 1).cpu().numpy()
    assert m_node.shape == (n,) and np.isfinite(m_node).all() and (np.abs(m_node) <= 1).all()
    print(f"loopy rrg d = 3, n = {n}, (p, c) = ({p}, {c}), lam = {lam}: {t} sweeps, delta = {delta:.2g}")
    print("BP m_node - exact m_node:", np.round(m_node - exact["m_node"], 4).tolist())
    print(f"BP phi - exact phi = {mjx_mod.phi_BP_GENERAL_ER(chi, plan, p, c, 1, lam) - exact['phi']:.4g}, "
          f"BP m_init - exact m_init = {mjx_mod.avg_m_init_GENERAL_ER(chi, plan, p, c, 1) - exact['m_init']:.4g}")


@pytest.mark.parametrize("av", [1, -1])
def test_the_node_terms_sum_to_avg_m_init(mjx_mod, av):
    n, edges, rp, col, _ = bc.small_case()
    plan = mjx_mod.BDCMPlan(edges, rp, col, n_total=n + bc.N_ISO, n_iso=bc.N_ISO)
    assert plan.n_iso == 3
    for p, c in ((1, 1), (2, 1), (1, 2), (0, 3)):
        chi = _dev(bc.random_chi(2 * plan.E, p + c, 3 * p + c))              # any messages: an identity of the sums
        m_node = mjx_mod.bdcm_node_m_init(chi, plan, p, c, av)
        assert tuple(m_node.shape) == (plan.n_core,) and bool((m_node.abs() <= 1).all())
        total = (float(m_node.sum()) + av * plan.n_iso) / plan.n
        assert abs(total - mjx_mod.avg_m_init_GENERAL_ER(chi, plan, p, c, av)) <= 1e-13


# ---- 8. CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_census_marginals_in_a_fresh_process(mjx_mod, tmp_path):
    out = tmp_path / "census.npz"
    run = subprocess.run([sys.executable, "-m", "mjx", "census", "--graph", "rrg", "--n", "14", "--d", "3",
                          "--graph-seed", "3", "--p", "2", "--c", "1", "--marginals", "--levels", "0", "2", "--lam",
                          "0", "0.5", "--out", str(out)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    adj = mjx_mod.random_regular_graph(3, 14, seed=3)
    want = cmo.census(co.step_ell(adj), 14, 2)
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["configs", "counts", "edges", "entropy", "m_min", "min_plus", "witness",
                                          "levels", "node_counts", "optimal", "backbone_plus", "backbone_minus", "lam",
                                          "phi", "m_init", "ent1", "p_plus", "m_node"])
        assert z["levels"].tolist() == [0, 2] and z["lam"].tolist() == [0.0, 0.5]
        assert np.array_equal(z["counts"], want["counts"])
        assert np.array_equal(z["node_counts"], want["node_counts"][[0, 2]])
        assert np.array_equal(z["backbone_plus"], want["backbone_plus"][[0, 2]])
        assert z["phi"].shape == (2, 2) and z["p_plus"].shape == (2, 2, 14)
        ref = mjx_mod.census_boltzmann({"counts": want["counts"], "levels": [0, 2],
                                        "node_counts": want["node_counts"][[0, 2]]}, [0.0, 0.5], level=1)
        assert np.array_equal(z["phi"][1], ref["phi"]) and np.array_equal(z["m_node"][1], ref["m_node"])
        assert (z["p_plus"][0] == 1).all(), "level 0 is all +1"
