"""Run-to-attractor layer on the GPU against the numpy restatement
(tests/attractor_oracle.py): random starts, the tracked sweeps on every path
(specialised and runtime-degree ELL, CSR with and without a visiting order,
16-byte and 8-byte units), the device bookkeeping, truncation, chunking, the
consensus curve and the CLI.  Integer exact: every comparison is array_equal."""
import functools
import importlib

import numpy as np
import pytest
import torch

import attractor_oracle as ao

pytestmark = pytest.mark.gpu


# ---- random_spins ----------------------------------------------------------
def _probs(R):
    return np.array([0.0, 1.0, 0.5, 0.37], np.float64)[np.arange(R) % 4]


@functools.lru_cache(maxsize=None)
def _spins_gpu(R):
    import mjx
    return mjx.random_spins(1000, R, 2.0 * _probs(R) - 1.0, seed=77).cpu().numpy()


@pytest.mark.parametrize("R", [1, 64, 100, 192])
def test_random_spins_equal_the_numpy_rule(R):
    n = 1000
    got, pad = ao.unpack_rp(_spins_gpu(R), n, R)
    assert not pad, "padding replicas must be 0"
    want = ao.random_spins(n, R, _probs(R), seed=77)
    assert np.array_equal(got, want)
    assert np.all(got[0::4] == -1) and np.all(got[1::4] == 1)


def test_random_spins_do_not_depend_on_R():
    a, _ = ao.unpack_rp(_spins_gpu(192), 1000, 192)
    b, _ = ao.unpack_rp(_spins_gpu(100), 1000, 100)
    assert np.array_equal(a[:100], b)


# ---- attractor on regular graphs -------------------------------------------
@functools.lru_cache(maxsize=None)
def _rrg_case(d, R):
    import mjx
    n = 1234 if d % 2 == 0 else 1236
    adj = mjx.random_regular_graph(d, n, seed=100 + d)
    S0 = 2 * np.random.default_rng(1000 * d + R).integers(0, 2, (R, n)) - 1
    return adj, S0          # shared between tests: never written


@functools.lru_cache(maxsize=None)
def _rrg_oracle(d, R, t_max):
    adj, S0 = _rrg_case(d, R)
    return ao.attractor(ao.step_ell(adj), S0, t_max=t_max, chunk=16)


def _assert_equal(res, want, n, R):
    import mjx
    assert np.array_equal(res["p"], want["p"])
    assert np.array_equal(res["c"], want["c"])
    assert np.array_equal(res["sum_att"], want["sum_att"])
    assert res["t_end"] == want["t_end"]
    assert np.array_equal(mjx.unpack(res["state"], n, R).cpu().numpy(), want["state"])


@pytest.mark.parametrize("R", [64, 100, 192])
@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
def test_attractor_equals_the_oracle_on_regular_graphs(mjx_mod, d, R):
    adj, S0 = _rrg_case(d, R)
    want = _rrg_oracle(d, R, 256)
    assert np.all(want["p"] >= 0), "a replica of the oracle did not settle"
    if d >= 4:
        assert (want["c"] == 1).any() and (want["c"] == 2).any(), "the case lost a cycle type"
    res = mjx_mod.attractor(adj, S0, t_max=256)
    _assert_equal(res, want, adj.shape[0], R)
    assert isinstance(res["p"], np.ndarray)


def test_attractor_truncates_at_the_budget(mjx_mod):
    adj, S0 = _rrg_case(4, 192)
    want = _rrg_oracle(4, 192, 8)
    assert (want["p"] == -1).any() and (want["p"] >= 0).any()
    assert np.all(want["c"][want["p"] == -1] == 0)
    res = mjx_mod.attractor(adj, S0, t_max=8)
    _assert_equal(res, want, adj.shape[0], 192)
    assert res["t_end"] == 10


def test_attractor_does_not_depend_on_the_chunk_and_keeps_its_input(mjx_mod):
    adj, S0 = _rrg_case(4, 192)
    want = _rrg_oracle(4, 192, 256)
    dev = torch.from_numpy(np.array(S0)).cuda()
    keep = dev.clone()
    bits = mjx_mod.pack(dev)
    keep_bits = bits.clone()
    for chunk in (1, 2, 16):
        res = mjx_mod.attractor(adj, dev, t_max=256, chunk=chunk)
        for key in ("p", "c", "sum_att"):
            assert res[key].is_cuda and np.array_equal(res[key].cpu().numpy(), want[key]), (chunk, key)
        packed = mjx_mod.attractor(adj, bits, t_max=256, chunk=chunk, words=3)
        for key in ("p", "c", "sum_att"):
            assert np.array_equal(packed[key].cpu().numpy(), want[key]), (chunk, key)
    assert torch.equal(dev, keep) and torch.equal(bits, keep_bits)
    one = mjx_mod.attractor(adj, np.array(S0[5]), t_max=256)            # a single (n,) vector
    assert one["p"].tolist() == [want["p"][5]] and one["c"].tolist() == [want["c"][5]]


@pytest.mark.parametrize("d,W", [(3, 1026), (5, 1025)])
def test_attractor_with_more_flag_words_than_fit_in_lds(mjx_mod, d, W):
    """Above 1024 words per node the flag words are ORed into global memory by
    the threads themselves (each thread of a block owns another unit) and the
    fused counts bypass LDS: 16-byte units on the specialised path, 8-byte
    units on the runtime-degree path.  Few nodes keep the oracle quick."""
    n, R = 24, 64 * W
    adj = mjx_mod.random_regular_graph(d, n, seed=d)
    bits = mjx_mod.random_spins(n, R, 0.0, seed=W)
    S0, _ = ao.unpack_rp(bits.cpu().numpy(), n, R)
    want = ao.attractor(ao.step_ell(adj), S0, t_max=64)
    assert np.all(want["p"] >= 0) and len(np.unique(want["p"])) > 2
    res = mjx_mod.attractor(adj, bits, t_max=64, words=W)
    for key in ("p", "c", "sum_att"):
        assert np.array_equal(res[key].cpu().numpy(), want[key]), key
    assert res["t_end"] == want["t_end"]
    got, _ = ao.unpack_rp(res["state"].cpu().numpy(), n, R)
    assert np.array_equal(got, want["state"])


# ---- CSR -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hub_case():
    import mjx
    n = 3000
    rng = np.random.default_rng(0)
    u = rng.integers(0, n, 6000)
    v = rng.integers(0, n, 6000)
    keep = u != v
    u, v = u[keep], v[keep]
    hub_u = np.zeros(200, np.int64) + 7
    hub_v = rng.choice(np.arange(8, n), 200, replace=False)
    key = np.unique(np.minimum(np.r_[u, hub_u], np.r_[v, hub_v]) * n + np.maximum(np.r_[u, hub_u], np.r_[v, hub_v]))
    rp, col = mjx.csr_from_edges(n, key // n, key % n)
    S0 = 2 * rng.integers(0, 2, size=(130, n)).astype(np.int64) - 1
    want = ao.attractor(ao.step_csr(rp, col), S0, t_max=512, chunk=16)
    return rp, col, S0, want


def test_attractor_on_csr_with_a_hub_and_isolated_nodes(mjx_mod):
    rp, col, S0, want = _hub_case()
    deg = np.diff(rp)
    assert (deg == 0).any() and deg.max() >= 200
    assert np.all(want["p"] >= 0)
    g = mjx_mod.Graph.csr(rp, col)
    assert g.order is not None                                        # degree-sorted visiting order
    res = mjx_mod.attractor(g, S0, t_max=512)
    _assert_equal(res, want, g.n, 130)
    plain = mjx_mod.Graph("csr", g.n, row_ptr=g.row_ptr, col=g.col, order=None)
    res2 = mjx_mod.attractor(plain, S0, t_max=512)
    _assert_equal(res2, want, g.n, 130)


# ---- raw entry point -------------------------------------------------------
@pytest.mark.parametrize("d,R", [(4, 192), (4, 128), (5, 128), (5, 64)])
def test_tracked_sweep_ping_pong_aliasing_and_null_prev(mjx_mod, d, R):
    """One mjx_sweep_track_ell_rp call with s_out aliasing s_prev gives the same
    s_out, counts and diff as with a separate s_out; s_prev = NULL leaves the
    second diff half untouched.  (d, R): specialised and runtime degree, 16-byte
    (even W) and 8-byte (odd W) units."""
    from mjx import _lib as L, _device as D
    adj, S0 = _rrg_case(d, 192)
    S0 = np.array(S0[:R])
    n, W = adj.shape[0], (R + 63) // 64
    g = mjx_mod.as_graph(adj)
    st = D.stream_handle()
    s0 = mjx_mod.pack(torch.from_numpy(S0).cuda())
    s1 = mjx_mod.rollout(g, s0, 1, words=W)

    def sweep(s_in, s_prev, s_out, fill=0):
        counts = torch.zeros(64 * W, dtype=torch.int64, device="cuda")
        diff = torch.full((2 * W,), fill, dtype=torch.int64, device="cuda")
        L.call("mjx_sweep_track_ell_rp", D.ptr(g.adj), n, d, W, D.ptr(s_in), D.ptr(s_prev), D.ptr(s_out),
               D.ptr(counts), D.ptr(diff), st)
        return counts.cpu().numpy(), diff.cpu().numpy()

    sep = torch.empty_like(s0)
    cnt_a, diff_a = sweep(s1, s0, sep)
    alias = s0.clone()
    cnt_b, diff_b = sweep(s1, alias, alias)
    assert torch.equal(sep, alias) and np.array_equal(cnt_a, cnt_b) and np.array_equal(diff_a, diff_b)
    # against the oracle's states
    step = ao.step_ell(adj)
    o1 = step(S0)
    o2 = step(o1)
    assert np.array_equal(mjx_mod.unpack(sep, n, R).cpu().numpy(), o2)
    assert np.array_equal(cnt_a[:R], (o2 == 1).sum(axis=1)) and not cnt_a[R:].any()
    flags, pad = ao.unpack_rp(diff_a, 2, R)                          # rows: != s_in, != s_prev
    assert not pad, "padding replicas set a flag"
    assert np.array_equal(flags[:, 0] == 1, (o2 != o1).any(axis=1))
    assert np.array_equal(flags[:, 1] == 1, (o2 != S0).any(axis=1))
    # no s_prev: the second half keeps what it held, the first is ORed into
    out = torch.empty_like(s0)
    _, diff_c = sweep(s1, None, out, fill=0x5A5A)
    assert torch.equal(out, sep)
    assert np.array_equal(diff_c[W:], np.full(W, 0x5A5A)) and np.array_equal(diff_c[:W], diff_a[:W] | 0x5A5A)
    # without counts
    diff = torch.zeros(2 * W, dtype=torch.int64, device="cuda")
    L.call("mjx_sweep_track_ell_rp", D.ptr(g.adj), n, d, W, D.ptr(s1), D.ptr(s0), D.ptr(out), None, D.ptr(diff), st)
    assert torch.equal(out, sep) and np.array_equal(diff.cpu().numpy(), diff_a)


# ---- consensus_curve and the CLI -------------------------------------------
def test_consensus_curve_counts_equal_the_oracle_on_its_own_starts(mjx_mod):
    d, n, K = 5, 1236, 64
    m_inits = (0.0, 0.1, 0.3)
    adj = mjx_mod.random_regular_graph(d, n, seed=105)
    cur = mjx_mod.consensus_curve(adj, m_inits, K, seed=4, t_max=256)
    bits = mjx_mod.random_spins(n, 3 * K, np.repeat(m_inits, K), seed=4)
    S0, pad = ao.unpack_rp(bits.cpu().numpy(), n, 3 * K)
    assert not pad
    want = ao.attractor(ao.step_ell(adj), S0, t_max=256)
    p, c, sa = want["p"].reshape(3, K), want["c"].reshape(3, K), want["sum_att"].reshape(3, K, 2)
    assert np.array_equal(cur["consensus"], ((c == 1) & (sa[..., 0] == n)).sum(axis=1))
    assert np.array_equal(cur["c1"], (c == 1).sum(axis=1)) and np.array_equal(cur["c2"], (c == 2).sum(axis=1))
    assert np.array_equal(cur["unsettled"], (p < 0).sum(axis=1))
    assert np.array_equal(cur["p"], p) and np.array_equal(cur["sum_att"], sa)
    assert np.array_equal(cur["init_plus"], (S0 == 1).sum(axis=1).reshape(3, K))
    assert all(cur[k].dtype == np.int64 for k in ("consensus", "c1", "c2", "unsettled"))
    assert cur["consensus"][2] > cur["consensus"][0]                  # m_init = 0.3 reaches consensus more often


@pytest.mark.parametrize("graph", [("rrg", "--d", "3"), ("er", "--deg", "3.0")])
def test_cli_attractor_writes_the_documented_keys(mjx_mod, tmp_path, graph):
    cli = importlib.import_module("mjx.cli")
    out = tmp_path / "att.npz"
    cli.main(["attractor", "--graph", *graph, "--n", "500", "--m-init", "0", "0.4", "--replicas", "64",
              "--seed", "1", "--t-max", "128", "--out", str(out)])
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == ["c", "c1", "c2", "consensus", "init_plus", "m_init", "p", "sum_att", "unsettled"]
        assert z["p"].shape == (2, 64) and z["sum_att"].shape == (2, 64, 2) and z["init_plus"].shape == (2, 64)
        assert np.array_equal(z["c1"] + z["c2"] + z["unsettled"], [64, 64])
        assert np.array_equal(z["m_init"], [0.0, 0.4])
