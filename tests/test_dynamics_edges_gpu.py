"""Edges of the majority sweeps at small shapes: replica slices, a graph per
replica, the majority threshold at every degree a kernel specialises or
bounds (1..12, around 32/64/128, 254/255), and one-class CSR graphs on the
degree-class layout.  Bit-exact against the numpy oracle and, for the
threshold ladders, the closed form sign(2r - d) / own at a tie.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import majority as orc

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _init_counts(W):
    return torch.arange(64 * W, dtype=torch.int64, device="cuda") * 5 + 2


def _plus(S):
    return torch.from_numpy((S > 0).sum(axis=1).astype(np.int64)).cuda()


# ---------------------------------------------------------------------------
# 1. rollout(..., slices=S): mjx_rollout_ell_rp_sliced with unit0 != 0
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rrg_states(d, R, T=3):
    """(adj, [s(0), ..., s(T)]) of R random replicas on a d-regular graph, by the oracle."""
    import mjx
    n = 1236
    adj = mjx.random_regular_graph(d, n, seed=40 + d)
    S = [(2 * np.random.default_rng(1000 * d + R).integers(0, 2, (R, n)) - 1).astype(np.int8)]
    for _ in range(T):
        nxt = np.empty_like(S[-1])
        for r0 in range(0, R, 1024):           # rows are independent: bounds the oracle's (R, n, d) temporary
            nxt[r0:r0 + 1024] = orc.s_endstate_batch(adj, S[-1][r0:r0 + 1024], 1, 1)
        S.append(nxt)
    return adj, S


def _sliced_equals_whole_and_oracle(mjx_mod, d, R, slices, steps):
    adj, S = _rrg_states(d, R, max(steps))
    g = mjx_mod.as_graph(adj)
    W = (R + 63) // 64
    bits = mjx_mod.pack(_cuda(S[0]))
    for T in steps:
        init = _init_counts(W)
        c1, cs = init.clone(), init.clone()
        whole = mjx_mod.rollout(g, bits, T, words=W, counts=c1, slices=1)
        sliced = mjx_mod.rollout(g, bits, T, words=W, counts=cs, slices=slices)
        assert torch.equal(sliced, whole) and torch.equal(cs, c1), (d, R, slices, T)
        assert torch.equal(sliced, mjx_mod.pack(_cuda(S[T]))), (d, R, slices, T)
        assert torch.equal((cs - init)[:R], _plus(S[T])) and not (cs - init)[R:].any(), (d, R, slices, T)


@pytest.mark.parametrize("d", [3, 4, 5])
@pytest.mark.parametrize("R,slices", [(256, 2), (256, 4), (512, 4), (4096, 8), (4096, 32), (320, 5), (192, 3)])
def test_sliced_rollout(mjx_mod, d, R, slices):
    """Slices of 16-byte units (even W) and of 8-byte units (R = 320, 192: odd
    W), down to one unit a slice; specialised and runtime degree.  S must
    divide the unit count U (include/mjx.h): R = 256 has W = 4, U = 2, so its
    4 slices are refused, for every step count; R = 512 is the smallest even W
    that 4 slices divide."""
    W = (R + 63) // 64
    U = W // 2 if W % 2 == 0 else W
    if U % slices:
        adj, S = _rrg_states(d, R)
        bits = mjx_mod.pack(_cuda(S[0]))
        for T in (1, 2, 3):
            with pytest.raises(mjx_mod.MjxError, match="invalid argument"):
                mjx_mod.rollout(mjx_mod.as_graph(adj), bits, T, words=W, slices=slices)
        return
    _sliced_equals_whole_and_oracle(mjx_mod, d, R, slices, (1, 2, 3))


def test_sliced_rollout_counters_fit_lds_only_per_slice(mjx_mod):
    """R = 16384: the whole row's counters bypass LDS, a half's fit."""
    _sliced_equals_whole_and_oracle(mjx_mod, 4, 16384, 2, (2,))


def test_sliced_rollout_arguments(mjx_mod):
    adj, S = _rrg_states(4, 256)
    g = mjx_mod.as_graph(adj)
    bits = mjx_mod.pack(_cuda(S[0]))
    for slices in (3, 5, 64):                  # W = 4: two units
        with pytest.raises(mjx_mod.MjxError, match="invalid argument"):
            mjx_mod.rollout(g, bits, 1, words=4, slices=slices)
    # steps = 0: a copy and a popcount
    init = _init_counts(4)
    cnt = init.clone()
    out = mjx_mod.rollout(g, bits, 0, words=4, counts=cnt, slices=2)
    assert out.data_ptr() != bits.data_ptr() and torch.equal(out, bits)
    assert torch.equal(cnt - init, _plus(S[0]))


# ---------------------------------------------------------------------------
# 2. mjx_rollout_ell_rp_multi: a graph per replica
# ---------------------------------------------------------------------------
G = 5


def _multi_call(mjx_mod, adj, n, d, R, rep, s_in, s_out, tmp, steps, counts):
    from mjx import _device as D
    return mjx_mod.load_library().mjx_rollout_ell_rp_multi(
        D.ptr(adj), n, d, R, D.ptr(rep), D.ptr(s_in), D.ptr(s_out), D.ptr(tmp), steps, D.ptr(counts),
        D.stream_handle())


@pytest.mark.parametrize("n", [64, 2002])
@pytest.mark.parametrize("d", [3, 4, 6, 5])
def test_graph_per_replica_equals_the_oracle_on_each_graph(mjx_mod, d, n):
    adjs = np.stack([mjx_mod.random_regular_graph(d, n, seed=7 * d + k) for k in range(G)])
    adj = _cuda(adjs.astype(np.int32))
    rng = np.random.default_rng(n + d)
    for R in (1, 64, 100, 200):
        W = (R + 63) // 64
        rep = rng.integers(0, G, R).astype(np.int32)
        if R == 1:
            rep[:] = 3
        else:
            rep[:4] = (4, 1, 1, 0)             # not monotone, with repeats
        S0 = 2 * rng.integers(0, 2, (R, n)).astype(np.int64) - 1
        bits = mjx_mod.pack(_cuda(S0))
        rep_dev = _cuda(rep)
        want = S0
        for T in (1, 2, 3):
            nxt = np.empty_like(want)
            for k in range(G):                  # each replica on ITS graph
                rows = np.flatnonzero(rep == k)
                if rows.size:
                    nxt[rows] = orc.s_endstate_batch(adjs[k], want[rows], 1, 1)
            want = nxt
            want_bits = mjx_mod.pack(_cuda(want))
            out, tmp = torch.empty_like(bits), torch.empty_like(bits)
            assert _multi_call(mjx_mod, adj, n, d, R, rep_dev, bits, out, tmp, T, None) == 0
            assert torch.equal(out, want_bits), (R, T)
            cnt = torch.full((64 * W + 3,), 77, dtype=torch.int64, device="cuda")
            out2 = torch.empty_like(bits)
            assert _multi_call(mjx_mod, adj, n, d, R, rep_dev, bits, out2, tmp, T, cnt) == 0
            assert torch.equal(out2, want_bits), (R, T)
            assert torch.equal(cnt[:R] - 77, _plus(want)), (R, T)
            assert bool((cnt[R:] == 77).all()), (R, T)   # entries past R are not touched


def test_graph_per_replica_arguments(mjx_mod):
    from mjx import _lib as L
    n, d, R = 64, 3, 64
    adj = _cuda(np.stack([mjx_mod.random_regular_graph(d, n, seed=k) for k in range(G)]).astype(np.int32))
    rep = torch.zeros(R, dtype=torch.int32, device="cuda")
    a = torch.zeros(n, dtype=torch.int64, device="cuda")
    b, c = torch.zeros_like(a), torch.zeros_like(a)
    assert _multi_call(mjx_mod, adj, n, d, R, rep, a, b, c, 1, None) == L.MJX_OK
    assert _multi_call(mjx_mod, adj, n, d, R, rep, a, b, c, 0, None) == L.MJX_EINVAL
    assert _multi_call(mjx_mod, adj, n, 0, R, rep, a, b, c, 1, None) == L.MJX_EINVAL
    for (x, y, z) in [(a, a, c), (a, b, a), (a, b, b)]:            # in == out, in == tmp, out == tmp
        assert _multi_call(mjx_mod, adj, n, d, R, rep, x, y, z, 2, None) == L.MJX_EINVAL


# ---------------------------------------------------------------------------
# 3. threshold ladder: the truth table of always-stay majority
# ---------------------------------------------------------------------------
def _ladder(deg, r, own):
    """New spin of a node of degree ``deg`` with r (+1) neighbours, own spin ``own``."""
    s = np.sign(2 * np.minimum(r, deg) - deg)
    return np.where(s == 0, own, s)


def _flag_bits(words, R):
    """(R,) bools from the W flag words of a tracked sweep."""
    w = words.cpu().numpy().astype(np.uint64)
    r = np.arange(R)
    return ((w[r >> 6] >> (r & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


LADDER_D = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 31, 32, 33, 63, 64, 127, 128, 254, 255]


@pytest.mark.parametrize("d", LADDER_D)
def test_threshold_ladder_regular(mjx_mod, d):
    """Disjoint copies of K_{d,d}: a left node sees all d right nodes of its
    copy.  Replica 2r + (own > 0): the first r right nodes +1, the left nodes
    ``own``.  One step: left = sign(2r - d) or own at a tie, right = own.
    (n = 2d * copies is a multiple of 64 for every copy count when 32 | d;
    otherwise the copy count leaves a ragged last word.)"""
    from mjx import _lib as L, _device as D
    copies = max(1, -(-100 // (2 * d)))
    n, R = 2 * d * copies, 2 * (d + 1)
    assert n % 64 or d % 32 == 0
    base = np.repeat(np.arange(copies) * 2 * d, d)                      # first node of each left node's copy
    left = base + np.tile(np.arange(d), copies)
    right = left + d
    adj = np.empty((n, d), dtype=np.int32)
    adj[left] = base[:, None] + d + np.arange(d)[None, :]
    adj[right] = base[:, None] + np.arange(d)[None, :]
    r = np.arange(R) >> 1
    own = 2 * (np.arange(R) & 1) - 1
    S0 = np.empty((R, n), dtype=np.int64)
    S0[:, left] = own[:, None]
    S0[:, right] = np.where(np.tile(np.arange(d), copies)[None, :] < r[:, None], 1, -1)
    want = np.empty_like(S0)
    want[:, left] = _ladder(d, r, own)[:, None]
    want[:, right] = own[:, None]
    for r0 in range(0, R, 64):                                          # bounds the oracle's (R, n, d) temporary
        assert np.array_equal(orc.s_endstate_batch(adj, S0[r0:r0 + 64], 1, 1), want[r0:r0 + 64])
    g = mjx_mod.Graph.ell(adj)
    W = (R + 63) // 64
    s0, want_dev = _cuda(S0), _cuda(want)
    want_bits = mjx_mod.pack(want_dev)
    # node-packed, replica by replica
    got = torch.stack([mjx_mod.s_endstate(g, s0[k], 1, 1) for k in range(R)])
    assert torch.equal(got, want_dev)
    # replica-packed rollout with counts
    bits = mjx_mod.pack(s0)
    init = _init_counts(W)
    cnt = init.clone()
    out = mjx_mod.rollout(g, bits, 1, words=W, counts=cnt)
    assert torch.equal(out, want_bits)
    assert torch.equal((cnt - init)[:R], _plus(want)) and not (cnt - init)[R:].any()
    # tracked sweep
    cnt = init.clone()
    diff = torch.zeros(2 * W, dtype=torch.int64, device="cuda")
    out = torch.empty_like(bits)
    L.call("mjx_sweep_track_ell_rp", D.ptr(g.adj), n, d, W, D.ptr(bits), None, D.ptr(out), D.ptr(cnt), D.ptr(diff),
           D.stream_handle())
    assert torch.equal(out, want_bits)
    assert torch.equal((cnt - init)[:R], _plus(want)) and not (cnt - init)[R:].any()
    assert np.array_equal(_flag_bits(diff[:W], R), (want != S0).any(axis=1)) and not diff[W:].any()


STAR_D = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255]


@functools.lru_cache(maxsize=None)
def _stars():
    """A union of stars with hub degrees STAR_D and a few isolated nodes; R =
    512 replicas 2r + (own > 0): the first r leaves of every star +1, hubs
    ``own``, isolated nodes alternating.  States after 0, 1, 2 steps in closed
    form: a hub follows the ladder, a leaf (degree 1) copies its hub."""
    R = 512
    r = np.arange(R) >> 1
    own = 2 * (np.arange(R) & 1) - 1
    hubs, u, v, pos = [], [], [], 0
    for Dh in STAR_D:
        hubs.append(pos)
        u += [pos] * Dh
        v += list(range(pos + 1, pos + 1 + Dh))
        pos += Dh + 1
    iso = 5 + (0 if (pos + 5) % 64 else 1)
    n = pos + iso
    import mjx
    rp, col = mjx.csr_from_edges(n, np.array(u), np.array(v))
    S = [np.empty((R, n), dtype=np.int64) for _ in range(3)]
    for Dh, h in zip(STAR_D, hubs):
        leaves = np.arange(h + 1, h + 1 + Dh)
        hub1 = _ladder(Dh, r, own)
        S[0][:, h] = own
        S[0][:, leaves] = np.where(np.arange(Dh)[None, :] < r[:, None], 1, -1)
        S[1][:, h] = hub1
        S[1][:, leaves] = own[:, None]
        S[2][:, h] = own                       # all Dh >= 1 leaves hold `own`
        S[2][:, leaves] = hub1[:, None]
    for k in range(3):
        S[k][:, pos:] = (2 * ((np.arange(iso)[None, :] + np.arange(R)[:, None]) & 1) - 1)
    for T in (1, 2):
        assert np.array_equal(orc.s_endstate_er(rp, col, S[0], T, 1), S[T])
    return rp, col, S


def test_threshold_ladder_stars_node_packed(mjx_mod):
    """k_sweep_csr_np (rollout_csr_np), replica by replica, with its count."""
    rp, col, S = _stars()
    g = mjx_mod.Graph.csr(rp, col)
    assert g.n % 64
    s0 = _cuda(S[0])
    for T in (1, 2):
        outs, cnts = [], torch.full((s0.shape[0],), 9, dtype=torch.int64, device="cuda")
        for k in range(s0.shape[0]):
            outs.append(mjx_mod.unpack(mjx_mod.rollout(g, mjx_mod.pack(s0[k]), T, counts=cnts[k:k + 1]), g.n))
        assert torch.equal(torch.stack(outs), _cuda(S[T])), T
        assert torch.equal(cnts - 9, _plus(S[T])), T


@pytest.mark.parametrize("layout", ["class", "csr", "csr_unordered"])
def test_threshold_ladder_stars_replica_packed(mjx_mod, layout):
    """class: k_sweep_cls_rp<D> (D <= 8, first sweep of two), k_sweep_cls_all_rp
    (counting sweep) and k_sweep_cls_gen_rp (the 15 classes above 8); csr:
    k_sweep_gen_rp over row_ptr/col with the degree order and without."""
    rp, col, S = _stars()
    g = mjx_mod.Graph.csr(rp, col)
    if layout == "class":
        degs = g.class_ell()[2][:, 2].tolist()
        assert degs == sorted({0} | set(STAR_D))
    else:
        if layout == "csr_unordered":
            g = mjx_mod.Graph("csr", g.n, row_ptr=g.row_ptr, col=g.col, order=None)
        g.rp_layout = "csr"
    R = S[0].shape[0]
    W = R // 64
    bits = mjx_mod.pack(_cuda(S[0]))
    for T in (1, 2):
        init = _init_counts(W)
        cnt = init.clone()
        out = mjx_mod.rollout(g, bits, T, words=W, counts=cnt)
        assert torch.equal(out, mjx_mod.pack(_cuda(S[T]))), T
        assert torch.equal(cnt - init, _plus(S[T])), T
        assert torch.equal(mjx_mod.rollout(g, bits, T, words=W), out), T


@pytest.mark.parametrize("layout", ["class", "csr"])
@pytest.mark.parametrize("R", [192, 128])
def test_row_tails_above_degree_8(mjx_mod, R, layout):
    """The runtime-degree row body's tail at both unit widths: stars with hub
    degrees 9, 10, 11, 13 (1, 2, 3, 1 neighbours after the four-wide steps)
    and two isolated nodes, W = 3 (8-byte units) and W = 2 (16-byte units), on
    k_sweep_cls_gen_rp (class) and k_sweep_gen_rp (csr), with and without the
    fused count."""
    u, v, pos = [], [], 0
    for Dh in (9, 10, 11, 13):
        u += [pos] * Dh
        v += list(range(pos + 1, pos + 1 + Dh))
        pos += Dh + 1
    n = pos + 2
    rp, col = mjx_mod.csr_from_edges(n, np.array(u), np.array(v))
    g = mjx_mod.Graph.csr(rp, col)
    assert g.class_ell()[2][:, 2].tolist() == [0, 1, 9, 10, 11, 13]
    g.rp_layout = layout
    W = R // 64
    S0 = 2 * np.random.default_rng(R).integers(0, 2, (R, n)).astype(np.int64) - 1
    bits = mjx_mod.pack(_cuda(S0))
    for T in (1, 2):
        want = orc.s_endstate_er(rp, col, S0, T, 1)
        init = _init_counts(W)
        cnt = init.clone()
        out = mjx_mod.rollout(g, bits, T, words=W, counts=cnt)
        assert np.array_equal(mjx_mod.unpack(out, n, R).cpu().numpy(), want), T
        assert torch.equal(cnt - init, _plus(want)), T
        assert torch.equal(mjx_mod.rollout(g, bits, T, words=W), out), T


def test_threshold_ladder_stars_tracked(mjx_mod):
    from mjx import _lib as L, _device as D
    rp, col, S = _stars()
    g = mjx_mod.Graph.csr(rp, col)
    R = S[0].shape[0]
    W = R // 64
    cur = mjx_mod.pack(_cuda(S[0]))
    for T in (1, 2):
        init = _init_counts(W)
        cnt = init.clone()
        diff = torch.zeros(2 * W, dtype=torch.int64, device="cuda")
        out = torch.empty_like(cur)
        L.call("mjx_sweep_track_csr_rp", D.ptr(g.row_ptr), D.ptr(g.col), D.ptr(g.order), g.n, W, D.ptr(cur), None,
               D.ptr(out), D.ptr(cnt), D.ptr(diff), D.stream_handle())
        assert torch.equal(out, mjx_mod.pack(_cuda(S[T]))), T
        assert torch.equal(cnt - init, _plus(S[T])), T
        assert np.array_equal(_flag_bits(diff[:W], R), (S[T] != S[T - 1]).any(axis=1)) and not diff[W:].any(), T
        cur = out


def test_csr_row_of_256_is_rejected(mjx_mod):
    def star(Dh):
        return mjx_mod.csr_from_edges(Dh + 1, np.zeros(Dh, np.int64), np.arange(1, Dh + 1))
    rp, col = star(255)
    assert mjx_mod.Graph.csr(rp, col).n == 256
    assert mjx_mod.Graph.csr_device(_cuda(rp), _cuda(col)).n == 256
    rp, col = star(256)
    with pytest.raises(ValueError, match="longer than 255"):
        mjx_mod.Graph.csr(rp, col)
    with pytest.raises(ValueError, match="longer than 255"):
        mjx_mod.Graph.csr(torch.from_numpy(rp), torch.from_numpy(col))
    with pytest.raises(ValueError, match="longer than 255"):
        mjx_mod.Graph.csr_device(_cuda(rp), _cuda(col))


# ---------------------------------------------------------------------------
# 4. one degree class: the per-class counting launch k_sweep_cls_rp<D, VW, true>
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [64, 192])
@pytest.mark.parametrize("d", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_one_class_csr_on_the_class_layout(mjx_mod, d, R):
    n = 1234 if d % 2 == 0 else 1236
    W = (R + 63) // 64
    rng = np.random.default_rng(100 * d + R)
    S0 = 2 * rng.integers(0, 2, (R, n)).astype(np.int64) - 1
    if d:
        adj = mjx_mod.random_regular_graph(d, n, seed=60 + d)
        rp, col = np.arange(n + 1, dtype=np.int64) * d, adj.reshape(-1)
        ell = mjx_mod.Graph.ell(adj)
    else:
        rp, col = np.zeros(n + 1, np.int64), np.zeros(0, np.int32)
    g = mjx_mod.Graph.csr(rp, col)
    assert g.rp_layout == "class" and g.class_ell()[2][:, 1:3].tolist() == [[n, d]]
    bits = mjx_mod.pack(_cuda(S0))
    for T in (1, 2, 3):
        want = orc.s_endstate_batch(adj, S0, T, 1) if d else S0
        assert np.array_equal(orc.s_endstate_er(rp, col, S0, T, 1), want)
        init = _init_counts(W)
        cnt = init.clone()
        out = mjx_mod.rollout(g, bits, T, words=W, counts=cnt)
        assert torch.equal(out, mjx_mod.pack(_cuda(want))), T
        assert torch.equal((cnt - init)[:R], _plus(want)) and not (cnt - init)[R:].any(), T
        if d:
            ce = init.clone()
            assert torch.equal(mjx_mod.rollout(ell, bits, T, words=W, counts=ce), out) and torch.equal(ce, cnt), T
