"""Flip gains and the greedy quench on the GPU against the numpy restatement
(tests/quench_oracle.py: brute-force flips, sequential pass) and against a
device brute force built from ``rollout`` alone.  Integer exact: every
comparison is array_equal."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import quench_oracle as qo
from conftest import ROOT
from quench_cases import R_CASE, TABLE, _case, _graph, hub_graph

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _want_gains(name):
    _, step, S, T = _case(name)
    return qo.flip_gains(step, S, T)


@functools.lru_cache(maxsize=None)
def _want_quench(name, seed):
    _, step, S, T = _case(name)
    order = None if seed is None else np.random.default_rng(seed).permutation(S.shape[1])
    return qo.quench(step, S, T, order)


def _not_degenerate(name):
    """The conditions a case must meet in the oracle before anything is compared."""
    _, _, S, _ = _case(name)
    w = _want_gains(name)
    cons = w["consensus"]
    assert cons.sum() >= 8 and (~cons).sum() >= 8, f"{name}: {cons.sum()} of {cons.size} replicas at consensus"
    plus = (S == 1) & cons[:, None]
    assert (plus & w["removable"]).any() and (plus & ~w["removable"]).any(), f"{name}: removable set degenerate"


def _assert_gains(res, want, S, R=None):
    n = S.shape[1]
    R = S.shape[0] if R is None else R
    assert res["gain"].dtype == np.int32 and res["gain"].shape == (R, n)
    assert np.array_equal(res["gain"], want["gain"][:R])
    assert res["consensus"].dtype == bool and np.array_equal(res["consensus"], want["consensus"][:R])
    mask, pad = qo.unpack_mask(res["removable"].cpu().numpy(), n, R)
    assert not pad, "padding replicas of the removable mask must stay 0"
    assert np.array_equal(mask, want["removable"][:R])
    assert res["n_removable"].dtype == np.int64 and np.array_equal(res["n_removable"], want["n_removable"][:R])


# ---- the table of cases ------------------------------------------------------
@pytest.mark.parametrize("name", TABLE)
def test_flip_gains_equal_the_oracle(mjx_mod, name):
    _not_degenerate(name)
    _, _, S, T = _case(name)
    keep = S.copy()
    res = mjx_mod.flip_gains(_graph(name), S, T, 1)
    _assert_gains(res, _want_gains(name), S)
    assert res["words"] == 2 and np.array_equal(S, keep)
    assert np.all(res["gain"] % 2 == 0) and np.abs(res["gain"]).max() <= 2 * S.shape[1]
    masks = mjx_mod.flip_gains(_graph(name), S, T, 1, gain=False)
    assert masks["gain"] is None
    assert torch.equal(masks["removable"], res["removable"])


@pytest.mark.parametrize("name", TABLE)
def test_gain_equals_a_device_brute_force_from_rollout(mjx_mod, name):
    """The parent's API alone: the n single-flip copies of one replica packed as
    n replicas, ``rollout`` with ``counts``; gain = 2 counts - n - F."""
    _not_degenerate(name)
    _, _, S, T = _case(name)
    g = _graph(name)
    n = S.shape[1]
    gain = mjx_mod.flip_gains(g, S, T, 1)["gain"]
    cons = _want_gains(name)["consensus"]
    W = (n + 63) // 64
    for r in (int(np.flatnonzero(cons)[0]), int(np.flatnonzero(~cons)[0])):
        flips = np.repeat(S[r][None, :], n, axis=0)
        flips[np.arange(n), np.arange(n)] *= -1
        counts = torch.zeros(64 * W, dtype=torch.int64, device="cuda")
        mjx_mod.rollout(g, mjx_mod.pack(flips), T, words=W, counts=counts)
        base = torch.zeros(64, dtype=torch.int64, device="cuda")
        mjx_mod.rollout(g, mjx_mod.pack(S[r][None, :]), T, words=1, counts=base)
        F = 2 * int(base[0].item()) - n
        brute = 2 * counts[:n].cpu().numpy() - n - F
        assert np.array_equal(gain[r], brute), (name, r)


@pytest.mark.parametrize("seed", [None, 3], ids=["identity", "seed3"])
@pytest.mark.parametrize("name", TABLE)
def test_quench_equals_the_sequential_oracle(mjx_mod, name, seed):
    _not_degenerate(name)
    _, _, S, T = _case(name)
    want = _want_quench(name, seed)
    assert want["flipped"].sum() > 0
    g = _graph(name)
    keep = S.copy()
    res = mjx_mod.quench(g, S, T, 1, seed=seed)
    assert np.array_equal(S, keep), "the input was written"
    assert res["conf"].dtype == S.dtype and np.array_equal(res["conf"], want["conf"])
    assert res["flipped"].dtype == np.int64 and np.array_equal(res["flipped"], want["flipped"])
    assert np.array_equal(res["consensus"], want["consensus"])
    assert res["mag"].dtype == np.float64 and np.array_equal(res["mag"], want["conf"].sum(axis=1) / S.shape[1])
    cons = want["consensus"]
    assert np.array_equal(res["conf"][~cons], S[~cons]) and not res["flipped"][~cons].any()
    after = mjx_mod.flip_gains(g, res["conf"], T, 1, gain=False)
    assert not after["n_removable"].any() and not bool(after["removable"].any())
    assert np.array_equal(after["consensus"], cons)
    if seed is not None:        # an explicit order is the same thing
        order = np.random.default_rng(seed).permutation(S.shape[1])
        again = mjx_mod.quench(g, S, T, 1, order=order)
        assert np.array_equal(again["conf"], res["conf"])


def test_tensor_in_tensor_out_and_the_input_buffer_is_untouched(mjx_mod):
    name = "rrg_d4_n96_T3"
    _, _, S, T = _case(name)
    want = _want_quench(name, None)
    for dtype in (torch.int8, torch.int64):
        s = torch.from_numpy(S).to("cuda", dtype)
        keep = s.clone()
        res = mjx_mod.quench(_graph(name), s, T, 1)
        assert torch.equal(s, keep)
        assert res["conf"].is_cuda and res["conf"].dtype == dtype
        assert np.array_equal(res["conf"].cpu().numpy(), want["conf"])
        assert res["flipped"].is_cuda and np.array_equal(res["flipped"].cpu().numpy(), want["flipped"])
        fg = mjx_mod.flip_gains(_graph(name), s, T, 1)
        assert torch.equal(s, keep) and fg["gain"].is_cuda
        assert np.array_equal(fg["gain"].cpu().numpy(), _want_gains(name)["gain"])
    # an (n,) vector: one replica, the vector's shape back
    r = int(np.flatnonzero(want["consensus"])[0])
    one = mjx_mod.quench(_graph(name), S[r], T, 1)
    assert one["conf"].shape == S[r].shape and np.array_equal(one["conf"], want["conf"][r])
    assert one["flipped"].tolist() == [want["flipped"][r]]


# ---- layout edges --------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 64, 70])
def test_replica_counts_and_padding(mjx_mod, R):
    name = "rrg_d3_n200_T2"
    _, _, S, T = _case(name)
    wg, wq = _want_gains(name), _want_quench(name, 3)
    first = int(np.flatnonzero(wg["consensus"])[0]) if R == 1 else 0     # R = 1: a replica that does something
    sl = slice(first, first + R)
    Ssub = np.ascontiguousarray(S[sl])
    n = S.shape[1]
    sub = {k: v[sl] for k, v in wg.items()}
    assert sub["consensus"].any() and sub["removable"].any()
    _assert_gains(mjx_mod.flip_gains(_graph(name), Ssub, T, 1), sub, Ssub, R)
    res = mjx_mod.quench(_graph(name), Ssub, T, 1, seed=3)
    assert np.array_equal(res["conf"], wq["conf"][sl]) and np.array_equal(res["flipped"], wq["flipped"][sl])
    assert res["words"] == (R + 63) // 64
    conf, pad = qo.unpack_mask(res["state"].cpu().numpy(), n, R)
    assert not pad, "padding replicas of the state must stay 0"
    assert np.array_equal(np.where(conf, 1, -1), wq["conf"][sl])


def test_packed_input_equals_the_spin_path(mjx_mod):
    name = "rrg_d3_n200_T2"
    _, _, S, T = _case(name)
    n = S.shape[1]
    Ssub = np.ascontiguousarray(S[:70])
    bits = mjx_mod.pack(Ssub)                       # 2 words per node, replicas 70..127 are -1
    keep = bits.clone()
    spins = mjx_mod.flip_gains(_graph(name), Ssub, T, 1)
    packed = mjx_mod.flip_gains(_graph(name), bits, T, 1, words=2)
    assert torch.equal(bits, keep) and packed["words"] == 2
    assert torch.equal(packed["removable"], spins["removable"])
    assert packed["gain"].shape == (128, n) and torch.equal(packed["gain"][:70].cpu(), torch.from_numpy(spins["gain"]))
    assert not bool(packed["consensus"][70:].any()) and not bool(packed["n_removable"][70:].any())
    qs = mjx_mod.quench(_graph(name), Ssub, T, 1, seed=3)
    qp = mjx_mod.quench(_graph(name), bits, T, 1, seed=3, words=2)
    assert torch.equal(bits, keep) and "conf" not in qp and qp["words"] == 2
    assert torch.equal(qp["state"], qs["state"])
    assert np.array_equal(mjx_mod.unpack(qp["state"], n, 70).cpu().numpy(), _want_quench(name, 3)["conf"][:70])
    assert np.array_equal(qp["flipped"][:70].cpu().numpy(), qs["flipped"]) and not bool(qp["flipped"][70:].any())


# ---- the scratch path ----------------------------------------------------------
def test_lists_beyond_lds_go_to_scratch_and_nothing_changes(mjx_mod):
    _not_degenerate("hub")
    _, _, S, T = _case("hub")
    lone = hub_graph()[2]
    g = _graph("hub")
    caps = mjx_mod.SAReplicasER.ball_bound(g, T)
    assert caps[T] > 64, "the default LDS part must overflow too"
    lib = mjx_mod.load_library()
    import ctypes
    caps_c = (ctypes.c_int64 * (T + 1))(*caps)
    assert lib.mjx_quench_scratch_bytes(R_CASE, T, caps_c, 4) > lib.mjx_quench_scratch_bytes(R_CASE, T, caps_c, 0) \
        > (1 + 65 * 2) * 8
    want = _want_gains("hub")
    wq = _want_quench("hub", 3)
    for kernel in ({"lds_entries": 4}, None, {"lds_entries": 1}):
        res = mjx_mod.flip_gains(g, S, T, 1, kernel=kernel)
        _assert_gains(res, want, S)
        q = mjx_mod.quench(g, S, T, 1, seed=3, kernel=kernel)
        assert np.array_equal(q["conf"], wq["conf"]) and np.array_equal(q["flipped"], wq["flipped"])
    # the isolated node keeps its spin: where it is +1 it is load-bearing
    cons = want["consensus"]
    assert (S[cons, lone] == 1).all() and cons.any()
    assert not want["removable"][:, lone].any()
    mask, _ = qo.unpack_mask(res["removable"].cpu().numpy(), S.shape[1], R_CASE)
    assert not mask[:, lone].any() and np.all(res["gain"][S[:, lone] == 1, lone] == -2)
    assert np.all(wq["conf"][cons, lone] == 1)


# ---- the ends of the T range ---------------------------------------------------
def test_T0_is_minus_two_s_and_T7_is_refused(mjx_mod):
    name = "rrg_d4_n200_T1"
    _, _, S, _ = _case(name)
    S = S.copy()
    S[5] = 1                                        # T = 0: consensus means all +1 already
    res = mjx_mod.flip_gains(_graph(name), S, 1, 0)
    assert np.array_equal(res["gain"], -2 * S)
    assert not bool(res["removable"].any()) and not res["n_removable"].any()
    assert np.array_equal(res["consensus"], (S == 1).all(axis=1)) and res["consensus"][5]
    q = mjx_mod.quench(_graph(name), S, 1, 0)
    assert np.array_equal(q["conf"], S) and not q["flipped"].any()
    for p, c in ((7, 1), (6, 2), (4, 4)):
        with pytest.raises(ValueError):
            mjx_mod.flip_gains(_graph(name), S, p, c)
        with pytest.raises(ValueError):
            mjx_mod.quench(_graph(name), S, p, c)


def test_T6_against_the_oracle(mjx_mod):
    name = "rrg_d3_n64_T6"
    _not_degenerate(name)
    _, _, S, T = _case(name)
    assert T == 6
    _assert_gains(mjx_mod.flip_gains(_graph(name), S, 6, 1), _want_gains(name), S)
    for seed in (None, 3):
        want = _want_quench(name, seed)
        res = mjx_mod.quench(_graph(name), S, 5, 2, seed=seed)          # p + c - 1 = 6 again
        assert np.array_equal(res["conf"], want["conf"]) and np.array_equal(res["flipped"], want["flipped"])


def test_an_asymmetric_graph_is_refused(mjx_mod):
    adj = mjx_mod.random_regular_graph(3, 20, seed=0).copy()
    a, b = (adj[0, 0], adj[1, 0]) if adj[0, 0] != adj[1, 0] else (adj[0, 0], adj[1, 1])
    adj[0, 0], adj[1, 0] = b, a
    with pytest.raises(ValueError, match="symmetric"):
        mjx_mod.flip_gains(adj, np.ones(20, np.int64), 1, 1)


# ---- CLI -------------------------------------------------------------------------
def test_cli_quenches_result_files_in_a_fresh_process(mjx_mod, tmp_path):
    # an SA / HPR shaped file: one graph per replica, conf as floats
    n, d, T = 96, 4, 3
    graphs = np.stack([mjx_mod.random_regular_graph(d, n, seed=40 + k) for k in range(4)])
    conf = qo.random_starts(4, n, 0.7, seed=41).astype(np.float64)
    conf[3] = 1.0
    f1 = tmp_path / "sa.npz"
    np.savez(f1, conf=conf, graphs=graphs.astype(np.float64), mag_reached=conf.mean(axis=1))
    # an sa-er shaped file: one graph for all replicas
    _, _, S, T2 = _case("er_n300_deg3_T2")
    spec = _case("er_n300_deg3_T2")[0]
    f2 = tmp_path / "er.npz"
    np.savez(f2, conf=S[:40].astype(np.float64), row_ptr=spec[1], col=spec[2], n_iso=np.int64(0))
    for f, p in ((f1, T), (f2, T2)):
        run = subprocess.run([sys.executable, "-m", "mjx", "quench", "--in", str(f), "--p", str(p), "--c", "1",
                              "--order-seed", "3", "--out", str(f) + ".out.npz"],
                             capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert run.returncode == 0, run.stderr[-2000:]
    with np.load(str(f1) + ".out.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["conf", "conf_quenched", "consensus", "flipped", "graphs", "mag_quenched",
                                   "mag_reached"]
        assert np.array_equal(z["conf"], conf) and z["conf_quenched"].dtype == np.float64
        assert z["consensus"][3] and z["flipped"][3] > 0
        for k in range(4):
            want = mjx_mod.quench(graphs[k], conf[k].astype(np.int64), T, 1, seed=3)
            assert np.array_equal(z["conf_quenched"][k], want["conf"])
            assert z["flipped"][k] == want["flipped"][0] and z["mag_quenched"][k] == want["mag"][0]
    with np.load(str(f2) + ".out.npz", allow_pickle=False) as z:
        want = mjx_mod.quench(_graph("er_n300_deg3_T2"), S[:40], T2, 1, seed=3)
        assert np.array_equal(z["conf_quenched"], want["conf"]) and np.array_equal(z["flipped"], want["flipped"])
        assert np.array_equal(z["consensus"], want["consensus"]) and np.array_equal(z["mag_quenched"], want["mag"])
        assert np.array_equal(z["conf_quenched"], _want_quench("er_n300_deg3_T2", 3)["conf"][:40])
        assert np.array_equal(z["row_ptr"], spec[1])
