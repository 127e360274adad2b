"""``census_minima`` on the GPU against the brute-force oracle
(tests/census_minima_oracle.py): the minima of every level by weight, the
heaviest minimum, the bitmap, and the census keys.  Integer exact: every
comparison is array_equal."""
import functools
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import census_minima_oracle as cm
import census_oracle as co
from conftest import ROOT
from test_census_gpu import _complete, _csr, _er14, _path, _ring, _rrg, _star

pytestmark = pytest.mark.gpu

# d, n of the random regular cases (T = 3)
REGULAR = {"rrg_d3_n10": (3, 10), "rrg_d3_n12": (3, 12), "rrg_d4_n14": (4, 14), "rrg_d4_n16": (4, 16),
           "rrg_d3_n18": (3, 18)}
# minima[3] of networkx.random_regular_graph(d, n, seed=1), rows sorted, from the first weight that has one;
# checked only when the graph comes from there
QUOTED = {"rrg_d3_n12": (7, [8, 61]), "rrg_d4_n16": (8, [18, 1547, 448, 2]), "rrg_d3_n18": (10, [2, 247, 490])}
ZONES = ["lone", "edge", "path3", "path5", "ring6", "path7", "rrg_d3_n10", "path11", "rrg_d3_n12", "rrg_d4_n13",
         "rrg_d4_n14", "rrg_d4_n16", "rrg_d3_n18"]
RULES = ["star", "K9", "er14", "rrg_d3_n12_T0", "rrg_d3_n12_T6"]
# the graphs too small or too symmetric for minima at two weights in one level (by the oracle): one, two or
# three nodes; the ring of six (nine minima of weight 4); the star, whose minima are the hub, 8 of the 15 leaves
# and the isolated node; K_9, where a level is "at least 5 of 9"; T = 0, where the only minimum is all +1
ONE_WEIGHT = {"lone", "edge", "path3", "ring6", "star", "K9", "rrg_d3_n12_T0"}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (kind, arrays, n, T, oracle).  The oracle dict adds ``min_plus`` and ``witness`` (the census keys)
    to census_minima_oracle.census_minima.  Shared: never written."""
    T = 3
    if name in REGULAR:
        d, n = REGULAR[name]
        spec = ("ell", (_rrg(d, n)[0],))
    elif name == "rrg_d4_n13":
        import mjx
        n = 13                                               # 13 * 3 is odd: d = 4
        spec = ("ell", (mjx.random_regular_graph(4, 13, seed=2),))
    elif name in ("rrg_d3_n12_T0", "rrg_d3_n12_T6"):
        n, T = 12, int(name[-1])
        spec = ("ell", (_rrg(3, 12)[0],))
    elif name.startswith("path"):
        n = int(name[4:])
        spec = ("csr", _path(n))
    elif name.startswith("ring"):
        n = int(name[4:])
        spec = ("ell", (_ring(n),))
    elif name == "lone":
        n, spec = 1, ("csr", _csr([[]]))
    elif name == "edge":
        n, spec = 2, ("ell", (np.array([[1], [0]]),))
    elif name == "star":
        n, spec = 17, ("csr", _star())
    elif name == "K9":
        n, spec = 9, ("ell", (_complete(9),))
    elif name == "er14":
        n, spec = 14, ("csr", _er14())
    else:
        raise KeyError(name)
    step = co.step_ell(spec[1][0]) if spec[0] == "ell" else co.step_csr(*spec[1])
    want = cm.census_minima(step, n, T)
    k = cm.weights(n)
    lightest = []
    for row in want["U"]:
        hit = np.flatnonzero(row)
        lightest.append(int(hit[k[hit] == k[hit].min()][0]))
    want["min_plus"] = np.array([k[x] for x in lightest], np.int64)
    want["witness"] = np.stack([co.spins(x, n) for x in lightest]).astype(np.int8)
    return spec[0], spec[1], n, T, want


def _graph(mjx_mod, name):
    kind, arrays, _, _, _ = _case(name)
    return mjx_mod.Graph.ell(arrays[0]) if kind == "ell" else mjx_mod.Graph.csr(*arrays)


def _pc(T):
    return (T, 1) if T else (1, 0)


def _assert_minima(res, want, n, T):
    # the keys of census
    assert res["counts"].dtype == np.int64 and np.array_equal(res["counts"], want["counts"])
    assert res["min_plus"].dtype == np.int64 and np.array_equal(res["min_plus"], want["min_plus"])
    assert res["witness"].dtype == np.int8 and np.array_equal(res["witness"], want["witness"])
    assert np.array_equal(res["m_min"], (2 * want["min_plus"] - n) / n) and res["configs"] == 1 << n
    with np.errstate(divide="ignore"):
        assert np.array_equal(res["entropy"], np.log(want["counts"].astype(np.float64)) / n)
    # the minima
    assert res["minima"].dtype == np.int64 and res["minima"].shape == (T + 1, n + 1)
    assert np.array_equal(res["minima"], want["minima"])
    assert res["minima_total"].shape == (T + 1,) and np.array_equal(res["minima_total"], want["M"].sum(axis=1))
    assert res["max_plus"].dtype == np.int64 and np.array_equal(res["max_plus"], want["max_plus"])
    assert np.array_equal(res["m_max"], (2 * want["max_plus"] - n) / n)
    assert res["witness_max"].dtype == np.int8 and res["witness_max"].shape == (T + 1, n)
    assert np.array_equal(res["witness_max"], want["witness_max"])
    mean = (want["minima"] * np.arange(n + 1)[None, :]).sum(axis=1) / want["minima"].sum(axis=1)
    assert res["mean_plus"].dtype == np.float64 and np.array_equal(res["mean_plus"], mean)
    # the invariants of include/mjx.h
    rows = np.arange(T + 1)
    assert np.array_equal(res["minima"][rows, res["min_plus"]], res["counts"][rows, res["min_plus"]])
    assert (res["minima"] <= res["counts"]).all() and res["minima"][0].tolist() == [0] * n + [1]
    assert "mask" not in res


# ---- 1. zone edges and rule edges ----------------------------------------------------------------
@pytest.mark.parametrize("name", ZONES + RULES)
def test_every_level_equals_the_oracle(mjx_mod, name):
    _, arrays, n, T, want = _case(name)
    spread = max(int((row > 0).sum()) for row in want["minima"])
    assert (spread == 1) if name in ONE_WEIGHT else (spread >= 2), "minima at two weights, where the graph allows it"
    if name in QUOTED and _rrg(*REGULAR[name])[1]:
        first, tail = QUOTED[name]
        assert want["minima"][3].tolist() == [0] * first + tail + [0] * (n + 1 - first - len(tail))
    res = mjx_mod.census_minima(_graph(mjx_mod, name), *_pc(T))
    _assert_minima(res, want, n, T)
    if name == "star":                                       # the isolated node 16 is in every minimum
        assert want["M"][:, :1 << 16].sum() == 0 and (res["witness_max"][:, 16] == 1).all()
    if name == "er14":
        iso = np.flatnonzero(np.diff(arrays[0]) == 0)
        assert (res["witness_max"][:, iso] == 1).all()
    if name == "K9":                                         # ties keep the spin: the minima are the 5-subsets
        assert res["minima"][1:, 5].tolist() == [126] * T and res["minima_total"][1:].tolist() == [126] * T
    if name == "rrg_d3_n12_T0":
        assert res["minima"].tolist() == [[0] * n + [1]] and res["witness_max"].tolist() == [[1] * n]


# ---- 2. pass 2 alone, on hand-made bitmaps ----------------------------------------------------------
def _pass2(mjx_mod, U, n, ranges=None, grid=0):
    """mjx_census_minima on the words of U bool (L, 2^n) -> (minima (L, n+1), keys uint64 (L,))."""
    lib = mjx_mod.load_library()
    L, B = U.shape[0], 1 << max(n - 6, 0)
    mask = torch.from_numpy(cm.words(U, n).view(np.int64)).cuda()
    minima = torch.zeros((L, n + 1), dtype=torch.int64, device="cuda")
    keys = torch.zeros((L,), dtype=torch.int64, device="cuda")
    for lo, hi in ranges or ((0, B),):
        assert lib.mjx_census_minima(mask.data_ptr(), n, L - 1, lo, hi, grid, minima.data_ptr(), keys.data_ptr(),
                                     None) == 0
    torch.cuda.synchronize()
    return minima.cpu().numpy(), keys.cpu().numpy().view(np.uint64)


def test_pass2_on_hand_made_up_sets(mjx_mod):
    n = 13
    x = np.arange(1 << n, dtype=np.int64)
    nodes = (0, 5, 6, 11, 12)                                # each zone alone, both ends of the middle one
    U = np.stack([((x >> v) & 1).astype(bool) for v in nodes] + [cm.weights(n) >= 5])
    want = cm.census_of(U, n)
    for lv, v in enumerate(nodes):                           # "bit v set": one minimum, x = 1 << v
        assert want["minima"][lv].tolist() == [0, 1] + [0] * (n - 1) and want["heaviest_x"][lv] == 1 << v
    assert want["minima"][5].tolist() == [0] * 5 + [math.comb(13, 5)] + [0] * 8
    for ranges, grid in ((None, 0), (((0, 64), (64, 128)), 0), (None, 1)):
        minima, keys = _pass2(mjx_mod, U, n, ranges, grid)
        assert np.array_equal(minima, want["minima"])
        assert np.array_equal(keys, ((want["max_plus"] << 48) | want["heaviest_x"]).astype(np.uint64))


# ---- 3. geometry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("rrg_d4_n13", {"kernel": {"grid": 1}}), ("rrg_d4_n13", {"kernel": {"grid": 2}}),
                                     ("rrg_d4_n13", {"kernel": {"grid": 3}}), ("rrg_d4_n14", {"kernel": {"grid": 3}}),
                                     ("rrg_d4_n14", {"chunk_blocks": 64}), ("rrg_d4_n14", {"chunk_blocks": 128}),
                                     ("rrg_d4_n14", {"chunk_blocks": 100, "kernel": {"grid": 2}})])
def test_the_result_does_not_depend_on_grid_or_split(mjx_mod, name, kw):
    _, _, n, T, want = _case(name)
    _assert_minima(mjx_mod.census_minima(_graph(mjx_mod, name), T, 1, **kw), want, n, T)


GUARD = 0x5A5A5A5A5A5A


def _guarded(size, fill, dev, pad=8):
    buf = torch.full((size + 2 * pad,), GUARD, dtype=torch.int64, device=dev)
    buf[pad:pad + size] = fill
    return buf


def test_split_ranges_into_guarded_buffers_and_a_mask_that_starts_as_ones(mjx_mod):
    """Pass 1 in three ranges, pass 2 on [0, 64) + [64, 256): the same as one call.  The mask buffer starts
    as all ones: pass 1 writes every word of its range at every level, swept or not."""
    _, arrays, n, T, want = _case("rrg_d4_n14")
    g = mjx_mod.Graph.ell(arrays[0])
    lib = mjx_mod.load_library()
    B, pad, dev = 1 << (n - 6), 8, g.adj.device
    assert B == 256
    cells = (T + 1) * (n + 1)
    cbuf, kbuf = _guarded(cells, 0, dev), _guarded(T + 1, -1, dev)
    mbuf, hbuf = _guarded(cells, 0, dev), _guarded(T + 1, 0, dev)
    bits = _guarded((T + 1) * B, -1, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    at = lambda buf: buf.data_ptr() + 8 * pad
    for lo, hi in ((0, 77), (77, 78), (78, B)):
        assert lib.mjx_census_mask_ell(g.adj.data_ptr(), n, 4, T, 1, lo, hi, 0, at(cbuf), at(kbuf), flag.data_ptr(),
                                       at(bits), None) == 0
    for lo, hi in ((0, 64), (64, B)):
        assert lib.mjx_census_minima(at(bits), n, T, lo, hi, 0, at(mbuf), at(hbuf), None) == 0
    torch.cuda.synchronize()
    assert int(flag) == 0
    for buf in (cbuf, kbuf, mbuf, hbuf, bits):
        assert bool((buf[:pad] == GUARD).all()) and bool((buf[-pad:] == GUARD).all())
    assert np.array_equal(bits[pad:-pad].cpu().numpy().view(np.uint64).reshape(T + 1, B), cm.words(want["U"], n))
    assert np.array_equal(cbuf[pad:-pad].cpu().numpy().reshape(T + 1, n + 1), want["counts"])
    assert np.array_equal(mbuf[pad:-pad].cpu().numpy().reshape(T + 1, n + 1), want["minima"])
    assert np.array_equal(hbuf[pad:-pad].cpu().numpy(), (want["max_plus"] << 48) | want["heaviest_x"])
    # the first range of pass 2 alone: fewer minima, and all +1 (level 0) lies in the last block
    mbuf2, hbuf2 = _guarded(cells, 0, dev), _guarded(T + 1, 0, dev)
    assert lib.mjx_census_minima(at(bits), n, T, 0, 64, 0, at(mbuf2), at(hbuf2), None) == 0
    torch.cuda.synchronize()
    part = mbuf2[pad:-pad].cpu().numpy().reshape(T + 1, n + 1)
    assert (part <= want["minima"]).all() and part.sum() < want["minima"].sum() and int(hbuf2[pad]) == 0


@pytest.mark.parametrize("name", ["path3", "path7", "rrg_d4_n13", "star"])
def test_the_returned_mask_is_the_oracles_set_bit_for_bit(mjx_mod, name):
    _, _, n, T, want = _case(name)
    res = mjx_mod.census_minima(_graph(mjx_mod, name), T, 1, return_mask=True)
    mask = res.pop("mask")
    _assert_minima(res, want, n, T)
    assert isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.int64
    assert tuple(mask.shape) == (T + 1, 1 << max(n - 6, 0))
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), cm.words(want["U"], n))


# ---- 4. against the product ----------------------------------------------------------------------------
def test_census_keys_heaviest_witness_and_quenches_on_n16(mjx_mod):
    _, arrays, n, T, want = _case("rrg_d4_n16")
    g = mjx_mod.Graph.ell(arrays[0])
    res = mjx_mod.census_minima(g, T, 1, return_mask=True)
    cen = mjx_mod.census(g, T, 1)
    assert sorted(cen) == ["configs", "counts", "entropy", "m_min", "min_plus", "witness"]
    for key in cen:
        assert np.array_equal(res[key], cen[key]), key
    assert res["max_plus"][T] > res["min_plus"][T], "a greedy pass can end above the optimum here"
    for t in range(T + 1):
        w = res["witness_max"][t].astype(np.int64)
        assert (w == 1).sum() == res["max_plus"][t]
        p, c = _pc(t)
        end = w if t == 0 else mjx_mod.s_endstate(g, w, p, c)
        assert int(np.asarray(end).sum()) == n               # all +1 after t steps of the rollout
        fg = mjx_mod.flip_gains(g, w, p, c, gain=False)
        assert bool(fg["consensus"][0]) and int(fg["n_removable"][0]) == 0 and not bool(fg["removable"].any())
        q = mjx_mod.quench(g, w, p, c)
        assert int(q["flipped"][0]) == 0 and np.array_equal(np.asarray(q["conf"]), w)
    # every greedy result is one of the minima: in the bitmap, in the oracle's minimal set, between the bounds
    K = 16
    qr = mjx_mod.quench_restarts(g, np.ones(n, np.int64), T, 1, restarts=K, seed=5, keep_all=True)
    conf = np.asarray(qr["conf"]).reshape(K, n)
    xs = ((conf == 1).astype(np.int64) << np.arange(n)[None, :]).sum(axis=1)
    words = res["mask"][T].cpu().numpy().view(np.uint64)
    assert all((int(words[x >> 6]) >> (x & 63)) & 1 for x in xs.tolist())
    assert want["M"][T][xs].all()
    plus = (conf == 1).sum(axis=1)
    assert (plus >= res["min_plus"][T]).all() and (plus <= res["max_plus"][T]).all()
    assert np.array_equal(np.asarray(qr["mag"]).reshape(K), (2 * plus - n) / n)


# ---- 5. CLI ------------------------------------------------------------------------------------------------
def test_cli_minima_in_a_fresh_process(mjx_mod, tmp_path):
    out = tmp_path / "census.npz"
    run = subprocess.run([sys.executable, "-m", "mjx", "census", "--graph", "rrg", "--n", "14", "--d", "3",
                          "--graph-seed", "3", "--p", "2", "--c", "1", "--minima", "--out", str(out)],
                         capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "minimal consensus sets" in run.stdout
    want = cm.census_minima(co.step_ell(mjx_mod.random_regular_graph(3, 14, seed=3)), 14, 2)
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == ["configs", "counts", "edges", "entropy", "m_max", "m_min", "max_plus", "mean_plus",
                                   "min_plus", "minima", "minima_total", "witness", "witness_max"]
        assert np.array_equal(z["counts"], want["counts"]) and np.array_equal(z["minima"], want["minima"])
        assert np.array_equal(z["max_plus"], want["max_plus"])
        assert np.array_equal(z["witness_max"], want["witness_max"])
        assert np.array_equal(z["minima_total"], want["M"].sum(axis=1))
